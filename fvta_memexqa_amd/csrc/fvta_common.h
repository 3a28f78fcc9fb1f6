// Common device/host helpers for the FVTA gfx950 kernels.
// Everything here is CDNA4-only (wave64, MFMA); there is no other backend.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/fvta_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef short bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned short bf16_t;  // a bf16 value as its raw 16 bits

#define FVTA_WAVE 64
#define FVTA_NEG (-1e30f)  // utils.py:205 VERY_NEGATIVE_NUMBER

// ---- error plumbing (never throw across the C ABI) -------------------------
void fvta_set_error(const char* fmt, ...);

#define FVTA_CHECK_ARG(cond, ...)                 \
  do {                                            \
    if (!(cond)) {                                \
      fvta_set_error(__VA_ARGS__);                \
      return FVTA_ERR_INVALID_ARG;                \
    }                                             \
  } while (0)

#define FVTA_CHECK_LAUNCH(what)                                                   \
  do {                                                                            \
    hipError_t e__ = hipGetLastError();                                           \
    if (e__ != hipSuccess) {                                                      \
      fvta_set_error("%s: launch failed: %s", what, hipGetErrorString(e__));      \
      return FVTA_ERR_LAUNCH;                                                     \
    }                                                                             \
  } while (0)

#define FVTA_CHECK_HIP(expr)                                                      \
  do {                                                                            \
    hipError_t e__ = (expr);                                                      \
    if (e__ != hipSuccess) {                                                      \
      fvta_set_error("%s failed: %s", #expr, hipGetErrorString(e__));             \
      return FVTA_ERR_LAUNCH;                                                     \
    }                                                                             \
  } while (0)

// Diagnostic switches (kernel-skipping ablations, shader-clock stamps, phase masks) exist only in a -DFVTA_DIAG build
// (`make DIAG=1`): a production library must not change its results, or write stamp areas the workspace query did not
// reserve, because of an environment variable.  Switches that choose between equally correct kernels stay plain getenv.
#include <stdlib.h>
static inline int fvta_diag_env(const char* name, int dflt) {
#ifdef FVTA_DIAG
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
#else
  (void)name;
  return dflt;
#endif
}

static inline size_t fvta_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Carve a caller-provided workspace into 256-byte aligned pieces.
struct FvtaCarver {
  char* base;
  size_t off;
  explicit FvtaCarver(void* p) : base((char*)p), off(0) {}
  template <typename T>
  T* take(size_t n) {
    T* r = (T*)(base ? base + off : nullptr);
    off = fvta_align_up(off + n * sizeof(T), 256);
    return r;
  }
};

// > 64 KB of dynamic LDS is opted into per kernel symbol
template <typename K>
static inline void fvta_allow_lds(K kernel, size_t bytes) {
  if (bytes > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

// ---- device math ------------------------------------------------------------
// Gate non-linearities on the hardware transcendental units (v_exp_f32 / v_rcp_f32, ~1 ulp each):
// absolute error ~1e-7 on values in [-1,1], far inside the 1e-4 parity budget, and ~10x fewer VALU
// instructions than the libm forms -- the LSTM gate epilogue runs 5 of these per cell update.
__device__ __forceinline__ float fvta_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float fvta_tanh(float x) {
  const float e = __expf(-2.0f * fabsf(x));  // in (0,1]: no overflow
  return copysignf((1.0f - e) * __builtin_amdgcn_rcpf(1.0f + e), x);
}

// 16-byte load of four floats
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }
// four bf16 (raw bits, two dwords) as four floats: a shift and a mask per dword.  Exact: bf16 is the upper half of an fp32
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x4 bf4_widen(u32x2 u) {
  return f32x4{__uint_as_float(u[0] << 16), __uint_as_float(u[0] & 0xffff0000u), __uint_as_float(u[1] << 16),
               __uint_as_float(u[1] & 0xffff0000u)};
}
// the same four channels from a row held in bf16: one 8-byte load (p 8-byte aligned), widened in registers
__device__ __forceinline__ f32x4 ld4(const bf16_t* p) { return bf4_widen(*reinterpret_cast<const u32x2*>(p)); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// ---- DPP reductions over aligned groups of 16 lanes (one DPP row); every lane ends with the group's result.
// quad_perm xor 1 / xor 2, then row_half_mirror / row_mirror (which pair a lane with the other quad / other half
// once the smaller groups are uniform).  No LDS crossbar (ds_bpermute) round trips, unlike __shfl_xor.
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_HALF_MIRROR = 0x141, DPP_MIRROR = 0x140;
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_f<DPP_XOR1>(v);
  v += dpp_f<DPP_XOR2>(v);
  v += dpp_f<DPP_HALF_MIRROR>(v);
  v += dpp_f<DPP_MIRROR>(v);
  return v;
}
__device__ __forceinline__ float row16_max(float v) {
  v = fmaxf(v, dpp_f<DPP_XOR1>(v));
  v = fmaxf(v, dpp_f<DPP_XOR2>(v));
  v = fmaxf(v, dpp_f<DPP_HALF_MIRROR>(v));
  v = fmaxf(v, dpp_f<DPP_MIRROR>(v));
  return v;
}
// arg-max with first-index tie break
template <int CTRL>
__device__ __forceinline__ void dpp_argmax_step(float& best, int& bestj) {
  const float ob = dpp_f<CTRL>(best);
  const int oj = dpp_i<CTRL>(bestj);
  if (ob > best || (ob == best && oj < bestj)) {
    best = ob;
    bestj = oj;
  }
}
__device__ __forceinline__ void row16_argmax(float& best, int& bestj) {
  dpp_argmax_step<DPP_XOR1>(best, bestj);
  dpp_argmax_step<DPP_XOR2>(best, bestj);
  dpp_argmax_step<DPP_HALF_MIRROR>(best, bestj);
  dpp_argmax_step<DPP_MIRROR>(best, bestj);
}

// dropout keep decision of element idx: splitmix64 of seed + golden * (idx + 1), top 32 bits below keep_prob * 2^32
// (oracle/fvta_fused.py dropout_keep_masks / dropout_keep_flat evaluate the same hash)
__device__ __forceinline__ bool dropout_keep(unsigned long long seed, unsigned long long idx, unsigned long long thr) {
  unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (idx + 1ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (z >> 32) < thr;
}
static inline unsigned long long dropout_thr(float keep_prob) { return (unsigned long long)((double)keep_prob * 4294967296.0); }

// float -> bf16 (round to nearest even), as raw 16-bit
__device__ __forceinline__ unsigned short f2bf(float f) {
  unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);  // keep NaN a NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}
__device__ __forceinline__ float bf2f(unsigned short h) { return __uint_as_float(((unsigned)h) << 16); }

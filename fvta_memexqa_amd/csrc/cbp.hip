// Compact bilinear pooling for gfx950: model_mcb.py:1254-1363 `compact_bilinear_pooling_layer` (sum_pool = False) and,
// fused, the `l2_normalize(sqrt(sign(g) * g))` that follows it (:645).  The reference takes two count sketches through
// complex FFTs of length D; the circular convolution of two count sketches IS the count sketch of the outer product, so
// no FFT is needed (the formulas are those of include/fvta_hip.h):
//   z[r,k] = sum over (i,j) with (h1[i] + h2[j]) mod D = k of  s1[i] s2[j] x[r,i] q[n(r),j]
// One workgroup of 1024 threads owns one row r for a whole call.  Forward, the GATHER form:
//   1. the count sketch of x[r] goes to LDS, TWICE back to back (sk[k] = sk[k + D]), so that (k - h2[j]) mod D becomes
//      the plain index k + D - h2[j] in [1, 2D): no wrap in the inner loop.  The sketch itself is a gather too: a bucket
//      sums its members in ascending i through a CSR of h1 (cbp_csr, rebuilt by every call: the ABI keeps no state);
//   2. thread t owns k = t, t + 1024, ... (KPT of them, in registers) and walks the taps j = 0 .. d2-1 in order:
//      z[k] += s2[j] q[j] * sk[k + D - h2[j]].  Consecutive lanes read consecutive dwords (conflict-free ds_read_b32), the
//      KPT reads of a tap differ by compile-time offsets, the tap's h2 / s2 / q are wave-uniform;
//   3. normalize = 1: |z| summed over the row (wave butterflies, then the 16 wave sums in order), y = sqrt|z| *
//      rsqrt(max(sum, 1e-12)).  z never leaves the registers.
// Backward: with normalize = 1 the row's z is computed again by the same steps (bitwise the forward's), dz follows from
// dy, goes to LDS twice back to back in the sketch's place, and both gradients gather from it at h1[i] + h2[j] < 2D:
//   dx[r,i] = s1[i] sum_j s2[j] q[n,j] dz[h1[i] + h2[j]]          (a thread per i, taps in order)
//   dq'[r,j] =      sum_i s1[i] x[r,i] dz[h1[i] + h2[j]]          (a thread per (j, slice of i), slices folded in order)
// and a second kernel folds dq' over the P rows of n in order: dq[n,j] = s2[j] sum_p dq'[n P + p, j].
// Zero conventions: d sqrt|z| / dz = sign(z) / (2 sqrt|z|) for z != 0 and 0 at z = 0 (TF gives inf / NaN there, and the
// reference's tf.where(is_nan) scrubs only the forward); the whole of dz is 0 at z = 0.  The normalisation's second term,
// -y_k (dy . y) / (2 w_k |w|), is computed as -(dy . y) / (2 |w|^2): y_k / w_k = 1 / |w| exactly, no quotient of two
// rounded numbers.  Below the 1e-12 clamp the norm is a constant and that term is absent.
// No floating-point atomics, fixed summation order everywhere: two runs are bitwise equal.  Exact fp32 on the VALU; the
// contraction is a gather through hashed indices, it has no matrix-pipe form.
#include "fvta_common.h"

namespace fvta {

constexpr int CBP_THREADS = 1024;
constexpr int CBP_WAVES = CBP_THREADS / FVTA_WAVE;
constexpr int CBP_KPT_MAX = 16;
constexpr int CBP_D_MAX = CBP_KPT_MAX * CBP_THREADS;   // 16384: the doubled row and its tail are 128 KB of the CU's 160 KB
constexpr int CBP_SCRATCH = CBP_THREADS + CBP_WAVES;   // floats behind the row: the slice partials of dq, the wave sums
static_assert(((size_t)CBP_KPT_MAX * CBP_THREADS + CBP_D_MAX + CBP_SCRATCH) * 4 <= 160 * 1024, "the row must fit the CU's LDS");

struct CbpArgs {
  int N, P, d1, d2, D;
  const float *x, *q;          // [N P, d1], [N, d2]
  const int *h1, *h2;
  const float *s1, *s2;
  const int *start, *perm;     // CSR of h1: bucket k holds perm[start[k] .. start[k+1]), ascending
  float* out;                  // forward: [N P, D]
  const float* dy;             // backward: [N P, D]
  float *dx, *dqp;             // backward: [N P, d1] (may be NULL), partials [N P, d2] (may be NULL)
  float* rowsum;               // `saved`: the row's sum of |z| [N P] (normalize = 1; NULL in a forward that keeps nothing)
  int accumulate;
};

__device__ __forceinline__ int cbp_bucket(int h, int D) { return h < 0 ? 0 : (h >= D ? D - 1 : h); }

// the sum of v over the workgroup, the same bits in every thread: butterflies inside a wave, the wave sums in order
__device__ __forceinline__ float cbp_block_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int w = 0; w < CBP_WAVES; ++w) s += red[w];
  return s;
}

// ---------------------------------------------------------------- the CSR of h1
// One workgroup.  Dynamic LDS: D counters, then CBP_THREADS scan cells.  Members of a bucket are placed through integer
// atomics (any order) and then sorted by the bucket's thread, so the table does not depend on the schedule.
__global__ __launch_bounds__(CBP_THREADS) void cbp_csr(const int* __restrict__ h1, int d1, int D, int* __restrict__ start,
                                                       int* __restrict__ perm) {
  extern __shared__ __attribute__((aligned(16))) char cbp_smem[];
  int* cnt = reinterpret_cast<int*>(cbp_smem);
  int* cell = cnt + (D + 3) / 4 * 4;
  const int tid = threadIdx.x;
  for (int k = tid; k < D; k += CBP_THREADS) cnt[k] = 0;
  __syncthreads();
  for (int i = tid; i < d1; i += CBP_THREADS) atomicAdd(&cnt[cbp_bucket(h1[i], D)], 1);
  __syncthreads();
  const int C = (D + CBP_THREADS - 1) / CBP_THREADS, lo = tid * C, hi = min(lo + C, D);
  int mine = 0;
  for (int k = lo; k < hi; ++k) mine += cnt[k];
  cell[tid] = mine;
  __syncthreads();
  for (int o = 1; o < CBP_THREADS; o <<= 1) {   // inclusive scan of the chunk sums
    const int v = tid >= o ? cell[tid - o] : 0;
    __syncthreads();
    cell[tid] += v;
    __syncthreads();
  }
  int run = cell[tid] - mine;
  for (int k = lo; k < hi; ++k) {
    const int c = cnt[k];
    start[k] = run;
    cnt[k] = run;                               // the bucket's cursor
    run += c;
  }
  if (tid == 0) start[D] = d1;
  __syncthreads();
  for (int i = tid; i < d1; i += CBP_THREADS) perm[atomicAdd(&cnt[cbp_bucket(h1[i], D)], 1)] = i;
  __threadfence_block();
  __syncthreads();
  for (int k = tid; k < D; k += CBP_THREADS) {  // cnt[k] is now the bucket's end; insertion sort (buckets are short)
    const int b = k ? cnt[k - 1] : 0, e = cnt[k];
    for (int a = b + 1; a < e; ++a) {
      const int v = perm[a];
      int p = a - 1;
      while (p >= b && perm[p] > v) {
        perm[p + 1] = perm[p];
        --p;
      }
      perm[p + 1] = v;
    }
  }
}

// ---------------------------------------------------------------- one row
// the count sketch of x[r], twice back to back, zeros behind it up to the last index a thread can form
template <int KPT>
__device__ __forceinline__ void cbp_sketch(const CbpArgs& a, const float* __restrict__ xr, float* sk) {
  const int D = a.D, tid = threadIdx.x;
  for (int k = tid; k < D; k += CBP_THREADS) {
    float v = 0.f;
    const int e = a.start[k + 1];
    for (int p = a.start[k]; p < e; ++p) {
      const int i = a.perm[p];
      v = fmaf(a.s1[i], xr[i], v);
    }
    sk[k] = v;
    sk[k + D] = v;
  }
  for (int k = 2 * D + tid; k < KPT * CBP_THREADS + D; k += CBP_THREADS) sk[k] = 0.f;
  __syncthreads();
}

// z[m] of k = tid + m * 1024.  For k >= D the reads stay inside the row (its tail is zero) and give a finite number the
// callers leave out.
template <int KPT>
__device__ __forceinline__ void cbp_taps(const CbpArgs& a, const float* __restrict__ qn, const float* sk, float (&z)[KPT]) {
  const int D = a.D, d2 = a.d2;
  const float* base = sk + threadIdx.x + D;
#pragma unroll
  for (int m = 0; m < KPT; ++m) z[m] = 0.f;
  for (int j = 0; j < d2; ++j) {
    const float* p = base - cbp_bucket(a.h2[j], D);
    const float sq = a.s2[j] * qn[j];
#pragma unroll
    for (int m = 0; m < KPT; ++m) z[m] = fmaf(sq, p[m * CBP_THREADS], z[m]);
  }
}

// grid N P.  Dynamic LDS: KPT * 1024 + D floats of row, CBP_SCRATCH floats of scratch.
template <int KPT, bool NORM>
__global__ __launch_bounds__(CBP_THREADS) void cbp_fwd_k(CbpArgs a) {
  extern __shared__ __attribute__((aligned(16))) char cbp_smem[];
  float* sk = reinterpret_cast<float*>(cbp_smem);
  float* red = sk + KPT * CBP_THREADS + a.D + CBP_THREADS;
  const int D = a.D, tid = threadIdx.x;
  const int64_t r = blockIdx.x, n = r / a.P;
  cbp_sketch<KPT>(a, a.x + r * a.d1, sk);
  float z[KPT];
  cbp_taps<KPT>(a, a.q + n * a.d2, sk, z);
  float inv = 1.f;
  if (NORM) {
    float s = 0.f;
#pragma unroll
    for (int m = 0; m < KPT; ++m) s += (tid + m * CBP_THREADS < D) ? fabsf(z[m]) : 0.f;
    const float ss = cbp_block_sum(s, red);
    if (a.rowsum && tid == 0) a.rowsum[r] = ss;
    inv = rsqrtf(fmaxf(ss, 1e-12f));
  }
  float* o = a.out + r * D;
#pragma unroll
  for (int m = 0; m < KPT; ++m) {
    const int k = tid + m * CBP_THREADS;
    if (k < D) o[k] = NORM ? sqrtf(fabsf(z[m])) * inv : z[m];
  }
}

// grid N P, the forward's LDS.
template <int KPT, bool NORM>
__global__ __launch_bounds__(CBP_THREADS) void cbp_bwd_k(CbpArgs a) {
  extern __shared__ __attribute__((aligned(16))) char cbp_smem[];
  float* dzl = reinterpret_cast<float*>(cbp_smem);
  float* part = dzl + KPT * CBP_THREADS + a.D;
  float* red = part + CBP_THREADS;
  const int D = a.D, d1 = a.d1, d2 = a.d2, tid = threadIdx.x;
  const int64_t r = blockIdx.x, n = r / a.P;
  const float* xr = a.x + r * d1;
  const float* qn = a.q + n * d2;
  const float* dyr = a.dy + r * D;
  float dz[KPT];
  if (NORM) {
    cbp_sketch<KPT>(a, xr, dzl);
    float z[KPT];
    cbp_taps<KPT>(a, qn, dzl, z);
    const float ss = a.rowsum[r];                                // the forward's own sum of |z|
    const float inv = rsqrtf(fmaxf(ss, 1e-12f));
    float w[KPT], dyv[KPT], c = 0.f;
#pragma unroll
    for (int m = 0; m < KPT; ++m) {
      const int k = tid + m * CBP_THREADS;
      w[m] = sqrtf(fabsf(z[m]));
      dyv[m] = k < D ? dyr[k] : 0.f;
      c = fmaf(dyv[m], w[m] * inv, c);
    }
    c = ss >= 1e-12f ? cbp_block_sum(c, red) : 0.f;   // (ss is uniform: every thread takes the same side)
    const float tail = 0.5f * c * inv * inv;
#pragma unroll
    for (int m = 0; m < KPT; ++m) {
      const float g = dyv[m] * (0.5f * inv / w[m]) - tail;       // (inf or NaN at w = 0: replaced below)
      dz[m] = z[m] > 0.f ? g : (z[m] < 0.f ? -g : 0.f);
    }
    __syncthreads();                                             // every thread is done with the sketch
  } else {
#pragma unroll
    for (int m = 0; m < KPT; ++m) {
      const int k = tid + m * CBP_THREADS;
      dz[m] = k < D ? dyr[k] : 0.f;
    }
  }
#pragma unroll
  for (int m = 0; m < KPT; ++m) {
    const int k = tid + m * CBP_THREADS;
    if (k < D) {
      dzl[k] = dz[m];
      dzl[k + D] = dz[m];
    }
  }
  __syncthreads();
  if (a.dx) {
    float* dxr = a.dx + r * d1;
    for (int i = tid; i < d1; i += CBP_THREADS) {
      const float* p = dzl + cbp_bucket(a.h1[i], D);
      float acc = 0.f;
      for (int j = 0; j < d2; ++j) acc = fmaf(a.s2[j] * qn[j], p[cbp_bucket(a.h2[j], D)], acc);
      const float v = a.s1[i] * acc;
      dxr[i] = a.accumulate ? dxr[i] + v : v;
    }
  }
  if (a.dqp) {
    float* dqr = a.dqp + r * d2;
    const int S = d2 < CBP_THREADS ? CBP_THREADS / d2 : 1;       // slices of i; S > 1 means d2 * S <= 1024: one pass
    for (int job = tid; job < d2 * S; job += CBP_THREADS) {
      const int sl = job / d2, j = job - sl * d2;
      const float* p = dzl + cbp_bucket(a.h2[j], D);
      float acc = 0.f;
      for (int i = sl; i < d1; i += S) acc = fmaf(a.s1[i] * xr[i], p[cbp_bucket(a.h1[i], D)], acc);
      if (S == 1) dqr[j] = acc;
      else part[job] = acc;
    }
    if (S > 1) {
      __syncthreads();
      if (tid < d2) {
        float acc = 0.f;
        for (int sl = 0; sl < S; ++sl) acc += part[sl * d2 + tid];
        dqr[tid] = acc;
      }
    }
  }
}

// dq[n,j] = s2[j] * (dq'[n P, j] + dq'[n P + 1, j] + ...), in this order
__global__ __launch_bounds__(256) void cbp_dq_fold(const float* __restrict__ dqp, const float* __restrict__ s2,
                                                   float* __restrict__ dq, int N, int P, int d2, int accumulate) {
  const int64_t total = (int64_t)N * d2;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t n = e / d2;
    const int j = (int)(e - n * d2);
    const float* src = dqp + n * P * d2 + j;
    float acc = 0.f;
    for (int p = 0; p < P; ++p) acc += src[(int64_t)p * d2];
    const float v = s2[j] * acc;
    dq[e] = accumulate ? dq[e] + v : v;
  }
}

static inline int cbp_kpt(int D) { return D <= CBP_THREADS ? 1 : (D <= 4 * CBP_THREADS ? 4 : CBP_KPT_MAX); }
static inline size_t cbp_lds_bytes(int D) { return ((size_t)cbp_kpt(D) * CBP_THREADS + D + CBP_SCRATCH) * sizeof(float); }

struct CbpWork {   // the CSR of h1; backward: the per-row partials of dq
  int *start, *perm;
  float* dqp;
  size_t bytes;
  CbpWork(const fvta_cbp_desc& d, int backward, void* p) {
    FvtaCarver c(p);
    start = c.take<int>((size_t)d.D + 1);
    perm = c.take<int>((size_t)d.d1);
    dqp = backward ? c.take<float>((size_t)d.N * d.P * d.d2) : nullptr;
    bytes = c.off;
  }
};

// 0: fine, FVTA_ERR_INVALID_ARG / FVTA_ERR_UNSUPPORTED with the message set otherwise
static int cbp_desc_check(const fvta_cbp_desc* d, const char* who) {
  if (!d || d->N <= 0 || d->P <= 0 || d->d1 <= 0 || d->d2 <= 0 || d->D <= 0 || (d->normalize != 0 && d->normalize != 1) ||
      (int64_t)d->N * d->P > 0x7fffffff) {
    fvta_set_error("%s: bad N/P/d1/d2/D/normalize", who);
    return FVTA_ERR_INVALID_ARG;
  }
  if (d->D > CBP_D_MAX) {
    fvta_set_error("%s: unsupported D = %d: a row of the output lives in one workgroup's LDS, the limit is D <= %d", who, d->D,
                   CBP_D_MAX);
    return FVTA_ERR_UNSUPPORTED;
  }
  return FVTA_OK;
}

template <int KPT>
static void cbp_launch_fwd(const CbpArgs& a, bool norm, size_t lds, hipStream_t s) {
  const dim3 grid((unsigned)((int64_t)a.N * a.P));
  if (norm) {
    fvta_allow_lds(cbp_fwd_k<KPT, true>, lds);
    hipLaunchKernelGGL((cbp_fwd_k<KPT, true>), grid, dim3(CBP_THREADS), lds, s, a);
  } else {
    fvta_allow_lds(cbp_fwd_k<KPT, false>, lds);
    hipLaunchKernelGGL((cbp_fwd_k<KPT, false>), grid, dim3(CBP_THREADS), lds, s, a);
  }
}
template <int KPT>
static void cbp_launch_bwd(const CbpArgs& a, bool norm, size_t lds, hipStream_t s) {
  const dim3 grid((unsigned)((int64_t)a.N * a.P));
  if (norm) {
    fvta_allow_lds(cbp_bwd_k<KPT, true>, lds);
    hipLaunchKernelGGL((cbp_bwd_k<KPT, true>), grid, dim3(CBP_THREADS), lds, s, a);
  } else {
    fvta_allow_lds(cbp_bwd_k<KPT, false>, lds);
    hipLaunchKernelGGL((cbp_bwd_k<KPT, false>), grid, dim3(CBP_THREADS), lds, s, a);
  }
}

static void cbp_launch_csr(const fvta_cbp_desc& d, const int* h1, const CbpWork& w, hipStream_t s) {
  const size_t lds = ((size_t)(d.D + 3) / 4 * 4 + CBP_THREADS) * sizeof(int);
  fvta_allow_lds(cbp_csr, lds);
  hipLaunchKernelGGL(cbp_csr, dim3(1), dim3(CBP_THREADS), lds, s, h1, d.d1, d.D, w.start, w.perm);
}

}  // namespace fvta
using namespace fvta;

#define CBP_DISPATCH(kpt, CALL)   \
  switch (kpt) {                  \
    case 1: CALL(1); break;       \
    case 4: CALL(4); break;       \
    default: CALL(16); break;     \
  }

extern "C" size_t fvta_cbp_saved_bytes(const fvta_cbp_desc* d) {
  if (cbp_desc_check(d, "cbp_saved_bytes") != FVTA_OK) return 0;
  // the backward computes a row's z again from x and q (the forward does not write it), so what is kept is one word per
  // row, the row's sum of |z|; without the normalisation the backward needs x, q and dy only
  return (d->training && d->normalize) ? fvta_align_up((size_t)d->N * d->P * sizeof(float), 256) : 0;
}

extern "C" size_t fvta_cbp_workspace_bytes(const fvta_cbp_desc* d, int32_t backward) {
  if (cbp_desc_check(d, "cbp_workspace_bytes") != FVTA_OK) return 0;
  return CbpWork(*d, backward, nullptr).bytes;
}

extern "C" int fvta_cbp_fwd(const fvta_cbp_desc* d, const float* x, const float* q, const int32_t* h1, const float* s1,
                            const int32_t* h2, const float* s2, float* out, void* saved, void* workspace,
                            fvta_stream_t stream_) {
  const int st = cbp_desc_check(d, "cbp_fwd");
  if (st != FVTA_OK) return st;
  FVTA_CHECK_ARG(x && q && h1 && s1 && h2 && s2 && out && workspace, "cbp_fwd: null pointer");
  const bool keep = d->training && d->normalize;
  FVTA_CHECK_ARG(!keep || saved, "cbp_fwd: training with normalize = 1 wants `saved`");
  hipStream_t s = (hipStream_t)stream_;
  CbpWork w(*d, 0, workspace);
  cbp_launch_csr(*d, h1, w, s);
  CbpArgs a{d->N, d->P, d->d1, d->d2, d->D, x, q, h1, h2, s1, s2, w.start, w.perm, out, nullptr, nullptr, nullptr,
            keep ? (float*)saved : nullptr, 0};
  const size_t lds = cbp_lds_bytes(d->D);
  const bool norm = d->normalize != 0;
#define CBP_CALL(KPT) cbp_launch_fwd<KPT>(a, norm, lds, s)
  CBP_DISPATCH(cbp_kpt(d->D), CBP_CALL)
#undef CBP_CALL
  FVTA_CHECK_LAUNCH("cbp_fwd");
  return FVTA_OK;
}

extern "C" int fvta_cbp_bwd(const fvta_cbp_desc* d, const float* x, const float* q, const int32_t* h1, const float* s1,
                            const int32_t* h2, const float* s2, const void* saved, const float* dy, float* dx, float* dq,
                            int32_t accumulate, void* workspace, fvta_stream_t stream_) {
  const int st = cbp_desc_check(d, "cbp_bwd");
  if (st != FVTA_OK) return st;
  FVTA_CHECK_ARG(d->training, "cbp_bwd: the forward ran with training = 0");
  FVTA_CHECK_ARG(x && q && h1 && s1 && h2 && s2 && dy && workspace, "cbp_bwd: null pointer");
  FVTA_CHECK_ARG(dx || dq, "cbp_bwd: dx and dq are both NULL");
  FVTA_CHECK_ARG(!d->normalize || saved, "cbp_bwd: normalize = 1 wants the forward's `saved`");
  hipStream_t s = (hipStream_t)stream_;
  CbpWork w(*d, 1, workspace);
  const bool norm = d->normalize != 0;
  if (norm) cbp_launch_csr(*d, h1, w, s);
  CbpArgs a{d->N, d->P, d->d1, d->d2, d->D, x, q, h1, h2, s1, s2, w.start, w.perm, nullptr, dy, dx, dq ? w.dqp : nullptr,
            (float*)const_cast<void*>(saved), accumulate != 0};
  const size_t lds = cbp_lds_bytes(d->D);
#define CBP_CALL(KPT) cbp_launch_bwd<KPT>(a, norm, lds, s)
  CBP_DISPATCH(cbp_kpt(d->D), CBP_CALL)
#undef CBP_CALL
  if (dq) {
    const int64_t total = (int64_t)d->N * d->d2;
    const unsigned blocks = (unsigned)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024);
    hipLaunchKernelGGL(cbp_dq_fold, dim3(blocks), dim3(256), 0, s, w.dqp, s2, dq, d->N, d->P, d->d2, accumulate != 0);
  }
  FVTA_CHECK_LAUNCH("cbp_bwd");
  return FVTA_OK;
}

// Context tensor (include/fvta_hip.h "Context tensor"; model_v2.py:863-914): K encoder outputs [N,M,J_k,w] padded to
// JMAX rows and stacked into hall [N,K,M,JMAX,w] (with the masks into hall_mask [N,K,M,JMAX]), and the slice back that is
// its gradient.  Pure data movement: one launch each way, every output element stored exactly once, nothing read back.
//
// Work split.  For one (n,k,m) the JMAX*w floats of hall are contiguous and so are the J_k*w floats of the stream they
// come from, so the copy is "the first J_k*w elements of a slab, then zeros".  blockIdx.x = the slab (n K + k) M + m
// (decomposed once per workgroup, on the scalar unit), blockIdx.y strides over the slab: no per-element division.  The
// K stream pointers and lengths travel in the kernel argument itself; `k` is uniform, so picking one is a scalar select.
//
// Byte model (memory bound, no reuse): 4 w (sum_k N M J_k  read  +  N K M JMAX  written) + the same without the 4 w for
// the masks.  16-byte loads / stores when w % 4 == 0 and every pointer is 16-byte aligned (every slab then starts on a
// 16-byte boundary), 4-byte ones otherwise.  All element offsets are 64-bit: BASELINE.json configs[4] has 3.3 G elements.
#include "fvta_common.h"

static_assert(sizeof(fvta_context_desc) == 4 * (4 + FVTA_CTX_KMAX), "fvta_context_desc: twelve int32, no padding");

namespace fvta {
constexpr int CTX_THREADS = 256;          // 4 waves; a handful of registers, so 8 workgroups fit a CU
constexpr int CTX_TARGET_BLOCKS = 4096;   // 256 CUs x 16: two rounds of full occupancy, the rest is strided

struct CtxArgs {
  const void* src[FVTA_CTX_KMAX];   // fwd: streams[k]; bwd: unused
  void* dst[FVTA_CTX_KMAX];         // bwd: d_streams[k] (NULL = skipped); fwd: unused
  const uint8_t* msk[FVTA_CTX_KMAX];
  int32_t J[FVTA_CTX_KMAX];
  void* hall;                       // fwd: written; bwd: d_hall, read
  uint8_t* hall_mask;               // NULL: no mask
  int32_t K, M, JMAX, w;
};

// pick entry k of a kernel-argument array with a chain of uniform selects (a dynamic index could send the array to scratch)
template <typename T>
__device__ __forceinline__ T ctx_pick(const T (&a)[FVTA_CTX_KMAX], int k) {
  T r = a[0];
#pragma unroll
  for (int i = 1; i < FVTA_CTX_KMAX; ++i) r = (k == i) ? a[i] : r;
  return r;
}

// V = f32x4 (wv = w / 4) or float (wv = w)
template <typename V>
__global__ __launch_bounds__(CTX_THREADS) void context_fwd_kernel(const CtxArgs a, const int64_t wv) {
  const int64_t slab = blockIdx.x;                  // (n K + k) M + m
  const int m = (int)(slab % a.M);
  const int64_t nk = slab / a.M;
  const int k = (int)(nk % a.K);
  const int64_t n = nk / a.K;
  const int64_t Jk = ctx_pick(a.J, k);
  const int64_t row0 = (n * a.M + m) * Jk;          // first row of this slab in stream k
  const int64_t nsrc = Jk * wv, nall = (int64_t)a.JMAX * wv;
  const V* __restrict__ src = (const V*)ctx_pick(a.src, k) + row0 * wv;
  V* __restrict__ dst = (V*)a.hall + slab * nall;
  const int64_t stride = (int64_t)gridDim.y * CTX_THREADS;
  const int64_t first = (int64_t)blockIdx.y * CTX_THREADS + threadIdx.x;
  V zero;
  __builtin_memset(&zero, 0, sizeof(V));
#pragma unroll 4
  for (int64_t i = first; i < nall; i += stride) dst[i] = i < nsrc ? src[i] : zero;
  if (a.hall_mask) {
    const uint8_t* __restrict__ ms = ctx_pick(a.msk, k) + row0;
    uint8_t* __restrict__ md = a.hall_mask + slab * a.JMAX;
    for (int64_t j = first; j < a.JMAX; j += stride) md[j] = j < Jk ? ms[j] : (uint8_t)0;
  }
}

template <typename V>
__global__ __launch_bounds__(CTX_THREADS) void context_bwd_kernel(const CtxArgs a, const int64_t wv) {
  const int64_t slab = blockIdx.x;
  const int m = (int)(slab % a.M);
  const int64_t nk = slab / a.M;
  const int k = (int)(nk % a.K);
  const int64_t n = nk / a.K;
  V* __restrict__ dst = (V*)ctx_pick(a.dst, k);
  if (!dst) return;                                 // (uniform) this stream wants no gradient
  const int64_t Jk = ctx_pick(a.J, k);
  const int64_t nsrc = Jk * wv;
  dst += (n * a.M + m) * nsrc;
  const V* __restrict__ src = (const V*)a.hall + slab * ((int64_t)a.JMAX * wv);
  const int64_t stride = (int64_t)gridDim.y * CTX_THREADS;
#pragma unroll 4
  for (int64_t i = (int64_t)blockIdx.y * CTX_THREADS + threadIdx.x; i < nsrc; i += stride) dst[i] = src[i];
}

static inline bool ctx_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// descriptor checks shared by both directions; returns JMAX (> 0) or 0 with the message set
static int ctx_check_desc(const char* what, const fvta_context_desc* d) {
  if (!d) {
    fvta_set_error("%s: null descriptor", what);
    return 0;
  }
  if (d->K < 1 || d->K > FVTA_CTX_KMAX) {
    fvta_set_error("%s: K must be in 1..%d (got %d)", what, FVTA_CTX_KMAX, d->K);
    return 0;
  }
  if (d->N < 1 || d->M < 1 || d->w < 1) {
    fvta_set_error("%s: N, M, w must be >= 1 (got N %d, M %d, w %d)", what, d->N, d->M, d->w);
    return 0;
  }
  int jmax = 0;
  for (int k = 0; k < d->K; ++k) {
    if (d->J[k] < 1) {
      fvta_set_error("%s: J[%d] must be >= 1 (got %d)", what, k, d->J[k]);
      return 0;
    }
    jmax = d->J[k] > jmax ? d->J[k] : jmax;
  }
  if ((int64_t)d->N * d->K * d->M > 2147483647ll) {
    fvta_set_error("%s: N * K * M must stay below 2^31 (got %lld)", what, (long long)d->N * d->K * d->M);
    return 0;
  }
  return jmax;
}

// blockIdx.y extent: enough workgroups per slab to reach CTX_TARGET_BLOCKS in all, never more than the slab has work for
static inline unsigned ctx_grid_y(int64_t slabs, int64_t per_slab) {
  int64_t need = (per_slab + CTX_THREADS - 1) / CTX_THREADS;
  int64_t want = (CTX_TARGET_BLOCKS + slabs - 1) / slabs;
  int64_t gy = need < want ? need : want;
  return (unsigned)(gy < 1 ? 1 : (gy > 65535 ? 65535 : gy));
}
}  // namespace fvta

extern "C" int fvta_context_fwd(const fvta_context_desc* d, const float* const* streams, const uint8_t* const* masks,
                                float* hall, uint8_t* hall_mask, fvta_stream_t stream) {
  const int JMAX = fvta::ctx_check_desc("context_fwd", d);
  if (!JMAX) return FVTA_ERR_INVALID_ARG;
  FVTA_CHECK_ARG(streams && hall, "context_fwd: null pointer (streams %p hall %p)", (const void*)streams, (void*)hall);
  FVTA_CHECK_ARG((masks == nullptr) == (hall_mask == nullptr),
                 "context_fwd: masks and hall_mask go together (masks %p hall_mask %p)", (const void*)masks,
                 (void*)hall_mask);
  fvta::CtxArgs a = {};
  bool vec = d->w % 4 == 0 && fvta::ctx_al16(hall);
  for (int k = 0; k < d->K; ++k) {
    FVTA_CHECK_ARG(streams[k], "context_fwd: streams[%d] is null", k);
    FVTA_CHECK_ARG(!masks || masks[k], "context_fwd: masks[%d] is null", k);
    FVTA_CHECK_ARG(((uintptr_t)streams[k] & 3) == 0, "context_fwd: streams[%d] needs 4-byte alignment", k);
    a.src[k] = streams[k];
    a.msk[k] = masks ? masks[k] : nullptr;
    a.J[k] = d->J[k];
    vec = vec && fvta::ctx_al16(streams[k]);
  }
  FVTA_CHECK_ARG(((uintptr_t)hall & 3) == 0, "context_fwd: hall needs 4-byte alignment");
  a.hall = hall;
  a.hall_mask = hall_mask;
  a.K = d->K;
  a.M = d->M;
  a.JMAX = JMAX;
  a.w = d->w;
  const int64_t slabs = (int64_t)d->N * d->K * d->M;
  const int64_t wv = vec ? d->w / 4 : d->w;
  const dim3 grid((unsigned)slabs, fvta::ctx_grid_y(slabs, (int64_t)JMAX * wv));
  if (vec)
    hipLaunchKernelGGL(fvta::context_fwd_kernel<f32x4>, grid, dim3(fvta::CTX_THREADS), 0, (hipStream_t)stream, a, wv);
  else
    hipLaunchKernelGGL(fvta::context_fwd_kernel<float>, grid, dim3(fvta::CTX_THREADS), 0, (hipStream_t)stream, a, wv);
  FVTA_CHECK_LAUNCH("context_fwd");
  return FVTA_OK;
}

extern "C" int fvta_context_bwd(const fvta_context_desc* d, const float* d_hall, float* const* d_streams,
                                fvta_stream_t stream) {
  const int JMAX = fvta::ctx_check_desc("context_bwd", d);
  if (!JMAX) return FVTA_ERR_INVALID_ARG;
  FVTA_CHECK_ARG(d_hall && d_streams, "context_bwd: null pointer (d_hall %p d_streams %p)", (const void*)d_hall,
                 (const void*)d_streams);
  FVTA_CHECK_ARG(((uintptr_t)d_hall & 3) == 0, "context_bwd: d_hall needs 4-byte alignment");
  fvta::CtxArgs a = {};
  bool vec = d->w % 4 == 0 && fvta::ctx_al16(d_hall), any = false;
  int jwant = 0;
  for (int k = 0; k < d->K; ++k) {
    FVTA_CHECK_ARG(((uintptr_t)d_streams[k] & 3) == 0, "context_bwd: d_streams[%d] needs 4-byte alignment", k);
    a.dst[k] = d_streams[k];
    a.J[k] = d->J[k];
    if (d_streams[k]) {
      any = true;
      vec = vec && fvta::ctx_al16(d_streams[k]);
      jwant = d->J[k] > jwant ? d->J[k] : jwant;
    }
  }
  if (!any) return FVTA_OK;   // every entry skipped: nothing to write
  a.hall = const_cast<float*>(d_hall);
  a.K = d->K;
  a.M = d->M;
  a.JMAX = JMAX;
  a.w = d->w;
  const int64_t slabs = (int64_t)d->N * d->K * d->M;
  const int64_t wv = vec ? d->w / 4 : d->w;
  const dim3 grid((unsigned)slabs, fvta::ctx_grid_y(slabs, (int64_t)jwant * wv));
  if (vec)
    hipLaunchKernelGGL(fvta::context_bwd_kernel<f32x4>, grid, dim3(fvta::CTX_THREADS), 0, (hipStream_t)stream, a, wv);
  else
    hipLaunchKernelGGL(fvta::context_bwd_kernel<float>, grid, dim3(fvta::CTX_THREADS), 0, (hipStream_t)stream, a, wv);
  FVTA_CHECK_LAUNCH("context_bwd");
  return FVTA_OK;
}

// Gradient guard (include/fvta_hip.h "Gradient guard"): statistics of the scaled, value-clipped flat gradient in one
// streaming read, then one workgroup that combines them and writes the device-resident control block the guarded
// optimiser steps (optim.hip) read.  Nothing here synchronises with the host.
//
// Summation order.  A lane adds the squares of its elements in fp32 (at most n / (grid * 256) of them, 4 per trip), the
// lanes of a workgroup are added in double through a fixed shuffle tree, each workgroup stores its partial with a plain
// store, and the finalise workgroup adds the partials in double in index order.  The grid is gg_grid(n): neither the
// layout of the partials nor the order of any addition depends on the device or on which workgroup finishes first, so
// every rank of a data-parallel run, holding the same reduced buffer, takes the same decision bit for bit.
#include <math.h>

#include "fvta_common.h"

namespace fvta {
constexpr int GG_THREADS = 256;       // 4 waves; the kernel needs few registers, so 8 such workgroups fit a CU
constexpr int GG_MAX_BLOCKS = 2048;   // 256 CUs x 8: every wave slot busy, the rest of n is grid-strided
constexpr int GG_WAVES = GG_THREADS / FVTA_WAVE;

static inline int gg_grid(int64_t n) {
  const int64_t b = (n + GG_THREADS * 4 - 1) / (GG_THREADS * 4);
  return (int)(b < 1 ? 1 : (b > GG_MAX_BLOCKS ? GG_MAX_BLOCKS : b));
}

// partials: [grid] double sum of squares | [grid] int64 non-finite count | [grid] float largest finite |g''|
struct GGParts {
  double* ss;
  long long* nf;
  float* mx;
};
static inline size_t gg_carve(void* ws, int grid, GGParts* p) {
  FvtaCarver c(ws);
  p->ss = c.take<double>(grid);
  p->nf = c.take<long long>(grid);
  p->mx = c.take<float>(grid);
  return c.off;
}

__device__ __forceinline__ void gg_take(float x, float gscale, float c, float& ss, float& mx, unsigned& nf) {
  nf += (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;   // NaN or +-inf in the RAW buffer
  float g = x * gscale;
  if (c > 0.f) g = g < -c ? -c : (g > c ? c : g);            // comparisons, not fminf/fmaxf: a NaN stays a NaN
  ss += g * g;
  const float a = fabsf(g);
  mx = (a < INFINITY && a > mx) ? a : mx;                    // false for NaN and inf
}

__global__ __launch_bounds__(GG_THREADS) void grad_stats_kernel(const float* __restrict__ grad, int64_t n, float gscale,
                                                                float clipv, double* __restrict__ p_ss,
                                                                long long* __restrict__ p_nf, float* __restrict__ p_mx) {
  // head: the 0..3 elements before the first 16-byte boundary; body: 16-byte loads; tail: the 0..3 elements left
  int64_t head = (int64_t)(((16u - (unsigned)((uintptr_t)grad & 15u)) & 15u) >> 2);
  if (head > n) head = n;
  const f32x4* __restrict__ body = (const f32x4*)(grad + head);
  const int64_t nv = (n - head) >> 2;
  const int64_t tail0 = head + (nv << 2);
  float ss = 0.f, mx = 0.f;
  unsigned nf = 0;
  const int64_t stride = (int64_t)gridDim.x * GG_THREADS;
  for (int64_t i = (int64_t)blockIdx.x * GG_THREADS + threadIdx.x; i < nv; i += stride) {
    const f32x4 v = body[i];
    gg_take(v[0], gscale, clipv, ss, mx, nf);
    gg_take(v[1], gscale, clipv, ss, mx, nf);
    gg_take(v[2], gscale, clipv, ss, mx, nf);
    gg_take(v[3], gscale, clipv, ss, mx, nf);
  }
  if (blockIdx.x == 0 && threadIdx.x < 3) {
    const int64_t t = threadIdx.x;
    if (t < head) gg_take(grad[t], gscale, clipv, ss, mx, nf);
    if (tail0 + t < n) gg_take(grad[tail0 + t], gscale, clipv, ss, mx, nf);
  }
  double dss = (double)ss;
  long long dnf = (long long)nf;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    dss += __shfl_xor(dss, o, 64);
    dnf += __shfl_xor(dnf, o, 64);
    const float om = __shfl_xor(mx, o, 64);
    mx = om > mx ? om : mx;
  }
  __shared__ double s_ss[GG_WAVES];
  __shared__ long long s_nf[GG_WAVES];
  __shared__ float s_mx[GG_WAVES];
  const int wave = threadIdx.x / FVTA_WAVE;
  if ((threadIdx.x & (FVTA_WAVE - 1)) == 0) {
    s_ss[wave] = dss;
    s_nf[wave] = dnf;
    s_mx[wave] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < GG_WAVES; ++w) {
      dss += s_ss[w];
      dnf += s_nf[w];
      mx = s_mx[w] > mx ? s_mx[w] : mx;
    }
    p_ss[blockIdx.x] = dss;
    p_nf[blockIdx.x] = dnf;
    p_mx[blockIdx.x] = mx;
  }
}

// one workgroup: partials in index order (thread t takes t, t + 256, ...), then a fixed tree; thread 0 writes the block
__global__ __launch_bounds__(GG_THREADS) void grad_finalise_kernel(const double* __restrict__ p_ss,
                                                                   const long long* __restrict__ p_nf,
                                                                   const float* __restrict__ p_mx, int grid,
                                                                   fvta_guard_desc d, fvta_guard_ctl* __restrict__ ctl) {
  __shared__ double s_ss[GG_THREADS];
  __shared__ long long s_nf[GG_THREADS];
  __shared__ float s_mx[GG_THREADS];
  double ss = 0.0;
  long long nf = 0;
  float mx = 0.f;
  for (int b = threadIdx.x; b < grid; b += GG_THREADS) {
    ss += p_ss[b];
    nf += p_nf[b];
    mx = p_mx[b] > mx ? p_mx[b] : mx;
  }
  s_ss[threadIdx.x] = ss;
  s_nf[threadIdx.x] = nf;
  s_mx[threadIdx.x] = mx;
  __syncthreads();
  for (int st = GG_THREADS / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) {
      s_ss[threadIdx.x] += s_ss[threadIdx.x + st];
      s_nf[threadIdx.x] += s_nf[threadIdx.x + st];
      const float om = s_mx[threadIdx.x + st];
      if (om > s_mx[threadIdx.x]) s_mx[threadIdx.x] = om;
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const double norm = sqrt(s_ss[0]);
  const long long nonfinite = s_nf[0];
  float factor = 1.f;
  if (d.clip_norm > 0.f) {
    const float nrm = (float)norm;
    factor = d.clip_norm / (nrm > d.clip_norm ? nrm : d.clip_norm);   // exactly 1.0f up to the threshold
  }
  const bool finite = norm <= 1.7976931348623157e308;                 // false for NaN and inf
  const int apply = !(d.skip_nonfinite && (nonfinite > 0 || !finite));
  long long applied = ctl->applied, skipped = ctl->skipped;
  float lr_t = 0.f;
  if (d.adam) {   // fvta_adam_step's formula with t = the number of applied steps including this one
    const double t = (double)(applied + 1);
    lr_t = (float)((double)d.lr * sqrt(1.0 - pow((double)d.beta2, t)) / (1.0 - pow((double)d.beta1, t)));
  }
  if (apply) ++applied; else ++skipped;
  ctl->grad_scale = d.grad_scale;
  ctl->clip_value = d.clip_value;
  ctl->factor = factor;
  ctl->lr_t = lr_t;
  ctl->apply = apply;
  ctl->maxabs = s_mx[0];
  ctl->norm = norm;
  ctl->nonfinite = nonfinite;
  ctl->applied = applied;
  ctl->skipped = skipped;
}
}  // namespace fvta

extern "C" size_t fvta_grad_guard_workspace_bytes(int64_t n) {
  if (n <= 0) {
    fvta_set_error("grad_guard_workspace_bytes: n must be positive (got %lld)", (long long)n);
    return 0;
  }
  fvta::GGParts p;
  return fvta::gg_carve(nullptr, fvta::gg_grid(n), &p);
}

extern "C" int fvta_grad_guard(const fvta_guard_desc* d, const float* grad, int64_t n, void* workspace,
                               fvta_guard_ctl* ctl, fvta_stream_t stream) {
  FVTA_CHECK_ARG(d && grad && workspace && ctl, "grad_guard: null pointer (desc %p grad %p workspace %p ctl %p)",
                 (const void*)d, (const void*)grad, workspace, (void*)ctl);
  FVTA_CHECK_ARG(n > 0, "grad_guard: n must be positive (got %lld)", (long long)n);
  FVTA_CHECK_ARG(((uintptr_t)grad & 3) == 0 && ((uintptr_t)ctl & 7) == 0 && ((uintptr_t)workspace & 7) == 0,
                 "grad_guard: grad needs 4-byte, workspace and ctl 8-byte alignment");
  // !(x >= 0) is true for a NaN as well
  FVTA_CHECK_ARG(d->clip_value >= 0.f && d->clip_value <= 3.4028235e38f,
                 "grad_guard: clip_value must be a finite number >= 0 (0 = off), got %g", (double)d->clip_value);
  FVTA_CHECK_ARG(d->clip_norm >= 0.f && d->clip_norm <= 3.4028235e38f,
                 "grad_guard: clip_norm must be a finite number >= 0 (0 = off), got %g", (double)d->clip_norm);
  FVTA_CHECK_ARG(d->grad_scale == d->grad_scale, "grad_guard: grad_scale is NaN");
  FVTA_CHECK_ARG(d->skip_nonfinite == 0 || d->skip_nonfinite == 1, "grad_guard: skip_nonfinite must be 0 or 1");
  FVTA_CHECK_ARG(d->adam == 0 || (d->adam == 1 && d->beta1 >= 0.f && d->beta1 < 1.f && d->beta2 >= 0.f && d->beta2 < 1.f &&
                                  d->lr == d->lr),
                 "grad_guard: adam must be 0 or 1, and with 1 beta1, beta2 in [0, 1) and lr a number");
  const int grid = fvta::gg_grid(n);
  fvta::GGParts p;
  fvta::gg_carve(workspace, grid, &p);
  hipLaunchKernelGGL(fvta::grad_stats_kernel, dim3(grid), dim3(fvta::GG_THREADS), 0, (hipStream_t)stream, grad, n,
                     d->grad_scale, d->clip_value, p.ss, p.nf, p.mx);
  FVTA_CHECK_LAUNCH("grad_stats");
  hipLaunchKernelGGL(fvta::grad_finalise_kernel, dim3(1), dim3(fvta::GG_THREADS), 0, (hipStream_t)stream, p.ss, p.nf,
                     p.mx, grid, *d, ctl);
  FVTA_CHECK_LAUNCH("grad_finalise");
  return FVTA_OK;
}

// Focal attention forward for MANY QUESTIONS OVER ONE ALBUM (fvta_attn_shared_fwd): hinfo [A,K,T,w] holds each album's
// context rows once, question i reads album[i]'s.  Per question the result is fvta_attn_fwd's on the pair
// (hinfo[album[i]], hq[i]) -- model_v2.py:210-298 -- but a row is fetched once per GROUP of up to G questions of the same
// album instead of once per question, and the logits of a group are one [rows, w] x [w, G JP] product on the fp32 matrix
// pipe (gemm_f32.h: v_mfma_f32_32x32x2_f32, exact fp32).  No shadow rows; the time warp: fvta_attn_shared_fwd_tw, the TW
// instantiations of (4) and (6), further down.  fvta_attn_shared_fwd keeps nothing
// for a backward; fvta_attn_shared_fwd_train runs the same kernels -- the same bits -- with the ordered plan (3) and the
// arg-max (4) compiled in, and leaves what attn_shared_bwd.hip reads in the caller-held `saved` (attn_shared_common.h).
// fvta_attn_shared_fwd_tw_train is that under the time warp: <TRAIN, TW> of (4), which also leaves lin at the arg-max and r2.
//
// Bilinear form (attn_common.h): x[t,(g,j)] = rs[t] sum_c h[t,c] Qs[g,j,c] + (Rh.h[t] + R2.h[t]^2) + ct[g,j].
// Launches, all on the caller's stream, none waits for the host:
//   1. attn_vecs_kernel            the per-channel vectors of att_logits/W (attn_fwd.hip's)
//   2. attn_shared_prep_q_kernel   Qs [NQ][JP][w] (rows j >= JQ zero), ct [NQ][JP]; JP = 32 (JQ <= 32) or 64
//   3. attn_shared_plan_kernel     one workgroup: counting sort of `album` (clamped into [0, A)), groups of <= G questions
//                                  cut per album: grp[] = {album, first, count}, order[], qslot[], ngroups
//   4. attn_shared_logits_kernel   one workgroup per (group, k, tile of SH_R rows): the product (BM x BN 256 = G JP), row
//                                  terms, tanh, exp_mask, max over j -> amax [NQ,K,T] (and a_logits).  A tile without a
//                                  valid row skips the product: its logits are -1e30 whatever the rows hold
//   5. attn_shared_softmax_kernel  per question: M[k] = max_t amax, L[k] = sum_t exp(amax - M[k]), coef[k] =
//                                  softmax_k(M)[k] / L[k].  Masking needs no special case: a fully masked (album, k) or
//                                  question has amax = -1e30 everywhere, which IS the uniform softmax over all T
//   6. attn_shared_wsum_kernel     one workgroup per (group, k, split of T): part[g] = coef sum_t exp(amax - M) h[t] for
//                                  the G questions from ONE read of each row
//   7. attn_shared_merge_kernel    h_a[q] = sum over (k, split) of the partials, in that order
// Row traffic: (4) and (6) read each row of an album once per group of that album: twice per group, never per question.
// Determinism: no floating-point atomics.  The split of T depends on the descriptor only; a question's numbers do not
// depend on which group, slot or wave it lands in (every column of the product is its own k-ordered fmaf chain, every
// question has its own accumulators), so the integer atomics that place the questions in `order` cannot change a bit.
// The backward DOES sum over an album's questions in `order`: the training plan fills it by ascending question index from a
// single wave (attn_shared_plan_kernel<true>), a function of `album` alone.
// The templates of (3), (4) and (6) stand in attn_shared_kernels.h: attn_pool.hip (per-question album lists over one
// album pool) instantiates them with its own addressing.
#include "attn_shared_kernels.h"
#include "timewarp_common.h"

namespace fvta {

// ---- question side.  grid (NQ, JP / 4), 256 threads: a wave per position j
__global__ __launch_bounds__(256) void attn_shared_prep_q_kernel(ShShape s, ShWork wk, const float* __restrict__ hq,
                                                                 const float* __restrict__ bptr) {
  const int q = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, w = s.w;
  const float* Uv = wk.vecs + VEC_U * w;
  const float* Cq = wk.vecs + VEC_CQ * w;
  const float* C2 = wk.vecs + VEC_C2 * w;
  const float bias = (s.simi == 4 || bptr == nullptr) ? 0.f : bptr[0];
  const int j = 4 * blockIdx.y + wave;
  float* dst = wk.Qs + ((size_t)q * s.JP + j) * w;
  if (j >= s.JQ) {  // (wave-uniform)
    for (int c = lane; c < w; c += 64) dst[c] = 0.f;
    if (lane == 0) wk.ct[(size_t)q * s.JP + j] = 0.f;
    return;
  }
  const float* row = hq + ((size_t)q * s.JQ + j) * w;
  float s1 = 0.f, s2 = 0.f;
  for (int c = lane; c < w; c += 64) {
    const float v = row[c];
    s1 += Cq[c] * v + C2[c] * v * v;
    s2 += v * v;
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  const float rq = rsqrtf(fmaxf(s2, 1e-12f));  // tf.nn.l2_normalize eps (cosine only)
  for (int c = lane; c < w; c += 64) dst[c] = s.simi == 4 ? row[c] * rq : row[c] * Uv[c];
  if (lane == 0) wk.ct[(size_t)q * s.JP + j] = s.simi == 4 ? 0.f : s1 + bias;
}

// the same bits in every thread: butterflies inside a wave, the four wave results in order
__device__ __forceinline__ float sh_block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
__device__ __forceinline__ float sh_block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// ---- the two softmaxes' scalars.  grid NQ, 256 threads, K <= 64
__global__ __launch_bounds__(256) void attn_shared_softmax_kernel(ShShape s, ShWork wk) {
  __shared__ float red[4], s_M[64], s_L[64];
  const int q = blockIdx.x, tid = threadIdx.x, T = s.T, K = s.K;
  for (int k = 0; k < K; ++k) {
    const float* am = wk.amax + ((size_t)q * K + k) * T;
    float m = -INFINITY;
    for (int t = tid; t < T; t += 256) m = fmaxf(m, am[t]);
    m = sh_block_max(m, red);
    float l = 0.f;
    for (int t = tid; t < T; t += 256) l += expf(am[t] - m);
    l = sh_block_sum(l, red);
    if (tid == 0) {
      s_M[k] = m;
      s_L[k] = l;
    }
  }
  __syncthreads();
  if (tid == 0) {  // outer softsel over K (model_v2.py:278): logits = max over (t, j) of the masked logits
    float mx = -INFINITY, sum = 0.f;
    for (int k = 0; k < K; ++k) mx = fmaxf(mx, s_M[k]);
    for (int k = 0; k < K; ++k) sum += expf(s_M[k] - mx);
    for (int k = 0; k < K; ++k) {
      wk.M[(size_t)q * K + k] = s_M[k];
      wk.coef[(size_t)q * K + k] = expf(s_M[k] - mx) / sum / s_L[k];
      if (wk.L) {  // training: the two factors of coef, apart
        wk.L[(size_t)q * K + k] = s_L[k];
        wk.r[(size_t)q * K + k] = expf(s_M[k] - mx) / sum;
      }
    }
  }
}

// ---- merge.  grid (NQ, ceil(w / 256)): a channel per thread, the partials in (k, split) order
__global__ __launch_bounds__(256) void attn_shared_merge_kernel(ShShape s, ShWork wk, float* __restrict__ h_a) {
  const int q = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x;
  if (c >= s.w) return;
  const int slot = wk.qslot[q], grp = slot / s.G, g = slot % s.G;
  float v = 0.f;
  for (int k = 0; k < s.K; ++k) {
    float vk = 0.f;  // training: r[k] u[k], beside h_a's own chain (whose order of sums stays what it is)
    for (int sp = 0; sp < s.S; ++sp) {
      const float p = wk.part[((((size_t)grp * s.K + k) * s.S + sp) * s.G + g) * s.w + c];
      v += p;
      vk += p;
    }
    if (wk.u) {  // r = 0 (underflow): u[k] reaches nothing in the backward, every use carries a factor r
      const float r = wk.r[(size_t)q * s.K + k];
      wk.u[((size_t)q * s.K + k) * s.w + c] = r > 0.f ? vk / r : 0.f;
    }
  }
  h_a[(size_t)q * s.w + c] = v;
}

// ---- under the time warp (fvta_attn_shared_fwd_tw).  The warp (timewarp.hip) is one scalar per (question, position):
//   h'[q,k,t,:] = h[a,k,t,:] scale[q,t],   scale[q,t] = tanh(e[a,t] + K (s0 + WC . lq[q])) cnt(t),   a = album[q]
//   e[a,t] = sum_k sum_c v[c] h[a,k,t,c]^2,   v = WH[:w] WC,   s0 = b_WH . WC + b_WC
// and only e reads the rows: it belongs to the album and is computed once per album set (fvta_attn_shared_energy).
// v[c] = sum_o WH[c][o] WC[o]: tw_vec_kernel's arithmetic (a wave per output, lane-strided, wave_sum).  grid w / 4
__global__ __launch_bounds__(256) void attn_shared_tw_vec_kernel(int w, const float* __restrict__ WH, const float* __restrict__ WC,
                                                                 float* __restrict__ v) {
  const int o = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (o >= w) return;
  float acc = 0.f;
  for (int c = lane; c < w; c += 64) acc += WH[(size_t)o * w + c] * WC[c];
  acc = wave_sum(acc);
  if (lane == 0) v[o] = acc;
}

// e[a,t]: a wave per (a, t), every k (masked rows included, as tw_coef_kernel), in tw_coef_kernel's order.  grid ceil(A T / 4)
__global__ __launch_bounds__(256) void attn_shared_energy_kernel(ShShape s, const float* __restrict__ hinfo, const float* __restrict__ v,
                                                                 float* __restrict__ energy) {
  const int64_t pos = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (pos >= (int64_t)s.A * s.T) return;
  const int a = (int)(pos / s.T), t = (int)(pos % s.T);
  float acc = 0.f;
  for (int k = 0; k < s.K; ++k) {
    const float* row = hinfo + (((size_t)a * s.K + k) * s.T + t) * s.w;
    for (int c = lane * 4; c < s.w; c += 256) {
      const f32x4 h = ld4(row + c), vv = ld4(v + c);
      const f32x4 p = h * h * vv;
      acc += (p[0] + p[1]) + (p[2] + p[3]);
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) energy[pos] = acc;
}

// scale[q,t].  grid (NQ, ceil(T / 256)), 256 threads; every wave takes the two dot products itself (w floats each)
// TRAIN: tanh(z) beside it, for the backward
template <bool TRAIN>
__global__ __launch_bounds__(256) void attn_shared_tw_scale_kernel(ShShape s, int warp_type, int win, const float* __restrict__ energy,
                                                                   const float* __restrict__ lq, const int* __restrict__ album,
                                                                   const float* __restrict__ WHb, const float* __restrict__ WC,
                                                                   const float* __restrict__ WCb, float* __restrict__ scale,
                                                                   float* __restrict__ scale_out, float* __restrict__ tz_out) {
  const int q = blockIdx.x, lane = threadIdx.x & 63, t = blockIdx.y * 256 + threadIdx.x;
  float s0 = 0.f, sq = 0.f;
  for (int c = lane; c < s.w; c += 64) {
    const float wc = WC[c];
    s0 += WHb[c] * wc;
    sq += lq[(size_t)q * s.w + c] * wc;
  }
  s0 = wave_sum(s0) + WCb[0];
  sq = wave_sum(sq);
  if (t >= s.T) return;
  const int a = sh_album(album, q, s.A);
  const float tz = tanhf(energy[(size_t)a * s.T + t] + (float)s.K * (s0 + sq));
  const float sc = tz * tw_count(t, s.T, warp_type, win);
  if constexpr (TRAIN) tz_out[(size_t)q * s.T + t] = tz;
  scale[(size_t)q * s.T + t] = sc;
  if (scale_out) scale_out[(size_t)q * s.T + t] = sc;
}

// 0: fine, else the status with the message set
int fvta_attn_shared_check(const fvta_attn_shared_desc* d, const char* who) {
  FVTA_CHECK_ARG(d != nullptr, "%s: null descriptor", who);
  FVTA_CHECK_ARG(d->A > 0 && d->NQ > 0 && d->K > 0 && d->T > 0 && d->JQ > 0 && d->w > 0, "%s: bad A/NQ/K/T/JQ/w (%d,%d,%d,%d,%d,%d)",
                 who, d->A, d->NQ, d->K, d->T, d->JQ, d->w);
  const char* why = nullptr;
  const int w = d->w;
  if (d->simi < 1 || d->simi > 4) {
    fvta_set_error("%s: similarity matrix not implemented (simiMatrix=%d)", who, d->simi);
    return FVTA_ERR_UNSUPPORTED;
  }
  if (!(w == 64 || w == 128 || w == 256 || w == 512 || w == 1024 || w == 2048))
    why = "w must be one of 64,128,256,512,1024,2048";
  else if (d->JQ > 64)
    why = "JQ must be 1..64";
  else if (d->K > 64)
    why = "K must be 1..64";
  else if (d->A > (1 << 28) || d->NQ > (1 << 28))
    why = "A and NQ must not exceed 2^28";
  if (!why) {
    const ShShape s = sh_shape(d);
    if ((int64_t)s.ngmax * d->K * s.ntile > 0x7fffffff || (int64_t)s.ngmax * d->K * s.S > 0x7fffffff) why = "too many workgroups";
  }
  if (why) {
    fvta_set_error("%s: unsupported shape (A=%d NQ=%d K=%d T=%d JQ=%d w=%d): %s", who, d->A, d->NQ, d->K, d->T, d->JQ, w, why);
    return FVTA_ERR_UNSUPPORTED;
  }
  return FVTA_OK;
}

}  // namespace fvta
using namespace fvta;

extern "C" size_t fvta_attn_shared_workspace_bytes(const fvta_attn_shared_desc* d) {
  if (fvta_attn_shared_check(d, "attn_shared_workspace_bytes") != FVTA_OK) return 0;
  return ShWork(sh_shape(d), nullptr).bytes;
}

extern "C" int fvta_attn_shared_plan(const fvta_attn_shared_desc* d, int32_t out[4]) {
  if (int e = fvta_attn_shared_check(d, "attn_shared_plan")) return e;
  FVTA_CHECK_ARG(out != nullptr, "attn_shared_plan: null pointer");
  const ShShape s = sh_shape(d);
  out[0] = s.G;
  out[1] = SH_R;
  out[2] = s.S;
  out[3] = s.rps;
  return FVTA_OK;
}

// the seven launches; TRAIN: the ordered plan and the arg-max, wk carved from (saved, workspace); TW: under the time warp,
// tw_scale [NQ,T] written by an earlier launch on the same stream
template <bool TRAIN, bool TW = false>
static int sh_forward(ShShape s, const ShWork& wk, const float* hinfo, const uint8_t* hmask, const float* hq, const uint8_t* qmask,
                      const int32_t* album, const float* W, const float* b, float* h_a, float* a_logits, hipStream_t st,
                      const float* tw_scale = nullptr, const char* who = nullptr, float* tw_lin = nullptr, float* tw_r2 = nullptr) {
  s.use_mask = (hmask && qmask) ? 1 : 0;  // model_v2.py:233: the mask applies only when both are given
  // attn_fwd.hip's kernel, declared in attn_common.h (feat_order 0 = model_v2.py's)
  hipLaunchKernelGGL(attn_vecs_kernel, dim3((s.w + 255) / 256), dim3(256), 0, st, W, s.w, s.simi, 0, wk.vecs);
  hipLaunchKernelGGL(attn_shared_prep_q_kernel, dim3(s.NQ, s.JP / 4), dim3(256), 0, st, s, wk, hq, b);
  hipLaunchKernelGGL(attn_shared_plan_kernel<TRAIN>, dim3(1), dim3(SH_PLAN_NT), 0, st, s, wk, (const int*)album);
  const dim3 lgrid((unsigned)((int64_t)s.ngmax * s.K * s.ntile));
  const ShTwArgs tw{tw_scale, tw_lin, tw_r2};
  if (s.JP == 32)
    hipLaunchKernelGGL((attn_shared_logits_kernel<1, TRAIN, TW>), lgrid, dim3(SH_NT), 0, st, s, wk, hinfo, hmask, qmask, a_logits,
                       tw);
  else
    hipLaunchKernelGGL((attn_shared_logits_kernel<2, TRAIN, TW>), lgrid, dim3(SH_NT), 0, st, s, wk, hinfo, hmask, qmask, a_logits,
                       tw);
  hipLaunchKernelGGL(attn_shared_softmax_kernel, dim3(s.NQ), dim3(256), 0, st, s, wk);
  if (s.G == 8)
    sh_launch_wsum<8, TW>(s, wk, hinfo, tw_scale, st);
  else
    sh_launch_wsum<4, TW>(s, wk, hinfo, tw_scale, st);
  hipLaunchKernelGGL(attn_shared_merge_kernel, dim3(s.NQ, (s.w + 255) / 256), dim3(256), 0, st, s, wk, h_a);
  FVTA_CHECK_LAUNCH(who ? who : (TRAIN ? "attn_shared_fwd_train" : "attn_shared_fwd"));
  return FVTA_OK;
}

extern "C" int fvta_attn_shared_fwd(const fvta_attn_shared_desc* d, const float* hinfo, const uint8_t* hmask, const float* hq,
                                    const uint8_t* qmask, const int32_t* album, const float* W, const float* b, float* h_a,
                                    float* a_logits, void* workspace, fvta_stream_t stream_) {
  if (int e = fvta_attn_shared_check(d, "attn_shared_fwd")) return e;
  FVTA_CHECK_ARG(hinfo && hq && album && h_a && workspace, "attn_shared_fwd: null pointer");
  FVTA_CHECK_ARG(d->simi == 4 || W, "attn_shared_fwd: simiMatrix %d needs att_logits/W", d->simi);
  const ShShape s = sh_shape(d);
  return sh_forward<false>(s, ShWork(s, workspace), hinfo, hmask, hq, qmask, album, W, b, h_a, a_logits, (hipStream_t)stream_);
}

// ---- training.  The same kernels on the same numbers (h_a and a_logits are fvta_attn_shared_fwd's bits: the placement of
// a question changes none, see the header), with what the backward (attn_shared_bwd.hip) reads left in `saved`.
int fvta::fvta_attn_shared_check_train(const fvta_attn_shared_desc* d, const char* who) {
  if (int e = fvta_attn_shared_check(d, who)) return e;
  if (d->simi == 4) {
    fvta_set_error("%s: simiMatrix 4 has no shared-context backward (simiMatrix 1-3); the per-question route "
                   "(fvta_attn_fwd / fvta_attn_bwd on the gathered rows) covers it", who);
    return FVTA_ERR_UNSUPPORTED;
  }
  return FVTA_OK;
}

extern "C" size_t fvta_attn_shared_saved_bytes(const fvta_attn_shared_desc* d) {
  if (fvta_attn_shared_check_train(d, "attn_shared_saved_bytes") != FVTA_OK) return 0;
  return ShWork(sh_shape(d), nullptr, nullptr).saved_bytes;
}

extern "C" int fvta_attn_shared_fwd_train(const fvta_attn_shared_desc* d, const float* hinfo, const uint8_t* hmask,
                                          const float* hq, const uint8_t* qmask, const int32_t* album, const float* W,
                                          const float* b, float* h_a, float* a_logits, void* saved, void* workspace,
                                          fvta_stream_t stream_) {
  if (int e = fvta_attn_shared_check_train(d, "attn_shared_fwd_train")) return e;
  FVTA_CHECK_ARG(hinfo && hq && album && W && h_a && saved && workspace, "attn_shared_fwd_train: null pointer");
  const ShShape s = sh_shape(d);
  return sh_forward<true>(s, ShWork(s, saved, workspace), hinfo, hmask, hq, qmask, album, W, b, h_a, a_logits,
                          (hipStream_t)stream_);
}

// ---- under the time warp.  The workspace: fvta_attn_shared_fwd's, then scale [NQ,T], then v [w] (the energy call's)
namespace fvta {
struct ShTwWork {
  ShWork wk;
  float *scale, *v;
  size_t bytes;
  ShTwWork(const ShShape& s, void* p) : wk(s, p) {
    FvtaCarver c(p);
    c.off = wk.bytes;
    scale = c.take<float>((size_t)s.NQ * s.T);
    v = c.take<float>((size_t)s.w);
    bytes = c.off;
  }
};

int fvta_attn_shared_check_warp(int warp_type, float window_t, const char* who) {
  if (warp_type < 1 || warp_type > 5) {
    fvta_set_error("%s: time warping type not implemented (warp_type=%d)", who, warp_type);  // model_v2.py:341
    return FVTA_ERR_INVALID_ARG;
  }
  FVTA_CHECK_ARG(window_t >= 0.f && window_t <= 1e9f, "%s: bad window_t (%g)", who, (double)window_t);
  return FVTA_OK;
}

int fvta_attn_shared_check_tw(const fvta_attn_shared_tw_desc* d, const char* who, bool train) {
  FVTA_CHECK_ARG(d != nullptr, "%s: null descriptor", who);
  if (int e = train ? fvta_attn_shared_check_train(&d->shape, who) : fvta_attn_shared_check(&d->shape, who)) return e;
  if (int e = fvta_attn_shared_check_warp(d->warp_type, d->window_t, who)) return e;
  if (d->shape.T > 65535 * 256) {
    fvta_set_error("%s: unsupported shape (T=%d): T must not exceed 65535 * 256 under the time warp", who, d->shape.T);
    return FVTA_ERR_UNSUPPORTED;
  }
  return FVTA_OK;
}
}  // namespace fvta

extern "C" size_t fvta_attn_shared_tw_workspace_bytes(const fvta_attn_shared_tw_desc* d) {
  if (fvta_attn_shared_check_tw(d, "attn_shared_tw_workspace_bytes") != FVTA_OK) return 0;
  return ShTwWork(sh_shape(&d->shape), nullptr).bytes;
}

extern "C" int fvta_attn_shared_energy(const fvta_attn_shared_tw_desc* d, const float* hinfo, const float* WH_W, const float* WC_W,
                                       float* energy, void* workspace, fvta_stream_t stream_) {
  if (int e = fvta_attn_shared_check_tw(d, "attn_shared_energy")) return e;
  FVTA_CHECK_ARG(hinfo && WH_W && WC_W && energy && workspace, "attn_shared_energy: null pointer");
  const ShShape s = sh_shape(&d->shape);
  const ShTwWork tw(s, workspace);
  hipStream_t st = (hipStream_t)stream_;
  hipLaunchKernelGGL(attn_shared_tw_vec_kernel, dim3((s.w + 3) / 4), dim3(256), 0, st, s.w, WH_W, WC_W, tw.v);
  hipLaunchKernelGGL(attn_shared_energy_kernel, dim3((unsigned)(((int64_t)s.A * s.T + 3) / 4)), dim3(256), 0, st, s, hinfo, tw.v,
                     energy);
  FVTA_CHECK_LAUNCH("attn_shared_energy");
  return FVTA_OK;
}

extern "C" int fvta_attn_shared_fwd_tw(const fvta_attn_shared_tw_desc* d, const float* hinfo, const uint8_t* hmask,
                                       const float* energy, const float* hq, const uint8_t* qmask, const float* lq,
                                       const int32_t* album, const float* W, const float* b, const float* WH_b, const float* WC_W,
                                       const float* WC_b, float* h_a, float* a_logits, float* scale_out, void* workspace,
                                       fvta_stream_t stream_) {
  if (int e = fvta_attn_shared_check_tw(d, "attn_shared_fwd_tw")) return e;
  FVTA_CHECK_ARG(hinfo && energy && hq && lq && album && WH_b && WC_W && WC_b && h_a && workspace, "attn_shared_fwd_tw: null pointer");
  FVTA_CHECK_ARG(d->shape.simi == 4 || W, "attn_shared_fwd_tw: simiMatrix %d needs att_logits/W", d->shape.simi);
  const ShShape s = sh_shape(&d->shape);
  const ShTwWork tw(s, workspace);
  hipStream_t st = (hipStream_t)stream_;
  hipLaunchKernelGGL(attn_shared_tw_scale_kernel<false>, dim3(s.NQ, (s.T + 255) / 256), dim3(256), 0, st, s, d->warp_type,
                     (int)ceilf(d->window_t), energy, lq, (const int*)album, WH_b, WC_W, WC_b, tw.scale, scale_out, (float*)nullptr);
  return sh_forward<false, true>(s, tw.wk, hinfo, hmask, hq, qmask, album, W, b, h_a, a_logits, st, tw.scale, "attn_shared_fwd_tw");
}

// ---- training under the time warp.  The kernels of fvta_attn_shared_fwd_tw on the same numbers -- h_a, a_logits and
// scale_out are its bits -- with the ordered plan, the arg-max, and in `saved` what attn_shared_bwd.hip's
// fvta_attn_shared_bwd_tw reads: fvta_attn_shared_fwd_train's pieces, then scale, tanh(z), lin at the arg-max and r2.
extern "C" size_t fvta_attn_shared_tw_saved_bytes(const fvta_attn_shared_tw_desc* d) {
  if (fvta_attn_shared_check_tw(d, "attn_shared_tw_saved_bytes", true) != FVTA_OK) return 0;
  const ShShape s = sh_shape(&d->shape);
  return ShTwSaved(s, ShWork(s, nullptr, nullptr), nullptr).bytes;
}

extern "C" int fvta_attn_shared_fwd_tw_train(const fvta_attn_shared_tw_desc* d, const float* hinfo, const uint8_t* hmask,
                                             const float* energy, const float* hq, const uint8_t* qmask, const float* lq,
                                             const int32_t* album, const float* W, const float* b, const float* WH_b,
                                             const float* WC_W, const float* WC_b, float* h_a, float* a_logits, float* scale_out,
                                             void* saved, void* workspace, fvta_stream_t stream_) {
  if (int e = fvta_attn_shared_check_tw(d, "attn_shared_fwd_tw_train", true)) return e;
  FVTA_CHECK_ARG(hinfo && energy && hq && lq && album && W && WH_b && WC_W && WC_b && h_a && saved && workspace,
                 "attn_shared_fwd_tw_train: null pointer");
  const ShShape s = sh_shape(&d->shape);
  const ShWork wk(s, saved, workspace);  // (its share of the workspace is no larger than the inference call's)
  const ShTwSaved ts(s, wk, saved);
  hipStream_t st = (hipStream_t)stream_;
  hipLaunchKernelGGL(attn_shared_tw_scale_kernel<true>, dim3(s.NQ, (s.T + 255) / 256), dim3(256), 0, st, s, d->warp_type,
                     (int)ceilf(d->window_t), energy, lq, (const int*)album, WH_b, WC_W, WC_b, ts.scale, scale_out, ts.tz);
  return sh_forward<true, true>(s, wk, hinfo, hmask, hq, qmask, album, W, b, h_a, a_logits, st, ts.scale, "attn_shared_fwd_tw_train",
                                ts.lin, ts.r2);
}

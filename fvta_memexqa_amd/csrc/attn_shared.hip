// Focal attention forward for MANY QUESTIONS OVER ONE ALBUM (fvta_attn_shared_fwd): hinfo [A,K,T,w] holds each album's
// context rows once, question i reads album[i]'s.  Per question the result is fvta_attn_fwd's on the pair
// (hinfo[album[i]], hq[i]) -- model_v2.py:210-298 -- but a row is fetched once per GROUP of up to G questions of the same
// album instead of once per question, and the logits of a group are one [rows, w] x [w, G JP] product on the fp32 matrix
// pipe (gemm_f32.h: v_mfma_f32_32x32x2_f32, exact fp32).  No shadow rows; the time warp: fvta_attn_shared_fwd_tw, the TW
// instantiations of (4) and (6), further down.  fvta_attn_shared_fwd keeps nothing
// for a backward; fvta_attn_shared_fwd_train runs the same kernels -- the same bits -- with the ordered plan (3) and the
// arg-max (4) compiled in, and leaves what attn_shared_bwd.hip reads in the caller-held `saved` (attn_shared_common.h).
// fvta_attn_shared_fwd_tw_train is that under the time warp: <TRAIN, TW> of (4), which also leaves lin at the arg-max and r2
// (fvta_attn_pool_fwd_tw_train: <TRAIN, TW, POOL>, lin at the reference's slot, r2 per pooled album).
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
// Under the time warp attn_shared_tw_scale_kernel goes in front: 8.  ONE driver makes them for every forward entry point:
// sh_forward, near the end of this file, which says what TRAIN, TW and POOL each change.
// Row traffic: (4) and (6) read each row of an album once per group of that album: twice per group, never per question.
// Determinism: no floating-point atomics.  The split of T depends on the descriptor only; a question's numbers do not
// depend on which group, slot or wave it lands in (every column of the product is its own k-ordered fmaf chain, every
// question has its own accumulators), so the integer atomics that place the questions in `order` cannot change a bit.
// The backward DOES sum over an album's questions in `order`: the training plan fills it by ascending question index from a
// single wave (attn_shared_plan_kernel<true>), a function of `album` alone.
// The templates of (3), (4) and (6) stand in attn_shared_kernels.h with the compile-time word POOL: the pooled call
// (per-question album lists over one album pool; attn_pool.hip has its entry points and says what POOL means) runs through
// the same driver, which adds attn_pool_empty_kernel after (4): 8 launches, 9 under the warp.
#include "attn_shared_kernels.h"
#include "attn_shared_bwd_kernels.h"  // (ShBwdShape: the training checks cover the backward's grids)
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

// ---- the pooled call's empty slots.  grid NQ M, 256 threads: a workgroup per reference, gone at once unless its slot is
// empty; then the slot's JX positions get amax = -1e30 for every k (a_logits too): no product, no row read
// TRAIN: jmax = 0 over the slot's positions too (never read: no reference stands there; defined all the same)
template <bool TRAIN>
__global__ __launch_bounds__(256) void attn_pool_empty_kernel(ShShape s, ShWork wk, const int* __restrict__ albums,
                                                              float* __restrict__ a_logits) {
  const int ref = blockIdx.x;
  if (albums[ref] >= 0) return;
  const int q = ref / s.M, off = (ref % s.M) * s.T;
  for (int k = 0; k < s.K; ++k) {
    const size_t at = ((size_t)q * s.K + k) * s.TO + off;
    for (int e = threadIdx.x; e < s.T; e += 256) wk.amax[at + e] = FVTA_NEG;
    if constexpr (TRAIN)
      for (int e = threadIdx.x; e < s.T; e += 256) wk.jmax[at + e] = 0;
    if (a_logits)
      for (int64_t e = threadIdx.x; e < (int64_t)s.T * s.JQ; e += 256) a_logits[at * s.JQ + e] = FVTA_NEG;
  }
}

// ---- merge.  grid (NQ, ceil(w / 256)): a channel per thread, the question's partials in (k, slot, split) order -- (k, split)
// with one slot; POOL: M slots, an empty one (qslot < 0) passed over: its rows are zero
// TRAIN: u[q,k] = (the partials of k, in that order) / r[q,k] beside h_a's own chain, whose order of sums stays what it is
template <bool TRAIN, bool POOL>
__global__ __launch_bounds__(256) void attn_shared_merge_kernel(ShShape s, ShWork wk, float* __restrict__ h_a) {
  const int q = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x, M = POOL ? s.M : 1;
  if (c >= s.w) return;
  float v = 0.f;
  for (int k = 0; k < s.K; ++k) {
    float vk = 0.f;
    for (int m = 0; m < M; ++m) {
      const int slot = wk.qslot[(size_t)q * M + m];
      if (POOL && slot < 0) continue;
      const int grp = slot / s.G, g = slot % s.G;
      for (int sp = 0; sp < s.S; ++sp) {
        const float p = wk.part[((((size_t)grp * s.K + k) * s.S + sp) * s.G + g) * s.w + c];
        v += p;
        if constexpr (TRAIN) vk += p;
      }
    }
    if constexpr (TRAIN) {  // r = 0 (underflow): u[k] reaches nothing in the backward, every use carries a factor r
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
// ROW: float, or bf16_t for a pool held in bf16 (attn_shared_kernels.h: the load widens, the sums are the fp32 kernel's)
template <class ROW>
__global__ __launch_bounds__(256) void attn_shared_energy_kernel(ShShape s, const ROW* __restrict__ hinfo, const float* __restrict__ v,
                                                                 float* __restrict__ energy) {
  const int64_t pos = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (pos >= (int64_t)s.A * s.T) return;
  const int a = (int)(pos / s.T), t = (int)(pos % s.T);
  float acc = 0.f;
  for (int k = 0; k < s.K; ++k) {
    const ROW* row = hinfo + (((size_t)a * s.K + k) * s.T + t) * s.w;
    for (int c = lane * 4; c < s.w; c += 256) {
      const f32x4 h = ld4(row + c), vv = ld4(v + c);
      const f32x4 p = h * h * vv;
      acc += (p[0] + p[1]) + (p[2] + p[3]);
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) energy[pos] = acc;
}

// scale[q,t] over the question's WHOLE TO positions.  grid (NQ, ceil(TO / 256)), 256 threads; every wave takes the two dot
// products itself (w floats each).  TRAIN: tanh(z) beside it, for the backward
// POOL: t = m JX + j; the energy is taken per slot -- the album index clamped as the plan clamps it, an empty slot's e = 0
// (JX zero rows) -- and the count is that of the GLOBAL position t.  With one slot: the same bits
template <bool TRAIN, bool POOL>
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
  if (t >= s.TO) return;
  const int m = POOL ? t / s.T : 0, a = sh_ref_album<POOL>(album, q * s.M + m, s.A);
  const float e = POOL && a < 0 ? 0.f : energy[(size_t)a * s.T + (t - m * s.T)];
  const float tz = tanhf(e + (float)s.K * (s0 + sq));
  const float sc = tz * tw_count(t, s.TO, warp_type, win);
  if constexpr (TRAIN) tz_out[(size_t)q * s.TO + t] = tz;
  scale[(size_t)q * s.TO + t] = sc;
  if (scale_out) scale_out[(size_t)q * s.TO + t] = sc;
}

// ---- the checks.  How a refusal prints the descriptor: the family's own letters
static const char* sh_describe(const ShShape& s, bool pool, char (&buf)[128]) {
  if (pool)
    snprintf(buf, sizeof buf, "P=%d NQ=%d M=%d K=%d JX=%d JQ=%d w=%d", s.A, s.NQ, s.M, s.K, s.T, s.JQ, s.w);
  else
    snprintf(buf, sizeof buf, "A=%d NQ=%d K=%d T=%d JQ=%d w=%d", s.A, s.NQ, s.K, s.T, s.JQ, s.w);
  return buf;
}

static int sh_refuse_shape(const ShShape& s, bool pool, const char* who, const char* why) {
  char buf[128];
  fvta_set_error("%s: unsupported shape (%s): %s", who, sh_describe(s, pool, buf), why);
  return FVTA_ERR_UNSUPPORTED;
}

// the backward's grids: the row pass's and the question pass's
static int sh_check_bwd_grids(const ShShape& s, bool pool, const char* who) {
  const ShBwdShape b = shb_shape(s);
  if ((int64_t)s.A * s.K * b.nch > 0x7fffffff || (int64_t)s.ngmax * b.TS * b.nsl > 0x7fffffff)
    return sh_refuse_shape(s, pool, who, "too many workgroups");
  return FVTA_OK;
}

int sh_check(ShShape& s, bool pool, const char* who, ShLevel level) {
  if (pool)
    FVTA_CHECK_ARG(s.A > 0 && s.NQ > 0 && s.M > 0 && s.K > 0 && s.T > 0 && s.JQ > 0 && s.w > 0,
                   "%s: bad P/NQ/M/K/JX/JQ/w (%d,%d,%d,%d,%d,%d,%d)", who, s.A, s.NQ, s.M, s.K, s.T, s.JQ, s.w);
  else
    FVTA_CHECK_ARG(s.A > 0 && s.NQ > 0 && s.K > 0 && s.T > 0 && s.JQ > 0 && s.w > 0, "%s: bad A/NQ/K/T/JQ/w (%d,%d,%d,%d,%d,%d)",
                   who, s.A, s.NQ, s.K, s.T, s.JQ, s.w);
  const char* why = nullptr;
  const int w = s.w;
  if (s.simi < 1 || s.simi > 4) {
    fvta_set_error("%s: similarity matrix not implemented (simiMatrix=%d)", who, s.simi);
    return FVTA_ERR_UNSUPPORTED;
  }
  if (!(w == 64 || w == 128 || w == 256 || w == 512 || w == 1024 || w == 2048))
    why = "w must be one of 64,128,256,512,1024,2048";
  else if (s.JQ > 64)
    why = "JQ must be 1..64";
  else if (s.K > 64)
    why = "K must be 1..64";
  else if (s.A > (1 << 28) || (int64_t)s.NQ * s.M > (1 << 28))
    why = pool ? "P and NQ*M must not exceed 2^28" : "A and NQ must not exceed 2^28";
  else if ((int64_t)s.M * s.T > 0x7fffffff)  // (one slot: T is an int)
    why = "M*JX must fit a 32-bit int";
  if (!why) {
    sh_derive(s);
    if ((int64_t)s.ngmax * s.K * s.ntile > 0x7fffffff || (int64_t)s.ngmax * s.K * s.S > 0x7fffffff) why = "too many workgroups";
  }
  if (why) return sh_refuse_shape(s, pool, who, why);
  if (level >= SH_TRAIN && s.simi == 4) {
    fvta_set_error("%s: simiMatrix 4 has no %s backward (simiMatrix 1-3); the per-question route "
                   "(fvta_attn_fwd / fvta_attn_bwd on the gathered rows) covers it", who, pool ? "pooled" : "shared-context");
    return FVTA_ERR_UNSUPPORTED;
  }
  return level >= SH_BWD ? sh_check_bwd_grids(s, pool, who) : FVTA_OK;
}

int sh_check_tw(ShShape& s, bool pool, int warp_type, float window_t, const char* who, ShLevel level) {
  if (int e = sh_check(s, pool, who, level >= SH_TRAIN ? SH_TRAIN : SH_FWD)) return e;
  if (warp_type < 1 || warp_type > 5) {
    fvta_set_error("%s: time warping type not implemented (warp_type=%d)", who, warp_type);  // model_v2.py:341
    return FVTA_ERR_INVALID_ARG;
  }
  FVTA_CHECK_ARG(window_t >= 0.f && window_t <= 1e9f, "%s: bad window_t (%g)", who, (double)window_t);
  if (s.TO > 65535 * 256) {  // the scale kernel's grid
    if (pool)
      fvta_set_error("%s: unsupported shape (M=%d JX=%d): M*JX must not exceed 65535 * 256 under the time warp", who, s.M, s.T);
    else
      fvta_set_error("%s: unsupported shape (T=%d): T must not exceed 65535 * 256 under the time warp", who, s.T);
    return FVTA_ERR_UNSUPPORTED;
  }
  if (pool && ((int64_t)s.A * s.T + 3) / 4 > 0x7fffffff) {  // the energy kernel's grid
    fvta_set_error("%s: unsupported shape (P=%d JX=%d): too many workgroups", who, s.A, s.T);
    return FVTA_ERR_UNSUPPORTED;
  }
  return level >= SH_BWD ? sh_check_bwd_grids(s, pool, who) : FVTA_OK;
}

int sh_plan(const ShShape& s, const char* who, int32_t out[4]) {
  FVTA_CHECK_ARG(out != nullptr, "%s: null pointer", who);
  out[0] = s.G;
  out[1] = SH_R;
  out[2] = s.S;
  out[3] = s.rps;
  return FVTA_OK;
}

int sh_energy(const ShShape& s, const char* who, const float* rows, const float* WH_W, const float* WC_W, float* energy,
              void* workspace, fvta_stream_t stream, const bf16_t* rows_bf16) {
  FVTA_CHECK_ARG((rows || rows_bf16) && WH_W && WC_W && energy && workspace, "%s: null pointer", who);
  const ShTwWork tw(s, workspace);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(((int64_t)s.A * s.T + 3) / 4));
  hipLaunchKernelGGL(attn_shared_tw_vec_kernel, dim3((s.w + 3) / 4), dim3(256), 0, st, s.w, WH_W, WC_W, tw.v);
  if (rows_bf16)
    hipLaunchKernelGGL(attn_shared_energy_kernel<bf16_t>, grid, dim3(256), 0, st, s, rows_bf16, tw.v, energy);
  else
    hipLaunchKernelGGL(attn_shared_energy_kernel<float>, grid, dim3(256), 0, st, s, rows, tw.v, energy);
  FVTA_CHECK_LAUNCH(who);
  return FVTA_OK;
}

// ---- the forward driver.  The launches of the header, in its order, for every entry point of both families:
//   TW    the scale kernel in front (into the workspace, TRAIN: into `saved`, tanh(z) beside it) and the TW logits / weighted sum
//   TRAIN the ordered plan, the arg-max, L / r / u: wk carved from (saved, workspace) -- its share of the workspace is no
//         larger than the inference call's
//   POOL  the references' addressing in plan / logits / weighted sum / merge, and the empty slots' launch after the logits
//   ROW   how the logits and the weighted sum load a row: c.rows (float), or c.rows_bf16 (bf16_t; <false, ., true> only)
// and nothing else depends on any of the four
template <bool TRAIN, bool TW, bool POOL, class ROW = float>
static int sh_forward_as(ShShape s, const char* who, const ShFwdCall& c, const ShWarpCall* warp) {
  hipStream_t st = (hipStream_t)c.stream;
  const ROW* rows;
  if constexpr (std::is_same<ROW, bf16_t>::value) rows = c.rows_bf16; else rows = c.rows;
  const ShWork wk = TRAIN ? ShWork(s, c.saved, c.workspace) : ShWork(s, c.workspace);
  ShTwArgs tw{nullptr, nullptr, nullptr};
  if constexpr (TW) {
    float *scale, *tz = nullptr;
    if constexpr (TRAIN) {
      const ShTwSaved ts(s, wk, c.saved);
      scale = ts.scale, tz = ts.tz, tw.lin = ts.lin, tw.r2 = ts.r2;
    } else {
      scale = ShTwWork(s, c.workspace).scale;
    }
    tw.scale = scale;
    hipLaunchKernelGGL((attn_shared_tw_scale_kernel<TRAIN, POOL>), dim3(s.NQ, (s.TO + 255) / 256), dim3(256), 0, st, s, warp->warp_type,
                       (int)ceilf(warp->window_t), warp->energy, warp->lq, (const int*)c.index, warp->WH_b, warp->WC_W, warp->WC_b,
                       scale, warp->scale_out, tz);
  }
  s.use_mask = (c.rows_mask && c.qmask) ? 1 : 0;  // model_v2.py:233: the mask applies only when both are given
  // attn_fwd.hip's kernel, declared in attn_common.h (feat_order 0 = model_v2.py's)
  hipLaunchKernelGGL(attn_vecs_kernel, dim3((s.w + 255) / 256), dim3(256), 0, st, c.W, s.w, s.simi, 0, wk.vecs);
  hipLaunchKernelGGL(attn_shared_prep_q_kernel, dim3(s.NQ, s.JP / 4), dim3(256), 0, st, s, wk, c.hq, c.b);
  hipLaunchKernelGGL((attn_shared_plan_kernel<TRAIN, POOL>), dim3(1), dim3(SH_PLAN_NT), 0, st, s, wk, (const int*)c.index);
  const dim3 lgrid((unsigned)((int64_t)s.ngmax * s.K * s.ntile));
  if (s.JP == 32)
    hipLaunchKernelGGL((attn_shared_logits_kernel<1, TRAIN, TW, POOL, ROW>), lgrid, dim3(SH_NT), 0, st, s, wk, rows, c.rows_mask,
                       c.qmask, c.a_logits, tw);
  else
    hipLaunchKernelGGL((attn_shared_logits_kernel<2, TRAIN, TW, POOL, ROW>), lgrid, dim3(SH_NT), 0, st, s, wk, rows, c.rows_mask,
                       c.qmask, c.a_logits, tw);
  if constexpr (POOL)
    hipLaunchKernelGGL(attn_pool_empty_kernel<TRAIN>, dim3(s.NR), dim3(256), 0, st, s, wk, (const int*)c.index, c.a_logits);
  ShShape sq = s;  // the softmaxes run per question over all of its positions
  sq.T = s.TO;
  hipLaunchKernelGGL(attn_shared_softmax_kernel, dim3(s.NQ), dim3(256), 0, st, sq, wk);
  if (s.G == 8)
    sh_launch_wsum<8, TW, POOL, ROW>(s, wk, rows, tw.scale, st);
  else
    sh_launch_wsum<4, TW, POOL, ROW>(s, wk, rows, tw.scale, st);
  hipLaunchKernelGGL((attn_shared_merge_kernel<TRAIN, POOL>), dim3(s.NQ, (s.w + 255) / 256), dim3(256), 0, st, s, wk, c.h_a);
  FVTA_CHECK_LAUNCH(who);
  return FVTA_OK;
}

// <TRAIN, TW, POOL> per entry point: TRAIN = a `saved` to fill, TW = the warp's arguments
//   fvta_attn_shared_fwd <0,0,0>   _fwd_train <1,0,0>   _fwd_tw <0,1,0>   _fwd_tw_train <1,1,0>
//   fvta_attn_pool_fwd   <0,0,1>   _fwd_train <1,0,1>   _fwd_tw <0,1,1>   _fwd_tw_train <1,1,1>
//   fvta_attn_pool_fwd_bf16 <0,0,1,bf16_t>   _fwd_tw_bf16 <0,1,1,bf16_t>: the only two with bf16 rows
int sh_forward(const ShShape& s, bool pool, const char* who, const ShFwdCall& c, const ShWarpCall* warp) {
  const bool train = c.saved != nullptr;
  if (c.rows_bf16) {
    FVTA_CHECK_ARG(pool && !train && !c.rows, "%s: bf16 rows are the pooled inference calls' only", who);
    return warp ? sh_forward_as<false, true, true, bf16_t>(s, who, c, warp) : sh_forward_as<false, false, true, bf16_t>(s, who, c, warp);
  }
  if (!pool) {
    if (warp) return train ? sh_forward_as<true, true, false>(s, who, c, warp) : sh_forward_as<false, true, false>(s, who, c, warp);
    return train ? sh_forward_as<true, false, false>(s, who, c, warp) : sh_forward_as<false, false, false>(s, who, c, warp);
  }
  if (!warp) return train ? sh_forward_as<true, false, true>(s, who, c, warp) : sh_forward_as<false, false, true>(s, who, c, warp);
  return train ? sh_forward_as<true, true, true>(s, who, c, warp) : sh_forward_as<false, true, true>(s, who, c, warp);
}

}  // namespace fvta
using namespace fvta;

extern "C" size_t fvta_attn_shared_workspace_bytes(const fvta_attn_shared_desc* d) {
  ShShape s;
  return sh_open(d, "attn_shared_workspace_bytes", s) == FVTA_OK ? ShWork(s, nullptr).bytes : 0;
}

extern "C" int fvta_attn_shared_plan(const fvta_attn_shared_desc* d, int32_t out[4]) {
  ShShape s;
  if (int e = sh_open(d, "attn_shared_plan", s)) return e;
  return sh_plan(s, "attn_shared_plan", out);
}

extern "C" int fvta_attn_shared_fwd(const fvta_attn_shared_desc* d, const float* hinfo, const uint8_t* hmask, const float* hq,
                                    const uint8_t* qmask, const int32_t* album, const float* W, const float* b, float* h_a,
                                    float* a_logits, void* workspace, fvta_stream_t stream_) {
  ShShape s;
  if (int e = sh_open(d, "attn_shared_fwd", s)) return e;
  FVTA_CHECK_ARG(hinfo && hq && album && h_a && workspace, "attn_shared_fwd: null pointer");
  FVTA_CHECK_ARG(d->simi == 4 || W, "attn_shared_fwd: simiMatrix %d needs att_logits/W", d->simi);
  return sh_forward(s, false, "attn_shared_fwd", {hinfo, hmask, hq, qmask, album, W, b, h_a, a_logits, nullptr, workspace, stream_});
}

// ---- training.  The same kernels on the same numbers (h_a and a_logits are fvta_attn_shared_fwd's bits: the placement of
// a question changes none, see the header), with what the backward (attn_shared_bwd.hip) reads left in `saved`.
extern "C" size_t fvta_attn_shared_saved_bytes(const fvta_attn_shared_desc* d) {
  ShShape s;
  return sh_open(d, "attn_shared_saved_bytes", s, SH_TRAIN) == FVTA_OK ? ShWork(s, nullptr, nullptr).saved_bytes : 0;
}

extern "C" int fvta_attn_shared_fwd_train(const fvta_attn_shared_desc* d, const float* hinfo, const uint8_t* hmask,
                                          const float* hq, const uint8_t* qmask, const int32_t* album, const float* W,
                                          const float* b, float* h_a, float* a_logits, void* saved, void* workspace,
                                          fvta_stream_t stream_) {
  ShShape s;
  if (int e = sh_open(d, "attn_shared_fwd_train", s, SH_TRAIN)) return e;
  FVTA_CHECK_ARG(hinfo && hq && album && W && h_a && saved && workspace, "attn_shared_fwd_train: null pointer");
  return sh_forward(s, false, "attn_shared_fwd_train", {hinfo, hmask, hq, qmask, album, W, b, h_a, a_logits, saved, workspace, stream_});
}

// ---- under the time warp.  The workspace: ShTwWork (attn_shared_common.h)
extern "C" size_t fvta_attn_shared_tw_workspace_bytes(const fvta_attn_shared_tw_desc* d) {
  ShShape s;
  return sh_open_tw(d, "attn_shared_tw_workspace_bytes", s) == FVTA_OK ? ShTwWork(s, nullptr).bytes : 0;
}

extern "C" int fvta_attn_shared_energy(const fvta_attn_shared_tw_desc* d, const float* hinfo, const float* WH_W, const float* WC_W,
                                       float* energy, void* workspace, fvta_stream_t stream_) {
  ShShape s;
  if (int e = sh_open_tw(d, "attn_shared_energy", s)) return e;
  return sh_energy(s, "attn_shared_energy", hinfo, WH_W, WC_W, energy, workspace, stream_);
}

extern "C" int fvta_attn_shared_fwd_tw(const fvta_attn_shared_tw_desc* d, const float* hinfo, const uint8_t* hmask,
                                       const float* energy, const float* hq, const uint8_t* qmask, const float* lq,
                                       const int32_t* album, const float* W, const float* b, const float* WH_b, const float* WC_W,
                                       const float* WC_b, float* h_a, float* a_logits, float* scale_out, void* workspace,
                                       fvta_stream_t stream_) {
  ShShape s;
  if (int e = sh_open_tw(d, "attn_shared_fwd_tw", s)) return e;
  FVTA_CHECK_ARG(hinfo && energy && hq && lq && album && WH_b && WC_W && WC_b && h_a && workspace, "attn_shared_fwd_tw: null pointer");
  FVTA_CHECK_ARG(d->shape.simi == 4 || W, "attn_shared_fwd_tw: simiMatrix %d needs att_logits/W", d->shape.simi);
  const ShWarpCall warp{d->warp_type, d->window_t, energy, lq, WH_b, WC_W, WC_b, scale_out};
  return sh_forward(s, false, "attn_shared_fwd_tw", {hinfo, hmask, hq, qmask, album, W, b, h_a, a_logits, nullptr, workspace, stream_},
                    &warp);
}

// ---- training under the time warp.  The kernels of fvta_attn_shared_fwd_tw on the same numbers -- h_a, a_logits and
// scale_out are its bits -- with the ordered plan, the arg-max, and in `saved` what attn_shared_bwd.hip's
// fvta_attn_shared_bwd_tw reads: fvta_attn_shared_fwd_train's pieces, then scale, tanh(z), lin at the arg-max and r2.
extern "C" size_t fvta_attn_shared_tw_saved_bytes(const fvta_attn_shared_tw_desc* d) {
  ShShape s;
  if (sh_open_tw(d, "attn_shared_tw_saved_bytes", s, SH_TRAIN) != FVTA_OK) return 0;
  return ShTwSaved(s, ShWork(s, nullptr, nullptr), nullptr).bytes;
}

extern "C" int fvta_attn_shared_fwd_tw_train(const fvta_attn_shared_tw_desc* d, const float* hinfo, const uint8_t* hmask,
                                             const float* energy, const float* hq, const uint8_t* qmask, const float* lq,
                                             const int32_t* album, const float* W, const float* b, const float* WH_b,
                                             const float* WC_W, const float* WC_b, float* h_a, float* a_logits, float* scale_out,
                                             void* saved, void* workspace, fvta_stream_t stream_) {
  ShShape s;
  if (int e = sh_open_tw(d, "attn_shared_fwd_tw_train", s, SH_TRAIN)) return e;
  FVTA_CHECK_ARG(hinfo && energy && hq && lq && album && W && WH_b && WC_W && WC_b && h_a && saved && workspace,
                 "attn_shared_fwd_tw_train: null pointer");
  const ShWarpCall warp{d->warp_type, d->window_t, energy, lq, WH_b, WC_W, WC_b, scale_out};
  return sh_forward(s, false, "attn_shared_fwd_tw_train", {hinfo, hmask, hq, qmask, album, W, b, h_a, a_logits, saved, workspace, stream_},
                    &warp);
}

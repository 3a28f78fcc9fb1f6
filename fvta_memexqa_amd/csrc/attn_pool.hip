// Focal attention over PER-QUESTION ALBUM LISTS FROM ONE ALBUM POOL (fvta_attn_pool_fwd): pool [P,K,JX,w] holds every
// encoded album once, question i lists M of them (albums [NQ,M]; a negative entry is an empty slot), and its context is
// those albums laid end to end: hinfo_i[k, m JX + j] = pool[albums[i,m], k, j], T = M JX (model_v2.py:863-914 builds that
// tensor per question; the encoders run per (question, album), :704-760, so an album's rows do not depend on its
// neighbours).  Per question the result is fvta_attn_fwd's on (hinfo_i, hq[i]) -- model_v2.py:210-298 -- and no
// [NQ,K,T,w] tensor exists.  fvta_attn_pool_fwd keeps nothing for a backward; the training pair (fvta_attn_pool_fwd_train /
// fvta_attn_pool_bwd) is at the end of this file.
//
// The launches are attn_shared.hip's seven with one change of meaning: a column block of a group's product stands for a
// REFERENCE (question q, slot m), id q M + m, instead of a question (attn_shared_kernels.h, POOL = true):
//   1. attn_vecs_kernel, 2. attn_shared_prep_q_kernel   as they are: Qs and ct belong to the question
//   3. attn_shared_plan_kernel<false, true>   counting sort of the NQ M references by pooled album, empty slots passed
//                                             over (qslot = -1); groups of <= G references of ONE album
//   4. attn_shared_logits_kernel<JT, false, false, true>   per (group, k, tile of SH_R of the album's JX rows): block g reads
//                                             its reference's question's Qs / ct / qmask, writes amax and a_logits at
//                                             positions m JX + row of that question
//      attn_pool_empty_kernel                 an empty slot's JX positions: amax = -1e30 for every k (a_logits too): no
//                                             product, no row read
//   5. attn_shared_softmax_kernel             per question over its T = M JX positions
//   6. attn_shared_wsum_kernel<G, CPT, false, true>   per (group, k, split of JX): one partial per reference from one read
//                                             of each row
//   7. attn_pool_merge_kernel                 h_a[q] = its references' partials in (k, slot, split) order, empty slots
//                                             passed over
// Row traffic: a pooled album's rows are read twice per group of <= G references to it, however many distinct lists there
// are; an album nobody lists is never read.  Determinism: as attn_shared.hip -- no floating-point atomics, the splits
// depend on the descriptor only, a reference's numbers do not depend on its group, block or wave.  At M = 1 every launch
// computes what attn_shared.hip's does: the same bits.
//
// Under the time warp (fvta_attn_pool_fwd_tw): the warp is one scalar per (question, position of its M JX), so the rows
// stay pooled.  attn_pool_tw_scale_kernel goes in front and writes scale [NQ,M JX] from energy [P,JX] (a pooled album's,
// fvta_attn_pool_energy: attn_shared.hip's two energy launches with A = P, T = JX) and the count of the GLOBAL position
// t = m JX + j; (4) and (6) are the <TW, POOL> instantiations, which read the scale at the reference's slot.  At M = 1
// every launch computes what fvta_attn_shared_fwd_tw's does: the same bits.
#include "attn_shared_kernels.h"
#include "attn_shared_bwd_kernels.h"
#include "timewarp_common.h"

namespace fvta {

// ---- empty slots.  grid NQ M, 256 threads: a workgroup per reference, gone at once unless its slot is empty
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

// ---- merge.  grid (NQ, ceil(w / 256)): a channel per thread, the partials in (k, slot, split) order
// TRAIN: u[q,k] = (the partials of k, in (slot, split) order) / r[q,k] beside it, by attn_shared_merge_kernel's rule: r = 0
// (underflow) leaves u = 0, and h_a's own chain of sums is what it was
template <bool TRAIN>
__global__ __launch_bounds__(256) void attn_pool_merge_kernel(ShShape s, ShWork wk, float* __restrict__ h_a) {
  const int q = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x;
  if (c >= s.w) return;
  float v = 0.f;
  for (int k = 0; k < s.K; ++k) {
    float vk = 0.f;
    for (int m = 0; m < s.M; ++m) {
      const int slot = wk.qslot[(size_t)q * s.M + m];
      if (slot < 0) continue;  // (an empty slot: its rows are zero)
      const int grp = slot / s.G, g = slot % s.G;
      for (int sp = 0; sp < s.S; ++sp) {
        const float p = wk.part[((((size_t)grp * s.K + k) * s.S + sp) * s.G + g) * s.w + c];
        v += p;
        if constexpr (TRAIN) vk += p;
      }
    }
    if constexpr (TRAIN) {
      const float r = wk.r[(size_t)q * s.K + k];
      wk.u[((size_t)q * s.K + k) * s.w + c] = r > 0.f ? vk / r : 0.f;
    }
  }
  h_a[(size_t)q * s.w + c] = v;
}

// ---- scale[q,t] under the time warp, t = m JX + j over the question's WHOLE M JX positions.  grid (NQ, ceil(M JX / 256)),
// 256 threads.  attn_shared_tw_scale_kernel's arithmetic (s0, WC.lq, tanhf, tw_count: at M = 1 its bits) with the energy
// taken per slot: the album index clamped as the plan clamps it, an empty slot's e = 0 (JX zero rows)
__global__ __launch_bounds__(256) void attn_pool_tw_scale_kernel(ShShape s, int warp_type, int win, const float* __restrict__ energy,
                                                                 const float* __restrict__ lq, const int* __restrict__ albums,
                                                                 const float* __restrict__ WHb, const float* __restrict__ WC,
                                                                 const float* __restrict__ WCb, float* __restrict__ scale,
                                                                 float* __restrict__ scale_out) {
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
  const int m = t / s.T, a = sh_ref_album<true>(albums, q * s.M + m, s.A);
  const float e = a < 0 ? 0.f : energy[(size_t)a * s.T + (t - m * s.T)];
  const float tz = tanhf(e + (float)s.K * (s0 + sq));
  const float sc = tz * tw_count(t, s.TO, warp_type, win);
  scale[(size_t)q * s.TO + t] = sc;
  if (scale_out) scale_out[(size_t)q * s.TO + t] = sc;
}

// 0: fine, else the status with the message set
static int fvta_attn_pool_check(const fvta_attn_pool_desc* d, const char* who) {
  FVTA_CHECK_ARG(d != nullptr, "%s: null descriptor", who);
  FVTA_CHECK_ARG(d->P > 0 && d->NQ > 0 && d->M > 0 && d->K > 0 && d->JX > 0 && d->JQ > 0 && d->w > 0,
                 "%s: bad P/NQ/M/K/JX/JQ/w (%d,%d,%d,%d,%d,%d,%d)", who, d->P, d->NQ, d->M, d->K, d->JX, d->JQ, d->w);
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
  else if (d->P > (1 << 28) || (int64_t)d->NQ * d->M > (1 << 28))
    why = "P and NQ*M must not exceed 2^28";
  else if ((int64_t)d->M * d->JX > 0x7fffffff)
    why = "M*JX must fit a 32-bit int";
  if (!why) {
    const ShShape s = sh_pool_shape(d);
    if ((int64_t)s.ngmax * d->K * s.ntile > 0x7fffffff || (int64_t)s.ngmax * d->K * s.S > 0x7fffffff) why = "too many workgroups";
  }
  if (why) {
    fvta_set_error("%s: unsupported shape (P=%d NQ=%d M=%d K=%d JX=%d JQ=%d w=%d): %s", who, d->P, d->NQ, d->M, d->K, d->JX, d->JQ,
                   w, why);
    return FVTA_ERR_UNSUPPORTED;
  }
  return FVTA_OK;
}

// under the time warp: the shape, the warp type and window (attn_shared.hip's checks), M JX within the scale kernel's grid
static int fvta_attn_pool_check_tw(const fvta_attn_pool_tw_desc* d, const char* who) {
  FVTA_CHECK_ARG(d != nullptr, "%s: null descriptor", who);
  if (int e = fvta_attn_pool_check(&d->shape, who)) return e;
  if (int e = fvta_attn_shared_check_warp(d->warp_type, d->window_t, who)) return e;
  if ((int64_t)d->shape.M * d->shape.JX > 65535 * 256) {
    fvta_set_error("%s: unsupported shape (M=%d JX=%d): M*JX must not exceed 65535 * 256 under the time warp", who, d->shape.M,
                   d->shape.JX);
    return FVTA_ERR_UNSUPPORTED;
  }
  if (((int64_t)d->shape.P * d->shape.JX + 3) / 4 > 0x7fffffff) {
    fvta_set_error("%s: unsupported shape (P=%d JX=%d): too many workgroups", who, d->shape.P, d->shape.JX);
    return FVTA_ERR_UNSUPPORTED;
  }
  return FVTA_OK;
}

// the workspace under the warp: fvta_attn_pool_fwd's, then scale [NQ,M JX], then v [w] (the energy call's)
struct PoolTwWork {
  ShWork wk;
  float *scale, *v;
  size_t bytes;
  PoolTwWork(const ShShape& s, void* p) : wk(s, p) {
    FvtaCarver c(p);
    c.off = wk.bytes;
    scale = c.take<float>((size_t)s.NQ * s.TO);
    v = c.take<float>((size_t)s.w);
    bytes = c.off;
  }
};

}  // namespace fvta
using namespace fvta;

extern "C" size_t fvta_attn_pool_workspace_bytes(const fvta_attn_pool_desc* d) {
  if (fvta_attn_pool_check(d, "attn_pool_workspace_bytes") != FVTA_OK) return 0;
  return ShWork(sh_pool_shape(d), nullptr).bytes;
}

extern "C" int fvta_attn_pool_plan(const fvta_attn_pool_desc* d, int32_t out[4]) {
  if (int e = fvta_attn_pool_check(d, "attn_pool_plan")) return e;
  FVTA_CHECK_ARG(out != nullptr, "attn_pool_plan: null pointer");
  const ShShape s = sh_pool_shape(d);
  out[0] = s.G;
  out[1] = SH_R;
  out[2] = s.S;
  out[3] = s.rps;
  return FVTA_OK;
}

// the eight launches; TW: under the time warp, tw_scale [NQ,M JX] written by an earlier launch on the same stream;
// TRAIN: the ordered plan, the arg-max, L / r / u, wk carved from (saved, workspace)
template <bool TW, bool TRAIN = false>
static int pool_forward(ShShape s, const ShWork& wk, const float* pool, const uint8_t* pool_mask, const float* hq,
                        const uint8_t* qmask, const int32_t* albums, const float* W, const float* b, float* h_a, float* a_logits,
                        hipStream_t st, const float* tw_scale, const char* who) {
  s.use_mask = (pool_mask && qmask) ? 1 : 0;  // model_v2.py:233: the mask applies only when both are given
  hipLaunchKernelGGL(attn_vecs_kernel, dim3((s.w + 255) / 256), dim3(256), 0, st, W, s.w, s.simi, 0, wk.vecs);
  hipLaunchKernelGGL(attn_shared_prep_q_kernel, dim3(s.NQ, s.JP / 4), dim3(256), 0, st, s, wk, hq, b);
  static_assert(!(TW && TRAIN), "training over the pool is not under the time warp");
  hipLaunchKernelGGL((attn_shared_plan_kernel<TRAIN, true>), dim3(1), dim3(SH_PLAN_NT), 0, st, s, wk, (const int*)albums);
  const dim3 lgrid((unsigned)((int64_t)s.ngmax * s.K * s.ntile));
  const ShTwArgs tw{tw_scale, nullptr, nullptr};
  if (s.JP == 32)
    hipLaunchKernelGGL((attn_shared_logits_kernel<1, TRAIN, TW, true>), lgrid, dim3(SH_NT), 0, st, s, wk, pool, pool_mask, qmask,
                       a_logits, tw);
  else
    hipLaunchKernelGGL((attn_shared_logits_kernel<2, TRAIN, TW, true>), lgrid, dim3(SH_NT), 0, st, s, wk, pool, pool_mask, qmask,
                       a_logits, tw);
  hipLaunchKernelGGL(attn_pool_empty_kernel<TRAIN>, dim3(s.NR), dim3(256), 0, st, s, wk, (const int*)albums, a_logits);
  ShShape sq = s;  // the softmaxes run per question over all of its positions
  sq.T = s.TO;
  hipLaunchKernelGGL(attn_shared_softmax_kernel, dim3(s.NQ), dim3(256), 0, st, sq, wk);
  if (s.G == 8)
    sh_launch_wsum<8, TW, true>(s, wk, pool, tw_scale, st);
  else
    sh_launch_wsum<4, TW, true>(s, wk, pool, tw_scale, st);
  hipLaunchKernelGGL(attn_pool_merge_kernel<TRAIN>, dim3(s.NQ, (s.w + 255) / 256), dim3(256), 0, st, s, wk, h_a);
  FVTA_CHECK_LAUNCH(who);
  return FVTA_OK;
}

extern "C" int fvta_attn_pool_fwd(const fvta_attn_pool_desc* d, const float* pool, const uint8_t* pool_mask, const float* hq,
                                  const uint8_t* qmask, const int32_t* albums, const float* W, const float* b, float* h_a,
                                  float* a_logits, void* workspace, fvta_stream_t stream_) {
  if (int e = fvta_attn_pool_check(d, "attn_pool_fwd")) return e;
  FVTA_CHECK_ARG(pool && hq && albums && h_a && workspace, "attn_pool_fwd: null pointer");
  FVTA_CHECK_ARG(d->simi == 4 || W, "attn_pool_fwd: simiMatrix %d needs att_logits/W", d->simi);
  const ShShape s = sh_pool_shape(d);
  return pool_forward<false>(s, ShWork(s, workspace), pool, pool_mask, hq, qmask, albums, W, b, h_a, a_logits, (hipStream_t)stream_,
                             nullptr, "attn_pool_fwd");
}

// ---- under the time warp
extern "C" size_t fvta_attn_pool_tw_workspace_bytes(const fvta_attn_pool_tw_desc* d) {
  if (fvta_attn_pool_check_tw(d, "attn_pool_tw_workspace_bytes") != FVTA_OK) return 0;
  return PoolTwWork(sh_pool_shape(&d->shape), nullptr).bytes;
}

extern "C" int fvta_attn_pool_energy(const fvta_attn_pool_tw_desc* d, const float* pool, const float* WH_W, const float* WC_W,
                                     float* energy, void* workspace, fvta_stream_t stream_) {
  if (int e = fvta_attn_pool_check_tw(d, "attn_pool_energy")) return e;
  FVTA_CHECK_ARG(pool && WH_W && WC_W && energy && workspace, "attn_pool_energy: null pointer");
  const ShShape s = sh_pool_shape(&d->shape);  // (A = P, T = JX: the energy of a pooled album's own rows)
  const PoolTwWork tw(s, workspace);
  hipStream_t st = (hipStream_t)stream_;
  hipLaunchKernelGGL(attn_shared_tw_vec_kernel, dim3((s.w + 3) / 4), dim3(256), 0, st, s.w, WH_W, WC_W, tw.v);
  hipLaunchKernelGGL(attn_shared_energy_kernel, dim3((unsigned)(((int64_t)s.A * s.T + 3) / 4)), dim3(256), 0, st, s, pool, tw.v,
                     energy);
  FVTA_CHECK_LAUNCH("attn_pool_energy");
  return FVTA_OK;
}

extern "C" int fvta_attn_pool_fwd_tw(const fvta_attn_pool_tw_desc* d, const float* pool, const uint8_t* pool_mask,
                                     const float* energy, const float* hq, const uint8_t* qmask, const float* lq,
                                     const int32_t* albums, const float* W, const float* b, const float* WH_b, const float* WC_W,
                                     const float* WC_b, float* h_a, float* a_logits, float* scale_out, void* workspace,
                                     fvta_stream_t stream_) {
  if (int e = fvta_attn_pool_check_tw(d, "attn_pool_fwd_tw")) return e;
  FVTA_CHECK_ARG(pool && energy && hq && lq && albums && WH_b && WC_W && WC_b && h_a && workspace, "attn_pool_fwd_tw: null pointer");
  FVTA_CHECK_ARG(d->shape.simi == 4 || W, "attn_pool_fwd_tw: simiMatrix %d needs att_logits/W", d->shape.simi);
  const ShShape s = sh_pool_shape(&d->shape);
  const PoolTwWork tw(s, workspace);
  hipStream_t st = (hipStream_t)stream_;
  hipLaunchKernelGGL(attn_pool_tw_scale_kernel, dim3(s.NQ, (s.TO + 255) / 256), dim3(256), 0, st, s, d->warp_type,
                     (int)ceilf(d->window_t), energy, lq, (const int*)albums, WH_b, WC_W, WC_b, tw.scale, scale_out);
  return pool_forward<true>(s, tw.wk, pool, pool_mask, hq, qmask, albums, W, b, h_a, a_logits, st, tw.scale, "attn_pool_fwd_tw");
}

// ================= training over the pool (fvta_attn_pool_fwd_train / fvta_attn_pool_bwd) ================================
// The forward is pool_forward<false, true>: the launches above on the training ShWork -- the ordered plan (an album's
// references by ascending id q M + m), the arg-max at the reference's slot, L / r / u -- with what the backward reads in
// `saved`.  h_a and a_logits are fvta_attn_pool_fwd's bits: the placement of a reference changes none.
// The backward is attn_shared_bwd.hip's five launches with the album's questions replaced by the album's references
// (attn_shared_bwd_kernels.h, POOL = true), and one small kernel in front of the fold:
//   1. attn_shared_bwd_prep_kernel            per question over its M JX positions
//   2. attn_shared_bwd_rows_kernel<.., POOL>  per (pooled album, k, chunk of row tiles): the album's references in plan
//                                             order; dx -> [NQ,K,M JX] at the reference's slot; every d_pool row stored once
//   3. attn_shared_bwd_q_kernel<G, ., POOL>   a lane group per reference; partials per (group, split)
//   3b. attn_pool_bwd_dct_kernel              d ct[q] = its non-empty slots' partials in (slot, split) order -> dctq [NQ,JP]
//   4. attn_pool_bwd_fold_kernel              attn_bwd_fold_body with dQs[q,j] summed the same way (slot ascending, then
//                                             split) and d ct taken from dctq as ONE slot; a question without a reference
//                                             sums nothing: d_hq = exact zeros
//   5. attn_shared_bwd_params_kernel          as it is: pvec per (question, 8 positions), rowp per row-pass workgroup
// Determinism: as attn_shared_bwd.hip.  The one sum whose order depends on data -- d_pool over an album's references --
// runs in `order`, a function of `albums` alone.  At M = 1 every launch computes what fvta_attn_shared_bwd's does (a sum
// over one slot starts from 0 + x): the same bits.
namespace fvta {

// the backward's workspace: attn_shared_bwd.hip's for the pooled shape, then dctq [NQ,JP]
struct PoolBwdWork {
  ShBwdWork base;
  float* dctq;
  size_t bytes;
  PoolBwdWork(const ShShape& s, const ShBwdShape& b, void* p) : base(s, b, p) {
    FvtaCarver c(p);
    c.off = base.bytes;
    dctq = c.take<float>((size_t)s.NQ * s.JP);
    bytes = c.off;
  }
};

// slot of reference (q, m) in the partials, -1 for an empty slot; the plan's own number, bounded all the same
__device__ __forceinline__ int pool_ref_slot(const ShShape& s, const ShWork& sv, int q, int m) {
  const int slot = sv.qslot[(size_t)q * s.M + m];
  return slot < 0 ? -1 : min(slot, s.ngmax * s.G - 1);
}

// acc += ld(0), += ld(1), ... in that order, eight loads in flight (attn_bwd_slot_sum's chain, continued across slots)
template <class V, class LD>
__device__ __forceinline__ void pool_slot_add(V& acc, int n, LD ld) {
  int i = 0;
  for (; i + 8 <= n; i += 8) {
    V v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = ld(i + u);
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += v[u];
  }
  for (; i < n; ++i) acc += ld(i);
}

// ---- 3b.  grid NQ, 64 threads: thread j < JP
__global__ __launch_bounds__(64) void attn_pool_bwd_dct_kernel(ShShape s, ShBwdShape bs, ShWork sv, ShBwdWork wk,
                                                              float* __restrict__ dctq) {
  const int q = blockIdx.x, j = threadIdx.x;
  if (j >= s.JP) return;
  float acc = 0.f;
  for (int m = 0; m < s.M; ++m) {
    const int slot = pool_ref_slot(s, sv, q, m);
    if (slot < 0) continue;
    const size_t row0 = (size_t)(slot / s.G) * bs.TS * SH_BN + (size_t)(slot % s.G) * s.JP + j;
    pool_slot_add(acc, bs.TS, [&](int ts) { return wk.dctp[row0 + (size_t)ts * SH_BN]; });
  }
  dctq[(size_t)q * s.JP + j] = acc;
}

// ---- 4.  grid (NQ, ceil(w / 256), JZ), 256 threads
__global__ __launch_bounds__(256) void attn_pool_bwd_fold_kernel(ShShape s, ShBwdShape bs, ShWork sv, ShBwdWork wk,
                                                                const float* __restrict__ dctq, const float* __restrict__ hq,
                                                                float* __restrict__ d_hq) {
  const int q = blockIdx.x, c = blockIdx.y * 256 + 4 * (threadIdx.x & 63);
  const int w = s.w, JP = s.JP, JQ = s.JQ, TS = bs.TS;
  const bool live = c < w;
  f32x4 pU, pCq, pC2;
  if (!attn_bwd_fold_body(sv.vecs, hq + (size_t)q * JQ * w, d_hq + (size_t)q * JQ * w, false, dctq + (size_t)q * JP, (size_t)0, 1,
                          wk.dctn + (size_t)q * JP, w, JP, JQ,
                          [&](int j) {
                            f32x4 acc = zero4();
                            for (int m = 0; m < s.M; ++m) {
                              const int slot = pool_ref_slot(s, sv, q, m);
                              if (slot < 0) continue;
                              const size_t row0 = (size_t)(slot / s.G) * TS * SH_BN + (size_t)(slot % s.G) * JP + j;
                              pool_slot_add(acc, TS, [&](int ts) { return ld4_if(live, wk.qpart + (row0 + (size_t)ts * SH_BN) * w + c); });
                            }
                            return acc;
                          },
                          pU, pCq, pC2))
    return;
  float* pv = wk.pvec + ((size_t)q * bs.JZ + blockIdx.z) * 3 * w;
  *reinterpret_cast<f32x4*>(pv + c) = pU;
  *reinterpret_cast<f32x4*>(pv + w + c) = pCq;
  *reinterpret_cast<f32x4*>(pv + 2 * w + c) = pC2;
}

// training: the shape, simiMatrix 1-3, the backward's grids
static int fvta_attn_pool_check_train(const fvta_attn_pool_desc* d, const char* who) {
  if (int e = fvta_attn_pool_check(d, who)) return e;
  if (d->simi == 4) {
    fvta_set_error("%s: simiMatrix 4 has no pooled backward (simiMatrix 1-3); the per-question route "
                   "(fvta_attn_fwd / fvta_attn_bwd on the gathered rows) covers it", who);
    return FVTA_ERR_UNSUPPORTED;
  }
  const ShShape s = sh_pool_shape(d);
  const ShBwdShape b = shb_shape(s);
  if ((int64_t)s.A * s.K * b.nch > 0x7fffffff || (int64_t)s.ngmax * b.TS * b.nsl > 0x7fffffff) {
    fvta_set_error("%s: unsupported shape (P=%d NQ=%d M=%d K=%d JX=%d JQ=%d w=%d): too many workgroups", who, d->P, d->NQ, d->M,
                   d->K, d->JX, d->JQ, d->w);
    return FVTA_ERR_UNSUPPORTED;
  }
  return FVTA_OK;
}

}  // namespace fvta

extern "C" size_t fvta_attn_pool_saved_bytes(const fvta_attn_pool_desc* d) {
  if (fvta_attn_pool_check_train(d, "attn_pool_saved_bytes") != FVTA_OK) return 0;
  return ShWork(sh_pool_shape(d), nullptr, nullptr).saved_bytes;
}

extern "C" int fvta_attn_pool_fwd_train(const fvta_attn_pool_desc* d, const float* pool, const uint8_t* pool_mask, const float* hq,
                                        const uint8_t* qmask, const int32_t* albums, const float* W, const float* b, float* h_a,
                                        float* a_logits, void* saved, void* workspace, fvta_stream_t stream_) {
  if (int e = fvta_attn_pool_check_train(d, "attn_pool_fwd_train")) return e;
  FVTA_CHECK_ARG(pool && hq && albums && W && h_a && saved && workspace, "attn_pool_fwd_train: null pointer");
  const ShShape s = sh_pool_shape(d);  // (the training ShWork's share of the workspace is no larger than the inference call's)
  return pool_forward<false, true>(s, ShWork(s, saved, workspace), pool, pool_mask, hq, qmask, albums, W, b, h_a, a_logits,
                                   (hipStream_t)stream_, nullptr, "attn_pool_fwd_train");
}

extern "C" size_t fvta_attn_pool_bwd_workspace_bytes(const fvta_attn_pool_desc* d) {
  if (fvta_attn_pool_check_train(d, "attn_pool_bwd_workspace_bytes") != FVTA_OK) return 0;
  const ShShape s = sh_pool_shape(d);
  return PoolBwdWork(s, shb_shape(s), nullptr).bytes;
}

extern "C" int fvta_attn_pool_bwd_plan(const fvta_attn_pool_desc* d, int32_t out[4]) {
  if (int e = fvta_attn_pool_check_train(d, "attn_pool_bwd_plan")) return e;
  FVTA_CHECK_ARG(out != nullptr, "attn_pool_bwd_plan: null pointer");
  const ShBwdShape b = shb_shape(sh_pool_shape(d));
  out[0] = b.TR;
  out[1] = b.TS;
  out[2] = SHB_CS;
  out[3] = b.tpw;
  return FVTA_OK;
}

extern "C" int fvta_attn_pool_bwd(const fvta_attn_pool_desc* d, const float* pool, const uint8_t* pool_mask, const float* hq,
                                  const uint8_t* qmask, const int32_t* albums, const float* W, const float* b, const float* d_h_a,
                                  const void* saved, float* d_pool, float* d_hq, float* dW, float* db, void* workspace,
                                  fvta_stream_t stream_) {
  if (int e = fvta_attn_pool_check_train(d, "attn_pool_bwd")) return e;
  FVTA_CHECK_ARG(pool && hq && albums && d_h_a && saved && d_pool && d_hq && dW && db && workspace, "attn_pool_bwd: null pointer");
  hipStream_t st = (hipStream_t)stream_;
  ShShape s = sh_pool_shape(d);
  s.use_mask = (pool_mask && qmask) ? 1 : 0;
  const ShBwdShape bs = shb_shape(s);
  const ShWork sv(s, const_cast<void*>(saved), nullptr);
  const PoolBwdWork pw(s, bs, workspace);
  const ShBwdWork& wk = pw.base;
  ShShape sq = s;  // the prep runs per question over all of its positions
  sq.T = s.TO;
  hipLaunchKernelGGL(attn_shared_bwd_prep_kernel, dim3(s.NQ), dim3(s.K > 4 ? 1024 : 256), 0, st, sq, sv, wk, d_h_a);
  const dim3 rgrid((unsigned)((int64_t)s.A * s.K * bs.nch));
#define FVTA_POOL_ROWS(TPR, CPT, RPT) \
  hipLaunchKernelGGL((attn_shared_bwd_rows_kernel<TPR, CPT, RPT, false, true>), rgrid, dim3(256), 0, st, s, bs, sv, wk, pool, d_h_a, \
                     d_pool, ShBwdTwArgs{})
  switch (s.w) {
    case 64: FVTA_POOL_ROWS(16, 1, 8); break;
    case 128: FVTA_POOL_ROWS(32, 1, 8); break;
    case 256: FVTA_POOL_ROWS(64, 1, 8); break;
    case 512: FVTA_POOL_ROWS(128, 1, 8); break;
    case 1024: FVTA_POOL_ROWS(256, 1, 8); break;
    default: FVTA_POOL_ROWS(256, 2, 4); break;
  }
#undef FVTA_POOL_ROWS
  const dim3 qgrid((unsigned)((int64_t)s.ngmax * bs.TS * bs.nsl));
  if (s.G == 8)
    hipLaunchKernelGGL((attn_shared_bwd_q_kernel<8, false, true>), qgrid, dim3(64), 0, st, s, bs, sv, wk, pool, (const float*)nullptr);
  else
    hipLaunchKernelGGL((attn_shared_bwd_q_kernel<4, false, true>), qgrid, dim3(64), 0, st, s, bs, sv, wk, pool, (const float*)nullptr);
  hipLaunchKernelGGL(attn_pool_bwd_dct_kernel, dim3(s.NQ), dim3(64), 0, st, s, bs, sv, wk, pw.dctq);
  hipLaunchKernelGGL(attn_pool_bwd_fold_kernel, dim3(s.NQ, (s.w + 255) / 256, bs.JZ), dim3(256), 0, st, s, bs, sv, wk,
                     (const float*)pw.dctq, hq, d_hq);
  hipLaunchKernelGGL(attn_shared_bwd_params_kernel, dim3((s.w + 63) / 64 + 1), dim3(256), 0, st, s, bs, wk, dW, db);
  FVTA_CHECK_LAUNCH("attn_pool_bwd");
  return FVTA_OK;
}

// Focal attention over PER-QUESTION ALBUM LISTS FROM ONE ALBUM POOL (fvta_attn_pool_fwd): pool [P,K,JX,w] holds every
// encoded album once, question i lists M of them (albums [NQ,M]; a negative entry is an empty slot), and its context is
// those albums laid end to end: hinfo_i[k, m JX + j] = pool[albums[i,m], k, j], T = M JX (model_v2.py:863-914 builds that
// tensor per question; the encoders run per (question, album), :704-760, so an album's rows do not depend on its
// neighbours).  Per question the result is fvta_attn_fwd's on (hinfo_i, hq[i]) -- model_v2.py:210-298 -- and no
// [NQ,K,T,w] tensor exists.  Inference only: nothing is kept for a backward.
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
#include "attn_shared_kernels.h"

namespace fvta {

// ---- empty slots.  grid NQ M, 256 threads: a workgroup per reference, gone at once unless its slot is empty
__global__ __launch_bounds__(256) void attn_pool_empty_kernel(ShShape s, ShWork wk, const int* __restrict__ albums,
                                                              float* __restrict__ a_logits) {
  const int ref = blockIdx.x;
  if (albums[ref] >= 0) return;
  const int q = ref / s.M, off = (ref % s.M) * s.T;
  for (int k = 0; k < s.K; ++k) {
    const size_t at = ((size_t)q * s.K + k) * s.TO + off;
    for (int e = threadIdx.x; e < s.T; e += 256) wk.amax[at + e] = FVTA_NEG;
    if (a_logits)
      for (int64_t e = threadIdx.x; e < (int64_t)s.T * s.JQ; e += 256) a_logits[at * s.JQ + e] = FVTA_NEG;
  }
}

// ---- merge.  grid (NQ, ceil(w / 256)): a channel per thread, the partials in (k, slot, split) order
__global__ __launch_bounds__(256) void attn_pool_merge_kernel(ShShape s, ShWork wk, float* __restrict__ h_a) {
  const int q = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x;
  if (c >= s.w) return;
  float v = 0.f;
  for (int k = 0; k < s.K; ++k)
    for (int m = 0; m < s.M; ++m) {
      const int slot = wk.qslot[(size_t)q * s.M + m];
      if (slot < 0) continue;  // (an empty slot: its rows are zero)
      const int grp = slot / s.G, g = slot % s.G;
      for (int sp = 0; sp < s.S; ++sp) v += wk.part[((((size_t)grp * s.K + k) * s.S + sp) * s.G + g) * s.w + c];
    }
  h_a[(size_t)q * s.w + c] = v;
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

extern "C" int fvta_attn_pool_fwd(const fvta_attn_pool_desc* d, const float* pool, const uint8_t* pool_mask, const float* hq,
                                  const uint8_t* qmask, const int32_t* albums, const float* W, const float* b, float* h_a,
                                  float* a_logits, void* workspace, fvta_stream_t stream_) {
  if (int e = fvta_attn_pool_check(d, "attn_pool_fwd")) return e;
  FVTA_CHECK_ARG(pool && hq && albums && h_a && workspace, "attn_pool_fwd: null pointer");
  FVTA_CHECK_ARG(d->simi == 4 || W, "attn_pool_fwd: simiMatrix %d needs att_logits/W", d->simi);
  ShShape s = sh_pool_shape(d);
  s.use_mask = (pool_mask && qmask) ? 1 : 0;  // model_v2.py:233: the mask applies only when both are given
  const ShWork wk(s, workspace);
  hipStream_t st = (hipStream_t)stream_;
  hipLaunchKernelGGL(attn_vecs_kernel, dim3((s.w + 255) / 256), dim3(256), 0, st, W, s.w, s.simi, 0, wk.vecs);
  hipLaunchKernelGGL(attn_shared_prep_q_kernel, dim3(s.NQ, s.JP / 4), dim3(256), 0, st, s, wk, hq, b);
  hipLaunchKernelGGL((attn_shared_plan_kernel<false, true>), dim3(1), dim3(SH_PLAN_NT), 0, st, s, wk, (const int*)albums);
  const dim3 lgrid((unsigned)((int64_t)s.ngmax * s.K * s.ntile));
  const ShTwArgs tw{nullptr, nullptr, nullptr};
  if (s.JP == 32)
    hipLaunchKernelGGL((attn_shared_logits_kernel<1, false, false, true>), lgrid, dim3(SH_NT), 0, st, s, wk, pool, pool_mask, qmask,
                       a_logits, tw);
  else
    hipLaunchKernelGGL((attn_shared_logits_kernel<2, false, false, true>), lgrid, dim3(SH_NT), 0, st, s, wk, pool, pool_mask, qmask,
                       a_logits, tw);
  hipLaunchKernelGGL(attn_pool_empty_kernel, dim3(s.NR), dim3(256), 0, st, s, wk, (const int*)albums, a_logits);
  ShShape sq = s;  // the softmaxes run per question over all of its positions
  sq.T = s.TO;
  hipLaunchKernelGGL(attn_shared_softmax_kernel, dim3(s.NQ), dim3(256), 0, st, sq, wk);
  if (s.G == 8)
    sh_launch_wsum<8, false, true>(s, wk, pool, nullptr, st);
  else
    sh_launch_wsum<4, false, true>(s, wk, pool, nullptr, st);
  hipLaunchKernelGGL(attn_pool_merge_kernel, dim3(s.NQ, (s.w + 255) / 256), dim3(256), 0, st, s, wk, h_a);
  FVTA_CHECK_LAUNCH("attn_pool_fwd");
  return FVTA_OK;
}

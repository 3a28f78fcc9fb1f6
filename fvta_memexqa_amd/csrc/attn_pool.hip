// Focal attention over PER-QUESTION ALBUM LISTS FROM ONE ALBUM POOL (fvta_attn_pool_fwd): pool [P,K,JX,w] holds every
// encoded album once, question i lists M of them (albums [NQ,M]; a negative entry is an empty slot), and its context is
// those albums laid end to end: hinfo_i[k, m JX + j] = pool[albums[i,m], k, j], T = M JX (model_v2.py:863-914 builds that
// tensor per question; the encoders run per (question, album), :704-760, so an album's rows do not depend on its
// neighbours).  Per question the result is fvta_attn_fwd's on (hinfo_i, hq[i]) -- model_v2.py:210-298 -- and no
// [NQ,K,T,w] tensor exists.  fvta_attn_pool_fwd keeps nothing for a backward; the training pair (fvta_attn_pool_fwd_train /
// fvta_attn_pool_bwd) is at the end of this file.
//
// The launches are attn_shared.hip's seven -- its forward driver, sh_forward with pool = true: the launch sequence is
// documented there -- with one change of meaning: a column block of a group's product stands for a REFERENCE (question q,
// slot m), id q M + m, instead of a question (attn_shared_kernels.h, POOL = true):
//   1. attn_vecs_kernel, 2. attn_shared_prep_q_kernel   as they are: Qs and ct belong to the question
//   3. attn_shared_plan_kernel<., true>       counting sort of the NQ M references by pooled album, empty slots passed
//                                             over (qslot = -1); groups of <= G references of ONE album
//   4. attn_shared_logits_kernel<JT, ., ., true>   per (group, k, tile of SH_R of the album's JX rows): block g reads
//                                             its reference's question's Qs / ct / qmask, writes amax and a_logits at
//                                             positions m JX + row of that question
//      attn_pool_empty_kernel                 an empty slot's JX positions: amax = -1e30 for every k (a_logits too): no
//                                             product, no row read
//   5. attn_shared_softmax_kernel             per question over its T = M JX positions
//   6. attn_shared_wsum_kernel<G, CPT, ., true>   per (group, k, split of JX): one partial per reference from one read
//                                             of each row
//   7. attn_shared_merge_kernel<., true>      h_a[q] = its references' partials in (k, slot, split) order, empty slots
//                                             passed over
// Row traffic: a pooled album's rows are read twice per group of <= G references to it, however many distinct lists there
// are; an album nobody lists is never read.  Determinism: as attn_shared.hip -- no floating-point atomics, the splits
// depend on the descriptor only, a reference's numbers do not depend on its group, block or wave.  At M = 1 every launch
// computes what attn_shared.hip's does: the same bits.
//
// Under the time warp (fvta_attn_pool_fwd_tw): the warp is one scalar per (question, position of its M JX), so the rows
// stay pooled.  attn_shared_tw_scale_kernel<., true> goes in front and writes scale [NQ,M JX] from energy [P,JX] (a pooled
// album's, fvta_attn_pool_energy: attn_shared.hip's two energy launches with A = P, T = JX) and the count of the GLOBAL
// position t = m JX + j; (4) and (6) are the <TW, POOL> instantiations, which read the scale at the reference's slot.  At
// M = 1 every launch computes what fvta_attn_shared_fwd_tw's does: the same bits.  Training under the warp
// (fvta_attn_pool_fwd_tw_train / fvta_attn_pool_bwd_tw): further down, after the unwarped training pair.
//
// This file holds the pooled descriptor's entry points -- thin calls of attn_shared.hip's and attn_shared_bwd.hip's checks
// and drivers -- and the two kernels of the backward that only the pool has.
#include "attn_shared_kernels.h"
#include "attn_shared_bwd_kernels.h"

// ================= training over the pool (fvta_attn_pool_fwd_train / fvta_attn_pool_bwd) ================================
// The forward is sh_forward's <TRAIN, ., POOL>: the launches above on the training ShWork -- the ordered plan (an album's
// references by ascending id q M + m), the arg-max at the reference's slot, L / r / u -- with what the backward reads in
// `saved`.  h_a and a_logits are fvta_attn_pool_fwd's bits: the placement of a reference changes none.
// The backward is attn_shared_bwd.hip's five launches (its driver, shb_backward with pool = true) with the album's
// questions replaced by the album's references (attn_shared_bwd_kernels.h, POOL = true), and one small kernel in front of
// the fold:
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
//
// ================= training over the pool under the time warp (fvta_attn_pool_fwd_tw_train / fvta_attn_pool_bwd_tw) ======
// The contract of fvta_attn_shared_fwd_tw_train / fvta_attn_shared_bwd_tw over the pooled descriptor.  The forward is
// sh_forward's <TRAIN, TW, POOL>: `saved` takes the training ShWork's share, then scale / tanh(z) [NQ,M JX], lin
// [NQ,K,M JX] at the reference's slot, r2 [P,K,JX] at the album's own row.  The backward is shb_backward's <TW, POOL>:
//   1. prep over M JX;  a. attn_shared_tw_vec_kernel;  2., 3. the <TW, POOL> row and question passes: ds / dx s / dbt
//      [NQ,K,M JX] at the reference's slot
//   b. attn_shared_bwd_tw_dz_kernel<POOL>   per question over its M JX positions, the count at the GLOBAL position
//                                           m JX + j; an empty slot's positions: dz = 0, nothing into dbq, by the slot's
//                                           own word (qslot < 0) -- no row pass wrote their ds, and zero is their value
//   c. attn_shared_bwd_tw_de_kernel<POOL>   de[p,j] = sum of dz[q, m JX + j] over album p's references in plan order
//   d. attn_shared_bwd_tw_energy_kernel     over [P,JX]: d_pool += 2 de v h; an album nobody lists is skipped
//   3b., 4. the pooled dct and fold;  5. parameters with db left to (e);  e., f. the warp's parameter kernels
// d_pool holds the attention's row gradient and the energy's term, both summed over every (question, slot) reference in
// plan order.  No [NQ,K,M JX,w] tensor, no floating-point atomics, no memset, no host wait; at M = 1 the bits of the
// shared warped pair, `saved` included.
namespace fvta {

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

}  // namespace fvta
using namespace fvta;

// ---- the entry points: the pooled descriptor through the one ladder of checks (attn_shared.hip: sh_check, with this
// family's letters P/NQ/M/K/JX/JQ/w in every refusal), then attn_shared.hip's helpers and driver with pool = true
extern "C" size_t fvta_attn_pool_workspace_bytes(const fvta_attn_pool_desc* d) {
  ShShape s;
  return sh_open(d, "attn_pool_workspace_bytes", s) == FVTA_OK ? ShWork(s, nullptr).bytes : 0;
}

extern "C" int fvta_attn_pool_plan(const fvta_attn_pool_desc* d, int32_t out[4]) {
  ShShape s;
  if (int e = sh_open(d, "attn_pool_plan", s)) return e;
  return sh_plan(s, "attn_pool_plan", out);
}

extern "C" int fvta_attn_pool_fwd(const fvta_attn_pool_desc* d, const float* pool, const uint8_t* pool_mask, const float* hq,
                                  const uint8_t* qmask, const int32_t* albums, const float* W, const float* b, float* h_a,
                                  float* a_logits, void* workspace, fvta_stream_t stream_) {
  ShShape s;
  if (int e = sh_open(d, "attn_pool_fwd", s)) return e;
  FVTA_CHECK_ARG(pool && hq && albums && h_a && workspace, "attn_pool_fwd: null pointer");
  FVTA_CHECK_ARG(d->simi == 4 || W, "attn_pool_fwd: simiMatrix %d needs att_logits/W", d->simi);
  return sh_forward(s, true, "attn_pool_fwd", {pool, pool_mask, hq, qmask, albums, W, b, h_a, a_logits, nullptr, workspace, stream_});
}

// ---- under the time warp.  The workspace: ShTwWork (attn_shared_common.h) with scale [NQ,M JX]
extern "C" size_t fvta_attn_pool_tw_workspace_bytes(const fvta_attn_pool_tw_desc* d) {
  ShShape s;
  return sh_open_tw(d, "attn_pool_tw_workspace_bytes", s) == FVTA_OK ? ShTwWork(s, nullptr).bytes : 0;
}

extern "C" int fvta_attn_pool_energy(const fvta_attn_pool_tw_desc* d, const float* pool, const float* WH_W, const float* WC_W,
                                     float* energy, void* workspace, fvta_stream_t stream_) {
  ShShape s;  // (A = P, T = JX: the energy of a pooled album's own rows)
  if (int e = sh_open_tw(d, "attn_pool_energy", s)) return e;
  return sh_energy(s, "attn_pool_energy", pool, WH_W, WC_W, energy, workspace, stream_);
}

extern "C" int fvta_attn_pool_fwd_tw(const fvta_attn_pool_tw_desc* d, const float* pool, const uint8_t* pool_mask,
                                     const float* energy, const float* hq, const uint8_t* qmask, const float* lq,
                                     const int32_t* albums, const float* W, const float* b, const float* WH_b, const float* WC_W,
                                     const float* WC_b, float* h_a, float* a_logits, float* scale_out, void* workspace,
                                     fvta_stream_t stream_) {
  ShShape s;
  if (int e = sh_open_tw(d, "attn_pool_fwd_tw", s)) return e;
  FVTA_CHECK_ARG(pool && energy && hq && lq && albums && WH_b && WC_W && WC_b && h_a && workspace, "attn_pool_fwd_tw: null pointer");
  FVTA_CHECK_ARG(d->shape.simi == 4 || W, "attn_pool_fwd_tw: simiMatrix %d needs att_logits/W", d->shape.simi);
  const ShWarpCall warp{d->warp_type, d->window_t, energy, lq, WH_b, WC_W, WC_b, scale_out};
  return sh_forward(s, true, "attn_pool_fwd_tw", {pool, pool_mask, hq, qmask, albums, W, b, h_a, a_logits, nullptr, workspace, stream_},
                    &warp);
}

// ---- the pool held in bf16 (raw bits; torch.bfloat16), inference only: the three calls above through the same checks,
// helpers and driver, with the rows' pointer in ShFwdCall::rows_bf16 / sh_energy's last argument -- the ROW = bf16_t
// instantiations of the three kernels that read rows (attn_shared_kernels.h).  Those load four bf16 where the fp32 kernels
// load four floats and widen them in registers, which is exact, and every lane keeps its channels: the results are the
// fp32 calls' on the widened pool, bit for bit.  Same launches, same workspace (the fp32 size queries serve)
static int pool_bf16_aligned(const uint16_t* pool, const char* who) {
  FVTA_CHECK_ARG(((uintptr_t)pool & 7) == 0, "%s: the bf16 pool must be 8-byte aligned", who);
  return FVTA_OK;
}

extern "C" int fvta_attn_pool_fwd_bf16(const fvta_attn_pool_desc* d, const uint16_t* pool, const uint8_t* pool_mask, const float* hq,
                                       const uint8_t* qmask, const int32_t* albums, const float* W, const float* b, float* h_a,
                                       float* a_logits, void* workspace, fvta_stream_t stream_) {
  ShShape s;
  if (int e = sh_open(d, "attn_pool_fwd_bf16", s)) return e;
  FVTA_CHECK_ARG(pool && hq && albums && h_a && workspace, "attn_pool_fwd_bf16: null pointer");
  FVTA_CHECK_ARG(d->simi == 4 || W, "attn_pool_fwd_bf16: simiMatrix %d needs att_logits/W", d->simi);
  if (int e = pool_bf16_aligned(pool, "attn_pool_fwd_bf16")) return e;
  return sh_forward(s, true, "attn_pool_fwd_bf16",
                    {nullptr, pool_mask, hq, qmask, albums, W, b, h_a, a_logits, nullptr, workspace, stream_, pool});
}

extern "C" int fvta_attn_pool_energy_bf16(const fvta_attn_pool_tw_desc* d, const uint16_t* pool, const float* WH_W, const float* WC_W,
                                          float* energy, void* workspace, fvta_stream_t stream_) {
  ShShape s;
  if (int e = sh_open_tw(d, "attn_pool_energy_bf16", s)) return e;
  if (int e = pool_bf16_aligned(pool, "attn_pool_energy_bf16")) return e;
  return sh_energy(s, "attn_pool_energy_bf16", nullptr, WH_W, WC_W, energy, workspace, stream_, pool);
}

extern "C" int fvta_attn_pool_fwd_tw_bf16(const fvta_attn_pool_tw_desc* d, const uint16_t* pool, const uint8_t* pool_mask,
                                          const float* energy, const float* hq, const uint8_t* qmask, const float* lq,
                                          const int32_t* albums, const float* W, const float* b, const float* WH_b, const float* WC_W,
                                          const float* WC_b, float* h_a, float* a_logits, float* scale_out, void* workspace,
                                          fvta_stream_t stream_) {
  ShShape s;
  if (int e = sh_open_tw(d, "attn_pool_fwd_tw_bf16", s)) return e;
  FVTA_CHECK_ARG(pool && energy && hq && lq && albums && WH_b && WC_W && WC_b && h_a && workspace,
                 "attn_pool_fwd_tw_bf16: null pointer");
  FVTA_CHECK_ARG(d->shape.simi == 4 || W, "attn_pool_fwd_tw_bf16: simiMatrix %d needs att_logits/W", d->shape.simi);
  if (int e = pool_bf16_aligned(pool, "attn_pool_fwd_tw_bf16")) return e;
  const ShWarpCall warp{d->warp_type, d->window_t, energy, lq, WH_b, WC_W, WC_b, scale_out};
  return sh_forward(s, true, "attn_pool_fwd_tw_bf16",
                    {nullptr, pool_mask, hq, qmask, albums, W, b, h_a, a_logits, nullptr, workspace, stream_, pool}, &warp);
}

// training: the checks at SH_TRAIN / SH_BWD -- simiMatrix 1-3, and from the backward's entries its grids
extern "C" size_t fvta_attn_pool_saved_bytes(const fvta_attn_pool_desc* d) {
  ShShape s;
  return sh_open(d, "attn_pool_saved_bytes", s, SH_BWD) == FVTA_OK ? ShWork(s, nullptr, nullptr).saved_bytes : 0;
}

extern "C" int fvta_attn_pool_fwd_train(const fvta_attn_pool_desc* d, const float* pool, const uint8_t* pool_mask, const float* hq,
                                        const uint8_t* qmask, const int32_t* albums, const float* W, const float* b, float* h_a,
                                        float* a_logits, void* saved, void* workspace, fvta_stream_t stream_) {
  ShShape s;
  if (int e = sh_open(d, "attn_pool_fwd_train", s, SH_BWD)) return e;
  FVTA_CHECK_ARG(pool && hq && albums && W && h_a && saved && workspace, "attn_pool_fwd_train: null pointer");
  return sh_forward(s, true, "attn_pool_fwd_train", {pool, pool_mask, hq, qmask, albums, W, b, h_a, a_logits, saved, workspace, stream_});
}

extern "C" size_t fvta_attn_pool_bwd_workspace_bytes(const fvta_attn_pool_desc* d) {
  ShShape s;
  return sh_open(d, "attn_pool_bwd_workspace_bytes", s, SH_BWD) == FVTA_OK ? shb_workspace_bytes(s, true) : 0;
}

extern "C" int fvta_attn_pool_bwd_plan(const fvta_attn_pool_desc* d, int32_t out[4]) {
  ShShape s;
  if (int e = sh_open(d, "attn_pool_bwd_plan", s, SH_BWD)) return e;
  return shb_plan(s, "attn_pool_bwd_plan", out);
}

extern "C" int fvta_attn_pool_bwd(const fvta_attn_pool_desc* d, const float* pool, const uint8_t* pool_mask, const float* hq,
                                  const uint8_t* qmask, const int32_t* albums, const float* W, const float* b, const float* d_h_a,
                                  const void* saved, float* d_pool, float* d_hq, float* dW, float* db, void* workspace,
                                  fvta_stream_t stream_) {
  ShShape s;
  if (int e = sh_open(d, "attn_pool_bwd", s, SH_BWD)) return e;
  FVTA_CHECK_ARG(pool && hq && albums && d_h_a && saved && d_pool && d_hq && dW && db && workspace, "attn_pool_bwd: null pointer");
  return shb_backward(s, true, "attn_pool_bwd", {pool, pool_mask, hq, qmask, d_h_a, saved, d_pool, d_hq, dW, db, workspace, stream_});
}

// ---- training under the time warp: the warped descriptor through sh_check_tw at SH_BWD, the same two drivers
extern "C" size_t fvta_attn_pool_tw_saved_bytes(const fvta_attn_pool_tw_desc* d) {
  ShShape s;
  if (sh_open_tw(d, "attn_pool_tw_saved_bytes", s, SH_BWD) != FVTA_OK) return 0;
  return ShTwSaved(s, ShWork(s, nullptr, nullptr), nullptr).bytes;
}

extern "C" int fvta_attn_pool_fwd_tw_train(const fvta_attn_pool_tw_desc* d, const float* pool, const uint8_t* pool_mask,
                                           const float* energy, const float* hq, const uint8_t* qmask, const float* lq,
                                           const int32_t* albums, const float* W, const float* b, const float* WH_b,
                                           const float* WC_W, const float* WC_b, float* h_a, float* a_logits, float* scale_out,
                                           void* saved, void* workspace, fvta_stream_t stream_) {
  ShShape s;
  if (int e = sh_open_tw(d, "attn_pool_fwd_tw_train", s, SH_BWD)) return e;
  FVTA_CHECK_ARG(pool && energy && hq && lq && albums && W && WH_b && WC_W && WC_b && h_a && saved && workspace,
                 "attn_pool_fwd_tw_train: null pointer");
  const ShWarpCall warp{d->warp_type, d->window_t, energy, lq, WH_b, WC_W, WC_b, scale_out};
  return sh_forward(s, true, "attn_pool_fwd_tw_train", {pool, pool_mask, hq, qmask, albums, W, b, h_a, a_logits, saved, workspace, stream_},
                    &warp);
}

extern "C" size_t fvta_attn_pool_tw_bwd_workspace_bytes(const fvta_attn_pool_tw_desc* d) {
  ShShape s;
  return sh_open_tw(d, "attn_pool_tw_bwd_workspace_bytes", s, SH_BWD) == FVTA_OK ? shb_workspace_bytes(s, true, true) : 0;
}

extern "C" int fvta_attn_pool_bwd_tw(const fvta_attn_pool_tw_desc* d, const float* pool, const uint8_t* pool_mask, const float* hq,
                                     const uint8_t* qmask, const float* lq, const int32_t* albums, const float* W, const float* b,
                                     const float* WH_W, const float* WH_b, const float* WC_W, const float* WC_b, const float* d_h_a,
                                     const void* saved, float* d_pool, float* d_hq, float* d_lq, float* dW, float* db, float* dWH_W,
                                     float* dWH_b, float* dWC_W, float* dWC_b, void* workspace, fvta_stream_t stream_) {
  ShShape s;
  if (int e = sh_open_tw(d, "attn_pool_bwd_tw", s, SH_BWD)) return e;
  FVTA_CHECK_ARG(pool && hq && lq && albums && W && WH_W && WH_b && WC_W && WC_b && d_h_a && saved && d_pool && d_hq && d_lq && dW &&
                     db && dWH_W && dWH_b && dWC_W && dWC_b && workspace,
                 "attn_pool_bwd_tw: null pointer");
  const ShBwdWarpCall warp{d->warp_type, d->window_t, lq, WH_W, WH_b, WC_W, WC_b, d_lq, dWH_W, dWH_b, dWC_W, dWC_b};
  return shb_backward(s, true, "attn_pool_bwd_tw", {pool, pool_mask, hq, qmask, d_h_a, saved, d_pool, d_hq, dW, db, workspace, stream_},
                      &warp);
}

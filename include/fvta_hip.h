/* fvta_hip.h -- C ABI of libfvta_hip.so: the FVTA hot path on MI355X (gfx950).
 *
 * The reference (JunweiLiang/FVTA_MemexQA) has no FFI/plugin layer: its hot path
 * is a TensorFlow-1 graph built in model_v2.py and entered through one
 * `sess.run` per step (trainer.py:36-38, tester.py:21).  This header is the
 * boundary a maintainer would bind instead (ctypes stub in INTEGRATION.md).  Each
 * entry point names the reference code it replaces (file:line in the reference
 * repository).
 *
 * Conventions
 *  - extern "C"; every call returns an int status (FVTA_OK or a negative
 *    FVTA_ERR_*); nothing throws; fvta_last_error() gives the message.
 *  - every buffer is a CALLER-OWNED DEVICE pointer, row-major, innermost =
 *    hidden/feature axis, 16-byte aligned.  The library never allocates:
 *    scratch is passed in (`*_bytes` queries size it) and may be reused
 *    between calls; "saved" buffers carry forward state to the backward call.
 *  - every call is asynchronous on the given hipStream_t, re-entrant, and
 *    keeps no global state.
 *  - masks are bytes (0 / non-0), as the reference feeds bool arrays
 *    (model_v2.py:1171-1200).
 */
#ifndef FVTA_HIP_H
#define FVTA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FVTA_OK 0
#define FVTA_ERR_INVALID_ARG (-1)
#define FVTA_ERR_LAUNCH (-2)
#define FVTA_ERR_UNSUPPORTED (-3)

#define FVTA_F32 0  /* exact fp32 arithmetic (v_mfma_f32_32x32x2_f32 + VALU) */
#define FVTA_BF16 1 /* bf16 MFMA operands, fp32 accumulate (BASELINE.json configs[2]) */
#define FVTA_BF16X3 2 /* bi-LSTM only: every MFMA operand split in two bf16 terms, three products per GEMM (hi hi + hi lo +
                         lo hi, fp32 accumulate; what is dropped is <= 3 * 2^-17 of |a||b| per product), saved gates fp32:
                         the 1e-4 parity engine on the bf16 matrix pipe (model_v2.py:652-661 computes in fp32) */

typedef void* fvta_stream_t; /* hipStream_t */

int fvta_version(void);
const char* fvta_last_error(void);
/* sizeof of a descriptor struct as the library was compiled: which = 0 fvta_attn_desc, 1 fvta_lstm_desc,
 * 2 fvta_scorer_desc, 3 fvta_timewarp_desc, 4 fvta_embed_desc, 5 fvta_imgtrans_desc, 6 fvta_guard_desc,
 * 7 fvta_guard_ctl, 9 fvta_attgru_seq_desc, 10 fvta_gru_seq_desc, 11 fvta_cbp_desc, 12 fvta_attn_shared_desc,
 * 13 fvta_attn_shared_tw_desc, 14 fvta_attn_pool_desc, 15 fvta_attn_pool_tw_desc (8 stays unassigned: bindings probe it
 * as the unknown id); -1 otherwise.
 * A binding compares
 * its own layout with it when it loads the library (fvta_memexqa_amd/_lib.py does). */
int64_t fvta_abi_struct_bytes(int32_t which);

/* ------------------------------------------------------------------------- *
 * Focal attention: model_v2.py:210-298 `attention_3d` (K modalities) and
 * model_v2.py:125-201 / model.py:117-186 `attention` (call with K = 1),
 * including the helpers they inline: `linear` 75-100, `exp_mask`
 * utils.py:210-213, `softsel`/`softmax` model_v2.py:23-48.
 *
 *   hinfo [N,K,T,w]  hq [N,JQ,w]  hmask [N,K,T]  qmask [N,JQ]  (masks may
 *   both be NULL = unmasked, model_v2.py:146/233)
 *   W [F], b [1]: att_logits/{W,b}; F = 3w|2w|4w for simi 1|2|3 (feature
 *   order of model_v2.py:242-248; feat_order=1 selects model.py:149's order
 *   for simi 2); simi 4 (cosine, model_v2.py:250-254) takes W = b = NULL.
 *   out: h_a [N,w]; a_logits [N,K,T,JQ] masked logits (NULL = not wanted;
 *   only tester.py:34-36 `step_vis` reads them).
 * ------------------------------------------------------------------------- */
typedef struct fvta_attn_desc {
  int32_t N, K, T, JQ, w;
  int32_t simi;       /* 1..4 */
  int32_t feat_order; /* 0: model_v2.py order, 1: model.py:149 order (simi 2 only) */
  int32_t add_tanh;   /* model_v2.py:92-93 via linear(add_tanh=) */
  /* Elements between consecutive batch rows n of hinfo / d_hinfo; 0 = dense (K*T*w).  Non-zero needs K == 1 and no
   * tscale: the 1-D attention of model.py:117-186 run on ONE stream of a context arena laid out [N][all streams' rows]
   * (model.py:836-846, per-stream attention; :929-944 runs over the concatenation of the same rows). */
  int64_t hinfo_stride;
} fvta_attn_desc;

size_t fvta_attn_workspace_bytes(const fvta_attn_desc* d);
size_t fvta_attn_saved_bytes(const fvta_attn_desc* d);
/* How the kernels split this descriptor's work (host only, launches nothing; use_mask = both masks given):
 * out = {nsplit, bsplit, gk, ng} -- workgroups per (n,k) of the forward main kernel and of the backward main kernel,
 * consecutive k of one n that share a backward workgroup (> 1 only with bsplit == 1), and ceil(K / gk) groups per n.
 * For tests and tools that must know which regime a shape runs in. */
int fvta_attn_plan(const fvta_attn_desc* d, int32_t use_mask, int32_t out[4]);

int fvta_attn_fwd(const fvta_attn_desc* d, const float* hinfo, const float* hq, const uint8_t* hmask,
                  const uint8_t* qmask, const float* W, const float* b, float* h_a, float* a_logits,
                  void* saved, void* workspace, fvta_stream_t stream);

/* Backward of fvta_attn_fwd given d_h_a [N,w].  accumulate = 0: d_hinfo [N,K,T,w]
 * and d_hq [N,JQ,w] are overwritten (masked rows of d_hinfo get zeros);
 * 1: both are accumulated into; 2: d_hq is accumulated into and only the VALID
 * rows of d_hinfo are written (plain stores, masked rows left untouched: the
 * encoders never read them -- this is what the fused model uses, it saves the
 * clear and the read-modify-write of the largest tensor of the step); 3: d_hq
 * accumulated into, d_hinfo overwritten with zeros on masked rows.  dW [F]
 * and db [1] are always accumulated into (slices of the flat gradient buffer).  Gradient routing through reduce_max goes to the first arg-max
 * (model_v2.py:268,278; TF splits exact ties). */
int fvta_attn_bwd(const fvta_attn_desc* d, const float* hinfo, const float* hq, const uint8_t* hmask,
                  const uint8_t* qmask, const float* W, const float* b, const float* d_h_a,
                  const void* saved, float* d_hinfo, float* d_hq, float* dW, float* db, int accumulate,
                  void* workspace, fvta_stream_t stream);

/* fvta_attn_fwd / fvta_attn_bwd over the encoders' bf16 SHADOW rows instead of an fp32 hinfo (model_v2.py:863-914's
 * context tensor is the concatenation of the two directions' outputs the bi-LSTM has already written as bf16):
 * table [2][N*K*T] device addresses, table[half][(n K + k) T + t] -> the w/2 bf16 values that are channels
 * half * w/2 .. of row (n,k,t) (fvta_lstm_shadow_rows; EVERY entry must be readable: rows no encoder writes point at
 * w/2 zeros).  JQ <= 32, w = 512 or 1024, simiMatrix 1-3, no hinfo_stride, no a_logits; FVTA_ERR_INVALID_ARG otherwise.  Results
 * are those of fvta_attn_fwd / fvta_attn_bwd run on the bf16-rounded rows.  `saved` / `workspace` sizes as above. */
int fvta_attn_fwd_shadow(const fvta_attn_desc* d, const uint64_t* table, const float* hq, const uint8_t* hmask,
                         const uint8_t* qmask, const float* W, const float* b, float* h_a, void* saved, void* workspace,
                         fvta_stream_t stream);
int fvta_attn_bwd_shadow(const fvta_attn_desc* d, const uint64_t* table, const float* hq, const uint8_t* hmask,
                         const uint8_t* qmask, const float* W, const float* b, const float* d_h_a, const void* saved,
                         float* d_hinfo, float* d_hq, float* dW, float* db, int accumulate, void* workspace,
                         fvta_stream_t stream);

/* attention_3d(..., time_warp_att=True, C=C): model_v2.py:269-275.  The max-pooled logits are multiplied by the
 * row sums of C before the softmax over t: tscale [N,T] = sum_t' C[n,t,t'] (with the model's time warp, c[n,t] cnt(t) =
 * fvta_timewarp_fwd's scale_out).  The softmax over K keeps the unscaled maxima.  The reference scales AFTER exp_mask,
 * so a masked row's logit is -1e30 * tscale: for tscale < 0 the masked rows take the softmax; the kernels
 * reproduce that.  tscale NULL = fvta_attn_fwd / fvta_attn_bwd.  d_tscale [N,T] is accumulated into. */
int fvta_attn_fwd_tw(const fvta_attn_desc* d, const float* hinfo, const float* hq, const uint8_t* hmask,
                     const uint8_t* qmask, const float* W, const float* b, const float* tscale, float* h_a,
                     float* a_logits, void* saved, void* workspace, fvta_stream_t stream);
int fvta_attn_bwd_tw(const fvta_attn_desc* d, const float* hinfo, const float* hq, const uint8_t* hmask,
                     const uint8_t* qmask, const float* W, const float* b, const float* tscale, const float* d_h_a,
                     const void* saved, float* d_hinfo, float* d_hq, float* dW, float* db, float* d_tscale,
                     int accumulate, void* workspace, fvta_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Focal attention, many questions over one album (this call: forward only; training: below).
 * The context tensor of model_v2.py:863-914 depends on
 * the album alone, the question enters at attention_3d (:210-298).  hinfo [A,K,T,w] / hmask [A,K,T] hold each album
 * once; question i (hq [NQ,JQ,w], qmask [NQ,JQ]) attends album[i]:
 *   h_a[i], a_logits[i] = what fvta_attn_fwd returns for (hinfo[album[i]], hq[i], hmask[album[i]], qmask[i]),
 * exp_mask on hmask & qmask, the max over j, the softmax over t per modality and over K of the per-modality maxima, the
 * uniform-over-all-T result of a fully masked (album, k) or question, and both masks NULL = unmasked, included.
 *   album [NQ]: int32 on the DEVICE, any order, repeats allowed, an album may have no question.  Indices are data: the
 *   kernels clamp them into [0, A) before they address anything; a binding validates them on the host
 *   (ops.check_album_index does).
 *   W, b: as fvta_attn_fwd (feature order of model_v2.py:242-254; simi 4 takes NULL).  a_logits [NQ,K,T,JQ] or NULL.
 * The time warp (use_time_warp, every warp type) is covered by fvta_attn_shared_fwd_tw further down (training:
 * fvta_attn_shared_fwd_tw_train / fvta_attn_shared_bwd_tw): the
 * warp is one scalar per (question, position), so the rows stay shared.  Not here, nor there: time_warp_att (a masked row
 * takes the softmax where its scale is negative), shadow rows, and a backward of THIS call -- it keeps no `saved`;
 * fvta_attn_shared_fwd_train / fvta_attn_shared_bwd below train over the shared rows (simiMatrix 1-3, no time warp),
 * fvta_attn_fwd / fvta_attn_bwd per question otherwise.
 * Range: w in {64,128,256,512,1024,2048}, JQ 1..64, K 1..64, simi 1..4, any T, A >= 1, NQ >= 1; otherwise the size
 * query returns 0 and the calls FVTA_ERR_UNSUPPORTED / FVTA_ERR_INVALID_ARG with a message.
 * The questions are grouped by album ON THE DEVICE (counting sort, groups of at most G: 8 at JQ <= 32, 4 above), no
 * host synchronisation.  A row is read twice per group of its album (logits, weighted sum), never once per question.
 * The logits are an exact-fp32 [rows, w] x [w, G*JP] product per group.  No floating-point atomics, fixed summation
 * order (the T splits depend on the descriptor only): two runs are bitwise equal, and a question's result does not
 * depend on which other questions are in the call.
 * fvta_attn_shared_plan (host only, launches nothing): out = {G, rows per logits tile, T splits of the weighted sum,
 * rows per split of the weighted sum}; the weighted sum stages a split's softmax weights 64 rows at a time.
 * ------------------------------------------------------------------------- */
typedef struct fvta_attn_shared_desc {
  int32_t A, NQ, K, T, JQ, w; /* A albums (context rows [A,K,T,w]), NQ questions */
  int32_t simi;               /* 1..4, feature order of model_v2.py:242-254 */
  int32_t add_tanh;
} fvta_attn_shared_desc; /* fvta_abi_struct_bytes(12) */

size_t fvta_attn_shared_workspace_bytes(const fvta_attn_shared_desc* d); /* 0 bytes: see fvta_last_error */
int fvta_attn_shared_plan(const fvta_attn_shared_desc* d, int32_t out[4]);
int fvta_attn_shared_fwd(const fvta_attn_shared_desc* d, const float* hinfo, const uint8_t* hmask, const float* hq,
                         const uint8_t* qmask, const int32_t* album, const float* W, const float* b, float* h_a,
                         float* a_logits, void* workspace, fvta_stream_t stream);

/* Training over shared rows (simiMatrix 1-3; with simi 4 the two size queries return 0 and the calls
 * FVTA_ERR_UNSUPPORTED: the per-question route, fvta_attn_fwd / fvta_attn_bwd on gathered rows, covers the cosine form).
 * fvta_attn_shared_fwd_train: the kernels of fvta_attn_shared_fwd -- h_a and a_logits are its bits -- and, in the
 *   caller-held `saved` (fvta_attn_shared_saved_bytes), what the backward reads: amax [NQ,K,T], the FIRST arg-max jmax
 *   [NQ,K,T] (u8), M, L, r [NQ,K], u [NQ,K,w], Qs, ct, the per-channel vectors, and the plan (grp, order, qslot, ngroups,
 *   per-album starts and counts).  In this plan the questions of an album stand by ascending question index.
 *   `workspace`: fvta_attn_shared_workspace_bytes, free again when the call returns.
 * fvta_attn_shared_bwd: from d_h_a [NQ,w], for question i: d_hq[i] and i's share of dW / db are what fvta_attn_bwd
 *   (accumulate = 0) gives for (hinfo[album[i]], hq[i], hmask[album[i]], qmask[i], d_h_a[i]); d_hinfo[a] is the sum of
 *   those calls' d_hinfo over the questions of album a.  d_hinfo [A,K,T,w] and d_hq [NQ,JQ,w] are OVERWRITTEN (an album
 *   without a question: zeros; a masked row: zeros, unless a fully masked question or (album, k) spreads its uniform
 *   softmax over it, as in fvta_attn_bwd); dW [F] and db [1] are accumulated into.  fvta_attn_bwd's deviations carry
 *   over: the max over j routes to the first arg-max, ties of the max over t are split, a fully masked (album, k) or
 *   question passes nothing into its masked logits.  The same arguments as the forward call; `workspace`:
 *   fvta_attn_shared_bwd_workspace_bytes.  Not here: shadow rows, accumulate modes, the gradient of a_logits; under the
 *   time warp fvta_attn_shared_bwd_tw (further down) is the call.
 *   No [NQ,K,T,w]-sized buffer: each d_hinfo row is written once, rows are read once per (album, k) and once per group of
 *   the album's questions.  No floating-point atomics, fixed summation order (the sum over an album's questions runs by
 *   ascending question index): two calls are bitwise equal in all four outputs.  No host synchronisation.
 * fvta_attn_shared_bwd_plan (host only): out = {rows per tile of the row pass, T splits of the question pass, channels
 *   per slice of the question pass, row tiles per workgroup of the row pass}. */
size_t fvta_attn_shared_saved_bytes(const fvta_attn_shared_desc* d);         /* 0 bytes: see fvta_last_error */
size_t fvta_attn_shared_bwd_workspace_bytes(const fvta_attn_shared_desc* d); /* 0 bytes: see fvta_last_error */
int fvta_attn_shared_bwd_plan(const fvta_attn_shared_desc* d, int32_t out[4]);
int fvta_attn_shared_fwd_train(const fvta_attn_shared_desc* d, const float* hinfo, const uint8_t* hmask, const float* hq,
                               const uint8_t* qmask, const int32_t* album, const float* W, const float* b, float* h_a,
                               float* a_logits, void* saved, void* workspace, fvta_stream_t stream);
int fvta_attn_shared_bwd(const fvta_attn_shared_desc* d, const float* hinfo, const uint8_t* hmask, const float* hq,
                         const uint8_t* qmask, const int32_t* album, const float* W, const float* b, const float* d_h_a,
                         const void* saved, float* d_hinfo, float* d_hq, float* dW, float* db, void* workspace,
                         fvta_stream_t stream);

/* fvta_attn_shared_fwd under the time warp (use_time_warp without use_time_warp_att).  The warp of
 * model_v2.py:953-1009 (fvta_timewarp_fwd below) takes the question's last state lq, but it is one scalar per
 * (question, position):
 *   h'[q,k,t,:] = hinfo[a,k,t,:] scale[q,t]                               a = album[q]
 *   scale[q,t]  = tanh(e[a,t] + K (s0 + WC . lq[q])) cnt(t)               cnt: the warp type's count, window ceil(window_t)
 *   e[a,t]      = sum_k sum_c v[c] hinfo[a,k,t,c]^2                       v = WH[:w] WC,  s0 = b_WH . WC + b_WC
 * Only e reads the rows, and it belongs to the album.  The scalar goes through the bilinear form of the logits and
 * through the weighted sum, so the rows stay held once and are read twice per group as in fvta_attn_shared_fwd; no
 * [NQ,K,T,w] tensor exists, warped or not.
 * fvta_attn_shared_energy: energy [A,T] = e, every k summed (masked rows too, as fvta_timewarp_fwd), fixed order.  It
 *   depends on hinfo, WH_W and WC_W alone: compute it once per album set and keep it while those stay what they are
 *   (A T floats beside the A K T w of the rows).  WH_W [2w,w]: the first w rows are read.  NQ, JQ and simi of the
 *   descriptor must be valid but do not enter.
 * fvta_attn_shared_fwd_tw: h_a[i], a_logits[i] = what fvta_attn_fwd returns for (fvta_timewarp_fwd's warp_h of
 *   (hinfo[album[i]], lq[i]), hq[i], hmask[album[i]], qmask[i]); scale_out [NQ,T] (or NULL) = that call's scale_out.
 *   lq [NQ,w]; WH_b [w], WC_W [w], WC_b [1]; the other arguments as fvta_attn_shared_fwd.  The masks stay the albums':
 *   a masked row is -1e30 whatever its scale.
 * `workspace`: fvta_attn_shared_tw_workspace_bytes, for either call.  warp_type outside 1..5: FVTA_ERR_INVALID_ARG, "time
 * warping type not implemented" (model_v2.py:341), and 0 from the size query.  No host synchronisation, no
 * floating-point atomics: two calls are bitwise equal, and a question's numbers do not depend on the other questions. */
typedef struct fvta_attn_shared_tw_desc {
  fvta_attn_shared_desc shape;
  int32_t warp_type; /* 1..5 (model_v2.py:301-341) */
  float window_t;    /* warp_type 5: time_warp_window_t */
} fvta_attn_shared_tw_desc; /* fvta_abi_struct_bytes(13) */

size_t fvta_attn_shared_tw_workspace_bytes(const fvta_attn_shared_tw_desc* d); /* 0 bytes: see fvta_last_error */
int fvta_attn_shared_energy(const fvta_attn_shared_tw_desc* d, const float* hinfo, const float* WH_W, const float* WC_W,
                            float* energy, void* workspace, fvta_stream_t stream);
int fvta_attn_shared_fwd_tw(const fvta_attn_shared_tw_desc* d, const float* hinfo, const uint8_t* hmask, const float* energy,
                            const float* hq, const uint8_t* qmask, const float* lq, const int32_t* album, const float* W,
                            const float* b, const float* WH_b, const float* WC_W, const float* WC_b, float* h_a,
                            float* a_logits, float* scale_out, void* workspace, fvta_stream_t stream);

/* Training under the time warp over shared rows (simiMatrix 1-3; with simi 4 the two size queries return 0 and the calls
 * FVTA_ERR_UNSUPPORTED; a warp type outside 1..5: 0 and FVTA_ERR_INVALID_ARG).
 * fvta_attn_shared_fwd_tw_train: the kernels of fvta_attn_shared_fwd_tw -- h_a, a_logits and scale_out are its bits --
 *   with the ordered plan of fvta_attn_shared_fwd_train, and in the caller-held `saved` (fvta_attn_shared_tw_saved_bytes)
 *   what fvta_attn_shared_fwd_train saves, then scale [NQ,T], tanh(z) [NQ,T], lin [NQ,K,T] (h.Qs + Rh.h at the arg-max,
 *   before the scale enters) and r2 [A,K,T] (R2.h^2).  `workspace`: fvta_attn_shared_tw_workspace_bytes.
 * fvta_attn_shared_bwd_tw: from d_h_a [NQ,w], for question i what fvta_timewarp_fwd -> fvta_attn_fwd -> fvta_attn_bwd
 *   (accumulate 0, masked rows zero) -> fvta_timewarp_bwd give on (hinfo[album[i]], lq[i], hq[i], ...), the row gradients
 *   summed per album, the parameter gradients over all questions.  d_hinfo [A,K,T,w], d_hq [NQ,JQ,w] and d_lq [NQ,w] are
 *   OVERWRITTEN (an album without a question: zeros); dW [F], db [1], dWH_W (its first w rows, [w,w]; rows w..2w-1 have no
 *   gradient and are not touched), dWH_b [w], dWC_W [w] and dWC_b [1] are accumulated into.  fvta_attn_bwd's deviations
 *   carry over (first arg-max over j, ties over t split, a fully masked (album, k) or question).  window_t has no gradient.
 *   db is summed as -sum damax x^2 (tanh; 0 without): the same number as the sum of the d ct without its cancellation.
 *   The energy is not an argument: tanh(z) is in `saved`, and the gradient through e reaches d_hinfo, dWH_W and dWC_W.
 *   No time_warp_att, no shadow rows, no gradient of a_logits or scale_out.  No [NQ,K,T,w]-sized buffer; each d_hinfo row
 *   is written once by the row pass and read and written once more by the energy's backward; the rows are read once per
 *   (album, k), once per group of the album's questions and once for the energy.  No floating-point atomics, fixed
 *   summation order (an album's questions by ascending index): two calls are bitwise equal in all nine outputs.  No host
 *   synchronisation, no memset.  `workspace`: fvta_attn_shared_tw_bwd_workspace_bytes. */
size_t fvta_attn_shared_tw_saved_bytes(const fvta_attn_shared_tw_desc* d);         /* 0 bytes: see fvta_last_error */
size_t fvta_attn_shared_tw_bwd_workspace_bytes(const fvta_attn_shared_tw_desc* d); /* 0 bytes: see fvta_last_error */
int fvta_attn_shared_fwd_tw_train(const fvta_attn_shared_tw_desc* d, const float* hinfo, const uint8_t* hmask,
                                  const float* energy, const float* hq, const uint8_t* qmask, const float* lq,
                                  const int32_t* album, const float* W, const float* b, const float* WH_b, const float* WC_W,
                                  const float* WC_b, float* h_a, float* a_logits, float* scale_out, void* saved, void* workspace,
                                  fvta_stream_t stream);
int fvta_attn_shared_bwd_tw(const fvta_attn_shared_tw_desc* d, const float* hinfo, const uint8_t* hmask, const float* hq,
                            const uint8_t* qmask, const float* lq, const int32_t* album, const float* W, const float* b,
                            const float* WH_W, const float* WH_b, const float* WC_W, const float* WC_b, const float* d_h_a,
                            const void* saved, float* d_hinfo, float* d_hq, float* d_lq, float* dW, float* db, float* dWH_W,
                            float* dWH_b, float* dWC_W, float* dWC_b, void* workspace, fvta_stream_t stream);

/* Focal attention over per-question album LISTS from one album pool (forward only, inference).  The encoders run per
 * (question, album) (model_v2.py:704-760), so the JX context rows of one album do not depend on which albums stand beside
 * it: pool [P,K,JX,w] / pool_mask [P,K,JX] hold every encoded album once, and question i lists M of them,
 * albums [NQ,M] int32 on the DEVICE: entries in [0, P), or negative for an EMPTY slot.  With T = M JX,
 *   hinfo_i[k, m JX + j] = pool[albums[i,m], k, j]   (an empty slot: JX zero rows, mask 0)
 *   h_a[i], a_logits[i] = what fvta_attn_fwd returns for (hinfo_i, hq[i], its mask, qmask[i]);
 * no [NQ,K,T,w] tensor exists anywhere.  h_a [NQ,w], a_logits [NQ,K,T,JQ] or NULL.  The same album may stand twice in one
 * list; an album nobody lists is never read; a question whose slots are all empty gets h_a = 0 (the uniform softmax over
 * T zero rows).  Indices are data: the kernels take a negative entry as empty and clamp an entry >= P to P - 1 before it
 * addresses anything; a binding validates them on the host (ops.check_album_lists does).
 * The masks apply only when both are given, as everywhere; an EMPTY SLOT IS MASKED ALL THE SAME (its positions hold
 * -1e30 whether or not masks are given), which is no longer the reference's unmasked result: a binding refuses empty
 * slots without masks (ops.check_album_lists(masked=False) does).
 * The kernels are fvta_attn_shared_fwd's with a column block of a group's product standing for a (question, slot)
 * reference instead of a question: the NQ M references are grouped by pooled album on the device (counting sort, groups
 * of at most G), a pooled album's rows are read twice per group of references to it, however many distinct lists there
 * are.  The softmax runs per question over its T positions; h_a[i] is the sum of its references' partial sums in
 * (k, slot, split) order.  No floating-point atomics, splits from the descriptor only: two calls are bitwise equal, so is
 * a call after relabelling the pool, and at M = 1 the call returns fvta_attn_shared_fwd's bits for (A = P, T = JX).
 * Range: fvta_attn_shared_fwd's (w, JQ <= 64, K <= 64, simi 1..4), P, NQ, M, JX >= 1, NQ M <= 2^28, M JX within int.
 * No host synchronisation, no memset, everything on the caller's stream.
 * fvta_attn_pool_plan (host only): out = {G, rows per logits tile, splits of JX in the weighted sum, rows per split}.
 * The time warp (use_time_warp, every warp type) is fvta_attn_pool_fwd_tw further down; training over the pool
 * (simiMatrix 1-3) is fvta_attn_pool_fwd_train / fvta_attn_pool_bwd below, and under the time warp
 * fvta_attn_pool_fwd_tw_train / fvta_attn_pool_bwd_tw at the end of this section.  Not here, nor there: time_warp_att,
 * shadow rows. */
typedef struct fvta_attn_pool_desc {
  int32_t P, NQ, M, K, JX, JQ, w; /* P pooled albums [P,K,JX,w], NQ questions listing M albums each */
  int32_t simi;                   /* 1..4 */
  int32_t add_tanh;
} fvta_attn_pool_desc; /* fvta_abi_struct_bytes(14) */

size_t fvta_attn_pool_workspace_bytes(const fvta_attn_pool_desc* d); /* 0 bytes: see fvta_last_error */
int fvta_attn_pool_plan(const fvta_attn_pool_desc* d, int32_t out[4]);
int fvta_attn_pool_fwd(const fvta_attn_pool_desc* d, const float* pool, const uint8_t* pool_mask, const float* hq,
                       const uint8_t* qmask, const int32_t* albums, const float* W, const float* b, float* h_a,
                       float* a_logits, void* workspace, fvta_stream_t stream);

/* Training over the pool (simiMatrix 1-3; under the time warp: the pair at the end of this section; with simi 4 the
 * two size queries return 0 and the calls FVTA_ERR_UNSUPPORTED: the per-question route, fvta_attn_fwd / fvta_attn_bwd on
 * gathered rows, covers the cosine form).
 * The contract is fvta_attn_shared_bwd's read per REFERENCE (question i, slot m):
 * fvta_attn_pool_fwd_train: the kernels of fvta_attn_pool_fwd -- h_a and a_logits are its bits -- and, in the
 *   caller-held `saved` (fvta_attn_pool_saved_bytes), what the backward reads: amax and the FIRST arg-max jmax (u8), both
 *   [NQ,K,M JX], M, L, r [NQ,K], u [NQ,K,w], Qs, ct, the per-channel vectors and the plan, in which the references of a
 *   pooled album stand by ascending id i M + m.  `workspace`: fvta_attn_pool_workspace_bytes.
 * fvta_attn_pool_bwd: from d_h_a [NQ,w], for question i: d_hq[i] and i's share of dW / db are what fvta_attn_bwd
 *   (accumulate = 0) gives for (hinfo_i, hq[i], its mask, qmask[i], d_h_a[i]); d_pool[p] is the sum of those calls' row
 *   gradients over every reference albums[i,m] == p (a question that lists p twice contributes twice).  d_pool
 *   [P,K,JX,w] and d_hq [NQ,JQ,w] are OVERWRITTEN in full (an album nobody lists: zeros; a masked row: zeros, unless a
 *   fully masked question or (question, k) spreads its uniform softmax over it; a question that lists nothing: d_hq = 0);
 *   dW [F] and db [1] are accumulated into.  fvta_attn_bwd's deviations carry over: first arg-max over j, ties of the max
 *   over t split, nothing passes into the masked logits of a fully masked (question, k) or question.  The same arguments
 *   as the forward call; `workspace`: fvta_attn_pool_bwd_workspace_bytes.
 *   No [NQ,K,M JX,w]-sized buffer in either direction: each d_pool row is written once, a pooled album's rows are read
 *   once per (album, k) and once per group of references to it.  No floating-point atomics, fixed summation order (an
 *   album's references by ascending id, a question's slots by ascending slot): two calls are bitwise equal in all four
 *   outputs, and at M = 1 they are fvta_attn_shared_bwd's bits for (A = P, T = JX).  No host synchronisation, no memset.
 * fvta_attn_pool_bwd_plan (host only): the four words of fvta_attn_shared_bwd_plan for (A = P, T = JX, NQ M references). */
size_t fvta_attn_pool_saved_bytes(const fvta_attn_pool_desc* d);         /* 0 bytes: see fvta_last_error */
size_t fvta_attn_pool_bwd_workspace_bytes(const fvta_attn_pool_desc* d); /* 0 bytes: see fvta_last_error */
int fvta_attn_pool_bwd_plan(const fvta_attn_pool_desc* d, int32_t out[4]);
int fvta_attn_pool_fwd_train(const fvta_attn_pool_desc* d, const float* pool, const uint8_t* pool_mask, const float* hq,
                             const uint8_t* qmask, const int32_t* albums, const float* W, const float* b, float* h_a,
                             float* a_logits, void* saved, void* workspace, fvta_stream_t stream);
int fvta_attn_pool_bwd(const fvta_attn_pool_desc* d, const float* pool, const uint8_t* pool_mask, const float* hq,
                       const uint8_t* qmask, const int32_t* albums, const float* W, const float* b, const float* d_h_a,
                       const void* saved, float* d_pool, float* d_hq, float* dW, float* db, void* workspace,
                       fvta_stream_t stream);

/* fvta_attn_pool_fwd under the time warp (use_time_warp without use_time_warp_att; forward only, inference).  Per
 * question the result is what fvta_attn_fwd returns on fvta_timewarp_fwd's warp of (hinfo_i, lq[i]), hinfo_i the
 * question's M albums laid end to end as above (an empty slot: JX zero rows, mask 0), with hinfo_i's masks.  The warp is
 * one scalar per (question, position), so neither hinfo_i nor its warp is ever built:
 *   scale[i,t] = tanh(e_i[t] + K (s0 + WC . lq[i])) cnt(t)       t = m JX + j, cnt over the question's WHOLE M JX positions
 *   e_i[t]     = energy[albums[i,m], j], 0 for an empty slot       (a band, past or future runs across slot boundaries)
 *   energy[p,j] = sum_k sum_c v[c] pool[p,k,j,c]^2                 v = WH[:w] WC,  s0 = b_WH . WC + b_WC
 * fvta_attn_pool_energy: energy [P,JX], the two launches of fvta_attn_shared_energy with A = P, T = JX: its bits.  It
 *   depends on pool, WH_W and WC_W alone: compute it once per pool and keep it while those stay what they are.  NQ, M, JQ
 *   and simi of the descriptor must be valid but do not enter.
 * fvta_attn_pool_fwd_tw: lq [NQ,w]; WH_b [w], WC_W [w], WC_b [1]; h_a [NQ,w], a_logits [NQ,K,M JX,JQ] or NULL, scale_out
 *   [NQ,M JX] or NULL (an empty slot's positions: tanh(K (s0 + WC . lq)) cnt(t), what the definition gives on zero rows);
 *   the other arguments as fvta_attn_pool_fwd.  The masks stay the albums': a masked row is -1e30 whatever its scale.
 *   The launches are fvta_attn_pool_fwd's with the scale kernel in front; at M = 1 all three outputs are
 *   fvta_attn_shared_fwd_tw's bits for (A = P, T = JX).
 * `workspace`: fvta_attn_pool_tw_workspace_bytes, for either call (no [NQ,K,M JX,w]-sized piece).  Range:
 * fvta_attn_pool_fwd's, and M JX <= 65535 * 256.  warp_type outside 1..5: FVTA_ERR_INVALID_ARG, "time warping type not
 * implemented" (model_v2.py:341), and 0 from the size query.  No host synchronisation, no memset, no floating-point
 * atomics, everything on the caller's stream: two calls are bitwise equal, and a question's numbers do not depend on the
 * other questions. */
typedef struct fvta_attn_pool_tw_desc {
  fvta_attn_pool_desc shape;
  int32_t warp_type; /* 1..5 (model_v2.py:301-341) */
  float window_t;    /* warp_type 5: time_warp_window_t */
} fvta_attn_pool_tw_desc; /* fvta_abi_struct_bytes(15) */

size_t fvta_attn_pool_tw_workspace_bytes(const fvta_attn_pool_tw_desc* d); /* 0 bytes: see fvta_last_error */
int fvta_attn_pool_energy(const fvta_attn_pool_tw_desc* d, const float* pool, const float* WH_W, const float* WC_W,
                          float* energy, void* workspace, fvta_stream_t stream);
int fvta_attn_pool_fwd_tw(const fvta_attn_pool_tw_desc* d, const float* pool, const uint8_t* pool_mask, const float* energy,
                          const float* hq, const uint8_t* qmask, const float* lq, const int32_t* albums, const float* W,
                          const float* b, const float* WH_b, const float* WC_W, const float* WC_b, float* h_a,
                          float* a_logits, float* scale_out, void* workspace, fvta_stream_t stream);

/* The pool held in bf16 (inference only): pool [P,K,JX,w] as raw bf16 bits (uint16_t; torch.bfloat16), contiguous, HALF
 * the bytes of the fp32 pool, and every row read moves half the bytes.  The three calls take the descriptors and the
 * argument order of their fp32 namesakes; masks, questions, weights, energy, outputs and workspace are fp32 / u8 as there,
 * and the fp32 size queries (fvta_attn_pool_workspace_bytes, fvta_attn_pool_tw_workspace_bytes) and fvta_attn_pool_plan
 * serve them: same launches, same workspace layout, same checks and refusals under the new names.
 * Contract: each call returns what its fp32 namesake returns on the WIDENED pool (every bf16 value as the fp32 value it
 * stands for), BIT FOR BIT -- h_a, a_logits, scale_out, energy.  The kernels are the fp32 ones with another row load: four
 * bf16 in one 8-byte load, widened in registers (exact), every lane on the channels it has there, the matrix pipe fed
 * fp32 as before.  So rows that came from a bf16 encoder lose nothing here; fp32 rows are rounded ONCE, by whoever makes
 * the bf16 pool (round to nearest even), never by these calls.
 * Alignment: `pool` must be 8-byte aligned (w is a multiple of 64, so then every row is); else FVTA_ERR_INVALID_ARG.
 * Not here: training (fvta_attn_pool_fwd_train / _bwd and the warped pair take fp32 rows, d_pool is fp32), the shared
 * family (fvta_attn_shared_*), and the bi-LSTM's shadow-row address tables -- the rows must stand as one contiguous
 * [P,K,JX,w] block. */
int fvta_attn_pool_fwd_bf16(const fvta_attn_pool_desc* d, const uint16_t* pool, const uint8_t* pool_mask, const float* hq,
                            const uint8_t* qmask, const int32_t* albums, const float* W, const float* b, float* h_a,
                            float* a_logits, void* workspace, fvta_stream_t stream);
int fvta_attn_pool_energy_bf16(const fvta_attn_pool_tw_desc* d, const uint16_t* pool, const float* WH_W, const float* WC_W,
                               float* energy, void* workspace, fvta_stream_t stream);
int fvta_attn_pool_fwd_tw_bf16(const fvta_attn_pool_tw_desc* d, const uint16_t* pool, const uint8_t* pool_mask,
                               const float* energy, const float* hq, const uint8_t* qmask, const float* lq,
                               const int32_t* albums, const float* W, const float* b, const float* WH_b, const float* WC_W,
                               const float* WC_b, float* h_a, float* a_logits, float* scale_out, void* workspace,
                               fvta_stream_t stream);

/* Training over the pool under the time warp (simiMatrix 1-3, every warp type, no time_warp_att; with simi 4 the two size
 * queries return 0 and the calls FVTA_ERR_UNSUPPORTED: the per-question route covers it; a warp type outside 1..5: 0 and
 * FVTA_ERR_INVALID_ARG).  The contract is fvta_attn_shared_fwd_tw_train / fvta_attn_shared_bwd_tw's read per REFERENCE
 * (question i, slot m), on the descriptor of fvta_attn_pool_fwd_tw:
 * fvta_attn_pool_fwd_tw_train: the kernels of fvta_attn_pool_fwd_tw -- h_a, a_logits and scale_out are its bits -- with
 *   the ordered plan of fvta_attn_pool_fwd_train, and in the caller-held `saved` (fvta_attn_pool_tw_saved_bytes) what
 *   fvta_attn_pool_fwd_train saves, then scale [NQ,M JX], tanh(z) [NQ,M JX], lin [NQ,K,M JX] (h.Qs + Rh.h at the arg-max,
 *   at the reference's slot) and r2 [P,K,JX] (R2.h^2 of the pooled album's own row).  `workspace`:
 *   fvta_attn_pool_tw_workspace_bytes.
 * fvta_attn_pool_bwd_tw: from d_h_a [NQ,w], for question i what fvta_timewarp_fwd -> fvta_attn_fwd -> fvta_attn_bwd
 *   (accumulate 0, masked rows zero) -> fvta_timewarp_bwd give on (hinfo_i, lq[i], hq[i], ...), hinfo_i the question's M
 *   albums laid end to end; d_pool[p] is the sum of those row gradients -- the attention's and the energy's 2 de v h --
 *   over every reference albums[i,m] == p in plan order (ascending id i M + m; a question that lists p twice contributes
 *   twice), the parameter gradients run over all questions.  d_pool [P,K,JX,w], d_hq [NQ,JQ,w] and d_lq [NQ,w] are
 *   OVERWRITTEN (an album nobody lists: zeros; a question that lists nothing: d_hq = 0 and d_lq = 0); dW [F], db [1], dWH_W
 *   (its first w rows, [w,w]; rows w..2w-1 are not touched), dWH_b [w], dWC_W [w] and dWC_b [1] are accumulated into.
 *   The count of a position is that of the global position m JX + j of the question's M JX: a band, past or future runs
 *   across slot boundaries.  The positions of an empty slot are zero rows: their dz is 0 and they add nothing to db; the
 *   kernels take that from the slot itself, never from memory no launch has written.  fvta_attn_shared_bwd_tw's
 *   deviations and its db carry over; window_t has no gradient; the energy is not an argument.  No [NQ,K,M JX,w]-sized
 *   buffer in either direction: each d_pool row is written once by the row pass and read and written once more by the
 *   energy's backward.  No floating-point atomics, fixed summation order: two calls are bitwise equal in all nine outputs,
 *   and at M = 1 the outputs and `saved` are the shared warped pair's bits for (A = P, T = JX).  No host synchronisation,
 *   no memset.  `workspace`: fvta_attn_pool_tw_bwd_workspace_bytes (the unwarped pooled backward's, then the warp's
 *   arrays: ds / dx s / dbt [NQ,K,M JX], dz [NQ,M JX], de [P,JX] and the small vectors). */
size_t fvta_attn_pool_tw_saved_bytes(const fvta_attn_pool_tw_desc* d);         /* 0 bytes: see fvta_last_error */
size_t fvta_attn_pool_tw_bwd_workspace_bytes(const fvta_attn_pool_tw_desc* d); /* 0 bytes: see fvta_last_error */
int fvta_attn_pool_fwd_tw_train(const fvta_attn_pool_tw_desc* d, const float* pool, const uint8_t* pool_mask,
                                const float* energy, const float* hq, const uint8_t* qmask, const float* lq,
                                const int32_t* albums, const float* W, const float* b, const float* WH_b, const float* WC_W,
                                const float* WC_b, float* h_a, float* a_logits, float* scale_out, void* saved, void* workspace,
                                fvta_stream_t stream);
int fvta_attn_pool_bwd_tw(const fvta_attn_pool_tw_desc* d, const float* pool, const uint8_t* pool_mask, const float* hq,
                          const uint8_t* qmask, const float* lq, const int32_t* albums, const float* W, const float* b,
                          const float* WH_W, const float* WH_b, const float* WC_W, const float* WC_b, const float* d_h_a,
                          const void* saved, float* d_pool, float* d_hq, float* d_lq, float* dW, float* db, float* dWH_W,
                          float* dWH_b, float* dWC_W, float* dWC_b, void* workspace, fvta_stream_t stream);

/* ------------------------------------------------------------------------- *
 * bi-LSTM modality encoders: model_v2.py:652-661 (cells), 667-678 (lengths),
 * 694/732/747/760/774/789/802/823 (the eight bidirectional_dynamic_rnn calls)
 * and the context-tensor assembly 863-914 (outputs are written straight into
 * the padded `hall` layout, so tf.pad/tf.stack never happen).
 *
 * One call runs every sequence that shares a cell (all 7 text streams of
 * model_v2.py:692-812 in ONE call; the photo stream in a second call with
 * `cell_img`).  Sequence s reads x + x_off[s] (+ t*in) and writes
 * out + out_off[s] (+ t*out_ld): forward half at [0,d), backward half at
 * [d,2d) of each output row; rows t >= len[s] (up to seq_J[s]) are zeroed as
 * dynamic_rnn does.
 * ------------------------------------------------------------------------- */
typedef struct fvta_lstm_desc {
  int32_t B;           /* sequences */
  int32_t J;           /* max padded steps over the call */
  int32_t in;          /* input features, multiple of 4 */
  int32_t d;           /* hidden size, multiple of 32 */
  int32_t share_fw_bw; /* 1: TF>=1.2 cell reuse, one kernel for both directions */
  int32_t precision;   /* FVTA_F32 | FVTA_BF16 | FVTA_BF16X3 */
  int32_t training;    /* 1: keep gate activations for fvta_bilstm_bwd */
  int32_t reserved;    /* profiling tag: this call's brackets are filed under id + 16*reserved */
  int32_t dx_overwrite; /* fvta_bilstm_bwd*: 0 = dx is accumulated into (the caller zeroes it), 1 = dx is WRITTEN: every row
                        * t < seq_J of every sequence (both copies under fvta_lstm_plan_xdir) holds the input gradient
                        * afterwards, zeros at t >= len, whatever it held before -- the caller's memset and, where the
                        * kernel writes both directions' sum at once, the read of dx go away */
  int32_t out_pads_persist; /* fvta_bilstm_fwd: 1 = the caller promises that nothing but this op writes `out` between forward
                        * calls on this plan memory: only the rows the previous call wrote and this one does not are zeroed
                        * (rows t >= len are zero after every call either way).  Under this flag the forward WRITES the plan
                        * (per sequence: how far the last forward wrote, into which `out`), although it takes it as const:
                        * (1) one plan must not be used by two forwards at once (two streams would race on that state);
                        * (2) the state is keyed by the output row's ADDRESS -- if `out` is freed and another buffer with
                        *     other contents comes back at the same address while the plan memory is kept, stale rows are not
                        *     zeroed: zero the plan memory (fvta_lstm_plan_bytes) whenever `out` is re-allocated, which also
                        *     is the way to invalidate the state; (3) the plan memory must start zeroed. */
  int64_t out_skip;    /* fvta_bilstm_fwd (FVTA_BF16 only): output half-rows at element offsets BELOW this are not stored into
                        * `out` (nor zeroed) -- their readers take the bf16 shadow rows the forward writes anyway
                        * (fvta_lstm_shadow_rows; the focal attention through fvta_attn_fwd_shadow / fvta_attn_bwd_shadow).
                        * 0: every row is stored.  The fp32 store of h is the single largest store of the forward step
                        * (4 of its 18 bytes per row and unit; the step is store-bound: 119 -> 100 us per launch). */
} fvta_lstm_desc;

size_t fvta_lstm_plan_bytes(const fvta_lstm_desc* d);
size_t fvta_lstm_saved_bytes(const fvta_lstm_desc* d);
size_t fvta_lstm_workspace_bytes(const fvta_lstm_desc* d);

/* Length-sorted schedule for one call (device side, no host sync).
 * len [B] int32 (mask row sums, model_v2.py:667-678), seq_J [B] padded length
 * of each sequence, x_off/out_off [B] element offsets, out_ld row stride.
 * Contract: 0 <= len[b] <= seq_J[b] <= J.  The plan clamps len to [0, J] only: a sequence with seq_J[b] < len[b] would
 * run (and write rows) past its own seq_J rows, into whatever the arenas hold behind them. */
int fvta_lstm_plan(const fvta_lstm_desc* d, const int32_t* len, const int32_t* seq_J, const int64_t* x_off,
                   const int64_t* out_off, int64_t out_ld, void* plan, fvta_stream_t stream);

/* The same with a separate input for the backward direction: its rows are read (and its dx rows written) x_bw_delta
 * ELEMENTS behind the forward direction's, i.e. the caller passes x = [x_fw | x_bw] and dx = [dx_fw | dx_bw] with
 * x_bw_delta = the size of one copy (a multiple of 4).  This is how DropoutWrapper(cell, input_keep_prob) enters
 * (model_v2.py:657-661): bidirectional_dynamic_rnn calls the wrapped cell in two loops, so each direction sees its own
 * dropped copy of the inputs -- fvta_dropout_pair_fwd makes the two copies, fvta_dropout_pair_bwd folds [dx_fw | dx_bw]
 * back.  x_bw_delta = 0 is fvta_lstm_plan. */
int fvta_lstm_plan_xdir(const fvta_lstm_desc* d, const int32_t* len, const int32_t* seq_J, const int64_t* x_off,
                        const int64_t* out_off, int64_t out_ld, int64_t x_bw_delta, void* plan, fvta_stream_t stream);
/* x2[dir][e] = x[e] * keep(dir, e) / keep_prob, dir = 0 / 1, e < n (tf.nn.dropout's x / keep_prob * floor(keep_prob + u)
 * with u from a counter-based hash of (seed, dir, e) -- TensorFlow's random stream is not reproducible, its distribution
 * is; oracle/fvta_fused.py dropout_keep_masks evaluates the same hash).  Backward: dx[e] (+)= sum_dir dx2[dir][e] *
 * keep(dir, e) / keep_prob. */
int fvta_dropout_pair_fwd(const float* x, float* x2, int64_t n, float keep_prob, uint64_t seed, fvta_stream_t stream);
int fvta_dropout_pair_bwd(const float* dx2, float* dx, int64_t n, float keep_prob, uint64_t seed, int32_t accumulate,
                          fvta_stream_t stream);

/* kernel [in+d, 4d] gate order i,j,f,o; bias [4d]; forget_bias 1.0 added at
 * run time (BasicLSTMCell).  kernel_bw/bias_bw ignored when
 * share_fw_bw. */
int fvta_bilstm_fwd(const fvta_lstm_desc* d, const void* plan, const float* x, float* out,
                    const float* kernel_fw, const float* bias_fw, const float* kernel_bw,
                    const float* bias_bw, void* saved, void* workspace, fvta_stream_t stream);

/* d_out has out's layout.  dx (x's layout, may be NULL), dkernel and dbias are
 * all ACCUMULATED INTO (the caller zeroes them once per step); dx is written instead under desc.dx_overwrite. */
int fvta_bilstm_bwd(const fvta_lstm_desc* d, const void* plan, const float* x, const float* out,
                    const float* d_out, const float* kernel_fw, const float* kernel_bw, void* saved,
                    float* dx, float* dkernel_fw, float* dbias_fw, float* dkernel_bw, float* dbias_bw,
                    void* workspace, fvta_stream_t stream);

/* The same signature with a second stream.  `side_stream` is ACCEPTED AND UNUSED (kept for ABI stability): running dx and
 * the weight gradient beside the recurrence measured slower, so everything runs on `stream`; results are bitwise those
 * of fvta_bilstm_bwd.  How dx is summed (bf16 engines, no atomics anywhere): when the two directions share one input (no
 * input dropout) ONE launch adds both directions in the same accumulators and writes every dx element once; the k-tile
 * order of that sum is rotated per workgroup, so the result is deterministic for a given batch but its last bits depend
 * on where a row's tile sits in the grid (a row moved to another position of the batch may round differently).  With a
 * separate input per direction (fvta_lstm_plan_xdir) two launches write one dx copy each. */
int fvta_bilstm_bwd_overlap(const fvta_lstm_desc* d, const void* plan, const float* x, const float* out,
                            const float* d_out, const float* kernel_fw, const float* kernel_bw, void* saved,
                            float* dx, float* dkernel_fw, float* dbias_fw, float* dkernel_bw, float* dbias_bw,
                            void* workspace, fvta_stream_t stream, fvta_stream_t side_stream);

/* The same with what the HOST knows about the batch: nactive_host[t] (host memory, J entries, or NULL) = sequences with
 * len > t, read while the call enqueues its launches.  The plan is built on the device without a host sync, so the
 * library cannot size a step's launch by its active rows itself; with the hint the backward recurrence gives a step
 * with few active rows the small block tile (bf16 engine; results are bitwise those of fvta_bilstm_bwd_overlap: the
 * order of every sum is the same).  A wrong hint costs time, never correctness.  The library acts on it only under
 * FVTA_LSTM_BWD_HINT=1: measured on ragged batches the shorter text-cell launches lengthen the step, whose end is the
 * photo cell's chain of small launches on the side stream. */
int fvta_bilstm_bwd_hint(const fvta_lstm_desc* d, const void* plan, const float* x, const float* out,
                         const float* d_out, const float* kernel_fw, const float* kernel_bw, void* saved,
                         float* dx, float* dkernel_fw, float* dbias_fw, float* dkernel_bw, float* dbias_bw,
                         void* workspace, fvta_stream_t stream, fvta_stream_t side_stream, const int32_t* nactive_host);

/* Final states = concat(fw .h at t=len-1, bw .h at t=0) of sequences
 * [s0, s0+count): lq model_v2.py:697, lchoices 807-812.  dst [count, 2d]. */
/* The bf16 shadow rows of a call's output (bf16 engine): table [2][nrows] of device addresses -- table[dir][row] points at
 * the d bf16 values that are the output half-row `dir` of output row `row` (= element offset / out_ld) for every row this
 * plan writes below nrows (rows t < len); entries of other rows are left untouched: initialise the table with the address of
 * d zero bf16 values (the rows dynamic_rnn zeroes).  Valid until the next forward on `saved`.  model_v2.py:863-914's
 * context tensor is then never materialised in fp32: fvta_attn_fwd_shadow / fvta_attn_bwd_shadow read these rows. */
int fvta_lstm_shadow_rows(const fvta_lstm_desc* d, const void* plan, const void* saved, int64_t nrows, uint64_t* table,
                          fvta_stream_t stream);
/* out [nrows, out_ld] fp32 <- the rows behind such a table (inspection outputs: Tester.step_vis' hall, tests). */
int fvta_rows_from_shadow(const uint64_t* table, int64_t nrows, int32_t d, int64_t out_ld, float* out, fvta_stream_t stream);
int fvta_lstm_last_state(const fvta_lstm_desc* d, const void* plan, const float* out, int32_t s0,
                         int32_t count, float* dst, fvta_stream_t stream);
/* d_out[...] += d_dst at the same places. */
int fvta_lstm_last_state_bwd(const fvta_lstm_desc* d, const void* plan, const float* d_dst, int32_t s0,
                             int32_t count, float* d_out, fvta_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Answer scorer + loss: model_v2.py:1053-1083 (logits/yp) and 1085-1096
 * (softmax cross-entropy, mean over ALL N rows).
 *   gq [N,w], g1 [N,w], gch [N,C,w], W [5w] (7w with use_eu_output), b [1],
 *   y [N,C] bytes (NULL at test time) -> logits [N,C], yp [N,C], loss [1].
 * ------------------------------------------------------------------------- */
typedef struct fvta_scorer_desc {
  int32_t N, C, w;
  int32_t use_eu_output; /* model_v2.py:1071-1073 */
  int32_t add_tanh;      /* only with use_eu_output */
  int32_t xent_grad;     /* backward only.  0: d logits = softmax - labels on EVERY row, what TF-1's
                          * SoftmaxCrossEntropyWithLogits kernel returns (model_v2.py:1088) -- rows whose labels are all
                          * False (the padded rows of a short batch, model_v2.py:1270) still push softmax/N into the
                          * scorer; 1: the gradient of -sum(y log softmax) proper, softmax * sum(y) - y */
} fvta_scorer_desc;

int fvta_scorer_ce_fwd(const fvta_scorer_desc* d, const float* gq, const float* g1, const float* gch,
                       const float* W, const float* b, const uint8_t* y, float* logits, float* yp,
                       float* loss, fvta_stream_t stream);
/* d loss = loss_scale (a host scalar: 1 for a single GPU, 1/world under data
 * parallelism).  dgq/dg1 [N,w], dgch [N,C,w] overwritten; dW, db accumulated. */
int fvta_scorer_ce_bwd(const fvta_scorer_desc* d, const float* gq, const float* g1, const float* gch,
                       const float* W, const float* b, const uint8_t* y, const float* logits,
                       const float* yp, float loss_scale, float* dgq, float* dg1, float* dgch, float* dW,
                       float* db, fvta_stream_t stream);

/* ------------------------------------------------------------------------- *
 * AttentionGRUCell.__call__: attention_gru_cell.py:50-70 (one step).
 *   inputs [B,d+1] (last column = attention gate g), state [B,d],
 *   Wg [2d,d] + bg [d] (gates), Wc [d,d] (candidate, no bias), Wi [d,d] + bi [d]
 * ------------------------------------------------------------------------- */
int fvta_attgru_fwd(int32_t B, int32_t d, const float* inputs, const float* state, const float* Wg,
                    const float* bg, const float* Wc, const float* Wi, const float* bi, float* new_h,
                    float* saved /* [B,3d]: r, hWc, h_hat */, fvta_stream_t stream);
int fvta_attgru_bwd(int32_t B, int32_t d, const float* inputs, const float* state, const float* Wg,
                    const float* Wc, const float* Wi, const float* saved, const float* d_new_h,
                    float* d_inputs, float* d_state, float* dWg, float* dbg, float* dWc, float* dWi,
                    float* dbi, void* workspace /* B*4d floats */, fvta_stream_t stream);

/* ------------------------------------------------------------------------- *
 * The AttentionGRU over a whole fact sequence: exactly F applications of the cell above with the state carried between
 * them (dynamic_rnn over the facts, model_dmnplus.py:123-134), forward and backward.
 *   facts [N,F,d]  gate [N,F] (the attention times `t < length`: a gate of 0 copies the state through, so the op takes
 *   no lengths)  h0 [N,d] or NULL (zeros)  Wg [2d,d] bg [d] Wc [d,d] Wi [d,d] bi [d]  ->  h_last [N,d]
 * The input-side products run once for all N*F rows ahead of the recurrence, the parameter and fact gradients as
 * contractions over all N*F rows after the reverse recurrence.  The recurrence has two regimes, by d (fvta_attgru_seq_plan):
 *   0: every d <= 128 -- ONE launch for all F steps, [Wg[d:] | Wc] resident in LDS, the state tile on chip;
 *   1: larger d -- one fused launch per step (state-side product + gate math; backward: gate gradient + d_h product).
 * Exact fp32 (v_mfma_f32_16x16x4_f32), no atomics, fixed summation order: two runs are bitwise equal.
 * training = 0: nothing is saved, `saved` may be NULL, and there is no backward.
 * ------------------------------------------------------------------------- */
typedef struct {
  int32_t N, F, d;
  int32_t training; /* 1: the forward fills `saved` for fvta_attgru_seq_bwd */
} fvta_attgru_seq_desc;

size_t fvta_attgru_seq_saved_bytes(const fvta_attgru_seq_desc* d); /* 0 with training = 0 */
size_t fvta_attgru_seq_workspace_bytes(const fvta_attgru_seq_desc* d, int32_t backward); /* 0: of _fwd, 1: of _bwd */
/* out[4] = {regime (0 / 1), launches of a forward, launches of a backward with accumulate = 0, rows per workgroup tile} */
int fvta_attgru_seq_plan(const fvta_attgru_seq_desc* d, int32_t* out);
int fvta_attgru_seq_fwd(const fvta_attgru_seq_desc* d, const float* facts, const float* gate, const float* h0,
                        const float* Wg, const float* bg, const float* Wc, const float* Wi, const float* bi,
                        float* h_last, void* saved, void* workspace, fvta_stream_t stream);
/* From d_h_last [N,d]: d_facts [N,F,d], d_gate [N,F] and d_h0 [N,d] (may be NULL) are overwritten; dWg, dbg, dWc, dWi,
 * dbi are stored (accumulate = 0) or added to (1).  `saved` is only read: a second backward gives the same result. */
int fvta_attgru_seq_bwd(const fvta_attgru_seq_desc* d, const float* facts, const float* gate, const float* Wg,
                        const float* Wc, const float* Wi, const void* saved, const float* d_h_last, float* d_facts,
                        float* d_gate, float* d_h0, float* dWg, float* dbg, float* dWc, float* dWi, float* dbi,
                        int32_t accumulate, void* workspace, fvta_stream_t stream);

/* ------------------------------------------------------------------------- *
 * A GRU over a whole sequence: TensorFlow 1's GRUCell under dynamic_rnn(sequence_length=lens), the cell the DMN+ baseline
 * instantiates for its encoders and for the fusion of the facts (model_dmnplus.py:344-345, 470-471):
 *   [r | u] = sigmoid([x_t, h] Wg + bg)      Wg [in+d, 2d], bg [2d] (TF initialises it to 1)
 *   c       = tanh([x_t, r * h] Wc + bc)     Wc [in+d, d],  bc [d]
 *   h'      = u * h + (1 - u) * c
 * PARITY UNPINNED: there is no TensorFlow to compare with, so these formulas (tensorflow/python/ops/rnn_cell_impl.py,
 * GRUCell.call, with its `gates` / `candidate` kernels) are the contract; the tests check them against an fp64 restatement.
 *   x [N,T,in]  lens int32 [N] or NULL (every row has length T)  h0 [N,d] or NULL (zeros)
 *   -> out [N,T,d] (may be NULL), h_last [N,d]
 * At a step t >= lens[n] the state of row n is carried and out[n,t] is zero; h_last[n] is the state after step
 * lens[n] - 1 (h0, or zero, when lens[n] == 0).  reverse = 1 is the backward half of bidirectional_dynamic_rnn: row n is
 * walked from lens[n] - 1 down to 0, out[n,t] is the state after consuming positions lens[n]-1 .. t, padded rows are zero;
 * the op indexes, it does not copy.
 * The input-side products run once for all N*T rows ahead of the recurrence, d_x and the parameter gradients as
 * contractions over all N*T rows after the reverse recurrence.  The recurrence is two dependent products per step and has
 * two regimes, by d (fvta_gru_seq_plan):
 *   0: every d <= 128 -- ONE launch for all T steps, the state-side weights in registers, the state tile in LDS;
 *   1: larger d -- two fused launches per step (one per product, the gate math as epilogue).
 * Exact fp32 (v_mfma_f32_16x16x4_f32), no atomics, fixed summation order: two runs are bitwise equal.
 * training = 0: nothing is saved, `saved` may be NULL, and there is no backward.
 * ------------------------------------------------------------------------- */
typedef struct {
  int32_t N, T, in_dim, d;
  int32_t reverse;  /* 0 / 1 */
  int32_t training; /* 1: the forward fills `saved` for fvta_gru_seq_bwd */
} fvta_gru_seq_desc;

size_t fvta_gru_seq_saved_bytes(const fvta_gru_seq_desc* d); /* 0 with training = 0 */
size_t fvta_gru_seq_workspace_bytes(const fvta_gru_seq_desc* d, int32_t backward); /* 0: of _fwd, 1: of _bwd */
/* out[4] = {regime (0 / 1), launches of a forward, launches of a backward with accumulate = 0, rows per workgroup tile} */
int fvta_gru_seq_plan(const fvta_gru_seq_desc* d, int32_t* out);
int fvta_gru_seq_fwd(const fvta_gru_seq_desc* d, const float* x, const int32_t* lens, const float* h0, const float* Wg,
                     const float* bg, const float* Wc, const float* bc, float* out, float* h_last, void* saved,
                     void* workspace, fvta_stream_t stream);
/* From d_out [N,T,d] and d_h_last [N,d] (either may be NULL, not both): d_x [N,T,in] and d_h0 [N,d] (may be NULL) are
 * overwritten; dWg, dbg, dWc, dbc are stored (accumulate = 0) or added to (1).  `saved` is only read: a second backward
 * gives the same result. */
int fvta_gru_seq_bwd(const fvta_gru_seq_desc* d, const float* x, const int32_t* lens, const float* Wg, const float* Wc,
                     const void* saved, const float* d_out, const float* d_h_last, float* d_x, float* d_h0, float* dWg,
                     float* dbg, float* dWc, float* dbc, int32_t accumulate, void* workspace, fvta_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Compact bilinear pooling: model_mcb.py:1254-1363 `compact_bilinear_pooling_layer` without its sum pool, and with
 * normalize = 1 the `tf.nn.l2_normalize(tf.sqrt(tf.sign(g) * g), dim=-1)` of :645 fused behind it.  The reference takes
 * two count sketches through FFTs of length D; their circular convolution is the count sketch of the outer product, and
 * that is what runs here, in exact fp32 with a fixed summation order (no FFT):
 *   z[r,k] = sum over (i,j) with (h1[i] + h2[j]) mod D = k of  s1[i] s2[j] x[r,i] q[n,j],   n = r / P
 *   x [N*P, d1]   q [N, d2]: shared by the P rows of its n (P = 1 is the general per-row layer)
 *   device tables h1 [d1], h2 [d2]: int32 in [0, D);  s1 [d1], s2 [d2]: +1 / -1.  The kernels trust them: a binding
 *   validates them on the host (ops.CompactBilinear does).
 *   normalize = 0: out = z [N*P, D]
 *   normalize = 1: out = y = w * rsqrt(max(sum_k w_k^2, 1e-12)), w = sqrt|z| (sum w^2 is taken as sum |z|).  The sign is
 *     not restored: the reference does not restore it.  A row whose z is all zero (a padded photo, a zero question) gives
 *     y = 0.  z is never written to memory; `saved` keeps one word per row.
 * Backward, from dy [N*P, D]:
 *   dx[r,i] = s1[i] sum_j s2[j] q[n,j] dz[r,(h1[i]+h2[j]) mod D]
 *   dq[n,j] = s2[j] sum_{r in n} sum_i s1[i] x[r,i] dz[r,(h1[i]+h2[j]) mod D]      (rows of n folded in order)
 * with dz = dy, or dy taken through the normalisation.  CONVENTION at z = 0: d w / d z = sign(z) / (2 sqrt|z|) for
 * z != 0 and 0 at z = 0, so dz is 0 at an empty or exactly cancelled bucket.  TensorFlow gives inf / NaN there (the
 * reference's tf.where(is_nan) scrubs only the forward); inputs are taken to be finite.
 * One workgroup owns an output row in LDS, so D is bounded: D <= 16384.  Above it the size queries return 0 and the
 * calls FVTA_ERR_UNSUPPORTED, with a message naming the limit.  d1 and d2 are any value >= 1 (d1 > D, d2 > D are legal).
 * No floating-point atomics: two runs are bitwise equal.
 * ------------------------------------------------------------------------- */
typedef struct {
  int32_t N, P, d1, d2, D;
  int32_t normalize; /* 0 / 1 */
  int32_t training;  /* 1: the forward fills `saved` for fvta_cbp_bwd */
} fvta_cbp_desc;

size_t fvta_cbp_saved_bytes(const fvta_cbp_desc* d); /* 0 with training = 0 or normalize = 0 */
size_t fvta_cbp_workspace_bytes(const fvta_cbp_desc* d, int32_t backward); /* 0: of _fwd, 1: of _bwd; 0 bytes: see fvta_last_error */
int fvta_cbp_fwd(const fvta_cbp_desc* d, const float* x, const float* q, const int32_t* h1, const float* s1,
                 const int32_t* h2, const float* s2, float* out, void* saved, void* workspace, fvta_stream_t stream);
/* dx [N*P, d1] and dq [N, d2] (either may be NULL, not both) are stored (accumulate = 0) or added to (1).  `saved` is only
 * read (it may be NULL with normalize = 0): a second backward gives the same result. */
int fvta_cbp_bwd(const fvta_cbp_desc* d, const float* x, const float* q, const int32_t* h1, const float* s1,
                 const int32_t* h2, const float* s2, const void* saved, const float* dy, float* dx, float* dq,
                 int32_t accumulate, void* workspace, fvta_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Time warp of the context tensor: model_v2.py:953-1009 with the indicator of
 * time_indication_func (301-341), in the closed form the reference's expression
 * reduces to:  warp_h[n,k,t,:] = hall[n,k,t,:] * c[n,t] * cnt(t).
 *   hall / warp_h / d_* [N,K,T,w]; lq [N,w] (WQ = lq, model_v2.py:970);
 *   WH_W [2w,w] (only its first w rows ever meet a non-zero feature), WH_b [w],
 *   WC_W [w], WC_b [1]: time_warp/{WH,WC}/{W,b}; window_t: time_warp_window_t
 *   (no gradient: tf.ceil, model_v2.py:335).  c_out / scale_out [N,T] are kept
 *   by the caller for the backward call.
 * ------------------------------------------------------------------------- */
typedef struct fvta_timewarp_desc {
  int32_t N, K, T, w;
  int32_t warp_type; /* 1 all, 2 current, 3 past, 4 future, 5 past-future window */
  float window_t;
} fvta_timewarp_desc;

size_t fvta_timewarp_workspace_bytes(const fvta_timewarp_desc* d);
int fvta_timewarp_fwd(const fvta_timewarp_desc* d, const float* hall, const float* lq, const float* WH_W,
                      const float* WH_b, const float* WC_W, const float* WC_b, float* warp_h, float* c_out,
                      float* scale_out, void* workspace, fvta_stream_t stream);
/* d_hall is overwritten; d_lq and the parameter gradients are accumulated into. */
int fvta_timewarp_bwd(const fvta_timewarp_desc* d, const float* hall, const float* lq, const float* WH_W,
                      const float* WH_b, const float* WC_W, const float* WC_b, const float* c_saved,
                      const float* d_warp, float* d_hall, float* d_lq, float* dWH_W, float* dWH_b, float* dWC_W,
                      float* dWC_b, void* workspace, fvta_stream_t stream);
/* The same warp over the bi-LSTM's bf16 SHADOW ROWS (fvta_lstm_shadow_rows; model_v2.py:953-1009 with the context tensor of
 * 863-914 never stored in fp32): row (n,k,t) is read as two bf16 half-rows through table [2][N*K*T] (device addresses),
 * warp_rows [N*K*T][w] receives the warped rows as bf16 -- the rows fvta_attn_fwd_shadow / fvta_attn_bwd_shadow then read
 * through a table of addresses into warp_rows.  w = 512 or 1024, K <= 8.  The backward takes the attention's fp32 gradient
 * of the warped rows (d_warp [N,K,T,w], zeros on masked rows) and overwrites d_hall; no time_warp_att term. */
int fvta_timewarp_fwd_shadow(const fvta_timewarp_desc* d, const uint64_t* table, const float* lq, const float* WH_W,
                             const float* WH_b, const float* WC_W, const float* WC_b, uint16_t* warp_rows, float* c_out,
                             float* scale_out, void* workspace, fvta_stream_t stream);
int fvta_timewarp_bwd_shadow(const fvta_timewarp_desc* d, const uint64_t* table, const float* lq, const float* WH_W,
                             const float* WH_b, const float* WC_W, const float* WC_b, const float* c_saved,
                             const float* d_warp, float* d_hall, float* d_lq, float* dWH_W, float* dWH_b, float* dWC_W,
                             float* dWC_b, void* workspace, fvta_stream_t stream);

/* The same with the attention's gradient w.r.t. the per-position scale (fvta_attn_bwd_tw's d_tscale, [N,T]; NULL =
 * fvta_timewarp_bwd): use_time_warp_att feeds c[n,t] cnt(t) into the attention as well (model_v2.py:1020). */
int fvta_timewarp_bwd_att(const fvta_timewarp_desc* d, const float* hall, const float* lq, const float* WH_W,
                          const float* WH_b, const float* WC_W, const float* WC_b, const float* c_saved,
                          const float* d_warp, const float* d_scale_att, float* d_hall, float* d_lq, float* dWH_W,
                          float* dWH_b, float* dWC_W, float* dWC_b, void* workspace, fvta_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Context tensor: model_v2.py:863-914, the 12 tf.pad + 2 tf.stack that turn the K encoder outputs
 * into hall [N,K,M,JMAX,w] and hall_mask [N,K,M,JMAX], JMAX = max_k J[k] (:869).  Model never builds it this way (its
 * bi-LSTMs write into the arena); this is the stand-alone form for graphs composed from the functional surface.
 *   streams / masks / d_streams: HOST arrays of K device pointers, passed to the kernel by value (no device table, no
 *   hidden allocation, no copy); streams[k] [N,M,J[k],w] f32, masks[k] [N,M,J[k]] u8.
 * fvta_context_fwd, one launch: hall[n,k,m,j,:] = streams[k][n,m,j,:] for j < J[k], zeros otherwise; hall_mask the same
 *   from masks[k].  Rows are copied whether or not their mask bit is set (tf.pad does; the encoders zero rows past the
 *   length themselves).  masks == NULL together with hall_mask == NULL: no mask is produced; one without the other is
 *   an invalid argument.  Every element of both outputs is written exactly once and none is read (no zero-fill).
 * fvta_context_bwd, one launch: d_streams[k][n,m,j,:] = d_hall[n,k,m,j,:] for j < J[k] (tf.pad's gradient, a slice);
 *   overwritten; an entry d_streams[k] == NULL is skipped.  The mask plays no part.
 * 16-byte loads and stores when w % 4 == 0 and every pointer is 16-byte aligned, 4-byte ones otherwise; every element
 * index is 64-bit (BASELINE.json configs[4]: 3.3 G elements).  N * K * M < 2^31.
 * ------------------------------------------------------------------------- */
#define FVTA_CTX_KMAX 8
typedef struct fvta_context_desc {
  int32_t N, K, M, w;       /* K <= FVTA_CTX_KMAX; w = floats per row, any value >= 1 */
  int32_t J[FVTA_CTX_KMAX]; /* rows per album of stream k (>= 1 for k < K) */
} fvta_context_desc;        /* 48 bytes, twelve int32: a layout with no padding to disagree about */

int fvta_context_fwd(const fvta_context_desc* d, const float* const* streams, const uint8_t* const* masks,
                     float* hall /* [N,K,M,JMAX,w] */, uint8_t* hall_mask /* [N,K,M,JMAX] */, fvta_stream_t stream);
int fvta_context_bwd(const fvta_context_desc* d, const float* d_hall, float* const* d_streams, fvta_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Embedding front-end (model_v2.py:524-645): what turns the
 * reference's token-id feed into the encoder inputs.
 *
 * fvta_embed_fwd replaces, for ALL text inputs of a batch at once (at, ad, when,
 * where, pts, q, choices: model_v2.py:531-620),
 *   tf.nn.embedding_lookup(char_emb, *_c) -> conv1d (52-70: conv2d VALID, +bias,
 *   relu, reduce_max over the width) -> concat([char part, word part]) with the
 *   word table concat([word_emb_mat (trainable, VW rows), existing_emb_mat
 *   (frozen GloVe, VT - VW rows)]) (590).
 * Token t: word_ids[t] in [0, VT), char_ids[t*W .. +W) in [0, VC); its row of
 * cwdim + wdim floats is written at x + tok_off[t] (element offset: the caller
 * lays tokens out as the encoder input arena wants them).  cwdim = 0: use_char
 * off (char_ids / char_emb / filt / bias ignored).  keep_prob is 1.
 *   filt [height, cdim, cwdim] (= TF's [1, height, cdim, cwdim]), bias [cwdim].
 *   argpos [ntok, cwdim] u8 (saved for backward): arg-max window, 255 where the
 *   relu is inactive.  Limits: cwdim <= 128, W <= 64, height*cdim <= 64, VC <= 1024.
 * fvta_embed_bwd: dx rows (same offsets) -> gradients ACCUMULATED into
 *   d_word_emb [VW, wdim] (rows >= VW are frozen; float atomics: the one
 *   order-dependent sum of the library, as TF's own IndexedSlices sum),
 *   d_char_emb [VC, cdim], d_filt, d_bias (fixed-order reductions).
 *   max ties go to the first window (TF splits them), as in the attention.
 * ------------------------------------------------------------------------- */
typedef struct fvta_embed_desc {
  int32_t ntok;
  int32_t W;      /* chars per word (config.max_word_size) */
  int32_t cdim;   /* char_emb_size */
  int32_t cwdim;  /* char_out_size; 0 = no char-CNN */
  int32_t wdim;   /* word_emb_size */
  int32_t VW;     /* trainable word rows */
  int32_t VT;     /* all word rows (trainable + frozen) */
  int32_t VC;     /* char vocabulary */
  int32_t height; /* conv window (5) */
  float keep_prob;       /* conv1d's dropout of the gathered char embeddings while training (model_v2.py:58-62); 0 or 1: off */
  uint64_t dropout_seed; /* element (tok, pos, c) is kept by the counter-based hash of (seed, (tok * W + pos) * cdim + c) */
} fvta_embed_desc;

size_t fvta_embed_workspace_bytes(const fvta_embed_desc* d);
int fvta_embed_fwd(const fvta_embed_desc* d, const int32_t* word_ids, const int32_t* char_ids,
                   const int64_t* tok_off, const float* word_emb, const float* fixed_emb, const float* char_emb,
                   const float* filt, const float* bias, float* x, uint8_t* argpos, fvta_stream_t stream);
int fvta_embed_bwd(const fvta_embed_desc* d, const int32_t* word_ids, const int32_t* char_ids,
                   const int64_t* tok_off, const float* char_emb, const float* filt, const uint8_t* argpos,
                   const float* dx, float* d_word_emb, float* d_char_emb, float* d_filt, float* d_bias,
                   void* workspace, fvta_stream_t stream);

/* Photo features (model_v2.py:634-645): row m of the output, at x + row_off[m]
 * (element offset), = embedding_lookup(image_emb_mat [*, idim], pidx[m]), passed
 * through image_trans_linear W [idim, tdim], b [tdim] (+tanh if add_tanh) when W
 * is not NULL (use_image_trans); with W NULL it is the gathered row itself
 * (tdim = idim).  image_emb_mat is a placeholder in the reference: no gradient.
 * Backward (use_image_trans only): dW, db accumulated; workspace M*tdim floats. */
typedef struct fvta_imgtrans_desc {
  int32_t M, idim, tdim, add_tanh;
} fvta_imgtrans_desc;

int fvta_image_trans_fwd(const fvta_imgtrans_desc* d, const int32_t* pidx, const int64_t* row_off,
                         const float* image_emb_mat, const float* W, const float* b, float* x,
                         fvta_stream_t stream);
int fvta_image_trans_bwd(const fvta_imgtrans_desc* d, const int32_t* pidx, const int64_t* row_off,
                         const float* image_emb_mat, const float* x, const float* dx, float* dW, float* db,
                         void* workspace, fvta_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Parameter update over the flat fp32 parameter buffer: trainer.py:16
 * AdadeltaOptimizer(init_lr) (rho 0.95, eps 1e-8) and the commented-out
 * AdamOptimizer of trainer.py:17.  grad_scale multiplies the gradient first
 * (1/world after the RCCL sum).
 * ------------------------------------------------------------------------- */
int fvta_adadelta_step(float* var, const float* grad, float* accum, float* accum_update, int64_t n,
                       float lr, float rho, float eps, float grad_scale, fvta_stream_t stream);
int fvta_adam_step(float* var, const float* grad, float* m, float* v, int64_t n, float lr, float beta1,
                   float beta2, float eps, int32_t t, float grad_scale, fvta_stream_t stream);
/* add_wd (model_v2.py:347-354; --wd, main.py:105): one l2 term of the "losses" collection for one variable:
 * loss[0] += coef/2 * sum(var^2) (if loss != NULL) and grad += coef * var (if grad != NULL); coef = wd x the number
 * of add_wd calls that cover the variable (the shared char-CNN filter is covered once per conv1d call,
 * model_v2.py:564-571).  Fixed summation order. */
int fvta_weight_decay(const float* var, float* grad, int64_t n, float coef, float* loss, fvta_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Gradient guard: clipping and a skip-on-overflow step with no host synchronisation.  The reference's trainer carries
 * the intent only (trainer.py:24-25, a commented-out tf.clip_by_value over every gradient).  Over the flat gradient:
 *   g'  = grad[i] * grad_scale
 *   g'' = clip_value > 0 ? clamp(g', -clip_value, clip_value) : g'      (a NaN stays a NaN)
 *   norm   = sqrt(sum g''^2)           maxabs = largest finite |g''|
 *   nonfinite = how many raw grad[i] are NaN or +-inf (exact)
 *   factor = clip_norm > 0 ? clip_norm / max(norm, clip_norm) : 1       (tf.clip_by_global_norm; exactly 1.0f below
 *            the threshold; a NaN norm leaves factor = 1, the NaN elements themselves carry on)
 *   apply  = !(skip_nonfinite && (nonfinite > 0 || !isfinite(norm)));   apply ? ++applied : ++skipped
 * fvta_grad_guard makes two launches: a streaming read that leaves one partial per workgroup in `workspace` (plain
 * stores; the grid depends on n alone, so the order of summation is the same on every device and in every run), and one
 * workgroup that adds the partials in double in a fixed order and writes the DEVICE-resident control block.  The
 * guarded steps are fvta_adadelta_step / fvta_adam_step fed with g = g'' * factor, taking grad_scale, clip_value,
 * factor, apply and (Adam) lr_t from that block; with apply == 0 they write nothing.  With factor == 1 and no
 * clip_value they are bit-identical to the unguarded steps called with the same grad_scale.
 * grad needs 4-byte alignment only (any n >= 1); ctl 8-byte.  The caller zeroes ctl once and may preset `applied`
 * (Adam's bias correction uses applied + 1) and `skipped`; every other field is overwritten by each call.
 * ------------------------------------------------------------------------- */
typedef struct fvta_guard_desc {
  float grad_scale;       /* 1/world, as fvta_adadelta_step's grad_scale */
  float clip_value;       /* 0 = off */
  float clip_norm;        /* 0 = off */
  int32_t skip_nonfinite; /* 0 / 1 */
  int32_t adam;           /* 1: also compute lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t), t = applied + 1, in double */
  float lr, beta1, beta2; /* read when adam == 1 */
} fvta_guard_desc;

typedef struct fvta_guard_ctl {
  float grad_scale, clip_value, factor, lr_t; /* what the guarded steps read ... */
  int32_t apply;                              /* ... and 0 = leave var and both slots alone */
  float maxabs;
  double norm;
  int64_t nonfinite;
  int64_t applied, skipped; /* running counters, advanced by every fvta_grad_guard */
} fvta_guard_ctl;

size_t fvta_grad_guard_workspace_bytes(int64_t n); /* 0 (and a message) for n <= 0 */
int fvta_grad_guard(const fvta_guard_desc* d, const float* grad, int64_t n, void* workspace, fvta_guard_ctl* ctl,
                    fvta_stream_t stream);
int fvta_adadelta_step_guarded(float* var, const float* grad, float* accum, float* accum_update, int64_t n, float lr,
                               float rho, float eps, const fvta_guard_ctl* ctl, fvta_stream_t stream);
int fvta_adam_step_guarded(float* var, const float* grad, float* m, float* v, int64_t n, float beta1, float beta2,
                           float eps, const fvta_guard_ctl* ctl, fvta_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Stand-alone forms of the reference's small graph helpers (SURVEY 8b "functional ops"); their backwards follow below.
 * Inside the model they are folded into the attention / scorer / embedding kernels.
 *   fvta_softmax_fwd : softmax(logits) over the last axis, model_v2.py:23-28 (logits viewed as [rows, J])
 *   fvta_softsel_fwd : softsel(target [rows,J,d], logits [rows,J]) -> [rows,d], model_v2.py:39-48
 *   fvta_exp_mask    : val + (1 - mask) * -1e30, utils.py:210-213
 *   fvta_linear_fwd  : flatten(x,1) * W[in,out] + b (+ tanh), model_v2.py:75-100 (b may be NULL)
 * ------------------------------------------------------------------------- */
int fvta_softmax_fwd(const float* logits, float* out, int64_t rows, int32_t J, fvta_stream_t stream);
int fvta_softsel_fwd(const float* target, const float* logits, float* out, int64_t rows, int32_t J, int32_t d,
                     fvta_stream_t stream);
int fvta_exp_mask(const float* val, const uint8_t* mask, float* out, int64_t n, fvta_stream_t stream);
int fvta_linear_fwd(const float* x, const float* W, const float* b, float* y, int64_t M, int32_t in, int32_t out,
                    int32_t add_tanh, fvta_stream_t stream);
/* Backward of fvta_linear_fwd (the `bidrection_squash` / concat linears of model.py:895-991): with dyt = dy, or
 * dy (1 - y^2) under add_tanh (y = the forward output): dx [M,in] = dyt W^T (overwritten, or added to when accumulate_dx),
 * dW [in,out] += x^T dyt, db [out] += sum_m dyt.  dx, dW (with db) may each be NULL. */
int fvta_linear_bwd(const float* x, const float* W, const float* y, const float* dy, float* dx, float* dW, float* db,
                    int64_t M, int32_t in, int32_t out, int32_t add_tanh, int32_t accumulate_dx, fvta_stream_t stream);
/* The same two with x (and dx) rows in blocks: row m starts at (m / rows_per_blk) * blk_stride + (m % rows_per_blk) * in
 * floats -- one context stream's rows inside the model.py graph's [N][all streams] arena (attention_tgif's mlp_h over a
 * stream, model.py:226).  y / dy stay dense [M,out]. */
int fvta_linear_fwd_blk(const float* x, const float* W, const float* b, float* y, int64_t M, int32_t in, int32_t out,
                        int32_t add_tanh, int64_t rows_per_blk, int64_t blk_stride, fvta_stream_t stream);
int fvta_linear_bwd_blk(const float* x, const float* W, const float* y, const float* dy, float* dx, float* dW, float* db,
                        int64_t M, int32_t in, int32_t out, int32_t add_tanh, int32_t accumulate_dx, int64_t rows_per_blk,
                        int64_t blk_stride, fvta_stream_t stream);
/* Backward of fvta_softmax_fwd: dx = p (dp - sum_j p dp), p = the forward output. */
int fvta_softmax_bwd(const float* p, const float* dp, float* dx, int64_t rows, int32_t J, fvta_stream_t stream);
/* sum_j weights[r,j] * target[r,j,:] -> out[r,:] (no softmax): the attended vector of attention_tgif, model.py:236-238 */
int fvta_wsum_fwd(const float* target, const float* weights, float* out, int64_t rows, int32_t J, int32_t d,
                  fvta_stream_t stream);
/* ... with the rows' [J,d] blocks target_ld floats apart, and its backward: d_weights [rows,J] = target . d_out
 * (overwritten; may be NULL), d_target += weights (x) d_out (same layout as target; may be NULL). */
int fvta_wsum_fwd_ld(const float* target, const float* weights, float* out, int64_t rows, int32_t J, int32_t d,
                     int64_t target_ld, fvta_stream_t stream);
int fvta_wsum_bwd(const float* target, const float* weights, const float* d_out, float* d_weights, float* d_target,
                  int64_t rows, int32_t J, int32_t d, int64_t target_ld, fvta_stream_t stream);
/* The feature vector of the DMN+ episode attention, model_dmnplus.py:93-98 (`_get_attention`), for all facts at once:
 * out[n,f,:] = [fact*q, fact*m, |fact-q|, |fact-m|]  (facts [N,F,d], q / m [N,d] -> out [N,F,4d]).  The two
 * fully_connected layers on top of it are fvta_linear_fwd, the softmax over facts fvta_softmax_fwd, the gated recurrence
 * fvta_attgru_seq_fwd over all facts (functional.generate_episode). */
int fvta_dmn_features(const float* facts, const float* q, const float* m, float* out, int32_t N, int32_t F, int32_t d,
                      fvta_stream_t stream);
/* Its backward (d_out [N,F,4d]): d_facts [N,F,d], d_q and d_m [N,d] are ACCUMULATED into (the facts and the question feed
 * every hop, model_dmnplus.py:507-509); |x| has derivative 0 at 0, as tf.abs. */
int fvta_dmn_features_bwd(const float* facts, const float* q, const float* m, const float* d_out, float* d_facts, float* d_q,
                          float* d_m, int32_t N, int32_t F, int32_t d, fvta_stream_t stream);
/* relu and its backward from the OUTPUT y (the memory update tf.layers.dense(..., activation=tf.nn.relu),
 * model_dmnplus.py:511-514; the dense itself is fvta_linear_fwd / _bwd). */
int fvta_relu_fwd(const float* x, float* y, int64_t n, fvta_stream_t stream);
int fvta_relu_bwd(const float* y, const float* dy, float* dx, int64_t n, fvta_stream_t stream);
/* The two shape ops the model.py graph (soft-attention baselines) puts between its attentions, forward and backward of
 * each other:
 *   fvta_rows_reduce    : out[r,:] (+)= scale * sum_j x[r,j,:]   x [rows,J,d], out rows `out_ld` floats apart.
 *                         tf.reduce_mean (model.py:874-885 means of the last states, :907 mean over the K streams) with
 *                         scale 1/J; with scale 1 the backward of the tile below.
 *   fvta_rows_broadcast : out[r,j,:] (+)= scale * v[r,:]         v rows `v_ld` floats apart, out [rows,J,d].
 *                         tf.tile (model.py:262 hq per choice) with scale 1; with scale 1/J the backward of reduce_mean.
 * accumulate != 0 adds into the destination. */
int fvta_rows_reduce(const float* x, float* out, int64_t rows, int32_t J, int32_t d, int64_t out_ld, float scale,
                     int32_t accumulate, fvta_stream_t stream);
int fvta_rows_broadcast(const float* v, float* out, int64_t rows, int32_t J, int32_t d, int64_t v_ld, float scale,
                        int32_t accumulate, fvta_stream_t stream);
/* The reversed direction of attention(..., bidirect=True) / attention_keeprank1(..., bidirect=True) (model_v2.py:184-192,
 * model.py:169-177, 297-307): q_a[r,:] = mean_v softsel(hq[r], a_logits[r,v,:]) over the MASKED logits fvta_attn_fwd
 * returns (a_logits [R,V,JQ], hq [R,JQ,w]; JQ <= 64, V*JQ <= 8192: the reference only runs this branch on short row
 * lists).  Backward: d_q_a [R,w] -> dA [R,V,JQ] (overwritten; the additive mask passes it to the raw logits unchanged)
 * and d_hq (accumulated).  fvta_attn_logits_bwd turns a DENSE logit gradient dA [N,T,JQ] of a K = 1 attention (no tanh,
 * simiMatrix 1-3; hinfo_stride honoured) into d_hinfo, d_hq (accumulated), dW, db (accumulated) -- the max-pooled h_a
 * path stays with fvta_attn_bwd. */
int fvta_attn_qside_fwd(const float* a_logits, const float* hq, float* q_a, int32_t R, int32_t V, int32_t JQ, int32_t w,
                        fvta_stream_t stream);
int fvta_attn_qside_bwd(const float* a_logits, const float* hq, const float* d_q_a, float* dA, float* d_hq, int32_t R,
                        int32_t V, int32_t JQ, int32_t w, fvta_stream_t stream);
size_t fvta_attn_logits_bwd_workspace_bytes(const fvta_attn_desc* d);
int fvta_attn_logits_bwd(const fvta_attn_desc* d, const float* hinfo, const float* hq, const float* W, const float* dA,
                         float* d_hinfo, float* d_hq, float* dW, float* db, void* workspace, fvta_stream_t stream);
/* The dense gradient of the focal logits CUBE: dA [N,K,T,JQ], the gradient of the value fvta_attn_fwd writes to a_logits
 * (model_v2.py:210-298's second result; tester.py:34-36 reads it, a loss on the evidence photos supervises it), at any K,
 * any T, with add_tanh, simiMatrix 1-3, both feat_orders, JQ <= 64, w in {64 .. 2048}; hinfo_stride as in
 * fvta_attn_logits_bwd.  The mask is additive (exp_mask), so dA reaches masked entries too and the call takes no masks;
 * under add_tanh the pre-activation is recomputed (a masked a_logits entry is exactly -1e30).  accumulate = 0: d_hinfo
 * [N,K,T,w] and d_hq [N,JQ,w] (summed over k) are overwritten, nothing of them is read; 1: both are added to.  dW, db are
 * always accumulated into.  Exact fp32, fixed summation order (per-workgroup slabs in `workspace`, no atomics). */
size_t fvta_attn_cube_bwd_workspace_bytes(const fvta_attn_desc* d);
int fvta_attn_cube_bwd(const fvta_attn_desc* d, const float* hinfo, const float* hq, const float* W, const float* b,
                       const float* dA, float* d_hinfo, float* d_hq, float* dW, float* db, int accumulate, void* workspace,
                       fvta_stream_t stream);
/* Backward of fvta_softsel_fwd from d_out [rows,d]: p = softmax(logits) is recomputed (an all -1e30 row is uniform, as in
 * the forward); d_target [rows,J,d] = p (x) d_out, d_logits [rows,J] = p (g - sum_j p g) with g[j] = d_out . target[j].
 * Both are overwritten; either may be NULL. */
int fvta_softsel_bwd(const float* target, const float* logits, const float* d_out, float* d_target, float* d_logits,
                     int64_t rows, int32_t J, int32_t d, fvta_stream_t stream);
/* attention_keeprank1 (model.py:247-314) = the per-(n,k) inner softsel of attention_3d without the softmax over k:
 * after fvta_attn_fwd(desc with K = M) this copies that result, u[N,K,w], out of the saved state. */
int fvta_attn_read_u(const fvta_attn_desc* d, const void* saved, float* u_out, fvta_stream_t stream);
/* Backward of "fvta_attn_fwd, then fvta_attn_read_u" given d_u [N,K,w]: every (n,k) is an attention of its own (no softmax
 * over k), d_hq is summed over k.  Arguments as fvta_attn_bwd; `saved` is what fvta_attn_fwd left, `workspace` has
 * fvta_attn_bwd_u_workspace_bytes (its own size: one k per workgroup at every shape).  accumulate = 0: d_hinfo and d_hq
 * are overwritten (masked rows of d_hinfo get zeros); 1: both are accumulated into; dW, db are always accumulated into.
 * simiMatrix 1-3, both feat_orders, add_tanh, every width, both masks or neither; FVTA_ERR_INVALID_ARG for simiMatrix 4,
 * a non-zero hinfo_stride, N*K > 65535 and any other accumulate.  The deviations of fvta_attn_bwd carry over (first
 * arg-max takes a tie; a fully masked (n,k) passes nothing into its logits).  Fixed summation order, no atomics; db --
 * N K T terms that largely cancel -- is summed in fp64 and rounded once, and the softmax denominators and g.u are recomputed
 * from the rows of hinfo (one more read of the row lists) so that they match the weights the row pass uses.
 * The workspace holds one dQs slab set per (n,k): N K bsplit (256 / min(w/4, 256)) 32 ceil(JQ/32) w floats, cleared on
 * every call -- 136 MB at N K = 1040, w = 64. */
size_t fvta_attn_bwd_u_workspace_bytes(const fvta_attn_desc* d);
int fvta_attn_bwd_u(const fvta_attn_desc* d, const float* hinfo, const float* hq, const uint8_t* hmask, const uint8_t* qmask,
                    const float* W, const float* b, const float* d_u, const void* saved, float* d_hinfo, float* d_hq,
                    float* dW, float* db, int accumulate, void* workspace, fvta_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Test hooks (not part of the reference surface): the MFMA tile engines the
 * LSTM kernels are built from, exposed as plain GEMMs so tests can check the
 * fragment layouts in isolation.  layout 0: C=A[M,K]*B[K,N];
 * 1: C=A[M,K]*B[N,K]^T; 2: C=A[K,M]^T*B[K,N].
 * ------------------------------------------------------------------------- */
int fvta_test_gemm(int32_t precision, int32_t layout, int32_t M, int32_t N, int32_t K, const float* A,
                   const float* B, float* C, fvta_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Opt-in measurement hook (bench.py): while enabled on the calling thread, the
 * kernels below are bracketed by hipEvent pairs recorded on the launch stream.
 * fvta_profile_collect synchronises on them and returns the summed elapsed
 * milliseconds and the number of kernel launches they covered.  The LSTM ids
 * bracket the whole per-step launch sequence of one call (J launches).
 * ------------------------------------------------------------------------- */
#define FVTA_PROF_LSTM_STEP_FWD 1 /* lstm_step_fwd_*  : J launches per fvta_bilstm_fwd */
#define FVTA_PROF_LSTM_STEP_BWD 2 /* the recurrence's step launches of one fvta_bilstm_bwd (fp32 engine: gate + step GEMM, with dx) */
#define FVTA_PROF_LSTM_DW 3       /* weight-gradient GEMM + slab reduce */
#define FVTA_PROF_ATTN_FWD_MAIN 4 /* attn_fwd_main */
#define FVTA_PROF_ATTN_BWD_MAIN 5 /* attn_bwd_main */
#define FVTA_PROF_LSTM_DX 6       /* lstm_dx_bf16: the input gradient of all steps, one launch (bf16 engine) */
int fvta_profile_enable(int32_t on);
int fvta_profile_collect(int32_t id, double* total_ms, int64_t* launches);
/* Test / measurement hook: which bi-LSTM step kernels the bf16 engine may use -- bit 0 the weights-stationary forward
 * (lstm_fwd_wreg_bf16), bit 1 the weights-stationary backward of steps with few rows (lstm_bwd_wreg_bf16), bit 2 the
 * pipelined weights-stationary backward (lstm_bwd_ring_bf16, d = 512); 0 = the tiled kernels for every shape; a negative
 * mask returns to the default (the FVTA_LSTM_WREG environment variable, else every bit set).  Returns the previous mask.
 * Every choice computes the same step (model_v2.py:652-661, 694-823); results differ in the last bits (summation order).
 * Process-wide, not thread-safe.  Not part of the reference surface. */
int fvta_lstm_kernel_select(int32_t mask);
/* Measurement hook: how many backward-step launches of calls with more than 64 sequences (the text cell) ran on which
 * kernel since the last call -- counts[0] the tiled step (lstm_bwd_fused_bf16), counts[1] the pipelined weights-stationary
 * step (lstm_bwd_ring_bf16), counts[2] the round-3 weights-stationary step (lstm_bwd_wreg_bf16); reading resets them.
 * bench.py labels its backward-step roofline by these instead of re-deriving the library's choice.  Process-wide. */
int fvta_lstm_bwd_kernel_counts(int64_t* counts);
/* Test / measurement hook: which focal-attention forward main kernel runs (every choice computes model_v2.py:210-298; the
 * fast kernels' logits carry the 3-term fp16 split, <= 3 2^-22 |h||q| per product).  exact: 1 the exact-fp32 kernel
 * (attn_fwd_main) for every shape, 0 the fast kernels where they cover the shape, negative: the default (environment
 * FVTA_ATTN_EXACT, read once, else 0).  wave16: 0 attn_fwd_rows16, 1 attn_fwd_wave16, 2 / 3 attn_fwd_pair16 with barriers /
 * with its flag hand-shake, negative: the default (FVTA_ATTN_WAVE16, read once, else 3).  Process-wide, not thread-safe. */
int fvta_attn_kernel_select(int32_t exact, int32_t wave16);
/* Measurement hook (bench.py, SURVEY 8d "achievable peak"): one read-only, fully coalesced, non-temporal pass over
 * `bytes` of device memory; the caller times it.  Not part of the reference surface. */
int fvta_probe_hbm_read(const void* buf, size_t bytes, float* sink, fvta_stream_t stream);
/* Measurement hook: `nread` streams read and `nwrite` streams written, bytes_per_stream each, all inside `buf`
 * (which must hold (nread + nwrite) * bytes_per_stream bytes), 16 B per lane, coalesced, non-temporal; the caller times
 * it.  The achievable rate of a mixed read/write stream set -- what the LSTM step epilogues are.  Not part of the
 * reference surface. */
int fvta_probe_hbm_mix(void* buf, size_t bytes_per_stream, int32_t nread, int32_t nwrite, fvta_stream_t stream);
/* Measurement hook (Model side-stream selection): one wave that occupies `stream` for `microseconds` of the 100 MHz
 * wall clock.  Two of them on two streams take one wait if the streams run concurrently (separate hardware queues)
 * and two if HIP mapped both streams onto one queue.  Not part of the reference surface. */
int fvta_probe_spin(int64_t microseconds, fvta_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FVTA_HIP_H */

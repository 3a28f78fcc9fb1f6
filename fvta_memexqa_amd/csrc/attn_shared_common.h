// What the shared-context focal attention's forward (attn_shared.hip) and backward (attn_shared_bwd.hip) agree on: the
// shape, the plan's layout, the forward's buffers and -- in training -- which of them live in the caller-held `saved`.
#pragma once
#include <type_traits>
#include "attn_common.h"

namespace fvta {

constexpr int SH_BN = 256;   // question columns of a group: G * JP
constexpr int SH_NT = 256;
constexpr int SH_CH = 64;    // rows whose softmax weights the weighted-sum kernel stages at a time
constexpr int SH_PLAN_NT = 1024;
constexpr int SH_R = 64;     // rows of a tile of the logits kernel (ShMma::BM)

struct ShShape {
  int A, NQ, K, T, JQ, w, simi, add_tanh, use_mask;
  int JP, G;      // padded question length (32 / 64), questions per group (8 / 4)
  int ntile;      // row tiles of a (k): ceil(T / SH_R)
  int S, rps;     // T splits of the weighted sum, rows per split
  int ngmax;      // upper bound of the number of groups: floor(NR / G) + min(A, NR), at most NR
  // A reference is what a column block of a group's product stands for.  Shared context: a question (M = 1, NR = NQ,
  // TO = T).  Album pool (attn_pool.hip): a (question, slot) pair -- A = P pooled albums of T = JX rows each, M slots per
  // question, NR = NQ M references, TO = M T positions per question
  int M, NR, TO;
};

// the derived words, from A, NQ, K, T, JQ, M
inline void sh_derive(ShShape& s) {
  s.use_mask = 0;
  s.NR = s.NQ * s.M;
  s.TO = s.M * s.T;
  s.JP = s.JQ <= 32 ? 32 : 64;
  s.G = SH_BN / s.JP;
  s.ntile = (s.T + SH_R - 1) / SH_R;
  const int64_t ng = (int64_t)s.NR / s.G + (s.A < s.NR ? s.A : s.NR);
  s.ngmax = (int)(ng < s.NR ? ng : s.NR);
  // about 1024 workgroups of the weighted sum (4 per CU), a split not shorter than one chunk
  int64_t S = (1024 + (int64_t)s.ngmax * s.K - 1) / ((int64_t)s.ngmax * s.K);
  const int maxs = (s.T + SH_CH - 1) / SH_CH;
  if (S > maxs) S = maxs;
  if (S < 1) S = 1;
  s.rps = (int)((s.T + S - 1) / S);
  s.S = (s.T + s.rps - 1) / s.rps;
}

// the descriptor's own words (M = 1: a question is its one reference); sh_check derives the rest
inline ShShape sh_words(const fvta_attn_shared_desc* d) {
  ShShape s{};
  s.A = d->A, s.NQ = d->NQ, s.K = d->K, s.T = d->T, s.JQ = d->JQ, s.w = d->w, s.simi = d->simi, s.add_tanh = d->add_tanh;
  s.M = 1;
  return s;
}

// the pooled call's: A = P pooled albums of T = JX rows each, M slots per question
inline ShShape sh_words(const fvta_attn_pool_desc* d) {
  ShShape s{};
  s.A = d->P, s.NQ = d->NQ, s.K = d->K, s.T = d->JX, s.JQ = d->JQ, s.w = d->w, s.simi = d->simi, s.add_tanh = d->add_tanh;
  s.M = d->M;
  return s;
}

// a reference's question, its first position in that question, and the positions per question (the stride of amax /
// jmax / a_logits / dx); POOL = false: (ref, 0, T)
template <bool POOL>
__device__ __forceinline__ int sh_ref_q(const ShShape& s, int ref) {
  if constexpr (POOL) return ref / s.M;
  return ref;
}
template <bool POOL>
__device__ __forceinline__ int sh_ref_off(const ShShape& s, int ref) {  // first position of the reference in its question
  if constexpr (POOL) return (ref % s.M) * s.T;
  return 0;
}
template <bool POOL>
__device__ __forceinline__ int sh_positions(const ShShape& s) {  // positions per question: the stride of amax / a_logits
  if constexpr (POOL) return s.TO;
  return s.T;
}

// The forward's buffers.  Inference (fvta_attn_shared_fwd) carves all of them from the workspace.  Training
// (fvta_attn_shared_fwd_train) carves what the backward reads from `saved` -- the four training-only pieces included -- and
// only the rest (coef, part, agrp) from the workspace; `bytes` is the workspace's share, `saved_bytes` the other.
struct ShWork {
  float *vecs, *Qs, *ct, *amax, *M, *coef, *part;
  int *acnt, *astart, *agrp, *order, *qslot, *ngroups;
  int4* grp;
  uint8_t* jmax;     // training only (else null): [NQ,K,TO] FIRST arg-max j of the masked (tanh'd) logits
  float *L, *r, *u;  // training only: L [NQ,K] = sum_t exp(amax - M), r [NQ,K] = softmax_k(M), u [NQ,K,w] = inner softsel
  size_t bytes, saved_bytes;
  ShWork(const ShShape& s, void* p) {
    FvtaCarver c(p);
    vecs = c.take<float>((size_t)VEC_COUNT * s.w);
    Qs = c.take<float>((size_t)s.NQ * s.JP * s.w);
    ct = c.take<float>((size_t)s.NQ * s.JP);
    amax = c.take<float>((size_t)s.NQ * s.K * s.TO);
    M = c.take<float>((size_t)s.NQ * s.K);
    coef = c.take<float>((size_t)s.NQ * s.K);
    part = c.take<float>((size_t)s.ngmax * s.K * s.S * s.G * s.w);
    acnt = c.take<int>((size_t)s.A);
    astart = c.take<int>((size_t)s.A);
    agrp = c.take<int>((size_t)s.A);
    order = c.take<int>((size_t)s.NR);
    qslot = c.take<int>((size_t)s.NR);
    ngroups = c.take<int>(1);
    grp = c.take<int4>((size_t)s.ngmax);
    bytes = c.off;
    saved_bytes = 0;
    jmax = nullptr;
    L = r = u = nullptr;
  }
  ShWork(const ShShape& s, void* saved, void* work) {
    FvtaCarver c(saved), v(work);
    const size_t nk = (size_t)s.NQ * s.K;
    amax = c.take<float>(nk * s.TO);   // (the pooled call: M T positions per question, NR = NQ M references)
    jmax = c.take<uint8_t>(nk * s.TO);
    M = c.take<float>(nk);
    L = c.take<float>(nk);
    r = c.take<float>(nk);
    u = c.take<float>(nk * s.w);
    Qs = c.take<float>((size_t)s.NQ * s.JP * s.w);
    ct = c.take<float>((size_t)s.NQ * s.JP);
    vecs = c.take<float>((size_t)VEC_COUNT * s.w);
    grp = c.take<int4>((size_t)s.ngmax);
    order = c.take<int>((size_t)s.NR);
    qslot = c.take<int>((size_t)s.NR);
    ngroups = c.take<int>(1);
    astart = c.take<int>((size_t)s.A);   // an album's questions (references) are order[astart[a] .. + acnt[a])
    acnt = c.take<int>((size_t)s.A);
    saved_bytes = c.off;
    coef = v.take<float>(nk);
    part = v.take<float>((size_t)s.ngmax * s.K * s.S * s.G * s.w);
    agrp = v.take<int>((size_t)s.A);
    bytes = v.off;
  }
};

// Training under the time warp (fvta_attn_shared_fwd_tw_train, fvta_attn_pool_fwd_tw_train): `saved` is the training
// ShWork's share, then these four.  The backward (fvta_attn_shared_bwd_tw, fvta_attn_pool_bwd_tw) reads them; none is the
// size of the rows.  The first three are per question over its TO positions (the pooled call: M T, a reference's at its
// slot; else TO = T); r2 belongs to the rows
struct ShTwSaved {
  float* scale;  // [NQ,TO]   s = tanh(z) cnt(t)
  float* tz;     // [NQ,TO]   tanh(z): cnt(t) >= 1 does not divide out of s exactly
  float* lin;    // [NQ,K,TO] h.Qs[q,j] + Rh.h at j = jmax[q,k,t], before the scale enters
  float* r2;     // [A,K,T]   R2.h^2
  size_t bytes;  // of the whole `saved`
  ShTwSaved(const ShShape& s, const ShWork& wk, void* saved) {
    FvtaCarver c(saved);
    c.off = wk.saved_bytes;
    scale = c.take<float>((size_t)s.NQ * s.TO);
    tz = c.take<float>((size_t)s.NQ * s.TO);
    lin = c.take<float>((size_t)s.NQ * s.K * s.TO);
    r2 = c.take<float>((size_t)s.A * s.K * s.T);
    bytes = c.off;
  }
};

// what the logits kernel takes under the warp: the scale it reads and -- training -- the two pieces it leaves
struct ShTwArgs {
  const float* scale;
  float *lin, *r2;
};

// The workspace under the warp: the inference ShWork's, then scale [NQ,TO], then v [w] (the energy call's)
struct ShTwWork {
  ShWork wk;
  float *scale, *v;
  size_t bytes;
  ShTwWork(const ShShape& s, void* p) : wk(s, p) {
    FvtaCarver c(p);
    c.off = wk.bytes;
    scale = c.take<float>((size_t)s.NQ * s.TO);
    v = c.take<float>((size_t)s.w);
    bytes = c.off;
  }
};

// ---- the checks (attn_shared.hip), ONE ladder for both families.  0: fine, else the status with the message set.  The
// refusal texts are part of the interface and each family keeps its own letters (A/NQ/K/T/JQ/w against
// P/NQ/M/K/JX/JQ/w): `pool` picks them.  s comes in with the descriptor's words (sh_words) and leaves with the derived ones
enum ShLevel {
  SH_FWD,    // the shape
  SH_TRAIN,  // and simiMatrix 1-3: the cosine form has no backward here
  SH_BWD     // and the backward's grids (attn_shared_bwd_kernels.h: ShBwdShape)
};
int sh_check(ShShape& s, bool pool, const char* who, ShLevel level = SH_FWD);
// the same under the time warp: then the warp type (1..5: else FVTA_ERR_INVALID_ARG), the window, the scale kernel's grid
// (TO <= 65535 * 256) and the pooled energy call's
int sh_check_tw(ShShape& s, bool pool, int warp_type, float window_t, const char* who, ShLevel level = SH_FWD);

// what every entry point begins with: the descriptor (D: fvta_attn_shared_desc or fvta_attn_pool_desc) into s, checked
template <class D>
int sh_open(const D* d, const char* who, ShShape& s, ShLevel level = SH_FWD) {
  FVTA_CHECK_ARG(d != nullptr, "%s: null descriptor", who);
  s = sh_words(d);
  return sh_check(s, std::is_same<D, fvta_attn_pool_desc>::value, who, level);
}
template <class D>  // D: fvta_attn_shared_tw_desc or fvta_attn_pool_tw_desc
int sh_open_tw(const D* d, const char* who, ShShape& s, ShLevel level = SH_FWD) {
  FVTA_CHECK_ARG(d != nullptr, "%s: null descriptor", who);
  s = sh_words(&d->shape);
  return sh_check_tw(s, std::is_same<D, fvta_attn_pool_tw_desc>::value, d->warp_type, d->window_t, who, level);
}

// ---- the forward driver (attn_shared.hip): every forward entry point of both families ends in it
struct ShFwdCall {
  const float* rows;          // hinfo [A,K,T,w] / pool [P,K,JX,w]
  const uint8_t* rows_mask;
  const float* hq;
  const uint8_t* qmask;
  const int32_t* index;       // album [NQ] / albums [NQ,M]
  const float *W, *b;
  float *h_a, *a_logits;
  void *saved, *workspace;    // saved: training (else null)
  fvta_stream_t stream;
  // the pool held in bf16 (raw bits, 8-byte aligned) IN PLACE OF rows, which is then null: the pooled inference calls
  // only (sh_forward refuses anything else).  The kernels' ROW = bf16_t instantiations; launches and workspace unchanged
  const bf16_t* rows_bf16 = nullptr;
};
struct ShWarpCall {           // under the time warp: what the scale kernel reads, and where the caller wants the scale
  int warp_type;
  float window_t;
  const float *energy, *lq, *WH_b, *WC_W, *WC_b;
  float* scale_out;
};
int sh_forward(const ShShape& s, bool pool, const char* who, const ShFwdCall& c, const ShWarpCall* warp = nullptr);
// the two launches of e[a,t] over the rows of A albums of T positions: fvta_attn_shared_energy, fvta_attn_pool_energy;
// rows_bf16 in place of rows (then null), as ShFwdCall's: fvta_attn_pool_energy_bf16
int sh_energy(const ShShape& s, const char* who, const float* rows, const float* WH_W, const float* WC_W, float* energy,
              void* workspace, fvta_stream_t stream, const bf16_t* rows_bf16 = nullptr);
// G, SH_R, S, rps (fvta_attn_shared_plan, fvta_attn_pool_plan)
int sh_plan(const ShShape& s, const char* who, int32_t out[4]);

// v[c] = sum_o WH[c][o] WC[o] (attn_shared.hip).  grid ceil(w / 4), 256 threads
__global__ __launch_bounds__(256) void attn_shared_tw_vec_kernel(int w, const float* __restrict__ WH, const float* __restrict__ WC,
                                                                 float* __restrict__ v);

}  // namespace fvta

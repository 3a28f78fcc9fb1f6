// What the shared-context backward (attn_shared_bwd.hip) and the pooled backward (attn_pool.hip) both run: the backward's
// shape and workspace, and the kernel templates of the row and question passes.  ONE copy of each; as in
// attn_shared_kernels.h the two callers differ in what a column block of a group stands for, the compile-time flag POOL:
//   POOL = false  a reference IS a question; amax / jmax / dx are [NQ,K,T]
//   POOL = true   a reference is a (question, slot) pair, id q * M + m, over ONE pooled album's T = JX rows; amax / jmax /
//                 dx are [NQ,K,TO] (TO = M * T) and the reference's positions start at m * T.  The loop of the row pass
//                 over "the album's questions" is the loop over the album's references, in plan order
// With POOL = false the kernels are what they were.  The non-template kernels both callers launch (prep, parameters) stay
// in attn_shared_bwd.hip.
#pragma once
#include "attn_shared_common.h"
#include "attn_bwd_shared.h"

namespace fvta {

constexpr int SHB_CS = 32;            // channels per slice of the question pass
constexpr int SHB_JG = ATTN_BWD_JG;   // question positions per workgroup of the fold
constexpr int SHB_ROW_WGS = 1024;     // about this many workgroups of the row pass (then several tiles per workgroup)
constexpr int SHB_Q_WAVES = 1280;     // about this many waves of the question pass (5 x 32 KB of LDS per CU)

struct ShBwdShape {
  int TPR, CPT, RH, RPT, TR;  // row pass: threads per row, float4 per thread and row, row groups, rows per thread, tile rows
  int ntb, tpw, nch;          // row tiles per (album, k), tiles per workgroup, workgroups per (album, k)
  int nsl, TS, rps;           // question pass: channel slices, T splits, rows per split
  int JZ;                     // fold: groups of SHB_JG question positions
};

static ShBwdShape shb_shape(const ShShape& s) {
  ShBwdShape b;
  b.TPR = s.w / 4 < 256 ? s.w / 4 : 256;
  b.CPT = s.w / (4 * b.TPR);
  b.RH = 256 / b.TPR;
  b.RPT = b.CPT == 1 ? 8 : 4;
  b.TR = b.RH * b.RPT;
  b.ntb = (s.T + b.TR - 1) / b.TR;
  const int64_t tiles = (int64_t)s.A * s.K * b.ntb;
  int64_t tpw = (tiles + SHB_ROW_WGS - 1) / SHB_ROW_WGS;
  if (tpw > b.ntb) tpw = b.ntb;
  if (tpw < 1) tpw = 1;
  b.tpw = (int)tpw;
  b.nch = (b.ntb + b.tpw - 1) / b.tpw;
  b.nsl = s.w / SHB_CS;
  int64_t ts = (SHB_Q_WAVES + (int64_t)s.ngmax * b.nsl - 1) / ((int64_t)s.ngmax * b.nsl);
  const int maxs = (s.T + 63) / 64;
  if (ts > maxs) ts = maxs;
  if (ts < 1) ts = 1;
  b.rps = (int)((s.T + ts - 1) / ts);
  b.TS = (s.T + b.rps - 1) / b.rps;
  b.JZ = (s.JQ + SHB_JG - 1) / SHB_JG;
  return b;
}

struct ShBwdWork {
  float *coef, *gu, *dss;  // [NQ,K]: r / L, g.u[k], ds[k] / ties (0 for a fully masked (question, k))
  float* dx;               // [NQ,K,TO] gradient of the row's winning logit (TO = T outside the pooled call)
  float* qpart;            // [ngmax][TS][G JP = 256][w]  dQs partials
  float* dctp;             // [ngmax][TS][256]            d ct partials
  float* rowp;             // [A K nch][RH][2][w]         d Rh, d R2 partials
  float* pvec;             // [NQ JZ][3][w]               d U, d Cq, d C2 partials
  float* dctn;             // [NQ][JP]
  size_t bytes;
  ShBwdWork(const ShShape& s, const ShBwdShape& b, void* p) {
    FvtaCarver c(p);
    const size_t nk = (size_t)s.NQ * s.K;
    coef = c.take<float>(nk);
    gu = c.take<float>(nk);
    dss = c.take<float>(nk);
    dx = c.take<float>(nk * s.TO);
    qpart = c.take<float>((size_t)s.ngmax * b.TS * SH_BN * s.w);
    dctp = c.take<float>((size_t)s.ngmax * b.TS * SH_BN);
    rowp = c.take<float>((size_t)s.A * s.K * b.nch * b.RH * 2 * s.w);
    pvec = c.take<float>((size_t)s.NQ * b.JZ * 3 * s.w);
    dctn = c.take<float>((size_t)s.NQ * s.JP);
    bytes = c.off;
  }
};

// the pooled backward's workspace: ShBwdWork for the pooled shape, then dctq [NQ,JP]
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

// ---- the backward driver (attn_shared_bwd.hip): fvta_attn_shared_bwd, fvta_attn_shared_bwd_tw, fvta_attn_pool_bwd and
// fvta_attn_pool_bwd_tw end in it
struct ShBwdCall {
  const float* rows;          // hinfo [A,K,T,w] / pool [P,K,JX,w]
  const uint8_t* rows_mask;
  const float* hq;
  const uint8_t* qmask;
  const float* d_h_a;
  const void* saved;
  float *d_rows, *d_hq, *dW, *db;
  void* workspace;
  fvta_stream_t stream;
};
struct ShBwdWarpCall {        // under the time warp: the warp's parameters, the question's state and their gradients
  int warp_type;
  float window_t;
  const float *lq, *WH_W, *WH_b, *WC_W, *WC_b;
  float *d_lq, *dWH_W, *dWH_b, *dWC_W, *dWC_b;
};
int shb_backward(const ShShape& s, bool pool, const char* who, const ShBwdCall& c, const ShBwdWarpCall* warp = nullptr);
// the backward's workspace, `warp`: under the time warp; TR, TS, SHB_CS, tpw (the *_bwd_workspace_bytes / *_bwd_plan pairs)
size_t shb_workspace_bytes(const ShShape& s, bool pool, bool warp = false);
int shb_plan(const ShShape& s, const char* who, int32_t out[4]);

// attn_pool.hip.  3b: grid NQ, 64 threads; 4: grid (NQ, ceil(w / 256), JZ), 256 threads
__global__ __launch_bounds__(64) void attn_pool_bwd_dct_kernel(ShShape s, ShBwdShape bs, ShWork sv, ShBwdWork wk,
                                                              float* __restrict__ dctq);
__global__ __launch_bounds__(256) void attn_pool_bwd_fold_kernel(ShShape s, ShBwdShape bs, ShWork sv, ShBwdWork wk,
                                                                const float* __restrict__ dctq, const float* __restrict__ hq,
                                                                float* __restrict__ d_hq);

// attn_shared_bwd.hip.  grid NQ, 1024 (K > 4) or 256 threads: attn_bwd_shared.h's prep body over s.T positions per
// (question, k) -- the pooled caller passes T = M * JX
__global__ __launch_bounds__(1024) void attn_shared_bwd_prep_kernel(ShShape s, ShWork sv, ShBwdWork wk,
                                                                   const float* __restrict__ d_h_a);
// attn_shared_bwd.hip.  grid ceil(w / 64) + 1, 256 threads: pvec [NQ JZ] and rowp [A K nch RH] in index order -> dW, db
__global__ __launch_bounds__(256) void attn_shared_bwd_params_kernel(ShShape s, ShBwdShape bs, ShBwdWork wk,
                                                                    float* __restrict__ dW, float* __restrict__ db);

// what the row and question passes take under the time warp: the forward's saved pieces, and three arrays [NQ,K,TO] of the
// backward's workspace: ds (the gradient of the scale, per k), dx s (the question pass multiplies the rows by it), dbt (the
// row's term of db, see the row pass)
struct ShBwdTwArgs {
  const float *scale, *lin, *r2;
  float *ds, *dxs, *dbt;
};

// dx s^2 per row of the tile, beside s_pr / s_dx: LDS of the TW instantiations alone
template <int TR>
__device__ __forceinline__ float* shb_tw_d2() {
  __shared__ float s_d2[TR];
  return s_d2;
}

// ---- row pass.  grid A K nch, 256 threads = RH row groups x TPR threads; a thread holds RPT rows x CPT float4
// TW (compile-time): under the time warp the attention saw the rows s h, s = scale[q,t].  pr and dx are what they were, on
// g.(s h); the thread that computes them also reads s, lin and r2 and stores ds = pr g.h + dx (lin + 2 s r2), dx and dx s;
// the rows' gradient takes s pr g + dx s (Qs + Rh) + 2 dx s^2 R2 h, the Rh / R2 partials sum dx s and dx s^2.
// db under the warp is NOT the sum of the d ct: the gradients damax of a question's max-pooled logits sum to zero over
// (k, t) -- two softmaxes -- so sum dx = sum damax (1 - x^2) = - sum damax x^2 under tanh and 0 without.  The warped rows
// are up to cmax times the rows, damax is of order 1 where db is of order 1e-3, and the plain sum kept the fp32 noise of
// that cancellation (1e-5 at w = 512); dbt [NQ,K,T] = - damax x^2 has none to cancel.  d ct per (question, j) stays dx
// POOL (compile-time): the loop runs over the pooled album's references; reference q M + m reads question q's scalars and
// d_h_a, and amax / jmax and writes dx at positions m T + t of q's TO.  A question that lists the album twice stands twice
// in the loop.  TW and POOL: scale, lin, ds, dx s and dbt are per question over its TO positions too, read and written at
// the same m T + t; r2 stays the album's own row
template <int TPR, int CPT, int RPT, bool TW, bool POOL = false>
__global__ __launch_bounds__(256) void attn_shared_bwd_rows_kernel(ShShape s, ShBwdShape bs, ShWork sv, ShBwdWork wk,
                                                                  const float* __restrict__ hinfo,
                                                                  const float* __restrict__ d_h_a,
                                                                  float* __restrict__ d_hinfo, ShBwdTwArgs tw) {
  constexpr int RH = 256 / TPR, TR = RH * RPT;
  constexpr int WPR = TPR >= 64 ? TPR / 64 : 1;  // waves that share a row
  __shared__ float s_dot[4][TR], s_pr[TR], s_dx[TR];
  __shared__ int s_jj[TR];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int cq = tid % TPR, rh = tid / TPR;
  const int ch = blockIdx.x % bs.nch, ak = blockIdx.x / bs.nch, a = ak / s.K, k = ak % s.K;
  const int T = s.T, w = s.w, K = s.K, JP = s.JP;
  const int TP = sh_positions<POOL>(s), NRF = POOL ? s.NR : s.NQ;  // positions per question; references in all
  const int q0 = min(max(sv.astart[a], 0), NRF), nqa = min(sv.acnt[a], NRF - q0);  // (the plan's own numbers; bounded all the same)
  const float* __restrict__ hbase = hinfo + (size_t)ak * T * w;
  float* __restrict__ dhbase = d_hinfo + (size_t)ak * T * w;
  f32x4 rh4[CPT], r24[CPT], accRh[CPT], accR2[CPT];
#pragma unroll
  for (int c = 0; c < CPT; ++c) {
    rh4[c] = ld4(sv.vecs + VEC_RH * w + 4 * (cq + c * TPR));
    r24[c] = ld4(sv.vecs + VEC_R2 * w + 4 * (cq + c * TPR));
    accRh[c] = accR2[c] = zero4();
  }
  const int tile_end = min(bs.ntb, (ch + 1) * bs.tpw);
  for (int tile = ch * bs.tpw; tile < tile_end; ++tile) {
    const int t0 = tile * TR;
    f32x4 h[RPT][CPT], dh[RPT][CPT];
    float sdx[RPT], sdx2[TW ? RPT : 1];
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int t = t0 + rh * RPT + i;
      sdx[i] = 0.f;
      if constexpr (TW) sdx2[i] = 0.f;
#pragma unroll
      for (int c = 0; c < CPT; ++c) {
        h[i][c] = t < T ? ld4(hbase + (size_t)t * w + 4 * (cq + c * TPR)) : zero4();
        dh[i][c] = zero4();
      }
    }
    for (int qi = 0; qi < nqa; ++qi) {
      int ref = sv.order[q0 + qi];
      ref = ref < 0 ? 0 : (ref >= NRF ? NRF - 1 : ref);
      const int q = sh_ref_q<POOL>(s, ref), off = sh_ref_off<POOL>(s, ref);
      f32x4 gv[CPT];
#pragma unroll
      for (int c = 0; c < CPT; ++c) gv[c] = ld4(d_h_a + (size_t)q * w + 4 * (cq + c * TPR));
      // g.h[t]: over the TPR threads of a row
#pragma unroll
      for (int i = 0; i < RPT; ++i) {
        float v = 0.f;
#pragma unroll
        for (int c = 0; c < CPT; ++c) {
          const f32x4 pd = h[i][c] * gv[c];
          v += (pd[0] + pd[1]) + (pd[2] + pd[3]);
        }
#pragma unroll
        for (int o = 1; o < (TPR < 64 ? TPR : 64); o <<= 1) v += __shfl_xor(v, o, 64);
        if (TPR >= 64) {
          if (lane == 0) s_dot[wave][rh * RPT + i] = v;
        } else {
          if (cq == 0) s_dot[0][rh * RPT + i] = v;
        }
      }
      __syncthreads();
      if (tid < TR) {
        const int t = t0 + tid;
        float pr = 0.f, dx = 0.f, sc = 0.f, dbt = 0.f;
        int j = 0;
        if (t < T) {
          float gh = 0.f;
          if (TPR >= 64) {
            const int rgp = tid / RPT;  // row `tid` belongs to row group rgp, whose waves are [rgp WPR, rgp WPR + WPR)
#pragma unroll
            for (int v = 0; v < WPR; ++v) gh += s_dot[rgp * WPR + v][tid];
          } else {
            gh = s_dot[0][tid];
          }
          const size_t qk = (size_t)q * K + k, at = qk * TP + off + t;  // (q, k, the reference's position t)
          const float M = sv.M[qk], am = sv.amax[at];
          if constexpr (TW) sc = tw.scale[(size_t)q * TP + off + t];
          pr = expf(am - M) * wk.coef[qk];
          // pr = 0: a masked row beside valid ones (its g.h may be anything), or r underflowed (then ds is 0 as well)
          if (pr != 0.f && M != FVTA_NEG) {
            const float damax = pr * ((TW ? sc * gh : gh) - wk.gu[qk]) + (am == M ? wk.dss[qk] : 0.f);
            dx = s.add_tanh ? damax * (1.f - am * am) : damax;
            if constexpr (TW) dbt = s.add_tanh ? -(damax * am * am) : 0.f;
          }
          j = min((int)sv.jmax[at], JP - 1);
          wk.dx[at] = dx;
          if constexpr (TW) {  // (pr = 0 beside a g.h that may be anything: no product with it)
            tw.dbt[at] = dbt;
            float ds = pr != 0.f ? pr * gh : 0.f;
            if (dx != 0.f) ds += dx * (tw.lin[at] + 2.f * sc * tw.r2[(size_t)ak * T + t]);
            tw.ds[at] = ds;
            tw.dxs[at] = dx * sc;
          }
        }
        if constexpr (TW) {
          s_pr[tid] = pr * sc;
          s_dx[tid] = dx * sc;
          shb_tw_d2<TR>()[tid] = dx * sc * sc;
        } else {
          s_pr[tid] = pr;
          s_dx[tid] = dx;
        }
        s_jj[tid] = j;
      }
      __syncthreads();
      const float* __restrict__ Qs = sv.Qs + (size_t)q * JP * w;
#pragma unroll
      for (int i = 0; i < RPT; ++i) {
        const int row = rh * RPT + i;
        const float pr = s_pr[row], dx = s_dx[row];
#pragma unroll
        for (int c = 0; c < CPT; ++c) dh[i][c] += gv[c] * pr;
        if (dx != 0.f) {
          const int j = s_jj[row];
#pragma unroll
          for (int c = 0; c < CPT; ++c) {
            const f32x4 qs = ld4(Qs + (size_t)j * w + 4 * (cq + c * TPR));
            if constexpr (TW)
              dh[i][c] += (qs + rh4[c]) * dx + r24[c] * h[i][c] * (2.f * shb_tw_d2<TR>()[row]);
            else
              dh[i][c] += (qs + rh4[c] + r24[c] * h[i][c] * 2.f) * dx;
          }
          sdx[i] += dx;
          if constexpr (TW) sdx2[i] += shb_tw_d2<TR>()[row];
        }
      }
      // (the next question's s_dot is written after this barrier pair, its s_pr / s_dx after the next first barrier, which
      // every thread reaches only when it is through with the reads above)
    }
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int t = t0 + rh * RPT + i;
      if (t < T) {
#pragma unroll
        for (int c = 0; c < CPT; ++c) {
          *reinterpret_cast<f32x4*>(dhbase + (size_t)t * w + 4 * (cq + c * TPR)) = dh[i][c];
          if constexpr (TW) {
            accRh[c] += h[i][c] * sdx[i];
            accR2[c] += h[i][c] * h[i][c] * sdx2[i];
          } else if (sdx[i] != 0.f) {
            accRh[c] += h[i][c] * sdx[i];
            accR2[c] += h[i][c] * h[i][c] * sdx[i];
          }
        }
      }
    }
    __syncthreads();  // the tile's last reads of s_pr / s_dx / s_jj before the next tile's first question
  }
  float* __restrict__ rowp = wk.rowp + ((size_t)blockIdx.x * RH + rh) * 2 * w;
#pragma unroll
  for (int c = 0; c < CPT; ++c) {
    *reinterpret_cast<f32x4*>(rowp + 4 * (cq + c * TPR)) = accRh[c];
    *reinterpret_cast<f32x4*>(rowp + w + 4 * (cq + c * TPR)) = accR2[c];
  }
}

// ---- question pass.  grid ngmax TS nsl, 64 threads: lane = (question g of the group, 4 of the slice's 32 channels)
// TW (compile-time): the rows entered as s h: dQs takes dx s (dxs [NQ,K,TO], the row pass's), d ct dx as it is
// POOL (compile-time): a lane group stands for a REFERENCE of the group's pooled album: dx / jmax are read at the
// reference's positions of its question; the partials stay per (group, split) and the pooled fold adds a question's slots
template <int G, bool TW, bool POOL = false>
__global__ __launch_bounds__(64) void attn_shared_bwd_q_kernel(ShShape s, ShBwdShape bs, ShWork sv, ShBwdWork wk,
                                                              const float* __restrict__ hinfo, const float* __restrict__ dxs) {
  constexpr int JP = SH_BN / G, C4 = SHB_CS / 4;
  __shared__ f32x4 s_acc[SH_BN][C4];
  __shared__ float s_dct[SH_BN];
  const int tid = threadIdx.x;
  const int sl = blockIdx.x % bs.nsl, ts = (blockIdx.x / bs.nsl) % bs.TS, grp = blockIdx.x / (bs.nsl * bs.TS);
  if (grp >= *sv.ngroups) return;
  const int4 gi = sv.grp[grp];
  const int a = min(max(gi.x, 0), s.A - 1), first = gi.y, cnt = min(max(gi.z, 0), G);
  const int T = s.T, w = s.w, K = s.K;
  const int TP = sh_positions<POOL>(s), NRF = POOL ? s.NR : s.NQ;
  for (int e = tid; e < SH_BN * C4; e += 64) (&s_acc[0][0])[e] = zero4();
  for (int e = tid; e < SH_BN; e += 64) s_dct[e] = 0.f;
  __syncthreads();
  // A group with fewer than G questions leaves accumulator regions free: `rep` lane groups then share a question, each
  // taking every rep-th run of four rows into a region of its own, and the regions are added in region order on the way
  // out.  rep depends on the group's count alone.
  const int rep = cnt > 0 ? max(G / cnt, 1) : 1;
  const int gl = tid / C4, c4 = tid % C4;                  // lane group = accumulator region
  const int g = cnt > 0 ? gl % cnt : 0, part = cnt > 0 ? gl / cnt : 0;
  int ref = (gl < G && cnt > 0 && part < rep && g < cnt && first + g < NRF) ? sv.order[first + g] : -1;
  if (ref >= NRF) ref = -1;
  const int q = ref < 0 ? -1 : sh_ref_q<POOL>(s, ref), off = ref < 0 ? 0 : sh_ref_off<POOL>(s, ref);
  const int tb = ts * bs.rps, te = min(T, tb + bs.rps);
  if (q >= 0 && tb < te) {
    for (int k = 0; k < K; ++k) {
      const float* __restrict__ hrow = hinfo + ((size_t)a * K + k) * T * w + sl * SHB_CS + 4 * c4;
      const float* __restrict__ dxp = wk.dx + ((size_t)q * K + k) * TP + off;
      const float* __restrict__ dsp = TW ? dxs + ((size_t)q * K + k) * TP + off : nullptr;
      const uint8_t* __restrict__ jp = sv.jmax + ((size_t)q * K + k) * TP + off;
      for (int t4 = tb + 4 * part; t4 < te; t4 += 4 * rep) {  // four rows in flight
        float dx[4], dm[TW ? 4 : 1];
        int j[4];
        f32x4 h[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int t = min(t4 + i, te - 1);
          dx[i] = t4 + i < te ? dxp[t] : 0.f;
          if constexpr (TW) dm[i] = dsp[t];
          j[i] = min((int)jp[t], JP - 1);
          h[i] = ld4(hrow + (size_t)t * w);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (dx[i] != 0.f) {
            s_acc[gl * JP + j[i]][c4] += h[i] * (TW ? dm[i] : dx[i]);
            if (sl == 0 && c4 == 0) s_dct[gl * JP + j[i]] += dx[i];
          }
      }
    }
  }
  __syncthreads();
  const size_t slot = (size_t)grp * bs.TS + ts;
  float* __restrict__ dst = wk.qpart + slot * SH_BN * w + sl * SHB_CS;
  for (int e = tid; e < SH_BN * C4; e += 64) {
    const int row = e / C4, cc = e % C4, gs = row / JP, j = row % JP;
    f32x4 v = zero4();
    if (gs < cnt)
      for (int p = 0; p < rep; ++p) v += s_acc[(gs + cnt * p) * JP + j][cc];
    *reinterpret_cast<f32x4*>(dst + (size_t)row * w + 4 * cc) = v;
  }
  if (sl == 0)
    for (int e = tid; e < SH_BN; e += 64) {
      const int gs = e / JP, j = e % JP;
      float v = 0.f;
      if (gs < cnt)
        for (int p = 0; p < rep; ++p) v += s_dct[(gs + cnt * p) * JP + j];
      wk.dctp[slot * SH_BN + e] = v;
    }
}

}  // namespace fvta

// Focal attention backward for gfx950 (gradient of model_v2.py:210-298 / 125-201).
//
// Because the logits are max-pooled over the question axis (model_v2.py:268),
// only ONE (t, j) pair per context row carries gradient, so the backward needs
// no GEMM: it is a single streaming pass (read h row, write dh row) with
//   dh[t]  = p[t] r[k] g  +  dx[t] (Qs[jmax[t]] + Rh + 2 R2 h[t])
//   dQs[j] += dx[t] h[t]   for j = jmax[t]
// A workgroup sorts its chunk of rows by jmax so that every thread can keep
// the dQs accumulator of the "current j" in registers and flush it once per j
// into a private slab (no atomics, bitwise reproducible).
//
// Deviation: gradient through reduce_max goes to the FIRST arg-max
// (TF splits exact ties) and fully masked (n,k) rows pass no gradient into the
// masked logits.
//
// What the small kernels here share with attn_shared_bwd.hip -- the prep body, the slot sum, the fold body, the pieces of
// the parameter kernel, the fp64 block sum -- is in attn_bwd_shared.h; the W mapping (attn_bwd_add_dW) and the
// declaration of fvta_attn_check_desc in attn_common.h.
#include "attn_bwd_shared.h"
#include "fvta_prof.h"

#ifndef FVTA_ATTN_BWD_NT_DEFAULT
#define FVTA_ATTN_BWD_NT_DEFAULT 0
#endif

namespace fvta {


constexpr int BWD_CHMAX = 1024;  // rows per backward workgroup chunk (LDS sort capacity)

static inline __host__ __device__ int attn_bwd_jz(const AttnShape& s) { return (s.JQ + ATTN_BWD_JG - 1) / ATTN_BWD_JG; }

struct AttnBwdWork {
  float* coef;   // [N,K]  r / L
  float* gu;     // [N,K]  g . u[k]
  float* dss;    // [N,K]  ds[k] / (#t with amax == M)
  float* slabs;  // [N*ng][bsplit][RH][JP][w]   dQs partials (ng = groups of gk consecutive k per n)
  float* dctp;   // [N*ng][bsplit][RH][JP]      d ct partials
  float* rowp;   // [N*ng][bsplit][RH][2][w]    d Rh, d R2 partials
  float* pvec;   // [N * JZ][5][w]             parameter-vector partials per n and group of 8 question positions
  float* dctn;   // [N][JP]
  float* dscr;   // [N,K,T] time_warp_att: per-row terms of d tscale[n,t] (summed over k in a fixed order afterwards)
  size_t bytes;
  size_t slab_bytes;
};

static inline int bwd_tpr(int W4) { return W4 < 256 ? W4 : 256; }
static inline int bwd_rh(int W4) { return 256 / bwd_tpr(W4); }

static AttnBwdWork bwd_work_view(const AttnShape& s, void* p) {
  FvtaCarver c(p);
  AttnBwdWork v;
  const size_t nk = (size_t)s.N * s.K;
  const int RH = bwd_rh(s.W4);
  v.coef = c.take<float>(nk);
  v.gu = c.take<float>(nk);
  v.dss = c.take<float>(nk);
  v.pvec = c.take<float>((size_t)s.N * attn_bwd_jz(s) * VEC_COUNT * s.w);
  v.dctn = c.take<float>((size_t)s.N * s.JP);
  v.dscr = c.take<float>(nk * s.T);
  const size_t before = c.off;
  const size_t ngr = (size_t)s.N * s.ng;
  v.slabs = c.take<float>(ngr * s.bsplit * RH * s.JP * s.w);
  v.dctp = c.take<float>(ngr * s.bsplit * RH * s.JP);
  v.rowp = c.take<float>(ngr * s.bsplit * RH * 2 * s.w);
  v.slab_bytes = c.off - before;
  v.bytes = c.off;
  return v;
}

// ---- per-(n,k) scalars (attn_bwd_shared.h: attn_bwd_prep_body).  grid N, 1024 threads (256 at K <= 4); a wave per k
__global__ __launch_bounds__(1024) void attn_bwd_prep_kernel(AttnShape s, AttnSaved sv, AttnBwdWork wk,
                                                            const float* __restrict__ d_h_a) {
  const size_t n = blockIdx.x, nk = n * s.K;
  const bool allmasked = (int)threadIdx.x < s.K && sv.allmasked[nk + threadIdx.x];
  attn_bwd_prep_body(d_h_a + n * s.w, sv.u + nk * s.w, sv.M + nk, sv.amax + nk * s.T, sv.r + nk, sv.L + nk, allmasked, s.w, s.K,
                     s.T, wk.coef + nk, wk.gu + nk, wk.dss + nk);
}

// ---- the same scalars when every (n,k) is an attention of its own (fvta_attn_bwd_u): g = d_u[n,k], no softmax over k --
// r[k] = 1 and the k-softmax term dss is 0.  A row's logit gradient is p[t] (g.h[t] - g.u) and sums to 0 over a list; the
// forward's L and u come from an online softmax (products of several expf), so against the weights the main kernel
// recomputes, expf(amax - Mz) / L, they are off by a few 1e-7 per row -- with a gradient vector per (n,k) that is a
// residue of ~1e-6 per list in db, 2.5e-5 at a thousand lists where the result is 0.  So this kernel takes both from the
// weights the main kernel will use: L = sum_t e[t] and g.u = sum_t e[t] (g.h[t]) / L with e[t] = expf(amax[t] - Mz) -- the
// same expression as there -- over the list's rows, in fp64, rounded once.  One more read of the rows (no target here).
// A wave per (n,k), grid ceil(N K / 4); a lane sums its channels over all rows, one wave reduction at the end.
__global__ __launch_bounds__(256) void attn_bwd_prep_u_kernel(AttnShape s, AttnSaved sv, AttnBwdWork wk,
                                                              const float* __restrict__ hinfo,
                                                              const float* __restrict__ d_u) {
  const int nk = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (nk >= s.N * s.K) return;
  const int T = s.T, w = s.w, cnt = sv.cnt[nk];
  const float* g = d_u + (size_t)nk * w;
  const float* h = hinfo + (size_t)nk * T * w;
  const int32_t* idx = sv.idx + (size_t)nk * T;
  const float* amax = sv.amax + (size_t)nk * T;
  const float Mz = sv.Mz[nk];
  double L = 0.0, acc = 0.0;
  for (int i = 0; i < cnt; ++i) {
    const int t = idx[i];
    const double e = (double)expf(tw_logit(amax[t], 1.f) - Mz);
    L += e;
    double row = 0.0;
    for (int c = lane; c < w; c += 64) row += (double)g[c] * (double)h[(size_t)t * w + c];
    acc += e * row;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) {
    wk.coef[nk] = (float)(1.0 / L);
    wk.gu[nk] = (float)(acc / L);
    wk.dss[nk] = 0.f;
  }
}

// ---- db of fvta_attn_bwd_u, summed in fp64 straight from the d ct partials of the main kernel.  db is the sum of every
// row's logit gradient, and with a gradient vector per (n,k) these are N K T terms of order 1 that cancel (exactly so per
// list without tanh): through the fp32 folds (reduce_q's per-n sums, then the bias block of attn_bwd_params_kernel) the partial
// sums reach ~50 at a thousand lists and leave ~2e-5 of rounding where the result is 0.  Fixed order, no atomics:
// grid N, 256 threads -> one double per n; then one workgroup adds those in n order.
__global__ __launch_bounds__(256) void attn_bwd_db_u_kernel(const float* __restrict__ dctp, size_t per_n,
                                                            double* __restrict__ dbn) {
  const float* p = dctp + (size_t)blockIdx.x * per_n;
  double acc = 0.0;
  for (size_t i = threadIdx.x; i < per_n; i += 256) acc += (double)p[i];
  acc = attn_bwd_block_sum_f64(acc);
  if (threadIdx.x == 0) dbn[blockIdx.x] = acc;
}
__global__ __launch_bounds__(256) void attn_bwd_db_u_sum_kernel(const double* __restrict__ dbn, int N, float* __restrict__ db) {
  double acc = 0.0;
  for (int n = threadIdx.x; n < N; n += 256) acc += dbn[n];
  acc = attn_bwd_block_sum_f64(acc);
  if (threadIdx.x == 0) db[0] += (float)acc;
}

struct AttnBwdArgs {
  AttnShape s;
  AttnSaved sv;
  AttnBwdWork wk;
  const float* hinfo;
  const float* d_h_a;  // [N,w]; PERK kernels: d_u [N,K,w]
  float* d_hinfo;
  int accumulate;
  const float* tscale;  // [N,T] or null (time_warp_att): the inner softmax ran on z = amax * tscale
  size_t hstride;       // elements between the row blocks of consecutive (n,k) of hinfo / d_hinfo (see AttnFwdArgs)
  int nt;               // bit 0: non-temporal stores of the d_hinfo rows (written once, read much later); bit 1: the h rows too
  const unsigned long long* table;  // SH kernels: [2][N K T] addresses of the rows' bf16 halves (fvta_lstm_shadow_rows), hinfo is null
};

// TPR threads cover one row (16 B each, G float4 per thread when w > 1024);
// RH = 256/TPR row groups; a tile is TR rows, each thread holds TR/RH of them.
// COS: cosine similarity (simi 4) -- a compile-time flag so that the bilinear shapes do not carry its registers.
// ACC: d_hinfo is accumulated into (accumulate == 1).  Compile-time: as a run-time switch every row's store sat behind a
// (possibly executed) load of its destination, i.e. behind an s_waitcnt vmcnt(0) that also waits for every EARLIER row's
// store -- the write stream of the kernel was one store round trip per row.  Without the load (and with the question
// operand of the current j in registers, below) the rows' stores stream.
// (16-row tiles with four workgroups per CU: 0.96 ms against 0.77 at the metric shape -- the 128-register budget spills)
// SH: the rows are read from the encoders' bf16 shadow (two half-rows per row, addressed through a.table: see
// attn_fwd_shadow.hip) -- 8 bytes per thread and row instead of 16; the chunk's 2 x rows addresses are fetched after the
// row sort and kept in LDS.  G == 1, no cosine.
// PERK: the incoming gradient is per (n,k) (fvta_attn_bwd_u: d_u [N,K,w] in a.d_h_a) -- launched with gk == 1 only, so a
// workgroup's one k is k0 and its gv is loaded once, as before.  Compile-time: the h_a instantiations are unchanged.
template <int TPR, int G, int TR, bool COS, bool ACC, bool SH = false, bool PERK = false>
__global__ __launch_bounds__(256, 2) void attn_bwd_main(AttnBwdArgs a) {
  static_assert(!SH || (G == 1 && !COS && TPR >= 2), "shadow rows: bilinear shapes with one float4 per thread and row");
  static_assert(!PERK || (!COS && !SH), "per-stream gradient: fp32 rows, simiMatrix 1-3");
  constexpr int RH = 256 / TPR;
  constexpr int RPT = TR / RH;
  constexpr int WPR = TPR >= 64 ? TPR / 64 : 1;  // waves that share a row
  __shared__ int s_rows[BWD_CHMAX];
  __shared__ uint8_t s_j[BWD_CHMAX];
  __shared__ int s_hist[4][65];
  __shared__ float s_dot[4][TR];
  __shared__ float s_nrm[4][TR];
  __shared__ float s_self[TR];
  __shared__ float s_pr[TR], s_dx[TR];
  __shared__ int s_tt[TR], s_jj[TR];
  __shared__ unsigned long long s_rp[SH ? 2 : 1][SH ? BWD_CHMAX : 1];
  // the workgroup's group of consecutive k: per-k scalars, and the start of each k's rows in the concatenated list
  __shared__ int s_kbase[17];
  __shared__ float s_kM[16], s_kMz[16], s_kcoef[16], s_kgu[16], s_kdss[16];
  __shared__ uint8_t s_kallm[16];

  const AttnShape& s = a.s;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int cq = tid % TPR, rh = tid / TPR;
  const int grp = blockIdx.y, n = grp / s.ng, k0 = (grp % s.ng) * s.gk, split = blockIdx.x;
  const int nkl = min(s.gk, s.K - k0);  // k's in this group
  const int nk = n * s.K + k0;          // first (n,k) of the group; rows of the group are contiguous from here
  const int T = s.T, w = s.w, JP = s.JP;
  if (tid == 0) {
    int run = 0;
    for (int kl = 0; kl < nkl; ++kl) {
      s_kbase[kl] = run;
      run += a.sv.cnt[nk + kl];
    }
    s_kbase[nkl] = run;
  }
  if (tid < nkl) {
    s_kM[tid] = a.sv.M[nk + tid];
    s_kMz[tid] = a.sv.Mz[nk + tid];
    s_kcoef[tid] = a.wk.coef[nk + tid];
    s_kgu[tid] = a.wk.gu[nk + tid];
    s_kdss[tid] = a.wk.dss[nk + tid];
    s_kallm[tid] = a.sv.allmasked[nk + tid] != 0;
  }
  __syncthreads();
  const int cnt = s_kbase[nkl];
  int chunk = (cnt + s.bsplit - 1) / s.bsplit;
  chunk = (chunk + TR - 1) / TR * TR;
  const int r0 = split * chunk, r1 = min(cnt, r0 + chunk);
  if (r0 >= r1) return;  // slabs were zeroed by the launcher
  const int nrows = r1 - r0;
  const int32_t* __restrict__ idx = a.sv.idx + (size_t)nk * T;
  const float* __restrict__ amax = a.sv.amax + (size_t)nk * T;
  const uint8_t* __restrict__ jmax = a.sv.jmax + (size_t)nk * T;
  // row i of the concatenated list -> flat row (k - k0) * T + t of the group
  auto flat_row = [&](int i) {
    int kl = 0;
    while (kl + 1 < nkl && i >= s_kbase[kl + 1]) ++kl;
    return kl * T + idx[(size_t)kl * T + (i - s_kbase[kl])];
  };

  // ---- stable counting sort of the chunk's rows by jmax (4 waves, contiguous quarters)
  for (int i = tid; i < 4 * 65; i += 256) (&s_hist[0][0])[i] = 0;
  __syncthreads();
  const int q = (nrows + 3) / 4;
  const int b0 = wave * q, b1 = min(nrows, b0 + q);
  for (int base = b0; base < b1; base += 64) {
    const int i = base + lane;
    const bool ok = i < b1;
    const int key = ok ? (int)jmax[flat_row(r0 + i)] : -1;
    unsigned long long todo = __ballot(ok);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int kv = __shfl(key, leader, 64);
      const unsigned long long same = __ballot(ok && key == kv);
      if (lane == leader) s_hist[wave][kv] += __popcll(same);
      todo &= ~same;
    }
  }
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int k = 0; k < 64; ++k)
      for (int wv = 0; wv < 4; ++wv) {
        const int c = s_hist[wv][k];
        s_hist[wv][k] = run;
        run += c;
      }
  }
  __syncthreads();
  for (int base = b0; base < b1; base += 64) {
    const int i = base + lane;
    const bool ok = i < b1;
    const int t = ok ? flat_row(r0 + i) : 0;
    const int key = ok ? (int)jmax[t] : -1;
    unsigned long long todo = __ballot(ok);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int kv = __shfl(key, leader, 64);
      const unsigned long long same = __ballot(ok && key == kv);
      const int basepos = s_hist[wave][kv];
      if (ok && key == kv) {
        const int pos = basepos + __popcll(same & ((1ull << lane) - 1ull));
        s_rows[pos] = t;
        s_j[pos] = (uint8_t)kv;
      }
      __builtin_amdgcn_wave_barrier();
      if (lane == leader) s_hist[wave][kv] = basepos + __popcll(same);
      __builtin_amdgcn_wave_barrier();
      todo &= ~same;
    }
  }
  __syncthreads();

  if constexpr (SH) {  // the sorted rows' addresses (independent loads: inside the sort's serial loop each one was a round trip)
    const unsigned long long* __restrict__ tab0 = a.table + (size_t)nk * T;
    const unsigned long long* __restrict__ tab1 = tab0 + (size_t)s.N * s.K * T;
    for (int i = tid; i < nrows; i += 256) {
      const int t = s_rows[i];
      s_rp[0][i] = tab0[t];
      s_rp[1][i] = tab1[t];
    }
    // (the main loop's first __syncthreads() orders these writes before the tiles' reads)
  }
  const float* __restrict__ hbase = SH ? nullptr : a.hinfo + (size_t)nk * a.hstride;
  // SH: this thread's four channels lie in half `shalf` of a row, `soff` bytes into it
  const int shalf = 4 * cq >= w / 2 ? 1 : 0, soff = 2 * (4 * cq - shalf * (w / 2));
  float* __restrict__ dhbase = a.d_hinfo + (size_t)nk * a.hstride;
  const float* __restrict__ Qs = a.sv.Qs + (size_t)n * s.W4 * JP * 4;
  constexpr bool cosine = COS;
  const size_t slot = ((size_t)grp * s.bsplit + split) * RH + rh;
  float* __restrict__ slab = a.wk.slabs + slot * JP * w;
  float* __restrict__ dctp = a.wk.dctp + slot * JP;
  float* __restrict__ rowp = a.wk.rowp + slot * 2 * w;

  f32x4 gv[G], rh4[G], r24[G], accq[G], accRh[G], accR2[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int c4 = cq + g * TPR;
    gv[g] = ld4(a.d_h_a + (size_t)(PERK ? nk : n) * w + 4 * c4);
    rh4[g] = ld4(a.sv.vecs + VEC_RH * w + 4 * c4);
    r24[g] = ld4(a.sv.vecs + VEC_R2 * w + 4 * c4);
    accq[g] = accRh[g] = accR2[g] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  int cur_j = -1;
  float acc_ct = 0.f;
  f32x4 qs_cur[G];
#pragma unroll
  for (int g = 0; g < G; ++g) qs_cur[g] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto flush = [&]() {
    if (cur_j >= 0) {
#pragma unroll
      for (int g = 0; g < G; ++g) {
        *reinterpret_cast<f32x4*>(slab + (size_t)cur_j * w + 4 * (cq + g * TPR)) = accq[g];
        accq[g] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      if (cq == 0) dctp[cur_j] = acc_ct;
      acc_ct = 0.f;
    }
  };

  typedef unsigned u32x2s __attribute__((ext_vector_type(2)));
  f32x4 hreg[SH ? 1 : RPT][G];
  u32x2s hraw[SH ? RPT : 1];  // SH: the tile stays packed (half the registers), unpacked at each use
  auto row_val = [&](int i, int g) {
    if constexpr (SH) {
      u32x2s raw = hraw[i];
      asm volatile("" : "+v"(raw));  // (unpacked again at each use: the compiler would keep the fp32 copy live instead)
      return f32x4{__uint_as_float(raw[0] << 16), __uint_as_float(raw[0] & 0xffff0000u), __uint_as_float(raw[1] << 16),
                   __uint_as_float(raw[1] & 0xffff0000u)};
    } else {
      return hreg[i][g];
    }
  };
  for (int tb = 0; tb < nrows; tb += TR) {
    __syncthreads();
    if (tid < TR) {
      const int i = tb + tid;
      s_tt[tid] = i < nrows ? s_rows[i] : -1;
      s_jj[tid] = i < nrows ? (int)s_j[i] : 0;
    }
    __syncthreads();
    float dot[RPT], nrm[RPT];
    if constexpr (SH) {
      // every row of the tile is requested before the first one is used (row_val's empty asm pins each use: in one loop
      // with the loads the compiler waited vmcnt(0) row by row -- 32 dependent round trips per tile)
#pragma unroll
      for (int i = 0; i < RPT; ++i) {
        // (a GLOBAL pointer: through a generic one the load is a FLAT instruction, which counts on lgkmcnt too)
        typedef const u32x2s __attribute__((address_space(1)))* grow8_ptr;
        hraw[i] = *(grow8_ptr)(s_rp[shalf][min(tb + rh * RPT + i, nrows - 1)] + soff);  // (padding rows of a tile: the last row's address)
      }
    }
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int t = s_tt[rh * RPT + i];
      float dsum = 0.f, nsum = 0.f;
#pragma unroll
      for (int g = 0; g < G; ++g) {
        if constexpr (SH) {
          hraw[i] = t >= 0 ? hraw[i] : u32x2s{0u, 0u};
        } else {
          const f32x4* hp = reinterpret_cast<const f32x4*>(hbase + (size_t)max(t, 0) * w + 4 * (cq + g * TPR));
          const f32x4 hv = (a.nt & 2) ? __builtin_nontemporal_load(hp) : *hp;  // unconditional, then zeroed
          hreg[i][g] = t >= 0 ? hv : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const f32x4 hcur = row_val(i, g);
        const f32x4 pdt = hcur * gv[g];
        dsum += (pdt[0] + pdt[1]) + (pdt[2] + pdt[3]);
        if (cosine) {
          const f32x4 hh = hcur * hcur;
          nsum += (hh[0] + hh[1]) + (hh[2] + hh[3]);
        }
      }
      dot[i] = dsum;
      nrm[i] = nsum;
    }
    // reduce g.h over the TPR threads of each row
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      float v = dot[i];
#pragma unroll
      for (int o = 1; o < (TPR < 64 ? TPR : 64); o <<= 1) v += __shfl_xor(v, o, 64);
      dot[i] = v;
      if (cosine) {
        float u = nrm[i];
#pragma unroll
        for (int o = 1; o < (TPR < 64 ? TPR : 64); o <<= 1) u += __shfl_xor(u, o, 64);
        nrm[i] = u;
      }
    }
    if (TPR >= 64) {
      if (lane == 0)
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
          s_dot[wave][rh * RPT + i] = dot[i];
          if (cosine) s_nrm[wave][rh * RPT + i] = nrm[i];
        }
    } else {
      if (cq == 0)
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
          s_dot[0][rh * RPT + i] = dot[i];
          if (cosine) s_nrm[0][rh * RPT + i] = nrm[i];
        }
    }
    __syncthreads();
    if (tid < TR) {
      const int t = s_tt[tid];
      float pr = 0.f, dx = 0.f, self = 0.f;
      if (t >= 0) {
        float gh, hh = 0.f;
        if (TPR >= 64) {
          // row `tid` belongs to row group tid / RPT whose waves are [rg*WPR, rg*WPR + WPR)
          const int rgp = tid / RPT;
          gh = 0.f;
#pragma unroll
          for (int v = 0; v < WPR; ++v) {
            gh += s_dot[rgp * WPR + v][tid];
            if (cosine) hh += s_nrm[rgp * WPR + v][tid];
          }
        } else {
          gh = s_dot[0][tid];
          if (cosine) hh = s_nrm[0][tid];
        }
        const int kl = t / T;
        const float M = s_kM[kl];
        const float am = amax[t];
        // z = am * tscale[n,t] under time_warp_att (model_v2.py:269-275); p = softmax_t(z), d z = p (g.h - g.u)
        const float sc = a.tscale ? a.tscale[(size_t)n * T + (t - kl * T)] : 1.f;
        pr = expf(tw_logit(am, sc) - s_kMz[kl]) * s_kcoef[kl];
        const float dz = pr * (gh - s_kgu[kl]);
        if (a.tscale) a.wk.dscr[(size_t)nk * T + t] = dz * am;  // d tscale[n,t] += d z * amax (also for -1e30 rows, as TF)
        if (!s_kallm[kl]) {  // fully masked rows: am = -1e30, no gradient into the masked logits
          const float damax = dz * sc + (am == M ? s_kdss[kl] : 0.f);
          dx = s.add_tanh ? damax * (1.f - am * am) : damax;
          if (cosine) {  // x = (h.qn) * rh with rh = rsqrt(max(|h|^2, eps)) (model_v2.py:250-254): am IS x
            const float rhn = rsqrtf(fmaxf(hh, 1e-12f));
            self = hh > 1e-12f ? -damax * am * rhn * rhn : 0.f;  // d/dh of the normaliser
            dx = damax * rhn;                                      // coefficient of qn[j] (and of h in dQs)
          }
        }
      }
      s_pr[tid] = pr;
      s_dx[tid] = dx;
      if (cosine) s_self[tid] = self;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int row = rh * RPT + i;
      const int t = s_tt[row];
      if (t < 0) continue;
      const int j = s_jj[row];
      const float pr = s_pr[row], dx = s_dx[row], self = cosine ? s_self[row] : 0.f;
      if (j != cur_j) {  // (rows come sorted by j: at most JQ changes per chunk)
        flush();
        cur_j = j;
        // The question operand of the current j stays in registers.  As a per-row load it was a gather of 64 cache lines per
        // wave-instruction (consecutive threads lie JP * 16 bytes apart): 107 M line requests per launch against 28 M for
        // the rows themselves, and the CU's address unit takes ~0.26 lines per clock -- that gather WAS the kernel's time.
        // (The empty asm makes the load's wait happen HERE, inside the branch: left pending across the merge point the
        // compiler must wait vmcnt(0) at every row's first use, which drains the row stores one by one.)
#pragma unroll
        for (int g = 0; g < G; ++g) {
          qs_cur[g] = ld4(Qs + ((size_t)(cq + g * TPR) * JP + j) * 4);
          asm volatile("" : "+v"(qs_cur[g]));
        }
      }
      acc_ct += dx;
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const int c4 = cq + g * TPR;
        const f32x4 h = row_val(i, g);
#ifdef FVTA_ATTN_BWD_QS_PER_ROW  // (A/B: the per-row gather this replaced)
        const f32x4 qs = ld4(Qs + ((size_t)c4 * JP + j) * 4);
#else
        const f32x4 qs = qs_cur[g];
#endif
        f32x4 dh = cosine ? gv[g] * pr + qs * dx + h * self : gv[g] * pr + (qs + rh4[g] + r24[g] * h * 2.f) * dx;
        float* dst = dhbase + (size_t)t * w + 4 * c4;
        if constexpr (ACC) dh += ld4(dst);
        if ((a.nt & 1) && !ACC)
          __builtin_nontemporal_store(dh, reinterpret_cast<f32x4*>(dst));
        else
          *reinterpret_cast<f32x4*>(dst) = dh;
        accq[g] += h * dx;
        if (!cosine) {
          accRh[g] += h * dx;
          accR2[g] += h * h * dx;
        }
      }
    }
  }
  flush();
#pragma unroll
  for (int g = 0; g < G; ++g) {
    *reinterpret_cast<f32x4*>(rowp + 4 * (cq + g * TPR)) = accRh[g];
    *reinterpret_cast<f32x4*>(rowp + w + 4 * (cq + g * TPR)) = accR2[g];
  }
}

// ---- fold slabs per n: d_hq and per-n parameter partials (attn_bwd_shared.h: attn_bwd_fold_body).  grid (N, ceil(w/256),
// ceil(JQ/8)); the slots of a position are summed in slot order, eight loads in flight.  Block jz == 0 also folds the
// d Rh / d R2 partials; a block's row of pvec holds all five vectors.
__global__ __launch_bounds__(256) void attn_bwd_reduce_q_kernel(AttnShape s, AttnSaved sv, AttnBwdWork wk, int RH,
                                                                const float* __restrict__ hq,
                                                                float* __restrict__ d_hq, int accumulate) {
  const int n = blockIdx.x, jz = blockIdx.z, c = blockIdx.y * 256 + 4 * (threadIdx.x & 63);
  const int w = s.w, JP = s.JP, JQ = s.JQ;
  const int nslot = s.ng * s.bsplit * RH;
  const size_t slot0 = (size_t)n * nslot;
  const bool live = c < w;
  auto fold = [&](const float* base, size_t stride) {
    return attn_bwd_slot_sum<f32x4>(nslot, [&](int sl) { return ld4_if(live, base + (size_t)sl * stride); });
  };
  f32x4 pU, pCq, pC2;
  if (!attn_bwd_fold_body(sv.vecs, hq + (size_t)n * JQ * w, d_hq + (size_t)n * JQ * w, accumulate != 0, wk.dctp + slot0 * JP,
                          (size_t)JP, nslot, wk.dctn + (size_t)n * JP, w, JP, JQ,
                          [&](int j) { return fold(wk.slabs + (slot0 * JP + j) * w + c, (size_t)JP * w); }, pU, pCq, pC2))
    return;
  f32x4 pRh = zero4(), pR2 = zero4();
  if (jz == 0) {
    pRh = fold(wk.rowp + slot0 * 2 * w + c, (size_t)2 * w);
    pR2 = fold(wk.rowp + slot0 * 2 * w + w + c, (size_t)2 * w);
  }
  float* pv = wk.pvec + ((size_t)n * gridDim.z + jz) * VEC_COUNT * w;
  *reinterpret_cast<f32x4*>(pv + VEC_U * w + c) = pU;
  *reinterpret_cast<f32x4*>(pv + VEC_RH * w + c) = pRh;
  *reinterpret_cast<f32x4*>(pv + VEC_R2 * w + c) = pR2;
  *reinterpret_cast<f32x4*>(pv + VEC_CQ * w + c) = pCq;
  *reinterpret_cast<f32x4*>(pv + VEC_C2 * w + c) = pC2;
}

// ---- cosine similarity (simi 4): d_hq from the dqn slabs; qn = q * rq, rq = rsqrt(max(|q|^2, eps)).
// grid N*JQ, 256 threads
__global__ __launch_bounds__(256) void attn_bwd_cosine_q_kernel(AttnShape s, AttnBwdWork wk, int RH,
                                                                const float* __restrict__ hq,
                                                                float* __restrict__ d_hq, int accumulate) {
  __shared__ float s_red[2][4];
  const int n = blockIdx.x / s.JQ, j = blockIdx.x % s.JQ, tid = threadIdx.x;
  const int w = s.w, JP = s.JP;
  const int nslot = s.ng * s.bsplit * RH;
  const size_t slot0 = (size_t)n * nslot;
  const float* q = hq + ((size_t)n * s.JQ + j) * w;
  float qq = 0.f, qd = 0.f;
  for (int c = tid; c < w; c += 256) {
    float dQ = 0.f;
    for (int sl = 0; sl < nslot; ++sl) dQ += wk.slabs[((slot0 + sl) * JP + j) * w + c];
    const float qv = q[c];
    qq += qv * qv;
    qd += qv * dQ;
  }
  qq = wave_sum(qq);
  qd = wave_sum(qd);
  if ((tid & 63) == 0) {
    s_red[0][tid >> 6] = qq;
    s_red[1][tid >> 6] = qd;
  }
  __syncthreads();
  qq = (s_red[0][0] + s_red[0][1]) + (s_red[0][2] + s_red[0][3]);
  qd = (s_red[1][0] + s_red[1][1]) + (s_red[1][2] + s_red[1][3]);
  const float rq = rsqrtf(fmaxf(qq, 1e-12f));
  const float proj = qq > 1e-12f ? qd * rq * rq : 0.f;  // (qn . dqn) rq, folded
  for (int c = tid; c < w; c += 256) {
    float dQ = 0.f;
    for (int sl = 0; sl < nslot; ++sl) dQ += wk.slabs[((slot0 + sl) * JP + j) * w + c];
    const float dq = (dQ - proj * q[c]) * rq;
    float* dst = d_hq + ((size_t)n * s.JQ + j) * w + c;
    *dst = accumulate != 0 ? *dst + dq : dq;
  }
}

// ---- sum over n, map back to att_logits/W's layout (attn_bwd_shared.h: the parameter kernels' pieces).  grid ceil(w/64) + 1;
// rows of pvec = (n, group of question positions).  db null: left to the caller (fvta_attn_bwd_u)
__global__ __launch_bounds__(256) void attn_bwd_params_kernel(AttnShape s, AttnBwdWork wk, float* __restrict__ dW,
                                                              float* __restrict__ db) {
  if (blockIdx.x == gridDim.x - 1) {
    attn_bwd_bias_block(wk.dctn, (size_t)s.N * s.JP, db);
    return;
  }
  const int part = threadIdx.x >> 6, c = blockIdx.x * 64 + (threadIdx.x & 63);
  float v[VEC_COUNT] = {0, 0, 0, 0, 0};
  if (c < s.w)
#pragma unroll
    for (int k = 0; k < VEC_COUNT; ++k) v[k] = attn_bwd_sum_rows(wk.pvec, (size_t)s.N * attn_bwd_jz(s), VEC_COUNT, k, part, s.w, c);
  attn_bwd_combine_dW(v, s.simi, s.feat_order, s.w, c, dW);
}

// ---- time_warp_att: the masked rows that carry softmax weight (see attn_pad_terms_kernel in attn_fwd.hip): their
// direct term p r g into d_hinfo and their share of d tscale (d z * -1e30, as TF computes it).  No gradient into the
// masked logits themselves (deviation (b)).  grid N*K, 256 threads.
__global__ __launch_bounds__(256) void attn_bwd_pad_kernel(AttnBwdArgs a, const uint8_t* __restrict__ hmask) {
  __shared__ float s_red[4];
  __shared__ int s_list[256];
  __shared__ int s_n;
  const AttnShape& s = a.s;
  const int nk = blockIdx.x, n = nk / s.K, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int T = s.T, w = s.w;
  if (a.sv.allmasked[nk]) return;
  const uint8_t* hm = hmask + (size_t)nk * T;
  const float* sc = a.tscale + (size_t)n * T;
  const float Mz = a.sv.Mz[nk], L = a.sv.L[nk], coef = a.wk.coef[nk];
  const float* g = a.d_h_a + (size_t)n * w;
  // Two passes over the masked rows that carry weight.  Pass 0 sums their weights and weighted g.h; when they hold
  // ALL of the softmax's weight (the usual case: exp() of every valid row's logit underflows against +1e30) the mean
  // g.u the softmax gradient subtracts is taken from these very sums, so that a single winner gets d z = 0 EXACTLY, as
  // TF's p (g - sum p g) does -- it is multiplied by -1e30 on its way into d tscale.
  float wsum = 0.f, gsum = 0.f, gbar = a.wk.gu[nk];
  for (int pass = 0; pass < 2; ++pass) {
    for (int t0 = 0; t0 < T; t0 += 256) {
      __syncthreads();
      if (tid == 0) s_n = 0;
      __syncthreads();
      const int t = t0 + tid;
      const bool on = t < T && !hm[t] && tw_logit(FVTA_NEG, sc[t]) >= Mz - 104.f;
      // ascending t within the chunk (ballot ranks), chunks in order: the sums below run in a fixed order
      const unsigned long long bal = __ballot(on);
      if (lane == 0) s_red[wave] = (float)__popcll(bal);
      __syncthreads();
      int base = 0;
      for (int v = 0; v < wave; ++v) base += (int)s_red[v];
      if (on) s_list[base + __popcll(bal & ((1ull << lane) - 1ull))] = t;
      if (tid == 0) s_n = (int)(s_red[0] + s_red[1] + s_red[2] + s_red[3]);
      __syncthreads();
      const int cnt = s_n;
      for (int i = 0; i < cnt; ++i) {
        const int tt = s_list[i];
        const float wt = expf(tw_logit(FVTA_NEG, sc[tt]) - Mz);
        const float pr = wt * coef;
        const float* row = a.hinfo + ((size_t)nk * T + tt) * w;
        float* drow = a.d_hinfo + ((size_t)nk * T + tt) * w;
        float dot = 0.f;
        for (int c = 4 * tid; c < w; c += 1024) {
          const f32x4 hv = ld4(row + c), gv = ld4(g + c);
          const f32x4 pdt = hv * gv;
          dot += (pdt[0] + pdt[1]) + (pdt[2] + pdt[3]);
          if (pass == 1) {
            f32x4 dh = gv * pr;
            if (a.accumulate != 2) dh += ld4(drow + c);  // modes 0/3 zeroed the row first, mode 1 accumulates; 2: plain store
            *reinterpret_cast<f32x4*>(drow + c) = dh;
          }
        }
        dot = wave_sum(dot);
        __syncthreads();
        if (lane == 0) s_red[wave] = dot;
        __syncthreads();
        dot = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
        if (pass == 0) {
          wsum += wt;
          gsum += wt * dot;
        } else if (tid == 0) {
          a.wk.dscr[(size_t)nk * T + tt] = pr * (dot - gbar) * FVTA_NEG;
        }
      }
    }
    if (pass == 0 && wsum == L) gbar = gsum / L;  // the masked rows hold all the weight
  }
}

// accumulate 0 / 3: the rows the main kernel does not write -- the MASKED rows -- are zeros.  (A memset of the whole gradient
// tensor before a kernel that overwrites every valid row of it was 1.9 GB of stores per step at the metric shape, 0.3 ms.)
// A wave per row, grid ceil(N K T / 4)
__global__ __launch_bounds__(256) void attn_zero_masked_rows_kernel(AttnShape s, const uint8_t* __restrict__ hmask,
                                                                    float* __restrict__ d_hinfo) {
  const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (size_t)s.N * s.K * s.T || hmask[row]) return;
  f32x4* dst = reinterpret_cast<f32x4*>(d_hinfo + row * s.w);
  for (int c = threadIdx.x & 63; c < s.w / 4; c += 64) dst[c] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// d_tscale[n,t] += sum_k dscr[n,k,t], fixed order
__global__ void attn_bwd_dscale_kernel(AttnShape s, const float* __restrict__ dscr, float* __restrict__ d_tscale) {
  const int pos = blockIdx.x * blockDim.x + threadIdx.x;
  if (pos >= s.N * s.T) return;
  const int n = pos / s.T, t = pos % s.T;
  float acc = 0.f;
  for (int k = 0; k < s.K; ++k) acc += dscr[((size_t)n * s.K + k) * s.T + t];
  d_tscale[pos] += acc;
}

}  // namespace fvta

using namespace fvta;

size_t fvta_attn_bwd_workspace_bytes(const AttnShape& s) { return bwd_work_view(s, nullptr).bytes; }

extern "C" int fvta_attn_bwd(const fvta_attn_desc* d, const float* hinfo, const float* hq, const uint8_t* hmask,
                             const uint8_t* qmask, const float* W, const float* b, const float* d_h_a,
                             const void* saved, float* d_hinfo, float* d_hq, float* dW, float* db, int accumulate,
                             void* workspace, fvta_stream_t stream_) {
  return fvta_attn_bwd_tw(d, hinfo, hq, hmask, qmask, W, b, nullptr, d_h_a, saved, d_hinfo, d_hq, dW, db, nullptr,
                          accumulate, workspace, stream_);
}

static int attn_bwd_impl(const fvta_attn_desc* d, const float* hinfo, const uint64_t* table, const float* hq, const uint8_t* hmask,
                         const uint8_t* qmask, const float* W, const float* b, const float* tscale,
                         const float* d_h_a, const void* saved, float* d_hinfo, float* d_hq, float* dW, float* db,
                         float* d_tscale, int accumulate, void* workspace, fvta_stream_t stream_);

static int attn_bwd_nt_mode() {
  static const int nt = [] {
    const char* e = getenv("FVTA_ATTN_BWD_NT");
    return e ? atoi(e) : FVTA_ATTN_BWD_NT_DEFAULT;
  }();
  return nt;
}

// ---- what the two entries (attn_bwd_impl: one gradient vector per n; fvta_attn_bwd_u: one per (n,k)) share on the host
static AttnBwdArgs attn_bwd_args(const AttnShape& s, const AttnSaved& sv, const AttnBwdWork& wk, const float* hinfo,
                                 const uint64_t* table, const float* g, float* d_hinfo, int accumulate, const float* tscale,
                                 size_t hstride) {
  return AttnBwdArgs{s, sv, wk, hinfo, g, d_hinfo, accumulate, tscale, hstride ? hstride : (size_t)s.T * s.w, attn_bwd_nt_mode(),
                     reinterpret_cast<const unsigned long long*>(table)};
}

// the main kernel of one shape: ACC (d_hinfo accumulated into) is accumulate == 1
template <int TPR, int G, int TR, bool COS, bool SH = false, bool PERK = false>
static void attn_bwd_launch(const AttnBwdArgs& a, hipStream_t stream) {
  const dim3 grid(a.s.bsplit, a.s.N * a.s.ng);
  if (a.accumulate == 1) hipLaunchKernelGGL((attn_bwd_main<TPR, G, TR, COS, true, SH, PERK>), grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL((attn_bwd_main<TPR, G, TR, COS, false, SH, PERK>), grid, dim3(256), 0, stream, a);
}

// before the main kernel: the slabs are zeros (a workgroup without rows writes none), and with `zero_rows` (accumulate 0 / 3)
// so are the rows of d_hinfo the main kernel does not write -- the MASKED rows; without masks every row is valid and written
static int attn_bwd_prologue(const fvta_attn_desc* d, const AttnShape& s, const AttnBwdWork& wk, const uint8_t* hmask,
                             float* d_hinfo, bool zero_rows, hipStream_t stream) {
  FVTA_CHECK_HIP(hipMemsetAsync(wk.slabs, 0, wk.slab_bytes, stream));
  if (zero_rows && d->hinfo_stride)
    FVTA_CHECK_HIP(hipMemset2DAsync(d_hinfo, (size_t)d->hinfo_stride * sizeof(float), 0, (size_t)s.T * s.w * sizeof(float),
                                    (size_t)s.N, stream));
  else if (zero_rows && s.use_mask)  // every valid row is written by the main kernel (a fully masked stream: all of its rows)
    hipLaunchKernelGGL(attn_zero_masked_rows_kernel, dim3((unsigned)(((size_t)s.N * s.K * s.T + 3) / 4)), dim3(256), 0, stream, s,
                       hmask, d_hinfo);
  return FVTA_OK;
}

extern "C" int fvta_attn_bwd_tw(const fvta_attn_desc* d, const float* hinfo, const float* hq, const uint8_t* hmask,
                                const uint8_t* qmask, const float* W, const float* b, const float* tscale,
                                const float* d_h_a, const void* saved, float* d_hinfo, float* d_hq, float* dW, float* db,
                                float* d_tscale, int accumulate, void* workspace, fvta_stream_t stream_) {
  FVTA_CHECK_ARG(hinfo != nullptr, "attn_bwd: null pointer");
  return attn_bwd_impl(d, hinfo, nullptr, hq, hmask, qmask, W, b, tscale, d_h_a, saved, d_hinfo, d_hq, dW, db, d_tscale,
                       accumulate, workspace, stream_);
}

// The backward of fvta_attn_fwd_shadow: the rows come from the same table of bf16 half-row addresses; d_hinfo is the
// fp32 [N,K,T,w] tensor as in fvta_attn_bwd.
extern "C" int fvta_attn_bwd_shadow(const fvta_attn_desc* d, const uint64_t* table, const float* hq, const uint8_t* hmask,
                                    const uint8_t* qmask, const float* W, const float* b, const float* d_h_a,
                                    const void* saved, float* d_hinfo, float* d_hq, float* dW, float* db, int accumulate,
                                    void* workspace, fvta_stream_t stream_) {
  FVTA_CHECK_ARG(table != nullptr, "attn_bwd_shadow: null pointer");
  FVTA_CHECK_ARG(d && d->JQ <= 32 && (d->w == 512 || d->w == 1024) && d->simi != 4 && !d->hinfo_stride,
                 "attn_bwd_shadow: needs JQ <= 32, w = 512 or 1024, simiMatrix 1-3, no hinfo_stride");
  return attn_bwd_impl(d, nullptr, table, hq, hmask, qmask, W, b, nullptr, d_h_a, saved, d_hinfo, d_hq, dW, db, nullptr,
                       accumulate, workspace, stream_);
}

static int attn_bwd_impl(const fvta_attn_desc* d, const float* hinfo, const uint64_t* table, const float* hq, const uint8_t* hmask,
                         const uint8_t* qmask, const float* W, const float* b, const float* tscale,
                         const float* d_h_a, const void* saved, float* d_hinfo, float* d_hq, float* dW, float* db,
                         float* d_tscale, int accumulate, void* workspace, fvta_stream_t stream_) {
  if (int e = fvta_attn_check_desc(d)) return e;
  FVTA_CHECK_ARG((tscale == nullptr) == (d_tscale == nullptr), "attn_bwd: tscale and d_tscale go together");
  FVTA_CHECK_ARG((hinfo || table) && hq && d_h_a && saved && d_hinfo && d_hq && workspace, "attn_bwd: null pointer");
  FVTA_CHECK_ARG(d->simi == 4 || (dW && db), "attn_bwd: dW/db required");
  FVTA_CHECK_ARG(!(tscale && d->hinfo_stride), "attn_bwd: tscale with a strided hinfo is not supported");
  hipStream_t stream = (hipStream_t)stream_;
  const bool use_mask = hmask && qmask;
  const AttnShape s = attn_shape(d, use_mask);
  AttnSaved sv = attn_saved_view(s, const_cast<void*>(saved));
  AttnBwdWork wk = bwd_work_view(s, workspace);
  const int RH = bwd_rh(s.W4);
  if (tscale) FVTA_CHECK_HIP(hipMemsetAsync(wk.dscr, 0, (size_t)s.N * s.K * s.T * sizeof(float), stream));
  if (int e = attn_bwd_prologue(d, s, wk, hmask, d_hinfo, accumulate == 0 || accumulate == 3, stream)) return e;
  hipLaunchKernelGGL(attn_bwd_prep_kernel, dim3(s.N), dim3(s.K > 4 ? 1024 : 256), 0, stream, s, sv, wk, d_h_a);
  const AttnBwdArgs a = attn_bwd_args(s, sv, wk, hinfo, table, d_h_a, d_hinfo, accumulate, tscale, (size_t)d->hinfo_stride);
  const bool prof_it = (size_t)s.N * s.K * s.T >= 65536;  // the context attention, see attn_fwd.hip
  if (prof_it) fvta_prof_begin(FVTA_PROF_ATTN_BWD_MAIN, stream);
  if (table) {  // shadow rows
    if (s.w == 512) attn_bwd_launch<128, 1, 32, false, true>(a, stream);
    else attn_bwd_launch<256, 1, 32, false, true>(a, stream);
  } else if (s.simi == 4) {
    switch (s.w) {
      case 64: attn_bwd_launch<16, 1, 32, true>(a, stream); break;
      case 128: attn_bwd_launch<32, 1, 32, true>(a, stream); break;
      case 256: attn_bwd_launch<64, 1, 32, true>(a, stream); break;
      case 512: attn_bwd_launch<128, 1, 32, true>(a, stream); break;
      case 1024: attn_bwd_launch<256, 1, 16, true>(a, stream); break;  // (the cosine variant of the 32-row tile would spill)
      case 2048: attn_bwd_launch<256, 2, 16, true>(a, stream); break;
    }
  } else {
    switch (s.w) {
      case 64: attn_bwd_launch<16, 1, 32, false>(a, stream); break;
      case 128: attn_bwd_launch<32, 1, 32, false>(a, stream); break;
      case 256: attn_bwd_launch<64, 1, 32, false>(a, stream); break;
      case 512: attn_bwd_launch<128, 1, 32, false>(a, stream); break;
      case 1024: attn_bwd_launch<256, 1, 32, false>(a, stream); break;
      case 2048: attn_bwd_launch<256, 2, 16, false>(a, stream); break;
    }
  }
  if (prof_it) fvta_prof_end(FVTA_PROF_ATTN_BWD_MAIN, 1, stream);
  FVTA_CHECK_LAUNCH("attn_bwd_main");
  if (tscale) {
    if (use_mask) hipLaunchKernelGGL(attn_bwd_pad_kernel, dim3(s.N * s.K), dim3(256), 0, stream, a, hmask);
    hipLaunchKernelGGL(attn_bwd_dscale_kernel, dim3((s.N * s.T + 255) / 256), dim3(256), 0, stream, s, wk.dscr, d_tscale);
    FVTA_CHECK_LAUNCH("attn_bwd_tw");
  }
  if (s.simi == 4) {
    hipLaunchKernelGGL(attn_bwd_cosine_q_kernel, dim3(s.N * s.JQ), dim3(256), 0, stream, s, wk, RH, hq, d_hq, accumulate);
  } else {
    hipLaunchKernelGGL(attn_bwd_reduce_q_kernel, dim3(s.N, (s.w + 255) / 256, attn_bwd_jz(s)), dim3(256), 0, stream, s, sv, wk, RH, hq,
                       d_hq, accumulate);
    hipLaunchKernelGGL(attn_bwd_params_kernel, dim3((s.w + 63) / 64 + 1), dim3(256), 0, stream, s, wk, dW, db);
  }
  FVTA_CHECK_LAUNCH("attn_bwd_reduce");
  return FVTA_OK;
}

// ---- fvta_attn_bwd_u: the backward of "fvta_attn_fwd, then fvta_attn_read_u" -- every (n,k) an attention of its own, its
// gradient d_u[n,k] in place of d_h_a[n].  `saved` does not depend on how the backward groups its work, so this entry runs
// on a shape of its own with one k per workgroup (gk = 1, ng = K: a grouped workgroup loads ONE gradient vector) and
// bsplit as attn_shape() chose it; the slabs of its workspace are laid out for that shape.
static AttnShape attn_shape_u(const fvta_attn_desc* d, bool use_mask) {
  AttnShape s = attn_shape(d, use_mask);
  s.gk = 1;
  s.ng = s.K;
  return s;
}

static int attn_bwd_u_check(const fvta_attn_desc* d) {
  if (int e = fvta_attn_check_desc(d)) return e;
  FVTA_CHECK_ARG(d->simi != 4, "attn_bwd_u: simiMatrix 4 is not supported (simiMatrix 1-3)");
  FVTA_CHECK_ARG(d->hinfo_stride == 0, "attn_bwd_u: hinfo_stride=%lld is not supported (dense hinfo only)", (long long)d->hinfo_stride);
  FVTA_CHECK_ARG((long long)d->N * d->K <= 65535, "attn_bwd_u: N*K=%lld exceeds 65535 workgroup rows", (long long)d->N * d->K);
  return FVTA_OK;
}

// the backward's workspace for that shape, then one double per n (attn_bwd_db_u_kernel)
static size_t attn_bwd_u_dbn_offset(const AttnBwdWork& wk) { return fvta_align_up(wk.bytes, 256); }

extern "C" size_t fvta_attn_bwd_u_workspace_bytes(const fvta_attn_desc* d) {
  if (attn_bwd_u_check(d)) return 0;
  return attn_bwd_u_dbn_offset(bwd_work_view(attn_shape_u(d, true), nullptr)) + (size_t)d->N * sizeof(double);
}

extern "C" int fvta_attn_bwd_u(const fvta_attn_desc* d, const float* hinfo, const float* hq, const uint8_t* hmask,
                               const uint8_t* qmask, const float* W, const float* b, const float* d_u, const void* saved,
                               float* d_hinfo, float* d_hq, float* dW, float* db, int accumulate, void* workspace,
                               fvta_stream_t stream_) {
  if (int e = attn_bwd_u_check(d)) return e;
  FVTA_CHECK_ARG(accumulate == 0 || accumulate == 1, "attn_bwd_u: accumulate=%d (0: overwrite, 1: add)", accumulate);
  FVTA_CHECK_ARG(hinfo && hq && d_u && saved && d_hinfo && d_hq && dW && db && workspace, "attn_bwd_u: null pointer");
  hipStream_t stream = (hipStream_t)stream_;
  const bool use_mask = hmask && qmask;
  const AttnShape s = attn_shape_u(d, use_mask);
  AttnSaved sv = attn_saved_view(s, const_cast<void*>(saved));
  AttnBwdWork wk = bwd_work_view(s, workspace);
  const int RH = bwd_rh(s.W4);
  if (int e = attn_bwd_prologue(d, s, wk, hmask, d_hinfo, accumulate == 0, stream)) return e;
  hipLaunchKernelGGL(attn_bwd_prep_u_kernel, dim3((s.N * s.K + 3) / 4), dim3(256), 0, stream, s, sv, wk, hinfo, d_u);
  const AttnBwdArgs a = attn_bwd_args(s, sv, wk, hinfo, nullptr, d_u, d_hinfo, accumulate, nullptr, 0);
  switch (s.w) {
    case 64: attn_bwd_launch<16, 1, 32, false, false, true>(a, stream); break;
    case 128: attn_bwd_launch<32, 1, 32, false, false, true>(a, stream); break;
    case 256: attn_bwd_launch<64, 1, 32, false, false, true>(a, stream); break;
    case 512: attn_bwd_launch<128, 1, 32, false, false, true>(a, stream); break;
    case 1024: attn_bwd_launch<256, 1, 32, false, false, true>(a, stream); break;
    case 2048: attn_bwd_launch<256, 2, 8, false, false, true>(a, stream); break;  // (16-row tiles: 24 bytes of scratch per lane, as the h_a path has)
  }
  FVTA_CHECK_LAUNCH("attn_bwd_main (per-stream gradient)");
  hipLaunchKernelGGL(attn_bwd_reduce_q_kernel, dim3(s.N, (s.w + 255) / 256, attn_bwd_jz(s)), dim3(256), 0, stream, s, sv, wk, RH, hq,
                     d_hq, accumulate);
  hipLaunchKernelGGL(attn_bwd_params_kernel, dim3((s.w + 63) / 64 + 1), dim3(256), 0, stream, s, wk, dW, (float*)nullptr);  // (db: below)
  double* dbn = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + attn_bwd_u_dbn_offset(wk));
  hipLaunchKernelGGL(attn_bwd_db_u_kernel, dim3(s.N), dim3(256), 0, stream, wk.dctp, (size_t)s.ng * s.bsplit * RH * s.JP, dbn);
  hipLaunchKernelGGL(attn_bwd_db_u_sum_kernel, dim3(1), dim3(256), 0, stream, dbn, s.N, db);
  FVTA_CHECK_LAUNCH("attn_bwd_u reduce");
  return FVTA_OK;
}

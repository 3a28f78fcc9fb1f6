// Shared by the focal-attention forward kernels (attn_fwd.hip, attn_fwd_shadow.hip, attn_fwd_wide.hip): the launch
// arguments, the fp16 split of a row value (hi = rtz_f16(x), lo = f16((x - hi) * 2^11)), the LDS-only barrier, the fused
// DPP row sum, and the one copy of what the 16- and 32-row kernels have in common: workgroup numbering, the dealing of an
// album's tiles, the pair hand-shake, question staging, row term, score finishing, the online-softmax step, partial heads.
// Every helper is inlined into the kernel's own, spelled-out tile loop (the kernels sit at the edge of their register
// budget: see _isa_guard.py).
#pragma once
#include <type_traits>
#include "attn_common.h"

namespace fvta {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4v __attribute__((ext_vector_type(4)));
// x[0..7] = (a0, a1) -> hi, lo fp16 pieces (see above); register pairs are concatenated, never re-packed
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split_f16x2(float x0, float x1, half2v& hi, half2v& lo) {
  hi = __builtin_bit_cast(half2v, __builtin_amdgcn_cvt_pkrtz(x0, x1));
  // lo = fp16((x - hi) * 2048) as ONE mixed-precision FMA per element, 2048 x - 2048 hi with the fp16 hi read in place
  // (v_fma_mixlo/mixhi_f16 write one half of the destination and keep the other): 4 instructions per pair instead of 6
  // (2 back-conversions, packed subtract, packed scale, pack).  Exact up to the final rounding, as before (x - hi is exact).
  const f32x2 xs = f32x2{x0, x1} * 2048.f;
  const float m2048 = -2048.f;
  unsigned hw = __builtin_bit_cast(unsigned, hi), lw;
  asm("v_fma_mixlo_f16 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=&v"(lw) : "v"(hw), "s"(m2048), "v"(xs[0]));
  asm("v_fma_mixhi_f16 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(lw) : "v"(hw), "s"(m2048), "v"(xs[1]));
  lo = __builtin_bit_cast(half2v, lw);
}
__device__ __forceinline__ half8 cat_h2(half2v a, half2v b, half2v c, half2v d) {
  const half4v ab = __builtin_shufflevector(a, b, 0, 1, 2, 3), cd = __builtin_shufflevector(c, d, 0, 1, 2, 3);
  return __builtin_shufflevector(ab, cd, 0, 1, 2, 3, 4, 5, 6, 7);
}
__device__ __forceinline__ void split_f16x8(const f32x4 a0, const f32x4 a1, half8& hi, half8& lo) {
  half2v h[4], l[4];
  split_f16x2(a0[0], a0[1], h[0], l[0]);
  split_f16x2(a0[2], a0[3], h[1], l[1]);
  split_f16x2(a1[0], a1[1], h[2], l[2]);
  split_f16x2(a1[2], a1[3], h[3], l[3]);
  hi = cat_h2(h[0], h[1], h[2], h[3]);
  lo = cat_h2(l[0], l[1], l[2], l[3]);
}


__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Sum of each of four values over the 16 lanes of its DPP row, every lane ending with the result: the butterfly of
// row16_sum as FUSED v_add_f32_dpp (the compiler emits v_mov_b32_dpp + a packed add + s_nop per step: 31 issue slots for
// what are 17 here).  The four values are interleaved, so a step's DPP read of a register comes three instructions after
// the previous step wrote it (the hazard wants two wait states; the assembler does not check inside inline asm, hence
// also the leading s_nop against whatever VALU instruction produced the inputs).
__device__ __forceinline__ void row16_sum4(f32x4& v) {
  float a = v[0], b = v[1], c = v[2], d = v[3];
#define FVTA_DPP4(CTRL)                                                   \
  "v_add_f32_dpp %0, %0, %0 " CTRL " row_mask:0xf bank_mask:0xf\n\t"      \
  "v_add_f32_dpp %1, %1, %1 " CTRL " row_mask:0xf bank_mask:0xf\n\t"      \
  "v_add_f32_dpp %2, %2, %2 " CTRL " row_mask:0xf bank_mask:0xf\n\t"      \
  "v_add_f32_dpp %3, %3, %3 " CTRL " row_mask:0xf bank_mask:0xf\n\t"
  asm("s_nop 1\n\t" FVTA_DPP4("quad_perm:[1,0,3,2]") FVTA_DPP4("quad_perm:[2,3,0,1]") FVTA_DPP4("row_half_mirror")
          FVTA_DPP4("row_mirror")
      : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
#undef FVTA_DPP4
  v = f32x4{a, b, c, d};
}


// ---- launch arguments of the forward main kernels
struct AttnFwdArgs {
  AttnShape s;
  AttnSaved sv;
  const float* hinfo;
  float* a_logits;  // may be null
  float* part;      // [N*K][nsplit][w+4] : m, l, mu, -, u[w]   (m: max of the softmax logits z, mu: max of amax)
  const float* tscale;  // [N,T] or null: z[n,k,t] = amax[n,k,t] * tscale[n,t] (time_warp_att)
  int ipw;          // 16-row kernel: items per workgroup
  int dbg;          // FVTA_ATTN_DBG experiment bits (diagnostics only)
  size_t hstride;   // elements between the row blocks of consecutive (n,k): T*w, or fvta_attn_desc.hinfo_stride (K == 1)
  const uint32_t* wgtab;  // pair kernel: workgroup -> n | g << 16 | G_n << 24 (attn_balance_kernel), null: G workgroups for every n
  int* fault;             // host-mapped status word (attn_fault_word): a kernel that has to trap says why first
};

// Fault codes a forward kernel leaves in AttnFwdArgs::fault before it traps: the trap aborts the queue -- a process that
// survives it (or the next call, whichever comes first) reads the word and reports instead of "unspecified launch failure".
enum { ATTN_FAULT_PAIR_WAIT = 1 };
int* attn_fault_word();   // attn_fwd.hip: the word (device-visible address of host memory), null if it cannot be had

// ---- host side, common to the launchers
// grid of nwg workgroups in XCD-contiguous order (attn_wg_index): whole rounds of the 8 XCDs
inline dim3 attn_xcd_grid(int nwg) { return dim3(((nwg + 7) / 8) * 8); }
// dynamic LDS of a kernel that stages the question as nkt k-steps of hi and lo fragments plus the two row-term vectors
inline size_t attn_question_lds(int nkt, int w) { return (size_t)2 * nkt * 2 * 64 * 16 + (size_t)2 * w * sizeof(float); }
// f(std::integral_constant<int, RMODE>) for the RMODE of simiMatrix `simi` (see row_term)
template <class F>
inline void attn_with_rmode(int simi, F f) {
  if (simi == 1)
    f(std::integral_constant<int, 1>{});
  else if (simi == 3)
    f(std::integral_constant<int, 3>{});
  else
    f(std::integral_constant<int, 2>{});
}

// ---- which workgroup this is.  XCD-contiguous order (see attn_fwd_main): hardware deals consecutive block numbers
// round-robin to the 8 XCDs, so block b becomes workgroup (b & 7) * per + (b >> 3) and the workgroups of one n share an
// L2.  false: a block of the grid's padding, which returns at once.
__device__ __forceinline__ bool attn_wg_index(int nwg, int& wg) {
  const int per = (nwg + 7) / 8;
  wg = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
  return !(wg >= nwg || (int)(blockIdx.x >> 3) >= per);
}
// the n this workgroup serves, its index among that n's workgroups and their number: uniform (G_all each), or dealt in
// proportion to the n's valid tiles (wgtab of attn_balance_kernel, masked batches: albums differ in rows).  false: a
// table entry nobody serves.
__device__ __forceinline__ bool attn_wg_album(const uint32_t* wgtab, int wg, int G_all, int& n, int& g0, int& G) {
  n = wg / G_all, g0 = wg % G_all, G = G_all;
  if (wgtab) {
    const uint32_t e = wgtab[wg];
    if (e == 0xffffffffu) return false;
    n = (int)(e & 0xffffu);
    g0 = (int)((e >> 16) & 0xffu);
    G = (int)(e >> 24);
  }
  return true;
}

// ---- a partial (m, l, mu, -, u[w]) for attn_merge_kernel: its head, and the head of one that summed no rows
// (no time_warp_att in the 16- and 32-row kernels: the softmax logits are amax itself, so mu = m)
__device__ __forceinline__ void store_partial_head(float* part, float m_run, float l_run) {
  part[0] = m_run;
  part[1] = l_run;
  part[2] = m_run;
}
__device__ __forceinline__ void store_empty_partial(float* part) {
  part[0] = -INFINITY;
  part[1] = 0.f;
  part[2] = -INFINITY;
}

// ---- dealing an album's tiles to the DEALERS that share it (attn_fwd_pair16 / pair16h: D = 4 pairs of waves per
// workgroup, tiles of TROWS = 16 rows; attn_fwd_wide: D = 1, the workgroup, 32 rows).  With G workgroups on album n there
// are P = D G dealers; dealer d of workgroup g0 is number pg = D g0 + d.
//   FLAT dealing: the n's tiles, in (k, tile) order, are cut into P equal runs, one per dealer (a run crosses stream
//   boundaries; dealer p's piece of stream k is that stream's partial number p - (first dealer that touches k)).  Only if
//   no stream is cut into more pieces than it has partial slots (nsplit); otherwise the (k, split) items are dealt
//   ROUND-ROBIN as in the other kernels (item g0 + G d, then every P-th; pieces of ceil(tiles / nsplit) tiles: unequal
//   sums per dealer).
// THE RULE THE HOST'S BOUNDS REST ON (wide_covers, attn_balance_kernel's run_cap; the wide kernel lists a run in LDS): a
// stream of c rows has ceil(c / TROWS) tiles, so an album has tot <= (its rows) / TROWS + K tiles (one ragged tile per
// stream).  A flat run is [tot pg / P, tot (pg + 1) / P): at most ceil(tot / P) tiles.  A round-robin dealer gets at most
// ceil(K nsplit / P) items of at most ceil(ceil(T / TROWS) / nsplit) tiles each.  Every (k, split) slot of the album is
// written exactly once: by the dealer whose piece it is, else as an empty partial (flat: by workgroup g0 = 0 up front;
// round-robin: by the dealer the item was dealt to).
template <int TROWS>
__device__ __forceinline__ int tiles_of(int rows) {
  static_assert(TROWS == 16 || TROWS == 32, "tile rows");
  return (rows + TROWS - 1) >> (TROWS == 16 ? 4 : 5);
}
struct Seg {  // a dealer's piece: consecutive tiles [t0, t1) of one stream, summed into one partial
  int nk, t0, t1, slot, cnt, allm;
};
struct AttnDeal {
  const int *kstart, *kcnt, *kall;  // the n's streams (LDS): first flat tile, valid rows, fully masked
  float* part;        // the partials [N K][nsplit][w + 4]
  int w;
  int n, K, nsplit, P, pg;
  int tot, lo, hi;    // flat: the album's tiles, this dealer's run
  int it_k, it_il;    // where next_seg stands: flat / round-robin
  bool flat;
  bool first_wg;      // workgroup g0 = 0 of the album: fills the partial slots no flat run owns
  bool writer;        // this lane writes the empty partials of the round-robin items its dealer passes over (one lane per dealer)
};
// one thread fills the stream table of album n and decides flat / round-robin
template <int TROWS>
__device__ __forceinline__ void deal_streams(const AttnSaved& sv, int n, int K, int nsplit, int P, int* kstart, int* kcnt, int* kall,
                                             int* flat) {
  int acc = 0;
  for (int k = 0; k < K; ++k) {
    const int c = sv.cnt[n * K + k];
    kcnt[k] = c;
    kall[k] = sv.allmasked[n * K + k];
    kstart[k] = acc;
    acc += tiles_of<TROWS>(c);
  }
  kstart[K] = acc;
  int ok = acc > 0;
  for (int k = 0; k < K && ok; ++k) {
    const int st = kstart[k], en = kstart[k + 1];
    if (en > st && ((en * P - 1) / acc) - (((st + 1) * P - 1) / acc) + 1 > nsplit) ok = 0;
  }
  *flat = ok;
}
// every thread, after the barrier behind deal_streams: dealer d of the D in workgroup g0 (of G on this n)
template <int D>
__device__ __forceinline__ AttnDeal deal_init(const int* kstart, const int* kcnt, const int* kall, int flat, const AttnFwdArgs& a, int n,
                                              int g0, int G, int d, bool writer) {
  AttnDeal dl;
  dl.kstart = kstart, dl.kcnt = kcnt, dl.kall = kall;
  dl.part = a.part, dl.w = a.s.w;
  dl.n = n, dl.K = a.s.K, dl.nsplit = a.s.nsplit;
  dl.first_wg = g0 == 0, dl.writer = writer;
  dl.P = D * G, dl.pg = D * g0 + d;
  dl.flat = flat != 0;
  dl.tot = kstart[dl.K];
  dl.lo = dl.flat ? dl.tot * dl.pg / dl.P : 0, dl.hi = dl.flat ? dl.tot * (dl.pg + 1) / dl.P : 0;
  dl.it_k = 0, dl.it_il = g0 + G * d - D * G;
  return dl;
}
__device__ __forceinline__ void deal_empty_partial(const AttnDeal& dl, int nk, int split) {
  store_empty_partial(dl.part + ((size_t)nk * dl.nsplit + split) * (dl.w + 4));
}
// flat dealing, the workgroup g0 = 0 of the album (all NT threads): the partial slots no dealer fills
template <int NT>
__device__ __forceinline__ void deal_fill_unowned(const AttnDeal& dl, int tid) {
  if (dl.flat && dl.first_wg) {
    const int P = dl.P, tot = dl.tot;
    for (int e = tid; e < dl.K * dl.nsplit; e += NT) {
      const int k = e / dl.nsplit, sp = e % dl.nsplit;
      const int st = dl.kstart[k], en = dl.kstart[k + 1];
      bool filled = false;  // slot sp belongs to dealer (first dealer that touches k) + sp, if that dealer's run meets k at all
      if (en > st) {
        const int px = ((st + 1) * P - 1) / tot + sp;
        filled = px < P && max(tot * px / P, st) < min(tot * (px + 1) / P, en);
      }
      if (!filled) deal_empty_partial(dl, dl.n * dl.K + k, sp);
    }
  }
}
template <int TROWS>
__device__ __forceinline__ bool item_seg(const AttnDeal& dl, int il, Seg& sg) {  // round-robin dealing: item il = (k, split)
  const int k = il / dl.nsplit, split = il % dl.nsplit;
  const int c = dl.kcnt[k];
  const int tiles_total = tiles_of<TROWS>(c);
  const int tiles_per = (tiles_total + dl.nsplit - 1) / dl.nsplit;
  sg.nk = dl.n * dl.K + k;
  sg.t0 = split * tiles_per;
  sg.t1 = min(tiles_total, sg.t0 + tiles_per);
  sg.slot = split;
  sg.cnt = c;
  sg.allm = dl.kall[k];
  return sg.t1 > sg.t0;
}
// the dealer's next piece; false: none left
template <int TROWS>
__device__ __forceinline__ bool next_seg(AttnDeal& dl, Seg& sg) {
  if (dl.flat) {
    while (dl.it_k < dl.K) {
      const int k = dl.it_k++;
      const int st = dl.kstart[k], en = dl.kstart[k + 1];
      if (st >= dl.hi) break;
      const int x0 = max(dl.lo, st), x1 = min(dl.hi, en);
      if (x0 < x1) {
        sg.nk = dl.n * dl.K + k;
        sg.t0 = x0 - st;
        sg.t1 = x1 - st;
        sg.slot = dl.pg - ((st + 1) * dl.P - 1) / dl.tot;
        sg.cnt = dl.kcnt[k];
        sg.allm = dl.kall[k];
        return true;
      }
    }
    dl.it_k = dl.K;
    return false;
  }
  for (;;) {
    dl.it_il += dl.P;
    if (dl.it_il >= dl.K * dl.nsplit) return false;
    if (item_seg<TROWS>(dl, dl.it_il, sg)) return true;
    if (dl.writer) deal_empty_partial(dl, sg.nk, sg.slot);  // empty split
  }
}
// tiles (= rounds of the tile loop) this dealer will be handed in all; before the first next_seg
template <int TROWS>
__device__ __forceinline__ int deal_rounds(const AttnDeal& dl) {
  int rounds = dl.hi - dl.lo;
  if (!dl.flat) {
    rounds = 0;
    Seg sg;
    for (int il = dl.it_il + dl.P; il < dl.K * dl.nsplit; il += dl.P)
      if (item_seg<TROWS>(dl, il, sg)) rounds += sg.t1 - sg.t0;
  }
  return rounds;
}
// the tile behind tile ftl of piece `from`: the same piece's next tile, or the first of the next piece
template <int TROWS>
__device__ __forceinline__ bool tile_after(AttnDeal& dl, const Seg& from, int ftl, Seg& to, int& ttl) {
  if (ftl + 1 < from.t1) {
    to = from;
    ttl = ftl + 1;
    return true;
  }
  if (next_seg<TROWS>(dl, to)) {
    ttl = to.t0;
    return true;
  }
  return false;
}

// ---- the hand-shake of a pair of waves through LDS flags (attn_fwd_pair16<FLAGS>, attn_fwd_pair16h)
// (the flags are accessed through LDS-address-space pointers: through a generic pointer the compiler emits FLAT
//  loads/stores, whose s_waitcnt vmcnt(0) would also wait for every outstanding load of the next tile)
typedef __attribute__((address_space(3))) int lds_int;
__device__ __forceinline__ void wait_flag(int* flag, int want, int* fault) {  // bounded poll of an LDS word
  volatile lds_int* f = (volatile lds_int*)flag;
  bool arrived = false;
  // (the partner wave is resident in this very workgroup: it can only be DELAYED -- counter collection serialising waves,
  //  pre-emption, a debugger -- so the bound is generous: 2^28 polls of s_sleep 2, tens of seconds)
  for (int spin = 0; spin < (1 << 28); ++spin) {
    if (*f >= want) {
      arrived = true;
      break;
    }
    __builtin_amdgcn_s_sleep(2);
  }
  // a partner that never arrives is a bug (a wedged wave).  The trap aborts the queue -- on ROCm that usually ends the
  // process, it is NOT a recoverable launch error -- which is still better than folding stale partials into amax /
  // jmax / h_a and training on them
  if (!arrived) {
    if (fault) {  // (host-mapped: visible to the host once the system-scope fence has drained)
      __hip_atomic_store(fault, (int)ATTN_FAULT_PAIR_WAIT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __threadfence_system();
    }
    __builtin_trap();
  }
  // acquire: the partner's published area (plain LDS loads below) is read only after the poll has matched; workgroup
  // scope lowers to s_waitcnt lgkmcnt(0) and, unlike an empty asm, is a compiler fence for __shared__ accesses too
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ void post_flag(int* flag, int v) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // my partials are written before the flag says so
  *(volatile lds_int*)flag = v;
}

// ---- staging album n's question operand (fp16 hi / lo pieces, B layout of v_mfma_f32_16x16x32_f16), the row-term
// vectors and ct into LDS, 512 threads, w <= 1024.  s_qhi / s_qlo: [NKT][2][64] half8, k-step ks, j tile jt, lane
// (col l15, k group q4) holds the 8 channels of Qh rows 8 ks + QM q4 and + QD: (QM, QD) = (1, 4) for rows loaded 4
// channels per lane and 16-channel block (channels 32 ks + 4 q4 + (0..3) and + 16), (2, 1) for the NATURAL order of
// 16-byte loads (channels 32 ks + 8 q4 .. + 7).
template <int NKT, int QM, int QD>
__device__ __forceinline__ void stage_question(const AttnSaved& sv, int n, int w, int JP, int tid, half8 (*s_qhi)[2][64], half8 (*s_qlo)[2][64],
                                               float* s_vec, float* s_ct) {
  const int W4c = w / 4;
  const uint16_t* qh = sv.Qh + (size_t)n * 2 * W4c * 32 * 4;
  // every load of the staging is issued before the first LDS write: as a rolled loop (two loads, wait, write) the
  // 128 KB took 16 dependent round trips per thread, 35-50 k cycles before the first tile was even requested
  typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  constexpr int QIT = 2 * NKT * 2 * 64 / 512;
  u32x2 x0[QIT], x1[QIT];
#pragma unroll
  for (int it = 0; it < QIT; ++it) {
    const int e = tid + 512 * it;
    const int ln = e & 63, jt = (e >> 6) & 1, ks = (e >> 7) % NKT, pc = (e >> 7) / NKT;
    const int j = (ln & 15) + 16 * jt, q4 = ln >> 4;
    x0[it] = *reinterpret_cast<const u32x2*>(qh + (((size_t)pc * W4c + 8 * ks + QM * q4) * 32 + j) * 4);
    x1[it] = *reinterpret_cast<const u32x2*>(qh + (((size_t)pc * W4c + 8 * ks + QM * q4 + QD) * 32 + j) * 4);
  }
  float v0[2], v1[2];  // w <= 1024: at most two channels of each row-term vector per thread
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int c = tid + 512 * it;
    v0[it] = c < w ? sv.vecs[VEC_RH * w + c] : 0.f;
    v1[it] = c < w ? sv.vecs[VEC_R2 * w + c] : 0.f;
  }
  const float ctv = tid < 32 ? sv.ct[(size_t)n * JP + tid] : 0.f;
#pragma unroll
  for (int it = 0; it < QIT; ++it) {
    const int e = tid + 512 * it;
    const int ln = e & 63, jt = (e >> 6) & 1, ks = (e >> 7) % NKT, pc = (e >> 7) / NKT;
    const u32x4 xx = __builtin_shufflevector(x0[it], x1[it], 0, 1, 2, 3);
    (pc == 0 ? s_qhi : s_qlo)[ks][jt][ln] = __builtin_bit_cast(half8, xx);
  }
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int c = tid + 512 * it;
    if (c < w) {
      s_vec[c] = v0[it];
      s_vec[w + c] = v1[it];
    }
  }
  if (tid < 32) s_ct[tid] = ctv;
}

// ---- the row term h.(Rh + R2 h) of 4 channels (vec[irh ..], vec[ir2 ..]: the two vectors at those channels, LDS), 4-wide
// so that it stays two packed FMAs per block.  (base + index, not ready-made pointers: the address is then formed where it
// is used, in the order of the spelled-out expression -- with pointers formed at the call the RMODE 2 kernels came out a
// few instructions longer.)  RMODE: which vectors of the bilinear form are non-zero: 1 = Rh (simi 1), 2 = R2 (simi 2
// and 4), 3 = both (simi 3)
template <int RMODE>
__device__ __forceinline__ void row_term(f32x4& rt4, const f32x4 h, const float* vec, int irh, int ir2) {
  if (RMODE == 1)
    rt4 += h * *reinterpret_cast<const f32x4*>(&vec[irh]);
  else if (RMODE == 2)
    rt4 += (h * h) * *reinterpret_cast<const f32x4*>(&vec[ir2]);
  else
    rt4 += h * (*reinterpret_cast<const f32x4*>(&vec[irh]) + *reinterpret_cast<const f32x4*>(&vec[ir2]) * h);
}
// the same over two blocks of 4 channels, DC channels apart, added as one sum (a different rounding from two row_terms)
template <int RMODE, int DC>
__device__ __forceinline__ void row_term2(f32x4& rt4, const f32x4 h0, const f32x4 h1, const float* vec, int irh, int ir2) {
  if (RMODE == 1)
    rt4 += h0 * *reinterpret_cast<const f32x4*>(&vec[irh]) + h1 * *reinterpret_cast<const f32x4*>(&vec[irh + DC]);
  else if (RMODE == 2)
    rt4 += (h0 * h0) * *reinterpret_cast<const f32x4*>(&vec[ir2]) + (h1 * h1) * *reinterpret_cast<const f32x4*>(&vec[ir2 + DC]);
  else
    rt4 += h0 * (*reinterpret_cast<const f32x4*>(&vec[irh]) + *reinterpret_cast<const f32x4*>(&vec[ir2]) * h0) +
           h1 * (*reinterpret_cast<const f32x4*>(&vec[irh + DC]) + *reinterpret_cast<const f32x4*>(&vec[ir2 + DC]) * h1);
}

// ---- finishing a 16-row tile's scores inside a wave.  D layout of 16x16xK: lane -> column j = l15 (+ 16 jt), rows
// 4 kq + i.  score(jt, i): the bilinear part of x[row 4 kq + i][j]; rterm(i): that row's row term.  Per row: max / FIRST
// arg-max over the valid j of score + rterm + ct[j]; then row l15's result, which sits in the lane group l15 >> 2 as its
// entry l15 & 3, goes to every lane of the row.
template <class Score, class RTerm>
__device__ __forceinline__ void finish_scores(Score score, RTerm rterm, const float* s_ct, uint64_t qvalid, int l15, float& bestv, int& bestj) {
  float amr[4];
  int jmr[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float rti = rterm(i);
    float best = -INFINITY;
    int bj = 0;
#pragma unroll
    for (int jt = 0; jt < 2; ++jt) {
      const int j = l15 + 16 * jt;
      const float x = score(jt, i) + rti + s_ct[j];
      if (((qvalid >> j) & 1ull) && x > best) {
        best = x;
        bj = j;
      }
    }
    row16_argmax(best, bj);
    amr[i] = best;
    jmr[i] = bj;
  }
  const int src = ((l15 >> 2) << 4) | l15;
  bestv = 0.f;
  bestj = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float v = __shfl(amr[i], src, 64);
    const int jj = __shfl(jmr[i], src, 64);
    if ((l15 & 3) == i) {
      bestv = v;
      bestj = jj;
    }
  }
}

// ---- one step of the online softmax over t (softsel inner, model_v2.py:278).  Precondition: every lane of a DPP row holds
// the logit `am` of its own row l15 of the tile, and all four DPP rows of the wave hold the SAME tile's 16 logits -- then
// m_new and scale are equal in every lane and the rescale branch does not diverge.  Returns the row's weight; the
// accumulators are rescaled to the new maximum.
template <int NU>
__device__ __forceinline__ float softmax_step(float am, float& m_run, float& l_run, f32x4 (&u)[NU]) {
  const float m_new = fmaxf(m_run, row16_max(am));
  const float scale = expf(m_run - m_new);
  const float pr = expf(am - m_new);
  l_run = l_run * scale + row16_sum(pr);
  m_run = m_new;
  if (scale != 1.f) {  // (the running max rarely moves after the first tiles of an item)
#pragma unroll
    for (int i = 0; i < NU; ++i) u[i] *= scale;
  }
  return pr;
}

}  // namespace fvta

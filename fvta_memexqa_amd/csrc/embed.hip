// Token embedding for gfx950: model_v2.py:524-645 (char lookup -> conv1d 52-70 -> concat with the word lookup).  SURVEY.md
// 8f rank 1: the step immediately before the encoders.  A token's row (char part | word part) is written once, straight
// into the encoder input arena; the backward leaves the char-CNN gradients in per-workgroup (or per-wave) slabs that
// embed_bwd_reduce_kernel sums in a fixed order, and adds the trainable word rows by atomics.  Four kernel families:
//  * general (embed_fwd_general<BIG> / embed_bwd_general<BIG>): a 128-thread workgroup walks tokens, thread f owns filter f.
//    BIG = false: height * cdim <= 64 and W * cdim <= 1024, filter in registers (forward) / LDS (backward) -- every narrow shape
//    the wave-per-token kernels do not take, and cwdim == 0 (word rows only).  BIG = true: any deeper window, filter streamed
//    from L2 -- the tested fallback of the wide kernels (FVTA_EMBED_MFMA=0, wdim > 128, VC > 128, W > 16, cwdim != 100);
//  * wave per token (embed_fwd_5x8_mfma / embed_bwd_5x8_char / embed_bwd_5x8_filt): the reference's default shape, height 5,
//    cdim 8, 100 filters, W <= 16, VC <= 256, on the fp32 matrix pipe;
//  * workgroup per token (embed_fwdw_f16x3 / embed_bwdw_filt_tok / embed_bwdw_char_tok): the published flag set's shape,
//    height 5, cdim 100, 100 filters, 5 <= W <= 16, wdim <= 128, VC <= 128, on the fp16 / bf16 matrix pipe.
// The photo-feature transform is image_trans.hip.
#include "fvta_common.h"
#include "attn_fwd_shared.h"  // split_f16x2: the fp16 (hi, lo') split of an fp32 value
#ifndef FVTA_EMBW_ABL
#define FVTA_EMBW_ABL 0   // timing ablations of the wide forward embed_fwdw_f16x3 (results garbage): 256 no k loop, 512 no staging
                          // stores, 1024 no barrier (bits 1 .. 128 belonged to the wave-per-(token, slice) backward kernels: gone with them)
#endif

namespace fvta {

constexpr int EMB_NT = 128;       // threads = max cwdim
constexpr int EMB_MAXKC = 64;     // height * cdim of the register-resident kernels
constexpr int EMB_MAXWC = 1024;   // W * cdim of the register-resident kernels
constexpr int EMB_BIG_WC = 8192;  // W * cdim of the general kernels (the published flag set: char_emb_size 100)
constexpr int EMB_MAXVC = 1024;   // char vocabulary (backward's per-workgroup table)
constexpr int EMB_BWD_BLOCKS = 2048;  // slabs of the backward workspace (one per workgroup, or per wave of the wave-per-token kernels)

// a slab of the backward workspace: [KC * cwdim d filt | cwdim d bias | VC * cdim d char_emb], KC = height * cdim
struct EmbSlab {
  size_t bias, chars, floats;  // offsets of the bias and char parts (the filter part is at 0), floats of one slab
  __host__ __device__ EmbSlab(int KC, int cwdim, int VC, int cdim)  // (kernels of one shape pass their compile-time sizes)
      : bias((size_t)KC * cwdim), chars(bias + cwdim), floats(chars + (size_t)VC * cdim) {}
  __host__ __device__ EmbSlab(const fvta_embed_desc& d) : EmbSlab(d.height * d.cdim, d.cwdim, d.VC, d.cdim) {}
};

struct EmbArgs {
  fvta_embed_desc d;
  const int32_t* word_ids;
  const int32_t* char_ids;
  const int64_t* tok_off;
  const float* word_emb;
  const float* fixed_emb;
  const float* char_emb;
  const float* filt;
  const float* bias;
  float* x;
  uint8_t* argpos;
  // backward
  const float* dx;
  float* d_word_emb;
  float* slab;  // [blocks] EmbSlab
  // conv1d's dropout of the gathered char embeddings while training (model_v2.py:58-62): element (tok, pos, c) of the
  // [ntok, W, cdim] block is kept by the hash of (seed, (tok * W + pos) * cdim + c) and scaled by 1 / keep_prob; thr 0 = off
  unsigned long long drop_thr, drop_seed;
  float drop_scale;
};
// keep / scale factor of element i = pos * cdim + c of token tok's character block (WC = W * cdim)
__device__ __forceinline__ float emb_ks(const EmbArgs& a, int tok, int i, int WC) {
  if (a.drop_thr == 0ull) return 1.f;
  return dropout_keep(a.drop_seed, (unsigned long long)tok * WC + i, a.drop_thr) ? a.drop_scale : 0.f;
}
// the arguments every launch shares (the caller fills in its own tables, outputs and gradients)
static inline EmbArgs emb_args(const fvta_embed_desc* d, const int32_t* word_ids, const int32_t* char_ids, const int64_t* tok_off,
                               const float* char_emb, const float* filt, const uint8_t* argpos) {
  EmbArgs a{};
  a.d = *d;
  a.word_ids = word_ids; a.char_ids = char_ids; a.tok_off = tok_off;
  a.char_emb = char_emb; a.filt = filt; a.argpos = const_cast<uint8_t*>(argpos);
  a.drop_thr = (d->keep_prob > 0.f && d->keep_prob < 1.f) ? dropout_thr(d->keep_prob) : 0ull;
  a.drop_seed = d->dropout_seed;
  a.drop_scale = a.drop_thr ? 1.0f / d->keep_prob : 1.f;
  return a;
}

// ---- what the kernels below share ------------------------------------------------------------------------------------
// The matrix-pipe kernels sit at the edge of their register budgets (embed_bwdw_filt_tok 256 VGPRs, embed_bwdw_char_tok 248,
// embed_fwd_5x8_mfma 168 = its launch bound), and their schedules move with the spelling of the source: each of them uses a
// helper from here only where its instruction stream came out unchanged.  What stays spelled out in them for that reason: the
// slab address in embed_bwd_5x8_char / _filt and embed_bwdw_filt_tok (int arithmetic there, folded into their stores), the
// 5 x 8 kernels' per-lane setup and look-ahead loads, the word-row atomics (the matrix-pipe kernels hold the elements in registers),
// the ReLU / arg-max store of embed_fwdw_f16x3, the four-pair fp16 splits of the wide kernels.
// this workgroup's (wave's) slab
__device__ __forceinline__ float* emb_slab(const EmbArgs& a, const EmbSlab& sl, unsigned idx) { return a.slab + (size_t)idx * sl.floats; }
// a word's row: the trainable table first, then the fixed (pre-trained) one
__device__ __forceinline__ const float* emb_word_src(const EmbArgs& a, int id) {
  return id < a.d.VW ? a.word_emb + (size_t)id * a.d.wdim : a.fixed_emb + (size_t)(id - a.d.VW) * a.d.wdim;
}
// token index clamped to the last token (look-ahead loads stay branch-free) and hidden from the compiler's uniformity
// analysis: it would move each freshly loaded id / offset into scalar registers with v_readfirstlane -- behind an
// s_waitcnt vmcnt(0) in every iteration, a round trip that also drains the prefetch queue
__device__ __forceinline__ int emb_ctok(const EmbArgs& a, int t) {
  int c = t < a.d.ntok ? t : a.d.ntok - 1;
  asm volatile("" : "+v"(c));
  return c;
}
// y = max over the windows + bias -> ReLU; the arg-max position is kept for the active filters only (255: inactive)
__device__ __forceinline__ void emb_relu_argpos(float best, float bias, int bp, float& y_out, uint8_t& ap_out) {
  const float y = best + bias;
  y_out = y > 0.f ? y : 0.f;
  ap_out = y > 0.f ? (uint8_t)bp : (uint8_t)255;
}
// token tok's character block [W][cdim], gathered and dropped, into E (EMB_NT threads)
__device__ __forceinline__ void emb_gather_block(const EmbArgs& a, int tok, int tid, float* E) {
  const fvta_embed_desc& d = a.d;
  const int WC = d.W * d.cdim;
  for (int i = tid; i < WC; i += EMB_NT)
    E[i] = a.char_emb[(size_t)a.char_ids[(size_t)tok * d.W + i / d.cdim] * d.cdim + i % d.cdim] * emb_ks(a, tok, i, WC);
}

// ---- general shapes: one 128-thread workgroup walks tokens, thread f owns filter f; the token's W x cdim character
// embeddings sit in LDS and are read as broadcasts.  Per token the default char-CNN is 12 windows x 100 filters x 40 MACs --
// 1.6 % of one LSTM step's work -- so this is a gather/scatter problem, not a GEMM.
// BIG = false: the filter's height * cdim <= EMB_MAXKC weights in registers; also the cwdim == 0 path (word rows only).
// BIG = true (any height * cdim, W * cdim <= EMB_BIG_WC): correct and order-fixed, not fast -- the filter does not fit
// registers or LDS, so it is streamed from L2 (coalesced over the filter index); dynamic LDS E [W * cdim].
template <bool BIG>
__global__ __launch_bounds__(EMB_NT) void embed_fwd_general(EmbArgs a) {
  __shared__ float s_Es[BIG ? 1 : EMB_MAXWC];
  extern __shared__ float s_dyn[];
  const fvta_embed_desc& d = a.d;
  const int tid = threadIdx.x;
  const int KC = d.height * d.cdim, P = d.W - d.height + 1;
  float* s_E = BIG ? s_dyn : s_Es;
  float wf[BIG ? 1 : EMB_MAXKC];
  float bf = 0.f;
  if (tid < d.cwdim) {
    if constexpr (!BIG)
#pragma unroll
      for (int i = 0; i < EMB_MAXKC; ++i) wf[i] = i < KC ? a.filt[(size_t)i * d.cwdim + tid] : 0.f;
    bf = a.bias[tid];
  }
  for (int tok = blockIdx.x; tok < d.ntok; tok += gridDim.x) {
    float* row = a.x + a.tok_off[tok];
    if (BIG || d.cwdim > 0) {
      __syncthreads();  // the previous token's readers of s_E are done
      emb_gather_block(a, tok, tid, s_E);
      __syncthreads();
      if (tid < d.cwdim) {
        float best = -INFINITY;
        int bp = 0;
        for (int p = 0; p < P; ++p) {
          const float* e = s_E + p * d.cdim;  // the window's height*cdim values are contiguous
          float v = 0.f;
          if constexpr (BIG) {
            for (int i = 0; i < KC; ++i) v += e[i] * a.filt[(size_t)i * d.cwdim + tid];
          } else {
#pragma unroll
            for (int i = 0; i < EMB_MAXKC; ++i)
              if (i < KC) v += e[i] * wf[i];
          }
          if (v > best) {  // first arg-max
            best = v;
            bp = p;
          }
        }
        emb_relu_argpos(best, bf, bp, row[tid], a.argpos[(size_t)tok * d.cwdim + tid]);
      }
    }
    const float* src = emb_word_src(a, a.word_ids[tok]);
    for (int i = tid; i < d.wdim; i += EMB_NT) row[d.cwdim + i] = src[i];
  }
}

// gradients of the char-CNN parameters per workgroup (fixed token order), word rows by atomics.
// BIG = false: partial d filt / d bias in registers, filter and char table dC in dynamic LDS (filt [KC][cwdim], then
// dC [VC][cdim]), written to the slab at the end.  BIG = true: the slab of this workgroup is zeroed by the launcher and
// accumulated in place by the owner threads of its columns, the filter is streamed; dynamic LDS E [W*cdim], dE [W*cdim].
template <bool BIG>
__global__ __launch_bounds__(EMB_NT) void embed_bwd_general(EmbArgs a) {
  __shared__ float s_EdE[BIG ? 1 : 2 * EMB_MAXWC];
  __shared__ float s_g[EMB_NT];
  __shared__ int s_p[EMB_NT];
  __shared__ int s_ch[64];
  extern __shared__ float s_dyn[];
  const fvta_embed_desc& d = a.d;
  const int tid = threadIdx.x;
  const int KC = d.height * d.cdim, WC = d.W * d.cdim;
  const EmbSlab sl(d);
  float* slab = emb_slab(a, sl, blockIdx.x);
  float* s_E = BIG ? s_dyn : s_EdE;
  float* s_dE = BIG ? s_dyn + WC : s_EdE + EMB_MAXWC;
  float* s_filt = s_dyn;                 // (!BIG)
  float* s_dC = s_dyn + KC * d.cwdim;    // (!BIG)
  float acc[BIG ? 1 : EMB_MAXKC];
  float accb = 0.f;
  if constexpr (!BIG) {
#pragma unroll
    for (int i = 0; i < EMB_MAXKC; ++i) acc[i] = 0.f;
    if (d.cwdim > 0) {
      for (int i = tid; i < KC * d.cwdim; i += EMB_NT) s_filt[i] = a.filt[i];
      for (int i = tid; i < d.VC * d.cdim; i += EMB_NT) s_dC[i] = 0.f;
    }
  }
  for (int tok = blockIdx.x; tok < d.ntok; tok += gridDim.x) {
    const float* row = a.dx + a.tok_off[tok];
    const int id = a.word_ids[tok];
    if (id < d.VW)  // (the fixed rows get no gradient)
      for (int i = tid; i < d.wdim; i += EMB_NT) atomicAdd(a.d_word_emb + (size_t)id * d.wdim + i, row[d.cwdim + i]);
    if (!BIG && d.cwdim == 0) continue;
    __syncthreads();
    if (tid < d.W) s_ch[tid] = a.char_ids[(size_t)tok * d.W + tid];
    emb_gather_block(a, tok, tid, s_E);
    float g = 0.f;  // thread f: the gradient of filter f's output and its arg-max position (inactive filters: 0, 0)
    int p = 0;
    if (tid < d.cwdim) {
      const int ap = a.argpos[(size_t)tok * d.cwdim + tid];
      if (ap != 255) {
        g = row[tid];
        p = ap;
      }
    }
    s_g[tid] = g;
    s_p[tid] = p;
    __syncthreads();
    // d filt[:, :, f] += g * window(p); d bias[f] += g
    const float* e = s_E + p * d.cdim;
    if constexpr (BIG) {
      if (tid < d.cwdim && g != 0.f) {  // the owner of filter column f accumulates its slab column
        slab[sl.bias + tid] += g;
        for (int i = 0; i < KC; ++i) slab[(size_t)i * d.cwdim + tid] += g * e[i];
      }
    } else if (tid < d.cwdim) {
      accb += g;
#pragma unroll
      for (int i = 0; i < EMB_MAXKC; ++i)
        if (i < KC) acc[i] += g * e[i];
    }
    // d E[pos][c] = sum_f g_f * filt[pos - p_f][c][f], one thread per (pos, c), f in order (inactive filters carry g = 0
    // and p = 0: they only cost the compare)
    const float* filt = BIG ? a.filt : s_filt;
    for (int i = tid; i < WC; i += EMB_NT) {
      const int pos = i / d.cdim, c = i % d.cdim;
      float v = 0.f;
      for (int f = 0; f < d.cwdim; ++f) {
        const int k = pos - s_p[f];
        const float gf = s_g[f];
        if (gf != 0.f && k >= 0 && k < d.height) v += gf * filt[(size_t)(k * d.cdim + c) * d.cwdim + f];
      }
      s_dE[i] = v * emb_ks(a, tok, i, WC);  // (dropout: the gradient reaches the table through the kept elements only)
    }
    __syncthreads();
    // into the workgroup's char table: thread c walks the positions serially (two positions may hold the same char)
    float* dC = BIG ? slab + sl.chars : s_dC;
    if (tid < d.cdim)
      for (int pos = 0; pos < d.W; ++pos) dC[(size_t)s_ch[pos] * d.cdim + tid] += s_dE[pos * d.cdim + tid];
  }
  if (BIG || d.cwdim == 0) return;
  __syncthreads();
  if (tid < d.cwdim) {
#pragma unroll
    for (int i = 0; i < EMB_MAXKC; ++i)
      if (i < KC) slab[(size_t)i * d.cwdim + tid] = acc[i];
    slab[sl.bias + tid] = accb;
  }
  for (int i = tid; i < d.VC * d.cdim; i += EMB_NT) slab[sl.chars + i] = s_dC[i];
}

// ---- the reference's shape on the matrix pipe: one WAVE per token ------------------------------------------------------
// The general kernels above spend their time waiting (two to four workgroup barriers and an LDS read-modify-write chain
// per token), not computing.  Here a wave owns a token from its ids to its gradients and never meets a workgroup barrier:
//  * forward: Y[p][f] = sum_kc E[p*8 + kc] filt[kc][f] is a 16 x 40 x CW product on v_mfma_f32_16x16x4_f32 (an exact fmaf
//    chain per output): rows = window positions (12 of 16 used), the filter fragments live in registers for the whole
//    launch, the A operand is the token's character block read from LDS; max / first arg-max over the rows of an
//    accumulator tile, then across the three lane groups that hold a column's rows;
//  * backward: the scatter of each active filter's 5 x 8 weights to its arg-max window is the product
//    T[p][kc] = sum_f G[p][f] filt[kc][f] with the one-hot G[p][f] = g_f [argpos_f == p] built on the fly from the staged
//    gradient row (12 x more MACs than the scatter, no dependent LDS chain); dE[p*8 + kc] += T[p][kc] by LDS float adds whose
//    addresses are distinct within an instruction and ordered between instructions (one wave, in-order LDS: a fixed
//    order), then into the wave's own char-gradient table; d filt stays the sparse form (lane f: 40 FMAs against the
//    window of ITS arg-max position).  Every wave writes its own slab; embed_bwd_reduce_kernel sums them in order.
// Word part as in the general kernels.  Shape: height 5, cdim 8, W <= 16, cwdim == CW (a multiple of 4, <= 128).
#ifndef FVTA_EMB_ABL
#define FVTA_EMB_ABL 0  // timing ablations (SRC=embed MACRO=FVTA_EMB_ABL tools/build_abl.sh): 1 no MFMA, 2 no LDS adds / no arg-max epilogue, 4 no stores
#endif
template <int CW>
struct Emb5x8 {
  static constexpr int NW = 4;                    // waves per workgroup
  static constexpr int NKS = CW / 4;              // backward: k-steps over the filters
  static constexpr int GP = (NKS + 3) / 4 * 4;    // staged gradient row: run of one k phase (f & 3), padded to 16 bytes
  static constexpr int NCF = (CW + 15) / 16;      // forward: column tiles over the filters
  static_assert(CW % 4 == 0 && CW > 64 && CW <= 128 && GP <= 32, "cwdim of the matrix-pipe char-CNN kernels");
};

__device__ __forceinline__ void wave_lds_fence() {  // orders this wave's LDS traffic for the compiler (the unit is in-order)
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ void lds_fadd(float* p, float v) {  // ds_add_f32, no return value
  (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <int CW>
__global__ __launch_bounds__(256, 3) void embed_fwd_5x8_mfma(EmbArgs a) {
  using C = Emb5x8<CW>;
  extern __shared__ __attribute__((aligned(16))) float s_dyn[];  // char_emb [VC][8]
  __shared__ __attribute__((aligned(16))) float s_E[C::NW][160], s_Y[C::NW][128];
  __shared__ uint8_t s_A[C::NW][128];
  __shared__ float s_bias[128];
  const fvta_embed_desc& d = a.d;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int j = lane & 15, q = lane >> 4;
  const int W = d.W, P = W - 4;
  for (int i = threadIdx.x; i < d.VC * 8; i += 256) s_dyn[i] = a.char_emb[i];
  if (lane < 32) s_E[wv][128 + lane] = 0.f;  // rows 12..15 of the product read past the block
  if (threadIdx.x < 128) s_bias[threadIdx.x] = threadIdx.x < CW ? a.bias[threadIdx.x] : 0.f;
  float Bf[10][C::NCF];
#pragma unroll
  for (int ct = 0; ct < C::NCF; ++ct) {
    const int f = 16 * ct + j;
#pragma unroll
    for (int ks = 0; ks < 10; ++ks) Bf[ks][ct] = f < CW ? a.filt[(size_t)(4 * ks + q) * CW + f] : 0.f;
  }
  __syncthreads();
  const int step = gridDim.x * C::NW;
  const int pos = lane >> 3, c = lane & 7;
  // Loads are branch-free (indices clamped, never predicated): in straight-line code the compiler counts the loads in
  // flight exactly, so waiting for the oldest leaves the newer ones flying; behind branches it waits for all of them and
  // every token pays a memory round trip.  Pipeline: ids of token i+2, word row and product of token i.
  // (The fp32 MFMA runs at the vector pipe's fp32 rate and does not overlap vector work -- neither another wave's nor,
  // interleaved by sched_group_barrier, this wave's: measured, the product's and the arg-max's times add up.  So the
  // kernel is kept short and at three waves per SIMD.)
  const int posA = pos < W ? pos : W - 1, posB = pos + 8 < W ? pos + 8 : W - 1;
  const int wl0 = lane < d.wdim ? lane : d.wdim - 1, wl1 = lane + 64 < d.wdim ? lane + 64 : d.wdim - 1;
  auto load_ids = [&](int tok, int& cA, int& cB, int& wid, int64_t& off) {
    const int t = tok < d.ntok ? tok : d.ntok - 1;
    cA = a.char_ids[(size_t)t * W + posA];
    cB = a.char_ids[(size_t)t * W + posB];
    wid = a.word_ids[t];
    off = a.tok_off[t];
  };
  auto stage = [&](float* E, int tok, int cA, int cB) {
    E[lane] = pos < W ? s_dyn[cA * 8 + c] * emb_ks(a, tok, lane, W * 8) : 0.f;
    E[64 + lane] = pos + 8 < W ? s_dyn[cB * 8 + c] * emb_ks(a, tok, 64 + lane, W * 8) : 0.f;
  };
  auto product = [&](const float* E, f32x4 (&acc)[C::NCF]) {
#pragma unroll
    for (int ct = 0; ct < C::NCF; ++ct) acc[ct] = zero4();
#pragma unroll
    for (int ks = 0; ks < 10; ++ks) {
      const float av = E[j * 8 + 4 * ks + q];
#pragma unroll
      for (int ct = 0; ct < C::NCF; ++ct) {
        if constexpr (FVTA_EMB_ABL & 1) acc[ct][ks & 3] += av * Bf[ks][ct];
        else acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, Bf[ks][ct], acc[ct], 0, 0, 0);
      }
    }
  };
  // max / first arg-max over the window positions of every filter -> s_Y / s_A (branch-free: lanes without a result
  // write a spare slot)
  auto argmax = [&](const f32x4 (&acc)[C::NCF]) {
#pragma unroll
    for (int ct = 0; ct < ((FVTA_EMB_ABL & 4) ? 0 : C::NCF); ++ct) {
      float best = -INFINITY;
      int bp = 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int p = 4 * q + r;
        const float v = p < P ? acc[ct][r] : -INFINITY;
        const bool up = v > best;  // first arg-max
        best = up ? v : best;
        bp = up ? p : bp;
      }
      if constexpr (!(FVTA_EMB_ABL & 2)) {
        // the rows of lane groups 1 and 2 (positions 4..7, 8..11) of this column, brought to group 0 by the row / half
        // swaps of the vector pipe (no LDS traffic), folded in position order
        const float v1 = __uint_as_float(__builtin_amdgcn_permlane16_swap(__float_as_uint(best), __float_as_uint(best), false, false)[1]);
        const int p1 = (int)__builtin_amdgcn_permlane16_swap((unsigned)bp, (unsigned)bp, false, false)[1];
        const float v2 = __uint_as_float(__builtin_amdgcn_permlane32_swap(__float_as_uint(best), __float_as_uint(best), false, false)[1]);
        const int p2 = (int)__builtin_amdgcn_permlane32_swap((unsigned)bp, (unsigned)bp, false, false)[1];
        const bool u1 = v1 > best;
        best = u1 ? v1 : best;
        bp = u1 ? p1 : bp;
        const bool u2 = v2 > best;
        best = u2 ? v2 : best;
        bp = u2 ? p2 : bp;
      }
      const int f = 16 * ct + j;
      const int slot = (q == 0 && f < CW) ? f : 112 + j;
      emb_relu_argpos(best, s_bias[16 * ct + j], bp, s_Y[wv][slot], s_A[wv][slot]);
    }
    if constexpr (FVTA_EMB_ABL & 4) {
      float t = 0.f;
#pragma unroll
      for (int ct = 0; ct < C::NCF; ++ct) t += acc[ct][0] + acc[ct][1] + acc[ct][2] + acc[ct][3];
      s_Y[wv][lane] = t;
    }
  };
  auto flush = [&](int tok, int64_t off, int wid, float w0, float w1) {
    float* row = a.x + off;
    row[lane] = s_Y[wv][lane];
    a.argpos[(size_t)tok * CW + lane] = s_A[wv][lane];
    if (lane + 64 < CW) {
      row[64 + lane] = s_Y[wv][64 + lane];
      a.argpos[(size_t)tok * CW + 64 + lane] = s_A[wv][64 + lane];
    }
    if (lane < d.wdim) row[CW + lane] = w0;
    if (lane + 64 < d.wdim) row[CW + 64 + lane] = w1;
    if (d.wdim > 128) {
      const float* src = emb_word_src(a, wid);
      for (int i = lane + 128; i < d.wdim; i += 64) row[CW + i] = src[i];
    }
  };
  int tok = blockIdx.x * C::NW + wv;
  int cA0, cB0, wid0, cA1, cB1, wid1, cA2, cB2, wid2;
  int64_t off0, off1, off2;
  load_ids(tok, cA0, cB0, wid0, off0);
  load_ids(tok + step, cA1, cB1, wid1, off1);
  for (; tok < d.ntok; tok += step) {
    load_ids(tok + 2 * step, cA2, cB2, wid2, off2);
    const float w0 = emb_word_src(a, wid0)[wl0], w1 = emb_word_src(a, wid0)[wl1];  // stored after the product
    stage(s_E[wv], tok, cA0, cB0);
    wave_lds_fence();
    f32x4 acc[C::NCF];
    product(s_E[wv], acc);
    argmax(acc);
    wave_lds_fence();
    flush(tok, off0, wid0, w0, w1);
    wave_lds_fence();
    cA0 = cA1; cB0 = cB1; wid0 = wid1; off0 = off1;
    cA1 = cA2; cB1 = cB2; wid1 = wid2; off1 = off2;
  }
}

// backward, part 1 (matrix pipe): d char_emb.  Slab part [40 CW + CW ..) of this wave.
template <int CW>
__global__ __launch_bounds__(256, 3) void embed_bwd_5x8_char(EmbArgs a) {
  using C = Emb5x8<CW>;
  extern __shared__ __attribute__((aligned(16))) float s_dyn[];  // char_emb [VC][8], then dC [VC][8] per wave
  __shared__ __attribute__((aligned(16))) float s_T[C::NW][40 * 16], s_G[C::NW][4 * C::GP];
  __shared__ __attribute__((aligned(16))) uint8_t s_P[C::NW][4 * 32];
  const fvta_embed_desc& d = a.d;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int j = lane & 15, q = lane >> 4;
  const int W = d.W;
  float* dC = s_dyn + (size_t)d.VC * 8 * wv;
  for (int i = lane; i < d.VC * 8; i += 64) dC[i] = 0.f;
  float* Tt = s_T[wv];
  for (int i = lane; i < 4 * C::GP; i += 64) s_G[wv][i] = 0.f;
  for (int i = lane; i < 128; i += 64) s_P[wv][i] = 255;
  float Bf[C::NKS][3];
#pragma unroll
  for (int ct = 0; ct < 3; ++ct) {
    const int kc = 16 * ct + j;
#pragma unroll
    for (int ks = 0; ks < C::NKS; ++ks) Bf[ks][ct] = kc < 40 ? a.filt[(size_t)kc * CW + 4 * ks + q] : 0.f;
  }
  const int step = gridDim.x * C::NW;
  const int pos = lane >> 3, c = lane & 7;
  const bool has2 = lane + 64 < CW;
  // branch-free loads (see embed_fwd_5x8_mfma)
  const int posA = pos < W ? pos : W - 1, posB = pos + 8 < W ? pos + 8 : W - 1;
  const int lane2 = has2 ? 64 + lane : lane;
  auto load_ids = [&](int tok, int& cA, int& cB, int64_t& off) {
    const int t = tok < d.ntok ? tok : d.ntok - 1;
    cA = a.char_ids[(size_t)t * W + posA];
    cB = a.char_ids[(size_t)t * W + posB];
    off = a.tok_off[t];
  };
  auto load_grad = [&](int tok, int64_t off, int& ap1, int& ap2, float& g1, float& g2) {
    const int t = tok < d.ntok ? tok : d.ntok - 1;
    const float* row = a.dx + off;
    ap1 = a.argpos[(size_t)t * CW + lane];
    const int b2 = a.argpos[(size_t)t * CW + lane2];
    g1 = row[lane];
    g2 = row[lane2];
    ap2 = has2 ? b2 : 255;
  };
  int tok = blockIdx.x * C::NW + wv;
  int cA0, cB0, cA1, cB1, cA2, cB2, ap1, ap2, ap1n, ap2n;
  int64_t off0, off1, off2;
  float g1, g2, g1n, g2n;
  load_ids(tok, cA0, cB0, off0);
  load_ids(tok + step, cA1, cB1, off1);
  load_grad(tok, off0, ap1, ap2, g1, g2);
  for (; tok < d.ntok; tok += step) {
    load_ids(tok + 2 * step, cA2, cB2, off2);
    load_grad(tok + step, off1, ap1n, ap2n, g1n, g2n);
    // stage the gradient row in k-phase order (filter f at [(f & 3)][f >> 2])
    s_G[wv][(lane & 3) * C::GP + (lane >> 2)] = ap1 == 255 ? 0.f : g1;
    s_P[wv][(lane & 3) * 32 + (lane >> 2)] = (uint8_t)ap1;
    if (has2) {
      s_G[wv][(lane & 3) * C::GP + 16 + (lane >> 2)] = ap2 == 255 ? 0.f : g2;
      s_P[wv][(lane & 3) * 32 + 16 + (lane >> 2)] = (uint8_t)ap2;
    }
    wave_lds_fence();
    // T[p][kc] = sum_f G[p][f] filt[kc][f]: lane (p = j, k phase q) builds G from the staged row
    uint32_t Pv[8];
    {
      const uint4 p0 = *reinterpret_cast<const uint4*>(&s_P[wv][q * 32]);
      const uint4 p1 = *reinterpret_cast<const uint4*>(&s_P[wv][q * 32 + 16]);
      Pv[0] = p0.x; Pv[1] = p0.y; Pv[2] = p0.z; Pv[3] = p0.w;
      Pv[4] = p1.x; Pv[5] = p1.y; Pv[6] = p1.z; Pv[7] = p1.w;
    }
    f32x4 accT[3];
#pragma unroll
    for (int ct = 0; ct < 3; ++ct) accT[ct] = zero4();
#pragma unroll
    for (int v = 0; v < C::GP / 4; ++v) {
      const f32x4 Gv = *reinterpret_cast<const f32x4*>(&s_G[wv][q * C::GP + 4 * v]);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int ks = 4 * v + i;
        if (ks < C::NKS) {
          const int pb = (int)((Pv[v] >> (8 * i)) & 255u);
          const float av = pb == j ? Gv[i] : 0.f;
#pragma unroll
          for (int ct = 0; ct < 3; ++ct) {
            if constexpr (FVTA_EMB_ABL & 1) accT[ct][ks & 3] += av * Bf[ks][ct];
            else accT[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, Bf[ks][ct], accT[ct], 0, 0, 0);
          }
        }
      }
    }
    // T -> LDS as [kc][p] (a lane's four rows p = 4 q + r are one 16-byte store; rows 12..15 are zero: no arg-max there),
    // then dE[pos][c] = sum_k T[pos - k][8 k + c] by the lane of (pos, c): plain stores and loads, no LDS atomics
#pragma unroll
    for (int ct = 0; ct < 3; ++ct)
      if (16 * ct + j < 40) *reinterpret_cast<f32x4*>(&Tt[(16 * ct + j) * 16 + 4 * q]) = accT[ct];
    wave_lds_fence();
    float v0 = 0.f, v1 = 0.f;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const float t0 = Tt[(8 * k + c) * 16 + (pos >= k ? pos - k : 0)];
      const float t1 = Tt[(8 * k + c) * 16 + pos + 8 - k];
      v0 += pos >= k ? t0 : 0.f;
      v1 += t1;
    }
    v0 *= emb_ks(a, tok, lane, W * 8);
    v1 *= emb_ks(a, tok, 64 + lane, W * 8);
    // into the wave's char table; positions of one character meet inside the instruction (the LDS unit serialises them)
    if (pos < W) lds_fadd(&dC[cA0 * 8 + c], v0);
    if (pos + 8 < W) lds_fadd(&dC[cB0 * 8 + c], v1);
    wave_lds_fence();
    cA0 = cA1; cB0 = cB1; off0 = off1;
    cA1 = cA2; cB1 = cB2; off1 = off2;
    ap1 = ap1n; ap2 = ap2n; g1 = g1n; g2 = g2n;
  }
  float* slab = a.slab + (size_t)(blockIdx.x * C::NW + wv) * (40 * CW + CW + d.VC * 8);
  wave_lds_fence();
  for (int i = lane; i < d.VC * 8; i += 64) slab[40 * CW + CW + i] = dC[i];
}

// backward, part 2 (sparse form, vector pipe): d filt, d bias -- lane l owns filters l and 64 + l -- and the word rows.
// Slab part [0, 40 CW + CW) of this wave.
template <int CW>
__global__ __launch_bounds__(256, 2) void embed_bwd_5x8_filt(EmbArgs a) {
  using C = Emb5x8<CW>;
  extern __shared__ __attribute__((aligned(16))) float s_dyn[];  // char_emb [VC][8]
  __shared__ __attribute__((aligned(16))) float s_E[C::NW][160];
  const fvta_embed_desc& d = a.d;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int W = d.W;
  for (int i = threadIdx.x; i < d.VC * 8; i += 256) s_dyn[i] = a.char_emb[i];
  float* E = s_E[wv];
  if (lane < 32) E[128 + lane] = 0.f;  // a window read may run 4 positions past W - 5 + 4
  float acc1[40], acc2[40];
#pragma unroll
  for (int i = 0; i < 40; ++i) acc1[i] = acc2[i] = 0.f;
  float accb1 = 0.f, accb2 = 0.f;
  __syncthreads();
  const int step = gridDim.x * C::NW;
  const int pos = lane >> 3, c = lane & 7;
  const bool has2 = lane + 64 < CW;
  // branch-free loads (see embed_fwd_5x8_mfma)
  const int posA = pos < W ? pos : W - 1, posB = pos + 8 < W ? pos + 8 : W - 1;
  const int lane2 = has2 ? 64 + lane : lane;
  const int wl0 = lane < d.wdim ? lane : d.wdim - 1, wl1 = lane + 64 < d.wdim ? lane + 64 : d.wdim - 1;
  auto load_ids = [&](int tok, int& cA, int& cB, int& wid, int64_t& off) {
    const int t = tok < d.ntok ? tok : d.ntok - 1;
    cA = a.char_ids[(size_t)t * W + posA];
    cB = a.char_ids[(size_t)t * W + posB];
    wid = a.word_ids[t];
    off = a.tok_off[t];
  };
  auto load_grad = [&](int tok, int64_t off, int& ap1, int& ap2, float& g1, float& g2, float& w0, float& w1) {
    const int t = tok < d.ntok ? tok : d.ntok - 1;
    const float* row = a.dx + off;
    ap1 = a.argpos[(size_t)t * CW + lane];
    const int b2 = a.argpos[(size_t)t * CW + lane2];
    g1 = row[lane];
    g2 = row[lane2];
    w0 = row[CW + wl0];
    w1 = row[CW + wl1];
    ap2 = has2 ? b2 : 255;
  };
  int tok = blockIdx.x * C::NW + wv;
  int cA0, cB0, wid0, cA1, cB1, wid1, cA2, cB2, wid2, ap1, ap2, ap1n, ap2n;
  int64_t off0, off1, off2;
  float g1, g2, w0, w1, g1n, g2n, w0n, w1n;
  load_ids(tok, cA0, cB0, wid0, off0);
  load_ids(tok + step, cA1, cB1, wid1, off1);
  load_grad(tok, off0, ap1, ap2, g1, g2, w0, w1);
  for (; tok < d.ntok; tok += step) {
    load_ids(tok + 2 * step, cA2, cB2, wid2, off2);
    load_grad(tok + step, off1, ap1n, ap2n, g1n, g2n, w0n, w1n);
    if (wid0 < d.VW) {
      float* dst = a.d_word_emb + (size_t)wid0 * d.wdim;
      if (lane < d.wdim) atomicAdd(dst + lane, w0);
      if (lane + 64 < d.wdim) atomicAdd(dst + lane + 64, w1);
      for (int i = lane + 128; i < d.wdim; i += 64) atomicAdd(dst + i, a.dx[off0 + CW + i]);
    }
    E[lane] = pos < W ? s_dyn[cA0 * 8 + c] * emb_ks(a, tok, lane, W * 8) : 0.f;
    E[64 + lane] = pos + 8 < W ? s_dyn[cB0 * 8 + c] * emb_ks(a, tok, 64 + lane, W * 8) : 0.f;
    wave_lds_fence();
    {  // d filt[:, :, f] += g_f * window(argpos_f) (40 contiguous values); inactive filters carry g = 0
      if (ap1 == 255) g1 = 0.f;
      if (ap2 == 255) g2 = 0.f;
      const float* e1 = E + (ap1 == 255 ? 0 : ap1) * 8;
      const float* e2 = E + (ap2 == 255 ? 0 : ap2) * 8;
      accb1 += g1;
      accb2 += g2;
#pragma unroll
      for (int i = 0; i < 10; ++i) {
        const f32x4 v1 = *reinterpret_cast<const f32x4*>(e1 + 4 * i);
        const f32x4 v2 = *reinterpret_cast<const f32x4*>(e2 + 4 * i);
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
          acc1[4 * i + cc] += g1 * v1[cc];
          acc2[4 * i + cc] += g2 * v2[cc];
        }
      }
    }
    wave_lds_fence();
    cA0 = cA1; cB0 = cB1; wid0 = wid1; off0 = off1;
    cA1 = cA2; cB1 = cB2; wid1 = wid2; off1 = off2;
    ap1 = ap1n; ap2 = ap2n; g1 = g1n; g2 = g2n; w0 = w0n; w1 = w1n;
  }
  float* slab = a.slab + (size_t)(blockIdx.x * C::NW + wv) * (40 * CW + CW + d.VC * 8);
#pragma unroll
  for (int i = 0; i < 40; ++i) {
    slab[(size_t)i * CW + lane] = acc1[i];
    if (has2) slab[(size_t)i * CW + 64 + lane] = acc2[i];
  }
  slab[40 * CW + lane] = accb1;
  if (has2) slab[40 * CW + 64 + lane] = accb2;
}

// ---- wide char embeddings on the matrix pipe (README.MD:144's --char_emb_size 100) ----------------------------------
// With a 500-deep window the convolution IS a GEMM: rows (token, window position p), k = (kh, c) -- the window of
// position p is the CONTIGUOUS slice E[tok][p*cdim .. p*cdim + height*cdim) of the token's character block -- columns
// the filters.
// The convolution on the FP16 matrix pipe with the 3-term split of the focal attention's logits (attn_fwd.hip): every
// value x = hi + 2^-11 lo' (hi = rtz_f16(x), lo' = f16((x - hi) 2^11)), product = hi hi + 2^-11 (hi lo' + lo' hi): three
// v_mfma_f32_16x16x32_f16 (16 cycles each) per 32 k instead of eight v_mfma_f32_16x16x4_f32 (32 cycles each), <= 3 2^-22
// |E| |filt| per product -- the fp32 kernel's own rounding is 2^-24 per product.  One workgroup = SEVEN waves = the seven
// 16-filter slices: the token's character block is gathered, dropped and split ONCE (the earlier wave-per-(token, slice) form
// re-staged it seven times: 45 KB of L2 reads per token), double-buffered in LDS as two fp16 arrays, and every wave multiplies
// it with its slice's filter fragments (2 x 64 registers, resident for the whole launch).  A[p][kc] = E[p CD + kc]: the
// windows overlap in memory, a lane's 8 consecutive k are 16 contiguous bytes of the block.  8.4 -> 2.6 ms at the
// published flag set's 394 k tokens.  grid (blocks), 448 threads.
template <int CW, int CD>
__global__ __launch_bounds__(64 * ((CW + 15) / 16), 1) void embed_fwdw_f16x3(EmbArgs a) {
  constexpr int KC = 5 * CD, NKS = (KC + 31) / 32;            // k-steps of 32
  constexpr int EB = 15 * CD + 32 * NKS, EBP = (EB + 7) / 8 * 8;  // halves of a staged block (the last window's reach)
  constexpr int NS = (CW + 15) / 16, NT = 64 * NS;            // filter slices = waves, threads
  constexpr int NU = 16 * CD / 4, NL = (NU + NT - 1) / NT;    // 16-byte pieces of a character block, pieces per thread
  static_assert(CD % 4 == 0, "character rows are read 16 bytes at a time");
  __shared__ __attribute__((aligned(16))) _Float16 s_hi[2][EBP], s_lo[2][EBP];
  const fvta_embed_desc& d = a.d;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int j = lane & 15, q = lane >> 4;
  const int W = d.W, P = W - 4;
  // the wave's filter fragments: B[k = 32 ks + 8 q + e][n = j] = filt[k][f] (k >= KC, f >= CW: zero)
  half8 Bh[NKS], Bl[NKS];
  const int f = wv * 16 + j, fc = f < CW ? f : CW - 1;
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    half2v h[4], l[4];
#pragma unroll
    for (int e2 = 0; e2 < 4; ++e2) {
      // (unconditional loads of clamped addresses, then a select: under a branch each of the loads was its own round trip)
      const int k0 = 32 * ks + 8 * q + 2 * e2;
      const float y0 = a.filt[(size_t)(k0 < KC ? k0 : KC - 1) * CW + fc], y1 = a.filt[(size_t)(k0 + 1 < KC ? k0 + 1 : KC - 1) * CW + fc];
      const float x0 = (k0 < KC && f < CW) ? y0 : 0.f, x1 = (k0 + 1 < KC && f < CW) ? y1 : 0.f;
      split_f16x2(x0, x1, h[e2], l[e2]);
    }
    Bh[ks] = cat_h2(h[0], h[1], h[2], h[3]);
    Bl[ks] = cat_h2(l[0], l[1], l[2], l[3]);
  }
  const float bias = a.bias[fc];
  for (int i = tid; i < 2 * EBP; i += NT) {  // (positions >= W and the reach beyond the block stay zero)
    (&s_hi[0][0])[i] = (_Float16)0.f;
    (&s_lo[0][0])[i] = (_Float16)0.f;
  }
  // piece u = tid + NT i: four channels of one character (clamped token and position: branch-free)
  int pos[NL], c4[NL], posc[NL];
  bool stager[NL];
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    const int u = tid + NT * i;
    pos[i] = u / (CD / 4), c4[i] = u % (CD / 4);
    stager[i] = u < NU && pos[i] < W;
    posc[i] = pos[i] < W ? pos[i] : W - 1;
  }
  struct Blk { f32x4 v[NL]; };
  struct Ids { int c[NL]; };
  auto load_id = [&](int tok) {
    const int t = tok < d.ntok ? tok : d.ntok - 1;
    Ids r;
#pragma unroll
    for (int i = 0; i < NL; ++i) r.c[i] = a.char_ids[(size_t)t * W + posc[i]];
    return r;
  };
  auto load_E = [&](const Ids& id) {
    Blk b;
#pragma unroll
    for (int i = 0; i < NL; ++i) b.v[i] = *reinterpret_cast<const f32x4*>(a.char_emb + (size_t)id.c[i] * CD + 4 * (stager[i] ? c4[i] : 0));
    return b;
  };
  // (the dropout mask is applied where the value is consumed: at the load, its wait drained the whole prefetch queue)
  auto store_E = [&](int buf, const Blk& b, int tok) {
    const int t = tok < d.ntok ? tok : d.ntok - 1;
#pragma unroll
    for (int i = 0; i < NL; ++i)
      if (stager[i]) {
        f32x4 v = b.v[i];
        if (a.drop_thr != 0ull)
#pragma unroll
          for (int x = 0; x < 4; ++x) v[x] *= emb_ks(a, t, pos[i] * CD + 4 * c4[i] + x, W * CD);
        half2v h0, l0, h1, l1;
        split_f16x2(v[0], v[1], h0, l0);
        split_f16x2(v[2], v[3], h1, l1);
        *reinterpret_cast<half4v*>(&s_hi[buf][pos[i] * CD + 4 * c4[i]]) = __builtin_shufflevector(h0, h1, 0, 1, 2, 3);
        *reinterpret_cast<half4v*>(&s_lo[buf][pos[i] * CD + 4 * c4[i]]) = __builtin_shufflevector(l0, l1, 0, 1, 2, 3);
      }
  };
  const int step = gridDim.x;
  int tok = blockIdx.x;
  __syncthreads();  // the zero fill
  store_E(0, load_E(load_id(tok)), tok);
  // the gather (character ids, then their rows: two dependent round trips) runs PD tokens ahead of the multiplication,
  // which takes a fraction of one round trip
  constexpr int PD = 4;
  Blk pre[PD];
#pragma unroll
  for (int i = 0; i < PD; ++i) pre[i] = load_E(load_id(tok + (i + 1) * step));
  Ids cid_n = load_id(tok + (PD + 1) * step);  // (the ids one more token ahead of the rows they address)
  // the token's row address and word id travel PD tokens ahead too, the word's row (element tid) one token ahead: left to
  // the token's own iteration, the word copy was two dependent round trips that every wave waited for at the barrier
  // (the index is hidden from the compiler's uniformity analysis: emb_ctok)
  auto ctok = [&](int t) { return emb_ctok(a, t); };
  int64_t off_q[PD + 1];
  int wid_q[PD + 1];
#pragma unroll
  for (int i = 0; i <= PD; ++i) {
    off_q[i] = a.tok_off[ctok(tok + i * step)];
    wid_q[i] = a.word_ids[ctok(tok + i * step)];
  }
  const int wcol = tid < d.wdim ? tid : 0;
  float w_cur = emb_word_src(a, wid_q[0])[wcol];
  __syncthreads();
  for (int it = 0; tok < d.ntok; tok += step, ++it) {
    const int buf = it & 1;
    const Blk e_n = pre[0];
    const int64_t off = off_q[0];
#pragma unroll
    for (int i = 0; i + 1 < PD; ++i) pre[i] = pre[i + 1];
#pragma unroll
    for (int i = 0; i < PD; ++i) off_q[i] = off_q[i + 1], wid_q[i] = wid_q[i + 1];
    pre[PD - 1] = load_E(cid_n);
    cid_n = load_id(tok + (PD + 2) * step);
    off_q[PD] = a.tok_off[ctok(tok + (PD + 1) * step)];
    wid_q[PD] = a.word_ids[ctok(tok + (PD + 1) * step)];
    const float w_nxt = emb_word_src(a, wid_q[0])[wcol];
    f32x4 acc[3];  // (three independent chains: hi hi, hi lo', lo' hi)
    acc[0] = acc[1] = acc[2] = zero4();
    const _Float16* ah = &s_hi[buf][j * CD + 8 * q];  // window position p = j
    const _Float16* al = &s_lo[buf][j * CD + 8 * q];
#pragma unroll
    for (int ks = 0; ks < ((FVTA_EMBW_ABL & 256) ? 0 : NKS); ++ks) {
      // (8-byte aligned: 2 (100 p + 32 ks + 8 q) bytes)
      const half4v h0 = *reinterpret_cast<const half4v*>(ah + 32 * ks), h1 = *reinterpret_cast<const half4v*>(ah + 32 * ks + 4);
      const half4v l0 = *reinterpret_cast<const half4v*>(al + 32 * ks), l1 = *reinterpret_cast<const half4v*>(al + 32 * ks + 4);
      const half8 Ah = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7), Al = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
      // (the last slice's filters past CW multiply zeros: a wave-uniform skip here would cut the unrolled loop into blocks)
      acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ah, Bh[ks], acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ah, Bl[ks], acc[1], 0, 0, 0);
      acc[2] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Al, Bh[ks], acc[2], 0, 0, 0);
    }
    float* row = a.x + off;
    // D[p = 4 q + r][f = j]: max / FIRST arg-max over the valid positions
    float best = -INFINITY;
    int bp = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v = acc[0][r] + (acc[1][r] + acc[2][r]) * (1.f / 2048.f);
      const int p = 4 * q + r;
      if (p < P && v > best) {
        best = v;
        bp = p;
      }
    }
#pragma unroll
    for (int sh = 16; sh <= 32; sh <<= 1) {
      const float ob = __shfl_xor(best, sh, 64);
      const int op = __shfl_xor(bp, sh, 64);
      if (ob > best || (ob == best && op < bp)) {
        best = ob;
        bp = op;
      }
    }
    if (q == 0 && f < CW) {
      const float y = best + bias;
      row[f] = y > 0.f ? y : 0.f;
      a.argpos[(size_t)tok * CW + f] = y > 0.f ? (uint8_t)bp : (uint8_t)255;
    }
    if (tid < d.wdim) row[CW + tid] = w_cur;  // the word part of the row (wdim <= threads: the launcher's condition -- a copy
                                              // loop here made the compiler drain every prefetch at the end of each token)
    w_cur = w_nxt;
    if constexpr (!(FVTA_EMBW_ABL & 512)) store_E(buf ^ 1, e_n, tok + step);  // (that buffer's readers finished before the barrier that ended the previous token)
    if constexpr (!(FVTA_EMBW_ABL & 1024)) __syncthreads();
  }
}
template __global__ void embed_fwdw_f16x3<100, 100>(EmbArgs);

// d filt / d bias of the wide shape, a WORKGROUP per token (round 4's form ran a wave per (token, slice): seven
// waves somewhere on the chip each gather the token's gradient row, arg-max positions and their 16 channels of its characters --
// 1.7 of its 6.1 ms -- and its four waves per workgroup work on four different tokens).  Here the seven waves of a workgroup ARE
// the seven 16-channel slices of ONE token: the character block (16 positions x cdim, dropped as in the forward), the gradient
// row and the arg-max positions are gathered once, two to four tokens ahead in registers (embed_fwdw_f16x3's queue), and
// double-buffered in LDS; wave v multiplies ITS slice -- dFilt[l = k 16 + c][f] += sum_p E[p + k][16 v + c] G[p][f], the same
// 5 x 7 x 3 v_mfma_f32_16x16x4_f32 per token as before, exact -- and keeps its 80 x 112 accumulator tile for the whole launch;
// no reduction across waves at the end (a slice belongs to one wave).  grid (blocks <= 256), 448 threads, slab part
// [0, KC cw + cw) of block x.
// The product runs on the bf16 matrix pipe with a three-term split -- x = hi + lo, both bf16 (fp32's exponent range: the low
// terms need no scaling), hi hi + hi lo + lo hi into ONE accumulator, ~2^-16 per product (the arg-max positions are inputs
// here: nothing can flip) -- one k-step of v_mfma_f32_16x16x16_bf16 over the 16 window positions instead of three of
// v_mfma_f32_16x16x4_f32: 105 x 16 matrix-pipe cycles per token and slice instead of 105 x 32.  The character block and the
// gradient row are split ONCE, by the threads that stage them, and kept in LDS as packed (hi | lo << 16) words.
template <int CW, int CD>
__global__ __launch_bounds__(448, 1) void embed_bwdw_filt_tok(EmbArgs a) {
  constexpr int CS = 16, NMT = 5, NNT = (CW + 15) / 16, NS = (CD + CS - 1) / CS;
  typedef short bf4 __attribute__((ext_vector_type(4)));
  typedef unsigned u2 __attribute__((ext_vector_type(2)));
  auto pack_hl = [](float x) {  // bf16(x) | bf16(x - bf16(x)) << 16, both rounded to nearest
    const unsigned h = f2bf(x);
    return h | ((unsigned)f2bf(x - bf2f((unsigned short)h)) << 16);
  };
  static_assert(NS == 7 && CD % 4 == 0, "seven slices of 16 channels");
  constexpr int NU = 16 * CD / 4;                       // 16-byte pieces of a character block
  __shared__ __attribute__((aligned(16))) float s_E[2][20 * CD];  // (positions 16 .. 19 stay zero: the reach of window position 15)
  __shared__ float s_g[2][16 * NNT];
  __shared__ unsigned s_gx[2][16 * NNT];  // (the gradient row as packed hi | lo)
  __shared__ int s_ap[2][16 * NNT];
  const fvta_embed_desc& d = a.d;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int j = lane & 15, q = lane >> 4;
  const int W = d.W;
  const int c0 = wv * CS, nc = min(CS, CD - c0);
  f32x4 acc[NMT][NNT];
#pragma unroll
  for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NNT; ++nt) acc[mt][nt] = zero4();
  float accb[NNT];
#pragma unroll
  for (int nt = 0; nt < NNT; ++nt) accb[nt] = 0.f;
  for (int i = tid; i < 2 * 20 * CD; i += 448) (&s_E[0][0])[i] = 0.f;
  for (int i = tid; i < 2 * 16 * NNT; i += 448) {
    (&s_g[0][0])[i] = 0.f;
    (&s_ap[0][0])[i] = 255;
    (&s_gx[0][0])[i] = 0u;
  }
  // A operand: lane (row l = 16 mt + j = tap mt, channel j; k phase q) reads E[(4 ks + q) + mt][c0 + j]; channels beyond the
  // slice multiply by zero
  const bool a_ok = j < nc;
  const int a0 = 4 * q * CD + c0 + (a_ok ? j : 0);  // (the lane's four window positions 4 q .. 4 q + 3)
  // staging: thread u < NU gathers four channels of one character; thread u < CW one gradient value and its arg-max position
  const int pos = tid / (CD / 4), c4 = tid % (CD / 4);
  const bool stager = tid < NU && pos < W;
  const int posc = pos < W ? pos : W - 1;
  const int fcol = tid < CW ? tid : CW - 1;
  auto ctok = [&](int t) { return emb_ctok(a, t); };
  auto load_id = [&](int tok) { return a.char_ids[(size_t)ctok(tok) * W + posc]; };
  auto load_E = [&](int cid) {
    f32x4 v = zero4();
    if (stager) v = *reinterpret_cast<const f32x4*>(a.char_emb + (size_t)cid * CD + 4 * c4);
    return v;
  };
  auto load_off = [&](int tok) { return a.tok_off[ctok(tok)]; };
  auto load_ap = [&](int tok) { return (int)a.argpos[(size_t)ctok(tok) * CW + fcol]; };
  auto store_tok = [&](int buf, f32x4 v, float g, int ap, int tok) {
    if (stager) {
      if (a.drop_thr != 0ull) {
        const int t = tok < d.ntok ? tok : d.ntok - 1;
#pragma unroll
        for (int x = 0; x < 4; ++x) v[x] *= emb_ks(a, t, pos * CD + 4 * c4 + x, W * CD);
      }
#pragma unroll
      for (int x = 0; x < 4; ++x) v[x] = __uint_as_float(pack_hl(v[x]));
      *reinterpret_cast<f32x4*>(&s_E[buf][pos * CD + 4 * c4]) = v;
    }
    if (tid < CW) {
      const float gm = ap == 255 ? 0.f : g;
      s_g[buf][tid] = gm;
      s_ap[buf][tid] = ap;
      s_gx[buf][tid] = pack_hl(gm);
    }
  };
  const int step = gridDim.x;
  int tok = blockIdx.x;
  constexpr int PD = 3;
  f32x4 e_q[PD + 1];
  int64_t off_q[PD + 2];
  int ap_q[PD + 1];
  float g_q[PD + 1];
  int wid_q[PD + 1];
#pragma unroll
  for (int i = 0; i <= PD + 1; ++i) off_q[i] = load_off(tok + i * step);
#pragma unroll
  for (int i = 0; i <= PD; ++i) {
    e_q[i] = load_E(load_id(tok + i * step));
    ap_q[i] = load_ap(tok + i * step);
    g_q[i] = a.dx[off_q[i] + fcol];
    wid_q[i] = a.word_ids[ctok(tok + i * step)];
  }
  int cid_n = load_id(tok + (PD + 1) * step);
  // the word part of the gradient row (elements lane and 64 + lane: wdim <= 128, the launcher's condition) one token ahead --
  // a copy loop with loads inside the token loop makes the compiler drain every prefetch at the loop's end
  const int wc0 = lane < d.wdim ? lane : 0, wc1 = 64 + lane < d.wdim ? 64 + lane : 0;
  float w0 = a.dx[off_q[0] + CW + wc0], w1 = a.dx[off_q[0] + CW + wc1];
  __syncthreads();  // the zero fill
  store_tok(0, e_q[0], g_q[0], ap_q[0], tok);
  __syncthreads();
  for (int it = 0; tok < d.ntok; tok += step, ++it) {
    const int buf = it & 1;
    const int wid = wid_q[0];
    const float w0n = a.dx[off_q[1] + CW + wc0], w1n = a.dx[off_q[1] + CW + wc1];
    // the queues move up one token; the new tail entries are requested now
#pragma unroll
    for (int i = 0; i < PD; ++i) e_q[i] = e_q[i + 1], ap_q[i] = ap_q[i + 1], g_q[i] = g_q[i + 1], wid_q[i] = wid_q[i + 1];
#pragma unroll
    for (int i = 0; i <= PD; ++i) off_q[i] = off_q[i + 1];
    e_q[PD] = load_E(cid_n);
    cid_n = load_id(tok + (PD + 2) * step);
    ap_q[PD] = load_ap(tok + (PD + 1) * step);
    g_q[PD] = a.dx[off_q[PD] + fcol];          // (its row address was requested a token ago)
    off_q[PD + 1] = load_off(tok + (PD + 2) * step);
    wid_q[PD] = a.word_ids[ctok(tok + (PD + 1) * step)];
    // the wave's one-hot operand: filter f = 16 nt + j
    float g_c[NNT];
    int ap_c[NNT];
#pragma unroll
    for (int nt = 0; nt < NNT; ++nt) {
      g_c[nt] = s_g[buf][16 * nt + j];
      ap_c[nt] = s_ap[buf][16 * nt + j];
    }
    if (wv == 0 && q == 0)
#pragma unroll
      for (int nt = 0; nt < NNT; ++nt) accb[nt] += g_c[nt];
    if (wv == NS - 1 && wid < d.VW) {  // the word rows ride along with the lightest slice
      if (lane < d.wdim) atomicAdd(a.d_word_emb + (size_t)wid * d.wdim + lane, w0);
      if (64 + lane < d.wdim) atomicAdd(a.d_word_emb + (size_t)wid * d.wdim + 64 + lane, w1);
    }
    w0 = w0n, w1 = w1n;
    const float* Es = s_E[buf];
    {
      bf4 Bh[NNT], Bl[NNT];
#pragma unroll
      for (int nt = 0; nt < NNT; ++nt) {
        const unsigned gx = s_gx[buf][16 * nt + j], gh = gx & 0xffffu, gl = gx >> 16;
        const int e = ap_c[nt] - 4 * q;  // the filter's arg-max position inside this lane's four (else: no contribution)
        Bh[nt] = __builtin_bit_cast(bf4, u2{e == 0 ? gh : (e == 1 ? gh << 16 : 0u), e == 2 ? gh : (e == 3 ? gh << 16 : 0u)});
        Bl[nt] = __builtin_bit_cast(bf4, u2{e == 0 ? gl : (e == 1 ? gl << 16 : 0u), e == 2 ? gl : (e == 3 ? gl << 16 : 0u)});
      }
#pragma unroll
      for (int mt = 0; mt < NMT; ++mt) {
        unsigned u[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const unsigned w = __float_as_uint(Es[a0 + (e + mt) * CD]);
          u[e] = a_ok ? w : 0u;
        }
        const bf4 Ah = __builtin_bit_cast(bf4, u2{(u[0] & 0xffffu) | (u[1] << 16), (u[2] & 0xffffu) | (u[3] << 16)});
        const bf4 Al = __builtin_bit_cast(bf4, u2{(u[0] >> 16) | (u[1] & 0xffff0000u), (u[2] >> 16) | (u[3] & 0xffff0000u)});
#pragma unroll
        for (int nt = 0; nt < NNT; ++nt) {
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(Ah, Bh[nt], acc[mt][nt], 0, 0, 0);
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(Ah, Bl[nt], acc[mt][nt], 0, 0, 0);
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(Al, Bh[nt], acc[mt][nt], 0, 0, 0);
        }
      }
    }
    store_tok(buf ^ 1, e_q[0], g_q[0], ap_q[0], tok + step);  // (that buffer's readers finished before the last barrier)
    __syncthreads();
  }
  // ---- the slab: tile (mt, nt), lane (j, q), element r: row l = 16 mt + 4 q + r = (tap mt, channel 4 q + r), filter f = 16 nt + j
  const int KC = 5 * CD;
  float* slab = a.slab + (size_t)blockIdx.x * ((size_t)KC * CW + CW + (size_t)d.VC * CD);
#pragma unroll
  for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NNT; ++nt) {
      const int f = 16 * nt + j;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = 4 * q + r;
        if (c < nc && f < CW) slab[(size_t)(mt * CD + c0 + c) * CW + f] = acc[mt][nt][r];
      }
    }
  if (wv == 0 && q == 0)
#pragma unroll
    for (int nt = 0; nt < NNT; ++nt)
      if (16 * nt + j < CW) slab[(size_t)KC * CW + 16 * nt + j] = accb[nt];
}
template __global__ void embed_bwdw_filt_tok<100, 100>(EmbArgs);

// d char_emb of the wide shape, a WORKGROUP per token, with NO transposed tile, NO 5-tap fold and NO LDS float adds (those three
// were 3.7 of the wave-per-(token, slice) form's 6.2 ms: -DFVTA_EMBW_ABL).  Two matrix products per token and 16-channel slice (wave):
//  (1) dE[pos][c] = sum over (k, f) of Gs[pos][(k, f)] filt[k][c][f] with the SHIFTED one-hot Gs[pos][(k, f)] = g_f [argpos_f + k = pos]:
//      the fold over the five taps is part of the contraction (K = 5 x 104: 17 k-steps of v_mfma_f32_16x16x32_f16 x 3, the fp16
//      3-term split of embed_fwdw_f16x3; the slice's filter fragments in 136 registers for the launch).  Gs is the same for
//      all seven slices: its fragments are built ONCE per token, k-steps dealt over the waves, and shared through LDS;
//  (2) dChar[v][c] += sum_pos [ch[pos] = v] dE[pos][c]: the scatter into the character table as a product with the exact
//      one-hot of the token's characters -- v_mfma_f32_16x16x16_f16, dE split (hi, lo') into two accumulators -- whose B operand
//      is product (1)'s accumulator AS IT LIES (lane (c, q) holds positions 4 q .. 4 q + 3 in both layouts); the table slice
//      [VC <= 128][16] stays in registers for the whole launch.
// grid (blocks), 448 threads; slab part [KC cw + cw ..) of block x.
template <int CW, int CD>
__global__ __launch_bounds__(448, 1) void embed_bwdw_char_tok(EmbArgs a) {
  constexpr int CS = 16, NS = (CD + CS - 1) / CS, FP = (CW + 7) / 8 * 8, KT = 5 * FP, NKS = (KT + 31) / 32, NVT = 8;
  static_assert(NS == 7 && FP == 104 && NKS == 17, "seven slices of 16 channels, filters padded to 104 per tap");
  typedef _Float16 half4v_ __attribute__((ext_vector_type(4)));
  extern __shared__ __attribute__((aligned(16))) char s_dyn_ct[];     // 2 x NKS x 2 x 64 x 16 bytes (68 KB: dynamic)
  half8(*s_A)[NKS][2][64] = reinterpret_cast<half8(*)[NKS][2][64]>(s_dyn_ct);  // the shifted one-hot's fragments (hi, lo') of a token
  // the last NBL low filter fragments of every wave live in LDS (read like the A fragments): with all 34 in registers the
  // compiler spilled six of them to scratch and re-loaded them in the k loop behind s_waitcnt vmcnt(0)
  constexpr int NBL = 7;
  half8(*s_Bl)[NBL][64] = reinterpret_cast<half8(*)[NBL][64]>(s_dyn_ct + (size_t)2 * NKS * 2 * 64 * 16);  // [wave][NBL][64]
  __shared__ __attribute__((aligned(16))) float s_g[2][FP + 8];
  __shared__ __attribute__((aligned(16))) uint8_t s_ap[2][FP + 8];
  __shared__ __attribute__((aligned(16))) int s_ch[3][16];
  const fvta_embed_desc& d = a.d;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int j = lane & 15, q = lane >> 4;
  const int W = d.W;
  const int c0 = wv * CS, nc = min(CS, CD - c0);
  // the slice's filter fragments: B[kappa = 32 ks + 8 q + e][n = j] = filt[k][c0 + j][f], (k, f) = (kappa / 104, kappa % 104)
  half8 Bh[NKS], Bl[NKS - NBL];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const int kap = 32 * ks + 8 * q, k = kap / FP, f0 = kap % FP;
    const bool ok = k < 5 && j < nc;
    const float* src = a.filt + (size_t)((ok ? k : 0) * CD + c0 + (j < nc ? j : 0)) * CW;
    half2v h[4], l[4];
#pragma unroll
    for (int e2 = 0; e2 < 4; ++e2) {
      const int fa = f0 + 2 * e2, fb = fa + 1;
      const float ya = src[fa < CW ? fa : CW - 1], yb = src[fb < CW ? fb : CW - 1];   // unconditional, then a select
      split_f16x2((ok && fa < CW) ? ya : 0.f, (ok && fb < CW) ? yb : 0.f, h[e2], l[e2]);
    }
    Bh[ks] = cat_h2(h[0], h[1], h[2], h[3]);
    if (ks < NKS - NBL) Bl[ks] = cat_h2(l[0], l[1], l[2], l[3]);
    else s_Bl[wv][ks - (NKS - NBL)][lane] = cat_h2(l[0], l[1], l[2], l[3]);
  }
  f32x4 tab[NVT];
#pragma unroll
  for (int mt = 0; mt < NVT; ++mt) tab[mt] = zero4();
  for (int i = tid; i < 2 * (FP + 8); i += 448) {
    (&s_g[0][0])[i] = 0.f;
    (&s_ap[0][0])[i] = 255;
  }
  auto ctok = [&](int t) { return emb_ctok(a, t); };
  const int fcol = tid < CW ? tid : CW - 1, pcol = tid < W ? tid : W - 1;
  // stage token `tok`'s gradient row, arg-max positions and characters (values already in registers)
  auto stage = [&](int tokidx, float g, int ap, int ch) {
    if (tid < CW) {
      s_g[tokidx & 1][tid] = ap == 255 ? 0.f : g;
      s_ap[tokidx & 1][tid] = (uint8_t)ap;
    }
    if (tid < 16) s_ch[tokidx % 3][tid] = tid < W ? ch : -1;
  };
  // build the fragments of the shifted one-hot of token `tokidx` (its g / ap staged before the last barrier): k-step ks by wave ks % 7
  auto build = [&](int tokidx) {
    const int b = tokidx & 1;
#pragma unroll
    for (int i = 0; i < (NKS + NS - 1) / NS; ++i) {
      const int ks = wv + NS * i;
      if (ks < NKS) {
        const int kap = 32 * ks + 8 * q, k = kap / FP, f0 = kap % FP;   // (k = 5: the padding beyond 520 -- nothing matches)
        const f32x4 G0 = *reinterpret_cast<const f32x4*>(&s_g[b][f0]), G1 = *reinterpret_cast<const f32x4*>(&s_g[b][f0 + 4]);
        const uint2 Pw = *reinterpret_cast<const uint2*>(&s_ap[b][f0]);
        half2v h[4], l[4];
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2) {
          const unsigned pw = e2 < 2 ? Pw.x : Pw.y;
          const int pa = (int)((pw >> (16 * (e2 & 1))) & 255u), pb = (int)((pw >> (16 * (e2 & 1) + 8)) & 255u);
          const float ga = e2 < 2 ? G0[2 * e2] : G1[2 * e2 - 4], gb = e2 < 2 ? G0[2 * e2 + 1] : G1[2 * e2 - 3];
          split_f16x2((k < 5 && pa + k == j) ? ga : 0.f, (k < 5 && pb + k == j) ? gb : 0.f, h[e2], l[e2]);
        }
        s_A[b][ks][0][lane] = cat_h2(h[0], h[1], h[2], h[3]);
        s_A[b][ks][1][lane] = cat_h2(l[0], l[1], l[2], l[3]);
      }
    }
  };
  const int step = gridDim.x;
  int tok = blockIdx.x;
  // prefetch queue: entry i = token tok + (2 + i) step (tokens tok and tok + step are staged in the prologue)
  constexpr int PD = 2;
  auto fetch = [&](int t, int64_t off, float& g, int& ap, int& ch) {
    g = a.dx[off + fcol];
    ap = a.argpos[(size_t)ctok(t) * CW + fcol];
    ch = a.char_ids[(size_t)ctok(t) * W + pcol];
  };
  float g_q[PD];
  int ap_q[PD], ch_q[PD];
  int64_t off_q[PD + 1];
  {
    float g0, g1;
    int ap0, ap1, ch0, ch1;
    fetch(tok, a.tok_off[ctok(tok)], g0, ap0, ch0);
    fetch(tok + step, a.tok_off[ctok(tok + step)], g1, ap1, ch1);
#pragma unroll
    for (int i = 0; i < PD; ++i) fetch(tok + (2 + i) * step, a.tok_off[ctok(tok + (2 + i) * step)], g_q[i], ap_q[i], ch_q[i]);
    off_q[PD] = a.tok_off[ctok(tok + (2 + PD) * step)];
    __syncthreads();  // the fills
    stage(0, g0, ap0, ch0);
    stage(1, g1, ap1, ch1);
    __syncthreads();
    build(0);
    __syncthreads();
  }
  for (int it = 0; tok < d.ntok; tok += step, ++it) {
    const int buf = it & 1;
    // the queue moves up: its head is token it + 2, staged at the end of this iteration
    const float g_s = g_q[0];
    const int ap_s = ap_q[0], ch_s = ch_q[0];
#pragma unroll
    for (int i = 0; i + 1 < PD; ++i) g_q[i] = g_q[i + 1], ap_q[i] = ap_q[i + 1], ch_q[i] = ch_q[i + 1];
    fetch(tok + (2 + PD) * step, off_q[PD], g_q[PD - 1], ap_q[PD - 1], ch_q[PD - 1]);   // (its row address: requested a token ago)
    off_q[PD] = a.tok_off[ctok(tok + (3 + PD) * step)];
    // ---- (1) dE[pos = 4 q + r][c = j]
    f32x4 aT = {0.f, 0.f, 0.f, 0.f}, aX = {0.f, 0.f, 0.f, 0.f}, aY = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      const half8 Ah = s_A[buf][ks][0][lane], Al = s_A[buf][ks][1][lane];
      aT = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ah, Bh[ks], aT, 0, 0, 0);
      half8 bl;
      if (ks < NKS - NBL) bl = Bl[ks < NKS - NBL ? ks : 0];
      else bl = s_Bl[wv][ks >= NKS - NBL ? ks - (NKS - NBL) : 0][lane];
      aX = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ah, bl, aX, 0, 0, 0);
      aY = __builtin_amdgcn_mfma_f32_16x16x32_f16(Al, Bh[ks], aY, 0, 0, 0);
      if (ks & 1) __builtin_amdgcn_sched_barrier(0);  // (the scheduler would hoist all 34 fragment reads: 136 registers, spills)
    }
    f32x4 dE = aT + (aX + aY) * (1.f / 2048.f);
    if (a.drop_thr != 0ull)
#pragma unroll
      for (int r = 0; r < 4; ++r) dE[r] *= emb_ks(a, tok, (4 * q + r) * CD + c0 + (j < nc ? j : 0), W * CD);
    // ---- (2) the scatter: table[v][c] += sum_pos [ch[pos] = v] dE[pos][c]
    half2v h0, l0, h1, l1;
    split_f16x2(dE[0], dE[1], h0, l0);
    split_f16x2(dE[2], dE[3], h1, l1);
    const half4v_ Eh = __builtin_shufflevector(h0, h1, 0, 1, 2, 3), El = __builtin_shufflevector(l0, l1, 0, 1, 2, 3);
    const int4 chq = *reinterpret_cast<const int4*>(&s_ch[it % 3][4 * q]);   // the characters at positions 4 q .. 4 q + 3
#pragma unroll
    for (int mt = 0; mt < NVT; ++mt) {
      const int v = 16 * mt + j;
      const half4v_ oh = {(_Float16)(chq.x == v ? 1.f : 0.f), (_Float16)(chq.y == v ? 1.f : 0.f), (_Float16)(chq.z == v ? 1.f : 0.f),
                          (_Float16)(chq.w == v ? 1.f : 0.f)};
      // (the low half through a temporary: a second table of 32 registers spilled the filter fragments)
      const f32x4 lo = __builtin_amdgcn_mfma_f32_16x16x16f16(oh, El, zero4(), 0, 0, 0);
      tab[mt] = __builtin_amdgcn_mfma_f32_16x16x16f16(oh, Eh, tab[mt], 0, 0, 0);
      tab[mt] += lo * (1.f / 2048.f);
    }
    // ---- the next tokens: fragments of token it + 1 (staged before the last barrier), staging of token it + 2
    build(it + 1);
    stage(it + 2, g_s, ap_s, ch_s);
    __syncthreads();
  }
  // ---- the slab: table tile mt, lane (c = j, q), element r: character v = 16 mt + 4 q + r
  const EmbSlab sl(5 * CD, CW, d.VC, CD);
  float* slab_c = emb_slab(a, sl, blockIdx.x) + sl.chars;
#pragma unroll
  for (int mt = 0; mt < NVT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int v = 16 * mt + 4 * q + r;
      if (v < d.VC && j < nc) slab_c[(size_t)v * CD + c0 + j] = tab[mt][r];
    }
}
template __global__ void embed_bwdw_char_tok<100, 100>(EmbArgs);

// slabs -> d_filt, d_bias, d_char_emb (accumulate), fixed order over slabs
// 1024 threads = 64 elements x 16 slab groups (group g sums slabs g, g+16, ...; the partials combine pairwise in order)
constexpr int EMB_RED_G = 16;
__global__ __launch_bounds__(64 * EMB_RED_G) void embed_bwd_reduce_kernel(const float* __restrict__ slab, int nblk, int nfb,
                                                                         int nchar, float* __restrict__ d_filt,
                                                                         float* __restrict__ d_bias, int nfilt,
                                                                         float* __restrict__ d_char) {
  __shared__ float s_part[EMB_RED_G][64];
  const int el = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + el, per = nfb + nchar;
  float part = 0.f;
  if (i < per)
    for (int b = grp; b < nblk; b += EMB_RED_G) part += slab[(size_t)b * per + i];
  s_part[grp][el] = part;
  __syncthreads();
  for (int w = EMB_RED_G / 2; w >= 1; w >>= 1) {
    if (grp < w) s_part[grp][el] += s_part[grp + w][el];
    __syncthreads();
  }
  if (grp != 0 || i >= per) return;
  const float v = s_part[0][el];
  if (i < nfilt) d_filt[i] += v;
  else if (i < nfb) d_bias[i - nfilt] += v;
  else d_char[i - nfb] += v;
}


template __global__ void embed_fwd_5x8_mfma<100>(EmbArgs);
template __global__ void embed_bwd_5x8_char<100>(EmbArgs);
template __global__ void embed_bwd_5x8_filt<100>(EmbArgs);
}  // namespace fvta
using namespace fvta;

static int check_embed(const fvta_embed_desc* d) {
  FVTA_CHECK_ARG(d && d->ntok > 0 && d->wdim > 0 && d->VW >= 0 && d->VT >= d->VW, "embed: bad descriptor");
  if (d->cwdim > 0) {
    FVTA_CHECK_ARG(d->cwdim <= EMB_NT && d->W >= d->height && d->W <= 64 && d->height > 0 && d->cdim > 0 &&
                       d->cdim <= EMB_NT && d->W * d->cdim <= EMB_BIG_WC && d->VC > 0 && d->VC <= EMB_MAXVC,
                   "embed: unsupported char-CNN shape (cwdim<=128, cdim<=128, height<=W<=64, W*cdim<=8192, VC<=1024)");
  }
  return FVTA_OK;
}

static bool embed_is_big(const fvta_embed_desc* d) {
  return d->cwdim > 0 && (d->height * d->cdim > EMB_MAXKC || d->W * d->cdim > EMB_MAXWC);
}
constexpr int EMB_BIG_BLOCKS = 256;
// the published flag set's char-CNN (README.MD:144: --char_emb_size 100, 100 filters of height 5): the matrix-pipe kernels
// embed_fwdw_f16x3 / embed_bwdw_filt_tok / embed_bwdw_char_tok.  Every other deep window runs the general kernels
// embed_fwd_general<true> / embed_bwd_general<true> (FVTA_EMBED_MFMA=0 sends the published shape there too: the A/B of the tests).
static bool embed_wide_ok(const fvta_embed_desc* d) {
  static const bool off = [] {
    const char* e = getenv("FVTA_EMBED_MFMA");
    return e && e[0] == '0';
  }();
  return !off && d->cwdim == 100 && d->cdim == 100 && d->height == 5 && d->W >= 5 && d->W <= 16 && d->wdim <= 128 &&
         d->VC <= 128;
}

// the reference's default shape (height 5, char_emb 8, 100 filters): wave-per-token kernels on the matrix pipe
constexpr int EMB_WAVE_FWD_BLOCKS = 768;
static bool embed_wave_ok(const fvta_embed_desc* d) {
  return d->cwdim == 100 && d->height == 5 && d->cdim == 8 && d->W <= 16 && d->VC <= 256;
}

extern "C" size_t fvta_embed_workspace_bytes(const fvta_embed_desc* d) {
  if (check_embed(d)) return 0;
  const size_t b = (size_t)(embed_is_big(d) ? EMB_BIG_BLOCKS : EMB_BWD_BLOCKS) * EmbSlab(*d).floats * sizeof(float);
  return b < 256 ? 256 : b;
}

extern "C" int fvta_embed_fwd(const fvta_embed_desc* d, const int32_t* word_ids, const int32_t* char_ids,
                              const int64_t* tok_off, const float* word_emb, const float* fixed_emb,
                              const float* char_emb, const float* filt, const float* bias, float* x,
                              uint8_t* argpos, fvta_stream_t stream_) {
  if (int e = check_embed(d)) return e;
  FVTA_CHECK_ARG(word_ids && tok_off && x, "embed_fwd: null pointer");
  FVTA_CHECK_ARG(d->VW == 0 || word_emb, "embed_fwd: word_emb required");
  FVTA_CHECK_ARG(d->VT == d->VW || fixed_emb, "embed_fwd: fixed_emb required");
  FVTA_CHECK_ARG(d->cwdim == 0 || (char_ids && char_emb && filt && bias && argpos), "embed_fwd: char-CNN pointers");
  EmbArgs a = emb_args(d, word_ids, char_ids, tok_off, char_emb, filt, argpos);
  a.word_emb = word_emb; a.fixed_emb = fixed_emb; a.bias = bias; a.x = x;
  const int blocks = d->ntok < 8192 ? d->ntok : 8192;
  if (embed_wide_ok(d)) {
    // the published --char_emb_size 100 on the fp16 matrix pipe (3-term split): a workgroup per token, its waves the filter
    // slices; one workgroup per CU (its filter fragments are loaded once)
    const int nbt = d->ntok < 256 ? d->ntok : 256;
    hipLaunchKernelGGL((embed_fwdw_f16x3<100, 100>), dim3(nbt), dim3(448), 0, (hipStream_t)stream_, a);
  } else if (embed_is_big(d)) {     // every other deep window: the general kernel
    const size_t dyn = (size_t)d->W * d->cdim * sizeof(float);
    hipLaunchKernelGGL(embed_fwd_general<true>, dim3(blocks), dim3(EMB_NT), dyn, (hipStream_t)stream_, a);
  } else if (embed_wave_ok(d)) {
    const int nb = (d->ntok + 3) / 4 < EMB_WAVE_FWD_BLOCKS ? (d->ntok + 3) / 4 : EMB_WAVE_FWD_BLOCKS;
    hipLaunchKernelGGL(embed_fwd_5x8_mfma<100>, dim3(nb), dim3(256), (size_t)d->VC * 8 * sizeof(float), (hipStream_t)stream_, a);
  } else
    hipLaunchKernelGGL(embed_fwd_general<false>, dim3(blocks), dim3(EMB_NT), 0, (hipStream_t)stream_, a);
  FVTA_CHECK_LAUNCH("embed_fwd");
  return FVTA_OK;
}

extern "C" int fvta_embed_bwd(const fvta_embed_desc* d, const int32_t* word_ids, const int32_t* char_ids,
                              const int64_t* tok_off, const float* char_emb, const float* filt,
                              const uint8_t* argpos, const float* dx, float* d_word_emb, float* d_char_emb,
                              float* d_filt, float* d_bias, void* workspace, fvta_stream_t stream_) {
  if (int e = check_embed(d)) return e;
  FVTA_CHECK_ARG(word_ids && tok_off && dx && workspace, "embed_bwd: null pointer");
  FVTA_CHECK_ARG(d->VW == 0 || d_word_emb, "embed_bwd: d_word_emb required");
  FVTA_CHECK_ARG(d->cwdim == 0 || (char_ids && char_emb && filt && argpos && d_char_emb && d_filt && d_bias),
                 "embed_bwd: char-CNN pointers");
  hipStream_t stream = (hipStream_t)stream_;
  EmbArgs a = emb_args(d, word_ids, char_ids, tok_off, char_emb, filt, argpos);
  a.dx = dx; a.d_word_emb = d_word_emb; a.slab = (float*)workspace;
  int blocks;
  if (embed_wide_ok(d)) {
    // the published shape: a workgroup per token for both gradients (d filt / d bias: the bf16 three-term product; d char_emb:
    // the tap fold and the table scatter as two chained matrix products); slabs reduced in a fixed order below
    blocks = d->ntok < EMB_BIG_BLOCKS ? d->ntok : EMB_BIG_BLOCKS;
    hipLaunchKernelGGL((embed_bwdw_filt_tok<100, 100>), dim3(blocks), dim3(448), 0, stream, a);
    constexpr int frag_bytes = 2 * 17 * 2 * 64 * 16 + 7 * 7 * 64 * 16;  // the A fragments (two tokens) + the waves' low filter fragments
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(embed_bwdw_char_tok<100, 100>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              frag_bytes);
    hipLaunchKernelGGL((embed_bwdw_char_tok<100, 100>), dim3(blocks), dim3(448), frag_bytes, stream, a);
  } else if (embed_is_big(d)) {
    blocks = d->ntok < EMB_BIG_BLOCKS ? d->ntok : EMB_BIG_BLOCKS;
    FVTA_CHECK_HIP(hipMemsetAsync(workspace, 0, (size_t)blocks * EmbSlab(*d).floats * sizeof(float), stream));
    const size_t dyn = (size_t)2 * d->W * d->cdim * sizeof(float);
    if (dyn > 32 * 1024)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(embed_bwd_general<true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
    hipLaunchKernelGGL(embed_bwd_general<true>, dim3(blocks), dim3(EMB_NT), dyn, stream, a);
  } else if (embed_wave_ok(d)) {
    // one slab per WAVE: 4 * blocks <= EMB_BWD_BLOCKS slabs
    blocks = (d->ntok + 3) / 4 < EMB_BWD_BLOCKS / 4 ? (d->ntok + 3) / 4 : EMB_BWD_BLOCKS / 4;
    const size_t tab = (size_t)d->VC * 8 * sizeof(float);
    hipLaunchKernelGGL(embed_bwd_5x8_filt<100>, dim3(blocks), dim3(256), tab, stream, a);
    hipLaunchKernelGGL(embed_bwd_5x8_char<100>, dim3(blocks), dim3(256), 4 * tab, stream, a);
    blocks *= 4;
  } else {
    const size_t dyn = ((size_t)d->height * d->cdim * d->cwdim + (size_t)d->VC * d->cdim) * sizeof(float);
    // one dispatch round: as many workgroups as fit the 256 CUs at once (LDS bound; ~9 KB static), never more than the
    // slab workspace holds -- a second, partly filled round would run at the speed of the first
    int per_cu = (int)((160 * 1024) / (dyn + 9 * 1024));
    if (per_cu > 8) per_cu = 8;
    if (per_cu < 1) per_cu = 1;
    blocks = 256 * per_cu;
    if (blocks > EMB_BWD_BLOCKS) blocks = EMB_BWD_BLOCKS;
    if (blocks > d->ntok) blocks = d->ntok;
    if (dyn > 32 * 1024)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(embed_bwd_general<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)dyn);
    hipLaunchKernelGGL(embed_bwd_general<false>, dim3(blocks), dim3(EMB_NT), dyn, stream, a);
  }
  if (d->cwdim > 0) {
    const int nfilt = d->height * d->cdim * d->cwdim, nfb = nfilt + d->cwdim, nchar = d->VC * d->cdim;
    hipLaunchKernelGGL(embed_bwd_reduce_kernel, dim3((nfb + nchar + 63) / 64), dim3(64 * EMB_RED_G), 0, stream,
                       (const float*)workspace, blocks, nfb, nchar, d_filt, d_bias, nfilt, d_char_emb);
  }
  FVTA_CHECK_LAUNCH("embed_bwd");
  return FVTA_OK;
}

// The dense gradient of the focal logits cube, and the fused backward of softsel: the two kernels the autograd layer
// (fvta_memexqa_amd/autograd.py) needs on top of the model's own backward.
//
// fvta_attn_cube_bwd: dA [N,K,T,JQ], the gradient of the value fvta_attn_fwd writes to a_logits (model_v2.py:210-298's
// second result), -> d_hinfo, d_hq, dW, db at any K, any T, with tanh.  attn_dense.hip's attn_logits_bwd_kernel is the
// same arithmetic for K = 1 with one batch row resident in LDS; here a workgroup takes (n, k, a range of rows):
//   x[t,j] = sum_c U h q + Rh.h + R2.h^2 + Cq.q + C2.q^2 + b                                          (attn_common.h)
//   G      = dA                      (the mask is additive: exp_mask passes the gradient to masked entries too)
//          = dA (1 - tanh(x)^2)      under add_tanh: x is recomputed, the forward's output holds -1e30 where masked
//   dh[t]  = U (G q)[t] + rs[t] (Rh + 2 R2 h[t])        rs = row sums of G
//   dq[j]  = U (G^T h)[j] + cs[j] (Cq + 2 C2 q[j])      cs = column sums of G;  d_hq sums over k
// G of the workgroup's rows lives in LDS; a thread owns a channel, keeps its column of q and of dq in registers and walks
// the rows, so h is read once and d_hinfo written once (plain stores unless `accumulate`).  Under add_tanh the
// pre-activation is a register-tiled product (4 x 4 per thread) ahead of that walk: the workgroup reads its rows a
// second time, right after the first (from L2 / the memory-side cache when the range fits).
// d_hq and the parameter vectors leave every workgroup as its own slab; fixed-order folds add them up (no atomics:
// two runs are bitwise equal).  The vectors come from W through attn_common.h's attn_vecs_of (no cosine branch: the entry
// refuses simiMatrix 4); the last fold is attn_dense.hip's attn_logits_bwd_params_kernel (attn_bwd_shared.h).
#include "attn_bwd_shared.h"

namespace fvta {

constexpr int CUBE_GMAX = 10240;  // floats of G one workgroup keeps in LDS
constexpr int CUBE_RMAX = 512;    // rows of one workgroup (row sums in LDS)
constexpr int CUBE_XC = 32;       // channels per slice of a pre-activation tile
typedef float f32x2 __attribute__((ext_vector_type(2)));

struct CubePlan {
  int jt;      // 8 | 16 | 32 | 64: questions padded, the LDS row stride of G and the register tile
  int nsp;     // workgroups per (n,k)
  int rw;      // rows per workgroup
  size_t nwg;  // N * K * nsp
};

inline CubePlan cube_plan(const fvta_attn_desc* d) {
  CubePlan p;
  p.jt = d->JQ <= 8 ? 8 : d->JQ <= 16 ? 16 : d->JQ <= 32 ? 32 : 64;
  int rmax = CUBE_GMAX / p.jt;
  if (rmax > CUBE_RMAX) rmax = CUBE_RMAX;
  const int64_t nk = (int64_t)d->N * d->K;
  int64_t want = (1024 + nk - 1) / nk;  // ~4 workgroups per CU when the shape allows
  const int maxs = (d->T + 63) / 64;
  if (want > maxs) want = maxs;
  const int need = (d->T + rmax - 1) / rmax;
  int nsp = (int)(want > need ? want : need);
  if (nsp < 1) nsp = 1;
  p.rw = (d->T + nsp - 1) / nsp;
  p.nsp = (d->T + p.rw - 1) / p.rw;
  p.nwg = (size_t)nk * p.nsp;
  return p;
}

struct CubeWork {
  float *slab_q, *slab_v, *slab_b, *pn, *pb;
  size_t bytes;
};

inline CubeWork cube_work(const fvta_attn_desc* d, const CubePlan& p, void* ws) {
  FvtaCarver c(ws);
  CubeWork v;
  v.slab_q = c.take<float>(p.nwg * d->JQ * d->w);      // [nwg][JQ][w]
  v.slab_v = c.take<float>(p.nwg * VEC_COUNT * d->w);  // [nwg][5][w]
  v.slab_b = c.take<float>(p.nwg);
  v.pn = c.take<float>((size_t)d->N * VEC_COUNT * d->w);  // [N][5][w]
  v.pb = c.take<float>((size_t)d->N);
  v.bytes = c.off;
  return v;
}

// grid N * K * nsp, 256 threads
template <int JT>
__global__ __launch_bounds__(256, 2) void attn_cube_bwd_kernel(const float* __restrict__ hinfo, size_t hstride,
                                                           const float* __restrict__ hq, const float* __restrict__ W,
                                                           const float* __restrict__ b, const float* __restrict__ dA,
                                                           float* __restrict__ d_hinfo, float* __restrict__ slab_q,
                                                           float* __restrict__ slab_v, float* __restrict__ slab_b, int K, int T,
                                                           int JQ, int w, int simi, int feat_order, int add_tanh,
                                                           int accumulate, int nsp, int rw) {
  __shared__ __attribute__((aligned(16))) float s_g[CUBE_GMAX];
  __shared__ float s_rs[CUBE_RMAX];
  __shared__ float s_cs[64], s_ct[64];
  // pre-activation tile: XJ questions (4 per thread) x XR rows (4 per thread) over the 256 threads
  constexpr int XJ = JT < 32 ? 32 : JT, TXN = XJ / 4, XR = 4 * (256 / TXN);
  __shared__ float s_xh[XR][CUBE_XC + 1];
  __shared__ float s_xq[XJ][CUBE_XC + 1];
  __shared__ float s_xv[2][CUBE_XC];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const size_t wg = blockIdx.x;
  const int sp = (int)(wg % nsp);
  const size_t nk = wg / nsp;
  const size_t n = nk / K;
  const int t0 = sp * rw;
  const int rows = min(rw, T - t0);
  const size_t hoff = (hstride ? n * hstride : nk * (size_t)T * w) + (size_t)t0 * w;
  const float* h = hinfo + hoff;
  float* dh = d_hinfo + hoff;
  const float* q = hq + n * JQ * w;
  const float* gin = dA + (nk * T + t0) * JQ;

  for (int i = tid; i < rows * JT; i += 256) {
    const int t = i / JT, j = i - t * JT;
    s_g[i] = j < JQ ? gin[(size_t)t * JQ + j] : 0.f;
  }
  __syncthreads();

  if (add_tanh) {  // G = dA (1 - tanh(x)^2): model_v2.py:92-93 under the additive mask
    for (int j = wave; j < JQ; j += 4) {  // ct[j] = Cq.q[j] + C2.q[j]^2 + b
      float acc = 0.f;
      for (int c = lane; c < w; c += 64) {
        float U, Rh, R2, Cq, C2;
        attn_vecs_of<false>(W, w, simi, feat_order, c, U, Rh, R2, Cq, C2);
        const float qv = q[(size_t)j * w + c];
        acc += qv * (Cq + C2 * qv);
      }
      acc = wave_sum(acc);
      if (lane == 0) s_ct[j] = acc + b[0];
    }
    const int tx = tid % TXN, ty = tid / TXN;  // a thread's 4 x 4 corner of the tile: rows ty*4.., questions tx*4..
    for (int r0 = 0; r0 < rows; r0 += XR) {
      f32x2 acc[4][2];
      float rt[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        rt[i] = 0.f;
        acc[i][0] = acc[i][1] = f32x2{0.f, 0.f};
      }
      for (int c0 = 0; c0 < w; c0 += CUBE_XC) {
        __syncthreads();
        {
          const int cc = tid & 31, rb = tid >> 5;  // 8 rows of the slice per pass, this thread's channel fixed
          float U, Rh, R2, Cq, C2;
          attn_vecs_of<false>(W, w, simi, feat_order, c0 + cc, U, Rh, R2, Cq, C2);
#pragma unroll
          for (int i = 0; i < XR / 8; ++i) {
            const int rr = rb + 8 * i;
            s_xh[rr][cc] = r0 + rr < rows ? h[(size_t)(r0 + rr) * w + c0 + cc] : 0.f;
          }
#pragma unroll
          for (int i = 0; i < XJ / 8; ++i) {
            const int rr = rb + 8 * i;
            s_xq[rr][cc] = rr < JQ ? U * q[(size_t)rr * w + c0 + cc] : 0.f;
          }
          if (rb == 0) {
            s_xv[0][cc] = Rh;
            s_xv[1][cc] = R2;
          }
        }
        __syncthreads();
#pragma unroll 8
        for (int cc = 0; cc < CUBE_XC; ++cc) {
          float hv[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) hv[i] = s_xh[ty * 4 + i][cc];
          const f32x2 qa = {s_xq[tx * 4][cc], s_xq[tx * 4 + 1][cc]}, qb = {s_xq[tx * 4 + 2][cc], s_xq[tx * 4 + 3][cc]};
          const float Rh = s_xv[0][cc], R2 = s_xv[1][cc];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            rt[i] += hv[i] * (Rh + R2 * hv[i]);
            const f32x2 h2 = {hv[i], hv[i]};
            acc[i][0] = __builtin_elementwise_fma(h2, qa, acc[i][0]);
            acc[i][1] = __builtin_elementwise_fma(h2, qb, acc[i][1]);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = r0 + ty * 4 + i;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const int j = tx * 4 + jj;
          if (row < rows && j < JQ) {
            const f32x2 a2 = acc[i][jj >> 1];
            const float y = tanhf((jj & 1 ? a2.y : a2.x) + rt[i] + s_ct[j]);
            s_g[row * JT + j] *= 1.f - y * y;
          }
        }
      }
    }
    __syncthreads();
  }

  // row sums (a wave per row), column sums (256 / JT partial sums per question, folded in order)
  for (int t = wave; t < rows; t += 4) {
    float v = lane < JT ? s_g[t * JT + lane] : 0.f;
    v = wave_sum(v);
    if (lane == 0) s_rs[t] = v;
  }
  {
    constexpr int P = 256 / JT;
    float* part = &s_xh[0][0];  // P * JT = 256 floats
    const int j = tid % JT, p = tid / JT;
    float acc = 0.f;
    for (int t = p; t < rows; t += P) acc += s_g[t * JT + j];
    __syncthreads();  // the pre-activation tiles are done with s_xh
    part[p * JT + j] = acc;
    __syncthreads();
    if (tid < JT) {
      float cs = 0.f;
      for (int pp = 0; pp < P; ++pp) cs += part[pp * JT + tid];
      s_cs[tid] = cs;
    }
    __syncthreads();
    if (tid == 0) {
      float tot = 0.f;
      for (int jj = 0; jj < JQ; ++jj) tot += s_cs[jj];
      slab_b[wg] = tot;
    }
  }

  for (int c = tid; c < w; c += 256) {
    float U, Rh, R2, Cq, C2;
    attn_vecs_of<false>(W, w, simi, feat_order, c, U, Rh, R2, Cq, C2);
    f32x2 qv[JT / 2], dq[JT / 2];  // pairs of questions: v_pk_fma_f32
#pragma unroll
    for (int j = 0; j < JT / 2; ++j) {
      qv[j].x = 2 * j < JQ ? q[(size_t)(2 * j) * w + c] : 0.f;
      qv[j].y = 2 * j + 1 < JQ ? q[(size_t)(2 * j + 1) * w + c] : 0.f;
      dq[j] = f32x2{0.f, 0.f};
    }
    float dRh = 0.f, dR2 = 0.f;
    // rows in groups of 4, the next group's h (and, when adding, d_hinfo) loads in flight under this group's arithmetic
    float hn[4], on[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      hn[u] = u < rows ? h[(size_t)u * w + c] : 0.f;
      on[u] = accumulate && u < rows ? dh[(size_t)u * w + c] : 0.f;
    }
    for (int t = 0; t < rows; t += 4) {
      float hc[4], oc[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        hc[u] = hn[u];
        oc[u] = on[u];
        const int tn = t + 4 + u;
        hn[u] = tn < rows ? h[(size_t)tn * w + c] : 0.f;
        on[u] = accumulate && tn < rows ? dh[(size_t)tn * w + c] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (t + u < rows) {
          const float hv = hc[u];
          const float4* g4 = reinterpret_cast<const float4*>(&s_g[(t + u) * JT]);
          const f32x2 hv2 = {hv, hv};
          f32x2 acc2 = {0.f, 0.f};
#pragma unroll
          for (int j4 = 0; j4 < JT / 4; ++j4) {
            const float4 g = g4[j4];
            const f32x2 ga = {g.x, g.y}, gb = {g.z, g.w};
            acc2 = __builtin_elementwise_fma(ga, qv[2 * j4], acc2);
            acc2 = __builtin_elementwise_fma(gb, qv[2 * j4 + 1], acc2);
            dq[2 * j4] = __builtin_elementwise_fma(ga, hv2, dq[2 * j4]);
            dq[2 * j4 + 1] = __builtin_elementwise_fma(gb, hv2, dq[2 * j4 + 1]);
            if ((j4 & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // keep the LDS reads of G from piling up in registers
          }
          const float acc = acc2.x + acc2.y;
          const float rs = s_rs[t + u];
          dh[(size_t)(t + u) * w + c] = oc[u] + (U * acc + rs * (Rh + 2.f * R2 * hv));
          dRh += rs * hv;
          dR2 += rs * hv * hv;
        }
      }
    }
    float dU = 0.f, dCq = 0.f, dC2 = 0.f;
    float* sq = slab_q + wg * JQ * w + c;
#pragma unroll
    for (int j = 0; j < JT; ++j) {
      if (j < JQ) {
        const float cs = s_cs[j];
        const float dqj = j & 1 ? dq[j / 2].y : dq[j / 2].x, qj = j & 1 ? qv[j / 2].y : qv[j / 2].x;
        sq[(size_t)j * w] = U * dqj + cs * (Cq + 2.f * C2 * qj);
        dU += dqj * qj;
        dCq += cs * qj;
        dC2 += cs * qj * qj;
      }
    }
    float* sv = slab_v + wg * VEC_COUNT * w + c;
    sv[(size_t)VEC_U * w] = dU;
    sv[(size_t)VEC_RH * w] = dRh;
    sv[(size_t)VEC_R2 * w] = dR2;
    sv[(size_t)VEC_CQ * w] = dCq;
    sv[(size_t)VEC_C2 * w] = dC2;
  }
}

// d_hq[n, e] (+)= sum over n's S slabs, in slab order (k major, then the row ranges).  e < per = JQ * w; grid (ceil(per/256), N)
__global__ __launch_bounds__(256) void cube_fold_q_kernel(const float* __restrict__ slab_q, float* __restrict__ d_hq, int S,
                                                         size_t per, int accumulate) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
  if (e >= per) return;
  const float* s = slab_q + n * S * per + e;
  float acc = 0.f;
  for (int i = 0; i < S; ++i) acc += s[(size_t)i * per];
  float* o = d_hq + n * per + e;
  *o = accumulate ? *o + acc : acc;
}

// pn[n, e] = sum over n's S slabs of the parameter-vector partials (e < per = 5 w), pb[n] likewise: the per-n partials
// attn_logits_bwd_params_kernel folds over n.  grid (ceil(per/256) + 1, N)
__global__ __launch_bounds__(256) void cube_fold_v_kernel(const float* __restrict__ slab_v, const float* __restrict__ slab_b,
                                                         float* __restrict__ pn, float* __restrict__ pb, int S, size_t per) {
  const size_t n = blockIdx.y;
  if (blockIdx.x == gridDim.x - 1) {
    if (threadIdx.x == 0) {
      float acc = 0.f;
      for (int i = 0; i < S; ++i) acc += slab_b[n * S + i];
      pb[n] = acc;
    }
    return;
  }
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= per) return;
  const float* s = slab_v + n * S * per + e;
  float acc = 0.f;
  for (int i = 0; i < S; ++i) acc += s[(size_t)i * per];
  pn[n * per + e] = acc;
}

// softsel backward, one workgroup per row: p = softmax(logits[r]) recomputed into LDS (an all -1e30 row comes out uniform,
// as in softsel_kernel), g[j] = d_out . target[j] (a wave per j), d_logits = p (g - sum p g), d_target[j] = p[j] d_out.
// grid rows, 256 threads, dyn LDS J floats
__global__ __launch_bounds__(256) void softsel_bwd_kernel(const float* __restrict__ target, const float* __restrict__ logits,
                                                         const float* __restrict__ d_out, float* __restrict__ d_target,
                                                         float* __restrict__ d_logits, int J, int d) {
  extern __shared__ float s_p[];
  __shared__ float s_red[4];
  const size_t r = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* lr = logits + r * J;
  float m = -INFINITY;
  for (int j = tid; j < J; j += 256) m = fmaxf(m, lr[j]);
  m = wave_max(m);
  if (lane == 0) s_red[wv] = m;
  __syncthreads();
  m = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
  __syncthreads();
  float s = 0.f;
  for (int j = tid; j < J; j += 256) {
    const float e = expf(lr[j] - m);
    s_p[j] = e;
    s += e;
  }
  s = wave_sum(s);
  if (lane == 0) s_red[wv] = s;
  __syncthreads();
  const float inv = 1.f / ((s_red[0] + s_red[1]) + (s_red[2] + s_red[3]));
  __syncthreads();
  const float* tr = target + r * (size_t)J * d;
  const float* go = d_out + r * d;
  if (d_logits) {
    float* dl = d_logits + r * J;
    float dot = 0.f;  // lane 0: sum of p g over this wave's j, in j order
    for (int j = wv; j < J; j += 4) {
      float acc = 0.f;
      for (int c = lane; c < d; c += 64) acc += go[c] * tr[(size_t)j * d + c];
      acc = wave_sum(acc);
      if (lane == 0) {
        dl[j] = acc;  // g[j], parked where its reader (this lane) finds it again
        dot += s_p[j] * inv * acc;
      }
    }
    if (lane == 0) s_red[wv] = dot;
    __syncthreads();
    dot = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
    if (lane == 0)
      for (int j = wv; j < J; j += 4) dl[j] = s_p[j] * inv * (dl[j] - dot);
  }
  if (d_target) {
    float* dt = d_target + r * (size_t)J * d;
    for (int c = tid; c < d; c += 256) {
      const float gc = go[c] * inv;
      for (int j = 0; j < J; ++j) dt[(size_t)j * d + c] = s_p[j] * gc;
    }
  }
}
}  // namespace fvta

using namespace fvta;

static bool cube_desc_ok(const fvta_attn_desc* d) {
  if (!d || d->N <= 0 || d->K <= 0 || d->T <= 0 || d->JQ <= 0 || d->JQ > 64) return false;
  if (d->w != 64 && d->w != 128 && d->w != 256 && d->w != 512 && d->w != 1024 && d->w != 2048) return false;
  if (d->simi < 1 || d->simi > 3) return false;
  if (d->hinfo_stride != 0 && (d->K != 1 || d->hinfo_stride < (int64_t)d->T * d->w)) return false;
  return true;
}

extern "C" size_t fvta_attn_cube_bwd_workspace_bytes(const fvta_attn_desc* d) {
  if (!cube_desc_ok(d)) return 0;
  return cube_work(d, cube_plan(d), nullptr).bytes;
}

extern "C" int fvta_attn_cube_bwd(const fvta_attn_desc* d, const float* hinfo, const float* hq, const float* W, const float* b,
                                  const float* dA, float* d_hinfo, float* d_hq, float* dW, float* db, int accumulate,
                                  void* workspace, fvta_stream_t stream) {
  FVTA_CHECK_ARG(d && hinfo && hq && W && b && dA && d_hinfo && d_hq && dW && db && workspace, "attn_cube_bwd: null pointer");
  FVTA_CHECK_ARG(cube_desc_ok(d),
                 "attn_cube_bwd: needs simiMatrix 1-3, JQ <= 64, w in {64..2048}, hinfo_stride only with K == 1 (N=%d K=%d T=%d "
                 "JQ=%d w=%d simi=%d)", d->N, d->K, d->T, d->JQ, d->w, d->simi);
  FVTA_CHECK_ARG(accumulate == 0 || accumulate == 1, "attn_cube_bwd: accumulate=%d (0 store, 1 add)", accumulate);
  const CubePlan p = cube_plan(d);
  FVTA_CHECK_ARG(p.nwg < (1ull << 31) && p.rw * p.jt <= CUBE_GMAX && p.rw <= CUBE_RMAX, "attn_cube_bwd: shape too large");
  const CubeWork v = cube_work(d, p, workspace);
  hipStream_t st = (hipStream_t)stream;
  const size_t hstride = (size_t)d->hinfo_stride;
#define CUBE_LAUNCH(JT_)                                                                                                    \
  hipLaunchKernelGGL(attn_cube_bwd_kernel<JT_>, dim3((unsigned)p.nwg), dim3(256), 0, st, hinfo, hstride, hq, W, b, dA, d_hinfo, \
                     v.slab_q, v.slab_v, v.slab_b, d->K, d->T, d->JQ, d->w, d->simi, d->feat_order, d->add_tanh, accumulate,   \
                     p.nsp, p.rw)
  if (p.jt == 8) CUBE_LAUNCH(8);
  else if (p.jt == 16) CUBE_LAUNCH(16);
  else if (p.jt == 32) CUBE_LAUNCH(32);
  else CUBE_LAUNCH(64);
#undef CUBE_LAUNCH
  FVTA_CHECK_LAUNCH("attn_cube_bwd");
  const int S = d->K * p.nsp;
  const size_t perq = (size_t)d->JQ * d->w, perv = (size_t)VEC_COUNT * d->w;
  hipLaunchKernelGGL(cube_fold_q_kernel, dim3((unsigned)((perq + 255) / 256), d->N), dim3(256), 0, st, v.slab_q, d_hq, S, perq,
                     accumulate);
  hipLaunchKernelGGL(cube_fold_v_kernel, dim3((unsigned)((perv + 255) / 256) + 1, d->N), dim3(256), 0, st, v.slab_v, v.slab_b,
                     v.pn, v.pb, S, perv);
  hipLaunchKernelGGL(attn_logits_bwd_params_kernel, dim3((d->w + 255) / 256 + 1), dim3(256), 0, st, v.pn, v.pb, dW, db, d->N,
                     d->w, d->simi, d->feat_order);
  FVTA_CHECK_LAUNCH("attn_cube_bwd folds");
  return FVTA_OK;
}

extern "C" int fvta_softsel_bwd(const float* target, const float* logits, const float* d_out, float* d_target, float* d_logits,
                                int64_t rows, int32_t J, int32_t d, fvta_stream_t stream) {
  FVTA_CHECK_ARG(target && logits && d_out && (d_target || d_logits) && rows > 0 && J > 0 && d > 0, "softsel_bwd: bad arguments");
  FVTA_CHECK_ARG(J <= 16000 && rows < (1ll << 31), "softsel_bwd: J=%d > 16000 or too many rows", J);
  hipLaunchKernelGGL(softsel_bwd_kernel, dim3((unsigned)rows), dim3(256), (size_t)J * sizeof(float), (hipStream_t)stream, target,
                     logits, d_out, d_target, d_logits, J, d);
  FVTA_CHECK_LAUNCH("softsel_bwd");
  return FVTA_OK;
}

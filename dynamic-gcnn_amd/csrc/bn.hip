// bn.hip -- K4/K5: slim.batch_norm (batch statistics, beta only, eps 1e-3: dgcnn/ops.py:53,68,
// model.py:52,71,100) + activation + reduce_max / reduce_mean over k (ops.py:56-57), and their
// backward.  All HBM-bound: one float4 column-quad per lane so that a
// wave reads whole 256-B feature rows, k rows per point streamed with k independent loads.
#include "bn_common.h"
#include <stdlib.h>
#include <type_traits>

namespace {

// Slot reduction shared by the two finalize kernels: 4 columns per workgroup, one WAVE per column; lane z adds slots z, z + 64, ...
// (ascending), the 64 partial sums are then combined by a butterfly of lane exchanges: one fixed order for a given slot count,
// whatever wrote the slots.  No LDS and no barrier on purpose: in the backward these small kernels run beside the weight-gradient
// GEMMs of the side stream, whose workgroups hold 154 KB of LDS on every CU (A/B in the step: no measurable difference, 4.75 vs
// 4.74 ms -- kept because it asks for less).
constexpr int FIN_COLS = 4, FIN_LANES = 64;
__device__ __forceinline__ bool slot_sums(const double* __restrict__ acc, int F, int nslots, int& f, double& s, double& q,
                                          int colblock) {
  const int c = threadIdx.x / FIN_LANES, z = threadIdx.x % FIN_LANES;
  f = colblock * FIN_COLS + c;
  if (f >= F) return false;                    // wave-uniform
  double a = 0.0, b = 0.0;
  // four slots in flight per lane (slots z, z + 64, z + 128, z + 192 of every group of 256), added in that order
  int sl = z;
  for (; sl + 3 * FIN_LANES < nslots; sl += 4 * FIN_LANES) {
    double va[4], vb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      va[u] = acc[((int64_t)(sl + u * FIN_LANES) * 2 + 0) * F + f];
      vb[u] = acc[((int64_t)(sl + u * FIN_LANES) * 2 + 1) * F + f];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) { a += va[u]; b += vb[u]; }
  }
  for (; sl < nslots; sl += FIN_LANES) {
    a += acc[((int64_t)sl * 2 + 0) * F + f];
    b += acc[((int64_t)sl * 2 + 1) * F + f];
  }
#pragma unroll
  for (int o = 1; o < FIN_LANES; o <<= 1) {
    a += __shfl_xor(a, o);
    b += __shfl_xor(b, o);
  }
  s = a;
  q = b;
  return z == 0;
}

__global__ __launch_bounds__(FIN_COLS * FIN_LANES) void bn_finalize_kernel(const double* __restrict__ stats, int F, int nslots,
                                                                           double count, float eps, float* __restrict__ mean,
                                                                           float* __restrict__ rstd) {
  int f;
  double s, q;
  if (!slot_sums(stats, F, nslots, f, s, q, blockIdx.x)) return;
  const double mu = s / count;
  double var = q / count - mu * mu;   // biased variance, in double: no fp32 cancellation
  if (var < 0.0) var = 0.0;
  mean[f] = (float)mu;
  rstd[f] = (float)(1.0 / sqrt(var + (double)eps));
}

// reduce the slots of a backward reduction in place into slot 0, and emit dbeta
__global__ __launch_bounds__(FIN_COLS * FIN_LANES) void bn_bwd_finalize_kernel(double* __restrict__ red, int F, int nslots,
                                                                               float* __restrict__ dbeta, float dbeta_beta) {
  int f;
  double s, q;
  if (!slot_sums(red, F, nslots, f, s, q, blockIdx.x)) return;
  red[f] = s;
  red[F + f] = q;
  if (dbeta) dbeta[f] = (dbeta_beta != 0.f) ? (float)s + dbeta_beta * dbeta[f] : (float)s;
}

// item -> (row, first channel).  FV (channel quads per row) is a power of two for every width of the
// model, so the 64-bit division that used to dominate the k = 1 kernels becomes a shift.
__device__ __forceinline__ void split_item(int64_t it, int FV, int fv_shift, int64_t& r, int& fq) {
  if (fv_shift >= 0) {
    r = it >> fv_shift;
    fq = (int)(it & (FV - 1));
  } else if (it < 0x7fffffffll) {
    const unsigned u = (unsigned)it, d = (unsigned)FV;
    r = u / d;
    fq = (int)(u % d);
  } else {
    r = it / FV;
    fq = (int)(it % FV);
  }
}

// ---- where the k rows of a point come from ------------------------------------------------------------
// G = false: the materialised tensor Y[(r*k + m)*F + f].
// G = true : conv0 of an EdgeConv layer, never materialised: y = V[cloud(r)*N + idx[r*k + m]][f] + U[r][f]
//            (dgcnn_edge_gather_add_f32's formula; the same single fp32 add everywhere, so values recomputed
//            in different kernels compare equal).  V / U are point-level (k times smaller than Y) and are
//            served by L2 / MALL: the forward writes no edge tensor at all, the backward only dY.
struct Src {
  const float* Y;
  const float* V; int64_t ldv;
  const float* U; int64_t ldu;
  const int32_t* idx;
  unsigned npts;
};

#ifndef BN_NB
#define BN_NB 4
#endif
constexpr int NB = BN_NB;    // rows in flight per lane

template <int V, bool G>
struct Rows {
  const float* base;
  const int32_t* ip;
  int64_t ld;
  float u[V];
  __device__ __forceinline__ void init(const Src& s, int64_t r, int k, int F, int f) {
    if (G) {
      const unsigned cloud = (unsigned)r / s.npts;
      base = s.V + (int64_t)cloud * s.npts * s.ldv + f;
      ip = s.idx + r * k;
      ld = s.ldv;
      Vec<V>::ld(s.U + r * s.ldu + f, u);
    } else {
      base = s.Y + (r * k) * F + f;
      ip = nullptr;
      ld = F;
    }
  }
  // rows m .. m+NB-1.  Gathered rows: no control flow, indices past k-1 re-read row k-1 (the caller ignores
  // them).  Dense rows (mostly k = 1): rows past k-1 are skipped (k, m are wave-uniform: scalar branches).
  __device__ __forceinline__ void load(int m, int k, float (&y)[NB][V]) const {
    if constexpr (G) {
      // row offset in ONE full-rate multiply (v_mul_u32_u24): index < N <= 2^24 and N * ld < 2^32 elements (check_edge); the
      // 64-bit form cost a v_mad_u64_u32 and two v_mul_lo_u32 -- quarter rate each -- per gathered row, a quarter of the vector
      // time of the forward max/mean pass (profiles/r03/kreduce_probe.txt)
      unsigned row[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b) row[b] = row_offset24((unsigned)ip[(m + b < k) ? (m + b) : (k - 1)], (unsigned)ld);
#pragma unroll
      for (int b = 0; b < NB; ++b) Vec<V>::ld(base + row[b], y[b]);
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int v = 0; v < V; ++v) y[b][v] += u[v];
    } else {
#pragma unroll
      for (int b = 0; b < NB; ++b)
        if (m + b < k) Vec<V>::ld(base + (int64_t)(m + b) * ld, y[b]);
    }
  }
};

// item = (row, channel quad).  G: XCD x (blockIdx % 8) owns the x-th eighth of the rows and its blocks sweep it
// side by side, so the clouds whose V rows an XCD's L2 holds at any moment are few.
struct Items { int64_t base, count, first, step; };
template <bool G>
__device__ __forceinline__ Items items_of(int64_t R, int FV) {
  Items it;
  if (G) {
    const int64_t per = (R + 7) / 8;
    const int64_t rb = (int64_t)(blockIdx.x & 7) * per;
    int64_t rows = R - rb;
    rows = rows < 0 ? 0 : (rows > per ? per : rows);
    it.base = rb * FV;
    it.count = rows * FV;
    it.first = (int64_t)(blockIdx.x >> 3) * blockDim.x + threadIdx.x;
    it.step = (int64_t)(gridDim.x >> 3) * blockDim.x;
  } else {
    it.base = 0;
    it.count = R * FV;
    it.first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    it.step = (int64_t)gridDim.x * blockDim.x;
  }
  return it;
}

// ---- forward: z = (y-mu)*rstd + beta; relu; max / mean over the k rows of each point ----
// Register-held form of the edge variant with a ReLU, for k <= HELD_K: the k x 4 values z of an item are computed once
// into registers (KC = k rounded up to whole groups of NB rows; rows past k - 1 repeat row k - 1 and are left out of sum and counts
// by wave-uniform branches), then maximum, sum over m ascending and the number of positive z in one walk, the number of z == max
// in a second.  Same z, same additions in the same order as the loop of bn_act_kreduce_kernel, so max, mean and the packed count
// are its bits.  What is gone is bookkeeping: the running-tie select chain (3 selects, a compare and a float add per element) and
// the float select-and-add of the positive count become compare + integer add-with-carry, converted to the packed float once.
// The maximum may be v_max_f32 HERE because every z left max(., 0): never a NaN, never -0.0, so "z > mx ? z : mx" from -inf picks
// the same bits (without a ReLU the first zero seen keeps its sign in the loop form; those calls keep the loop).
constexpr int HELD_GROUPS = 5;              // 5 x NB = 20 rows: 80 values; the kernel stays at 4 waves / SIMD with no scratch
constexpr int HELD_K = HELD_GROUPS * NB;
template <int KC>
__device__ __forceinline__ void kreduce_held(const Rows<4, true>& rows, int k, const float (&mu)[4], const float (&rs)[4],
                                             const float (&be)[4], float (&mx)[4], float (&sm)[4], float (&cn)[4]) {
  constexpr int V = 4, H = V / 2;
  static_assert(KC % NB == 0 && KC <= HELD_K, "whole groups of NB rows");
  // channel pairs as 2-vectors: the element-wise v_pk_add_f32 / v_pk_mul_f32 the loop form compiles to (no contraction: Makefile)
  f32x2 u2[H], mu2[H], rs2[H], be2[H], z[KC][H];
#pragma unroll
  for (int h = 0; h < H; ++h) {
    u2[h] = f32x2{rows.u[2 * h], rows.u[2 * h + 1]};
    mu2[h] = f32x2{mu[2 * h], mu[2 * h + 1]};
    rs2[h] = f32x2{rs[2 * h], rs[2 * h + 1]};
    be2[h] = f32x2{be[2 * h], be[2 * h + 1]};
  }
#pragma unroll
  for (int m = 0; m < KC; ++m) {
    // Rows::load's gather; only the last group can reach past k - 1 (KC - NB < k), the rows before it take their index from a
    // constant offset
    const unsigned row = row_offset24((unsigned)rows.ip[(m < KC - NB + 1 || m < k) ? m : (k - 1)], (unsigned)rows.ld);
    float yv[V];
    Vec<V>::ld(rows.base + row, yv);
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const f32x2 y = f32x2{yv[2 * h], yv[2 * h + 1]} + u2[h];           // Rows::load's add
      f32x2 xh;
      z[m][h] = bn_z(y, mu2[h], rs2[h], be2[h], 1, xh);
    }
  }
  f32x2 sm2[H];
  unsigned nt[V], np[V];
#pragma unroll
  for (int v = 0; v < V; ++v) { mx[v] = -INFINITY; nt[v] = 0; np[v] = 0; }
#pragma unroll
  for (int h = 0; h < H; ++h) sm2[h] = f32x2{0.f, 0.f};
#pragma unroll
  for (int m = 0; m < KC; ++m)
    if (m < KC - NB + 1 || m < k) {          // KC - NB < k <= KC: only the last group can hold repeated rows
#pragma unroll
      for (int h = 0; h < H; ++h) {
        mx[2 * h] = fmaxf(mx[2 * h], z[m][h].x);
        mx[2 * h + 1] = fmaxf(mx[2 * h + 1], z[m][h].y);
        sm2[h] += z[m][h];
        np[2 * h] += (z[m][h].x > 0.f) ? 1u : 0u;
        np[2 * h + 1] += (z[m][h].y > 0.f) ? 1u : 0u;
      }
    }
#pragma unroll
  for (int m = 0; m < KC; ++m)
    if (m < KC - NB + 1 || m < k) {
#pragma unroll
      for (int h = 0; h < H; ++h) {          // ties share the max gradient (A.5)
        nt[2 * h] += (z[m][h].x == mx[2 * h]) ? 1u : 0u;
        nt[2 * h + 1] += (z[m][h].y == mx[2 * h + 1]) ? 1u : 0u;
      }
    }
#pragma unroll
  for (int h = 0; h < H; ++h) { sm[2 * h] = sm2[h].x; sm[2 * h + 1] = sm2[h].y; }
#pragma unroll
  for (int v = 0; v < V; ++v) cn[v] = (float)(nt[v] + CNT_POS * np[v]);
}

// The loop form: every k, with or without a ReLU; also the dense (G = false) variants.
template <int V, bool G>
__global__ __launch_bounds__(256) void bn_act_kreduce_kernel(
    Src src, int64_t R, int k, int F, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ beta, int relu,
    float* __restrict__ max_out, int64_t ldmax, float* __restrict__ mean_out, int64_t ldmean,
    float* __restrict__ out2, int64_t ldout2, float* __restrict__ cnt_out, int fv_shift) {
  const int FV = F / V;
  const Items its = items_of<G>(R, FV);
  const float invk = 1.0f / (float)k;
  for (int64_t q = its.first; q < its.count; q += its.step) {
    int64_t r;
    int fq;
    split_item(its.base + q, FV, fv_shift, r, fq);
    const int f = fq * V;
    float mu[V], rs[V], be[V], mx[V], sm[V], cn[V], np[V];
    Vec<V>::ld(mean + f, mu); Vec<V>::ld(rstd + f, rs); Vec<V>::ld(beta + f, be);
#pragma unroll
    for (int v = 0; v < V; ++v) { mx[v] = -INFINITY; sm[v] = 0.f; cn[v] = 0.f; np[v] = 0.f; }
    Rows<V, G> rows;
    rows.init(src, r, k, F, f);
    for (int m = 0; m < k; m += NB) {
      float yv[NB][V];
      rows.load(m, k, yv);
#pragma unroll
      for (int b = 0; b < NB; ++b)
        if (m + b < k) {
#pragma unroll
          for (int v = 0; v < V; ++v) {
            float xh;
            const float z = bn_z(yv[b][v], mu[v], rs[v], be[v], relu, xh);
            const bool gt = z > mx[v];
            cn[v] = gt ? 1.f : ((z == mx[v]) ? cn[v] + 1.f : cn[v]);   // ties share the max gradient (A.5)
            mx[v] = gt ? z : mx[v];
            sm[v] += z;
            if (G) np[v] += cnt_pos_term(z);
          }
        }
    }
    Vec<V>::st(max_out + r * ldmax + f, mx);
    if (out2) Vec<V>::st(out2 + r * ldout2 + f, mx);
    if (G) {                       // edge variant: ties + CNT_POS x (rows with z > 0), both exact small integers
#pragma unroll
      for (int v = 0; v < V; ++v) cn[v] += np[v];
    }
    if (cnt_out) Vec<V>::st(cnt_out + r * F + f, cn);
    if (mean_out) {
#pragma unroll
      for (int v = 0; v < V; ++v) sm[v] *= invk;
      Vec<V>::st(mean_out + r * ldmean + f, sm);
    }
  }
}

// The register-held form as a kernel of its own, one instance per group count: inside bn_act_kreduce_kernel<4, true> its 80 values
// would set that kernel's register allocation (71 -> 135 VGPRs, 7 -> 3 waves / SIMD) for the loop form as well.  Same items, same
// grid, same stores.
template <int KC>
__global__ __launch_bounds__(256) void bn_act_kreduce_held_kernel(
    Src src, int64_t R, int k, int F, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ beta,
    float* __restrict__ max_out, int64_t ldmax, float* __restrict__ mean_out, int64_t ldmean,
    float* __restrict__ out2, int64_t ldout2, float* __restrict__ cnt_out, int fv_shift) {
  constexpr int V = 4;
  const int FV = F / V;
  const Items its = items_of<true>(R, FV);
  const float invk = 1.0f / (float)k;
  for (int64_t q = its.first; q < its.count; q += its.step) {
    int64_t r;
    int fq;
    split_item(its.base + q, FV, fv_shift, r, fq);
    const int f = fq * V;
    float mu[V], rs[V], be[V], mx[V], sm[V], cn[V];
    Vec<V>::ld(mean + f, mu); Vec<V>::ld(rstd + f, rs); Vec<V>::ld(beta + f, be);
    Rows<V, true> rows;
    rows.init(src, r, k, F, f);
    kreduce_held<KC>(rows, k, mu, rs, be, mx, sm, cn);
    Vec<V>::st(max_out + r * ldmax + f, mx);
    if (out2) Vec<V>::st(out2 + r * ldout2 + f, mx);
    if (cnt_out) Vec<V>::st(cnt_out + r * F + f, cn);
    if (mean_out) {
#pragma unroll
      for (int v = 0; v < V; ++v) sm[v] *= invk;
      Vec<V>::st(mean_out + r * ldmean + f, sm);
    }
  }
}

// dZ for the k rows of one (point, channel-quad); shared by reduce and apply
template <int V>
struct KState { float mx[V]; float cnt[V]; };

template <int V, bool G>
__device__ __forceinline__ void k_pass_max(const Rows<V, G>& rows, int k, const float (&mu)[V],
                                           const float (&rs)[V], const float (&be)[V], int relu,
                                           KState<V>& st) {
#pragma unroll
  for (int v = 0; v < V; ++v) { st.mx[v] = -INFINITY; st.cnt[v] = 0.f; }
  for (int m = 0; m < k; m += NB) {
    float yv[NB][V];
    rows.load(m, k, yv);
#pragma unroll
    for (int b = 0; b < NB; ++b)
      if (m + b < k) {
#pragma unroll
        for (int v = 0; v < V; ++v) {
          float xh;
          const float z = bn_z(yv[b][v], mu[v], rs[v], be[v], relu, xh);
          if (z > st.mx[v]) { st.mx[v] = z; st.cnt[v] = 1.f; }
          else if (z == st.mx[v]) st.cnt[v] += 1.f;
        }
      }
  }
}

template <int V, bool G>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(
    Src src, int64_t R, int k, int F, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ beta, int relu,
    const float* __restrict__ dmax, int64_t lddmax, const float* __restrict__ dmean, int64_t lddmean,
    const float* __restrict__ mx_in, int64_t ldmx, const float* __restrict__ cnt_in, double* __restrict__ red,
    int fv_shift, int nslots) {
  extern __shared__ float lred[];  // [2][F]
  for (int e = threadIdx.x; e < 2 * F; e += blockDim.x) lred[e] = 0.f;
  __syncthreads();
  const int FV = F / V;
  const Items its = items_of<G>(R, FV);
  const float invk = 1.0f / (float)k;
  int curf = -1;
  float s0[V], s1[V];
#pragma unroll
  for (int v = 0; v < V; ++v) { s0[v] = 0.f; s1[v] = 0.f; }
  for (int64_t q = its.first; q < its.count; q += its.step) {
    int64_t r;
    int fq;
    split_item(its.base + q, FV, fv_shift, r, fq);
    const int f = fq * V;
    if (f != curf) {
      if (curf >= 0) {
#pragma unroll
        for (int v = 0; v < V; ++v) { atomicAdd(&lred[curf + v], s0[v]); atomicAdd(&lred[F + curf + v], s1[v]); s0[v] = 0.f; s1[v] = 0.f; }
      }
      curf = f;
    }
    float mu[V], rs[V], be[V], dmx[V], dmn[V];
    Vec<V>::ld(mean + f, mu); Vec<V>::ld(rstd + f, rs); Vec<V>::ld(beta + f, be);
    Vec<V>::ld(dmax + r * lddmax + f, dmx);
    Rows<V, G> rows;
    rows.init(src, r, k, F, f);
    KState<V> st;
    if (dmean) {
      Vec<V>::ld(dmean + r * lddmean + f, dmn);
      if (mx_in) {                 // forward kept (max, #ties): the rows are read once
        Vec<V>::ld(mx_in + r * ldmx + f, st.mx);
        Vec<V>::ld(cnt_in + r * F + f, st.cnt);
        if (G) {
#pragma unroll
          for (int v = 0; v < V; ++v) st.cnt[v] = cnt_ties(st.cnt[v]);
        }
      } else {
        k_pass_max<V, G>(rows, k, mu, rs, be, relu, st);
      }
    }
    for (int m = 0; m < k; m += NB) {
      float yv[NB][V];
      rows.load(m, k, yv);
#pragma unroll
      for (int b = 0; b < NB; ++b)
        if (m + b < k) {
#pragma unroll
          for (int v = 0; v < V; ++v) {
            float xh;
            const float z = bn_z(yv[b][v], mu[v], rs[v], be[v], relu, xh);
            const float d = dmean ? bn_edge_dout(z, st.mx[v], dmx[v] / st.cnt[v], dmn[v] * invk) : dmx[v];
            const float dz = bn_dz_row(z, d, relu);
            s0[v] += dz;
            s1[v] += dz * xh;
          }
        }
    }
  }
  if (curf >= 0) {
#pragma unroll
    for (int v = 0; v < V; ++v) { atomicAdd(&lred[curf + v], s0[v]); atomicAdd(&lred[F + curf + v], s1[v]); }
  }
  __syncthreads();
  const int slot = blockIdx.x % nslots;
  for (int e = threadIdx.x; e < 2 * F; e += blockDim.x)
    atomicAdd(red + (int64_t)slot * 2 * F + e, (double)lred[e]);
}

template <int V, bool G>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(
    Src src, int64_t R, int k, int F, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ beta, int relu,
    const float* __restrict__ dmax, int64_t lddmax, const float* __restrict__ dmean, int64_t lddmean,
    const float* __restrict__ mx_in, int64_t ldmx, const float* __restrict__ cnt_in,
    const double* __restrict__ red, float* dY, float* __restrict__ dYsum, int64_t lddysum, int fv_shift) {
  // relu: bit 0 = the layer has a ReLU; bit 1 = dY is written as bf16 VALUES (round to nearest even, stored as fp32) and dYsum adds
  // those -- the operand rounding of the bf16 edge-MLP's gradient products (oracle.conv_bn_act_bwd(operand_round)), done once here
  const bool round_dy = (relu & 2) != 0;
  relu &= 1;
  const int FV = F / V;
  const Items its = items_of<G>(R, FV);
  const float invk = 1.0f / (float)k;
  const double inv_cnt = 1.0 / ((double)R * (double)k);
  for (int64_t q = its.first; q < its.count; q += its.step) {
    int64_t r;
    int fq;
    split_item(its.base + q, FV, fv_shift, r, fq);
    const int f = fq * V;
    float mu[V], rs[V], be[V], dmx[V], dmn[V], c1[V], c2[V], acc[V];
    Vec<V>::ld(mean + f, mu); Vec<V>::ld(rstd + f, rs); Vec<V>::ld(beta + f, be);
    Vec<V>::ld(dmax + r * lddmax + f, dmx);
#pragma unroll
    for (int v = 0; v < V; ++v) {
      c1[v] = (float)(red[f + v] * inv_cnt);
      c2[v] = (float)(red[F + f + v] * inv_cnt);
      acc[v] = 0.f;
    }
    Rows<V, G> rows;
    rows.init(src, r, k, F, f);
    float* dy = dY + (r * k) * F + f;
    KState<V> st;
    if (dmean) {
      Vec<V>::ld(dmean + r * lddmean + f, dmn);
      if (mx_in) {                 // forward kept (max, #ties): the rows are read once
        Vec<V>::ld(mx_in + r * ldmx + f, st.mx);
        Vec<V>::ld(cnt_in + r * F + f, st.cnt);
        if (G) {
#pragma unroll
          for (int v = 0; v < V; ++v) st.cnt[v] = cnt_ties(st.cnt[v]);
        }
      } else {
        k_pass_max<V, G>(rows, k, mu, rs, be, relu, st);
      }
    }
    for (int m = 0; m < k; m += NB) {
      float yv[NB][V];
      rows.load(m, k, yv);                 // all NB rows are in registers before the first store (dY may be Y)
#pragma unroll
      for (int b = 0; b < NB; ++b)
        if (m + b < k) {
          float o[V];
#pragma unroll
          for (int v = 0; v < V; ++v) {
            float xh;
            const float z = bn_z(yv[b][v], mu[v], rs[v], be[v], relu, xh);
            const float d = dmean ? bn_edge_dout(z, st.mx[v], dmx[v] / st.cnt[v], dmn[v] * invk) : dmx[v];
            const float dz = bn_dz_row(z, d, relu);
            o[v] = bn_dy(rs[v], dz, c1[v], xh, c2[v]);
            if (round_dy) o[v] = round_bf16_rne(o[v]);
            acc[v] += o[v];
          }
          Vec<V>::st(dy + (int64_t)(m + b) * F, o);
        }
    }
    if (dYsum) Vec<V>::st(dYsum + r * lddysum + f, acc);
  }
}


// ---- conv0 backward of an EdgeConv layer whose input needs NO gradient and has C <= 4 channels (the first layer: raw
// coordinates): the whole edge-level backward collapses into this one pass.  Per edge it forms dY exactly as
// bn_bwd_apply_kernel<4, true> does -- and consumes it on the spot: dW0 = E^T dY with E = [x_i, x_j - x_i] (ops.py:39-52),
//   dW0[c]     += x_i[c] * sum_m dY[i, m]          dW0[C + c] += sum_m (x_j[c] - x_i[c]) * dY[i, m]
// so no dY (252 MB at configs[1]) is written, no transposed adjacency is built or summed, and the two point-level GEMMs of
// the folded form are not needed.  A thread owns one channel quad for its whole life (items_of<true>: the item stride is a
// multiple of F / 4), accumulates 2 C x 4 partial sums in registers, the block reduces them through LDS into
// partial[block][2 C][F]; reduce_partials_kernel (gemm.hip) adds the blocks up in fixed order.
// EXACT = false: C <= CC at run time (a padded channel contributes fmaf(0, o, .) to sums nobody reads).  EXACT = true: C == CC, the
// form of edge_bwd_apply_wgrad_exact_kernel below.
template <int CC, bool EXACT>
__device__ __forceinline__ void edge_bwd_apply_wgrad_body(
    Src src, int64_t R, int k, int F, const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ beta, const float* __restrict__ dmax, int64_t lddmax, const float* __restrict__ dmean,
    int64_t lddmean, const float* __restrict__ mx_in, int64_t ldmx, const float* __restrict__ cnt_in,
    const double* __restrict__ red, const float* __restrict__ x, int64_t ldx, int C, float* __restrict__ partial, int fv_shift) {
  constexpr int V = 4;
  extern __shared__ float sh[];                   // [256 / FV row lanes][2 CC][F]
  const int FV = F / V;
  const Items its = items_of<true>(R, FV);
  const float invk = 1.0f / (float)k;
  const double inv_cnt = 1.0 / ((double)R * (double)k);
  float wc[CC][V], wd[CC][V];
#pragma unroll
  for (int c = 0; c < CC; ++c)
#pragma unroll
    for (int v = 0; v < V; ++v) { wc[c][v] = 0.f; wd[c][v] = 0.f; }
  const int fq_fixed = (int)((its.base + its.first) & (FV - 1));          // FV is a power of two here (checked by the host)
  const int f = fq_fixed * V;
  float mu[V], rs[V], be[V], c1[V], c2[V];
  Vec<V>::ld(mean + f, mu); Vec<V>::ld(rstd + f, rs); Vec<V>::ld(beta + f, be);
#pragma unroll
  for (int v = 0; v < V; ++v) {
    c1[v] = (float)(red[f + v] * inv_cnt);
    c2[v] = (float)(red[F + f + v] * inv_cnt);
  }
  for (int64_t q = its.first; q < its.count; q += its.step) {
    const int64_t r = (its.base + q) >> fv_shift;
    float dmx[V], dmn[V];
    Vec<V>::ld(dmax + r * lddmax + f, dmx);
    Vec<V>::ld(dmean + r * lddmean + f, dmn);
    Rows<V, true> rows;
    rows.init(src, r, k, F, f);
    KState<V> st;
    Vec<V>::ld(mx_in + r * ldmx + f, st.mx);
    Vec<V>::ld(cnt_in + r * F + f, st.cnt);
#pragma unroll
    for (int v = 0; v < V; ++v) st.cnt[v] = cnt_ties(st.cnt[v]);
    float xi[CC];
#pragma unroll
    for (int c = 0; c < CC; ++c) xi[c] = (EXACT || c < C) ? x[r * ldx + c] : 0.f;
    const int64_t cloud0 = (int64_t)((unsigned)r / src.npts) * src.npts;
    float acc[V] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (EXACT) {
      // C == CC: a group's NB neighbour rows of x are fetched like its rows of V -- no branch on the channel, one
      // 24-bit multiply per row offset inside the cloud (unsigned 32-bit element offsets; host: N * ldv, N * ldx < 2^32), the channels at constant offsets from it -- so all
      // of a group's loads are in flight together; the loop of the other form issues them one channel at a time behind a branch
      // and a wait each.  Whole groups (m + NB <= k) take their indices from constant offsets and test no row; the last, partial
      // group repeats row k - 1 and skips the repeats.  Same x_j[c] - x_i[c], same dz / o / fmaf chains in m order; no fmaf on a
      // padded channel when CC == 3.
      const float* xc = x + cloud0 * ldx;
      float q1[V], q2[V];                          // loop-invariant operands of dz, formed once: the same division, the same product
#pragma unroll
      for (int v = 0; v < V; ++v) { q1[v] = dmx[v] / st.cnt[v]; q2[v] = dmn[v] * invk; }
      auto group = [&](int m, auto tail) {
        constexpr bool TAIL = decltype(tail)::value;
        float yv[NB][V], dx[NB][CC];
        unsigned j[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) j[b] = (unsigned)rows.ip[(!TAIL || m + b < k) ? (m + b) : (k - 1)];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          // (row_offset24's unsigned product, as in Rows::load: an offset of 2^31 elements or more is zero-extended into the
          // pointer sum, not sign-extended)
          const unsigned xo = row_offset24(j[b], (unsigned)ldx);
          const float* xj = xc + xo;
#pragma unroll
          for (int c = 0; c < CC; ++c) dx[b][c] = xj[c];
        }
        unsigned vo[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) vo[b] = row_offset24(j[b], (unsigned)rows.ld);
#pragma unroll
        for (int b = 0; b < NB; ++b) Vec<V>::ld(rows.base + vo[b], yv[b]);      // Rows::load
#pragma unroll
        for (int b = 0; b < NB; ++b) {
#pragma unroll
          for (int v = 0; v < V; ++v) yv[b][v] += rows.u[v];
#pragma unroll
          for (int c = 0; c < CC; ++c) dx[b][c] -= xi[c];
        }
#pragma unroll
        for (int b = 0; b < NB; ++b)
          if (!TAIL || m + b < k) {
#pragma unroll
            for (int v = 0; v < V; ++v) {
              float xh;
              const float z = bn_z(yv[b][v], mu[v], rs[v], be[v], 1, xh);
              // bn_common.h:bn_dz_edge with relu = 1, spelled out: the call moves this kernel's registers (profiles/bn_common/isa_compare.txt)
              float dz = ((z == st.mx[v]) ? q1[v] : 0.f) + q2[v];
              if (!(z > 0.f)) dz = 0.f;
              const float o = bn_dy(rs[v], dz, c1[v], xh, c2[v]);
              acc[v] += o;
#pragma unroll
              for (int c = 0; c < CC; ++c) wd[c][v] = fmaf(dx[b][c], o, wd[c][v]);
            }
          }
      };
      int m = 0;
      for (; m + NB <= k; m += NB) group(m, std::false_type{});
      if (m < k) group(m, std::true_type{});
    } else {
      for (int m = 0; m < k; m += NB) {
        float yv[NB][V];
        rows.load(m, k, yv);
#pragma unroll
        for (int b = 0; b < NB; ++b)
          if (m + b < k) {
            const float* xj = x + (cloud0 + rows.ip[m + b]) * ldx;
            float dx[CC];
#pragma unroll
            for (int c = 0; c < CC; ++c) dx[c] = (c < C) ? xj[c] - xi[c] : 0.f;
#pragma unroll
            for (int v = 0; v < V; ++v) {
              float xh;
              const float z = bn_z(yv[b][v], mu[v], rs[v], be[v], 1, xh);
              const float o = bn_dy(rs[v], bn_dz_edge(z, st.mx[v], dmx[v] / st.cnt[v], dmn[v] * invk, 1), c1[v], xh, c2[v]);
              acc[v] += o;
#pragma unroll
              for (int c = 0; c < CC; ++c) wd[c][v] = fmaf(dx[c], o, wd[c][v]);
            }
          }
      }
    }
#pragma unroll
    for (int c = 0; c < CC; ++c)
#pragma unroll
      for (int v = 0; v < V; ++v) wc[c][v] = fmaf(xi[c], acc[v], wc[c][v]);
  }
  // block reduction: threads t and t + FV, t + 2 FV ... hold the same channel quad
  const int lanes = 256 / FV;
  const int rl = threadIdx.x / FV;
#pragma unroll
  for (int c = 0; c < CC; ++c)
#pragma unroll
    for (int v = 0; v < V; ++v) {
      sh[(rl * 2 * CC + c) * F + f + v] = wc[c][v];
      sh[(rl * 2 * CC + CC + c) * F + f + v] = wd[c][v];
    }
  __syncthreads();
  float* out = partial + (int64_t)blockIdx.x * 2 * C * F;
  for (int e = threadIdx.x; e < 2 * CC * F; e += 256) {
    const int cr = e / F, ff = e % F;
    const int c = cr < CC ? cr : cr - CC;
    if (c >= C) continue;
    float s = 0.f;
    for (int l = 0; l < lanes; ++l) s += sh[(l * 2 * CC + cr) * F + ff];
    out[(int64_t)(cr < CC ? c : C + c) * F + ff] = s;
  }
}

template <int CC>
__global__ __launch_bounds__(256) void edge_bwd_apply_wgrad_kernel(
    Src src, int64_t R, int k, int F, const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ beta, const float* __restrict__ dmax, int64_t lddmax, const float* __restrict__ dmean,
    int64_t lddmean, const float* __restrict__ mx_in, int64_t ldmx, const float* __restrict__ cnt_in,
    const double* __restrict__ red, const float* __restrict__ x, int64_t ldx, int C, float* __restrict__ partial, int fv_shift) {
  edge_bwd_apply_wgrad_body<CC, false>(src, R, k, F, mean, rstd, beta, dmax, lddmax, dmean, lddmean, mx_in, ldmx, cnt_in, red,
                                       x, ldx, C, partial, fv_shift);
}

// C == CC exactly (3: raw coordinates; 4: the reference's other input width), a kernel of its own so that the run-time-C kernel
// above keeps its code and registers as the fallback (DGCNN_EDGE_VALU=0; C = 1, 2; an ldx the 24-bit row offset cannot hold).
template <int CC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(CC == 3 ? 3 : 2, CC == 3 ? 3 : 2))) void
edge_bwd_apply_wgrad_exact_kernel(
    Src src, int64_t R, int k, int F, const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ beta, const float* __restrict__ dmax, int64_t lddmax, const float* __restrict__ dmean,
    int64_t lddmean, const float* __restrict__ mx_in, int64_t ldmx, const float* __restrict__ cnt_in,
    const double* __restrict__ red, const float* __restrict__ x, int64_t ldx, float* __restrict__ partial, int fv_shift) {
  edge_bwd_apply_wgrad_body<CC, true>(src, R, k, F, mean, rstd, beta, dmax, lddmax, dmean, lddmean, mx_in, ldmx, cnt_in, red,
                                      x, ldx, CC, partial, fv_shift);
}

// ---- k = 1 (per-point layers: conv1, shortcut, merged, FC, Final): column-fixed streaming kernels -------------
// A thread keeps ONE channel quad for its whole life (mean / rstd / beta / the backward constants live in
// registers) and walks rows with 4 independent row loads in flight; block = (256 / FVB rows) x FVB quads,
// blockIdx.y = chunk of 256 quads when F > 1024.  The generic kernels above reload the three parameter quads
// per item, which for k = 1 is most of their load instructions.
struct K1Map {
  int f; int64_t r0, rstep; bool on;
};
__device__ __forceinline__ K1Map k1_map(int F, int FVB, int RP) {   // RP = blockDim.x / FVB
  K1Map m;
  const int t = threadIdx.x;
  const int fq = blockIdx.y * 256 + (t % FVB);
  m.f = fq * 4;
  m.on = (t < RP * FVB) && (m.f < F);
  m.r0 = (int64_t)blockIdx.x * RP + t / FVB;
  m.rstep = (int64_t)gridDim.x * RP;
  return m;
}

// Column sums of a K1-mapped workgroup in a FIXED order: every (row group rp, column quad) thread parks its two partial quads in
// lpark[rp][2][4 FVB] (2048 floats), then one thread per (sum, column) adds the RP row groups in ascending order and hands the
// result to slot (blockIdx.x % nslots) -- no LDS float atomics, whose order changed from run to run.
constexpr int K1_PARK_FLOATS = 2048;
__device__ __forceinline__ void k1_block_sums(float* lpark, const K1Map& m, int F, int FVB, int RP, const float (&s0)[4],
                                              const float (&s1)[4], double* __restrict__ red, int nslots) {
  const int t = threadIdx.x;
  const int W = 4 * FVB;
  if (t < RP * FVB) {
    const int rp = t / FVB, cb = (t % FVB) * 4;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      lpark[(rp * 2 + 0) * W + cb + v] = m.on ? s0[v] : 0.f;
      lpark[(rp * 2 + 1) * W + cb + v] = m.on ? s1[v] : 0.f;
    }
  }
  __syncthreads();
  const int fbase = blockIdx.y * 1024;
  const int slot = blockIdx.x % nslots;
  for (int e = t; e < 2 * W; e += blockDim.x) {
    const int which = e / W, cb = e % W;
    if (fbase + cb < F) {
      float a = 0.f;
      for (int rp = 0; rp < RP; ++rp) a += lpark[(rp * 2 + which) * W + cb];
      atomicAdd(red + ((int64_t)slot * 2 + which) * F + fbase + cb, (double)a);
    }
  }
}

__global__ __launch_bounds__(256) void bn1_act_kernel(const float* __restrict__ T, int64_t R, int F, int FVB, int RP,
                                                      const float* __restrict__ mean, const float* __restrict__ rstd,
                                                      const float* __restrict__ beta, int relu,
                                                      float* __restrict__ out, int64_t ldo, float* __restrict__ out2,
                                                      int64_t ldo2, float* __restrict__ cnt_out,
                                                      const uint64_t* __restrict__ drop_seed, float drop_keep) {
  const K1Map m = k1_map(F, FVB, RP);
  if (!m.on) return;
  // optional dropout fused behind the activation (model.py:90-91): element (row, f) of the (R, F) output keeps its value x 1/keep
  // iff the counter-based mask of dropout_dev_kernel keeps flattened index row * F + f
  const uint64_t dseed = drop_seed ? *drop_seed : 0ull;
  const uint32_t dthr = dropout_threshold(drop_keep);
  const float dscale = drop_seed ? 1.0f / drop_keep : 1.0f;
  float mu[4], rs[4], be[4];
  Vec<4>::ld(mean + m.f, mu); Vec<4>::ld(rstd + m.f, rs); Vec<4>::ld(beta + m.f, be);
  const float one[4] = {1.f, 1.f, 1.f, 1.f};
  for (int64_t r = m.r0; r < R; r += 4 * m.rstep) {
    float y[4][4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int64_t rr = r + b * m.rstep;
      if (rr < R) Vec<4>::ld(T + rr * F + m.f, y[b]);
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int64_t rr = r + b * m.rstep;
      if (rr < R) {
        float z[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) z[v] = bn_z(y[b][v], mu[v], rs[v], be[v], relu);
        if (drop_seed) {
#pragma unroll
          for (int v = 0; v < 4; ++v) z[v] = dropout_keeps(dseed, (uint64_t)(rr * F + m.f + v), dthr) ? z[v] * dscale : 0.f;
        }
        Vec<4>::st(out + rr * ldo + m.f, z);
        if (out2) Vec<4>::st(out2 + rr * ldo2 + m.f, z);
        if (cnt_out) Vec<4>::st(cnt_out + rr * F + m.f, one);
      }
    }
  }
}

// APPLY = false: column sums of dz and dz*xhat into red;  APPLY = true: dT = rstd (dz - c1 - xhat c2) (in place ok)
template <bool APPLY>
__global__ __launch_bounds__(256) void bn1_bwd_kernel(const float* T, int64_t R, int F, int FVB, int RP,
                                                      const float* __restrict__ mean, const float* __restrict__ rstd,
                                                      const float* __restrict__ beta, int relu,
                                                      const float* __restrict__ dout, int64_t lddo,
                                                      const float* __restrict__ dout2, int64_t lddo2,
                                                      double* __restrict__ red, float* dT, float* __restrict__ dsum,
                                                      int64_t lddsum, const uint64_t* __restrict__ drop_seed, float drop_keep,
                                                      int nslots) {
  extern __shared__ float lred[];   // reduce only: K1_PARK_FLOATS
  const uint64_t dseed = drop_seed ? *drop_seed : 0ull;      // dout is the gradient of the DROPPED output (fused dropout backward)
  const uint32_t dthr = dropout_threshold(drop_keep);
  const float dscale = drop_seed ? 1.0f / drop_keep : 1.0f;
  const K1Map m = k1_map(F, FVB, RP);
  float mu[4] = {0, 0, 0, 0}, rs[4] = {0, 0, 0, 0}, be[4] = {0, 0, 0, 0}, c1[4] = {0, 0, 0, 0}, c2[4] = {0, 0, 0, 0};
  float s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0};
  if (m.on) {
    Vec<4>::ld(mean + m.f, mu); Vec<4>::ld(rstd + m.f, rs); Vec<4>::ld(beta + m.f, be);
    if (APPLY) {
      const double inv_cnt = 1.0 / (double)R;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        c1[v] = (float)(red[m.f + v] * inv_cnt);
        c2[v] = (float)(red[F + m.f + v] * inv_cnt);
      }
    }
    for (int64_t r = m.r0; r < R; r += 4 * m.rstep) {
      float y[4][4], d[4][4];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int64_t rr = r + b * m.rstep;
        if (rr < R) {
          Vec<4>::ld(T + rr * F + m.f, y[b]); Vec<4>::ld(dout + rr * lddo + m.f, d[b]);
          if (dout2) {               // the output had two consumers (conv1: the concat slice and MergedEdgeConv's input): dz = d + d2
            float e[4];
            Vec<4>::ld(dout2 + rr * lddo2 + m.f, e);
#pragma unroll
            for (int v = 0; v < 4; ++v) d[b][v] += e[v];
          }
        }
      }
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int64_t rr = r + b * m.rstep;
        if (rr < R) {
          float o[4];
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            float xh;
            const float z = bn_z(y[b][v], mu[v], rs[v], be[v], relu, xh);
            float dz = d[b][v];
            if (drop_seed) dz = dropout_keeps(dseed, (uint64_t)(rr * F + m.f + v), dthr) ? dz * dscale : 0.f;
            dz = bn_dz_row(z, dz, relu);
            if (APPLY) o[v] = bn_dy(rs[v], dz, c1[v], xh, c2[v]);
            else { s0[v] += dz; s1[v] += dz * xh; }
          }
          if (APPLY) {
            Vec<4>::st(dT + rr * F + m.f, o);
            if (dsum) Vec<4>::st(dsum + rr * lddsum + m.f, o);
          }
        }
      }
    }
  }
  if (!APPLY) k1_block_sums(lred, m, F, FVB, RP, s0, s1, red, nslots);
}

// ---- the class-dimension tail (model.py:88-101, trainval.py:39-54): last FC layer (F = 256, dropout behind it) -> Final
// (NUM_CLASS <= 4 columns) -> softmax / loss, and the way back.  At F = 256 the k = 1 map gives one wave per row, lane l on
// columns 4l .. 4l+3 -- the operand mapping of skinny_nn_kernel / skinny_nt_kernel (gemm.hip) -- so the Final layer's products
// are formed in registers beside the BatchNorm passes instead of re-reading the (R, 256) tensors from HBM.  Every kernel here
// performs, per output element and per partial sum, the operations of the launches it replaces in their order (the shared
// helpers of common.h, bn_z, slot_sums): results are bit-identical to the separate launches.

// F1 = bn1_act_kernel (dropout form) + skinny_nn_kernel<N> with statistics (+ the zero fill of [loss, accuracy]).  Launched
// on the grid of the streaming product: rows r = 4 blockIdx.x + wave, stride 4 gridDim.x, in both.
template <int N>
__global__ __launch_bounds__(256) void bn1_act_class_kernel(const float* __restrict__ T, int64_t R,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            const float* __restrict__ beta, int relu,
                                                            float* __restrict__ out, int64_t ldo,
                                                            const uint64_t* __restrict__ drop_seed, float drop_keep,
                                                            const float* __restrict__ W, int64_t ldw,
                                                            float* __restrict__ C, int64_t ldc, double* __restrict__ stats,
                                                            int nslots, float* __restrict__ scal) {
  constexpr int F = 256;
  __shared__ float bs[F * N + 8 * N];            // [F][N] weight, then [4 waves][2][N] for the statistics
  float* red = bs + F * N;
  for (int e = threadIdx.x; e < F * N; e += 256) bs[e] = W[(int64_t)(e / N) * ldw + (e % N)];
  if (scal && blockIdx.x == 0 && threadIdx.x < 2) scal[threadIdx.x] = 0.f;
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int f = lane * 4;
  const int64_t rstep = (int64_t)gridDim.x * 4;
  const uint64_t dseed = *drop_seed;
  const uint32_t dthr = dropout_threshold(drop_keep);
  const float dscale = 1.0f / drop_keep;
  float mu[4], rs[4], be[4];
  Vec<4>::ld(mean + f, mu); Vec<4>::ld(rstd + f, rs); Vec<4>::ld(beta + f, be);
  float cs[N], cq[N];
#pragma unroll
  for (int n = 0; n < N; ++n) { cs[n] = 0.f; cq[n] = 0.f; }
  for (int64_t r = (int64_t)blockIdx.x * 4 + wv; r < R; r += 4 * rstep) {
    float y[4][4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int64_t rr = r + b * rstep;
      if (rr < R) Vec<4>::ld(T + rr * F + f, y[b]);
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int64_t rr = r + b * rstep;             // (wave-uniform: the whole wave takes the tree below)
      if (rr < R) {
        float z[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) z[v] = bn_z(y[b][v], mu[v], rs[v], be[v], relu);
#pragma unroll
        for (int v = 0; v < 4; ++v) z[v] = dropout_keeps(dseed, (uint64_t)(rr * F + f + v), dthr) ? z[v] * dscale : 0.f;
        Vec<4>::st(out + rr * ldo + f, z);
        float acc[N];
#pragma unroll
        for (int n = 0; n < N; ++n) acc[n] = 0.f;
        skinny_nn_chunk<N>(acc, make_float4(z[0], z[1], z[2], z[3]), bs + f * N);
        skinny_nn_tree<N>(acc);
        if (lane == 0) {
#pragma unroll
          for (int n = 0; n < N; ++n) {
            const float v = acc[n];
            C[rr * ldc + n] = v;
            cs[n] += v;
            cq[n] += v * v;
          }
        }
      }
    }
  }
  if (lane == 0) {                               // the four waves' partial sums, added below in wave order (fixed)
#pragma unroll
    for (int n = 0; n < N; ++n) { red[wv * 2 * N + n] = cs[n]; red[wv * 2 * N + N + n] = cq[n]; }
  }
  __syncthreads();
  if (threadIdx.x < 2 * N) {
    const int which = threadIdx.x / N, n = threadIdx.x % N;
    const float a = ((red[threadIdx.x] + red[2 * N + threadIdx.x]) + red[4 * N + threadIdx.x]) + red[6 * N + threadIdx.x];
    atomicAdd(stats + ((int64_t)(blockIdx.x % nslots) * 2 + which) * N + n, (double)a);
  }
}

// F2 = bn_finalize_kernel + bn_act_kreduce_kernel<1, false> (k = 1) + softmax_xent_kernel on the (rows, ncls <= 4) logits:
// every workgroup folds the statistics slots itself (wave c = column c, slot_sums' order), workgroup 0 stores mean / rstd for
// the backward; then row by row z = bn_z(...) -> fin, and softmax / seed / loss / accuracy from fin as softmax_xent_kernel.
__global__ __launch_bounds__(256) void bn_softmax_xent_kernel(const float* __restrict__ Y, const double* __restrict__ stats,
                                                              int nslots, double count, float eps,
                                                              const float* __restrict__ beta, int relu, int64_t rows, int ncls,
                                                              float* __restrict__ mean, float* __restrict__ rstd, float* fin,
                                                              const int32_t* __restrict__ labels,
                                                              const float* __restrict__ weight, float* __restrict__ softmax,
                                                              float* __restrict__ dlogits, float* __restrict__ scal) {
  __shared__ float sl[256], sc[256];
  __shared__ float smu[FIN_COLS], srs[FIN_COLS];
  {
    int f;
    double s, q;
    if (slot_sums(stats, ncls, nslots, f, s, q, 0)) {
      const double mu = s / count;
      double var = q / count - mu * mu;
      if (var < 0.0) var = 0.0;
      smu[f] = (float)mu;
      srs[f] = (float)(1.0 / sqrt(var + (double)eps));
      if (blockIdx.x == 0) { mean[f] = smu[f]; rstd[f] = srs[f]; }
    }
  }
  __syncthreads();
  float loss = 0.f, corr = 0.f;
  const float inv_rows = 1.0f / (float)rows;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x) {
    float* z = fin + r * ncls;
    for (int c = 0; c < ncls; ++c) z[c] = bn_z(Y[r * ncls + c], smu[c], srs[c], beta[c], relu);
    const int lab = labels ? labels[r] : -1;
    const float w = weight ? weight[r] : 1.f;
    softmax_xent_row(z, ncls, lab, w, inv_rows, softmax ? softmax + r * ncls : nullptr,
                     dlogits ? dlogits + r * ncls : nullptr, loss, corr);
  }
  sl[threadIdx.x] = loss;
  sc[threadIdx.x] = corr;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) { sl[threadIdx.x] += sl[threadIdx.x + s]; sc[threadIdx.x] += sc[threadIdx.x + s]; }
    __syncthreads();
  }
  if (threadIdx.x == 0 && scal) {
    atomicAdd(scal + 0, sl[0] * inv_rows);
    atomicAdd(scal + 1, sc[0] * inv_rows);
  }
}

// B1 (APPLY = false) / B2 (APPLY = true) = bn1_bwd_kernel<APPLY> of the last FC layer whose incoming gradient
// d(out) = dT_final W_final^T (skinny_nt_kernel<NC> at beta = 0) is formed in registers instead of loaded.
// B1 first applies the Final layer's own BatchNorm backward to its row (bn_bwd_finalize_kernel + bn_bwd_apply_kernel<1, false>:
// every workgroup folds red_f itself, workgroup 0 adds d(beta_final)); lane 0 of the wave that owns the row stores dT_final in
// place of the Final layer's GEMM output Tf (the weight gradient and B2 read it).  B2 reads the stored dT_final.
template <bool APPLY, int NC>
__global__ __launch_bounds__(256) void bn1_bwd_class_kernel(const float* T, int64_t R, const float* __restrict__ mean,
                                                            const float* __restrict__ rstd, const float* __restrict__ beta,
                                                            int relu, const uint64_t* __restrict__ drop_seed, float drop_keep,
                                                            float* Tf, const float* __restrict__ mean_f,
                                                            const float* __restrict__ rstd_f, const float* __restrict__ beta_f,
                                                            int relu_f, const float* __restrict__ dfin,
                                                            const double* __restrict__ red_f, int nslots_f,
                                                            float* __restrict__ dbeta_f, float dbeta_f_beta,
                                                            const float* __restrict__ W, int64_t ldw,
                                                            double* __restrict__ red, float* dT, int nslots) {
  constexpr int F = 256, FVB = 64, RP = 4;
  extern __shared__ float lred[];   // reduce only: K1_PARK_FLOATS
  __shared__ float sc1[FIN_COLS], sc2[FIN_COLS];
  const uint64_t dseed = *drop_seed;
  const uint32_t dthr = dropout_threshold(drop_keep);
  const float dscale = 1.0f / drop_keep;
  const K1Map m = k1_map(F, FVB, RP);              // (every thread is on: 256 threads = 4 rows x 64 quads)
  float muf[NC], rsf[NC], bef[NC], c1f[NC], c2f[NC];
  if (!APPLY) {
    int f;
    double s, q;
    if (slot_sums(red_f, NC, nslots_f, f, s, q, 0)) {
      const double inv_cnt = 1.0 / ((double)R * (double)1);
      sc1[f] = (float)(s * inv_cnt);
      sc2[f] = (float)(q * inv_cnt);
      if (blockIdx.x == 0 && dbeta_f) dbeta_f[f] = (dbeta_f_beta != 0.f) ? (float)s + dbeta_f_beta * dbeta_f[f] : (float)s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NC; ++k) { muf[k] = mean_f[k]; rsf[k] = rstd_f[k]; bef[k] = beta_f[k]; c1f[k] = sc1[k]; c2f[k] = sc2[k]; }
  }
  float w[4][NC];
#pragma unroll
  for (int v = 0; v < 4; ++v)
#pragma unroll
    for (int k = 0; k < NC; ++k) w[v][k] = W[(int64_t)(m.f + v) * ldw + k];
  float mu[4], rs[4], be[4], c1[4] = {0, 0, 0, 0}, c2[4] = {0, 0, 0, 0};
  float s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0};
  Vec<4>::ld(mean + m.f, mu); Vec<4>::ld(rstd + m.f, rs); Vec<4>::ld(beta + m.f, be);
  if (APPLY) {
    const double inv_cnt = 1.0 / (double)R;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      c1[v] = (float)(red[m.f + v] * inv_cnt);
      c2[v] = (float)(red[F + m.f + v] * inv_cnt);
    }
  }
  for (int64_t r = m.r0; r < R; r += 4 * m.rstep) {
    float y[4][4], a[4][NC], g[4][NC];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int64_t rr = r + b * m.rstep;
      if (rr < R) {
        Vec<4>::ld(T + rr * F + m.f, y[b]);
#pragma unroll
        for (int k = 0; k < NC; ++k) {
          a[b][k] = Tf[rr * NC + k];
          if (!APPLY) g[b][k] = dfin[rr * NC + k];
        }
      }
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int64_t rr = r + b * m.rstep;            // (wave-uniform: one wave per row)
      if (rr < R) {
        if (!APPLY) {                                // the Final layer's BatchNorm backward on this row: a <- dT_final[rr]
#pragma unroll
          for (int k = 0; k < NC; ++k) {
            float xh;
            const float z = bn_z(a[b][k], muf[k], rsf[k], bef[k], relu_f, xh);
            a[b][k] = bn_dy(rsf[k], bn_dz_row(z, g[b][k], relu_f), c1f[k], xh, c2f[k]);
          }
          if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int k = 0; k < NC; ++k) Tf[rr * NC + k] = a[b][k];
          }
        }
        float d[4], o[4];
        skinny_nt_quad<NC>(a[b], w, d);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          float xh;
          const float z = bn_z(y[b][v], mu[v], rs[v], be[v], relu, xh);
          float dz = d[v];
          dz = dropout_keeps(dseed, (uint64_t)(rr * F + m.f + v), dthr) ? dz * dscale : 0.f;
          if (relu && !(z > 0.f)) dz = 0.f;        // bn_common.h:bn_dz_row, spelled out (profiles/bn_common/isa_compare.txt)
          if (APPLY) o[v] = bn_dy(rs[v], dz, c1[v], xh, c2[v]);
          else { s0[v] += dz; s1[v] += dz * xh; }
        }
        if (APPLY) Vec<4>::st(dT + rr * F + m.f, o);
      }
    }
  }
  if (!APPLY) k1_block_sums(lred, m, F, FVB, RP, s0, s1, red, nslots);
}

// Backward BN reduction of an EdgeConv conv0 WITHOUT touching the edges.  With relu and dz_e = [z_e = max_i]
// dmax_i / ties_i + dmean_i / k  (zero where z_e <= 0), summing over the k rows of point i gives
//   sum_m dz        = [max_i > 0] dmax_i + dmean_i npos_i / k
//   sum_m dz xhat   = [max_i > 0] dmax_i (max_i - beta) + (dmean_i / k) (k mean_i - beta npos_i)
// (xhat = z - beta where z > 0; the ties all equal max_i; k mean_i = sum of the positive z): only the forward's
// per-point outputs (max, mean, packed ties/positives) and the incoming gradients are needed.
__global__ __launch_bounds__(256) void edge_bwd_reduce_points_kernel(
    const float* __restrict__ mx, int64_t ldmx, const float* __restrict__ mn, int64_t ldmn,
    const float* __restrict__ cntpos, const float* __restrict__ dmax, int64_t lddmax,
    const float* __restrict__ dmean, int64_t lddmean, const float* __restrict__ beta, int64_t R, int k, int F,
    int FVB, int RP, double* __restrict__ red, int nslots) {
  extern __shared__ float lred[];          // K1_PARK_FLOATS
  const K1Map m = k1_map(F, FVB, RP);
  float s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0};
  if (m.on) {
    float be[4];
    Vec<4>::ld(beta + m.f, be);
    const float invk = 1.0f / (float)k, kf = (float)k;
    for (int64_t r = m.r0; r < R; r += m.rstep) {
      float a[4], b[4], c[4], d[4], e[4];
      Vec<4>::ld(mx + r * ldmx + m.f, a); Vec<4>::ld(mn + r * ldmn + m.f, b); Vec<4>::ld(cntpos + r * F + m.f, c);
      Vec<4>::ld(dmax + r * lddmax + m.f, d); Vec<4>::ld(dmean + r * lddmean + m.f, e);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const float npos = cnt_npos(c[v]);
        const float g1 = (a[v] > 0.f) ? d[v] : 0.f;
        const float g2 = e[v] * invk;
        s0[v] += g1 + g2 * npos;
        s1[v] += g1 * (a[v] - be[v]) + g2 * (kf * b[v] - be[v] * npos);
      }
    }
  }
  k1_block_sums(lred, m, F, FVB, RP, s0, s1, red, nslots);
}

struct K1Grid { dim3 grid; int FVB, RP; };
inline K1Grid k1_grid(int64_t R, int F, int max_blocks, int threads = 256) {
  K1Grid g;
  const int FV = F / 4;
  g.FVB = FV < 256 ? FV : 256;
  g.RP = threads / g.FVB;
  int64_t gx = dg::cdiv(R, (int64_t)g.RP * 4);             // >= 4 rows per thread
  if (gx > max_blocks) gx = max_blocks;
  if (gx < 1) gx = 1;
  g.grid = dim3((unsigned)gx, (unsigned)dg::cdiv(FV, 256));
  return g;
}

inline unsigned grid_for(int64_t items) {
  int64_t g = dg::cdiv(items, 256);
  if (g > 256 * 16) g = 256 * 16;
  if (g < 1) g = 1;
  return (unsigned)g;
}

inline bool a16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline int shift_of(int fv) {
  if (fv <= 0 || (fv & (fv - 1))) return -1;
  int s = 0;
  while ((1 << s) < fv) ++s;
  return s;
}

// the reduce kernel ends with 2F atomics per block: keep the grid small (4 blocks per CU)
inline unsigned grid_reduce(int64_t items) {
  int64_t g = dg::cdiv(items, 256);
  if (g > 1024) g = 1024;
  if (g < 1) g = 1;
  return (unsigned)g;
}

inline Src dense_src(const float* Y) { Src s = {}; s.Y = Y; return s; }

inline Src edge_src(const float* V, int64_t ldv, const float* U, int64_t ldu, const int32_t* idx, int N) {
  Src s = {};
  s.V = V; s.ldv = ldv; s.U = U; s.ldu = ldu; s.idx = idx; s.npts = (unsigned)N;
  return s;
}

// DGCNN_EDGE_VALU=0 (dgcnn_edge_valu(0) in-process): the edge-level passes as they were before the instruction-count forms of
// DESIGN 9.8 -- the loop of bn_act_kreduce_kernel<4, true> for every k, edge_bwd_apply_wgrad_kernel<4> with its run-time C.  Same bits
// either way (tests/test_gpu_edge_valu.py); the old forms also serve the shapes the new ones do not take.
bool edge_valu_on() { return dg::sw_get(dg::SW_EDGE_VALU) == 1; }

inline unsigned grid8(unsigned g) { return (g + 7u) & ~7u; }     // XCD-aware item mapping needs a multiple of 8

// shared argument checks of the gather-sourced (edge) variants
int check_edge(const char* what, const float* V, int64_t ldv, const float* U, int64_t ldu, const int32_t* idx,
               int B, int N, int k, int F) {
  DG_REQUIRE(V && U && idx, DGCNN_EINVAL, "%s: null pointer", what);
  DG_REQUIRE(B > 0 && N > 0 && k > 0 && F > 0, DGCNN_EINVAL, "%s: bad shape", what);
  DG_REQUIRE(F % 4 == 0, DGCNN_EUNSUP, "%s: F must be a multiple of 4 (got %d)", what, F);
  DG_REQUIRE((int64_t)B * N * k < (1ll << 31), DGCNN_EUNSUP, "%s: B*N*k >= 2^31", what);
  DG_REQUIRE(k < CNT_POS, DGCNN_EUNSUP, "%s: k must be < %d", what, CNT_POS);
  DG_REQUIRE(row_offset24_ok(N, ldv), DGCNN_EUNSUP,
             "%s: N * ldv must be < 2^32 elements (32-bit row offsets inside a cloud)", what);
  DG_REQUIRE(a16(V) && a16(U) && ldv % 4 == 0 && ldu % 4 == 0 && ldv >= F && ldu >= F, DGCNN_EINVAL,
             "%s: V, U must be 16-byte aligned with leading dimensions %% 4 == 0", what);
  return DGCNN_OK;
}

template <bool G>
int launch_act_kreduce(const char* what, Src src, int64_t R, int k, int F, const float* mean, const float* rstd,
                       const float* beta, int relu, float* max_out, int64_t ldmax, float* mean_out, int64_t ldmean,
                       float* out2, int64_t ldout2, float* cnt_out, hipStream_t st) {
  DG_REQUIRE(mean && rstd && beta && max_out, DGCNN_EINVAL, "%s: null pointer", what);
  DG_REQUIRE(relu == 0 || relu == 1, DGCNN_EINVAL, "%s: relu must be 0 or 1 (got %d; the bf16 flag belongs to the apply pass)", what, relu);
  const bool vec = (F % 4 == 0) && (ldmax % 4 == 0) && (G || a16(src.Y)) && a16(max_out) && a16(mean) && a16(rstd) &&
                   a16(beta) && (!mean_out || ((ldmean % 4 == 0) && a16(mean_out))) &&
                   (!out2 || ((ldout2 % 4 == 0) && a16(out2))) && (!cnt_out || a16(cnt_out));
  if (G) {
    DG_REQUIRE(vec, DGCNN_EINVAL, "%s: outputs must be 16-byte aligned with leading dimensions %% 4 == 0", what);
    const dim3 grid(grid8(grid_for(R * (F / 4))));
    const int held = (edge_valu_on() && relu == 1 && k <= HELD_K) ? (k + NB - 1) / NB : 0;     // groups of NB rows held in registers
#define DG_HELD(G_)                                                                                                              \
  dg::launch((bn_act_kreduce_held_kernel<(G_) * NB>), grid, dim3(256), 0, st, src, R, k, F, mean, rstd, beta, max_out, ldmax,    \
             mean_out, ldmean, out2, ldout2, cnt_out, shift_of(F / 4))
    static_assert(HELD_GROUPS == 5, "one case per group count");
    switch (held) {
      case 1: DG_HELD(1); break;
      case 2: DG_HELD(2); break;
      case 3: DG_HELD(3); break;
      case 4: DG_HELD(4); break;
      case 5: DG_HELD(5); break;
      default:
        dg::launch((bn_act_kreduce_kernel<4, true>), grid, dim3(256), 0, st, src, R, k, F, mean, rstd, beta, relu, max_out, ldmax,
                   mean_out, ldmean, out2, ldout2, cnt_out, shift_of(F / 4));
    }
#undef DG_HELD
  } else if (vec && k == 1 && !mean_out) {
    const K1Grid g = k1_grid(R, F, 4096);
    dg::launch(bn1_act_kernel, g.grid, dim3(256), 0, st, src.Y, R, F, g.FVB, g.RP, mean, rstd, beta, relu, max_out,
                       ldmax, out2, ldout2, cnt_out, (const uint64_t*)nullptr, 1.0f);
  } else if (vec) {
    dg::launch((bn_act_kreduce_kernel<4, false>), dim3(grid_for(R * (F / 4))), dim3(256), 0, st, src, R, k, F, mean,
                       rstd, beta, relu, max_out, ldmax, mean_out, ldmean, out2, ldout2, cnt_out, shift_of(F / 4));
  } else {
    dg::launch((bn_act_kreduce_kernel<1, false>), dim3(grid_for(R * F)), dim3(256), 0, st, src, R, k, F, mean, rstd,
                       beta, relu, max_out, ldmax, mean_out, ldmean, out2, ldout2, cnt_out, shift_of(F));
  }
  return dg::check_launch(what);
}

template <bool G>
int launch_bwd_reduce(const char* what, Src src, int64_t R, int k, int F, const float* mean, const float* rstd,
                      const float* beta, int relu, const float* dmax, int64_t lddmax, const float* dmean,
                      int64_t lddmean, const float* mx_in, int64_t ldmx, const float* cnt_in, double* red,
                      hipStream_t st) {
  DG_REQUIRE(mean && rstd && beta && dmax && red, DGCNN_EINVAL, "%s: null pointer", what);
  DG_REQUIRE(F <= 8192, DGCNN_EINVAL, "%s: F > 8192", what);
  DG_REQUIRE(!mx_in || cnt_in, DGCNN_EINVAL, "%s: mx_in needs cnt_in", what);
  DG_REQUIRE(relu == 0 || relu == 1, DGCNN_EINVAL, "%s: relu must be 0 or 1 (got %d; the bf16 flag belongs to the apply pass)", what, relu);
  const bool vec = (F % 4 == 0) && (lddmax % 4 == 0) && (G || a16(src.Y)) && a16(dmax) && a16(mean) && a16(rstd) &&
                   a16(beta) && (!dmean || ((lddmean % 4 == 0) && a16(dmean))) &&
                   (!mx_in || ((ldmx % 4 == 0) && a16(mx_in) && a16(cnt_in)));
  const size_t sh = (size_t)2 * F * sizeof(float);
  if (G) {
    DG_REQUIRE(vec, DGCNN_EINVAL, "%s: operands must be 16-byte aligned with leading dimensions %% 4 == 0", what);
    dg::launch((bn_bwd_reduce_kernel<4, true>), dim3(grid8(grid_reduce(R * (F / 4)))), dim3(256), sh, st, src, R, k,
                       F, mean, rstd, beta, relu, dmax, lddmax, dmean, lddmean, mx_in, ldmx, cnt_in, red, shift_of(F / 4), dg::stat_slots());
  } else if (vec && k == 1 && !mx_in) {          // k = 1: dz = dmax + dmean / 1 -- `dmean` is the gradient of a second copy of the output
    const int mb = 256;
    // the kernel ends with 2F double atomics per workgroup, which dominate above ~1 workgroup per CU
    // (F = 256: 19 us at 256 workgroups, 32 us at 2048; 1024-thread workgroups are slower: profiles/bn1_bench.py)
    const K1Grid g = k1_grid(R, F, mb);
    const size_t sh1 = sizeof(float) * K1_PARK_FLOATS;
    dg::launch((bn1_bwd_kernel<false>), g.grid, dim3(256), sh1, st, src.Y, R, F, g.FVB, g.RP, mean, rstd, beta, relu,
                       dmax, lddmax, dmean, lddmean, red, (float*)nullptr, (float*)nullptr, (int64_t)0, (const uint64_t*)nullptr, 1.0f,
                       dg::stat_slots());
  } else if (vec) {
    dg::launch((bn_bwd_reduce_kernel<4, false>), dim3(grid_reduce(R * (F / 4))), dim3(256), sh, st, src, R, k, F,
                       mean, rstd, beta, relu, dmax, lddmax, dmean, lddmean, mx_in, ldmx, cnt_in, red, shift_of(F / 4), dg::stat_slots());
  } else {
    dg::launch((bn_bwd_reduce_kernel<1, false>), dim3(grid_reduce(R * F)), dim3(256), sh, st, src, R, k, F, mean,
                       rstd, beta, relu, dmax, lddmax, dmean, lddmean, mx_in, ldmx, cnt_in, red, shift_of(F), dg::stat_slots());
  }
  return dg::check_launch(what);
}

template <bool G>
int launch_bwd_apply(const char* what, Src src, int64_t R, int k, int F, const float* mean, const float* rstd,
                     const float* beta, int relu, const float* dmax, int64_t lddmax, const float* dmean,
                     int64_t lddmean, const float* mx_in, int64_t ldmx, const float* cnt_in, double* red, float* dY,
                     float* dYsum, int64_t lddysum, float* dbeta, float dbeta_beta, hipStream_t st) {
  DG_REQUIRE(mean && rstd && beta && dmax && red && dY, DGCNN_EINVAL, "%s: null pointer", what);
  DG_REQUIRE(!dYsum || lddysum >= F, DGCNN_EINVAL, "%s: lddysum < F", what);
  DG_REQUIRE(relu >= 0 && relu <= 3, DGCNN_EINVAL, "%s: relu must be 0 .. 3 (bit 0 = ReLU, bit 1 = bf16 dY; got %d)", what, relu);
  dg::launch(bn_bwd_finalize_kernel, dim3((unsigned)dg::cdiv(F, FIN_COLS)), dim3(FIN_COLS * FIN_LANES), 0, st, red, F, dg::stat_slots(), dbeta,
                     dbeta_beta);
  const bool vec = (F % 4 == 0) && (lddmax % 4 == 0) && (G || a16(src.Y)) && a16(dY) && a16(dmax) && a16(mean) &&
                   a16(rstd) && a16(beta) && (!dmean || ((lddmean % 4 == 0) && a16(dmean))) &&
                   (!dYsum || (a16(dYsum) && lddysum % 4 == 0)) &&
                   (!mx_in || ((ldmx % 4 == 0) && a16(mx_in) && a16(cnt_in)));
  if (G) {
    DG_REQUIRE(vec, DGCNN_EINVAL, "%s: operands must be 16-byte aligned with leading dimensions %% 4 == 0", what);
    dg::launch((bn_bwd_apply_kernel<4, true>), dim3(grid8(grid_for(R * (F / 4)))), dim3(256), 0, st, src, R, k, F,
                       mean, rstd, beta, relu, dmax, lddmax, dmean, lddmean, mx_in, ldmx, cnt_in, red, dY, dYsum, lddysum,
                       shift_of(F / 4));
  } else if (vec && k == 1 && !mx_in && !(relu & 2)) {       // (the column-fixed kernel has no bf16 rounding: bit 1 takes the general one)
    const K1Grid g = k1_grid(R, F, 4096);
    dg::launch((bn1_bwd_kernel<true>), g.grid, dim3(256), 0, st, src.Y, R, F, g.FVB, g.RP, mean, rstd, beta, relu,
                       dmax, lddmax, dmean, lddmean, red, dY, dYsum, lddysum, (const uint64_t*)nullptr, 1.0f, dg::stat_slots());
  } else if (vec) {
    dg::launch((bn_bwd_apply_kernel<4, false>), dim3(grid_for(R * (F / 4))), dim3(256), 0, st, src, R, k, F, mean,
                       rstd, beta, relu, dmax, lddmax, dmean, lddmean, mx_in, ldmx, cnt_in, red, dY, dYsum, lddysum,
                       shift_of(F / 4));
  } else {
    dg::launch((bn_bwd_apply_kernel<1, false>), dim3(grid_for(R * F)), dim3(256), 0, st, src, R, k, F, mean, rstd,
                       beta, relu, dmax, lddmax, dmean, lddmean, mx_in, ldmx, cnt_in, red, dY, dYsum, lddysum, shift_of(F));
  }
  return dg::check_launch(what);
}

}  // namespace

extern "C" int dgcnn_bn_finalize_f32(const double* stats, int F, double count, float eps,
                                     float* mean, float* rstd, void* stream) {
  DG_REQUIRE(stats && mean && rstd && F > 0 && count > 0, DGCNN_EINVAL, "dgcnn_bn_finalize_f32: bad args");
  dg::launch(bn_finalize_kernel, dim3((unsigned)dg::cdiv(F, FIN_COLS)), dim3(FIN_COLS * FIN_LANES), 0, (hipStream_t)stream,
                     stats, F, dg::stat_slots(), count, eps, mean, rstd);
  return dg::check_launch("dgcnn_bn_finalize_f32");
}

extern "C" int dgcnn_bn_act_kreduce_f32(const float* Y, int64_t R, int k, int F,
                                        const float* mean, const float* rstd, const float* beta, int relu,
                                        float* max_out, int64_t ldmax, float* mean_out, int64_t ldmean,
                                        float* out2, int64_t ldout2, float* cnt_out, void* stream) {
  DG_REQUIRE(Y, DGCNN_EINVAL, "dgcnn_bn_act_kreduce_f32: null pointer");
  DG_REQUIRE(R > 0 && k > 0 && F > 0, DGCNN_EINVAL, "dgcnn_bn_act_kreduce_f32: bad shape");
  return launch_act_kreduce<false>("dgcnn_bn_act_kreduce_f32", dense_src(Y), R, k, F, mean, rstd, beta, relu, max_out,
                                   ldmax, mean_out, ldmean, out2, ldout2, cnt_out, (hipStream_t)stream);
}

extern "C" int dgcnn_bn_bwd_reduce_f32(const float* Y, int64_t R, int k, int F,
                                       const float* mean, const float* rstd, const float* beta, int relu,
                                       const float* dmax, int64_t lddmax, const float* dmean, int64_t lddmean,
                                       const float* mx_in, int64_t ldmx, const float* cnt_in,
                                       double* red, void* stream) {
  DG_REQUIRE(Y, DGCNN_EINVAL, "dgcnn_bn_bwd_reduce_f32: null pointer");
  DG_REQUIRE(R > 0 && k > 0 && F > 0, DGCNN_EINVAL, "dgcnn_bn_bwd_reduce_f32: bad shape");
  return launch_bwd_reduce<false>("dgcnn_bn_bwd_reduce_f32", dense_src(Y), R, k, F, mean, rstd, beta, relu, dmax, lddmax,
                                  dmean, lddmean, mx_in, ldmx, cnt_in, red, (hipStream_t)stream);
}

extern "C" int dgcnn_bn_bwd_apply_f32(const float* Y, int64_t R, int k, int F,
                                      const float* mean, const float* rstd, const float* beta, int relu,
                                      const float* dmax, int64_t lddmax, const float* dmean, int64_t lddmean,
                                      const float* mx_in, int64_t ldmx, const float* cnt_in,
                                      double* red, float* dY, float* dYsum, int64_t lddysum, float* dbeta,
                                      float dbeta_beta, void* stream) {
  DG_REQUIRE(Y, DGCNN_EINVAL, "dgcnn_bn_bwd_apply_f32: null pointer");
  DG_REQUIRE(R > 0 && k > 0 && F > 0, DGCNN_EINVAL, "dgcnn_bn_bwd_apply_f32: bad shape");
  return launch_bwd_apply<false>("dgcnn_bn_bwd_apply_f32", dense_src(Y), R, k, F, mean, rstd, beta, relu, dmax, lddmax,
                                 dmean, lddmean, mx_in, ldmx, cnt_in, red, dY, dYsum, lddysum, dbeta, dbeta_beta,
                                 (hipStream_t)stream);
}

// ---- the same three passes over the never-materialised conv0 output  y = V[neighbour] + U[point] ----
extern "C" int dgcnn_edge_bn_act_kreduce_f32(const float* V, int64_t ldv, const float* U, int64_t ldu,
                                             const int32_t* idx, int B, int N, int k, int F,
                                             const float* mean, const float* rstd, const float* beta, int relu,
                                             float* max_out, int64_t ldmax, float* mean_out, int64_t ldmean,
                                             float* cnt_out, void* stream) {
  int rc = check_edge("dgcnn_edge_bn_act_kreduce_f32", V, ldv, U, ldu, idx, B, N, k, F);
  if (rc) return rc;
  return launch_act_kreduce<true>("dgcnn_edge_bn_act_kreduce_f32", edge_src(V, ldv, U, ldu, idx, N), (int64_t)B * N, k, F,
                                  mean, rstd, beta, relu, max_out, ldmax, mean_out, ldmean, nullptr, 0, cnt_out,
                                  (hipStream_t)stream);
}

extern "C" int dgcnn_edge_bn_bwd_reduce_f32(const float* V, int64_t ldv, const float* U, int64_t ldu,
                                            const int32_t* idx, int B, int N, int k, int F,
                                            const float* mean, const float* rstd, const float* beta, int relu,
                                            const float* dmax, int64_t lddmax, const float* dmean, int64_t lddmean,
                                            const float* mx_in, int64_t ldmx, const float* cnt_in,
                                            double* red, void* stream) {
  int rc = check_edge("dgcnn_edge_bn_bwd_reduce_f32", V, ldv, U, ldu, idx, B, N, k, F);
  if (rc) return rc;
  return launch_bwd_reduce<true>("dgcnn_edge_bn_bwd_reduce_f32", edge_src(V, ldv, U, ldu, idx, N), (int64_t)B * N, k, F,
                                 mean, rstd, beta, relu, dmax, lddmax, dmean, lddmean, mx_in, ldmx, cnt_in, red,
                                 (hipStream_t)stream);
}

extern "C" int dgcnn_edge_bn_bwd_reduce_points_f32(const float* mx, int64_t ldmx, const float* mn, int64_t ldmn,
                                                   const float* cntpos, const float* dmax, int64_t lddmax,
                                                   const float* dmean, int64_t lddmean, const float* beta,
                                                   int64_t R, int k, int F, double* red, void* stream) {
  DG_REQUIRE(mx && mn && cntpos && dmax && dmean && beta && red, DGCNN_EINVAL, "dgcnn_edge_bn_bwd_reduce_points_f32: null pointer");
  DG_REQUIRE(R > 0 && k > 0 && k < CNT_POS && F > 0 && F % 4 == 0, DGCNN_EINVAL,
             "dgcnn_edge_bn_bwd_reduce_points_f32: bad shape (F %% 4 == 0, k < %d)", CNT_POS);
  DG_REQUIRE(a16(mx) && a16(mn) && a16(cntpos) && a16(dmax) && a16(dmean) && a16(beta) && ldmx % 4 == 0 && ldmn % 4 == 0 &&
                 lddmax % 4 == 0 && lddmean % 4 == 0, DGCNN_EINVAL,
             "dgcnn_edge_bn_bwd_reduce_points_f32: operands must be 16-byte aligned with leading dimensions %% 4 == 0");
  const K1Grid g = k1_grid(R, F, 256);
  const size_t sh = sizeof(float) * K1_PARK_FLOATS;
  dg::launch(edge_bwd_reduce_points_kernel, g.grid, dim3(256), sh, (hipStream_t)stream, mx, ldmx, mn, ldmn, cntpos,
                     dmax, lddmax, dmean, lddmean, beta, R, k, F, g.FVB, g.RP, red, dg::stat_slots());
  return dg::check_launch("dgcnn_edge_bn_bwd_reduce_points_f32");
}

extern "C" int dgcnn_edge_bn_bwd_apply_f32(const float* V, int64_t ldv, const float* U, int64_t ldu,
                                           const int32_t* idx, int B, int N, int k, int F,
                                           const float* mean, const float* rstd, const float* beta, int relu,
                                           const float* dmax, int64_t lddmax, const float* dmean, int64_t lddmean,
                                           const float* mx_in, int64_t ldmx, const float* cnt_in,
                                           double* red, float* dY, float* dYsum, int64_t lddysum, float* dbeta,
                                           float dbeta_beta, void* stream) {
  int rc = check_edge("dgcnn_edge_bn_bwd_apply_f32", V, ldv, U, ldu, idx, B, N, k, F);
  if (rc) return rc;
  return launch_bwd_apply<true>("dgcnn_edge_bn_bwd_apply_f32", edge_src(V, ldv, U, ldu, idx, N), (int64_t)B * N, k, F, mean,
                                rstd, beta, relu, dmax, lddmax, dmean, lddmean, mx_in, ldmx, cnt_in, red, dY, dYsum,
                                lddysum, dbeta, dbeta_beta, (hipStream_t)stream);
}

// ---- the last FC layer with tf.nn.dropout fused behind it (model.py:88-91): out = dropout(relu(bn(T))), and its backward
// reading the gradient of the dropped output through the same mask.  (R, F) contiguous, F % 4 == 0.
static int check_bn1_drop(const char* what, const float* T, int64_t R, int F, const float* mean, const float* rstd,
                          const float* beta, int relu, float keep, const uint64_t* seed_dev) {
  DG_REQUIRE(relu == 0 || relu == 1, DGCNN_EINVAL, "%s: relu must be 0 or 1 (got %d)", what, relu);
  DG_REQUIRE(T && mean && rstd && beta && seed_dev && R > 0 && F > 0 && keep > 0.f && keep <= 1.f, DGCNN_EINVAL, "%s: bad args", what);
  DG_REQUIRE(F % 4 == 0 && a16(T) && a16(mean) && a16(rstd) && a16(beta), DGCNN_EUNSUP, "%s: F %% 4 == 0 and 16-byte aligned operands required", what);
  return DGCNN_OK;
}

extern "C" int dgcnn_bn1_act_dropout_f32(const float* T, int64_t R, int F, const float* mean, const float* rstd,
                                         const float* beta, int relu, float keep, const uint64_t* seed_dev, float* out,
                                         int64_t ldo, void* stream) {
  int rc = check_bn1_drop("dgcnn_bn1_act_dropout_f32", T, R, F, mean, rstd, beta, relu, keep, seed_dev);
  if (rc) return rc;
  DG_REQUIRE(out && ldo % 4 == 0 && a16(out), DGCNN_EINVAL, "dgcnn_bn1_act_dropout_f32: out must be 16-byte aligned, ld %% 4 == 0");
  const K1Grid g = k1_grid(R, F, 4096);
  dg::launch(bn1_act_kernel, g.grid, dim3(256), 0, (hipStream_t)stream, T, R, F, g.FVB, g.RP, mean, rstd, beta, relu, out,
                     ldo, (float*)nullptr, (int64_t)0, (float*)nullptr, seed_dev, keep);
  return dg::check_launch("dgcnn_bn1_act_dropout_f32");
}

extern "C" int dgcnn_bn1_bwd_dropout_f32(const float* T, int64_t R, int F, const float* mean, const float* rstd,
                                         const float* beta, int relu, float keep, const uint64_t* seed_dev,
                                         const float* dout, int64_t lddo, double* red, float* dT, float* dbeta,
                                         float dbeta_beta, void* stream) {
  int rc = check_bn1_drop("dgcnn_bn1_bwd_dropout_f32", T, R, F, mean, rstd, beta, relu, keep, seed_dev);
  if (rc) return rc;
  DG_REQUIRE(dout && red && dT && lddo % 4 == 0 && a16(dout) && a16(dT) && F <= 8192, DGCNN_EINVAL, "dgcnn_bn1_bwd_dropout_f32: bad args");
  hipStream_t st = (hipStream_t)stream;
  const K1Grid gr = k1_grid(R, F, 256);
  const size_t sh1 = sizeof(float) * K1_PARK_FLOATS;
  dg::launch((bn1_bwd_kernel<false>), gr.grid, dim3(256), sh1, st, T, R, F, gr.FVB, gr.RP, mean, rstd, beta, relu, dout, lddo,
                     (const float*)nullptr, (int64_t)0, red, (float*)nullptr, (float*)nullptr, (int64_t)0, seed_dev, keep, dg::stat_slots());
  dg::launch(bn_bwd_finalize_kernel, dim3((unsigned)dg::cdiv(F, FIN_COLS)), dim3(FIN_COLS * FIN_LANES), 0, st, red, F, dg::stat_slots(), dbeta, dbeta_beta);
  const K1Grid ga = k1_grid(R, F, 4096);
  dg::launch((bn1_bwd_kernel<true>), ga.grid, dim3(256), 0, st, T, R, F, ga.FVB, ga.RP, mean, rstd, beta, relu, dout, lddo,
                     (const float*)nullptr, (int64_t)0, red, dT, (float*)nullptr, (int64_t)0, seed_dev, keep, dg::stat_slots());
  return dg::check_launch("dgcnn_bn1_bwd_dropout_f32");
}

// ---- the class-dimension tail: see bn1_act_class_kernel.  F = 256, NUM_CLASS <= 4, dense (R, F) / (R, ncls) tensors.
static int check_class_tail(const char* what, int F, int ncls, const float* W, int64_t ldw) {
  DG_REQUIRE(F == 256, DGCNN_EUNSUP, "%s: the last FC layer must be 256 wide (got %d): one wave per row", what, F);
  DG_REQUIRE(ncls >= 1 && ncls <= 4, DGCNN_EUNSUP, "%s: 1 .. 4 classes (got %d)", what, ncls);
  DG_REQUIRE(W && ldw >= ncls, DGCNN_EINVAL, "%s: bad class weight", what);
  return DGCNN_OK;
}

extern "C" int dgcnn_bn1_act_class_f32(const float* T, int64_t R, int F, const float* mean, const float* rstd,
                                       const float* beta, int relu, float keep, const uint64_t* seed_dev, float* out,
                                       int64_t ldo, const float* W, int64_t ldw, int ncls, float* logits, int64_t ldc,
                                       double* stats, float* scal, void* stream) {
  int rc = check_bn1_drop("dgcnn_bn1_act_class_f32", T, R, F, mean, rstd, beta, relu, keep, seed_dev);
  if (rc) return rc;
  rc = check_class_tail("dgcnn_bn1_act_class_f32", F, ncls, W, ldw);
  if (rc) return rc;
  DG_REQUIRE(out && ldo % 4 == 0 && ldo >= F && a16(out), DGCNN_EINVAL, "dgcnn_bn1_act_class_f32: out must be 16-byte aligned, ld %% 4 == 0");
  DG_REQUIRE(logits && ldc >= ncls && stats && R < (1ll << 31), DGCNN_EINVAL, "dgcnn_bn1_act_class_f32: bad logits / stats");
  // the grid of dgcnn_gemm_f32's streaming product for these rows: same rows per wave, same writers per statistics slot
  const unsigned g = (unsigned)dg::cap_writers(dg::cdiv(R, 4) < 2048 ? dg::cdiv(R, 4) : 2048);
  hipStream_t st = (hipStream_t)stream;
#define DG_ACT_CLASS(NN) dg::launch((bn1_act_class_kernel<NN>), dim3(g), dim3(256), 0, st, T, R, mean, rstd, beta, relu, out, ldo, \
                                    seed_dev, keep, W, ldw, logits, ldc, stats, dg::stat_slots(), scal)
  if (ncls == 1) DG_ACT_CLASS(1); else if (ncls == 2) DG_ACT_CLASS(2); else if (ncls == 3) DG_ACT_CLASS(3); else DG_ACT_CLASS(4);
#undef DG_ACT_CLASS
  return dg::check_launch("dgcnn_bn1_act_class_f32");
}

extern "C" int dgcnn_bn_softmax_xent_f32(const float* Y, const double* stats, double count, float eps, const float* beta,
                                         int relu, int64_t rows, int ncls, float* mean, float* rstd, float* fin,
                                         const int32_t* labels, const float* weight, float* softmax, float* dlogits,
                                         float* scal, void* stream) {
  DG_REQUIRE(Y && stats && beta && mean && rstd && fin && rows > 0 && count > 0, DGCNN_EINVAL, "dgcnn_bn_softmax_xent_f32: bad args");
  DG_REQUIRE(ncls >= 1 && ncls <= FIN_COLS, DGCNN_EUNSUP, "dgcnn_bn_softmax_xent_f32: 1 .. %d classes (got %d)", FIN_COLS, ncls);
  DG_REQUIRE(relu == 0 || relu == 1, DGCNN_EINVAL, "dgcnn_bn_softmax_xent_f32: relu must be 0 or 1 (got %d)", relu);
  DG_REQUIRE(!dlogits || labels, DGCNN_EINVAL, "dgcnn_bn_softmax_xent_f32: dlogits needs labels");
  int64_t g = dg::cdiv(rows, 256);                  // dgcnn_softmax_xent_f32's grid
  if (g > 1024) g = 1024;
  dg::launch(bn_softmax_xent_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, Y, stats, dg::stat_slots(), count, eps,
             beta, relu, rows, ncls, mean, rstd, fin, labels, weight, softmax, dlogits, scal);
  return dg::check_launch("dgcnn_bn_softmax_xent_f32");
}

extern "C" int dgcnn_bn1_bwd_class_f32(const float* T, int64_t R, int F, const float* mean, const float* rstd,
                                       const float* beta, int relu, float keep, const uint64_t* seed_dev, float* Tf, int ncls,
                                       const float* mean_f, const float* rstd_f, const float* beta_f, int relu_f,
                                       const float* dfin, double* red_f, float* dbeta_f, float dbeta_f_beta, const float* W,
                                       int64_t ldw, double* red, float* dT, float* dbeta, float dbeta_beta, int phases, void* stream) {
  DG_REQUIRE(phases >= 1 && phases <= 3, DGCNN_EINVAL, "dgcnn_bn1_bwd_class_f32: phases must be 1 (sums), 2 (finalize + dT) or 3 (got %d)", phases);
  int rc = check_bn1_drop("dgcnn_bn1_bwd_class_f32", T, R, F, mean, rstd, beta, relu, keep, seed_dev);
  if (rc) return rc;
  rc = check_class_tail("dgcnn_bn1_bwd_class_f32", F, ncls, W, ldw);
  if (rc) return rc;
  DG_REQUIRE(Tf && mean_f && rstd_f && beta_f && dfin && red_f && red && dT && a16(dT) && (relu_f == 0 || relu_f == 1), DGCNN_EINVAL,
             "dgcnn_bn1_bwd_class_f32: bad args");
  hipStream_t st = (hipStream_t)stream;
  const K1Grid gr = k1_grid(R, F, 256);
  const K1Grid ga = k1_grid(R, F, 4096);
  const size_t sh1 = sizeof(float) * K1_PARK_FLOATS;
  const int ns = dg::stat_slots();
#define DG_BWD_CLASS(NC)                                                                                                         \
  do {                                                                                                                           \
    if (phases & 1)                                                                                                              \
      dg::launch((bn1_bwd_class_kernel<false, NC>), gr.grid, dim3(256), sh1, st, T, R, mean, rstd, beta, relu, seed_dev, keep,    \
                 Tf, mean_f, rstd_f, beta_f, relu_f, dfin, red_f, ns, dbeta_f, dbeta_f_beta, W, ldw, red, (float*)nullptr, ns);   \
    if (!(phases & 2)) break;                                                                                                    \
    dg::launch(bn_bwd_finalize_kernel, dim3((unsigned)dg::cdiv(F, FIN_COLS)), dim3(FIN_COLS * FIN_LANES), 0, st, red, F, ns,     \
               dbeta, dbeta_beta);                                                                                               \
    dg::launch((bn1_bwd_class_kernel<true, NC>), ga.grid, dim3(256), 0, st, T, R, mean, rstd, beta, relu, seed_dev, keep, Tf,     \
               mean_f, rstd_f, beta_f, relu_f, dfin, red_f, ns, (float*)nullptr, 0.f, W, ldw, red, dT, ns);                       \
  } while (0)
  if (ncls == 1) DG_BWD_CLASS(1); else if (ncls == 2) DG_BWD_CLASS(2); else if (ncls == 3) DG_BWD_CLASS(3); else DG_BWD_CLASS(4);
#undef DG_BWD_CLASS
  return dg::check_launch("dgcnn_bn1_bwd_class_f32");
}

extern "C" int dgcnn_edge_valu(int on) {
  return dg::sw_set_or_query(dg::SW_EDGE_VALU, on >= 0, on ? 1 : 0);
}

namespace dg {
void launch_reduce_partials(const float* part, int splits, int M, int N, float* C, int64_t ldc, float beta, hipStream_t st);
// slots of a backward reduction -> slot 0 (+ d(beta)); edge_mlp_bf16.hip
void launch_bn_bwd_finalize(double* red, int F, float* dbeta, float dbeta_beta, hipStream_t st) {
  dg::launch(bn_bwd_finalize_kernel, dim3((unsigned)cdiv(F, FIN_COLS)), dim3(FIN_COLS * FIN_LANES), 0, st, red, F, stat_slots(), dbeta, dbeta_beta);
}
}

extern "C" int dgcnn_edge_bn_bwd_apply_wgrad_f32(const float* V, int64_t ldv, const float* U, int64_t ldu,
                                                 const int32_t* idx, int B, int N, int k, int F,
                                                 const float* mean, const float* rstd, const float* beta,
                                                 const float* dmax, int64_t lddmax, const float* dmean, int64_t lddmean,
                                                 const float* mx_in, int64_t ldmx, const float* cnt_in, double* red,
                                                 const float* x, int64_t ldx, int C, float* dW0, float* dbeta,
                                                 float dbeta_beta, void* ws, size_t ws_bytes, void* stream) {
  int rc = check_edge("dgcnn_edge_bn_bwd_apply_wgrad_f32", V, ldv, U, ldu, idx, B, N, k, F);
  if (rc) return rc;
  DG_REQUIRE(mean && rstd && beta && dmax && dmean && mx_in && cnt_in && red && x && dW0 && ws, DGCNN_EINVAL,
             "dgcnn_edge_bn_bwd_apply_wgrad_f32: null pointer");
  DG_REQUIRE(C >= 1 && C <= 4, DGCNN_EUNSUP, "dgcnn_edge_bn_bwd_apply_wgrad_f32: C must be <= 4 (got %d)", C);
  const int FV = F / 4;
  DG_REQUIRE(shift_of(FV) >= 0 && FV <= 256 && lddmax % 4 == 0 && lddmean % 4 == 0 && ldmx % 4 == 0 && a16(dmax) && a16(dmean) &&
                 a16(mx_in) && a16(cnt_in) && a16(mean) && a16(rstd) && a16(beta), DGCNN_EUNSUP,
             "dgcnn_edge_bn_bwd_apply_wgrad_f32: F / 4 must be a power of two <= 256, operands 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int64_t R = (int64_t)B * N;
  dg::launch(bn_bwd_finalize_kernel, dim3((unsigned)dg::cdiv(F, FIN_COLS)), dim3(FIN_COLS * FIN_LANES), 0, st, red, F, dg::stat_slots(), dbeta, dbeta_beta);
  const unsigned grid = grid8(grid_reduce(R * FV));                 // <= 1024 blocks: one partial tile each
  const size_t need = (size_t)grid * 2 * C * F * sizeof(float);
  DG_REQUIRE(ws_bytes >= need, DGCNN_ENOSPC, "dgcnn_edge_bn_bwd_apply_wgrad_f32: workspace too small (%zu < %zu)", ws_bytes, need);
  const size_t shb = (size_t)(256 / FV) * 2 * 4 * F * sizeof(float);
  // the exact-width form takes row offsets inside a cloud as unsigned 32-bit element counts from one 24-bit multiply: x must keep
  // row_offset24's contract as V does (check_edge); anything else keeps the run-time-C kernel and its 64-bit x offsets
  const bool exact = edge_valu_on() && (C == 3 || C == 4) && ldx >= C && row_offset24_ok(N, ldx);
  const Src src = edge_src(V, ldv, U, ldu, idx, N);
  float* part = reinterpret_cast<float*>(ws);
  if (exact && C == 3)
    dg::launch((edge_bwd_apply_wgrad_exact_kernel<3>), dim3(grid), dim3(256), shb / 4 * 3, st, src, R, k, F, mean, rstd, beta, dmax,
               lddmax, dmean, lddmean, mx_in, ldmx, cnt_in, red, x, ldx, part, shift_of(FV));
  else if (exact)
    dg::launch((edge_bwd_apply_wgrad_exact_kernel<4>), dim3(grid), dim3(256), shb, st, src, R, k, F, mean, rstd, beta, dmax,
               lddmax, dmean, lddmean, mx_in, ldmx, cnt_in, red, x, ldx, part, shift_of(FV));
  else
    dg::launch((edge_bwd_apply_wgrad_kernel<4>), dim3(grid), dim3(256), shb, st, src, R, k, F, mean, rstd, beta, dmax, lddmax,
               dmean, lddmean, mx_in, ldmx, cnt_in, red, x, ldx, C, part, shift_of(FV));
  rc = dg::check_launch("dgcnn_edge_bn_bwd_apply_wgrad_f32");
  if (rc) return rc;
  dg::launch_reduce_partials(reinterpret_cast<const float*>(ws), (int)grid, 2 * C, F, dW0, (int64_t)F, 1.0f, st);
  return dg::check_launch("dgcnn_edge_bn_bwd_apply_wgrad_f32(reduce)");
}

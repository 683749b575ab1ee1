// knn.hip -- K1: fused pairwise squared distance + per-row top-k select (dgcnn/ops.py:8-19).
//
// MUST be compiled with -ffp-contract=off: the arithmetic order is normative
// (oracle/knn_oracle.c) and the indices are bit-exact against it:
//     s_i  = sequential sum of fl(x*x)          (no FMA)
//     p_ij = fmaf chain over c ascending from +0
//     D_ij = fl( fl(s_i + s_j) - 2 p_ij )
// Selection: k smallest by (D_ij, j) lexicographic, ascending, self included.
//
// Mapping (wave64): a workgroup owns 64 query rows (one per lane, x_i in VGPRs) and 4 waves that
// split every 128-candidate LDS tile four ways, so B*N/64*4 waves are in flight (3072 at the
// headline shape).  All lanes of a wave read the same candidate row from LDS (broadcast, no bank
// conflicts); each lane keeps a private sorted (d, j) list of KC entries in registers and inserts
// with a branch-free v_med3/v_cndmask network, skipped wave-uniformly when no lane improves.
// The four per-wave lists are merged through LDS at the end.  The (B,N,N) matrix never exists.
#include "knn_scan.h"
#include <type_traits>
#include <stdlib.h>

namespace {

constexpr int WAVES = 4;
constexpr int TJ = 128;
constexpr int PERW = TJ / WAVES;

// s_i = sequential sum of fl(x^2) over c ascending (the oracle's order: no FMA, no reassociation), one thread per row.
// 64 rows per block (B*N/64 blocks: 768 at the headline shape -- the round-1 kernel ran 192 blocks of 256 rows, under one
// block per CU, 24 us at C = 64): the block's rows are staged through LDS with coalesced loads (a thread walking its own
// 256-byte row in global memory touches 64 cache lines per wave-load), then 64 threads walk one row each, stride C + 1.
constexpr int SQ_ROWS = 64;
__global__ __launch_bounds__(256) void sqnorm_kernel(const float* __restrict__ x, int64_t ldx, int64_t rows, int C,
                                                     float* __restrict__ sq) {
  extern __shared__ float sq_tile[];          // [64][C + 1]
  const int64_t r0 = (int64_t)blockIdx.x * SQ_ROWS;
  const int t = threadIdx.x;
  const int S = C + 1;
  for (int e = t; e < SQ_ROWS * C; e += 256) {
    const int rr = e / C, cc = e - rr * C;
    if (r0 + rr < rows) sq_tile[rr * S + cc] = x[(r0 + rr) * ldx + cc];
  }
  __syncthreads();
  if (t < SQ_ROWS && r0 + t < rows) {
    float s = 0.0f;
    for (int c = 0; c < C; ++c) {
      const float v = sq_tile[t * S + c];
      const float q = v * v;
      s = s + q;
    }
    sq[r0 + t] = s;
  }
}


// ------------------------------------------------------------------------------------------------
// A bound for the raw-coordinate layer (C <= 4, no previous graph to seed from; round 6).  One thread per query row counts the
// cloud's candidates (every STRIDE-th: k of a SAMPLE within t still puts the row's k-th distance below t) into half-octave bins of the
// NORMATIVE distance -- bin = (float bits of max(d, 0)) >> 22, i.e. exponent and leading mantissa bit, taken relative to the cloud's
// largest possible distance so that 48 bins span 24 octaves of d whatever the cloud's scale -- and reports the upper edge of the first
// bin at which the count reaches k.  The scan then drops every candidate at or above that edge before it reaches the sorted lists:
// ~1.3 k candidates pass per row instead of ~k (1 + ln(N / k)) per LIST (four lists per row), and the sorted inserts were three
// quarters of the scan's instructions (r05_pmc_sq.txt).  Rigorous for any input: a candidate dropped has k candidates strictly below it;
// a coarse bin (many equal distances) only makes the bound looser; a NaN distance (+inf in the selection's order) and +inf are counted
// in the top bin, under no edge.  Per candidate: one LDS broadcast read, the 6-operation distance,
// clamp, shift, one ds_add_u32 into the thread's own column of the histogram ([bin][thread]: bank = thread, conflict free).
constexpr int HB_NB = 48;
template <int STRIDE, class Clouds = DenseClouds>
__global__ __launch_bounds__(256) void knn_hist_bound_kernel(const float* __restrict__ x, const float* __restrict__ sq, Clouds cl, int C,
                                                             int64_t ldx, int k, float* __restrict__ tau0) {
  // 64 query rows per workgroup (lane = row); wave w counts quarter w of every 256-candidate tile into its own histogram
  // ([wave][bin][lane]: bank = lane), the four are added at the end -- 3072 waves at (24,2048) instead of 768: the per-candidate chain
  // (two LDS broadcast reads -> distance -> bin -> ds_add) is latency bound with one wave per SIMD (125 us; 4 waves per row: see
  // profiles/r06/knn_hist.txt)
  __shared__ unsigned hist[4 * HB_NB * 64];
  __shared__ float4 tile[256];                          // the sampled candidates' coordinates (zero padded to 4)
  __shared__ float ts[256];                             // ... and their s_j
  __shared__ float wmax[4];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int b = blockIdx.y;
  const int N = cl.size(b);
  if (Clouds::kPacked && (int)blockIdx.x * 64 >= N) return;
  const int64_t cb = cl.base(b);
  const int row = blockIdx.x * 64 + lane;
  const float* xb = x + cb * ldx;
  const float* sqb = sq + cb;
  const int rowc = row < N ? row : N - 1;
  float xi[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) xi[c] = (c < C) ? xb[(int64_t)rowc * ldx + c] : 0.0f;
  const float si = sqb[rowc];
  unsigned* myh = hist + w * HB_NB * 64 + lane;
#pragma unroll
  for (int q = 0; q < HB_NB; ++q) myh[q * 64] = 0u;
  // the cloud's largest s_j bounds every distance: d <= 2 (s_i + s_j) <= 4 max s (4.5: room for the roundings of d)
  float m = 0.f;
  for (int j = tid; j < N; j += 256) m = fmaxf(m, sqb[j]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if (lane == 0) wmax[w] = m;
  __syncthreads();
  m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
  const int raw_top = (int)(__float_as_uint(4.5f * m) >> 22);
  const int bin0 = raw_top - (HB_NB - 1);
  const int ns = (N + STRIDE - 1) / STRIDE;            // sampled candidates j = STRIDE u, u < ns
#pragma unroll 1
  for (int u0 = 0; u0 < ns; u0 += 256) {
    __syncthreads();
    if (u0 + tid < ns) {
      const int64_t j = (int64_t)(u0 + tid) * STRIDE;
      const float* src = xb + j * ldx;
      tile[tid] = make_float4(src[0], (C > 1) ? src[1] : 0.f, (C > 2) ? src[2] : 0.f, (C > 3) ? src[3] : 0.f);
      ts[tid] = sqb[j];
    }
    __syncthreads();
    const int lo = 64 * w;
    const int hi = (ns - u0 < lo + 64) ? ns - u0 : lo + 64;
    // the scan's arithmetic, operation for operation (knn_kernel<4, KC>): a candidate counted below an edge here IS below it there
    auto bin_of = [&](const float4& v, float sj) -> int {
      float p = 0.f;
      p = fmaf(xi[0], v.x, p);
      p = fmaf(xi[1], v.y, p);
      p = fmaf(xi[2], v.z, p);
      p = fmaf(xi[3], v.w, p);
      const float tt = si + sj;
      const float tp = 2.0f * p;
      const float dn = tt - tp;
      const float d = fmaxf(dn, 0.0f);
      const int bin = (int)(__float_as_uint(d) >> 22) - bin0;
      // a NaN distance counts as +inf (fmaxf has made it 0): the top bin, which has no edge -- below an edge it would be counted as
      // one of the k that the edge's bound rests on, and the scan never lists it
      return (dn != dn) ? HB_NB - 1 : (bin < 0 ? 0 : (bin > HB_NB - 1 ? HB_NB - 1 : bin));
    };
    int t = lo;
    // groups of 8: all LDS reads of a group first, then the arithmetic, then the 8 adds (hipcc will not move a read across a
    // ds_add that may alias it: candidate by candidate the loop was one LDS round trip per candidate)
    for (; t + 8 <= hi; t += 8) {
      float4 v[8];
      float sj[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) { v[q] = tile[t + q]; sj[q] = ts[t + q]; }
      int bn[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) bn[q] = bin_of(v[q], sj[q]);
#pragma unroll
      for (int q = 0; q < 8; ++q) atomicAdd(&myh[bn[q] * 64], 1u);
    }
    for (; t < hi; ++t) atomicAdd(&myh[bin_of(tile[t], ts[t]) * 64], 1u);
  }
  __syncthreads();
  if (w != 0) return;
  // first bin at which the count reaches k; its upper edge bounds the row's k-th distance (the top bin has none: +inf)
  unsigned cum = 0u;
  int bsel = HB_NB - 1;
#pragma unroll 1
  for (int q = 0; q < HB_NB; ++q) {
    cum += hist[q * 64 + lane] + hist[(HB_NB + q) * 64 + lane] + hist[(2 * HB_NB + q) * 64 + lane] + hist[(3 * HB_NB + q) * 64 + lane];
    if (cum >= (unsigned)k) { bsel = q; break; }
  }
  float tau = INFINITY;
  const int eraw = bin0 + bsel + 1;
  if (bsel < HB_NB - 1 && eraw > 0 && eraw < 0x1FE) tau = __uint_as_float((unsigned)eraw << 22);
  if (row < N) tau0[cb + row] = tau;
}

// Register budget: x_i (CP) + list (2*KC) + ~70 for the candidate stream -> waves/SIMD target.
template <int CP, int KC>
constexpr int knn_min_waves() {
  return (CP + 2 * KC + 70 <= 128) ? 4 : ((CP + 2 * KC + 70 <= 168) ? 3 : ((CP + 2 * KC + 70 <= 256) ? 2 : 1));
}

template <int CP, int KC, class Clouds = DenseClouds>
__global__ __launch_bounds__(256, (knn_min_waves<CP, KC>())) void knn_kernel(const float* __restrict__ x,
                                                                            const float* __restrict__ sq, Clouds cl, int C,
                                                                            int64_t ldx, int k, int vec_ok,
                                                                            int32_t* __restrict__ idx, const float* __restrict__ tau0) {
  constexpr int TILE_F = TJ * CP;
  constexpr int DQ_F = PERW * 256;           // per-lane distance slots of the current 32 candidates
  constexpr int MERGE_F = ROWS * KC * 2;
  constexpr int SH = (TILE_F + DQ_F > MERGE_F ? TILE_F + DQ_F : MERGE_F);
  __shared__ __attribute__((aligned(16))) float smem[SH + TJ + WAVES * ROWS];
  float* xs = smem;
  float* dq = smem + TILE_F;
  float* sjs = smem + SH;
  volatile float* thrw = smem + SH + TJ;     // [4 lists = waves][64 rows]: list[KC/4 - 1] so far

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int b = blockIdx.y;
  const int N = cl.size(b);
  if (Clouds::kPacked && (int)blockIdx.x * ROWS >= N) return;
  const int64_t cb = cl.base(b);
  const int row = blockIdx.x * ROWS + lane;
  const float* xb = x + cb * ldx;
  const float* sqb = sq + cb;

  const int rowc = row < N ? row : N - 1;
  float xi[CP];
#pragma unroll
  for (int c = 0; c < CP; ++c) xi[c] = (c < C) ? xb[(int64_t)rowc * ldx + c] : 0.0f;
  const float si = sqb[rowc];
  // a bound known in advance (knn_hist_bound_kernel: the row's k-th distance is < tau_row): candidates at or above it never enter
  const float tau_row = tau0 ? tau0[cb + rowc] : INFINITY;

  float dl[KC];
  int jl[KC];
  list_init<KC>(dl, jl);

  thrw[tid] = INFINITY;
#pragma unroll 1
  for (int j0 = 0; j0 < N; j0 += TJ) {
    __syncthreads();
    // ---- stage TJ candidate rows (zero padded to CP channels) into LDS ----
    for (int e = tid; e < TJ * (CP / 4); e += 256) {
      const int r = e / (CP / 4);
      const int c4 = (e % (CP / 4)) * 4;
      const int j = j0 + r;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (j < N) {
        const float* src = xb + (int64_t)j * ldx + c4;
        if (vec_ok && c4 + 3 < C) {
          v = *reinterpret_cast<const float4*>(src);
        } else {
          if (c4 + 0 < C) v.x = src[0];
          if (c4 + 1 < C) v.y = src[1];
          if (c4 + 2 < C) v.z = src[2];
          if (c4 + 3 < C) v.w = src[3];
        }
      }
      *reinterpret_cast<float4*>(&xs[r * CP + c4]) = v;
    }
    if (tid < TJ) {
      const int j = j0 + tid;
      sjs[tid] = (j < N) ? sqb[j] : INFINITY;
    }
    __syncthreads();
    if (j0 + w * PERW >= N) continue;        // wave-uniform: nothing for this wave in the tile

    // ---- phase A: distances of this wave's 32 candidates (2 independent fmaf chains at a time;
    // the channel loop is fully unrolled so x_i stays in registers, fenced every 16 channels so
    // the scheduler cannot hoist every LDS read).  Each lane parks d in its LDS slot and keeps a
    // 32-bit mask of the candidates that beat its current k-th distance. ----
    const float thr = fminf(dl[KC - 1], tau_row);
    unsigned mask = 0u;
#pragma unroll 1
    for (int g = 0; g < PERW; g += 2) {
      const int jl0 = w * PERW + g;
      const float* c0 = &xs[jl0 * CP];
      float p0 = 0.f, p1 = 0.f;
#pragma unroll
      for (int c = 0; c < CP; c += 4) {
        const float4 v0 = *reinterpret_cast<const float4*>(c0 + c);
        const float4 v1 = *reinterpret_cast<const float4*>(c0 + CP + c);
        p0 = fmaf(xi[c], v0.x, p0); p1 = fmaf(xi[c], v1.x, p1);
        p0 = fmaf(xi[c + 1], v0.y, p0); p1 = fmaf(xi[c + 1], v1.y, p1);
        p0 = fmaf(xi[c + 2], v0.z, p0); p1 = fmaf(xi[c + 2], v1.z, p1);
        p0 = fmaf(xi[c + 3], v0.w, p0); p1 = fmaf(xi[c + 3], v1.w, p1);
        if ((c & 15) == 12) __builtin_amdgcn_sched_barrier(0);
      }
      const float t0 = si + sjs[jl0], t1 = si + sjs[jl0 + 1];
      const float tp0 = 2.0f * p0, tp1 = 2.0f * p1;
      const float d0 = t0 - tp0, d1 = t1 - tp1;
      dq[g * 256 + tid] = d0;
      dq[(g + 1) * 256 + tid] = d1;
      mask |= (unsigned)sel_i(m_flt(d0, thr), (int)(1u << g), 0);
      mask |= (unsigned)sel_i(m_flt(d1, thr), (int)(2u << g), 0);
    }
    // ---- phase B: drain.  Every iteration each lane pops ITS lowest surviving candidate (ascending
    // j, which the tie rule needs) and all lanes run one insert: max-over-lanes(popcount) inserts
    // per 32 candidates instead of one per candidate with any taker. ----
    while (__any(mask != 0u)) {
      const lmask_t live = m_ine((int)mask, 0);
      const int g = sel_i(live, __builtin_ctz(mask | 0x80000000u), 0);
      const float d = sel_f(live, dq[g * 256 + tid], INFINITY);
      mask &= mask - 1u;
      list_insert<KC, false>(dl, jl, d, j0 + w * PERW + g);
    }
  }

  // ---- the 4 per-wave lists into wave 0 ----
  merge_lists_write<KC, Clouds::kPacked>(smem, dl, jl, w, lane, w == 0, true, row < N, idx, cb + row, k, N, (int)cb);
}

// ------------------------------------------------------------------------------------------------
// MFMA variant for feature-space graphs (C > 4): the inner products p_ij come from
// v_mfma_f32_32x32x2_f32, which on gfx950 is bit-for-bit an fmaf chain in k order (one rounding per
// product, no wider accumulation; MI355X_MICROARCH.md "Matrix cores"): feeding c = 2s, 2s+1 at step
// s reproduces the normative chain exactly -- the bit-exact tests against oracle/knn_oracle.c run on
// this kernel.  The matrix pipe does the 2*N^2*C flops; the VALU is left for the selection.
//   A operand = candidates (k-major LDS tile [c][cand], one conflict-free ds_read_b32 per step),
//   B operand = this wave's 32 query rows, resident in CP/2 VGPRs for the whole kernel.
//   D layout: lane l holds query row (l & 31) and candidates (r&3) + 8(r>>2) + 4(l>>5), r = 0..15:
//   two lanes per row, each with its own register-resident sorted list over its candidate subset.
// Block = 64 query rows x 2 candidate halves (4 waves); 64-candidate LDS tiles, double buffered, next
// tile prefetched into registers under the MFMAs; 4 lists per row merged through LDS.
// This kernel keeps its own text of what knn_scan.h holds for the other scans (ScanLane, load_row_quad, shared_bound, park_and_flag,
// drain_parked, merge_lists_write: the same code, and the arguments written there hold here).  Calling the shared functions left every
// resource figure as it was, yet the KC = 40 and KC = 64 instances (256 VGPRs, scratch at two waves) ran 4.5 % and 5.3 % slower at
// (24, 2048, 64), whichever of the calls was taken back (profiles/knn_scan_shared.txt); with this text the assembly is the parent's.
template <int CP, int KC, bool VEC>
__global__ __launch_bounds__(256, (KC <= 20 ? 3 : 2)) void knn_mfma_kernel(const float* __restrict__ x, const float* __restrict__ sq,
                                                                           int N, int C, int64_t ldx, int k,
                                                                           int32_t* __restrict__ idx, const float* __restrict__ tau0) {
  using f32x16 = __attribute__((ext_vector_type(16))) float;
  constexpr int TJM = 64;                    // candidates per LDS tile: 32 per candidate-half wave
  constexpr int ST = TJM + 2;                // k-major candidate tile [CP][ST]
  constexpr int TILE_F = CP * ST;
  constexpr int DQ_F = 16 * 256;
  constexpr int MERGE_F = ROWS * KC * 2;
  constexpr int WORK_F = 2 * TILE_F + DQ_F + 2 * TJM + 4 * ROWS;
  constexpr int SH = (WORK_F > MERGE_F ? WORK_F : MERGE_F);
  constexpr int NV = (TJM * (CP / 4)) / 256;  // float4 staged per thread per tile
  static_assert(NV >= 1, "tile too small");
  __shared__ __attribute__((aligned(16))) float smem[SH];
  float* dq = smem + 2 * TILE_F;
  float* sjs = smem + 2 * TILE_F + DQ_F;     // [2][TJM]
  volatile float* thrw = smem + 2 * TILE_F + DQ_F + 2 * TJM;   // [4 lists][64 rows]: list[KC/4 - 1] so far

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int qg = w & 1;                      // which 32 query rows of the block
  const int cs = w >> 1;                     // which 32 candidates of every 64-candidate tile
  const int b = blockIdx.y;
  const int row = blockIdx.x * ROWS + qg * 32 + l31;
  const float* xb = x + (int64_t)b * N * ldx;
  const float* sqb = sq + (int64_t)b * N;
  const int rowc = row < N ? row : N - 1;

  float bq[CP / 2];                          // B operand: x_q[row][2s + h]
#pragma unroll
  for (int s2 = 0; s2 < CP / 2; ++s2) {
    const int c = 2 * s2 + h;
    bq[s2] = (c < C) ? xb[(int64_t)rowc * ldx + c] : 0.0f;
  }
  const float si = sqb[rowc];
  // seed bound (dgcnn_knn_seeded_f32): tau0 = the largest distance to k DISTINCT candidates, so the row's k-th distance is <= tau0
  // and a candidate with d > tau0 can never enter its top k (d == tau0 passes: ties are decided by index in the merge)
  const float t0 = tau0 ? next_up(tau0[(int64_t)b * N + rowc]) : INFINITY;

  float dl[KC];
  int jl[KC];
#pragma unroll
  for (int t = 0; t < KC; ++t) {
    dl[t] = INFINITY;
    jl[t] = 0x7fffffff;
  }

  // ---- candidate tiles: global -> registers one tile ahead, transposed ([c][cand]) into the other
  // LDS buffer after the current tile's MFMAs; one barrier per tile ----
  // VEC (16-byte aligned rows, C % 4 == 0): one unconditional float4 load per piece from a clamped, always valid address;
  // rows past N carry |x_j|^2 = +inf (their distance is +inf: never selected), channel quads past C are zeroed.
  float4 pre[NV];
  float pre_s = INFINITY;
  auto fetch = [&](int j0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int e = tid + 256 * i;
      const int r = e / (CP / 4);
      const int c4 = (e % (CP / 4)) * 4;
      const int j = j0 + r;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (VEC) {
        const int jc = j < N ? j : N - 1;
        const int cc = c4 < C ? c4 : C - 4;
        const float4 t4 = *reinterpret_cast<const float4*>(xb + (int64_t)jc * ldx + cc);
        const bool ok = c4 < C;
        v.x = ok ? t4.x : 0.f; v.y = ok ? t4.y : 0.f; v.z = ok ? t4.z : 0.f; v.w = ok ? t4.w : 0.f;
      } else if (j < N) {
        const float* src = xb + (int64_t)j * ldx + c4;
        if (c4 + 0 < C) v.x = src[0];
        if (c4 + 1 < C) v.y = src[1];
        if (c4 + 2 < C) v.z = src[2];
        if (c4 + 3 < C) v.w = src[3];
      }
      pre[i] = v;
    }
    if (tid < TJM) pre_s = (j0 + tid < N) ? sqb[j0 + tid] : INFINITY;
  };
  auto stash = [&](int buf) {
    float* d = smem + buf * TILE_F;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int e = tid + 256 * i;
      const int r = e / (CP / 4);
      const int c4 = (e % (CP / 4)) * 4;
      d[(c4 + 0) * ST + r] = pre[i].x;
      d[(c4 + 1) * ST + r] = pre[i].y;
      d[(c4 + 2) * ST + r] = pre[i].z;
      d[(c4 + 3) * ST + r] = pre[i].w;
    }
    if (tid < TJM) sjs[buf * TJM + tid] = pre_s;
  };

  const int nt = (N + TJM - 1) / TJM;
  fetch(0);
  stash(0);
  thrw[tid] = INFINITY;
  const int lid = (w >> 1) * 2 + h;          // list id of this lane among the 4 lists of its row (= `me` below)
  const int rslot = (w & 1) * 32 + l31;      // row within the block
  __syncthreads();

#pragma unroll 1
  for (int t = 0; t < nt; ++t) {
    const int buf = t & 1;
    const int j0 = t * TJM;
    thrw[lid * ROWS + rslot] = dl[KC / 4 - 1];       // publish this list's KC/4-th entry (as of the previous tile)
    if (t + 1 < nt) fetch(j0 + TJM);
    const int cbase = cs * 32;
    if (j0 + cbase < N) {                    // wave-uniform
      const float* xsT = smem + buf * TILE_F;
      // the other three lists' KC/4-th entries (shared selection bound): requested before the chain, needed after it
      const float o1 = thrw[(lid ^ 1) * ROWS + rslot], o2 = thrw[(lid ^ 2) * ROWS + rslot], o3 = thrw[(lid ^ 3) * ROWS + rslot];
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      const float* ap = xsT + h * ST + cbase + l31;
      {
        // A operand ring, two MFMAs deep: the operand of step s + 2 is requested right behind MFMA s, whose 64 clocks in
        // the pipe (the chain is dependent) cover the LDS round trip.  (Round 1 staged 8 + 8 operands: 12 registers more.)
        constexpr int NS = CP / 2;
        float a0 = ap[0], a1 = ap[2 * ST];
#pragma unroll
        for (int s2 = 0; s2 < NS; s2 += 2) {
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bq[s2], acc, 0, 0, 0);
          if (s2 + 2 < NS) a0 = ap[2 * (s2 + 2) * ST];
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bq[s2 + 1], acc, 0, 0, 0);
          if (s2 + 3 < NS) a1 = ap[2 * (s2 + 3) * ST];
        }
      }

      // ---- distances of this lane's 16 candidates; park them, flag the ones that can still enter the row's top KC ----
      const float thr = fminf(fminf(dl[KC - 1], t0), next_up(fmaxf(fmaxf(dl[KC / 4 - 1], o1), fmaxf(o2, o3))));
      const float* sj = sjs + buf * TJM + cbase + 4 * h;
      unsigned mask = 0u;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 s4 = *reinterpret_cast<const float4*>(sj + 8 * q);     // candidates 8 q + 4 h + (0..3)
        const float sv[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * q + e;
          const float tt = si + sv[e];
          // (tt - 2 p in ONE rounding: 2 p is exact, so the fused form equals the oracle's  tt - fl(2 p)  bit for bit)
          const float d = __builtin_fmaf(-2.0f, acc[r], tt);
          dq[r * 256 + tid] = d;
          mask |= sel_01(m_flt(d, thr)) << r;
        }
      }
      // drain: the parked distance of the NEXT surviving candidate is fetched before the insert of
      // the current one (LDS round trip hidden behind ~90 VALU ops)
      int g = __builtin_ctz(mask | 0x80000000u) & 15;
      float dcur = dq[g * 256 + tid];
      while (__any(mask != 0u)) {
        const lmask_t live = m_ine((int)mask, 0);
        const int gc = g;
        mask &= mask - 1u;
        g = __builtin_ctz(mask | 0x80000000u) & 15;
        const float dnext = dq[g * 256 + tid];
        const float d = sel_f(live, dcur, INFINITY);
        const int i = (gc & 3) + 8 * (gc >> 2) + 4 * h;
        list_insert<KC, false>(dl, jl, d, j0 + cbase + i);
        dcur = dnext;
      }

    }
    if (t + 1 < nt) stash(buf ^ 1);
    __syncthreads();
  }

  // ---- merge: 4 lists per query row (2 lane halves x 2 candidate halves) -> lanes 0..31 of waves 0,1 ----
  __syncthreads();
  float* md = smem;
  int* mj = reinterpret_cast<int*>(smem + ROWS * KC);
  const int me = cs * 2 + h;                 // list id of this lane; id 0 is the destination
  const int slot = qg * 32 + l31;            // row within the block
#pragma unroll 1
  for (int src = 1; src < 4; ++src) {
    if (src > 1) __syncthreads();
    if (me == src) {
#pragma unroll
      for (int t = 0; t < KC; ++t) {
        md[t * ROWS + slot] = dl[t];
        mj[t * ROWS + slot] = jl[t];
      }
    }
    __syncthreads();
    if (cs == 0) {                           // wave-uniform; lanes with h == 1 idle along (d = +inf)
#pragma unroll 1
      for (int t = 0; t < KC; ++t) {
        const float d = (h == 0) ? md[t * ROWS + slot] : INFINITY;
        const int j = (h == 0) ? mj[t * ROWS + slot] : 0x7fffffff;
        const lmask_t need = key_less<true>(d, j, dl[KC - 1], jl[KC - 1]);
        if (need == 0) break;
        list_insert<KC, true>(dl, jl, d, j);
      }
    }
  }
  if (me == 0 && row < N) {
    int32_t* out = idx + ((int64_t)b * N + row) * k;
#pragma unroll
    for (int t = 0; t < KC; ++t)
      if (t < k) out[t] = jl[t];
    fill_short_list<KC>(jl, k, N, 0, out);                                  // fewer than k candidates below +inf (knn_common.h)
  }
}

// ------------------------------------------------------------------------------------------------
// Large-N kernel (C = 64 feature graphs, N >= 8192): distances on the BF16 matrix pipe, exact fp32 only for the survivors.
//
// At N = 65536 the fp32 MFMA chain is ~80 % of the kernel above (almost nothing survives the filter), and on gfx950
// v_mfma_f32_32x32x2_f32 runs at the vector rate and blocks the vector pipe.  Here every 32 x 32 tile of inner products is
// computed APPROXIMATELY from the two leading bf16 terms of each operand (x = x1 + x2 + x3 exactly; products x1y1 + x1y2 +
// x2y1 on v_mfma_f32_32x32x16_bf16: 12 instructions of 32 clocks per tile instead of 32 of 64), with a rigorous bound:
//     |p' - P| <= 3.25 * 2^-16 * sum|x_c y_c|   (dropped terms x2y2, x3 y, (x1+x2) y3 and the fp32 accumulation)
//     |p  - P| <= C * 2^-24 * sum|x_c y_c|      (the oracle's fmaf chain p; P = exact inner product)
//  => |d' - d| <= 2 |p' - p| + 2^-22 t  <  2^-14 t,   t = fl(s_i + s_j)   (sum|xy| <= (S_i + S_j)/2; d, d' share t)
// (reached: 1.86 * 2^-16 t on the true neighbours of the `rounddown` clouds of tests/knn_adversarial.py, float64 model of the products)
// A candidate can enter the list only if d < thr, hence only if d' < thr + eps with eps = 2^-13 t (2x margin).  For those
// (and only those) the NORMATIVE distance is recomputed on the VALU -- fmaf chain over c ascending from +0, x_i and x_j from
// fp32 LDS copies of the block's query rows and of the current candidate tile (a first version read x_j from global memory:
// 60 ms at (8,65536,64,20) against 9.8 ms without any re-check -- the re-check is latency, not work) -- and goes through the
// exact filter and the same insert as everywhere else.  Indices are therefore bit-identical to the oracle's; the tests that pin knn_mfma_kernel
// pin this kernel too (N = 16384 / 65536 compares, and every small-N case with the kernel forced on).
// No parking area: a survivor is identified by its mask bit, its distance is recomputed anyway.
template <int KC>
struct Bf16fCfg {
  static constexpr int OCC = (KC <= 20) ? 3 : 2;
};

template <int KC>
__global__ __launch_bounds__(256, (Bf16fCfg<KC>::OCC)) void knn_bf16f_kernel(const float* __restrict__ x, const float* __restrict__ sq,
                                                                            int N, int C, int64_t ldx, int k,
                                                                            int32_t* __restrict__ idx, const float* __restrict__ tau0) {
  constexpr int CP = 64;
  constexpr int TJM = 64;
  constexpr unsigned CS = TJM * 16 + 16;     // bytes per 8-channel chunk of one bf16 plane: [cand][8 bf16], padded (bank shift of 4)
  constexpr unsigned PB = 8 * CS;            // bytes per plane (8 chunks = 64 channels)
  constexpr unsigned TILE_B = 2 * PB;        // two planes (single buffer: the MFMA phase of a tile is short, other blocks of the CU fill the refill)
  constexpr int RS = CP + 4;                 // fp32 row stride of the two re-check tiles: 16-byte aligned rows, bank = 4 row + c
  constexpr unsigned WORK_B = TILE_B + 4 * (2 * ROWS * RS + TJM + 4 * ROWS);
  constexpr unsigned MERGE_B = 4u * ROWS * KC * 2;
  constexpr unsigned SH_B = WORK_B > MERGE_B ? WORK_B : MERGE_B;
  __shared__ __attribute__((aligned(16))) char smem_raw[SH_B];
  float* xq = reinterpret_cast<float*>(smem_raw + TILE_B);         // [64 query rows][RS]    fp32, resident
  float* xc = xq + ROWS * RS;                                      // [64 candidates][RS]    fp32 copy of the current tile
  float* sjs = xc + TJM * RS;                                      // [TJM]
  volatile float* thrw = sjs + TJM;                                // [4 lists][64 rows]

  const ScanLane m;
  const int tid = m.tid, l31 = m.l31, h = m.h, cbase = m.cbase, lid = m.lid, rslot = m.rslot;
  const int b = blockIdx.y;
  const int row0 = blockIdx.x * ROWS;
  const int row = row0 + rslot;
  const float* xb = x + (int64_t)b * N * ldx;
  const float* sqb = sq + (int64_t)b * N;
  const int rowc = row < N ? row : N - 1;
  const float si = sqb[rowc];
  const float t0 = tau0 ? next_up(tau0[(int64_t)b * N + rowc]) : INFINITY;      // seed bound: knn_mfma_kernel's t0 (its own line there)

  bf16x8 q1[4], q2[4];                       // B operand
  split_query_planes(xb + (int64_t)rowc * ldx, C, h, q1, q2);
  // fp32 copy of the block's query rows for the exact re-check
  for (int e = tid; e < ROWS * (CP / 4); e += 256) {
    const int r = e / (CP / 4), c4 = (e % (CP / 4)) * 4;
    const int rr = (row0 + r < N) ? row0 + r : N - 1;
    float4 t4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c4 < C) t4 = *reinterpret_cast<const float4*>(xb + (int64_t)rr * ldx + c4);
    *reinterpret_cast<float4*>(xq + r * RS + c4) = t4;
  }

  float dl[KC];
  int jl[KC];
  list_init<KC>(dl, jl);

  // candidate tile: 64 rows x 64 channels -> registers (float4 pieces) -> two bf16 planes in LDS
  constexpr int NV = (TJM * (CP / 4)) / 256;   // 4
  float4 pre[NV];
  float pre_s = INFINITY;
  auto fetch = [&](int j0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int e = tid + 256 * i;
      const int r = e / (CP / 4);
      const int c4 = (e % (CP / 4)) * 4;
      const int j = j0 + r;
      pre[i] = load_row_quad<true>(xb, ldx, j < N ? j : N - 1, c4, C, true);
    }
    if (tid < TJM) pre_s = (j0 + tid < N) ? sqb[j0 + tid] : INFINITY;
  };
  auto stash = [&]() {
    char* base = smem_raw;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int e = tid + 256 * i;
      const int r = e / (CP / 4);
      const int c4 = (e % (CP / 4)) * 4;
      unsigned h0, m0, h1, m1;
      split2_pair(pre[i].x, pre[i].y, h0, m0);
      split2_pair(pre[i].z, pre[i].w, h1, m1);
      const unsigned off = (unsigned)(c4 >> 3) * CS + (unsigned)r * 16u + (unsigned)(c4 & 4) * 2u;
      *reinterpret_cast<uint2*>(base + off) = make_uint2(h0, h1);
      *reinterpret_cast<uint2*>(base + PB + off) = make_uint2(m0, m1);
      *reinterpret_cast<float4*>(xc + r * RS + c4) = pre[i];
    }
    if (tid < TJM) sjs[tid] = pre_s;
  };

  const int nt = (N + TJM - 1) / TJM;
  fetch(0);
  thrw[tid] = INFINITY;
  const unsigned a_off = (unsigned)h * CS + (unsigned)(cbase + l31) * 16u;     // chunk 2 s + h of candidate cbase + l31
  const float kappa = 1.0f / 8192.0f;                                          // eps = 2^-13 (s_i + s_j)

#pragma unroll 1
  for (int t = 0; t < nt; ++t) {
    const int j0 = t * TJM;
    if (t > 0) __syncthreads();              // every wave is done with tile t-1 (planes, fp32 copy)
    stash();                                 // tile t: registers -> LDS
    thrw[lid * ROWS + rslot] = dl[KC / 4 - 1];
    if (t + 1 < nt) fetch(j0 + TJM);         // tile t+1: global -> registers, in flight during this step
    __syncthreads();
    if (j0 + cbase < N) {                    // wave-uniform
      const float o1 = thrw[(lid ^ 1) * ROWS + rslot], o2 = thrw[(lid ^ 2) * ROWS + rslot], o3 = thrw[(lid ^ 3) * ROWS + rslot];
      const char* base = smem_raw + a_off;
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(base + 2 * s * CS);
        const bf16x8 a2 = *reinterpret_cast<const bf16x8*>(base + PB + 2 * s * CS);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, q1[s], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, q2[s], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, q1[s], acc, 0, 0, 0);
      }
      // ---- conservative filter on the approximate distances
      const float thr = fminf(fminf(dl[KC - 1], t0), next_up(fmaxf(fmaxf(dl[KC / 4 - 1], o1), fmaxf(o2, o3))));
      const float* sj = sjs + cbase + 4 * h;
      unsigned mask = 0u;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 s4 = *reinterpret_cast<const float4*>(sj + 8 * q);
        const float sv[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * q + e;
          const float tt = si + sv[e];
          const float tp = 2.0f * acc[r];
          const float da = tt - tp;
          const float lim = fmaf(tt, kappa, thr);            // thr + eps(i, j); +inf while the list is not full
          mask |= sel_01(m_flt(da, lim)) << r;
        }
      }
      // ---- survivors: the normative distance on the VALU, the exact filter, the insert
      while (__any(mask != 0u)) {
        const lmask_t live = m_ine((int)mask, 0);
        const int g = __builtin_ctz(mask | 0x80000000u) & 15;
        mask &= mask - 1u;
        const int i = d_layout_index(g, h);
        const int j = j0 + cbase + i;
        const float* xj = xc + (cbase + i) * RS;             // fp32 copy of the candidate row (rows past N: zeros, s_j = +inf)
        const float* xi = xq + rslot * RS;
        float p = 0.f;
        // the oracle's chain, c ascending from +0 (C % 4 == 0).  C = 64 (every feature-space graph of the model): fully
        // unrolled with the row quads of step q + 2 requested before the four fmas of step q -- the chain is latency bound
        // (16 dependent LDS round trips otherwise; 0.68 -> 0.31 ms at (24,2048,64,20) with the kernel forced on).
        if (C == 64) {
          float4 a[3], v[3];
          a[0] = *reinterpret_cast<const float4*>(xi); v[0] = *reinterpret_cast<const float4*>(xj);
          a[1] = *reinterpret_cast<const float4*>(xi + 4); v[1] = *reinterpret_cast<const float4*>(xj + 4);
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            if (q + 2 < 16) {
              a[(q + 2) % 3] = *reinterpret_cast<const float4*>(xi + 4 * (q + 2));
              v[(q + 2) % 3] = *reinterpret_cast<const float4*>(xj + 4 * (q + 2));
            }
            const float4 aa = a[q % 3], vv = v[q % 3];
            p = fmaf(aa.x, vv.x, p); p = fmaf(aa.y, vv.y, p); p = fmaf(aa.z, vv.z, p); p = fmaf(aa.w, vv.w, p);
          }
        } else {
#pragma unroll 2
          for (int c0 = 0; c0 < C; c0 += 4) {
            const float4 aa = *reinterpret_cast<const float4*>(xi + c0);
            const float4 vv = *reinterpret_cast<const float4*>(xj + c0);
            p = fmaf(aa.x, vv.x, p); p = fmaf(aa.y, vv.y, p); p = fmaf(aa.z, vv.z, p); p = fmaf(aa.w, vv.w, p);
          }
        }
        const float tt = si + sjs[cbase + i];
        const float tp = 2.0f * p;
        const float d = tt - tp;
        const lmask_t pass = live & m_flt(d, thr);           // exact filter (thr as of the start of the tile: conservative)
        list_insert<KC, false>(dl, jl, sel_f(pass, d, INFINITY), j);
      }
    }
  }

  merge_lists_write<KC, false>(reinterpret_cast<float*>(smem_raw), dl, jl, lid, rslot, m.cs == 0, h == 0, row < N, idx,
                               (int64_t)b * N + row, k, N, 0);
}

// ------------------------------------------------------------------------------------------------
// Seeded scan, append form (round 5).  With a rigorous bound tau_r >= the row's k-th distance known IN ADVANCE (the seed bound), the
// scan does not need sorted lists at all: a candidate is either farther than tau_r (dropped) or it is APPENDED, unsorted, to the row's
// candidate buffer in global memory -- a superset of the row's true top k, ~1.7 ... 3 k entries (profiles/r05/knn_seed.txt) -- and a
// second kernel picks the k smallest of every buffer in (d, j) order.  What that removes from the bf16-filter kernel above is its
// dominant cost at N = 2048 (116 of 168 us; the filter alone runs in 52): the per-lane sorted insert (90 VALU ops per round, rounds
// = the maximum over 64 lanes of a count whose mean is 0.4), and most of the exact re-check, because the survivors of a wave are
// first COMPACTED across lanes through a small LDS queue (any lane re-checks any (row, candidate) pair: both rows are in LDS): one
// re-check round per tile at ~40 % lane use instead of ~2.5 rounds at 15 %.
//   entry  = 64-bit key (orderable bits of d << 32 | j): unsigned order == (d, j) lexicographic order (d never NaN / -0)
//   buffer = cap entries per row, cap >= k + 64; invariant at the start of every tile: count <= cap - 64 (a tile adds at most 64).
//            A row that crosses the mark is compacted at the next tile boundary by one wave: its k smallest entries stay, its bound
//            becomes their largest distance (rigorous again: k candidates at distance <= it).  Rows without a usable seed (tau0 =
//            +inf) work the same way -- they just compact after their first tiles.
// Append order is arbitrary (LDS atomics), the result is not: the selection is by a total order on distinct keys, and WHEN a row
// compacts depends only on its counts at tile boundaries.  Distances are the normative ones (same chain as above): bit-exact indices.
__device__ __forceinline__ float knn_key_dist(unsigned long long key) {
  const unsigned o = (unsigned)(key >> 32);
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}
__device__ __forceinline__ unsigned long long readlane64(unsigned long long v, int l) {
  const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)v, l), hi = __builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}

constexpr int KA_MAXE = 8;                   // entries per lane: cap <= 512
// Levels of the append-form scan's bound tightening: T 0.9^m, m = 0..6 (down to 0.53 T: the seed bound is ~1.3 ... 1.5 x the true
// k-th distance, profiles/r05/knn_seed.txt).  The SAME float product T * ka_level(m) is what candidates are counted under and what
// the bound becomes, so the rounding of the constants does not matter.
constexpr int KA_SLACK = 192;                // appends a row can receive between two tile boundaries: 2 waves x (32 new + < 64 waiting)
constexpr int KA_SLACK_LX = 64;              // ... when nothing waits across tiles: the tile's 64 candidates
constexpr float KA_C1 = 0.5f * (1.0f - 1.0f / 8192.0f);
constexpr int KA_LEVELS = 7;
__device__ __forceinline__ constexpr float ka_level(int m) {
  constexpr float L[KA_LEVELS] = {1.0f, 0.9f, 0.81f, 0.729f, 0.6561f, 0.59049f, 0.531441f};
  return L[m];
}

template <int J2>
__device__ __forceinline__ unsigned long long bitonic_steps_down(unsigned long long key, int lane, bool up) {
  key = bitonic_step<J2>(key, lane, up);
  if constexpr (J2 > 1) key = bitonic_steps_down<J2 / 2>(key, lane, up);
  return key;
}
// bitonic merge: a bitonic sequence of one key per lane -> ascending by lane
__device__ __forceinline__ unsigned long long wave_merge64(unsigned long long key, int lane) {
  return bitonic_steps_down<32>(key, lane, true);
}
// bitonic sort of one key per lane across the wave, ascending by lane
__device__ __forceinline__ unsigned long long wave_sort64(unsigned long long key, int lane) {
  key = bitonic_steps_down<1>(key, lane, (lane & 2) == 0);
  key = bitonic_steps_down<2>(key, lane, (lane & 4) == 0);
  key = bitonic_steps_down<4>(key, lane, (lane & 8) == 0);
  key = bitonic_steps_down<8>(key, lane, (lane & 16) == 0);
  key = bitonic_steps_down<16>(key, lane, (lane & 32) == 0);
  return wave_merge64(key, lane);
}
// One wave: the 64 smallest of the S (<= 64 E) keys of a row, ascending by lane.  key[q] = entry lane + 64 q (~0 beyond S): every
// register is sorted across the lanes, then folded into the running lowest 64: min(a[l], b[63 - l]) is a bitonic sequence that
// holds the 64 smallest of a and b (the half-cleaner), one merge sorts it.
template <int E>
__device__ __forceinline__ unsigned long long wave_lowest64(const unsigned long long (&key)[E], int S, int lane) {
  unsigned long long res = wave_sort64(key[0], lane);
#pragma unroll
  for (int q = 1; q < E; ++q) {
    if (64 * q < S) {                        // wave-uniform
      const unsigned long long sq = wave_sort64(key[q], lane);
      const unsigned lo = __shfl((unsigned)sq, 63 - lane, 64), hi = __shfl((unsigned)(sq >> 32), 63 - lane, 64);
      const unsigned long long rb = ((unsigned long long)hi << 32) | lo;
      res = wave_merge64(rb < res ? rb : res, lane);
    }
  }
  return res;
}

// LX: the candidates' fp32 rows are kept in LDS next to the tile and a wave's survivors are re-checked tile by tile (N < 8192: ~10
// pairs per wave and tile, LDS is the cheaper source); !LX: pairs wait in the queue across tiles until 64 are there and read the
// candidate row from global memory (L2) -- at N = 65536 a wave meets a survivor every other tile.
// NPR = products of the filter's inner product: 3 = a1 q1 + a1 q2 + a2 q1 (two bf16 terms per operand; |d' - d| <= 2^-14 t; reached:
// 1.86 * 2^-16 t, as above), 1 = a1 q1 only (plain bf16 operands, unit roundoff 2^-8: |p' - p| <= sum |a q| (2^-7 + 2^-16) <=
// (t / 2) 2^-7 (1 + 2^-9), fp32 accumulation of exact products on top: |d' - d| <= 2^-7 t (1 + 2^-8); reached: 0.96 * 2^-7 t on the
// same clouds; tested with 2^-6 t): a third of the MFMAs, a quarter of the staging arithmetic, one plane in LDS -- for a wider
// margin, i.e. more pairs re-checked exactly.  The result is the same bit for bit (the re-check decides).
template <bool LX, int NPR = 3, class Clouds = DenseClouds>
// N >= 8192 with the one-product filter: 4 workgroups per CU (128 VGPRs; the re-check's candidate ring 8 -> 4 deep keeps it out of
// scratch): (8,16384,64,40) 2048 workgroups = 2 rounds of 1024 instead of 2.67 of 768, 1.71 -> 1.54 ms (profiles/r06/knn_occ.txt)
__global__ __launch_bounds__(256, ((LX || NPR != 1) ? 3 : 4)) void knn_bf16a_kernel(const float* __restrict__ x, const float* __restrict__ sq, Clouds cl, int C,
                                                           int64_t ldx, int k, const float* __restrict__ tau0, int cap,
                                                           unsigned long long* __restrict__ ent, int* __restrict__ cnt,
                                                           int ka_tight_mask) {
  constexpr int CP = 64;
  constexpr int TJM = 64;
  constexpr unsigned CS = TJM * 16 + 16;
  constexpr unsigned PB = 8 * CS;
  constexpr unsigned TILE_B = 2 * PB;
  constexpr int RS = CP + 4;                 // (LX) fp32 row stride of the candidate copy: bank = 4 row + c
  constexpr int QN = 128;                    // queue entries per wave
  using qent_t = typename std::conditional<LX, unsigned short, unsigned>::type;
  // [planes | xq (64 query rows x 64 fp32, 16-byte granules XOR-swizzled by the row) | LX: xc (the tile's rows, fp32, padded) |
  //  sjs | thr_s | cnt_s | hist | queue | flags]
  constexpr unsigned SH_B = TILE_B + 4 * (ROWS * CP + (LX ? TJM * RS : 0) + TJM + ROWS + ROWS + 4 * ROWS) + sizeof(qent_t) * 4 * QN + 16;
  __shared__ __attribute__((aligned(16))) char smem_raw[SH_B];
  float* xq = reinterpret_cast<float*>(smem_raw + TILE_B);
  float* xc = xq + ROWS * CP;
  float* sjs = xc + (LX ? TJM * RS : 0);
  volatile float* thr_s = sjs + TJM;                               // [64 rows]: a candidate stays iff d < thr_s
  int* cnt_s = reinterpret_cast<int*>(const_cast<float*>(thr_s) + ROWS);   // [64 rows]: entries in the row's buffer
  // [64 rows][4 words]: level histogram of the row's candidates (below).  word 0 = bin 0 << 16 | upper half of T's bits, words 1-3 =
  // bins 1..6, two 16-bit counters each
  unsigned* hist = reinterpret_cast<unsigned*>(cnt_s + ROWS);
  // per wave: survivors of the conservative filter waiting for their exact distance: (row of the wave, candidate) as
  // LX: row << 6 | candidate of the tile;  !LX: row << 27 | candidate of the cloud
  volatile qent_t* queue = reinterpret_cast<qent_t*>(hist + 4 * ROWS);
  volatile int* flags = reinterpret_cast<int*>(const_cast<qent_t*>(queue) + 4 * QN);   // [2]: a row crossed the mark in tile t (t & 1)

  const ScanLane m;
  const int tid = m.tid, lane = m.lane, w = m.w, l31 = m.l31, h = m.h, qg = m.qg, cbase = m.cbase, rslot = m.rslot;
  const int b = blockIdx.y;
  const int N = cl.size(b);
  if (Clouds::kPacked && (int)blockIdx.x * ROWS >= N) return;
  const int row0 = blockIdx.x * ROWS;
  const int row = row0 + rslot;
  const float* xb = x + cl.base(b) * ldx;
  const float* sqb = sq + cl.base(b);
  const int rowc = row < N ? row : N - 1;
  const float si = sqb[rowc];
  const int64_t grow0 = cl.base(b) + row0;                         // global row of the block's first query row
  const int trig = cap - (LX ? KA_SLACK_LX : KA_SLACK);
  volatile qent_t* myq = queue + w * QN;
  constexpr float C1 = (NPR == 3) ? KA_C1 : 0.5f * (1.0f - 1.0f / 64.0f);       // the filter's (1 - E') / 2
  const int tight_mask = ka_tight_mask;

  bf16x8 q1[4], q2[4];                       // B operand (NPR == 1: q2 is not used)
  split_query_planes(xb + (int64_t)rowc * ldx, C, h, q1, q2);
  for (int e = tid; e < ROWS * (CP / 4); e += 256) {
    const int r = e / (CP / 4), c4 = (e % (CP / 4)) * 4;
    const int rr = (row0 + r < N) ? row0 + r : N - 1;
    float4 t4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c4 < C) t4 = *reinterpret_cast<const float4*>(xb + (int64_t)rr * ldx + c4);
    *reinterpret_cast<float4*>(xq + r * CP + ((((c4 >> 2) ^ r) & 15) << 2)) = t4;
  }
  if (tid < ROWS) {
    const int rr = (row0 + tid < N) ? row0 + tid : N - 1;
    const float t0 = tau0[cl.base(b) + rr];
    thr_s[tid] = next_up(t0);
    cnt_s[tid] = 0;
    // levels T c_m, T = t0 truncated to its upper 16 bits (any positive T <= t0 serves; 16 bits fit beside a counter).  Rows
    // without a finite positive bound, and clouds whose candidates could overflow a 16-bit counter, do not count (T = 0).
    const bool lv = (t0 > 1e-30f) && (t0 < INFINITY) && (N <= 65536);
    hist[4 * tid] = lv ? (__float_as_uint(t0) >> 16) : 0u;
    hist[4 * tid + 1] = 0u; hist[4 * tid + 2] = 0u; hist[4 * tid + 3] = 0u;
  }
  if (tid < 2) flags[tid] = 0;

  const int fr = tid >> 4, fc4 = (tid & 15) << 2;
  constexpr int NV = (TJM * (CP / 4)) / 256;   // 4
  float4 pre[NV];
  float pre_s = INFINITY;
  auto fetch = [&](int j0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int e = tid + 256 * i;
      const int r = e / (CP / 4);
      const int c4 = (e % (CP / 4)) * 4;
      const int j = j0 + r;
      pre[i] = load_row_quad<true>(xb, ldx, j < N ? j : N - 1, c4, C, true);
    }
    if (tid < TJM) pre_s = (j0 + tid < N) ? sqb[j0 + tid] : INFINITY;
  };
  auto stash = [&]() {
    char* base = smem_raw;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int r = fr + 16 * i;
      const int c4 = fc4;
      unsigned h0, m0, h1, m1;
      const unsigned off = (unsigned)(c4 >> 3) * CS + (unsigned)r * 16u + (unsigned)(c4 & 4) * 2u;
      if (NPR == 3) {
        split2_pair(pre[i].x, pre[i].y, h0, m0);
        split2_pair(pre[i].z, pre[i].w, h1, m1);
        *reinterpret_cast<uint2*>(base + PB + off) = make_uint2(m0, m1);
      } else {
        h0 = cvt_pk_bf16(pre[i].x, pre[i].y);
        h1 = cvt_pk_bf16(pre[i].z, pre[i].w);
      }
      *reinterpret_cast<uint2*>(base + off) = make_uint2(h0, h1);
      if (LX) *reinterpret_cast<float4*>(xc + r * RS + c4) = pre[i];
    }
    if (tid < TJM) sjs[tid] = pre_s * C1;             // the filter's per-candidate term (below); rows past N: +inf
  };

  // exact distance of the queued (row, candidate) pairs of this wave, one per lane, and the append.  x_i from the block's fp32 LDS
  // copy, x_j from global memory (L2: the cloud's rows) -- pairs wait in the queue until 64 of them are there, whatever tile they
  // came from (at N = 2048 a wave meets ~10 survivors per tile, at N = 65536 one every other tile: re-checking them tile by tile
  // runs the 64-step chain for a handful of lanes).  The row's bound is applied when the pair is appended, as it stands then.
  auto process = [&](int nvalid, int j0, int par) {
    const bool on = lane < nvalid;
    const unsigned e = on ? (unsigned)myq[lane] : 0u;
    const int rl = LX ? (int)(e >> 6) : (int)(e >> 27);
    const int j = LX ? j0 + (int)(e & 63u) : (int)(e & 0x7ffffffu);
    const int rs = qg * 32 + rl;
    const float* xi = xq + rs * CP;
    const int rx = (rs & 15) << 2;                                   // granule q of the row sits at float offset (4 q) ^ rx
    const float* xj = LX ? xc + (j - j0) * RS : xb + (int64_t)j * ldx;
    const float sjv = sqb[j];
    float p = 0.f;
    if (C == 64) {
      constexpr int VR = LX ? 3 : (NPR == 1 ? 4 : 8);                                 // ring of candidate quads: LDS two ahead, global eight ahead
      float4 v[VR], a[3];
#pragma unroll
      for (int q = 0; q < VR - (LX ? 1 : 0); ++q) v[q] = *reinterpret_cast<const float4*>(xj + 4 * q);
      a[0] = *reinterpret_cast<const float4*>(xi + (0 ^ rx));
      a[1] = *reinterpret_cast<const float4*>(xi + (4 ^ rx));
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        if (q + 2 < 16) a[(q + 2) % 3] = *reinterpret_cast<const float4*>(xi + ((4 * (q + 2)) ^ rx));
        if (LX && q + 2 < 16) v[(q + 2) % 3] = *reinterpret_cast<const float4*>(xj + 4 * (q + 2));
        const float4 aa = a[q % 3], vv = v[q % VR];
        if (!LX && q + VR < 16) v[q % VR] = *reinterpret_cast<const float4*>(xj + 4 * (q + VR));
        p = fmaf(aa.x, vv.x, p); p = fmaf(aa.y, vv.y, p); p = fmaf(aa.z, vv.z, p); p = fmaf(aa.w, vv.w, p);
      }
    } else {
#pragma unroll 2
      for (int c0 = 0; c0 < C; c0 += 4) {
        const float4 aa = *reinterpret_cast<const float4*>(xi + (c0 ^ rx));
        const float4 vv = *reinterpret_cast<const float4*>(xj + c0);
        p = fmaf(aa.x, vv.x, p); p = fmaf(aa.y, vv.y, p); p = fmaf(aa.z, vv.z, p); p = fmaf(aa.w, vv.w, p);
      }
    }
    const float sir = __shfl(si, rl, 64);                            // lane rl (h = 0) holds s_i of row rl of this wave
    const float tt = sir + sjv;
    const float tp = 2.0f * p;
    const float d = tt - tp;
    if (on && d < thr_s[rs]) {
      const int pos = atomicAdd(&cnt_s[rs], 1);                      // < cap by the invariant
      ent[(grow0 + rs) * cap + pos] = knn_key(d, Clouds::kPacked ? (int)cl.base(b) + j : j);     // (one offset per row: same order)
      if (pos >= trig) flags[par] = 1;
      // level histogram: the finest level T c_m the candidate lies under (the row itself is left out: one count less can
      // never overflow a 16-bit counter at N <= 65536)
      const float T = __uint_as_float(hist[4 * rs] << 16);
      int m = 0;
#pragma unroll
      for (int u = 0; u < KA_LEVELS; ++u) m += (d < T * ka_level(u)) ? 1 : 0;
      if (m > 0 && j != row0 + rs) atomicAdd(&hist[4 * rs + (m >> 1)], 1u << ((m & 1) << 4));      // bin m - 1 = 16-bit field m
    }
  };

  const int nt = (N + TJM - 1) / TJM;
  fetch(0);
  const unsigned a_off = (unsigned)h * CS + (unsigned)(cbase + l31) * 16u;
  int qn = 0;                                // pairs waiting in this wave's queue (wave-uniform)

#pragma unroll 1
  for (int t = 0; t < nt; ++t) {
    const int j0 = t * TJM;
    const int par = t & 1;
    __syncthreads();                         // every wave is done with tile t-1 (planes, fp32 copy, appends; first trip: the set-up)
    stash();
    if (t + 1 < nt) fetch(j0 + TJM);
    if (tid == 0) flags[par] = 0;            // (last read between the barriers of tile t-1, next set behind the barrier below)
    if (t > 0 && ((t & tight_mask) == 0 || t < 8) && lane < 16) {
      // (every tile for the first 8 tiles, where the bounds move most, then every (tight_mask + 1)-th: the ~80 instructions below
      //  were a third of a tile's vector work)
      // Bound tightening from the histogram: k candidates seen under T c_m  =>  the row's k-th distance is < T c_m, and a candidate
      // at d >= T c_m has k candidates strictly before it.  (Rows r = w + 4 lane': the wave that would also compact the row.)
      const int r = w + 4 * lane;
      const uint4 hw = *reinterpret_cast<const uint4*>(hist + 4 * r);
      const float T = __uint_as_float(hw.x << 16);
      const unsigned bin[KA_LEVELS] = {hw.x >> 16, hw.y & 0xffffu, hw.y >> 16, hw.z & 0xffffu, hw.z >> 16, hw.w & 0xffffu, hw.w >> 16};
      unsigned c = 0u;
      float tn = INFINITY;
#pragma unroll
      for (int u = KA_LEVELS - 1; u >= 0; --u) {
        c += bin[u];
        if (c >= (unsigned)k && tn == INFINITY) tn = T * ka_level(u);
      }
      if (T > 0.f && tn < thr_s[r]) thr_s[r] = tn;
    }
    if (t > 0 && flags[par ^ 1]) {           // block-uniform: some row crossed the mark in tile t-1 -> compact it to its k smallest
#pragma unroll 1
      for (int r = w; r < ROWS; r += 4) {
        const int S = cnt_s[r];
        if (S > trig) {                      // wave-uniform
          unsigned long long* buf = ent + (grow0 + r) * cap;
          unsigned long long key[KA_MAXE];
#pragma unroll
          for (int q = 0; q < KA_MAXE; ++q) {
            const int e = lane + 64 * q;
            key[q] = (e < S) ? __hip_atomic_load(buf + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ~0ull;
          }
          const unsigned long long best = wave_lowest64<KA_MAXE>(key, S, lane);       // lane l: the row's (l + 1)-th smallest key
          if (lane < k) buf[lane] = best;
          if (lane == k - 1) {
            thr_s[r] = next_up(knn_key_dist(best));
            cnt_s[r] = k;
          }
        }
      }
    }
    __syncthreads();
    if (j0 + cbase < N) {                    // wave-uniform
      const char* base = smem_raw + a_off;
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(base + 2 * s * CS);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, q1[s], acc, 0, 0, 0);
        if (NPR == 3) {
          const bf16x8 a2 = *reinterpret_cast<const bf16x8*>(base + PB + 2 * s * CS);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, q2[s], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, q1[s], acc, 0, 0, 0);
        }
      }
      // Conservative filter on the approximate inner products a: the exact rule "d < thr" can only hold if  t - 2 a < thr + 2^-14 t
      // (t = s_i + s_j; bound on |d' - d| above), i.e.  a > (1 - 2^-14) t / 2 - thr / 2.  Tested with 2^-13 for 2^-14 and the right
      // side as  c1 s_j + (c1 s_i - thr / 2),  c1 = (1 - 2^-13) / 2: the roundings of that sum (< 2^-20 t) sit far inside the
      // 2^-15 t of slack; one add and one compare per candidate.  thr = +inf: everything passes; rows past N: nothing does.
      // A positive thr below 2 FLT_MIN must not halve to zero: all-zero rows seeded with all-zero rows have tau0 = 0 and thr =
      // next_up(0), the smallest denormal, and with s_i = s_j = a = 0 the test would read 0 < 0 and drop the very pairs at d = 0 that
      // thr admits.  FLT_MIN for the half instead: a larger half-threshold only sends more pairs to the exact re-check.
      const float thr = (row < N) ? thr_s[rslot] : -INFINITY;
      const float hthr = (thr > 0.f) ? fmaxf(0.5f * thr, 1.17549435e-38f) : 0.5f * thr;
      const float gi = si * C1 - hthr;
      const float* sj = sjs + cbase + 4 * h;
      unsigned mask = 0u;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 s4 = *reinterpret_cast<const float4*>(sj + 8 * q);
        const float sv[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * q + e;
          mask |= sel_01(m_flt(sv[e] + gi, acc[r])) << r;
        }
      }
      // survivors -> this wave's queue, compacted across lanes; a full batch of 64 is re-checked at once
      while (true) {
        const bool has = mask != 0u;
        const unsigned long long bal = __ballot(has);
        if (bal == 0ull) break;
        const int g = __builtin_ctz(mask | 0x80000000u) & 15;
        const int before = __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
        if (has) {
          const unsigned ci = (unsigned)(cbase + d_layout_index(g, h));
          myq[qn + before] = LX ? (qent_t)(((unsigned)l31 << 6) | ci) : (qent_t)(((unsigned)l31 << 27) | ((unsigned)j0 + ci));
          mask &= mask - 1u;
        }
        qn += __popcll(bal);
        if (qn >= 64) {
          process(64, j0, par);
          qn -= 64;
          const qent_t mv = myq[64 + lane];
          if (lane < qn) myq[lane] = mv;
        }
      }
      if (LX && qn > 0) {                    // the tile's rows leave LDS at the next barrier
        process(qn, j0, par);
        qn = 0;
      }
    }
  }
  if (qn > 0) process(qn, 0, (nt - 1) & 1);
  __syncthreads();
  if (tid < ROWS && row0 + tid < N) cnt[grow0 + tid] = cnt_s[tid];
}

// the k smallest keys of every row's buffer, ascending: one wave per row.
// S < k (non-finite input only: the scan appends d < thr <= +inf, so a buffer holds every candidate below +inf until k of them have
// been seen -- the seed bound is finite only if k seeds are at finite distance, every later bound is the k-th of a buffer): the row's
// other k - S entries are the candidates at D~ = +inf by ascending j, i.e. the lowest j of the cloud that the buffer does not hold.
// They are among 0 .. 2 k - 1 < 128: two 64-bit presence masks built from the S sorted entries, every lane ranks its own two values.
template <class Clouds>
__global__ __launch_bounds__(256) void knn_select_kernel(const unsigned long long* __restrict__ ent, const int* __restrict__ cnt,
                                                         Clouds cl, int64_t rows, int cap, int k, int32_t* __restrict__ idx) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));       // (one row per wave)
  if (row >= rows) return;
  const int S = cnt[row];
  const unsigned long long* buf = ent + row * cap;
  int32_t* out = idx + row * k;
  if (S <= 64) {
    unsigned long long key = (lane < S) ? buf[lane] : ~0ull;
    key = wave_sort64(key, lane);
    if (lane < (S < k ? S : k)) out[lane] = (int32_t)(unsigned)key;
    if (S < k) {                             // wave-uniform
      int base = 0, N = 0;
      if constexpr (Clouds::kPacked) {
        const int cloud = cl.cloud_of(row);
        base = (int)cl.base(cloud);
        N = cl.size(cloud);
      } else {
        N = cl.N;
      }
      const int jloc = (lane < S) ? (int)(unsigned)key - base : -1;
      unsigned long long held0 = 0ull, held1 = 0ull;
      for (int t = 0; t < S; ++t) {
        const unsigned st = (unsigned)__builtin_amdgcn_readlane(jloc, t);
        if (st < 64u) held0 |= 1ull << st;
        else if (st < 128u) held1 |= 1ull << (st - 64u);
      }
      // values v < N only (k <= N: there are at least k - S of them)
      const unsigned long long in0 = N >= 64 ? ~0ull : ((1ull << N) - 1ull);
      const unsigned long long in1 = N >= 128 ? ~0ull : (N > 64 ? ((1ull << (N - 64)) - 1ull) : 0ull);
      const unsigned long long free0 = ~held0 & in0, free1 = ~held1 & in1;
      const unsigned long long below = (1ull << lane) - 1ull;
      const int p0 = S + __popcll(free0 & below), p1 = S + __popcll(free0) + __popcll(free1 & below);
      if (((free0 >> lane) & 1ull) && p0 < k) out[p0] = base + lane;
      if (((free1 >> lane) & 1ull) && p1 < k) out[p1] = base + 64 + lane;
    }
    return;
  }
  unsigned long long key[KA_MAXE];
#pragma unroll
  for (int q = 0; q < KA_MAXE; ++q) {
    const int e = lane + 64 * q;
    key[q] = (e < S) ? buf[e] : ~0ull;
  }
  const unsigned long long best = wave_lowest64<KA_MAXE>(key, S, lane);
  if (lane < k) out[lane] = (int32_t)(unsigned)best;
}

// Dispatch threshold: with the pipelined re-check the kernel also wins in isolation at (24,2048,64,20) (0.253 vs 0.272 ms), but
// inside the training step it LOSES there (5.19 vs 5.05 ms/step with the side stream on, 5.06 vs 5.11 with it off): its 54 KB x 3
// workgroups leave no LDS for the transposed-adjacency build that runs on the side stream.  So: N >= 8192 only.
int knn_bf16f_mode() { return dg::sw_get(dg::SW_KNN_BF16F); }      // 0 never; 1 always (where applicable); 2 auto (N >= 8192)

bool knn_force_valu() { return dg::sw_get(dg::SW_KNN_FORCE_VALU) == 1; }      // dgcnn_knn_force_valu (tests): VALU fmaf distances for every C

// tau0[row] >= max over the row's first k seed candidates j of D(row, j), D in the normative arithmetic of the scan kernels.
// One wave per query row; LP = C / 4 lanes per pair (lane = LP * slot + channel quad, 64 / LP pairs per step), every pair's
// candidate row read as LP consecutive float4 (whole lines), all steps' loads in flight before the first use.  The inner product
// is summed in a different order than the scan's fmaf chain (4 products per lane, then a butterfly over the LP lanes), so the
// value differs from the scan's by rounding only: both are within 64 * 2^-24 * sum|x_c y_c| <= 2^-19 (s_i + s_j) of the exact
// product; adding 2^-16 (s_i + s_j) (> 4x the worst case, and far below anything that matters to the filter) makes
//     tau0 = max_m [ (s_i + s_j) - 2 p~ + 2^-16 (s_i + s_j) ]
// an upper bound of the normative distances -- all the proof needs (k distinct candidates at distance <= tau0).
// Seeds that are not k DISTINCT in-range indices give +inf (no bound), and so does a seed at a NaN distance.
// Packed towers: seeds are tower rows, and only rows of the query row's own cloud count (a row of a neighbouring cloud can be nearer
// than every true candidate: its distance would be no bound).
template <int LP, int MAXSTEPS, class Clouds = DenseClouds>
__global__ __launch_bounds__(256) void knn_seed_bound_kernel(const float* __restrict__ x, const float* __restrict__ sq, Clouds cl,
                                                             int64_t ldx, const int32_t* __restrict__ seed, int64_t ldseed, int k,
                                                             int64_t rows, float* __restrict__ tau0) {
  constexpr int PPS = 64 / LP;                            // pairs per step
  constexpr int RW = 2;                                   // query rows per wave: their loads are all in flight together
  const int lane = threadIdx.x & 63;
  // XCD x (= block id % 8; each XCD has its own 4 MB L2) owns the x-th eighth of the rows: the neighbour rows its waves gather
  // are then those of a few clouds (1.5 MB at the headline shape) instead of all of them (12.6 MB through every L2: 38 us)
  const int64_t per = ((rows + 7) / 8 + 4 * RW - 1) / (4 * RW) * (4 * RW);       // rows per XCD, a whole number of blocks
  const int64_t g0 = (int64_t)(blockIdx.x & 7) * per + ((int64_t)(blockIdx.x >> 3) * 4 + (threadIdx.x >> 6)) * RW;
  if (g0 >= rows || ((int64_t)(blockIdx.x >> 3) * 4 + (threadIdx.x >> 6)) * RW >= per) return;       // (wave-uniform)
  const int slot = lane / LP, cq = lane % LP;
  const int steps = (k + PPS - 1) / PPS;
  int jj[RW], nn[RW];
  int64_t gr[RW];
  const float* xc[RW];                                    // the row's cloud: x and s_i of its first point (wave-uniform)
  const float* sc[RW];
#pragma unroll
  for (int w = 0; w < RW; ++w) {
    gr[w] = (g0 + w < rows) ? g0 + w : rows - 1;
    jj[w] = (lane < k) ? seed[gr[w] * ldseed + lane] : -1 - lane;      // the row's seeds, one per lane
    if constexpr (Clouds::kPacked) {
      const int cloud = cl.cloud_of(gr[w]);
      const int64_t cb = cl.base(cloud);
      nn[w] = cl.size(cloud);
      jj[w] -= (int)cb;                                                 // tower rows -> rows of the cloud (others: out of range)
      xc[w] = x + cb * ldx;
      sc[w] = sq + cb;
    } else {
      const int N = cl.N;
      const int64_t cloud = (rows < 0x7fffffffll) ? (int64_t)((unsigned)gr[w] / (unsigned)N) : gr[w] / N;
      xc[w] = x + cloud * N * ldx;
      sc[w] = sq + cloud * N;
    }
  }
  const unsigned uld = (unsigned)ldx;                     // (N * ldx < 2^31: checked by the host)
  float4 a[RW], v[RW][MAXSTEPS];
  float si[RW], sj[RW][MAXSTEPS];
#pragma unroll
  for (int w = 0; w < RW; ++w) {
    a[w] = *reinterpret_cast<const float4*>(x + gr[w] * ldx + 4 * cq);
    si[w] = sq[gr[w]];
#pragma unroll
    for (int s = 0; s < MAXSTEPS; ++s) {
      if (s < steps) {                                    // (wave-uniform)
        const int m = s * PPS + slot;
        int jm = __shfl(jj[w], m < 64 ? m : 63, 64);
        int lim;
        if constexpr (Clouds::kPacked) lim = nn[w]; else lim = cl.N;
        jm = (m < k && (unsigned)jm < (unsigned)lim) ? jm : 0;
        v[w][s] = *reinterpret_cast<const float4*>(xc[w] + ((unsigned)jm * uld + 4u * (unsigned)cq));
        sj[w][s] = sc[w][jm];
      }
    }
  }
  // validity of the seeds (k in-range, pairwise distinct indices), under the loads: every seed is broadcast from its lane
  // (v_readlane -> SGPR) and must match exactly one of the k lanes
  const unsigned long long kmask = (k >= 64) ? ~0ull : ((1ull << k) - 1ull);
  bool anybad[RW];
#pragma unroll
  for (int w = 0; w < RW; ++w) {
    bool b = false;
    for (int t = 0; t < k; ++t) {
      const int st = __builtin_amdgcn_readlane(jj[w], t);
      const unsigned long long eq = __ballot(jj[w] == st) & kmask;
      int lim;
      if constexpr (Clouds::kPacked) lim = nn[w]; else lim = cl.N;
      b = b || (__popcll(eq) != 1) || ((unsigned)st >= (unsigned)lim);
    }
    anybad[w] = b;
  }
  // The maximum is taken on the distances' BIT PATTERNS as unsigned integers.  Every d here is +0 or positive, +inf or NaN (the slack
  // 2^-16 tt outweighs the rounding of tt - 2 p~, and finite s_i, s_j leave no way to an infinite p~), and on those the unsigned order is
  // the float order with every NaN, of either sign, above +inf -- fmaxf would DROP a NaN and leave a bound that rests on fewer than k
  // candidates.  A NaN distance is +inf in the selection's order: anything above +inf's pattern means no bound.  (One v_max_u32 per pair
  // where fmaxf was one v_max_f32; a pattern with the sign bit set, should one ever occur, also reads as no bound.)
#pragma unroll
  for (int w = 0; w < RW; ++w) {
    unsigned best = 0u;
#pragma unroll
    for (int s = 0; s < MAXSTEPS; ++s) {
      if (s < steps) {
        float p = a[w].x * v[w][s].x;
        p = fmaf(a[w].y, v[w][s].y, p); p = fmaf(a[w].z, v[w][s].z, p); p = fmaf(a[w].w, v[w][s].w, p);
#pragma unroll
        for (int o = 1; o < LP; o <<= 1) p += __shfl_xor(p, o, 64);
        const float tt = si[w] + sj[w][s];
        const unsigned d = __float_as_uint(fmaf(-2.0f, p, tt) + tt * (1.0f / 65536.0f));
        best = (s * PPS + slot < k) ? (d > best ? d : best) : best;
      }
    }
#pragma unroll
    for (int o = LP; o < 64; o <<= 1) {
      const unsigned ob = __shfl_xor(best, o, 64);
      best = ob > best ? ob : best;
    }
    if (lane == 0 && g0 + w < rows) tau0[g0 + w] = (anybad[w] || best > 0x7f800000u) ? INFINITY : __uint_as_float(best);
  }
}

// C in {16, 32, 64} (LP = 4, 8, 16 lanes per pair), rows 16-byte aligned; k <= 64.  Returns false when the shape is not taken.
template <class Clouds>
bool launch_seed_bound(const float* x, const float* sq, int64_t rows, Clouds cl, int C, int64_t ldx, const int32_t* seed,
                       int64_t ldseed, int k, float* tau0, hipStream_t st) {
  const int64_t per = dg::cdiv(dg::cdiv(rows, 8), 8) * 8;  // rows per XCD (blocks of 4 waves x 2 rows)
  const dim3 grid((unsigned)(per / 8 * 8));                // block id = 8 * (block within the XCD's share) + XCD
#define DG_SB(LPV, MS) dg::launch((knn_seed_bound_kernel<LPV, MS, Clouds>), grid, dim3(256), 0, st, x, sq, cl, ldx, seed, ldseed, k, rows, tau0)
  if (C == 64) { if (k <= 20) DG_SB(16, 5); else if (k <= 40) DG_SB(16, 10); else DG_SB(16, 16); }
  else if (C == 32) { if (k <= 24) DG_SB(8, 3); else DG_SB(8, 8); }
  else if (C == 16) { if (k <= 32) DG_SB(4, 2); else DG_SB(4, 4); }
  else return false;
#undef DG_SB
  return true;
}

}  // namespace

extern "C" int dgcnn_knn_force_valu(int on) {   // A/B switch (tests): 1 = VALU fmaf distances for every C, 0 = MFMA for C > 4
  return dg::sw_exchange(dg::SW_KNN_FORCE_VALU, on ? 1 : 0);
}

extern "C" int dgcnn_knn_bf16_filter(int mode) {   // A/B switch (tests): 0 never, 1 whenever applicable, 2 auto (N >= 8192); returns the previous mode
  return dg::sw_exchange(dg::SW_KNN_BF16F, mode < 0 ? dg::sw_initial(dg::SW_KNN_BF16F) : mode);      // (negative: back to what the environment gave)
}

namespace dg {
size_t knn_grid_workspace_bytes(int B, int N);
bool knn_grid_applicable(int C, int k);
int knn_grid_min_n();
int launch_knn_grid(const float* x, const float* sq, int B, int N, int C, int64_t ldx, int k, int32_t* idx, void* ws, hipStream_t st);
size_t knn_grid_seg_workspace_bytes(int rows, int nseg);
int launch_knn_grid_seg(const float* x, const float* sq, int nseg, const int32_t* seg_off, int rows, int max_n, int C, int64_t ldx, int k,
                        int32_t* idx, void* ws, hipStream_t st);
int launch_knn_grid_listed(const char* what, const float* x, const float* sq, const int32_t* seg_off, const int32_t* list, int nlist,
                           int rows, int max_n, int C, int64_t ldx, int k, int32_t* idx, void* ws, hipStream_t st);
// knn_wide.hip: the channel-slab matrix-pipe scan (C up to 1024; seg_off null = dense clouds) and the s_i kernel for C > 128
void launch_sqnorm_wide(const float* x, int64_t ldx, int64_t rows, int C, float* sq, hipStream_t st);
void launch_knn_wide(const float* x, const float* sq, const int32_t* seg_off, int ny, int max_n, int C, int64_t ldx, int k, int vec_ok,
                     int32_t* idx, hipStream_t st);
// knn_bigk.hip: the append-and-compact scan for 64 < k <= 256 (any C up to 1024; seg_off null = dense clouds); ent: knn_bigk_cap(k)
// 8-byte keys for every row
int knn_bigk_cap(int k);
void launch_knn_bigk(const float* x, const float* sq, const int32_t* seg_off, int ny, int max_n, int C, int64_t ldx, int k, int vec_ok,
                     int32_t* idx, unsigned long long* ent, hipStream_t st);
// s_i of `rows` rows of any width up to 1024 (every entry here, and knn_cross.hip once per operand)
void launch_sqnorm_rows(const float* x, int64_t ldx, int64_t rows, int C, float* sq, hipStream_t st) {
  if (C > 128) {                             // [64][C + 1] floats would not fit: the chunked form of knn_wide.hip, the same sum
    launch_sqnorm_wide(x, ldx, rows, C, sq, st);
    return;
  }
  launch(sqnorm_kernel, dim3((unsigned)cdiv(rows, SQ_ROWS)), dim3(256), sizeof(float) * SQ_ROWS * (C + 1), st, x, ldx, rows, C, sq);
}
}  // namespace dg

static bool knn_append_lx(int N) { return N < 8192; }     // which form of the append scan (knn_bf16a_kernel<LX>)
static int knn_append_cap(int k, int N) {    // entries per row buffer: >= k + slack of the form, <= 64 KA_MAXE
  if (knn_append_lx(N)) return k <= 20 ? 256 : (k <= 40 ? 384 : 512);
  return k <= 20 ? 320 : (k <= 40 ? 448 : 512);
}
static bool knn_append_shape(int C, int k) { return C > 16 && C <= 64 && C % 4 == 0 && k <= 64; }
static int knn_append_tighten_mask(bool lx) {
  const int tight = dg::sw_get(dg::SW_KNN_TIGHTEN_EVERY);      // DGCNN_KNN_TIGHTEN_EVERY (power of two; A/B switch): bound tightening every n-th tile
  // default: every 4th tile below N = 8192, every 8th above (profiles/r06/knn_tight.txt: 175 -> 168 us, 1.83 -> 1.70 ms, 19.2 -> 17.6 ms per call)
  return (tight ? tight : (lx ? 4 : 8)) - 1;
}

// Smallest k that the large-k scan of knn_bigk.hip takes (dense and packed, any C): 1 ... 65, default 65 = only the neighbour counts no
// other kernel has an instance for, so every k <= 64 launches what it always launched.  k > 64 goes there whatever the value.
// DGCNN_KNN_BIG_K_MIN=<1 ... 65>
constexpr int KNN_MAX_K = 256, KNN_BIG_ONLY_K = dg::SW_KNN_BIG_ONLY_K;
static int knn_big_k_min() { return dg::sw_get(dg::SW_KNN_BIG_K_MIN); }
extern "C" int dgcnn_knn_big_k_min(int k) {             // tools / tests: 1 ... 65; any other value only queries; returns the previous value
  return dg::sw_set_or_query(dg::SW_KNN_BIG_K_MIN, k >= 1 && k <= KNN_BIG_ONLY_K, k);
}
// the large-k scan takes this k (the VALU switch keeps every k it has an instance for)
static bool knn_bigk_takes(int k) { return k >= KNN_BIG_ONLY_K || (k >= knn_big_k_min() && !knn_force_valu()); }

// ---- the workspace of every k-NN entry ---------------------------------------------------------------------------------------------
// [s_i of every row | bounds of every row: the seeds' or the histogram's (not in the cell-grid-only entry) | scratch: the cell grid's
// (knn_grid.hip), or the append-form scan's -- one count and `cap` 8-byte entries per row -- or the large-k scan's: the same layout
// (its counts stay in LDS; the count region is left unused)], every region but the last padded to 256 bytes.  An entry and its *_workspace_bytes query build the layout with the same function below: the query answers `end`.
struct KnnWorkspace {
  char* base;                                // the caller's buffer and its size (null, 0: a size query)
  size_t bytes;
  size_t bound, scratch, ent, end;           // byte offsets of the regions (s_i at 0); ent: the append form's entries, after its counts
  int cap;                                   // entries per row of the append form; 0: the scratch is not the append form's
  static size_t pad(size_t n) { return (n + 255) & ~(size_t)255; }
  KnnWorkspace(void* ws, size_t ws_bytes, size_t rows, bool bounds, size_t grid_bytes, int append_cap)
      : base(static_cast<char*>(ws)), bytes(ws_bytes), bound(pad(rows * sizeof(float))), scratch(bounds ? 2 * bound : bound),
        ent(scratch + pad(rows * sizeof(int))),
        end(append_cap ? ent + rows * (size_t)append_cap * sizeof(unsigned long long) : scratch + grid_bytes), cap(append_cap) {}
  bool aligned() const { return (reinterpret_cast<uintptr_t>(base) & 15) == 0; }
  bool holds(size_t upto) const { return bytes >= upto; }
  float* s_i() const { return reinterpret_cast<float*>(base); }
  float* bounds() const { return holds(scratch) ? reinterpret_cast<float*>(base + bound) : nullptr; }   // null: no room for them
  void* grid() const { return base + scratch; }
  int* cnt() const { return reinterpret_cast<int*>(base + scratch); }
  unsigned long long* entries() const { return reinterpret_cast<unsigned long long*>(base + ent); }
};
// dense: the cell grid's scratch for raw coordinates (C <= 4, k <= 40), the append form's for 16 < C <= 64
static KnnWorkspace knn_ws_dense(void* ws, size_t n, int B, int N, int C, int k) {
  if (knn_bigk_takes(k)) return KnnWorkspace(ws, n, (size_t)B * (size_t)N, true, 0, dg::knn_bigk_cap(k));
  const bool grid = dg::knn_grid_applicable(C, k);
  return KnnWorkspace(ws, n, (size_t)B * (size_t)N, true, grid ? dg::knn_grid_workspace_bytes(B, N) : 0,
                      !grid && knn_append_shape(C, k) ? knn_append_cap(k, N) : 0);
}
static KnnWorkspace knn_ws_seg(void* ws, size_t n, int rows, int max_n, int C, int k) {
  if (knn_bigk_takes(k)) return KnnWorkspace(ws, n, (size_t)rows, true, 0, dg::knn_bigk_cap(k));
  return KnnWorkspace(ws, n, (size_t)rows, true, 0, knn_append_shape(C, k) ? knn_append_cap(k, max_n) : 0);
}
static KnnWorkspace knn_ws_seg_grid(void* ws, size_t n, int rows, int nseg) {              // no bounds: the grid uses none
  return KnnWorkspace(ws, n, (size_t)rows, false, dg::knn_grid_seg_workspace_bytes(rows, nseg), 0);
}
static KnnWorkspace knn_ws_seg_mix(void* ws, size_t n, int rows, int n_grid) {             // cell tables for the GRID clouds only
  return KnnWorkspace(ws, n, (size_t)rows, true, dg::knn_grid_seg_workspace_bytes(rows, n_grid), 0);
}

// Seeds are used (a) whenever the append-form scan takes the shape (C in {32, 64}: the bound is what makes it possible) and (b) by
// the list-keeping kernels from N ~ 4096 on: at (24,2048,64,20) the bound kernel (33 us: 252 MB of gathered rows) costs them what
// the scan saves; at (8,16384,64,40) the step goes 39.0 -> 35.8 ms, at (8,65536,64,20) 101 -> 97 (profiles/r05/knn_seed.txt).
static int knn_seed_min_n() { return dg::sw_get(dg::SW_KNN_SEED_MIN_N); }      // DGCNN_KNN_SEED_MIN_N (A/B switch); below 0: auto (the rule above)
extern "C" int dgcnn_knn_seed_min_n(int n) {            // tools / tests: smallest N for which seeds are used (-1: the rule); returns the previous value
  return dg::sw_set_or_query(dg::SW_KNN_SEED_MIN_N, n >= -1, n);
}

static bool knn_append_on() { return dg::sw_get(dg::SW_KNN_APPEND) != 0; }      // DGCNN_KNN_APPEND=0: seeded searches keep per-lane lists (A/B switch)
extern "C" int dgcnn_knn_append(int on) {               // tools / tests; returns the previous setting
  return dg::sw_set_or_query(dg::SW_KNN_APPEND, on >= 0, on ? 1 : 0);
}

// products of the append-form scan's filter per form (LX: N < 8192): 1 since round 6 (profiles/r06/knn_npr.txt: 187 -> 176 us per call
// at (24,2048,64,20), 2.05 -> 1.82 ms at (8,16384,64,40), 22.3 -> 18.9 ms at (8,65536,64,20)); DGCNN_KNN_APPEND_NPR="<lx>,<big>"
// (A/B switch; tests run both)
static int knn_append_products(bool lx) { return dg::sw_get(lx ? dg::SW_KNN_APPEND_NPR_LX : dg::SW_KNN_APPEND_NPR_BIG); }
extern "C" int dgcnn_knn_append_products(int n) {       // tools / tests: 1 or 3 for both forms (other values: query only); returns the previous setting of the N < 8192 form
  dg::sw_set_or_query(dg::SW_KNN_APPEND_NPR_BIG, n == 1 || n == 3, n);
  return dg::sw_set_or_query(dg::SW_KNN_APPEND_NPR_LX, n == 1 || n == 3, n);
}

// raw-coordinate layer (C <= 4): sample stride of the histogram bound (knn_hist_bound_kernel); 0 = no bound.  DGCNN_KNN_HIST=<0|1|2|4>
static int knn_hist_stride(int N) { return N >= 256 ? dg::sw_get(dg::SW_KNN_HIST) : 0; }
extern "C" int dgcnn_knn_hist(int stride) {              // tools / tests: 0 off, 1 / 2 / 4 = sample stride; other values only query; returns the previous setting
  return dg::sw_set_or_query(dg::SW_KNN_HIST, dg::sw_valid(dg::SW_KNN_HIST, stride), stride);
}

// Smallest C that the channel-slab scan of knn_wide.hip takes (dense and packed, any k <= 64): 5 ... 129, default 129 = only the widths
// no other kernel has an instance for, so every narrower shape launches what it always launched.  C > 128 goes there whatever the
// value.  DGCNN_KNN_WIDE_MIN_C=<5 ... 129>
constexpr int KNN_MAX_C = 1024, KNN_WIDE_ONLY_C = dg::SW_KNN_WIDE_ONLY_C;
static int knn_wide_min_c() { return dg::sw_get(dg::SW_KNN_WIDE_MIN_C); }
extern "C" int dgcnn_knn_wide_min_c(int c) {            // tools / tests: 5 ... 129; any other value only queries; returns the previous value
  return dg::sw_set_or_query(dg::SW_KNN_WIDE_MIN_C, c >= 5 && c <= KNN_WIDE_ONLY_C, c);
}
// the channel-slab scan takes this width (the VALU switch keeps every width it has an instance for)
static bool knn_wide_takes(int C) { return C >= KNN_WIDE_ONLY_C || (C >= knn_wide_min_c() && !knn_force_valu()); }


// ---- one dispatch for dense, packed and listed clouds ------------------------------------------------------------------------------
namespace {

// What the host knows of the clouds a call searches: the device-side map, how many there are (grid y), the smallest, the largest and
// the sum of their sizes.  Every size rule is written once in these terms: a kernel's PRECONDITION must hold for the smallest cloud
// (min_n); grids and the form of a kernel go by the largest (max_n).  Dense (B clouds of N points): min_n = max_n = N.
template <class Clouds>
struct CloudSet {
  Clouds cl;
  int ny, min_n, max_n;
  int64_t rows;
  static constexpr bool kDense = std::is_same<Clouds, DenseClouds>::value;
  // ListedClouds exist for the raw-coordinate scan of dgcnn_knn_seg_mix_f32 only (C <= 4, k <= 40, no seeds): nothing else is built
  static constexpr bool kRawOnly = std::is_same<Clouds, ListedClouds>::value;
  dim3 grid(int rows_per_block) const { return dim3((unsigned)dg::cdiv(max_n, rows_per_block), (unsigned)ny); }
};

// what every stage of one call passes on unchanged
struct KnnCall {
  const char* what;                          // the entry's name
  const float* x;
  int C;
  int64_t ldx;
  int k, vec_ok;                             // vec_ok: rows are float4-loadable
  int32_t* idx;
  KnnWorkspace w;
  hipStream_t st;
  const float* sq() const { return w.s_i(); }
};
int knn_vec_ok(const float* x, int64_t ldx) { return (ldx % 4 == 0) && ((reinterpret_cast<uintptr_t>(x) & 15) == 0); }

void launch_sqnorm(const KnnCall& a, int64_t rows) { dg::launch_sqnorm_rows(a.x, a.ldx, rows, a.C, a.w.s_i(), a.st); }

// Raw coordinates (C <= 4): the histogram bound of every row.  Null (no bound) when it is switched off (stride 0, or a cloud under 256
// points), VALU distances are forced, the kernel's precondition N >= 4 k stride fails for the smallest cloud, or there is no room.
template <class Clouds>
const float* launch_hist_bound(const CloudSet<Clouds>& s, const KnnCall& a) {
  const int hs = knn_hist_stride(s.min_n);
  float* tb = a.w.bounds();
  if (hs == 0 || knn_force_valu() || s.min_n < 4 * a.k * hs || !tb) return nullptr;
#define DG_HB(HSV) dg::launch((knn_hist_bound_kernel<HSV, Clouds>), s.grid(64), dim3(256), 0, a.st, a.x, a.sq(), s.cl, a.C, a.ldx, a.k, tb)
  if (hs == 1) DG_HB(1); else if (hs == 2) DG_HB(2); else DG_HB(4);
#undef DG_HB
  return tb;
}

// Bound known in advance (tau0: launch_seed_bound): the append-form scan, then one selection per row
template <class Clouds>
void launch_append_scan(const CloudSet<Clouds>& s, const KnnCall& a, const float* tau0) {
  const bool lx = knn_append_lx(s.max_n);
  const int npr = knn_append_products(lx), tmask = knn_append_tighten_mask(lx);
  const KnnWorkspace& w = a.w;
#define DG_KA(LXV, NPRV) dg::launch((knn_bf16a_kernel<LXV, NPRV, Clouds>), s.grid(ROWS), dim3(256), 0, a.st, a.x, a.sq(), s.cl, a.C, a.ldx, a.k, tau0, w.cap, w.entries(), w.cnt(), tmask)
  if (lx) { if (npr == 1) DG_KA(true, 1); else DG_KA(true, 3); }
  else { if (npr == 1) DG_KA(false, 1); else DG_KA(false, 3); }
#undef DG_KA
  dg::launch(knn_select_kernel<Clouds>, dim3((unsigned)dg::cdiv(s.rows, 4)), dim3(256), 0, a.st, w.entries(), w.cnt(), s.cl, s.rows, w.cap, a.k,
             a.idx);
}

// The scan that keeps its lists.  Dense, 16 < C <= 64: the bf16 matrix pipe + exact re-check of the survivors (large graphs, or a seed
// bound); dense, 4 < C <= 64: fp32 distances on the matrix pipe; everything else, and every packed or listed tower: the VALU scan,
// which takes a bound for C <= 4 only (the histogram's).
template <int CP, int KC, class Clouds>
void launch_scan(const CloudSet<Clouds>& s, const KnnCall& a, const float* tau0) {
  if constexpr (CloudSet<Clouds>::kDense && CP >= 16 && CP <= 64) {
    const int N = s.max_n, m = knn_bf16f_mode();
    const bool vec = a.vec_ok && a.C % 4 == 0;
    if constexpr (CP == 64) {
      if (!knn_force_valu() && vec && a.C > 16 && (m == 1 || (m == 2 && (N >= 8192 || tau0)))) {
        dg::launch((knn_bf16f_kernel<KC>), s.grid(ROWS), dim3(256), 0, a.st, a.x, a.sq(), N, a.C, a.ldx, a.k, a.idx, tau0);
        return;
      }
    }
    if (!knn_force_valu()) {
      if (vec) dg::launch((knn_mfma_kernel<CP, KC, true>), s.grid(ROWS), dim3(256), 0, a.st, a.x, a.sq(), N, a.C, a.ldx, a.k, a.idx, tau0);
      else dg::launch((knn_mfma_kernel<CP, KC, false>), s.grid(ROWS), dim3(256), 0, a.st, a.x, a.sq(), N, a.C, a.ldx, a.k, a.idx, tau0);
      return;
    }
  }
  dg::launch((knn_kernel<CP, KC, Clouds>), s.grid(ROWS), dim3(256), 0, a.st, a.x, a.sq(), s.cl, a.C, a.ldx, a.k, a.vec_ok, a.idx,
             (CP <= 4) ? tau0 : (const float*)nullptr);
}

template <int CP, class Clouds>
void launch_scan_k(const CloudSet<Clouds>& s, const KnnCall& a, const float* tau0) {
  if (a.k <= 8) launch_scan<CP, 8>(s, a, tau0);
  else if (a.k <= 20) launch_scan<CP, 20>(s, a, tau0);
  else if (a.k <= 40 || CloudSet<Clouds>::kRawOnly) launch_scan<CP, 40>(s, a, tau0);
  else if constexpr (!CloudSet<Clouds>::kRawOnly) launch_scan<CP, 64>(s, a, tau0);
}

// The all-pairs search of one set of clouds, s_i already in the workspace.  seed: null, or the graph that the entry's seeding rule
// admitted; append: the append-form scan may take the shape (knn_append_usable, and the workspace holds its scratch).
template <class Clouds>
int knn_scan(const CloudSet<Clouds>& s, const KnnCall& a, const int32_t* seed, int64_t ldseed, bool append) {
  const float* tau0 = nullptr;
  if constexpr (!CloudSet<Clouds>::kRawOnly) {
    if (knn_bigk_takes(a.k)) {               // k > 64, or the switch: the large-k scan; it takes no bound (a seed is ignored)
      const int32_t* off = nullptr;          // dense clouds
      if constexpr (!CloudSet<Clouds>::kDense) off = s.cl.off;
      dg::launch_knn_bigk(a.x, a.sq(), off, s.ny, s.max_n, a.C, a.ldx, a.k, a.vec_ok, a.idx, a.w.entries(), a.st);
      return dg::check_launch(a.what);
    }
    // the bound of the first k seeds of every row (C in {16, 32, 64}; otherwise none)
    if (seed && launch_seed_bound(a.x, a.sq(), s.rows, s.cl, a.C, a.ldx, seed, ldseed, a.k, a.w.bounds(), a.st)) tau0 = a.w.bounds();
  }
  if constexpr (CloudSet<Clouds>::kRawOnly) launch_scan_k<4>(s, a, launch_hist_bound(s, a));
  else if (tau0 && append) launch_append_scan(s, a, tau0);
  else if (knn_wide_takes(a.C)) {            // wide rows, or the switch: the channel-slab scan; it takes no bound (a seed is ignored)
    const int32_t* off = nullptr;            // dense clouds
    if constexpr (!CloudSet<Clouds>::kDense && !CloudSet<Clouds>::kRawOnly) off = s.cl.off;
    dg::launch_knn_wide(a.x, a.sq(), off, s.ny, s.max_n, a.C, a.ldx, a.k, a.vec_ok, a.idx, a.st);
  }
  else if (a.C <= 4) launch_scan_k<4>(s, a, launch_hist_bound(s, a));
  else if (a.C <= 16) launch_scan_k<16>(s, a, tau0);
  else if (a.C <= 64) launch_scan_k<64>(s, a, tau0);
  else launch_scan_k<128>(s, a, tau0);
  return dg::check_launch(a.what);
}

// the append-form scan takes 16 < C <= 64 on float4-loadable rows, unless a switch turns it or the bf16 matrix pipe off
bool knn_append_usable(const KnnCall& a) {
  return knn_append_on() && knn_append_shape(a.C, a.k) && a.vec_ok && !knn_force_valu() && knn_bf16f_mode() != 0 && a.w.holds(a.w.end);
}
// The two seeding rules.  Both need kseed >= k seeds per row and 32-bit element offsets within a cloud; dgcnn_knn_seed_min_n overrides
// the cloud size from which either applies.
// Dense: seeds are used by the list-keeping and matrix-pipe scans (4 < C <= 64, float4-loadable rows) from N >= 4096 without the append
// form, and from any N with it (the measurements: at DGCNN_KNN_SEED_MIN_N).
bool knn_seeds_used_dense(const KnnCall& a, const int32_t* seed, int kseed, int N, bool append) {
  const int min_n = knn_seed_min_n() >= 0 ? knn_seed_min_n() : (append ? 0 : 4096);
  return seed && kseed >= a.k && kseed <= 64 && a.C > 4 && a.C <= 64 && a.C % 4 == 0 && a.vec_ok && !knn_force_valu() && N >= min_n &&
         (int64_t)N * a.ldx < ((int64_t)1 << 31) && a.w.bounds();
}
// Packed: seeds are used only together with the append form (the packed list-keeping scan takes no seed bound).
bool knn_seeds_used_packed(const KnnCall& a, const int32_t* seed, int kseed, int min_n, int max_n, bool append) {
  const int seed_min = knn_seed_min_n() >= 0 ? knn_seed_min_n() : 0;
  return append && seed && kseed >= a.k && kseed <= 64 && min_n >= seed_min && (int64_t)max_n * a.ldx < ((int64_t)1 << 31);
}

int knn_impl(const char* what, const float* x, int B, int N, int C, int64_t ldx, int k, const int32_t* seed, int64_t ldseed, int kseed,
             int32_t* idx, void* ws, size_t ws_bytes, void* stream) {
  DG_REQUIRE(x && idx && ws, DGCNN_EINVAL, "%s: null pointer", what);
  DG_REQUIRE(B > 0 && N > 0 && C > 0 && ldx >= C, DGCNN_EINVAL, "%s: bad shape B=%d N=%d C=%d", what, B, N, C);
  DG_REQUIRE(k > 0 && k <= N, DGCNN_EINVAL, "%s: k=%d must be in [1, N=%d] (tf.nn.top_k raises otherwise)", what, k, N);
  DG_REQUIRE(k <= KNN_MAX_K, DGCNN_EUNSUP, "%s: k=%d > %d unsupported", what, k, KNN_MAX_K);
  DG_REQUIRE(C <= KNN_MAX_C, DGCNN_EUNSUP, "%s: C=%d > %d unsupported", what, C, KNN_MAX_C);
  DG_REQUIRE(C <= 128 || !knn_force_valu(), DGCNN_EUNSUP, "%s: C=%d > 128 unsupported by the VALU scan (dgcnn_knn_force_valu)", what, C);
  DG_REQUIRE(k <= 64 || !knn_force_valu(), DGCNN_EUNSUP, "%s: k=%d > 64 unsupported by the VALU scan (dgcnn_knn_force_valu)", what, k);
  const KnnCall a{what, x, C, ldx, k, knn_vec_ok(x, ldx), idx, knn_ws_dense(ws, ws_bytes, B, N, C, k), (hipStream_t)stream};
  const bool bigk = knn_bigk_takes(k);       // the large-k scan keeps its row buffers in the workspace: all of it is required
  DG_REQUIRE(a.w.aligned() && a.w.holds(C > 128 || bigk ? a.w.end : a.w.bound), DGCNN_EINVAL,
             "%s: workspace must be 16-byte aligned and hold dgcnn_knn_workspace_bytes(B, N, C, k) bytes (got %zu)", what, ws_bytes);
  const CloudSet<DenseClouds> s{DenseClouds(N), B, N, N, (int64_t)B * N};
  const bool append = !bigk && knn_append_usable(a);
  const bool seeded = !bigk && knn_seeds_used_dense(a, seed, kseed, N, append);
  launch_sqnorm(a, s.rows);
  // raw coordinates (C <= 4) when the caller provided the scratch: exact search over a uniform cell grid (knn_grid.hip)
  if (!bigk && dg::knn_grid_applicable(C, k) && !knn_force_valu() && a.w.holds(a.w.end) && N >= dg::knn_grid_min_n())
    return dg::launch_knn_grid(x, a.sq(), B, N, C, ldx, k, idx, a.w.grid(), a.st);
  return knn_scan(s, a, seeded ? seed : nullptr, ldseed, append);
}

// The argument rules that the three packed-tower entries share, in the order they report them.  grid: the entry searches (some of) the
// clouds with the cell grid.  mix: null, or the grid class of dgcnn_knn_seg_mix_f32 -- min_n / max_n then describe its scan class.
struct GridClass { int n, max_n; };
int knn_check_tower(const char* what, bool pointers, int nseg, int rows, int C, int64_t ldx, int k, bool grid, int min_n, int max_n,
                    const GridClass* mix = nullptr) {
  DG_REQUIRE(pointers, DGCNN_EINVAL, "%s: null pointer", what);
  DG_REQUIRE(nseg > 0 && nseg <= 65535 && rows > 0 && C > 0 && ldx >= C, DGCNN_EINVAL, "%s: bad shape nseg=%d rows=%d C=%d", what,
             nseg, rows, C);
  DG_REQUIRE(!grid || (C <= 4 && k <= 40), DGCNN_EINVAL, "%s: C=%d k=%d: the cell grid searches raw coordinates (C <= 4) for k <= 40",
             what, C, k);
  int smallest = min_n;
  if (mix) {
    const int nscan = nseg - mix->n;
    DG_REQUIRE(mix->n > 0 && mix->n < nseg, DGCNN_EINVAL,
               "%s: n_grid=%d must be in [1, nseg=%d): a tower of one class goes to dgcnn_knn_seg_f32 or dgcnn_knn_seg_grid_f32", what,
               mix->n, nseg);
    DG_REQUIRE(mix->max_n > 0 && min_n > 0 && min_n <= max_n && (int64_t)mix->max_n + (int64_t)min_n * nscan <= rows &&
                   (int64_t)mix->max_n * mix->n + (int64_t)max_n * nscan >= rows,
               DGCNN_EINVAL, "%s: cloud sizes grid_max_n=%d scan_min_n=%d scan_max_n=%d do not fit %d rows in %d + %d clouds", what,
               mix->max_n, min_n, max_n, rows, mix->n, nscan);
    if (mix->max_n < smallest) smallest = mix->max_n;
  } else {
    DG_REQUIRE(min_n > 0 && min_n <= max_n && max_n <= rows && (int64_t)min_n * nseg <= rows && (int64_t)max_n * nseg >= rows,
               DGCNN_EINVAL, "%s: cloud sizes min_n=%d max_n=%d do not fit %d rows in %d clouds", what, min_n, max_n, rows, nseg);
  }
  DG_REQUIRE(k > 0 && k <= smallest, DGCNN_EINVAL, "%s: k=%d must be in [1, smallest cloud=%d] (tf.nn.top_k raises otherwise)", what, k,
             smallest);
  return DGCNN_OK;
}

}  // namespace

extern "C" int64_t dgcnn_knn_workspace_bytes(int B, int N, int C, int k) {
  return (B <= 0 || N <= 0) ? 0 : (int64_t)knn_ws_dense(nullptr, 0, B, N, C, k).end;
}

extern "C" int dgcnn_knn_f32(const float* x, int B, int N, int C, int64_t ldx, int k, int32_t* idx,
                             void* ws, size_t ws_bytes, void* stream) {
  return knn_impl("dgcnn_knn_f32", x, B, N, C, ldx, k, nullptr, 0, 0, idx, ws, ws_bytes, stream);
}

// The same search, seeded: `seed` (B, N, >= kseed; row stride ldseed) lists kseed >= k DISTINCT candidates of every row (any:
// the previous EdgeConv layer's graph in dgcnn/ops.py:95-96's stack).  Their largest distance bounds the row's k-th distance from
// above, so the scan can drop farther candidates from its first tile on instead of inserting them into lists that are still
// filling up (~k (1 + ln(N / k)) inserts per row become ~k + the candidates between the k-th distance and the bound).  The result
// is the unseeded one bit for bit; rows whose seeds are not distinct in-range indices simply get no bound.
extern "C" int dgcnn_knn_seeded_f32(const float* x, int B, int N, int C, int64_t ldx, int k, const int32_t* seed, int64_t ldseed,
                                    int kseed, int32_t* idx, void* ws, size_t ws_bytes, void* stream) {
  DG_REQUIRE(!seed || (ldseed >= kseed && kseed > 0), DGCNN_EINVAL, "dgcnn_knn_seeded_f32: bad seed shape");
  return knn_impl("dgcnn_knn_seeded_f32", x, B, N, C, ldx, k, seed, ldseed, kseed, idx, ws, ws_bytes, stream);
}

// ---- packed towers: clouds of different sizes concatenated row-wise, cloud b = rows [seg_off[b], seg_off[b + 1]) -----------------
// The dense dispatch over PackedClouds (a block maps to its cloud's base and size instead of b N and N).
extern "C" int64_t dgcnn_knn_seg_workspace_bytes(int rows, int max_n, int C, int k) {
  return (rows <= 0 || max_n <= 0) ? 0 : (int64_t)knn_ws_seg(nullptr, 0, rows, max_n, C, k).end;
}

extern "C" int dgcnn_knn_seg_f32(const float* x, int64_t ldx, int C, int k, int nseg, const int32_t* seg_off, int rows, int min_n,
                                 int max_n, const int32_t* seed, int64_t ldseed, int kseed, int32_t* idx, void* ws, size_t ws_bytes,
                                 void* stream) {
  const char* what = "dgcnn_knn_seg_f32";
  if (const int rc = knn_check_tower(what, x && idx && ws && seg_off, nseg, rows, C, ldx, k, false, min_n, max_n)) return rc;
  DG_REQUIRE(k <= KNN_MAX_K, DGCNN_EUNSUP, "%s: k=%d > %d unsupported", what, k, KNN_MAX_K);
  DG_REQUIRE(C <= KNN_MAX_C, DGCNN_EUNSUP, "%s: C=%d > %d unsupported", what, C, KNN_MAX_C);
  DG_REQUIRE(C <= 128 || !knn_force_valu(), DGCNN_EUNSUP, "%s: C=%d > 128 unsupported by the VALU scan (dgcnn_knn_force_valu)", what, C);
  DG_REQUIRE(k <= 64 || !knn_force_valu(), DGCNN_EUNSUP, "%s: k=%d > 64 unsupported by the VALU scan (dgcnn_knn_force_valu)", what, k);
  DG_REQUIRE(!seed || (ldseed >= kseed && kseed > 0), DGCNN_EINVAL, "%s: bad seed shape", what);
  const KnnCall a{what, x, C, ldx, k, knn_vec_ok(x, ldx), idx, knn_ws_seg(ws, ws_bytes, rows, max_n, C, k), (hipStream_t)stream};
  const bool bigk = knn_bigk_takes(k);       // the large-k scan keeps its row buffers in the workspace: all of it is required
  DG_REQUIRE(a.w.aligned() && a.w.holds(C > 128 || bigk ? a.w.end : a.w.bound), DGCNN_EINVAL,
             "%s: workspace must be 16-byte aligned and hold dgcnn_knn_seg_workspace_bytes(rows, max_n, C, k) bytes (got %zu)", what,
             ws_bytes);
  const CloudSet<PackedClouds> s{PackedClouds{seg_off, nseg}, nseg, min_n, max_n, (int64_t)rows};
  const bool append = !bigk && knn_append_usable(a);
  const bool seeded = !bigk && knn_seeds_used_packed(a, seed, kseed, min_n, max_n, append);
  launch_sqnorm(a, s.rows);
  return knn_scan(s, a, seeded ? seed : nullptr, ldseed, append);
}

// ---- packed towers, raw coordinates (C <= 4, k <= 40): the exact cell-grid search of knn_grid.hip with one grid per cloud ---------
// No seed: the grid never used one.  dgcnn_knn_seg_grid_use (knn_grid.hip) is the rule by which a caller chooses between this entry
// and dgcnn_knn_seg_f32; the indices are the same either way.
extern "C" int64_t dgcnn_knn_seg_grid_workspace_bytes(int rows, int nseg) {
  return (rows <= 0 || nseg <= 0) ? 0 : (int64_t)knn_ws_seg_grid(nullptr, 0, rows, nseg).end;
}

extern "C" int dgcnn_knn_seg_grid_f32(const float* x, int64_t ldx, int C, int k, int nseg, const int32_t* seg_off, int rows, int min_n,
                                      int max_n, int32_t* idx, void* ws, size_t ws_bytes, void* stream) {
  const char* what = "dgcnn_knn_seg_grid_f32";
  if (const int rc = knn_check_tower(what, x && idx && ws && seg_off, nseg, rows, C, ldx, k, true, min_n, max_n)) return rc;
  const KnnCall a{what, x, C, ldx, k, knn_vec_ok(x, ldx), idx, knn_ws_seg_grid(ws, ws_bytes, rows, nseg), (hipStream_t)stream};
  DG_REQUIRE(a.w.aligned() && a.w.holds(a.w.end), DGCNN_EINVAL,
             "%s: workspace must be 16-byte aligned and hold dgcnn_knn_seg_grid_workspace_bytes(rows, nseg) bytes (got %zu)", what, ws_bytes);
  launch_sqnorm(a, rows);
  return dg::launch_knn_grid_seg(x, a.sq(), nseg, seg_off, rows, max_n, C, ldx, k, idx, a.w.grid(), a.st);
}

// ---- packed towers, raw coordinates: every cloud through the search that suits its own size, in one call ----------------------------
// cloud_list (device, nseg int32) names the tower's clouds in two classes: the first n_grid go through the cell grid, the others through
// the all-pairs scan with the histogram bound; both sub-searches are the kernels of the two entries above instantiated with
// ListedClouds (knn_common.h), launched over their own class only -- grids cdiv(grid_max_n, 256) x n_grid and cdiv(scan_max_n, 64) x
// (nseg - n_grid), so a small cloud launches no row of blocks for the large ones and owns no cell table.  A pair's D has the same bits
// in either kernel and both select by (D, j): idx is dgcnn_knn_seg_f32's and dgcnn_knn_seg_grid_f32's, bit for bit.  The histogram
// bounds are those of the scan rows; the grid's records, s_j and original indices (24 bytes per row) are indexed by tower row.
extern "C" int64_t dgcnn_knn_seg_mix_workspace_bytes(int rows, int n_grid) {
  return (rows <= 0 || n_grid <= 0) ? 0 : (int64_t)knn_ws_seg_mix(nullptr, 0, rows, n_grid).end;
}

extern "C" int dgcnn_knn_seg_mix_f32(const float* x, int64_t ldx, int C, int k, int nseg, const int32_t* seg_off, int rows,
                                     const int32_t* cloud_list, int n_grid, int grid_max_n, int scan_min_n, int scan_max_n,
                                     int32_t* idx, void* ws, size_t ws_bytes, void* stream) {
  const char* what = "dgcnn_knn_seg_mix_f32";
  const GridClass g{n_grid, grid_max_n};
  if (const int rc = knn_check_tower(what, x && idx && ws && seg_off && cloud_list, nseg, rows, C, ldx, k, true, scan_min_n, scan_max_n, &g))
    return rc;
  const KnnCall a{what, x, C, ldx, k, knn_vec_ok(x, ldx), idx, knn_ws_seg_mix(ws, ws_bytes, rows, n_grid), (hipStream_t)stream};
  DG_REQUIRE(a.w.aligned() && a.w.holds(a.w.end), DGCNN_EINVAL,
             "%s: workspace must be 16-byte aligned and hold dgcnn_knn_seg_mix_workspace_bytes(rows, n_grid) bytes (got %zu)", what, ws_bytes);
  launch_sqnorm(a, rows);
  const int rc = dg::launch_knn_grid_listed(what, x, a.sq(), seg_off, cloud_list, n_grid, rows, grid_max_n, C, ldx, k, idx, a.w.grid(), a.st);
  if (rc != 0) return rc;
  const int nscan = nseg - n_grid;
  return knn_scan(CloudSet<ListedClouds>{ListedClouds{seg_off, cloud_list + n_grid, nscan}, nscan, scan_min_n, scan_max_n, (int64_t)rows},
                  a, nullptr, 0, false);
}

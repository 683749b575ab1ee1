// knn_scan.h -- the pieces that the all-pairs scan kernels of knn.hip, knn_wide.hip, knn_bigk.hip and knn_cross.hip have in common,
// each once: the thread mapping and D layout of the matrix-pipe forms, the guarded row-quad load, the channel-slab stage and its MFMA
// step (and its two-source sibling for the search between two sets), the distance, park / flag / drain, the bf16 query planes and
// the 4-list merge with the index (and distance) write-out.  The bit-exactness and non-finite-input arguments of these blocks are
// written here, at the function.
// ONE SECOND COPY EXISTS: knn.hip:knn_mfma_kernel keeps its own text of the mapping, the guarded load, shared_bound, park_and_flag,
// drain_parked (all 16 slots at once) and merge_lists_write, for speed (said there).  A change to one of these functions -- a
// non-finite-input fix above all -- has to be made in that kernel too.  knn_bigk_kernel writes out ScanLane's mapping lines.
//
// MUST be compiled with -ffp-contract=off (csrc/Makefile).  The arithmetic is the normative one of oracle/knn_oracle.c:
//     s_i  = sequential sum of fl(x*x) over c ascending (no FMA)
//     p_ij = fmaf chain over c = 0 .. C-1 from +0
//     D_ij = fl( fl(s_i + s_j) - 2 p_ij )
#pragma once
#include "knn_common.h"

namespace {

constexpr int ROWS = 64;                     // query rows per block, in every scan kernel

using f32x16 = __attribute__((ext_vector_type(16))) float;

// ---- thread mapping of the matrix-pipe forms: block = 64 query rows x 2 candidate halves (4 waves of 64) -------------------------
// D layout of the 32x32 MFMAs: lane l holds query row (l & 31) of its wave's 32 and, in accumulator r = 0..15, candidate
// d_layout_index(r, l >> 5) of its wave's 32: two lanes per row, so a query row has 4 (d, j) lists -- 2 lane halves x 2 candidate
// halves -- with list 0 in lanes 0..31 of waves 0 and 1.
struct ScanLane {
  int tid, lane, w;
  int l31, h;                                // lane & 31 = query row of the wave, lane >> 5 = which half of the D layout
  int qg;                                    // which 32 query rows of the block
  int cs;                                    // which 32 candidates of every 64-candidate tile
  int cbase;                                 // = 32 cs
  int lid;                                   // list id of this lane among the 4 lists of its row
  int rslot;                                 // row within the block
  __device__ __forceinline__ ScanLane()
      : tid(threadIdx.x), lane(tid & 63), w(tid >> 6), l31(lane & 31), h(lane >> 5), qg(w & 1), cs(w >> 1), cbase(cs * 32),
        lid(cs * 2 + h), rslot(qg * 32 + l31) {}
};
__device__ __forceinline__ constexpr int d_layout_index(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

template <int KC>
__device__ __forceinline__ void list_init(float (&dl)[KC], int (&jl)[KC]) {
#pragma unroll
  for (int t = 0; t < KC; ++t) {
    dl[t] = INFINITY;
    jl[t] = 0x7fffffff;                      // open slot: the sentinel of fill_short_list (knn_common.h)
  }
}

// D = fl(t - 2 p), t = fl(s_i + s_j), in ONE rounding: 2 p is exact, so the fused form equals the oracle's  t - fl(2 p)  bit for bit.
__device__ __forceinline__ float scan_dist(float p, float si, float sj) {
  const float tt = si + sj;
  return __builtin_fmaf(-2.0f, p, tt);
}

// ---- one float4 of row r of the cloud at channels ch .. ch + 3, zero past C ------------------------------------------------------
// VEC (16-byte aligned rows, C % 4 == 0): one unconditional load from a clamped, always valid address (r < N is the caller's clamp,
// channel quads past C read the row's last quad and are zeroed).  Otherwise element by element, and only if `live`.  A value loaded
// is only ever an operand: no address depends on it.
template <bool VEC>
__device__ __forceinline__ float4 load_row_quad(const float* __restrict__ xb, int64_t ldx, int r, int ch, int C, bool live) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (VEC) {
    const int cc = ch < C ? ch : C - 4;
    const float4 t4 = *reinterpret_cast<const float4*>(xb + (int64_t)r * ldx + cc);
    const bool ok = ch < C;
    v.x = ok ? t4.x : 0.f; v.y = ok ? t4.y : 0.f; v.z = ok ? t4.z : 0.f; v.w = ok ? t4.w : 0.f;
  } else if (live) {
    const float* src = xb + (int64_t)r * ldx + ch;
    if (ch + 0 < C) v.x = src[0];
    if (ch + 1 < C) v.y = src[1];
    if (ch + 2 < C) v.z = src[2];
    if (ch + 3 < C) v.w = src[3];
  }
  return v;
}

// ---- channel-slab stage (knn_wide_kernel, knn_bigk_kernel) --------------------------------------------------------------------------
// Every step of the flattened (tile, slab) sequence stages TWO k-major slab tiles [64 channels][66], double buffered: 64 candidates'
// and the block's own 64 query rows' (a re-read that hits L2: a block's query rows are 64 C floats, <= 256 KB).  The query slab in
// the candidates' layout makes the B operand the same conflict-free ds_read_b32 as the A operand (lane = row, one channel per
// instruction); a direct per-lane load from global memory would be 32 strided 4-byte loads of 32 different lines per
// wave-instruction per step, and an LDS copy of the whole rows fits only to C ~ 256.
//   fetch: global -> registers, one step ahead;  stash: registers -> the other LDS buffer, transposed ([c][row]), after the current
//   step's MFMAs; one barrier per step.  `tiles` = 4 TILE_F floats ([buffer][candidates | queries]), `sjs` = [2][TJM] by tile parity.
// Candidate rows past N repeat row N - 1 and carry |x_j|^2 = +inf (never selected); query rows past N repeat row N - 1 (never
// written); channel quads past C are +0 on both operands: fmaf(0, 0, p) = p for every p (NaN and infinities included), so a partly
// filled last slab changes nothing.
// v_mfma_f32_32x32x2_f32 is bit for bit an fmaf chain in k order on gfx950, and its accumulator input is never rounded or flushed,
// so the 16 accumulators of a 64-candidate tile carried through slab_mfma from slab s to slab s + 1 ARE the oracle's chain over all
// C channels.
template <bool VEC>
struct SlabStage {
  static constexpr int SL = 64;              // channels per slab
  static constexpr int TJM = 64;             // candidates per tile: 32 per candidate-half wave
  static constexpr int ST = TJM + 2;         // k-major slab tile [SL][ST]
  static constexpr int TILE_F = SL * ST;
  static constexpr int NV = (TJM * (SL / 4)) / 256;   // float4 staged per thread per slab tile

  const float* __restrict__ xb;              // the cloud's first row
  const float* __restrict__ sqb;             // ... and its s_i
  int64_t ldx;
  int N, C, row0, tid;
  float* tiles;
  float* sjs;
  float4 prec[NV], preq[NV];
  float pre_s = INFINITY;

  __device__ __forceinline__ SlabStage(const float* xb_, const float* sqb_, int64_t ldx_, int N_, int C_, int row0_, int tid_,
                                       float* tiles_, float* sjs_)
      : xb(xb_), sqb(sqb_), ldx(ldx_), N(N_), C(C_), row0(row0_), tid(tid_), tiles(tiles_), sjs(sjs_) {}

  __device__ __forceinline__ void fetch(int j0, int c0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int e = tid + 256 * i;
      const int r = e >> 4;
      const int ch = c0 + (e & 15) * 4;
      const int j = j0 + r, q = row0 + r;
      prec[i] = load_row_quad<VEC>(xb, ldx, j < N ? j : N - 1, ch, C, j < N);
      preq[i] = load_row_quad<VEC>(xb, ldx, q < N ? q : N - 1, ch, C, true);
    }
    if (c0 == 0 && tid < TJM) pre_s = (j0 + tid < N) ? sqb[j0 + tid] : INFINITY;
  }
  __device__ __forceinline__ void stash(int buf, int tpar, bool first_slab) {
    float* dc = tiles + buf * 2 * TILE_F;
    float* dqr = dc + TILE_F;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int e = tid + 256 * i;
      const int r = e >> 4;
      const int c4 = (e & 15) * 4;
      dc[(c4 + 0) * ST + r] = prec[i].x;
      dc[(c4 + 1) * ST + r] = prec[i].y;
      dc[(c4 + 2) * ST + r] = prec[i].z;
      dc[(c4 + 3) * ST + r] = prec[i].w;
      dqr[(c4 + 0) * ST + r] = preq[i].x;
      dqr[(c4 + 1) * ST + r] = preq[i].y;
      dqr[(c4 + 2) * ST + r] = preq[i].z;
      dqr[(c4 + 3) * ST + r] = preq[i].w;
    }
    if (first_slab && tid < TJM) sjs[tpar * TJM + tid] = pre_s;
  }
  // The 32 MFMAs of one slab on buffer `buf`: A = candidate cbase + l31, B = query row rslot, channel 2 s2 + h at step s2.  Both
  // operands run through a ring two MFMAs deep -- the operands of step s2 + 2 are requested right behind MFMA s2, whose 64 clocks in
  // the pipe (the chain is dependent) cover the LDS round trip -- so the query operand costs 2 VGPRs instead of 32.
  __device__ __forceinline__ void slab_mfma(f32x16& acc, int buf, const ScanLane& m) const {
    const float* ap = tiles + buf * 2 * TILE_F + m.h * ST + m.cbase + m.l31;
    const float* bp = tiles + buf * 2 * TILE_F + TILE_F + m.h * ST + m.qg * 32 + m.l31;
    constexpr int NS = SL / 2;
    float a0 = ap[0], b0 = bp[0], a1 = ap[2 * ST], b1 = bp[2 * ST];
#pragma unroll
    for (int s2 = 0; s2 < NS; s2 += 2) {
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc, 0, 0, 0);
      if (s2 + 2 < NS) { a0 = ap[2 * (s2 + 2) * ST]; b0 = bp[2 * (s2 + 2) * ST]; }
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc, 0, 0, 0);
      if (s2 + 3 < NS) { a1 = ap[2 * (s2 + 3) * ST]; b1 = bp[2 * (s2 + 3) * ST]; }
    }
  }
};

// ---- the same stage with TWO operand sources and a slab width of its own (knn_cross.hip:knn_cross_kernel) ----------------------------
// SlabStage with the ties between its two tiles cut: the query tile comes from (qb, ldq), rows clamped to M - 1 (never written past
// M), the candidate tile from (pb, ldp), rows clamped to N - 1 with |p_j|^2 = +inf past N, from spb.  SLV = channels per slab, 64 or
// 16: a 16-channel slab is one float4 per thread per tile and 8 MFMAs where the 64-channel one is four and 32, for rows of at most 16
// channels (raw coordinates above all); the zero channels past C change nothing, as said at SlabStage.  Layout, fetch / stash protocol
// and the MFMA ring are SlabStage's, line for line; with qb == pb, ldq == ldp, M == N and SLV = 64 the two stage the same floats.
template <bool VEC, int SLV>
struct CrossSlabStage {
  static_assert(SLV == 16 || SLV == 64, "CrossSlabStage: slabs of 16 or 64 channels");
  static constexpr int SL = SLV;             // channels per slab
  static constexpr int TJM = 64;             // candidates per tile: 32 per candidate-half wave
  static constexpr int ST = TJM + 2;         // k-major slab tile [SL][ST]
  static constexpr int TILE_F = SL * ST;
  static constexpr int QR = SL / 4;          // float4 per row per slab
  static constexpr int NV = (TJM * QR) / 256;   // float4 staged per thread per slab tile

  const float* __restrict__ qb;              // the query cloud's first row
  const float* __restrict__ pb;              // the candidate cloud's first row
  const float* __restrict__ spb;             // ... and its s_j
  int64_t ldq, ldp;
  int M, N, C, row0, tid;
  float* tiles;
  float* sjs;
  float4 prec[NV], preq[NV];
  float pre_s = INFINITY;

  __device__ __forceinline__ CrossSlabStage(const float* qb_, int64_t ldq_, int M_, const float* pb_, const float* spb_, int64_t ldp_,
                                            int N_, int C_, int row0_, int tid_, float* tiles_, float* sjs_)
      : qb(qb_), pb(pb_), spb(spb_), ldq(ldq_), ldp(ldp_), M(M_), N(N_), C(C_), row0(row0_), tid(tid_), tiles(tiles_), sjs(sjs_) {}

  __device__ __forceinline__ void fetch(int j0, int c0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int e = tid + 256 * i;
      const int r = e / QR;
      const int ch = c0 + (e % QR) * 4;
      const int j = j0 + r, q = row0 + r;
      prec[i] = load_row_quad<VEC>(pb, ldp, j < N ? j : N - 1, ch, C, j < N);
      preq[i] = load_row_quad<VEC>(qb, ldq, q < M ? q : M - 1, ch, C, true);
    }
    if (c0 == 0 && tid < TJM) pre_s = (j0 + tid < N) ? spb[j0 + tid] : INFINITY;
  }
  __device__ __forceinline__ void stash(int buf, int tpar, bool first_slab) {
    float* dc = tiles + buf * 2 * TILE_F;
    float* dqr = dc + TILE_F;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int e = tid + 256 * i;
      const int r = e / QR;
      const int c4 = (e % QR) * 4;
      dc[(c4 + 0) * ST + r] = prec[i].x;
      dc[(c4 + 1) * ST + r] = prec[i].y;
      dc[(c4 + 2) * ST + r] = prec[i].z;
      dc[(c4 + 3) * ST + r] = prec[i].w;
      dqr[(c4 + 0) * ST + r] = preq[i].x;
      dqr[(c4 + 1) * ST + r] = preq[i].y;
      dqr[(c4 + 2) * ST + r] = preq[i].z;
      dqr[(c4 + 3) * ST + r] = preq[i].w;
    }
    if (first_slab && tid < TJM) sjs[tpar * TJM + tid] = pre_s;
  }
  // SL / 2 MFMAs on buffer `buf`: A = candidate cbase + l31, B = query row rslot, channel 2 s2 + h at step s2 (SlabStage::slab_mfma)
  __device__ __forceinline__ void slab_mfma(f32x16& acc, int buf, const ScanLane& m) const {
    const float* ap = tiles + buf * 2 * TILE_F + m.h * ST + m.cbase + m.l31;
    const float* bp = tiles + buf * 2 * TILE_F + TILE_F + m.h * ST + m.qg * 32 + m.l31;
    constexpr int NS = SL / 2;
    float a0 = ap[0], b0 = bp[0], a1 = ap[2 * ST], b1 = bp[2 * ST];
#pragma unroll
    for (int s2 = 0; s2 < NS; s2 += 2) {
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc, 0, 0, 0);
      if (s2 + 2 < NS) { a0 = ap[2 * (s2 + 2) * ST]; b0 = bp[2 * (s2 + 2) * ST]; }
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc, 0, 0, 0);
      if (s2 + 3 < NS) { a1 = ap[2 * (s2 + 3) * ST]; b1 = bp[2 * (s2 + 3) * ST]; }
    }
  }
};

// ---- shared selection bound, park / flag / drain over the D layout: NP slots of a lane's 16 at a time (knn_wide_kernel: two halves
// of 8, the only caller; knn_mfma_kernel's own copy does all 16 at once) ----
// The candidates of a query row are split over FOUR sorted lists (KC entries each, KC % 4 == 0).  If every list holds at least KC/4
// entries, the row has seen KC candidates with d <= tau := max_i list_i[KC/4 - 1], so a candidate with d > tau has KC candidates
// strictly before it in (d, j) order and can never enter the row's top KC: dropping it is exact.  Candidates with d == tau pass (the
// tie is decided by index in the merge), hence the filter  d < min(own k-th, next_up(tau)).  tau is about the row's GLOBAL k-th
// distance (the KC/4-th best of a quarter of the candidates), where a list's own k-th is about the global 4k-th: ~2.5x fewer
// inserts.  The lists publish list_i[KC/4 - 1] in `thrw` ([4 lists][64 rows]) once per tile; a stale (older = larger) value only
// makes the filter looser.  o1..o3 = the other three lists' entries.
template <int KC>
__device__ __forceinline__ float shared_bound(const float (&dl)[KC], float o1, float o2, float o3) {
  return next_up(fmaxf(fmaxf(dl[KC / 4 - 1], o1), fmaxf(o2, o3)));
}
// Distances of accumulators off .. off + NP - 1 of this lane: parked in dq[slot][tid], bit `slot` of the result set where d < thr
// (the candidate can still enter the row's top KC).  sj = the tile's s_j at this lane's first candidate (cbase + 4 h).
// Non-finite input: d < thr is false for NaN and +inf, so such a distance sets no bit and is never listed.
template <int NP>
__device__ __forceinline__ unsigned park_and_flag(const f32x16& acc, int off, float si, const float* sj, float thr, float* dq, int tid) {
  unsigned mask = 0u;
#pragma unroll
  for (int q = 0; q < NP / 4; ++q) {
    const float4 s4 = *reinterpret_cast<const float4*>(sj + 8 * (off / 4 + q));     // candidates 8 (off / 4 + q) + 4 h + (0..3)
    const float sv[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = 4 * q + e;
      const float d = scan_dist(acc[off + r], si, sv[e]);
      dq[r * 256 + tid] = d;
      mask |= sel_01(m_flt(d, thr)) << r;
    }
  }
  return mask;
}
// Drain: every iteration each lane pops ITS lowest flagged slot -- ascending j, the order the strict insert's tie rule needs -- and
// all lanes run one insert.  The parked distance of the NEXT flagged slot is fetched before the insert of the current one (LDS round
// trip hidden behind ~90 VALU ops).  jbase = cloud-local j of the wave's first candidate of the tile.  The loop pops one bit per
// iteration whatever the distances are; a lane with no bit left inserts d = +inf, a no-op.
template <int KC, int NP>
__device__ __forceinline__ void drain_parked(float (&dl)[KC], int (&jl)[KC], unsigned mask, const float* dq, int tid, int off, int h,
                                             int jbase) {
  int g = __builtin_ctz(mask | 0x80000000u) & (NP - 1);
  float dcur = dq[g * 256 + tid];
  while (__any(mask != 0u)) {
    const lmask_t live = m_ine((int)mask, 0);
    const int gc = g + off;
    mask &= mask - 1u;
    g = __builtin_ctz(mask | 0x80000000u) & (NP - 1);
    const float dnext = dq[g * 256 + tid];
    const float d = sel_f(live, dcur, INFINITY);
    list_insert<KC, false>(dl, jl, d, jbase + d_layout_index(gc, h));
    dcur = dnext;
  }
}

// ---- query row into two bf16 planes (knn_bf16f_kernel, knn_bf16a_kernel) ---------------------------------------------------------------
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

__device__ __forceinline__ unsigned cvt_pk_bf16(float lo, float hi) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}
// (x0, x1) -> packed bf16 pairs of the two leading split terms
__device__ __forceinline__ void split2_pair(float x0, float x1, unsigned& h, unsigned& m) {
  h = cvt_pk_bf16(x0, x1);
  const float r0 = x0 - __uint_as_float(h << 16);
  const float r1 = x1 - __uint_as_float(h & 0xffff0000u);
  m = cvt_pk_bf16(r0, r1);
}
// B operand of v_mfma_f32_32x32x16_bf16: this lane's query row (float4-loadable, C % 4 == 0), channels 16 s + 8 h + (0..7), zero past
// C, as its two leading bf16 terms q1 + q2.  The planes only feed a conservative filter: what passes is decided by the exact distance.
__device__ __forceinline__ void split_query_planes(const float* __restrict__ xi_row, int C, int h, bf16x8 (&q1)[4], bf16x8 (&q2)[4]) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int c = 16 * s + 8 * h + 4 * e;
      float4 t4 = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < C) t4 = *reinterpret_cast<const float4*>(xi_row + c);
      v[4 * e] = t4.x; v[4 * e + 1] = t4.y; v[4 * e + 2] = t4.z; v[4 * e + 3] = t4.w;
    }
    unsigned hh[4], mm[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) split2_pair(v[2 * e], v[2 * e + 1], hh[e], mm[e]);
    const uint4 H4 = make_uint4(hh[0], hh[1], hh[2], hh[3]), M4 = make_uint4(mm[0], mm[1], mm[2], mm[3]);
    q1[s] = *reinterpret_cast<const bf16x8*>(&H4);
    q2[s] = *reinterpret_cast<const bf16x8*>(&M4);
  }
}

// ---- merge of a row's 4 lists through LDS, index write-out ----------------------------------------------------------------------------
// Lists 1, 2, 3 are written to md / mj ([KC][64 rows] distances, then indices, over the scan's LDS: the leading barrier ends the
// scan) one after the other and inserted into list 0 by (d, j) lexicographic order -- the scan's lists are strict in d alone, which
// is enough within one list (it meets its candidates by ascending j) and not across lists.  A source list is ascending: once an
// entry does not beat the destination's last, nothing later can, and the wave leaves the loop (wave-uniform).
//   lid       this lane's list id; list 0 is the destination and writes the row's k indices
//   rslot     the row's slot in md / mj
//   dst_wave  wave-uniform: this wave holds list 0 of its rows
//   active    lane-level: this lane holds list 0 (lanes of a destination wave that do not idle along with d = +inf, a no-op)
// knn_kernel: one list per wave (lid = w, rslot = lane, active everywhere); the matrix-pipe forms: lid and rslot of ScanLane, the
// destination is h == 0 of the waves with cs == 0.
// PACKED: the keys hold the cloud-local j and `base`, the cloud's first tower row, is added when the indices are written.
// Non-finite input: every trip count is KC or k and every store goes to the row's LDS slot or its k output slots (out = idx +
// grow k); rows with fewer than k candidates below +inf end with open slots, which fill_short_list (knn_common.h) fills.
template <int KC>
__device__ __forceinline__ void merge_lists(float* smem, float (&dl)[KC], int (&jl)[KC], int lid, int rslot, bool dst_wave,
                                            bool active) {
  __syncthreads();
  float* md = smem;
  int* mj = reinterpret_cast<int*>(smem + ROWS * KC);
#pragma unroll 1
  for (int src = 1; src < 4; ++src) {
    if (src > 1) __syncthreads();
    if (lid == src) {
#pragma unroll
      for (int t = 0; t < KC; ++t) {
        md[t * ROWS + rslot] = dl[t];
        mj[t * ROWS + rslot] = jl[t];
      }
    }
    __syncthreads();
    if (dst_wave) {
#pragma unroll 1
      for (int t = 0; t < KC; ++t) {
        const float d = active ? md[t * ROWS + rslot] : INFINITY;
        const int j = active ? mj[t * ROWS + rslot] : 0x7fffffff;
        const lmask_t need = key_less<true>(d, j, dl[KC - 1], jl[KC - 1]);
        if (need == 0) break;
        list_insert<KC, true>(dl, jl, d, j);
      }
    }
  }
}
template <int KC, bool PACKED>
__device__ __forceinline__ void merge_lists_write(float* smem, float (&dl)[KC], int (&jl)[KC], int lid, int rslot, bool dst_wave,
                                                  bool active, bool row_ok, int32_t* __restrict__ idx, int64_t grow, int k, int N,
                                                  int base) {
  merge_lists<KC>(smem, dl, jl, lid, rslot, dst_wave, active);
  if (lid == 0 && row_ok) {
    int32_t* out = idx + grow * k;
#pragma unroll
    for (int t = 0; t < KC; ++t)
      if (t < k) out[t] = PACKED ? base + jl[t] : jl[t];
    fill_short_list<KC>(jl, k, N, PACKED ? base : 0, out);
  }
}
// The same merge with the selected D~ written beside the indices (knn_cross_kernel): dist null, or k floats per row in the order of
// idx.  An open slot of a list holds d = +inf (list_init; an entry is listed only with d < thr <= +inf), so the slots that
// fill_short_list fills -- candidates at D~ = +inf, by its argument -- carry +inf without another pass.  N and base are the
// CANDIDATE cloud's size and first tower row, grow the query's global row.
template <int KC, bool PACKED>
__device__ __forceinline__ void merge_lists_write_dist(float* smem, float (&dl)[KC], int (&jl)[KC], int lid, int rslot, bool dst_wave,
                                                       bool active, bool row_ok, int32_t* __restrict__ idx, float* __restrict__ dist,
                                                       int64_t grow, int k, int N, int base) {
  merge_lists<KC>(smem, dl, jl, lid, rslot, dst_wave, active);
  if (lid == 0 && row_ok) {
    int32_t* out = idx + grow * k;
#pragma unroll
    for (int t = 0; t < KC; ++t)
      if (t < k) out[t] = PACKED ? base + jl[t] : jl[t];
    if (dist) {
      float* dout = dist + grow * k;
#pragma unroll
      for (int t = 0; t < KC; ++t)
        if (t < k) dout[t] = dl[t];
    }
    fill_short_list<KC>(jl, k, N, PACKED ? base : 0, out);
  }
}

}  // namespace

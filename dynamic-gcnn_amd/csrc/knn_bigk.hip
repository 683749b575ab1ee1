// knn_bigk.hip -- K1 for 64 < k <= 256: one exact all-pairs scan for every width 1 <= C <= 1024, dense clouds and packed towers.
//
// MUST be compiled with -ffp-contract=off (csrc/Makefile).  Distances are the normative ones of oracle/knn_oracle.c, produced by
// the code that knn_wide_kernel runs: s_i from sqnorm_kernel / sqnorm_wide_kernel, SlabStage and scan_dist of knn_scan.h -- for ANY
// C, so C <= 4 is one partly filled slab.  What differs from knn_wide_kernel is the selection.
//
// Selection.  The list-keeping kernels hold KC sorted (d, j) pairs per lane in registers (KC = 64 already takes 345 registers in
// knn_wide_kernel); past 64 the scan keeps no list at all.  Every query row owns a buffer of `cap` 64-bit keys (knn_key: unsigned
// order == (D~, j) order, D~ = +inf where D is NaN) and a bound key, ~0 at first.  A candidate whose key is below the row's bound
// is appended (LDS atomic on the row's count, one 8-byte store).  At every tile boundary a row whose count has passed the mark
// cap - 64 is compacted by one wave: a bitonic network over the whole buffer (cap / 64 keys per lane) sorts it, the k smallest
// keys are written back and the k-th becomes the bound.  After the last tile the same network sorts every row once more and the
// low 32 bits of its first k keys are the row's indices.
//   KP  = 128 (k <= 128) or 256;  cap = 2 KP <= 512 = 64 KA_MAXE of knn.hip: 4 or 8 keys per lane.
//   Invariant at the start of every tile: count <= cap - 64.  A tile has 64 candidates, so a row receives at most 64 appends in
//   it and every append position is < cap; a compaction leaves k <= KP <= cap - 64.
// Where the buffers live: in the caller's workspace (KnnWorkspace: cap keys per row behind the bounds; the counts stay in LDS), as
// the append form's do.  Keeping them in LDS would take 32 query rows x 256 keys x 8 bytes = 64 KB (128 KB for KP = 256) beside the
// 67.5 KB of slab tiles, i.e. a block of 32 query rows at one block per CU: half the rows per staged candidate tile and half the
// waves of the step loop below, which is the proven part.  A buffer is written and re-read by its own block only, ~k (1 + ln(N / k))
// keys per row in all, so the traffic stays in the XCD's L2: the stores are write-through and the compacting wave reads with
// agent-scope loads (past this CU's L1, which may hold the lines from the row's previous compaction), both sides of a barrier.
//
// Properties.
//  * Total order: the result is the k smallest of the row's N distinct keys.  A key is dropped only when k keys below it are known
//    (bound = the k-th smallest of a buffer), so the buffer always holds the k smallest seen so far whatever the order of the
//    appends and whenever a row compacts -- and WHEN it compacts depends only on its counts at tile boundaries, which are functions
//    of the keys.  Two calls are bit-identical.
//  * Non-finite input: no trip count and no store address depends on a value.  Loops run to N, C, cap, or the 64 rows of a block; a
//    distance only decides WHETHER a lane appends; stores go to the row's own buffer below cap (the invariant), the first k slots
//    of it, the block's LDS words, or the row's k output slots.
//  * Rows with fewer than k candidates below +inf: candidates at D~ = +inf are keys like any other ((+inf, j) < ~0) and are appended
//    until k keys are known, so the k smallest keys list them after the finite ones by ascending cloud-local j: the contract of
//    include/dgcnn_hip.h (K1) without a fill pass.  Every buffer ends with >= k keys (k <= N, and nothing is dropped before k keys
//    are there), so all k output slots are written from real keys.
//  * Packed towers: keys hold the cloud-local j; a block past its cloud's rows leaves before its first barrier; the cloud's first
//    tower row is added when the indices are written.
//  * Resources (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; dense and packed alike): 4 keys per lane: 120
//    VGPRs (float4 loader) / 118 (scalar loader); 8 keys per lane: 130 / 130; no AGPRs, no scratch in any instance (6 ... 28 SGPRs
//    spilled to VGPR lanes), so nothing in the tile loop touches scratch; LDS 68,864 bytes; 2 waves per SIMD = two blocks per CU,
//    which is what the LDS admits.  Times: profiles/knn_bigk.txt.
#include "knn_scan.h"

namespace {

// One step of the bitonic sorting network over n = 64 E keys, element i = 64 q + lane in key[q] of `lane`: compare-exchange of
// elements i and i ^ J within sorted runs of S2, ascending where (i & S2) == 0.  J >= 64: two registers of the same lane; J < 64:
// the same register of lanes l and l ^ J (bitonic_step, knn_common.h).  Then the steps J / 2 ... 1 of the same run size.
template <int E, int S2, int J>
__device__ __forceinline__ void sortnet_steps(unsigned long long (&key)[E], int lane) {
  if constexpr (J >= 64) {
    constexpr int dq = J / 64;
#pragma unroll
    for (int q = 0; q < E; ++q) {
      if ((q & dq) == 0) {
        const bool up = ((64 * q) & S2) == 0;                    // S2 >= 128: a function of q alone
        const unsigned long long a = key[q], b = key[q | dq];
        const bool sw = (b < a) == up;
        key[q] = sw ? b : a;
        key[q | dq] = sw ? a : b;
      }
    }
  } else {
#pragma unroll
    for (int q = 0; q < E; ++q) key[q] = bitonic_step<J>(key[q], lane, (((64 * q) | lane) & S2) == 0);
  }
  if constexpr (J > 1) sortnet_steps<E, S2, J / 2>(key, lane);
}
// the whole network: runs of 2, 4, ... 64 E.  Afterwards element i is the (i + 1)-th smallest key.
template <int E, int S2 = 2>
__device__ __forceinline__ void wave_sort_all(unsigned long long (&key)[E], int lane) {
  sortnet_steps<E, S2, S2 / 2>(key, lane);
  if constexpr (S2 < 64 * E) wave_sort_all<E, 2 * S2>(key, lane);
}

// Block and D layout: ScanLane; slab staging: SlabStage (knn_scan.h).  E = cap / 64.
template <int E, bool VEC, class Clouds>
__global__ __launch_bounds__(256, 2) void knn_bigk_kernel(const float* __restrict__ x, const float* __restrict__ sq, Clouds cl, int C,
                                                          int64_t ldx, int k, unsigned long long* ent, int32_t* __restrict__ idx) {
  using Stage = SlabStage<VEC>;
  constexpr int SL = Stage::SL, TJM = Stage::TJM, TILE_F = Stage::TILE_F;
  constexpr int CAP = 64 * E;
  constexpr int TRIG = CAP - TJM;            // a row whose count is above this at a tile boundary is compacted
  __shared__ __attribute__((aligned(16))) float smem[4 * TILE_F + 2 * TJM];
  __shared__ unsigned long long bnd[ROWS];   // the row's bound key: a candidate is appended iff its key is below it
  __shared__ int cnt_s[ROWS];                // keys in the row's buffer
  float* sjs = smem + 4 * TILE_F;            // [2][TJM], by tile parity

  // The mapping is ScanLane's, written out: `m` goes to slab_mfma only.  With lane and w taken from `m` the 64-bit compares of
  // wave_sort_all come out with the opposite polarity (v_cmp_lt_u64 for v_cmp_ge_u64, the selects swapped) and the 8-key instances
  // run 0.8 % slower at (8, 16384, 64, 256); with these lines the network is the one measured in profiles/knn_bigk.txt
  // (profiles/knn_scan_shared.txt).
  const ScanLane m;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int qg = w & 1;
  const int cs = w >> 1;
  const int b = blockIdx.y;
  const int N = cl.size(b);
  const int row0 = blockIdx.x * ROWS;
  if (Clouds::kPacked && row0 >= N) return;
  const int64_t cb = cl.base(b);
  const int row = row0 + qg * 32 + l31;
  const float* sqb = sq + cb;
  const int rowc = row < N ? row : N - 1;
  const float si = sqb[rowc];

  // (rows past N repeat row N - 1: never appended, never written)
  Stage stage(x + cb * ldx, sqb, ldx, N, C, row0, tid, smem, sjs);
  const int nt = (N + TJM - 1) / TJM;
  const int ns = (C + SL - 1) / SL;
  const int nu = nt * ns;                    // steps of the flattened (tile, slab) sequence
  stage.fetch(0, 0);
  stage.stash(0, 0, true);
  if (tid < ROWS) {
    bnd[tid] = ~0ull;
    cnt_s[tid] = 0;
  }
  const int rslot = qg * 32 + l31;           // row within the block
  const int cbase = cs * 32;
  unsigned long long* mybuf = ent + (cb + rowc) * (int64_t)CAP;
  __syncthreads();

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  int t = 0, s = 0;                          // tile and slab of step u
#pragma unroll 1
  for (int u = 0; u <= nu; ++u) {            // u == nu: the pass that writes the result (s == 0 again, t == nt)
    if (s == 0 && u > 0) {
      // ---- tile boundary: every append of the tiles before is behind a barrier.  Wave w looks after rows w, w + 4, ...: it sorts
      // the buffers that passed the mark and keeps their k smallest keys; in the last pass it sorts every row of the cloud and
      // writes the indices.  One copy of the network serves both. ----
      const bool last = (u == nu);
#pragma unroll 1
      for (int r = w; r < ROWS; r += 4) {
        const int S = __builtin_amdgcn_readfirstlane(cnt_s[r]);
        if (S > TRIG || (last && row0 + r < N)) {                // wave-uniform
          unsigned long long* buf = ent + (cb + row0 + r) * (int64_t)CAP;
          unsigned long long key[E];
#pragma unroll
          for (int q = 0; q < E; ++q) {
            const int e = lane + 64 * q;
            key[q] = (e < S) ? __hip_atomic_load(buf + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ~0ull;
          }
          wave_sort_all<E>(key, lane);
          if (last) {
            int32_t* out = idx + (cb + row0 + r) * k;
#pragma unroll
            for (int q = 0; q < E; ++q) {
              const int e = lane + 64 * q;
              if (e < k) out[e] = (Clouds::kPacked ? (int)cb : 0) + (int)(unsigned)key[q];
            }
          } else {
#pragma unroll
            for (int q = 0; q < E; ++q) {
              const int e = lane + 64 * q;
              if (e < k) buf[e] = key[q];
              if (e == k - 1) {
                bnd[r] = key[q];
                cnt_s[r] = k;
              }
            }
          }
        }
      }
      if (last) break;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // the kept keys are in L2 before any wave appends behind them
      __syncthreads();                       // bounds and counts are read by the drain of this tile (the same step when ns == 1)
    }
    const int buf = u & 1;
    const int j0 = t * TJM;
    const int sn = (s + 1 < ns) ? s + 1 : 0; // the next step's slab and tile
    const int tn = (s + 1 < ns) ? t : t + 1;
    if (u + 1 < nu) stage.fetch(tn * TJM, sn * SL);
    if (j0 + cbase < N) {                    // wave-uniform, the same for every slab of a tile
      stage.slab_mfma(acc, buf, m);
      if (s == ns - 1) {
        // ---- the chain is complete: the keys of this lane's 16 candidates against the row's bound ----
        const unsigned long long bk = bnd[rslot];
        const float* sj = sjs + (t & 1) * TJM + cbase + 4 * h;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 s4 = *reinterpret_cast<const float4*>(sj + 8 * q);          // candidates 8 q + 4 h + (0..3)
          const float sv[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int j = j0 + cbase + d_layout_index(4 * q + e, h);
            const float d = scan_dist(acc[4 * q + e], si, sv[e]);
            const unsigned long long key = knn_key((d != d) ? INFINITY : d, j);
            if (row < N && j < N && key < bk) {
              const int pos = atomicAdd(&cnt_s[rslot], 1);       // < CAP by the invariant
              mybuf[pos] = key;
            }
          }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        // the appended keys are in L2 before the step's barrier: the compacting wave reads them past the L1 (the barrier itself
        // waits for LDS traffic only)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    }
    if (u + 1 < nu) stage.stash(buf ^ 1, tn & 1, sn == 0);
    __syncthreads();
    s = sn;
    t = tn;
  }
}

template <int E, class Clouds>
void launch_bigk_e(dim3 grid, hipStream_t st, const float* x, const float* sq, Clouds cl, int C, int64_t ldx, int k, bool vec,
                   unsigned long long* ent, int32_t* idx) {
  if (vec) dg::launch((knn_bigk_kernel<E, true, Clouds>), grid, dim3(256), 0, st, x, sq, cl, C, ldx, k, ent, idx);
  else dg::launch((knn_bigk_kernel<E, false, Clouds>), grid, dim3(256), 0, st, x, sq, cl, C, ldx, k, ent, idx);
}

template <class Clouds>
void launch_bigk(dim3 grid, hipStream_t st, const float* x, const float* sq, Clouds cl, int C, int64_t ldx, int k, bool vec,
                 unsigned long long* ent, int32_t* idx) {
  if (k <= 128) launch_bigk_e<4>(grid, st, x, sq, cl, C, ldx, k, vec, ent, idx);
  else launch_bigk_e<8>(grid, st, x, sq, cl, C, ldx, k, vec, ent, idx);
}

}  // namespace

namespace dg {

// entries per row buffer of the large-k scan: 2 KP, KP = 128 for k <= 128, else 256
int knn_bigk_cap(int k) { return k <= 128 ? 256 : 512; }

// The all-pairs search of ny clouds for k <= 256, s_i in sq, `ent` = knn_bigk_cap(k) 8-byte keys for every row.  seg_off null: dense
// clouds of max_n rows each; else the nseg + 1 offsets of a packed tower (ny = nseg).  vec_ok: rows are float4-loadable (the float4
// loader also needs C % 4 == 0).  1 <= C <= 1024.
void launch_knn_bigk(const float* x, const float* sq, const int32_t* seg_off, int ny, int max_n, int C, int64_t ldx, int k, int vec_ok,
                     int32_t* idx, unsigned long long* ent, hipStream_t st) {
  const dim3 grid((unsigned)dg::cdiv(max_n, ROWS), (unsigned)ny);
  const bool vec = vec_ok && C % 4 == 0;
  if (seg_off) launch_bigk(grid, st, x, sq, PackedClouds{seg_off, ny}, C, ldx, k, vec, ent, idx);
  else launch_bigk(grid, st, x, sq, DenseClouds(max_n), C, ldx, k, vec, ent, idx);
}

}  // namespace dg

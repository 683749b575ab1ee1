// knn_wide.hip -- K1 for wide feature rows (C up to 1024): the fp32 matrix-pipe scan of knn.hip:knn_mfma_kernel with the channel
// dimension walked in slabs of 64, and the s_i kernel for rows too wide for one LDS stage.
//
// MUST be compiled with -ffp-contract=off (csrc/Makefile); the arithmetic, and why the accumulators carried from slab to slab are
// the oracle's chain: knn_scan.h.
//
// Where the operands come from.  knn_mfma_kernel keeps the query rows resident (CP / 2 VGPRs) and the whole candidate tile [CP][66]
// in LDS twice; neither scales past C = 128.  Here both operands are staged slab by slab (knn_scan.h:SlabStage); the selection is
// knn_mfma_kernel's: per-lane sorted lists behind the shared bound, park_and_flag / drain_parked, merge_lists_write.
// LDS: 4 slab tiles + 8 parked distances per thread + s_j + the shared bound = 77,312 bytes: two blocks per CU.  (Parking all 16
// distances of a lane, as knn_mfma_kernel does, is 85.5 KB: one block per CU; the drain therefore runs in two halves of 8.)
#include "knn_scan.h"

namespace {

// s_i for C > 128 (knn.hip:sqnorm_kernel stages [64][C + 1] floats, which passes 64 KB at C = 255): the same sequential
// s = s + fl(v v) over c ascending, the block's 64 rows staged through LDS in chunks of 64 channels (coalesced loads), the running s
// kept by the row's thread.
__global__ __launch_bounds__(256) void sqnorm_wide_kernel(const float* __restrict__ x, int64_t ldx, int64_t rows, int C,
                                                          float* __restrict__ sq) {
  constexpr int CH = 64, S = CH + 1;
  __shared__ float tile[ROWS * S];
  const int64_t r0 = (int64_t)blockIdx.x * ROWS;
  const int t = threadIdx.x;
  float s = 0.0f;
#pragma unroll 1
  for (int c0 = 0; c0 < C; c0 += CH) {
    const int cw = (C - c0 < CH) ? C - c0 : CH;
    __syncthreads();
    for (int e = t; e < ROWS * CH; e += 256) {
      const int rr = e >> 6, cc = e & 63;
      if (cc < cw) tile[rr * S + cc] = (r0 + rr < rows) ? x[(r0 + rr) * ldx + c0 + cc] : 0.0f;
    }
    __syncthreads();
    if (t < ROWS) {
      for (int c = 0; c < cw; ++c) {
        const float v = tile[t * S + c];
        const float q = v * v;
        s = s + q;
      }
    }
  }
  if (t < ROWS && r0 + t < rows) sq[r0 + t] = s;
}

// Block and lists: ScanLane (knn_scan.h).  Clouds as in knn_kernel: keys keep the cloud-local j, a packed block past its cloud leaves
// before the first barrier, the cloud's first tower row is added when the indices are written.
// Non-finite input: every trip count below is a function of N, C and k; what a distance can and cannot do is said at park_and_flag,
// drain_parked and merge_lists_write.
// Two waves per SIMD (what the LDS admits) for KC <= 40; the KC = 64 lists (128 VGPRs) beside the 32 staging registers do not fit 256
// registers without scratch, so that instance takes one wave per SIMD (345 registers).
template <int KC, bool VEC, class Clouds>
__global__ __launch_bounds__(256, (KC <= 40 ? 2 : 1)) void knn_wide_kernel(const float* __restrict__ x, const float* __restrict__ sq,
                                                                           Clouds cl, int C, int64_t ldx, int k,
                                                                           int32_t* __restrict__ idx) {
  using Stage = SlabStage<VEC>;
  constexpr int SL = Stage::SL, TJM = Stage::TJM, TILE_F = Stage::TILE_F;
  constexpr int DQ_F = 8 * 256;
  constexpr int MERGE_F = ROWS * KC * 2;
  constexpr int WORK_F = 4 * TILE_F + DQ_F + 2 * TJM + 4 * ROWS;
  constexpr int SH = (WORK_F > MERGE_F ? WORK_F : MERGE_F);
  __shared__ __attribute__((aligned(16))) float smem[SH];
  float* dq = smem + 4 * TILE_F;
  float* sjs = dq + DQ_F;                    // [2][TJM], by tile parity
  volatile float* thrw = sjs + 2 * TJM;      // [4 lists][64 rows]: list[KC/4 - 1] so far

  const ScanLane m;
  const int tid = m.tid, h = m.h, cbase = m.cbase, lid = m.lid, rslot = m.rslot;
  const int b = blockIdx.y;
  const int N = cl.size(b);
  const int row0 = blockIdx.x * ROWS;
  if (Clouds::kPacked && row0 >= N) return;
  const int64_t cb = cl.base(b);
  const int row = row0 + rslot;
  const float* sqb = sq + cb;
  const int rowc = row < N ? row : N - 1;
  const float si = sqb[rowc];

  float dl[KC];
  int jl[KC];
  list_init<KC>(dl, jl);

  Stage stage(x + cb * ldx, sqb, ldx, N, C, row0, tid, smem, sjs);
  const int nt = (N + TJM - 1) / TJM;
  const int ns = (C + SL - 1) / SL;
  const int nu = nt * ns;                    // steps of the flattened (tile, slab) sequence
  stage.fetch(0, 0);
  stage.stash(0, 0, true);
  thrw[tid] = INFINITY;
  __syncthreads();

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  int t = 0, s = 0;                          // tile and slab of step u
#pragma unroll 1
  for (int u = 0; u < nu; ++u) {
    const int buf = u & 1;
    const int j0 = t * TJM;
    const int sn = (s + 1 < ns) ? s + 1 : 0; // the next step's slab and tile
    const int tn = (s + 1 < ns) ? t : t + 1;
    if (s == 0) thrw[lid * ROWS + rslot] = dl[KC / 4 - 1];    // publish this list's KC/4-th entry (as of the previous tile)
    if (u + 1 < nu) stage.fetch(tn * TJM, sn * SL);
    if (j0 + cbase < N) {                    // wave-uniform, the same for every slab of a tile
      stage.slab_mfma(acc, buf, m);
      if (s == ns - 1) {
        // ---- the chain is complete: this lane's 16 candidates in two halves of 8 ----
        const float o1 = thrw[(lid ^ 1) * ROWS + rslot], o2 = thrw[(lid ^ 2) * ROWS + rslot], o3 = thrw[(lid ^ 3) * ROWS + rslot];
        const float* sj = sjs + (t & 1) * TJM + cbase + 4 * h;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const float thr = fminf(dl[KC - 1], shared_bound<KC>(dl, o1, o2, o3));
          const unsigned mask = park_and_flag<8>(acc, 8 * half, si, sj, thr, dq, tid);
          drain_parked<KC, 8>(dl, jl, mask, dq, tid, 8 * half, h, j0 + cbase);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      }
    }
    if (u + 1 < nu) stage.stash(buf ^ 1, tn & 1, sn == 0);
    __syncthreads();
    s = sn;
    t = tn;
  }

  merge_lists_write<KC, Clouds::kPacked>(smem, dl, jl, lid, rslot, m.cs == 0, h == 0, row < N, idx, cb + row, k, N, (int)cb);
}

template <int KC, class Clouds>
void launch_wide_k(dim3 grid, hipStream_t st, const float* x, const float* sq, Clouds cl, int C, int64_t ldx, int k, bool vec,
                   int32_t* idx) {
  if (vec) dg::launch((knn_wide_kernel<KC, true, Clouds>), grid, dim3(256), 0, st, x, sq, cl, C, ldx, k, idx);
  else dg::launch((knn_wide_kernel<KC, false, Clouds>), grid, dim3(256), 0, st, x, sq, cl, C, ldx, k, idx);
}

template <class Clouds>
void launch_wide(dim3 grid, hipStream_t st, const float* x, const float* sq, Clouds cl, int C, int64_t ldx, int k, bool vec,
                 int32_t* idx) {
  if (k <= 8) launch_wide_k<8>(grid, st, x, sq, cl, C, ldx, k, vec, idx);
  else if (k <= 20) launch_wide_k<20>(grid, st, x, sq, cl, C, ldx, k, vec, idx);
  else if (k <= 40) launch_wide_k<40>(grid, st, x, sq, cl, C, ldx, k, vec, idx);
  else launch_wide_k<64>(grid, st, x, sq, cl, C, ldx, k, vec, idx);
}

}  // namespace

namespace dg {

void launch_sqnorm_wide(const float* x, int64_t ldx, int64_t rows, int C, float* sq, hipStream_t st) {
  dg::launch(sqnorm_wide_kernel, dim3((unsigned)dg::cdiv(rows, ROWS)), dim3(256), 0, st, x, ldx, rows, C, sq);
}

// The all-pairs search of ny clouds, s_i in sq.  seg_off null: dense clouds of max_n rows each; else the nseg + 1 offsets of a packed
// tower (ny = nseg).  vec_ok: rows are float4-loadable (the float4 loader also needs C % 4 == 0).  5 <= C <= 1024, k <= 64.
void launch_knn_wide(const float* x, const float* sq, const int32_t* seg_off, int ny, int max_n, int C, int64_t ldx, int k, int vec_ok,
                     int32_t* idx, hipStream_t st) {
  const dim3 grid((unsigned)dg::cdiv(max_n, ROWS), (unsigned)ny);
  const bool vec = vec_ok && C % 4 == 0;
  if (seg_off) launch_wide(grid, st, x, sq, PackedClouds{seg_off, ny}, C, ldx, k, vec, idx);
  else launch_wide(grid, st, x, sq, DenseClouds(max_n), C, ldx, k, vec, idx);
}

}  // namespace dg

// knn_cross.hip -- k-NN between TWO point sets: for every row of a query set the k nearest rows of a separate candidate set
// (include/dgcnn_hip.h: dgcnn_knn_cross_f32).  The kernel is knn_wide.hip:knn_wide_kernel with a second operand source: query rows
// from (q, ldq, s_q) under the query-cloud map, candidates from (p, ldp, s_p) under the candidate-cloud map, and the slab width a
// template parameter, so that rows of at most 16 channels (raw coordinates) stage 16-channel slabs instead of 64-channel ones.
//
// MUST be compiled with -ffp-contract=off (csrc/Makefile); the arithmetic, and why the accumulators carried from slab to slab are
// the oracle's chain: knn_scan.h.  s of a row is sqnorm_kernel's / sqnorm_wide_kernel's, one launch per operand.
//
// LDS (floats): 4 slab tiles [SL][66] + 8 parked distances per thread + s_j by tile parity + the shared bound, or the merge's
// 2 x 64 x KC if that is more.  SL = 64: knn_wide_kernel's 77,312 bytes, two blocks per CU.  SL = 16: 26,624 bytes (32,768 at KC = 64,
// the merge); the register budget, not the LDS, then holds a CU at two blocks.
#include "knn_scan.h"

namespace {

// Block and lists: ScanLane (knn_scan.h).  Block (x, b) searches query rows [64 x, 64 x + 64) of query cloud b against ALL rows of
// candidate cloud b.  Keys keep the candidate-cloud-local j; the candidate cloud's first tower row is added when the indices are
// written (packed), and the output row is the query's global row cl_q.base(b) + row.
//   M = cl_q.size(b): the clamp of the query rows, the early exit of a packed block (row0 >= M, before the first barrier) and the
//                     guard of the write-out (row < M);
//   N = cl_p.size(b): the clamp of the candidate rows, s_j = +inf from N on, the tile loop, the wave-level skip of a candidate half
//                     past the cloud (j0 + cbase < N) and the bound of fill_short_list.
// Value independence (non-finite input).  No trip count and no address below is a function of a loaded coordinate, norm or distance:
// the step loop runs cdiv(N, 64) * cdiv(C, SL) times; every global load is from a row clamped to [0, M) or [0, N) and a channel quad
// clamped to [0, C) (load_row_quad); a distance only sets bits of an 8-bit mask (d < thr is false for NaN and +inf: park_and_flag),
// the drain pops one bit per trip and indexes the parked distances by the bit's number (drain_parked), the merge walks KC entries
// (merge_lists); the stores go to idx / dist + (cl_q.base(b) + row) k + t with row < M and t < k, and fill_short_list runs v < N,
// c < k.  What is written to idx is a list entry j < N or the fill's v < N, plus cl_p.base(b).
// Two waves per SIMD for KC <= 40, one for KC = 64, as knn_wide_kernel (the lists are the registers).
template <int KC, bool VEC, int SL, class Clouds>
__global__ __launch_bounds__(256, (KC <= 40 ? 2 : 1)) void knn_cross_kernel(const float* __restrict__ q, const float* __restrict__ p,
                                                                            const float* __restrict__ sq_q,
                                                                            const float* __restrict__ sq_p, Clouds cl_q, Clouds cl_p,
                                                                            int C, int64_t ldq, int64_t ldp, int k,
                                                                            int32_t* __restrict__ idx, float* __restrict__ dist) {
  using Stage = CrossSlabStage<VEC, SL>;
  constexpr int TJM = Stage::TJM, TILE_F = Stage::TILE_F;
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
  const int M = cl_q.size(b);
  const int N = cl_p.size(b);
  const int row0 = blockIdx.x * ROWS;
  if (Clouds::kPacked && row0 >= M) return;
  const int64_t qbase = cl_q.base(b), pbase = cl_p.base(b);
  const int row = row0 + rslot;
  const int rowc = row < M ? row : M - 1;
  const float si = sq_q[qbase + rowc];

  float dl[KC];
  int jl[KC];
  list_init<KC>(dl, jl);

  Stage stage(q + qbase * ldq, ldq, M, p + pbase * ldp, sq_p + pbase, ldp, N, C, row0, tid, smem, sjs);
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

  merge_lists_write_dist<KC, Clouds::kPacked>(smem, dl, jl, lid, rslot, m.cs == 0, h == 0, row < M, idx, dist, qbase + row, k, N,
                                              (int)pbase);
}

struct CrossCall {
  const float *q, *p, *sq_q, *sq_p;
  int C;
  int64_t ldq, ldp;
  int k;
  int32_t* idx;
  float* dist;
  dim3 grid;
  hipStream_t st;
};

template <int KC, bool VEC, int SL, class Clouds>
void launch_cross_one(const CrossCall& a, Clouds cq, Clouds cp) {
  dg::launch((knn_cross_kernel<KC, VEC, SL, Clouds>), a.grid, dim3(256), 0, a.st, a.q, a.p, a.sq_q, a.sq_p, cq, cp, a.C, a.ldq, a.ldp,
             a.k, a.idx, a.dist);
}
template <int KC, class Clouds>
void launch_cross_k(const CrossCall& a, Clouds cq, Clouds cp, bool vec, bool narrow) {
  if (narrow) {
    if (vec) launch_cross_one<KC, true, 16>(a, cq, cp); else launch_cross_one<KC, false, 16>(a, cq, cp);
  } else {
    if (vec) launch_cross_one<KC, true, 64>(a, cq, cp); else launch_cross_one<KC, false, 64>(a, cq, cp);
  }
}
template <class Clouds>
void launch_cross(const CrossCall& a, Clouds cq, Clouds cp, bool vec, bool narrow) {
  if (a.k <= 8) launch_cross_k<8>(a, cq, cp, vec, narrow);
  else if (a.k <= 20) launch_cross_k<20>(a, cq, cp, vec, narrow);
  else if (a.k <= 40) launch_cross_k<40>(a, cq, cp, vec, narrow);
  else launch_cross_k<64>(a, cq, cp, vec, narrow);
}

constexpr int CROSS_MAX_K = 64, CROSS_MAX_C = 1024, CROSS_NARROW_C = 16;
size_t cross_pad(size_t n) { return (n + 255) & ~(size_t)255; }       // knn.hip:KnnWorkspace::pad
bool cross_vec_ok(const float* x, int64_t ld) { return (ld % 4 == 0) && ((reinterpret_cast<uintptr_t>(x) & 15) == 0); }

// Slab width of a call: 16 channels for rows of at most 16, else 64.  There is no switch: profiles/knn_cross_bench.py measures the
// 64-channel slab on raw coordinates by padding the same points with zero channels to C = 20, which changes no distance.
bool cross_narrow(int C) { return C <= CROSS_NARROW_C; }

}  // namespace

namespace dg {
void launch_sqnorm_rows(const float* x, int64_t ldx, int64_t rows, int C, float* sq, hipStream_t st);     // knn.hip
}

extern "C" int64_t dgcnn_knn_cross_workspace_bytes(int q_rows, int p_rows) {
  return (q_rows <= 0 || p_rows <= 0) ? 0 : (int64_t)(cross_pad((size_t)q_rows * sizeof(float)) + cross_pad((size_t)p_rows * sizeof(float)));
}

extern "C" int dgcnn_knn_cross_f32(const float* q, int64_t ldq, const float* p, int64_t ldp, int C, int k, int nseg, const int32_t* q_off,
                                   const int32_t* p_off, int q_rows, int p_rows, int max_m, int min_n, int max_n, int32_t* idx,
                                   float* dist, void* ws, size_t ws_bytes, void* stream) {
  const char* what = "dgcnn_knn_cross_f32";
  DG_REQUIRE(q && p && idx && ws, DGCNN_EINVAL, "%s: null pointer", what);
  DG_REQUIRE((q_off == nullptr) == (p_off == nullptr), DGCNN_EINVAL,
             "%s: q_off and p_off must both be null (dense clouds) or both be given (packed towers)", what);
  DG_REQUIRE(nseg > 0 && nseg <= 65535 && q_rows > 0 && p_rows > 0 && C > 0 && ldq >= C && ldp >= C, DGCNN_EINVAL,
             "%s: bad shape nseg=%d q_rows=%d p_rows=%d C=%d", what, nseg, q_rows, p_rows, C);
  DG_REQUIRE(k >= 1, DGCNN_EINVAL, "%s: k=%d must be in [1, smallest candidate cloud=%d]", what, k, min_n);
  DG_REQUIRE(k <= CROSS_MAX_K, DGCNN_EUNSUP, "%s: k=%d > %d unsupported (the large-k scan searches a cloud against itself only)", what,
             k, CROSS_MAX_K);
  DG_REQUIRE(C <= CROSS_MAX_C, DGCNN_EUNSUP, "%s: C=%d > %d unsupported", what, C, CROSS_MAX_C);
  if (q_off) {
    DG_REQUIRE(max_m > 0 && max_m <= q_rows && nseg <= q_rows && (int64_t)max_m * nseg >= q_rows, DGCNN_EINVAL,
               "%s: query cloud sizes max_m=%d do not fit %d rows in %d clouds", what, max_m, q_rows, nseg);
    DG_REQUIRE(min_n > 0 && min_n <= max_n && max_n <= p_rows && (int64_t)min_n * nseg <= p_rows && (int64_t)max_n * nseg >= p_rows,
               DGCNN_EINVAL, "%s: candidate cloud sizes min_n=%d max_n=%d do not fit %d rows in %d clouds", what, min_n, max_n, p_rows,
               nseg);
  } else {
    DG_REQUIRE(max_m > 0 && (int64_t)max_m * nseg == q_rows, DGCNN_EINVAL, "%s: dense queries: q_rows=%d is not nseg=%d x max_m=%d",
               what, q_rows, nseg, max_m);
    DG_REQUIRE(max_n > 0 && min_n == max_n && (int64_t)max_n * nseg == p_rows, DGCNN_EINVAL,
               "%s: dense candidates: p_rows=%d is not nseg=%d x max_n=%d (min_n=%d must equal max_n)", what, p_rows, nseg, max_n, min_n);
  }
  DG_REQUIRE(k <= min_n, DGCNN_EINVAL, "%s: k=%d must be in [1, smallest candidate cloud=%d]", what, k, min_n);
  const size_t sq_bytes = cross_pad((size_t)q_rows * sizeof(float));
  DG_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0 && ws_bytes >= sq_bytes + cross_pad((size_t)p_rows * sizeof(float)), DGCNN_EINVAL,
             "%s: workspace must be 16-byte aligned and hold dgcnn_knn_cross_workspace_bytes(q_rows, p_rows) bytes (got %zu)", what,
             ws_bytes);

  hipStream_t st = (hipStream_t)stream;
  float* s_q = reinterpret_cast<float*>(ws);
  float* s_p = reinterpret_cast<float*>(static_cast<char*>(ws) + sq_bytes);
  // one set of rows under one map on both sides: its norms serve both operands
  const bool same = q == p && ldq == ldp && q_rows == p_rows && (q_off ? q_off == p_off : max_m == max_n);
  dg::launch_sqnorm_rows(q, ldq, q_rows, C, s_q, st);
  if (same) s_p = s_q;
  else dg::launch_sqnorm_rows(p, ldp, p_rows, C, s_p, st);

  const bool vec = C % 4 == 0 && cross_vec_ok(q, ldq) && cross_vec_ok(p, ldp);
  const CrossCall a{q, p, s_q, s_p, C, ldq, ldp, k, idx, dist, dim3((unsigned)dg::cdiv(max_m, ROWS), (unsigned)nseg), st};
  if (q_off) launch_cross(a, PackedClouds{q_off, nseg}, PackedClouds{p_off, nseg}, vec, cross_narrow(C));
  else launch_cross(a, DenseClouds(max_m), DenseClouds(max_n), vec, cross_narrow(C));
  return dg::check_launch(what);
}

// interp.hip -- K6: feature interpolation between two point sets (PointNet++ feature propagation): every query row receives the
// inverse-distance-weighted mean of the feature rows of its k nearest candidates, from the (idx, dist) pair the two-set k-NN
// (knn_cross.hip) returns.  Forward: one gather kernel, no (q_rows, k, F) tensor.  Backward (features only; coordinates and weights
// carry no gradient): the transposed adjacency of the bipartite graph -- who interpolates from me? -- by integer counting sort with
// every bucket in ascending edge order, then one weighted gather-sum per candidate row.  No float atomics anywhere: the result has
// one value, run to run.  The arithmetic is normative (include/dgcnn_hip.h, K6): every product, sum and quotient is one fp32
// operation in a fixed order (the build uses -ffp-contract=off and `/` is the correctly rounded division).
#include "common.h"
#include <math.h>

namespace {

constexpr int IT = 256;          // threads of every block here
constexpr int FWD_E = 2048;      // (row, neighbour) entries a forward block keeps in LDS: rows per block <= FWD_E / k
constexpr int BWD_U = 8;         // dy rows the backward gather keeps in flight per thread

// candidate row of entry e = i * k + m: dense towers (M > 0) add the cloud's first row to the cloud-local index
__device__ __forceinline__ int32_t cand_row(const int32_t* __restrict__ idx, unsigned e, unsigned k, unsigned M, unsigned N) {
  const int32_t j = idx[e];
  return M ? (int32_t)((e / k) / M * N) + j : j;
}

// Forward.  A block owns RB = min(256 / (F/4), FWD_E / k) consecutive query rows.  Their RB * k weights are worked out once, by
// the block's first threads through LDS (one thread per entry for the two divisions, one thread per row for the ascending sum W),
// not once per channel lane; then thread (row, channel quad) gathers its k feature quads, four rows in flight, and adds them in
// the normative order m = 0 ... k-1.
__global__ __launch_bounds__(IT) void interp_fwd_kernel(const float* __restrict__ feat, int64_t ldf, const int32_t* __restrict__ idx,
                                                        const float* __restrict__ dist, int q_rows, int M, int N, int k, int FV, int RB,
                                                        float eps, float* __restrict__ a_out, float* __restrict__ y, int64_t ldy) {
  __shared__ float s_a[FWD_E];
  __shared__ int32_t s_j[FWD_E];
  __shared__ float s_W[IT];
  const int t = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * RB;
  const int rows = (q_rows - r0 < RB) ? (int)(q_rows - r0) : RB;
  const int ne = rows * k;
  const unsigned e0 = (unsigned)(r0 * k);                       // q_rows * k < 2^31
  for (int e = t; e < ne; e += IT) {
    const float D = dist[e0 + e];
    s_a[e] = (D < INFINITY) ? 1.0f / fmaxf(D, eps) : 0.0f;      // NaN and +inf: no weight; D <= eps (negative, -inf): 1 / eps
    s_j[e] = cand_row(idx, e0 + e, (unsigned)k, (unsigned)M, (unsigned)N);
  }
  __syncthreads();
  if (t < rows) {
    float W = s_a[t * k];
    for (int m = 1; m < k; ++m) W = W + s_a[t * k + m];
    s_W[t] = W;
  }
  __syncthreads();
  for (int e = t; e < ne; e += IT) {
    const float W = s_W[e / k];
    const float a = (W > 0.f) ? s_a[e] / W : 0.0f;
    s_a[e] = a;
    if (a_out) a_out[e0 + e] = a;
  }
  __syncthreads();
  const int r = t / FV;
  if (r >= rows) return;
  const int f = (t - r * FV) * 4;
  const float* sa = s_a + r * k;
  const int32_t* sj = s_j + r * k;
  const float* fp = feat + f;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int m0 = 0; m0 < k; m0 += 4) {
    float4 v[4];
    float w[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (m0 + u < k) {
        v[u] = ld4(fp + (int64_t)sj[m0 + u] * ldf);
        w[u] = sa[m0 + u];
      }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (m0 + u < k) {
        const float px = w[u] * v[u].x, py = w[u] * v[u].y, pz = w[u] * v[u].z, pw = w[u] * v[u].w;
        if (m0 + u == 0) acc = make_float4(px, py, pz, pw);     // y = a_0 x_0, not 0 + a_0 x_0 (the sign of a zero)
        else { acc.x = acc.x + px; acc.y = acc.y + py; acc.z = acc.z + pz; acc.w = acc.w + pw; }
      }
  }
  *reinterpret_cast<float4*>(y + (r0 + r) * ldy + f) = acc;
}

// ---- transposed adjacency of the bipartite graph: bucket j = the edges e = i * k + m whose candidate row is j.  The technique of
// dgcnn_edge_csr_build / dgcnn_edge_csr_sort (misc.hip, det.hip) without their assumption that sources and targets are the same
// rows: integer histogram whose atomic hands every edge a slot of its bucket (any order), exclusive scan over all p_rows buckets,
// fill, then every edge is placed at the number of smaller edge ids in its bucket.
__global__ void interp_count_kernel(const int32_t* __restrict__ idx, unsigned total, unsigned k, unsigned M, unsigned N,
                                    int32_t* __restrict__ cnt, int32_t* __restrict__ slot) {
  GRID_STRIDE(e, total) slot[e] = atomicAdd(cnt + cand_row(idx, (unsigned)e, k, M, N), 1);
}

// one block, 4096 counts a round: an int4 per thread, the wave's inclusive scan by shuffles, the 16 wave sums through LDS, the
// running total carried from round to round.  cnt is 16-byte aligned (a 256-byte aligned part of the workspace).
__global__ __launch_bounds__(1024) void interp_scan_kernel(const int32_t* __restrict__ cnt, int p_rows, int32_t* __restrict__ off) {
  __shared__ int wsum[16];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  int carry = 0;
  for (int64_t base = 0; base < p_rows; base += 4096) {
    const int64_t i0 = base + 4 * t;
    int4 c = make_int4(0, 0, 0, 0);
    if (i0 + 3 < p_rows) c = *reinterpret_cast<const int4*>(cnt + i0);
    else {
      if (i0 < p_rows) c.x = cnt[i0];
      if (i0 + 1 < p_rows) c.y = cnt[i0 + 1];
      if (i0 + 2 < p_rows) c.z = cnt[i0 + 2];
    }
    const int s = c.x + c.y + c.z + c.w;
    int inc = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_up(inc, d, 64);
      if (lane >= d) inc += v;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    int below = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
      const int v = wsum[w];
      if (w < wv) below += v;
      tot += v;
    }
    int run = carry + below + inc - s;
    if (i0 < p_rows) off[i0] = run;
    run += c.x;
    if (i0 + 1 < p_rows) off[i0 + 1] = run;
    run += c.y;
    if (i0 + 2 < p_rows) off[i0 + 2] = run;
    run += c.z;
    if (i0 + 3 < p_rows) off[i0 + 3] = run;
    carry += tot;
    __syncthreads();                                            // wsum is rewritten by the next round
  }
  if (t == 0) off[p_rows] = carry;
}

__global__ void interp_fill_kernel(const int32_t* __restrict__ idx, unsigned total, unsigned k, unsigned M, unsigned N,
                                   const int32_t* __restrict__ off, const int32_t* __restrict__ slot, int32_t* __restrict__ rev) {
  GRID_STRIDE(e, total) rev[off[cand_row(idx, (unsigned)e, k, M, N)] + slot[e]] = (int32_t)e;
}

// Out of place, one thread per stored edge: its place is the number of smaller edge ids in its bucket.  deg reads per edge, that
// is sum over buckets of deg^2 in all: q_rows k * (M k / N) on average (24 reads per edge for 65536 -> 8192 at k = 3), quadratic
// in the largest bucket in the worst case.  The threads of a wave walk the same bucket words, so the reads are broadcasts.
__global__ __launch_bounds__(IT) void interp_rank_kernel(const int32_t* __restrict__ idx, unsigned total, unsigned k, unsigned M,
                                                         unsigned N, const int32_t* __restrict__ off, const int32_t* __restrict__ rev,
                                                         int32_t* __restrict__ out) {
  GRID_STRIDE(p, total) {
    const int32_t e = rev[p];
    const int32_t j = cand_row(idx, (unsigned)e, k, M, N);
    const int b = off[j], n = off[j + 1] - b;
    int rank = 0;
    for (int q = 0; q < n; ++q) rank += (rev[b + q] < e) ? 1 : 0;
    out[b + rank] = e;
  }
}

// dfeat[j][:] (+)= sum over the bucket of j, ascending edge id, of a[e] * dy[e / k][:] -- sequential adds from 0.f, BWD_U dy rows
// in flight (a bucket holds M k / N edges on average, and every row is two dependent loads away: edge id, then a and dy).  One
// float4 channel quad per lane.  A candidate nobody interpolates from gets 0 (beta = 0) or keeps its row.
__global__ __launch_bounds__(IT) void interp_bwd_gather_kernel(const float* __restrict__ dy, int64_t lddy, const float* __restrict__ a,
                                                               const int32_t* __restrict__ off, const int32_t* __restrict__ srt,
                                                               int64_t p_rows, unsigned k, int FV, float* __restrict__ dfeat,
                                                               int64_t lddf, int beta) {
  GRID_STRIDE(it, p_rows * FV) {
    const int64_t j = it / FV;
    const int f = (int)(it - j * FV) * 4;
    const int p0 = off[j], p1 = off[j + 1];
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int p = p0; p < p1; p += BWD_U) {
      float4 v[BWD_U];
      float w[BWD_U];
#pragma unroll
      for (int u = 0; u < BWD_U; ++u)
        if (p + u < p1) {
          const unsigned e = (unsigned)srt[p + u];
          w[u] = a[e];
          v[u] = ld4(dy + (int64_t)(e / k) * lddy + f);
        }
#pragma unroll
      for (int u = 0; u < BWD_U; ++u)
        if (p + u < p1) {
          g.x = g.x + w[u] * v[u].x;
          g.y = g.y + w[u] * v[u].y;
          g.z = g.z + w[u] * v[u].z;
          g.w = g.w + w[u] * v[u].w;
        }
    }
    float* o = dfeat + j * lddf + f;
    if (beta) {
      const float4 d = ld4(o);
      g.x = d.x + g.x; g.y = d.y + g.y; g.z = d.z + g.z; g.w = d.w + g.w;
    }
    *reinterpret_cast<float4*>(o) = g;
  }
}

inline int64_t pad256(int64_t n) { return (n + 255) / 256 * 256; }
inline bool a16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// what both entries ask of the graph's shape; 0 when it is fine, else the message is set
int check_graph(const char* who, int q_rows, int p_rows, int M, int N, int k, int F) {
  DG_REQUIRE(k <= 64, DGCNN_EUNSUP, "%s: k=%d > 64 (the limit of the search between two sets)", who, k);
  DG_REQUIRE(k >= 1, DGCNN_EINVAL, "%s: k=%d must be at least 1", who, k);
  DG_REQUIRE(F > 0, DGCNN_EINVAL, "%s: F=%d must be positive", who, F);
  DG_REQUIRE(F % 4 == 0 && F <= 1024, DGCNN_EUNSUP, "%s: F must be a multiple of 4, <= 1024 (got F=%d)", who, F);
  DG_REQUIRE(q_rows > 0 && p_rows > 0, DGCNN_EINVAL, "%s: q_rows=%d and p_rows=%d must be positive", who, q_rows, p_rows);
  DG_REQUIRE((int64_t)q_rows * k < (1ll << 31), DGCNN_EUNSUP, "%s: q_rows * k >= 2^31", who);
  DG_REQUIRE(M >= 0 && N >= 0, DGCNN_EINVAL, "%s: M=%d and N=%d must not be negative", who, M, N);
  if (M > 0) {
    DG_REQUIRE(N > 0 && q_rows % M == 0 && (int64_t)p_rows == (int64_t)(q_rows / M) * N, DGCNN_EINVAL,
               "%s: dense towers need q_rows = B * M and p_rows = B * N (q_rows=%d, p_rows=%d, M=%d, N=%d)", who, q_rows, p_rows, M, N);
  } else {
    DG_REQUIRE(N == 0, DGCNN_EINVAL, "%s: M = 0 (idx holds candidate tower rows) needs N = 0, got N=%d", who, N);
  }
  return DGCNN_OK;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int dgcnn_interp_f32(const float* feat, int64_t ldf, const int32_t* idx, const float* dist, int q_rows, int p_rows, int M,
                                int N, int k, int F, float eps, float* a, float* y, int64_t ldy, void* stream) {
  static const char* who = "dgcnn_interp_f32";
  DG_REQUIRE(feat && idx && dist && y, DGCNN_EINVAL, "%s: null feat, idx, dist or y", who);
  if (int rc = check_graph(who, q_rows, p_rows, M, N, k, F)) return rc;
  DG_REQUIRE(eps >= 1e-30f && eps < INFINITY, DGCNN_EINVAL, "%s: eps=%g must be finite and at least 1e-30", who, (double)eps);
  DG_REQUIRE(ldf >= F && ldy >= F && ldf % 4 == 0 && ldy % 4 == 0, DGCNN_EINVAL,
             "%s: leading dimensions must be multiples of 4 and at least F (ldf=%lld, ldy=%lld, F=%d)", who, (long long)ldf,
             (long long)ldy, F);
  DG_REQUIRE(a16(feat) && a16(y), DGCNN_EINVAL, "%s: feat and y must be 16-byte aligned", who);
  const int FV = F / 4;
  int RB = IT / FV;
  if (RB > FWD_E / k) RB = FWD_E / k;
  dg::launch(interp_fwd_kernel, dim3((unsigned)dg::cdiv(q_rows, RB)), dim3(IT), 0, ST, feat, ldf, idx, dist, q_rows, M, N, k, FV, RB,
             eps, a, y, ldy);
  return dg::check_launch(who);
}

// ws = [off: p_rows + 1 ints | counts: p_rows ints | rev: q_rows k ints | srt: q_rows k ints], every part rounded up to 256 bytes.
// srt first holds every edge's slot in its bucket (count -> fill), then the buckets in ascending edge order (rank -> gather).
extern "C" int64_t dgcnn_interp_bwd_workspace_bytes(int q_rows, int p_rows, int k) {
  if (q_rows <= 0 || p_rows <= 0 || k <= 0 || (int64_t)q_rows * k >= (1ll << 31)) return 0;
  return pad256(4 * ((int64_t)p_rows + 1)) + pad256(4 * (int64_t)p_rows) + 2 * pad256(4 * (int64_t)q_rows * k);
}

extern "C" int dgcnn_interp_bwd_f32(const float* dy, int64_t lddy, const int32_t* idx, const float* a, int q_rows, int p_rows, int M,
                                    int N, int k, int F, float* dfeat, int64_t lddf, int beta, void* ws, size_t ws_bytes,
                                    void* stream) {
  static const char* who = "dgcnn_interp_bwd_f32";
  DG_REQUIRE(dy && idx && a && dfeat && ws, DGCNN_EINVAL, "%s: null dy, idx, a, dfeat or ws", who);
  if (int rc = check_graph(who, q_rows, p_rows, M, N, k, F)) return rc;
  DG_REQUIRE(beta == 0 || beta == 1, DGCNN_EINVAL, "%s: beta must be 0 or 1 (got %d)", who, beta);
  DG_REQUIRE(lddy >= F && lddf >= F && lddy % 4 == 0 && lddf % 4 == 0, DGCNN_EINVAL,
             "%s: leading dimensions must be multiples of 4 and at least F (lddy=%lld, lddf=%lld, F=%d)", who, (long long)lddy,
             (long long)lddf, F);
  DG_REQUIRE(a16(dy) && a16(dfeat) && a16(ws), DGCNN_EINVAL, "%s: dy, dfeat and the workspace must be 16-byte aligned", who);
  DG_REQUIRE((int64_t)ws_bytes >= dgcnn_interp_bwd_workspace_bytes(q_rows, p_rows, k), DGCNN_ENOSPC,
             "%s: workspace too small (%lld bytes needed)", who, (long long)dgcnn_interp_bwd_workspace_bytes(q_rows, p_rows, k));
  const unsigned total = (unsigned)((int64_t)q_rows * k);
  char* w = reinterpret_cast<char*>(ws);
  int32_t* off = reinterpret_cast<int32_t*>(w);
  int32_t* cnt = reinterpret_cast<int32_t*>(w + pad256(4 * ((int64_t)p_rows + 1)));
  int32_t* rev = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(cnt) + pad256(4 * (int64_t)p_rows));
  int32_t* srt = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(rev) + pad256(4 * (int64_t)total));
  if (int rc = dg::memset_async(cnt, 0, sizeof(int32_t) * (size_t)p_rows, ST)) return rc;
  dg::launch(interp_count_kernel, dim3(grid1d(total, IT)), dim3(IT), 0, ST, idx, total, (unsigned)k, (unsigned)M, (unsigned)N, cnt, srt);
  dg::launch(interp_scan_kernel, dim3(1), dim3(1024), 0, ST, cnt, p_rows, off);
  dg::launch(interp_fill_kernel, dim3(grid1d(total, IT)), dim3(IT), 0, ST, idx, total, (unsigned)k, (unsigned)M, (unsigned)N, off, srt, rev);
  dg::launch(interp_rank_kernel, dim3(grid1d(total, IT)), dim3(IT), 0, ST, idx, total, (unsigned)k, (unsigned)M, (unsigned)N, off, rev, srt);
  const int FV = F / 4;
  dg::launch(interp_bwd_gather_kernel, dim3(grid1d((int64_t)p_rows * FV, IT)), dim3(IT), 0, ST, dy, lddy, a, off, srt, (int64_t)p_rows,
             (unsigned)k, FV, dfeat, lddf, beta);
  return dg::check_launch(who);
}

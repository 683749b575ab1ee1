// seg_bn.hip -- BatchNorm of a PACKED tower with the statistics of the row's OWN cloud (forward only).  Cloud b = rows
// [seg_off[b], seg_off[b + 1]) of the tower; the statistics are double[nseg][2][F] (sum, sum of squares per cloud), mean / rstd are
// float[nseg][F] tables, and the apply passes pick the table row through the row -> cloud map.  With these, a cloud's outputs do not
// depend on which other clouds share its tower: packed inference reproduces the inference of every cloud alone.
//
// The two statistics kernels sum in ONE fixed order (no atomics variant): stage 1 works over 64-row chunks of the tower cut at the
// cloud boundaries inside them (seg.hip: grids over chunks, never one workgroup per cloud), every (chunk, cloud) piece leaves its
// workgroup as one double per (sum, column) in partial slot (chunk + b) -- slots grow strictly with (chunk, b), so the pieces of
// cloud b are a contiguous run; stage 2 adds a cloud's slots first chunk to last, in double.
#include "gemm_common.h"

namespace {

constexpr int SEG_CHUNK = 64;   // rows of the tower per workgroup (stage 1 of both statistics kernels)
constexpr int SEG_WAVES = 4;    // k = 1 statistics: wave w owns rows w, w + 4, ... of a piece
constexpr int SEG_UNROLL = 4;   // independent row loads in flight per lane

inline unsigned grid1d(int64_t n, int bs = 256) {
  int64_t g = dg::cdiv(n, bs);
  if (g > 65536) g = 65536;
  if (g < 1) g = 1;
  return (unsigned)g;
}

#define GRID_STRIDE(i, n) \
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

// the cloud that holds row r: the largest b in [0, nseg) with seg_off[b] <= r
__device__ __forceinline__ int cloud_of_row(const int32_t* __restrict__ seg_off, int nseg, int r) {
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (seg_off[mid] <= r) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// bn.hip's definition of xhat and z, operation for operation (the library is built with -ffp-contract=off): a one-cloud tower
// gives the dense kernels' outputs bit for bit
__device__ __forceinline__ float bn_z(float y, float mu, float rs, float be, int relu) {
  const float xh = (y - mu) * rs;
  float z = xh + be;
  if (relu) z = fmaxf(z, 0.f);
  return z;
}

template <int V> struct Vec;
template <> struct Vec<4> {
  static __device__ __forceinline__ void ld(const float* p, float (&o)[4]) {
    const float4 v = *reinterpret_cast<const float4*>(p); o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; }
  static __device__ __forceinline__ void st(float* p, const float (&o)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]); }
};
template <> struct Vec<1> {
  static __device__ __forceinline__ void ld(const float* p, float (&o)[1]) { o[0] = *p; }
  static __device__ __forceinline__ void st(float* p, const float (&o)[1]) { *p = o[0]; }
};

// ---- statistics of a materialised (rows, F) tensor (the k = 1 layers), stage 1 -------------------------------------------------
// grid = (row chunks, column blocks of 64 * VW), lane = VW adjacent columns.  A wave sums its <= 16 rows of the piece in fp32
// (ascending), the four waves are added in double (0..3): part[chunk + b][2][F].
template <int VW>
__global__ __launch_bounds__(64 * SEG_WAVES) void seg_colstats_partial_kernel(const float* __restrict__ x, int64_t ldx, int rows, int F,
                                                                              const int32_t* __restrict__ seg_off, int nseg,
                                                                              double* __restrict__ part) {
  __shared__ float sv[2][SEG_WAVES][64 * VW];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c0 = (blockIdx.y * 64 + lane) * VW;
  const bool col_ok = c0 < F;                                 // (VW = 4: F % 4 == 0, a quad is inside or outside as a whole)
  const int chunk = blockIdx.x;
  const int r0 = chunk * SEG_CHUNK;
  const int r1 = imin(r0 + SEG_CHUNK, rows);
  int b = cloud_of_row(seg_off, nseg, r0);
  int ps = r0;
  while (ps < r1 && b < nseg) {
    const int pe = imin(seg_off[b + 1], r1);
    float s[VW], q[VW];
#pragma unroll
    for (int j = 0; j < VW; ++j) { s[j] = 0.f; q[j] = 0.f; }
    if (col_ok) {
      const float* p = x + c0;
      int i = ps + w;
      for (; i + (SEG_UNROLL - 1) * SEG_WAVES < pe; i += SEG_UNROLL * SEG_WAVES) {
        float v[SEG_UNROLL][VW];
#pragma unroll
        for (int u = 0; u < SEG_UNROLL; ++u) Vec<VW>::ld(p + (int64_t)(i + u * SEG_WAVES) * ldx, v[u]);
#pragma unroll
        for (int u = 0; u < SEG_UNROLL; ++u)
#pragma unroll
          for (int j = 0; j < VW; ++j) { s[j] += v[u][j]; q[j] += v[u][j] * v[u][j]; }
      }
      for (; i < pe; i += SEG_WAVES) {
        float v[VW];
        Vec<VW>::ld(p + (int64_t)i * ldx, v);
#pragma unroll
        for (int j = 0; j < VW; ++j) { s[j] += v[j]; q[j] += v[j] * v[j]; }
      }
    }
#pragma unroll
    for (int j = 0; j < VW; ++j) { sv[0][w][lane * VW + j] = s[j]; sv[1][w][lane * VW + j] = q[j]; }
    __syncthreads();
    // one thread per (sum, column) of the block's 2 * 64 * VW: coalesced double stores
    for (int e = threadIdx.x; e < 2 * 64 * VW; e += 64 * SEG_WAVES) {
      const int which = e / (64 * VW), cl = e % (64 * VW);
      const int col = blockIdx.y * 64 * VW + cl;
      double t = 0.0;
      for (int ww = 0; ww < SEG_WAVES; ++ww) t += (double)sv[which][ww][cl];
      if (col < F) part[((int64_t)(chunk + b) * 2 + which) * F + col] = t;
    }
    __syncthreads();
    ps = pe;
    ++b;
  }
}

// ---- statistics of the never-materialised conv0 output y = V[idx[r, m]] + U[r] (idx holds tower rows), stage 1 -------------------
// One workgroup per chunk; F / 4 lanes own a point (its U quad in registers, its k neighbour rows four at a time: the point-major
// layout and the single fp32 add of edge_gather_add_kernel, so values recomputed by the apply pass compare equal), RP = 256 / (F / 4)
// points side by side.  A point's k terms are summed in fp32, the points of a group in double (ascending), the RP groups in double
// (ascending).  XCD x (blockIdx % 8) owns the x-th eighth of the chunks -- consecutive chunks on one XCD -- so the V rows an XCD's
// L2 holds at any moment belong to few clouds.
__global__ __launch_bounds__(256) void seg_edge_stats_partial_kernel(const float* __restrict__ V, int64_t ldv, const float* __restrict__ U,
                                                                     int64_t ldu, const int32_t* __restrict__ idx, int rows, int knn,
                                                                     int F, const int32_t* __restrict__ seg_off, int nseg, int chunks,
                                                                     double* __restrict__ part) {
  __shared__ double red[2 * 1024];                            // [group][2][F], RP * 2 * F = 2048 doubles
  const int per = (chunks + 7) >> 3;
  const int chunk = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
  if ((int)(blockIdx.x >> 3) >= per || chunk >= chunks) return;   // (workgroup-uniform)
  const int FV = F >> 2;
  const int RP = 256 / FV;
  const int t = threadIdx.x;
  const bool active = t < RP * FV;
  const int g = t / FV;
  const int f = (t % FV) * 4;
  const int r0 = chunk * SEG_CHUNK;
  const int r1 = imin(r0 + SEG_CHUNK, rows);
  int b = cloud_of_row(seg_off, nseg, r0);
  int ps = r0;
  while (ps < r1 && b < nseg) {
    const int pe = imin(seg_off[b + 1], r1);
    double ds[4] = {0.0, 0.0, 0.0, 0.0}, dq[4] = {0.0, 0.0, 0.0, 0.0};
    if (active) {
      for (int i = ps + g; i < pe; i += RP) {
        const int32_t* ip = idx + (int64_t)i * knn;
        const float4 u = *reinterpret_cast<const float4*>(U + (int64_t)i * ldu + f);
        float cs[4] = {0.f, 0.f, 0.f, 0.f}, cq[4] = {0.f, 0.f, 0.f, 0.f};
        for (int m = 0; m < knn; m += 4) {
          int row[4];
          float4 v[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) row[j] = ip[(m + j < knn) ? (m + j) : (knn - 1)];
#pragma unroll
          for (int j = 0; j < 4; ++j)   // (full-rate 24-bit multiply: rows, ldv < 2^24, rows * ldv < 2^32: host check)
            v[j] = *reinterpret_cast<const float4*>(V + f + __umul24((unsigned)row[j], (unsigned)ldv));
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (m + j < knn) {
              const float4 y = make_float4(v[j].x + u.x, v[j].y + u.y, v[j].z + u.z, v[j].w + u.w);
              cs[0] += y.x; cs[1] += y.y; cs[2] += y.z; cs[3] += y.w;
              cq[0] += y.x * y.x; cq[1] += y.y * y.y; cq[2] += y.z * y.z; cq[3] += y.w * y.w;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) { ds[j] += (double)cs[j]; dq[j] += (double)cq[j]; }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        red[(g * 2 + 0) * F + f + j] = ds[j];
        red[(g * 2 + 1) * F + f + j] = dq[j];
      }
    }
    __syncthreads();
    for (int e = t; e < 2 * F; e += 256) {
      const int which = e / F, c = e % F;
      double a = 0.0;
      for (int gg = 0; gg < RP; ++gg) a += red[(gg * 2 + which) * F + c];
      part[((int64_t)(chunk + b) * 2 + which) * F + c] = a;
    }
    __syncthreads();
    ps = pe;
    ++b;
  }
}

// stage 2 of both: stats[b][which][f] = the partial slots of cloud b, first chunk to last
__global__ void seg_stats_final_kernel(const double* __restrict__ part, const int32_t* __restrict__ seg_off, int F, int64_t total,
                                       double* __restrict__ stats) {
  GRID_STRIDE(i, total) {
    const int b = (int)(i / (2 * F));
    const int e = (int)(i % (2 * F));                        // which * F + f
    const int cfirst = seg_off[b] / SEG_CHUNK, clast = (seg_off[b + 1] - 1) / SEG_CHUNK;
    double t = 0.0;
    for (int c = cfirst; c <= clast; ++c) t += part[(int64_t)(c + b) * 2 * F + e];
    stats[i] = t;
  }
}

// bn_finalize_kernel's arithmetic per (cloud, column): double, biased variance clamped at 0
__global__ void seg_bn_finalize_kernel(const double* __restrict__ stats, int F, int64_t total, const int32_t* __restrict__ seg_off,
                                       int k, float eps, float* __restrict__ mean, float* __restrict__ rstd) {
  GRID_STRIDE(i, total) {
    const int b = (int)(i / F);
    const int f = (int)(i % F);
    const double count = (double)(seg_off[b + 1] - seg_off[b]) * (double)k;
    const double s = stats[((int64_t)b * 2 + 0) * F + f], q = stats[((int64_t)b * 2 + 1) * F + f];
    const double mu = s / count;
    double var = q / count - mu * mu;
    if (var < 0.0) var = 0.0;
    mean[i] = (float)mu;
    rstd[i] = (float)(1.0 / sqrt(var + (double)eps));
  }
}

// ---- k = 1: out[r] = act(bn_z(T[r]; mean[g], rstd[g], beta)), g = row_group[r] (row_group == nullptr: g = r) ----------------------
template <int VW>
__global__ __launch_bounds__(256) void seg_bn_act_kernel(const float* __restrict__ T, int64_t ldt, int64_t rows, int F,
                                                         const int32_t* __restrict__ row_group, const float* __restrict__ mean,
                                                         const float* __restrict__ rstd, const float* __restrict__ beta, int relu,
                                                         float* __restrict__ out, int64_t ldo, float* __restrict__ out2, int64_t ldo2) {
  const int FV = F / VW;
  GRID_STRIDE(it, rows * FV) {
    const int64_t r = it / FV;
    const int f = (int)(it % FV) * VW;
    const int64_t g = row_group ? (int64_t)row_group[r] : r;
    float y[VW], mu[VW], rs[VW], be[VW], z[VW];
    Vec<VW>::ld(T + r * ldt + f, y);
    Vec<VW>::ld(mean + g * F + f, mu);
    Vec<VW>::ld(rstd + g * F + f, rs);
    Vec<VW>::ld(beta + f, be);
#pragma unroll
    for (int j = 0; j < VW; ++j) z[j] = bn_z(y[j], mu[j], rs[j], be[j], relu);
    Vec<VW>::st(out + r * ldo + f, z);
    if (out2) Vec<VW>::st(out2 + r * ldo2 + f, z);
  }
}

// ---- conv0: BN + ReLU + max / mean over the k recomputed edge rows of each point, with the table row of the point's cloud ---------
// item = (point, channel quad); XCD x (blockIdx % 8) owns the x-th eighth of the points and its blocks sweep it side by side (the
// item map of bn.hip's edge kernels).  The k terms of the mean are added in ascending m and scaled by 1.0f / k, as there.
__global__ __launch_bounds__(256) void seg_edge_bn_act_kreduce_kernel(const float* __restrict__ V, int64_t ldv, const float* __restrict__ U,
                                                                      int64_t ldu, const int32_t* __restrict__ idx, int64_t rows, int k,
                                                                      int F, const int32_t* __restrict__ row_group,
                                                                      const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                      const float* __restrict__ beta, int relu, float* __restrict__ max_out,
                                                                      int64_t ldmax, float* __restrict__ mean_out, int64_t ldmean) {
  const int FV = F >> 2;
  const int64_t per = (rows + 7) / 8;
  const int64_t rb = (int64_t)(blockIdx.x & 7) * per;
  int64_t nr = rows - rb;
  nr = nr < 0 ? 0 : (nr > per ? per : nr);
  const int64_t count = nr * FV;
  const int64_t step = (int64_t)(gridDim.x >> 3) * blockDim.x;
  const float invk = 1.0f / (float)k;
  for (int64_t q = (int64_t)(blockIdx.x >> 3) * blockDim.x + threadIdx.x; q < count; q += step) {
    const unsigned qu = (unsigned)q;                          // (rows < 2^24, FV <= 256: an eighth of the items fits 32 bits)
    const int64_t r = rb + qu / (unsigned)FV;
    const int f = (int)(qu % (unsigned)FV) * 4;
    const int64_t g = row_group[r];
    float mu[4], rs[4], be[4], u[4], mx[4], sm[4];
    Vec<4>::ld(mean + g * F + f, mu); Vec<4>::ld(rstd + g * F + f, rs); Vec<4>::ld(beta + f, be);
    Vec<4>::ld(U + r * ldu + f, u);
#pragma unroll
    for (int j = 0; j < 4; ++j) { mx[j] = -INFINITY; sm[j] = 0.f; }
    const int32_t* ip = idx + r * k;
    const float* vb = V + f;
    for (int m = 0; m < k; m += 4) {
      unsigned row[4];
      float y[4][4];
#pragma unroll
      for (int j = 0; j < 4; ++j) row[j] = __umul24((unsigned)ip[(m + j < k) ? (m + j) : (k - 1)], (unsigned)ldv);
#pragma unroll
      for (int j = 0; j < 4; ++j) Vec<4>::ld(vb + row[j], y[j]);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (m + j < k) {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float z = bn_z(y[j][c] + u[c], mu[c], rs[c], be[c], relu);
            mx[c] = (z > mx[c]) ? z : mx[c];
            sm[c] += z;
          }
        }
    }
    Vec<4>::st(max_out + r * ldmax + f, mx);
    if (mean_out) {
#pragma unroll
      for (int c = 0; c < 4; ++c) sm[c] *= invk;
      Vec<4>::st(mean_out + r * ldmean + f, sm);
    }
  }
}

inline bool a16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline unsigned grid_items(int64_t items) {
  int64_t g = dg::cdiv(items, 256);
  if (g > 256 * 16) g = 256 * 16;
  if (g < 1) g = 1;
  return (unsigned)g;
}

// the checks the two gather-sourced entries share (dgcnn_edge_gather_add_f32's conditions with one "cloud" of `rows` points: idx
// holds tower rows)
int check_seg_edge(const char* what, const float* V, int64_t ldv, const float* U, int64_t ldu, const int32_t* idx, int rows, int k,
                   int F) {
  DG_REQUIRE(V && U && idx, DGCNN_EINVAL, "%s: null pointer", what);
  DG_REQUIRE(rows > 0 && k > 0 && F > 0, DGCNN_EINVAL, "%s: bad shape", what);
  DG_REQUIRE(F % 4 == 0 && F <= 1024, DGCNN_EUNSUP, "%s: F must be a multiple of 4, <= 1024 (got %d)", what, F);
  DG_REQUIRE((int64_t)rows * k < (1ll << 31), DGCNN_EUNSUP, "%s: rows * k >= 2^31", what);
  DG_REQUIRE(rows < (1 << 24) && ldv < (1 << 24) && (int64_t)rows * ldv < (1ll << 32), DGCNN_EUNSUP,
             "%s: rows * ldv must be < 2^32 elements (32-bit row offsets inside the tower)", what);
  DG_REQUIRE(a16(V) && a16(U) && ldv % 4 == 0 && ldu % 4 == 0 && ldv >= F && ldu >= F, DGCNN_EINVAL,
             "%s: V, U must be 16-byte aligned with leading dimensions %% 4 == 0", what);
  return DGCNN_OK;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int64_t dgcnn_seg_stats_workspace_bytes(int rows, int nseg, int F) {
  if (rows <= 0 || nseg <= 0 || F <= 0) return 0;
  return (dg::cdiv(rows, SEG_CHUNK) + nseg) * 2 * (int64_t)F * (int64_t)sizeof(double);
}

static int seg_stats_final(const char* what, const double* part, const int32_t* seg_off, int nseg, int F, double* stats,
                           hipStream_t st) {
  int rc = dg::check_launch(what);
  if (rc) return rc;
  const int64_t total = (int64_t)nseg * 2 * F;
  dg::launch(seg_stats_final_kernel, dim3(grid1d(total)), dim3(256), 0, st, part, seg_off, F, total, stats);
  return dg::check_launch(what);
}

extern "C" int dgcnn_seg_colstats_f32(const float* x, int64_t ldx, int rows, int F, const int32_t* seg_off, int nseg, double* stats,
                                      void* ws, size_t ws_bytes, void* stream) {
  DG_REQUIRE(x && seg_off && stats && rows > 0 && F > 0 && nseg > 0 && nseg <= rows && ldx >= F, DGCNN_EINVAL,
             "dgcnn_seg_colstats_f32: bad args");
  const size_t need = (size_t)dgcnn_seg_stats_workspace_bytes(rows, nseg, F);
  DG_REQUIRE(ws && ws_bytes >= need && (reinterpret_cast<uintptr_t>(ws) & 7) == 0, DGCNN_ENOSPC,
             "dgcnn_seg_colstats_f32: workspace too small or not 8-byte aligned (%zu < %zu bytes)", ws_bytes, need);
  double* part = reinterpret_cast<double*>(ws);
  const unsigned chunks = (unsigned)dg::cdiv(rows, SEG_CHUNK);
  if (F % 4 == 0 && ldx % 4 == 0 && a16(x))
    dg::launch(seg_colstats_partial_kernel<4>, dim3(chunks, (unsigned)dg::cdiv(F, 256)), dim3(64 * SEG_WAVES), 0, ST, x, ldx, rows, F,
               seg_off, nseg, part);
  else
    dg::launch(seg_colstats_partial_kernel<1>, dim3(chunks, (unsigned)dg::cdiv(F, 64)), dim3(64 * SEG_WAVES), 0, ST, x, ldx, rows, F,
               seg_off, nseg, part);
  return seg_stats_final("dgcnn_seg_colstats_f32", part, seg_off, nseg, F, stats, ST);
}

extern "C" int dgcnn_seg_edge_stats_f32(const float* V, int64_t ldv, const float* U, int64_t ldu, const int32_t* idx, int rows, int k,
                                        int F, const int32_t* seg_off, int nseg, double* stats, void* ws, size_t ws_bytes,
                                        void* stream) {
  int rc = check_seg_edge("dgcnn_seg_edge_stats_f32", V, ldv, U, ldu, idx, rows, k, F);
  if (rc) return rc;
  DG_REQUIRE(seg_off && stats && nseg > 0 && nseg <= rows, DGCNN_EINVAL, "dgcnn_seg_edge_stats_f32: bad args");
  const size_t need = (size_t)dgcnn_seg_stats_workspace_bytes(rows, nseg, F);
  DG_REQUIRE(ws && ws_bytes >= need && (reinterpret_cast<uintptr_t>(ws) & 7) == 0, DGCNN_ENOSPC,
             "dgcnn_seg_edge_stats_f32: workspace too small or not 8-byte aligned (%zu < %zu bytes)", ws_bytes, need);
  double* part = reinterpret_cast<double*>(ws);
  const int chunks = (int)dg::cdiv(rows, SEG_CHUNK);
  const unsigned grid = 8u * (unsigned)dg::cdiv(chunks, 8);
  dg::launch(seg_edge_stats_partial_kernel, dim3(grid), dim3(256), 0, ST, V, ldv, U, ldu, idx, rows, k, F, seg_off, nseg, chunks, part);
  return seg_stats_final("dgcnn_seg_edge_stats_f32", part, seg_off, nseg, F, stats, ST);
}

extern "C" int dgcnn_seg_bn_finalize_f32(const double* stats, int nseg, int F, const int32_t* seg_off, int k, float eps, float* mean,
                                         float* rstd, void* stream) {
  DG_REQUIRE(stats && seg_off && mean && rstd && nseg > 0 && F > 0 && k > 0, DGCNN_EINVAL, "dgcnn_seg_bn_finalize_f32: bad args");
  const int64_t total = (int64_t)nseg * F;
  dg::launch(seg_bn_finalize_kernel, dim3(grid1d(total)), dim3(256), 0, ST, stats, F, total, seg_off, k, eps, mean, rstd);
  return dg::check_launch("dgcnn_seg_bn_finalize_f32");
}

extern "C" int dgcnn_seg_bn_act_f32(const float* T, int64_t ldt, int rows, int F, const int32_t* row_group, const float* mean,
                                    const float* rstd, const float* beta, int relu, float* out, int64_t ldo, float* out2, int64_t ldo2,
                                    void* stream) {
  DG_REQUIRE(T && mean && rstd && beta && out && rows > 0 && F > 0 && ldt >= F && ldo >= F && (!out2 || ldo2 >= F), DGCNN_EINVAL,
             "dgcnn_seg_bn_act_f32: bad args");
  DG_REQUIRE(relu == 0 || relu == 1, DGCNN_EINVAL, "dgcnn_seg_bn_act_f32: relu must be 0 or 1 (got %d)", relu);
  const bool vec = F % 4 == 0 && ldt % 4 == 0 && ldo % 4 == 0 && a16(T) && a16(out) && a16(mean) && a16(rstd) && a16(beta) &&
                   (!out2 || (ldo2 % 4 == 0 && a16(out2)));
  if (vec)
    dg::launch(seg_bn_act_kernel<4>, dim3(grid_items((int64_t)rows * (F / 4))), dim3(256), 0, ST, T, ldt, (int64_t)rows, F, row_group,
               mean, rstd, beta, relu, out, ldo, out2, ldo2);
  else
    dg::launch(seg_bn_act_kernel<1>, dim3(grid_items((int64_t)rows * F)), dim3(256), 0, ST, T, ldt, (int64_t)rows, F, row_group, mean,
               rstd, beta, relu, out, ldo, out2, ldo2);
  return dg::check_launch("dgcnn_seg_bn_act_f32");
}

extern "C" int dgcnn_seg_edge_bn_act_kreduce_f32(const float* V, int64_t ldv, const float* U, int64_t ldu, const int32_t* idx, int rows,
                                                 int k, int F, const int32_t* row_group, const float* mean, const float* rstd,
                                                 const float* beta, int relu, float* max_out, int64_t ldmax, float* mean_out,
                                                 int64_t ldmean, void* stream) {
  int rc = check_seg_edge("dgcnn_seg_edge_bn_act_kreduce_f32", V, ldv, U, ldu, idx, rows, k, F);
  if (rc) return rc;
  DG_REQUIRE(row_group && mean && rstd && beta && max_out, DGCNN_EINVAL, "dgcnn_seg_edge_bn_act_kreduce_f32: null pointer");
  DG_REQUIRE(relu == 0 || relu == 1, DGCNN_EINVAL, "dgcnn_seg_edge_bn_act_kreduce_f32: relu must be 0 or 1 (got %d)", relu);
  DG_REQUIRE(ldmax >= F && ldmax % 4 == 0 && a16(max_out) && a16(mean) && a16(rstd) && a16(beta) &&
                 (!mean_out || (ldmean >= F && ldmean % 4 == 0 && a16(mean_out))),
             DGCNN_EINVAL, "dgcnn_seg_edge_bn_act_kreduce_f32: outputs and tables must be 16-byte aligned with leading dimensions %% 4 == 0");
  const unsigned grid = (grid_items((int64_t)rows * (F / 4)) + 7u) & ~7u;     // (the XCD item map needs a multiple of 8)
  dg::launch(seg_edge_bn_act_kreduce_kernel, dim3(grid), dim3(256), 0, ST, V, ldv, U, ldu, idx, (int64_t)rows, k, F, row_group, mean, rstd,
             beta, relu, max_out, ldmax, mean_out, ldmean);
  return dg::check_launch("dgcnn_seg_edge_bn_act_kreduce_f32");
}

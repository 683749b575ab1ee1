// seg_bn.hip -- BatchNorm of a PACKED tower with the statistics of the row's OWN cloud, forward and backward.  Cloud b = rows
// [seg_off[b], seg_off[b + 1]) of the tower; the statistics are double[nseg][2][F] (sum, sum of squares per cloud), mean / rstd are
// float[nseg][F] tables, and the apply passes pick the table row through the row -> cloud map.  With these, a cloud's outputs do not
// depend on which other clouds share its tower: packed inference reproduces the inference of every cloud alone.
//
// The two statistics kernels sum in ONE fixed order (no atomics variant): stage 1 works over 64-row chunks of the tower cut at the
// cloud boundaries inside them (seg.hip: grids over chunks, never one workgroup per cloud), every (chunk, cloud) piece leaves its
// workgroup as one double per (sum, column) in partial slot (chunk + b) -- slots grow strictly with (chunk, b), so the pieces of
// cloud b are a contiguous run; stage 2 adds a cloud's slots first chunk to last, in double.
//
// The backward (second half of the file) takes its per-cloud sums red = double[nseg][2][F] (sum dz, sum dz * xhat) by the same two
// stages, turns them into the float tables c1 / c2 = red / (n_b k) and applies dY = rstd_g ((dz - c1_g) - xhat c2_g) through the
// row -> cloud map.
//
// The element arithmetic (xhat, z, the packed count, dz, dY) is bn_common.h's, shared with bn.hip's dense kernels: a one-cloud tower
// gives their outputs bit for bit.
#include "gemm_common.h"
#include "bn_common.h"

namespace {

constexpr int SEG_CHUNK = 64;   // rows of the tower per workgroup (stage 1 of both statistics kernels)
constexpr int SEG_WAVES = 4;    // k = 1 statistics: wave w owns rows w, w + 4, ... of a piece
constexpr int SEG_UNROLL = 4;   // independent row loads in flight per lane

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
          for (int j = 0; j < 4; ++j)   // (rows, ldv < 2^24, rows * ldv < 2^32: host check; offsets of 2^31 and more zero-extended)
            v[j] = *reinterpret_cast<const float4*>(V + f + row_offset24((unsigned)row[j], (unsigned)ldv));
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
// CNT: also cnt_out (rows, F) = the packed count of bn_common.h (k < CNT_POS), which the backward reads; max_out / mean_out are
// formed by the same instructions in both instantiations.
template <bool CNT>
__global__ __launch_bounds__(256) void seg_edge_bn_act_kreduce_kernel(const float* __restrict__ V, int64_t ldv, const float* __restrict__ U,
                                                                      int64_t ldu, const int32_t* __restrict__ idx, int64_t rows, int k,
                                                                      int F, const int32_t* __restrict__ row_group,
                                                                      const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                      const float* __restrict__ beta, int relu, float* __restrict__ max_out,
                                                                      int64_t ldmax, float* __restrict__ mean_out, int64_t ldmean,
                                                                      float* __restrict__ cnt_out) {
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
    float mu[4], rs[4], be[4], u[4], mx[4], sm[4], cn[4], np[4];
    Vec<4>::ld(mean + g * F + f, mu); Vec<4>::ld(rstd + g * F + f, rs); Vec<4>::ld(beta + f, be);
    Vec<4>::ld(U + r * ldu + f, u);
#pragma unroll
    for (int j = 0; j < 4; ++j) { mx[j] = -INFINITY; sm[j] = 0.f; cn[j] = 0.f; np[j] = 0.f; }
    const int32_t* ip = idx + r * k;
    const float* vb = V + f;
    for (int m = 0; m < k; m += 4) {
      unsigned row[4];
      float y[4][4];
#pragma unroll
      for (int j = 0; j < 4; ++j) row[j] = row_offset24((unsigned)ip[(m + j < k) ? (m + j) : (k - 1)], (unsigned)ldv);
#pragma unroll
      for (int j = 0; j < 4; ++j) Vec<4>::ld(vb + row[j], y[j]);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (m + j < k) {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float z = bn_z(y[j][c] + u[c], mu[c], rs[c], be[c], relu);
            if (CNT) {
              cn[c] = (z > mx[c]) ? 1.f : ((z == mx[c]) ? cn[c] + 1.f : cn[c]);
              np[c] += cnt_pos_term(z);
            }
            mx[c] = (z > mx[c]) ? z : mx[c];
            sm[c] += z;
          }
        }
    }
    Vec<4>::st(max_out + r * ldmax + f, mx);
    if (CNT) {
#pragma unroll
      for (int c = 0; c < 4; ++c) cn[c] += np[c];
      Vec<4>::st(cnt_out + r * F + f, cn);
    }
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
  DG_REQUIRE(row_offset24_ok(rows, ldv), DGCNN_EUNSUP,
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

static int seg_edge_act_kreduce(const char* what, const float* V, int64_t ldv, const float* U, int64_t ldu, const int32_t* idx, int rows,
                                int k, int F, const int32_t* row_group, const float* mean, const float* rstd, const float* beta, int relu,
                                float* max_out, int64_t ldmax, float* mean_out, int64_t ldmean, float* cnt_out, bool cnt, hipStream_t st) {
  int rc = check_seg_edge(what, V, ldv, U, ldu, idx, rows, k, F);
  if (rc) return rc;
  DG_REQUIRE(row_group && mean && rstd && beta && max_out && (!cnt || cnt_out), DGCNN_EINVAL, "%s: null pointer", what);
  DG_REQUIRE(relu == 0 || relu == 1, DGCNN_EINVAL, "%s: relu must be 0 or 1 (got %d)", what, relu);
  DG_REQUIRE(!cnt || k < CNT_POS, DGCNN_EUNSUP, "%s: k must be < %d (the packed tie / positive counts)", what, CNT_POS);
  DG_REQUIRE(ldmax >= F && ldmax % 4 == 0 && a16(max_out) && a16(mean) && a16(rstd) && a16(beta) &&
                 (!mean_out || (ldmean >= F && ldmean % 4 == 0 && a16(mean_out))) && (!cnt || a16(cnt_out)),
             DGCNN_EINVAL, "%s: outputs and tables must be 16-byte aligned with leading dimensions %% 4 == 0", what);
  const unsigned grid = (grid_items((int64_t)rows * (F / 4)) + 7u) & ~7u;     // (the XCD item map needs a multiple of 8)
  if (cnt)
    dg::launch(seg_edge_bn_act_kreduce_kernel<true>, dim3(grid), dim3(256), 0, st, V, ldv, U, ldu, idx, (int64_t)rows, k, F, row_group, mean,
               rstd, beta, relu, max_out, ldmax, mean_out, ldmean, cnt_out);
  else
    dg::launch(seg_edge_bn_act_kreduce_kernel<false>, dim3(grid), dim3(256), 0, st, V, ldv, U, ldu, idx, (int64_t)rows, k, F, row_group, mean,
               rstd, beta, relu, max_out, ldmax, mean_out, ldmean, (float*)nullptr);
  return dg::check_launch(what);
}

extern "C" int dgcnn_seg_edge_bn_act_kreduce_f32(const float* V, int64_t ldv, const float* U, int64_t ldu, const int32_t* idx, int rows,
                                                 int k, int F, const int32_t* row_group, const float* mean, const float* rstd,
                                                 const float* beta, int relu, float* max_out, int64_t ldmax, float* mean_out,
                                                 int64_t ldmean, void* stream) {
  return seg_edge_act_kreduce("dgcnn_seg_edge_bn_act_kreduce_f32", V, ldv, U, ldu, idx, rows, k, F, row_group, mean, rstd, beta, relu,
                              max_out, ldmax, mean_out, ldmean, nullptr, false, ST);
}

extern "C" int dgcnn_seg_edge_bn_act_kreduce_cnt_f32(const float* V, int64_t ldv, const float* U, int64_t ldu, const int32_t* idx, int rows,
                                                     int k, int F, const int32_t* row_group, const float* mean, const float* rstd,
                                                     const float* beta, int relu, float* max_out, int64_t ldmax, float* mean_out,
                                                     int64_t ldmean, float* cnt_out, void* stream) {
  return seg_edge_act_kreduce("dgcnn_seg_edge_bn_act_kreduce_cnt_f32", V, ldv, U, ldu, idx, rows, k, F, row_group, mean, rstd, beta, relu,
                              max_out, ldmax, mean_out, ldmean, cnt_out, true, ST);
}

// =====================================================================================================================================
// Backward.  red = double[nseg][2][F]: per cloud sum dz and sum dz * xhat (WRITTEN, not accumulated; not in the slot arena).
// =====================================================================================================================================
namespace {

// ---- what a row contributes to the two sums: the integrands of the two reduce kernels ---------------------------------------------
// k = 1 layers: dz = (dout + d2) [z > 0 if relu], terms (dz, dz * xhat) with z, xhat from bn_z -- bn1_bwd_kernel<false>'s row
template <int VW>
struct K1Terms {
  static constexpr int UNROLL = SEG_UNROLL;
  const float* T; int64_t ldt;
  const float* mean; const float* rstd; const float* beta; int relu;
  const float* dout; int64_t lddo;
  const float* d2; int64_t ldd2;
  struct Par { float mu[VW], rs[VW], be[VW]; };
  struct Row { float y[VW], d[VW], e[VW]; };
  __device__ __forceinline__ void par(int b, int F, int c0, Par& p) const {
    Vec<VW>::ld(mean + (int64_t)b * F + c0, p.mu); Vec<VW>::ld(rstd + (int64_t)b * F + c0, p.rs); Vec<VW>::ld(beta + c0, p.be);
  }
  __device__ __forceinline__ void load(int r, int c0, Row& v) const {
    Vec<VW>::ld(T + (int64_t)r * ldt + c0, v.y); Vec<VW>::ld(dout + (int64_t)r * lddo + c0, v.d);
    if (d2) Vec<VW>::ld(d2 + (int64_t)r * ldd2 + c0, v.e);
  }
  __device__ __forceinline__ void add(const Row& v, const Par& p, float (&s0)[VW], float (&s1)[VW]) const {
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      float xh;
      const float z = bn_z(v.y[j], p.mu[j], p.rs[j], p.be[j], relu, xh);
      const float dz = bn_dz_row(z, d2 ? v.d[j] + v.e[j] : v.d[j], relu);     // (two consumers of the output: one fp32 add)
      s0[j] += dz;
      s1[j] += dz * xh;
    }
  }
};

// conv0 (a ReLU layer): the k rows of a point in closed form from the forward's per-point outputs -- edge_bwd_reduce_points_kernel's
// row:  sum_m dz = [max > 0] dmax + dmean npos / k,   sum_m dz xhat = [max > 0] dmax (max - beta) + (dmean / k) (k mean - beta npos)
struct PointTerms {
  static constexpr int UNROLL = 2;
  const float* mx; int64_t ldmx;
  const float* mn; int64_t ldmn;
  const float* cntpos;
  const float* dmax; int64_t lddmax;
  const float* dmean; int64_t lddmean;
  const float* beta; int k; int F;                              // (cntpos is (rows, F) contiguous)
  struct Par { float be[4]; };
  struct Row { float a[4], b[4], c[4], d[4], e[4]; };
  __device__ __forceinline__ void par(int, int, int c0, Par& p) const { Vec<4>::ld(beta + c0, p.be); }
  __device__ __forceinline__ void load(int r, int c0, Row& v) const {
    Vec<4>::ld(mx + (int64_t)r * ldmx + c0, v.a); Vec<4>::ld(mn + (int64_t)r * ldmn + c0, v.b);
    Vec<4>::ld(cntpos + (int64_t)r * F + c0, v.c);
    Vec<4>::ld(dmax + (int64_t)r * lddmax + c0, v.d); Vec<4>::ld(dmean + (int64_t)r * lddmean + c0, v.e);
  }
  __device__ __forceinline__ void add(const Row& v, const Par& p, float (&s0)[4], float (&s1)[4]) const {
    const float invk = 1.0f / (float)k, kf = (float)k;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float npos = cnt_npos(v.c[j]);
      const float g1 = (v.a[j] > 0.f) ? v.d[j] : 0.f;
      const float g2 = v.e[j] * invk;
      s0[j] += g1 + g2 * npos;
      s1[j] += g1 * (v.a[j] - p.be[j]) + g2 * (kf * v.b[j] - p.be[j] * npos);
    }
  }
};

// ---- stage 1 of both reduces: seg_colstats_partial_kernel's scheme with the integrand TM.  grid = (row chunks, column blocks of
// 64 * VW); a wave sums its <= 16 rows of a (chunk, cloud) piece in fp32 (ascending), the four waves are added in double (0..3) into
// part[chunk + b][2][F]; seg_stats_final_kernel adds a cloud's slots.
template <int VW, class TM>
__global__ __launch_bounds__(64 * SEG_WAVES) void seg_bwd_partial_kernel(TM tm, int rows, int F, const int32_t* __restrict__ seg_off, int nseg,
                                                                         double* __restrict__ part) {
  __shared__ float sv[2][SEG_WAVES][64 * VW];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c0 = (blockIdx.y * 64 + lane) * VW;
  const bool col_ok = c0 < F;
  const int chunk = blockIdx.x;
  const int r0 = chunk * SEG_CHUNK;
  const int r1 = imin(r0 + SEG_CHUNK, rows);
  int b = cloud_of_row(seg_off, nseg, r0);
  int ps = r0;
  while (ps < r1 && b < nseg) {
    const int pe = imin(seg_off[b + 1], r1);
    float s0[VW], s1[VW];
#pragma unroll
    for (int j = 0; j < VW; ++j) { s0[j] = 0.f; s1[j] = 0.f; }
    if (col_ok) {
      typename TM::Par p;
      tm.par(b, F, c0, p);
      int i = ps + w;
      for (; i + (TM::UNROLL - 1) * SEG_WAVES < pe; i += TM::UNROLL * SEG_WAVES) {
        typename TM::Row v[TM::UNROLL];
#pragma unroll
        for (int u = 0; u < TM::UNROLL; ++u) tm.load(i + u * SEG_WAVES, c0, v[u]);
#pragma unroll
        for (int u = 0; u < TM::UNROLL; ++u) tm.add(v[u], p, s0, s1);
      }
      for (; i < pe; i += SEG_WAVES) {
        typename TM::Row v;
        tm.load(i, c0, v);
        tm.add(v, p, s0, s1);
      }
    }
#pragma unroll
    for (int j = 0; j < VW; ++j) { sv[0][w][lane * VW + j] = s0[j]; sv[1][w][lane * VW + j] = s1[j]; }
    __syncthreads();
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

// ---- c1[b][f] = float(red0 * (1.0 / (n_b k))), c2 likewise (bn_bwd_apply_kernel's constants, per cloud);
// dbeta[f] = dbeta_beta * dbeta[f] + float(sum_b red0[b][f]), b ascending, in double (bn_bwd_finalize_kernel's dbeta)
__global__ void seg_bn_bwd_finalize_kernel(const double* __restrict__ red, int nseg, int F, const int32_t* __restrict__ seg_off, int k,
                                           float* __restrict__ c1, float* __restrict__ c2, float* __restrict__ dbeta, float dbeta_beta) {
  const int64_t total = (int64_t)nseg * F;
  GRID_STRIDE(i, total) {
    const int b = (int)(i / F);
    const int f = (int)(i % F);
    const double inv_cnt = 1.0 / ((double)(seg_off[b + 1] - seg_off[b]) * (double)k);
    c1[i] = (float)(red[((int64_t)b * 2 + 0) * F + f] * inv_cnt);
    c2[i] = (float)(red[((int64_t)b * 2 + 1) * F + f] * inv_cnt);
    if (b == 0 && dbeta) {
      double s = 0.0;
      for (int bb = 0; bb < nseg; ++bb) s += red[(int64_t)bb * 2 * F + f];
      dbeta[f] = (dbeta_beta != 0.f) ? (float)s + dbeta_beta * dbeta[f] : (float)s;
    }
  }
}

// ---- k = 1: dT[r] = rstd_g ((dz - c1_g) - xhat c2_g), g = row_group[r]; dT may be T (an item reads its elements before it writes them)
template <int VW>
__global__ __launch_bounds__(256) void seg_bn_bwd_apply_kernel(const float* T, int64_t ldt, int64_t rows, int F,
                                                               const int32_t* __restrict__ row_group, const float* __restrict__ mean,
                                                               const float* __restrict__ rstd, const float* __restrict__ beta, int relu,
                                                               const float* __restrict__ dout, int64_t lddo, const float* __restrict__ d2,
                                                               int64_t ldd2, const float* __restrict__ c1, const float* __restrict__ c2,
                                                               float* dT, int64_t lddt) {
  const int FV = F / VW;
  GRID_STRIDE(it, rows * FV) {
    const int64_t r = it / FV;
    const int f = (int)(it % FV) * VW;
    const int64_t g = row_group[r];
    float y[VW], d[VW], mu[VW], rs[VW], be[VW], k1[VW], k2[VW], o[VW];
    Vec<VW>::ld(T + r * ldt + f, y);
    Vec<VW>::ld(dout + r * lddo + f, d);
    if (d2) {
      float e[VW];
      Vec<VW>::ld(d2 + r * ldd2 + f, e);
#pragma unroll
      for (int j = 0; j < VW; ++j) d[j] += e[j];
    }
    Vec<VW>::ld(mean + g * F + f, mu); Vec<VW>::ld(rstd + g * F + f, rs); Vec<VW>::ld(beta + f, be);
    Vec<VW>::ld(c1 + g * F + f, k1); Vec<VW>::ld(c2 + g * F + f, k2);
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      float xh;
      const float z = bn_z(y[j], mu[j], rs[j], be[j], relu, xh);
      o[j] = bn_dy(rs[j], bn_dz_row(z, d[j], relu), k1[j], xh, k2[j]);
    }
    Vec<VW>::st(dT + r * lddt + f, o);
  }
}

// ---- conv0: y = V[idx] + U and z recomputed by the forward's instruction sequence (z == mx compares equal to the maximum it took);
// dz = bn_dz_edge with dmax / ties and dmean * (1.0f / k); dY (rows * k, F) and dYsum (rows, F) = the k rows added in ascending m.
// The item map of seg_edge_bn_act_kreduce_kernel.
__global__ __launch_bounds__(256) void seg_edge_bn_bwd_apply_kernel(const float* __restrict__ V, int64_t ldv, const float* __restrict__ U,
                                                                    int64_t ldu, const int32_t* __restrict__ idx, int64_t rows, int k, int F,
                                                                    const int32_t* __restrict__ row_group, const float* __restrict__ mean,
                                                                    const float* __restrict__ rstd, const float* __restrict__ beta, int relu,
                                                                    const float* __restrict__ dmax, int64_t lddmax,
                                                                    const float* __restrict__ dmean, int64_t lddmean,
                                                                    const float* __restrict__ mx_in, int64_t ldmx,
                                                                    const float* __restrict__ cnt_in, const float* __restrict__ c1,
                                                                    const float* __restrict__ c2, float* __restrict__ dY,
                                                                    float* __restrict__ dYsum, int64_t lddysum) {
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
    float mu[4], rs[4], be[4], u[4], k1[4], k2[4], dmx[4], dmn[4], mx[4], ties[4], acc[4];
    Vec<4>::ld(mean + g * F + f, mu); Vec<4>::ld(rstd + g * F + f, rs); Vec<4>::ld(beta + f, be);
    Vec<4>::ld(c1 + g * F + f, k1); Vec<4>::ld(c2 + g * F + f, k2);
    Vec<4>::ld(U + r * ldu + f, u);
    Vec<4>::ld(dmax + r * lddmax + f, dmx); Vec<4>::ld(dmean + r * lddmean + f, dmn);
    Vec<4>::ld(mx_in + r * ldmx + f, mx); Vec<4>::ld(cnt_in + r * F + f, ties);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      ties[c] = cnt_ties(ties[c]);
      acc[c] = 0.f;
    }
    const int32_t* ip = idx + r * k;
    const float* vb = V + f;
    float* dy = dY + (r * k) * F + f;
    for (int m = 0; m < k; m += 4) {
      unsigned row[4];
      float y[4][4];
#pragma unroll
      for (int j = 0; j < 4; ++j) row[j] = row_offset24((unsigned)ip[(m + j < k) ? (m + j) : (k - 1)], (unsigned)ldv);
#pragma unroll
      for (int j = 0; j < 4; ++j) Vec<4>::ld(vb + row[j], y[j]);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (m + j < k) {
          float o[4];
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            float xh;
            const float z = bn_z(y[j][c] + u[c], mu[c], rs[c], be[c], relu, xh);
            // bn_common.h:bn_edge_dout spelled out: as an argument the division leaves the tie's arm (profiles/bn_common/isa_compare.txt)
            const float dz = bn_dz_row(z, ((z == mx[c]) ? dmx[c] / ties[c] : 0.f) + dmn[c] * invk, relu);
            o[c] = bn_dy(rs[c], dz, k1[c], xh, k2[c]);
            acc[c] += o[c];
          }
          Vec<4>::st(dy + (int64_t)(m + j) * F, o);
        }
    }
    if (dYsum) Vec<4>::st(dYsum + r * lddysum + f, acc);
  }
}

// workspace check + stage 2 of the two reduces
int seg_bwd_ws(const char* what, int rows, int nseg, int F, void* ws, size_t ws_bytes) {
  const size_t need = (size_t)dgcnn_seg_stats_workspace_bytes(rows, nseg, F);
  DG_REQUIRE(ws && ws_bytes >= need && (reinterpret_cast<uintptr_t>(ws) & 7) == 0, DGCNN_ENOSPC,
             "%s: workspace too small or not 8-byte aligned (%zu < %zu bytes)", what, ws_bytes, need);
  return DGCNN_OK;
}

}  // namespace

extern "C" int dgcnn_seg_bn_bwd_reduce_f32(const float* T, int64_t ldt, int rows, int F, const int32_t* seg_off, int nseg,
                                           const float* mean, const float* rstd, const float* beta, int relu, const float* dout,
                                           int64_t lddo, const float* d2, int64_t ldd2, double* red, void* ws, size_t ws_bytes,
                                           void* stream) {
  const char* what = "dgcnn_seg_bn_bwd_reduce_f32";
  DG_REQUIRE(T && seg_off && mean && rstd && beta && dout && red, DGCNN_EINVAL, "%s: null pointer", what);
  DG_REQUIRE(rows > 0 && F > 0 && nseg > 0 && nseg <= rows && ldt >= F && lddo >= F && (!d2 || ldd2 >= F), DGCNN_EINVAL,
             "%s: bad shape", what);
  DG_REQUIRE(relu == 0 || relu == 1, DGCNN_EINVAL, "%s: relu must be 0 or 1 (got %d)", what, relu);
  int rc = seg_bwd_ws(what, rows, nseg, F, ws, ws_bytes);
  if (rc) return rc;
  double* part = reinterpret_cast<double*>(ws);
  const unsigned chunks = (unsigned)dg::cdiv(rows, SEG_CHUNK);
  const bool vec = F % 4 == 0 && ldt % 4 == 0 && lddo % 4 == 0 && a16(T) && a16(dout) && a16(mean) && a16(rstd) && a16(beta) &&
                   (!d2 || (ldd2 % 4 == 0 && a16(d2)));
  if (vec) {
    const K1Terms<4> tm = {T, ldt, mean, rstd, beta, relu, dout, lddo, d2, ldd2};
    dg::launch((seg_bwd_partial_kernel<4, K1Terms<4>>), dim3(chunks, (unsigned)dg::cdiv(F, 256)), dim3(64 * SEG_WAVES), 0, ST, tm, rows, F,
               seg_off, nseg, part);
  } else {
    const K1Terms<1> tm = {T, ldt, mean, rstd, beta, relu, dout, lddo, d2, ldd2};
    dg::launch((seg_bwd_partial_kernel<1, K1Terms<1>>), dim3(chunks, (unsigned)dg::cdiv(F, 64)), dim3(64 * SEG_WAVES), 0, ST, tm, rows, F,
               seg_off, nseg, part);
  }
  return seg_stats_final(what, part, seg_off, nseg, F, red, ST);
}

extern "C" int dgcnn_seg_edge_bn_bwd_reduce_points_f32(const float* mx, int64_t ldmx, const float* mn, int64_t ldmn, const float* cntpos,
                                                       const float* dmax, int64_t lddmax, const float* dmean, int64_t lddmean,
                                                       const float* beta, int rows, int k, int F, const int32_t* seg_off, int nseg,
                                                       double* red, void* ws, size_t ws_bytes, void* stream) {
  const char* what = "dgcnn_seg_edge_bn_bwd_reduce_points_f32";
  DG_REQUIRE(mx && mn && cntpos && dmax && dmean && beta && seg_off && red, DGCNN_EINVAL, "%s: null pointer", what);
  DG_REQUIRE(rows > 0 && k > 0 && F > 0 && nseg > 0 && nseg <= rows, DGCNN_EINVAL, "%s: bad shape", what);
  DG_REQUIRE(F % 4 == 0 && k < CNT_POS, DGCNN_EUNSUP, "%s: F must be a multiple of 4 (got %d) and k < %d (got %d)", what, F, CNT_POS, k);
  DG_REQUIRE(a16(mx) && a16(mn) && a16(cntpos) && a16(dmax) && a16(dmean) && a16(beta) && ldmx % 4 == 0 && ldmn % 4 == 0 &&
                 lddmax % 4 == 0 && lddmean % 4 == 0 && ldmx >= F && ldmn >= F && lddmax >= F && lddmean >= F, DGCNN_EINVAL,
             "%s: operands must be 16-byte aligned with leading dimensions %% 4 == 0", what);
  int rc = seg_bwd_ws(what, rows, nseg, F, ws, ws_bytes);
  if (rc) return rc;
  double* part = reinterpret_cast<double*>(ws);
  const unsigned chunks = (unsigned)dg::cdiv(rows, SEG_CHUNK);
  PointTerms tm = {mx, ldmx, mn, ldmn, cntpos, dmax, lddmax, dmean, lddmean, beta, k, F};
  dg::launch((seg_bwd_partial_kernel<4, PointTerms>), dim3(chunks, (unsigned)dg::cdiv(F, 256)), dim3(64 * SEG_WAVES), 0, ST, tm, rows, F,
             seg_off, nseg, part);
  return seg_stats_final(what, part, seg_off, nseg, F, red, ST);
}

extern "C" int dgcnn_seg_bn_bwd_finalize_f32(const double* red, int nseg, int F, const int32_t* seg_off, int k, float* c1, float* c2,
                                             float* dbeta, float dbeta_beta, void* stream) {
  DG_REQUIRE(red && seg_off && c1 && c2 && nseg > 0 && F > 0 && k > 0, DGCNN_EINVAL, "dgcnn_seg_bn_bwd_finalize_f32: bad args");
  dg::launch(seg_bn_bwd_finalize_kernel, dim3(grid1d((int64_t)nseg * F)), dim3(256), 0, ST, red, nseg, F, seg_off, k, c1, c2, dbeta,
             dbeta_beta);
  return dg::check_launch("dgcnn_seg_bn_bwd_finalize_f32");
}

extern "C" int dgcnn_seg_bn_bwd_apply_f32(const float* T, int64_t ldt, int rows, int F, const int32_t* row_group, const float* mean,
                                          const float* rstd, const float* beta, int relu, const float* dout, int64_t lddo,
                                          const float* d2, int64_t ldd2, const float* c1, const float* c2, float* dT, int64_t lddt,
                                          void* stream) {
  const char* what = "dgcnn_seg_bn_bwd_apply_f32";
  DG_REQUIRE(T && row_group && mean && rstd && beta && dout && c1 && c2 && dT, DGCNN_EINVAL, "%s: null pointer", what);
  DG_REQUIRE(rows > 0 && F > 0 && ldt >= F && lddo >= F && lddt >= F && (!d2 || ldd2 >= F), DGCNN_EINVAL, "%s: bad shape", what);
  DG_REQUIRE(relu == 0 || relu == 1, DGCNN_EINVAL, "%s: relu must be 0 or 1 (got %d)", what, relu);
  const bool vec = F % 4 == 0 && ldt % 4 == 0 && lddo % 4 == 0 && lddt % 4 == 0 && a16(T) && a16(dout) && a16(dT) && a16(mean) &&
                   a16(rstd) && a16(beta) && a16(c1) && a16(c2) && (!d2 || (ldd2 % 4 == 0 && a16(d2)));
  if (vec)
    dg::launch(seg_bn_bwd_apply_kernel<4>, dim3(grid_items((int64_t)rows * (F / 4))), dim3(256), 0, ST, T, ldt, (int64_t)rows, F, row_group,
               mean, rstd, beta, relu, dout, lddo, d2, ldd2, c1, c2, dT, lddt);
  else
    dg::launch(seg_bn_bwd_apply_kernel<1>, dim3(grid_items((int64_t)rows * F)), dim3(256), 0, ST, T, ldt, (int64_t)rows, F, row_group, mean,
               rstd, beta, relu, dout, lddo, d2, ldd2, c1, c2, dT, lddt);
  return dg::check_launch(what);
}

extern "C" int dgcnn_seg_edge_bn_bwd_apply_f32(const float* V, int64_t ldv, const float* U, int64_t ldu, const int32_t* idx, int rows, int k,
                                               int F, const int32_t* row_group, const float* mean, const float* rstd, const float* beta,
                                               int relu, const float* dmax, int64_t lddmax, const float* dmean, int64_t lddmean,
                                               const float* mx_in, int64_t ldmx, const float* cnt_in, const float* c1, const float* c2,
                                               float* dY, float* dYsum, int64_t lddysum, void* stream) {
  const char* what = "dgcnn_seg_edge_bn_bwd_apply_f32";
  int rc = check_seg_edge(what, V, ldv, U, ldu, idx, rows, k, F);
  if (rc) return rc;
  DG_REQUIRE(row_group && mean && rstd && beta && dmax && dmean && mx_in && cnt_in && c1 && c2 && dY, DGCNN_EINVAL, "%s: null pointer",
             what);
  DG_REQUIRE(relu == 0 || relu == 1, DGCNN_EINVAL, "%s: relu must be 0 or 1 (got %d)", what, relu);
  DG_REQUIRE(k < CNT_POS, DGCNN_EUNSUP, "%s: k must be < %d (the packed tie / positive counts)", what, CNT_POS);
  DG_REQUIRE(a16(mean) && a16(rstd) && a16(beta) && a16(c1) && a16(c2) && a16(dmax) && a16(dmean) && a16(mx_in) && a16(cnt_in) && a16(dY) &&
                 lddmax >= F && lddmax % 4 == 0 && lddmean >= F && lddmean % 4 == 0 && ldmx >= F && ldmx % 4 == 0 &&
                 (!dYsum || (a16(dYsum) && lddysum >= F && lddysum % 4 == 0)),
             DGCNN_EINVAL, "%s: operands and tables must be 16-byte aligned with leading dimensions %% 4 == 0", what);
  const unsigned grid = (grid_items((int64_t)rows * (F / 4)) + 7u) & ~7u;     // (the XCD item map needs a multiple of 8)
  dg::launch(seg_edge_bn_bwd_apply_kernel, dim3(grid), dim3(256), 0, ST, V, ldv, U, ldu, idx, (int64_t)rows, k, F, row_group, mean, rstd, beta,
             relu, dmax, lddmax, dmean, lddmean, mx_in, ldmx, cnt_in, c1, c2, dY, dYsum, lddysum);
  return dg::check_launch(what);
}

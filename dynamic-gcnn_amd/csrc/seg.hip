// seg.hip -- the head of a PACKED tower: clouds of different sizes concatenated row-wise, cloud b = rows
// [seg_off[b], seg_off[b + 1]).  The per-cloud passes of model.py:76-85 (max-pool over the points of a cloud, tf.tile and
// its transpose) for such a tower.  All four are streaming kernels over a row-major (rows, F) tensor; their grids are shaped
// over fixed-size ROW CHUNKS of the tower, never over clouds: one 8192-point cloud next to twenty 300-point clouds loads the
// chip as evenly as a dense tower does.  A chunk is cut at the cloud boundaries inside it; every piece is reduced by the
// workgroup (registers per wave, then LDS across the waves) before ONE result per (piece, column) leaves it.
#include "gemm_common.h"
#include "bn_common.h"   // Vec

namespace {

constexpr int SEG_CHUNK = 64;   // rows of the tower per workgroup
constexpr int SEG_WAVES = 4;    // waves per workgroup; wave w owns rows w, w + 4, ... of a piece (ascending: first arg-max / fixed order)
constexpr int SEG_UNROLL = 4;   // independent row loads in flight per lane

// Per-cloud column maximum as keys (gemm_common.h: f32_ordered(value) << 32 | ~row-in-cloud): grid = (row chunks, column blocks of
// 64 * VW), lane = VW adjacent columns (one float4 per row when VW = 4: a wave reads 1 KiB of a row per load).
template <int VW>
__global__ __launch_bounds__(64 * SEG_WAVES) void colmax_seg_kernel(const float* __restrict__ x, int64_t ldx, int rows, int F,
                                                                    const int32_t* __restrict__ seg_off, int nseg,
                                                                    unsigned long long* __restrict__ keys) {
  __shared__ float sv[SEG_WAVES][64 * VW];
  __shared__ int si[SEG_WAVES][64 * VW];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c0 = (blockIdx.y * 64 + lane) * VW;
  const bool col_ok = c0 < F;                                 // (VW = 4: F % 4 == 0, a quad is inside or outside as a whole)
  const int r0 = blockIdx.x * SEG_CHUNK;
  const int r1 = imin(r0 + SEG_CHUNK, rows);
  int b = cloud_of_row(seg_off, nseg, r0);
  int ps = r0;
  while (ps < r1 && b < nseg) {
    const int cb = seg_off[b];
    const int pe = imin(seg_off[b + 1], r1);
    float best[VW];
    int bi[VW];
#pragma unroll
    for (int q = 0; q < VW; ++q) { best[q] = -INFINITY; bi[q] = 0x7fffffff; }
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
          for (int q = 0; q < VW; ++q)
            if (v[u][q] > best[q] || (v[u][q] == best[q] && bi[q] == 0x7fffffff)) { best[q] = v[u][q]; bi[q] = i + u * SEG_WAVES; }
      }
      for (; i < pe; i += SEG_WAVES) {
        float v[VW];
        Vec<VW>::ld(p + (int64_t)i * ldx, v);
#pragma unroll
        for (int q = 0; q < VW; ++q)
          if (v[q] > best[q] || (v[q] == best[q] && bi[q] == 0x7fffffff)) { best[q] = v[q]; bi[q] = i; }
      }
    }
#pragma unroll
    for (int q = 0; q < VW; ++q) { sv[w][lane * VW + q] = best[q]; si[w][lane * VW + q] = bi[q]; }
    __syncthreads();
    // across the waves: wave q takes the 64 columns [q * 64, q * 64 + 64) of the block's 64 * VW -- one lane per column, so a wave's
    // atomics fall on 512 contiguous bytes of the key row
    for (int q = w; q < VW; q += SEG_WAVES) {
      const int cl = q * 64 + lane;
      const int col = blockIdx.y * 64 * VW + cl;
      float mx = sv[0][cl];
      int mr = si[0][cl];
      for (int ww = 1; ww < SEG_WAVES; ++ww) {
        const float v = sv[ww][cl];
        const int r = si[ww][cl];
        if (v > mx || (v == mx && r < mr)) { mx = v; mr = r; }
      }
      // (a piece whose values all compared false -- NaN -- sends nothing: an all-NaN column keeps its zero key, which the decode
      // reports as (NaN, row 0))
      if (col < F && mr != 0x7fffffff) {
        const unsigned long long key = ((unsigned long long)f32_ordered(mx) << 32) |
                                       (unsigned long long)(0xffffffffu - (unsigned)(mr - cb));
        atomicMax(keys + (int64_t)b * F + col, key);
      }
    }
    __syncthreads();
    ps = pe;
    ++b;
  }
}

// dx[seg_off[b] + arg[b][f]][f] += dout[b][f]: one writer per (cloud, column)
__global__ void global_max_bwd_seg_kernel(const float* __restrict__ dout, const int32_t* __restrict__ arg,
                                          const int32_t* __restrict__ seg_off, int F, int64_t total, float* __restrict__ dx,
                                          int64_t lddx) {
  GRID_STRIDE(i, total) {
    const int b = (int)(i / F);
    const int f = (int)(i % F);
    const int64_t row = (int64_t)seg_off[b] + arg[i];
    if (row < seg_off[b + 1]) dx[row * lddx + f] += dout[i];
  }
}

// Per-cloud column sums, stage 1: the chunk's piece of cloud b, summed in a fixed order (every wave its rows ascending, then the
// waves 0..3), goes to partial slot (chunk + b).  Slots grow strictly with (chunk, b) -- the first cloud of chunk c + 1 is the last
// cloud of chunk c or a later one -- so the pieces of cloud b are the slots (c + b) of the chunks c it touches: a contiguous run.
template <int VW>
__global__ __launch_bounds__(64 * SEG_WAVES) void seg_colsum_partial_kernel(const float* __restrict__ x, int64_t ldx, int rows, int F,
                                                                            const int32_t* __restrict__ seg_off, int nseg,
                                                                            float* __restrict__ part) {
  __shared__ float sv[SEG_WAVES][64 * VW];
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
    float s[VW];
#pragma unroll
    for (int q = 0; q < VW; ++q) s[q] = 0.f;
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
          for (int q = 0; q < VW; ++q) s[q] += v[u][q];
      }
      for (; i < pe; i += SEG_WAVES) {
        float v[VW];
        Vec<VW>::ld(p + (int64_t)i * ldx, v);
#pragma unroll
        for (int q = 0; q < VW; ++q) s[q] += v[q];
      }
    }
#pragma unroll
    for (int q = 0; q < VW; ++q) sv[w][lane * VW + q] = s[q];
    __syncthreads();
    for (int q = w; q < VW; q += SEG_WAVES) {                // wave q: columns [q * 64, q * 64 + 64) of the block, coalesced stores
      const int cl = q * 64 + lane;
      const int col = blockIdx.y * 64 * VW + cl;
      float t = 0.f;
      for (int ww = 0; ww < SEG_WAVES; ++ww) t += sv[ww][cl];
      if (col < F) part[(int64_t)(chunk + b) * F + col] = t;
    }
    __syncthreads();
    ps = pe;
    ++b;
  }
}

// stage 2: out[b][f] = the partial slots of cloud b, first chunk to last
__global__ void seg_colsum_final_kernel(const float* __restrict__ part, const int32_t* __restrict__ seg_off, int F, int64_t total,
                                        float* __restrict__ out) {
  GRID_STRIDE(i, total) {
    const int b = (int)(i / F);
    const int f = (int)(i % F);
    const int cfirst = seg_off[b] / SEG_CHUNK, clast = (seg_off[b + 1] - 1) / SEG_CHUNK;
    float t = 0.f;
    for (int c = cfirst; c <= clast; ++c) t += part[(int64_t)(c + b) * F + f];
    out[i] = t;
  }
}

__global__ void tile_rows_seg_kernel(const float* __restrict__ src, int64_t lds, const int32_t* __restrict__ row_group,
                                     float* __restrict__ dst, int64_t ldd, int64_t R, int F) {
  GRID_STRIDE(i, R * F) {
    const int64_t r = i / F;
    const int f = (int)(i % F);
    dst[r * ldd + f] = src[(int64_t)row_group[r] * lds + f];
  }
}

inline bool vec4_ok(const float* x, int64_t ldx, int F) {
  return F % 4 == 0 && ldx % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int dgcnn_colmax_seg_f32(const float* x, int64_t ldx, int rows, int F, const int32_t* seg_off, int nseg, void* keys,
                                    void* stream) {
  DG_REQUIRE(x && seg_off && keys && rows > 0 && F > 0 && nseg > 0 && nseg <= rows && ldx >= F, DGCNN_EINVAL,
             "dgcnn_colmax_seg_f32: bad args");
  const unsigned chunks = (unsigned)dg::cdiv(rows, SEG_CHUNK);
  unsigned long long* k = reinterpret_cast<unsigned long long*>(keys);
  if (vec4_ok(x, ldx, F))
    dg::launch(colmax_seg_kernel<4>, dim3(chunks, (unsigned)dg::cdiv(F, 256)), dim3(64 * SEG_WAVES), 0, ST, x, ldx, rows, F, seg_off,
               nseg, k);
  else
    dg::launch(colmax_seg_kernel<1>, dim3(chunks, (unsigned)dg::cdiv(F, 64)), dim3(64 * SEG_WAVES), 0, ST, x, ldx, rows, F, seg_off,
               nseg, k);
  return dg::check_launch("dgcnn_colmax_seg_f32");
}

extern "C" int dgcnn_global_max_bwd_seg_f32(const float* dout, const int32_t* arg, const int32_t* seg_off, int nseg, int F,
                                            float* dx, int64_t lddx, void* stream) {
  DG_REQUIRE(dout && arg && seg_off && dx && nseg > 0 && F > 0 && lddx >= F, DGCNN_EINVAL, "dgcnn_global_max_bwd_seg_f32: bad args");
  const int64_t total = (int64_t)nseg * F;
  dg::launch(global_max_bwd_seg_kernel, dim3(grid1d(total)), dim3(256), 0, ST, dout, arg, seg_off, F, total, dx, lddx);
  return dg::check_launch("dgcnn_global_max_bwd_seg_f32");
}

extern "C" int64_t dgcnn_seg_colsum_workspace_bytes(int rows, int nseg, int F) {
  if (rows <= 0 || nseg <= 0 || F <= 0) return 0;
  return (dg::cdiv(rows, SEG_CHUNK) + nseg) * (int64_t)F * (int64_t)sizeof(float);
}

extern "C" int dgcnn_seg_colsum_f32(const float* x, int64_t ldx, int rows, int F, const int32_t* seg_off, int nseg, float* out,
                                    void* ws, size_t ws_bytes, void* stream) {
  DG_REQUIRE(x && seg_off && out && rows > 0 && F > 0 && nseg > 0 && nseg <= rows && ldx >= F, DGCNN_EINVAL,
             "dgcnn_seg_colsum_f32: bad args");
  const size_t need = (size_t)dgcnn_seg_colsum_workspace_bytes(rows, nseg, F);
  DG_REQUIRE(ws && ws_bytes >= need && (reinterpret_cast<uintptr_t>(ws) & 3) == 0, DGCNN_ENOSPC,
             "dgcnn_seg_colsum_f32: workspace too small (%zu < %zu bytes)", ws_bytes, need);
  float* part = reinterpret_cast<float*>(ws);
  const unsigned chunks = (unsigned)dg::cdiv(rows, SEG_CHUNK);
  if (vec4_ok(x, ldx, F))
    dg::launch(seg_colsum_partial_kernel<4>, dim3(chunks, (unsigned)dg::cdiv(F, 256)), dim3(64 * SEG_WAVES), 0, ST, x, ldx, rows, F,
               seg_off, nseg, part);
  else
    dg::launch(seg_colsum_partial_kernel<1>, dim3(chunks, (unsigned)dg::cdiv(F, 64)), dim3(64 * SEG_WAVES), 0, ST, x, ldx, rows, F,
               seg_off, nseg, part);
  int rc = dg::check_launch("dgcnn_seg_colsum_f32");
  if (rc) return rc;
  const int64_t total = (int64_t)nseg * F;
  dg::launch(seg_colsum_final_kernel, dim3(grid1d(total)), dim3(256), 0, ST, (const float*)part, seg_off, F, total, out);
  return dg::check_launch("dgcnn_seg_colsum_f32");
}

extern "C" int dgcnn_tile_rows_seg_f32(const float* src, int64_t lds, const int32_t* row_group, int rows, int F, float* dst,
                                       int64_t ldd, void* stream) {
  DG_REQUIRE(src && row_group && dst && rows > 0 && F > 0 && lds >= F && ldd >= F, DGCNN_EINVAL, "dgcnn_tile_rows_seg_f32: bad args");
  dg::launch(tile_rows_seg_kernel, dim3(grid1d((int64_t)rows * F)), dim3(256), 0, ST, src, lds, row_group, dst, ldd, (int64_t)rows, F);
  return dg::check_launch("dgcnn_tile_rows_seg_f32");
}

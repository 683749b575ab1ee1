// fps.hip -- K7: farthest point sampling, and the row take with its backward: the downsampling half of a hierarchical point network
// (PointNet++ set abstraction; the producer of the second point set of knn_cross.hip and interp.hip).
// FPS is a chain of m dependent steps -- lower every row's distance to the selected set, then take the arg-max -- so its cost is the
// latency of one step.  ONE workgroup of 1024 threads owns a cloud for the whole chain (no workgroup ever waits for another one: the
// idle CUs are the stated cost), in one of two forms chosen per cloud from its own size:
//   resident   C <= 4, n <= 16384: every thread keeps its rows' coordinates and `mind` in registers (row i = p * 1024 + t lives in
//              slot p of thread t).  A step is the per-thread update with a local arg-max, a 16-lane reduction by DPP, the 64 row
//              winners (key and coordinates) through a double-buffered LDS slot, ONE barrier, and the same reduction of the 64
//              winners done redundantly by every 16 lanes -- nobody broadcasts the winner, everybody works it out.
//   streaming  everything else: the coordinates are re-read every step (they stay in L2), `mind` lives in the caller's workspace,
//              the winner's coordinates are read back through its row index.
// The arg-max runs on one 64-bit integer key: mind is never -0.0 or NaN, so the non-negative floats and +inf order as their bit
// patterns; key = ((bits + 1) << 32) | ~row for a live row and (0 << 32) | ~row for a selected one -- the largest key is the largest
// mind, ties to the LOWER row.  The arithmetic is normative (include/dgcnn_hip.h, K7; the build uses -ffp-contract=off).
#include "common.h"
#include <math.h>

namespace {

constexpr int FT = 1024;                 // threads of an FPS workgroup: 16 waves, the whole of a CU's wave slots at 128 registers each
constexpr int RES_P = 16;                // rows a thread of the resident form keeps at most
constexpr int RES_MAX_C = 4;
constexpr int RES_MAX_N = FT * RES_P;
constexpr int GT = 256;                  // threads of the gather / scatter blocks

typedef unsigned long long key_t;

template <int CTRL>
__device__ __forceinline__ key_t dpp_key(key_t k) {
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)k, CTRL, 0xf, 0xf, true);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(k >> 32), CTRL, 0xf, 0xf, true);
  return ((key_t)hi << 32) | lo;
}
template <int CTRL>
__device__ __forceinline__ key_t max_with(key_t k) {
  const key_t o = dpp_key<CTRL>(k);
  return o > k ? o : k;
}
// the largest key of the lane's row of 16, in every lane of it: quad_perm [1,0,3,2] and [2,3,0,1], row_half_mirror, row_mirror
__device__ __forceinline__ key_t row_max(key_t k) {
  k = max_with<0xB1>(k);
  k = max_with<0x4E>(k);
  k = max_with<0x141>(k);
  return max_with<0x140>(k);
}
// the largest of the 64 row winners: lane l takes four of them, the row of 16 reduces -- every lane of the block ends with it
__device__ __forceinline__ key_t block_max(const key_t* keys, int t) {
  const ulonglong2* q = reinterpret_cast<const ulonglong2*>(keys + 4 * (t & 15));
  const ulonglong2 a = q[0], b = q[1];
  const key_t k0 = a.x > a.y ? a.x : a.y, k1 = b.x > b.y ? b.x : b.y;
  return row_max(k0 > k1 ? k0 : k1);
}
__device__ __forceinline__ key_t make_key(float m, int i) {
  const unsigned hi = (m < 0.f) ? 0u : __float_as_uint(m) + 1u;
  return ((key_t)hi << 32) | (unsigned)~i;
}
__device__ __forceinline__ int key_row(key_t k) { return (int)~(unsigned)k; }
__device__ __forceinline__ float key_mind(key_t k) {
  const unsigned hi = (unsigned)(k >> 32);
  return hi ? __uint_as_float(hi - 1u) : -1.0f;
}
__device__ __forceinline__ bool finite(float v) { return fabsf(v) < INFINITY; }

struct Cloud {
  int x0, n, o0, m;
};
__device__ __forceinline__ Cloud cloud_of_block(const int32_t* __restrict__ x_off, const int32_t* __restrict__ s_off, int max_n,
                                                int max_m) {
  const int b = blockIdx.x;
  Cloud c;
  if (x_off) {
    c.x0 = x_off[b]; c.n = x_off[b + 1] - c.x0;
    c.o0 = s_off[b]; c.m = s_off[b + 1] - c.o0;
  } else {
    c.x0 = b * max_n; c.n = max_n;
    c.o0 = b * max_m; c.m = max_m;
  }
  return c;
}
// a cloud asked for more samples than it has rows (the Python layer refuses it): the entries past the n-th hold -1
__device__ __forceinline__ void fill_rest(const Cloud& c, int from, int32_t* __restrict__ idx, float* __restrict__ dist) {
  for (int j = from + (int)threadIdx.x; j < c.m; j += FT) {
    idx[c.o0 + j] = -1;
    if (dist) dist[c.o0 + j] = -1.0f;
  }
}

template <int C, int P>
__global__ __launch_bounds__(FT) void fps_resident_kernel(const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ x_off,
                                                          const int32_t* __restrict__ s_off, int max_n, int max_m,
                                                          const int32_t* __restrict__ start, int32_t* __restrict__ idx,
                                                          float* __restrict__ dist) {
  __shared__ __attribute__((aligned(16))) key_t s_key[2][64];
  __shared__ float s_xs[2][64][C];
  const int t = threadIdx.x;
  const Cloud cl = cloud_of_block(x_off, s_off, max_n, max_m);
  const int n = cl.n;
  if (n < 1 || cl.m < 1 || n > RES_MAX_N) return;             // n > RES_MAX_N: the streaming launch owns this cloud
  if (n > P * FT) {                                           // a cloud above the max_n the caller stated: nothing is read
    fill_rest(cl, 0, idx, dist);
    return;
  }
  const float* xc = x + (int64_t)cl.x0 * ldx;
  float px[P][C], mind[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int i = p * FT + t;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      px[p][c] = (i < n) ? xc[(int64_t)i * ldx + c] : 0.f;
      ok = ok && finite(px[p][c]);
    }
    mind[p] = (i < n) ? (ok ? INFINITY : 0.0f) : -1.0f;      // a slot without a row is a selected row: it never wins
  }
  int s = start ? start[blockIdx.x] : 0;
  if ((unsigned)s >= (unsigned)n) s = 0;
  float cur[C];
  bool ok = true;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    cur[c] = xc[(int64_t)s * ldx + c];
    ok = ok && finite(cur[c]);
  }
  float curd = ok ? INFINITY : 0.0f;
  const int add = x_off ? cl.x0 : 0;
  const int steps = cl.m < n ? cl.m : n;
  int buf = 0;
  for (int j = 0;; ++j) {
    if (t == 0) {
      idx[cl.o0 + j] = s + add;
      if (dist) dist[cl.o0 + j] = curd;
    }
    if (j == steps - 1) break;
    float bm = -1.0f, bx[C];
    int bi = t;
#pragma unroll
    for (int c = 0; c < C; ++c) bx[c] = 0.f;
#pragma unroll
    for (int p = 0; p < P; ++p) {
      if (p * FT < n) {                                        // block-uniform
        const int i = p * FT + t;
        float d = px[p][0] - cur[0];
        float D = d * d;
#pragma unroll
        for (int c = 1; c < C; ++c) {
          d = px[p][c] - cur[c];
          D = D + d * d;
        }
        float m = mind[p];
        m = (D < m) ? D : m;
        m = (i == s) ? -1.0f : m;
        mind[p] = m;
        if (m > bm) {                                          // ascending rows, strict: ties stay with the lower row
          bm = m;
          bi = i;
#pragma unroll
          for (int c = 0; c < C; ++c) bx[c] = px[p][c];
        }
      }
    }
    const key_t key = make_key(bm, bi);
    if (row_max(key) == key) {                                 // one lane of every 16: the keys are distinct
      s_key[buf][t >> 4] = key;
#pragma unroll
      for (int c = 0; c < C; ++c) s_xs[buf][t >> 4][c] = bx[c];
    }
    __syncthreads();                                           // the only barrier of a step: the next step writes the other buffer
    const key_t w = block_max(s_key[buf], t);
    s = key_row(w);
    curd = key_mind(w);
    const int slot = (s & (FT - 1)) >> 4;                      // row s lives in thread s % 1024, whose 16 lanes wrote slot (s % 1024) / 16
#pragma unroll
    for (int c = 0; c < C; ++c) cur[c] = s_xs[buf][slot][c];
    buf ^= 1;
  }
  fill_rest(cl, steps, idx, dist);
}

// CT > 0: the channel count at compile time (the winner's coordinates in registers); CT == 0: C at run time
template <int CT>
__global__ __launch_bounds__(FT) void fps_stream_kernel(const float* __restrict__ x, int64_t ldx, int C_rt,
                                                        const int32_t* __restrict__ x_off, const int32_t* __restrict__ s_off, int max_n,
                                                        int max_m, int res_max, const int32_t* __restrict__ start,
                                                        int32_t* __restrict__ idx, float* __restrict__ dist, float* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) key_t s_key[2][64];
  const int C = CT ? CT : C_rt;
  const int t = threadIdx.x;
  const Cloud cl = cloud_of_block(x_off, s_off, max_n, max_m);
  const int n = cl.n;
  if (n < 1 || cl.m < 1 || n <= res_max) return;              // n <= res_max: the resident launch owns this cloud
  const float* xc = x + (int64_t)cl.x0 * ldx;
  float* mind = ws + cl.x0;                                    // row i is read and written by thread i % 1024 alone: no barrier for it
  for (int i = t; i < n; i += FT) {
    const float* xi = xc + (int64_t)i * ldx;
    bool ok = true;
    for (int c = 0; c < C; ++c) ok = ok && finite(xi[c]);
    mind[i] = ok ? INFINITY : 0.0f;
  }
  int s = start ? start[blockIdx.x] : 0;
  if ((unsigned)s >= (unsigned)n) s = 0;
  float curd;
  {
    const float* xs = xc + (int64_t)s * ldx;
    bool ok = true;
    for (int c = 0; c < C; ++c) ok = ok && finite(xs[c]);
    curd = ok ? INFINITY : 0.0f;
  }
  const int add = x_off ? cl.x0 : 0;
  const int steps = cl.m < n ? cl.m : n;
  int buf = 0;
  for (int j = 0;; ++j) {
    if (t == 0) {
      idx[cl.o0 + j] = s + add;
      if (dist) dist[cl.o0 + j] = curd;
    }
    if (j == steps - 1) break;
    const float* xs = xc + (int64_t)s * ldx;                   // one address for the whole block
    float cur[CT ? CT : 1];
    if (CT) {
#pragma unroll
      for (int c = 0; c < CT; ++c) cur[c] = xs[c];
    }
    float bm = -1.0f;
    int bi = t;
    for (int i = t; i < n; i += FT) {
      const float* xi = xc + (int64_t)i * ldx;
      float d = xi[0] - (CT ? cur[0] : xs[0]);
      float D = d * d;
      if (CT) {
#pragma unroll
        for (int c = 1; c < CT; ++c) {
          d = xi[c] - cur[c];
          D = D + d * d;
        }
      } else {
        for (int c = 1; c < C; ++c) {
          d = xi[c] - xs[c];
          D = D + d * d;
        }
      }
      float m = mind[i];
      m = (D < m) ? D : m;
      m = (i == s) ? -1.0f : m;
      mind[i] = m;
      if (m > bm) {
        bm = m;
        bi = i;
      }
    }
    const key_t key = make_key(bm, bi);
    if (row_max(key) == key) s_key[buf][t >> 4] = key;
    __syncthreads();
    const key_t w = block_max(s_key[buf], t);
    s = __builtin_amdgcn_readfirstlane(key_row(w));
    curd = key_mind(w);
    buf ^= 1;
  }
  fill_rest(cl, steps, idx, dist);
}

// ---- the row take and its backward.  row(s) = (s / M) * N + idx[s] for a dense tower (M > 0), idx[s] for tower rows (M == N == 0).
__device__ __forceinline__ int64_t taken_row(const int32_t* __restrict__ idx, int64_t s, int M, int N) {
  const int64_t j = idx[s];
  return M ? (s / M) * N + j : j;
}

template <bool VEC>
__global__ __launch_bounds__(GT) void rows_gather_kernel(const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ idx,
                                                         int64_t s_rows, int M, int N, int FV, float* __restrict__ y, int64_t ldy) {
  GRID_STRIDE(it, s_rows * FV) {
    const int64_t s = it / FV;
    const int f = (int)(it - s * FV);
    const int64_t r = taken_row(idx, s, M, N);
    if (VEC) *reinterpret_cast<float4*>(y + s * ldy + 4 * f) = ld4(x + r * ldx + 4 * f);
    else y[s * ldy + f] = x[r * ldx + f];
  }
}

template <bool VEC>
__global__ __launch_bounds__(GT) void rows_zero_kernel(float* __restrict__ dx, int64_t lddx, int64_t x_rows, int FV) {
  GRID_STRIDE(it, x_rows * FV) {
    const int64_t r = it / FV;
    const int f = (int)(it - r * FV);
    if (VEC) *reinterpret_cast<float4*>(dx + r * lddx + 4 * f) = make_float4(0.f, 0.f, 0.f, 0.f);
    else dx[r * lddx + f] = 0.f;
  }
}

// the rows of idx are distinct (FPS guarantees it): every dx row has at most one writer -- no atomics, one result run to run
template <bool VEC>
__global__ __launch_bounds__(GT) void rows_scatter_kernel(const float* __restrict__ dy, int64_t lddy, const int32_t* __restrict__ idx,
                                                          int64_t s_rows, int M, int N, int FV, float* __restrict__ dx, int64_t lddx,
                                                          int beta) {
  GRID_STRIDE(it, s_rows * FV) {
    const int64_t s = it / FV;
    const int f = (int)(it - s * FV);
    const int64_t r = taken_row(idx, s, M, N);
    if (VEC) {
      float4 g = ld4(dy + s * lddy + 4 * f);
      float* o = dx + r * lddx + 4 * f;
      if (beta) {
        const float4 d = ld4(o);
        g.x = d.x + g.x; g.y = d.y + g.y; g.z = d.z + g.z; g.w = d.w + g.w;
      }
      *reinterpret_cast<float4*>(o) = g;
    } else {
      const float g = dy[s * lddy + f];
      float* o = dx + r * lddx + f;
      *o = beta ? *o + g : g;
    }
  }
}

inline int64_t pad256(int64_t n) { return (n + 255) / 256 * 256; }
inline bool a16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool vec_ok(int F, int64_t lda, int64_t ldb, const void* a, const void* b) {
  return F % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0 && a16(a) && a16(b);
}

// what the take and its backward ask of their shapes (check_graph of interp.hip, without k and the limits on F)
int check_rows(const char* who, int s_rows, int x_rows, int M, int N, int F) {
  DG_REQUIRE(F > 0, DGCNN_EINVAL, "%s: F=%d must be positive", who, F);
  DG_REQUIRE(s_rows > 0 && x_rows > 0, DGCNN_EINVAL, "%s: s_rows=%d and x_rows=%d must be positive", who, s_rows, x_rows);
  DG_REQUIRE(M >= 0 && N >= 0, DGCNN_EINVAL, "%s: M=%d and N=%d must not be negative", who, M, N);
  if (M > 0) {
    DG_REQUIRE(N > 0 && s_rows % M == 0 && (int64_t)x_rows == (int64_t)(s_rows / M) * N, DGCNN_EINVAL,
               "%s: dense towers need s_rows = B * M and x_rows = B * N (s_rows=%d, x_rows=%d, M=%d, N=%d)", who, s_rows, x_rows, M, N);
  } else {
    DG_REQUIRE(N == 0, DGCNN_EINVAL, "%s: M = 0 (idx holds tower rows) needs N = 0, got N=%d", who, N);
  }
  return DGCNN_OK;
}

typedef void (*resident_fn)(const float*, int64_t, const int32_t*, const int32_t*, int, int, const int32_t*, int32_t*, float*);
template <int C>
resident_fn resident_for(int n) {
  return n <= 1 * FT ? fps_resident_kernel<C, 1> : n <= 2 * FT ? fps_resident_kernel<C, 2> : n <= 4 * FT ? fps_resident_kernel<C, 4>
       : n <= 8 * FT ? fps_resident_kernel<C, 8> : fps_resident_kernel<C, 16>;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int dgcnn_fps_resident_max_n(int C) { return (C >= 1 && C <= RES_MAX_C) ? RES_MAX_N : 0; }

extern "C" int64_t dgcnn_fps_workspace_bytes(int rows, int C, int max_n) {
  if (rows <= 0 || C < 1 || C > 64 || max_n < 1 || max_n > rows) return 0;
  return max_n > dgcnn_fps_resident_max_n(C) ? pad256(4 * (int64_t)rows) : 0;
}

extern "C" int dgcnn_fps_f32(const float* x, int64_t ldx, int C, int nseg, const int32_t* x_off, const int32_t* s_off, int rows,
                             int samples, int max_n, int max_m, const int32_t* start, int32_t* idx, float* dist, void* ws,
                             size_t ws_bytes, void* stream) {
  static const char* who = "dgcnn_fps_f32";
  DG_REQUIRE(x && idx, DGCNN_EINVAL, "%s: null x or idx", who);
  DG_REQUIRE((x_off == nullptr) == (s_off == nullptr), DGCNN_EINVAL, "%s: x_off and s_off are both given (packed) or both null (dense)",
             who);
  DG_REQUIRE(C >= 1, DGCNN_EINVAL, "%s: C=%d must be at least 1", who, C);
  DG_REQUIRE(C <= 64, DGCNN_EUNSUP, "%s: C=%d > 64 channels", who, C);
  DG_REQUIRE(nseg >= 1, DGCNN_EINVAL, "%s: nseg=%d must be at least 1", who, nseg);
  DG_REQUIRE(nseg <= 65535, DGCNN_EUNSUP, "%s: nseg=%d > 65535 clouds", who, nseg);
  DG_REQUIRE(rows > 0 && samples > 0 && max_n > 0 && max_m > 0, DGCNN_EINVAL,
             "%s: rows=%d, samples=%d, max_n=%d and max_m=%d must be positive", who, rows, samples, max_n, max_m);
  DG_REQUIRE(max_m <= max_n, DGCNN_EINVAL, "%s: max_m=%d exceeds max_n=%d: a cloud cannot give more samples than it has rows", who,
             max_m, max_n);
  DG_REQUIRE(ldx >= C, DGCNN_EINVAL, "%s: ldx=%lld is below C=%d", who, (long long)ldx, C);
  if (!x_off) {
    DG_REQUIRE((int64_t)rows == (int64_t)nseg * max_n && (int64_t)samples == (int64_t)nseg * max_m, DGCNN_EINVAL,
               "%s: a dense call needs rows = nseg * max_n and samples = nseg * max_m (rows=%d, samples=%d, nseg=%d, max_n=%d, max_m=%d)",
               who, rows, samples, nseg, max_n, max_m);
  } else {
    DG_REQUIRE(max_n <= rows && max_m <= samples && nseg <= rows && nseg <= samples, DGCNN_EINVAL,
               "%s: a packed call needs nseg <= samples <= rows, max_n <= rows and max_m <= samples (rows=%d, samples=%d, nseg=%d, "
               "max_n=%d, max_m=%d)", who, rows, samples, nseg, max_n, max_m);
  }
  const int res_max = dgcnn_fps_resident_max_n(C);
  const int64_t need = dgcnn_fps_workspace_bytes(rows, C, max_n);
  if (need) {
    DG_REQUIRE(ws && a16(ws), DGCNN_EINVAL, "%s: the streaming form (max_n=%d > %d) needs a 16-byte aligned workspace", who, max_n,
               res_max);
    DG_REQUIRE((int64_t)ws_bytes >= need, DGCNN_ENOSPC, "%s: workspace too small (%lld bytes needed)", who, (long long)need);
  }
  const dim3 grid((unsigned)nseg), block(FT);
  if (res_max && (x_off || max_n <= res_max)) {               // a dense call has one cloud size: one form, one launch
    const int nr = max_n < res_max ? max_n : res_max;
    const resident_fn fn = C == 1 ? resident_for<1>(nr) : C == 2 ? resident_for<2>(nr) : C == 3 ? resident_for<3>(nr) : resident_for<4>(nr);
    dg::launch(fn, grid, block, 0, ST, x, ldx, x_off, s_off, max_n, max_m, start, idx, dist);
  }
  if (max_n > res_max) {
    if (C == 3)
      dg::launch(fps_stream_kernel<3>, grid, block, 0, ST, x, ldx, C, x_off, s_off, max_n, max_m, res_max, start, idx, dist, (float*)ws);
    else
      dg::launch(fps_stream_kernel<0>, grid, block, 0, ST, x, ldx, C, x_off, s_off, max_n, max_m, res_max, start, idx, dist, (float*)ws);
  }
  return dg::check_launch(who);
}

extern "C" int dgcnn_rows_gather_f32(const float* x, int64_t ldx, const int32_t* idx, int s_rows, int x_rows, int M, int N, int F,
                                     float* y, int64_t ldy, void* stream) {
  static const char* who = "dgcnn_rows_gather_f32";
  DG_REQUIRE(x && idx && y, DGCNN_EINVAL, "%s: null x, idx or y", who);
  if (int rc = check_rows(who, s_rows, x_rows, M, N, F)) return rc;
  DG_REQUIRE(ldx >= F && ldy >= F, DGCNN_EINVAL, "%s: leading dimensions must be at least F (ldx=%lld, ldy=%lld, F=%d)", who,
             (long long)ldx, (long long)ldy, F);
  if (vec_ok(F, ldx, ldy, x, y))
    dg::launch(rows_gather_kernel<true>, dim3(grid1d((int64_t)s_rows * (F / 4), GT)), dim3(GT), 0, ST, x, ldx, idx, (int64_t)s_rows, M, N,
               F / 4, y, ldy);
  else
    dg::launch(rows_gather_kernel<false>, dim3(grid1d((int64_t)s_rows * F, GT)), dim3(GT), 0, ST, x, ldx, idx, (int64_t)s_rows, M, N, F,
               y, ldy);
  return dg::check_launch(who);
}

extern "C" int dgcnn_rows_scatter_f32(const float* dy, int64_t lddy, const int32_t* idx, int s_rows, int x_rows, int M, int N, int F,
                                      float* dx, int64_t lddx, int beta, void* stream) {
  static const char* who = "dgcnn_rows_scatter_f32";
  DG_REQUIRE(dy && idx && dx, DGCNN_EINVAL, "%s: null dy, idx or dx", who);
  if (int rc = check_rows(who, s_rows, x_rows, M, N, F)) return rc;
  DG_REQUIRE(beta == 0 || beta == 1, DGCNN_EINVAL, "%s: beta must be 0 or 1 (got %d)", who, beta);
  DG_REQUIRE(lddy >= F && lddx >= F, DGCNN_EINVAL, "%s: leading dimensions must be at least F (lddy=%lld, lddx=%lld, F=%d)", who,
             (long long)lddy, (long long)lddx, F);
  const bool vec = vec_ok(F, lddy, lddx, dy, dx);
  const int FV = vec ? F / 4 : F;
  if (!beta) {
    if (vec) dg::launch(rows_zero_kernel<true>, dim3(grid1d((int64_t)x_rows * FV, GT)), dim3(GT), 0, ST, dx, lddx, (int64_t)x_rows, FV);
    else dg::launch(rows_zero_kernel<false>, dim3(grid1d((int64_t)x_rows * FV, GT)), dim3(GT), 0, ST, dx, lddx, (int64_t)x_rows, FV);
  }
  if (vec)
    dg::launch(rows_scatter_kernel<true>, dim3(grid1d((int64_t)s_rows * FV, GT)), dim3(GT), 0, ST, dy, lddy, idx, (int64_t)s_rows, M, N, FV,
               dx, lddx, beta);
  else
    dg::launch(rows_scatter_kernel<false>, dim3(grid1d((int64_t)s_rows * FV, GT)), dim3(GT), 0, ST, dy, lddy, idx, (int64_t)s_rows, M, N, FV,
               dx, lddx, beta);
  return dg::check_launch(who);
}

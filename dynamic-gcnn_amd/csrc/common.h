// common.h -- shared helpers of libdgcnn_hip.so (gfx950 only; no CUDA compatibility paths).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <tuple>
#include <utility>
#include "../../include/dgcnn_hip.h"
#include "switches.h"

namespace dg {

void set_error(const char* fmt, ...);

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return DGCNN_ELAUNCH;
  }
  return DGCNN_OK;
}

#define DG_REQUIRE(cond, code, ...)          \
  do {                                       \
    if (!(cond)) {                           \
      dg::set_error(__VA_ARGS__);            \
      return (code);                         \
    }                                        \
  } while (0)

static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- launch plans (plan.cc) --------------------------------------------------------------------------------------------
// Every kernel launch, memset, cross-stream wait and collective of the library goes through the four functions below.  While a
// plan is being recorded (dgcnn_plan_begin .. dgcnn_plan_end) each of them ALSO appends itself -- kernel address, launch
// geometry, a private copy of the argument values, the stream -- to the plan; dgcnn_plan_replay then re-issues the whole list
// from one C loop.  The reference replays a static TF graph with sess.run (dgcnn/trainval.py:103-129); this is that, with plain
// stream semantics (same two-stream schedule as the eager step, RCCL calls included) and ~2 us of host time per launch.
bool plan_recording();
void plan_add_kernel(const void* fn, dim3 g, dim3 b, size_t sh, hipStream_t st, void** argv, const size_t* sizes, int n);
int memset_async(void* p, int value, size_t bytes, hipStream_t st);
int stream_wait(hipStream_t waiter, hipStream_t signaller);

template <class Tuple, size_t... I>
inline void launch_tuple(const void* fn, dim3 g, dim3 b, size_t sh, hipStream_t st, Tuple& args, std::index_sequence<I...>) {
  void* argv[] = {(void*)&std::get<I>(args)..., nullptr};
  (void)hipLaunchKernel(fn, g, b, argv, sh, st);
  if (plan_recording()) {
    const size_t sizes[] = {sizeof(std::get<I>(args))..., 0};
    plan_add_kernel(fn, g, b, sh, st, argv, sizes, (int)sizeof...(I));
  }
}

// launch(kernel, grid, block, dynamic LDS bytes, stream, kernel arguments...): arguments are converted to the kernel's
// parameter types exactly as a call would convert them
template <class... KA, class... A>
inline void launch(void (*k)(KA...), dim3 g, dim3 b, size_t sh, hipStream_t st, A&&... a) {
  static_assert(sizeof...(KA) == sizeof...(A), "dg::launch: argument count differs from the kernel's parameter list");
  std::tuple<KA...> args{static_cast<KA>(std::forward<A>(a))...};
  launch_tuple(reinterpret_cast<const void*>(k), g, b, sh, st, args, std::index_sequence_for<KA...>{});
}

// Accumulation slots of every `stats` / `red` buffer (double[slots][2][F]): a producer workgroup adds its partial sums to slot
// (writer index % slots).  Default DGCNN_STAT_SLOTS; dgcnn_set_stat_slots(n) with n >= the number of writers gives every slot a
// single writer -- the sums then do not depend on the order in which workgroups finish (bit-reproducible runs), api.cc.
int stat_slots();
// a grid of `g` writers, capped so that every slot keeps a single writer when the reproducible configuration is on
static inline int64_t cap_writers(int64_t g) {
  const int64_t n = stat_slots();
  return (n > DGCNN_STAT_SLOTS && g > n) ? n : g;
}

// arithmetic of the plain GEMMs (0 native fp32 MFMA, 6 / 9 = partial products of the exact three-way bf16 split on the bf16
// matrix pipe), and gemm_x3.hip's launcher (pv = GemmP*, tiles already planned)
inline int gemm_arith() { return sw_get(SW_GEMM_ARITH); }
inline void set_gemm_arith(int v) { sw_exchange(SW_GEMM_ARITH, v); }
int x3_tile_m(int M, int N, int K);
int x3_tile_n(int M, int N, int K);      // 256: the 256 x 256 kernel takes this product; 0: column tile from gemm.hip:tile_n
void launch_gemm_x3(int asrc, int bsrc, void* pv, hipStream_t st, int bn, int np);

}  // namespace dg

// ---- the small row helpers of the streaming kernels ---------------------------------------------------------------------
// grid of a grid-stride kernel over n items: blocks of bs threads, at most 65536 of them
static inline unsigned grid1d(int64_t n, int bs = 256) {
  int64_t g = dg::cdiv(n, bs);
  if (g > 65536) g = 65536;
  if (g < 1) g = 1;
  return (unsigned)g;
}

#define GRID_STRIDE(i, n) \
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// packed towers (cloud b = rows [seg_off[b], seg_off[b + 1])): the cloud that holds row r, the largest b in [0, nseg) with
// seg_off[b] <= r
__device__ __forceinline__ int cloud_of_row(const int32_t* __restrict__ seg_off, int nseg, int r) {
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (seg_off[mid] <= r) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// ---- dropout (tf.nn.dropout(net, 0.7), model.py:91): counter-based mask, element i of the flattened tensor is kept iff
// mix32(seed * K + i) < keep * 2^32; the backward regenerates the mask from the same seed (misc.hip, bn.hip)
__device__ __forceinline__ uint32_t mix32(uint64_t z) {   // splitmix64 finaliser
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return (uint32_t)(z >> 32);
}

__device__ __forceinline__ bool dropout_keeps(uint64_t seed, uint64_t i, uint32_t thr) {
  return mix32(seed * 0xD1342543DE82EF95ull + i) < thr;
}
__device__ __forceinline__ uint32_t dropout_threshold(float keep) {
  return (keep >= 1.f) ? 0xffffffffu : (uint32_t)((double)keep * 4294967296.0);
}

// ---- element offset of a gathered row: j * ld in ONE full-rate multiply (v_mul_u32_u24) -- the only caller of __umul24.
// Contract (row_offset24_ok, which every entry that launches a gathering kernel asks on the host): j < rows < 2^24, ld < 2^24,
// rows * ld < 2^32.  The product may be 2^31 or more, and HIP declares __umul24 as returning int: the UNSIGNED result must enter the
// address zero-extended (`p + row_offset24(j, ld)`, or through an `unsigned` variable).  Never cast it to int or add it to a signed
// offset first -- a sign-extended product addresses 2^32 elements before the intended row.
__device__ __forceinline__ unsigned row_offset24(unsigned j, unsigned ld) { return (unsigned)__umul24(j, ld); }
static inline bool row_offset24_ok(int64_t rows, int64_t ld) { return rows < (1 << 24) && ld < (1 << 24) && rows * ld < (1ll << 32); }

// fp32 -> the nearest bf16 value (ties to even), kept as fp32 bits.  The carry of the rounding add would run a NaN whose upper
// mantissa bits are all ones into the exponent and sign (0x7fffffff -> -0.0): a NaN stays a (quiet) NaN of the same sign instead,
// as v_cvt_pk_bf16_f32 keeps it.
__device__ __forceinline__ float round_bf16_rne(float v) {
  const unsigned u = __float_as_uint(v);
  const unsigned r = (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;
  return __uint_as_float(((u & 0x7fffffffu) > 0x7f800000u) ? ((u | 0x00400000u) & 0xffff0000u) : r);
}

// ---- the class dimension (Final layer, NUM_CLASS <= 4): the arithmetic of the streaming products of gemm.hip, shared with the
// BatchNorm kernels of bn.hip that form the same products in registers -- one definition each, so that a fused kernel performs,
// per output element, the operations of the launches it replaces in their order.
// NN: one float4 chunk of k of a row's N dots (b = the [K][N] weight in LDS at row k4), then the wave's fixed tree.
template <int N>
__device__ __forceinline__ void skinny_nn_chunk(float (&acc)[N], const float4 v, const float* b) {
#pragma unroll
  for (int n = 0; n < N; ++n) acc[n] += v.x * b[n] + v.y * b[N + n] + v.z * b[2 * N + n] + v.w * b[3 * N + n];
}
template <int N>
__device__ __forceinline__ void skinny_nn_tree(float (&acc)[N]) {
#pragma unroll
  for (int n = 0; n < N; ++n)
    for (int d = 32; d > 0; d >>= 1) acc[n] += __shfl_down(acc[n], d, 64);
}
// NT at beta = 0: o[q] = sum over k (ascending, from 0.f) of a[k] * w[q][k] -- four output columns of one row.
template <int K>
__device__ __forceinline__ void skinny_nt_quad(const float (&a)[K], const float (&w)[4][K], float (&o)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    o[q] = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) o[q] += a[k] * w[q][k];
  }
}

// softmax / cross-entropy / accuracy of ONE row of logits z[ncls] (trainval.py:39-52): probabilities, the seed of the backward
// pass and the row's terms of the two means.  Shared by softmax_xent_kernel (misc.hip) and its BatchNorm-fused form (bn.hip).
__device__ __forceinline__ void softmax_xent_row(const float* z, int ncls, int lab, float w, float inv_rows, float* softmax,
                                                 float* dlogits, float& loss, float& corr) {
  float mx = z[0];
  int am = 0;
  for (int c = 1; c < ncls; ++c)
    if (z[c] > mx) { mx = z[c]; am = c; }
  float se = 0.f;
  for (int c = 0; c < ncls; ++c) se += expf(z[c] - mx);
  const float inv = 1.0f / se;
  for (int c = 0; c < ncls; ++c) {
    const float p = expf(z[c] - mx) * inv;
    if (softmax) softmax[c] = p;
    if (dlogits) dlogits[c] = (p - (c == lab ? 1.f : 0.f)) * w * inv_rows;
  }
  if (lab >= 0) {
    loss += (logf(se) - (z[lab] - mx)) * w;
    corr += (am == lab) ? 1.f : 0.f;
  }
}

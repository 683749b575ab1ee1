// knn_common.h -- the cloud maps (dense / packed tower), lane-mask selects and the register-resident sorted (d, j) list shared by the
// k-NN kernels (knn.hip, knn_grid.hip, knn_wide.hip, knn_bigk.hip, knn_cross.hip).  What only the all-pairs scans share is in knn_scan.h.
#pragma once
#include "common.h"
#include <math.h>

namespace {

// Which rows of x a grid row (blockIdx.y = b) searches.  Dense: cloud b = rows [b N, b N + N), indices cloud-local.  Packed tower:
// cloud b = rows [off[b], off[b + 1]), indices tower rows (off[b] + j), grid cdiv(max_n, 64) x nseg -- a block past its cloud's rows
// leaves before its first barrier.  Within a cloud the arithmetic is the same: per cloud the packed result is the dense one.
struct DenseClouds {
  int N;
  __host__ __device__ constexpr DenseClouds(int n) : N(n) {}
  static constexpr bool kPacked = false;
  __device__ int64_t base(int b) const { return (int64_t)b * N; }
  __device__ int size(int) const { return N; }
};
struct PackedClouds {
  const int* __restrict__ off;               // nseg + 1 increasing tower rows, off[0] = 0
  int nseg;
  static constexpr bool kPacked = true;
  __device__ int64_t base(int b) const { return off[b]; }
  __device__ int size(int b) const { return off[b + 1] - off[b]; }
  __device__ int cloud_of(int64_t row) const {                 // last b with off[b] <= row (row wave-uniform: a scalar loop)
    int lo = 0, hi = nseg;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (off[mid] <= row) lo = mid; else hi = mid;
    }
    return lo;
  }
};
// Some clouds of a packed tower, in a listed order: grid row (slot) y = cloud list[y].  base() is still the cloud's first tower row, so
// keys keep the cloud-local j and written indices are tower rows, while everything a kernel indexes by its grid row -- GridInfo[y], cell
// table y, the early exit of blocks past the cloud's rows -- is per slot: a launch over nlist clouds is shaped cdiv(max n of the LIST,
// ...) x nlist and holds scratch for nlist clouds, whatever the tower holds besides (dgcnn_knn_seg_mix_f32).
struct ListedClouds {
  const int* __restrict__ off;               // the tower's nseg + 1 offsets
  const int* __restrict__ list;              // nlist clouds of the tower
  int nlist;
  static constexpr bool kPacked = true;
  __device__ int64_t base(int y) const { return off[list[y]]; }
  __device__ int size(int y) const { const int b = list[y]; return off[b + 1] - off[b]; }
};

// ---- lane-mask helpers.  hipcc turns nested ?: on register arrays into exec-masked branches (20
// s_and_saveexec/s_cbranch per insert, measured 10x slower); v_cmp -> SGPR-pair mask -> v_cndmask
// is forced with the fcmp/icmp builtins and a one-instruction asm select.
typedef unsigned long long lmask_t;
__device__ __forceinline__ lmask_t m_flt(float a, float b) { return __builtin_amdgcn_fcmpf(a, b, 4); }   // a <  b (ordered)
__device__ __forceinline__ lmask_t m_feq(float a, float b) { return __builtin_amdgcn_fcmpf(a, b, 1); }   // a == b
__device__ __forceinline__ lmask_t m_ilt(int a, int b) { return __builtin_amdgcn_sicmp(a, b, 40); }      // a <  b (signed)
__device__ __forceinline__ lmask_t m_ine(int a, int b) { return __builtin_amdgcn_sicmp(a, b, 33); }      // a != b
__device__ __forceinline__ float sel_f(lmask_t m, float t, float f) {
  float r;
  asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(f), "v"(t), "s"(m));
  return r;
}
__device__ __forceinline__ int sel_i(lmask_t m, int t, int f) {
  int r;
  asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(f), "v"(t), "s"(m));
  return r;
}

// smallest float greater than f (f finite or +inf; -0 counts as +0): d <= f  <=>  d < next_up(f)
__device__ __forceinline__ float next_up(float f) {
  const float g = f + 0.0f;
  const unsigned u = __float_as_uint(g);
  const unsigned v = (g >= 0.0f) ? u + 1u : u - 1u;
  return (g == INFINITY) ? g : __uint_as_float(v);
}

// lane mask -> 0 / 1 with inline constants (sel_i would park its two constants in VGPRs)
__device__ __forceinline__ unsigned sel_01(lmask_t m) {
  unsigned r;
  asm("v_cndmask_b32_e64 %0, 0, 1, %1" : "=v"(r) : "s"(m));
  return r;
}

template <bool LEX>
__device__ __forceinline__ lmask_t key_less(float d, int j, float dt, int jt) {
  return LEX ? (m_flt(d, dt) | (m_feq(d, dt) & m_ilt(j, jt))) : m_flt(d, dt);
}

// Branch-free sorted insert of (d, j) into an ascending list held in registers: per slot one
// v_cmp, one v_med3_f32 (new dl[t] = clamp(d, dl[t-1], dl[t])) and two v_cndmask for the index.
// A lane whose (d, j) is not smaller than its last entry is left unchanged (d = +inf is a no-op).
template <int KC, bool LEX>
__device__ __forceinline__ void list_insert(float (&dl)[KC], int (&jl)[KC], float d, int j) {
  lmask_t ct = key_less<LEX>(d, j, dl[KC - 1], jl[KC - 1]);
#pragma unroll
  for (int t = KC - 1; t >= 1; --t) {
    const lmask_t cp = key_less<LEX>(d, j, dl[t - 1], jl[t - 1]);
    dl[t] = __builtin_amdgcn_fmed3f(dl[t - 1], d, dl[t]);
    jl[t] = sel_i(ct, sel_i(cp, jl[t - 1], j), jl[t]);
    ct = cp;
  }
  dl[0] = sel_f(ct, d, dl[0]);
  jl[0] = sel_i(ct, j, jl[0]);
}

// ---- rows with fewer than k candidates below +inf (non-finite input; include/dgcnn_hip.h, K1) ---------------------------------------
// The selection is by (D~, j), D~ = +inf where D is NaN: the candidates no form ever lists (d < thr fails for NaN and +inf) all have
// D~ = +inf and follow the listed ones by ascending j.  Every filter in front of a list (its own k-th entry, the shared bound, a seed
// or histogram bound, a bf16 margin on a finite threshold) is finite only once k candidates at finite distance exist, so a row that
// ends with F < k entries has dropped no candidate with D < +inf: its other k - F entries are the lowest j of the cloud that are not
// among the F.  One lane per row, after the scan (a finite cloud never takes the branch): `jat(t)` = the t-th listed cloud-local j,
// t < F; the fill is written to out[F .. k) with `base` added (the cloud's first tower row, 0 for dense clouds).  k <= N: the loop
// ends by v < N whatever the list holds, and stores to out[c], c < k, only.
template <int KC, class JAt>
__device__ __forceinline__ void fill_short_row(JAt jat, int F, int k, int N, int base, int32_t* out) {
  int c = F;
#pragma unroll 1
  for (int v = 0; v < N && c < k; ++v) {
    bool in = false;
#pragma unroll
    for (int t = 0; t < KC; ++t) in = in || (t < F && jat(t) == v);
    if (!in) out[c++] = base + v;
  }
}
// the sentinel form: a list of the scan kernels, ascending, open slots = 0x7fffffff at its end
template <int KC>
__device__ __forceinline__ void fill_short_list(const int (&jl)[KC], int k, int N, int base, int32_t* out) {
  int F = 0;
#pragma unroll
  for (int t = 0; t < KC; ++t) F += (t < k && jl[t] != 0x7fffffff) ? 1 : 0;
  if (F < k) fill_short_row<KC>([&](int t) { return jl[t]; }, F, k, N, base, out);
}

// ---- 64-bit selection keys and the wave-level compare-exchange (the append-form scan of knn.hip, the large-k scan of knn_bigk.hip) ----
// key = orderable bits of d << 32 | j: unsigned order == (d, j) lexicographic order (d never NaN / -0)
__device__ __forceinline__ unsigned long long knn_key(float d, int j) {
  const unsigned u = __float_as_uint(d + 0.0f);
  const unsigned o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)o << 32) | (unsigned)j;
}

// value of lane (l ^ M): quad permutes and bank-masked row shifts on the DPP path for M < 16 (no LDS round trip, no address register),
// ds_swizzle for 16, ds_bpermute for 32
template <int M>
__device__ __forceinline__ unsigned xchg32(unsigned v) {
  if constexpr (M == 1) return (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xF, 0xF, false);        // quad_perm [1,0,3,2]
  else if constexpr (M == 2) return (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]
  else if constexpr (M == 4) {
    const int t = __builtin_amdgcn_update_dpp((int)v, (int)v, 0x104, 0xF, 0x5, false);       // row_shl:4 into banks 0, 2 (lanes with bit 2 clear)
    return (unsigned)__builtin_amdgcn_update_dpp(t, (int)v, 0x114, 0xF, 0xA, false);         // row_shr:4 into banks 1, 3
  } else if constexpr (M == 8) {
    const int t = __builtin_amdgcn_update_dpp((int)v, (int)v, 0x108, 0xF, 0x3, false);       // row_shl:8 into banks 0, 1
    return (unsigned)__builtin_amdgcn_update_dpp(t, (int)v, 0x118, 0xF, 0xC, false);         // row_shr:8 into banks 2, 3
  } else if constexpr (M == 16) return (unsigned)__builtin_amdgcn_ds_swizzle((int)v, 0x401F);   // bit mode: and 0x1f, or 0, xor 16
  else return __shfl_xor(v, M, 64);
}
template <int M>
__device__ __forceinline__ unsigned long long xchg64(unsigned long long v) {
  const unsigned lo = xchg32<M>((unsigned)v), hi = xchg32<M>((unsigned)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}
template <int J2>
__device__ __forceinline__ unsigned long long bitonic_step(unsigned long long key, int lane, bool up) {
  const unsigned long long pk = xchg64<J2>(key);
  const bool take_min = ((lane & J2) == 0) == up;
  return (take_min == (pk < key)) ? pk : key;
}

}  // namespace

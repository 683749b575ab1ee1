// bn_common.h -- the element arithmetic of every BatchNorm family (bn.hip, seg_bn.hip, planes_bn.hip, edge_mlp_bf16.hip), ONE
// definition each.  The library is built with -ffp-contract=off (Makefile): every expression below is the fp32 operations it spells,
// in that order, in whichever kernel it is inlined.  The bit-level properties of the library rest on that and on these functions
// being shared: the max recomputed in a backward compares equal to the values the forward took it over, a one-cloud tower gives the
// dense kernels' output, the fused bf16 backward reads the count the fp32 forward packed.
#pragma once
#include "common.h"

// xhat and z = act(xhat + beta) of one element (T = float), or of a channel pair (T = f32x2, kreduce_held of bn.hip: the same
// operations element-wise, as v_pk_add_f32 / v_pk_mul_f32)
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float bn_relu(float z) { return fmaxf(z, 0.f); }
__device__ __forceinline__ f32x2 bn_relu(f32x2 z) { return f32x2{fmaxf(z.x, 0.f), fmaxf(z.y, 0.f)}; }
template <class T>
__device__ __forceinline__ T bn_z(T y, T mu, T rs, T be, int relu, T& xh) {
  xh = (y - mu) * rs;
  T z = xh + be;
  if (relu) z = bn_relu(z);
  return z;
}
__device__ __forceinline__ float bn_z(float y, float mu, float rs, float be, int relu) {
  float xh;
  return bn_z(y, mu, rs, be, relu, xh);
}

// ---- the packed count of a point's k edge rows: #ties of the max + CNT_POS * #(rows with z > 0), both exact small integers in fp32
// (k < CNT_POS).  The edge forwards write it, the backwards read the ties, the point-level reduce reads the positives.
constexpr int CNT_POS = 256;
__device__ __forceinline__ float cnt_pack(float ties, float npos) { return ties + (float)CNT_POS * npos; }
// what ONE row adds to the packed count beside the ties, for the loops that keep the second term already scaled
__device__ __forceinline__ float cnt_pos_term(float z) { return (z > 0.f) ? (float)CNT_POS : 0.f; }
__device__ __forceinline__ float cnt_npos(float c) { return floorf(c * (1.0f / CNT_POS)); }
__device__ __forceinline__ float cnt_ties(float c) { return c - (float)CNT_POS * cnt_npos(c); }

// ---- backward.  What reaches an edge row from the max and the mean over k: the ties share the gradient of
// the max, every row takes its share of the mean's; dmax_tie = dmax / ties and dmean_k = dmean * (1.0f / k) are formed by the caller
// -- per element or hoisted out of the loop over the k rows, the same division and the same product either way.
__device__ __forceinline__ float bn_edge_dout(float z, float mx, float dmax_tie, float dmean_k) {
  return ((z == mx) ? dmax_tie : 0.f) + dmean_k;
}
// dz of a k = 1 row from its incoming gradient d (consumers already added, dropout already applied): zero where the layer has a ReLU
// and !(z > 0).  dz of an edge row: the same gate on bn_edge_dout.
__device__ __forceinline__ float bn_dz_row(float z, float d, int relu) {
  if (relu && !(z > 0.f)) d = 0.f;
  return d;
}
__device__ __forceinline__ float bn_dz_edge(float z, float mx, float dmax_tie, float dmean_k, int relu) {
  return bn_dz_row(z, bn_edge_dout(z, mx, dmax_tie, dmean_k), relu);
}
// dY = rstd (dz - c1 - xhat c2), c1 = mean dz, c2 = mean dz xhat
__device__ __forceinline__ float bn_dy(float rs, float dz, float c1, float xh, float c2) { return rs * (dz - c1 - xh * c2); }

// ---- V adjacent channels of a row <-> registers: one 16-byte access (V = 4) or one element (V = 1)
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

// seg_loss.hip -- softmax, accuracy and sparse softmax cross-entropy of a PACKED tower taken CLOUD BY CLOUD (dgcnn/trainval.py:39-52
// as `-mbs 1` runs it: one reduce_mean per cloud).  Cloud b = rows [seg_off[b], seg_off[b + 1]) of the tower, n_b rows:
//   l_b = (1 / n_b) sum_{r in b} w_r (log sum_c e^{z_rc} - z_{r, lab_r}),   a_b = #{r in b : first arg-max of z_r == lab_r} / n_b,
//   dlogits_r = (p_r - onehot_r) w_r / n_b   (the SUM over the clouds of the per-cloud means: M micro-steps of -mbs 1 add up),
//   scal = [(1 / nseg) sum_b l_b, (1 / nseg) sum_b a_b].
// The per-row arithmetic is misc.hip's softmax_xent_kernel operation for operation, with 1.0f / n_b where that kernel has
// 1.0f / rows: a one-cloud tower gives its softmax and dlogits bit for bit.
//
// The sums follow seg_bn.hip's two stages, in ONE fixed order (no atomics variant; results are WRITTEN, nothing is zero-filled):
// stage 1 works over 64-row chunks of the tower cut at the cloud boundaries inside them (grids over chunks, never one workgroup
// per cloud); wave w owns rows w, w + 4, ... of a (chunk, cloud) piece -- one row per lane, 16 lanes -- and adds their terms in
// fp32 (ascending), the four waves are added in double (0..3) into partial slot (chunk + b): slots grow strictly with (chunk, b),
// so the pieces of cloud b are a contiguous run.  Stage 2 adds a cloud's slots first chunk to last in double, and the clouds
// b-ascending in double for the tower's two scalars.
#include "common.h"

namespace {

constexpr int SEG_CHUNK = 64;                       // rows of the tower per workgroup (seg_bn.hip's chunk)
constexpr int SEG_WAVES = 4;                        // wave w owns rows w, w + 4, ... of a piece
constexpr int SEG_LANES = SEG_CHUNK / SEG_WAVES;    // ... one per lane: a piece is covered in one pass
constexpr int FIN_THREADS = 256;
constexpr int FIN_BATCH = 8;                        // independent slot loads in flight per thread (stage 2)

// ---- stage 1: the rows (softmax, dlogits) and, with labels, part[chunk + b][2] = (sum of w * xent, #correct) of every piece ------
// SUMS = false (labels == nullptr): the softmax only, no shared memory, `part` untouched.
template <bool SUMS>
__global__ __launch_bounds__(64 * SEG_WAVES) void seg_xent_partial_kernel(const float* __restrict__ logits,
                                                                          const int32_t* __restrict__ labels,
                                                                          const float* __restrict__ weight, int rows, int ncls,
                                                                          const int32_t* __restrict__ seg_off, int nseg,
                                                                          float* __restrict__ softmax, float* __restrict__ dlogits,
                                                                          double* __restrict__ part) {
  __shared__ float sv[SUMS ? SEG_CHUNK : 1][2][SEG_WAVES];    // [piece of the chunk][sum][wave]: at most one piece per row
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int chunk = blockIdx.x;
  const int r0 = chunk * SEG_CHUNK;
  const int r1 = imin(r0 + SEG_CHUNK, rows);
  const int b0 = cloud_of_row(seg_off, nseg, r0);
  int b = b0, ps = r0, np = 0;
  while (ps < r1 && b < nseg) {                               // (workgroup-uniform)
    const int pe = imin(seg_off[b + 1], r1);
    const float inv_n = 1.0f / (float)(seg_off[b + 1] - seg_off[b]);
    float loss = 0.f, corr = 0.f;
    const int i = ps + w + SEG_WAVES * lane;
    if (lane < SEG_LANES && i < pe) {
      const int64_t r = i;
      const float* z = logits + r * ncls;
      float mx = z[0];
      int am = 0;
      for (int c = 1; c < ncls; ++c)
        if (z[c] > mx) { mx = z[c]; am = c; }
      float se = 0.f;
      for (int c = 0; c < ncls; ++c) se += expf(z[c] - mx);
      const float inv = 1.0f / se;
      const int lab = SUMS ? labels[r] : -1;
      const float wr = weight ? weight[r] : 1.f;
      for (int c = 0; c < ncls; ++c) {
        const float p = expf(z[c] - mx) * inv;
        if (softmax) softmax[r * ncls + c] = p;
        if (dlogits) dlogits[r * ncls + c] = (p - (c == lab ? 1.f : 0.f)) * wr * inv_n;
      }
      if (lab >= 0) {
        loss = (logf(se) - (z[lab] - mx)) * wr;
        corr = (am == lab) ? 1.f : 0.f;
      }
    }
    if (SUMS) {
      float sl = 0.f, sc = 0.f;                               // the wave's <= 16 rows, ascending (lanes without a row hold 0)
      for (int j = 0; j < SEG_LANES; ++j) { sl += __shfl(loss, j); sc += __shfl(corr, j); }
      if (lane == 0) { sv[np][0][w] = sl; sv[np][1][w] = sc; }
    }
    ps = pe;
    ++b;
    ++np;
  }
  if (SUMS) {
    __syncthreads();
    for (int e = threadIdx.x; e < 2 * np; e += 64 * SEG_WAVES) {
      const int p = e >> 1, which = e & 1;
      double t = 0.0;
      for (int ww = 0; ww < SEG_WAVES; ++ww) t += (double)sv[p][which][ww];
      part[(int64_t)(chunk + b0 + p) * 2 + which] = t;
    }
  }
}

// ---- stage 2 (one workgroup: the tower's scalars need every cloud): thread per cloud, its slots first chunk to last in double
// (FIN_BATCH loads in flight, added in order); cl[b] = (l_b, a_b) in double, cloud_scal[b] = their fp32 values; then one thread
// per scalar adds cl over the clouds, b ascending, and scales by 1.0 / nseg
__global__ __launch_bounds__(FIN_THREADS) void seg_xent_final_kernel(const double* __restrict__ part, const int32_t* __restrict__ seg_off,
                                                                     int nseg, double* __restrict__ cl, float* __restrict__ cloud_scal,
                                                                     float* __restrict__ scal) {
  for (int b = threadIdx.x; b < nseg; b += FIN_THREADS) {
    const int o0 = seg_off[b], o1 = seg_off[b + 1];
    const int cfirst = o0 / SEG_CHUNK, clast = (o1 - 1) / SEG_CHUNK;
    const double* p = part + (int64_t)b * 2;
    double s = 0.0, q = 0.0;
    int c = cfirst;
    for (; c + FIN_BATCH - 1 <= clast; c += FIN_BATCH) {
      double vs[FIN_BATCH], vq[FIN_BATCH];
#pragma unroll
      for (int u = 0; u < FIN_BATCH; ++u) { vs[u] = p[(int64_t)(c + u) * 2]; vq[u] = p[(int64_t)(c + u) * 2 + 1]; }
#pragma unroll
      for (int u = 0; u < FIN_BATCH; ++u) { s += vs[u]; q += vq[u]; }
    }
    for (; c <= clast; ++c) { s += p[(int64_t)c * 2]; q += p[(int64_t)c * 2 + 1]; }
    const double n = (double)(o1 - o0);
    const double lb = s * (1.0 / n), ab = q / n;
    cl[(int64_t)b * 2] = lb;
    cl[(int64_t)b * 2 + 1] = ab;
    cloud_scal[(int64_t)b * 2] = (float)lb;
    cloud_scal[(int64_t)b * 2 + 1] = (float)ab;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0 && (threadIdx.x >> 6) < 2) {    // (one wave per scalar)
    const int which = threadIdx.x >> 6;
    double t = 0.0;
    for (int b = 0; b < nseg; ++b) t += cl[(int64_t)b * 2 + which];
    scal[which] = (float)(t * (1.0 / (double)nseg));
  }
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int64_t dgcnn_seg_softmax_xent_workspace_bytes(int rows, int nseg) {
  if (rows <= 0 || nseg <= 0) return 0;
  // [partial slots (chunks + nseg)][2] + [per-cloud doubles nseg][2]
  return (dg::cdiv(rows, SEG_CHUNK) + 2 * (int64_t)nseg) * 2 * (int64_t)sizeof(double);
}

extern "C" int dgcnn_seg_softmax_xent_f32(const float* logits, const int32_t* labels, const float* weight, int rows, int ncls,
                                          const int32_t* seg_off, int nseg, float* softmax, float* dlogits, float* cloud_scal,
                                          float* scal, void* ws, size_t ws_bytes, void* stream) {
  const char* what = "dgcnn_seg_softmax_xent_f32";
  DG_REQUIRE(logits && seg_off, DGCNN_EINVAL, "%s: null pointer", what);
  DG_REQUIRE(rows > 0 && ncls > 0 && nseg > 0, DGCNN_EINVAL, "%s: bad shape", what);
  DG_REQUIRE(nseg <= rows && nseg <= 65535, DGCNN_EINVAL, "%s: %d clouds in %d rows (at most one per row, at most 65535)", what, nseg,
             rows);
  DG_REQUIRE(!dlogits || labels, DGCNN_EINVAL, "%s: dlogits needs labels", what);
  DG_REQUIRE(labels || softmax, DGCNN_EINVAL, "%s: neither labels nor a softmax to write", what);
  const unsigned chunks = (unsigned)dg::cdiv(rows, SEG_CHUNK);
  if (!labels) {                                              // the softmax only: cloud_scal / scal / ws untouched
    dg::launch(seg_xent_partial_kernel<false>, dim3(chunks), dim3(64 * SEG_WAVES), 0, ST, logits, labels, weight, rows, ncls, seg_off,
               nseg, softmax, dlogits, (double*)nullptr);
    return dg::check_launch(what);
  }
  DG_REQUIRE(cloud_scal && scal, DGCNN_EINVAL, "%s: labels need cloud_scal and scal", what);
  const size_t need = (size_t)dgcnn_seg_softmax_xent_workspace_bytes(rows, nseg);
  DG_REQUIRE(ws && ws_bytes >= need && (reinterpret_cast<uintptr_t>(ws) & 7) == 0, DGCNN_EINVAL,
             "%s: workspace too small or not 8-byte aligned (%zu < %zu bytes)", what, ws_bytes, need);
  double* part = reinterpret_cast<double*>(ws);
  double* cl = part + ((int64_t)chunks + nseg) * 2;
  dg::launch(seg_xent_partial_kernel<true>, dim3(chunks), dim3(64 * SEG_WAVES), 0, ST, logits, labels, weight, rows, ncls, seg_off, nseg,
             softmax, dlogits, part);
  int rc = dg::check_launch(what);
  if (rc) return rc;
  dg::launch(seg_xent_final_kernel, dim3(1), dim3(FIN_THREADS), 0, ST, part, seg_off, nseg, cl, cloud_scal, scal);
  return dg::check_launch(what);
}

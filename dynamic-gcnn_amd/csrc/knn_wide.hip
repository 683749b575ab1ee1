// knn_wide.hip -- K1 for wide feature rows (C up to 1024): the fp32 matrix-pipe scan of knn.hip:knn_mfma_kernel with the channel
// dimension walked in slabs of 64, and the s_i kernel for rows too wide for one LDS stage.
//
// MUST be compiled with -ffp-contract=off (csrc/Makefile).  The arithmetic is the normative one of oracle/knn_oracle.c:
//     s_i  = sequential sum of fl(x*x) over c ascending (no FMA)
//     p_ij = fmaf chain over c = 0 .. C-1 from +0
//     D_ij = fl( fl(s_i + s_j) - 2 p_ij )
// v_mfma_f32_32x32x2_f32 is bit for bit an fmaf chain in k order on gfx950, and its accumulator input is never rounded or flushed, so
// the 16 accumulators of a 64-candidate tile carried from slab s to slab s + 1 ARE that chain over all C channels.  Channels past C
// in the last slab are +0 on both operands: fmaf(0, 0, p) = p for every p (NaN and infinities included), so they change nothing.
//
// Where the operands come from.  knn_mfma_kernel keeps the query rows resident (CP / 2 VGPRs) and the whole candidate tile [CP][66]
// in LDS twice; neither scales past C = 128.  Here every step of the flattened (tile, slab) sequence stages TWO k-major slab tiles
// [64 channels][66], double buffered: the candidates' and the block's own 64 query rows' (a re-read that hits L2: a block's query rows
// are 64 C floats, <= 256 KB).  The query slab in the candidates' layout makes the B operand the same conflict-free ds_read_b32 as the
// A operand (lane = row, one channel per instruction); a direct per-lane load from global memory would be 32 strided 4-byte loads
// of 32 different lines per wave-instruction per step, and an LDS copy of the whole rows fits only to C ~ 256.  Both operands run
// through a ring two MFMAs deep, so the query operand costs 2 VGPRs instead of 32.
// LDS: 4 slab tiles + 8 parked distances per thread + s_j + the shared bound = 77,312 bytes: two blocks per CU.  (Parking all 16
// distances of a lane, as knn_mfma_kernel does, is 85.5 KB: one block per CU; the drain therefore runs in two halves of 8.)
#include "knn_common.h"

namespace {

constexpr int ROWS = 64;

// s_i for C > 128 (knn.hip:sqnorm_kernel stages [64][C + 1] floats, which passes 64 KB at C = 255): the same sequential
// s = s + fl(v v) over c ascending, the block's 64 rows staged through LDS in chunks of 64 channels (coalesced loads), the running s
// kept by the row's thread.
__global__ __launch_bounds__(256) void sqnorm_wide_kernel(const float* __restrict__ x, int64_t ldx, int64_t rows, int C,
                                                          float* __restrict__ sq) {
  constexpr int CH = 64, S = CH + 1;
  __shared__ float tile[ROWS * S];
  const int64_t r0 = (int64_t)blockIdx.x * ROWS;
  const int t = threadIdx.x;
  float s = 0.0f;
#pragma unroll 1
  for (int c0 = 0; c0 < C; c0 += CH) {
    const int cw = (C - c0 < CH) ? C - c0 : CH;
    __syncthreads();
    for (int e = t; e < ROWS * CH; e += 256) {
      const int rr = e >> 6, cc = e & 63;
      if (cc < cw) tile[rr * S + cc] = (r0 + rr < rows) ? x[(r0 + rr) * ldx + c0 + cc] : 0.0f;
    }
    __syncthreads();
    if (t < ROWS) {
      for (int c = 0; c < cw; ++c) {
        const float v = tile[t * S + c];
        const float q = v * v;
        s = s + q;
      }
    }
  }
  if (t < ROWS && r0 + t < rows) sq[r0 + t] = s;
}

// Block = 64 query rows x 2 candidate halves (4 waves), D layout, per-lane sorted lists, shared selection bound, LDS merge and
// fill_short_list as in knn_mfma_kernel (knn.hip); Clouds as in knn_kernel: keys keep the cloud-local j, a packed block past its cloud
// leaves before the first barrier, the cloud's first tower row is added when the indices are written.
// Non-finite input: every trip count below is a function of N, C and k, and every store address of a lane, an LDS slot or the row's k
// output slots; a distance only ever sets mask bits (d < thr is false for NaN and +inf), and the drain pops one bit per iteration.
// Two waves per SIMD (what the LDS admits) for KC <= 40; the KC = 64 lists (128 VGPRs) beside the 32 staging registers do not fit 256
// registers without scratch, so that instance takes one wave per SIMD (344 registers).
template <int KC, bool VEC, class Clouds>
__global__ __launch_bounds__(256, (KC <= 40 ? 2 : 1)) void knn_wide_kernel(const float* __restrict__ x, const float* __restrict__ sq,
                                                                           Clouds cl, int C, int64_t ldx, int k,
                                                                           int32_t* __restrict__ idx) {
  using f32x16 = __attribute__((ext_vector_type(16))) float;
  constexpr int SL = 64;                     // channels per slab
  constexpr int TJM = 64;                    // candidates per tile: 32 per candidate-half wave
  constexpr int ST = TJM + 2;                // k-major slab tile [SL][ST]
  constexpr int TILE_F = SL * ST;
  constexpr int DQ_F = 8 * 256;
  constexpr int MERGE_F = ROWS * KC * 2;
  constexpr int WORK_F = 4 * TILE_F + DQ_F + 2 * TJM + 4 * ROWS;
  constexpr int SH = (WORK_F > MERGE_F ? WORK_F : MERGE_F);
  constexpr int NV = (TJM * (SL / 4)) / 256;  // float4 staged per thread per slab tile
  __shared__ __attribute__((aligned(16))) float smem[SH];
  float* dq = smem + 4 * TILE_F;
  float* sjs = dq + DQ_F;                    // [2][TJM], by tile parity
  volatile float* thrw = sjs + 2 * TJM;      // [4 lists][64 rows]: list[KC/4 - 1] so far

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int qg = w & 1;                      // which 32 query rows of the block
  const int cs = w >> 1;                     // which 32 candidates of every 64-candidate tile
  const int b = blockIdx.y;
  const int N = cl.size(b);
  const int row0 = blockIdx.x * ROWS;
  if (Clouds::kPacked && row0 >= N) return;
  const int64_t cb = cl.base(b);
  const int row = row0 + qg * 32 + l31;
  const float* xb = x + cb * ldx;
  const float* sqb = sq + cb;
  const int rowc = row < N ? row : N - 1;
  const float si = sqb[rowc];

  float dl[KC];
  int jl[KC];
#pragma unroll
  for (int t = 0; t < KC; ++t) {
    dl[t] = INFINITY;
    jl[t] = 0x7fffffff;
  }

  // ---- slab tiles: global -> registers one step ahead, transposed ([c][row]) into the other LDS buffer after the current step's
  // MFMAs; one barrier per step.  VEC (16-byte aligned rows, C % 4 == 0): one unconditional float4 load per piece from a clamped,
  // always valid address.  Candidate rows past N carry |x_j|^2 = +inf (never selected); query rows past N repeat row N - 1 (never
  // written); channel quads past C are zeroed.
  float4 prec[NV], preq[NV];
  float pre_s = INFINITY;
  auto load4 = [&](int r, int ch, bool live) -> float4 {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (VEC) {
      const int cc = ch < C ? ch : C - 4;
      const float4 t4 = *reinterpret_cast<const float4*>(xb + (int64_t)r * ldx + cc);
      const bool ok = ch < C;
      v.x = ok ? t4.x : 0.f; v.y = ok ? t4.y : 0.f; v.z = ok ? t4.z : 0.f; v.w = ok ? t4.w : 0.f;
    } else if (live) {
      const float* src = xb + (int64_t)r * ldx + ch;
      if (ch + 0 < C) v.x = src[0];
      if (ch + 1 < C) v.y = src[1];
      if (ch + 2 < C) v.z = src[2];
      if (ch + 3 < C) v.w = src[3];
    }
    return v;
  };
  auto fetch = [&](int j0, int c0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int e = tid + 256 * i;
      const int r = e >> 4;
      const int ch = c0 + (e & 15) * 4;
      const int j = j0 + r, q = row0 + r;
      prec[i] = load4(j < N ? j : N - 1, ch, j < N);
      preq[i] = load4(q < N ? q : N - 1, ch, true);
    }
    if (c0 == 0 && tid < TJM) pre_s = (j0 + tid < N) ? sqb[j0 + tid] : INFINITY;
  };
  auto stash = [&](int buf, int tpar, bool first_slab) {
    float* dc = smem + buf * 2 * TILE_F;
    float* dqr = dc + TILE_F;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int e = tid + 256 * i;
      const int r = e >> 4;
      const int c4 = (e & 15) * 4;
      dc[(c4 + 0) * ST + r] = prec[i].x;
      dc[(c4 + 1) * ST + r] = prec[i].y;
      dc[(c4 + 2) * ST + r] = prec[i].z;
      dc[(c4 + 3) * ST + r] = prec[i].w;
      dqr[(c4 + 0) * ST + r] = preq[i].x;
      dqr[(c4 + 1) * ST + r] = preq[i].y;
      dqr[(c4 + 2) * ST + r] = preq[i].z;
      dqr[(c4 + 3) * ST + r] = preq[i].w;
    }
    if (first_slab && tid < TJM) sjs[tpar * TJM + tid] = pre_s;
  };

  const int nt = (N + TJM - 1) / TJM;
  const int ns = (C + SL - 1) / SL;
  const int nu = nt * ns;                    // steps of the flattened (tile, slab) sequence
  fetch(0, 0);
  stash(0, 0, true);
  thrw[tid] = INFINITY;
  const int lid = cs * 2 + h;                // list id of this lane among the 4 lists of its row (= `me` below)
  const int rslot = qg * 32 + l31;           // row within the block
  const int cbase = cs * 32;
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
    if (u + 1 < nu) fetch(tn * TJM, sn * SL);
    if (j0 + cbase < N) {                    // wave-uniform, the same for every slab of a tile
      const float* ap = smem + buf * 2 * TILE_F + h * ST + cbase + l31;          // A: candidate cbase + l31, channel 2 s2 + h
      const float* bp = smem + buf * 2 * TILE_F + TILE_F + h * ST + qg * 32 + l31;   // B: query row, channel 2 s2 + h
      {
        // operand rings, two MFMAs deep: the operands of step s2 + 2 are requested right behind MFMA s2, whose 64 clocks in the pipe
        // (the chain is dependent) cover the LDS round trip
        constexpr int NS = SL / 2;
        float a0 = ap[0], b0 = bp[0], a1 = ap[2 * ST], b1 = bp[2 * ST];
#pragma unroll
        for (int s2 = 0; s2 < NS; s2 += 2) {
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc, 0, 0, 0);
          if (s2 + 2 < NS) { a0 = ap[2 * (s2 + 2) * ST]; b0 = bp[2 * (s2 + 2) * ST]; }
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc, 0, 0, 0);
          if (s2 + 3 < NS) { a1 = ap[2 * (s2 + 3) * ST]; b1 = bp[2 * (s2 + 3) * ST]; }
        }
      }
      if (s == ns - 1) {
        // ---- the chain is complete: distances of this lane's 16 candidates in two halves of 8; park them, flag the ones that can
        // still enter the row's top KC, drain in ascending j (the order the strict insert's tie rule needs) ----
        const float o1 = thrw[(lid ^ 1) * ROWS + rslot], o2 = thrw[(lid ^ 2) * ROWS + rslot], o3 = thrw[(lid ^ 3) * ROWS + rslot];
        const float* sj = sjs + (t & 1) * TJM + cbase + 4 * h;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const float thr = fminf(dl[KC - 1], next_up(fmaxf(fmaxf(dl[KC / 4 - 1], o1), fmaxf(o2, o3))));
          unsigned mask = 0u;
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            const float4 s4 = *reinterpret_cast<const float4*>(sj + 8 * (2 * half + q));   // candidates 8 (2 half + q) + 4 h + (0..3)
            const float sv[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int r = 4 * q + e;
              const float tt = si + sv[e];
              // (tt - 2 p in ONE rounding: 2 p is exact, so the fused form equals the oracle's  tt - fl(2 p)  bit for bit)
              const float d = __builtin_fmaf(-2.0f, acc[8 * half + r], tt);
              dq[r * 256 + tid] = d;
              mask |= sel_01(m_flt(d, thr)) << r;
            }
          }
          int g = __builtin_ctz(mask | 0x80000000u) & 7;
          float dcur = dq[g * 256 + tid];
          while (__any(mask != 0u)) {
            const lmask_t live = m_ine((int)mask, 0);
            const int gc = g + 8 * half;
            mask &= mask - 1u;
            g = __builtin_ctz(mask | 0x80000000u) & 7;
            const float dnext = dq[g * 256 + tid];
            const float d = sel_f(live, dcur, INFINITY);
            const int i = (gc & 3) + 8 * (gc >> 2) + 4 * h;
            list_insert<KC, false>(dl, jl, d, j0 + cbase + i);
            dcur = dnext;
          }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      }
    }
    if (u + 1 < nu) stash(buf ^ 1, tn & 1, sn == 0);
    __syncthreads();
    s = sn;
    t = tn;
  }

  // ---- merge: 4 lists per query row (2 lane halves x 2 candidate halves) -> lanes 0..31 of waves 0,1 ----
  __syncthreads();
  float* md = smem;
  int* mj = reinterpret_cast<int*>(smem + ROWS * KC);
  const int me = lid;                        // id 0 is the destination
#pragma unroll 1
  for (int src = 1; src < 4; ++src) {
    if (src > 1) __syncthreads();
    if (me == src) {
#pragma unroll
      for (int q = 0; q < KC; ++q) {
        md[q * ROWS + rslot] = dl[q];
        mj[q * ROWS + rslot] = jl[q];
      }
    }
    __syncthreads();
    if (cs == 0) {                           // wave-uniform; lanes with h == 1 idle along (d = +inf)
#pragma unroll 1
      for (int q = 0; q < KC; ++q) {
        const float d = (h == 0) ? md[q * ROWS + rslot] : INFINITY;
        const int j = (h == 0) ? mj[q * ROWS + rslot] : 0x7fffffff;
        const lmask_t need = key_less<true>(d, j, dl[KC - 1], jl[KC - 1]);
        if (need == 0) break;
        list_insert<KC, true>(dl, jl, d, j);
      }
    }
  }
  if (me == 0 && row < N) {
    int32_t* out = idx + (cb + row) * k;
#pragma unroll
    for (int q = 0; q < KC; ++q)
      if (q < k) out[q] = Clouds::kPacked ? (int)cb + jl[q] : jl[q];
    fill_short_list<KC>(jl, k, N, Clouds::kPacked ? (int)cb : 0, out);      // fewer than k candidates below +inf (knn_common.h)
  }
}

template <int KC, class Clouds>
void launch_wide_k(dim3 grid, hipStream_t st, const float* x, const float* sq, Clouds cl, int C, int64_t ldx, int k, bool vec,
                   int32_t* idx) {
  if (vec) dg::launch((knn_wide_kernel<KC, true, Clouds>), grid, dim3(256), 0, st, x, sq, cl, C, ldx, k, idx);
  else dg::launch((knn_wide_kernel<KC, false, Clouds>), grid, dim3(256), 0, st, x, sq, cl, C, ldx, k, idx);
}

template <class Clouds>
void launch_wide(dim3 grid, hipStream_t st, const float* x, const float* sq, Clouds cl, int C, int64_t ldx, int k, bool vec,
                 int32_t* idx) {
  if (k <= 8) launch_wide_k<8>(grid, st, x, sq, cl, C, ldx, k, vec, idx);
  else if (k <= 20) launch_wide_k<20>(grid, st, x, sq, cl, C, ldx, k, vec, idx);
  else if (k <= 40) launch_wide_k<40>(grid, st, x, sq, cl, C, ldx, k, vec, idx);
  else launch_wide_k<64>(grid, st, x, sq, cl, C, ldx, k, vec, idx);
}

}  // namespace

namespace dg {

void launch_sqnorm_wide(const float* x, int64_t ldx, int64_t rows, int C, float* sq, hipStream_t st) {
  dg::launch(sqnorm_wide_kernel, dim3((unsigned)dg::cdiv(rows, ROWS)), dim3(256), 0, st, x, ldx, rows, C, sq);
}

// The all-pairs search of ny clouds, s_i in sq.  seg_off null: dense clouds of max_n rows each; else the nseg + 1 offsets of a packed
// tower (ny = nseg).  vec_ok: rows are float4-loadable (the float4 loader also needs C % 4 == 0).  5 <= C <= 1024, k <= 64.
void launch_knn_wide(const float* x, const float* sq, const int32_t* seg_off, int ny, int max_n, int C, int64_t ldx, int k, int vec_ok,
                     int32_t* idx, hipStream_t st) {
  const dim3 grid((unsigned)dg::cdiv(max_n, ROWS), (unsigned)ny);
  const bool vec = vec_ok && C % 4 == 0;
  if (seg_off) launch_wide(grid, st, x, sq, PackedClouds{seg_off, ny}, C, ldx, k, vec, idx);
  else launch_wide(grid, st, x, sq, DenseClouds(max_n), C, ldx, k, vec, idx);
}

}  // namespace dg

/*
 * dgcnn_hip.h -- C ABI of libdgcnn_hip.so: the MI355X (gfx950) EdgeConv hot path of DGCNN.
 *
 * The reference (DeepLearnPhysics/dynamic-gcnn) has no FFI of its own: its hot path is Python
 * that composes stock TensorFlow-1 ops.  Each entry point below therefore names
 * the reference *call site* (file:line under /root/reference) whose TF op group it replaces; the
 * Python mirror of the reference's operator surface (dynamic-gcnn_amd/dgcnn/{ops,model,trainval}.py)
 * binds exactly these symbols through ctypes.
 *
 * Conventions
 *   - every function returns 0 on success or a negative DGCNN_E* code; dgcnn_last_error() gives
 *     the message of the last failure on the calling thread;
 *   - all pointers are DEVICE pointers owned by the caller (the library allocates nothing and
 *     keeps no state), tensors are dense row-major fp32 unless a leading dimension `ld*`
 *     (in elements) is given; indices are batch-local int32;
 *   - every call is asynchronous on the caller-supplied hipStream_t (passed as void*);
 *   - `stats` buffers are double[slots][2][F] (sum, sum of squares), zeroed by the
 *     caller, accumulated by the producing kernel's epilogue, reduced by dgcnn_bn_finalize_f32;
 *     slots = DGCNN_STAT_SLOTS unless dgcnn_set_stat_slots() changed it.
 */
#ifndef DGCNN_HIP_H_
#define DGCNN_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DGCNN_OK 0
#define DGCNN_EINVAL (-1)   /* bad argument (e.g. k > N: tf.nn.top_k would raise, dgcnn/ops.py:18) */
#define DGCNN_ELAUNCH (-2)  /* HIP launch/runtime error */
#define DGCNN_ENOSPC (-3)   /* workspace too small */
#define DGCNN_EUNSUP (-4)   /* shape not supported by this build */

#define DGCNN_STAT_SLOTS 32
/* Slots of every stats / red buffer prepared by THE CALLING THREAD from now on (thread-local; default DGCNN_STAT_SLOTS; read on
 * the host at launch time and passed to the kernels as an argument, so calls of other threads / streams are not affected).  A producer workgroup adds its partial
 * sums -- themselves formed in a fixed order -- to slot (writer index mod slots) with a double atomic; with slots >= the number of
 * writers (the library then also caps the grids of its reduction kernels at `slots`) every slot has ONE writer, and the finalize
 * kernels add the slots in a fixed order: sums, hence whole training steps, are bit-reproducible run to run at the speed of the
 * default kernels (the host's DETERMINISTIC mode: 768 slots for 49152 rows).  Buffers must be sized for the value in force. */
int dgcnn_set_stat_slots(int n);
int dgcnn_get_stat_slots(void);

/* ---- process-wide switches (csrc/switches.cc): A/B and test switches of the dispatch rules, one table.  Where a row has an
 * environment variable of its own name it is read ONCE, when the table is first touched; afterwards only the calls below and the
 * switch's own setter (documented with the kernels it steers) change a value.  Unlike the slot count above they are shared by all
 * threads; values are atomic ints, so any thread may read or set at any time (a call in flight sees the old or the new value).
 *   DGCNN_KNN_BF16F            0 | 1 | 2 (env: "auto" = 2)            dgcnn_knn_bf16_filter
 *   DGCNN_KNN_FORCE_VALU       0 | 1 (no env)                         dgcnn_knn_force_valu
 *   DGCNN_KNN_TIGHTEN_EVERY    0 (per-form default: 4 / 8) or a power of two: the append-form scan tightens its bound every n-th tile
 *   DGCNN_KNN_BIG_K_MIN        1 ... 65                               dgcnn_knn_big_k_min
 *   DGCNN_KNN_SEED_MIN_N       -1 (the rule) or a cloud size          dgcnn_knn_seed_min_n
 *   DGCNN_KNN_APPEND           0 | 1                                  dgcnn_knn_append
 *   DGCNN_KNN_APPEND_NPR_LX    1 | 3, the N < 8192 form               dgcnn_knn_append_products (env DGCNN_KNN_APPEND_NPR="<lx>,<big>")
 *   DGCNN_KNN_APPEND_NPR_BIG   1 | 3, the N >= 8192 form              (the same setter and variable)
 *   DGCNN_KNN_HIST             0 | 1 | 2 | 4                          dgcnn_knn_hist
 *   DGCNN_KNN_WIDE_MIN_C       5 ... 129                              dgcnn_knn_wide_min_c
 *   DGCNN_KNN_GRID             0 | 1 | 2 (env: only a leading 0 = 0)  dgcnn_knn_grid
 *   DGCNN_KNN_GRID_MIN_N       DGCNN_SWITCH_UNSET or a size: the dense cell grid's smallest N (unset: 4096) and the packed towers'
 *                              smallest mean cloud size (unset: 16384)
 *   DGCNN_KNN_MIX_MIN_N        >= 0                                   dgcnn_knn_seg_mix_min_n
 *   DGCNN_EDGE_VALU            0 | 1 (env: only a leading 0 = 0)      dgcnn_edge_valu
 *   DGCNN_GEMM_ARITH           0 | 1 | 6 | 9 (env: f32 | bf16x1 ...)  dgcnn_gemm_set_arith / dgcnn_gemm_get_arith
 *   DGCNN_GEMM_X3_TILE         0 | 128 | 256 | 448 | 512 (no env)     dgcnn_gemm_x3_tile_override
 *   DGCNN_EVENT_FLAGS          hipEventCreateWithFlags flags (as the int of the same bits) of the cross-stream wait events; a new
 *                              value only affects events created afterwards (the eager ring of 16 and the waits of plans recorded later)
 * dgcnn_switch_get: *value = the value in force; nothing is changed.  dgcnn_switch_set: the validation of the row's environment
 * parse -- a value the parse would have replaced (BIG_K_MIN = 99 reads as 65 from the environment) is refused, not replaced.  Both:
 * DGCNN_EINVAL for an unknown name (dgcnn_last_error lists the known ones). */
#define DGCNN_SWITCH_UNSET (-2147483647 - 1)
int dgcnn_switch_get(const char* name, int* value);
int dgcnn_switch_set(const char* name, int value);

int dgcnn_version(void);
const char* dgcnn_last_error(void);

/* ---- K1: dgcnn/ops.py:8-19 k_nn --------------------------------------------------------
 * idx[b][i][0..k) = the k smallest D_ij = (s_i + s_j) - 2 <x_i,x_j> of row i (self included),
 * ascending, ties -> lower j.  Arithmetic order is normative (oracle/knn_oracle.c): bit-exact.
 * x: (B,N,C) with row stride ldx.  No (B,N,N) matrix is ever written to HBM.
 * C <= 1024 and k <= 256 in the dense, seeded and packed entries (k <= 40 in the cell-grid and mix entries); DGCNN_EUNSUP beyond,
 *   before any launch.  Rows wider than 128 channels run the channel-slab matrix-pipe scan (csrc/knn_wide.hip): it takes no bound, so
 *   a seed is accepted and ignored there, and its workspace is [s_i | bounds] with no scratch, all of which the call requires
 *   (DGCNN_EINVAL if smaller).
 * 64 < k <= 256, at every width C <= 1024: the large-k scan (csrc/knn_bigk.hip) -- the same distances on the fp32 matrix pipe, no
 *   sorted lists: a candidate whose (D~, j) key is below the row's bound is appended to the row's buffer of 256 (k <= 128) or 512
 *   eight-byte keys, a buffer that fills up is cut back to its k smallest keys, whose largest is the new bound, and one sort per row
 *   at the end writes the indices.  A seed is accepted and ignored.  Its workspace is [s_i | bounds | one count and 256 or 512 keys
 *   per row], all of which the call requires (DGCNN_EINVAL if smaller).
 * Non-finite input (NaN or infinite coordinates, or finite ones whose s_i, s_i + s_j or 2 <x_i,x_j> overflow): the key of candidate
 *   j for row i is (D~_ij, j), D~ = +inf where D_ij is NaN and D_ij otherwise (-inf sorts first); idx[i] = the k smallest keys,
 *   ascending, ties -> lower j, in every kernel form and entry (dense, seeded, packed).  So every row of every cloud holds k DISTINCT
 *   indices of its own cloud whatever x holds: a row with a NaN coordinate holds 0 .. k-1, and a finite row lists candidates at
 *   infinite or NaN distance only when fewer than k are at a finite one, lowest j first, after the finite ones.  What reads idx
 *   (edge gathers, scatters) may index with it unchecked.
 * ws: caller scratch (16-byte aligned) of dgcnn_knn_workspace_bytes(B,N,C,k) bytes: the s_i of ops.py:14 and, for raw
 *   coordinates (C <= 4, k <= 40), the sorted copy / cell table of the exact cell-grid search (csrc/knn_grid.hip: the points of
 *   a cloud are bucketed into a uniform grid and a row only meets the candidates of the cells around its own until its k-th
 *   distance provably beats everything further out -- same pairs' arithmetic, same (D, j) order, same indices); for feature-space
 *   rows (16 < C <= 64) the seed bounds and the per-row candidate buffers of the append-form scan of dgcnn_knn_seeded_f32 (one count
 *   + 256 ... 512 eight-byte entries per row).  A workspace that only holds the s_i (B*N floats rounded up to 256 bytes) selects the
 *   all-pairs, list-keeping kernels. */
int64_t dgcnn_knn_workspace_bytes(int B, int N, int C, int k);
/* 0 = all-pairs kernel for C <= 4 too, 1 (default) = cell grid where it pays (N >= 4096: $DGCNN_KNN_GRID_MIN_N), 2 = cell grid
 * whenever applicable (tests); returns the previous setting ($DGCNN_KNN_GRID=0 switches it off).  Packed towers follow the same
 * modes through dgcnn_knn_seg_grid_use. */
int dgcnn_knn_grid(int mode);
/* A/B switch: 1 = distances by VALU fmaf chains for every C (exact by construction), 0 (default) =
 * v_mfma_f32_32x32x2_f32 for C > 4 (bit-identical on gfx950; the tests compare both).  Returns the
 * previous setting.  The VALU scan has instances for C <= 128 and k <= 64 only: while the switch is on, C > 128 and k > 64 are
 * DGCNN_EUNSUP. */
int dgcnn_knn_force_valu(int on);
/* Smallest C that the channel-slab scan (csrc/knn_wide.hip: fp32 matrix pipe, the channel dimension in slabs of 64, C <= 1024) takes
 * in the dense, seeded and packed entries: 5 ... 129; any other value (-1) only queries.  Default 129: only the widths that no other
 * kernel has an instance for, so every narrower shape launches what it launched before.  C > 128 goes there whatever the value;
 * below, the seeded append-form scan keeps the calls it takes and dgcnn_knn_force_valu(1) keeps every call.  Identical indices either
 * way.  Returns the previous value.  (tools / tests; env DGCNN_KNN_WIDE_MIN_C) */
int dgcnn_knn_wide_min_c(int c);
/* Smallest k that the large-k scan (csrc/knn_bigk.hip) takes in the dense, seeded and packed entries: 1 ... 65; any other value (-1)
 * only queries.  Default 65: only the neighbour counts that no other kernel has an instance for, so every k <= 64 launches what it
 * launched before and dgcnn_knn_workspace_bytes / dgcnn_knn_seg_workspace_bytes answer what they answered before.  k > 64 goes there
 * whatever the value; below, dgcnn_knn_force_valu(1) keeps every call (and refuses k > 64: DGCNN_EUNSUP).  While the value is below
 * 65 the two workspace queries answer the large-k layout for the k it covers, and the entries require it.  Identical indices either
 * way.  Returns the previous value.  (tools / tests; env DGCNN_KNN_BIG_K_MIN) */
int dgcnn_knn_big_k_min(int k);
/* Large feature-space graphs (16 < C <= 64, C % 4 == 0, 16-byte aligned rows): approximate distances from the two leading bf16
 * terms of every operand on the bf16 matrix pipe with a rigorous error bound as a conservative filter, the normative fp32 fmaf
 * chain only for the survivors -- the same indices, bit for bit.  mode 0 = never, 1 = whenever applicable, 2 (default) = for
 * N >= 8192 and wherever a seed bound exists ($DGCNN_KNN_BF16F = 0 | 1 | auto).  Returns the previous mode. */
int dgcnn_knn_bf16_filter(int mode);
int dgcnn_knn_f32(const float* x, int B, int N, int C, int64_t ldx, int k, int32_t* idx,
                  void* ws, size_t ws_bytes, void* stream);
/* The same search with a per-row upper bound taken from `seed` (B, N, >= kseed int32, row stride ldseed): kseed >= k DISTINCT
 * candidates of every row -- in the EdgeConv stack the previous layer's graph (ops.py:95-96).  Their largest distance bounds the
 * row's k-th distance before the scan starts: feature-space rows (16 < C <= 64) then run the append-form scan (no sorted lists: a
 * candidate under the bound is appended to the row's buffer, one selection per row at the end), other shapes filter their list
 * inserts with it.  Identical result (csrc/knn.hip).  seed == NULL or kseed < k: plain dgcnn_knn_f32.  Workspace as
 * dgcnn_knn_workspace_bytes says. */
int dgcnn_knn_seeded_f32(const float* x, int B, int N, int C, int64_t ldx, int k, const int32_t* seed, int64_t ldseed,
                         int kseed, int32_t* idx, void* ws, size_t ws_bytes, void* stream);
/* smallest N for which the seeds are used; -1 = the library's rule (always where the append-form scan applies -- 16 < C <= 64,
 * C % 4 == 0 -- else from 4096 on: below, computing the bound costs the list-keeping kernels what it saves); n < -1 only queries.
 * Returns the previous value.  (tools / tests) */
int dgcnn_knn_seed_min_n(int n);
/* 1 (default) / 0: seeded searches of feature-space rows (16 < C <= 64) run the append-form scan (candidates under the seed bound are
 * appended to a per-row buffer, one selection per row at the end: csrc/knn.hip) / keep per-lane sorted lists; on < 0 only queries.
 * Identical indices either way.  Returns the previous setting.  (tools / tests; env DGCNN_KNN_APPEND) */
int dgcnn_knn_append(int on);
/* Products of the append-form scan's bf16 filter: 1 (default since round 6: plain bf16 operands, margin 2^-6 (s_i + s_j)) or 3 (two bf16
 * terms per operand, margin 2^-13 (s_i + s_j)); any other n only queries.  Identical indices either way (survivors of the filter get
 * their normative distance).  Returns the previous setting.  (tools / tests; env DGCNN_KNN_APPEND_NPR="<N < 8192>,<N >= 8192>") */
int dgcnn_knn_append_products(int n);
/* Raw-coordinate rows (C <= 4) below the cell grid's range: a histogram pass over every `stride`-th candidate (half-octave bins of the
 * normative distance) bounds every row's k-th distance before the scan starts, so that ~1.3 k candidates reach the sorted lists instead
 * of ~k (1 + ln(N / k)) per list.  stride 0 = off, 1 / 2 (default) / 4; any other value only queries.  Identical indices either way.
 * Returns the previous setting.  (tools / tests; env DGCNN_KNN_HIST) */
int dgcnn_knn_hist(int stride);
/* Packed tower: nseg clouds of different sizes concatenated row-wise, cloud b = rows [seg_off[b], seg_off[b + 1]) of x (rows, C),
 * seg_off (device, nseg + 1 int32) strictly increasing from 0 to rows.  Every row searches its own cloud only; idx (rows, k) holds
 * TOWER rows (seg_off[b] + j).  Per cloud the result is dgcnn_knn_f32 of that cloud alone, bit for bit (same order, self included,
 * ties -> lower row).  min_n / max_n: the smallest / largest cloud (host-known; they choose the kernel forms); k <= min_n.
 * seed (rows, >= kseed, row stride ldseed) or NULL: an earlier packed graph of the same tower (tower rows); a seed outside the
 * query row's cloud invalidates that row's bound (the row is searched without one).  Workspace: dgcnn_knn_seg_workspace_bytes. */
int64_t dgcnn_knn_seg_workspace_bytes(int rows, int max_n, int C, int k);
int dgcnn_knn_seg_f32(const float* x, int64_t ldx, int C, int k, int nseg, const int32_t* seg_off, int rows, int min_n, int max_n,
                      const int32_t* seed, int64_t ldseed, int kseed, int32_t* idx, void* ws, size_t ws_bytes, void* stream);
/* The same packed search for raw coordinates (C <= 4, k <= 40) through the exact cell grid of csrc/knn_grid.hip: one uniform grid per
 * cloud (its cell count from the cloud's own size), every row walks the rings of cells around its own until its k-th distance
 * provably beats everything further out -- ~22 k candidates per row whatever the cloud's size, where dgcnn_knn_seg_f32 scans all n_b
 * rows of the cloud.  Same pairs' arithmetic, same (D, j) order: idx is dgcnn_knn_seg_f32's, bit for bit.  No seed (the grid needs
 * none).  DGCNN_EINVAL for C > 4, k > 40, k > min_n, nseg outside [1, 65535], a null pointer, a misaligned workspace or one
 * smaller than dgcnn_knn_seg_grid_workspace_bytes(rows, nseg) = the s_i of every row + 24 bytes per row (sorted records, s_j,
 * original indices) + one cell table (16^3 + 1 int32) and one 64-byte grid description per cloud.
 * dgcnn_knn_seg_grid_use: host only (no GPU call) -- 1 when the library's rule sends this tower through the grid: dgcnn_knn_grid
 * mode 2 = whenever C <= 4 and k <= 40, mode 1 = also sum_n2 / rows >= 4096 ($DGCNN_KNN_GRID_MIN_N), sum_n2 = sum of n_b^2: the
 * row-weighted mean cloud size, i.e. the candidates per row of the all-pairs scan (N for a dense tower: the dense rule), mode 0 =
 * never.  dgcnn/_engine.py:knn_packed asks it and calls this entry or dgcnn_knn_seg_f32. */
int64_t dgcnn_knn_seg_grid_workspace_bytes(int rows, int nseg);
int dgcnn_knn_seg_grid_f32(const float* x, int64_t ldx, int C, int k, int nseg, const int32_t* seg_off, int rows, int min_n, int max_n,
                           int32_t* idx, void* ws, size_t ws_bytes, void* stream);
int dgcnn_knn_seg_grid_use(int C, int k, int nseg, int rows, int min_n, int max_n, int64_t sum_n2);
/* The same packed search for raw coordinates (C <= 4, k <= 40) with every cloud in the search that suits its own size, in ONE call:
 * cloud_list (device, nseg int32) names every cloud of the tower once -- the n_grid clouds of the grid class first, then the
 * nseg - n_grid clouds of the scan class, each part ascending.  The grid class goes through the cell grid of dgcnn_knn_seg_grid_f32,
 * launched over its n_grid clouds only (grid_max_n: its largest cloud); the scan class through the all-pairs scan with the histogram
 * bound of dgcnn_knn_seg_f32, launched over its clouds only (scan_min_n / scan_max_n: its smallest / largest cloud; the bound needs
 * scan_min_n >= 4 k stride, as there).  Same kernels, same pairs' arithmetic, same (D, j) order: idx is the two other entries', bit
 * for bit.  0 < n_grid < nseg -- a tower of one class belongs to one of the two other entries.  The list's contents are trusted, as
 * seg_off is.  DGCNN_EINVAL, before any launch, for a null pointer, C > 4, k > 40, k > scan_min_n, n_grid outside (0, nseg), sizes
 * that do not fit `rows`, a misaligned workspace or one smaller than dgcnn_knn_seg_mix_workspace_bytes(rows, n_grid) = the s_i of
 * every row and one bound per row (each rows floats rounded up to 256 bytes) + 24 bytes per row (sorted records, s_j, original
 * indices) + one cell table (16^3 + 1 int32) and one 64-byte grid description per GRID cloud (+ 256): it grows with n_grid, not with
 * nseg. */
int64_t dgcnn_knn_seg_mix_workspace_bytes(int rows, int n_grid);
int dgcnn_knn_seg_mix_f32(const float* x, int64_t ldx, int C, int k, int nseg, const int32_t* seg_off, int rows,
                          const int32_t* cloud_list, int n_grid, int grid_max_n, int scan_min_n, int scan_max_n, int32_t* idx, void* ws,
                          size_t ws_bytes, void* stream);
/* The per-cloud size from which a cloud of a packed tower goes to the grid class in dgcnn_knn_grid mode 1 (dgcnn/_engine.py:knn_packed
 * splits the tower and calls dgcnn_knn_seg_mix_f32 when both classes are non-empty); 0 = the mix is off and the whole tower follows
 * dgcnn_knn_seg_grid_use; n < 0 only queries.  Returns the previous value.  Initialised once from $DGCNN_KNN_MIX_MIN_N if set, else
 * from the library's default. */
int dgcnn_knn_seg_mix_min_n(int n);
/* ---- K1 between TWO point sets (csrc/knn_cross.hip): for every row of a query set q the k nearest rows of a separate candidate set p
 * of the same cloud b -- PyG's knn(x, y, k) beside the knn_graph of the entries above.
 * idx[(first query row of cloud b) + i][0..k) = the k smallest keys (D~_ij, j) over the candidates j of cloud b, ascending, ties -> lower
 * j; D_ij = (s_i + s_j) - 2 <q_i,p_j> in K1's normative arithmetic (s = the sequential sum of squares of the row, the product an fmaf
 * chain over the channels ascending), D~ = +inf where D is NaN, -inf sorts first: K1's non-finite rule, so every row holds k DISTINCT
 * rows of its own candidate cloud whatever q and p hold.  The candidate set is not assumed to be the query set: there is no "self
 * included" rule; called with q == p (same rows, same map) the result is dgcnn_knn_f32's / dgcnn_knn_seg_f32's, bit for bit.
 * dist: NULL, or (q_rows, k) floats: the selected D~ in the order of idx (+inf where a candidate at D~ = +inf fills the row).
 * Dense call: q_off == p_off == NULL, nseg = B clouds of max_m query rows (q: (B, max_m, C), row stride ldq) and max_n = min_n
 *   candidate rows (p: (B, max_n, C), row stride ldp) each, q_rows = B max_m, p_rows = B max_n; idx holds cloud-local j.
 * Packed call: q_off and p_off (device, nseg + 1 int32 each) strictly increasing from 0 to q_rows / p_rows: cloud b = query rows
 *   [q_off[b], q_off[b + 1]) against candidate rows [p_off[b], p_off[b + 1]); idx holds rows of the candidate TOWER (p_off[b] + j).
 *   max_m = the largest query cloud, min_n / max_n = the smallest / largest candidate cloud (host-known, as in dgcnn_knn_seg_f32).
 * 1 <= C <= 1024, 1 <= k <= 64 and k <= min_n, nseg in [1, 65535].  The fp32 matrix-pipe scan of csrc/knn_wide.hip with two operand
 *   sources; rows of at most 16 channels (raw coordinates) walk 16-channel slabs instead of 64-channel ones.  The large-k scan
 *   (64 < k <= 256), seeds, the bf16 filter and the cell grid search a cloud against itself only: k > 64 here is DGCNN_EUNSUP.
 * DGCNN_EUNSUP for k > 64 or C > 1024; DGCNN_EINVAL for a null q, p, idx or ws, exactly one of q_off / p_off null, k < 1 or k > min_n,
 *   sizes that do not fit (dense: q_rows != nseg max_m, p_rows != nseg max_n, min_n != max_n), a misaligned workspace or one smaller
 *   than dgcnn_knn_cross_workspace_bytes(q_rows, p_rows) = [s of every query row | s of every candidate row], each rows floats rounded
 *   up to 256 bytes (ws 16-byte aligned).  Every refusal happens before any launch, with the reason in dgcnn_last_error. */
int64_t dgcnn_knn_cross_workspace_bytes(int q_rows, int p_rows);
int dgcnn_knn_cross_f32(const float* q, int64_t ldq, const float* p, int64_t ldp, int C, int k, int nseg, const int32_t* q_off,
                        const int32_t* p_off, int q_rows, int p_rows, int max_m, int min_n, int max_n, int32_t* idx, float* dist,
                        void* ws, size_t ws_bytes, void* stream);

/* ---- K6: feature interpolation between two point sets (csrc/interp.hip) -- PointNet++ feature propagation, PyG's knn_interpolate:
 * y(query i) = the inverse-distance-weighted mean of the feature rows of its k nearest candidates, from the (idx, dist) pair that
 * dgcnn_knn_cross_f32 returns.  NORMATIVE arithmetic: row i has the entries (j_m, D_m), m = 0 ... k-1, in the order the search
 * returned them; every product, sum and quotient below is rounded to fp32 once, nothing is fused or reassociated, `/` is the
 * correctly rounded division:
 *     w_m = (D_m < +inf) ? 1.0f / fmaxf(D_m, eps) : 0.0f      +inf and NaN give 0; D_m <= eps (also negative, -inf) gives 1 / eps
 *     W   = w_0;  W = W + w_m                      for m = 1 ... k-1, ascending
 *     a_m = (W > 0) ? w_m / W : 0.0f               a row whose k distances are all +inf: every a_m = 0, y_i = 0, no gradient
 *     y_i[f] = a_0 * feat[j_0][f];  y_i[f] = y_i[f] + a_m * feat[j_m][f]     for m = 1 ... k-1, ascending
 *   backward, with the edge id e = i * k + m (the gradient of the FEATURES only: coordinates and weights carry none, as the k-NN has
 *   no backward here and PyG takes the weights under no_grad):
 *     g_j[f] = 0;  g_j[f] = g_j[f] + a_e * dy_i[f]            over the edges e whose candidate row is j, in ASCENDING e
 *     dfeat_j[f] = g_j[f] (beta = 0; a row nobody interpolates from gets 0)   or   dfeat_j[f] + g_j[f] (beta = 1)
 *   No float atomics: one form, the same bits run to run, in every mode.  Non-finite features propagate as the expressions say
 *   (0 * inf = NaN).  The distances carry K1's absolute error of about 2^-23 (s_i + s_j), so the weights of near-coincident points
 *   are noisy: inherited from the search, not corrected here.
 * feat (p_rows, F; row stride ldf), idx / dist (q_rows, k) dense, y (q_rows, F; row stride ldy: a column slice of a wider buffer is
 *   fine).  M > 0: dense towers -- the candidate row of entry (i, m) is (i / M) * N + idx[i][m] (idx cloud-local; q_rows = B M and
 *   p_rows = B N).  M == 0 (then N == 0): idx holds rows of the candidate tower, what the packed search returns.  The contents of idx
 *   are trusted (the search guarantees k distinct rows of the query's own cloud).
 * a: NULL, or (q_rows, k) floats that receive the normalised weights a_m -- what the backward reads.
 * eps: the clamp of the distance (PyG: 1e-16); finite and at least 1e-30, so that k / eps cannot overflow.
 * 1 <= k <= 64; F % 4 == 0, F <= 1024; 16-byte aligned feat, y, dy, dfeat, ws; leading dimensions % 4 == 0 and >= F;
 *   q_rows k < 2^31.  The forward works the k weights of a row out once (not once per channel lane) and writes no (q_rows, k, F) tensor.
 * Backward workspace, dgcnn_interp_bwd_workspace_bytes(q_rows, p_rows, k) (0 for sizes the entry refuses) =
 *   [off: p_rows + 1 int32 | counts: p_rows int32 | rev: q_rows k int32 | rev in ascending order: q_rows k int32],
 *   each part rounded up to 256 bytes: the transposed adjacency of the bipartite graph by integer counting sort (integer atomics
 *   only); every edge is then placed by the number of smaller edge ids in its bucket, which reads deg_j words per edge -- sum of
 *   deg_j^2 in all, q_rows k * (q_rows k / p_rows) on average, quadratic in the heaviest bucket.
 * DGCNN_EUNSUP for k > 64, F % 4 != 0, F > 1024 or q_rows k >= 2^31; DGCNN_ENOSPC for a workspace that is too small; DGCNN_EINVAL for
 *   a null pointer (a excepted in the forward), k < 1, F < 1, rows < 1, a leading dimension below F or not a multiple of 4, a
 *   misaligned base, eps outside [1e-30, +inf), M > 0 with q_rows % M != 0 or p_rows != (q_rows / M) N, M == 0 with N != 0, beta
 *   outside {0, 1}.  Every refusal happens before any launch, with the reason in dgcnn_last_error. */
int dgcnn_interp_f32(const float* feat, int64_t ldf, const int32_t* idx, const float* dist, int q_rows, int p_rows, int M, int N,
                     int k, int F, float eps, float* a, float* y, int64_t ldy, void* stream);
int64_t dgcnn_interp_bwd_workspace_bytes(int q_rows, int p_rows, int k);
int dgcnn_interp_bwd_f32(const float* dy, int64_t lddy, const int32_t* idx, const float* a, int q_rows, int p_rows, int M, int N,
                         int k, int F, float* dfeat, int64_t lddf, int beta, void* ws, size_t ws_bytes, void* stream);

/* ---- K7: farthest point sampling, the row take and its backward (csrc/fps.hip) -- the downsampling half of a hierarchical point
 * network (PointNet++ set abstraction, PyG's fps): the producer of the second point set of dgcnn_knn_cross_f32 / dgcnn_interp_f32.
 * NORMATIVE arithmetic, for one cloud of n rows and C channels sampled m times (1 <= m <= n); every operation is rounded to fp32 once,
 * nothing is fused or reassociated:
 *     bad_i   = row i holds a coordinate that is not finite (NaN, +inf or -inf)
 *     mind_i  = bad_i ? 0.0f : +inf                                  for every row i
 *     D(i, s) : t = x_i[0] - x_s[0]; D = t * t;  then t = x_i[c] - x_s[c]; D = D + t * t     for c = 1 ... C-1, ascending
 *     s_0     = start (cloud-local; 0 when no start is given; a start outside [0, n) counts as 0)
 *     step j = 0 ... m-1:
 *         idx[j]  = s_j;   dist[j] = mind_{s_j} as it stands at this moment (+inf for an ordinary start row)
 *         mind_i  = (D(i, s_j) < mind_i) ? D(i, s_j) : mind_i        for every row i (a NaN or +inf D lowers nothing)
 *         mind_{s_j} = -1.0f                                          a selected row is never selected again
 *         s_{j+1} = the row with the largest mind; ties -> the LOWER row index
 *   What follows from these rules:
 *   - the result is m DISTINCT rows of the cloud, whatever the input holds;
 *   - bad rows are chosen only after every finite row that is not a duplicate of a selected one; such duplicates tie with the bad rows
 *     at mind = 0, lower index first.  A bad row does not disturb the others: its D is NaN or +inf towards every row, in both roles;
 *   - the first m' entries of an m-sample are the m'-sample (prefix property);
 *   - duplicates of a selected point sit at mind = 0;
 *   - mind is never -0.0 (t * t is +0.0 or larger, or NaN) and never NaN, so the non-negative floats and +inf order as their bit
 *     patterns: a kernel may reduce on an integer key, provided the selected-row sentinel maps below every real value.
 *   dist[j] for j >= 1 is the squared distance of sample j to the samples before it (the coverage radius after j samples, squared).
 * x: rows of C floats, row stride ldx >= C, no alignment beyond 4 bytes (raw coordinates have C = 3).
 * Dense call: x_off == s_off == NULL, nseg clouds of max_n rows and max_m samples each, rows = nseg max_n, samples = nseg max_m; idx
 *   (samples int32) holds cloud-local rows.
 * Packed call: x_off and s_off (device, nseg + 1 int32 each) strictly increasing from 0 to rows / samples: cloud b = rows
 *   [x_off[b], x_off[b + 1]) sampled s_off[b + 1] - s_off[b] times; idx holds rows of the TOWER.  max_n / max_m = the host-known largest
 *   cloud and largest sample count.  A cloud asked for more samples than it has rows cannot be seen on the host by this entry (the
 *   Python layer refuses it from its host offsets): the kernel clamps it to n samples and writes -1 into the rest of idx (and dist).
 * start: NULL, or nseg device int32 of cloud-local rows.  dist: NULL, or samples floats.
 * 1 <= C <= 64, nseg in [1, 65535].  One workgroup of 1024 threads per cloud, in one of two forms chosen per cloud from its own n:
 *   resident  (C <= 4 and n <= dgcnn_fps_resident_max_n(C) = 16384): coordinates and mind in registers, one barrier per step;
 *   streaming (everything else): coordinates re-read every step, mind in the workspace.
 *   No workgroup waits for another one.  No host synchronisation, no read-back; one launch for a dense call, at most two (one per form) for a
 *   packed one.
 * dgcnn_fps_resident_max_n(C): the largest cloud the resident form takes for that C, 0 where it takes none.
 * dgcnn_fps_workspace_bytes(rows, C, max_n): rows floats rounded up to 256 bytes when some cloud of the call can need the streaming
 *   form (max_n > dgcnn_fps_resident_max_n(C)), else 0 (ws may then be NULL); 0 also for sizes the entry refuses.
 * DGCNN_EINVAL for a null x / idx, exactly one of x_off / s_off null, non-positive sizes, dense sizes that do not multiply out,
 *   max_m > max_n, ldx < C, a missing or misaligned (16 bytes) workspace where one is needed; DGCNN_EUNSUP for C > 64 or nseg > 65535;
 *   DGCNN_ENOSPC for a workspace that is too small.  Every refusal happens before any launch, with the reason in dgcnn_last_error. */
int dgcnn_fps_resident_max_n(int C);
int64_t dgcnn_fps_workspace_bytes(int rows, int C, int max_n);
int dgcnn_fps_f32(const float* x, int64_t ldx, int C, int nseg, const int32_t* x_off, const int32_t* s_off, int rows, int samples,
                  int max_n, int max_m, const int32_t* start, int32_t* idx, float* dist, void* ws, size_t ws_bytes, void* stream);
/* The row take and its backward.  row(s) = (s / M) * N + idx[s] for M > 0 (dense: idx cloud-local, s_rows = B M, x_rows = B N), and
 * idx[s] for M == N == 0 (idx holds tower rows) -- what dgcnn_fps_f32 returns in its two call forms.
 * gather:  y[s][0..F) = x[row(s)][0..F).
 * scatter: beta = 0: dx = 0 everywhere (x_rows rows of F), then dx[row(s)] = dy[s];  beta = 1: dx[row(s)] = dx[row(s)] + dy[s].
 *   The rows of idx are TRUSTED TO BE DISTINCT (per cloud), as farthest point sampling guarantees: every dx row has at most one
 *   writer, so there are no atomics and one result run to run.  With repeated rows the scatter keeps one of the writers.
 * Any F >= 1; leading dimensions >= F.  A float4 path when F % 4 == 0, both leading dimensions % 4 == 0 and both bases are 16-byte
 *   aligned; a scalar path otherwise (coordinates have F = 3).  The contents of idx are trusted to lie inside the cloud.
 * DGCNN_EINVAL for a null pointer, F < 1, rows < 1, negative M / N, M > 0 with s_rows % M != 0 or x_rows != (s_rows / M) N, M == 0
 *   with N != 0, a leading dimension below F, beta outside {0, 1}.  Every refusal happens before any launch. */
int dgcnn_rows_gather_f32(const float* x, int64_t ldx, const int32_t* idx, int s_rows, int x_rows, int M, int N, int F, float* y,
                          int64_t ldy, void* stream);
int dgcnn_rows_scatter_f32(const float* dy, int64_t lddy, const int32_t* idx, int s_rows, int x_rows, int M, int N, int F, float* dx,
                           int64_t lddx, int beta, void* stream);

/* ---- K3 in its bf16-operand form (BASELINE configs[2] "bf16 edge-MLP MFMA"): conv0 of an EdgeConv layer, ops.py:21-52 ------
 * E[e] = [x_i, x_j - x_i] formed in fp32 and rounded to bf16 once (RNE), W0 (2C x F, row-major) rounded to bf16 once,
 * y = E W0 on v_mfma_f32_32x32x16_bf16 with fp32 accumulation; neither E nor y is written by the two forward passes:
 *   dgcnn_edge_mlp_bf16_stats      stats[slot][0][f] += sum_e y[e][f], stats[slot][1][f] += sum_e y[e][f]^2  (double[slots][2][F], zeroed)
 *   dgcnn_edge_mlp_bf16_bn_kreduce z = relu((y - mean) rstd + beta) recomputed; max / mean over the k edges of each point and the
 *                                  number of edges attaining the max (cnt, (B N, F) dense; may be null); pack_cnt = 1: cnt =
 *                                  #ties + 256 #(z > 0), the packing of the fp32 edge kernels (dgcnn_edge_bn_act_kreduce_f32), which
 *                                  dgcnn_edge_bn_bwd_reduce_points_f32 and dgcnn_edge_mlp_bf16_bwd read (k < 256)
 *   dgcnn_edge_mlp_bf16            y written out, (B N k, F) dense -- bit-identical to what the two passes saw
 *   dgcnn_edge_mlp_bf16_bwd        the layer's backward in ONE pass over the edges, y recomputed: red = the slots written by
 *                                  dgcnn_edge_bn_bwd_reduce_points_f32 (reduced here; dbeta = dbeta_beta * dbeta + sum dz);
 *                                  dY = rstd (dz - c1 - xhat c2) rounded to bf16 -> dYb (B N k, F) bf16 and dysum = sum_m dY (B N, F)
 *                                  (either may be null); dW0 (2C, F) += E^T dY on the matrix pipe.  Neither E nor y nor an fp32 dY
 *                                  is written.  ws >= dgcnn_edge_mlp_bf16_bwd_workspace_bytes.  8 <= k <= 128 (C = 64 with F = 128: k >= 9, LDS);
 *                                  dgcnn_edge_mlp_bf16_bwd_supported tells.
 *   dgcnn_edge_gather_sum_bf16     dgcnn_edge_gather_sum_f32 over that bf16 dY (same additions in the same order)
 * Shapes: C <= 4 or C == 64 (x float4-loadable), F in {32, 64, 128}, k <= 128 (dgcnn_edge_mlp_bf16_supported; DGCNN_EUNSUP else). */
int dgcnn_edge_mlp_bf16_supported(int C, int k, int F);
int dgcnn_edge_mlp_bf16_bwd_supported(int C, int k, int F);
int64_t dgcnn_edge_mlp_bf16_bwd_workspace_bytes(int B, int N, int C, int k, int F);
int dgcnn_edge_mlp_bf16_bwd(const float* x, int64_t ldx, const int32_t* idx, const float* W0, int B, int N, int C, int k, int F,
                            const float* mean, const float* rstd, const float* beta, const float* mx, int64_t ldmx,
                            const float* cnt, const float* dmx, int64_t lddmx, const float* dmn, int64_t lddmn, double* red,
                            void* dYb, float* dysum, int64_t lddysum, float* dW0, float* dbeta, float dbeta_beta, void* ws,
                            size_t ws_bytes, void* stream);
int dgcnn_edge_gather_sum_bf16(const void* dY, const int32_t* off, const int32_t* rev, int64_t R, int F, float* S, int64_t lds,
                               void* stream);
/* dst[i] = src[i] rounded to the nearest bf16 value (ties to even), kept as fp32 (weights of the mode's point-level gradient products);
 * a NaN stays a quiet NaN of its sign (also where the rounding add would carry it into the exponent: 0x7fffffff), as does the
 * bf16 rounding of dY in dgcnn_bn_bwd_apply_f32 / dgcnn_edge_bn_bwd_apply_f32 (relu bit 1) */
int dgcnn_round_bf16_f32(const float* src, float* dst, int64_t n, void* stream);
int dgcnn_edge_mlp_bf16(const float* x, int64_t ldx, const int32_t* idx, const float* W0, int B, int N, int C, int k, int F,
                        float* Y, void* stream);
int dgcnn_edge_mlp_bf16_stats(const float* x, int64_t ldx, const int32_t* idx, const float* W0, int B, int N, int C, int k, int F,
                              double* stats, void* stream);
int dgcnn_edge_mlp_bf16_bn_kreduce(const float* x, int64_t ldx, const int32_t* idx, const float* W0, int B, int N, int C, int k,
                                   int F, const float* mean, const float* rstd, const float* beta, float* mx, int64_t ldmx,
                                   float* mn, int64_t ldmn, float* cnt, int pack_cnt, void* stream);

/* ---- K2: dgcnn/ops.py:21-40 edges (gather + tile + sub + concat) ------------------------
 * E[b][i][m][0..C) = x_i ; E[b][i][m][C..2C) = x_{idx[b][i][m]} - x_i.                    */
int dgcnn_edge_gather_f32(const float* x, int64_t ldx, const int32_t* idx, int B, int N, int C, int k,
                          float* E, void* stream);
/* transpose of the above (tf.gather^T = scatter-add, tf.tile^T = sum over k): dx += ...   */
int dgcnn_edge_gather_bwd_f32(const float* dE, const int32_t* idx, int B, int N, int C, int k,
                              float* dx, int64_t lddx, void* stream);

/* ---- K3: dgcnn/ops.py:47-52 slim.conv2d 1x1 on the edge tensor (conv0) --------------------
 * Y[(b,i,m)][f] = sum_c E[(b,i,m)][c] W0[c][f], E gathered on the fly from (x, idx) into the LDS
 * A-tile (never written to HBM); fp32 MFMA; epilogue accumulates per-channel sum / sum-of-squares
 * of Y for the batch-norm statistics (ops.py:53).                                           */
int dgcnn_edge_mlp_f32(const float* x, int64_t ldx, const int32_t* idx, const float* W0,
                       int B, int N, int C, int k, int F, float* Y, double* stats, void* stream);
/* dW0[2C][F] (+)= E^T dY  (split over the edge dimension; ws = workspace)                   */
int dgcnn_edge_mlp_wgrad_f32(const float* x, int64_t ldx, const int32_t* idx, const float* dY,
                             int B, int N, int C, int k, int F, float* dW0, float beta,
                             void* ws, size_t ws_bytes, void* stream);
/* dx[nbr] += dY W0[C:2C]^T (scatter, fp32 atomics); the centre part
 * dx[i] += (sum_m dY[i,m]) (W0[:C]-W0[C:])^T is a plain GEMM issued by the host.            */
int dgcnn_edge_mlp_dgrad_scatter_f32(const float* dY, const float* W0, const int32_t* idx,
                                     int B, int N, int C, int k, int F, float* dx, int64_t lddx,
                                     void* stream);

/* conv0 in FACTORED form (what dgcnn.ops.edge_conv issues): E W0 = x_i (W0[:C]-W0[C:]) + x_j W0[C:].
 * The centre term U[point] = X (Wa-Wb) is one per-point dgcnn_gemm_f32; per edge remains the
 * (B*N*k) x C GEMM of the gathered neighbour rows with Wb = W0[C:], with U added per group of k rows
 * in the epilogue (+ BN column statistics): half the per-edge flops, identical result up to fp32
 * rounding (tests compare both forms).                                                          */
int dgcnn_edge_nbr_gemm_f32(const float* x, int64_t ldx, const int32_t* idx, const float* Wb,
                            const float* U, int64_t ldu, int B, int N, int C, int k, int F,
                            float* Y, double* stats, void* stream);
/* dWb[C][F] (+)= sum_e x_j(e)^T dY[e]; the host adds X^T (sum_m dY) for the centre half.        */
int dgcnn_edge_nbr_wgrad_f32(const float* x, int64_t ldx, const int32_t* idx, const float* dY,
                             int B, int N, int C, int k, int F, float* dWb, float beta,
                             void* ws, size_t ws_bytes, void* stream);

/* Deterministic-shape alternative to the scatter: bucket the edges by target once (transposed
 * adjacency: off[B*N+1], rev[B*N*k]; cnt_ws = 2*B*N int32 scratch) ...                         */
int dgcnn_edge_csr_build(const int32_t* idx, int B, int N, int k, int32_t* cnt_ws, int32_t* off,
                         int32_t* rev, void* stream);
/* ... then S[j][:] = sum over incoming edges e of dY[e][:] (tf.gather^T as a gather); the host
 * finishes with a plain GEMM dx += S W0[C:2C]^T.                                              */
int dgcnn_edge_gather_sum_f32(const float* dY, const int32_t* off, const int32_t* rev, int64_t R, int F,
                              float* S, int64_t lds, void* stream);

/* ---- conv0 of an EdgeConv layer (ops.py:47-52) as point-level GEMM + per-edge gather-add ---------
 * The convolution is linear: [x_i, x_j - x_i] W0 = x_i (Wa - Wb) + x_j Wb with W0 = [Wa ; Wb].  So
 *   Wcat = [Wa - Wb | Wb]              (C x 2F)    dgcnn_edge_weight_split_f32
 *   [U | V] = X Wcat                   (B*N x 2F)  dgcnn_gemm_f32   (k times fewer MACs than the edge tensor product)
 *   Y[b,i,m,:] = V[b, idx[b,i,m], :] + U[b,i,:]    dgcnn_edge_gather_add_f32 (+ BN column sums of Y into stats)
 * backward: dU = sum_m dY (dgcnn_bn_bwd_apply_f32's dYsum), dV = dgcnn_edge_gather_sum_f32(dY);
 *   dWcat = X^T [dU | dV], dX += [dU | dV] Wcat^T (dgcnn_gemm_f32), then
 *   dW0[:C] += dWcat[:, :F] ; dW0[C:] += dWcat[:, F:] - dWcat[:, :F]     dgcnn_edge_wgrad_combine_f32
 * F %% 4 == 0, F <= 1024, 16-byte aligned rows.
 * dgcnn_edge_gather_add_f32 and the dgcnn_edge_bn_* entries below address row idx of a cloud as V + idx * ldv with one 24-bit multiply
 * and a 32-bit unsigned element offset: N < 2^24, ldv < 2^24 and N * ldv < 2^32 (DGCNN_EUNSUP otherwise; nothing is written).  Within
 * that, a row may start 2^31 elements or more past its cloud's first row.  (dgcnn_edge_bn_bwd_apply_wgrad_f32 takes the same range
 * for x and ldx in its exact-width form and falls back to 64-bit offsets outside it.)                                              */
int dgcnn_edge_weight_split_f32(const float* W0, int C, int F, float* Wcat, void* stream);
int dgcnn_edge_gather_add_f32(const float* V, int64_t ldv, const float* U, int64_t ldu, const int32_t* idx,
                              int B, int N, int k, int F, float* Y, double* stats, void* stream);
int dgcnn_edge_wgrad_combine_f32(const float* dWcat, int C, int F, float* dW0, void* stream);
/* Y may be NULL in dgcnn_edge_gather_add_f32 (column sums only).  The three BatchNorm passes below are
 * dgcnn_bn_act_kreduce_f32 / _bwd_reduce_f32 / _bwd_apply_f32 with the k rows of point (b,i) RECOMPUTED as
 * V[b, idx[b,i,m], :] + U[b,i,:] instead of read from a (B*N*k, F) tensor: the forward then writes no edge
 * tensor to HBM at all and the backward only dY (which the transposed-adjacency sum needs).  Same argument
 * meaning as their dense counterparts (see below); dY is (B*N*k, F) dense.                           */
int dgcnn_edge_bn_act_kreduce_f32(const float* V, int64_t ldv, const float* U, int64_t ldu,
                                  const int32_t* idx, int B, int N, int k, int F,
                                  const float* mean, const float* rstd, const float* beta, int relu,
                                  float* max_out, int64_t ldmax, float* mean_out, int64_t ldmean,
                                  float* cnt_out, void* stream);
int dgcnn_edge_bn_bwd_reduce_f32(const float* V, int64_t ldv, const float* U, int64_t ldu,
                                 const int32_t* idx, int B, int N, int k, int F,
                                 const float* mean, const float* rstd, const float* beta, int relu,
                                 const float* dmax, int64_t lddmax, const float* dmean, int64_t lddmean,
                                 const float* mx_in, int64_t ldmx, const float* cnt_in,
                                 double* red, void* stream);
/* The backward BN reduction of a relu conv0 from per-point data only (no pass over the edges): cntpos is the
 * cnt_out of dgcnn_edge_bn_act_kreduce_f32, which for the edge variants holds (#ties of the max) + 256 * (#rows
 * with z > 0) (k < 256); mx / mn are that call's max_out / mean_out.  Fills red like _bwd_reduce_f32.            */
int dgcnn_edge_bn_bwd_reduce_points_f32(const float* mx, int64_t ldmx, const float* mn, int64_t ldmn,
                                        const float* cntpos, const float* dmax, int64_t lddmax,
                                        const float* dmean, int64_t lddmean, const float* beta,
                                        int64_t R, int k, int F, double* red, void* stream);
int dgcnn_edge_bn_bwd_apply_f32(const float* V, int64_t ldv, const float* U, int64_t ldu,
                                const int32_t* idx, int B, int N, int k, int F,
                                const float* mean, const float* rstd, const float* beta, int relu,
                                const float* dmax, int64_t lddmax, const float* dmean, int64_t lddmean,
                                const float* mx_in, int64_t ldmx, const float* cnt_in,
                                double* red, float* dY, float* dYsum, int64_t lddysum, float* dbeta,
                                float dbeta_beta, void* stream);

/* The last FC layer with tf.nn.dropout fused behind it (model.py:88-91): out = dropout(relu?(bn(T)), keep) with the counter-based
 * mask of dgcnn_dropout_dev_f32 (seed read from device memory), and its whole BatchNorm backward (sums, finalise + dbeta, dT in
 * place or not) reading dout = d(dropped output) through the same mask: the activated tensor is never stored undropped and the
 * separate dropout passes (forward and backward) disappear.  T, out, dT: (R, F) contiguous rows of F floats (out: leading dim ldo). */
int dgcnn_bn1_act_dropout_f32(const float* T, int64_t R, int F, const float* mean, const float* rstd, const float* beta,
                              int relu, float keep, const uint64_t* seed_dev, float* out, int64_t ldo, void* stream);
int dgcnn_bn1_bwd_dropout_f32(const float* T, int64_t R, int F, const float* mean, const float* rstd, const float* beta,
                              int relu, float keep, const uint64_t* seed_dev, const float* dout, int64_t lddo, double* red,
                              float* dT, float* dbeta, float dbeta_beta, void* stream);

/* The class-dimension tail (model.py:88-101, trainval.py:39-54): last FC layer (F = 256, dropout behind it) -> Final layer
 * (ncls <= 4 columns, W: its [F][ncls] weight, leading dim ldw) -> softmax / loss, with the Final layer's two class products
 * formed in registers beside the BatchNorm passes.  Each call computes, bit for bit, what the sequence it replaces computes:
 *   dgcnn_bn1_act_class_f32   = dgcnn_bn1_act_dropout_f32 + dgcnn_gemm_f32 (logits = out W, beta 0, with column statistics, on
 *                               that product's grid) + the zero fill of scal = [loss, accuracy] (may be NULL);
 *   dgcnn_bn_softmax_xent_f32 = dgcnn_bn_finalize_f32 (mean, rstd are still written) + dgcnn_bn_act_kreduce_f32 (k = 1, -> fin)
 *                               + dgcnn_softmax_xent_f32 on fin; scal must already be zero;
 *   dgcnn_bn1_bwd_class_f32   = dgcnn_bn_bwd_apply_f32 (k = 1) on the Final layer (red_f: slot 0 filled by
 *                               dgcnn_bn_bwd_reduce_det_f32; dT_final replaces Tf, dbeta_f as there) + dgcnn_gemm_f32
 *                               (d(out) = dT_final W^T, beta 0 -- never stored) + dgcnn_bn1_bwd_dropout_f32 on the FC layer;
 *                               phases: 1 = the sums pass (leaves dT_final in Tf: the Final layer's weight gradient can start),
 *                               2 = finalize + dT, 3 = both. */
int dgcnn_bn1_act_class_f32(const float* T, int64_t R, int F, const float* mean, const float* rstd, const float* beta,
                            int relu, float keep, const uint64_t* seed_dev, float* out, int64_t ldo, const float* W,
                            int64_t ldw, int ncls, float* logits, int64_t ldc, double* stats, float* scal, void* stream);
int dgcnn_bn_softmax_xent_f32(const float* Y, const double* stats, double count, float eps, const float* beta, int relu,
                              int64_t rows, int ncls, float* mean, float* rstd, float* fin, const int32_t* labels,
                              const float* weight, float* softmax, float* dlogits, float* scal, void* stream);
int dgcnn_bn1_bwd_class_f32(const float* T, int64_t R, int F, const float* mean, const float* rstd, const float* beta,
                            int relu, float keep, const uint64_t* seed_dev, float* Tf, int ncls, const float* mean_f,
                            const float* rstd_f, const float* beta_f, int relu_f, const float* dfin, double* red_f,
                            float* dbeta_f, float dbeta_f_beta, const float* W, int64_t ldw, double* red, float* dT,
                            float* dbeta, float dbeta_beta, int phases, void* stream);

/* conv0 backward of a layer whose input needs no gradient and has C <= 4 channels (the first EdgeConv layer: raw coordinates),
 * in ONE pass: dY is formed per edge exactly as in dgcnn_edge_bn_bwd_apply_f32 and consumed on the spot,
 * dW0[2C][F] += [x_i, x_j - x_i]^T dY (ops.py:39-52) -- no dY tensor, no transposed adjacency, no point-level GEMMs.
 * red: the sums of dgcnn_edge_bn_bwd_reduce(_points)_f32 (finalised here; dbeta as in the apply call); relu is implied (conv0).
 * ws >= (<= 1024 blocks) * 2C * F floats.                                                                                    */
int dgcnn_edge_bn_bwd_apply_wgrad_f32(const float* V, int64_t ldv, const float* U, int64_t ldu,
                                      const int32_t* idx, int B, int N, int k, int F,
                                      const float* mean, const float* rstd, const float* beta,
                                      const float* dmax, int64_t lddmax, const float* dmean, int64_t lddmean,
                                      const float* mx_in, int64_t ldmx, const float* cnt_in, double* red,
                                      const float* x, int64_t ldx, int C, float* dW0, float* dbeta, float dbeta_beta,
                                      void* ws, size_t ws_bytes, void* stream);
/* Process switch of the instruction-count forms of the edge-level passes: the register-held max / mean / count walk of
 * dgcnn_edge_bn_act_kreduce_f32 (ReLU, k <= 20) and the exact-width first-layer pass of dgcnn_edge_bn_bwd_apply_wgrad_f32 (C = 3, 4).
 * on = 0: the earlier kernels' code for every shape; on > 0: the new forms where they apply; on < 0 only queries.  Returns the
 * previous value.  Initialised once from $DGCNN_EDGE_VALU (0 = off), else on.  Results are bit-identical either way. */
int dgcnn_edge_valu(int on);

/* ---- plain fp32 MFMA GEMM: every other slim.conv2d 1x1 (ops.py:62-70,125-133,153-160;
 * model.py:46-53,65-72,94-101) and their dgrad / wgrad --------------------------------------
 * C[M][N] = op(A)[M][K] op(B)[K][N] (+ beta*C) (+ gbias[row / rows_per_group][n]);
 * transA: A stored [K][M]; transB: B stored [N][K].  stats (optional): BN sums of C's columns.
 * ws is needed when the library decides to split K (transA, tall reductions).                */
/* Arithmetic of dgcnn_gemm_f32 when its operands are float4-loadable (16-byte aligned, leading dimensions
 * and contiguous extents multiples of 4):  0 = v_mfma_f32_32x32x2_f32 (an fmaf chain, 157 TFLOP/s peak);
 * 6 / 9 = every fp32 operand is split EXACTLY into three bf16 terms and 6 (terms below 2^-23 |a b| dropped)
 * or all 9 partial products run on the bf16 matrix pipe with fp32 accumulation (fp32-class results, see
 * gemm_x3.hip).  1 = only the leading bf16 term of each operand: plain bf16 operands with fp32 accumulation (NOT fp32
 * class: the bf16 edge-MLP mode of BASELINE configs[2]; the host selects it around the EdgeConv conv0 / conv1 products).
 * Operands that are not float4-loadable run the fp32 kernel unrounded in every mode, and the streaming kernels for N <= 4
 * and for K <= 4 never round either: a caller that needs mode 1 there rounds its operands itself (dgcnn_round_bf16_f32).
 * Default 6, or $DGCNN_GEMM_ARITH = f32 | bf16x6 | bf16x9 | bf16x1.  Process-wide.                     */
int dgcnn_gemm_set_arith(int mode);
int dgcnn_gemm_get_arith(void);
/* Rows of the output tile the bf16-split GEMM picks for an (M,N,K) product: 64 | 128 | 256 (256 = the wave-specialised
 * gemm_x3w2_kernel).  For tools that name kernel instances (bench.py's per-kernel table); no effect on results. */
/* row tiles (= workgroups that add column sums into `stats`) of the dgcnn_gemm_f32 launch with these operands (transA = 0); 0 when
 * the launch sizes its grid from the slot count by itself.  The host picks the slot count of that buffer from it (deterministic mode). */
int dgcnn_gemm_stat_writers(int transB, int M, int N, int K, const float* A, int64_t lda, const float* B, int64_t ldb);
int dgcnn_gemm_x3_tile_rows(int M, int N, int K);
/* 256 when the product runs on a 256-column kernel (gemm_x3q_kernel: 256 x 256 or 192 x 256 tiles, rows from the call above), else 0 */
int dgcnn_gemm_x3_tile_cols(int M, int N, int K);
/* tools: force the 128- / 256-row tile of the bf16-split kernels (0 = the automatic rule); returns the previous setting */
int dgcnn_gemm_x3_tile_override(int bm);
/* colmax_keys (optional, uint64[M / colmax_rows_per_group][N], zeroed): the per-group column maximum of C and its FIRST row
 * (model.py:76-77: max-pool over the points of a cloud, taken in the epilogue of the GEMM that produces the tensor), as packed
 * keys decoded by dgcnn_colmax_decode_f32 -> value[g][n], row-in-group[g][n].  rows_per_group % 256 == 0, no transA.       */
int dgcnn_gemm_f32(int transA, int transB, int M, int N, int K,
                   const float* A, int64_t lda, const float* B, int64_t ldb,
                   float* C, int64_t ldc, float beta,
                   const float* gbias, int64_t ldgbias, int rows_per_group,
                   double* stats, void* colmax_keys, int colmax_rows_per_group,
                   void* ws, size_t ws_bytes, void* stream);
int dgcnn_colmax_decode_f32(const void* keys, int64_t n, float* vals, int32_t* arg, void* stream);
/* dgcnn_gemm_f32 for a PACKED tower (clouds of different sizes concatenated row-wise): the per-cloud bias row of output row r
 * is gbias[row_group[r]] (row_group: int32[M], the row -> cloud map) instead of gbias[r / rows_per_group].  Same kernels, tiles and
 * arithmetic as dgcnn_gemm_f32: C equals the product without bias plus that one fp32 add, and the column statistics include the
 * bias.  No column-maximum epilogue (a row tile may straddle clouds: dgcnn_colmax_seg_f32); no bias with transA.              */
int dgcnn_gemm_seg_f32(int transA, int transB, int M, int N, int K,
                       const float* A, int64_t lda, const float* B, int64_t ldb,
                       float* C, int64_t ldc, float beta,
                       const float* gbias, int64_t ldgbias, const int32_t* row_group,
                       double* stats, void* ws, size_t ws_bytes, void* stream);

/* ---- GEMM from PRE-SPLIT operand planes (gemm_pl.hip) -------------------------------------------
 * The same 1x1 convolutions and their dgrad / wgrad (ops.py:62-70,153-160; model.py:65-72) when the
 * operands were split into 16-bit planes ONCE by their producer instead of inside every GEMM tile.
 * Plane set of a tensor X (rows x cols):  element (row, c) of plane p at
 *     base + p * plane_stride + ((c / 8) * rows_alloc + row) * 16 + (c % 8) * 2        [bytes]
 * rows_alloc = rows rounded up to 64, pad rows are zero.
 *   DGCNN_PLANES_F16X2 : x * scale = h1 + h2 (2 fp16 planes; scale = a power of two read from scale_dev, chosen so that
 *                        max |x| * scale < 2^15: dgcnn_planes_scale_f32 or a producer's analytic bound), 3 partial products;
 *                        the GEMM divides its result by scale_A * scale_B (device scalars, exact).
 * dgcnn_split_planes_f32: plane element (row, c) = src[row * row_stride + c * col_stride]  (col_stride 1 = an activation
 *   view; row_stride 1 = the transpose of a row-major matrix, for weights).
 * dgcnn_gemm_planes_f32:  C[M][N] (+= beta C) = sum_k A(m,k) B(n,k)
 *   DGCNN_PL_KC: A has M rows, B has N rows, the reduction runs over the K channels of both (K % 32 == 0); A / B point at the
 *                first octet of the channel range;   DGCNN_PL_TR: A has M channels, B has N channels (M, N % 16 == 0), the
 *                reduction runs over the K rows of both (X^T dY; split over K into ws).  gbias / stats as dgcnn_gemm_f32 (KC only). */
/* (format 0, three bf16 planes / 6 partial products, existed in round 3: slower than the in-kernel split, removed) */
#define DGCNN_PLANES_F16X2 1
#define DGCNN_PL_KC 0
#define DGCNN_PL_TR 1
int dgcnn_planes_scale_f32(const float* src, int64_t ld, int64_t rows, int cols, float bound_mul, float* scale_dev,
                           void* ws, void* stream);
int dgcnn_split_planes_f32(const float* src, int64_t row_stride, int64_t col_stride, int64_t rows, int cols, int fmt,
                           const float* scale_dev, void* dst, int64_t plane_stride, int64_t rows_alloc, void* stream);
int dgcnn_gemm_planes_f32(int form, int fmt, int M, int N, int K,
                          const void* A, int64_t a_plane_stride, int64_t a_rows_alloc,
                          const void* B, int64_t b_plane_stride, int64_t b_rows_alloc,
                          const float* a_scale_dev, const float* b_scale_dev,
                          float* C, int64_t ldc, float beta,
                          const float* gbias, int64_t ldgbias, int rows_per_group,
                          double* stats, void* colmax_keys, int colmax_rows_per_group,
                          void* ws, size_t ws_bytes, void* stream);

/* ---- BatchNorm passes that WRITE operand planes (planes_bn.hip) ------------------------------------
 * The per-point conv + BN + ReLU layers of the head (model.py:65-72, ops.py:153-160): the pass that normalises a GEMM
 * output writes the planes the next plane GEMM reads; the backward-apply pass writes dT as planes.
 * dgcnn_param_scales_f32: scales[0] = power-of-two scale of every activation plane set of the step, from the bound
 *   |z| <= act_mul (sqrt(rows_max) + max |parameter|) that holds for any batch-normalised tensor; scales[1] = scale of the
 *   weight plane sets (max |parameter|).  ws = 4 bytes.
 * dgcnn_bn_act_planes_f32: z = relu?((T - mean) rstd + beta) -> planes (pad rows zero) and, optionally, fp32 copies.
 * dgcnn_bn1_bwd_reduce_max_f32: red[slot][0/1][F] += column sums of dz, dz xhat; maxbits[0/1][F] = max |dz|, max |xhat| (uint bits;
 *   maxbits has 2 F + 1 zeroed words, the last one receives the tensor-wide bound in the apply call).
 * dgcnn_bn1_bwd_apply_planes_f32: finalises red (slot 0 <- sums; dbeta; maxbits is overwritten by the two column means), bounds |dT| per column from the maxima, writes the
 *   plane set's power-of-two scale to scale_dev and dT = rstd (dz - c1 - xhat c2) as planes (+ optional fp32 dT, + optional
 *   per-group column sums gsum[row / rows_per_group][F], rows_per_group % 64 == 0). */
int dgcnn_param_scales_f32(const float* params, int64_t n, double rows_max, float act_mul, float* scales, void* ws, void* stream);
int dgcnn_bn_act_planes_f32(const float* T, int64_t ldt, int64_t R, int F, const float* mean, const float* rstd,
                            const float* beta, int relu, int fmt, const float* scale_dev, void* planes,
                            int64_t plane_stride, int64_t rows_alloc, float* out, int64_t ldo, float* out2, int64_t ldo2,
                            void* stream);
int dgcnn_bn1_bwd_reduce_max_f32(const float* T, int64_t R, int F, const float* mean, const float* rstd,
                                 const float* beta, int relu, const float* dout, int64_t lddo, double* red,
                                 void* maxbits, void* stream);
int dgcnn_bn1_bwd_apply_planes_f32(const float* T, int64_t R, int F, const float* mean, const float* rstd,
                                   const float* beta, int relu, const float* dout, int64_t lddo, double* red,
                                   void* maxbits, int fmt, float* scale_dev, void* planes, int64_t plane_stride,
                                   int64_t rows_alloc, float* dT, float* gsum, int64_t ldgsum, int rows_per_group,
                                   float* dbeta, float dbeta_beta, void* stream);

/* ---- K4/K5: slim.batch_norm (ops.py:53,68 ...) + activation + reduce_max/mean (ops.py:56-57)
 * mean/rstd from the stats slots: mean = S/count, var = Q/count - mean^2 (double), rstd=1/sqrt(var+eps) */
int dgcnn_bn_finalize_f32(const double* stats, int F, double count, float eps,
                          float* mean, float* rstd, void* stream);
/* z = (Y - mean)*rstd + beta ; relu? ; over the k rows of each of the R points:
 * max_out[r][f] = max_m z, mean_out[r][f] = (sum_m z)/k.  k = 1: out = act(bn(Y)) -> max_out
 * (mean_out may be NULL; out2 optionally receives a second copy of max_out; cnt_out (R,F), optional,
 * receives the number of rows attaining the max -- reduce_max's gradient is shared among ties).  */
int dgcnn_bn_act_kreduce_f32(const float* Y, int64_t R, int k, int F,
                             const float* mean, const float* rstd, const float* beta, int relu,
                             float* max_out, int64_t ldmax, float* mean_out, int64_t ldmean,
                             float* out2, int64_t ldout2, float* cnt_out, void* stream);
/* backward, pass 1: red[0][f] = sum dZ, red[1][f] = sum dZ*xhat over all R*k rows, where
 * dZ = relu'(z) * ( dmax*[z==max]/ties + dmean/k ).  red: double[DGCNN_STAT_SLOTS][2][F], zeroed. */
int dgcnn_bn_bwd_reduce_f32(const float* Y, int64_t R, int k, int F,
                            const float* mean, const float* rstd, const float* beta, int relu,
                            const float* dmax, int64_t lddmax, const float* dmean, int64_t lddmean,
                            const float* mx_in, int64_t ldmx, const float* cnt_in,   /* forward's max / #ties, or NULL: recompute */
                            double* red, void* stream);
/* backward, pass 2: dY = rstd*(dZ - red0/cnt - xhat*red1/cnt) written to dY (may alias Y);
 * dbeta[f] (+)= red0 ; dYsum[r][f] = sum_m dY (optional, feeds the centre dgrad).
 * `red` is reduced over its slots in place (slot 0 then holds the totals).
 * relu: bit 0 = the layer has a ReLU; bit 1 (value 2) = dY is written as bf16 VALUES (nearest even, stored as fp32)
 * and dYsum adds those: the operand rounding of the bf16 edge-MLP's gradient products, done once where dY is formed.
 * Bit 1 exists in dgcnn_bn_bwd_apply_f32 and dgcnn_edge_bn_bwd_apply_f32 only (any k), which take relu in 0 .. 3; every
 * other entry point with a `relu` argument (forward, reduce, deterministic reduce, dropout-fused and plane-writing passes)
 * takes 0 or 1 and returns DGCNN_EINVAL otherwise, so that a reduce and an apply can never disagree about the ReLU. */
int dgcnn_bn_bwd_apply_f32(const float* Y, int64_t R, int k, int F,
                           const float* mean, const float* rstd, const float* beta, int relu,
                           const float* dmax, int64_t lddmax, const float* dmean, int64_t lddmean,
                           const float* mx_in, int64_t ldmx, const float* cnt_in,
                           double* red, float* dY, float* dYsum, int64_t lddysum, float* dbeta,
                           float dbeta_beta, void* stream);

/* ---- deterministic mode: fixed-order replacements of the three atomically accumulated steps -------------------------
 * (the fused epilogues sum the BatchNorm statistics with LDS / fp64 atomics and the transposed adjacency is filled through
 * LDS cursors: results are reproducible to ~1e-7 only, and a dynamic graph amplifies that into different neighbour lists).
 * Two-stage sums: DGCNN_DET blocks own contiguous row ranges and walk them in order, then one thread per column adds the
 * partials in block order into SLOT 0 of `stats` / `red` (caller-zeroed, same layout as above).  ws: dgcnn_det_workspace_bytes(F). */
int dgcnn_det_workspace_bytes(int F);
/* column sum / sum of squares of a materialised (rows, F) tensor (leading dimension ld): slim.batch_norm's statistics */
int dgcnn_colstats_det_f32(const float* Y, int64_t rows, int F, int64_t ld, double* stats, void* ws, size_t ws_bytes,
                           void* stream);
/* dgcnn_bn_bwd_reduce_f32 on a materialised Y (dmean == NULL: the k = 1 form) */
int dgcnn_bn_bwd_reduce_det_f32(const float* Y, int64_t R, int k, int F, const float* mean, const float* rstd,
                                const float* beta, int relu, const float* dmax, int64_t lddmax,
                                const float* dmean, int64_t lddmean, const float* mx_in, int64_t ldmx,
                                const float* cnt_in, double* red, void* ws, size_t ws_bytes, void* stream);
/* every bucket of the transposed adjacency (dgcnn_edge_csr_build: off, rev) in ascending edge order, out of place -> rev_sorted */
int dgcnn_edge_csr_sort(const int32_t* idx, int B, int N, int k, const int32_t* off, const int32_t* rev,
                        int32_t* rev_sorted, void* stream);

/* ---- head helpers (model.py:76-91) and residual add (ops.py:134) -------------------------- */
/* max_pool_v2 over the N points of each cloud: out[b][f] = max_i x[b][i][f], arg[b][f] = first i */
int dgcnn_global_max_f32(const float* x, int64_t ldx, int B, int N, int F, float* out, int32_t* arg,
                         void* stream);
/* its gradient: dx[b][arg[b][f]][f] += dout[b][f] */
int dgcnn_global_max_bwd_f32(const float* dout, const int32_t* arg, int B, int N, int F,
                             float* dx, int64_t lddx, void* stream);
/* out[g][f] = sum over the rows_per_group rows of group g (tf.tile^T, model.py:81) */
int dgcnn_group_colsum_f32(const float* x, int64_t ldx, int G, int rows_per_group, int F,
                           float* out, void* stream);
/* tf.tile (model.py:80-81): dst[g * rows_per_group + i][f] = src[g][f] -- only FC_LAYERS = 0 materialises the tiled global
 * feature (the dropout of model.py:90-91 then acts on it element by element); FC0 otherwise folds it into a per-cloud bias */
int dgcnn_tile_rows_f32(const float* src, int64_t lds, int G, int rows_per_group, int F, float* dst, int64_t ldd,
                        void* stream);
/* ---- the same per-cloud passes for a PACKED tower (csrc/seg.hip): cloud b = rows [seg_off[b], seg_off[b + 1]) of a row-major
 * (rows, F) tensor, seg_off = int32[nseg + 1] on the device, strictly increasing from 0 to rows.  Grids are shaped over 64-row
 * chunks of the tower, cut at the cloud boundaries inside them -- never one workgroup per cloud.
 *   dgcnn_colmax_seg_f32           keys[b][f] (uint64, caller-zeroed) <- atomicMax(f32_ordered(value) << 32 | ~row-in-cloud): the key
 *                                  format of dgcnn_gemm_f32's column-maximum epilogue; dgcnn_colmax_decode_f32 -> (max, FIRST arg-max),
 *                                  (NaN, 0) for an all-NaN column.  Independent of the order in which the atomics land.
 *   dgcnn_global_max_bwd_seg_f32   dx[seg_off[b] + arg[b][f]][f] += dout[b][f]
 *   dgcnn_seg_colsum_f32           out[b][f] = sum over the rows of cloud b (tf.tile^T), summed in a fixed order (bit-reproducible);
 *                                  ws: dgcnn_seg_colsum_workspace_bytes(rows, nseg, F) bytes of scratch, 4-byte aligned
 *   dgcnn_tile_rows_seg_f32        dst[r][f] = src[row_group[r]][f] (tf.tile; row_group = int32[rows], the row -> cloud map)      */
int dgcnn_colmax_seg_f32(const float* x, int64_t ldx, int rows, int F, const int32_t* seg_off, int nseg, void* keys,
                         void* stream);
int dgcnn_global_max_bwd_seg_f32(const float* dout, const int32_t* arg, const int32_t* seg_off, int nseg, int F,
                                 float* dx, int64_t lddx, void* stream);
int64_t dgcnn_seg_colsum_workspace_bytes(int rows, int nseg, int F);
int dgcnn_seg_colsum_f32(const float* x, int64_t ldx, int rows, int F, const int32_t* seg_off, int nseg, float* out,
                         void* ws, size_t ws_bytes, void* stream);
int dgcnn_tile_rows_seg_f32(const float* src, int64_t lds, const int32_t* row_group, int rows, int F, float* dst, int64_t ldd,
                            void* stream);
/* ---- BatchNorm of a packed tower with the statistics of the row's OWN cloud (csrc/seg_bn.hip; the forward here, the backward
 * below).  Cloud b = rows [seg_off[b], seg_off[b + 1]); idx (rows, k) holds TOWER rows; statistics are double[nseg][2][F] (sum and sum
 * of squares per cloud; WRITTEN, not accumulated: the caller does not zero them); mean / rstd are float[nseg][F] tables; row_group =
 * int32[rows], the row -> cloud map.  With these a cloud's outputs do not depend on the other clouds of its tower.
 *   dgcnn_seg_colstats_f32     per cloud, the column sums of a materialised (rows, F) tensor (the k = 1 layers)
 *   dgcnn_seg_edge_stats_f32   the same over the never-materialised conv0 output y = V[idx[r, m]] + U[r] (the single fp32 add of
 *                              dgcnn_edge_gather_add_f32).  F % 4 == 0, F <= 1024, 16-byte aligned rows, rows < 2^24, ldv < 2^24,
 *                              rows * ldv < 2^32 (DGCNN_EUNSUP otherwise)
 *     Both sum in ONE fixed order, whatever dgcnn_set_stat_slots says (two runs are bit-identical): stage 1 over 64-row chunks of
 *     the tower cut at the cloud boundaries (grids over chunks, never one workgroup per cloud; the edge form keeps consecutive chunks
 *     on one XCD), every (chunk, cloud) piece one double per column; stage 2 adds a cloud's pieces first chunk to last, in double.
 *     ws: dgcnn_seg_stats_workspace_bytes(rows, nseg, F) bytes (host only; 0 for an empty tower), 8-byte aligned; DGCNN_ENOSPC with
 *     the needed count in dgcnn_last_error otherwise.
 *   dgcnn_seg_bn_finalize_f32  mean / rstd of cloud b from its sums and the count (seg_off[b + 1] - seg_off[b]) * k:
 *                              dgcnn_bn_finalize_f32's arithmetic (double, biased variance clamped at 0)
 *   dgcnn_seg_bn_act_f32       k = 1: out[r] = act((T[r] - mean[g]) * rstd[g] + beta), g = row_group[r]; row_group == NULL: g = r
 *                              (normalises the per-cloud max-pool, rows = nseg).  out2: optional second copy.  float4 path when
 *                              everything is 16-byte aligned with F, ld % 4 == 0, scalar path otherwise (the class dimension)
 *   dgcnn_seg_edge_bn_act_kreduce_f32   BN + ReLU + max / mean (mean_out may be NULL) over the k recomputed edge rows of each point
 *                              with the table row of the point's cloud; the shapes of dgcnn_seg_edge_stats_f32.  No tie / positive
 *                              counts (they serve the backward only).
 * A one-cloud tower with the dense kernels' mean / rstd gives dgcnn_bn_act_kreduce_f32 / dgcnn_edge_bn_act_kreduce_f32's outputs bit
 * for bit.  DGCNN_EINVAL for null or misshapen arguments; nothing is written on error. */
int64_t dgcnn_seg_stats_workspace_bytes(int rows, int nseg, int F);
int dgcnn_seg_colstats_f32(const float* x, int64_t ldx, int rows, int F, const int32_t* seg_off, int nseg, double* stats,
                           void* ws, size_t ws_bytes, void* stream);
int dgcnn_seg_edge_stats_f32(const float* V, int64_t ldv, const float* U, int64_t ldu, const int32_t* idx, int rows, int k, int F,
                             const int32_t* seg_off, int nseg, double* stats, void* ws, size_t ws_bytes, void* stream);
int dgcnn_seg_bn_finalize_f32(const double* stats, int nseg, int F, const int32_t* seg_off, int k, float eps, float* mean,
                              float* rstd, void* stream);
int dgcnn_seg_bn_act_f32(const float* T, int64_t ldt, int rows, int F, const int32_t* row_group, const float* mean,
                         const float* rstd, const float* beta, int relu, float* out, int64_t ldo, float* out2, int64_t ldo2,
                         void* stream);
int dgcnn_seg_edge_bn_act_kreduce_f32(const float* V, int64_t ldv, const float* U, int64_t ldu, const int32_t* idx, int rows, int k,
                                      int F, const int32_t* row_group, const float* mean, const float* rstd, const float* beta,
                                      int relu, float* max_out, int64_t ldmax, float* mean_out, int64_t ldmean, void* stream);
/* ---- the backward of the per-cloud BatchNorm (csrc/seg_bn.hip).  red = double[nseg][2][F]: per cloud sum dz and sum dz * xhat
 * (WRITTEN, not accumulated: no zeroing, not in the slot arena); c1 / c2 = float[nseg][F] tables red / (n_b k).  The arithmetic is
 * that of dgcnn_bn_bwd_reduce_f32 / dgcnn_bn_bwd_apply_f32 and their edge forms, operation for operation: a one-cloud tower gives
 * their dY / dYsum bit for bit.  Both reduces sum in ONE fixed order in every dgcnn_set_stat_slots setting (no atomics variant), by
 * the two stages of dgcnn_seg_colstats_f32 (64-row chunks cut at the cloud boundaries; per piece fp32 per wave over <= 16 rows, the
 * four waves in double; then a cloud's pieces first chunk to last); ws: dgcnn_seg_stats_workspace_bytes(rows, nseg, F), 8-byte
 * aligned (DGCNN_ENOSPC otherwise).  relu must be 0 or 1.  DGCNN_EINVAL for null / misshapen / (edge entries) misaligned arguments,
 * DGCNN_EUNSUP for F % 4 != 0 or k >= 256 in the edge entries; nothing is written on error.
 *   dgcnn_seg_edge_bn_act_kreduce_cnt_f32    dgcnn_seg_edge_bn_act_kreduce_f32 (one kernel template; max_out / mean_out bit-identical)
 *                              that also writes cnt_out (rows, F) = #ties of the max + 256 * #(z > 0), dgcnn_edge_bn_act_kreduce_f32's
 *                              packing (k < 256)
 *   dgcnn_seg_bn_bwd_reduce_f32   k = 1: the sums of dz = (dout + d2) [z > 0 if relu] and dz * xhat over the rows of each cloud, z and
 *                              xhat from T with the cloud's mean / rstd row; d2 (optional): the gradient of a second copy of the
 *                              output.  float4 path when everything is 16-byte aligned with F, ld % 4 == 0, scalar path otherwise
 *   dgcnn_seg_edge_bn_bwd_reduce_points_f32  conv0 (a ReLU layer): the same sums in closed form from the forward's per-point outputs
 *                              (max, mean, packed counts) and dmax / dmean -- dgcnn_edge_bn_bwd_reduce_points_f32's integrand, no pass
 *                              over the edges
 *   dgcnn_seg_bn_bwd_finalize_f32  c1[b][f] = float(red0 * (1.0 / (n_b k))), c2 likewise; dbeta (may be NULL):
 *                              dbeta[f] = dbeta_beta * dbeta[f] + float(sum_b red0[b][f]), b ascending, in double
 *   dgcnn_seg_bn_bwd_apply_f32    k = 1: dT[r] = rstd_g ((dz - c1_g) - xhat c2_g), g = row_group[r]; dT may alias T
 *   dgcnn_seg_edge_bn_bwd_apply_f32  conv0: y = V[idx] + U and z recomputed by the forward's instructions (z == mx compares equal),
 *                              dz = ((z == mx) ? dmax / ties : 0) + dmean * (1.0f / k), zero where relu and !(z > 0); writes
 *                              dY (rows * k, F) and dYsum (rows, F; may be NULL) = the k rows of dY added in ascending m */
int dgcnn_seg_edge_bn_act_kreduce_cnt_f32(const float* V, int64_t ldv, const float* U, int64_t ldu, const int32_t* idx, int rows, int k,
                                          int F, const int32_t* row_group, const float* mean, const float* rstd, const float* beta,
                                          int relu, float* max_out, int64_t ldmax, float* mean_out, int64_t ldmean, float* cnt_out,
                                          void* stream);
int dgcnn_seg_bn_bwd_reduce_f32(const float* T, int64_t ldt, int rows, int F, const int32_t* seg_off, int nseg, const float* mean,
                                const float* rstd, const float* beta, int relu, const float* dout, int64_t lddo, const float* d2,
                                int64_t ldd2, double* red, void* ws, size_t ws_bytes, void* stream);
int dgcnn_seg_edge_bn_bwd_reduce_points_f32(const float* mx, int64_t ldmx, const float* mn, int64_t ldmn, const float* cntpos,
                                            const float* dmax, int64_t lddmax, const float* dmean, int64_t lddmean, const float* beta,
                                            int rows, int k, int F, const int32_t* seg_off, int nseg, double* red, void* ws,
                                            size_t ws_bytes, void* stream);
int dgcnn_seg_bn_bwd_finalize_f32(const double* red, int nseg, int F, const int32_t* seg_off, int k, float* c1, float* c2,
                                  float* dbeta, float dbeta_beta, void* stream);
int dgcnn_seg_bn_bwd_apply_f32(const float* T, int64_t ldt, int rows, int F, const int32_t* row_group, const float* mean,
                               const float* rstd, const float* beta, int relu, const float* dout, int64_t lddo, const float* d2,
                               int64_t ldd2, const float* c1, const float* c2, float* dT, int64_t lddt, void* stream);
int dgcnn_seg_edge_bn_bwd_apply_f32(const float* V, int64_t ldv, const float* U, int64_t ldu, const int32_t* idx, int rows, int k, int F,
                                    const int32_t* row_group, const float* mean, const float* rstd, const float* beta, int relu,
                                    const float* dmax, int64_t lddmax, const float* dmean, int64_t lddmean, const float* mx_in,
                                    int64_t ldmx, const float* cnt_in, const float* c1, const float* c2, float* dY, float* dYsum,
                                    int64_t lddysum, void* stream);
/* tf.nn.dropout(net, keep) (model.py:91): counter-based RNG keyed by (seed, element index) so the
 * backward regenerates the same mask.  y may alias x. */
int dgcnn_dropout_f32(const float* x, float* y, int64_t n, float keep, uint64_t seed, void* stream);
/* the same mask function with the seed read from DEVICE memory at execution time: the host advances *seed_dev between
 * replays of a captured HIP graph (a by-value seed would be frozen into the graph). */
int dgcnn_dropout_dev_f32(const float* x, float* y, int64_t n, float keep, const uint64_t* seed_dev, void* stream);
/* out = relu(a + b) (ops.py:134); bwd: d = dout * [out > 0] */
int dgcnn_add_relu_f32(const float* a, int64_t lda, const float* b, int64_t ldb, int64_t R, int F,
                       float* out, int64_t ldo, void* stream);
int dgcnn_relu_bwd_f32(const float* dout, int64_t lddo, const float* out, int64_t ldo, int64_t R, int F,
                       float* d, int64_t ldd, void* stream);
/* dst (R, Cp) dense <- [src (R, C) | zero columns]: C = 3 coordinates padded to float4 rows */
int dgcnn_pad_copy_f32(const float* src, int64_t lds, int C, float* dst, int Cp, int64_t R, void* stream);
/* strided 2-D copy / accumulate: dst (+)= src   (views of concatenated buffers, tf.concat) */
int dgcnn_copy2d_f32(const float* src, int64_t lds, float* dst, int64_t ldd, int64_t R, int F,
                     int accumulate, void* stream);

/* ---- dgcnn/trainval.py:39-52: softmax, accuracy, sparse softmax CE (x weight), mean --------
 * scal[0] += sum loss*w / rows ; scal[1] += #correct / rows (caller zeroes scal).
 * dlogits = (softmax - onehot) * w / rows (NULL to skip); softmax optional.                   */
int dgcnn_softmax_xent_f32(const float* logits, const int32_t* labels, const float* weight,
                           int64_t rows, int ncls, float* softmax, float* dlogits, float* scal,
                           void* stream);

/* ---- the same CLOUD BY CLOUD for a packed tower (csrc/seg_loss.hip): what M micro-steps of `-mbs 1` compute.  Cloud b = rows
 * [seg_off[b], seg_off[b + 1]) (seg_off = int32[nseg + 1] on the device, STRICTLY increasing from 0 to rows: no empty cloud -- device
 * memory cannot be checked on the host, and an empty cloud would divide by n_b = 0 and leave a partial slot unwritten), n_b rows:
 *   l_b = (1 / n_b) sum_{r in b} w_r (log sum_c e^{z_rc} - z_{r, lab_r}),   a_b = #{r in b : FIRST arg-max of z_r == lab_r} / n_b
 *   (a negative label adds nothing to either sum but counts in n_b; w_r = 1 when weight == NULL),
 *   dlogits_r = (softmax_r - onehot_r) * w_r / n_b: the SUM over the clouds of the per-cloud means (micro-steps add up),
 *   cloud_scal = float[nseg][2] = {l_b, a_b},  scal = float[2] = {(1 / nseg) sum_b l_b, (1 / nseg) sum_b a_b}.
 * cloud_scal and scal are WRITTEN, not accumulated (no zeroing by the caller).  The per-row arithmetic is dgcnn_softmax_xent_f32's
 * operation for operation with 1.0f / n_b for its 1.0f / rows: a one-cloud tower gives its softmax and dlogits bit for bit.  The
 * sums are taken in ONE fixed order in every dgcnn_set_stat_slots setting (no atomics; two calls are bit-identical), by the two
 * stages of dgcnn_seg_colstats_f32: 64-row chunks cut at the cloud boundaries (grids over chunks, never one workgroup per cloud),
 * per (chunk, cloud) piece fp32 per wave over its <= 16 rows, the four waves in double; then a cloud's pieces first chunk to
 * last in double, l_b = float(sum * (1.0 / n_b)), a_b = float(count / n_b), and the clouds b-ascending in double for scal.
 * labels == NULL: the softmax only (cloud_scal / scal / ws untouched and may be NULL).  softmax or dlogits may be NULL; dlogits
 * needs labels.  ws: dgcnn_seg_softmax_xent_workspace_bytes(rows, nseg) bytes (host only; 0 for an empty tower), 8-byte aligned.
 * DGCNN_EINVAL -- before anything is launched or written -- for a null logits / seg_off (with labels: cloud_scal / scal / ws),
 * non-positive sizes, nseg > rows, nseg > 65535, a workspace that is too small or misaligned. */
int64_t dgcnn_seg_softmax_xent_workspace_bytes(int rows, int nseg);
int dgcnn_seg_softmax_xent_f32(const float* logits, const int32_t* labels, const float* weight, int rows, int ncls,
                               const int32_t* seg_off, int nseg, float* softmax, float* dlogits, float* cloud_scal, float* scal,
                               void* ws, size_t ws_bytes, void* stream);

/* ---- dgcnn/trainval.py:17,75-80: accumulators + tf.train.AdamOptimizer ---------------------- */
/* y = a*x + b*y over n elements */
int dgcnn_axpby_f32(const float* x, float a, float* y, float b, int64_t n, void* stream);
/* one Adam step on a flat parameter bucket; lr_t = lr*sqrt(1-b2^t)/(1-b1^t) computed by caller */
int dgcnn_adam_f32(float* param, const float* grad, float* m, float* v, int64_t n,
                   float lr_t, float b1, float b2, float eps, void* stream);

/* ---- launch plans (csrc/plan.cc): the counterpart of replaying a static TF graph with sess.run (dgcnn/trainval.py:103-129) ----
 * dgcnn_plan_begin .. dgcnn_plan_end: every launch, memset, cross-stream wait and all-reduce the library issues in between is
 * executed as usual AND recorded (kernel, geometry, a copy of the argument values, streams); dgcnn_plan_replay re-issues the list
 * from one C loop on the same streams (the GPU sees the eager schedule; ~2 us of host time per launch).  The caller keeps every
 * device address of the recorded step valid and unchanged for as long as the plan is replayed, and keeps per-step host values
 * (dropout seed: device memory; Adam's step size: outside the plan) out of it.  One recorder per process.
 * dgcnn_stream_wait: `waiter` waits for everything issued so far on `signaller` (event record + wait; recordable).
 * dgcnn_memset_async: hipMemsetAsync (recordable): the zero-fills of the step go through it.
 * dgcnn_plan_kernel: read kernel node `i` of a finished plan back, 0 <= i < `kernels` of dgcnn_plan_info, in recorded order
 * (memsets, waits and collectives are not counted).  `name` receives the demangled kernel name with its template arguments, e.g.
 * "void (anonymous namespace)::knn_mfma_kernel<64, 20, true>(float const*, ...)", NUL-terminated and truncated to name_bytes - 1
 * (the raw symbol where it does not demangle); grid / block (x, y, z) and the dynamic LDS bytes of the launch go to the other
 * outputs, each of which may be null.  The name is resolved when it is read, from the recorded kernel address; recording and
 * replay do not change, and the streams the plan recorded must still exist (the runtime looks the kernel up for the node's
 * stream).  DGCNN_EINVAL: null plan, null name, name_bytes == 0, i out of range; DGCNN_ELAUNCH: the runtime has no name for the
 * node.  A read walks the plan from its first node.  Tests assert from this which kernel a call launched (tests/launch_trace.py). */
int dgcnn_plan_begin(void);
int dgcnn_plan_end(void** plan_out);
int dgcnn_plan_abort(void);
int dgcnn_plan_replay(void* plan);
int dgcnn_plan_info(void* plan, int* kernels, int* memsets, int* waits, int* collectives);
int dgcnn_plan_kernel(void* plan, int i, char* name, size_t name_bytes, unsigned grid[3], unsigned block[3], unsigned* lds_bytes);
int dgcnn_plan_destroy(void* plan);
int dgcnn_stream_wait(void* waiter, void* signaller);
int dgcnn_memset_async(void* ptr, int value, size_t bytes, void* stream);
/* A stream for work nothing on the critical path waits for (the reference has no counterpart: TF schedules its graph itself):
 * low_priority != 0 -> the device's least stream priority; reserve_cus > 0 -> created on a CU mask that leaves that many compute
 * units (evenly over the XCDs) to the other streams (then at the default priority: the masked entry point takes none).
 * The caller owns the stream (dgcnn_stream_destroy). */
int dgcnn_stream_create(int low_priority, int reserve_cus, void** stream_out);
int dgcnn_stream_destroy(void* stream);
int dgcnn_stream_priority_range(int* least, int* greatest);

/* ---- the gradient collective (trainval.py:64-73 mean over the towers; here: one process per GPU, RCCL over xGMI) ----
 * RCCL is dlopen'ed on first use (librccl.so, or $DGCNN_RCCL_LIB); no torch.distributed involved.
 * dgcnn_comm_unique_id: rank 0 fills 128 bytes; the host ships them to the other ranks (dgcnn/rccl.py).
 * dgcnn_comm_init: ncclCommInitRank for this process' current HIP device -> opaque communicator.
 * dgcnn_allreduce_f32: in-place SUM over the ranks on `stream`;  dgcnn_broadcast_f32: root's buffer to every rank. */
int dgcnn_comm_available(void);        /* dlopen + symbol lookup only: DGCNN_OK or DGCNN_EUNSUP with the reason in dgcnn_last_error */
int dgcnn_comm_unique_id(void* id128);
int dgcnn_comm_init(int world, int rank, const void* id128, void** comm_out);
int dgcnn_comm_destroy(void* comm);
/* ranks / this rank / HIP device of the communicator as RCCL reports them (ncclCommCount, ncclCommUserRank, ncclCommCuDevice) */
int dgcnn_comm_info(void* comm, int* nranks, int* rank, int* device);
int dgcnn_allreduce_f32(float* buf, int64_t count, void* comm, void* stream);
int dgcnn_broadcast_f32(float* buf, int64_t count, int root, void* comm, void* stream);
/* all-reduce calls / elements issued through the library so far, replayed launch plans included */
int dgcnn_comm_counters(int64_t* allreduce_calls, int64_t* allreduce_elems);

#ifdef __cplusplus
}
#endif
#endif /* DGCNN_HIP_H_ */

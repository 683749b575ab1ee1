"""The kernels every k-NN and GEMM entry is expected to launch at the edges of its host dispatch, as LITERALS: read from
csrc/knn.hip (knn_impl, knn_scan, launch_scan, launch_hist_bound, launch_append_scan, launch_seed_bound), knn_wide.hip, knn_bigk.hip,
knn_grid.hip, knn_cross.hip, gemm.hip and gemm_x3.hip, not computed by a rule -- dgcnn/_engine.py already holds one copy of the rule
too many.  tests/test_gpu_knn_dispatch.py and tests/test_gpu_gemm_dispatch.py run every row, record its launches
(tests/launch_trace.py) and compare; tests/test_launch_names.py checks on the CPU that every kernel of those sources has a row.

A row that disagrees with a recorded launch is corrected only after deciding that the CODE is right (include/dgcnn_hip.h).

An expectation is (base name, [leading template arguments that matter]); "*" stands for an argument the row does not pin.
D / P / L: the cloud maps of knn_common.h."""

D, P, L = "DenseClouds", "PackedClouds", "ListedClouds"

# every k-NN switch at the library's default; a row's `sw` overrides some (all are restored after the row)
KNN_DEFAULTS = dict(grid=1, force_valu=0, wide_min_c=129, big_k_min=65, bf16_filter=2, seed_min_n=-1, append=1, append_products=1,
                    hist=2)
# the switches without a setter of their own, by their names in dgcnn_switch_set; a row's `table` overrides some (restored likewise)
GRID_MIN_N_UNSET = -2 ** 31                  # DGCNN_SWITCH_UNSET
TABLE_DEFAULTS = dict(DGCNN_KNN_GRID_MIN_N=GRID_MIN_N_UNSET)

SQ = ("sqnorm_kernel", [])
SQW = ("sqnorm_wide_kernel", [])
GRID = lambda kc, c4, cl: [("knn_grid_build_kernel", [cl]), ("knn_grid_query_kernel", [str(kc), c4, "*", cl])]


def knn_row(id, N, C, k, expect, B=2, ld=None, sw=None, seed=None, ws="full", engine=True, table=None):
    """One dense call.  ld: leading dimension of the view the call reads (None: C, contiguous).  seed: None, "own" (the row's own
    oracle graph, k columns) or "short" (k - 1 columns: kseed < k).  ws: "full" = dgcnn_knn_workspace_bytes, "s_i" = room for the norms
    only.  engine: the call can be issued through dgcnn._engine.knn as well (its tag is then held against the launches)."""
    return dict(id=id, B=B, N=N, C=C, k=k, ld=ld, sw=sw or {}, seed=seed, ws=ws, engine=engine and ws == "full" and seed != "short",
                expect=expect, table=table or {})


def _valu(cp, kc, cl=D):
    return ("knn_kernel", [str(cp), str(kc), cl])


def _mfma(cp, kc, vec):
    return ("knn_mfma_kernel", [str(cp), str(kc), vec])


def _hist(hs, cl=D):
    return ("knn_hist_bound_kernel", [str(hs), cl])


_APPEND = lambda lx, npr, cl=D, lp=16, ms=5: [SQ, ("knn_seed_bound_kernel", [str(lp), str(ms), cl]),
                                              ("knn_bf16a_kernel", [lx, str(npr), cl]), ("knn_select_kernel", [cl])]

KNN_DENSE = [
    # ---- raw coordinates, C = 3, k = 20: the histogram bound of launch_hist_bound (N >= 256, N >= 4 k stride, not with VALU forced)
    knn_row("c3_n300", 300, 3, 20, [SQ, _hist(2), _valu(4, 20)]),
    knn_row("c3_n255_no_hist", 255, 3, 20, [SQ, _valu(4, 20)]),
    knn_row("c3_n300_k40_no_hist", 300, 3, 40, [SQ, _valu(4, 40)]),                       # 4 * 40 * 2 > 300
    knn_row("c3_n300_k40_hist1", 300, 3, 40, [SQ, _hist(1), _valu(4, 40)], sw=dict(hist=1)),
    knn_row("c3_n300_hist4", 300, 3, 8, [SQ, _hist(4), _valu(4, 8)], sw=dict(hist=4)),
    knn_row("c3_n300_hist_off", 300, 3, 20, [SQ, _valu(4, 20)], sw=dict(hist=0)),
    knn_row("c3_n300_valu", 300, 3, 20, [SQ, _valu(4, 20)], sw=dict(force_valu=1)),
    # ---- the cell grid (knn_impl: grid applicable, not VALU, the workspace holds its scratch, N >= 4096 in mode 1)
    knn_row("c3_n4096_grid", 4096, 3, 20, [SQ] + GRID(20, "false", D), B=1),
    knn_row("c3_n4095_scan", 4095, 3, 20, [SQ, _hist(2), _valu(4, 20)], B=1),
    knn_row("c3_n4096_ws_s_i_scan", 4096, 3, 20, [SQ, _valu(4, 20)], B=1, ws="s_i"),      # no room for the histogram's bounds either
    knn_row("c3_n4096_k64_scan", 4096, 3, 64, [SQ, _hist(2), _valu(4, 64)], B=1),         # the grid keeps k <= 40
    knn_row("c3_n300_grid_mode2", 300, 3, 20, [SQ] + GRID(20, "false", D), sw=dict(grid=2)),
    knn_row("c3_n4096_grid_mode0", 4096, 3, 20, [SQ, _hist(2), _valu(4, 20)], B=1, sw=dict(grid=0)),
    # DGCNN_KNN_GRID_MIN_N moves the smallest N of mode 1, in the library and in the engine's tag alike
    knn_row("c3_n1024_grid_min_n_1024", 1024, 3, 20, [SQ] + GRID(20, "false", D), table=dict(DGCNN_KNN_GRID_MIN_N=1024)),
    knn_row("c3_n1024_grid_min_n_unset", 1024, 3, 20, [SQ, _hist(2), _valu(4, 20)]),
    knn_row("c4_n4096_grid", 4096, 4, 8, [SQ] + GRID(8, "true", D), B=1),
    knn_row("c1_n4096_grid", 4096, 1, 40, [SQ] + GRID(40, "false", D), B=1),
    # ---- C <= 16: fp32 distances on the matrix pipe, float4 or scalar loader
    knn_row("c16_k8", 300, 16, 8, [SQ, _mfma(16, 8, "true")]),
    knn_row("c16_k8_ld17", 300, 16, 8, [SQ, _mfma(16, 8, "false")], ld=17),
    knn_row("c5_k8", 300, 5, 8, [SQ, _mfma(16, 8, "false")]),
    knn_row("c16_k8_valu", 300, 16, 8, [SQ, _valu(16, 8)], sw=dict(force_valu=1)),
    # ---- 16 < C <= 64, k = 20: matrix pipe below N = 8192, bf16 filter from there on (float4-loadable rows, C % 4 == 0 only)
    knn_row("c64_n300", 300, 64, 20, [SQ, _mfma(64, 20, "true")]),
    knn_row("c64_n8191", 8191, 64, 20, [SQ, _mfma(64, 20, "true")], B=1),
    knn_row("c64_n8192_bf16f", 8192, 64, 20, [SQ, ("knn_bf16f_kernel", ["20"])], B=1),
    knn_row("c64_n300_filter1", 300, 64, 20, [SQ, ("knn_bf16f_kernel", ["20"])], sw=dict(bf16_filter=1)),
    knn_row("c64_n8192_filter0", 8192, 64, 20, [SQ, _mfma(64, 20, "true")], B=1, sw=dict(bf16_filter=0)),
    knn_row("c20_filter1", 300, 20, 20, [SQ, ("knn_bf16f_kernel", ["20"])], sw=dict(bf16_filter=1)),
    knn_row("c18_filter1", 300, 18, 20, [SQ, _mfma(64, 20, "false")], sw=dict(bf16_filter=1)),
    knn_row("c17_filter1", 300, 17, 20, [SQ, _mfma(64, 20, "false")], sw=dict(bf16_filter=1)),
    knn_row("c64_ld65_filter1", 300, 64, 20, [SQ, _mfma(64, 20, "false")], ld=65, sw=dict(bf16_filter=1)),
    knn_row("c64_valu", 300, 64, 20, [SQ, _valu(64, 20)], sw=dict(force_valu=1)),
    # KC edges (launch_scan_k)
    knn_row("c64_k8", 300, 64, 8, [SQ, _mfma(64, 8, "true")]),
    knn_row("c64_k9", 300, 64, 9, [SQ, _mfma(64, 20, "true")]),
    knn_row("c64_k21", 300, 64, 21, [SQ, _mfma(64, 40, "true")]),
    knn_row("c64_k40", 300, 64, 40, [SQ, _mfma(64, 40, "true")]),
    knn_row("c64_k41", 300, 64, 41, [SQ, _mfma(64, 64, "true")]),
    knn_row("c64_k64", 300, 64, 64, [SQ, _mfma(64, 64, "true")]),
    # ---- 64 < C <= 128: the VALU scan only (no matrix-pipe instance), or the channel-slab scan from dgcnn_knn_wide_min_c on
    knn_row("c65", 300, 65, 20, [SQ, _valu(128, 20)]),
    knn_row("c128", 300, 128, 20, [SQ, _valu(128, 20)]),
    knn_row("c65_wide", 300, 65, 20, [SQ, ("knn_wide_kernel", ["20", "false", D])], sw=dict(wide_min_c=65)),   # 65 % 4 != 0
    knn_row("c128_wide", 300, 128, 8, [SQ, ("knn_wide_kernel", ["8", "true", D])], sw=dict(wide_min_c=65)),
    # ---- C > 128: the chunked norm kernel and the channel-slab scan
    knn_row("c129", 300, 129, 20, [SQW, ("knn_wide_kernel", ["20", "false", D])]),
    knn_row("c132", 300, 132, 40, [SQW, ("knn_wide_kernel", ["40", "true", D])]),
    knn_row("c1024", 300, 1024, 64, [SQW, ("knn_wide_kernel", ["64", "true", D])], B=1),
    # ---- k > 64 (or dgcnn_knn_big_k_min): the large-k scan, E = 4 up to k = 128, else 8; a seed is ignored
    knn_row("k65", 300, 64, 65, [SQ, ("knn_bigk_kernel", ["4", "true", D])]),
    knn_row("k128", 300, 64, 128, [SQ, ("knn_bigk_kernel", ["4", "true", D])]),
    knn_row("k129", 300, 64, 129, [SQ, ("knn_bigk_kernel", ["8", "true", D])]),
    knn_row("k256", 300, 64, 256, [SQ, ("knn_bigk_kernel", ["8", "true", D])], B=1),
    knn_row("k65_c192", 300, 192, 65, [SQW, ("knn_bigk_kernel", ["4", "true", D])], B=1),
    knn_row("k65_c3", 300, 3, 65, [SQ, ("knn_bigk_kernel", ["4", "false", D])], B=1),
    knn_row("k20_big_k_min", 300, 64, 20, [SQ, ("knn_bigk_kernel", ["4", "true", D])], sw=dict(big_k_min=20)),
    knn_row("k20_big_k_min_seeded", 300, 64, 20, [SQ, ("knn_bigk_kernel", ["4", "true", D])], sw=dict(big_k_min=20), seed="own"),
    # ---- seeded with the row's own graph, C = 64, k = 20
    knn_row("seeded_n300", 300, 64, 20, _APPEND("true", 1), seed="own"),
    knn_row("seeded_n300_products3", 300, 64, 20, _APPEND("true", 3), seed="own", sw=dict(append_products=3)),
    knn_row("seeded_n8192", 8192, 64, 20, _APPEND("false", 1), B=1, seed="own"),
    knn_row("seeded_n300_k40", 300, 64, 40, _APPEND("true", 1, ms=10), seed="own"),
    knn_row("seeded_n300_k41", 300, 64, 41, _APPEND("true", 1, ms=16), seed="own"),
    knn_row("seeded_n300_no_append", 300, 64, 20, [SQ, _mfma(64, 20, "true")], seed="own", sw=dict(append=0)),   # below the list-seeding N
    knn_row("seeded_n4096_no_append", 4096, 64, 20, [SQ, ("knn_seed_bound_kernel", ["16", "5", D]), ("knn_bf16f_kernel", ["20"])],
            B=1, seed="own", sw=dict(append=0)),
    knn_row("seeded_n300_no_append_min0", 300, 64, 20, [SQ, ("knn_seed_bound_kernel", ["16", "5", D]), ("knn_bf16f_kernel", ["20"])],
            seed="own", sw=dict(append=0, seed_min_n=0)),
    knn_row("seeded_short", 300, 64, 20, [SQ, _mfma(64, 20, "true")], seed="short"),
    knn_row("seeded_ws_s_i", 300, 64, 20, [SQ, _mfma(64, 20, "true")], seed="own", ws="s_i"),
    knn_row("seeded_c16_min0", 300, 16, 20, [SQ, ("knn_seed_bound_kernel", ["4", "2", D]), _mfma(16, 20, "true")], seed="own",
            sw=dict(seed_min_n=0)),
    knn_row("seeded_c32", 300, 32, 20, _APPEND("true", 1, lp=8, ms=3), seed="own"),
    knn_row("seeded_c32_k25", 300, 32, 25, _APPEND("true", 1, lp=8, ms=8), seed="own"),
    # launch_seed_bound takes C = 16, 32, 64 only: any other width gets no bound, and without a bound there is no append-form scan
    knn_row("seeded_c20", 300, 20, 20, [SQ, _mfma(64, 20, "true")], seed="own", sw=dict(seed_min_n=0)),
    knn_row("seeded_c48", 300, 48, 20, [SQ, _mfma(64, 20, "true")], seed="own", sw=dict(seed_min_n=0)),
    # knn_seeds_used_dense: the seeded probe forms 32-bit element offsets inside a cloud, so seeds are used only while N * ld < 2^31.
    # ld = 2^20 - 4: N * ld = 2^31 - 8192, the list of seeded_n300; ld = 2^20: N * ld = 2^31, the seeds are dropped (the call does not
    # fail) and the list is the unseeded one.  The view is built on the device inside an 8.6 GB buffer that is never filled.
    knn_row("seeded_n2048_ld_below_2_31", 2048, 64, 20, _APPEND("true", 1), B=1, ld=(1 << 20) - 4, seed="own"),
    knn_row("seeded_n2048_ld_at_2_31", 2048, 64, 20, [SQ, _mfma(64, 20, "true")], B=1, ld=1 << 20, seed="own"),
]


def seg_row(id, sizes, C, k, expect, entry="seg", sw=None, seed=None, mix_t=None, engine=True, geom=None):
    """One packed tower of clouds of `sizes` rows.  entry: "seg" = dgcnn_knn_seg_f32, "grid" = dgcnn_knn_seg_grid_f32, "mix" =
    dgcnn_knn_seg_mix_f32 with the clouds of at least mix_t points in the grid class, "engine" = whatever dgcnn._engine.knn_packed
    picks under the row's switches and dgcnn_knn_seg_mix_min_n(mix_t).  geom: {kernel: (largest cloud, clouds)} where a kernel runs
    over one class of the tower only."""
    return dict(id=id, sizes=sizes, C=C, k=k, entry=entry, sw=sw or {}, seed=seed, mix_t=mix_t, engine=engine, expect=expect,
                geom=geom or {})


_MIX_GEOM = {"knn_grid_build_kernel": (500, 1), "knn_grid_query_kernel": (500, 1), "knn_hist_bound_kernel": (300, 2),
             "knn_kernel": (300, 2)}
_MIX = [SQ] + GRID(20, "false", L) + [_hist(2, L), _valu(4, 20, L)]

KNN_PACKED = [
    seg_row("seg_c64", [70, 131, 300], 64, 20, [SQ, _valu(64, 20, P)]),
    seg_row("seg_c64_seeded", [70, 131, 300], 64, 20, _APPEND("true", 1, P), seed="own"),
    seg_row("seg_c64_seeded_products3", [70, 131, 300], 64, 20, _APPEND("true", 3, P), seed="own", sw=dict(append_products=3)),
    seg_row("seg_c64_seeded_below_min_n", [70, 131, 300], 64, 20, [SQ, _valu(64, 20, P)], seed="own", sw=dict(seed_min_n=100)),
    seg_row("seg_c64_seeded_no_append", [70, 131, 300], 64, 20, [SQ, _valu(64, 20, P)], seed="own", sw=dict(append=0)),
    seg_row("seg_c16", [70, 131, 300], 16, 8, [SQ, _valu(16, 8, P)]),
    seg_row("seg_c128", [70, 131, 300], 128, 40, [SQ, _valu(128, 40, P)]),
    seg_row("seg_c3_hist", [300, 333, 401], 3, 20, [SQ, _hist(2, P), _valu(4, 20, P)]),
    seg_row("seg_c3_k40_no_hist", [200, 333, 401], 3, 40, [SQ, _valu(4, 40, P)]),
    seg_row("seg_c129", [70, 131, 300], 129, 20, [SQW, ("knn_wide_kernel", ["20", "false", P])]),
    seg_row("seg_k65", [70, 131, 300], 64, 65, [SQ, ("knn_bigk_kernel", ["4", "true", P])]),
    seg_row("seg_grid", [70, 131, 300], 3, 20, [SQ] + GRID(20, "false", P), entry="grid", engine=False),
    seg_row("seg_mix", [300, 500, 280], 3, 20, _MIX, entry="mix", mix_t=400, engine=False, geom=_MIX_GEOM),
    # dgcnn._engine.knn_packed choosing among the three entries: grid mode x dgcnn_knn_seg_mix_min_n x the tower's sizes
    seg_row("engine_mode0", [300, 500, 280], 3, 20, [SQ, _hist(2, P), _valu(4, 20, P)], entry="engine", sw=dict(grid=0), mix_t=0),
    seg_row("engine_mode0_t400", [300, 500, 280], 3, 20, [SQ, _hist(2, P), _valu(4, 20, P)], entry="engine", sw=dict(grid=0), mix_t=400),
    seg_row("engine_mode1_t0", [300, 500, 280], 3, 20, [SQ, _hist(2, P), _valu(4, 20, P)], entry="engine", mix_t=0),   # mean size < 16384
    seg_row("engine_mode2", [300, 500, 280], 3, 20, [SQ] + GRID(20, "false", P), entry="engine", sw=dict(grid=2), mix_t=0),
    seg_row("engine_mode2_t400", [300, 500, 280], 3, 20, [SQ] + GRID(20, "false", P), entry="engine", sw=dict(grid=2), mix_t=400),
    seg_row("engine_mode1_t400_mixed", [300, 500, 280], 3, 20, _MIX, entry="engine", mix_t=400, geom=_MIX_GEOM),
    seg_row("engine_mode1_t100_all_grid", [300, 500, 280], 3, 20, [SQ] + GRID(20, "false", P), entry="engine", mix_t=100),
    seg_row("engine_mode1_t1000_all_scan", [300, 500, 280], 3, 20, [SQ, _hist(2, P), _valu(4, 20, P)], entry="engine", mix_t=1000),
]


def cross_row(id, M, N, C, k, expect, B=2, ldq=None, ldp=None, sizes=None, same=False):
    """One dgcnn_knn_cross_f32 call: B clouds of M queries against N candidates, or packed towers of `sizes` = [(m, n), ...].
    same: queries and candidates are the same buffer under the same map."""
    return dict(id=id, B=B, M=M, N=N, C=C, k=k, ldq=ldq, ldp=ldp, sizes=sizes, same=same, expect=expect)


def _cross(kc, vec, sl, cl=D):
    return ("knn_cross_kernel", [str(kc), vec, str(sl), cl])


_TOWERS = [(70, 90), (131, 64), (20, 300)]

KNN_CROSS = [
    cross_row("c3", 100, 300, 3, 20, [SQ, SQ, _cross(20, "false", 16)]),
    cross_row("c16", 100, 300, 16, 20, [SQ, SQ, _cross(20, "true", 16)]),
    cross_row("c16_ldq17", 100, 300, 16, 20, [SQ, SQ, _cross(20, "false", 16)], ldq=17),
    cross_row("c16_ldp17", 100, 300, 16, 20, [SQ, SQ, _cross(20, "false", 16)], ldp=17),
    cross_row("c17", 100, 300, 17, 20, [SQ, SQ, _cross(20, "false", 64)]),
    cross_row("c20", 100, 300, 20, 20, [SQ, SQ, _cross(20, "true", 64)]),
    cross_row("c64_k8", 100, 300, 64, 8, [SQ, SQ, _cross(8, "true", 64)]),
    cross_row("c64_k9", 100, 300, 64, 9, [SQ, SQ, _cross(20, "true", 64)]),
    cross_row("c64_k21", 100, 300, 64, 21, [SQ, SQ, _cross(40, "true", 64)]),
    cross_row("c64_k41", 100, 300, 64, 41, [SQ, SQ, _cross(64, "true", 64)]),
    cross_row("c64_k64", 100, 300, 64, 64, [SQ, SQ, _cross(64, "true", 64)]),
    cross_row("c129", 100, 300, 129, 20, [SQW, SQW, _cross(20, "false", 64)]),
    cross_row("c64_same", 300, 300, 64, 20, [SQ, _cross(20, "true", 64)], same=True),
    cross_row("packed_c3", 0, 0, 3, 20, [SQ, SQ, _cross(20, "false", 16, P)], sizes=_TOWERS),
    cross_row("packed_c64", 0, 0, 64, 20, [SQ, SQ, _cross(20, "true", 64, P)], sizes=_TOWERS),
    cross_row("packed_c64_same", 0, 0, 64, 20, [SQ, _cross(20, "true", 64, P)], sizes=[(70, 70), (131, 131), (300, 300)], same=True),
]

# query rows (or points) per block of the kernels whose grid is (ceil(largest cloud / rows), clouds), as their launch sites have it
ROWS_PER_BLOCK = {"knn_kernel": 64, "knn_mfma_kernel": 64, "knn_bf16f_kernel": 64, "knn_bf16a_kernel": 64, "knn_wide_kernel": 64,
                  "knn_bigk_kernel": 64, "knn_cross_kernel": 64, "knn_hist_bound_kernel": 64, "knn_grid_query_kernel": 256}

# where a kernel's template arguments carry CP and KC (None: it has no such parameter), for the <C..,k..> of the engine's tags
CP_KC_ARGS = {"knn_kernel": (0, 1), "knn_mfma_kernel": (0, 1), "knn_bf16f_kernel": (None, 0), "knn_bf16a_kernel": (None, None),
              "knn_wide_kernel": (None, 0), "knn_cross_kernel": (None, 0), "knn_grid_query_kernel": (None, 0),
              "knn_bigk_kernel": (None, None)}

def gemm_row(id, layout, M, N, K, expect, arith=6, override=0, unaligned=False, colmax_rpg=0, seg=False):
    """One product C (M, N) = op(A) op(B) with a reduction of K through dgcnn._engine.gemm.  layout: NN / NT / TN (the stored A is
    K x M for TN, the stored B N x K for NT).  arith: dgcnn_gemm_set_arith.  override: dgcnn_gemm_x3_tile_override.  unaligned: A is a
    view into a buffer one column wider (not float4-loadable).  colmax_rpg: rows per group of the column-maximum epilogue.  seg:
    dgcnn_gemm_seg_f32 with a per-cloud bias through the row -> cloud map."""
    return dict(id=id, layout=layout, M=M, N=N, K=K, arith=arith, override=override, unaligned=unaligned, colmax_rpg=colmax_rpg, seg=seg,
                expect=expect)


# template arguments as the demangler prints the enums of gemm_common.h / gemm_x3.hip: A_ROW 0, A_COL 1; B_ROW 0, B_COL 1; E_STORE 0;
# KCONTIG 0, KSTRIDED 1
def _native(a, b, bn, vec):
    return ("gemm_kernel", [a, b, "0", "128", str(bn), vec])          # <ASRC, BSRC, EPI, BM, BN, VEC>


def _x3(ak, bk, bn, np_=6, bm=128):
    return ("gemm_x3_kernel", [ak, bk, str(bn), str(np_), str(bm)])   # <AKIND, BKIND, BN, NP, BM>


def _w2(ak, bk, np_=6):
    return ("gemm_x3w2_kernel", [ak, bk, str(np_)])                   # <AKIND, BKIND, NP>: 256 x 128, wave-specialised


def _q(ak, bk, bm):
    return ("gemm_x3q_kernel", [ak, bk, "6", str(bm)])                # <AKIND, BKIND, NP, BM>: BM x 256


RED = ("reduce_partials_kernel", [])

GEMM = [
    # ---- arithmetic 0: the native fp32-MFMA kernel, 128-row tiles, 64 columns for small problems (gemm.hip:tile_n)
    gemm_row("f32_nn", "NN", 300, 200, 100, [_native("0", "0", 64, "true")], arith=0),
    gemm_row("f32_nt", "NT", 300, 200, 100, [_native("0", "1", 64, "true")], arith=0),
    gemm_row("f32_tn", "TN", 300, 200, 100, [_native("1", "0", 64, "true")], arith=0),
    gemm_row("f32_nn_bn128", "NN", 384, 1408, 2048, [_native("0", "0", 128, "true")], arith=0),     # 3 x 11 x 8 = 264 >= 256 tiles
    gemm_row("f32_tn_split", "TN", 128, 64, 512, [_native("1", "0", 64, "true"), RED], arith=0),
    # ---- arithmetic 6 on operands that are not float4-loadable: the native kernel with scalar loads
    gemm_row("x6_unaligned", "NN", 300, 200, 100, [_native("0", "0", 64, "false")], unaligned=True),
    gemm_row("x6_n_not_mult4", "NN", 300, 202, 100, [_native("0", "0", 64, "false")]),
    # ---- arithmetic 6: gemm_x3_kernel with 128-row tiles (small problems), both column tiles, the three layouts
    gemm_row("x3_128_nn", "NN", 300, 200, 100, [_x3("0", "1", 64)]),
    gemm_row("x3_128_nt", "NT", 300, 200, 100, [_x3("0", "0", 64)]),
    gemm_row("x3_128_tn", "TN", 300, 200, 100, [_x3("1", "1", 64)]),
    gemm_row("x3_128_bn128", "NN", 384, 1408, 2048, [_x3("0", "1", 128)]),          # 128-row tiles: 264 tiles; 256-row tiles: 176 < 256
    gemm_row("x3_128_forced", "NN", 4096, 512, 1024, [_x3("0", "1", 128)], override=128),
    gemm_row("x3_seg", "NN", 300, 200, 100, [_x3("0", "1", 64)], seg=True),
    # 64-row tiles: K <= 256, N <= 256, M >= 8192
    gemm_row("x3_64_bn64", "NN", 8192, 64, 64, [_x3("0", "1", 64, bm=64)]),
    gemm_row("x3_64_bn128", "NN", 16384, 256, 64, [_x3("0", "1", 128, bm=64)]),     # 128 x 2 = 256 tiles of 128 x 128: the wide column tile
    gemm_row("x3_m8191_no_64", "NN", 8191, 64, 64, [_x3("0", "1", 64)]),
    # ---- the 256 x 128 wave-specialised kernel: by the rule from 256 tiles x k-slabs on, and by the override at any M > 128, N > 64
    gemm_row("w2_rule", "NN", 4096, 512, 1024, [_w2("0", "1")]),                     # 16 x 4 x 4 = 256
    gemm_row("w2_forced_nn", "NN", 300, 200, 100, [_w2("0", "1")], override=256),
    gemm_row("w2_forced_nt", "NT", 300, 200, 100, [_w2("0", "0")], override=256),
    gemm_row("w2_forced_tn", "TN", 300, 200, 100, [_w2("1", "1")], override=256),
    # ---- the 256-column kernels: by the cost rule and by the override (M > 128, N > 128)
    gemm_row("q256_rule", "NN", 16384, 1024, 192, [_q("0", "1", 256)]),              # 64 x 4 = 256 tiles: one full round, K <= 192
    gemm_row("q192_rule", "NN", 10240, 1024, 192, [_q("0", "1", 192)]),
    gemm_row("q256_colmax", "NN", 10240, 1024, 192, [_q("0", "1", 256)], colmax_rpg=512),   # 512 % 192 != 0: no tile may straddle groups
    gemm_row("q256_forced", "NN", 300, 200, 100, [_q("0", "1", 256)], override=512),
    gemm_row("q192_forced", "NT", 300, 200, 100, [_q("0", "0", 192)], override=448),
    gemm_row("q_forced_n128_w2", "NN", 300, 128, 100, [_w2("0", "1")], override=512),        # N <= 128: no 256-column kernel
    # ---- the streaming kernels of the class dimension
    gemm_row("skinny_nn", "NN", 300, 2, 64, [("skinny_nn_kernel", ["2"])]),
    gemm_row("skinny_tn", "TN", 64, 2, 300, [("skinny_tn_kernel", ["2"]), RED]),
    gemm_row("skinny_nt", "NT", 300, 64, 3, [("skinny_nt_kernel", ["3"])]),
    gemm_row("n5_not_skinny", "NN", 300, 5, 64, [_native("0", "0", 64, "false")]),
    # ---- split-K with its reduction kernel
    gemm_row("split_nn", "NN", 128, 64, 512, [_x3("0", "1", 64), RED]),
    gemm_row("split_tn", "TN", 128, 64, 512, [_x3("1", "1", 64), RED]),
    gemm_row("split_tn_tall", "TN", 640, 384, 4100, [_x3("1", "1", 64), RED]),       # a k-chunk per XCD (plan_splits: zmajor)
    gemm_row("k508_no_split", "NN", 128, 64, 508, [_x3("0", "1", 64)]),
    # ---- arithmetics 9 and 1 once each
    gemm_row("x9", "NN", 300, 200, 100, [_x3("0", "1", 64, np_=9)], arith=9),
    gemm_row("x9_w2", "NN", 300, 200, 100, [_w2("0", "1", np_=9)], arith=9, override=256),
    gemm_row("x1", "NN", 300, 200, 100, [_x3("0", "1", 64, np_=1)], arith=1),
]


# kernels of the sources the coverage test lists that no row can reach through dgcnn_knn_* / dgcnn_gemm_f32 / dgcnn_gemm_seg_f32
NOT_DISPATCHED = {
    "edge_wgrad_smallc_kernel": "launched by dgcnn_edge_mlp_wgrad_f32 (the C <= 4 weight gradient of the edge MLP), not by a GEMM entry",
    "colmax_decode_kernel": "launched by dgcnn_colmax_decode_f32, after the GEMMs of a column-maximum group have all run",
}

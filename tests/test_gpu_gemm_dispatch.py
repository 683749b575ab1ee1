"""Which kernel does a GEMM call launch?  Within one arithmetic every tile kernel gives the same bits (gemm_x3.hip), so a test that
forces a tile passes just as well when gemm.hip:launch<> changes it.  Each row of tests/dispatch_tables.py:GEMM is one case: the
arithmetic and the tile override are set, the call is recorded (tests/launch_trace.py) and
  1. the ordered kernel list is the row's, with the template arguments it names;
  2. the tag dgcnn._engine.gemm gives the call (bench.py's per-kernel table) names the recorded kernel: kernel name, layout words,
     tile numbers and bf16xN;
  3. the product is right against float64 numpy, at the bar the GEMM tests use for that arithmetic: REL_BAR of
     tests/test_gpu_gemm_tiles.py relative to |A| |B|; arithmetic 1 as tests/test_gpu_gemm_modes.py has it, against the product of
     the bf16-rounded operands relative to |A^| |B^|.
Also here: one eager training step recorded whole, which must give a demangled name for every kernel node of the library."""
import re

import numpy as np
import pytest
import torch

from oracle import dgcnn_oracle as O
from gpu_helpers import dev, host
from launch_trace import launches, timed, check_kernels
from test_gpu_gemm_tiles import REL_BAR, tile
import dispatch_tables as T

pytestmark = pytest.mark.gpu

A_WORDS = {"A_ROW": "0", "A_COL": "1"}
B_WORDS = {"B_ROW": "0", "B_COL": "1"}
K_WORDS = {"KCONTIG": "0", "KSTRIDED": "1"}


@pytest.fixture()
def dg():
    import dgcnn
    dgcnn.reset()
    return dgcnn


def check_tag(tag, L, what):
    """The engine's tag against the recorded kernels (a split reduction's reduce_partials_kernel belongs to the call, not the tag).
    The gemm_x3_kernel tag carries the column tile and bf16xN but NOT the row tile (64 or 128): its string is a row name of the
    benchmark's table and keeps its form, so this check cannot tell rows x3_64_bn64 and x3_m8191_no_64 apart -- the table's expected
    template arguments (BM) do."""
    name, args = L[0][0], L[0][1]
    m = re.match(r"^gemm_call\[(.*)\]$", tag)
    if m:                                                    # the streaming kernels: the call's kernels, in order
        ran = ["%s<%s>" % (e[0], ", ".join(e[1])) if e[1] else e[0] for e in L]
        assert m.group(1).split("+") == ran, "%s: the tag says %s, launched %s" % (what, tag, ran)
        return
    m = re.match(r"^(\w+)<(.*)>$", tag)
    assert m and m.group(1) == name, "%s: the tag says %s, launched %s<%s>" % (what, tag, name, ", ".join(args))
    w = m.group(2).split(",")
    if name == "gemm_kernel":                                # <A_*, B_*, STORE, BM, BN> against <ASRC, BSRC, EPI, BM, BN, VEC>
        said = [A_WORDS[w[0]], B_WORDS[w[1]], {"STORE": "0"}[w[2]], w[3], w[4]]
        ran = args[:5]
    elif name == "gemm_x3_kernel":                           # <kinds, BN, bf16xNP> against <AKIND, BKIND, BN, NP, BM>
        said = [K_WORDS[w[0]], K_WORDS[w[1]], w[2], w[3].replace("bf16x", "")]
        ran = args[:4]
    elif name == "gemm_x3w2_kernel":                         # <kinds, bf16xNP> against <AKIND, BKIND, NP>
        said = [K_WORDS[w[0]], K_WORDS[w[1]], w[2].replace("bf16x", "")]
        ran = args[:3]
    else:                                                    # gemm_x3q_kernel<kinds, BM, bf16xNP> against <AKIND, BKIND, NP, BM>
        assert name == "gemm_x3q_kernel", name
        said = [K_WORDS[w[0]], K_WORDS[w[1]], w[3].replace("bf16x", ""), w[2]]
        ran = args[:4]
    assert said == ran, "%s: the tag says %s, launched %s<%s>" % (what, tag, name, ", ".join(args))


@pytest.mark.parametrize("r", T.GEMM, ids=[r["id"] for r in T.GEMM])
def test_gemm_row(dg, r):
    from dgcnn import _engine as E
    M, N, K, layout = r["M"], r["N"], r["K"], r["layout"]
    rng = np.random.default_rng(M + 3 * N + 7 * K)
    A = rng.normal(size=(M, K)).astype(np.float32)
    Bm = rng.normal(size=(K, N)).astype(np.float32)
    As = A.T.copy() if layout == "TN" else A                 # as stored
    Bs = Bm.T.copy() if layout == "NT" else Bm
    if r["unaligned"]:
        buf = torch.full((As.shape[0], As.shape[1] + 1), 777.0, device="cuda")
        buf[:, :As.shape[1]] = dev(As)
        Ad = buf[:, :As.shape[1]]
    else:
        Ad = dev(As)
    Bd = dev(Bs)
    kw = dict(transA=layout == "TN", transB=layout == "NT")
    plus = 0.0
    if r["seg"]:
        sizes = [70, 131, M - 201]
        gb = rng.normal(size=(3, N)).astype(np.float32)
        rg = np.repeat(np.arange(3, dtype=np.int32), sizes)
        kw.update(gbias=dev(gb), row_group=dev(rg))
        plus = gb[rg].astype(np.float64)
    keys = None
    if r["colmax_rpg"]:
        assert M % r["colmax_rpg"] == 0
        keys = torch.zeros((M // r["colmax_rpg"]) * N, dtype=torch.int64, device="cuda")
        kw.update(colmax=keys, colmax_rpg=r["colmax_rpg"])
    C = torch.full((M, N), float("nan"), device="cuda")      # beta = 0 must not read C
    with tile(r["override"], r["arith"]):
        with timed() as rec, launches() as L:
            E.gemm(Ad, Bd, C, **kw)
    print(r["id"], rec[0][0], [(e[0], e[1], e[2]) for e in L])
    check_kernels(L, r["expect"], r["id"])
    assert len(rec) == 1
    check_tag(rec[0][0], L, r["id"])
    if r["arith"] == 1:                                      # plain bf16 operands: the product of the rounded operands
        A, Bm = O.bf16_round(A), O.bf16_round(Bm)
    ref = A.astype(np.float64) @ Bm.astype(np.float64) + plus
    scale = np.abs(A).astype(np.float64) @ np.abs(Bm).astype(np.float64)
    got = host(C).astype(np.float64)
    assert np.isfinite(got).all(), r["id"]
    e = float((np.abs(got - ref) / np.maximum(scale, 1e-30)).max())
    print("%s: %.3e of |A| |B| (bar %.1e)" % (r["id"], e, REL_BAR))
    assert e < REL_BAR, (r["id"], e)
    if keys is not None:                                     # the maximum of every group's own rows, from the epilogue
        from test_gpu_gemm_tiles import assert_colmax, decode
        B = M // r["colmax_rpg"]
        vals, arg = decode(keys, B, N)
        assert_colmax(vals, arg, host(C), B, r["colmax_rpg"], N, r["id"])


BENCH_GEMMS = [   # (layout, M, N, K) of four products of the benchmark's step (B N = 49152 rows), the tag of each, recorded with it
    ("NN", 49152, 1024, 192, "gemm_x3q_kernel<KCONTIG,KSTRIDED,256,bf16x6>"),        # MergedEdgeConv
    ("NN", 49152, 512, 1728, "gemm_x3w2_kernel<KCONTIG,KSTRIDED,bf16x6>"),           # FC0
    ("NN", 49152, 64, 128, "gemm_x3_kernel<KCONTIG,KSTRIDED,64,bf16x6>"),            # conv1 of the last EdgeConv layer
    # the class layer's weight gradient: the one row of the benchmark's table whose name CHANGED -- it read
    # gemm_kernel<A_COL,B_ROW,STORE,128,64>, a kernel the call never launched
    ("TN", 256, 2, 49152, "gemm_call[skinny_tn_kernel<2>+reduce_partials_kernel]"),
]


@pytest.mark.parametrize("layout,M,N,K,tag", BENCH_GEMMS, ids=[g[4].split("<")[0].split("[")[-1] + "-%d" % g[2] for g in BENCH_GEMMS])
def test_tags_at_the_benchmark_shapes(dg, layout, M, N, K, tag):
    """The tag strings of the benchmark's per-kernel table at its own shapes (BASELINE.json configs[1]), as literals, each held against
    the launches of the same call."""
    from dgcnn import _engine as E
    A = torch.ones((K, M) if layout == "TN" else (M, K), device="cuda")
    Bm = torch.ones((K, N), device="cuda")
    C = torch.empty((M, N), device="cuda")
    with tile(0, 6):
        with timed() as rec, launches() as L:
            E.gemm(A, Bm, C, transA=layout == "TN")
    assert [t[0] for t in rec] == [tag]
    check_tag(tag, L, tag)
    assert bool((C == float(K)).all())


def test_the_mirrors_of_the_tile_rule_agree_with_the_launch(dg):
    """dgcnn_gemm_x3_tile_rows / dgcnn_gemm_x3_tile_cols are host mirrors that tools and tests ask; for every float4-loadable row of
    the table without a column maximum (which changes the tile inside gemm.hip:launch<>) they name the tile that was recorded."""
    lib = dg._hip.load()
    for r in T.GEMM:
        name, args = r["expect"][0]
        if not name.startswith("gemm_x3") or r["colmax_rpg"]:
            continue
        with tile(r["override"], r["arith"]):
            rows, cols = lib.dgcnn_gemm_x3_tile_rows(r["M"], r["N"], r["K"]), lib.dgcnn_gemm_x3_tile_cols(r["M"], r["N"], r["K"])
        want = (256, 0) if name == "gemm_x3w2_kernel" else (int(args[-1]), 256 if name == "gemm_x3q_kernel" else 0)   # BM is the last
        assert (rows, cols) == want, (r["id"], rows, cols, want)


# ------------------------------------------------------------------------------------------------------
def test_every_kernel_of_a_training_step_has_a_demangled_name(dg):
    """One eager training step of a small model (the one __graft_entry__.smoke() trains: 2 EdgeConv layers, k = 10, 2 x 256 points;
    zero_gradients, accum_gradient, apply_gradient) recorded whole: every kernel node reads back with a non-empty name that parses
    as a demangled kernel name -- the route from the recorded kernel address to its name works for every kernel such a step
    launches (BatchNorm, edge, loss and optimizer kernels among them), not only the k-NN and GEMM ones."""
    flags = dg.DGCNN_FLAGS(EDGE_CONV_LAYERS=2, EDGE_CONV_FILTERS=[64, 64], KVALUE=10, NUM_CHANNEL=3, FC_FILTERS=[128, 64], TRAIN=True)
    rng = np.random.default_rng(0)
    pts = rng.random((2, 256, 3), dtype=np.float32)
    lab = rng.integers(0, 2, (2, 256)).astype(np.int32)
    tv = dg.trainval(flags).initialize()
    tv.use_graph(False)                                      # eager: a step in plan mode would open the one recorder itself
    with launches() as L:
        tv.zero_gradients(None)
        _, acc, loss = tv.accum_gradient(None, [pts], [lab])
        tv.apply_gradient(None)
    assert np.isfinite(float(loss))
    assert len(L) >= 40, len(L)
    for base, args, g, b, lds in L:
        assert base and re.match(r"^[A-Za-z_]\w*$", base) and not base.startswith("_Z"), "no demangled name: %r" % (base,)
        assert all(x > 0 for x in g + b)
    ran = {e[0] for e in L}
    print(len(L), "kernel nodes,", len(ran), "distinct kernels:", sorted(ran))
    assert {"sqnorm_kernel", "knn_kernel"} <= ran and any(n.startswith("gemm") for n in ran), sorted(ran)


def test_plan_kernel_reads_back_what_was_recorded(dg):
    """dgcnn_plan_kernel on a two-kernel plan: nodes in recorded order with grid, block and LDS bytes, null outputs allowed, the name
    truncated to name_bytes - 1 and NUL-terminated, an index outside [0, kernels) refused."""
    import ctypes
    from dgcnn import _engine as E
    from dgcnn import _hip as H
    lib = H.load()
    x = dev(np.random.default_rng(5).standard_normal((300, 16)).astype(np.float32))
    with H.Plan.record() as plan:
        E.knn(x, 1, 300, 8)
    try:
        assert plan.info()["kernels"] == 2
        ks = plan.kernels()
        assert [k[0].split("(anonymous namespace)::")[1].split("(")[0].split("<")[0] for k in ks] == ["sqnorm_kernel", "knn_mfma_kernel"]
        assert ks[0][1:] == ((5, 1, 1), (256, 1, 1), 4 * 64 * 17) and ks[1][1:] == ((5, 1, 1), (256, 1, 1), 0)
        assert "knn_mfma_kernel<16, 8, true>(float const*" in ks[1][0]
        name = ctypes.create_string_buffer(b"#" * 32, 32)
        assert lib.dgcnn_plan_kernel(plan.handle, 1, name, 12, None, None, None) == 0
        assert name.raw[:12] == ks[1][0].encode()[:11] + b"\0" and name.raw[12:] == b"#" * 20
        for i in (-1, 2):
            assert lib.dgcnn_plan_kernel(plan.handle, i, name, 32, None, None, None) == -1
    finally:
        plan.destroy()

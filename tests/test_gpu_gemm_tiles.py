"""The tile kernels of dgcnn_gemm_f32 one by one (run with -m gpu on an MI355X).

The bf16-split family (csrc/gemm_x3.hip) has five kernels -- gemm_x3_kernel with 64- and 128-row tiles, the 256 x 128
wave-specialised gemm_x3w2_kernel, gemm_x3q_kernel with 256 x 256 and 192 x 256 tiles -- and a cost rule that picks one per
shape.  Here every kernel is forced in turn (dgcnn_gemm_x3_tile_override) and checked against float64 numpy in each layout
(NN, NT, TN), with each epilogue option (beta, per-group bias, BatchNorm column sums, per-group column maximum, strided
output), with split-K, and at ragged shapes whose tails run masked.

All tiles of one arithmetic give the same bits, so which kernel a forced call ran is taken from its recorded launches
(tests/launch_trace.py), not from the host mirrors of the rule (dgcnn_gemm_x3_tile_rows / _cols), which are asserted against the
recording as well."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import dgcnn_oracle as O
from gpu_helpers import dev, host, run_model, set_vars
from launch_trace import launches, names

pytestmark = pytest.mark.gpu

# error / (|A| |B|) of an fp32-class product (test_gpu_parity.py:test_gemm_split_accuracy)
REL_BAR = 2e-6

# (arithmetic, dgcnn_gemm_x3_tile_override): 0 = the cost rule, 128 = gemm_x3_kernel<128>, 256 = gemm_x3w2_kernel (256 x 128),
# 512 = gemm_x3q_kernel<256> (256 x 256), 448 = gemm_x3q_kernel<192> (192 x 256); arithmetics 0 (native fp32 MFMA) and 9 (nine
# partial products) run the cost rule and the 256-row request only (the 256-column kernels run the default arithmetic only)
TILES6 = (0, 128, 256, 512, 448)
CONFIGS = [(6, t) for t in TILES6] + [(0, 0), (0, 256), (9, 0), (9, 256)]
FORCED = {128: (128, 0), 256: (256, 0), 512: (256, 256), 448: (192, 256)}      # override -> (tile rows, 256-column kernel?)


@pytest.fixture()
def dg():
    import dgcnn
    dgcnn.reset()
    return dgcnn


@contextlib.contextmanager
def tile(override, arith=6):
    """Run the block with this arithmetic and tile override; both are restored afterwards."""
    from dgcnn import _hip as H
    lib = H.load()
    prev_arith = H.gemm_arith()
    prev = lib.dgcnn_gemm_x3_tile_override(override)
    try:
        H.set_gemm_arith(arith)
        yield
    finally:
        lib.dgcnn_gemm_x3_tile_override(prev)
        H.set_gemm_arith(prev_arith)


def kernel_name(M, N, K):
    """The kernel dgcnn_gemm_f32 takes for a float4-loadable product under the current arithmetic / override (for messages)."""
    from dgcnn import _hip as H
    lib = H.load()
    if H.gemm_arith() == 0:
        return "gemm_kernel"
    rows, cols = lib.dgcnn_gemm_x3_tile_rows(M, N, K), lib.dgcnn_gemm_x3_tile_cols(M, N, K)
    if cols == 256:
        return "gemm_x3q_kernel<%d>" % rows
    return "gemm_x3w2_kernel" if rows == 256 else "gemm_x3_kernel<%d>" % rows


def launched_name(L):
    """The kernel that formed the product of a recorded dgcnn_gemm_f32 call, in kernel_name's words (a split reduction's
    reduce_partials_kernel follows it)."""
    name, args = L[0][0], L[0][1]
    if name == "gemm_x3q_kernel":                              # <AKIND, BKIND, NP, BM>
        return "gemm_x3q_kernel<%s>" % args[3]
    if name == "gemm_x3_kernel":                               # <AKIND, BKIND, BN, NP, BM>
        return "gemm_x3_kernel<%s>" % args[4]
    return name


def recorded_gemm(A, Bm, C, expect=None, **kw):
    """E.gemm with its launches recorded -> the recording; expect: the kernel (kernel_name's words) that must have formed the product."""
    from dgcnn import _engine as E
    with launches() as L:
        E.gemm(A, Bm, C, **kw)
    if expect is not None:
        assert launched_name(L) == expect, "expected %s, launched %s" % (expect, [(e[0], e[1]) for e in L])
    return L


def check_forced(override, M, N, K, L=None):
    """A forced tile is really the one the library reports for this shape -- and, given the recording L of a call of that shape
    without a column maximum, the one that was launched: for every override and for the cost rule the mirrors name the recorded kernel."""
    from dgcnn import _hip as H
    lib = H.load()
    if override in FORCED and H.gemm_arith() == 6:
        rows, wide = FORCED[override]
        assert lib.dgcnn_gemm_x3_tile_rows(M, N, K) == rows, (override, M, N, K)
        assert lib.dgcnn_gemm_x3_tile_cols(M, N, K) == wide, (override, M, N, K)
        if L is not None:
            forced_name = {128: "gemm_x3_kernel<128>", 256: "gemm_x3w2_kernel", 512: "gemm_x3q_kernel<256>", 448: "gemm_x3q_kernel<192>"}
            assert launched_name(L) == forced_name[override], (override, M, N, K, [(e[0], e[1]) for e in L])
    if L is not None:
        assert launched_name(L) == kernel_name(M, N, K), (override, M, N, K, kernel_name(M, N, K), [(e[0], e[1]) for e in L])


def decode(keys, B, F):
    from dgcnn import _hip as H
    vals = torch.empty((B, F), device="cuda")
    arg = torch.empty((B, F), dtype=torch.int32, device="cuda")
    H.call("dgcnn_colmax_decode_f32", keys.data_ptr(), B * F, vals.data_ptr(), arg.data_ptr())
    return host(vals), host(arg)


def tied_operands(rng, R, Cin, F):
    """Activations with 200 copies of row 0 (exact ties of whole output rows) and a weight whose first three columns are zero
    (every row of those columns ties: the first row must win)."""
    X = rng.normal(size=(R, Cin)).astype(np.float32)
    X[rng.integers(0, R, 200)] = X[0]
    W = rng.normal(0, 0.2, size=(Cin, F)).astype(np.float32)
    W[:, :3] = 0.0
    return X, W


def assert_colmax(vals, arg, T, B, N, F, what):
    Th = T.reshape(B, N, F)
    assert arg.min() >= 0 and arg.max() < N, "%s: arg outside the cloud [%d, %d]" % (what, arg.min(), arg.max())
    bad = np.argwhere((vals != Th.max(1)) | (arg != Th.argmax(1)))
    assert len(bad) == 0, "%s: %d of %d (cloud, column) maxima wrong, first %s: got %r at row %d, numpy %r at row %d" % (
        what, len(bad), B * F, bad[0], vals[tuple(bad[0])], arg[tuple(bad[0])], Th.max(1)[tuple(bad[0])], Th.argmax(1)[tuple(bad[0])])


def assert_colsums(st, C64, slots, what):
    """Column sums / sums of squares of the epilogue (summed over the slots) against float64 sums of the kernel's own output.
    Bar: 1e-5 of sum |c| (fp32 partial sums of a few dozen rows per thread); a missing or doubled row tile is O(1 / tiles)."""
    N = C64.shape[1]
    s = host(st).reshape(slots, 2, N).sum(0)
    for j, ref, mag in ((0, C64.sum(0), np.abs(C64).sum(0)), (1, (C64 ** 2).sum(0), (C64 ** 2).sum(0))):
        err = np.abs(s[j] - ref) / np.maximum(mag, 1e-30)
        assert err.max() < 1e-5, "%s: column %s %.2e of the magnitude (column %d)" % (
            what, ("sums", "sums of squares")[j], err.max(), int(err.argmax()))


# ------------------------------------------------------------------------------------------
# 1. per-cloud column maximum from the GEMM epilogue, on every tile
# ------------------------------------------------------------------------------------------
# what gemm.hip:launch<> is recorded to run under the column maximum, by override: the cost rule (0) and override 448 pick 192 x 256
# for these shapes, and a cloud of 512 or 2048 rows is no multiple of 192, so both must be seen to run 256-row tiles instead
COLMAX_LAUNCHED = {0: "gemm_x3q_kernel<256>", 448: "gemm_x3q_kernel<256>", 128: "gemm_x3_kernel<128>", 256: "gemm_x3w2_kernel",
                   512: "gemm_x3q_kernel<256>"}


@pytest.mark.parametrize("B,N,Cin,F,override", [
    (20, 512, 192, 1024, 0), (12, 2048, 192, 1024, 0), (24, 512, 256, 1024, 0),       # the cost rule picks 192 x 256 here
    (20, 512, 192, 1024, 128), (20, 512, 192, 1024, 256), (20, 512, 192, 1024, 512), (20, 512, 192, 1024, 448)])
def test_column_maximum_on_every_tile(dg, B, N, Cin, F, override):
    """model.py:76-77 max-pool over the points of each cloud, taken in the GEMM's epilogue: a tile's keys go to the cloud of its
    first row, so no tile may straddle two clouds -- clouds of 512 or 2048 points are not whole multiples of 192 rows.  The kernel
    the call is recorded to launch is COLMAX_LAUNCHED's."""
    from dgcnn import _engine as E
    rng = np.random.default_rng(B * N + Cin + override)
    R = B * N
    X, W = tied_operands(rng, R, Cin, F)
    with tile(override):
        if override == 0:
            assert E.H.load().dgcnn_gemm_x3_tile_rows(R, F, Cin) == 192      # (what makes these shapes the interesting ones)
        check_forced(override, R, F, Cin)
        what = "%s (B=%d N=%d Cin=%d, override %d)" % (kernel_name(R, F, Cin), B, N, Cin, override)
        T = torch.empty((R, F), device="cuda")
        keys = torch.zeros(B * F, dtype=torch.int64, device="cuda")
        st = torch.zeros(E.H.stat_slots() * 2 * F, dtype=torch.float64, device="cuda")
        recorded_gemm(dev(X), dev(W), T, expect=COLMAX_LAUNCHED[override], stats=st, colmax=keys, colmax_rpg=N)
        vals, arg = decode(keys, B, F)
    Th = host(T)
    assert_colmax(vals, arg, Th, B, N, F, what)
    assert_colsums(st, Th.astype(np.float64), E.H.stat_slots(), what)
    ref = X.astype(np.float64) @ W.astype(np.float64)
    err = np.abs(Th - ref) / (np.abs(X) @ np.abs(W) + 1e-30)
    assert err.max() < REL_BAR, (what, float(err.max()))


def test_headline_merged_edgeconv_keeps_its_tile(dg):
    """configs[1] (24 x 2048 points, K = 192): MergedEdgeConv's product keeps the 256 x 256 tile, with or without the maximum."""
    lib = dg._hip.load()
    with tile(0):
        assert (lib.dgcnn_gemm_x3_tile_rows(49152, 1024, 192), lib.dgcnn_gemm_x3_tile_cols(49152, 1024, 192)) == (256, 256)


# ------------------------------------------------------------------------------------------
# 2. the layer and the model at a shape that takes the 192-row tile
# ------------------------------------------------------------------------------------------
def test_merged_edgeconv_global_feature_at_a_192_row_shape(dg):
    """conv_bn_act(gmax=(B, N)) as MergedEdgeConv runs it (R x 1024, K = 192): the per-cloud maximum of its own GEMM output, the
    arg-max the backward scatters through, and the normalised global feature."""
    from dgcnn import _engine as E
    B, N, Cin, F = 20, 512, 192, 1024
    R = B * N
    rng = np.random.default_rng(11)
    X, W = tied_operands(rng, R, Cin, F)
    beta = rng.normal(0, 0.2, F).astype(np.float32)
    c = dg.ctx()
    c.begin_step()
    c.get_variable("MergedEdgeConv/weights", (Cin, F))
    c.get_variable("MergedEdgeConv/BatchNorm/beta", (F,))
    set_vars(dg, {"MergedEdgeConv/weights": W, "MergedEdgeConv/BatchNorm/beta": beta})
    x = c.new_buffer(R, Cin)
    x.copy_(dev(X))
    seen = {}
    orig = E.gemm

    def spy(A, Bm, C, *a, **kw):                 # the layer's own pre-BatchNorm tensor T and its key buffer
        orig(A, Bm, C, *a, **kw)
        if kw.get("colmax") is not None:
            seen["T"], seen["keys"] = C, kw["colmax"]
    E.gemm = spy
    try:
        out, g = E.conv_bn_act(x, "MergedEdgeConv", F, relu=True, gmax=(B, N))
    finally:
        E.gemm = orig
    assert "keys" in seen, "MergedEdgeConv's max-pool did not come from the GEMM epilogue"
    Th = host(seen["T"])
    vals, arg = decode(seen["keys"], B, F)
    assert_colmax(vals, arg, Th, B, N, F, "conv_bn_act(gmax=(%d, %d))" % (B, N))
    T64 = Th.astype(np.float64)
    mean, var = T64.mean(0), T64.var(0)
    g_ref = np.maximum((T64.reshape(B, N, F).max(1) - mean) / np.sqrt(var + E.BN_EPS) + beta, 0.0)
    np.testing.assert_allclose(host(g), g_ref, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(host(g), host(out).reshape(B, N, F).max(1), rtol=0, atol=1e-5)


def test_model_logits_at_a_192_row_shape(dg):
    """dgcnn 3 x (64, 64, 128) + FC (512, 256) at B = 20, N = 512: MergedEdgeConv (10240 x 1024, K = 256) takes the 192 x 256 tile by
    the cost rule.  Inference logits against the oracle fed the HIP path's graphs (test_gpu_parity.py:test_model_logits_and_gradients)."""
    import dgcnn
    B, N, C, k = 20, 512, 3, 20
    assert dgcnn._hip.load().dgcnn_gemm_x3_tile_rows(B * N, 1024, 64 + 64 + 128) == 192
    flags = dg.DGCNN_FLAGS(MODEL_NAME="dgcnn", EDGE_CONV_LAYERS=3, EDGE_CONV_FILTERS=[64, 64, 128], KVALUE=k, NUM_CLASS=2,
                           FC_LAYERS=2, FC_FILTERS=[512, 256], TRAIN=False, NUM_CHANNEL=C)
    rng = np.random.default_rng(0)
    pts = rng.random((B, N, C), dtype=np.float32)
    params = O.init_params(flags, C, seed=1)
    for n in params:
        if n.endswith("beta"):
            params[n] = rng.normal(0, 0.2, params[n].shape).astype(np.float32)
    _, _, cap = run_model(dg, flags, pts, params, train=False)
    idx_list = []
    for i in range(3):
        xin, idx = cap["EdgeConv%d" % i]
        np.testing.assert_array_equal(idx, O.k_nn(xin, k))
        idx_list.append(idx)
    logits_ref, _ = O.model_forward(pts, flags, params, idx_list=idx_list)
    dg.ctx().recording = False
    logits = host(dgcnn.build(dev(pts), flags))
    err = np.abs(logits - logits_ref)
    assert err.max() <= 1e-3, "logits differ from the oracle: max %g at %s" % (err.max(), np.unravel_index(err.argmax(), err.shape))


# ------------------------------------------------------------------------------------------
# 3. + 4. tile x layout x epilogue against float64; bit identity of the three big kernels
# ------------------------------------------------------------------------------------------
# ragged: M not a multiple of 64 / 192 / 256, N not of 128 / 256, K a multiple of 4 but not of 16 / 32 (the float4 path with masked
# tails).  The cost rule alone picks q192, w2, w2, w2 and 128 for these.  K < 512 keeps TN unsplit (plan_splits: s <= K / 256).
RAGGED = [(9000, 1000, 200), (6000, 520, 1028), (12000, 1216, 204), (14000, 192, 1020), (4100, 300, 1220)]
RPG = 1000                                                     # per-group bias: not a multiple of any tile height


class Problem(object):
    """Operands in every stored layout and the float64 reference (on the device, for cheap comparisons)."""

    def __init__(self, M, N, K, seed):
        rng = np.random.default_rng(seed)
        A = rng.normal(size=(M, K)).astype(np.float32)
        Bm = rng.normal(size=(K, N)).astype(np.float32)
        self.M, self.N, self.K = M, N, K
        self.A, self.At = dev(A), dev(A.T.copy())
        self.B, self.Bt = dev(Bm), dev(Bm.T.copy())
        self.ref = dev(A.astype(np.float64) @ Bm.astype(np.float64))
        self.scale = dev((np.abs(A) @ np.abs(Bm)).astype(np.float64))

    def operands(self, layout):
        return {"NN": (self.A, self.B, {}), "NT": (self.A, self.Bt, {"transB": True}), "TN": (self.At, self.B, {"transA": True})}[layout]

    def rel_err(self, C, plus=None):
        ref = self.ref if plus is None else self.ref + plus
        d = C.double() - ref
        assert bool(torch.isfinite(d).all()), "non-finite outputs"
        return float((d.abs() / self.scale).max())


@pytest.mark.parametrize("M,N,K", RAGGED)
def test_tiles_layouts_epilogues_against_float64(dg, M, N, K):
    from dgcnn import _engine as E
    P = Problem(M, N, K, M + N + K)
    rng = np.random.default_rng(K)
    C0 = dev(rng.normal(size=(M, N)).astype(np.float32))
    G = -(-M // RPG)
    gb_host = rng.normal(size=(G, N)).astype(np.float32)
    bias = dev(np.repeat(gb_host, RPG, 0)[:M].astype(np.float64))
    gbuf = {True: torch.zeros((G, N + 4), device="cuda"), False: torch.zeros((G, N + 1), device="cuda")}   # ldgbias % 4 == 0 / not
    for v in gbuf.values():
        v[:, :N] = dev(gb_host)
    big = {}                                                   # layout -> {override: C} of the three big kernels
    for arith, override in CONFIGS:
        with tile(override, arith):
            check_forced(override, M, N, K)
            kname = kernel_name(M, N, K)
            for layout in ("NN", "NT", "TN"):
                A, Bm, tr = P.operands(layout)
                what = "%s %s arith %d override %d (%d, %d, %d)" % (layout, kname, arith, override, M, N, K)
                C = torch.full((M, N), float("nan"), device="cuda")         # beta = 0 must not read C
                check_forced(override, M, N, K, recorded_gemm(A, Bm, C, **tr))
                e = P.rel_err(C)
                assert e < REL_BAR, (what, "beta 0", e)
                if arith == 6 and override in (256, 512, 448):
                    big.setdefault(layout, {})[override] = C
                C1 = C0.clone()
                E.gemm(A, Bm, C1, beta=1.0, **tr)
                e = P.rel_err(C1, C0.double())
                assert e < REL_BAR, (what, "beta 1", e)
            # per-group bias (groups straddle tiles), column sums and a strided output slice -- NN with a float4-aligned bias row
            # stride and output, NT with neither (scalar bias loads and stores)
            for layout, aligned in (("NN", True), ("NT", False)):
                A, Bm, tr = P.operands(layout)
                what = "%s %s arith %d override %d (%d, %d, %d) gbias/stats/slice" % (layout, kname, arith, override, M, N, K)
                lo, pad = (4, 8) if aligned else (1, 3)
                outw = torch.zeros((M, N + pad), device="cuda")
                C = outw[:, lo:lo + N]
                gb = gbuf[aligned][:, :N]
                st = torch.zeros(E.H.stat_slots() * 2 * N, dtype=torch.float64, device="cuda")
                recorded_gemm(A, Bm, C, expect=kname, gbias=gb, rpg=RPG, stats=st, **tr)
                e = P.rel_err(C, bias)
                assert e < REL_BAR, (what, e)
                assert not bool(outw[:, :lo].any()) and not bool(outw[:, lo + N:].any()), (what, "wrote outside its columns")
                assert_colsums(st, host(C).astype(np.float64), E.H.stat_slots(), what)
    # gemm_x3.hip: the 256 x 128 wave-specialised kernel and both 256-column kernels keep the same per-element k order
    for layout, outs in big.items():
        if layout == "TN" and K >= 512:
            continue                                           # (split-K: the plan depends on the tile)
        for o in (512, 448):
            if not torch.equal(outs[256], outs[o]):
                d = (outs[256] - outs[o]).abs()
                raise AssertionError("%s (%d, %d, %d): override %d differs from gemm_x3w2_kernel in %d elements, max %g" % (
                    layout, M, N, K, o, int((d != 0).sum()), float(d.max())))


# ------------------------------------------------------------------------------------------
# 5. split-K: zmajor and z-grid plans, reduce_partials with beta, workspace too small
# ------------------------------------------------------------------------------------------
# plan_splits (gemm.hip) on these, every tile: NN (256, 512, 4096) and TN (640, 384, 4100) take a zmajor plan (8 or more k-chunks,
# one XCD each) under the bf16 split; NN (300, 260, 1500) and TN (520, 300, 1020) a plain z-grid of 3 - 5 chunks; the native
# arithmetic always a plain z-grid.  K = 4100 / 1020 / 1500 leave a ragged last chunk.
@pytest.mark.parametrize("M,N,K,layout", [(256, 512, 4096, "NN"), (300, 260, 1500, "NN"), (640, 384, 4100, "TN"), (520, 300, 1020, "TN")])
def test_split_k_on_every_tile(dg, M, N, K, layout):
    from dgcnn import _engine as E
    P = Problem(M, N, K, M * 3 + K)
    C0 = dev(np.random.default_rng(N).normal(size=(M, N)).astype(np.float32))
    A, Bm, tr = P.operands(layout)
    for arith, override in [(6, t) for t in TILES6] + [(0, 0)]:
        with tile(override, arith):
            what = "%s %s arith %d override %d (%d, %d, %d)" % (layout, kernel_name(M, N, K), arith, override, M, N, K)
            C = torch.full((M, N), float("nan"), device="cuda")
            L = recorded_gemm(A, Bm, C, **tr)
            check_forced(override, M, N, K, L)
            assert names(L)[1:] == ["reduce_partials_kernel"], (what, "not a split reduction", names(L))
            e = P.rel_err(C)
            assert e < REL_BAR, (what, "beta 0", e)
            C1 = C0.clone()
            E.gemm(A, Bm, C1, beta=1.0, **tr)
            e = P.rel_err(C1, C0.double())
            assert e < REL_BAR, (what, "beta 1", e)


@pytest.mark.parametrize("layout", ["NN", "TN"])
def test_split_k_workspace_too_small(dg, layout):
    """A split plan whose partials do not fit the workspace is refused (DGCNN_ENOSPC, with a message) before anything runs."""
    from dgcnn import _hip as H
    M, N, K = (256, 512, 4096) if layout == "NN" else (640, 384, 4100)
    rng = np.random.default_rng(3)
    A = dev(rng.normal(size=(K, M) if layout == "TN" else (M, K)).astype(np.float32))
    Bm = dev(rng.normal(size=(K, N)).astype(np.float32))
    C0 = rng.normal(size=(M, N)).astype(np.float32)
    C = dev(C0)
    ws = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    with pytest.raises(H.HipError, match=r"\(-3\).*workspace too small"):
        H.call("dgcnn_gemm_f32", int(layout == "TN"), 0, M, N, K, A.data_ptr(), H.ld2(A), Bm.data_ptr(), H.ld2(Bm),
               C.data_ptr(), H.ld2(C), 1.0, 0, 0, 0, 0, 0, 0, ws.data_ptr(), ws.numel())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(host(C), C0)


# ------------------------------------------------------------------------------------------
# 6. statistics slots: one writer per slot in the reproducible configuration
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,transB,colmax_rpg", [(9000, 1000, 200, 0, 0), (14000, 192, 1020, 1, 0), (10240, 1024, 192, 0, 512)])
def test_stat_writers_cover_the_row_tiles(dg, M, N, K, transB, colmax_rpg):
    """dgcnn_gemm_stat_writers >= the row tiles the launch uses, on every tile (it cannot see colmax, which never takes the
    192-row tile: it then over-counts); a launch with that many slots is accepted (the library refuses one with too few) and
    its sums are right."""
    from dgcnn import _engine as E
    H = E.H
    lib = H.load()
    P = Problem(M, N, K, M + K)
    A, Bm, tr = P.operands("NT" if transB else "NN")
    B = M // colmax_rpg if colmax_rpg else 0
    prev_slots = H.stat_slots()
    try:
        for arith, override in CONFIGS:
            with tile(override, arith):
                what = "%s arith %d override %d (%d, %d, %d)" % (kernel_name(M, N, K), arith, override, M, N, K)
                writers = lib.dgcnn_gemm_stat_writers(transB, M, N, K, A.data_ptr(), H.ld2(A), Bm.data_ptr(), H.ld2(Bm))
                rows = lib.dgcnn_gemm_x3_tile_rows(M, N, K) if arith else 128
                if colmax_rpg and colmax_rpg % rows:
                    rows = 256
                assert writers >= -(-M // rows), (what, writers, rows)
                slots = max(32, writers)
                H.set_stat_slots(slots)
                st = torch.zeros(slots * 2 * N, dtype=torch.float64, device="cuda")
                C = torch.empty((M, N), device="cuda")
                keys = torch.zeros(max(B, 1) * N, dtype=torch.int64, device="cuda")
                # (a group of 512 rows is no multiple of the 192-row tile: gemm.hip:launch<> takes 256 x 256 instead)
                straddles = arith == 6 and colmax_rpg and colmax_rpg % lib.dgcnn_gemm_x3_tile_rows(M, N, K)
                launched = "gemm_x3q_kernel<256>" if straddles else kernel_name(M, N, K)
                recorded_gemm(A, Bm, C, expect=launched, stats=st, colmax=keys if B else None, colmax_rpg=colmax_rpg, **tr)
                e = P.rel_err(C)
                assert e < REL_BAR, (what, e)
                assert_colsums(st, host(C).astype(np.float64), slots, what)
                if B:
                    vals, arg = decode(keys, B, N)
                    assert_colmax(vals, arg, host(C), B, colmax_rpg, N, what)
    finally:
        H.set_stat_slots(prev_slots)

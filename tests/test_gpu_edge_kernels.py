"""Every kernel that indexes through the k-NN graph idx (B, N, k), called through its C entry point and checked against
tests/edge_reference.py (run with -m gpu on an MI355X):

  dgcnn_edge_mlp_f32 / dgcnn_edge_nbr_gemm_f32                  gemm_kernel<A_EDGE>: float4 and scalar loader, 64- and 128-column tiles
  dgcnn_edge_mlp_wgrad_f32 / dgcnn_edge_nbr_wgrad_f32           edge_wgrad_smallc_kernel; gemm_kernel<A_EDGE_T>, split and unsplit K
  dgcnn_edge_mlp_dgrad_scatter_f32                              gemm_kernel<.., E_SCATTER>
  dgcnn_edge_gather_f32 / dgcnn_edge_gather_bwd_f32             the explicit edge tensor and its transpose
  dgcnn_edge_csr_build / dgcnn_edge_csr_sort                    csr_cloud_kernel (LDS) and csr_count / scan / fill (fallback)
  dgcnn_edge_gather_sum_f32 / dgcnn_edge_gather_sum_bf16        sums over incoming edges
  dgcnn_round_bf16_f32

Their typical bug reads or writes a WRONG ROW -- a dropped cloud offset, a wrong edge -> point division, a lost tail of a bucket or
of a chunk -- which faults nothing and hides inside a model-level tolerance.  So every sum is checked in two tiers:

* LATTICE operands (small integers, multiples of 1/8; edge_reference.lattice_precondition is asserted for every case in
  tests/test_edge_reference.py): every partial sum is exact in fp32, the kernel must EQUAL float64 whatever its order of
  additions or of atomics, and one wrong term among thousands shows.
* RANDOM operands: |err| <= (n_terms + 8) 2^-24 sum |term| (bn_reference.sum_bound: fp32 summation in any order plus the
  roundings inside a term), n_terms the reduction length of that output element.  The edge forms always run the native fp32
  gemm_kernel (launch<>: `plain` is false for them), so no bf16-split term enters.  The worst ratio per kernel is printed at
  the end of the module ($DGCNN_EDGE_ERROR_TABLE writes it; profiles/edge_kernel_errors.txt holds a measured copy).

Clouds differ from each other (x offset per cloud, every graph drawn per cloud), B > 1 runs with the `last` and `hub` graphs,
outputs are NaN-filled where beta = 0, and every buffer sits between sentinel guards (gpu_helpers.Guard)."""
import numpy as np
import pytest
import torch

import bn_reference as BR
import edge_reference as ER
from gpu_helpers import Guard, RATIOS, SENT, host, note_ratio, ptr, ratio_table

pytestmark = pytest.mark.gpu

NAN = float("nan")
MINE = set()              # the kernels this module recorded in RATIOS
HEADER = ["# worst |hip - float64| / (2^-24 * sum |term|) per output element over the random-input cases of tests/test_gpu_edge_kernels.py;",
          "# n_terms = the longest reduction of the case that gave the worst ratio; bound = n_terms + 8 (any-order fp32 summation plus",
          "# the roundings inside a term).  Elements with a shorter reduction are held to their own n_terms + 8: their ratio is scaled",
          "# by (n_terms + 8) / (own n_terms + 8) before the comparison."]


@pytest.fixture()
def dg():
    import dgcnn
    dgcnn.reset()
    return dgcnn


@pytest.fixture(scope="module", autouse=True)
def _error_table():
    yield
    ratio_table(header=HEADER, env="DGCNN_EDGE_ERROR_TABLE", names=sorted(MINE & set(RATIOS)))


def cdiv(a, b):
    return -(-a // b)


def exact(what, got, ref):
    got = np.asarray(got, np.float64)
    bad = np.argwhere(~(got == ref))
    assert len(bad) == 0, "%s: %d of %d elements differ from float64 on the lattice, first %s: got %r, float64 %r" % (
        what, len(bad), got.size, bad[0], got[tuple(bad[0])], ref[tuple(bad[0])])


def within(kernel, got, ref, scale, n_terms):
    """|got - ref| <= (n + 8) 2^-24 scale element by element, n broadcast against the output."""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), "%s: non-finite outputs" % kernel
    n = np.asarray(n_terms, np.float64)
    nmax = int(n.max())
    MINE.add(kernel)
    note_ratio(kernel, got - ref, np.asarray(scale, np.float64) * ((n + 8) / (nmax + 8)), nmax, nmax + 8)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def put_cols(g, a, lay):
    """a (rows, W) as a device matrix: "dense", or a column slice of a wider buffer of other values -- "aligned" (offset 4
    floats, leading dimension W + 8: stays float4-loadable when W % 4 == 0) or "unaligned" (offset 1 float, W + 3).
    -> (view, leading dimension)"""
    rows, W = a.shape
    if lay == "dense":
        return g.put(a), W
    lo, ld = (4, W + 8) if lay == "aligned" else (1, W + 3)
    wide = (100 * np.random.default_rng(W + rows).normal(size=(rows, ld))).astype(np.float32)
    wide[:, lo:lo + W] = a
    return g.put(wide)[:, lo:lo + W], ld


def assert_colsums(st, Y64, what):
    """Column sums / sums of squares of the epilogue (summed over the slots) against float64 sums of the kernel's own output, as
    test_gpu_gemm_tiles.py:assert_colsums: 1e-5 of the magnitude; a missing or doubled row tile is O(1 / tiles)."""
    s = host(st).sum(0)
    for j, ref, mag in ((0, Y64.sum(0), np.abs(Y64).sum(0)), (1, (Y64 ** 2).sum(0), (Y64 ** 2).sum(0))):
        err = np.abs(s[j] - ref) / np.maximum(mag, 1e-30)
        assert err.max() < 1e-5, "%s: column %s %.2e of the magnitude (column %d)" % (
            what, ("sums", "sums of squares")[j], err.max(), int(err.argmax()))


def tiers(seed, B, N, C, k, F, kind, need):
    """The lattice operands of a case (same seed and same `need` as tests/test_edge_reference.py, which checks the lattice
    precondition on them) and random ones."""
    for lattice in (True, False):
        yield ER.Operands(lattice, seed + (0 if lattice else 1000), B, N, C, k, F, kind, need=need)


# ------------------------------------------------------------------------------------------------------------ forward forms
def tile_n(M, N, K):
    """gemm.hip:tile_n -- 128 columns, or 64 for narrow outputs and for problems of fewer than 256 tiles."""
    return 64 if (N <= 64 or cdiv(M, 128) * cdiv(N, 128) * cdiv(K, 256) < 256) else 128


WIDE_TILE = (2, 1024, 64, 16, 128, "random")


@pytest.mark.parametrize("lay", ["dense", "aligned", "unaligned"])
@pytest.mark.parametrize("case", ER.FWD_CASES, ids=ER.case_id)
def test_forward_forms(dg, case, lay):
    """Y = [x_i, x_j - x_i] W0 (literal) and x_j Wb + U[point] (factored), with and without the BatchNorm column sums; x and U
    dense, or column slices of wider buffers (aligned: the float4 loader where C % 4 == 0; one float off: the scalar one)."""
    from dgcnn import _hip as H
    B, N, C, k, F, kind = case
    Me = B * N * k
    want_bn = 128 if case == WIDE_TILE else 64
    assert tile_n(Me, F, 2 * C) == want_bn and tile_n(Me, F, C) == want_bn      # the case sits on the tile width it is meant for
    assert Me % 128 != 0 or case == WIDE_TILE
    for o in tiers(ER.case_seed(case), *case, need=("W0", "U")):
        g = Guard()
        x, ldx = put_cols(g, o.x, lay)
        U, ldu = put_cols(g, o.U, lay)
        idx, W0, Wb = g.put(o.idx), g.put(o.W0), g.put(o.W0[C:])
        forms = {"edge_mlp_f32": ER.mlp64(o.x, o.idx, o.W0) + (2 * C,),
                 "edge_nbr_gemm_f32": ER.nbr_gemm64(o.x, o.idx, o.W0[C:], o.U) + (C + 1,)}
        for form, (ref, scale, n_terms) in forms.items():
            outs = []
            for with_stats in (True, False):
                what = "%s %s %s lattice=%d stats=%d" % (form, case, lay, o.lattice, with_stats)
                Y = g.new((Me, F))
                Y.fill_(NAN)                                                     # beta = 0: the kernel must not read Y
                st = g.zeros((H.stat_slots(), 2, F), torch.float64) if with_stats else None
                if form == "edge_mlp_f32":
                    H.call("dgcnn_edge_mlp_f32", x.data_ptr(), ldx, idx.data_ptr(), W0.data_ptr(), B, N, C, k, F, Y.data_ptr(), ptr(st))
                else:
                    H.call("dgcnn_edge_nbr_gemm_f32", x.data_ptr(), ldx, idx.data_ptr(), Wb.data_ptr(), U.data_ptr(), ldu, B, N, C, k, F,
                           Y.data_ptr(), ptr(st))
                Yh = host(Y)
                if o.lattice:
                    exact(what, Yh, ref)
                else:
                    within(form, Yh, ref, scale, n_terms)
                if with_stats:
                    assert_colsums(st, Yh.astype(np.float64), what)
                outs.append(Yh)
            np.testing.assert_array_equal(outs[0], outs[1])                     # the statistics epilogue does not change Y
        g.check()


# --------------------------------------------------------------------------------------------------------- weight gradients
def smallc_blocks(Me):
    """gemm.hip: the small-C kernel (C <= 4, F <= 256) runs one block per 64 edges, 1024 blocks at the most."""
    return cdiv(Me, 64) if Me < 1024 * 64 else 1024


def native_splits(M, N, K):
    """gemm.hip:plan_splits for the native fp32 kernel: ~1024 workgroups, k-chunks of at least 256 (a multiple of 32)."""
    tiles = cdiv(M, 128) * cdiv(N, tile_n(M, N, K))
    s = max(1, min(cdiv(1024, tiles), max(K // 256, 1)))
    chunk = cdiv(cdiv(K, s), 32) * 32
    return cdiv(K, chunk)


def run_wgrad(H, g, o, nbr, beta, lay, ws_bytes):
    B, N, C, k, F = o.B, o.N, o.C, o.k, o.F
    rows = C if nbr else 2 * C
    rng = np.random.default_rng(o.Me + rows)
    dW0 = (rng.integers(-16, 17, (rows, F)) / 8.0 if o.lattice else rng.normal(size=(rows, F))).astype(np.float32)
    x, ldx = put_cols(g, o.x, lay)
    idx, dY = g.put(o.idx), g.put(o.dY)
    dW = g.put(dW0)
    if beta == 0:
        dW.fill_(NAN)
    ws = g.new((ws_bytes,), torch.uint8, fill=7)
    H.call("dgcnn_edge_nbr_wgrad_f32" if nbr else "dgcnn_edge_mlp_wgrad_f32", x.data_ptr(), ldx, idx.data_ptr(), dY.data_ptr(),
           B, N, C, k, F, dW.data_ptr(), float(beta), ws.data_ptr(), ws_bytes)
    ref, scale = (ER.nbr_wgrad64 if nbr else ER.wgrad64)(o.x, o.idx, o.dY)
    if beta:
        ref, scale = ref + beta * dW0.astype(np.float64), scale + np.abs(dW0)
    return host(dW), ref, scale, o.Me + (1 if beta else 0)


@pytest.mark.parametrize("beta", [0, 1])
@pytest.mark.parametrize("case", ER.WGRAD_SMALLC, ids=ER.case_id)
def test_weight_gradients_small_c(dg, case, beta):
    """edge_wgrad_smallc_kernel + reduce_partials: dW0 = E^T dY and dWb = x_j^T dY at chunk boundaries (Me = 1, 63, 64, 65, and
    65540 = 1024 ragged chunks), with a workspace of exactly the bytes the call needs, between guards."""
    from dgcnn import _hip as H
    B, N, C, k, F, kind = case
    assert C <= 4 and F <= 256
    lay = "dense" if beta == 0 else "unaligned"
    for o in tiers(ER.case_seed(case), *case, need=("W0", "dY")):
        for nbr in (False, True):
            g = Guard()
            need = smallc_blocks(o.Me) * (C if nbr else 2 * C) * F * 4
            what = "%s wgrad small C %s beta=%d lattice=%d" % ("nbr" if nbr else "mlp", case, beta, o.lattice)
            got, ref, scale, n_terms = run_wgrad(H, g, o, nbr, beta, lay, need)
            if o.lattice:
                exact(what, got, ref)
            else:
                within("edge_%s_wgrad_f32 (small C)" % ("nbr" if nbr else "mlp"), got, ref, scale, n_terms)
            g.check()


SPLIT = {case: case[0] * case[1] * case[3] >= 512 for case in ER.WGRAD_GEMM}


@pytest.mark.parametrize("beta", [0, 1])
@pytest.mark.parametrize("case", ER.WGRAD_GEMM, ids=ER.case_id)
def test_weight_gradients_gemm(dg, case, beta):
    """gemm_kernel<A_EDGE_T> (scalar at C = 3, float4 at C = 64 and 20), without a split of the edge dimension (Me / 256 < 2:
    plan_splits allows one chunk only) and with one (Me / 256 >= 2 and far fewer than 1024 tiles: several chunks under either
    arithmetic's plan)."""
    from dgcnn import _hip as H
    B, N, C, k, F, kind = case
    Me = B * N * k
    assert C > 4 or F > 256
    for nbr in (False, True):
        s = native_splits(C if nbr else 2 * C, F, Me)
        assert (s > 1 and Me // 256 >= 2) if SPLIT[case] else (s == 1 and Me // 256 < 2), (case, s)
    lay = "dense" if beta == 0 else "aligned"
    for o in tiers(ER.case_seed(case), *case, need=("W0", "dY")):
        for nbr in (False, True):
            g = Guard()
            rows = C if nbr else 2 * C
            ws_bytes = max(Me // 256, 1) * rows * F * 4                          # no plan has more chunks than K / 256
            what = "%s wgrad gemm %s beta=%d lattice=%d" % ("nbr" if nbr else "mlp", case, beta, o.lattice)
            got, ref, scale, n_terms = run_wgrad(H, g, o, nbr, beta, lay, ws_bytes)
            if o.lattice:
                exact(what, got, ref)
            else:
                within("edge_%s_wgrad_f32 (gemm%s)" % ("nbr" if nbr else "mlp", ", split K" if SPLIT[case] else ""), got, ref, scale, n_terms)
            g.check()


@pytest.mark.parametrize("case", [ER.WGRAD_SMALLC[3]] + [c for c in ER.WGRAD_GEMM if SPLIT[c]], ids=ER.case_id)
def test_weight_gradient_workspace_too_small(dg, case):
    """One byte less than the partial tiles need: DGCNN_ENOSPC and an untouched output; exactly the bytes: the right answer.
    The GEMM path runs under the native arithmetic here, whose plan native_splits restates."""
    from dgcnn import _hip as H
    B, N, C, k, F, kind = case
    Me = B * N * k
    small = C <= 4 and F <= 256
    prev = H.gemm_arith()
    H.set_gemm_arith(0)
    try:
        o = ER.Operands(False, ER.case_seed(case) + 1000, B, N, C, k, F, kind, need=("W0", "dY"))
        for nbr in (False, True):
            rows = C if nbr else 2 * C
            name = "dgcnn_edge_nbr_wgrad_f32" if nbr else "dgcnn_edge_mlp_wgrad_f32"
            need = (smallc_blocks(Me) if small else native_splits(rows, F, Me)) * rows * F * 4
            g = Guard()
            x, idx, dY = g.put(o.x), g.put(o.idx), g.put(o.dY)
            dW = g.new((rows, F))
            dW.fill_(5.0)
            ws = g.new((need,), torch.uint8, fill=7)
            args = (x.data_ptr(), C, idx.data_ptr(), dY.data_ptr(), B, N, C, k, F, dW.data_ptr(), 1.0, ws.data_ptr())
            with pytest.raises(H.HipError, match=r"\(-3\).*workspace too small"):
                H.call(name, *args, need - 1)
            torch.cuda.synchronize()
            assert (host(dW) == 5.0).all(), "%s: a refused call changed dW" % name
            H.call(name, *args, need)
            ref, scale = (ER.nbr_wgrad64 if nbr else ER.wgrad64)(o.x, o.idx, o.dY)
            within("edge_%s_wgrad_f32 (%s)" % ("nbr" if nbr else "mlp", "small C" if small else "gemm, split K"), host(dW), ref + 5.0,
                   scale + 5.0, Me + 1)
            g.check()
    finally:
        H.set_gemm_arith(prev)


# ------------------------------------------------------------------------------------------------ scatter / explicit gather
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("case", ER.SCATTER_CASES, ids=ER.case_id)
def test_dgrad_scatter(dg, case, wide):
    """dx[nbr(e)] += dY[e] W0[C:]^T by fp32 atomics onto a non-zero dx (a column slice when lddx > C): exact on the lattice
    whatever the order of the atomics; n_terms = F * in-degree (+ 1 for the prior dx)."""
    from dgcnn import _hip as H
    B, N, C, k, F, kind = case
    lddx = C + 3 if wide else C
    for o in tiers(ER.case_seed(case), *case, need=("W0", "dY", "dx0")):
        g = Guard()
        buf = np.full((o.R, lddx), 3.0, np.float32)
        buf[:, :C] = o.dx0
        dx, dY, W0, idx = g.put(buf), g.put(o.dY), g.put(o.W0), g.put(o.idx)
        H.call("dgcnn_edge_mlp_dgrad_scatter_f32", dY.data_ptr(), W0.data_ptr(), idx.data_ptr(), B, N, C, k, F, dx.data_ptr(), lddx)
        got = host(dx)
        assert (got[:, C:] == 3.0).all(), "wrote outside its columns"
        ref, scale = ER.scatter64(o.dY, o.W0, o.idx)
        ref, scale = ref + o.dx0, scale + np.abs(o.dx0)
        what = "dgrad_scatter %s lddx=%d lattice=%d" % (case, lddx, o.lattice)
        if o.lattice:
            exact(what, got[:, :C], ref)
        else:
            within("edge_mlp_dgrad_scatter_f32", got[:, :C], ref, scale, F * ER.in_degrees(o.idx)[:, None] + 1)
        g.check()


@pytest.mark.parametrize("lay", ["dense", "aligned", "unaligned"])
@pytest.mark.parametrize("case", ER.GATHER_CASES, ids=ER.case_id)
def test_edge_gather_and_its_transpose(dg, case, lay):
    """dgcnn_edge_gather_f32 == edges32 bit for bit (x dense or a column slice); dgcnn_edge_gather_bwd_f32 adds its transpose
    onto a non-zero dx: n_terms = k (centre) + in-degree (neighbour) + 1."""
    from dgcnn import _hip as H
    B, N, C, k, kind = case
    for o in tiers(ER.case_seed(case), B, N, C, k, 4, kind, need=("dE", "dx0")):
        g = Guard()
        x, ldx = put_cols(g, o.x, lay)
        idx = g.put(o.idx)
        E = g.new((o.Me, 2 * C))
        E.fill_(NAN)
        H.call("dgcnn_edge_gather_f32", x.data_ptr(), ldx, idx.data_ptr(), B, N, C, k, E.data_ptr())
        np.testing.assert_array_equal(bits(host(E)), bits(ER.edges32(o.x, o.idx)))
        lddx = {"dense": C, "aligned": C + 4, "unaligned": C + 3}[lay]
        buf = np.full((o.R, lddx), 3.0, np.float32)
        buf[:, :C] = o.dx0
        dx, dE = g.put(buf), g.put(o.dE)
        H.call("dgcnn_edge_gather_bwd_f32", dE.data_ptr(), idx.data_ptr(), B, N, C, k, dx.data_ptr(), lddx)
        got = host(dx)
        assert (got[:, C:] == 3.0).all(), "wrote outside its columns"
        ref, scale = ER.gather_bwd64(o.dE, o.idx)
        ref, scale = ref + o.dx0, scale + np.abs(o.dx0)
        if o.lattice:
            exact("gather_bwd %s %s" % (case, lay), got[:, :C], ref)
        else:
            within("edge_gather_bwd_f32", got[:, :C], ref, scale, k + ER.in_degrees(o.idx)[:, None] + 1)
        g.check()


# ---------------------------------------------------------------------------------------------------- transposed adjacency
def csr_plan(B, N):
    """misc.hip:dgcnn_edge_csr_build -- every cloud's targets are split over G blocks (doubling G while fewer than 256 blocks
    would run or a range would not fit, as long as a range keeps 64 targets, 64 at the most); the LDS kernel runs when a range
    T = ceil(N / G) holds at most 12288 targets.  -> (G, T, LDS kernel?)"""
    G = 1
    while G < 64 and (B * G < 256 or cdiv(N, G) > 12288) and cdiv(N, G * 2) >= 64:
        G *= 2
    T = cdiv(N, G)
    return G, T, T <= 12288


# (B, N, k, graph), the plan csr_plan must give for it
CSR_SHAPES = [
    ((2, 50, 3, "random"), (1, 50, True)),             # N < 64: ceil(N / 2) < 64 keeps G = 1, T = N
    ((1, 1001, 5, "random"), (8, 126, True)),          # ceil(1001 / 16) = 63 < 64 stops at G = 8; 8 * 126 = 1008 > N: the last block is short
    ((2, 300, 7, "hub"), (4, 75, True)),               # one bucket of N k = 2100 edges per cloud
    ((3, 100, 5, "degrees"), (1, 100, True)),          # planted in-degrees 0 .. 9
    ((300, 40, 3, "random"), (1, 40, True)),           # B >= 256: G stays 1
    ((1, 70000, 2, "random"), (64, 1094, True)),       # G = 64 (the cap); 64 * 1094 = 70016 > N
    ((1, 786432, 2, "random"), (64, 12288, True)),     # 786432 = 64 * 12288: the last N the LDS kernel takes
    ((1, 786433, 2, "random"), (64, 12289, False)),    # T = 12289: the first N on csr_count / csr_scan / csr_fill
    ((2, 786433, 1, "random"), (64, 12289, False)),    # the fallback with two clouds (cloud offset of counts, cursors and positions)
]
SORT_MAX_N = 70000


@pytest.mark.parametrize("shape,plan", CSR_SHAPES, ids=[ER.case_id(s) for s, _ in CSR_SHAPES])
def test_csr_build_both_kernels_and_sort(dg, shape, plan):
    """off == exclusive prefix of the in-degrees (its last word included), rev a permutation of the edges, every bucket holding
    exactly the edges that point at it; then (N <= 70000) dgcnn_edge_csr_sort of the built rev AND of a rev whose buckets were
    shuffled on the host == the stable-sorted reference, word for word: the deterministic mode's bit reproducibility rests on it."""
    from dgcnn import _hip as H
    B, N, k, kind = shape
    assert csr_plan(B, N) == plan, (shape, csr_plan(B, N))      # a change of the rule in misc.hip must not silently move the case
    rng = np.random.default_rng(N + k)
    idx = ER.graph(kind, rng, B, N, k)
    R, Me = B * N, B * N * k
    want_off, want_rev = ER.csr(idx)                             # bincount / cumsum / argsort only
    tgt = ER.nbr_rows(idx)
    deg = want_off[1:] - want_off[:-1]
    g = Guard()
    d_idx = g.put(idx)
    cws = g.zeros((2 * R,), torch.int32)
    off = g.new((R + 1,), torch.int32, fill=-7)
    rev = g.new((Me,), torch.int32, fill=-7)
    H.call("dgcnn_edge_csr_build", d_idx.data_ptr(), B, N, k, cws.data_ptr(), off.data_ptr(), rev.data_ptr())
    np.testing.assert_array_equal(host(off), want_off)
    assert int(host(off)[-1]) == Me
    r = host(rev).astype(np.int64)
    assert r.min() >= 0 and r.max() < Me
    assert np.array_equal(np.sort(r), np.arange(Me)), "rev is not a permutation of the edges"
    np.testing.assert_array_equal(tgt[r], np.repeat(np.arange(R), deg))      # bucket j holds only edges pointing at j
    if N <= SORT_MAX_N:
        shuffled = want_rev[np.lexsort((rng.random(Me), tgt[want_rev]))]        # every bucket in a random order
        assert not np.array_equal(shuffled, want_rev) and np.array_equal(tgt[shuffled], tgt[want_rev])
        for name, src in (("built", rev), ("shuffled", g.put(shuffled.astype(np.int32)))):
            out = g.new((Me,), torch.int32, fill=-7)
            H.call("dgcnn_edge_csr_sort", d_idx.data_ptr(), B, N, k, off.data_ptr(), src.data_ptr(), out.data_ptr())
            np.testing.assert_array_equal(host(out), want_rev, err_msg="csr_sort of the %s rev" % name)
    g.check()


# ------------------------------------------------------------------------------------------------- sums over incoming edges
@pytest.mark.parametrize("F", ER.GSUM_F)
@pytest.mark.parametrize("case", ER.GSUM_CASES, ids=ER.case_id)
def test_incoming_sums(dg, case, F):
    """S[j] = sum of the dY rows of the edges pointing at j, over a sorted rev: bit-equal to the float32 replay of the kernel's
    own order (groups of four, then the tail), exact on the lattice, within the bound on random rows; points nobody points at
    are written 0; lds = F, and lds = 2 F into the right half of a (R, 2F) buffer whose left half must not change.  The bf16
    kernel on bf16-representable rows: bit-equal to the fp32 kernel and to the replay."""
    from dgcnn import _hip as H
    B, N, k, kind = case
    for o in tiers(ER.case_seed(case) + F, B, N, 1, k, F, kind, need=("dY",)):
        R = o.R
        off, rev = ER.csr(o.idx)
        deg = off[1:] - off[:-1]
        assert (deg == 0).any() or kind == "permutation"
        dYb = BR.round_bf16(o.dY)
        assert not o.lattice or np.array_equal(dYb, o.dY)
        runs = (("f32", o.dY), ("f32", dYb), ("bf16", dYb))
        for wide in (False, True):
            g = Guard()
            d_off, d_rev = g.put(off.astype(np.int32)), g.put(rev.astype(np.int32))
            lds = 2 * F if wide else F
            outs = []
            for kern, vals in runs:
                S64, scale = ER.incoming_sum64(vals, o.idx)
                replay = ER.incoming_sum32_replay(vals, off, rev)
                d = g.put(vals if kern == "f32" else (bits(vals) >> 16).astype(np.uint16).view(np.int16))
                buf = g.new((R, lds))
                S = buf[:, lds - F:]
                S.fill_(NAN)
                H.call("dgcnn_edge_gather_sum_" + kern, d.data_ptr(), d_off.data_ptr(), d_rev.data_ptr(), R, F, S.data_ptr(), lds)
                got = host(buf)
                assert (got[:, :lds - F] == SENT).all(), "the left half of the (R, 2F) buffer changed"
                got = got[:, lds - F:]
                what = "gather_sum_%s %s F=%d lds=%d lattice=%d" % (kern, case, F, lds, o.lattice)
                assert (bits(got[deg == 0]) == 0).all(), "%s: a point without incoming edges is not +0" % what
                np.testing.assert_array_equal(bits(got), bits(replay), err_msg=what)
                if o.lattice:
                    exact(what, got, S64)
                else:
                    within("edge_gather_sum_" + kern, got, S64, scale, deg[:, None])
                outs.append(got)
            np.testing.assert_array_equal(bits(outs[1]), bits(outs[2]))         # bf16 kernel == fp32 kernel on the same values
            g.check()


def test_incoming_sum_refusals(dg):
    from dgcnn import _hip as H
    R, F = 8, 8
    z = torch.zeros(4096, device="cuda")
    zi = torch.zeros(64, dtype=torch.int32, device="cuda")
    for name, unsup in (("dgcnn_edge_gather_sum_f32", ValueError), ("dgcnn_edge_gather_sum_bf16", H.HipError)):
        H.call(name, z.data_ptr(), zi.data_ptr(), zi.data_ptr(), R, F, z.data_ptr() + 1024, F)        # (the accepted call)
        with pytest.raises(unsup):                                                                     # F % 4 != 0
            H.call(name, z.data_ptr(), zi.data_ptr(), zi.data_ptr(), R, 6, z.data_ptr() + 1024, 8)
        with pytest.raises(ValueError):                                                                # S not 16-byte aligned
            H.call(name, z.data_ptr(), zi.data_ptr(), zi.data_ptr(), R, F, z.data_ptr() + 1028, F)
        with pytest.raises(ValueError):                                                                # lds < F
            H.call(name, z.data_ptr(), zi.data_ptr(), zi.data_ptr(), R, F, z.data_ptr() + 1024, F - 4)
        with pytest.raises(ValueError):                                                                # lds % 4 != 0
            H.call(name, z.data_ptr(), zi.data_ptr(), zi.data_ptr(), R, F, z.data_ptr() + 1024, F + 2)
    torch.cuda.synchronize()
    assert not bool(z[:256].any())


# ------------------------------------------------------------------------------------------------------------ bf16 rounding
def test_round_bf16_bit_for_bit(dg):
    """dgcnn_round_bf16_f32 == bn_reference.round_bf16 on every tie boundary (...7fff, ...8000, ...8001 below an even and an odd
    kept bit), both signs, denormals, +-0, +-inf, the largest finite value (-> inf) and NaNs: a NaN stays a NaN of its sign,
    also one whose upper mantissa bits are all ones (the bare formula would carry 0x7fffffff into -0.0)."""
    from dgcnn import _hip as H
    hi = np.array([0x3f80, 0x3f81, 0x4049, 0x4048, 0x0000, 0x0001, 0x007f, 0x0080, 0x7f00, 0x7f7f, 0x7f7e], np.uint32)
    lo = np.array([0x0000, 0x0001, 0x7fff, 0x8000, 0x8001, 0xffff], np.uint32)
    u = ((hi[:, None] << 16) | lo[None, :]).reshape(-1)
    nans = np.array([0x7fc00000, 0x7fffffff, 0x7fff8000, 0x7fff7fff, 0x7f800001, 0x7fbfffff, 0x7f808000], np.uint32)
    special = np.array([0x00000000, 0x7f800000, 0x7f7fffff], np.uint32)
    rnd = np.random.default_rng(0).integers(0, 0x7f800000, 4096).astype(np.uint32)
    u = np.concatenate([u, nans, special, rnd])
    u = np.concatenate([u, u | np.uint32(0x80000000)])
    g = Guard()
    src = g.put(u.view(np.int32))
    dst = g.new((u.size,))
    H.call("dgcnn_round_bf16_f32", src.data_ptr(), dst.data_ptr(), u.size)
    got = bits(host(dst))
    g.check()
    want = bits(BR.round_bf16(u.view(np.float32)))
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%d differ, first: %08x -> %08x, reference %08x" % (bad.size, u[bad[0]], got[bad[0]], want[bad[0]])
    # and what the reference itself must say, independently of its formula
    f_in, f_out = u.view(np.float32), got.view(np.float32)
    assert ((got & 0xffff) == 0).all()
    np.testing.assert_array_equal(np.isnan(f_out), np.isnan(f_in))
    np.testing.assert_array_equal((got >> 31)[np.isnan(f_in)], (u >> 31)[np.isnan(f_in)])
    fin = np.isfinite(f_in) & np.isfinite(f_out)                     # (the top half-binade rounds to inf: pinned below)
    d = np.abs(f_out[fin].astype(np.float64) - f_in[fin].astype(np.float64))
    assert (d <= np.abs(f_in[fin].astype(np.float64)) * 2.0 ** -8 + 2.0 ** -134).all()     # within half a bf16 spacing
    for a, b in ((0x7f7fffff, 0x7f800000), (0xff7fffff, 0xff800000), (0x00000000, 0x00000000), (0x80000000, 0x80000000),
                 (0x7f800000, 0x7f800000), (0xff800000, 0xff800000), (0x3f808000, 0x3f800000), (0x3f818000, 0x3f820000)):
        assert (got[u == a] == b).all() and (u == a).any(), "%08x" % a


# ---------------------------------------------------------------------------------------------------------------- refusals
def _entry_points(z, zi):
    """name -> (argument list of an accepted tiny call, positions of its required pointers); B = 1, N = 2, C = 4, k = 1, F = 4,
    all indices 0 and one zero-filled buffer behind every pointer."""
    B, N, C, k, F = 1, 2, 4, 1, 4
    f, f2, i, i2 = z.data_ptr(), z.data_ptr() + 4096, zi.data_ptr(), zi.data_ptr() + 256
    return {
        "dgcnn_edge_mlp_f32": ([f, C, i, f, B, N, C, k, F, f2, 0], (0, 2, 3, 9)),
        "dgcnn_edge_nbr_gemm_f32": ([f, C, i, f, f, F, B, N, C, k, F, f2, 0], (0, 2, 3, 4, 11)),
        "dgcnn_edge_mlp_wgrad_f32": ([f, C, i, f, B, N, C, k, F, f2, 0.0, f2 + 4096, 4096], (0, 2, 3, 9)),
        "dgcnn_edge_nbr_wgrad_f32": ([f, C, i, f, B, N, C, k, F, f2, 0.0, f2 + 4096, 4096], (0, 2, 3, 9)),
        "dgcnn_edge_mlp_dgrad_scatter_f32": ([f, f, i, B, N, C, k, F, f2, C], (0, 1, 2, 8)),
        "dgcnn_edge_gather_f32": ([f, C, i, B, N, C, k, f2], (0, 2, 7)),
        "dgcnn_edge_gather_bwd_f32": ([f, i, B, N, C, k, f2, C], (0, 1, 6)),
        "dgcnn_edge_csr_build": ([i, B, N, k, i2, i2 + 256, i2 + 512], (0, 4, 5, 6)),
        "dgcnn_edge_csr_sort": ([i, B, N, k, i, i, i2], (0, 4, 5, 6)),
        "dgcnn_edge_gather_sum_f32": ([f, i, i, B * N, F, f2, F], (0, 1, 2, 5)),
        "dgcnn_edge_gather_sum_bf16": ([f, i, i, B * N, F, f2, F], (0, 1, 2, 5)),
        "dgcnn_round_bf16_f32": ([f, f2, 16], (0, 1)),
    }


ENTRY_POINTS = ["dgcnn_edge_mlp_f32", "dgcnn_edge_nbr_gemm_f32", "dgcnn_edge_mlp_wgrad_f32", "dgcnn_edge_nbr_wgrad_f32",
                "dgcnn_edge_mlp_dgrad_scatter_f32", "dgcnn_edge_gather_f32", "dgcnn_edge_gather_bwd_f32", "dgcnn_edge_csr_build",
                "dgcnn_edge_csr_sort", "dgcnn_edge_gather_sum_f32", "dgcnn_edge_gather_sum_bf16", "dgcnn_round_bf16_f32"]


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_null_pointers_are_refused(dg, name):
    """Every required pointer of every entry point above, nulled in turn: DGCNN_EINVAL before anything is launched."""
    from dgcnn import _hip as H
    z = torch.zeros(8192, device="cuda")
    zi = torch.zeros(2048, dtype=torch.int32, device="cuda")
    table = _entry_points(z, zi)
    assert sorted(table) == sorted(ENTRY_POINTS)
    args, ptrs = table[name]
    H.call(name, *args)                                             # the argument list itself is accepted
    for pos in ptrs:
        bad = list(args)
        bad[pos] = 0
        with pytest.raises(ValueError):
            H.call(name, *bad)
    if name == "dgcnn_edge_csr_sort":                               # in place is refused too
        bad = list(args)
        bad[6] = bad[5]
        with pytest.raises(ValueError):
            H.call(name, *bad)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["dgcnn_edge_mlp_f32", "dgcnn_edge_nbr_gemm_f32"])
def test_bad_shapes_are_refused(dg, name):
    from dgcnn import _hip as H
    z = torch.zeros(8192, device="cuda")
    zi = torch.zeros(2048, dtype=torch.int32, device="cuda")
    args, _ = _entry_points(z, zi)[name]
    first = 4 if name == "dgcnn_edge_mlp_f32" else 6                # position of B; N, C, k, F follow
    for pos in range(first, first + 5):
        for v in (0, -1):
            bad = list(args)
            bad[pos] = v
            with pytest.raises(ValueError, match="bad shape"):
                H.call(name, *bad)
    torch.cuda.synchronize()
    assert not bool(z[1024:].any())

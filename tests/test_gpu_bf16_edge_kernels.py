"""The four fused kernels of the bf16 edge-MLP mode (csrc/edge_mlp_bf16.hip), called through their C entry points and checked
against tests/edge_bf16_reference.py (run with -m gpu on an MI355X):

  dgcnn_edge_mlp_bf16               y = bf16(E) bf16(W0) written out
  dgcnn_edge_mlp_bf16_stats         column sums of y and y^2, y never written
  dgcnn_edge_mlp_bf16_bn_kreduce    relu(BatchNorm(y)) reduced over the k edges of every point
  dgcnn_edge_mlp_bf16_bwd           dY (bf16), its per-point sums, d(beta) and dW0 = E^T dY in one pass over the edges

What tests/test_gpu_bf16_edge_mlp.py leaves open, and the cases (edge_bf16_reference.FWD_CASES / BWD_CASES) are chosen for:
every one of the six (CK, FB) template instances; C = 1 and 2 (the `row = -1` maps of the weight fragments and of the dW0
write-out); k = 1, k < 5, 64 < k < 128 (one point and up to 63 pad rows per tile), P k = 128 against P k < 128; more tiles than
workgroups (1024 forward, 512 backward, the slot count in the deterministic statistics pass), so that the persistent tile loops,
the cross-tile sums and the backward's two LDS buffers run more than once; and the calling convention of dgcnn/_engine.py (`prod`:
x a column slice of a wider buffer, max / mean and their gradients the halves of one (R, 2F) buffer, lddysum > F, dbeta_beta = 1
onto a prior d(beta), a non-zero dW0 to accumulate into).

Tiers (edge_bf16_reference.py; tests/test_edge_bf16_reference.py asserts their preconditions for every case on the host):
* lattice and wide lattice: y, its column sums and dW0 must EQUAL float64 -- one tile in a thousand dropped, doubled or read from a
  stale buffer is off by whole terms.  The wide lattice needs the bf16 rounding in about one entry of E in eight, exact ties among
  them, and gives another exact y when x_i and x_j are rounded BEFORE the subtraction.
* random: |err| <= (n_terms + 8) 2^-24 sum |term| (bn_reference.sum_bound).  The worst ratio per kernel is printed at the end of
  the module ($DGCNN_EDGE_BF16_ERROR_TABLE writes it; profiles/edge_bf16_kernel_errors.txt holds a measured copy).
* in every tier the k-reduce, dY, dYsum and d(beta) are compared BIT FOR BIT with the float32 replays of bn_reference.py.

Every buffer sits between sentinel guards (gpu_helpers.Guard), outputs are NaN-filled, the clouds differ from each other."""
import numpy as np
import pytest
import torch

import bn_reference as BR
import edge_bf16_reference as EB
from gpu_helpers import Guard, RATIOS, SENT, host, note_ratio, ratio_table
from test_gpu_edge_kernels import bits, exact, put_cols

pytestmark = pytest.mark.gpu

NAN = float("nan")
NAN_BF16 = 0x7fc0         # a bf16 NaN as an int16 pattern
MINE = set()              # the kernels this module recorded in RATIOS
HEADER = ["# worst |hip - float64| / (2^-24 * sum |term|) per output element over the random-input cases of",
          "# tests/test_gpu_bf16_edge_kernels.py; bound = n_terms + 8 (any-order fp32 summation plus the roundings inside a term).",
          "# edge_mlp_bf16: y = bf16(E) bf16(W0), 2C terms; edge_mlp_bf16_stats: the 16 values a lane adds in fp32 per tile before it",
          "# goes on in double, against float64 sums of the kernel's own y; edge_mlp_bf16_bwd (dW0): bf16(E)^T dY + prior over all",
          "# B N k edges, against float64 on the kernel's own bf16 dY."]

SIX = {(ck, fb) for ck in (1, 8) for fb in (1, 2, 4)}
# every template instance of all four kernels runs in the exact tiers (they run on every case of both lists)
assert {EB.instance(c) for c in EB.FWD_CASES} == SIX and {EB.instance(c) for c in EB.BWD_CASES} == SIX
assert "lattice" in EB.TIERS and "wide" in EB.TIERS and "lattice" in EB.BWD_TIERS


@pytest.fixture()
def dg():
    import dgcnn
    dgcnn.reset()
    return dgcnn


@pytest.fixture(scope="module", autouse=True)
def _error_table():
    yield
    ratio_table(header=HEADER, env="DGCNN_EDGE_BF16_ERROR_TABLE", names=sorted(MINE & set(RATIOS)))


def within(kernel, got, ref, scale, n_terms, record=True):
    """|got - ref| <= (n_terms + 8) 2^-24 scale, element by element."""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), "%s: non-finite outputs" % kernel
    if record:
        MINE.add(kernel)
    note_ratio(kernel, got - ref, scale, n_terms, n_terms + 8, record=record)


def same_bits(what, got, ref):
    got, ref = bits(got), bits(ref)
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, "%s: %d of %d words differ from the float32 replay, first %s: got %08x, replay %08x" % (
        what, len(bad), got.size, bad[0], got[tuple(bad[0])], ref[tuple(bad[0])])


def put_x(g, o, lay):
    """x dense, or (`prod`) a column slice of a wider buffer of other values: float4-loadable at C = 64, one float off at C <= 4."""
    C = o.case[2]
    return put_cols(g, o.x, "dense" if lay == "dense" else ("aligned" if C == 64 else "unaligned"))


def halves(g, R, F, lay, a=None, b=None):
    """Two (R, F) matrices: dense, or (`prod`) the halves of one (R, 2F) buffer.  NaN-filled, or holding a and b.
    -> (first, second, leading dimension)"""
    if lay == "dense":
        m1, m2, ld = g.new((R, F)), g.new((R, F)), F
    else:
        mm = g.new((R, 2 * F))
        m1, m2, ld = mm[:, :F], mm[:, F:], 2 * F
    for m, v in ((m1, a), (m2, b)):
        if v is None:
            m.fill_(NAN)
        else:
            m.copy_(torch.from_numpy(np.ascontiguousarray(v)))
    return m1, m2, ld


def source(g, o, lay):
    B, N, C, k, F, kind = o.case
    x, ldx = put_x(g, o, lay)
    idx, W0 = g.put(o.idx), g.put(o.W0)
    keep = (x, idx, W0)
    return (x.data_ptr(), ldx, idx.data_ptr(), W0.data_ptr(), B, N, C, k, F), keep


def write_y(H, g, o, src, what):
    """dgcnn_edge_mlp_bf16 into a NaN-filled buffer; lattice tiers: EQUALS float64, random: within the any-order fp32 bound."""
    C, F = o.case[2], o.case[4]
    Y = g.new((o.Me, F))
    Y.fill_(NAN)
    H.call("dgcnn_edge_mlp_bf16", *src, Y.data_ptr())
    Yh = host(Y)
    if o.lattice:
        exact(what + " y", Yh, o.Y)
    else:
        within("edge_mlp_bf16", Yh, o.Y, o.Yscale, 2 * C)
    return Yh


def check_stats(what, S, o, Yh):
    """S (2, F): the slots added up in float64.  Lattice tiers: the column sum EQUALS float64, the sum of squares too where the 16
    squares a lane adds in fp32 are exact (edge_bf16_reference.sq_exact: every lattice case; no wide one); otherwise, and on random
    operands, against float64 sums of the kernel's own y within the bound of a 16-term fp32 sum."""
    if o.lattice:
        ref, scale = EB.stats64(o.Y)
        exact(what + " column sums", S[0], ref[0])
        if EB.sq_exact(o.Y):
            exact(what + " column sums of squares", S[1], ref[1])
        else:
            assert o.tier == "wide"
            within("edge_mlp_bf16_stats", S[1], ref[1], scale[1], 16, record=False)
    else:
        ref, scale = EB.stats64(Yh)
        within("edge_mlp_bf16_stats", S, ref, scale, 16)


def launched_grid(H, g, o, src, what, Yh):
    """The workgroups launch_pass starts for this case, read off the library instead of a constant restated here: with more
    slots than tiles (and than workgroups) cap_writers leaves the grid alone and workgroup b adds its sums into slot b, so the
    number of written slots IS the grid.  The three forward passes share that one expression (min(tiles, cap)); the dense and
    the point tiling of the multi-tile cases both exceed it.  The totals over those slots are checked like any others."""
    F = o.case[4]
    assert EB.geometry(o.case)["dense"] < EB.PROBE_SLOTS
    try:
        H.set_stat_slots(EB.PROBE_SLOTS)
        st = g.zeros((EB.PROBE_SLOTS, 2, F), torch.float64)
        H.call("dgcnn_edge_mlp_bf16_stats", *src, st.data_ptr())
        sh = host(st)
    finally:
        H.set_stat_slots(EB.DEFAULT_SLOTS)
    written = (sh[:, 1] != 0).any(1)
    grid = int(written.sum())
    assert written[:grid].all(), what + ": the written slots are not the first ones"
    check_stats(what + " (one slot per workgroup)", sh.sum(0), o, Yh)
    return grid


# ------------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("lay", ["dense", "prod"])
@pytest.mark.parametrize("tier", EB.TIERS)
@pytest.mark.parametrize("case", EB.FWD_CASES, ids=EB.case_id)
def test_forward_passes(dg, case, tier, lay):
    """Write, statistics (default slots) and k-reduce of one case.  The k-reduce with pack_cnt 0 and 1 and once without cnt: max,
    mean and counts bit for bit bn_reference.Fwd -- of the float64 y under lattice parameters (the written y EQUALS it), of the
    kernel's own written y on random operands.  Column 0 is dead (z = 0 on every edge): max 0, ties = k, no positives."""
    from dgcnn import _hip as H
    B, N, C, k, F, kind = case
    geo = EB.geometry(case)
    R, Me = geo["R"], geo["Me"]
    assert H.stat_slots() == EB.DEFAULT_SLOTS
    o = EB.forward_case(case, tier)
    what = "%s %s %s" % (case, tier, lay)
    g = Guard()
    src, keep = source(g, o, lay)
    Yh = write_y(H, g, o, src, what)

    st = g.zeros((H.stat_slots(), 2, F), torch.float64)
    H.call("dgcnn_edge_mlp_bf16_stats", *src, st.data_ptr())
    check_stats(what, host(st).sum(0), o, Yh)
    if case in EB.FWD_MULTI_TILE:           # the tile loops loop: a change of the caps must not silently undo that
        grid = launched_grid(H, g, o, src, what, Yh)
        assert grid == EB.FWD_GRID, "launch_pass runs %d workgroups: restate the cap in edge_bf16_reference.FWD_GRID" % grid
        assert geo["dense"] > grid and geo["points"] > grid, (geo, grid)

    fw = EB.kreduce(o.Y if o.lattice else Yh, R, k, o.mean, o.rstd, o.beta)
    par = [g.put(a) for a in (o.mean, o.rstd, o.beta)]
    for pack, with_cnt in ((0, True), (1, True), (0, False)):
        mx, mn, ld = halves(g, R, F, lay)
        cnt = g.new((R, F)) if with_cnt else None
        if with_cnt:
            cnt.fill_(NAN)
        H.call("dgcnn_edge_mlp_bf16_bn_kreduce", *src, par[0].data_ptr(), par[1].data_ptr(), par[2].data_ptr(), mx.data_ptr(), ld,
               mn.data_ptr(), ld, cnt.data_ptr() if with_cnt else 0, pack)
        w = "%s k-reduce pack=%d cnt=%d" % (what, pack, with_cnt)
        same_bits(w + " max", host(mx), fw.mx)
        same_bits(w + " mean", host(mn), fw.mean32)
        if with_cnt:
            ch = host(cnt)
            same_bits(w + " counts", ch, fw.packed if pack else fw.ties)
            assert (ch[:, 0] == k).all()                                        # dead column: ties = k (+ 256 * 0 positives)
        assert (host(mx)[:, 0] == 0).all() and (host(mn)[:, 0] == 0).all()
    g.check()


@pytest.mark.parametrize("tier", EB.TIERS)
@pytest.mark.parametrize("case", EB.SLOT_CASES, ids=EB.case_id)
def test_stats_with_more_slots(dg, case, tier):
    """The deterministic configuration: with more than the default 32 slots the grid is capped at the slot count and every slot
    has one writer.  Same totals as with the default slots, slots >= min(tiles, slots) stay zero, every other slot is written,
    two runs are bit-identical.  On the 1050-tile case every workgroup walks 31 to 32 tiles (33 slots) or one to two (768)."""
    from dgcnn import _hip as H
    B, N, C, k, F, kind = case
    geo = EB.geometry(case)
    o = EB.forward_case(case, tier)
    g = Guard()
    src, keep = source(g, o, "dense")
    Yh = write_y(H, g, o, src, "%s %s" % (case, tier))
    try:
        for slots in EB.SLOT_COUNTS:
            H.set_stat_slots(slots)
            grid = EB.stats_grid(geo["dense"], slots)
            assert grid == min(geo["dense"], slots)
            if case in EB.FWD_MULTI_TILE:
                assert geo["dense"] > grid
            runs = []
            for rep in range(2):
                st = g.zeros((slots, 2, F), torch.float64)
                H.call("dgcnn_edge_mlp_bf16_stats", *src, st.data_ptr())
                runs.append(host(st).copy())
            what = "%s %s %d slots" % (case, tier, slots)
            np.testing.assert_array_equal(runs[0].view(np.uint64), runs[1].view(np.uint64), err_msg=what + ": two runs differ")
            assert not runs[0][grid:].any(), what + ": a slot without a writer is not zero"
            assert (runs[0][:grid, 1] != 0).any(1).all(), what + ": a slot with a writer holds no sum of squares"
            check_stats(what, runs[0].sum(0), o, Yh)
    finally:
        H.set_stat_slots(EB.DEFAULT_SLOTS)
    g.check()


# ----------------------------------------------------------------------------------------------------------------- backward
def bf16_rows(t):
    """int16 words of a bf16 matrix -> the float32 values."""
    return (host(t).view(np.uint16).astype(np.uint32) << 16).view(np.float32)


@pytest.mark.parametrize("lay", ["dense", "prod"])
@pytest.mark.parametrize("tier", EB.BWD_TIERS)
@pytest.mark.parametrize("case", EB.BWD_CASES, ids=EB.case_id)
def test_backward_pass(dg, case, tier, lay):
    """dgcnn_edge_mlp_bf16_bwd after the forward with packed counts.
    dY (bf16), dYsum and d(beta) bit for bit the float32 replay (dz32 -> apply32(bf16=True), dbeta32) on bn_reference.Fwd of the
    kernel's written y, with the totals the call itself left in slot 0 of `red`.
    dW0, random tier: against float64 bf16(E)^T dY_kernel + prior within the bound of an (Me + 1)-term fp32 sum.  That bound is
    about 8e-3 of the scale at Me = 134 000 and one lost tile among 1050 is 1e-3 of it, so the tile loop is checked in the
    lattice tier: `red` written as zeros on the host (c1 = c2 = 0), dmax = 0, dmean = k g -- dY = rstd g [z > 0] is a lattice
    value and dW0 must EQUAL float64.
    dense: d(beta) and dW0 from scratch (dbeta_beta = 0 into NaNs, dW0 = 0), then once more with dYb = dysum = NULL: dW0, d(beta)
    and `red` come out the same, to the bit.  prod: dbeta_beta = 1 onto a prior, dW0 accumulated onto a prior, lddysum = F + 4."""
    from dgcnn import _hip as H
    lib = H.load()
    B, N, C, k, F, kind = case
    geo = EB.geometry(case)
    R, Me = geo["R"], geo["Me"]
    grid = min(geo["points"], EB.BWD_GRID)
    if case in EB.BWD_MULTI_TILE:
        assert geo["points"] > EB.BWD_GRID and geo["points"] > grid
    assert lib.dgcnn_edge_mlp_bf16_bwd_supported(C, k, F) == 1
    need = int(lib.dgcnn_edge_mlp_bf16_bwd_workspace_bytes(B, N, C, k, F))
    assert need == grid * 2 * C * F * 4
    o = EB.backward_case(case, tier)
    prod = lay == "prod"
    what = "%s %s %s" % (case, tier, lay)
    g = Guard()
    src, keep = source(g, o, lay)
    Yh = write_y(H, g, o, src, what)
    par = [g.put(a).data_ptr() for a in (o.mean, o.rstd, o.beta)]
    mx, mn, ldm = halves(g, R, F, lay)
    cnt = g.new((R, F))
    cnt.fill_(NAN)
    H.call("dgcnn_edge_mlp_bf16_bn_kreduce", *src, *par, mx.data_ptr(), ldm, mn.data_ptr(), ldm, cnt.data_ptr(), 1)
    fw = EB.kreduce(Yh, R, k, o.mean, o.rstd, o.beta)
    same_bits(what + " max", host(mx), fw.mx)
    same_bits(what + " packed counts", host(cnt), fw.packed)
    dmx, dmn, ldd = halves(g, R, F, lay, o.dmax, o.dmean)
    if o.lattice:
        red0 = np.zeros((H.stat_slots(), 2, F))
    else:
        red = g.zeros((H.stat_slots(), 2, F), torch.float64)
        H.call("dgcnn_edge_bn_bwd_reduce_points_f32", mx.data_ptr(), ldm, mn.data_ptr(), ldm, cnt.data_ptr(), dmx.data_ptr(), ldd,
               dmn.data_ptr(), ldd, par[2], R, k, F, red.data_ptr())
        red0 = host(red).copy()
    ws = g.new((need,), torch.uint8, fill=7)
    dW_prior = o.dW0 if prod else np.zeros((2 * C, F), np.float32)
    dbeta_beta = 1.0 if prod else 0.0
    lds = F + 4 if prod else F

    def run(with_dy):
        red = g.put(red0)
        dW = g.put(dW_prior)
        db = g.put(o.dbeta0)
        if not prod:
            db.fill_(NAN)                                                       # dbeta_beta = 0: never read
        dYb = dsb = None
        if with_dy:
            dYb = g.new((Me, F), torch.int16, fill=NAN_BF16)
            dsb = g.new((R, lds))
            dsb[:, :F] = NAN
        H.call("dgcnn_edge_mlp_bf16_bwd", *src, *par, mx.data_ptr(), ldm, cnt.data_ptr(), dmx.data_ptr(), ldd, dmn.data_ptr(), ldd,
               red.data_ptr(), dYb.data_ptr() if with_dy else 0, dsb.data_ptr() if with_dy else 0, lds, dW.data_ptr(), db.data_ptr(),
               dbeta_beta, ws.data_ptr(), need)
        return host(red)[0].copy(), host(dW), host(db), dYb, dsb

    tot, dW, db, dYb, dsb = run(True)
    if o.lattice:
        assert not tot.any()
    dY_ref, dsum_ref = EB.backward(fw, o.dmax, o.dmean, tot)
    dY_k = bf16_rows(dYb)
    same_bits(what + " dY", dY_k, dY_ref.reshape(Me, F))
    dsh = host(dsb)
    assert (dsh[:, F:] == SENT).all(), what + ": dysum wrote outside its columns"
    same_bits(what + " dYsum", dsh[:, :F], dsum_ref)
    same_bits(what + " d(beta)", db, BR.dbeta32(tot[0], o.dbeta0, dbeta_beta))
    if o.lattice:
        np.testing.assert_array_equal(dY_ref, np.where(fw.pos, (o.rstd * o.g)[:, None, :], np.float32(0)))
        ref, scale = EB.wgrad64(o.Eb, dY_ref)
        exact(what + " dW0", dW, ref + dW_prior)
    else:
        ref, scale = EB.wgrad64(o.Eb, dY_k)
        within("edge_mlp_bf16_bwd (dW0)", dW, ref + dW_prior, scale + np.abs(dW_prior), Me + 1)
    if not prod:
        tot2, dW2, db2, _, _ = run(False)                                        # no input gradient wanted
        np.testing.assert_array_equal(tot2.view(np.uint64), tot.view(np.uint64))
        same_bits(what + " dW0 without dY", dW2, dW)
        same_bits(what + " d(beta) without dY", db2, db)
    g.check()


# ----------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(dg):
    """Shapes and arguments the entry points do not take: the right code before anything is launched, NaN-filled outputs and the
    guards untouched.  The backward takes 8 <= k <= 128 (include/dgcnn_hip.h)."""
    from dgcnn import _hip as H
    lib = H.load()
    B, N, C, k, F = 1, 16, 64, 8, 32
    R = B * N
    rng = np.random.default_rng(0)
    g = Guard()
    xw = g.put(rng.normal(size=(R, 72)).astype(np.float32))
    idx = g.put(rng.integers(0, N, (B, N, 129)).astype(np.int32))
    W0 = g.put(rng.normal(size=(128, 128)).astype(np.float32))
    par = [g.put(rng.random(128).astype(np.float32) + 0.5) for _ in range(3)]
    pp = [p.data_ptr() for p in par]
    # an accepted forward: the inputs of the backward calls below
    src = (xw.data_ptr(), 72, idx.data_ptr(), W0.data_ptr(), B, N, C, k, F)
    mxv, mnv, cntv = g.new((R, 128)), g.new((R, 128)), g.new((R, 128))
    H.call("dgcnn_edge_mlp_bf16_bn_kreduce", *src, *pp, mxv.data_ptr(), F, mnv.data_ptr(), F, cntv.data_ptr(), 1)
    dm = g.put(rng.normal(size=(R, 128)).astype(np.float32))
    red0 = rng.normal(size=(H.stat_slots(), 2, 128))
    red = g.put(red0)
    need = int(lib.dgcnn_edge_mlp_bf16_bwd_workspace_bytes(B, N, C, k, 128))
    ws = g.new((need,), torch.uint8, fill=7)
    # the outputs no refused call may touch
    Y = g.new((R * 129, 128))
    mx, mn, cnt, dsum = (g.new((R, 128)) for _ in range(4))
    for t in (Y, mx, mn, cnt, dsum):
        t.fill_(NAN)
    st = g.zeros((H.stat_slots(), 2, 128), torch.float64)
    dYb = g.new((R * 129, 128), torch.int16, fill=NAN_BF16)
    dW, db = g.new((128, 128)), g.new((128,))
    dW.fill_(5.0)
    db.fill_(5.0)

    def calls(x=xw.data_ptr(), ldx=72, C=C, k=k, F=F, mean=pp[0], dyb=None, ws_bytes=None):
        s = (x, ldx, idx.data_ptr(), W0.data_ptr(), B, N, C, k, F)
        bwd_need = int(lib.dgcnn_edge_mlp_bf16_bwd_workspace_bytes(B, N, C, min(k, 128), F)) if ws_bytes is None else ws_bytes
        return {
            "dgcnn_edge_mlp_bf16": s + (Y.data_ptr(),),
            "dgcnn_edge_mlp_bf16_stats": s + (st.data_ptr(),),
            "dgcnn_edge_mlp_bf16_bn_kreduce": s + (mean, pp[1], pp[2], mx.data_ptr(), F, mn.data_ptr(), F, cnt.data_ptr(), 1),
            "dgcnn_edge_mlp_bf16_bwd": s + (mean, pp[1], pp[2], mxv.data_ptr(), F, cntv.data_ptr(), dm.data_ptr(), F, dm.data_ptr(), F,
                                            red.data_ptr(), dYb.data_ptr() if dyb is None else dyb, dsum.data_ptr(), F, dW.data_ptr(),
                                            db.data_ptr(), 1.0, ws.data_ptr(), bwd_need),
        }

    def refused(exc, match, names=None, **kw):
        table = calls(**kw)
        for name in names or sorted(table):
            with pytest.raises(exc, match=match):
                H.call(name, *table[name])

    unsup, nospc = r"\(-4\)", r"\(-3\)"
    for c_, k_, f_ in ((5, 8, 32), (32, 8, 32), (64, 8, 48), (64, 129, 32)):        # DGCNN_EUNSUP in all four entry points
        assert lib.dgcnn_edge_mlp_bf16_supported(c_, k_, f_) == 0 and lib.dgcnn_edge_mlp_bf16_bwd_supported(c_, k_, f_) == 0
        refused(H.HipError, unsup, C=c_, k=k_, F=f_)
    assert lib.dgcnn_edge_mlp_bf16_supported(64, 128, 32) == 1 and lib.dgcnn_edge_mlp_bf16_supported(1, 1, 128) == 1
    refused(ValueError, "float4-loadable", ldx=66)                                     # C = 64: ldx % 4 != 0
    refused(ValueError, "float4-loadable", x=xw.data_ptr() + 4)                        # ... a base 4 bytes off
    # the backward alone: 8 <= k <= 128, and C = 64 with F = 128 from k = 9 (LDS)
    for c_, k_, f_, ok in ((64, 7, 32, 0), (64, 8, 32, 1), (64, 128, 32, 1), (64, 129, 32, 0), (64, 8, 128, 0), (64, 9, 128, 1),
                           (64, 10, 128, 1), (4, 8, 128, 1), (4, 7, 128, 0)):
        assert lib.dgcnn_edge_mlp_bf16_bwd_supported(c_, k_, f_) == ok, (c_, k_, f_)
    assert lib.dgcnn_edge_mlp_bf16_supported(64, 7, 32) == 1 and lib.dgcnn_edge_mlp_bf16_supported(64, 8, 128) == 1
    refused(H.HipError, unsup, names=["dgcnn_edge_mlp_bf16_bwd"], k=7)
    refused(H.HipError, unsup, names=["dgcnn_edge_mlp_bf16_bwd"], F=128)
    own = int(lib.dgcnn_edge_mlp_bf16_bwd_workspace_bytes(B, N, C, k, F))
    assert own == 2 * C * F * 4                                                        # P = 16: the 16 points are one tile
    refused(H.HipError, nospc, names=["dgcnn_edge_mlp_bf16_bwd"], ws_bytes=own - 1)
    refused(ValueError, "16-byte aligned", names=["dgcnn_edge_mlp_bf16_bwd"], dyb=dYb.data_ptr() + 2)
    refused(ValueError, "bad args", names=["dgcnn_edge_mlp_bf16_bn_kreduce", "dgcnn_edge_mlp_bf16_bwd"], mean=0)
    torch.cuda.synchronize()
    for t in (Y, mx, mn, cnt, dsum):
        assert bool(torch.isnan(t).all()), "a refused call wrote an output"
    assert (host(dYb).view(np.uint16) == NAN_BF16).all() and not host(st).any()
    assert (host(dW) == 5.0).all() and (host(db) == 5.0).all()
    np.testing.assert_array_equal(host(red), red0)
    # and the untampered argument lists are accepted
    table = calls()
    for name in sorted(table):
        H.call(name, *table[name])
    torch.cuda.synchronize()
    assert np.isfinite(host(dW)).all() and np.isfinite(host(Y)[:R * k * F // 128]).all()
    g.check()

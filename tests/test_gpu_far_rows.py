"""Every entry that gathers neighbour rows as V + idx * ldv, on rows that start 2^31 elements or more past their base -- inside the
N < 2^24, ldv < 2^24, N * ldv < 2^32 the host checks admit, and the range where a 24-bit product held as `int` is sign-extended into
the address (csrc/common.h: row_offset24).  Inputs and float64 references: tests/far_rows.py; that the inputs reach the range, and
that the sign-extending arithmetic could not pass on them, is asserted on the CPU in tests/test_far_rows_reference.py.

Shape W (N = 160 rows, ld = 2^24 - 4, rows 129.. far, lattice values): every result must EQUAL the float64 reference -- sums
exactly, fp32 outputs bit for bit.  The V operand is an N x F view into a torch.empty buffer of (N - 1) ld + F floats (10.7 GB; 17.6 GB
for the two-cloud case) of which only the view is ever written; one such buffer is live at a time and it is returned to the
driver at the end of each test.  Shape R (N = 2^24 - 256 rows, ld = 132): the two statistics passes within the any-order fp32
summation bound.  Outputs and small inputs sit between sentinel guards.  Refusals just outside the contract use small buffers."""
import contextlib

import numpy as np
import pytest
import torch

import bn_reference as BR
import far_rows as FR
from gpu_helpers import Guard, SENT, host

pytestmark = pytest.mark.gpu

EUNSUP = -4


@pytest.fixture()
def H():
    import dgcnn
    dgcnn.reset()
    from dgcnn import _hip
    return _hip


@contextlib.contextmanager
def far_view(values, ld):
    """-> the device address of a (rows, F) view with leading dimension ld whose rows hold `values` (host, fp32).  The buffer behind
    it is never filled and is handed back to the driver on exit."""
    n, F = values.shape
    big = torch.empty((n - 1) * ld + F, dtype=torch.float32, device="cuda")
    try:
        assert big.data_ptr() % 16 == 0
        big.as_strided((n, F), (ld, 1)).copy_(torch.from_numpy(np.array(values, np.float32)).cuda())
        yield big.data_ptr()
    finally:
        torch.cuda.synchronize()
        del big
        torch.cuda.empty_cache()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(got, want, what):
    got, want = bits(got), bits(np.asarray(want, np.float32))
    assert got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert not len(bad), "%s: %d of %d words differ from the reference, first at %s" % (what, len(bad), got.size, tuple(bad[0]))


def rc(H, name, *args):
    """The entry's return code (H.call raises instead)."""
    return int(getattr(H.load(), name)(*args, torch.cuda.current_stream().cuda_stream))


def p(t):
    return 0 if t is None else t.data_ptr()


def put(g, a):
    """g.put of a copy: the cached cases and references are read-only arrays, which torch will not wrap."""
    return g.put(np.array(a))


class DenseDev(object):
    """The small operands of a dense case in guarded buffers."""

    def __init__(self, c, g):
        self.c, self.g = c, g
        self.U, self.idx = put(g, c.U), put(g, c.idx)
        self.par = tuple(put(g, a).data_ptr() for a in (c.mu, c.rs, c.be))
        self.dmax, self.dmean = put(g, c.dmax), put(g, c.dmean)

    def head(self, V):
        c = self.c
        return (V, c.ld, self.U.data_ptr(), c.F, self.idx.data_ptr(), c.B, c.N, c.k, c.F)


class PackedDev(object):
    def __init__(self, c, g):
        self.c, self.g = c, g
        self.U, self.idx, self.off, self.rg = put(g, c.U), put(g, c.idx), put(g, c.off), put(g, c.row_group)
        self.par = tuple(put(g, a).data_ptr() for a in (c.mu, c.rs, c.be))
        self.dmax, self.dmean = put(g, c.dmax), put(g, c.dmean)

    def head(self, V):
        c = self.c
        return (V, c.ld, self.U.data_ptr(), c.F, self.idx.data_ptr(), c.R, c.k, c.F)

    def stats(self, H, V):
        c, g = self.c, self.g
        nb = int(H.load().dgcnn_seg_stats_workspace_bytes(c.R, c.nseg, c.F))
        ws = g.new((nb // 8,), torch.float64)
        st = g.new((c.nseg, 2, c.F), torch.float64)
        H.call("dgcnn_seg_edge_stats_f32", *self.head(V), self.off.data_ptr(), c.nseg, st.data_ptr(), ws.data_ptr(), nb)
        return host(st)


def dense_gather_add(H, d, V, want_y=True):
    c, g = d.c, d.g
    Y = g.new((c.R * c.k, c.F)) if want_y else None
    st = g.zeros((H.stat_slots(), 2, c.F), torch.float64)
    H.call("dgcnn_edge_gather_add_f32", *d.head(V), p(Y), st.data_ptr())
    return (host(Y).reshape(c.R, c.k, c.F) if want_y else None), host(st).sum(0)


def dense_apply(H, d, V, ref, relu):
    """-> dY (R, k, F), dYsum with the exact float64 sums in slot 0 of red, max / packed count given."""
    c, g = d.c, d.g
    red = g.zeros((H.stat_slots(), 2, c.F), torch.float64)
    red[0] = torch.from_numpy(ref["red"]).cuda()
    mx, cnt = put(g, ref["max"]), put(g, ref["packed"])
    dY, ds, dbeta = g.new((c.R * c.k, c.F)), g.new((c.R, c.F)), g.zeros((c.F,))
    H.call("dgcnn_edge_bn_bwd_apply_f32", *d.head(V), *d.par, relu, d.dmax.data_ptr(), c.F, d.dmean.data_ptr(), c.F, mx.data_ptr(), c.F,
           cnt.data_ptr(), red.data_ptr(), dY.data_ptr(), ds.data_ptr(), c.F, dbeta.data_ptr(), 0.0)
    return host(dY).reshape(c.R, c.k, c.F), host(ds)


# ---- dense, shape W ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", FR.W_KS)
def test_dense_gather_add(H, k):
    """Y bit-equal, `stats` summed over its slots EQUAL to the float64 column sums and sums of squares; with Y and with Y = NULL."""
    c = FR.dense_case(1, FR.W_N, k)
    ref = FR.dense_reference(c, 1)
    g = Guard()
    d = DenseDev(c, g)
    with far_view(c.V, c.ld) as V:
        Y, st = dense_gather_add(H, d, V)
        _, st0 = dense_gather_add(H, d, V, want_y=False)
        g.check()
    same_bits(Y, ref["y"], "Y")
    np.testing.assert_array_equal(st, ref["stats"], err_msg="stats")
    np.testing.assert_array_equal(st0, ref["stats"], err_msg="stats (Y = NULL)")


def test_dense_bwd_reduce(H):
    """red totals EQUAL to float64, with mx_in / cnt_in and with the maximum recomputed."""
    c = FR.dense_case(1, FR.W_N, FR.W_K)
    ref = FR.dense_reference(c, 1)
    g = Guard()
    d = DenseDev(c, g)
    mx, cnt = put(g, ref["max"]), put(g, ref["packed"])
    with far_view(c.V, c.ld) as V:
        for m, n in ((mx, cnt), (None, None)):
            red = g.zeros((H.stat_slots(), 2, c.F), torch.float64)
            H.call("dgcnn_edge_bn_bwd_reduce_f32", *d.head(V), *d.par, 1, d.dmax.data_ptr(), c.F, d.dmean.data_ptr(), c.F, p(m),
                   c.F if m is not None else 0, p(n), red.data_ptr())
            np.testing.assert_array_equal(host(red).sum(0), ref["red"], err_msg="red (%s)" % ("mx_in" if m is not None else "recomputed"))
        g.check()


@pytest.mark.parametrize("relu", [0, 1])
def test_dense_bwd_apply(H, relu):
    """dY and dYsum bit-equal to the float32 replay of tests/bn_reference.py (apply32), given the exact sums."""
    c = FR.dense_case(1, FR.W_N, FR.W_K)
    ref = FR.dense_reference(c, relu)
    g = Guard()
    d = DenseDev(c, g)
    with far_view(c.V, c.ld) as V:
        dY, ds = dense_apply(H, d, V, ref, relu)
        g.check()
    same_bits(dY, ref["dY"], "dY")
    same_bits(ds, ref["dYsum"], "dYsum")


def test_two_clouds(H):
    """B = 2, N = 132: rows 129..131 of each cloud are far -- the second cloud's base plus a far row (3.0e9 .. 4.4e9 elements from the
    pointer) is the one address no other case forms.  dgcnn_edge_gather_add_f32 and dgcnn_edge_bn_bwd_apply_f32."""
    c = FR.dense_case(2, FR.W_N2, FR.W_K)
    ref = FR.dense_reference(c, 1)
    g = Guard()
    d = DenseDev(c, g)
    with far_view(c.V, c.ld) as V:
        Y, st = dense_gather_add(H, d, V)
        dY, ds = dense_apply(H, d, V, ref, 1)
        g.check()
    same_bits(Y, ref["y"], "Y")
    np.testing.assert_array_equal(st, ref["stats"], err_msg="stats")
    same_bits(dY, ref["dY"], "dY")
    same_bits(ds, ref["dYsum"], "dYsum")


# ---- packed, shape W ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", FR.W_KS)
def test_packed_edge_stats(H, k):
    """Per-cloud sums EQUAL to float64: cloud 1 straddles the 2^31 mark, cloud 2 lies beyond it."""
    c = FR.packed_case(FR.W_OFF, k)
    ref = FR.packed_reference(c, 1)
    g = Guard()
    d = PackedDev(c, g)
    with far_view(c.V, c.ld) as V:
        st = d.stats(H, V)
        g.check()
    np.testing.assert_array_equal(st, ref["stats"])


def packed_forward(H, d, V):
    """-> (max, mean, packed count) of the counting entry, (max, mean) of the plain one."""
    c, g = d.c, d.g
    out = [g.new((c.R, c.F)) for _ in range(5)]
    H.call("dgcnn_seg_edge_bn_act_kreduce_cnt_f32", *d.head(V), d.rg.data_ptr(), *d.par, 1, out[0].data_ptr(), c.F, out[1].data_ptr(), c.F,
           out[2].data_ptr())
    H.call("dgcnn_seg_edge_bn_act_kreduce_f32", *d.head(V), d.rg.data_ptr(), *d.par, 1, out[3].data_ptr(), c.F, out[4].data_ptr(), c.F)
    return [host(t) for t in out]


def packed_apply(H, d, V, ref):
    c, g = d.c, d.g
    c1, c2 = g.new((c.nseg, c.F)), g.new((c.nseg, c.F))
    H.call("dgcnn_seg_bn_bwd_finalize_f32", put(g, ref["red"]).data_ptr(), c.nseg, c.F, d.off.data_ptr(), c.k, c1.data_ptr(), c2.data_ptr(),
           0, 0.0)
    same_bits(host(c1), ref["c1"], "c1")
    same_bits(host(c2), ref["c2"], "c2")
    mx, cnt = put(g, ref["max"]), put(g, ref["packed"])
    dY, ds = g.new((c.R * c.k, c.F)), g.new((c.R, c.F))
    H.call("dgcnn_seg_edge_bn_bwd_apply_f32", *d.head(V), d.rg.data_ptr(), *d.par, 1, d.dmax.data_ptr(), c.F, d.dmean.data_ptr(), c.F,
           mx.data_ptr(), c.F, cnt.data_ptr(), c1.data_ptr(), c2.data_ptr(), dY.data_ptr(), ds.data_ptr(), c.F)
    return host(dY).reshape(c.R, c.k, c.F), host(ds)


def test_packed_forward_max_mean_counts(H):
    c = FR.packed_case(FR.W_OFF, FR.W_K)
    ref = FR.packed_reference(c, 1)
    g = Guard()
    d = PackedDev(c, g)
    with far_view(c.V, c.ld) as V:
        mx, mn, cnt, mx0, mn0 = packed_forward(H, d, V)
        g.check()
    same_bits(mx, ref["max"], "max")
    same_bits(mn, ref["mean"], "mean")
    same_bits(cnt, ref["packed"], "packed counts")
    same_bits(mx0, mx, "max of the entry without counts")
    same_bits(mn0, mn, "mean of the entry without counts")


def test_packed_bwd_apply(H):
    c = FR.packed_case(FR.W_OFF, FR.W_K)
    ref = FR.packed_reference(c, 1)
    g = Guard()
    d = PackedDev(c, g)
    with far_view(c.V, c.ld) as V:
        dY, ds = packed_apply(H, d, V, ref)
        g.check()
    same_bits(dY, ref["dY"], "dY")
    same_bits(ds, ref["dYsum"], "dYsum")


def test_one_cloud_tower_gives_the_dense_entries_bits(H):
    """include/dgcnn_hip.h: a one-cloud tower with the dense kernels' mean / rstd gives the dense entries' outputs bit for bit -- here
    with rows 129.. of that cloud far.  Both sides are also held to the reference."""
    dc = FR.dense_case(1, FR.W_N, FR.W_K)
    pc = FR.one_cloud_tower(dc)
    ref = FR.dense_reference(dc, 1)
    g = Guard()
    d, q = DenseDev(dc, g), PackedDev(pc, g)
    F = dc.F
    with far_view(dc.V, dc.ld) as V:
        _, st = dense_gather_add(H, d, V, want_y=False)
        pst = q.stats(H, V)
        fwd = [g.new((dc.R, F)) for _ in range(3)]
        H.call("dgcnn_edge_bn_act_kreduce_f32", *d.head(V), *d.par, 1, fwd[0].data_ptr(), F, fwd[1].data_ptr(), F, fwd[2].data_ptr())
        mx, mn, cnt, _, _ = packed_forward(H, q, V)
        dY, ds = dense_apply(H, d, V, ref, 1)
        pdY, pds = packed_apply(H, q, V, FR.packed_reference(pc, 1))
        g.check()
    np.testing.assert_array_equal(st, ref["stats"])
    np.testing.assert_array_equal(pst[0], st)
    for got, tower, key in zip([host(t) for t in fwd], (mx, mn, cnt), ("max", "mean", "packed")):
        same_bits(got, ref[key], key)
        same_bits(tower, got, key + " of the one-cloud tower")
    same_bits(dY, ref["dY"], "dY")
    same_bits(ds, ref["dYsum"], "dYsum")
    same_bits(pdY, dY, "dY of the one-cloud tower")
    same_bits(pds, ds, "dYsum of the one-cloud tower")


# ---- shape R: the other operand at its limit ---------------------------------------------------------------------------------------
def _r_bound(n_terms, sums):
    """(2, F): (n_terms + 8) 2^-24 sum |term| per column for sum y and sum y^2 (bn_reference.sum_bound, as tests/test_gpu_bn_kernels.py)."""
    return np.stack([BR.sum_bound(n_terms, sums[2]), BR.sum_bound(n_terms, sums[1])])


def _r_device(c, g):
    return put(g, c.U), put(g, c.idx)


def test_shape_r_dense_statistics(H):
    """N = 2^24 - 256 rows of ld = 132 (N * ld = 2 214 558 720): rows 16 268 816.. are far, and 28 % of the points read one.
    Asserted: the any-order fp32 summation bound (n_terms + 8) 2^-24 sum |term| per column, n_terms = N k = 33.5 M.  Measured on
    MI355X: |err| = 0 in both sums -- the values are quarters, and the fp32 chains of this kernel (one thread's points, then a block's
    point groups, before the double-precision slots) are short enough to stay exact on them; 1.9 s wall, most of it the upload."""
    c = FR.r_case()
    g = Guard()
    U, idx = _r_device(c, g)
    st = g.zeros((H.stat_slots(), 2, c.F), torch.float64)
    with far_view(c.V, c.ld) as V:
        H.call("dgcnn_edge_gather_add_f32", V, c.ld, U.data_ptr(), c.F, idx.data_ptr(), 1, c.N, c.k, c.F, 0, st.data_ptr())
        got = host(st).sum(0)
        g.check()
    tot = c.sums.sum(0)
    err, bound = np.abs(got - tot[:2]), _r_bound(c.N * c.k, tot)
    print("dense: worst |err| / bound = %.3g, worst |err| / (2^-24 sum |term|) = %.4g" % (
        (err / bound).max(), (err / (2.0 ** -24 * np.stack([tot[2], tot[1]]))).max()))
    assert (err <= bound).all()


def test_shape_r_packed_statistics(H):
    """The same tower through dgcnn_seg_edge_stats_f32 with clouds of 5 M, 7 M and 4.8 M rows (the last holds the far rows), the bound
    per cloud with n_terms = n_b k.  Measured on MI355X: |err| = 0 in every cloud, 0.1 s wall (the case is cached)."""
    c = FR.r_case()
    g = Guard()
    U, idx = _r_device(c, g)
    off = put(g, c.off)
    nb = int(H.load().dgcnn_seg_stats_workspace_bytes(c.N, c.nseg, c.F))
    ws = g.new((nb // 8,), torch.float64)
    st = g.new((c.nseg, 2, c.F), torch.float64)
    with far_view(c.V, c.ld) as V:
        H.call("dgcnn_seg_edge_stats_f32", V, c.ld, U.data_ptr(), c.F, idx.data_ptr(), c.N, c.k, c.F, off.data_ptr(), c.nseg, st.data_ptr(),
               ws.data_ptr(), nb)
        got = host(st)
        g.check()
    for b in range(c.nseg):
        err, bound = np.abs(got[b] - c.sums[b, :2]), _r_bound(c.sizes[b] * c.k, c.sums[b])
        print("cloud %d: worst |err| / bound = %.3g, worst |err| / (2^-24 sum |term|) = %.4g" % (
            b, (err / bound).max(), (err / (2.0 ** -24 * np.stack([c.sums[b, 2], c.sums[b, 1]]))).max()))
        assert (err <= bound).all(), "cloud %d" % b


# ---- just outside the contract, and its last accepted shape ------------------------------------------------------------------------
def _entries(H, g, V, ldv, N, F=FR.W_F, k=FR.W_K, rows_out=256):
    """name -> (argument list, the tensors the call may write) of every gathering entry on one cloud / tower of N rows; small
    valid pointers throughout (a refused call must not touch them, an accepted one writes rows_out >= N rows)."""
    U, idx = g.zeros((rows_out, F)), g.zeros((rows_out, k), torch.int32)
    v, db = g.zeros((F,)), g.zeros((F,))
    a, b, cnt = g.new((rows_out, F)), g.new((rows_out, F)), g.new((rows_out, F))
    big = g.new((rows_out * k, F))
    red = g.new((H.stat_slots(), 2, F), torch.float64)
    seg = g.put(np.array([0, min(N, rows_out)], np.int32))
    rg = g.zeros((rows_out,), torch.int32)
    nb = 4 * 1024 * 1024
    ws = g.new((nb // 8,), torch.float64)
    sst = g.new((1, 2, F), torch.float64)
    dn = (V, ldv, U.data_ptr(), F, idx.data_ptr(), 1, N, k, F)
    pk = (V, ldv, U.data_ptr(), F, idx.data_ptr(), N, k, F)
    par = (v.data_ptr(), v.data_ptr(), v.data_ptr())
    grads = (a.data_ptr(), F, b.data_ptr(), F)
    return U, idx, {
        "dgcnn_edge_gather_add_f32": (dn + (big.data_ptr(), red.data_ptr()), [big, red]),
        "dgcnn_edge_bn_act_kreduce_f32": (dn + par + (1, a.data_ptr(), F, b.data_ptr(), F, cnt.data_ptr()), [a, b, cnt]),
        "dgcnn_edge_bn_bwd_reduce_f32": (dn + par + (1,) + grads + (0, 0, 0, red.data_ptr()), [red]),
        "dgcnn_edge_bn_bwd_apply_f32": (dn + par + (1,) + grads + (0, 0, 0, red.data_ptr(), big.data_ptr(), cnt.data_ptr(), F, db.data_ptr(), 0.0),
                                        [big, cnt]),
        "dgcnn_seg_edge_stats_f32": (pk + (seg.data_ptr(), 1, sst.data_ptr(), ws.data_ptr(), nb), [sst, ws]),
        "dgcnn_seg_edge_bn_act_kreduce_f32": (pk + (rg.data_ptr(),) + par + (1, a.data_ptr(), F, b.data_ptr(), F), [a, b]),
        "dgcnn_seg_edge_bn_act_kreduce_cnt_f32": (pk + (rg.data_ptr(),) + par + (1, a.data_ptr(), F, b.data_ptr(), F, cnt.data_ptr()),
                                                  [a, b, cnt]),
        "dgcnn_seg_edge_bn_bwd_apply_f32": (pk + (rg.data_ptr(),) + par + (1,) + grads + (a.data_ptr(), F, b.data_ptr()) + par[:2]
                                            + (big.data_ptr(), cnt.data_ptr(), F), [big, cnt]),
    }


@pytest.mark.parametrize("N,ldv", [(160, 1 << 24), (1 << 24, 64), (257, (1 << 24) - 4)], ids=["ldv=2^24", "N=2^24", "N*ldv>=2^32"])
def test_refusals_just_outside_the_contract(H, N, ldv):
    """ldv = 2^24, N (packed: rows) = 2^24, and N * ldv = 2^32 + 15 351 808 with both factors in range: DGCNN_EUNSUP from every entry,
    nothing written."""
    g = Guard()
    V = g.zeros((64, FR.W_F))
    _, _, entries = _entries(H, g, V.data_ptr(), ldv, N)
    for name, (args, outs) in entries.items():
        assert rc(H, name, *args) == EUNSUP, name
        torch.cuda.synchronize()
        for t in outs:
            assert (host(t) == SENT).all(), "%s: a refused call wrote to an output" % name
    g.check()


def test_the_last_accepted_shape(H):
    """N = 256, ldv = 2^24 - 4: N * ldv = 2^32 - 1024 passes every check.  idx names rows 0..3 only, so a buffer of 3 ldv + F floats
    (201 MB) is all the call can touch; the return code is what is asserted, and Y of the first entry that the rows were read."""
    N, ldv, F, k = 256, FR.W_LD, FR.W_F, FR.W_K
    assert N * ldv == (1 << 32) - 1024
    rng = np.random.default_rng(256)
    vals = FR.quarter(rng, (4, F))
    g = Guard()
    with far_view(vals, ldv) as V:
        U, idx, entries = _entries(H, g, V, ldv, N)
        nbr = rng.integers(0, 4, (N, k)).astype(np.int32)
        idx.copy_(torch.from_numpy(nbr).cuda())
        for name, (args, outs) in entries.items():
            assert rc(H, name, *args) == 0, "%s: %s" % (name, H.load().dgcnn_last_error().decode())
            if name == "dgcnn_edge_gather_add_f32":
                same_bits(host(outs[0]).reshape(N, k, F), vals[nbr], "Y")
        g.check()

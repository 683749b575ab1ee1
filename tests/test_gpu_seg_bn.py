"""Per-cloud BatchNorm of a packed tower (run with -m gpu on an MI355X): the kernels of csrc/seg_bn.hip against float64 / the fp32
replays of tests/bn_reference.py, then the engine, ops.*(bn_per_cloud=True), model.build under flags.BN_PER_CLOUD and the
inference loop against the float64 oracle on every cloud ALONE (tests/seg_bn_reference.py) -- a cloud's outputs must not depend on
the clouds that share its tower."""
import numpy as np
import pytest
import torch

from oracle import dgcnn_oracle as O
import bn_reference as BR
import seg_bn_reference as SR
from gpu_helpers import Guard, capture_layers, dev, host, set_vars

pytestmark = pytest.mark.gpu

COL_SIZES = [1, 63, 64, 65, 130, 5]       # R = 328: below a 64-row chunk, exactly one, straddling two, spanning three, partial last chunk
EDGE_SIZES = [21, 64, 150, 40]
TOWER_SIZES = [21, 700, 64, 333]


@pytest.fixture()
def dg():
    import dgcnn
    from dgcnn import _engine as E
    dgcnn.reset()
    yield dgcnn
    E.DETERMINISTIC = E.DETERMINISTIC_ENV_DEFAULT
    E.EDGE_MLP_DTYPE = "f32"
    dgcnn.reset()


def offsets_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def row_group_of(sizes):
    return np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)


def padded(g, a, pad):
    """`a` (R, F) as the leading F columns of a guarded (R, F + pad) buffer whose padding holds the sentinel."""
    R, F = a.shape
    buf = g.new((R, F + pad))
    v = buf[:, :F]
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return buf, v


def ws_of(H, g, R, nseg, F):
    nb = int(H.load().dgcnn_seg_stats_workspace_bytes(R, nseg, F))
    return g.new((nb // 8,), torch.float64), nb


def seg_colstats(H, g, xv, ld, R, F, offd, nseg):
    st = g.new((nseg, 2, F), torch.float64)                    # written, not accumulated: starts as the sentinel
    ws, nb = ws_of(H, g, R, nseg, F)
    H.call("dgcnn_seg_colstats_f32", xv.data_ptr(), ld, R, F, offd.data_ptr(), nseg, st.data_ptr(), ws.data_ptr(), nb)
    return st


def check_sums(got, rows64, n_terms, what):
    """got (2, F) against the float64 sums of `rows64` (n, F): the project's any-order fp32 bound, (n + 8) 2^-24 sum |term|."""
    S, Q = rows64.sum(0), (rows64 * rows64).sum(0)
    bS, bQ = BR.sum_bound(n_terms, np.abs(rows64).sum(0)), BR.sum_bound(n_terms, (rows64 * rows64).sum(0))
    eS, eQ = np.abs(got[0] - S), np.abs(got[1] - Q)
    assert (eS <= bS).all() and (eQ <= bQ).all(), "%s: worst err / bound %.3g (sum) %.3g (squares)" % (
        what, float((eS / np.maximum(bS, 1e-300)).max()), float((eQ / np.maximum(bQ, 1e-300)).max()))
    return float((eS / np.maximum(bS, 1e-300)).max()), float((eQ / np.maximum(bQ, 1e-300)).max())


# ------------------------------------------------------------------------------------------
# 1. the kernels through H.call
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,pad", [(3, 0), (70, 5), (64, 4), (1024, 4), (1024, 3)],
                         ids=["F3-scalar", "F70-scalar", "F64-float4", "F1024-float4x4", "F1024-unaligned"])
def test_seg_colstats(dg, F, pad):
    """Per (cloud, column) both sums within the any-order fp32 bound of float64; two runs bit-identical; nothing outside the buffers."""
    from dgcnn import _hip as H
    rng = np.random.default_rng(F + pad)
    off = offsets_of(COL_SIZES)
    R, nseg = int(off[-1]), len(COL_SIZES)
    x = rng.normal(0.5, 2.0, (R, F)).astype(np.float32)
    g = Guard()
    buf, xv = padded(g, x, pad)
    offd = g.put(off.astype(np.int32))
    a = seg_colstats(H, g, xv, F + pad, R, F, offd, nseg)
    b = seg_colstats(H, g, xv, F + pad, R, F, offd, nseg)
    g.check()
    assert torch.equal(a, b), "two runs of the fixed-order sums differ"
    got = host(a)
    worst = (0.0, 0.0)
    for c in range(nseg):
        worst = max(worst, check_sums(got[c], x[off[c]:off[c + 1]].astype(np.float64), COL_SIZES[c], "cloud %d" % c))
    print("seg_colstats F=%d pad=%d: worst err / bound %.3g (sum) %.3g (squares)" % ((F, pad) + worst))


def test_seg_colstats_of_a_cloud_wherever_its_chunks_fall(dg):
    """The same 130-row cloud at offset 0 and at offset 37 behind another cloud: the pieces are cut differently (the summation order
    changes), both stay within the bound."""
    from dgcnn import _hip as H
    rng = np.random.default_rng(5)
    F = 72
    body = rng.normal(0.5, 2.0, (130, F)).astype(np.float32)
    lead = rng.normal(size=(37, F)).astype(np.float32)
    for sizes, x, c in (([130], body, 0), ([37, 130], np.concatenate([lead, body]), 1)):
        off = offsets_of(sizes)
        g = Guard()
        st = seg_colstats(H, g, g.put(x), F, len(x), F, g.put(off.astype(np.int32)), len(sizes))
        g.check()
        check_sums(host(st)[c], body.astype(np.float64), 130, "offset %d" % off[c])


def edge_case(rng, sizes, k, F):
    """[U | V] halves of one (R, 2F) buffer, idx = random tower rows inside the row's own cloud (self and duplicates included)."""
    off = offsets_of(sizes)
    R = int(off[-1])
    UV = rng.normal(0.2, 1.5, (R, 2 * F)).astype(np.float32)
    idx = np.concatenate([rng.integers(off[b], off[b + 1], (sizes[b], k)) for b in range(len(sizes))]).astype(np.int32)
    y = BR.edge_rows32(UV[:, F:], UV[:, :F], idx.reshape(1, R, k), 1, R)      # (R, k, F), the single fp32 add
    return off, R, UV, idx, y


def edge_head(UVd, idxd, R, k, F):
    return (UVd[:, F:].data_ptr(), 2 * F, UVd.data_ptr(), 2 * F, idxd.data_ptr(), R, k, F)


@pytest.mark.parametrize("F", [32, 128])
@pytest.mark.parametrize("k", [20, 5])
def test_seg_edge_stats(dg, k, F):
    from dgcnn import _hip as H
    rng = np.random.default_rng(k * 1000 + F)
    off, R, UV, idx, y = edge_case(rng, EDGE_SIZES, k, F)
    nseg = len(EDGE_SIZES)
    g = Guard()
    UVd, idxd, offd = g.put(UV), g.put(idx), g.put(off.astype(np.int32))
    out = []
    for _ in range(2):
        st = g.new((nseg, 2, F), torch.float64)
        ws, nb = ws_of(H, g, R, nseg, F)
        H.call("dgcnn_seg_edge_stats_f32", *edge_head(UVd, idxd, R, k, F), offd.data_ptr(), nseg, st.data_ptr(), ws.data_ptr(), nb)
        out.append(st)
    g.check()
    assert torch.equal(out[0], out[1]), "two runs of the fixed-order sums differ"
    got = host(out[0])
    worst = (0.0, 0.0)
    for b in range(nseg):
        rows = y[off[b]:off[b + 1]].reshape(-1, F).astype(np.float64)
        worst = max(worst, check_sums(got[b], rows, EDGE_SIZES[b] * k, "cloud %d" % b))
    print("seg_edge_stats k=%d F=%d: worst err / bound %.3g (sum) %.3g (squares)" % ((k, F) + worst))


@pytest.mark.parametrize("F,k", [(3, 1), (64, 20)])
def test_seg_bn_finalize(dg, F, k):
    """From the double sums the test feeds: f32(finalize64(S_b, Q_b, n_b k)) within one ulp.  A one-point cloud, a constant column
    (rstd = 1 / sqrt(eps)), a column whose Q / n - mu^2 rounds negative (clamped at 0), a cancelling column (1000 +- 0.01)."""
    from dgcnn import _hip as H
    rng = np.random.default_rng(F)
    sizes = [1, 4000, 37]
    off = offsets_of(sizes)
    nseg = len(sizes)
    S, Q = np.empty((nseg, F)), np.empty((nseg, F))
    for b, n in enumerate(sizes):
        Y = rng.normal(2, 3, (n * k, F)).astype(np.float32).astype(np.float64)
        Y[:, 0] = 1.25                                                          # constant
        if F >= 3:
            Y[:, 1] = (1000 + 0.01 * rng.normal(size=n * k)).astype(np.float32)
        S[b], Q[b] = Y.sum(0), (Y * Y).sum(0)
    if F >= 3:
        S[2, 2], Q[2, 2] = 3.0 * 37 * k / 3.0, 2.9999999 * 37 * k / 3.0         # Q / n - mu^2 < 0 from rounding: clamps to 0
    g = Guard()
    st = g.put(np.stack([S, Q], axis=1))                                        # (nseg, 2, F) float64
    mean, rstd = g.new((nseg, F)), g.new((nseg, F))
    H.call("dgcnn_seg_bn_finalize_f32", st.data_ptr(), nseg, F, g.put(off.astype(np.int32)).data_ptr(), k, BR.EPS, mean.data_ptr(),
           rstd.data_ptr())
    g.check()
    m, r = host(mean), host(rstd)
    for b, n in enumerate(sizes):
        mu64, rs64 = BR.finalize64(S[b], Q[b], n * k)
        em, er = mu64.astype(np.float32), rs64.astype(np.float32)
        assert (np.abs(m[b] - em) <= np.spacing(np.abs(em))).all(), "cloud %d mean" % b
        assert (np.abs(r[b] - er) <= np.spacing(er)).all(), "cloud %d rstd" % b
        assert m[b, 0] == np.float32(1.25) and r[b, 0] == np.float32(1.0 / np.sqrt(np.float64(np.float32(BR.EPS))))
    if F >= 3:
        assert m[2, 2] == 1 and r[2, 2] == r[2, 0]


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("F,pad", [(3, 0), (70, 5), (1024, 4)], ids=["F3-scalar", "F70-scalar", "F1024-float4"])
def test_seg_bn_act(dg, F, pad, relu):
    """Bit-equal to bn_z32 with the table rows broadcast through row_group; out2; padded leading dimensions; the row_group = NULL
    form (g = r: the per-cloud max-pool, rows = nseg)."""
    from dgcnn import _hip as H
    rng = np.random.default_rng(F + relu)
    off = offsets_of(COL_SIZES)
    R, nseg = int(off[-1]), len(COL_SIZES)
    rg = row_group_of(COL_SIZES)
    T = rng.normal(0.3, 2.0, (R, F)).astype(np.float32)
    mu, rs = rng.normal(0.3, 0.5, (nseg, F)).astype(np.float32), rng.uniform(0.3, 3.0, (nseg, F)).astype(np.float32)
    be = rng.normal(0, 0.3, F).astype(np.float32)
    g = Guard()
    _, Tv = padded(g, T, pad)
    mud, rsd, bed, rgd = g.put(mu), g.put(rs), g.put(be), g.put(rg)
    ob, ov = padded(g, np.zeros((R, F), np.float32), pad)
    o2b, o2v = padded(g, np.zeros((R, F), np.float32), pad + 4)
    H.call("dgcnn_seg_bn_act_f32", Tv.data_ptr(), F + pad, R, F, rgd.data_ptr(), mud.data_ptr(), rsd.data_ptr(), bed.data_ptr(), relu,
           ov.data_ptr(), F + pad, o2v.data_ptr(), F + pad + 4)
    ref, _ = BR.bn_z32(T, mu[rg], rs[rg], be, relu)
    np.testing.assert_array_equal(host(ob)[:, :F], ref)
    np.testing.assert_array_equal(host(o2b)[:, :F], ref)
    if pad:
        assert (host(ob)[:, F:] == 777.0).all() and (host(o2b)[:, F:] == 777.0).all(), "the padding columns were written"
    # row_group = NULL: row b of a (nseg, F) tensor with row b of the tables
    G = rng.normal(0.3, 2.0, (nseg, F)).astype(np.float32)
    go = g.new((nseg, F))
    H.call("dgcnn_seg_bn_act_f32", g.put(G).data_ptr(), F, nseg, F, None, mud.data_ptr(), rsd.data_ptr(), bed.data_ptr(), relu,
           go.data_ptr(), F, None, 0)
    g.check()
    np.testing.assert_array_equal(host(go), BR.bn_z32(G, mu, rs, be, relu)[0])


@pytest.mark.parametrize("F", [32, 128])
@pytest.mark.parametrize("k", [20, 5])
def test_seg_edge_bn_act_kreduce(dg, k, F):
    """max_out bit for bit; mean_out equal to the fp32 replay (sum in m order, then * 1.0f / k), as the dense edge kernel is checked."""
    from dgcnn import _hip as H
    rng = np.random.default_rng(k * 100 + F)
    off, R, UV, idx, y = edge_case(rng, EDGE_SIZES, k, F)
    nseg = len(EDGE_SIZES)
    rg = row_group_of(EDGE_SIZES)
    mu, rs = rng.normal(0.2, 0.5, (nseg, F)).astype(np.float32), rng.uniform(0.3, 2.0, (nseg, F)).astype(np.float32)
    be = rng.normal(0, 0.3, F).astype(np.float32)
    g = Guard()
    UVd, idxd = g.put(UV), g.put(idx)
    mm = g.new((R, 2 * F + 4))                                     # [max | mean] column slices of one padded buffer, as the model's
    mx, mn = mm[:, :F], mm[:, F:2 * F]
    H.call("dgcnn_seg_edge_bn_act_kreduce_f32", *edge_head(UVd, idxd, R, k, F), g.put(rg).data_ptr(), g.put(mu).data_ptr(),
           g.put(rs).data_ptr(), g.put(be).data_ptr(), 1, mx.data_ptr(), 2 * F + 4, mn.data_ptr(), 2 * F + 4)
    g.check()
    out = host(mm)
    assert (out[:, 2 * F:] == 777.0).all()
    for b in range(nseg):
        fw = BR.Fwd(y[off[b]:off[b + 1]], mu[b], rs[b], be, 1)
        np.testing.assert_array_equal(out[off[b]:off[b + 1], :F], fw.mx, err_msg="cloud %d max" % b)
        np.testing.assert_array_equal(out[off[b]:off[b + 1], F:2 * F], fw.mean32, err_msg="cloud %d mean" % b)


def test_one_cloud_tower_is_the_dense_kernels(dg):
    """nseg = 1: with the dense kernels' own mean / rstd the two apply kernels equal dgcnn_bn_act_kreduce_f32 /
    dgcnn_edge_bn_act_kreduce_f32 bit for bit; the per-cloud sums agree with the total of the dense slots within the bound."""
    from dgcnn import _hip as H
    rng = np.random.default_rng(8)
    g = Guard()
    nslots = H.stat_slots()
    # ---- k = 1
    R, F = 333, 64
    T = rng.normal(0.4, 2.0, (R, F)).astype(np.float32)
    Td, offd, rgd = g.put(T), g.put(np.array([0, R], np.int32)), g.put(np.zeros(R, np.int32))
    be = g.put(rng.normal(0, 0.3, F).astype(np.float32))
    dst = g.zeros((nslots, 2, F), torch.float64)
    nb = int(H.load().dgcnn_det_workspace_bytes(F))
    dws = g.new((nb // 4,))
    H.call("dgcnn_colstats_det_f32", Td.data_ptr(), R, F, F, dst.data_ptr(), dws.data_ptr(), nb)
    mean, rstd = g.new((F,)), g.new((F,))
    H.call("dgcnn_bn_finalize_f32", dst.data_ptr(), F, float(R), BR.EPS, mean.data_ptr(), rstd.data_ptr())
    sst = seg_colstats(H, g, Td, F, R, F, offd, 1)
    T64 = T.astype(np.float64)
    check_sums(host(sst)[0], T64, R, "k = 1 per-cloud sums")
    dense_total = host(dst).sum(0)
    bS, bQ = BR.sum_bound(R, np.abs(T64).sum(0)), BR.sum_bound(R, (T64 * T64).sum(0))
    assert (np.abs(host(sst)[0][0] - dense_total[0]) <= 2 * bS).all() and (np.abs(host(sst)[0][1] - dense_total[1]) <= 2 * bQ).all()
    od, os_ = g.new((R, F)), g.new((R, F))
    H.call("dgcnn_bn_act_kreduce_f32", Td.data_ptr(), R, 1, F, mean.data_ptr(), rstd.data_ptr(), be.data_ptr(), 1, od.data_ptr(), F,
           0, 0, 0, 0, 0)
    H.call("dgcnn_seg_bn_act_f32", Td.data_ptr(), F, R, F, rgd.data_ptr(), mean.data_ptr(), rstd.data_ptr(), be.data_ptr(), 1,
           os_.data_ptr(), F, None, 0)
    assert torch.equal(od, os_)
    # ---- conv0
    k, F = 20, 32
    off, R, UV, idx, y = edge_case(rng, [150], k, F)
    UVd, idxd = g.put(UV), g.put(idx)
    offd, rgd = g.put(np.array([0, R], np.int32)), g.put(np.zeros(R, np.int32))
    be = g.put(rng.normal(0, 0.3, F).astype(np.float32))
    dst = g.zeros((nslots, 2, F), torch.float64)
    H.call("dgcnn_edge_gather_add_f32", UVd[:, F:].data_ptr(), 2 * F, UVd.data_ptr(), 2 * F, idxd.data_ptr(), 1, R, k, F, 0, dst.data_ptr())
    mean, rstd = g.new((F,)), g.new((F,))
    H.call("dgcnn_bn_finalize_f32", dst.data_ptr(), F, float(R * k), BR.EPS, mean.data_ptr(), rstd.data_ptr())
    sst = g.new((1, 2, F), torch.float64)
    ws, nb = ws_of(H, g, R, 1, F)
    H.call("dgcnn_seg_edge_stats_f32", *edge_head(UVd, idxd, R, k, F), offd.data_ptr(), 1, sst.data_ptr(), ws.data_ptr(), nb)
    y64 = y.reshape(-1, F).astype(np.float64)
    check_sums(host(sst)[0], y64, R * k, "conv0 per-cloud sums")
    dense_total = host(dst).sum(0)
    bS, bQ = BR.sum_bound(R * k, np.abs(y64).sum(0)), BR.sum_bound(R * k, (y64 * y64).sum(0))
    assert (np.abs(host(sst)[0][0] - dense_total[0]) <= 2 * bS).all() and (np.abs(host(sst)[0][1] - dense_total[1]) <= 2 * bQ).all()
    md, ms = g.new((R, 2 * F)), g.new((R, 2 * F))
    H.call("dgcnn_edge_bn_act_kreduce_f32", UVd[:, F:].data_ptr(), 2 * F, UVd.data_ptr(), 2 * F, idxd.data_ptr(), 1, R, k, F,
           mean.data_ptr(), rstd.data_ptr(), be.data_ptr(), 1, md[:, :F].data_ptr(), 2 * F, md[:, F:].data_ptr(), 2 * F, 0)
    H.call("dgcnn_seg_edge_bn_act_kreduce_f32", *edge_head(UVd, idxd, R, k, F), rgd.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
           be.data_ptr(), 1, ms[:, :F].data_ptr(), 2 * F, ms[:, F:].data_ptr(), 2 * F)
    g.check()
    assert torch.equal(md, ms)


def test_seg_bn_refusals_write_nothing(dg):
    """A null pointer, F % 4 != 0 for the two edge entries and a small workspace are refused; every output keeps its sentinel."""
    from dgcnn import _hip as H
    rng = np.random.default_rng(1)
    k = 5
    off, R, UV, idx, _ = edge_case(rng, [30, 40], k, 8)
    g = Guard()
    UVd, idxd, offd, rgd = g.put(UV), g.put(idx), g.put(off.astype(np.int32)), g.put(row_group_of([30, 40]))
    F = 8
    st = g.new((2, 2, F), torch.float64)
    ws, nb = ws_of(H, g, R, 2, F)
    out, tab = g.new((R, 2 * F)), g.new((2, F))
    with pytest.raises(ValueError):                                                        # null input
        H.call("dgcnn_seg_colstats_f32", None, 2 * F, R, F, offd.data_ptr(), 2, st.data_ptr(), ws.data_ptr(), nb)
    with pytest.raises(ValueError):                                                        # more clouds than rows
        H.call("dgcnn_seg_colstats_f32", UVd.data_ptr(), 2 * F, R, F, offd.data_ptr(), R + 1, st.data_ptr(), ws.data_ptr(), nb)
    with pytest.raises(H.HipError, match="workspace too small"):
        H.call("dgcnn_seg_colstats_f32", UVd.data_ptr(), 2 * F, R, F, offd.data_ptr(), 2, st.data_ptr(), ws.data_ptr(), nb - 8)
    with pytest.raises(H.HipError, match="workspace too small"):
        H.call("dgcnn_seg_edge_stats_f32", *edge_head(UVd, idxd, R, k, F), offd.data_ptr(), 2, st.data_ptr(), ws.data_ptr(), nb - 8)
    with pytest.raises(ValueError):                                                        # null idx
        H.call("dgcnn_seg_edge_stats_f32", UVd[:, F:].data_ptr(), 2 * F, UVd.data_ptr(), 2 * F, None, R, k, F, offd.data_ptr(), 2,
               st.data_ptr(), ws.data_ptr(), nb)
    with pytest.raises(H.HipError, match="multiple of 4"):                                 # F % 4
        H.call("dgcnn_seg_edge_stats_f32", UVd[:, F:].data_ptr(), 2 * F, UVd.data_ptr(), 2 * F, idxd.data_ptr(), R, k, 6, offd.data_ptr(), 2,
               st.data_ptr(), ws.data_ptr(), nb)
    with pytest.raises(H.HipError, match="multiple of 4"):
        H.call("dgcnn_seg_edge_bn_act_kreduce_f32", UVd[:, F:].data_ptr(), 2 * F, UVd.data_ptr(), 2 * F, idxd.data_ptr(), R, k, 6,
               rgd.data_ptr(), tab.data_ptr(), tab.data_ptr(), tab.data_ptr(), 1, out.data_ptr(), 2 * F, None, 0)
    with pytest.raises(ValueError):                                                        # no row -> cloud map
        H.call("dgcnn_seg_edge_bn_act_kreduce_f32", *edge_head(UVd, idxd, R, k, F), None, tab.data_ptr(), tab.data_ptr(), tab.data_ptr(),
               1, out.data_ptr(), 2 * F, None, 0)
    with pytest.raises(ValueError):                                                        # null tables
        H.call("dgcnn_seg_bn_act_f32", UVd.data_ptr(), 2 * F, R, F, rgd.data_ptr(), None, tab.data_ptr(), tab.data_ptr(), 1,
               out.data_ptr(), 2 * F, None, 0)
    with pytest.raises(ValueError):
        H.call("dgcnn_seg_bn_finalize_f32", st.data_ptr(), 2, F, None, k, BR.EPS, tab.data_ptr(), tab.data_ptr())
    g.check()
    for t in (st, out, tab, ws):
        assert (host(t) == 777.0).all(), "a refused call wrote to an output"


# ------------------------------------------------------------------------------------------
# 2. engine and ops: the EdgeConv stacks
# ------------------------------------------------------------------------------------------
def stack_params(rng, C, fl):
    P = {}
    cin = C
    for i, f in enumerate(fl):
        s = "EdgeConv%d/" % i
        P[s + "conv0/weights"] = rng.normal(0, 0.4, (2 * cin, f)).astype(np.float32)
        P[s + "conv0/BatchNorm/beta"] = rng.normal(0, 0.2, f).astype(np.float32)
        P[s + "conv1/weights"] = rng.normal(0, 0.2, (2 * f, 64)).astype(np.float32)
        P[s + "conv1/BatchNorm/beta"] = rng.normal(0, 0.2, 64).astype(np.float32)
        if i > 0 and f != fl[i - 1]:
            P[s + "shortcut/weights"] = rng.normal(0, 0.2, (64, f)).astype(np.float32)
            P[s + "shortcut/BatchNorm/beta"] = rng.normal(0, 0.2, f).astype(np.float32)
        cin = 64
    return P


def graphs_of(cap, L, off, k):
    """The captured packed graphs, each checked against the oracle's k-NN of the layer's own input, cloud by cloud, bit for bit."""
    out = []
    for i in range(L):
        xin, idx = cap.layers["EdgeConv%d" % i]
        assert idx.shape == (1, off[-1], k)
        flat = idx.reshape(-1, k)
        for b in range(len(off) - 1):
            part = flat[off[b]:off[b + 1]]
            assert part.min() >= off[b] and part.max() < off[b + 1], "layer %d cloud %d: an index outside the cloud" % (i, b)
            np.testing.assert_array_equal(part - off[b], O.k_nn(xin[0, off[b]:off[b + 1]][None], k)[0], err_msg="layer %d cloud %d" % (i, b))
        out.append(idx)
    return out


@pytest.mark.parametrize("residual", [False, True], ids=["edgeconv", "residual"])
def test_packed_stack_per_cloud_against_the_float64_oracle(dg, residual):
    """repeat_(residual_)edge_conv(bn_per_cloud=True) on four unequal clouds: graphs per cloud bit for bit, every tensor within
    rtol = atol = 1e-4 of the float64 oracle run on each cloud alone with those graphs.  32 -> 64 filters: the shortcut conv runs."""
    rng = np.random.default_rng(21 + residual)
    C, k, fl = 4, 20, [32, 64]
    off = offsets_of(TOWER_SIZES)
    R = int(off[-1])
    pts = rng.random((R, C), dtype=np.float32)
    P = stack_params(rng, C, fl)
    c = dg.ctx()
    c.begin_step()
    for n, v in P.items():
        c.get_variable(n, v.shape)
    set_vars(dg, P)
    fn = dg.ops.repeat_residual_edge_conv if residual else dg.ops.repeat_edge_conv
    with capture_layers() as cap:
        tensors = fn(dev(pts), 2, k, fl, False, offsets=off, bn_per_cloud=True)
    graphs = graphs_of(cap, 2, off, k)
    p64 = {n: v.astype(np.float64) for n, v in P.items()}
    ref = SR.stack_forward(pts.astype(np.float64), off, 2, k, fl, p64, residual, graphs)
    assert len(tensors) == len(ref) == 6
    worst = 0.0
    for j, (a, b) in enumerate(zip(tensors, ref)):
        assert tuple(a.shape) == b.shape == (1, R, 1, b.shape[-1])
        worst = max(worst, float(np.abs(host(a) - b).max()))
        np.testing.assert_allclose(host(a), b, rtol=1e-4, atol=1e-4, err_msg="tensor %d" % j)
    print("per-cloud %s stack: max |err| %.3g" % ("residual" if residual else "plain", worst))


# ------------------------------------------------------------------------------------------
# 3. model.build under BN_PER_CLOUD
# ------------------------------------------------------------------------------------------
MODELS = [("dgcnn", 2), ("dgcnn", 0), ("residual-dgcnn", 2), ("residual-dgcnn", 0), ("residual-dgcnn-nofc", 2)]


def model_flags(dg, model, fcl, **kw):
    base = dict(MODEL_NAME=model, EDGE_CONV_LAYERS=2, EDGE_CONV_FILTERS=[32, 64], KVALUE=20, NUM_CLASS=3, FC_LAYERS=fcl,
                FC_FILTERS=[64, 32][:fcl] if fcl else 64, TRAIN=False, NUM_CHANNEL=4)
    base.update(kw)
    return dg.DGCNN_FLAGS(**base)


def random_params(flags, rng, C):
    params = O.init_params(flags, C, seed=1)
    for n in params:
        if n.endswith("beta"):
            params[n] = rng.normal(0, 0.2, params[n].shape).astype(np.float32)
    return params


def build_with(dg, flags, params, pts, off):
    import dgcnn
    dg.trainval(flags).initialize()
    set_vars(dg, params)
    with capture_layers() as cap:
        logits = host(dgcnn.build(dev(pts), flags, **({} if off is None else {"offsets": off})))
    return logits, cap


@pytest.mark.parametrize("model,fcl", MODELS, ids=["%s-fc%d" % m for m in MODELS])
def test_model_logits_per_cloud(dg, model, fcl):
    """Four unequal clouds: with BN_PER_CLOUD the logits lie within 1e-3 (the project's bar) of the float64 oracle run on every
    cloud alone with the captured graphs; WITHOUT the flag the same tower differs from that reference by more than 1e-2 -- the
    two semantics are far apart at this shape (tests/test_seg_bn_reference.py), so the first assertion is not vacuous."""
    rng = np.random.default_rng(17)
    flags = model_flags(dg, model, fcl, BN_PER_CLOUD=True)
    off = offsets_of(TOWER_SIZES)
    R = int(off[-1])
    pts = rng.random((R, 4), dtype=np.float32)
    params = random_params(flags, rng, 4)
    p64 = {n: v.astype(np.float64) for n, v in params.items()}
    logits, cap = build_with(dg, flags, params, pts, off)
    assert logits.shape == (1, R, 3)
    graphs = graphs_of(cap, 2, off, 20)
    ref = SR.model_forward(pts.astype(np.float64), off, flags, p64, graphs)
    err = np.abs(logits - ref)
    print("%s fc%d per-cloud: logits max |err| %.3g" % (model, fcl, err.max()))
    assert err.max() <= 1e-3, "logits differ from the per-cloud reference: max %g at %s" % (err.max(), np.unravel_index(err.argmax(), err.shape))
    # the tower-wide statistics of the default packed path: another function of the same tower
    flags.BN_PER_CLOUD = False
    wide, cap_w = build_with(dg, flags, params, pts, off)
    ref_w = SR.model_forward(pts.astype(np.float64), off, flags, p64, graphs_of(cap_w, 2, off, 20))
    d = np.abs(wide - ref_w)
    print("%s fc%d tower-wide: max |difference| from the per-cloud reference %.3g" % (model, fcl, d.max()))
    assert d.max() > 1e-2


def test_companions_do_not_matter(dg, monkeypatch):
    """Cloud b's logits in the packed tower against model.build on cloud b ALONE (dense, B = 1), same library, same variables:
    layer 0's graph bit-identical; layer 1's graph of the single-cloud run is replaced by the packed run's (minus the offset), so
    both runs are on identical graphs.  Within 1e-3; the maximum is printed."""
    import dgcnn
    from dgcnn import _engine as E
    rng = np.random.default_rng(23)
    flags = model_flags(dg, "dgcnn", 2, BN_PER_CLOUD=True)
    off = offsets_of(TOWER_SIZES)
    pts = rng.random((int(off[-1]), 4), dtype=np.float32)
    params = random_params(flags, rng, 4)
    packed, cap = build_with(dg, flags, params, pts, off)
    graphs = [cap.layers["EdgeConv%d" % i][1] for i in range(2)]
    real_knn = E.knn
    worst = 0.0
    for b in range(len(TOWER_SIZES)):
        lo, hi = int(off[b]), int(off[b + 1])
        calls = []

        def knn(x2d, B, N, k, seed=None, seg=None):
            calls.append(len(calls))
            want = np.ascontiguousarray(graphs[len(calls) - 1][:, lo:hi] - lo).astype(np.int32)
            if len(calls) == 1:
                got = real_knn(x2d, B, N, k, seed=seed, seg=seg)
                np.testing.assert_array_equal(host(got), want, err_msg="cloud %d: layer 0's graph" % b)
                return got
            return dev(want)
        monkeypatch.setattr(E, "knn", knn)
        dg.trainval(flags).initialize()
        set_vars(dg, params)
        alone = host(dgcnn.build(dev(pts[None, lo:hi]), flags))
        monkeypatch.setattr(E, "knn", real_knn)
        assert len(calls) == 2 and alone.shape == (1, hi - lo, 3)
        d = float(np.abs(alone[0] - packed[0, lo:hi]).max())
        worst = max(worst, d)
        assert d <= 1e-3, "cloud %d: packed with companions vs alone differ by %g" % (b, d)
    print("companions: max |packed - alone| over the four clouds %.3g" % worst)


def test_dense_input_under_the_flag_is_the_packed_tower(dg):
    """(2, 300, 4) under BN_PER_CLOUD = the packed tower with offsets [0, 300, 600], bit for bit, shaped (2, 300, ncls); it differs
    from the dense tower-wide result by more than 1e-2.  B = 1 keeps the dense path (already per cloud): bit-equal with and without."""
    rng = np.random.default_rng(31)
    flags = model_flags(dg, "dgcnn", 2, BN_PER_CLOUD=True)
    pts = rng.random((2, 300, 4), dtype=np.float32)
    params = random_params(flags, rng, 4)
    dense_bpc, _ = build_with(dg, flags, params, pts, None)
    packed, _ = build_with(dg, flags, params, pts.reshape(600, 4), np.array([0, 300, 600]))
    assert dense_bpc.shape == (2, 300, 3) and packed.shape == (1, 600, 3)
    np.testing.assert_array_equal(dense_bpc.reshape(1, 600, 3), packed)
    one_bpc, _ = build_with(dg, flags, params, pts[:1], None)
    flags.BN_PER_CLOUD = False
    wide, _ = build_with(dg, flags, params, pts, None)
    one, _ = build_with(dg, flags, params, pts[:1], None)
    d = float(np.abs(wide - dense_bpc).max())
    print("dense (2, 300): per-cloud vs tower-wide statistics differ by %.3g" % d)
    assert d > 1e-2
    np.testing.assert_array_equal(one, one_bpc)


def test_per_cloud_inference_is_bit_reproducible(dg):
    """Default (deterministic) mode: two runs of the same packed tower under BN_PER_CLOUD give bit-identical logits."""
    rng = np.random.default_rng(37)
    flags = model_flags(dg, "residual-dgcnn", 2, BN_PER_CLOUD=True)
    off = offsets_of(TOWER_SIZES)
    pts = rng.random((int(off[-1]), 4), dtype=np.float32)
    params = random_params(flags, rng, 4)
    a, _ = build_with(dg, flags, params, pts, off)
    b, _ = build_with(dg, flags, params, pts, off)
    np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------------------------------
# 4. the inference loop
# ------------------------------------------------------------------------------------------
def test_inference_loop_packs_what_mbs_1_writes(dg, tmp_path, capsys):
    """A ragged .npz through the inference loop.  EDGE_CONV_LAYERS = 1: the only graph is on the raw coordinates, so the graphs
    are identical by construction and no near-tie can flip.  `-mbs 4 --pack_towers 1 --bn_per_cloud 1` writes softmax within 1e-3
    of `-mbs 1` for every entry; without --bn_per_cloud some entry differs by more than 1e-2."""
    from dgcnn import main_funcs as M
    rng = np.random.default_rng(4)
    counts = [300, 1400, 517, 256, 256, 777, 1100, 400]              # (every cloud >= 256 points: the source drops smaller ones)
    off = offsets_of(counts)
    pts = rng.random((off[-1], 4), dtype=np.float32)
    np.savez(tmp_path / "ragged.npz", data=pts, label=(pts[:, 0] > 0.5).astype(np.int32), data_offsets=off)
    common = dict(IO_TYPE="npz", INPUT_FILE=str(tmp_path / "ragged.npz"), NUM_POINT=-1, NUM_CHANNEL=-1, BATCH_SIZE=8, SHUFFLE=0,
                  KVALUE=8, EDGE_CONV_LAYERS=1, EDGE_CONV_FILTERS=[32], FC_LAYERS=1, FC_FILTERS=[64], NUM_CLASS=2, REPORT_STEP=0,
                  SUMMARY_STEP=0, SEED=5, ITERATION=1)
    out = {}
    for name, kw in (("mbs1", dict(MINIBATCH_SIZE=1)),
                     ("packed-bpc", dict(MINIBATCH_SIZE=4, PACK_TOWERS=True, BN_PER_CLOUD=True)),
                     ("packed", dict(MINIBATCH_SIZE=4, PACK_TOWERS=True))):
        f = dg.DGCNN_FLAGS(OUTPUT_FILE=str(tmp_path / (name + ".npz")), **common, **kw)
        M.inference(f)
        z = np.load(tmp_path / (name + ".npz"))
        assert z["idx"].tolist() == list(range(8)) and np.diff(z["data_offsets"]).tolist() == counts
        out[name] = z["softmax"]
    capsys.readouterr()
    d_bpc = np.array([np.abs(out["packed-bpc"][off[b]:off[b + 1]] - out["mbs1"][off[b]:off[b + 1]]).max() for b in range(8)])
    d_wide = np.array([np.abs(out["packed"][off[b]:off[b + 1]] - out["mbs1"][off[b]:off[b + 1]]).max() for b in range(8)])
    with capsys.disabled():
        print("inference loop: per entry max |softmax - mbs 1|: per-cloud %s, tower-wide %s" % (
            np.array2string(d_bpc, precision=2), np.array2string(d_wide, precision=2)))
    assert (d_bpc <= 1e-3).all(), d_bpc
    assert d_wide.max() > 1e-2, d_wide


# ------------------------------------------------------------------------------------------
# 5. errors, before any launch
# ------------------------------------------------------------------------------------------
def test_per_cloud_errors_before_any_launch(dg, monkeypatch):
    import dgcnn
    from dgcnn import _engine as E, _hip as H
    flags = model_flags(dg, "dgcnn", 2, BN_PER_CLOUD=True)
    tv = dg.trainval(flags).initialize()
    x = dev(np.random.default_rng(0).random((60, 4), dtype=np.float32))
    off = [0, 25, 60]
    launches = []
    orig = H.call
    monkeypatch.setattr(H, "call", lambda name, *a, **kw: (launches.append(name), orig(name, *a, **kw))[1])
    # the mode with TRAIN = True
    with pytest.raises(NotImplementedError, match="no backward"):
        dg.trainval(model_flags(dg, "dgcnn", 2, BN_PER_CLOUD=True, TRAIN=True)).initialize()
    flags.TRAIN = True
    with pytest.raises(NotImplementedError, match="no backward"):
        dgcnn.build(x, flags, offsets=off)
    with pytest.raises(NotImplementedError, match="no backward"):
        tv.accum_gradient(None, [host(x)], [np.zeros(60, np.int32)], offsets=[off])
    flags.TRAIN = False
    # the mode inside a recording
    c = dg.ctx()
    c.recording = True
    try:
        with pytest.raises(NotImplementedError, match="per-cloud BatchNorm has no backward yet"):
            dg.ops.edge_conv(x, 20, 32, True, offsets=off, bn_per_cloud=True)
        with pytest.raises(NotImplementedError, match="per-cloud BatchNorm has no backward yet"):
            dg.ops.fc(x, 1, 8, True, offsets=off, bn_per_cloud=True)
        with pytest.raises(NotImplementedError, match="no backward"):
            dgcnn.build(x, flags, offsets=off)
    finally:
        c.recording = False
    # conv0 forms the per-cloud kernels do not take
    E.EDGE_MLP_DTYPE = "bf16"
    try:
        with pytest.raises(ValueError, match="default conv0"):
            dg.ops.edge_conv(x, 20, 32, False, offsets=off, bn_per_cloud=True)
    finally:
        E.EDGE_MLP_DTYPE = "f32"
    with pytest.raises(ValueError, match="multiples of 4"):
        dg.ops.edge_conv(x, 20, 30, False, offsets=off, bn_per_cloud=True)
    # the mode without a packed tower
    for fn, args in ((dg.ops.edge_conv, (x[None], 20, 32, False)), (dg.ops.repeat_edge_conv, (x[None], 1, 20, 32, False)),
                     (dg.ops.repeat_residual_edge_conv, (x[None], 1, 20, 32, False)), (dg.ops.fc, (x[None], 1, 8, False))):
        with pytest.raises(ValueError, match="needs offsets"):
            fn(*args, bn_per_cloud=True)
    assert launches == []

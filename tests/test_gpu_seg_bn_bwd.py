"""The backward of per-cloud BatchNorm on a packed tower (run with -m gpu on an MI355X): the backward kernels of csrc/seg_bn.hip
against the float64 sums / fp32 replays of tests/bn_reference.py applied per cloud (tests/seg_bn_bwd_reference.py), then the engine
under a recording (Segments(bn_per_cloud_train=True)), trainval.accum_gradient under flags.BN_PER_CLOUD_TRAIN and the training
loop against the float64 oracle run on every cloud ALONE."""
import os

import numpy as np
import pytest
import torch

from oracle import dgcnn_oracle as O
import bn_reference as BR
import seg_bn_bwd_reference as SB
from gpu_helpers import Guard, capture_layers, dev, host, set_vars

pytestmark = pytest.mark.gpu

TOWER_SIZES = [21, 700, 64, 333]
COL_SIZES = [1, 63, 64, 65, 130, 5]        # R = 328: a one-row cloud, one ending on a chunk edge, exactly a chunk, clouds straddling chunks
NEW_ENTRIES = ("dgcnn_seg_edge_bn_act_kreduce_cnt_f32", "dgcnn_seg_bn_bwd_reduce_f32", "dgcnn_seg_edge_bn_bwd_reduce_points_f32",
               "dgcnn_seg_bn_bwd_finalize_f32", "dgcnn_seg_bn_bwd_apply_f32", "dgcnn_seg_edge_bn_bwd_apply_f32")


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


def within(got, cases, what):
    """got (nseg, 2, F) against every cloud's float64 sums: sum_bound(n_terms, sum |term|).  -> worst err / bound."""
    worst = 0.0
    for b, (_, _, s) in enumerate(cases):
        err, bound = np.abs(got[b] - s.red), BR.sum_bound(s.n_terms, s.scale)
        ratio = float((err / np.maximum(bound, 1e-300))[bound > 0].max(initial=0.0))
        assert (err <= bound).all(), "%s cloud %d: worst err / bound %.3g" % (what, b, ratio)
        worst = max(worst, ratio)
    return worst


def fro(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-9))


# ------------------------------------------------------------------------------------------
# 1. the k = 1 kernels: reduce (b), finalize (d), apply (e)
# ------------------------------------------------------------------------------------------
def k1_inputs(rng, sizes, F, relu, second, exact):
    off = offsets_of(sizes)
    R, nseg = int(off[-1]), len(sizes)
    if exact:
        par = [BR.lattice_params(rng, F) for _ in sizes]
        mu, rs, be = np.stack([p[0] for p in par]), np.stack([p[1] for p in par]), par[0][2]
        T = np.concatenate([BR.lattice_dense(rng, n, 1, F, relu)[:, 0] for n in sizes])
        d1 = BR.lattice_grads(rng, R, 1, F, with_mean=False)[0]
        d2 = BR.lattice_grads(rng, R, 1, F, with_mean=False)[0] if second else None
    else:
        T = np.concatenate([rng.normal(0.3 * b, 1.0 + 0.5 * b, (n, F)) for b, n in enumerate(sizes)]).astype(np.float32)
        mu, rs = SB.tables32(T, off)
        be = rng.normal(0, 0.3, F).astype(np.float32)
        d1 = rng.normal(size=(R, F)).astype(np.float32)
        d2 = rng.normal(size=(R, F)).astype(np.float32) if second else None
    dsum = d1 if d2 is None else (d1 + d2).astype(np.float32)            # the kernels' single fp32 add
    return off, R, nseg, T, mu, rs, be, d1, d2, dsum


@pytest.mark.parametrize("kind", ["lattice", "random"])
@pytest.mark.parametrize("second", [0, 1], ids=["d", "d+d2"])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("F,pad", [(2, 0), (3, 4), (64, 0), (64, 4), (260, 0), (260, 4), (3, 0), (2, 4)])
def test_k1_reduce_finalize_apply(dg, F, pad, relu, second, kind):
    """Both towers.  Reduce: per cloud within sum_bound of the float64 sums on float32 decisions (lattice inputs: EQUAL), two calls
    bit-identical.  Finalize from the float64 sums: c1, c2, dbeta (dbeta_beta = 1 on a prior value) bit-exact.  Apply: bit-exact
    against apply32 per cloud with n = n_b; in place == out of place; padding untouched; a one-row cloud gives dT == 0."""
    from dgcnn import _hip as H
    exact = kind == "lattice"
    for sizes in (TOWER_SIZES, COL_SIZES):
        rng = np.random.default_rng(1000 * F + 100 * pad + 10 * relu + second + len(sizes))
        off, R, nseg, T, mu, rs, be, d1, d2, dsum = k1_inputs(rng, sizes, F, relu, second, exact)
        cases = SB.k1_clouds(T, off, mu, rs, be, relu, dsum)
        g = Guard()
        ld = F + pad
        _, Tv = padded(g, T, pad)
        _, d1v = padded(g, d1, pad)
        d2v = padded(g, d2, pad)[1] if second else None
        mud, rsd, bed = g.put(mu), g.put(rs), g.put(be)
        offd, rgd = g.put(off.astype(np.int32)), g.put(row_group_of(sizes))
        par = (mud.data_ptr(), rsd.data_ptr(), bed.data_ptr(), relu, d1v.data_ptr(), ld, 0 if d2v is None else d2v.data_ptr(),
               ld if second else 0)
        # ---- reduce
        outs = []
        for _ in range(2):
            red = g.new((nseg, 2, F), torch.float64)                          # written, not accumulated: starts as the sentinel
            ws, nb = ws_of(H, g, R, nseg, F)
            H.call("dgcnn_seg_bn_bwd_reduce_f32", Tv.data_ptr(), ld, R, F, offd.data_ptr(), nseg, *par, red.data_ptr(), ws.data_ptr(), nb)
            outs.append(red)
        g.check()
        assert torch.equal(outs[0], outs[1]), "two runs of the fixed-order sums differ"
        got = host(outs[0])
        ref = np.stack([s.red for _, _, s in cases])
        if exact:
            for lo_hi, (fw, _, s) in zip(SB.clouds(off), cases):
                BR.lattice_precondition(fw, dsum[lo_hi[1]:lo_hi[2]], None)
            np.testing.assert_array_equal(got, ref)
        else:
            print("k1 reduce %s F=%d pad=%d relu=%d second=%d: worst err / bound %.3g" % (sizes, F, pad, relu, second, within(got, cases, "k1")))
        # ---- finalize from the float64 sums
        prior = np.arange(F, dtype=np.float32)
        redd = g.put(ref)
        for bb in (0.0, 1.0):
            c1, c2, db = g.new((nseg, F)), g.new((nseg, F)), g.put(prior)
            H.call("dgcnn_seg_bn_bwd_finalize_f32", redd.data_ptr(), nseg, F, offd.data_ptr(), 1, c1.data_ptr(), c2.data_ptr(), db.data_ptr(), bb)
            e1, e2, edb = SB.finalize32(ref, sizes, 1, prior, bb)
            np.testing.assert_array_equal(host(c1), e1)
            np.testing.assert_array_equal(host(c2), e2)
            np.testing.assert_array_equal(host(db), edb)
        # ---- apply: out of place, then in place of T
        eo, _ = SB.apply32(cases, ref, 1)
        ob, ov = padded(g, np.zeros((R, F), np.float32), pad)
        H.call("dgcnn_seg_bn_bwd_apply_f32", Tv.data_ptr(), ld, R, F, rgd.data_ptr(), *par, c1.data_ptr(), c2.data_ptr(), ov.data_ptr(), ld)
        np.testing.assert_array_equal(host(ob)[:, :F], eo[:, 0])
        H.call("dgcnn_seg_bn_bwd_apply_f32", Tv.data_ptr(), ld, R, F, rgd.data_ptr(), *par, c1.data_ptr(), c2.data_ptr(), Tv.data_ptr(), ld)
        g.check()
        assert torch.equal(Tv, ov), "the in-place apply differs from the out-of-place one"
        if pad:
            assert (host(ob)[:, F:] == 777.0).all(), "the padding columns were written"
        if sizes[0] == 1 and not exact:                                         # (tables from the cloud's own row: xhat = 0, c1 = dz)
            assert (host(ob)[0, :F] == 0).all(), "a one-row cloud must give dT == 0"


# ------------------------------------------------------------------------------------------
# 2. the edge kernels: forward with counts (a), closed-form reduce (c), finalize (d), apply (f)
# ------------------------------------------------------------------------------------------
def edge_inputs(rng, sizes, k, F, relu, exact):
    """[U | V] halves of one (R, 2F) buffer, idx = tower rows inside the row's own cloud with self, repeats (exact ties) and, under
    ReLU, all-dead points; the lattice form plants 1 / 2 / 4 ties (BR.lattice_edge, cloud by cloud)."""
    off = offsets_of(sizes)
    R = int(off[-1])
    if exact:
        par = [BR.lattice_params(rng, F) for _ in sizes]
        mu, rs, be = np.stack([p[0] for p in par]), np.stack([p[1] for p in par]), par[0][2]
        parts = [BR.lattice_edge(rng, 1, n, k, F, relu) for n in sizes]
        V, U = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        idx = np.concatenate([p[2][0] + off[b] for b, p in enumerate(parts)]).astype(np.int32)
        dmax, dmean = BR.lattice_grads(rng, R, k, F)
    else:
        V = np.concatenate([rng.normal(0.2 * b, 1.0 + 0.3 * b, (n, F)) for b, n in enumerate(sizes)]).astype(np.float32)
        U = rng.normal(0.1, 1.0, (R, F)).astype(np.float32)
        idx = np.concatenate([rng.integers(off[b], off[b + 1], (sizes[b], k)) for b in range(len(sizes))]).astype(np.int32)
        idx[::3, 0] = np.arange(R, dtype=np.int32)[::3]                          # self
        idx[1::4, 1] = idx[1::4, 0]                                              # repeats: exact ties
        if relu:
            for b in range(len(sizes)):
                U[off[b + 1] - max(1, sizes[b] // 10):off[b + 1]] -= 50          # all-dead points
        dmax, dmean = rng.normal(size=(R, F)).astype(np.float32), rng.normal(size=(R, F)).astype(np.float32)
    UV = np.ascontiguousarray(np.concatenate([U, V], 1))
    y = BR.edge_rows32(V, U, idx.reshape(1, R, k), 1, R)                        # (R, k, F), the single fp32 add
    if not exact:
        mu, rs = SB.tables32(y, off)
        be = rng.normal(0, 0.3, F).astype(np.float32)
    return off, R, UV, idx, y, mu, rs, be, dmax, dmean


def edge_head(UVd, idxd, R, k, F):
    return (UVd[:, F:].data_ptr(), 2 * F, UVd.data_ptr(), 2 * F, idxd.data_ptr(), R, k, F)


def run_edge_passes(H, sizes, k, F, relu, exact, seed):
    rng = np.random.default_rng(seed)
    if exact:
        k = BR.nearest_pow2(k)
    off, R, UV, idx, y, mu, rs, be, dmax, dmean = edge_inputs(rng, sizes, k, F, relu, exact)
    nseg = len(sizes)
    cases = SB.edge_clouds(y, off, mu, rs, be, relu, dmax, dmean)
    g = Guard()
    UVd, idxd, offd, rgd = g.put(UV), g.put(idx), g.put(off.astype(np.int32)), g.put(row_group_of(sizes))
    mud, rsd, bed = g.put(mu), g.put(rs), g.put(be)
    head = edge_head(UVd, idxd, R, k, F)
    tab = (rgd.data_ptr(), mud.data_ptr(), rsd.data_ptr(), bed.data_ptr(), relu)
    # ---- (a) forward with counts against the existing entry and the decisions
    mm, mm0 = g.new((R, 2 * F + 4)), g.new((R, 2 * F + 4))
    cnt = g.new((R, F))
    H.call("dgcnn_seg_edge_bn_act_kreduce_cnt_f32", *head, *tab, mm[:, :F].data_ptr(), 2 * F + 4, mm[:, F:2 * F].data_ptr(), 2 * F + 4,
           cnt.data_ptr())
    H.call("dgcnn_seg_edge_bn_act_kreduce_f32", *head, *tab, mm0[:, :F].data_ptr(), 2 * F + 4, mm0[:, F:2 * F].data_ptr(), 2 * F + 4)
    g.check()
    assert torch.equal(mm, mm0), "max / mean of the counting entry differ from the existing entry"
    fmx = np.concatenate([fw.mx for fw, _, _ in cases])
    fmn = np.concatenate([fw.mean32 for fw, _, _ in cases])
    fpk = np.concatenate([fw.packed for fw, _, _ in cases])
    np.testing.assert_array_equal(host(mm)[:, :F], fmx)
    np.testing.assert_array_equal(host(mm)[:, F:2 * F], fmn)
    np.testing.assert_array_equal(host(cnt), fpk)
    assert (host(mm)[:, 2 * F:] == 777.0).all()
    ref = np.stack([s.red for _, _, s in cases])
    dmxd, dmnd = g.put(dmax), g.put(dmean)
    # ---- (c) the closed form (a ReLU layer by definition)
    if relu:
        outs = []
        for _ in range(2):
            red = g.new((nseg, 2, F), torch.float64)
            ws, nb = ws_of(H, g, R, nseg, F)
            H.call("dgcnn_seg_edge_bn_bwd_reduce_points_f32", mm[:, :F].data_ptr(), 2 * F + 4, mm[:, F:2 * F].data_ptr(), 2 * F + 4,
                   cnt.data_ptr(), dmxd.data_ptr(), F, dmnd.data_ptr(), F, bed.data_ptr(), R, k, F, offd.data_ptr(), nseg, red.data_ptr(),
                   ws.data_ptr(), nb)
            outs.append(red)
        g.check()
        assert torch.equal(outs[0], outs[1]), "two runs of the fixed-order sums differ"
        got = host(outs[0])
        if exact:
            for (_, lo, hi), (fw, _, _) in zip(SB.clouds(off), cases):
                BR.lattice_precondition(fw, dmax[lo:hi], dmean[lo:hi])
            np.testing.assert_array_equal(got, ref)
        else:
            w_pt = w_edge = 0.0
            for (b, lo, hi), (fw, _, s) in zip(SB.clouds(off), cases):
                t0, t1 = SB.point_terms64(fw.mx, fw.mean32, fw.npos, dmax[lo:hi], dmean[lo:hi], be, k)
                closed = np.stack([t0.sum(0), t1.sum(0)])
                bound = BR.sum_bound(hi - lo, np.stack([np.abs(t0).sum(0), np.abs(t1).sum(0)]))
                err = np.abs(got[b] - closed)
                assert (err <= bound).all(), "closed form, cloud %d: worst err / bound %.3g" % (b, float((err / np.maximum(bound, 1e-300)).max()))
                w_pt = max(w_pt, float((err / np.maximum(bound, 1e-300))[bound > 0].max(initial=0.0)))
            w_edge = within(got, cases, "closed form against the explicit edge sums")
            print("edge reduce_points k=%d F=%d: worst err / bound %.3g (per-point terms) %.3g (edge sums)" % (k, F, w_pt, w_edge))
    # ---- (d) finalize from the float64 edge sums, count n_b k
    prior = np.arange(F, dtype=np.float32)
    redd = g.put(ref)
    c1, c2, db = g.new((nseg, F)), g.new((nseg, F)), g.put(prior)
    H.call("dgcnn_seg_bn_bwd_finalize_f32", redd.data_ptr(), nseg, F, offd.data_ptr(), k, c1.data_ptr(), c2.data_ptr(), db.data_ptr(), 1.0)
    e1, e2, edb = SB.finalize32(ref, sizes, k, prior, 1.0)
    np.testing.assert_array_equal(host(c1), e1)
    np.testing.assert_array_equal(host(c2), e2)
    np.testing.assert_array_equal(host(db), edb)
    # ---- (f) apply
    dY, dsb = g.new((R * k, F)), g.new((R, 2 * F))                              # dYsum = the dU half of [dU | dV]
    H.call("dgcnn_seg_edge_bn_bwd_apply_f32", *head, *tab, dmxd.data_ptr(), F, dmnd.data_ptr(), F, mm[:, :F].data_ptr(), 2 * F + 4,
           cnt.data_ptr(), c1.data_ptr(), c2.data_ptr(), dY.data_ptr(), dsb.data_ptr(), 2 * F)
    g.check()
    eo, eacc = SB.apply32(cases, ref, k)
    np.testing.assert_array_equal(host(dY).reshape(R, k, F), eo)
    np.testing.assert_array_equal(host(dsb)[:, :F], eacc)
    assert (host(dsb)[:, F:] == 777.0).all()
    if relu:
        dead = np.concatenate([(fw.mx <= 0) for fw, _, _ in cases])             # all-dead (point, channel): every dz is zeroed
        assert dead.any(), "the case has no all-dead point"
    return cases


@pytest.mark.parametrize("kind", ["lattice", "random"])
@pytest.mark.parametrize("F", [4, 64, 128])
@pytest.mark.parametrize("k", [4, 5, 20, 40])
def test_edge_forward_counts_reduce_finalize_apply(dg, k, F, kind):
    """(a) max / mean bit-identical to the existing entry, cnt == Fwd.packed per cloud; (c) two calls bit-identical, within
    sum_bound of the float64 closed form AND of the explicit edge sums (lattice: EQUAL to them); (d) bit-exact; (f) dY / dYsum
    bit-exact against apply32 per cloud with n = n_b k.  The smallest cloud holds >= k points."""
    from dgcnn import _hip as H
    sizes = [max(21, k)] + TOWER_SIZES[1:]
    run_edge_passes(H, sizes, k, F, 1, kind == "lattice", 1000 * k + F + (kind == "lattice"))


@pytest.mark.parametrize("kind", ["lattice", "random"])
def test_edge_apply_without_relu(dg, kind):
    from dgcnn import _hip as H
    run_edge_passes(H, [9, 130, 64, 5], 5, 64, 0, kind == "lattice", 77)


# ------------------------------------------------------------------------------------------
# 3. a one-cloud tower is the dense kernels
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [64, 3])
def test_one_cloud_k1_apply_is_the_dense_kernel(dg, F):
    from dgcnn import _hip as H
    rng = np.random.default_rng(F)
    R, relu = 333, 1
    off, _, _, T, mu, rs, be, d1, d2, dsum = k1_inputs(rng, [R], F, relu, True, False)
    s = SB.k1_clouds(T, off, mu, rs, be, relu, dsum)[0][2]
    g = Guard()
    Td, d1d, d2d = g.put(T), g.put(d1), g.put(d2)
    mud, rsd, bed = g.put(mu[0]), g.put(rs[0]), g.put(be)
    dense_red = g.zeros((H.stat_slots(), 2, F), torch.float64)
    dense_red[0].copy_(torch.from_numpy(s.red))                                 # the totals in slot 0, zeros elsewhere
    dd, dbd = g.new((R, F)), g.zeros((F,))
    H.call("dgcnn_bn_bwd_apply_f32", Td.data_ptr(), R, 1, F, mud.data_ptr(), rsd.data_ptr(), bed.data_ptr(), relu, d1d.data_ptr(), F,
           d2d.data_ptr(), F, 0, 0, 0, dense_red.data_ptr(), dd.data_ptr(), 0, 0, dbd.data_ptr(), 0.0)
    c1, c2, dbs = g.new((1, F)), g.new((1, F)), g.zeros((F,))
    offd = g.put(np.array([0, R], np.int32))
    H.call("dgcnn_seg_bn_bwd_finalize_f32", g.put(s.red[None]).data_ptr(), 1, F, offd.data_ptr(), 1, c1.data_ptr(), c2.data_ptr(),
           dbs.data_ptr(), 0.0)
    ds = g.new((R, F))
    H.call("dgcnn_seg_bn_bwd_apply_f32", Td.data_ptr(), F, R, F, g.put(np.zeros(R, np.int32)).data_ptr(), mud.data_ptr(), rsd.data_ptr(),
           bed.data_ptr(), relu, d1d.data_ptr(), F, d2d.data_ptr(), F, c1.data_ptr(), c2.data_ptr(), ds.data_ptr(), F)
    g.check()
    assert torch.equal(dd, ds) and torch.equal(dbd, dbs)


def test_one_cloud_edge_apply_is_the_dense_kernel(dg):
    from dgcnn import _hip as H
    rng = np.random.default_rng(9)
    k, F, R = 20, 32, 150
    off, _, UV, idx, y, mu, rs, be, dmax, dmean = edge_inputs(rng, [R], k, F, 1, False)
    fw, _, s = SB.edge_clouds(y, off, mu, rs, be, 1, dmax, dmean)[0]
    g = Guard()
    UVd, idxd = g.put(UV), g.put(idx)
    mud, rsd, bed = g.put(mu[0]), g.put(rs[0]), g.put(be)
    mxd, cnd, dmxd, dmnd = g.put(fw.mx), g.put(fw.packed), g.put(dmax), g.put(dmean)
    dense_red = g.zeros((H.stat_slots(), 2, F), torch.float64)
    dense_red[0].copy_(torch.from_numpy(s.red))
    dYd, dsd, dbd = g.new((R * k, F)), g.new((R, F)), g.zeros((F,))
    H.call("dgcnn_edge_bn_bwd_apply_f32", UVd[:, F:].data_ptr(), 2 * F, UVd.data_ptr(), 2 * F, idxd.data_ptr(), 1, R, k, F, mud.data_ptr(),
           rsd.data_ptr(), bed.data_ptr(), 1, dmxd.data_ptr(), F, dmnd.data_ptr(), F, mxd.data_ptr(), F, cnd.data_ptr(),
           dense_red.data_ptr(), dYd.data_ptr(), dsd.data_ptr(), F, dbd.data_ptr(), 0.0)
    c1, c2, dbs = g.new((1, F)), g.new((1, F)), g.zeros((F,))
    H.call("dgcnn_seg_bn_bwd_finalize_f32", g.put(s.red[None]).data_ptr(), 1, F, g.put(np.array([0, R], np.int32)).data_ptr(), k,
           c1.data_ptr(), c2.data_ptr(), dbs.data_ptr(), 0.0)
    dYs, dss = g.new((R * k, F)), g.new((R, F))
    H.call("dgcnn_seg_edge_bn_bwd_apply_f32", *edge_head(UVd, idxd, R, k, F), g.put(np.zeros(R, np.int32)).data_ptr(), mud.data_ptr(),
           rsd.data_ptr(), bed.data_ptr(), 1, dmxd.data_ptr(), F, dmnd.data_ptr(), F, mxd.data_ptr(), F, cnd.data_ptr(), c1.data_ptr(),
           c2.data_ptr(), dYs.data_ptr(), dss.data_ptr(), F)
    g.check()
    assert torch.equal(dYd, dYs) and torch.equal(dsd, dss) and torch.equal(dbd, dbs)


# ------------------------------------------------------------------------------------------
# 4. refusals: the code, and nothing written
# ------------------------------------------------------------------------------------------
def test_backward_refusals_write_nothing(dg):
    from dgcnn import _hip as H
    rng = np.random.default_rng(1)
    k, F, sizes = 5, 8, [30, 40]
    off, R, UV, idx, _, _, _, _, _, _ = edge_inputs(rng, sizes, k, F, 1, False)
    g = Guard()
    UVd, idxd, offd, rgd = g.put(UV), g.put(idx), g.put(off.astype(np.int32)), g.put(row_group_of(sizes))
    head = edge_head(UVd, idxd, R, k, F)
    x = g.put(rng.normal(size=(R, 2 * F)).astype(np.float32))                  # any (R, F) operand, leading dimension 2F
    tab = g.put(np.ones((2, F), np.float32))
    red = g.new((2, 2, F), torch.float64)
    ws, nb = ws_of(H, g, R, 2, F)
    out, out2, dY, cnt = g.new((R, 2 * F)), g.new((R, 2 * F)), g.new((R * k, F)), g.new((R, F))
    t, xp, xq = tab.data_ptr(), x.data_ptr(), x[:, F:].data_ptr()
    k1 = lambda **kw: H.call("dgcnn_seg_bn_bwd_reduce_f32", kw.get("T", xp), 2 * F, R, F, offd.data_ptr(), 2, t, t, t, kw.get("relu", 1),
                             xq, 2 * F, None, 0, red.data_ptr(), ws.data_ptr(), kw.get("nb", nb))
    pts = lambda **kw: H.call("dgcnn_seg_edge_bn_bwd_reduce_points_f32", kw.get("mx", xp), 2 * F, xq, 2 * F, cnt.data_ptr(), xp, 2 * F, xq,
                              2 * F, t, R, k, kw.get("F", F), offd.data_ptr(), 2, red.data_ptr(), ws.data_ptr(), kw.get("nb", nb))
    app = lambda **kw: H.call("dgcnn_seg_bn_bwd_apply_f32", xp, 2 * F, R, F, kw.get("rg", rgd.data_ptr()), t, t, t, kw.get("relu", 1), xq,
                              2 * F, None, 0, t, t, out.data_ptr(), 2 * F)
    fwd = lambda **kw: H.call("dgcnn_seg_edge_bn_act_kreduce_cnt_f32", *head[:7], kw.get("F", F), rgd.data_ptr(), t, t, t, kw.get("relu", 1),
                              kw.get("mx", out.data_ptr()), 2 * F, out2.data_ptr(), 2 * F, kw.get("cnt", cnt.data_ptr()))
    eap = lambda **kw: H.call("dgcnn_seg_edge_bn_bwd_apply_f32", *head[:7], kw.get("F", F), rgd.data_ptr(), t, t, t, kw.get("relu", 1), xp,
                              2 * F, xq, 2 * F, kw.get("mx", xp), 2 * F, cnt.data_ptr(), t, kw.get("c2", t), dY.data_ptr(), out.data_ptr(),
                              2 * F)
    for bad in (lambda: k1(T=None), lambda: k1(relu=2), lambda: pts(mx=None), lambda: pts(mx=xp + 4), lambda: app(rg=None),
                lambda: app(relu=-1), lambda: fwd(cnt=None), lambda: fwd(relu=2), lambda: fwd(mx=out.data_ptr() + 4), lambda: eap(c2=None),
                lambda: eap(relu=2), lambda: eap(mx=xp + 4),
                lambda: H.call("dgcnn_seg_bn_bwd_finalize_f32", None, 2, F, offd.data_ptr(), k, t, t, t, 1.0)):
        with pytest.raises(ValueError):                                          # DGCNN_EINVAL: null, misaligned, relu outside {0, 1}
            bad()
    for bad in (lambda: k1(nb=nb - 8), lambda: pts(nb=nb - 8)):
        with pytest.raises(H.HipError, match="workspace too small"):            # DGCNN_ENOSPC
            bad()
    for bad in (lambda: pts(F=6), lambda: fwd(F=6), lambda: eap(F=6)):
        with pytest.raises(H.HipError, match="multiple of 4"):                  # DGCNN_EUNSUP
            bad()
    g.check()
    for buf in (red, ws, out, out2, dY, cnt):
        assert (host(buf) == 777.0).all(), "a refused call wrote to an output"
    assert (host(tab) == 1.0).all()


# ------------------------------------------------------------------------------------------
# 5. engine: the EdgeConv stacks under a recording
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
def test_recorded_stack_per_cloud_against_the_float64_oracle(dg, residual):
    """repeat_(residual_)edge_conv(bn_per_cloud_train=True) under a recording on four unequal clouds, C = 4, k = 20, 32 -> 64
    filters (the shortcut conv runs): graphs per cloud bit for bit; every parameter gradient and d(points) within 5e-3 relative
    Frobenius of the float64 oracle run on each cloud alone with those graphs and the same upstream gradients."""
    from dgcnn import _engine as E
    rng = np.random.default_rng(41 + residual)
    C, k, fl = 4, 20, [32, 64]
    off = offsets_of(TOWER_SIZES)
    R = int(off[-1])
    pts = rng.random((R, C), dtype=np.float32)
    P = stack_params(rng, C, fl)
    c = dg.ctx()
    c.begin_step()
    c.recording = True
    try:
        for n, v in P.items():
            c.get_variable(n, v.shape)
        set_vars(dg, P)
        x = c.new_buffer(R, C)                                                  # tracked, so that d(points) is produced
        x.copy_(dev(pts))
        fn = dg.ops.repeat_residual_edge_conv if residual else dg.ops.repeat_edge_conv
        with capture_layers() as cap:
            tensors = fn(x, 2, k, fl, True, offsets=off, bn_per_cloud_train=True)
        graphs = graphs_of(cap, 2, off, k)
        d = [rng.normal(size=(1, R, 1, t.shape[-1])) for t in tensors]
        for t, gr in zip(tensors, d):
            v, _, _ = E.as2d(t)
            c.grad(v).copy_(dev(gr.reshape(R, -1).astype(np.float32)))
        c.backward()
        dx = host(c.grad(x)).astype(np.float64)
    finally:
        c.recording = False
    p64 = {n: v.astype(np.float64) for n, v in P.items()}
    ref_t, ref_dx, G = SB.oracle_stack(pts.astype(np.float64), off, 2, k, fl, p64, residual, graphs, d)
    for j, (a, b) in enumerate(zip(tensors, ref_t)):
        np.testing.assert_allclose(host(a), b, rtol=1e-4, atol=1e-4, err_msg="tensor %d" % j)
    worst = (fro(dx, ref_dx), "d(points)")
    assert set(G) == set(n for n in P if residual or "shortcut" not in n)      # (the plain stack has no shortcut conv)
    for n in G:
        worst = max(worst, (fro(host(c.var_grads[n]).astype(np.float64), G[n]), n))
    print("recorded per-cloud %s stack: worst relative Frobenius gradient error %.3g (%s)" % ("residual" if residual else "plain", *worst))
    assert worst[0] <= 5e-3, worst


# ------------------------------------------------------------------------------------------
# 6. trainval.accum_gradient under BN_PER_CLOUD_TRAIN
# ------------------------------------------------------------------------------------------
MODELS = [("dgcnn", 2), ("dgcnn", 0), ("residual-dgcnn", 2), ("residual-dgcnn", 0), ("residual-dgcnn-nofc", 2)]


def model_flags(dg, model, fcl, det=True, **kw):
    base = dict(MODEL_NAME=model, EDGE_CONV_LAYERS=2, EDGE_CONV_FILTERS=[32, 64], KVALUE=20, NUM_CLASS=3, FC_LAYERS=fcl,
                FC_FILTERS=[64, 32][:fcl] if fcl else 64, TRAIN=True, NUM_CHANNEL=4, DETERMINISTIC=None if det else False,
                BN_PER_CLOUD_TRAIN=True)
    base.update(kw)
    return dg.DGCNN_FLAGS(**base)


def make_tower(rng, sizes, C, ncls):
    pts = np.concatenate([rng.random((n, C), dtype=np.float32) for n in sizes])
    return pts, offsets_of(sizes), rng.integers(0, ncls, len(pts)).astype(np.int32), (rng.random(len(pts), dtype=np.float32) + 0.5)


def random_params(flags, rng, C):
    params = O.init_params(flags, C, seed=1)
    for n in params:
        if n.endswith("beta"):
            params[n] = rng.normal(0, 0.2, params[n].shape).astype(np.float32)
    return params


class no_dropout(object):
    def __enter__(self):
        from dgcnn import _engine as E
        self.E, self.keep = E, E.DROPOUT_KEEP
        E.DROPOUT_KEEP = 1.0

    def __exit__(self, *exc):
        self.E.DROPOUT_KEEP = self.keep
        return False


@pytest.mark.parametrize("det", [True, False], ids=["default", "atomics"])
@pytest.mark.parametrize("model,fcl", MODELS, ids=["%s-fc%d" % m for m in MODELS])
def test_accum_gradient_per_cloud(dg, model, fcl, det):
    """Four unequal clouds with row weights, dropout off: loss within 1e-3 and every gradient tensor within 5e-3 (default mode) /
    2e-2 (DETERMINISTIC=False) relative Frobenius of sum_b (n_b / R) oracle.train_step_grads(cloud b, weight_b) in float64, fed
    the captured graphs."""
    from dgcnn import _engine as E
    rng = np.random.default_rng(17)
    flags = model_flags(dg, model, fcl, det)
    pts, off, lab, wgt = make_tower(rng, TOWER_SIZES, 4, 3)
    params = random_params(flags, rng, 4)
    with no_dropout():
        tv = dg.trainval(flags).initialize()
        set_vars(dg, params)
        assert E.DETERMINISTIC == det
        tv.zero_gradients(None)
        with capture_layers() as cap:
            res = tv.accum_gradient(None, [pts], [lab], [wgt], offsets=[off])
    graphs = graphs_of(cap, 2, off, 20)
    G, loss64 = SB.train_step_grads(pts, lab, off, flags, params, graphs, wgt)
    print("%s fc%d %s: loss %.7g reference %.7g" % (model, fcl, "det" if det else "atomics", float(res[2]), loss64))
    worst = (0.0, "")
    for n in params:
        worst = max(worst, (fro(host(tv.gradients[n]).astype(np.float64), G[n]), n))
    print("%s fc%d %s: worst relative Frobenius gradient error %.3g (%s)" % (model, fcl, "det" if det else "atomics", worst[0], worst[1]))
    assert abs(float(res[2]) - loss64) < 1e-3
    assert worst[0] <= (5e-3 if det else 2e-2), worst


def test_per_cloud_training_steps_are_bit_reproducible(dg):
    """Default (deterministic) mode: two zero_gradients -> accum_gradient -> apply_gradient steps from the same seed, done twice,
    leave bit-identical parameters (dropout on: the mask stream restarts with the instance)."""
    rng = np.random.default_rng(3)
    flags = model_flags(dg, "residual-dgcnn", 2)
    pts, off, lab, wgt = make_tower(rng, TOWER_SIZES, 4, 3)
    finals = []
    for _ in range(2):
        tv = dg.trainval(flags).initialize()
        for _ in range(2):
            tv.zero_gradients(None)
            res = tv.accum_gradient(None, [pts], [lab], [wgt], offsets=[off])
            tv.apply_gradient(None)
        assert np.isfinite(float(res[2]))
        finals.append(tv._ctx.flat_param.clone())
    assert torch.equal(finals[0], finals[1]), int((finals[0] != finals[1]).sum())


def test_dense_input_under_the_flag_is_the_packed_tower(dg):
    """A dense (3, 64, C) input under BN_PER_CLOUD_TRAIN = the packed tower with offsets b * 64: loss and gradients bit for bit;
    B = 1 keeps the dense path."""
    rng = np.random.default_rng(31)
    flags = model_flags(dg, "dgcnn", 2)
    pts = rng.random((3, 64, 4), dtype=np.float32)
    lab = rng.integers(0, 3, (3, 64)).astype(np.int32)
    params = random_params(flags, rng, 4)
    grads, losses = [], []
    with no_dropout():
        for data, label, kw in ((pts, lab, {}), (pts.reshape(192, 4), lab.reshape(192), {"offsets": [np.arange(4) * 64]})):
            tv = dg.trainval(flags).initialize()
            set_vars(dg, params)
            tv.zero_gradients(None)
            res = tv.accum_gradient(None, [data], [label], **kw)
            grads.append(tv._ctx.flat_grad.clone())
            losses.append(float(res[2]))
        assert torch.equal(grads[0], grads[1]), int((grads[0] != grads[1]).sum())
        assert losses[0] == losses[1]
        # B = 1: the dense kernels, with and without the flag
        one = []
        for bpct in (True, False):
            f1 = model_flags(dg, "dgcnn", 2, BN_PER_CLOUD_TRAIN=bpct)
            tv = dg.trainval(f1).initialize()
            set_vars(dg, params)
            tv.zero_gradients(None)
            tv.accum_gradient(None, [pts[:1]], [lab[:1]])
            one.append(tv._ctx.flat_grad.clone())
        assert torch.equal(one[0], one[1])


def test_switch_off_launches_no_new_entry(dg, monkeypatch):
    """A tower-wide packed training step (the switch off) calls none of the new entries; with the switch on it calls all of them."""
    from dgcnn import _hip as H
    rng = np.random.default_rng(5)
    pts, off, lab, wgt = make_tower(rng, TOWER_SIZES, 4, 3)
    seen = {}
    orig = H.call
    for on in (False, True):
        names = seen[on] = set()
        monkeypatch.setattr(H, "call", lambda name, *a, _n=names, **kw: (_n.add(name), orig(name, *a, **kw))[1])
        tv = dg.trainval(model_flags(dg, "residual-dgcnn", 2, BN_PER_CLOUD_TRAIN=on)).initialize()
        tv.zero_gradients(None)
        tv.accum_gradient(None, [pts], [lab], [wgt], offsets=[off])
        monkeypatch.setattr(H, "call", orig)
    assert not (seen[False] & set(NEW_ENTRIES)), seen[False] & set(NEW_ENTRIES)
    assert not [n for n in seen[False] if n.startswith("dgcnn_seg_bn") or n.startswith("dgcnn_seg_edge") or n == "dgcnn_seg_colstats_f32"]
    assert set(NEW_ENTRIES) <= seen[True], set(NEW_ENTRIES) - seen[True]


def test_validation_inside_a_training_run_matches(dg):
    """Under the flag inference() of a TRAIN=True instance uses per-cloud BatchNorm as well: a cloud's softmax does not depend on
    its companions (the tower of four against the same cloud in a tower of two, identical first-layer graphs; EDGE_CONV_LAYERS = 1)."""
    rng = np.random.default_rng(8)
    flags = model_flags(dg, "dgcnn", 1, EDGE_CONV_LAYERS=1, EDGE_CONV_FILTERS=[32], FC_FILTERS=[64])
    pts, off, lab, _ = make_tower(rng, TOWER_SIZES, 4, 3)
    with no_dropout():
        tv = dg.trainval(flags).initialize()
        a = host(tv.inference(None, [pts], offsets=[off])[0])
        lo, hi = int(off[1]), int(off[3])
        b = host(tv.inference(None, [pts[lo:hi]], offsets=[off[1:4] - lo])[0])
    d = float(np.abs(a[0, lo:hi] - b[0]).max())
    print("validation under the flag: max |softmax(tower of 4) - softmax(tower of 2)| on the shared clouds %.3g" % d)
    assert d <= 1e-3


# ------------------------------------------------------------------------------------------
# 7. the training loop
# ------------------------------------------------------------------------------------------
def test_training_loop_per_cloud_then_inference(dg, tmp_path, capsys):
    """A ragged .npz (8 clouds of 256 ... 1400 points): `train --pack_towers 1 --bn_per_cloud_train 1 -mbs 4` for three iterations
    ends with a finite loss and a checkpoint; `inference --bn_per_cloud 1` from that checkpoint writes softmax rows that sum to 1."""
    from dgcnn import main_funcs as M
    rng = np.random.default_rng(4)
    counts = [300, 1400, 517, 256, 256, 777, 1100, 400]
    off = offsets_of(counts)
    pts = rng.random((off[-1], 4), dtype=np.float32)
    np.savez(tmp_path / "ragged.npz", data=pts, label=(pts[:, 0] > 0.5).astype(np.int32), data_offsets=off)
    common = dict(IO_TYPE="npz", INPUT_FILE=str(tmp_path / "ragged.npz"), NUM_POINT=-1, NUM_CHANNEL=-1, BATCH_SIZE=8, MINIBATCH_SIZE=4,
                  PACK_TOWERS=True, SHUFFLE=0, KVALUE=8, EDGE_CONV_LAYERS=2, EDGE_CONV_FILTERS=[32, 64], FC_LAYERS=1, FC_FILTERS=[64],
                  NUM_CLASS=2, REPORT_STEP=0, SUMMARY_STEP=0, SEED=5, WEIGHT_PREFIX=str(tmp_path / "w" / "snap"))
    f = dg.DGCNN_FLAGS(ITERATION=3, CHECKPOINT_STEP=3, LOG_DIR=str(tmp_path / "log"), BN_PER_CLOUD_TRAIN=True, **common)
    M.train(f)
    rows = open(tmp_path / "log" / "train_log-0000000.csv").read().strip().split("\n")[1:]
    assert len(rows) == 3 and all(np.isfinite(float(r.split(",")[-2])) for r in rows)
    assert os.path.exists(f.WEIGHT_PREFIX + "-2.npz")
    g = dg.DGCNN_FLAGS(ITERATION=1, MODEL_PATH=f.WEIGHT_PREFIX + "-2", OUTPUT_FILE=str(tmp_path / "out.npz"), LOG_DIR=str(tmp_path / "ilog"),
                       BN_PER_CLOUD=True, **common)
    M.inference(g)
    capsys.readouterr()
    z = np.load(tmp_path / "out.npz")
    assert z["idx"].tolist() == list(range(8)) and np.diff(z["data_offsets"]).tolist() == counts
    assert z["softmax"].shape == (sum(counts), 2) and np.isfinite(z["softmax"]).all()
    assert np.allclose(z["softmax"].sum(1), 1.0, atol=1e-5)

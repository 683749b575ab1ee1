"""The BatchNorm passes that write operand planes (csrc/planes_bn.hip) against tests/bn_reference.py: fp32 outputs bit-equal to the
float32 replay, decoded planes within the two-fp16-term split bound, sums against float64, column maxima and the derived
power-of-two scale exactly as planes_bn.hip states them."""
import math

import numpy as np
import pytest
import torch

import bn_reference as BR
from dgcnn import _planes as P
from gpu_helpers import Guard, SENT, host, note_ratio, planes_to_host, ptr as p, ratio_table

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture()
def dg():
    import dgcnn
    dgcnn.reset()
    return dgcnn


@pytest.fixture(scope="module", autouse=True)
def _error_table():
    yield
    ratio_table()


def pow2_scale_for(bound):
    """planes_common.h: the power of two that brings `bound` (fp32) into [2^14, 2^15)."""
    bound = float(F32(bound))
    if not (bound > 0 and math.isfinite(bound)):
        return 1.0
    e = math.frexp(bound)[1]
    return 2.0 ** max(-100, min(100, 15 - e))


def plane_set(g, R, F):
    """A PlaneSet whose storage sits between guards and starts out as 0x55 bytes (pad rows must be WRITTEN as zeros)."""
    ps = P.PlaneSet(R, F, device="cuda")
    ps.buf = g.new((ps.buf.numel(),), torch.uint8, fill=0x55)
    return ps


def check_planes(ps, want, R, F, what):
    """Decoded planes against the fp32 tensor `want`: 22 significant bits per element (h1 = rn16(x s), h2 = rn16(x s - h1)), never
    worse than 2^-25 in scaled units (h2 subnormal) -- which implies the 2^-21 bar relative to the tensor's scale; pad rows zero; no
    inf / NaN halves."""
    sc = float(ps.scale)
    raw = host(ps.buf).reshape(2, F // 8, ps.ra, 16)
    assert not raw[:, :, R:, :].any(), what + ": pad rows are not zero"
    assert np.isfinite(raw.view(np.float16).astype(np.float32)).all(), what + ": inf / NaN halves"
    got = planes_to_host(ps)
    err = np.abs(got - want.astype(np.float64))
    bound = np.maximum(np.abs(want).astype(np.float64) * 2.0 ** -22, 2.0 ** -25 / sc)
    assert (err <= bound).all(), "%s: %g" % (what, float((err / bound).max()))
    assert err.max() <= 2.0 ** -21 * max(float(np.abs(want).max()), 2.0 ** 14 / sc)
    assert float(np.abs(want).max()) * sc < 2.0 ** 15, what + ": the scale lets a value reach 2^15"


def param_scales(H, g, params, rows_max, act_mul):
    pd = g.put(params)
    sc = g.new((2,))
    ws = g.new((1,), torch.int32)
    H.call("dgcnn_param_scales_f32", pd.data_ptr(), params.size, float(rows_max), float(act_mul), sc.data_ptr(), ws.data_ptr())
    pm = F32(np.abs(params).max())
    want0 = pow2_scale_for(F32(act_mul) * (F32(math.sqrt(rows_max)) + pm))      # the formula of its comment, evaluated in fp32
    want1 = pow2_scale_for(pm)
    got = host(sc)
    assert (float(got[0]), float(got[1])) == (want0, want1), (got, want0, want1)
    return sc


def stats_of(H, g, T):
    n, F = T.shape
    Td = T.astype(np.float64)
    st = g.zeros((H.stat_slots(), 2, F), torch.float64)
    st[0, 0], st[0, 1] = torch.from_numpy(Td.sum(0)).cuda(), torch.from_numpy((Td * Td).sum(0)).cuda()
    mean, rstd = g.new((F,)), g.new((F,))
    H.call("dgcnn_bn_finalize_f32", st.data_ptr(), F, float(n), BR.EPS, mean.data_ptr(), rstd.data_ptr())
    return host(mean).copy(), host(rstd).copy()


@pytest.mark.parametrize("R", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("F", [8, 24, 128, 136, 1024])
def test_bn_act_planes(dg, R, F):
    """dgcnn_bn_act_planes_f32: F = 24 / 136: a partial last wave of octets; strided ldt; scale from dgcnn_param_scales_f32."""
    from dgcnn import _hip as H
    _act_planes(H, R, F)


def test_bn_act_planes_beyond_one_grid(dg):
    """plane_grid caps the grid at 4096 workgroups of 64 rows: above 262144 rows a workgroup walks on with `r += step`."""
    from dgcnn import _hip as H
    _act_planes(H, 262144 + 64 * 37 + 5, 8)


def _act_planes(H, R, F):
    rng = np.random.default_rng(R * 10 + F)
    g = Guard()
    ldt = F + 8
    Tw = rng.normal(size=(R, ldt)).astype(F32)
    T = Tw[:, :F]
    if R >= 8:
        T[:, 0] = 1.25
    mu, rs = stats_of(H, g, np.ascontiguousarray(T))
    be = rng.normal(0, 0.3, F).astype(F32)
    par = tuple(g.put(a).data_ptr() for a in (mu, rs, be))
    relu = (R + F // 8) % 2
    act_mul = 1 + (F // 8) % 2
    sc = param_scales(H, g, np.concatenate([be, rng.normal(0, 0.1, 1000 + F).astype(F32)]), max(R, 1), act_mul)
    Td = g.put(Tw)
    ps = plane_set(g, R, F)
    ps.scale = sc[:1]
    out, out2 = g.new((R, F + 4)), g.new((R, F))
    H.call("dgcnn_bn_act_planes_f32", Td.data_ptr(), ldt, R, F, *par, relu, P.F16X2, sc.data_ptr(), ps.ptr(), ps.plane_stride, ps.ra,
           out.data_ptr(), F + 4, out2.data_ptr(), F)
    z = BR.Fwd(np.ascontiguousarray(T)[:, None, :], mu, rs, be, relu).z[:, 0]
    oh = host(out)
    np.testing.assert_array_equal(oh[:, :F], z)
    assert (oh[:, F:] == SENT).all()
    np.testing.assert_array_equal(host(out2), z)
    check_planes(ps, z, R, F, "bn_act_planes (%d, %d)" % (R, F))
    # without the fp32 copies: the same planes
    ps2 = plane_set(g, R, F)
    ps2.scale = sc[:1]
    H.call("dgcnn_bn_act_planes_f32", Td.data_ptr(), ldt, R, F, *par, relu, P.F16X2, sc.data_ptr(), ps2.ptr(), ps2.plane_stride, ps2.ra, 0, 0, 0, 0)
    assert torch.equal(ps.buf, ps2.buf)
    g.check()


@pytest.mark.parametrize("act_mul,n", [(1.0, 5000), (2.0, 4097), (1.0, 3)])
def test_activation_bound_holds_a_one_hot_column(dg, act_mul, n):
    """The bound behind scales[0]: a column that is 100 in one row and 0 elsewhere (R = 4096) reaches xhat ~ sqrt(R - 1); with
    rows_max = R the planes must hold it without overflow.  dgcnn_param_scales_f32 against the formula of its comment, n not a
    multiple of 4096."""
    from dgcnn import _hip as H
    R, F = 4096, 8
    rng = np.random.default_rng(n)
    g = Guard()
    T = np.zeros((R, F), F32)
    T[np.arange(F) * 37, np.arange(F)] = 100
    T[:, 1] *= -1
    mu, rs = stats_of(H, g, T)
    params = rng.normal(0, 0.5, n).astype(F32)
    be = np.resize(params, F).astype(F32)
    sc = param_scales(H, g, params, R, act_mul)
    par = tuple(g.put(a).data_ptr() for a in (mu, rs, be))
    ps = plane_set(g, R, F)
    ps.scale = sc[:1]
    out = g.new((R, F))
    H.call("dgcnn_bn_act_planes_f32", g.put(T).data_ptr(), F, R, F, *par, 0, P.F16X2, sc.data_ptr(), ps.ptr(), ps.plane_stride, ps.ra,
           out.data_ptr(), F, 0, 0)
    z = BR.Fwd(T[:, None, :], mu, rs, be, 0).z[:, 0]
    assert np.abs(z).max() > math.sqrt(R - 1) - 1.0                       # the bound is nearly attained
    np.testing.assert_array_equal(host(out), z)
    check_planes(ps, z, R, F, "one-hot column")
    g.check()


def _reduce_apply(H, g, T, mu, rs, be, relu, dout, rpg, want_dT=True):
    """-> dict of host results of dgcnn_bn1_bwd_reduce_max_f32 + dgcnn_bn1_bwd_apply_planes_f32."""
    R, F = T.shape
    par = tuple(g.put(a).data_ptr() for a in (mu, rs, be))
    Td = g.put(T)
    ldd = F + 4
    dd = g.new((R, ldd))
    dd[:, :F] = torch.from_numpy(dout).cuda()
    red = g.zeros((max(H.stat_slots(), 32), 2, F), torch.float64)
    mb = g.zeros((2 * F + 1,), torch.int32)
    H.call("dgcnn_bn1_bwd_reduce_max_f32", Td.data_ptr(), R, F, *par, relu, dd.data_ptr(), ldd, red.data_ptr(), mb.data_ptr())
    res = {"sums": host(red).sum(0), "maxima": host(mb)[:2 * F].view(F32).reshape(2, F).copy()}
    assert host(mb)[2 * F] == 0
    if F % 8:
        return res
    ps = plane_set(g, R, F)
    ps.scale = g.new((1,))
    dT = g.new((R, F)) if want_dT else None
    G = -(-R // rpg) if rpg else 0
    gs = g.zeros((G, F + 4)) if rpg else None
    prior = np.arange(F, dtype=F32)
    dbeta = g.put(prior)
    H.call("dgcnn_bn1_bwd_apply_planes_f32", Td.data_ptr(), R, F, *par, relu, dd.data_ptr(), ldd, red.data_ptr(), mb.data_ptr(), P.F16X2,
           ps.scale.data_ptr(), ps.ptr(), ps.plane_stride, ps.ra, p(dT), p(gs), F + 4 if rpg else 0, rpg, dbeta.data_ptr(), 1.0)
    res.update(ps=ps, dT=host(dT) if want_dT else None, gsum=host(gs) if rpg else None, dbeta=host(dbeta), prior=prior, red0=host(red)[0],
               cf=host(mb).view(F32)[:2 * F].reshape(2, F).copy(), bound=float(host(mb)[2 * F:].view(F32)[0]), scale=float(host(ps.scale)[0]))
    return res


@pytest.mark.parametrize("nslots", [32, 256])
@pytest.mark.parametrize("R,F,rpg,adv", [(1000, 128, 64, False), (1536, 64, 192, False), (2048, 8, 512, True), (4096, 24, 2048, False),
                                         (333, 1032, 0, False), (64, 136, 64, True), (1, 8, 0, False)])
def test_bn1_bwd_reduce_max_and_apply_planes(dg, R, F, rpg, adv, nslots):
    """Sums against float64, column maxima EQUAL max |dz| / max |xhat| of the replay, the scale a power of two derived from the
    largest column bound rstd (max |dz| + |m1| + max |xhat| |m2|) times 1.0001, max |dT| scale < 2^15, fp32 dT bit-equal to the
    replay, decoded planes within the split bound, per-group column sums against float64; adversarial dout (one element 1e4, the
    rest 1e-3); F = 1032: a second blockIdx.y.  The plane kernels use 32 slots whatever the runtime slot count is."""
    from dgcnn import _hip as H
    old = H.stat_slots()
    H.set_stat_slots(nslots)
    try:
        rng = np.random.default_rng(R + F)
        g = Guard()
        T = rng.normal(size=(R, F)).astype(F32)
        if R >= 8:
            T[-(R // 10):] -= 50                                             # dead rows under ReLU
            T[:, 0] = 1.25
            T[:, -1] = (1000 + 0.01 * rng.normal(size=R)).astype(F32)
        mu, rs = stats_of(H, g, T)
        be = rng.normal(0, 0.3, F).astype(F32)
        if adv:
            dout = np.full((R, F), 1e-3, F32)
            dout[R // 2, F // 2] = 1e4
        else:
            dout = rng.normal(size=(R, F)).astype(F32)
        relu = 1
        res = _reduce_apply(H, g, T, mu, rs, be, relu, dout, rpg)
        fw = BR.Fwd(T[:, None, :], mu, rs, be, relu)
        d32 = BR.dz32(fw, dout, None)
        s = BR.Sums(BR.dz64(fw, dout, None), fw.xh)
        bound = BR.sum_bound(s.n_terms, s.scale)
        note_ratio("bn1_bwd_reduce_max sums", res["sums"] - s.red, s.scale, s.n_terms, s.n_terms + 8)
        np.testing.assert_array_equal(res["maxima"][0], np.abs(d32[:, 0]).max(0))
        np.testing.assert_array_equal(res["maxima"][1], np.abs(fw.xh[:, 0]).max(0))
        # ---- apply: everything below is a function of the sums the reduce pass itself formed
        tot = res["red0"]
        assert (np.abs(tot - s.red) <= bound).all()
        m = (tot / float(R)).astype(F32)                                   # the two column means, float(s / count)
        np.testing.assert_array_equal(res["cf"], m)
        np.testing.assert_array_equal(res["dbeta"], tot[0].astype(F32) + res["prior"])
        colb = fw.rs * ((res["maxima"][0] + np.abs(m[0])) + res["maxima"][1] * np.abs(m[1]))
        assert colb.dtype == F32
        want_bound = F32(colb.max()) * F32(1.0001)
        assert res["bound"] == float(want_bound)
        assert res["scale"] == pow2_scale_for(want_bound) and math.frexp(res["scale"])[0] == 0.5
        edT = fw.rs * ((d32[:, 0] - m[0]) - fw.xh[:, 0] * m[1])             # the kernel's operation order
        np.testing.assert_array_equal(res["dT"], edT)
        assert float(np.abs(edT).max()) * res["scale"] < 2.0 ** 15
        ref = BR.dy64(BR.dz64(fw, dout, None), fw.xh, fw.rs, tot)[:, 0]
        sc_ = np.abs(fw.rs.astype(np.float64)) * (np.abs(d32[:, 0]) + np.abs(tot[0] / R) + np.abs(fw.xh[:, 0] * (tot[1] / R)))
        assert (np.abs(edT - ref) <= 8 * 2.0 ** -24 * sc_ + 1e-30).all()
        check_planes(res["ps"], edT, R, F, "bn1_bwd_apply_planes (%d, %d)" % (R, F))
        if rpg:
            G = -(-R // rpg)
            pad = np.zeros((G * rpg, F))
            pad[:R] = edT
            gref, gabs = pad.reshape(G, rpg, F).sum(1), np.abs(pad).reshape(G, rpg, F).sum(1)
            assert (res["gsum"][:, F:] == 0).all()
            note_ratio("bn1_bwd_apply_planes gsum", res["gsum"][:, :F] - gref, gabs, rpg, rpg + 8)
        g.check()
    finally:
        H.set_stat_slots(old)


@pytest.mark.parametrize("R,F", [(85, 12), (1000, 1028), (3, 100), (3000, 1028), (12000, 100)])
def test_bn1_bwd_reduce_max_on_an_exact_lattice(dg, R, F):
    """Sums must EQUAL the float64 sums on lattice input (any order); F = 1028: one live quad in the second blockIdx.y; (3000, 1028)
    and (12000, 100): more rows than the grid (capped at 256 workgroups x 256 / min(F / 4, 256) row groups x 4 rows in flight) covers
    in one trip, so the row loop runs again."""
    from dgcnn import _hip as H
    rng = np.random.default_rng(R + F)
    g = Guard()
    mu, rs, be = BR.lattice_params(rng, F)
    y = BR.lattice_dense(rng, R, 1, F, 1)
    dout, _ = BR.lattice_grads(rng, R, 1, F, with_mean=False)
    fw = BR.Fwd(y, mu, rs, be, 1)
    s = BR.lattice_precondition(fw, dout, None)
    res = _reduce_apply(H, g, y[:, 0], mu, rs, be, 1, dout, 0)
    np.testing.assert_array_equal(res["sums"], s.red)
    np.testing.assert_array_equal(res["maxima"][0], np.abs(BR.dz32(fw, dout, None)[:, 0]).max(0))
    np.testing.assert_array_equal(res["maxima"][1], np.abs(fw.xh[:, 0]).max(0))
    g.check()


def test_group_sums_refuse_groups_that_are_no_multiple_of_64(dg):
    from dgcnn import _hip as H
    g = Guard()
    R, F = 200, 8
    z = g.zeros((R, F))
    v = g.zeros((F,))
    red = g.zeros((32, 2, F), torch.float64)
    mb = g.zeros((2 * F + 1,), torch.int32)
    ps = plane_set(g, R, F)
    sc = g.new((1,))
    gs = g.zeros((2, F))
    with pytest.raises(H.HipError):
        H.call("dgcnn_bn1_bwd_apply_planes_f32", z.data_ptr(), R, F, v.data_ptr(), v.data_ptr(), v.data_ptr(), 1, z.data_ptr(), F, red.data_ptr(),
               mb.data_ptr(), P.F16X2, sc.data_ptr(), ps.ptr(), ps.plane_stride, ps.ra, 0, gs.data_ptr(), F, 100, 0, 0.0)
    for bad in (2, 3):
        with pytest.raises(ValueError):
            H.call("dgcnn_bn1_bwd_apply_planes_f32", z.data_ptr(), R, F, v.data_ptr(), v.data_ptr(), v.data_ptr(), bad, z.data_ptr(), F, red.data_ptr(),
                   mb.data_ptr(), P.F16X2, sc.data_ptr(), ps.ptr(), ps.plane_stride, ps.ra, 0, 0, 0, 0, 0, 0.0)
        with pytest.raises(ValueError):
            H.call("dgcnn_bn1_bwd_reduce_max_f32", z.data_ptr(), R, F, v.data_ptr(), v.data_ptr(), v.data_ptr(), bad, z.data_ptr(), F, red.data_ptr(),
                   mb.data_ptr())
        with pytest.raises(ValueError):
            H.call("dgcnn_bn_act_planes_f32", z.data_ptr(), F, R, F, v.data_ptr(), v.data_ptr(), v.data_ptr(), bad, P.F16X2, 0, ps.ptr(),
                   ps.plane_stride, ps.ra, 0, 0, 0, 0)
    assert (host(ps.buf) == 0x55).all()
    g.check()

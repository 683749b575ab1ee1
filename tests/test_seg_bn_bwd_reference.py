"""CPU checks of tests/seg_bn_bwd_reference.py (float64): its per-cloud backward is the oracle's backward on each cloud alone, and
the tower-wide backward of the default packed path is another function of the same tower -- far apart at the shapes of the GPU
tests (tests/test_gpu_seg_bn_bwd.py), so their 5e-3 bar can tell the two apart."""
import numpy as np

from oracle import dgcnn_oracle as O
import seg_bn_bwd_reference as SB

SIZES = [21, 700, 64, 333]


def offsets_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def scaled_clouds(rng, sizes, C):
    """Clouds on different scales and positions: what makes tower-wide statistics differ from per-cloud ones."""
    return np.concatenate([rng.normal(0.5 * b, 0.5 + 0.7 * b, (n, C)) for b, n in enumerate(sizes)])


def fro(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def test_conv_bn_act_bwd_is_the_oracle_on_each_cloud():
    rng = np.random.default_rng(0)
    off = offsets_of([1, 63, 64, 65, 130, 5])
    R, Cin, F = int(off[-1]), 7, 12
    x, W, beta, dout = rng.normal(size=(R, Cin)), rng.normal(size=(Cin, F)), rng.normal(0, 0.3, F), rng.normal(size=(R, F))
    for relu in (True, False):
        dx, dW, dbeta = SB.conv_bn_act_bwd(x, W, beta, relu, off, dout)
        rW, rb = np.zeros_like(W), np.zeros(F)
        for _, lo, hi in SB.clouds(off):
            _, cache = O.conv_bn_act(x[None, lo:hi, None, :], W, beta, relu=relu)
            odx, odW, odb = O.conv_bn_act_bwd(dout[None, lo:hi, None, :], cache)
            np.testing.assert_allclose(dx[lo:hi], odx[0, :, 0, :], rtol=0, atol=1e-10)
            rW += odW
            rb += odb
        np.testing.assert_allclose(dW, rW, rtol=0, atol=1e-10)
        np.testing.assert_allclose(dbeta, rb, rtol=0, atol=1e-10)


def test_edge_conv_bwd_is_the_oracle_on_each_cloud():
    rng = np.random.default_rng(1)
    sizes = [9, 40, 17]
    off = offsets_of(sizes)
    R, C, k, F = int(off[-1]), 3, 5, 8
    x = rng.normal(size=(R, C))
    W0, b0, W1, b1 = rng.normal(size=(2 * C, F)), rng.normal(0, 0.3, F), rng.normal(size=(2 * F, 64)), rng.normal(0, 0.3, 64)
    idx = np.concatenate([O.k_nn(x[None, lo:hi].astype(np.float32), k)[0] + lo for _, lo, hi in SB.clouds(off)])
    idx[::3, 1] = idx[::3, 0]                                                   # duplicates: exact ties of the max
    d_max, d_mean, d_net = rng.normal(size=(R, F)), rng.normal(size=(R, F)), rng.normal(size=(R, 64))
    for relu1 in (True, False):
        dx, g = SB.edge_conv_bwd(x, idx, W0, b0, W1, b1, relu1, off, d_max, d_mean, d_net)
        ref = dict(W0=0.0, beta0=0.0, W1=0.0, beta1=0.0)
        for _, lo, hi in SB.clouds(off):
            _, cache = O.edge_conv(x[None, lo:hi], k, W0, b0, W1, b1, relu1=relu1, idx=(idx[lo:hi] - lo)[None])
            odx, og = O.edge_conv_bwd(d_max[None, lo:hi, None, :], d_mean[None, lo:hi, None, :], d_net[None, lo:hi, None, :], cache)
            np.testing.assert_allclose(dx[lo:hi], odx[0], rtol=0, atol=1e-10)
            for key in ref:
                ref[key] = ref[key] + og[key]
        for key in ref:
            np.testing.assert_allclose(g[key], ref[key], rtol=0, atol=1e-10, err_msg=key)


def test_closed_form_terms_sum_to_the_closed_form():
    import bn_reference as BR
    rng = np.random.default_rng(2)
    n, k, F = 50, 5, 6
    y = rng.normal(size=(n, k, F)).astype(np.float32)
    fw = BR.Fwd(y, np.zeros(F), np.ones(F), rng.normal(0, 0.3, F), 1)
    dmax, dmean = rng.normal(size=(n, F)), rng.normal(size=(n, F))
    t0, t1 = SB.point_terms64(fw.mx, fw.mean64, fw.npos, dmax, dmean, fw.be, k)
    np.testing.assert_allclose(np.stack([t0.sum(0), t1.sum(0)]), BR.points_closed_form64(fw.mx, fw.mean64, fw.npos, dmax, dmean, fw.be, k),
                               rtol=1e-13, atol=1e-13)


def test_tower_wide_backward_is_another_function():
    """Four clouds of 21 / 700 / 64 / 333 points: the backward with tower-wide statistics (one 'cloud' of R rows) differs from the
    per-cloud backward by more than 10 x the 5e-3 bar on every output, for a k = 1 layer and for an EdgeConv layer."""
    rng = np.random.default_rng(3)
    off = offsets_of(SIZES)
    R = int(off[-1])
    wide = np.array([0, R])
    x = scaled_clouds(rng, SIZES, 8)
    W, beta, dout = rng.normal(size=(8, 16)), rng.normal(0, 0.3, 16), rng.normal(size=(R, 16))
    a, b = SB.conv_bn_act_bwd(x, W, beta, True, off, dout), SB.conv_bn_act_bwd(x, W, beta, True, wide, dout)
    d = [fro(u, v) for u, v in zip(b, a)]
    print("k = 1 layer: tower-wide vs per-cloud (dx, dW, dbeta) relative Frobenius %s" % np.array2string(np.array(d), precision=3))
    assert min(d) > 10 * 5e-3
    C, k, F = 4, 8, 16
    pts = scaled_clouds(rng, SIZES, C)
    idx = np.concatenate([O.k_nn(pts[None, lo:hi].astype(np.float32), k)[0] + lo for _, lo, hi in SB.clouds(off)])
    W0, b0, W1, b1 = rng.normal(size=(2 * C, F)), rng.normal(0, 0.3, F), rng.normal(size=(2 * F, 64)), rng.normal(0, 0.3, 64)
    dm, dn, dt = rng.normal(size=(R, F)), rng.normal(size=(R, F)), rng.normal(size=(R, 64))
    dxa, ga = SB.edge_conv_bwd(pts, idx, W0, b0, W1, b1, True, off, dm, dn, dt)
    dxb, gb = SB.edge_conv_bwd(pts, idx, W0, b0, W1, b1, True, wide, dm, dn, dt)
    d = [fro(dxb, dxa)] + [fro(gb[key], ga[key]) for key in ("W0", "beta0", "W1", "beta1")]
    print("EdgeConv layer: tower-wide vs per-cloud (dx, dW0, dbeta0, dW1, dbeta1) %s" % np.array2string(np.array(d), precision=3))
    assert min(d) > 10 * 5e-3

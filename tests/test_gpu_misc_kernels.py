"""The scalar tail of csrc/misc.hip (softmax / cross-entropy / accuracy, Adam, axpby, global max-pool and its gradient, group column
sums, tile, residual add + ReLU, strided copies) at the shapes and edges the model tests do not reach: each kernel against a plain
numpy reference, element-wise results bit for bit where the kernel is a fixed sequence of fp32 operations, sums against float64
with the any-order fp32 bound, strided outputs inside sentinel-filled buffers."""
import numpy as np
import pytest
import torch

from gpu_helpers import Guard, SENT, host
from oracle import dgcnn_oracle as O

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture()
def dg():
    import dgcnn
    dgcnn.reset()
    return dgcnn


def wide(g, a, pad=3):
    """`a` (R, F) inside a sentinel-filled (R, F + pad) device buffer -> (view, whole buffer)."""
    R, F = a.shape
    w = g.new((R, F + pad))
    w[:, :F] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return w[:, :F], w


def pads_untouched(w, F):
    return (host(w)[:, F:] == SENT).all()


# ------------------------------------------------------------------------------------------------------ softmax / xent
@pytest.mark.parametrize("rows", [1, 255, 257, 49152])
@pytest.mark.parametrize("ncls", [2, 3, 5, 8])
def test_softmax_xent(dg, ncls, rows):
    from dgcnn import _hip as H
    rng = np.random.default_rng(ncls * 7 + rows)
    g = Guard()
    z = rng.normal(0, 3, (rows, ncls)).astype(F32)
    z[::5] = rng.choice(np.array([-80, 80, 0], F32), (len(z[::5]), ncls))              # saturating logits: no inf / NaN
    z[1::7, :] = z[1::7, :1]                                                           # ties: accuracy counts the FIRST class
    lab = rng.integers(0, ncls, rows).astype(np.int32)
    lab[1::7] = rng.integers(0, 2, len(lab[1::7]))
    w = (0.5 + rng.random(rows)).astype(F32)
    zd, ld_, wd = g.put(z), g.put(lab), g.put(w)
    loss64, sm64, acc64, dl64 = O.softmax_xent(z.astype(np.float64)[None], lab[None], w.astype(np.float64)[None])
    lse = -np.log(sm64[0][np.arange(rows), lab])
    # a thread adds ceil(rows / (blocks 256)) terms, the block tree 8 levels, then one atomic per block: any-order bound
    blocks = min(max(1, -(-rows // 256)), 1024)
    depth = -(-rows // (blocks * 256)) + 8 + blocks
    for weighted in (True, False):
        sm, dl, sc = g.new((rows, ncls)), g.new((rows, ncls)), g.zeros((2,))
        H.call("dgcnn_softmax_xent_f32", zd.data_ptr(), ld_.data_ptr(), wd.data_ptr() if weighted else 0, rows, ncls, sm.data_ptr(),
               dl.data_ptr(), sc.data_ptr())
        ww = w.astype(np.float64) if weighted else np.ones(rows)
        smh, dlh, sch = host(sm), host(dl), host(sc)
        assert np.isfinite(smh).all() and np.isfinite(dlh).all() and np.isfinite(sch).all()
        # p = expf(z - mx) / se: expf within 2 ulp, ncls additions, one division, one product
        tol_p = (ncls + 8) * 2.0 ** -23
        assert np.abs(smh - sm64[0]).max() <= tol_p
        dref = (sm64[0] - np.eye(ncls)[lab]) * (ww / rows)[:, None]
        assert (np.abs(dlh - dref) <= (tol_p + 2.0 ** -22) * (ww / rows)[:, None]).all()
        terms = lse * ww / rows
        # per row: logf(se) and z - mx are each within ~2 ulp of values up to 160
        tol_loss = (depth + 8) * 2.0 ** -24 * np.abs(terms).sum() + 4 * 2.0 ** -23 * (160.0 * ww / rows).sum()
        assert abs(sch[0] - terms.sum()) <= tol_loss, (sch[0], terms.sum(), tol_loss)
        acc = float((np.argmax(z, 1) == lab).mean())                                   # np.argmax: the first maximum
        assert abs(sch[1] - acc) <= (depth + 8) * 2.0 ** -24 * max(acc, 1.0 / rows)
    # labels == NULL: softmax only, nothing is added to scal; softmax / dlogits NULL
    sm, sc = g.new((rows, ncls)), g.zeros((2,))
    H.call("dgcnn_softmax_xent_f32", zd.data_ptr(), 0, 0, rows, ncls, sm.data_ptr(), 0, sc.data_ptr())
    assert np.abs(host(sm) - sm64[0]).max() <= (ncls + 8) * 2.0 ** -23 and not host(sc).any()
    sc2 = g.zeros((2,))
    H.call("dgcnn_softmax_xent_f32", zd.data_ptr(), ld_.data_ptr(), wd.data_ptr(), rows, ncls, 0, 0, sc2.data_ptr())
    assert abs(host(sc2)[0] - (lse * w / rows).sum()) <= (depth + 8) * 2.0 ** -24 * np.abs(lse * w / rows).sum() + 4 * 2.0 ** -23 * (160.0 * w / rows).sum()
    with pytest.raises(ValueError):
        H.call("dgcnn_softmax_xent_f32", zd.data_ptr(), 0, 0, rows, ncls, 0, sm.data_ptr(), 0)      # dlogits needs labels
    g.check()


# --------------------------------------------------------------------------------------------------------- Adam / axpby
def test_adam_three_steps_against_the_oracle(dg):
    from dgcnn import _hip as H
    rng = np.random.default_rng(0)
    n, lr = 100003, 1e-3
    b1, b2, eps = (float(F32(v)) for v in (0.9, 0.999, 1e-8))                           # the fp32 values the kernel receives
    g = Guard()
    p0 = rng.normal(size=n).astype(F32)
    pd, md, vd = g.put(p0), g.zeros((n,)), g.zeros((n,))
    pr, mr, vr = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    sm, sv = np.zeros(n), np.zeros(n)
    for t in (1, 2, 3):
        gr = (rng.normal(size=n) * 10.0 ** rng.integers(-4, 2, n)).astype(F32)
        lr_t = lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
        H.call("dgcnn_adam_f32", pd.data_ptr(), g.put(gr).data_ptr(), md.data_ptr(), vd.data_ptr(), n, float(lr_t), b1, b2, eps)
        O.adam_step(pr, gr.astype(np.float64), mr, vr, t, lr, b1, b2, eps)
        # m, v: three roundings per step, each relative to the terms of that step, on top of the carried error (which decays by
        # b1 / b2): the scale is the same recurrence run on |g| and g^2, where nothing cancels.  The update: |lr_t m / (sqrt v +
        # eps)| <~ lr, and an error dm moves it by lr_t dm / sqrt(v) with sqrt(v) >= sqrt(1 - b2) b2 max |g|: <= 2^-16 lr per step
        gs = np.abs(gr).astype(np.float64)
        sm, sv = b1 * sm + gs, b2 * sv + gs * gs
        assert (np.abs(host(md) - mr) <= t * 4 * 2.0 ** -24 * sm).all()
        assert (np.abs(host(vd) - vr) <= t * 4 * 2.0 ** -24 * sv).all()
        assert (np.abs(host(pd) - pr) <= t * (2.0 ** -23 * np.abs(pr) + 2.0 ** -16 * lr)).all()
    assert np.abs(host(pd) - p0).max() > 0.5 * lr
    g.check()


def test_axpby_does_not_read_y_when_b_is_zero(dg):
    from dgcnn import _hip as H
    rng = np.random.default_rng(1)
    n = 70001
    g = Guard()
    x, y = rng.normal(size=n).astype(F32), rng.normal(size=n).astype(F32)
    y[::3] = np.nan
    y[1::3] = np.inf
    yd = g.put(y)
    H.call("dgcnn_axpby_f32", g.put(x).data_ptr(), 0.75, yd.data_ptr(), 0.0, n)
    np.testing.assert_array_equal(host(yd), F32(0.75) * x)                             # NaN / inf in y do not propagate
    y2 = rng.normal(size=n).astype(F32)
    yd2 = g.put(y2)
    H.call("dgcnn_axpby_f32", g.put(x).data_ptr(), 0.3, yd2.data_ptr(), -1.7, n)
    np.testing.assert_array_equal(host(yd2), F32(0.3) * x + F32(-1.7) * y2)            # two products, one sum, no contraction
    g.check()


# ------------------------------------------------------------------------------------------------------ global max-pool
@pytest.mark.parametrize("N", [1, 15, 16, 128, 129, 2048])
@pytest.mark.parametrize("F", [1, 63, 64, 70])
def test_global_max_and_its_gradient(dg, N, F):
    """Strided ldx; the same maximum in two different row groups -> the lowest index; a -inf column -> arg 0."""
    from dgcnn import _hip as H
    B = 3
    rng = np.random.default_rng(N * 100 + F)
    g = Guard()
    a = rng.normal(size=(B, N, F)).astype(F32)
    if N >= 15:
        a[1, 13, :] = a[1, 2, :] = 9.0                                                 # rows 13 and 2: different row groups, found in any order
        a[2, N - 1, 0] = a[2, N - 6, 0] = 9.0
    a[0, :, F - 1] = -np.inf
    xv, xw = wide(g, a.reshape(B * N, F))
    out = g.new((B, F))
    arg = g.new((B, F), torch.int32)
    H.call("dgcnn_global_max_f32", xv.data_ptr(), F + 3, B, N, F, out.data_ptr(), arg.data_ptr())
    np.testing.assert_array_equal(host(out), a.max(1))
    np.testing.assert_array_equal(host(arg), a.argmax(1))
    assert (host(arg)[0, F - 1] == 0) and pads_untouched(xw, F)
    # gradient: dx[b][arg][f] += dout[b][f], everything else untouched
    prior = rng.normal(size=(B * N, F)).astype(F32)
    dv, dw = wide(g, prior, pad=5)
    dout = rng.normal(size=(B, F)).astype(F32)
    H.call("dgcnn_global_max_bwd_f32", g.put(dout).data_ptr(), arg.data_ptr(), B, N, F, dv.data_ptr(), F + 5)
    want = prior.reshape(B, N, F).copy()
    bi, fi = np.meshgrid(np.arange(B), np.arange(F), indexing="ij")
    want[bi, a.argmax(1), fi] += dout
    np.testing.assert_array_equal(host(dw)[:, :F], want.reshape(B * N, F))
    assert pads_untouched(dw, F)
    g.check()


@pytest.mark.parametrize("G,rpg,F", [(1, 1, 1), (3, 500, 70), (5, 127, 64), (2, 129, 63), (4, 2048, 8)])
def test_group_colsum_and_tile_rows(dg, G, rpg, F):
    from dgcnn import _hip as H
    rng = np.random.default_rng(G * 1000 + rpg + F)
    g = Guard()
    for exact in (True, False):
        a = (rng.integers(-8, 9, (G * rpg, F)) if exact else rng.normal(size=(G * rpg, F))).astype(F32)
        xv, xw = wide(g, a)
        out = g.new((G, F))
        H.call("dgcnn_group_colsum_f32", xv.data_ptr(), F + 3, G, rpg, F, out.data_ptr())
        ref = a.astype(np.float64).reshape(G, rpg, F).sum(1)
        if exact:
            np.testing.assert_array_equal(host(out), ref)                              # integers: exact in any order
        else:
            bound = (rpg + 8) * 2.0 ** -24 * np.abs(a).astype(np.float64).reshape(G, rpg, F).sum(1)
            assert (np.abs(host(out) - ref) <= bound).all()
    src = rng.normal(size=(G, F)).astype(F32)
    sv, sw = wide(g, src, pad=1)
    dv, dw = wide(g, np.zeros((G * rpg, F), F32), pad=2)
    H.call("dgcnn_tile_rows_f32", sv.data_ptr(), F + 1, G, rpg, F, dv.data_ptr(), F + 2)
    np.testing.assert_array_equal(host(dw)[:, :F], np.repeat(src, rpg, axis=0))
    assert pads_untouched(dw, F) and pads_untouched(sw, F)
    g.check()


# ------------------------------------------------------------------------------------- element-wise kernels with strides
@pytest.mark.parametrize("R,F", [(1, 1), (37, 70), (1000, 3), (513, 64)])
def test_add_relu_copy_and_pad_kernels(dg, R, F):
    from dgcnn import _hip as H
    rng = np.random.default_rng(R + F)
    g = Guard()
    a, b = rng.normal(size=(R, F)).astype(F32), rng.normal(size=(R, F)).astype(F32)
    b[::2] = -a[::2]                                                                   # exact zeros: relu(0) = 0, gradient 0
    av, aw = wide(g, a, 1)
    bv, bw = wide(g, b, 2)
    ov, ow = wide(g, np.full((R, F), 5, F32), 3)
    H.call("dgcnn_add_relu_f32", av.data_ptr(), F + 1, bv.data_ptr(), F + 2, R, F, ov.data_ptr(), F + 3)
    want = np.maximum(a + b, F32(0))
    np.testing.assert_array_equal(host(ow)[:, :F], want)
    assert pads_untouched(ow, F)
    dout = rng.normal(size=(R, F)).astype(F32)
    dv, dw = wide(g, dout, 4)
    rv, rw = wide(g, np.full((R, F), 5, F32), 1)
    H.call("dgcnn_relu_bwd_f32", dv.data_ptr(), F + 4, ov.data_ptr(), F + 3, R, F, rv.data_ptr(), F + 1)
    np.testing.assert_array_equal(host(rw)[:, :F], np.where(want > 0, dout, F32(0)))
    assert pads_untouched(rw, F)
    # copy2d: overwrite, then accumulate
    cv, cw = wide(g, b, 5)
    H.call("dgcnn_copy2d_f32", av.data_ptr(), F + 1, cv.data_ptr(), F + 5, R, F, 0)
    np.testing.assert_array_equal(host(cw)[:, :F], a)
    H.call("dgcnn_copy2d_f32", bv.data_ptr(), F + 2, cv.data_ptr(), F + 5, R, F, 1)
    np.testing.assert_array_equal(host(cw)[:, :F], a + b)
    assert pads_untouched(cw, F) and pads_untouched(aw, F) and pads_untouched(bw, F)
    # pad_copy: dst (R, Cp) dense <- [src | zeros]
    for Cp in (F, F + 1, ((F + 3) // 4) * 4 + 4):
        dst = g.new((R, Cp))
        H.call("dgcnn_pad_copy_f32", av.data_ptr(), F + 1, F, dst.data_ptr(), Cp, R)
        d = host(dst)
        np.testing.assert_array_equal(d[:, :F], a)
        assert not d[:, F:].any()
    g.check()

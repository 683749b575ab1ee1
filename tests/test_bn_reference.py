"""The numpy restatement of the BatchNorm passes (tests/bn_reference.py) against torch float64 autograd of the literal graph,
the per-point closed form against the edge-level sums, and the exact-lattice generators against their own precondition.
No GPU."""
import numpy as np
import pytest
import torch

import bn_reference as BR


def _case(rng, R, k, F, relu):
    """fp32 data with planted ties (two equal rows) and, under ReLU, all-dead points; true batch statistics."""
    y = rng.normal(size=(R, k, F)).astype(np.float32)
    if k > 1:
        y[: R // 3, 1] = y[: R // 3, 0]                       # ties wherever one of the two is the maximum
        y[R // 3: R // 2, :, : F // 2] = y[R // 3: R // 2, :1, : F // 2]     # k-fold ties
    if relu:
        y[-max(1, R // 10):] = -50 - rng.random((max(1, R // 10), k, F)).astype(np.float32)
    mu64, var64 = BR.two_pass_stats64(y.reshape(R * k, F))
    rs64 = 1.0 / np.sqrt(var64 + BR.EPS)
    be = rng.normal(0, 0.3, F).astype(np.float32)
    dmax = rng.normal(size=(R, F)).astype(np.float32)
    dmean = rng.normal(size=(R, F)).astype(np.float32)
    return y, mu64, rs64, be, dmax, dmean


def _autograd(y, mu64, rs64, be, dmax, dmean, relu):
    """d/dt of sum(dmax amax_k z + dmean mean_k z), z = relu?((t - mean(t)) / sqrt(var(t) + eps) + beta), in float64.
    The batch statistics are functions of t, as in slim.batch_norm's training mode."""
    R, k, F = y.shape
    t = torch.tensor(y.astype(np.float64), requires_grad=True)
    flat = t.reshape(R * k, F)
    mean = flat.mean(0)
    var = ((flat - mean) ** 2).mean(0)
    z = (t - mean) / torch.sqrt(var + BR.EPS) + torch.tensor(be.astype(np.float64))
    if relu:
        z = torch.relu(z)
    loss = (z.amax(1) * torch.tensor(dmax.astype(np.float64))).sum() + (z.mean(1) * torch.tensor(dmean.astype(np.float64))).sum()
    loss.backward()
    return t.grad.numpy()


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 7, 20])
def test_float64_layer_equals_autograd_of_the_literal_graph(k, relu):
    R, F = 300, 16
    rng = np.random.default_rng(10 * k + relu)
    y, mu64, rs64, be, dmax, dmean = _case(rng, R, k, F, relu)
    ref = _autograd(y, mu64, rs64, be, dmax, dmean, relu)
    # (a) the statistics rounded to fp32, as every kernel receives them
    fw = BR.Fwd(y, mu64.astype(np.float32), rs64.astype(np.float32), be, relu)
    if relu:
        assert (fw.ties == k).any() and (fw.npos == 0).any()        # all-dead points: every row ties at 0
    if k > 1:
        assert (fw.ties > 1).any()
    dz = BR.dz64(fw, dmax, dmean)
    s = BR.Sums(dz, fw.xh)
    dY = BR.dy64(dz, fw.xh, fw.rs, s.red)
    # torch shares amax's gradient evenly among ties, as the reference graph (tf.reduce_max) does: same function.
    # Bar: the effect of rounding mean / rstd to fp32 (each moves xh by <= 2^-24 (|xh| + |mu rs|); dY is quadratic in xh)
    bar = 4 * 2.0 ** -24 * np.abs(ref).max() * (1 + np.abs(fw.xh).max() ** 2)
    err = np.abs(dY - ref).max()
    print("k=%d relu=%d: max|dY - autograd| = %.3g (bar %.3g) at max|dY| = %.3g, ties up to %d" % (k, relu, err, bar, np.abs(ref).max(), fw.ties.max()))
    assert err <= bar
    # (b) float64 statistics: the decisions must be those of the float64 graph for the comparison to be exact, so the chain is
    # evaluated in float64 here (no fp32 decision layer) -- this pins the formulas alone
    z64 = (y.astype(np.float64) - mu64) * rs64 + be.astype(np.float64)
    xh64 = z64 - be.astype(np.float64)
    if relu:
        z64 = np.maximum(z64, 0)
    mx = z64.max(1, keepdims=True)
    ismax = z64 == mx
    dz_ = np.where(ismax, dmax.astype(np.float64)[:, None] / ismax.sum(1, keepdims=True), 0.0) + dmean.astype(np.float64)[:, None] / k
    if relu:
        dz_ = np.where(z64 > 0, dz_, 0.0)
    s_ = BR.Sums(dz_, xh64)
    assert np.abs(BR.dy64(dz_, xh64, rs64, s_.red) - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


def test_k1_form_and_replays_agree_with_the_float64_layer():
    rng = np.random.default_rng(3)
    R, F = 200, 12
    y, mu64, rs64, be, dmax, _ = _case(rng, R, 1, F, 1)
    fw = BR.Fwd(y, mu64.astype(np.float32), rs64.astype(np.float32), be, 1)
    assert np.array_equal(fw.ties, np.ones((R, F), np.float32)) and np.array_equal(fw.mean32, fw.mx)
    d32, d64 = BR.dz32(fw, dmax, None), BR.dz64(fw, dmax, None)
    assert np.array_equal(d32.astype(np.float64), d64)                                     # dz = dout exactly
    s = BR.Sums(d64, fw.xh)
    o, acc = BR.apply32(d32, fw.xh, fw.rs, s.red, R)
    assert np.array_equal(o[:, 0], acc)
    ref = BR.dy64(d64, fw.xh, fw.rs, s.red)
    # the replay differs from the float64 layer by the roundings of its own operations: c1, c2, the product, two differences, rs *
    scale = np.abs(fw.rs) * (np.abs(d64) + np.abs(s.red[0] / R) + np.abs(fw.xh * (s.red[1] / R)))
    assert (np.abs(o - ref) <= 6 * 2.0 ** -24 * scale + 1e-30).all()
    ob, accb = BR.apply32(d32, fw.xh, fw.rs, s.red, R, bf16=True)
    assert not (ob.view(np.uint32) & 0xffff).any() and (np.abs(ob - o) <= 2.0 ** -8 * np.abs(o)).all()
    assert np.array_equal(BR.round_bf16(np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], np.float32)),
                          np.array([1.0, 1.0 + 2.0 ** -6], np.float32))                    # ties go to the even neighbour


@pytest.mark.parametrize("k", [1, 6, 20])
def test_per_point_closed_form_equals_the_edge_level_sums(k):
    """sum_m dz = [max > 0] dmax + dmean npos / k ;  sum_m dz xh = [max > 0] dmax (max - beta) + (dmean / k) (k mean - beta npos)
    holds exactly when z = xh + beta is exact, so the chain is evaluated in float64 here."""
    rng = np.random.default_rng(k)
    R, F = 250, 8
    y, mu64, rs64, be, dmax, dmean = _case(rng, R, k, F, 1)
    xh = (y.astype(np.float64) - mu64) * rs64
    z = np.maximum(xh + be, 0)
    mx, mn, npos = z.max(1), z.mean(1), (z > 0).sum(1)
    ismax = z == mx[:, None]
    dz = np.where(z > 0, np.where(ismax, dmax.astype(np.float64)[:, None] / ismax.sum(1, keepdims=True), 0.0) + dmean.astype(np.float64)[:, None] / k, 0.0)
    s = BR.Sums(dz, xh)
    got = BR.points_closed_form64(mx, mn, npos, dmax, dmean, be, k)
    # float64 round-off only: z - beta for xh (relative to |xh| + 2 |beta|) and the sums themselves
    bound = 16 * R * k * 2.0 ** -53 * np.stack([s.abs0, s.abs1 + s.abs0 * 2 * np.abs(be)]) + 1e-300
    assert (np.abs(got - s.red) <= bound).all(), (np.abs(got - s.red) / bound).max()


@pytest.mark.parametrize("R,k,F,relu", [(100, 8, 64, 1), (37, 16, 128, 0), (513, 4, 48, 1), (5, 128, 8, 1), (3, 2, 1024, 0),
                                        (1000, 1, 3, 1), (4097, 1, 12, 1)])
def test_dense_lattice_satisfies_its_precondition(R, k, F, relu):
    rng = np.random.default_rng(R + k + F)
    mu, rs, be = BR.lattice_params(rng, F)
    y = BR.lattice_dense(rng, R, k, F, relu)
    dmax, dmean = BR.lattice_grads(rng, R, k, F, with_mean=True)
    fw = BR.Fwd(y, mu, rs, be, relu)
    s = BR.lattice_precondition(fw, dmax, dmean)
    assert set(np.unique(fw.ties[np.abs(BR.dz64(fw, dmax, dmean)).sum(1) > 0])) <= {1.0, 2.0, 4.0}
    if k >= 4 and not relu:
        assert set(np.unique(fw.ties)) == {1.0, 2.0, 4.0}
    # exactness means order independence: summing the float32 terms in fp32, forwards and backwards, gives the float64 sums
    t = (BR.dz32(fw, dmax, dmean) * fw.xh).reshape(R * k, F)
    for order in (t, t[::-1]):
        acc = np.zeros(F, np.float32)
        for row in order[: 4096]:
            acc = acc + row
        assert np.array_equal(acc.astype(np.float64), order[: 4096].astype(np.float64).sum(0))
    assert np.array_equal(fw.mean32.astype(np.float64), fw.mean64)
    assert np.abs(s.red).max() > 0


@pytest.mark.parametrize("B,N,k,F,relu", [(1, 5, 4, 8, 1), (3, 77, 8, 64, 1), (9, 40, 8, 16, 0), (2, 50, 1, 8, 1), (1, 130, 128, 4, 1)])
def test_edge_lattice_satisfies_its_precondition(B, N, k, F, relu):
    rng = np.random.default_rng(B + N + k)
    mu, rs, be = BR.lattice_params(rng, F)
    V, U, idx = BR.lattice_edge(rng, B, N, k, F, relu)
    assert idx.min() >= 0 and idx.max() < N
    y = BR.edge_rows32(V, U, idx, B, N)
    dmax, dmean = BR.lattice_grads(rng, B * N, k, F)
    fw = BR.Fwd(y, mu, rs, be, relu)
    s = BR.lattice_precondition(fw, dmax, dmean)
    # on the lattice z = xh + beta is exact, so the per-point closed form equals the edge-level sums exactly
    if relu:
        assert np.array_equal(BR.points_closed_form64(fw.mx, fw.mean64, fw.npos, dmax, dmean, be, k), s.red)
    assert np.array_equal(fw.packed % 256, fw.ties) and np.array_equal(np.floor(fw.packed / 256), fw.npos)


def test_finalize64_and_nearest_pow2():
    rng = np.random.default_rng(0)
    Y = rng.normal(3, 2, (500, 6)).astype(np.float32)
    Y[:, 0] = 1.25                                                   # constant column: var = 0 -> rstd = 1 / sqrt(eps)
    Yd = Y.astype(np.float64)
    mu, rs = BR.finalize64(Yd.sum(0), (Yd * Yd).sum(0), 500)
    m2, v2 = BR.two_pass_stats64(Y)
    np.testing.assert_allclose(mu, m2, rtol=1e-14)
    np.testing.assert_allclose(rs, 1 / np.sqrt(v2 + BR.EPS), rtol=1e-12)
    assert abs(rs[0] - 1 / np.sqrt(BR.EPS)) < 1e-9
    assert BR.finalize64(np.array([3.0]), np.array([2.9999999]), 3.0)[1][0] == 1 / np.sqrt(BR.EPS)      # negative variance clamps to 0
    assert [BR.nearest_pow2(k) for k in (1, 2, 3, 5, 6, 7, 20, 128, 255)] == [1, 2, 4, 4, 8, 8, 16, 128, 256]
    assert BR.nearest_pow2(255, cap=255) == 128

"""The float32 restatement of the feature interpolation (tests/interp_reference.py, what the kernels of csrc/interp.hip must equal bit for
bit) against the same expressions in float64, and the properties of the operator the restatement has to have.  No GPU, no kernel code.

Bounds (u = 2^-24), from the count of roundings, each allowed twice over:
  forward   |y32 - y64| <= (4k + 8) u max|feat|: a weight is one division, W k - 1 additions, the normalisation one division, the
            accumulation k products and k - 1 additions -- together under (2k + 3) u relative to sum a |feat| <= max|feat|;
  backward  per element |err| <= (deg_j + k + 4) u sum |a_e dy| over the bucket: deg_j - 1 additions and the product on top of the k + 2
            roundings inside a_e.
Measured on a CPU, over the shapes below (each test prints its ratio): at most 0.13 resp. 0.22 of these bounds, so they hide nothing."""
import numpy as np
import pytest

import interp_reference as R

U = 2.0 ** -24
SHAPES = [(1, 1, 1, 4), (65, 3, 3, 8), (257, 65, 3, 68), (130, 129, 8, 32), (300, 64, 64, 16), (33, 200, 20, 4)]     # (M, N, k, F)
EPS = 1e-16


@pytest.fixture(scope="module", params=SHAPES, ids=["M%d-N%d-k%d-F%d" % s for s in SHAPES])
def case(request):
    M, N, k, F = request.param
    q, p, feat, idx, dist = R.make_case(M, N, k, F, seed=M + 7 * N + k)
    dy = (np.random.default_rng(5).random((M, F), dtype=np.float32) * 2 - 1).astype(np.float32)
    a32, y32 = R.interp_f32(feat, idx, dist, EPS)
    a64, y64 = R.interp_f64(feat, idx, dist, EPS)
    return dict(M=M, N=N, k=k, F=F, feat=feat, idx=idx, dist=dist, dy=dy, a32=a32, y32=y32, a64=a64, y64=y64)


def test_forward_float32_against_float64(case):
    k = case["k"]
    assert case["y32"].dtype == np.float32 and case["a32"].dtype == np.float32
    err = np.abs(case["y32"].astype(np.float64) - case["y64"]).max()
    bound = (4 * k + 8) * U * np.abs(case["feat"]).max()
    print("forward: |y32 - y64| = %.3g, bound %.3g, ratio %.3f" % (err, bound, err / bound))
    assert err <= bound


def test_backward_float32_against_float64(case):
    k, N = case["k"], case["N"]
    d32 = R.interp_bwd_f32(case["a32"], case["idx"], case["dy"], N)
    d64 = R.interp_bwd_f64(case["a64"], case["idx"], case["dy"], N)
    assert d32.dtype == np.float32
    deg = np.bincount(case["idx"].ravel(), minlength=N).astype(np.float64)
    mag = np.zeros_like(d64)
    np.add.at(mag, case["idx"].ravel(), np.abs(case["a64"].reshape(-1, 1) * np.repeat(case["dy"].astype(np.float64), k, 0)))
    bound = (deg[:, None] + k + 4) * U * mag
    err = np.abs(d32.astype(np.float64) - d64)
    ratio = float((err / np.maximum(bound, 1e-300))[bound > 0].max(initial=0.0))
    print("backward: worst |err| / bound = %.3f" % ratio)
    assert (err <= bound).all()
    assert (d32[deg == 0] == 0).all()                       # nobody interpolates from the row: no gradient


def test_backward_is_the_adjoint_of_the_forward(case):
    """the operator is linear in feat: <dy, interp(f)> = <interp_bwd(dy), f> in float64"""
    N = case["N"]
    d64 = R.interp_bwd_f64(case["a64"], case["idx"], case["dy"], N)
    lhs = float((case["dy"].astype(np.float64) * case["y64"]).sum())
    rhs = float((d64 * case["feat"].astype(np.float64)).sum())
    scale = float(np.abs(case["dy"].astype(np.float64) * case["y64"]).sum()) + 1e-300
    assert abs(lhs - rhs) <= 1e-12 * scale, (lhs, rhs)


def test_weights_sum_to_one(case):
    s = case["a32"].astype(np.float64).sum(-1)
    assert np.abs(s - 1).max() <= case["k"] * 2.0 ** -23


def test_beta_one_adds_to_what_is_there(case):
    N, F = case["N"], case["F"]
    d0 = np.random.default_rng(9).random((N, F), dtype=np.float32)
    g = R.interp_bwd_f32(case["a32"], case["idx"], case["dy"], N)
    assert np.array_equal(R.interp_bwd_f32(case["a32"], case["idx"], case["dy"], N, dfeat0=d0), d0 + g)


def test_a_query_on_a_candidate_returns_its_feature_exactly():
    feat = np.random.default_rng(0).standard_normal((5, 8)).astype(np.float32)
    idx = np.array([[3], [0]], np.int32)
    dist = np.array([[0.0], [-1e-7]], np.float32)           # D = 0, and the small negative D the k-NN's cancellation can give
    a, y = R.interp_f32(feat, idx, dist, EPS)
    assert np.array_equal(a, np.ones((2, 1), np.float32)) and np.array_equal(y, feat[[3, 0]])


def test_nonfinite_distances():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    feat = np.arange(1, 25, dtype=np.float32).reshape(6, 4)
    idx = np.array([[0, 1, 2], [3, 4, 5], [1, 3, 5], [0, 2, 4]], np.int32)
    dist = np.array([[inf, inf, inf],                       # no finite distance: y = 0, nothing flows back
                     [0.25, nan, inf],                      # NaN counts as +inf: the whole weight on the first entry
                     [0.5, 0.5, nan],
                     [-inf, -1.0, 1e-20]], np.float32)      # D <= eps, negative and -inf included: 1 / eps each
    a, y = R.interp_f32(feat, idx, dist, EPS)
    assert np.array_equal(a[0], [0, 0, 0]) and np.array_equal(y[0], np.zeros(4, np.float32))
    assert np.array_equal(a[1], [1, 0, 0]) and np.array_equal(y[1], feat[3])
    assert np.array_equal(a[2], [0.5, 0.5, 0])
    assert a[3, 0] == a[3, 1] == a[3, 2] and abs(float(a[3].sum()) - 1) <= 3 * 2.0 ** -23
    assert np.isfinite(y).all()
    dy = np.ones((4, 4), np.float32)
    d = R.interp_bwd_f32(a, idx, dy, 6)
    only_row0 = R.interp_bwd_f32(a[1:], idx[1:], dy[1:], 6)
    assert np.array_equal(d, only_row0)                     # the all-inf row contributes nothing
    a64, y64 = R.interp_f64(feat, idx, dist, EPS)
    assert np.array_equal(a64[0], [0, 0, 0]) and np.array_equal(a64[1], [1, 0, 0])


def test_nonfinite_features_propagate():
    feat = np.array([[np.inf, 1, 2, 3], [1, 1, 1, 1]], np.float32)
    idx = np.array([[1, 0]], np.int32)
    dist = np.array([[0.5, np.inf]], np.float32)            # weight 0 on the infinite feature: 0 * inf = NaN, as the expression says
    a, y = R.interp_f32(feat, idx, dist, EPS)
    assert np.isnan(y[0, 0]) and np.array_equal(y[0, 1:], [1, 1, 1])


def test_tower_rows():
    idx = np.array([[[0, 2]], [[1, 0]]], np.int32)
    assert np.array_equal(R.tower_rows(idx, 3), [[0, 2], [4, 3]])

"""tests/knn_cross_reference.py, the yardstick of tests/test_gpu_knn_cross.py, against the oracle itself: with q = p the search between
two sets IS the self search, so cross_knn(x, x, k) must equal O.k_nn(x, k) on every row -- on exact ties, duplicates and every
non-finite family of tests/knn_nonfinite.py -- and its distances must be the oracle's distance matrix at the chosen indices."""
import numpy as np
import pytest

from oracle import dgcnn_oracle as O
import knn_cross_reference as R
import knn_nonfinite as NF


def check_self(x, k):
    idx, dist = R.cross_knn(x, x, k)
    np.testing.assert_array_equal(idx, O.k_nn(x[None], k)[0])
    with np.errstate(all="ignore"):
        D = O.dist_matrix_f32(x)
    Dt = np.where(np.isnan(D), np.float32(np.inf), D)
    np.testing.assert_array_equal(dist.view(np.uint32), np.take_along_axis(Dt, idx.astype(np.int64), -1).view(np.uint32))
    assert not np.isnan(dist).any() and (dist[:, 1:] >= dist[:, :-1]).all()                  # ascending, +inf and -inf included
    return idx, dist


@pytest.mark.parametrize("N,C,k", [(200, 3, 20), (257, 64, 40), (129, 192, 64), (300, 4, 1)])
def test_lattice_with_ties(N, C, k):
    x = (np.random.default_rng([N, C]).integers(-8, 9, (N, C)) * 0.25).astype(np.float32)
    idx, dist = check_self(x, k)
    if C <= 4 and k > 1:
        assert (dist[:, 1:] == dist[:, :-1]).any()                   # the lattice does produce equal distances


@pytest.mark.parametrize("N,C,k", [(200, 3, 20), (257, 64, 40), (129, 192, 64), (300, 4, 1)])
def test_random_rows(N, C, k):
    check_self(np.random.default_rng([N, C, 1]).standard_normal((N, C)).astype(np.float32), k)


def test_duplicates_follow_the_original():
    N, C, k = 150, 5, 8
    x = np.random.default_rng(3).standard_normal((N, C)).astype(np.float32)
    x[100:150] = x[0:50]
    idx, _ = check_self(x, k)
    assert (np.sort(idx[:50, :2], -1) == np.stack([np.arange(50), np.arange(100, 150)], -1)).all()


NONFINITE = [(f, 129, 5, 9) for f in NF.FAMILIES if NF._fits(f, 129, 5, 9)]
assert len(NONFINITE) == len(NF.FAMILIES)


@pytest.mark.parametrize("family,N,C,k", NONFINITE, ids=[c[0] for c in NONFINITE])
def test_non_finite_families(family, N, C, k):
    for label, x in NF.variants(family, N, C, k):
        idx, dist = check_self(np.asarray(x), k)
        assert all(len(set(r)) == k for r in idx.tolist()), (family, label)
        assert not np.isnan(dist).any()


def test_two_different_sets_against_plain_numpy():
    """M != N: the helper's index arithmetic (rows 0..M-1, candidates M..M+N-1) on integer data, where float64 numpy is exact."""
    q = np.random.default_rng(5).integers(-3, 4, (7, 3)).astype(np.float32)
    p = np.random.default_rng(6).integers(-3, 4, (11, 3)).astype(np.float32)
    idx, dist = R.cross_knn(q, p, 4)
    D = ((q[:, None, :].astype(np.float64) - p[None].astype(np.float64)) ** 2).sum(-1)
    np.testing.assert_array_equal(idx, np.argsort(D, -1, kind="stable")[:, :4])
    np.testing.assert_array_equal(dist, np.take_along_axis(D, idx.astype(np.int64), -1).astype(np.float32))
    with pytest.raises(ValueError):
        R.cross_knn(q, p, 12)

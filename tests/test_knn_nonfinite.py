"""The oracle's k-NN on non-finite input (oracle/knn_oracle.c, NON-FINITE INPUT), on the CPU: on every cloud that
tests/test_gpu_knn_nonfinite.py compares the kernels with,

  * O.k_nn (and the row routine O.k_nn_rows) equals a np.lexsort by (D~, j) over O.dist_matrix_f32, D~ = +inf where D is NaN -- the
    whole array, no tolerance: the rule is what the oracle computes, whichever candidates come first;
  * the cloud has the property its family is named for (knn_nonfinite.properties, on the oracle's own distance matrix);
  * every row holds k distinct indices of [0, N), and a row with a NaN coordinate holds 0 .. k - 1.

Before the rule the oracle filled its first k slots unconditionally and replaced only on d < bd[k - 1]: a NaN among the first k
candidates stayed for good (N = 40, k = 5, C = 3 with one NaN, one inf and one 1e20 point: 37 of 40 rows off the order)."""
import numpy as np
import pytest

from oracle import dgcnn_oracle as O
import knn_nonfinite as NF


def _ids(c):
    return "%s-N%d-C%d-k%d" % c


@pytest.mark.parametrize("family,N,C,k", NF.small_clouds(), ids=[_ids(c) for c in NF.small_clouds()])
def test_oracle_selects_by_the_total_order(family, N, C, k):
    for label, x in NF.variants(family, N, C, k):
        D = O.dist_matrix_f32(x)
        NF.properties(family, label, x, D, k)
        want = NF.rule_knn(D, k)
        got = O.k_nn(x[None], k)[0]
        np.testing.assert_array_equal(got, want, err_msg="%s (%s) %s" % (family, label, (N, C, k)))
        assert got.min() >= 0 and got.max() < N
        assert (np.diff(np.sort(got, 1), axis=1) > 0).all(), "a row lists an index twice"
        nanrow = np.flatnonzero(np.isnan(x).any(1))
        np.testing.assert_array_equal(got[nanrow], np.broadcast_to(np.arange(k, dtype=np.int32), (len(nanrow), k)))
        rows = np.unique(np.concatenate([NF.bad_rows(x), [0, N // 2, N - 1]])).astype(np.int32)
        np.testing.assert_array_equal(O.k_nn_rows(x, k, rows), want[rows], err_msg="row routine, %s (%s)" % (family, label))


def test_oracle_is_unchanged_on_finite_input():
    """The mapping touches NaN only: on finite clouds (ties, duplicates, a far offset) the oracle still equals a stable argsort of
    its own distance matrix."""
    rng = np.random.default_rng(5)
    for x in (rng.random((300, 3), dtype=np.float32), rng.integers(0, 4, (200, 4)).astype(np.float32),
              (rng.random((257, 20)) + 1000.0).astype(np.float32)):
        D = O.dist_matrix_f32(x)
        assert np.isfinite(D).all()
        np.testing.assert_array_equal(O.k_nn(x[None], 8)[0], np.argsort(D, axis=1, kind="stable")[:, :8].astype(np.int32))


def test_float64_twin_follows_the_same_rule():
    """O.k_nn on another dtype (numpy, stable sort) maps NaN to +inf as well: argsort alone would put every NaN after every +inf,
    whatever their j."""
    x = NF.base(40, 3).astype(np.float64)
    x[36, 2] = -np.inf                                           # at +inf from every finite point: sorts among the NaN points, by j
    x[3:34] = np.nan                                             # 31 NaN points: a finite row has < 8 finite candidates
    with np.errstate(invalid="ignore"):
        s = (x * x).sum(1)
        D = s[:, None] + s[None, :] - 2.0 * (x @ x.T)
        got = O.k_nn(x[None], 8)[0]
    assert np.isnan(D).any() and (D == np.inf).any()
    np.testing.assert_array_equal(got, NF.rule_knn(D, 8))


def test_big_cloud_has_its_bad_rows_in_the_sample():
    """The 8200-point clouds of the GPU module: sampled rows, the bad rows and their neighbours by index always among them."""
    N, C, k = NF.BIG_CLOUD
    for family in NF.FAMILIES:
        label, x = NF.variants(family, N, C, k)[0]
        rows = NF.sample_rows(x)
        bad = NF.bad_rows(x)
        near = np.clip(np.concatenate([bad[:64] - 1, bad[:64], bad[:64] + 1]), 0, N - 1)
        assert np.isin(near, rows).all() and len(rows) <= 1024 and (np.diff(rows) > 0).all(), family

"""Preconditions of tests/test_gpu_knn_adversarial.py, checked on the CPU against the oracle: conditions on the INPUTS (tests/
knn_adversarial.py), not measurements of the kernels.  The GPU tests compare indices only; without these a case could pass merely
because its cloud turned out tame.

  rounddown*   over the k true neighbours of every row the one-product filter's modelled (d' - d) / t is >= 0.75 * 2^-7 (the proof's
               bound is 2^-7 (1 + 2^-8), the filter tests with 2^-6); the largest modelled three-product value over true-neighbour
               pairs is >= 2^-16 (proof: < 2^-14, filter: 2^-13); at most 10 % of the rows have an exact tie at their k-th distance
               where the seed bound takes the width (C = 16, 32, 64): on at least 10 % of the rows the bound of the row's own graph,
               modelled in the bound kernel's summation order without its 2^-16 t of slack, is below the normative k-th distance
  offset       at least 90 % of the rows change their index list when d is evaluated in another summation order
  clusters     at least 10 % of the rows have a negative k-th distance and at least 10 % one of exactly zero

The achieved figures are printed, and the table is written to $DGCNN_KNN_ADVERSARIAL_TABLE when set (profiles/knn_adversarial.txt holds
a copy, with the GPU module's mutation table under it)."""
import os

import numpy as np
import pytest

from oracle import dgcnn_oracle as O
import knn_adversarial as A

FIGURES = {}             # (family, N, C, k) -> text of the achieved figures


def _oracle(x, k):
    return O.dist_matrix_f32(x), O.k_nn(x[None], k)[0]


def _note(family, N, C, k, text):
    FIGURES[(family, N, C, k)] = text
    print("%-17s N %4d C %3d k %2d  %s" % (family, N, C, k, text))


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    lines = ["# achieved figures of the preconditions of tests/test_knn_adversarial.py (CPU, against the oracle)",
             "# e1 = one-product filter's modelled (d' - d) / t over the k true neighbours of every row, in units of 2^-7 (needs min >= 0.75)",
             "# e3 = three-product filter's, in units of 2^-16 (needs max >= 1); tied = rows with an exact tie at the k-th distance (<= 10 %)",
             "# changed = rows whose list changes with the summation order (>= 90 %); kth<0, kth=0 = rows by k-th distance (>= 10 % each)"]
    for key in sorted(FIGURES, key=lambda q: (A.FAMILIES.index(q[0]), q[2], q[3], q[1])):
        lines.append("%-17s N %4d C %3d k %2d  %s" % (key + (FIGURES[key],)))
    text = "\n".join(lines) + "\n"
    print("\n" + text)
    path = os.environ.get("DGCNN_KNN_ADVERSARIAL_TABLE")
    if path:
        with open(path, "w") as f:
            f.write(text)


def test_bf16_emulation_rounds_to_nearest_even():
    v = np.array([0x3F800000, 0x3F807FFF, 0x3F808000, 0x3F808001, 0x3F818000, 0x3F817FFF, 0xBF808001, 0x00000000], np.uint32)
    want = np.array([0x3F800000, 0x3F800000, 0x3F800000, 0x3F810000, 0x3F820000, 0x3F810000, 0xBF810000, 0x00000000], np.uint32)
    np.testing.assert_array_equal(A.bf16_rne(v.view(np.float32)).view(np.uint32), want)
    rng = np.random.default_rng(0)
    a = rng.normal(size=1000).astype(np.float32)
    a1, a2 = A.split2(a)
    assert (np.abs(a.astype(np.float64) - a1) <= 2.0 ** -8 * np.abs(a)).all()                       # unit roundoff 2^-8 (half an ulp)
    assert (np.abs(a.astype(np.float64) - a1 - a2) <= 2.0 ** -16 * np.abs(a)).all()


def test_sq_norm_model_is_the_oracles():
    """d(zero row, j) = fl(0 + s_j) - 0: the oracle's own s_j, bit for bit."""
    x = A.make("offset100", 300, 20, 8)
    z = np.concatenate([x, np.zeros((1, x.shape[1]), np.float32)])
    np.testing.assert_array_equal(O.dist_matrix_f32(z)[-1, :-1], A.sq_norm_f32(x))


@pytest.mark.parametrize("family,N,C,k", A.all_clouds(("rounddown", "rounddown_scaled")))
def test_rounddown_clouds_drive_both_filters_toward_their_bounds(family, N, C, k):
    x = A.make(family, N, C, k)
    u = x.view(np.uint32)
    low = u & np.uint32(0xFFFF)
    assert (low >= 0x7000).all() and (low <= 0x7FFF).all() and (((u >> np.uint32(16)) & np.uint32(0x7F)) < 16).all()
    assert (np.sign(x) == np.sign(x[:1])).all()                                     # one sign per channel
    D, idx = _oracle(x, k)
    j = idx.astype(np.int64)
    e1 = np.take_along_axis(A.filter_error(x, D, 1), j, 1) * 2.0 ** 7
    e3 = np.take_along_axis(A.filter_error(x, D, 3), j, 1) * 2.0 ** 16
    st = A.kth_stats(D, idx)
    _note(family, N, C, k, "e1 min %.3f max %.3f   e3 min %.3f max %.3f   tied %4.1f %%" % (
        e1.min(), e1.max(), e3.min(), e3.max(), 100 * st["kth_tied"]))
    assert e1.min() >= 0.75
    assert e1.max() <= 1.0 + 2.0 ** -8                                               # (the model agrees with the proof's bound)
    assert e3.max() >= 1.0
    assert e3.max() < 4.0                                                            # (proof: < 2^-14 t)
    assert st["kth_tied"] <= 0.10
    if C in (16, 32, 64):
        # the seed bound's summation order, modelled, without its 2^-16 t of slack: with the row's own graph as seeds the bound would
        # lie BELOW the normative k-th distance on these rows -- the slack is what keeps their k-th neighbour
        low = float((A.seed_bound_distances(x, idx).max(1) < np.take_along_axis(D, j, 1)[:, -1]).mean())
        FIGURES[(family, N, C, k)] += "   slack-free seed bound under the k-th distance %4.1f %%" % (100 * low)
        print("   slack-free seed bound under the k-th distance: %4.1f %% of the rows" % (100 * low))
        assert low >= 0.10


@pytest.mark.parametrize("N,C,k", A.CASES)
def test_crossscale_cloud_has_true_neighbours_of_far_larger_norm(N, C, k):
    """Not under the 0.75 * 2^-7 condition above (a pair g scales apart has 2 p / t = 2^(g + 1) / (1 + 4^g) < 1, and the one-product
    error is 2 (p - p') / t): held to the same 0.75 * 2^-7 per unit of 2 p / t on every true-neighbour pair, and to what the family is
    for -- at least k / 2 rows (those of the smallest scales: only they run out of smaller points) have a true neighbour with
    s_j >= 3.9 s_i.  (The share of rows with a neighbour at s_j <= s_i / 3.9 is printed.)"""
    x = A.make("rounddown_crossscale", N, C, k)
    D, idx = _oracle(x, k)
    j = idx.astype(np.int64)
    s = A.sq_norm_f32(x).astype(np.float64)
    x64 = x.astype(np.float64)
    t = s[:, None] + s[j]
    w = 2.0 * np.einsum("ic,ikc->ik", x64, x64[j]) / t                                # 2 p / t per true-neighbour pair
    e1 = np.take_along_axis(A.filter_error(x, D, 1), j, 1) * 2.0 ** 7
    up = int(((s[j] / s[:, None]).max(1) >= 3.9).sum())
    down = float(((s[j] / s[:, None]).min(1) <= 1 / 3.9).mean())
    _note("rounddown_crossscale", N, C, k, "e1 min %.3f (min of e1 / (2p/t) %.3f)   rows with a true neighbour at s_j >= 3.9 s_i: %d, "
          "at s_j <= s_i / 3.9: %4.1f %%, largest s_j / s_i %.0f" % (e1.min(), (e1 / w).min(), up, 100 * down, (s[j] / s[:, None]).max()))
    assert (e1 >= 0.75 * w).all()
    assert up >= k // 2


@pytest.mark.parametrize("family,N,C,k", A.all_clouds(("offset8", "offset100")))
def test_offset_clouds_depend_on_the_summation_order(family, N, C, k):
    x = A.make(family, N, C, k)
    ref = O.k_nn(x[None], k)[0]
    changed = float((ref != A.other_order_knn(x, k)).any(1).mean())
    _note(family, N, C, k, "changed %5.1f %%" % (100 * changed))
    assert changed >= 0.90


@pytest.mark.parametrize("family,N,C,k", A.all_clouds(("clusters",)))
def test_cluster_clouds_have_non_positive_kth_distances(family, N, C, k):
    x = A.make("clusters", N, C, k)
    assert A.cluster_size(N, k) >= k + 8
    D, idx = _oracle(x, k)
    st = A.kth_stats(D, idx)
    _note("clusters", N, C, k, "kth<0 %4.1f %%  kth=0 %4.1f %%  a negative distance among the k %5.1f %%  self not first %5.1f %%  "
          "distinct values among the k %.1f" % (100 * st["kth_negative"], 100 * st["kth_zero"], 100 * st["any_negative"],
                                                100 * st["self_not_first"], st["distinct"]))
    assert st["kth_negative"] >= 0.10 and st["kth_zero"] >= 0.10
    # the seeds "k copies from the row's own cluster": k distinct rows whose distances are rounding noise (< 2^-18 t), so the seed
    # bound is its own slack, 2^-16 t, and nothing else.  (A bound <= 0 cannot come out of such rows: the kernel adds 2^-16 t and a
    # distance is never below -2^-19 t.  Only rows with t = 0, all-zero rows, reach tau0 = 0: zero_rows() below.)
    seeds = A.cluster_members(x, k)
    assert (np.sort(seeds, 1)[:, 1:] != np.sort(seeds, 1)[:, :-1]).all()
    s = A.sq_norm_f32(x)
    worst = np.take_along_axis(D, seeds.astype(np.int64), 1).max(1)
    assert (np.abs(worst) <= 2.0 ** -18 * 2 * s).all()


def test_zero_rows_are_the_only_way_to_a_seed_bound_of_zero():
    """zero_rows(): k + 8 all-zero rows inside an offset cloud.  Among themselves t = 0 and d = 0 exactly, so with their own graph as
    seeds tau0 = 0 + 2^-16 * 0 = 0: the threshold next_up(0), the smallest denormal, and the `T = 0` rule of the tightening."""
    for (N, C, k) in A.CASES:
        x, zr = A.zero_rows(N, C, k)
        D, idx = _oracle(x, k)
        assert len(zr) == k + 8 and (x[zr] == 0).all() and (D[np.ix_(zr, zr)] == 0).all()
        np.testing.assert_array_equal(idx[zr], np.broadcast_to(zr[:k], (len(zr), k)))          # the k lowest-numbered zero rows
        others = np.setdiff1d(np.arange(N), zr)
        assert (D[np.ix_(zr, others)] > 0).all()


@pytest.mark.parametrize("family,N,C,k", A.all_clouds(("mixed",)))
def test_mixed_cloud_holds_rows_of_every_family(family, N, C, k):
    """No condition of its own beyond its make-up: a quarter of the rows from each family, so a tile of 64 candidates holds operands
    of every kind, with s_i at least a hundred times apart (offset rows: C * 1e4, rounddown rows: below C * 73); the figures are printed."""
    x = A.make("mixed", N, C, k)
    assert x.shape == (N, C) and np.isfinite(x).all()
    D, idx = _oracle(x, k)
    st = A.kth_stats(D, idx)
    s = A.sq_norm_f32(x)
    _note("mixed", N, C, k, "kth<0 %4.1f %%  kth=0 %4.1f %%  tied %4.1f %%  s_i from %.3g to %.3g" % (
        100 * st["kth_negative"], 100 * st["kth_zero"], 100 * st["kth_tied"], s.min(), s.max()))
    assert s.max() / s.min() >= 100.0

"""CPU checks of the float32 restatement of farthest point sampling (tests/fps_reference.py, include/dgcnn_hip.h K7): against a
float64 brute force on coordinates where both are exact, and the properties the header states, on crafted inputs."""
import numpy as np
import pytest

import fps_reference as R

NAN, INF = np.float32(np.nan), np.float32(np.inf)
CASES = [(C, n, m) for C in (1, 3, 4, 5) for n in (1, 2, 63, 64, 65, 300) for m in sorted({1, n // 2, n}) if 1 <= m <= n]


@pytest.mark.parametrize("C,n,m", CASES, ids=["C%d-n%d-m%d" % c for c in CASES])
def test_equal_to_the_float64_brute_force_on_exact_coordinates(C, n, m):
    x = R.integer_cloud(n, C, 1000 * C + n)
    for start in (0, n - 1, n + 5):                      # the last one is out of range: counts as 0
        i32, d32 = R.fps_f32(x, m, start)
        i64, d64 = R.fps_f64(x, m, start)
        assert np.array_equal(i32, i64), (start, i32, i64)
        assert np.array_equal(d32.astype(np.float64), d64), start
        assert i32[0] == (start if start < n else 0) and d32[0] == INF
        assert len(set(i32.tolist())) == m


def test_duplicates_still_give_distinct_rows():
    x = np.tile(np.array([[1.0, 2.0, 3.0]], np.float32), (40, 1))
    idx, dist = R.fps_f32(x, 40)
    assert idx.tolist() == list(range(40))               # every row ties at mind = 0: ascending rows
    assert dist[0] == INF and (dist[1:] == 0).all()
    x[7] = [5.0, 5.0, 5.0]
    idx, dist = R.fps_f32(x, 40, start=3)
    assert idx[:2].tolist() == [3, 7] and sorted(idx.tolist()) == list(range(40))
    assert idx[2:].tolist() == [i for i in range(40) if i not in (3, 7)]


@pytest.mark.parametrize("bad", [(NAN, 0.0, 0.0), (0.0, INF, 0.0), (INF, 0.0, -INF)], ids=["nan", "inf", "both-infs"])
@pytest.mark.parametrize("pos", [0, 17, 49])
def test_a_bad_row_comes_after_every_finite_row_that_is_no_duplicate(bad, pos):
    rng = np.random.default_rng(3)
    good = rng.random((49, 3), dtype=np.float32)
    good[30] = good[4]                                    # one duplicate pair among the finite rows
    x = np.insert(good, pos, np.array(bad, np.float32), axis=0)
    start = 1 if pos == 0 else 0
    idx, dist = R.fps_f32(x, 50, start)
    where = {int(r): j for j, r in enumerate(idx)}
    assert sorted(where) == list(range(50))
    dup = [r if r < pos else r + 1 for r in (4, 30)]
    late = max(where[dup[0]], where[dup[1]])              # the second of the pair ties with the bad row at mind = 0
    assert where[pos] >= 48 and late >= 48
    assert (where[pos] < late) == (pos < [r for r in dup if where[r] == late][0])       # lower index first
    assert dist[where[pos]] == 0 and dist[late] == 0 and (dist[1:48] > 0).all()
    # the bad row does not disturb the others: without it the finite rows come in the same order
    ref, rd = R.fps_f32(good, 49, start - (1 if pos == 0 else 0))
    rest = [int(r) for r in idx if r != pos]
    assert [r if r < pos else r - 1 for r in rest] == ref.tolist()
    assert np.array_equal(np.delete(dist, where[pos]), rd)


def test_a_bad_start_row_leaves_the_rest_as_the_cloud_without_it():
    rng = np.random.default_rng(5)
    good = rng.random((33, 4), dtype=np.float32)
    x = np.insert(good, 9, np.array([NAN, INF, 0, 1], np.float32), axis=0)
    idx, dist = R.fps_f32(x, 34, start=9)
    assert idx[0] == 9 and dist[0] == 0                   # mind of a bad row as it stands: 0
    # nothing was lowered by the bad start: every finite row ties at +inf and row 0 wins -- the chain of the cloud without the bad row
    ref, rd = R.fps_f32(good, 33, start=0)
    assert [int(r) if r < 9 else int(r) - 1 for r in idx[1:]] == ref.tolist()
    assert np.array_equal(dist[1:], rd)


def test_lattice_ties_go_to_the_lower_index():
    x = R.lattice(4)                                      # 64 rows, row-major
    idx, dist = R.fps_f32(x, 64)
    i64, d64 = R.fps_f64(x, 64)
    assert np.array_equal(idx, i64) and np.array_equal(dist.astype(np.float64), d64)
    assert idx[0] == 0 and idx[1] == 63 and dist[1] == 27          # the opposite corner
    # step 2: the corners (0,3,3), (3,0,3), (3,3,0), (0,0,3) ... tie at 18; the lowest row among the tied wins
    tied = [r for r in range(64) if min(((x[r] - x[0]) ** 2).sum(), ((x[r] - x[63]) ** 2).sum()) == dist[2]]
    assert len(tied) > 1 and idx[2] == min(tied)
    assert len(set(idx.tolist())) == 64


def test_prefix_property():
    x = np.random.default_rng(7).random((200, 3), dtype=np.float32)
    full_i, full_d = R.fps_f32(x, 200, start=11)
    for m in (1, 2, 17, 100):
        i, d = R.fps_f32(x, m, start=11)
        assert np.array_equal(i, full_i[:m]) and np.array_equal(d, full_d[:m])
    assert (np.diff(full_d[1:]) <= 0).all()               # the coverage radius never grows


def test_overflowing_squares_lower_nothing():
    x = np.array([[0, 0, 0], [3e38, 0, 0], [1e20, 1e20, 0], [1, 0, 0], [-3e38, 0, 0]], np.float32)
    idx, dist = R.fps_f32(x, 5)
    assert sorted(idx.tolist()) == [0, 1, 2, 3, 4]
    assert idx[1] == 1 and dist[1] == INF                 # D(1, 0) overflows to +inf: row 1 keeps +inf and is the lowest such row
    assert np.isfinite(dist[-1]) and dist[-1] == 1


def test_a_packed_tower_equals_its_clouds_alone():
    rng = np.random.default_rng(9)
    sizes, counts, start = (1, 65, 300, 40), (1, 65, 7, 13), (0, 64, 5, 0)
    off = np.concatenate([[0], np.cumsum(sizes)])
    x = rng.random((off[-1], 3), dtype=np.float32)
    idx, dist = R.fps_packed(x, off, counts, start)
    assert idx.shape == (sum(counts),) and idx.dtype == np.int32
    p = 0
    for b, m in enumerate(counts):
        i, d = R.fps_f32(x[off[b]:off[b + 1]], m, start[b])
        assert np.array_equal(idx[p:p + m], i + off[b]) and np.array_equal(dist[p:p + m], d)
        p += m
    xd = rng.random((3, 50, 3), dtype=np.float32)
    di, dd = R.fps_dense(xd, 9)
    assert di.shape == (3, 9) and np.array_equal(R.tower_rows(di, 50)[9:18], R.fps_f32(xd[1], 9)[0] + 50)


def test_take_and_scatter_restatements():
    rng = np.random.default_rng(11)
    x = rng.standard_normal((20, 3)).astype(np.float32)
    rows = np.array([5, 0, 19, 7], np.int32)
    y = R.take_rows(x, rows)
    assert np.array_equal(y, x[[5, 0, 19, 7]])
    d0 = rng.standard_normal((20, 3)).astype(np.float32)
    g0, g1 = R.scatter_rows(y, rows, 20), R.scatter_rows(y, rows, 20, d0)
    assert np.array_equal(g0[rows], y) and (np.delete(g0, rows, 0) == 0).all()
    assert np.array_equal(g1[rows], d0[rows] + y) and np.array_equal(np.delete(g1, rows, 0), np.delete(d0, rows, 0))

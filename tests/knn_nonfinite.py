"""Clouds with non-finite coordinates, and finite ones whose squares or sums overflow, for the k-NN (csrc/knn.hip, csrc/knn_grid.hip).
numpy only; after the pattern of tests/knn_adversarial.py.

The rule the kernels and the oracle share (oracle/knn_oracle.c, include/dgcnn_hip.h K1): the key of candidate j for row i is
(D~_ij, j), D~ = +inf where the normative D_ij is NaN and D_ij otherwise; idx[i] = the k smallest keys, ascending, ties to the lower j.

Every family is ordinary uniform points in [0, 1)^C with a few BAD points.  Where a family has a free choice of positions they come
from positions(N): row 0 (a member of the first k candidates, which the oracle's insert once kept for good), one even and one odd
index (both parities of a sample stride), 63 and 64 (the 64-row block edge, the last lane of a wave and the first of the next) and
N - 1 (the last row, the ragged tile).  A family is a list of VARIANTS (label, cloud): the same idea with the bad points and
channels moved.

  nan_one       one NaN in one point; over the variants the point walks through positions(N) and the channel through 0, C - 1 (the
                last real channel of a zero-padded tile) and C // 2
  hist_trap     m in {1, 3, k} NaN points at multiples of 4 -- every sample stride of knn_hist_bound_kernel (1, 2, 4) meets all of
                them; a NaN distance counted below a bin edge makes the bound drop true neighbours of EVERY row of the cloud
  inf           one point with +inf, one with -inf, one with both signs in different channels (C >= 2)
  sq_overflow   finite coordinates of +-1e20: s_i = +inf; p finite against ordinary points (D = +inf), +-inf among themselves (D NaN or +inf)
  sum_overflow  one coordinate of 1.5e19 in a few points: s_i = 2.25e38 is finite, but between two of them s_i + s_j and 2 p both
                overflow: D = inf - inf = NaN, also for the point itself -- a finite row that does not list itself
  few_finite    all but k // 2 points bad (NaN and 1e20 alternating: NaN and +inf distances, which sort TOGETHER by j): every finite
                row lists the finite points, then bad ones, lowest j first
  all_bad       every point holds a NaN: every row is 0 .. k - 1

properties(family, D, k, ...) asserts on the oracle's distance matrix that a cloud is what its family's name says, so that an edit
of a builder cannot empty the tests built on it."""
import numpy as np

FAMILIES = ("nan_one", "hist_trap", "inf", "sq_overflow", "sum_overflow", "few_finite", "all_bad")
BIG = np.float32(1e20)            # BIG * BIG overflows
HALF = np.float32(1.5e19)         # HALF * HALF = 2.25e38 is finite, twice that is not


def positions(N):
    """Row 0, an even and an odd index, 63, 64, N - 1 -- those below N, ascending, distinct."""
    return sorted({p for p in (0, 20, 37, 63, 64, N - 1) if 0 <= p < N})


def base(N, C, seed=0):
    return np.random.default_rng([seed, N, C, 11]).random((N, C), dtype=np.float32)


def _channels(C):
    return sorted({0, C - 1, C // 2})


def nan_one(N, C, k, seed=0):
    out = []
    ch = _channels(C)
    for v, p in enumerate(positions(N)):
        x = base(N, C, seed)
        c = ch[v % len(ch)]
        x[p, c] = np.nan
        out.append(("point %d channel %d" % (p, c), x))
    return out


def trap_rows(N, m):
    """m multiples of 4: 0, 64, the last one below N, then 20 and every further one from 4 up."""
    first = [p for p in (0, 64, 4 * ((N - 1) // 4), 20) if p < N]
    rows = []
    for p in first + list(range(4, N, 4)):
        if p not in rows:
            rows.append(p)
    assert len(rows) >= m, "hist_trap: N = %d has no %d multiples of 4" % (N, m)
    return sorted(rows[:m])


def hist_trap(N, C, k, seed=0):
    out = []
    for m in (1, 3, k):
        x = base(N, C, seed)
        for t, p in enumerate(trap_rows(N, m)):
            x[p, t % C] = np.nan
        out.append(("%d NaN points" % m, x))
    return out


def inf(N, C, k, seed=0):
    out = []
    P = positions(N)
    for v in range(2):
        x = base(N, C, seed)
        a, b = (P[0], P[-1]) if v == 0 else (P[-1], P[len(P) // 2 - 1])
        c = next(p for p in (P[::-1] if v == 0 else P) + list(range(N)) if p not in (a, b))
        x[a, 0] = np.inf
        x[b, C - 1] = -np.inf
        if C >= 2:
            x[c, 0] = np.inf
            x[c, C - 1] = -np.inf
        out.append(("+inf at %d, -inf at %d, both at %d" % (a, b, c), x))
    return out


def sq_overflow(N, C, k, seed=0):
    P = positions(N)
    x = base(N, C, seed)
    for t, p in enumerate(P):
        x[p, _channels(C)[t % len(_channels(C))]] = BIG
    y = base(N, C, seed)
    for t, p in enumerate(P):                                  # both signs: p = -inf between two of them, D = +inf, not NaN
        y[p, 0] = BIG if t % 2 == 0 else -BIG
    return [("1e20", x), ("+-1e20 in channel 0", y)]


def sum_overflow(N, C, k, seed=0):
    x = base(N, C, seed)
    for p in positions(N):
        x[p, C - 1] = HALF
    return [("1.5e19 in the last channel", x)]


def finite_rows(N, k):
    """The k // 2 finite points of few_finite: spread over the index range, none at positions(N)."""
    f = max(1, k // 2)
    bad = set(positions(N))
    rows = []
    for p in np.linspace(1, N - 2, f).astype(int):
        while p in bad or p in rows:
            p += 1
        rows.append(int(p))
    assert len(rows) == f and max(rows) < N
    return sorted(rows)


def few_finite(N, C, k, seed=0):
    x = base(N, C, seed)
    fin = set(finite_rows(N, k))
    for p in range(N):
        if p not in fin:
            x[p, p % C] = np.nan if p % 2 == 0 else BIG
    return [("%d finite points" % len(fin), x)]


def all_bad(N, C, k, seed=0):
    x = base(N, C, seed)
    x[np.arange(N), np.arange(N) % C] = np.nan
    return [("a NaN in every point", x)]


_CACHE = {}


def variants(family, N, C, k, seed=0):
    """[(label, cloud (N, C) float32)] of a family at a shape; built once per process and read-only."""
    key = (family, N, C, k, seed)
    if key not in _CACHE:
        if family not in FAMILIES:
            raise ValueError(family)
        out = globals()[family](N, C, k, seed)
        for _, x in out:
            assert x.shape == (N, C) and x.dtype == np.float32
            x.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------
# the rule, restated with numpy on the oracle's distance matrix
# ------------------------------------------------------------------------------------------------
def rule_knn(D, k):
    """(N, k) int32: the k smallest (D~, j) of every row of D (N, N), D~ = +inf where D is NaN."""
    Dt = np.where(np.isnan(D), np.float32(np.inf), D)
    j = np.broadcast_to(np.arange(len(D)), D.shape)
    return np.lexsort((j, Dt), axis=-1)[:, :k].astype(np.int32)       # last key first: by D~, then by j


def bad_rows(x):
    """Rows of x with a coordinate that is not finite or whose square overflows, and rows of sum_overflow's kind (|v| >= 1e19)."""
    return np.flatnonzero((~np.isfinite(x) | (np.abs(x) >= np.float32(1e19))).any(1))


def sample_rows(x, n=512):
    """Query rows of a large cloud to check against the oracle's row routine: n random ones, and ALWAYS the bad rows (the first 64 of
    them where nearly every row is bad) with their neighbours by index, rows 0 and N - 1."""
    N = len(x)
    bad = bad_rows(x)[:64]
    rows = np.concatenate([np.random.default_rng(N).choice(N, n, replace=False), bad - 1, bad, bad + 1, [0, N - 1]])
    return np.unique(np.clip(rows, 0, N - 1)).astype(np.int32)


def properties(family, label, x, D, k):
    """Assert that the cloud x with the oracle's distance matrix D has the property its family is named for."""
    N, C = x.shape
    nanrow = np.isnan(x).any(1)
    fin_lt = (D < np.inf).sum(1)                               # candidates below +inf per row (NaN fails the comparison)
    what = "%s (%s) %s" % (family, label, (N, C, k))
    if family == "nan_one":
        assert np.isnan(x).sum() == 1, what
        r = int(np.flatnonzero(nanrow)[0])
        assert r in positions(N) and np.isnan(D[r]).all() and np.isnan(D[:, r]).all(), what
        assert (fin_lt[np.arange(N) != r] == N - 1).all(), what
    elif family == "hist_trap":
        rows = np.flatnonzero(nanrow)
        assert len(rows) in (1, 3, k) and (rows % 4 == 0).all() and rows[0] == 0, what     # sampled by strides 1, 2 and 4
        assert np.isnan(D[:, rows]).all(), what
        assert np.isfinite(np.delete(np.delete(D, rows, 0), rows, 1)).all(), what
        assert N - len(rows) >= k, what                        # every finite row still has k finite candidates
    elif family == "inf":
        assert (x == np.inf).any() and (x == -np.inf).any() and not np.isnan(x).any(), what
        rows = np.flatnonzero(~np.isfinite(x).all(1))
        assert 2 <= len(rows) <= 3, what
        if C >= 2:
            assert any((x[r] == np.inf).any() and (x[r] == -np.inf).any() for r in rows), what
        ok = np.setdiff1d(np.arange(N), rows)
        assert not (D[np.ix_(ok, rows)] < np.inf).any(), what  # an infinite point is at +inf or NaN from every finite one
        assert np.isnan(D[rows, rows]).all(), what
    elif family == "sq_overflow":
        assert np.isfinite(x).all(), what
        rows = np.flatnonzero((np.abs(x) >= BIG).any(1))
        assert list(rows) == positions(N), what
        with np.errstate(over="ignore"):
            s = (x.astype(np.float32) ** 2).sum(1, dtype=np.float32)
        assert (s[rows] == np.inf).all(), what
        ok = np.setdiff1d(np.arange(N), rows)
        assert (D[np.ix_(ok, rows)] == np.inf).all(), what     # s_i = inf, p finite
        assert not (D[np.ix_(rows, rows)] < np.inf).any(), what
        if len(rows) > 1:
            among = D[np.ix_(rows, rows)]
            assert np.isnan(among).any(), what
            if "+-" in label:
                assert (among == np.inf).any(), what           # opposite signs: p = -inf, D = +inf
    elif family == "sum_overflow":
        assert np.isfinite(x).all(), what
        rows = np.flatnonzero((np.abs(x) >= np.float32(1e19)).any(1))
        assert list(rows) == positions(N), what
        s = (x.astype(np.float32) ** 2).sum(1, dtype=np.float32)
        assert np.isfinite(s).all(), what                      # s_i is finite ...
        assert np.isnan(D[rows, rows]).all(), what             # ... the self-distance is NaN
        assert np.isnan(D[np.ix_(rows, rows)]).all(), what
        ok = np.setdiff1d(np.arange(N), rows)
        assert np.isfinite(D[np.ix_(rows, ok)]).all(), what    # and the distance to an ordinary point finite
    elif family == "few_finite":
        fin = np.flatnonzero(np.isfinite(x).all(1) & (np.abs(x) < BIG).all(1))
        assert list(fin) == finite_rows(N, k) and len(fin) < k and N - len(fin) > N - k, what
        assert (fin_lt[fin] == len(fin)).all() and (fin_lt[fin] < k).all(), what           # fewer than k finite distances
        assert np.isnan(D[fin]).any() and (D[fin] == np.inf).any(), what                   # both kinds of D~ = +inf among the rest
        assert set(positions(N)).isdisjoint(fin), what
    elif family == "all_bad":
        assert nanrow.all() and np.isnan(D).all(), what
    else:
        raise ValueError(family)


# ------------------------------------------------------------------------------------------------
# the shapes both test modules use
# ------------------------------------------------------------------------------------------------
# (N, k): two blocks and a ragged third, five blocks and a ragged sixth, eleven blocks at the 20-entry lists
SHAPES = ((200, 8), (333, 8), (700, 20))
FEW_SHAPE = (40, 20)                                           # few_finite: one block, k = N / 2
# raw coordinates below 256 points run without the histogram bound (knn.hip: knn_hist_stride), from 256 on with it where
# N >= 4 k stride: (128, 8) is the smallest shape that meets the second rule at stride 4, (256, 8) the smallest that meets both
HIST_SHAPES = ((128, 8), (256, 8))
C_RAW = (3, 4)
C_VALU = (16, 20, 128)
C_MFMA = (16, 20, 48, 64)
C_BF16F = (20, 48, 64)
C_SEEDED = (16, 32, 64)
C_APPEND = (32, 64)
C_GRID = (1, 2, 3, 4)
GRID_N = (5, 300, 777, 2048)
BIG_CLOUD = (8200, 64, 20)                                     # knn_bf16a_kernel<false, ..>: past 8192 points


def shapes_of(family):
    return SHAPES + ((FEW_SHAPE,) if family == "few_finite" else ())


def grid_k(N):
    return 3 if N == 5 else 8 if N == 300 else 20


def small_clouds():
    """Every (family, N, C, k) that the GPU module checks on ALL rows: the CPU module pins the oracle on each of them."""
    out = []
    for f in FAMILIES:
        for N, k in shapes_of(f):
            out += [(f, N, C, k) for C in sorted(set(C_RAW + C_VALU + C_MFMA + C_BF16F + C_SEEDED + C_APPEND))]
        out += [(f, N, C, k) for N, k in HIST_SHAPES for C in C_RAW]
        out += [(f, N, C, grid_k(N)) for N in GRID_N for C in C_GRID if not (f == "hist_trap" and N == 5)]
        out += [(f, 2048, 3, 40)]
    out += [("hist_trap", 2048, 3, 20)]
    seen, uniq = set(), []
    for c in out:
        if c not in seen and _fits(*c):
            seen.add(c)
            uniq.append(c)
    return uniq


def _fits(family, N, C, k):
    """hist_trap needs k multiples of 4 and k finite points besides; few_finite k // 2 free rows."""
    if family == "hist_trap":
        return (N + 3) // 4 >= k and N - k >= k
    return N >= k and N >= 5

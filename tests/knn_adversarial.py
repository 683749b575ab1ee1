"""Adversarial operands for the feature-space k-NN (csrc/knn.hip) and a CPU model of its approximate filters.  numpy only.

The kernels promise the oracle's indices bit for bit; the bf16 filters in front of the exact re-check, the seed bound and the code for
distances <= 0 rest on proofs in the kernel comments.  The builders below make the clouds those proofs are about:

  rounddown          every coordinate +-2^e_c (1 + m / 128 + low / 2^23): sign and exponent fixed per channel (every product of two
                     points is positive), m < M_MAX (a small leading mantissa: the relative bf16 error stays near 2^-8), low just under
                     the bf16 tie, and low's last seven bits just under the tie of the SECOND bf16 term.  Both operands of every product
                     round toward zero, so the filters' inner products are too small by nearly the whole bound, on every pair.
  rounddown_scaled   the same cloud with every point multiplied by 2^g: a power of two keeps every mantissa, so the roundings are the
                     same while s_i spans 2^24 inside one tile.  Every scale holds at least k + 8 points (the true neighbours of a row
                     share its scale: a neighbour of another scale has 2 p < 0.8 t, which would take the error below the precondition).
  rounddown_crossscale   the same over 13 scales with too few points at the small ones: true neighbours with s_j = 4 s_i and more.
  offset             offset + sigma * normal: cancellation, d << t, the order of the neighbours depends on the last bits of s_i and p.
  clusters           near-duplicate clusters at a large offset: distances that are rounding noise around zero -- negative, exactly
                     zero, a handful of distinct values per row, self not first; the index decides the order.
  mixed              one cloud with rows of all of the above.

filter_error models the filters' inner products (bf16 round-to-nearest-even on the uint32 view, products and sums in float64: the fp32
accumulation is covered by the proofs' own constants and is not what is probed) and returns (d' - d) / t per pair.
"""
import numpy as np

M_MAX = 8            # leading mantissa values of `rounddown` (m < 8: few exact ties at the k-th distance; m < 16 still rounds the same way)


# ------------------------------------------------------------------------------------------------
# bf16
# ------------------------------------------------------------------------------------------------
def bf16_rne(a):
    """float32 -> the nearest bf16 (ties to even) as float32; finite inputs."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def split2(a):
    """a -> (a1, a2) = (bf16(a), bf16(a - a1)); a - a1 is exact in fp32."""
    a = np.ascontiguousarray(a, np.float32)
    a1 = bf16_rne(a)
    return a1, bf16_rne(a - a1)


# ------------------------------------------------------------------------------------------------
# builders: (N, C, k, seed, ...) -> (N, C) float32
# ------------------------------------------------------------------------------------------------
def rounddown(N, C, k=20, seed=0, m_max=M_MAX):
    rng = np.random.default_rng([seed, N, C, 1])
    sign = rng.integers(0, 2, C).astype(np.uint32) << np.uint32(31)
    expo = (rng.integers(-3, 4, C) + 127).astype(np.uint32) << np.uint32(23)
    m = rng.integers(0, m_max, (N, C)).astype(np.uint32) << np.uint32(16)
    # low = 0x7000 | five free bits << 7 | 0x30 ... 0x3F: in [0x7000, 0x7FFF], under the tie of the first bf16 term (0x8000) and, its
    # last seven bits, under the tie of the second (0x40)
    low = (np.uint32(0x7000) | (rng.integers(0, 32, (N, C)).astype(np.uint32) << np.uint32(7))
           | rng.integers(0x30, 0x40, (N, C)).astype(np.uint32))
    return (sign[None] | expo[None] | m | low).view(np.float32)


def scale_levels(N, k):
    """The exponents g of rounddown_scaled: as many levels in [-6, 6] as leave k + 8 points to each (at most 13)."""
    L = int(max(1, min(13, N // (k + 8))))
    return np.round(np.linspace(-6, 6, L)).astype(np.int64) if L > 1 else np.array([6], np.int64)


def rounddown_scaled(N, C, k=20, seed=0, m_max=M_MAX):
    x = rounddown(N, C, k, seed, m_max)
    rng = np.random.default_rng([seed, N, C, 2])
    lv = scale_levels(N, k)
    g = lv[rng.permutation(N) % len(lv)]                       # balanced: every level gets N // L points or one more
    return (x * np.exp2(g)[:, None].astype(np.float32)).astype(np.float32)


def rounddown_crossscale(N, C, k=20, seed=0, m_max=M_MAX):
    """The rounddown cloud over all 13 scales 2^-6 ... 2^6, with only k / 4 points at each of the six smallest (the other seven share
    the rest).  A point one scale DOWN is at d = s_i / 4, one scale UP at d = s_i: a row takes smaller points first, and goes up only
    when fewer than k points are at its scale and below -- here the rows of the three smallest scales, about 3 k / 4 rows, whose true
    neighbours then have s_j = 4 s_i ... 64 s_i: the pairs on which a margin applied to s_i alone instead of t = s_i + s_j is too
    small.  The other rows of the thin scales have true neighbours with s_j = s_i / 4 and less.  Kept apart from rounddown_scaled: on a
    pair g levels apart 2 p / t = 2^(g + 1) / (1 + 4^g), so the one-product error is 0.8 (g = 1), 0.47 (g = 2) ... of what it is
    inside a scale."""
    x = rounddown(N, C, k, seed, m_max)
    rng = np.random.default_rng([seed, N, C, 7])
    few = max(1, k // 4)
    assert N > 6 * few + 7, "rounddown_crossscale: N = %d is too small for k = %d" % (N, k)
    g = np.concatenate([np.repeat(np.arange(-6, 0), few), np.arange(N - 6 * few) % 7])[rng.permutation(N)]
    return (x * np.exp2(g)[:, None].astype(np.float32)).astype(np.float32)


def offset(N, C, k=20, seed=0, off=100.0, sigma=None):
    """sigma defaults to off / 1024: d / t ~ 2^-20, so the fp32 roundings of s_i, p and d (~ 2^-22 t) are a good part of d, far more
    than the spacing of a row's nearest distances (tuned on the CPU: with off / 128 only 12 % of the rows of a (300, 20) cloud
    change their k = 8 list with the summation order, with off / 512 80 %, with off / 1024 92 % or more at every shape of CASES;
    from off / 2048 on half of the k-th distances are exactly zero -- that is the `clusters` family)."""
    rng = np.random.default_rng([seed, N, C, 3])
    sigma = off / 1024.0 if sigma is None else sigma
    return (off + sigma * rng.normal(size=(N, C))).astype(np.float32)


def cluster_size(N, k):
    """Points per cluster: 2 k + 20 (>= k + 8), or N / 12 where that is more.  Tuned on the CPU: with k + 8 points per cluster the k-th
    neighbour is nearly the farthest point of the cluster and its distance is positive (300 points, C = 64, k = 64: no negative k-th
    distance, 6 % zero; with 2 k + 20: 45 % and 43 %); the spread hardly matters between 5e-6 and 1e-4."""
    return int(max(2 * k + 20, N // 12))


def clusters(N, C, k=20, seed=0, off=100.0, spread=2e-5, size=None):
    """Near-copies of N // size centres (the last cluster takes the remainder): centre = off + normal, point = centre (1 + spread *
    normal).  Rows of a cluster are interleaved with the others' (index order is not cluster order)."""
    rng = np.random.default_rng([seed, N, C, 4])
    size = cluster_size(N, k) if size is None else size
    G = max(1, N // size)
    centre = off + rng.normal(size=(G, C))
    member = np.minimum(np.arange(N) // size, G - 1)[rng.permutation(N)]
    return (centre[member] * (1.0 + spread * rng.normal(size=(N, C)))).astype(np.float32)


def zero_rows(N, C, k=20, seed=0):
    """(cloud, rows): an offset-8 cloud in which k + 8 rows, spread over the index range, are all zero.  Between two of them s_i, p, t
    and d are exactly 0 -- the only pairs for which a seed bound (max d + 2^-16 t) can be <= 0."""
    x = offset(N, C, k, seed, off=8.0).copy()
    rows = np.sort(np.random.default_rng([seed, N, C, 6]).permutation(N)[:k + 8])
    x[rows] = 0.0
    return x, rows


def cluster_members(x, k):
    """(N, k) int32: k rows of every row's own cluster (its k nearest in float64, self included) -- seeds at distance ~0."""
    x64 = x.astype(np.float64)
    s = (x64 * x64).sum(1)
    D = s[:, None] + s[None, :] - 2.0 * (x64 @ x64.T)
    return np.argsort(D, axis=1, kind="stable")[:, :k].astype(np.int32)


def mixed(N, C, k=20, seed=0, spread=2e-5):
    """A quarter of the rows from each family (clusters: the remainder), shuffled into one cloud; every part holds >= k + 8 rows."""
    q = N // 4
    assert q >= k + 8, "mixed: N = %d is too small for k = %d" % (N, k)
    parts = [rounddown(q, C, k, seed), rounddown_scaled(q, C, k, seed + 1), offset(q, C, k, seed, off=100.0),
             clusters(N - 3 * q, C, k, seed, spread=spread)]
    rng = np.random.default_rng([seed, N, C, 5])
    return np.concatenate(parts, 0)[rng.permutation(N)]


# ------------------------------------------------------------------------------------------------
# the filters' error, modelled
# ------------------------------------------------------------------------------------------------
def sq_norm_f32(x):
    """s_i in the oracle's arithmetic: sequential fp32 sum of fl(x * x)."""
    x = np.ascontiguousarray(x, np.float32)
    s = np.zeros(len(x), np.float32)
    for c in range(x.shape[1]):
        s = s + x[:, c] * x[:, c]
    return s


def filter_error(x, D, products):
    """(d' - d) / t for every pair of the cloud x (N, C): d = D, the oracle's distances (O.dist_matrix_f32(x)); t = fl(s_i + s_j);
    d' = t - 2 p', p' = a1.q1 (products = 1) or a1.q1 + a1.q2 + a2.q1 (products = 3) in float64."""
    a1, a2 = split2(x)
    h, m = a1.astype(np.float64), a2.astype(np.float64)
    p = h @ h.T
    if products == 3:
        hm = h @ m.T
        p = p + hm + hm.T
    elif products != 1:
        raise ValueError(products)
    s = sq_norm_f32(x)
    t = (s[:, None] + s[None, :]).astype(np.float32).astype(np.float64)
    return (t - 2.0 * p - D.astype(np.float64)) / t


def _fma32(a, b, c):
    """fl32(a * b + c) for float32 arrays: the product is exact in float64, the sum is rounded twice (53 bits, then 24) -- equal to the
    fused result except on rare double-rounding ties, which a share of rows does not notice."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def seed_bound_distances(x, seeds):
    """d~(i, seeds[i][m]) in the summation order of knn_seed_bound_kernel, WITHOUT its 2^-16 t of slack: per lane four channels
    (one product, three fmas), a butterfly over the C / 4 lanes of the pair, then fl(t - 2 p).  C in {16, 32, 64}."""
    x = np.ascontiguousarray(x, np.float32)
    N, C = x.shape
    assert C in (16, 32, 64)
    j = seeds.astype(np.int64)
    a = x[:, None, :].reshape(N, 1, C // 4, 4)
    v = x[j].reshape(N, j.shape[1], C // 4, 4)
    p = a[..., 0] * v[..., 0]
    for c in (1, 2, 3):
        p = _fma32(np.broadcast_to(a[..., c], v[..., c].shape), v[..., c], p)
    while p.shape[-1] > 1:                                     # lanes l and l ^ o, o = 1, 2, 4, ...: neighbours first
        p = p[..., 0::2] + p[..., 1::2]
    p = p[..., 0]
    s = sq_norm_f32(x)
    t = s[:, None] + s[j]
    return _fma32(np.float32(-2.0) * np.ones_like(p), p, t)


def kth_stats(D, idx):
    """Of the oracle's distances D (N, N) and lists idx (N, k): the share of rows whose k-th distance is negative / exactly zero /
    tied exactly with the (k + 1)-th, whose list holds a negative distance, whose first entry is not the row itself; and the mean
    number of distinct distance values among a row's k."""
    N, k = idx.shape
    dk = np.take_along_axis(D, idx.astype(np.int64), 1)
    kth = dk[:, -1]
    tie = ((D == kth[:, None]).sum(1) + (D < kth[:, None]).sum(1) > k) if k < N else np.zeros(N, bool)
    return {"kth_negative": float((kth < 0).mean()), "kth_zero": float((kth == 0).mean()), "kth_tied": float(tie.mean()),
            "any_negative": float((dk < 0).any(1).mean()), "self_not_first": float((idx[:, 0] != np.arange(N)).mean()),
            "distinct": float(np.mean([len(np.unique(r)) for r in dk]))}


def other_order_knn(x, k):
    """The k-NN lists with d evaluated in another summation order: numpy fp32 (x * x).sum(1) and x @ x.T, the oracle's formula and
    tie rule (stable sort)."""
    x = np.ascontiguousarray(x, np.float32)
    s = (x * x).sum(1)
    D = (s[:, None] + s[None, :]) - np.float32(2.0) * (x @ x.T)
    return np.argsort(D, axis=1, kind="stable")[:, :k].astype(np.int32)


# ------------------------------------------------------------------------------------------------
# the cases both test modules use: every (family, N, C, k) below meets the preconditions of tests/test_knn_adversarial.py
# ------------------------------------------------------------------------------------------------
FAMILIES = ("rounddown", "rounddown_scaled", "rounddown_crossscale", "offset8", "offset100", "clusters", "mixed")
# N in {300, 512, 1000}; every list size class (k <= 8, 20, 40, 64); C = 20 and 48 run the zero-padded channels of the 64-wide tile,
# C = 16 / 32 / 64 are the widths the seed bound takes, C = 128 the widest VALU form
CASES = ((512, 64, 20), (300, 20, 8), (1000, 48, 40), (300, 64, 64), (512, 16, 20), (300, 128, 20), (1000, 64, 40), (300, 32, 8))

# packed towers (C, k): one cloud of each family, unaligned sizes (130, 257, 600, k + 8), neighbouring clouds 2^+-12 apart in norm
TOWER_SHAPES = ((64, 20), (20, 8), (128, 40), (16, 64), (32, 8), (64, 40), (64, 64))


def tower_spec(C, k):
    """[(family, N, power-of-two factor)] of the tower of a shape: the rounddown cloud scaled by 2^-12 sits next to the offset-100
    cloud (s_i ~ 1e-5 next to 1e6); the cloud of k + 8 points is the smallest a search for k admits with a margin."""
    big = 600 if 257 // 4 < k + 8 else 257                     # `mixed` needs N / 4 >= k + 8
    return [("rounddown", 130 if k + 8 <= 130 else 257, -12), ("offset100", 257, 0), ("clusters", 600, 0), ("rounddown_scaled", k + 8, 0),
            ("offset8", 130 if 2 * k <= 130 else 257, 0), ("mixed", big, 0)]


def tower(C, k):
    """-> [cloud (N_b, C) float32] of tower_spec(C, k)."""
    return [(make(f, n, C, k) * np.float32(2.0 ** g)).astype(np.float32) for f, n, g in tower_spec(C, k)]


def all_clouds(families):
    """Every (family, N, C, k) the GPU module feeds, of the given families: CASES and the towers' clouds."""
    out = [(f, N, C, k) for f in FAMILIES for (N, C, k) in CASES]
    for C, k in TOWER_SHAPES:
        out += [(f, n, C, k) for f, n, _ in tower_spec(C, k)]
    seen, uniq = set(), []
    for c in out:
        if c[0] in families and c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


_CACHE = {}


def make(family, N, C, k, seed=0):
    """The cloud of a family at a shape, (N, C) float32; built once per process and read-only."""
    key = (family, N, C, k, seed)
    if key not in _CACHE:
        if family == "offset8":
            x = offset(N, C, k, seed, off=8.0)
        elif family == "offset100":
            x = offset(N, C, k, seed, off=100.0)
        elif family in ("rounddown", "rounddown_scaled", "rounddown_crossscale", "clusters", "mixed"):
            x = globals()[family](N, C, k, seed)
        else:
            raise ValueError(family)
        x.setflags(write=False)
        _CACHE[key] = x
    return _CACHE[key]

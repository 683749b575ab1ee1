"""The expected result of farthest point sampling and of the row take (csrc/fps.hip), restated from the normative arithmetic of
include/dgcnn_hip.h K7; numpy only, no kernel code.

fps_f32 performs every difference, product and sum in float32, one rounding each, in the header's order -- what the kernels must
reproduce bit for bit, one cloud at a time; fps_packed applies it to the clouds of a tower.  fps_f64 is a brute force in float64 that
keeps no running minimum: it recomputes every row's distance to every selected row at every step -- the yardstick of
tests/test_fps_reference.py for the float32 restatement itself (on integer-valued coordinates both are exact)."""
import numpy as np

F32 = np.float32
INF = np.float32(np.inf)


def sqdist_f32(x, s):
    """D(i, s) of every row i of x (n, C) float32: the header's expression, channel by channel ascending"""
    with np.errstate(all="ignore"):
        t = x[:, 0] - x[s, 0]
        D = t * t
        for c in range(1, x.shape[1]):
            t = x[:, c] - x[s, c]
            D = D + t * t
    assert D.dtype == np.float32
    return D


def fps_f32(x, m, start=0):
    """(idx (m,) int32 cloud-local, dist (m,) float32) of one cloud x (n, C)"""
    x = np.ascontiguousarray(x, F32)
    n = x.shape[0]
    assert 1 <= m <= n
    mind = np.where(np.isfinite(x).all(1), INF, F32(0)).astype(F32)
    s = int(start) if 0 <= int(start) < n else 0
    idx, dist = np.empty(m, np.int32), np.empty(m, F32)
    for j in range(m):
        idx[j], dist[j] = s, mind[s]
        D = sqdist_f32(x, s)
        mind = np.where(D < mind, D, mind)                      # a NaN or +inf D lowers nothing
        mind[s] = F32(-1)
        s = int(np.argmax(mind))                                # the first of the largest: ties -> the lower row
    return idx, dist


def fps_f64(x, m, start=0):
    """The same selection by brute force in float64: at every step, for every unselected row, the smallest finite distance to any
    selected row (0 for a row with a non-finite coordinate, +inf where there is none), then the first arg-max"""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    bad = ~np.isfinite(x).all(1)
    s = int(start) if 0 <= int(start) < n else 0
    chosen, idx, dist = [], np.empty(m, np.int32), np.empty(m, np.float64)
    score = np.where(bad, 0.0, np.inf)
    for j in range(m):
        idx[j], dist[j] = s, score[s]
        chosen.append(s)
        with np.errstate(all="ignore"):
            D = ((x[:, None, :] - x[None, chosen, :]) ** 2).sum(-1)          # (n, j + 1)
        D = np.where(np.isfinite(D), D, np.inf)
        score = np.minimum(np.where(bad, 0.0, np.inf), D.min(1))
        score[chosen] = -1.0
        s = int(np.argmax(score))
    return idx, dist


def fps_packed(x, offsets, counts, start=None):
    """(idx (S,) int32 rows of the tower, dist (S,)): cloud b = rows [offsets[b], offsets[b + 1]) sampled counts[b] times"""
    idx, dist = [], []
    for b, m in enumerate(counts):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        i, d = fps_f32(x[lo:hi], int(m), 0 if start is None else int(start[b]))
        idx.append(i + lo)
        dist.append(d)
    return np.concatenate(idx).astype(np.int32), np.concatenate(dist)


def fps_dense(x, m, start=None):
    """x (B, N, C) -> (idx (B, m) cloud-local, dist (B, m))"""
    res = [fps_f32(x[b], m, 0 if start is None else int(start[b])) for b in range(x.shape[0])]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def take_rows(x, rows):
    return np.ascontiguousarray(x[np.asarray(rows).reshape(-1)])


def scatter_rows(dy, rows, x_rows, dx0=None):
    """beta = 0 (dx0 None): zeros, then dx[rows[s]] = dy[s]; beta = 1: dx0 with dx[rows[s]] = dx0[rows[s]] + dy[s].  rows distinct."""
    rows = np.asarray(rows).reshape(-1)
    assert len(set(rows.tolist())) == rows.size
    dx = np.zeros((x_rows, dy.shape[1]), F32) if dx0 is None else np.array(dx0, F32)
    with np.errstate(all="ignore"):
        dx[rows] = dy if dx0 is None else (dx[rows] + dy).astype(F32)
    return dx


def tower_rows(idx, N):
    """idx (B, m) cloud-local -> (B * m,) rows of the (B * N)-row tower"""
    B = idx.shape[0]
    return (idx.astype(np.int64) + (np.arange(B, dtype=np.int64) * N)[:, None]).reshape(-1).astype(np.int32)


def integer_cloud(n, C, seed):
    """integer-valued coordinates in [-64, 64]: every difference, square and sum is exact in float32"""
    return np.random.default_rng(seed).integers(-64, 65, (n, C)).astype(F32)


def lattice(side, C=3):
    """the side^C integer lattice, row-major: exact ties everywhere"""
    g = np.stack(np.meshgrid(*[np.arange(side)] * C, indexing="ij"), -1).reshape(-1, C)
    return g.astype(F32)

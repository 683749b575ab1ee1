"""The expected result of the feature interpolation between two point sets (csrc/interp.hip), restated from the normative arithmetic
of include/dgcnn_hip.h K6; numpy only, no kernel code.

idx holds rows of the candidate set (a dense tower's cloud-local indices plus the cloud's first row: `tower_rows`); edge e = i * k + m.
interp_f32 / interp_bwd_f32 perform every product, sum and quotient in float32, one rounding each, in the header's order -- what the
kernels must reproduce bit for bit.  interp_f64 / interp_bwd_f64 are the same expressions in float64 from the same float32 distances:
the yardstick of tests/test_interp_reference.py for the float32 restatement itself."""
import numpy as np

F32 = np.float32


def tower_rows(idx, N):
    """idx (B, M, k) cloud-local -> (B * M, k) rows of the (B * N)-row candidate tower"""
    B, M, k = idx.shape
    return (idx.astype(np.int64) + (np.arange(B, dtype=np.int64) * N)[:, None, None]).reshape(B * M, k).astype(np.int32)


def _weights(dist, eps, T):
    D = np.asarray(dist, F32)
    e = T(F32(eps))
    with np.errstate(all="ignore"):
        w = np.where(D < np.inf, T(1) / np.maximum(D.astype(T), e), T(0)).astype(T)      # NaN < inf is False
    W = w[:, 0].copy()
    for m in range(1, w.shape[1]):
        W = (W + w[:, m]).astype(T)
    with np.errstate(all="ignore"):
        a = np.where(W[:, None] > 0, w / np.where(W > 0, W, T(1))[:, None], T(0)).astype(T)
    return a


def _interp(feat, idx, dist, eps, T):
    feat = np.asarray(feat, F32).astype(T)
    idx = np.asarray(idx)
    a = _weights(dist, eps, T)
    with np.errstate(all="ignore"):
        y = (a[:, 0, None] * feat[idx[:, 0]]).astype(T)
        for m in range(1, idx.shape[1]):
            y = (y + (a[:, m, None] * feat[idx[:, m]]).astype(T)).astype(T)
    return a, y


def _interp_bwd(a, idx, dy, p_rows, dfeat0, T):
    a = np.asarray(a).astype(T)
    dy = np.asarray(dy, F32).astype(T)
    idx = np.asarray(idx)
    Q, k = idx.shape
    g = np.zeros((p_rows, dy.shape[1]), T)
    with np.errstate(all="ignore"):
        for i in range(Q):                              # ascending e = i * k + m: the order of every bucket
            for m in range(k):
                j = idx[i, m]
                g[j] = (g[j] + (a[i, m] * dy[i]).astype(T)).astype(T)
        if dfeat0 is None:
            return g
        return (np.asarray(dfeat0, F32).astype(T) + g).astype(T)


def interp_f32(feat, idx, dist, eps):
    """(a (Q, k), y (Q, F)) float32: feat (P, F), idx (Q, k) rows of feat, dist (Q, k)"""
    return _interp(feat, idx, dist, eps, np.float32)


def interp_f64(feat, idx, dist, eps):
    return _interp(feat, idx, dist, eps, np.float64)


def interp_bwd_f32(a, idx, dy, p_rows, dfeat0=None):
    """dfeat (p_rows, F) float32: beta = 0 (dfeat0 None) or dfeat0 + g (beta = 1)"""
    return _interp_bwd(a, idx, dy, p_rows, dfeat0, np.float32)


def interp_bwd_f64(a, idx, dy, p_rows, dfeat0=None):
    return _interp_bwd(a, idx, dy, p_rows, dfeat0, np.float64)


def make_case(M, N, k, F, seed, C=3):
    """One cloud: candidates p (N, C) and queries q (M, C) uniform in [0, 1), every other query a copy of a candidate (D ~ 0: the
    clamp and the heavy weights), features in [-1, 1); -> (q, p, feat, idx (M, k) local, dist (M, k)) through the k-NN's own
    arithmetic (tests/knn_cross_reference.py)."""
    from knn_cross_reference import cross_knn
    rng = np.random.default_rng(seed)
    p = rng.random((N, C), dtype=np.float32)
    q = rng.random((M, C), dtype=np.float32)
    q[::2] = p[rng.integers(0, N, len(q[::2]))]
    feat = (rng.random((N, F), dtype=np.float32) * 2 - 1).astype(np.float32)
    idx, dist = cross_knn(q, p, k)
    return q, p, feat, idx, dist

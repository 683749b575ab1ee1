"""The expected result of the k-NN between two point sets (csrc/knn_cross.hip), from the oracle's own arithmetic; numpy and the oracle
only, no kernel code.

cross_knn(q, p, k): the rows of z = [q; p] are one cloud to the oracle, whose O.dist_pairs_f32 gives the normative
D[i][j] = fl(fl(s_i + s_j) - 2 p_ij) between query row i (row i of z) and candidate j (row M + j of z) -- s and the fmaf chain are
per-row and per-pair quantities, so the concatenation changes no bit.  NaN becomes +inf (D~) and a stable argsort keeps the k smallest
(D~, j), ties to the lower j: the rule of include/dgcnn_hip.h K1.  tests/test_knn_cross_reference.py pins this helper to O.k_nn on
q = p."""
import numpy as np

from oracle import dgcnn_oracle as O


def cross_dist(q, p):
    """D~ (M, N) float32 between the rows of q (M, C) and p (N, C)."""
    q = np.ascontiguousarray(q, np.float32)
    p = np.ascontiguousarray(p, np.float32)
    M, N = len(q), len(p)
    assert q.ndim == 2 and p.ndim == 2 and q.shape[1] == p.shape[1]
    z = np.concatenate([q, p], 0)
    cand = np.broadcast_to(M + np.arange(N, dtype=np.int32), (M, N))
    with np.errstate(all="ignore"):
        D = O.dist_pairs_f32(z, np.arange(M, dtype=np.int32), cand)
    return np.where(np.isnan(D), np.float32(np.inf), D).astype(np.float32)


def cross_knn(q, p, k):
    """(idx (M, k) int32, dist (M, k) float32): the k smallest (D~, j) of every query row, ascending, ties to the lower j."""
    D = cross_dist(q, p)
    if not 1 <= k <= D.shape[1]:
        raise ValueError("cross_knn: k=%d outside [1, N=%d]" % (k, D.shape[1]))
    order = np.argsort(D, axis=-1, kind="stable")[:, :k]
    return order.astype(np.int32), np.take_along_axis(D, order, -1)


def cross_knn_batch(q, p, k):
    """q (B, M, C), p (B, N, C) -> (idx (B, M, k), dist (B, M, k))"""
    out = [cross_knn(q[b], p[b], k) for b in range(len(q))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])

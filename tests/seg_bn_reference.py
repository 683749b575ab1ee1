"""Float64 reference of a packed tower with PER-CLOUD BatchNorm (flags.BN_PER_CLOUD, ops.*(bn_per_cloud=True)): the oracle on each
cloud alone, concatenated.  With per-cloud statistics nothing couples the clouds of a tower -- neighbours, max-pool, tile and every
BatchNorm see one cloud -- so cloud b of the tower IS oracle/dgcnn_oracle.py on rows [offsets[b], offsets[b + 1]) as a (1, n_b)
tower, which is also what the reference computes at `-mbs 1`.  The graphs are given as tower rows (what the HIP path captures)."""
import numpy as np

from oracle import dgcnn_oracle as O


def _tower(points):
    pts = np.asarray(points)
    pts = pts[None] if pts.ndim == 2 else pts
    assert pts.ndim == 3 and pts.shape[0] == 1
    return pts


def _cloud_graphs(idx_list, off, b):
    return [np.asarray(g)[:, off[b]:off[b + 1]].astype(np.int64) - off[b] for g in idx_list]


def model_forward(points, offsets, flags, params, idx_list):
    """points (R,C) or (1,R,C); idx_list: one (1,R,k) array of tower rows per EdgeConv layer -> logits (1,R,num_class)."""
    pts = _tower(points)
    off = np.asarray(offsets, np.int64)
    assert off[0] == 0 and off[-1] == pts.shape[1]
    P = {n: v.astype(pts.dtype) for n, v in params.items()}
    out = []
    for b in range(len(off) - 1):
        logits, _ = O.model_forward(pts[:, off[b]:off[b + 1]], flags, P, idx_list=_cloud_graphs(idx_list, off, b))
        out.append(logits)
    return np.concatenate(out, axis=1)


def own_graphs(points, offsets, flags, params):
    """The graphs the oracle builds by itself on every cloud alone, as tower rows: one (1,R,k) int32 array per EdgeConv layer."""
    pts = _tower(points)
    off = np.asarray(offsets, np.int64)
    P = {n: v.astype(pts.dtype) for n, v in params.items()}
    L = int(flags.EDGE_CONV_LAYERS)
    per = [[] for _ in range(L)]
    for b in range(len(off) - 1):
        _, cache = O.model_forward(pts[:, off[b]:off[b + 1]], flags, P)
        for i in range(L):
            per[i].append(cache["layers"][i]["ec"]["idx"].astype(np.int64) + off[b])
    return [np.concatenate(g, axis=1).astype(np.int32) for g in per]


def stack_forward(points, offsets, repeat, k, num_filters, params, residual, idx_list):
    """ops.repeat_edge_conv / repeat_residual_edge_conv with per-cloud BatchNorm -> the 3 * repeat tensors, each (1,R,1,ch)."""
    pts = _tower(points)
    off = np.asarray(offsets, np.int64)
    P = {n: v.astype(pts.dtype) for n, v in params.items()}
    per = []
    for b in range(len(off) - 1):
        tensors, _ = O.repeat_edge_conv(pts[:, off[b]:off[b + 1]], repeat, k, num_filters, P, residual=residual,
                                        idx_list=_cloud_graphs(idx_list, off, b))
        per.append(tensors)
    return [np.concatenate([t[i] for t in per], axis=1) for i in range(len(per[0]))]

"""Float64 reference of the per-cloud loss (flags.LOSS_PER_CLOUD, csrc/seg_loss.hip).  Cloud b = rows [off[b], off[b + 1]) of a
packed tower, n_b rows:

    l_b = (1 / n_b) sum_{r in b} w_r (log sum_c e^{z_rc} - z_{r, lab_r}),    a_b = #{r in b : first arg-max of z_r == lab_r} / n_b,
    dlogits_r = (p_r - onehot_r) w_r / n_b,    tower scalars = the mean over the clouds of (l_b, a_b)

-- what `-bs M -mbs 1` computes in M micro-steps: each seeds its backward with the mean loss of its one cloud
(dgcnn/trainval.py:52) and ADDS its gradient to the accumulators (trainval.py:79), and the log shows the mean over the micro-steps.
Rows with a negative label add nothing to either sum but count in n_b."""
import numpy as np

import seg_bn_bwd_reference as SB


def xent(logits, labels, weight, off):
    """logits (R, ncls), labels (R,), weight (R,) or None, off (nseg + 1,) -> dict of float64 arrays: softmax (R, ncls),
    dlogits (R, ncls), term (R,) = w_r xent_r (0 for a negative label), correct (R,), n (nseg,), loss (nseg,), acc (nseg,)."""
    z = np.asarray(logits, np.float64)
    lab = np.asarray(labels, np.int64)
    R, ncls = z.shape
    w = np.ones(R) if weight is None else np.asarray(weight, np.float64)
    off = np.asarray(off, np.int64)
    assert off[0] == 0 and off[-1] == R
    n = np.diff(off).astype(np.float64)
    mx = z.max(1, keepdims=True)
    e = np.exp(z - mx)
    se = e.sum(1)
    sm = e / se[:, None]
    has = lab >= 0
    safe = np.where(has, lab, 0)
    term = np.where(has, (np.log(se) - (z[np.arange(R), safe] - mx[:, 0])) * w, 0.0)
    correct = np.where(has, np.argmax(z, 1) == safe, False).astype(np.float64)          # np.argmax: the first maximum
    onehot = np.zeros_like(sm)
    onehot[np.arange(R)[has], lab[has]] = 1.0
    row_n = np.repeat(n, np.diff(off))
    out = dict(softmax=sm, dlogits=(sm - onehot) * (w / row_n)[:, None], term=term, correct=correct, n=n)
    out["loss"] = np.array([term[lo:hi].sum() / (hi - lo) for _, lo, hi in SB.clouds(off)])
    out["count"] = np.array([correct[lo:hi].sum() for _, lo, hi in SB.clouds(off)])
    out["acc"] = out["count"] / n
    return out


def train_step_grads(points, labels, off, flags, params, idx_list, weight):
    """trainval.accum_gradient on a packed tower under BN_PER_CLOUD_TRAIN + LOSS_PER_CLOUD: the UNWEIGHTED sum over the clouds of
    oracle.train_step_grads(cloud b, weight_b) in float64 (idx_list: tower rows, as the HIP path captures them; None: the oracle's
    own graphs).  -> ({name: gradient}, [l_b], [a_b])."""
    from oracle import dgcnn_oracle as O
    pts = np.asarray(points, np.float64)
    G, losses, accs = {}, [], []
    for _, lo, hi in SB.clouds(off):
        graphs = None if idx_list is None else [np.asarray(g)[:, lo:hi].astype(np.int64) - lo for g in idx_list]
        g, l, a, _ = O.train_step_grads(pts[None, lo:hi], np.asarray(labels)[None, lo:hi], flags,
                                        {n: np.asarray(v, np.float64) for n, v in params.items()},
                                        weight=None if weight is None else np.asarray(weight, np.float64)[None, lo:hi],
                                        idx_list=graphs)
        losses.append(float(l))
        accs.append(float(a))
        for n, v in g.items():
            G[n] = G.get(n, 0.0) + v
    return G, losses, accs

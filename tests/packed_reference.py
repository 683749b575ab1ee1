"""Float64 reference of the model on a PACKED tower (dgcnn.model.build(offsets=...)): clouds of different sizes concatenated
row-wise into (R, C), cloud b = rows [offsets[b], offsets[b + 1]).

oracle/dgcnn_oracle.py:model_forward takes its max-pool over axis 1 of a (B, N) tower, so the packed forward and backward are
assembled here from the oracle's own pieces -- repeat_edge_conv(idx_list=...), conv_bn_act, conv_bn_act_bwd, edge_conv_bwd,
softmax_xent -- on the (1, R) tower: BatchNorm over all R rows, neighbours as given (tower rows), and per cloud
  * the max over the cloud's rows with its FIRST arg-max (model.py:76-77),
  * the tile of that maximum over the cloud's rows (model.py:80-81),
  * the tile's transpose: the sum over the cloud's rows.
With equal-sized clouds this is O.model_forward / O.model_backward on the (B, N) tower (tests/test_packed_reference.py)."""
import numpy as np

from oracle import dgcnn_oracle as O


def tower_graphs(idx_dense):
    """(B,N,k) per-cloud indices of a dense tower -> (1, B*N, k) tower rows of the same clouds packed with offsets b*N."""
    B, N, k = idx_dense.shape
    return (idx_dense.astype(np.int64) + (np.arange(B) * N)[:, None, None]).reshape(1, B * N, k).astype(np.int32)


def model_forward(points, offsets, flags, params, idx_list, dropout_mask=None):
    """points (R,C) or (1,R,C); idx_list: one (1,R,k_i) array of tower rows per EdgeConv layer (required: the dynamic graphs of a
    packed tower are per cloud, which O.k_nn on the (1, R) tower is not).  -> (logits (1,R,num_class), cache)."""
    if idx_list is None:
        raise ValueError("the packed reference needs every layer's graph (tower rows)")
    pts = np.asarray(points)
    pts = pts[None] if pts.ndim == 2 else pts
    assert pts.ndim == 3 and pts.shape[0] == 1
    off = np.asarray(offsets, np.int64)
    R = pts.shape[1]
    assert off[0] == 0 and off[-1] == R and (np.diff(off) > 0).all()
    dt = pts.dtype
    P = {n: v.astype(dt) for n, v in params.items()}
    L = int(flags.EDGE_CONV_LAYERS)
    name = flags.MODEL_NAME
    if name not in ("dgcnn", "residual-dgcnn", "residual-dgcnn-nofc"):
        raise NotImplementedError("Unsupported MODEL_NAME: %s" % name)
    residual = name != "dgcnn"
    tensors, layers = O.repeat_edge_conv(pts, L, int(flags.KVALUE), flags.EDGE_CONV_FILTERS, P, residual=residual, idx_list=idx_list,
                                         edge_mlp_dtype=str(getattr(flags, "EDGE_MLP_DTYPE", "f32") or "f32"))
    cache = dict(layers=layers, L=L, residual=residual, off=off)
    if name == "residual-dgcnn-nofc":
        fin, cf = O.conv_bn_act(tensors[-1], P["Final/weights"], P["Final/BatchNorm/beta"], relu=True)
        cache.update(final=cf, nofc=True)
        return fin[:, :, 0, :], cache
    cat = np.concatenate([tensors[3 * i + 2] for i in range(L)], axis=-1)
    merged, cm = O.conv_bn_act(cat, P["MergedEdgeConv/weights"], P["MergedEdgeConv/BatchNorm/beta"], relu=True)
    tensors.append(merged)
    nseg = len(off) - 1
    m2 = merged[0, :, 0, :]                                                   # (R, 1024)
    gmax = np.stack([m2[off[b]:off[b + 1]].max(axis=0) for b in range(nseg)])
    garg = np.stack([m2[off[b]:off[b + 1]].argmax(axis=0) for b in range(nseg)])    # first arg-max, row within the cloud
    gtile = np.repeat(gmax, np.diff(off), axis=0)[None, :, None, :]            # the per-cloud tile
    big = np.concatenate([gtile] + tensors, axis=3)
    fcs = []
    net = big
    for i in range(int(flags.FC_LAYERS)):
        net, cfc = O.conv_bn_act(net, P["FC%d/weights" % i], P["FC%d/BatchNorm/beta" % i], relu=True)
        fcs.append(cfc)
    if bool(flags.TRAIN) and dropout_mask is not None:
        net = net * dropout_mask.astype(dt)
    fin, cf = O.conv_bn_act(net, P["Final/weights"], P["Final/BatchNorm/beta"], relu=True)
    cache.update(merged=cm, garg=garg, fcs=fcs, final=cf, nofc=False, dropout_mask=dropout_mask if bool(flags.TRAIN) else None,
                 widths=[t.shape[-1] for t in tensors])
    return fin[:, :, 0, :], cache


def model_backward(dlogits, cache):
    """dlogits (1,R,num_class) -> dict name -> gradient of every trainable variable."""
    G = {}
    L, off = cache["L"], cache["off"]
    nseg = len(off) - 1
    d = dlogits[:, :, None, :]
    d, G["Final/weights"], G["Final/BatchNorm/beta"] = O.conv_bn_act_bwd(d, cache["final"])
    layers = cache["layers"]
    if cache["nofc"]:
        d_t = [None] * (3 * L)
        d_t[-1] = d
    else:
        if cache["dropout_mask"] is not None:
            d = d * cache["dropout_mask"].astype(d.dtype)
        for i in reversed(range(len(cache["fcs"]))):
            d, G["FC%d/weights" % i], G["FC%d/BatchNorm/beta" % i] = O.conv_bn_act_bwd(d, cache["fcs"][i])
        d2 = d[0, :, 0, :]
        d_g = np.stack([d2[off[b]:off[b + 1], :1024].sum(axis=0) for b in range(nseg)])      # tile^T: the sum over the cloud
        d_t = []
        o = 1024
        for w in cache["widths"]:
            d_t.append(d[..., o:o + w])
            o += w
        d_merged = d_t.pop().copy()
        for b in range(nseg):                                                  # max-pool gradient to the first arg-max
            d_merged[0, off[b] + cache["garg"][b], 0, np.arange(1024)] += d_g[b]
        dcat, G["MergedEdgeConv/weights"], G["MergedEdgeConv/BatchNorm/beta"] = O.conv_bn_act_bwd(d_merged, cache["merged"])
        for i in range(L):
            d_t[3 * i + 2] = d_t[3 * i + 2] + dcat[..., 64 * i:64 * (i + 1)]
    # the EdgeConv stack (row-wise passes on the (1, R) tower, graphs from the caches): oracle/dgcnn_oracle.py:model_backward
    d_next = None
    for i in reversed(range(L)):
        s = "EdgeConv%d/" % i
        rec = layers[i]
        d_net = d_t[3 * i + 2] if d_t[3 * i + 2] is not None else 0
        if d_next is not None:
            d_net = d_net + d_next
        zero = np.zeros_like(rec["ec"]["net_max"])
        d_max = d_t[3 * i] if d_t[3 * i] is not None else zero
        d_mean = d_t[3 * i + 1] if d_t[3 * i + 1] is not None else zero
        d_short = None
        if rec["pre"] is not None:
            d_pre = d_net * (rec["pre"] > 0)
            d_net = d_pre
            d_short = d_pre
            if rec["sc"] is not None:
                d_short, G[s + "shortcut/weights"], G[s + "shortcut/BatchNorm/beta"] = O.conv_bn_act_bwd(d_pre, rec["sc"])
        dx, g = O.edge_conv_bwd(d_max, d_mean, d_net, rec["ec"])
        G[s + "conv0/weights"], G[s + "conv0/BatchNorm/beta"] = g["W0"], g["beta0"]
        G[s + "conv1/weights"], G[s + "conv1/BatchNorm/beta"] = g["W1"], g["beta1"]
        d_next = dx[:, :, None, :]
        if d_short is not None:
            d_next = d_next + d_short
    return G


def train_step_grads(points, labels, offsets, flags, params, idx_list, weight=None):
    """One packed micro-step: (grads, loss, accuracy, softmax (1,R,ncls)); loss / accuracy are means over the R rows."""
    logits, cache = model_forward(points, offsets, flags, params, idx_list)
    R = logits.shape[1]
    loss, sm, acc, dlogits = O.softmax_xent(logits, np.asarray(labels).reshape(1, R),
                                            None if weight is None else np.asarray(weight).reshape(1, R))
    return model_backward(dlogits, cache), loss, acc, sm

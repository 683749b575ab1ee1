"""Reference of the BACKWARD of per-cloud BatchNorm on a packed tower (Segments(bn_per_cloud_train=True), flags.BN_PER_CLOUD_TRAIN):
tests/bn_reference.py applied to each cloud's row slice.  With per-cloud statistics nothing couples the clouds of a tower, so every
sum of the backward (sum dz, sum dz xhat, dbeta, dW) is a sum of per-cloud pieces and every row's gradient is that of its cloud alone.

Two layers, as in bn_reference.py:
* float32 DECISIONS + float64 SUMS + float32 REPLAYS per cloud, for the kernels of csrc/seg_bn.hip (k1_*, edge_*, finalize32);
* an all-float64 restatement of conv_bn_act / edge_conv backward per cloud (conv_bn_act_bwd, edge_conv_bwd), which
  tests/test_seg_bn_bwd_reference.py holds against oracle/dgcnn_oracle.py run on each cloud alone; oracle_stack / train_step_grads
  are that oracle, cloud by cloud, in the shape the GPU tests compare against."""
import numpy as np

import bn_reference as BR

F32 = np.float32


def clouds(off):
    off = np.asarray(off, np.int64)
    return [(b, int(off[b]), int(off[b + 1])) for b in range(len(off) - 1)]


def tables32(y, off, eps=BR.EPS):
    """float32 (mean, rstd) tables (nseg, F) from the float64 two-pass statistics of each cloud's rows of y (R, F) or (R, k, F)."""
    mu, rs = [], []
    for _, lo, hi in clouds(off):
        m, v = BR.two_pass_stats64(np.asarray(y[lo:hi]).reshape(-1, y.shape[-1]))
        mu.append(m.astype(F32))
        rs.append((1.0 / np.sqrt(v + eps)).astype(F32))
    return np.stack(mu), np.stack(rs)


# ------------------------------------------------------------------------------------------------ kernels: decisions, sums, replays
def k1_clouds(T, off, mu, rs, be, relu, d):
    """k = 1 layer: per cloud (fw, dz32, Sums) with the cloud's table row; d (R, F) float32 = the (already added) gradient input."""
    out = []
    for b, lo, hi in clouds(off):
        fw = BR.Fwd(BR.f32(T[lo:hi])[:, None, :], mu[b], rs[b], be, relu)
        out.append((fw, BR.dz32(fw, d[lo:hi], None), BR.Sums(BR.dz64(fw, d[lo:hi], None), fw.xh)))
    return out


def edge_clouds(y, off, mu, rs, be, relu, dmax, dmean):
    """conv0: y (R, k, F) float32 rows; per cloud (fw, dz32, Sums)."""
    out = []
    for b, lo, hi in clouds(off):
        fw = BR.Fwd(y[lo:hi], mu[b], rs[b], be, relu)
        out.append((fw, BR.dz32(fw, dmax[lo:hi], dmean[lo:hi]), BR.Sums(BR.dz64(fw, dmax[lo:hi], dmean[lo:hi]), fw.xh)))
    return out


def point_terms64(mx, mn, npos, dmax, dmean, beta, k):
    """The per-point terms whose column sums BR.points_closed_form64 returns: (t0, t1), each (n, F) float64."""
    mx, mn, npos, dmax, dmean, beta = (np.asarray(a, np.float64) for a in (mx, mn, npos, dmax, dmean, beta))
    g1 = np.where(mx > 0, dmax, 0.0)
    g2 = dmean / k
    return g1 + g2 * npos, g1 * (mx - beta) + g2 * (k * mn - beta * npos)


def finalize32(red, sizes, k, prior=None, dbeta_beta=0.0):
    """dgcnn_seg_bn_bwd_finalize_f32 from red (nseg, 2, F) float64: c1 / c2 (nseg, F) by apply32's arithmetic with n = n_b k, and
    dbeta by dbeta32 of the sum of red0 over the clouds, b ascending, in double."""
    red = np.asarray(red, np.float64)
    c1 = np.stack([(red[b, 0] * (1.0 / float(n * k))).astype(F32) for b, n in enumerate(sizes)])
    c2 = np.stack([(red[b, 1] * (1.0 / float(n * k))).astype(F32) for b, n in enumerate(sizes)])
    s = np.zeros(red.shape[-1])
    for b in range(len(sizes)):
        s = s + red[b, 0]
    return c1, c2, BR.dbeta32(s, prior, dbeta_beta)


def apply32(cases, red, k):
    """The apply pass per cloud given red (nseg, 2, F): (dY (R, k, F), dYsum (R, F)) float32, cloud b with n = n_b k."""
    dy, ds = [], []
    for b, (fw, d32, _) in enumerate(cases):
        o, acc = BR.apply32(d32, fw.xh, fw.rs, red[b], fw.R * k)
        dy.append(o)
        ds.append(acc)
    return np.concatenate(dy), np.concatenate(ds)


# ------------------------------------------------------------------------------------------------------- float64, against the oracle
class Fwd64(object):
    """The forward of one cloud's (n, k, F) rows in float64, with the attributes BR.dz64 reads.  eps is the oracle's 1e-3 (the
    float64 value, not the fp32 one the kernels receive: this layer is held against the oracle to 1e-10)."""

    def __init__(self, y, beta, relu, eps=1e-3):
        y = np.asarray(y, np.float64)
        self.R, self.k, self.F = y.shape
        self.relu = int(bool(relu))
        mu, var = BR.two_pass_stats64(y.reshape(-1, self.F))
        self.rs = 1.0 / np.sqrt(var + eps)
        self.xh = (y - mu) * self.rs
        z = self.xh + np.asarray(beta, np.float64)
        self.z = np.maximum(z, 0.0) if self.relu else z
        self.mx = self.z.max(1)
        self.ismax = self.z == self.mx[:, None, :]
        self.ties = self.ismax.sum(1).astype(np.float64)
        self.pos = self.z > 0


def conv_bn_act_bwd(x, W, beta, relu, off, dout):
    """1x1 conv + per-cloud BatchNorm (+ ReLU) on the packed tower x (R, Cin): -> (dx (R, Cin), dW, dbeta), float64."""
    x, W, dout = (np.asarray(a, np.float64) for a in (x, W, dout))
    dx, dW, dbeta = np.zeros_like(x), np.zeros_like(W), np.zeros(W.shape[1])
    for _, lo, hi in clouds(off):
        fw = Fwd64((x[lo:hi] @ W)[:, None, :], beta, relu)
        dz = BR.dz64(fw, dout[lo:hi], None)
        s = BR.Sums(dz, fw.xh)
        dy = BR.dy64(dz, fw.xh, fw.rs, s.red)[:, 0]
        dx[lo:hi] = dy @ W.T
        dW += x[lo:hi].T @ dy
        dbeta += s.red0
    return dx, dW, dbeta


def edge_conv_bwd(x, idx, W0, beta0, W1, beta1, relu1, off, d_max, d_mean, d_net):
    """ops.edge_conv on the packed tower x (R, C) with per-cloud BatchNorm, idx (R, k) TOWER rows: -> (dx, dict(W0, beta0, W1, beta1))."""
    x, W0, W1 = (np.asarray(a, np.float64) for a in (x, W0, W1))
    R, C = x.shape
    k, F = idx.shape[1], W0.shape[1]
    idx = np.asarray(idx, np.int64)
    dx, dW0, db0 = np.zeros_like(x), np.zeros_like(W0), np.zeros(F)
    mm = np.empty((R, 2 * F))
    fws = []
    for _, lo, hi in clouds(off):
        E = np.concatenate([np.broadcast_to(x[lo:hi, None, :], (hi - lo, k, C)), x[idx[lo:hi]] - x[lo:hi, None, :]], -1)
        fw = Fwd64(E @ W0, beta0, 1)
        mm[lo:hi, :F], mm[lo:hi, F:] = fw.mx, fw.z.mean(1)
        fws.append(fw)
    dcat, dW1, db1 = conv_bn_act_bwd(mm, W1, beta1, relu1, off, d_net)
    dmx, dmn = np.asarray(d_max, np.float64) + dcat[:, :F], np.asarray(d_mean, np.float64) + dcat[:, F:]
    for (_, lo, hi), fw in zip(clouds(off), fws):
        dz = BR.dz64(fw, dmx[lo:hi], dmn[lo:hi])
        s = BR.Sums(dz, fw.xh)
        dY = BR.dy64(dz, fw.xh, fw.rs, s.red)                                       # (n, k, F)
        dW0 += BR.wgrad64(x[lo:hi], (idx[lo:hi] - lo)[None], 1, hi - lo, dY)
        db0 += s.red0
        dx[lo:hi] += dY.sum(1) @ (W0[:C] - W0[C:]).T
        np.add.at(dx, idx[lo:hi].reshape(-1), dY.reshape(-1, F) @ W0[C:].T)
    return dx, dict(W0=dW0, beta0=db0, W1=dW1, beta1=db1)


def oracle_stack(points, off, repeat, k, num_filters, P, residual, idx_list, d):
    """ops.repeat_edge_conv / repeat_residual_edge_conv with per-cloud BatchNorm and its backward = oracle/dgcnn_oracle.py on each
    cloud ALONE.  points (R, C) float64; idx_list: one (1, R, k_i) array of tower rows per layer; d: upstream gradients of the
    3 * repeat returned tensors, each (1, R, 1, ch).  -> (tensors [(1, R, 1, ch)], d(points) (R, C), {name: gradient})."""
    from oracle import dgcnn_oracle as O
    pts = np.asarray(points, np.float64)
    per, dxs, G = [], [], {}

    def acc(name, g):
        G[name] = G[name] + g if name in G else g
    for _, lo, hi in clouds(off):
        graphs = [np.asarray(g)[:, lo:hi].astype(np.int64) - lo for g in idx_list]
        tensors, layers = O.repeat_edge_conv(pts[None, lo:hi], repeat, k, num_filters, P, residual=residual, idx_list=graphs)
        per.append(tensors)
        d_next = None
        for i in reversed(range(repeat)):                          # the EdgeConv loop of O.model_backward
            s, rec = "EdgeConv%d/" % i, layers[i]
            d_net = d[3 * i + 2][:, lo:hi] + (0 if d_next is None else d_next)
            d_short = None
            if rec["pre"] is not None:                               # relu(shortcut + net), ops.py:134
                d_net = d_net * (rec["pre"] > 0)
                d_short = d_net
                if rec["sc"] is not None:
                    d_short, gw, gb = O.conv_bn_act_bwd(d_net, rec["sc"])
                    acc(s + "shortcut/weights", gw)
                    acc(s + "shortcut/BatchNorm/beta", gb)
            dx, g = O.edge_conv_bwd(d[3 * i][:, lo:hi], d[3 * i + 1][:, lo:hi], d_net, rec["ec"])
            for leaf, key in (("conv0/weights", "W0"), ("conv0/BatchNorm/beta", "beta0"), ("conv1/weights", "W1"),
                              ("conv1/BatchNorm/beta", "beta1")):
                acc(s + leaf, g[key])
            d_next = dx[:, :, None, :] + (0 if d_short is None else d_short)
        dxs.append(d_next[0, :, 0, :])
    return [np.concatenate([t[j] for t in per], axis=1) for j in range(len(per[0]))], np.concatenate(dxs), G


def train_step_grads(points, labels, off, flags, params, idx_list, weight):
    """trainval.accum_gradient on a packed tower with per-cloud BatchNorm: sum_b (n_b / R) oracle.train_step_grads(cloud b, weight_b)
    in float64 (loss and accuracy are the mean over the R rows).  -> ({name: gradient}, loss)."""
    from oracle import dgcnn_oracle as O
    pts = np.asarray(points, np.float64)
    R = len(pts)
    G, loss = {}, 0.0
    for _, lo, hi in clouds(off):
        graphs = [np.asarray(g)[:, lo:hi].astype(np.int64) - lo for g in idx_list]
        g, l, _, _ = O.train_step_grads(pts[None, lo:hi], np.asarray(labels)[None, lo:hi], flags,
                                        {n: np.asarray(v, np.float64) for n, v in params.items()},
                                        weight=np.asarray(weight, np.float64)[None, lo:hi], idx_list=graphs)
        w = (hi - lo) / float(R)
        loss += w * float(l)
        for n, v in g.items():
            G[n] = G.get(n, 0.0) + w * v
    return G, loss

"""MI355X-native counterpart of the reference's operator module (dgcnn/ops.py:8-163).

Same names, positional order, defaults, return conventions and errors as the reference; tensors
are torch-ROCm tensors (memory holders) instead of tf.Tensor, and a call executes the HIP
kernels at once instead of adding nodes to a TF graph.  `knn` / `build_edge_conv` are the
aliases BASELINE.json's north_star uses for `k_nn` / `edge_conv`.
"""
from __future__ import annotations

import math

import torch

from . import _engine as E
from . import _hip as H


def relu(x):
    """Marker for `activation=` (tf.nn.relu in the reference); never called on tensors."""
    raise TypeError("dgcnn.ops.relu is an activation marker, not a callable op")


def _is_relu(activation):
    if activation is None:
        return False
    if activation is relu or getattr(activation, "__name__", "") == "relu":
        return True
    raise NotImplementedError("only relu / None activations exist in the reference (ops.py:42,123)")


def _segments(points, offsets, ks, bn_per_cloud=False, bn_per_cloud_train=False):
    """Host-side checks of a packed tower, before any device work: points (R,C), (1,R,C) or (1,R,1,C); offsets (nseg + 1 ints from
    0 to R, strictly increasing) or a Segments; every k at most the smallest cloud.  Returns None for a dense tower (offsets None).
    bn_per_cloud: BatchNorm with each cloud's own statistics (forward only) -- needs offsets; a Segments keeps its own setting.
    bn_per_cloud_train: the same with its backward (allowed inside a recording); implies bn_per_cloud."""
    if offsets is None:
        if bn_per_cloud or bn_per_cloud_train:
            raise ValueError("bn_per_cloud=True needs offsets: per-cloud BatchNorm is a mode of a packed tower")
        return None
    shp = tuple(points.shape)
    if len(shp) == 2 or (len(shp) in (3, 4) and shp[0] == 1 and (len(shp) == 3 or shp[2] == 1)):
        R = shp[0] if len(shp) == 2 else shp[1]
    else:
        raise ValueError("a packed tower is (R,C), (1,R,C) or (1,R,1,C), got %s" % (shp,))
    seg = offsets if isinstance(offsets, E.Segments) else E.Segments(offsets, R, bn_per_cloud=bn_per_cloud,
                                                                               bn_per_cloud_train=bn_per_cloud_train)
    if seg.rows != R:
        raise ValueError("offsets end at %d, the tower has %d rows" % (seg.rows, R))
    for k in ks:
        seg.check_k(int(k))
    return seg


def _rows_channels(t, what, packed, who="k_nn"):
    """(B, rows per cloud, C) of a dense (B,N,C) set, or (1, R, C) of a packed (R,C) / (1,R,C) tower -- from the shape alone"""
    shp = tuple(t.shape)
    if packed:
        if len(shp) == 2:
            return 1, shp[0], shp[1]
        if len(shp) == 3 and shp[0] == 1:
            return 1, shp[1], shp[2]
        raise ValueError("%s: a packed %s tower is (R,C) or (1,R,C), got %s" % (who, what, shp))
    if len(shp) != 3:
        raise ValueError("%s: %s must be (B,N,C), got %s" % (who, what, shp))
    return shp


def _k_nn_cross(points, k, offsets, queries, query_offsets, return_dist):
    """k_nn between two sets (queries given) or of one set with its distances (return_dist): every check on the host, from shapes and
    offsets alone, before any device work; then E.knn_cross."""
    if queries is None and query_offsets is not None:
        raise ValueError("k_nn: query_offsets without queries")
    if queries is not None and (offsets is None) != (query_offsets is None):
        raise ValueError("k_nn: packed towers need offsets (points) AND query_offsets (queries); got only %s"
                         % ("offsets" if query_offsets is None else "query_offsets"))
    if k > E.KNN_CROSS_MAX_K:
        raise ValueError("k_nn: k=%d > %d: with queries= or return_dist= at most %d neighbours are kept" % (k, E.KNN_CROSS_MAX_K,
                                                                                                          E.KNN_CROSS_MAX_K))
    packed = offsets is not None
    Bp, N, C = _rows_channels(points, "points", packed)
    Bq, M, Cq = (Bp, N, C) if queries is None else _rows_channels(queries, "queries", packed)
    if Cq != C:
        raise ValueError("k_nn: queries have %d channels, points %d" % (Cq, C))
    if Bq != Bp:
        raise ValueError("k_nn: %d query clouds, %d clouds of points" % (Bq, Bp))
    pseg = qseg = None
    if packed:
        pseg = _segments(points, offsets, [k])
        qseg = pseg if queries is None else (query_offsets if isinstance(query_offsets, E.Segments) else E.Segments(query_offsets, M))
        if qseg.rows != M:
            raise ValueError("query_offsets end at %d, the query tower has %d rows" % (qseg.rows, M))
        if qseg.nseg != pseg.nseg:
            raise ValueError("k_nn: %d query clouds, %d clouds of points" % (qseg.nseg, pseg.nseg))
    elif k > N or k <= 0:
        raise ValueError("k_nn: k=%d must be in [1, N=%d] (tf.nn.top_k raises otherwise)" % (k, N))
    p2d = E.as2d(points)[0]
    q2d = p2d if queries is None else E.as2d(queries)[0]
    return E.knn_cross(q2d, p2d, Bp, M, N, k, qseg=qseg, pseg=pseg, want_dist=return_dist)


def k_nn(points, k, offsets=None, queries=None, query_offsets=None, return_dist=False):
    """dgcnn/ops.py:8-19.  points (B,N,C) -> idx (B,N,k) int32: the k nearest (squared L2 via
    (s_i+s_j)-2<x_i,x_j>), self included, ascending, ties -> lower index.  Bit-exact vs the oracle.
    offsets: a packed tower of clouds of different sizes, points (R,C) or (1,R,C), cloud b = rows [offsets[b], offsets[b + 1]):
    idx (1,R,k) holds tower rows (offsets[b] + j), per cloud the dense k_nn of that cloud alone.
    queries (B,M,C): the search between two sets -- idx (B,M,k) = for every query row the k nearest rows of `points` of the same cloud
    (cloud-local j; no row is "self"), same arithmetic, tie and non-finite rules; k <= 64.  Packed: queries (Rq,C) or (1,Rq,C) with
    query_offsets, points with offsets, the same number of clouds; idx (1,Rq,k) holds rows of the `points` tower.
    return_dist: (idx, dist) with dist float32 in idx's shape, the selected distances (+inf where a NaN or infinite one fills a row);
    with queries=None the points are their own queries and idx is the plain call's."""
    k = int(k)
    if queries is not None or query_offsets is not None or return_dist:
        return _k_nn_cross(points, k, offsets, queries, query_offsets, bool(return_dist))
    if offsets is not None:
        seg = _segments(points, offsets, [k])
        x, _, R = E.as2d(points)
        return E.knn(x, 1, R, k, seg=seg)
    x, B, N = E.as2d(points)
    if k > N or k <= 0:
        raise ValueError("k_nn: k=%d must be in [1, N=%d] (tf.nn.top_k raises otherwise)" % (k, N))
    return E.knn(x, B, N, k)


knn = k_nn


def _interp_rows(t, what, packed, rank4=False, who="interpolate"):
    """(clouds, rows per cloud, channels) of an argument of `interpolate`, from its shape alone: dense (B,N,C) [(B,N,1,C) with rank4],
    packed (R,C) or (1,R,C) [(1,R,1,C) with rank4]"""
    shp = tuple(t.shape)
    if rank4 and len(shp) == 4:
        if shp[2] != 1:
            raise ValueError("%s: a rank-4 %s has a singleton axis -2, got %s" % (who, what, shp))
        shp = (shp[0], shp[1], shp[3])
    if packed:
        if len(shp) == 2:
            return 1, shp[0], shp[1]
        if len(shp) == 3 and shp[0] == 1:
            return 1, shp[1], shp[2]
        raise ValueError("%s: a packed %s tower is (R,C) or (1,R,C), got %s" % (who, what, tuple(t.shape)))
    if len(shp) != 3:
        raise ValueError("%s: %s must be (B,N,C), got %s" % (who, what, tuple(t.shape)))
    return shp


def interpolate(features, points, queries, k=3, offsets=None, query_offsets=None, eps=1e-16, graph=None, skip=None):
    """Carry features from one point set to another (PointNet++ feature propagation, PyG's knn_interpolate): every query row receives
    the inverse-distance-weighted mean of the features of its k nearest `points`, weights 1 / max(d, eps) over the squared distances
    k_nn returns, normalised to sum 1 (include/dgcnn_hip.h K6 states the arithmetic bit for bit).
    features (B,N,F) or (B,N,1,F) live on `points` (B,N,C); queries (B,M,C); the result is (B,M,1,F).  Packed towers: features (R,F),
    (1,R,F) or (1,R,1,F), points (R,C) or (1,R,C) with offsets, queries (Rq,C) or (1,Rq,C) with query_offsets (the rules of k_nn's
    search between two sets); the result is (1,Rq,1,F).
    graph=(idx, dist): a graph the caller already has from k_nn(points, k, queries=..., return_dist=True); points and queries may
    then be None.  skip (B,M,Cs) [packed: (Rq,Cs) or (1,Rq,Cs)]: the skip connection of a feature-propagation block -- the result
    is (B,M,1,F+Cs) = [interpolated | skip] in one buffer, without a concat pass.
    Recorded, the features and skip receive gradients (fixed order, the same bits run to run); the coordinates and the weights do
    not -- k_nn has no backward.  The weights of near-coincident points inherit the absolute error of k_nn's distances."""
    k = int(k)
    if k < 1 or k > E.INTERP_MAX_K:
        raise ValueError("interpolate: k=%d must be in [1, %d], the limit of k_nn between two sets" % (k, E.INTERP_MAX_K))
    eps = E.check_interp_eps(eps)
    if (offsets is None) != (query_offsets is None):
        raise ValueError("interpolate: packed towers need offsets (points, features) AND query_offsets (queries); got only %s"
                         % ("offsets" if query_offsets is None else "query_offsets"))
    packed = offsets is not None
    B, N, F = _interp_rows(features, "features", packed, rank4=True)
    if F % 4 or F > 1024 or F < 1:
        raise ValueError("interpolate: features need F %% 4 == 0 and F <= 1024 channels, got F=%d" % F)
    C = None
    if points is not None:
        Bp, Np, C = _interp_rows(points, "points", packed)
        if (Bp, Np) != (B, N):
            raise ValueError("interpolate: features cover %d clouds of %d rows, points %d of %d" % (B, N, Bp, Np))
    M = None
    if queries is not None:
        Bq, M, Cq = _interp_rows(queries, "queries", packed)
        if Bq != B:
            raise ValueError("interpolate: %d clouds of queries, %d of points" % (Bq, B))
        if C is not None and Cq != C:
            raise ValueError("interpolate: queries have %d channels, points %d" % (Cq, C))
    if graph is not None:
        if not (isinstance(graph, (tuple, list)) and len(graph) == 2):
            raise ValueError("interpolate: graph must be the (idx, dist) pair of k_nn(..., return_dist=True)")
        gi, gd = tuple(graph[0].shape), tuple(graph[1].shape)
        if len(gi) != 3 or gi != gd or gi[0] != B or gi[2] != k or (M is not None and gi[1] != M):
            raise ValueError("interpolate: graph must hold idx and dist of shape (%d, %s, %d), got %s and %s"
                             % (B, "M" if M is None else M, k, gi, gd))
        M = gi[1]
    elif points is None or queries is None:
        raise ValueError("interpolate: points and queries are needed when no graph is given")
    pseg = qseg = None
    if packed:
        pseg = offsets if isinstance(offsets, E.Segments) else E.Segments(offsets)
        if pseg.rows != N:
            raise ValueError("interpolate: offsets end at %d, the features have %d rows" % (pseg.rows, N))
        qseg = query_offsets if isinstance(query_offsets, E.Segments) else E.Segments(query_offsets)
        if qseg.rows != M:
            raise ValueError("interpolate: query_offsets end at %d, the query tower has %d rows" % (qseg.rows, M))
        if qseg.nseg != pseg.nseg:
            raise ValueError("interpolate: query_offsets name %d clouds, offsets %d" % (qseg.nseg, pseg.nseg))
        if k > pseg.min_n:
            raise ValueError("interpolate: k=%d exceeds the smallest candidate cloud (%d rows)" % (k, pseg.min_n))
    elif k > N:
        raise ValueError("interpolate: k=%d exceeds the N=%d points of a cloud" % (k, N))
    Cs = 0
    if skip is not None:
        Bs, Ms, Cs = _interp_rows(skip, "skip", packed, rank4=True)
        if (Bs, Ms) != (B, M):
            raise ValueError("interpolate: skip covers %d clouds of %d rows, the queries %d of %d" % (Bs, Ms, B, M))
        if Cs % 4 or Cs < 1:
            raise ValueError("interpolate: skip needs Cs %% 4 == 0 channels, got Cs=%d" % Cs)
    # ---- device work from here on
    if graph is None:
        idx, dist = k_nn(points, k, offsets=pseg, queries=queries, query_offsets=qseg, return_dist=True)
    else:
        idx, dist = graph
    f2d = E.as2d(features)[0]
    if skip is None:
        return E.rank4(E.interpolate(f2d, idx, dist, B, M, N, k, packed, eps), B, M)
    s2d = E.as2d(skip)[0]
    buf = E.ctx().new_buffer(B * M, F + Cs)
    E.interpolate(f2d, idx, dist, B, M, N, k, packed, eps, out=buf[:, :F])
    tail = buf[:, F:]
    H.call("dgcnn_copy2d_f32", s2d.data_ptr(), H.ld2(s2d), tail.data_ptr(), H.ld2(tail), B * M, Cs, 0)
    E_copy_grad(s2d, tail)
    return E.rank4(buf, B, M)


def _fps_counts(m, ratio, sizes, dense):
    """The sample count of every cloud, from m (an int for every cloud, or -- packed only -- one int per cloud) or ratio in (0, 1]"""
    if (m is None) == (ratio is None):
        raise ValueError("farthest_point_sample: exactly one of m and ratio is given (got %s)" % ("both" if m is not None else "neither"))
    if ratio is not None:
        ratio = float(ratio)
        if not (0.0 < ratio <= 1.0):
            raise ValueError("farthest_point_sample: ratio=%r must be in (0, 1]" % ratio)
        return [int(math.ceil(ratio * n)) for n in sizes]
    if isinstance(m, (list, tuple)) or (hasattr(m, "ndim") and getattr(m, "ndim") == 1):
        if dense:
            raise ValueError("farthest_point_sample: a dense call takes one m for every cloud, got a sequence")
        counts = [int(v) for v in m]
        if len(counts) != len(sizes):
            raise ValueError("farthest_point_sample: m holds %d counts, the tower has %d clouds" % (len(counts), len(sizes)))
    else:
        counts = [int(m)] * len(sizes)
    for b, (v, n) in enumerate(zip(counts, sizes)):
        if v < 1:
            raise ValueError("farthest_point_sample: m=%d must be at least 1" % v)
        if v > n:
            raise ValueError("farthest_point_sample: m=%d exceeds the %d rows of cloud %d" % (v, n, b))
    return counts


def farthest_point_sample(points, m=None, ratio=None, offsets=None, start=None, return_dist=False):
    """Farthest point sampling (PointNet++ set abstraction, PyG's fps): from every cloud the start row, then again and again the row
    farthest (squared L2) from the rows selected so far, ties -> the lower row (include/dgcnn_hip.h K7 states the arithmetic bit for
    bit).  One persistent workgroup per cloud walks the whole chain in one launch.
    Exactly one of m (samples per cloud) and ratio in (0, 1] (ceil(ratio * n) samples of a cloud of n rows, as PyG counts).
    Dense: points (B,N,C) -> idx (B,m) int32, cloud-local rows.
    Packed: points (R,C) or (1,R,C) with offsets (a sequence or a Segments); m an int for every cloud or one int per cloud ->
    (idx (S,) int32 rows of the tower, sample_offsets): sample_offsets is a Segments over the S samples, ready to be the
    query_offsets= of k_nn / interpolate for the sampled set.
    start: None (row 0 of every cloud), an int, or a host sequence of one cloud-local row per cloud.
    return_dist: appends dist, float32 in idx's shape: +inf for the start row, then the squared distance of every sample to the ones
    before it.  The result is m distinct rows whatever the input holds; rows with a non-finite coordinate are taken last.
    C <= 64.  No gradient: a selection, like k_nn."""
    packed = offsets is not None
    _, N, C = _rows_channels(points, "points", packed, who="farthest_point_sample")
    B = 1 if packed else points.shape[0]
    if C > E.FPS_MAX_C or C < 1:
        raise ValueError("farthest_point_sample: C=%d channels, the sampling takes 1 ... %d" % (C, E.FPS_MAX_C))
    seg = _segments(points, offsets, []) if packed else None
    sizes = [int(v) for v in (seg.host[1:] - seg.host[:-1])] if packed else [N] * B
    if not packed and (B < 1 or N < 1):
        raise ValueError("farthest_point_sample: points must hold at least one cloud of at least one row, got %s" % (tuple(points.shape),))
    counts = _fps_counts(m, ratio, sizes, not packed)
    if start is not None:
        st = [int(v) for v in start] if hasattr(start, "__len__") else [int(start)] * len(sizes)
        if len(st) != len(sizes):
            raise ValueError("farthest_point_sample: start holds %d rows, there are %d clouds" % (len(st), len(sizes)))
        for b, (v, n) in enumerate(zip(st, sizes)):
            if v < 0 or v >= n:
                raise ValueError("farthest_point_sample: start=%d is outside the %d rows of cloud %d" % (v, n, b))
        start = st
    # ---- device work from here on
    x2d = E.as2d(points)[0]
    if packed:
        soff = [0]
        for v in counts:
            soff.append(soff[-1] + v)
        sseg = E.Segments(soff)
        res = E.fps(x2d, 1, N, 0, seg=seg, sseg=sseg, start=start, want_dist=bool(return_dist))
        return (res[0], sseg, res[1]) if return_dist else (res, sseg)
    return E.fps(x2d, B, N, counts[0], start=start, want_dist=bool(return_dist))


def take_rows(x, idx, offsets=None):
    """The rows of x that idx names -- the sampled coordinates or features after farthest_point_sample.
    Dense: x (B,N,F) or (B,N,1,F), idx (B,m) int32 cloud-local -> (B,m,F) / (B,m,1,F).
    Packed: x (R,F), (1,R,F) or (1,R,1,F) with offsets (the tower's), idx (S,) int32 tower rows -> (S,F), (1,S,F) / (1,S,1,F).
    idx must hold DISTINCT rows per cloud (farthest_point_sample guarantees it): the backward writes every gradient row from one
    sample, without atomics.  Recorded, x receives the scatter of the result's gradient; idx carries none."""
    packed = offsets is not None
    shp = tuple(x.shape)
    B, N, F = _interp_rows(x, "x", packed, rank4=True, who="take_rows")
    ishp = tuple(idx.shape)
    if packed:
        seg = offsets if isinstance(offsets, E.Segments) else E.Segments(offsets)
        if seg.rows != N:
            raise ValueError("take_rows: offsets end at %d, x has %d rows" % (seg.rows, N))
        if len(ishp) != 1 or ishp[0] < 1:
            raise ValueError("take_rows: a packed idx is (S,), got %s" % (ishp,))
        M = ishp[0]
    else:
        if len(ishp) != 2 or ishp[0] != B or ishp[1] < 1 or ishp[1] > N:
            raise ValueError("take_rows: idx must be (B=%d, m <= N=%d), got %s" % (B, N, ishp))
        M = ishp[1]
    if idx.dtype != torch.int32:
        raise ValueError("take_rows: idx must be int32 (what farthest_point_sample returns), got %s" % idx.dtype)
    # ---- device work from here on
    y = E.take_rows(E.as2d(x)[0], idx, B, M, N, packed)
    if len(shp) == 4:
        return E.rank4(y, B, M)
    return y if len(shp) == 2 else y.view(B, M, F)


def edges(points, k=20, offsets=None):
    """dgcnn/ops.py:21-40.  (B,N,C) -> edge features (B,N,k,2C) = concat[x_i, x_j - x_i].  offsets: a packed tower (k_nn), (1,R,k,2C)."""
    idx = k_nn(points, k, offsets=offsets)
    x, B, N = E.as2d(points)
    C = x.shape[1]
    out = torch.empty((B, N, int(k), 2 * C), dtype=torch.float32, device=x.device)
    H.call("dgcnn_edge_gather_f32", x.data_ptr(), H.ld2(x), idx.data_ptr(), B, N, C, int(k), out.data_ptr())
    return out


def edge_conv(point_cloud, k, num_filters, trainable, activation=relu, debug=False, _outs=None, _net2=None, _seed=None,
              offsets=None, bn_per_cloud=False, bn_per_cloud_train=False):
    """dgcnn/ops.py:42-73.  Returns the list [net_max, net_mean, net], each (B,N,1,ch).
    _seed: the previous layer's neighbour graph (the stacks pass it): only speeds this layer's k-NN up.
    offsets: a packed tower (k_nn): the neighbours come from the row's own cloud, every other pass (BatchNorm included) runs over
    all R rows as in a dense tower; outputs (1,R,1,ch).
    bn_per_cloud (with offsets; forward only): both BatchNorms take the statistics of the row's own cloud, so a cloud's outputs do
    not depend on the other clouds of the tower.
    bn_per_cloud_train (with offsets): the same mode with its backward -- the call may be recorded."""
    seg = _segments(point_cloud, offsets, [k], bn_per_cloud, bn_per_cloud_train)
    x, B, N = E.as2d(point_cloud)
    F = int(num_filters)
    mm, net, idx = E.edge_conv_block(x, B, N, int(k), F, relu1=_is_relu(activation), outs=_outs, net2=_net2, seed=_seed, seg=seg)
    res = [E.rank4(mm[:, :F], B, N), E.rank4(mm[:, F:], B, N), E.rank4(net, B, N)]
    if debug:
        for t in res:
            print("Shape %s ... Name %s" % (tuple(t.shape), E.ctx().full_name("edge_conv")))
    edge_conv.last_idx = idx
    return res


build_edge_conv = edge_conv


def _listify(v, repeat, what):
    if isinstance(v, list):
        if len(v) != repeat:
            print("Length of %s != repeat" % what)
            raise ValueError("Length of %s != repeat" % what)     # ops.py:80-87
        return [int(a) for a in v]
    return [int(v)] * repeat


def repeat_edge_conv(point_cloud, repeat, k, num_filters, trainable, debug=False, _plan=None, offsets=None, bn_per_cloud=False,
                     bn_per_cloud_train=False):
    """dgcnn/ops.py:75-98.  Flat list of 3*repeat tensors; layer i+1 builds its k-NN graph on
    squeeze(tensors[-1]) -- the dynamic graph.  offsets / bn_per_cloud / bn_per_cloud_train: a packed tower (edge_conv)."""
    repeat = int(repeat)
    k = _listify(k, repeat, "k")
    num_filters = _listify(num_filters, repeat, "num_filters")
    seg = _segments(point_cloud, offsets, k, bn_per_cloud, bn_per_cloud_train)
    net = point_cloud
    tensors = []
    seed = None
    for i in range(repeat):
        with E.variable_scope("EdgeConv%d" % i):
            outs, net2 = _plan(i) if _plan is not None else (None, None)
            tensors += edge_conv(net, k[i], num_filters[i], trainable, debug=debug, _outs=outs, _net2=net2, _seed=seed,
                                 offsets=seg)
            seed = edge_conv.last_idx                    # layer i's graph seeds layer i + 1's search (same points)
            net = tensors[-1][:, :, 0, :]
    return tensors


def repeat_residual_edge_conv(point_cloud, repeat, k, num_filters, trainable, debug=False, _plan=None, offsets=None,
                              bn_per_cloud=False, bn_per_cloud_train=False):
    """dgcnn/ops.py:100-140.  Layers >= 1: conv1 without activation, optional shortcut conv when
    num_filters changes, tensors[-1] = relu(shortcut + tensors[-1]).  offsets / bn_per_cloud / bn_per_cloud_train: a packed tower
    (edge_conv)."""
    repeat = int(repeat)
    k = _listify(k, repeat, "k")
    num_filters = _listify(num_filters, repeat, "num_filters")
    seg = _segments(point_cloud, offsets, k, bn_per_cloud, bn_per_cloud_train)
    net = point_cloud
    tensors = []
    shortcut = None
    seed = None
    for i in range(repeat):
        with E.variable_scope("EdgeConv%d" % i):
            outs, net2 = _plan(i) if _plan is not None else (None, None)
            if shortcut is None:
                tensors += edge_conv(net, k[i], num_filters[i], trainable, debug=debug, _outs=outs, _net2=net2, _seed=seed,
                                     offsets=seg)
            else:
                # conv1 (no activation) goes to a scratch buffer; relu(shortcut + conv1) takes the planned slot
                tensors += edge_conv(net, k[i], num_filters[i], trainable, activation=None, debug=debug,
                                     _outs=None if outs is None else (outs[0], None), _seed=seed, offsets=seg)
                sc, B, N = E.as2d(shortcut)
                if not num_filters[i] == num_filters[i - 1]:
                    sc = E.conv_bn_act(sc, "shortcut", num_filters[i], relu=False, seg=seg)       # ops.py:125-133
                pre, _, _ = E.as2d(tensors[-1])
                res = E.add_relu(sc, pre, out=None if outs is None else outs[1])          # ops.py:134
                if net2 is not None:
                    H.call("dgcnn_copy2d_f32", res.data_ptr(), H.ld2(res), net2.data_ptr(), H.ld2(net2),
                           res.shape[0], res.shape[1], 0)
                    E_copy_grad(res, net2)
                tensors[-1] = E.rank4(res, B, N)
            seed = edge_conv.last_idx                    # layer i's graph seeds layer i + 1's search (same points)
            net = tensors[-1]
            shortcut = tensors[-1]
            net = net[:, :, 0, :]
    return tensors


def E_copy_grad(src, dst):
    """Backward of `dst = copy(src)`: d(src) += d(dst)."""
    c = E.ctx()
    if not c.recording:
        return

    def bwd():
        gd, gs = c.grad(dst), c.grad(src)
        if gd is not None and gs is not None:
            H.call("dgcnn_copy2d_f32", gd.data_ptr(), H.ld2(gd), gs.data_ptr(), H.ld2(gs), gd.shape[0], gd.shape[1], 1)
    c.tape.append(bwd)


def fc(net, repeat, num_filters, trainable, debug=False, offsets=None, bn_per_cloud=False, bn_per_cloud_train=False):
    """dgcnn/ops.py:142-163.  repeat x [1x1 conv + BN + ReLU] under scopes FC0, FC1, ...
    offsets: net is a packed tower (R,C), (1,R,C) or (1,R,1,C); bn_per_cloud (with offsets; forward only): every BatchNorm takes
    the statistics of the row's own cloud; bn_per_cloud_train: the same with its backward."""
    repeat = int(repeat)
    num_filters = _listify(num_filters, repeat, "num_filters")
    seg = _segments(net, offsets, [], bn_per_cloud, bn_per_cloud_train)
    x, B, N = E.as2d(net)
    for i in range(repeat):
        x = E.conv_bn_act(x, "FC%d" % i, num_filters[i], relu=True, seg=seg)
        if debug:
            print("Shape %s ... Name FC%d" % ((B, N, 1, num_filters[i]), i))
    return E.rank4(x, B, N)

"""-m gpu: the feature interpolation between two point sets (csrc/interp.hip) against its float32 restatement
(tests/interp_reference.py), BIT FOR BIT -- the arithmetic is normative (include/dgcnn_hip.h K6) -- through the C ABI with guarded
buffers, and through dgcnn.ops.interpolate under a recording.  Distances and indices of the ABI cases come from the k-NN's own
arithmetic on the host (tests/knn_cross_reference.py)."""
import functools

import numpy as np
import pytest
import torch

from gpu_helpers import dev, host, Guard, SENT
import interp_reference as R
import knn_cross_reference as KR

pytestmark = pytest.mark.gpu

EPS = 1e-16
FS = (4, 68, 256, 1024)
KS = (1, 3, 8, 64)
DENSE = ((1, 1, 1), (2, 65, 3), (1, 257, 65), (3, 64, 129))                  # (B, M, N)
PACKED = ((1, 65, 300), (3, 64, 129))                                       # query clouds against candidate clouds


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def same_bits(x, y):
    return x.shape == y.shape and np.array_equal(bits(x), bits(y))


@functools.lru_cache(maxsize=None)
def dense_graph(B, M, N, k):
    """(idx (B, M, k) cloud-local, dist (B, M, k)); every other query is a copy of a candidate"""
    rng = np.random.default_rng(100 * B + M + N + k)
    p = rng.random((B, N, 3), dtype=np.float32)
    q = rng.random((B, M, 3), dtype=np.float32)
    for b in range(B):
        q[b, ::2] = p[b, rng.integers(0, N, len(q[b, ::2]))]
    return KR.cross_knn_batch(q, p, k)


@functools.lru_cache(maxsize=None)
def packed_graph(k):
    """(idx (Q, k) rows of the candidate tower, dist (Q, k), Q, P) of the packed pair"""
    rng = np.random.default_rng(17 + k)
    rows, dists, p0 = [], [], 0
    for m, n in zip(*PACKED):
        p = rng.random((n, 3), dtype=np.float32)
        q = rng.random((m, 3), dtype=np.float32)
        q[::2] = p[rng.integers(0, n, len(q[::2]))]
        i, d = KR.cross_knn(q, p, k)
        rows.append(i + p0)
        dists.append(d)
        p0 += n
    return np.concatenate(rows).astype(np.int32), np.concatenate(dists), sum(PACKED[0]), sum(PACKED[1])


def widen(x, ld, fill=SENT):
    """x (rows, F) inside a (rows, ld) array whose other columns hold `fill`"""
    out = np.full((x.shape[0], ld), fill, np.float32)
    out[:, :x.shape[1]] = x
    return out


def H():
    from dgcnn import _hip
    return _hip


def forward(g, feat, idx_arg, dist, q_rows, p_rows, M, N, k, F, eps=EPS, want_a=True, pad=(4, 8)):
    """dgcnn_interp_f32 on guarded buffers with ld > F on feat and y -> (y (q_rows, F), a (q_rows, k) or None, device a or None)"""
    ldf, ldy = F + pad[0], F + pad[1]
    fd = g.put(widen(feat, ldf))
    yd = g.new((q_rows, ldy))
    ad = g.new((q_rows, k)) if want_a else None
    H().call("dgcnn_interp_f32", fd.data_ptr(), ldf, g.put(idx_arg.astype(np.int32)).data_ptr(), g.put(dist.astype(np.float32)).data_ptr(),
             q_rows, p_rows, M, N, k, F, eps, 0 if ad is None else ad.data_ptr(), yd.data_ptr(), ldy)
    y = host(yd)
    assert (y[:, F:] == SENT).all(), "the forward wrote beyond column F of y"
    return y[:, :F].copy(), None if ad is None else host(ad), ad


def backward(g, dy, idx_arg, ad, q_rows, p_rows, M, N, k, F, d0, beta, pad=(12, 4)):
    """dgcnn_interp_bwd_f32 on guarded buffers with ld > F on dy and dfeat, dfeat pre-filled with d0 -> dfeat (p_rows, F)"""
    lddy, lddf = F + pad[0], F + pad[1]
    nws = int(H().load().dgcnn_interp_bwd_workspace_bytes(q_rows, p_rows, k))
    assert nws > 0 and nws % 4 == 0
    ws = g.new((nws // 4,), dtype=torch.int32, fill=777)
    dd = g.put(widen(d0, lddf))
    H().call("dgcnn_interp_bwd_f32", g.put(widen(dy, lddy)).data_ptr(), lddy, g.put(idx_arg.astype(np.int32)).data_ptr(), ad.data_ptr(),
             q_rows, p_rows, M, N, k, F, dd.data_ptr(), lddf, beta, ws.data_ptr(), nws)
    d = host(dd)
    assert (d[:, F:] == SENT).all(), "the backward wrote beyond column F of dfeat"
    return d[:, :F].copy()


def check_all(idx_arg, rows, dist, q_rows, p_rows, M, N, k, F, seed=0):
    """forward (with and without a), backward at beta = 0 and beta = 1 on a pre-filled dfeat: all bit-equal to the restatement"""
    rng = np.random.default_rng(seed + F + k)
    feat = rng.standard_normal((p_rows, F)).astype(np.float32)
    dy = rng.standard_normal((q_rows, F)).astype(np.float32)
    d0 = rng.standard_normal((p_rows, F)).astype(np.float32)
    a_ref, y_ref = R.interp_f32(feat, rows, dist, EPS)
    g = Guard()
    y, a, ad = forward(g, feat, idx_arg, dist, q_rows, p_rows, M, N, k, F)
    assert same_bits(a, a_ref), "a: %d of %d words differ" % ((bits(a) != bits(a_ref)).sum(), a.size)
    assert same_bits(y, y_ref), "y: %d of %d words differ" % ((bits(y) != bits(y_ref)).sum(), y.size)
    y2, _, _ = forward(g, feat, idx_arg, dist, q_rows, p_rows, M, N, k, F, want_a=False, pad=(0, 4))
    assert same_bits(y2, y_ref), "y with a = NULL"
    d = backward(g, dy, idx_arg, ad, q_rows, p_rows, M, N, k, F, d0, 0)
    ref0 = R.interp_bwd_f32(a_ref, rows, dy, p_rows)
    assert same_bits(d, ref0), "dfeat (beta = 0): %d of %d words differ" % ((bits(d) != bits(ref0)).sum(), d.size)
    d = backward(g, dy, idx_arg, ad, q_rows, p_rows, M, N, k, F, d0, 1, pad=(0, 8))
    assert same_bits(d, R.interp_bwd_f32(a_ref, rows, dy, p_rows, dfeat0=d0)), "dfeat (beta = 1)"
    g.check()


DENSE_CASES = [(s, k) for s in DENSE for k in KS if k <= s[2]]


@pytest.mark.parametrize("shape,k", DENSE_CASES, ids=["B%d-M%d-N%d-k%d" % (s + (k,)) for s, k in DENSE_CASES])
def test_dense_bit_equal_to_the_restatement(shape, k):
    B, M, N = shape
    idx, dist = dense_graph(B, M, N, k)
    rows = R.tower_rows(idx, N)
    for F in FS:
        check_all(idx.reshape(B * M, k), rows, dist.reshape(B * M, k), B * M, B * N, M, N, k, F)


@pytest.mark.parametrize("k", [k for k in KS if k <= min(PACKED[1])])
def test_packed_bit_equal_to_the_restatement(k):
    rows, dist, Q, P = packed_graph(k)
    for F in FS:
        check_all(rows, rows, dist, Q, P, 0, 0, k, F, seed=3)


def test_heavy_buckets_are_reproducible():
    """N = k = 3, M = 4096: every candidate has in-degree 4096 (the quadratic rank step at its worst per edge); 5 runs, the same bits"""
    M, N, k, F = 4096, 3, 3, 8
    idx, dist = dense_graph(1, M, N, k)
    idx, dist = idx[0], dist[0]
    assert (np.bincount(idx.ravel(), minlength=N) == M).all()
    rng = np.random.default_rng(1)
    feat = rng.standard_normal((N, F)).astype(np.float32)
    dy = rng.standard_normal((M, F)).astype(np.float32)
    a_ref, y_ref = R.interp_f32(feat, idx, dist, EPS)
    ref = R.interp_bwd_f32(a_ref, idx, dy, N)
    g = Guard()
    y, a, ad = forward(g, feat, idx, dist, M, N, M, N, k, F)
    assert same_bits(y, y_ref) and same_bits(a, a_ref)
    for run in range(5):
        d = backward(g, dy, idx, ad, M, N, M, N, k, F, np.zeros((N, F), np.float32), 0)
        assert same_bits(d, ref), "run %d" % run
    g.check()


def test_more_candidate_rows_than_one_scan_round():
    """p_rows = 9003: the one-block scan of the bucket sizes takes 4096 a round -- two full rounds, a partial one, a tail that is no
    multiple of 4; most buckets empty, some shared"""
    Q, P, k, F = 3001, 9003, 3, 4
    rng = np.random.default_rng(21)
    idx = np.stack([rng.choice(P, k, replace=False) for _ in range(Q)]).astype(np.int32)
    idx[::7, 0] = P - 1                                                   # the last bucket is used, and heavy
    idx[::7, 1] = 4096
    idx[::7, 2] = 4095
    dist = rng.random((Q, k), dtype=np.float32)
    check_all(idx, idx, dist, Q, P, 0, 0, k, F, seed=22)


def test_candidates_without_incoming_edges():
    """rows nobody interpolates from receive 0 (beta = 0) or stay as they were (beta = 1)"""
    Q, P, k, F = 37, 12, 2, 8
    rng = np.random.default_rng(2)
    idx = np.stack([rng.permutation(5)[:k] * 2 for _ in range(Q)]).astype(np.int32)          # rows 0, 2, 4, 6, 8 only
    dist = rng.random((Q, k), dtype=np.float32)
    feat = rng.standard_normal((P, F)).astype(np.float32)
    dy = rng.standard_normal((Q, F)).astype(np.float32)
    d0 = rng.standard_normal((P, F)).astype(np.float32)
    a_ref, y_ref = R.interp_f32(feat, idx, dist, EPS)
    g = Guard()
    y, a, ad = forward(g, feat, idx, dist, Q, P, 0, 0, k, F)
    assert same_bits(y, y_ref)
    d = backward(g, dy, idx, ad, Q, P, 0, 0, k, F, d0, 0)
    lone = [1, 3, 5, 7, 9, 10, 11]
    assert same_bits(d, R.interp_bwd_f32(a_ref, idx, dy, P)) and (d[lone] == 0).all() and np.abs(d[::2][:5]).min() > 0
    d = backward(g, dy, idx, ad, Q, P, 0, 0, k, F, d0, 1)
    assert same_bits(d, R.interp_bwd_f32(a_ref, idx, dy, P, dfeat0=d0)) and same_bits(d[lone], d0[lone])
    g.check()


def test_nonfinite_and_negative_distances():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    P, k, F = 6, 3, 8
    idx = np.array([[0, 1, 2], [3, 4, 5], [1, 3, 5], [0, 2, 4], [5, 4, 3], [2, 1, 0]], np.int32)
    dist = np.array([[inf, inf, inf],                      # a whole row of +inf: y = 0, no gradient
                     [0.25, nan, inf],
                     [0.5, 0.5, nan],
                     [-inf, -1.0, 1e-20],
                     [-3e-8, 0.0, 2.0],
                     [nan, nan, nan]], np.float32)
    Q = len(idx)
    rng = np.random.default_rng(4)
    feat = rng.standard_normal((P, F)).astype(np.float32)
    dy = rng.standard_normal((Q, F)).astype(np.float32)
    a_ref, y_ref = R.interp_f32(feat, idx, dist, EPS)
    g = Guard()
    y, a, ad = forward(g, feat, idx, dist, Q, P, 0, 0, k, F)
    assert same_bits(a, a_ref) and same_bits(y, y_ref)
    assert (y[0] == 0).all() and (y[5] == 0).all() and (a[0] == 0).all() and np.isfinite(y).all()
    assert same_bits(y[1], feat[3])
    d = backward(g, dy, idx, ad, Q, P, 0, 0, k, F, np.zeros((P, F), np.float32), 0)
    assert same_bits(d, R.interp_bwd_f32(a_ref, idx, dy, P))
    assert same_bits(d, R.interp_bwd_f32(a_ref[1:5], idx[1:5], dy[1:5], P))          # the rows without a finite distance: nothing
    # another clamp: every distance below eps = 0.5 weighs 2
    y2, a2, _ = forward(g, feat, idx, dist, Q, P, 0, 0, k, F, eps=0.5)
    a_ref2, y_ref2 = R.interp_f32(feat, idx, dist, 0.5)
    assert same_bits(a2, a_ref2) and same_bits(y2, y_ref2) and not same_bits(a2, a_ref)
    g.check()


# ---------------------------------------------------------------------------------------------------------------
# through dgcnn.ops.interpolate
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture
def dg():
    import dgcnn
    dgcnn.reset()
    yield dgcnn
    dgcnn.ctx().recording = False
    dgcnn.reset()


def clouds(B, M, N, seed):
    rng = np.random.default_rng(seed)
    p = rng.random((B, N, 3), dtype=np.float32)
    q = rng.random((B, M, 3), dtype=np.float32)
    q[:, ::3] = p[:, np.arange(len(q[0, ::3])) % N]              # every third query sits on a candidate
    return q, p


def tracked(c, a2d):
    """a tracked root holding a2d: its gradient is collected"""
    assert c.recording
    t = c.new_buffer(*a2d.shape)
    t.copy_(dev(a2d))
    return t


def test_ops_forward_backward_under_a_recording(dg):
    from dgcnn import _engine as E
    B, M, N, k, F = 2, 131, 37, 3, 20
    q, p = clouds(B, M, N, 5)
    rng = np.random.default_rng(6)
    feat = rng.standard_normal((B * N, F)).astype(np.float32)
    dy = rng.standard_normal((B * M, F)).astype(np.float32)
    c = dg.ctx()
    c.begin_step()
    c.recording = True
    f = tracked(c, feat)
    out = dg.ops.interpolate(f.view(B, N, F), dev(p), dev(q), k=k)
    assert tuple(out.shape) == (B, M, 1, F)
    idx, dist = dg.ops.k_nn(dev(p), k, queries=dev(q), return_dist=True)
    ref_idx, ref_dist = KR.cross_knn_batch(q, p, k)
    assert np.array_equal(host(idx), ref_idx) and same_bits(host(dist), ref_dist)
    rows = R.tower_rows(host(idx), N)
    a_ref, y_ref = R.interp_f32(feat, rows, host(dist).reshape(B * M, k), EPS)
    assert same_bits(host(out).reshape(B * M, F), y_ref)
    c.grad(E.as2d(out)[0]).copy_(dev(dy))
    c.backward()
    zero = np.zeros((B * N, F), np.float32)
    assert same_bits(host(c.grad(f)), R.interp_bwd_f32(a_ref, rows, dy, B * N, dfeat0=zero))


def test_ops_graph_reuse_gives_the_same_bits(dg):
    B, M, N, k, F = 2, 70, 33, 4, 8
    q, p = clouds(B, M, N, 7)
    feat = dev(np.random.default_rng(8).standard_normal((B, N, F)).astype(np.float32))
    inner = dg.ops.interpolate(feat, dev(p), dev(q), k=k, eps=1e-12)
    graph = dg.ops.k_nn(dev(p), k, queries=dev(q), return_dist=True)
    assert same_bits(host(dg.ops.interpolate(feat, None, None, k=k, eps=1e-12, graph=graph)), host(inner))
    assert same_bits(host(dg.ops.interpolate(feat.view(B, N, 1, F), dev(p), dev(q), k=k, eps=1e-12, graph=graph)), host(inner))
    assert not same_bits(host(dg.ops.interpolate(feat, None, None, k=k, eps=1e-2, graph=graph)), host(inner))     # eps is used


def test_ops_skip_connection_lands_in_one_buffer(dg):
    from dgcnn import _engine as E
    B, M, N, k, F, Cs = 2, 45, 19, 3, 12, 8
    q, p = clouds(B, M, N, 9)
    rng = np.random.default_rng(10)
    feat = rng.standard_normal((B * N, F)).astype(np.float32)
    skip = rng.standard_normal((B * M, Cs)).astype(np.float32)
    dy = rng.standard_normal((B * M, F + Cs)).astype(np.float32)
    c = dg.ctx()
    c.begin_step()
    c.recording = True
    f, s = tracked(c, feat), tracked(c, skip)
    out = dg.ops.interpolate(f.view(B, N, F), dev(p), dev(q), k=k, skip=s.view(B, M, Cs))
    assert tuple(out.shape) == (B, M, 1, F + Cs)
    o2 = E.as2d(out)[0]
    assert o2.stride(0) == F + Cs                                      # one buffer, no concat pass
    idx, dist = dg.ops.k_nn(dev(p), k, queries=dev(q), return_dist=True)
    rows = R.tower_rows(host(idx), N)
    a_ref, y_ref = R.interp_f32(feat, rows, host(dist).reshape(B * M, k), EPS)
    o = host(out).reshape(B * M, F + Cs)
    assert same_bits(o[:, :F], y_ref) and same_bits(o[:, F:], skip)
    c.grad(o2).copy_(dev(dy))
    c.backward()
    assert same_bits(host(c.grad(f)), R.interp_bwd_f32(a_ref, rows, dy[:, :F], B * N, dfeat0=np.zeros((B * N, F), np.float32)))
    assert same_bits(host(c.grad(s)), dy[:, F:] + np.float32(0))


def test_ops_two_interpolations_accumulate_their_gradients(dg):
    from dgcnn import _engine as E
    B, N, F = 1, 29, 8
    (q1, p), (q2, _) = clouds(B, 50, N, 11), clouds(B, 77, N, 12)
    q2[0, ::3] = p[0, np.arange(len(q2[0, ::3])) % N]
    rng = np.random.default_rng(13)
    feat = rng.standard_normal((N, F)).astype(np.float32)
    dy1 = rng.standard_normal((50, F)).astype(np.float32)
    dy2 = rng.standard_normal((77, F)).astype(np.float32)
    c = dg.ctx()
    c.begin_step()
    c.recording = True
    f = tracked(c, feat)
    o1 = dg.ops.interpolate(f.view(B, N, F), dev(p), dev(q1), k=3)
    o2 = dg.ops.interpolate(f.view(B, N, F), dev(p), dev(q2), k=5)
    c.grad(E.as2d(o1)[0]).copy_(dev(dy1))
    c.grad(E.as2d(o2)[0]).copy_(dev(dy2))
    c.backward()
    refs = []
    for q, k in ((q1, 3), (q2, 5)):
        idx, dist = KR.cross_knn(q[0], p[0], k)
        refs.append((R.interp_f32(feat, idx, dist, EPS)[0], idx))
    first = R.interp_bwd_f32(refs[1][0], refs[1][1], dy2, N, dfeat0=np.zeros((N, F), np.float32))     # the tape runs in reverse
    assert same_bits(host(c.grad(f)), R.interp_bwd_f32(refs[0][0], refs[0][1], dy1, N, dfeat0=first))


def test_ops_dense_equals_packed(dg):
    """B equal-sized clouds: the dense call and the packed call of the same clouds give the same bits, forward and backward"""
    from dgcnn import _engine as E
    B, M, N, k, F = 3, 41, 23, 3, 16
    q, p = clouds(B, M, N, 14)
    rng = np.random.default_rng(15)
    feat = rng.standard_normal((B * N, F)).astype(np.float32)
    dy = rng.standard_normal((B * M, F)).astype(np.float32)
    res = []
    for packed in (False, True):
        c = dg.ctx()
        c.begin_step()
        c.recording = True
        f = tracked(c, feat)
        if packed:
            out = dg.ops.interpolate(f, dev(p.reshape(B * N, 3)), dev(q.reshape(B * M, 3)), k=k,
                                     offsets=[b * N for b in range(B + 1)], query_offsets=[b * M for b in range(B + 1)])
            assert tuple(out.shape) == (1, B * M, 1, F)
        else:
            out = dg.ops.interpolate(f.view(B, N, F), dev(p), dev(q), k=k)
        c.grad(E.as2d(out)[0]).copy_(dev(dy))
        c.backward()
        res.append((host(out).reshape(B * M, F), host(c.grad(f)).copy()))
        c.recording = False
    assert same_bits(res[0][0], res[1][0]) and same_bits(res[0][1], res[1][1])
    assert np.abs(res[0][1]).max() > 0

"""-m gpu: farthest point sampling and the row take (csrc/fps.hip) against their float32 restatement (tests/fps_reference.py), BIT FOR
BIT -- the arithmetic is normative (include/dgcnn_hip.h K7) -- through the C ABI with guarded buffers (ld > C, sentinel columns), and
through dgcnn.ops under a recording.  The two kernel forms return the same bits by design: the recorded kernel names tell which ran."""
import functools

import numpy as np
import pytest
import torch

from gpu_helpers import dev, host, Guard, SENT
import fps_reference as R
import interp_reference as IR
import knn_cross_reference as KR
import launch_trace as LT

pytestmark = pytest.mark.gpu

NAN, INF = np.float32(np.nan), np.float32(np.inf)
TOWER = ((1, 65, 300, 1024), (1, 65, 7, 64))                    # rows of the clouds, samples of the clouds


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def same_bits(x, y):
    return x.shape == y.shape and np.array_equal(bits(x), bits(y))


def H():
    from dgcnn import _hip
    return _hip


def limit(C):
    return int(H().load().dgcnn_fps_resident_max_n(C))


def widen(x, ld, fill=SENT):
    out = np.full((x.shape[0], ld), fill, np.float32)
    out[:, :x.shape[1]] = x
    return out


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def fps_call(x, nseg, max_n, max_m, samples, x_off=None, s_off=None, start=None, want_dist=True, pad=2, base_off=0):
    """dgcnn_fps_f32 on guarded buffers, x (rows, C) inside rows of C + pad floats -> (idx, dist or None, the launches)"""
    rows, C = x.shape
    g = Guard()
    xd = g.put(widen(x, C + pad), off=base_off)
    idx = g.new((samples,), dtype=torch.int32, fill=-7)
    dist = g.new((samples,)) if want_dist else None
    nws = int(H().load().dgcnn_fps_workspace_bytes(rows, C, max_n))
    ws = g.new((nws // 4,)) if nws else None
    xo = None if x_off is None else g.put(np.asarray(x_off, np.int32))
    so = None if s_off is None else g.put(np.asarray(s_off, np.int32))
    st = None if start is None else g.put(np.asarray(start, np.int32))
    p = lambda t: 0 if t is None else t.data_ptr()
    with LT.launches() as L:
        H().call("dgcnn_fps_f32", xd.data_ptr(), C + pad, C, nseg, p(xo), p(so), rows, samples, max_n, max_m, p(st), idx.data_ptr(),
                 p(dist), p(ws), nws)
    g.check()
    assert (host(xd)[:, C:] == SENT).all()
    return host(idx), None if dist is None else host(dist), L


def dense_check(x, m, form, start=None, ref=None, **kw):
    """x (B, n, C): the dense call at m samples is the restatement's (or the first m of `ref`, by the prefix property)"""
    B, n, C = x.shape
    ri, rd = R.fps_dense(x, m, start) if ref is None else (ref[0][:, :m], ref[1][:, :m])
    idx, dist, L = fps_call(x.reshape(B * n, C), B, n, m, B * m, start=start, **kw)
    assert np.array_equal(idx.reshape(B, m), ri), "n=%d m=%d C=%d: idx differs" % (n, m, C)
    assert same_bits(dist.reshape(B, m), rd), "n=%d m=%d C=%d: dist differs" % (n, m, C)
    names = LT.names(L)
    want = {"resident": ["fps_resident_kernel"], "streaming": ["fps_stream_kernel"]}[form]     # a dense call: one form, one launch
    assert names == want, (names, form)
    return L


@functools.lru_cache(maxsize=None)
def cloud(B, n, C, seed=0):
    """coordinates in [0, 1) on a 2^-6 grid in every second cloud row block: plenty of exact ties and duplicates"""
    rng = np.random.default_rng(seed + 7 * n + C)
    x = rng.random((B, n, C), dtype=np.float32)
    x[:, ::3] = np.round(x[:, ::3] * 64) / 64
    return x


def counts_for(n):
    return sorted({m for m in (1, 2, 64) if m <= n} | ({n} if n <= 300 else set()))


@pytest.mark.parametrize("C", [1, 3, 4])
def test_resident_form_bit_equal_to_the_restatement(C):
    for n in (1, 63, 64, 65, 1023, 1024, 1025, 4097):
        x = cloud(2, n, C)
        ms = counts_for(n)
        ref = R.fps_dense(x, ms[-1])
        for m in ms:
            L = dense_check(x, m, "resident", ref=ref)
        P = 1 if n <= 1024 else 2 if n <= 2048 else 4 if n <= 4096 else 8
        LT.assert_launched(L, "fps_resident_kernel", [C, P])


@pytest.mark.parametrize("C", [1, 3, 4])
def test_resident_form_at_its_largest_cloud(C):
    n = limit(C)
    assert n >= 1024
    L = dense_check(cloud(1, n, C), 8, "resident", start=[n - 1])
    assert L[0][3] == (1024, 1, 1) and L[0][2] == (1, 1, 1)


def test_streaming_form_one_row_above_the_resident_limit():
    n = limit(3) + 1
    x = cloud(1, n, 3)
    L = dense_check(x, 8, "streaming", start=[n - 1])
    LT.assert_launched(L, "fps_stream_kernel", [3])
    # the cloud one row shorter goes to the other form
    ri, rd = R.fps_dense(x[:, :n - 1], 8, [5])
    dense_check(x[:, :n - 1], 8, "resident", start=[5], ref=(ri, rd))


@pytest.mark.parametrize("C", [5, 16, 64])
def test_streaming_form_wide_rows(C):
    assert limit(C) == 0
    for n in (65, 1025):
        x = cloud(2, n, C)
        ms = counts_for(n)
        ref = R.fps_dense(x, ms[-1])
        for m in ms:
            L = dense_check(x, m, "streaming", ref=ref, pad=3)
        LT.assert_launched(L, "fps_stream_kernel", [0])


def tower(sizes, C, seed):
    rng = np.random.default_rng(seed)
    x = rng.random((int(sum(sizes)), C), dtype=np.float32)
    x[::3] = np.round(x[::3] * 64) / 64
    return x


def test_packed_tower():
    sizes, counts = TOWER
    x = tower(sizes, 3, 1)
    xo, so = offsets(sizes), offsets(counts)
    for start in (None, [0, 64, 5, 1023]):
        ri, rd = R.fps_packed(x, xo, counts, start)
        idx, dist, L = fps_call(x, 4, max(sizes), max(counts), int(so[-1]), xo, so, start=start)
        assert np.array_equal(idx, ri) and same_bits(dist, rd)
        assert LT.names(L) == ["fps_resident_kernel"] and L[0][2] == (4, 1, 1)
    # a start outside its cloud counts as 0 (the C entry cannot see it; dgcnn.ops refuses it on the host); dist = NULL
    ri, _ = R.fps_packed(x, xo, counts, [0, 65, -1, 1 << 20])
    assert np.array_equal(ri, R.fps_packed(x, xo, counts, [0, 0, 0, 0])[0])
    idx, dist, _ = fps_call(x, 4, max(sizes), max(counts), int(so[-1]), xo, so, start=[0, 65, -1, 1 << 20], want_dist=False, base_off=1)
    assert dist is None and np.array_equal(idx, ri)


def test_packed_tower_with_both_forms_in_one_call():
    sizes, counts = (65, limit(3) + 1, 300, 1), (65, 8, 7, 1)
    x = tower(sizes, 3, 2)
    xo, so = offsets(sizes), offsets(counts)
    start = [3, limit(3), 0, 0]
    ri, rd = R.fps_packed(x, xo, counts, start)
    idx, dist, L = fps_call(x, 4, max(sizes), max(counts), int(so[-1]), xo, so, start=start)
    assert np.array_equal(idx, ri) and same_bits(dist, rd)
    assert LT.names(L) == ["fps_resident_kernel", "fps_stream_kernel"]
    LT.assert_launched(L, "fps_resident_kernel", [3, 16])
    LT.assert_launched(L, "fps_stream_kernel", [3])


def test_a_cloud_sampled_beyond_its_size_is_clamped():
    """the Python layer refuses it; the kernels write the cloud's n rows and -1 into the rest, in both forms"""
    for C in (3, 5):
        sizes, counts = (5, 40), (9, 4)
        x = tower(sizes, C, 3)
        idx, dist, _ = fps_call(x, 2, 40, 9, 13, offsets(sizes), offsets(counts))
        ri, rd = R.fps_packed(x, offsets(sizes), (5, 4))
        assert np.array_equal(idx[:5], ri[:5]) and (idx[5:9] == -1).all() and np.array_equal(idx[9:], ri[5:])
        assert same_bits(dist[:5], rd[:5]) and (dist[5:9] == -1).all() and same_bits(dist[9:], rd[5:])


def both_forms(x, m, start=None):
    """one cloud x (n, 3) through the resident form, and with two zero channels appended (the same distances) through the streaming one"""
    ri, rd = R.fps_f32(x, m, 0 if start is None else start)
    st = None if start is None else [start]
    dense_check(x[None], m, "resident", start=st, ref=(ri[None], rd[None]))
    x5 = np.concatenate([x, np.zeros((len(x), 2), np.float32)], 1)
    r5 = R.fps_f32(x5, m, 0 if start is None else start)
    assert np.array_equal(r5[0], ri) and same_bits(r5[1], rd)
    dense_check(x5[None], m, "streaming", start=st, ref=(ri[None], rd[None]))
    return ri, rd


def test_adversarial_ties_and_duplicates():
    ri, rd = both_forms(R.lattice(4), 64)
    assert ri[1] == 63 and len(set(ri.tolist())) == 64
    ri, rd = both_forms(np.tile(np.array([[1, 2, 3]], np.float32), (100, 1)), 100)
    assert ri.tolist() == list(range(100)) and (rd[1:] == 0).all()
    ri, rd = both_forms(np.tile(np.array([[1, 2, 3]], np.float32), (1500, 1)), 64, start=1499)
    assert ri.tolist() == [1499] + list(range(63))


@pytest.mark.parametrize("bad", [(NAN, 0.0, 0.0), (0.0, INF, 0.0), (INF, 0.0, -INF)], ids=["nan", "inf", "both-infs"])
def test_adversarial_bad_rows(bad):
    base = np.random.default_rng(4).random((65, 3), dtype=np.float32)
    for pos in (0, 31, 64):
        x = base.copy()
        x[pos] = bad
        ri, rd = both_forms(x, 65, start=1 if pos == 0 else None)
        assert ri[-1] == pos and rd[-1] == 0 and sorted(ri.tolist()) == list(range(65))
        ri, rd = both_forms(x, 65, start=pos)                      # the bad row as the start row
        assert ri[0] == pos and rd[0] == 0 and rd[1] == INF
    x = base.copy()
    x[[0, 31, 64]] = bad
    ri, rd = both_forms(x, 65, start=2)
    assert ri[-3:].tolist() == [0, 31, 64]


def test_adversarial_overflowing_squares():
    rng = np.random.default_rng(6)
    x = ((rng.random((300, 3), dtype=np.float32) * 2 - 1) * np.float32(3e38)).astype(np.float32)
    x[::4] *= np.float32(1e-20)
    ri, rd = both_forms(x, 300)
    assert np.isinf(rd).sum() > 1 and np.isfinite(rd).sum() > 1 and sorted(ri.tolist()) == list(range(300))


# ---------------------------------------------------------------------------------------------------------------
# the row take and its backward
# ---------------------------------------------------------------------------------------------------------------
def distinct_rows(B, M, N, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(N)[:M] for _ in range(B)]).astype(np.int32)


def take_check(idx_arg, rows, s_rows, x_rows, M, N, F, pads, base_off=0, seed=0):
    """gather, scatter at beta = 0 and beta = 1 on a pre-filled dx: bit-equal to the restatement, sentinel columns intact"""
    rng = np.random.default_rng(seed + F)
    x = rng.standard_normal((x_rows, F)).astype(np.float32)
    dy = rng.standard_normal((s_rows, F)).astype(np.float32)
    d0 = rng.standard_normal((x_rows, F)).astype(np.float32)
    g = Guard()
    ldx, ldy = F + pads[0], F + pads[1]
    xd, yd = g.put(widen(x, ldx), off=base_off), g.new((s_rows, ldy), off=base_off)
    ii = g.put(idx_arg.astype(np.int32).reshape(-1))
    with LT.launches() as L:
        H().call("dgcnn_rows_gather_f32", xd.data_ptr(), ldx, ii.data_ptr(), s_rows, x_rows, M, N, F, yd.data_ptr(), ldy)
    vec = F % 4 == 0 and ldx % 4 == 0 and ldy % 4 == 0 and base_off % 4 == 0
    LT.check_kernels(L, [("rows_gather_kernel", ["true" if vec else "false"])], "gather F=%d" % F)
    y = host(yd)
    assert (y[:, F:] == SENT).all() and same_bits(y[:, :F], R.take_rows(x, rows))
    for beta in (0, 1):
        dd = g.put(widen(d0, ldx), off=base_off)
        dyd = g.put(widen(dy, ldy), off=base_off)
        with LT.launches() as L:
            H().call("dgcnn_rows_scatter_f32", dyd.data_ptr(), ldy, ii.data_ptr(), s_rows, x_rows, M, N, F, dd.data_ptr(), ldx, beta)
        assert LT.names(L) == (["rows_zero_kernel"] if beta == 0 else []) + ["rows_scatter_kernel"]
        d = host(dd)
        assert (d[:, F:] == SENT).all(), "the scatter wrote beyond column F"
        assert same_bits(d[:, :F], R.scatter_rows(dy, rows, x_rows, d0 if beta else None)), "scatter beta=%d F=%d" % (beta, F)
    g.check()


@pytest.mark.parametrize("F", [1, 3, 4, 68, 1024])
def test_take_and_scatter_bit_equal_to_the_restatement(F):
    for B, M, N in ((1, 1, 1), (2, 65, 129), (3, 64, 64)):
        idx = distinct_rows(B, M, N, 10 * B + M)
        for pads in ((4, 8), (0, 0)):
            take_check(idx, R.tower_rows(idx, N), B * M, B * N, M, N, F, pads)
    sizes, counts = TOWER
    xo = offsets(sizes)
    rows = np.concatenate([xo[b] + np.random.default_rng(b).permutation(sizes[b])[:counts[b]] for b in range(4)]).astype(np.int32)
    for pads in ((4, 8), (0, 0)):
        take_check(rows, rows, len(rows), int(xo[-1]), 0, 0, F, pads, seed=5)


def test_take_of_coordinates_from_a_misaligned_base():
    idx = distinct_rows(2, 65, 129, 3)
    for base_off in (0, 1, 3):
        take_check(idx, R.tower_rows(idx, 129), 130, 258, 65, 129, 3, (1, 0), base_off=base_off)
        take_check(idx, R.tower_rows(idx, 129), 130, 258, 65, 129, 4, (0, 0), base_off=base_off)      # F = 4 on the scalar path


# ---------------------------------------------------------------------------------------------------------------
# through dgcnn.ops: farthest_point_sample -> take_rows -> k_nn between the two sets -> interpolate back onto the full set
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture
def dg():
    import dgcnn
    dgcnn.reset()
    yield dgcnn
    dgcnn.ctx().recording = False
    dgcnn.reset()


def pipeline(dg, pts, feat, dy, m, k, off=None, start=None):
    """-> (idx, dist, sampled coordinates, sampled features, graph idx, graph dist, output, d(feat)) on the host"""
    from dgcnn import _engine as E
    c = dg.ctx()
    c.begin_step()
    c.recording = True
    f = c.new_buffer(*feat.shape)
    f.copy_(dev(feat))
    p = dev(pts)
    if off is None:
        B, N, _ = pts.shape
        idx, dist = dg.ops.farthest_point_sample(p, m=m, start=start, return_dist=True)
        fv, qoff = f.view(B, N, -1), None
    else:
        idx, qoff, dist = dg.ops.farthest_point_sample(p, m=m, offsets=off, start=start, return_dist=True)
        assert isinstance(qoff, E.Segments) and qoff.rows == idx.shape[0]
        fv = f
    sp = dg.ops.take_rows(p, idx, offsets=off)
    sf = dg.ops.take_rows(fv, idx, offsets=off)
    gi, gd = dg.ops.k_nn(sp, k, offsets=qoff, queries=p, query_offsets=off, return_dist=True)
    out = dg.ops.interpolate(sf, None, None, k=k, offsets=qoff, query_offsets=off, graph=(gi, gd))
    # the grouping direction as well: every sample's neighbours in the full set (sample_offsets as query_offsets)
    back = dg.ops.k_nn(p, k, offsets=off, queries=sp, query_offsets=qoff)
    c.grad(E.as2d(out)[0]).copy_(dev(dy))
    c.backward()
    res = [host(t).copy() for t in (idx, dist, sp, sf, gi, gd, out, c.grad(f), back)]
    c.recording = False
    return res


def pipeline_reference(clouds, feats, dy, counts, k, start):
    """the numpy composition of the restatements, cloud by cloud on tower rows"""
    xo, so = offsets([len(c) for c in clouds]), offsets(counts)
    x, feat = np.concatenate(clouds), np.concatenate(feats)
    rows, dist = R.fps_packed(x, xo, counts, start)
    sp, sf = R.take_rows(x, rows), R.take_rows(feat, rows)
    gi, gd, back = [], [], []
    for b in range(len(clouds)):
        i, d = KR.cross_knn(clouds[b], sp[so[b]:so[b + 1]], k)
        gi.append(i + so[b])
        gd.append(d)
        back.append(KR.cross_knn(sp[so[b]:so[b + 1]], clouds[b], k)[0] + xo[b])
    gi, gd, back = np.concatenate(gi).astype(np.int32), np.concatenate(gd), np.concatenate(back).astype(np.int32)
    a, y = IR.interp_f32(sf, gi, gd, 1e-16)
    dsf = IR.interp_bwd_f32(a, gi, dy, len(rows), dfeat0=np.zeros_like(sf))
    return rows, dist, sp, sf, gi, gd, y, R.scatter_rows(dsf, rows, len(x)), back


def test_ops_dense_pipeline_under_a_recording(dg):
    B, N, m, k, F = 2, 257, 65, 3, 8
    rng = np.random.default_rng(20)
    pts = rng.random((B, N, 3), dtype=np.float32)
    feat = rng.standard_normal((B * N, F)).astype(np.float32)
    dy = rng.standard_normal((B * N, F)).astype(np.float32)
    start = [0, 100]
    rows, dist, sp, sf, gi, gd, y, dfeat, back = pipeline_reference(list(pts), list(feat.reshape(B, N, F)), dy, [m] * B, k, start)
    for run in range(2):                                          # two runs, the same bits
        got = pipeline(dg, pts, feat, dy, m, k, start=start)
        assert got[0].shape == (B, m) and np.array_equal(R.tower_rows(got[0], N), rows) and same_bits(got[1].reshape(-1), dist)
        assert got[2].shape == (B, m, 3) and same_bits(got[2].reshape(-1, 3), sp)
        assert got[3].shape == (B, m, F) and same_bits(got[3].reshape(-1, F), sf)
        assert np.array_equal(IR.tower_rows(got[4], m), gi) and same_bits(got[5].reshape(-1, k), gd)
        assert got[6].shape == (B, N, 1, F) and same_bits(got[6].reshape(-1, F), y), "run %d: forward" % run
        assert same_bits(got[7], dfeat), "run %d: feature gradient" % run
        assert np.array_equal(IR.tower_rows(got[8], N), back)
        assert (got[7][np.setdiff1d(np.arange(B * N), rows)] == 0).all() and np.abs(got[7][rows]).min() > 0


def test_ops_packed_pipeline_under_a_recording(dg):
    sizes, counts = TOWER
    k, F = 1, 8
    rng = np.random.default_rng(21)
    xo = offsets(sizes)
    pts = rng.random((int(xo[-1]), 3), dtype=np.float32)
    feat = rng.standard_normal((len(pts), F)).astype(np.float32)
    dy = rng.standard_normal((len(pts), F)).astype(np.float32)
    start = [0, 7, 299, 512]
    cl = [pts[xo[b]:xo[b + 1]] for b in range(4)]
    rows, dist, sp, sf, gi, gd, y, dfeat, back = pipeline_reference(cl, [feat[xo[b]:xo[b + 1]] for b in range(4)], dy, counts, k, start)
    for run in range(2):
        got = pipeline(dg, pts, feat, dy, list(counts), k, off=xo.tolist(), start=start)
        assert got[0].shape == (sum(counts),) and np.array_equal(got[0], rows) and same_bits(got[1], dist)
        assert got[2].shape == (sum(counts), 3) and same_bits(got[2], sp) and same_bits(got[3], sf)
        assert np.array_equal(got[4].reshape(-1, k), gi) and same_bits(got[5].reshape(-1, k), gd)
        assert got[6].shape == (1, len(pts), 1, F) and same_bits(got[6].reshape(-1, F), y), "run %d: forward" % run
        assert same_bits(got[7], dfeat), "run %d: feature gradient" % run
        assert np.array_equal(got[8].reshape(-1, k), back)


def test_ops_ratio_rank4_and_accumulating_gradients(dg):
    """ratio counts as ceil(ratio n); a rank-4 input gives a rank-4 result; a second take from the same features ADDS its gradient
    (beta = 1 behind the first touch)"""
    from dgcnn import _engine as E
    B, N, F = 2, 129, 4
    rng = np.random.default_rng(22)
    pts = rng.random((B, N, 3), dtype=np.float32)
    feat = rng.standard_normal((B * N, F)).astype(np.float32)
    c = dg.ctx()
    c.begin_step()
    c.recording = True
    f = c.new_buffer(B * N, F)
    f.copy_(dev(feat))
    idx = dg.ops.farthest_point_sample(dev(pts), ratio=0.25)
    assert tuple(idx.shape) == (B, 33) and np.array_equal(host(idx), R.fps_dense(pts, 33)[0])
    idx2 = dg.ops.farthest_point_sample(dev(pts), m=10, start=5)
    y1 = dg.ops.take_rows(E.rank4(f, B, N), idx)
    y2 = dg.ops.take_rows(f.view(B, N, F), idx2)
    assert tuple(y1.shape) == (B, 33, 1, F) and tuple(y2.shape) == (B, 10, F)
    d1 = rng.standard_normal((B * 33, F)).astype(np.float32)
    d2 = rng.standard_normal((B * 10, F)).astype(np.float32)
    c.grad(E.as2d(y1)[0]).copy_(dev(d1))
    c.grad(E.as2d(y2)[0]).copy_(dev(d2))
    c.backward()
    r1, r2 = R.tower_rows(host(idx), N), R.tower_rows(host(idx2), N)
    first = R.scatter_rows(d2, r2, B * N)                          # the tape runs in reverse: y2's scatter is the first touch
    assert same_bits(host(c.grad(f)), R.scatter_rows(d1, r1, B * N, first))

"""The head of a packed tower (run with -m gpu on an MI355X): clouds of different sizes concatenated row-wise go through the whole
model -- the segmented kernels of csrc/seg.hip, dgcnn_gemm_seg_f32 on every tile kernel, model.build(offsets=...), trainval and the
run loops with PACK_TOWERS.  References: numpy for the kernels, tests/packed_reference.py (float64, assembled from the oracle's
pieces) for the model."""
import contextlib
import os

import numpy as np
import pytest
import torch

from oracle import dgcnn_oracle as O
import packed_reference as PR
from gpu_helpers import Guard, capture_layers, dev, host, set_vars

pytestmark = pytest.mark.gpu

# no tile (64 / 128 / 192 / 256 rows) or 64-row chunk divides these; clouds below a wave (1, 3, 5) and above a row tile (700, 2000)
SIZES = [5, 3, 1, 700, 64, 2000, 1, 257]
KNN_SIZES = [300, 517, 1000, 256]


@pytest.fixture()
def dg():
    import dgcnn
    from dgcnn import _engine as E
    dgcnn.reset()
    yield dgcnn
    E.DETERMINISTIC = E.DETERMINISTIC_ENV_DEFAULT
    dgcnn.reset()


def offsets_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def row_group_of(sizes):
    return np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)


def padded(g, a, pad):
    """`a` (R, F) as the leading F columns of a guarded (R, F + pad) buffer whose padding holds the sentinel."""
    R, F = a.shape
    buf = g.new((R, F + pad))
    v = buf[:, :F]
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return buf, v


# ------------------------------------------------------------------------------------------
# 1. the segmented kernels through H.call
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,pad", [(70, 5), (1024, 4), (1024, 3)], ids=["F70-scalar", "F1024-float4", "F1024-unaligned"])
def test_colmax_seg_value_and_first_argmax(dg, F, pad):
    """Integer-valued data (exact ties everywhere): per cloud the maximum and its FIRST row, as numpy; an all-NaN column decodes
    to (NaN, 0).  Padded leading dimension; nothing outside the buffers is written."""
    from dgcnn import _hip as H
    rng = np.random.default_rng(F + pad)
    off = offsets_of(SIZES)
    R, nseg = int(off[-1]), len(SIZES)
    x = rng.integers(-3, 4, (R, F)).astype(np.float32)
    x[:, 3] = np.nan
    x[off[3]:off[4], 5] = -np.inf                              # a column of one cloud that is all -inf: (-inf, row 0)
    g = Guard()
    buf, xv = padded(g, x, pad)
    offd = g.put(off.astype(np.int32))
    keys = g.zeros((nseg * F,), torch.int64)
    vals, arg = g.new((nseg, F)), g.new((nseg, F), torch.int32, fill=-7)
    H.call("dgcnn_colmax_seg_f32", xv.data_ptr(), F + pad, R, F, offd.data_ptr(), nseg, keys.data_ptr())
    H.call("dgcnn_colmax_decode_f32", keys.data_ptr(), nseg * F, vals.data_ptr(), arg.data_ptr())
    g.check()
    v, a = host(vals), host(arg)
    for b in range(nseg):
        part = x[off[b]:off[b + 1]]
        cols = np.ones(F, bool)
        cols[3] = False
        np.testing.assert_array_equal(v[b][cols], part.max(0)[cols], err_msg="cloud %d values" % b)
        np.testing.assert_array_equal(a[b][cols], part.argmax(0)[cols], err_msg="cloud %d first arg-max" % b)
        assert np.isnan(v[b, 3]) and a[b, 3] == 0, "all-NaN column of cloud %d: (%r, %d)" % (b, v[b, 3], a[b, 3])


def test_colmax_seg_does_not_depend_on_where_chunks_fall(dg):
    """The same clouds behind a one-row cloud (every chunk boundary moves by one row): the same maxima and arg-maxima."""
    from dgcnn import _hip as H
    F = 72
    body = np.random.default_rng(9).integers(-5, 6, (sum(SIZES), F)).astype(np.float32)
    out = []
    for lead in ([], [1]):
        sizes = lead + SIZES
        off = offsets_of(sizes)
        R, nseg = int(off[-1]), len(sizes)
        xd, offd = dev(np.concatenate([np.zeros((len(lead), F), np.float32), body])), dev(off.astype(np.int32))
        keys = torch.zeros(nseg * F, dtype=torch.int64, device="cuda")
        vals = torch.empty((nseg, F), device="cuda")
        arg = torch.empty((nseg, F), dtype=torch.int32, device="cuda")
        H.call("dgcnn_colmax_seg_f32", xd.data_ptr(), F, R, F, offd.data_ptr(), nseg, keys.data_ptr())
        H.call("dgcnn_colmax_decode_f32", keys.data_ptr(), nseg * F, vals.data_ptr(), arg.data_ptr())
        out.append((host(vals)[len(lead):], host(arg)[len(lead):]))
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])


@pytest.mark.parametrize("F,pad", [(70, 5), (1024, 4)])
def test_global_max_bwd_seg_scatters_inside_each_cloud(dg, F, pad):
    from dgcnn import _hip as H
    rng = np.random.default_rng(F)
    off = offsets_of(SIZES)
    R, nseg = int(off[-1]), len(SIZES)
    dout = rng.normal(size=(nseg, F)).astype(np.float32)
    arg = np.stack([rng.integers(0, n, F) for n in SIZES]).astype(np.int32)
    dx0 = rng.normal(size=(R, F)).astype(np.float32)
    g = Guard()
    buf, dxv = padded(g, dx0, pad)
    H.call("dgcnn_global_max_bwd_seg_f32", g.put(dout).data_ptr(), g.put(arg).data_ptr(), g.put(off.astype(np.int32)).data_ptr(),
           nseg, F, dxv.data_ptr(), F + pad)
    g.check()
    ref = dx0.copy()
    for b in range(nseg):
        ref[off[b] + arg[b], np.arange(F)] += dout[b]          # one writer per (cloud, column): a single fp32 add
    np.testing.assert_array_equal(host(buf)[:, :F], ref)
    assert (host(buf)[:, F:] == 777.0).all()


@pytest.mark.parametrize("F,pad", [(70, 5), (1024, 4)])
def test_tile_rows_seg(dg, F, pad):
    from dgcnn import _hip as H
    rng = np.random.default_rng(F + 1)
    R, nseg = sum(SIZES), len(SIZES)
    src = rng.normal(size=(nseg, F)).astype(np.float32)
    rg = row_group_of(SIZES)
    g = Guard()
    sbuf, sv = padded(g, src, 3)
    dbuf = g.new((R, F + pad))
    H.call("dgcnn_tile_rows_seg_f32", sv.data_ptr(), F + 3, g.put(rg).data_ptr(), R, F, dbuf[:, :F].data_ptr(), F + pad)
    g.check()
    np.testing.assert_array_equal(host(dbuf)[:, :F], src[rg])
    assert (host(dbuf)[:, F:] == 777.0).all()


@pytest.mark.parametrize("F,pad", [(70, 5), (1024, 4), (1024, 3)], ids=["F70-scalar", "F1024-float4", "F1024-unaligned"])
def test_seg_colsum_is_reproducible_and_within_the_fp32_summation_bound(dg, F, pad):
    """Two runs bit-identical (fixed summation order); against the float64 sum within n_b 2^-24 sum|x| per output -- the worst case
    of an fp32 sum of n_b terms in any order."""
    from dgcnn import _hip as H
    lib = H.load()
    rng = np.random.default_rng(F * 3 + pad)
    off = offsets_of(SIZES)
    R, nseg = int(off[-1]), len(SIZES)
    x = rng.normal(size=(R, F)).astype(np.float32)
    g = Guard()
    buf, xv = padded(g, x, pad)
    offd = g.put(off.astype(np.int32))
    nws = int(lib.dgcnn_seg_colsum_workspace_bytes(R, nseg, F))
    assert nws == 4 * F * (-(-R // 64) + nseg)
    runs = []
    for _ in range(2):
        ws = g.new((nws // 4,))
        out = g.new((nseg, F))
        H.call("dgcnn_seg_colsum_f32", xv.data_ptr(), F + pad, R, F, offd.data_ptr(), nseg, out.data_ptr(), ws.data_ptr(), nws)
        runs.append(host(out).copy())
    g.check()
    np.testing.assert_array_equal(runs[0], runs[1])
    for b, n in enumerate(SIZES):
        part = x[off[b]:off[b + 1]].astype(np.float64)
        err = np.abs(runs[0][b].astype(np.float64) - part.sum(0))
        bound = n * 2.0 ** -24 * np.abs(part).sum(0)
        assert (err <= bound).all(), "cloud %d (%d rows): error %.3g over the bound %.3g" % (b, n, (err - bound).max(), bound[(err - bound).argmax()])
    with pytest.raises(H.HipError, match="workspace too small"):
        H.call("dgcnn_seg_colsum_f32", xv.data_ptr(), F + pad, R, F, offd.data_ptr(), nseg, g.new((nseg, F)).data_ptr(),
               g.new((16,)).data_ptr(), 64)


def test_engine_global_max_and_tile_rows_on_a_packed_tower(dg):
    """E.global_max(seg=) and E.tile_rows(seg=) with their backward passes (max-pool gradient to the first arg-max of each cloud,
    tf.tile^T as the per-cloud sum), on a column slice of a wider buffer."""
    from dgcnn import _engine as E
    rng = np.random.default_rng(12)
    F = 96
    off = offsets_of(SIZES)
    R, nseg = int(off[-1]), len(SIZES)
    seg = E.Segments(off, R)
    xh = rng.integers(-4, 5, (R, F)).astype(np.float32)
    c = dg.ctx()
    c.begin_step()
    c.recording = True
    wide = c.new_buffer(R, F + 8)
    x = wide[:, 4:4 + F]
    x.copy_(dev(xh))
    g = E.global_max(x, 0, 0, seg=seg)
    tiled = c.new_buffer(R, F)
    E.tile_rows(g, tiled, 0, seg=seg)
    ref = np.stack([xh[off[b]:off[b + 1]].max(0) for b in range(nseg)])
    np.testing.assert_array_equal(host(g), ref)
    np.testing.assert_array_equal(host(tiled), ref[row_group_of(SIZES)])
    dt = rng.integers(-3, 4, (R, F)).astype(np.float32)            # integers: every order of summation gives the same sum
    c.grad(tiled).copy_(dev(dt))
    c.backward()
    dx = host(c.grad(x))
    c.recording = False
    want = np.zeros((R, F), np.float32)
    for b in range(nseg):
        want[off[b] + xh[off[b]:off[b + 1]].argmax(0), np.arange(F)] = dt[off[b]:off[b + 1]].sum(0)
    np.testing.assert_array_equal(dx, want)


# ------------------------------------------------------------------------------------------
# 2. dgcnn_gemm_seg_f32 on every tile kernel
# ------------------------------------------------------------------------------------------
@contextlib.contextmanager
def tile(override, arith):
    from dgcnn import _hip as H
    lib = H.load()
    prev_arith = H.gemm_arith()
    prev = lib.dgcnn_gemm_x3_tile_override(override)
    try:
        H.set_gemm_arith(arith)
        yield
    finally:
        lib.dgcnn_gemm_x3_tile_override(prev)
        H.set_gemm_arith(prev_arith)


# (arithmetic, tile override, expected (tile rows, 256-column kernel) or None, cloud sizes, N, K): the forcing of
# tests/test_gpu_gemm_tiles.py -- 128 = gemm_x3_kernel<128>, 256 = gemm_x3w2_kernel (256 x 128), 512 / 448 = gemm_x3q_kernel 256 x 256 /
# 192 x 256, arithmetic 0 = the fp32-MFMA gemm_kernel; the 64-row gemm_x3_kernel is what the cost rule picks for a short reduction over
# many rows.  K < 512: the product without bias is not split over K.
BIG = SIZES + [1072]                                              # 4103 rows
LONG = SIZES + [16972]                                            # 20003 rows
GEMM_CASES = [(6, 128, (128, 0), BIG, 520, 204), (6, 256, (256, 0), BIG, 520, 204), (6, 512, (256, 256), BIG, 520, 204),
              (6, 448, (192, 256), BIG, 520, 204), (6, 0, (64, 0), LONG, 64, 128), (0, 0, None, BIG, 520, 204)]


def assert_colsums(st, C64, slots, what):
    """The bar tests/test_gpu_gemm_tiles.py applies to the dense statistics: 1e-5 of the column's magnitude."""
    N = C64.shape[1]
    s = host(st).reshape(slots, 2, N).sum(0)
    for j, ref, mag in ((0, C64.sum(0), np.abs(C64).sum(0)), (1, (C64 ** 2).sum(0), (C64 ** 2).sum(0))):
        err = np.abs(s[j] - ref) / np.maximum(mag, 1e-30)
        assert err.max() < 1e-5, "%s: column %s %.2e of the magnitude (column %d)" % (what, ("sums", "sums of squares")[j], err.max(), int(err.argmax()))


@pytest.mark.parametrize("arith,override,forced,sizes,N,K", GEMM_CASES,
                         ids=["x3-128", "x3w2-256x128", "x3q-256x256", "x3q-192x256", "x3-64", "fp32-mfma"])
def test_gemm_seg_bias_on_every_tile(dg, arith, override, forced, sizes, N, K):
    """C = A B + gbias[row_group]: bit-identical to the product without bias plus that one fp32 add (done on the host), in the NN and
    NT layouts, with float4-loadable and scalar bias rows; the statistics include the bias."""
    from dgcnn import _engine as E
    lib = E.H.load()
    rng = np.random.default_rng(sum(sizes) + override)
    M, nseg = sum(sizes), len(sizes)
    A = rng.normal(size=(M, K)).astype(np.float32)
    Bm = rng.normal(size=(K, N)).astype(np.float32)
    gb = rng.normal(size=(nseg, N)).astype(np.float32)
    rg = row_group_of(sizes)
    rgd = dev(rg)
    with tile(override, arith):
        if forced is not None:
            assert (lib.dgcnn_gemm_x3_tile_rows(M, N, K), lib.dgcnn_gemm_x3_tile_cols(M, N, K)) == forced
        for layout, Bd, tr in (("NN", dev(Bm), {}), ("NT", dev(Bm.T.copy()), {"transB": True})):
            C0 = torch.full((M, N), float("nan"), device="cuda")
            E.gemm(dev(A), Bd, C0, **tr)
            want = host(C0) + gb[rg]                               # float32 + float32: the epilogue's one add
            for gpad in (4, 1):                                    # ldgbias % 4 == 0 (float4 bias rows) / not
                what = "%s arith %d override %d gbias ld %d" % (layout, arith, override, N + gpad)
                gbuf = torch.zeros((nseg, N + gpad), device="cuda")
                gbuf[:, :N] = dev(gb)
                outw = torch.zeros((M, N + 8), device="cuda")
                C1 = outw[:, 4:4 + N]
                st = torch.zeros(E.H.stat_slots() * 2 * N, dtype=torch.float64, device="cuda")
                E.gemm(dev(A), Bd, C1, gbias=gbuf[:, :N], stats=st, row_group=rgd, **tr)
                got = host(C1)
                bad = np.argwhere(got != want)
                assert len(bad) == 0, "%s: %d elements differ from product + bias, first %s: %r vs %r" % (
                    what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
                assert not bool(outw[:, :4].any()) and not bool(outw[:, 4 + N:].any()), (what, "wrote outside its columns")
                assert_colsums(st, got.astype(np.float64), E.H.stat_slots(), what)


@pytest.mark.parametrize("arith,override", [(6, 128), (6, 256), (6, 512), (6, 448), (0, 0)])
def test_gemm_seg_equals_the_dense_bias_on_equal_clouds(dg, arith, override):
    """Six clouds of 1000 rows (no multiple of a tile height): row_group and rows_per_group = 1000 address the same bias rows -- the
    same kernel, the same output bits."""
    from dgcnn import _engine as E
    rng = np.random.default_rng(override)
    G, n, N, K = 6, 1000, 520, 204
    A, Bm = dev(rng.normal(size=(G * n, K)).astype(np.float32)), dev(rng.normal(size=(K, N)).astype(np.float32))
    gb = dev(rng.normal(size=(G, N)).astype(np.float32))
    rgd = dev(row_group_of([n] * G))
    with tile(override, arith):
        Cd, Cs = torch.empty((G * n, N), device="cuda"), torch.empty((G * n, N), device="cuda")
        E.gemm(A, Bm, Cd, gbias=gb, rpg=n)
        E.gemm(A, Bm, Cs, gbias=gb, row_group=rgd)
    assert torch.equal(Cd, Cs), int((Cd != Cs).sum())


def test_gemm_seg_refusals(dg):
    from dgcnn import _engine as E, _hip as H
    A, Bm, C = torch.zeros((64, 8), device="cuda"), torch.zeros((8, 8), device="cuda"), torch.zeros((64, 8), device="cuda")
    gb = torch.zeros((2, 8), device="cuda")
    rg = torch.zeros(64, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        E.gemm(A, Bm, C, gbias=gb, row_group=rg[:60])              # not one entry per row
    with pytest.raises(ValueError):
        E.gemm(A, Bm, C, gbias=gb, row_group=rg, colmax=torch.zeros(16, dtype=torch.int64, device="cuda"), colmax_rpg=256)
    ws = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    with pytest.raises(H.HipError, match="transA"):                # no bias with transA, as in the dense call
        H.call("dgcnn_gemm_seg_f32", 1, 0, 8, 8, 64, A.data_ptr(), 8, C.data_ptr(), 8, Bm.data_ptr(), 8, 0.0, gb.data_ptr(), 8,
               rg.data_ptr(), 0, ws.data_ptr(), ws.numel())


# ------------------------------------------------------------------------------------------
# 3. model.build(offsets=...) against the packed float64 reference
# ------------------------------------------------------------------------------------------
MODELS = [("dgcnn", 2), ("dgcnn", 0), ("residual-dgcnn", 2), ("residual-dgcnn", 0), ("residual-dgcnn-nofc", 2)]


def model_flags(dg, model, fcl, det, **kw):
    base = dict(MODEL_NAME=model, EDGE_CONV_LAYERS=2, EDGE_CONV_FILTERS=[32, 64], KVALUE=20, NUM_CLASS=3, FC_LAYERS=fcl,
                FC_FILTERS=[64, 32][:fcl] if fcl else 64, TRAIN=False, NUM_CHANNEL=4, DETERMINISTIC=None if det else False)
    base.update(kw)
    return dg.DGCNN_FLAGS(**base)


def make_tower(rng, sizes, C, ncls):
    clouds = [rng.random((n, C), dtype=np.float32) for n in sizes]
    pts = np.concatenate(clouds)
    return pts, offsets_of(sizes), rng.integers(0, ncls, len(pts)).astype(np.int32), (rng.random(len(pts), dtype=np.float32) + 0.5)


def random_params(flags, rng, C):
    params = O.init_params(flags, C, seed=1)
    for n in params:
        if n.endswith("beta"):
            params[n] = rng.normal(0, 0.2, params[n].shape).astype(np.float32)
    return params


def graphs_of(cap, L, off, k):
    """The captured packed graphs, each checked against the oracle's k-NN of the layer's own input, cloud by cloud, bit for bit."""
    out = []
    for i in range(L):
        xin, idx = cap.layers["EdgeConv%d" % i]
        assert idx.shape == (1, off[-1], k)
        flat = idx.reshape(-1, k)
        for b in range(len(off) - 1):
            part = flat[off[b]:off[b + 1]]
            assert part.min() >= off[b] and part.max() < off[b + 1], "layer %d cloud %d: an index outside the cloud" % (i, b)
            np.testing.assert_array_equal(part - off[b], O.k_nn(xin[0, off[b]:off[b + 1]][None], k)[0], err_msg="layer %d cloud %d" % (i, b))
        out.append(idx)
    return out


@pytest.mark.parametrize("det", [True, False], ids=["default", "atomics"])
@pytest.mark.parametrize("model,fcl", MODELS, ids=["%s-fc%d" % m for m in MODELS])
def test_packed_model_logits_and_gradients(dg, model, fcl, det):
    """Four unequal clouds, C = 4, k = 20: per-cloud graphs bit for bit, logits within 1e-3 absolute of the packed float64 reference
    fed those graphs, every gradient within 5e-3 (deterministic) / 2e-2 (atomics) relative Frobenius.  Dropout off."""
    import dgcnn
    from dgcnn import _engine as E
    rng = np.random.default_rng(17)
    flags = model_flags(dg, model, fcl, det)
    pts, off, lab, wgt = make_tower(rng, KNN_SIZES, 4, 3)
    R = len(pts)
    params = random_params(flags, rng, 4)
    p64 = {n: v.astype(np.float64) for n, v in params.items()}
    tv = dg.trainval(flags).initialize()
    set_vars(dg, params)
    assert E.DETERMINISTIC == det
    with capture_layers() as cap:
        logits = host(dgcnn.build(dev(pts), flags, offsets=off))
    assert logits.shape == (1, R, 3)
    graphs = graphs_of(cap, 2, off, 20)
    ref, _ = PR.model_forward(pts.astype(np.float64), off, flags, p64, graphs)
    err = np.abs(logits - ref)
    print("%s fc%d %s: logits max |err| %.3g" % (model, fcl, "det" if det else "atomics", err.max()))
    assert err.max() <= 1e-3, "logits differ from the packed reference: max %g at %s" % (err.max(), np.unravel_index(err.argmax(), err.shape))
    if det:                                                       # (1, R, C) in, offsets as a Segments: the same tower, bit for bit
        np.testing.assert_array_equal(host(dgcnn.build(dev(pts[None]), flags, offsets=E.Segments(off, R))), logits)

    flags.TRAIN = True
    keep = E.DROPOUT_KEEP
    E.DROPOUT_KEEP = 1.0
    try:
        tv = dg.trainval(flags).initialize()
        set_vars(dg, params)
        tv.zero_gradients(None)
        with capture_layers() as cap:
            res = tv.accum_gradient(None, [pts], [lab], [wgt], offsets=[off])
    finally:
        E.DROPOUT_KEEP = keep
    graphs = graphs_of(cap, 2, off, 20)
    G, loss64, acc64, _ = PR.train_step_grads(pts.astype(np.float64), lab, off, flags, p64, graphs, weight=wgt.astype(np.float64))
    assert abs(float(res[2]) - float(loss64)) < 1e-3
    bar = 5e-3 if det else 2e-2
    worst = (0.0, "")
    for n in params:
        got = host(tv.gradients[n]).astype(np.float64)
        worst = max(worst, (float(np.linalg.norm(got - G[n]) / max(np.linalg.norm(G[n]), 1e-6)), n))
    print("%s fc%d %s: worst relative Frobenius gradient error %.3g (%s)" % (model, fcl, "det" if det else "atomics", worst[0], worst[1]))
    assert worst[0] <= bar, worst


# ------------------------------------------------------------------------------------------
# 4. packed against dense
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("N", [512, 700])
def test_equal_clouds_pack_equals_the_dense_model(dg, N, B):
    """offsets = [0, N(, 2N)] against the dense (B, N) tower: the same graphs (after subtracting the offsets), logits within 1e-6.
    N = 512: the dense path takes the GEMM-epilogue column maximum; N = 700: its separate pass."""
    import dgcnn
    rng = np.random.default_rng(N + B)
    flags = model_flags(dg, "dgcnn", 2, True, KVALUE=20, NUM_CHANNEL=3)
    pts = rng.random((B, N, 3), dtype=np.float32)
    params = random_params(flags, rng, 3)
    dg.trainval(flags).initialize()
    set_vars(dg, params)
    with capture_layers(keep_inputs=False) as cap_d:
        dense = host(dgcnn.build(dev(pts), flags))
    dg.trainval(flags).initialize()
    set_vars(dg, params)
    off = np.arange(B + 1) * N
    with capture_layers(keep_inputs=False) as cap_p:
        packed = host(dgcnn.build(dev(pts.reshape(B * N, 3)), flags, offsets=off))
    assert packed.shape == (1, B * N, 3) and dense.shape == (B, N, 3)
    for i in range(2):
        gd, gp = cap_d.layers["EdgeConv%d" % i][1], cap_p.layers["EdgeConv%d" % i][1]
        np.testing.assert_array_equal(gp.reshape(B, N, -1) - (np.arange(B) * N)[:, None, None], gd, err_msg="layer %d" % i)
    np.testing.assert_allclose(packed.reshape(B, N, 3), dense, rtol=1e-6, atol=1e-6)


# ------------------------------------------------------------------------------------------
# 5. trainval
# ------------------------------------------------------------------------------------------
def test_packed_training_steps_are_bit_reproducible(dg):
    """Default (deterministic) mode: two zero_gradients -> accum_gradient(offsets) -> apply_gradient steps from a fresh initialize,
    done twice, leave bit-identical parameters (dropout on: the mask stream restarts with the instance)."""
    rng = np.random.default_rng(3)
    flags = model_flags(dg, "dgcnn", 2, True, TRAIN=True)
    pts, off, lab, wgt = make_tower(rng, KNN_SIZES, 4, 3)
    finals = []
    for _ in range(2):
        tv = dg.trainval(flags).initialize()
        for _ in range(2):
            tv.zero_gradients(None)
            res = tv.accum_gradient(None, [pts[None]], [lab[None]], [wgt[None]], offsets=[off])
            tv.apply_gradient(None)
        assert np.isfinite(float(res[2]))
        finals.append(tv._ctx.flat_param.clone())
    assert torch.equal(finals[0], finals[1]), int((finals[0] != finals[1]).sum())


def test_packed_tower_runs_eagerly_under_a_launch_plan(dg):
    """use_graph("plan"): a packed tower still runs (eagerly -- the offsets change every step), nothing is recorded for it, and it
    gives the eager step: bit-identical gradients (deterministic mode) and the same loss.  The reported loss alone is summed with
    fp32 atomics over the softmax kernel's workgroups (_engine.py: "summed with atomics in both" modes), so two runs of it agree to
    the order-of-summation bound of cdiv(R, 256) positive partial sums: cdiv(R, 256) 2^-24 loss."""
    from dgcnn import _engine as E
    rng = np.random.default_rng(4)
    flags = model_flags(dg, "dgcnn", 2, True, TRAIN=True)
    pts, off, lab, _ = make_tower(rng, KNN_SIZES, 4, 3)
    keep = E.DROPOUT_KEEP
    E.DROPOUT_KEEP = 1.0
    try:
        losses, grads = [], []
        for mode in (False, "plan"):
            tv = dg.trainval(flags).initialize().use_graph(mode)
            assert tv._wants_graph(len(pts), packed=True) is None
            for _ in range(3):                                     # (a dense shape would be recorded at its second sighting)
                tv.zero_gradients(None)
                res = tv.accum_gradient(None, [pts], [lab], offsets=[off])
            losses.append(float(res[2]))
            grads.append(tv._ctx.flat_grad.clone())
            assert tv.launch_plan_info() == []
    finally:
        E.DROPOUT_KEEP = keep
    assert torch.equal(grads[0], grads[1]), int((grads[0] != grads[1]).sum())
    print("eager loss %.9g, under use_graph('plan') %.9g" % tuple(losses))
    assert abs(losses[0] - losses[1]) <= -(-len(pts) // 256) * 2.0 ** -24 * losses[0], losses


def test_packed_loss_and_accuracy_are_row_means(dg):
    """loss / accuracy / softmax of a packed tower against the packed float64 reference fed the captured graphs (dropout off): the
    mean over the R rows.  Loss within 1e-5; the accuracy may differ by the rows whose two largest reference logits lie within
    2e-3 of each other (the logits agree within 1e-3, so only those can flip their arg-max)."""
    from dgcnn import _engine as E
    rng = np.random.default_rng(6)
    flags = model_flags(dg, "dgcnn", 2, True, TRAIN=True)
    pts, off, lab, wgt = make_tower(rng, KNN_SIZES, 4, 3)
    R = len(pts)
    params = random_params(flags, rng, 4)
    keep = E.DROPOUT_KEEP
    E.DROPOUT_KEEP = 1.0
    try:
        tv = dg.trainval(flags).initialize()
        set_vars(dg, params)
        with capture_layers() as cap:
            res = tv.inference(None, [pts], [lab], [wgt], offsets=[off])
    finally:
        E.DROPOUT_KEEP = keep
    sm, acc, loss = host(res[0]), float(res[1]), float(res[2])
    assert sm.shape == (1, R, 3)
    graphs = [cap.layers["EdgeConv%d" % i][1] for i in range(2)]
    p64 = {n: v.astype(np.float64) for n, v in params.items()}
    logits64, _ = PR.model_forward(pts.astype(np.float64), off, flags, p64, graphs)
    loss64, sm64, acc64, _ = O.softmax_xent(logits64, lab.reshape(1, R), wgt.astype(np.float64).reshape(1, R))
    print("packed loss %.9g reference %.9g (diff %.3g); accuracy %.6f reference %.6f" % (loss, loss64, loss - loss64, acc, acc64))
    top = np.sort(logits64[0], axis=-1)
    close = int((top[:, -1] - top[:, -2] < 2e-3).sum())
    assert abs(acc - float(acc64)) <= (close + 0.5) / R, (acc, float(acc64), close)
    np.testing.assert_allclose(sm, sm64, rtol=0, atol=1e-3)
    assert abs(loss - float(loss64)) <= 1e-5, (loss, float(loss64))


# ------------------------------------------------------------------------------------------
# 6. run loops with PACK_TOWERS
# ------------------------------------------------------------------------------------------
def test_run_loops_pack_a_ragged_source(dg, tmp_path, capsys):
    """A ragged .npz, MINIBATCH_SIZE = 2, PACK_TOWERS: two training iterations (finite loss, checkpoint), one inference iteration
    whose stored softmax has one array per entry with that entry's row count."""
    from dgcnn import main_funcs as M
    rng = np.random.default_rng(4)
    counts = [300, 517, 256, 777]
    off = offsets_of(counts)
    pts = rng.random((off[-1], 4), dtype=np.float32)
    np.savez(tmp_path / "ragged.npz", data=pts, label=(pts[:, 0] > 0.5).astype(np.int32), data_offsets=off)
    common = dict(IO_TYPE="npz", INPUT_FILE=str(tmp_path / "ragged.npz"), NUM_POINT=-1, NUM_CHANNEL=-1, BATCH_SIZE=4, MINIBATCH_SIZE=2,
                  PACK_TOWERS=True, SHUFFLE=0, KVALUE=8, EDGE_CONV_LAYERS=2, EDGE_CONV_FILTERS=[32, 64], FC_LAYERS=1, FC_FILTERS=[64],
                  NUM_CLASS=2, REPORT_STEP=0, SUMMARY_STEP=0, SEED=5, WEIGHT_PREFIX=str(tmp_path / "w" / "snap"))
    f = dg.DGCNN_FLAGS(ITERATION=2, CHECKPOINT_STEP=2, LOG_DIR=str(tmp_path / "log"), **common)
    M.train(f)
    rows = open(tmp_path / "log" / "train_log-0000000.csv").read().strip().split("\n")[1:]
    assert len(rows) == 2 and all(np.isfinite(float(r.split(",")[-2])) for r in rows)
    assert os.path.exists(f.WEIGHT_PREFIX + "-1.npz")
    g = dg.DGCNN_FLAGS(ITERATION=1, MODEL_PATH=f.WEIGHT_PREFIX + "-1", OUTPUT_FILE=str(tmp_path / "out.npz"),
                       LOG_DIR=str(tmp_path / "ilog"), **common)
    seen = []
    g.TRAIN = False
    h = M.prepare(g)
    store = h.data_io.store
    h.data_io.store = lambda idx, row: (seen.append((int(idx), tuple(row.shape))), store(idx, row))[1]
    M.inference_loop(g, h)
    capsys.readouterr()
    assert seen == [(i, (n, 2)) for i, n in enumerate(counts)]     # one softmax array per entry, that entry's rows, batch order
    z = np.load(tmp_path / "out.npz")
    assert z["idx"].tolist() == [0, 1, 2, 3] and np.diff(z["data_offsets"]).tolist() == counts
    assert z["softmax"].shape == (sum(counts), 2) and np.allclose(z["softmax"].sum(1), 1.0, atol=1e-5)


# ------------------------------------------------------------------------------------------
# 7. errors, before any launch
# ------------------------------------------------------------------------------------------
def test_packed_model_errors_before_any_launch(dg, monkeypatch):
    import dgcnn
    from dgcnn import _hip as H
    flags = model_flags(dg, "dgcnn", 2, True, TRAIN=True)
    tv = dg.trainval(flags).initialize()
    launches = []
    orig = H.call
    monkeypatch.setattr(H, "call", lambda name, *a, **kw: (launches.append(name), orig(name, *a, **kw))[1])
    x = dev(np.zeros((50, 4), np.float32))
    with pytest.raises(ValueError, match="smallest cloud=19"):
        dgcnn.build(x, flags, offsets=[0, 19, 50])                 # k = 20 above the smallest cloud
    with pytest.raises(ValueError, match="offsets end at 49"):
        dgcnn.build(x, flags, offsets=[0, 24, 49])                 # offsets do not end at R
    lab = np.zeros(50, np.int32)
    with pytest.raises(ValueError):
        tv.accum_gradient(None, [np.zeros((2, 25, 4), np.float32)], [lab], offsets=[[0, 25, 50]])    # 3-D data with B > 1
    with pytest.raises(ValueError, match="smallest cloud=19"):
        tv.inference(None, [np.zeros((50, 4), np.float32)], offsets=[[0, 19, 50]])
    with pytest.raises(ValueError):
        tv.accum_gradient(None, [np.zeros((50, 4), np.float32)], [lab[:40]], offsets=[[0, 25, 50]])  # label of another length
    with pytest.raises(ValueError):
        tv.feed_dict([np.zeros((50, 4), np.float32)], offsets=[None, None])
    assert launches == []

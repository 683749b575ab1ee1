"""EDGE_MLP_DTYPE='bf16' -- BASELINE.json configs[2] in its named mode ("bf16 edge-MLP MFMA"): conv0 of every EdgeConv layer as the
literal (B*N*k) x 2C x F product with bf16 OPERANDS (E = [x_i, x_j - x_i] formed in fp32 first, E and W0 rounded once, RNE) and
fp32 accumulation on v_mfma_f32_32x32x16_bf16; the two gradient products round their operands the same way.

The checker is the oracle IN THE SAME MODE (oracle.edge_conv(edge_mlp_dtype='bf16'): operands through oracle.bf16_round,
products and sums in float64): with operands that are exactly representable the only difference left is the accumulation
order, so the bars are the fp32 ones (1e-3 on the logits).  The distance to the UNROUNDED fp64 twin -- what the rounding itself
costs -- is printed, not asserted (it is a property of the mode, 2^-9 per operand, not of the implementation)."""
import numpy as np
import pytest
import torch

from oracle import dgcnn_oracle as O
from gpu_helpers import (BF16_BLOCK_GRAD_TOL, BF16_BLOCK_OUT_TOL, BF16_MODEL_GRAD_TOL, BF16_MODEL_LOSS_TOL, LAYER_ATOL, capture_layers, dev,
                         host, run_model, set_vars)

pytestmark = pytest.mark.gpu


@pytest.fixture()
def dg():
    import dgcnn
    from dgcnn import _engine as E
    dgcnn.reset()
    yield dgcnn
    E.EDGE_MLP_DTYPE = "f32"
    E.DETERMINISTIC = E.DETERMINISTIC_ENV_DEFAULT
    dgcnn.reset()


@pytest.mark.parametrize("B,N,C,k,F", [(2, 64, 3, 5, 8), (2, 128, 64, 20, 64), (1, 96, 4, 7, 128), (2, 64, 64, 10, 32),
                                       (1, 96, 4, 10, 128), (2, 64, 3, 8, 64), (1, 50, 64, 40, 128), (1, 70, 64, 10, 128), (1, 60, 64, 8, 128),
                                       # conv0 widths whose products E W0 and E^T dY leave dgcnn_gemm_f32's rounding path (F = 4: the
                                       # streaming kernels; F % 4 != 0: the scalar fp32 kernel, legal without DETERMINISTIC) -- the
                                       # engine rounds E and W0 itself there -- and F = 12, the smallest width that stays on it
                                       (2, 64, 3, 5, 4), (2, 64, 64, 10, 4), (2, 64, 3, 5, 6), (1, 96, 4, 7, 10), (2, 64, 3, 5, 12)])
def test_edge_conv_bf16_forward_backward(dg, B, N, C, k, F):
    """One edge_conv block in bf16 mode against the oracle in bf16 mode (same graph): [max, mean, net] within 1e-4 and the
    gradients w.r.t. X (C % 4 == 0), W0, beta0, W1, beta1 within 2e-3 -- the bars of the fp32 block test
    (test_gpu_parity.py::test_edge_conv_forward_backward).  F % 4 != 0 runs with DETERMINISTIC off (the fixed-order column sums
    take float4 columns) and without d(X): the mode refuses the input gradient at such widths."""
    from dgcnn import _engine as E
    E.EDGE_MLP_DTYPE = "bf16"
    if F % 4:
        E.DETERMINISTIC = False
    rng = np.random.default_rng(C * 10 + F)
    pts = rng.random((B, N, C), dtype=np.float32)
    P = {"conv0/weights": rng.normal(0, 0.5, (2 * C, F)).astype(np.float32),
         "conv0/BatchNorm/beta": rng.normal(0, 0.3, F).astype(np.float32),
         "conv1/weights": rng.normal(0, 0.3, (2 * F, 64)).astype(np.float32),
         "conv1/BatchNorm/beta": rng.normal(0, 0.3, 64).astype(np.float32)}
    c = dg.ctx()
    c.begin_step()
    c.recording = True
    want_dx = C % 4 == 0 and F % 4 == 0
    if want_dx:
        x = c.new_buffer(B * N, C)
    else:
        x = torch.empty((B * N, C), dtype=torch.float32, device="cuda")     # raw coordinates: nobody wants d(points)
    x.copy_(dev(pts.reshape(B * N, C)))
    for n, v in P.items():
        c.get_variable(n, v.shape)
    set_vars(dg, P)
    outs = dg.ops.edge_conv(x.view(B, N, C), k, F, True)
    idx = host(dg.ops.edge_conv.last_idx)
    np.testing.assert_array_equal(idx, O.k_nn(pts, k))

    P64 = [P[n].astype(np.float64) for n in P]
    ref, cache = O.edge_conv(pts.astype(np.float64), k, *P64, idx=idx, edge_mlp_dtype="bf16")
    plain, _ = O.edge_conv(pts.astype(np.float64), k, *P64, idx=idx)
    for name, a, b, p in zip(("max", "mean", "net"), outs, ref, plain):
        print("%s: max |HIP bf16 - oracle bf16| %.2e;  |oracle bf16 - oracle f32-operands| %.2e (what the mode costs)"
              % (name, np.abs(host(a) - b).max(), np.abs(b - p).max()))
        np.testing.assert_allclose(host(a), b, rtol=BF16_BLOCK_OUT_TOL, atol=BF16_BLOCK_OUT_TOL, err_msg=name)
    assert np.abs(ref[0] - plain[0]).max() > 1e-4              # the mode IS different arithmetic: the test would notice fp32 operands

    d = [rng.normal(size=r.shape) for r in ref]
    for t, g in zip(outs, d):
        v, _, _ = E.as2d(t)
        c.grad(v).copy_(dev(g.reshape(B * N, -1).astype(np.float32)))
    c.backward()
    dx_ref, g_ref = O.edge_conv_bwd(d[0], d[1], d[2], cache)
    scale = lambda r: BF16_BLOCK_GRAD_TOL * max(1.0, float(np.abs(r).max()))
    if want_dx:
        np.testing.assert_allclose(host(c.grad(x)).reshape(B, N, C), dx_ref, rtol=BF16_BLOCK_GRAD_TOL, atol=scale(dx_ref), err_msg="dx")
    for n, key in (("conv0/weights", "W0"), ("conv0/BatchNorm/beta", "beta0"), ("conv1/weights", "W1"),
                   ("conv1/BatchNorm/beta", "beta1")):
        np.testing.assert_allclose(host(c.var_grads[n]), g_ref[key], rtol=BF16_BLOCK_GRAD_TOL, atol=scale(g_ref[key]), err_msg=n)


def config2_flags(dg, train, emd="bf16"):
    return dg.DGCNN_FLAGS(MODEL_NAME="residual-dgcnn", EDGE_CONV_LAYERS=6, EDGE_CONV_FILTERS=64, FC_LAYERS=2,
                          FC_FILTERS=[512, 256], NUM_CLASS=2, KVALUE=40, NUM_CHANNEL=3, TRAIN=train, EDGE_MLP_DTYPE=emd)


def test_config2_architecture_logits_n2048_bf16(dg):
    """configs[2] architecture (residual-dgcnn, 6 x 64, k = 40) at B=2, N=2048 in its named mode.
      * every layer's graph bit-exact against the C oracle on the layer's actual input;
      * LAYER BY LAYER (the oracle in bf16 mode is fed the fp32 input the HIP layer really saw): the layer's output within 1e-4 --
        the implementation is the mode's arithmetic and nothing else;
      * END TO END against the float64 oracle in the same mode on the same graphs the bar cannot be the fp32 one: a feature
        that differs in its last fp32 bit between two evaluations can land on the other side of a bf16 rounding boundary of
        the NEXT layer's operand (a 2^-9 jump), so any two evaluations of this mode drift apart through six layers.  Measured:
        max 2.2e-2 / mean 1.1e-3, one tenth of what the mode itself costs against fp32 operands (max 0.21 / mean 1.7e-2).
        Asserted: max <= 6e-2, mean <= 3e-3 and at least 5x closer to the bf16-mode oracle than that oracle is to the fp32 one."""
    B, N, C, L = 2, 2048, 3, 6
    flags = config2_flags(dg, train=False)
    rng = np.random.default_rng(2)
    pts = rng.random((B, N, C), dtype=np.float32)
    params = O.init_params(flags, C, seed=3)
    for n in params:
        if n.endswith("beta"):
            params[n] = rng.normal(0, 0.2, params[n].shape).astype(np.float32)
    dg.trainval(flags).initialize()
    from dgcnn import _engine as E
    assert E.EDGE_MLP_DTYPE == "bf16"
    set_vars(dg, params)
    dg.ctx().begin_step()
    with capture_layers() as capl:
        logits = host(dg.build(dev(pts), flags))
    idx_list, xin = [], []
    for i in range(L):
        x_i, idx = capl.layers["EdgeConv%d" % i]
        np.testing.assert_array_equal(idx, O.k_nn(x_i, 40), err_msg="layer %d" % i)
        idx_list.append(idx)
        xin.append(x_i)
    p64 = {n: v.astype(np.float64) for n, v in params.items()}
    worst = 0.0
    for i in range(L - 1):                  # layer i on ITS OWN fp32 input -> the input layer i + 1 saw (ops.py:116-138)
        s = "EdgeConv%d/" % i
        outs, _ = O.edge_conv(xin[i].astype(np.float64), 40, p64[s + "conv0/weights"], p64[s + "conv0/BatchNorm/beta"],
                              p64[s + "conv1/weights"], p64[s + "conv1/BatchNorm/beta"], relu1=(i == 0), idx=idx_list[i],
                              edge_mlp_dtype="bf16")
        nxt = outs[2][:, :, 0, :]
        if i > 0:
            nxt = np.maximum(xin[i].astype(np.float64) + nxt, 0)          # relu(shortcut + net), equal widths: ops.py:134
        err = np.abs(xin[i + 1] - nxt).max()
        worst = max(worst, err)
        np.testing.assert_allclose(xin[i + 1], nxt, rtol=0, atol=LAYER_ATOL, err_msg="layer %d output" % i)
    ref, _ = O.model_forward(pts.astype(np.float64), flags, p64, idx_list=idx_list)
    plain, _ = O.model_forward(pts.astype(np.float64), config2_flags(dg, train=False, emd="f32"), p64, idx_list=idx_list)
    e, m = np.abs(logits - ref), np.abs(ref - plain)
    print("configs[2] architecture, bf16 edge-MLP, same graphs: per-layer (same fp32 input) max %.2e | end to end logits "
          "max|HIP - fp64 oracle (bf16 mode)| %.3e (mean %.1e) | bf16-mode oracle vs fp32-operand twin: max %.3e mean %.1e"
          % (worst, e.max(), e.mean(), m.max(), m.mean()))
    assert e.max() <= 6e-2 and e.mean() <= 3e-3, (e.max(), e.mean())
    assert e.mean() * 5 <= m.mean(), (e.mean(), m.mean())


def test_model_gradients_bf16_small(dg):
    """A small residual model (3 layers, k = 10, N = 256) trained one micro-step in bf16 mode: loss and every gradient tensor
    against the float64 oracle in the same mode on the HIP path's graphs."""
    from dgcnn import _engine as E
    B, N, C = 2, 256, 4
    flags = dg.DGCNN_FLAGS(MODEL_NAME="residual-dgcnn", EDGE_CONV_LAYERS=3, EDGE_CONV_FILTERS=64, FC_LAYERS=2, FC_FILTERS=[128, 64],
                           NUM_CLASS=3, KVALUE=10, NUM_CHANNEL=C, TRAIN=True, EDGE_MLP_DTYPE="bf16")
    rng = np.random.default_rng(5)
    pts = rng.random((B, N, C), dtype=np.float32)
    labels = rng.integers(0, 3, (B, N)).astype(np.int32)
    params = O.init_params(flags, C, seed=2)
    keep, E.DROPOUT_KEEP = E.DROPOUT_KEEP, 1.0
    try:
        tv, res, cap = run_model(dg, flags, dev(pts), params, train=True, labels=dev(labels))
    finally:
        E.DROPOUT_KEEP = keep
    idx_list = [cap["EdgeConv%d" % i][1] for i in range(3)]
    p64 = {n: v.astype(np.float64) for n, v in params.items()}
    G, loss, _, _ = O.train_step_grads(pts.astype(np.float64), labels, flags, p64, idx_list=idx_list)
    assert abs(float(res[2]) - float(loss)) < BF16_MODEL_LOSS_TOL
    rel = lambda a, b: np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)
    r = {n: rel(host(tv.gradients[n]).astype(np.float64), G[n]) for n in params}
    print("bf16 edge-MLP, small residual model: worst relative Frobenius gradient error vs the fp64 oracle in the same mode %.2e (%s)"
          % (max(r.values()), max(r, key=r.get)))
    # (measured 1.0e-2 .. 2.0e-2 run to run: a 512-point model, default (atomically summed) statistics, and bf16 operands that
    # turn a last-bit feature difference into a 2^-9 operand difference)
    assert max(r.values()) < BF16_MODEL_GRAD_TOL, r


def test_config2_full_size_property_run_bf16(dg):
    """configs[2] at FULL size (B=8, N=16384, k=40, residual-dgcnn x 6) in its named mode, one training step: finite loss near
    ln 2, finite non-zero gradients for every variable, k-NN lists bit-exact on seeded rows, Adam step finite."""
    from test_gpu_baseline_sizes import _full_size_property_run
    torch.cuda.reset_peak_memory_stats()
    loss = _full_size_property_run(dg, config2_flags(dg, train=True), B=8, N=16384, k=40, L=6, nrows=256, seed=43)
    print("configs[2] full size, bf16 edge-MLP: loss %.5f, peak HBM %.1f GB" % (loss, torch.cuda.max_memory_allocated() / 2 ** 30))


def test_bf16_mode_rejects_unknown_values_and_runs_deterministically(dg):
    """An unknown EDGE_MLP_DTYPE is refused at initialize(); with DETERMINISTIC the mode is bit-reproducible run to run (its
    neighbour gradient is a sum over sorted incoming edges at the points, not an atomic scatter)."""
    from dgcnn import _engine as E
    with pytest.raises(ValueError):
        dg.trainval(dg.DGCNN_FLAGS(EDGE_MLP_DTYPE="fp8")).initialize()
    B, N, C = 2, 256, 3
    rng = np.random.default_rng(9)
    pts = dev(rng.random((B, N, C), dtype=np.float32))
    labels = dev(rng.integers(0, 2, (B, N)).astype(np.int32))
    runs = []
    try:
        for _ in range(2):
            dg.reset()
            f = dg.DGCNN_FLAGS(MODEL_NAME="residual-dgcnn", EDGE_CONV_LAYERS=3, EDGE_CONV_FILTERS=64, FC_LAYERS=1, FC_FILTERS=[64], NUM_CLASS=2,
                               KVALUE=8, NUM_CHANNEL=C, TRAIN=True, SEED=4, EDGE_MLP_DTYPE="bf16", DETERMINISTIC=True)
            tv = dg.trainval(f).initialize()
            for _ in range(2):
                tv.zero_gradients(None)
                tv.accum_gradient(None, [pts], [labels])
                g = host(dg.ctx().flat_grad).copy()
                tv.apply_gradient(None)
            runs.append((g, host(dg.ctx().flat_param).copy()))
    finally:
        E.DETERMINISTIC = E.DETERMINISTIC_ENV_DEFAULT
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
    assert np.abs(runs[0][0]).sum() > 0


@pytest.mark.parametrize("B,N,C,k,F", [(2, 100, 64, 20, 64), (1, 333, 64, 40, 128), (3, 77, 3, 7, 32), (2, 64, 4, 10, 128), (1, 130, 64, 128, 32)])
def test_fused_passes_agree_with_each_other_and_with_the_rounded_product(dg, B, N, C, k, F):
    """csrc/edge_mlp_bf16.hip: the written-out y equals round_bf16(E) round_bf16(W0) accumulated in wide arithmetic (1e-5 of the
    row scale: only the fp32 accumulation differs), and the two passes that never write y -- BatchNorm sums, BN + ReLU + max /
    mean / ties over k -- give exactly what the dense kernels compute from the written-out y (same y bits in all three passes)."""
    from dgcnn import _hip as H
    rng = np.random.default_rng(B * 1000 + F)
    R = B * N
    pts = rng.normal(size=(B, N, C)).astype(np.float32)
    W0 = rng.normal(0, 0.3, (2 * C, F)).astype(np.float32)
    x = dev(pts.reshape(R, C)) if C % 4 == 0 else dev(pts.reshape(R, C))
    idx_h = rng.integers(0, N, (B, N, k)).astype(np.int32)
    idx, W = dev(idx_h), dev(W0)
    assert H.load().dgcnn_edge_mlp_bf16_supported(C, k, F) == 1
    src = (x.data_ptr(), C, idx.data_ptr(), W.data_ptr(), B, N, C, k, F)
    Y = torch.full((R * k, F), float("nan"), device="cuda")
    H.call("dgcnn_edge_mlp_bf16", *src, Y.data_ptr())
    E = O.edges(pts.astype(np.float64), k, idx_h).reshape(R * k, 2 * C)
    ref = O.bf16_round(O.edges(pts, k, idx_h).reshape(R * k, 2 * C)).astype(np.float64) @ O.bf16_round(W0).astype(np.float64)
    got = host(Y).astype(np.float64)
    scale = np.abs(O.bf16_round(E.astype(np.float32)).astype(np.float64)) @ np.abs(O.bf16_round(W0).astype(np.float64))
    assert (np.abs(got - ref) <= 2e-6 * scale + 1e-30).all(), float((np.abs(got - ref) / np.maximum(scale, 1e-30)).max())
    # statistics pass == column sums of the written-out y (fp32 partial sums in a different grouping: 1e-5 relative)
    st = torch.zeros(H.stat_slots() * 2 * F, dtype=torch.float64, device="cuda")
    H.call("dgcnn_edge_mlp_bf16_stats", *src, st.data_ptr())
    s = host(st).reshape(H.stat_slots(), 2, F).sum(0)
    np.testing.assert_allclose(s[0], got.sum(0), rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(s[1], (got * got).sum(0), rtol=1e-5, atol=1e-3)
    # BN + ReLU + k-reduce pass == the dense kernel on the written-out y, bit for bit
    mean, rstd, beta = dev(rng.normal(0, 0.3, F).astype(np.float32)), dev((0.5 + rng.random(F)).astype(np.float32)), dev(rng.normal(0, 0.3, F).astype(np.float32))
    outs = []
    for fused in (True, False):
        mm = torch.zeros((R, 2 * F + 4), device="cuda")
        mx, mn = mm[:, :F], mm[:, F:2 * F]
        cnt = torch.zeros((R, F), device="cuda")
        if fused:
            H.call("dgcnn_edge_mlp_bf16_bn_kreduce", *src, mean.data_ptr(), rstd.data_ptr(), beta.data_ptr(),
                   mx.data_ptr(), H.ld2(mx), mn.data_ptr(), H.ld2(mn), cnt.data_ptr(), 0)
        else:
            H.call("dgcnn_bn_act_kreduce_f32", Y.data_ptr(), R, k, F, mean.data_ptr(), rstd.data_ptr(), beta.data_ptr(), 1,
                   mx.data_ptr(), H.ld2(mx), mn.data_ptr(), H.ld2(mn), 0, 0, cnt.data_ptr())
        outs.append((host(mm).copy(), host(cnt).copy()))
    np.testing.assert_array_equal(outs[0][0][:, :F], outs[1][0][:, :F])            # max
    np.testing.assert_array_equal(outs[0][1], outs[1][1])                          # ties
    np.testing.assert_allclose(outs[0][0][:, F:2 * F], outs[1][0][:, F:2 * F], rtol=0, atol=2e-6)   # mean: the order of the k additions differs


@pytest.mark.parametrize("B,N,C,k,F", [(2, 100, 64, 20, 64), (1, 333, 64, 40, 128), (3, 77, 3, 8, 32), (2, 64, 4, 10, 128), (1, 130, 64, 128, 32),
                                       (2, 50, 64, 9, 64)])
def test_fused_backward_pass_against_the_dense_kernels(dg, B, N, C, k, F):
    """dgcnn_edge_mlp_bf16_bwd (one pass over the edges, y recomputed) against the dense route it replaces -- y written out,
    dgcnn_bn_bwd_apply_f32 with the bf16 rounding flag, E gathered, a separate weight-gradient product: dY bit for bit (as bf16),
    its per-point sums and d(beta) bit for bit, dW0 = round(E)^T dY against float64 (only the fp32 accumulation differs), and the
    transposed-adjacency sum over the bf16 dY equal to the fp32 kernel's over the same values."""
    from dgcnn import _hip as H
    lib = H.load()
    rng = np.random.default_rng(B * 100 + k)
    R = B * N
    pts = rng.normal(size=(B, N, C)).astype(np.float32)
    W0 = rng.normal(0, 0.3, (2 * C, F)).astype(np.float32)
    x, W = dev(pts.reshape(R, C)), dev(W0)
    idx_h = rng.integers(0, N, (B, N, k)).astype(np.int32)
    idx = dev(idx_h)
    assert lib.dgcnn_edge_mlp_bf16_bwd_supported(C, k, F) == 1
    assert lib.dgcnn_edge_mlp_bf16_bwd_supported(64, 7, 64) == 0 and lib.dgcnn_edge_mlp_bf16_bwd_supported(64, 8, 64) == 1
    assert lib.dgcnn_edge_mlp_bf16_bwd_supported(64, 8, 128) == 0 and lib.dgcnn_edge_mlp_bf16_bwd_supported(64, 10, 128) == 1   # LDS
    src = (x.data_ptr(), C, idx.data_ptr(), W.data_ptr(), B, N, C, k, F)
    Y = torch.empty((R * k, F), device="cuda")
    H.call("dgcnn_edge_mlp_bf16", *src, Y.data_ptr())
    mean, rstd, beta = dev(rng.normal(0, 0.3, F).astype(np.float32)), dev((0.5 + rng.random(F)).astype(np.float32)), dev(rng.normal(0, 0.3, F).astype(np.float32))
    mx, mn, cntp = (torch.empty((R, F), device="cuda") for _ in range(3))
    H.call("dgcnn_edge_mlp_bf16_bn_kreduce", *src, mean.data_ptr(), rstd.data_ptr(), beta.data_ptr(), mx.data_ptr(), F, mn.data_ptr(), F,
           cntp.data_ptr(), 1)
    ties = cntp - 256.0 * torch.floor(cntp / 256.0)
    npos = host(torch.floor(cntp / 256.0))
    z = np.maximum((host(Y).reshape(R, k, F) - host(mean)) * host(rstd) + host(beta), 0)
    np.testing.assert_array_equal(npos, (z > 0).sum(1))                                   # the packed half the forward adds
    dmx, dmn = dev(rng.normal(size=(R, F)).astype(np.float32)), dev(rng.normal(size=(R, F)).astype(np.float32))
    red = torch.zeros((H.stat_slots(), 2, F), dtype=torch.float64, device="cuda")
    H.call("dgcnn_edge_bn_bwd_reduce_points_f32", mx.data_ptr(), F, mn.data_ptr(), F, cntp.data_ptr(), dmx.data_ptr(), F, dmn.data_ptr(), F,
           beta.data_ptr(), R, k, F, red.data_ptr())
    redA, redB = red.clone(), red.clone()
    # dense route
    dYd, dysA, dbA = torch.empty_like(Y), torch.empty((R, F), device="cuda"), torch.zeros(F, device="cuda")
    H.call("dgcnn_bn_bwd_apply_f32", Y.data_ptr(), R, k, F, mean.data_ptr(), rstd.data_ptr(), beta.data_ptr(), 3, dmx.data_ptr(), F,
           dmn.data_ptr(), F, mx.data_ptr(), F, ties.data_ptr(), redA.data_ptr(), dYd.data_ptr(), dysA.data_ptr(), F, dbA.data_ptr(), 0.0)
    # fused pass
    need = int(lib.dgcnn_edge_mlp_bf16_bwd_workspace_bytes(B, N, C, k, F))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    dYb = torch.full((R * k, F), float("nan"), dtype=torch.bfloat16, device="cuda")
    dysB, dbB = torch.full((R, F), float("nan"), device="cuda"), torch.zeros(F, device="cuda")
    dW0 = torch.ones((2 * C, F), device="cuda")                                           # accumulated into
    H.call("dgcnn_edge_mlp_bf16_bwd", *src, mean.data_ptr(), rstd.data_ptr(), beta.data_ptr(), mx.data_ptr(), F, cntp.data_ptr(),
           dmx.data_ptr(), F, dmn.data_ptr(), F, redB.data_ptr(), dYb.data_ptr(), dysB.data_ptr(), F, dW0.data_ptr(), dbB.data_ptr(), 0.0,
           ws.data_ptr(), need)
    dY_h = host(dYd)
    np.testing.assert_array_equal(host(dYb.float()), dY_h)
    np.testing.assert_array_equal(host(dysB), host(dysA))
    np.testing.assert_array_equal(host(dbB), host(dbA))
    Eb = O.bf16_round(O.edges(pts, k, idx_h).reshape(R * k, 2 * C)).astype(np.float64)
    ref = Eb.T @ dY_h.astype(np.float64)
    scale = np.abs(Eb).T @ np.abs(dY_h.astype(np.float64))
    got = host(dW0).astype(np.float64) - 1.0
    assert (np.abs(got - ref) <= 3e-6 * scale + 1e-5).all(), float((np.abs(got - ref) / (scale + 1e-30)).max())
    # without an input gradient nothing but dW0 / d(beta) is written
    dW0n, dbN = torch.zeros((2 * C, F), device="cuda"), torch.zeros(F, device="cuda")
    redC = red.clone()
    H.call("dgcnn_edge_mlp_bf16_bwd", *src, mean.data_ptr(), rstd.data_ptr(), beta.data_ptr(), mx.data_ptr(), F, cntp.data_ptr(),
           dmx.data_ptr(), F, dmn.data_ptr(), F, redC.data_ptr(), 0, 0, 0, dW0n.data_ptr(), dbN.data_ptr(), 0.0, ws.data_ptr(), need)
    np.testing.assert_allclose(host(dW0n), host(dW0) - 1.0, rtol=0, atol=1e-5 * float(np.abs(ref).max() + 1))
    # transposed-adjacency sum over the bf16 rows == over the same values stored as fp32
    cws = torch.empty(2 * R, dtype=torch.int32, device="cuda")
    off, rev = torch.empty(R + 1, dtype=torch.int32, device="cuda"), torch.empty(R * k, dtype=torch.int32, device="cuda")
    H.call("dgcnn_edge_csr_build", idx.data_ptr(), B, N, k, cws.data_ptr(), off.data_ptr(), rev.data_ptr())
    srt = torch.empty_like(rev)
    H.call("dgcnn_edge_csr_sort", idx.data_ptr(), B, N, k, off.data_ptr(), rev.data_ptr(), srt.data_ptr())
    rev = srt
    S1, S2 = torch.empty((R, F), device="cuda"), torch.empty((R, F), device="cuda")
    H.call("dgcnn_edge_gather_sum_f32", dYd.data_ptr(), off.data_ptr(), rev.data_ptr(), R, F, S1.data_ptr(), F)
    H.call("dgcnn_edge_gather_sum_bf16", dYb.data_ptr(), off.data_ptr(), rev.data_ptr(), R, F, S2.data_ptr(), F)
    np.testing.assert_array_equal(host(S1), host(S2))
    with pytest.raises(H.HipError):
        H.call("dgcnn_edge_mlp_bf16_bwd", *src[:7], 4, F, mean.data_ptr(), rstd.data_ptr(), beta.data_ptr(), mx.data_ptr(), F, cntp.data_ptr(),
               dmx.data_ptr(), F, dmn.data_ptr(), F, redC.data_ptr(), 0, 0, 0, dW0n.data_ptr(), dbN.data_ptr(), 0.0, ws.data_ptr(), need)


def test_fused_and_unfused_backward_of_a_block_agree(dg):
    """The same block, gradients with the one-pass backward and with the dense route (E.BF16_FUSED_BWD off): equal up to the one
    place where they differ by construction -- the two column sums of the BatchNorm backward come from the per-point outputs in the
    fused route (xhat = z - beta where z > 0) and from the edges in the dense one -- i.e. a few 1e-7 of c1 / c2, which can move a
    dY across a bf16 rounding boundary now and then (2^-9 of that element)."""
    from dgcnn import _engine as E
    B, N, C, k, F = 2, 128, 64, 20, 64
    rng = np.random.default_rng(5)
    pts = rng.random((B, N, C), dtype=np.float32)
    P = {"conv0/weights": rng.normal(0, 0.5, (2 * C, F)).astype(np.float32),
         "conv0/BatchNorm/beta": rng.normal(0, 0.3, F).astype(np.float32),
         "conv1/weights": rng.normal(0, 0.3, (2 * F, 64)).astype(np.float32),
         "conv1/BatchNorm/beta": rng.normal(0, 0.3, 64).astype(np.float32)}
    d = None
    res = []
    try:
        for fused in (True, False):
            dg.reset()
            E.EDGE_MLP_DTYPE = "bf16"
            E.BF16_FUSED_BWD = fused
            c = dg.ctx()
            c.begin_step()
            c.recording = True
            x = c.new_buffer(B * N, C)
            x.copy_(dev(pts.reshape(B * N, C)))
            for n, v in P.items():
                c.get_variable(n, v.shape)
            set_vars(dg, P)
            calls = []
            orig = E.H.call
            E.H.call = lambda name, *a, **kw: (calls.append(name), orig(name, *a, **kw))[1]
            try:
                outs = dg.ops.edge_conv(x.view(B, N, C), k, F, True)
                if d is None:
                    d = [rng.normal(size=tuple(o.shape)).astype(np.float32) for o in outs]
                for t, g in zip(outs, d):
                    v, _, _ = E.as2d(t)
                    c.grad(v).copy_(dev(g.reshape(B * N, -1)))
                c.backward()
            finally:
                E.H.call = orig
            assert ("dgcnn_edge_mlp_bf16_bwd" in calls) == fused and ("dgcnn_edge_gather_f32" in calls) == (not fused)
            res.append({n: host(c.var_grads[n]).copy() for n in P} | {"dx": host(c.grad(x)).copy()})
    finally:
        E.BF16_FUSED_BWD = True
    for n in res[0]:
        a, b = res[0][n], res[1][n]
        assert np.abs(a - b).max() <= 2e-3 * max(1.0, np.abs(b).max()), (n, np.abs(a - b).max())
        assert np.median(np.abs(a - b)) <= 1e-5 * max(1.0, np.abs(b).max()), n

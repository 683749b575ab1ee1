"""model.build, trainval and the launch plan on wide EdgeConv stacks: EDGE_CONV_FILTERS beyond 128 and point features beyond 128.

What reaches the k-NN.  conv1 of every EdgeConv block emits 64 channels (ops.py:63), so layer l + 1 always searches 64-channel rows
whatever EDGE_CONV_FILTERS says; the search is wider than 128 only for layer 0 of a cloud with more than 128 input features
(NUM_CHANNEL).  The configurations below therefore come in three kinds:
  channels = 4,   switch at its default   the wide filter stack on raw coordinates: the edge passes, BatchNorm kernels and GEMMs at
                                          F = 192, 256, 132; no search is wide (this kind passes without knn_wide.hip);
  channels = 192, switch at its default   layer 0 searches C = 192: knn_wide_kernel inside the model, layers 1 .. 3 as always;
  channels = 192, dgcnn_knn_wide_min_c(5) every layer's search runs knn_wide_kernel (C = 192, then 64).
Without csrc/knn_wide.hip the two kinds with 192 channels stop with "C=192 > 128 unsupported".

Bars: the project's own for small configurations (tests/test_gpu_parity.py, tests/test_gpu_seg_bn.py): every
layer's graph bit-exact against the oracle's k-NN of that layer's captured input, logits within 1e-3 absolute of the float64 twin fed
the HIP graphs, gradients of accum_gradient within 5e-3 relative Frobenius per tensor.  Every graph the model computes is checked on
the host (all indices inside the row's own cloud) before anything gathers with it.  The module refuses to build a model when a
kernel-level comparison of tests/test_gpu_knn_wide.py has failed in the same process: its tests are skipped then."""
import numpy as np
import pytest
import torch

from oracle import dgcnn_oracle as O
import seg_bn_reference as SR
from gpu_helpers import capture_layers, dev, host, set_vars
from test_gpu_knn_adversarial import forced
from test_gpu_seg_bn import graphs_of, offsets_of
import test_gpu_knn_wide as KW

pytestmark = pytest.mark.gpu

K, B, N, NCLS = 8, 2, 200, 3
STACKS = {"dgcnn": [64, 192, 256, 132], "residual-dgcnn": [192, 192, 192, 192]}
KINDS = [(4, 129), (192, 129), (192, 5)]
PACKED_SIZES = [21, 130, 64, 85]


@pytest.fixture()
def dg():
    import dgcnn
    from dgcnn import _engine as E
    if KW._FAILED:
        pytest.skip("kernel-level k-NN comparisons failed in this process (%d, first: %s): no model is built on such graphs"
                    % (len(KW._FAILED), KW._FAILED[0]))
    dgcnn.reset()
    yield dgcnn
    E.DETERMINISTIC = E.DETERMINISTIC_ENV_DEFAULT
    dgcnn.reset()


@pytest.fixture()
def checked(monkeypatch):
    """E.knn with the host's check behind it (eager runs only: it synchronises)."""
    from dgcnn import _engine as E
    real_knn = E.knn

    def checked_knn(x2d, B_, N_, k, seed=None, seg=None):     # every graph of the model: host-checked before anything gathers with it
        idx = real_knn(x2d, B_, N_, k, seed=seed, seg=seg)
        torch.cuda.synchronize()
        g = host(idx).reshape(-1, k)
        if seg is None:
            lo, hi = 0, N_                                    # dense graphs hold cloud-local indices
        else:
            n = np.diff(seg.host)
            lo, hi = np.repeat(seg.host[:-1], n)[:, None], np.repeat(seg.host[1:], n)[:, None]
        assert ((g >= lo) & (g < hi)).all(), "a graph of the model (C = %d): an index outside the row's own cloud" % x2d.shape[1]
        return idx
    monkeypatch.setattr(E, "knn", checked_knn)


def flags_of(dg, model, channels, **kw):
    base = dict(MODEL_NAME=model, EDGE_CONV_LAYERS=4, EDGE_CONV_FILTERS=list(STACKS[model]), KVALUE=K, NUM_CLASS=NCLS, FC_LAYERS=2,
                FC_FILTERS=[64, 32], TRAIN=False, NUM_CHANNEL=channels)
    base.update(kw)
    return dg.DGCNN_FLAGS(**base)


def params_of(flags, rng, channels):
    params = O.init_params(flags, channels, seed=1)
    for n in params:
        if n.endswith("beta"):
            params[n] = rng.normal(0, 0.2, params[n].shape).astype(np.float32)
    return params


def run(dg, flags, params, pts, train, labels=None):
    tv = dg.trainval(flags).initialize()
    set_vars(dg, params)
    with capture_layers() as cap:
        if train:
            tv.zero_gradients(None)
            res = tv.accum_gradient(None, [pts], [labels])
        else:
            res = tv.inference(None, [pts], [labels])
    return tv, res, cap.layers


def dense_graphs(layers, L):
    """The captured graphs, each bit-exact against the oracle's k-NN of the layer's own captured input."""
    out = []
    for i in range(L):
        xin, idx = layers["EdgeConv%d" % i]
        want = O.k_nn(xin, K)
        KW.same(idx, want, 0, xin.shape[1], "model layer %d (C = %d)" % (i, xin.shape[2]))
        out.append(idx)
    return out


@pytest.mark.parametrize("channels,min_c", KINDS, ids=["ch%d-minc%d" % c for c in KINDS])
@pytest.mark.parametrize("model", sorted(STACKS))
def test_dense_model_logits_and_gradients(dg, checked, model, channels, min_c):
    import dgcnn
    from dgcnn import _engine as E
    rng = np.random.default_rng(3)
    flags = flags_of(dg, model, channels)
    pts = rng.random((B, N, channels), dtype=np.float32)
    labels = rng.integers(0, NCLS, (B, N)).astype(np.int32)
    params = params_of(flags, rng, channels)
    p64 = {n: v.astype(np.float64) for n, v in params.items()}
    with forced(wide_min_c=min_c):
        assert E._knn_wide(192) and E._knn_wide(64) == (min_c == 5)
        tv, res, layers = run(dg, flags, params, pts, train=False, labels=labels)
        widths = [layers["EdgeConv%d" % i][0].shape[2] for i in range(4)]
        assert widths == [channels, 64, 64, 64]                        # what every layer searches
        idx_list = dense_graphs(layers, 4)
        ref, _ = O.model_forward(pts.astype(np.float64), flags, p64, idx_list=idx_list)
        dg.ctx().recording = False
        logits = host(dgcnn.build(dev(pts), flags))
        err = np.abs(logits - ref)
        print("%s channels=%d min_c=%d: logits max |err| vs the float64 twin %.3g" % (model, channels, min_c, err.max()))
        assert logits.shape == (B, N, NCLS) and err.max() <= 1e-3, err.max()

        flags.TRAIN = True
        keep = E.DROPOUT_KEEP
        E.DROPOUT_KEEP = 1.0
        try:
            tv, res, layers = run(dg, flags, params, pts, train=True, labels=labels)
        finally:
            E.DROPOUT_KEEP = keep
        idx_list = dense_graphs(layers, 4)
        G, loss64, _, _ = O.train_step_grads(pts.astype(np.float64), labels, flags, p64, idx_list=idx_list)
        assert abs(float(res[2]) - float(loss64)) < 1e-3
        worst = (0.0, "")
        for n in params:
            g = host(tv.gradients[n]).astype(np.float64)
            worst = max(worst, (float(np.linalg.norm(g - G[n]) / max(np.linalg.norm(G[n]), 1e-6)), n))
        print("%s channels=%d min_c=%d: worst relative Frobenius gradient error vs the float64 twin %.2e (%s)"
              % (model, channels, min_c, worst[0], worst[1]))
        assert worst[0] <= 5e-3, worst


@pytest.mark.parametrize("channels,min_c", KINDS, ids=["ch%d-minc%d" % c for c in KINDS])
@pytest.mark.parametrize("model", sorted(STACKS))
def test_packed_model_logits_per_cloud(dg, checked, model, channels, min_c):
    import dgcnn
    rng = np.random.default_rng(5)
    flags = flags_of(dg, model, channels, BN_PER_CLOUD=True)
    off = offsets_of(PACKED_SIZES)
    R = int(off[-1])
    pts = rng.random((R, channels), dtype=np.float32)
    params = params_of(flags, rng, channels)
    p64 = {n: v.astype(np.float64) for n, v in params.items()}
    with forced(wide_min_c=min_c):
        dg.trainval(flags).initialize()
        set_vars(dg, params)
        with capture_layers() as cap:
            logits = host(dgcnn.build(dev(pts), flags, offsets=off))
        assert logits.shape == (1, R, NCLS)
        graphs = graphs_of(cap, 4, off, K)                              # per cloud, bit for bit, plus offsets[b]
    ref = SR.model_forward(pts.astype(np.float64), off, flags, p64, graphs)
    err = np.abs(logits - ref)
    print("%s channels=%d min_c=%d packed: logits max |err| vs the per-cloud float64 twin %.3g" % (model, channels, min_c, err.max()))
    assert err.max() <= 1e-3, err.max()


@pytest.mark.parametrize("channels", [4, 192])
def test_a_training_step_under_a_launch_plan_equals_the_eager_step(dg, channels):
    """Compared the way tests/test_gpu_graph.py compares (deterministic kernels): the gradient bucket -- what training depends on -- and
    the accuracy bit for bit; the REPORTED loss is summed with atomics in both modes (last bit), so it is held to that module's 1e-6.
    A plan is recorded the second time a shape is seen and replayed from the third call on: four steps each way, every one compared."""
    import dgcnn
    rng = np.random.default_rng(9)
    pts = torch.from_numpy(rng.random((B, N, channels), dtype=np.float32)).cuda()
    lab = torch.from_numpy(rng.integers(0, NCLS, (B, N)).astype(np.int32)).cuda()

    def steps(graph):
        flags = flags_of(dgcnn, "dgcnn", channels, TRAIN=True, SEED=11, LEARNING_RATE=1e-3, DETERMINISTIC=True)
        tv = dgcnn.trainval(flags).initialize().use_graph(graph)
        out = []
        for s in range(4):
            tv.zero_gradients(None)
            res = tv.accum_gradient(None, [pts], [lab])
            out.append((float(res[2]), float(res[1]), host(res[0]).copy()))
        return tv, out
    tv_e, eager = steps(False)
    tv_p, plan = steps("plan")
    info = tv_p.launch_plan_info()
    assert len(info) == 1 and info[0]["kernels"] > 60 and not tv_e.launch_plan_info(), info
    for s, ((le, ae, ge), (lp, ap, gp)) in enumerate(zip(eager, plan)):
        assert np.isfinite(le) and np.abs(ge).max() > 0
        assert abs(lp - le) <= 1e-6, (s, lp, le)
        assert ap == ae, (s, ap, ae)
        np.testing.assert_array_equal(gp, ge, err_msg="step %d: gradient bucket" % s)

"""flags.LOSS_PER_CLOUD through the stack (run with -m gpu on an MI355X): trainval.accum_gradient on a packed tower against the
float64 oracle run on every cloud ALONE and summed (tests/loss_per_cloud_reference.py), against four real -mbs 1 micro-steps, a
dense (B, N, C) tower against the packed one, launch-plan replay, reproducibility, the switch, and the inference loop's per-entry
rows."""
import numpy as np
import pytest
import torch

from oracle import dgcnn_oracle as O
import loss_per_cloud_reference as LP
from gpu_helpers import capture_layers, host, set_vars

pytestmark = pytest.mark.gpu
F32 = np.float32

TOWER_SIZES = [21, 700, 64, 333]
MODELS = [("dgcnn", 2), ("dgcnn", 0), ("residual-dgcnn", 2), ("residual-dgcnn", 0), ("residual-dgcnn-nofc", 2)]
NEW_ENTRY = "dgcnn_seg_softmax_xent_f32"
DENSE_ENTRY = "dgcnn_softmax_xent_f32"


@pytest.fixture()
def dg():
    import dgcnn
    from dgcnn import _engine as E
    dgcnn.reset()
    yield dgcnn
    E.DETERMINISTIC = E.DETERMINISTIC_ENV_DEFAULT
    E.EDGE_MLP_DTYPE = "f32"
    dgcnn.reset()


def offsets_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def fro(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-9))


def model_flags(dg, model, fcl, det=True, **kw):
    base = dict(MODEL_NAME=model, EDGE_CONV_LAYERS=2, EDGE_CONV_FILTERS=[32, 64], KVALUE=20, NUM_CLASS=3, FC_LAYERS=fcl,
                FC_FILTERS=[64, 32][:fcl] if fcl else 64, TRAIN=True, NUM_CHANNEL=4, DETERMINISTIC=None if det else False,
                BN_PER_CLOUD_TRAIN=True, LOSS_PER_CLOUD=True)
    base.update(kw)
    return dg.DGCNN_FLAGS(**base)


def make_tower(rng, sizes, C, ncls):
    pts = np.concatenate([rng.random((n, C), dtype=np.float32) for n in sizes])
    return pts, offsets_of(sizes), rng.integers(0, ncls, len(pts)).astype(np.int32), (rng.random(len(pts), dtype=np.float32) + 0.5)


def random_params(flags, rng, C):
    params = O.init_params(flags, C, seed=1)
    for n in params:
        if n.endswith("beta"):
            params[n] = rng.normal(0, 0.2, params[n].shape).astype(np.float32)
    return params


class no_dropout(object):
    def __enter__(self):
        from dgcnn import _engine as E
        self.E, self.keep = E, E.DROPOUT_KEEP
        E.DROPOUT_KEEP = 1.0

    def __exit__(self, *exc):
        self.E.DROPOUT_KEEP = self.keep
        return False


class logits_of_the_loss(object):
    """Records the (R, ncls) logits every E.softmax_loss call receives (device clones, in call order)."""

    def __enter__(self):
        from dgcnn import _engine as E
        self.E, self.orig, self.seen = E, E.softmax_loss, []

        def hook(logits2d, *a, **kw):
            self.seen.append(logits2d.clone())
            return self.orig(logits2d, *a, **kw)
        E.softmax_loss = hook
        return self

    def __exit__(self, *exc):
        self.E.softmax_loss = self.orig
        return False


def tower_scalars64(ref):
    """The kernel's tower scalars from float64 per-cloud values: clouds added b-ascending in double, times 1.0 / nseg."""
    nseg = len(ref["n"])
    tl = ta = 0.0
    for b in range(nseg):
        tl += ref["loss"][b]
        ta += ref["count"][b] / ref["n"][b]
    return tl * (1.0 / nseg), ta * (1.0 / nseg)


def graphs_of(cap, L, off, k):
    out = []
    for i in range(L):
        xin, idx = cap.layers["EdgeConv%d" % i]
        assert idx.shape == (1, off[-1], k)
        out.append(idx)
    return out


# ------------------------------------------------------------------------------------------
# 1. accum_gradient against the oracle, cloud by cloud
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", [True, False], ids=["default", "atomics"])
@pytest.mark.parametrize("model,fcl", MODELS, ids=["%s-fc%d" % m for m in MODELS])
def test_accum_gradient_sums_the_clouds(dg, model, fcl, det):
    """Four unequal clouds with row weights, dropout off, BN_PER_CLOUD_TRAIN + LOSS_PER_CLOUD: every gradient tensor within 5e-3
    (default mode) / 2e-2 (DETERMINISTIC=False) relative Frobenius of sum_b oracle.train_step_grads(cloud b, weight_b) in float64,
    fed the captured graphs.  The reported loss: within 1e-6 of the oracle's mean_b l_b (measured: 1.6e-7 at the worst); the
    accuracy exact: every cloud's count of correct rows is the oracle's, and the reported value is float32 of the b-ascending
    double mean of count_b / n_b.  Both are also held against float64 of the logits the step itself handed to the loss."""
    from dgcnn import _engine as E
    rng = np.random.default_rng(17)
    flags = model_flags(dg, model, fcl, det)
    pts, off, lab, wgt = make_tower(rng, TOWER_SIZES, 4, 3)
    params = random_params(flags, rng, 4)
    with no_dropout():
        tv = dg.trainval(flags).initialize()
        set_vars(dg, params)
        assert E.DETERMINISTIC == det
        tv.zero_gradients(None)
        with capture_layers() as cap, logits_of_the_loss() as rec:
            res = tv.accum_gradient(None, [pts], [lab], [wgt], offsets=[off])
    graphs = graphs_of(cap, 2, off, 20)
    G, l64, a64 = LP.train_step_grads(pts, lab, off, flags, params, graphs, wgt)
    worst = (0.0, "")
    for n in params:
        worst = max(worst, (fro(host(tv.gradients[n]).astype(np.float64), G[n]), n))
    assert len(rec.seen) == 1
    own = LP.xent(host(rec.seen[0]), lab, wgt, off)
    loss_own, acc_own = tower_scalars64(own)
    loss, acc = float(res[2]), float(res[1])
    tag = "%s fc%d %s" % (model, fcl, "det" if det else "atomics")
    print("%s: loss %.9g (float64 of its own logits %.9g, oracle %.9g), accuracy %.9g (%.9g, oracle %.9g)"
          % (tag, loss, loss_own, np.mean(l64), acc, acc_own, np.mean(a64)))
    print("%s: worst relative Frobenius gradient error %.3g (%s)" % (tag, worst[0], worst[1]))
    assert abs(loss - loss_own) <= 1e-6
    assert F32(acc) == F32(acc_own)
    assert abs(loss - float(np.mean(l64))) <= 1e-6
    assert (own["count"] == np.rint(np.asarray(a64, np.float64) * TOWER_SIZES)).all()     # (the oracle's a_b is a float32 mean)
    per = tv.per_cloud_scalars()
    assert len(per) == 1 and tuple(per[0].shape) == (4, 2)
    pc = host(per[0])
    assert np.abs(pc[:, 0] - own["loss"]).max() <= 1e-6 and (pc[:, 1] == (own["count"] / own["n"]).astype(F32)).all()
    assert worst[0] <= (5e-3 if det else 2e-2), worst


# ------------------------------------------------------------------------------------------
# 2. one packed step = four -mbs 1 micro-steps
# ------------------------------------------------------------------------------------------
def test_packed_step_is_four_mbs1_micro_steps(dg):
    """EDGE_CONV_LAYERS = 1: the only graph is the raw-coordinate one, which the packed k-NN reproduces bit for bit per cloud.
    flat_grad after ONE packed step under both flags lies within 1e-2 relative Frobenius of flat_grad after the four -mbs 1
    accum_gradient calls (each side is within the project's 5e-3 of float64: triangle inequality); the reported loss within 1e-6
    of the mean of the four reported losses; the accuracy the same: every cloud's count of correct rows agrees, the packed value
    is float32(mean_b count_b / n_b) exactly, and the -mbs 1 mean -- fp32 partial sums per block, then an fp32 mean -- lies within
    1e-6 of it.  With LOSS_PER_CLOUD off the same comparison exceeds 0.5: the tower-wide mean is another objective."""
    rng = np.random.default_rng(23)
    kw = dict(EDGE_CONV_LAYERS=1, EDGE_CONV_FILTERS=[32], FC_FILTERS=[64, 32])
    pts, off, lab, wgt = make_tower(rng, TOWER_SIZES, 4, 3)
    flags = model_flags(dg, "dgcnn", 2, **kw)
    params = random_params(flags, rng, 4)
    nseg = len(TOWER_SIZES)
    with no_dropout():
        tv = dg.trainval(model_flags(dg, "dgcnn", 2, BN_PER_CLOUD_TRAIN=False, LOSS_PER_CLOUD=False, **kw)).initialize()
        set_vars(dg, params)
        tv.zero_gradients(None)
        step = []
        for b in range(nseg):
            lo, hi = int(off[b]), int(off[b + 1])
            res = tv.accum_gradient(None, [pts[None, lo:hi]], [lab[None, lo:hi]], [wgt[None, lo:hi]], last=(b == nseg - 1))
            step.append((float(res[2]), float(res[1])))
        want = host(tv._ctx.flat_grad).astype(np.float64)
        got = {}
        for lpc in (True, False):
            tv = dg.trainval(model_flags(dg, "dgcnn", 2, LOSS_PER_CLOUD=lpc, **kw)).initialize()
            set_vars(dg, params)
            tv.zero_gradients(None)
            res = tv.accum_gradient(None, [pts], [lab], [wgt], offsets=[off])
            got[lpc] = (host(tv._ctx.flat_grad).astype(np.float64), float(res[2]), float(res[1]), tv.per_cloud_scalars())
    d_on, d_off = fro(got[True][0], want), fro(got[False][0], want)
    loss1, acc1 = float(np.mean([s[0] for s in step])), float(np.mean([s[1] for s in step]))
    print("packed vs four -mbs 1 steps: relative Frobenius %.3g under the flag, %.3g without; loss %.9g vs %.9g, accuracy %.9g vs %.9g"
          % (d_on, d_off, got[True][1], loss1, got[True][2], acc1))
    assert d_on <= 1e-2
    assert d_off > 0.5
    assert abs(got[True][1] - loss1) <= 1e-6
    pc = host(got[True][3][0])
    counts = np.rint(pc[:, 1].astype(np.float64) * TOWER_SIZES)
    assert (counts == np.rint(np.array([s[1] for s in step], np.float64) * TOWER_SIZES)).all()
    assert (pc[:, 1] == (counts / TOWER_SIZES).astype(F32)).all()
    t = 0.0
    for b in range(nseg):
        t += counts[b] / TOWER_SIZES[b]
    assert F32(got[True][2]) == F32(t * (1.0 / nseg))
    assert abs(got[True][2] - acc1) <= 1e-6
    assert got[False][3] == []                                                       # flag off: no per-cloud tensors


# ------------------------------------------------------------------------------------------
# 3. a dense (B, N, C) tower
# ------------------------------------------------------------------------------------------
def test_dense_tower_is_the_packed_tower_with_offsets_bN(dg):
    """(4, 256, C) under both flags = the packed tower with offsets b * 256, bit for bit: logits, loss, accuracy, flat_grad and
    the per-cloud tensor.  B = 1 is one cloud already: the dense call, the same numbers with and without the flag."""
    rng = np.random.default_rng(31)
    flags = model_flags(dg, "dgcnn", 2)
    pts = rng.random((4, 256, 4), dtype=np.float32)
    lab = rng.integers(0, 3, (4, 256)).astype(np.int32)
    wgt = rng.random((4, 256), dtype=np.float32) + 0.5
    params = random_params(flags, rng, 4)
    out = []
    with no_dropout():
        for data, label, weight, kw in ((pts, lab, wgt, {}),
                                        (pts.reshape(1024, 4), lab.reshape(1024), wgt.reshape(1024), {"offsets": [np.arange(5) * 256]})):
            tv = dg.trainval(flags).initialize()
            set_vars(dg, params)
            tv.zero_gradients(None)
            with logits_of_the_loss() as rec:
                res = tv.accum_gradient(None, [data], [label], [weight], **kw)
            out.append((rec.seen[0].reshape(1024, 3).clone(), tv._ctx.flat_grad.clone(), res[2].clone(), res[1].clone(),
                        tv.per_cloud_scalars()[0].clone()))
        for a, b in zip(*out):
            assert torch.equal(a, b), int((a != b).sum())
        assert tuple(out[0][4].shape) == (4, 2)
        one = []
        for lpc in (True, False):
            tv = dg.trainval(model_flags(dg, "dgcnn", 2, LOSS_PER_CLOUD=lpc)).initialize()
            set_vars(dg, params)
            tv.zero_gradients(None)
            res = tv.accum_gradient(None, [pts[:1]], [lab[:1]], [wgt[:1]])
            one.append((tv._ctx.flat_grad.clone(), float(res[2]), float(res[1])))
            assert [tuple(t.shape) for t in tv.per_cloud_scalars()] == ([(1, 2)] if lpc else [])
        assert torch.equal(one[0][0], one[1][0])
        assert abs(one[0][1] - one[1][1]) <= 1e-6 and abs(one[0][2] - one[1][2]) <= 1e-6     # (the dense sums are atomics: last bit)


def _train(dg, graph, steps, pts, lab, **kw):
    flags = dg.DGCNN_FLAGS(EDGE_CONV_LAYERS=2, EDGE_CONV_FILTERS=[64, 64], KVALUE=10, FC_LAYERS=2, FC_FILTERS=[128, 64], NUM_CLASS=2,
                           NUM_CHANNEL=3, TRAIN=True, SEED=11, LEARNING_RATE=1e-3, DETERMINISTIC=True, LOSS_PER_CLOUD=True, **kw)
    tv = dg.trainval(flags).initialize().use_graph(graph)
    scal, clouds = [], []
    for s in range(steps):
        tv.zero_gradients(None)
        for micro in range(2):
            res = tv.accum_gradient(None, [pts[s]], [lab[s]])
            scal.append((float(res[2]), float(res[1])))
            clouds.append(host(tv.per_cloud_scalars()[0]).copy())
        tv.apply_gradient(None)
    return tv, scal, clouds, dg.ctx().flat_param.cpu().numpy().copy()


def test_launch_plan_replay_of_a_dense_tower_equals_the_eager_steps(dg):
    """A dense (4, 512, 3) tower under LOSS_PER_CLOUD alone (tower-wide BatchNorm: the step can be recorded), deterministic kernels,
    dropout on: three updates of two micro-steps replayed from ONE launch plan equal the eager run bit for bit -- parameters, and
    here also every reported loss, accuracy and per-cloud tensor (the new sums are fixed-order) -- and the plan holds the new
    call's two launches."""
    rng = np.random.default_rng(5)
    pts = torch.from_numpy(rng.random((3, 4, 512, 3), dtype=np.float32)).cuda()
    lab = torch.from_numpy(rng.integers(0, 2, (3, 4, 512)).astype(np.int32)).cuda()
    tv_e, scal_e, clouds_e, p_e = _train(dg, False, 3, pts, lab)
    tv_p, scal_p, clouds_p, p_p = _train(dg, "plan", 3, pts, lab)
    assert len(tv_p._graphs) == 1 and not tv_e._graphs
    assert scal_p == scal_e
    for a, b in zip(clouds_p, clouds_e):
        assert a.shape == (4, 2) and np.array_equal(a, b)
    np.testing.assert_array_equal(p_p, p_e)
    # the flag is part of the plan's key: the same shape without it is another recording
    key_on = next(iter(tv_p._graphs))
    tv_off = dg.trainval(dg.DGCNN_FLAGS(EDGE_CONV_LAYERS=2, EDGE_CONV_FILTERS=[64, 64], KVALUE=10, FC_LAYERS=2, FC_FILTERS=[128, 64],
                                        NUM_CLASS=2, NUM_CHANNEL=3, TRAIN=True, SEED=11, DETERMINISTIC=True)).initialize().use_graph("plan")
    for _ in range(2):
        tv_off.zero_gradients(None)
        tv_off.accum_gradient(None, [pts[0]], [lab[0]])
    key_off = next(iter(tv_off._graphs))
    assert key_off != key_on and len(key_off) == len(key_on)
    assert [a for a, b in zip(key_on, key_off) if a != b] == [True]
    on, off = tv_p.launch_plan_info()[0], tv_off.launch_plan_info()[0]
    assert on["kernels"] == off["kernels"] + 1 and on["memsets"] == off["memsets"] - 1, (on, off)   # two launches for launch + zero fill


# ------------------------------------------------------------------------------------------
# 4. reproducibility, the switch
# ------------------------------------------------------------------------------------------
def test_training_steps_report_bit_identical_loss_and_accuracy(dg):
    """Default (deterministic) mode, dropout on: two training steps from the same seed, done twice, report == loss and accuracy
    (the per-cloud sums have one fixed order; the tower-wide loss needed `< 1e-6`) and leave bit-identical parameters."""
    rng = np.random.default_rng(3)
    flags = model_flags(dg, "residual-dgcnn", 2)
    pts, off, lab, wgt = make_tower(rng, TOWER_SIZES, 4, 3)
    runs = []
    for _ in range(2):
        tv = dg.trainval(flags).initialize()
        scal = []
        for _ in range(2):
            tv.zero_gradients(None)
            res = tv.accum_gradient(None, [pts], [lab], [wgt], offsets=[off])
            tv.apply_gradient(None)
            scal.append((float(res[2]), float(res[1]), host(tv.per_cloud_scalars()[0]).tolist()))
        assert np.isfinite(scal[-1][0])
        runs.append((scal, tv._ctx.flat_param.clone()))
    assert runs[0][0] == runs[1][0]
    assert runs[0][0][0][0] != runs[0][0][1][0]                                      # (it trained: the second step's loss moved)
    assert torch.equal(runs[0][1], runs[1][1])


def test_switch_off_launches_no_new_entry(dg, monkeypatch):
    """Flag off: a packed training step, a dense one and an inference call issue dgcnn_softmax_xent_f32 and never the new entry.
    Flag on: towers of several clouds issue the new entry and not the dense one; a one-cloud tower -- B = 1, or a packed tower of
    one cloud -- issues dgcnn_softmax_xent_f32 as it does today."""
    from dgcnn import _hip as H
    rng = np.random.default_rng(5)
    pts, off, lab, wgt = make_tower(rng, TOWER_SIZES, 4, 3)
    dense = rng.random((2, 64, 4), dtype=np.float32)
    dlab = rng.integers(0, 3, (2, 64)).astype(np.int32)
    orig = H.call

    def record(fn):
        names = []
        monkeypatch.setattr(H, "call", lambda name, *a, _n=names, **kw: (_n.append(name), orig(name, *a, **kw))[1])
        try:
            fn()
        finally:
            monkeypatch.setattr(H, "call", orig)
        return [n for n in names if n in (NEW_ENTRY, DENSE_ENTRY)]

    for on in (False, True):
        tv = dg.trainval(model_flags(dg, "residual-dgcnn", 2, LOSS_PER_CLOUD=on)).initialize()
        tv.zero_gradients(None)
        many = NEW_ENTRY if on else DENSE_ENTRY
        assert record(lambda: tv.accum_gradient(None, [pts], [lab], [wgt], offsets=[off])) == [many]
        assert record(lambda: tv.accum_gradient(None, [dense], [dlab])) == [many]
        assert record(lambda: tv.inference(None, [pts], [lab], offsets=[off])) == [many]
        assert record(lambda: tv.inference(None, [pts], offsets=[off])) == [many]                         # no labels: softmax only
        assert record(lambda: tv.accum_gradient(None, [dense[:1]], [dlab[:1]])) == [DENSE_ENTRY]
        assert record(lambda: tv.accum_gradient(None, [pts[:700]], [lab[:700]], offsets=[[0, 700]])) == [DENSE_ENTRY]


# ------------------------------------------------------------------------------------------
# 5. the inference loop
# ------------------------------------------------------------------------------------------
def test_inference_loop_writes_one_row_per_entry(dg, tmp_path, capsys):
    """Eight clouds of 256 ... 1400 points, `inference --pack_towers 1 --bn_per_cloud 1 --loss_per_cloud 1 -mbs 4`: the per-entry
    CSV has eight rows (entry, points, loss, accuracy) whose loss is within 1e-5 of the float64 loss of the WRITTEN softmax and the
    labels and whose accuracy equals float32(count / points); the main CSV keeps its columns; without the flag no second file."""
    from dgcnn import main_funcs as M
    rng = np.random.default_rng(4)
    counts = [300, 1400, 517, 256, 256, 777, 1100, 400]
    off = offsets_of(counts)
    pts = rng.random((off[-1], 4), dtype=np.float32)
    lab = (pts[:, 0] > 0.5).astype(np.int32)
    np.savez(tmp_path / "ragged.npz", data=pts, label=lab, data_offsets=off)
    common = dict(IO_TYPE="npz", INPUT_FILE=str(tmp_path / "ragged.npz"), NUM_POINT=-1, NUM_CHANNEL=-1, BATCH_SIZE=8, MINIBATCH_SIZE=4,
                  PACK_TOWERS=True, SHUFFLE=0, KVALUE=8, EDGE_CONV_LAYERS=2, EDGE_CONV_FILTERS=[32, 64], FC_LAYERS=1, FC_FILTERS=[64],
                  NUM_CLASS=2, REPORT_STEP=0, SEED=5, ITERATION=1, BN_PER_CLOUD=True)
    g = dg.DGCNN_FLAGS(OUTPUT_FILE=str(tmp_path / "out.npz"), LOG_DIR=str(tmp_path / "log"), LOSS_PER_CLOUD=True, **common)
    M.inference(g)
    capsys.readouterr()
    z = np.load(tmp_path / "out.npz")
    sm = z["softmax"].astype(np.float64)
    assert z["idx"].tolist() == list(range(8)) and sm.shape == (sum(counts), 2)
    lines = open(tmp_path / "log" / "inference_entries-0000000.csv").read().strip().split("\n")
    assert lines[0] == M.ENTRY_COLUMNS == "entry,points,loss,accuracy" and len(lines) == 9
    losses, accs = [], []
    for b, line in enumerate(lines[1:]):
        entry, points, loss, acc = line.split(",")
        lo, hi = int(off[b]), int(off[b + 1])
        assert int(entry) == b and int(points) == counts[b]
        want = float(-np.log(sm[np.arange(lo, hi), lab[lo:hi]]).mean())
        count = int((np.argmax(sm[lo:hi], 1) == lab[lo:hi]).sum())
        assert abs(float(loss) - want) <= 1e-5, (b, loss, want)
        assert F32(float(acc)) == F32(count / counts[b]), (b, acc, count)
        losses.append(float(loss))
        accs.append(float(acc))
    main = open(tmp_path / "log" / "inference_log-0000000.csv").read().strip().split("\n")
    assert main[0] == M.INFERENCE_COLUMNS == "iter,epoch,titer,tinference,tio,tsumiter,tsuminference,tsumio,loss,accuracy"
    assert len(main) == 2 and len(main[1].split(",")) == 10
    # its loss / accuracy: the mean over the two towers of the mean over their four clouds
    assert abs(float(main[1].split(",")[-2]) - np.mean(losses)) <= 1e-5 and abs(float(main[1].split(",")[-1]) - np.mean(accs)) <= 1e-5
    h = dg.DGCNN_FLAGS(LOG_DIR=str(tmp_path / "log_off"), **common)
    M.inference(h)
    capsys.readouterr()
    assert sorted(p.name for p in (tmp_path / "log_off").iterdir()) == ["inference_log-0000000.csv"]

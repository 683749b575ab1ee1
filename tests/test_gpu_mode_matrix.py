"""The run modes in combination (run with -m gpu on an MI355X): DETERMINISTIC x EDGE_MLP_DTYPE x HEAD_PLANES x packed towers (with
and without per-cloud BatchNorm) x LOSS_PER_CLOUD x launch mode (eager, launch plan, HIP graph), and the size thresholds and
FC_LAYERS values that ROUTE a step between kernels (dgcnn/_engine.py, model.py, trainval.py).  Every kernel has its own module;
this one holds the routing: tests/mode_matrix_cells.py lists the cells (test_<cell>_...) and tests/test_mode_matrix_cells.py checks
on the host that every pair of values of two settings is run by one of them.

Three comparisons, all owned by older modules:
  (1) equality with the eager run under the deterministic kernels (test_gpu_graph.py: loss atol 1e-6, parameters <= 1e-6);
  (2) layer by layer, the float64 oracle fed the input the HIP layer really read (gpu_helpers.capture_layers / capture_convs;
      where a tensor exists only as operand planes it is decoded with gpu_helpers.planes_to_host), bar gpu_helpers.LAYER_ATOL;
  (3) an EdgeConv block against the oracle in the same mode on the same graph (gpu_helpers.BF16_BLOCK_*).
The shapes are small (R <= 1024): the module lowers E.PLANES_MIN_ROWS / E.SIDE_STREAM_MIN_ROWS where a cell needs the paths behind
them; the fixture below puts every engine global back.  Every twin / bar comparison records its measured error next to its bar
(written to $DGCNN_MODE_MATRIX_ERRORS when set; profiles/mode_matrix_errors.txt is a copy of one run)."""
import os

import numpy as np
import pytest
import torch

import dgcnn
from dgcnn import _engine as E, _hip as H, _planes as P
from oracle import dgcnn_oracle as O
import mode_matrix_cells as M
import packed_reference as PR
import seg_bn_bwd_reference as SB
from gpu_helpers import (BF16_BLOCK_GRAD_TOL, BF16_BLOCK_OUT_TOL, BF16_MODEL_GRAD_TOL, BF16_MODEL_LOSS_TOL, LAYER_ATOL, capture_convs,
                         capture_layers, dev, host, set_vars)

pytestmark = pytest.mark.gpu

B, N, C, K, NCLS = 4, 256, 3, 10, 3                # the dense tower: R = 1024 rows, four 64-row tiles per cloud
OFF = [0, 70, 120, 216]                            # the packed tower of the block tests: clouds of 70, 50 and 96 points
# bars of the modules that own them (each named where it is used)
PLANE_LOSS, PLANE_GRAD, PLANE_SOFTMAX = 1e-4, 1e-2, 1e-3      # test_gpu_head_planes.py
PACKED_LOGITS, PACKED_LOSS, PACKED_GRAD_ATOMICS = 1e-3, 1e-3, 2e-2   # test_gpu_packed_head.py / test_gpu_seg_bn_bwd.py (atomics mode)
REPLAY_LOSS, REPLAY_PARAM, REPLAY_INFER = 1e-6, 1e-6, 2e-4    # test_gpu_graph.py
# cell I (bf16 + planes + LOSS_PER_CLOUD + launch plan; atomics mode): four times the spread of EAGER runs of the same three
# micro-steps, measured on an MI355X as the worst pair among eight runs (profiles/mode_matrix_errors.txt): the spread is the
# atomics' noise, a wrong path is orders of magnitude larger.  The gradient's spread is the bf16 mode's: last-bit differences of the
# atomically summed BatchNorm-backward sums move a few dY across a bf16 rounding boundary (2^-9 of that element).  The losses
# came out bit-identical in all eight runs (fp64 atomics under an fp32 rounding, fixed-order per-cloud sums): their recorded spread
# is floored at the resolution of the number format, one float32 ulp at the loss's magnitude (1.2 .. 1.3: 2^-23).
I_EAGER_SPREAD = {"loss": 2.0 ** -23, "per-cloud loss": 2.0 ** -23, "gradient": 1.106e-4}
I_BAR = {n: 4 * v for n, v in I_EAGER_SPREAD.items()}

ERRORS = {}             # comparison -> [worst measured error, bar]


def note(name, err, bar, strict=False):
    """Print and record the measured error of a comparison, then assert it against its bar."""
    err = float(err)
    old = ERRORS.get(name)
    if old is None or err > old[0]:
        ERRORS[name] = [err, float(bar)]
    print("%-100s %.3e (bar %.1e)" % (name, err, bar))
    assert np.isfinite(err) and (err < bar if strict else err <= bar), "%s: %.3e over the bar %.1e" % (name, err, bar)


@pytest.fixture(scope="module", autouse=True)
def error_table():
    yield
    lines = ["# tests/test_gpu_mode_matrix.py: worst measured error of every twin / bar comparison, next to its bar",
             "%-100s %12s %10s" % ("comparison", "measured", "bar")]
    lines += ["%-100s %12.3e %10.1e" % (n, e, b) for n, (e, b) in sorted(ERRORS.items())]
    text = "\n".join(lines) + "\n"
    print("\n" + text)
    path = os.environ.get("DGCNN_MODE_MATRIX_ERRORS")
    if path:
        with open(path, "w") as f:
            f.write(text)


@pytest.fixture(autouse=True)
def engine_state():
    """Every engine global a cell may move, put back whatever the cell did; a fresh context before and after."""
    names = ("PLANES_MIN_ROWS", "SIDE_STREAM_MIN_ROWS", "WGRAD_SIDE_STREAM", "DROPOUT_KEEP", "BF16_FUSED_BWD")
    saved = {n: getattr(E, n) for n in names}
    gemm, prepared, call, drop = P.gemm, E.prepared, H.call, E.dropout
    dgcnn.reset()
    try:
        yield
    finally:
        for n, v in saved.items():
            setattr(E, n, v)
        P.gemm, E.prepared, H.call, E.dropout = gemm, prepared, call, drop
        E.HEAD_PLANES, E.DETERMINISTIC, E.EDGE_MLP_DTYPE = E.HEAD_PLANES_ENV_DEFAULT, E.DETERMINISTIC_ENV_DEFAULT, "f32"
        dgcnn.reset()


class spies(object):
    """Counts the plane GEMMs (P.gemm: their forms, in issue order), the weights E.prepared was asked for ((kind, served from
    c.wprep?)) and the names of every H.call while active.  forbid_planes: a plane GEMM raises instead of running."""

    def __init__(self, forbid_planes=False):
        self.gemms, self.served, self.calls, self.forbid = [], [], [], forbid_planes

    def __enter__(self):
        self._g, self._p, self._c = P.gemm, E.prepared, H.call

        def gemm(form, A, Bm, Cm, **kw):
            self.gemms.append(form)
            if self.forbid:
                raise AssertionError("a plane GEMM (form %d, C %s) was issued where the fp32-class GEMMs must run" % (form, tuple(Cm.shape)))
            return self._g(form, A, Bm, Cm, **kw)

        def prepared(key):
            v = self._p(key)
            self.served.append((key[0], v is not None))
            return v

        def call(name, *a, **kw):
            self.calls.append(name)
            return self._c(name, *a, **kw)
        P.gemm, E.prepared, H.call = gemm, prepared, call
        return self

    def __exit__(self, *exc):
        P.gemm, E.prepared, H.call = self._g, self._p, self._c
        return False

    def kinds(self, kind):
        return [ok for k, ok in self.served if k == kind]


def fro(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def f64(params):
    return {n: np.asarray(v, np.float64) for n, v in params.items()}


def random_params(flags, seed, beta_seed=8):
    rng = np.random.default_rng(beta_seed)
    params = O.init_params(flags, int(flags.NUM_CHANNEL), seed=seed)
    for n in params:
        if n.endswith("beta"):
            params[n] = rng.normal(0, 0.2, params[n].shape).astype(np.float32)
    return params


def head_flags(train, fcl=2, model="dgcnn", **kw):
    """The smallest plane-eligible model: Cin = 128 into MergedEdgeConv, ctot = 1408 into FC0, FC widths 128."""
    base = dict(MODEL_NAME=model, EDGE_CONV_LAYERS=2, EDGE_CONV_FILTERS=[64, 64], FC_LAYERS=fcl, FC_FILTERS=[128] * fcl, NUM_CLASS=NCLS,
                KVALUE=K, NUM_CHANNEL=C, TRAIN=train, SEED=3, HEAD_PLANES="f16")
    base.update(kw)
    return dgcnn.DGCNN_FLAGS(**base)


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(21)
    pts = rng.random((B, N, C), dtype=np.float32)
    labels = rng.integers(0, NCLS, (B, N)).astype(np.int32)
    return pts, labels


def packed_tower(sizes, Cc, seed):
    rng = np.random.default_rng(seed)
    pts = np.concatenate([rng.random((n, Cc), dtype=np.float32) for n in sizes])
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return pts, off, rng.integers(0, NCLS, len(pts)).astype(np.int32)


def packed_graphs(layers, L, off, k):
    """The captured graphs of a packed tower, each bit for bit the oracle's k-NN of the layer's own input, cloud by cloud."""
    out = []
    for i in range(L):
        xin, idx = layers["EdgeConv%d" % i]
        assert idx.shape == (1, off[-1], k)
        flat = idx.reshape(-1, k)
        for b in range(len(off) - 1):
            lo, hi = int(off[b]), int(off[b + 1])
            np.testing.assert_array_equal(flat[lo:hi] - lo, O.k_nn(xin[0, lo:hi][None], k)[0], err_msg="layer %d cloud %d" % (i, b))
        out.append(idx)
    return out


# ------------------------------------------------------------------------------------------
# comparison (2) on the head, and the whole plane-mode step (cells A, B, G)
# ------------------------------------------------------------------------------------------
def check_head_layers(calls, params, flags, Bc, Nc, tag, planes):
    """Every head layer against the float64 oracle on the input it read: MergedEdgeConv (and the per-cloud maximum returned with
    it), FC0 on [tile(g) | its input] with the whole weight (model.py splits it; the oracle does not), FC1.., Final."""
    fcl = int(flags.FC_LAYERS)
    p64 = f64(params)
    g = None
    for n in ["MergedEdgeConv"] + ["FC%d" % i for i in range(fcl)] + ["Final"]:
        rec = calls[n]
        x = rec["x"]
        if n == "FC0":
            x = np.concatenate([np.repeat(g, Nc, axis=0), x], axis=1)
        ref, _ = O.conv_bn_act(x, p64[n + "/weights"], p64[n + "/BatchNorm/beta"], relu=True)
        assert rec["out"].shape == ref.shape, (n, rec["out"].shape, ref.shape)
        note("%s: %s output on its own input" % (tag, n), np.abs(rec["out"] - ref).max(), LAYER_ATOL)
        if rec["g"] is not None:
            g = rec["g"]
            note("%s: %s per-cloud maximum" % (tag, n), np.abs(g - ref.reshape(Bc, Nc, -1).max(1)).max(), LAYER_ATOL)
    assert g is not None
    if planes:       # where the tensors lived: MergedEdgeConv -> planes only -> FC0 (-> planes only -> FC1 when there is one)
        assert calls["MergedEdgeConv"]["planes_out"] and calls["FC0"]["planes_in"]
        assert calls["FC0"]["planes_out"] == (fcl >= 2)
        if fcl >= 2:
            assert calls["FC1"]["planes_in"] and not calls["FC1"]["planes_out"]
    else:
        assert not any(r["planes_in"] or r["planes_out"] for r in calls.values())


def plane_step(tv, flags, params, pts, lab, train, side, tag):
    """One inference / training step of `tv` in plane mode: the products ran on the plane GEMM (and in what order), the weight planes
    came from the side stream's preparation exactly when it is on, every head layer by comparison (2), and the softmax (inference) or
    the loss and every gradient (training) against the float64 twin fed the same graphs at the plane mode's own bars."""
    fcl, L = int(flags.FC_LAYERS), int(flags.EDGE_CONV_LAYERS)
    nl = fcl + 1                                   # plane layers: MergedEdgeConv, FC0 .. FC<fcl-1>
    nprep = min(nl, 3) if side else 0              # model.build prepares MergedEdgeConv, FC0 and FC1 ahead
    Bc, Nc = pts.shape[:2]
    with spies() as spy, capture_layers() as capl, capture_convs() as capc:
        if train:
            tv.zero_gradients(None)
            res = tv.accum_gradient(None, [pts], [lab])
        else:
            res = tv.inference(None, [pts], [lab])
        torch.cuda.synchronize()
    assert E.HEAD_PLANES == P.F16X2 and not E.DETERMINISTIC
    assert spy.gemms == [P.KC] * nl + ([P.KC, P.TR] * nl if train else []), spy.gemms
    assert spy.kinds("wT") == [True] * nprep + [False] * (nl - nprep), spy.served
    assert spy.kinds("w") == ([False] * (nl - nprep) + [True] * nprep if train else []), spy.served
    assert spy.kinds("wcat") == [side] * L, spy.served
    assert (E.ctx().side is not None) == side
    check_head_layers(capc.calls, params, flags, Bc, Nc, tag, planes=True)
    idx_list = [capl.layers["EdgeConv%d" % i][1] for i in range(L)]
    for i in range(L):
        np.testing.assert_array_equal(idx_list[i], O.k_nn(capl.layers["EdgeConv%d" % i][0], K), err_msg="layer %d" % i)
    p64 = f64(params)
    if train:
        G64, loss64, _, _ = O.train_step_grads(pts.astype(np.float64), lab, flags, p64, idx_list=idx_list)
        note("%s: loss vs float64 twin" % tag, abs(float(res[2]) - float(loss64)), PLANE_LOSS, strict=True)
        rel = {n: fro(host(tv.gradients[n]).astype(np.float64), G64[n]) for n in params}
        worst = max(rel, key=rel.get)
        note("%s: worst gradient vs float64 twin, rel. Frobenius (%s)" % (tag, worst.split("/")[0]), rel[worst], PLANE_GRAD, strict=True)
    else:
        ref, _ = O.model_forward(pts.astype(np.float64), flags, p64, idx_list=idx_list)
        e = np.exp(ref - ref.max(-1, keepdims=True))
        note("%s: softmax vs float64 twin" % tag, np.abs(host(res[0]) - e / e.sum(-1, keepdims=True)).max(), PLANE_SOFTMAX)
    return spy


def dropout_is_the_separate_pass(flags, params, pts, lab, tag):
    """Plane mode with the dropout behind a plane layer (FC_LAYERS 1 and 3): the layer's BatchNorm output is what the oracle computes
    on the layer's input, and the tensor the layer hands on is dgcnn_dropout_dev_f32 of it under the step's seed, bit for bit --
    not the fused BatchNorm + dropout pass, which the plane route does not take."""
    fcl = int(flags.FC_LAYERS)
    last = "FC%d" % (fcl - 1)
    seen = []
    orig = E.dropout

    def drop(x, keep=E.DROPOUT_KEEP):
        out = orig(x, keep)
        seen.append((x, out, keep))
        return out
    E.dropout = drop
    try:
        tv = dgcnn.trainval(flags).initialize()
        set_vars(dgcnn, params)
        tv.zero_gradients(None)
        with spies() as spy, capture_convs() as capc:
            tv.accum_gradient(None, [pts], [lab])
            torch.cuda.synchronize()
    finally:
        E.dropout = orig
    assert len(seen) == 1 and seen[0][2] == 0.7 and "dgcnn_bn1_act_dropout_f32" not in spy.calls
    x, out, keep = seen[0]
    again = torch.empty_like(x)
    H.call("dgcnn_dropout_dev_f32", x.data_ptr(), again.data_ptr(), x.numel(), float(keep), E.ctx().seed_dev.data_ptr())
    np.testing.assert_array_equal(host(out), host(again))
    np.testing.assert_array_equal(capc.calls[last]["out"], host(out).astype(np.float64))        # ... and it is what the layer returned
    xin = capc.calls[last]["x"]
    if last == "FC0":
        xin = np.concatenate([np.repeat(capc.calls["MergedEdgeConv"]["g"], pts.shape[1], axis=0), xin], axis=1)
    p64 = f64(params)
    ref, _ = O.conv_bn_act(xin, p64[last + "/weights"], p64[last + "/BatchNorm/beta"], relu=True)
    note("%s: %s BatchNorm output in front of the dropout" % (tag, last), np.abs(host(x) - ref).max(), LAYER_ATOL)
    h = host(out)
    dropped = float(((h == 0) & (host(x) != 0)).mean() / max((host(x) != 0).mean(), 1e-9))
    assert 0.25 <= dropped <= 0.35, dropped                       # keep = 0.7 over 131072 elements
    kept = (h != 0)
    np.testing.assert_allclose(h[kept], (host(x) / np.float32(0.7))[kept], rtol=4e-7, atol=0)     # (x / keep or x * (1 / keep): two roundings)


HEAD_CASES = [("dgcnn", 2, True), ("dgcnn", 1, False), ("dgcnn", 2, False), ("dgcnn", 3, False), ("residual-dgcnn", 2, False),
              ("dgcnn", 3, True)]


def _head_case(case, model, fcl, side):
    pts, lab = case
    E.PLANES_MIN_ROWS = 0
    if side:
        E.SIDE_STREAM_MIN_ROWS = 0
    E.DROPOUT_KEEP = 1.0
    tag = "%s fc%d %s" % (model, fcl, "side-stream" if side else "one-stream")
    for train in (False, True):
        flags = head_flags(train, fcl, model)
        params = random_params(flags, seed=4)
        tv = dgcnn.trainval(flags).initialize()
        set_vars(dgcnn, params)
        plane_step(tv, flags, params, pts, lab, train, side, tag + (" train" if train else " infer"))
    if fcl in (1, 3):
        E.DROPOUT_KEEP = 0.7
        dropout_is_the_separate_pass(flags, params, pts, lab, tag)


@pytest.mark.parametrize("model,fcl,side", [c for c in HEAD_CASES if c[2]], ids=lambda v: str(v))
def test_A_plane_mode_with_the_weight_planes_from_the_side_stream(case, model, fcl, side):
    """SIDE_STREAM_MIN_ROWS = 0: model.build issues prepare_step_weights, so the head's weight planes in both orientations (keys
    ("wT", ptr) / ("w", ptr)) and conv0's folded weights come out of c.wprep behind the prepared() wait -- the path every
    bench-size plane run takes and no test ran.  Inference and one training step: 3 and 9 plane products (FC_LAYERS = 3: FC2's
    weight is not prepared ahead and is split in line), every head layer by comparison (2), softmax / loss / gradients against
    the twin at the plane bars."""
    _head_case(case, model, fcl, side)


@pytest.mark.parametrize("model,fcl,side", [c for c in HEAD_CASES if not c[2]], ids=lambda v: str(v))
def test_B_plane_mode_at_every_fc_depth_and_on_the_residual_stack(case, model, fcl, side):
    """FC_LAYERS = 1: FC0 takes model.build's non-plane branch, reads `big` (whose MergedEdgeConv slice exists only as planes)
    through c.planes_of and still runs on P.gemm -- 2 / 6 products; FC_LAYERS = 3: FC2 splits FC1's fp32 output itself -- 4 / 12;
    residual-dgcnn: one training step.  Same checks as cell A; FC_LAYERS 1 and 3 carry the dropout behind a plane layer.
    Measured: the residual step's gradients from MergedEdgeConv down lie 1.2e-3 .. 3.2e-3 from the twin where the plain stack's
    lie 4e-6 (with the planes off: 1.2e-4 from FC0 down), every layer's OUTPUT within 2e-5 in both -- the size one near-tie of the
    max-pool or one ReLU boundary decided the other way would give; not traced to its element."""
    _head_case(case, model, fcl, side)


# ------------------------------------------------------------------------------------------
# C. plane mode replayed
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,side", [("plan", False), ("plan", True), (True, False)], ids=["launch-plan", "launch-plan-side-stream", "hip-graph"])
def test_C_plane_mode_replay_reissues_scales_and_weight_planes(case, capfd, mode, side):
    """Plane-mode inference under a launch plan / HIP graph: one captured entry, no capture failure, the recording issues the three
    plane products and a replay none from Python.  Then the parameters change UNDER the recording and the replay must give what an
    eager step gives on the new values: at 8x their values, and at another draw (a frozen weight PLANE, which BatchNorm's scale
    invariance hides at any multiple).  The 8x step alone does not catch a frozen SCALE: the weight planes' power-of-two scale
    follows the largest parameter of the bucket, here a BatchNorm beta 11x above the head's largest weight, so a stale scale
    still holds 8x weights without saturating fp16 (measured: a recording that skips dgcnn_param_scales_f32 passed it).  So the
    step's scales buffer (c.pl_scales, one device buffer for all steps) is also set to 2^40 before every replay: a recording that
    re-issues dgcnn_param_scales_f32 overwrites that, one that does not splits its operands into infinities."""
    pts, lab = case
    E.PLANES_MIN_ROWS = 0
    if side:
        E.SIDE_STREAM_MIN_ROWS = 0
    flags = head_flags(False)
    params = random_params(flags, seed=4)
    tv = dgcnn.trainval(flags).initialize().use_graph(mode)
    set_vars(dgcnn, params)
    x, y = dev(pts), dev(lab)
    counts = []
    with spies() as spy:
        for _ in range(3):                                          # eager sighting, recording, replay
            tv.inference(None, [x], [y])
            counts.append(len(spy.gemms))
        assert counts == [3, 6, 6] and spy.gemms == [P.KC] * 6, (counts, spy.gemms)
        assert len(tv._graphs) == 1
        assert spy.kinds("wT") == [side] * 6
        p8 = {n: 8.0 * v for n, v in params.items()}
        other = random_params(flags, seed=9, beta_seed=10)
        tag = "plane mode, %s%s" % ("launch plan" if mode == "plan" else "HIP graph", " + side stream" if side else "")
        first = None
        for what, new in (("same", params), ("8x", p8), ("new draw", other)):
            set_vars(dgcnn, new)
            issued = len(spy.gemms)
            dgcnn.ctx().pl_scales.fill_(2.0 ** 40)                    # (stream ordered, in front of the replay)
            got = [o.clone() for o in tv.inference(None, [x], [y])]
            assert len(spy.gemms) == issued and len(tv._graphs) == 1     # a replay: nothing issued from Python
            tv.use_graph(False)
            want = tv.inference(None, [x], [y])
            tv.use_graph(mode)
            assert bool(torch.isfinite(want[0]).all())
            if first is None:
                first = want[0].clone()
            else:                                                    # the new values ARE another model: a replay deaf to them would show
                assert float((want[0] - first).abs().max()) > 1e-2
            note("%s: replayed softmax vs eager, parameters %s" % (tag, what), float((got[0] - want[0]).abs().max()), REPLAY_INFER)
            note("%s: replayed loss vs eager, parameters %s" % (tag, what), abs(float(got[-1]) - float(want[-1])), REPLAY_INFER, strict=True)
    assert "capture failed" not in capfd.readouterr().err


# ------------------------------------------------------------------------------------------
# D. bf16 mode replayed;  H. packed towers between replays  -- comparison (1)
# ------------------------------------------------------------------------------------------
def train_flags(**kw):
    base = dict(EDGE_CONV_LAYERS=2, EDGE_CONV_FILTERS=[64, 64], KVALUE=K, FC_LAYERS=2, FC_FILTERS=[128, 64], NUM_CLASS=2, NUM_CHANNEL=3,
                TRAIN=True, SEED=11, LEARNING_RATE=1e-3, DETERMINISTIC=True)
    base.update(kw)
    return dgcnn.DGCNN_FLAGS(**base)


def assert_equals_the_eager_run(tag, loss_g, p_g, loss_e, p_e, p_init):
    note("%s: losses vs the eager run" % tag, np.abs(np.asarray(loss_g) - np.asarray(loss_e)).max(), REPLAY_LOSS)
    note("%s: parameters vs the eager run" % tag, np.abs(p_g - p_e).max(), REPLAY_PARAM)
    assert np.abs(p_e - p_init).max() > 1e-3                        # it trained


@pytest.mark.parametrize("mode", ["plan", True], ids=["launch-plan", "hip-graph"])
def test_D_bf16_mode_replay_retraces_the_eager_training_run(capfd, mode):
    """EDGE_MLP_DTYPE = 'bf16' (fused forward and backward: k = 10), deterministic kernels, dropout on: three updates of two
    micro-steps replayed from one recording equal the eager run."""
    rng = np.random.default_rng(0)
    pts = torch.from_numpy(rng.random((3, B, N, 3), dtype=np.float32)).cuda()
    lab = torch.from_numpy(rng.integers(0, 2, (3, B, N)).astype(np.int32)).cuda()
    flags = train_flags(EDGE_MLP_DTYPE="bf16")

    def train(graph):
        tv = dgcnn.trainval(flags).initialize().use_graph(graph)
        p0 = host(dgcnn.ctx().flat_param).copy()
        losses = []
        with spies() as spy:
            for s in range(3):
                tv.zero_gradients(None)
                for _ in range(2):
                    losses.append(float(tv.accum_gradient(None, [pts[s]], [lab[s]])[2]))
                tv.apply_gradient(None)
        assert E.EDGE_MLP_DTYPE == "bf16" and E.DETERMINISTIC
        assert "dgcnn_edge_mlp_bf16_stats" in spy.calls and "dgcnn_edge_mlp_bf16_bwd" in spy.calls
        return tv, losses, host(dgcnn.ctx().flat_param).copy(), p0
    tv_e, loss_e, p_e, p0 = train(False)
    tv_g, loss_g, p_g, _ = train(mode)
    assert len(tv_g._graphs) == 1 and not tv_e._graphs
    assert_equals_the_eager_run("bf16 mode, %s" % ("launch plan" if mode == "plan" else "HIP graph"), loss_g, p_g, loss_e, p_e, p0)
    assert "capture failed" not in capfd.readouterr().err


@pytest.mark.parametrize("tower,lpc,launch", M.H_RUNS, ids=["%s-%s-%s" % (t, "lpc" if l else "mean", m) for t, l, m in M.H_RUNS])
def test_H_packed_steps_between_replays_of_a_dense_shape(capfd, tower, lpc, launch):
    """use_graph('plan') / use_graph(True), deterministic kernels, dropout on: dense, dense (recorded), PACKED, dense (replayed),
    PACKED, dense (replayed), an Adam update after each.  The packed towers (1024 rows against the dense tower's 384: the arena
    extent and stat_off move under the recording) run eagerly -- nothing is recorded for them -- and every loss and the final
    parameters equal those of the all-eager sequence.  packed-bpc: BN_PER_CLOUD_TRAIN (the dense tower is one cloud: B > 1 would
    itself run as a packed tower).  LOSS_PER_CLOUD: the eager sequence's reported loss is the mean of its per-cloud losses."""
    bpc = tower == "packed-bpc"
    mode = "plan" if launch == "plan" else True
    flags = train_flags(BN_PER_CLOUD_TRAIN=bpc, LOSS_PER_CLOUD=lpc)
    rng = np.random.default_rng(7)
    dshape = (1, 384) if bpc else (2, 192)
    dpts = torch.from_numpy(rng.random((6,) + dshape + (3,), dtype=np.float32)).cuda()
    dlab = torch.from_numpy(rng.integers(0, 2, (6,) + dshape).astype(np.int32)).cuda()
    sizes = [300, 212, 512]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    ppts = torch.from_numpy(rng.random((6, 1024, 3), dtype=np.float32)).cuda()
    plab = torch.from_numpy(rng.integers(0, 2, (6, 1024)).astype(np.int32)).cuda()
    seq = "ddpdpd"

    def train(graph):
        tv = dgcnn.trainval(flags).initialize().use_graph(graph)
        p0 = host(dgcnn.ctx().flat_param).copy()
        losses = []
        for i, s in enumerate(seq):
            tv.zero_gradients(None)
            if s == "d":
                res = tv.accum_gradient(None, [dpts[i]], [dlab[i]])
            else:
                res = tv.accum_gradient(None, [ppts[i]], [plab[i]], offsets=[off])
            losses.append(float(res[2]))
            if lpc:
                per = tv.per_cloud_scalars()
                assert len(per) == 1 and tuple(per[0].shape) == ((3 if s == "p" else dshape[0]), 2)
                if not graph:
                    assert abs(float(host(per[0])[:, 0].astype(np.float64).mean()) - losses[-1]) <= 1e-6
            tv.apply_gradient(None)
            if graph:                                               # only the dense shape is ever recorded, at its second sighting
                assert len(tv._graphs) == (0 if i == 0 else 1)
                assert all(k[1] == dshape + (3,) for k in tv._graphs)
        return tv, losses, host(dgcnn.ctx().flat_param).copy(), p0
    tv_e, loss_e, p_e, p0 = train(False)
    tv_g, loss_g, p_g, _ = train(mode)
    assert not tv_e._graphs and E.DETERMINISTIC
    assert len({round(l, 6) for l in loss_e}) == 6
    assert_equals_the_eager_run("%s tower%s between replays, %s" % (tower, " + LOSS_PER_CLOUD" if lpc else "", launch), loss_g, p_g, loss_e, p_e, p0)
    assert "capture failed" not in capfd.readouterr().err


# ------------------------------------------------------------------------------------------
# E. bf16 block with the side stream;  F. bf16 on a packed tower  -- comparison (3)
# ------------------------------------------------------------------------------------------
def block_params(rng, Cc, F):
    return {"conv0/weights": rng.normal(0, 0.5, (2 * Cc, F)).astype(np.float32),
            "conv0/BatchNorm/beta": rng.normal(0, 0.3, F).astype(np.float32),
            "conv1/weights": rng.normal(0, 0.3, (2 * F, 64)).astype(np.float32),
            "conv1/BatchNorm/beta": rng.normal(0, 0.3, 64).astype(np.float32)}


def run_block(pts2d, Bc, Nc, k, F, Pm, want_dx, d=None, offsets=None, seed=0):
    """One recorded edge_conv block on a fresh context + its backward with random upstream gradients `d`.
    -> (outs on the host, idx, {gradients}, d, names of the forward's calls, names of the backward's calls, context)."""
    dgcnn.reset()
    c = dgcnn.ctx()
    c.begin_step()
    c.recording = True
    R, Cc = pts2d.shape
    x = c.new_buffer(R, Cc) if want_dx else torch.empty((R, Cc), dtype=torch.float32, device="cuda")
    x.copy_(dev(pts2d))
    for n, v in Pm.items():
        c.get_variable(n, v.shape)
    set_vars(dgcnn, Pm)
    with spies() as spy:
        if offsets is None:
            outs = dgcnn.ops.edge_conv(x.view(Bc, Nc, Cc), k, F, True)
        else:
            outs = dgcnn.ops.edge_conv(x, k, F, True, offsets=offsets)
        nfwd = len(spy.calls)
        idx = host(dgcnn.ops.edge_conv.last_idx)
        if d is None:
            rng = np.random.default_rng(seed)
            d = [rng.normal(size=tuple(o.shape)).astype(np.float32) for o in outs]
        for t, g in zip(outs, d):
            v, _, _ = E.as2d(t)
            c.grad(v).copy_(dev(g.reshape(R, -1)))
        c.backward()
        torch.cuda.synchronize()
    grads = {n: host(c.var_grads[n]).copy() for n in Pm}
    if want_dx:
        grads["dx"] = host(c.grad(x)).copy()
    return [host(o).copy() for o in outs], idx, grads, d, spy.calls[:nfwd], spy.calls[nfwd:], c


@pytest.mark.parametrize("k", [10, 5], ids=["k10-fused-backward", "k5-dense-backward"])
def test_E_bf16_block_with_the_side_stream_is_bit_identical(k):
    """bf16 mode, deterministic kernels, d(X) wanted, SIDE_STREAM_MIN_ROWS = 0: with the side stream on (conv1's weight-gradient GEMM
    runs there) the block gives bit for bit what it gives with WGRAD_SIDE_STREAM off, with the one-pass backward (k = 10) and
    without it (k = 5).  In bf16 mode the transposed adjacency is never pre-built during the forward (csr stays None: that
    branch belongs to the fp32 fold): it is built in the backward, on the main stream -- asserted here."""
    Bc, Nc, Cc, F = 2, 128, 64, 64
    rng = np.random.default_rng(5)
    pts = rng.random((Bc * Nc, Cc), dtype=np.float32)
    Pm = block_params(rng, Cc, F)
    E.SIDE_STREAM_MIN_ROWS = 0
    res = {}
    d = None
    for side in (False, True):
        E.WGRAD_SIDE_STREAM = side
        E.EDGE_MLP_DTYPE, E.DETERMINISTIC = "bf16", True
        outs, idx, grads, d, fwd, bwd, c = run_block(pts, Bc, Nc, k, F, Pm, True, d=d)
        assert (c.side is not None) == side                          # the side stream was really engaged
        assert ("dgcnn_edge_mlp_bf16_bwd" in bwd) == (k == 10) and "dgcnn_edge_mlp_bf16_stats" in fwd
        assert "dgcnn_edge_csr_build" not in fwd and bwd.count("dgcnn_edge_csr_build") == 1
        res[side] = (outs, grads)
    for a, b in zip(res[True][0], res[False][0]):
        np.testing.assert_array_equal(a, b)
    for n in res[False][1]:
        np.testing.assert_array_equal(res[True][1][n], res[False][1][n], err_msg=n)
        assert np.abs(res[False][1][n]).sum() > 0, n


# (C, F, k, DETERMINISTIC): fused forward + backward; fused forward, dense backward (k < 8); conv0 width off the GEMM's rounding
# path (the engine rounds E and W0 itself; F % 4: atomics mode); and the smallest width ON the rounding path with a shape the
# fused kernels do not take -- the one product whose `arith=1` alone makes it the mode's arithmetic
PACKED_BLOCKS = [(64, 64, 8, True), (3, 32, 5, True), (4, 6, 7, False), (4, 12, 7, True)]


@pytest.mark.parametrize("Cc,F,k,det", PACKED_BLOCKS, ids=["C%d-F%d-k%d" % c[:3] for c in PACKED_BLOCKS])
def test_F_bf16_block_on_a_packed_tower(Cc, F, k, det):
    """ops.edge_conv(..., offsets=[0, 70, 120, 216]) in bf16 mode, whole-tower BatchNorm: the graph is the oracle's k-NN of every
    cloud alone, bit for bit; outputs and gradients against the oracle in bf16 mode on the (1, R) tower with tower-row indices at
    the bars of test_gpu_bf16_edge_mlp.py::test_edge_conv_bf16_forward_backward."""
    rng = np.random.default_rng(Cc * 10 + F)
    R = OFF[-1]
    pts = rng.random((R, Cc), dtype=np.float32)
    Pm = block_params(rng, Cc, F)
    want_dx = Cc % 4 == 0 and F % 4 == 0
    E.EDGE_MLP_DTYPE, E.DETERMINISTIC = "bf16", det
    outs, idx, grads, d, fwd, bwd, c = run_block(pts, 1, R, k, F, Pm, want_dx, offsets=OFF, seed=F)
    fused = bool(H.load().dgcnn_edge_mlp_bf16_supported(Cc, k, F))
    assert fused == ((Cc, F, k) in ((64, 64, 8), (3, 32, 5)))
    assert ("dgcnn_edge_mlp_bf16_stats" in fwd) == fused and ("dgcnn_edge_mlp_bf16_bwd" in bwd) == ((Cc, F, k) == (64, 64, 8))
    assert ("dgcnn_round_bf16_f32" in fwd) == (F == 6)               # off the rounding path: the engine rounds the operands
    assert idx.shape == (1, R, k)
    for b in range(3):
        lo, hi = OFF[b], OFF[b + 1]
        np.testing.assert_array_equal(idx[0, lo:hi] - lo, O.k_nn(pts[None, lo:hi], k)[0], err_msg="cloud %d" % b)
    P64 = [Pm[n].astype(np.float64) for n in Pm]
    ref, cache = O.edge_conv(pts[None].astype(np.float64), k, *P64, idx=idx, edge_mlp_dtype="bf16")
    plain, _ = O.edge_conv(pts[None].astype(np.float64), k, *P64, idx=idx)
    tag = "packed bf16 block C%d F%d k%d" % (Cc, F, k)
    for name, a, r in zip(("max", "mean", "net"), outs, ref):
        note("%s: %s vs oracle (bf16 mode), units of the bar" % (tag, name),
             (np.abs(a - r) / (BF16_BLOCK_OUT_TOL + BF16_BLOCK_OUT_TOL * np.abs(r))).max(), 1.0)
    assert np.abs(ref[0] - plain[0]).max() > 1e-4                   # the mode IS different arithmetic
    dx_ref, g_ref = O.edge_conv_bwd(d[0].astype(np.float64), d[1].astype(np.float64), d[2].astype(np.float64), cache)
    pairs = [(n, grads[n], g_ref[key]) for n, key in (("conv0/weights", "W0"), ("conv0/BatchNorm/beta", "beta0"), ("conv1/weights", "W1"),
                                                      ("conv1/BatchNorm/beta", "beta1"))]
    if want_dx:
        pairs.append(("dx", grads["dx"].reshape(1, R, Cc), dx_ref))
    for n, got, want in pairs:
        atol = BF16_BLOCK_GRAD_TOL * max(1.0, float(np.abs(want).max()))
        note("%s: d(%s) vs oracle (bf16 mode), units of the bar" % (tag, n), (np.abs(got - want) / (atol + BF16_BLOCK_GRAD_TOL * np.abs(want))).max(), 1.0)


def test_F_bf16_model_step_on_a_packed_tower():
    """One packed training step in bf16 mode (layer 0: C = 4, F = 48, the unfused product on the GEMM's rounding path; layer 1:
    C = 64, F = 64, the fused kernels) against tests/packed_reference.py in bf16 mode on the step's own per-cloud graphs, at the
    bars of test_gpu_bf16_edge_mlp.py::test_model_gradients_bf16_small."""
    kw = dict(MODEL_NAME="dgcnn", EDGE_CONV_LAYERS=2, EDGE_CONV_FILTERS=[48, 64], FC_LAYERS=2, FC_FILTERS=[128, 64], NUM_CLASS=NCLS, KVALUE=8,
              NUM_CHANNEL=4, TRAIN=True)
    flags, plain = dgcnn.DGCNN_FLAGS(EDGE_MLP_DTYPE="bf16", **kw), dgcnn.DGCNN_FLAGS(EDGE_MLP_DTYPE="f32", **kw)
    pts, off, lab = packed_tower([70, 50, 96], 4, seed=5)
    params = O.init_params(flags, 4, seed=2)
    E.DROPOUT_KEEP = 1.0
    tv = dgcnn.trainval(flags).initialize()
    set_vars(dgcnn, params)
    tv.zero_gradients(None)
    with capture_layers() as cap, spies() as spy:
        res = tv.accum_gradient(None, [pts], [lab], offsets=[off])
        torch.cuda.synchronize()
    assert E.EDGE_MLP_DTYPE == "bf16" and E.DETERMINISTIC == E.DETERMINISTIC_ENV_DEFAULT
    assert spy.calls.count("dgcnn_edge_mlp_bf16_stats") == 1 and spy.calls.count("dgcnn_edge_gather_f32") >= 1      # one layer each way
    graphs = packed_graphs(cap.layers, 2, off, 8)
    G, loss64, _, _ = PR.train_step_grads(pts.astype(np.float64), lab, off, flags, f64(params), graphs)
    _, loss_f32, _, _ = PR.train_step_grads(pts.astype(np.float64), lab, off, plain, f64(params), graphs)
    print("packed bf16 model step: loss %.7f, reference in bf16 mode %.7f, with fp32 operands %.7f" % (float(res[2]), loss64, loss_f32))
    note("packed bf16 model step: loss vs packed reference (bf16 mode)", abs(float(res[2]) - float(loss64)), BF16_MODEL_LOSS_TOL, strict=True)
    rel = {n: fro(host(tv.gradients[n]).astype(np.float64), G[n]) for n in params}
    worst = max(rel, key=rel.get)
    note("packed bf16 model step: worst gradient, rel. Frobenius (%s)" % worst.split("/")[0], rel[worst], BF16_MODEL_GRAD_TOL, strict=True)


# ------------------------------------------------------------------------------------------
# G. planes asked for on a packed tower
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bpc", [False, True], ids=["packed", "packed-bpc"])
def test_G_a_packed_tower_runs_no_plane_gemm_and_leaks_nothing_into_the_next_dense_step(case, bpc):
    """HEAD_PLANES = 'f16' with PLANES_MIN_ROWS = 0 on a packed tower (and on one with BN_PER_CLOUD_TRAIN): "the plane mode is NOT
    packed" -- P.gemm is never called (here it would raise), and logits, loss and gradients stay within the packed bars of
    test_gpu_packed_head.py / test_gpu_seg_bn_bwd.py (atomics mode: planes asked for).  A dense step of the SAME trainval afterwards
    runs its nine products on the plane GEMM again and passes cell A's checks: nothing of c.planes / pl_scales_ready leaked.
    (BN_PER_CLOUD_TRAIN: the dense tower is one cloud of 1024 points -- with B > 1 it would itself run as a packed tower.)"""
    E.PLANES_MIN_ROWS = 0
    E.DROPOUT_KEEP = 1.0
    flags = head_flags(True, BN_PER_CLOUD_TRAIN=bpc)
    params = random_params(flags, seed=4)
    pts, off, lab = packed_tower([70, 50, 96], C, seed=3)
    R = len(pts)
    p64 = f64(params)
    tag = "planes asked on a %s tower" % ("packed-bpc" if bpc else "packed")
    tv = dgcnn.trainval(flags).initialize()
    set_vars(dgcnn, params)
    assert E.HEAD_PLANES == P.F16X2 and not E.DETERMINISTIC
    assert E.planes_ok(R, 128, 1024) and E.planes_ok(R, 1408, 128)            # a dense tower of these sizes WOULD take the planes
    with spies(forbid_planes=True) as spy:
        if not bpc:
            fi = head_flags(False)
            with capture_layers() as cap:
                logits = host(dgcnn.build(dev(pts), fi, offsets=off))
            ref, _ = PR.model_forward(pts.astype(np.float64), off, fi, p64, packed_graphs(cap.layers, 2, off, K))
            note("%s: logits vs packed reference" % tag, np.abs(logits - ref).max(), PACKED_LOGITS)
        tv.zero_gradients(None)
        with capture_layers() as cap, capture_convs() as capc:
            res = tv.accum_gradient(None, [pts], [lab], offsets=[off])
            torch.cuda.synchronize()
        assert spy.gemms == [] and "dgcnn_gemm_planes_f32" not in spy.calls and "dgcnn_split_planes_f32" not in spy.calls
        assert "dgcnn_param_scales_f32" not in spy.calls
    assert not any(r["planes_in"] or r["planes_out"] for r in capc.calls.values()) and not E.ctx().planes
    graphs = packed_graphs(cap.layers, 2, off, K)
    if bpc:
        G, loss64 = SB.train_step_grads(pts, lab, off, flags, params, graphs, np.ones(R))
    else:
        G, loss64, _, _ = PR.train_step_grads(pts.astype(np.float64), lab, off, flags, p64, graphs)
    note("%s: loss vs packed reference" % tag, abs(float(res[2]) - float(loss64)), PACKED_LOSS, strict=True)
    rel = {n: fro(host(tv.gradients[n]).astype(np.float64), G[n]) for n in params}
    worst = max(rel, key=rel.get)
    note("%s: worst gradient, rel. Frobenius (%s)" % (tag, worst.split("/")[0]), rel[worst], PACKED_GRAD_ATOMICS)
    # the same trainval, a dense tower: the plane GEMMs are back
    dpts, dlab = case
    if bpc:
        dpts, dlab = dpts.reshape(1, B * N, C), dlab.reshape(1, B * N)
    plane_step(tv, flags, params, dpts, dlab, True, False, "dense step after a %s step" % ("packed-bpc" if bpc else "packed"))


# ------------------------------------------------------------------------------------------
# I. everything at once
# ------------------------------------------------------------------------------------------
def cell_i_run(graph, x, y):
    """Three accumulated micro-steps of the everything-at-once model -> (losses, accumulated gradient, per-cloud [loss, accuracy])."""
    flags = head_flags(True, EDGE_MLP_DTYPE="bf16", LOSS_PER_CLOUD=True)
    tv = dgcnn.trainval(flags).initialize().use_graph(graph)
    tv.zero_gradients(None)
    losses, counts, clouds = [], [], []
    with spies() as spy:
        for _ in range(3):
            losses.append(float(tv.accum_gradient(None, [x], [y])[2]))
            counts.append(len(spy.gemms))
            clouds.append(host(tv.per_cloud_scalars()[0]).copy())
    assert E.EDGE_MLP_DTYPE == "bf16" and E.HEAD_PLANES == P.F16X2 and not E.DETERMINISTIC
    assert counts == ([9, 18, 18] if graph else [9, 18, 27]), counts              # a replay issues nothing from Python
    assert "dgcnn_edge_mlp_bf16_stats" in spy.calls and "dgcnn_seg_softmax_xent_f32" in spy.calls
    assert all(cl.shape == (B, 2) for cl in clouds)
    assert len(tv._graphs) == (1 if graph else 0)
    return np.asarray(losses), host(dgcnn.ctx().flat_grad).astype(np.float64), np.asarray(clouds)


def test_I_bf16_planes_loss_per_cloud_under_a_launch_plan(case, capfd):
    """bf16 edge MLP + plane head + LOSS_PER_CLOUD on the dense B = 4 tower, atomics mode (planes force it), dropout on: three
    micro-steps -- eager sighting, recording, replay -- under use_graph('plan') against the same three eager micro-steps: every loss
    and the accumulated gradient.  The bar is four times the measured spread of two eager runs (the atomics' noise)."""
    pts, lab = case
    E.PLANES_MIN_ROWS = 0
    x, y = dev(pts), dev(lab)
    l1, g1, c1 = cell_i_run(False, x, y)
    l2, g2, c2 = cell_i_run(False, x, y)
    lp, gp, cp = cell_i_run("plan", x, y)
    spread = {"loss": np.abs(l1 - l2).max(), "per-cloud loss": np.abs(c1[:, :, 0] - c2[:, :, 0]).max(), "gradient": fro(g2, g1)}
    plan = {"loss": np.abs(lp - l1).max(), "per-cloud loss": np.abs(cp[:, :, 0] - c1[:, :, 0]).max(), "gradient": fro(gp, g1)}
    for n in spread:                                                # (this run's spread, next to the recorded one the bar comes from)
        print("cell I: %s: two eager runs differ by %.3e (recorded %.3e); launch plan vs eager %.3e" % (n, spread[n], I_EAGER_SPREAD[n], plan[n]))
        ERRORS["cell I: spread of two eager runs, %s (recorded: sets the bar, x 4)" % n] = [float(spread[n]), I_EAGER_SPREAD[n]]
    assert len({round(float(l), 6) for l in l1}) == 3               # three masks, three losses
    for n in plan:
        note("cell I: launch plan vs eager, %s%s" % (n, " (rel. Frobenius)" if n == "gradient" else ""), plan[n], I_BAR[n])
    assert "capture failed" not in capfd.readouterr().err


# ------------------------------------------------------------------------------------------
# J. mode hygiene
# ------------------------------------------------------------------------------------------
def test_J_modes_do_not_outlive_their_trainval(case):
    """A bf16 + planes trainval runs a step; a default one initialised afterwards in the same process gives, in DETERMINISTIC mode,
    bit for bit the step it gives after a fresh dgcnn.reset().  DETERMINISTIC asked for together with HEAD_PLANES: the planes are
    off (their statistics are atomic) -- no plane GEMM, the same bits."""
    pts, lab = case
    E.PLANES_MIN_ROWS = 0
    plain = train_flags(NUM_CLASS=NCLS)

    def step(flags, expect_planes=0):
        tv = dgcnn.trainval(flags).initialize()
        tv.zero_gradients(None)
        with spies() as spy:
            res = tv.accum_gradient(None, [pts], [lab])
        assert len(spy.gemms) == expect_planes
        return float(res[2]), host(dgcnn.ctx().flat_grad).copy()
    dgcnn.reset()
    l0, g0 = step(plain)
    step(head_flags(True, EDGE_MLP_DTYPE="bf16", SEED=11), expect_planes=9)
    assert E.EDGE_MLP_DTYPE == "bf16" and E.HEAD_PLANES == P.F16X2 and not E.DETERMINISTIC
    l1, g1 = step(plain)
    assert E.EDGE_MLP_DTYPE == "f32" and E.HEAD_PLANES == E.HEAD_PLANES_ENV_DEFAULT and E.DETERMINISTIC
    np.testing.assert_array_equal(g1, g0)
    assert abs(l1 - l0) <= REPLAY_LOSS and np.abs(g0).sum() > 0       # (the REPORTED loss is summed with atomics: last bit)
    l2, g2 = step(train_flags(NUM_CLASS=NCLS, HEAD_PLANES="f16"))
    assert E.HEAD_PLANES == P.F16X2 and E.DETERMINISTIC and not E.planes_ok(B * N, 128, 1024)
    np.testing.assert_array_equal(g2, g0)


def test_J_per_cloud_batchnorm_with_bf16_stays_refused_before_any_launch():
    """EDGE_MLP_DTYPE = 'bf16' with per-cloud BatchNorm: refused with the engine's message, on the host -- not one H.call."""
    msg = "per-cloud BatchNorm takes the default conv0 only"
    E.EDGE_MLP_DTYPE = "bf16"
    x = torch.rand(OFF[-1], 4, device="cuda")
    with spies() as spy:
        for kw in (dict(bn_per_cloud=True), dict(bn_per_cloud_train=True)):
            with pytest.raises(ValueError, match=msg):
                dgcnn.ops.edge_conv(x, 8, 32, True, offsets=OFF, **kw)
        assert spy.calls == [] and spy.gemms == []
    pts, off, lab = packed_tower([70, 50, 96], 4, seed=1)
    tv = dgcnn.trainval(dgcnn.DGCNN_FLAGS(EDGE_CONV_LAYERS=2, EDGE_CONV_FILTERS=[32, 64], KVALUE=8, FC_FILTERS=[64, 32], NUM_CLASS=NCLS,
                                          NUM_CHANNEL=4, TRAIN=True, EDGE_MLP_DTYPE="bf16", BN_PER_CLOUD_TRAIN=True)).initialize()
    tv.zero_gradients(None)
    with spies() as spy:
        with pytest.raises(ValueError, match=msg):
            tv.accum_gradient(None, [pts], [lab], offsets=[off])
        assert not [n for n in spy.calls if n.startswith(("dgcnn_knn", "dgcnn_gemm", "dgcnn_edge", "dgcnn_seg"))], spy.calls

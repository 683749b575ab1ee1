"""The class-dimension tail (csrc/bn.hip: bn1_act_class_kernel, bn_softmax_xent_kernel, bn1_bwd_class_kernel; _engine.FUSE_CLASS_TAIL):
last FC layer (F = 256, dropout behind it) -> Final (NUM_CLASS <= 4) -> softmax / loss and back, in 8 launches instead of 15.

The design rule is that every fused kernel performs, per output element and per partial sum, the operations of the launches it
replaces in their order, so the fused entry points are compared BITWISE (torch.equal) with the sequence of separate launches on
the same inputs -- kernel by kernel and over whole training steps, eager and replayed.  Loss and accuracy are summed with float
atomics in both paths: they get the bar the replay tests already use, |difference| < 1e-6.  One float64 check of the fused path
alone keeps the module meaningful without the separate launches."""
import numpy as np
import pytest
import torch

import dgcnn
from dgcnn import _engine as E
from dgcnn import _hip as H
from gpu_helpers import host, note_ratio

pytestmark = pytest.mark.gpu

F = 256
EPS = 1e-3
KEEP = 0.7
SEED = 0x5EED1234


def _inputs(R, ncls, seed, dead_logit=None, dead_fc=None):
    rng = np.random.default_rng(seed)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    T1 = rng.standard_normal((R, F)).astype(np.float32) * 1.5 + 0.25
    mean1 = T1.mean(0).astype(np.float32)
    rstd1 = (1.0 / np.sqrt(T1.astype(np.float64).var(0) + EPS)).astype(np.float32)
    beta1 = (0.3 * rng.standard_normal(F)).astype(np.float32)
    if dead_fc is not None:
        beta1[dead_fc] = -100.0                                  # relu((t - mean) rstd + beta) == 0 in every row
    W = (rng.uniform(-1, 1, (F, ncls)) * np.sqrt(6.0 / (F + ncls))).astype(np.float32)
    betaf = (0.2 * rng.standard_normal(ncls)).astype(np.float32)
    if dead_logit is not None:
        betaf[dead_logit] = -100.0
    labels = rng.integers(0, ncls, R).astype(np.int32)
    weight = rng.uniform(0.5, 1.5, R).astype(np.float32)
    d = dict(T1=t(T1), mean1=t(mean1), rstd1=t(rstd1), beta1=t(beta1), W=t(W), betaf=t(betaf), labels=t(labels), weight=t(weight),
             seed=torch.tensor([SEED], dtype=torch.int64, device="cuda"))
    return d


def _alloc(R, ncls, nslots):
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")
    return dict(out1=z(R, F), logits=z(R, ncls), st=z(nslots, 2, ncls, dt=torch.float64), meanf=z(ncls), rstdf=z(ncls),
                fin=z(R, ncls), sm=z(R, ncls), dl=z(R, ncls), scal=torch.full((2,), 7.0, device="cuda"),
                redf=z(nslots, 2, ncls, dt=torch.float64), dbetaf=z(ncls) + 0.5, red1=z(nslots, 2, F, dt=torch.float64),
                dT1=z(R, F), dbeta1=z(F) + 0.25)


def _ws():
    return torch.empty(int(H.load().dgcnn_det_workspace_bytes(4)) + (1 << 20), dtype=torch.uint8, device="cuda")


def _reduce_det(i, o, R, ncls, ws):
    H.call("dgcnn_bn_bwd_reduce_det_f32", o["logits"].data_ptr(), R, 1, ncls, o["meanf"].data_ptr(), o["rstdf"].data_ptr(),
           i["betaf"].data_ptr(), 1, o["dl"].data_ptr(), ncls, 0, 0, 0, 0, 0, o["redf"].data_ptr(), ws.data_ptr(), ws.numel())


def _unfused(i, R, ncls, nslots):
    """The 15-launch chain through the entry points it has always used; -> outputs (+ the raw logits before the backward)."""
    o = _alloc(R, ncls, nslots)
    ws = _ws()
    p1 = (i["mean1"].data_ptr(), i["rstd1"].data_ptr(), i["beta1"].data_ptr())
    H.call("dgcnn_bn1_act_dropout_f32", i["T1"].data_ptr(), R, F, *p1, 1, KEEP, i["seed"].data_ptr(), o["out1"].data_ptr(), F)
    H.call("dgcnn_gemm_f32", 0, 0, R, ncls, F, o["out1"].data_ptr(), F, i["W"].data_ptr(), ncls, o["logits"].data_ptr(), ncls, 0.0,
           0, 0, 0, o["st"].data_ptr(), 0, 0, ws.data_ptr(), ws.numel())
    H.call("dgcnn_bn_finalize_f32", o["st"].data_ptr(), ncls, float(R), EPS, o["meanf"].data_ptr(), o["rstdf"].data_ptr())
    H.call("dgcnn_bn_act_kreduce_f32", o["logits"].data_ptr(), R, 1, ncls, o["meanf"].data_ptr(), o["rstdf"].data_ptr(),
           i["betaf"].data_ptr(), 1, o["fin"].data_ptr(), ncls, 0, 0, 0, 0, 0)
    H.memset(o["scal"])
    H.call("dgcnn_softmax_xent_f32", o["fin"].data_ptr(), i["labels"].data_ptr(), i["weight"].data_ptr(), R, ncls, o["sm"].data_ptr(),
           o["dl"].data_ptr(), o["scal"].data_ptr())
    o["logits_raw"] = o["logits"].clone()
    _reduce_det(i, o, R, ncls, ws)
    H.call("dgcnn_bn_bwd_apply_f32", o["logits"].data_ptr(), R, 1, ncls, o["meanf"].data_ptr(), o["rstdf"].data_ptr(),
           i["betaf"].data_ptr(), 1, o["dl"].data_ptr(), ncls, 0, 0, 0, 0, 0, o["redf"].data_ptr(), o["logits"].data_ptr(), 0, 0,
           o["dbetaf"].data_ptr(), 1.0)
    dout1 = torch.empty((R, F), dtype=torch.float32, device="cuda")
    H.call("dgcnn_gemm_f32", 0, 1, R, F, ncls, o["logits"].data_ptr(), ncls, i["W"].data_ptr(), ncls, dout1.data_ptr(), F, 0.0,
           0, 0, 0, 0, 0, 0, ws.data_ptr(), ws.numel())
    H.call("dgcnn_bn1_bwd_dropout_f32", i["T1"].data_ptr(), R, F, *p1, 1, KEEP, i["seed"].data_ptr(), dout1.data_ptr(), F,
           o["red1"].data_ptr(), o["dT1"].data_ptr(), o["dbeta1"].data_ptr(), 1.0)
    o["dout1"] = dout1
    return o


def _fused(i, R, ncls, nslots):
    o = _alloc(R, ncls, nslots)
    ws = _ws()
    p1 = (i["mean1"].data_ptr(), i["rstd1"].data_ptr(), i["beta1"].data_ptr())
    H.call("dgcnn_bn1_act_class_f32", i["T1"].data_ptr(), R, F, *p1, 1, KEEP, i["seed"].data_ptr(), o["out1"].data_ptr(), F,
           i["W"].data_ptr(), ncls, ncls, o["logits"].data_ptr(), ncls, o["st"].data_ptr(), o["scal"].data_ptr())
    H.call("dgcnn_bn_softmax_xent_f32", o["logits"].data_ptr(), o["st"].data_ptr(), float(R), EPS, i["betaf"].data_ptr(), 1, R, ncls,
           o["meanf"].data_ptr(), o["rstdf"].data_ptr(), o["fin"].data_ptr(), i["labels"].data_ptr(), i["weight"].data_ptr(),
           o["sm"].data_ptr(), o["dl"].data_ptr(), o["scal"].data_ptr())
    o["logits_raw"] = o["logits"].clone()
    _reduce_det(i, o, R, ncls, ws)
    o["redf_in"] = o["redf"].clone()
    H.call("dgcnn_bn1_bwd_class_f32", i["T1"].data_ptr(), R, F, *p1, 1, KEEP, i["seed"].data_ptr(), o["logits"].data_ptr(), ncls,
           o["meanf"].data_ptr(), o["rstdf"].data_ptr(), i["betaf"].data_ptr(), 1, o["dl"].data_ptr(), o["redf"].data_ptr(),
           o["dbetaf"].data_ptr(), 1.0, i["W"].data_ptr(), ncls, o["red1"].data_ptr(), o["dT1"].data_ptr(), o["dbeta1"].data_ptr(), 1.0, 3)
    torch.cuda.synchronize()
    return o


class _slots(object):
    def __init__(self, n):
        self.n = n

    def __enter__(self):
        self.prev = H.stat_slots()
        H.set_stat_slots(self.n)

    def __exit__(self, *exc):
        H.set_stat_slots(self.prev)
        return False


# (R, classes, statistics slots, dead logit column, dead FC column).  The streaming product's grid is min(ceil(R / 4), 2048) workgroups,
# capped at the slot count when that is above 32: 256 slots at R = 4099 / 1025 give a grid EQUAL to the slot count (R = 1025 is
# 4 x grid + 1: one wave gets a second row), 32 slots at R = 1000 a grid of 250 workgroups on 32 slots (the sums of a slot's
# writers are exact in fp64 for these magnitudes, so the order of the atomics does not show).
CASES = [(4, 2, 256, None, None),
         (1000, 2, 32, None, None),
         (1000, 3, 256, 1, 17),
         (1025, 4, 256, None, None),
         (4099, 2, 256, 0, 255),
         (4099, 3, 320, None, None)]


@pytest.mark.parametrize("R,ncls,nslots,dead_logit,dead_fc", CASES)
def test_fused_entry_points_match_the_separate_launches_bitwise(R, ncls, nslots, dead_logit, dead_fc):
    i = _inputs(R, ncls, 100 + R + ncls, dead_logit, dead_fc)
    with _slots(nslots):
        a = _unfused(i, R, ncls, nslots)
        b = _fused(i, R, ncls, nslots)
    torch.cuda.synchronize()
    # forward: dropped FC output, raw logits, their raw statistics slots, mean / rstd, activated logits, softmax, d(logits)
    # backward: dT_final (in place of the logits), d(beta_final), the FC layer's sums (slot 0 after the finalize), dT, d(beta)
    for name in ("out1", "logits_raw", "st", "meanf", "rstdf", "fin", "sm", "dl", "logits", "dbetaf", "red1", "dT1", "dbeta1"):
        assert torch.equal(a[name], b[name]), "%s differs (R %d, %d classes, %d slots)" % (name, R, ncls, nslots)
    assert torch.equal(b["redf"], b["redf_in"])                    # the fused backward folds red_f without rewriting it
    sa, sb = host(a["scal"]), host(b["scal"])
    print("loss/accuracy separate %r fused %r" % (sa.tolist(), sb.tolist()))
    assert np.abs(sa - sb).max() < 1e-6
    if dead_logit is not None:
        assert not host(b["fin"])[:, dead_logit].any()
    if dead_fc is not None:
        assert not host(b["out1"])[:, dead_fc].any()
        assert not host(b["red1"])[0, :, dead_fc].any()
    assert host(b["out1"]).any() and host(b["dT1"]).any() and host(b["dl"]).any()


def test_fused_path_against_float64():
    """The fused kernels alone: each product / sum against float64 on the operands the kernel itself read, within
    (n_terms + 8) x 2^-24 x sum |term| (any-order fp32 summation plus the roundings inside a term, as in test_gpu_bn_kernels.py)."""
    R, ncls, nslots = 1000, 3, 256
    i = _inputs(R, ncls, 7)
    with _slots(nslots):
        o = _fused(i, R, ncls, nslots)
    f8 = lambda t: host(t).astype(np.float64)
    T1, mu, rs, be, W = f8(i["T1"]), f8(i["mean1"]), f8(i["rstd1"]), f8(i["beta1"]), f8(i["W"])
    out1, logits, dTf = f8(o["out1"]), f8(o["logits_raw"]), f8(o["logits"])
    # the dropped activation: relu(bn) / keep or 0, a keep fraction near 0.7 among the positive ones
    z = np.maximum((host(i["T1"]) - host(i["mean1"])) * host(i["rstd1"]) + host(i["beta1"]), np.float32(0))
    kept = host(o["out1"]) != 0
    np.testing.assert_array_equal(host(o["out1"])[kept], (z * (np.float32(1) / np.float32(KEEP)))[kept])
    frac = kept[z > 0].mean()
    assert 0.68 < frac < 0.72, frac
    # logits = out1 W: 256 terms per element
    note_ratio("class tail: logits", logits - out1 @ W, np.abs(out1) @ np.abs(W), F, F + 8, record=False)
    # statistics: column sums of the logits and of their squares over R rows (sum of the slots)
    st = f8(o["st"]).sum(0)
    lg32 = host(o["logits_raw"])
    note_ratio("class tail: stats sum", st[0] - logits.sum(0), np.abs(logits).sum(0), R, R + 8, record=False)
    note_ratio("class tail: stats sumsq", st[1] - (lg32 * lg32).astype(np.float64).sum(0), (logits ** 2).sum(0), R, R + 8, record=False)
    mean64 = logits.sum(0) / R
    np.testing.assert_allclose(f8(o["meanf"]), mean64, rtol=0, atol=(R + 8) * 2.0 ** -24 * np.abs(logits).sum(0).max() / R + 1e-7)
    # softmax of the activated logits, rows sum to one
    fin = f8(o["fin"])
    e = np.exp(fin - fin.max(1, keepdims=True))
    np.testing.assert_allclose(f8(o["sm"]), e / e.sum(1, keepdims=True), rtol=0, atol=1e-6)
    # the FC layer's backward sums: dz = [out1 > 0] (dT_final W^T) / keep, sums of dz and dz xhat over R rows
    dz = np.where(out1 > 0, (dTf @ W.T) * float(np.float32(1) / np.float32(KEEP)), 0.0)
    absdz = np.where(out1 > 0, (np.abs(dTf) @ np.abs(W).T) * float(np.float32(1) / np.float32(KEEP)), 0.0)
    xh = (T1 - mu) * rs
    red = f8(o["red1"])[0]
    note_ratio("class tail: sum dz", red[0] - dz.sum(0), absdz.sum(0), R, R + 8, record=False)
    note_ratio("class tail: sum dz xhat", red[1] - (dz * xh).sum(0), (absdz * np.abs(xh)).sum(0), R, R + 8, record=False)
    # dT = rstd (dz - c1 - xhat c2) with the kernel's own sums
    c1, c2 = red[0] / R, red[1] / R
    want = rs * (dz - c1 - xh * c2)
    np.testing.assert_allclose(f8(o["dT1"]), want, rtol=0, atol=16 * 2.0 ** -24 * np.abs(rs).max() * (absdz.max() + np.abs(c1).max() + np.abs(xh).max() * np.abs(c2).max()))


def test_wrong_shapes_are_refused():
    i = _inputs(8, 2, 1)
    o = _alloc(8, 2, 256)
    p1 = (i["mean1"].data_ptr(), i["rstd1"].data_ptr(), i["beta1"].data_ptr())
    with pytest.raises((ValueError, H.HipError)):                  # a 128-wide layer has two rows per wave
        H.call("dgcnn_bn1_act_class_f32", i["T1"].data_ptr(), 8, 128, *p1, 1, KEEP, i["seed"].data_ptr(), o["out1"].data_ptr(), 128,
               i["W"].data_ptr(), 2, 2, o["logits"].data_ptr(), 2, o["st"].data_ptr(), o["scal"].data_ptr())
    with pytest.raises((ValueError, H.HipError)):                  # five classes
        H.call("dgcnn_bn1_act_class_f32", i["T1"].data_ptr(), 8, F, *p1, 1, KEEP, i["seed"].data_ptr(), o["out1"].data_ptr(), F,
               i["W"].data_ptr(), 5, 5, o["logits"].data_ptr(), 5, o["st"].data_ptr(), o["scal"].data_ptr())
    torch.cuda.synchronize()
    assert not host(o["out1"]).any() and not host(o["logits"]).any()


# ---- whole steps -------------------------------------------------------------------------------------------------------------
FUSED_TAGS = {"bn1_act_class_kernel", "bn_softmax_xent_kernel", "bn1_bwd_class_kernel"}


def _flags(**kw):
    base = dict(EDGE_CONV_LAYERS=3, EDGE_CONV_FILTERS=[64, 64, 128], KVALUE=8, FC_LAYERS=2, FC_FILTERS=[512, 256], NUM_CLASS=2,
                NUM_CHANNEL=3, TRAIN=True, SEED=5, LEARNING_RATE=1e-3, DETERMINISTIC=True)
    base.update(kw)
    return dgcnn.DGCNN_FLAGS(**base)


def _data(steps=3, B=2, N=256, ncls=2):
    rng = np.random.default_rng(21)
    return (torch.from_numpy(rng.random((steps, B, N, 3), dtype=np.float32)).cuda(),
            torch.from_numpy(rng.integers(0, ncls, (steps, B, N)).astype(np.int32)).cuda())


def _train(fuse, graph, steps=3, **kw):
    pts, lab = _data(steps, ncls=kw.get("NUM_CLASS", 2))
    prev, E.FUSE_CLASS_TAIL = E.FUSE_CLASS_TAIL, fuse
    try:
        tv = dgcnn.trainval(_flags(**kw)).initialize().use_graph(graph)
        c = dgcnn.ctx()
        out, seen = [], []
        tower = tv._tower

        def keep_softmax(*a, **k):                                 # (accum_gradient drops the tower's softmax)
            r = tower(*a, **k)
            seen.append(r[0].clone())
            return r
        tv._tower = keep_softmax
        for s in range(steps):
            tv.zero_gradients(None)
            res = tv.accum_gradient(None, [pts[s]], [lab[s]])
            grad = c.flat_grad.clone()
            tv.apply_gradient(None)
            out.append((seen[-1], grad, c.flat_param.clone(), float(res[1]), float(res[2])))
        assert len(seen) == steps
        return tv, out
    finally:
        E.FUSE_CLASS_TAIL = prev
        E.DETERMINISTIC = E.DETERMINISTIC_ENV_DEFAULT


@pytest.mark.parametrize("graph", [False, "plan", True], ids=["eager", "launch-plan", "hip-graph"])
def test_training_steps_are_bitwise_equal_with_the_switch_on_and_off(graph):
    """B = 2, N = 256, k = 8, (64, 64, 128) + (512, 256), 2 classes, 3 steps (eager; recorded; replayed under the replay modes)."""
    tv_a, a = _train(False, graph)
    tv_b, b = _train(True, graph)
    if graph:
        assert len(tv_a._graphs) == 1 and len(tv_b._graphs) == 1
    for s, ((sm_a, g_a, p_a, acc_a, loss_a), (sm_b, g_b, p_b, acc_b, loss_b)) in enumerate(zip(a, b)):
        assert torch.equal(sm_a, sm_b), "softmax, step %d" % s
        assert torch.equal(g_a, g_b), "flat_grad, step %d" % s
        assert torch.equal(p_a, p_b), "flat_param, step %d" % s
        assert abs(acc_a - acc_b) < 1e-6 and abs(loss_a - loss_b) < 1e-6
    assert not torch.equal(a[0][2], a[-1][2])                      # it trained


def _tags(fuse=True, **kw):
    H.TIMER = tm = H.Timer()
    try:
        _train(fuse, False, steps=1, **kw)
        return set(tm.summary())
    finally:
        H.TIMER = None


def test_fused_path_is_taken_only_where_it_applies():
    """Launch tags recorded by H.Timer over one eager training step."""
    on = _tags()
    assert FUSED_TAGS <= on, on
    assert not (FUSED_TAGS & _tags(fuse=False))                    # the switch
    assert not (FUSED_TAGS & _tags(FC_FILTERS=[512, 128]))         # a narrower last FC layer: two rows per wave
    assert not (FUSED_TAGS & _tags(NUM_CLASS=5))                   # more classes than the streaming product takes
    assert not (FUSED_TAGS & _tags(DETERMINISTIC=False))           # atomics mode
    assert not (FUSED_TAGS & _tags(LOSS_PER_CLOUD=True))           # per-cloud loss
    assert not (FUSED_TAGS & _tags(FC_LAYERS=1, FC_FILTERS=[256]))  # FC0 carries the per-cloud bias of the global feature
    prev, E.FUSE_DROPOUT = E.FUSE_DROPOUT, False
    try:
        assert not (FUSED_TAGS & _tags())                          # without the fused dropout pass there is nothing to extend
    finally:
        E.FUSE_DROPOUT = prev

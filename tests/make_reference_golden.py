#!/usr/bin/env python
"""Generates tests/golden/ref_*.npz -- known-answer vectors RECORDED FROM THE REFERENCE PROGRAM.

tests/make_golden.py records what the oracle computes; this generator executes the reference's own dgcnn/ops.py, dgcnn/model.py
and dgcnn/trainval.py under tests/tf1_standin.py (float64) and records what THEY compute.  It runs on the CPU, where the
reference tree is present ($DGCNN_REFERENCE_DIR); the fixtures are pure data -- inputs, parameters, per-layer neighbour
indices, the tensors the reference's functions returned, logits / softmax / loss / accuracy, gradients, parameters after the
Adam step, and a `cfg` literal -- which the CPU suite (oracle) and the GPU suite (HIP path) reproduce without the reference.

    python tests/make_reference_golden.py        # rewrites tests/golden/ref_*.npz

Storage.  Parameters are drawn, then rounded to the nearest float16 and stored as float16: the upcast to float32 / float64 is
exact, the files are half the size.  Small outputs are float64; the large ones (parameter gradients, accumulators, parameters
after Adam, the nine tensors of the three-layer stack, the layer inputs of the models) are float32, and the gradients of a
model live in a second file `<case>_grads.npz` where one file would pass the size limit of a committed file.  The EdgeConv
widths are ones the GPU suite already runs the block at.  The widths are the smallest the graph allows (MergedEdgeConv is 64 L x 1024 whatever the filters): all cases together
stay under 4 MB.

Near-ties.  The reference runs in float64 here; the HIP k-NN and the float32 oracle do not.  An input is accepted only if at
every EdgeConv layer and row the k-th and the (k + 1)-th smallest squared distance are at least 100 x the largest
|float32-oracle - float64| distance discrepancy seen at that layer apart (`knn_gap`, `knn_disc` per layer in the file), and
O.k_nn on the float32 layer input reproduces the stored indices -- their order included -- exactly.  Seeds are tried in order; 50 failures are an error.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
from oracle import dgcnn_oracle as O  # noqa: E402
import tf1_standin as S  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
GAP_FACTOR = 100.0
MAX_SEEDS = 50

MODEL_CASES = {
    # 3 layers with a different last width: the `3 * i + 2` picks and the concat order [global] + tensors are all distinguishable
    "ref_model_dgcnn": dict(MODEL_NAME="dgcnn", EDGE_CONV_LAYERS=3, EDGE_CONV_FILTERS=[64, 64, 128], KVALUE=5, FC_LAYERS=2,
                            FC_FILTERS=[8, 8], NUM_CLASS=3, NUM_CHANNEL=3),
    # unequal filters: the shortcut convolution appears (its width must be 64: ops.py:62-63,134)
    "ref_model_residual": dict(MODEL_NAME="residual-dgcnn", EDGE_CONV_LAYERS=2, EDGE_CONV_FILTERS=[32, 64], KVALUE=6, FC_LAYERS=2,
                               FC_FILTERS=[8, 8], NUM_CLASS=2, NUM_CHANNEL=4),
    "ref_model_nofc": dict(MODEL_NAME="residual-dgcnn-nofc", EDGE_CONV_LAYERS=2, EDGE_CONV_FILTERS=[32, 64], KVALUE=5, FC_LAYERS=2,
                           FC_FILTERS=[8, 8], NUM_CLASS=5, NUM_CHANNEL=3),
}
TRAINVAL_CFG = dict(MODEL_NAME="dgcnn", EDGE_CONV_LAYERS=1, EDGE_CONV_FILTERS=8, KVALUE=6, FC_LAYERS=2, FC_FILTERS=[8, 8],
                    NUM_CLASS=3, NUM_CHANNEL=3, LEARNING_RATE=1e-3, MINIBATCH_SIZE=2, GPUS=[0, 1], WEIGHT_KEY="weight")
B, N = 2, 40
CASES = ["ref_edge_conv", "ref_repeat_list_k"] + list(MODEL_CASES) + ["ref_trainval_two_towers"]


class NearTie(Exception):
    pass


def f16_exact(a):
    return np.asarray(a).astype(np.float16)


def draw_params(flags, num_channel, rng, prefix=""):
    """Xavier weights, perturbed (non-zero) betas, every value a float16 -> {name: float16 array}."""
    P = O.init_params(flags, num_channel, seed=int(rng.integers(1 << 30)))
    for n in P:
        if n.endswith("beta"):
            P[n] = rng.normal(0, 0.2, P[n].shape)
    return {prefix + n: f16_exact(v) for n, v in P.items()}


def knn_margin(x64, idx, k):
    """(smallest gap between the k-th and the (k + 1)-th smallest float64 squared distance of any row, largest
    |float32 oracle - float64| distance) of one layer input (B, N, C) float64; raises NearTie when the condition fails or the
    float32 oracle does not reproduce idx."""
    x64 = np.asarray(x64, np.float64)
    sq = np.sum(np.square(x64), axis=-1, keepdims=True)
    D = sq + np.transpose(sq, (0, 2, 1)) - 2 * np.matmul(x64, np.transpose(x64, (0, 2, 1)))
    x32 = x64.astype(np.float32)
    disc = max(float(np.abs(O.dist_matrix_f32(x32[b]).astype(np.float64) - D[b]).max()) for b in range(len(x32)))
    s = np.sort(D, axis=-1)
    gap = float((s[..., k] - s[..., k - 1]).min()) if k < s.shape[-1] else np.inf
    if not gap >= GAP_FACTOR * disc:
        raise NearTie("gap %.3g < %g x %.3g" % (gap, GAP_FACTOR, disc))
    if not np.array_equal(O.k_nn(x32, k), np.asarray(idx)):
        raise NearTie("the float32 oracle picks other neighbours")
    return gap, disc


class knn_spy(object):
    """Records (layer input, idx, k) of every k_nn call the reference program makes, eager or deferred."""

    def __init__(self, ref):
        self.ref, self.calls = ref, []

    def __enter__(self):
        self.orig = orig = self.ref.ops.k_nn

        def rec(points, idx, k):
            self.calls.append((S._t(points).detach().numpy().copy(), S._t(idx).numpy().astype(np.int32), int(k)))
            return idx

        def spy(points, k):
            idx = orig(points, k)
            return S.Node(rec, (points, idx, k), {}) if isinstance(idx, S.Node) else rec(points, idx, k)
        self.ref.ops.k_nn = spy
        return self

    def __exit__(self, *exc):
        self.ref.ops.k_nn = self.orig
        return False

    def margins(self, arrays, names):
        """Checks every recorded call; stores idx / gap / disc under the given names."""
        assert len(names) == len(self.calls)
        for name, (x, idx, k) in zip(names, self.calls):
            gap, disc = knn_margin(x, idx, k)
            arrays["idx" + name] = idx
            arrays["knn_gap" + name] = np.float64(gap)
            arrays["knn_disc" + name] = np.float64(disc)


def leaves(P):
    return {n: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for n, v in P.items()}


def np64(t):
    return t.detach().numpy().astype(np.float64)


# ------------------------------------------------------------------------------------------------------------
def gen_edge_conv(rng):
    C, k, F = 4, 5, 8
    pts = rng.random((B, N, C), dtype=np.float32)
    P = {"conv0/weights": f16_exact(rng.normal(0, 0.5, (2 * C, F))), "conv0/BatchNorm/beta": f16_exact(rng.normal(0, 0.3, F)),
         "conv1/weights": f16_exact(rng.normal(0, 0.3, (2 * F, 64))), "conv1/BatchNorm/beta": f16_exact(rng.normal(0, 0.3, 64))}
    d = [rng.normal(size=(B, N, 1, w)).astype(np.float32) for w in (F, F, 64)]
    L = leaves(P)
    x = torch.tensor(pts.astype(np.float64), requires_grad=True)
    arrays = {}
    with S.reference_program(L) as ref, knn_spy(ref) as spy:
        outs = ref.ops.edge_conv(x, k, F, True)
        assert isinstance(outs, list) and len(outs) == 3
        g = torch.autograd.grad(sum((o * torch.tensor(di.astype(np.float64))).sum() for o, di in zip(outs, d)), [x] + list(L.values()))
        spy.margins(arrays, [""])
    arrays.update(points=pts, k=np.int32(k), W0=P["conv0/weights"], beta0=P["conv0/BatchNorm/beta"], W1=P["conv1/weights"],
                  beta1=P["conv1/BatchNorm/beta"], net_max=np64(outs[0]), net_mean=np64(outs[1]), net=np64(outs[2]),
                  d_max=d[0], d_mean=d[1], d_net=d[2], dx=np64(g[0]), dW0=np64(g[1]), dbeta0=np64(g[2]), dW1=np64(g[3]),
                  dbeta1=np64(g[4]), cfg=np.array(repr(dict(k=k, num_filters=F))))
    return {"": arrays}


def gen_repeat_list_k(rng):
    C, ks, Fs = 3, [6, 4, 2], [8, 32, 32]
    flags = O.Flags(MODEL_NAME="residual-dgcnn-nofc", EDGE_CONV_LAYERS=3, EDGE_CONV_FILTERS=Fs, NUM_CLASS=2)
    P = {n: v for n, v in draw_params(flags, C, rng).items() if n.startswith("EdgeConv") and "shortcut" not in n}
    pts = rng.random((B, N, C), dtype=np.float32)
    L = leaves(P)
    x = torch.tensor(pts.astype(np.float64), requires_grad=True)
    arrays = {}
    with S.reference_program(L) as ref, knn_spy(ref) as spy:
        outs = ref.ops.repeat_edge_conv(x, 3, list(ks), list(Fs), True)
        assert len(outs) == 9
        d = [rng.normal(size=tuple(o.shape)).astype(np.float32) for o in outs]
        g = torch.autograd.grad(sum((o * torch.tensor(di.astype(np.float64))).sum() for o, di in zip(outs, d)), [x] + list(L.values()))
        spy.margins(arrays, ["%d" % i for i in range(3)])
    arrays.update(points=pts, dx=np64(g[0]), cfg=np.array(repr(dict(repeat=3, k=ks, num_filters=Fs))))
    for i, (o, di) in enumerate(zip(outs, d)):
        arrays["tensor%d" % i], arrays["d%d" % i] = np64(o), di
    arrays.update({"param:" + n: v for n, v in P.items()})
    arrays.update({"grad:" + n: np64(gi) for n, gi in zip(L, g[1:])})
    return {"": arrays}


def gen_model(name, rng):
    cfg = MODEL_CASES[name]
    flags = O.Flags(TRAIN=True, **cfg)
    C = cfg["NUM_CHANNEL"]
    P = draw_params(flags, C, rng)
    pts = rng.random((B, N, C), dtype=np.float32)
    labels = rng.integers(0, cfg["NUM_CLASS"], (B, N)).astype(np.int32)
    L = leaves(P)
    x = torch.tensor(pts.astype(np.float64), requires_grad=True)
    arrays = {}
    with S.reference_program(L) as ref, knn_spy(ref) as spy:      # dropout mask None: model.py:91 is the identity
        logits = ref.model.build(x, flags)
        lab = torch.tensor(labels.astype(np.int64))
        # the loss / softmax / accuracy lines of trainval.py:39-52, evaluated by the stand-in's functions
        loss = S.reduce_mean(S.sparse_softmax_cross_entropy_with_logits(logits=logits, labels=lab))
        sm = S.softmax(logits=logits)
        acc = S.reduce_mean(S.cast(S.equal(S.argmax(logits, 2), S.to_int64(lab)), S.float32))
        g = torch.autograd.grad(loss, [x] + list(L.values()))
        spy.margins(arrays, ["%d" % i for i in range(int(cfg["EDGE_CONV_LAYERS"]))])
        for i, (xin, _, _) in enumerate(spy.calls):
            if i:
                arrays["layer_in%d" % i] = xin                    # squeeze(tensors[3 * (i - 1) + 2]): what layer i's graph is built on
        assert [v.scoped_name for v in S.created_variables()] == list(P)
    arrays.update(points=pts, labels=labels, logits=np64(logits), softmax=np64(sm), loss=np.float64(loss.item()),
                  accuracy=np.float64(acc.item()), dpoints=np64(g[0]), cfg=np.array(repr(cfg)))
    arrays.update({"param:" + n: v for n, v in P.items()})
    grads = {"grad:" + n: np64(gi) for n, gi in zip(L, g[1:])}
    head = [n for n in grads if n.startswith(("grad:FC", "grad:Final"))]      # (small enough for the first file)
    arrays.update({n: grads.pop(n) for n in head})
    return {"": arrays, "_grads": grads}


def gen_trainval(rng, weighted=True, second_apply=False):
    """trainval.py end to end through the deferred stand-in: two towers, MINIBATCH_SIZE 2, per-point weights; initialize,
    zero_gradients, two accum_gradient calls, apply_gradient, inference with labels and weights (and without: arity only)."""
    cfg = dict(TRAINVAL_CFG, WEIGHT_KEY="weight" if weighted else "")
    flags = O.Flags(TRAIN=True, DEBUG=False, **cfg)
    C, nc = cfg["NUM_CHANNEL"], cfg["NUM_CLASS"]
    P = draw_params(flags, C, rng)
    arrays = {"cfg": np.array(repr(cfg))}
    feeds = []
    for s in range(3):                                             # micro-steps 0, 1; then the inference feed
        pts = [rng.random((B, N, C), dtype=np.float32) for _ in range(2)]
        lab = [rng.integers(0, nc, (B, N)).astype(np.int32) for _ in range(2)]
        wgt = [(0.5 + rng.random((B, N))).astype(np.float32) for _ in range(2)]
        feeds.append((pts, lab, wgt) if weighted else (pts, lab))
        tag = "inf" if s == 2 else "s%d" % s
        for r in range(2):
            arrays["points_%s_r%d" % (tag, r)], arrays["labels_%s_r%d" % (tag, r)] = pts[r], lab[r]
            if weighted:
                arrays["weights_%s_r%d" % (tag, r)] = wgt[r]
    with S.reference_program({"dgcnn/" + n: np.asarray(v, np.float64) for n, v in P.items()}) as ref, knn_spy(ref) as spy:
        tv = ref.trainval.trainval(flags)
        tv.initialize()
        tvars = S.trainable_variables()
        assert [v.scoped_name for v in tvars] == ["dgcnn/" + n for n in P]          # AUTO_REUSE: each variable listed once
        sess = S.Session()
        tv.zero_gradients(sess)
        for s in range(2):
            res = tv.accum_gradient(sess, *feeds[s])
            assert len(res) == 3 and len(res[0]) == len(P)
            arrays["accuracy_s%d" % s], arrays["loss_s%d" % s] = np.float64(res[1]), np.float64(res[2])
        arrays.update({"accum:" + n: a for n, a in zip(P, res[0])})
        assert tv.apply_gradient(sess) is None
        arrays.update({"new:" + n: v.value.numpy().copy() for n, v in zip(P, tvars)})
        res = tv.inference(sess, *feeds[2])
        assert len(res) == 4 and len(tv.inference(sess, feeds[2][0])) == 2
        arrays.update(softmax_inf_r0=res[0], softmax_inf_r1=res[1], accuracy_inf=np.float64(res[2]), loss_inf=np.float64(res[3]))
        names = ["_s%d_r%d" % (s, r) for s in range(2) for r in range(2)] + ["_inf_r0", "_inf_r1"] * 2
        del spy.calls[6:]                                          # (the label-free inference repeats the last two)
        spy.margins(arrays, names[:6])
        if second_apply:                                           # (tests only: the same accumulators again, Adam's t = 2)
            tv.apply_gradient(sess)
            arrays.update({"new2:" + n: v.value.numpy().copy() for n, v in zip(P, tvars)})
    arrays.update({"param:" + n: v for n, v in P.items()})
    return {"": arrays}


def generate(name, seed):
    """{file suffix: {key: array}} of one case from one seed; NearTie when the seed's inputs are not acceptable."""
    rng = np.random.default_rng([seed, CASES.index(name)])
    if name == "ref_edge_conv":
        return gen_edge_conv(rng)
    if name == "ref_repeat_list_k":
        return gen_repeat_list_k(rng)
    if name == "ref_trainval_two_towers":
        return gen_trainval(rng)
    return gen_model(name, rng)


F32_STORED = ("accum:", "new:", "grad:", "tensor", "layer_in")


def stored(files):
    """The arrays as they are written: the large results -- parameter gradients, accumulators, parameters after Adam, the
    tensors of the three-layer stack and the layer inputs of the models -- cast to float32."""
    return {suffix: {k: (v.astype(np.float32) if k.startswith(F32_STORED) else v) for k, v in arrays.items()} for suffix, arrays in files.items()}


def load(name):
    """One case as the tests read it: both files merged, the float16 parameters upcast (exactly) to float32."""
    g = dict(np.load(os.path.join(OUT, name + ".npz"), allow_pickle=False))
    extra = os.path.join(OUT, name + "_grads.npz")
    if os.path.exists(extra):
        g.update(np.load(extra, allow_pickle=False))
    return {k: (v.astype(np.float32) if v.dtype == np.float16 else v) for k, v in g.items()}


def group(g, prefix):
    return {k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix)}


def generate_accepted(name):
    for seed in range(MAX_SEEDS):
        try:
            files = generate(name, seed)
        except NearTie as e:
            print("%s: seed %d rejected (%s)" % (name, seed, e))
            continue
        files[""]["seed"] = np.int64(seed)
        return files
    raise RuntimeError("%s: no seed below %d gives inputs without near-ties" % (name, MAX_SEEDS))


def main():
    if not S.reference_present():
        raise SystemExit("the reference tree is not at %s (set DGCNN_REFERENCE_DIR)" % S.reference_dir())
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(1)                                       # one summation order, whatever the machine
    total = 0
    for name in CASES:
        for suffix, arrays in stored(generate_accepted(name)).items():
            path = os.path.join(OUT, name + suffix + ".npz")
            np.savez_compressed(path, **arrays)
            total += os.path.getsize(path)
            print("%-36s %8d bytes  %d arrays" % (name + suffix, os.path.getsize(path), len(arrays)))
    print("total %d bytes" % total)


if __name__ == "__main__":
    main()

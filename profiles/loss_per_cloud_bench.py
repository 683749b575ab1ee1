"""The per-cloud loss (flags.LOSS_PER_CLOUD, csrc/seg_loss.hip) on the 24-cloud tower of profiles/bn_per_cloud_train_bench.py
(N ~ U[1024, 8192], rng 0, R = 114234; BASELINE configs[1]'s model, C = 4, eager launches, default deterministic mode), from HIP
events after a synchronise, the variants alternating over several rounds (min / median / max of the rounds):

    the call        dgcnn_seg_softmax_xent_f32 (two launches, nothing zero-filled) against dgcnn_softmax_xent_f32 (one launch behind a
                    zero fill of its two scalars) on the same (R, 2) logits, labels and row weights, softmax and dlogits written
    the step        zero_gradients + accum_gradient of the packed tower under BN_PER_CLOUD_TRAIN, with LOSS_PER_CLOUD on and off

    python profiles/loss_per_cloud_bench.py [--reps 5] [--rounds 5] [--out profiles/packed/loss_per_cloud.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dynamic-gcnn_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import dgcnn                                   # noqa: E402
from dgcnn import _engine as E                 # noqa: E402
from dgcnn import _hip as H                    # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--call_reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed", "loss_per_cloud.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "loss_per_cloud_bench measures on the GPU"
    rng = np.random.default_rng(0)
    sizes = rng.integers(1024, 8193, 24)
    off = np.concatenate([[0], np.cumsum(sizes)])
    R, nseg, ncls = int(off[-1]), len(sizes), 2
    flags = dgcnn.DGCNN_FLAGS(MODEL_NAME="dgcnn", EDGE_CONV_LAYERS=3, EDGE_CONV_FILTERS=[64, 64, 128], FC_LAYERS=2, FC_FILTERS=[512, 256],
                              NUM_CLASS=ncls, KVALUE=20, NUM_CHANNEL=4, TRAIN=True, SEED=1, BN_PER_CLOUD_TRAIN=True)
    tv = dgcnn.trainval(flags).initialize()
    pts = torch.from_numpy(rng.random((R, 4), dtype=np.float32)).cuda()
    lab = torch.from_numpy(rng.integers(0, ncls, R).astype(np.int32)).cuda()
    wgt = torch.from_numpy(rng.random(R, dtype=np.float32) + 0.5).cuda()

    # ---- the call alone
    z = torch.from_numpy(rng.normal(0, 3, (R, ncls)).astype(np.float32)).cuda()
    sm, dl = torch.empty_like(z), torch.empty_like(z)
    scal, cs = torch.empty(2, device="cuda"), torch.empty((nseg, 2), device="cuda")
    offd = torch.from_numpy(off.astype(np.int32)).cuda()
    need = int(H.load().dgcnn_seg_softmax_xent_workspace_bytes(R, nseg))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def dense():
        H.memset(scal)
        H.call("dgcnn_softmax_xent_f32", z.data_ptr(), lab.data_ptr(), wgt.data_ptr(), R, ncls, sm.data_ptr(), dl.data_ptr(), scal.data_ptr())

    def per_cloud():
        H.call("dgcnn_seg_softmax_xent_f32", z.data_ptr(), lab.data_ptr(), wgt.data_ptr(), R, ncls, offd.data_ptr(), nseg, sm.data_ptr(),
               dl.data_ptr(), cs.data_ptr(), scal.data_ptr(), ws.data_ptr(), need)

    def step(lpc):
        flags.LOSS_PER_CLOUD = lpc
        tv.zero_gradients(None)
        return tv.accum_gradient(None, [pts], [lab], [wgt], offsets=[off])[2]

    loss = {True: float(step(True)), False: float(step(False))}
    t = {"dense": [], "cloud": [], "on": [], "off": []}
    for _ in range(args.rounds):
        t["dense"].append(1e3 * timed(dense, args.call_reps))
        t["cloud"].append(1e3 * timed(per_cloud, args.call_reps))
        t["off"].append(timed(lambda: step(False), args.reps))
        t["on"].append(timed(lambda: step(True), args.reps))
    prop = torch.cuda.get_device_properties(0)
    row = lambda name, v, unit: "%-62s %9.3f /%9.3f /%9.3f %s" % (name, min(v), float(np.median(v)), max(v), unit)
    lines = ["device: %s (%s, %d CUs), one GPU" % (prop.name or "AMD Instinct", getattr(prop, "gcnArchName", "?"), prop.multi_processor_count),
             "one tower: 24 clouds, N ~ U[1024, 8192] (rng 0), R = %d rows, %d classes, row weights; %d rounds alternating the variants; "
             "min / median / max of the rounds" % (R, ncls, args.rounds),
             "the call (%d back-to-back calls between HIP events: launch rate included), softmax and dlogits written:" % args.call_reps,
             row("  dgcnn_softmax_xent_f32 (zero fill + 1 launch)", t["dense"], "us"),
             row("  dgcnn_seg_softmax_xent_f32 (2 launches)", t["cloud"], "us"),
             "the step: zero_gradients + accum_gradient, configs[1]'s model, C = 4, eager launches, %s mode, dropout on, "
             "BN_PER_CLOUD_TRAIN; %d calls per round:" % ("deterministic" if E.DETERMINISTIC else "atomics", args.reps),
             row("  LOSS_PER_CLOUD off (mean over the tower's rows)", t["off"], "ms"),
             row("  LOSS_PER_CLOUD on (mean over the clouds of the per-cloud means)", t["on"], "ms"),
             "on / off %.4f (medians)" % (np.median(t["on"]) / np.median(t["off"])),
             "loss of the first step (dropout masks differ): flag on %.5f, off %.5f" % (loss[True], loss[False])]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()

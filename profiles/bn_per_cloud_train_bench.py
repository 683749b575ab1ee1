"""Training with per-cloud BatchNorm on a packed tower (flags.BN_PER_CLOUD_TRAIN): device time of zero_gradients + accum_gradient
for ONE tower of 24 clouds (N ~ U[1024, 8192], rng 0 -- the tower of profiles/bn_per_cloud_bench.py; BASELINE configs[1]'s model,
C = 4, eager launches, default deterministic mode) three ways, from HIP events around the whole sequence of calls after a
synchronise:

    tower-wide   one packed step, BatchNorm statistics over all R rows                (--pack_towers 1)
    per-cloud    one packed step, statistics of each row's own cloud, with backward   (--pack_towers 1 --bn_per_cloud_train 1)
    24 x mbs 1   the 24 one-cloud steps whose statistics the per-cloud step has (zero_gradients once, 24 accum_gradient)

The three are run alternating over several rounds; min / median / max of the rounds are reported.

    python profiles/bn_per_cloud_train_bench.py [--reps 5] [--rounds 5] [--out profiles/packed/bn_per_cloud_train.txt]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed", "bn_per_cloud_train.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bn_per_cloud_train_bench measures on the GPU"
    rng = np.random.default_rng(0)
    sizes = rng.integers(1024, 8193, 24)
    off = np.concatenate([[0], np.cumsum(sizes)])
    R = int(off[-1])
    flags = dgcnn.DGCNN_FLAGS(MODEL_NAME="dgcnn", EDGE_CONV_LAYERS=3, EDGE_CONV_FILTERS=[64, 64, 128], FC_LAYERS=2, FC_FILTERS=[512, 256],
                              NUM_CLASS=2, KVALUE=20, NUM_CHANNEL=4, TRAIN=True, SEED=1)
    tv = dgcnn.trainval(flags).initialize()
    pts = torch.from_numpy(rng.random((R, 4), dtype=np.float32)).cuda()
    lab = torch.from_numpy(rng.integers(0, 2, R).astype(np.int32)).cuda()
    clouds = [(pts[off[b]:off[b + 1]][None], lab[off[b]:off[b + 1]][None]) for b in range(len(sizes))]

    def packed(bpct):
        flags.BN_PER_CLOUD_TRAIN = bpct
        tv.zero_gradients(None)
        return tv.accum_gradient(None, [pts], [lab], offsets=[off])[2]

    def alone():
        flags.BN_PER_CLOUD_TRAIN = False
        tv.zero_gradients(None)
        return [tv.accum_gradient(None, [c], [l])[2] for c, l in clouds]

    loss = {"bpc": float(packed(True)), "wide": float(packed(False)), "one": float(sum(float(l) * n for l, n in zip(alone(), sizes)) / R)}
    t = {"wide": [], "bpc": [], "one": []}
    for _ in range(args.rounds):
        t["wide"].append(timed(lambda: packed(False), args.reps))
        t["bpc"].append(timed(lambda: packed(True), args.reps))
        t["one"].append(timed(alone, max(2, args.reps // 2)))
    prop = torch.cuda.get_device_properties(0)
    row = lambda name, v: "%-52s %8.3f /%8.3f /%8.3f" % (name, min(v), float(np.median(v)), max(v))
    lines = ["device: %s (%s, %d CUs), one GPU" % (prop.name or "AMD Instinct", getattr(prop, "gcnArchName", "?"), prop.multi_processor_count),
             "one training tower: 24 clouds, N ~ U[1024, 8192] (rng 0), R = %d rows; configs[1]'s model, C = 4, eager launches, %s mode, "
             "dropout on" % (R, "deterministic" if E.DETERMINISTIC else "atomics"),
             "zero_gradients + accum_gradient; %d rounds alternating the three, %d calls per round between HIP events; ms per tower as "
             "min / median / max of the rounds" % (args.rounds, args.reps),
             row("packed, BatchNorm over the tower", t["wide"]),
             row("packed, BatchNorm per cloud (BN_PER_CLOUD_TRAIN)", t["bpc"]),
             row("24 x mbs 1 (the statistics per-cloud trains with)", t["one"]),
             "per-cloud / tower-wide %.3f; per-cloud / 24 x mbs 1 %.3f (medians)" % (
                 np.median(t["bpc"]) / np.median(t["wide"]), np.median(t["bpc"]) / np.median(t["one"])),
             "loss of the first step (row mean; dropout masks differ between the three): per cloud %.5f, tower-wide %.5f, "
             "24 x mbs 1 weighted by n_b / R %.5f" % (loss["bpc"], loss["wide"], loss["one"])]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()

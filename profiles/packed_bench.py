"""Packed towers, k-NN only: one segmented search over a tower of 24 clouds (N ~ U[1024, 8192], seeded rng) against the same 24
clouds searched one dense call each, in the same kernel forms, for the layers of the default model (k = 20) and of the production
one (k = 40): layer 0 on raw coordinates (C = 4; cell grid off, then on for the dense calls, which is not segmented) and a later layer
on 64 features seeded with the previous layer's graph (append-form scan).  Device time from HIP events around the whole sequence of
calls, after a synchronise; the dense sequence includes its launch gaps.  Every packed result is checked against the dense ones.

Whole step: the same 24 clouds through trainval with BASELINE configs[1]'s model (3 EdgeConv (64, 64, 128), merged 1024, FC (512, 256),
2 classes, k = 20; C = 4 as a variable-N source delivers) -- ONE packed accum_gradient(offsets=...) against 24 `-mbs 1` calls, both
launched eagerly, default (deterministic) mode, same event timing.  The two compute different BatchNorm statistics (over the tower
/ over each cloud), so only the times are compared.

    python profiles/packed_bench.py [--reps 20] [--out profiles/packed/bench.txt]
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

from dgcnn import _engine as E, _hip as H      # noqa: E402


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


def whole_step(rng, sizes, off, reps):
    """One packed training micro-step against 24 one-cloud micro-steps on the same clouds (zero_gradients + accum_gradient; no Adam)."""
    import dgcnn
    R = int(off[-1])
    flags = dgcnn.DGCNN_FLAGS(MODEL_NAME="dgcnn", EDGE_CONV_LAYERS=3, EDGE_CONV_FILTERS=[64, 64, 128], FC_LAYERS=2, FC_FILTERS=[512, 256],
                              NUM_CLASS=2, KVALUE=20, NUM_CHANNEL=4, LEARNING_RATE=1e-3, TRAIN=True, SEED=1)
    tv = dgcnn.trainval(flags).initialize()
    pts = torch.from_numpy(rng.random((R, 4), dtype=np.float32)).cuda()
    lab = torch.from_numpy(rng.integers(0, 2, R).astype(np.int32)).cuda()
    clouds = [(pts[off[b]:off[b + 1]][None], lab[off[b]:off[b + 1]][None]) for b in range(len(sizes))]

    def packed():
        tv.zero_gradients(None)
        return tv.accum_gradient(None, [pts], [lab], offsets=[off])

    def dense():
        tv.zero_gradients(None)
        return [tv.accum_gradient(None, [p], [l]) for p, l in clouds]

    lp = float(packed()[2])
    ld = float(np.mean([float(r[2]) for r in dense()]))
    assert np.isfinite(lp) and np.isfinite(ld)
    tp, td = timed(packed, reps), timed(dense, reps)
    mode = "deterministic" if E.DETERMINISTIC else "atomics"
    return ["",
            "whole training micro-step (configs[1]'s model, C = 4, eager launches, %s mode, %d reps): zero_gradients + accum_gradient" % (mode, reps),
            "%-34s %12s %12s %8s" % ("", "packed ms", "24 x mbs 1", "ratio"),
            "%-34s %12.3f %12.3f %8.3f" % ("forward + backward, R = %d" % R, tp, td, tp / td),
            "(loss of the first step: packed %.4f, mean of the 24 clouds %.4f -- BatchNorm over the tower / over each cloud)" % (lp, ld)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed", "bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "packed_bench measures on the GPU"
    lib = H.load()
    rng = np.random.default_rng(0)
    sizes = rng.integers(1024, 8193, 24)
    off = np.concatenate([[0], np.cumsum(sizes)])
    R = int(off[-1])
    seg = E.Segments(off, R)
    prop = torch.cuda.get_device_properties(0)
    lines = ["device: %s (%s, %d CUs), one GPU" % (prop.name or "AMD Instinct", getattr(prop, "gcnArchName", "?"), prop.multi_processor_count),
             "clouds: 24, N ~ U[1024, 8192] (rng 0): R = %d rows, min %d, max %d" % (R, seg.min_n, seg.max_n),
             "%-34s %12s %12s %8s" % ("layer", "packed ms", "24 dense ms", "ratio")]
    x0 = torch.from_numpy(rng.random((R, 4), dtype=np.float32)).cuda()
    x1 = torch.from_numpy(np.maximum(rng.normal(size=(R, 64)), 0).astype(np.float32)).cuda()
    prev_grid = lib.dgcnn_knn_grid(0)
    try:
        for k in (20, 40):
            for grid in (0, 1):
                lib.dgcnn_knn_grid(grid)
                packed = lambda: E.knn(x0, 1, R, k, seg=seg)
                dense = lambda: [E.knn(x0[off[b]:off[b + 1]], 1, int(sizes[b]), k) for b in range(24)]
                pi = packed().reshape(R, k).cpu().numpy()
                di = np.concatenate([d.reshape(-1, k).cpu().numpy() + off[b] for b, d in enumerate(dense())])
                assert np.array_equal(pi, di), "layer 0, k=%d: packed != dense" % k
                tp, td = timed(packed, args.reps), timed(dense, args.reps)
                lines.append("%-34s %12.3f %12.3f %8.3f" % ("C=4  k=%d  (dense cell grid %s)" % (k, "on" if grid else "off"),
                                                            tp, td, tp / td))
            lib.dgcnn_knn_grid(0)
            sp = E.knn(x0, 1, R, k, seg=seg)
            sd = [E.knn(x0[off[b]:off[b + 1]], 1, int(sizes[b]), k) for b in range(24)]
            packed = lambda: E.knn(x1, 1, R, k, seed=sp, seg=seg)
            dense = lambda: [E.knn(x1[off[b]:off[b + 1]], 1, int(sizes[b]), k, seed=sd[b]) for b in range(24)]
            pi = packed().reshape(R, k).cpu().numpy()
            di = np.concatenate([d.reshape(-1, k).cpu().numpy() + off[b] for b, d in enumerate(dense())])
            assert np.array_equal(pi, di), "layer 1, k=%d: packed != dense" % k
            tp, td = timed(packed, args.reps), timed(dense, args.reps)
            lines.append("%-34s %12.3f %12.3f %8.3f" % ("C=64 k=%d  seeded (append scan)" % k, tp, td, tp / td))
    finally:
        lib.dgcnn_knn_grid(prev_grid)
    lines += whole_step(rng, sizes, off, max(2, args.reps // 4))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()

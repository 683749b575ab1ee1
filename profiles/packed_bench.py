"""Packed towers, k-NN only: one segmented search over a tower of 24 clouds (N ~ U[1024, 8192], seeded rng) against the same 24
clouds searched one dense call each, in the same kernel forms, for the layers of the default model (k = 20) and of the production
one (k = 40): layer 0 on raw coordinates (C = 4; cell grid off, then on for the dense calls, which is not segmented) and a later layer
on 64 features seeded with the previous layer's graph (append-form scan).  Device time from HIP events around the whole sequence of
calls, after a synchronise; the dense sequence includes its launch gaps.  Every packed result is checked against the dense ones.

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
    lines = ["clouds: 24, N ~ U[1024, 8192] (rng 0): R = %d rows, min %d, max %d" % (R, seg.min_n, seg.max_n),
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
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()

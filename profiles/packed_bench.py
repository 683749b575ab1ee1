"""Packed towers, k-NN only: one segmented search over a tower of 24 clouds (N ~ U[1024, 8192], seeded rng) against the same 24
clouds searched one dense call each, in the same kernel forms, for the layers of the default model (k = 20) and of the production
one (k = 40): layer 0 on raw coordinates (C = 4; cell grid off, then on by the library's rule for both sides) and a later layer on 64
features seeded with the previous layer's graph (append-form scan).  Device time from HIP events around the whole sequence of
calls, after a synchronise; the dense sequence includes its launch gaps.  Every packed result is checked against the dense ones.

Whole step: the same 24 clouds through trainval with BASELINE configs[1]'s model (3 EdgeConv (64, 64, 128), merged 1024, FC (512, 256),
2 classes, k = 20; C = 4 as a variable-N source delivers) -- ONE packed accum_gradient(offsets=...) against 24 `-mbs 1` calls, both
launched eagerly, default (deterministic) mode, same event timing.  The two compute different BatchNorm statistics (over the tower
/ over each cloud), so only the times are compared.

Cell grid on packed towers (--grid-out): one packed layer-0 call at C = 4, k = 20 and k = 40, the all-pairs scan with the histogram
bound (dgcnn_knn_grid(0)) against the per-cloud cell grid (dgcnn_knn_grid(2)), alternating in the same process over several rounds, on
three towers from fixed seeds: (a) the mix above, (b) 8 clouds N ~ U[8192, 32768], (c) one 65536-point cloud + 23 clouds N ~ U[512, 2048].
Per path the min / median / max of the rounds; the indices of the two paths are asserted equal; the last column says what the
library's default rule (mode 1: dgcnn_knn_seg_grid_use) picks for the tower.

Per-cloud mix (--mix-out): the same call on all of those towers in mode 1 with dgcnn_knn_seg_mix_min_n = T for T in MIX_T, next to the
scan, the all-grid call and the baseline (what mode 1 picks with the mix off), alternating in one process.

    python profiles/packed_bench.py --mix-out profiles/packed/mix_bench.txt --reps 10
    python profiles/packed_bench.py [--reps 20] [--out profiles/packed/bench.txt] [--grid-out profiles/packed/grid_bench.txt] [--grid-only]
                                   [--grid-sweep profiles/packed/grid_sweep.txt]   (more towers: where the two paths cross)
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


def grid_towers():
    r0, r1, r2 = np.random.default_rng(0), np.random.default_rng(1), np.random.default_rng(2)
    return [("a: 24 clouds N ~ U[1024, 8192]", r0.integers(1024, 8193, 24)),
            ("b: 8 clouds N ~ U[8192, 32768]", r1.integers(8192, 32769, 8)),
            ("c: 65536 + 23 clouds N ~ U[512, 2048]", np.concatenate([[65536], r2.integers(512, 2049, 23)]))]


def grid_sweep_towers():
    """Where the two paths cross: equal-sized clouds, a wider mix, and one large cloud among 23 small ones."""
    r = np.random.default_rng(3)
    tw = [("16 x %d" % n, np.full(16, n)) for n in (6144, 8192, 10240, 12288, 16384, 20480)]
    tw.append(("24 clouds U[4096,16384]", r.integers(4096, 16385, 24)))
    tw.append(("16384 + 23 U[512,2048]", np.concatenate([[16384], r.integers(512, 2049, 23)])))
    tw.append(("32768 + 23 U[512,2048]", np.concatenate([[32768], r.integers(512, 2049, 23)])))
    return tw


def grid_section(lib, reps, rounds=5, towers=None):
    """The packed raw-coordinate layer: all-pairs scan (grid mode 0) against the per-cloud cell grid (mode 2), alternating."""
    prop = torch.cuda.get_device_properties(0)
    lines = ["device: %s (%s, %d CUs), one GPU" % (prop.name or "AMD Instinct", getattr(prop, "gcnArchName", "?"), prop.multi_processor_count),
             "one packed layer-0 k-NN call, C = 4: all-pairs scan + histogram bound (dgcnn_knn_grid(0)) vs per-cloud cell grid (dgcnn_knn_grid(2)),",
             "%d rounds alternating the two, %d calls per round between HIP events; ms per call as min / median / max of the rounds" % (rounds, reps),
             "%-40s %4s %26s %26s %8s %s" % ("tower", "k", "all-pairs ms", "cell grid ms", "speedup", "verdict; rule (mode 1)")]
    prev = lib.dgcnn_knn_grid(0)
    try:
        for name, sizes in (towers or grid_towers()):
            off = np.concatenate([[0], np.cumsum(sizes)])
            R = int(off[-1])
            seg = E.Segments(off, R)
            s2 = int((sizes.astype(np.int64) ** 2).sum())
            x = torch.from_numpy(np.random.default_rng(R).random((R, 4), dtype=np.float32)).cuda()
            lines.append("%s: R = %d rows, min %d, max %d, row-weighted mean cloud size %.0f" % (name, R, seg.min_n, seg.max_n, s2 / R))
            for k in (20, 40):
                call = lambda: E.knn(x, 1, R, k, seg=seg)
                lib.dgcnn_knn_grid(1)
                rule = int(lib.dgcnn_knn_seg_grid_use(4, k, seg.nseg, R, seg.min_n, seg.max_n, s2))
                res, t = {}, {0: [], 2: []}
                for rd in range(rounds):
                    for mode in (0, 2):
                        lib.dgcnn_knn_grid(mode)
                        if rd == 0:
                            res[mode] = call().cpu().numpy()
                        t[mode].append(timed(call, reps))
                assert np.array_equal(res[0], res[2]), "%s, k=%d: cell grid != all-pairs scan" % (name, k)
                a, g = np.array(t[0]), np.array(t[2])
                verdict = "grid faster beyond the spread" if g.max() < a.min() else ("scan faster beyond the spread" if a.max() < g.min() else "within the spread")
                lines.append("%-40s %4d %8.3f /%8.3f /%8.3f %8.3f /%8.3f /%8.3f %8.2f %s; rule picks the %s" % (
                    "", k, a.min(), np.median(a), a.max(), g.min(), np.median(g), g.max(), np.median(a) / np.median(g), verdict,
                    "grid" if rule else "scan"))
    finally:
        lib.dgcnn_knn_grid(prev)
    return lines


MIX_T = (4096, 6144, 8192, 12288, 16384)


def mix_section(lib, reps, rounds=5):
    """The per-cloud mix (dgcnn_knn_seg_mix_f32 through knn_packed: mode 1 with dgcnn_knn_seg_mix_min_n = T) at every T of MIX_T against
    the scan (mode 0), the all-grid call (mode 2) and the baseline = whichever of the two mode 1 picks with the mix off (T = 0: the
    mean rule, dgcnn_knn_seg_grid_use), all alternating in one process."""
    prop = torch.cuda.get_device_properties(0)
    paths = ["scan", "grid"] + ["T=%d" % t for t in MIX_T]
    lines = ["device: %s (%s, %d CUs), one GPU" % (prop.name or "AMD Instinct", getattr(prop, "gcnArchName", "?"), prop.multi_processor_count),
             "one packed layer-0 k-NN call, C = 4: all-pairs scan (dgcnn_knn_grid(0)), all-grid (dgcnn_knn_grid(2)) and mode 1 with the per-cloud",
             "threshold dgcnn_knn_seg_mix_min_n = T (clouds of >= T points through the grid, the others through the scan, one call; [g/s] = clouds",
             "per class; a tower of one class issues the existing scan / all-grid call).  %d rounds alternating all paths, %d calls per round" % (rounds, reps),
             "between HIP events; ms per call as min / median / max of the rounds.  base = what mode 1 picks with the mix off (the mean rule).",
             "vs base: median(base) / median(path); + faster / - slower than base beyond the spread of the rounds (no overlap), = within it"]
    prev = lib.dgcnn_knn_grid(0)
    prev_t = lib.dgcnn_knn_seg_mix_min_n(0)
    verdicts = {t: [] for t in MIX_T}
    try:
        for name, sizes in grid_towers() + grid_sweep_towers():
            sizes = np.asarray(sizes)
            off = np.concatenate([[0], np.cumsum(sizes)])
            R = int(off[-1])
            seg = E.Segments(off, R)
            s2 = int((sizes.astype(np.int64) ** 2).sum())
            x = torch.from_numpy(np.random.default_rng(R).random((R, 4), dtype=np.float32)).cuda()
            lines.append("%s: R = %d rows, min %d, max %d, row-weighted mean cloud size %.0f" % (name, R, seg.min_n, seg.max_n, s2 / R))
            for k in (20, 40):
                call = lambda: E.knn(x, 1, R, k, seg=seg)
                lib.dgcnn_knn_grid(1)
                base = "grid" if lib.dgcnn_knn_seg_grid_use(4, k, seg.nseg, R, seg.min_n, seg.max_n, s2) else "scan"

                def setup(path):
                    lib.dgcnn_knn_grid(0 if path == "scan" else 2 if path == "grid" else 1)
                    lib.dgcnn_knn_seg_mix_min_n(int(path[2:]) if path.startswith("T=") else 0)
                res, t = {}, {p_: [] for p_ in paths}
                for rd in range(rounds):
                    for path in paths:
                        setup(path)
                        if rd == 0:
                            res[path] = call().cpu().numpy()
                        t[path].append(timed(call, reps))
                for path in paths[1:]:
                    assert np.array_equal(res["scan"], res[path]), "%s, k=%d: %s != all-pairs scan" % (name, k, path)
                b = np.array(t[base])
                for path in paths:
                    a = np.array(t[path])
                    v = "+" if a.max() < b.min() else ("-" if b.max() < a.min() else "=")
                    tag = ""
                    if path.startswith("T="):
                        T = int(path[2:])
                        g = int((sizes >= T).sum())
                        tag = "[%d/%d]" % (g, len(sizes) - g)
                        verdicts[T].append(v)
                    lines.append("%-6s k=%-3d %-8s %-8s %8.3f /%8.3f /%8.3f   vs base %5.2f %s%s" % (
                        "", k, path, tag, a.min(), np.median(a), a.max(), np.median(b) / np.median(a), v, "   <- base" if path == base else ""))
    finally:
        lib.dgcnn_knn_seg_mix_min_n(prev_t)
        lib.dgcnn_knn_grid(prev)
    lines.append("per T over all towers and k: faster / within the spread / slower than base")
    for T in MIX_T:
        lines.append("  T=%-6d %2d / %2d / %2d" % (T, verdicts[T].count("+"), verdicts[T].count("="), verdicts[T].count("-")))
    return lines


def write(path, lines):
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed", "bench.txt"))
    ap.add_argument("--grid-out", default=os.path.join(ROOT, "profiles", "packed", "grid_bench.txt"))
    ap.add_argument("--grid-only", action="store_true", help="only the cell-grid section")
    ap.add_argument("--grid-sweep", default=None, metavar="FILE",
                    help="also time the towers of grid_sweep_towers() (3 rounds) into FILE (profiles/packed/grid_sweep.txt)")
    ap.add_argument("--mix-out", default=None, metavar="FILE",
                    help="only the per-cloud mix of grid and scan at every threshold of MIX_T, into FILE (profiles/packed/mix_bench.txt)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "packed_bench measures on the GPU"
    lib = H.load()
    if args.mix_out:
        write(args.mix_out, mix_section(lib, args.reps))
        return
    write(args.grid_out, grid_section(lib, args.reps))
    if args.grid_sweep:
        write(args.grid_sweep, grid_section(lib, args.reps, rounds=3, towers=grid_sweep_towers()))
    if args.grid_only:
        return
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
                lines.append("%-34s %12.3f %12.3f %8.3f" % ("C=4  k=%d  (cell grid %s)" % (k, "by the rule" if grid else "off"),
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
    write(args.out, lines)


if __name__ == "__main__":
    main()

"""The channel-slab k-NN scan for wide rows (csrc/knn_wide.hip), per call, on one GPU:

  (24, 2048, C, 20) for C in {64, 128, 256, 512}; (8, 16384, 256, 40); the packed tower of 24 clouds N ~ U[1024, 8192] (rng 0) at C = 256.
  C = 64  with dgcnn_knn_wide_min_c(5)  against knn_mfma_kernel<64> (the default, unseeded): what re-staging the query operand costs.
  C = 128 with dgcnn_knn_wide_min_c(65) against knn_kernel<128> (the default): what a later change of the default would rest on.

A call is the library entry (sqnorm + scan).  Device time from HIP events around `reps` calls after a warm-up call and a synchronise;
where two forms exist they alternate in one process and their indices are asserted equal; 5 rounds, ms per call as min / median /
max of the rounds.  Achieved rate = 2 sum(n^2) C / median, against the 157.3 TFLOP/s fp32 matrix-pipe peak of the MI355X (the bound of
every shape here: at N = 2048 a block re-reads 2 N C floats from L2 for 2 * 64 N C flops).  Features are standard normal, seeded.

    python profiles/knn_wide_bench.py [--out profiles/knn_wide/bench.txt] [--rounds 5]
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

PEAK = 157.3e12


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


def features(rows, C, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((rows, C)).astype(np.float32)).cuda()


def measure(lib, call, forms, rounds, reps):
    """forms: [(name, wide_min_c)] -> {name: ms per call of every round}; the forms alternate, their indices are compared"""
    prev = lib.dgcnn_knn_wide_min_c(-1)
    t, res = {n: [] for n, _ in forms}, {}
    try:
        for rd in range(rounds):
            for name, min_c in forms:
                lib.dgcnn_knn_wide_min_c(min_c)
                if rd == 0:
                    res[name] = call().cpu()
                t[name].append(timed(call, reps))
    finally:
        lib.dgcnn_knn_wide_min_c(prev)
    first = forms[0][0]
    for name, _ in forms[1:]:
        assert torch.equal(res[first], res[name]), "%s != %s" % (name, first)
    return {n: np.array(v) for n, v in t.items()}


def row(shape, form, flops, a):
    med = float(np.median(a))
    return "%-30s %-34s %9.3f /%9.3f /%9.3f %7.1f%% %9.1f %7.1f%%" % (
        shape, form, a.min(), med, a.max(), 100 * (a.max() - a.min()) / med, flops / (med * 1e-3) / 1e12, 100 * flops / (med * 1e-3) / PEAK)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_wide", "bench.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "knn_wide_bench measures on the GPU"
    lib = H.load()
    assert lib.dgcnn_knn_wide_min_c(-1) == 129
    prop = torch.cuda.get_device_properties(0)
    lines = ["device: %s (%s, %d CUs), one GPU" % (prop.name or "AMD Instinct", getattr(prop, "gcnArchName", "?"), prop.multi_processor_count),
             "one k-NN call (sqnorm + scan), unseeded; %d rounds, the forms of a shape alternating; ms per call as min / median / max of the" % args.rounds,
             "rounds, spread = (max - min) / median; TFLOP/s = 2 sum(n^2) C / median; share of the 157.3 TFLOP/s fp32 matrix-pipe peak",
             "%-30s %-34s %31s %8s %9s %8s" % ("shape (B, N, C, k)", "form", "ms per call", "spread", "TFLOP/s", "of peak")]
    med = {}
    B, N, k = 24, 2048, 20
    for C, forms in ((64, [("knn_mfma_kernel<64> (default)", 129), ("knn_wide_kernel (min_c = 5)", 5)]),
                     (128, [("knn_kernel<128> (default)", 129), ("knn_wide_kernel (min_c = 65)", 65)]),
                     (256, [("knn_wide_kernel", 129)]), (512, [("knn_wide_kernel", 129)])):
        x = features(B * N, C, C)
        t = measure(lib, lambda: E.knn(x, B, N, k), forms, args.rounds, 20)
        for name, _ in forms:
            lines.append(row("(%d, %d, %d, %d)" % (B, N, C, k), name, 2.0 * B * N * N * C, t[name]))
            med[(C, name.split()[0].split("<")[0])] = float(np.median(t[name]))
        del x
    B2, N2, C2, k2 = 8, 16384, 256, 40
    x = features(B2 * N2, C2, 7)
    t = measure(lib, lambda: E.knn(x, B2, N2, k2), [("knn_wide_kernel", 129)], args.rounds, 3)
    lines.append(row("(%d, %d, %d, %d)" % (B2, N2, C2, k2), "knn_wide_kernel", 2.0 * B2 * N2 * N2 * C2, t["knn_wide_kernel"]))
    del x
    sizes = np.random.default_rng(0).integers(1024, 8193, 24)
    off = np.concatenate([[0], np.cumsum(sizes)])
    R = int(off[-1])
    seg = E.Segments(off, R)
    x = features(R, 256, 9)
    t = measure(lib, lambda: E.knn(x, 1, R, 20, seg=seg), [("knn_wide_kernel<PackedClouds>", 129)], args.rounds, 5)
    lines.append(row("packed 24 x U[1024,8192], 256, 20", "knn_wide_kernel<PackedClouds>", 2.0 * float((sizes.astype(np.float64) ** 2).sum()) * 256,
                     t["knn_wide_kernel<PackedClouds>"]))
    lines.append("  (R = %d rows, min %d, max %d; the grid is cdiv(max, 64) x 24 blocks, those past their cloud leave at once)" % (R, seg.min_n, seg.max_n))
    lines += ["",
              "C = 64: re-staging the query slab with every candidate tile costs %.2fx knn_mfma_kernel<64> (median over median)"
              % (med[(64, "knn_wide_kernel")] / med[(64, "knn_mfma_kernel")]),
              "C = 128: knn_wide_kernel takes %.2fx the time of knn_kernel<128> (the default stays knn_kernel<128>: DGCNN_KNN_WIDE_MIN_C)"
              % (med[(128, "knn_wide_kernel")] / med[(128, "knn_kernel")]),
              "slab scaling at (24, 2048, C, 20), ms per call per 64 channels: " + ", ".join(
                  "C = %d: %.3f" % (C, med[(C, "knn_wide_kernel")] / (C / 64)) for C in (64, 128, 256, 512)),
              "per-channel time at C = 256 relative to knn_mfma_kernel<64> at C = 64: %.2f"
              % ((med[(256, "knn_wide_kernel")] / 256) / (med[(64, "knn_mfma_kernel")] / 64))]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()

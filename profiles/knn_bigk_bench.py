"""The large-k k-NN scan (csrc/knn_bigk.hip), per call, on one GPU:

  (24, 2048, 64, k) and (8, 16384, 64, k) for k = 65, 128, 256, beside k = 64 at the same shapes, once through the default dispatch
  (knn_mfma_kernel<64, 64> at N = 2048, knn_bf16f_kernel<64> at N = 16384: the yardstick) and once through knn_bigk_kernel with
  dgcnn_knn_big_k_min(1), whose indices are asserted equal to the default's.

A call is the library entry (sqnorm + scan), unseeded.  Device time from HIP events around `reps` calls after a warm-up call and a
synchronise; the forms of one shape alternate in one process; 5 rounds, ms per call as min / median / max of the rounds, the spread
(max - min) / median, and ns per selected neighbour = median / (rows k).  Features are standard normal, seeded.

    python profiles/knn_bigk_bench.py [--out profiles/knn_bigk_times.txt] [--rounds 5]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_bigk_times.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "knn_bigk_bench measures on the GPU"
    lib = H.load()
    assert lib.dgcnn_knn_big_k_min(-1) == 65
    prop = torch.cuda.get_device_properties(0)
    lines = ["# %s, %d CUs; ms per call: min / median / max of %d rounds" % (prop.name, prop.multi_processor_count, args.rounds),
             "%-22s %-44s %9s /%9s /%9s %8s %12s" % ("(B, N, C, k)", "form", "min", "median", "max", "spread", "ns/neighbour")]
    for B, N, reps in ((24, 2048, 10), (8, 16384, 3)):
        x = torch.from_numpy(np.random.default_rng([B, N]).standard_normal((B * N, 64)).astype(np.float32)).cuda()
        forms = [(64, 65), (64, 1), (65, 65), (128, 65), (256, 65)]            # (k, big_k_min)
        t, res = {f: [] for f in forms}, {}
        try:
            for rd in range(args.rounds):
                for f in (forms if rd % 2 == 0 else forms[::-1]):              # alternating order
                    k, kmin = f
                    lib.dgcnn_knn_big_k_min(kmin)
                    call = lambda: E.knn(x, B, N, k)
                    if rd == 0:
                        res[f] = call().cpu()
                    t[f].append(timed(call, reps))
        finally:
            lib.dgcnn_knn_big_k_min(65)
        assert torch.equal(res[(64, 65)], res[(64, 1)]), "k = 64: the large-k scan differs from the default dispatch"
        assert torch.equal(res[(65, 65)][:, :, :64], res[(64, 65)]) and torch.equal(res[(256, 65)][:, :, :128], res[(128, 65)])
        for f in forms:
            k, kmin = f
            a = np.array(t[f])
            med = float(np.median(a))
            name = "knn_bigk_kernel" + (" (dgcnn_knn_big_k_min(1))" if kmin == 1 else "") if (k > 64 or kmin == 1) else \
                "default: " + ("knn_bf16f_kernel<64>" if N >= 8192 else "knn_mfma_kernel<64, 64>")
            lines.append("%-22s %-44s %9.3f /%9.3f /%9.3f %7.1f%% %12.2f" % ((B, N, 64, k), name, a.min(), med, a.max(),
                                                                            100 * (a.max() - a.min()) / med, med * 1e6 / (B * N * k)))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

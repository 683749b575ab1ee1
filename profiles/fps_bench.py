"""Times farthest point sampling (csrc/fps.hip, dgcnn_fps_f32) against the obvious torch composition on the same card, in the same
process, alternating the two: per step one (B, N) distance update `minimum(mind, ((x - x[s]) ** 2).sum(-1))` and one `argmax`, no host
synchronisation inside the chain.  Stand-alone; not part of bench.py.

    python profiles/fps_bench.py [--rounds 7] [--inner 3] [--out FILE]

Both paths get the same points and pre-allocated results.  Times are device events around back-to-back calls (`inner` of the new path,
one of the composition, whose chain is thousands of launches), per call; median [min, max] over the rounds.  us / step = the call's
time over the m dependent steps of a chain (the clouds of a call run side by side, one workgroup each); us / point = over all B m
selected points."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dynamic-gcnn_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

CASES = [(8, 8192, 2048, 3), (8, 2048, 512, 3), (1, 65536, 4096, 3)]      # (B, N, m, C); the last one takes the streaming form


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def stats(v):
    v = np.asarray(v)
    return float(np.median(v)), float(v.min()), float(v.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fps_bench.py measures on a GPU; none is visible")
    import dgcnn  # noqa: F401
    from dgcnn import _hip as H
    lib = H.load()
    lines = ["# %s, torch %s; %d rounds; ms per call: median [min, max]" % (torch.cuda.get_device_name(0), torch.__version__, args.rounds)]
    for B, N, m, C in CASES:
        g = torch.Generator(device="cuda").manual_seed(B + N + m)
        x = torch.rand((B, N, C), device="cuda", generator=g)
        idx = torch.empty((B, m), dtype=torch.int32, device="cuda")
        dist = torch.empty((B, m), device="cuda")
        nws = int(lib.dgcnn_fps_workspace_bytes(B * N, C, N))
        ws = torch.empty((max(nws, 16),), dtype=torch.uint8, device="cuda")
        form = "resident" if N <= lib.dgcnn_fps_resident_max_n(C) else "streaming"

        def new():
            H.call("dgcnn_fps_f32", x.data_ptr(), C, C, B, 0, 0, B * N, B * m, N, m, 0, idx.data_ptr(), dist.data_ptr(),
                   ws.data_ptr() if nws else 0, nws)

        ar = torch.arange(B, device="cuda")
        tidx = torch.empty((B, m), dtype=torch.int64, device="cuda")

        def composition():
            mind = torch.full((B, N), float("inf"), device="cuda")
            s = torch.zeros((B,), dtype=torch.int64, device="cuda")
            for j in range(m):
                tidx[:, j] = s
                mind = torch.minimum(mind, ((x - x[ar, s][:, None, :]) ** 2).sum(-1))
                s = mind.argmax(1)

        new()
        composition()
        torch.cuda.synchronize()
        differ = int((tidx != idx.long()).sum())
        t = {"new": [], "torch": []}
        for _ in range(args.rounds):
            t["new"].append(timed(new, args.inner))
            t["torch"].append(timed(composition, 1))
        n_, t_ = stats(t["new"]), stats(t["torch"])
        lines.append("case %d x (%d -> %d), C = %d, %s form: %d of %d indices differ from the composition's (its sum order and tie rule "
                     "are torch's)" % (B, N, m, C, form, differ, B * m))
        lines.append("  new %9.4f [%9.4f, %9.4f]   torch %9.4f [%9.4f, %9.4f]   new / torch %.4f   torch spread %.3f"
                     % (n_ + t_ + (n_[0] / t_[0], (t_[2] - t_[1]) / t_[0])))
        lines.append("  new %.3f us / step, %.4f us / point;   torch %.3f us / step, %.4f us / point"
                     % (1e3 * n_[0] / m, 1e3 * n_[0] / (B * m), 1e3 * t_[0] / m, 1e3 * t_[0] / (B * m)))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

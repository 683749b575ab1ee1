"""Times the feature interpolation between two point sets (csrc/interp.hip) against the torch composition on the same card, in the same
process, alternating the two: forward `(feat[idx] * a[..., None]).sum(-2)`, backward its autograd backward ((M, k, F) tensors written
and re-read, an accumulating index_put).  Stand-alone; not part of bench.py.

    python profiles/interp_bench.py [--rounds 20] [--inner 5] [--out FILE]

Both paths get the same graph (dgcnn.ops.k_nn between the two sets, not timed) and pre-allocated operands; the new path is the two C
entries (forward writing the weights; backward with its adjacency build, beta = 0).  Times are device events around `inner` back-to-back
calls, per call; median [min, max] over the rounds.  bytes = the compulsory operand and result bytes of the direction (workspace traffic
not counted); `copy` = a device copy moving the same number of bytes (half read, half written), timed in the same rounds."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dynamic-gcnn_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

CASES = [(8, 2048, 16384, 64), (8, 2048, 16384, 256), (1, 8192, 65536, 64)]      # (B, N candidates, M queries, F), k = 3
K = 3
EPS = 1e-16


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
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("interp_bench.py measures on a GPU; none is visible")
    import dgcnn
    from dgcnn import _hip as H
    lines = ["# %s, torch %s; k = %d, eps = %g; %d rounds x %d calls; ms per call: median [min, max]"
             % (torch.cuda.get_device_name(0), torch.__version__, K, EPS, args.rounds, args.inner)]
    for B, N, M, F in CASES:
        g = torch.Generator(device="cuda").manual_seed(B + N + F)
        pts = torch.rand((B, N, 3), device="cuda", generator=g)
        qry = torch.rand((B, M, 3), device="cuda", generator=g)
        feat = torch.randn((B * N, F), device="cuda", generator=g)
        dy = torch.randn((B * M, F), device="cuda", generator=g)
        idx, dist = dgcnn.ops.k_nn(pts, K, queries=qry, return_dist=True)
        Q, P = B * M, B * N
        y = torch.empty((Q, F), device="cuda")
        a = torch.empty((Q, K), device="cuda")
        dfeat = torch.empty((P, F), device="cuda")
        nws = int(H.load().dgcnn_interp_bwd_workspace_bytes(Q, P, K))
        ws = torch.empty((nws,), dtype=torch.uint8, device="cuda")

        def new_fwd():
            H.call("dgcnn_interp_f32", feat.data_ptr(), F, idx.data_ptr(), dist.data_ptr(), Q, P, M, N, K, F, EPS, a.data_ptr(),
                   y.data_ptr(), F)

        def new_both():
            new_fwd()
            H.call("dgcnn_interp_bwd_f32", dy.data_ptr(), F, idx.data_ptr(), a.data_ptr(), Q, P, M, N, K, F, dfeat.data_ptr(), F, 0,
                   ws.data_ptr(), nws)

        new_both()
        rows = (idx.long() + (torch.arange(B, device="cuda") * N)[:, None, None]).reshape(Q, K)
        at = a.clone()
        ft = feat.clone().requires_grad_(True)
        res = {}

        def torch_fwd():
            with torch.no_grad():
                res["y"] = (feat[rows] * at[..., None]).sum(-2)

        def torch_both():
            ft.grad = None
            out = (ft[rows] * at[..., None]).sum(-2)
            out.backward(dy)

        torch_fwd()
        torch_both()
        torch.cuda.synchronize()
        err_y = float((res["y"] - y).abs().max())
        err_d = float((ft.grad - dfeat).abs().max())
        bytes_f = 4.0 * (P * F + Q * F + 3 * Q * K)
        bytes_b = bytes_f + 4.0 * (Q * F + P * F + 2 * Q * K)
        cp = {}
        for name, nb in (("fwd", bytes_f), ("fwd+bwd", bytes_b)):
            n = int(nb // 8)
            cp[name] = (torch.empty(n, device="cuda"), torch.empty(n, device="cuda"))
        paths = {"fwd": (new_fwd, torch_fwd), "fwd+bwd": (new_both, torch_both)}
        t = {(d, w): [] for d in paths for w in ("new", "torch", "copy")}
        for d, (fn, ft_) in paths.items():
            for _ in range(3):
                fn(), ft_(), cp[d][1].copy_(cp[d][0])
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for d, (fn, ft_) in paths.items():
                t[(d, "new")].append(timed(fn, args.inner))
                t[(d, "torch")].append(timed(ft_, args.inner))
                t[(d, "copy")].append(timed(lambda: cp[d][1].copy_(cp[d][0]), args.inner))
        lines.append("case %d x (%d -> %d), F = %d: max |new - torch| y %.3g, dfeat %.3g"
                     % (B, N, M, F, err_y, err_d))
        for d, nb in (("fwd", bytes_f), ("fwd+bwd", bytes_b)):
            n_, t_, c_ = stats(t[(d, "new")]), stats(t[(d, "torch")]), stats(t[(d, "copy")])
            lines.append("  %-8s new %8.4f [%8.4f, %8.4f]   torch %8.4f [%8.4f, %8.4f]   new / torch %.3f   torch spread %.3f"
                         % ((d,) + n_ + t_ + (n_[0] / t_[0], (t_[2] - t_[1]) / t_[0])))
            lines.append("  %-8s %.1f MB compulsory: new %.0f GB/s, device copy of the same bytes %.0f GB/s (%8.4f ms), new / copy %.2f"
                         % ("", nb / 1e6, nb / n_[0] / 1e6, nb / c_[0] / 1e6, c_[0], n_[0] / c_[0]))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

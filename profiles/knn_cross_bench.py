"""k-NN between two point sets (csrc/knn_cross.hip: dgcnn_knn_cross_f32), per call, on one GPU -> profiles/knn_cross.txt.

timings (default mode; one process, HIP events, 5 rounds, median with the spread = (max - min) / median):
  1. cross against self at equal work: (24, 2048 -> 2048, C, 20) for C = 64 and 256, (8, 16384 -> 16384, 64, 20).  The cross entry
     gets distinct q and p buffers holding the same data, with and without dist; the yardstick is dgcnn_knn_f32 on the same points
     with the channel-slab scan forced (dgcnn_knn_wide_min_c(5)): the same staging, MFMAs and selection.  The observed ratio is
     printed next to three times the yardstick's own spread.  The indices are asserted equal.
  2. raw coordinates: (24, 2048 -> 2048, 3, 20) and the propagation shape (8, 65536 queries -> 8192 candidates, 3, k = 3): the
     16-channel slab against the same kernel with 64-channel slabs.  The library has no switch for the slab width; the 64-channel
     form is measured on the same points padded with zero channels to C = 20 (ld = 20), which selects it and changes no distance
     (asserted: same indices, same distance bits).  For the square shape also the self search in its default form (histogram bound +
     VALU scan): what a cell-grid / bounded cross search would be worth.
resources (--resources [--parent REV]; needs hipcc, no GPU): VGPRs, AGPRs, scratch, LDS and occupancy of every knn_cross_kernel
  instance, and of every knn_wide_kernel / knn_bigk_kernel instance in this tree and in revision REV (the last one before knn_scan.h
  changed), from hipcc -Rpass-analysis=kernel-resource-usage.
Each mode rewrites its own section of the output file and keeps the other.

    python profiles/knn_cross_bench.py [--out profiles/knn_cross.txt] [--rounds 5]
    python profiles/knn_cross_bench.py --resources --parent <revision before knn_scan.h changed>
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dynamic-gcnn_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

MARK = {"timings": "==== timings ====", "resources": "==== resources ===="}


def write_section(path, name, lines):
    """replace section `name` of the file, keep the other"""
    parts = {"timings": [], "resources": []}
    if os.path.exists(path):
        cur = None
        for ln in open(path).read().splitlines():
            hit = [n for n, m in MARK.items() if ln == m]
            if hit:
                cur = hit[0]
            elif cur:
                parts[cur].append(ln)
    parts[name] = list(lines)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        for n in ("timings", "resources"):
            if parts[n]:
                f.write("\n".join([MARK[n]] + parts[n]).rstrip("\n") + "\n\n")


# ---------------------------------------------------------------------------------------------------------------------
# timings
# ---------------------------------------------------------------------------------------------------------------------
def timed(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def measure(torch, forms, rounds, reps):
    """forms: [(name, call)] alternating within every round -> {name: ms per call of every round}"""
    t = {n: [] for n, _ in forms}
    for _ in range(rounds):
        for name, call in forms:
            t[name].append(timed(torch, call, reps))
    return {n: np.array(v) for n, v in t.items()}


def spread(a):
    return float((a.max() - a.min()) / np.median(a))


def row(shape, form, a):
    return "%-34s %-46s %9.3f /%9.3f /%9.3f %7.1f%%" % (shape, form, a.min(), float(np.median(a)), a.max(), 100 * spread(a))


def timings(args):
    import torch
    from dgcnn import _engine as E, _hip as H
    assert torch.cuda.is_available(), "the timings are measured on the GPU"
    lib = H.load()
    assert lib.dgcnn_knn_wide_min_c(-1) == 129
    prop = torch.cuda.get_device_properties(0)

    def feats(rows, C, seed):
        return torch.from_numpy(np.random.default_rng(seed).standard_normal((rows, C)).astype(np.float32)).cuda()

    def forced_wide(x, B, N, k):
        prev = lib.dgcnn_knn_wide_min_c(5)
        try:
            return E.knn(x, B, N, k)
        finally:
            lib.dgcnn_knn_wide_min_c(prev)

    lines = ["device: %s (%s, %d CUs), one GPU" % (prop.name or "AMD Instinct", getattr(prop, "gcnArchName", "?"), prop.multi_processor_count),
             "one library call (norms + scan); %d rounds, the forms of a shape alternating; ms per call as min / median / max of the rounds," % args.rounds,
             "spread = (max - min) / median",
             "%-34s %-46s %31s %8s" % ("shape (B, M -> N, C, k)", "form", "ms per call", "spread"),
             "-- 1. cross against self at equal work (yardstick: dgcnn_knn_f32 with dgcnn_knn_wide_min_c(5) = knn_wide_kernel)"]
    notes = []
    for (B, N, C, k, reps) in ((24, 2048, 64, 20, 20), (24, 2048, 256, 20, 10), (8, 16384, 64, 20, 3)):
        x = feats(B * N, C, C + N)
        q, p = x.clone(), x.clone()
        forms = [("dgcnn_knn_f32, knn_wide_kernel (yardstick)", lambda: forced_wide(x, B, N, k)),
                 ("dgcnn_knn_cross_f32, dist = NULL", lambda: E.knn_cross(q, p, B, N, N, k)),
                 ("dgcnn_knn_cross_f32, with dist", lambda: E.knn_cross(q, p, B, N, N, k, want_dist=True))]
        ref = forms[0][1]().cpu()
        assert torch.equal(forms[1][1]().cpu(), ref) and torch.equal(forms[2][1]()[0].cpu(), ref), "cross != self"
        t = measure(torch, forms, args.rounds, reps)
        shape = "(%d, %d -> %d, %d, %d)" % (B, N, N, C, k)
        for name, _ in forms:
            lines.append(row(shape, name, t[name]))
        y = t[forms[0][0]]
        notes.append("%s: cross / yardstick = %.3f (dist = NULL), %.3f (with dist); three times the yardstick's spread = %.3f"
                     % (shape, np.median(t[forms[1][0]]) / np.median(y), np.median(t[forms[2][0]]) / np.median(y), 3 * spread(y)))
        del x, q, p
    lines += notes
    lines.append("-- 2. raw coordinates: the 16-channel slab against the same kernel with 64-channel slabs (zero channels up to C = 20)")
    notes = []
    for (B, M, N, k, reps, with_self) in ((24, 2048, 2048, 20, 20, True), (8, 65536, 8192, 3, 5, False)):
        C = 3
        p = feats(B * N, C, 11)
        q = p.clone() if M == N else feats(B * M, C, 12)
        q20, p20 = torch.zeros((B * M, 20), device="cuda"), torch.zeros((B * N, 20), device="cuda")
        q20[:, :C], p20[:, :C] = q, p
        forms = [("knn_cross_kernel, 16-channel slab (C = 3)", lambda: E.knn_cross(q, p, B, M, N, k, want_dist=True)),
                 ("knn_cross_kernel, 64-channel slab (C = 20)", lambda: E.knn_cross(q20, p20, B, M, N, k, want_dist=True))]
        a, b = forms[0][1](), forms[1][1]()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), "zero channels changed a result"
        if with_self:
            forms.append(("dgcnn_knn_f32, default (hist bound + knn_kernel)", lambda: E.knn(p, B, N, k)))
            assert torch.equal(forms[2][1](), a[0]), "cross != self"
        del a, b
        t = measure(torch, forms, args.rounds, reps)
        shape = "(%d, %d -> %d, %d, %d)" % (B, M, N, C, k)
        for name, _ in forms:
            lines.append(row(shape, name, t[name]))
        m16, m64 = np.median(t[forms[0][0]]), np.median(t[forms[1][0]])
        note = "%s: 64-channel slab / 16-channel slab = %.2f" % (shape, m64 / m16)
        if with_self:
            note += "; cross (16-channel slab) / default self search = %.2f" % (m16 / np.median(t[forms[2][0]]))
        notes.append(note)
        del q, p, q20, p20
    lines += notes
    lines.append("(a VALU list scan on knn_kernel<4, KC>'s pattern for C <= 4 was not built: the cross search runs the matrix-pipe kernel at every width)")
    print("\n".join(lines))
    write_section(args.out, "timings", lines)


# ---------------------------------------------------------------------------------------------------------------------
# resources
# ---------------------------------------------------------------------------------------------------------------------
FIELDS = (("VGPRs", r"VGPRs: (\d+)"), ("AGPRs", r"AGPRs: (\d+)"), ("scratch B/lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
          ("LDS B/block", r"LDS Size \[bytes/block\]: (\d+)"), ("waves/SIMD", r"Occupancy \[waves/SIMD\]: (\d+)"))


def resource_usage(csrc, source, want):
    """{demangled kernel name: (figures in FIELDS' order)} of the kernels of csrc/source whose name starts with one of `want`"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--cuda-device-only", "-c", source, "-o",
           os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    err = subprocess.run(cmd, cwd=csrc, stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, text=True, check=True).stderr
    out, name = {}, None
    for ln in err.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], stdout=subprocess.PIPE, text=True).stdout.strip()
            name = re.sub(r"\(anonymous namespace\)::", "", name).split("(")[0].replace("void ", "")
            out[name] = {}
            continue
        for key, pat in FIELDS:
            m = re.search(pat, ln)
            if m and name:
                out[name][key] = int(m.group(1))
    return {n: tuple(v.get(k, -1) for k, _ in FIELDS) for n, v in out.items() if n.startswith(tuple(want))}


def resources(args):
    csrc = os.path.join(ROOT, "dynamic-gcnn_amd", "csrc")
    head = "%-72s" + " %14s" * len(FIELDS)
    lines = ["hipcc -O3 -ffp-contract=off --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage", "",
             "knn_cross_kernel<KC, VEC, SL, Clouds>", head % (("instance",) + tuple(k for k, _ in FIELDS))]
    for n, v in sorted(resource_usage(csrc, "knn_cross.hip", ["knn_cross_kernel"]).items()):
        lines.append(head % ((n,) + v))
    if args.parent:
        with tempfile.TemporaryDirectory() as tmp:
            tar = subprocess.run(["git", "-C", ROOT, "archive", args.parent, "dynamic-gcnn_amd/csrc", "include"], stdout=subprocess.PIPE, check=True)
            subprocess.run(["tar", "-x", "-C", tmp], input=tar.stdout, check=True)
            old_csrc = os.path.join(tmp, "dynamic-gcnn_amd", "csrc")
            lines += ["", "knn_wide_kernel / knn_bigk_kernel: this tree against %s (knn_scan.h gained CrossSlabStage, merge_lists and" % args.parent,
                      "merge_lists_write_dist; merge_lists_write now calls merge_lists)", head % (("instance",) + tuple(k for k, _ in FIELDS))]
            diff = 0
            for src, want in (("knn_wide.hip", ["knn_wide_kernel"]), ("knn_bigk.hip", ["knn_bigk_kernel"])):
                new, old = resource_usage(csrc, src, want), resource_usage(old_csrc, src, want)
                assert set(new) == set(old), set(new) ^ set(old)
                for n in sorted(new):
                    same = new[n] == old[n]
                    diff += 0 if same else 1
                    lines.append(head % ((n,) + new[n]) + ("   = before" if same else "   before: %s" % (old[n],)))
            lines.append("%d instances differ from %s" % (diff, args.parent))
    print("\n".join(lines))
    write_section(args.out, "resources", lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_cross.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--parent", default=None)
    args = ap.parse_args()
    (resources if args.resources else timings)(args)


if __name__ == "__main__":
    main()

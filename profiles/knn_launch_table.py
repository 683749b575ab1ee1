"""A fixed list of direct k-NN library calls that takes every branch of the host dispatch in knn.hip (both sides of every size
threshold, every A/B switch), each with its own workspace of exactly the size its query returns.  Run it under a kernel trace on two
builds (DGCNN_HIP_LIB selects the library) and compare the sequences of (kernel, grid, workgroup, LDS): all forms return the same
indices, so only the trace shows which kernels a call launched.  B <= 2, N <= 8192: well under a second of GPU time.
usage: knn_launch_table.py"""
import sys
sys.path.insert(0, __file__.rsplit("/", 2)[0] + "/dynamic-gcnn_amd")
import numpy as np, torch
from dgcnn import _hip as H

lib = H.load()
dev = torch.device("cuda:0")
rng = np.random.default_rng(0)
_x = {}


def cloud(rows, C, ldx):
    """(rows, C) view of a 16-byte aligned (rows, ldx) tensor: coordinates in [0, 1) for C <= 4, ReLU features otherwise"""
    if (rows, C, ldx) not in _x:
        a = rng.random((rows, ldx)) if C <= 4 else np.maximum(rng.normal(size=(rows, ldx)), 0)
        _x[rows, C, ldx] = torch.from_numpy(a.astype(np.float32)).to(dev)
    return _x[rows, C, ldx]


def run(name, nws, *args):
    """every entry ends (..., idx, ws, ws_bytes, stream)"""
    ws = torch.empty((int(nws),), dtype=torch.uint8, device=dev)
    rc = getattr(lib, name)(*args, ws.data_ptr(), int(nws), None)
    torch.cuda.synchronize()
    if rc != 0:
        raise SystemExit("%s: %d %s" % (name, rc, lib.dgcnn_last_error().decode()))


def dense(B, N, C, k, seeded=False, ldx=None):
    ldx = ldx or C
    x = cloud(B * N, C, ldx)
    idx = torch.empty((B, N, k), dtype=torch.int32, device=dev)
    nws = lib.dgcnn_knn_workspace_bytes(B, N, C, k)
    print("dense B=%d N=%d C=%d ldx=%d k=%d%s" % (B, N, C, ldx, k, " seeded" if seeded else ""), flush=True)
    run("dgcnn_knn_f32", nws, x.data_ptr(), B, N, C, ldx, k, idx.data_ptr())
    if seeded:                                 # the graph just computed seeds the same search
        out = torch.empty_like(idx)
        run("dgcnn_knn_seeded_f32", nws, x.data_ptr(), B, N, C, ldx, k, idx.data_ptr(), k, k, out.data_ptr())


def tower(sizes, C):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return cloud(int(off[-1]), C, 4 if C <= 4 else C), torch.from_numpy(off).to(dev), int(off[-1])


def packed(sizes, C, k, seeded=False):
    x, off, R = tower(sizes, C)
    idx = torch.empty((1, R, k), dtype=torch.int32, device=dev)
    nws = lib.dgcnn_knn_seg_workspace_bytes(R, max(sizes), C, k)
    print("packed %s C=%d k=%d%s" % (sizes, C, k, " seeded" if seeded else ""), flush=True)
    a = (x.data_ptr(), H.ld2(x), C, k, len(sizes), off.data_ptr(), R, min(sizes), max(sizes))
    run("dgcnn_knn_seg_f32", nws, *a, None, 0, 0, idx.data_ptr())
    if seeded:
        out = torch.empty_like(idx)
        run("dgcnn_knn_seg_f32", nws, *a, idx.data_ptr(), k, k, out.data_ptr())


def packed_grid(sizes, k):
    x, off, R = tower(sizes, 3)
    idx = torch.empty((1, R, k), dtype=torch.int32, device=dev)
    print("packed grid %s k=%d" % (sizes, k), flush=True)
    run("dgcnn_knn_seg_grid_f32", lib.dgcnn_knn_seg_grid_workspace_bytes(R, len(sizes)), x.data_ptr(), H.ld2(x), 3, k, len(sizes),
        off.data_ptr(), R, min(sizes), max(sizes), idx.data_ptr())


def packed_mix(sizes, T, k):
    x, off, R = tower(sizes, 3)
    idx = torch.empty((1, R, k), dtype=torch.int32, device=dev)
    grid, scan = [b for b, n in enumerate(sizes) if n >= T], [b for b, n in enumerate(sizes) if n < T]
    lst = torch.tensor(grid + scan, dtype=torch.int32).to(dev)
    print("packed mix %s T=%d k=%d" % (sizes, T, k), flush=True)
    run("dgcnn_knn_seg_mix_f32", lib.dgcnn_knn_seg_mix_workspace_bytes(R, len(grid)), x.data_ptr(), H.ld2(x), 3, k, len(sizes),
        off.data_ptr(), R, lst.data_ptr(), len(grid), max(sizes[b] for b in grid), min(sizes[b] for b in scan),
        max(sizes[b] for b in scan), idx.data_ptr())


class switch:
    """with switch("dgcnn_knn_hist", 4): ... -- the setter returns the previous value, which is put back on the way out"""
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        print("%s(%d)" % (self.name, self.value), flush=True)
        self.prev = getattr(lib, self.name)(self.value)

    def __exit__(self, *exc):
        getattr(lib, self.name)(self.prev)


def feature_layers():
    """16 < C <= 64: matrix-pipe scan | bf16 filter unseeded, both LX forms of the append scan (or what replaces it) seeded"""
    dense(2, 2048, 64, 20, seeded=True)
    dense(1, 4096, 64, 20, seeded=True)
    dense(1, 8192, 64, 20, seeded=True)


# raw coordinates: the scan with the histogram bound below N = 4096, the cell grid from there; the bound is off below N = 256
for N in (4095, 4096, 255, 256):
    dense(2, N, 3, 20)
for stride in (0, 1, 2, 4):                    # N >= 4 k stride holds at (1024, 20) for every stride, fails at (300, 64) for 2 and 4
    with switch("dgcnn_knn_hist", stride):
        dense(2, 1024, 3, 20)
        dense(2, 300, 3, 64)
dense(1, 4096, 3, 64)                          # k > 40: no grid
dense(2, 1024, 3, 8)
dense(2, 1024, 3, 40)
dense(2, 512, 4, 20)
dense(2, 1024, 16, 20)                         # vector loader
dense(2, 1024, 16, 20, ldx=17)                 # scalar loader
feature_layers()
for k in (8, 40, 64):
    dense(2, 2048, 64, k, seeded=True)
with switch("dgcnn_knn_append", 0):            # seeds then go to the list-keeping scans, from N = 4096
    feature_layers()
with switch("dgcnn_knn_append_products", 3):
    feature_layers()
dense(2, 2048, 32, 20, seeded=True)
dense(2, 2048, 16, 20, seeded=True)            # C = 16 has no append form: seeded from N = 4096 only
dense(1, 4096, 16, 20, seeded=True)
dense(1, 4096, 20, 20, seeded=True)            # the seed bound declines C = 20
dense(2, 512, 128, 64)
with switch("dgcnn_knn_force_valu", 1):
    dense(2, 1024, 64, 20, seeded=True)
    dense(2, 1024, 16, 20)
    dense(2, 1024, 3, 20)
    dense(1, 4096, 3, 20)
with switch("dgcnn_knn_bf16_filter", 0):
    dense(1, 8192, 64, 20)
    dense(2, 2048, 64, 20, seeded=True)
with switch("dgcnn_knn_bf16_filter", 1):
    dense(2, 2048, 64, 20)
# packed towers of unequal clouds
small, large = [100, 300, 200], [300, 700, 512]
packed(small, 3, 20)                           # smallest cloud under 256 points: no histogram bound
packed(large, 3, 20)
packed(large, 3, 64)                           # 300 < 4 * 64 * 2: the precondition fails
packed(large, 16, 20)
packed(large, 64, 20, seeded=True)
packed([8192, 1000], 64, 40, seeded=True)      # the N >= 8192 form of the append scan, chosen by the largest cloud
with switch("dgcnn_knn_append", 0):
    packed(large, 64, 20, seeded=True)
packed(large, 128, 20)
packed_grid(large, 20)
for k in (8, 20, 40):                          # the scan class's smallest cloud (300) takes the bound at k = 8 and 20, not at 40
    packed_mix([1200, 300, 2000, 500], 1000, k)
print("done", flush=True)

"""The exact cell-grid k-NN on packed towers (dgcnn_knn_seg_grid_f32, csrc/knn_grid.hip with PackedClouds; C <= 4, k <= 40): one
uniform grid per cloud, its cell count from the cloud's own size.  Every comparison is exact -- per cloud the indices are the C
oracle's k_nn of that cloud alone (oracle/knn_oracle.c) plus the cloud's first tower row -- on towers that mix cloud kinds chosen to
break a spatial search (ties, duplicates, flat axes, clouds far from the origin next to tiny and huge ones), so that a cloud reading
its neighbour's grid description or cell table shows up."""
import numpy as np
import pytest
import torch

from oracle import dgcnn_oracle as O
from gpu_helpers import dev, host, set_vars

pytestmark = pytest.mark.gpu

GRID_TAG = "knn_grid_*"
# the all-pairs scan closes the engine's tag; knn_hist_bound_kernel stands in front of it only where every cloud has the 256 points
# (and 4 k stride) the histogram bound needs -- the tag lists what the call launches (tests/test_gpu_knn_dispatch.py)
SCAN_TAG = "knn_kernel]"


@pytest.fixture()
def dg():
    import dgcnn
    from dgcnn import _engine as E
    dgcnn.reset()
    yield dgcnn
    E.DETERMINISTIC = E.DETERMINISTIC_ENV_DEFAULT
    dgcnn.reset()


def lib():
    from dgcnn import _hip as H
    return H.load()


def pack(clouds):
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    return np.concatenate(clouds, 0), off


def check_per_cloud(idx, clouds, off, k):
    """Every index inside the row's own cloud, and per cloud the oracle's k_nn of that cloud alone."""
    idx = idx.reshape(-1, k)
    for b, cl in enumerate(clouds):
        part = idx[off[b]:off[b + 1]]
        assert part.min() >= off[b] and part.max() < off[b + 1], "cloud %d (n = %d): an index outside the cloud" % (b, len(cl))
        np.testing.assert_array_equal(part, O.k_nn(cl[None], k)[0] + off[b], err_msg="cloud %d (n = %d)" % (b, len(cl)))


def cloud(kind, rng, n, C):
    if kind == "uniform":
        return rng.random((n, C), dtype=np.float32)
    if kind == "lattice":                                   # exact ties, duplicates
        return rng.integers(0, 12, (n, C)).astype(np.float32)
    if kind == "same":                                      # all points identical: every distance 0, ties decided by index
        return np.full((n, C), 0.25, np.float32)
    if kind == "line":                                      # two flat axes
        x = np.zeros((n, C), np.float32)
        x[:, 0] = rng.random(n)
        return x
    if kind == "plane":
        x = rng.random((n, C), dtype=np.float32)
        x[:, min(2, C - 1)] = 0.5
        return x
    if kind == "far":                                       # the margins of the stop rule swallow the bound
        return rng.random((n, C), dtype=np.float32) + np.float32(1000.0)
    if kind == "tiny":                                      # denormal squares
        return (rng.random((n, C)) * 1e-20).astype(np.float32)
    if kind == "huge":
        return (rng.random((n, C)) * 1e15).astype(np.float32)
    if kind == "cluster":                                   # tight cluster + distant outliers
        x = rng.normal(0, 0.01, (n, C)).astype(np.float32)
        m = max(1, n // 75)
        x[:m] += 50.0
        x[m:2 * m] -= 30.0
        return x
    if kind == "track":                                     # random walk: very uneven density
        return np.cumsum(rng.normal(0, 0.02, (n, C)), axis=0).astype(np.float32)
    raise ValueError(kind)


def seg_grid_call(x, off, C, k):
    """dgcnn_knn_seg_grid_f32 directly; idx is pre-filled with -1."""
    from dgcnn import _hip as H
    R, nseg = len(x), len(off) - 1
    sizes = np.diff(off)
    xd = dev(x)
    od = dev(off.astype(np.int32))
    idx = torch.full((R, k), -1, dtype=torch.int32, device="cuda")
    full = int(lib().dgcnn_knn_seg_grid_workspace_bytes(R, nseg))
    ws = torch.empty(full, dtype=torch.uint8, device="cuda")
    H.call("dgcnn_knn_seg_grid_f32", xd.data_ptr(), x.shape[1], C, k, nseg, od.data_ptr(), R, int(sizes.min()), int(sizes.max()),
           idx.data_ptr(), ws.data_ptr(), full)
    return idx


# ------------------------------------------------------------------------------------------------------
# 1. the C entry directly
# ------------------------------------------------------------------------------------------------------
SIZES = [20, 63, 64, 65, 255, 256, 257, 300, 777, 1500, 4500]
# the far cloud directly between the tiny and the huge one; the 4500-point cloud (past the dense search's LDS-copy limit; its G reaches
# GMAX at k = 8) is a track
TOWER_KINDS = ["uniform", "plane", "same", "line", "tiny", "far", "huge", "uniform", "cluster", "lattice", "track"]


@pytest.mark.parametrize("C,k", [(3, 20), (4, 20), (3, 8), (3, 40), (2, 20), (1, 8), (3, 1)])
def test_seg_grid_entry_equals_the_oracle_per_cloud(dg, C, k):
    """Both sides of the wave (64) and query-block (256) edges, n == k, ragged n, one cloud of 4500 points; clouds smaller than k are
    dropped for that k."""
    rng = np.random.default_rng(1000 * C + k)
    clouds = [cloud(kind, rng, n, C) for n, kind in zip(SIZES, TOWER_KINDS) if n >= k]
    x, off = pack(clouds)
    idx = host(seg_grid_call(x, off, C, k))
    check_per_cloud(idx, clouds, off, k)


# ------------------------------------------------------------------------------------------------------
# 2. no leak across clouds
# ------------------------------------------------------------------------------------------------------
def test_equal_clouds_side_by_side_do_not_leak(dg):
    """The same 700-point cloud three times in a row and the same lattice cloud twice: a row that looked into a neighbouring copy
    would find its own point there at distance 0."""
    rng = np.random.default_rng(5)
    a = cloud("uniform", rng, 700, 3)
    l = cloud("lattice", rng, 500, 3)
    clouds = [a, a.copy(), a.copy(), l, l.copy()]
    x, off = pack(clouds)
    idx = host(seg_grid_call(x, off, 3, 20))
    check_per_cloud(idx, clouds, off, 20)


# ------------------------------------------------------------------------------------------------------
# 3. single cloud
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [777, 5000])
def test_single_cloud_tower_equals_the_dense_search(dg, N):
    rng = np.random.default_rng(N)
    x = rng.random((1, N, 3), dtype=np.float32)
    prev = lib().dgcnn_knn_grid(2)
    try:
        packed = host(dg.ops.k_nn(dev(x[0]), 20, offsets=[0, N]))
        dense = host(dg.ops.k_nn(dev(x), 20))
    finally:
        lib().dgcnn_knn_grid(prev)
    np.testing.assert_array_equal(packed, dense)
    np.testing.assert_array_equal(dense, O.k_nn(x, 20))


# ------------------------------------------------------------------------------------------------------
# 4 / 5. the rule at work through ops
# ------------------------------------------------------------------------------------------------------
def tagged_k_nn(dg, xd, k, off):
    """(indices, the tags recorded by a Timer around the call)."""
    from dgcnn import _hip as H
    prev_t = H.TIMER
    H.TIMER = tm = H.Timer()
    try:
        idx = host(dg.ops.k_nn(xd, k, offsets=off))
    finally:
        H.TIMER = prev_t
    return idx, sorted(tm.summary())


def test_a_large_cloud_among_small_ones_takes_the_grid(dg):
    """Sizes [300, 20000, 64, 1100]: the row-weighted mean cloud size is ~18.7 k, so the default rule (mode 1) picks the grid.  The
    small clouds in full, 1024 seeded rows of the large one; with the grid off the same indices from the all-pairs scan."""
    rng = np.random.default_rng(20000)
    sizes, k = [300, 20000, 64, 1100], 20
    clouds = [rng.random((n, 3), dtype=np.float32) for n in sizes]
    x, off = pack(clouds)
    xd = dev(x)
    prev = lib().dgcnn_knn_grid(1)
    try:
        idx, tags = tagged_k_nn(dg, xd, k, off)
        lib().dgcnn_knn_grid(0)
        idx0, tags0 = tagged_k_nn(dg, xd, k, off)
    finally:
        lib().dgcnn_knn_grid(prev)
    assert len(tags) == 1 and GRID_TAG in tags[0], tags
    assert len(tags0) == 1 and SCAN_TAG in tags0[0] and GRID_TAG not in tags0[0], tags0
    flat = idx.reshape(-1, k)
    for b in (0, 2, 3):
        part = flat[off[b]:off[b + 1]]
        assert part.min() >= off[b] and part.max() < off[b + 1]
        np.testing.assert_array_equal(part, O.k_nn(clouds[b][None], k)[0] + off[b], err_msg="cloud %d" % b)
    rows = np.sort(rng.permutation(sizes[1])[:1024]).astype(np.int32)
    np.testing.assert_array_equal(flat[off[1] + rows], O.k_nn_rows(clouds[1], k, rows) + off[1])
    big = flat[off[1]:off[2]]
    assert big.min() >= off[1] and big.max() < off[2]
    np.testing.assert_array_equal(idx0, idx)


def test_small_clouds_keep_the_all_pairs_scan_unless_the_grid_is_forced(dg):
    rng = np.random.default_rng(3000)
    clouds = [rng.random((1000, 3), dtype=np.float32) for _ in range(3)]
    x, off = pack(clouds)
    xd = dev(x)
    prev = lib().dgcnn_knn_grid(1)
    try:
        idx1, tags1 = tagged_k_nn(dg, xd, 20, off)
        lib().dgcnn_knn_grid(2)
        idx2, tags2 = tagged_k_nn(dg, xd, 20, off)
    finally:
        lib().dgcnn_knn_grid(prev)
    assert len(tags1) == 1 and SCAN_TAG in tags1[0] and GRID_TAG not in tags1[0], tags1
    assert len(tags2) == 1 and GRID_TAG in tags2[0], tags2
    np.testing.assert_array_equal(idx1, idx2)
    check_per_cloud(idx2, clouds, off, 20)


# ------------------------------------------------------------------------------------------------------
# 6. errors, before any launch
# ------------------------------------------------------------------------------------------------------
def test_errors_leave_idx_untouched(dg):
    rng = np.random.default_rng(6)
    sizes = [39, 300, 81]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    R = int(off[-1])
    full = int(lib().dgcnn_knn_seg_grid_workspace_bytes(R, 3))
    from dgcnn import _hip as H
    for what, C, k, kw in (("C = 5", 5, 20, {}), ("k = 41", 3, 41, {}), ("k = 40 above the smallest cloud (39)", 3, 40, {}),
                           ("workspace one byte short", 3, 20, {"ws_bytes": full - 1})):
        x = rng.random((R, max(C, 3)), dtype=np.float32)
        xd, od = dev(x), dev(off.astype(np.int32))
        idx = torch.full((R, k), -1, dtype=torch.int32, device="cuda")
        ws = torch.empty(full, dtype=torch.uint8, device="cuda")
        with pytest.raises(ValueError):
            H.call("dgcnn_knn_seg_grid_f32", xd.data_ptr(), x.shape[1], C, k, 3, od.data_ptr(), R, 39, 300,
                   idx.data_ptr(), ws.data_ptr(), kw.get("ws_bytes", full))
        torch.cuda.synchronize()
        assert (host(idx) == -1).all(), what


# ------------------------------------------------------------------------------------------------------
# 7. end to end
# ------------------------------------------------------------------------------------------------------
def test_model_logits_do_not_depend_on_the_search(dg):
    """model.build(offsets=) in deterministic mode with the grid forced and with the grid off: the same layer-0 graph, the same
    kernels downstream, so the logits are equal bit for bit."""
    import dgcnn
    rng = np.random.default_rng(77)
    flags = dg.DGCNN_FLAGS(MODEL_NAME="dgcnn", EDGE_CONV_LAYERS=2, EDGE_CONV_FILTERS=[32, 64], KVALUE=8, NUM_CLASS=2, FC_LAYERS=2,
                           FC_FILTERS=[64, 32], TRAIN=False, NUM_CHANNEL=3, DETERMINISTIC=None)
    sizes = [257, 600, 64]
    pts, off = pack([rng.random((n, 3), dtype=np.float32) for n in sizes])
    params = O.init_params(flags, 3, seed=1)
    out = []
    prev = lib().dgcnn_knn_grid(2)
    try:
        for mode in (2, 0):
            lib().dgcnn_knn_grid(mode)
            dg.trainval(flags).initialize()
            set_vars(dg, params)
            out.append(host(dgcnn.build(dev(pts), flags, offsets=off)))
    finally:
        lib().dgcnn_knn_grid(prev)
    assert out[0].shape == (1, len(pts), 2) and np.isfinite(out[0]).all()
    np.testing.assert_array_equal(out[0], out[1])

"""Packed raw-coordinate k-NN with every cloud in the search that suits its own size (dgcnn_knn_seg_mix_f32: the cell grid for the clouds
of at least dgcnn_knn_seg_mix_min_n points, the all-pairs scan with the histogram bound for the others, both kernels instantiated with
ListedClouds and launched over their own class, in one call).  Every comparison is exact: per cloud the indices are the C oracle's
k_nn of that cloud alone (oracle/knn_oracle.c) plus the cloud's first tower row.  The towers interleave the two classes and mix cloud
kinds chosen to break a spatial search (the kinds of test_gpu_packed_grid.py), so that a cloud that read another slot's grid description,
cell table or bound shows up."""
import numpy as np
import pytest
import torch

from oracle import dgcnn_oracle as O
from gpu_helpers import dev, host, set_vars
from launch_trace import launches, assert_launched

pytestmark = pytest.mark.gpu

# the engine's tag lists the kernels the call launches: the two cell-grid kernels as one word; the all-pairs scan closes the list, with
# knn_hist_bound_kernel in front of it only where every scan cloud has the 256 points (and 4 k stride) the histogram bound needs
GRID_TAG = "knn_grid_*"
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


_ORACLE = {}


def oracle_knn(cl, k):
    """The oracle's k_nn of one cloud alone; computed once per (cloud, k) and shared by the tests (read only)."""
    key = (cl.shape, k, cl.tobytes())
    if key not in _ORACLE:
        r = O.k_nn(cl[None], k)[0]
        r.setflags(write=False)
        _ORACLE[key] = r
    return _ORACLE[key]


def check_per_cloud(idx, clouds, off, k):
    """No -1 left, every index inside the row's own cloud, and per cloud the oracle's k_nn of that cloud alone."""
    idx = idx.reshape(-1, k)
    assert (idx != -1).all(), "rows left unwritten: %s" % np.flatnonzero((idx == -1).any(1))[:8]
    for b, cl in enumerate(clouds):
        part = idx[off[b]:off[b + 1]]
        assert part.min() >= off[b] and part.max() < off[b + 1], "cloud %d (n = %d): an index outside the cloud" % (b, len(cl))
        np.testing.assert_array_equal(part, oracle_knn(cl, k) + off[b], err_msg="cloud %d (n = %d)" % (b, len(cl)))


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


def classes(off, T):
    """What Segments.mix makes of a tower, written out independently: (list, n_grid, grid_max_n, scan_min_n, scan_max_n)."""
    sizes = np.diff(off)
    grid = [b for b, n in enumerate(sizes) if n >= T]
    scan = [b for b, n in enumerate(sizes) if n < T]
    return (np.array(grid + scan, np.int32), len(grid), int(max(sizes[b] for b in grid)), int(min(sizes[b] for b in scan)),
            int(max(sizes[b] for b in scan)))


def seg_mix_call(x, off, C, k, T):
    """dgcnn_knn_seg_mix_f32 directly, the clouds of at least T points as the grid class; idx is pre-filled with -1.  The call is
    recorded (tests/launch_trace.py): both sub-searches must have run as their ListedClouds instances."""
    from dgcnn import _hip as H
    R, nseg = len(x), len(off) - 1
    lst, n_grid, gmax, smin, smax = classes(off, T)
    xd, od, ld = dev(x), dev(off.astype(np.int32)), dev(lst)
    idx = torch.full((R, k), -1, dtype=torch.int32, device="cuda")
    full = int(lib().dgcnn_knn_seg_mix_workspace_bytes(R, n_grid))
    ws = torch.empty(full, dtype=torch.uint8, device="cuda")
    with launches() as L:
        H.call("dgcnn_knn_seg_mix_f32", xd.data_ptr(), x.shape[1], C, k, nseg, od.data_ptr(), R, ld.data_ptr(), n_grid, gmax, smin, smax,
               idx.data_ptr(), ws.data_ptr(), full)
    kc = 8 if k <= 8 else 20 if k <= 20 else 40
    assert_launched(L, "knn_grid_build_kernel", ["ListedClouds"])
    assert_launched(L, "knn_grid_query_kernel", [kc, "true" if C == 4 else "false", "false", "ListedClouds"])
    assert_launched(L, "knn_kernel", [4, kc, "ListedClouds"])
    if smin >= 256 and smin >= 8 * k and lib().dgcnn_knn_hist(-1) == 2:      # every scan cloud can take the histogram bound
        assert_launched(L, "knn_hist_bound_kernel", [2, "ListedClouds"])
    return idx


# ------------------------------------------------------------------------------------------------------
# 1. the C entry directly
# ------------------------------------------------------------------------------------------------------
T0 = 256
# at threshold 256 the classes alternate from cloud to cloud (grid, scan, grid, ...); the first cloud is a grid cloud.  (The 257-point cloud
# at the end is a grid cloud as well: towers that END with a scan cloud are in test_class_edges.)
SIZES = [300, 20, 777, 63, 4500, 64, 256, 65, 1500, 255, 257]
# "far" between "tiny" and "huge"; one lattice and one all-same cloud in each class (grid: 777 lattice, 256 same; scan: 63 lattice,
# 64 same); the 4500-point cloud is a track
KINDS = ["uniform", "tiny", "lattice", "lattice", "track", "same", "same", "tiny", "far", "huge", "cluster"]
# the classes' positions swapped: the first cloud a scan cloud, the last a grid cloud
SIZES_SWAPPED = [40, 300, 20, 777, 64, 4500, 65, 256, 255, 1500, 100, 257]
KINDS_SWAPPED = ["tiny", "uniform", "lattice", "lattice", "same", "track", "plane", "same", "tiny", "far", "huge", "line"]
CK = [(3, 20), (4, 20), (3, 8), (3, 40), (2, 20), (1, 8), (3, 1)]


def tower(sizes, kinds, C, k, seed):
    rng = np.random.default_rng(seed)
    return [cloud(kind, rng, n, C) for n, kind in zip(sizes, kinds) if n >= k]


@pytest.mark.parametrize("C,k", CK)
def test_seg_mix_entry_equals_the_oracle_per_cloud(dg, C, k):
    """Grid and scan clouds interleaved, the first cloud a grid cloud; both sides of the wave (64) and query-block (256) edges and of
    the threshold; clouds smaller than k are dropped for that k."""
    clouds = tower(SIZES, KINDS, C, k, 1000 * C + k)
    x, off = pack(clouds)
    lst, n_grid = classes(off, T0)[:2]
    assert lst[0] == 0 and 0 < n_grid < len(clouds)
    check_per_cloud(host(seg_mix_call(x, off, C, k, T0)), clouds, off, k)


@pytest.mark.parametrize("C,k", CK)
def test_seg_mix_entry_with_the_classes_swapped(dg, C, k):
    """The first cloud a scan cloud, the last a grid cloud."""
    clouds = tower(SIZES_SWAPPED, KINDS_SWAPPED, C, k, 2000 * C + k)
    x, off = pack(clouds)
    sizes = np.diff(off)
    assert sizes[0] < T0 <= sizes[-1]
    check_per_cloud(host(seg_mix_call(x, off, C, k, T0)), clouds, off, k)


# ------------------------------------------------------------------------------------------------------
# 2. class edges
# ------------------------------------------------------------------------------------------------------
# The histogram bound runs when the smallest cloud of the SCAN class has at least 256 points and at least 4 k stride (stride 2 by default:
# 160 at k = 20, 320 at k = 40) -- csrc/knn.hip: knn_hist_stride; at threshold 256 every scan runs without it, at 1024 both ways.
@pytest.mark.parametrize("T,sizes,k,what", [
    (256, [255, 256, 257], 20, "T - 1, T, T + 1 side by side"),
    (1024, [1023, 1024, 1025], 20, "T - 1, T, T + 1 side by side, the scan with its histogram bound"),
    (256, [100, 200, 700, 90, 130], 20, "one grid cloud among scan clouds"),
    (256, [300, 700, 120, 450, 256], 20, "one scan cloud among grid clouds"),
    (256, [600, 20, 200, 300], 20, "a scan class whose smallest cloud has n == k"),
    (1024, [1100, 319, 700, 1024, 1000], 40, "the smallest scan cloud below 4 k stride = 320, next to clouds above it: no bound"),
    (1024, [1100, 320, 700, 1024, 1000], 40, "the smallest scan cloud at 4 k stride exactly: with the bound"),
    (1024, [700, 1100, 256, 300], 20, "the smallest scan cloud at 256 points: with the bound, a scan cloud first and last"),
])
def test_class_edges(dg, T, sizes, k, what):
    rng = np.random.default_rng(sum(sizes) + T)
    clouds = [cloud("uniform" if i % 2 == 0 else "cluster", rng, n, 3) for i, n in enumerate(sizes)]
    x, off = pack(clouds)
    check_per_cloud(host(seg_mix_call(x, off, 3, k, T)), clouds, off, k)


# ------------------------------------------------------------------------------------------------------
# 3. no leak across clouds or classes
# ------------------------------------------------------------------------------------------------------
def test_equal_clouds_of_both_classes_interleaved_do_not_leak(dg):
    """The same 700-point cloud twice (grid class) and the same 200-point lattice twice (scan class), [a, l, a, l]: a row that looked
    into the other copy would find its own point there at distance 0."""
    rng = np.random.default_rng(5)
    a = cloud("uniform", rng, 700, 3)
    l = cloud("lattice", rng, 200, 3)
    clouds = [a, l, a.copy(), l.copy()]
    x, off = pack(clouds)
    check_per_cloud(host(seg_mix_call(x, off, 3, 20, T0)), clouds, off, 20)


# ------------------------------------------------------------------------------------------------------
# 4. the same bits as both existing entries
# ------------------------------------------------------------------------------------------------------
def test_same_indices_as_the_scan_entry_and_the_grid_entry(dg):
    from dgcnn import _hip as H
    C, k = 3, 20
    clouds = tower(SIZES, KINDS, C, k, 1000 * C + k)
    x, off = pack(clouds)
    R, nseg = len(x), len(off) - 1
    sizes = np.diff(off)
    mix = host(seg_mix_call(x, off, C, k, T0))
    xd, od = dev(x), dev(off.astype(np.int32))
    scan = torch.full((R, k), -1, dtype=torch.int32, device="cuda")
    n = int(lib().dgcnn_knn_seg_workspace_bytes(R, int(sizes.max()), C, k))
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    H.call("dgcnn_knn_seg_f32", xd.data_ptr(), x.shape[1], C, k, nseg, od.data_ptr(), R, int(sizes.min()), int(sizes.max()), None, 0, 0,
           scan.data_ptr(), ws.data_ptr(), n)
    grid = torch.full((R, k), -1, dtype=torch.int32, device="cuda")
    n = int(lib().dgcnn_knn_seg_grid_workspace_bytes(R, nseg))
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    H.call("dgcnn_knn_seg_grid_f32", xd.data_ptr(), x.shape[1], C, k, nseg, od.data_ptr(), R, int(sizes.min()), int(sizes.max()),
           grid.data_ptr(), ws.data_ptr(), n)
    np.testing.assert_array_equal(mix, host(scan))
    np.testing.assert_array_equal(mix, host(grid))


# ------------------------------------------------------------------------------------------------------
# 5. the rule through ops
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


def is_mix(tags):
    return len(tags) == 1 and GRID_TAG in tags[0] and SCAN_TAG in tags[0]


def is_scan(tags):
    return len(tags) == 1 and SCAN_TAG in tags[0] and GRID_TAG not in tags[0]


def is_grid(tags):
    return len(tags) == 1 and GRID_TAG in tags[0] and "knn_kernel" not in tags[0]


def test_the_threshold_splits_a_tower_in_mode_1_only(dg):
    rng = np.random.default_rng(1024)
    k = 20
    clouds = [rng.random((n, 3), dtype=np.float32) for n in [300, 2000, 64, 1100]]
    x, off = pack(clouds)
    xd = dev(x)
    prev_mode = lib().dgcnn_knn_grid(1)
    prev_t = lib().dgcnn_knn_seg_mix_min_n(1024)
    try:
        idx, tags = tagged_k_nn(dg, xd, k, off)
        assert is_mix(tags), tags
        check_per_cloud(idx, clouds, off, k)
        lib().dgcnn_knn_seg_mix_min_n(0)
        idx0, tags0 = tagged_k_nn(dg, xd, k, off)
        assert is_scan(tags0), tags0                      # the mean rule: ~1.5 k candidates per row is far below its threshold
        np.testing.assert_array_equal(idx0, idx)
        lib().dgcnn_knn_seg_mix_min_n(1024)
        lib().dgcnn_knn_grid(0)
        idx_m0, tags_m0 = tagged_k_nn(dg, xd, k, off)
        assert is_scan(tags_m0), tags_m0
        lib().dgcnn_knn_grid(2)
        idx_m2, tags_m2 = tagged_k_nn(dg, xd, k, off)
        assert is_grid(tags_m2), tags_m2
        np.testing.assert_array_equal(idx_m0, idx)
        np.testing.assert_array_equal(idx_m2, idx)
    finally:
        lib().dgcnn_knn_seg_mix_min_n(prev_t)
        lib().dgcnn_knn_grid(prev_mode)


@pytest.mark.parametrize("n,grid", [(1000, False), (1100, True)])
def test_a_tower_of_one_class_issues_the_existing_call(dg, n, grid):
    rng = np.random.default_rng(n)
    clouds = [rng.random((n, 3), dtype=np.float32) for _ in range(3)]
    x, off = pack(clouds)
    prev_mode = lib().dgcnn_knn_grid(1)
    prev_t = lib().dgcnn_knn_seg_mix_min_n(1024)
    try:
        idx, tags = tagged_k_nn(dg, dev(x), 20, off)
    finally:
        lib().dgcnn_knn_seg_mix_min_n(prev_t)
        lib().dgcnn_knn_grid(prev_mode)
    assert is_grid(tags) if grid else is_scan(tags), tags
    check_per_cloud(idx, clouds, off, 20)


# ------------------------------------------------------------------------------------------------------
# 6. errors, before any launch
# ------------------------------------------------------------------------------------------------------
def test_errors_leave_idx_untouched(dg):
    from dgcnn import _hip as H
    rng = np.random.default_rng(6)
    sizes = [39, 300, 81]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    R = int(off[-1])
    lst = np.array([1, 0, 2], np.int32)                   # grid class: the 300-point cloud
    full = int(lib().dgcnn_knn_seg_mix_workspace_bytes(R, 1))
    big = int(lib().dgcnn_knn_seg_mix_workspace_bytes(R, 3))
    cases = (("C = 5", 5, 20, {}), ("k = 41", 3, 41, {}), ("k = 40 above the smallest cloud (39)", 3, 40, {}),
             ("n_grid = 0", 3, 20, {"n_grid": 0}), ("n_grid = nseg", 3, 20, {"n_grid": 3}),
             ("workspace one byte short", 3, 20, {"ws_bytes": full - 1}), ("misaligned workspace", 3, 20, {"shift": 4}))
    for what, C, k, kw in cases:
        x = rng.random((R, max(C, 3)), dtype=np.float32)
        xd, od, ld = dev(x), dev(off.astype(np.int32)), dev(lst)
        idx = torch.full((R, k), -1, dtype=torch.int32, device="cuda")
        ws = torch.empty(big + 16, dtype=torch.uint8, device="cuda")
        assert ws.data_ptr() % 16 == 0
        with pytest.raises(ValueError):
            H.call("dgcnn_knn_seg_mix_f32", xd.data_ptr(), x.shape[1], C, k, 3, od.data_ptr(), R, ld.data_ptr(), kw.get("n_grid", 1), 300,
                   39, 81, idx.data_ptr(), ws.data_ptr() + kw.get("shift", 0), kw.get("ws_bytes", big))
        torch.cuda.synchronize()
        assert (host(idx) == -1).all(), what


# ------------------------------------------------------------------------------------------------------
# 7. end to end
# ------------------------------------------------------------------------------------------------------
def test_model_logits_do_not_depend_on_the_split(dg):
    """model.build(offsets=) in deterministic mode with the tower split at 256 points (sizes [257, 600, 64]: two grid clouds, one scan
    cloud) and with the grid off: the same layer-0 graph, the same kernels downstream, so the logits are equal bit for bit."""
    import dgcnn
    from dgcnn import _hip as H
    rng = np.random.default_rng(77)
    flags = dg.DGCNN_FLAGS(MODEL_NAME="dgcnn", EDGE_CONV_LAYERS=2, EDGE_CONV_FILTERS=[32, 64], KVALUE=8, NUM_CLASS=2, FC_LAYERS=2,
                           FC_FILTERS=[64, 32], TRAIN=False, NUM_CHANNEL=3, DETERMINISTIC=None)
    sizes = [257, 600, 64]
    pts, off = pack([rng.random((n, 3), dtype=np.float32) for n in sizes])
    params = O.init_params(flags, 3, seed=1)
    out, tags = [], []
    prev_mode = lib().dgcnn_knn_grid(1)
    prev_t = lib().dgcnn_knn_seg_mix_min_n(256)
    try:
        for mode in (1, 0):
            lib().dgcnn_knn_grid(mode)
            dg.trainval(flags).initialize()
            set_vars(dg, params)
            prev_tm = H.TIMER
            H.TIMER = tm = H.Timer()
            try:
                out.append(host(dgcnn.build(dev(pts), flags, offsets=off)))
            finally:
                H.TIMER = prev_tm
            tags.append([t for t in tm.summary() if t.startswith("knn_seg_call<C4")])
    finally:
        lib().dgcnn_knn_seg_mix_min_n(prev_t)
        lib().dgcnn_knn_grid(prev_mode)
    assert is_mix(tags[0]) and is_scan(tags[1]), tags
    assert out[0].shape == (1, len(pts), 2) and np.isfinite(out[0]).all()
    np.testing.assert_array_equal(out[0], out[1])

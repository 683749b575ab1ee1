"""The large-k k-NN scan (csrc/knn_bigk.hip: knn_bigk_kernel<4 | 8 keys per lane, vector | scalar, DenseClouds | PackedClouds>;
64 < k <= 256 at every width, and smaller k under dgcnn_knn_big_k_min) against oracle/knn_oracle.c: EVERY row, bit for bit, no
tolerance.  Packed towers are compared cloud by cloud with offsets[b] added.  Before any comparison the host asserts that every index
lies inside the row's own cloud.

What the shapes cover (the kernel walks 64-candidate tiles x 64-channel slabs, 64 query rows per block; a row's buffer holds 256 keys
for k <= 128 and 512 above, and is cut back to its k smallest when it holds more than 192 / 448 at a tile boundary):
  k   65 96 127 128 129 192 255 256              both buffer sizes and their edges
  N   65 127 128 129 256 257 300 513 700         tile and row-block edges; N = k at k = 65, 128, 256 (every candidate is listed)
  C   1 3 4 5 16 63 64 65 128 129 192 260        slab edges, both s_i kernels; C % 4 != 0 takes the scalar loader
  B   1 3                                        batch base offsets
  loaders: contiguous rows, ld = C + 4 (float4-loadable where C % 4 == 0), ld = C + 1 (never float4-loadable), the views cut out of a
  buffer filled with 777.
Several compactions per row: normal clouds of 2048 points, and the descending line x_j = -j, on which every candidate of row N - 1 is
closer than all before it, so that row appends every candidate and compacts at the highest possible rate.

WHY THE NON-FINITE RUNS ARE SAFE.  These tests call k-NN entries only, which write idx and their own workspace; no graph reaches a
gather before the host has asserted that its indices lie inside the cloud.  No trip count or store address of the new kernel depends
on a value being finite (read from the code):
  knn_bigk_kernel      the step loop runs cdiv(N, 64) * cdiv(C, 64) + 1 times; loads come from rows clamped to [0, N) and channels
                       clamped to [0, C).  A distance is turned into a key (NaN first replaced by +inf) and only DECIDES whether the
                       lane appends (key < the row's bound key, row < N, j < N); the append position is the row's LDS count, at most
                       192 / 448 at the start of a tile plus the tile's 64 candidates: below the buffer's 256 / 512 keys whatever the
                       keys are.  The loop over the block's rows at a tile boundary runs 16 times per wave; the sort is a fixed
                       network; a compaction stores to the first k slots of the row's buffer and the row's two LDS words; the last
                       pass stores to the row's k output slots, each the low word of a key (a cloud-local j < N, since every buffer
                       ends with at least k real keys: nothing is dropped before k keys are known) plus the cloud's first row."""
import numpy as np
import pytest
import torch

from oracle import dgcnn_oracle as O
from gpu_helpers import dev, host, Guard
from launch_trace import launches, assert_launched
import knn_nonfinite as NF
from test_gpu_knn_adversarial import forced, unrelated

pytestmark = pytest.mark.gpu

_REF = {}
_FAILED = []                     # comparisons that failed in this process (tests/test_gpu_bigk_model.py looks here first)
EINVAL, EUNSUP = -1, -4
DEFAULT_BIG_K_MIN = 65

K_AXIS = (65, 96, 127, 128, 129, 192, 255, 256)
N_AXIS = (65, 127, 128, 129, 256, 257, 300, 513, 700)
C_AXIS = (1, 3, 4, 5, 16, 63, 64, 65, 128, 129, 192, 260)
LOADERS = ("contiguous", "ld+4", "ld+1")
# (N, k) pairs: every N, every k, N = k at k = 65, 128, 256; four of them per C, cycling
NK = ((65, 65), (127, 65), (128, 96), (129, 127), (256, 128), (257, 129), (300, 192), (513, 255), (700, 256), (128, 128), (256, 256),
      (300, 65), (513, 96), (700, 127), (257, 255), (256, 192))


def _dense_cases():
    out = []
    for ci, C in enumerate(C_AXIS):
        for q in range(4):
            N, k = NK[(4 * ci + q) % len(NK)]
            i = len(out)
            out.append((1 if i % 2 else 3, N, C, k, LOADERS[i % 3]))
    out.append((3, 129, 192, 65, "contiguous"))          # odd tile count x odd slab count for the double buffer, more than one cloud
    out.append((1, 700, 260, 256, "ld+1"))               # five slabs, the large buffer, the scalar loader
    return out


DENSE = _dense_cases()
assert len(DENSE) <= 60
for axis, col in ((C_AXIS, 2), (N_AXIS, 1), (K_AXIS, 3), ((1, 3), 0), (LOADERS, 4)):
    assert {c[col] for c in DENSE} == set(axis), (col, {c[col] for c in DENSE} ^ set(axis))
assert {(65, 65), (128, 128), (256, 256)} <= {(c[1], c[3]) for c in DENSE}
for C in C_AXIS:                                         # every width meets a float4-loadable and a scalar view where it can
    assert {c[4] for c in DENSE if c[2] == C} >= {"contiguous", "ld+1"}, C


def normal(B, N, C):
    key = ("normal", B, N, C)
    if key not in _REF:
        x = np.random.default_rng([B, N, C, 5]).standard_normal((B, N, C)).astype(np.float32)
        x.setflags(write=False)
        _REF[key] = x
    return _REF[key]


def oracle(x, k, key):
    key = ("knn", key, k)
    if key not in _REF:
        r = O.k_nn(x, k)
        r.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def view(x2d, loader):
    """x2d (R, C) on the device as the loader's kind of view; the buffer around it holds 777."""
    R, C = x2d.shape
    if loader == "contiguous":
        return dev(np.array(x2d, np.float32))
    buf = torch.full((R, C + (4 if loader == "ld+4" else 1)), 777.0, dtype=torch.float32, device="cuda")
    buf[:, :C] = dev(np.array(x2d, np.float32))
    return buf[:, :C]


def bigk_kernel(xd, k, clouds):
    """The instance a call on this view is for: knn_bigk_kernel<keys per lane, float4 loader, cloud map> (knn_bigk.hip:launch_knn_bigk)"""
    from dgcnn import _hip as H
    vec = H.ld2(xd) % 4 == 0 and xd.data_ptr() % 16 == 0 and xd.shape[1] % 4 == 0
    return ("knn_bigk_kernel", [4 if k <= 128 else 8, "true" if vec else "false", clouds])


def recorded(call, expect):
    """call() with its launches recorded: the expected kernel (name, leading template arguments) must be among them."""
    if expect is None:
        return call()
    with launches() as L:
        out = call()
    assert_launched(L, *expect)
    return out


def dense_knn(x, k, loader="contiguous", seed=None, expect="bigk"):
    """expect: "bigk" = the call must launch the knn_bigk_kernel instance of its shape; None = whatever the dispatch picks."""
    from dgcnn import _engine as E
    B, N, C = x.shape
    xd = view(x.reshape(B * N, C), loader)
    sd = None if seed is None else dev(np.array(seed, np.int32).reshape(B, N, -1))
    return host(recorded(lambda: E.knn(xd, B, N, k, seed=sd), bigk_kernel(xd, k, "DenseClouds") if expect == "bigk" else expect))


def same(got, want, lo, n, what):
    """Every index of got inside [lo, lo + n) (asserted first, on the host), then every row equal to the oracle's."""
    got = np.asarray(got).reshape(want.shape)
    out = ((got < lo) | (got >= lo + n)).any(-1)
    bad = (got != want).any(-1)
    if out.any() or bad.any():
        _FAILED.append(what)
        first = tuple(np.argwhere(out | bad)[0])
        raise AssertionError("%s: %d rows hold an index outside the cloud, %d of %d rows differ from the oracle; first row %s: %s vs %s"
                             % (what, int(out.sum()), int(bad.sum()), bad.size, first, got[first], want[first]))


# ------------------------------------------------------------------------------------------------------
# dense
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,C,k,loader", DENSE, ids=["B%d-N%d-C%d-k%d-%s" % c for c in DENSE])
def test_dense_covering_set(B, N, C, k, loader):
    from dgcnn import _hip as H
    x = normal(B, N, C)
    xd = view(x.reshape(B * N, C), loader)
    assert H.ld2(xd) == C + {"contiguous": 0, "ld+4": 4, "ld+1": 1}[loader]          # float4-loadable iff this is a multiple of 4
    same(dense_knn(x, k, loader), oracle(x, k, ("normal", B, N, C)), 0, N, "dense %s %s" % ((B, N, C, k), loader))


@pytest.mark.parametrize("k", (65, 256))
def test_a_normal_cloud_of_2048_points_compacts_several_times(k):
    x = normal(2, 2048, 64)
    same(dense_knn(x, k), oracle(x, k, ("normal", 2, 2048, 64)), 0, 2048, "normal (2, 2048, 64, %d)" % k)


@pytest.mark.parametrize("C", (1, 5))
@pytest.mark.parametrize("k", (65, 256))
def test_the_descending_line_appends_every_candidate(k, C):
    """x_j = -j (C = 5: padded with zeros): distances are exact integers below 2^24, and for row N - 1 every candidate is closer than
    all before it -- the row appends all 2048 and compacts as often as a row can."""
    N = 2048
    x = np.zeros((1, N, C), np.float32)
    x[0, :, 0] = -np.arange(N, dtype=np.float32)
    want = oracle(x, k, ("line", C))
    assert (want[0, N - 1] == N - 1 - np.arange(k)).all()
    for loader in ("contiguous", "ld+1"):
        same(dense_knn(x, k, loader), want, 0, N, "descending line C=%d k=%d %s" % (C, k, loader))


@pytest.mark.parametrize("C", (64, 260))
def test_ties_break_to_the_lower_index(C):
    """Integer-lattice features in [-2, 2], rows 100-149 copies of rows 0-49: exact distances, many equal, duplicates at distance 0."""
    N, k = 300, 65
    x = np.random.default_rng(7).integers(-2, 3, (1, N, C)).astype(np.float32)
    x[0, 100:150] = x[0, 0:50]
    want = oracle(x, k, ("lattice", C))
    assert (want[0, 100:150, 0] == np.arange(50)).all() and (want[0, 100:150, 1] == np.arange(100, 150)).all()   # the copy after the original
    for loader in LOADERS:
        same(dense_knn(x, k, loader), want, 0, N, "ties C=%d %s" % (C, loader))


def test_a_cloud_of_identical_rows_lists_the_lowest_indices():
    N, C, k = 600, 64, 200
    x = np.full((1, N, C), 0.37, np.float32)
    want = oracle(x, k, "identical")
    assert (want[0] == np.arange(k)).all()
    same(dense_knn(x, k), want, 0, N, "identical rows")


NF_SHAPES = ((300, 64, 65), (300, 5, 65), (700, 64, 130), (700, 192, 130), (600, 64, 256))
NONFINITE = [(f, N, C, k) for f in NF.FAMILIES for (N, C, k) in NF_SHAPES if NF._fits(f, N, C, k)]
assert len(NONFINITE) == 7 * 5 - 1 and ("hist_trap", 600, 64, 256) not in NONFINITE


@pytest.mark.parametrize("family,N,C,k", NONFINITE, ids=["%s-N%d-C%d-k%d" % c for c in NONFINITE])
def test_non_finite_input(family, N, C, k):
    for label, x in NF.variants(family, N, C, k):
        NF.properties(family, label, x, O.dist_matrix_f32(x), k)                 # the cloud is what its family's name says
        want = oracle(x[None], k, ("nf", family, label, N, C))
        for loader in ("contiguous", "ld+1"):
            same(dense_knn(np.asarray(x)[None], k, loader), want, 0, N, "family=%s (%s) %s %s" % (family, label, (N, C, k), loader))


# ------------------------------------------------------------------------------------------------------
# packed towers
# ------------------------------------------------------------------------------------------------------
def tower(sizes, C, k):
    """(x (R, C), offsets, [the oracle's lists of cloud b as tower rows])"""
    key = ("tower", sizes, C, k)
    if key not in _REF:
        clouds = [np.random.default_rng([b, n, C, 9]).standard_normal((n, C)).astype(np.float32) for b, n in enumerate(sizes)]
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        want = [(O.k_nn(c[None], k)[0] + off[b]).astype(np.int32) for b, c in enumerate(clouds)]
        _REF[key] = (np.concatenate(clouds, 0), off, want)
    return _REF[key]


def packed_knn(x, off, k, loader="contiguous", seed=None, expect="bigk"):
    from dgcnn import _engine as E
    R = len(x)
    sd = None if seed is None else dev(np.array(seed, np.int32).reshape(1, R, -1))
    xd = view(x, loader)
    return host(recorded(lambda: E.knn(xd, 1, R, k, seed=sd, seg=E.Segments(off, R)),
                         bigk_kernel(xd, k, "PackedClouds") if expect == "bigk" else expect)).reshape(R, k)


def check_tower(idx, off, want, what):
    for b, w in enumerate(want):
        same(idx[off[b]:off[b + 1]], w, int(off[b]), int(off[b + 1] - off[b]), "%s cloud=%d" % (what, b))


PACKED = [(sizes, C, k) for sizes, k in (((256, 65, 130, 700, 66), 65), ((300, 257, 513), 256)) for C in (3, 64, 192)]
assert min(PACKED[0][0]) == PACKED[0][2]                 # k = the smallest cloud


@pytest.mark.parametrize("sizes,C,k", PACKED, ids=["%s-C%d-k%d" % ("/".join(map(str, s)), C, k) for s, C, k in PACKED])
def test_packed_towers(sizes, C, k):
    x, off, want = tower(sizes, C, k)
    for loader in ("contiguous", "ld+1"):
        check_tower(packed_knn(x, off, k, loader), off, want, "packed %s C=%d k=%d %s" % (sizes, C, k, loader))


def test_a_one_cloud_tower_equals_the_dense_call():
    N, C, k = 300, 64, 65
    x = normal(1, N, C)
    dense = dense_knn(x, k)
    same(dense, oracle(x, k, ("normal", 1, N, C)), 0, N, "dense (1, %d, %d, %d)" % (N, C, k))
    np.testing.assert_array_equal(packed_knn(x[0], np.array([0, N], np.int64), k), dense[0])


# ------------------------------------------------------------------------------------------------------
# seeds are accepted and ignored
# ------------------------------------------------------------------------------------------------------
def test_seeds_do_not_matter_dense():
    B, N, C, k = 1, 300, 64, 65
    x = normal(B, N, C)
    want = oracle(x, k, ("normal", B, N, C))
    plain = dense_knn(x, k)
    same(plain, want, 0, N, "unseeded")
    with forced(seed_min_n=0):
        for name, sd in (("own graph reversed", want[:, :, ::-1]), ("graph of unrelated features", unrelated(N, k)[None])):
            got = dense_knn(x, k, seed=sd)
            same(got, want, 0, N, "seeded k=65, seeds=%s" % name)
            np.testing.assert_array_equal(got, plain)


def test_seeds_do_not_matter_packed():
    sizes, C, k = (256, 65, 130, 700, 66), 64, 65
    x, off, want = tower(sizes, C, k)
    plain = packed_knn(x, off, k)
    check_tower(plain, off, want, "packed unseeded")
    other = np.concatenate([unrelated(int(n), k) + off[b] for b, n in enumerate(sizes)], 0).astype(np.int32)
    with forced(seed_min_n=0):
        got = packed_knn(x, off, k, seed=other)
        check_tower(got, off, want, "packed seeded k=65, seeds=graph of unrelated features")
        np.testing.assert_array_equal(got, plain)


# ------------------------------------------------------------------------------------------------------
# the switch
# ------------------------------------------------------------------------------------------------------
SWITCH = [(C, N) for C in (3, 16, 64, 128, 192) for N in (65, 200)]


@pytest.mark.parametrize("C,N", SWITCH, ids=["C%d-N%d" % c for c in SWITCH])
def test_the_switch_sends_small_k_to_the_large_k_scan(C, N):
    """The default dispatch and dgcnn_knn_big_k_min(1) differ in the kernel only, never in the indices."""
    from dgcnn import _engine as E
    from dgcnn import _hip as H
    B = 2
    x = normal(B, N, C)
    for k in (1, 8, 20, 40, 64):
        want = oracle(x, k, ("normal", B, N, C))
        assert H.load().dgcnn_knn_big_k_min(-1) == DEFAULT_BIG_K_MIN and not E._knn_big(k)
        default = dense_knn(x, k, expect=None)                # the small-k kernels: what the switch is held against
        same(default, want, 0, N, "default path %s" % ((B, N, C, k),))
        with forced(big_k_min=1) as lib:
            assert lib.dgcnn_knn_big_k_min(-1) == 1 and E._knn_big(k)
            for loader in ("contiguous", "ld+1"):
                got = dense_knn(x, k, loader)
                same(got, want, 0, N, "big_k_min=1 %s %s" % ((B, N, C, k), loader))
                np.testing.assert_array_equal(got, default)
            R = B * N                                                # the same rows as one packed tower of B clouds
            off = np.arange(B + 1, dtype=np.int64) * N
            tw = [(want[b] + off[b]).astype(np.int32) for b in range(B)]
            check_tower(packed_knn(x.reshape(R, C), off, k), off, tw, "big_k_min=1 packed %s" % ((B, N, C, k),))
        assert H.load().dgcnn_knn_big_k_min(-1) == DEFAULT_BIG_K_MIN


# ------------------------------------------------------------------------------------------------------
# arguments
# ------------------------------------------------------------------------------------------------------
def _guarded_call(B, N, C, k, ws_short=0):
    """dgcnn_knn_f32 on guarded buffers -> (status, guard, idx view)"""
    from dgcnn import _hip as H
    lib = H.load()
    g = Guard()
    x = g.put(np.random.default_rng(1).standard_normal((B * N, C)).astype(np.float32))
    idx = g.new((B, N, k), torch.int32, fill=777)
    need = int(lib.dgcnn_knn_workspace_bytes(B, N, C, k))
    ws = g.new((need - ws_short,), torch.uint8, fill=77)
    rc = lib.dgcnn_knn_f32(x.data_ptr(), B, N, C, C, k, idx.data_ptr(), ws.data_ptr(), need - ws_short, H._stream())
    return rc, g, idx, ws


def _untouched(g, idx, ws):
    g.check()
    assert (host(idx) == 777).all() and (host(ws) == 77).all(), "a refused call wrote to its buffers"


def test_k_above_256_is_unsupported():
    rc, g, idx, ws = _guarded_call(1, 300, 64, 257)
    assert rc == EUNSUP
    _untouched(g, idx, ws)


def test_force_valu_refuses_large_k():
    with forced(force_valu=1):
        rc, g, idx, ws = _guarded_call(1, 100, 64, 65)
    assert rc == EUNSUP
    _untouched(g, idx, ws)


def test_a_workspace_one_byte_short_is_refused():
    rc, g, idx, ws = _guarded_call(2, 100, 64, 65, ws_short=1)
    assert rc == EINVAL
    _untouched(g, idx, ws)
    rc, g, idx, ws = _guarded_call(2, 100, 64, 65)             # and the full one runs, inside its buffers
    assert rc == 0
    g.check()
    assert (host(idx) >= 0).all() and (host(idx) < 100).all()


def test_the_packed_entry_refuses_the_same():
    from dgcnn import _hip as H
    lib = H.load()
    g = Guard()
    R, C = 600, 64
    off = g.put(np.array([0, 300, 600], np.int32))
    x = g.put(np.random.default_rng(2).standard_normal((R, C)).astype(np.float32))
    for k, valu, short, code in ((257, 0, 0, EUNSUP), (65, 1, 0, EUNSUP), (65, 0, 1, EINVAL)):
        idx = g.new((R, k), torch.int32, fill=777)
        need = int(lib.dgcnn_knn_seg_workspace_bytes(R, 300, C, k))
        ws = g.new((need - short,), torch.uint8, fill=77)
        with forced(force_valu=valu):
            rc = lib.dgcnn_knn_seg_f32(x.data_ptr(), C, C, k, 2, off.data_ptr(), R, 300, 300, None, 0, 0, idx.data_ptr(), ws.data_ptr(),
                                       need - short, H._stream())
        assert rc == code, (k, valu, short, rc)
        _untouched(g, idx, ws)


# ------------------------------------------------------------------------------------------------------
# repeatability
# ------------------------------------------------------------------------------------------------------
def test_two_calls_are_bit_identical():
    x = normal(3, 700, 64)
    a, b = dense_knn(x, 130), dense_knn(x, 130)
    np.testing.assert_array_equal(a, b)
    same(a, oracle(x, 130, ("normal", 3, 700, 64)), 0, 700, "repeatability (3, 700, 64, 130)")

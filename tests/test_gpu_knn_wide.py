"""The channel-slab k-NN scan for wide feature rows (csrc/knn_wide.hip: sqnorm_wide_kernel, knn_wide_kernel<KC, vector | scalar,
DenseClouds | PackedClouds>; 128 < C <= 1024, and narrower rows under dgcnn_knn_wide_min_c) against oracle/knn_oracle.c: EVERY row,
bit for bit, no tolerance.  Packed towers are compared cloud by cloud with offsets[b] added.  Before any comparison the host asserts
that every index lies inside the row's own cloud.

What the shapes cover (the kernel walks 64-candidate tiles x 64-channel slabs, double buffered over the flattened sequence, 64 query
rows per block, lists of KC in {8, 20, 40, 64}):
  C   129 130 132 191 192 193 256 260 512 1024   slab edges; C % 4 != 0 takes the scalar loader
  N   1 63 64 65 127 128 129 200                 tile and row-block edges; N = 129 x C = 192: odd tile count x odd slab count
  k   1 8 9 20 21 40 41 64                       the KC ladder, k = N at N = 1 and N = 64
  B   1 3                                        batch base offsets
  loaders: contiguous rows, ld = C + 4 (float4-loadable where C % 4 == 0), ld = C + 1 (never float4-loadable), the views cut out of a
  buffer filled with 777.

WHY THE NON-FINITE RUNS ARE SAFE.  These tests call k-NN entries only, which write idx and their own workspace; no graph reaches a
gather before the host has asserted that its indices lie inside the cloud.  No trip count or store address of the new kernels depends
on a value being finite (read from the code):
  sqnorm_wide_kernel   loops over the chunks of C and the block's rows; a thread stores s to its own row's slot.
  knn_wide_kernel      the step loop runs cdiv(N, 64) * cdiv(C, 64) times; loads come from rows clamped to [0, N) and channels clamped
                       to [0, C); a distance only sets bits of an 8-bit mask (d < thr is false for NaN and +inf: NaN counts as +inf
                       and is never listed), the drain pops one bit per trip and indexes the parked distances by the bit's number; the
                       merge walks KC entries; fill_short_list (knn_common.h) runs v < N and c < k and stores to out[c] only; the
                       indices written are list entries below N or the fill's v < N, plus the cloud's first row."""
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
_FAILED = []                     # comparisons that failed in this process (tests/test_gpu_wide_model.py looks here first)
EINVAL, EUNSUP = -1, -4
DEFAULT_MIN_C = 129

C_AXIS = (129, 130, 132, 191, 192, 193, 256, 260, 512, 1024)
N_AXIS = (1, 63, 64, 65, 127, 128, 129, 200)
K_AXIS = (1, 8, 9, 20, 21, 40, 41, 64)
LOADERS = ("contiguous", "ld+4", "ld+1")
# (N, k) pairs: every N, every k, k = N at N = 1 and N = 64; five of them per C, cycling
NK = ((1, 1), (63, 8), (64, 64), (65, 9), (127, 20), (128, 21), (129, 40), (200, 41), (200, 64), (63, 40), (65, 64), (127, 1),
      (128, 9), (129, 8), (200, 20), (64, 21))


def _dense_cases():
    out = []
    for ci, C in enumerate(C_AXIS):
        for q in range(5):
            N, k = NK[(5 * ci + q) % len(NK)]
            i = len(out)
            out.append((1 if i % 2 else 3, N, C, k, LOADERS[i % 3]))
    out.append((3, 129, 192, 20, "contiguous"))          # odd tile count x odd slab count for the double buffer, more than one cloud
    out.append((1, 200, 1024, 64, "ld+1"))               # sixteen slabs, the longest lists, the scalar loader
    return out


DENSE = _dense_cases()
assert len(DENSE) <= 60
for axis, col in ((C_AXIS, 2), (N_AXIS, 1), (K_AXIS, 3), ((1, 3), 0), (LOADERS, 4)):
    assert {c[col] for c in DENSE} == set(axis), (col, {c[col] for c in DENSE} ^ set(axis))
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


def wide_kernel(xd, k, clouds):
    """The instance a call on this view is for: knn_wide_kernel<KC, float4 loader, cloud map> (knn_wide.hip:launch_knn_wide)"""
    from dgcnn import _hip as H
    kc = 8 if k <= 8 else 20 if k <= 20 else 40 if k <= 40 else 64
    vec = H.ld2(xd) % 4 == 0 and xd.data_ptr() % 16 == 0 and xd.shape[1] % 4 == 0
    return ("knn_wide_kernel", [kc, "true" if vec else "false", clouds])


def recorded(call, expect):
    """call() with its launches recorded: the expected kernel (name, leading template arguments) must be among them."""
    if expect is None:
        return call()
    with launches() as L:
        out = call()
    assert_launched(L, *expect)
    return out


def dense_knn(x, k, loader="contiguous", seed=None, expect="wide"):
    """expect: "wide" = the call must launch the knn_wide_kernel instance of its shape; None = whatever the dispatch picks."""
    from dgcnn import _engine as E
    B, N, C = x.shape
    xd = view(x.reshape(B * N, C), loader)
    sd = None if seed is None else dev(np.array(seed, np.int32).reshape(B, N, -1))
    return host(recorded(lambda: E.knn(xd, B, N, k, seed=sd), wide_kernel(xd, k, "DenseClouds") if expect == "wide" else expect))


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


def test_ties_break_to_the_lower_index():
    """Integer-lattice features in [-2, 2], rows 100-149 copies of rows 0-49: exact distances, many equal, duplicates at distance 0."""
    N, C, k = 200, 260, 8
    x = np.random.default_rng(7).integers(-2, 3, (1, N, C)).astype(np.float32)
    x[0, 100:150] = x[0, 0:50]
    want = oracle(x, k, "lattice")
    assert (want[0, 100:150, 0] == np.arange(50)).all() and (want[0, 100:150, 1] == np.arange(100, 150)).all()   # the copy after the original
    for loader in LOADERS:
        same(dense_knn(x, k, loader), want, 0, N, "ties %s" % loader)


NONFINITE = [(f, N, C, k) for f in NF.FAMILIES for (N, C, k) in ((200, 260, 8), (333, 192, 8)) if NF._fits(f, N, C, k)]


@pytest.mark.parametrize("family,N,C,k", NONFINITE, ids=["%s-N%d-C%d-k%d" % c for c in NONFINITE])
def test_non_finite_input(family, N, C, k):
    for label, x in NF.variants(family, N, C, k):
        want = oracle(x[None], k, ("nf", family, label, N, C))
        for loader in ("contiguous", "ld+1"):
            same(dense_knn(np.asarray(x)[None], k, loader), want, 0, N, "family=%s (%s) %s %s" % (family, label, (N, C, k), loader))


# ------------------------------------------------------------------------------------------------------
# packed towers
# ------------------------------------------------------------------------------------------------------
def tower(sizes, C, k, bad=None):
    """(x (R, C), offsets, [the oracle's lists of cloud b as tower rows]); bad = (place, family): that cloud is a non-finite one."""
    key = ("tower", sizes, C, k, bad)
    if key not in _REF:
        clouds = [np.random.default_rng([b, n, C, 9]).standard_normal((n, C)).astype(np.float32) for b, n in enumerate(sizes)]
        if bad is not None:
            clouds[bad[0]] = np.array(NF.variants(bad[1], sizes[bad[0]], C, k)[0][1])
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        want = [(O.k_nn(c[None], k)[0] + off[b]).astype(np.int32) for b, c in enumerate(clouds)]
        _REF[key] = (np.concatenate(clouds, 0), off, want)
    return _REF[key]


def packed_knn(x, off, k, loader="contiguous", seed=None, expect="wide"):
    from dgcnn import _engine as E
    R = len(x)
    sd = None if seed is None else dev(np.array(seed, np.int32).reshape(1, R, -1))
    xd = view(x, loader)
    return host(recorded(lambda: E.knn(xd, 1, R, k, seed=sd, seg=E.Segments(off, R)),
                         wide_kernel(xd, k, "PackedClouds") if expect == "wide" else expect)).reshape(R, k)


def check_tower(idx, off, want, what):
    for b, w in enumerate(want):
        same(idx[off[b]:off[b + 1]], w, int(off[b]), int(off[b + 1] - off[b]), "%s cloud=%d" % (what, b))


PACKED = [((21, 700, 64, 333), C, k) for C in (132, 192, 260) for k in (1, 8, 20, 21)] + \
         [((1, 63, 64, 65, 130, 5), C, 1) for C in (132, 192, 260)]


@pytest.mark.parametrize("sizes,C,k", PACKED, ids=["%s-C%d-k%d" % ("/".join(map(str, s)), C, k) for s, C, k in PACKED])
def test_packed_towers(sizes, C, k):
    x, off, want = tower(sizes, C, k)
    loader = LOADERS[(C + k) % 3]
    check_tower(packed_knn(x, off, k, loader), off, want, "packed %s C=%d k=%d %s" % (sizes, C, k, loader))


@pytest.mark.parametrize("family", NF.FAMILIES)
def test_packed_tower_with_a_non_finite_cloud_in_the_middle(family):
    sizes, C, k = (130, 200, 65), 192, 8
    assert NF._fits(family, 200, C, k)
    x, off, want = tower(sizes, C, k, bad=(1, family))
    check_tower(packed_knn(x, off, k), off, want, "packed, cloud 1 of family %s" % family)


@pytest.mark.parametrize("C,k", [(132, 8), (260, 21)])
def test_a_one_cloud_tower_equals_the_dense_call(C, k):
    N = 200
    x = normal(1, N, C)
    dense = dense_knn(x, k)
    same(dense, oracle(x, k, ("normal", 1, N, C)), 0, N, "dense (1, %d, %d, %d)" % (N, C, k))
    np.testing.assert_array_equal(packed_knn(x[0], np.array([0, N], np.int64), k), dense[0])


# ------------------------------------------------------------------------------------------------------
# seeds are accepted and ignored
# ------------------------------------------------------------------------------------------------------
def test_seeds_do_not_matter_dense():
    B, N, C, k = 1, 200, 192, 8
    x = normal(B, N, C)
    want = oracle(x, k, ("normal", B, N, C))
    plain = dense_knn(x, k)
    same(plain, want, 0, N, "unseeded")
    with forced(seed_min_n=0):
        for name, sd in (("own graph", want), ("own graph reversed", want[:, :, ::-1]), ("graph of unrelated features", unrelated(N, k)[None])):
            got = dense_knn(x, k, seed=sd)
            same(got, want, 0, N, "seeded C=192, seeds=%s" % name)
            np.testing.assert_array_equal(got, plain)


def test_seeds_do_not_matter_packed():
    sizes, C, k = (21, 700, 64, 333), 192, 8
    x, off, want = tower(sizes, C, k)
    plain = packed_knn(x, off, k)
    check_tower(plain, off, want, "packed unseeded")
    full = np.concatenate(want, 0)
    other = np.concatenate([unrelated(int(n), k) + off[b] for b, n in enumerate(sizes)], 0).astype(np.int32)
    with forced(seed_min_n=0):
        for name, sd in (("own graph", full), ("own graph reversed", full[:, ::-1]), ("graph of unrelated features", other)):
            got = packed_knn(x, off, k, seed=sd)
            check_tower(got, off, want, "packed seeded C=192, seeds=%s" % name)
            np.testing.assert_array_equal(got, plain)


# ------------------------------------------------------------------------------------------------------
# the switch
# ------------------------------------------------------------------------------------------------------
SWITCH = [(C, N) for C in (5, 16, 64, 65, 68, 127, 128) for N in (65, 200)]


@pytest.mark.parametrize("C,N", SWITCH, ids=["C%d-N%d" % c for c in SWITCH])
def test_the_switch_sends_narrow_rows_to_the_wide_kernel(C, N):
    from dgcnn import _engine as E
    from dgcnn import _hip as H
    B, k = 2, 9 if N == 65 else 20
    x = normal(B, N, C)
    want = oracle(x, k, ("normal", B, N, C))
    assert H.load().dgcnn_knn_wide_min_c(-1) == DEFAULT_MIN_C and not E._knn_wide(C)
    default = dense_knn(x, k, expect=None)                    # the narrow kernels: what the switch is held against
    same(default, want, 0, N, "default path %s" % ((B, N, C, k),))
    with forced(wide_min_c=5) as lib:
        assert lib.dgcnn_knn_wide_min_c(-1) == 5 and E._knn_wide(C)
        for loader in ("contiguous", "ld+1"):
            got = dense_knn(x, k, loader)
            same(got, want, 0, N, "wide_min_c=5 %s %s" % ((B, N, C, k), loader))
            np.testing.assert_array_equal(got, default)
        R = B * N                                                    # the same rows as one packed tower of B clouds
        off = np.arange(B + 1, dtype=np.int64) * N
        tw = [(want[b] + off[b]).astype(np.int32) for b in range(B)]
        check_tower(packed_knn(x.reshape(R, C), off, k), off, tw, "wide_min_c=5 packed %s" % ((B, N, C, k),))
    assert H.load().dgcnn_knn_wide_min_c(-1) == DEFAULT_MIN_C


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
    need = int(lib.dgcnn_knn_workspace_bytes(B, N, min(C, 1024), k))
    ws = g.new((need - ws_short,), torch.uint8, fill=77)
    rc = lib.dgcnn_knn_f32(x.data_ptr(), B, N, C, C, k, idx.data_ptr(), ws.data_ptr(), need - ws_short, H._stream())
    return rc, g, idx, ws


def _untouched(g, idx, ws):
    g.check()
    assert (host(idx) == 777).all() and (host(ws) == 77).all(), "a refused call wrote to its buffers"


def test_c_above_1024_is_unsupported():
    rc, g, idx, ws = _guarded_call(1, 64, 1025, 8)
    assert rc == EUNSUP
    _untouched(g, idx, ws)


def test_force_valu_refuses_wide_rows():
    with forced(force_valu=1):
        rc, g, idx, ws = _guarded_call(1, 64, 129, 8)
    assert rc == EUNSUP
    _untouched(g, idx, ws)


def test_a_workspace_one_byte_short_is_refused():
    rc, g, idx, ws = _guarded_call(2, 100, 260, 8, ws_short=1)
    assert rc == EINVAL
    _untouched(g, idx, ws)
    rc, g, idx, ws = _guarded_call(2, 100, 260, 8)            # and the full one runs, inside its buffers
    assert rc == 0
    g.check()
    assert (host(idx) >= 0).all() and (host(idx) < 100).all()


def test_the_packed_entry_refuses_the_same():
    from dgcnn import _hip as H
    lib = H.load()
    g = Guard()
    R, k = 128, 8
    off = g.put(np.array([0, 64, 128], np.int32))
    idx = g.new((R, k), torch.int32, fill=777)
    for C, valu, short, code in ((1025, 0, 0, EUNSUP), (129, 1, 0, EUNSUP), (260, 0, 1, EINVAL)):
        x = g.put(np.random.default_rng(2).standard_normal((R, C)).astype(np.float32))
        need = int(lib.dgcnn_knn_seg_workspace_bytes(R, 64, min(C, 1024), k))
        ws = g.new((need - short,), torch.uint8, fill=77)
        with forced(force_valu=valu):
            rc = lib.dgcnn_knn_seg_f32(x.data_ptr(), C, C, k, 2, off.data_ptr(), R, 64, 64, None, 0, 0, idx.data_ptr(), ws.data_ptr(),
                                       need - short, H._stream())
        assert rc == code, (C, valu, short, rc)
        _untouched(g, idx, ws)


# ------------------------------------------------------------------------------------------------------
# repeatability
# ------------------------------------------------------------------------------------------------------
def test_two_calls_are_bit_identical():
    x = normal(3, 200, 260)
    a, b = dense_knn(x, 20), dense_knn(x, 20)
    np.testing.assert_array_equal(a, b)
    xt, off, _ = tower((21, 700, 64, 333), 192, 20)
    np.testing.assert_array_equal(packed_knn(xt, off, 20), packed_knn(xt, off, 20))

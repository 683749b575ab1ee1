"""CPU checks of the host side of farthest point sampling and the row take (csrc/fps.hip: dgcnn_fps_resident_max_n,
dgcnn_fps_workspace_bytes, dgcnn_fps_f32, dgcnn_rows_gather_f32, dgcnn_rows_scatter_f32; dgcnn/ops.py: farthest_point_sample, take_rows):
the workspace formula, every refusal of the C entries -- its code, its reason, and no device call: the library loads without a GPU, the
pointers are never dereferenced on the host and nothing is launched before the checks pass -- and every ValueError of the Python
interface, raised from shapes and offsets alone."""
import ctypes
import inspect

import pytest
import torch

EINVAL, ENOSPC, EUNSUP = -1, -3, -4
P = ctypes.c_void_p(4096)                    # a non-null, 16-byte aligned address that no check reads through
ODD = ctypes.c_void_p(4100)                  # 4-byte aligned only


def lib():
    from dgcnn import _hip as H
    return H.load()


def pad(n):
    return (n + 255) // 256 * 256


@pytest.mark.parametrize("C", [1, 3, 4, 5, 64])
def test_workspace_on_both_sides_of_the_resident_limit(C):
    L = lib()
    lim = L.dgcnn_fps_resident_max_n(C)
    assert (lim >= 1024) if C <= 4 else (lim == 0)
    for rows in (lim + 1, 3 * lim + 7, 100000):
        if lim:
            assert L.dgcnn_fps_workspace_bytes(rows, C, lim) == 0, (rows, C)
            assert L.dgcnn_fps_workspace_bytes(rows, C, 1) == 0
        assert L.dgcnn_fps_workspace_bytes(rows, C, lim + 1) == pad(4 * rows), (rows, C)
    assert L.dgcnn_fps_workspace_bytes(100000, C, 100000) == pad(400000)


def test_workspace_is_zero_for_sizes_the_entry_refuses():
    L = lib()
    for rows, C, max_n in ((0, 3, 1), (-5, 3, 1), (100, 0, 10), (100, 65, 10), (100, 3, 0), (100, 3, 101), (100, -1, 10)):
        assert L.dgcnn_fps_workspace_bytes(rows, C, max_n) == 0, (rows, C, max_n)
    for C in (0, -1, 65, 1000):
        assert L.dgcnn_fps_resident_max_n(C) == 0


def test_prototypes():
    from dgcnn import _hip as H
    assert "dgcnn_fps_workspace_bytes" in H.INT64_RESULTS
    for name in ("dgcnn_fps_f32", "dgcnn_fps_resident_max_n", "dgcnn_rows_gather_f32", "dgcnn_rows_scatter_f32"):
        assert name not in H.INT64_RESULTS
    assert len(H.PROTOTYPES["dgcnn_fps_f32"]) == 16
    assert len(H.PROTOTYPES["dgcnn_rows_gather_f32"]) == 11 and len(H.PROTOTYPES["dgcnn_rows_scatter_f32"]) == 12
    assert H.PROTOTYPES["dgcnn_fps_workspace_bytes"] == [ctypes.c_int] * 3 and H.PROTOTYPES["dgcnn_fps_resident_max_n"] == [ctypes.c_int]
    assert H.PROTOTYPES["dgcnn_fps_f32"][1] is ctypes.c_int64 and H.PROTOTYPES["dgcnn_fps_f32"][14] is ctypes.c_size_t


def fps(x=P, ldx=3, C=3, nseg=2, x_off=None, s_off=None, rows=200, samples=20, max_n=100, max_m=10, start=None, idx=P, dist=None,
        ws=None, nws=0):
    """dgcnn_fps_f32 with a valid dense call's arguments (2 clouds of 100 rows, 10 samples each) unless overridden"""
    return lib().dgcnn_fps_f32(x, ldx, C, nseg, x_off, s_off, rows, samples, max_n, max_m, start, idx, dist, ws, nws, None)


BIG = dict(nseg=1, rows=20000, samples=10, max_n=20000)          # one cloud above the resident limit: the streaming form
FPS = [
    ("null x", dict(x=None), EINVAL, b"null"),
    ("null idx", dict(idx=None), EINVAL, b"null"),
    ("x_off without s_off", dict(x_off=P), EINVAL, b"x_off"),
    ("s_off without x_off", dict(s_off=P), EINVAL, b"s_off"),
    ("C = 0", dict(C=0), EINVAL, b"C=0"),
    ("C = 65", dict(C=65, ldx=65), EUNSUP, b"C=65"),
    ("nseg = 0", dict(nseg=0), EINVAL, b"nseg=0"),
    ("nseg = 65536", dict(nseg=65536, rows=65536, samples=65536, max_n=1, max_m=1), EUNSUP, b"nseg=65536"),
    ("rows = 0", dict(rows=0), EINVAL, b"rows=0"),
    ("samples = 0", dict(samples=0), EINVAL, b"samples=0"),
    ("max_n = 0", dict(max_n=0), EINVAL, b"max_n=0"),
    ("max_m = -1", dict(max_m=-1), EINVAL, b"max_m=-1"),
    ("max_m > max_n", dict(max_m=101, samples=202), EINVAL, b"max_m=101"),
    ("ldx < C", dict(ldx=2), EINVAL, b"ldx=2"),
    ("dense rows do not multiply out", dict(rows=201), EINVAL, b"rows=201"),
    ("dense samples do not multiply out", dict(samples=21), EINVAL, b"samples=21"),
    ("packed max_n > rows", dict(x_off=P, s_off=P, max_n=201), EINVAL, b"max_n=201"),
    ("streaming without a workspace", dict(BIG), EINVAL, b"workspace"),
    ("streaming with a misaligned workspace", dict(BIG, ws=ODD, nws=1 << 20), EINVAL, b"workspace"),
    ("streaming workspace one byte short", dict(BIG, ws=P, nws=pad(80000) - 1), ENOSPC, b"workspace"),
    ("wide rows without a workspace", dict(C=5, ldx=5), EINVAL, b"workspace"),
]


@pytest.mark.parametrize("what,args,code,reason", FPS, ids=[r[0] for r in FPS])
def test_fps_refusals_return_their_code_before_any_device_call(what, args, code, reason):
    assert fps(**args) == code, what
    msg = lib().dgcnn_last_error()
    assert b"dgcnn_fps_f32" in msg and reason in msg, msg


def gather(x=P, ldx=8, idx=P, s_rows=10, x_rows=16, M=5, N=8, F=8, y=P, ldy=8):
    """dgcnn_rows_gather_f32 with a valid dense call's arguments (2 clouds of 8 rows, 5 taken from each) unless overridden"""
    return lib().dgcnn_rows_gather_f32(x, ldx, idx, s_rows, x_rows, M, N, F, y, ldy, None)


def scatter(dy=P, lddy=8, idx=P, s_rows=10, x_rows=16, M=5, N=8, F=8, dx=P, lddx=8, beta=0):
    return lib().dgcnn_rows_scatter_f32(dy, lddy, idx, s_rows, x_rows, M, N, F, dx, lddx, beta, None)


SHARED = [
    ("null idx", dict(idx=None), b"null"),
    ("F = 0", dict(F=0), b"F=0"),
    ("F = -4", dict(F=-4), b"F=-4"),
    ("s_rows = 0", dict(s_rows=0), b"s_rows=0"),
    ("x_rows = 0", dict(x_rows=0), b"x_rows=0"),
    ("s_rows % M != 0", dict(s_rows=11), b"s_rows=11"),
    ("x_rows != B N", dict(x_rows=17), b"x_rows=17"),
    ("M > 0 with N = 0", dict(N=0), b"N=0"),
    ("M = 0 with N != 0", dict(M=0), b"N=8"),
    ("M < 0", dict(M=-1), b"M=-1"),
]
GATHER = [
    ("null x", dict(x=None), b"null"),
    ("null y", dict(y=None), b"null"),
    ("ldx < F", dict(ldx=7), b"ldx=7"),
    ("ldy < F", dict(ldy=4), b"ldy=4"),
]
SCATTER = [
    ("null dy", dict(dy=None), b"null"),
    ("null dx", dict(dx=None), b"null"),
    ("lddy < F", dict(lddy=7), b"lddy=7"),
    ("lddx < F", dict(lddx=4), b"lddx=4"),
    ("beta = 2", dict(beta=2), b"beta"),
    ("beta = -1", dict(beta=-1), b"beta"),
]


def _only(args, fn):
    names = set(inspect.signature(fn).parameters)
    return {k: v for k, v in args.items() if k in names}


@pytest.mark.parametrize("what,args,reason", SHARED + GATHER, ids=[r[0] for r in SHARED + GATHER])
def test_gather_refusals_return_einval_before_any_device_call(what, args, reason):
    assert gather(**_only(args, gather)) == EINVAL, what
    msg = lib().dgcnn_last_error()
    assert b"dgcnn_rows_gather_f32" in msg and reason in msg, msg


@pytest.mark.parametrize("what,args,reason", SHARED + SCATTER, ids=[r[0] for r in SHARED + SCATTER])
def test_scatter_refusals_return_einval_before_any_device_call(what, args, reason):
    assert scatter(**_only(args, scatter)) == EINVAL, what
    msg = lib().dgcnn_last_error()
    assert b"dgcnn_rows_scatter_f32" in msg and reason in msg, msg


# ---------------------------------------------------------------------------------------------------------------
# dgcnn.ops.farthest_point_sample / take_rows: ValueError from shapes and offsets alone (CPU tensors: a call that got past the checks
# would raise HipError, not ValueError, at the first look at the device)
# ---------------------------------------------------------------------------------------------------------------
def z(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


def _fps_cases():
    dense = dict(points=z(2, 8, 3), m=4)
    packed = dict(points=z(30, 3), offsets=[0, 10, 30], m=4)
    return [
        ("neither m nor ratio", dict(dense, m=None), "exactly one"),
        ("both m and ratio", dict(dense, ratio=0.5), "exactly one"),
        ("m = 0", dict(dense, m=0), "m=0"),
        ("m = -2", dict(dense, m=-2), "m=-2"),
        ("m > N", dict(dense, m=9), "m=9"),
        ("m above the smallest cloud", dict(packed, m=11), "m=11"),
        ("one m of a sequence above its cloud", dict(packed, m=[11, 5]), "m=11"),
        ("ratio = 0", dict(dense, m=None, ratio=0.0), "ratio"),
        ("ratio > 1", dict(dense, m=None, ratio=1.5), "ratio"),
        ("ratio < 0", dict(dense, m=None, ratio=-0.5), "ratio"),
        ("ratio = nan", dict(dense, m=None, ratio=float("nan")), "ratio"),
        ("m sequence of the wrong length", dict(packed, m=[4, 4, 4]), "3 counts"),
        ("m sequence in a dense call", dict(dense, m=[4, 4]), "sequence"),
        ("start out of range", dict(dense, start=8), "start=8"),
        ("start negative", dict(dense, start=-1), "start=-1"),
        ("start sequence of the wrong length", dict(dense, start=[0, 1, 2]), "start"),
        ("start outside its own cloud", dict(packed, start=[10, 0]), "start=10"),
        ("C > 64", dict(points=z(2, 8, 65), m=4), "C=65"),
        ("points rank 2 in a dense call", dict(points=z(16, 3), m=4), "points"),
        ("packed points not a tower", dict(packed, points=z(2, 15, 3)), "tower"),
        ("offsets do not end at the rows", dict(packed, offsets=[0, 10, 29]), "offsets"),
        ("an empty cloud", dict(packed, offsets=[0, 30, 30]), "empty"),
    ]


FPS_CASES = _fps_cases()


@pytest.mark.parametrize("what,kw,word", FPS_CASES, ids=[c[0] for c in FPS_CASES])
def test_farthest_point_sample_raises_value_error_on_the_host(what, kw, word):
    import dgcnn
    with pytest.raises(ValueError) as e:
        dgcnn.ops.farthest_point_sample(**kw)
    assert word in str(e.value), str(e.value)


def _take_cases():
    i32 = torch.int32
    return [
        ("idx of another B", dict(x=z(2, 8, 16), idx=z(3, 4, dtype=i32)), "idx"),
        ("idx rank 1 in a dense call", dict(x=z(2, 8, 16), idx=z(8, dtype=i32)), "idx"),
        ("more samples than rows", dict(x=z(2, 8, 16), idx=z(2, 9, dtype=i32)), "idx"),
        ("idx not int32", dict(x=z(2, 8, 16), idx=z(2, 4, dtype=torch.int64)), "int32"),
        ("x rank 2 in a dense call", dict(x=z(16, 16), idx=z(2, 4, dtype=i32)), "x"),
        ("x rank 4 without the singleton", dict(x=z(2, 8, 2, 16), idx=z(2, 4, dtype=i32)), "x"),
        ("packed x not a tower", dict(x=z(2, 15, 16), idx=z(8, dtype=i32), offsets=[0, 10, 30]), "x"),
        ("offsets do not end at the rows", dict(x=z(30, 16), idx=z(8, dtype=i32), offsets=[0, 10, 29]), "offsets"),
        ("packed idx rank 2", dict(x=z(30, 16), idx=z(2, 4, dtype=i32), offsets=[0, 10, 30]), "idx"),
    ]


TAKE_CASES = _take_cases()


@pytest.mark.parametrize("what,kw,word", TAKE_CASES, ids=[c[0] for c in TAKE_CASES])
def test_take_rows_raises_value_error_on_the_host(what, kw, word):
    import dgcnn
    with pytest.raises(ValueError) as e:
        dgcnn.ops.take_rows(**kw)
    assert "take_rows" in str(e.value) and word in str(e.value), str(e.value)


def test_valid_calls_get_past_the_host_checks():
    """the same shapes without the defect reach the device (a CPU tensor: HipError, not ValueError) -- the checks refuse nothing valid"""
    import dgcnn
    from dgcnn import _hip as H
    for kw in (dict(points=z(2, 8, 3), m=8), dict(points=z(2, 8, 3), ratio=0.3, start=7, return_dist=True),
               dict(points=z(1, 30, 64), offsets=[0, 10, 30], m=[10, 1], start=[9, 19]),
               dict(points=z(30, 3), offsets=[0, 10, 30], ratio=1.0)):
        with pytest.raises(H.HipError):
            dgcnn.ops.farthest_point_sample(**kw)
    i32 = torch.int32
    for kw in (dict(x=z(2, 8, 3), idx=z(2, 8, dtype=i32)), dict(x=z(2, 8, 1, 16), idx=z(2, 1, dtype=i32)),
               dict(x=z(1, 30, 1, 16), idx=z(11, dtype=i32), offsets=[0, 10, 30])):
        with pytest.raises(H.HipError):
            dgcnn.ops.take_rows(**kw)


def test_ratio_counts_as_pyg_does():
    from dgcnn import ops
    assert ops._fps_counts(None, 0.25, [8, 9, 1, 1000], False) == [2, 3, 1, 250]
    assert ops._fps_counts(None, 1.0, [8, 9], False) == [8, 9]
    assert ops._fps_counts(None, 1e-9, [8, 9], True) == [1, 1]
    assert ops._fps_counts(3, None, [8, 9], False) == [3, 3] and ops._fps_counts([3, 9], None, [8, 9], False) == [3, 9]


def test_signatures():
    import dgcnn
    sig = inspect.signature(dgcnn.ops.farthest_point_sample)
    assert list(sig.parameters) == ["points", "m", "ratio", "offsets", "start", "return_dist"]
    assert all(sig.parameters[n].default is None for n in ("m", "ratio", "offsets", "start")) and sig.parameters["return_dist"].default is False
    assert list(inspect.signature(dgcnn.ops.take_rows).parameters) == ["x", "idx", "offsets"]
    assert "distinct" in dgcnn.ops.take_rows.__doc__.lower()


def test_the_engine_entries_check_too():
    from dgcnn import _engine as E
    with pytest.raises(ValueError):
        E.fps(z(16, 3), 2, 8, 9)                                              # m > N
    with pytest.raises(ValueError):
        E.fps(z(16, 65), 2, 8, 4)                                             # C
    with pytest.raises(ValueError):
        E.fps(z(16, 3), 2, 8, 4, start=[0, 8])                                # start
    with pytest.raises(ValueError):
        E.fps(z(30, 3), 1, 30, 0, seg=E.Segments([0, 10, 30]), sseg=E.Segments([0, 11, 12]))      # a cloud sampled beyond its size
    with pytest.raises(ValueError):
        E.take_rows(z(17, 16), z(2, 4, dtype=torch.int32), 2, 4, 8, False)
    assert E.FPS_MAX_C == 64

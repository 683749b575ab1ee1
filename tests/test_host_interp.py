"""CPU checks of the host side of the feature interpolation (csrc/interp.hip: dgcnn_interp_f32, dgcnn_interp_bwd_workspace_bytes,
dgcnn_interp_bwd_f32; dgcnn/ops.py:interpolate): the workspace formula, every refusal of the C entries -- its code, its reason, and no
device call: the library loads without a GPU, the pointers are never dereferenced on the host and nothing is launched before the checks
pass -- and every ValueError of the Python interface, raised from shapes and offsets alone."""
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


def ws_bytes(q, p, k):
    """the documented layout: [off: p + 1 int32 | counts: p int32 | rev: q k int32 | rev sorted: q k int32], each part padded"""
    return pad(4 * (p + 1)) + pad(4 * p) + 2 * pad(4 * q * k)


def test_workspace_is_the_documented_layout():
    L = lib()
    for q, p, k in ((1, 1, 1), (130, 6, 3), (257, 65, 3), (8 * 16384, 8 * 2048, 3), (65536, 8192, 3), (4096, 3, 3), (1000, 999, 64)):
        assert L.dgcnn_interp_bwd_workspace_bytes(q, p, k) == ws_bytes(q, p, k), (q, p, k)
    for q, p, k in ((0, 5, 3), (5, 0, 3), (5, 5, 0), (-1, 5, 3), (1 << 30, 5, 2)):
        assert L.dgcnn_interp_bwd_workspace_bytes(q, p, k) == 0, (q, p, k)


def test_prototypes():
    from dgcnn import _hip as H
    assert "dgcnn_interp_bwd_workspace_bytes" in H.INT64_RESULTS
    assert "dgcnn_interp_f32" not in H.INT64_RESULTS and "dgcnn_interp_bwd_f32" not in H.INT64_RESULTS
    assert len(H.PROTOTYPES["dgcnn_interp_f32"]) == 15 and len(H.PROTOTYPES["dgcnn_interp_bwd_f32"]) == 16
    assert H.PROTOTYPES["dgcnn_interp_bwd_workspace_bytes"] == [ctypes.c_int] * 3
    assert H.PROTOTYPES["dgcnn_interp_f32"][10] is ctypes.c_float


def fwd(feat=P, ldf=8, idx=P, dist=P, q_rows=20, p_rows=16, M=10, N=8, k=3, F=8, eps=1e-16, a=None, y=P, ldy=8):
    """dgcnn_interp_f32 with a valid dense call's arguments (2 clouds of 10 queries on 8 candidates) unless overridden"""
    return lib().dgcnn_interp_f32(feat, ldf, idx, dist, q_rows, p_rows, M, N, k, F, eps, a, y, ldy, None)


def bwd(dy=P, lddy=8, idx=P, a=P, q_rows=20, p_rows=16, M=10, N=8, k=3, F=8, dfeat=P, lddf=8, beta=0, ws=P, nws=None):
    nws = ws_bytes(20, 16, 3) if nws is None else nws
    return lib().dgcnn_interp_bwd_f32(dy, lddy, idx, a, q_rows, p_rows, M, N, k, F, dfeat, lddf, beta, ws, nws, None)


SHARED = [      # refusals of both entries: the graph's shape
    ("null idx", dict(idx=None), EINVAL, b"null"),
    ("k = 0", dict(k=0), EINVAL, b"k=0"),
    ("k = -1", dict(k=-1), EINVAL, b"k=-1"),
    ("k = 65", dict(k=65), EUNSUP, b"k=65"),
    ("F = 0", dict(F=0), EINVAL, b"F=0"),
    ("F = 6", dict(F=6), EUNSUP, b"F=6"),
    ("F = 1028", dict(F=1028, ldf=1028, ldy=1028, lddy=1028, lddf=1028), EUNSUP, b"F=1028"),
    ("q_rows = 0", dict(q_rows=0), EINVAL, b"q_rows=0"),
    ("p_rows = 0", dict(p_rows=0), EINVAL, b"p_rows=0"),
    ("q_rows k >= 2^31", dict(q_rows=1 << 30, p_rows=8, M=1 << 30, N=8, k=2), EUNSUP, b"2^31"),
    ("q_rows % M != 0", dict(q_rows=21), EINVAL, b"q_rows=21"),
    ("p_rows != B N", dict(p_rows=17), EINVAL, b"p_rows=17"),
    ("M > 0 with N = 0", dict(N=0), EINVAL, b"N=0"),
    ("M = 0 with N != 0", dict(M=0), EINVAL, b"N=8"),
    ("M < 0", dict(M=-1), EINVAL, b"M=-1"),
]
FWD = [
    ("null feat", dict(feat=None), EINVAL, b"null"),
    ("null dist", dict(dist=None), EINVAL, b"null"),
    ("null y", dict(y=None), EINVAL, b"null"),
    ("ldf < F", dict(ldf=4), EINVAL, b"ldf=4"),
    ("ldy < F", dict(ldy=4), EINVAL, b"ldy=4"),
    ("ldf % 4", dict(ldf=10), EINVAL, b"ldf=10"),
    ("ldy % 4", dict(ldy=9), EINVAL, b"ldy=9"),
    ("misaligned feat", dict(feat=ODD), EINVAL, b"aligned"),
    ("misaligned y", dict(y=ODD), EINVAL, b"aligned"),
    ("eps = 0", dict(eps=0.0), EINVAL, b"eps"),
    ("eps = 1e-31", dict(eps=1e-31), EINVAL, b"eps"),
    ("eps < 0", dict(eps=-1.0), EINVAL, b"eps"),
    ("eps = inf", dict(eps=float("inf")), EINVAL, b"eps"),
    ("eps = nan", dict(eps=float("nan")), EINVAL, b"eps"),
]
BWD = [
    ("null dy", dict(dy=None), EINVAL, b"null"),
    ("null a", dict(a=None), EINVAL, b"null"),
    ("null dfeat", dict(dfeat=None), EINVAL, b"null"),
    ("null ws", dict(ws=None), EINVAL, b"null"),
    ("lddy < F", dict(lddy=4), EINVAL, b"lddy=4"),
    ("lddf < F", dict(lddf=4), EINVAL, b"lddf=4"),
    ("lddf % 4", dict(lddf=10), EINVAL, b"lddf=10"),
    ("misaligned dy", dict(dy=ODD), EINVAL, b"aligned"),
    ("misaligned dfeat", dict(dfeat=ODD), EINVAL, b"aligned"),
    ("misaligned ws", dict(ws=ODD), EINVAL, b"aligned"),
    ("beta = 2", dict(beta=2), EINVAL, b"beta"),
    ("beta = -1", dict(beta=-1), EINVAL, b"beta"),
    ("ws one byte short", dict(nws=ws_bytes(20, 16, 3) - 1), ENOSPC, b"workspace"),
    ("ws = 0 bytes", dict(nws=0), ENOSPC, b"workspace"),
]


def _only(args, fn):
    names = set(inspect.signature(fn).parameters)
    return {k: v for k, v in args.items() if k in names}


@pytest.mark.parametrize("what,args,code,reason", SHARED + FWD, ids=[r[0] for r in SHARED + FWD])
def test_forward_refusals_return_their_code_before_any_device_call(what, args, code, reason):
    assert fwd(**_only(args, fwd)) == code, what
    msg = lib().dgcnn_last_error()
    assert b"dgcnn_interp_f32" in msg and reason in msg, msg


@pytest.mark.parametrize("what,args,code,reason", SHARED + BWD, ids=[r[0] for r in SHARED + BWD])
def test_backward_refusals_return_their_code_before_any_device_call(what, args, code, reason):
    assert bwd(**_only(args, bwd)) == code, what
    msg = lib().dgcnn_last_error()
    assert b"dgcnn_interp_bwd_f32" in msg and reason in msg, msg


def test_a_packed_call_passes_the_shape_checks_up_to_the_workspace():
    """M = N = 0 (idx holds tower rows) is a valid shape: the call gets as far as the workspace check"""
    assert bwd(M=0, N=0, q_rows=21, p_rows=17, nws=0) == ENOSPC


# ---------------------------------------------------------------------------------------------------------------
# dgcnn.ops.interpolate: ValueError from shapes and offsets alone (CPU tensors: a call that got past the checks would raise HipError,
# not ValueError, at the first look at the device)
# ---------------------------------------------------------------------------------------------------------------
def z(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


def _cases():
    off, qoff = [0, 10, 30], [0, 5, 12]
    dense = dict(features=z(2, 8, 16), points=z(2, 8, 3), queries=z(2, 5, 3))
    packed = dict(features=z(30, 16), points=z(30, 3), queries=z(12, 3), offsets=off, query_offsets=qoff)
    g = lambda B, M, k: (z(B, M, k, dtype=torch.int32), z(B, M, k))
    return [
        ("feature rows != point rows", dict(dense, features=z(2, 9, 16)), "features"),
        ("feature clouds != point clouds", dict(dense, features=z(3, 8, 16)), "features"),
        ("features rank 2 in a dense call", dict(dense, features=z(16, 16)), "features"),
        ("features rank 4 without the singleton", dict(dense, features=z(2, 8, 2, 16)), "features"),
        ("F % 4", dict(dense, features=z(2, 8, 6)), "F=6"),
        ("F > 1024", dict(dense, features=z(2, 8, 1028)), "F=1028"),
        ("queries of another B", dict(dense, queries=z(3, 5, 3)), "queries"),
        ("queries of other channels", dict(dense, queries=z(2, 5, 4)), "queries"),
        ("queries not rank 3", dict(dense, queries=z(5, 3)), "queries"),
        ("points not rank 3", dict(dense, points=z(16, 3)), "points"),
        ("k = 0", dict(dense, k=0), "k=0"),
        ("k > 64", dict(features=z(2, 100, 16), points=z(2, 100, 3), queries=z(2, 5, 3), k=65), "k=65"),
        ("k > N", dict(dense, k=9), "k=9"),
        ("eps = 0", dict(dense, eps=0.0), "eps"),
        ("eps = 1e-31", dict(dense, eps=1e-31), "eps"),
        ("eps = inf", dict(dense, eps=float("inf")), "eps"),
        ("eps = nan", dict(dense, eps=float("nan")), "eps"),
        ("no graph and no queries", dict(dense, queries=None), "queries"),
        ("no graph and no points", dict(dense, points=None), "points"),
        ("graph of another k", dict(dense, graph=g(2, 5, 4)), "graph"),
        ("graph of another M", dict(dense, graph=g(2, 6, 3)), "graph"),
        ("graph of another B", dict(dense, points=None, queries=None, graph=g(3, 5, 3)), "graph"),
        ("graph idx and dist differ", dict(dense, graph=(z(2, 5, 3, dtype=torch.int32), z(2, 5, 2))), "graph"),
        ("graph not a pair", dict(dense, graph=z(2, 5, 3)), "graph"),
        ("skip rows != query rows", dict(dense, skip=z(2, 6, 8)), "skip"),
        ("skip clouds != query clouds", dict(dense, skip=z(1, 5, 8)), "skip"),
        ("skip Cs % 4", dict(dense, skip=z(2, 5, 6)), "Cs=6"),
        ("offsets without query_offsets", dict(packed, query_offsets=None), "query_offsets"),
        ("query_offsets without offsets", dict(packed, offsets=None), "offsets"),
        ("packed features not a tower", dict(packed, features=z(2, 15, 16)), "features"),
        ("offsets do not end at the feature rows", dict(packed, offsets=[0, 10, 29]), "offsets"),
        ("packed feature rows != point rows", dict(packed, points=z(31, 3)), "features"),
        ("query_offsets do not end at the query rows", dict(packed, query_offsets=[0, 5, 11]), "query_offsets"),
        ("different number of clouds", dict(packed, query_offsets=[0, 3, 5, 12]), "clouds"),
        ("an empty query cloud", dict(packed, query_offsets=[0, 12, 12]), "empty"),
        ("k > smallest candidate cloud", dict(packed, k=11, queries=z(40, 3), query_offsets=[0, 20, 40]), "k=11"),
        ("packed skip rows", dict(packed, skip=z(13, 8)), "skip"),
    ]


CASES = _cases()


@pytest.mark.parametrize("what,kw,word", CASES, ids=[c[0] for c in CASES])
def test_interpolate_raises_value_error_on_the_host(what, kw, word):
    import dgcnn
    with pytest.raises(ValueError) as e:
        dgcnn.ops.interpolate(**kw)
    assert "interpolate" in str(e.value) or "offsets" in str(e.value), str(e.value)
    assert word in str(e.value), str(e.value)


def test_valid_calls_get_past_the_host_checks():
    """the same shapes without the defect reach the device (a CPU tensor: HipError, not ValueError) -- the checks refuse nothing valid"""
    import dgcnn
    from dgcnn import _hip as H
    g = (z(2, 5, 3, dtype=torch.int32), z(2, 5, 3))
    for kw in (dict(features=z(2, 8, 16), points=z(2, 8, 3), queries=z(2, 5, 3)),
               dict(features=z(2, 8, 1, 16), points=None, queries=None, graph=g, skip=z(2, 5, 8)),
               dict(features=z(1, 30, 16), points=z(30, 3), queries=z(1, 12, 3), offsets=[0, 10, 30], query_offsets=[0, 5, 12], k=10)):
        with pytest.raises(H.HipError):
            dgcnn.ops.interpolate(**kw)


def test_signature():
    import dgcnn
    sig = inspect.signature(dgcnn.ops.interpolate)
    assert list(sig.parameters) == ["features", "points", "queries", "k", "offsets", "query_offsets", "eps", "graph", "skip"]
    assert sig.parameters["k"].default == 3 and sig.parameters["eps"].default == 1e-16


def test_the_engine_entry_checks_too():
    from dgcnn import _engine as E
    i, d = z(2, 5, 3, dtype=torch.int32), z(2, 5, 3)
    with pytest.raises(ValueError):
        E.interpolate(z(17, 16), i, d, 2, 5, 8, 3, False, 1e-16)          # feature rows
    with pytest.raises(ValueError):
        E.interpolate(z(16, 6), i, d, 2, 5, 8, 3, False, 1e-16)           # F % 4
    with pytest.raises(ValueError):
        E.interpolate(z(16, 16), i, d, 2, 5, 8, 3, False, 0.0)            # eps
    with pytest.raises(ValueError):
        E.interpolate(z(16, 16), i, d, 2, 5, 8, 4, False, 1e-16)          # graph shape
    with pytest.raises(ValueError):
        E.interpolate(z(200, 16), z(2, 5, 65, dtype=torch.int32), z(2, 5, 65), 2, 5, 100, 65, False, 1e-16)
    assert E.INTERP_MAX_K == 64

"""CPU checks of the host side of the k-NN between two point sets (csrc/knn_cross.hip: dgcnn_knn_cross_f32; dgcnn/ops.py:k_nn with
queries= / return_dist=): the workspace formula, every refusal of the C entry -- its code, its reason, and no device call: the library
loads without a GPU, the pointers are never dereferenced on the host and nothing is launched before the checks pass -- and every
ValueError of the Python interface, raised from shapes and offsets alone."""
import ctypes

import numpy as np
import pytest
import torch

EINVAL, EUNSUP = -1, -4
P = ctypes.c_void_p(4096)                    # a non-null, 16-byte aligned address that no check reads through


def lib():
    from dgcnn import _hip as H
    return H.load()


def pad(n):
    return (n + 255) // 256 * 256


def test_workspace_is_the_two_norm_vectors():
    L = lib()
    for q, p in ((1, 1), (64, 64), (65, 63), (24 * 2048, 24 * 2048), (8 * 65536, 8 * 8192), (1000, 3)):
        assert L.dgcnn_knn_cross_workspace_bytes(q, p) == pad(4 * q) + pad(4 * p), (q, p)
    assert L.dgcnn_knn_cross_workspace_bytes(0, 5) == 0 and L.dgcnn_knn_cross_workspace_bytes(5, 0) == 0
    assert L.dgcnn_knn_cross_workspace_bytes(-1, 5) == 0


def test_prototypes():
    from dgcnn import _hip as H
    assert "dgcnn_knn_cross_workspace_bytes" in H.INT64_RESULTS and "dgcnn_knn_cross_f32" not in H.INT64_RESULTS
    assert len(H.PROTOTYPES["dgcnn_knn_cross_f32"]) == 19 and H.PROTOTYPES["dgcnn_knn_cross_workspace_bytes"] == [ctypes.c_int] * 2


def call(q=P, ldq=3, p=P, ldp=3, C=3, k=4, nseg=2, q_off=None, p_off=None, q_rows=20, p_rows=16, max_m=10, min_n=8, max_n=8, idx=P,
         dist=None, ws=P, ws_bytes=1 << 20):
    """dgcnn_knn_cross_f32 with a valid dense call's arguments (2 clouds of 10 queries against 8 candidates) unless overridden"""
    return lib().dgcnn_knn_cross_f32(q, ldq, p, ldp, C, k, nseg, q_off, p_off, q_rows, p_rows, max_m, min_n, max_n, idx, dist, ws, ws_bytes,
                                     None)


PACKED = dict(q_off=P, p_off=P, q_rows=30, p_rows=25, max_m=20, min_n=5, max_n=20)      # a valid packed call: 2 clouds

REFUSALS = [
    ("null q", dict(q=None), EINVAL, b"null"),
    ("null p", dict(p=None), EINVAL, b"null"),
    ("null idx", dict(idx=None), EINVAL, b"null"),
    ("null ws", dict(ws=None), EINVAL, b"null"),
    ("only q_off", dict(q_off=P), EINVAL, b"q_off"),
    ("only p_off", dict(p_off=P), EINVAL, b"p_off"),
    ("k = 0", dict(k=0), EINVAL, b"k=0"),
    ("k < 0", dict(k=-3), EINVAL, b"k=-3"),
    ("k > min_n", dict(k=9), EINVAL, b"k=9"),
    ("k > 64", dict(k=65, q_rows=200, p_rows=200, max_m=100, min_n=100, max_n=100), EUNSUP, b"64"),
    ("k > 64 and > min_n", dict(k=65), EUNSUP, b"64"),
    ("C > 1024", dict(C=1025, ldq=1025, ldp=1025), EUNSUP, b"1025"),
    ("C = 0", dict(C=0), EINVAL, b"shape"),
    ("ldq < C", dict(ldq=2), EINVAL, b"shape"),
    ("ldp < C", dict(ldp=2), EINVAL, b"shape"),
    ("nseg = 0", dict(nseg=0), EINVAL, b"shape"),
    ("nseg > 65535", dict(nseg=65536, q_rows=65536 * 10, p_rows=65536 * 8), EINVAL, b"shape"),
    ("dense q_rows", dict(q_rows=21), EINVAL, b"q_rows"),
    ("dense p_rows", dict(p_rows=17), EINVAL, b"p_rows"),
    ("dense min_n != max_n", dict(min_n=7), EINVAL, b"min_n"),
    ("misaligned ws", dict(ws=ctypes.c_void_p(4100)), EINVAL, b"workspace"),
    ("ws one byte short", dict(ws_bytes=pad(80) + pad(64) - 1), EINVAL, b"workspace"),
    ("packed max_m too small", dict(PACKED, max_m=14), EINVAL, b"max_m"),
    ("packed max_m > q_rows", dict(PACKED, max_m=31), EINVAL, b"max_m"),
    ("packed min_n > max_n", dict(PACKED, min_n=21), EINVAL, b"min_n"),
    ("packed max_n too small", dict(PACKED, max_n=12), EINVAL, b"max_n"),
    ("packed min_n too large", dict(PACKED, min_n=13, max_n=13), EINVAL, b"min_n"),
    ("packed k > min_n", dict(PACKED, k=6), EINVAL, b"k=6"),
    ("packed ws short", dict(PACKED, ws_bytes=pad(120) + pad(100) - 1), EINVAL, b"workspace"),
]


@pytest.mark.parametrize("what,args,code,reason", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_return_their_code_before_any_device_call(what, args, code, reason):
    assert call(**args) == code, what
    msg = lib().dgcnn_last_error()
    assert b"dgcnn_knn_cross_f32" in msg and reason in msg, msg


# ---------------------------------------------------------------------------------------------------------------
# dgcnn.ops.k_nn: ValueError from shapes and offsets alone (CPU tensors: a call that got past the checks would raise HipError, not
# ValueError, at the first look at the device)
# ---------------------------------------------------------------------------------------------------------------
def z(*shape):
    return torch.zeros(*shape)


def _cases():
    off = [0, 10, 30]
    return [
        ("C mismatch", dict(points=z(2, 8, 3), k=4, queries=z(2, 5, 4)), "channels"),
        ("B mismatch", dict(points=z(2, 8, 3), k=4, queries=z(3, 5, 3)), "clouds"),
        ("queries not rank 3", dict(points=z(2, 8, 3), k=4, queries=z(5, 3)), "queries"),
        ("query_offsets without queries", dict(points=z(30, 3), k=4, offsets=off, query_offsets=off), "query_offsets without queries"),
        ("query_offsets without queries, dense", dict(points=z(2, 8, 3), k=4, query_offsets=off), "query_offsets without queries"),
        ("offsets without query_offsets", dict(points=z(30, 3), k=4, offsets=off, queries=z(12, 3)), "query_offsets"),
        ("query_offsets without offsets", dict(points=z(30, 3), k=4, queries=z(12, 3), query_offsets=[0, 5, 12]), "offsets"),
        ("different number of clouds", dict(points=z(30, 3), k=4, offsets=off, queries=z(12, 3), query_offsets=[0, 3, 5, 12]), "clouds"),
        ("query_offsets do not end at the rows", dict(points=z(30, 3), k=4, offsets=off, queries=z(12, 3), query_offsets=[0, 5, 11]), "rows"),
        ("an empty query cloud", dict(points=z(30, 3), k=4, offsets=off, queries=z(12, 3), query_offsets=[0, 12, 12]), "empty"),
        ("k = 0", dict(points=z(2, 8, 3), k=0, queries=z(2, 5, 3)), "k=0"),
        ("k > N", dict(points=z(2, 8, 3), k=9, queries=z(2, 50, 3)), "k=9"),
        ("k > N with return_dist", dict(points=z(2, 8, 3), k=9, return_dist=True), "k=9"),
        ("k > smallest candidate cloud", dict(points=z(30, 3), k=11, offsets=off, queries=z(40, 3), query_offsets=[0, 20, 40]), "k=11"),
        ("k > 64 with queries", dict(points=z(2, 100, 3), k=65, queries=z(2, 5, 3)), "64"),
        ("k > 64 with return_dist", dict(points=z(2, 100, 3), k=65, return_dist=True), "64"),
        ("k > 64 packed", dict(points=z(200, 3), k=65, offsets=[0, 100, 200], queries=z(12, 3), query_offsets=[0, 5, 12]), "64"),
    ]


CASES = _cases()


@pytest.mark.parametrize("what,kw,word", CASES, ids=[c[0] for c in CASES])
def test_k_nn_raises_value_error_on_the_host(what, kw, word):
    import dgcnn
    with pytest.raises(ValueError) as e:
        dgcnn.ops.k_nn(**kw)
    assert word in str(e.value), str(e.value)


def test_the_engine_entry_checks_too():
    from dgcnn import _engine as E
    with pytest.raises(ValueError):
        E.knn_cross(z(10, 3), z(16, 4), 2, 5, 8, 4)
    with pytest.raises(ValueError):
        E.knn_cross(z(10, 3), z(16, 3), 2, 5, 8, 65)
    with pytest.raises(ValueError):
        E.knn_cross(z(10, 3), z(16, 3), 2, 5, 8, 9)
    with pytest.raises(ValueError):
        E.knn_cross(z(10, 3), z(16, 3), 1, 10, 16, 4, qseg=E.Segments([0, 4, 10], 10))
    with pytest.raises(ValueError):
        E.knn_cross(z(10, 3), z(16, 3), 1, 10, 16, 4, qseg=E.Segments([0, 4, 10], 10), pseg=E.Segments([0, 4, 10, 16], 16))
    assert E.KNN_CROSS_MAX_K == 64


def test_the_plain_call_keeps_its_signature_and_path():
    """queries=None, return_dist=False: today's code path -- the plain call's own ValueError text, and no knn_cross call"""
    import inspect
    import dgcnn
    from dgcnn import _engine as E
    sig = inspect.signature(dgcnn.ops.k_nn)
    assert list(sig.parameters) == ["points", "k", "offsets", "queries", "query_offsets", "return_dist"]
    assert sig.parameters["queries"].default is None and sig.parameters["return_dist"].default is False
    called = []
    orig = E.knn_cross
    E.knn_cross = lambda *a, **kw: called.append(a)
    try:
        with pytest.raises(Exception) as e:
            dgcnn.ops.k_nn(z(1, 8, 3), 2)                     # a CPU tensor: the plain path refuses it at its first device look
        assert not isinstance(e.value, ValueError)
    finally:
        E.knn_cross = orig
    assert not called

"""CPU checks of the wide-feature k-NN's host side (csrc/knn.hip dispatch, csrc/knn_wide.hip): the switch dgcnn_knn_wide_min_c is
plain host state, the workspace of wide rows keeps the [s_i | bounds] layout, and the header, the library's exports and the ctypes
prototypes agree on the new entry."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = 129


def lib():
    from dgcnn import _hip as H
    return H.load()


def test_the_switch_round_trips():
    L = lib()
    prev = L.dgcnn_knn_wide_min_c(-1)                       # query only
    assert prev == DEFAULT
    try:
        assert L.dgcnn_knn_wide_min_c(5) == DEFAULT and L.dgcnn_knn_wide_min_c(-1) == 5
        assert L.dgcnn_knn_wide_min_c(65) == 5 and L.dgcnn_knn_wide_min_c(-1) == 65
        assert L.dgcnn_knn_wide_min_c(129) == 65 and L.dgcnn_knn_wide_min_c(-1) == 129
    finally:
        L.dgcnn_knn_wide_min_c(prev)
    assert L.dgcnn_knn_wide_min_c(-1) == DEFAULT


def test_the_switch_refuses_values_outside_5_to_129():
    L = lib()
    prev = L.dgcnn_knn_wide_min_c(-1)
    try:
        assert L.dgcnn_knn_wide_min_c(64) == prev
        for bad in (-2, -1, 0, 1, 4, 130, 256, 1024, 1 << 30):
            assert L.dgcnn_knn_wide_min_c(bad) == 64, bad       # returns the value in force and leaves it alone
        assert L.dgcnn_knn_wide_min_c(-1) == 64
    finally:
        L.dgcnn_knn_wide_min_c(prev)


def test_the_engine_names_the_kernel_the_library_will_pick():
    from dgcnn import _engine as E
    L = lib()
    prev = L.dgcnn_knn_wide_min_c(-1)
    try:
        assert not E._knn_wide(128) and E._knn_wide(129) and E._knn_wide(1024)
        assert E._knn_instance(128, 20) == (128, 20) and E._knn_instance(64, 8) == (64, 8)
        assert E._knn_instance(129, 20) == (192, 20) and E._knn_instance(260, 41) == (320, 64)
        L.dgcnn_knn_wide_min_c(65)
        assert not E._knn_wide(64) and E._knn_wide(65) and E._knn_instance(128, 20) == (128, 20) and E._knn_instance(64, 20) == (64, 20)
        L.dgcnn_knn_wide_min_c(5)
        assert E._knn_wide(5) and E._knn_instance(3, 8) == (4, 8)                # raw coordinates never go there
    finally:
        L.dgcnn_knn_wide_min_c(prev)


def test_workspace_of_wide_rows_is_s_i_and_bounds():
    L = lib()
    pad = lambda n: (n + 255) // 256 * 256
    assert L.dgcnn_knn_workspace_bytes(2, 300, 260, 8) == 2 * pad(4 * 2 * 300)
    for C in (129, 192, 512, 1024):
        for k in (1, 20, 64):
            assert L.dgcnn_knn_workspace_bytes(24, 2048, C, k) == 2 * pad(4 * 24 * 2048)
            assert L.dgcnn_knn_seg_workspace_bytes(1237, 700, C, k) == 2 * pad(4 * 1237)
    prev = L.dgcnn_knn_wide_min_c(5)                           # the switch changes no layout
    try:
        assert L.dgcnn_knn_workspace_bytes(2, 300, 128, 8) == 2 * pad(4 * 2 * 300)
        assert L.dgcnn_knn_workspace_bytes(2, 300, 64, 8) > 3 * pad(4 * 2 * 300)          # the append form's buffers stay
    finally:
        L.dgcnn_knn_wide_min_c(prev)


def test_header_exports_and_prototypes_agree_on_the_switch():
    from dgcnn import _hip as H
    text = open(os.path.join(ROOT, "include", "dgcnn_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+dgcnn_knn_wide_min_c\s*\(\s*int\s+\w+\s*\)\s*;", text)
    assert H.PROTOTYPES["dgcnn_knn_wide_min_c"] == [ctypes.c_int]
    assert hasattr(ctypes.CDLL(H.LIB_PATH), "dgcnn_knn_wide_min_c")
    assert "dgcnn_knn_wide_min_c" not in H.INT64_RESULTS


def test_wide_rows_are_refused_without_a_launch_where_they_must_be():
    """C > 1024, and C > 128 under the VALU switch: DGCNN_EUNSUP from the argument checks (no device is touched: the pointers are
    never dereferenced on the host and nothing is launched before the checks pass)."""
    L = lib()
    EUNSUP = -4
    x = ctypes.c_void_p(4096)
    assert L.dgcnn_knn_f32(x, 1, 64, 1025, 1025, 8, x, x, 1 << 20, None) == EUNSUP
    assert b"1025" in L.dgcnn_last_error()
    assert L.dgcnn_knn_seg_f32(x, 1025, 1025, 8, 1, x, 64, 64, 64, None, 0, 0, x, x, 1 << 20, None) == EUNSUP
    prev = L.dgcnn_knn_force_valu(1)
    try:
        assert L.dgcnn_knn_f32(x, 1, 64, 129, 129, 8, x, x, 1 << 20, None) == EUNSUP
        assert L.dgcnn_knn_seg_f32(x, 129, 129, 8, 1, x, 64, 64, 64, None, 0, 0, x, x, 1 << 20, None) == EUNSUP
    finally:
        L.dgcnn_knn_force_valu(prev)

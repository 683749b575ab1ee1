"""The process-wide switches of the library (csrc/switches.cc: one table, filled from the environment when it is first touched) on
the host: dgcnn_switch_get agrees with every switch's own setter, the environment parse keeps every quirk it had while each
switch parsed its own variable, dgcnn_switch_set refuses what that parse would have replaced, and reading -- through the C entry
or through the engine's tag rule -- changes nothing.  No GPU call is made."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

UNSET = -2 ** 31                              # DGCNN_SWITCH_UNSET

NAMES = ["DGCNN_KNN_BF16F", "DGCNN_KNN_FORCE_VALU", "DGCNN_KNN_TIGHTEN_EVERY", "DGCNN_KNN_BIG_K_MIN", "DGCNN_KNN_SEED_MIN_N",
         "DGCNN_KNN_APPEND", "DGCNN_KNN_APPEND_NPR_LX", "DGCNN_KNN_APPEND_NPR_BIG", "DGCNN_KNN_HIST", "DGCNN_KNN_WIDE_MIN_C",
         "DGCNN_KNN_GRID", "DGCNN_KNN_GRID_MIN_N", "DGCNN_KNN_MIX_MIN_N", "DGCNN_EDGE_VALU", "DGCNN_GEMM_ARITH", "DGCNN_GEMM_X3_TILE",
         "DGCNN_EVENT_FLAGS"]

# every switch with nothing in the environment
DEFAULTS = dict(DGCNN_KNN_BF16F=2, DGCNN_KNN_FORCE_VALU=0, DGCNN_KNN_TIGHTEN_EVERY=0, DGCNN_KNN_BIG_K_MIN=65, DGCNN_KNN_SEED_MIN_N=-1,
                DGCNN_KNN_APPEND=1, DGCNN_KNN_APPEND_NPR_LX=1, DGCNN_KNN_APPEND_NPR_BIG=1, DGCNN_KNN_HIST=2, DGCNN_KNN_WIDE_MIN_C=129,
                DGCNN_KNN_GRID=1, DGCNN_KNN_GRID_MIN_N=UNSET, DGCNN_KNN_MIX_MIN_N=0, DGCNN_EDGE_VALU=1, DGCNN_GEMM_ARITH=6,
                DGCNN_GEMM_X3_TILE=0, DGCNN_EVENT_FLAGS=0x20000002)

# (variable, its text, {switch: value}): every other switch stays at its default.  The values were recorded from the library as it
# was while every switch parsed its own variable, by running the same child against it and asking each switch's own setter for its
# "previous" value (dgcnn_knn_bf16_filter set and put back; DGCNN_KNN_GRID as dgcnn_knn_seg_grid_use answered at mean cloud sizes 0
# and 2^62; DGCNN_KNN_GRID_MIN_N as the mean size at which dgcnn_knn_seg_grid_use flipped).  Three had no setter or query that
# runs without a GPU -- DGCNN_KNN_TIGHTEN_EVERY, the N >= 8192 half of DGCNN_KNN_APPEND_NPR and DGCNN_EVENT_FLAGS -- and are
# written down from the parse they had (knn.hip:knn_append_tighten_mask, knn_append_products; plan.cc:event_flags).
ENV_CASES = [
    ("DGCNN_KNN_BF16F", "1", dict(DGCNN_KNN_BF16F=1)),
    ("DGCNN_KNN_BF16F", "0", dict(DGCNN_KNN_BF16F=0)),
    ("DGCNN_KNN_BF16F", "auto", dict(DGCNN_KNN_BF16F=2)),                    # a leading a
    ("DGCNN_KNN_BF16F", "x", dict(DGCNN_KNN_BF16F=0)),                       # atoi
    ("DGCNN_KNN_TIGHTEN_EVERY", "2", dict(DGCNN_KNN_TIGHTEN_EVERY=2)),
    ("DGCNN_KNN_TIGHTEN_EVERY", "0", dict(DGCNN_KNN_TIGHTEN_EVERY=0)),      # the per-form default
    ("DGCNN_KNN_TIGHTEN_EVERY", "3", dict(DGCNN_KNN_TIGHTEN_EVERY=1)),      # no power of two
    ("DGCNN_KNN_TIGHTEN_EVERY", "-4", dict(DGCNN_KNN_TIGHTEN_EVERY=1)),
    ("DGCNN_KNN_BIG_K_MIN", "20", dict(DGCNN_KNN_BIG_K_MIN=20)),
    ("DGCNN_KNN_BIG_K_MIN", "99", dict(DGCNN_KNN_BIG_K_MIN=65)),            # out of range: the default
    ("DGCNN_KNN_BIG_K_MIN", "0", dict(DGCNN_KNN_BIG_K_MIN=65)),
    ("DGCNN_KNN_SEED_MIN_N", "4096", dict(DGCNN_KNN_SEED_MIN_N=4096)),
    ("DGCNN_KNN_SEED_MIN_N", "junk", dict(DGCNN_KNN_SEED_MIN_N=0)),
    ("DGCNN_KNN_APPEND", "0", dict(DGCNN_KNN_APPEND=0)),
    ("DGCNN_KNN_APPEND", "5", dict(DGCNN_KNN_APPEND=1)),
    ("DGCNN_KNN_APPEND", "junk", dict(DGCNN_KNN_APPEND=0)),
    ("DGCNN_KNN_APPEND_NPR", "3,1", dict(DGCNN_KNN_APPEND_NPR_LX=3, DGCNN_KNN_APPEND_NPR_BIG=1)),
    ("DGCNN_KNN_APPEND_NPR", "1,3", dict(DGCNN_KNN_APPEND_NPR_LX=1, DGCNN_KNN_APPEND_NPR_BIG=3)),
    ("DGCNN_KNN_APPEND_NPR", "3", dict(DGCNN_KNN_APPEND_NPR_LX=3, DGCNN_KNN_APPEND_NPR_BIG=1)),
    ("DGCNN_KNN_APPEND_NPR", "7,2", dict(DGCNN_KNN_APPEND_NPR_LX=1, DGCNN_KNN_APPEND_NPR_BIG=1)),   # each of them 3 or else 1
    ("DGCNN_KNN_HIST", "4", dict(DGCNN_KNN_HIST=4)),
    ("DGCNN_KNN_HIST", "0", dict(DGCNN_KNN_HIST=0)),
    ("DGCNN_KNN_HIST", "3", dict(DGCNN_KNN_HIST=2)),                         # invalid becomes 2
    ("DGCNN_KNN_WIDE_MIN_C", "65", dict(DGCNN_KNN_WIDE_MIN_C=65)),
    ("DGCNN_KNN_WIDE_MIN_C", "4", dict(DGCNN_KNN_WIDE_MIN_C=129)),
    ("DGCNN_KNN_WIDE_MIN_C", "200", dict(DGCNN_KNN_WIDE_MIN_C=129)),
    ("DGCNN_KNN_GRID", "0", dict(DGCNN_KNN_GRID=0)),
    ("DGCNN_KNN_GRID", "1", dict(DGCNN_KNN_GRID=1)),
    ("DGCNN_KNN_GRID", "2", dict(DGCNN_KNN_GRID=1)),                         # only a leading 0 switches it off; mode 2 has no text
    ("DGCNN_KNN_GRID", "off", dict(DGCNN_KNN_GRID=1)),
    ("DGCNN_KNN_GRID_MIN_N", "1024", dict(DGCNN_KNN_GRID_MIN_N=1024)),
    ("DGCNN_KNN_GRID_MIN_N", "junk", dict(DGCNN_KNN_GRID_MIN_N=0)),
    ("DGCNN_KNN_MIX_MIN_N", "400", dict(DGCNN_KNN_MIX_MIN_N=400)),
    ("DGCNN_KNN_MIX_MIN_N", "-5", dict(DGCNN_KNN_MIX_MIN_N=0)),
    ("DGCNN_EDGE_VALU", "0", dict(DGCNN_EDGE_VALU=0)),
    ("DGCNN_EDGE_VALU", "no", dict(DGCNN_EDGE_VALU=1)),
    ("DGCNN_GEMM_ARITH", "f32", dict(DGCNN_GEMM_ARITH=0)),
    ("DGCNN_GEMM_ARITH", "bf16x9", dict(DGCNN_GEMM_ARITH=9)),
    ("DGCNN_GEMM_ARITH", "bf16x1", dict(DGCNN_GEMM_ARITH=1)),
    ("DGCNN_GEMM_ARITH", "9", dict(DGCNN_GEMM_ARITH=9)),
    ("DGCNN_GEMM_ARITH", "zzz", dict(DGCNN_GEMM_ARITH=6)),
    ("DGCNN_EVENT_FLAGS", "0x2", dict(DGCNN_EVENT_FLAGS=2)),                 # strtoul, base 0
    ("DGCNN_EVENT_FLAGS", "010", dict(DGCNN_EVENT_FLAGS=8)),
    ("DGCNN_EVENT_FLAGS", "junk", dict(DGCNN_EVENT_FLAGS=0)),
    ("DGCNN_EVENT_FLAGS", "0x80000002", dict(DGCNN_EVENT_FLAGS=0x80000002 - 2 ** 32)),   # the unsigned's bits as an int
]

# ctypes only (no torch import): prints every switch as dgcnn_switch_get reads it in a fresh process
CHILD = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
out = {}
for name in sys.argv[2:]:
    v = ctypes.c_int(0)
    assert lib.dgcnn_switch_get(name.encode(), ctypes.byref(v)) == 0, name
    out[name] = v.value
print(json.dumps(out))
"""


@pytest.fixture()
def H():
    from dgcnn import _hip
    _hip.load()
    return _hip


def snapshot(H):
    return {name: H.switch(name) for name in NAMES}


def fresh_process_reads(H, var=None, text=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DGCNN_")}
    if var is not None:
        env[var] = text
    out = subprocess.run([sys.executable, "-c", CHILD, H.LIB_PATH] + NAMES, env=env, check=True, capture_output=True, text=True)
    return json.loads(out.stdout)


# ---- (a) dgcnn_switch_get is what the switch's own setter reports as "previous" -------------------------------------------------
def _setter_previous(lib, name):
    """The value in force as the switch's own setter gives it (a query form where it has one, else set and put back)."""
    def swap(fn, probe):
        prev = fn(probe)
        fn(prev)
        return prev
    return {
        "DGCNN_KNN_BF16F": lambda: swap(lib.dgcnn_knn_bf16_filter, 2),
        "DGCNN_KNN_FORCE_VALU": lambda: swap(lib.dgcnn_knn_force_valu, 0),
        "DGCNN_KNN_BIG_K_MIN": lambda: lib.dgcnn_knn_big_k_min(-1),
        "DGCNN_KNN_SEED_MIN_N": lambda: lib.dgcnn_knn_seed_min_n(-2),
        "DGCNN_KNN_APPEND": lambda: lib.dgcnn_knn_append(-1),
        "DGCNN_KNN_APPEND_NPR_LX": lambda: lib.dgcnn_knn_append_products(0),
        "DGCNN_KNN_HIST": lambda: lib.dgcnn_knn_hist(-1),
        "DGCNN_KNN_WIDE_MIN_C": lambda: lib.dgcnn_knn_wide_min_c(-1),
        "DGCNN_KNN_GRID": lambda: swap(lib.dgcnn_knn_grid, 1),
        "DGCNN_KNN_MIX_MIN_N": lambda: lib.dgcnn_knn_seg_mix_min_n(-1),
        "DGCNN_EDGE_VALU": lambda: lib.dgcnn_edge_valu(-1),
        "DGCNN_GEMM_ARITH": lambda: lib.dgcnn_gemm_get_arith(),
        "DGCNN_GEMM_X3_TILE": lambda: swap(lib.dgcnn_gemm_x3_tile_override, 0),
    }.get(name)


# a second value of every switch, different from its default, that its own setter (where it has one) accepts too
OTHER = dict(DGCNN_KNN_BF16F=1, DGCNN_KNN_FORCE_VALU=1, DGCNN_KNN_TIGHTEN_EVERY=2, DGCNN_KNN_BIG_K_MIN=20, DGCNN_KNN_SEED_MIN_N=4096,
             DGCNN_KNN_APPEND=0, DGCNN_KNN_APPEND_NPR_LX=3, DGCNN_KNN_APPEND_NPR_BIG=3, DGCNN_KNN_HIST=4, DGCNN_KNN_WIDE_MIN_C=65,
             DGCNN_KNN_GRID=2, DGCNN_KNN_GRID_MIN_N=1024, DGCNN_KNN_MIX_MIN_N=400, DGCNN_EDGE_VALU=0, DGCNN_GEMM_ARITH=9,
             DGCNN_GEMM_X3_TILE=448, DGCNN_EVENT_FLAGS=2)


@pytest.mark.parametrize("name", NAMES)
def test_get_is_what_the_switch_s_own_setter_calls_previous(H, name):
    """At the value the process started with and at a second one set through dgcnn_switch_set.  The three switches without a
    setter of their own (and the N >= 8192 half of APPEND_NPR, which dgcnn_knn_append_products sets but does not return) are
    held against what was set."""
    lib = H.load()
    query = _setter_previous(lib, name)
    before = H.switch(name)
    try:
        if query is not None:
            assert query() == before
        H.set_switch(name, OTHER[name])
        assert H.switch(name) == OTHER[name]
        if query is not None:
            assert query() == OTHER[name] and H.switch(name) == OTHER[name]
    finally:
        H.set_switch(name, before)
    assert H.switch(name) == before


def test_append_products_sets_both_forms_and_returns_the_lx_one(H):
    lib = H.load()
    before = H.switch("DGCNN_KNN_APPEND_NPR_LX"), H.switch("DGCNN_KNN_APPEND_NPR_BIG")
    try:
        H.set_switch("DGCNN_KNN_APPEND_NPR_LX", 1)
        H.set_switch("DGCNN_KNN_APPEND_NPR_BIG", 3)
        assert lib.dgcnn_knn_append_products(7) == 1                            # query only: nothing moves
        assert (H.switch("DGCNN_KNN_APPEND_NPR_LX"), H.switch("DGCNN_KNN_APPEND_NPR_BIG")) == (1, 3)
        assert lib.dgcnn_knn_append_products(3) == 1
        assert (H.switch("DGCNN_KNN_APPEND_NPR_LX"), H.switch("DGCNN_KNN_APPEND_NPR_BIG")) == (3, 3)
    finally:
        H.set_switch("DGCNN_KNN_APPEND_NPR_LX", before[0])
        H.set_switch("DGCNN_KNN_APPEND_NPR_BIG", before[1])


# ---- (b) the environment parse, one fresh process per case ----------------------------------------------------------------------
def test_defaults_with_nothing_in_the_environment(H):
    assert set(DEFAULTS) == set(NAMES)
    assert fresh_process_reads(H) == DEFAULTS


@pytest.mark.parametrize("var,text,expect", ENV_CASES, ids=["%s=%s" % (c[0][6:], c[1]) for c in ENV_CASES])
def test_environment_parse(H, var, text, expect):
    want = dict(DEFAULTS)
    want.update(expect)
    assert fresh_process_reads(H, var, text) == want


# ---- (c) dgcnn_switch_set refuses what the parse would have replaced ------------------------------------------------------------
REFUSED = dict(DGCNN_KNN_FORCE_VALU=[2, -1], DGCNN_KNN_TIGHTEN_EVERY=[3, 6, -1, -4], DGCNN_KNN_BIG_K_MIN=[0, 66, 99, -1],
               DGCNN_KNN_APPEND=[2, -1], DGCNN_KNN_APPEND_NPR_LX=[0, 2, 7], DGCNN_KNN_APPEND_NPR_BIG=[0, 2, 7],
               DGCNN_KNN_HIST=[3, 8, -1], DGCNN_KNN_WIDE_MIN_C=[4, 130, 200, -1], DGCNN_KNN_GRID=[3, -1], DGCNN_KNN_MIX_MIN_N=[-1, -5],
               DGCNN_EDGE_VALU=[2, -1], DGCNN_GEMM_ARITH=[2, 3, -1], DGCNN_GEMM_X3_TILE=[64, 192, -1])
# every int is a value of these: their parse replaces nothing
ANYTHING = ["DGCNN_KNN_BF16F", "DGCNN_KNN_SEED_MIN_N", "DGCNN_KNN_GRID_MIN_N", "DGCNN_EVENT_FLAGS"]


def test_set_refuses_what_the_parse_would_have_replaced(H):
    assert set(REFUSED) | set(ANYTHING) == set(NAMES)
    lib = H.load()
    before = snapshot(H)
    for name, values in REFUSED.items():
        for v in values:
            assert lib.dgcnn_switch_set(name.encode(), v) == -1, (name, v)
            assert name.encode() in lib.dgcnn_last_error()
            with pytest.raises(ValueError):
                H.set_switch(name, v)
    assert snapshot(H) == before


def test_unknown_names_are_refused_with_the_list_of_known_ones(H):
    lib = H.load()
    v = ctypes.c_int(7)
    for name in (b"DGCNN_KNN_APPEND_NPR", b"DGCNN_NOPE", b"", None):
        assert lib.dgcnn_switch_get(name, ctypes.byref(v)) == -1 and v.value == 7
        msg = lib.dgcnn_last_error().decode()
        assert all(n in msg for n in NAMES), msg
        assert lib.dgcnn_switch_set(name, 1) == -1
        assert all(n in lib.dgcnn_last_error().decode() for n in NAMES)
    assert lib.dgcnn_switch_get(b"DGCNN_KNN_HIST", None) == -1
    with pytest.raises(ValueError):
        H.switch("DGCNN_NOPE")
    with pytest.raises(ValueError):
        H.set_switch("DGCNN_NOPE", 1)


# ---- (d), (e) reading changes nothing -------------------------------------------------------------------------------------------
def test_reading_every_switch_leaves_every_switch_unchanged(H):
    a = snapshot(H)
    for name in NAMES:
        H.switch(name)
    assert snapshot(H) == a


class _Rows(object):
    """What _knn_call_kernels asks of its tensor: the leading dimension (through _hip.ld2) and the address."""

    def __init__(self, rows, C, ld=None, ptr=1 << 20):
        self.shape, self._ld, self._ptr = (rows, C), ld or C, ptr

    def dim(self):
        return 2

    def stride(self, i):
        return (self._ld, 1)[i]

    def data_ptr(self):
        return self._ptr


def test_the_tag_rule_reads_without_setting_anything(H):
    """With a timer set dgcnn._engine names the kernels of every k-NN call (_knn_call_kernels and what it calls): the switches stand
    afterwards as they stood before, at their defaults and at a second value of each."""
    from dgcnn import _engine as E

    def tags():
        out = []
        for C, k, n, kseed, dense in ((3, 20, 1024, 0, True), (3, 20, 8192, 0, True), (64, 20, 2048, 20, True), (64, 20, 8192, 0, True),
                                      (64, 20, 300, 20, False), (128, 20, 300, 0, True), (192, 65, 300, 0, False), (16, 8, 300, 8, True)):
            out.append((E._knn_instance(C, k), E._knn_call_kernels(_Rows(n, C), C, k, n, n, kseed, dense), E._knn_grid_mode(C, k)))
        return out

    prev_timer = H.TIMER
    H.TIMER = H.Timer()
    before = snapshot(H)
    try:
        at_defaults = tags()
        assert snapshot(H) == before
        assert at_defaults[0][1] == ["sqnorm_kernel", "knn_hist_bound_kernel", "knn_kernel"]          # N = 1024 < 4096
        assert at_defaults[1][1] == ["sqnorm_kernel", "knn_grid_*"]
        H.set_switch("DGCNN_KNN_GRID_MIN_N", 1024)
        assert tags()[0][1] == ["sqnorm_kernel", "knn_grid_*"]                                     # the tag follows the switch
        for name in NAMES:
            H.set_switch(name, OTHER[name])
        moved = snapshot(H)
        assert moved == OTHER
        tags()
        assert snapshot(H) == moved
    finally:
        H.TIMER = prev_timer
        for name in NAMES:
            H.set_switch(name, before[name])
    assert snapshot(H) == before

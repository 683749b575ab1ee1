"""The feature-space k-NN (csrc/knn.hip) on adversarial OPERANDS: the clouds of tests/knn_adversarial.py, whose properties
tests/test_knn_adversarial.py pins on the CPU -- bf16 roundings that all go one way (the filters' error at 0.85 ... 0.96 of the
one-product bound and 1.5 ... 1.8 x 2^-16 t for three products), cancellation (d << t: the order hangs on the last bits of s_i, p and
d), near-duplicate clusters (k-th distances negative or exactly zero, a handful of distinct values per row) and all-zero rows (t = 0:
the only way to a seed bound of 0).  Every kernel form, forced the way the other k-NN tests force it; indices equal to the oracle's
(oracle/knn_oracle.c) bit for bit, no tolerance anywhere.

  knn_kernel<CP, KC>                         dgcnn_knn_force_valu(1)
  knn_mfma_kernel<CP, KC, vector / scalar>   the default below N = 8192, unseeded; the scalar loader through a view with ld % 4 != 0
  knn_bf16f_kernel<KC>                       dgcnn_knn_bf16_filter(1) unseeded; seeded with dgcnn_knn_append(0) (C = 16: knn_mfma_kernel
                                             with the seed bound)
  knn_seed_bound_kernel + knn_bf16a_kernel<true, 1 | 3> + knn_select_kernel      seeded, dgcnn_knn_seed_min_n(0), dgcnn_knn_append(1)
  knn_bf16a_kernel<false, 1 | 3>             one cloud of 8200 points (sampled rows against the oracle's row routine)
  knn_kernel / knn_bf16a_kernel<.., PackedClouds>                                 towers with one cloud of each family

Seeds of every seeded form: the row's own exact graph (the tightest legal bound), the same reversed, the graph of unrelated random
features, and on `clusters` k rows of the row's own cluster (a bound that is its slack and nothing else).

Every forced call names the kernel it is for (expect=) and is recorded (tests/launch_trace.py): the kernel, with the template
arguments above, must be among those the call launched -- all forms return the same bits, so nothing else would notice a call that
the dispatch sent elsewhere."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import dgcnn_oracle as O
from gpu_helpers import dev, host
from launch_trace import launches, assert_launched
import knn_adversarial as A

pytestmark = pytest.mark.gpu

_REF = {}


def ref(family, N, C, k):
    """The oracle's lists of a cloud of A.make, computed once."""
    key = (family, N, C, k)
    if key not in _REF:
        r = O.k_nn(A.make(family, N, C, k)[None], k)[0]
        r.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def unrelated(N, k):
    """The oracle's graph of N random points in 8 dimensions: k distinct candidates per row that have nothing to do with the cloud."""
    key = ("unrelated", N, k)
    if key not in _REF:
        _REF[key] = O.k_nn(np.random.default_rng(N + k).random((1, N, 8), dtype=np.float32), k)[0]
    return _REF[key]


@contextlib.contextmanager
def forced(**setters):
    """dgcnn_knn_<name>(value) for every name = value; every previous setting restored on the way out."""
    from dgcnn import _hip as H
    lib = H.load()
    prev = []
    try:
        for name, value in setters.items():
            prev.append((name, getattr(lib, "dgcnn_knn_" + name)(value)))
        yield lib
    finally:
        for name, value in reversed(prev):
            getattr(lib, "dgcnn_knn_" + name)(value)


def check_seeded_path(lib, N, C, k, append, products=None):
    """What decides that a seeded call runs the seeded kernels (dgcnn/_engine.py:knn, knn.hip:knn_impl): the engine passes seeds on,
    the setters hold what the test set, the seed bound takes the width, and the workspace has the append scan's buffers."""
    from dgcnn import _engine as E
    assert E.KNN_SEED, "DGCNN_KNN_SEED=0: the engine would drop the seeds"
    assert lib.dgcnn_knn_seed_min_n(-2) == 0 and lib.dgcnn_knn_append(-1) == append and lib.dgcnn_knn_force_valu(0) == 0
    assert C in (16, 32, 64) and k <= 64
    if append:
        assert lib.dgcnn_knn_append_products(0) == products
        sq = (N * 4 + 255) // 256 * 256
        assert C > 16 and int(lib.dgcnn_knn_workspace_bytes(1, N, C, k)) > 3 * sq + N * 8 * k


def up(x):
    """A cloud on the device (the builders' arrays are shared and read-only: upload a copy)."""
    return dev(np.array(x, np.float32))


def cp_of(C):
    """CP of knn_kernel / knn_mfma_kernel for C <= 128 channels"""
    return 4 if C <= 4 else 16 if C <= 16 else 64 if C <= 64 else 128


def kc_of(k):
    """KC, the list size class of k <= 64"""
    return 8 if k <= 8 else 20 if k <= 20 else 40 if k <= 40 else 64


def knn(xd, N, k, seed=None, seg=None, expect=None):
    """expect: [(kernel, leading template arguments), ...] that must be among the kernels the call launches."""
    from dgcnn import _engine as E
    sd = None if seed is None else dev(np.array(seed, np.int32).reshape(1, N, -1))
    if expect is None:
        return host(E.knn(xd, 1, N, k, seed=sd, seg=seg))[0]
    with launches() as L:
        idx = E.knn(xd, 1, N, k, seed=sd, seg=seg)
    for name, args in expect:
        assert_launched(L, name, args)
    return host(idx)[0]


def seeded_kernels(C, k, form, cl="DenseClouds", lx="true"):
    """What a seeded call of this form is for: the seed bound, then the append-form scan with its selection (C = 32, 64) or, with
    dgcnn_knn_append(0) / at C = 16, the list-keeping scan that takes the bound."""
    f = SEEDED_FORMS[form]
    out = [("knn_seed_bound_kernel", None)]
    if f["append"] and C > 16:
        return out + [("knn_bf16a_kernel", [lx, f["append_products"], cl]), ("knn_select_kernel", [cl])]
    return out + [("knn_mfma_kernel", [16, kc_of(k), "true"]) if C == 16 else ("knn_bf16f_kernel", [kc_of(k)])]


def same(got, want, what):
    bad = np.flatnonzero((got != want).any(-1))
    assert len(bad) == 0, "%s: %d of %d rows differ from the oracle, first row %d: %s vs %s" % (
        what, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]])


def seeds_of(family, x, want, k):
    N = len(x)
    out = {"own graph": want, "own graph reversed": want[:, ::-1], "graph of unrelated features": unrelated(N, k)}
    if family == "clusters":
        out["k rows of the row's own cluster"] = A.cluster_members(x, k)
    return out


SEEDED_FORMS = {"append-1-product": dict(append=1, append_products=1), "append-3-products": dict(append=1, append_products=3),
                "lists": dict(append=0)}


def _path_args(form):
    f = SEEDED_FORMS[form]
    return dict(append=f["append"], products=f.get("append_products"))


# ------------------------------------------------------------------------------------------------------
# unseeded forms
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", A.FAMILIES)
@pytest.mark.parametrize("N,C,k", [c for c in A.CASES if c[1] in (16, 20, 64, 128)])
def test_valu_scan(N, C, k, family):
    with forced(force_valu=1):
        same(knn(up(A.make(family, N, C, k)), N, k, expect=[("knn_kernel", [cp_of(C), kc_of(k), "DenseClouds"])]),
             ref(family, N, C, k), "knn_kernel %s" % ((family, N, C, k),))


@pytest.mark.parametrize("loader", ["vector", "scalar"])
@pytest.mark.parametrize("family", A.FAMILIES)
@pytest.mark.parametrize("N,C,k", [c for c in A.CASES if c[1] in (16, 20, 48, 64)])
def test_mfma_scan(N, C, k, family, loader):
    from dgcnn import _hip as H
    x = A.make(family, N, C, k)
    if loader == "vector":
        xd = up(x)
    else:                                                       # a view into a buffer one column wider: ld = C + 1, not float4-loadable
        buf = torch.full((N, C + 1), 777.0, dtype=torch.float32, device="cuda")
        buf[:, :C] = up(x)
        xd = buf[:, :C]
    assert (H.ld2(xd) % 4 != 0) == (loader == "scalar")
    with forced(force_valu=0, bf16_filter=2):
        same(knn(xd, N, k, expect=[("knn_mfma_kernel", [cp_of(C), kc_of(k), "true" if loader == "vector" else "false"])]),
             ref(family, N, C, k), "knn_mfma_kernel %s" % ((family, N, C, k, loader),))


@pytest.mark.parametrize("family", A.FAMILIES)
@pytest.mark.parametrize("N,C,k", [c for c in A.CASES if 16 < c[1] <= 64])
def test_bf16_filter_scan(N, C, k, family):
    with forced(force_valu=0, bf16_filter=1):
        same(knn(up(A.make(family, N, C, k)), N, k, expect=[("knn_bf16f_kernel", [kc_of(k)])]), ref(family, N, C, k),
             "knn_bf16f_kernel %s" % ((family, N, C, k),))


# ------------------------------------------------------------------------------------------------------
# seeded forms (the seed bound takes C = 16, 32, 64; the append-form scan 32 and 64)
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(SEEDED_FORMS))
@pytest.mark.parametrize("family", A.FAMILIES)
@pytest.mark.parametrize("N,C,k", [c for c in A.CASES if c[1] in (16, 32, 64)])
def test_seeded_scan_whatever_the_seeds(N, C, k, family, form):
    x = A.make(family, N, C, k)
    want = ref(family, N, C, k)
    xd = up(x)
    with forced(force_valu=0, bf16_filter=2, seed_min_n=0, **SEEDED_FORMS[form]) as lib:
        if C > 16 or form == "lists":
            check_seeded_path(lib, N, C, k, **_path_args(form))
        same(knn(xd, N, k), want, "unseeded %s" % ((family, N, C, k),))
        for name, sd in seeds_of(family, x, want, k).items():
            same(knn(xd, N, k, seed=sd, expect=seeded_kernels(C, k, form)), want, "%s, seeds: %s %s" % (form, name, (family, N, C, k)))


@pytest.mark.parametrize("form", sorted(SEEDED_FORMS))
@pytest.mark.parametrize("N,C,k", [c for c in A.CASES if c[1] in (16, 32, 64)])
def test_seeded_scan_with_a_seed_bound_of_zero(N, C, k, form):
    """All-zero rows seeded with their own graph: tau0 = 0, the threshold is the smallest denormal and only d <= 0 may stay -- the
    k lowest-numbered zero rows, for every zero row."""
    x, zr = A.zero_rows(N, C, k)
    want = O.k_nn(x[None], k)[0]
    xd = up(x)
    with forced(force_valu=0, bf16_filter=2, seed_min_n=0, **SEEDED_FORMS[form]) as lib:
        if C > 16 or form == "lists":
            check_seeded_path(lib, N, C, k, **_path_args(form))
        for name, sd in (("own graph", want), ("own graph reversed", want[:, ::-1]), ("graph of unrelated features", unrelated(N, k))):
            got = knn(xd, N, k, seed=sd, expect=seeded_kernels(C, k, form))
            same(got[zr], want[zr], "%s, zero rows, seeds: %s %s" % (form, name, (N, C, k)))
            same(got, want, "%s, seeds: %s %s" % (form, name, (N, C, k)))


@pytest.mark.parametrize("products", [1, 3])
def test_seeded_scan_past_8192_points(products):
    """knn_bf16a_kernel<false, NPR>: one `mixed` cloud of 8200 points, C = 64, k = 20.  512 sampled rows against the oracle's row routine;
    the seeded results equal to the unseeded one (knn_bf16f_kernel at this size) on every row."""
    from dgcnn import _engine as E
    N, C, k = 8200, 64, 20
    x = A.make("mixed", N, C, k)
    rows = np.sort(np.random.default_rng(N).choice(N, 512, replace=False)).astype(np.int32)
    key = ("rows", N, C, k)
    if key not in _REF:
        _REF[key] = O.k_nn_rows(x, k, rows)
    want = _REF[key]
    xd = up(x)
    with forced(force_valu=0, bf16_filter=2, seed_min_n=0, append=1, append_products=products) as lib:
        check_seeded_path(lib, N, C, k, 1, products)
        plain = knn(xd, N, k, expect=[("knn_bf16f_kernel", [20])])
        same(plain[rows], want, "unseeded, N = 8200")
        other = host(E.knn(dev(np.random.default_rng(3).random((N, 3), dtype=np.float32)), 1, N, k))[0]
        for name, sd in (("own graph", plain), ("own graph reversed", plain[:, ::-1]), ("graph of unrelated features", other)):
            got = knn(xd, N, k, seed=sd, expect=[("knn_seed_bound_kernel", None), ("knn_bf16a_kernel", ["false", products, "DenseClouds"]),
                                                 ("knn_select_kernel", ["DenseClouds"])])
            same(got[rows], want, "%d products, seeds: %s, N = 8200" % (products, name))
            np.testing.assert_array_equal(got, plain, err_msg=name)


# ------------------------------------------------------------------------------------------------------
# packed towers: one cloud of each family, unaligned sizes, neighbouring clouds 2^+-12 apart in norm
# ------------------------------------------------------------------------------------------------------
def packed(C, k):
    """(tower (R, C), offsets, oracle lists as tower rows (R, k), [(family, first row, rows)])."""
    key = ("tower", C, k)
    if key not in _REF:
        clouds = A.tower(C, k)
        off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
        want = np.concatenate([O.k_nn(c[None], k)[0] + off[b] for b, c in enumerate(clouds)], 0).astype(np.int32)
        spec = [(f, int(off[b]), len(clouds[b])) for b, (f, _, _) in enumerate(A.tower_spec(C, k))]
        _REF[key] = (np.concatenate(clouds, 0), off, want, spec)
    return _REF[key]


@pytest.mark.parametrize("C,k", [s for s in A.TOWER_SHAPES if s[0] in (16, 20, 64, 128)])
def test_packed_scan(C, k):
    from dgcnn import _engine as E
    x, off, want, _ = packed(C, k)
    with forced(force_valu=0, bf16_filter=2):
        same(knn(up(x), len(x), k, seg=E.Segments(off, len(x)), expect=[("knn_kernel", [cp_of(C), kc_of(k), "PackedClouds"])]), want,
             "packed knn_kernel %s" % ((C, k),))


@pytest.mark.parametrize("products", [1, 3])
@pytest.mark.parametrize("C,k", [s for s in A.TOWER_SHAPES if s[0] in (32, 64)])
def test_packed_seeded_scan_whatever_the_seeds(C, k, products):
    from dgcnn import _engine as E
    x, off, want, spec = packed(C, k)
    R = len(x)
    seg = E.Segments(off, R)
    other = np.concatenate([unrelated(n, k) + r0 for _, r0, n in spec], 0)
    members = want.copy()                                      # k rows of the row's own cluster, for the rows of the `clusters` cloud
    for f, r0, n in spec:
        if f == "clusters":
            members[r0:r0 + n] = A.cluster_members(x[r0:r0 + n], k) + r0
    xd = up(x)
    with forced(force_valu=0, bf16_filter=2, seed_min_n=0, append=1, append_products=products) as lib:
        check_seeded_path(lib, seg.max_n, C, k, 1, products)
        for name, sd in (("own graph", want), ("own graph reversed", want[:, ::-1]), ("graph of unrelated features", other),
                         ("clusters: k rows of the row's own cluster", members)):
            same(knn(xd, R, k, seed=sd, seg=seg, expect=[("knn_seed_bound_kernel", None), ("knn_bf16a_kernel", ["true", products, "PackedClouds"]),
                                                         ("knn_select_kernel", ["PackedClouds"])]), want,
                 "packed, %d products, seeds: %s %s" % (products, name, (C, k)))

"""Every k-NN form (csrc/knn.hip, csrc/knn_grid.hip) on NON-FINITE input: the clouds of tests/knn_nonfinite.py (a NaN in one point,
NaN points that every stride of the histogram bound samples, infinities of both signs, squares and sums that overflow, clouds with
fewer than k finite points, clouds of NaN only), whose properties and whose oracle lists tests/test_knn_nonfinite.py pins on the CPU.
The rule (include/dgcnn_hip.h K1, oracle/knn_oracle.c): candidate j of row i has the key (D~_ij, j), D~ = +inf where D_ij is NaN; idx[i]
= the k smallest keys, ascending, ties to the lower j.  Every row of every cloud is compared with the oracle: no tolerance, no row
left out (one cloud of 8200 points: sampled rows, the bad rows and their neighbours by index always among them), and before that
comparison the host asserts that every index lies inside the row's own cloud.

Forms, forced the way tests/test_gpu_knn_adversarial.py and tests/test_gpu_knn_grid.py force them (their helpers, imported):

  knn_hist_bound_kernel<1 | 2 | 4> + knn_kernel<4, KC>     C in {3, 4}, dgcnn_knn_grid(0), dgcnn_knn_hist(0 | 1 | 2 | 4)
  knn_kernel<CP, KC>                                       dgcnn_knn_force_valu(1), C in {16, 20, 128}
  knn_mfma_kernel<CP, KC, vector | scalar>                 the default below N = 8192, unseeded; scalar: a view with ld % 4 != 0
  knn_bf16f_kernel<KC>                                     dgcnn_knn_bf16_filter(1) unseeded; seeded with dgcnn_knn_append(0)
  knn_seed_bound_kernel + knn_bf16a_kernel<true, 1 | 3> + knn_select_kernel      dgcnn_knn_seed_min_n(0), dgcnn_knn_append(1)
  knn_bf16a_kernel<false, 1 | 3>                           one cloud of 8200 points
  knn_grid_build_kernel + knn_grid_query_kernel            dgcnn_knn_grid(2), C in {1, 2, 3, 4}
  packed towers                                            dgcnn_knn_seg_f32 (C = 3 with the histogram bound, C = 64 unseeded and seeded),
                                                           dgcnn_knn_seg_grid_f32, dgcnn_knn_seg_mix_f32; one bad cloud between finite ones
  the default dispatch                                     dgcnn.ops.k_nn, nothing forced, (1, 333, 3, 8) and (2, 2048, 3, 20)

Seeds of every seeded form, none of which may change the result: the oracle's own graph of the cloud (in few_finite it holds bad
points: a seed at a NaN distance), the same reversed, the graph of unrelated features.

WHY THESE RUNS ARE SAFE.  The kernel-level tests call k-NN entries only, which write idx and their own workspace and nothing else; no
graph goes to a gather, an edge kernel or the model before the host has asserted 0 <= idx < N on it.  No trip count or store address
of a form depends on a distance or a coordinate being finite (read from the code):
  sqnorm_kernel            loops over C and the block's rows only.
  knn_hist_bound_kernel    loops over N; the bin is integer arithmetic on the float's bits, clamped to [0, 47] on both sides whatever the
                           bits; the cloud's largest s_j starts from 0 and takes fmaxf (a NaN drops out, +inf gives the largest exponent).
  list forms               tile loops over N; the drain pops one bit of a 32-bit (16-bit) mask per trip; parked distances are indexed
                           by the bit's number; the merge walks KC entries; rows past N and candidates past N are clamped.  The new
                           fill of a short row runs v < N and c < k and stores to out[c] only.
  knn_seed_bound_kernel    loops over k; a seed outside [0, N) (of the row's own cloud) is replaced by row 0 before any load.
  knn_bf16a_kernel         a wave's re-check queue holds 128 entries and is emptied whenever 64 wait: at most 63 + 64 are ever in it,
                           by COUNT; a row's buffer takes at most 64 (192) appends between two tile boundaries and is compacted to k
                           entries when it passes cap minus that, by COUNT; a NaN or +inf distance is never appended (d < thr fails), so
                           "every key at +inf" cannot occur in a buffer, and -inf has an ordinary key (next_up(-inf) = -FLT_MAX); the
                           level histogram's field index is a count of seven comparisons.
  knn_select_kernel        reads S <= cap entries; the fill of a short row walks S < k <= 64 lanes and stores to out[p], p < k.
  cell grid                a cell coordinate is clamped to [0, G - 1] after the conversion (NaN -> 0, out of range saturates); runs come from
                           the cell table; at most 16 candidates are parked between two drains, by COUNT; the ring loop ends at GMAX, or
                           when lb == INFINITY once the ring covers the grid; every comparison of the stop test is false for a NaN.
The end-to-end test (the model on a packed tower with a NaN in the middle cloud) comes last, refuses to run when a kernel-level test
of this module has failed in the same process, calls the packed k-NN alone first and asserts on the host that every index lies inside
its cloud, and checks every graph the model computes the same way before the model may gather with it."""
import numpy as np
import pytest
import torch

from oracle import dgcnn_oracle as O
from gpu_helpers import dev, host, set_vars
import knn_nonfinite as NF
from test_gpu_knn_adversarial import (forced, check_seeded_path, knn, up, unrelated, SEEDED_FORMS, _path_args, cp_of, kc_of,
                                       seeded_kernels)
from test_gpu_packed_mix import seg_mix_call, classes

pytestmark = pytest.mark.gpu

_REF = {}
_FAILED = []                     # kernel-level comparisons that failed in this process (the end-to-end test looks here first)


@pytest.fixture()
def dg():
    import dgcnn
    dgcnn.reset()
    yield dgcnn
    dgcnn.reset()


def ref(family, N, C, k):
    """[(label, cloud, the oracle's lists)] of a family at a shape, computed once."""
    key = (family, N, C, k)
    if key not in _REF:
        out = []
        for label, x in NF.variants(family, N, C, k):
            r = O.k_nn(x[None], k)[0]
            r.setflags(write=False)
            out.append((label, x, r))
        _REF[key] = out
    return _REF[key]


def same(got, want, lo, n, what):
    """Every index of got inside [lo, lo + n) (asserted first, on the host), then every row equal to the oracle's."""
    got = np.asarray(got).reshape(want.shape)
    out = ((got < lo) | (got >= lo + n)).any(-1)
    bad = (got != want).any(-1)
    if out.any() or bad.any():
        _FAILED.append(what)
        first = int(np.flatnonzero(out | bad)[0])
        raise AssertionError("%s: %d rows hold an index outside the cloud, %d of %d rows differ from the oracle; first row %d: %s vs %s"
                             % (what, int(out.sum()), int(bad.sum()), len(want), first, got[first], want[first]))


def cases(cs, shapes=None, families=NF.FAMILIES):
    """[(family, N, C, k)] over the families' shapes (few_finite: N = 40, k = 20 as well) that a family fits."""
    return [(f, N, C, k) for f in families for (N, k) in (NF.shapes_of(f) if shapes is None else shapes) for C in cs if NF._fits(f, N, C, k)]


def ids(cs):
    return ["%s-N%d-C%d-k%d" % c for c in cs]


# ------------------------------------------------------------------------------------------------------
# unseeded forms
# ------------------------------------------------------------------------------------------------------
RAW = cases(NF.C_RAW) + cases(NF.C_RAW, NF.HIST_SHAPES)


@pytest.mark.parametrize("hist", [0, 1, 2, 4])
@pytest.mark.parametrize("family,N,C,k", RAW, ids=ids(RAW))
def test_raw_coordinate_scan_with_the_histogram_bound(family, N, C, k, hist):
    """knn_kernel<4, KC> behind knn_hist_bound_kernel<hist> (no bound: hist = 0, a cloud under 256 points, or N < 4 k hist)."""
    with forced(grid=0, force_valu=0, hist=hist) as lib:
        assert lib.dgcnn_knn_seg_grid_use(C, k, 1, 1, 1, 1, 1 << 62) == 0      # the cell grid is off: the scan takes every N
        assert lib.dgcnn_knn_hist(-1) == hist and lib.dgcnn_knn_force_valu(0) == 0
        for label, x, want in ref(family, N, C, k):
            expect = [("knn_kernel", [4, kc_of(k), "DenseClouds"])]
            if hist and N >= 256 and N >= 4 * k * hist:
                expect.append(("knn_hist_bound_kernel", [hist, "DenseClouds"]))
            same(knn(up(x), N, k, expect=expect), want, 0, N, "form=hist%d+knn_kernel family=%s (%s) %s" % (hist, family, label, (N, C, k)))


VALU = cases(NF.C_VALU)


@pytest.mark.parametrize("family,N,C,k", VALU, ids=ids(VALU))
def test_valu_scan(family, N, C, k):
    with forced(force_valu=1):
        for label, x, want in ref(family, N, C, k):
            same(knn(up(x), N, k, expect=[("knn_kernel", [cp_of(C), kc_of(k), "DenseClouds"])]), want, 0, N,
                 "form=knn_kernel family=%s (%s) %s" % (family, label, (N, C, k)))


MFMA = cases(NF.C_MFMA)


@pytest.mark.parametrize("loader", ["vector", "scalar"])
@pytest.mark.parametrize("family,N,C,k", MFMA, ids=ids(MFMA))
def test_mfma_scan(family, N, C, k, loader):
    from dgcnn import _hip as H
    with forced(force_valu=0, bf16_filter=2):
        for label, x, want in ref(family, N, C, k):
            if loader == "vector":
                xd = up(x)
            else:                                               # a view into a buffer one column wider: ld = C + 1, not float4-loadable
                buf = torch.full((N, C + 1), 777.0, dtype=torch.float32, device="cuda")
                buf[:, :C] = up(x)
                xd = buf[:, :C]
            assert (H.ld2(xd) % 4 != 0) == (loader == "scalar")
            same(knn(xd, N, k, expect=[("knn_mfma_kernel", [cp_of(C), kc_of(k), "true" if loader == "vector" else "false"])]), want, 0, N,
                 "form=knn_mfma_kernel-%s family=%s (%s) %s" % (loader, family, label, (N, C, k)))


BF16F = cases(NF.C_BF16F)


@pytest.mark.parametrize("family,N,C,k", BF16F, ids=ids(BF16F))
def test_bf16_filter_scan(family, N, C, k):
    with forced(force_valu=0, bf16_filter=1):
        for label, x, want in ref(family, N, C, k):
            same(knn(up(x), N, k, expect=[("knn_bf16f_kernel", [kc_of(k)])]), want, 0, N,
                 "form=knn_bf16f_kernel family=%s (%s) %s" % (family, label, (N, C, k)))


# ------------------------------------------------------------------------------------------------------
# seeded forms (the seed bound takes C = 16, 32, 64; the append-form scan 32 and 64)
# ------------------------------------------------------------------------------------------------------
def seeds_of(want, N, k):
    return (("own graph", want), ("own graph reversed", want[:, ::-1]), ("graph of unrelated features", unrelated(N, k)))


SEEDED = cases(NF.C_SEEDED)


@pytest.mark.parametrize("form", sorted(SEEDED_FORMS))
@pytest.mark.parametrize("family,N,C,k", SEEDED, ids=ids(SEEDED))
def test_seeded_scan_whatever_the_seeds(family, N, C, k, form):
    """lists: knn_bf16f_kernel (C = 16: knn_mfma_kernel) behind the seed bound; append-*: knn_bf16a_kernel<true, 1 | 3> and the
    selection (C = 16 is not the append form's: it runs the lists there too)."""
    with forced(force_valu=0, bf16_filter=2, seed_min_n=0, **SEEDED_FORMS[form]) as lib:
        if C > 16 or form == "lists":
            check_seeded_path(lib, N, C, k, **_path_args(form))
        for label, x, want in ref(family, N, C, k):
            xd = up(x)
            for name, sd in seeds_of(want, N, k):
                same(knn(xd, N, k, seed=sd, expect=seeded_kernels(C, k, form)), want, 0, N,
                     "form=seeded-%s family=%s (%s) seeds=%s %s" % (form, family, label, name, (N, C, k)))


@pytest.mark.parametrize("products", [1, 3])
@pytest.mark.parametrize("family", NF.FAMILIES)
def test_seeded_scan_past_8192_points(family, products):
    """knn_bf16a_kernel<false, NPR>: one cloud of 8200 points, C = 64, k = 20.  Sampled rows -- the bad rows and their neighbours by
    index always among them -- against the oracle's row routine; EVERY row inside the cloud and k distinct indices; the seeded results
    equal to the unseeded one (knn_bf16f_kernel at this size) on every row."""
    from dgcnn import _engine as E
    N, C, k = NF.BIG_CLOUD
    label, x = NF.variants(family, N, C, k)[0]
    rows = NF.sample_rows(x)
    key = ("rows", family, N, C, k)
    if key not in _REF:
        _REF[key] = O.k_nn_rows(x, k, rows)
    want = _REF[key]
    xd = up(x)
    what = "family=%s (%s) N=8200" % (family, label)
    with forced(force_valu=0, bf16_filter=2, seed_min_n=0, append=1, append_products=products) as lib:
        check_seeded_path(lib, N, C, k, 1, products)
        plain = knn(xd, N, k, expect=[("knn_bf16f_kernel", [20])])
        assert plain.min() >= 0 and plain.max() < N, "form=knn_bf16f_kernel %s: an index outside the cloud" % what
        assert (np.diff(np.sort(plain, 1), axis=1) > 0).all(), "form=knn_bf16f_kernel %s: a row lists an index twice" % what
        same(plain[rows], want, 0, N, "form=knn_bf16f_kernel %s" % what)
        other = host(E.knn(dev(np.random.default_rng(3).random((N, 3), dtype=np.float32)), 1, N, k))[0]
        for name, sd in (("own graph", plain), ("own graph reversed", plain[:, ::-1]), ("graph of unrelated features", other)):
            got = knn(xd, N, k, seed=sd, expect=[("knn_seed_bound_kernel", None), ("knn_bf16a_kernel", ["false", products, "DenseClouds"]),
                                                 ("knn_select_kernel", ["DenseClouds"])])
            same(got[rows], want, 0, N, "form=knn_bf16a_kernel<false,%d> %s seeds=%s" % (products, what, name))
            same(got, plain, 0, N, "form=knn_bf16a_kernel<false,%d> against the unseeded search, %s seeds=%s" % (products, what, name))


# ------------------------------------------------------------------------------------------------------
# dense cell grid
# ------------------------------------------------------------------------------------------------------
GRID = [(f, N, C, NF.grid_k(N)) for f in NF.FAMILIES for N in NF.GRID_N for C in NF.C_GRID if NF._fits(f, N, C, NF.grid_k(N))
        and not (f == "hist_trap" and N == 5)] + [(f, 2048, 3, 40) for f in NF.FAMILIES]


@pytest.mark.parametrize("family,N,C,k", GRID, ids=ids(GRID))
def test_cell_grid(family, N, C, k):
    with forced(grid=2, force_valu=0) as lib:
        assert lib.dgcnn_knn_seg_grid_use(C, k, 1, 1, 1, 1, 0) == 1          # mode 2: the grid whenever applicable
        for label, x, want in ref(family, N, C, k):
            expect = [("knn_grid_build_kernel", ["DenseClouds"]),
                      ("knn_grid_query_kernel", [8 if k <= 8 else 20 if k <= 20 else 40, "true" if C == 4 else "false"])]
            same(knn(up(x), N, k, expect=expect), want, 0, N, "form=cell-grid family=%s (%s) %s" % (family, label, (N, C, k)))


# ------------------------------------------------------------------------------------------------------
# packed towers: one bad cloud between finite ones -- first, in the middle, last
# ------------------------------------------------------------------------------------------------------
TOWER = (300, 200, 270)          # at threshold 256 of the mix entry: grid, scan, grid; 300 and 270 run the histogram bound alone


def tower(family, C, k, place, sizes=TOWER):
    """(x (R, C), offsets, the oracle's lists as tower rows, place of the bad cloud): finite clouds are NF.base with their own seed."""
    key = ("tower", family, C, k, place, sizes)
    if key not in _REF:
        clouds = [NF.variants(family, n, C, k)[0][1] if b == place else NF.base(n, C, seed=b + 1) for b, n in enumerate(sizes)]
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        want = [O.k_nn(c[None], k)[0] + off[b] for b, c in enumerate(clouds)]
        _REF[key] = (np.concatenate(clouds, 0), off, [w.astype(np.int32) for w in want])
    return _REF[key]


def check_tower(idx, off, want, what):
    idx = np.asarray(idx).reshape(-1, want[0].shape[1])
    for b, w in enumerate(want):
        same(idx[off[b]:off[b + 1]], w, int(off[b]), int(off[b + 1] - off[b]), "%s cloud=%d" % (what, b))


@pytest.mark.parametrize("place", [0, 1, 2])
@pytest.mark.parametrize("family", NF.FAMILIES)
@pytest.mark.parametrize("sizes", [TOWER, (300, 333, 270)], ids=["hist-off", "hist-on"])
def test_packed_scan_raw_coordinates(family, place, sizes):
    """dgcnn_knn_seg_f32, C = 3: knn_kernel<4, 8, PackedClouds>; with every cloud at 256 points or more behind the histogram bound."""
    from dgcnn import _engine as E
    x, off, want = tower(family, 3, 8, place, sizes)
    with forced(grid=0, force_valu=0, hist=2):
        expect = [("knn_kernel", [4, 8, "PackedClouds"])] + ([("knn_hist_bound_kernel", [2, "PackedClouds"])] if min(sizes) >= 256 else [])
        got = knn(up(x), len(x), 8, seg=E.Segments(off, len(x)), expect=expect)
        check_tower(got, off, want, "form=packed-scan-C3-%s family=%s bad=%d" % ("hist" if min(sizes) >= 256 else "nohist", family, place))


@pytest.mark.parametrize("place", [0, 1, 2])
@pytest.mark.parametrize("family", NF.FAMILIES)
def test_packed_scan_features(family, place):
    """dgcnn_knn_seg_f32, C = 64, k = 8: knn_kernel<64, 8, PackedClouds> unseeded, then the packed append-form scan (1 and 3 products)
    with every kind of seed."""
    from dgcnn import _engine as E
    x, off, want = tower(family, 64, 8, place)
    R = len(x)
    seg = E.Segments(off, R)
    xd = up(x)
    what = "family=%s bad=%d" % (family, place)
    with forced(force_valu=0, bf16_filter=2):
        check_tower(knn(xd, R, 8, seg=seg, expect=[("knn_kernel", [64, 8, "PackedClouds"])]), off, want, "form=packed-scan-C64 " + what)
    full = np.concatenate(want, 0)
    other = np.concatenate([unrelated(int(n), 8) + off[b] for b, n in enumerate(np.diff(off))], 0).astype(np.int32)
    for products in (1, 3):
        with forced(force_valu=0, bf16_filter=2, seed_min_n=0, append=1, append_products=products) as lib:
            check_seeded_path(lib, seg.max_n, 64, 8, 1, products)
            for name, sd in (("own graph", full), ("own graph reversed", full[:, ::-1]), ("graph of unrelated features", other)):
                expect = [("knn_seed_bound_kernel", None), ("knn_bf16a_kernel", ["true", products, "PackedClouds"]),
                          ("knn_select_kernel", ["PackedClouds"])]
                check_tower(knn(xd, R, 8, seed=sd, seg=seg, expect=expect), off, want,
                            "form=packed-append-%d %s seeds=%s" % (products, what, name))


@pytest.mark.parametrize("place", [0, 1, 2])
@pytest.mark.parametrize("family", NF.FAMILIES)
@pytest.mark.parametrize("C", [3, 4])
def test_packed_cell_grid(family, place, C):
    """dgcnn_knn_seg_grid_f32: one grid per cloud."""
    from dgcnn import _engine as E
    x, off, want = tower(family, C, 8, place)
    with forced(grid=2, force_valu=0) as lib:
        n = np.diff(off)
        assert lib.dgcnn_knn_seg_grid_use(C, 8, len(n), len(x), int(n.min()), int(n.max()), int((n * n).sum())) == 1
        expect = [("knn_grid_build_kernel", ["PackedClouds"]),
                  ("knn_grid_query_kernel", [8, "true" if C == 4 else "false", "false", "PackedClouds"])]
        check_tower(knn(up(x), len(x), 8, seg=E.Segments(off, len(x)), expect=expect), off, want,
                    "form=packed-grid-C%d family=%s bad=%d" % (C, family, place))


@pytest.mark.parametrize("place", [0, 1, 2])
@pytest.mark.parametrize("family", NF.FAMILIES)
def test_packed_mix(family, place):
    """dgcnn_knn_seg_mix_f32 at threshold 256, as tests/test_gpu_packed_mix.py calls it: clouds 0 and 2 through the cell grid, cloud 1
    through the scan -- the bad cloud in either class."""
    x, off, want = tower(family, 3, 8, place)
    assert classes(off, 256)[1] == 2
    with forced(force_valu=0, hist=2):
        check_tower(host(seg_mix_call(x, off, 3, 8, 256)), off, want, "form=packed-mix family=%s bad=%d" % (family, place))


# ------------------------------------------------------------------------------------------------------
# the default dispatch
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,k", [(1, 333, 8), (2, 2048, 20)], ids=["1x333", "2x2048"])
def test_default_dispatch_on_hist_trap(dg, B, N, k):
    """dgcnn.ops.k_nn with nothing forced; (B, 2048, 3, 20) is the shape a user runs (the histogram bound at its default stride)."""
    vs = ref("hist_trap", N, 3, k)
    for v in range(len(vs)):
        batch = [vs[(v + b) % len(vs)] for b in range(B)]
        got = host(dg.ops.k_nn(dev(np.stack([x for _, x, _ in batch])), k))
        for b, (label, _, want) in enumerate(batch):
            same(got[b], want, 0, N, "form=default-dispatch family=hist_trap (%s) %s cloud=%d" % (label, (B, N, 3, k), b))


# ------------------------------------------------------------------------------------------------------
# end to end, packed: a NaN in one cloud stays in that cloud
# ------------------------------------------------------------------------------------------------------
def test_end_to_end_a_nan_in_one_cloud_leaves_the_other_clouds_logits_alone(dg, monkeypatch):
    """A packed tower of three clouds (300, 333, 270 points; C = 4, k = 8) under BN_PER_CLOUD (batch-independent inference, the flags
    of tests/test_gpu_seg_bn.py), once with a NaN coordinate in the middle cloud and once with that coordinate finite: the logits of
    clouds 0 and 2 are bit-identical between the two runs."""
    import dgcnn
    from dgcnn import _engine as E
    assert not _FAILED, "kernel-level k-NN comparisons failed in this process (%d, first: %s): the model is not built on such graphs" % (
        len(_FAILED), _FAILED[0])
    sizes = (300, 333, 270)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    R = int(off[-1])
    rng = np.random.default_rng(41)
    clean = rng.random((R, 4), dtype=np.float32)
    bad = clean.copy()
    bad[off[1] + 64, 2] = np.nan
    cloud_lo = np.repeat(off[:-1], sizes)[:, None]
    cloud_hi = np.repeat(off[1:], sizes)[:, None]

    def inside(idx, what):
        g = host(idx).reshape(R, -1)
        assert ((g >= cloud_lo) & (g < cloud_hi)).all(), "%s: an index outside the row's own cloud" % what

    # the packed k-NN alone on both inputs, checked on the host, before any model is built
    for name, pts in (("clean", clean), ("NaN", bad)):
        idx = dg.ops.k_nn(dev(pts), 8, offsets=off)
        inside(idx, "k-NN alone, %s input" % name)
        for b in range(3):
            want = O.k_nn(pts[None, off[b]:off[b + 1]], 8)[0] + off[b]
            same(host(idx).reshape(R, 8)[off[b]:off[b + 1]], want.astype(np.int32), int(off[b]), sizes[b], "end-to-end k-NN alone, %s cloud=%d" % (name, b))

    real_knn = E.knn

    def checked_knn(x2d, B, N, k, seed=None, seg=None):               # every graph of the model: host-checked before anything gathers with it
        idx = real_knn(x2d, B, N, k, seed=seed, seg=seg)
        torch.cuda.synchronize()
        inside(idx, "a graph of the model (C = %d)" % x2d.shape[1])
        return idx
    monkeypatch.setattr(E, "knn", checked_knn)

    flags = dg.DGCNN_FLAGS(MODEL_NAME="dgcnn", EDGE_CONV_LAYERS=2, EDGE_CONV_FILTERS=[32, 64], KVALUE=8, NUM_CLASS=3, FC_LAYERS=2,
                           FC_FILTERS=[64, 32], TRAIN=False, NUM_CHANNEL=4, BN_PER_CLOUD=True)
    params = O.init_params(flags, 4, seed=1)
    for n in params:
        if n.endswith("beta"):
            params[n] = rng.normal(0, 0.2, params[n].shape).astype(np.float32)
    logits = {}
    for name, pts in (("clean", clean), ("NaN", bad)):
        dg.trainval(flags).initialize()
        set_vars(dg, params)
        logits[name] = host(dgcnn.build(dev(pts), flags, offsets=off)).reshape(R, 3)
    assert np.isfinite(logits["clean"]).all()
    for b in (0, 2):
        lo, hi = int(off[b]), int(off[b + 1])
        np.testing.assert_array_equal(logits["NaN"][lo:hi], logits["clean"][lo:hi], err_msg="cloud %d" % b)

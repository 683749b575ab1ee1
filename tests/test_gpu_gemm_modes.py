"""The single-product bf16 arithmetic of dgcnn_gemm_f32 and the plane GEMM at their tile edges (run with -m gpu on an MI355X).

A. dgcnn_gemm_set_arith(1) -- operands rounded once to bf16 (round to nearest even), fp32 accumulation -- has instantiations of its
   own in csrc/gemm_x3.hip: gemm_x3_kernel<64 | 128 columns, 1> and gemm_x3w2_kernel<1>, each in the NN, NT and TN operand forms,
   with their own staging code (write<1>, stage<MASK, 1>).  The reference is float64 of the ROUNDED operands
   (oracle.bf16_round); the bar on the random and ties tiers is REL_BAR of tests/test_gpu_gemm_tiles.py, relative to |A^| |B^|.
B. dgcnn_gemm_planes_f32 (csrc/gemm_pl.hip, DGCNN_PLANES_F16X2): 256 x 128 tiles, loader waves, three LDS stages; the KC form
   with every epilogue on ragged shapes, the TR form (ds_read_tr) with and without split-K, and what the entry refuses.

Operand tiers (tests/gemm_modes_reference.py; their preconditions are asserted on the host in tests/test_gemm_modes_reference.py):
lattice and ternary operands make every fp32 partial sum exact, so a kernel must EQUAL the int64 product / column sums whatever
its summation order; ties operands sit halfway between two bf16 values, so a wrong rounding moves every element; random operands
are held to the float64 bars.  The worst ratio to its bar per kernel and tier is printed at the end of the module
($DGCNN_GEMM_MODES_ERROR_TABLE writes it; profiles/gemm_modes_errors.txt holds a measured copy)."""
import os

import numpy as np
import pytest
import torch

import gemm_modes_reference as R
from gpu_helpers import dev, host
from test_gpu_gemm_planes import _err
from test_gpu_gemm_tiles import CONFIGS, REL_BAR, assert_colmax, assert_colsums, check_forced, decode, kernel_name, tile

pytestmark = pytest.mark.gpu

PLANE_BAR = 6e-7          # tests/test_gpu_gemm_planes.py: 2^-22 per operand, worst case 2 x 2.4e-7 + the dropped h2 h2 term
NAN = float("nan")
RPG = 100                 # rows per bias group: no multiple of any tile height, groups straddle the row tiles
WORST = {}                # (kernel, tier) -> [worst error / bar (0 on the exact tiers: equality), checks]
LAYOUTS = ("NN", "NT", "TN")
KINDS = {"NN": ("KCONTIG", "KSTRIDED"), "NT": ("KCONTIG", "KCONTIG"), "TN": ("KSTRIDED", "KSTRIDED")}


@pytest.fixture()
def dg():
    import dgcnn
    dgcnn.reset()
    return dgcnn


@pytest.fixture(scope="module", autouse=True)
def _error_table():
    yield
    lines = ["# worst measured error / bar per kernel and operand tier over tests/test_gpu_gemm_modes.py.  dgcnn_gemm_f32: error relative",
             "# to |A^| |B^| of the bf16-rounded operands (raw operands on the unrounded paths) against REL_BAR = %g; plane GEMM: error" % REL_BAR,
             "# relative to |A| |B| against %g.  lattice / ternary: held to equality with the int64 result (ratio 0 by assertion)." % PLANE_BAR,
             "%-58s %-8s %12s %8s" % ("kernel", "tier", "worst / bar", "checks")]
    for (kernel, tier) in sorted(WORST):
        r, n = WORST[(kernel, tier)]
        lines.append("%-58s %-8s %12.4g %8d" % (kernel, tier, r, n))
    text = "\n".join(lines) + "\n"
    print("\n" + text)
    path = os.environ.get("DGCNN_GEMM_MODES_ERROR_TABLE")
    if path:
        with open(path, "w") as f:
            f.write(text)


def note(kernel, tier, ratio):
    w = WORST.setdefault((kernel, tier), [0.0, 0])
    w[0] = max(w[0], float(ratio))
    w[1] += 1


def instance(M, N, K, layout, A, Bm):
    """The kernel instance dgcnn_gemm_f32 takes under the current arithmetic / override, as the engine names it for its tables: the
    row tile and the 256-column choice come from the library (dgcnn_gemm_x3_tile_rows / _cols)."""
    from dgcnn import _engine as E
    prev, E.H.TIMER = E.H.TIMER, E.H.Timer(watch=set())
    try:
        return E._gemm_tag(M, N, K, layout == "TN", layout == "NT", A, Bm)
    finally:
        E.H.TIMER = prev


def np1_instance(family, layout):
    """-> the tag of one of the nine single-product instantiations; family = 64 | 128 (gemm_x3_kernel's column tile) | 'w2'."""
    if family == "w2":
        return "gemm_x3w2_kernel<%s,%s,bf16x1>" % KINDS[layout]
    return "gemm_x3_kernel<%s,%s,%d,bf16x1>" % (KINDS[layout] + (family,))


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Case(object):
    """Operands of one tier in every stored layout and the float64 product of the operands as the kernel sees them: rounded to
    bf16 (`rounded`, arithmetic 1) or raw."""

    def __init__(self, tier, M, N, K, seed=0, rounded=True):
        A, Bm = R.operands(tier, M, N, K, seed)
        self.tier, self.exact = tier, tier in R.EXACT_TIERS
        self.M, self.N, self.K = M, N, K
        self.hA, self.hB = A, Bm
        self.A, self.At = dev(A), dev(A.T.copy())
        self.B, self.Bt = dev(Bm), dev(Bm.T.copy())
        ref, scale = R.product64(R.bf16_round(A), R.bf16_round(Bm)) if rounded else R.product64(A, Bm)
        if self.exact:
            assert np.array_equal(ref, R.product_int(A, Bm)) and scale.max() + 16 < R.LIMIT
        self.ref, self.scale = dev(ref), dev(scale)

    def operands(self, layout):
        return {"NN": (self.A, self.B, {}), "NT": (self.A, self.Bt, {"transB": True}), "TN": (self.At, self.B, {"transA": True})}[layout]

    def extra(self, shape, seed):
        return R.extra(self.tier, shape, seed)

    def check(self, C, kernel, what, plus=None, bar=REL_BAR):
        """C against the reference (+ a prior C / bias): equality on the exact tiers, error / scale below the bar on the others."""
        ref = self.ref if plus is None else self.ref + plus
        Cd = C.double()
        assert bool(torch.isfinite(Cd).all()), (what, "non-finite outputs")
        if self.exact:
            bad = Cd != ref
            nbad = int(bad.sum())
            assert nbad == 0, "%s: %d of %d elements differ from the exact product, max |diff| %g, first at %s" % (
                what, nbad, bad.numel(), float((Cd - ref).abs().max()), bad.nonzero()[0].tolist())
            note(kernel, self.tier, 0.0)
            return 0.0
        e = float(((Cd - ref).abs() / self.scale).max())
        print("%s: %.3e of the scale (bar %.1e)" % (what, e, bar))
        note(kernel, self.tier, e / bar)
        assert e < bar, (what, e)
        return e

    def check_stats(self, st, C, slots, kernel, what):
        """The epilogue's column sums, summed over the slots: EQUAL to the int64 sums on the ternary tier, the bar of
        tests/test_gpu_gemm_tiles.py:assert_colsums against the kernel's own output on the others."""
        Ch = host(C)
        if self.tier == "ternary":
            s = host(st).reshape(slots, 2, self.N).sum(0)
            want = R.column_sums_int(Ch)
            bad = np.argwhere(s != want)
            assert len(bad) == 0, "%s: %d of %d column sums differ from the int64 sums, first %s: %r != %d" % (
                what, len(bad), want.size, bad[0], s[tuple(bad[0])], want[tuple(bad[0])])
            note(kernel + " statistics", self.tier, 0.0)
        else:
            assert_colsums(st, Ch.astype(np.float64), slots, what)


def bias_of(case, seed):
    """-> bias rows (G, N) on the host, their expansion to (M, N) float64 on the device, and the two device buffers: a float4-aligned
    row stride and an odd one."""
    M, N = case.M, case.N
    G = -(-M // RPG)
    gb = case.extra((G, N), seed)
    bufs = {True: torch.zeros((G, N + 4 - N % 4), device="cuda"), False: torch.zeros((G, N + 1 + (N % 4 == 3)), device="cuda")}
    assert bufs[True].stride(0) % 4 == 0 and bufs[False].stride(0) % 4 != 0
    for v in bufs.values():
        v[:, :N] = dev(gb)
    return dev(np.repeat(gb, RPG, 0)[:M].astype(np.float64)), {a: v[:, :N] for a, v in bufs.items()}


def out_slice(M, N, aligned):
    """A column slice of a wider zero buffer: float4-storable (offset 4, row stride % 4 == 0) or not (offset 1, odd row stride)."""
    lo = 4 if aligned else 1
    width = N + 8 - N % 4 if aligned else N + 3 + ((N + 3) % 4 == 0)
    outw = torch.zeros((M, width), device="cuda")
    assert (outw.stride(0) % 4 == 0) == aligned
    return outw, outw[:, lo:lo + N], lo


def outside_untouched(outw, lo, N):
    return not bool(outw[:, :lo].any()) and not bool(outw[:, lo + N:].any())


# ------------------------------------------------------------------------------------------
# A. arithmetic 1 of dgcnn_gemm_f32
# ------------------------------------------------------------------------------------------
A1_CONFIGS = [(1, 0), (1, 128), (1, 256)]
# shape -> {override: family}.  gemm.hip:tile_n gives 64-column tiles to (300, 72, 44) and (520, 136, 100) (few tiles) and 128-column
# tiles to (4100, 1000, 44), whose 33 row tiles of 128 (17 of 256) x 8 column tiles run on the padded XCD grid (mtiles % 8 != 0);
# M, N, K all ragged, K a multiple of 4 but not of 16.  A 256-row request takes the wave-specialised kernel where M > 128, N > 64.
A1_SHAPES = {(300, 72, 44): {0: 64, 128: 64, 256: "w2"},
             (4100, 1000, 44): {0: 128, 128: 128, 256: "w2"},
             (520, 136, 100): {0: 64, 128: 64, 256: "w2"}}
# the shapes the engine issues in bf16 mode (R k x 2Cp x F and its transpose) and a plain z-grid split: (shape, layout) -> families.
# TN (8, 128, 4100): plan_splits takes the zmajor plan (15 chunks of 288, the last of 68); TN (136, 72, 1300): 5 chunks on grid z
A1_ENGINE = {(640, 8, 8, "NN"): {0: 64, 128: 64, 256: 64},
             (8, 128, 4100, "TN"): {0: 64, 128: 64, 256: 64},
             (136, 72, 1300, "TN"): {0: 64, 128: 64, 256: "w2"}}
assert {f for d in list(A1_SHAPES.values()) + list(A1_ENGINE.values()) for f in d.values()} == {64, 128, "w2"}


@pytest.mark.parametrize("tier", ["lattice", "ties", "random", "ternary"])
@pytest.mark.parametrize("M,N,K", sorted(A1_SHAPES))
def test_arith1_layouts_and_epilogues(dg, M, N, K, tier):
    """Every single-product instantiation in every layout: beta 0 into a NaN-filled C and beta 1; per-group bias with groups that
    straddle tiles, BatchNorm column sums and a strided output slice (NN float4-aligned, NT not)."""
    from dgcnn import _engine as E
    P = Case(tier, M, N, K, seed=M + N + K)
    C0h = P.extra((M, N), 1)
    C0 = dev(C0h)
    bias, gbuf = bias_of(P, 2)
    for arith, override in A1_CONFIGS:
        with tile(override, arith):
            for layout in LAYOUTS:
                A, Bm, tr = P.operands(layout)
                kname = instance(M, N, K, layout, A, Bm)
                assert kname == np1_instance(A1_SHAPES[(M, N, K)][override], layout), (kname, override, layout)
                what = "%s %s override %d (%d, %d, %d) %s" % (layout, kname, override, M, N, K, tier)
                C = torch.full((M, N), NAN, device="cuda")                  # beta = 0 must not read C
                E.gemm(A, Bm, C, **tr)
                P.check(C, kname, what + " beta 0")
                C1 = C0.clone()
                E.gemm(A, Bm, C1, beta=1.0, **tr)
                P.check(C1, kname, what + " beta 1", C0.double())
            for layout, aligned in (("NN", True), ("NT", False)):
                A, Bm, tr = P.operands(layout)
                kname = instance(M, N, K, layout, A, Bm)
                what = "%s %s override %d (%d, %d, %d) %s gbias/stats/slice" % (layout, kname, override, M, N, K, tier)
                outw, C, lo = out_slice(M, N, aligned)
                st = torch.zeros(E.H.stat_slots() * 2 * N, dtype=torch.float64, device="cuda")
                E.gemm(A, Bm, C, gbias=gbuf[aligned], rpg=RPG, stats=st, **tr)
                P.check(C, kname, what, bias)
                assert outside_untouched(outw, lo, N), (what, "wrote outside its columns")
                P.check_stats(st, C, E.H.stat_slots(), kname, what)


@pytest.mark.parametrize("tier", ["lattice", "ties", "random"])
@pytest.mark.parametrize("M,N,K,layout", sorted(A1_ENGINE))
def test_arith1_engine_shapes_and_split_k(dg, M, N, K, layout, tier):
    """conv0 of the bf16 mode where the fused kernels do not take the shape (R k x 2Cp x F, NN) and its weight gradient (TN over
    all edges: split-K, zmajor with a ragged last chunk), and a plain z-grid split that the 256-row request runs on the
    wave-specialised kernel."""
    from dgcnn import _engine as E
    P = Case(tier, M, N, K, seed=M + K)
    C0 = dev(P.extra((M, N), 3))
    A, Bm, tr = P.operands(layout)
    for arith, override in A1_CONFIGS:
        with tile(override, arith):
            kname = instance(M, N, K, layout, A, Bm)
            assert kname == np1_instance(A1_ENGINE[(M, N, K, layout)][override], layout), (kname, override)
            what = "%s %s override %d (%d, %d, %d) %s" % (layout, kname, override, M, N, K, tier)
            split = " split-K" if K >= 512 else ""
            C = torch.full((M, N), NAN, device="cuda")
            E.gemm(A, Bm, C, **tr)
            P.check(C, kname + split, what + " beta 0")
            C1 = C0.clone()
            E.gemm(A, Bm, C1, beta=1.0, **tr)
            P.check(C1, kname + split, what + " beta 1", C0.double())


@pytest.mark.parametrize("tier", ["lattice", "random"])
@pytest.mark.parametrize("M,N,K", sorted(A1_SHAPES))
def test_arith1_equals_arith6_bit_for_bit_on_bf16_operands(dg, M, N, K, tier):
    """Operands that are bf16 values already split exactly into (a, 0, 0): the five further partial products of arithmetic 6 add
    exact zeros to the same accumulator in the same k order, so the same tile gives the same bits (NN and NT, unsplit)."""
    from dgcnn import _engine as E
    A, Bm = R.operands(tier, M, N, K, seed=11)
    A, Bm = R.bf16_round(A), R.bf16_round(Bm)
    ops = {"NN": (dev(A), dev(Bm), {}), "NT": (dev(A), dev(Bm.T.copy()), {"transB": True})}
    for override in (128, 256):
        for layout, (a, b, tr) in ops.items():
            out = {}
            for arith in (1, 6):
                with tile(override, arith):
                    out[arith] = torch.full((M, N), NAN, device="cuda")
                    E.gemm(a, b, out[arith], **tr)
                    kname = instance(M, N, K, layout, a, b)
            if not same_bits(out[1], out[6]):
                d = (out[1] - out[6]).abs()
                raise AssertionError("%s override %d (%d, %d, %d) %s: arithmetic 1 differs from arithmetic 6 in %d elements, max %g" % (
                    layout, override, M, N, K, tier, int((d != 0).sum()), float(d.max())))
            note(kname + " == bf16x1 bits", tier, 0.0)


@pytest.mark.parametrize("M,N,K", [(520, 136, 100), (300, 72, 44)])
def test_every_tile_kernel_equals_the_exact_lattice_product(dg, M, N, K):
    """Arithmetics 0, 6 and 9 on every tile override of tests/test_gpu_gemm_tiles.py: integers up to 8 split into (a, 0, 0), every
    partial sum is exact -- each kernel must return the int64 product in each layout."""
    from dgcnn import _engine as E
    P = Case("lattice", M, N, K, seed=K, rounded=False)
    for arith, override in CONFIGS:
        with tile(override, arith):
            if M > 128 and N > 128:                                        # (the 256-column kernels need both)
                check_forced(override, M, N, K)
            for layout in LAYOUTS:
                A, Bm, tr = P.operands(layout)
                kname = instance(M, N, K, layout, A, Bm)
                assert kname.startswith(kernel_name(M, N, K).split("<")[0]), (kname, kernel_name(M, N, K))
                C = torch.full((M, N), NAN, device="cuda")
                E.gemm(A, Bm, C, **tr)
                P.check(C, kname, "%s %s arith %d override %d (%d, %d, %d)" % (layout, kname, arith, override, M, N, K))


# what include/dgcnn_hip.h documents of dgcnn_gemm_set_arith: only float4-loadable products with N > 4 and K > 4 round their
# operands.  (M, N, K, layout, the kernel that runs instead)
UNROUNDED = [(300, 6, 44, "NN", "gemm_kernel (N % 4 != 0)"), (300, 4, 44, "NN", "skinny_nn_kernel"),
             (72, 4, 300, "TN", "skinny_tn_kernel"), (300, 8, 4, "NT", "skinny_nt_kernel")]


@pytest.mark.parametrize("tier", ["ties", "random"])
@pytest.mark.parametrize("M,N,K,layout,kname", UNROUNDED)
def test_arith1_leaves_these_products_unrounded(dg, M, N, K, layout, kname, tier):
    """Under arithmetic 1 these products are the product of the UNROUNDED operands: within REL_BAR of float64 of the raw operands
    and, on the ties tier (every element moves by half a bf16 ulp), far outside it for the rounded reference.  The engine rounds
    such operands itself (_engine.py:edge_conv_block, bf16_operands)."""
    from dgcnn import _engine as E
    P = Case(tier, M, N, K, seed=N + K, rounded=False)
    A, Bm, tr = P.operands(layout)
    with tile(0, 1):
        C = torch.full((M, N), NAN, device="cuda")
        E.gemm(A, Bm, C, **tr)
    P.check(C, kname + " under arith 1 (unrounded)", "%s %s (%d, %d, %d) %s" % (layout, kname, M, N, K, tier))
    if tier == "ties":
        ref, scale = R.product64(R.bf16_round(P.hA), R.bf16_round(P.hB))
        e = float((np.abs(host(C) - ref) / scale).max())
        assert e > REL_BAR, (kname, "matches the ROUNDED operands", e)


# ------------------------------------------------------------------------------------------
# B. the plane GEMM
# ------------------------------------------------------------------------------------------
def planes(x, transpose=False):
    from dgcnn import _planes as PL
    return PL.from_f32(dev(x), PL.F16X2, transpose=transpose)


def exact_equal(C, want, what):
    got = host(C).astype(np.float64)
    assert np.isfinite(got).all(), (what, "non-finite outputs")
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: %d of %d elements differ from the exact result, first %s: %r != %r" % (
        what, len(bad), want.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


# M in {1, 255, 256, 257, 520} x N in {1, 127, 128, 129, 136, 260} (both store paths: ldc % 4 zero and not) x K in {32, 64, 96, 160}
# (nk = 1, 2, 3, 5 slabs against three LDS stages), pairwise; (4100, 136, 32): 17 row tiles x 2 column tiles on the padded XCD grid
KC_CASES = [(1, 1, 32), (255, 127, 64), (256, 128, 96), (257, 129, 160), (520, 136, 32), (1, 260, 64), (255, 136, 160), (256, 260, 32),
            (257, 1, 96), (520, 127, 160), (520, 260, 96), (256, 129, 64), (1, 128, 160), (4100, 136, 32)]
KC_RANDOM = [(520, 136, 32), (255, 127, 64), (520, 260, 96), (257, 129, 160)]           # one ragged case per K
assert {c[0] for c in KC_CASES} == {1, 255, 256, 257, 520, 4100} and {c[1] for c in KC_CASES} == {1, 127, 128, 129, 136, 260}
assert {c[2] for c in KC_CASES} == {32, 64, 96, 160} == {c[2] for c in KC_RANDOM} and set(KC_RANDOM) <= set(KC_CASES)


@pytest.mark.parametrize("M,N,K", KC_CASES)
def test_planes_kc_at_the_tile_edges(dg, M, N, K):
    """C = X W with X (M, K) and W^T (N, K) as planes: the lattice tier must equal the int64 product; the random tier of one
    ragged case per K meets the bar of tests/test_gpu_gemm_planes.py."""
    from dgcnn import _planes as PL
    tiers = ["lattice"] + (["random"] if (M, N, K) in KC_RANDOM else [])
    for tier in tiers:
        X, W = R.operands(tier, M, N, K, seed=M + N + K)
        C = torch.full((M, N), NAN, device="cuda")
        PL.gemm(PL.KC, planes(X), planes(W, transpose=True), C)
        what = "gemm_pl_kernel<KC> (%d, %d, %d) %s" % (M, N, K, tier)
        if tier == "lattice":
            exact_equal(C, R.product_int(X, W), what)
            note("gemm_pl_kernel<KC>", tier, 0.0)
        else:
            ref, _ = R.product64(X, W)
            e = _err(host(C).astype(np.float64), ref, X.astype(np.float64), W.astype(np.float64))
            print("%s: %.3e (bar %.1e)" % (what, e, PLANE_BAR))
            note("gemm_pl_kernel<KC>", tier, e / PLANE_BAR)
            assert e < PLANE_BAR, (what, e)


@pytest.mark.parametrize("M,N,K", [(520, 136, 64), (257, 260, 96)])
def test_planes_kc_epilogues_on_a_ragged_last_row_tile(dg, M, N, K):
    """beta 1, per-group bias (groups of 100 rows) through a float4-aligned and an odd bias stride, a channel view of a wider plane
    set at a non-zero octet, an output slice of a wider buffer (lattice tier: equality); column sums with 32 and with 256 slots
    (ternary tier: equality with the int64 sums)."""
    from dgcnn import _hip as H, _planes as PL
    P = Case("lattice", M, N, K, seed=5, rounded=False)
    X, W = P.hA, P.hB
    want = R.product_int(X, W).astype(np.float64)
    Xp, Wp = planes(X), planes(W, transpose=True)
    kname = "gemm_pl_kernel<KC> epilogue"
    # beta 1
    C0 = P.extra((M, N), 1)
    C = dev(C0)
    PL.gemm(PL.KC, Xp, Wp, C, beta=1.0)
    exact_equal(C, want + C0, "beta 1 (%d, %d, %d)" % (M, N, K))
    # per-group bias, both strides; into an output slice of a wider buffer (float4-storable and not)
    bias, gbuf = bias_of(P, 2)
    for aligned in (True, False):
        outw, Cs, lo = out_slice(M, N, aligned)
        PL.gemm(PL.KC, Xp, Wp, Cs, gbias=gbuf[aligned], rpg=RPG)
        exact_equal(Cs, want + host(bias), "gbias / slice aligned=%s (%d, %d, %d)" % (aligned, M, N, K))
        assert outside_untouched(outw, lo, N), "wrote outside its columns"
        note(kname, "lattice", 0.0)
    # a channel range of a wider plane set, starting at octet 8
    rng = np.random.default_rng(K)
    big = R.lattice(rng, (M, 64 + K + 32))
    big[:, 64:64 + K] = X
    C = torch.full((M, N), NAN, device="cuda")
    PL.gemm(PL.KC, planes(big).cols_view(64, 64 + K), Wp, C)
    exact_equal(C, want, "cols_view (%d, %d, %d)" % (M, N, K))
    # statistics: ternary operands, lattice bias
    T = Case("ternary", M, N, K, seed=6, rounded=False)
    tb, tg = bias_of(T, 7)
    twant = R.product_int(T.hA, T.hB).astype(np.float64) + host(tb)
    Tx, Tw = planes(T.hA), planes(T.hB, transpose=True)
    prev = H.stat_slots()
    try:
        for slots in (32, 256):
            H.set_stat_slots(slots)
            st = torch.zeros(slots * 2 * N, dtype=torch.float64, device="cuda")
            C = torch.full((M, N), NAN, device="cuda")
            PL.gemm(PL.KC, Tx, Tw, C, gbias=tg[slots == 32], rpg=RPG, stats=st)
            exact_equal(C, twant, "statistics run, %d slots (%d, %d, %d)" % (slots, M, N, K))
            T.check_stats(st, C, slots, "gemm_pl_kernel<KC>", "%d slots (%d, %d, %d)" % (slots, M, N, K))
            used = host(st).reshape(slots, 2 * N).any(1)
            assert used[:-(-M // 256)].all() and not used[-(-M // 256):].any(), "row tile t writes slot t"
    finally:
        H.set_stat_slots(prev)


@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("N", [136, 260])
@pytest.mark.parametrize("rpg", [256, 512])
def test_planes_kc_column_maximum(dg, rpg, N, negative):
    """The per-group column maximum of the KC epilogue, three groups: value and FIRST row among ties equal numpy's max / argmax of
    the returned C.  Lattice rows drawn from a pool of eight (every maximum is tied many times) and three zero columns of W (the
    whole column ties: row 0 wins); `negative`: A >= 1 and one all-negative column of W, so a whole column of C is negative."""
    from dgcnn import _planes as PL
    G, K = 3, 64
    M = G * rpg
    rng = np.random.default_rng(rpg + N + negative)
    pool = R.lattice(rng, (8, K), lo=1 if negative else -R.LATTICE_MAX)
    X = pool[rng.integers(0, 8, M)]
    W = R.lattice(rng, (K, N))
    W[:, :3] = 0
    if negative:
        W[:, 5] = -np.abs(W[:, 5]) - 1 + (np.abs(W[:, 5]) == R.LATTICE_MAX)          # in [-8, -1]
    C = torch.full((M, N), NAN, device="cuda")
    keys = torch.zeros(G * N, dtype=torch.int64, device="cuda")
    PL.gemm(PL.KC, planes(X), planes(W, transpose=True), C, colmax=keys, colmax_rpg=rpg)
    what = "gemm_pl_kernel<KC> colmax rpg %d N %d%s" % (rpg, N, " negative column" if negative else "")
    exact_equal(C, R.product_int(X, W), what)
    Ch = host(C)
    if negative:
        assert (Ch[:, 5] < 0).all()
    vals, arg = decode(keys, G, N)
    assert_colmax(vals, arg, Ch, G, rpg, N, what)
    tied = (Ch.reshape(G, rpg, N) == Ch.reshape(G, rpg, N).max(1, keepdims=True)).sum(1)
    assert (tied > 1).mean() > 0.9, "the tier does not tie"
    note("gemm_pl_kernel<KC> column maximum", "lattice", 0.0)


# M in {32, 96, 288} x N in {32, 160} x K in {1, 31, 33, 64, 100, 2047, 2100, 4100}: a last slab that runs into the zero pad rows,
# K = rows_alloc exactly (64), no split (K / 256 < 8) against split (2100: 8 chunks of 288; 4100: 15)
TR_CASES = [(32, 32, 1), (96, 160, 31), (288, 32, 33), (32, 160, 64), (96, 32, 100), (288, 160, 2047), (96, 160, 2100), (288, 32, 4100),
            (32, 32, 2100), (288, 160, 4100)]
TR_RANDOM = [(96, 32, 100), (96, 160, 2100)]
assert {c[2] for c in TR_CASES} == {1, 31, 33, 64, 100, 2047, 2100, 4100} and set(TR_RANDOM) <= set(TR_CASES)
FILL = 0x55


@pytest.mark.parametrize("M,N,K", TR_CASES)
def test_planes_tr_with_and_without_a_workspace(dg, M, N, K):
    """dW = X^T dY with X (K, M) and dY (K, N) as planes, with a workspace (K >= 2048 splits the reduction), with none and with one
    that is too small (both run unsplit and leave it alone), beta 0 and beta 1: the lattice tier equals the int64 product every
    time; the random tier of two cases meets the bar."""
    from dgcnn import _planes as PL
    rng = np.random.default_rng(M + N + K)
    tiers = ["lattice"] + (["random"] if (M, N, K) in TR_RANDOM else [])
    for tier in tiers:
        gen = R.GENERATORS[tier]
        X, dY = gen(rng, (K, M)), gen(rng, (K, N))
        C0 = R.extra(tier, (M, N), K)
        Xp, Yp = planes(X), planes(dY)
        assert Xp.ra == Yp.ra == -(-K // 64) * 64
        ref, scale = R.product64(X.T, dY)
        for mode in ("workspace", "none", "too small"):
            ws = None if mode == "none" else torch.full(((16 << 20) if mode == "workspace" else 1024,), FILL, dtype=torch.uint8, device="cuda")
            for beta in (0.0, 1.0):
                C = dev(C0) if beta else torch.full((M, N), NAN, device="cuda")
                PL.gemm(PL.TR, Xp, Yp, C, beta=beta, ws=ws)
                want = ref + (C0 if beta else 0)
                what = "gemm_pl_kernel<TR> (%d, %d, %d) %s, %s, beta %g" % (M, N, K, tier, mode, beta)
                kname = "gemm_pl_kernel<TR>" + (" split-K" if mode == "workspace" and K >= 2048 else "")
                if tier == "lattice":
                    exact_equal(C, want, what)
                    note(kname, tier, 0.0)
                else:
                    got = host(C).astype(np.float64)
                    assert np.isfinite(got).all(), what
                    e = float((np.abs(got - want) / np.maximum(scale, 1e-30)).max())
                    print("%s: %.3e (bar %.1e)" % (what, e, PLANE_BAR))
                    note(kname, tier, e / PLANE_BAR)
                    assert e < PLANE_BAR, (what, e)
            if ws is not None:
                used = bool((ws != FILL).any())
                assert used == (mode == "workspace" and K >= 2048), "%s: workspace %s" % (what, "written" if used else "not used")


def test_planes_refusals_leave_c_alone(dg):
    """What dgcnn_gemm_planes_f32 refuses, each with its documented code, before anything runs: C is unchanged afterwards."""
    from dgcnn import _hip as H, _planes as PL
    rng = np.random.default_rng(0)
    ps = lambda rows, cols: planes(R.random(rng, (rows, cols)))
    a64, b64, a40 = ps(64, 64), ps(64, 64), ps(64, 40)
    gb = torch.zeros((1, 64), device="cuda")
    st = torch.zeros(H.stat_slots() * 2 * 64, dtype=torch.float64, device="cuda")
    keys = torch.zeros(64, dtype=torch.int64, device="cuda")

    def view(p, **kw):
        v = p.cols_view(0, p.cols)
        v.__dict__.update(kw)
        return v
    unsup = (H.HipError, r"\(-4\)")
    inval = (ValueError, "")
    cases = [("KC with K % 32 != 0", PL.KC, a40, ps(64, 40), (64, 64), {}, unsup),
             ("TR with M % 32 != 0", PL.TR, a40, b64, (40, 64), {}, unsup),
             ("TR with a bias", PL.TR, a64, b64, (64, 64), {"gbias": gb, "rpg": 64}, unsup),
             ("TR with statistics", PL.TR, a64, b64, (64, 64), {"stats": st}, unsup),
             ("column maximum in TR", PL.TR, a64, b64, (64, 64), {"colmax": keys, "colmax_rpg": 256}, unsup),
             ("column maximum with rpg % 256 != 0", PL.KC, a64, b64, (64, 64), {"colmax": keys, "colmax_rpg": 64}, unsup),
             ("TR operands with different rows_alloc", PL.TR, a64, view(b64, ra=128), (64, 64), {}, inval),
             ("misaligned planes", PL.KC, view(a64, buf=a64.buf[8:]), b64, (64, 64), {}, inval)]
    for name, form, A, B, shape, kw, (exc, match) in cases:
        C0 = R.random(rng, shape)
        C = dev(C0)
        with pytest.raises(exc, match=match):
            PL.gemm(form, A, B, C, **kw)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(host(C), C0, err_msg=name)
        assert not bool(st.any()) and not bool(keys.any()), name

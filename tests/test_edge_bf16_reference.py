"""tests/edge_bf16_reference.py pinned down on the host: the preconditions that tests/test_gpu_bf16_edge_kernels.py relies on,
asserted for every one of its cases (same case lists, same seeds, same operands), the reference forward against the oracle's
bf16 edge product, and apply32(bf16=True) against what tests/test_gpu_bn_kernels.py expects of the rounding flag."""
import numpy as np
import pytest

import bn_reference as BR
import edge_bf16_reference as EB
import edge_reference as ER
from oracle import dgcnn_oracle as O

LIMIT = 2.0 ** 24


def test_case_lists_cover_every_instance_and_loop():
    """Every (CK, FB) instance in the forward and in the backward list; the multi-tile cases have more tiles than workgroups."""
    six = {(ck, fb) for ck in (1, 8) for fb in (1, 2, 4)}
    assert {EB.instance(c) for c in EB.FWD_CASES} == six and {EB.instance(c) for c in EB.BWD_CASES} == six
    for c in EB.FWD_MULTI_TILE:
        g = EB.geometry(c)
        assert g["dense"] > EB.FWD_GRID and g["points"] > EB.FWD_GRID
    for c in EB.BWD_MULTI_TILE:
        assert EB.geometry(c)["points"] > EB.BWD_GRID
    assert {EB.instance(c)[0] for c in EB.FWD_MULTI_TILE} == {1, 8} == {EB.instance(c)[0] for c in EB.BWD_MULTI_TILE}
    for c in EB.FWD_CASES + EB.BWD_CASES:
        assert c[3] <= EB.RT and (c[2] <= 4 or c[2] == 64) and c[4] in (32, 64, 128)
    for c in EB.BWD_CASES:                  # k >= 8 and the 160 KB of LDS (edge_mlp_bf16.hip:bwd_lds_bytes)
        K, P = (16 if c[2] <= 4 else 128), EB.RT // c[3]
        assert c[3] >= 8 and 2 * EB.RT * (2 * K + 16) + EB.RT * (2 * c[4] + 16) + 2 * 16 * P * c[4] <= 160 * 1024
    assert EB.geometry(EB.FWD_CASES[0]) == {"R": 37, "Me": 259, "P": 18, "dense": 3, "points": 3, "pad": 2}
    assert EB.geometry(EB.FWD_CASES[6])["pad"] == 28 and EB.geometry(EB.FWD_CASES[7])["pad"] == 0
    assert EB.stats_grid(1050, 32) == 1024 and EB.stats_grid(1050, 33) == 33 and EB.stats_grid(15, 33) == 15


@pytest.mark.parametrize("tier", ["lattice", "wide"])
@pytest.mark.parametrize("case", EB.FWD_CASES, ids=EB.case_id)
def test_forward_preconditions(case, tier):
    """Lattice: Eb == E, Wb == W0.  Both lattice tiers: every partial sum of y exact in fp32 (sum |term| < 2^24 units of 1/64),
    the 16 values a lane of the statistics pass adds in fp32 exact (16 max |y| 8 < 2^24), z exact in fp32 (the mean over k is
    replayed in fp32 in the kernel's order, so it needs no precondition).  Lattice: the 16
    squares exact as well.  Wide: a positive share of E needs the rounding, exact ties among them, rounding before the
    subtraction changes a positive share of E, and it changes y."""
    B, N, C, k, F, kind = case
    o = EB.forward_case(case, tier)
    E = ER.edges32(o.x, o.idx)
    Eb, Wb = EB.operands_bf16(o.x, o.idx, o.W0)
    np.testing.assert_array_equal(Wb, o.W0)
    worst = ER.lattice_precondition(o.Yscale, (o.x, o.W0, Eb))
    assert worst < LIMIT
    assert 16 * EB.units(o.Y, 3) < LIMIT
    fw = EB.kreduce(o.Y, o.R, k, o.mean, o.rstd, o.beta)
    rows = slice(0, 256)
    assert np.array_equal(fw.z[rows].astype(np.float64), np.maximum((o.Y.reshape(o.R, k, F)[rows] - o.mean) * o.rstd + o.beta, 0))
    assert (fw.mx[:, 0] == 0).all() and (fw.ties[:, 0] == k).all() and (fw.npos[:, 0] == 0).all()      # the dead column
    assert (fw.npos[:, 1:] > 0).any() and (fw.npos[:, 1:] < k).any() or k == 1
    if tier == "lattice":
        np.testing.assert_array_equal(Eb, E)
        assert EB.sq_exact(o.Y), "16 max y^2 64 = %g" % (16 * 64 * (o.Y ** 2).max())
    else:
        share = float((Eb != E).mean())
        odd = np.abs(E) % 2 == 1
        ties = (np.abs(E) >= 256) & (np.abs(E) < 512) & odd
        assert share > 0 and ties.any(), share
        np.testing.assert_array_equal(np.abs(Eb[ties]) % 4, 0)                       # ties go to the even neighbour
        assert worst < 0.08 * LIMIT                                                  # (units of 1/64: 1 % of 2^24 units of 1/8)
        rows = slice(0, 1 << 15)                                                     # (a property of the tier: the first rows do)
        Ew = EB.operands_rounded_first(o.x, o.idx)[rows]
        assert float((Ew != Eb[rows]).mean()) > 0
        Yw, sw = EB.mlp64(Ew, Wb)
        assert ER.lattice_precondition(sw) < LIMIT                                   # the wrong y is exact too ...
        differ = Yw != o.Y[rows]
        assert differ.mean() > 0                                                     # ... and another one,
        assert np.abs(Yw - o.Y[rows])[differ].min() >= 0.125                         # by whole units of 1/8


@pytest.mark.parametrize("case", EB.BWD_CASES, ids=EB.case_id)
def test_backward_preconditions(case):
    """The exact tier of dW0: with red = 0, dmax = 0 and dmean = k g the rounded dY IS rstd g [z > 0], a multiple of 1/16, and
    sum |term| of Eb^T dY + prior stays below 2^24 units of 1/16: dW0 is exact in fp32 in any order, over any split into tiles."""
    B, N, C, k, F, kind = case
    o = EB.backward_case(case, "lattice")
    np.testing.assert_array_equal(o.Eb, ER.edges32(o.x, o.idx))
    np.testing.assert_array_equal(o.Wb, o.W0)
    assert ER.lattice_precondition(o.Yscale, (o.x, o.W0)) < LIMIT
    fw = EB.kreduce(o.Y, o.R, k, o.mean, o.rstd, o.beta)
    dY, dYsum = EB.backward(fw, o.dmax, o.dmean, np.zeros((2, F)))
    want = np.where(fw.pos, (o.rstd * o.g)[:, None, :], np.float32(0))
    np.testing.assert_array_equal(dY, want)
    assert (dY != 0).mean() > 0.2
    EB.units(dY, 4)
    np.testing.assert_array_equal(dYsum.astype(np.float64), dY.astype(np.float64).sum(1))
    ref, scale = EB.wgrad64(o.Eb, dY)
    assert EB.units(scale + np.abs(o.dW0), 4) < LIMIT
    assert EB.units(ref + o.dW0, 4) < LIMIT
    # one tile lost among them moves dW0: every tile carries a non-zero term of some element
    P = EB.RT // k
    per_tile = np.add.reduceat(np.abs(o.Eb).sum(1) * np.abs(dY.reshape(o.Me, F)).sum(1), np.arange(0, o.Me, P * k))
    assert (per_tile > 0).all()


@pytest.mark.parametrize("case", [EB.FWD_CASES[0], EB.FWD_CASES[3], EB.FWD_CASES[5]], ids=EB.case_id)
def test_reference_forward_equals_the_oracle(case):
    """operands_bf16 / mlp64 on a random case == oracle.bf16_round(oracle.edges(...)) @ oracle.bf16_round(W0) in float64."""
    B, N, C, k, F, kind = case
    o = EB.forward_case(case, "random")
    Eb, Wb = EB.operands_bf16(o.x, o.idx, o.W0)
    Eo = O.bf16_round(O.edges(o.x.reshape(B, N, C), k, o.idx)).reshape(o.Me, 2 * C)
    assert Eo.dtype == np.float32
    np.testing.assert_array_equal(Eb, Eo)
    np.testing.assert_array_equal(Wb, O.bf16_round(o.W0))
    np.testing.assert_array_equal(o.Y, Eo.astype(np.float64) @ O.bf16_round(o.W0).astype(np.float64))
    assert (Eb != ER.edges32(o.x, o.idx)).mean() > 0.9          # random operands: nearly every entry is rounded
    S, sc = EB.stats64(o.Y)
    np.testing.assert_array_equal(S[0], o.Y.sum(0))
    np.testing.assert_array_equal(S[1], sc[1])


@pytest.mark.parametrize("R,k,F", [(60, 4, 16), (33, 7, 8), (50, 1, 12)])
def test_apply32_bf16_is_what_the_bn_kernel_test_expects(R, k, F):
    """One cloud, dense rows: EB.backward is the chain of tests/test_gpu_bn_kernels.py::
    test_bf16_flag_rounds_dy_and_sums_the_rounded_values (Fwd -> Sums -> dz32 -> apply32(bf16=True)), and what that test asserts
    of the kernel holds of the replay: bf16 values (16 zero low bits), round-to-nearest-even of the plain fp32 replay, dYsum the
    sequential fp32 sum of the ROUNDED values, and different from the plain replay."""
    rng = np.random.default_rng(R + k)
    y = rng.normal(size=(R, k, F)).astype(np.float32)
    mu, var = BR.two_pass_stats64(y.reshape(R * k, F))
    mu, rs = mu.astype(np.float32), (1.0 / np.sqrt(var + BR.EPS)).astype(np.float32)
    be = rng.normal(0, 0.3, F).astype(np.float32)
    dmax, dmean = rng.normal(size=(R, F)).astype(np.float32), rng.normal(size=(R, F)).astype(np.float32)
    fw = EB.kreduce(y.reshape(R * k, F), R, k, mu, rs, be)
    s = BR.Sums(BR.dz64(fw, dmax, dmean), fw.xh)
    eo, eacc = BR.apply32(BR.dz32(fw, dmax, dmean), fw.xh, fw.rs, s.red, R * k, bf16=True)
    dY, dYsum = EB.backward(fw, dmax, dmean, s.red)
    np.testing.assert_array_equal(dY, eo)
    np.testing.assert_array_equal(dYsum, eacc)
    assert not (dY.view(np.uint32) & 0xffff).any()
    plain, psum = BR.apply32(BR.dz32(fw, dmax, dmean), fw.xh, fw.rs, s.red, R * k)
    np.testing.assert_array_equal(dY, BR.round_bf16(plain))
    assert (dY != plain).any()
    acc = np.zeros((R, F), np.float32)
    for m in range(k):
        acc = acc + dY[:, m]
    np.testing.assert_array_equal(dYsum, acc)
    assert k == 1 or (dYsum != psum).any()
    np.testing.assert_array_equal(BR.dbeta32(s.red[0], be, 1.0), s.red[0].astype(np.float32) + be)

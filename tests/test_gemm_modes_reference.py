"""tests/gemm_modes_reference.py pinned down on the host: what the tiers of tests/test_gpu_gemm_modes.py rely on, asserted at the
largest shapes that module uses."""
import numpy as np
import pytest

import gemm_modes_reference as R
from oracle import dgcnn_oracle as O


def shuffled_f32_product(A, B, seed):
    """A B in float32 with the K terms in a shuffled order (and whatever blocking the BLAS picks)."""
    perm = np.random.default_rng(seed).permutation(A.shape[1])
    return np.ascontiguousarray(A[:, perm]) @ np.ascontiguousarray(B[perm])


@pytest.mark.parametrize("M,N,K", [(520, 136, 4100), (8, 128, 4100), (300, 72, 44), (640, 8, 8)])
def test_lattice_products_are_exact_in_float32_in_any_order(M, N, K):
    A, B = R.operands("lattice", M, N, K, seed=M + N + K)
    assert A.dtype == np.float32 and np.abs(A).max() <= R.LATTICE_MAX and np.abs(B).max() <= R.LATTICE_MAX
    np.testing.assert_array_equal(O.bf16_round(A), A)                 # bf16 values already: the rounding is the identity
    np.testing.assert_array_equal(O.bf16_round(B), B)
    Ci = R.product_int(A, B)
    ref, scale = R.product64(A, B)
    np.testing.assert_array_equal(ref, Ci)
    # every partial sum, in any order and over any split of K, is an integer bounded by sum |term| (+ a prior C or bias <= 8 each)
    assert scale.max() + 2 * R.LATTICE_MAX < R.LIMIT
    C32 = shuffled_f32_product(A, B, K)
    assert C32.dtype == np.float32
    np.testing.assert_array_equal(C32, Ci)
    if (M, N, K) == (520, 136, 4100):
        print("max |C| = %d, max sum |term| = %d" % (np.abs(Ci).max(), scale.max()))


@pytest.mark.parametrize("M,N,K", [(520, 136, 100), (4100, 1000, 44), (520, 136, 64)])
def test_ternary_statistics_are_exact_in_float32(M, N, K):
    A, B = R.operands("ternary", M, N, K, seed=M + K)
    assert set(np.unique(A)) <= {-1.0, 0.0, 1.0} and set(np.unique(B)) <= {-1.0, 0.0, 1.0}
    Ci = R.product_int(A, B)
    np.testing.assert_array_equal(shuffled_f32_product(A, B, N), Ci)
    # sums of |c| and of c^2 over the rows of one tile: every fp32 partial sum of the epilogue is an integer below 2^24
    assert K <= R.TERNARY_K and R.STAT_TILE_ROWS * K * K < R.LIMIT
    S = R.column_sums_int(Ci)
    for r0 in range(0, M, R.STAT_TILE_ROWS):
        t = Ci[r0:r0 + R.STAT_TILE_ROWS]
        assert np.abs(t).sum(0).max() < R.LIMIT and (t * t).sum(0).max() < R.LIMIT
        rows = np.random.default_rng(r0).permutation(t.shape[0])
        s32 = np.zeros(N, np.float32)
        q32 = np.zeros(N, np.float32)
        for r in rows[:64]:                                           # (a sequential fp32 replay of part of the tile)
            s32 = s32 + t[r].astype(np.float32)
            q32 = q32 + t[r].astype(np.float32) * t[r].astype(np.float32)
        np.testing.assert_array_equal(s32, t[rows[:64]].sum(0))
        np.testing.assert_array_equal(q32, (t[rows[:64]] ** 2).sum(0))
    assert (S[1] > 0).all()                                           # no dead column: a lost row tile moves every sum of squares


def test_ties_are_moved_by_the_rounding_and_tell_the_wrong_roundings_apart():
    T = R.ties(np.random.default_rng(1), (300, 44))
    u = T.view(np.uint32)
    n = R.TIE_SPECIALS.size
    np.testing.assert_array_equal(u.reshape(-1)[:n], R.TIE_SPECIALS)
    body = T.reshape(-1)[n:]
    assert np.isfinite(T).all() and (np.abs(body) >= 2.0 ** -126).all()              # normal numbers only
    assert (np.abs(body) >= 2.0 ** -3).all() and (np.abs(body) < 2.0 ** 4).all()
    np.testing.assert_array_equal(body.view(np.uint32) & 0xFFFF, 0x8000)             # exactly halfway
    assert (body > 0).any() and (body < 0).any()
    rne, trunc, away = O.bf16_round(T), R.bf16_truncate(T), R.bf16_half_away(T)
    rb, tb, ab = (x.reshape(-1)[n:] for x in (rne, trunc, away))
    assert (rb != body).all()                                                         # the rounding changes every tie ...
    half_ulp = (body.view(np.uint32) & np.uint32(0x7F800000)).view(np.float32) * 2.0 ** -8
    np.testing.assert_array_equal(np.abs(rb - body), half_ulp)                       # ... by half a bf16 ulp
    assert ((rb.view(np.uint32) >> 16) & 1 == 0).all()                                # ... to the even neighbour
    assert ((rb == tb) ^ (rb == ab)).all()                                            # which one wrong rounding or the other misses
    assert 0.4 < (rb != tb).mean() < 0.6 and 0.4 < (rb != ab).mean() < 0.6
    # the carry into the exponent, and the zeros
    np.testing.assert_array_equal(rne.reshape(-1)[:n].view(np.uint32), [0x3F800000] * 3 + [0, 0x80000000])
    assert trunc.reshape(-1)[0] != 1.0
    # a product of tie operands tells rounded from unrounded operands far outside an fp32 accumulation bar
    A, B = R.operands("ties", 300, 6, 44, seed=3)
    raw, raw_scale = R.product64(A, B)
    rounded, _ = R.product64(O.bf16_round(A), O.bf16_round(B))
    assert (np.abs(raw - rounded) / raw_scale).max() > 100 * 2e-6


@pytest.mark.parametrize("tier", ["lattice", "ternary"])
@pytest.mark.parametrize("shape", [(520, 64), (1, 32), (4100, 32), (160, 260)])
def test_plane_split_of_the_exact_tiers_has_no_second_term(tier, shape):
    x = R.GENERATORS[tier](np.random.default_rng(shape[0]), shape)
    sc = R.pow2_scale_for(np.abs(x).max())
    assert sc == 1.0 or 2.0 ** 14 <= np.abs(x).max() * sc < 2.0 ** 15
    h1, h2 = R.split_f16x2(x, sc)
    assert not h2.any()
    np.testing.assert_array_equal(h1.astype(np.float64) / sc, x)
    # the products of two such planes: integers times 2^(sa + sb), summed exactly in fp32 while the integer stays below 2^24
    assert R.LATTICE_K * R.LATTICE_MAX ** 2 < R.LIMIT


def test_reference_products():
    A, B = R.operands("random", 37, 20, 44, seed=5)
    ref, scale = R.product64(O.bf16_round(A), O.bf16_round(B))
    np.testing.assert_array_equal(ref, O.bf16_round(A).astype(np.float64) @ O.bf16_round(B).astype(np.float64))
    assert (O.bf16_round(A) != A).mean() > 0.9 and (scale > 0).all()
    assert [R.pow2_scale_for(v) for v in (8.0, 7.0, 1.0, 0.0)] == [2.0 ** 11, 2.0 ** 12, 2.0 ** 14, 1.0]

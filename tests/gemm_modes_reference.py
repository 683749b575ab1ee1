"""Operand generators and float64 references of tests/test_gpu_gemm_modes.py: the single-product bf16 arithmetic of dgcnn_gemm_f32
(dgcnn_gemm_set_arith(1): operands rounded once to bf16, round to nearest even, fp32 accumulation) and the plane GEMM
(dgcnn_gemm_planes_f32, DGCNN_PLANES_F16X2).  No GPU, no torch.

Four operand tiers, all seeded:
  lattice   integers in [-8, 8] as float32: bf16 values already, and fp16 values with h2 = 0 after the power-of-two plane scale.
            With K <= 4100 every partial sum of a product is an integer below 2^24: the fp32 result is EXACT in any summation
            order, over any split of K -- a kernel must equal the int64 product
  ternary   values in {-1, 0, 1}, K <= 100: |c| <= 100, so the column sums of C and of C^2 over a tile of at most 256 rows stay
            below 2^24 in fp32 -- the BatchNorm statistics of the epilogue, summed over their slots, must equal the int64 sums
  ties      every element exactly halfway between two neighbouring bf16 values: ((128 + m) 2 + 1) 2^(e - 8), m in [0, 128), e in
            [-3, 3], both signs.  Round-to-nearest-even moves every element, down where m is even (what truncation gives) and up
            where m is odd (what round-half-away gives): either wrong rounding differs on about half of them.  The first elements
            are three copies of 0x3F7FFFFF (the rounding carry runs into the exponent: 1.0), +0 and -0.  Normal numbers only
  random    standard Gaussian, as Problem of tests/test_gpu_gemm_tiles.py
tests/test_gemm_modes_reference.py asserts on the host what the GPU tiers rely on."""
import math

import numpy as np

from oracle import dgcnn_oracle as O

F32 = np.float32
LIMIT = 2.0 ** 24
TIERS = ("lattice", "ternary", "ties", "random")
EXACT_TIERS = ("lattice", "ternary")
SEED_OF_TIER = {"lattice": 0, "ternary": 300, "ties": 600, "random": 900}
LATTICE_MAX, LATTICE_K = 8, 4100          # |v| <= 8, K <= 4100
TERNARY_K, STAT_TILE_ROWS = 100, 256      # K <= 100; the tallest row tile that adds its column sums in fp32
TIE_SPECIALS = np.array([0x3F7FFFFF, 0x3F7FFFFF, 0x3F7FFFFF, 0x00000000, 0x80000000], np.uint32)


def lattice(rng, shape, lo=-LATTICE_MAX, hi=LATTICE_MAX):
    return rng.integers(lo, hi + 1, shape).astype(F32)


def ternary(rng, shape):
    return rng.integers(-1, 2, shape).astype(F32)


def ties(rng, shape):
    """Exact bf16 ties; the first len(TIE_SPECIALS) elements (row-major) are the special values when the tensor has room."""
    m = rng.integers(0, 128, shape)
    e = rng.integers(-3, 4, shape)
    sign = rng.integers(0, 2, shape) * 2 - 1
    v = (sign * ((128 + m) * 2 + 1) * 2.0 ** (e - 8)).astype(F32)
    flat = v.reshape(-1)
    if flat.size >= 4 * TIE_SPECIALS.size:
        flat[:TIE_SPECIALS.size] = TIE_SPECIALS.view(F32)
    return v


def random(rng, shape):
    return rng.normal(size=shape).astype(F32)


GENERATORS = {"lattice": lattice, "ternary": ternary, "ties": ties, "random": random}


def operands(tier, M, N, K, seed=0):
    """-> A (M, K), B (K, N) float32 of one tier."""
    assert tier != "lattice" or K <= LATTICE_K
    assert tier != "ternary" or K <= TERNARY_K
    rng = np.random.default_rng(SEED_OF_TIER[tier] + seed)
    gen = GENERATORS[tier]
    return gen(rng, (M, K)), gen(rng, (K, N))


def extra(tier, shape, seed):
    """A prior C or a bias of the same tier (lattice for both exact tiers: integers keep every sum exact)."""
    rng = np.random.default_rng(SEED_OF_TIER[tier] + 7919 + seed)
    return lattice(rng, shape) if tier in EXACT_TIERS else random(rng, shape)


def bf16_round(a):
    return O.bf16_round(np.asarray(a, F32))


def bf16_truncate(a):
    """The WRONG rounding: drop the low 16 bits."""
    return (np.ascontiguousarray(a, F32).view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)


def bf16_half_away(a):
    """The other WRONG rounding: halfway cases away from zero."""
    u = np.ascontiguousarray(a, F32).view(np.uint32)
    return ((u + np.uint32(0x8000)) & np.uint32(0xFFFF0000)).view(F32)


def product64(A, B):
    """-> (A B, |A| |B|) in float64."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    return A @ B, np.abs(A) @ np.abs(B)


def product_int(A, B):
    """The int64 product of integer-valued operands."""
    Ai, Bi = np.asarray(A).astype(np.int64), np.asarray(B).astype(np.int64)
    assert np.array_equal(Ai, A) and np.array_equal(Bi, B), "operands off the integer lattice"
    return Ai @ Bi


def column_sums_int(C):
    """-> (2, N) int64: column sums of C and of C^2."""
    Ci = np.asarray(C).astype(np.int64)
    assert np.array_equal(Ci, C)
    return np.stack([Ci.sum(0), (Ci * Ci).sum(0)])


def pow2_scale_for(bound):
    """planes_common.h: the power of two that brings `bound` (fp32) into [2^14, 2^15) -- what dgcnn_planes_scale_f32 writes for a
    tensor whose largest magnitude is `bound`."""
    bound = float(F32(bound))
    if not (bound > 0 and math.isfinite(bound)):
        return 1.0
    e = math.frexp(bound)[1]
    return 2.0 ** max(-100, min(100, 15 - e))


def split_f16x2(x, scale):
    """planes_common.h:split_f16x2 -> (h1, h2) float16: h1 = rn16(x s), h2 = rn16(x s - h1)."""
    xs = np.clip(np.asarray(x, F32) * F32(scale), -65504.0, 65504.0).astype(F32)
    h1 = xs.astype(np.float16)
    h2 = (xs - h1.astype(F32)).astype(np.float16)
    return h1, h2

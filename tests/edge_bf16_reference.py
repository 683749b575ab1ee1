"""Plain numpy restatement of the four fused kernels of the bf16 edge-MLP mode (csrc/edge_mlp_bf16.hip: dgcnn_edge_mlp_bf16,
_stats, _bn_kreduce, _bwd), put together from edge_reference.py and bn_reference.py.  No GPU, no torch.

* OPERANDS: E = [x_i, x_j - x_i] with the subtraction in float32 (edge_reference.edges32), THEN one round-to-nearest-even to
  bf16; W0 rounded the same way.  Everything a kernel multiplies is one of these values.
* PRODUCT and SUMS in float64, each with its scale (the same sum over absolute values of the terms): y = Eb Wb (2C terms per
  element), the column sums of y and y^2, dW0 = Eb^T dY.
* DECISIONS and REPLAYS are bn_reference's: Fwd (z, max, ties, positives, mean32), dz32, apply32(bf16=True), dbeta32.

Three operand tiers:
  lattice   edge_reference.Operands(lattice=True): Eb == E and Wb == W0, y exact in fp32 in any order -- a kernel must EQUAL float64
  wide      x integer in [-300, 300], W0 multiples of 1/8: about one entry of E in eight needs the rounding (odd values in [256, 511]
            are exact ties), y is still exact in fp32, and bf16(x_j) - bf16(x_i) gives ANOTHER exact y -- rounding before the
            subtraction is off by whole units
  random    edge_reference.Operands(lattice=False)
tests/test_edge_bf16_reference.py asserts the preconditions of every case below on the host; tests/test_gpu_bf16_edge_kernels.py
runs them."""
import functools

import numpy as np

import bn_reference as BR
import edge_reference as ER

F32 = np.float32
f32 = BR.f32

RT = 128                  # edge rows per tile (edge_mlp_bf16.hip)
FWD_GRID = 1024           # workgroups of the forward passes at the most
BWD_GRID = 512            # ... of the backward
DEFAULT_SLOTS = 32        # DGCNN_STAT_SLOTS
TIERS = ("lattice", "wide", "random")
BWD_TIERS = ("lattice", "random")

# (B, N, C, k, F, graph); P = 128 // k whole points per tile of the k-reduce and of the backward
FWD_CASES = [
    (1, 37, 3, 7, 64, "random"),          # CK = 1, FB = 2; Me = 259: three dense tiles, the last of 3 rows; P = 18 (2 pad rows), last tile 1 point
    (2, 50, 1, 1, 32, "last"),            # C = 1, k = 1, P = 128
    (3, 33, 2, 5, 128, "hub"),            # C = 2, three clouds
    (2, 40, 4, 20, 32, "permutation"),    # C = 4; P = 6, 8 pad rows
    (1, 50, 64, 3, 128, "random"),        # k < 5; P = 42
    (2, 45, 64, 20, 64, "degrees"),       # the model's size
    (1, 70, 64, 100, 128, "random"),      # 64 < k < 128: P = 1, 28 pad rows per tile
    (2, 30, 64, 128, 32, "permutation"),  # k = 128: no pad rows
    (1, 2100, 64, 64, 32, "random"),      # 1050 dense tiles and 1050 point tiles against a grid of 1024
    (2, 1100, 64, 128, 64, "random"),     # 2200 tiles: two to three per workgroup
    (1, 17000, 4, 8, 128, "random"),      # 1063 tiles on the C <= 4 instances, P = 16
]
BWD_CASES = [
    (1, 37, 3, 8, 64, "random"),          # CK = 1, FB = 2; P = 16
    (2, 50, 1, 9, 32, "hub"),             # C = 1: dW0 rows through the row = -1 map; P = 14, 2 pad rows
    (3, 33, 2, 20, 128, "last"),          # C = 2
    (2, 45, 64, 10, 128, "degrees"),      # next to the LDS limit at C = 64, F = 128: P = 12
    (2, 45, 64, 9, 128, "degrees"),       # the LDS limit itself, the smallest k at C = 64, F = 128: P = 14, 161 792 of 163 840 bytes
    (2, 40, 64, 20, 64, "permutation"),   # the model's size
    (1, 70, 64, 100, 64, "random"),       # P = 1 with pad rows
    (2, 30, 64, 128, 32, "permutation"),  # k = 128
    (1, 2100, 64, 64, 32, "random"),      # 1050 tiles on 512 workgroups: two to three tiles each, both LDS buffers reused
    (1, 17000, 4, 8, 128, "random"),      # 1063 tiles on the C <= 4 instance
]
# Narrowed generators (lattice tiers).  W0 in multiples of 1/8 up to this many eighths instead of 8, where the case as drawn would
# break 16 max y^2 64 < 2^24 (the fp32 partial sums of y^2 in the statistics pass): the C = 64 cases with two clouds, whose centre
# half carries the cloud offset.  The C <= 4 and the one-cloud cases hold as drawn.  Keyed by the tuple: a backward case that is the
# same tuple as a forward one -- (2, 30, 64, 128, 32, permutation) -- gets the forward's narrower weights too (harmless there).
W0_EIGHTHS = {c: 3 for c in FWD_CASES if c[2] == 64 and c[0] > 1}


def cdiv(a, b):
    return -(-a // b)


def case_id(case):
    return ER.case_id(case)


def instance(case):
    """-> (CK, FB): the template instance the case runs."""
    return (1 if case[2] <= 4 else 8), case[4] // 32


def geometry(case):
    """-> R, Me, P, dense tiles (write, statistics), point tiles (k-reduce, backward), pad rows behind the P k rows of a tile."""
    B, N, C, k, F, _ = case
    R, Me, P = B * N, B * N * k, RT // k
    return {"R": R, "Me": Me, "P": P, "dense": cdiv(Me, RT), "points": cdiv(R, P), "pad": RT - P * k}


def _tiles(case):
    g = geometry(case)
    return g["dense"], g["points"]


def stats_grid(ntiles, slots):
    """Workgroups of the statistics pass: min(ntiles, 1024), capped at the slot count above the default (common.h:cap_writers)."""
    g = min(ntiles, FWD_GRID)
    return slots if (slots > DEFAULT_SLOTS and g > slots) else g


# More tiles than workgroups, in the dense AND in the point tiling: the persistent loops loop.  FWD_GRID / BWD_GRID restate the caps of
# edge_mlp_bf16.hip (launch_pass: `ntiles < 1024 ? ntiles : 1024`; dgcnn_edge_mlp_bf16_bwd: 512).  The GPU module does not trust
# them: it reads the forward's grid off the library (the number of slots the statistics pass writes when there are more slots
# than tiles) and the backward's off dgcnn_edge_mlp_bf16_bwd_workspace_bytes, and asserts tiles > grid on those.
FWD_MULTI_TILE = [c for c in FWD_CASES if min(_tiles(c)) > FWD_GRID]
BWD_MULTI_TILE = [c for c in BWD_CASES if _tiles(c)[1] > BWD_GRID]
# the statistics pass with 33 and 768 slots: the model's size (15 tiles, fewer than either count: the slots behind them stay zero)
# and the 1050-tile case (more than either count: 31 to 32 tiles per workgroup, or one to two)
SLOT_FEW_TILES = (2, 45, 64, 20, 64, "degrees")
SLOT_MANY_TILES = (1, 2100, 64, 64, 32, "random")
SLOT_CASES = [SLOT_FEW_TILES, SLOT_MANY_TILES]
SLOT_COUNTS = (33, 768)
PROBE_SLOTS = 4096        # more slots than any case has tiles (and than any plausible cap): one slot per workgroup
assert all(c in FWD_CASES for c in SLOT_CASES) and len(FWD_MULTI_TILE) == 3 and len(BWD_MULTI_TILE) == 2
assert _tiles(SLOT_FEW_TILES)[0] < min(SLOT_COUNTS) and _tiles(SLOT_MANY_TILES)[0] > max(SLOT_COUNTS)
assert max(_tiles(c)[0] for c in FWD_CASES) < PROBE_SLOTS


# ------------------------------------------------------------------------------------------------------------------ reference
def operands_bf16(x, idx, W0):
    """-> Eb (B N k, 2C), Wb (2C, F): what the kernels multiply.  The fp32 subtraction first, then ONE rounding."""
    return BR.round_bf16(ER.edges32(x, idx)), BR.round_bf16(W0)


def operands_rounded_first(x, idx):
    """The WRONG edge tensor [bf16(x_i), bf16(x_j) - bf16(x_i)] rounded once more: what a kernel forms that rounds before it
    subtracts.  Only for showing that a tier can tell the two apart."""
    return BR.round_bf16(ER.edges32(BR.round_bf16(x), idx))


def mlp64(Eb, Wb):
    """y = Eb Wb -> (y, |Eb| |Wb|) float64; 2C terms per element."""
    return ER._mm(Eb, Wb)


def stats64(Y):
    """-> (S, scale), both (2, F) float64: column sums of y and of y^2, and the sums of |y| and of y^2."""
    Y = np.asarray(Y, np.float64)
    q = (Y * Y).sum(0)
    return np.stack([Y.sum(0), q]), np.stack([np.abs(Y).sum(0), q])


def kreduce(Y, R, k, mean, rstd, beta):
    """The forward k-reduce of y (B N k, F): bn_reference.Fwd with ReLU -- mx, mean32, ties, packed."""
    Y = f32(Y)
    return BR.Fwd(Y.reshape(R, k, Y.shape[1]), mean, rstd, beta, 1)


def backward(fw, dmax, dmean, red):
    """-> (dY (R, k, F) of bf16 values, dYsum (R, F)) in float32: dz32 -> apply32(bf16=True) with the given totals red (2, F)."""
    return BR.apply32(BR.dz32(fw, dmax, dmean), fw.xh, fw.rs, red, fw.R * fw.k, bf16=True)


def wgrad64(Eb, dY):
    """dW0 = Eb^T dY -> (dW0, |Eb|^T |dY|) float64 (2C, F); B N k terms per element."""
    dY = np.asarray(dY)
    return ER._mm(np.asarray(Eb).T, dY.reshape(-1, dY.shape[-1]))


def units(a, p):
    """max |a| in units of 2^-p, after asserting that every element is a multiple of that unit."""
    a = np.asarray(a, np.float64) * 2.0 ** p
    assert np.array_equal(a, np.round(a)), "off the lattice"
    return float(np.abs(a).max(initial=0.0))


def sq_exact(Y):
    """True when the statistics pass adds its 16 squares per lane and tile exactly in fp32: y a multiple of 1/8, y^2 of 1/64."""
    return 16.0 * float((np.asarray(Y, np.float64) ** 2).max(initial=0.0)) * 64 < 2.0 ** 24


# ---------------------------------------------------------------------------------------------------------------------- cases
SEED_OF_TIER = {"lattice": 0, "wide": 500, "random": 1000}


def wide_x(rng, B, N, C):
    """Integers in [-300, 300], every cloud drawn on its own."""
    return np.concatenate([rng.integers(-300, 301, (N, C)) for _ in range(B)]).astype(F32)


class Case(object):
    """Operands, BatchNorm parameters and the float64 product of one (case, tier); with backward=True also Eb, the incoming
    gradients, the prior d(beta) and the prior dW0.

    Backward, tier lattice (the exact tier of dW0): dmax = 0, dmean = k g with g a multiple of 1/8 in [-1/2, 1/2]; with red = 0
    (written on the host) dY = rstd g [z > 0] after the bf16 rounding -- k g f32(1 / k) rounds back to g -- a multiple of 1/16."""

    def __init__(self, case, tier, backward=False, dead_column=False):
        B, N, C, k, F, kind = case
        self.case, self.tier = case, tier
        self.lattice = tier != "random"
        seed = ER.case_seed(case) + SEED_OF_TIER[tier] + (250 if backward else 0)
        o = ER.Operands(self.lattice, seed, B, N, C, k, F, kind, need=("W0",))
        rng = np.random.default_rng(seed + 77)
        self.R, self.Me = o.R, o.Me
        self.x, self.idx, self.W0 = o.x, o.idx, o.W0
        if tier == "wide":
            self.x = wide_x(rng, B, N, C)
        wq = W0_EIGHTHS.get(case, 8)
        if self.lattice and wq != 8:
            self.W0 = (rng.integers(-wq, wq + 1, (2 * C, F)) / 8.0).astype(F32)
        Eb, self.Wb = operands_bf16(self.x, self.idx, self.W0)
        self.Y, self.Yscale = mlp64(Eb, self.Wb)
        if self.lattice:
            self.mean, self.rstd, self.beta = BR.lattice_params(rng, F)
        else:
            self.mean = rng.normal(0, 0.3, F).astype(F32)
            self.rstd = (0.5 + rng.random(F)).astype(F32)
            self.beta = rng.normal(0, 0.3, F).astype(F32)
        if dead_column:                   # column 0: z = 0 for every edge of every point -- max 0, ties = k, no positives
            self.mean[0] = np.ceil(self.Y[:, 0].max()) + 1
            self.beta[0] = 0
        if not backward:
            return
        self.Eb = Eb
        R = self.R
        if self.lattice:
            self.g = (rng.integers(-4, 5, (R, F)) / 8.0).astype(F32)
            self.dmax = np.zeros((R, F), F32)
            self.dmean = (k * self.g).astype(F32)
            self.dbeta0 = (rng.integers(-16, 17, F) / 8.0).astype(F32)
            self.dW0 = (rng.integers(-16, 17, (2 * C, F)) / 8.0).astype(F32)
        else:
            self.dmax = rng.normal(size=(R, F)).astype(F32)
            self.dmean = rng.normal(size=(R, F)).astype(F32)
            self.dbeta0 = rng.normal(size=F).astype(F32)
            self.dW0 = rng.normal(size=(2 * C, F)).astype(F32)


@functools.lru_cache(maxsize=2)
def forward_case(case, tier):
    """Shared by the tests of one (case, tier); nobody writes into it."""
    return Case(case, tier, dead_column=True)


@functools.lru_cache(maxsize=2)
def backward_case(case, tier):
    return Case(case, tier, backward=True)

"""Plain numpy restatement of the BatchNorm + activation + max/mean-over-k passes (csrc/bn.hip, planes_bn.hip, det.hip).
No GPU, no torch.  Two layers, kept apart on purpose:

* DECISIONS are taken in float32, operation by operation as the kernels' bn_z does (csrc is built with -ffp-contract=off):
  xh = (y - mu) * rs ; z = xh + be ; relu.  Max over k, the tie count #{m : z_m == max}, the ReLU mask z > 0, the gathered row
  y = V[cloud * N + idx] + U (one fp32 add) and the packed count ties + 256 * #{z > 0}.  Taken on other values they would
  describe a different function.
* SUMS are float64: dz = relu'(z) (dmax [z == max] / ties + dmean / k), red0 = sum dz, red1 = sum dz xh, their absolute
  counterparts (the error scales), dY = rs (dz - red0 / n - xh red1 / n), dYsum, dbeta, dW0 and the column statistics.

On top, float32 REPLAYS of the passes whose result does not depend on a summation order (the forward mean, the apply pass
given `red`), in the kernels' operation order, for bit-exact expectations."""
import numpy as np

F32 = np.float32
CNT_POS = 256            # bn.hip: the edge variants pack ties + CNT_POS * (#rows with z > 0)
EPS = float(np.float32(1e-3))      # slim.batch_norm's epsilon, the fp32 value the kernels receive


def f32(a):
    return np.ascontiguousarray(a, dtype=F32)


# ---------------------------------------------------------------------------------------------------------------- decisions
def bn_z32(y, mu, rs, be, relu):
    """-> (z, xh) in float32, one rounding per operation (bn_common.h:bn_z).  `relu` is tested for truth of bit 0."""
    y, mu, rs, be = f32(y), f32(mu), f32(rs), f32(be)
    xh = (y - mu) * rs
    z = xh + be
    if relu & 1:
        z = np.maximum(z, F32(0))
    assert xh.dtype == F32 and z.dtype == F32
    return z, xh


def edge_rows32(V, U, idx, B, N):
    """y[r, m, :] = V[cloud(r) * N + idx[r, m]] + U[r]  (one fp32 add); V, U (B*N, F), idx (B, N, k) -> (B*N, k, F)."""
    V, U = f32(V), f32(U)
    k = idx.shape[-1]
    rows = (np.arange(B)[:, None, None] * N + idx.reshape(B, N, k)).reshape(B * N, k)
    return V[rows] + U[:, None, :]


class Fwd(object):
    """Forward of one (R, k, F) tensor: float32 decisions + the float32 replay of the mean."""

    def __init__(self, y, mu, rs, be, relu):
        y = f32(y)
        assert y.ndim == 3
        self.R, self.k, self.F = y.shape
        self.relu = relu & 1
        self.mu, self.rs, self.be = f32(mu), f32(rs), f32(be)
        self.z, self.xh = bn_z32(y, self.mu, self.rs, self.be, relu)
        self.mx = self.z.max(1)
        self.ismax = self.z == self.mx[:, None, :]
        self.ties = self.ismax.sum(1).astype(F32)
        self.pos = self.z > 0
        self.npos = self.pos.sum(1).astype(F32)
        self.packed = self.ties + F32(CNT_POS) * self.npos                  # exact small integers
        sm = np.zeros((self.R, self.F), F32)
        for m in range(self.k):                                             # sm += z in m order, then * (1.0f / k)
            sm = sm + self.z[:, m]
        self.mean32 = sm * (F32(1) / F32(self.k))
        self.mean64 = self.z.astype(np.float64).sum(1) / self.k


def dz32(fw, dmax, dmean):
    """dz as the kernels form it, in float32: ((z == max) ? dmax / ties : 0) + dmean * (1.0f / k), zero where relu and !(z > 0).
    dmean None: dz = dmax (the k = 1 form, fw.k must be 1)."""
    dmax = f32(dmax)[:, None, :]
    if dmean is None:
        assert fw.k == 1
        dz = np.broadcast_to(dmax, fw.z.shape).copy()
    else:
        invk = F32(1) / F32(fw.k)
        share = dmax / fw.ties[:, None, :]
        dz = np.where(fw.ismax, share, F32(0)) + f32(dmean)[:, None, :] * invk
    if fw.relu:
        dz = np.where(fw.pos, dz, F32(0))
    assert dz.dtype == F32
    return dz


# --------------------------------------------------------------------------------------------------------------------- sums
def dz64(fw, dmax, dmean):
    """dz = relu'(z) (dmax [z == max] / ties + dmean / k) in float64 on the float32 decisions."""
    dmax = np.asarray(dmax, np.float64)[:, None, :]
    if dmean is None:
        assert fw.k == 1
        dz = np.broadcast_to(dmax, fw.z.shape).copy()
    else:
        dz = np.where(fw.ismax, dmax / fw.ties.astype(np.float64)[:, None, :], 0.0) + np.asarray(dmean, np.float64)[:, None, :] / fw.k
    if fw.relu:
        dz = np.where(fw.pos, dz, 0.0)
    return dz


class Sums(object):
    """red0 = sum dz, red1 = sum dz xh over all R k rows, and the sums of absolute values (the error scales)."""

    def __init__(self, dz, xh):
        dz = np.asarray(dz, np.float64)
        t = dz * np.asarray(xh, np.float64)
        self.n_terms = dz.shape[0] * dz.shape[1]
        self.red0, self.red1 = dz.sum((0, 1)), t.sum((0, 1))
        self.abs0, self.abs1 = np.abs(dz).sum((0, 1)), np.abs(t).sum((0, 1))

    @property
    def red(self):
        return np.stack([self.red0, self.red1])

    @property
    def scale(self):
        return np.stack([self.abs0, self.abs1])


def dy64(dz, xh, rs, red):
    """dY = rs (dz - red0 / n - xh red1 / n), float64; red (2, F)."""
    dz, xh = np.asarray(dz, np.float64), np.asarray(xh, np.float64)
    n = dz.shape[0] * dz.shape[1]
    return np.asarray(rs, np.float64) * (dz - red[0] / n - xh * (red[1] / n))


def wgrad64(x, idx, B, N, dY):
    """dW0 = [x_i, x_j - x_i]^T dY (ops.py:39-52); x (B*N, C), idx (B, N, k), dY (B*N, k, F) -> (2C, F) float64."""
    x = np.asarray(x, np.float64)
    k = idx.shape[-1]
    rows = (np.arange(B)[:, None, None] * N + idx.reshape(B, N, k)).reshape(B * N, k)
    dY = np.asarray(dY, np.float64)
    centre = np.einsum("rc,rmf->cf", x, dY)
    diff = np.einsum("rmc,rmf->cf", x[rows] - x[:, None, :], dY)
    return np.concatenate([centre, diff], 0)


def points_closed_form64(mx, mn, npos, dmax, dmean, beta, k):
    """edge_bwd_reduce_points (bn.hip): the two sums of a ReLU layer from per-point data only,
         sum_m dz      = [max > 0] dmax + dmean npos / k
         sum_m dz xhat = [max > 0] dmax (max - beta) + (dmean / k) (k mean - beta npos)        -> (2, F) float64"""
    mx, mn, npos, dmax, dmean, beta = (np.asarray(a, np.float64) for a in (mx, mn, npos, dmax, dmean, beta))
    g1 = np.where(mx > 0, dmax, 0.0)
    g2 = dmean / k
    return np.stack([(g1 + g2 * npos).sum(0), (g1 * (mx - beta) + g2 * (k * mn - beta * npos)).sum(0)])


def finalize64(S, Q, count, eps=EPS):
    """bn_finalize: column sum / sum of squares -> (mean, rstd) in float64 (biased variance, clamped at 0)."""
    S, Q = np.asarray(S, np.float64), np.asarray(Q, np.float64)
    mu = S / count
    var = np.maximum(Q / count - mu * mu, 0.0)
    return mu, 1.0 / np.sqrt(var + eps)


def two_pass_stats64(Y):
    """float64 two-pass mean / biased variance of the columns of fp32 data (rows, F): no Q / n - mu^2 cancellation."""
    Y = np.asarray(Y, np.float64)
    mu = Y.mean(0)
    return mu, ((Y - mu) ** 2).mean(0)


# ------------------------------------------------------------------------------------------------------------------ replays
def round_bf16(o):
    """fp32 -> nearest-even bf16 VALUE stored as fp32 (common.h:round_bf16_rne: (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000;
    a NaN stays a quiet NaN of its sign, (u | 0x00400000) & 0xffff0000, instead of carrying into exponent and sign)."""
    u = f32(o).view(np.uint32).astype(np.uint64)
    r = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    r = np.where((u & 0x7fffffff) > 0x7f800000, (u | 0x00400000) & 0xffff0000, r).astype(np.uint32)
    return r.view(F32).reshape(np.shape(o))


def apply32(dz, xh, rs, red, n, bf16=False):
    """float32 replay of the apply pass given `red` (2, F) float64: c1 = float(red0 * (1.0 / n)), o = rs * ((dz - c1) - xh * c2),
    optional bf16 rounding of o, dYsum added sequentially over m in fp32.  -> (dY (R, k, F), dYsum (R, F))."""
    dz, xh, rs = f32(dz), f32(xh), f32(rs)
    inv = 1.0 / float(n)
    c1 = (np.asarray(red[0], np.float64) * inv).astype(F32)
    c2 = (np.asarray(red[1], np.float64) * inv).astype(F32)
    o = rs * ((dz - c1) - xh * c2)
    assert o.dtype == F32
    if bf16:
        o = round_bf16(o)
    acc = np.zeros((o.shape[0], o.shape[2]), F32)
    for m in range(o.shape[1]):
        acc = acc + o[:, m]
    return o, acc


def dbeta32(red0, prior=None, dbeta_beta=0.0):
    """bn_bwd_finalize_kernel: dbeta = float(red0) (+ dbeta_beta * prior)."""
    s = np.asarray(red0, np.float64).astype(F32)
    if dbeta_beta != 0.0:
        return s + F32(dbeta_beta) * f32(prior)
    return s


def sum_bound(n_terms, scale, extra=8):
    """Any-order fp32 summation of n_terms terms plus the roundings inside a term: (n_terms + extra) 2^-24 sum |term|."""
    return (n_terms + extra) * 2.0 ** -24 * np.asarray(scale, np.float64)


# ------------------------------------------------------------------------------------------------------------ exact lattice
# Inputs for which every product and every partial sum of the passes is exactly representable in fp32, so that no result
# depends on a summation order and the kernels must EQUAL the float64 layer, sums included:
#   y small integers, mean integer, rstd in {1/2, 1, 2}, beta a multiple of 1/4       -> xh in Z/2, z in Z/4
#   k a power of two, dmax in 4 Z, dmean in k Z, tie counts in {1, 2, 4}               -> dz in Z, dz xh in Z/2
# The tie count is planted: the rows hold values in [-4, 4] and 1 / 2 / 4 of them are overwritten with 6, the strict maximum
# (equal values below the maximum do not take part in any decision).  Under ReLU some points are all-dead (every row <= -5 + ...
# far below the mean): their tie count is k but their dz is zeroed.
LATTICE_P = 1             # 2^-p = spacing of the terms dz xh


def _pow2(k):
    return k >= 1 and (k & (k - 1)) == 0


def nearest_pow2(k, cap=None):
    lo = 1 << (int(k).bit_length() - 1)
    hi = lo * 2
    p = lo if (k - lo) < (hi - k) else hi
    while cap is not None and p > cap:
        p //= 2
    return p


def lattice_params(rng, F):
    mu = rng.integers(-2, 3, F).astype(F32)
    rs = rng.choice(np.array([0.5, 1.0, 2.0], F32), F)
    be = (rng.integers(-4, 5, F) * 0.25).astype(F32)
    return mu, rs, be


def lattice_grads(rng, R, k, F, with_mean=True):
    dmax = (4 * rng.integers(-2, 3, (R, F))).astype(F32)
    dmean = (k * rng.integers(-1, 2, (R, F))).astype(F32) if with_mean else None
    return dmax, dmean


def lattice_dense(rng, R, k, F, relu):
    """-> y (R, k, F) with planted tie counts in {1, 2, 4} (<= k) and, under ReLU, a few all-dead points."""
    assert _pow2(k)
    y = rng.integers(-4, 5, (R, k, F)).astype(F32)
    if k > 1:                                                               # (k = 1: the only row is the maximum)
        t = rng.choice([c for c in (1, 2, 4) if c <= k], (R, F))
        order = np.argsort(rng.random((R, k, F)), axis=1)                  # a random permutation of the rows per (point, channel)
        y[order < t[:, None, :]] = 6
    if relu & 1 and R > 2:
        dead = rng.random(R) < 0.1
        y[dead] = -rng.integers(20, 24, (int(dead.sum()), k, F)).astype(F32)
    return y


def lattice_edge(rng, B, N, k, F, relu):
    """-> V, U (B*N, F), idx (B, N, k): point 0 of every cloud is the strict maximum of every channel (V = 6, the others in
    [-4, 4]); each point lists it 1 / 2 / 4 times among otherwise arbitrary neighbours (self and duplicates included)."""
    assert _pow2(k)
    R = B * N
    V = rng.integers(-4, 5, (R, F)).astype(F32)
    V[::N] = 6
    U = rng.integers(-3, 4, (R, F)).astype(F32)
    if relu & 1 and R > 2:
        dead = rng.random(R) < 0.1
        U[dead] = -30
    if N > 1:
        idx = rng.integers(1, N, (B, N, k)).astype(np.int32)
    else:
        idx = np.zeros((B, N, k), np.int32)
    t = rng.choice([c for c in (1, 2, 4) if c <= k], (B, N))
    order = np.argsort(rng.random((B, N, k)), axis=2)
    idx[order < t[:, :, None]] = 0
    return V, U, idx


def lattice_precondition(fw, dmax, dmean, p_xh=1, p_term=LATTICE_P, p_z=2, tie_counts=(1, 2, 4)):
    """Asserts, in float64 / integer arithmetic, that every term lies on the lattice and that no partial sum can leave the
    exactly representable range: max_f sum |dz xh| 2^p < 2^24 (and the same for sum |dz| and the forward's sum |z| 2^p_z).
    The defaults are the lattice above; a finer one names its spacings 2^-p_xh (xh), 2^-p_term (dz xh), 2^-p_z (z), and
    tie_counts=None where dz is an integer for every tie count that can occur (the lattice assertion on dz then stands for it).
    -> the float64 sums (exact)."""
    dz = dz64(fw, dmax, dmean)
    xh, z = fw.xh.astype(np.float64), fw.z.astype(np.float64)
    for a, p in ((dz, 0), (xh, p_xh), (dz * xh, p_term), (z, p_z)):
        assert np.array_equal(a * 2 ** p, np.round(a * 2 ** p)), "off the lattice"
    if tie_counts is not None:
        live = np.abs(dz).sum(1) > 0
        tl = fw.ties[live]
        assert np.isin(tl, tie_counts).all(), "a live point has a tie count outside %s" % (tie_counts,)
    s = Sums(dz, xh)
    assert s.abs1.max() * 2 ** p_term < 2 ** 24 and s.abs0.max() < 2 ** 24
    assert np.abs(z).sum(1).max() * 2 ** p_z < 2 ** 24
    assert np.array_equal(dz32(fw, dmax, dmean).astype(np.float64), dz)       # the fp32 dz is the float64 dz
    return s

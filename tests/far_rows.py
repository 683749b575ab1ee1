"""Inputs and float64 references for gathered rows that lie 2^31 elements or more past their base (tests/test_gpu_far_rows.py on the
GPU, tests/test_far_rows_reference.py on the CPU).  No GPU, no torch.

The edge-level kernels address neighbour row j of a cloud (or packed tower) as V + j * ldv with ONE 24-bit multiply (common.h:
row_offset24).  Their host checks admit j < N < 2^24, ldv < 2^24, N * ldv < 2^32, so an element offset in [2^31, 2^32) is inside the
contract -- and it is the range where a product held as `int` and sign-extended into the pointer sum lands 2^32 elements BEFORE
the row.  element_offset() models both readings of the same 32 product bits.

Two shapes:
  W   N = 160 rows with ld = 2^24 - 4 (rows 129.. far; a 10.7 GB buffer of which only the N x F view is ever written), F = 16,
      k = 5 (and 1, 20 for the statistics passes); dense (B = 1, and B = 2 with N = 132: rows 129..131 of each cloud) and packed
      (seg_off = 0, 40, 140, 160: cloud 1 straddles the 2^31 mark, cloud 2 lies beyond it; and the one-cloud tower 0, 160).
      Values sit on a lattice (V, U, mean, beta in quarters, rstd in {1/2, 1, 2}, dmax in 60 Z, dmean in k Z) on which every term
      and every partial sum of every pass is exact in fp32: results must EQUAL the float64 reference, in any summation order.
  R   N = 2^24 - 256 rows with ld = 132 (rows 16 268 816.. far), F = 4, k = 2, for the two statistics passes; the fp32 partial sums
      are not exact at 33 M terms, so the bound is the any-order summation bound of bn_reference.sum_bound."""
import functools

import numpy as np

import bn_reference as BR
import seg_bn_bwd_reference as SB

F32 = np.float32
FAR = 1 << 31

# ---- shape W
W_LD = (1 << 24) - 4
W_N, W_F, W_K = 160, 16, 5
W_KS = (1, 5, 20)                      # the statistics passes: one row, two row groups with a tail, five whole groups
W_N2 = 132                             # B = 2: rows 129..131 of each cloud are far
W_OFF = (0, 40, 140, 160)
W_FIRST_FAR = 129                      # 128 * (2^24 - 4) = 2^31 - 512
# ---- shape R
R_N, R_LD, R_F, R_K = (1 << 24) - 256, 132, 4, 2
R_OFF = (0, 5000000, 12000000, R_N)
R_FIRST_FAR = 16268816
# the lattice of shape W: spacings 2^-p of xh, dz * xh and z (bn_reference.lattice_precondition)
W_LATTICE = dict(p_xh=3, p_term=3, p_z=3, tie_counts=None)


def quarter(rng, shape, lo=-8, hi=9):
    return (rng.integers(lo, hi, shape) / 4.0).astype(np.float32)


def element_offset(j, ld, extend):
    """The element offset the address of row j takes under a 24-bit multiply (v_mul_u32_u24: the low 24 bits of each operand, the
    low 32 bits of the product), with those 32 bits entering the 64-bit pointer sum zero-extended ("zero": an unsigned product,
    what the contract needs) or sign-extended ("sign": the product held as int).  -> int64, the shape of j."""
    j = np.asarray(j).astype(np.uint64) & np.uint64(0xffffff)
    p = (j * np.uint64(int(ld) & 0xffffff)) & np.uint64(0xffffffff)
    if extend == "zero":
        return p.astype(np.int64)
    assert extend == "sign"
    return np.ascontiguousarray(p.astype(np.uint32)).view(np.int32).astype(np.int64)


def is_far(j, ld):
    return element_offset(j, ld, "zero") >= FAR


def rows_read(idx, ld, extend, stand_in=0):
    """The row each index resolves to under the model; an offset outside the buffer (negative) is replaced by row `stand_in`."""
    off = element_offset(idx, ld, extend)
    assert (off[off >= 0] % ld == 0).all()
    return np.where(off < 0, stand_in, off // ld).astype(np.int32)


def neighbours(rng, off, k, ld):
    """idx (rows, k) int32, rows relative to the base of ONE V operand whose clouds are rows [off[b], off[b + 1]); every point's
    neighbours lie in its own cloud.  Column 0 mirrors the cloud (row lo + hi - 1 - i): every row is some point's neighbour.  Then
    points whose neighbours are all near get a far row of their cloud in column k - 1, until a quarter of all points have a far
    neighbour.  (k = 1: column k - 1 IS column 0, and 160 points cannot both cover 160 rows and send 40 of themselves to the 31
    far ones; the quarter and every far row are kept, a few near rows lose their only reader.)"""
    off = [int(o) for o in off]
    rows = off[-1]
    far = is_far(np.arange(rows), ld)
    idx = np.empty((rows, k), np.int32)
    for lo, hi in zip(off[:-1], off[1:]):
        idx[lo:hi] = rng.integers(lo, hi, (hi - lo, k))
        idx[lo:hi, 0] = lo + hi - 1 - np.arange(lo, hi)
    need = -(-rows // 4) - int(far[idx].any(1).sum())
    for lo, hi in zip(off[:-1], off[1:]):
        fr = lo + np.flatnonzero(far[lo:hi])
        if need <= 0 or not len(fr):
            continue
        cand = lo + np.flatnonzero(~far[idx[lo:hi]].any(1))[:need]
        idx[cand, k - 1] = fr[np.arange(len(cand)) % len(fr)]
        need -= len(cand)
    assert need <= 0
    return idx


class Case(object):
    pass


def _params(rng, c, tables):
    F = c.F
    shape = (tables, F) if tables else (F,)
    c.mu = quarter(rng, shape, -2, 3)
    c.rs = rng.choice(np.array([0.5, 1.0, 2.0], F32), shape)
    c.be = quarter(rng, (F,), -4, 5)
    c.dmax = (60 * rng.integers(-2, 3, (c.R, F))).astype(F32)          # 60 / ties is an integer for ties = 1 .. 5
    c.dmean = (c.k * rng.integers(-1, 2, (c.R, F))).astype(F32)        # fl(k m * fl(1 / k)) = m (asserted: dz32 == dz64)


@functools.lru_cache(maxsize=None)
def dense_case(B, N, k, F=W_F, ld=W_LD):
    """B clouds of N rows; idx (B, N, k) holds rows of the point's own cloud (what the dense entries take)."""
    rng = np.random.default_rng(1000 * B + 10 * N + k)
    c = Case()
    c.B, c.N, c.k, c.F, c.ld, c.R = B, N, k, F, ld, B * N
    c.V, c.U = quarter(rng, (c.R, F)), quarter(rng, (c.R, F))
    c.idx = np.stack([neighbours(rng, (0, N), k, ld) for _ in range(B)])
    _params(rng, c, 0)
    for a in (c.V, c.U, c.idx, c.mu, c.rs, c.be, c.dmax, c.dmean):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def packed_case(off, k, F=W_F, ld=W_LD):
    """One tower; idx (rows, k) holds tower rows of the point's own cloud; mu / rs are (nseg, F) tables."""
    rng = np.random.default_rng(7000 + 10 * len(off) + k)
    c = Case()
    c.off, c.k, c.F, c.ld, c.R, c.nseg = np.asarray(off, np.int32), k, F, ld, int(off[-1]), len(off) - 1
    c.sizes = [int(b - a) for a, b in zip(off[:-1], off[1:])]
    c.row_group = np.repeat(np.arange(c.nseg, dtype=np.int32), c.sizes)
    c.V, c.U = quarter(rng, (c.R, F)), quarter(rng, (c.R, F))
    c.idx = neighbours(rng, off, k, ld)
    _params(rng, c, c.nseg)
    for a in (c.V, c.U, c.idx, c.mu, c.rs, c.be, c.dmax, c.dmean, c.off, c.row_group):
        a.setflags(write=False)
    return c


def one_cloud_tower(d):
    """The dense case d (B = 1) as a packed tower of one cloud: the same rows, graph and gradients, mean / rstd as (1, F) tables."""
    assert d.B == 1
    c = Case()
    c.off, c.k, c.F, c.ld, c.R, c.nseg, c.sizes = np.array([0, d.N], np.int32), d.k, d.F, d.ld, d.N, 1, [d.N]
    c.row_group = np.zeros(d.N, np.int32)
    c.V, c.U, c.idx, c.be, c.dmax, c.dmean = d.V, d.U, d.idx[0], d.be, d.dmax, d.dmean
    c.mu, c.rs = d.mu[None], d.rs[None]
    return c


def stats64(y):
    """(2, F) float64 column sums and sums of squares of the fp32 rows y (..., F), asserted exact in fp32 in any order:
    sum |y| in quarters and sum y^2 in sixteenths stay below 2^24."""
    y = np.asarray(y, np.float64).reshape(-1, y.shape[-1])
    assert np.array_equal(y * 4, np.round(y * 4)), "off the lattice"
    assert np.abs(y).sum(0).max() * 4 < 2 ** 24 and (y * y).sum(0).max() * 16 < 2 ** 24
    return np.stack([y.sum(0), (y * y).sum(0)])


def dense_reference(c, relu, idx=None, exact=True):
    """Every output of the dense entries on case c, from bn_reference.py: y (R, k, F) fp32, stats (2, F) float64, max / mean / packed
    count, red (2, F) float64, dY (R, k, F) and dYsum (R, F) fp32 (the replay given red).  idx: the rows actually read (default:
    c.idx); exact: assert the lattice preconditions (the sums are then exact in fp32 in any order)."""
    y = BR.edge_rows32(c.V, c.U, c.idx if idx is None else idx, c.B, c.N)
    y64 = y.astype(np.float64)
    st = stats64(y) if exact else np.stack([y64.sum((0, 1)), (y64 * y64).sum((0, 1))])
    if c.k != W_K:                                    # k = 1, 20: the statistics passes only (dmax / ties is exact for ties <= 5)
        return dict(y=y, stats=st)
    fw = BR.Fwd(y, c.mu, c.rs, c.be, relu)
    s = BR.lattice_precondition(fw, c.dmax, c.dmean, **W_LATTICE) if exact else BR.Sums(BR.dz64(fw, c.dmax, c.dmean), fw.xh)
    dY, dYsum = BR.apply32(BR.dz32(fw, c.dmax, c.dmean), fw.xh, fw.rs, s.red, c.R * c.k)
    return dict(y=y, stats=st, max=fw.mx, mean=fw.mean32, packed=fw.packed, red=s.red, dY=dY, dYsum=dYsum)


def packed_reference(c, relu, idx=None, exact=True):
    """The same for the packed entries, cloud by cloud (seg_bn_bwd_reference.py): stats and red are (nseg, 2, F), c1 / c2 (nseg, F)."""
    y = c.V[c.idx if idx is None else idx] + c.U[:, None, :]
    assert y.dtype == F32
    st = []
    for _, lo, hi in SB.clouds(c.off):
        y64 = y[lo:hi].astype(np.float64)
        st.append(stats64(y[lo:hi]) if exact else np.stack([y64.sum((0, 1)), (y64 * y64).sum((0, 1))]))
    if c.k != W_K:
        return dict(y=y, stats=np.stack(st))
    cases = SB.edge_clouds(y, c.off, c.mu, c.rs, c.be, relu, c.dmax, c.dmean)
    red = np.stack([BR.lattice_precondition(fw, c.dmax[lo:hi], c.dmean[lo:hi], **W_LATTICE).red if exact else s.red
                    for (_, lo, hi), (fw, _, s) in zip(SB.clouds(c.off), cases)])
    c1, c2, _ = SB.finalize32(red, c.sizes, c.k)
    dY, dYsum = SB.apply32(cases, red, c.k)
    return dict(y=y, stats=np.stack(st), max=np.concatenate([fw.mx for fw, _, _ in cases]),
                mean=np.concatenate([fw.mean32 for fw, _, _ in cases]), packed=np.concatenate([fw.packed for fw, _, _ in cases]),
                red=red, c1=c1, c2=c2, dY=dY, dYsum=dYsum)


# ------------------------------------------------------------------------------------------------------------------ shape R
def _r_sums(V, U, idx):
    """(3, F) float64 over the points of U (n, F) with neighbours idx (n, k): sum y, sum y^2, sum |y| (y = V[idx] + U, one fp32 add)."""
    out = np.zeros((3, V.shape[1]))
    for m in range(idx.shape[1]):
        y = V[idx[:, m]] + U                          # quarters up to 4: y * y is exact in fp32; the sums accumulate in float64
        out[0] += y.sum(0, dtype=np.float64)
        out[1] += (y * y).sum(0, dtype=np.float64)
        out[2] += np.abs(y).sum(0, dtype=np.float64)
    return out


@functools.lru_cache(maxsize=None)
def r_case():
    """Shape R: V, U (N, 4) in quarters, idx (N, 2) tower rows inside the point's own cloud of R_OFF (so the dense entry with B = 1
    takes the same graph).  Column 0 mirrors the cloud; column 1 sends every point of the last cloud -- 28 % of all points -- to
    a far row, all far rows in turn, and shifts the other clouds by a third of their size.  sums: (nseg, 3, F) float64 per cloud (sum y, sum y^2, sum |y|)."""
    rng = np.random.default_rng(132)
    c = Case()
    c.N, c.ld, c.F, c.k, c.off, c.nseg = R_N, R_LD, R_F, R_K, np.asarray(R_OFF, np.int32), len(R_OFF) - 1
    c.sizes = [int(b - a) for a, b in zip(R_OFF[:-1], R_OFF[1:])]
    c.V = (rng.integers(-8, 9, (R_N, R_F), dtype=np.int8) / F32(4)).astype(F32)
    c.U = (rng.integers(-8, 9, (R_N, R_F), dtype=np.int8) / F32(4)).astype(F32)
    idx = np.empty((R_N, R_K), np.int32)
    i = np.arange(R_N, dtype=np.int64)
    nfar = R_N - R_FIRST_FAR
    for b, (lo, hi) in enumerate(zip(R_OFF[:-1], R_OFF[1:])):
        idx[lo:hi, 0] = lo + hi - 1 - i[lo:hi]
        idx[lo:hi, 1] = (R_FIRST_FAR + i[lo:hi] % nfar) if b == c.nseg - 1 else (lo + (i[lo:hi] - lo + (hi - lo) // 3) % (hi - lo))
    c.idx = idx
    c.sums = np.stack([_r_sums(c.V, c.U[lo:hi], idx[lo:hi]) for lo, hi in zip(R_OFF[:-1], R_OFF[1:])])
    for a in (c.V, c.U, c.idx, c.sums, c.off):
        a.setflags(write=False)
    return c


def r_sums_under(c, extend):
    """The per-cloud sums with the rows the model reads (only the last cloud holds far rows: the others are c.sums')."""
    lo, hi = R_OFF[-2], R_OFF[-1]
    out = np.array(c.sums)
    out[-1] = _r_sums(c.V, c.U[lo:hi], rows_read(c.idx[lo:hi], c.ld, extend))
    return out

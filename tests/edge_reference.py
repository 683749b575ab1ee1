"""Plain numpy restatement of the kernels that read the k-NN graph idx (B, N, k): the edge tensor E = [x_i, x_j - x_i] and its
products (csrc/gemm.hip: A_EDGE, A_EDGE_T, E_SCATTER, edge_wgrad_smallc_kernel), the explicit gather and its transpose, the
transposed adjacency and the sums over incoming edges (csrc/misc.hip, det.hip).  No GPU, no torch.

* E is formed in float32 (edges32): the one subtraction x_j - x_i is the only rounding a kernel may make before its products,
  so every kernel must form exactly these values.  Everything downstream is float64, and every sum comes with its SCALE, the
  same sum over absolute values of the terms, which is what an fp32 summation error is measured against
  (bn_reference.sum_bound).
* incoming_sum32_replay repeats csr_gather_sum_kernel's additions in float32, in its order, for bit-exact expectations.
* Lattice operands: small integers for x, multiples of 1/8 for weights and gradients.  Every product and every partial sum is
  then exactly representable in fp32 (lattice_precondition), no result depends on a summation order and a kernel must EQUAL
  the float64 value -- a dropped, doubled or wrong-row term is off by a whole term.
* Clouds differ: x carries a per-cloud offset and every generator draws each cloud on its own, so a read from the wrong cloud
  changes the result.

Rows are global: point r = b * N + i, edge e = r * k + m."""
import numpy as np

import bn_reference as BR

F32 = np.float32
f32 = BR.f32


# ------------------------------------------------------------------------------------------------------------------ indices
def nbr_rows(idx):
    """Global row of the neighbour of every edge, (B N k,) int64."""
    B, N, k = idx.shape
    return (np.arange(B, dtype=np.int64)[:, None, None] * N + idx.astype(np.int64)).reshape(-1)


def point_rows(idx):
    """Global row of the centre point of every edge, (B N k,) int64."""
    B, N, k = idx.shape
    return np.repeat(np.arange(B * N, dtype=np.int64), k)


def in_degrees(idx):
    B, N, k = idx.shape
    return np.bincount(nbr_rows(idx), minlength=B * N)


# ------------------------------------------------------------------------------------------------------------- edge tensor
def edges32(x, idx):
    """E (B N k, 2C) float32 = [x_i, x_j - x_i] with the subtraction in float32; x (B N, C)."""
    x = f32(x)
    cen = x[point_rows(idx)]
    E = np.concatenate([cen, x[nbr_rows(idx)] - cen], 1)
    assert E.dtype == F32
    return E


def _mm(A, B):
    """float64 product and its scale |A| |B|."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    return A @ B, np.abs(A) @ np.abs(B)


def mlp64(x, idx, W0):
    """Y = E W0 -> (Y, scale) float64 (B N k, F); 2C terms per element."""
    return _mm(edges32(x, idx), W0)


def nbr_gemm64(x, idx, Wb, U):
    """Y[e] = x[nbr(e)] Wb + U[point(e)] -> (Y, scale); C + 1 terms per element."""
    Y, s = _mm(f32(x)[nbr_rows(idx)], Wb)
    Up = np.asarray(U, np.float64)[point_rows(idx)]
    return Y + Up, s + np.abs(Up)


def wgrad64(x, idx, dY):
    """dW0 = E^T dY -> (dW0, |E|^T |dY|) float64 (2C, F); B N k terms per element.  bn_reference.wgrad64 subtracts in float64;
    here E is edges32, the values a kernel multiplies (the two agree wherever the subtraction is exact)."""
    return _mm(edges32(x, idx).T, dY)


def nbr_wgrad64(x, idx, dY):
    """dWb = x[nbr]^T dY -> (dWb, scale) float64 (C, F)."""
    return _mm(f32(x)[nbr_rows(idx)].T, dY)


def _scatter_rows(R, rows, vals):
    out = np.zeros((R,) + vals.shape[1:])
    np.add.at(out, rows, vals)
    return out


def scatter64(dY, W0, idx):
    """dx[nbr(e)] += dY[e] W0[C:]^T -> (dx, scale) float64 (B N, C); F * in-degree terms per row."""
    B, N, k = idx.shape
    C = W0.shape[0] // 2
    G, s = _mm(dY, np.asarray(W0)[C:].T)
    rows = nbr_rows(idx)
    return _scatter_rows(B * N, rows, G), _scatter_rows(B * N, rows, s)


def gather_bwd64(dE, idx):
    """Transpose of edges32: dx[i] += sum_m (dE[e, :C] - dE[e, C:]), dx[nbr(e)] += dE[e, C:] -> (dx, scale) (B N, C)."""
    B, N, k = idx.shape
    dE = np.asarray(dE, np.float64)
    C = dE.shape[1] // 2
    dc, dn = dE[:, :C], dE[:, C:]
    rows = nbr_rows(idx)
    dx = (dc - dn).reshape(B * N, k, C).sum(1) + _scatter_rows(B * N, rows, dn)
    sc = (np.abs(dc) + np.abs(dn)).reshape(B * N, k, C).sum(1) + _scatter_rows(B * N, rows, np.abs(dn))
    return dx, sc


# ---------------------------------------------------------------------------------------------------- transposed adjacency
def csr(idx):
    """-> (off (B N + 1,) exclusive prefix of the in-degrees, rev (B N k,) the edges bucketed by target, every bucket in
    ascending edge order (stable sort)).  bincount / cumsum / argsort only: usable at a million points."""
    B, N, k = idx.shape
    tgt = nbr_rows(idx)
    deg = np.bincount(tgt, minlength=B * N)
    off = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    rev = np.argsort(tgt, kind="stable").astype(np.int64)
    return off, rev


def incoming_sum64(dY, idx):
    """S[j] = sum of dY[e] over the edges that point at j -> (S, scale) float64 (B N, F)."""
    B, N, k = idx.shape
    dY = np.asarray(dY, np.float64)
    rows = nbr_rows(idx)
    return _scatter_rows(B * N, rows, dY), _scatter_rows(B * N, rows, np.abs(dY))


def incoming_sum32_replay(dY, off, rev):
    """csr_gather_sum_kernel's own additions in float32, bucket by bucket in the order of `rev`: groups of four as
    (v0 + v1) + (v2 + v3) added to the accumulator, then the tail one row at a time.  Vectorised over the buckets."""
    dY = f32(dY)
    off, rev = np.asarray(off, np.int64), np.asarray(rev, np.int64)
    R = off.size - 1
    deg = off[1:] - off[:-1]
    acc = np.zeros((R, dY.shape[1]), F32)
    for s in range(int(deg.max(initial=0)) // 4):
        b = np.nonzero(deg >= 4 * (s + 1))[0]
        p = off[b] + 4 * s
        v0, v1, v2, v3 = (dY[rev[p + q]] for q in range(4))
        acc[b] = acc[b] + ((v0 + v1) + (v2 + v3))
    for t in range(3):
        b = np.nonzero(deg % 4 > t)[0]
        p = off[b] + (deg[b] // 4) * 4 + t
        acc[b] = acc[b] + dY[rev[p]]
    assert acc.dtype == F32
    return acc


# ------------------------------------------------------------------------------------------------------------------ graphs
# every index lies in [0, N): the kernels do no bounds check
PLANTED = (0, 1, 2, 3, 4, 5, 7, 8, 9)         # in-degrees of the first nine points of every cloud of a `degrees` graph


def g_random(rng, B, N, k):
    return rng.integers(0, N, (B, N, k)).astype(np.int32)


def g_permutation(rng, B, N, k):
    """Column m of every cloud is a permutation of its points: every in-degree is exactly k."""
    idx = np.empty((B, N, k), np.int32)
    for b in range(B):
        for m in range(k):
            idx[b, :, m] = rng.permutation(N)
    return idx


def g_hub(rng, B, N, k):
    """Every edge of a cloud points at one point of it (another one per cloud): in-degree N k, all others 0."""
    hub = rng.integers(0, N, B).astype(np.int32)
    return np.broadcast_to(hub[:, None, None], (B, N, k)).copy()


def g_last(rng, B, N, k):
    return np.full((B, N, k), N - 1, np.int32)


def g_self(rng, B, N, k):
    return np.broadcast_to(np.arange(N, dtype=np.int32)[None, :, None], (B, N, k)).copy()


def g_degrees(rng, B, N, k):
    """In-degrees PLANTED on points 0 .. 8 of every cloud (the unroll-by-4 loops and their tails of 0 .. 3), every other edge
    at a random point >= 9.  Needs N > 9 and N k >= sum(PLANTED) = 39."""
    assert N > len(PLANTED) and N * k >= sum(PLANTED)
    idx = rng.integers(len(PLANTED), N, (B, N * k)).astype(np.int32)
    plant = np.repeat(np.arange(len(PLANTED), dtype=np.int32), PLANTED)
    for b in range(B):
        idx[b, rng.permutation(N * k)[:plant.size]] = plant
    return idx.reshape(B, N, k)


GRAPHS = {"random": g_random, "permutation": g_permutation, "hub": g_hub, "last": g_last, "self": g_self, "degrees": g_degrees}


def graph(kind, rng, B, N, k):
    idx = GRAPHS[kind](rng, B, N, k)
    assert idx.dtype == np.int32 and idx.shape == (B, N, k) and idx.min() >= 0 and idx.max() < N
    return idx


# ---------------------------------------------------------------------------------------------------------------- operands
LATTICE_P = 6             # 2^-p = spacing of the finest terms (gradient * weight, both multiples of 1/8)


class Operands(object):
    """x (B N, C), idx, W0 (2C, F), U (B N, F), dY (B N k, F), dE (B N k, 2C), dx0 (B N, C) of one case, all float32.
    lattice: x integer in [-4, 4] + 9 * cloud (disjoint ranges), W0 / dY / dE multiples of 1/8 in [-1, 1] / [-1/2, 1/2], U / dx0 multiples of 1/8.
    random: normal, x shifted by the cloud number."""

    def __init__(self, lattice, seed, B, N, C, k, F, kind="random", need=("W0", "U", "dY", "dE", "dx0")):
        rng = np.random.default_rng(seed)
        self.lattice, self.B, self.N, self.C, self.k, self.F, self.kind = lattice, B, N, C, k, F, kind
        self.R, self.Me = B * N, B * N * k
        self.idx = graph(kind, rng, B, N, k)
        R, Me = self.R, self.Me
        cloud = np.repeat(np.arange(B), N)[:, None]
        shapes = {"W0": (2 * C, F), "U": (R, F), "dY": (Me, F), "dE": (Me, 2 * C), "dx0": (R, C)}
        if lattice:
            self.x = (rng.integers(-4, 5, (R, C)) + 9 * cloud).astype(F32)
            half = {"W0": 8, "U": 16, "dY": 4, "dE": 4, "dx0": 16}
            for n in need:
                setattr(self, n, (rng.integers(-half[n], half[n] + 1, shapes[n]) / 8.0).astype(F32))
        else:
            self.x = (rng.normal(size=(R, C)) + cloud).astype(F32)
            sd = {"W0": 0.3, "U": 1.0, "dY": 1.0, "dE": 1.0, "dx0": 1.0}
            for n in need:
                setattr(self, n, rng.normal(0, sd[n], shapes[n]).astype(F32))


def lattice_precondition(scale, values=()):
    """-> the largest sum |term| of any output element in lattice units (2^-LATTICE_P); the caller asserts it is < 2^24: then
    every partial sum, in any order, is a multiple of the unit below 2^24 units, i.e. exact in fp32.  `values`: arrays that
    must lie on the lattice themselves."""
    unit = 2.0 ** LATTICE_P
    for v in values:
        v = np.asarray(v, np.float64) * unit
        assert np.array_equal(v, np.round(v)), "off the lattice"
    s = np.asarray(scale, np.float64) * unit
    assert np.array_equal(s, np.round(s)), "a scale off the lattice"
    return float(s.max(initial=0.0))


# ------------------------------------------------------------------------------------------------ cases of the GPU module
# Shared with tests/test_edge_reference.py, which checks the lattice precondition of every one of them on the host.
def case_seed(case):
    """One seed per case tuple, the same in both modules."""
    return sum(int(v) * (i + 3) for i, v in enumerate(case) if not isinstance(v, str)) + len(case[-1])


def case_id(case):
    return "-".join(str(v) for v in case)


# forward forms (dgcnn_edge_mlp_f32, dgcnn_edge_nbr_gemm_f32): (B, N, C, k, F, graph)
FWD_CASES = [
    (1, 37, 3, 7, 8, "random"),           # scalar loader (C % 4 != 0), Me = 259: three row tiles, the last of 3 rows
    (2, 50, 6, 1, 30, "last"),            # scalar loader and scalar B (F % 4 != 0), k = 1, two clouds that all point at N - 1
    (2, 33, 4, 7, 100, "hub"),            # K = 8 < one k-slab of 16 on the float4 path; F = 100: a ragged column tile
    (1, 45, 20, 7, 64, "degrees"),        # k-slab 16 .. 31 straddles the centre / difference boundary at 20
    (3, 35, 36, 20, 128, "random"),       # k-slab 32 .. 47 straddles it at 36; 17 x 2 tiles of 128 x 64: the XCD-grouped tile order
    (2, 40, 64, 20, 64, "permutation"),   # the model's size
    (2, 1024, 64, 16, 128, "random"),     # cdiv(Me, 128) = 256 row tiles: the 128-column instantiation (gemm.hip:tile_n)
]
# weight gradients (dgcnn_edge_mlp_wgrad_f32, dgcnn_edge_nbr_wgrad_f32): (B, N, C, k, F, graph)
WGRAD_SMALLC = [
    (1, 1, 1, 1, 8, "self"),              # Me = 1
    (1, 9, 3, 7, 100, "random"),          # Me = 63
    (2, 32, 4, 1, 256, "last"),           # Me = 64
    (1, 13, 3, 5, 8, "hub"),              # Me = 65
    (1, 3277, 3, 20, 100, "random"),      # Me = 65540 > 65536: 1024 blocks of 65 edges, the last one of 5
    (3, 50, 1, 7, 256, "degrees"),
]
WGRAD_GEMM = [                             # each unsplit (Me / 256 < 2) and split
    (2, 25, 3, 7, 260, "hub"),            # scalar A_EDGE_T (F > 256 leaves the small-C kernel), Me = 350
    (2, 500, 3, 7, 260, "random"),        # Me = 7000: split
    (2, 27, 64, 7, 64, "last"),           # Me = 378
    (3, 300, 64, 7, 64, "random"),        # Me = 6300: split
    (1, 45, 20, 7, 100, "degrees"),       # Me = 315
    (2, 333, 20, 9, 100, "permutation"),  # Me = 5994: split
]
# dgcnn_edge_mlp_dgrad_scatter_f32: (B, N, C, k, F, graph)
SCATTER_CASES = [
    (2, 40, 3, 7, 30, "hub"), (2, 40, 4, 7, 64, "permutation"), (2, 30, 64, 5, 64, "self"), (1, 45, 64, 7, 30, "degrees"),
    (3, 50, 3, 20, 64, "degrees"), (2, 21, 4, 1, 30, "last"),
]
# dgcnn_edge_gather_f32 / dgcnn_edge_gather_bwd_f32: (B, N, C, k, graph)
GATHER_CASES = [(2, 40, 3, 7, "hub"), (1, 45, 64, 5, "degrees"), (3, 33, 5, 1, "last"), (2, 50, 4, 20, "random")]
# dgcnn_edge_gather_sum_f32 / _bf16: (B, N, k, graph) x F in GSUM_F
GSUM_CASES = [(2, 45, 7, "degrees"), (2, 40, 5, "hub"), (3, 33, 6, "permutation"), (1, 300, 20, "degrees")]
GSUM_F = (4, 8, 64, 68, 128, 256)

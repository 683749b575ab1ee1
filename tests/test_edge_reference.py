"""tests/edge_reference.py pinned down on the host: against torch float64 autograd of E = cat(x_i, x_j - x_i), Y = E W0, against
oracle.dgcnn_oracle.edges, np.add.at, and its own stated properties (in-degrees of the generators, replay == float64 on the
lattice, the lattice precondition of every lattice case tests/test_gpu_edge_kernels.py runs)."""
import numpy as np
import pytest
import torch

import bn_reference as BR
import edge_reference as ER
from oracle import dgcnn_oracle as O


def _autograd(x, idx, W0, dY):
    """Forward, dW0 and dx of Y = cat(x_i, x_j - x_i) W0 by torch float64 autograd; the subtraction is float64 here."""
    B, N, k = idx.shape
    xt = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    Wt = torch.tensor(np.asarray(W0, np.float64), requires_grad=True)
    nb = torch.from_numpy(ER.nbr_rows(idx))
    pt = torch.from_numpy(ER.point_rows(idx))
    E = torch.cat([xt[pt], xt[nb] - xt[pt]], 1)
    Y = E @ Wt
    Y.backward(torch.tensor(np.asarray(dY, np.float64)))
    return Y.detach().numpy(), Wt.grad.numpy(), xt.grad.numpy()


@pytest.mark.parametrize("kind", sorted(ER.GRAPHS))
def test_reference_equals_float64_autograd(kind):
    """On lattice operands the float32 subtraction of edges32 is exact, so forward, dW0 and dx equal autograd's; dx is put
    together from the pieces the kernels compute: scatter64 (neighbour half) + the centre half (sum_m dY) (Wa - Wb)^T."""
    B, N, C, k, F = 3, 17, 5, 4, 6
    o = ER.Operands(True, 5, B, N, C, k, F, kind)
    Y, dW, dx = _autograd(o.x, o.idx, o.W0, o.dY)
    np.testing.assert_array_equal(ER.mlp64(o.x, o.idx, o.W0)[0], Y)
    np.testing.assert_array_equal(ER.wgrad64(o.x, o.idx, o.dY)[0], dW)
    np.testing.assert_array_equal(dW, BR.wgrad64(o.x, o.idx, B, N, o.dY.reshape(B * N, k, F)))     # (float64 subtraction: same here)
    W64 = o.W0.astype(np.float64)
    centre = o.dY.astype(np.float64).reshape(B * N, k, F).sum(1) @ (W64[:C] - W64[C:]).T
    np.testing.assert_array_equal(ER.scatter64(o.dY, o.W0, o.idx)[0] + centre, dx)
    # factored form: E W0 = x_j Wb + x_i (Wa - Wb), dWb = x_j^T dY
    U = o.x.astype(np.float64) @ (W64[:C] - W64[C:])
    np.testing.assert_array_equal(ER.nbr_gemm64(o.x, o.idx, o.W0[C:], U)[0], Y)
    xi = o.x.astype(np.float64)[ER.point_rows(o.idx)]
    np.testing.assert_array_equal(ER.nbr_wgrad64(o.x, o.idx, o.dY)[0], dW[C:] + xi.T @ o.dY.astype(np.float64))
    # transpose of the explicit gather: dx of sum(E * dE)
    xt = torch.tensor(o.x.astype(np.float64), requires_grad=True)
    nb, pt = torch.from_numpy(ER.nbr_rows(o.idx)), torch.from_numpy(ER.point_rows(o.idx))
    (torch.cat([xt[pt], xt[nb] - xt[pt]], 1) * torch.tensor(o.dE.astype(np.float64))).sum().backward()
    np.testing.assert_array_equal(ER.gather_bwd64(o.dE, o.idx)[0], xt.grad.numpy())


def test_random_operands_within_the_rounding_of_one_subtraction():
    """Random operands: edges32 differs from the float64 edge tensor by the rounding of its one subtraction only."""
    B, N, C, k, F = 2, 23, 7, 5, 9
    o = ER.Operands(False, 6, B, N, C, k, F, "random")
    E = ER.edges32(o.x, o.idx)
    x64 = o.x.astype(np.float64)
    d64 = x64[ER.nbr_rows(o.idx)] - x64[ER.point_rows(o.idx)]
    np.testing.assert_array_equal(E[:, :C], o.x[ER.point_rows(o.idx)])
    assert (np.abs(E[:, C:] - d64) <= 2.0 ** -24 * np.abs(d64)).all()
    Y, dW, _ = _autograd(o.x, o.idx, o.W0, o.dY)
    Yr, Ys = ER.mlp64(o.x, o.idx, o.W0)
    assert (np.abs(Yr - Y) <= 2.0 ** -24 * Ys + 1e-300).all()
    Wr, Ws = ER.wgrad64(o.x, o.idx, o.dY)
    assert (np.abs(Wr - dW) <= 2.0 ** -24 * Ws + 1e-300).all()


@pytest.mark.parametrize("kind", ["random", "hub", "last"])
def test_edges32_equals_the_oracle(kind):
    B, N, C, k = 3, 19, 4, 6
    o = ER.Operands(False, 7, B, N, C, k, 4, kind, need=())
    ref = O.edges(o.x.reshape(B, N, C), k, o.idx)
    assert ref.dtype == np.float32
    np.testing.assert_array_equal(ER.edges32(o.x, o.idx), ref.reshape(B * N * k, 2 * C))
    dE = np.random.default_rng(1).integers(-4, 5, (B, N, k, 2 * C)).astype(np.float64)
    np.testing.assert_array_equal(ER.gather_bwd64(dE.reshape(-1, 2 * C), o.idx)[0], O.edges_bwd(dE, o.idx, B, N, C).reshape(B * N, C))


@pytest.mark.parametrize("kind", sorted(ER.GRAPHS))
def test_csr_against_add_at(kind):
    B, N, k, F = 3, 41, 5, 4
    rng = np.random.default_rng(8)
    idx = ER.graph(kind, rng, B, N, k)
    off, rev = ER.csr(idx)
    deg = np.zeros(B * N, np.int64)
    np.add.at(deg, ER.nbr_rows(idx), 1)
    np.testing.assert_array_equal(off, np.concatenate([[0], np.cumsum(deg)]))
    assert off[-1] == B * N * k
    np.testing.assert_array_equal(np.sort(rev), np.arange(B * N * k))
    np.testing.assert_array_equal(ER.nbr_rows(idx)[rev], np.repeat(np.arange(B * N), deg))
    for j in np.nonzero(deg > 1)[0][:50]:                                  # every bucket ascending
        assert (np.diff(rev[off[j]:off[j + 1]]) > 0).all()
    dY = rng.integers(-4, 5, (B * N * k, F)).astype(np.float32)
    want = np.zeros((B * N, F))
    for e, j in enumerate(ER.nbr_rows(idx)):                                # the definition, edge by edge
        want[j] += dY[e]
    S, sc = ER.incoming_sum64(dY, idx)
    np.testing.assert_array_equal(S, want)
    np.testing.assert_array_equal(sc[deg == 0], 0)
    np.testing.assert_array_equal(ER.incoming_sum32_replay(dY, off, rev).astype(np.float64), want)


def test_replay_keeps_the_kernels_order():
    """A bucket of 4 rows whose sum depends on the order, and a tail of 3 added one by one."""
    v2 = np.array([2.0 ** 24, 1.0, 1.0, 1.0], np.float32)[:, None]          # (2^24 + 1) + (1 + 1) = 2^24 + 2, sequentially 2^24
    assert ER.incoming_sum32_replay(v2, np.array([0, 4]), np.arange(4))[0, 0] == np.float32(2.0 ** 24 + 2)
    assert ER.incoming_sum32_replay(v2, np.array([0, 1, 4]), np.arange(4))[1, 0] == np.float32(3.0)


@pytest.mark.parametrize("kind", sorted(ER.GRAPHS))
def test_generators_have_their_stated_in_degrees(kind):
    B, N, k = 3, 29, 4
    idx = ER.graph(kind, np.random.default_rng(9), B, N, k)
    deg = ER.in_degrees(idx).reshape(B, N)
    assert deg.sum() == B * N * k
    if kind == "permutation":
        assert (deg == k).all()
    elif kind == "hub":
        assert ((deg == N * k).sum(1) == 1).all() and ((deg == 0).sum(1) == N - 1).all()
    elif kind == "last":
        assert (deg[:, -1] == N * k).all() and (deg[:, :-1] == 0).all()
    elif kind == "self":
        assert (deg == k).all() and (idx == np.arange(N)[None, :, None]).all()
    elif kind == "degrees":
        np.testing.assert_array_equal(deg[:, :9], np.broadcast_to(ER.PLANTED, (B, 9)))
        assert sorted(set(d % 4 for d in ER.PLANTED)) == [0, 1, 2, 3] and max(ER.PLANTED) >= 8


def test_clouds_differ():
    """A read from the wrong cloud must change the result: the clouds of x differ, lattice or not."""
    for lattice in (True, False):
        o = ER.Operands(lattice, 3, 3, 16, 4, 3, 4, "last", need=())
        x = o.x.reshape(3, 16, 4)
        assert not (x[0] == x[1]).any() and not (x[1] == x[2]).any()


# ---- the lattice precondition of every lattice case of the GPU module (same seeds, same operands)
LIMIT = 2.0 ** 24


@pytest.mark.parametrize("case", ER.FWD_CASES, ids=ER.case_id)
def test_lattice_precondition_forward(case):
    B, N, C, k, F, kind = case
    o = ER.Operands(True, ER.case_seed(case), B, N, C, k, F, kind, need=("W0", "U"))
    assert ER.lattice_precondition(ER.mlp64(o.x, o.idx, o.W0)[1], (o.x, o.W0)) < LIMIT
    assert ER.lattice_precondition(ER.nbr_gemm64(o.x, o.idx, o.W0[C:], o.U)[1], (o.U,)) < LIMIT


@pytest.mark.parametrize("case", ER.WGRAD_SMALLC + ER.WGRAD_GEMM, ids=ER.case_id)
def test_lattice_precondition_wgrad(case):
    B, N, C, k, F, kind = case
    o = ER.Operands(True, ER.case_seed(case), B, N, C, k, F, kind, need=("W0", "dY"))
    # (+ 1: beta = 1 onto a dW of multiples of 1/8 in [-2, 2])
    assert ER.lattice_precondition(ER.wgrad64(o.x, o.idx, o.dY)[1] + 2, (o.x, o.dY)) < LIMIT
    assert ER.lattice_precondition(ER.nbr_wgrad64(o.x, o.idx, o.dY)[1] + 2) < LIMIT


@pytest.mark.parametrize("case", ER.SCATTER_CASES, ids=ER.case_id)
def test_lattice_precondition_scatter(case):
    B, N, C, k, F, kind = case
    o = ER.Operands(True, ER.case_seed(case), B, N, C, k, F, kind, need=("W0", "dY", "dx0"))
    assert ER.lattice_precondition(ER.scatter64(o.dY, o.W0, o.idx)[1] + np.abs(o.dx0), (o.dY, o.W0, o.dx0)) < LIMIT


@pytest.mark.parametrize("case", ER.GATHER_CASES, ids=ER.case_id)
def test_lattice_precondition_gather_bwd(case):
    B, N, C, k, kind = case
    o = ER.Operands(True, ER.case_seed(case), B, N, C, k, 4, kind, need=("dE", "dx0"))
    assert ER.lattice_precondition(ER.gather_bwd64(o.dE, o.idx)[1] + np.abs(o.dx0), (o.dE, o.dx0)) < LIMIT


@pytest.mark.parametrize("case", ER.GSUM_CASES, ids=ER.case_id)
def test_lattice_precondition_incoming_sum(case):
    B, N, k, kind = case
    for F in ER.GSUM_F:
        o = ER.Operands(True, ER.case_seed(case) + F, B, N, 1, k, F, kind, need=("dY",))
        S, sc = ER.incoming_sum64(o.dY, o.idx)
        assert ER.lattice_precondition(sc, (o.dY,)) < LIMIT
        off, rev = ER.csr(o.idx)
        np.testing.assert_array_equal(ER.incoming_sum32_replay(o.dY, off, rev).astype(np.float64), S)   # replay == float64
        np.testing.assert_array_equal(BR.round_bf16(o.dY), o.dY)                                       # bf16-representable


def test_round_bf16_reference():
    """Ties to even, carries into the exponent, and NaNs stay NaNs (the plain formula turns 0x7fffffff into -0.0)."""
    u = np.array([0x3f807fff, 0x3f808000, 0x3f808001, 0x3f817fff, 0x3f818000, 0x3f818001, 0x7f7fffff, 0xff7fffff,
                  0x7fffffff, 0xffffffff, 0x7fc00000, 0x7f800001, 0x00000001, 0x80008000, 0x7f800000], np.uint32)
    want = np.array([0x3f800000, 0x3f800000, 0x3f810000, 0x3f810000, 0x3f820000, 0x3f820000, 0x7f800000, 0xff800000,
                     0x7fff0000, 0xffff0000, 0x7fc00000, 0x7fc00000, 0x00000000, 0x80000000, 0x7f800000], np.uint32)
    got = BR.round_bf16(u.view(np.float32)).view(np.uint32)
    np.testing.assert_array_equal(got, want)

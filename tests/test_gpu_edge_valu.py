"""The instruction-count forms of the edge-level BatchNorm passes (csrc/bn.hip) against the kernels they stand in for:
  bn_act_kreduce_held_kernel<KC>         conv0's BN + ReLU + max / mean / tie and positive counts with a point's k x 4 values held in
                                         registers (ReLU, k <= 20), against the loop of bn_act_kreduce_kernel<4, true>;
  edge_bwd_apply_wgrad_exact_kernel<C>   the first layer's whole conv0 backward at its exact input width (C = 3, 4), against
                                         edge_bwd_apply_wgrad_kernel<4> and its run-time C.
Every case runs both on the same buffers -- dgcnn_edge_valu(1) and dgcnn_edge_valu(0), the in-process form of DGCNN_EDGE_VALU -- and
compares every output as uint32: -0.0 and NaN payloads count.  What the values ARE is held to float64 bars elsewhere
(tests/test_gpu_bn_kernels.py, tests/test_gpu_edge_kernels.py run the default, i.e. the new forms where they apply); here only "the
same bits" is asserted, plus the few properties named in the cases.  Shapes: two clouds of N = k + 1 and N = 37 points (cloud offsets,
a grid tail), k around the group size of 4 and around the register-held limit of 20, F = 16 / 64 / 128 (4, 16, 32 lanes per row)."""
import numpy as np
import pytest
import torch

from far_rows import quarter
from gpu_helpers import Guard, host
from launch_trace import launches, names

pytestmark = pytest.mark.gpu

HELD_K = 20                      # csrc/bn.hip: HELD_K
KS = [1, 3, 4, 5, 20, 21, 24]    # 21, 24: above the limit -- the loop kernel with the switch on
FS = [16, 64, 128]
CNT_POS = 256


@pytest.fixture()
def H():
    import dgcnn
    dgcnn.reset()
    from dgcnn import _hip
    return _hip


class switch(object):
    def __init__(self, H, on):
        self.lib, self.on = H.load(), on

    def __enter__(self):
        self.prev = self.lib.dgcnn_edge_valu(self.on)

    def __exit__(self, *exc):
        self.lib.dgcnn_edge_valu(self.prev)
        return False


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b, what):
    a, b = bits(a), bits(b)
    assert a.shape == b.shape
    bad = np.argwhere(a != b)
    assert not len(bad), "%s: %d of %d words differ, first at %s: %08x != %08x" % (
        what, len(bad), a.size, tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])])


def inputs(kind, seed, B, N, k, F):
    """-> V, U (B N, F), idx (B, N, k), mean, rstd, beta (F,).  The values sit on a lattice of quarters with power-of-two rstd, so every
    z is exact and several rows of a point share the maximum."""
    rng = np.random.default_rng(seed)
    R = B * N
    V, U = quarter(rng, (R, F)), quarter(rng, (R, F))
    idx = rng.integers(0, N, (B, N, k)).astype(np.int32)
    mu = quarter(rng, (F,), -2, 3)
    rs = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), F)
    be = quarter(rng, (F,), -4, 5)
    if kind == "nonpos":                          # every z <= 0 before the ReLU: max 0, all k rows tie
        be = np.full(F, -64.0, np.float32)
    elif kind == "negzero":                       # zeros of both signs in every operand; z = max(+-0, 0) and small values around it
        V = rng.choice(np.array([-0.0, 0.0, 0.25, -0.25], np.float32), (R, F))
        U = rng.choice(np.array([-0.0, 0.0], np.float32), (R, F))
        mu = rng.choice(np.array([-0.0, 0.0], np.float32), F)
        be = rng.choice(np.array([-0.0, 0.0], np.float32), F)
    elif kind == "nonfinite":
        flat = V.reshape(-1)
        pos = rng.choice(flat.size, max(3, flat.size // 7), replace=False)
        flat[pos] = rng.choice(np.array([np.inf, -np.inf, np.nan], np.float32), pos.size)
        flat[pos[0]] = np.array([0xffc12345], np.uint32).view(np.float32)[0]          # a NaN with a payload and a sign
    elif kind == "random":
        V, U = rng.normal(size=(R, F)).astype(np.float32), rng.normal(size=(R, F)).astype(np.float32)
        mu, be = rng.normal(size=F).astype(np.float32), rng.normal(size=F).astype(np.float32)
        rs = rng.uniform(0.5, 2.0, F).astype(np.float32)
    else:
        assert kind == "lattice"
    return V, U, idx, mu, rs, be


class Case(object):
    """The device buffers of one case ([U | V] rows with a pad, as the engine lays them out)."""

    def __init__(self, kind, seed, B, N, k, F):
        self.B, self.N, self.k, self.F, self.R = B, N, k, F, B * N
        V, U, idx, mu, rs, be = inputs(kind, seed, B, N, k, F)
        self.g = g = Guard()
        self.ld = 2 * F + 4
        self.UV = g.new((self.R, self.ld))
        self.UV[:, :F] = torch.from_numpy(U).cuda()
        self.UV[:, F:2 * F] = torch.from_numpy(V).cuda()
        self.idx = g.put(idx)
        self.par = [g.put(a) for a in (mu, rs, be)]

    def head(self):
        F = self.F
        return (self.UV[:, F:].data_ptr(), self.ld, self.UV.data_ptr(), self.ld, self.idx.data_ptr(), self.B, self.N, self.k, F)

    def forward(self, H, relu=1):
        """-> host max, mean, packed count of the path the switch selects."""
        g, R, F = self.g, self.R, self.F
        wide = g.new((R, 2 * F + 4))
        cnt = g.new((R, F))
        H.call("dgcnn_edge_bn_act_kreduce_f32", *self.head(), *(t.data_ptr() for t in self.par), relu, wide.data_ptr(), 2 * F + 4,
               wide[:, F:].data_ptr(), 2 * F + 4, cnt.data_ptr())
        w = host(wide)
        return w[:, :F].copy(), w[:, F:2 * F].copy(), host(cnt)

    def backward(self, H, x, ldx, C, dmax, dmean, mx, cnt, red0):
        """-> host partial sums of the blocks, dW0 (on zeros), dbeta."""
        g, R, F = self.g, self.R, self.F
        red = g.zeros((H.stat_slots(), 2, F), torch.float64)
        red[0] = torch.from_numpy(red0).cuda()
        xd = g.new((R, ldx))
        xd[:, :C] = torch.from_numpy(x).cuda()
        ops = [g.put(a) for a in (dmax, dmean, mx, cnt)]
        grid = ((min(1024, max(1, -(-R * (F // 4) // 256))) + 7) // 8) * 8
        need = grid * 2 * C * F * 4
        ws = g.new((need // 4,))
        dW, dbeta = g.zeros((2 * C, F)), g.zeros((F,))
        H.call("dgcnn_edge_bn_bwd_apply_wgrad_f32", *self.head(), *(t.data_ptr() for t in self.par), ops[0].data_ptr(), F,
               ops[1].data_ptr(), F, ops[2].data_ptr(), F, ops[3].data_ptr(), red.data_ptr(), xd.data_ptr(), ldx, C, dW.data_ptr(),
               dbeta.data_ptr(), 0.0, ws.data_ptr(), need)
        return host(ws), host(dW), host(dbeta)


def both(H, fn):
    with switch(H, 1):
        new = fn()
    with switch(H, 0):
        old = fn()
    return new, old


# ---- forward ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("k", KS)
def test_forward_max_mean_counts_are_the_loop_kernels_bits(H, k, F):
    for N in (k + 1, 37):
        c = Case("lattice", 1000 * k + F + N, 2, N, k, F)
        new, old = both(H, lambda: c.forward(H))
        for a, b, what in zip(new, old, ("max", "mean", "packed count")):
            same_bits(a, b, "%s, N = %d" % (what, N))
        ties = new[2] % CNT_POS
        assert (ties >= 1).all() and (ties <= k).all() and (new[2] // CNT_POS <= k).all()
        if k >= 4:
            assert (ties > 1).any(), "the lattice gave no tie"
        c.g.check()


@pytest.mark.parametrize("k", [3, 20])
@pytest.mark.parametrize("kind", ["nonpos", "negzero", "nonfinite", "random"])
def test_forward_zeros_of_both_signs_and_non_finite_values(H, kind, k):
    F = 64
    c = Case(kind, 7 * k + len(kind), 2, 37, k, F)
    new, old = both(H, lambda: c.forward(H))
    for a, b, what in zip(new, old, ("max", "mean", "packed count")):
        same_bits(a, b, what)
    if kind == "nonpos":                           # max 0 (+0.0), every row ties, no row is positive
        assert not bits(new[0]).any() and (new[2] == k).all()
    if kind == "negzero":
        assert (new[0] >= 0).all() and not np.signbit(new[0]).any()      # a ReLU output is never -0.0
    if kind == "nonfinite":
        assert np.isinf(new[0]).any() and not np.isnan(new[0]).any()     # max(NaN, 0) = 0: a NaN row never reaches max or mean
    c.g.check()


def test_forward_without_a_relu_keeps_the_loop_and_its_signed_zeros(H):
    """relu = 0 is outside the register-held form (the first zero seen keeps its sign in the loop; v_max_f32 would not): both
    settings launch the loop kernel and give the same bits, NaN rows included."""
    for kind in ("negzero", "nonfinite"):
        c = Case(kind, 5, 2, 37, 20, 64)
        new, old = both(H, lambda: c.forward(H, relu=0))
        for a, b, what in zip(new, old, ("max", "mean", "packed count")):
            same_bits(a, b, what)
    with switch(H, 1), launches() as L:
        c.forward(H, relu=0)
    assert names(L) == ["bn_act_kreduce_kernel"], L


# ---- which kernels ran -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,groups", [(1, 1), (4, 1), (5, 2), (20, 5), (21, 0), (24, 0)])
def test_the_switch_and_the_limit_select_the_kernels(H, k, groups):
    c = Case("lattice", k, 2, 37, k, 64)
    with switch(H, 1), launches() as L:
        c.forward(H)
    if groups:
        assert [(e[0], e[1]) for e in L] == [("bn_act_kreduce_held_kernel", [str(4 * groups)])], L
    else:
        assert [(e[0], e[1]) for e in L] == [("bn_act_kreduce_kernel", ["4", "true"])], L
    with switch(H, 0), launches() as L0:
        c.forward(H)
    assert [(e[0], e[1]) for e in L0] == [("bn_act_kreduce_kernel", ["4", "true"])], L0
    assert L0[0][2:] == L[0][2:]                   # same grid, block and LDS either way


@pytest.mark.parametrize("C,on,off", [(3, ("edge_bwd_apply_wgrad_exact_kernel", ["3"]), ("edge_bwd_apply_wgrad_kernel", ["4"])),
                                      (4, ("edge_bwd_apply_wgrad_exact_kernel", ["4"]), ("edge_bwd_apply_wgrad_kernel", ["4"])),
                                      (2, ("edge_bwd_apply_wgrad_kernel", ["4"]), ("edge_bwd_apply_wgrad_kernel", ["4"]))])
def test_the_switch_selects_the_backward_kernel(H, C, on, off):
    c = Case("lattice", C, 2, 37, 5, 64)
    args = _backward_args(H, c, C, 4, 11)
    for sw, want in ((1, on), (0, off)):
        with switch(H, sw), launches() as L:
            c.backward(H, *args)
        assert [e[0] for e in L] == ["bn_bwd_finalize_kernel", want[0], "reduce_partials_kernel"], L
        assert L[1][1] == want[1] and L[1][3] == (256, 1, 1), L


# ---- backward --------------------------------------------------------------------------------------------------------------------
def _backward_args(H, c, C, ldx, seed, lattice=True):
    """x, ldx, C, dmax, dmean, max, packed count (from the forward of the path the switch selects now), BN sums."""
    rng = np.random.default_rng(seed)
    R, F = c.R, c.F
    x = (quarter(rng, (R, C)) if lattice else rng.normal(size=(R, C)).astype(np.float32))
    dmax, dmean = rng.normal(size=(R, F)).astype(np.float32), rng.normal(size=(R, F)).astype(np.float32)
    mx, _, cnt = c.forward(H)
    red0 = rng.normal(size=(2, F)) * R * c.k
    return x, ldx, C, dmax, dmean, mx, cnt, red0


@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("k", [1, 3, 4, 5, 20, 21])
@pytest.mark.parametrize("C,ldx", [(3, 3), (3, 4), (4, 4)])
def test_first_layer_backward_partials_and_dw0_are_the_loop_kernels_bits(H, C, ldx, k, F):
    for N, lattice in ((k + 1, True), (37, False)):
        c = Case("lattice" if lattice else "random", 31 * k + F + C + ldx, 2, N, k, F)
        out = []
        for sw in (1, 0):
            with switch(H, sw):
                out.append(c.backward(H, *_backward_args(H, c, C, ldx, 17 * k + F, lattice)))    # forward of the same path
        for a, b, what in zip(out[0], out[1], ("partial sums per block", "dW0", "dbeta")):
            same_bits(a, b, "%s, N = %d" % (what, N))
        assert np.abs(out[0][1]).max() > 0
        c.g.check()


def test_first_layer_backward_with_non_finite_rows(H):
    """+-inf and NaN in V through the backward.  Every word that is not a NaN is bit-equal, the NaNs sit in the same places and carry
    the same payload.  The SIGN of a NaN is not asserted, and in this one corner the rule "partial and dW0 are bit-identical, NaNs
    included" is NOT met: where one point's rows bring +inf, -inf and then a NaN to the running sum of dY (acc += o), the sum holds
    the NaN that inf - inf generated (ffc00000) and the row adds the input's (7fc00000).  Which of two NaN operands v_pk_add_f32
    propagates depends on operand position, and the compiler commutes the commutative add as it likes: in this library's
    edge_bwd_apply_wgrad_kernel<4> two of a group's four rows are emitted `acc, o, acc` and two `acc, acc, o` (the parent commit's
    build of the same source text emits all four `acc, acc, o`: the position changes with register allocation alone); in the
    exact kernel every row of a whole group is `acc, acc, o`, and its tail group has commuted rows of its own.  The order of
    operations is the same; the operand position is not something C++ source controls.  Measured on MI355X: the sign bit of 57 of 3072 words of
    this case (6 of 384 of dW0), all in the x_i rows, which are the ones that read acc; +-inf alone, NaN alone, and any order with
    the NaN first give equal bits.  Finite inputs, and everything in the forward, are held to strict uint32 equality above."""
    c = Case("nonfinite", 3, 2, 37, 20, 64)
    out = []
    for sw in (1, 0):
        with switch(H, sw):
            out.append(c.backward(H, *_backward_args(H, c, 3, 4, 9)))
    for a, b, what in zip(out[0], out[1], ("partial sums per block", "dW0", "dbeta")):
        na, nb = np.isnan(a), np.isnan(b)
        assert np.array_equal(na, nb), what
        same_bits(np.where(na, 0, a), np.where(nb, 0, b), what)
        same_bits(bits(a) & 0x7fffffff, bits(b) & 0x7fffffff, what + " (NaN payloads)")
        print("%s: %d words, %d NaN, %d differ in the sign of a NaN" % (what, a.size, int(na.sum()), int((bits(a) != bits(b)).sum())))
    assert np.isnan(out[0][1]).any()
    c.g.check()


def test_row_offsets_of_two_to_the_31_elements_and_more(H):
    """One cloud of 160 rows whose V and x are views into matrices with a leading dimension of 2^24 - 4: rows 129.. start 2^31
    elements or more past the cloud's first row (128 * (2^24 - 4) = 2^31 - 512), inside the N * ld < 2^32 the entries accept.  The
    24-bit product must enter the address zero-extended (HIP's __umul24 returns int); forward and backward against the loop
    kernels, which take this range.  Every other gathering entry in this range: tests/test_gpu_far_rows.py."""
    B, N, k, F, C = 1, 160, 5, 16, 3
    LD = (1 << 24) - 4
    assert (N - 1) * LD >= 1 << 31 and N * LD < 1 << 32
    rng = np.random.default_rng(31)
    V, U = quarter(rng, (N, F)), quarter(rng, (N, F))
    idx = rng.integers(0, N, (B, N, k)).astype(np.int32)
    idx[0, :, 0] = N - 1 - np.arange(N)                          # every row is some point's neighbour, the far ones too
    g = Guard()
    bigV = torch.empty((N - 1) * LD + F, dtype=torch.float32, device="cuda")
    bigX = torch.empty((N - 1) * LD + C, dtype=torch.float32, device="cuda")
    bigV.as_strided((N, F), (LD, 1)).copy_(torch.from_numpy(V).cuda())
    x = quarter(rng, (N, C))
    bigX.as_strided((N, C), (LD, 1)).copy_(torch.from_numpy(x).cuda())
    Ud, idxd = g.put(U), g.put(idx)
    par = [g.put(a) for a in (quarter(rng, (F,), -2, 3), rng.choice(np.array([0.5, 1.0, 2.0], np.float32), F), quarter(rng, (F,), -4, 5))]
    head = (bigV.data_ptr(), LD, Ud.data_ptr(), F, idxd.data_ptr(), B, N, k, F)
    pp = tuple(t.data_ptr() for t in par)
    dmax, dmean = (g.put(rng.normal(size=(N, F)).astype(np.float32)) for _ in range(2))
    red0 = rng.normal(size=(2, F)) * N * k
    grid = ((min(1024, max(1, -(-N * (F // 4) // 256))) + 7) // 8) * 8
    need = grid * 2 * C * F * 4
    out = []
    for sw in (1, 0):
        with switch(H, sw):
            mx, mn, cnt = g.new((N, F)), g.new((N, F)), g.new((N, F))
            H.call("dgcnn_edge_bn_act_kreduce_f32", *head, *pp, 1, mx.data_ptr(), F, mn.data_ptr(), F, cnt.data_ptr())
            red = g.zeros((H.stat_slots(), 2, F), torch.float64)
            red[0] = torch.from_numpy(red0).cuda()
            ws, dW, dbeta = g.new((need // 4,)), g.zeros((2 * C, F)), g.zeros((F,))
            H.call("dgcnn_edge_bn_bwd_apply_wgrad_f32", *head, *pp, dmax.data_ptr(), F, dmean.data_ptr(), F, mx.data_ptr(), F,
                   cnt.data_ptr(), red.data_ptr(), bigX.data_ptr(), LD, C, dW.data_ptr(), dbeta.data_ptr(), 0.0, ws.data_ptr(), need)
            out.append([host(t) for t in (mx, mn, cnt, ws, dW)])
    for a, b, what in zip(out[0], out[1], ("max", "mean", "packed count", "partial sums per block", "dW0")):
        same_bits(a, b, what)
    # the far rows were really read: the maximum over k of a point whose only positive neighbour is far away, on the host
    y = V[idx[0]] + U[:, None, :]
    mu, rs, be = (host(t) for t in par)
    z = np.maximum((y - mu) * rs + be, 0).max(1) + np.float32(0)
    same_bits(out[0][0], z.astype(np.float32), "max against the host")
    g.check()


# ---- a training step -------------------------------------------------------------------------------------------------------------
def _step(H, on):
    import dgcnn
    with switch(H, on):
        dgcnn.reset()
        flags = dgcnn.DGCNN_FLAGS(EDGE_CONV_LAYERS=2, EDGE_CONV_FILTERS=[64, 64], KVALUE=10, NUM_CHANNEL=3, FC_FILTERS=[128, 64],
                                  TRAIN=True, SEED=3)
        rng = np.random.default_rng(0)
        pts = rng.random((2, 256, 3), dtype=np.float32)
        lab = rng.integers(0, 2, (2, 256)).astype(np.int32)
        tv = dgcnn.trainval(flags).initialize()
        c = dgcnn.ctx()
        prev = H.TIMER
        H.TIMER = tm = H.Timer()
        try:
            tv.zero_gradients(None)
            _, acc, loss = tv.accum_gradient(None, [pts], [lab])
        finally:
            H.TIMER = prev
        grad = c.flat_grad.clone()
        tv.apply_gradient(None)
        return grad, c.flat_param.clone(), float(loss), set(tm.summary())


def test_a_training_step_of_the_small_model_is_bitwise_equal_with_the_switch_on_and_off(H):
    """The model of __graft_entry__.smoke(): 2 x 256 points, k = 10 (three groups of rows), widths (64, 64) + (128, 64); both
    EdgeConv layers run the forward pass in question, the first one the fused backward."""
    g1, p1, l1, tags = _step(H, 1)
    g0, p0, l0, _ = _step(H, 0)
    assert "edge_bwd_apply_wgrad_kernel" in tags, tags             # the engine's tag of the fused first-layer backward
    assert torch.equal(g1.view(torch.int32), g0.view(torch.int32)), "gradient bucket"
    assert torch.equal(p1.view(torch.int32), p0.view(torch.int32)), "parameters"
    assert l1 == l0 and np.isfinite(l1) and float(g1.abs().max()) > 0

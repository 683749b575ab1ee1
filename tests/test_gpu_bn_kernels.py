"""Every kernel of csrc/bn.hip and the deterministic reduce of csrc/det.hip against tests/bn_reference.py: float32 decisions and
replays bit for bit, sums against float64.  Each dispatch row of launch_act_kreduce / launch_bwd_reduce / launch_bwd_apply runs on

* an EXACT LATTICE input (every product and partial sum exactly representable: the kernel must EQUAL the float64 sums, in any
  summation order -- a dropped, duplicated or mis-owned row is off by a whole term), and
* a RANDOM input (true batch statistics through dgcnn_bn_finalize_f32, planted ties, all-dead points, a constant column, a
  column with mean 1e3 and std 1e-2) with derived bounds: decisions, dY and dYsum given `red` bit-equal to the float32 replay;
  sums within (n_terms + 8) 2^-24 sum |term| per column (any-order fp32 summation plus the roundings inside a term).

The bit-equal expectations rest on correctly rounded fp32 division (dmax / ties, 1.0f / k), on float64 division and multiplication
rounding as numpy's do, and on -ffp-contract=off; on gfx950 they hold for every case below, so no operation needed a one-ulp bound.

Every buffer a kernel writes sits between sentinel guards, and strided outputs inside wider sentinel-filled buffers: nothing
outside the documented extent may change.  The worst observed |err| / (2^-24 sum |term|) per kernel is printed at the end of the
module (and written to $DGCNN_BN_ERROR_TABLE when set; profiles/bn_kernel_errors.txt holds a measured copy)."""
import numpy as np
import pytest
import torch

import bn_reference as BR
from gpu_helpers import Guard, RATIOS, SENT, host, note_ratio, ptr as p, ratio_table

pytestmark = pytest.mark.gpu



@pytest.fixture()
def dg():
    import dgcnn
    dgcnn.reset()
    return dgcnn


@pytest.fixture(scope="module", autouse=True)
def _error_table():
    yield
    ratio_table()


def slots(H):
    return H.stat_slots()


class Dense(object):
    edge = False
    fwd, red, app = "dgcnn_bn_act_kreduce_f32", "dgcnn_bn_bwd_reduce_f32", "dgcnn_bn_bwd_apply_f32"

    def __init__(self, g, y, off=0):
        self.R, self.k, self.F = y.shape
        self.y = y
        self.Y = g.put(y.reshape(self.R * self.k, self.F), off=off)

    def head(self):
        return (self.Y.data_ptr(), self.R, self.k, self.F)


class Edge(object):
    edge = True
    fwd, red, app = "dgcnn_edge_bn_act_kreduce_f32", "dgcnn_edge_bn_bwd_reduce_f32", "dgcnn_edge_bn_bwd_apply_f32"

    def __init__(self, g, V, U, idx, B, N):
        self.B, self.N, self.k, self.F = B, N, idx.shape[-1], V.shape[1]
        self.R = B * N
        F = self.F
        self.ld = 2 * F + 4                                   # a [U | V] buffer with a pad
        self.UV = g.new((self.R, self.ld))
        self.UV[:, :F] = torch.from_numpy(U).cuda()
        self.UV[:, F:2 * F] = torch.from_numpy(V).cuda()
        self.idx = g.put(idx.astype(np.int32))
        self.y = BR.edge_rows32(V, U, idx, B, N)

    def head(self):
        F = self.F
        return (self.UV[:, F:].data_ptr(), self.ld, self.UV.data_ptr(), self.ld, self.idx.data_ptr(), self.B, self.N, self.k, F)


def run_forward(H, g, src, par, relu, want_mean=True, want_cnt=True, out2=False, ldpad=4):
    """-> host (max, mean or None, cnt or None, out2 or None); checks the pad columns of the wide output buffer."""
    R, F = src.R, src.F
    ld = 2 * F + ldpad
    wide = g.new((R, ld))
    mx, mn = wide[:, :F], (wide[:, F:2 * F] if want_mean else None)
    cnt = g.new((R, F)) if want_cnt else None
    o2w = g.new((R, F + ldpad)) if out2 else None
    o2 = o2w[:, :F] if out2 else None
    tail = (mx.data_ptr(), ld, p(mn), ld if want_mean else 0)
    if src.edge:
        assert not out2
        H.call(src.fwd, *src.head(), *par, relu, *tail, p(cnt))
    else:
        H.call(src.fwd, *src.head(), *par, relu, *tail, p(o2), (F + ldpad) if out2 else 0, p(cnt))
    w = host(wide)
    lo = 2 * F if want_mean else F
    assert (w[:, lo:] == SENT).all(), "the forward wrote pad columns"
    if out2:
        assert (host(o2w)[:, F:] == SENT).all()
    return (w[:, :F].copy(), w[:, F:2 * F].copy() if want_mean else None, host(cnt) if want_cnt else None,
            host(o2w)[:, :F].copy() if out2 else None)


def run_reduce(H, g, src, par, relu, dmax, dmean, mx, cnt, ldpad=0, off=0, name=None):
    """-> the (2, F) totals of a zeroed red buffer (sum over its slots)."""
    R, F = src.R, src.F
    ld = F + ldpad
    dmw = g.new((R, ld), off=off)
    dmw[:, :F] = torch.from_numpy(dmax).cuda()
    dnw = None
    if dmean is not None:
        dnw = g.new((R, ld))
        dnw[:, :F] = torch.from_numpy(dmean).cuda()
    mxd = g.put(mx) if mx is not None else None
    cnd = g.put(cnt) if mx is not None else None
    red = g.zeros((slots(H), 2, F), torch.float64)
    H.call(name or src.red, *src.head(), *par, relu, dmw.data_ptr(), ld, p(dnw), ld if dnw is not None else 0, p(mxd), F if mxd is not None else 0,
           p(cnd), red.data_ptr())
    return host(red).sum(0)


def run_apply(H, g, src, par, relu, dmax, dmean, mx, cnt, red_in, prior=None, dbeta_beta=0.0, in_place=False, want_sum=True, ldpad=0, off=0):
    """red_in (2, F) float64 goes to slot 0 of a zeroed red.  -> host (dY (R, k, F), dYsum or None, dbeta, red slot 0 afterwards)."""
    R, k, F = src.R, src.k, src.F
    ld = F + ldpad
    dmw = g.new((R, ld), off=off)
    dmw[:, :F] = torch.from_numpy(dmax).cuda()
    dnw = None
    if dmean is not None:
        dnw = g.new((R, ld))
        dnw[:, :F] = torch.from_numpy(dmean).cuda()
    mxd = g.put(mx) if mx is not None else None
    cnd = g.put(cnt) if mx is not None else None
    red = g.zeros((slots(H), 2, F), torch.float64)
    red[0] = torch.from_numpy(np.ascontiguousarray(red_in)).cuda()
    dY = src.Y if in_place else g.new((R * k, F), off=off)
    dsw = g.new((R, F + 4)) if want_sum else None
    dbeta = g.put(np.zeros(F, np.float32) if prior is None else prior)
    H.call(src.app, *src.head(), *par, relu, dmw.data_ptr(), ld, p(dnw), ld if dnw is not None else 0, p(mxd), F if mxd is not None else 0,
           p(cnd), red.data_ptr(), dY.data_ptr(), p(dsw), F + 4 if want_sum else 0, dbeta.data_ptr(), float(dbeta_beta))
    if want_sum:
        assert (host(dsw)[:, F:] == SENT).all(), "the apply pass wrote dYsum's pad columns"
    return host(dY).reshape(R, k, F).copy(), (host(dsw)[:, :F].copy() if want_sum else None), host(dbeta), host(red)[0]


def gpu_stats(H, g, rows2d):
    """True batch statistics of fp32 rows through dgcnn_bn_finalize_f32 (float64 column sums spread over the slots).
    -> host (mean, rstd) fp32, checked against the float64 formula and against a two-pass float64 variance."""
    n, F = rows2d.shape
    Yd = rows2d.astype(np.float64)
    S, Q = Yd.sum(0), (Yd * Yd).sum(0)
    st = g.zeros((slots(H), 2, F), torch.float64)
    st[0, 0], st[0, 1] = torch.from_numpy(S).cuda(), torch.from_numpy(Q).cuda()
    mean, rstd = g.new((F,)), g.new((F,))
    H.call("dgcnn_bn_finalize_f32", st.data_ptr(), F, float(n), BR.EPS, mean.data_ptr(), rstd.data_ptr())
    mu64, rs64 = BR.finalize64(S, Q, n)
    m, r = host(mean).copy(), host(rstd).copy()
    # one fp32 rounding of a float64 value (+ a float64 ulp or two inside)
    assert (np.abs(m - mu64) <= 2.0 ** -24 * np.abs(mu64) * 1.001 + 1e-45).all()
    assert (np.abs(r - rs64) <= 2.0 ** -24 * np.abs(rs64) * 1.001).all()
    # Q / n - mu^2 in float64 against the two-pass variance of the same data: the cancellation costs <= (n + 4) 2^-53 Q / n
    mu2, var2 = BR.two_pass_stats64(rows2d)
    dvar = (n + 4) * 2.0 ** -53 * (Q / n)
    rs2 = 1.0 / np.sqrt(var2 + BR.EPS)
    assert (np.abs(r - rs2) <= rs2 * (2.0 ** -23 + 0.5 * dvar / (var2 + BR.EPS))).all()
    return m, r


def random_rows(rng, R, k, F, relu):
    y = rng.normal(size=(R, k, F)).astype(np.float32)
    if k > 1:
        y[: max(1, R // 3), 1] = y[: max(1, R // 3), 0]              # planted ties
    if relu and R >= 4:
        nd = max(1, R // 10)
        y[-nd:] = -50 - rng.random((nd, k, F)).astype(np.float32)    # points whose k rows are all dead
    if R * k >= 8:
        y[:, :, 0] = 1.25                                            # constant column: var = 0, rstd = 1 / sqrt(eps), everything ties
        if F >= 2:
            y[:, :, -1] = (1000 + 0.01 * rng.normal(size=(R, k))).astype(np.float32)     # Q / n - mu^2 cancellation
    return y


def random_grads(rng, R, F, with_mean=True):
    return rng.normal(size=(R, F)).astype(np.float32), (rng.normal(size=(R, F)).astype(np.float32) if with_mean else None)


def check_passes(H, src, g, mu, rs, be, relu, dmax, dmean, exact, tag, off=0, ldpad=0, fwd_ldpad=4, k1=False):
    """forward, reduce (mx_in given / NULL) and apply of one source against the reference."""
    R, k, F = src.R, src.k, src.F
    par_t = [g.put(a) for a in (mu, rs, be)]
    par = tuple(t.data_ptr() for t in par_t)
    fw = BR.Fwd(src.y, mu, rs, be, relu)
    s = BR.lattice_precondition(fw, dmax, dmean) if exact else BR.Sums(BR.dz64(fw, dmax, dmean), fw.xh)
    d32 = BR.dz32(fw, dmax, dmean)
    cnt_ref = fw.packed if src.edge else fw.ties
    # ---- forward
    mx, mn, cnt, _ = run_forward(H, g, src, par, relu, want_mean=not k1, ldpad=fwd_ldpad)
    np.testing.assert_array_equal(mx, fw.mx, err_msg=tag + ": max")
    np.testing.assert_array_equal(cnt, cnt_ref, err_msg=tag + ": tie / positive counts")
    if not k1:
        np.testing.assert_array_equal(mn, fw.mean32, err_msg=tag + ": mean (fp32 replay)")
        if exact:
            np.testing.assert_array_equal(mn.astype(np.float64), fw.mean64, err_msg=tag + ": mean (float64)")
    # ---- reduce
    kern = ("edge" if src.edge else "k1" if k1 else "dense<%d>" % (4 if (F % 4 == 0 and not off and not ldpad) else 1))
    forms = [(fw.mx, cnt_ref), (None, None)] if dmean is not None else [(None, None)]
    for mxi, cni in forms:
        got = run_reduce(H, g, src, par, relu, dmax, dmean, mxi, cni, ldpad=ldpad, off=off)
        if exact:
            np.testing.assert_array_equal(got, s.red, err_msg="%s: red (%s)" % (tag, "mx_in" if mxi is not None else "recomputed max"))
        else:
            # (k = 1, float4-loadable operands, no mx_in: the column-fixed kernel, `dmean` being its second gradient input)
            k1_two = kern == "dense<4>" and k == 1 and mxi is None and dmean is not None
            note_ratio("bwd_reduce " + ("k1 (two gradients)" if k1_two else kern), got - s.red, s.scale, s.n_terms, s.n_terms + 8)
    # ---- apply, given the float64 sums
    prior = np.arange(F, dtype=np.float32)
    eo, eacc = BR.apply32(d32, fw.xh, fw.rs, s.red, R * k)
    for (mxi, cni), bb in zip(forms, (1.0, 0.0)):
        dY, dsum, dbeta, red0 = run_apply(H, g, src, par, relu, dmax, dmean, mxi, cni, s.red, prior=prior, dbeta_beta=bb, ldpad=ldpad, off=off)
        np.testing.assert_array_equal(dY, eo, err_msg=tag + ": dY")
        np.testing.assert_array_equal(dsum, eacc, err_msg=tag + ": dYsum")
        np.testing.assert_array_equal(dbeta, BR.dbeta32(s.red[0], prior, bb), err_msg=tag + ": dbeta")
        np.testing.assert_array_equal(red0, s.red, err_msg=tag + ": red slot 0 after the apply")
        if k1:
            np.testing.assert_array_equal(dsum, dY[:, 0])
    # the replay itself against the float64 layer: the roundings inside dz (quotient, 1 / k, product, sum), of c1, c2, the product,
    # two differences and rs * -- a check of the reference, not of the kernel
    ref = BR.dy64(BR.dz64(fw, dmax, dmean), fw.xh, fw.rs, s.red)
    n = R * k
    parts = BR.dz64(fw, np.abs(dmax), None if dmean is None else np.abs(dmean))          # |dmax| / ties + |dmean| / k under the same masks
    scale = np.abs(fw.rs.astype(np.float64)) * (parts + np.abs(s.red[0] / n) + np.abs(fw.xh * (s.red[1] / n)))
    assert (np.abs(eo - ref) <= 12 * 2.0 ** -24 * scale + 1e-30).all(), tag + ": the fp32 dY is not the float64 dY"
    g.check()
    return fw, s


# ------------------------------------------------------------------------------------------------------------------ dense
# The grids are capped (grid_for: 4096 workgroups, grid_reduce: 1024), so an item loop `q += its.step` runs a second time only above
# 256 x 1024 items in the reduce and 256 x 4096 in the forward / apply.  (9000, 1, 128): 288000 quad items, mean_out and mx_in given so
# that the general kernels are taken at k = 1 -- a second trip in the <4> reduce.  (17000, 1, 64) misaligned: 1088000 scalar items --
# a second trip in all three <1> kernels.  (Within R k F <= 4e6 the <4> forward / apply cannot reach their cap.)
DENSE4 = [(100, 7, 64, 1), (37, 20, 128, 0), (513, 4, 48, 1), (5, 128, 8, 1), (3, 2, 1024, 0), (9000, 1, 128, 1)]
DENSE1 = [(1000, 1, 3, 1, 0), (257, 1, 2, 0, 0), (64, 5, 70, 1, 0), (100, 7, 64, 1, 1), (17000, 1, 64, 1, 1)]   # last field: misaligned operands


def _dense_case(H, R, k, F, relu, kind, mis=0, k1=False, second=False):
    rng = np.random.default_rng(1000 * R + 10 * k + F + (kind == "lattice"))
    g = Guard()
    exact = kind == "lattice"
    if exact:
        k = BR.nearest_pow2(k)
        mu, rs, be = BR.lattice_params(rng, F)
        y = BR.lattice_dense(rng, R, k, F, relu)
        dmax, dmean = BR.lattice_grads(rng, R, k, F, with_mean=(not k1) or second)
    else:
        y = random_rows(rng, R, k, F, relu)
        mu, rs = gpu_stats(H, g, y.reshape(R * k, F))
        be = rng.normal(0, 0.3, F).astype(np.float32)
        dmax, dmean = random_grads(rng, R, F, with_mean=(not k1) or second)
    src = Dense(g, y, off=mis)
    if k1 and second:                              # k = 1: `dmean` is the gradient of a second consumer, dz = d + d2 (one fp32 add)
        return _k1_second(H, g, src, mu, rs, be, relu, dmax, dmean, exact)
    return check_passes(H, src, g, mu, rs, be, relu, dmax, dmean, exact, "%s (%d,%d,%d)" % (kind, R, k, F), off=mis, ldpad=mis,
                        fwd_ldpad=5 if mis else 4, k1=k1)


@pytest.mark.parametrize("kind", ["lattice", "random"])
@pytest.mark.parametrize("R,k,F,relu", DENSE4)
def test_dense_vector_kernels(dg, R, k, F, relu, kind):
    """bn_act_kreduce / bn_bwd_reduce / bn_bwd_apply <4, false>: F % 4 == 0, aligned; (513, 4, 48): F / 4 is no power of two, so
    split_item divides."""
    from dgcnn import _hip as H
    _dense_case(H, R, k, F, relu, kind)


@pytest.mark.parametrize("kind", ["lattice", "random"])
@pytest.mark.parametrize("R,k,F,relu,mis", DENSE1)
def test_dense_scalar_kernels(dg, R, k, F, relu, mis, kind):
    """The <1, false> instantiations: F % 4 != 0 (the Final layer with 2 - 5 classes) or operands one float off alignment with
    leading dimensions that are no multiple of 4."""
    from dgcnn import _hip as H
    _dense_case(H, R, k, F, relu, kind, mis=mis)


# --------------------------------------------------------------------------------------------------------------------- K1
# F in {4, 12, 64, 100, 1024, 1028, 1728} x R in {1, 3, 85, 1000, 4097}, except that R = 4097 at F >= 1024 would exceed the size limit
# of a GPU case (R F <= 4e6: 4097 x 1024 = 4.2e6).  What those shapes were for is the ROW LOOP of the column-fixed reduce: k1_grid caps
# its grid at 256 workgroups of RP = 256 / min(F / 4, 256) row groups with 4 rows in flight, so `r += 4 * rstep` makes a second trip
# only for R > 1024 RP -- R > 1024 at F >= 1024 (with and without the second blockIdx.y), R > 10240 at F = 100.  In their place:
# (2049, 1024), (3000, 1028), (2049, 1728) (two / three trips, ragged last trip), and (12000, 100) for a width whose F / 4 is no
# power of two.
K1 = ([(R, F) for F in (4, 12, 64, 100) for R in (1, 3, 85, 1000, 4097)] + [(R, F) for F in (1024, 1028, 1728) for R in (1, 3, 85, 1000)] +
      [(2049, 1024), (3000, 1028), (2049, 1728), (12000, 100)])


def _k1_second(H, g, src, mu, rs, be, relu, d1, d2, exact):
    R, F = src.R, src.F
    par = tuple(g.put(a).data_ptr() for a in (mu, rs, be))
    fw = BR.Fwd(src.y, mu, rs, be, relu)
    dsum = (d1 + d2).astype(np.float32)                                  # the kernel's single fp32 add
    s = BR.Sums(BR.dz64(fw, dsum, None), fw.xh)
    got = run_reduce(H, g, src, par, relu, d1, d2, None, None)
    if exact:
        BR.lattice_precondition(fw, dsum, None)
        np.testing.assert_array_equal(got, s.red)
    else:
        note_ratio("bwd_reduce k1 (two gradients)", got - s.red, s.scale, s.n_terms, s.n_terms + 8)
    eo, eacc = BR.apply32(BR.dz32(fw, dsum, None), fw.xh, fw.rs, s.red, R)
    dY, ds, dbeta, _ = run_apply(H, g, src, par, relu, d1, d2, None, None, s.red)
    np.testing.assert_array_equal(dY, eo)
    np.testing.assert_array_equal(ds, eacc)
    np.testing.assert_array_equal(dbeta, BR.dbeta32(s.red[0]))
    g.check()


@pytest.mark.parametrize("kind", ["lattice", "random"])
@pytest.mark.parametrize("R,F", K1)
def test_k1_column_fixed_kernels(dg, R, F, kind):
    """bn1_act_kernel / bn1_bwd_kernel<false / true> (k == 1, no mean_out, no mx_in): F / 4 not a power of two (12, 100), F > 1024
    (second blockIdx.y, with ONE live quad at 1028), R below one row group, R % (4 RP) != 0, more rows than the capped grid of the
    reduce covers in one trip (see K1 above)."""
    from dgcnn import _hip as H
    _dense_case(H, R, 1, F, (R + F // 4) % 2, kind, k1=True)


@pytest.mark.parametrize("kind", ["lattice", "random"])
@pytest.mark.parametrize("R,F", [(85, 12), (1000, 64), (3, 1028), (2049, 1028)])
def test_k1_second_gradient_input(dg, R, F, kind):
    from dgcnn import _hip as H
    _dense_case(H, R, 1, F, 1, kind, k1=True, second=True)


# ------------------------------------------------------------------------------------------------------------------- edge
# (B, N, k, F, relu); (4, 2100, 2, 128): 268800 quad items, more than the capped grid of the reduce covers in one trip
EDGE = [(1, 5, 3, 8, 1), (3, 77, 7, 64, 1), (9, 40, 6, 16, 0), (2, 50, 1, 8, 1), (1, 130, 255, 4, 0), (4, 2100, 2, 128, 1), (3, 77, 7, 64, 0)]


def _edge_inputs(H, g, rng, B, N, k, F, relu, exact):
    if exact:
        k = BR.nearest_pow2(k, cap=BR.CNT_POS - 1)
        mu, rs, be = BR.lattice_params(rng, F)
        V, U, idx = BR.lattice_edge(rng, B, N, k, F, relu)
        dmax, dmean = BR.lattice_grads(rng, B * N, k, F)
    else:
        V = rng.normal(size=(B * N, F)).astype(np.float32)
        U = rng.normal(size=(B * N, F)).astype(np.float32)
        idx = rng.integers(0, N, (B, N, k)).astype(np.int32)
        idx[:, ::3, 0] = np.arange(N, dtype=np.int32)[::3]                      # self
        if k > 1:
            idx[:, 1::4, 1] = idx[:, 1::4, 0]                                   # duplicates: exact ties
        idx[-1, N // 2:] = 0                                                    # every row -> point 0
        if relu and B * N >= 4:
            U[-max(1, B * N // 10):] -= 50                                      # all-dead points
        if B * N * k >= 8:
            V[:, 0], U[:, 0] = 0.5, 0.75                                        # constant column
            V[:, -1] = (1000 + 0.01 * rng.normal(size=B * N)).astype(np.float32)
            U[:, -1] = (0.01 * rng.normal(size=B * N)).astype(np.float32)
        y = BR.edge_rows32(V, U, idx, B, N)
        mu, rs = gpu_stats(H, g, y.reshape(B * N * k, F))
        be = rng.normal(0, 0.3, F).astype(np.float32)
        dmax, dmean = random_grads(rng, B * N, F)
    return V, U, idx, mu, rs, be, dmax, dmean


@pytest.mark.parametrize("kind", ["lattice", "random"])
@pytest.mark.parametrize("B,N,k,F,relu", EDGE)
def test_edge_kernels(dg, B, N, k, F, relu, kind):
    """The <4, true> instantiations (y = V[cloud N + idx] + U recomputed) on a [U | V] buffer with a padded leading dimension;
    (1, 5, 3, 8): fewer points than XCD ranges; idx with self, duplicates, every row -> point 0.  Also the per-point closed form
    dgcnn_edge_bn_bwd_reduce_points_f32 (a ReLU layer by definition) against the edge-level float64 sums."""
    from dgcnn import _hip as H
    rng = np.random.default_rng(B * 1000 + N + k + (kind == "lattice"))
    g = Guard()
    exact = kind == "lattice"
    V, U, idx, mu, rs, be, dmax, dmean = _edge_inputs(H, g, rng, B, N, k, F, relu, exact)
    src = Edge(g, V, U, idx, B, N)
    fw, s = check_passes(H, src, g, mu, rs, be, relu, dmax, dmean, exact, "%s edge (%d,%d,%d,%d)" % (kind, B, N, src.k, F))
    # the materialising twin writes the same rows
    Y = g.new((src.R * src.k, F))
    H.call("dgcnn_edge_gather_add_f32", *src.head(), Y.data_ptr(), 0)
    np.testing.assert_array_equal(host(Y).reshape(src.R, src.k, F), src.y)
    if not relu:
        g.check()
        return
    # ---- the per-point closed form
    R, kk = src.R, src.k
    red = g.zeros((slots(H), 2, F), torch.float64)
    mxd, mnd, cnd, dmd, dnd, bed = (g.put(a) for a in (fw.mx, fw.mean32, fw.packed, dmax, dmean, be))
    H.call("dgcnn_edge_bn_bwd_reduce_points_f32", mxd.data_ptr(), F, mnd.data_ptr(), F, cnd.data_ptr(), dmd.data_ptr(), F, dnd.data_ptr(), F,
           bed.data_ptr(), R, kk, F, red.data_ptr())
    got = host(red).sum(0)
    if exact:
        np.testing.assert_array_equal(got, s.red)
    else:
        # the closed form replaces xh by z - beta and sum z by k mean: 4 2^-24 sum |dz| (|xh| + 2 |beta|), plus the summation term
        dz = np.abs(BR.dz64(fw, dmax, dmean))
        extra = 4 * 2.0 ** -24 * (dz * (np.abs(fw.xh) + 2 * np.abs(be.astype(np.float64)))).sum((0, 1))
        bound = np.stack([BR.sum_bound(s.n_terms, s.abs0), BR.sum_bound(s.n_terms, s.abs1) + extra])
        err = np.abs(got - s.red)
        ratio = float((err / np.maximum(2.0 ** -24 * s.scale, 1e-300))[s.scale > 0].max(initial=0.0))
        print("reduce_points: worst err / bound = %.3g, worst err / (2^-24 sum|term|) = %.4g" % (float((err / np.maximum(bound, 1e-300)).max()), ratio))
        if ratio > RATIOS.get("edge_bwd_reduce_points", [-1])[0]:              # the bound column: what is asserted, in the same units
            RATIOS["edge_bwd_reduce_points"] = [ratio, s.n_terms, float((bound / np.maximum(2.0 ** -24 * s.scale, 1e-300))[s.scale > 0].min(initial=np.inf))]
        assert (err <= bound).all()
    g.check()


# ---------------------------------------------------------------------------------------------------------------- options
def test_forward_options_out2_counts_and_strides(dg):
    from dgcnn import _hip as H
    rng = np.random.default_rng(5)
    for (R, k, F) in [(100, 7, 64), (85, 1, 12), (64, 5, 70), (1000, 1, 3)]:
        g = Guard()
        y = random_rows(rng, R, k, F, 1)
        mu, rs = gpu_stats(H, g, y.reshape(R * k, F))
        be = rng.normal(0, 0.3, F).astype(np.float32)
        par = tuple(g.put(a).data_ptr() for a in (mu, rs, be))
        src = Dense(g, y)
        fw = BR.Fwd(y, mu, rs, be, 1)
        mx, mn, cnt, o2 = run_forward(H, g, src, par, 1, want_mean=(k > 1), out2=True, ldpad=4 if F % 4 == 0 else 3)
        np.testing.assert_array_equal(mx, fw.mx)
        np.testing.assert_array_equal(o2, mx)                                   # out2 is a second copy of max_out
        np.testing.assert_array_equal(cnt, fw.ties)
        if k == 1:
            assert (cnt == 1).all()                                             # cnt_out is all ones at k = 1
            mx1, _, _, _ = run_forward(H, g, src, par, 1, want_mean=True, want_cnt=False)      # the general kernel at k = 1
            np.testing.assert_array_equal(mx1, mx)
        g.check()


@pytest.mark.parametrize("R,k,F", [(100, 7, 64), (1000, 1, 64), (64, 5, 70)])
def test_apply_in_place_and_dbeta_accumulation(dg, R, k, F):
    """dY aliasing Y (every row of a point is in registers before its first store) and dbeta_beta in {0, 1} with a prior dbeta."""
    from dgcnn import _hip as H
    rng = np.random.default_rng(R + F)
    g = Guard()
    y = random_rows(rng, R, k, F, 1)
    mu, rs = gpu_stats(H, g, y.reshape(R * k, F))
    be = rng.normal(0, 0.3, F).astype(np.float32)
    par = tuple(g.put(a).data_ptr() for a in (mu, rs, be))
    dmax, dmean = random_grads(rng, R, F, with_mean=k > 1)
    fw = BR.Fwd(y, mu, rs, be, 1)
    s = BR.Sums(BR.dz64(fw, dmax, dmean), fw.xh)
    eo, eacc = BR.apply32(BR.dz32(fw, dmax, dmean), fw.xh, fw.rs, s.red, R * k)
    prior = rng.normal(size=F).astype(np.float32)
    for bb in (0.0, 1.0):
        for mxi, cni in ([(fw.mx, fw.ties), (None, None)] if k > 1 else [(None, None)]):
            src = Dense(g, y)
            dY, dsum, dbeta, _ = run_apply(H, g, src, par, 1, dmax, dmean, mxi, cni, s.red, prior=prior, dbeta_beta=bb, in_place=True)
            np.testing.assert_array_equal(dY, eo)
            np.testing.assert_array_equal(dsum, eacc)
            np.testing.assert_array_equal(dbeta, BR.dbeta32(s.red[0], prior, bb))
    g.check()


@pytest.mark.parametrize("R,k,F,edge,two", [(100, 7, 64, False, False), (64, 5, 70, False, False), (120, 1, 8, False, False),
                                            (120, 1, 8, False, True), (120, 6, 16, True, False)])
def test_bf16_flag_rounds_dy_and_sums_the_rounded_values(dg, R, k, F, edge, two):
    """relu = 3: dY values are bf16 (16 zero low bits), equal round-to-nearest-even of the fp32 replay, and dYsum adds the rounded
    values; also at k = 1, where the flag selects the general kernel -- with one gradient input and with two (no mx_in)."""
    from dgcnn import _hip as H
    rng = np.random.default_rng(R + k)
    g = Guard()
    if edge:
        B, N = 3, R // 3
        V, U, idx, mu, rs, be, dmax, dmean = _edge_inputs(H, g, rng, B, N, k, F, 1, False)
        src = Edge(g, V, U, idx, B, N)
    else:
        y = random_rows(rng, R, k, F, 1)
        mu, rs = gpu_stats(H, g, y.reshape(R * k, F))
        be = rng.normal(0, 0.3, F).astype(np.float32)
        dmax, dmean = random_grads(rng, R, F, with_mean=k > 1 or two)
        src = Dense(g, y)
    par = tuple(g.put(a).data_ptr() for a in (mu, rs, be))
    fw = BR.Fwd(src.y, mu, rs, be, 1)
    s = BR.Sums(BR.dz64(fw, dmax, dmean), fw.xh)
    eo, eacc = BR.apply32(BR.dz32(fw, dmax, dmean), fw.xh, fw.rs, s.red, R * k, bf16=True)
    mxi, cni = ((fw.mx, fw.packed if edge else fw.ties) if (dmean is not None and not two) else (None, None))
    dY, dsum, _, _ = run_apply(H, g, src, par, 3, dmax, dmean, mxi, cni, s.red)
    assert not (dY.view(np.uint32) & 0xffff).any()
    np.testing.assert_array_equal(dY, eo)
    np.testing.assert_array_equal(dsum, eacc)
    plain, _ = BR.apply32(BR.dz32(fw, dmax, dmean), fw.xh, fw.rs, s.red, R * k)
    assert (dY != plain).any()
    g.check()


def test_relu_flag_means_the_same_in_every_pass(dg):
    """Bit 1 of `relu` (bf16 dY) exists in the two apply entry points only; every other entry point refuses anything but 0 / 1, so a
    reduce can never read `2` as "ReLU on" while the apply reads it as "off".  In the apply, 2 = round without ReLU."""
    from dgcnn import _hip as H
    rng = np.random.default_rng(9)
    R, k, F = 60, 4, 16
    g = Guard()
    y = random_rows(rng, R, k, F, 0)
    mu, rs = gpu_stats(H, g, y.reshape(R * k, F))
    be = rng.normal(0, 0.3, F).astype(np.float32)
    par = tuple(g.put(a).data_ptr() for a in (mu, rs, be))
    dmax, dmean = random_grads(rng, R, F)
    src = Dense(g, y)
    for bad in (2, 3, -1, 4):
        with pytest.raises(ValueError):
            run_forward(H, g, src, par, bad)
        with pytest.raises(ValueError):
            run_reduce(H, g, src, par, bad, dmax, dmean, None, None)
        ws = torch.empty(H.load().dgcnn_det_workspace_bytes(F), dtype=torch.uint8, device="cuda")
        red = g.zeros((slots(H), 2, F), torch.float64)
        dm = g.put(dmax)
        with pytest.raises(ValueError):
            H.call("dgcnn_bn_bwd_reduce_det_f32", *src.head(), *par, bad, dm.data_ptr(), F, 0, 0, 0, 0, 0, red.data_ptr(), ws.data_ptr(), ws.numel())
    for bad in (-1, 4):
        with pytest.raises(ValueError):
            run_apply(H, g, src, par, bad, dmax, dmean, None, None, np.zeros((2, F)))
    # the gather-sourced and the dropout-fused entry points
    B, N = 2, 30
    V, U, idx, _, _, _, _, _ = _edge_inputs(H, g, rng, B, N, k, F, 0, True)
    esrc = Edge(g, V, U, idx, B, N)
    seed = torch.tensor([77], dtype=torch.int64, device="cuda")
    T1, d1, o1 = g.put(y[:, 0]), g.put(dmax), g.new((R, F))
    red = g.zeros((slots(H), 2, F), torch.float64)
    dbeta = g.zeros((F,))
    for bad in (2, 3, -1):
        with pytest.raises(ValueError):
            run_forward(H, g, esrc, par, bad)
        with pytest.raises(ValueError):
            run_reduce(H, g, esrc, par, bad, dmax, dmean, None, None)
        with pytest.raises(ValueError):
            H.call("dgcnn_bn1_act_dropout_f32", T1.data_ptr(), R, F, *par, bad, 0.7, seed.data_ptr(), o1.data_ptr(), F)
        with pytest.raises(ValueError):
            H.call("dgcnn_bn1_bwd_dropout_f32", T1.data_ptr(), R, F, *par, bad, 0.7, seed.data_ptr(), d1.data_ptr(), F, red.data_ptr(),
                   o1.data_ptr(), dbeta.data_ptr(), 0.0)
    for bad in (-1, 4):
        with pytest.raises(ValueError):
            run_apply(H, g, esrc, par, bad, dmax, dmean, None, None, np.zeros((2, F)))
    assert (host(o1) == SENT).all() and not host(red).any()
    # relu = 2 in the apply: no ReLU, rounded -- consistent with a reduce called with relu = 0
    fw = BR.Fwd(y, mu, rs, be, 0)
    s = BR.Sums(BR.dz64(fw, dmax, dmean), fw.xh)
    got = run_reduce(H, g, src, par, 0, dmax, dmean, None, None)
    note_ratio("bwd_reduce dense<4>", got - s.red, s.scale, s.n_terms, s.n_terms + 8)
    eo, eacc = BR.apply32(BR.dz32(fw, dmax, dmean), fw.xh, fw.rs, s.red, R * k, bf16=True)
    dY, dsum, _, _ = run_apply(H, g, src, par, 2, dmax, dmean, None, None, s.red)
    np.testing.assert_array_equal(dY, eo)
    np.testing.assert_array_equal(dsum, eacc)
    g.check()


# ------------------------------------------------------------------------------------------------------------- stat slots
@pytest.mark.parametrize("nslots", [32, 256])
def test_every_stat_slot_is_reduced(dg, nslots):
    """`red` / `stats` pre-filled in several slots with integer-valued doubles (exact in any order): the apply pass must reduce all
    stat_slots of them into slot 0, dgcnn_bn_finalize_f32 must use all of them; at 32 and at 256 slots."""
    from dgcnn import _hip as H
    old = H.stat_slots()
    H.set_stat_slots(nslots)
    try:
        rng = np.random.default_rng(nslots)
        for (R, k, F) in [(50, 4, 16), (200, 1, 12), (30, 2, 5)]:
            g = Guard()
            redh = np.zeros((nslots, 2, F))
            for sl in (0, 1, 31, nslots - 1, nslots // 2 + 3):
                redh[sl] += rng.integers(-1000, 1000, (2, F))
            tot = redh.sum(0)
            mu, rs, be = BR.lattice_params(rng, F)
            y = BR.lattice_dense(rng, R, k, F, 1)
            dmax, dmean = BR.lattice_grads(rng, R, k, F, with_mean=k > 1)
            par = tuple(g.put(a).data_ptr() for a in (mu, rs, be))
            src = Dense(g, y)
            fw = BR.Fwd(y, mu, rs, be, 1)
            red = g.put(redh)
            dY, dsum, dbeta = g.new((R * k, F)), g.new((R, F)), g.new((F,))
            dm, dn = g.put(dmax), (g.put(dmean) if dmean is not None else None)
            H.call(src.app, *src.head(), *par, 1, dm.data_ptr(), F, p(dn), F if dn is not None else 0, 0, 0, 0, red.data_ptr(), dY.data_ptr(),
                   dsum.data_ptr(), F, dbeta.data_ptr(), 0.0)
            np.testing.assert_array_equal(host(red)[0], tot)
            np.testing.assert_array_equal(host(dbeta), tot[0].astype(np.float32))
            eo, eacc = BR.apply32(BR.dz32(fw, dmax, dmean), fw.xh, fw.rs, tot, R * k)
            np.testing.assert_array_equal(host(dY).reshape(R, k, F), eo)
            np.testing.assert_array_equal(host(dsum), eacc)
            # a reduce followed by an apply on the same buffer: the kernels' own slot choice
            red2 = g.zeros((nslots, 2, F), torch.float64)
            H.call(src.red, *src.head(), *par, 1, dm.data_ptr(), F, p(dn), F if dn is not None else 0, 0, 0, 0, red2.data_ptr())
            s = BR.lattice_precondition(fw, dmax, dmean)
            np.testing.assert_array_equal(host(red2).sum(0), s.red)
            # finalize: S, Q spread over the same slots
            st = np.zeros((nslots, 2, F))
            for sl in (0, 1, 31, nslots - 1, nslots // 2 + 3):
                st[sl, 0] += rng.integers(-50, 50, F)
                st[sl, 1] += rng.integers(5000, 9000, F)
            mean, rstd = g.new((F,)), g.new((F,))
            H.call("dgcnn_bn_finalize_f32", g.put(st).data_ptr(), F, 100.0, BR.EPS, mean.data_ptr(), rstd.data_ptr())
            mu64, rs64 = BR.finalize64(st[:, 0].sum(0), st[:, 1].sum(0), 100.0)
            assert (np.abs(host(mean) - mu64) <= 2.0 ** -24 * np.abs(mu64) * 1.001).all()
            assert (np.abs(host(rstd) - rs64) <= 2.0 ** -24 * rs64 * 1.001).all()
            g.check()
    finally:
        H.set_stat_slots(old)


@pytest.mark.parametrize("F", [1, 3, 4, 5, 1024])
def test_finalize_constant_cancelling_and_negative_variance_columns(dg, F):
    from dgcnn import _hip as H
    rng = np.random.default_rng(F)
    g = Guard()
    n = 4000
    Y = rng.normal(2, 3, (n, F)).astype(np.float32)
    Y[:, 0] = 1.25                                                               # constant: rstd = 1 / sqrt(eps)
    if F >= 3:
        Y[:, 1] = (1000 + 0.01 * rng.normal(size=n)).astype(np.float32)
    m, r = gpu_stats(H, g, Y)                                                    # asserts against float64 and the two-pass variance
    assert m[0] == np.float32(1.25) and r[0] == np.float32(1.0 / np.sqrt(np.float64(np.float32(BR.EPS))))
    # Q / n - mu^2 < 0 from rounding clamps to 0 (S, Q chosen directly)
    st = g.zeros((slots(H), 2, F), torch.float64)
    st[0, 0] = 3.0
    st[0, 1] = 2.9999999
    mean, rstd = g.new((F,)), g.new((F,))
    H.call("dgcnn_bn_finalize_f32", st.data_ptr(), F, 3.0, BR.EPS, mean.data_ptr(), rstd.data_ptr())
    assert (host(mean) == 1).all() and (host(rstd) == r[0]).all()
    g.check()


# -------------------------------------------------------------------------------------------------------------- det twin
DET = [(1000, 1, 3, 1), (70, 1, 2, 0), (500, 20, 64, 1), (2000, 1, 255, 1), (100, 1, 256, 0), (300, 1, 1024, 1), (5, 1, 700, 1), (500, 20, 64, 0)]


@pytest.mark.parametrize("kind", ["lattice", "random"])
@pytest.mark.parametrize("R,k,F,relu", DET)
def test_deterministic_reduce(dg, R, k, F, relu, kind):
    """dgcnn_bn_bwd_reduce_det_f32 (the default path of the class-dimension layer) accumulates in float64: only the fp32 roundings
    inside a term remain -- red0 within 4 2^-24 sum |dz|, red1 within 5 2^-24 sum |dz xh|, no factor n_terms; in the k = 1 form
    dz = dout exactly and red0 equals the float64 sum to n_terms 2^-53 sum |dz|.  Slot 0 only; (5, 1, 700): fewer rows than
    row ranges."""
    from dgcnn import _hip as H
    rng = np.random.default_rng(R + k + F + (kind == "lattice"))
    g = Guard()
    exact = kind == "lattice"
    if exact:
        k = BR.nearest_pow2(k)
        mu, rs, be = BR.lattice_params(rng, F)
        y = BR.lattice_dense(rng, R, k, F, relu)
        dmax, dmean = BR.lattice_grads(rng, R, k, F, with_mean=k > 1)
    else:
        y = random_rows(rng, R, k, F, relu)
        mu, rs = gpu_stats(H, g, y.reshape(R * k, F))
        be = rng.normal(0, 0.3, F).astype(np.float32)
        dmax, dmean = random_grads(rng, R, F, with_mean=k > 1)
    par = tuple(g.put(a).data_ptr() for a in (mu, rs, be))
    src = Dense(g, y)
    fw = BR.Fwd(y, mu, rs, be, relu)
    s = BR.lattice_precondition(fw, dmax, dmean) if exact else BR.Sums(BR.dz64(fw, dmax, dmean), fw.xh)
    nb = H.load().dgcnn_det_workspace_bytes(F)
    ws = g.new((nb // 4,))
    red = g.zeros((slots(H), 2, F), torch.float64)
    dm, dn = g.put(dmax), (g.put(dmean) if dmean is not None else None)
    mxd, cnd = (g.put(fw.mx), g.put(fw.ties)) if dmean is not None else (None, None)
    args = (*src.head(), *par, relu, dm.data_ptr(), F, p(dn), F if dn is not None else 0, p(mxd), F if mxd is not None else 0, p(cnd), red.data_ptr())
    H.call("dgcnn_bn_bwd_reduce_det_f32", *args, ws.data_ptr(), nb)
    rh = host(red)
    assert not rh[1:].any(), "the deterministic reduce writes slot 0 only"
    got = rh[0]
    if exact:
        np.testing.assert_array_equal(got, s.red)
    else:
        if k == 1:
            assert (np.abs(got[0] - s.red0) <= s.n_terms * 2.0 ** -53 * s.abs0).all()
        note_ratio("bn_bwd_reduce_det red0", got[0] - s.red0, s.abs0, s.n_terms, 4)
        note_ratio("bn_bwd_reduce_det red1", got[1] - s.red1, s.abs1, s.n_terms, 5)
        red2 = g.zeros((slots(H), 2, F), torch.float64)                         # run to run: bit-identical
        H.call("dgcnn_bn_bwd_reduce_det_f32", *args[:-1], red2.data_ptr(), ws.data_ptr(), nb)
        np.testing.assert_array_equal(host(red2), rh)
    with pytest.raises(H.HipError):
        H.call("dgcnn_bn_bwd_reduce_det_f32", *args, ws.data_ptr(), nb - 1)      # one byte short: ENOSPC
    g.check()


# ------------------------------------------------------------------------------------------- fused first-layer backward
@pytest.mark.parametrize("C,F", [(1, 4), (3, 64), (4, 128), (3, 1024)])
def test_edge_apply_with_fused_weight_gradient(dg, C, F):
    """dgcnn_edge_bn_bwd_apply_wgrad_f32: dW0 += [x_i, x_j - x_i]^T dY against float64, on a non-zero prior, with a workspace that is
    exactly large enough and one byte short."""
    from dgcnn import _hip as H
    B, N, k = 2, 60, 5
    R = B * N
    rng = np.random.default_rng(C * 100 + F)
    for exact in (True, False):
        g = Guard()
        kk = BR.nearest_pow2(k) if exact else k
        V, U, idx, mu, rs, be, dmax, dmean = _edge_inputs(H, g, rng, B, N, kk, F, 1, exact)
        src = Edge(g, V, U, idx, B, N)
        fw = BR.Fwd(src.y, mu, rs, be, 1)
        s = BR.lattice_precondition(fw, dmax, dmean) if exact else BR.Sums(BR.dz64(fw, dmax, dmean), fw.xh)
        x = (rng.integers(-3, 4, (R, C)) if exact else rng.normal(size=(R, C))).astype(np.float32)
        par = tuple(g.put(a).data_ptr() for a in (mu, rs, be))
        prior = rng.integers(-5, 6, (2 * C, F)).astype(np.float32)
        red = g.zeros((slots(H), 2, F), torch.float64)
        red[0] = torch.from_numpy(s.red).cuda()
        xd = g.new((R, 4))
        xd[:, :C] = torch.from_numpy(x).cuda()
        dW = g.put(prior)
        dbeta = g.zeros((F,))
        grid = ((min(1024, max(1, -(-R * (F // 4) // 256))) + 7) // 8) * 8
        need = grid * 2 * C * F * 4
        ws = g.new((need // 4,))
        ops = [g.put(a) for a in (dmax, dmean, fw.mx, fw.packed)]
        args = (*src.head(), *par, ops[0].data_ptr(), F, ops[1].data_ptr(), F, ops[2].data_ptr(), F, ops[3].data_ptr(), red.data_ptr(),
                xd.data_ptr(), 4, C, dW.data_ptr(), dbeta.data_ptr(), 0.0, ws.data_ptr())
        with pytest.raises(H.HipError):
            H.call("dgcnn_edge_bn_bwd_apply_wgrad_f32", *args, need - 1)
        np.testing.assert_array_equal(host(dW), prior)
        H.call("dgcnn_edge_bn_bwd_apply_wgrad_f32", *args, need)
        eo, _ = BR.apply32(BR.dz32(fw, dmax, dmean), fw.xh, fw.rs, s.red, R * src.k)
        ref = BR.wgrad64(x, idx, B, N, eo)                        # float64 E^T dY of the fp32 dY the kernel forms
        eo64 = np.abs(eo.astype(np.float64))
        kidx = (np.arange(B)[:, None, None] * N + idx).reshape(R, src.k)
        scale = np.concatenate([np.einsum("rc,rmf->cf", np.abs(x.astype(np.float64)), eo64),
                                np.einsum("rmc,rmf->cf", np.abs(x[kidx].astype(np.float64) - x[:, None, :]), eo64)], 0)
        got = host(dW).astype(np.float64) - prior
        np.testing.assert_array_equal(host(dbeta), BR.dbeta32(s.red[0]))
        n_terms = R * src.k
        # (no extra allowance for the fp32 rounding of `prior + sum`: in a nearly dead column, where sum |term| is small against the
        # prior, that rounding is most of the measured ratio -- still inside the bound)
        note_ratio("edge_bwd_apply_wgrad dW0", got - ref, scale, n_terms, n_terms + 8, record=not exact)
        g.check()


# ---------------------------------------------------------------------------------------------------------- fused dropout
@pytest.mark.parametrize("keep", [1.0, 0.7])
@pytest.mark.parametrize("F", [4, 256, 1028])
def test_bn1_with_fused_dropout(dg, F, keep):
    """dgcnn_bn1_act_dropout_f32 / dgcnn_bn1_bwd_dropout_f32: the mask is that of dgcnn_dropout_dev_f32 on ones with the same device
    seed; forward bit-equal to mask z / keep, backward against the float64 reference with dz masked; dT in place."""
    from dgcnn import _hip as H
    R = 333
    rng = np.random.default_rng(F)
    g = Guard()
    y = random_rows(rng, R, 1, F, 1)
    mu, rs = gpu_stats(H, g, y.reshape(R, F))
    be = rng.normal(0, 0.3, F).astype(np.float32)
    par = tuple(g.put(a).data_ptr() for a in (mu, rs, be))
    seed = torch.tensor([0x1234567 + F], dtype=torch.int64, device="cuda")
    ones = torch.ones(R * F, device="cuda")
    m = g.new((R * F,))
    H.call("dgcnn_dropout_dev_f32", ones.data_ptr(), m.data_ptr(), R * F, keep, seed.data_ptr())
    mh = host(m).reshape(R, F)
    kept = mh != 0
    dscale = np.float32(1) / np.float32(keep)
    assert (mh[kept] == dscale).all() and (keep < 1 or kept.all()) and abs(kept.mean() - keep) <= 5 * np.sqrt(keep * (1 - keep) / kept.size)
    for relu in (1, 0):
        src = Dense(g, y)
        fw = BR.Fwd(y, mu, rs, be, relu)
        outw = g.new((R, F + 4))
        H.call("dgcnn_bn1_act_dropout_f32", src.Y.data_ptr(), R, F, *par, relu, keep, seed.data_ptr(), outw.data_ptr(), F + 4)
        oh = host(outw)
        assert (oh[:, F:] == SENT).all()
        np.testing.assert_array_equal(oh[:, :F], np.where(kept, fw.z[:, 0] * dscale, np.float32(0)))
        dout = rng.normal(size=(R, F)).astype(np.float32)
        dzk = np.where(kept, dout * dscale, np.float32(0))                       # the gradient behind the mask (one fp32 product)
        s = BR.Sums(BR.dz64(fw, dzk, None), fw.xh)
        red = g.zeros((slots(H), 2, F), torch.float64)
        dbeta = g.zeros((F,))
        dd = g.put(dout)
        H.call("dgcnn_bn1_bwd_dropout_f32", src.Y.data_ptr(), R, F, *par, relu, keep, seed.data_ptr(), dd.data_ptr(), F, red.data_ptr(),
               src.Y.data_ptr(), dbeta.data_ptr(), 0.0)                          # dT in place
        got = host(red)[0]
        note_ratio("bn1_bwd_dropout sums", got - s.red, s.scale, s.n_terms, s.n_terms + 8)
        eo, _ = BR.apply32(BR.dz32(fw, dzk, None), fw.xh, fw.rs, got, R)         # the replay from the sums the call itself formed
        np.testing.assert_array_equal(host(src.Y).reshape(R, 1, F), eo)
        np.testing.assert_array_equal(host(dbeta), BR.dbeta32(got[0]))
    g.check()


# --------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_stay_refusals(dg):
    from dgcnn import _hip as H
    g = Guard()
    B, N, F = 1, 300, 8
    R = B * N
    buf = g.zeros((R, 2 * F))
    idx = g.zeros((R * 256,), torch.int32)
    v = g.zeros((F,))
    out = g.zeros((R, 2 * F))
    cnt = g.zeros((R, F))
    red = g.zeros((slots(H), 2, F), torch.float64)

    def edge_fwd(k, F_):
        H.call("dgcnn_edge_bn_act_kreduce_f32", buf[:, F:].data_ptr(), 2 * F, buf.data_ptr(), 2 * F, idx.data_ptr(), B, N, k, F_, v.data_ptr(),
               v.data_ptr(), v.data_ptr(), 1, out.data_ptr(), 2 * F, out[:, F:].data_ptr(), 2 * F, cnt.data_ptr())

    def edge_red(k, F_):
        H.call("dgcnn_edge_bn_bwd_reduce_f32", buf[:, F:].data_ptr(), 2 * F, buf.data_ptr(), 2 * F, idx.data_ptr(), B, N, k, F_, v.data_ptr(),
               v.data_ptr(), v.data_ptr(), 1, out.data_ptr(), 2 * F, out[:, F:].data_ptr(), 2 * F, 0, 0, 0, red.data_ptr())

    for fn in (edge_fwd, edge_red):
        with pytest.raises(H.HipError):
            fn(256, F)                                                           # k >= 256: the packed count has no room
        with pytest.raises(H.HipError):
            fn(4, 6)                                                             # F % 4 != 0
    edge_fwd(255, F)                                                             # the largest k passes
    with pytest.raises(ValueError):                                              # mx_in without cnt_in
        H.call("dgcnn_bn_bwd_reduce_f32", buf.data_ptr(), R, 1, F, v.data_ptr(), v.data_ptr(), v.data_ptr(), 1, out.data_ptr(), 2 * F,
               out[:, F:].data_ptr(), 2 * F, out.data_ptr(), 2 * F, 0, red.data_ptr())
    with pytest.raises(ValueError):                                              # F > 8192
        H.call("dgcnn_bn_bwd_reduce_f32", buf.data_ptr(), 1, 1, 8196, v.data_ptr(), v.data_ptr(), v.data_ptr(), 1, out.data_ptr(), 8196,
               0, 0, 0, 0, 0, red.data_ptr())
    g.check()

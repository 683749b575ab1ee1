"""k-NN between two point sets (csrc/knn_cross.hip: knn_cross_kernel<KC, vector | scalar, 16- | 64-channel slab, DenseClouds |
PackedClouds> behind dgcnn_knn_cross_f32, dgcnn/_engine.py:knn_cross, dgcnn/ops.py:k_nn(queries=, return_dist=)) against
tests/knn_cross_reference.py (the oracle's own distances, a stable sort): EVERY row, bit for bit, no tolerance; dist is compared as
uint32.  Packed towers are compared cloud by cloud with p_off[b] added.  Before any comparison the host asserts that every index
lies inside the row's own candidate cloud.  idx, dist and the workspace of the raw calls are gpu_helpers.Guard buffers, checked
after each call.

What the shapes cover (64 query rows per block, 64-candidate tiles, slabs of 16 channels for C <= 16 and of 64 above):
  C   1 3 4 5 16 17 63 64 65 128 129 192 260 1024     both slab widths and their edges, both norm kernels, C % 4 != 0
  M   1 63 64 65 129          N   1 63 64 65 127 128 129 200          M > N: 129 x 63, 65 x 1;  M < N: 1 x 200, 63 x 129
  k   1 8 9 20 21 40 41 64, k = N at N = 1 and N = 64                 B   1 3
  loaders: contiguous, ld + 4, ld + 1 views cut out of buffers filled with 777, chosen independently for q and p: the float4 loader
  runs only when BOTH are float4-loadable and C % 4 == 0.

WHY THE NON-FINITE RUNS ARE SAFE.  These tests call the k-NN entries only, which write idx, dist and their own workspace; nothing
gathers through an index before the host has asserted that it lies inside the cloud.  No trip count or store address of the new
kernel depends on a value being finite (read from the code, csrc/knn_cross.hip and csrc/knn_scan.h):
  sqnorm_kernel / sqnorm_wide_kernel   loop over C and the block's rows; a thread stores s to its own row's slot.
  knn_cross_kernel   M and N come from the cloud maps; a packed block leaves by row0 >= M; the step loop runs cdiv(N, 64) *
                     cdiv(C, SL) times; CrossSlabStage loads from query rows clamped to [0, M), candidate rows clamped to [0, N) and
                     channel quads clamped to [0, C), and stores to LDS slots that are functions of the thread id; a distance only
                     sets bits of an 8-bit mask (d < thr is false for NaN and +inf), the drain pops one bit per trip and indexes the
                     parked distances by the bit's number; merge_lists walks KC entries; merge_lists_write_dist stores to
                     idx / dist + (query row) k + t, t < k, for rows below M only; fill_short_list runs v < N and c < k and stores
                     to out[c]; what is written to idx is a list entry below N or the fill's v < N, plus the candidate cloud's
                     first row.

The few_finite family has no 65-row form at k = 9 or 20 (its builder needs free rows past 63 and 64), and hist_trap none at 65 rows
and k = 20: there the 65-row set is the first 65 rows of the family's 129-row cloud (rows_of)."""
import numpy as np
import pytest
import torch

from gpu_helpers import dev, host, Guard
from launch_trace import launches, assert_launched
import knn_cross_reference as R
import knn_nonfinite as NF

pytestmark = pytest.mark.gpu

_REF = {}

C_AXIS = (1, 3, 4, 5, 16, 17, 63, 64, 65, 128, 129, 192, 260, 1024)
M_AXIS = (1, 63, 64, 65, 129)
N_AXIS = (1, 63, 64, 65, 127, 128, 129, 200)
K_AXIS = (1, 8, 9, 20, 21, 40, 41, 64)
LOADERS = ("contiguous", "ld+4", "ld+1")
# (M, N, k): every M, every N, every k, M > N and M < N, k = N at N = 1 and N = 64; five of them per C, cycling
MNK = ((129, 63, 8), (65, 1, 1), (1, 200, 20), (63, 129, 40), (64, 64, 64), (1, 1, 1), (65, 127, 9), (129, 128, 21), (63, 65, 41),
       (64, 200, 64), (129, 129, 20), (65, 63, 40), (1, 64, 8), (63, 127, 1), (64, 128, 9), (129, 200, 41))
# (q's loader, p's loader): all nine; any five in a row hold a pair with both float4-loadable and a mixed one
PAIRS = (("contiguous", "contiguous"), ("contiguous", "ld+1"), ("ld+4", "ld+4"), ("ld+1", "contiguous"), ("ld+4", "ld+1"),
         ("contiguous", "ld+4"), ("ld+1", "ld+4"), ("ld+1", "ld+1"), ("ld+4", "contiguous"))


def _dense_cases():
    out = []
    for ci, C in enumerate(C_AXIS):
        for s in range(5):
            i = len(out)
            M, N, k = MNK[(5 * ci + s) % len(MNK)]
            out.append((1 if i % 2 else 3, M, N, C, k) + PAIRS[i % len(PAIRS)])
    out.append((3, 129, 129, 192, 20, "contiguous", "contiguous"))     # odd tile count x odd slab count, more than one cloud
    out.append((1, 129, 200, 1024, 64, "ld+1", "ld+4"))                # sixteen slabs, the longest lists, the scalar loader
    out.append((3, 129, 200, 3, 64, "contiguous", "contiguous"))       # raw coordinates, the longest lists, the 16-channel slab
    return out


DENSE = _dense_cases()
assert len(DENSE) <= 80
for axis, col in ((C_AXIS, 3), (M_AXIS, 1), (N_AXIS, 2), (K_AXIS, 4), ((1, 3), 0), (LOADERS, 5), (LOADERS, 6)):
    assert {c[col] for c in DENSE} == set(axis), (col, {c[col] for c in DENSE} ^ set(axis))
assert {(129, 63), (65, 1), (1, 200), (63, 129)} <= {(c[1], c[2]) for c in DENSE}
assert {(1, 1), (64, 64)} <= {(c[2], c[4]) for c in DENSE}             # k = N
assert set(PAIRS) == {(c[5], c[6]) for c in DENSE}                     # both mixed pairs among them
F4 = ("contiguous", "ld+4")
for C in C_AXIS:
    mine = [c for c in DENSE if c[3] == C]
    assert any(c[5] in F4 and c[6] in F4 for c in mine) and any((c[5] in F4) != (c[6] in F4) for c in mine), C


def normal(tag, *shape):
    key = ("normal", tag) + shape
    if key not in _REF:
        x = np.random.default_rng([len(tag)] + [ord(ch) for ch in tag] + list(shape)).standard_normal(shape).astype(np.float32)
        x.setflags(write=False)
        _REF[key] = x
    return _REF[key]


def reference(q, p, k, key):
    """(idx (B, M, k), dist (B, M, k)) of q (B, M, C) against p (B, N, C); computed once per key"""
    key = ("ref", key, k)
    if key not in _REF:
        r = R.cross_knn_batch(q, p, k)
        for a in r:
            a.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def view(x2d, loader):
    """x2d (R, C) on the device as the loader's kind of view; the buffer around it holds 777."""
    rows, C = x2d.shape
    if loader == "contiguous":
        return dev(np.array(x2d, np.float32))
    buf = torch.full((rows, C + (4 if loader == "ld+4" else 1)), 777.0, dtype=torch.float32, device="cuda")
    buf[:, :C] = dev(np.array(x2d, np.float32))
    return buf[:, :C]


def raw_cross(qd, pd, k, M, N, B=1, q_off=None, p_off=None, want_dist=True, expect="cross"):
    """dgcnn_knn_cross_f32 on device views qd (q_rows, C), pd (p_rows, C) with idx, dist and the workspace between guards.
    Dense: B clouds of M queries against N candidates.  Packed: q_off / p_off host offsets (M, N unused).  -> (idx, dist | None)
    The call is recorded (tests/launch_trace.py); expect: (kernel, leading template arguments) that must be among its launches,
    "cross" = knn_cross_kernel<KC, vector | scalar, slab, cloud map> of the shape and the views."""
    from dgcnn import _hip as H
    lib = H.load()
    g = Guard()
    q_rows, C = qd.shape
    p_rows = pd.shape[0]
    if q_off is None:
        nseg, max_m, min_n, max_n, qo, po = B, M, N, N, None, None
    else:
        nseg = len(q_off) - 1
        max_m = int(np.diff(q_off).max())
        min_n, max_n = int(np.diff(p_off).min()), int(np.diff(p_off).max())
        qo, po = g.put(np.asarray(q_off, np.int32)), g.put(np.asarray(p_off, np.int32))
    idx = g.new((q_rows, k), torch.int32, fill=777)
    dist = g.new((q_rows, k), torch.float32) if want_dist else None
    need = int(lib.dgcnn_knn_cross_workspace_bytes(q_rows, p_rows))
    ws = g.new((need,), torch.uint8, fill=77)
    with launches() as L:
        H.call("dgcnn_knn_cross_f32", qd.data_ptr(), H.ld2(qd), pd.data_ptr(), H.ld2(pd), C, k, nseg, H._p(qo), H._p(po), q_rows, p_rows,
               max_m, min_n, max_n, idx.data_ptr(), H._p(dist), ws.data_ptr(), need)
    if expect == "cross":                                     # the instance this shape and these views are for
        vec = C % 4 == 0 and all(H.ld2(t) % 4 == 0 and t.data_ptr() % 16 == 0 for t in (qd, pd))
        expect = ("knn_cross_kernel", [8 if k <= 8 else 20 if k <= 20 else 40 if k <= 40 else 64, "true" if vec else "false",
                                       16 if C <= 16 else 64, "DenseClouds" if q_off is None else "PackedClouds"])
    assert_launched(L, *expect)
    g.check()
    return host(idx), (host(dist) if want_dist else None)


def same(got, want, lo, n, what):
    """Every index of got inside [lo, lo + n) (asserted first, on the host), then every row's indices and distance bits equal."""
    gi, wi = np.asarray(got[0]).reshape(want[0].shape), want[0]
    out = ((gi < lo) | (gi >= lo + n)).any(-1)
    assert not out.any(), "%s: %d rows hold an index outside the candidate cloud; first %s: %s" % (
        what, int(out.sum()), tuple(np.argwhere(out)[0]), gi[tuple(np.argwhere(out)[0])])
    bad = (gi != wi + lo).any(-1)
    if got[1] is not None:
        bad |= (np.asarray(got[1]).reshape(want[1].shape).view(np.uint32) != want[1].view(np.uint32)).any(-1)
    if bad.any():
        first = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d rows differ from the reference; first row %s: %s vs %s%s" % (
            what, int(bad.sum()), bad.size, first, gi[first], wi[first] + lo,
            "" if got[1] is None else "; dist %s vs %s" % (np.asarray(got[1]).reshape(want[1].shape)[first], want[1][first])))


def dense_cross(q, p, k, lq="contiguous", lp="contiguous", want_dist=True):
    B, M, C = q.shape
    N = p.shape[1]
    return raw_cross(view(q.reshape(B * M, C), lq), view(p.reshape(B * N, C), lp), k, M, N, B=B, want_dist=want_dist)


# ------------------------------------------------------------------------------------------------------
# dense
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,M,N,C,k,lq,lp", DENSE, ids=["B%d-M%d-N%d-C%d-k%d-%s-%s" % c for c in DENSE])
def test_dense_covering_set(B, M, N, C, k, lq, lp):
    from dgcnn import _hip as H
    q, p = normal("q", B, M, C), normal("p", B, N, C)
    add = {"contiguous": 0, "ld+4": 4, "ld+1": 1}
    assert H.ld2(view(q.reshape(B * M, C), lq)) == C + add[lq] and H.ld2(view(p.reshape(B * N, C), lp)) == C + add[lp]
    got = dense_cross(q, p, k, lq, lp)
    want = reference(q, p, k, ("normal", B, M, N, C))
    same(got, want, 0, N, "dense %s %s/%s" % ((B, M, N, C, k), lq, lp))


def test_dist_null_gives_the_same_indices():
    for (B, M, N, C, k) in ((3, 65, 129, 3, 9), (1, 129, 65, 192, 20)):
        q, p = normal("q", B, M, C), normal("p", B, N, C)
        want = reference(q, p, k, ("normal", B, M, N, C))
        with_d = dense_cross(q, p, k)
        without = dense_cross(q, p, k, want_dist=False)
        assert without[1] is None
        same(with_d, want, 0, N, "with dist %s" % ((B, M, N, C, k),))
        same(without, want, 0, N, "dist = NULL %s" % ((B, M, N, C, k),))
        np.testing.assert_array_equal(with_d[0], without[0])


def test_the_python_entries_return_the_raw_call():
    """E.knn_cross and ops.k_nn(queries=..., return_dist=...): shapes, dtypes and the same bits"""
    import dgcnn
    from dgcnn import _engine as E
    B, M, N, C, k = 3, 65, 129, 3, 9
    q, p = normal("q", B, M, C), normal("p", B, N, C)
    want = reference(q, p, k, ("normal", B, M, N, C))
    qd, pd = dev(np.array(q)), dev(np.array(p))
    idx, dist = dgcnn.ops.k_nn(pd, k, queries=qd, return_dist=True)
    assert idx.shape == (B, M, k) and idx.dtype == torch.int32 and dist.shape == (B, M, k) and dist.dtype == torch.float32
    same((host(idx), host(dist)), want, 0, N, "ops.k_nn queries= return_dist=")
    only = dgcnn.ops.k_nn(pd, k, queries=qd)
    assert isinstance(only, torch.Tensor)
    same((host(only), None), want, 0, N, "ops.k_nn queries=")
    e_idx = E.knn_cross(qd.view(B * M, C), pd.view(B * N, C), B, M, N, k)
    same((host(e_idx), None), want, 0, N, "E.knn_cross")


# ------------------------------------------------------------------------------------------------------
# ties
# ------------------------------------------------------------------------------------------------------
def test_ties_break_to_the_lower_index():
    """Quarter-integer lattice coordinates at C = 3: exact distances, many equal.  Candidate rows 100-149 are copies of rows 0-49, and
    query rows 0-39 are exact copies of candidates 0-39: the copy's D (s_i + s_j - 2 p, each rounded) need not be exactly 0 on other
    data, so the random-data twin below repeats both duplications off the lattice."""
    M, N, C, k = 129, 200, 3, 9
    rng = np.random.default_rng(7)
    p = (rng.integers(-8, 9, (1, N, C)) * 0.25).astype(np.float32)
    p[0, 100:150] = p[0, 0:50]
    q = (rng.integers(-8, 9, (1, M, C)) * 0.25).astype(np.float32)
    q[0, :40] = p[0, :40]
    want = reference(q, p, k, "lattice")
    assert (want[1][0, :, 1:] == want[1][0, :, :-1]).any()
    assert (want[0][0, :40, 0] == np.arange(40)).all() and (want[0][0, :40, 1] == np.arange(100, 140)).all()   # the copy after the original
    for lq, lp in (("contiguous", "contiguous"), ("ld+1", "contiguous"), ("ld+4", "ld+1")):
        same(dense_cross(q, p, k, lq, lp), want, 0, N, "lattice %s/%s" % (lq, lp))


@pytest.mark.parametrize("C", [3, 5, 64, 192])
def test_copies_of_candidates_off_the_lattice(C):
    M, N, k = 65, 129, 8
    p = np.array(normal("p", 1, N, C)) * np.float32(37.3)
    p[0, 100:129] = p[0, 0:29]
    q = np.array(normal("q", 1, M, C))
    q[0, :50] = p[0, 10:60]
    want = reference(q, p, k, ("copies", C))
    hit = want[0][0, :50, 0] == np.arange(10, 60)
    assert hit.mean() > 0.9                                            # the copy is (nearly always) its own nearest candidate
    same(dense_cross(q, p, k), want, 0, N, "copies C=%d" % C)


# ------------------------------------------------------------------------------------------------------
# packed towers
# ------------------------------------------------------------------------------------------------------
def towers(Ms, Ns, C, k, tag="t"):
    """(q tower, q_off, p tower, p_off, [(idx, dist) of cloud b, idx cloud-local])"""
    key = ("towers", Ms, Ns, C, k, tag)
    if key not in _REF:
        qs = [normal("q%s%d" % (tag, b), m, C) for b, m in enumerate(Ms)]
        ps = [normal("p%s%d" % (tag, b), n, C) for b, n in enumerate(Ns)]
        qo = np.concatenate([[0], np.cumsum(Ms)]).astype(np.int64)
        po = np.concatenate([[0], np.cumsum(Ns)]).astype(np.int64)
        _REF[key] = (np.concatenate(qs, 0), qo, np.concatenate(ps, 0), po, [R.cross_knn(a, b, k) for a, b in zip(qs, ps)])
    return _REF[key]


def check_towers(got, qo, po, want, what):
    for b, w in enumerate(want):
        sl = slice(int(qo[b]), int(qo[b + 1]))
        same((got[0][sl], None if got[1] is None else got[1][sl]), w, int(po[b]), int(po[b + 1] - po[b]), "%s cloud=%d" % (what, b))


# M_b = 1; N_b = k; a cloud whose M_b passes every other's (its later blocks find the other clouds' rows exhausted and leave);
# M_b > N_b in one cloud and < in the next
PACKED = [((1, 130, 20, 63), (40, 9, 64, 129), 3, 9), ((1, 130, 20, 63), (40, 9, 64, 129), 192, 9),
          ((64, 1, 200), (20, 300, 65), 5, 20), ((64, 1, 200), (20, 300, 65), 64, 20), ((64, 1, 200), (21, 300, 65), 16, 21),
          ((7, 65, 1, 129, 30), (64, 1, 200, 63, 128), 4, 1), ((7, 65, 1, 129, 30), (64, 41, 200, 63, 128), 260, 41),
          ((129, 65, 70), (64, 200, 64), 17, 64)]


@pytest.mark.parametrize("Ms,Ns,C,k", PACKED, ids=["%s-%s-C%d-k%d" % ("/".join(map(str, a)), "/".join(map(str, b)), C, k)
                                                   for a, b, C, k in PACKED])
def test_packed_towers(Ms, Ns, C, k):
    qt, qo, pt, po, want = towers(Ms, Ns, C, k)
    assert min(Ms) == 1 or k == min(Ns)
    lq, lp = PAIRS[(C + k) % len(PAIRS)]
    got = raw_cross(view(qt, lq), view(pt, lp), k, 0, 0, q_off=qo, p_off=po)
    check_towers(got, qo, po, want, "packed %s %s C=%d k=%d %s/%s" % (Ms, Ns, C, k, lq, lp))


def test_packed_through_ops():
    import dgcnn
    Ms, Ns, C, k = (1, 130, 20, 63), (40, 9, 64, 129), 3, 9
    qt, qo, pt, po, want = towers(Ms, Ns, C, k)
    idx, dist = dgcnn.ops.k_nn(dev(np.array(pt)), k, offsets=po, queries=dev(np.array(qt))[None], query_offsets=qo, return_dist=True)
    assert idx.shape == (1, sum(Ms), k) and dist.shape == idx.shape
    check_towers((host(idx)[0], host(dist)[0]), qo, po, want, "ops.k_nn packed")


# ------------------------------------------------------------------------------------------------------
# the same buffer on both sides: the self search
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 64, 192])
def test_the_same_buffer_is_the_self_search_dense(C):
    import dgcnn
    from dgcnn import _engine as E
    B, N, k = 2, 200, 20
    xd = dev(np.array(normal("x", B, N, C)))
    x2 = xd.view(B * N, C)
    self_idx = host(E.knn(x2, B, N, k))
    got = raw_cross(x2, x2, k, N, N, B=B)
    np.testing.assert_array_equal(got[0].reshape(B, N, k), self_idx)
    want = reference(normal("x", B, N, C), normal("x", B, N, C), k, ("self", B, N, C))
    same(got, want, 0, N, "q = p, C=%d" % C)
    idx, dist = dgcnn.ops.k_nn(xd, k, return_dist=True)
    np.testing.assert_array_equal(host(idx), self_idx)
    np.testing.assert_array_equal(host(dist).view(np.uint32), want[1].view(np.uint32))
    np.testing.assert_array_equal(host(dgcnn.ops.k_nn(xd, k)), self_idx)


@pytest.mark.parametrize("C", [3, 64, 192])
def test_the_same_buffer_is_the_self_search_packed(C):
    import dgcnn
    from dgcnn import _engine as E
    sizes, k = (21, 200, 64, 130), 20
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rows = int(off[-1])
    xd = dev(np.array(normal("xt", rows, C)))
    self_idx = host(E.knn(xd, 1, rows, k, seg=E.Segments(off, rows))).reshape(rows, k)
    got = raw_cross(xd, xd, k, 0, 0, q_off=off, p_off=off)
    for b in range(len(sizes)):
        blk = got[0][off[b]:off[b + 1]]
        assert ((blk >= off[b]) & (blk < off[b + 1])).all()
    np.testing.assert_array_equal(got[0], self_idx)
    idx, dist = dgcnn.ops.k_nn(xd, k, offsets=off, return_dist=True)
    np.testing.assert_array_equal(host(idx)[0], self_idx)
    np.testing.assert_array_equal(host(dist)[0].view(np.uint32), got[1].view(np.uint32))


# ------------------------------------------------------------------------------------------------------
# non-finite input
# ------------------------------------------------------------------------------------------------------
def rows_of(family, rows, C, k):
    """[(label, cloud (rows, C))]: the family at `rows` rows, or the first `rows` rows of its 129-row cloud where its builder has no
    form of that size (the module docstring names the two cases)"""
    try:
        if NF._fits(family, rows, C, k):
            return NF.variants(family, rows, C, k)
    except AssertionError:
        pass
    assert rows == 65 and family in ("few_finite", "hist_trap"), (family, rows, k)
    return [(label + ", first 65 rows", np.ascontiguousarray(x[:rows])) for label, x in NF.variants(family, 129, C, k)]


NONFINITE = [(f, where, M, N, C, k) for f in NF.FAMILIES for where in ("p", "q", "both") for (M, N, C, k) in ((65, 129, 5, 9), (129, 65, 64, 20))]


@pytest.mark.parametrize("family,where,M,N,C,k", NONFINITE, ids=["%s-%s-M%d-N%d-C%d-k%d" % c for c in NONFINITE])
def test_non_finite_input(family, where, M, N, C, k):
    clean_q, clean_p = NF.base(M, C, seed=1), NF.base(N, C, seed=2)
    qs = rows_of(family, M, C, k) if where in ("q", "both") else [("clean", clean_q)]
    ps = rows_of(family, N, C, k) if where in ("p", "both") else [("clean", clean_p)]
    if where == "both":
        n = max(len(qs), len(ps))
        pairs = [(qs[i % len(qs)], ps[i % len(ps)]) for i in range(n)]
    else:
        pairs = [(a, b) for a in qs for b in ps]
    assert pairs
    for (lq_label, q), (lp_label, p) in pairs:
        what = "family=%s in %s (%s | %s) %s" % (family, where, lq_label, lp_label, (M, N, C, k))
        want = R.cross_knn(np.asarray(q), np.asarray(p), k)
        assert all(len(set(r)) == k for r in want[0].tolist()), what
        for lq, lp in (("contiguous", "contiguous"), ("ld+1", "ld+4")):
            got = dense_cross(np.asarray(q)[None], np.asarray(p)[None], k, lq, lp)
            same(got, (want[0][None], want[1][None]), 0, N, what + " %s/%s" % (lq, lp))
            assert all(len(set(r)) == k for r in got[0].tolist()), what              # k distinct candidates in every row
            np.testing.assert_array_equal(np.isposinf(got[1]), np.isposinf(want[1]))
            assert not np.isnan(got[1]).any(), what


def test_packed_towers_with_a_non_finite_cloud_in_the_middle():
    Ms, Ns, C, k = (30, 65, 129), (70, 129, 65), 5, 9
    for family in NF.FAMILIES:
        qs = [NF.base(Ms[0], C, seed=3), np.asarray(rows_of(family, Ms[1], C, k)[0][1]), NF.base(Ms[2], C, seed=4)]
        ps = [NF.base(Ns[0], C, seed=5), np.asarray(rows_of(family, Ns[1], C, k)[0][1]), NF.base(Ns[2], C, seed=6)]
        qo = np.concatenate([[0], np.cumsum(Ms)]).astype(np.int64)
        po = np.concatenate([[0], np.cumsum(Ns)]).astype(np.int64)
        want = [R.cross_knn(a, b, k) for a, b in zip(qs, ps)]
        got = raw_cross(dev(np.concatenate(qs, 0)), dev(np.concatenate(ps, 0)), k, 0, 0, q_off=qo, p_off=po)
        check_towers(got, qo, po, want, "packed, cloud 1 of family %s" % family)


# ------------------------------------------------------------------------------------------------------
# arguments, on the device: a refused call writes nothing
# ------------------------------------------------------------------------------------------------------
def test_a_refused_call_leaves_its_buffers_alone():
    from dgcnn import _hip as H
    lib = H.load()
    g = Guard()
    M, N, C, k = 65, 63, 5, 8
    q, p = g.put(np.array(normal("q", M, C))), g.put(np.array(normal("p", N, C)))
    idx = g.new((M, k), torch.int32, fill=777)
    dist = g.new((M, k), torch.float32)
    need = int(lib.dgcnn_knn_cross_workspace_bytes(M, N))
    ws = g.new((need,), torch.uint8, fill=77)
    for kk, short, code in ((65, 0, -4), (64, 0, -1), (8, 1, -1)):      # k > 64; k > N; a workspace one byte short
        rc = lib.dgcnn_knn_cross_f32(q.data_ptr(), C, p.data_ptr(), C, C, kk, 1, None, None, M, N, M, N, N, idx.data_ptr(), dist.data_ptr(),
                                     ws.data_ptr(), need - short, H._stream())
        assert rc == code, (kk, short, rc)
        g.check()
        assert (host(idx) == 777).all() and (host(dist) == 777.0).all() and (host(ws) == 77).all(), "a refused call wrote to its buffers"
    rc = lib.dgcnn_knn_cross_f32(q.data_ptr(), C, p.data_ptr(), C, C, k, 1, None, None, M, N, M, N, N, idx.data_ptr(), dist.data_ptr(),
                                 ws.data_ptr(), need, H._stream())
    assert rc == 0
    g.check()
    assert (host(idx) >= 0).all() and (host(idx) < N).all()


def test_two_calls_are_bit_identical():
    q, p = normal("q", 3, 129, 260), normal("p", 3, 200, 260)
    a, b = dense_cross(q, p, 20), dense_cross(q, p, 20)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32))

"""Packed towers: clouds of different sizes concatenated row-wise and described by offsets (dgcnn.ops.* offsets=, the C entry point
dgcnn_knn_seg_f32).  Every row searches its own cloud only and the indices come back as tower rows: per cloud, bit for bit the dense
k_nn of that cloud alone (oracle/knn_oracle.c).  The EdgeConv stacks run on the packed graphs with every other pass row-wise."""
import numpy as np
import pytest
import torch

from oracle import dgcnn_oracle as O
from gpu_helpers import capture_layers, dev, host, set_vars

pytestmark = pytest.mark.gpu


@pytest.fixture()
def dg():
    import dgcnn
    dgcnn.reset()
    return dgcnn


def pack(clouds):
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    return np.concatenate(clouds, 0), off


def check_per_cloud(idx, clouds, off, k):
    """idx (1,R,k) of the tower: every index in the row's own cloud, and per cloud the oracle's k_nn of that cloud alone."""
    idx = idx.reshape(-1, k)
    for b, cl in enumerate(clouds):
        part = idx[off[b]:off[b + 1]]
        assert part.min() >= off[b] and part.max() < off[b + 1], "cloud %d: an index outside the cloud" % b
        np.testing.assert_array_equal(part - off[b], O.k_nn(cl[None], k)[0], err_msg="cloud %d" % b)


def make_clouds(rng, sizes, C, lattice=1):
    out = []
    for i, n in enumerate(sizes):
        if i == lattice:
            out.append(rng.integers(0, 6, (n, C)).astype(np.float32))          # integer coordinates: exact ties, duplicates
        else:
            out.append(rng.normal(size=(n, C)).astype(np.float32) + np.float32(3 * i))
    return out


@pytest.mark.parametrize("k", [1, 8, 20, 40])
@pytest.mark.parametrize("C", [3, 4, 16, 64, 128])
def test_packed_knn_matches_the_oracle_per_cloud(dg, C, k):
    """Unaligned cloud sizes, one cloud of exactly k points, one of integer coordinates; and (C <= 4) a pack whose smallest cloud
    admits the histogram bound of the raw-coordinate scan."""
    rng = np.random.default_rng(100 * C + k)
    packs = [[130, 257, 1000, k, 513]]
    if C <= 4:
        packs.append([330, 517, 1000, 400])
    for sizes in packs:
        clouds = make_clouds(rng, sizes, C)
        x, off = pack(clouds)
        idx = host(dg.ops.k_nn(dev(x), k, offsets=off))
        assert idx.shape == (1, len(x), k) and idx.dtype == np.int32
        check_per_cloud(idx, clouds, off, k)
        idx3 = host(dg.ops.k_nn(dev(x[None]), k, offsets=torch.from_numpy(off)))     # (1,R,C) in, offsets as a tensor
        np.testing.assert_array_equal(idx3, idx)


def test_packed_knn_single_cloud_equals_dense(dg):
    rng = np.random.default_rng(3)
    for C, k in ((3, 20), (64, 20), (32, 8)):
        x = rng.random((1, 777, C), dtype=np.float32)
        a = host(dg.ops.k_nn(dev(x), k, offsets=[0, 777]))
        np.testing.assert_array_equal(a, host(dg.ops.k_nn(dev(x), k)))


@pytest.mark.parametrize("append", [1, 0], ids=["append-scan", "lists"])
@pytest.mark.parametrize("C,k", [(64, 20), (32, 8), (16, 20), (64, 40)])
def test_seeded_packed_knn_equals_the_unseeded_search(dg, C, k, append):
    """Seeds from a packed graph of other features, with the append-form scan on and off: the unseeded result, bit for bit."""
    from dgcnn import _engine as E, _hip as H
    lib = H.load()
    rng = np.random.default_rng(C + k)
    clouds = [np.maximum(rng.normal(size=(n, C)), 0).astype(np.float32) for n in (300, 517, 1000, 256, 70)]
    x, off = pack(clouds)
    seg = E.Segments(off, len(x))
    other = host(E.knn(dev(rng.random((len(x), 3), dtype=np.float32)), 1, len(x), k, seg=seg))
    prev = lib.dgcnn_knn_append(append)
    try:
        xd = dev(x)
        plain = host(E.knn(xd, 1, len(x), k, seg=seg))
        check_per_cloud(plain, clouds, off, k)
        for name, sd in (("other features' graph", other), ("own graph", plain)):
            got = host(E.knn(xd, 1, len(x), k, seed=dev(sd), seg=seg))
            np.testing.assert_array_equal(got, plain, err_msg=name)
    finally:
        lib.dgcnn_knn_append(prev)


@pytest.mark.parametrize("C,k", [(64, 8), (64, 20), (32, 20)])
def test_seeds_in_a_neighbouring_cloud_give_no_bound(dg, C, k):
    """Cloud 1 holds every point of cloud 0 k times over.  Seeds of a cloud-0 row that name the k copies of that very row are at
    distance ~0, far nearer than the row's true k-th neighbour: counted as a bound, they would drop the true neighbours.  They lie in
    the neighbouring cloud, so the row must be searched without a bound -- the result stays the oracle's."""
    from dgcnn import _engine as E, _hip as H
    lib = H.load()
    rng = np.random.default_rng(7 * C + k)
    a = np.maximum(rng.normal(size=(130, C)), 0).astype(np.float32) + np.float32(0.25)
    clouds = [a, np.repeat(a, k, axis=0), rng.random((200, C), dtype=np.float32)]
    x, off = pack(clouds)
    R = len(x)
    seg = E.Segments(off, R)
    prev = lib.dgcnn_knn_append(1)
    try:
        xd = dev(x)
        plain = host(E.knn(xd, 1, R, k, seg=seg))
        check_per_cloud(plain, clouds, off, k)
        adv = plain.reshape(R, k).copy()
        adv[:130] = off[1] + np.arange(130)[:, None] * k + np.arange(k)[None, :]    # the k copies of row i in cloud 1
        adv[off[2]::2] = off[1] + np.arange(k)[None, :]                              # cloud 2 rows: seeds in cloud 1 too
        got = host(E.knn(xd, 1, R, k, seed=dev(adv.reshape(1, R, k)), seg=seg))
        np.testing.assert_array_equal(got, plain)
    finally:
        lib.dgcnn_knn_append(prev)


def test_packed_knn_with_a_cloud_past_8192_points(dg):
    """A cloud of 8200 points next to small ones, C = 64, k = 20: the list scan unseeded, the append-form scan for N >= 8192 seeded.
    ~512 sampled rows per cloud against the oracle's row routine, the seeded result equal to the unseeded one."""
    from dgcnn import _engine as E
    rng = np.random.default_rng(8200)
    C, k = 64, 20
    clouds = [np.maximum(rng.normal(size=(n, C)), 0).astype(np.float32) for n in (300, 8200, 700)]
    x, off = pack(clouds)
    R = len(x)
    seg = E.Segments(off, R)
    xd = dev(x)
    plain = host(E.knn(xd, 1, R, k, seg=seg)).reshape(R, k)
    for b, cl in enumerate(clouds):
        rows = np.sort(rng.choice(len(cl), min(512, len(cl)), replace=False)).astype(np.int32)
        np.testing.assert_array_equal(plain[off[b] + rows] - off[b], O.k_nn_rows(cl, k, rows), err_msg="cloud %d" % b)
    seed = host(E.knn(dev(rng.random((R, 4), dtype=np.float32)), 1, R, k, seg=seg))
    got = host(E.knn(xd, 1, R, k, seed=dev(seed), seg=seg)).reshape(R, k)
    np.testing.assert_array_equal(got, plain)


def test_packed_edges_are_the_dense_gather_of_tower_rows(dg):
    rng = np.random.default_rng(5)
    clouds = make_clouds(rng, [40, 97, 64], 3, lattice=-1)
    x, off = pack(clouds)
    e = host(dg.ops.edges(dev(x), 8, offsets=off))
    idx = host(dg.ops.k_nn(dev(x), 8, offsets=off))
    assert e.shape == (1, len(x), 8, 6)
    np.testing.assert_array_equal(e, O.edges(x[None], 8, idx=idx))


def _stack_params(rng, C, fl):
    P = {}
    cin = C
    for i, f in enumerate(fl):
        s = "EdgeConv%d/" % i
        P[s + "conv0/weights"] = rng.normal(0, 0.4, (2 * cin, f)).astype(np.float32)
        P[s + "conv0/BatchNorm/beta"] = rng.normal(0, 0.2, f).astype(np.float32)
        P[s + "conv1/weights"] = rng.normal(0, 0.2, (2 * f, 64)).astype(np.float32)
        P[s + "conv1/BatchNorm/beta"] = rng.normal(0, 0.2, 64).astype(np.float32)
        if i > 0 and f != fl[i - 1]:
            P[s + "shortcut/weights"] = rng.normal(0, 0.2, (64, f)).astype(np.float32)
            P[s + "shortcut/BatchNorm/beta"] = rng.normal(0, 0.2, f).astype(np.float32)
        cin = 64
    return P


def _run_stack(dg, pts, residual, kl, fl, P, offsets):
    c = dg.ctx()
    c.begin_step()
    c.recording = True
    for n, v in P.items():
        c.get_variable(n, v.shape)
    set_vars(dg, P)
    fn = dg.ops.repeat_residual_edge_conv if residual else dg.ops.repeat_edge_conv
    with capture_layers() as cap:
        tensors = fn(dev(pts), len(kl), kl, fl, True, offsets=offsets)
    return c, tensors, cap


@pytest.mark.parametrize("det", [True, False], ids=["deterministic", "atomic"])
@pytest.mark.parametrize("residual", [False, True], ids=["edgeconv", "residual"])
def test_packed_stack_against_the_float64_oracle(dg, residual, det):
    """repeat_(residual_)edge_conv on a packed tower of 4 clouds: each layer's packed graph is the oracle's k_nn of that layer's input
    per cloud, bit for bit; the outputs match the float64 oracle fed those graphs on the (1, R) tower (BatchNorm over all R rows) within
    1e-4, and the gradients of every variable within 2e-3 relative Frobenius.  The residual stack goes 32 -> 64 filters (the shortcut conv runs)."""
    from dgcnn import _engine as E
    E.DETERMINISTIC = det
    try:
        rng = np.random.default_rng(11 + residual)
        C = 4
        kl, fl = ([20, 10], [32, 64]) if residual else ([20, 10, 5], [64, 64, 128])
        clouds = [rng.random((n, C), dtype=np.float32) for n in (300, 517, 1000, 256)]
        pts, off = pack(clouds)
        R = len(pts)
        P = _stack_params(rng, C, fl)
        c, tensors, cap = _run_stack(dg, pts, residual, kl, fl, P, off)
        assert len(tensors) == 3 * len(kl)
        idx_list = []
        for i in range(len(kl)):
            xin, idx = cap.layers["EdgeConv%d" % i]
            assert idx.shape == (1, R, kl[i])
            check_per_cloud(idx, [xin[0, off[b]:off[b + 1]] for b in range(len(clouds))], off, kl[i])
            idx_list.append(idx)
        p64 = {n: v.astype(np.float64) for n, v in P.items()}
        ref, layers = O.repeat_edge_conv(pts[None].astype(np.float64), len(kl), kl, fl, p64, residual=residual, idx_list=idx_list)
        for j, (a, b) in enumerate(zip(tensors, ref)):
            assert tuple(a.shape) == b.shape == (1, R, 1, b.shape[-1])
            np.testing.assert_allclose(host(a), b, rtol=1e-4, atol=1e-4, err_msg="tensor %d" % j)
        if residual:
            return                                   # (the oracle's backward restates the plain stack; the residual one is checked forward)
        d = [rng.normal(size=r.shape) for r in ref]
        for t, g in zip(tensors, d):
            v, _, _ = E.as2d(t)
            c.grad(v).copy_(dev(g.reshape(R, -1).astype(np.float32)))
        c.backward()
        d_next = None
        for i in reversed(range(len(kl))):
            d_net = d[3 * i + 2] if d_next is None else d[3 * i + 2] + d_next
            dx, g = O.edge_conv_bwd(d[3 * i], d[3 * i + 1], d_net, layers[i]["ec"])
            d_next = dx[:, :, None, :]
            s = "EdgeConv%d/" % i
            for leaf, key in (("conv0/weights", "W0"), ("conv0/BatchNorm/beta", "beta0"), ("conv1/weights", "W1"),
                              ("conv1/BatchNorm/beta", "beta1")):
                got = host(c.var_grads[s + leaf]).astype(np.float64)
                fro = np.linalg.norm(got - g[key]) / max(np.linalg.norm(g[key]), 1e-9)
                assert fro <= 2e-3, (s + leaf, fro)
    finally:
        E.DETERMINISTIC = E.DETERMINISTIC_ENV_DEFAULT


def test_single_cloud_pack_equals_the_dense_stack(dg):
    """offsets=[0, N] runs the same stack as the dense B = 1 tower: identical graphs, outputs within 1e-6."""
    rng = np.random.default_rng(21)
    kl, fl = [20, 10], [64, 64]
    pts = rng.random((1, 700, 3), dtype=np.float32)
    P = _stack_params(rng, 3, fl)
    _, dense, cap_d = _run_stack(dg, pts, False, kl, fl, P, None)
    dense = [host(t) for t in dense]
    dg.reset()
    _, packed, cap_p = _run_stack(dg, pts, False, kl, fl, P, [0, 700])
    for i in range(len(kl)):
        np.testing.assert_array_equal(cap_p.layers["EdgeConv%d" % i][1], cap_d.layers["EdgeConv%d" % i][1])
    for a, b in zip(packed, dense):
        np.testing.assert_allclose(host(a), b, rtol=1e-6, atol=1e-6)


def test_packed_errors_before_any_launch(dg):
    x = dev(np.zeros((50, 3), np.float32))
    with pytest.raises(ValueError):
        dg.ops.k_nn(x, 21, offsets=[0, 20, 50])                # k above the smallest cloud
    with pytest.raises(ValueError):
        dg.ops.repeat_edge_conv(x, 2, [5, 25], 64, True, offsets=[0, 24, 50])
    with pytest.raises(ValueError):
        dg.ops.k_nn(x, 4, offsets=[0, 20, 49])                 # does not end at R

"""The per-cloud loss without a GPU: the LOSS_PER_CLOUD flag, the float64 statement of what it computes
(tests/loss_per_cloud_reference.py) against `-mbs 1` accumulation of the oracle, and the host checks of the new entry."""
import numpy as np
import pytest

from oracle import dgcnn_oracle as O
import loss_per_cloud_reference as LP
import seg_bn_bwd_reference as SB

TOWER_SIZES = [21, 700, 64, 333]


def offsets_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def flat(G, names):
    return np.concatenate([np.asarray(G[n], np.float64).reshape(-1) for n in names])


def fro(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def test_flag_default_and_cli(capsys):
    from dgcnn import DGCNN_FLAGS
    assert DGCNN_FLAGS().LOSS_PER_CLOUD is False
    for script in ("train", "inference"):
        f = DGCNN_FLAGS()
        assert f.parse_args([script, "--loss_per_cloud", "1"], run=False) == script
        assert f.LOSS_PER_CLOUD is True and f.BN_PER_CLOUD is False and f.BN_PER_CLOUD_TRAIN is False      # orthogonal to BatchNorm
        g = DGCNN_FLAGS()
        g.parse_args([script, "-lpc", "y", "-mbs", "8"], run=False)
        assert g.LOSS_PER_CLOUD is True and g.MINIBATCH_SIZE == 8
        h = DGCNN_FLAGS()
        h.parse_args([script], run=False)
        assert h.LOSS_PER_CLOUD is False
    f = DGCNN_FLAGS()
    f.parse_args(["train", "-pt", "1", "-bpct", "1", "-lpc", "1"], run=False)
    assert f.PACK_TOWERS is True and f.BN_PER_CLOUD_TRAIN is True and f.LOSS_PER_CLOUD is True
    with pytest.raises(SystemExit):
        DGCNN_FLAGS().parse_args(["iotest", "--loss_per_cloud", "1"], run=False)
    capsys.readouterr()


@pytest.fixture(scope="module")
def tower():
    """The four-cloud tower with row weights, and its gradients three ways, all float64 with the oracle's own graphs:
    mbs1   = the accumulators after four `-bs 4 -mbs 1` micro-steps (each cloud a (1, n_b, C) batch of its own, added up),
    seeded = every cloud's backward seeded with ITS rows of the tower-wide seed dlogits_r = (p_r - onehot_r) w_r / n_b,
    summed = tests/loss_per_cloud_reference.train_step_grads (what the GPU tests compare against),
    shared = tests/seg_bn_bwd_reference.train_step_grads: sum_b (n_b / R) grads(cloud b), the mean over the tower's rows."""
    import dgcnn
    rng = np.random.default_rng(17)
    flags = dgcnn.DGCNN_FLAGS(MODEL_NAME="dgcnn", EDGE_CONV_LAYERS=2, EDGE_CONV_FILTERS=[32, 64], KVALUE=20, NUM_CLASS=3, FC_LAYERS=2,
                              FC_FILTERS=[64, 32], TRAIN=True, NUM_CHANNEL=4)
    off = offsets_of(TOWER_SIZES)
    R = int(off[-1])
    pts = rng.random((R, 4))
    lab = rng.integers(0, 3, R).astype(np.int32)
    wgt = rng.random(R) + 0.5
    params = {n: np.asarray(v, np.float64) for n, v in O.init_params(flags, 4, seed=1).items()}
    for n in params:
        if n.endswith("beta"):
            params[n] = rng.normal(0, 0.2, params[n].shape)
    names = sorted(params)
    mbs1, step_loss, step_acc, logits, caches = {}, [], [], [], []
    for _, lo, hi in SB.clouds(off):
        g, l, a, _ = O.train_step_grads(pts[None, lo:hi], lab[None, lo:hi], flags, params, weight=wgt[None, lo:hi])
        for n in names:
            mbs1[n] = mbs1.get(n, 0.0) + g[n]
        step_loss.append(float(l))
        step_acc.append(float(a))
        z, cache = O.model_forward(pts[None, lo:hi], flags, params)
        logits.append(z[0])
        caches.append(cache)
    ref = LP.xent(np.concatenate(logits), lab, wgt, off)
    seeded = {}
    for (_, lo, hi), cache in zip(SB.clouds(off), caches):
        g = O.model_backward(ref["dlogits"][None, lo:hi], cache)
        for n in names:
            seeded[n] = seeded.get(n, 0.0) + g[n]
    summed, l_b, a_b = LP.train_step_grads(pts, lab, off, flags, params, None, wgt)
    graphs = [np.concatenate([c["layers"][i]["ec"]["idx"].astype(np.int64) + lo for (_, lo, _), c in zip(SB.clouds(off), caches)], 1)
              for i in range(2)]
    shared, shared_loss = SB.train_step_grads(pts, lab, off, flags, params, graphs, wgt)
    return dict(names=names, mbs1=mbs1, seeded=seeded, summed=summed, shared=shared, step_loss=step_loss, step_acc=step_acc,
                ref=ref, l_b=l_b, a_b=a_b, shared_loss=shared_loss, off=off)


def test_sum_over_clouds_is_the_accumulation_of_mbs1_steps(tower):
    t = tower
    a = flat(t["mbs1"], t["names"])
    assert np.linalg.norm(a) > 0
    assert fro(flat(t["seeded"], t["names"]), a) <= 1e-12          # the tower-wide seed, cloud by cloud
    assert fro(flat(t["summed"], t["names"]), a) <= 1e-12
    for n in t["names"]:
        assert fro(np.asarray(t["seeded"][n]), np.asarray(t["mbs1"][n])) <= 1e-10, n
    np.testing.assert_allclose(t["ref"]["loss"], t["step_loss"], rtol=1e-13)
    np.testing.assert_allclose(t["ref"]["acc"], t["step_acc"], rtol=0, atol=1e-7)        # (the oracle's accuracy is a float32 mean)
    np.testing.assert_allclose(t["l_b"], t["step_loss"], rtol=1e-13)


def test_the_tower_wide_mean_is_another_objective(tower):
    """sum_b (n_b / R) grads(cloud b) -- the mean over the tower's rows, what a packed tower computed so far -- differs from the
    -mbs 1 accumulation by more than 0.5 relative Frobenius on this tower, and so do the logged losses unless the clouds agree."""
    t = tower
    a = flat(t["mbs1"], t["names"])
    d = fro(flat(t["shared"], t["names"]), a)
    print("||sum_b (n_b / R) g_b - sum_b g_b|| / ||sum_b g_b|| = %.4f" % d)
    assert d > 0.5
    n = np.diff(t["off"])
    assert np.isclose(t["shared_loss"], float((np.asarray(t["step_loss"]) * n).sum() / n.sum()), rtol=1e-12)


def test_reference_counts_negative_labels_in_n_only():
    rng = np.random.default_rng(2)
    z = rng.normal(size=(10, 3))
    lab = rng.integers(0, 3, 10)
    lab[[1, 7]] = -1
    r = LP.xent(z, lab, None, [0, 4, 10])
    keep = lab >= 0
    full = LP.xent(z[keep], lab[keep], None, [0, 3, 8])
    np.testing.assert_allclose(r["loss"] * np.array([4, 6]), full["loss"] * np.array([3, 5]), rtol=1e-13)
    assert r["count"].tolist() == full["count"].tolist() and r["acc"].tolist() == (full["count"] / np.array([4.0, 6.0])).tolist()
    assert np.array_equal(r["dlogits"][1], r["softmax"][1] / 4.0)                          # no one-hot row, still / n_b


def test_entry_reuses_the_chunk_slots_and_refuses_before_any_launch():
    """dgcnn_seg_softmax_xent_workspace_bytes(rows, nseg) = the (chunks + nseg) partial slots of the two sums plus one pair of
    doubles per cloud; every host-checkable argument is DGCNN_EINVAL (-1).  The pointers are never dereferenced: every check runs
    on the host before a launch, so this needs no device."""
    from dgcnn import _hip as H
    lib = H.load()
    p = 4096                                                             # an aligned non-null address
    rows, nseg, ncls = 328, 6, 3
    need = lib.dgcnn_seg_softmax_xent_workspace_bytes(rows, nseg)
    assert need == ((rows + 63) // 64 + nseg) * 2 * 8 + nseg * 2 * 8
    assert lib.dgcnn_seg_softmax_xent_workspace_bytes(0, 1) == 0 and lib.dgcnn_seg_softmax_xent_workspace_bytes(64, 0) == 0

    def call(logits=p, labels=p, rows=rows, ncls=ncls, off=p, nseg=nseg, sm=p, dl=p, cs=p, sc=p, ws=p, nb=need):
        return lib.dgcnn_seg_softmax_xent_f32(logits, labels, None, rows, ncls, off, nseg, sm, dl, cs, sc, ws, nb, None)
    for kw in (dict(logits=None), dict(off=None), dict(rows=0), dict(rows=-5), dict(ncls=0), dict(nseg=0), dict(nseg=rows + 1),
               dict(rows=1 << 20, nseg=65536, nb=1 << 30), dict(labels=None), dict(labels=None, dl=None, sm=None), dict(cs=None),
               dict(sc=None), dict(ws=None), dict(ws=p + 4), dict(nb=need - 1), dict(nb=0)):
        assert call(**kw) == -1, kw
        assert b"dgcnn_seg_softmax_xent_f32" in lib.dgcnn_last_error()
    call(nb=need - 1)
    assert ("%d bytes" % need) in lib.dgcnn_last_error().decode()


def test_entry_rows_one_row_per_cloud_in_batch_order():
    """main_funcs._entry_rows: the per-cloud tensors of the towers, tower by tower, next to the point counts -> one
    (points, loss, accuracy) row per entry; a count that does not match the clouds is an error, not a shifted file."""
    import torch
    from dgcnn import main_funcs as M
    h = M.Handlers()
    per = [torch.tensor([[0.5, 0.25], [0.75, 1.0]]), torch.tensor([[1.5, 0.0]])]
    rows = M._entry_rows(h, per, [300, 16777217, 64], [7, 8, 9])
    assert [r.tolist() for r in rows] == [[300.0, 0.5, 0.25], [16777217.0, 0.75, 1.0], [64.0, 1.5, 0.0]]      # (float64: counts past 2^24 stay exact)
    with pytest.raises(RuntimeError, match="3 per-cloud results for 2 clouds"):
        M._entry_rows(h, per, [300, 64], [7, 8])

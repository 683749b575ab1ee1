"""The float64 packed reference (tests/packed_reference.py) pinned against the oracle: with equal-sized clouds a packed tower IS the
dense (B, N) tower, so logits and every gradient must equal O.model_forward / O.model_backward on it -- same operations, float64."""
import numpy as np
import pytest

from oracle import dgcnn_oracle as O
import packed_reference as PR


class Flags(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


@pytest.mark.parametrize("model", ["dgcnn", "residual-dgcnn"])
@pytest.mark.parametrize("fcl", [2, 0])
def test_equal_clouds_reproduce_the_dense_oracle(model, fcl):
    B, N, C, k = 3, 40, 4, 8
    flags = Flags(MODEL_NAME=model, EDGE_CONV_LAYERS=2, EDGE_CONV_FILTERS=[32, 64], KVALUE=k, NUM_CLASS=3, FC_LAYERS=fcl,
                  FC_FILTERS=[24, 12][:fcl] if fcl else [], TRAIN=True, NUM_CHANNEL=C)
    rng = np.random.default_rng(5 + fcl)
    pts = rng.random((B, N, C))
    lab = rng.integers(0, 3, (B, N))
    wgt = rng.random((B, N)) + 0.5
    params = {n: v.astype(np.float64) for n, v in O.init_params(flags, C, seed=2).items()}
    for n in params:
        if n.endswith("beta"):
            params[n] = rng.normal(0, 0.2, params[n].shape)
    logits_d, cache_d = O.model_forward(pts, flags, params)
    loss_d, sm_d, acc_d, dl_d = O.softmax_xent(logits_d, lab, wgt)
    G_d = O.model_backward(dl_d, cache_d)
    graphs_d = [rec["ec"]["idx"] for rec in cache_d["layers"]]

    off = [0, N, 2 * N, 3 * N]
    graphs = [PR.tower_graphs(g) for g in graphs_d]
    logits_p, _ = PR.model_forward(pts.reshape(B * N, C), off, flags, params, graphs)
    assert logits_p.shape == (1, B * N, 3)
    assert np.abs(logits_p.reshape(B, N, 3) - logits_d).max() <= 1e-12
    G_p, loss_p, acc_p, sm_p = PR.train_step_grads(pts.reshape(1, B * N, C), lab.reshape(-1), off, flags, params, graphs,
                                                   weight=wgt.reshape(-1))
    assert abs(loss_p - loss_d) <= 1e-12 and acc_p == acc_d
    assert np.abs(sm_p.reshape(B, N, 3) - sm_d).max() <= 1e-12
    assert set(G_p) == set(G_d) == set(params)
    for n in G_d:
        assert np.abs(G_p[n] - G_d[n]).max() <= 1e-12, (n, float(np.abs(G_p[n] - G_d[n]).max()))


@pytest.mark.parametrize("model", ["dgcnn", "residual-dgcnn"])
def test_equal_clouds_reproduce_the_dense_oracle_in_bf16_mode(model):
    """flags.EDGE_MLP_DTYPE reaches the EdgeConv stack of the packed reference: at equal cloud sizes it equals O.model_forward /
    O.model_backward in bf16 mode (same operations, same operand rounding, float64) -- and differs from the fp32-operand twin by
    what the rounding costs, so a reference that dropped the flag would not pass."""
    B, N, C, k = 3, 40, 4, 8
    kw = dict(MODEL_NAME=model, EDGE_CONV_LAYERS=2, EDGE_CONV_FILTERS=[32, 64], KVALUE=k, NUM_CLASS=3, FC_LAYERS=2,
              FC_FILTERS=[24, 12], TRAIN=True, NUM_CHANNEL=C)
    flags, plain = Flags(EDGE_MLP_DTYPE="bf16", **kw), Flags(EDGE_MLP_DTYPE="f32", **kw)
    rng = np.random.default_rng(11)
    pts = rng.random((B, N, C))
    lab = rng.integers(0, 3, (B, N))
    params = {n: v.astype(np.float64) for n, v in O.init_params(flags, C, seed=2).items()}
    for n in params:
        if n.endswith("beta"):
            params[n] = rng.normal(0, 0.2, params[n].shape)
    logits_d, cache_d = O.model_forward(pts, flags, params)
    loss_d, sm_d, acc_d, dl_d = O.softmax_xent(logits_d, lab)
    G_d = O.model_backward(dl_d, cache_d)
    graphs_d = [rec["ec"]["idx"] for rec in cache_d["layers"]]
    off = [0, N, 2 * N, 3 * N]
    graphs = [PR.tower_graphs(g) for g in graphs_d]
    G_p, loss_p, acc_p, sm_p = PR.train_step_grads(pts.reshape(1, B * N, C), lab.reshape(-1), off, flags, params, graphs)
    assert abs(loss_p - loss_d) <= 1e-12 and acc_p == acc_d
    assert np.abs(sm_p.reshape(B, N, 3) - sm_d).max() <= 1e-12
    for n in G_d:
        assert np.abs(G_p[n] - G_d[n]).max() <= 1e-12, (n, float(np.abs(G_p[n] - G_d[n]).max()))
    logits_p, _ = PR.model_forward(pts.reshape(B * N, C), off, flags, params, graphs)
    logits_f, _ = PR.model_forward(pts.reshape(B * N, C), off, plain, params, graphs)
    assert np.abs(logits_p.reshape(B, N, 3) - logits_d).max() <= 1e-12
    assert np.abs(logits_p - logits_f).max() > 1e-4              # the mode IS different arithmetic


def test_unequal_clouds_pool_and_tile_per_cloud():
    """Clouds of 7, 30 and 12 points: the arg-max of every cloud lies inside that cloud, and a missing graph is refused."""
    C, k = 3, 4
    flags = Flags(MODEL_NAME="dgcnn", EDGE_CONV_LAYERS=1, EDGE_CONV_FILTERS=[8], KVALUE=k, NUM_CLASS=2, FC_LAYERS=0, FC_FILTERS=[],
                  TRAIN=False, NUM_CHANNEL=C)
    rng = np.random.default_rng(1)
    sizes = [7, 30, 12]
    off = np.concatenate([[0], np.cumsum(sizes)])
    clouds = [rng.random((n, C)) for n in sizes]
    pts = np.concatenate(clouds)
    graph = np.concatenate([O.k_nn(c[None].astype(np.float32), k)[0] + off[b] for b, c in enumerate(clouds)])[None]
    params = {n: v.astype(np.float64) for n, v in O.init_params(flags, C, seed=3).items()}
    logits, cache = PR.model_forward(pts, off, flags, params, [graph])
    assert logits.shape == (1, 49, 2)
    assert cache["garg"].shape == (3, 1024)
    assert (cache["garg"] >= 0).all() and (cache["garg"] < np.asarray(sizes)[:, None]).all()
    with pytest.raises(ValueError):
        PR.model_forward(pts, off, flags, params, None)

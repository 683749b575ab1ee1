"""The per-cloud float64 reference (tests/seg_bn_reference.py: the oracle on each cloud alone) against the tower-wide packed
reference (tests/packed_reference.py), on the CPU: one cloud -- the two are the same function; several unequal clouds -- they differ
far above the project's 1e-3 bar for logits, so the GPU tests of BN_PER_CLOUD can tell the two semantics apart at their shapes."""
import types

import numpy as np
import pytest

from oracle import dgcnn_oracle as O
import packed_reference as PR
import seg_bn_reference as SR

MODELS = [("dgcnn", 2), ("dgcnn", 0), ("residual-dgcnn", 2), ("residual-dgcnn-nofc", 2)]
SIZES = [21, 700, 64, 333]


def flags_of(model, fcl):
    return types.SimpleNamespace(MODEL_NAME=model, EDGE_CONV_LAYERS=2, EDGE_CONV_FILTERS=[32, 64], KVALUE=20, NUM_CLASS=3, FC_LAYERS=fcl,
                                 FC_FILTERS=[64, 32][:fcl] if fcl else 64, TRAIN=False, NUM_CHANNEL=4, EDGE_MLP_DTYPE="f32")


def params_of(flags, rng):
    params = O.init_params(flags, 4, seed=1, dtype=np.float64)
    for n in params:
        if n.endswith("beta"):
            params[n] = rng.normal(0, 0.2, params[n].shape)
    return params


def test_one_cloud_is_the_packed_reference():
    rng = np.random.default_rng(2)
    flags = flags_of("dgcnn", 2)
    params = params_of(flags, rng)
    pts = rng.random((150, 4))
    off = np.array([0, 150])
    graphs = SR.own_graphs(pts, off, flags, params)
    a = SR.model_forward(pts, off, flags, params, graphs)
    b, _ = PR.model_forward(pts, off, flags, params, graphs)
    assert a.shape == b.shape == (1, 150, 3)
    assert np.abs(a - b).max() <= 1e-12


@pytest.mark.parametrize("model,fcl", MODELS, ids=["%s-fc%d" % m for m in MODELS])
def test_unequal_clouds_tell_the_two_semantics_apart(model, fcl):
    rng = np.random.default_rng(17)
    flags = flags_of(model, fcl)
    params = params_of(flags, rng)
    off = np.concatenate([[0], np.cumsum(SIZES)])
    pts = rng.random((off[-1], 4))
    graphs = SR.own_graphs(pts, off, flags, params)
    for g, k in zip(graphs, (20, 20)):
        assert g.shape == (1, off[-1], k)
        for b in range(len(SIZES)):
            part = g[0, off[b]:off[b + 1]]
            assert part.min() >= off[b] and part.max() < off[b + 1]
    per_cloud = SR.model_forward(pts, off, flags, params, graphs)
    tower, _ = PR.model_forward(pts, off, flags, params, graphs)
    d = np.abs(per_cloud - tower)
    print("%s fc%d: per-cloud vs tower-wide statistics, max %.3g median %.3g" % (model, fcl, d.max(), np.median(d)))
    assert d.max() > 1e-2

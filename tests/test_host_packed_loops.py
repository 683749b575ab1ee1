"""Host side of the packed run loops (no GPU): PACK_TOWERS turns a micro-batch of clouds with different point counts into one
packed tower (concatenated data / label / weight plus offsets); without the flag such a micro-batch is refused as before."""
import numpy as np
import pytest

from dgcnn import DGCNN_FLAGS
from dgcnn import main_funcs as M


def _ragged(with_weight=True):
    rng = np.random.default_rng(0)
    sizes = (300, 512, 300, 700)
    data = [rng.random((n, 4), dtype=np.float32) for n in sizes]
    label = [rng.integers(0, 2, n).astype(np.int32) for n in sizes]
    weight = [rng.random(n, dtype=np.float32) for n in sizes] if with_weight else None
    return sizes, data, label, weight


def test_pack_towers_packs_a_mixed_micro_batch():
    sizes, data, label, weight = _ragged()
    f = DGCNN_FLAGS(BATCH_SIZE=4, MINIBATCH_SIZE=2, PACK_TOWERS=True, KVALUE=20)
    steps = list(M._micro_batches(f, M.Handlers(), data, label, weight))
    assert len(steps) == 2
    for s, (a, b) in zip(steps, ((0, 1), (2, 3))):
        dv, lv, wv, ov = s
        assert len(dv) == len(lv) == len(wv) == len(ov) == 1
        assert ov[0].tolist() == [0, sizes[a], sizes[a] + sizes[b]]
        np.testing.assert_array_equal(dv[0], np.concatenate([data[a], data[b]]))
        np.testing.assert_array_equal(lv[0], np.concatenate([label[a], label[b]]))
        np.testing.assert_array_equal(wv[0], np.concatenate([weight[a], weight[b]]))
        assert dv[0].shape == (sizes[a] + sizes[b], 4) and lv[0].shape == wv[0].shape == (sizes[a] + sizes[b],)


def test_pack_towers_keeps_a_stackable_chunk_dense_and_takes_2d_labels():
    sizes, data, label, _ = _ragged(with_weight=False)
    f = DGCNN_FLAGS(BATCH_SIZE=4, MINIBATCH_SIZE=2, PACK_TOWERS=True, KVALUE=20)
    steps = list(M._micro_batches(f, M.Handlers(), [data[0], data[2], data[1], data[3]],
                                  [label[0][None], label[2][None], label[1][None], label[3][None]], None))
    (dv0, lv0, wv0, ov0), (dv1, lv1, wv1, ov1) = steps
    assert ov0 == [None] and dv0[0].shape == (2, 300, 4) and wv0 is None          # equal N stacks: a dense tower
    assert ov1[0].tolist() == [0, 512, 1212] and dv1[0].shape == (1212, 4) and lv1[0].shape == (1212,)


def test_mixed_micro_batch_is_still_refused_without_the_flag():
    _, data, label, weight = _ragged()
    f = DGCNN_FLAGS(BATCH_SIZE=4, MINIBATCH_SIZE=2)
    assert f.PACK_TOWERS is False
    with pytest.raises(ValueError, match="minibatch_size 1"):
        list(M._micro_batches(f, M.Handlers(), data, label, weight))
    steps = list(M._micro_batches(DGCNN_FLAGS(BATCH_SIZE=4, MINIBATCH_SIZE=1), M.Handlers(), data, label, weight))
    assert all(len(s) == 3 for s in steps)                                        # the dense form of a step is unchanged


def test_a_cloud_smaller_than_k_is_refused_on_the_host():
    _, data, label, _ = _ragged(with_weight=False)
    data[1], label[1] = data[1][:12], label[1][:12]
    f = DGCNN_FLAGS(BATCH_SIZE=4, MINIBATCH_SIZE=2, PACK_TOWERS=True, KVALUE=20)
    with pytest.raises(ValueError, match="smallest cloud=12"):
        list(M._micro_batches(f, M.Handlers(), data, label, None))


def test_pack_towers_parses_from_the_cli(capsys):
    f = DGCNN_FLAGS()
    assert f.parse_args(["train", "--pack_towers", "1", "-mbs", "2", "-bs", "4"], run=False) == "train"
    assert f.PACK_TOWERS is True and f.MINIBATCH_SIZE == 2
    g = DGCNN_FLAGS()
    g.parse_args(["inference", "-pt", "0"], run=False)
    assert g.PACK_TOWERS is False
    capsys.readouterr()

"""Host side of per-cloud BatchNorm (no GPU): the workspace formula of the two-stage sums, the BN_PER_CLOUD flag, the Segments
that carries the mode, and the refusals that need no device."""
import pytest


def test_seg_stats_workspace_formula():
    """One double per (sum, column) and (chunk, cloud) piece: chunks + nseg slots bound the pieces of any tower; 0 when empty."""
    from dgcnn import _hip as H
    lib = H.load()
    for rows, nseg, F in ((328, 6, 3), (1118, 4, 64), (100000, 24, 1024), (64, 1, 4), (65, 65, 1)):
        assert lib.dgcnn_seg_stats_workspace_bytes(rows, nseg, F) == ((rows + 63) // 64 + nseg) * 2 * F * 8
    for rows, nseg, F in ((0, 1, 4), (10, 0, 4), (10, 1, 0), (-1, 1, 1)):
        assert lib.dgcnn_seg_stats_workspace_bytes(rows, nseg, F) == 0


def test_bn_per_cloud_flag_default_and_cli(capsys):
    from dgcnn import DGCNN_FLAGS
    assert DGCNN_FLAGS().BN_PER_CLOUD is False
    f = DGCNN_FLAGS()
    assert f.parse_args(["inference", "--pack_towers", "1", "--bn_per_cloud", "1", "-mbs", "4"], run=False) == "inference"
    assert f.BN_PER_CLOUD is True and f.PACK_TOWERS is True and f.MINIBATCH_SIZE == 4
    g = DGCNN_FLAGS()
    g.parse_args(["inference", "-bpc", "y"], run=False)
    assert g.BN_PER_CLOUD is True
    h = DGCNN_FLAGS()
    h.parse_args(["inference"], run=False)
    assert h.BN_PER_CLOUD is False
    t = DGCNN_FLAGS()
    t.parse_args(["train"], run=False)
    assert t.BN_PER_CLOUD is False                                  # present on every DGCNN_FLAGS, offered by `inference` only
    with pytest.raises(SystemExit):
        DGCNN_FLAGS().parse_args(["train", "--bn_per_cloud", "1"], run=False)
    capsys.readouterr()


def test_segments_carries_the_mode():
    import numpy as np
    from dgcnn import _engine as E, ops
    assert E.Segments([0, 5, 9]).bn_per_cloud is False
    assert E.Segments([0, 5, 9], 9, bn_per_cloud=True).bn_per_cloud is True
    pts = np.zeros((9, 3), np.float32)
    assert ops._segments(pts, [0, 5, 9], [2], bn_per_cloud=True).bn_per_cloud is True
    seg = E.Segments([0, 5, 9], bn_per_cloud=True)
    assert ops._segments(pts, seg, [2]) is seg and seg.bn_per_cloud is True         # a Segments keeps its own setting
    assert ops._segments(pts, E.Segments([0, 5, 9]), [2], bn_per_cloud=True).bn_per_cloud is False
    assert ops._segments(pts, None, [2]) is None
    with pytest.raises(ValueError, match="needs offsets"):
        ops._segments(pts, None, [2], bn_per_cloud=True)


def test_the_mode_refuses_training_on_the_host():
    import dgcnn
    with pytest.raises(NotImplementedError, match="no backward"):
        dgcnn.trainval(dgcnn.DGCNN_FLAGS(TRAIN=True, BN_PER_CLOUD=True)).initialize()

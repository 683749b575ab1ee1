"""Host side of the per-cloud BatchNorm backward (no GPU): the BN_PER_CLOUD_TRAIN flag, the Segments that carries the switch, the
refusals that stay, and the new entries' argument checks, which run before any launch (so they can be exercised without a device)."""
import ctypes

import pytest


def test_flag_default_and_cli(capsys):
    from dgcnn import DGCNN_FLAGS
    assert DGCNN_FLAGS().BN_PER_CLOUD_TRAIN is False
    f = DGCNN_FLAGS()
    assert f.parse_args(["train", "--pack_towers", "1", "--bn_per_cloud_train", "1", "-mbs", "4"], run=False) == "train"
    assert f.BN_PER_CLOUD_TRAIN is True and f.BN_PER_CLOUD is False and f.PACK_TOWERS is True and f.MINIBATCH_SIZE == 4
    g = DGCNN_FLAGS()
    g.parse_args(["train", "-bpct", "y"], run=False)
    assert g.BN_PER_CLOUD_TRAIN is True
    h = DGCNN_FLAGS()
    h.parse_args(["train"], run=False)
    assert h.BN_PER_CLOUD_TRAIN is False and h.BN_PER_CLOUD is False
    i = DGCNN_FLAGS()
    i.parse_args(["inference", "-bpc", "1"], run=False)
    assert i.BN_PER_CLOUD is True and i.BN_PER_CLOUD_TRAIN is False      # present on every DGCNN_FLAGS, offered by `train` only
    for argv in (["inference", "--bn_per_cloud_train", "1"], ["train", "--bn_per_cloud", "1"], ["train", "-bpc", "1"]):
        with pytest.raises(SystemExit):                                   # (the inference-only spelling is no abbreviation of the new one)
            DGCNN_FLAGS().parse_args(argv, run=False)
    capsys.readouterr()


def test_segments_carries_the_switch():
    import numpy as np
    from dgcnn import _engine as E, ops
    s = E.Segments([0, 5, 9])
    assert s.bn_per_cloud is False and s.bn_per_cloud_train is False
    assert E.Segments([0, 5, 9], bn_per_cloud=True).bn_per_cloud_train is False
    t = E.Segments([0, 5, 9], 9, bn_per_cloud_train=True)
    assert t.bn_per_cloud_train is True and t.bn_per_cloud is True          # the switch implies the mode
    pts = np.zeros((9, 3), np.float32)
    u = ops._segments(pts, [0, 5, 9], [2], bn_per_cloud_train=True)
    assert u.bn_per_cloud is True and u.bn_per_cloud_train is True
    assert ops._segments(pts, t, [2]) is t and t.bn_per_cloud_train is True  # a Segments keeps its own setting
    assert ops._segments(pts, E.Segments([0, 5, 9]), [2], bn_per_cloud_train=True).bn_per_cloud_train is False
    with pytest.raises(ValueError, match="needs offsets"):
        ops._segments(pts, None, [2], bn_per_cloud_train=True)


def test_per_cloud_raises_inside_a_recording_only_without_the_switch():
    from dgcnn import _engine as E
    c = E.ctx()
    c.recording = True
    try:
        with pytest.raises(NotImplementedError, match="per-cloud BatchNorm has no backward yet"):
            E.per_cloud(E.Segments([0, 5, 9], bn_per_cloud=True))
        assert E.per_cloud(E.Segments([0, 5, 9], bn_per_cloud_train=True)) is True
        assert E.per_cloud(E.Segments([0, 5, 9])) is False and E.per_cloud(None) is False
    finally:
        c.recording = False
    assert E.per_cloud(E.Segments([0, 5, 9], bn_per_cloud=True)) is True


def test_the_forward_only_flag_keeps_refusing_training():
    import dgcnn
    from dgcnn import _hip as H
    with pytest.raises(NotImplementedError, match="no backward"):
        dgcnn.trainval(dgcnn.DGCNN_FLAGS(TRAIN=True, BN_PER_CLOUD=True)).initialize()
    for kw in (dict(BN_PER_CLOUD_TRAIN=True), dict(BN_PER_CLOUD=True, BN_PER_CLOUD_TRAIN=True)):
        try:                                                              # past the refusal (then it needs a device)
            dgcnn.trainval(dgcnn.DGCNN_FLAGS(TRAIN=True, **kw)).initialize()
        except H.HipError:
            pass
    dgcnn.reset()


def test_reduce_entries_reuse_the_workspace_formula_and_refuse_before_any_launch():
    """The two reduce entries need dgcnn_seg_stats_workspace_bytes(rows, nseg, F) bytes: one byte less is DGCNN_ENOSPC with the
    needed count in the message.  Null pointers, relu outside {0, 1} and F % 4 != 0 are refused too.  The pointers are never
    dereferenced: every check runs on the host before a launch."""
    from dgcnn import _hip as H
    lib = H.load()
    p = 4096                                                             # a 16-byte aligned non-null address
    rows, nseg, F, k = 328, 6, 64, 20
    need = lib.dgcnn_seg_stats_workspace_bytes(rows, nseg, F)
    assert need == ((rows + 63) // 64 + nseg) * 2 * F * 8
    k1 = lambda ws, relu=1, T=p, F=F: lib.dgcnn_seg_bn_bwd_reduce_f32(T, F, rows, F, p, nseg, p, p, p, relu, p, F, None, 0, p, p, ws, None)
    pts = lambda ws, F=F, mx=p: lib.dgcnn_seg_edge_bn_bwd_reduce_points_f32(mx, F, p, F, p, p, F, p, F, p, rows, k, F, p, nseg, p, p, ws, None)
    for fn in (k1, pts):
        assert fn(need - 1) == -3
        assert ("%d bytes" % need) in lib.dgcnn_last_error().decode()
    assert k1(need, relu=2) == -1 and k1(need, T=None) == -1
    assert pts(need, mx=None) == -1 and pts(need, mx=p + 4) == -1            # null, misaligned
    assert pts(lib.dgcnn_seg_stats_workspace_bytes(rows, nseg, 6), F=6) == -4
    assert lib.dgcnn_seg_bn_bwd_finalize_f32(None, nseg, F, p, k, p, p, p, ctypes.c_float(1.0), None) == -1
    assert lib.dgcnn_seg_bn_bwd_apply_f32(p, F, rows, F, None, p, p, p, 1, p, F, None, 0, p, p, p, F, None) == -1
    assert lib.dgcnn_seg_bn_bwd_apply_f32(p, F, rows, F, p, p, p, p, 3, p, F, None, 0, p, p, p, F, None) == -1

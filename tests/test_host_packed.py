"""Packed towers on the host: the offsets of a tower (clouds of different sizes concatenated row-wise) are checked before any device
work, so a malformed tower fails with ValueError on a machine without a GPU, and a valid one reaches the device layer."""
import numpy as np
import pytest
import torch


def _pts(R, C=3):
    return torch.zeros(R, C)                       # a CPU tensor: anything past the host checks fails (no CPU fallback)


@pytest.mark.parametrize("offsets,k,what", [
    ([0, 20, 20, 50], 4, "strictly"),              # an empty cloud
    ([0, 30, 20, 50], 4, "strictly"),              # not increasing
    ([5, 20, 50], 4, "start at 0"),
    ([0, 20, 49], 4, "49"),                        # does not end at R
    ([0, 20, 50], 21, "smallest cloud=20"),        # k above the smallest cloud (tf.nn.top_k raises)
    ([0, 20, 50], 0, "smallest cloud"),
    ([50], 4, "nseg \\+ 1"),
    ([[0, 50]], 4, "nseg \\+ 1"),
    ([0.0, 50.0], 4, "integers"),
])
def test_offsets_are_validated_without_a_gpu(offsets, k, what):
    import dgcnn
    with pytest.raises(ValueError, match=what):
        dgcnn.ops.k_nn(_pts(50), k, offsets=offsets)
    with pytest.raises(ValueError, match=what):
        dgcnn.ops.edge_conv(_pts(50)[None], k, 64, True, offsets=offsets)


def test_stacks_check_every_layers_k_first():
    import dgcnn
    with pytest.raises(ValueError, match="k=25"):
        dgcnn.ops.repeat_edge_conv(_pts(50)[None], 2, [5, 25], 64, True, offsets=[0, 24, 50])
    with pytest.raises(ValueError, match="k=25"):
        dgcnn.ops.repeat_residual_edge_conv(_pts(50)[None], 2, [25, 5], 64, True, offsets=[0, 24, 50])


def test_packed_shapes_are_checked():
    import dgcnn
    with pytest.raises(ValueError, match="packed tower"):
        dgcnn.ops.k_nn(torch.zeros(2, 25, 3), 4, offsets=[0, 25, 50])      # two dense clouds are not one tower
    with pytest.raises(ValueError, match="packed tower"):
        dgcnn.ops.edges(torch.zeros(1, 50, 2, 3), 4, offsets=[0, 25, 50])


def test_valid_offsets_pass_the_host_checks():
    """A valid tower gets past the checks: the call then fails at the device boundary (CPU tensor), not with ValueError."""
    import dgcnn
    from dgcnn import _engine as E, _hip as H
    seg = E.Segments(np.array([0, 7, 50, 113]), 113)
    assert (seg.nseg, seg.rows, seg.min_n, seg.max_n) == (3, 113, 7, 63)
    seg.check_k(7)
    with pytest.raises(ValueError):
        seg.check_k(8)
    if torch.cuda.is_available():
        pytest.skip("GPU present: the device path is covered by test_gpu_packed.py")
    with pytest.raises(H.HipError):
        dgcnn.ops.k_nn(_pts(50), 4, offsets=torch.tensor([0, 20, 50]))


def test_packed_workspace_query_without_a_gpu():
    """dgcnn_knn_seg_workspace_bytes: the s_i and bound regions of the tower's rows, plus the append-form scan's buffers where that
    form applies (16 < C <= 64), sized by the largest cloud; zero for an empty tower."""
    from dgcnn import _hip as H
    lib = H.load()
    rows = 4000
    base = 2 * ((rows * 4 + 255) // 256 * 256)
    assert lib.dgcnn_knn_seg_workspace_bytes(rows, 1000, 3, 20) == base
    small = lib.dgcnn_knn_seg_workspace_bytes(rows, 1000, 64, 20)
    big = lib.dgcnn_knn_seg_workspace_bytes(rows, 9000, 64, 20)
    assert base < small < big                      # the N >= 8192 form keeps more entries per row
    assert lib.dgcnn_knn_seg_workspace_bytes(0, 1000, 64, 20) == 0

"""The per-cloud mix of cell grid and all-pairs scan on packed towers, on the host: the workspace query of dgcnn_knn_seg_mix_f32, the
threshold's setter (dgcnn_knn_seg_mix_min_n; csrc/knn.hip, csrc/knn_grid.hip) and the two classes Segments makes of a tower
(dgcnn/_engine.py).  None of this makes a GPU call."""
import numpy as np
import pytest
import torch

GMAX3 = 16 ** 3                 # cells of the largest grid (csrc/knn_grid.hip: GMAX = 16)
GRID_INFO = 64                  # sizeof(GridInfo)


@pytest.fixture()
def lib():
    from dgcnn import _hip as H
    return H.load()


def expected_bytes(rows, n_grid):
    sq = (rows * 4 + 255) // 256 * 256                          # s_i of every row, padded; the bounds take the same again
    return 2 * sq + rows * (16 + 4 + 4) + n_grid * ((GMAX3 + 1) * 4 + GRID_INFO) + 256


@pytest.mark.parametrize("rows,n_grid", [(2, 1), (300, 2), (114234, 5)])
def test_workspace_is_the_documented_sum(lib, rows, n_grid):
    assert lib.dgcnn_knn_seg_mix_workspace_bytes(rows, n_grid) == expected_bytes(rows, n_grid)


def test_workspace_grows_with_the_grid_clouds_only_and_is_zero_for_an_empty_tower(lib):
    """The query does not even take nseg: a tower of thousands of small clouds around two large ones pays two cell tables."""
    a, b = lib.dgcnn_knn_seg_mix_workspace_bytes(5000, 2), lib.dgcnn_knn_seg_mix_workspace_bytes(5000, 3)
    assert b - a == (GMAX3 + 1) * 4 + GRID_INFO
    rows, nseg = 3000 * 100 + 2 * 20000, 3002
    per_cloud, bounds = (GMAX3 + 1) * 4 + GRID_INFO, (rows * 4 + 255) // 256 * 256
    assert lib.dgcnn_knn_seg_grid_workspace_bytes(rows, nseg) - lib.dgcnn_knn_seg_mix_workspace_bytes(rows, 2) == 3000 * per_cloud - bounds
    for rows, n_grid in ((0, 3), (-1, 3), (0, 0)):
        assert lib.dgcnn_knn_seg_mix_workspace_bytes(rows, n_grid) == 0


def test_setter_returns_the_previous_value_and_a_negative_argument_only_queries(lib):
    start = lib.dgcnn_knn_seg_mix_min_n(-1)
    try:
        assert start >= 0
        assert lib.dgcnn_knn_seg_mix_min_n(-1) == start
        assert lib.dgcnn_knn_seg_mix_min_n(4096) == start
        assert lib.dgcnn_knn_seg_mix_min_n(-1) == 4096
        assert lib.dgcnn_knn_seg_mix_min_n(-7) == 4096
        assert lib.dgcnn_knn_seg_mix_min_n(0) == 4096          # 0 = the mix is off
        assert lib.dgcnn_knn_seg_mix_min_n(-1) == 0
        assert lib.dgcnn_knn_seg_mix_min_n(12288) == 0
        assert lib.dgcnn_knn_seg_mix_min_n(-1) == 12288
    finally:
        lib.dgcnn_knn_seg_mix_min_n(start)
    assert lib.dgcnn_knn_seg_mix_min_n(-1) == start


def test_segments_splits_a_tower_into_grid_clouds_first_then_scan_clouds():
    from dgcnn import _engine as E
    sizes = [300, 1000, 64, 999, 2000, 1000, 1001, 20]
    seg = E.Segments(np.concatenate([[0], np.cumsum(sizes)]))
    cpu = torch.device("cpu")
    lst, n_grid, grid_max, scan_min, scan_max = seg.mix(1000, cpu)
    assert lst.dtype == torch.int32 and lst.tolist() == [1, 4, 5, 6, 0, 2, 3, 7]      # a cloud of exactly T points is a grid cloud
    assert (n_grid, grid_max, scan_min, scan_max) == (4, 2000, 20, 999)
    lst2, n2, g2, s2, x2 = seg.mix(1001, cpu)
    assert lst2.tolist() == [4, 6, 0, 1, 2, 3, 5, 7] and (n2, g2, s2, x2) == (2, 2000, 20, 1000)
    # one list per threshold, made once
    assert seg.mix(1000, cpu)[0] is lst and seg.mix(1001, cpu)[0] is lst2
    assert lst.tolist() == [1, 4, 5, 6, 0, 2, 3, 7]
    # a tower of one class: the other class is empty, its numbers 0
    assert seg.mix(20, cpu)[1:] == (8, 2000, 0, 0) and seg.mix(20, cpu)[0].tolist() == list(range(8))
    assert seg.mix(2001, cpu)[1:] == (0, 0, 20, 2000) and seg.mix(2001, cpu)[0].tolist() == list(range(8))

"""The cell-grid k-NN of packed towers on the host: the workspace query and the rule by which the library sends a tower through the
grid (dgcnn_knn_seg_grid_workspace_bytes, dgcnn_knn_seg_grid_use; csrc/knn.hip, csrc/knn_grid.hip).  Neither makes a GPU call."""
import os

import pytest

GMAX3 = 16 ** 3                 # cells of the largest grid (csrc/knn_grid.hip: GMAX = 16)
GRID_INFO = 64                  # sizeof(GridInfo)
# the packed rule's threshold on the row-weighted mean cloud size (csrc/knn_grid.hip: GRID_SEG_MIN_MEAN, set by the measurement in
# profiles/packed/grid_bench.txt and grid_sweep.txt; the dense search's is 4096); the library reads the same variable as an override of both
MIN_MEAN = int(os.environ.get("DGCNN_KNN_GRID_MIN_N", 16384))


@pytest.fixture()
def lib():
    from dgcnn import _hip as H
    return H.load()


def expected_bytes(rows, nseg):
    sq = (rows * 4 + 255) // 256 * 256                          # s_i of every row, padded
    return sq + rows * (16 + 4 + 4) + nseg * ((GMAX3 + 1) * 4 + GRID_INFO) + 256


@pytest.mark.parametrize("rows,nseg", [(1, 1), (300, 3), (114234, 24)])
def test_workspace_is_the_documented_sum(lib, rows, nseg):
    assert lib.dgcnn_knn_seg_grid_workspace_bytes(rows, nseg) == expected_bytes(rows, nseg)


def test_workspace_grows_with_the_number_of_clouds_and_is_zero_for_an_empty_tower(lib):
    a, b = lib.dgcnn_knn_seg_grid_workspace_bytes(5000, 2), lib.dgcnn_knn_seg_grid_workspace_bytes(5000, 3)
    assert b - a == (GMAX3 + 1) * 4 + GRID_INFO
    for rows, nseg in ((0, 3), (-1, 3), (300, 0), (300, -2), (0, 0)):
        assert lib.dgcnn_knn_seg_grid_workspace_bytes(rows, nseg) == 0


def _dense(lib, C, k, nseg, N):
    """A dense-shaped tower: nseg clouds of N points."""
    return lib.dgcnn_knn_seg_grid_use(C, k, nseg, nseg * N, N, N, nseg * N * N)


def test_mode_0_never_and_mode_2_whenever_applicable(lib):
    prev = lib.dgcnn_knn_grid(0)
    try:
        for C, k, nseg, N in ((3, 20, 1, 65536), (4, 40, 24, 8192), (1, 1, 3, 100)):
            assert _dense(lib, C, k, nseg, N) == 0
        lib.dgcnn_knn_grid(2)
        for C, k, nseg, N in ((3, 20, 1, 65536), (4, 40, 24, 8192), (1, 1, 3, 100), (2, 8, 5, 20), (4, 40, 1, 40)):
            assert _dense(lib, C, k, nseg, N) == 1
        assert _dense(lib, 5, 20, 3, 8192) == 0                 # not raw coordinates
        assert _dense(lib, 3, 41, 3, 8192) == 0                 # the grid keeps at most 40 list entries
    finally:
        lib.dgcnn_knn_grid(prev)


def test_mode_1_flips_at_the_row_weighted_mean_cloud_size(lib):
    """sum_n2 / rows is what the all-pairs scan evaluates per row on average; the grid takes the tower from MIN_MEAN on."""
    prev = lib.dgcnn_knn_grid(1)
    try:
        rows = 30000
        at = MIN_MEAN * rows                                    # sum_n2 / rows == MIN_MEAN exactly
        assert lib.dgcnn_knn_seg_grid_use(3, 20, 7, rows, 100, 20000, at) == 1
        assert lib.dgcnn_knn_seg_grid_use(3, 20, 7, rows, 100, 20000, at - 1) == 0
        assert lib.dgcnn_knn_seg_grid_use(4, 40, 7, rows, 100, 20000, at + 1) == 1
        # a dense-shaped tower: sum_n2 / rows = N, so the rule is N >= MIN_MEAN, the form of the dense search's N >= 4096
        assert _dense(lib, 3, 20, 24, MIN_MEAN) == 1
        assert _dense(lib, 3, 20, 24, MIN_MEAN - 1) == 0
        if "DGCNN_KNN_GRID_MIN_N" not in os.environ:
            # one 65536-point event among 23 clouds of 1024 points: row-weighted mean ~48.8 k
            sizes = [65536] + [1024] * 23
            r, s2 = sum(sizes), sum(n * n for n in sizes)
            assert 48000 < s2 / r < 49500
            assert lib.dgcnn_knn_seg_grid_use(4, 20, len(sizes), r, 1024, 65536, s2) == 1
        assert lib.dgcnn_knn_seg_grid_use(5, 20, 7, rows, 100, 20000, at + 1) == 0
        assert lib.dgcnn_knn_seg_grid_use(3, 41, 7, rows, 100, 20000, at + 1) == 0
    finally:
        lib.dgcnn_knn_grid(prev)

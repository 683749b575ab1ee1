"""The mode matrix of tests/test_gpu_mode_matrix.py is complete (no GPU needed): every pair of values of two different settings is
run by at least one cell or is a refusal a cell asserts, every cell has its tests, and every run is a full assignment.  A seventh
setting added to mode_matrix_cells.SETTINGS fails here until the cells cover its pairs."""
import os
import re

import mode_matrix_cells as M


def test_every_run_assigns_every_setting_a_known_value():
    for cell, runs in M.CELLS.items():
        assert runs, cell
        for r in runs:
            assert tuple(r) == M.ORDER, (cell, r)
            for s, v in r.items():
                assert v in M.SETTINGS[s], (cell, s, v)


def test_every_pair_of_values_is_run_or_refused():
    missing, both = [], []
    for pair in M.all_pairs():
        cells = M.cells_running(pair)
        if pair in M.REFUSED:
            assert M.REFUSED[pair] in M.CELLS, pair
            if cells:
                both.append((pair, cells))
        elif not cells:
            missing.append(pair)
    assert not missing, "pairs of settings no cell runs: %s" % (missing,)
    assert not both, "refused pairs that a cell claims to run: %s" % (both,)
    assert all(p in M.all_pairs() for p in M.REFUSED), "a refusal names an unknown pair"
    n = len(M.all_pairs())
    assert n == sum(len(M.SETTINGS[a]) * len(M.SETTINGS[b]) for i, a in enumerate(M.ORDER) for b in M.ORDER[i + 1:]) == 81


def test_every_cell_has_a_gpu_test_and_every_gpu_test_a_cell():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_mode_matrix.py")).read()
    named = re.findall(r"^def test_([A-Z])_\w+\(", src, flags=re.M)
    assert named and len(named) == len(re.findall(r"^def test_\w+\(", src, flags=re.M)), "a test of the module names no cell"
    assert set(named) == set(M.CELLS), (sorted(set(named)), sorted(M.CELLS))
    assert "pytestmark = pytest.mark.gpu" in src


def test_the_replayed_sequences_of_cell_h_cover_both_packed_towers_under_both_replay_modes():
    assert sorted(M.H_RUNS) == sorted(set(M.H_RUNS)) and len(M.H_RUNS) == 4
    assert {(t, l) for t, _, l in M.H_RUNS} == {(t, l) for t in ("packed", "packed-bpc") for l in ("plan", "graph")}
    assert {lpc for _, lpc, _ in M.H_RUNS} == {False, True}

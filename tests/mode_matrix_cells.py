"""The run modes _engine.py, model.py and trainval.py switch on, and the cells of tests/test_gpu_mode_matrix.py that run them in
combination.  No GPU is needed to import this: tests/test_mode_matrix_cells.py checks on the host that every pair of values of two
different settings is run by some cell, or is a refusal some cell asserts.

A run lists what is ASKED FOR.  Where the engine answers a combination with a documented fall-back -- planes asked for in
DETERMINISTIC mode or on a packed tower run the fp32-class GEMMs, a packed tower under a replay mode runs eagerly -- the cell
asserts the fall-back (no plane GEMM was issued / nothing was recorded) next to the results."""

SETTINGS = {
    "det": (True, False),                              # flags.DETERMINISTIC
    "emd": ("f32", "bf16"),                            # flags.EDGE_MLP_DTYPE
    "planes": (False, True),                           # flags.HEAD_PLANES = "f16"
    "tower": ("dense", "packed", "packed-bpc"),        # offsets=..., with BN_PER_CLOUD_TRAIN
    "lpc": (False, True),                              # flags.LOSS_PER_CLOUD
    "launch": ("eager", "plan", "graph"),              # trainval.use_graph(False / "plan" / True)
}
ORDER = tuple(SETTINGS)


def run(det, emd, planes, tower, lpc, launch):
    return dict(zip(ORDER, (det, emd, planes, tower, lpc, launch)))


# cell -> the runs (full assignments) its tests make and check
CELLS = {
    "A": [run(False, "f32", True, "dense", False, "eager")],
    "B": [run(False, "f32", True, "dense", False, "eager")],
    "C": [run(False, "f32", True, "dense", False, "plan"), run(False, "f32", True, "dense", False, "graph")],
    "D": [run(True, "bf16", False, "dense", False, "plan"), run(True, "bf16", False, "dense", False, "graph")],
    "E": [run(True, "bf16", False, "dense", False, "eager")],
    "F": [run(True, "bf16", False, "packed", False, "eager"), run(False, "bf16", False, "packed", False, "eager")],
    "G": [run(False, "f32", True, "packed", False, "eager"), run(False, "f32", True, "packed-bpc", False, "eager")],
    "H": [run(True, "f32", False, "packed", False, "plan"), run(True, "f32", False, "packed", True, "graph"),
          run(True, "f32", False, "packed-bpc", True, "plan"), run(True, "f32", False, "packed-bpc", False, "graph"),
          # the all-eager sequences the replayed ones are held against; under LOSS_PER_CLOUD their reported loss is held against
          # the mean of the per-cloud losses
          run(True, "f32", False, "packed", True, "eager"), run(True, "f32", False, "packed-bpc", True, "eager")],
    "I": [run(False, "bf16", True, "dense", True, "plan")],
    "J": [run(True, "f32", False, "dense", False, "eager"), run(True, "f32", True, "dense", False, "eager")],
}

# pairs of values no run can have: (setting, value, setting, value) -> the cell whose test asserts the refusal
REFUSED = {
    ("emd", "bf16", "tower", "packed-bpc"): "J",       # per-cloud BatchNorm takes the default conv0 only (_engine.edge_conv_block)
}

# the H parametrisation: (tower, lpc, launch) of its four replayed sequences
H_RUNS = [(r["tower"], r["lpc"], r["launch"]) for r in CELLS["H"] if r["launch"] != "eager"]


def all_pairs():
    """Every (setting a, value, setting b, value) with a before b in ORDER."""
    out = []
    for i, a in enumerate(ORDER):
        for b in ORDER[i + 1:]:
            out += [(a, va, b, vb) for va in SETTINGS[a] for vb in SETTINGS[b]]
    return out


def cells_running(pair):
    a, va, b, vb = pair
    return sorted(c for c, runs in CELLS.items() if any(r[a] == va and r[b] == vb for r in runs))

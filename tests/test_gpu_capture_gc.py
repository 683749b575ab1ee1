"""trainval records a step (launch plan or HIP graph) with the cyclic garbage collector off: a collection in the middle of a recording can
free the private memory pools and captured graphs of an earlier trainval that died in a reference cycle, which the caching allocator
refuses while another pool or a capture is in use -- inside a destructor, which ends the process.  When the collector runs depends on
every allocation the process has made, so the recording must not depend on it: collected before, off during, back on after."""
import gc

import numpy as np
import pytest
import torch

import dgcnn

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("graph", ["plan", True], ids=["launch-plan", "hip-graph"])
def test_no_cyclic_collection_while_a_step_is_recorded(graph):
    rng = np.random.default_rng(3)
    pts = torch.from_numpy(rng.random((3, 2, 128, 3), dtype=np.float32)).cuda()
    lab = torch.from_numpy(rng.integers(0, 2, (3, 2, 128)).astype(np.int32)).cuda()
    flags = dgcnn.DGCNN_FLAGS(EDGE_CONV_LAYERS=2, EDGE_CONV_FILTERS=[32, 64], KVALUE=8, FC_LAYERS=1, FC_FILTERS=[64], NUM_CLASS=2,
                              NUM_CHANNEL=3, TRAIN=True, SEED=5, LEARNING_RATE=1e-3, DETERMINISTIC=True)
    assert gc.isenabled()
    tv = dgcnn.trainval(flags).initialize().use_graph(graph)
    c = dgcnn.ctx()
    body, seen = tv._tower_body, []

    def spy(*a, **k):
        seen.append((bool(c.capturing), gc.isenabled()))
        return body(*a, **k)
    tv._tower_body = spy
    try:
        for s in range(3):
            tv.zero_gradients(None)
            tv.accum_gradient(None, [pts[s]], [lab[s]])
            tv.apply_gradient(None)
            assert gc.isenabled(), "the collector stayed off after step %d" % s
    finally:
        tv._tower_body = body                                     # (the wrapper made a cycle through tv: undo it)
    assert len(tv._graphs) == 1
    recorded = [on for capturing, on in seen if capturing]
    assert len(recorded) == 1 and recorded == [False], seen      # one step was recorded, with the collector off
    assert all(on for capturing, on in seen if not capturing), seen

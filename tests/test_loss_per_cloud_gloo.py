"""The per-entry gather of the inference loop (main_funcs._entry_rows) with two replicas on CPU (gloo): shards that hold
DIFFERENT numbers of clouds arrive on rank 0 in batch order, the other rank gets nothing, and a rank that drew other entry
indices than rank 0 is an error on every rank."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

WORLD = 2
PER_CLOUD = {0: [[[0.5, 0.25], [0.75, 1.0]], [[1.5, 0.0]]],        # rank 0: a tower of two clouds and a tower of one
             1: [[[2.5, 0.5], [3.5, 0.125]]]}                      # rank 1: one tower of two
POINTS = {0: [300, 1400, 64], 1: [16777217, 256]}


def _worker(rank, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    from dgcnn import main_funcs as M
    from dgcnn import parallel
    h = M.Handlers()
    _, h.rank, h.world = parallel.dist_state()
    per = [torch.tensor(t, dtype=torch.float32) for t in PER_CLOUD[rank]]
    rows = M._entry_rows(h, per, POINTS[rank], [10, 11, 12, 13, 14])
    err = ""
    try:
        M._entry_rows(h, per, POINTS[rank], [10, 11, 12, 13, 14 + rank])
    except RuntimeError as e:                            # raised on EVERY rank: nobody waits in the gather for a rank that left
        err = str(e)
    torch.save({"rows": [r.tolist() for r in rows], "err": err}, "%s.r%d" % (out, rank))
    dist.destroy_process_group()


def test_two_ranks_with_unequal_shards_gather_in_batch_order(tmp_path):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "rows.pt")
    mp.spawn(_worker, args=(port, out), nprocs=WORLD, join=True)
    r0, r1 = torch.load(out + ".r0"), torch.load(out + ".r1")
    assert r0["rows"] == [[300.0, 0.5, 0.25], [1400.0, 0.75, 1.0], [64.0, 1.5, 0.0], [16777217.0, 2.5, 0.5], [256.0, 3.5, 0.125]]
    assert r1["rows"] == []
    for r in (r0, r1):
        assert "rank(s) 1 drew different entry indices than rank 0" in r["err"]

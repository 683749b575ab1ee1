"""Which kernel does a k-NN call launch?  Every k-NN form returns the same bits by design, so a test of one form passes just as well
when the host dispatch sends the call to another.  Each row of tests/dispatch_tables.py is one case here: the switches are set, the
call is recorded (tests/launch_trace.py: the library's own launch plan, read back through dgcnn_plan_kernel) and three things are
asserted --
  1. the ordered kernel list is the row's: base names and the template arguments the row names;
  2. grid y is the number of clouds, grid x ceil(largest cloud / rows per block) for the scan kernels;
  3. the indices are the oracle's (every row up to N = 4096, 512 sampled rows through O.k_nn_rows above), so no case only launches.
Rows that dgcnn._engine can issue go through it with a timer set, and the tag bench.py would print for the call is held against the
same recording: its [a+b+c] list equals the recorded base names ("knn_grid_*" for the two cell-grid kernels), its <C..,k..> the
CP / KC of the scan kernel that ran."""
import contextlib
import re

import numpy as np
import pytest
import torch

from oracle import dgcnn_oracle as O
from gpu_helpers import dev, host
from launch_trace import launches, timed, check_kernels, assert_launched
import dispatch_tables as T

pytestmark = pytest.mark.gpu

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        v = make()
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


def cloud(rows, C, tag=0):
    """Normals; raw coordinates (C <= 4): uniform, with two duplicated points."""
    def make():
        rng = np.random.default_rng(1000 * C + rows + tag)
        if C <= 4:
            x = rng.random((rows, C), dtype=np.float32)
            x[rows // 2] = x[3]
            x[rows - 1] = x[7]
            return x
        return rng.standard_normal((rows, C)).astype(np.float32)
    return cached(("x", rows, C, tag), make)


BIG_VIEW = 1 << 28      # elements (1 GiB of fp32) from which a view's buffer is allocated but never filled


def view(x, ld):
    """The rows on the device, contiguous or as a view into a buffer of `ld` columns (sentinel in the others; from BIG_VIEW
    elements on the buffer is torch.empty and only the view is written, on the device)."""
    if ld is None:
        return dev(np.array(x))
    if x.shape[0] * ld >= BIG_VIEW:
        buf = torch.empty(((x.shape[0] - 1) * ld + x.shape[1],), dtype=torch.float32, device="cuda")
        v = buf.as_strided(tuple(x.shape), (ld, 1))
        v.copy_(dev(np.array(x)))
        return v
    buf = torch.full((x.shape[0], ld), 777.0, dtype=torch.float32, device="cuda")
    buf[:, :x.shape[1]] = dev(np.array(x))
    return buf[:, :x.shape[1]]


@contextlib.contextmanager
def switches(sw, mix_t=None, table=None):
    from dgcnn import _hip as H
    lib = H.load()
    want = dict(T.KNN_DEFAULTS)
    want.update(sw)
    named = dict(T.TABLE_DEFAULTS)
    named.update(table or {})
    prev, prev_named = [], []
    try:
        for name, value in want.items():
            prev.append((name, getattr(lib, "dgcnn_knn_" + name)(value)))
        if mix_t is not None:
            prev.append(("seg_mix_min_n", lib.dgcnn_knn_seg_mix_min_n(mix_t)))
        for name, value in named.items():
            prev_named.append((name, H.switch(name)))
            H.set_switch(name, value)
        yield lib
    finally:
        for name, value in reversed(prev_named):
            H.set_switch(name, value)
        for name, value in reversed(prev):
            getattr(lib, "dgcnn_knn_" + name)(value)


def check_grids(L, max_n, ny, what, geom=None):
    for name, _, g, b, _ in L:
        m, y = (geom or {}).get(name, (max_n, ny))
        if name in T.ROWS_PER_BLOCK:
            rpb = T.ROWS_PER_BLOCK[name]
            assert g == ((m + rpb - 1) // rpb, y, 1), "%s: %s grid %s, largest cloud %d, %d clouds" % (what, name, g, m, y)
            assert b == (256, 1, 1)
        elif name == "knn_grid_build_kernel":
            assert g == (y, 1, 1) and b == (1024, 1, 1), (what, name, g, b)


def check_tag(tag, L, C, what):
    m = re.match(r"^knn_(?:seg_|cross_)?call<C(\d+),k(\d+)>\[(.*)\]$", tag)
    assert m, tag
    ran = []
    for e in L:
        if e[0] == "knn_grid_query_kernel" and ran and ran[-1] == "knn_grid_build_kernel":
            ran[-1] = "knn_grid_*"
        else:
            ran.append(e[0])
    assert m.group(3).split("+") == ran, "%s: the tag says %s, launched %s" % (what, tag, ran)
    scan = [e for e in L if e[0] in T.CP_KC_ARGS][-1]
    icp, ikc = T.CP_KC_ARGS[scan[0]]
    if icp is not None:
        cp = int(scan[1][icp])
    elif scan[0] == "knn_grid_query_kernel":
        cp = 4
    elif scan[0] in ("knn_bf16f_kernel", "knn_bf16a_kernel"):
        cp = 64
    elif scan[0] == "knn_cross_kernel":
        cp = int(scan[1][2]) if C <= 16 else (C + 63) // 64 * 64            # whole slabs of SL channels
    else:
        cp = (C + 63) // 64 * 64                                            # knn_wide_kernel, knn_bigk_kernel: slabs of 64
    assert int(m.group(1)) == cp, "%s: the tag says %s, %s<%s> ran" % (what, tag, scan[0], ", ".join(scan[1]))
    if ikc is not None:
        assert int(m.group(2)) == int(scan[1][ikc]), "%s: the tag says %s, %s<%s> ran" % (what, tag, scan[0], ", ".join(scan[1]))
    elif scan[0] == "knn_bigk_kernel":
        assert int(m.group(2)) == {"4": 128, "8": 256}[scan[1][0]], (what, tag, scan)


def same(got, want, what):
    bad = np.flatnonzero((got != want).any(-1))
    assert len(bad) == 0, "%s: %d of %d rows differ from the oracle, first row %d: %s vs %s" % (
        what, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]])


# ------------------------------------------------------------------------------------------------------
# dense: dgcnn_knn_f32 / dgcnn_knn_seeded_f32
# ------------------------------------------------------------------------------------------------------
SAMPLE = 512


def dense_ref(B, N, C, k):
    """-> (rows checked (None: all), the oracle's lists for them); above N = 4096 a sample of rows of the (single) cloud."""
    x = cloud(B * N, C)
    if N <= 4096:
        return None, cached(("ref", B, N, C, k), lambda: O.k_nn(np.array(x).reshape(B, N, C), k))
    assert B == 1
    rows = np.sort(np.random.default_rng(N).choice(N, SAMPLE, replace=False)).astype(np.int32)
    return rows, cached(("ref", B, N, C, k), lambda: O.k_nn_rows(np.array(x), k, rows))


def call_dense(r, xd, seed_d, kseed):
    """The row's call through the C entry, with the workspace the row names."""
    from dgcnn import _hip as H
    B, N, C, k = r["B"], r["N"], r["C"], r["k"]
    full = int(H.load().dgcnn_knn_workspace_bytes(B, N, C, k))
    s_i = (4 * B * N + 255) // 256 * 256
    nws = full if r["ws"] == "full" else s_i
    assert s_i < full
    ws = torch.empty((nws,), dtype=torch.uint8, device="cuda")
    idx = torch.full((B, N, k), -1, dtype=torch.int32, device="cuda")
    if seed_d is None:
        H.call("dgcnn_knn_f32", xd.data_ptr(), B, N, C, H.ld2(xd), k, idx.data_ptr(), ws.data_ptr(), nws)
    else:
        H.call("dgcnn_knn_seeded_f32", xd.data_ptr(), B, N, C, H.ld2(xd), k, seed_d.data_ptr(), int(seed_d.shape[2]), kseed,
               idx.data_ptr(), ws.data_ptr(), nws)
    return idx


@pytest.mark.parametrize("r", T.KNN_DENSE, ids=[r["id"] for r in T.KNN_DENSE])
def test_dense_row(r):
    from dgcnn import _engine as E
    from dgcnn import _hip as H
    B, N, C, k = r["B"], r["N"], r["C"], r["k"]
    rows, want = dense_ref(B, N, C, k)
    xd = view(cloud(B * N, C), r["ld"])
    assert H.ld2(xd) == (r["ld"] or C)
    seed_d, kseed = None, 0
    with switches(r["sw"], table=r["table"]):
        if r["seed"] is not None:
            # the row's own graph: the oracle's, or above N = 4096 (where only sampled rows have one) the library's unseeded lists,
            # which the check below holds against the oracle on the sampled rows like every other result
            g = want if rows is None else host(E.knn(xd, B, N, k))
            kseed = k if r["seed"] == "own" else k - 1
            seed_d = dev(np.array(g[..., :kseed], np.int32).reshape(B, N, kseed))
        if r["engine"]:
            assert E.KNN_SEED, "DGCNN_KNN_SEED=0: the engine would drop the seeds"
            with timed() as rec, launches() as L:
                idx = E.knn(xd, B, N, k, seed=seed_d)
            assert len(rec) == 1
            check_tag(rec[0][0], L, C, r["id"])
        else:
            with launches() as L:
                idx = call_dense(r, xd, seed_d, kseed)
    print(r["id"], [(e[0], e[1], e[2]) for e in L])
    check_kernels(L, r["expect"], r["id"])
    check_grids(L, N, B, r["id"])
    got = host(idx)
    if r["ld"] is not None and B * N * r["ld"] >= BIG_VIEW:        # hand the big buffer back: the pool would keep its block
        del xd
        torch.cuda.empty_cache()
    same(got.reshape(B * N, k) if rows is None else got[0][rows], want.reshape(-1, k), r["id"])


@pytest.mark.parametrize("N", [2048, 8192], ids=["lx", "carried_queue"])
def test_tighten_every_gives_the_same_indices(N):
    """DGCNN_KNN_TIGHTEN_EVERY = 1, 2 and 8 against the default (0: every 4th tile below N = 8192, every 8th from there on): one
    seeded append-form call of each form, (B, C, k) = (1, 64, 20), seeded by the k = 20 graph of the same cloud, gives bit-equal
    indices.  A row meets N / 64 candidate tiles (knn.hip:knn_bf16a_kernel: TJM = 64) and the first 8 are tightened at every
    setting, so a setting only shows from the 9th tile on: N = 2048 has 32 tiles, N = 8192 (the first N of the other form) 128."""
    from dgcnn import _engine as E
    from dgcnn import _hip as H
    B, C, k = 1, 64, 20
    assert N // 64 >= 16
    xd = dev(np.array(cloud(N, C)))
    out = {}
    with switches({}):
        seed = E.knn(xd, B, N, k)
        prev = H.switch("DGCNN_KNN_TIGHTEN_EVERY")
        try:
            for every in (0, 1, 2, 8):
                H.set_switch("DGCNN_KNN_TIGHTEN_EVERY", every)
                with launches() as L:
                    idx = E.knn(xd, B, N, k, seed=seed)
                print(N, every, [(e[0], e[1]) for e in L])
                assert_launched(L, "knn_bf16a_kernel", ["true" if N < 8192 else "false"])
                out[every] = host(idx)
        finally:
            H.set_switch("DGCNN_KNN_TIGHTEN_EVERY", prev)
    assert np.array_equal(out[0], host(seed)), "the seeded call differs from the unseeded graph of the same cloud"
    for every in (1, 2, 8):
        assert np.array_equal(out[every], out[0]), "DGCNN_KNN_TIGHTEN_EVERY=%d differs from the default" % every


# ------------------------------------------------------------------------------------------------------
# packed towers: dgcnn_knn_seg_f32 / dgcnn_knn_seg_grid_f32 / dgcnn_knn_seg_mix_f32, and the engine's choice among them
# ------------------------------------------------------------------------------------------------------
def tower(sizes, C, k):
    """-> (rows (R, C), offsets, the oracle's lists as tower rows (R, k))."""
    def make():
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        x = np.array(cloud(int(off[-1]), C, tag=len(sizes)))
        want = np.concatenate([O.k_nn(x[off[b]:off[b + 1]][None], k)[0] + off[b] for b in range(len(sizes))], 0).astype(np.int32)
        return x, off, want
    return cached(("tower", tuple(sizes), C, k), make)


@pytest.mark.parametrize("r", T.KNN_PACKED, ids=[r["id"] for r in T.KNN_PACKED])
def test_packed_row(r):
    from dgcnn import _engine as E
    from dgcnn import _hip as H
    sizes, C, k = r["sizes"], r["C"], r["k"]
    x, off, want = tower(sizes, C, k)
    R = len(x)
    seg = E.Segments(off, R)
    xd = dev(np.array(x))
    seed_d = None if r["seed"] is None else dev(np.array(want).reshape(1, R, k))
    mix_t = r["mix_t"] if r["entry"] == "engine" else 0
    with switches(r["sw"], mix_t=mix_t):
        if r["engine"]:
            with timed() as rec, launches() as L:
                idx = E.knn_packed(xd, k, seg, seed=seed_d)
            assert len(rec) == 1
            check_tag(rec[0][0], L, C, r["id"])
        else:
            idx = torch.full((1, R, k), -1, dtype=torch.int32, device="cuda")
            od = seg.device(xd.device)
            with launches() as L:
                if r["entry"] == "grid":
                    ws, nws = E._knn_workspace(xd, "dgcnn_knn_seg_grid_workspace_bytes", R, seg.nseg)
                    H.call("dgcnn_knn_seg_grid_f32", xd.data_ptr(), H.ld2(xd), C, k, seg.nseg, od.data_ptr(), R, seg.min_n, seg.max_n,
                           idx.data_ptr(), ws.data_ptr(), nws)
                else:
                    lst, n_grid, grid_max, scan_min, scan_max = seg.mix(r["mix_t"], xd.device)
                    assert 0 < n_grid < seg.nseg
                    ws, nws = E._knn_workspace(xd, "dgcnn_knn_seg_mix_workspace_bytes", R, n_grid)
                    H.call("dgcnn_knn_seg_mix_f32", xd.data_ptr(), H.ld2(xd), C, k, seg.nseg, od.data_ptr(), R, lst.data_ptr(), n_grid,
                           grid_max, scan_min, scan_max, idx.data_ptr(), ws.data_ptr(), nws)
    print(r["id"], [(e[0], e[1], e[2]) for e in L])
    check_kernels(L, r["expect"], r["id"])
    check_grids(L, max(sizes), len(sizes), r["id"], r["geom"])
    same(host(idx)[0], want, r["id"])


# ------------------------------------------------------------------------------------------------------
# two point sets: dgcnn_knn_cross_f32
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", T.KNN_CROSS, ids=[r["id"] for r in T.KNN_CROSS])
def test_cross_row(r):
    from dgcnn import _engine as E
    import knn_cross_reference as X
    C, k = r["C"], r["k"]
    if r["sizes"] is None:
        B, M, N = r["B"], r["M"], r["N"]
        ms, ns = [M] * B, [N] * B
    else:
        ms, ns = [s[0] for s in r["sizes"]], [s[1] for s in r["sizes"]]
        B, M, N = 1, sum(ms), sum(ns)
    p = cloud(sum(ns), C, tag=7)
    q = p if r["same"] else cloud(sum(ms), C, tag=8)
    qo, po = np.concatenate([[0], np.cumsum(ms)]), np.concatenate([[0], np.cumsum(ns)])
    want = cached(("cross", r["id"]), lambda: np.concatenate(
        [X.cross_knn(np.array(q[qo[b]:qo[b + 1]]), np.array(p[po[b]:po[b + 1]]), k)[0] + (po[b] if r["sizes"] is not None else 0)
         for b in range(len(ms))], 0).astype(np.int32))
    pd = view(p, r["ldp"])
    qd = pd if r["same"] else view(q, r["ldq"])
    qseg = pseg = None
    if r["sizes"] is not None:
        pseg = E.Segments(po, N)
        qseg = pseg if r["same"] else E.Segments(qo, M)
    with switches({}):
        with timed() as rec, launches() as L:
            idx = E.knn_cross(qd, pd, B, M, N, k, qseg=qseg, pseg=pseg)
    print(r["id"], [(e[0], e[1], e[2]) for e in L])
    assert len(rec) == 1
    check_tag(rec[0][0], L, C, r["id"])
    check_kernels(L, r["expect"], r["id"])
    check_grids(L, max(ms), len(ms), r["id"])
    same(host(idx).reshape(-1, k), want, r["id"])


# ------------------------------------------------------------------------------------------------------
# the tags at the shapes bench.py runs are the strings its per-kernel table has always shown
# ------------------------------------------------------------------------------------------------------
def test_tags_at_the_benchmark_shapes():
    """(B, N, k) = (24, 2048, 20): the raw-coordinate layer (C = 3), an unseeded 64-wide layer and one seeded with the graph before it
    (BASELINE.json configs[1], bench.py).  The strings are those of the committed benchmark records (BENCH_r06.json)."""
    from dgcnn import _engine as E
    B, N, k = 24, 2048, 20
    with switches({}):
        with timed() as rec:
            x3 = dev(np.random.default_rng(1).random((B * N, 3), dtype=np.float32))
            g0 = E.knn(x3, B, N, k)
            x64 = dev(np.random.default_rng(2).standard_normal((B * N, 64)).astype(np.float32))
            E.knn(x64, B, N, k)
            E.knn(x64, B, N, k, seed=g0)
    assert [t[0] for t in rec] == [
        "knn_call<C4,k20>[sqnorm_kernel+knn_hist_bound_kernel+knn_kernel]",
        "knn_call<C64,k20>[sqnorm_kernel+knn_mfma_kernel]",
        "knn_call<C64,k20>[sqnorm_kernel+knn_seed_bound_kernel+knn_bf16a_kernel+knn_select_kernel]"]


@pytest.mark.parametrize("B,N,k", [(8, 16384, 40), (8, 65536, 20)], ids=["configs2", "configs4-shard"])
def test_tags_at_the_larger_configs(B, N, k):
    """BASELINE.json configs[2] (B, N, k) = (8, 16384, 40) and one GPU's shard of configs[4], (8, 65536, 20): the raw-coordinate
    layer, an unseeded 64-wide layer and a seeded one.  The 64-wide strings are what they always were.  The raw-coordinate string
    CHANGED with the tags' rule "the list is what the call launches": these shapes take the cell grid, whose tag used to read
    knn_call<C4,k..>[knn_grid_*] and now names the norm kernel the call launches first, like every other tag.  Only the tags are read
    here; the indices at these sizes are tests/test_gpu_production_sizes.py's."""
    from dgcnn import _engine as E
    with switches({}):
        with timed() as rec:
            x3 = dev(np.random.default_rng(1).random((B * N, 3), dtype=np.float32))
            g0 = E.knn(x3, B, N, k)
            x64 = dev(np.random.default_rng(2).standard_normal((B * N, 64)).astype(np.float32))
            E.knn(x64, B, N, k)
            E.knn(x64, B, N, k, seed=g0)
            torch.cuda.synchronize()
    assert [t[0] for t in rec] == [
        "knn_call<C4,k%d>[sqnorm_kernel+knn_grid_*]" % k,
        "knn_call<C64,k%d>[sqnorm_kernel+knn_bf16f_kernel]" % k,
        "knn_call<C64,k%d>[sqnorm_kernel+knn_seed_bound_kernel+knn_bf16a_kernel+knn_select_kernel]" % k]

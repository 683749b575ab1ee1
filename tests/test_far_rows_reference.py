"""The inputs of tests/test_gpu_far_rows.py, checked without a GPU: that they reach the range they are meant for, and that a kernel
which sign-extends its 24-bit row product could not pass on them.  For every GPU case (tests/far_rows.py):
  (a) at least a quarter of the points have a neighbour whose row starts 2^31 elements or more past the base, and every row (k = 1:
      every far row, see far_rows.neighbours) is some point's neighbour -- conditions the graphs are built to meet;
  (b) under the "sign" model of the address exactly those rows resolve to a negative offset, under "zero" every row resolves to its
      own start inside the buffer;
  (c) the reference computed from the rows the "sign" model reads (row 0 standing in for what lies outside the buffer) differs from
      the true one in every output the GPU test compares -- the old arithmetic of edge_gather_add_kernel and of the packed
      statistics pass could not have passed;
  (d) the lattice bounds hold (asserted inside far_rows.dense_reference / packed_reference: bn_reference.lattice_precondition and
      far_rows.stats64), so "bit-equal to float64" is a fair demand."""
import numpy as np
import pytest

import far_rows as FR

DENSE = [(1, FR.W_N, k) for k in FR.W_KS] + [(2, FR.W_N2, FR.W_K)]
PACKED = [(FR.W_OFF, k) for k in FR.W_KS] + [((0, FR.W_N), FR.W_K)]


def test_the_address_model():
    ld = FR.W_LD
    assert 128 * ld == (1 << 31) - 512 and FR.W_FIRST_FAR * ld >= FR.FAR and FR.W_N * ld < 1 << 32
    assert FR.element_offset(128, ld, "sign") == 128 * ld == FR.element_offset(128, ld, "zero")
    assert FR.element_offset(129, ld, "zero") == 129 * ld and FR.element_offset(129, ld, "sign") == 129 * ld - (1 << 32)
    assert (FR.R_FIRST_FAR - 1) * FR.R_LD < FR.FAR <= FR.R_FIRST_FAR * FR.R_LD and FR.R_N * FR.R_LD == 2214558720 < 1 << 32
    far = FR.is_far(np.arange(FR.W_N), ld)
    assert not far[:FR.W_FIRST_FAR].any() and far[FR.W_FIRST_FAR:].all()
    assert FR.W_OFF[1] < FR.W_FIRST_FAR < FR.W_OFF[2]                      # cloud 1 straddles the mark, cloud 2 lies beyond it
    assert (FR.W_N2 - 1) * ld >= FR.FAR and (2 * FR.W_N2 - 1) * ld + FR.W_F < (1 << 32) + (1 << 31)


def check_graph(idx, rows, k, ld):
    """(a) and (b) for the neighbours idx (points, k) of one V operand of `rows` rows (the model per row, then per neighbour)."""
    j = np.arange(rows, dtype=np.int64)
    zero, sign = FR.element_offset(j, ld, "zero"), FR.element_offset(j, ld, "sign")
    far_rows = zero >= FR.FAR
    assert np.array_equal(zero, j * ld) and zero[-1] == (rows - 1) * ld            # "zero": every row at its own start, in the buffer
    assert np.array_equal(sign < 0, far_rows) and np.array_equal(sign[~far_rows], zero[~far_rows])
    assert idx.min() >= 0 and idx.max() < rows
    far = far_rows[idx]
    assert int(far.any(1).sum()) * 4 >= len(idx), "fewer than a quarter of the points have a far neighbour"
    seen = np.bincount(idx.reshape(-1), minlength=rows) > 0
    assert seen[far_rows].all() and (k == 1 or seen.all())
    return far


def differs(a, b, keys):
    for key in keys:
        assert a[key].shape == b[key].shape and not np.array_equal(a[key], b[key]), "%s does not depend on the far rows" % key


@pytest.mark.parametrize("B,N,k", DENSE)
def test_dense_cases(B, N, k):
    c = FR.dense_case(B, N, k)
    for b in range(B):
        check_graph(c.idx[b], N, k, c.ld)
    keys = ("y", "stats") + (("max", "mean", "packed", "red", "dY", "dYsum") if k == FR.W_K else ())
    for relu in (0, 1):
        true = FR.dense_reference(c, relu)                                           # (d) is asserted inside
        wrong = FR.dense_reference(c, relu, idx=FR.rows_read(c.idx, c.ld, "sign"), exact=False)
        differs(true, wrong, keys)


@pytest.mark.parametrize("off,k", PACKED)
def test_packed_cases(off, k):
    c = FR.packed_case(off, k)
    check_graph(c.idx, c.R, k, c.ld)
    assert all((c.idx[lo:hi] >= lo).all() and (c.idx[lo:hi] < hi).all() for lo, hi in zip(off[:-1], off[1:]))
    keys = ("y", "stats") + (("max", "mean", "packed", "red", "c1", "c2", "dY", "dYsum") if k == FR.W_K else ())
    true = FR.packed_reference(c, 1)
    wrong = FR.packed_reference(c, 1, idx=FR.rows_read(c.idx, c.ld, "sign"), exact=False)
    differs(true, wrong, keys)
    if len(off) > 2:                                                                  # per cloud: every cloud with far rows is off
        hit = [b for b in range(c.nseg) if not np.array_equal(true["stats"][b], wrong["stats"][b])]
        assert hit == [b for b in range(c.nseg) if off[b + 1] > FR.W_FIRST_FAR]


def test_the_one_cloud_tower_is_the_dense_case():
    """The header's promise "a one-cloud tower with the dense kernels' mean / rstd gives the dense entries' outputs bit for bit" is
    asserted on the GPU with the dense case's graph and parameters; the two references agree on it here."""
    d = FR.dense_case(1, FR.W_N, FR.W_K)
    p = FR.one_cloud_tower(d)
    a, b = FR.dense_reference(d, 1), FR.packed_reference(p, 1)
    for key in ("y", "max", "mean", "packed", "dY", "dYsum"):
        assert np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), key
    assert np.array_equal(a["stats"], b["stats"][0]) and np.array_equal(a["red"], b["red"][0])


def test_shape_r():
    c = FR.r_case()
    off = FR.R_OFF
    check_graph(c.idx, c.N, c.k, c.ld)
    assert all((c.idx[lo:hi] >= lo).all() and (c.idx[lo:hi] < hi).all() for lo, hi in zip(off[:-1], off[1:]))
    assert not FR.is_far(FR.R_FIRST_FAR - 1, c.ld) and FR.is_far(FR.R_FIRST_FAR, c.ld)
    wrong = FR.r_sums_under(c, "sign")
    assert np.array_equal(wrong[:-1], c.sums[:-1]) and not (wrong[-1, :2] == c.sums[-1, :2]).any()
    assert not (wrong[:, :2].sum(0) == c.sums[:, :2].sum(0)).any()                    # the dense totals

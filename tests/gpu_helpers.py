"""Shared helpers of the -m gpu tests (imported by test modules; nothing here runs without a GPU)."""
import os

import numpy as np
import torch


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def set_vars(dg, params):
    c = dg.ctx()
    for n, v in params.items():
        c.set_variable(n, v)


class capture_layers(object):
    """Context manager: records (input features (B,N,C) on the host, idx (B,N,k)) of every EdgeConv layer the
    HIP path runs, keyed by the layer's variable scope ('EdgeConv0', ...)."""

    def __init__(self, keep_inputs=True):
        self.layers = {}
        self.keep_inputs = keep_inputs

    def __enter__(self):
        from dgcnn import _engine as E
        self._E = E
        self._orig = orig = E.edge_conv_block
        cap = self

        def hook(x, B, N, k, F, **kw):
            mm, net, idx = orig(x, B, N, k, F, **kw)
            xin = host(x).reshape(B, N, -1).copy() if cap.keep_inputs else None
            cap.layers["/".join(E.ctx().scope)] = (xin, host(idx))
            return mm, net, idx
        E.edge_conv_block = hook
        return self

    def __exit__(self, *exc):
        self._E.edge_conv_block = self._orig
        return False


def run_model(dg, flags, pts, params, train, labels=None):
    """trainval on `pts` with the given parameter values; -> (trainval, result list, {scope: (x_in, idx)})."""
    tv = dg.trainval(flags)
    tv.initialize()
    if params is not None:
        set_vars(dg, params)
    with capture_layers() as cap:
        if train:
            tv.zero_gradients(None)
            res = tv.accum_gradient(None, [pts], [labels])
        else:
            res = tv.inference(None, [pts], None if labels is None else [labels])
    return tv, res, cap.layers


def idx_set_mismatch(a, b):
    """Fraction of rows whose neighbour SET differs / whose ordered list differs, for two (B,N,k) index arrays."""
    sa, sb = np.sort(a, axis=-1), np.sort(b, axis=-1)
    return float((sa != sb).any(-1).mean()), float((a != b).any(-1).mean())


def planes_to_host(ps):
    """Reassemble the fp32 values a plane set represents (sum of its planes), on the host."""
    from dgcnn import _planes as P
    npl = P.NPLANES[ps.fmt]
    raw = ps.buf.cpu().numpy().reshape(npl, -1)
    out = np.zeros((ps.rows, ps.cols), np.float64)
    for p in range(npl):
        a = raw[p].view(np.uint16).reshape(-1, ps.ra, 8)
        v = a.view(np.float16).astype(np.float32)
        o0 = ps.c0 // 8
        blk = v[o0:o0 + ps.cols // 8]                         # (noct, ra, 8)
        out += blk.transpose(1, 0, 2).reshape(ps.ra, -1)[:ps.rows].astype(np.float64)
    return out / (1.0 if ps.scale is None else float(ps.scale))


SENT = 777.0            # sentinel of the guarded buffers below
PAD = 64                # guard elements either side of every buffer (>= 256 bytes: keeps 16-byte alignment)


class Guard(object):
    """Device buffers between sentinel guards; check() asserts that no guard changed."""

    def __init__(self):
        self.bufs = []

    def new(self, shape, dtype=torch.float32, off=0, fill=SENT):
        n = int(np.prod(shape))
        flat = torch.full((n + 2 * PAD + off,), fill, dtype=dtype, device="cuda")
        self.bufs.append((flat, PAD + off, n, fill))
        return flat[PAD + off:PAD + off + n].view(*shape)

    def zeros(self, shape, dtype=torch.float32):
        v = self.new(shape, dtype)
        v.zero_()
        return v

    def put(self, a, off=0):
        a = np.ascontiguousarray(a)
        t = torch.from_numpy(a)
        v = self.new(a.shape, t.dtype, off)
        v.copy_(t)
        return v

    def check(self):
        torch.cuda.synchronize()
        for flat, lo, n, fill in self.bufs:
            h = host(flat)
            assert (h[:lo] == fill).all() and (h[lo + n:] == fill).all(), "a kernel wrote outside its buffer"


def ptr(t):
    return 0 if t is None else t.data_ptr()


# ---- worst observed summation error per kernel, in units of 2^-24 sum |term| (tests/test_gpu_bn_kernels.py, test_gpu_planes_bn.py)
RATIOS = {}             # kernel -> [worst |err| / (2^-24 sum |term|), n_terms of that case, bound factor]


def note_ratio(kernel, err, scale, n_terms, factor, record=True):
    """Assert that |err| / (2^-24 scale) (worst column) is within `factor`; record it in RATIOS (random-input cases only)."""
    scale = np.asarray(scale, np.float64)
    ratio = float((np.abs(err) / np.maximum(2.0 ** -24 * scale, 1e-300))[scale > 0].max(initial=0.0))
    dead = np.abs(err)[scale == 0]
    assert not dead.size or dead.max() == 0, "%s: a column whose terms are all zero has a non-zero sum" % kernel
    old = RATIOS.get(kernel)
    if record and (old is None or ratio > old[0]):
        RATIOS[kernel] = [ratio, int(n_terms), float(factor)]
    print("%s: worst |err| / (2^-24 sum|term|) = %.4g (bound %.6g, n_terms %d)" % (kernel, ratio, factor, n_terms))
    assert ratio <= factor, "%s: %.6g > %.6g" % (kernel, ratio, factor)


BN_HEADER = ["# worst |hip - float64| / (2^-24 * sum |term|) per column over the random-input cases of tests/test_gpu_bn_kernels.py and",
             "# tests/test_gpu_planes_bn.py; n_terms = terms per column of the case that gave the worst ratio; bound = what the test allows",
             "# (n_terms + 8: any-order fp32 summation plus the roundings inside a term; 4 / 5: the float64-accumulating det kernel;",
             "# edge_bwd_reduce_points: the summation term plus 4 sum |dz| (|xh| + 2 |beta|), smallest column of that case)"]


def ratio_table(header=None, env="DGCNN_BN_ERROR_TABLE", names=None):
    """Print the table of RATIOS: the rows of every module that has run in this process so far, so the table is complete after
    the last of them (test_gpu_bn_kernels.py, then test_gpu_planes_bn.py).  Also written to $DGCNN_BN_ERROR_TABLE when set
    (profiles/bn_kernel_errors.txt is a measured copy of a run of both modules).  A module with a table of its own passes its
    header lines, its environment variable and the kernels it recorded (`names`)."""
    lines = list(BN_HEADER if header is None else header)
    lines.append("%-44s %12s %10s %12s" % ("kernel", "worst ratio", "n_terms", "bound"))
    for name in sorted(RATIOS if names is None else names):
        r, n, b = RATIOS[name]
        lines.append("%-44s %12.4g %10d %12.6g" % (name, r, n, b))
    text = "\n".join(lines) + "\n"
    print("\n" + text)
    path = os.environ.get(env)
    if path:
        with open(path, "w") as f:
            f.write(text)

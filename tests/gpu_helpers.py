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


class capture_convs(object):
    """Context manager: records every E.conv_bn_act call the HIP path makes (the head's layers and conv1 / shortcut of the EdgeConv
    stack), keyed by the layer's variable scope ('MergedEdgeConv', 'FC0', 'EdgeConv1/conv1', ...):
      x    the (R, Cin) input the layer read, on the host in float64 -- decoded from its operand planes where the producer
           registered some (plane mode: the fp32 slice may never have been written), else the fp32 view;
      out  the (R, Cout) tensor the call returned (behind the dropout, when the layer carries one), from the planes where the
           call wrote no fp32 copy (f32_out=False);
      g    the per-cloud maximum returned with it (gmax=...), or None;
      planes_in / planes_out   whether x / out were read from planes;  kw   the call's keyword arguments."""

    def __init__(self):
        self.calls = {}

    def __enter__(self):
        from dgcnn import _engine as E
        self._E = E
        self._orig = orig = E.conv_bn_act
        cap = self

        def hook(x, leaf_scope, num_outputs, **kw):
            c = E.ctx()
            ps = c.planes.get(c.plane_key(x))
            xin = planes_to_host(ps) if ps is not None else host(x).astype(np.float64)
            ret = orig(x, leaf_scope, num_outputs, **kw)
            out, g = ret if isinstance(ret, tuple) else (ret, None)
            po = c.planes.get(c.plane_key(out)) if not kw.get("f32_out", True) else None
            cap.calls["/".join(c.scope + [leaf_scope])] = dict(
                x=xin, out=planes_to_host(po) if po is not None else host(out).astype(np.float64),
                g=None if g is None else host(g).astype(np.float64), planes_in=ps is not None, planes_out=po is not None, kw=dict(kw))
            return ret
        E.conv_bn_act = hook
        return self

    def __exit__(self, *exc):
        self._E.conv_bn_act = self._orig
        return False


# Bars other GPU modules share with the tests that set them (one definition, so that a mode's bar cannot drift between modules)
BF16_BLOCK_OUT_TOL = 1e-4      # test_gpu_bf16_edge_mlp.py::test_edge_conv_bf16_forward_backward: [max, mean, net], rtol = atol
BF16_BLOCK_GRAD_TOL = 2e-3     # ... its gradients: rtol, and atol = this times max(1, max |reference|)
BF16_MODEL_LOSS_TOL = 1e-4     # test_gpu_bf16_edge_mlp.py::test_model_gradients_bf16_small: loss against the oracle in bf16 mode
BF16_MODEL_GRAD_TOL = 4e-2     # ... every gradient tensor, relative Frobenius
LAYER_ATOL = 1e-4              # test_gpu_bf16_edge_mlp.py::test_config2_architecture_logits_n2048_bf16: a layer on its own input


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

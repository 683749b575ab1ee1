"""tests/tf1_standin.py -- TEST INFRASTRUCTURE ONLY (imported by tests/test_reference_program.py and tests/make_reference_golden.py).

A stand-in for the part of TensorFlow 1.x + tf.contrib.slim that the reference's dgcnn/ops.py, dgcnn/model.py and
dgcnn/trainval.py call (about 30 functions), backed by torch-CPU float64 tensors, so that the reference's UNMODIFIED program text
can be executed here and compared with oracle/dgcnn_oracle.py and oracle/torch_twin.py.  Written from TensorFlow's documented
behaviour; every library semantic below cites the paragraph of SURVEY.md Appendix A that states our reading of it.  What running
the reference under this module pins is the GRAPH and the TRAINING RULE as the reference's program text states them; the library
semantics (A.1-A.5) stay assumptions of this file, and TF's own float32 rounding order is not modelled at all: `tf.float32`
maps to float64 here.

Two ways to drive it:
  eager     tensors in, tensors out -- ops.py / model.py called directly, torch autograd gives every backward;
  deferred  a call with a placeholder-derived argument (also one nested in a list: ksize=[1, num_point, 1, 1]) returns a Node;
            Session.run(fetches, feed_dict) evaluates nested lists of Nodes with one memo per call -- trainval.py's way.

Variables are looked up by their scoped name ('EdgeConv0/conv0/weights') in the dict given to reference_program(); a conv
kernel is held as (Cin, Cout), the [1, 1] kernel axes of slim's [1, 1, Cin, Cout] dropped.  The stand-in has no initialisers.

    with reference_program(params) as ref:        # ref.ops / ref.model / ref.trainval: the reference's modules; ref.tf: this one
        logits = ref.model.build(points, flags)
Python's module table is the same before and after the `with` block (the project's own package is called `dgcnn` too).
"""
import contextlib
import operator
import os
import sys
import types

import numpy as np
import torch

F64 = torch.float64


# ----------------------------------------------------------------------------------------------------------------
# dtypes, graph state
# ----------------------------------------------------------------------------------------------------------------
class DType(object):
    def __init__(self, name, torch_dtype):
        self.name, self.torch = name, torch_dtype

    def __repr__(self):
        return "tf." + self.name


float32 = DType("float32", torch.float64)      # the stand-in computes every float in float64 (module docstring)
float64 = DType("float64", torch.float64)
int32 = DType("int32", torch.int64)
int64 = DType("int64", torch.int64)
AUTO_REUSE = "AUTO_REUSE"


class _Graph(object):
    def __init__(self, params=None, dropout_mask=None):
        self.params = dict(params or {})
        self.dropout_mask = dropout_mask      # None: tf.nn.dropout is the identity; else a {0, 1} keep mask (torch / numpy)
        self.scopes = []                      # [(name, reuse)]
        self.by_name = {}
        self.created = []                     # every Variable, creation order
        self.anon = 0


_G = _Graph()
_RUN = None                                   # the Session.run in flight: {"memo": {}, "feed": {}, "leaves": {}}


def reset(params=None, dropout_mask=None):
    """A fresh graph: no variables, no scopes.  params: scoped name -> array / tensor (a tensor with requires_grad is used as is)."""
    global _G
    _G = _Graph(params, dropout_mask)
    return _G


def created_variables():
    return list(_G.created)


# ----------------------------------------------------------------------------------------------------------------
# Variables
# ----------------------------------------------------------------------------------------------------------------
class Variable(object):
    """tf.Variable(initial_value, trainable=True).  Named variables come from _get_variable (slim's layers)."""

    def __init__(self, initial_value, trainable=True, name=None):
        v = initial_value
        if isinstance(v, Variable):
            v = v.value
        if not isinstance(v, torch.Tensor):
            v = torch.as_tensor(np.asarray(v))
        if v.is_floating_point() and v.dtype != F64:
            v = v.to(F64)
        if name is None:
            name = "Variable" if _G.anon == 0 else "Variable_%d" % _G.anon
            _G.anon += 1
            name = "/".join([s for s, _ in _G.scopes] + [name])
            v = v.detach().clone()
        self.value, self.trainable, self.scoped_name = v, bool(trainable), name
        _G.created.append(self)

    @property
    def name(self):
        return self.scoped_name + ":0"

    @property
    def shape(self):
        return tuple(self.value.shape)

    def initialized_value(self):
        return self.value.detach().clone()

    def read(self):
        if _RUN is None:
            return self.value
        leaf = _RUN["leaves"].get(id(self))
        if leaf is None:                      # one differentiable read per Session.run, so that compute_gradients can reach it
            leaf = self.value.detach().clone().requires_grad_(self.value.is_floating_point())
            _RUN["leaves"][id(self)] = leaf
        return leaf

    def assign(self, value):
        return Node(_assign, (self, value, False), {})

    def assign_add(self, value):
        return Node(_assign, (self, value, True), {})


def _assign(var, value, add):
    value = _t(value).detach()
    var.value = (var.value.detach() + value) if add else value.clone()
    if _RUN is not None:
        _RUN["leaves"].pop(id(var), None)
    return var.value


def trainable_variables():
    return [v for v in _G.created if v.trainable]


def _get_variable(name, shape, trainable):
    full = "/".join([s for s, _ in _G.scopes] + [name])
    reuse = any(r for _, r in _G.scopes)      # a scope's reuse flag is inherited by the scopes opened inside it
    if full in _G.by_name:
        if not reuse:
            raise ValueError("Variable %s already exists, disallowed. Did you mean to set reuse=tf.AUTO_REUSE?" % full)
        var = _G.by_name[full]                # AUTO_REUSE: the second tower gets the first tower's variable, listed once
    else:
        if full not in _G.params:
            raise KeyError("the stand-in has no initialisers: no value was supplied for variable %r" % full)
        var = Variable(_G.params[full], trainable=trainable, name=full)
        _G.by_name[full] = var
    if shape is not None and tuple(var.value.shape) != tuple(shape):
        raise ValueError("variable %s: supplied value has shape %s, the layer needs %s" % (full, tuple(var.value.shape), tuple(shape)))
    return var


@contextlib.contextmanager
def variable_scope(name, reuse=None):
    _G.scopes.append((name, bool(reuse)))
    try:
        yield name
    finally:
        _G.scopes.pop()


@contextlib.contextmanager
def name_scope(name):
    yield name + "/"                          # names ops only; variables ignore it (tf.get_variable ignores name_scope)


@contextlib.contextmanager
def device(name):
    yield


# ----------------------------------------------------------------------------------------------------------------
# Deferred nodes
# ----------------------------------------------------------------------------------------------------------------
class Node(object):
    last_dim = None                           # static size of the last axis where a layer knows it (slim.conv2d's output)

    def __init__(self, fn, args, kwargs):
        self.fn, self.args, self.kwargs = fn, args, kwargs

    def _bin(op, swap=False):
        def f(self, other):
            return Node(_arith, (op, other, self) if swap else (op, self, other), {})
        return f

    __add__, __radd__ = _bin(operator.add), _bin(operator.add, True)
    __sub__, __rsub__ = _bin(operator.sub), _bin(operator.sub, True)
    __mul__, __rmul__ = _bin(operator.mul), _bin(operator.mul, True)
    __truediv__, __rtruediv__ = _bin(operator.truediv), _bin(operator.truediv, True)
    __div__, __rdiv__ = __truediv__, __rtruediv__
    del _bin

    def __neg__(self):
        return Node(_arith, (operator.neg, self), {})

    def __getitem__(self, key):
        return Node(_arith, (operator.getitem, self, key), {})

    def __iter__(self):
        raise TypeError("a deferred tensor is not iterable")

    __hash__ = object.__hash__                # (feed_dict keys; no __eq__: tf.equal is the comparison)


class Placeholder(Node):
    def __init__(self, dtype, shape):
        Node.__init__(self, None, (), {})
        self.dtype, self.shape = dtype, None if shape is None else tuple(shape)
        if self.shape:
            self.last_dim = self.shape[-1]


def placeholder(dtype, shape=None, name=None):
    return Placeholder(dtype, shape)


def _arith(op, *a):
    return op(*[_t(x) if isinstance(x, (Variable, np.ndarray)) else x for x in a])


def _has_node(x):
    if isinstance(x, Node):
        return True
    if isinstance(x, (list, tuple)):
        return any(_has_node(y) for y in x)
    if isinstance(x, dict):
        return any(_has_node(y) for y in x.values())
    return False


def _evaluate(x):
    """Value of a fetch inside the Session.run in flight: Nodes once each (memo), containers element by element."""
    if isinstance(x, Placeholder):
        if x not in _RUN["feed"]:
            raise ValueError("You must feed a value for placeholder tensor of dtype %r and shape %r" % (x.dtype, x.shape))
        memo = _RUN["memo"]
        if id(x) not in memo:
            v = torch.as_tensor(np.asarray(_RUN["feed"][x])).to(x.dtype.torch)
            if x.shape is not None and (v.dim() != len(x.shape) or any(s is not None and s != d for s, d in zip(x.shape, v.shape))):
                raise ValueError("Cannot feed value of shape %s for a placeholder of shape %s" % (tuple(v.shape), x.shape))
            memo[id(x)] = v
        return memo[id(x)]
    if isinstance(x, Node):
        memo = _RUN["memo"]
        if id(x) not in memo:
            memo[id(x)] = x.fn(*_evaluate(x.args), **_evaluate(x.kwargs))
        return memo[id(x)]
    if isinstance(x, list):
        return [_evaluate(y) for y in x]
    if isinstance(x, tuple):
        return tuple(_evaluate(y) for y in x)
    if isinstance(x, dict):
        return {k: _evaluate(v) for k, v in x.items()}
    return x


def _op(fn, nout=1):
    """fn computes at once; the wrapped form returns a Node instead when an argument (nested ones included) is deferred."""
    def wrapper(*a, **kw):
        if _has_node((a, kw)):
            n = Node(fn, a, kw)
            return n if nout == 1 else tuple(n[i] for i in range(nout))
        return fn(*a, **kw)
    wrapper.__name__ = fn.__name__
    wrapper.raw = fn
    return wrapper


def _t(x):
    if isinstance(x, Variable):
        return x.read()
    if isinstance(x, torch.Tensor):
        return x
    t = torch.as_tensor(np.asarray(x))
    return t.to(F64) if t.is_floating_point() else t


def _ints(v):
    return [int(a) for a in v]


class Session(object):
    def __init__(self, *a, **kw):
        pass

    def run(self, fetches, feed_dict=None):
        global _RUN
        if _RUN is not None:
            raise RuntimeError("Session.run is not re-entrant")
        _RUN = {"memo": {}, "feed": dict(feed_dict or {}), "leaves": {}}
        try:
            return _to_numpy(_evaluate(fetches))
        finally:
            _RUN = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def _to_numpy(x):
    if isinstance(x, list):
        return [_to_numpy(y) for y in x]
    if isinstance(x, tuple):
        return tuple(_to_numpy(y) for y in x)
    if isinstance(x, Variable):
        return x.value.detach().numpy().copy()
    if isinstance(x, torch.Tensor):
        a = x.detach().numpy().copy()
        return a[()] if a.ndim == 0 else a
    return x


# ----------------------------------------------------------------------------------------------------------------
# tf.* functions (documented TF1 semantics; the axes / keyword names are TF's)
# ----------------------------------------------------------------------------------------------------------------
@_op
def transpose(a, perm=None):
    a = _t(a)
    return a.permute(*_ints(perm)) if perm is not None else a.permute(*reversed(range(a.dim())))


@_op
def matmul(a, b):
    return torch.matmul(_t(a), _t(b))


@_op
def square(x):
    x = _t(x)
    return x * x


@_op
def reduce_sum(x, axis=None, keepdims=False):
    x = _t(x)
    return x.sum() if axis is None else x.sum(dim=axis, keepdim=keepdims)


@_op
def reduce_max(x, axis=None, keepdims=False):
    x = _t(x)                                  # gradient: ties share equally, as TF's reduce_max does (A.5); torch.amax does the same
    return x.amax() if axis is None else x.amax(dim=axis, keepdim=keepdims)


@_op
def reduce_mean(x, axis=None, keepdims=False):
    x = _t(x)
    return x.mean() if axis is None else x.mean(dim=axis, keepdim=keepdims)


@_op
def tf_shape(x):
    return torch.tensor(list(_t(x).shape), dtype=torch.int64)


@_op
def tf_range(limit):
    return torch.arange(int(limit), dtype=torch.int64)


@_op
def reshape(x, shape):
    return _t(x).reshape(_ints(shape))


@_op
def gather(params, indices):
    return _t(params)[_t(indices)]             # axis 0; gradient = scatter-add, duplicates summed (A.5)


@_op
def expand_dims(x, axis):
    return _t(x).unsqueeze(axis)


@_op
def tile(x, multiples):
    return _t(x).repeat(*_ints(multiples))


@_op
def concat(values, axis):
    return torch.cat([_t(v) for v in values], dim=int(axis))


@_op
def squeeze(x, axis=None):
    x = _t(x)
    if axis is None:
        return x.squeeze()
    if x.shape[axis] != 1:
        raise ValueError("Can not squeeze dim[%d], expected a dimension of 1, got %d" % (axis, x.shape[axis]))
    return x.squeeze(axis)


@_op
def multiply(a, b):
    return _t(a) * _t(b)


@_op
def equal(a, b):
    return _t(a) == _t(b)


@_op
def argmax(x, axis=None):
    return _t(x).argmax(dim=axis)              # first maximal index, as tf.argmax


@_op
def to_int64(x):
    return _t(x).to(torch.int64)


@_op
def cast(x, dtype):
    return _t(x).to(dtype.torch)


def add_n(inputs):
    if not inputs:
        raise ValueError("inputs must be a list of at least one Tensor/IndexedSlices with the same dtype and shape")
    return _add_n(inputs)


@_op
def _add_n(inputs):
    out = _t(inputs[0])
    for v in inputs[1:]:
        out = out + _t(v)
    return out


@_op
def zeros_like(x):
    return torch.zeros_like(_t(x).detach())


# ---- tf.nn
@_op
def relu(x):
    return torch.relu(_t(x))                   # gradient 0 at 0 (A.5)


def _top_k(x, k=1):
    """A.1: descending values; among equal values the lower index first (TF's documented tie rule) -- a stable sort of -x."""
    x = _t(x)
    if k > x.shape[-1]:
        raise ValueError("input must have at least k columns")
    idx = torch.sort(-x.detach(), dim=-1, stable=True).indices[..., :k]
    return torch.gather(x, -1, idx), idx


top_k = _op(_top_k, nout=2)


@_op
def softmax(logits):
    return torch.softmax(_t(logits), dim=-1)


@_op
def dropout(x, keep_prob, noise_shape=None):
    """A.4: each element kept with probability keep_prob, kept values scaled by 1 / keep_prob.  The draw is the caller's: the
    graph's dropout_mask ({0, 1}, x's shape); None means the identity (no scaling either: what keep = 1.0 gives)."""
    x = _t(x)
    if _G.dropout_mask is None:
        return x
    return x * _t(_G.dropout_mask).to(F64) / float(keep_prob)


@_op
def sparse_softmax_cross_entropy_with_logits(logits=None, labels=None):
    logits, labels = _t(logits), _t(labels).to(torch.int64)        # A.4: per-element -log softmax(logits)[label]
    return -torch.gather(torch.log_softmax(logits, dim=-1), -1, labels.unsqueeze(-1)).squeeze(-1)


@_op
def max_pool_v2(x, ksize, strides, padding, name=None):
    """A.4 / A.5: NHWC window maximum; the gradient goes to the FIRST maximal element of a window (no splitting)."""
    x, ksize, strides = _t(x), _ints(ksize), _ints(strides)
    if ksize[0] != 1 or ksize[2] != 1 or ksize[3] != 1 or strides != [1, 1, 1, 1] or padding != "VALID":
        raise NotImplementedError("stand-in: max_pool_v2 over axis 1 only (ksize [1, h, 1, 1], unit strides, VALID)")
    u = x.unfold(1, ksize[1], 1)                                       # (B, H - h + 1, W, C, h)
    return torch.gather(u, -1, u.detach().argmax(dim=-1, keepdim=True)).squeeze(-1)


# ---- tf.contrib.slim
def conv2d(inputs, num_outputs, kernel_size, stride=1, padding="SAME", activation_fn=relu, normalizer_fn=None,
           normalizer_params=None, trainable=True, scope=None):
    """A.2: NHWC 1 x 1 convolution = a product over the last axis with `<scope>/weights`; NO bias when normalizer_fn is given;
    then normalizer_fn(outputs, **normalizer_params) -- `trainable` is not forwarded to it --; then activation_fn (default ReLU)."""
    if kernel_size not in (1, [1, 1], (1, 1)) or stride not in (1, [1, 1], (1, 1)):
        raise NotImplementedError("stand-in: 1 x 1 convolutions with stride 1 only")
    if normalizer_fn is None:
        raise NotImplementedError("stand-in: a conv2d without normalizer_fn would carry a bias; the reference has none")
    with variable_scope(scope if scope is not None else "Conv"):
        cin = inputs.last_dim if isinstance(inputs, Node) else int(_t(inputs).shape[-1])
        full = "/".join([s for s, _ in _G.scopes] + ["weights"])
        if cin is None and full in _G.params:
            # a deferred input of unknown width: the supplied value sets the static shape, the product checks it when it runs
            w = _get_variable("weights", None, trainable)
            if w.shape[1] != int(num_outputs):
                raise ValueError("variable %s: supplied value has shape %s, the layer has %d outputs" % (full, w.shape, num_outputs))
        else:
            w = _get_variable("weights", (cin, int(num_outputs)), trainable)
        out = _conv1x1(inputs, w)
        if isinstance(out, Node):
            out.last_dim = int(num_outputs)
        out = normalizer_fn(out, **(normalizer_params or {}))
        if activation_fn is not None:
            out = activation_fn(out)
        if isinstance(out, Node):
            out.last_dim = int(num_outputs)
    return out


@_op
def _conv1x1(x, w):
    x, w = _t(x), _t(w)
    if x.shape[-1] != w.shape[0]:
        raise ValueError("conv2d: input has %d channels, the kernel %s" % (x.shape[-1], tuple(w.shape)))
    return torch.matmul(x, w)


def batch_norm(inputs, decay=0.999, center=True, scale=False, epsilon=0.001, is_training=True, trainable=True, scope=None):
    """A.3: the defaults -- batch statistics (mean, BIASED variance) over all axes but the last, in training AND inference
    graphs (is_training is never set False by the reference), + beta (zero-initialised, always trainable), no gamma.  The
    moving averages are neither created nor updated here: the reference never runs UPDATE_OPS and never reads them."""
    if scale or not center or not is_training:
        raise NotImplementedError("stand-in: slim.batch_norm with its defaults only")
    with variable_scope(scope if scope is not None else "BatchNorm"):
        c = inputs.last_dim if isinstance(inputs, Node) else int(_t(inputs).shape[-1])
        beta = _get_variable("beta", None if c is None else (c,), trainable)
    out = _bn(inputs, beta, float(epsilon))
    if isinstance(out, Node):
        out.last_dim = c
    return out


@_op
def _bn(x, beta, eps):
    x, beta = _t(x), _t(beta)
    dims = tuple(np.arange(x.dim() - 1).tolist())
    mu = x.mean(dim=dims)
    var = ((x - mu) ** 2).mean(dim=dims)
    return (x - mu) / torch.sqrt(var + eps) + beta


# ---- tf.train
class AdamOptimizer(object):
    """A.4: m <- b1 m + (1 - b1) g;  v <- b2 v + (1 - b2) g^2;  theta <- theta - lr_t m / (sqrt(v) + eps) with
    lr_t = lr sqrt(1 - b2^t) / (1 - b1^t), t the 1-based count of apply_gradients runs: eps OUTSIDE the root."""

    def __init__(self, learning_rate=0.001, beta1=0.9, beta2=0.999, epsilon=1e-8):
        self.lr, self.b1, self.b2, self.eps = float(learning_rate), float(beta1), float(beta2), float(epsilon)
        self.t = 0
        self.slots = {}

    def compute_gradients(self, loss, var_list=None):
        """[(gradient, variable)] over tf.trainable_variables() as it stands at the call."""
        vs = list(var_list) if var_list is not None else trainable_variables()
        if not isinstance(loss, Node):
            g = torch.autograd.grad(_t(loss), [v.read() for v in vs], retain_graph=True, allow_unused=True)
            return list(zip(g, vs))
        bundle = Node(_gradients, (loss, vs), {})
        return [(bundle[i], v) for i, v in enumerate(vs)]

    def apply_gradients(self, grads_and_vars, global_step=None):
        return Node(self._apply, (list(grads_and_vars),), {})

    def _apply(self, gv):
        self.t += 1
        lr_t = self.lr * np.sqrt(1.0 - self.b2 ** self.t) / (1.0 - self.b1 ** self.t)
        for g, var in gv:
            if g is None:
                continue
            g = _t(g).detach()
            m, v = self.slots.setdefault(id(var), (torch.zeros_like(var.value), torch.zeros_like(var.value)))
            m.mul_(self.b1).add_(g, alpha=1.0 - self.b1)
            v.mul_(self.b2).add_(g * g, alpha=1.0 - self.b2)
            _assign(var, var.value.detach() - lr_t * m / (torch.sqrt(v) + self.eps), False)
        return None


def _gradients(loss, vs):
    return torch.autograd.grad(loss, [v.read() for v in vs], retain_graph=True, allow_unused=True)


# ---- tf.summary (inert)
def _summary_scalar(name, tensor):
    return None


def _summary_merge_all():
    return Node(lambda: None, (), {})


# ----------------------------------------------------------------------------------------------------------------
# The module objects the reference imports, and the loader of the reference's files
# ----------------------------------------------------------------------------------------------------------------
def _module(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    return m


def make_modules():
    """{'tensorflow': module, 'tensorflow.contrib.slim': module, ...}: everything the three reference files import."""
    nn = _module("tensorflow.nn", relu=relu, top_k=top_k, softmax=softmax, dropout=dropout,
                 sparse_softmax_cross_entropy_with_logits=sparse_softmax_cross_entropy_with_logits)
    train = _module("tensorflow.train", AdamOptimizer=AdamOptimizer)
    summary = _module("tensorflow.summary", scalar=_summary_scalar, merge_all=_summary_merge_all)
    slim = _module("tensorflow.contrib.slim", conv2d=conv2d, batch_norm=batch_norm)
    layers = _module("tensorflow.contrib.layers")
    contrib = _module("tensorflow.contrib", slim=slim, layers=layers)
    gen_nn_ops = _module("tensorflow.python.ops.gen_nn_ops", max_pool_v2=max_pool_v2)
    pops = _module("tensorflow.python.ops", gen_nn_ops=gen_nn_ops)
    platform = _module("tensorflow.python.platform")
    python = _module("tensorflow.python", ops=pops, platform=platform)
    tf = _module("tensorflow", transpose=transpose, matmul=matmul, square=square, reduce_sum=reduce_sum, reduce_max=reduce_max,
                 reduce_mean=reduce_mean, shape=tf_shape, range=tf_range, reshape=reshape, gather=gather, expand_dims=expand_dims,
                 tile=tile, concat=concat, squeeze=squeeze, multiply=multiply, equal=equal, argmax=argmax, to_int64=to_int64,
                 cast=cast, add_n=add_n, zeros_like=zeros_like, nn=nn, train=train, summary=summary, contrib=contrib,
                 python=python, variable_scope=variable_scope, name_scope=name_scope, device=device, placeholder=placeholder,
                 float32=float32, float64=float64, int32=int32, int64=int64, AUTO_REUSE=AUTO_REUSE, Variable=Variable,
                 trainable_variables=trainable_variables, Session=Session)
    return {m.__name__: m for m in (tf, nn, train, summary, contrib, slim, layers, python, pops, gen_nn_ops, platform)}


def reference_dir():
    return os.environ.get("DGCNN_REFERENCE_DIR", "/root/reference")


REFERENCE_FILES = ("ops", "model", "trainval")     # flags.py, iotool.py and main_funcs.py are Python-2-only: out of scope


def reference_present():
    return all(os.path.isfile(os.path.join(reference_dir(), "dgcnn", f + ".py")) for f in REFERENCE_FILES)


def _foreign(key):
    return key == "dgcnn" or key == "tensorflow" or key.startswith("tensorflow.")


class _Ref(object):
    pass


@contextlib.contextmanager
def reference_program(params=None, dropout_mask=None):
    """Load the reference's ops.py / model.py / trainval.py BY FILE PATH (its dgcnn/__init__.py uses Python-2 implicit imports)
    under the stand-in, bound to a synthetic `dgcnn` package object; yield an object with .ops .model .trainval .tf (this
    module) .graph.  sys.modules['dgcnn'] and every tensorflow* entry are restored to exactly what they were on exit."""
    before = {k: v for k, v in sys.modules.items() if _foreign(k)}
    graph = reset(params, dropout_mask)
    try:
        sys.modules.update(make_modules())
        pkg = types.ModuleType("dgcnn")
        pkg.__path__ = []
        sys.modules["dgcnn"] = pkg
        ref = _Ref()
        for f in REFERENCE_FILES:
            path = os.path.join(reference_dir(), "dgcnn", f + ".py")
            mod = types.ModuleType("dgcnn." + f)
            mod.__file__ = path
            with open(path) as fh:
                exec(compile(fh.read(), path, "exec"), mod.__dict__)    # (no bytecode is written next to the reference)
            setattr(pkg, f, mod)
            setattr(ref, f, mod)
        ref.tf, ref.graph = sys.modules[__name__], graph
        yield ref
    finally:
        for k in [k for k in sys.modules if _foreign(k)]:
            del sys.modules[k]
        sys.modules.update(before)
        reset()

"""Host-side engine: variable store, backward tape and the composite EdgeConv / conv+BN blocks.

The reference builds a TF1 graph once and replays it with sess.run (dgcnn/trainval.py:12-85).
Here every call runs the HIP kernels immediately on the current stream and records one closure
per block on a tape; `backward()` replays the tape in reverse.  There is no autograd and no
torch math on the path: torch tensors only hold memory.

Layout conventions (DESIGN.md "Data layout"):
  * every activation is a 2-D row-major view (rows = points or edges, cols = channels) with an
    explicit leading dimension, so the outputs of one block can be written straight into column
    slices of a wider buffer (the tf.concat of dgcnn/ops.py:58 and model.py:63,85 never copies);
  * gradients mirror the forward buffers: the gradient of a column slice is the same slice of the
    gradient of its parent buffer (found by address), zero-initialised, always accumulated into;
  * parameters, their gradient accumulators and the Adam moments live in four flat fp32 buckets
    (one RCCL all-reduce, one fused Adam launch per step);
  * conv0 of an EdgeConv layer is a point-level GEMM [U|V] = X [Wa-Wb | Wb]; its (B*N*k, F) output is never
    written: the BatchNorm passes recompute V[neighbour] + U[point] (edge_conv_block);
  * work that only the optimizer needs (weight-gradient GEMMs, the transposed adjacency) runs on a second
    HIP stream (Context.off_critical_path) and joins before the tape is released.
"""
from __future__ import annotations

import contextlib
import os
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import torch

from . import _hip as H
from . import _planes as PL

BN_EPS = 1e-3          # slim.batch_norm default epsilon [TF1-lib]
DROPOUT_KEEP = 0.7     # tf.nn.dropout(net, 0.7): dgcnn/model.py:91
WS_BYTES = 256 << 20
EDGE_MLP_LITERAL = False  # True: conv0 as the literal (B*N*k) x 2C GEMM over E = [x_i, x_j - x_i] (A/B switch)
EDGE_MATERIALIZE_Y = False  # True: gather-add writes the (B*N*k, F) conv0 output and BatchNorm streams it (A/B switch);
                            # False: the BatchNorm passes recompute y = V[neighbour] + U[point] (no edge tensor in the forward)
WGRAD_SIDE_STREAM = os.environ.get("DGCNN_SIDE_STREAM", "1") != "0"   # weight-gradient GEMMs on a second HIP stream
# Fusions with a separate-pass twin that the tests compare them against (module constants, not run-time switches):
EDGE_BWD_FUSED_L0 = True   # input layer (C <= 4, no input gradient): conv0's whole backward in one pass
FUSE_DROPOUT = True        # tf.nn.dropout inside the last FC layer's BatchNorm passes
# the class-dimension tail (last FC layer -> Final -> loss) in 8 launches instead of 15: the Final layer's two class products are
# formed inside the FC layer's BatchNorm passes, the launches on the (R, NUM_CLASS) logits fold into their neighbours
# (csrc/bn.hip: bn1_act_class_kernel ...).  Bit-identical to the separate launches; DGCNN_FUSE_CLASS_TAIL=0 selects those.
FUSE_CLASS_TAIL = os.environ.get("DGCNN_FUSE_CLASS_TAIL", "1") != "0"
BF16_FUSED_BWD = True      # bf16 edge-MLP: the layer's backward in one pass over the edges (tests switch it off to compare)
SIDE_STREAM_MIN_ROWS = 16384   # below this many points the side stream is not used
# the side stream's work is off the critical path: least priority / a CU mask that leaves some compute units to the main stream alone
# (csrc/plan.cc:dgcnn_stream_create; A/B switches -- neither helps, the mask costs 40 %: profiles/r06/side_stream.txt)
SIDE_STREAM_LOW_PRIORITY = os.environ.get("DGCNN_SIDE_LOW_PRIORITY", "0") not in ("0", "")
SIDE_STREAM_RESERVE_CUS = int(os.environ.get("DGCNN_SIDE_RESERVE_CUS", "0"))
# conv0 of every EdgeConv layer with bf16 OPERANDS (BASELINE.json configs[2] "bf16 edge-MLP MFMA"): E = [x_i, x_j - x_i] is formed
# in fp32, E and W0 are rounded to bf16 once, the literal (B*N*k) x 2C x F product runs on v_mfma_f32_32x32x16_bf16 with fp32
# accumulation; the two gradient products round their operands the same way.  "f32" (default): the fp32-class folded form.
# trainval.initialize() sets it per instance from flags.EDGE_MLP_DTYPE.
EDGE_MLP_DTYPE = "f32"
EDGE_MLP_NBR_GEMM = False  # True: factored conv0 with an edge-level neighbour GEMM instead of point-level GEMM + gather-add
# Deterministic mode (the DEFAULT since round 5): run-to-run bit-reproducible results.  Every statistics / reduction slot has ONE
# writer (dgcnn_set_stat_slots raises the slot count to the widest producer's workgroup count), the finalize kernels add the slots
# in a fixed order, the transposed adjacency's buckets are sorted.  Same kernels as the atomics mode otherwise: +3-4 % at
# configs[1].  The atomics mode (DETERMINISTIC=False / DGCNN_DETERMINISTIC=0: 32 slots, fp64 atomics from several
# workgroups per slot, unsorted buckets) is reproducible to ~1e-7 per step only, which the dynamic graphs amplify into a few
# different neighbour lists per step.  The reported loss / accuracy scalars are summed with atomics in both (they feed nothing back).
DETERMINISTIC_ENV_DEFAULT = os.environ.get("DGCNN_DETERMINISTIC", "1") not in ("0", "")
DETERMINISTIC = DETERMINISTIC_ENV_DEFAULT      # trainval.initialize() sets it per instance (flag, else this default)


# Head GEMMs (MergedEdgeConv, FC0, FC1: 98 % of the step's GEMM flops) from pre-split operand planes (csrc/gemm_pl.hip):
#   "f16"  two fp16 planes per operand, 3 partial products   "0"  off
HEAD_PLANES_ENV_DEFAULT = {"f16": PL.F16X2}.get(os.environ.get("DGCNN_HEAD_PLANES", "0").lower())
HEAD_PLANES = HEAD_PLANES_ENV_DEFAULT          # trainval.initialize() sets it per instance (flag HEAD_PLANES, else this default)
PLANES_MIN_ROWS = 8192


def planes_ok(R, Cin, Cout):
    """The plane GEMM takes this layer: head-sized problems with tile-friendly widths, variables in the flat bucket (the
    step's scales come from it), default (atomically summed) BatchNorm statistics."""
    return (HEAD_PLANES is not None and not DETERMINISTIC and ctx().flat_param is not None and R >= PLANES_MIN_ROWS and
            Cin % 32 == 0 and Cout % 32 == 0 and Cout >= 128 and Cin >= 128 and Cout <= 1024)


class Context(object):
    def __init__(self):
        self.vars = OrderedDict()        # name -> 2-D / 1-D tensor (views of flat_param when allocated)
        self.var_grads = {}              # name -> tensor (views of flat_grad)
        self.flat_param = self.flat_grad = self.flat_m = self.flat_v = None
        self.scope = []
        self.tape = []
        self.roots = []                  # [(buffer, [grad or None])]
        self.recording = False
        self.ws = None
        self.ws_side = None
        self.side = None                 # second HIP stream: weight-gradient GEMMs (nothing on the critical path needs them)
        self.side_busy = False
        self.side_hold = []              # recording a launch plan: tensors the side stream touches, kept until the join
        self._slot_stack = []
        self.step_slots = 32             # slot count the step's arena is sized for (configure_slots); ops may use fewer (op_slots)
        self.capture_extent = None       # recording: doubles of the arena the recorded step zeroes (what an eager run of it used)
        self.seed = 1
        self._rng = None
        self.stat_arena = None
        self.stat_off = 0
        self.arena_gen = 0               # bumped whenever the statistics arena is (re)allocated
        self.step_seed = 0
        self.seed_dev = None             # device uint64: the dropout seed of the running step (read by the kernels)
        self.capturing = False           # inside a HIP-graph capture: no host-side per-step state may be baked in
        self.debug = False
        self.planes = {}                 # (data_ptr, rows, cols) of an fp32 2-D view -> PlaneSet holding it as GEMM operand planes (this step)
        self.pl_scales = None            # device float[2]: power-of-two scales of the step's activation / weight plane sets (fp16 planes)
        self.pl_scales_ready = False
        self.pl_ws = None
        self.wprep = {}                  # weight-only work of the step, issued ahead on the side stream: key -> tensor / PlaneSet
        self.wprep_event = None          # True while the main stream has not yet been made to wait for it (prepared())
        self.head_grads_hook = None      # called by the backward when every head gradient is final (trainval: bucketed all-reduce)
        # the class-dimension tail (FUSE_CLASS_TAIL): launches held back until their consumer is known
        self.dense_loss_follows = False  # set by trainval around model.build: the dense softmax_loss consumes the logits next
        self.class_tail = None           # last FC layer: its BatchNorm + dropout pass, waiting for the Final layer's weight
        self.loss_tail = None            # Final layer: its BatchNorm finalize + activation, waiting for softmax_loss

    # ---- device / scratch -------------------------------------------------------------
    @property
    def device(self):
        if not torch.cuda.is_available():
            raise H.HipError("no GPU visible: the dgcnn HIP path has no CPU fallback")
        return torch.device("cuda", torch.cuda.current_device())

    def workspace(self):
        if torch.cuda.current_stream() == self.side and self.side is not None:
            if self.ws_side is None or self.ws_side.device != self.device:
                self.ws_side = torch.empty(WS_BYTES, dtype=torch.uint8, device=self.device)
            return self.ws_side
        if self.ws is None or self.ws.device != self.device:
            self.ws = torch.empty(WS_BYTES, dtype=torch.uint8, device=self.device)
        return self.ws

    @contextlib.contextmanager
    def off_critical_path(self, *temporaries, rows=1 << 30):
        """Run the enclosed launches on the side stream, ordered after everything issued so far on the
        current stream.  The bf16-split GEMMs run at the package power cap while the BatchNorm / gather passes
        of the backward chain are bandwidth bound: a weight-gradient GEMM (needed only by the optimizer)
        issued here overlaps the chain instead of stalling it.  `temporaries`: tensors allocated on the main
        stream that the side work touches and that may be freed before the streams join."""
        if not WGRAD_SIDE_STREAM or rows < SIDE_STREAM_MIN_ROWS:      # tiny problems are host-launch bound: the
            yield                                                       # stream switches only add latency there
            return
        main = torch.cuda.current_stream()
        if self.side is None or self.side.device != self.device:
            self.side = H.make_stream(self.device, low_priority=SIDE_STREAM_LOW_PRIORITY, reserve_cus=SIDE_STREAM_RESERVE_CUS)
        H.stream_wait(self.side, main)
        for t in temporaries:
            t.record_stream(self.side)
        if self.capturing:
            # a recorded step is replayed with the addresses of THIS run: a block the allocator handed out again because it SAW the
            # side stream finish (an event query, not stream order) would be a race on replay -- side-stream temporaries stay
            # alive until the streams have joined
            self.side_hold.extend(temporaries)
        self.side_busy = True
        with torch.cuda.stream(self.side):
            yield

    def join_side(self):
        if self.side_busy:
            H.stream_wait(torch.cuda.current_stream(), self.side)
            self.side_busy = False
        self.side_hold = []

    def stats(self, F):
        """Zeroed double[SLOTS][2][F] carved from one arena that is memset once per step."""
        slots = H.stat_slots()
        n = slots * 2 * F
        want = self.arena_want(slots)
        if self.stat_arena is None or self.stat_arena.device != self.device or self.stat_arena.numel() < want:
            # a captured HIP graph has the arena's address (and the slot count) baked into its launches: trainval keys its
            # graphs on arena_key() and drops those recorded against an arena that no longer exists
            self.stat_arena = H.zeros(want, torch.float64, self.device)
            self.stat_off = 0
            self.arena_gen += 1
        if self.stat_off + n > want:
            return H.zeros(n, torch.float64, self.device)
        s = self.stat_arena[self.stat_off:self.stat_off + n]
        self.stat_off += n
        return s

    def arena_want(self, slots=None):
        """Doubles of the statistics arena a step may use at its slot count: 8 MB at 32 slots, 96 MB at 768.  The arena itself may
        be larger (an earlier, larger cloud grew it): a step carves from -- and a captured step zeroes -- at most this much.
        slots: the calling thread's count where the caller has just read it."""
        n = max(self.step_slots, H.stat_slots() if slots is None else slots)
        return (1 << 20) if n <= 32 else (1 << 19) * -(-n // 32)

    def arena_key(self):
        """What a captured step depends on besides its inputs: the statistics arena it zeroes / writes and the slot count its
        launches carry as arguments."""
        return (self.arena_gen, H.stat_slots(), 0 if self.stat_arena is None else self.stat_arena.data_ptr())

    def ensure_arena(self, rows):
        """Slot count and arena for a step over `rows` points, settled OUTSIDE a capture (so that the capture neither allocates
        the arena inside its private pool nor changes the slot count half way)."""
        self.configure_slots(rows)
        off = self.stat_off
        self.stats(1)
        self.stat_off = off

    def configure_slots(self, rows=0):
        """DETERMINISTIC: every stats / red slot gets a single writer -- as many slots as the producer with the most workgroups has
        (a GEMM over `rows` rows in 64-row tiles; the reduction kernels cap their grids at the slot count) -- so that no sum
        depends on the order in which workgroups finish.  A pure function of `rows`: the reduction kernels' grids follow the slot
        count, so a count that remembered earlier, larger steps would make a step's rounding depend on the process' history
        (round 5: the same step in a fresh process and after a 65536-point cloud differed by 4e-4 -- both "deterministic").
        Atomics mode: DGCNN_STAT_SLOTS (32) slots, several writers each."""
        if DETERMINISTIC:
            n = max(256, -(-int(rows) // 64))                              # (the finalize kernels walk all of them: no rounding up)
            n = -(-n // 64) * 64
        else:
            n = 32
        self.step_slots = n
        if n != H.stat_slots():
            H.set_stat_slots(n)

    def push_slots(self, writers=0):
        """op_slots() as a pair of calls (the producer and its finalize sit far apart in the block functions)."""
        prev = H.stat_slots()
        self._slot_stack.append(prev)
        if DETERMINISTIC:
            n = max(256, -(-int(writers) // 64) * 64)
            if n != prev:
                H.set_stat_slots(n)

    def pop_slots(self):
        prev = self._slot_stack.pop()
        if H.stat_slots() != prev:
            H.set_stat_slots(prev)

    @contextlib.contextmanager
    def op_slots(self, writers=0):
        """DETERMINISTIC: the slot count of ONE op's statistics buffers -- its producer's writer workgroups (a GEMM's row tiles:
        dgcnn_gemm_stat_writers; 0 for the reduction kernels, whose grids follow the slot count), at least 256 -- instead of the
        step-wide maximum: the head's GEMMs run 192 row tiles where conv1's run 768, and every finalize kernel walks (and every
        step zeroes) all slots of its buffer.  Producer and finalize are issued inside the block: they see the same count."""
        self.push_slots(writers)
        try:
            yield
        finally:
            self.pop_slots()

    # ---- operand planes of the head GEMMs (csrc/gemm_pl.hip, planes_bn.hip) ------------------------------
    @staticmethod
    def plane_key(v):
        return (v.data_ptr(), int(v.shape[0]), int(v.shape[1]))

    def ensure_plane_scales(self, rows_max):
        """One pass over the parameter bucket per step: the power-of-two scales of every activation plane set
        (|z| <= 2 (sqrt(rows_max) + max |parameter|) bounds any batch-normalised tensor of the model and the residual sums
        of two of them) and of the weight plane sets.  Only the fp16 plane format is scaled."""
        if HEAD_PLANES != PL.F16X2 or self.pl_scales_ready:
            return
        if self.pl_scales is None or self.pl_scales.device != self.device:
            self.pl_scales = torch.ones(2, dtype=torch.float32, device=self.device)
            self.pl_ws = torch.zeros(1, dtype=torch.int32, device=self.device)
        H.call("dgcnn_param_scales_f32", self.flat_param.data_ptr(), self.flat_param.numel(), float(rows_max), 2.0,
               self.pl_scales.data_ptr(), self.pl_ws.data_ptr())
        self.pl_scales_ready = True

    def new_planes(self, rows, cols, kind):
        """An empty plane set in the head format; kind 'act' / 'w' picks the step's preset scale, 'own' leaves it to the producer."""
        ps = PL.PlaneSet(rows, cols, HEAD_PLANES, device=self.device)
        if HEAD_PLANES == PL.F16X2:
            if kind == "own":
                ps.scale = torch.empty(1, dtype=torch.float32, device=self.device)
            else:
                ps.scale = self.pl_scales[0:1] if kind == "act" else self.pl_scales[1:2]
        return ps

    def planes_of(self, x):
        """The operand planes of the fp32 view x: registered by its producer, or split here (one extra pass)."""
        ps = self.planes.get(self.plane_key(x))
        if ps is None:
            ps = self.new_planes(x.shape[0], x.shape[1], "act").fill_from(x)
            self.planes[self.plane_key(x)] = ps
        return ps

    def stats_raw(self, n):
        """n zeroed doubles from the per-step arena."""
        if self.stat_arena is None or self.stat_arena.device != self.device:
            self.stats(1)
            self.stat_off = 0
        if self.stat_off + n > min(self.stat_arena.numel(), self.arena_want()):
            return H.zeros(n, torch.float64, self.device)
        s = self.stat_arena[self.stat_off:self.stat_off + n]
        self.stat_off += n
        return s

    def zeros_f32(self, n):
        """n zeroed floats: small requests come out of the statistics arena (zeroed once per step by ONE memset; every separate
        memset is a ~6-us serial step of its own on the main stream), large ones get their own fill."""
        if n <= 65536 and self.stat_arena is not None:
            nd = ((n + 3) // 4) * 2                       # whole 16-byte units, from a 16-byte aligned start
            off = (self.stat_off + 1) & ~1
            if off + nd <= min(self.stat_arena.numel(), self.arena_want()):
                s = self.stat_arena[off:off + nd].view(torch.float32)[:n]
                self.stat_off = off + nd
                return s
        return H.zeros(n, torch.float32, self.device)

    def zeros_like_small(self, t):
        if t.dtype == torch.float32 and t.is_contiguous():
            return self.zeros_f32(t.numel()).view(t.shape)
        return H.memset(torch.empty_like(t))

    def begin_step(self):
        """Drop the previous tape / gradient roots, re-zero the statistics arena and advance the dropout stream."""
        self.tape = []
        self.roots = []
        self.planes = {}
        self.pl_scales_ready = False
        self.wprep = {}
        self.wprep_event = None
        self._slot_stack = []
        self.class_tail = self.loss_tail = None
        slots = H.stat_slots()
        if not DETERMINISTIC and slots != 32:
            H.set_stat_slots(32)
        elif DETERMINISTIC and slots < 256:
            self.configure_slots(0)           # (stand-alone ops; a model step sets its own count in model.build)
        if self.stat_arena is not None:
            if self.capturing:
                # a captured step cannot know what ran before it: everything the step uses -- as measured on an eager run of the
                # same shape (trainval passes it) -- else everything a step at this slot count may use
                ext = min(self.stat_arena.numel(), self.arena_want())
                if self.capture_extent is not None:
                    ext = min(ext, max(int(self.capture_extent), 1))
                H.memset(self.stat_arena[:ext])
            elif self.stat_off > 0:
                H.memset(self.stat_arena[:self.stat_off])
        self.stat_off = 0
        if not self.capturing:                   # (a replayed graph gets its seed from advance_seed(), called by the replayer)
            self.advance_seed()

    def advance_seed(self):
        """Next position of the dropout mask stream.  The seed lives in DEVICE memory (dgcnn_dropout_dev_f32 reads it at
        execution time), written here by a fill kernel that carries the value as a launch argument -- stream ordered, so
        several towers / micro-steps in flight each see their own value, and a captured graph sees a fresh one per replay."""
        self.step_seed += 1
        if self.seed_dev is None or self.seed_dev.device != self.device:
            self.seed_dev = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.seed_dev.fill_((self.seed * 1000003 + self.step_seed) & 0xFFFFFFFFFFFF)

    # ---- variables (tf.variable_scope / slim variables) ---------------------------------
    def full_name(self, leaf):
        return "/".join(self.scope + [leaf])

    def allocate_variables(self, specs, seed=1):
        """Create every variable of `specs` ([(name, shape)] in creation order) inside flat buckets."""
        dev = self.device
        total = sum(int(np.prod(s)) for _, s in specs)
        self.flat_param = torch.empty(total, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_m = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_v = torch.zeros(total, dtype=torch.float32, device=dev)
        self.vars = OrderedDict()
        self.var_grads = {}
        rng = np.random.default_rng(seed)
        host = np.empty(total, np.float32)
        off = 0
        for name, shape in specs:
            n = int(np.prod(shape))
            if name.endswith("weights"):     # slim default: xavier_initializer (uniform)
                lim = np.sqrt(6.0 / (shape[0] + shape[1]))
                host[off:off + n] = rng.uniform(-lim, lim, size=shape).astype(np.float32).reshape(-1)
            else:                            # BatchNorm beta: zeros
                host[off:off + n] = 0
            self.vars[name] = self.flat_param[off:off + n].view(*shape)
            self.var_grads[name] = self.flat_grad[off:off + n].view(*shape)
            off += n
        self.flat_param.copy_(torch.from_numpy(host))
        self.adam_t = 0

    def get_variable(self, leaf, shape):
        name = self.full_name(leaf)
        v = self.vars.get(name)
        if v is None:        # stand-alone use of an op outside trainval: create on first use
            dev = self.device
            if self._rng is None:
                self._rng = np.random.default_rng(self.seed)
            if leaf.endswith("weights"):
                lim = np.sqrt(6.0 / (shape[0] + shape[1]))
                host = self._rng.uniform(-lim, lim, size=shape).astype(np.float32)
            else:
                host = np.zeros(shape, np.float32)
            v = torch.from_numpy(host).to(dev)
            self.vars[name] = v
            self.var_grads[name] = torch.zeros_like(v)
        if tuple(v.shape) != tuple(shape):
            raise ValueError("variable %s has shape %s, requested %s" % (name, tuple(v.shape), tuple(shape)))
        return name, v

    def set_variable(self, name, array):
        self.vars[name].copy_(torch.as_tensor(np.ascontiguousarray(array, np.float32)).to(self.vars[name].device))

    # ---- gradient buffers ---------------------------------------------------------------
    def new_buffer(self, rows, cols):
        t = torch.empty((rows, cols), dtype=torch.float32, device=self.device)
        if self.recording:
            self.roots.append((t, [None]))
        return t

    def grad(self, v):
        """Gradient view matching the 2-D view `v` (same slice of its root's gradient) or None."""
        if not self.recording:
            return None
        ptr = v.data_ptr()
        for root, slot in self.roots:
            base = root.data_ptr()
            if base <= ptr < base + root.numel() * 4:
                if slot[0] is None:
                    slot[0] = self.zeros_like_small(root)
                off = (ptr - base) // 4
                ld = root.shape[1]
                r0, c0 = off // ld, off % ld
                assert H.ld2(v) == ld or v.shape[0] == 1, (v.shape, v.stride(), ld)
                return slot[0][r0:r0 + v.shape[0], c0:c0 + v.shape[1]]
        return None

    def tracked(self, v):
        """True when `v` lies inside a buffer whose gradient is being tracked (no allocation, unlike grad())."""
        if not self.recording:
            return False
        ptr = v.data_ptr()
        return any(root.data_ptr() <= ptr < root.data_ptr() + root.numel() * 4 for root, _ in self.roots)

    def grad_w(self, v):
        """(gradient view, beta) for a GEMM that adds into d(v): beta = 0.0 -- and the buffer is left
        uninitialised instead of zero-filled -- when this is the first touch and v IS its whole root
        (saves a memset and a read-modify-write pass over e.g. the 340 MB d(big) of FC0's dgrad)."""
        if not self.recording:
            return None, 1.0
        ptr = v.data_ptr()
        for root, slot in self.roots:
            if root.data_ptr() == ptr and tuple(root.shape) == tuple(v.shape) and slot[0] is None:
                slot[0] = torch.empty_like(root)
                return slot[0], 0.0
        return self.grad(v), 1.0

    def first_touch(self, v):
        """True when `v` IS a whole tracked root whose gradient nobody has touched yet (what grad_w answers with beta = 0.0)."""
        if not self.recording:
            return False
        ptr = v.data_ptr()
        return any(root.data_ptr() == ptr and tuple(root.shape) == tuple(v.shape) and slot[0] is None for root, slot in self.roots)

    def backward(self):
        flush_class_tail(self)
        self.join_side()                 # side work issued during the forward (transposed adjacency)
        for fn in reversed(self.tape):
            fn()
        self.join_side()                 # before the tape's tensors are released
        self.tape = []


_CTX = Context()


def ctx():
    return _CTX


def reset():
    """Forget all variables / state (tf.reset_default_graph analogue)."""
    global _CTX
    _CTX = Context()
    if H.stat_slots() != 32:
        H.set_stat_slots(32)                 # (the first step picks the count of its mode and shape)
    return _CTX


@contextlib.contextmanager
def variable_scope(name):
    c = ctx()
    c.scope.append(name)
    try:
        yield
    finally:
        c.scope.pop()


# ----------------------------------------------------------------------------------------------
# shape helpers
# ----------------------------------------------------------------------------------------------
def as2d(t):
    """(B,N,C) / (B,N,1,C) / (R,C) -> ((R,C) row-major view with stride (ld,1), B, N)."""
    H.require_gpu(t)
    H.f32(t)
    if t.dim() == 4:
        if t.shape[2] != 1:
            raise ValueError("rank-4 inputs must have a singleton axis -2, got %s" % (tuple(t.shape),))
        t = t[:, :, 0, :]
    if t.dim() == 2:
        if t.stride(1) != 1 and t.shape[1] != 1:
            t = t.contiguous()
        return t, 1, t.shape[0]
    if t.dim() != 3:
        raise ValueError("expected a rank 2/3/4 tensor, got rank %d" % t.dim())
    B, N, C = t.shape
    ok = (t.stride(2) == 1 or C == 1) and (B == 1 or t.stride(0) == N * t.stride(1)) and t.stride(1) >= C
    if not ok:
        t = t.contiguous()
    v = t.as_strided((B * N, C), (t.stride(1), 1), t.storage_offset())
    return v, B, N


def rank4(v, B, N):
    """(R,C) view -> (B,N,1,C) view (the rank the reference's ops return, ops.py:73)."""
    return v.as_strided((B, N, 1, v.shape[1]), (N * v.stride(0), v.stride(0), v.stride(0), 1), v.storage_offset())


# ----------------------------------------------------------------------------------------------
# thin kernel wrappers (2-D views in, explicit leading dimensions out)
# ----------------------------------------------------------------------------------------------
KNN_SEED = os.environ.get("DGCNN_KNN_SEED", "1") != "0"   # seed a layer's k-NN filter with the previous layer's graph (A/B switch)


class Segments(object):
    """A packed tower: nseg clouds of different sizes concatenated row-wise, cloud b = rows [offsets[b], offsets[b + 1]).  Holds the
    host offsets (validated here, before any device work), their device copy and the row -> cloud map row_group[r] = b (each made
    once, on the host, on first use) and the smallest / largest cloud, from which the k-NN picks its kernel forms.
    bn_per_cloud: every BatchNorm of the tower takes the statistics of the row's own cloud instead of all rows (csrc/seg_bn.hip;
    forward only) -- the mode travels with the `seg=` every pass already receives.
    bn_per_cloud_train: the same mode WITH its backward (a recording is allowed); implies bn_per_cloud.  Two settings, because the
    forward-only one keeps refusing a recording exactly as it did before the backward existed."""

    def __init__(self, offsets, rows=None, bn_per_cloud=False, bn_per_cloud_train=False):
        if isinstance(offsets, torch.Tensor):
            offsets = offsets.detach().cpu().numpy()
        off = np.asarray(offsets)
        if off.ndim != 1 or off.size < 2 or not np.issubdtype(off.dtype, np.integer):
            raise ValueError("offsets: expected nseg + 1 >= 2 integers, got %r" % (offsets,))
        off = off.astype(np.int64)
        sizes = np.diff(off)
        if off[0] != 0 or (sizes <= 0).any():
            raise ValueError("offsets must start at 0 and increase strictly (no empty cloud): %s" % (off.tolist(),))
        if rows is not None and off[-1] != rows:
            raise ValueError("offsets end at %d, the tower has %d rows" % (off[-1], rows))
        if off[-1] >= 1 << 31 or off.size - 1 > 65535:
            raise ValueError("a packed tower holds < 2^31 rows in at most 65535 clouds")
        self.host = off
        self.nseg = int(off.size - 1)
        self.rows = int(off[-1])
        self.min_n, self.max_n = int(sizes.min()), int(sizes.max())
        self._dev = None
        self._rg = None
        self._mix = {}
        self.bn_per_cloud_train = bool(bn_per_cloud_train)
        self.bn_per_cloud = bool(bn_per_cloud) or self.bn_per_cloud_train

    def check_k(self, k):
        if k <= 0 or k > self.min_n:
            raise ValueError("k_nn: k=%d must be in [1, smallest cloud=%d] (tf.nn.top_k raises otherwise)" % (k, self.min_n))

    def device(self, dev):
        if self._dev is None or self._dev.device != dev:
            self._dev = torch.from_numpy(self.host.astype(np.int32)).to(dev)
        return self._dev

    def mix(self, T, dev):
        """The tower's clouds in two classes for dgcnn_knn_seg_mix_f32: (list, n_grid, grid_max_n, scan_min_n, scan_max_n) -- list =
        int32[nseg] on the device, the clouds of at least T points (the grid class: n_grid of them, the largest grid_max_n) first, then
        the smaller ones (the scan class, scan_min_n ... scan_max_n points), each part ascending.  From the host offsets; made once
        per threshold.  An empty class: its numbers are 0."""
        T = int(T)
        m = self._mix.get(T)
        if m is None:
            sizes = np.diff(self.host)
            grid, scan = np.flatnonzero(sizes >= T), np.flatnonzero(sizes < T)
            lst = np.concatenate([grid, scan]).astype(np.int32)
            m = self._mix[T] = [lst, int(grid.size), int(sizes[grid].max()) if grid.size else 0,
                                int(sizes[scan].min()) if scan.size else 0, int(sizes[scan].max()) if scan.size else 0, None]
        if m[5] is None or m[5].device != dev:
            m[5] = torch.from_numpy(m[0]).to(dev)
        return m[5], m[1], m[2], m[3], m[4]

    def row_group(self, dev):
        """int32[rows] on the device: the cloud of every tower row (the per-cloud bias of FC0, tf.tile)."""
        if self._rg is None or self._rg.device != dev:
            rg = np.repeat(np.arange(self.nseg, dtype=np.int32), np.diff(self.host))
            self._rg = torch.from_numpy(rg).to(dev)
        return self._rg


def knn(x2d, B, N, k, seed=None, seg=None):
    """idx (B,N,k) of x2d (B*N, C).  seed: an earlier graph of the same clouds, (B,N,ks) int32 with ks >= k -- ks distinct candidates
    per row whose largest distance bounds the row's k-th distance from above (dgcnn_knn_seeded_f32); the result does not depend on it.
    seg: a packed tower (Segments; B = 1, N = rows): every row searches its own cloud, idx holds tower rows (dgcnn_knn_seg_f32, or
    dgcnn_knn_seg_grid_f32 for raw coordinates where dgcnn_knn_seg_grid_use picks the cell grid, or dgcnn_knn_seg_mix_f32 where
    dgcnn_knn_seg_mix_min_n splits the tower's clouds between the two)."""
    if seg is not None:
        return knn_packed(x2d, k, seg, seed=seed)
    C = x2d.shape[1]
    idx = torch.empty((B, N, k), dtype=torch.int32, device=x2d.device)
    ws, nws = _knn_workspace(x2d, "dgcnn_knn_workspace_bytes", B, N, C, k)   # knn.hip:KnnWorkspace
    Cp, kc = _knn_instance(C, k)
    seeded = _knn_seed_ok(seed, B, N, k)
    # bench.py's tag of the CALL: the kernels it launches (the library picks the form: knn.hip:knn_impl, knn_scan)
    tag = None
    if H.TIMER is not None:
        tag = "knn_call<C%d,k%d>[%s]" % (Cp, kc, "+".join(_knn_call_kernels(
            x2d, C, k, N, N, int(seed.shape[2]) if seeded else 0, dense=True)))
    if seeded:
        H.call("dgcnn_knn_seeded_f32", x2d.data_ptr(), B, N, C, H.ld2(x2d), k, seed.data_ptr(), int(seed.shape[2]), int(seed.shape[2]),
               idx.data_ptr(), ws.data_ptr(), nws, tag=tag, work=2.0 * B * N * N * C)
    else:
        H.call("dgcnn_knn_f32", x2d.data_ptr(), B, N, C, H.ld2(x2d), k, idx.data_ptr(), ws.data_ptr(), nws, tag=tag,
               work=2.0 * B * N * N * C)
    return idx


def _knn_switches():
    """The k-NN switches of the library as they stand (include/dgcnn_hip.h lists them); reading changes none."""
    return dict(valu=_knn_valu(), bf16f=H.switch("DGCNN_KNN_BF16F"), append=bool(H.switch("DGCNN_KNN_APPEND")),
                seed_min_n=H.switch("DGCNN_KNN_SEED_MIN_N"), hist=H.switch("DGCNN_KNN_HIST"))


def _knn_call_kernels(x2d, C, k, min_n, max_n, kseed, dense):
    """The kernels one dgcnn_knn_f32 / dgcnn_knn_seeded_f32 / dgcnn_knn_seg_f32 call launches with the workspace its *_workspace_bytes
    query sizes, in order, for bench.py's tags ("knn_grid_*": the two cell-grid kernels).  Only evaluated while a timer is set.
    kseed: the seeds per row the call passes (0: none).  dense: B clouds of min_n = max_n points; else a packed tower.
    tests/test_gpu_knn_dispatch.py holds every tag against the launches recorded from the same call.
    This restates knn.hip:knn_impl / knn_scan / launch_scan because the library has no host query that answers "which kernels would
    this call launch": its queries give the workspace size, the packed grid rule (dgcnn_knn_seg_grid_use) and each switch
    (dgcnn_switch_get: reading changes nothing), and those are what is asked here; the rest of the rule needs the call's pointer,
    leading dimension and seed, which only the entry sees.  The dense cell grid's smallest N is the switch DGCNN_KNN_GRID_MIN_N
    (unset: 4096; knn_grid.hip:knn_grid_min_n).  The names come from here only while a timer is set, never on the training path."""
    sw = _knn_switches()
    valu = sw["valu"]
    vec_ok = H.ld2(x2d) % 4 == 0 and x2d.data_ptr() % 16 == 0                  # knn.hip:knn_vec_ok
    names = [_sqnorm_name(C)]
    if _knn_big(k):                                                             # knn_scan: no bound, whatever the seed
        return names + ["knn_bigk_kernel"]
    append = sw["append"] and 16 < C <= 64 and C % 4 == 0 and k <= 64 and vec_ok and not valu and sw["bf16f"] != 0   # knn_append_usable
    in_range = max_n * H.ld2(x2d) < 2 ** 31
    if dense:                                                                   # knn_seeds_used_dense / knn_seeds_used_packed
        seed_min = sw["seed_min_n"] if sw["seed_min_n"] >= 0 else (0 if append else 4096)
        seeded = k <= kseed <= 64 and 4 < C <= 64 and C % 4 == 0 and vec_ok and not valu and min_n >= seed_min and in_range
        grid, grid_min_n = _knn_grid_mode(C, k), H.switch("DGCNN_KNN_GRID_MIN_N")
        if grid == 2 or (grid == 1 and max_n >= (4096 if grid_min_n == H.SWITCH_UNSET else grid_min_n)):
            if not valu:
                return names + ["knn_grid_*"]
    else:
        seeded = append and k <= kseed <= 64 and min_n >= max(sw["seed_min_n"], 0) and in_range
    bound = seeded and C in (16, 32, 64)                                        # knn.hip:launch_seed_bound takes these widths only
    if bound:
        names.append("knn_seed_bound_kernel")
    if bound and append:
        return names + ["knn_bf16a_kernel", "knn_select_kernel"]
    if _knn_wide(C):
        return names + ["knn_wide_kernel"]
    if C <= 4:
        hs = sw["hist"] if min_n >= 256 else 0                                  # knn.hip:launch_hist_bound
        return names + (["knn_hist_bound_kernel"] if hs and not valu and min_n >= 4 * k * hs else []) + ["knn_kernel"]
    if dense and C <= 64 and not valu:                                          # knn.hip:launch_scan
        if 16 < C and C % 4 == 0 and vec_ok and (sw["bf16f"] == 1 or (sw["bf16f"] == 2 and (max_n >= 8192 or bound))):
            return names + ["knn_bf16f_kernel"]
        return names + ["knn_mfma_kernel"]
    return names + ["knn_kernel"]


def _knn_valu():
    """dgcnn_knn_force_valu as it stands"""
    return bool(H.switch("DGCNN_KNN_FORCE_VALU"))


def _knn_big(k):
    """the library gives this k to the large-k scan (knn_bigk.hip; knn.hip:knn_bigk_takes): k > 64 always, smaller k from
    dgcnn_knn_big_k_min on unless the VALU scan is forced"""
    return k >= 65 or (k >= H.switch("DGCNN_KNN_BIG_K_MIN") and not _knn_valu())


def _sqnorm_name(C):
    return "sqnorm_wide_kernel" if C > 128 else "sqnorm_kernel"


def _knn_wide(C):
    """the library gives this width to the channel-slab scan (knn_wide.hip; knn.hip:knn_wide_takes): C > 128 always, narrower rows
    from dgcnn_knn_wide_min_c on unless the VALU scan is forced"""
    return C >= 129 or (C >= H.switch("DGCNN_KNN_WIDE_MIN_C") and not _knn_valu())


def _knn_instance(C, k):
    """(CP, KC) of the scan kernel a shape instantiates (knn.hip:knn_scan, launch_scan_k), for bench.py's tags; CP = the channels
    rounded up to whole slabs of 64 where the channel-slab scan or the large-k scan takes the shape (their kernels have no CP
    parameter); KC = 128 or 256 is the large-k scan's KP (half its row buffer)"""
    if _knn_big(k):
        return (C + 63) // 64 * 64, 128 if k <= 128 else 256
    kc = 8 if k <= 8 else 20 if k <= 20 else 40 if k <= 40 else 64
    if C > 4 and _knn_wide(C):
        return (C + 63) // 64 * 64, kc
    return (4 if C <= 4 else 16 if C <= 16 else 64 if C <= 64 else 128), kc


def _knn_workspace(x2d, query, *shape):
    """(uint8 tensor, its size): the workspace whose size the library's `query`(*shape) asks for"""
    nws = int(getattr(H.load(), query)(*shape))
    return torch.empty((nws,), dtype=torch.uint8, device=x2d.device), nws


def _knn_seed_ok(seed, B, N, k):
    """seed is a usable earlier graph of these clouds: (B, N, >= k) contiguous int32, and seeding is switched on"""
    return (KNN_SEED and seed is not None and seed.dim() == 3 and seed.shape[0] == B and seed.shape[1] == N and seed.shape[2] >= k
            and seed.dtype == torch.int32 and seed.is_contiguous())


def _knn_grid_mode(C, k):
    """dgcnn_knn_grid's mode for this shape (knn_grid.hip:knn_grid_applicable): 0 = never (switched off, or C > 4 or k > 40),
    2 = whenever applicable, 1 = where the library's rule says it pays."""
    return H.switch("DGCNN_KNN_GRID") if C <= 4 and k <= 40 else 0


def knn_packed(x2d, k, seg, seed=None):
    """idx (1,R,k) of the packed tower x2d (R, C): per cloud the dense k_nn of that cloud, as tower rows."""
    R, C = x2d.shape
    if R != seg.rows:
        raise ValueError("offsets end at %d, the tower has %d rows" % (seg.rows, R))
    seg.check_k(k)
    off = seg.device(x2d.device)
    idx = torch.empty((1, R, k), dtype=torch.int32, device=x2d.device)
    n = seg.host[1:] - seg.host[:-1]
    Cp, kc = _knn_instance(C, k)
    # raw coordinates: the cell grid, one per cloud, where the library's rule picks it (the same indices; a seed is not needed).  Mode 1
    # with a per-cloud threshold T > 0: the clouds of at least T points through the grid, the others through the scan, in one call
    lib = H.load()
    big = _knn_big(k)                        # the large-k scan: dgcnn_knn_seg_f32 whatever the width
    T = H.switch("DGCNN_KNN_MIX_MIN_N") if C <= 4 and not big and _knn_grid_mode(C, k) == 1 else 0
    if T > 0:
        lst, n_grid, grid_max, scan_min, scan_max = seg.mix(T, x2d.device)
        use_grid = n_grid == seg.nseg
        if 0 < n_grid < seg.nseg:
            ws, nws = _knn_workspace(x2d, "dgcnn_knn_seg_mix_workspace_bytes", R, n_grid)
            H.call("dgcnn_knn_seg_mix_f32", x2d.data_ptr(), H.ld2(x2d), C, k, seg.nseg, off.data_ptr(), R, lst.data_ptr(), n_grid, grid_max,
                   scan_min, scan_max, idx.data_ptr(), ws.data_ptr(), nws,
                   tag=None if H.TIMER is None else "knn_seg_call<C4,k%d>[sqnorm_kernel+knn_grid_*+%s]" % (
                       kc, "+".join(_knn_call_kernels(x2d, C, k, scan_min, scan_max, 0, dense=False)[1:])),
                   work=2.0 * float((n * n).sum()) * C)
            return idx
    else:
        use_grid = C <= 4 and not big and lib.dgcnn_knn_seg_grid_use(C, k, seg.nseg, R, seg.min_n, seg.max_n, int((n * n).sum()))
    if use_grid:
        ws, nws = _knn_workspace(x2d, "dgcnn_knn_seg_grid_workspace_bytes", R, seg.nseg)
        H.call("dgcnn_knn_seg_grid_f32", x2d.data_ptr(), H.ld2(x2d), C, k, seg.nseg, off.data_ptr(), R, seg.min_n, seg.max_n,
               idx.data_ptr(), ws.data_ptr(), nws, tag="knn_seg_call<C4,k%d>[sqnorm_kernel+knn_grid_*]" % kc,
               work=2.0 * float((n * n).sum()) * C)
        return idx
    ws, nws = _knn_workspace(x2d, "dgcnn_knn_seg_workspace_bytes", R, seg.max_n, C, k)
    seeded = _knn_seed_ok(seed, 1, R, k)
    tag = None
    if H.TIMER is not None:
        tag = "knn_seg_call<C%d,k%d>[%s]" % (Cp, kc, "+".join(_knn_call_kernels(
            x2d, C, k, seg.min_n, seg.max_n, int(seed.shape[2]) if seeded else 0, dense=False)))
    H.call("dgcnn_knn_seg_f32", x2d.data_ptr(), H.ld2(x2d), C, k, seg.nseg, off.data_ptr(), R, seg.min_n, seg.max_n,
           seed.data_ptr() if seeded else None, int(seed.shape[2]) if seeded else 0, int(seed.shape[2]) if seeded else 0,
           idx.data_ptr(), ws.data_ptr(), nws, tag=tag, work=2.0 * float((n * n).sum()) * C)
    return idx


KNN_CROSS_MAX_K = 64                         # knn_cross.hip: the large-k scan searches a cloud against itself only


def knn_cross(q2d, p2d, B, M, N, k, qseg=None, pseg=None, want_dist=False):
    """k-NN between two point sets (dgcnn_knn_cross_f32): idx (B,M,k) int32 -- for every row of q2d (B*M, C) the k nearest rows of
    p2d (B*N, C) of the same cloud, cloud-local j; with want_dist also dist (B,M,k) float32, the selected D~ in the same order.
    qseg / pseg (both or neither): packed towers (Segments; B = 1, M / N = the towers' rows) of the same number of clouds: query
    cloud b searches candidate cloud b, idx holds rows of the candidate tower.  Returns idx or (idx, dist)."""
    C = q2d.shape[1]
    if p2d.shape[1] != C:
        raise ValueError("knn_cross: queries have %d channels, points %d" % (C, p2d.shape[1]))
    if (qseg is None) != (pseg is None):
        raise ValueError("knn_cross: both towers packed (qseg and pseg) or neither")
    if k > KNN_CROSS_MAX_K:
        raise ValueError("knn_cross: k=%d > %d: the search between two sets keeps at most %d neighbours" % (k, KNN_CROSS_MAX_K,
                                                                                                       KNN_CROSS_MAX_K))
    if qseg is not None:
        if qseg.nseg != pseg.nseg:
            raise ValueError("knn_cross: %d query clouds, %d candidate clouds" % (qseg.nseg, pseg.nseg))
        if q2d.shape[0] != qseg.rows or p2d.shape[0] != pseg.rows:
            raise ValueError("knn_cross: offsets end at %d / %d, the towers have %d / %d rows" % (qseg.rows, pseg.rows, q2d.shape[0],
                                                                                                p2d.shape[0]))
        pseg.check_k(k)
        nseg, q_rows, p_rows, max_m, min_n, max_n = qseg.nseg, qseg.rows, pseg.rows, qseg.max_n, pseg.min_n, pseg.max_n
        qo, po = qseg.device(q2d.device), pseg.device(p2d.device)
        pairs = float((np.diff(qseg.host) * np.diff(pseg.host)).sum())
    else:
        if k <= 0 or k > N:
            raise ValueError("knn_cross: k=%d must be in [1, N=%d]" % (k, N))
        nseg, q_rows, p_rows, max_m, min_n, max_n = B, B * M, B * N, M, N, N
        qo = po = None
        pairs = float(B) * M * N
    idx = torch.empty((B, M, k), dtype=torch.int32, device=q2d.device)
    dist = torch.empty((B, M, k), dtype=torch.float32, device=q2d.device) if want_dist else None
    ws, nws = _knn_workspace(q2d, "dgcnn_knn_cross_workspace_bytes", q_rows, p_rows)
    kc = 8 if k <= 8 else 20 if k <= 20 else 40 if k <= 40 else 64
    Cp = 16 if C <= 16 else (C + 63) // 64 * 64                  # channels rounded up to whole slabs (16 or 64 wide)
    # one set of rows under one map on both sides: the library computes its norms once (knn_cross.hip)
    same = (q2d.data_ptr() == p2d.data_ptr() and H.ld2(q2d) == H.ld2(p2d) and q_rows == p_rows and
            (max_m == max_n if qo is None else qo.data_ptr() == po.data_ptr()))
    tag = "knn_cross_call<C%d,k%d>[%s+knn_cross_kernel]" % (Cp, kc, "+".join([_sqnorm_name(C)] * (1 if same else 2)))
    H.call("dgcnn_knn_cross_f32", q2d.data_ptr(), H.ld2(q2d), p2d.data_ptr(), H.ld2(p2d), C, k, nseg, H._p(qo), H._p(po), q_rows, p_rows,
           max_m, min_n, max_n, idx.data_ptr(), H._p(dist), ws.data_ptr(), nws, tag=tag, work=2.0 * pairs * C)
    return (idx, dist) if want_dist else idx


INTERP_MAX_K = KNN_CROSS_MAX_K               # interp.hip reads what the search between two sets returns
INTERP_MIN_EPS = 1e-30                       # k / eps must not overflow


def check_interp_eps(eps):
    eps = float(eps)
    if not (INTERP_MIN_EPS <= eps < float("inf")):
        raise ValueError("interpolate: eps=%r must be finite and at least %g" % (eps, INTERP_MIN_EPS))
    return eps


def interpolate(f2d, idx, dist, B, M, N, k, packed, eps, out=None):
    """Feature interpolation between two point sets (dgcnn_interp_f32, include/dgcnn_hip.h K6): y (B*M, F) -- every query row the
    inverse-distance-weighted mean of the rows of f2d (B*N, F) that idx (B,M,k) int32 names, weights from dist (B,M,k) float32,
    both as knn_cross returns them.  packed: B = 1, M / N = the towers' rows and idx holds rows of the candidate tower.
    out: a 2-D (B*M, F) view with its own leading dimension (a column slice of a wider buffer) to write into.
    Recorded: d(f2d) += the weighted sums over the transposed graph (dgcnn_interp_bwd_f32: fixed order, no float atomics); the
    coordinates and the weights get no gradient."""
    c = ctx()
    eps = check_interp_eps(eps)
    p_rows, F = f2d.shape
    q_rows = B * M
    if p_rows != B * N:
        raise ValueError("interpolate: features have %d rows, the candidate set %d" % (p_rows, B * N))
    if not 1 <= k <= INTERP_MAX_K:
        raise ValueError("interpolate: k=%d must be in [1, %d]" % (k, INTERP_MAX_K))
    if F % 4 or F > 1024 or F <= 0:
        raise ValueError("interpolate: features need F %% 4 == 0 and F <= 1024, got F=%d" % F)
    if tuple(idx.shape) != (B, M, k) or tuple(dist.shape) != (B, M, k):
        raise ValueError("interpolate: graph must be idx, dist of shape %s, got %s and %s" % ((B, M, k), tuple(idx.shape),
                                                                                           tuple(dist.shape)))
    if idx.dtype != torch.int32 or dist.dtype != torch.float32:
        raise TypeError("interpolate: graph must be (int32 idx, float32 dist), got %s and %s" % (idx.dtype, dist.dtype))
    H.require_gpu(f2d, idx, dist, out)
    idx, dist = idx.contiguous(), dist.contiguous()
    y = c.new_buffer(q_rows, F) if out is None else out
    if tuple(y.shape) != (q_rows, F):
        raise ValueError("interpolate: out must be %s, got %s" % ((q_rows, F), tuple(y.shape)))
    a = torch.empty((q_rows, k), dtype=torch.float32, device=f2d.device) if c.recording else None
    Md, Nd = (0, 0) if packed else (M, N)
    edges = float(q_rows) * k
    H.call("dgcnn_interp_f32", f2d.data_ptr(), H.ld2(f2d), idx.data_ptr(), dist.data_ptr(), q_rows, p_rows, Md, Nd, k, F, eps,
           H._p(a), y.data_ptr(), H.ld2(y), tag="interp_fwd_kernel", work=4.0 * (edges * F + q_rows * F + 2 * edges),
           nbytes=4.0 * (float(p_rows) * F + q_rows * F + 2 * edges))
    if c.recording:
        def bwd():
            dy, df = c.grad(y), c.grad(f2d)
            if dy is None or df is None:
                return
            ws, nws = _knn_workspace(f2d, "dgcnn_interp_bwd_workspace_bytes", q_rows, p_rows, k)
            H.call("dgcnn_interp_bwd_f32", dy.data_ptr(), H.ld2(dy), idx.data_ptr(), a.data_ptr(), q_rows, p_rows, Md, Nd, k, F,
                   df.data_ptr(), H.ld2(df), 1, ws.data_ptr(), nws,
                   tag="interp_bwd[count+scan+fill+rank+interp_bwd_gather_kernel]",
                   work=4.0 * (edges * F + 2 * float(p_rows) * F + 6 * edges),
                   nbytes=4.0 * (q_rows * F + 2 * float(p_rows) * F + 2 * edges))
        c.tape.append(bwd)
    return y


FPS_MAX_C = 64                               # fps.hip: sampling runs on coordinates or narrow feature rows


def fps(x2d, B, N, m, seg=None, sseg=None, start=None, want_dist=False):
    """Farthest point sampling (dgcnn_fps_f32, include/dgcnn_hip.h K7).  Dense: x2d (B*N, C), m samples per cloud -> idx (B, m) int32,
    cloud-local.  Packed (seg and sseg, both Segments of the same number of clouds; B = 1, N = the tower's rows): cloud b is sampled
    sseg's b-th size times -> idx (sseg.rows,) int32, rows of the tower.  start: None or a host sequence of one cloud-local row per
    cloud.  Returns idx or (idx, dist).  A selection: nothing is recorded."""
    C = x2d.shape[1]
    if C > FPS_MAX_C or C < 1:
        raise ValueError("farthest_point_sample: C=%d channels, the sampling takes 1 ... %d" % (C, FPS_MAX_C))
    if (seg is None) != (sseg is None):
        raise ValueError("farthest_point_sample: both offsets (rows and samples) or neither")
    if seg is not None:
        sizes, counts = np.diff(seg.host), np.diff(sseg.host)
        if seg.nseg != sseg.nseg or x2d.shape[0] != seg.rows:
            raise ValueError("farthest_point_sample: %d clouds of rows (%d rows, the tower has %d), %d clouds of samples"
                             % (seg.nseg, seg.rows, x2d.shape[0], sseg.nseg))
        if (counts > sizes).any():
            b = int(np.flatnonzero(counts > sizes)[0])
            raise ValueError("farthest_point_sample: m=%d exceeds the %d rows of cloud %d" % (counts[b], sizes[b], b))
        nseg, rows, samples, max_n, max_m = seg.nseg, seg.rows, sseg.rows, seg.max_n, sseg.max_n
        steps = float((sizes * counts).sum())
    else:
        if x2d.shape[0] != B * N:
            raise ValueError("farthest_point_sample: %d rows, expected B * N = %d" % (x2d.shape[0], B * N))
        if m < 1 or m > N:
            raise ValueError("farthest_point_sample: m=%d must be in [1, N=%d]" % (m, N))
        nseg, rows, samples, max_n, max_m = B, B * N, B * m, N, m
        sizes = np.full(B, N)
        steps = float(B) * N * m
    if start is not None:
        start = np.asarray(start, np.int64).reshape(-1)
        if start.size != nseg or (start < 0).any() or (start >= sizes).any():
            raise ValueError("farthest_point_sample: start must hold one row inside each of the %d clouds, got %s" % (nseg, start.tolist()))
    H.require_gpu(x2d)
    dev = x2d.device
    idx = torch.empty((samples,) if seg is not None else (B, m), dtype=torch.int32, device=dev)
    dist = torch.empty(tuple(idx.shape), dtype=torch.float32, device=dev) if want_dist else None
    st = None if start is None else torch.from_numpy(start.astype(np.int32)).to(dev)
    ws, nws = _knn_workspace(x2d, "dgcnn_fps_workspace_bytes", rows, C, max_n)
    res = int(H.load().dgcnn_fps_resident_max_n(C))
    tag = "fps[%s]" % "+".join((["fps_resident_kernel<C%d>" % C] if res and (seg is not None or max_n <= res) else []) + (["fps_stream_kernel"] if max_n > res else []))
    H.call("dgcnn_fps_f32", x2d.data_ptr(), H.ld2(x2d), C, nseg, H._p(None if seg is None else seg.device(dev)),
           H._p(None if sseg is None else sseg.device(dev)), rows, samples, max_n, max_m, H._p(st), idx.data_ptr(), H._p(dist),
           ws.data_ptr() if nws else 0, nws, tag=tag, work=3.0 * C * steps)
    return (idx, dist) if want_dist else idx


def take_rows(x2d, idx, B, M, N, packed):
    """y (s_rows, F) = the rows of x2d that idx names (dgcnn_rows_gather_f32): dense -- x2d (B*N, F), idx (B, M) int32 cloud-local;
    packed -- x2d (N, F) with B = 1, idx (M,) int32 tower rows.  idx must hold DISTINCT rows per cloud (farthest point sampling
    guarantees it).  Recorded: d(x2d) receives the scatter of d(y) (dgcnn_rows_scatter_f32; beta = 0 on a gradient buffer nobody has
    touched, which the scatter then fills whole, else beta = 1)."""
    c = ctx()
    x_rows, F = x2d.shape
    s_rows = B * M
    if x_rows != B * N:
        raise ValueError("take_rows: x has %d rows, expected %d" % (x_rows, B * N))
    if idx.dtype != torch.int32:
        raise TypeError("take_rows: idx must be int32 (what farthest_point_sample returns), got %s" % idx.dtype)
    if idx.numel() != s_rows:
        raise ValueError("take_rows: idx holds %d rows, expected %d" % (idx.numel(), s_rows))
    H.require_gpu(x2d, idx)
    idx = idx.contiguous()
    Md, Nd = (0, 0) if packed else (M, N)
    y = c.new_buffer(s_rows, F)
    moved = 8.0 * s_rows * F
    H.call("dgcnn_rows_gather_f32", x2d.data_ptr(), H.ld2(x2d), idx.data_ptr(), s_rows, x_rows, Md, Nd, F, y.data_ptr(), H.ld2(y),
           tag="rows_gather_kernel", work=moved, nbytes=moved)
    if c.recording:
        def bwd():
            dy = c.grad(y)
            if dy is None or not c.tracked(x2d):
                return
            dx, beta = c.grad_w(x2d)
            H.call("dgcnn_rows_scatter_f32", dy.data_ptr(), H.ld2(dy), idx.data_ptr(), s_rows, x_rows, Md, Nd, F, dx.data_ptr(),
                   H.ld2(dx), int(beta), tag="rows_scatter_kernel", work=moved, nbytes=moved)
        c.tape.append(bwd)
    return y


def _tile_m(M, N):
    """Mirror of gemm.hip:tile_m (only used to name the kernel instance in bench.py's roofline tags)."""
    return 128


def _gemm_tag(M, N, K, transA, transB, A, Bm, colmax_rpg=0, C_out=None, has_bias=False, has_stats=False):
    """Kernel identity of a dgcnn_gemm_f32 launch for bench.py's table (mirrors the C dispatch); None when nobody is timing.  The tag
    names the kernel that forms the product; a split reduction adds reduce_partials_kernel to the call without changing the tag.
    tests/test_gpu_gemm_dispatch.py holds every tag against the launches recorded from the same call."""
    if H.TIMER is None:
        return None
    lda, ldb = H.ld2(A), H.ld2(Bm)
    # the streaming kernels of the class dimension (gemm.hip:gemm_f32_impl, ahead of every tile kernel); the engine always passes a
    # workspace, whose size the transA form also checks (512 partial products at most)
    if N <= 4 and lda % 4 == 0 and A.data_ptr() % 16 == 0:
        if not transA and not transB and K % 4 == 0 and K <= 4096 and not has_bias:
            return "gemm_call[skinny_nn_kernel<%d>]" % N
        if transA and M % 4 == 0 and M <= 4096 and not has_bias and not has_stats and ctx().workspace().numel() >= min(-(-K // 64), 512) * M * N * 4:
            return "gemm_call[skinny_tn_kernel<%d>+reduce_partials_kernel]" % N
    if transB and K <= 4 and N % 4 == 0 and not has_bias and not has_stats and C_out is not None and \
            H.ld2(C_out) % 4 == 0 and C_out.data_ptr() % 16 == 0:
        return "gemm_call[skinny_nt_kernel<%d>]" % K
    vec = (lda % 4 == 0 and ldb % 4 == 0 and A.data_ptr() % 16 == 0 and Bm.data_ptr() % 16 == 0 and
           ((M if transA else K) % 4 == 0) and ((K if transB else N) % 4 == 0))
    arith = H.gemm_arith()
    cd = lambda a, b: -(-a // b)
    small = cd(M, 128) * cd(N, 128) * cd(K, 256) < 256       # gemm.hip:tile_n
    bn = 64 if (N <= 64 or small) else 128
    if vec and arith:
        kinds = ("KSTRIDED" if transA else "KCONTIG", "KCONTIG" if transB else "KSTRIDED")
        rows = H.load().dgcnn_gemm_x3_tile_rows(M, N, K)
        if colmax_rpg and colmax_rpg % rows:                      # gemm.hip:launch<>: no tile may straddle two groups
            rows = 256
        if H.load().dgcnn_gemm_x3_tile_cols(M, N, K) == 256:     # dg::x3_tile_n: the 256-column unspecialised kernels
            return "gemm_x3q_kernel<%s,%s,%d,bf16x%d>" % (kinds + (rows, arith))
        if rows == 256:                                           # dg::x3_tile_m: the 256 x 128 wave-specialised kernel
            return "gemm_x3w2_kernel<%s,%s,bf16x%d>" % (kinds + (arith,))
        return "gemm_x3_kernel<%s,%s,%d,bf16x%d>" % (kinds + (bn, arith))
    return "gemm_kernel<%s,%s,STORE,%d,%d>" % ("A_COL" if transA else "A_ROW", "B_COL" if transB else "B_ROW", _tile_m(M, N), bn)


def gemm(A, Bm, C, transA=False, transB=False, beta=0.0, gbias=None, rpg=0, stats=None, arith=None, colmax=None, colmax_rpg=0,
         row_group=None):
    """C (+)= op(A) op(B); shapes are those of the stored matrices.  arith: arithmetic of THIS product (None = the
    process-wide setting; 1 = plain bf16 operands: measurements only, not fp32 class).
    row_group: int32[M] row -> cloud map of a packed tower: the bias row of output row r is gbias[row_group[r]] (dgcnn_gemm_seg_f32;
    no colmax -- a row tile may straddle clouds)."""
    if arith is not None and arith != H.gemm_arith():
        prev = H.gemm_arith()
        H.set_gemm_arith(arith)
        try:
            if row_group is not None:
                return gemm(A, Bm, C, transA, transB, beta, gbias, rpg, stats, None, colmax, colmax_rpg, row_group=row_group)
            return gemm(A, Bm, C, transA, transB, beta, gbias, rpg, stats, None, colmax, colmax_rpg)
        finally:
            H.set_gemm_arith(prev)
    M = A.shape[1] if transA else A.shape[0]
    K = A.shape[0] if transA else A.shape[1]
    N = Bm.shape[0] if transB else Bm.shape[1]
    Kb = Bm.shape[1] if transB else Bm.shape[0]
    assert K == Kb and tuple(C.shape) == (M, N), (A.shape, Bm.shape, C.shape, transA, transB)
    ws = ctx().workspace()
    tag = _gemm_tag(M, N, K, transA, transB, A, Bm, colmax_rpg if colmax is not None else 0, C_out=C, has_bias=gbias is not None,
                    has_stats=stats is not None)
    if row_group is not None:
        if colmax is not None:
            raise ValueError("gemm: the column-maximum epilogue does not take a packed tower")
        if row_group.dtype != torch.int32 or row_group.numel() != M or not row_group.is_contiguous():
            raise ValueError("gemm: row_group must be a contiguous int32[%d]" % M)
        H.call("dgcnn_gemm_seg_f32", int(transA), int(transB), M, N, K, A.data_ptr(), H.ld2(A), Bm.data_ptr(), H.ld2(Bm),
               C.data_ptr(), H.ld2(C), float(beta), H._p(gbias), 0 if gbias is None else H.ld2(gbias), row_group.data_ptr(),
               H._p(stats), ws.data_ptr(), ws.numel(), tag=tag, work=2.0 * M * N * K,
               nbytes=4.0 * (M * K + K * N + (2 if beta != 0.0 else 1) * M * N))
        return
    H.call("dgcnn_gemm_f32", int(transA), int(transB), M, N, K, A.data_ptr(), H.ld2(A), Bm.data_ptr(), H.ld2(Bm),
           C.data_ptr(), H.ld2(C), float(beta), H._p(gbias), 0 if gbias is None else H.ld2(gbias), int(rpg),
           H._p(stats), H._p(colmax), int(colmax_rpg), ws.data_ptr(), ws.numel(), tag=tag, work=2.0 * M * N * K,
           nbytes=4.0 * (M * K + K * N + (2 if beta != 0.0 else 1) * M * N))


def colstats_det(T, st):
    """Fixed-order BatchNorm column sums of the materialised (R,F) tensor T into slot 0 of `st` (deterministic mode)."""
    ws = ctx().workspace()
    H.call("dgcnn_colstats_det_f32", T.data_ptr(), T.shape[0], T.shape[1], H.ld2(T), st.data_ptr(), ws.data_ptr(), ws.numel())


def k1_reduce_fixed_order(Y, k, F, mean, rstd, beta, dmx, dmn, mx):
    """The k = 1 BatchNorm-backward reduce kernel (float4 channels, column-fixed threads) sums in a fixed order by itself."""
    return (k == 1 and F % 4 == 0 and mx is None and Y.data_ptr() % 16 == 0 and dmx.data_ptr() % 16 == 0 and H.ld2(dmx) % 4 == 0 and
            mean.data_ptr() % 16 == 0 and rstd.data_ptr() % 16 == 0 and beta.data_ptr() % 16 == 0 and
            (dmn is None or (dmn.data_ptr() % 16 == 0 and H.ld2(dmn) % 4 == 0)))


def bn_bwd_reduce(Y, R, k, F, mean, rstd, beta, relu, dmx, dmn, mx, cnt, red, tag, work):
    """sum dZ / sum dZ*xhat of a materialised Y.  DETERMINISTIC: the column-fixed k = 1 kernel (float4 channels) reduces in a fixed
    order by itself; every other shape (the class dimension, materialised edge tensors) takes the fixed-order twin of det.hip."""
    k1 = k1_reduce_fixed_order(Y, k, F, mean, rstd, beta, dmx, dmn, mx)
    if DETERMINISTIC and not k1:
        ws = ctx().workspace()
        H.call("dgcnn_bn_bwd_reduce_det_f32", Y.data_ptr(), R, k, F, mean.data_ptr(), rstd.data_ptr(), beta.data_ptr(), int(relu),
               dmx.data_ptr(), H.ld2(dmx), H._p(dmn), 0 if dmn is None else H.ld2(dmn), H._p(mx), 0 if mx is None else H.ld2(mx),
               H._p(cnt), red.data_ptr(), ws.data_ptr(), ws.numel())
    else:
        H.call("dgcnn_bn_bwd_reduce_f32", Y.data_ptr(), R, k, F, mean.data_ptr(), rstd.data_ptr(), beta.data_ptr(), int(relu),
               dmx.data_ptr(), H.ld2(dmx), H._p(dmn), 0 if dmn is None else H.ld2(dmn), H._p(mx), 0 if mx is None else H.ld2(mx),
               H._p(cnt), red.data_ptr(), tag=tag, work=work)


def seg_colsum(x, seg, out):
    """out (nseg, F) <- the column sums of every cloud of the packed tower x (rows, F): tf.tile^T, summed in a fixed order."""
    R, F = x.shape
    ws = ctx().workspace()
    H.call("dgcnn_seg_colsum_f32", x.data_ptr(), H.ld2(x), R, F, seg.device(x.device).data_ptr(), seg.nseg, out.data_ptr(),
           ws.data_ptr(), ws.numel(), tag="seg_colsum_kernel", work=4.0 * R * F)
    return out


def per_cloud(seg):
    """True when `seg` is a packed tower whose BatchNorm runs per cloud.  Without seg.bn_per_cloud_train the mode is forward only:
    inside a recording it raises here, on the host, before anything is launched."""
    if seg is None or not seg.bn_per_cloud:
        return False
    if ctx().recording and not seg.bn_per_cloud_train:
        raise NotImplementedError("per-cloud BatchNorm has no backward yet")
    return True


def seg_stats_workspace(R, nseg, F, dev):
    """Scratch of the two-stage per-cloud sums: the context's workspace, or a temporary where that is too small."""
    need = int(H.load().dgcnn_seg_stats_workspace_bytes(R, nseg, F))
    ws = ctx().workspace()
    if ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    return ws


def seg_bn_finalize(stats, seg, F, k):
    """(mean, rstd), each (nseg, F): cloud b from its own sums and the count n_b * k."""
    dev = stats.device
    mr = torch.empty((2, seg.nseg, F), dtype=torch.float32, device=dev)
    H.call("dgcnn_seg_bn_finalize_f32", stats.data_ptr(), seg.nseg, F, seg.device(dev).data_ptr(), int(k), BN_EPS,
           mr[0].data_ptr(), mr[1].data_ptr())
    return mr[0], mr[1]


def seg_bn_bwd_finalize(red, seg, F, k, dbeta):
    """(c1, c2), each (nseg, F): cloud b's sums over its count n_b * k; dbeta += the sum of red0 over the clouds."""
    dev = red.device
    cc = torch.empty((2, seg.nseg, F), dtype=torch.float32, device=dev)
    H.call("dgcnn_seg_bn_bwd_finalize_f32", red.data_ptr(), seg.nseg, F, seg.device(dev).data_ptr(), int(k), cc[0].data_ptr(),
           cc[1].data_ptr(), dbeta.data_ptr(), 1.0)
    return cc[0], cc[1]


def bn_finalize(stats, F, count):
    dev = stats.device
    mr = torch.empty((2, F), dtype=torch.float32, device=dev)
    H.call("dgcnn_bn_finalize_f32", stats.data_ptr(), F, float(count), BN_EPS, mr[0].data_ptr(), mr[1].data_ptr())
    return mr[0], mr[1]


def _launch_bn1_act_dropout(h):
    """The last FC layer's BatchNorm + activation + dropout pass on its own (h: the record conv_bn_act holds it back in)."""
    H.call("dgcnn_bn1_act_dropout_f32", h["T"].data_ptr(), h["R"], h["F"], h["mean"].data_ptr(), h["rstd"].data_ptr(),
           h["beta"].data_ptr(), int(h["relu"]), float(h["keep"]), h["seed"].data_ptr(), h["out"].data_ptr(), H.ld2(h["out"]),
           tag="bn_act_kreduce_kernel<k=1>", work=4.0 * h["R"] * h["F"] * 2)


def _launch_loss_tail(lt):
    """The Final layer's BatchNorm finalize + activation on their own (lt: the record conv_bn_act holds them back in)."""
    prev = H.stat_slots()
    if lt["nslots"] != prev:
        H.set_stat_slots(lt["nslots"])
    try:
        H.call("dgcnn_bn_finalize_f32", lt["st"].data_ptr(), lt["F"], float(lt["R"]), BN_EPS, lt["mean"].data_ptr(), lt["rstd"].data_ptr())
    finally:
        if lt["nslots"] != prev:
            H.set_stat_slots(prev)
    H.call("dgcnn_bn_act_kreduce_f32", lt["T"].data_ptr(), lt["R"], 1, lt["F"], lt["mean"].data_ptr(), lt["rstd"].data_ptr(),
           lt["beta"].data_ptr(), int(lt["relu"]), lt["out"].data_ptr(), H.ld2(lt["out"]), 0, 0, 0, 0, 0,
           tag="bn_act_kreduce_kernel<k=1>", work=4.0 * lt["R"] * lt["F"] * 2)


def flush_class_tail(c):
    """Issue whatever the class-dimension tail still holds back (its consumer did not come)."""
    tail, c.class_tail = c.class_tail, None
    if tail is not None:
        _launch_bn1_act_dropout(tail)
    lt, c.loss_tail = c.loss_tail, None
    if lt is not None:
        _launch_loss_tail(lt)


# ----------------------------------------------------------------------------------------------
# slim.conv2d(1x1, no bias) + slim.batch_norm + activation on per-point tensors (k = 1)
# dgcnn/ops.py:62-70,125-133,153-160 ; dgcnn/model.py:46-53,65-72,94-101
# ----------------------------------------------------------------------------------------------
def conv_bn_act(x, leaf_scope, num_outputs, relu=True, out=None, out2=None, gbias=None, rpg=0, w_rows=None, arith=None,
                plane_out=None, f32_out=True, gmax=None, drop_keep=None, seg=None, class_tail=None):
    """x: (R,Cin) view.  Variables `<scope>/weights` [Cin(+extra), Cout], `<scope>/BatchNorm/beta`.
    w_rows: (lo, hi) row range of the weight that multiplies x (FC0 with the folded global feature).
    Returns the (R,Cout) output (a fresh tracked buffer unless `out` is given).
    Plane mode (HEAD_PLANES, planes_ok): the products run on the plane GEMM; plane_out = PlaneSet view that receives the
    activated output as operand planes of the NEXT product (f32_out = False: the fp32 `out` is then never written -- it only
    names the tensor and carries its gradient); gmax = (B, N): also return the per-cloud max over the points of the output
    (model.py:76-77), taken on the GEMM output and normalised afterwards (BN + ReLU are monotone).
    drop_keep: tf.nn.dropout(out, drop_keep) behind the layer (model.py:90-91), fused into the BatchNorm passes where the
    kernels allow it (the returned tensor is the DROPPED output either way).
    seg: a packed tower (Segments; x holds its seg.rows rows).  BatchNorm runs over all rows as in a dense tower (seg.bn_per_cloud:
    over the rows of each cloud alone, _conv_bn_act_per_cloud -- recorded only with seg.bn_per_cloud_train); what is per
    cloud goes through the segmented kernels (csrc/seg.hip): gbias is (nseg, Cout) and is addressed through the row -> cloud map
    (rpg is ignored), its gradient is the per-cloud column sum, gmax (any value but None) is the max-pool over each cloud's own
    rows -- always the separate pass over the GEMM output, never the epilogue.  The plane mode is NOT packed: a packed tower
    runs the fp32-class GEMMs (bf16-split / fp32 MFMA) even when HEAD_PLANES is set.
    class_tail: NUM_CLASS of the Final layer that consumes this output NEXT (the last FC layer; FUSE_CLASS_TAIL): where the
    shapes and modes allow, this layer's BatchNorm + dropout pass is held back and runs with the Final layer's product in it.
    Behind the GEMM: one of the tails _conv_tail_class / _dropout / _planes or the plain pass, each a BatchNorm pass with its backward."""
    c = ctx()
    R, Cin = x.shape
    tail, c.class_tail = c.class_tail, None
    if tail is not None and not (tail["out"].data_ptr() == x.data_ptr() and tuple(tail["out"].shape) == tuple(x.shape) and
                                 num_outputs == tail["ncls"] and out2 is None and gbias is None and w_rows is None and
                                 arith is None and gmax is None and drop_keep is None and seg is None and plane_out is None and
                                 x.is_contiguous() and (out is None or out.is_contiguous())):
        _launch_bn1_act_dropout(tail)           # somebody else's input: the plain pass
        tail = None
    if seg is not None and seg.rows != R:
        raise ValueError("offsets end at %d, the tower has %d rows" % (seg.rows, R))
    bpc = per_cloud(seg)
    rgrp = seg.row_group(x.device) if (seg is not None and gbias is not None) else None
    with variable_scope(leaf_scope):
        if w_rows is None:
            wname, W = c.get_variable("weights", (Cin, num_outputs))
            Wx = W
        else:
            wname, W = c.get_variable("weights", (w_rows[2], num_outputs))
            Wx = W[w_rows[0]:w_rows[1]]
        bname, beta = c.get_variable("BatchNorm/beta", (num_outputs,))
    F = num_outputs
    if tail is not None:
        if H.load().dgcnn_gemm_stat_writers(0, R, F, Cin, x.data_ptr(), H.ld2(x), Wx.data_ptr(), H.ld2(Wx)) != 0 or planes_ok(R, Cin, F):
            _launch_bn1_act_dropout(tail)       # (not the streaming class product)
            tail = None
    # the layer's state: what its passes and its tape closure read (the closure keeps every tensor in it alive)
    L = SimpleNamespace(x=x, Wx=Wx, beta=beta, R=R, F=F, relu=relu, out=out, out2=out2, gbias=gbias, rpg=rpg, arith=arith, seg=seg,
                        drop_keep=drop_keep, wname=wname, w_rows=w_rows, bname=bname, xp=None)
    if bpc:
        return _conv_bn_act_per_cloud(c, L, rgrp, gmax)
    L.T = T = torch.empty((R, F), dtype=torch.float32, device=x.device)
    # slots of this layer's statistics buffer = row tiles of its GEMM (asked from the library; another arithmetic: the step's maximum)
    # (0 = a kernel whose grid FOLLOWS the slot count -- the class dimension's streaming product: the step's maximum, more writers)
    c.push_slots((H.load().dgcnn_gemm_stat_writers(0, R, F, Cin, x.data_ptr(), H.ld2(x), Wx.data_ptr(), H.ld2(Wx)) or c.step_slots)
                 if arith is None else c.step_slots)
    st = c.stats(F)
    if tail is not None:
        return _conv_tail_class(c, L, tail, st)
    use_pl = arith is None and seg is None and planes_ok(R, Cin, F)
    # the per-cloud column maximum (model.py:76-77), when asked for, comes out of the GEMM's epilogue as packed (value, first row)
    # keys -- every row tile must lie inside one cloud: clouds of a multiple of 256 points (the library then runs no 192-row tile,
    # gemm.hip:launch<>); otherwise a separate pass over T below
    keys = None
    if seg is not None:
        if gmax is not None:
            keys = c.stats_raw(seg.nseg * F)                                   # zeroed uint64[nseg][F], filled by the pass below
    elif gmax is not None and gmax[1] % 256 == 0 and gmax[0] * gmax[1] == R and F > 4:
        keys = c.stats_raw(gmax[0] * F)                                    # zeroed uint64[B][F]
    if use_pl:
        c.ensure_plane_scales(R)
        L.xp = c.planes_of(x)                                              # (R, Cin) activations
        wt = prepared(("wT", Wx.data_ptr()))                               # (F rows, Cin channels) = W^T
        if wt is None:
            wt = c.new_planes(F, Cin, "w").fill_from(Wx, transpose=True)
        PL.gemm(PL.KC, L.xp, wt, T, gbias=gbias, rpg=rpg, stats=st, colmax=keys, colmax_rpg=0 if keys is None else gmax[1])
    elif seg is not None:
        gemm(x, Wx, T, gbias=gbias, stats=st, arith=arith, row_group=rgrp)
        if gmax is not None:
            H.call("dgcnn_colmax_seg_f32", T.data_ptr(), H.ld2(T), R, F, seg.device(x.device).data_ptr(), seg.nseg,
                   keys.data_ptr(), tag="colmax_seg_kernel", work=4.0 * R * F)
    else:
        gemm(x, Wx, T, gbias=gbias, rpg=rpg, stats=st, arith=arith, colmax=keys, colmax_rpg=0 if keys is None else gmax[1])
    L.mean, L.rstd = bn_finalize(st, F, R)
    c.pop_slots()
    if out is None:
        L.out = c.new_buffer(R, F)
    fuse_drop = drop_keep is not None and FUSE_DROPOUT and not use_pl and F % 4 == 0 and out2 is None and gmax is None
    if fuse_drop:
        _conv_tail_dropout(c, L, class_tail)
    elif use_pl:
        _conv_tail_planes(c, L, plane_out, f32_out)     # (only the plane GEMM's layers write operand planes)
    else:
        _bn1_act(L)
        if c.recording:
            _record(c, _conv_plain_bwd, L, None)
    if gmax is None:
        if drop_keep is not None and not fuse_drop:
            return dropout(L.out, drop_keep)       # (plane / deterministic modes: the separate pass)
        return L.out
    return L.out, _conv_gmax(c, L, gmax, keys)


def _record(c, bwd, *args):
    """Append bwd(c, *args) to the tape; it runs at the slot count of the reduction kernels (their grids follow it: 256 writers)."""
    def run():
        with c.op_slots(0):
            bwd(c, *args)
    c.tape.append(run)


def _dWx(c, L):
    """The gradient accumulator of the weight rows that multiply the layer's input."""
    return c.var_grads[L.wname] if L.w_rows is None else c.var_grads[L.wname][L.w_rows[0]:L.w_rows[1]]


def _bn1_act(L):
    """BatchNorm + activation of the GEMM output T into out (and its second copy out2)."""
    R, F, out, out2 = L.R, L.F, L.out, L.out2
    H.call("dgcnn_bn_act_kreduce_f32", L.T.data_ptr(), R, 1, F, L.mean.data_ptr(), L.rstd.data_ptr(), L.beta.data_ptr(),
           int(L.relu), out.data_ptr(), H.ld2(out), 0, 0, H._p(out2), 0 if out2 is None else H.ld2(out2), 0,
           tag="bn_act_kreduce_kernel<k=1>", work=4.0 * R * F * (2 if out2 is None else 3))


def _bn1_bwd_inputs(c, L, join):
    """(d(out), d(out2) or None, zeroed sums, d(gbias) or None) of a k = 1 BatchNorm backward; None: nobody wants the gradient.
    join: the passes read ONE gradient (fused dropout, planes; the default passes read both, except for the shapes tested here)."""
    dout = c.grad(L.out)
    if dout is None:
        return None
    d2 = c.grad(L.out2) if L.out2 is not None else None
    # (DETERMINISTIC: unaligned parameter slices send the reduce to the fixed-order twin, which takes one gradient)
    if d2 is not None and (join or L.F % 4 != 0 or
                           (DETERMINISTIC and not k1_reduce_fixed_order(L.T, 1, L.F, L.mean, L.rstd, L.beta, dout, d2, None))):
        # the second copy's gradient joins the first (the default passes read both instead)
        H.call("dgcnn_copy2d_f32", d2.data_ptr(), H.ld2(d2), dout.data_ptr(), H.ld2(dout), L.R, L.F, 1)
        d2 = None
    red = c.stats(L.F)
    dgb = c.grad(L.gbias) if L.gbias is not None else None
    return dout, d2, red, dgb


def _conv_bwd_products(c, L, dT, dgb):
    """The end of a layer's backward, from dT = d(GEMM output).  Data gradient FIRST, on the critical path; the weight gradient is
    issued behind it on the side stream, so that it runs under the bandwidth-bound BatchNorm / gather passes that follow on the main
    stream -- not next to the data gradient, another matrix-pipe kernel at the package power cap (both then run at half speed:
    profiles/r03/wgrad_order.txt).  Last the gradient of the per-cloud bias."""
    dx, bx = c.grad_w(L.x)
    if dx is not None:
        gemm(dT, L.Wx, dx, transB=True, beta=bx, arith=L.arith)       # dx (+)= dT W^T
    with c.off_critical_path(rows=L.R):
        gemm(L.x, dT, _dWx(c, L), transA=True, beta=1.0, arith=L.arith)   # dW += x^T dT
    if dgb is not None:                                                 # tf.tile^T: sum over the cloud
        tmp = torch.empty_like(L.gbias)
        if L.seg is not None:
            seg_colsum(dT, L.seg, tmp)
        else:
            H.call("dgcnn_group_colsum_f32", dT.data_ptr(), H.ld2(dT), L.gbias.shape[0], L.rpg, L.F, tmp.data_ptr())
        H.call("dgcnn_axpby_f32", tmp.data_ptr(), 1.0, dgb.data_ptr(), 1.0, tmp.numel())


def _conv_tail_class(c, L, tail, st):
    """The Final layer behind a held-back FC layer (tail).  F1: the held-back BatchNorm + dropout pass of the FC layer writes x AND
    forms T = x W with its column statistics, on the streaming product's grid; F2 (softmax_loss) folds the statistics, applies
    this layer's BatchNorm + ReLU and the loss.  Backward: the sums here, the rest inside the FC layer's passes where it can."""
    x, Wx, T, R, F = L.x, L.Wx, L.T, L.R, L.F
    scal = torch.empty(2, dtype=torch.float32, device=x.device)           # [loss, accuracy]: zeroed by F1
    H.call("dgcnn_bn1_act_class_f32", tail["T"].data_ptr(), R, x.shape[1], tail["mean"].data_ptr(), tail["rstd"].data_ptr(),
           tail["beta"].data_ptr(), int(tail["relu"]), float(tail["keep"]), tail["seed"].data_ptr(), x.data_ptr(), H.ld2(x),
           Wx.data_ptr(), H.ld2(Wx), F, T.data_ptr(), F, st.data_ptr(), scal.data_ptr(),
           tag="bn1_act_class_kernel", work=4.0 * R * x.shape[1] * 2)
    mr = torch.empty((2, F), dtype=torch.float32, device=x.device)
    L.mean, L.rstd = mr[0], mr[1]
    if L.out is None:
        L.out = c.new_buffer(R, F)
    c.loss_tail = dict(T=T, st=st, F=F, R=R, beta=L.beta, relu=L.relu, mean=L.mean, rstd=L.rstd, out=L.out, scal=scal,
                       nslots=H.stat_slots())
    c.pop_slots()
    if c.recording:
        _record(c, _conv_plain_bwd, L, tail)
    return L.out


def _conv_plain_bwd(c, L, tail):
    """Sums, then dT in place of T, then the products.  tail: the FC layer's record when this is the Final layer behind it."""
    g = _bn1_bwd_inputs(c, L, False)
    if g is None:
        return
    dout, d2, red, dgb = g
    T, R, F, mean, rstd, beta, relu = L.T, L.R, L.F, L.mean, L.rstd, L.beta, L.relu
    nsrc = 1 if d2 is None else 2                                  # k = 1: dz = dout + d2 (the kernels' dmax + dmean / k)
    bn_bwd_reduce(T, R, 1, F, mean, rstd, beta, relu, dout, d2, None, None, red,
                  tag="bn_bwd_reduce_kernel<k=1>", work=4.0 * R * F * (1 + nsrc))
    if tail is not None and FUSE_CLASS_TAIL and d2 is None and dgb is None and dout.is_contiguous() and c.first_touch(L.x):
        # the rest of this layer's backward runs inside the FC layer's passes (B1 / B2: _conv_dropout_bwd)
        tail["bwd"] = dict(Tf=T, ncls=F, mean=mean, rstd=rstd, beta=beta, relu=relu, dfin=dout, red=red,
                           dbeta=c.var_grads[L.bname], W=L.Wx, dWx=_dWx(c, L))
        return
    H.call("dgcnn_bn_bwd_apply_f32", T.data_ptr(), R, 1, F, mean.data_ptr(), rstd.data_ptr(), beta.data_ptr(),
           int(relu), dout.data_ptr(), H.ld2(dout), H._p(d2), 0 if d2 is None else H.ld2(d2), 0, 0, 0, red.data_ptr(),
           T.data_ptr(), 0, 0, c.var_grads[L.bname].data_ptr(), 1.0, tag="bn_bwd_apply_kernel<k=1>", work=4.0 * R * F * (2 + nsrc))
    _conv_bwd_products(c, L, T, dgb)


def _conv_tail_dropout(c, L, class_tail):
    """tf.nn.dropout inside the layer's BatchNorm passes (FUSE_DROPOUT).  class_tail: the pass is held back for the Final layer's
    call (c.class_tail; conv_bn_act, flush_class_tail and the backward of that layer answer through the record)."""
    if c.seed_dev is None:
        c.advance_seed()
    L.seed = c.seed_dev                     # device-resident: the backward regenerates the mask from the same value
    held = dict(T=L.T, R=L.R, F=L.F, mean=L.mean, rstd=L.rstd, beta=L.beta, relu=L.relu, keep=L.drop_keep, seed=L.seed, out=L.out,
                ncls=class_tail, bwd=None)
    if (class_tail is not None and FUSE_CLASS_TAIL and DETERMINISTIC and c.dense_loss_follows and c.recording and
            L.seg is None and L.gbias is None and L.w_rows is None and L.F == 256 and 1 <= int(class_tail) <= 4 and
            L.out.is_contiguous()):
        c.class_tail = held                 # runs inside the Final layer's call (F1), or as the plain pass if that is not next
    else:
        _launch_bn1_act_dropout(held)
    if c.recording:
        _record(c, _conv_dropout_bwd, L, held)


def _conv_dropout_bwd(c, L, held):
    T, R, F, mean, rstd, beta, relu = L.T, L.R, L.F, L.mean, L.rstd, L.beta, L.relu
    tb = held["bwd"]
    if tb is not None:
        # B1, finalize, B2: d(out) = dT_final W_final^T is formed in registers (never stored); B1 also applies the Final
        # layer's BatchNorm backward (dT_final in place of its GEMM output, d(beta_final))
        red = c.stats(F)
        args = (T.data_ptr(), R, F, mean.data_ptr(), rstd.data_ptr(), beta.data_ptr(), int(relu), float(L.drop_keep),
                L.seed.data_ptr(), tb["Tf"].data_ptr(), tb["ncls"], tb["mean"].data_ptr(), tb["rstd"].data_ptr(),
                tb["beta"].data_ptr(), int(tb["relu"]), tb["dfin"].data_ptr(), tb["red"].data_ptr(), tb["dbeta"].data_ptr(),
                1.0, tb["W"].data_ptr(), H.ld2(tb["W"]), red.data_ptr(), T.data_ptr(), c.var_grads[L.bname].data_ptr(), 1.0)
        H.call("dgcnn_bn1_bwd_class_f32", *args, 1, tag="bn1_bwd_class_kernel", work=4.0 * R * F)
        # the Final layer's weight gradient starts as soon as B1 has left dT_final: on the side stream, under the two
        # bandwidth-bound launches below -- not next to this layer's data-gradient GEMM
        with c.off_critical_path(rows=R):
            gemm(L.out, tb["Tf"], tb["dWx"], transA=True, beta=1.0)
        H.call("dgcnn_bn1_bwd_class_f32", *args, 2, tag="bn1_bwd_class_kernel", work=4.0 * R * F * 2)
        held["bwd"] = None
        _conv_bwd_products(c, L, T, None)
        return
    g = _bn1_bwd_inputs(c, L, True)
    if g is None:
        return
    dout, _, red, dgb = g
    # sums, finalise (+ dbeta) and dT (in place of T), all reading d(dropped output) through the regenerated mask
    H.call("dgcnn_bn1_bwd_dropout_f32", T.data_ptr(), R, F, mean.data_ptr(), rstd.data_ptr(), beta.data_ptr(), int(relu),
           float(L.drop_keep), L.seed.data_ptr(), dout.data_ptr(), H.ld2(dout), red.data_ptr(), T.data_ptr(),
           c.var_grads[L.bname].data_ptr(), 1.0, tag="bn_bwd_apply_kernel<k=1>", work=4.0 * R * F * 5)
    _conv_bwd_products(c, L, T, dgb)


def _conv_tail_planes(c, L, plane_out, f32_out):
    """A layer of the plane GEMM: plane_out receives the activated output as operand planes of the next product (else the plain
    pass); the backward writes dT as planes and runs both products on the plane GEMM."""
    if plane_out is None:
        _bn1_act(L)
    else:
        T, R, F, out, out2 = L.T, L.R, L.F, L.out, L.out2
        H.call("dgcnn_bn_act_planes_f32", T.data_ptr(), F, R, F, L.mean.data_ptr(), L.rstd.data_ptr(), L.beta.data_ptr(), int(L.relu),
               plane_out.fmt, H._p(plane_out.scale), plane_out.ptr(), plane_out.plane_stride, plane_out.ra,
               out.data_ptr() if f32_out else 0, H.ld2(out), H._p(out2) if f32_out else 0, 0 if out2 is None else H.ld2(out2),
               tag="bn_act_planes_kernel", work=4.0 * R * F * (2 + (1 if f32_out else 0)))
        c.planes[c.plane_key(out)] = plane_out
    if c.recording:
        _record(c, _conv_planes_bwd, L)


def _conv_planes_bwd(c, L):
    g = _bn1_bwd_inputs(c, L, True)
    if g is None:
        return
    dout, _, red, dgb = g
    x, Wx, T, R, F, gbias, rpg = L.x, L.Wx, L.T, L.R, L.F, L.gbias, L.rpg
    # sums + column maxima -> bound on |dT| -> the dT plane set's scale -> dT written as planes (never as fp32)
    maxbits = c.stats_raw(F + 1)                              # uint32[2 F + 1]: column maxima + the tensor-wide bound
    H.call("dgcnn_bn1_bwd_reduce_max_f32", T.data_ptr(), R, F, L.mean.data_ptr(), L.rstd.data_ptr(), L.beta.data_ptr(),
           int(L.relu), dout.data_ptr(), H.ld2(dout), red.data_ptr(), maxbits.data_ptr(),
           tag="bn1_bwd_reduce_max_kernel", work=4.0 * R * F * 2)
    dTp = PL.PlaneSet(R, F, HEAD_PLANES, device=x.device)
    sc = torch.empty(1, dtype=torch.float32, device=x.device)
    if HEAD_PLANES == PL.F16X2:
        dTp.scale = sc
    fused_gsum = dgb is not None and rpg % 64 == 0
    tmp = H.memset(torch.empty_like(gbias)) if fused_gsum else None
    dT32 = T if (dgb is not None and not fused_gsum) else None        # (in place: every element is read before it is written)
    H.call("dgcnn_bn1_bwd_apply_planes_f32", T.data_ptr(), R, F, L.mean.data_ptr(), L.rstd.data_ptr(), L.beta.data_ptr(),
           int(L.relu), dout.data_ptr(), H.ld2(dout), red.data_ptr(), maxbits.data_ptr(), HEAD_PLANES, sc.data_ptr(),
           dTp.ptr(), dTp.plane_stride, dTp.ra, H._p(dT32), H._p(tmp), F, int(rpg), c.var_grads[L.bname].data_ptr(), 1.0,
           tag="bn1_bwd_apply_planes_kernel", work=4.0 * R * F * 3)
    # the products in the order of _conv_bwd_products (data gradient first, weight gradient on the side stream), on the plane GEMM
    dx, bx = c.grad_w(x)
    if dx is not None:
        wd = prepared(("w", Wx.data_ptr()))                                  # (Cin rows, F channels)
        if wd is None:
            wd = c.new_planes(Wx.shape[0], F, "w").fill_from(Wx)
        PL.gemm(PL.KC, dTp, wd, dx, beta=bx)                                 # dx (+)= dT W^T
    with c.off_critical_path(dTp.buf, sc, rows=R):
        PL.gemm(PL.TR, L.xp, dTp, _dWx(c, L), beta=1.0, ws=c.workspace())  # dW += x^T dT
    if dgb is not None:                                                     # tf.tile^T: sum over the cloud
        if not fused_gsum:
            tmp = torch.empty_like(gbias)
            H.call("dgcnn_group_colsum_f32", dT32.data_ptr(), F, gbias.shape[0], rpg, F, tmp.data_ptr())
        H.call("dgcnn_axpby_f32", tmp.data_ptr(), 1.0, dgb.data_ptr(), 1.0, tmp.numel())


def _conv_gmax(c, L, gmax, keys, per_cloud=False):
    """model.py:76-77 max_pool over the points of each cloud, on the GEMM output: z = relu((t - mean) rstd + beta) is
    non-decreasing in t, so max_n z[n] = z(max_n t[n]) and the first arg-max of t is an arg-max of z.  per_cloud: mean / rstd are
    (nseg, F) tables, every cloud's maxima are normalised with its own row."""
    x, T, F, out, seg = L.x, L.T, L.F, L.out, L.seg
    Bc, Nc = (seg.nseg, 0) if seg is not None else gmax
    graw = torch.empty((Bc, F), dtype=torch.float32, device=x.device)
    arg = torch.empty((Bc, F), dtype=torch.int32, device=x.device)
    if keys is not None:
        H.call("dgcnn_colmax_decode_f32", keys.data_ptr(), Bc * F, graw.data_ptr(), arg.data_ptr())
    else:
        H.call("dgcnn_global_max_f32", T.data_ptr(), F, Bc, Nc, F, graw.data_ptr(), arg.data_ptr())
    g = c.new_buffer(Bc, F)
    if per_cloud:
        H.call("dgcnn_seg_bn_act_f32", graw.data_ptr(), F, Bc, F, None, L.mean.data_ptr(), L.rstd.data_ptr(), L.beta.data_ptr(),
               int(L.relu), g.data_ptr(), F, None, 0)
    else:
        H.call("dgcnn_bn_act_kreduce_f32", graw.data_ptr(), Bc, 1, F, L.mean.data_ptr(), L.rstd.data_ptr(), L.beta.data_ptr(),
               int(L.relu), g.data_ptr(), F, 0, 0, 0, 0, 0)
    if c.recording:
        def bwd_g():
            dg_, dout = c.grad(g), c.grad(out)
            if dg_ is None or dout is None:
                return
            if seg is not None:
                H.call("dgcnn_global_max_bwd_seg_f32", dg_.data_ptr(), arg.data_ptr(), seg.device(x.device).data_ptr(), Bc, F,
                       dout.data_ptr(), H.ld2(dout))
            else:
                H.call("dgcnn_global_max_bwd_f32", dg_.data_ptr(), arg.data_ptr(), Bc, Nc, F, dout.data_ptr(), H.ld2(dout))
        c.tape.append(bwd_g)
    return g


def _conv_bn_act_per_cloud(c, L, rgrp, gmax):
    """conv_bn_act of a packed tower with per-cloud BatchNorm.  The GEMM runs WITHOUT epilogue statistics (a row
    tile straddles clouds; the per-cloud bias through the row -> cloud map stays); then the per-cloud sums of T in a fixed
    order, the (nseg, F) tables and the apply pass that picks the table row of the row's cloud.  gmax: the per-cloud maxima of T
    are normalised with their own cloud's table row -- BN + ReLU are monotone per cloud, so the max-pool identity holds.
    Recording (seg.bn_per_cloud_train): one tape closure -- per-cloud sum dz / sum dz xhat (both gradient inputs read in place),
    the c1 / c2 tables (+ dbeta), dT in place of T, then the dense branch's products (_conv_bwd_products; the per-cloud bias
    gradient is mathematically 0 per cloud -- the literal form, as the forward keeps the bias in T)."""
    x, beta, F, relu, out2, seg = L.x, L.beta, L.F, L.relu, L.out2, L.seg
    R = x.shape[0]
    dev = x.device
    off = seg.device(dev)
    rg = seg.row_group(dev)
    T = torch.empty((R, F), dtype=torch.float32, device=dev)
    gemm(x, L.Wx, T, gbias=L.gbias, arith=L.arith, row_group=rgrp)
    st = torch.empty(seg.nseg * 2 * F, dtype=torch.float64, device=dev)
    ws = seg_stats_workspace(R, seg.nseg, F, dev)
    H.call("dgcnn_seg_colstats_f32", T.data_ptr(), H.ld2(T), R, F, off.data_ptr(), seg.nseg, st.data_ptr(), ws.data_ptr(), ws.numel(),
           tag="seg_colstats_kernel", work=4.0 * R * F)
    mean, rstd = seg_bn_finalize(st, seg, F, 1)
    out = L.out
    if out is None:
        out = c.new_buffer(R, F)
    H.call("dgcnn_seg_bn_act_f32", T.data_ptr(), H.ld2(T), R, F, rg.data_ptr(), mean.data_ptr(), rstd.data_ptr(), beta.data_ptr(),
           int(relu), out.data_ptr(), H.ld2(out), H._p(out2), 0 if out2 is None else H.ld2(out2),
           tag="seg_bn_act_kernel", work=4.0 * R * F * (2 if out2 is None else 3))
    if c.recording:
        def bwd():
            dout = c.grad(out)
            if dout is None:
                return
            d2 = c.grad(out2) if out2 is not None else None
            nsrc = 1 if d2 is None else 2
            red = torch.empty(seg.nseg * 2 * F, dtype=torch.float64, device=dev)
            wsb = seg_stats_workspace(R, seg.nseg, F, dev)
            par = (mean.data_ptr(), rstd.data_ptr(), beta.data_ptr(), int(relu), dout.data_ptr(), H.ld2(dout), H._p(d2),
                   0 if d2 is None else H.ld2(d2))
            H.call("dgcnn_seg_bn_bwd_reduce_f32", T.data_ptr(), H.ld2(T), R, F, off.data_ptr(), seg.nseg, *par, red.data_ptr(),
                   wsb.data_ptr(), wsb.numel(), tag="seg_bn_bwd_reduce_kernel", work=4.0 * R * F * (1 + nsrc))
            c1, c2 = seg_bn_bwd_finalize(red, seg, F, 1, c.var_grads[L.bname])
            H.call("dgcnn_seg_bn_bwd_apply_f32", T.data_ptr(), H.ld2(T), R, F, rg.data_ptr(), *par, c1.data_ptr(), c2.data_ptr(),
                   T.data_ptr(), H.ld2(T), tag="seg_bn_bwd_apply_kernel", work=4.0 * R * F * (2 + nsrc))
            _conv_bwd_products(c, L, T, c.grad(L.gbias) if L.gbias is not None else None)
        c.tape.append(bwd)
    if gmax is None:
        return out if L.drop_keep is None else dropout(out, L.drop_keep)
    keys = c.stats_raw(seg.nseg * F)                                          # zeroed uint64[nseg][F]
    H.call("dgcnn_colmax_seg_f32", T.data_ptr(), H.ld2(T), R, F, off.data_ptr(), seg.nseg, keys.data_ptr(),
           tag="colmax_seg_kernel", work=4.0 * R * F)
    L.T, L.out, L.mean, L.rstd = T, out, mean, rstd
    return out, _conv_gmax(c, L, gmax, keys, per_cloud=True)


# ----------------------------------------------------------------------------------------------
# dgcnn/ops.py:42-73 edge_conv as one block
# ----------------------------------------------------------------------------------------------
def prepare_step_weights(edge_w0, head_w):
    """Everything that depends on the PARAMETERS only -- conv0's folded weights [Wa - Wb | Wb] of every EdgeConv layer and, in
    plane mode, the head weights as operand planes in both orientations -- issued at the start of the step on the side stream,
    where it runs under the first k-NN instead of as ~10 six-microsecond kernels on the critical path.
    edge_w0: [(W0 (2C, F), C, F)]; head_w: [Wx views] (plane mode, else empty)."""
    c = ctx()
    if not (WGRAD_SIDE_STREAM and c.flat_param is not None) or c.wprep:
        return
    dev = c.device
    items, temps = [], []
    for W0, C, F in edge_w0:
        Cp = (C + 3) // 4 * 4
        wcat = torch.empty((Cp, 2 * F), dtype=torch.float32, device=dev)
        if Cp != C:
            H.memset(wcat)
        items.append((("wcat", W0.data_ptr()), wcat, W0, C, F))
        temps.append(wcat)
    planes = []
    for Wx in head_w:
        wt = c.new_planes(Wx.shape[1], Wx.shape[0], "w")
        wd = c.new_planes(Wx.shape[0], Wx.shape[1], "w")
        planes.append((Wx, wt, wd))
        temps += [wt.buf, wd.buf]
    with c.off_critical_path(*temps):
        for key, wcat, W0, C, F in items:
            H.call("dgcnn_edge_weight_split_f32", W0.data_ptr(), C, F, wcat.data_ptr())
            c.wprep[key] = wcat
        for Wx, wt, wd in planes:
            c.wprep[("wT", Wx.data_ptr())] = wt.fill_from(Wx, transpose=True)
            c.wprep[("w", Wx.data_ptr())] = wd.fill_from(Wx)
        if c.side is not None and torch.cuda.current_stream() == c.side:
            c.wprep_event = True          # the first consumer makes the main stream wait for the side stream (prepared())


def prepared(key):
    """A tensor prepared by prepare_step_weights (the main stream is made to wait for the preparation once), or None."""
    c = ctx()
    v = c.wprep.get(key)
    if v is not None and c.wprep_event:
        # (waits for everything on the side stream so far: between the preparation and its first consumer -- conv0 of the first
        # EdgeConv layer, right behind the first k-NN -- nothing else is issued there)
        H.stream_wait(torch.cuda.current_stream(), c.side)
        c.wprep_event = None
    return v


def _point_gemm(c, x, W0, R, C, F):
    """Wcat = [Wa - Wb | Wb] and [U | V] = X Wcat (conv0 folded to the points).  C = 3 (raw coordinates): the reduction
    dimension is padded to 4 with a zero column / zero weight row so that the GEMM takes the float4 path."""
    Cp = (C + 3) // 4 * 4
    xg = x
    ready = prepared(("wcat", W0.data_ptr()))
    if Cp != C:
        xg = torch.empty((R, Cp), dtype=torch.float32, device=x.device)
        wcat = ready if ready is not None else H.zeros((Cp, 2 * F), torch.float32, x.device)
    else:
        wcat = ready if ready is not None else torch.empty((C, 2 * F), dtype=torch.float32, device=x.device)
    UV = torch.empty((R, 2 * F), dtype=torch.float32, device=x.device)

    if Cp != C:
        H.call("dgcnn_pad_copy_f32", x.data_ptr(), H.ld2(x), C, xg.data_ptr(), Cp, R)
    if ready is None:
        H.call("dgcnn_edge_weight_split_f32", W0.data_ptr(), C, F, wcat.data_ptr())
    gemm(xg, wcat, UV, arith=None)
    return Cp, xg, wcat, UV


def build_csr(idx, B, N, k, side=None):
    """Transposed adjacency of idx (B,N,k): (off (R+1), rev (R*k)) -- for every point the ids e = point * k + m of the edges that
    point at it.  DETERMINISTIC: every bucket in ascending edge order (the build fills buckets through LDS cursors: any order).
    side = (ctx, rows): the kernels run on the side stream (the buffers are allocated on the current one and handed over)."""
    R = B * N
    dev = idx.device
    cws = torch.empty(2 * R, dtype=torch.int32, device=dev)
    off = torch.empty(R + 1, dtype=torch.int32, device=dev)
    rev = torch.empty(R * k, dtype=torch.int32, device=dev)
    srt = torch.empty(R * k, dtype=torch.int32, device=dev) if DETERMINISTIC else None

    def fill():
        H.call("dgcnn_edge_csr_build", idx.data_ptr(), B, N, k, cws.data_ptr(), off.data_ptr(), rev.data_ptr())
        if srt is not None:
            H.call("dgcnn_edge_csr_sort", idx.data_ptr(), B, N, k, off.data_ptr(), rev.data_ptr(), srt.data_ptr())
    if side is None:
        fill()
    else:
        with side[0].off_critical_path(*[t for t in (cws, off, rev, srt) if t is not None], rows=side[1]):
            fill()
    return off, (rev if srt is None else srt)


def _csr_ahead(c, L):
    """The transposed adjacency depends only on idx: built during the forward, off the critical path (None: no side stream)."""
    if WGRAD_SIDE_STREAM and L.R >= SIDE_STREAM_MIN_ROWS:
        return build_csr(L.idx, L.B, L.N, L.k, side=(c, L.R))
    return None


def _incoming_sum(L, dY, S, csr=None):
    """tf.gather^T as a gather: bucket the edges by target (csr: built on the side stream during the forward), then every point
    sums its incoming dY rows (fp32 or bf16) into S (None: a fresh (R, F), allocated behind the adjacency).  Returns S."""
    R, k, F = L.R, L.k, L.F
    off, rev = csr if csr is not None else build_csr(L.idx, L.B, L.N, k)
    if S is None:
        S = torch.empty((R, F), dtype=torch.float32, device=dY.device)
    if dY.dtype == torch.bfloat16:
        H.call("dgcnn_edge_gather_sum_bf16", dY.data_ptr(), off.data_ptr(), rev.data_ptr(), R, F, S.data_ptr(), H.ld2(S),
               tag="csr_gather_sum_kernel<bf16>", work=2.0 * R * k * F + 4.0 * R * F)
    else:
        H.call("dgcnn_edge_gather_sum_f32", dY.data_ptr(), off.data_ptr(), rev.data_ptr(), R, F, S.data_ptr(), H.ld2(S),
               tag="csr_gather_sum_kernel", work=4.0 * (R * k * F + R * F))
    return S


def _centre_weight(W0, C, F, bf16=False):
    """(wd, W): the centre weight wd = W[:C] - W[C:] of E = [x_i, x_j - x_i], a fresh (C, F); W = W0, or with bf16 a copy of W0
    rounded to bf16 (never W0 itself: a variable)."""
    W = W0
    if bf16:
        W = torch.empty_like(W0)
        H.call("dgcnn_round_bf16_f32", W0.data_ptr(), W.data_ptr(), W0.numel())
    wd = torch.empty((C, F), dtype=torch.float32, device=W0.device)
    H.call("dgcnn_copy2d_f32", W[:C].data_ptr(), F, wd.data_ptr(), F, C, F, 0)
    H.call("dgcnn_axpby_f32", W[C:].data_ptr(), -1.0, wd.data_ptr(), 1.0, C * F)
    return wd, W


def _edge_dx(L, dx, dysum, dY, bf16=False, wd=None):
    """dx from the edge gradients dY (dysum = sum_m dY).  dE = dY W^T never exists: the transpose of `edges` is linear, so
      dx_i += (sum_m dY) (W[:C] - W[C:])^T        dx_j += (sum of the dY rows of the edges that point at j) W[C:]^T
    -- the same sums of the same products as the literal edge-level product + scatter-add, taken at the points (k times fewer
    MACs, no atomics).  bf16: W = bf16(W0), dY on the bf16 grid; the point-level products run in the exact arithmetic.
    wd: the centre weight where the forward kept it.  F % 4 != 0: the second term as the edge-level product + scatter."""
    C, F, W = L.C, L.F, L.W0
    if wd is None:
        wd, W = _centre_weight(W, C, F, bf16)
    gemm(dysum, wd, dx, transB=True, beta=1.0)
    if F % 4 != 0:
        if bf16:
            raise H.HipError("bf16 edge-MLP: the input gradient needs filter counts that are multiples of 4 (F = %d)" % F)
        H.call("dgcnn_edge_mlp_dgrad_scatter_f32", dY.data_ptr(), W.data_ptr(), L.idx.data_ptr(), L.B, L.N, C, L.k,
               F, dx.data_ptr(), H.ld2(dx),
               tag="gemm_kernel<A_ROW,B_COL,SCATTER,%d,%d>" % (_tile_m(L.R * L.k, C), 64 if C <= 64 else 128),
               work=2.0 * L.R * L.k * C * F)
        return
    # (an fp32 dY's sum is allocated before the adjacency is built, a bf16 dY's behind it: the order either route always had)
    S = None if dY.dtype == torch.bfloat16 else torch.empty((L.R, F), dtype=torch.float32, device=dx.device)
    gemm(_incoming_sum(L, dY, S), W[C:], dx, transB=True, beta=1.0)


def _edge_outputs(c, L, outs):
    if outs is None:
        L.mm, L.net_out = c.new_buffer(L.R, 2 * L.F), None
    else:
        L.mm, L.net_out = outs
    L.mx, L.mn = L.mm[:, :L.F], L.mm[:, L.F:]


def _edge_finalize(c, L, st, outs):
    """conv0's BatchNorm statistics are complete: mean / rstd, the output buffers, the backward's counts."""
    L.mean, L.rstd = bn_finalize(st, L.F, L.R * L.k)                    # ops.py:53
    c.pop_slots()
    _edge_outputs(c, L, outs)
    L.cnt = torch.empty((L.R, L.F), dtype=torch.float32, device=L.x.device) if c.recording else None   # ties of the max


def _edge_bn_act_y(L):
    R, k, F, mx, mn = L.R, L.k, L.F, L.mx, L.mn
    H.call("dgcnn_bn_act_kreduce_f32", L.Y.data_ptr(), R, k, F, L.mean.data_ptr(), L.rstd.data_ptr(), L.beta0.data_ptr(), 1,
           mx.data_ptr(), H.ld2(mx), mn.data_ptr(), H.ld2(mn), 0, 0, H._p(L.cnt),
           tag="bn_act_kreduce_kernel", work=4.0 * (R * k * F + 2 * R * F))   # ops.py:54-58


def _edge_bwd_inputs(c, L):
    """(d(max), d(mean), zeroed sums) of a conv0 backward, or None when nobody wants the layer's gradient."""
    dmm = c.grad(L.mm)
    if dmm is None:
        return None
    return dmm[:, :L.F], dmm[:, L.F:], c.stats(L.F)


def _edge_reduce_points(L, dmx, dmn, red):
    """sum dz, sum dz*xhat from the forward's per-point outputs alone (bn.hip): no pass over the edges."""
    mx, mn, R, F = L.mx, L.mn, L.R, L.F
    H.call("dgcnn_edge_bn_bwd_reduce_points_f32", mx.data_ptr(), H.ld2(mx), mn.data_ptr(), H.ld2(mn),
           L.cnt.data_ptr(), dmx.data_ptr(), H.ld2(dmx), dmn.data_ptr(), H.ld2(dmn), L.beta0.data_ptr(), R, L.k, F,
           red.data_ptr(), tag="edge_bwd_reduce_points_kernel", work=4.0 * 5 * R * F)


def _edge_bn_bwd_reduce_y(L, dmx, dmn, red):
    R, k, F = L.R, L.k, L.F
    bn_bwd_reduce(L.Y, R, k, F, L.mean, L.rstd, L.beta0, 1, dmx, dmn, L.mx, L.cnt, red,
                  tag="bn_bwd_reduce_kernel", work=4.0 * (R * k * F + 2 * R * F))


def _edge_bn_bwd_apply_y(c, L, dmx, dmn, red, dysum, relu=1):
    """dY in place of the materialised Y (+ dysum = sum_m dY where asked for, dbeta)."""
    Y, R, k, F, mx = L.Y, L.R, L.k, L.F, L.mx
    H.call("dgcnn_bn_bwd_apply_f32", Y.data_ptr(), R, k, F, L.mean.data_ptr(), L.rstd.data_ptr(), L.beta0.data_ptr(),
           relu, dmx.data_ptr(), H.ld2(dmx), dmn.data_ptr(), H.ld2(dmn), mx.data_ptr(), H.ld2(mx), L.cnt.data_ptr(),
           red.data_ptr(), Y.data_ptr(),
           H._p(dysum), 0 if dysum is None else H.ld2(dysum), c.var_grads[L.b0name].data_ptr(), 1.0,
           tag="bn_bwd_apply_kernel", work=4.0 * (2 * R * k * F + 3 * R * F))


def _conv0_fold(c, L, st, outs, virtual):
    """conv0 is linear: E W0 = x_i (Wa-Wb) + x_j Wb = U[i] + V[j] with [U | V] = X [Wa-Wb | Wb] -- ONE point-level GEMM (k times
    fewer MACs than the edge tensor product), then a per-edge gather-add that takes the BatchNorm column sums and, unless
    `virtual`, writes Y (it is then bound by that HBM write).  C = 3 (raw coordinates): _point_gemm pads the reduction dimension
    to 4 so that the point-level GEMMs take the float4 path (the generic scalar kernel costs ~10x more on them)."""
    R, k, F = L.R, L.k, L.F
    L.Y = None if virtual else torch.empty((R * k, F), dtype=torch.float32, device=L.x.device)
    L.Cp, L.xg, L.wcat, L.UV = _point_gemm(c, L.x, L.W0, R, L.C, F)
    L.esrc = (L.UV[:, F:].data_ptr(), 2 * F, L.UV.data_ptr(), 2 * F, L.idx.data_ptr(), L.B, L.N, k, F)
    H.call("dgcnn_edge_gather_add_f32", *L.esrc, H._p(L.Y), st.data_ptr(),
           tag="edge_gather_add_kernel", work=4.0 * ((0 if virtual else R * k * F) + 2 * R * F) + 4.0 * R * k,
           nbytes=4.0 * (R * k * F + R * F))   # ops.py:21-52   (nbytes: rows gathered from L2 -- bench.py's l2-gather roof)
    if not virtual:
        L.UV = L.esrc = None
    _edge_finalize(c, L, st, outs)
    if virtual:
        # esrc holds raw pointers into UV: L.UV keeps it alive for the backward
        H.call("dgcnn_edge_bn_act_kreduce_f32", *L.esrc, L.mean.data_ptr(), L.rstd.data_ptr(), L.beta0.data_ptr(), 1,
               L.mx.data_ptr(), H.ld2(L.mx), L.mn.data_ptr(), H.ld2(L.mn), H._p(L.cnt),
               tag="bn_act_kreduce_kernel<edge>", work=4.0 * (4 * R * F) + 4.0 * R * k, nbytes=4.0 * (R * k * F + R * F))   # ops.py:54-58
    else:
        _edge_bn_act_y(L)
    if not c.recording:
        return
    fv = F // 4
    fused_l0 = (virtual and EDGE_BWD_FUSED_L0 and L.C <= 4 and F % 4 == 0 and fv & (fv - 1) == 0 and fv <= 256 and
                not c.tracked(L.x))
    _record(c, _conv0_fold_bwd, L, None if fused_l0 else _csr_ahead(c, L), fused_l0)


def _conv0_fold_bwd(c, L, csr, fused_l0):
    g = _edge_bwd_inputs(c, L)
    if g is None:
        return
    dmx, dmn, red = g
    x, R, k, F, mx = L.x, L.R, L.k, L.F, L.mx
    if L.Y is None:
        _edge_reduce_points(L, dmx, dmn, red)
    else:
        _edge_bn_bwd_reduce_y(L, dmx, dmn, red)
    dx = c.grad(x)
    if fused_l0 and dx is None:
        # first layer (raw coordinates, nobody wants d(points)): dY is formed and consumed in one pass, straight into dW0
        ws = c.workspace()
        H.call("dgcnn_edge_bn_bwd_apply_wgrad_f32", *L.esrc, L.mean.data_ptr(), L.rstd.data_ptr(), L.beta0.data_ptr(),
               dmx.data_ptr(), H.ld2(dmx), dmn.data_ptr(), H.ld2(dmn), mx.data_ptr(), H.ld2(mx), L.cnt.data_ptr(),
               red.data_ptr(), x.data_ptr(), H.ld2(x), L.C, c.var_grads[L.w0name].data_ptr(), c.var_grads[L.b0name].data_ptr(), 1.0,
               ws.data_ptr(), ws.numel(), tag="edge_bwd_apply_wgrad_kernel", work=4.0 * (4 * R * F) + 4.0 * R * k,
               nbytes=4.0 * (R * k * F + R * F))
        return
    dUV = torch.empty((R, 2 * F), dtype=torch.float32, device=x.device)    # [dU | dV]
    dysum = dUV[:, :F]
    if L.Y is None:
        assert L.UV is not None          # esrc holds raw pointers into UV: this reference keeps it alive
        dY = torch.empty((R * k, F), dtype=torch.float32, device=x.device)
        H.call("dgcnn_edge_bn_bwd_apply_f32", *L.esrc, L.mean.data_ptr(), L.rstd.data_ptr(), L.beta0.data_ptr(),
               1, dmx.data_ptr(), H.ld2(dmx), dmn.data_ptr(), H.ld2(dmn), mx.data_ptr(), H.ld2(mx), L.cnt.data_ptr(),
               red.data_ptr(), dY.data_ptr(), dysum.data_ptr(), H.ld2(dysum), c.var_grads[L.b0name].data_ptr(), 1.0,
               tag="bn_bwd_apply_kernel<edge>", work=4.0 * (R * k * F + 7 * R * F) + 4.0 * R * k, nbytes=4.0 * (R * k * F + R * F))
    else:
        _edge_bn_bwd_apply_y(c, L, dmx, dmn, red, dysum)
        dY = L.Y
    # dU = sum_m dY, dV = sum of incoming dY;  dWcat = X^T [dU|dV],  dx += [dU|dV] Wcat^T
    _incoming_sum(L, dY, dUV[:, F:], csr)
    _fold_bwd_products(c, L, dUV)


def _fold_bwd_products(c, L, dUV):
    """dx += [dU | dV] Wcat^T on the main stream, dWcat = X^T [dU | dV] folded back into dW0 on the side stream."""
    dwcat = torch.empty((L.Cp, 2 * L.F), dtype=torch.float32, device=dUV.device)
    # dUV / dwcat are allocated on the main stream by the running closure: record them on the side stream,
    # or the caching allocator may hand dUV's block to the next main-stream allocation while the side GEMM reads it
    dx = c.grad(L.x)
    if dx is not None:                                                  # (layer 0, raw coordinates: nobody wants d(points))
        gemm(dUV, L.wcat[:L.C], dx, transB=True, beta=1.0, arith=None)
    with c.off_critical_path(dwcat, dUV, rows=L.R):
        gemm(L.xg, dUV, dwcat, transA=True, arith=None)
        H.call("dgcnn_edge_wgrad_combine_f32", dwcat.data_ptr(), L.C, L.F, c.var_grads[L.w0name].data_ptr())


def _conv0_per_cloud(c, L, outs):
    """The fold with the virtual Y, BatchNorm over the edges of each cloud alone (csrc/seg_bn.hip): no statistics slots, the
    per-cloud sums have buffers of their own.  Returns its scratch (see edge_conv_block)."""
    x, R, k, F, seg = L.x, L.R, L.k, L.F, L.seg
    dev = x.device
    L.Cp, L.xg, L.wcat, L.UV = _point_gemm(c, x, L.W0, R, L.C, F)       # [U | V] = X [Wa-Wb | Wb]
    L.esrc = esrc = (L.UV[:, F:].data_ptr(), 2 * F, L.UV.data_ptr(), 2 * F, L.idx.data_ptr(), R, k, F)
    st = torch.empty(seg.nseg * 2 * F, dtype=torch.float64, device=dev)
    ws = seg_stats_workspace(R, seg.nseg, F, dev)
    H.call("dgcnn_seg_edge_stats_f32", *esrc, seg.device(dev).data_ptr(), seg.nseg, st.data_ptr(), ws.data_ptr(), ws.numel(),
           tag="seg_edge_stats_kernel", work=4.0 * (2 * R * F) + 4.0 * R * k, nbytes=4.0 * (R * k * F + R * F))
    L.mean, L.rstd = seg_bn_finalize(st, seg, F, k)                     # ops.py:53, count n_b * k
    _edge_outputs(c, L, outs)
    if not c.recording:
        H.call("dgcnn_seg_edge_bn_act_kreduce_f32", *esrc, seg.row_group(dev).data_ptr(), L.mean.data_ptr(), L.rstd.data_ptr(),
               L.beta0.data_ptr(), 1, L.mx.data_ptr(), H.ld2(L.mx), L.mn.data_ptr(), H.ld2(L.mn),
               tag="seg_edge_bn_act_kreduce_kernel", work=4.0 * (4 * R * F) + 4.0 * R * k, nbytes=4.0 * (R * k * F + R * F))   # ops.py:54-58
        return st, ws
    # inside a recording: the forward pass that also keeps the packed tie / positive counts, and the tape closure -- per-cloud sums
    # from the per-point outputs (no pass over the edges), the c1 / c2 tables (+ dbeta), dY and dU = sum_m dY, dV = the incoming
    # sum, then the fold's products.  L.UV stays referenced: esrc holds raw pointers into it.
    mean, rstd, beta0, mx, mn = L.mean, L.rstd, L.beta0, L.mx, L.mn
    off, rg = seg.device(dev), seg.row_group(dev)
    cnt = torch.empty((R, F), dtype=torch.float32, device=dev)             # ties of the max + 256 * positives
    H.call("dgcnn_seg_edge_bn_act_kreduce_cnt_f32", *esrc, rg.data_ptr(), mean.data_ptr(), rstd.data_ptr(), beta0.data_ptr(), 1,
           mx.data_ptr(), H.ld2(mx), mn.data_ptr(), H.ld2(mn), cnt.data_ptr(),
           tag="seg_edge_bn_act_kreduce_kernel<cnt>", work=4.0 * (5 * R * F) + 4.0 * R * k, nbytes=4.0 * (R * k * F + R * F))   # ops.py:54-58
    csr = _csr_ahead(c, L)

    def bwd():
        assert L.UV is not None
        dmm = c.grad(L.mm)
        if dmm is None:
            return
        dmx, dmn = dmm[:, :F], dmm[:, F:]
        red = torch.empty(seg.nseg * 2 * F, dtype=torch.float64, device=dev)
        wsb = seg_stats_workspace(R, seg.nseg, F, dev)
        H.call("dgcnn_seg_edge_bn_bwd_reduce_points_f32", mx.data_ptr(), H.ld2(mx), mn.data_ptr(), H.ld2(mn), cnt.data_ptr(),
               dmx.data_ptr(), H.ld2(dmx), dmn.data_ptr(), H.ld2(dmn), beta0.data_ptr(), R, k, F, off.data_ptr(), seg.nseg,
               red.data_ptr(), wsb.data_ptr(), wsb.numel(), tag="seg_edge_bwd_reduce_points_kernel", work=4.0 * 5 * R * F)
        c1, c2 = seg_bn_bwd_finalize(red, seg, F, k, c.var_grads[L.b0name])
        dUV = torch.empty((R, 2 * F), dtype=torch.float32, device=dev)     # [dU | dV]
        dY = torch.empty((R * k, F), dtype=torch.float32, device=dev)
        H.call("dgcnn_seg_edge_bn_bwd_apply_f32", *esrc, rg.data_ptr(), mean.data_ptr(), rstd.data_ptr(), beta0.data_ptr(), 1,
               dmx.data_ptr(), H.ld2(dmx), dmn.data_ptr(), H.ld2(dmn), mx.data_ptr(), H.ld2(mx), cnt.data_ptr(), c1.data_ptr(),
               c2.data_ptr(), dY.data_ptr(), dUV.data_ptr(), 2 * F, tag="seg_edge_bn_bwd_apply_kernel",
               work=4.0 * (R * k * F + 7 * R * F) + 4.0 * R * k, nbytes=4.0 * (R * k * F + R * F))
        adj = csr if csr is not None else build_csr(L.idx, 1, R, k)
        _incoming_sum(L, dY, dUV[:, F:], adj)
        _fold_bwd_products(c, L, dUV)
    c.tape.append(bwd)
    return st, ws


def _conv0_bf16_fused(c, L, st, outs, one_pass):
    """csrc/edge_mlp_bf16.hip: E = [x_i, x_j - x_i] gathered, rounded and multiplied tile by tile on the bf16 MFMA pipe;
    neither E nor y is written: one pass takes the BatchNorm sums, the next one recomputes y for BN + ReLU + max / mean.
    one_pass: the backward in one pass over the edges (8 <= k <= 128): the forward then packs (#ties, #positives) as the fp32 edge
    kernels do.  Otherwise the backward forms Y again and goes the way of the forms that wrote it (_conv0_dense_y_bwd)."""
    R, C, k, F, bsrc = L.R, L.C, L.k, L.F, L.bsrc
    H.call("dgcnn_edge_mlp_bf16_stats", *bsrc, st.data_ptr(), tag="edge_mlp_bf16_kernel<stats>",
           work=2.0 * R * k * 2 * C * F, nbytes=4.0 * (R * k * C + R * C))
    _edge_finalize(c, L, st, outs)
    mx, mn = L.mx, L.mn
    H.call("dgcnn_edge_mlp_bf16_bn_kreduce", *bsrc, L.mean.data_ptr(), L.rstd.data_ptr(), L.beta0.data_ptr(),
           mx.data_ptr(), H.ld2(mx), mn.data_ptr(), H.ld2(mn), H._p(L.cnt), 1 if one_pass else 0,
           tag="edge_mlp_bf16_kernel<bn_kreduce>", work=2.0 * R * k * 2 * C * F, nbytes=4.0 * (R * k * C + R * C))   # ops.py:53-58
    if c.recording:
        _record(c, _conv0_bf16_one_pass_bwd if one_pass else _conv0_dense_y_bwd, L)


def _conv0_bf16_one_pass_bwd(c, L):
    """Sums of the BatchNorm backward from the forward's per-point outputs, then ONE pass over the edges that recomputes y, forms
    dY (rounded to bf16), takes dW0 = E^T dY on the matrix pipe and leaves dY as bf16 for the transposed-adjacency sum -- E, y
    and an fp32 dY are never written."""
    g = _edge_bwd_inputs(c, L)
    if g is None:
        return
    dmx, dmn, red = g
    x, R, C, k, F, mx = L.x, L.R, L.C, L.k, L.F, L.mx
    _edge_reduce_points(L, dmx, dmn, red)
    dx = c.grad(x)
    dYb = dysum = None
    if dx is not None:
        dYb = torch.empty((R * k, F), dtype=torch.bfloat16, device=x.device)
        dysum = torch.empty((R, F), dtype=torch.float32, device=x.device)
    ws = c.workspace()
    H.call("dgcnn_edge_mlp_bf16_bwd", *L.bsrc, L.mean.data_ptr(), L.rstd.data_ptr(), L.beta0.data_ptr(), mx.data_ptr(), H.ld2(mx),
           L.cnt.data_ptr(), dmx.data_ptr(), H.ld2(dmx), dmn.data_ptr(), H.ld2(dmn), red.data_ptr(), H._p(dYb), H._p(dysum),
           F, c.var_grads[L.w0name].data_ptr(), c.var_grads[L.b0name].data_ptr(), 1.0, ws.data_ptr(), ws.numel(),
           tag="edge_mlp_bf16_kernel<bwd>", work=2.0 * R * k * 2 * C * F * 2, nbytes=4.0 * (R * k * C + R * C))
    if dx is not None:
        _edge_dx(L, dx, dysum, dYb, bf16=True)


def _bf16_operands(L):
    """The literal edge tensor in fp32 (the difference x_j - x_i BEFORE any rounding; channels padded to a multiple of 4 so
    that the products take the float4 path) and the matching weight rows -- the operands the bf16 products round.
    dgcnn_gemm_f32 rounds its operands (arith = 1) only on its float4 path with N > 4 (include/dgcnn_hip.h); where the products
    E W0 and E^T dY (both N = F) will not take it, E and the weight are rounded here instead: rounded values are bf16 values, so
    the fp32 product of them is the mode's arithmetic.  (Rounding is idempotent: the other shapes see the same bits as before.)"""
    x, W0, R, C, Cp, k, F = L.x, L.W0, L.R, L.C, L.Cp, L.k, L.F
    xg, Wp = x, W0
    if Cp != C:
        xg = H.zeros((R, Cp), torch.float32, x.device)
        H.call("dgcnn_copy2d_f32", x.data_ptr(), H.ld2(x), xg.data_ptr(), Cp, R, C, 0)
        Wp = H.zeros((2 * Cp, F), torch.float32, x.device)
        H.call("dgcnn_copy2d_f32", W0[:C].data_ptr(), F, Wp[:C].data_ptr(), F, C, F, 0)
        H.call("dgcnn_copy2d_f32", W0[C:].data_ptr(), F, Wp[Cp:Cp + C].data_ptr(), F, C, F, 0)
    E_ = torch.empty((R * k, 2 * Cp), dtype=torch.float32, device=x.device)
    H.call("dgcnn_edge_gather_f32", xg.data_ptr(), H.ld2(xg), L.idx.data_ptr(), L.B, L.N, Cp, k, E_.data_ptr())   # ops.py:21-40
    if not (F % 4 == 0 and F > 4 and H.ld2(Wp) % 4 == 0 and Wp.data_ptr() % 16 == 0):
        H.call("dgcnn_round_bf16_f32", E_.data_ptr(), E_.data_ptr(), E_.numel())
        Wr = torch.empty((Wp.shape[0], F), dtype=torch.float32, device=x.device)      # (never W0 itself: a variable)
        Wc = Wp.contiguous()
        H.call("dgcnn_round_bf16_f32", Wc.data_ptr(), Wr.data_ptr(), Wr.numel())
        Wp = Wr
    return E_, Wp


def _conv0_dense_y(c, L, st, outs):
    """conv0 written out as Y (R*k, F), L.kind one of
      "bf16"     shapes the fused bf16 kernels do not take: the edge tensor in fp32, then ONE product whose operands the GEMM rounds
                 to bf16 (arith = 1: v_cvt_pk_bf16_f32, round to nearest even) with fp32 accumulation on the bf16 MFMA pipe
      "literal"  the (B*N*k) x 2C product over E = [x_i, x_j - x_i], the gather fused into the GEMM's loads
      "nbr"      factored conv0, edge-level form (kept for odd F and as a cross-check): centre term once per point (U); the
                 per-edge (B*N*k) x C GEMM gathers the neighbour rows and adds U[point] in its epilogue
    then BatchNorm streams Y.  The members differ only in how Y and dW0 are produced.  Returns the forward's scratch."""
    x, W0, R, C, k, F, idx = L.x, L.W0, L.R, L.C, L.k, L.F, L.idx
    L.Y = Y = torch.empty((R * k, F), dtype=torch.float32, device=x.device)
    U = None
    edge_tag = "gemm_kernel<A_EDGE,B_ROW,STORE,%d,%d>" % (_tile_m(R * k, F), 64 if F <= 64 else 128)
    if L.kind == "bf16":
        L.Ee, L.W0p = _bf16_operands(L)
        gemm(L.Ee, L.W0p, Y, stats=None if DETERMINISTIC else st, arith=1)                                      # ops.py:47-52
    elif L.kind == "literal":
        H.call("dgcnn_edge_mlp_f32", x.data_ptr(), H.ld2(x), idx.data_ptr(), W0.data_ptr(), L.B, L.N, C, k, F,
               Y.data_ptr(), 0 if DETERMINISTIC else st.data_ptr(), tag=edge_tag,
               work=2.0 * R * k * 2 * C * F)                            # ops.py:21-52 (gather fused)
    else:
        L.wd, _ = _centre_weight(W0, C, F)
        U = torch.empty((R, F), dtype=torch.float32, device=x.device)
        gemm(x, L.wd, U)
        H.call("dgcnn_edge_nbr_gemm_f32", x.data_ptr(), H.ld2(x), idx.data_ptr(), W0[C:].data_ptr(), U.data_ptr(), F,
               L.B, L.N, C, k, F, Y.data_ptr(), 0 if DETERMINISTIC else st.data_ptr(), tag=edge_tag,
               work=2.0 * R * k * C * F)                                # ops.py:21-52 (gather fused)
    if DETERMINISTIC:
        colstats_det(Y, st)
    if not c.recording:
        L.Ee = None
    _edge_finalize(c, L, st, outs)
    _edge_bn_act_y(L)
    if c.recording:
        _record(c, _conv0_dense_y_bwd, L)
    return U


def _conv0_dense_y_bwd(c, L):
    g = _edge_bwd_inputs(c, L)
    if g is None:
        return
    dmx, dmn, red = g
    x, R, C, Cp, k, F, idx, kind = L.x, L.R, L.C, L.Cp, L.k, L.F, L.idx, L.kind
    recompute = L.Y is None
    if recompute:
        # the fused bf16 forward wrote neither E nor y: both are formed again for the backward (y by the SAME instruction sequence,
        # so the recomputed z compares equal to the maxima the forward took), used by the passes below and dropped
        L.Y = torch.empty((R * k, F), dtype=torch.float32, device=x.device)
        H.call("dgcnn_edge_mlp_bf16", *L.bsrc, L.Y.data_ptr(), tag="edge_mlp_bf16_kernel<write>",
               work=2.0 * R * k * 2 * C * F, nbytes=4.0 * (R * k * C + R * C))
        L.Ee, L.W0p = _bf16_operands(L)
    _edge_bn_bwd_reduce_y(L, dmx, dmn, red)
    dx = c.grad(x)
    dysum = None
    if dx is not None or kind == "nbr":
        dysum = torch.empty((R, F), dtype=torch.float32, device=x.device)
    _edge_bn_bwd_apply_y(c, L, dmx, dmn, red, dysum, relu=3 if kind == "bf16" else 1)
    dY = L.Y
    ws = c.workspace()
    dW0 = c.var_grads[L.w0name]
    wgrad_tag = "edge_wgrad_smallc_kernel" if C <= 4 else "gemm_kernel<A_EDGE_T,B_ROW,STORE,128,%d>" % (64 if F <= 64 else 128)
    if kind == "bf16":
        # dW0 = E^T dY with bf16 operands: E and W0 rounded as in the forward; dY was written on the bf16 grid by the
        # apply pass (relu flag 3), so the product's own rounding (arith = 1) leaves it unchanged
        if L.W0p is L.W0:
            gemm(L.Ee, dY, dW0, transA=True, beta=1.0, arith=1)
        else:
            dWp = torch.empty_like(L.W0p)
            gemm(L.Ee, dY, dWp, transA=True, arith=1)
            H.call("dgcnn_copy2d_f32", dWp[:C].data_ptr(), F, dW0[:C].data_ptr(), F, C, F, 1)
            H.call("dgcnn_copy2d_f32", dWp[Cp:Cp + C].data_ptr(), F, dW0[C:].data_ptr(), F, C, F, 1)
    elif kind == "literal":
        H.call("dgcnn_edge_mlp_wgrad_f32", x.data_ptr(), H.ld2(x), idx.data_ptr(), dY.data_ptr(), L.B, L.N, C, k, F,
               dW0.data_ptr(), 1.0, ws.data_ptr(), ws.numel(), tag=wgrad_tag, work=2.0 * R * k * 2 * C * F)
    else:
        # dW0[C:] += sum_e x_j^T dY  -  X^T dYsum ;  dW0[:C] += X^T dYsum   (W0[:C]-W0[C:] and W0[C:] are the
        # factors of the forward: d(Wa-Wb) = X^T dYsum, dWb = edge part)
        H.call("dgcnn_edge_nbr_wgrad_f32", x.data_ptr(), H.ld2(x), idx.data_ptr(), dY.data_ptr(), L.B, L.N, C, k, F,
               dW0[C:].data_ptr(), 1.0, ws.data_ptr(), ws.numel(), tag=wgrad_tag, work=2.0 * R * k * C * F)
        dwd = torch.empty((C, F), dtype=torch.float32, device=x.device)
        gemm(x, dysum, dwd, transA=True)
        H.call("dgcnn_axpby_f32", dwd.data_ptr(), 1.0, dW0[:C].data_ptr(), 1.0, C * F)
        H.call("dgcnn_axpby_f32", dwd.data_ptr(), -1.0, dW0[C:].data_ptr(), 1.0, C * F)
    if dx is not None:
        _edge_dx(L, dx, dysum, dY, bf16=kind == "bf16", wd=L.wd)
    if recompute:
        dY = L.Y = L.Ee = None              # (recomputed for this backward only)


def edge_conv_block(x, B, N, k, num_filters, relu1=True, outs=None, net2=None, seed=None, seg=None):
    """x: (B*N, C) view.  Returns (mm, net, idx): mm = (R,2F) [max | mean], net = (R,64).
    outs = (mm_view, net_view) destination slices (model path) or None (fresh buffers).
    seed: the previous EdgeConv layer's graph (B,N,k') or None: seeds this layer's k-NN filter (same result, fewer inserts).
    seg: a packed tower (Segments) with B = 1, N = R: only the k-NN is tied to a cloud (idx holds tower rows), every other pass is
    row-wise -- BatchNorm statistics run over all rows of the tower, as in a dense (B, N) tower; seg.bn_per_cloud: over the rows
    (conv0: the edges) of each cloud alone -- only the default form of conv0 (the fold with the virtual Y); recorded only with
    seg.bn_per_cloud_train (the general backward: dY is written, the fused layer-0 pass has no per-cloud form).
    conv0: one of _conv0_per_cloud / _fold / _bf16_fused / _dense_y -- its forward into L.mm and, in a recording, its backward."""
    c = ctx()
    R, C = x.shape
    F = int(num_filters)
    if seg is not None:
        if B != 1 or N != seg.rows:
            raise ValueError("a packed tower is one (1, R) block: got B=%d N=%d for %d rows" % (B, N, seg.rows))
        seg.check_k(k)
    if k > N:
        raise ValueError("k_nn: k=%d > N=%d (tf.nn.top_k raises InvalidArgument)" % (k, N))
    bpc = per_cloud(seg)
    if bpc:
        # every form of conv0 the per-cloud kernels do not take is refused here, on the host, before any launch
        if EDGE_MLP_DTYPE == "bf16" or EDGE_MLP_LITERAL or EDGE_MLP_NBR_GEMM or EDGE_MATERIALIZE_Y:
            raise ValueError("per-cloud BatchNorm takes the default conv0 only (fp32 fold, virtual edge tensor): EDGE_MLP_DTYPE=%r, "
                             "literal / neighbour-GEMM / materialised switches off" % (EDGE_MLP_DTYPE,))
        if F % 4 != 0 or F > 1024 or k >= 256:
            raise ValueError("per-cloud BatchNorm needs EdgeConv filter counts that are multiples of 4, <= 1024, and k < 256 "
                             "(got F=%d, k=%d)" % (F, k))
        if R >= 1 << 24 or 2 * F * R >= 1 << 32:
            raise ValueError("per-cloud BatchNorm: a tower of %d rows x %d filters exceeds the 32-bit row offsets of the gather" % (R, F))
    with variable_scope("conv0"):
        w0name, W0 = c.get_variable("weights", (2 * C, F))
        b0name, beta0 = c.get_variable("BatchNorm/beta", (F,))
    # the layer's state: what conv0's passes and its tape closure read (the closure keeps every tensor in it alive)
    L = SimpleNamespace(x=x, B=B, N=N, R=R, C=C, Cp=(C + 3) // 4 * 4, k=k, F=F, seg=seg, W0=W0, beta0=beta0, w0name=w0name,
                        b0name=b0name, Y=None, UV=None, Ee=None, W0p=None, wd=None)
    scratch = None
    if bpc:
        L.idx = idx = knn(x, B, N, k, seed=seed, seg=seg)                   # ops.py:8-19
        scratch = _conv0_per_cloud(c, L, outs)
    else:
        c.push_slots(c.step_slots)               # conv0's statistics come from passes whose grids FOLLOW the slot count: the maximum
        st = c.stats(F)
        L.idx = idx = knn(x, B, N, k, seed=seed, seg=seg)                   # ops.py:8-19
        bf16 = EDGE_MLP_DTYPE == "bf16"
        fold = not (EDGE_MLP_LITERAL or bf16 or EDGE_MLP_NBR_GEMM) and F % 4 == 0 and F <= 1024
        # conv0 output never written: recomputed from (V, U, idx) (the edge BN passes pack tie / positive counts: k < 256)
        virtual = fold and not EDGE_MATERIALIZE_Y and k < 256
        # the fused bf16 kernels write neither E nor y: decided BEFORE anything of (R*k, F) is allocated (1.3 GB per layer at configs[2])
        fused_bf16 = (bf16 and bool(H.load().dgcnn_edge_mlp_bf16_supported(C, k, F)) and W0.is_contiguous() and
                      (C <= 4 or (H.ld2(x) % 4 == 0 and x.data_ptr() % 16 == 0)))
        if fold:
            _conv0_fold(c, L, st, outs, virtual)
        elif fused_bf16:
            L.kind = "bf16"
            L.bsrc = (x.data_ptr(), H.ld2(x), idx.data_ptr(), W0.data_ptr(), B, N, C, k, F)
            _conv0_bf16_fused(c, L, st, outs, one_pass=(c.recording and BF16_FUSED_BWD and
                                                        bool(H.load().dgcnn_edge_mlp_bf16_bwd_supported(C, k, F))))
        else:
            L.kind = "bf16" if bf16 else "literal" if EDGE_MLP_LITERAL else "nbr"
            scratch = _conv0_dense_y(c, L, st, outs)
    # (scratch, and L outside a recording: the forward's temporaries stay allocated until conv1 has been issued)
    net = conv_bn_act(L.mm, "conv1", 64, relu=relu1, out=L.net_out, out2=net2, arith=None, seg=seg if bpc else None)   # ops.py:62-70 (64 hard-coded)
    return L.mm, net, idx


# ----------------------------------------------------------------------------------------------
# residual add (ops.py:134), dropout (model.py:91), global max-pool (model.py:76-81)
# ----------------------------------------------------------------------------------------------
def add_relu(a, b, out=None):
    c = ctx()
    R, F = a.shape
    if tuple(b.shape) != (R, F):
        raise ValueError("residual shortcut shape mismatch %s vs %s (ops.py:134)" % (tuple(a.shape), tuple(b.shape)))
    if out is None:
        out = c.new_buffer(R, F)
    H.call("dgcnn_add_relu_f32", a.data_ptr(), H.ld2(a), b.data_ptr(), H.ld2(b), R, F, out.data_ptr(), H.ld2(out))
    if c.recording:
        def bwd():
            dout = c.grad(out)
            if dout is None:
                return
            d = torch.empty((R, F), dtype=torch.float32, device=a.device)
            H.call("dgcnn_relu_bwd_f32", dout.data_ptr(), H.ld2(dout), out.data_ptr(), H.ld2(out), R, F, d.data_ptr(), F)
            for t in (a, b):
                g = c.grad(t)
                if g is not None:
                    H.call("dgcnn_copy2d_f32", d.data_ptr(), F, g.data_ptr(), H.ld2(g), R, F, 1)
        c.tape.append(bwd)
    return out


def dropout(x, keep=DROPOUT_KEEP):
    c = ctx()
    R, F = x.shape
    assert x.is_contiguous()
    out = c.new_buffer(R, F)
    if c.seed_dev is None:
        c.advance_seed()
    seed = c.seed_dev                       # device-resident: the backward regenerates the mask from the same value
    H.call("dgcnn_dropout_dev_f32", x.data_ptr(), out.data_ptr(), R * F, float(keep), seed.data_ptr())
    if c.recording:
        def bwd():
            dout = c.grad(out)
            if dout is None:
                return
            dx, bx = c.grad_w(x)
            if dx is None:
                return
            if bx == 0.0:                                   # first touch of d(x): write the masked gradient in place
                H.call("dgcnn_dropout_dev_f32", dout.data_ptr(), dx.data_ptr(), R * F, float(keep), seed.data_ptr())
                return
            tmp = torch.empty_like(dout)
            H.call("dgcnn_dropout_dev_f32", dout.data_ptr(), tmp.data_ptr(), R * F, float(keep), seed.data_ptr())
            H.call("dgcnn_copy2d_f32", tmp.data_ptr(), F, dx.data_ptr(), H.ld2(dx), R, F, 1)
        c.tape.append(bwd)
    return out


def tile_rows(g, out, rows, seg=None):
    """tf.tile of a per-cloud (B,F) tensor over the `rows` points of its cloud into the (B*rows, F) view `out` (model.py:80-81);
    backward: tf.tile^T = the sum over the cloud.  seg: a packed tower (Segments): row r receives the row of its own cloud
    (`rows` is ignored)."""
    c = ctx()
    G, F = g.shape
    if seg is not None:
        if G != seg.nseg or out.shape[0] != seg.rows:
            raise ValueError("tile_rows: %d clouds / %d rows for a packed tower of %d / %d" % (G, out.shape[0], seg.nseg, seg.rows))
        H.call("dgcnn_tile_rows_seg_f32", g.data_ptr(), H.ld2(g), seg.row_group(g.device).data_ptr(), seg.rows, F, out.data_ptr(),
               H.ld2(out))
    else:
        H.call("dgcnn_tile_rows_f32", g.data_ptr(), H.ld2(g), G, int(rows), F, out.data_ptr(), H.ld2(out))
    if c.recording:
        def bwd():
            dout, dg_ = c.grad(out), c.grad(g)
            if dout is None or dg_ is None:
                return
            tmp = torch.empty((G, F), dtype=torch.float32, device=g.device)
            if seg is not None:
                seg_colsum(dout, seg, tmp)
            else:
                H.call("dgcnn_group_colsum_f32", dout.data_ptr(), H.ld2(dout), G, int(rows), F, tmp.data_ptr())
            H.call("dgcnn_copy2d_f32", tmp.data_ptr(), F, dg_.data_ptr(), H.ld2(dg_), G, F, 1)
        c.tape.append(bwd)
    return out


def global_max(x, B, N, seg=None):
    """(B*N,F) -> (B,F) max over the points of each cloud, first arg-max remembered for the backward.
    seg: a packed tower (Segments; B, N ignored): (rows,F) -> (nseg,F), the max over each cloud's own rows."""
    c = ctx()
    F = x.shape[1]
    if seg is not None:
        if x.shape[0] != seg.rows:
            raise ValueError("offsets end at %d, the tower has %d rows" % (seg.rows, x.shape[0]))
        B = seg.nseg
        off = seg.device(x.device)
        out = c.new_buffer(B, F)
        arg = torch.empty((B, F), dtype=torch.int32, device=x.device)
        keys = c.stats_raw(B * F)
        H.call("dgcnn_colmax_seg_f32", x.data_ptr(), H.ld2(x), seg.rows, F, off.data_ptr(), B, keys.data_ptr())
        H.call("dgcnn_colmax_decode_f32", keys.data_ptr(), B * F, out.data_ptr(), arg.data_ptr())
        if c.recording:
            def bwd_seg():
                dout = c.grad(out)
                dx = c.grad(x)
                if dout is None or dx is None:
                    return
                H.call("dgcnn_global_max_bwd_seg_f32", dout.data_ptr(), arg.data_ptr(), off.data_ptr(), B, F, dx.data_ptr(), H.ld2(dx))
            c.tape.append(bwd_seg)
        return out
    out = c.new_buffer(B, F)
    arg = torch.empty((B, F), dtype=torch.int32, device=x.device)
    H.call("dgcnn_global_max_f32", x.data_ptr(), H.ld2(x), B, N, F, out.data_ptr(), arg.data_ptr())
    if c.recording:
        def bwd():
            dout = c.grad(out)
            dx = c.grad(x)
            if dout is None or dx is None:
                return
            H.call("dgcnn_global_max_bwd_f32", dout.data_ptr(), arg.data_ptr(), B, N, F, dx.data_ptr(), H.ld2(dx))
        c.tape.append(bwd)
    return out


def plain_gemm(a, leaf_scope_weight, w_rows, Cout):
    """out = a @ W[lo:hi]  (the per-cloud part of FC0: global feature x its 1024 weight rows)."""
    c = ctx()
    wname, W = leaf_scope_weight
    Wx = W[w_rows[0]:w_rows[1]]
    out = c.new_buffer(a.shape[0], Cout)
    gemm(a, Wx, out)
    if c.recording:
        def bwd():
            dout = c.grad(out)
            if dout is None:
                return
            gemm(a, dout, c.var_grads[wname][w_rows[0]:w_rows[1]], transA=True, beta=1.0)
            da = c.grad(a)
            if da is not None:
                gemm(dout, Wx, da, transB=True, beta=1.0)
        c.tape.append(bwd)
    return out


# ----------------------------------------------------------------------------------------------
# dgcnn/trainval.py:39-52 softmax / accuracy / loss (+ the seed of the backward pass)
# ----------------------------------------------------------------------------------------------
def mark_head_gradients_complete():
    """Tape marker placed (in forward order) right after the EdgeConv stack: in the backward it runs when every closure of
    the head (MergedEdgeConv, FC*, Final) has run, i.e. when the head's share of the gradient bucket is final."""
    c = ctx()
    if not c.recording:
        return

    def bwd():
        hook, c.head_grads_hook = c.head_grads_hook, None
        if hook is not None:
            hook()
    c.tape.append(bwd)


def softmax_loss(logits2d, labels, weight, want_grad, seg=None, per_cloud=False):
    """-> (softmax (R,ncls), scal tensor [loss, accuracy] on device).  Seeds d(logits) if want_grad.
    per_cloud with a Segments `seg`: loss, accuracy and the seed are taken cloud by cloud (csrc/seg_loss.hip) -- scal is the mean
    over the clouds of the per-cloud means, d(logits) the sum of their gradients, what nseg micro-steps of -mbs 1 add up to -- and
    the (nseg, 2) device tensor [loss, accuracy] of every cloud is returned as a third value (None without labels)."""
    c = ctx()
    R, ncls = logits2d.shape
    assert logits2d.is_contiguous()
    dev = logits2d.device
    lt = c.loss_tail
    if lt is not None and not (lt["out"].data_ptr() == logits2d.data_ptr() and tuple(lt["out"].shape) == (R, ncls) and
                               not (per_cloud and seg is not None)):
        lt = None
    if lt is None:
        flush_class_tail(c)                     # (not the held-back logits: whatever is pending runs on its own)
    else:
        c.loss_tail = None
    sm = torch.empty((R, ncls), dtype=torch.float32, device=dev)
    dl = None
    if want_grad:
        dl, _ = c.grad_w(logits2d)          # (written, not accumulated: a first touch of a whole root needs no zero fill)
        assert dl is not None and dl.is_contiguous()
    if per_cloud and seg is not None:
        if seg.rows != R:
            raise ValueError("softmax_loss: the offsets end at %d, the logits have %d rows" % (seg.rows, R))
        cs = None
        scal = torch.empty(2, dtype=torch.float32, device=dev)      # (written by the call, as cloud_scal is)
        ws = None
        if labels is not None:
            cs = torch.empty((seg.nseg, 2), dtype=torch.float32, device=dev)
            need = int(H.load().dgcnn_seg_softmax_xent_workspace_bytes(R, seg.nseg))
            ws = c.workspace()
            if ws.numel() < need:
                ws = torch.empty(need, dtype=torch.uint8, device=dev)
        else:
            H.memset(scal)                  # (no labels: nothing writes the scalars; keep the dense call's zeros)
        H.call("dgcnn_seg_softmax_xent_f32", logits2d.data_ptr(), H._p(labels), H._p(weight), R, ncls, seg.device(dev).data_ptr(),
               seg.nseg, sm.data_ptr(), H._p(dl), H._p(cs), scal.data_ptr(), H._p(ws), 0 if ws is None else ws.numel())
        return sm, scal, cs
    if lt is not None:
        # F2: folds the Final layer's statistics slots (mean / rstd for the backward), applies its BatchNorm + ReLU -> logits2d,
        # then softmax / seed / loss / accuracy as below; [loss, accuracy] were zeroed by F1
        prev = H.stat_slots()
        if lt["nslots"] != prev:
            H.set_stat_slots(lt["nslots"])
        try:
            H.call("dgcnn_bn_softmax_xent_f32", lt["T"].data_ptr(), lt["st"].data_ptr(), float(R), BN_EPS, lt["beta"].data_ptr(),
                   int(lt["relu"]), R, ncls, lt["mean"].data_ptr(), lt["rstd"].data_ptr(), logits2d.data_ptr(), H._p(labels),
                   H._p(weight), sm.data_ptr(), H._p(dl), lt["scal"].data_ptr(), tag="bn_softmax_xent_kernel", work=4.0 * R * ncls * 4)
        finally:
            if lt["nslots"] != prev:
                H.set_stat_slots(prev)
        return sm, lt["scal"]
    scal = H.zeros(2, torch.float32, dev)      # (its own tensor: the caller reads it after later towers' begin_step)
    H.call("dgcnn_softmax_xent_f32", logits2d.data_ptr(), H._p(labels), H._p(weight), R, ncls, sm.data_ptr(),
           H._p(dl), scal.data_ptr())
    return sm, scal

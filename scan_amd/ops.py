"""torch.autograd wrappers around the C ABI (include/scan_hip.h).

PyTorch is plumbing here: it owns device memory, the current HIP stream and the
autograd tape; all arithmetic of the ops below happens in libscan_hip.so.
Every op requires CUDA(HIP) tensors and raises otherwise -- there is no CPU
fallback in the product path.

Activations are "pyramids": a contiguous fp32 matrix [M, Cs] (rows = pixels in
level-major / image / y / x order, Cs = channel stride, a multiple of 4) plus a
``PyramidShape`` describing how rows split into levels (see include/scan_hip.h).
"""
import contextlib
import ctypes
import os
import weakref

import torch

from . import _lib
from ._lib import PyramidDesc, call, query


# ----------------------------------------------------------------------------- plumbing
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    # the raw handle of torch's current stream on the current device; the Python-level torch.cuda.current_stream() builds a
    # Stream object per call (~10 us, 900 calls per training step)
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


def _chk(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("scan_amd ops run only on the GPU (HIP) -- got a %s tensor; no CPU fallback" % t.device)
        if t.dtype == torch.float32 and not t.is_contiguous():
            raise RuntimeError("scan_amd op got a non-contiguous tensor")


def pad4(c):
    return (c + 3) // 4 * 4


def _level_table(who, shape, ctype, values, what, per_level=1):
    """the host table of a per-level quantity (strides, anchor sizes, sizes of interest, counts) as the ctypes array the library
    reads: ``per_level`` entries for each of the shape's levels"""
    values = list(values)
    if len(values) != per_level * shape.n_levels:
        raise ValueError("%s: %d %s for a pyramid of %d levels" % (who, len(values) // per_level, what, shape.n_levels))
    return (ctype * len(values))(*[(float if ctype is ctypes.c_float else int)(v) for v in values])


# ----------------------------------------------------------------------------- deterministic mode
# scan_tune "deterministic" (SCAN_TUNE=deterministic=1) lives in the library and is the only copy of the switch: it is read
# at every call that chooses between an atomic reduction and its *_ordered twin, never cached -- for the losses and the conv
# epilogue's GroupNorm sums here (_call_reduction, _Conv2d), for GroupNorm itself in the library (scan_groupnorm_plan, which
# this module and the compiled scan_ops module both ask).  With it on, two runs from one seed end with the same bits
# (DESIGN.md section 4).
def deterministic():
    return query("scan_tune_get", b"deterministic") == 1


def set_deterministic(flag):
    """switch the ordered reductions on / off; returns the previous setting (as scan_tune does)"""
    return query("scan_tune", b"deterministic", 1 if flag else 0) == 1


def _partials(name, like, *args):
    """the per-workgroup slots of an *_ordered call (name: its *_ordered_ws_floats query): one fresh buffer per call, so
    calls on side streams never share one; not cleared -- every workgroup of the launch writes all of its slots"""
    return torch.empty((max(int(query(name, *args)), 1),), dtype=torch.float32, device=like.device)


def _call_reduction(base, fwd, like, ws_args, *args):
    """a loss forward that ends in a sum: ``base + fwd`` with atomics, or in deterministic mode its *_ordered twin (the same
    arguments + the per-workgroup slots before the stream; base + "_ordered_ws_floats"(*ws_args) sizes them)"""
    if deterministic():
        call(base + fwd + "_ordered", *args, _ptr(_partials(base + "_ordered_ws_floats", like, *ws_args)), _stream())
    else:
        call(base + fwd, *args, _stream())


class KernelTimer:
    """Optional HIP-event timing of the MFMA conv launches on the stream they run on (bench.py uses it
    for the live roofline figure).  Disabled by default: no events are recorded."""

    def __init__(self):
        self.enabled = False
        self.records = {}

    def begin(self, name, flops):
        if not self.enabled:
            return None
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.records.setdefault(name, []).append((s, e, flops))
        s.record(torch.cuda.current_stream())
        return e

    def end(self, e):
        if e is not None:
            e.record(torch.cuda.current_stream())

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, recs in self.records.items():
            ms = sum(s.elapsed_time(e) for s, e, _ in recs)
            fl = sum(f for _, _, f in recs)
            out[name] = {"launches": len(recs), "total_ms": ms, "avg_ms": ms / len(recs), "flops": fl,
                         "tflops": fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0}
        return out

    def reset(self):
        self.records = {}


kernel_timer = KernelTimer()


class PyramidShape:
    """Level table of a pyramid activation (mirrors scan_pyramid_t)."""

    def __init__(self, n_images, sizes):
        self.n_images = int(n_images)
        self.sizes = [(int(h), int(w)) for h, w in sizes]
        self.row_off = [0]
        for h, w in self.sizes:
            self.row_off.append(self.row_off[-1] + self.n_images * h * w)
        d = PyramidDesc()
        d.n_levels = len(self.sizes)
        d.n_images = self.n_images
        for i, (h, w) in enumerate(self.sizes):
            d.h[i], d.w[i] = h, w
        for i, o in enumerate(self.row_off):
            d.row_off[i] = o
        self.desc = d

    @property
    def rows(self):
        return self.row_off[-1]

    @property
    def n_levels(self):
        return len(self.sizes)

    def level(self, l):
        return PyramidShape(self.n_images, [self.sizes[l]])

    def conv_out(self, ksize, stride):
        pad = ksize // 2
        return PyramidShape(self.n_images, [((h + 2 * pad - ksize) // stride + 1, (w + 2 * pad - ksize) // stride + 1)
                                            for h, w in self.sizes])

    def ref(self):
        return ctypes.byref(self.desc)

    def __eq__(self, o):
        return isinstance(o, PyramidShape) and self.n_images == o.n_images and self.sizes == o.sizes

    def __repr__(self):
        return "PyramidShape(N=%d, %s)" % (self.n_images, self.sizes)


def nchw_to_rows(x, cs=None):
    """[N,C,H,W] -> ([N*H*W, Cs] rows, PyramidShape); zero-pads channels to Cs."""
    N, C, H, W = x.shape
    cs = cs or pad4(C)
    rows = x.permute(0, 2, 3, 1).reshape(N * H * W, C)
    if cs != C:
        rows = torch.nn.functional.pad(rows, (0, cs - C))
    return rows.contiguous(), PyramidShape(N, [(H, W)])


def rows_to_nchw(rows, shape, l=0, c=None):
    """view of level l as a logical [N,C,H,W] tensor (channels_last strides)."""
    h, w = shape.sizes[l]
    r = rows[shape.row_off[l]:shape.row_off[l + 1]]
    if c is not None:
        r = r[:, :c]
    return r.view(shape.n_images, h, w, r.shape[1]).permute(0, 3, 1, 2)


# ----------------------------------------------------------------------------- weights
def pack_weight(weight, cs):
    """[Cout,Cin,k,k] parameter -> [Cout, k*k, Cs] fp32 ("OHWI").  Zero-copy when the
    parameter is stored channels_last and Cin == Cs."""
    co, ci, kh, kw = weight.shape
    w = weight.permute(0, 2, 3, 1)  # [Cout,k,k,Cin]
    if ci == cs and w.is_contiguous():
        return w.reshape(co, kh * kw, ci)
    out = weight.new_zeros(co, kh * kw, cs)
    out[:, :, :ci] = w.reshape(co, kh * kw, ci)
    return out


def unpack_weight_grad(dw, weight):
    """[Cout, T, Cs] -> gradient with the parameter's logical shape (channels_last strides)."""
    co, ci, kh, kw = weight.shape
    return dw[:, :, :ci].reshape(co, kh, kw, ci).permute(0, 3, 1, 2)


# How the 3x3 / stride-1 and 1x1 convolutions multiply (csrc/conv_split.h):
#   "bf16x6" (default): on the bf16 matrix cores with every fp32 operand cut into THREE bf16 pieces (all 24 significand
#            bits) and six piece products per product -- the reference's fp32 multiply / fp32 accumulate up to summation order;
#   "bf16x3": two pieces (16 significand bits per operand), three piece products: 2e-6 on the losses of a DA iteration, 2x
#            the rate of bf16x6;
#   "fp32":  everything on v_mfma_f32_32x32x2_f32 (bit-for-bit an fp32 fma chain), the slowest.
CONV_MODE = "bf16x6"
SPLIT_MODES = {"bf16x6": 3, "bf16x3": 2}


def split_pieces():
    """bf16 pieces per fp32 operand in the current CONV_MODE (0: the exact fp32-MFMA kernels)."""
    return SPLIT_MODES.get(CONV_MODE, 0)


def _round32(c):
    return (c + 31) // 32 * 32


def _round8(c):
    return (c + 7) // 8 * 8


# bf16 hi/lo planes of the parameters are valid for one optimizer step: engine.Trainer bumps SPLIT_EPOCH at the
# start of every iteration and the planes of flat-buffer parameters are reused by the source / target passes.
# SCAN_BATCHED=0 in the environment (or ops.BATCHED = False): the one-launch-per-tensor paths this build replaced --
# per-weight plane splits, per-group SGD launches, the torch construction of the discriminators' stacked weights, the
# separate GroupNorm statistics finalisation -- for same-box A/B measurements (profiles/r02_batched_ab.txt).  Same
# results either way.
BATCHED = os.environ.get("SCAN_BATCHED", "1") != "0"
# SCAN_CAT_IN_PLACE=0: the CKA discriminators build their class-branch input with torch.cat (+ the contiguous() copy of
# its gradient slice in the GroupNorm backward) instead of normalising into place, for A/B.  Same values.
CAT_IN_PLACE = os.environ.get("SCAN_CAT_IN_PLACE", "1") != "0"
# SCAN_FPN_DIRECT=0: the FPN output convs write tensors of their own that are concatenated afterwards, and the top-down
# join is an up-sampling copy + add (torch), for A/B.  Same values.
FPN_DIRECT = os.environ.get("SCAN_FPN_DIRECT", "1") != "0"
# Side streams other parts may borrow for short independent chains (the post-processor's per-image NMS): engine.Trainer
# registers the ones it made.  Borrowing instead of creating matters: one more HIP stream in the process shifts the stream ->
# hardware-queue assignment of all the others (profiles/r03_head_out_split.txt).
SIDE_STREAMS = []


def borrow_side_streams(n):
    while len(SIDE_STREAMS) < n:
        SIDE_STREAMS.append(torch.cuda.Stream())
    return SIDE_STREAMS[:n]


# Stream the weight-gradient launches of flat-buffer parameters are queued on (engine.Trainer sets it; None = the stream
# of the backward pass).  A weight gradient is a leaf of the backward graph -- nothing but the optimizer step (and the
# gradient all-reduce) reads it -- so on a stream of its own it fills what the dependent chain leaves idle: the graph
# tier's tiny launches, the tails of launches that are 1.4 waves of workgroups long.
WGRAD_STREAM = None
# SCAN_HEAD_OUT_SPLIT=0: the middle head's output conv runs as ONE conv over cat(features, act maps) as in the reference,
# instead of feature share + act-map share (modeling/condgraph.py: _out_features), for A/B.  Same sum, other rounding order.
HEAD_OUT_SPLIT = os.environ.get("SCAN_HEAD_OUT_SPLIT", "1") != "0"
SPLIT_EPOCH = None
_split_cache = {}
_epoch_counter = [0]
_active_plan = None


class SplitPlan:
    """The conv weights one owner (an engine.Trainer) needs as bf16 planes in every iteration.  The first iteration
    splits them one launch per weight as they are met and records (parameter, geometry, plane buffers) here; every later
    begin_weight_epoch(plan) re-splits ALL of them with ONE launch (scan_weight_split_batched) into the same buffers
    -- ~120 launches of 3-8 us on the critical path become one.  A job holds only a weak reference to its parameter:
    it is dropped when the parameter dies, and a weight that stops matching (another model at the same address) misses
    on the shape test in _conv_split and replaces its job."""

    def __init__(self):
        self.jobs = {}     # (data_ptr, mode, csw, pieces) -> (weakref to the parameter, O, T, cs_w, mode, rows, csw, planes)
        self.table = None  # device int64 [n_jobs, SPLIT_JOB_WORDS]
        self.order = []
        self.blocks = 0
        self.dirty = True

    def add(self, key, param, O, T, cs_w, mode, rows, csw, planes):
        self.jobs[key] = (weakref.ref(param), O, T, cs_w, mode, rows, csw, planes)
        self.dirty = True

    def run(self):
        # a job also dies when the arithmetic it was recorded for is no longer the current one (ops.CONV_MODE switched from
        # three pieces to two or back: k[3] is the piece count) -- otherwise every epoch would keep re-splitting, and
        # holding, the planes of BOTH modes
        npc = split_pieces()
        dead = [k for k, j in self.jobs.items() if j[0]() is None or j[0]().data_ptr() != k[0] or (npc > 0 and k[3] != npc)]
        for k in dead:
            _split_cache.pop(k, None)
            del self.jobs[k]
        if dead:
            self.dirty = True
        if not self.jobs:
            return
        if self.dirty:
            rows, off = [], 0
            self.order = list(self.jobs.keys())
            for k in self.order:
                _, O, T, cs_w, mode, r, csw, planes = self.jobs[k]
                rows.append([k[0], planes[0].data_ptr(), planes[1].data_ptr(), O, T, cs_w, mode, r, csw, off,
                             planes[2].data_ptr() if len(planes) == 3 else 0])
                off += query("scan_weight_split_job_blocks", O, T, cs_w, mode, csw)
            dev = self.jobs[self.order[0]][7][0].device
            self.table = torch.tensor(rows, dtype=torch.int64).to(dev)
            self.blocks = off
            self.dirty = False
        call("scan_weight_split_batched", _ptr(self.table), len(self.order), int(self.table.shape[1]), self.blocks, _stream())
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        for k in self.order:
            _split_cache[k] = (SPLIT_EPOCH, self.jobs[k][7], ev)


# GroupNorm workspaces (fp64 sums the kernels accumulate into with atomics) must start at zero.  Cleared one by one that is a
# memset launch per conv-with-sums and per GroupNorm backward, 60 per training step; instead they are slices of one buffer
# that begin_weight_epoch() clears with ONE memset (what the previous iteration used of it), and the library is told not to
# clear (scan_conv3x3_gn_acc_bf16x3; scan_groupnorm_run_backward's ws_cleared).  Outside an epoch, or when the buffer
# runs out, the workspace is a fresh allocation the library call clears itself.
ZERO_POOL = os.environ.get("SCAN_ZERO_POOL", "1") != "0"
_zero_pool = {"buf": None, "off": 0, "active": False}
_ZERO_POOL_DOUBLES = 1 << 20


def _ws_f64(n, device):
    """n doubles on `device` for a kernel that accumulates into them -> (tensor, True if it is already zero: a slice of
    the pool, valid until the next begin_weight_epoch; False: uninitialised, the library call clears it)."""
    zp = _zero_pool
    n_al = (n + 31) // 32 * 32
    if ZERO_POOL and zp["active"] and zp["buf"] is not None and zp["buf"].device == device \
            and zp["off"] + n_al <= _ZERO_POOL_DOUBLES:
        out = zp["buf"][zp["off"]:zp["off"] + n]
        zp["off"] += n_al
        return out, True
    return torch.empty((n,), dtype=torch.float64, device=device), False


_loss_zero = {"buf": None, "off": 0}


def _zeros_f32(n, device):
    """n zeroed floats for a loss kernel's accumulators.  Inside a training iteration they are carved from ONE torch.zeros
    allocated per iteration (a NEW tensor every iteration, so loss scalars that are views of it stay valid after the next
    iteration starts) -- ten fill launches per step become one."""
    lz = _loss_zero
    n_al = (n + 15) // 16 * 16
    if ZERO_POOL and _zero_pool["active"] and lz["buf"] is not None and lz["buf"].device == device \
            and lz["off"] + n_al <= lz["buf"].numel():
        out = lz["buf"][lz["off"]:lz["off"] + n]
        lz["off"] += n_al
        return out
    return torch.zeros((n,), dtype=torch.float32, device=device)


def _reset_zero_pool(device):
    _loss_zero["buf"] = torch.zeros((1024,), dtype=torch.float32, device=device) \
        if ZERO_POOL and device is not None and device.type == "cuda" else None
    _loss_zero["off"] = 0
    zp = _zero_pool
    if not ZERO_POOL or device is None or device.type != "cuda":
        zp["active"] = False
        return
    if zp["buf"] is None or zp["buf"].device != device:
        zp["buf"] = torch.zeros((_ZERO_POOL_DOUBLES,), dtype=torch.float64, device=device)
    elif zp["off"] > 0:
        zp["buf"][:zp["off"]].zero_()
    zp["off"] = 0
    zp["active"] = True


# True only inside engine.inference(): plain nn.Parameters (not re-homed into a Trainer's flat buffers) may then use the plane
# cache too.  Anywhere else a cached plane of a Parameter could outlive its model (another model's weight at the same address
# and shape would be served the old planes), so the switch is off and such weights are split per call.
CACHE_PLAIN_PARAMS = False


def begin_weight_epoch(plan=None, device=None):
    """Start of a span in which parameters do not change (one training iteration): the bf16 planes split inside it are
    reused by every launch that reads the same weight (forward, data gradient, source / target passes).  With a
    SplitPlan the planes it knows are produced right here, in one launch."""
    global SPLIT_EPOCH, _active_plan
    _epoch_counter[0] += 1
    SPLIT_EPOCH = _epoch_counter[0]
    _split_cache.clear()
    _active_plan = plan if BATCHED else None
    _reset_zero_pool(device)
    if _active_plan is not None:
        _active_plan.run()


def invalidate_weight_planes():
    """Parameters are about to change or have changed in place (optimizer step, state_dict / checkpoint load): drop
    every cached plane and stop caching until the next begin_weight_epoch().  In-place updates keep data_ptr, so a
    stale entry would otherwise be served to e.g. inference() after training."""
    global SPLIT_EPOCH, _active_plan
    SPLIT_EPOCH = None
    _active_plan = None
    _zero_pool["active"] = False
    _split_cache.clear()
    if _EXT_INVALIDATE is not None:  # the compiled operators' own plane cache (scan_ops_ext.cpp), when that module is loaded
        _EXT_INVALIDATE()


_EXT_INVALIDATE = None  # set by scan_amd.layers when scan_ops._ops is imported


# GroupNorm sums produced by a conv epilogue, handed to the groupnorm_relu call that consumes that conv's output
_gn_sums = {}


def _conv_split(x, shape, wp, cout, rows_out, cs_src, mode, bias, relu, ns, name, flops, cache_key=None,
                mask=None, dst_shape=None, cmap=0, pool=False, gn_sums=False, param=None, out=None, pieces=None):
    """Forward / data gradient of a 3x3 / stride-1 or 1x1 conv on the bf16 matrix cores with split operands (pieces = 3:
    "bf16x6", 2: "bf16x3"; default: the current CONV_MODE).  wp: packed fp32 weights [O][T][Cs_w], T = 9 or 1 (1x1; dst_shape = output pyramid, cmap =
    scan_conv1x1_*'s map).  mode 0: forward (Nout = O); mode 1: dgrad (Nout = Cs_w)."""
    st = _stream()
    npc = pieces or split_pieces()
    O, T, cs_w = wp.shape
    # planes, kernel family and launch cut come from the library (scan_conv_plan, include/scan_hip.h): the compiled operators
    # (csrc/scan_ops_ext.cpp) ask the same function
    plan = _lib.ConvPlan()
    call("scan_conv_plan", npc, T, mode, O, cs_w, cs_src, (dst_shape or shape).ref(),
         (_lib.CONV_SUMS if gn_sums else 0) | (_lib.CONV_POOL if pool else 0), ctypes.byref(plan))
    smode, csw, rows, TP, nout = plan.split_mode, plan.csw, plan.plane_rows, plan.plane_taps, plan.nout
    key = (cache_key, smode, csw, npc)
    hit = None
    if cache_key is not None and SPLIT_EPOCH is not None:
        hit = _split_cache.get(key)
        if hit is not None and (hit[0] != SPLIT_EPOCH or tuple(hit[1][0].shape) != (rows, TP, csw)):
            hit = None
    if hit is not None:
        planes = hit[1]
        # planes written on another stream (e.g. the target pass on its side stream) must be complete
        torch.cuda.current_stream().wait_event(hit[2])
    else:
        planes = tuple(torch.empty((rows, TP, csw), dtype=torch.bfloat16, device=x.device) for _ in range(npc))
        call("scan_conv_weight_split", ctypes.byref(plan), _ptr(wp), *[_ptr(t) for t in planes], *[None] * (3 - npc), st)
        if cache_key is not None and SPLIT_EPOCH is not None:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            _split_cache[key] = (SPLIT_EPOCH, planes, ev)
            if _active_plan is not None and param is not None and wp.data_ptr() == cache_key == param.data_ptr():
                _active_plan.add(key, param, O, T, cs_w, smode, rows, csw, planes)
    y = out if out is not None else (x.new_zeros if ns != nout else x.new_empty)((rows_out, ns))
    # the record carries the template instance the launch takes (64 / 128 / 256 channels; 3128: the Winograd instance, whose
    # roofline counts direct-conv FLOPs)
    ev = kernel_timer.begin("%s_bn%d" % (name, plan.instance), flops) if kernel_timer.enabled else None
    sums, cleared = (None, True)
    if gn_sums:
        sums, cleared = _ws_f64(shape.n_levels * shape.n_images * 32 * 2, x.device)
        _gn_sums.clear()  # at most one pending hand-over: conv and its GroupNorm are adjacent calls of one thread
        _gn_sums[y.data_ptr()] = sums
    call("scan_conv_run", ctypes.byref(plan), _ptr(x), shape.ref(), cs_src, *[_ptr(t) for t in planes], *[None] * (3 - npc),
         _ptr(bias), _ptr(mask), _ptr(y), (dst_shape or shape).ref(), ns, int(bool(relu)), cmap, _ptr(sums),
         0 if cleared else 1, st)
    kernel_timer.end(ev)
    return y


class _Conv2d(torch.autograd.Function):
    """conv (k in {1,3,5,7}, stride in {1,2}, pad k//2) + bias (+ ReLU) on a pyramid.

    relu = "deferred": the forward applies the ReLU, the backward does NOT mask dy -- the contract is that every
    consumer of y multiplies its dx by (y > 0) itself (mask_dx=True on a conv, relu_input=True on the max-pool),
    which those kernels do for free in their epilogue; it removes the separate relu-backward pass over dy."""

    @staticmethod
    def forward(ctx, x, weight, bias, shape, ksize, stride, relu, cout_s, mask_dx=False, pool=False, gn_sums=False,
                out=None):
        _chk(x, bias)
        if not weight.is_cuda:
            raise RuntimeError("scan_amd ops run only on the GPU (HIP); no CPU fallback")
        cs = x.shape[1]
        assert x.shape[0] == shape.rows, (x.shape, shape)
        cout = weight.shape[0]
        cout_s = cout_s or pad4(cout)
        wp = pack_weight(weight, cs)
        oshape = shape.conv_out(ksize, stride)
        if out is not None:  # write into a caller-provided row block (a slice of a pyramid buffer, see assemble_rows)
            if pool or not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
                            and tuple(out.shape) == (oshape.rows, cout_s) and cout_s == cout):
                raise RuntimeError("conv2d(out=...): needs a contiguous fp32 [%d, %d] GPU block with Cout == Cout_s"
                                   % (oshape.rows, cout_s))
        fast = split_pieces() > 0 and ((ksize == 3 and stride == 1) or ksize == 1)
        tag = CONV_MODE  # kernel_timer labels
        flops = 2.0 * oshape.rows * cout * ksize * ksize * weight.shape[1]
        # planes are cached per weight epoch for tensors whose storage outlives a call: flat-buffer parameters (a Trainer's)
        # and plain nn.Parameters (an inference-only model: engine.inference(static_weights=True) keeps the epoch open across
        # batches -- without this its 32 conv weights were re-split every batch).  A temporary (torch.cat of two heads'
        # weights, stacked discriminator weights) is never cached: the allocator hands its address to the next temporary
        ckey = weight.data_ptr() if (getattr(weight, "_scan_flat", False)
                                     or (CACHE_PLAIN_PARAMS and isinstance(weight, torch.nn.Parameter))) else None
        # first layer (3 input channels): dedicated K = taps x 4 forward kernel (the backward, if any, is generic)
        first = split_pieces() > 0 and cs == 4 and cout <= 64 and (ksize, stride) in ((3, 1), (7, 2)) \
            and shape.n_levels == 1
        if first:
            (h, w_), n = shape.sizes[0], shape.n_images
            y = out if out is not None else (x.new_zeros if cout_s != cout else x.new_empty)((oshape.rows, cout_s))
            ev = kernel_timer.begin("conv_smallcin_" + tag, flops)
            call("scan_conv_smallcin_" + tag, _ptr(x), n, h, w_, _ptr(wp), _ptr(bias), _ptr(y), cout, cout_s, ksize,
                 stride, int(bool(relu)), _stream())
            kernel_timer.end(ev)
        elif fast:
            if pool:  # conv + ReLU + 2x2 max-pool in one launch: forward only (frozen stages)
                if ksize != 3 or shape.n_levels != 1:
                    raise RuntimeError("conv2d(pool=True) needs a 3x3 conv on a single-level pyramid")
                (h, w_) = shape.sizes[0]
                y = _conv_split(x, shape, wp, cout, shape.n_images * (h // 2) * (w_ // 2), cs, 0, bias, relu, cout_s,
                                    "conv3x3_%s_fwd" % tag, flops, cache_key=ckey, pool=True, param=weight)
            else:
                y = _conv_split(x, shape, wp, cout, oshape.rows, cs, 0, bias, relu, cout_s,
                                    ("conv3x3_%s_fwd" if ksize == 3 else "conv1x1_%s_fwd") % tag, flops,
                                    cache_key=ckey, dst_shape=oshape, cmap=stride - 1, param=weight,
                                    # deterministic mode: the epilogue's sums are atomic -- groupnorm_relu then takes its
                                    # statistics from the ordered stats kernel (one more read of y)
                                    gn_sums=gn_sums and ksize == 3 and cout == 256 and cout_s == 256 and not relu
                                    and not deterministic(),
                                    out=out)
        else:
            y = out if out is not None else (x.new_zeros if cout_s != cout else x.new_empty)((oshape.rows, cout_s))
            ev = kernel_timer.begin("conv_igemm_fwd", flops)
            call("scan_conv2d_forward", _ptr(x), shape.ref(), cs, _ptr(wp), _ptr(bias), _ptr(y), oshape.ref(), cout,
                 cout_s, ksize, stride, int(bool(relu)), _stream())
            kernel_timer.end(ev)
        ctx.save_for_backward(x, weight, y if relu is True else None)
        ctx.cfg = (shape, oshape, ksize, stride, relu, cout_s, bias is not None, fast)
        ctx.conv_mode = CONV_MODE  # the backward runs on the kernels of the mode the forward ran in
        ctx.mask_dx = mask_dx
        ctx.ckey = ckey
        # parameters re-homed into a flat gradient buffer (engine.FlatGroup): accumulate straight into it
        ctx.wgrad_buf = ctx.bgrad_buf = None
        if getattr(weight, "_scan_flat", False) and weight.grad is not None and weight.shape[1] == cs \
                and weight.grad.permute(0, 2, 3, 1).is_contiguous():
            ctx.wgrad_buf = weight.grad
            if bias is not None and getattr(bias, "_scan_flat", False) and bias.grad is not None:
                ctx.bgrad_buf = bias.grad
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        shape, oshape, ksize, stride, relu, cout_s, has_bias, fast = ctx.cfg
        cs = x.shape[1]
        cout, cin = weight.shape[0], weight.shape[1]
        T = ksize * ksize
        st = _stream()
        sfx = ctx.conv_mode if ctx.conv_mode in SPLIT_MODES else "bf16x3"
        dy = dy.contiguous()
        if relu is True:
            g = torch.empty_like(dy)
            call("scan_relu_backward", _ptr(dy), _ptr(y), _ptr(g), dy.numel(), st)
            dy = g
        dx = dw = db = None
        mask = x if ctx.mask_dx else None  # x is a deferred-ReLU output: dx *= (x > 0) in the dgrad epilogue
        if ctx.needs_input_grad[0] and fast:
            dx = _conv_split(dy, oshape, pack_weight(weight, cs), cout, x.shape[0], cout_s, 1, None, False, cs,
                                 ("conv3x3_%s_dgrad" if ksize == 3 else "conv1x1_%s_dgrad") % sfx,
                                 2.0 * oshape.rows * cout * T * cin, cache_key=ctx.ckey, mask=mask, dst_shape=shape,
                                 cmap=0 if stride == 1 else 2, param=weight, pieces=SPLIT_MODES[sfx])
        elif ctx.needs_input_grad[0]:
            wp = pack_weight(weight, cs)
            wt = x.new_empty((cs, T, cout_s))
            call("scan_weight_transpose", _ptr(wp), cout, T, cs, _ptr(wt), cout_s, st)
            dx = torch.empty_like(x)
            ev = kernel_timer.begin("conv_igemm_dgrad", 2.0 * oshape.rows * cout * T * cin)
            call("scan_conv2d_dgrad", _ptr(dy), oshape.ref(), cout_s, _ptr(wt), _ptr(dx), shape.ref(), cs, cs, ksize,
                 stride, _ptr(mask), st)
            kernel_timer.end(ev)
        direct_w = ctx.wgrad_buf is not None
        direct_b = direct_w and ctx.bgrad_buf is not None
        want_db = has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1]:
            # family, kernel, split-K cut and workspace come from the library (scan_conv_wgrad_plan, include/scan_hip.h): the
            # compiled operators (csrc/scan_ops_ext.cpp) ask the same function
            plan = _lib.WgradPlan()
            call("scan_conv_wgrad_plan", SPLIT_MODES[sfx] if fast else 0, ksize, stride, cs, cout, shape.ref(), oshape.ref(),
                 ctypes.byref(plan))
            split3 = plan.family == _lib.WGRAD_SPLIT3X3
            label = "conv_wgrad" if plan.family == _lib.WGRAD_GENERIC else ("conv3x3_%s_wgrad" if split3 else "conv1x1_%s_wgrad") % sfx
            side = WGRAD_STREAM if (split3 and direct_w and (direct_b or not want_db) and not kernel_timer.enabled) else None
            if side is not None:  # in place into the flat gradient buffers, nothing returned to autograd: off the chain
                side.wait_stream(torch.cuda.current_stream())
                x.record_stream(side)
                dy.record_stream(side)
            with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
                # one launch sequence on the current stream: dw and db (the split kernels fuse dy's column sums, the generic one
                # is followed by them) straight into the flat gradient buffers or into fresh tensors for autograd
                ws = x.new_empty((plan.ws_floats,))
                dwp = ctx.wgrad_buf if direct_w else x.new_empty((cout, T, cs))
                if want_db:
                    db = ctx.bgrad_buf if direct_b else x.new_empty((cout,))
                ev = kernel_timer.begin(label, 2.0 * oshape.rows * cout * T * cin)
                try:
                    call("scan_conv_wgrad_run", ctypes.byref(plan), _ptr(x), shape.ref(), cs, _ptr(dy), oshape.ref(), cout, cout_s,
                         _ptr(dwp), _ptr(db), int(direct_w) | 2 * int(direct_b), _ptr(ws), _stream())
                except RuntimeError:
                    if plan.fused_db and want_db and direct_w and not direct_b:  # the library refuses differing accumulate bits
                        raise RuntimeError("conv2d: flat weight gradient without a flat bias gradient") from None
                    raise
                kernel_timer.end(ev)
            dw = None if direct_w else unpack_weight_grad(dwp, weight)
        elif want_db:  # a bias gradient alone (frozen weight): dy's column sums, no weight-gradient launch
            M = dy.shape[0]
            ws = x.new_empty((query("scan_colsum_ws_floats", M, cout),))
            db = ctx.bgrad_buf if direct_b else x.new_empty((cout,))
            call("scan_colsum", _ptr(dy), M, cout, cout_s, _ptr(db), int(direct_b), _ptr(ws), st)
        if direct_b:
            db = None
        return dx, dw, db, None, None, None, None, None, None, None, None, None


def conv2d(x, weight, bias, shape, ksize=3, stride=1, relu=False, cout_s=None, mask_dx=False, pool=False,
           gn_sums=False, out=None):
    """Returns rows [M_out, Cout_s]; the output PyramidShape is shape.conv_out(ksize, stride).
    relu: False | True | "deferred" (see _Conv2d); mask_dx: x is a deferred-ReLU output; pool: fuse the following
    2x2 / stride-2 max-pool (forward-only, bf16x3 mode: frozen VGG stages) -- the rows returned are the pooled ones;
    gn_sums: the output feeds groupnorm_relu -- let the conv epilogue accumulate the GroupNorm sums (bf16x3 mode,
    256 channels; otherwise ignored and groupnorm_relu computes its own statistics)."""
    assert relu in (False, True, "deferred")
    if pool and torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad
                                             or (bias is not None and bias.requires_grad)):
        raise RuntimeError("conv2d(pool=True) is forward-only (frozen 3x3 conv on a single-level pyramid)")
    return _Conv2d.apply(x, weight, bias, shape, ksize, stride, relu, cout_s, mask_dx, pool, gn_sums, out)


def conv_pool_fusable(x, weight, bias, shape):
    """True when conv2d(pool=True) applies: bf16x3 mode, a 3x3 conv on a single-level pyramid with even sizes that is
    not the 3-channel first layer, and nothing on it needs a gradient."""
    (h, w_) = shape.sizes[0]
    needs = torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad
                                         or (bias is not None and bias.requires_grad))
    return (split_pieces() > 0 and shape.n_levels == 1 and h % 2 == 0 and w_ % 2 == 0 and x.shape[1] != 4
            and tuple(weight.shape[2:]) == (3, 3) and not needs)


# ----------------------------------------------------------------------------- pyramid row split
# ----------------------------------------------------------------------------- deformable convolution (DCNv2)
def _row_pitch(t, cols, name, who="deform_conv2d"):
    """offset / mask operands: fp32 GPU matrices with at least `cols` columns whose rows are contiguous; a column slice of a
    wider matrix is taken as it is (its pitch is passed on)"""
    if not t.is_cuda:
        raise RuntimeError("scan_amd ops run only on the GPU (HIP) -- got a %s tensor; no CPU fallback" % t.device)
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] < cols or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        raise RuntimeError("%s: %s must be an fp32 [M, >= %d] matrix with contiguous rows" % (who, name, cols))
    return t.stride(0)


class _DeformSample(torch.autograd.Function):
    """rows [M, Cs], offset [M, >= 18], mask [M, >= 9] or None -> cols [M, 9 * Cs] (csrc/deform.hip).  The backward has no
    float atomics: the sampling gradient writes (destination row, weight) per (row, tap, corner), a stable sort of the
    destinations and a per-row sum in sorted order give dx -- bit-reproducible with ``deterministic`` on or off."""

    @staticmethod
    def forward(ctx, x, offset, mask, shape, c):
        _chk(x)
        ld_off = _row_pitch(offset, 18, "offset")
        ld_mask = _row_pitch(mask, 9, "mask") if mask is not None else 0
        M, cs = x.shape
        if M != shape.rows or offset.shape[0] != M or (mask is not None and mask.shape[0] != M):
            raise RuntimeError("deform_conv2d: rows %d, offset %d, mask %s do not match %r"
                               % (M, offset.shape[0], None if mask is None else mask.shape[0], shape))
        cols = x.new_empty((M, 9 * cs))
        call("scan_deform_sample_forward", _ptr(x), shape.ref(), c, cs, _ptr(offset), ld_off, _ptr(mask), ld_mask, _ptr(cols),
             _stream())
        ctx.save_for_backward(x, offset, mask)
        ctx.cfg = (shape, c)
        return cols

    @staticmethod
    def backward(ctx, dcols):
        x, offset, mask = ctx.saved_tensors
        shape, c = ctx.cfg
        M, cs = x.shape
        st = _stream()
        dcols = dcols.contiguous()
        doff = torch.empty(offset.shape, dtype=torch.float32, device=x.device)
        dmask = torch.empty(mask.shape, dtype=torch.float32, device=x.device) if mask is not None else None
        keys = torch.empty((36 * M,), dtype=torch.int32, device=x.device)
        wgts = torch.empty((36 * M,), dtype=torch.float32, device=x.device)
        call("scan_deform_sample_backward", _ptr(x), shape.ref(), c, cs, _ptr(dcols), _ptr(offset), offset.stride(0), _ptr(mask),
             mask.stride(0) if mask is not None else 0, _ptr(doff), doff.shape[1], _ptr(dmask),
             dmask.shape[1] if dmask is not None else 0, _ptr(keys), _ptr(wgts), st)
        dx = None
        if ctx.needs_input_grad[0]:
            # the inverted index: entries grouped by destination row, original order kept inside a group (key M = no destination)
            skeys, perm = torch.sort(keys, stable=True)
            seg = torch.searchsorted(skeys, torch.arange(M + 1, dtype=torch.int32, device=x.device))
            dx = torch.empty_like(x)
            call("scan_deform_dx_gather", _ptr(dcols), _ptr(perm), _ptr(seg), _ptr(wgts), M, c, cs, _ptr(dx), st)
        return dx, doff if ctx.needs_input_grad[1] else None, dmask if mask is not None and ctx.needs_input_grad[2] else None, \
            None, None


def deform_conv2d(rows, offset, mask, weight, bias, shape, relu=False, cout_s=None, gn_sums=False):
    """Modulated deformable 3x3 convolution (DCNv2; mask=None: DCNv1) on a pyramid: stride 1, padding 1, dilation 1, one
    group, one deformable group, input and output on the same pyramid, all levels in one launch.  Returns rows [M, Cout_s].

    rows [M, Cs]; offset [M, >= 18], column 2k = dy and 2k + 1 = dx of tap k = 3 i + j (the mmcv / torchvision order); mask
    [M, >= 9] or None -- both may be column slices of one wider matrix; weight [O, C, 3, 3] (channels_last, as for conv2d).
    The definition is include/scan_hip.h's (scan_deform_sample_forward).

    Two steps: the nine taps are sampled into cols [M, 9 * Cs] (csrc/deform.hip), then y is conv2d's 1x1 convolution over cols
    with the weight read as [O, 9 * Cs] -- so the op runs in the current CONV_MODE with that mode's error contract, and its
    weight and bias gradients are the 1x1 ones.  The weight planes are split by that conv2d call under conv2d's own rules (a
    view of the parameter is a temporary there: split per call, never cached, so there is nothing of this op's to invalidate).
    gn_sums is accepted for symmetry with conv2d: the 1x1 kernels have no GroupNorm-sums epilogue, so groupnorm_relu takes its
    own statistics pass.

    Memory: cols is kept for the backward and its gradient dcols has the same size, M * 9 * Cs floats each -- about 1.6 GB
    each on the bench pyramid (N = 4, 1024 x 2048, C = 256).  That fits this board and is not chunked."""
    if not (rows.is_cuda and weight.is_cuda):
        raise RuntimeError("scan_amd ops run only on the GPU (HIP); no CPU fallback")
    o, c, kh, kw = weight.shape
    cs = rows.shape[1]
    if (kh, kw) != (3, 3) or c > cs:
        raise RuntimeError("deform_conv2d: needs a [O, C, 3, 3] weight with C <= Cs (got %s, Cs=%d)" % (tuple(weight.shape), cs))
    if gn_sums:
        _gn_sums.clear()  # this output carries no sums: a pending hand-over must not be matched to its address
    cols = _DeformSample.apply(rows, offset, mask, shape, c)
    w1 = pack_weight(weight, cs).reshape(o, 9 * cs, 1, 1)  # [O][tap][Cs]: the column order of cols
    return conv2d(cols, w1, bias, shape, 1, 1, relu=relu, cout_s=cout_s, gn_sums=gn_sums)


class _SplitLevels(torch.autograd.Function):
    """rows [M, C] -> one view per level.  The backward concatenates the level gradients once instead of
    autograd's per-slice zero-fill + add of full-size tensors."""

    @staticmethod
    def forward(ctx, rows, shape):
        ctx.shape = shape
        ctx.cols = rows.shape[1]
        return tuple(rows[shape.row_off[l]:shape.row_off[l + 1]] for l in range(shape.n_levels))

    @staticmethod
    def backward(ctx, *grads):
        shape = ctx.shape
        ref = next(g for g in grads if g is not None)
        parts = [g if g is not None else ref.new_zeros((shape.row_off[l + 1] - shape.row_off[l], ctx.cols))
                 for l, g in enumerate(grads)]
        return torch.cat(parts, 0), None


def split_levels(rows, shape):
    return _SplitLevels.apply(rows, shape)


class _SplitLevelsGRL(torch.autograd.Function):
    """rows [M, C] -> one view per level, each behind a gradient-reversal layer of its own strength (reference
    discriminator/layer.py:6-33: forward identity, backward -lambda_l * g).  The backward scales every level's gradient
    STRAIGHT INTO its row range of one [M, C] matrix: no per-level scaled copy followed by a concatenation."""

    @staticmethod
    def forward(ctx, rows, shape, lams):
        _chk(rows)
        ctx.cfg = (shape, tuple(float(v) for v in lams), rows.shape[1])
        return tuple(rows[shape.row_off[l]:shape.row_off[l + 1]] for l in range(shape.n_levels))

    @staticmethod
    def backward(ctx, *grads):
        shape, lams, cols = ctx.cfg
        ref = next(g for g in grads if g is not None)
        out = ref.new_empty((shape.rows, cols))
        st = _stream()
        for l, g in enumerate(grads):
            part = out[shape.row_off[l]:shape.row_off[l + 1]]
            if g is None:
                part.zero_()
            else:
                g = g.contiguous()
                call("scan_scale", _ptr(g), -lams[l], _ptr(part), g.numel(), st)
        return out, None, None


def split_levels_grl(rows, shape, lams):
    """split_levels with grad_reverse(., lams[l]) applied to level l (the discriminators' own GRL is then skipped)."""
    return _SplitLevelsGRL.apply(rows, shape, lams)


# ----------------------------------------------------------------------------- centre-aware alignment (EPM baseline)
def center_aware_map(cls_rows, ctr, C, weight):
    """atten [M] = sigmoid(weight * max_c sigmoid(cls_rows[m, c]) * sigmoid(ctr[m])) (reference discriminator/
    fcos_head_discriminator_CA.py:61-69) for the whole pyramid in one launch.  cls_rows: the head's class-logit rows, [M, >= C]
    with unit column stride -- the column slice the head returns is taken as it is, its row pitch is the conv's padded width and
    only the first C columns are read; ctr: [M] with any stride (a column of the head's bbox / centerness conv).  No gradient:
    the reference detaches the score maps (engine/trainer.py:320-322)."""
    cls_rows, ctr = cls_rows.detach(), ctr.detach()
    if not (cls_rows.is_cuda and ctr.is_cuda):
        raise RuntimeError("scan_amd ops run only on the GPU (HIP) -- got %s / %s tensors; no CPU fallback" % (cls_rows.device, ctr.device))
    if cls_rows.dtype != torch.float32 or ctr.dtype != torch.float32 or cls_rows.dim() != 2:
        raise RuntimeError("center_aware_map: fp32 [M, Cs] class rows and fp32 [M] centerness")
    M = cls_rows.shape[0]
    if ctr.dim() == 2 and ctr.shape[1] == 1:
        ctr = ctr[:, 0]
    if not 1 <= C <= cls_rows.shape[1] or ctr.dim() != 1 or ctr.shape[0] != M:
        raise RuntimeError("center_aware_map: C=%d of %d columns, %s centerness for %d rows" % (C, cls_rows.shape[1], tuple(ctr.shape), M))
    if M > 1 and (cls_rows.stride(1) != 1 or cls_rows.stride(0) < cls_rows.shape[1]):
        cls_rows = cls_rows.contiguous()
    cs = cls_rows.stride(0) if M > 1 else max(cls_rows.shape[1], 1)
    atten = torch.empty((M,), dtype=torch.float32, device=cls_rows.device)
    call("scan_center_aware_map", _ptr(cls_rows), cs, C, _ptr(ctr), max(ctr.stride(0), 1), float(weight), M, _ptr(atten), _stream())
    return atten


def _row_scale_levels(x_levels, ldx, atten, scales, shape, C, out):
    """out[m, :C] = (scales[l(m)] * atten[m]) * x[m, :C]; x_levels: one matrix, or one tensor (or None: zeros) per level"""
    s = (ctypes.c_float * shape.n_levels)(*scales)
    if isinstance(x_levels, torch.Tensor):
        call("scan_row_scale_levels", _ptr(x_levels), ldx, _ptr(atten), s, shape.ref(), C, _ptr(out), out.stride(0), _stream())
    else:
        ptrs = (ctypes.c_void_p * shape.n_levels)(*[t.data_ptr() if t is not None else None for t in x_levels])
        call("scan_row_scale_levels_ptrs", ptrs, ldx, _ptr(atten), s, shape.ref(), C, _ptr(out), out.stride(0), _stream())
    return out


class _CenterAwareSplitLevelsGRL(torch.autograd.Function):
    """rows [M, C] -> the five level views of atten[:, None] * rows, each behind a gradient-reversal layer of its own strength
    (reference fcos_head_discriminator_CA.py:93: grad_reverse(atten_map * feature)).  One launch forward; the backward scales the
    five level gradients by -lambda_l * atten[m] straight into their row ranges of one [M, C] matrix, in one launch too.
    atten = None: split_levels_grl's values (the 'ca_loss' form keeps the feature as it is) with that one-launch backward."""

    @staticmethod
    def forward(ctx, rows, atten, shape, lams):
        _chk(rows, atten)
        M, C = rows.shape
        if M != shape.rows or C % 4 or (atten is not None and atten.shape != (M,)):
            raise RuntimeError("center_aware_split_levels_grl: rows %s, atten %s for %d pyramid rows (columns: a multiple of 4)"
                               % (tuple(rows.shape), None if atten is None else tuple(atten.shape), shape.rows))
        if len(lams) != shape.n_levels:
            raise RuntimeError("center_aware_split_levels_grl: %d strengths for %d levels" % (len(lams), shape.n_levels))
        ctx.cfg = (shape, tuple(float(v) for v in lams), C)
        ctx.save_for_backward(atten)
        y = rows if atten is None else _row_scale_levels(rows, C, atten, [1.0] * shape.n_levels, shape, C, torch.empty_like(rows))
        return tuple(y[shape.row_off[l]:shape.row_off[l + 1]] for l in range(shape.n_levels))

    @staticmethod
    def backward(ctx, *grads):
        shape, lams, C = ctx.cfg
        atten, = ctx.saved_tensors
        ref = next(g for g in grads if g is not None)
        grads = [g if g is None or g.is_contiguous() else g.contiguous() for g in grads]
        out = ref.new_empty((shape.rows, C))
        _row_scale_levels(grads, C, atten, [-v for v in lams], shape, C, out)
        return out, None, None, None


def center_aware_split_levels_grl(feats, atten, shape, lams):
    """the level views of atten[:, None] * feats behind grad_reverse(., lams[l]); atten from center_aware_map (detached)"""
    return _CenterAwareSplitLevelsGRL.apply(feats, atten, shape, lams)


class _TakeImages(torch.autograd.Function):
    """rows of images [i0, i1) of every level, as the pyramid of those images (level-major order is kept)."""

    @staticmethod
    def forward(ctx, rows, shape, i0, i1):
        ctx.cfg = (shape, i0, i1, rows.shape)
        parts = []
        for l, (h, w) in enumerate(shape.sizes):
            r0 = shape.row_off[l]
            parts.append(rows[r0 + i0 * h * w:r0 + i1 * h * w])
        return torch.cat(parts, 0)

    @staticmethod
    def backward(ctx, g):
        shape, i0, i1, full = ctx.cfg
        if g.is_cuda and g.dtype == torch.float32 and len(full) == 2:
            out = g.new_empty(full)  # one pass: the taken images' rows copied, the others zeroed
            call("scan_take_images_backward", _ptr(g.contiguous()), shape.ref(), i0, i1, full[1], _ptr(out), _stream())
            return out, None, None, None
        out = g.new_zeros(full)
        o = 0
        for l, (h, w) in enumerate(shape.sizes):
            r0, n = shape.row_off[l], (i1 - i0) * h * w
            out[r0 + i0 * h * w:r0 + i0 * h * w + n] = g[o:o + n]
            o += n
        return out, None, None, None


def take_images(rows, shape, i0, i1):
    """sub-batch [i0, i1) of a pyramid -> (rows, PyramidShape of i1 - i0 images)."""
    return _TakeImages.apply(rows, shape, i0, i1), PyramidShape(i1 - i0, shape.sizes)


# ----------------------------------------------------------------------------- per-level NCHW lists <-> pyramid rows
def _level_descs(levels):
    """the scan_level_t array of a list of [N, C, h, w] tensors (element strides as torch reports them)"""
    arr = (_lib.LevelDesc * len(levels))()
    for d, t in zip(arr, levels):
        d.data, d.h, d.w = t.data_ptr(), t.shape[2], t.shape[3]
        d.sn, d.sc, d.sy, d.sx = t.stride()
    return arr


def _chk_levels(levels):
    if not levels:
        raise ValueError("pack_levels: empty level list")
    if len(levels) > _lib.MAX_LEVELS:
        raise ValueError("pack_levels: %d levels, a PyramidShape holds at most %d" % (len(levels), _lib.MAX_LEVELS))
    n, c = levels[0].shape[0], levels[0].shape[1]
    for t in levels:
        if not t.is_cuda:
            raise RuntimeError("scan_amd ops run only on the GPU (HIP) -- got a %s tensor; no CPU fallback" % t.device)
        if t.dtype != torch.float32 or t.dim() != 4 or t.shape[0] != n or t.shape[1] != c:
            raise ValueError("pack_levels: every level must be a fp32 [N, C, h, w] tensor with the same N and C")
    return n, c


def _level_format(t):
    """memory format a gradient / copy of level t is allocated in: channels_last when its channels are the fastest dimension"""
    return torch.channels_last if t.stride(1) == 1 and t.shape[1] > 1 else torch.contiguous_format


def _unpack_into(rows, shape, c, formats):
    out = [torch.empty((shape.n_images, c, h, w), dtype=rows.dtype, device=rows.device, memory_format=f)
           for (h, w), f in zip(shape.sizes, formats)]
    call("scan_pyramid_unpack", _ptr(rows), rows.shape[1], _level_descs(out), len(out), shape.n_images, c, _stream())
    return out


class _PackLevels(torch.autograd.Function):
    """per-level [N, C, h, w] tensors of any strides -> rows [M, Cs] in one launch (csrc/pyramid_pack.hip); the backward is the
    unpack kernel on the row gradient."""

    @staticmethod
    def forward(ctx, shape, cs, *levels):
        c = levels[0].shape[1]
        rows = levels[0].new_empty((shape.rows, cs))  # every element, padding columns included, is written by the kernel
        call("scan_pyramid_pack", _level_descs(levels), len(levels), shape.n_images, c, _ptr(rows), cs, _stream())
        ctx.cfg = (shape, c, [_level_format(t) for t in levels])
        return rows

    @staticmethod
    def backward(ctx, g):
        shape, c, formats = ctx.cfg
        grads = _unpack_into(g.contiguous(), shape, c, formats)
        return (None, None) + tuple(gl if need else None for gl, need in zip(grads, ctx.needs_input_grad[2:]))


class _UnpackLevels(torch.autograd.Function):
    """rows [M, Cs] -> one fresh [N, c, h, w] tensor per level in one launch; the backward is the pack kernel on the level
    gradients, whatever their strides (an absent one counts as zeros)."""

    @staticmethod
    def forward(ctx, rows, shape, c, memory_format):
        ctx.cfg = (shape, c, rows.shape[1])
        return tuple(_unpack_into(rows, shape, c, [memory_format] * shape.n_levels))

    @staticmethod
    def backward(ctx, *grads):
        shape, c, cs = ctx.cfg
        ref = next(g for g in grads if g is not None)
        grads = [g if g is not None else ref.new_zeros((shape.n_images, c, h, w)) for g, (h, w) in zip(grads, shape.sizes)]
        out = ref.new_empty((shape.rows, cs))
        call("scan_pyramid_pack", _level_descs(grads), len(grads), shape.n_images, c, _ptr(out), cs, _stream())
        return out, None, None, None


class PyramidLevels(list):
    """The per-level channels_last [N, C, h, w] views of ONE pyramid row matrix, as the reference-shaped modules
    (scan_amd/modeling/factory.py) return them -- a plain list to a caller that indexes or iterates it -- together with the
    ``rows`` [M, Cs] matrix and the ``shape`` they are views of.  pack_levels hands ``rows`` back without a copy as long as
    every element still is the view it was made as."""

    def __init__(self, rows, shape, c=None):
        if rows.dim() != 2 or rows.shape[0] != shape.rows:
            raise ValueError("PyramidLevels: rows %s do not fit %r" % (tuple(rows.shape), shape))
        self.rows, self.shape = rows, shape
        self.c = rows.shape[1] if c is None else int(c)
        parts = split_levels(rows, shape) if rows.requires_grad and torch.is_grad_enabled() else \
            [rows[shape.row_off[l]:shape.row_off[l + 1]] for l in range(shape.n_levels)]
        super().__init__((p if self.c == p.shape[1] else p[:, :self.c]).view(shape.n_images, h, w, self.c).permute(0, 3, 1, 2)
                         for p, (h, w) in zip(parts, shape.sizes))
        self._made = [(t.data_ptr(), tuple(t.shape), t.stride()) for t in self]

    def intact(self):
        """every element still has the data_ptr, shape and strides of its slice of ``rows`` (nobody replaced or reordered one)"""
        return len(self) == len(self._made) and all(
            isinstance(t, torch.Tensor) and (t.data_ptr(), tuple(t.shape), t.stride()) == m for t, m in zip(self, self._made))


def pack_levels(levels, cs=None):
    """list of per-level [N, C, h, w] fp32 tensors (any strides) -> (rows [M, Cs], PyramidShape); Cs defaults to pad4(C).
    A PyramidLevels whose elements are untouched gives its own ``rows`` back (no launch, same storage), unless another
    ``cs`` than its row pitch is asked for."""
    if isinstance(levels, PyramidLevels) and (cs is None or cs == levels.rows.shape[1]) and levels.rows.is_contiguous() \
            and levels.c == levels.rows.shape[1] and levels.intact():
        _chk(levels.rows)
        return levels.rows, levels.shape
    levels = list(levels)
    n, c = _chk_levels(levels)
    cs = pad4(c) if cs is None else int(cs)
    if cs < c or cs % 4:
        raise ValueError("pack_levels: cs=%d must be a multiple of 4 and >= C=%d" % (cs, c))
    shape = PyramidShape(n, [tuple(t.shape[2:]) for t in levels])
    return _PackLevels.apply(shape, cs, *levels), shape


def unpack_levels(rows, shape, c=None, memory_format=torch.channels_last):
    """rows [M, Cs] -> list of fresh per-level [N, c, h, w] tensors in ``memory_format`` (columns c..Cs-1 are dropped)."""
    _chk(rows)
    c = rows.shape[1] if c is None else int(c)
    if rows.dim() != 2 or rows.shape[0] != shape.rows or not 1 <= c <= rows.shape[1] or rows.shape[1] % 4:
        raise ValueError("unpack_levels: rows %s do not fit %r with c=%d (the row pitch must be a multiple of 4)"
                         % (tuple(rows.shape), shape, c))
    return list(_UnpackLevels.apply(rows, shape, c, memory_format))


# ----------------------------------------------------------------------------- region pooling (ROIAlign / ROIPool)
def _roi_args(who, rows, shape, rois, output_size, scales, levels, c):
    """the checks every pooling op shares; returns (rois, levels, (PH, PW), host scale array, C)"""
    _chk(rows, rois, levels)
    if rows.dtype != torch.float32 or rows.dim() != 2 or rows.shape[0] != shape.rows or rows.shape[1] % 4:
        raise RuntimeError("%s: rows %s (%s) do not fit %r as an fp32 [M, Cs] matrix with Cs %% 4 == 0"
                           % (who, tuple(rows.shape), rows.dtype, shape))
    if rois.dtype != torch.float32 or rois.dim() != 2 or rois.shape[1] != 5:
        raise RuntimeError("%s: rois must be an fp32 [K, 5] matrix (image index, x1, y1, x2, y2), got %s %s"
                           % (who, tuple(rois.shape), rois.dtype))
    ph, pw = (output_size, output_size) if isinstance(output_size, int) else (int(output_size[0]), int(output_size[1]))
    if ph < 1 or pw < 1:
        raise RuntimeError("%s: output_size %r must be >= 1 x 1" % (who, output_size))
    scales = [float(s) for s in ((scales,) if isinstance(scales, (int, float)) else scales)]
    if len(scales) != shape.n_levels:
        raise RuntimeError("%s: %d scales for the %d levels of %r" % (who, len(scales), shape.n_levels, shape))
    c = rows.shape[1] if c is None else int(c)
    if not 1 <= c <= rows.shape[1]:
        raise RuntimeError("%s: c=%d must be in [1, Cs=%d]" % (who, c, rows.shape[1]))
    rois = rois.contiguous()
    if levels is None and len(scales) > 1:
        levels = roi_levels(rois, -torch.log2(torch.tensor(scales[0], dtype=torch.float32)).item(),
                            -torch.log2(torch.tensor(scales[-1], dtype=torch.float32)).item())  # modeling/poolers.py:74-76
    if levels is not None:
        if levels.dtype != torch.int32 or levels.dim() != 1 or levels.shape[0] != rois.shape[0]:
            raise RuntimeError("%s: levels must be int32 [K=%d], got %s %s" % (who, rois.shape[0], tuple(levels.shape), levels.dtype))
        levels = levels.contiguous()
    return rois, levels, (ph, pw), (ctypes.c_float * len(scales))(*scales), c


def roi_levels(rois, k_min, k_max, canonical_scale=224, canonical_level=4, eps=1e-6):
    """The reference's LevelMapper (modeling/poolers.py:11-42) on the device: rois [K, 5] (or boxes [K, 4], xyxy) -> int32 [K]
    = clamp(floor(canonical_level + log2(sqrt(area) / canonical_scale + eps)), k_min, k_max) - k_min in fp32, with
    area = (x2 - x1 + 1)(y2 - y1 + 1).  No host read."""
    _chk(rois)
    if rois.dtype != torch.float32 or rois.dim() != 2 or rois.shape[1] not in (4, 5):
        raise RuntimeError("roi_levels: needs an fp32 [K, 5] ROI or [K, 4] box matrix, got %s %s" % (tuple(rois.shape), rois.dtype))
    rois = rois.contiguous()
    K, ld = rois.shape
    levels = torch.empty((K,), dtype=torch.int32, device=rois.device)
    call("scan_roi_levels", ctypes.c_void_p(rois.data_ptr() + 4 * (ld - 4)), ld, K, float(k_min), float(k_max),
         float(canonical_scale), float(canonical_level), float(eps), _ptr(levels), _stream())
    return levels


class _RoiAlign(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, shape, rois, levels, sizes, scales, sr, c):
        K, cs = rois.shape[0], x.shape[1]
        y = x.new_empty((K, sizes[0], sizes[1], cs))
        call("scan_roi_align_forward", _ptr(x), shape.ref(), c, cs, _ptr(rois), _ptr(levels), scales, K, sizes[0], sizes[1], sr,
             _ptr(y), _stream())
        ctx.save_for_backward(rois, levels)
        ctx.cfg = (shape, sizes, scales, sr, c, cs)
        return y

    @staticmethod
    def backward(ctx, dy):
        rois, levels = ctx.saved_tensors
        shape, sizes, scales, sr, c, cs = ctx.cfg
        dy = dy.contiguous()
        dx = torch.empty((shape.rows, cs), dtype=torch.float32, device=dy.device)
        call("scan_roi_align_backward", _ptr(dy), shape.ref(), c, cs, _ptr(rois), _ptr(levels), scales, rois.shape[0], sizes[0],
             sizes[1], sr, _ptr(dx), _stream())
        return dx, None, None, None, None, None, None, None


def roi_align(rows, shape, rois, output_size, scales, sampling_ratio, levels=None, c=None):
    """ROIAlign (reference csrc/cuda/ROIAlign_cuda.cu, aligned=False semantics; include/scan_hip.h has the definition) of pyramid
    rows [M, Cs] for rois [K, 5] = (image, x1, y1, x2, y2): returns [K, PH, PW, Cs] channel-last, columns c..Cs-1 zeros.  One
    launch for all levels: ``scales`` has one spatial scale per level, ``levels`` int32 [K] names each ROI's level (None: level
    0 for a single scale, otherwise roi_levels, the reference's LevelMapper).  A ROI whose image or level is out of range gives
    zeros and no gradient.  sampling_ratio <= 0: the adaptive grid ceil(roi / pooled) per ROI and axis.

    Autograd to ``rows`` only.  The gradient is summed per destination row in a fixed order without float atomics
    (csrc/roi.hip): bit-identical from run to run whether ``deterministic`` is on or off, for every sampling_ratio, and with
    NO host read (0 device-to-host copies, the adaptive grid included)."""
    rois, levels, sizes, sc, c = _roi_args("roi_align", rows, shape, rois, output_size, scales, levels, c)
    return _RoiAlign.apply(rows, shape, rois, levels, sizes, sc, int(sampling_ratio), c)


def roi_align_samples(shape, rois, output_size, scales, sampling_ratio, gmax, levels=None):
    """what roi_align's kernels form per sample, for tests: (grid int32 [K, 2], pos [K, PH, PW, gmax, gmax, 2],
    weights [..., 4], cells int32 [..., 4]) -- see scan_roi_align_samples"""
    dummy = torch.empty((shape.rows, 4), dtype=torch.float32, device=rois.device)
    rois, levels, (ph, pw), sc, _ = _roi_args("roi_align_samples", dummy, shape, rois, output_size, scales, levels, None)
    K, dev = rois.shape[0], rois.device
    grid = torch.zeros((K, 2), dtype=torch.int32, device=dev)
    pos = torch.zeros((K, ph, pw, gmax, gmax, 2), dtype=torch.float32, device=dev)
    wgt = torch.zeros((K, ph, pw, gmax, gmax, 4), dtype=torch.float32, device=dev)
    cell = torch.zeros((K, ph, pw, gmax, gmax, 4), dtype=torch.int32, device=dev)
    call("scan_roi_align_samples", shape.ref(), _ptr(rois), _ptr(levels), sc, K, ph, pw, int(sampling_ratio), int(gmax), _ptr(grid),
         _ptr(pos), _ptr(wgt), _ptr(cell), _stream())
    return grid, pos, wgt, cell


class _RoiPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, shape, rois, levels, sizes, scales, c):
        K, cs = rois.shape[0], x.shape[1]
        y = x.new_empty((K, sizes[0], sizes[1], cs))
        argmax = torch.empty((K, sizes[0], sizes[1], cs), dtype=torch.int32, device=x.device)
        call("scan_roi_pool_forward", _ptr(x), shape.ref(), c, cs, _ptr(rois), _ptr(levels), scales, K, sizes[0], sizes[1],
             _ptr(y), _ptr(argmax), _stream())
        ctx.save_for_backward(rois, levels, argmax)
        ctx.cfg = (shape, sizes, scales, c, cs)
        ctx.mark_non_differentiable(argmax)
        return y, argmax

    @staticmethod
    def backward(ctx, dy, _dargmax):
        rois, levels, argmax = ctx.saved_tensors
        shape, sizes, scales, c, cs = ctx.cfg
        dx = roi_pool_backward(dy.contiguous(), argmax, shape, rois, sizes, scales, levels, c)
        return dx, None, None, None, None, None, None


def roi_pool_backward(dy, argmax, shape, rois, sizes, scales, levels, c):
    """dx [M, Cs] of roi_pool for dy, argmax [K, PH, PW, Cs] (scan_roi_pool_backward): per destination, no atomics"""
    cs = dy.shape[-1]
    dx = torch.empty((shape.rows, cs), dtype=torch.float32, device=dy.device)
    call("scan_roi_pool_backward", _ptr(dy), _ptr(argmax), shape.ref(), c, cs, _ptr(rois), _ptr(levels), scales, rois.shape[0],
         sizes[0], sizes[1], _ptr(dx), _stream())
    return dx


def roi_pool(rows, shape, rois, output_size, scales, levels=None, c=None, return_argmax=False):
    """ROIPool (reference csrc/cuda/ROIPool_cuda.cu; include/scan_hip.h has the definition) of pyramid rows [M, Cs]: returns
    [K, PH, PW, Cs] channel-last (and, with return_argmax, the int32 argmax h * W + w of the ROI's level per channel, -1 for an
    empty bin).  ``scales`` / ``levels`` as for roi_align.  Autograd to ``rows`` only; the gradient is summed per destination
    in ascending (ROI, ph, pw) order without float atomics: bit-identical from run to run, no host read."""
    rois, levels, sizes, sc, c = _roi_args("roi_pool", rows, shape, rois, output_size, scales, levels, c)
    y, argmax = _RoiPool.apply(rows, shape, rois, levels, sizes, sc, c)
    return (y, argmax) if return_argmax else y


# ----------------------------------------------------------------------------- 2x2 max pooling
class _MaxPool2x2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, shape, relu_input=False):
        _chk(x)
        (h, w), n = shape.sizes[0], shape.n_images
        c = x.shape[1]
        y = x.new_empty((n * (h // 2) * (w // 2), c))
        call("scan_maxpool2x2_forward", _ptr(x), n, h, w, c, _ptr(y), _stream())
        ctx.save_for_backward(x, y)
        ctx.dims = (n, h, w, c, int(relu_input))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        n, h, w, c, relu_input = ctx.dims
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        call("scan_maxpool2x2_backward", _ptr(x), _ptr(y), _ptr(dy), n, h, w, c, _ptr(dx), relu_input, _stream())
        return dx, None, None


def maxpool2x2(x, shape, relu_input=False):
    """2x2/2 max-pool of a single-level pyramid; returns (rows, PyramidShape).  relu_input: x is a deferred-ReLU
    conv output (ops.conv2d relu="deferred"): the backward also applies that ReLU's mask."""
    assert shape.n_levels == 1
    (h, w) = shape.sizes[0]
    return _MaxPool2x2.apply(x, shape, relu_input), PyramidShape(shape.n_images, [(h // 2, w // 2)])


def maxpool3x3s2(x, shape):
    """F.max_pool2d(x, 3, 2, 1) of a single-level pyramid (ResNet stem, reference backbone/resnet.py:335).
    Forward only: the stem is frozen for FREEZE_CONV_BODY_AT >= 1."""
    assert shape.n_levels == 1
    _chk(x)
    if x.requires_grad:
        raise RuntimeError("maxpool3x3s2 has no backward: the ResNet stem must be frozen (FREEZE_CONV_BODY_AT >= 1)")
    (h, w), n = shape.sizes[0], shape.n_images
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    y = x.new_empty((n * ho * wo, x.shape[1]))
    call("scan_maxpool3x3s2_forward", _ptr(x), n, h, w, x.shape[1], _ptr(y), _stream())
    return y, PyramidShape(n, [(ho, wo)])


class _Upsample2xAdd(torch.autograd.Function):
    """lateral + nearest-2x-upsampled coarse map (FPN top-down join) in one pass; backward: the gradient itself for the
    lateral, its 2x2 window sums for the coarse map."""

    @staticmethod
    def forward(ctx, lat, coarse, shape_c):
        _chk(lat, coarse)
        (h, w), n = shape_c.sizes[0], shape_c.n_images
        C = lat.shape[1]
        assert coarse.shape == (n * h * w, C) and lat.shape[0] == 4 * n * h * w
        y = torch.empty_like(lat)
        call("scan_upsample2x_add", _ptr(lat), _ptr(coarse), n, h, w, C, _ptr(y), _stream())
        ctx.dims = (n, h, w, C)
        return y

    @staticmethod
    def backward(ctx, g):
        n, h, w, C = ctx.dims
        g = g.contiguous()
        d = g.new_empty((n * h * w, C))
        call("scan_downsample2x_sum", _ptr(g), n, h, w, C, _ptr(d), _stream())
        return g, d, None


def upsample2x_add(lat, coarse, shape_coarse):
    """lat rows of a single-level pyramid twice the size of shape_coarse (exactly: FPN levels of /32-padded frames)."""
    return _Upsample2xAdd.apply(lat, coarse, shape_coarse)


class _AssembleRows(torch.autograd.Function):
    """The row blocks ``parts`` already ARE consecutive row ranges of ``buf`` (convs launched with out=buf[r0:r1]):
    return buf as one tensor; backward hands each producer its rows of the gradient as a view.  Replaces
    torch.cat(parts, 0) -- a read + write of the whole pyramid -- by nothing."""

    @staticmethod
    def forward(ctx, buf, *parts):
        off, offs = 0, []
        for p in parts:
            if p.data_ptr() != buf.data_ptr() + off * buf.shape[1] * buf.element_size() or p.shape[1] != buf.shape[1] \
                    or not p.is_contiguous():
                raise RuntimeError("assemble_rows: parts must be consecutive row ranges of buf")
            offs.append((off, off + p.shape[0]))
            off += p.shape[0]
        if off != buf.shape[0]:
            raise RuntimeError("assemble_rows: parts do not cover buf")
        ctx.offs = offs
        return torch.empty(0, dtype=buf.dtype, device=buf.device).set_(buf.untyped_storage(), buf.storage_offset(),
                                                                      buf.shape, buf.stride())

    @staticmethod
    def backward(ctx, g):
        return (None,) + tuple(g[a:b] for a, b in ctx.offs)


def assemble_rows(buf, parts):
    return _AssembleRows.apply(buf, *parts)


class _AddReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        _chk(a, b)
        assert a.shape == b.shape
        y = torch.empty_like(a)
        call("scan_add_relu", _ptr(a), _ptr(b), _ptr(y), a.numel(), _stream())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = dy.contiguous()
        g = torch.empty_like(dy)
        call("scan_relu_backward", _ptr(dy), _ptr(y), _ptr(g), dy.numel(), _stream())
        return g, g


def add_relu(a, b):
    """max(a + b, 0): the residual join of a bottleneck block."""
    return _AddReLU.apply(a, b)


# ----------------------------------------------------------------------------- GroupNorm + ReLU
def _col_slice_ld(t, C):
    """row stride (floats) of t when it is a [M, C] column slice of a wider row-major fp32 matrix that the kernels can
    address in place (unit column stride, 16-byte aligned rows), else None"""
    if t.dim() == 2 and t.shape[1] == C and t.stride(1) == 1 and t.stride(0) >= C and t.stride(0) % 4 == 0 \
            and t.data_ptr() % 16 == 0:
        return t.stride(0)
    return None


def _gn_plan(shape, C, flags=0):
    """statistics from x or from a conv epilogue's sums, atomic or ordered reductions, workspace sizes: the library decides
    (scan_groupnorm_plan, include/scan_hip.h) -- the compiled operators (csrc/scan_ops_ext.cpp) ask the same function"""
    plan = _lib.GroupNormPlan()
    call("scan_groupnorm_plan", shape.ref(), C, 32, flags, ctypes.byref(plan))
    return plan


class _GroupNormReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, shape, relu, eps, out_buf=None):
        _chk(x, gamma, beta)
        C = x.shape[1]
        # accumulated by the epilogue of the conv that produced x: one launch normalises and leaves (mean, rstd) behind for the
        # backward (SCAN_BATCHED=0: a launch of its own finalises them first)
        sums = _gn_sums.pop(x.data_ptr(), None)
        plan = _gn_plan(shape, C, 0 if sums is None else _lib.GN_SUMS | (0 if BATCHED else _lib.GN_SEPARATE_FINAL))
        stats = x.new_empty((plan.stats_floats,))
        if out_buf is None:
            y, ldy = torch.empty_like(x), C
        else:  # normalise straight into the first C columns of a wider matrix (cat_into completes it)
            if not (out_buf.is_cuda and out_buf.dtype == torch.float32 and out_buf.is_contiguous()
                    and out_buf.shape[0] == x.shape[0] and out_buf.shape[1] >= C and out_buf.shape[1] % 4 == 0):
                raise RuntimeError("groupnorm_relu: out_buf must be a contiguous fp32 [M, >= C] GPU matrix with a row "
                                   "length that is a multiple of 4")
            y, ldy = out_buf[:, :C], out_buf.shape[1]
        ws = torch.empty((plan.fwd_ws_doubles,), dtype=torch.float64, device=x.device) if plan.source == _lib.GN_FROM_X else None
        call("scan_groupnorm_run_forward", ctypes.byref(plan), _ptr(x), shape.ref(), _ptr(sums), eps, _ptr(gamma), _ptr(beta),
             int(relu), _ptr(y), ldy, _ptr(stats), _ptr(ws), _stream())
        ctx.save_for_backward(x, beta, gamma, stats)  # the backward recomputes the ReLU mask from x: y is not kept
        ctx.cfg = (shape, relu)
        ctx.gbuf = ctx.bbuf = None
        if getattr(gamma, "_scan_flat", False) and getattr(beta, "_scan_flat", False) and gamma.grad is not None \
                and beta.grad is not None:
            ctx.gbuf, ctx.bbuf = gamma.grad, beta.grad
        return y

    @staticmethod
    def backward(ctx, dy):
        x, beta, gamma, stats = ctx.saved_tensors
        shape, relu = ctx.cfg
        C = x.shape[1]
        lddy = _col_slice_ld(dy, C)  # e.g. the first C columns of the class-branch conv's data gradient: read in place
        if lddy is None:
            dy, lddy = dy.contiguous(), C
        dx = torch.empty_like(x)
        direct = ctx.gbuf is not None
        dg = ctx.gbuf if direct else x.new_empty((C,))
        db = ctx.bbuf if direct else x.new_empty((C,))
        plan = _gn_plan(shape, C)  # under the knob of the moment, as the forward's
        # atomic sums: a slice of the zeroed pool where there is one.  Ordered: per-block slots, all written by the launch
        ws, cleared = _ws_f64(plan.bwd_ws_doubles, x.device) if not plan.ordered \
            else (torch.empty((plan.bwd_ws_doubles,), dtype=torch.float64, device=x.device), False)
        call("scan_groupnorm_run_backward", ctypes.byref(plan), _ptr(x), _ptr(beta), _ptr(dy), lddy, shape.ref(), _ptr(stats),
             _ptr(gamma), int(relu), _ptr(dx), _ptr(dg), _ptr(db), int(direct), _ptr(ws), int(cleared), _stream())
        return dx, None if direct else dg, None if direct else db, None, None, None, None


def groupnorm_relu(x, gamma, beta, shape, relu=True, eps=1e-5, out_buf=None):
    """out_buf: a contiguous [M, C + e] matrix -- the result is written into (and returned as) its first C columns;
    cat_into() then adds the remaining columns without copying these."""
    return _GroupNormReLU.apply(x, gamma, beta, shape, relu, eps, out_buf)


class _CatInto(torch.autograd.Function):
    """cat([y, extra, zeros], 1) where y already IS the first C columns of ``buf`` (groupnorm_relu(out_buf=buf)): only
    the few extra columns are copied.  Backward: the two column slices of the gradient, as views -- the GroupNorm
    backward reads its slice in place (scan_groupnorm_run_backward's lddy)."""

    @staticmethod
    def forward(ctx, y, extra, buf):
        C, e = y.shape[1], extra.shape[1]
        if y.data_ptr() != buf.data_ptr() or y.stride(0) != buf.shape[1] or C + e > buf.shape[1]:
            raise RuntimeError("cat_into: y must be the leading columns of buf")
        if buf.is_cuda and extra.dtype == torch.float32 and extra.stride(1) == 1:
            # one coalesced pass (scan_copy_cols): the e columns + the zero tail (torch: a strided slice copy + a fill)
            call("scan_copy_cols", _ptr(extra), extra.stride(0), ctypes.c_void_p(buf.data_ptr() + 4 * C), buf.shape[1],
                 buf.shape[0], e, buf.shape[1] - C - e, _stream())
        else:
            buf[:, C:C + e] = extra
            if C + e < buf.shape[1]:
                buf[:, C + e:] = 0
        ctx.cols = (C, e)
        # a fresh tensor object over buf's storage: to autograd the result is not a view of an input
        return torch.empty(0, dtype=buf.dtype, device=buf.device).set_(buf.untyped_storage(), buf.storage_offset(),
                                                                      buf.shape, buf.stride())

    @staticmethod
    def backward(ctx, g):
        C, e = ctx.cols
        return g[:, :C], g[:, C:C + e], None


def cat_into(y, extra, buf):
    return _CatInto.apply(y, extra, buf)


class _PadCols(torch.autograd.Function):
    """[M, K] -> [M, cs] with zero columns behind (F.pad(x, (0, cs - K))) in one pass; backward: the first K columns."""

    @staticmethod
    def forward(ctx, x, cs):
        _chk(x)
        M, K = x.shape
        ctx.k = K
        y = x.new_empty((M, cs))
        call("scan_copy_cols", _ptr(x), K, _ptr(y), cs, M, K, cs - K, _stream())
        return y

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        d = g.new_empty((g.shape[0], ctx.k))
        call("scan_copy_cols", _ptr(g), g.shape[1], _ptr(d), ctx.k, g.shape[0], ctx.k, 0, _stream())
        return d, None


def pad_cols(x, cs):
    return x if x.shape[1] == cs else _PadCols.apply(x, int(cs))


# ----------------------------------------------------------------------------- dynamic conv + softmax
class _DynConvSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, kernels):
        _chk(feat, kernels)
        M, C = feat.shape
        K = kernels.shape[0]
        kernels = kernels.contiguous()
        logits = feat.new_empty((M, K))
        probs = feat.new_empty((M, K))
        call("scan_dynconv_softmax_forward", _ptr(feat), _ptr(kernels), M, C, K, _ptr(logits), _ptr(probs), _stream())
        ctx.save_for_backward(feat, kernels, probs)
        return logits, probs

    @staticmethod
    def backward(ctx, d_logits, d_probs):
        feat, kernels, probs = ctx.saved_tensors
        M, C = feat.shape
        K = kernels.shape[0]
        d_logits = d_logits.contiguous() if d_logits is not None else None
        d_probs = d_probs.contiguous() if d_probs is not None else None
        d_feat = torch.empty_like(feat)
        d_k = torch.empty_like(kernels)
        ws = feat.new_empty((query("scan_dynconv_ws_floats", M, C, K),))
        call("scan_dynconv_softmax_backward", _ptr(feat), _ptr(kernels), _ptr(probs), _ptr(d_logits), _ptr(d_probs), M,
             C, K, _ptr(d_feat), _ptr(d_k), _ptr(ws), _stream())
        return d_feat, d_k


_limits = {}  # constants of the loaded library, asked once


def _limit(name):
    if name not in _limits:
        _limits[name] = int(query(name))
    return _limits[name]


def dynconv_max_classes():
    """largest class count (background included) the dynamic conv is built for"""
    return _limit("scan_dynconv_max_classes")


def dynconv_softmax(feat, kernels):
    """feat [M,256], kernels [K,256] -> (logits [M,K], probs [M,K]); 2 <= K <= dynconv_max_classes().  K = 2 and 9 run
    kernels compiled for them, every other K the generic ones."""
    K = int(kernels.shape[0])
    if not 2 <= K <= dynconv_max_classes():
        raise ValueError("dynconv_softmax: %d classes, the kernels are built for 2..%d" % (K, dynconv_max_classes()))
    return _DynConvSoftmax.apply(feat, kernels)


# ----------------------------------------------------------------------------- losses
class _SigmoidFocalSum(torch.autograd.Function):
    """sum of the element-wise sigmoid focal loss (what SigmoidFocalLoss.forward returns)."""

    @staticmethod
    def forward(ctx, logits, targets, gamma, alpha):
        _chk(logits, targets)
        if logits.dim() != 2:
            raise RuntimeError("logits must be [M, C]")
        if targets.dtype != torch.int32:
            raise RuntimeError("targets must be int32")
        M, C = logits.shape
        out = logits.new_zeros((1,))
        _call_reduction("scan_sigmoid_focal_loss", "_forward", logits, (M, C), _ptr(logits), _ptr(targets), M, C, gamma, alpha, None,
                        _ptr(out))
        ctx.save_for_backward(logits, targets)
        ctx.cfg = (gamma, alpha)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        logits, targets = ctx.saved_tensors
        gamma, alpha = ctx.cfg
        M, C = logits.shape
        d = torch.empty_like(logits)
        dl = g.expand(M, C).contiguous()
        call("scan_sigmoid_focal_loss_backward", _ptr(logits), _ptr(targets), _ptr(dl), 1.0, M, C, gamma, alpha, _ptr(d),
             _stream())
        return d, None, None, None


def sigmoid_focal_loss_sum(logits, targets, gamma, alpha):
    return _SigmoidFocalSum.apply(logits.contiguous(), targets, float(gamma), float(alpha))


class _SigmoidFocalElem(torch.autograd.Function):
    """element-wise losses [M,C]; the _C.sigmoid_focalloss_forward/backward pair."""

    @staticmethod
    def forward(ctx, logits, targets, gamma, alpha):
        _chk(logits, targets)
        M, C = logits.shape
        losses = torch.empty_like(logits)
        call("scan_sigmoid_focal_loss_forward", _ptr(logits), _ptr(targets), M, C, gamma, alpha, _ptr(losses), None,
             _stream())
        ctx.save_for_backward(logits, targets)
        ctx.cfg = (gamma, alpha)
        return losses

    @staticmethod
    def backward(ctx, d_loss):
        logits, targets = ctx.saved_tensors
        gamma, alpha = ctx.cfg
        M, C = logits.shape
        d_loss = d_loss.contiguous()
        d = torch.empty_like(logits)
        call("scan_sigmoid_focal_loss_backward", _ptr(logits), _ptr(targets), _ptr(d_loss), 1.0, M, C, gamma, alpha,
             _ptr(d), _stream())
        return d, None, None, None


class _IouLoss(torch.autograd.Function):
    """the reference's rule (layers/iou_loss.py:32-36): the weighted mean when a weight is given AND sums to more than 0, the plain
    mean otherwise.  Which of the two holds is known on the device only, and nothing here waits for it: with a weight, a second,
    unweighted launch fills out[2:4], torch.where on the device sum of weights picks the pair the value is formed from, and the
    backward gets the weight that goes with it (the weight itself, or ones) and the matching normaliser."""

    @staticmethod
    def forward(ctx, pred, target, weight):
        _chk(pred, target, weight)
        P = pred.shape[0]
        out = pred.new_zeros((4,))
        _call_reduction("scan_iou_loss", "_forward", pred, (P,), _ptr(pred), _ptr(target), _ptr(weight), P, _ptr(out))
        if weight is None:
            use, sel = None, out[:2]
        else:
            _call_reduction("scan_iou_loss", "_forward", pred, (P,), _ptr(pred), _ptr(target), None, P, _ptr(out[2:]))
            use = out[1] > 0
            sel = torch.where(use, out[:2], out[2:])
        ctx.save_for_backward(pred, target, weight, sel, use)
        return sel[0] / sel[1]

    @staticmethod
    def backward(ctx, g):
        pred, target, weight, sel, use = ctx.saved_tensors
        gn = (g / sel[1]).reshape(1).contiguous()
        if weight is not None:
            weight = torch.where(use, weight, 1.0)
        d = torch.empty_like(pred)
        call("scan_iou_loss_backward", _ptr(pred), _ptr(target), _ptr(weight), pred.shape[0], _ptr(gn), _ptr(d),
             _stream())
        return d, None, None


def iou_loss(pred, target, weight=None):
    """weighted mean when weight is given (and sums > 0), plain mean otherwise."""
    return _IouLoss.apply(pred.contiguous(), target.contiguous(), weight.contiguous() if weight is not None else None)


# ----------------------------------------------------------------------------- ground-truth plans of the heads
# (csrc/targets.hip, atss.hip, retina.hip).  Ground truth as modeling.fcos.upload_ground_truth packs it: boxes [N, G, 4] fp32 xyxy
# zero-padded, glab [N, G] int64, ng [N] int32 (the boxes each image has), on the device.  Nothing here reads the device: the
# one host read of a plan (the positive counts) is its builder's, between the assignment and the target step.
def _anchor_geometry(who, shape, strides, cells):
    """(strides table, A) of a head with the cell anchors cells [n_levels, A, 4]"""
    if cells.dim() != 3 or cells.shape[0] != shape.n_levels or cells.shape[2] != 4:
        raise ValueError("%s: cell anchors %r for a pyramid of %d levels" % (who, tuple(cells.shape), shape.n_levels))
    return _level_table(who, shape, ctypes.c_int32, strides, "strides"), int(cells.shape[1])


def _ground_truth(who, shape, boxes, glab, ng):
    if boxes.dim() != 3 or boxes.shape[0] != shape.n_images or boxes.shape[2] != 4 or boxes.shape[1] < 1 or boxes.dtype != torch.float32:
        raise ValueError("%s: boxes must be fp32 [N, G >= 1, 4], got %r" % (who, tuple(boxes.shape)))
    if glab.dtype != torch.int64 or tuple(glab.shape) != tuple(boxes.shape[:2]) or not glab.is_contiguous():
        raise ValueError("%s: box labels must be contiguous int64 [N, G], got %r %s" % (who, tuple(glab.shape), glab.dtype))
    if ng.dtype != torch.int32 or ng.numel() != shape.n_images:
        raise ValueError("%s: ng must be int32 [N]" % who)
    return int(boxes.shape[1])


def _row_vector(who, shape, t, dtype, name, per_row=1):
    if t.dtype != dtype or t.numel() != shape.rows * per_row or not t.is_contiguous():
        raise ValueError("%s: %s must be contiguous %s with %d elements, got %r %s"
                         % (who, name, dtype, shape.rows * per_row, tuple(t.shape), t.dtype))


def _level_counts(who, shape, counts):
    if len(counts) == shape.n_levels and any(not 0 <= int(c) <= shape.n_images * h * w for c, (h, w) in zip(counts, shape.sizes)):
        raise ValueError("%s: positive counts %r beyond the levels' rows" % (who, list(counts)))
    return _level_table(who, shape, ctypes.c_int32, counts, "positive counts")


def _row_lists(shape, device):
    """level_pos int32 [8] and the pos_list / neg_list int32 [M] scan_fcos_compact fills"""
    return (torch.empty((8,), dtype=torch.int32, device=device), torch.empty((shape.rows,), dtype=torch.int32, device=device),
            torch.empty((shape.rows,), dtype=torch.int32, device=device))


def fcos_assign(shape, strides, sizes_of_interest, boxes, glab, ng):
    """The FCOS assignment (reference rpn/fcos/loss.py:40-126) and its compaction, two launches: strides and sizes_of_interest
    [(lo, hi)] per level -> labels int64 [M], labels_i32 [M], reg_targets [M, 4], level_pos int32 [8] (the positives of every
    level, on the device) and pos_list / neg_list int32 [M] (the positive / background rows of every level in row order)."""
    strides_h = _level_table("fcos_assign", shape, ctypes.c_int32, strides, "strides")
    soi_h = _level_table("fcos_assign", shape, ctypes.c_float, [v for lo_hi in sizes_of_interest for v in lo_hi],
                         "sizes of interest", per_level=2)
    G = _ground_truth("fcos_assign", shape, boxes, glab, ng)
    _chk(boxes, glab, ng)
    dev, st = boxes.device, _stream()
    labels = torch.empty((shape.rows,), dtype=torch.int64, device=dev)
    labels_i32 = torch.empty((shape.rows,), dtype=torch.int32, device=dev)
    reg_targets = torch.empty((shape.rows, 4), dtype=torch.float32, device=dev)
    level_pos, pos_list, neg_list = _row_lists(shape, dev)
    call("scan_fcos_assign", shape.ref(), strides_h, soi_h, _ptr(boxes), _ptr(glab), _ptr(ng), G, _ptr(labels), _ptr(labels_i32),
         _ptr(reg_targets), _ptr(level_pos), st)
    call("scan_fcos_compact", shape.ref(), _ptr(labels), _ptr(pos_list), _ptr(neg_list), st)
    return labels, labels_i32, reg_targets, level_pos, pos_list, neg_list


def fcos_nodes(shape, counts, labels, reg_targets, pos_list, neg_list):
    """The positives' targets and the graph-node sampling index (reference rpn/fcos/loss.py:128-133, 428-463) from
    ops.fcos_assign's outputs and counts, the per-level positives read on the host; one launch -> node_index / node_labels
    int64 [nodes], pos_inds int64 [n_pos], reg_pos [n_pos, 4], ctr_pos [n_pos]."""
    cnt_h = _level_counts("fcos_nodes", shape, counts)
    _row_vector("fcos_nodes", shape, labels, torch.int64, "labels")
    _row_vector("fcos_nodes", shape, reg_targets, torch.float32, "reg_targets", 4)
    _row_vector("fcos_nodes", shape, pos_list, torch.int32, "pos_list")
    _row_vector("fcos_nodes", shape, neg_list, torch.int32, "neg_list")
    _chk(labels, reg_targets, pos_list, neg_list)
    dev, n_pos = labels.device, int(sum(counts))
    n_nodes = query("scan_fcos_nodes_count", shape.ref(), cnt_h)
    node_index = torch.empty((n_nodes,), dtype=torch.int64, device=dev)
    node_labels = torch.empty((n_nodes,), dtype=torch.int64, device=dev)
    pos_inds = torch.empty((n_pos,), dtype=torch.int64, device=dev)
    reg_pos = torch.empty((n_pos, 4), dtype=torch.float32, device=dev)
    ctr_pos = torch.empty((n_pos,), dtype=torch.float32, device=dev)
    call("scan_fcos_nodes", shape.ref(), cnt_h, _ptr(labels), _ptr(reg_targets), _ptr(pos_list), _ptr(neg_list), _ptr(node_index),
         _ptr(node_labels), _ptr(pos_inds), _ptr(reg_pos), _ptr(ctr_pos), _stream())
    return node_index, node_labels, pos_inds, reg_pos, ctr_pos


def atss_assign(shape, strides, sizes, topk, boxes, glab, ng):
    """The ATSS assignment (reference rpn/atss/loss.py:159-218; candidates, vote, labels) and scan_fcos_compact: strides and
    anchor sizes per level -> labels int64 [M], labels_i32 [M], matched int32 [M] (the box of every row, 0 where background),
    level_pos int32 [8] on the device and pos_list / neg_list int32 [M]."""
    strides_h = _level_table("atss_assign", shape, ctypes.c_int32, strides, "strides")
    sizes_h = _level_table("atss_assign", shape, ctypes.c_float, sizes, "anchor sizes")
    G = _ground_truth("atss_assign", shape, boxes, glab, ng)
    if int(topk) < 1:
        raise ValueError("atss_assign: topk %r < 1" % (topk,))
    _chk(boxes, glab, ng)
    dev, st = boxes.device, _stream()
    labels = torch.empty((shape.rows,), dtype=torch.int64, device=dev)
    labels_i32 = torch.empty((shape.rows,), dtype=torch.int32, device=dev)
    matched = torch.empty((shape.rows,), dtype=torch.int32, device=dev)
    level_pos, pos_list, neg_list = _row_lists(shape, dev)
    ws = torch.empty((query("scan_atss_assign_ws_bytes", shape.ref(), G, int(topk)) // 8,), dtype=torch.int64, device=dev)
    call("scan_atss_assign", shape.ref(), strides_h, sizes_h, _ptr(boxes), _ptr(glab), _ptr(ng), G, int(topk), _ptr(labels),
         _ptr(labels_i32), _ptr(matched), _ptr(level_pos), _ptr(ws), st)
    call("scan_fcos_compact", shape.ref(), _ptr(labels), _ptr(pos_list), _ptr(neg_list), st)
    return labels, labels_i32, matched, level_pos, pos_list, neg_list


def atss_targets(shape, strides, sizes, counts, boxes, matched, pos_list):
    """The positives of an ATSS plan from ops.atss_assign's outputs and counts, the per-level positives read on the host; one
    launch (none without positives) -> pos_inds int64 [n_pos], reg_pos [n_pos, 4] (BoxCoder.encode of the matched box against
    the row's anchor), ctr_pos [n_pos]."""
    strides_h = _level_table("atss_targets", shape, ctypes.c_int32, strides, "strides")
    sizes_h = _level_table("atss_targets", shape, ctypes.c_float, sizes, "anchor sizes")
    cnt_h = _level_counts("atss_targets", shape, counts)
    if boxes.dim() != 3 or boxes.shape[0] != shape.n_images or boxes.shape[2] != 4 or boxes.shape[1] < 1 or boxes.dtype != torch.float32:
        raise ValueError("atss_targets: boxes must be fp32 [N, G >= 1, 4], got %r" % (tuple(boxes.shape),))
    _row_vector("atss_targets", shape, matched, torch.int32, "matched")
    _row_vector("atss_targets", shape, pos_list, torch.int32, "pos_list")
    _chk(boxes, matched, pos_list)
    dev, n_pos = boxes.device, int(sum(counts))
    pos_inds = torch.empty((n_pos,), dtype=torch.int64, device=dev)
    reg_pos = torch.empty((n_pos, 4), dtype=torch.float32, device=dev)
    ctr_pos = torch.empty((n_pos,), dtype=torch.float32, device=dev)
    call("scan_atss_targets", shape.ref(), strides_h, sizes_h, cnt_h, _ptr(boxes), int(boxes.shape[1]), _ptr(matched),
         _ptr(pos_list), _ptr(pos_inds), _ptr(reg_pos), _ptr(ctr_pos), _stream())
    return pos_inds, reg_pos, ctr_pos


def retina_match(shape, strides, cells, boxes, glab, ng, bg_thr, fg_thr, who="retina_match"):
    """The Matcher with allow_low_quality_matches (reference modeling/matcher.py:42-112) over the anchors of cells [n_levels,
    A, 4] (on the device), two launches -> labels_i32 [M * A] (0 below bg_thr, -1 between the thresholds, else the matched
    box's label), matched int32 [M * A] (0 where label <= 0) and the number of positives, int32 [1] on the device."""
    strides_h, A = _anchor_geometry(who, shape, strides, cells)
    G = _ground_truth(who, shape, boxes, glab, ng)
    if not float(bg_thr) <= float(fg_thr):
        raise ValueError("%s: bg_thr %r above fg_thr %r" % (who, bg_thr, fg_thr))
    _chk(cells, boxes, glab, ng)
    dev = boxes.device
    labels = torch.empty((shape.rows * A,), dtype=torch.int32, device=dev)
    matched = torch.empty((shape.rows * A,), dtype=torch.int32, device=dev)
    n_pos = torch.empty((1,), dtype=torch.int32, device=dev)
    ws = torch.empty((query("scan_retina_match_ws_bytes", shape.ref(), G) // 4,), dtype=torch.int32, device=dev)
    call("scan_retina_match", shape.ref(), strides_h, _ptr(cells), A, _ptr(boxes), _ptr(glab), _ptr(ng), G, float(bg_thr),
         float(fg_thr), _ptr(labels), _ptr(matched), _ptr(n_pos), _ptr(ws), _stream())
    return labels, matched, n_pos


def paradigm_update_(P, pb, it):
    """GRAPHModule.update_prototype_nx1_rnn with COSINE_UPDATE_ON (reference rpn/fcos/condgraph.py:586-606) on the paradigm
    buffer P [K, C, T] in place, one launch: slot ``it`` (the last one, after shifting the others down, when it == T) moves
    towards the batch means pb [K, C] by their cosine similarity; classes whose mean is all zero keep their value."""
    if P.dim() != 3 or P.dtype != torch.float32 or not P.is_contiguous() or P.shape[1] > 1024:
        raise ValueError("paradigm_update_: P must be contiguous fp32 [K, C <= 1024, T], got %r %s" % (tuple(P.shape), P.dtype))
    if tuple(pb.shape) != tuple(P.shape[:2]):
        raise ValueError("paradigm_update_: pb %r for P %r" % (tuple(pb.shape), tuple(P.shape)))
    if not 0 <= int(it) <= P.shape[2]:
        raise ValueError("paradigm_update_: it %r outside 0..%d" % (it, P.shape[2]))
    pb = pb.contiguous().float()
    _chk(P, pb)
    call("scan_paradigm_update", _ptr(P), _ptr(pb), P.shape[0], P.shape[1], P.shape[2], int(it), _stream())


class _AtssGiouLoss(torch.autograd.Function):
    """sum(w * (1 - GIoU)) / sum(w) of anchor deltas (reference rpn/atss/loss.py:64-105, 396-397); the anchors are formed in the
    kernel from the rows (csrc/atss.hip).  The weight is a target (the centerness of the matched box): no gradient to it."""

    @staticmethod
    def forward(ctx, pred, target, rows, weight, shape, strides, sizes):
        _chk(pred, target, rows, weight)
        P = pred.shape[0]
        out = pred.new_zeros((2,))
        geo = (shape.ref(), strides, sizes)
        _call_reduction("scan_atss_giou", "_forward", pred, (P,), *geo, _ptr(pred), _ptr(target), _ptr(rows), _ptr(weight), P,
                        _ptr(out))
        ctx.save_for_backward(pred, target, rows, weight, out)
        ctx.geo = geo + (shape,)  # (the shape owns the descriptor geo[0] points to)
        return out[0] / out[1]

    @staticmethod
    def backward(ctx, g):
        pred, target, rows, weight, out = ctx.saved_tensors
        gn = (g / out[1]).reshape(1).contiguous()
        d = torch.empty_like(pred)
        call("scan_atss_giou_backward", *ctx.geo[:3], _ptr(pred), _ptr(target), _ptr(rows), _ptr(weight), pred.shape[0], _ptr(gn),
             _ptr(d), _stream())
        return d, None, None, None, None, None, None


def atss_giou_loss(pred, target, rows, weight, shape, strides, sizes):
    """pred / target [P, 4] BoxCoder deltas of the pyramid rows ``rows`` [P] int64, weight [P]: the centerness-weighted GIoU
    loss of the ATSS head, normalised by the sum of the weights."""
    return _AtssGiouLoss.apply(pred.contiguous(), target.contiguous(), rows.contiguous(), weight.contiguous(), shape,
                               _level_table("atss_giou_loss", shape, ctypes.c_int32, strides, "strides"),
                               _level_table("atss_giou_loss", shape, ctypes.c_float, sizes, "anchor sizes"))


class _RetinaSmoothL1(torch.autograd.Function):
    """sum over the anchors with label > 0 of smooth_l1(bbox_reg slice - BoxCoder.encode(matched box, anchor)) (reference
    rpn/retinanet/loss.py:66-71, layers/smooth_l1_loss.py with size_average=False); anchors and targets are formed in the
    kernel (csrc/retina.hip), over all M * A anchors.  bbox_reg is read in place through its row pitch."""

    @staticmethod
    def forward(ctx, bbox_reg, geo, boxes, labels_i32, matched, beta, targets_out):
        shape, strides, cells, A = geo
        _chk(boxes, labels_i32, matched, cells, targets_out)
        ld = _row_pitch(bbox_reg, 4 * A, "bbox_reg", who="retina_smooth_l1_loss")
        out = bbox_reg.new_zeros((1,))
        args = (shape.ref(), strides, _ptr(cells), A, _ptr(boxes), boxes.shape[1], _ptr(labels_i32), _ptr(matched), _ptr(bbox_reg),
                ld, beta)
        _call_reduction("scan_retina_smooth_l1", "_forward", bbox_reg, (shape.rows * A,), *args, _ptr(targets_out), _ptr(out))
        ctx.save_for_backward(bbox_reg, boxes, labels_i32, matched, cells)
        ctx.args = args + (shape,)  # (the shape owns the descriptor args[0] points to)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        bbox_reg = ctx.saved_tensors[0]
        d = torch.empty(bbox_reg.shape, dtype=torch.float32, device=bbox_reg.device)
        call("scan_retina_smooth_l1_backward", *ctx.args[:-1], _ptr(g.reshape(1).contiguous()), _ptr(d), d.shape[1], _stream())
        return d, None, None, None, None, None, None


def retina_smooth_l1_loss(bbox_reg, shape, strides, cells, boxes, labels_i32, matched, beta, targets_out=None):
    """bbox_reg [M, 4 A] (a column slice of a wider row matrix is read in place through its pitch), cells [n_levels, A, 4] the
    cell anchors on the device, boxes [N, G, 4], labels_i32 / matched [M * A] of the RetinaNet plan: the summed smooth-L1 loss
    of the positive anchors against their encoded boxes.  targets_out [M * A, 4] (optional) receives the targets."""
    strides_h, A = _anchor_geometry("retina_smooth_l1_loss", shape, strides, cells)
    if bbox_reg.dim() != 2 or bbox_reg.shape != (shape.rows, 4 * A):
        raise ValueError("retina_smooth_l1_loss: bbox_reg %r for %d rows of %d anchors" % (tuple(bbox_reg.shape), shape.rows, A))
    if labels_i32.dtype != torch.int32 or matched.dtype != torch.int32 or labels_i32.numel() != shape.rows * A \
            or matched.numel() != shape.rows * A:
        raise ValueError("retina_smooth_l1_loss: labels / matched must be int32 [M * A]")
    if targets_out is not None and (targets_out.shape != (shape.rows * A, 4) or targets_out.dtype != torch.float32):
        raise ValueError("retina_smooth_l1_loss: targets_out must be fp32 [M * A, 4]")
    return _RetinaSmoothL1.apply(bbox_reg, (shape, strides_h, cells, A), boxes, labels_i32, matched, float(beta), targets_out)


# ----------------------------------------------------------------------------- region-proposal network (csrc/rpn.hip)
def _rpn_image_hw(who, shape, image_hw):
    if image_hw.dtype != torch.int32 or tuple(image_hw.shape) != (shape.n_images, 2) or not image_hw.is_contiguous():
        raise ValueError("%s: image_hw must be int32 [N, 2] (height, width), got %r %s" % (who, tuple(image_hw.shape), image_hw.dtype))


def rpn_labels(shape, strides, cells, boxes, ng, image_hw, bg_thr, fg_thr, straddle_thresh):
    """RPN labels of every anchor (reference rpn/loss.py:56-89): 1 matched (IoU >= fg_thr, or a low-quality match), 0 below
    bg_thr, -1 between the thresholds or not visible in its image.  boxes [N, G, 4] fp32, ng [N] int32, image_hw [N, 2] int32
    (height, width), all on the device.  -> labels_i32 [M * A], matched [M * A] int32.  The matcher's two launches with every
    box label 1, then the visibility launch (none when straddle_thresh < 0); no host read."""
    strides_h, A = _anchor_geometry("rpn_labels", shape, strides, cells)
    _rpn_image_hw("rpn_labels", shape, image_hw)
    if image_hw.device != boxes.device:  # (the matcher refuses boxes that are not on the GPU)
        raise ValueError("rpn_labels: image_hw on %s, boxes on %s" % (image_hw.device, boxes.device))
    glab = torch.ones(tuple(boxes.shape[:2]), dtype=torch.int64, device=boxes.device)
    # the matcher's positive counter is not read here: the visibility launch makes it stale, and the sampler counts
    labels, matched, _ = retina_match(shape, strides, cells, boxes, glab, ng, bg_thr, fg_thr, who="rpn_labels")
    call("scan_rpn_visibility", shape.ref(), strides_h, _ptr(cells), A, _ptr(image_hw), float(straddle_thresh), _ptr(labels),
         _ptr(matched), _stream())
    return labels, matched


def rpn_sample(shape, A, labels_i32, batch_size_per_image, positive_fraction, seed=0, keys=None):
    """BalancedPositiveNegativeSampler on the device, one launch for all images: per image the int(batch_size_per_image *
    positive_fraction) positives (label >= 1) and then the negatives (label == 0) with the smallest (key, anchor index) pairs;
    the key is the integer mix of (seed, image, anchor index) written out in include/scan_hip.h, or keys [M * A] (int32 /
    uint32 bits) when given.  -> sampled uint8 [M * A] (1 positive, 2 negative, 0 not sampled), counts int32 [N, 2]."""
    n = shape.rows * int(A)
    if labels_i32.dtype != torch.int32 or labels_i32.numel() != n:
        raise ValueError("rpn_sample: labels_i32 must be int32 [M * A] = [%d]" % n)
    if int(batch_size_per_image) < 1:
        raise ValueError("rpn_sample: batch_size_per_image %r < 1" % (batch_size_per_image,))
    if not 0 < float(positive_fraction) <= 1:
        raise ValueError("rpn_sample: positive_fraction %r outside (0, 1]" % (positive_fraction,))
    if keys is not None and (keys.dtype not in (torch.int32, torch.uint32) or keys.numel() != n or not keys.is_contiguous()):
        raise ValueError("rpn_sample: keys must be 32-bit integers [M * A]")
    _chk(labels_i32, keys)
    sampled = torch.empty((n,), dtype=torch.uint8, device=labels_i32.device)
    counts = torch.empty((shape.n_images, 2), dtype=torch.int32, device=labels_i32.device)
    call("scan_rpn_sample", shape.ref(), int(A), _ptr(labels_i32), int(batch_size_per_image),
         int(int(batch_size_per_image) * float(positive_fraction)), int(seed) & 0xffffffff, _ptr(keys), _ptr(sampled), _ptr(counts),
         _stream())
    return sampled, counts


class _RpnLoss(torch.autograd.Function):
    """(sum of the objectness BCE over the sampled anchors, sum of smooth-L1 over the sampled positives) as a [2] tensor
    (reference rpn/loss.py:92-131 before the division by the sampled count); anchors and encoded targets are formed in the
    kernel (csrc/rpn.hip), over all M * A anchors.  Both head outputs are read in place through their row pitches."""

    @staticmethod
    def forward(ctx, objectness, bbox_reg, geo, boxes, matched, sampled, beta, targets_out):
        shape, strides, cells, A = geo
        _chk(boxes, matched, sampled, cells, targets_out)
        ld_obj = _row_pitch(objectness, A, "objectness", who="rpn_loss")
        ld_reg = _row_pitch(bbox_reg, 4 * A, "bbox_reg", who="rpn_loss")
        out = bbox_reg.new_zeros((2,))
        args = (shape.ref(), strides, _ptr(cells), A, _ptr(boxes), boxes.shape[1], _ptr(matched), _ptr(sampled), _ptr(objectness),
                ld_obj, _ptr(bbox_reg), ld_reg, beta)
        _call_reduction("scan_rpn_loss", "_forward", bbox_reg, (shape.rows * A,), *args, _ptr(targets_out), _ptr(out))
        ctx.save_for_backward(objectness, bbox_reg, boxes, matched, sampled, cells)
        ctx.args = args + (shape,)  # (the shape owns the descriptor args[0] points to)
        return out

    @staticmethod
    def backward(ctx, g):
        objectness, bbox_reg = ctx.saved_tensors[:2]
        d_obj = torch.empty(objectness.shape, dtype=torch.float32, device=objectness.device)
        d_reg = torch.empty(bbox_reg.shape, dtype=torch.float32, device=bbox_reg.device)
        call("scan_rpn_loss_backward", *ctx.args[:-1], _ptr(g.reshape(2).contiguous()), _ptr(d_obj), d_obj.shape[1], _ptr(d_reg),
             d_reg.shape[1], _stream())
        return d_obj, d_reg, None, None, None, None, None, None


def rpn_loss(objectness, bbox_reg, shape, strides, cells, boxes, matched, sampled, beta, targets_out=None):
    """objectness [M, A] and bbox_reg [M, 4 A] (column slices of wider row matrices are read in place), cells [n_levels, A, 4]
    on the device, boxes [N, G, 4], matched int32 [M * A] (ops.rpn_labels), sampled uint8 [M * A] (ops.rpn_sample) -> [2]:
    the summed BCE-with-logits of the sampled anchors (target 1 where sampled == 1, 0 where sampled == 2) and the summed
    smooth-L1 of the sampled positives against BoxCoder.encode (weights 1) of their matched boxes.  targets_out [M * A, 4]
    (optional) receives the encoded targets."""
    strides_h, A = _anchor_geometry("rpn_loss", shape, strides, cells)
    n = shape.rows * A
    if objectness.dim() != 2 or tuple(objectness.shape) != (shape.rows, A):
        raise ValueError("rpn_loss: objectness %r for %d rows of %d anchors" % (tuple(objectness.shape), shape.rows, A))
    if bbox_reg.dim() != 2 or tuple(bbox_reg.shape) != (shape.rows, 4 * A):
        raise ValueError("rpn_loss: bbox_reg %r for %d rows of %d anchors" % (tuple(bbox_reg.shape), shape.rows, A))
    if boxes.dim() != 3 or boxes.shape[0] != shape.n_images or boxes.shape[2] != 4 or boxes.shape[1] < 1:
        raise ValueError("rpn_loss: boxes must be fp32 [N, G >= 1, 4], got %r" % (tuple(boxes.shape),))
    if matched.dtype != torch.int32 or matched.numel() != n:
        raise ValueError("rpn_loss: matched must be int32 [M * A]")
    if sampled.dtype != torch.uint8 or sampled.numel() != n:
        raise ValueError("rpn_loss: sampled must be uint8 [M * A]")
    if targets_out is not None and (tuple(targets_out.shape) != (n, 4) or targets_out.dtype != torch.float32):
        raise ValueError("rpn_loss: targets_out must be fp32 [M * A, 4]")
    if not float(beta) > 0:
        raise ValueError("rpn_loss: beta %r must be positive" % (beta,))
    return _RpnLoss.apply(objectness, bbox_reg, (shape, strides_h, cells, A), boxes, matched, sampled, float(beta), targets_out)


def rpn_decode_proposals(bbox_reg, shape, strides, cells, topk_idx, ks, image_hw, min_size=0):
    """The decode / clip / small-box step of the proposal selection (reference rpn/inference.py:95-113) in one launch: topk_idx
    [N, sum(ks)] int64, the per-level top-k anchor indices within each image's level side by side (ks[l] columns for level l)
    -> boxes [N, K, 4] clipped to the image, keep [N, K] uint8 (both extents >= min_size)."""
    strides_h, A = _anchor_geometry("rpn_decode_proposals", shape, strides, cells)
    if bbox_reg.dim() != 2 or tuple(bbox_reg.shape) != (shape.rows, 4 * A):
        raise ValueError("rpn_decode_proposals: bbox_reg %r for %d rows of %d anchors" % (tuple(bbox_reg.shape), shape.rows, A))
    if len(ks) != shape.n_levels or any(not 0 <= int(k) <= h * w * A for k, (h, w) in zip(ks, shape.sizes)):
        raise ValueError("rpn_decode_proposals: ks %r: one candidate count per level, at most h * w * A" % (tuple(ks),))
    K = sum(int(k) for k in ks)
    if topk_idx.dtype != torch.int64 or tuple(topk_idx.shape) != (shape.n_images, K) or not topk_idx.is_contiguous():
        raise ValueError("rpn_decode_proposals: topk_idx must be contiguous int64 [N, sum(ks)] = [%d, %d]" % (shape.n_images, K))
    _rpn_image_hw("rpn_decode_proposals", shape, image_hw)
    _chk(cells, topk_idx, image_hw)
    ld = _row_pitch(bbox_reg, 4 * A, "bbox_reg", who="rpn_decode_proposals")
    off = [0]
    for k in ks:
        off.append(off[-1] + int(k))
    boxes = torch.empty((shape.n_images, K, 4), dtype=torch.float32, device=bbox_reg.device)
    keep = torch.empty((shape.n_images, K), dtype=torch.uint8, device=bbox_reg.device)
    call("scan_rpn_decode", shape.ref(), strides_h, _ptr(cells), A, _ptr(bbox_reg), ld, _ptr(topk_idx),
         (ctypes.c_int32 * len(off))(*off), _ptr(image_hw), float(min_size), _ptr(boxes), _ptr(keep), _stream())
    return boxes, keep


# ----------------------------------------------------------------------------- Fast R-CNN box head (csrc/roi_box.hip)
# Proposals of a batch are padded as the ground truth is: props [N, P, 4] fp32 xyxy, n_props [N] int32, on the device.
def _roi_box_props(who, props, n_props=None):
    if props.dim() != 3 or props.shape[2] != 4 or props.shape[0] < 1 or props.shape[1] < 1 or props.dtype != torch.float32:
        raise ValueError("%s: proposals must be fp32 [N >= 1, P >= 1, 4], got %r %s" % (who, tuple(props.shape), props.dtype))
    if props.shape[0] * props.shape[1] >= 2 ** 31:
        raise ValueError("%s: 2^31 proposals or more" % who)
    if n_props is not None and (n_props.dtype != torch.int32 or n_props.numel() != props.shape[0]):
        raise ValueError("%s: proposal counts must be int32 [N]" % who)
    return int(props.shape[0]), int(props.shape[1])


def _roi_box_weights(who, weights):
    weights = tuple(float(w) for w in weights)
    if len(weights) != 4 or not all(w > 0 for w in weights):
        raise ValueError("%s: box coder weights %r: four positive numbers (wx, wy, ww, wh)" % (who, weights))
    return weights


def _roi_box_plan_vector(who, t, dtype, n, name):
    if t.dtype != dtype or t.numel() != n or not t.is_contiguous():
        raise ValueError("%s: %s must be contiguous %s with N * P = %d elements, got %r %s" % (who, name, dtype, n, tuple(t.shape), t.dtype))


def roi_box_match(props, n_props, boxes, glab, ng, bg_thr, fg_thr):
    """The Matcher without the low-quality rule (reference roi_heads/box_head/loss.py:39-70) of padded proposals against the
    padded ground truth (boxes [N, G, 4], glab [N, G] int64, ng [N] int32), one launch -> labels_i32 [N * P] (0 below bg_thr,
    -1 between the thresholds and on padding rows, else the matched box's label), matched int32 [N * P] (0 where label <= 0)."""
    N, P = _roi_box_props("roi_box_match", props, n_props)
    G = _ground_truth("roi_box_match", PyramidShape(N, [(P, 1)]), boxes, glab, ng)
    if not float(bg_thr) <= float(fg_thr):
        raise ValueError("roi_box_match: bg_thr %r above fg_thr %r" % (bg_thr, fg_thr))
    _chk(props, n_props, boxes, glab, ng)
    labels = torch.empty((N * P,), dtype=torch.int32, device=props.device)
    matched = torch.empty((N * P,), dtype=torch.int32, device=props.device)
    call("scan_roi_box_match", _ptr(props), _ptr(n_props), N, P, _ptr(boxes), _ptr(glab), _ptr(ng), G, float(bg_thr), float(fg_thr),
         _ptr(labels), _ptr(matched), _stream())
    return labels, matched


def roi_box_gather(props, boxes, labels_i32, matched, sampled, counts, R, weights=(10., 10., 5., 5.)):
    """The sampled proposals of every image in one launch (reference loss.py:108-113: proposals[img][nonzero(pos | neg)]), image
    by image and by ascending proposal index: sampled uint8 [N * P] and counts int32 [N, 2] of ops.rpn_sample on
    PyramidShape(N, [(P, 1)]) with A = 1, R their total (read on the host by the caller) -> rois [R, 5] (image index, box),
    labels int32 [R] (0 for a sampled negative), reg_targets [R, 4] (BoxCoder.encode with ``weights`` of the matched box where
    label > 0, zero elsewhere), src int32 [R] (the proposal's index within its image)."""
    N, P = _roi_box_props("roi_box_gather", props)
    if boxes.dim() != 3 or boxes.shape[0] != N or boxes.shape[2] != 4 or boxes.shape[1] < 1 or boxes.dtype != torch.float32:
        raise ValueError("roi_box_gather: boxes must be fp32 [N, G >= 1, 4], got %r" % (tuple(boxes.shape),))
    _roi_box_plan_vector("roi_box_gather", labels_i32, torch.int32, N * P, "labels_i32")
    _roi_box_plan_vector("roi_box_gather", matched, torch.int32, N * P, "matched")
    _roi_box_plan_vector("roi_box_gather", sampled, torch.uint8, N * P, "sampled")
    if counts.dtype != torch.int32 or tuple(counts.shape) != (N, 2) or not counts.is_contiguous():
        raise ValueError("roi_box_gather: counts must be contiguous int32 [N, 2], got %r %s" % (tuple(counts.shape), counts.dtype))
    if not 0 <= int(R) <= N * P:
        raise ValueError("roi_box_gather: R %r outside 0..N * P = %d" % (R, N * P))
    wx, wy, ww, wh = _roi_box_weights("roi_box_gather", weights)
    _chk(props, boxes, labels_i32, matched, sampled, counts)
    dev, R = props.device, int(R)
    rois = torch.empty((R, 5), dtype=torch.float32, device=dev)
    labels = torch.empty((R,), dtype=torch.int32, device=dev)
    reg_targets = torch.empty((R, 4), dtype=torch.float32, device=dev)
    src = torch.empty((R,), dtype=torch.int32, device=dev)
    call("scan_roi_box_gather", _ptr(props), N, P, _ptr(boxes), int(boxes.shape[1]), _ptr(labels_i32), _ptr(matched), _ptr(sampled),
         _ptr(counts), wx, wy, ww, wh, R, _ptr(rois), _ptr(labels), _ptr(reg_targets), _ptr(src), _stream())
    return rois, labels, reg_targets, src


def _roi_box_head_outputs(who, class_logits, box_regression):
    """(R, C, Cr) of the predictor's outputs: class_logits [R, C >= 2], box_regression [R, 4 C] or [R, 8] (class-agnostic)"""
    if class_logits.dim() != 2 or class_logits.shape[1] < 2 or class_logits.dtype != torch.float32:
        raise ValueError("%s: class_logits must be fp32 [R, C >= 2], got %r %s" % (who, tuple(class_logits.shape), class_logits.dtype))
    R, C = int(class_logits.shape[0]), int(class_logits.shape[1])
    if box_regression.dim() != 2 or box_regression.shape[0] != R or box_regression.shape[1] not in (4 * C, 8) \
            or box_regression.dtype != torch.float32:
        raise ValueError("%s: box_regression %r %s for class_logits %r: fp32 [R, 4 C] or [R, 8] (class-agnostic)"
                         % (who, tuple(box_regression.shape), box_regression.dtype, tuple(class_logits.shape)))
    if R > 2 ** 30:
        raise ValueError("%s: more than 2^30 rows" % who)
    for t, name in ((class_logits, "class_logits"), (box_regression, "box_regression")):
        if R > 0 and (t.stride(1) != 1 or t.stride(0) < t.shape[1]):
            raise ValueError("%s: %s must have contiguous rows" % (who, name))
    if R > 0 and (box_regression.stride(0) % 4 != 0 or box_regression.data_ptr() % 16 != 0):
        raise ValueError("%s: box_regression must start 16-byte aligned with a row pitch that is a multiple of 4" % who)
    return R, C, int(box_regression.shape[1]) // 4


def _pitch(t):
    """the row pitch of a head output (a column slice of a wider matrix is taken as it is); GPU tensors only"""
    if not t.is_cuda:
        raise RuntimeError("scan_amd ops run only on the GPU (HIP) -- got a %s tensor; no CPU fallback" % t.device)
    return int(t.stride(0)) if t.shape[0] > 0 else int(t.shape[1])


class _RoiBoxLoss(torch.autograd.Function):
    """(sum of the cross-entropy over the R sampled rows, sum of the class-specific smooth-L1 over the positives) as a [2] tensor
    (reference roi_heads/box_head/loss.py:146-164 before the divisions by R; csrc/roi_box.hip).  Both head outputs are read in
    place through their row pitches."""

    @staticmethod
    def forward(ctx, class_logits, box_regression, dims, labels, reg_targets):
        R, C, Cr = dims
        _chk(labels, reg_targets)
        out = class_logits.new_zeros((2,))
        args = (_ptr(class_logits), _pitch(class_logits), _ptr(box_regression), _pitch(box_regression), R, C, Cr, _ptr(labels),
                _ptr(reg_targets))
        _call_reduction("scan_roi_box_loss", "_forward", class_logits, (R,), *args, _ptr(out))
        ctx.save_for_backward(class_logits, box_regression, labels, reg_targets)
        ctx.args = args
        return out

    @staticmethod
    def backward(ctx, g):
        class_logits, box_regression = ctx.saved_tensors[:2]
        d_cls = torch.empty(class_logits.shape, dtype=torch.float32, device=class_logits.device)
        d_reg = torch.empty(box_regression.shape, dtype=torch.float32, device=box_regression.device)
        call("scan_roi_box_loss_backward", *ctx.args, _ptr(g.reshape(2).contiguous()), _ptr(d_cls), d_cls.shape[1], _ptr(d_reg),
             d_reg.shape[1], _stream())
        return d_cls, d_reg, None, None, None


def roi_box_loss(class_logits, box_regression, labels, reg_targets):
    """class_logits [R, C] and box_regression [R, 4 C] ([R, 8]: class-agnostic; column slices of a wider row matrix are read in
    place), labels int32 [R] and reg_targets [R, 4] of ops.roi_box_gather -> [2]: the summed cross-entropy of every row and the
    summed smooth-L1 (beta 1) of the positives' own four regression columns.  The caller divides both by R."""
    R, C, Cr = _roi_box_head_outputs("roi_box_loss", class_logits, box_regression)
    if labels.dtype != torch.int32 or tuple(labels.shape) != (R,) or not labels.is_contiguous():
        raise ValueError("roi_box_loss: labels must be contiguous int32 [R] = [%d], got %r %s" % (R, tuple(labels.shape), labels.dtype))
    if reg_targets.dtype != torch.float32 or tuple(reg_targets.shape) != (R, 4) or not reg_targets.is_contiguous():
        raise ValueError("roi_box_loss: reg_targets must be contiguous fp32 [R, 4], got %r %s" % (tuple(reg_targets.shape), reg_targets.dtype))
    return _RoiBoxLoss.apply(class_logits, box_regression, (R, C, Cr), labels, reg_targets)


def roi_box_decode(class_logits, box_regression, rois, image_hw, weights=(10., 10., 5., 5.), score_thresh=0.05):
    """The test-time softmax, BoxCoder.decode, clip and score threshold of every (ROI, class) in one launch (reference
    roi_heads/box_head/inference.py:55-84, 118): rois [R, 5] (image index, box), image_hw int32 [N, 2] on the device -> scores
    [R, C], boxes [R, C, 4] clipped to the ROI's image, cand uint8 [R, C] (class >= 1 and score > score_thresh)."""
    R, C, Cr = _roi_box_head_outputs("roi_box_decode", class_logits, box_regression)
    if rois.dtype != torch.float32 or tuple(rois.shape) != (R, 5) or not rois.is_contiguous():
        raise ValueError("roi_box_decode: rois must be contiguous fp32 [R, 5] = [%d, 5], got %r %s" % (R, tuple(rois.shape), rois.dtype))
    if image_hw.dtype != torch.int32 or image_hw.dim() != 2 or image_hw.shape[0] < 1 or image_hw.shape[1] != 2 \
            or not image_hw.is_contiguous():
        raise ValueError("roi_box_decode: image_hw must be contiguous int32 [N >= 1, 2] (height, width), got %r %s"
                         % (tuple(image_hw.shape), image_hw.dtype))
    wx, wy, ww, wh = _roi_box_weights("roi_box_decode", weights)
    _chk(rois, image_hw)
    dev = class_logits.device
    scores = torch.empty((R, C), dtype=torch.float32, device=dev)
    boxes = torch.empty((R, C, 4), dtype=torch.float32, device=dev)
    cand = torch.empty((R, C), dtype=torch.uint8, device=dev)
    call("scan_roi_box_decode", _ptr(class_logits), _pitch(class_logits), _ptr(box_regression), _pitch(box_regression), R, C, Cr,
         _ptr(rois), _ptr(image_hw), int(image_hw.shape[0]), wx, wy, ww, wh, float(score_thresh), _ptr(scores), _ptr(boxes),
         _ptr(cand), _stream())
    return scores, boxes, cand


# ----------------------------------------------------------------------------- Mask R-CNN mask head (csrc/roi_mask.hip)
# Ground-truth masks of a batch: masks uint8 [sum G_n h_n w_n] flat, moff int64 [N + 1], mhw int32 [N, 2] (h, w), on the device.
def _roi_mask_vector(who, t, dtype, n, name):
    if t.dtype != dtype or tuple(t.shape) != (n,) or not t.is_contiguous():
        raise ValueError("%s: %s must be contiguous %s [%d], got %r %s" % (who, name, dtype, n, tuple(t.shape), t.dtype))


def _roi_mask_rois(who, rois, n=None):
    if rois.dtype != torch.float32 or rois.dim() != 2 or rois.shape[1] != 5 or not rois.is_contiguous() \
            or (n is not None and rois.shape[0] != n):
        raise ValueError("%s: rois must be contiguous fp32 [%s, 5], got %r %s" % (who, "R" if n is None else n, tuple(rois.shape), rois.dtype))
    return int(rois.shape[0])


def _roi_mask_size(who, M):
    if not 1 <= int(M) <= 1024:
        raise ValueError("%s: mask size M %r outside 1..1024" % (who, M))
    return int(M)


def _roi_mask_logits(who, logits, n, M, C):
    """the conv output rows [n M M, Cs] holding C classes in their first columns -> C"""
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.shape[0] != n * M * M:
        raise ValueError("%s: logits must be fp32 rows [%d * %d * %d, Cs], got %r %s" % (who, n, M, M, tuple(logits.shape), logits.dtype))
    C = int(logits.shape[1] if C is None else C)
    if not 1 <= C <= logits.shape[1]:
        raise ValueError("%s: C %r classes in rows of %d columns" % (who, C, logits.shape[1]))
    if n * M * M >= 2 ** 31:
        raise ValueError("%s: 2^31 mask elements or more" % who)
    if n > 0 and (logits.stride(1) != 1 or logits.stride(0) < logits.shape[1]):
        raise ValueError("%s: logits must have contiguous rows" % who)
    return C


def roi_mask_positives(labels, rois, src, matched, N, P, Rp):
    """The positive rows of the box head's sampled plan in one launch (reference mask_head.py:14-32 keep_only_positive_boxes and
    mask_head/loss.py:54-68, whose re-match gives the box plan's ``matched``): labels int32 [R], rois [R, 5], src int32 [R] of
    ops.roi_box_gather, matched int32 [N * P] of ops.roi_box_match, Rp the number of rows with label > 0 (known to the caller from
    the plan's per-image counts) -> pos_rows int32 [Rp], pos_rois [Rp, 5], pos_labels int32 [Rp], pos_gt int32 [Rp], in row order."""
    R = _roi_mask_rois("roi_mask_positives", rois)
    _roi_mask_vector("roi_mask_positives", labels, torch.int32, R, "labels")
    _roi_mask_vector("roi_mask_positives", src, torch.int32, R, "src")
    N, P, Rp = int(N), int(P), int(Rp)
    if N < 1 or P < 1 or N * P >= 2 ** 31:
        raise ValueError("roi_mask_positives: N %r, P %r: at least 1, N * P below 2^31" % (N, P))
    _roi_mask_vector("roi_mask_positives", matched, torch.int32, N * P, "matched")
    if not 0 <= Rp <= R:
        raise ValueError("roi_mask_positives: Rp %r outside 0..R = %d" % (Rp, R))
    _chk(labels, rois, src, matched)
    dev = rois.device
    pos_rows = torch.empty((Rp,), dtype=torch.int32, device=dev)
    pos_rois = torch.empty((Rp, 5), dtype=torch.float32, device=dev)
    pos_labels = torch.empty((Rp,), dtype=torch.int32, device=dev)
    pos_gt = torch.empty((Rp,), dtype=torch.int32, device=dev)
    call("scan_roi_mask_positives", _ptr(labels), _ptr(rois), _ptr(src), _ptr(matched), N, P, R, Rp, _ptr(pos_rows), _ptr(pos_rois),
         _ptr(pos_labels), _ptr(pos_gt), _stream())
    return pos_rows, pos_rois, pos_labels, pos_gt


def roi_mask_targets(pos_rois, pos_gt, masks, moff, mhw, M):
    """project_masks_on_boxes (reference mask_head/loss.py:11-42: BinaryMaskList.crop + resize((M, M)) + get_mask_tensor per
    positive proposal) in one launch: pos_rois [Rp, 5], pos_gt int32 [Rp], the batch's masks (uint8 flat, moff int64 [N + 1], mhw
    int32 [N, 2]) -> targets fp32 [Rp, M, M] of 0 / 1 by the integer rule of include/scan_hip.h."""
    Rp = _roi_mask_rois("roi_mask_targets", pos_rois)
    _roi_mask_vector("roi_mask_targets", pos_gt, torch.int32, Rp, "pos_gt")
    M = _roi_mask_size("roi_mask_targets", M)
    if masks.dtype != torch.uint8 or masks.dim() != 1 or not masks.is_contiguous():
        raise ValueError("roi_mask_targets: masks must be a flat contiguous uint8 buffer, got %r %s" % (tuple(masks.shape), masks.dtype))
    if mhw.dtype != torch.int32 or mhw.dim() != 2 or mhw.shape[0] < 1 or mhw.shape[1] != 2 or not mhw.is_contiguous():
        raise ValueError("roi_mask_targets: mhw must be contiguous int32 [N >= 1, 2] (height, width), got %r %s" % (tuple(mhw.shape), mhw.dtype))
    N = int(mhw.shape[0])
    _roi_mask_vector("roi_mask_targets", moff, torch.int64, N + 1, "moff")
    _chk(pos_rois, pos_gt, masks, moff, mhw)
    out = torch.empty((Rp, M, M), dtype=torch.float32, device=pos_rois.device)
    call("scan_roi_mask_targets", _ptr(pos_rois), _ptr(pos_gt), Rp, _ptr(masks), int(masks.numel()), _ptr(moff), _ptr(mhw), N, M,
         _ptr(out), _stream())
    return out


# scan_roi_mask_loss_forward is ONE workgroup (no float atomics, no cleared output, one launch): about 1.1 us per 1024 elements,
# a single CU's load rate -- 440 us at 401,408 elements against 25 us for the slots + ordered sum, and level with it (9.6 against
# 8.5 us) at 7,840 elements (profiles/r24_roi_mask.txt).  Up to 8 passes of the workgroup it saves the host one launch at no
# device time; past that the two-launch form is used whatever the mode.
ROI_MASK_LOSS_ONE_LAUNCH_ELEMS = 8192


class _RoiMaskLoss(torch.autograd.Function):
    """the mean over Rp M M elements of the binary cross-entropy of the label's column of the logits rows, read in place"""

    @staticmethod
    def forward(ctx, logits, dims, labels, targets):
        Rp, M, C = dims
        out = logits.new_empty((1,))
        args = (_ptr(logits), _pitch(logits), Rp, M, C, _ptr(labels), _ptr(targets))
        if Rp * M * M > ROI_MASK_LOSS_ONE_LAUNCH_ELEMS:
            call("scan_roi_mask_loss_forward_ordered", *args, _ptr(out),
                 _ptr(_partials("scan_roi_mask_loss_ordered_ws_floats", logits, Rp * M * M)), _stream())
        else:
            _call_reduction("scan_roi_mask_loss", "_forward", logits, (Rp * M * M,), *args, _ptr(out))
        ctx.save_for_backward(logits, labels, targets)
        ctx.args, ctx.count = args, Rp * M * M
        return out[0] / (Rp * M * M)

    @staticmethod
    def backward(ctx, g):
        logits = ctx.saved_tensors[0]
        gn = (g / ctx.count).reshape(1).contiguous()
        d = torch.empty(logits.shape, dtype=torch.float32, device=logits.device)
        call("scan_roi_mask_loss_backward", *ctx.args, _ptr(gn), _ptr(d), d.shape[1], _stream())
        return d, None, None, None


def roi_mask_loss(logits, labels, targets, C=None):
    """F.binary_cross_entropy_with_logits(mask_logits[pos, labels_pos], targets), mean reduction (reference mask_head/loss.py:
    124-127): logits the conv output rows [Rp M M, Cs] (C classes in the first columns; read in place), labels int32 [Rp],
    targets fp32 [Rp, M, M] -> a scalar.  Rp = 0: a zero that still reaches the logits (the reference's mask_logits.sum() * 0)."""
    if targets.dim() != 3 or targets.shape[1] != targets.shape[2] or targets.dtype != torch.float32 or not targets.is_contiguous():
        raise ValueError("roi_mask_loss: targets must be contiguous fp32 [Rp, M, M], got %r %s" % (tuple(targets.shape), targets.dtype))
    Rp = int(targets.shape[0])
    M = _roi_mask_size("roi_mask_loss", targets.shape[1])
    C = _roi_mask_logits("roi_mask_loss", logits, Rp, M, C)
    _roi_mask_vector("roi_mask_loss", labels, torch.int32, Rp, "labels")
    _chk(labels, targets)
    if Rp == 0:
        if not logits.is_cuda:
            raise RuntimeError("scan_amd ops run only on the GPU (HIP) -- got a %s tensor; no CPU fallback" % logits.device)
        return logits.sum() * 0
    return _RoiMaskLoss.apply(logits, (Rp, M, C), labels, targets)


def roi_mask_prob(logits, labels, M, C=None):
    """MaskPostProcessor.forward's sigmoid of the predicted class's channel (reference mask_head/inference.py:41-49) in one
    launch: logits rows [K M M, Cs], labels int32 / int64 [K] -> [K, 1, M, M]"""
    M = _roi_mask_size("roi_mask_prob", M)
    if labels.dim() != 1 or labels.dtype not in (torch.int32, torch.int64):
        raise ValueError("roi_mask_prob: labels must be int32 or int64 [K], got %r %s" % (tuple(labels.shape), labels.dtype))
    K = int(labels.shape[0])
    C = _roi_mask_logits("roi_mask_prob", logits, K, M, C)
    _chk(labels)
    labels = labels.to(torch.int32).contiguous()
    out = torch.empty((K, 1, M, M), dtype=torch.float32, device=logits.device)
    call("scan_roi_mask_prob", _ptr(logits), _pitch(logits), K, M, C, _ptr(labels), _ptr(out), _stream())
    return out


def roi_mask_paste(prob, boxes, image_hw, thresh=0.5):
    """Masker.forward_single_image with padding 1 (reference mask_head/inference.py:91-194) in one launch: prob [K, 1, M, M],
    boxes fp32 [K, 4] xyxy of ONE image of size image_hw = (H, W) -> uint8 [K, 1, H, W]; K = 0 gives an empty [0, 1, M, M] as
    the reference does.  thresh < 0 (the reference's mask * 255 debugging mode) is refused."""
    if not float(thresh) >= 0:
        raise ValueError("roi_mask_paste: thresh %r below 0 (the reference's mask * 255 debugging mode) is not built" % (thresh,))
    if prob.dim() != 4 or prob.shape[1] != 1 or prob.shape[2] != prob.shape[3] or prob.dtype != torch.float32 or not prob.is_contiguous():
        raise ValueError("roi_mask_paste: prob must be contiguous fp32 [K, 1, M, M], got %r %s" % (tuple(prob.shape), prob.dtype))
    K = int(prob.shape[0])
    M = _roi_mask_size("roi_mask_paste", prob.shape[2])
    if boxes.dtype != torch.float32 or tuple(boxes.shape) != (K, 4) or not boxes.is_contiguous():
        raise ValueError("roi_mask_paste: boxes must be contiguous fp32 [K, 4] = [%d, 4], got %r %s" % (K, tuple(boxes.shape), boxes.dtype))
    H, W = (int(v) for v in image_hw)
    if H < 1 or W < 1:
        raise ValueError("roi_mask_paste: image_hw %r: a positive height and width" % (image_hw,))
    _chk(prob, boxes)
    if K == 0:
        return prob.new_empty((0, 1, M, M))
    out = torch.empty((K, 1, H, W), dtype=torch.uint8, device=prob.device)
    call("scan_roi_mask_paste", _ptr(prob), _ptr(boxes), K, M, H, W, float(thresh), _ptr(out), _stream())
    return out


class _BceLogitsMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets):
        _chk(logits, targets)
        M = logits.numel()
        out = logits.new_zeros((2,))
        _call_reduction("scan_bce_logits", "_forward", logits, (M,), _ptr(logits), _ptr(targets), 0.0, None, 0, M, _ptr(out))
        ctx.save_for_backward(logits, targets)
        return out[0] / M

    @staticmethod
    def backward(ctx, g):
        logits, targets = ctx.saved_tensors
        M = logits.numel()
        gn = (g / M).reshape(1).contiguous()
        d = torch.empty_like(logits)
        call("scan_bce_logits_backward", _ptr(logits), _ptr(targets), 0.0, None, 0, M, _ptr(gn), _ptr(d), _stream())
        return d, None


def bce_with_logits_mean(logits, targets):
    return _BceLogitsMean.apply(logits.contiguous(), targets.contiguous())


class _BceLogitsConstMean(torch.autograd.Function):
    """mean_m w[m] * bce(logits[m], t) against ONE constant label t, w optional (None: 1) and without gradient: the domain loss of
    the EPM discriminators (reference fcos_head_discriminator.py:71-72; _CA.py:86-88 with w = the centre-aware map).  The divisor
    is M, not sum(w).  No label tensor is built: the kernels take the constant."""

    @staticmethod
    def forward(ctx, logits, target, weight):
        _chk(logits, weight)
        M = logits.numel()
        out = logits.new_zeros((2,))
        _call_reduction("scan_bce_logits", "_forward", logits, (M,), _ptr(logits), None, target, _ptr(weight), 1, M, _ptr(out))
        ctx.save_for_backward(logits, weight)
        ctx.target = target
        return out[0] / M

    @staticmethod
    def backward(ctx, g):
        logits, weight = ctx.saved_tensors
        M = logits.numel()
        gn = (g / M).reshape(1).contiguous()
        d = torch.empty_like(logits)
        call("scan_bce_logits_backward", _ptr(logits), None, ctx.target, _ptr(weight), 1, M, _ptr(gn), _ptr(d), _stream())
        return d, None, None


def bce_with_logits_const_mean(logits, target, weight=None):
    return _BceLogitsConstMean.apply(logits.contiguous(), float(target), None if weight is None else weight.detach().contiguous())


def _cka_forward_loss(logits, act, M, cf, target, out):
    """out [2 cf + 2]: the per-class sums, a ticket word, the loss (atomic form: last block; ordered form: second launch)"""
    _call_reduction("scan_cka_bce", "_forward_loss", logits, (M, cf), _ptr(logits), _ptr(act), M, cf, target, _ptr(out))


class _CkaBce(torch.autograd.Function):
    """sum_c [ sum_m act[m,c+1] bce(logit[m,c], t) / sum_m act[m,c+1] ] / Cf -- one launch forward (the last block to
    finish forms the scalar), one launch backward (the kernel forms the per-class coefficients from the gradient of the
    scalar and the forward's sums)."""

    @staticmethod
    def forward(ctx, logits, act, target, cf):
        _chk(logits, act)
        M = logits.shape[0]
        assert logits.shape[1] == cf and act.shape[1] == cf + 1
        out = _zeros_f32(2 * cf + 2, logits.device)
        if M > 0:
            _cka_forward_loss(logits, act, M, cf, target, out)
        ctx.save_for_backward(logits, act, out)
        ctx.cfg = (target, cf)
        return out[2 * cf + 1] if M > 0 else out[2 * cf + 1] / 0.0  # no rows: the reference's 0 / 0

    @staticmethod
    def backward(ctx, g):
        logits, act, out = ctx.saved_tensors
        target, cf = ctx.cfg
        d = torch.empty_like(logits)
        if logits.shape[0] > 0:
            call("scan_cka_bce_backward_loss", _ptr(logits), _ptr(act), logits.shape[0], cf, target,
                 _ptr(g.reshape(1).contiguous()), _ptr(out), _ptr(d), _stream())
        return d, None, None, None


class _CkaBcePair(torch.autograd.Function):
    """the two domain losses of one level in the paired step -- rows [0, m) against label 1 (source), rows [m, M) against label 0
    (target), each with its own act-map normaliser (_CkaBce on the two halves) -- with ONE gradient buffer: the two backward
    launches write their halves of d_logits directly (split_rows2 + two _CkaBce nodes: two buffers + two copies per level)."""

    @staticmethod
    def forward(ctx, logits, act, m, cf):
        _chk(logits, act)
        M = logits.shape[0]
        assert logits.shape[1] == cf and act.shape[1] == cf + 1 and 0 < m < M
        outs = []
        for lo, hi, target in ((0, m, 1.0), (m, M, 0.0)):
            out = _zeros_f32(2 * cf + 2, logits.device)
            _cka_forward_loss(logits[lo:hi], act[lo:hi], hi - lo, cf, target, out)
            outs.append(out)
        ctx.save_for_backward(logits, act, outs[0], outs[1])
        ctx.cfg = (m, cf)
        return outs[0][2 * cf + 1], outs[1][2 * cf + 1]

    @staticmethod
    def backward(ctx, gs, gt):
        logits, act, out_s, out_t = ctx.saved_tensors
        m, cf = ctx.cfg
        M = logits.shape[0]
        d = torch.empty_like(logits)
        for lo, hi, target, g, out in ((0, m, 1.0, gs, out_s), (m, M, 0.0, gt, out_t)):
            if g is None:
                d[lo:hi].zero_()
            else:
                call("scan_cka_bce_backward_loss", _ptr(logits[lo:hi]), _ptr(act[lo:hi]), hi - lo, cf, target,
                     _ptr(g.reshape(1).contiguous()), _ptr(out), _ptr(d[lo:hi]), _stream())
        return d, None, None, None


def cka_bce_pair(logits, act_detached, m, cf):
    return _CkaBcePair.apply(logits.contiguous(), act_detached.contiguous(), int(m), int(cf))


class _SplitRows2(torch.autograd.Function):
    """(x[:m], x[m:]) as views; the backward writes the two gradients into ONE buffer (torch's two slice backwards each
    zero-fill a full-size tensor, copy their part and are then added: 2 fills + 2 copies + 1 add per use)."""

    @staticmethod
    def forward(ctx, x, m):
        ctx.m = m
        ctx.shape = x.shape
        return x[:m], x[m:]

    @staticmethod
    def backward(ctx, g1, g2):
        m = ctx.m
        g = (g1 if g1 is not None else g2).new_empty(ctx.shape)
        if g1 is not None:
            g[:m] = g1
        else:
            g[:m].zero_()
        if g2 is not None:
            g[m:] = g2
        else:
            g[m:].zero_()
        return g, None


def split_rows2(x, m):
    return _SplitRows2.apply(x, m)


def cka_bce(logits, act_detached, target, cf):
    return _CkaBce.apply(logits.contiguous(), act_detached.contiguous(), float(target), int(cf))


class _SoftmaxFocalMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, gamma):
        _chk(logits, labels)
        if labels.dtype != torch.int64:
            raise RuntimeError("labels must be int64")
        M, K = logits.shape
        out = logits.new_zeros((1,))
        _call_reduction("scan_softmax_focal", "_forward", logits, (M,), _ptr(logits), _ptr(labels), M, K, gamma, _ptr(out))
        ctx.save_for_backward(logits, labels)
        ctx.gamma = gamma
        return out[0] / M

    @staticmethod
    def backward(ctx, g):
        logits, labels = ctx.saved_tensors
        M, K = logits.shape
        d = torch.empty_like(logits)
        # d_scale must be a host float: one small sync-free path would pass it by pointer; g is a 0-dim tensor
        call("scan_softmax_focal_backward", _ptr(logits), _ptr(labels), M, K, ctx.gamma, 1.0 / M, _ptr(d), _stream())
        return d * g, None, None


def softmax_focal_loss_mean(logits, labels, gamma=2.0):
    return _SoftmaxFocalMean.apply(logits.contiguous(), labels.contiguous(), float(gamma))


class _GradReverse(torch.autograd.Function):
    """reference discriminator/layer.py:6-24: forward x.clone(), backward -lambda * g.  The forward here is a view of
    x -- same values, and nothing downstream writes into it in place -- which saves a read + write of every feature
    and act map handed to the five discriminators (375 MB per iteration at the bench size).  Any dense layout is taken as
    it is (row matrices; channels_last NCHW tensors on the drop-in surface): the backward is element-wise on the storage."""

    @staticmethod
    def forward(ctx, x, lam):
        if not x.is_cuda:
            raise RuntimeError("scan_amd ops run only on the GPU (HIP) -- got a %s tensor; no CPU fallback" % x.device)
        ctx.lam = lam
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        if not (g.is_contiguous() or (g.dim() == 4 and g.is_contiguous(memory_format=torch.channels_last))):
            g = g.contiguous()
        d = torch.empty_like(g)  # preserve_format: the same dense strides as g
        call("scan_scale", _ptr(g), -ctx.lam, _ptr(d), g.numel(), _stream())
        return d, None


def grad_reverse(x, lam):
    return _GradReverse.apply(x, float(lam))


# ----------------------------------------------------------------------------- NMS
def _nms_impl(dets, scores, labels, thr, rule_ge):
    n = dets.shape[0]
    if n == 0:
        # reference csrc/nms.h:17-18: empty input -> empty CPU int64 tensor
        return torch.empty((0,), dtype=torch.int64, device="cpu")
    _chk(dets, scores, labels)
    if n > _lib.NMS_MAX:
        raise RuntimeError("nms: n=%d exceeds SCAN_NMS_MAX=%d" % (n, _lib.NMS_MAX))
    dets = dets.contiguous().float()
    scores = scores.contiguous().float()
    if labels is not None:
        labels = labels.contiguous().float()
    keep, cnt = _nms_launch(dets, scores, labels, thr, rule_ge)
    return keep[:int(cnt.item())]


def _nms_launch(dets, scores, labels, thr, rule_ge):
    """the launches of one NMS without the host read of the count: (keep buffer [n], count [1] int32)"""
    n = dets.shape[0]
    ws = torch.empty((query("scan_nms_ws_bytes", n) + 15) // 16 * 2, dtype=torch.float64, device=dets.device)
    keep = torch.empty((n,), dtype=torch.int64, device=dets.device)
    cnt = torch.empty((1,), dtype=torch.int32, device=dets.device)
    call("scan_nms", _ptr(dets), _ptr(scores), _ptr(labels), n, float(thr), int(rule_ge), _ptr(keep), _ptr(cnt),
         _ptr(ws), _stream())
    return keep, cnt


def nms_by_label_async(dets, scores, labels, thr):
    """ml_nms / per-class NMS launched on the current stream, nothing read back: returns finish() -> kept indices.  Lets a
    caller queue the NMS of several images (each a single-workgroup chain of kernels) on different streams before the
    first host read."""
    n = dets.shape[0]
    if n == 0:
        return lambda: torch.empty((0,), dtype=torch.int64, device="cpu")
    _chk(dets, scores, labels)
    if n > _lib.NMS_MAX:
        raise RuntimeError("nms: n=%d exceeds SCAN_NMS_MAX=%d" % (n, _lib.NMS_MAX))
    keep, cnt = _nms_launch(dets.contiguous().float(), scores.contiguous().float(), labels.contiguous().float(), thr, True)
    return lambda: keep[:int(cnt.item())]


def nms(dets, scores, thr, rule_ge=True):
    """kept original indices, ascending (reference csrc/cpu/nms_cpu.cpp:64, cuda/nms.cu:127-130)."""
    return _nms_impl(dets, scores, None, thr, rule_ge)


def nms_by_label(dets, scores, labels, thr):
    """greedy NMS per label in one launch, CPU '>=' rule (= boxlist_nms applied class by class,
    reference rpn/fcos/inference.py:160-176 + csrc/cpu/nms_cpu.cpp:60); kept original indices ascending."""
    return _nms_impl(dets, scores, labels.float(), thr, True)


def ml_nms(dets, scores, labels, thr):
    """label-aware NMS with the CUDA '>' rule (reference csrc/cuda/ml_nms.cu:13-24,62)."""
    return _nms_impl(dets, scores, labels, thr, False)


# ----------------------------------------------------------------------------- density clustering (target nodes)
def dbscan_in_cluster0(pts, eps, min_samples=5):
    """bool [n]: True where sklearn.cluster.DBSCAN(eps, min_samples).fit_predict(pts) would return label 0 -- all the
    target-node sampling needs (reference rpn/fcos/loss.py:397-423: noise -> 1, cluster 0 -> 0, selected = non-zero).
    Neighbour search, core test, breadth-first growth of cluster 0 and border assignment run on the device
    (scan_dbscan_*); the host only reads one flag per breadth-first level.
    eps is rounded to fp32 before it is squared (the C entry point takes a float): the threshold is fp32(eps)^2, where sklearn
    -- and condgraph's "host" backend -- squares the Python double.  The two differ only for a pair whose distance lies between eps and
    fp32(eps): within 6e-8 relative (half an fp32 ulp) of an eps that fp32 does not represent."""
    _chk(pts)
    n, d = pts.shape
    if n == 0:
        return torch.zeros((0,), dtype=torch.bool, device=pts.device)
    nbytes = query("scan_dbscan_ws_bytes", n)
    if nbytes < 0:
        raise RuntimeError("dbscan: n=%d exceeds SCAN_DBSCAN_MAX" % n)
    ws = torch.empty((nbytes // 8 + 1,), dtype=torch.float64, device=pts.device)
    info = torch.empty((2,), dtype=torch.int32, device=pts.device)
    st = _stream()
    call("scan_dbscan_prepare", _ptr(pts), n, d, float(eps), int(min_samples), _ptr(ws), _ptr(info), st)
    if int(info[0].item()) >= n:  # no core point: everything is noise
        return torch.zeros((n,), dtype=torch.bool, device=pts.device)
    changed = torch.zeros((1,), dtype=torch.int32, device=pts.device)
    parity = 0
    while True:
        call("scan_dbscan_bfs_step", n, _ptr(ws), parity, _ptr(changed), st)
        if int(changed.item()) == 0:
            break
        parity ^= 1
    out = torch.empty((n,), dtype=torch.uint8, device=pts.device)
    call("scan_dbscan_finish", n, _ptr(ws), _ptr(out), st)
    return out.bool()


# ----------------------------------------------------------------------------- CKA discriminator class branches
class _CkaStackedWeights(torch.autograd.Function):
    """The Cf per-class classifier branches (conv3x3 C+1 -> H, conv3x3 H -> 1; reference
    discriminator/fcos_head_discriminator_con.py:44-62) as the weights of two stacked convolutions -- one launch
    forward (scan_cka_stack_weights), one launch backward (scan_cka_unstack_grads, straight into the parameters' flat
    gradient buffers when they have them) instead of the ~40 stack / slice / mul / cat kernels and their autograd
    mirror images per discriminator."""

    @staticmethod
    def forward(ctx, C, H, cs1, *params):
        cf = len(params) // 4
        w0s, b0s, w2s, b2s = params[0::4], params[1::4], params[2::4], params[3::4]
        for t in params:  # strided (channels-last) weights are fine here: the kernel takes element strides
            if not t.is_cuda or t.dtype != torch.float32:
                raise RuntimeError("scan_amd ops run only on fp32 GPU (HIP) tensors -- got %s %s; no CPU fallback"
                                   % (t.device, t.dtype))
        w0, w2 = w0s[0], w2s[0]
        assert tuple(w0.shape) == (H, C + 1, 3, 3) and tuple(w2.shape) == (1, H, 3, 3), (w0.shape, w2.shape)
        for a, b in zip(w0s, w2s):
            if a.stride() != w0.stride() or b.stride() != w2.stride() or a.shape != w0.shape or b.shape != w2.shape:
                raise RuntimeError("cka_stacked_weights: the class branches must share one memory layout")
        if w0.stride(2) != 3 * w0.stride(3) or w2.stride(2) != 3 * w2.stride(3):
            raise RuntimeError("cka_stacked_weights: the 3x3 taps of a weight must be evenly strided")
        strides = (w0.stride(0), w0.stride(1), w0.stride(3), w2.stride(1), w2.stride(3))
        cs2 = cf * H
        dev = w0.device
        w1 = torch.empty((cf * H, 9, cs1), device=dev)
        b1 = torch.empty((cf * H,), device=dev)
        w2o = torch.empty((cf, 9, cs2), device=dev)
        b2 = torch.empty((cf,), device=dev)
        arr = (_lib.CkaBranch * cf)()
        for a, p0, q0, p2, q2 in zip(arr, w0s, b0s, w2s, b2s):
            a.w0, a.b0, a.w2, a.b2 = p0.data_ptr(), q0.data_ptr(), p2.data_ptr(), q2.data_ptr()
        call("scan_cka_stack_weights", arr, cf, C, H, *strides, cs1, cs2, _ptr(w1), _ptr(b1), _ptr(w2o), _ptr(b2),
             _stream())
        ctx.cfg = (cf, C, H, cs1, cs2, strides)
        ctx.params = params  # parameters (leaf tensors), needed for their .grad buffers; not graph intermediates
        # logical conv weights [O, Cin, 3, 3] stored channels-last: conv2d reads them in place
        return (w1.view(cf * H, 3, 3, cs1).permute(0, 3, 1, 2), b1, w2o.view(cf, 3, 3, cs2).permute(0, 3, 1, 2), b2)

    @staticmethod
    def backward(ctx, dw1, db1, dw2, db2):
        cf, C, H, cs1, cs2, strides = ctx.cfg
        params = ctx.params

        def ohwi(g):
            return None if g is None else g.permute(0, 2, 3, 1).contiguous()

        dw1, dw2 = ohwi(dw1), ohwi(dw2)
        db1 = None if db1 is None else db1.contiguous()
        db2 = None if db2 is None else db2.contiguous()
        direct = all(getattr(p, "_scan_flat", False) and p.grad is not None and p.grad.stride() == p.stride()
                     for p in params)
        tgt = [p.grad for p in params] if direct else [torch.zeros_like(p) for p in params]
        arr = (_lib.CkaBranch * cf)()
        for c, a in enumerate(arr):
            a.w0, a.b0, a.w2, a.b2 = (t.data_ptr() for t in tgt[4 * c:4 * c + 4])
        call("scan_cka_unstack_grads", arr, cf, C, H, *strides, cs1, cs2, _ptr(dw1), _ptr(db1), _ptr(dw2), _ptr(db2),
             1, _stream())
        return (None, None, None) + (tuple(None for _ in params) if direct else tuple(tgt))


CKA_STACK_MAX = _lib.CKA_MAX_CLASSES  # branches scan_cka_stack_weights / scan_cka_unstack_grads take in one launch


def cka_stacked_weights(branches, C, H, cs1):
    """branches: the Cf (conv0, conv2) module pairs.  Returns (w1 [Cf*H, cs1, 3, 3], b1, w2 [Cf, Cf*H, 3, 3], b2) with
    cs1 = the (padded) channel count of cat(x, act[1:])."""
    params = []
    for c0, c2 in branches:
        params += [c0.weight, c0.bias, c2.weight, c2.bias]
    return _CkaStackedWeights.apply(int(C), int(H), int(cs1), *params)


GCONV_BITS, GCONV_ACT = 4, 8  # SCAN_GCONV_BITS / _ACT of scan_gconv3x3_to1_caps: what the library runs for a G right now


class _GroupedConvTo1(torch.autograd.Function):
    """conv3x3 [M, G*128] -> [M, Ns >= G], one output channel per group of 128 (the class branches' second conv);
    w = the stacked weight [G, G*128, 3, 3] (channels-last) whose diagonal blocks are the per-class weights.
    mask_dx: x is a deferred-ReLU output (see _Conv2d) -- the forward then also leaves (x > 0) as a bit mask (1/32 of x)
    so that the backward does not read x a second time for it."""

    @staticmethod
    def forward(ctx, x, w, bias, shape, G, mask_dx):
        _chk(x, bias)
        gc = G * 128
        assert x.shape == (shape.rows, gc) and tuple(w.shape) == (G, gc, 3, 3) and w.permute(0, 2, 3, 1).is_contiguous()
        ns = pad4(G)
        y = x.new_empty((shape.rows, ns))
        ws = x.new_empty((query("scan_gconv3x3_to1_ws_floats", shape.ref(), G, 128),))
        bits = None
        # the bit mask serves the matrix-core kernels: only where the library would run those
        if query("scan_gconv3x3_to1_caps", G, 128) & GCONV_BITS and mask_dx and torch.is_grad_enabled() and x.requires_grad:
            bits = torch.empty((shape.rows * G * 4,), dtype=torch.int32, device=x.device)
            call("scan_gconv3x3_to1_forward_bits", _ptr(x), shape.ref(), G, 128, _ptr(w), _ptr(bias), _ptr(y), ns,
                 _ptr(ws), _ptr(bits), _stream())
        else:
            call("scan_gconv3x3_to1_any_forward", _ptr(x), shape.ref(), G, 128, _ptr(w), _ptr(bias), _ptr(y), ns, _ptr(ws),
                 _stream())
        ctx.save_for_backward(x, w, bits)
        ctx.cfg = (shape, G, ns, mask_dx, bias is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, bits = ctx.saved_tensors
        shape, G, ns, mask_dx, has_bias = ctx.cfg
        dy = dy.contiguous()
        st = _stream()
        dx = dw = db = dwp = None
        if ctx.needs_input_grad[1]:
            dwp = x.new_zeros((G, 9, G * 128))  # off-diagonal blocks: exact zeros (they meet a zero in the adjoint)
            ws = x.new_empty((query("scan_gconv3x3_to1_ws_floats", shape.ref(), G, 128),))
            dw = dwp.view(G, 3, 3, G * 128).permute(0, 3, 1, 2)
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
        if dx is not None and dwp is not None and bits is not None:
            call("scan_gconv3x3_to1_backward_bits", _ptr(x), _ptr(dy), ns, shape.ref(), G, 128, _ptr(w), _ptr(bits),
                 _ptr(dx), _ptr(dwp), 0, _ptr(ws), st)
        elif dx is not None and dwp is not None:
            call("scan_gconv3x3_to1_any_backward", _ptr(x), _ptr(dy), ns, shape.ref(), G, 128, _ptr(w), int(mask_dx), _ptr(dx),
                 _ptr(dwp), 0, _ptr(ws), st)
        elif dx is not None:
            call("scan_gconv3x3_to1_any_dgrad", _ptr(dy), ns, shape.ref(), G, 128, _ptr(w), _ptr(x if mask_dx else None),
                 _ptr(dx), st)
        elif dwp is not None:
            call("scan_gconv3x3_to1_any_wgrad", _ptr(x), _ptr(dy), ns, shape.ref(), G, 128, _ptr(dwp), 0, _ptr(ws), st)
        if has_bias and ctx.needs_input_grad[2]:
            M = dy.shape[0]
            cws = x.new_empty((query("scan_colsum_ws_floats", M, G),))
            db = x.new_empty((G,))
            call("scan_colsum", _ptr(dy), M, G, ns, _ptr(db), 0, _ptr(cws), st)
        return dx, dw, db, None, None, None


# SCAN_GROUPED_CLS=0: the class branches' second conv on the dense MFMA kernel (block-diagonal weight), for A/B
GROUPED_CLS = os.environ.get("SCAN_GROUPED_CLS", "1") != "0"


def gconv_max_groups():
    """largest group count of gconv3x3_to1 (G = 1, 2, 4, 8 have kernels of their own, every other G the generic ones)"""
    return _limit("scan_gconv3x3_to1_max_groups")


def gconv3x3_to1(x, w, bias, shape, G, mask_dx=False):
    """x [M, G*128] -> [M, pad4(G)]: y[:, g] = conv3x3(x[:, g*128:(g+1)*128], w[g, g*128:(g+1)*128]) + bias[g]."""
    return _GroupedConvTo1.apply(x, w, bias, shape, int(G), bool(mask_dx))


# SCAN_CLS_SPLIT=0: the class branches' first conv as one dense conv over cat(x, act[1:]) with a block-diagonal act weight
# (264 input channels for 8 classes), for A/B.  On (default): the dense conv runs on the 256 feature channels alone and
# the per-class act-map channel -- nine multiply-adds per hidden element -- is formed in registers by the grouped conv
# that reads the hidden map (gconv3x3_to1_act, csrc/gconv.hip).  Same values up to the summation order.
CLS_SPLIT = os.environ.get("SCAN_CLS_SPLIT", "1") != "0"


# SCAN_CLS_SPLIT_FUSED=0: the act term's gradients (d act, dE) in a pass of their own over dh (scan_gconv3x3_to1_act_grads)
# instead of inside the kernel that produces dh, for A/B.  Same sums in the same per-workgroup slab order.
CLS_SPLIT_FUSED = os.environ.get("SCAN_CLS_SPLIT_FUSED", "1") != "0"


def cls_split_supported(G):
    """the act-term kernels exist for the lane-mapped class counts on the fp32 FMA gconv path"""
    return bool(query("scan_gconv3x3_to1_caps", int(G), 128) & GCONV_ACT)


class _CkaStackedWeightsSplit(torch.autograd.Function):
    """_CkaStackedWeights for the split class branches: (wmain [Cf*H, C, 3, 3] channels-last, e [Cf, 9, H], b1, w2, b2) in one
    launch; the backward scatters dwmain and de into the per-class conv0.weight gradients in one launch (straight into the
    flat gradient buffers when the parameters have them)."""

    @staticmethod
    def forward(ctx, C, H, *params):
        cf = len(params) // 4
        w0s, b0s, w2s, b2s = params[0::4], params[1::4], params[2::4], params[3::4]
        for t in params:
            if not t.is_cuda or t.dtype != torch.float32:
                raise RuntimeError("scan_amd ops run only on fp32 GPU (HIP) tensors -- got %s %s; no CPU fallback"
                                   % (t.device, t.dtype))
        w0, w2 = w0s[0], w2s[0]
        assert tuple(w0.shape) == (H, C + 1, 3, 3) and tuple(w2.shape) == (1, H, 3, 3), (w0.shape, w2.shape)
        for a, b in zip(w0s, w2s):
            if a.stride() != w0.stride() or b.stride() != w2.stride() or a.shape != w0.shape or b.shape != w2.shape:
                raise RuntimeError("cka_stacked_weights_split: the class branches must share one memory layout")
        if w0.stride(2) != 3 * w0.stride(3) or w2.stride(2) != 3 * w2.stride(3):
            raise RuntimeError("cka_stacked_weights_split: the 3x3 taps of a weight must be evenly strided")
        strides = (w0.stride(0), w0.stride(1), w0.stride(3), w2.stride(1), w2.stride(3))
        cs2 = cf * H
        dev = w0.device
        wm = torch.empty((cf * H, 9, C), device=dev)
        e = torch.empty((cf, 9, H), device=dev)
        b1 = torch.empty((cf * H,), device=dev)
        w2o = torch.empty((cf, 9, cs2), device=dev)
        b2 = torch.empty((cf,), device=dev)
        arr = (_lib.CkaBranch * cf)()
        for a, p0, q0, p2, q2 in zip(arr, w0s, b0s, w2s, b2s):
            a.w0, a.b0, a.w2, a.b2 = p0.data_ptr(), q0.data_ptr(), p2.data_ptr(), q2.data_ptr()
        call("scan_cka_stack_weights_split", arr, cf, C, H, *strides, cs2, _ptr(wm), _ptr(e), _ptr(b1), _ptr(w2o), _ptr(b2),
             _stream())
        ctx.cfg = (cf, C, H, cs2, strides)
        ctx.params = params  # parameters (leaf tensors), needed for their .grad buffers; not graph intermediates
        return (wm.view(cf * H, 3, 3, C).permute(0, 3, 1, 2), e, b1, w2o.view(cf, 3, 3, cs2).permute(0, 3, 1, 2), b2)

    @staticmethod
    def backward(ctx, dwm, de, db1, dw2, db2):
        cf, C, H, cs2, strides = ctx.cfg
        params = ctx.params

        def ohwi(g):
            return None if g is None else g.permute(0, 2, 3, 1).contiguous()

        dwm, dw2 = ohwi(dwm), ohwi(dw2)
        de, db1, db2 = (None if g is None else g.contiguous() for g in (de, db1, db2))
        direct = all(getattr(p, "_scan_flat", False) and p.grad is not None and p.grad.stride() == p.stride()
                     for p in params)
        tgt = [p.grad for p in params] if direct else [torch.zeros_like(p) for p in params]
        arr = (_lib.CkaBranch * cf)()
        for c, a in enumerate(arr):
            a.w0, a.b0, a.w2, a.b2 = (t.data_ptr() for t in tgt[4 * c:4 * c + 4])
        call("scan_cka_unstack_grads_split", arr, cf, C, H, *strides, cs2, _ptr(dwm), _ptr(de), _ptr(db1), _ptr(dw2),
             _ptr(db2), 1, _stream())
        return (None, None) + (tuple(None for _ in params) if direct else tuple(tgt))


def cka_stacked_weights_split(branches, C, H):
    """branches: the Cf (conv0, conv2) module pairs.  Returns (wmain [Cf*H, C, 3, 3], e [Cf, 9, H], b1, w2 [Cf, Cf*H, 3, 3],
    b2): conv0.weight[:, :C] of the classes stacked, conv0.weight[:, C] as e[c][ky * 3 + kx][o], and the second conv as in
    cka_stacked_weights."""
    params = []
    for c0, c2 in branches:
        params += [c0.weight, c0.bias, c2.weight, c2.bias]
    return _CkaStackedWeightsSplit.apply(int(C), int(H), *params)


class _GroupedConvTo1Act(torch.autograd.Function):
    """_GroupedConvTo1 on relu(h + hact) with the class branches' act term hact formed inside the kernels: h [M, G*128] is
    the first conv on the feature channels, stored before its ReLU; act [M, K] holds class g in column col0 + g; e [G, 9, 128]
    is each class's act-column weight.  One node: the backward returns dh (the gradient of h, already masked by the ReLU),
    dw, db, d act and de."""

    @staticmethod
    def forward(ctx, h, w, bias, act, e, shape, G, col0):
        _chk(h, bias, act, e)
        gc = G * 128
        assert h.shape == (shape.rows, gc) and tuple(w.shape) == (G, gc, 3, 3) and w.permute(0, 2, 3, 1).is_contiguous()
        assert act.shape[0] == shape.rows and act.shape[1] >= col0 + G and act.is_contiguous(), (act.shape, col0, G)
        assert tuple(e.shape) == (G, 9, 128) and e.is_contiguous() and h.is_contiguous()
        if not cls_split_supported(G):
            raise RuntimeError("gconv3x3_to1_act: G=%d on the fp32 FMA kernels only (G in 1, 2, 4, 8; gconv_mfma = 0)" % G)
        ns = pad4(G)
        y = h.new_empty((shape.rows, ns))
        ws = h.new_empty((query("scan_gconv3x3_to1_act_ws_floats", shape.ref(), G, 128),))
        call("scan_gconv3x3_to1_act_forward", _ptr(h), shape.ref(), G, 128, _ptr(w), _ptr(bias), _ptr(act), act.shape[1], col0,
             _ptr(e), _ptr(y), ns, _ptr(ws), _stream())
        ctx.save_for_backward(h, w, act, e)
        ctx.cfg = (shape, G, ns, col0, bias is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        h, w, act, e = ctx.saved_tensors
        shape, G, ns, col0, has_bias = ctx.cfg
        dy = dy.contiguous()
        st = _stream()
        K = act.shape[1]
        ws = h.new_empty((query("scan_gconv3x3_to1_act_ws_floats", shape.ref(), G, 128),))
        dwp = h.new_zeros((G, 9, G * 128))  # off-diagonal blocks: exact zeros (they meet a zero in the adjoint)
        dh = torch.empty_like(h)
        want_act = ctx.needs_input_grad[3] or ctx.needs_input_grad[4]
        fused = CLS_SPLIT_FUSED and want_act
        if fused:  # d act and de from dh while it is in registers: no second pass over dh
            dact, de = torch.empty_like(act), torch.empty_like(e)
            call("scan_gconv3x3_to1_act_backward_all", _ptr(h), _ptr(dy), ns, shape.ref(), G, 128, _ptr(w), _ptr(act), K, col0,
                 _ptr(e), _ptr(dh), _ptr(dwp), _ptr(dact), K, col0, _ptr(de), 0, _ptr(ws), st)
        else:
            call("scan_gconv3x3_to1_act_backward", _ptr(h), _ptr(dy), ns, shape.ref(), G, 128, _ptr(w), _ptr(act), K, col0,
                 _ptr(e), _ptr(dh), _ptr(dwp), 0, _ptr(ws), st)
        dw = dwp.view(G, 3, 3, G * 128).permute(0, 3, 1, 2) if ctx.needs_input_grad[1] else None
        db = None
        if not fused:
            dact = de = None
        if has_bias and ctx.needs_input_grad[2]:
            M = dy.shape[0]
            cws = h.new_empty((query("scan_colsum_ws_floats", M, G),))
            db = h.new_empty((G,))
            call("scan_colsum", _ptr(dy), M, G, ns, _ptr(db), 0, _ptr(cws), st)
        if want_act and not fused:
            dact = torch.empty_like(act)
            de = torch.empty_like(e)
            call("scan_gconv3x3_to1_act_grads", _ptr(dh), shape.ref(), G, 128, _ptr(act), K, col0, _ptr(e), _ptr(dact), K, col0,
                 _ptr(de), 0, _ptr(ws), st)
        dact = dact if ctx.needs_input_grad[3] else None
        de = de if ctx.needs_input_grad[4] else None
        return (dh if ctx.needs_input_grad[0] else None), dw, db, dact, de, None, None, None


def gconv3x3_to1_act(h, w, bias, act, e, shape, G, col0=1):
    """y[:, g] = conv3x3(relu(h + hact)[:, g*128:(g+1)*128], w[g, g*128:(g+1)*128]) + bias[g] -> [M, pad4(G)], with
    hact[p, g*128 + i] = sum_t e[g, t, i] * act[nb(p, t), col0 + g] (zero outside the image)."""
    return _GroupedConvTo1Act.apply(h, w, bias, act.contiguous(), e, shape, int(G), int(col0))


# ----------------------------------------------------------------------------- optimizer
# SCAN_COND_RNN=0: the conditioned-kernel generator (paradigm -> 2-layer tanh RNN -> (T, 1) conv) runs as the torch loop it is
# written as in modeling/condgraph.py (T x 2 x (2 linear + add + tanh), ~120 launches with its backward) instead of the
# 15 launches of csrc/condrnn.hip (one per link of the chain, spread over 8-32 workgroups), for A/B.  Same values up to the summation order.
COND_RNN_FUSED = os.environ.get("SCAN_COND_RNN", "1") != "0"


class _CondRnn(torch.autograd.Function):
    """proto [K, 256, T] (a buffer: no gradient), the ten parameters in scan_cond_rnn_forward's order -> kernels [K, 256]"""

    @staticmethod
    def forward(ctx, proto, *params):
        if not (proto.is_cuda and all(p.is_cuda and p.dtype == torch.float32 for p in params)):
            raise RuntimeError("scan_amd ops run only on the GPU (HIP); no CPU fallback")
        K, C, T = proto.shape
        proto = proto.permute(2, 0, 1).contiguous()  # [T, K, 256]: the RNN's sequence-first input
        ws_ = [p.detach().contiguous() for p in params]
        h0 = proto.new_empty((T, K, 512))
        h1 = torch.empty_like(h0)
        ker = proto.new_empty((K, 256))
        wptr = (ctypes.c_void_p * 10)(*[w.data_ptr() for w in ws_])
        call("scan_cond_rnn_forward", _ptr(proto), K, T, wptr, _ptr(h0), _ptr(h1), _ptr(ker), _stream())
        ctx.save_for_backward(proto, h0, h1, *ws_)
        return ker

    @staticmethod
    def backward(ctx, dker):
        proto, h0, h1, *ws_ = ctx.saved_tensors
        T, K, C = proto.shape
        dker = dker.contiguous()
        grads = [torch.empty_like(w) for w in ws_]
        wptr = (ctypes.c_void_p * 10)(*[w.data_ptr() for w in ws_])
        gptr = (ctypes.c_void_p * 10)(*[g.data_ptr() for g in grads])
        ws = proto.new_empty((query("scan_cond_rnn_ws_floats"),))
        call("scan_cond_rnn_backward", _ptr(proto), K, T, wptr, _ptr(h0), _ptr(h1), _ptr(dker), gptr, _ptr(ws), _stream())
        return (None, *grads)


def cond_rnn_supported(proto, params):
    K, C, T = proto.shape
    return (COND_RNN_FUSED and proto.is_cuda and K <= 9 and T <= 3 and C == 256 and tuple(params[0].shape) == (512, 256)
            and tuple(params[8].shape[:3]) == (256, 512, T))


def cond_rnn(proto, params):
    """reference condgraph.py:313-319 get_conded_weight as one launch (two in the backward); params: weight_ih_l0,
    weight_hh_l0, bias_ih_l0, bias_hh_l0, weight_ih_l1, weight_hh_l1, bias_ih_l1, bias_hh_l1, cond_nx1.weight, cond_nx1.bias"""
    return _CondRnn.apply(proto, *params)


def sgd_momentum_multi_(segments, momentum):
    """segments: list of (p, g, buf, lr, wd, first_step) flat fp32 tensors of equal length -- all updated by ONE launch
    (scan_sgd_momentum_multi), element arithmetic as sgd_momentum_."""
    segments = [sg for sg in segments if sg[0].numel() > 0]
    for k in range(0, len(segments), _lib.SGD_MAX_SEGMENTS):
        part = segments[k:k + _lib.SGD_MAX_SEGMENTS]
        arr = (_lib.SgdSegment * len(part))()
        for a, (p, g, buf, lr, wd, first) in zip(arr, part):
            _chk(p, g, buf)
            assert p.numel() == g.numel() == buf.numel()
            a.p, a.g, a.buf, a.n = p.data_ptr(), g.data_ptr(), buf.data_ptr(), p.numel()
            a.lr, a.wd, a.first_step, a.reserved = float(lr), float(wd), int(bool(first)), 0
        call("scan_sgd_momentum_multi", arr, len(part), float(momentum), _stream())


def sgd_momentum_(p, g, buf, lr, wd, momentum, first_step):
    _chk(p, g, buf)
    call("scan_sgd_momentum", _ptr(p), _ptr(g), _ptr(buf), p.numel(), float(lr), float(wd), float(momentum),
         int(first_step), _stream())

"""Drop-in for the reference's pybind module ``fcos_core._C``
(reference fcos_core/csrc/vision.cpp:8-17): same names, argument meaning and
error behaviour, backed by libscan_hip.so through the C ABI.

    nms(dets[n,4], scores[n], thr[, cuda_rule]) -> int64[k]     (CPU tensors: the host loop of nms_host below)
    ml_nms(dets[n,4], scores[n], labels[n] float, thr) -> int64[k]
    sigmoid_focalloss_forward(logits[M,C], targets[M] int32, num_classes, gamma, alpha) -> losses[M,C]
    sigmoid_focalloss_backward(logits, targets, d_losses, num_classes, gamma, alpha) -> d_logits[M,C]

    roi_align_forward(input[N,C,H,W], rois[K,5], scale, PH, PW, sampling_ratio) -> [K,C,PH,PW]  (CPU tensors: roi_align_host)
    roi_align_backward(grad[K,C,PH,PW], rois, scale, PH, PW, N, C, H, W, sampling_ratio) -> [N,C,H,W]
    roi_pool_forward(input, rois, scale, PH, PW) -> (output[K,C,PH,PW], argmax int32 [K,C,PH,PW])
    roi_pool_backward(grad, input, rois, argmax, scale, PH, PW, N, C, H, W) -> [N,C,H,W]

All eight functions of vision.cpp; the pooling ones run csrc/roi.hip.
"""
import ctypes

import torch

from . import ops
from ._lib import call
from .ops import _ptr, _stream


def _require_gpu(t, who):
    if not t.is_cuda:
        # the reference raises "Not implemented on the CPU" (csrc/SigmoidFocalLoss.h:23, csrc/ml_nms.h:26)
        raise RuntimeError("%s: not implemented on the CPU" % who)


def nms_host(dets, scores, threshold, rule_ge=True):
    """The reference's CPU dispatch (csrc/nms.h:26, csrc/cpu/nms_cpu.cpp:5-65) for host tensors: candidates by
    descending score (ties: lower index first), a kept box suppresses every later box whose IoU -- areas with the +1
    pixel rule, in the tensors' own dtype -- reaches the threshold; kept ORIGINAL indices ascending.  One vectorised
    row of IoUs per kept box (same operations in the same order as the scalar loop, so the same keep list)."""
    if scores.is_cuda:
        raise RuntimeError("scores must be a CPU tensor")           # nms_cpu.cpp:10
    if dets.dtype != scores.dtype:
        raise RuntimeError("dets should have the same type as scores")  # nms_cpu.cpp:11
    if dets.dtype not in (torch.float32, torch.float64):
        raise RuntimeError("nms: float or double boxes")
    n = dets.shape[0]
    by_score = torch.sort(scores, descending=True, stable=True).indices
    b = dets[by_score].contiguous()
    area = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    dead = torch.zeros(n, dtype=torch.bool)
    zero = torch.zeros((), dtype=dets.dtype)
    thr = float(torch.tensor(threshold, dtype=torch.float32))  # the reference's `const float threshold`
    for r in range(n):
        if dead[r]:
            continue
        rest = b[r + 1:]
        w = torch.maximum(zero, torch.minimum(b[r, 2], rest[:, 2]) - torch.maximum(b[r, 0], rest[:, 0]) + 1)
        h = torch.maximum(zero, torch.minimum(b[r, 3], rest[:, 3]) - torch.maximum(b[r, 1], rest[:, 1]) + 1)
        inter = w * h
        iou = inter / (area[r] + area[r + 1:] - inter)
        dead[r + 1:] |= (iou >= thr) if rule_ge else (iou > thr)
    return torch.sort(by_score[~dead]).values


def _cuda_rule_env():
    import os
    return os.environ.get("SCAN_NMS_RULE", "") in ("gt", "cuda")


def nms(dets, scores, threshold, cuda_rule=False):
    """Greedy NMS.  Default: IoU >= threshold suppresses (the reference CPU rule, csrc/cpu/nms_cpu.cpp:60, which its
    tests/test_nms.py pins); ``cuda_rule=True`` or SCAN_NMS_RULE=gt: IoU > threshold (csrc/cuda/nms.cu:60).  GPU tensors
    run on libscan_hip.so, CPU tensors on ``nms_host`` (csrc/nms.h:10-30 dispatches the same way).  Empty input returns
    an empty CPU tensor (csrc/nms.h:17-18)."""
    if dets.numel() == 0:
        return torch.empty((0,), dtype=torch.int64, device="cpu")
    rule_ge = not (cuda_rule or _cuda_rule_env())
    if not dets.is_cuda:
        return nms_host(dets, scores, threshold, rule_ge)
    return ops.nms(dets, scores, threshold, rule_ge=rule_ge)


def ml_nms(dets, scores, labels, threshold):
    if dets.numel() == 0:
        return torch.empty((0,), dtype=torch.int64, device="cpu")
    _require_gpu(dets, "ml_nms")
    return ops.ml_nms(dets, scores, labels, threshold)


def sigmoid_focalloss_forward(logits, targets, num_classes, gamma, alpha):
    _require_gpu(logits, "sigmoid_focalloss_forward")
    if logits.dim() != 2:
        raise RuntimeError("logits should be NxClass")  # SigmoidFocalLoss_cuda.cu:112
    if logits.shape[1] != num_classes:
        raise RuntimeError("logits.size(1) should be num_classes")
    logits = logits.contiguous()
    targets = targets.contiguous()
    losses = torch.empty_like(logits)
    call("scan_sigmoid_focal_loss_forward", _ptr(logits), _ptr(targets), logits.shape[0], num_classes, float(gamma),
         float(alpha), _ptr(losses), None, _stream())
    return losses


def sigmoid_focalloss_backward(logits, targets, d_losses, num_classes, gamma, alpha):
    _require_gpu(logits, "sigmoid_focalloss_backward")
    if logits.dim() != 2 or logits.shape[1] != num_classes:
        raise RuntimeError("logits.size(1) should be num_classes")  # SigmoidFocalLoss_cuda.cu:158
    logits = logits.contiguous()
    targets = targets.contiguous()
    d_losses = d_losses.contiguous()
    d_logits = torch.empty_like(logits)
    call("scan_sigmoid_focal_loss_backward", _ptr(logits), _ptr(targets), _ptr(d_losses), 1.0, logits.shape[0],
         num_classes, float(gamma), float(alpha), _ptr(d_logits), _stream())
    return d_logits


# ----------------------------------------------------------------------------- region pooling
# The four functions take the reference's positional arguments (csrc/ROIAlign.h:11-45, csrc/ROIPool.h:10-47) through *args: a
# wrong count raises RuntimeError naming them, as every other failure of this module does (a plain signature would raise
# TypeError).  NCHW is converted to the kernels' row matrix here (a view for channels_last inputs with C % 4 == 0, one
# permuting copy otherwise) and the channel-last result back to contiguous NCHW; INTEGRATION.md prices both.
def _take(who, names, args, kwargs):
    if kwargs or len(args) != len(names):
        raise RuntimeError("%s(%s): expected %d positional arguments, got %d%s"
                           % (who, ", ".join(names), len(names), len(args), " and keyword arguments" if kwargs else ""))
    return args


def _rows_in(t, who):
    """NCHW fp32 -> (rows [N*H*W, Cs], PyramidShape, C)"""
    if t.dim() != 4:
        raise RuntimeError("%s: input must be [N, C, H, W]" % who)
    rows, shape = ops.nchw_to_rows(t.float())
    return rows, shape, t.shape[1]


def _pooled_in(t, c, fill, who):
    """[K, C, PH, PW] -> channel-last [K, PH, PW, Cs], padding columns = fill"""
    if t.dim() != 4 or t.shape[1] != c:
        raise RuntimeError("%s: expected a [K, %d, PH, PW] tensor, got %s" % (who, c, tuple(t.shape)))
    t = t.permute(0, 2, 3, 1)
    if c % 4:
        t = torch.nn.functional.pad(t, (0, ops.pad4(c) - c), value=fill)
    return t.contiguous()


def _rois_in(rois, who):
    if not rois.is_cuda:
        raise RuntimeError("rois must be a CUDA tensor")  # ROIAlign_cuda.cu:264
    if rois.dim() != 2 or rois.shape[1] != 5:
        raise RuntimeError("%s: rois must be [K, 5]" % who)
    return rois.float().contiguous()


def _scale1(s):
    return (ctypes.c_float * 1)(float(s))


def roi_align_host(input, rois, spatial_scale, pooled_height, pooled_width, sampling_ratio):
    """The reference's CPU dispatch (csrc/ROIAlign.h:24, csrc/cpu/ROIAlign_cpu.cpp:113-257) for host tensors, float or double:
    positions, weights and cells in the tensors' own dtype, operation by operation in the source's order; per ROI the samples
    of all bins are formed once for all channels.  An image index outside [0, N) gives zeros (the reference reads out of
    bounds there)."""
    if input.is_cuda or rois.is_cuda:
        raise RuntimeError("input and rois must be CPU tensors")  # ROIAlign_cpu.cpp:227-228
    if input.dtype not in (torch.float32, torch.float64) or rois.dtype != input.dtype:
        raise RuntimeError("ROIAlign_forward: float or double input, rois of the same type")
    N, C, H, W = input.shape
    K, PH, PW = rois.shape[0], int(pooled_height), int(pooled_width)
    out = torch.zeros((K, C, PH, PW), dtype=input.dtype)
    x = input.contiguous()
    T = input.dtype
    scale = torch.tensor(spatial_scale, dtype=torch.float32).to(T)  # `const float spatial_scale`, then `const T&`

    def axis(start, binsz, P, g, size):
        """positions of the P * g samples of an axis -> live, low cell, high cell, l, h"""
        p = torch.arange(P, dtype=T).repeat_interleave(g)
        i = torch.arange(g, dtype=torch.float32).repeat(P)
        y = start + p * binsz + (i + 0.5).to(T) * binsz / torch.tensor(float(g), dtype=T)
        live = ~((y < -1.0) | (y > size))
        y = torch.where((y <= 0) | ~live, torch.zeros_like(y), y)
        lo = y.to(torch.int64).clamp(max=size - 1)  # dead samples are masked below
        top = lo >= size - 1
        hi = torch.where(top, lo, lo + 1)
        y = torch.where(top, lo.to(T), y)
        l = y - lo.to(T)
        return live, lo, hi, l, 1.0 - l

    for k in range(K):
        r = rois[k]
        n = int(r[0])
        if not 0 <= n < N:
            continue
        sw, sh, ew, eh = r[1] * scale, r[2] * scale, r[3] * scale, r[4] * scale
        one = torch.ones((), dtype=T)
        rw, rh = torch.maximum(ew - sw, one), torch.maximum(eh - sh, one)
        bh, bw = rh / PH, rw / PW
        gh = sampling_ratio if sampling_ratio > 0 else int(torch.ceil(rh / PH))
        gw = sampling_ratio if sampling_ratio > 0 else int(torch.ceil(rw / PW))
        ly_, ylo, yhi, ly, hy = axis(sh, bh, PH, gh, H)
        lx_, xlo, xhi, lx, hx = axis(sw, bw, PW, gw, W)
        live = (ly_[:, None] & lx_[None, :]).to(T)
        img = x[n]  # [C, H, W]
        w1, w2, w3, w4 = hy[:, None] * hx[None, :], hy[:, None] * lx[None, :], ly[:, None] * hx[None, :], ly[:, None] * lx[None, :]
        v1, v2 = img[:, ylo[:, None], xlo[None, :]], img[:, ylo[:, None], xhi[None, :]]
        v3, v4 = img[:, yhi[:, None], xlo[None, :]], img[:, yhi[:, None], xhi[None, :]]
        val = ((w1 * live) * v1 + (w2 * live) * v2 + (w3 * live) * v3 + (w4 * live) * v4).view(C, PH, gh, PW, gw)
        acc = torch.zeros((C, PH, PW), dtype=T)
        for iy in range(gh):
            for ix in range(gw):
                acc = acc + val[:, :, iy, :, ix]
        out[k] = acc / torch.tensor(float(gh * gw), dtype=T)
    return out


def roi_align_forward(*args, **kwargs):
    """roi_align_forward(input [N,C,H,W], rois [K,5], spatial_scale, pooled_height, pooled_width, sampling_ratio) ->
    [K,C,PH,PW]   (csrc/ROIAlign.h:11-25; CPU tensors: roi_align_host)"""
    input, rois, scale, ph, pw, sr = _take("roi_align_forward", ("input", "rois", "spatial_scale", "pooled_height",
                                                                 "pooled_width", "sampling_ratio"), args, kwargs)
    if not input.is_cuda:
        return roi_align_host(input, rois, scale, ph, pw, sr)
    rows, shape, c = _rows_in(input, "roi_align_forward")
    rois = _rois_in(rois, "roi_align_forward")
    y = torch.empty((rois.shape[0], int(ph), int(pw), rows.shape[1]), dtype=torch.float32, device=input.device)
    call("scan_roi_align_forward", _ptr(rows), shape.ref(), c, rows.shape[1], _ptr(rois), None, _scale1(scale), rois.shape[0],
         int(ph), int(pw), int(sr), _ptr(y), _stream())
    return y[..., :c].permute(0, 3, 1, 2).contiguous().to(input.dtype)


def roi_align_backward(*args, **kwargs):
    """roi_align_backward(grad [K,C,PH,PW], rois, spatial_scale, pooled_height, pooled_width, batch_size, channels, height,
    width, sampling_ratio) -> [N,C,H,W]   (csrc/ROIAlign.h:27-45)"""
    grad, rois, scale, ph, pw, bs, ch, h, w, sr = _take(
        "roi_align_backward", ("grad", "rois", "spatial_scale", "pooled_height", "pooled_width", "batch_size", "channels",
                               "height", "width", "sampling_ratio"), args, kwargs)
    if not grad.is_cuda:
        raise RuntimeError("Not implemented on the CPU")  # csrc/ROIAlign.h:44
    rois = _rois_in(rois, "roi_align_backward")
    dy = _pooled_in(grad.float(), int(ch), 0.0, "roi_align_backward")
    shape = ops.PyramidShape(int(bs), [(int(h), int(w))])
    cs = dy.shape[-1]
    dx = torch.empty((shape.rows, cs), dtype=torch.float32, device=grad.device)
    call("scan_roi_align_backward", _ptr(dy), shape.ref(), int(ch), cs, _ptr(rois), None, _scale1(scale), rois.shape[0], int(ph),
         int(pw), int(sr), _ptr(dx), _stream())
    return dx.view(int(bs), int(h), int(w), cs)[..., :int(ch)].permute(0, 3, 1, 2).contiguous().to(grad.dtype)


def roi_pool_forward(*args, **kwargs):
    """roi_pool_forward(input [N,C,H,W], rois [K,5], spatial_scale, pooled_height, pooled_width) -> (output [K,C,PH,PW],
    argmax int32 [K,C,PH,PW])   (csrc/ROIPool.h:10-25)"""
    input, rois, scale, ph, pw = _take("roi_pool_forward", ("input", "rois", "spatial_scale", "pooled_height", "pooled_width"),
                                       args, kwargs)
    if not input.is_cuda:
        raise RuntimeError("Not implemented on the CPU")  # csrc/ROIPool.h:24
    rows, shape, c = _rows_in(input, "roi_pool_forward")
    rois = _rois_in(rois, "roi_pool_forward")
    y = torch.empty((rois.shape[0], int(ph), int(pw), rows.shape[1]), dtype=torch.float32, device=input.device)
    argmax = torch.empty(y.shape, dtype=torch.int32, device=input.device)
    call("scan_roi_pool_forward", _ptr(rows), shape.ref(), c, rows.shape[1], _ptr(rois), None, _scale1(scale), rois.shape[0],
         int(ph), int(pw), _ptr(y), _ptr(argmax), _stream())
    return (y[..., :c].permute(0, 3, 1, 2).contiguous().to(input.dtype), argmax[..., :c].permute(0, 3, 1, 2).contiguous())


def roi_pool_backward(*args, **kwargs):
    """roi_pool_backward(grad [K,C,PH,PW], input, rois, argmax, spatial_scale, pooled_height, pooled_width, batch_size, channels,
    height, width) -> [N,C,H,W]   (csrc/ROIPool.h:27-47)"""
    grad, input, rois, argmax, scale, ph, pw, bs, ch, h, w = _take(
        "roi_pool_backward", ("grad", "input", "rois", "argmax", "spatial_scale", "pooled_height", "pooled_width", "batch_size",
                              "channels", "height", "width"), args, kwargs)
    if not grad.is_cuda:
        raise RuntimeError("Not implemented on the CPU")  # csrc/ROIPool.h:46
    rois = _rois_in(rois, "roi_pool_backward")
    dy = _pooled_in(grad.float(), int(ch), 0.0, "roi_pool_backward")
    am = _pooled_in(argmax.to(torch.int32), int(ch), -1, "roi_pool_backward")
    shape = ops.PyramidShape(int(bs), [(int(h), int(w))])
    cs = dy.shape[-1]
    dx = torch.empty((shape.rows, cs), dtype=torch.float32, device=grad.device)
    call("scan_roi_pool_backward", _ptr(dy), _ptr(am), shape.ref(), int(ch), cs, _ptr(rois), None, _scale1(scale), rois.shape[0],
         int(ph), int(pw), _ptr(dx), _stream())
    return dx.view(int(bs), int(h), int(w), cs)[..., :int(ch)].permute(0, 3, 1, 2).contiguous().to(grad.dtype)


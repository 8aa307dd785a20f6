"""Operator surface mirroring ``fcos_core.layers`` for the SCAN hot path
(reference fcos_core/layers/__init__.py:4-27): same class names, constructor
arguments and forward semantics, HIP underneath."""
import torch
from torch import nn

from .. import _C as _C_ctypes, ops

# ``_C``: the compiled pybind11 module a reference checkout imports as fcos_core._C (scan_amd/csrc/fcos_core_C.cpp, built by
# __graft_entry__.build() into scan_amd/ext/fcos_core/); scan_amd/_C.py is the same eight functions bound through ctypes
# (kept for environments without a C++ toolchain -- both sit on the C ABI of libscan_hip.so, neither computes anything itself)
try:
    from ..ext.fcos_core import _C
    C_BACKEND = "compiled"
except ImportError:
    _C = _C_ctypes
    C_BACKEND = "ctypes"

nms = _C.nms
ml_nms = _C.ml_nms

# ``_ops``: the conv / GroupNorm / dynamic-conv operators with C++ autograd (scan_amd/csrc/scan_ops_ext.cpp ->
# scan_amd/ext/scan_ops/_ops<EXT_SUFFIX>): the NCHW drop-in modules below run forward and backward on it without entering
# the Python interpreter between kernel launches.  Without a C++ toolchain (or with SCAN_OPS_BACKEND=python) the same
# modules go through scan_amd.ops (Python autograd.Function -> ctypes): same kernels, bit-identical results.
import os as _os
try:
    if _os.environ.get("SCAN_OPS_BACKEND", "") == "python":
        raise ImportError("SCAN_OPS_BACKEND=python")
    from ..ext.scan_ops import _ops
    from .._lib import lib as _lib_handle
    # a module left over from an earlier build must not run against a newer library: both report the ABI they were built for
    if int(_ops.scan_abi_version()) != int(_lib_handle().scan_abi_version()):
        raise ImportError("scan_ops._ops was built for ABI %d, libscan_hip.so is ABI %d: rebuild (__graft_entry__.build())"
                          % (_ops.scan_abi_version(), _lib_handle().scan_abi_version()))
    OPS_BACKEND = "compiled"
    ops._EXT_INVALIDATE = _ops.invalidate_weight_cache  # ops.invalidate_weight_planes() then drops the C++ side's planes too
except ImportError as _e:
    if "ABI" in str(_e):
        import warnings as _warnings
        _warnings.warn(str(_e) + " -- scan_amd.layers uses its ctypes bindings")
    _ops = None
    OPS_BACKEND = "python"


class SigmoidFocalLoss(nn.Module):
    """reference layers/sigmoid_focal_loss.py:56-70: returns the SUM of the element losses."""

    def __init__(self, gamma, alpha):
        super().__init__()
        self.gamma = gamma
        self.alpha = alpha

    def forward(self, logits, targets):
        return ops.sigmoid_focal_loss_sum(logits, targets, self.gamma, self.alpha)

    def __repr__(self):
        return "%s(gamma=%s, alpha=%s)" % (self.__class__.__name__, self.gamma, self.alpha)


class IOULoss(nn.Module):
    """reference layers/iou_loss.py:5-36."""

    def forward(self, pred, target, weight=None):
        assert pred.numel() != 0
        return ops.iou_loss(pred, target, weight)


class FocalLoss(nn.Module):
    """The FocalLoss actually bound by the reference (layers/__init__.py:24 ->
    layers/sigmoid_focal_loss_wbg.py:7-64): softmax focal loss, alpha = 1, mean."""

    def __init__(self, class_num, alpha=None, gamma=2, size_average=True):
        super().__init__()
        assert alpha is None and size_average, "only the configuration SCAN uses is built"
        self.class_num = class_num
        self.gamma = gamma

    def forward(self, inputs, targets):
        return ops.softmax_focal_loss_mean(inputs, targets, self.gamma)


class Scale(nn.Module):
    """reference layers/scale.py:5-11."""

    def __init__(self, init_value=1.0):
        super().__init__()
        self.scale = nn.Parameter(torch.FloatTensor([init_value]))

    def forward(self, input):
        return input * self.scale


class GradientReversal(nn.Module):
    """reference modeling/discriminator/layer.py:27-33."""

    def __init__(self, lambda_=1):
        super().__init__()
        self.lambda_ = lambda_

    def forward(self, x):
        return ops.grad_reverse(x, self.lambda_)


class MultiHeadAttention(nn.Module):
    """Graph-node aggregation (reference layers/transformer.py:36-90).  Stays on the torch
    tier (north star: node aggregation is host-side glue): a handful of [n,256] matmuls.
    Quirks kept: heads are a plain .view(heads,-1,64) of the [1,n,256] tensor; scale is
    (64 // heads) ** -0.5; dropout on attention and output."""

    def __init__(self, model_dim=400, num_heads=4, dropout=0.0):
        super().__init__()
        self.dim_per_head = model_dim // num_heads
        self.num_heads = num_heads
        self.linear_k = nn.Linear(model_dim, self.dim_per_head * num_heads)
        self.linear_v = nn.Linear(model_dim, self.dim_per_head * num_heads)
        self.linear_q = nn.Linear(model_dim, self.dim_per_head * num_heads)
        self.linear_final = nn.Linear(model_dim, model_dim)
        self.dropout = nn.Dropout(dropout)
        self.attn_dropout = nn.Dropout(dropout)
        self.layer_norm = nn.LayerNorm(model_dim)

    def forward(self, key, value, query, attn_mask=None):
        residual = query
        d, h = self.dim_per_head, self.num_heads
        b = key.size(0)
        key = self.linear_k(key).view(b * h, -1, d)
        value = self.linear_v(value).view(b * h, -1, d)
        query = self.linear_q(query).view(b * h, -1, d)
        scale = (key.size(-1) // h) ** -0.5
        attention = self.attn_dropout(torch.softmax(torch.bmm(query, key.transpose(1, 2)) * scale, dim=2))
        context = torch.bmm(attention, value).view(b, -1, d * h)
        output = self.dropout(self.linear_final(context))
        return self.layer_norm(residual + output), attention


# ----------------------------------------------------------------------------- NCHW drop-in modules
# The reference's modules call torch.nn.Conv2d / nn.GroupNorm / F.conv2d on NCHW tensors (rpn/fcos/fcos.py:25-64,
# rpn/fcos/condgraph.py:86-106,619-629, discriminator/fcos_head_discriminator_con.py:20-87).  These classes keep those
# constructor signatures and the NCHW call convention, so such a module file runs on the HIP kernels by swapping the
# import.  A torch.channels_last NCHW tensor IS the kernels' pixel-major row matrix, so the adaptor
# is a view in both directions; any other layout is converted once on entry.
def _to_rows(x):
    """[N,C,H,W] -> (rows [N*H*W, Cs], PyramidShape, C): zero-copy for channels_last tensors with C % 4 == 0."""
    n, c, h, w = x.shape
    rows = x.permute(0, 2, 3, 1)
    if c % 4 != 0:
        rows = torch.nn.functional.pad(rows, (0, ops.pad4(c) - c))
    rows = rows.contiguous().view(n * h * w, -1)
    return rows, ops.PyramidShape(n, [(h, w)]), c


def _to_nchw(rows, shape, c):
    h, w = shape.sizes[0]
    return rows.view(shape.n_images, h, w, rows.shape[1])[..., :c].permute(0, 3, 1, 2)  # channels_last NCHW view


class Conv2d(nn.Conv2d):
    """torch.nn.Conv2d(in_channels, out_channels, kernel_size, stride=1, padding=0, ...) on the MFMA conv kernels:
    kernel 1 / 3 (5 / 7 through the generic kernel), stride 1 / 2, padding = kernel // 2, dilation 1, groups 1 -- the
    convolutions the SCAN modules build.  Input and output are NCHW (channels_last memory format)."""

    def forward(self, x):
        k, s = self.kernel_size[0], self.stride[0]
        if (self.kernel_size[0] != self.kernel_size[1] or self.stride[0] != self.stride[1] or self.groups != 1
                or tuple(self.dilation) != (1, 1) or tuple(self.padding) != (k // 2, k // 2) or s not in (1, 2)
                or self.padding_mode != "zeros"):
            raise RuntimeError("scan_amd.layers.Conv2d: only square kernels, stride 1 / 2, padding = k // 2, "
                               "dilation 1, groups 1 are built (what the SCAN modules use)")
        if _ops is not None and k in (1, 3) and ops.CONV_MODE == "bf16x6":
            return _ops.conv2d(x, self.weight, self.bias, s, False)
        rows, shape, _ = _to_rows(x)
        w = self.weight
        if not w.permute(0, 2, 3, 1).is_contiguous():  # kernels read [Cout][k*k][Cin]
            w = w.contiguous(memory_format=torch.channels_last)
        y = ops.conv2d(rows, w, self.bias, shape, k, s)
        return _to_nchw(y, shape.conv_out(k, s), self.out_channels)


class GroupNorm(nn.GroupNorm):
    """torch.nn.GroupNorm(32, 256) (+ the ReLU that follows it in every SCAN tower when relu=True) on NCHW tensors."""

    def __init__(self, num_groups, num_channels, eps=1e-5, affine=True, relu=False):
        super().__init__(num_groups, num_channels, eps, affine)
        self.fuse_relu = relu

    def forward(self, x):
        # the kernels are built for the one GroupNorm the SCAN modules use: 32 groups, affine, whole float4 channel groups
        if self.num_groups != 32 or not self.affine or self.num_channels % 32 != 0 or x.shape[1] != self.num_channels:
            raise RuntimeError("scan_amd.layers.GroupNorm: only GroupNorm(32, C) with affine=True and C %% 32 == 0 is built "
                               "(got num_groups=%d, num_channels=%d, affine=%s, input channels=%d)"
                               % (self.num_groups, self.num_channels, self.affine, x.shape[1]))
        if _ops is not None:
            return _ops.group_norm_relu(x, self.weight, self.bias, self.eps, self.fuse_relu)
        rows, shape, c = _to_rows(x)
        y = ops.groupnorm_relu(rows, self.weight, self.bias, shape, relu=self.fuse_relu, eps=self.eps)
        return _to_nchw(y, shape, c)


def conv3x3_gn_relu(x, conv, gn, relu=True):
    """The tower block of every SCAN head -- ``[nn.Conv2d(C, 256, 3, 1, 1), nn.GroupNorm(32, 256), nn.ReLU()]``
    (rpn/fcos/fcos.py:36-49, rpn/fcos/condgraph.py:99-105, discriminator/fcos_head_discriminator_con.py:20-34) -- as ONE
    operator: the GroupNorm statistics come out of the conv's epilogue, normalisation + ReLU are one pass.  ``conv`` / ``gn``:
    modules (or anything with .weight / .bias, gn.eps) holding the parameters; x and the result are NCHW."""
    if _ops is not None and ops.CONV_MODE == "bf16x6":
        return _ops.conv3x3_gn_relu(x, conv.weight, conv.bias, gn.weight, gn.bias, gn.eps, relu)
    rows, shape, _ = _to_rows(x)
    w = conv.weight
    if not w.permute(0, 2, 3, 1).is_contiguous():
        w = w.contiguous(memory_format=torch.channels_last)
    y = ops.conv2d(rows, w, conv.bias, shape, 3, 1, gn_sums=True)
    y = ops.groupnorm_relu(y, gn.weight, gn.bias, shape, relu=relu, eps=gn.eps)
    return _to_nchw(y, shape, conv.weight.shape[0])


def dynamic_conv_softmax(features, kernel_par):
    """GRAPHModule.dynamic_conv + softmax(dim=1) (reference condgraph.py:619-629, 344-346): features [N,256,H,W],
    kernel_par [K,256] -> (act-map logits [N,K,H,W], act maps [N,K,H,W])."""
    if _ops is not None:
        return tuple(_ops.dynamic_conv_softmax(features, kernel_par))
    rows, shape, _ = _to_rows(features)
    logits, probs = ops.dynconv_softmax(rows, kernel_par)
    h, w = shape.sizes[0]
    back = lambda t: t.view(shape.n_images, h, w, t.shape[1]).permute(0, 3, 1, 2)
    return back(logits), back(probs)


# ----------------------------------------------------------------------------- deformable convolution (DCNv2)
# The reference exports DFConv2d (layers/__init__.py:8,29, layers/misc.py:113-184) on top of the ModulatedDeformConv / DeformConv
# of a package it does not ship, so there is no reference arithmetic: these modules implement the published DCNv2 definition
# (the mmcv / torchvision semantics, include/scan_hip.h: scan_deform_sample_forward) -- Python backend only, scan_ops._ops has
# no binding for it.
def _dcn_unsupported(name, kernel_size, stride, padding, dilation, groups, deformable_groups):
    pair = lambda v: tuple(v) if isinstance(v, (list, tuple)) else (v, v)
    if (pair(kernel_size) != (3, 3) or pair(stride) != (1, 1) or pair(padding) != (1, 1) or pair(dilation) != (1, 1)
            or groups != 1 or deformable_groups != 1):
        raise RuntimeError("scan_amd.layers.%s: only kernel 3, stride 1, padding 1, dilation 1, groups 1, "
                           "deformable_groups 1 are built (what the FCOS tower uses)" % name)


class ModulatedDeformConv(nn.Module):
    """mmcv-style ModulatedDeformConv(in_channels, out_channels, kernel_size, ...): weight [O, C, 3, 3] (channels_last) and an
    optional bias; forward(x, offset, mask) on NCHW tensors, offset [N, 18, H, W] (dy, dx per tap), mask [N, 9, H, W]."""
    modulated = True

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=1, dilation=1, groups=1,
                 deformable_groups=1, bias=True):
        super().__init__()
        _dcn_unsupported(type(self).__name__, kernel_size, stride, padding, dilation, groups, deformable_groups)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, 3, 3).contiguous(memory_format=torch.channels_last))
        self.bias = nn.Parameter(torch.zeros(out_channels)) if bias else None
        stdv = 1.0 / (in_channels * 9) ** 0.5  # mmcv's reset_parameters
        nn.init.uniform_(self.weight, -stdv, stdv)

    def rows_forward(self, rows, offset, mask, shape, gn_sums=False):
        """the op on pyramid rows: offset [M, >= 18], mask [M, >= 9] or None (ops.deform_conv2d)"""
        w = self.weight
        if not w.permute(0, 2, 3, 1).is_contiguous():  # kernels read [Cout][k*k][Cin]
            w = w.contiguous(memory_format=torch.channels_last)
        return ops.deform_conv2d(rows, offset, mask, w, self.bias, shape, gn_sums=gn_sums)

    def forward(self, x, offset, mask=None):
        if self.modulated and mask is None:
            raise RuntimeError("ModulatedDeformConv: forward(x, offset, mask) needs a mask")
        if offset.shape[1] != 18 or (mask is not None and mask.shape[1] != 9) or x.shape[1] != self.in_channels:
            raise RuntimeError("deformable conv: x %s, offset %s (18 channels), mask %s (9 channels) do not fit"
                               % (tuple(x.shape), tuple(offset.shape), None if mask is None else tuple(mask.shape)))
        rows, shape, _ = _to_rows(x)
        off = _to_rows(offset)[0]
        msk = _to_rows(mask)[0] if mask is not None else None
        return _to_nchw(self.rows_forward(rows, off, msk, shape), shape, self.out_channels)


class DeformConv(ModulatedDeformConv):
    """DCNv1: forward(x, offset), the mask is 1."""
    modulated = False

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=1, dilation=1, groups=1,
                 deformable_groups=1, bias=False):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, deformable_groups, bias)

    def forward(self, x, offset):
        return super().forward(x, offset, None)


class DFConv2d(nn.Module):
    """reference layers/misc.py:113-184: ``offset`` = Conv2d(in, 27 or 18, 3, 1, 1) predicting the offsets (and the mask
    logits), ``conv`` = ModulatedDeformConv or DeformConv; state_dict keys offset.weight, offset.bias, conv.weight(, conv.bias)."""

    def __init__(self, in_channels, out_channels, with_modulated_dcn=True, kernel_size=3, stride=1, groups=1, padding=1,
                 dilation=1, deformable_groups=1, bias=False):
        super().__init__()
        _dcn_unsupported("DFConv2d", kernel_size, stride, padding, dilation, groups, deformable_groups)
        self.offset_base_channels = 9
        self.offset = Conv2d(in_channels, 27 if with_modulated_dcn else 18, kernel_size=3, stride=1, padding=1)
        nn.init.kaiming_uniform_(self.offset.weight, a=1)
        nn.init.constant_(self.offset.bias, 0.)
        self.offset.weight.data = self.offset.weight.data.contiguous(memory_format=torch.channels_last)
        self.conv = (ModulatedDeformConv if with_modulated_dcn else DeformConv)(in_channels, out_channels, bias=bias)
        self.with_modulated_dcn = with_modulated_dcn
        self.kernel_size, self.stride, self.padding, self.dilation = kernel_size, stride, padding, dilation

    def rows_forward(self, rows, shape, gn_sums=False):
        """the layer on pyramid rows (modeling.fcos.run_tower): ONE conv gives the 27 (18) offset / mask channels at pitch 28
        (20); the deformable conv reads its offsets as the first 18 columns of that matrix."""
        w = self.offset.weight
        if not w.permute(0, 2, 3, 1).is_contiguous():
            w = w.contiguous(memory_format=torch.channels_last)
        om = ops.conv2d(rows, w, self.offset.bias, shape, 3, 1)
        mask = om[:, 18:27].sigmoid() if self.with_modulated_dcn else None
        return self.conv.rows_forward(rows, om, mask, shape, gn_sums=gn_sums)

    def forward(self, x):
        assert x.numel() > 0, "only non-empty tensors are supported"
        if not x.is_cuda:
            raise RuntimeError("scan_amd.layers.DFConv2d runs only on the GPU (HIP) -- got a %s tensor; no CPU fallback" % x.device)
        if not self.with_modulated_dcn:
            return self.conv(x, self.offset(x))
        offset_mask = self.offset(x)
        split_point = self.offset_base_channels * 2
        return self.conv(x, offset_mask[:, :split_point, :, :], offset_mask[:, split_point:, :, :].sigmoid())


# ----------------------------------------------------------------------------- region pooling (ROIAlign / ROIPool)
# reference layers/roi_align.py:11-68 and layers/roi_pool.py:11-63 over _C.roi_align_* / _C.roi_pool_* (csrc/cuda/ROIAlign_cuda.cu,
# csrc/cuda/ROIPool_cuda.cu): the same call signatures and __repr__ on NCHW tensors, contiguous NCHW [K, C, PH, PW] out.  The
# arithmetic is ops.roi_align / ops.roi_pool on the row matrix of the input (csrc/roi.hip; a channels_last input with C % 4 == 0
# IS that matrix), whose gradients are per-destination sums without float atomics.  GPU tensors only, as every op here;
# _C.roi_align_forward mirrors the reference's CPU dispatch for host tensors.
def _pair(v):
    return tuple(v) if isinstance(v, (list, tuple)) else (v, v)


def roi_align(input, roi, output_size, spatial_scale, sampling_ratio):
    rows, shape, c = _to_rows(input)
    y = ops.roi_align(rows, shape, roi, _pair(output_size), (spatial_scale,), sampling_ratio, c=c)
    return y[..., :c].permute(0, 3, 1, 2).contiguous()


class ROIAlign(nn.Module):
    def __init__(self, output_size, spatial_scale, sampling_ratio):
        super().__init__()
        self.output_size = output_size
        self.spatial_scale = spatial_scale
        self.sampling_ratio = sampling_ratio

    def forward(self, input, rois):
        return roi_align(input, rois, self.output_size, self.spatial_scale, self.sampling_ratio)

    def __repr__(self):
        return "%s(output_size=%s, spatial_scale=%s, sampling_ratio=%s)" % (
            self.__class__.__name__, self.output_size, self.spatial_scale, self.sampling_ratio)


def roi_pool(input, roi, output_size, spatial_scale):
    rows, shape, c = _to_rows(input)
    y = ops.roi_pool(rows, shape, roi, _pair(output_size), (spatial_scale,), c=c)
    return y[..., :c].permute(0, 3, 1, 2).contiguous()


class ROIPool(nn.Module):
    def __init__(self, output_size, spatial_scale):
        super().__init__()
        self.output_size = output_size
        self.spatial_scale = spatial_scale

    def forward(self, input, rois):
        return roi_pool(input, rois, self.output_size, self.spatial_scale)

    def __repr__(self):
        return "%s(output_size=%s, spatial_scale=%s)" % (self.__class__.__name__, self.output_size, self.spatial_scale)

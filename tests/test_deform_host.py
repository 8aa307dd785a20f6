"""Deformable convolution (DCNv2), everything that needs no GPU: the oracle of tests/deform_ref.py against two independent
statements of the definition, the new C-ABI symbols and their argument checks, the DFConv2d module surface and the FCOS
head's state-dict layout with the tower switch off and on."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import deform_ref as R
from scan_amd import _lib, layers, ops
from scan_amd.layers import DFConv2d, DeformConv, ModulatedDeformConv
from scan_amd.modeling import fcos

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("scan_deform_sample_forward", "scan_deform_sample_backward", "scan_deform_dx_gather")


# ----------------------------------------------------------------------------- the oracle
def test_oracle_zero_offsets_is_plain_conv():
    g = torch.Generator().manual_seed(1)
    n, sizes, C, O = 2, ((6, 7), (3, 2), (1, 2)), 5, 4
    xs = [torch.randn(n, C, h, w, generator=g, dtype=torch.float64) for h, w in sizes]
    wgt = torch.randn(O, C, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(O, generator=g, dtype=torch.float64)
    rows = torch.cat([x.permute(0, 2, 3, 1).reshape(-1, C) for x in xs], 0)
    y = R.deform_conv(rows, torch.zeros(rows.shape[0], 18), torch.ones(rows.shape[0], 9), wgt, b, n, sizes)
    ref = torch.cat([F.conv2d(x, wgt, b, padding=1).permute(0, 2, 3, 1).reshape(-1, O) for x in xs], 0)
    np.testing.assert_allclose(y.numpy(), ref.numpy(), rtol=1e-12, atol=1e-13)


def test_oracle_matches_grid_sample_formulation():
    """random fractional offsets: every tap is F.grid_sample(align_corners=True, padding_mode="zeros") at the same positions;
    forward and the gradients w.r.t. x, offset and mask"""
    g = torch.Generator().manual_seed(2)
    n, H, W, C, O = 2, 6, 7, 3, 4
    M = n * H * W
    x0 = torch.randn(M, C, generator=g, dtype=torch.float64)
    off0 = (torch.rand(M, 18, generator=g) * 5 - 2.5).double()  # fp32-representable
    mask0 = torch.sigmoid(torch.randn(M, 9, generator=g, dtype=torch.float64))
    wgt = torch.randn(O, C, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(O, generator=g, dtype=torch.float64)
    gy = torch.randn(M, O, generator=g, dtype=torch.float64)

    def grads(fn):
        leaves = [t.clone().requires_grad_(True) for t in (x0, off0, mask0)]
        y = fn(*leaves)
        (y * gy).sum().backward()
        return [y.detach()] + [t.grad for t in leaves]

    def by_grid_sample(x, off, mask):
        xn = x.view(n, H, W, C).permute(0, 3, 1, 2)
        o = off.view(n, H, W, 18)
        ys = torch.arange(H, dtype=torch.float32).view(1, H, 1).expand(n, H, W)
        xs = torch.arange(W, dtype=torch.float32).view(1, 1, W).expand(n, H, W)
        y = b.view(1, O, 1, 1)
        for k in range(9):
            i, j = divmod(k, 3)
            oy, ox = o[..., 2 * k], o[..., 2 * k + 1]
            h = ((ys - 1 + i) + oy.detach().float()).double() + (oy - oy.detach())  # the fp32 position, promoted
            w = ((xs - 1 + j) + ox.detach().float()).double() + (ox - ox.detach())
            grid = torch.stack([2 * w / (W - 1) - 1, 2 * h / (H - 1) - 1], -1)
            s = F.grid_sample(xn, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
            s = s * mask.view(n, H, W, 9)[..., k][:, None]
            y = y + torch.einsum("oc,nchw->nohw", wgt[:, :, i, j], s)
        return y.permute(0, 2, 3, 1).reshape(M, O)

    mine = grads(lambda x, off, mask: R.deform_conv(x, off, mask, wgt, b, n, ((H, W),)))
    ref = grads(by_grid_sample)
    for name, a, r in zip(("y", "dx", "doffset", "dmask"), mine, ref):
        np.testing.assert_allclose(a.numpy(), r.numpy(), rtol=1e-9, atol=1e-13, err_msg=name)


@pytest.mark.parametrize("with_mask", [True, False])
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("C,O", R.CHANNELS)
def test_fp32_oracle_stays_inside_the_gpu_bars(C, O, family, with_mask):
    """the bars the GPU test holds the op to (those of test_conv2d_fwd_bwd) leave room for fp32 arithmetic on these exact
    inputs: the same formulas evaluated in fp32 are inside the tighter bar (2e-5) against fp64"""
    ref = R.reference(C, O, family, with_mask)
    f32 = R.reference(C, O, family, with_mask, torch.float32)
    for name in ("y", "dx", "doff", "dmask", "dw", "db"):
        if ref[name] is not None:
            R.assert_within(f32[name], ref[name], R.bar("bf16x6"), name)


def test_edge_family_hits_every_boundary():
    """the hand-made offsets put samples exactly on -1, 0, H - 1 and H, inside (-1, 0) and (H - 1, H), and at +-1e6 / +-1e30"""
    _, off, _, _, _, _ = R.case(4, 8, "edges", True)
    ro = R.row_offsets(R.N_IMAGES, R.SIZES)
    H, W = R.SIZES[0]
    o = off[ro[0]:ro[1]].view(R.N_IMAGES, H, W, 18)
    hs = torch.stack([(torch.arange(H).view(1, H, 1).float() - 1 + k // 3) + o[..., 2 * k] for k in range(9)]).reshape(-1)
    for v in (-1.0, 0.0, H - 1.0, float(H)):
        assert bool((hs == v).any()), v
    assert bool(((hs > -1) & (hs < 0)).any()) and bool(((hs > H - 1) & (hs < H)).any())
    for v in (1e6, -1e6, 1e30, -1e30):
        assert bool((off == torch.tensor(v, dtype=torch.float32)).any()), v


# ----------------------------------------------------------------------------- C ABI
def test_symbols_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "scan_hip.h")).read()
    declared = set(re.findall(r"\b(scan_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(L, name), name
    assert L.scan_abi_version() == 1


def test_arguments_validated_without_device():
    d = ops.PyramidShape(1, [(2, 2)])
    p = ctypes.c_void_p(64)
    fwd = lambda **kw: _lib.call("scan_deform_sample_forward", *[kw.get(k, v) for k, v in (
        ("x", p), ("d", d.ref()), ("C", 4), ("Cs", 4), ("off", p), ("ld_off", 18), ("mask", p), ("ld_mask", 9), ("cols", p),
        ("stream", None))])
    bwd = lambda **kw: _lib.call("scan_deform_sample_backward", *[kw.get(k, v) for k, v in (
        ("x", p), ("d", d.ref()), ("C", 4), ("Cs", 4), ("dcols", p), ("off", p), ("ld_off", 18), ("mask", p), ("ld_mask", 9),
        ("doff", p), ("ld_doff", 18), ("dmask", p), ("ld_dmask", 9), ("keys", p), ("wgts", p), ("stream", None))])
    gat = lambda **kw: _lib.call("scan_deform_dx_gather", *[kw.get(k, v) for k, v in (
        ("dcols", p), ("perm", p), ("seg", p), ("wgts", p), ("M", 4), ("C", 4), ("Cs", 4), ("dx", p), ("stream", None))])
    for fn in (fwd, bwd):
        for ptr in ("x", "d", "off"):
            with pytest.raises(RuntimeError, match="null"):
                fn(**{ptr: None})
        with pytest.raises(RuntimeError, match="Cs"):
            fn(Cs=6, C=4)
        with pytest.raises(RuntimeError, match="C=5"):
            fn(C=5)
        with pytest.raises(RuntimeError, match="ld_off"):
            fn(ld_off=17)
        with pytest.raises(RuntimeError, match="ld_mask"):
            fn(ld_mask=8)
        bad = ops.PyramidShape(1, [(2, 2)])
        bad.desc.n_levels = 6
        with pytest.raises(RuntimeError, match="bad pyramid"):
            fn(d=bad.ref())
        bad = ops.PyramidShape(1, [(2, 2)])
        bad.desc.row_off[1] = 5  # not n_images * h * w
        with pytest.raises(RuntimeError, match="bad pyramid"):
            fn(d=bad.ref())
        big = ops.PyramidShape(1, [(8192, 8192)])  # 36 * M = 2^31 + ...
        with pytest.raises(RuntimeError, match="2\\^31"):
            fn(d=big.ref())
    with pytest.raises(RuntimeError, match="null"):
        fwd(cols=None)
    for ptr in ("dcols", "doff", "keys", "wgts", "dmask"):
        with pytest.raises(RuntimeError, match="null"):
            bwd(**{ptr: None})
    with pytest.raises(RuntimeError, match="ld_doff"):
        bwd(ld_doff=17)
    for ptr in ("dcols", "perm", "seg", "wgts", "dx"):
        with pytest.raises(RuntimeError, match="null"):
            gat(**{ptr: None})
    with pytest.raises(RuntimeError, match="Cs"):
        gat(Cs=6)
    with pytest.raises(RuntimeError, match="C=5"):
        gat(C=5)
    with pytest.raises(RuntimeError, match="2\\^31"):
        gat(M=(1 << 31) // 36 + 1)
    with pytest.raises(RuntimeError, match="aligned"):
        fwd(x=ctypes.c_void_p(68))


# ----------------------------------------------------------------------------- modules
def test_dfconv2d_state_dict_init_and_refusals():
    m = DFConv2d(8, 6)  # the reference's defaults: modulated, no bias
    assert list(m.state_dict()) == ["offset.weight", "offset.bias", "conv.weight"]
    assert tuple(m.offset.weight.shape) == (27, 8, 3, 3) and tuple(m.conv.weight.shape) == (6, 8, 3, 3)
    assert isinstance(m.offset, layers.Conv2d) and isinstance(m.conv, ModulatedDeformConv)
    m = DFConv2d(8, 6, with_modulated_dcn=False, bias=True)
    assert list(m.state_dict()) == ["offset.weight", "offset.bias", "conv.weight", "conv.bias"]
    assert tuple(m.offset.weight.shape) == (18, 8, 3, 3) and isinstance(m.conv, DeformConv)
    # kaiming_uniform_(a=1): bound = sqrt(6 / ((1 + a^2) * fan_in)) = sqrt(3 / fan_in); zero bias
    bound = math.sqrt(3.0 / (8 * 9))
    assert 0.5 * bound < float(m.offset.weight.detach().abs().max()) <= bound
    assert float(m.offset.bias.abs().max()) == 0.0
    for kw in ({"kernel_size": 5}, {"kernel_size": 1}, {"stride": 2}, {"padding": 0}, {"dilation": 2}, {"groups": 2},
               {"deformable_groups": 2}):
        with pytest.raises(RuntimeError, match="scan_amd.layers.DFConv2d: only .* are built"):
            DFConv2d(8, 8, **kw)
        with pytest.raises(RuntimeError, match="only .* are built"):
            ModulatedDeformConv(8, 8, **kw)


def test_deformable_modules_refuse_cpu_tensors():
    x = torch.zeros(1, 8, 4, 4)
    with pytest.raises(RuntimeError, match="GPU"):
        DFConv2d(8, 8)(x)
    with pytest.raises(RuntimeError, match="GPU"):
        ModulatedDeformConv(8, 8)(x, torch.zeros(1, 18, 4, 4), torch.ones(1, 9, 4, 4))
    with pytest.raises(RuntimeError, match="GPU"):
        DeformConv(8, 8)(x, torch.zeros(1, 18, 4, 4))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.deform_conv2d(torch.zeros(16, 8), torch.zeros(16, 18), None, torch.zeros(8, 8, 3, 3), None, ops.PyramidShape(1, [(4, 4)]))


@pytest.mark.parametrize("num_convs", [1, 2, 4])
def test_fcos_head_keys_with_and_without_the_tower_switch(num_convs):
    plain = []
    for tower in ("cls_tower", "bbox_tower"):
        for i in range(num_convs):
            plain += ["%s.%d.%s" % (tower, 3 * i + s, p) for s in (0, 1) for p in ("weight", "bias")]
    tail = ["%s.%s" % (m, p) for m in ("cls_logits", "bbox_pred", "centerness") for p in ("weight", "bias")]
    tail += ["scales.%d.scale" % l for l in range(5)]
    head = fcos.FCOSHead(9, num_convs)
    assert list(head.state_dict().keys()) == plain + tail  # the default: today's layout
    assert list(fcos.FCOSHead(9, num_convs, use_dcn_in_tower=False).state_dict().keys()) == plain + tail
    assert [type(m).__name__ for m in head.cls_tower] == ["Conv2d", "GroupNorm", "ReLU"] * num_convs
    assert all(type(m) is torch.nn.Conv2d for m in head.cls_tower if hasattr(m, "kernel_size"))
    last = 3 * (num_convs - 1)
    dcn = []
    for k in plain:
        tower, idx, p = k.split(".")
        if int(idx) == last:  # the upstream FCOS layout of USE_DCN_IN_TOWER
            if p == "weight":
                dcn += ["%s.%d.%s" % (tower, last, q) for q in ("offset.weight", "offset.bias", "conv.weight", "conv.bias")]
        else:
            dcn.append(k)
    on = fcos.FCOSHead(9, num_convs, use_dcn_in_tower=True)
    assert list(on.state_dict().keys()) == dcn + tail
    assert isinstance(on.cls_tower[last], DFConv2d) and isinstance(on.bbox_tower[last], DFConv2d)
    assert tuple(on.cls_tower[last].conv.weight.shape) == (256, 256, 3, 3) and on.cls_tower[last].conv.bias is not None

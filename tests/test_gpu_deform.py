"""Deformable convolution (DCNv2) on the GPU against the definition-level oracle of tests/deform_ref.py: the sampling kernel
alone through the C ABI, ops.deform_conv2d forward and backward in every conv mode, its reduction to the plain 3x3 conv,
bit-reproducible gradients, the NCHW module layers.DFConv2d and the FCOS head's tower switch."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import deform_ref as R

pytestmark = pytest.mark.gpu

MODES = ("bf16x6", "bf16x3", "fp32")


def _shape():
    from scan_amd import ops
    return ops.PyramidShape(R.N_IMAGES, R.SIZES)


def _pad_cols(t, cs):
    return F.pad(t, (0, cs - t.shape[1])).contiguous() if cs != t.shape[1] else t.contiguous()


def _im2col(x, cs):
    """[M, C] pyramid rows -> [M, 9 * cs]: tap k = 3 i + j of row (n, y, x) is x at (y - 1 + i, x - 1 + j), zero outside"""
    ro, out = R.row_offsets(R.N_IMAGES, R.SIZES), []
    for l, (H, W) in enumerate(R.SIZES):
        xl = F.pad(_pad_cols(x[ro[l]:ro[l + 1]], cs).view(R.N_IMAGES, H, W, cs), (0, 0, 1, 1, 1, 1))
        out.append(torch.cat([xl[:, i:i + H, j:j + W, :] for i in range(3) for j in range(3)], -1).reshape(-1, 9 * cs))
    return torch.cat(out, 0)


# ----------------------------------------------------------------------------- 1. the sampling kernel alone
@pytest.mark.parametrize("with_mask", [True, False])
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("C,O", R.CHANNELS)
def test_sampling_alone(device, C, O, family, with_mask):
    """C ABI into a NaN-filled cols.  The bound is derived, not measured: the position is bit-equal to the oracle's, what is
    left are fewer than 16 fp32 roundings of terms bounded by S = |mask| * sum_corners w_i |x_i|."""
    from scan_amd import ops
    x, off, mask, _, _, _ = R.case(C, O, family, with_mask)
    shape, cs, M = _shape(), ops.pad4(C), x.shape[0]
    xd = _pad_cols(x, cs).to(device)
    # offsets and mask as column slices of one wider matrix (pitch 28), as the tower hands them over
    om = torch.full((M, 28), float("nan"), device=device)
    om[:, :18] = off.to(device)
    mk = None
    if with_mask:
        om[:, 18:27] = mask.to(device)
        mk = om[:, 18:27]
    cols = torch.full((M, 9 * cs), float("nan"), device=device)
    ops.call("scan_deform_sample_forward", ops._ptr(xd), shape.ref(), C, cs, ops._ptr(om), 28, ops._ptr(mk), 28 if with_mask else 0,
             ops._ptr(cols), ops._stream())
    got = cols.cpu().view(M, 9, cs)
    assert not bool(torch.isnan(got).any())
    if cs > C:
        assert float(got[:, :, C:].abs().max()) == 0.0
    ref, S = R.sample(x, off, mask, R.N_IMAGES, R.SIZES)
    err = (got[:, :, :C].double() - ref).abs()
    bound = 16 * 2.0 ** -24 * S
    print("sampling: max err %.3g, worst err / bound %.3g" % (float(err.max()), float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all())
    if family == "zeros" and not with_mask:  # the weights are exactly 1 and 0
        assert torch.equal(got.reshape(M, 9 * cs), _im2col(x, cs))


# ----------------------------------------------------------------------------- 2. the op against the oracle
def _run_op(device, C, O, family, with_mask):
    from scan_amd import ops
    x, off, mask, weight, bias, gy = R.case(C, O, family, with_mask)
    shape, cs = _shape(), ops.pad4(C)
    t = {"x": _pad_cols(x, cs).to(device).requires_grad_(True), "off": off.to(device).requires_grad_(True),
         "mask": mask.to(device).requires_grad_(True) if mask is not None else None,
         "w": weight.to(device).contiguous(memory_format=torch.channels_last).requires_grad_(True),
         "b": bias.to(device).requires_grad_(True)}
    y = ops.deform_conv2d(t["x"], t["off"], t["mask"], t["w"], t["b"], shape)
    assert y.shape == (x.shape[0], ops.pad4(O))
    if y.shape[1] > O:
        assert float(y.detach()[:, O:].abs().max()) == 0.0
    y.backward(_pad_cols(gy, y.shape[1]).to(device))
    return {"y": y.detach()[:, :O], "dx": t["x"].grad[:, :C], "doff": t["off"].grad,
            "dmask": t["mask"].grad if mask is not None else None, "dw": t["w"].grad, "db": t["b"].grad}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("with_mask", [True, False])
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("C,O", R.CHANNELS)
def test_deform_conv2d_fwd_bwd(device, C, O, family, with_mask, mode, monkeypatch):
    """y, dx, dW, db, doffset and dmask under the bars of test_conv2d_fwd_bwd, no element excluded"""
    from scan_amd import ops
    monkeypatch.setattr(ops, "CONV_MODE", mode)
    got, ref = _run_op(device, C, O, family, with_mask), R.reference(C, O, family, with_mask)
    for name in ("y", "dx", "dw", "db", "doff", "dmask"):
        if ref[name] is not None:
            R.assert_within(got[name], ref[name], R.bar(mode), "%s %s" % (mode, name))


# ----------------------------------------------------------------------------- 3. zero offsets, no mask: the plain conv
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C,O", R.CHANNELS)
def test_zero_offsets_reduce_to_conv2d(device, C, O, mode, monkeypatch):
    from scan_amd import ops
    monkeypatch.setattr(ops, "CONV_MODE", mode)
    got = _run_op(device, C, O, "zeros", False)
    x, _, _, weight, bias, gy = R.case(C, O, "zeros", False)
    shape, cs = _shape(), ops.pad4(C)
    xd = _pad_cols(x, cs).to(device).requires_grad_(True)
    wd = weight.to(device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    bd = bias.to(device).requires_grad_(True)
    y = ops.conv2d(xd, wd, bd, shape, 3, 1)
    y.backward(_pad_cols(gy, y.shape[1]).to(device))
    for name, ref in (("y", y.detach()[:, :O]), ("dx", xd.grad[:, :C]), ("dw", wd.grad), ("db", bd.grad)):
        R.assert_within(got[name], ref, R.bar(mode), "%s %s vs conv2d" % (mode, name))


# ----------------------------------------------------------------------------- 4. reproducibility
@pytest.fixture
def deterministic_knob():
    from scan_amd import ops
    old = ops.deterministic()
    yield ops.set_deterministic
    ops.set_deterministic(old)


@pytest.mark.parametrize("flag", [False, True])
@pytest.mark.parametrize("C,O", [(72, 40), (256, 256)])
def test_backward_is_bit_reproducible(device, C, O, flag, deterministic_knob):
    deterministic_knob(flag)
    a, b = _run_op(device, C, O, "fractional", True), _run_op(device, C, O, "fractional", True)
    for name in ("dx", "doff", "dmask", "dw"):
        assert torch.equal(a[name], b[name]), name


# ----------------------------------------------------------------------------- 5. the NCHW module
@pytest.mark.parametrize("modulated", [True, False])
def test_dfconv2d_module_followed_by_inplace_relu(device, modulated):
    """layers.DFConv2d against the oracle composed with an fp64 F.conv2d for the offset branch; the in-place ReLU behind it
    must be able to modify its output (as in test_nchw_modules_followed_by_inplace_relu)"""
    from scan_amd import layers
    torch.manual_seed(5)
    n, C, O, H, W = 2, 8, 6, 9, 15
    dcn = layers.DFConv2d(C, O, with_modulated_dcn=modulated, bias=True)
    nn.init.normal_(dcn.conv.bias, std=0.5)
    nn.init.normal_(dcn.offset.bias, std=0.5)
    x = torch.randn(n, C, H, W)
    gy = torch.randn(n, O, H, W)
    P = {k: v.detach().clone().double().requires_grad_(True) for k, v in dcn.state_dict().items()}
    x64 = x.double().requires_grad_(True)
    om = F.conv2d(x64, P["offset.weight"], P["offset.bias"], padding=1).permute(0, 2, 3, 1).reshape(n * H * W, -1)
    pre = R.deform_conv(x64.permute(0, 2, 3, 1).reshape(n * H * W, C), om[:, :18], om[:, 18:27].sigmoid() if modulated else None,
                        P["conv.weight"], P["conv.bias"], n, ((H, W),))
    pre = pre.view(n, H, W, O).permute(0, 3, 1, 2)
    gy = gy * (pre.detach().abs() > 1e-3)  # an output within rounding distance of 0 may take the other side of the ReLU
    (F.relu(pre) * gy).sum().backward()
    mine = nn.Sequential(dcn, nn.ReLU(inplace=True)).to(device)
    xd = x.to(device).requires_grad_(True)
    y = mine(xd)
    y.backward(gy.float().to(device))
    tol = R.bar("bf16x6")
    R.assert_within(y, F.relu(pre), tol, "y")
    R.assert_within(xd.grad, x64.grad, tol, "dx")
    for k, p in dcn.named_parameters():
        R.assert_within(p.grad, P[k].grad, tol, k)


# ----------------------------------------------------------------------------- 6. the tower switch
def test_tower_switch_matches_a_half_weight_plain_head(device):
    """offset convs zeroed: offsets are 0 and the mask is sigmoid(0) = 0.5, so the deformable layer is the plain conv with
    0.5 x its weights and biases (the biases are zero after the head's initialisation).  After a backward pass the offset
    convs receive finite, non-zero weight gradients."""
    from scan_amd import ops
    from scan_amd.modeling import fcos
    torch.manual_seed(6)
    dcn = fcos.FCOSHead(3, num_convs=2, use_dcn_in_tower=True)
    plain = fcos.FCOSHead(3, num_convs=2)
    sd = {}
    for k, v in dcn.state_dict().items():
        if ".offset." in k:
            continue
        sd[k.replace(".conv.", ".")] = 0.5 * v if ".conv." in k else v
    plain.load_state_dict(sd)
    for m in (dcn, plain):
        m.to(device)
        for p in m.parameters():
            if p.dim() == 4:
                p.data = p.data.contiguous(memory_format=torch.channels_last)
    for tower in (dcn.cls_tower, dcn.bbox_tower):
        nn.init.zeros_(tower[3].offset.weight)
        nn.init.zeros_(tower[3].offset.bias)
    shape = ops.PyramidShape(1, [(8, 12), (4, 6)])
    rows = torch.randn(shape.rows, 256, device=device)
    ref = plain(rows, shape)
    got = dcn(rows, shape)
    for name, a, r in zip(("logits", "bbox_reg", "centerness"), got, ref):
        R.assert_within(a, r, 2e-5, name)
    sum(t.sum() for t in got).backward()
    for tower in (dcn.cls_tower, dcn.bbox_tower):
        g = tower[3].offset.weight.grad
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0.0


def test_training_step_with_deformable_towers(device):
    """engine.build_model(dcn_in_tower=True): the upstream key layout in the FCOS head, and one domain-adaptation iteration of
    the Trainer (flat parameter buffers, side streams) gives finite losses and moves the deformable layers' parameters"""
    from scan_amd import engine, synth
    torch.manual_seed(7)
    assert "head.cls_tower.9.weight" in engine.build_model(9, device=device, attn_dropout=0.0)["fcos"].state_dict()
    model = engine.build_model(9, device=device, attn_dropout=0.0, dcn_in_tower=True)
    keys = set(model["fcos"].state_dict())
    for tower in ("cls_tower", "bbox_tower"):
        assert {"head.%s.9.%s" % (tower, k) for k in ("offset.weight", "offset.bias", "conv.weight", "conv.bias")} <= keys
        assert "head.%s.9.weight" % tower not in keys
    trainer = engine.Trainer(model)
    layer = model["fcos"].head.bbox_tower[9]
    before = {k: v.detach().clone() for k, v in layer.state_dict().items()}
    H, W, N = 128, 128, 1
    losses = trainer.step(synth.synth_images(N, H, W, 1234).to(device), synth.synth_targets(N, H, W, 8, 6, 4321),
                          synth.synth_images(N, H, W, 2234).to(device))
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v.detach()).all()) for v in losses.values()), losses
    after = layer.state_dict()
    for k in ("offset.weight", "conv.weight", "conv.bias"):
        assert bool(torch.isfinite(after[k]).all()) and not torch.equal(after[k], before[k]), k

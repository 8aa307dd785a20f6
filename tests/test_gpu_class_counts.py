"""Class counts beyond the two shipped label sets: the generic dynamic-conv kernels (2 <= K <= 32), the generic grouped
class-branch conv (1 <= G <= 31), the loss kernels at odd counts, and the full DA iteration at K = 8 / 21 against the
reference (tests/golden/step_k8_128x256.*, step_k21_128x256.*; oracle/make_golden.gen_step with MODEL.FCOS.NUM_CLASSES K)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-4  # the bar of tests/test_gpu_model.py


def _digest(g):
    flat = g.detach().double().reshape(-1).cpu()
    return [flat.sum().item(), flat.abs().sum().item()]


def _dynconv_case(M, K):
    """the construction of test_dynconv_softmax (tests/test_gpu_kernels.py): inputs and the torch-CPU fp32 results"""
    g = torch.Generator().manual_seed(M)
    feat = torch.randn(M, 256, generator=g)
    ker = torch.randn(K, 256, generator=g) / 16
    fr, kr = feat.clone().requires_grad_(True), ker.clone().requires_grad_(True)
    lr = fr @ kr.t()
    pr = lr.softmax(1)
    g1, g2 = torch.randn(M, K, generator=g), torch.randn(M, K, generator=g)
    ((lr * g1).sum() + (pr * g2).sum()).backward()
    return feat, ker, g1, g2, lr.detach(), pr.detach(), fr.grad, kr.grad


def _dynconv_run(device, feat, ker, g1, g2):
    from scan_amd import ops
    fd, kd = feat.to(device).requires_grad_(True), ker.to(device).requires_grad_(True)
    l, p = ops.dynconv_softmax(fd, kd)
    ((l * g1.to(device)).sum() + (p * g2.to(device)).sum()).backward()
    return l.detach(), p.detach(), fd.grad, kd.grad


def _dynconv_check(got, ref):
    """the bars of test_dynconv_softmax"""
    (l, p, df, dk), (lr, pr, dfr, dkr) = got, ref
    np.testing.assert_allclose(l.cpu().numpy(), lr.cpu().numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(p.cpu().numpy(), pr.cpu().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(df.cpu().numpy(), dfr.cpu().numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(dk.cpu().numpy(), dkr.cpu().numpy(), rtol=1e-4, atol=1e-4 * max(1.0, float(dkr.abs().max())))


# ----------------------------------------------------------------------------- 1. generic dynconv against torch-CPU fp32
@pytest.mark.parametrize("M", [1, 15, 17, 4099])
@pytest.mark.parametrize("K", [3, 8, 15, 16, 17, 21, 32])
def test_generic_dynconv_softmax(device, M, K):
    """K = 15 / 16 / 17 straddle the 16-class tile, M = 1 / 15 / 17 the 16-pixel group and the backward's row chunk,
    M = 4099 is many workgroups with a ragged tail"""
    feat, ker, g1, g2, *ref = _dynconv_case(M, K)
    _dynconv_check(_dynconv_run(device, feat, ker, g1, g2), ref)


# ----------------------------------------------------------------------------- 2. generic against specialised
@pytest.mark.parametrize("K", [2, 9])
def test_generic_dynconv_equals_specialised(device, K):
    """the generic kernels run the same MFMA chain per class column as the <K> instances: identical logits"""
    from scan_amd import _lib
    feat, ker, g1, g2, *_ = _dynconv_case(4099, K)
    spec = _dynconv_run(device, feat, ker, g1, g2)
    old = _lib.query("scan_tune", b"dynconv_generic", 1)
    try:
        assert old == 0
        gen = _dynconv_run(device, feat, ker, g1, g2)
    finally:
        _lib.query("scan_tune", b"dynconv_generic", old)
    assert _lib.query("scan_tune_get", b"dynconv_generic") == 0
    assert torch.equal(gen[0], spec[0])
    _dynconv_check(gen, spec)


# ----------------------------------------------------------------------------- 3. determinism
def test_generic_dynconv_backward_is_run_to_run_identical(device):
    feat, ker, g1, g2, *_ = _dynconv_case(4099, 21)
    a = _dynconv_run(device, feat, ker, g1, g2)
    b = _dynconv_run(device, feat, ker, g1, g2)
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


# ----------------------------------------------------------------------------- 4. limits
@pytest.mark.parametrize("K", [1, 33])
def test_dynconv_class_count_limits(device, K):
    from scan_amd import _lib, ops
    assert _lib.query("scan_dynconv_max_classes") == 32 and ops.dynconv_max_classes() == 32
    feat = torch.zeros((16, 256), device=device)
    ker = torch.zeros((K, 256), device=device)
    with pytest.raises(ValueError, match=r"2\.\.32"):
        ops.dynconv_softmax(feat, ker)
    # the C entry points: non-zero, the range in scan_last_error, and nothing launched (the outputs keep their fill)
    L, P = _lib.lib(), ops._ptr
    out = torch.full((2, 16, K), 7.0, device=device)
    ws = torch.zeros((1 << 16,), device=device)
    assert L.scan_dynconv_softmax_forward(P(feat), P(ker), 16, 256, K, P(out[0]), P(out[1]), ops._stream()) != 0
    assert "2..32" in L.scan_last_error().decode() and "got %d" % K in L.scan_last_error().decode()
    dfeat, dker = torch.full_like(feat, 7.0), torch.full_like(ker, 7.0)
    assert L.scan_dynconv_softmax_backward(P(feat), P(ker), P(out[1]), P(out[0]), P(out[0]), 16, 256, K, P(dfeat), P(dker),
                                           P(ws), ops._stream()) != 0
    assert "2..32" in L.scan_last_error().decode()
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 and float(dfeat.min()) == 7.0 and float(dker.min()) == 7.0


# ----------------------------------------------------------------------------- 5. generic grouped conv
@pytest.mark.parametrize("G", [3, 7, 20, 31])
def test_generic_grouped_conv(device, G):
    """scan_gconv3x3_to1_any_* at group counts without a lane map of their own, against F.conv2d(groups=G) on the CPU: a
    two-level pyramid of 2 images (5x7 and 3x4: every border case of the nine taps, levels abutting in row space)"""
    from scan_amd import _lib, ops
    assert _lib.query("scan_gconv3x3_to1_max_groups") == 31
    g = torch.Generator().manual_seed(41 + G)
    N, gc, ns, sizes = 2, G * 128, ops.pad4(G), [(5, 7), (3, 4)]
    xs = [torch.randn(N, gc, h, w, generator=g) for h, w in sizes]  # signed: the ReLU mask zeroes about half of dx
    wg = torch.randn(G, 128, 3, 3, generator=g) / 30
    bg = torch.randn(G, generator=g)
    ws_ = torch.randn(G, gc, 3, 3, generator=g)  # junk off the diagonal blocks: must be ignored
    for c in range(G):
        ws_[c, c * 128:(c + 1) * 128] = wg[c]
    gys = [torch.randn(N, G, h, w, generator=g) for h, w in sizes]
    # reference
    wr, br = wg.clone().requires_grad_(True), bg.clone().requires_grad_(True)
    y_ref, dx_ref = [], []
    for x, gy in zip(xs, gys):
        xr = x.clone().requires_grad_(True)
        yr = F.conv2d(xr, wr, br, padding=1, groups=G)
        yr.backward(gy)
        y_ref.append(yr.detach())
        dx_ref.append(xr.grad)
    rows_l, size_l = zip(*[ops.nchw_to_rows(x.to(device)) for x in xs])
    shape = ops.PyramidShape(N, [s.sizes[0] for s in size_l])
    rows = torch.cat(rows_l, 0).contiguous()
    gy_l = [ops.nchw_to_rows(F.pad(t, (0, 0, 0, 0, 0, ns - G)).to(device))[0] for t in gys]
    gy_rows = torch.cat(gy_l, 0).contiguous()
    wpk = ws_.to(device).permute(0, 2, 3, 1).contiguous()  # [G][9][G*128]
    L, P, st = _lib, ops._ptr, ops._stream()
    wsb = torch.empty((L.query("scan_gconv3x3_to1_ws_floats", shape.ref(), G, 128),), device=device)
    y = torch.full((shape.rows, ns), 7.0, device=device)
    bias = bg.to(device)
    L.call("scan_gconv3x3_to1_any_forward", P(rows), shape.ref(), G, 128, P(wpk), P(bias), P(y), ns, P(wsb), st)
    assert float(y[:, G:].abs().sum()) == 0
    for l in range(2):
        got = ops.rows_to_nchw(y, shape, l, G).cpu()
        np.testing.assert_allclose(got.numpy(), y_ref[l].numpy(), rtol=1e-4, atol=1e-5)

    def check_dx(dx, masked):
        for l in range(2):
            got = ops.rows_to_nchw(dx, shape, l, gc).cpu()
            want = dx_ref[l] * (xs[l] > 0) if masked else dx_ref[l]
            np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-4, atol=1e-5)

    def check_dw(dw, base):
        dw = dw.view(G, 3, 3, gc).permute(0, 3, 1, 2).cpu()
        for c in range(G):
            np.testing.assert_allclose((dw[c, c * 128:(c + 1) * 128] - base).numpy(), wr.grad[c].numpy(), rtol=2e-4,
                                       atol=2e-5 * float(wr.grad.abs().max()))
            off = torch.cat([dw[c, :c * 128], dw[c, (c + 1) * 128:]], 0)
            assert float((off - base).abs().sum()) == 0  # the off-diagonal blocks are not touched

    dws = []
    for relu_mask in (1, 0):
        dx, dw = torch.full_like(rows, 7.0), torch.zeros_like(wpk)
        L.call("scan_gconv3x3_to1_any_backward", P(rows), P(gy_rows), ns, shape.ref(), G, 128, P(wpk), relu_mask, P(dx), P(dw), 0,
               P(wsb), st)
        check_dx(dx, bool(relu_mask))
        check_dw(dw, 0.0)
        dws.append(dw)
    assert torch.equal(dws[0], dws[1])  # two runs: the same bits
    # the single-gradient entry points, and accumulate = 1 on top of a filled buffer
    for mask in (rows, None):
        dx = torch.full_like(rows, 7.0)
        L.call("scan_gconv3x3_to1_any_dgrad", P(gy_rows), ns, shape.ref(), G, 128, P(wpk), P(mask), P(dx), st)
        check_dx(dx, mask is not None)
    dw = torch.full_like(wpk, 0.5)
    L.call("scan_gconv3x3_to1_any_wgrad", P(rows), P(gy_rows), ns, shape.ref(), G, 128, P(dw), 1, P(wsb), st)
    check_dw(dw, 0.5)
    dw0 = torch.zeros_like(wpk)
    L.call("scan_gconv3x3_to1_any_wgrad", P(rows), P(gy_rows), ns, shape.ref(), G, 128, P(dw0), 0, P(wsb), st)
    check_dw(dw0, 0.0)
    # the autograd wrapper (bias gradient included) takes the same kernels
    rows_g = rows.clone().requires_grad_(True)
    wd = ws_.to(device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    bd = bg.to(device).requires_grad_(True)
    ya = ops.gconv3x3_to1(rows_g, wd, bd, shape, G, mask_dx=True)
    assert torch.equal(ya, y)
    ya.backward(gy_rows)
    check_dx(rows_g.grad, True)
    np.testing.assert_allclose(bd.grad.cpu().numpy(), br.grad.numpy(), rtol=2e-4, atol=1e-4)


def test_grouped_conv_group_limit(device):
    from scan_amd import _lib, ops
    P, st = ops._ptr, ops._stream()
    shape = ops.PyramidShape(1, [(4, 4)])
    z = torch.zeros((1 << 16,), device=device)
    with pytest.raises(RuntimeError, match=r"G=32 out of 1\.\.31"):
        _lib.call("scan_gconv3x3_to1_any_forward", P(z), shape.ref(), 32, 128, P(z), None, P(z), 32, P(z), st)
    with pytest.raises(RuntimeError, match=r"G=0 out of 1\.\.31"):
        _lib.call("scan_gconv3x3_to1_any_dgrad", P(z), 4, shape.ref(), 0, 128, P(z), None, P(z), st)
    with pytest.raises(RuntimeError, match=r"G=32 out of 1\.\.31"):
        _lib.call("scan_gconv3x3_to1_any_backward", P(z), P(z), 32, shape.ref(), 32, 128, P(z), 1, P(z), P(z), 0, P(z), st)
    # the entry points without "any" keep to the four lane-mapped group counts
    with pytest.raises(RuntimeError, match="G=7 must be 1, 2, 4 or 8"):
        _lib.call("scan_gconv3x3_to1_forward", P(z), shape.ref(), 7, 128, P(z), None, P(z), 8, P(z), st)
    # the bit-mask variants have no generic form
    with pytest.raises(RuntimeError, match="G=3 must be 1, 2, 4 or 8"):
        _lib.call("scan_gconv3x3_to1_forward_bits", P(z), shape.ref(), 3, 128, P(z), None, P(z), 4, P(z), P(z), st)


# ----------------------------------------------------------------------------- 6. discriminator parity at Cf = 7
def test_discriminator_generic_grouped_branch_equals_dense_branch(device):
    """FCOSDiscriminator_con at 8 classes (Cf = 7): the generic grouped second conv against the dense block-diagonal
    conv, the bars of test_discriminator_grouped_branch_equals_dense_branch"""
    from scan_amd import ops
    from scan_amd.modeling.discriminator import FCOSDiscriminator_con
    torch.manual_seed(5)
    dis = FCOSDiscriminator_con(num_convs=2, in_channels=256, num_classes=8).to(device)
    for m in dis.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.normal_(m.weight, std=0.05)
    shape = ops.PyramidShape(2, [(24, 40)])
    feat = torch.randn(shape.rows, 256, device=device)
    act = torch.softmax(torch.randn(shape.rows, 8, device=device), 1)
    res = []
    for flag in (True, False):
        ops.GROUPED_CLS = flag
        try:
            f = feat.clone().requires_grad_(True)
            dis.zero_grad()
            logits, _ = dis._logits(f, act, shape)
            ls, lt = dis.forward_pair(f, act, shape, 1)
            (ls + 2 * lt).backward()
            res.append([logits.detach(), ls.detach(), lt.detach(), f.grad,
                        dict(dis.named_parameters())["classifier_cls_3.2.weight"].grad.clone()])
        finally:
            ops.GROUPED_CLS = True
    for a, b in zip(*res):
        assert (a - b).abs().max().item() <= 2e-4 * max(b.abs().max().item(), 1e-6), (a.shape, (a - b).abs().max().item())


# ----------------------------------------------------------------------------- 7. loss kernels at odd counts
def test_softmax_focal_at_21_classes(device):
    """the generic path of the softmax focal kernel (reference layers/sigmoid_focal_loss_wbg.py:7-64: alpha 1, gamma 2,
    mean), bars of test_softmax_focal_golden"""
    from scan_amd import ops
    g = torch.Generator().manual_seed(21)
    M, C = 1003, 21
    z = torch.randn(M, C, generator=g) * 2
    lab = torch.randint(0, C, (M,), generator=g)
    zr = z.clone().requires_grad_(True)
    p = zr.softmax(1).gather(1, lab[:, None])[:, 0]
    ref = (-(1 - p) ** 2 * p.log()).mean()
    ref.backward()
    zd = z.to(device).requires_grad_(True)
    l = ops.softmax_focal_loss_mean(zd, lab.to(device), 2.0)
    assert abs(l.item() - ref.item()) <= 1e-5 * abs(ref.item())
    l.backward()
    np.testing.assert_allclose(zd.grad.cpu().numpy(), zr.grad.numpy(), rtol=1e-4, atol=1e-8)


@pytest.mark.parametrize("Cf", [7, 20])
def test_cka_bce_at_odd_class_counts(device, Cf):
    """ops.cka_bce / cka_bce_pair off the Cf == 8 fast path, against the torch spelling of test_bce_and_cka"""
    from scan_amd import ops
    torch.manual_seed(3 + Cf)
    M, m = 777, 300
    logits = torch.randn(M, Cf) * 2
    act = torch.softmax(torch.randn(M, Cf + 1), 1)

    def ref_loss(lc, a_all, target):
        ref = 0
        for c in range(Cf):
            a = a_all[:, c + 1]
            ref = ref + F.binary_cross_entropy_with_logits(lc[:, c], torch.full((lc.shape[0],), target), weight=a,
                                                           reduction="sum") / a.sum() / Cf
        return ref

    for target in (0.0, 1.0):
        lg = logits.to(device).requires_grad_(True)
        l = ops.cka_bce(lg, act.to(device), target, Cf)
        lc = logits.clone().requires_grad_(True)
        ref = ref_loss(lc, act, target)
        assert abs(l.item() - ref.item()) < 1e-5 * abs(ref.item())
        l.backward()
        ref.backward()
        np.testing.assert_allclose(lg.grad.cpu().numpy(), lc.grad.numpy(), rtol=1e-4, atol=1e-9)
    # the pair: rows [0, m) with label 1, rows [m, M) with label 0, each half with its own normaliser
    lg = logits.to(device).requires_grad_(True)
    ls, lt = ops.cka_bce_pair(lg, act.to(device), m, Cf)
    lc = logits.clone().requires_grad_(True)
    rs, rt = ref_loss(lc[:m], act[:m], 1.0), ref_loss(lc[m:], act[m:], 0.0)
    assert abs(ls.item() - rs.item()) < 1e-5 * abs(rs.item()) and abs(lt.item() - rt.item()) < 1e-5 * abs(rt.item())
    (ls + 2 * lt).backward()
    (rs + 2 * rt).backward()
    np.testing.assert_allclose(lg.grad.cpu().numpy(), lc.grad.numpy(), rtol=1e-4, atol=1e-9)


# ----------------------------------------------------------------------------- 8. full DA iteration at K = 8 / 21
@pytest.mark.parametrize("mode", ["fp32", "bf16x6"])
@pytest.mark.parametrize("K", [8, 21])
def test_step_other_class_counts_match_reference(device, gold_dir, K, mode):
    """the shape of test_step_s2c_matches_reference: procedural weights, synth inputs with the fixture's seeds, lr 0.
    K = 8: generic dynconv, Cf = 7 through the generic grouped conv, the fused cond-RNN.  K = 21: two class tiles,
    Cf = 20, the torch tier of the cond-RNN (K > 9)."""
    from scan_amd import engine, ops, synth
    name = "step_k%d_128x256" % K
    gold = json.load(open(os.path.join(gold_dir, name + ".json")))
    assert gold["num_classes"] == K and gold["transfer_cfg"] == ["NODES", "ADJ"]
    H, W, N = gold["H"], gold["W"], gold["N"]
    ops.CONV_MODE = mode
    try:
        model = engine.build_model(K, device=device, attn_dropout=0.0)
        engine.load_procedural_weights(model, K)
        trainer = engine.Trainer(model)
        for g in trainer.groups.values():
            g.lr = 0.0
        losses = trainer.step(synth.synth_images(N, H, W, gold["seeds"]["src"]).to(device),
                              synth.synth_targets(N, H, W, K - 1, 12, gold["seeds"]["boxes"]),
                              synth.synth_images(N, H, W, gold["seeds"]["tgt"]).to(device))
        torch.cuda.synchronize()
    finally:
        ops.CONV_MODE = "bf16x6"
    fails = []
    for k, ref in gold["losses"].items():
        v = float(losses[k])
        print("%s %s loss %s: %.8g ref %.8g rel %.2e" % (name, mode, k, v, ref, abs(v - ref) / max(abs(ref), 1e-30)))
        if ref == 0.0:
            assert v == 0.0
        elif not abs(v - ref) <= LOSS_RTOL * abs(ref):
            fails.append((k, v, ref))
    for mk, name_ in (("backbone", "body.features.28.weight"), ("fcos", "head.cls_logits.weight"),
                      ("middle_head", "head_out.middle_tower.0.weight"), ("dis_P3_CON", "classifier_cls_0.0.weight"),
                      ("dis_P4_CON", "dis_tower.0.weight")):
        ref = gold["grad_digest"][mk][name_]
        mine = _digest(dict(model[mk].named_parameters())[name_].grad)
        print("%s %s digest %s/%s: %.8g ref %.8g rel %.2e" % (name, mode, mk, name_, mine[1], ref[1],
                                                             abs(mine[1] - ref[1]) / ref[1]))
        if not abs(mine[1] - ref[1]) <= 5e-3 * ref[1]:
            fails.append((mk, name_, mine[1], ref[1]))
    assert not fails, (mode, fails)
    g = np.load(os.path.join(gold_dir, name + ".npz"))
    np.testing.assert_allclose(model["middle_head"].prototype.cpu().numpy(), g["prototype_after"], rtol=1e-4, atol=1e-4)


def test_model_construction_names_the_class_limit(device):
    from scan_amd import engine
    with pytest.raises(ValueError, match=r"2\.\.32"):
        engine.build_model(33, device=device)


# ----------------------------------------------------------------------------- 9. drop-in path
def test_dynamic_conv_softmax_layer_at_8_classes(device):
    """layers.dynamic_conv_softmax (the compiled operator when it is built) on NCHW input against F.conv2d + softmax"""
    from scan_amd import layers
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 256, 6, 10, generator=g)
    ker = torch.randn(8, 256, generator=g) / 16
    g1, g2 = torch.randn(2, 8, 6, 10, generator=g), torch.randn(2, 8, 6, 10, generator=g)
    xr, kr = x.clone().requires_grad_(True), ker.clone().requires_grad_(True)
    lr = F.conv2d(xr, kr[:, :, None, None])
    pr = lr.softmax(1)
    ((lr * g1).sum() + (pr * g2).sum()).backward()
    xd, kd = x.to(device).requires_grad_(True), ker.to(device).requires_grad_(True)
    l, p = layers.dynamic_conv_softmax(xd, kd)
    assert l.shape == (2, 8, 6, 10) and p.shape == (2, 8, 6, 10)
    ((l * g1.to(device)).sum() + (p * g2.to(device)).sum()).backward()
    _dynconv_check((l.detach(), p.detach(), xd.grad, kd.grad), (lr.detach(), pr.detach(), xr.grad, kr.grad))

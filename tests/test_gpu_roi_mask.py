"""Mask R-CNN mask head on the GPU: the positives compaction, the mask targets, the loss with its ordered twin and backward, the
test-time probabilities and the paste of csrc/roi_mask.hip against the reference's fixtures (tests/golden/roi_mask_*.npz) and the
fp64 / integer restatement (tests/roi_mask_ref.py); the convolutions at the head's 14 x 14 and 28 x 28 ROI images against fp64
F.conv2d / F.conv_transpose2d within the conv kernels' bounds (tests/conv3x3_ref.py, tests/conv1x1_ref.py); the modules of
modeling/roi_mask_head.py through CombinedROIHeads and factory.GeneralizedRCNN."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv1x1_ref as C1
import conv3x3_ref as C3
import roi_mask_ref as R
from roi_mask_ref import CASES, load_case

pytestmark = pytest.mark.gpu


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(scope="module")
def cases(gold_dir):
    """per fixture the stored arrays and the integer-rule targets of its positives, computed once"""
    out = {}
    for name in CASES:
        f = load_case(gold_dir, name)
        f["rule"] = R.targets_rule(f["masks_per_image"], f["pos_rois"], f["pos_gt"], f["M"])
        out[name] = f
    return out


# ----------------------------------------------------------------------------- 1. positives
def _positives(dev, labels, rois, src, matched, N, P, Rp):
    from scan_amd import ops
    out = ops.roi_mask_positives(_t(labels.astype(np.int32), dev), _t(rois.astype(np.float32), dev), _t(src.astype(np.int32), dev),
                                 _t(matched.astype(np.int32), dev), N, P, Rp)
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("name", CASES)
def test_positives_equal_nonzero_order_on_the_fixtures(device, cases, name):
    f = cases[name]
    rows, rois, lab, gt = _positives(device, f["sub_labels"], f["sub_rois"], f["sub_src"], f["matched"], f["N"], f["P"], f["Rp"])
    assert np.array_equal(rows, np.nonzero(f["sub_labels"] > 0)[0]) and np.array_equal(rows, f["pos_rows"])
    assert np.array_equal(rois, f["pos_rois"]) and np.array_equal(lab, f["pos_labels"]) and np.array_equal(gt, f["pos_gt"])
    assert rows.dtype == np.int32 and lab.dtype == np.int32 and gt.dtype == np.int32


@pytest.mark.parametrize("R_, kind", [(r, k) for r in (1, 257, 1025) for k in ("none", "one", "all", "some")])
def test_positives_synthetic_sizes(device, R_, kind):
    """Rp in {0, 1, R} and a random share; the outputs are guarded: nothing is written at or beyond row Rp"""
    from scan_amd import ops
    rs = np.random.RandomState(R_)
    N, P = 3, 40
    labels = {"none": np.zeros(R_, np.int32), "all": rs.randint(1, 81, R_).astype(np.int32),
              "one": np.eye(1, R_, R_ // 2, dtype=np.int32)[0] * 7,
              "some": np.where(rs.rand(R_) < 0.3, rs.randint(1, 81, R_), 0).astype(np.int32)}[kind]
    rois = np.concatenate([rs.randint(0, N, (R_, 1)), rs.uniform(0, 90, (R_, 4))], 1).astype(np.float32)
    src = rs.randint(0, P, R_).astype(np.int32)
    matched = rs.randint(0, 5, N * P).astype(np.int32)
    want = R.positives(labels, rois, src, matched, P)
    Rp = len(want[0])
    got = _positives(device, labels, rois, src, matched, N, P, Rp)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    if Rp >= 2:  # the library call on guarded buffers, Rp two rows short of the positives
        short, t = Rp - 2, [_t(a, device) for a in (labels, rois, src, matched)]
        bufs = [torch.full((Rp,), -7, dtype=torch.int32, device=device), torch.full((Rp, 5), -7.0, device=device),
                torch.full((Rp,), -7, dtype=torch.int32, device=device), torch.full((Rp,), -7, dtype=torch.int32, device=device)]
        ops.call("scan_roi_mask_positives", *[ops._ptr(a) for a in t], N, P, R_, short, *[ops._ptr(b) for b in bufs], ops._stream())
        for b, w in zip(bufs, want):
            b = b.cpu().numpy()
            assert (b[short:] == -7).all() and np.array_equal(b[:short], w[:short])


# ----------------------------------------------------------------------------- 2. targets
def _targets(dev, pos_rois, pos_gt, masks_per_image, M):
    from scan_amd import ops
    flat, moff, mhw = R.pack_masks(masks_per_image)
    return ops.roi_mask_targets(_t(pos_rois.astype(np.float32), dev), _t(pos_gt.astype(np.int32), dev), _t(flat, dev), _t(moff, dev),
                                _t(mhw, dev), M).cpu().numpy()


@pytest.mark.parametrize("name", CASES)
def test_targets_equal_the_rule_and_cover_the_references(device, cases, name):
    f = cases[name]
    got = _targets(device, f["pos_rois"], f["pos_gt"], f["masks_per_image"], f["M"])
    assert got.dtype == np.float32 and set(np.unique(got)) <= {0.0, 1.0}
    assert np.array_equal(got, f["rule"].astype(np.float32))
    ref = f["ref_targets"]
    assert (got >= ref).all() and int((got != ref).sum()) == int(f["n_rounding"])  # only the reference's rounding zeros differ
    assert (got[got != ref] == 1).all()


@pytest.mark.parametrize("M", [14, 28])
def test_targets_synthetic_crops(device, M):
    """images of different sizes back to back; a 1 x 1 crop, a crop of the whole image, all-ones and all-zeros masks, boxes
    beyond the image, .5 coordinates of both parities, an out-of-range ground-truth index (clamped) and image index (zeros)"""
    rs = np.random.RandomState(M)
    masks = [(rs.rand(3, 37, 53) < 0.6).astype(np.uint8), np.ones((1, 59, 20), np.uint8), np.zeros((2, 16, 16), np.uint8),
             (rs.rand(2, 64, 96) < 0.9).astype(np.uint8)]
    rois = np.array([[0, 10.2, 11.7, 10.4, 11.9], [0, 0, 0, 53, 37], [0, -5, -9, 80, 80], [0, 2.5, 3.5, 30.5, 31.5],
                     [1, 0, 0, 20, 59], [1, 3.2, 0.5, 19.5, 58.5], [1, 19.6, 58.7, 25, 70], [2, 1, 1, 14, 14],
                     [3, 0.4, 0.6, 95.5, 63.5], [3, 40.5, 20.5, 41.5, 21.5], [3, 12.3, 9.9, 70.1, 50.7], [0, 7.7, 5.1, 44.4, 30.9],
                     [3, 30, 50, 10, 20]], np.float32)
    gt = np.array([0, 2, 1, 1, 0, 0, 0, 1, 1, 0, 1, 2, 0], np.int32)
    want = R.targets_rule(masks, rois, gt, M)
    got = _targets(device, rois, gt, masks, M)
    assert np.array_equal(got, want.astype(np.float32))
    assert (got[4] == 1).all() and (got[5] == 1).all() and (got[7] == 0).all() and got[:4].any()
    # a ground-truth index past the image's masks is clamped, an image index out of range gives zeros
    odd_rois = rois[[0, 1, 1]].copy()
    odd_rois[1, 0], odd_rois[2, 0] = 4, -1
    odd = _targets(device, odd_rois, np.array([9, 0, 0], np.int32), masks, M)
    assert np.array_equal(odd[0], R.target_rule(masks[0][2], rois[0, 1:], M).astype(np.float32)) and (odd[1:] == 0).all()
    empty = _targets(device, np.zeros((0, 5), np.float32), np.zeros((0,), np.int32), masks, M)
    assert empty.shape == (0, M, M)


# ----------------------------------------------------------------------------- 3. loss
def _loss(dev, logits, labels, targets, cs=None):
    """logits [Rp, C, M, M] -> (loss, d logits [Rp, C, M, M], the gradient's padded columns) of ops.roi_mask_loss on the rows"""
    from scan_amd import ops
    Rp, C, M, _ = logits.shape
    rows = _t(R.logits_rows(logits, cs), dev).requires_grad_(True)
    loss = ops.roi_mask_loss(rows, _t(labels.astype(np.int32), dev), _t(targets.astype(np.float32), dev), C)
    loss.backward()
    g = rows.grad.cpu().numpy()
    return float(loss.detach()), g[:, :C].reshape(Rp, M, M, C).transpose(0, 3, 1, 2), g[:, C:]


def _check_loss(got, want_loss, want_d_label, labels):
    """the box head's bars (tests/test_gpu_roi_box.py: 1e-5 on a loss against fp64, rtol 1e-4 / atol 1e-7 on a gradient)"""
    loss, d, pad = got
    assert abs(loss - want_loss) <= 1e-5 * abs(want_loss)
    Rp = d.shape[0]
    assert np.allclose(d[np.arange(Rp), labels], want_d_label, rtol=1e-4, atol=1e-7)
    own = np.zeros(d.shape, bool)
    own[np.arange(Rp), labels] = True
    assert (d[~own] == 0).all() and (pad == 0).all()  # exact zeros in every other column, the padded ones included


@pytest.mark.parametrize("name", CASES)
def test_loss_on_the_references_targets_and_on_its_own(device, cases, name):
    from scan_amd import ops
    f = cases[name]
    Rp, C, M, lab = f["Rp"], f["C"], f["M"], f["pos_labels"]
    logits = R.make_logits(f["logit_seed"], Rp, C, M)
    x = logits[np.arange(Rp), lab]
    got = _loss(device, logits, lab, f["ref_targets"])
    want, wd = R.bce(x, f["ref_targets"])
    _check_loss(got, want, wd, lab)
    assert abs(got[0] - float(f["loss"])) <= 1e-4 * float(f["loss"])  # the box head's bar against the reference's fp32
    assert np.allclose(got[1][np.arange(Rp), lab], f["d_label"], rtol=1e-4, atol=1e-7)
    own = _loss(device, logits, lab, f["rule"], cs=C + 7 if C % 4 else C + 4)  # a wider pitch, its own targets
    _check_loss(own, *R.bce(x, f["rule"]), lab)
    # the ordered twin: bit-identical across two runs, within the same bar of the default
    prev = ops.set_deterministic(True)
    try:
        one, two = _loss(device, logits, lab, f["ref_targets"]), _loss(device, logits, lab, f["ref_targets"])
    finally:
        ops.set_deterministic(prev)
    assert np.float32(one[0]).tobytes() == np.float32(two[0]).tobytes() and one[1].tobytes() == two[1].tobytes()
    assert abs(one[0] - got[0]) <= 1e-5 * abs(got[0])
    _check_loss(one, want, wd, lab)
    # the library's one-launch entry on the same inputs, whichever of the two the wrapper chose for this size
    rows, out = _t(R.logits_rows(logits), device), torch.empty((1,), device=device)
    lab_d, tg_d = _t(lab.astype(np.int32), device), _t(f["ref_targets"].astype(np.float32), device)  # (held: the call takes pointers)
    ops.call("scan_roi_mask_loss_forward", ops._ptr(rows), rows.shape[1], Rp, M, C, ops._ptr(lab_d), ops._ptr(tg_d), ops._ptr(out),
             ops._stream())
    assert abs(float(out) / (Rp * M * M) - want) <= 1e-5 * want and abs(float(out) / (Rp * M * M) - one[0]) <= 1e-5 * one[0]


@pytest.mark.parametrize("M, entry", [(32, "scan_roi_mask_loss_forward"), (33, "scan_roi_mask_loss_forward_ordered")])
def test_loss_entry_on_either_side_of_the_one_launch_size(device, monkeypatch, M, entry):
    """8 ROIs of 32 x 32 are ops.ROI_MASK_LOSS_ONE_LAUNCH_ELEMS elements: the one-workgroup entry; of 33 x 33: slots + ordered sum"""
    from scan_amd import ops
    rs = np.random.RandomState(M)
    Rp, C = 8, 9
    assert (Rp * M * M <= ops.ROI_MASK_LOSS_ONE_LAUNCH_ELEMS) == (M == 32) and not ops.deterministic()
    logits = (rs.randn(Rp, C, M, M) * 2).astype(np.float32)
    labels, targets = rs.randint(1, C, Rp), (rs.rand(Rp, M, M) < 0.5).astype(np.float32)
    called = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (called.append(name), real(name, *a))[1])
    got = _loss(device, logits, labels, targets)
    assert called == [entry, "scan_roi_mask_loss_backward"]
    _check_loss(got, *R.bce(logits[np.arange(Rp), labels], targets), labels)


def test_ordered_twin_over_many_blocks_is_selected_by_deterministic(device, monkeypatch):
    from scan_amd import ops
    rs = np.random.RandomState(8)
    Rp, C, M = 400, 9, 28  # 313,600 elements: 154 blocks, the per-block slots matter
    rows = _t(rs.randn(Rp * M * M, 12).astype(np.float32) * 2, device)
    labels = _t(rs.randint(1, C, Rp).astype(np.int32), device)
    targets = _t((rs.rand(Rp, M, M) < 0.5).astype(np.float32), device)
    plain = float(ops.roi_mask_loss(rows, labels, targets, C))
    called = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (called.append(name), real(name, *a))[1])
    prev = ops.set_deterministic(True)
    try:
        one, two = ops.roi_mask_loss(rows, labels, targets, C), ops.roi_mask_loss(rows, labels, targets, C)
    finally:
        ops.set_deterministic(prev)
    assert called == ["scan_roi_mask_loss_forward_ordered"] * 2
    assert one.cpu().numpy().tobytes() == two.cpu().numpy().tobytes()
    x = rows.cpu().numpy().reshape(Rp, M, M, 12)[np.arange(Rp), :, :, labels.cpu().numpy()]
    want, _ = R.bce(x, targets.cpu().numpy())
    assert abs(float(one) - want) <= 1e-5 * want and abs(plain - want) <= 1e-5 * want


def test_loss_extreme_logits_and_no_positives(device):
    from scan_amd import ops
    rs = np.random.RandomState(4)
    Rp, C, M = 5, 9, 14
    logits = rs.choice([-80.0, 80.0, 0.0], size=(Rp, C, M, M)).astype(np.float32)
    labels = rs.randint(1, C, Rp)
    targets = (rs.rand(Rp, M, M) < 0.5).astype(np.float32)
    got = _loss(device, logits, labels, targets)
    assert np.isfinite(got[0]) and np.isfinite(got[1]).all()
    _check_loss(got, *R.bce(logits[np.arange(Rp), labels], targets), labels)
    for det in (False, True):
        prev = ops.set_deterministic(det)
        try:
            rows = torch.zeros((0, 12), device=device, requires_grad=True)
            loss = ops.roi_mask_loss(rows, torch.zeros((0,), dtype=torch.int32, device=device), torch.zeros((0, M, M), device=device), C)
            loss.backward()
        finally:
            ops.set_deterministic(prev)
        assert float(loss.detach()) == 0.0 and tuple(rows.grad.shape) == (0, 12)


# ----------------------------------------------------------------------------- 4. probabilities and paste
@pytest.mark.parametrize("name", CASES)
def test_probabilities_and_paste_equal_the_references(device, cases, name):
    from scan_amd import ops
    f = cases[name]
    K, C, M, H, W = f["K"], f["C"], f["M"], f["H"], f["W"]
    rows = _t(R.logits_rows(R.make_logits(f["inf_seed"], K, C, M, scale=3.0)), device)
    prob = ops.roi_mask_prob(rows, _t(f["det_label"], device), M, C)
    assert tuple(prob.shape) == (K, 1, M, M)
    assert np.allclose(prob.cpu().numpy(), f["ref_prob"], rtol=1e-5, atol=0)  # the box head's bar for scores
    k0 = 0
    for n, k in enumerate(f["det_count"]):
        out = ops.roi_mask_paste(prob[k0:k0 + k].contiguous(), _t(f["det_box"][k0:k0 + k], device), (H, W), float(f["thresh"]))
        assert out.dtype == torch.uint8 and tuple(out.shape) == (k, 1, H, W)
        assert np.array_equal(out.cpu().numpy()[:, 0], f["ref_paste"][k0:k0 + k]), (name, n)
        k0 += k


@pytest.mark.parametrize("H, W", [(20, 30), (21, 31)])
def test_paste_no_detection_one_pixel_and_far_boxes(device, H, W):
    """(21 x 31: 5 H W is no multiple of 4, so the last output bytes are not a whole 32-bit store)"""
    from scan_amd import ops
    M = 14
    empty = ops.roi_mask_paste(torch.zeros((0, 1, M, M), device=device), torch.zeros((0, 4), device=device), (H, W))
    assert tuple(empty.shape) == (0, 1, M, M)
    assert tuple(ops.roi_mask_prob(torch.zeros((0, 12), device=device), torch.zeros((0,), dtype=torch.int64, device=device), M, 9).shape) \
        == (0, 1, M, M)
    rs = np.random.RandomState(3)
    prob = rs.uniform(0.6, 1.0, (5, M, M)).astype(np.float32)
    boxes = np.array([[7.3, 9.2, 7.3, 9.2], [12.3, 4.4, 12.9, 4.8], [-90.2, -80.3, -60.7, -50.1], [100.3, 90.2, 140.6, 120.7],
                      [25.3, 15.2, 20.1, 10.6]], np.float32)  # a 1 x 1 box twice, beyond every side, an inverted box
    out = ops.roi_mask_paste(_t(prob[:, None], device), _t(boxes, device), (H, W)).cpu().numpy()[:, 0]
    want = np.stack([R.paste(prob[k].astype(np.float64), boxes[k], H, W)[0] for k in range(5)])
    assert np.array_equal(out, want)
    assert out[0].sum() == 1 and out[0, 9, 7] == 1 and out[1].sum() == 1 and not out[2:].any()


# ----------------------------------------------------------------------------- 5. the convolutions at ROI-sized images
def _mode():
    from scan_amd import ops
    return ops.CONV_MODE


def _ratios(got, ref, bounds):
    return {k: C1.worst_ratio(got[k], ref[k], bounds[k]) for k in ref}


@pytest.mark.parametrize("R_", [1, 5])
def test_conv3x3_on_14x14_roi_images(device, R_):
    """mask_fcn: 3x3, 256 -> 256 + ReLU on PyramidShape(R, [(14, 14)]) against fp64 F.conv2d: forward and input gradient within
    conv3x3_ref.bound_factor x the absolute-term sum of the kernel family that runs (Winograd in bf16x6 where the output has more
    than 64 channels), weight and bias gradient within conv1x1_ref.bound_factor over the R * 196 rows they reduce.  The bf16x6
    weight gradient transforms pairs of rows (Winograd F(2,3)): each transformed operand is a sum or difference of two values, so
    the sum of its absolute terms is at most twice sum |dy| |x| -- the factor 2 on that bound."""
    from scan_amd import ops
    mode, P, Cc = _mode(), 14, 256
    g = torch.Generator().manual_seed(R_)
    x = torch.randn(R_, Cc, P, P, generator=g)
    w = torch.randn(Cc, Cc, 3, 3, generator=g) * 0.03
    b = torch.randn(Cc, generator=g) * 0.1
    dy = torch.randn(R_, Cc, P, P, generator=g)
    shape = ops.PyramidShape(R_, [(P, P)])
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()
    xd = rows(x).to(device).requires_grad_(True)
    wd, bd = w.to(device).requires_grad_(True), b.to(device).requires_grad_(True)
    y = ops.conv2d(xd, wd, bd, shape, 3, 1, relu=True)
    x6, w6, b6 = (t.double().requires_grad_(True) for t in (x, w, b))
    pre = F.conv2d(x6, w6, b6, padding=1)
    dy = dy * (pre.detach().abs() > 1e-3)  # an output within 1e-3 of zero gets no gradient: a ReLU flipped by rounding cannot enter
    y.backward(rows(dy.float()).to(device))
    F.relu(pre).backward(dy)
    dye = (dy * (pre.detach() > 0)).numpy()
    xh, wh, bh = rows(x).numpy(), w.numpy(), b.numpy()
    dyh = dye.transpose(0, 2, 3, 1).reshape(-1, Cc)
    d3 = C3.Shape(R_, [(P, P)])
    wino = mode == "bf16x6"
    Sy = C3.forward_abs_wino(xh, wh, bh, d3) if wino else C3.forward_abs(xh, wh, bh, d3)
    Sdx = (C3.forward_abs_wino if wino else C3.forward_abs)(dyh, C3.dgrad_weight(wh), None, d3)
    Sdw, Sdb = C3.wgrad(np.abs(xh).astype(np.float64), np.abs(dyh), d3)
    fam = "wino" if wino else "direct"
    n = R_ * P * P
    got = {"y": y.detach().cpu().numpy(), "dx": xd.grad.cpu().numpy(), "dw": wd.grad.cpu().numpy(), "db": bd.grad.cpu().numpy()}
    ref = {"y": rows(F.relu(pre).detach()).numpy(), "dx": rows(x6.grad).numpy(), "dw": w6.grad.numpy(), "db": b6.grad.numpy()}
    bounds = {"y": C3.bound_factor(mode, Cc, fam) * Sy, "dx": C3.bound_factor(mode, Cc, fam) * Sdx,
              "dw": (2.0 if wino else 1.0) * C1.bound_factor(mode, n) * Sdw, "db": C1.bound_factor(mode, n, colsum=True) * Sdb}
    ratios = _ratios(got, ref, bounds)
    print("mask_fcn 3x3 R=%d %s: %s" % (R_, mode, {k: "%.2e" % v for k, v in ratios.items()}))
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("R_, cout", [(1, 256), (5, 256), (1, 9), (5, 9)])
def test_conv5_mask_and_logits_convs(device, R_, cout):
    """MaskRCNNC4Predictor: the transposed conv as a 4 D-column 1x1 conv + shuffle against fp64 F.conv_transpose2d + ReLU, then the
    logits conv on [(28, 28)] against fp64 F.conv2d; every result within conv1x1_ref.bound_factor x its absolute-term sum
    (cout = 256: the two layers one by one at 256 -> 256; cout = 9: the logits conv at 256 -> 9)"""
    from scan_amd import ops
    from scan_amd.modeling import roi_mask_head as rm
    mode, P, Cc = _mode(), 14, 256
    torch.manual_seed(R_ * 10 + cout)
    pr = rm.MaskRCNNC4Predictor(Cc, Cc, cout).to(device)
    pr.conv5_mask.weight.data.normal_(0, 0.05)
    pr.conv5_mask.bias.data.normal_(0, 0.1)
    pr.mask_fcn_logits.weight.data.normal_(0, 0.05)
    pr.mask_fcn_logits.bias.data.normal_(0, 0.1)
    g = torch.Generator().manual_seed(R_)
    x = torch.randn(R_, Cc, P, P, generator=g)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()
    shape = ops.PyramidShape(R_, [(P, P)])
    # ---- conv5_mask
    xd = rows(x).to(device).requires_grad_(True)
    up, ushape = pr.upsampled(xd, shape)
    assert ushape == ops.PyramidShape(R_, [(2 * P, 2 * P)]) and tuple(up.shape) == (R_ * 4 * P * P, Cc)
    w5, b5 = pr.conv5_mask.weight.detach().cpu(), pr.conv5_mask.bias.detach().cpu()
    x6, w6, b6 = (t.double().requires_grad_(True) for t in (x, w5, b5))
    pre = F.conv_transpose2d(x6, w6, b6, stride=2)
    dy = torch.randn(R_, Cc, 2 * P, 2 * P, generator=g).double() * (pre.detach().abs() > 1e-3)
    up.backward(rows(dy.float()).to(device))
    F.relu(pre).backward(dy)
    dye = dy * (pre.detach() > 0)
    ax, aw, ady = x.double().abs(), w5.double().abs(), dye.abs()
    n_out = R_ * 4 * P * P
    got = {"y": up.detach().cpu().numpy(), "dx": xd.grad.cpu().numpy(), "dw": pr.conv5_mask.weight.grad.cpu().numpy(),
           "db": pr.conv5_mask.bias.grad.cpu().numpy()}
    ref = {"y": rows(F.relu(pre).detach()).numpy(), "dx": rows(x6.grad).numpy(), "dw": w6.grad.numpy(), "db": b6.grad.numpy()}
    bounds = {"y": C1.bound_factor(mode, Cc) * rows(F.conv_transpose2d(ax, aw, b5.double().abs(), stride=2)).numpy(),
              "dx": C1.bound_factor(mode, 4 * Cc) * rows(F.conv2d(ady, aw, stride=2)).numpy(),
              # dw[c, d, kh, kw] sums R P P products, db[d] sums the 4 R P P values of dy's channel d (the bias is repeated)
              "dw": C1.bound_factor(mode, R_ * P * P) * torch.einsum("ncyx,ndykxl->cdkl", ax, ady.reshape(R_, Cc, P, 2, P, 2)).numpy(),
              "db": C1.bound_factor(mode, n_out, colsum=True) * ady.sum((0, 2, 3)).numpy()}
    r5 = _ratios(got, ref, bounds)
    # ---- mask_fcn_logits on the 28 x 28 rows
    u = torch.randn(R_, Cc, 2 * P, 2 * P, generator=g)
    ud = rows(u).to(device).requires_grad_(True)
    pr.zero_grad()
    lg = pr.logits(ud, ushape)
    assert tuple(lg.shape) == (n_out, ops.pad4(cout)) and (cout % 4 == 0 or float(lg[:, cout:].abs().max()) == 0)
    wl, bl = pr.mask_fcn_logits.weight.detach().cpu(), pr.mask_fcn_logits.bias.detach().cpu()
    u6, wl6, bl6 = (t.double().requires_grad_(True) for t in (u, wl, bl))
    dl = torch.randn(R_, cout, 2 * P, 2 * P, generator=g).double()
    lg[:, :cout].backward(rows(dl.float()).to(device))
    out6 = F.conv2d(u6, wl6, bl6)
    out6.backward(dl)
    au, awl, adl = rows(u).double().abs(), wl.double().abs().reshape(cout, Cc), rows(dl).abs()
    got = {"y": lg[:, :cout].detach().cpu().numpy(), "dx": ud.grad.cpu().numpy(),
           "dw": pr.mask_fcn_logits.weight.grad.cpu().numpy().reshape(cout, Cc), "db": pr.mask_fcn_logits.bias.grad.cpu().numpy()}
    ref = {"y": rows(out6.detach()).numpy(), "dx": rows(u6.grad).numpy(), "dw": wl6.grad.numpy().reshape(cout, Cc), "db": bl6.grad.numpy()}
    bounds = {"y": C1.bound_factor(mode, Cc) * (au @ awl.t() + bl.double().abs()).numpy(), "dx": C1.bound_factor(mode, cout) * (adl @ awl).numpy(),
              "dw": C1.bound_factor(mode, n_out) * (adl.t() @ au).numpy(), "db": C1.bound_factor(mode, n_out, colsum=True) * adl.sum(0).numpy()}
    rl = _ratios(got, ref, bounds)
    print("conv5_mask R=%d %s: %s; mask_fcn_logits -> %d: %s" % (R_, mode, {k: "%.2e" % v for k, v in r5.items()}, cout,
                                                               {k: "%.2e" % v for k, v in rl.items()}))
    assert max(r5.values()) <= 1.0 and max(rl.values()) <= 1.0, (r5, rl)


# ----------------------------------------------------------------------------- 6. modules
def _proposal_lists(f, dev):
    from scan_amd.structures import BoxList
    return [BoxList(_t(f["props"][n, :int(f["np"][n])].copy(), dev), (f["W"], f["H"]), mode="xyxy") for n in range(f["N"])]


def _targets_with_masks(f):
    from scan_amd.structures import BoxList, SegmentationMask
    out = []
    for n in range(f["N"]):
        k = int(f["ng"][n])
        t = BoxList(torch.from_numpy(f["boxes"][n, :k].copy()), (f["W"], f["H"]), mode="xyxy")
        t.add_field("labels", torch.from_numpy(f["glabels"][n, :k].copy()))
        t.add_field("masks", SegmentationMask(torch.from_numpy(f["masks_per_image"][n].copy()), (f["W"], f["H"]), mode="mask"))
        out.append(t)
    return out


def _heads(f, dev, postprocess=False):
    from scan_amd.modeling import roi_box_head as rb, roi_mask_head as rm
    P = f["M"] // 2 if f["predictor"] == "MaskRCNNC4Predictor" else f["M"]
    box = rb.ROIBoxHead(dict(rb.DEFAULT_SETTINGS, num_classes=f["C"], mlp_head_dim=32, pooler_resolution=3,
                             bg_iou_threshold=float(f["bg"]), fg_iou_threshold=float(f["fg"]),
                             batch_size_per_image=int(f["batch_size_per_image"]), positive_fraction=float(f["positive_fraction"])),
                        in_channels=8)
    mask = rm.ROIMaskHead(dict(rm.DEFAULT_SETTINGS, num_classes=f["C"], predictor=f["predictor"], pooler_resolution=P,
                               resolution=f["M"], conv_layers=(8, 8), bg_iou_threshold=float(f["bg"]),
                               fg_iou_threshold=float(f["fg"]), postprocess_masks=postprocess,
                               postprocess_masks_threshold=float(f["thresh"])), in_channels=8)
    return rb.CombinedROIHeads({"box": box, "mask": mask}).to(dev)


def _features(f, dev, grad=False):
    return [torch.randn(f["N"], 8, -(-f["H"] // s), -(-f["W"] // s), device=dev, requires_grad=grad) for s in (8, 16, 32, 64, 128)]


@pytest.mark.parametrize("name", CASES[:2])
def test_mask_head_training_step_through_the_combined_heads(device, cases, name):
    """fed the reference's draw: the plan's positives and targets are the fixture's, loss_mask equals the fp64 restatement on the
    device targets, and the mask head adds two launches and no host read to the box head's plan"""
    from scan_amd.modeling import roi_box_head as rb, roi_mask_head as rm
    f = cases[name]
    torch.manual_seed(0)
    heads = _heads(f, device).train()
    feats = _features(f, device, grad=True)
    sampled = torch.from_numpy(f["sampled"].reshape(f["N"], f["P"]))
    rm.plan_stats.update(launches=-1, host_reads=-1)
    x, props, losses = heads(feats, _proposal_lists(f, device), _targets_with_masks(f), sampled=sampled)
    assert rb.plan_stats == {"launches": 2, "host_reads": 1} and rm.plan_stats == {"launches": 2, "host_reads": 0}
    assert sorted(losses) == ["loss_box_reg", "loss_classifier", "loss_mask"] and all(torch.isfinite(v) for v in losses.values())
    le = heads.mask.loss_evaluator
    assert np.array_equal(le.pos_rows.cpu().numpy(), f["pos_rows"]) and np.array_equal(le.pos_rois.cpu().numpy(), f["pos_rois"])
    assert np.array_equal(le.pos_labels.cpu().numpy(), f["pos_labels"]) and np.array_equal(le.pos_gt.cpu().numpy(), f["pos_gt"])
    assert np.array_equal(le.targets.cpu().numpy(), f["rule"].astype(np.float32))
    assert [len(p) for p in props] == f["sub_count"].tolist()  # the proposals come back as the box head sampled them
    P = heads.mask.feature_extractor.resolution
    assert tuple(x.shape) == (f["Rp"], 8, P, P)
    sum(losses.values()).backward()
    for k, p in heads.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    assert feats[0].grad is not None
    # the loss on given logits rows equals the restatement on the device targets
    logits = R.make_logits(f["logit_seed"], f["Rp"], f["C"], f["M"])
    got = float(le(_t(R.logits_rows(logits), device), f["C"]))
    want, _ = R.bce(logits[np.arange(f["Rp"]), f["pos_labels"]], f["rule"])
    assert abs(got - want) <= 1e-5 * want
    # called on its own with the box head's subsampled proposals: the same plan, one launch and one host read more
    x2, props2, l2 = heads.mask(feats, props, _targets_with_masks(f))
    assert rm.plan_stats == {"launches": 3, "host_reads": 1} and props2 is props
    assert np.array_equal(le.pos_gt.cpu().numpy(), f["pos_gt"]) and np.array_equal(le.targets.cpu().numpy(), f["rule"].astype(np.float32))
    assert float(l2["loss_mask"]) == float(losses["loss_mask"])


def test_mask_head_without_positives(device, cases):
    f = cases["roi_mask_64x96"]
    torch.manual_seed(0)
    heads = _heads(f, device).train()
    feats = _features(f, device, grad=True)
    sampled = torch.from_numpy(np.where(f["sampled"] == 1, 0, f["sampled"]).reshape(f["N"], f["P"]))  # the negatives alone
    x, props, losses = heads(feats, _proposal_lists(f, device), _targets_with_masks(f), sampled=sampled)
    assert float(losses["loss_mask"]) == 0.0 and x.shape[0] == 0
    sum(losses.values()).backward()
    g = heads.mask.predictor.mask_fcn_logits.weight.grad
    assert g is not None and float(g.abs().max()) == 0.0


@pytest.mark.parametrize("name", [CASES[0], CASES[1]])
@pytest.mark.parametrize("postprocess", [False, True])
def test_mask_head_eval_step(device, cases, name, postprocess):
    """detections with a ``mask`` field of the reference's shape; with the predictor's logits replaced by the fixture's, the
    reference's probabilities and pasted masks"""
    from scan_amd.structures import BoxList
    f = cases[name]
    torch.manual_seed(0)
    head = _heads(f, device, postprocess).mask.eval()
    K, C, M, H, W = f["K"], f["C"], f["M"], f["H"], f["W"]
    dets, k0 = [], 0
    for k in f["det_count"]:
        d = BoxList(_t(f["det_box"][k0:k0 + k], device), (W, H), mode="xyxy")
        d.add_field("labels", _t(f["det_label"][k0:k0 + k], device))
        d.add_field("scores", torch.ones(int(k), device=device))
        dets.append(d)
        k0 += k
    dets.append(BoxList(torch.zeros((0, 4), device=device), (W, H), mode="xyxy"))  # an image without detections
    dets[-1].add_field("labels", torch.zeros((0,), dtype=torch.int64, device=device))
    dets[-1].add_field("scores", torch.zeros((0,), device=device))
    feats = [torch.randn(len(dets), 8, -(-H // s), -(-W // s), device=device) for s in (8, 16, 32, 64, 128)]
    x, res, losses = head(feats, dets)
    assert losses == {} and len(res) == len(dets) and x.shape[0] == K
    for d, r in zip(dets, res):
        want = (len(d), 1, H, W) if postprocess and len(d) else (len(d), 1, M, M)
        assert tuple(r.get_field("mask").shape) == want and r.get_field("mask").dtype == (torch.uint8 if postprocess and len(d) else torch.float32)
        assert r.has_field("scores") and torch.equal(r.bbox, d.bbox)
    rows = _t(R.logits_rows(R.make_logits(f["inf_seed"], K, C, M, scale=3.0)), device)
    res = head.post_processor(rows, dets[:-1])
    got = torch.cat([r.get_field("mask") for r in res]).cpu().numpy()
    if postprocess:
        assert np.array_equal(got[:, 0], f["ref_paste"])
    else:
        assert np.allclose(got, f["ref_prob"], rtol=1e-5, atol=0)
    none = head(feats[:1] + feats[1:], [dets[-1]] * len(dets))[1]  # no detection in any image
    assert all(tuple(r.get_field("mask").shape) == (0, 1, M, M) for r in none)


def test_reference_state_dict_loads_and_generalized_rcnn_trains_with_masks(device, gold_dir):
    from scan_amd import config
    from scan_amd.modeling import factory, roi_mask_head as rm
    from scan_amd.structures import BoxList, SegmentationMask
    with open(os.path.join(gold_dir, "roi_mask_keys.json")) as fh:
        ref = json.load(fh)["state_dict"]
    for pred, res in (("MaskRCNNC4Predictor", 28), ("MaskRCNNConv1x1Predictor", 14)):
        head = rm.ROIMaskHead(dict(rm.DEFAULT_SETTINGS, predictor=pred, resolution=res)).to(device)
        state = {k: torch.full(s, 0.5) for k, s in ref[pred].items()}  # what torch.save of the reference's head holds: key -> tensor
        head.load_state_dict(state, strict=True)
        assert all(float(p.min()) == 0.5 for p in head.parameters())
    cfg = config.load("c2f", ["MODEL.FCOS_ON", False, "MODEL.RPN_ONLY", False, "MODEL.ATSS_ON", False, "MODEL.RETINANET_ON", False,
                              "MODEL.MIDDLE_HEAD.CONDGRAPH_ON", False, "MODEL.BACKBONE.CONV_BODY", "VGG-16-FPN-RETINANET",
                              "MODEL.RPN.USE_FPN", True, "MODEL.RPN.BATCH_SIZE_PER_IMAGE", 32, "MODEL.RPN.PRE_NMS_TOP_N_TRAIN", 60,
                              "MODEL.RPN.POST_NMS_TOP_N_TRAIN", 40, "MODEL.RPN.FPN_POST_NMS_TOP_N_TRAIN", 60,
                              "MODEL.RPN.PRE_NMS_TOP_N_TEST", 60, "MODEL.RPN.POST_NMS_TOP_N_TEST", 40,
                              "MODEL.RPN.FPN_POST_NMS_TOP_N_TEST", 30,
                              "MODEL.ROI_HEADS.USE_FPN", True, "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", 16,
                              "MODEL.ROI_HEADS.DETECTIONS_PER_IMG", 10,
                              "MODEL.ROI_BOX_HEAD.FEATURE_EXTRACTOR", "FPN2MLPFeatureExtractor",
                              "MODEL.ROI_BOX_HEAD.PREDICTOR", "FPNPredictor", "MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION", 3,
                              "MODEL.ROI_BOX_HEAD.POOLER_SCALES", (0.125, 0.0625, 0.03125, 0.015625),
                              "MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO", 2, "MODEL.ROI_BOX_HEAD.NUM_CLASSES", 9,
                              "MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM", 64, "MODEL.MASK_ON", True,
                              "MODEL.ROI_MASK_HEAD.FEATURE_EXTRACTOR", "MaskRCNNFPNFeatureExtractor",
                              "MODEL.ROI_MASK_HEAD.PREDICTOR", "MaskRCNNC4Predictor", "MODEL.ROI_MASK_HEAD.POOLER_RESOLUTION", 4,
                              "MODEL.ROI_MASK_HEAD.POOLER_SCALES", (0.125, 0.0625, 0.03125, 0.015625),
                              "MODEL.ROI_MASK_HEAD.POOLER_SAMPLING_RATIO", 2, "MODEL.ROI_MASK_HEAD.RESOLUTION", 8,
                              "MODEL.ROI_MASK_HEAD.CONV_LAYERS", (32, 32), "MODEL.ROI_MASK_HEAD.SHARE_BOX_FEATURE_EXTRACTOR", False,
                              "MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS", True])
    torch.manual_seed(0)
    model = factory.build_detection_model(cfg).to(device).train()
    assert any(k.startswith("roi_heads.mask.predictor.conv5_mask") for k in model.state_dict())
    images = torch.randn(2, 3, 64, 96, device=device)
    targets = []
    for b, l in (([[6.3, 5.2, 40.6, 37.7], [48.4, 8.6, 88.3, 44.8]], [3, 8]), ([[30.4, 12.3, 70.7, 50.2]], [5])):
        t = BoxList(torch.tensor(b), (96, 64), mode="xyxy")
        t.add_field("labels", torch.tensor(l))
        m = torch.zeros((len(b), 64, 96), dtype=torch.uint8)
        for g, (x0, y0, x1, y1) in enumerate(b):
            m[g, int(y0) + 3:int(y1) - 2, int(x0) + 4:int(x1) - 3] = 1
        t.add_field("masks", SegmentationMask(m, (96, 64), mode="mask"))
        targets.append(t)
    losses = model(images, targets)
    assert sorted(losses) == ["loss_box_reg", "loss_classifier", "loss_mask", "loss_objectness", "loss_rpn_box_reg"]
    assert all(torch.isfinite(v) for v in losses.values())
    sum(losses.values()).backward()
    missing = [k for k, p in model.named_parameters() if p.requires_grad and p.grad is None]
    assert not missing, missing
    model.eval()
    with torch.no_grad():
        dets = model(images)
    assert len(dets) == 2
    for d in dets:
        assert d.has_field("mask") and tuple(d.get_field("mask").shape[1:]) in ((1, 64, 96), (1, 8, 8))

"""GPU parity tests of the individual HIP kernels, called through the C ABI (scan_amd.ops /
scan_amd._C -> ctypes -> libscan_hip.so), against the CPU oracle (oracle/) and the golden vectors
captured from the reference (tests/golden/, oracle/make_golden.py)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu


def _rows(x_nchw, dev, cs=None):
    from scan_amd import ops
    r, s = ops.nchw_to_rows(x_nchw.to(dev), cs)
    return r, s


def _pyr(levels, dev, cs=None):
    """list of NCHW CPU tensors -> (rows on GPU, PyramidShape)"""
    from scan_amd import ops
    rows, sizes = [], []
    for x in levels:
        r, s = ops.nchw_to_rows(x.to(dev), cs)
        rows.append(r)
        sizes.append(s.sizes[0])
    return torch.cat(rows, 0).contiguous(), ops.PyramidShape(levels[0].shape[0], sizes)


def _unrows(rows, shape, c):
    from scan_amd import ops
    return [ops.rows_to_nchw(rows.detach(), shape, l, c).contiguous().cpu() for l in range(shape.n_levels)]


# ----------------------------------------------------------------------------- loader
def test_library_loaded(device):
    from scan_amd import _lib
    assert _lib.lib().scan_abi_version() == 1
    assert os.path.basename(_lib.LIB_PATH) == "libscan_hip.so"


# ----------------------------------------------------------------------------- pointwise vs golden
def test_sigmoid_focal_golden(device, gold_dir):
    from scan_amd import _C
    from oracle import coracle
    g = np.load(os.path.join(gold_dir, "pointwise.npz"))
    x = torch.from_numpy(g["focal_logits"]).to(device)
    t = torch.from_numpy(g["focal_targets"]).to(device)
    l = _C.sigmoid_focalloss_forward(x, t, 8, 2.0, 0.25).cpu().numpy()
    # reference CPU formula (unstable tail) vs the CUDA formula we follow: SURVEY 8c numerics caveat
    np.testing.assert_allclose(l, g["focal_loss"], rtol=2e-4, atol=1e-4)
    np.testing.assert_allclose(l, coracle.sigmoid_focal_fwd(g["focal_logits"], g["focal_targets"], 2.0, 0.25),
                               rtol=1e-5, atol=1e-7)
    d = _C.sigmoid_focalloss_backward(x, t, torch.from_numpy(g["focal_dloss"]).to(device), 8, 2.0, 0.25).cpu().numpy()
    np.testing.assert_allclose(d, g["focal_dlogits"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(d, coracle.sigmoid_focal_bwd(g["focal_logits"], g["focal_targets"], g["focal_dloss"],
                                                            2.0, 0.25), rtol=1e-5, atol=1e-7)


def test_sigmoid_focal_layer_sum_and_tail(device):
    from scan_amd.layers import SigmoidFocalLoss
    from oracle import coracle
    rs = np.random.RandomState(0)
    for M, C in ((1, 8), (1000, 8), (4097, 1), (333, 3)):
        x = (rs.randn(M, C) * 8).astype(np.float32)  # includes |x| > 17 where the reference CPU formula overflows
        t = rs.randint(-1, C + 1, M).astype(np.int32)
        xt = torch.from_numpy(x).to(device).requires_grad_(True)
        loss = SigmoidFocalLoss(2.0, 0.25)(xt, torch.from_numpy(t).to(device))
        ref = coracle.sigmoid_focal_fwd(x, t, 2.0, 0.25).astype(np.float64).sum()
        assert abs(loss.item() - ref) <= 1e-4 * max(1.0, abs(ref))
        (loss * 0.5).backward()
        gref = coracle.sigmoid_focal_bwd(x, t, np.full((M, C), 0.5, np.float32), 2.0, 0.25)
        np.testing.assert_allclose(xt.grad.cpu().numpy(), gref, rtol=1e-5, atol=1e-7)
    with pytest.raises(RuntimeError):
        from scan_amd import _C
        _C.sigmoid_focalloss_forward(torch.zeros(4, 3, device=device), torch.zeros(4, dtype=torch.int32, device=device),
                                     8, 2.0, 0.25)
    with pytest.raises(RuntimeError):
        _C.sigmoid_focalloss_forward(torch.zeros(4, 8), torch.zeros(4, dtype=torch.int32), 8, 2.0, 0.25)


def test_compiled_fcos_core_C_runs_the_reference_call_sequences(device, gold_dir):
    """the module built from scan_amd/csrc/fcos_core_C.cpp, imported under the reference's name ``fcos_core._C``, driven the
    way the reference drives it: layers/nms.py:4-7 (``nms = _C.nms``), the ``_SigmoidFocalLoss`` autograd Function of
    layers/sigmoid_focal_loss.py:9-36 (forward: _C.sigmoid_focalloss_forward, backward: _C.sigmoid_focalloss_backward) and
    its module's ``loss.sum()`` (:56-70) -- against the reference's own test vectors, the C oracle, and the ctypes binding."""
    import importlib
    import sys
    ext = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scan_amd", "ext")
    if ext not in sys.path:
        sys.path.insert(0, ext)
    _C = importlib.import_module("fcos_core._C")
    from scan_amd import _C as ctypes_C
    from oracle import coracle

    class _SigmoidFocalLoss(torch.autograd.Function):  # the reference's Function, verbatim in structure
        @staticmethod
        def forward(ctx, logits, targets, gamma, alpha):
            ctx.save_for_backward(logits, targets)
            ctx.num_classes, ctx.gamma, ctx.alpha = logits.shape[1], gamma, alpha
            return _C.sigmoid_focalloss_forward(logits, targets, ctx.num_classes, gamma, alpha)

        @staticmethod
        def backward(ctx, d_loss):
            logits, targets = ctx.saved_tensors
            return _C.sigmoid_focalloss_backward(logits, targets, d_loss.contiguous(), ctx.num_classes, ctx.gamma,
                                                 ctx.alpha), None, None, None

    g = np.load(os.path.join(gold_dir, "pointwise.npz"))
    x = torch.from_numpy(g["focal_logits"]).to(device).requires_grad_(True)
    t = torch.from_numpy(g["focal_targets"]).to(device)
    loss = _SigmoidFocalLoss.apply(x, t.int(), 2.0, 0.25)
    np.testing.assert_allclose(loss.detach().cpu().numpy(), coracle.sigmoid_focal_fwd(g["focal_logits"], g["focal_targets"], 2.0, 0.25),
                               rtol=1e-5, atol=1e-7)
    loss.sum().backward()
    ones = np.ones_like(g["focal_logits"])
    np.testing.assert_allclose(x.grad.cpu().numpy(), coracle.sigmoid_focal_bwd(g["focal_logits"], g["focal_targets"], ones, 2.0, 0.25),
                               rtol=1e-5, atol=1e-7)
    assert torch.equal(loss.detach(), ctypes_C.sigmoid_focalloss_forward(x.detach(), t, 8, 2.0, 0.25))
    # nms: the reference's own known answers (tests/test_nms.py) and random boxes against the oracle, ml_nms likewise
    kat = json.load(open(os.path.join(gold_dir, "nms_kat.json")))
    for case in kat["cases"]:
        keep = _C.nms(torch.tensor(case["boxes"], device=device), torch.tensor(case["scores"], device=device), case["thresh"])
        assert sorted(keep.cpu().tolist()) == case["keep_sorted"]
    rs = np.random.RandomState(3)
    boxes, scores = _rand_boxes(rs, 3000, quant=4.0), rs.rand(3000).astype(np.float32)
    labels = rs.randint(1, 9, 3000).astype(np.float32)
    bd, sd, ld = (torch.from_numpy(a).to(device) for a in (boxes, scores, labels))
    assert np.array_equal(_C.nms(bd, sd, 0.5).cpu().numpy(), coracle.nms(boxes, scores, 0.5))
    assert np.array_equal(_C.ml_nms(bd, sd, ld, 0.6).cpu().numpy(), coracle.ml_nms(boxes, scores, labels, 0.6))
    assert torch.equal(_C.ml_nms(bd, sd, ld, 0.6), ctypes_C.ml_nms(bd, sd, ld, 0.6))
    with pytest.raises(RuntimeError, match="num_classes"):
        _C.sigmoid_focalloss_forward(torch.zeros(4, 3, device=device), torch.zeros(4, dtype=torch.int32, device=device), 8, 2.0, 0.25)
    # the '>' rule of the reference's GPU build (csrc/cuda/nms.cu:60) through the module: argument and environment
    one = np.ones(3000, np.float32)
    assert np.array_equal(_C.nms(bd, sd, 0.5, cuda_rule=True).cpu().numpy(), coracle.ml_nms(boxes, scores, one, 0.5))
    assert torch.equal(_C.nms(bd, sd, 0.5, cuda_rule=True), ctypes_C.nms(bd, sd, 0.5, cuda_rule=True))
    # CPU tensors take the module's host loop (csrc/nms.h:26): same keep list as the device path
    assert np.array_equal(_C.nms(bd.cpu(), sd.cpu(), 0.5).numpy(), _C.nms(bd, sd, 0.5).cpu().numpy())
    with pytest.raises(RuntimeError, match="SCAN_NMS_MAX"):
        _C.nms(torch.zeros(262145, 4, device=device), torch.zeros(262145, device=device), 0.5)


def test_iou_loss_golden(device, gold_dir):
    from scan_amd.layers import IOULoss
    g = np.load(os.path.join(gold_dir, "pointwise.npz"))
    p = torch.from_numpy(g["iou_pred"]).to(device).requires_grad_(True)
    l = IOULoss()(p, torch.from_numpy(g["iou_target"]).to(device), torch.from_numpy(g["iou_weight"]).to(device))
    assert abs(l.item() - float(g["iou_loss"])) <= 1e-5 * abs(float(g["iou_loss"]))
    l.backward()
    np.testing.assert_allclose(p.grad.cpu().numpy(), g["iou_dpred"], rtol=1e-4, atol=1e-7)
    # unweighted mean
    p2 = torch.from_numpy(g["iou_pred"]).to(device)
    l2 = IOULoss()(p2, torch.from_numpy(g["iou_target"]).to(device))
    from oracle import coracle
    v, _ = coracle.iou_loss(g["iou_pred"], g["iou_target"], None)
    assert abs(l2.item() - v) <= 1e-5 * abs(v)


def test_softmax_focal_golden(device, gold_dir):
    from scan_amd.layers import FocalLoss
    g = np.load(os.path.join(gold_dir, "pointwise.npz"))
    z = torch.from_numpy(g["sfl_logits"]).to(device).requires_grad_(True)
    l = FocalLoss(9)(z, torch.from_numpy(g["sfl_labels"]).to(device))
    assert abs(l.item() - float(g["sfl_loss"])) <= 1e-5 * abs(float(g["sfl_loss"]))
    l.backward()
    np.testing.assert_allclose(z.grad.cpu().numpy(), g["sfl_dlogits"], rtol=1e-4, atol=1e-8)


def test_grl_golden(device, gold_dir):
    from scan_amd.layers import GradientReversal
    g = np.load(os.path.join(gold_dir, "pointwise.npz"))
    x = torch.from_numpy(g["grl_x"]).to(device).requires_grad_(True)
    y = GradientReversal(0.02)(x)
    assert torch.equal(y.cpu(), torch.from_numpy(g["grl_y"]))
    y.backward(torch.from_numpy(g["grl_gy"]).to(device))
    np.testing.assert_allclose(x.grad.cpu().numpy(), g["grl_gx"], rtol=1e-6, atol=0)


def test_bce_and_cka(device):
    from scan_amd import ops
    torch.manual_seed(3)
    M, Cf = 777, 8
    x = torch.randn(M) * 3
    t = torch.rand(M)
    xg = x.to(device).requires_grad_(True)
    l = ops.bce_with_logits_mean(xg, t.to(device))
    xr = x.clone().requires_grad_(True)
    lr = F.binary_cross_entropy_with_logits(xr, t)
    assert abs(l.item() - lr.item()) < 1e-6 * max(1, abs(lr.item()))
    l.backward()
    lr.backward()
    np.testing.assert_allclose(xg.grad.cpu().numpy(), xr.grad.numpy(), rtol=1e-5, atol=1e-9)
    # CKA: per-class act-weighted BCE (reference fcos_head_discriminator_con.py:105-124)
    logits = torch.randn(M, Cf) * 2
    act = torch.softmax(torch.randn(M, Cf + 1), 1)
    for target in (0.0, 1.0):
        lg = logits.to(device).requires_grad_(True)
        l = ops.cka_bce(lg, act.to(device), target, Cf)
        lc = logits.clone().requires_grad_(True)
        ref = 0
        for c in range(Cf):
            a = act[:, c + 1]
            ref = ref + F.binary_cross_entropy_with_logits(lc[:, c], torch.full((M,), target), weight=a,
                                                           reduction="sum") / a.sum() / Cf
        assert abs(l.item() - ref.item()) < 1e-5 * abs(ref.item())
        l.backward()
        ref.backward()
        np.testing.assert_allclose(lg.grad.cpu().numpy(), lc.grad.numpy(), rtol=1e-4, atol=1e-9)


# ----------------------------------------------------------------------------- NMS (bit-exact)
def test_nms_known_answers(device, gold_dir):
    from scan_amd.layers import nms
    kat = json.load(open(os.path.join(gold_dir, "nms_kat.json")))
    for case in kat["cases"]:
        keep = nms(torch.tensor(case["boxes"], device=device), torch.tensor(case["scores"], device=device), case["thresh"])
        assert sorted(keep.cpu().tolist()) == case["keep_sorted"]
        assert keep.cpu().tolist() == sorted(keep.cpu().tolist())


def _rand_boxes(rs, n, span=200.0, quant=None):
    xy = rs.uniform(0, span, (n, 2))
    wh = rs.uniform(1, span / 3, (n, 2))
    b = np.concatenate([xy, xy + wh], 1).astype(np.float32)
    if quant:
        b = np.round(b / quant) * quant
    return b.astype(np.float32)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 500, 1000, 4097, 8192])
def test_nms_random_bit_exact(device, n):
    from scan_amd import ops
    from oracle import coracle
    rs = np.random.RandomState(n)
    # quantised coordinates produce exact IoU ties with the threshold and duplicate boxes
    boxes = _rand_boxes(rs, n, quant=4.0 if n % 2 else None)
    scores = rs.rand(n).astype(np.float32)
    if n > 10:
        scores[::7] = scores[3]  # score ties: order must fall back to the index
    for thr in (0.3, 0.5, 0.6):
        keep = ops.nms(torch.from_numpy(boxes).to(device), torch.from_numpy(scores).to(device), thr, rule_ge=True)
        ref = coracle.nms(boxes, scores, thr)
        assert np.array_equal(keep.cpu().numpy(), ref), (n, thr)


def test_nms_empty_and_limits(device):
    from scan_amd.layers import nms
    k = nms(torch.zeros(0, 4, device=device), torch.zeros(0, device=device), 0.5)
    assert k.numel() == 0 and k.dtype == torch.int64 and k.device.type == "cpu"  # reference csrc/nms.h:17-18
    with pytest.raises(RuntimeError, match="SCAN_NMS_MAX"):
        nms(torch.zeros(262145, 4, device=device), torch.zeros(262145, device=device), 0.5)


def _tie_boxes(rs, n, span):
    """corners on a 4-pixel grid with x2 = 4 j - 1 (widths + 1 multiples of 4): IoU hits 1/4 and 1/2 EXACTLY, which is where
    the CPU rule (>=, csrc/cpu/nms_cpu.cpp:60) and the CUDA rule (>, csrc/cuda/nms.cu:60) part; duplicates included"""
    xy = np.floor(rs.uniform(0, span, (n, 2)) / 4.0) * 4.0
    return np.concatenate([xy, xy + np.ceil(rs.uniform(1, span / 3, (n, 2)) / 4.0) * 4.0 - 1.0], 1).astype(np.float32)


@pytest.mark.parametrize("n", [8193, 12000, 20000, 33000])
def test_nms_beyond_one_panel_bit_exact_both_rules(device, n):
    """n > SCAN_NMS_PANEL (nms_cuda has no size limit, csrc/cuda/nms.cu:70-131): the panel path -- multi-block bitonic sort,
    chain state one 8192-candidate panel at a time -- against the C oracle, with score ties and exact IoU ties, both tie
    rules, through the C ABI and through the compiled module; ml_nms on the same path."""
    from scan_amd import ops
    from scan_amd.layers import _C
    from oracle import coracle
    rs = np.random.RandomState(n)
    boxes = _tie_boxes(rs, n, 1500.0)
    scores = (rs.randint(0, n // 3, n) / float(n // 3)).astype(np.float32)
    one = np.ones(n, np.float32)
    labels = rs.randint(1, 4, n).astype(np.float32)
    bd, sd, ld = (torch.from_numpy(a).to(device) for a in (boxes, scores, labels))
    for thr in (0.25, 0.5):
        ge, gt = coracle.nms(boxes, scores, thr), coracle.ml_nms(boxes, scores, one, thr)
        assert not np.array_equal(ge, gt), "tie rules agree: the case does not tell them apart"
        assert np.array_equal(ops.nms(bd, sd, thr, rule_ge=True).cpu().numpy(), ge), (n, thr, ">=")
        assert np.array_equal(ops.nms(bd, sd, thr, rule_ge=False).cpu().numpy(), gt), (n, thr, ">")
        assert np.array_equal(_C.nms(bd, sd, thr).cpu().numpy(), ge)
        assert np.array_equal(_C.nms(bd, sd, thr, cuda_rule=True).cpu().numpy(), gt)
    assert np.array_equal(_C.ml_nms(bd, sd, ld, 0.5).cpu().numpy(), coracle.ml_nms(boxes, scores, labels, 0.5))
    keep = ops.nms(bd, sd, 0.5)
    assert ops.nms(bd[keep], sd[keep], 0.5).numel() == keep.numel()  # idempotence


def test_nms_at_maximum_size_properties(device):
    """n = SCAN_NMS_MAX (262,144 boxes, 8.6 GB of mask): no oracle at this size -- size-independent properties instead: kept
    indices strictly ascending, NMS of the survivors keeps every one of them (idempotence), and a sample of suppressed boxes
    each overlap a kept, higher-scored box at or above the threshold (and no kept box does)."""
    from scan_amd import _lib, ops
    n = _lib.NMS_MAX
    rs = np.random.RandomState(1)
    xy = rs.uniform(0, 20000, (n, 2))
    boxes = np.concatenate([xy, xy + rs.uniform(5, 300, (n, 2))], 1).astype(np.float32)
    scores = rs.rand(n).astype(np.float32)
    bd, sd = torch.from_numpy(boxes).to(device), torch.from_numpy(scores).to(device)
    keep = ops.nms(bd, sd, 0.5)
    assert 0 < keep.numel() < n and bool((keep[1:] > keep[:-1]).all())
    assert ops.nms(bd[keep], sd[keep], 0.5).numel() == keep.numel()
    kept = torch.zeros(n, dtype=torch.bool, device=device)
    kept[keep] = True

    def iou_with_kept_better(i):
        b = bd[i]
        better = kept & (sd > sd[i])
        bb = bd[better]
        w = (torch.minimum(b[2], bb[:, 2]) - torch.maximum(b[0], bb[:, 0]) + 1).clamp(min=0)
        h = (torch.minimum(b[3], bb[:, 3]) - torch.maximum(b[1], bb[:, 1]) + 1).clamp(min=0)
        inter = w * h
        area = lambda t: (t[..., 2] - t[..., 0] + 1) * (t[..., 3] - t[..., 1] + 1)
        return float((inter / (area(b) + area(bb) - inter)).max()) if bb.numel() else 0.0
    dropped = torch.nonzero(~kept).squeeze(1)
    for i in dropped[torch.linspace(0, dropped.numel() - 1, 12).long()].tolist():
        assert iou_with_kept_better(i) >= 0.5, i
    for i in keep[torch.linspace(0, keep.numel() - 1, 12).long()].tolist():
        assert iou_with_kept_better(i) < 0.5, i


def test_nms_many_panels_bit_exact(device):
    """n = 70,000: nine 8,192-candidate panels of the scan, 1,094 mask words per row (the OR phase walks 18 groups of 64), a
    131,072-key bitonic network (stages 16,384 ... 131,072 through the global compare-exchange steps) -- against the C oracle."""
    from scan_amd import ops
    from oracle import coracle
    n = 70000
    rs = np.random.RandomState(n)
    boxes = _tie_boxes(rs, n, 4000.0)
    scores = (rs.randint(0, n // 2, n) / float(n // 2)).astype(np.float32)
    keep = ops.nms(torch.from_numpy(boxes).to(device), torch.from_numpy(scores).to(device), 0.5, rule_ge=True)
    ref = coracle.nms(boxes, scores, 0.5)
    assert 0 < len(ref) < n and np.array_equal(keep.cpu().numpy(), ref)


def test_ml_nms_bit_exact(device):
    from scan_amd.layers import ml_nms
    from oracle import coracle
    rs = np.random.RandomState(5)
    for n in (10, 300, 2500):
        boxes = _rand_boxes(rs, n, span=120.0)
        scores = rs.rand(n).astype(np.float32)
        labels = rs.randint(1, 9, n).astype(np.float32)
        keep = ml_nms(torch.from_numpy(boxes).to(device), torch.from_numpy(scores).to(device),
                      torch.from_numpy(labels).to(device), 0.6)
        assert np.array_equal(keep.cpu().numpy(), coracle.ml_nms(boxes, scores, labels, 0.6))


def test_nms_idempotent_full_size(device):
    """size-independent property at the path's maximum n: NMS of the survivors keeps all of them."""
    from scan_amd import ops
    rs = np.random.RandomState(11)
    boxes = torch.from_numpy(_rand_boxes(rs, 8192, span=2048.0)).to(device)
    scores = torch.from_numpy(rs.rand(8192).astype(np.float32)).to(device)
    keep = ops.nms(boxes, scores, 0.6)
    again = ops.nms(boxes[keep], scores[keep], 0.6)
    assert again.numel() == keep.numel()


# ----------------------------------------------------------------------------- conv (fp32 MFMA)
CONV_CASES = [
    # (levels [(H,W)], N, Cin, Cout, k, stride, relu)
    ([(8, 16)], 2, 256, 256, 3, 1, False),
    ([(16, 32), (8, 16), (4, 8), (2, 4), (1, 2)], 2, 256, 256, 3, 1, False),  # shared-weight tower
    ([(9, 13)], 1, 64, 128, 3, 1, True),     # ragged spatial size, fused ReLU
    ([(32, 64)], 1, 3, 64, 3, 1, True),      # first VGG conv (Cin 3 -> stride 4)
    ([(8, 16)], 2, 512, 256, 1, 1, False),   # FPN lateral 1x1
    ([(8, 16)], 2, 256, 256, 3, 2, False),   # P6/P7 stride 2
    ([(7, 9)], 1, 256, 256, 3, 2, False),    # stride 2, odd size
    ([(8, 16), (4, 8)], 2, 265, 256, 3, 1, True),   # head_out: cat(features, act maps)
    ([(8, 16)], 2, 256, 8, 3, 1, False),     # cls_logits (skinny N kernel)
    ([(8, 16)], 2, 256, 5, 3, 1, False),     # bbox_pred + centerness fused
    ([(8, 16)], 1, 264, 1024, 3, 1, True),   # stacked CKA class branches
    ([(6, 10)], 2, 128, 40, 3, 1, False),    # Cout tail inside a 128-wide tile
    ([(32, 48)], 2, 3, 64, 7, 2, True),      # ResNet stem 7x7 / stride 2 (+ folded FrozenBN + ReLU)
    ([(12, 20)], 2, 256, 128, 1, 2, True),   # bottleneck conv1 with the stride in the 1x1 (layer2.0.conv1)
    ([(11, 15)], 1, 256, 512, 1, 2, False),  # downsample 1x1 / stride 2, odd size
    ([(8, 12)], 2, 128, 512, 1, 1, False),   # bottleneck conv3
]


@pytest.fixture
def conv_generation(request):
    """1 = the production kernels; 0 = the independent implementations kept as cross-checks: scan_tune("conv_v2", 0) sends
    the two-piece forward / data gradient to the 32x32x16 kernel of csrc/conv_gen1.hip, scan_tune("wgrad_v6", 0) the 3x3
    weight gradient (two and three pieces) to conv_wgrad_v4_kernel."""
    from scan_amd import _lib
    old = _lib.query("scan_tune", b"conv_v2", int(request.param))
    oldw = _lib.query("scan_tune", b"wgrad_v6", int(request.param))
    yield request.param
    _lib.query("scan_tune", b"conv_v2", old)
    _lib.query("scan_tune", b"wgrad_v6", oldw)


@pytest.mark.parametrize("mode,conv_generation", [("fp32", 1), ("bf16x6", 1), ("bf16x6", 0), ("bf16x3", 1), ("bf16x3", 0)],
                         indirect=["conv_generation"])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv2d_fwd_bwd(device, case, mode, conv_generation, monkeypatch):
    from scan_amd import ops
    monkeypatch.setattr(ops, "CONV_MODE", mode)
    # bf16x6 carries all 24 significand bits of both operands: the bar of the exact fp32-MFMA kernels.
    # bf16x3: operands carry 16 significand bits (hi + lo); products exact, fp32 accumulate
    tol = 1e-4 if mode == "bf16x3" else 2e-5
    sizes, N, cin, cout, k, stride, relu = case
    import zlib
    g = torch.Generator().manual_seed(zlib.crc32(str(case).encode()))
    xs = [torch.randn(N, cin, h, w, generator=g) for h, w in sizes]
    wgt = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    bias = torch.randn(cout, generator=g)
    # oracle: plain fp32 torch on the CPU
    xr = [x.clone().requires_grad_(True) for x in xs]
    wr, br = wgt.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    yr = [F.conv2d(x, wr, br, stride=stride, padding=k // 2) for x in xr]
    if relu:
        yr = [F.relu(y) for y in yr]
    gys = [torch.randn(y.shape, generator=g) for y in yr]
    if relu:
        # an output within rounding distance of 0 may land on the other side of the ReLU on the GPU; give
        # those (measure-zero) elements no upstream gradient so a mask flip cannot enter the comparison
        pre = [F.conv2d(x, wgt, bias, stride=stride, padding=k // 2) for x in xs]
        gys = [gy * (p.abs() > 1e-3) for gy, p in zip(gys, pre)]
    sum((y * gy).sum() for y, gy in zip(yr, gys)).backward()
    # HIP
    cs = ops.pad4(cin)
    rows, shape = _pyr(xs, device, cs)
    rows.requires_grad_(True)
    wd = wgt.to(device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    bd = bias.to(device).requires_grad_(True)
    y = ops.conv2d(rows, wd, bd, shape, k, stride, relu=relu)
    oshape = shape.conv_out(k, stride)
    if y.shape[1] > cout:  # padding columns of the row matrix stay zero (the next conv reads them as channels)
        assert float(y[:, cout:].abs().max()) == 0.0
    ys = _unrows(y, oshape, cout)
    for a, b in zip(ys, yr):
        np.testing.assert_allclose(a.numpy(), b.detach().numpy(), rtol=1e-4, atol=tol)
    gy_rows, _ = _pyr(gys, device, y.shape[1])
    y.backward(gy_rows)
    dxs = _unrows(rows.grad, shape, cin)
    for a, b in zip(dxs, xr):
        np.testing.assert_allclose(a.numpy(), b.grad.numpy(), rtol=1e-4, atol=tol * max(1.0, float(b.grad.abs().max())))
    scale = max(1.0, float(wr.grad.abs().max()))
    np.testing.assert_allclose(wd.grad.cpu().numpy(), wr.grad.numpy(), rtol=1e-4, atol=tol * scale)
    np.testing.assert_allclose(bd.grad.cpu().numpy(), br.grad.numpy(), rtol=1e-4, atol=2e-5 * max(1.0, float(br.grad.abs().max())))


def test_conv_64_channel_tiles_agree(device, monkeypatch):
    """the <= 64-channel 3x3 instance on 32x16- (default for H % 32 == 0), 16x16- and 8x16-pixel tiles (scan_tune
    conv_bn64_th16 = 2 / 1 / 0): the same K order per output element, so the results are bit-identical -- plain, with the fused
    ReLU + 2x2 max-pool epilogue of the frozen stages, and as a data gradient; on a size where the 32-row tile does not apply
    (H = 48) the default is the 16x16 tile."""
    from scan_amd import _lib, ops
    monkeypatch.setattr(ops, "CONV_MODE", "bf16x6")
    torch.manual_seed(11)
    for (h, w_), want in (((64, 96), 2064), ((48, 64), 1064)):
        shape = ops.PyramidShape(2, [(h, w_)])
        assert _lib.query("scan_conv3x3_bf16x6_instance", shape.ref(), 64) == want
        x = torch.randn(shape.rows, 64, device=device).relu_()
        w = (torch.randn(64, 64, 3, 3, device=device) / 24).contiguous(memory_format=torch.channels_last)
        b = torch.randn(64, device=device)
        gy = torch.randn(shape.rows, 64, device=device)

        def run():
            with torch.no_grad():
                pooled = ops.conv2d(x, w, b, shape, 3, 1, relu=True, pool=True)
            xx = x.clone().requires_grad_(True)
            y = ops.conv2d(xx, w, b, shape, 3, 1, relu="deferred")
            y.backward(gy)
            return pooled, y.detach(), xx.grad.clone()

        outs = {}
        for knob in (2, 1, 0):
            old = _lib.query("scan_tune", b"conv_bn64_th16", knob)
            try:
                outs[knob] = run()
            finally:
                _lib.query("scan_tune", b"conv_bn64_th16", old)
        for knob in (1, 0):
            for a, c in zip(outs[2], outs[knob]):
                assert torch.equal(a, c), (h, w_, knob)
        ref = torch.nn.functional.conv2d(x.view(2, h, w_, 64).permute(0, 3, 1, 2).double().cpu(), w.double().cpu(), b.double().cpu(),
                                         padding=1)
        got = outs[2][1].view(2, h, w_, 64).permute(0, 3, 1, 2).double().cpu()
        assert (got - ref.relu()).abs().max().item() <= 5e-6 * ref.abs().max().item()


@pytest.mark.parametrize("mode", ["bf16x6", "bf16x3"])
def test_conv_instances_agree_full_size(device, mode, monkeypatch):
    """the ways a 256 -> 256 tower layer can run on 4 frames of 128x256 (P3 of the bench workload): 16x16x32
    kernel with 256-channel tiles (the default for this launch), with 128-channel tiles (bit-identical: same K order
    per output), and -- two pieces -- the 32x32x16 kernel (agrees to rounding); three pieces: against the exact fp32-MFMA
    kernels at the fp32 bar -- forward with GroupNorm sums, and the masked data gradient."""
    from scan_amd import _lib, ops
    monkeypatch.setattr(ops, "CONV_MODE", mode)
    inst = "scan_conv3x3_%s_instance" % mode
    shape = ops.PyramidShape(4, [(128, 256)])
    assert _lib.query(inst, shape.ref(), 256) % 1000 == 256
    torch.manual_seed(3)
    x = torch.randn(shape.rows, 256, device=device)
    w = (torch.randn(256, 256, 3, 3, device=device) / 48).contiguous(memory_format=torch.channels_last)
    b = torch.randn(256, device=device)
    gy = torch.randn(shape.rows, 256, device=device)

    with torch.no_grad():
        h0 = ops.conv2d(x, w, b, shape, 3, 1, relu=True)  # a ReLU output: the mask (h0 > 0) of the data gradient

    def run():
        hh = h0.clone().requires_grad_(True)
        y = ops.conv2d(hh, w, b, shape, 3, 1, mask_dx=True, gn_sums=True)  # mask_dx: dx *= (hh > 0) in the epilogue
        sums = ops._gn_sums.pop(y.data_ptr()).clone()
        y.backward(gy)
        return y.detach(), sums, hh.grad.clone()

    ref = run()
    old = _lib.query("scan_tune", b"conv_bn256", 0)
    try:
        assert _lib.query(inst, shape.ref(), 256) % 1000 == 128
        narrow = run()
    finally:
        _lib.query("scan_tune", b"conv_bn256", old)
    assert torch.equal(ref[0], narrow[0]) and torch.equal(ref[2], narrow[2])
    assert torch.allclose(ref[1], narrow[1], rtol=1e-12, atol=0)  # fp64 atomics: order may differ
    if mode == "bf16x3":
        old = _lib.query("scan_tune", b"conv_v2", 0)
        try:
            other = run()
        finally:
            _lib.query("scan_tune", b"conv_v2", old)
        bar = 1e-5
    else:
        monkeypatch.setattr(ops, "CONV_MODE", "fp32")
        hh = h0.clone().requires_grad_(True)
        y = ops.conv2d(hh, w, b, shape, 3, 1, mask_dx=True)
        y.backward(gy)
        other = (y.detach(), None, hh.grad.clone())
        bar = 2e-6
    for a, c in zip(ref, other):
        if c is None:
            continue
        assert torch.allclose(a.double(), c.double(), rtol=1e-4, atol=bar * float(c.abs().max())), \
            (a.double() - c.double()).abs().max().item()


def test_conv_16_wave_instance_on_pyramid(device, monkeypatch):
    """(two-piece instances) a tower layer over the five-level pyramid of 4 frames takes the 256-channel tile on 16-wave workgroups; the
    8-wave workgroups (scan_tune conv_wg1024 = 0), the three-taps-per-barrier staging and per-level launches give
    bit-identical results."""
    from scan_amd import _lib, ops
    monkeypatch.setattr(ops, "CONV_MODE", "bf16x3")
    pyr = ops.PyramidShape(4, [(128, 256), (64, 128), (32, 64), (16, 32), (8, 16)])
    assert _lib.query("scan_conv3x3_bf16x3_instance", pyr.ref(), 256) == (2256 if _lib.query("scan_tune_get", b"conv_w8") else 1256)
    assert _lib.query("scan_conv3x3_bf16x3_instance", ops.PyramidShape(2, [(64, 64)]).ref(), 256) == 1128
    torch.manual_seed(5)
    x = torch.randn(pyr.rows, 256, device=device)
    w = (torch.randn(256, 256, 3, 3, device=device) / 48).contiguous(memory_format=torch.channels_last)
    b = torch.randn(256, device=device)
    with torch.no_grad():
        y16 = ops.conv2d(x, w, b, pyr, 3, 1, relu=True)
        old = _lib.query("scan_tune", b"conv_wg1024", 0)
        try:
            y8 = ops.conv2d(x, w, b, pyr, 3, 1, relu=True)
        finally:
            _lib.query("scan_tune", b"conv_wg1024", old)
        assert torch.equal(y16, y8)
        for w8 in (0, 1):  # the 256-channel LDS-DMA tile on 16 waves / on 8 waves
            old = _lib.query("scan_tune", b"conv_w8", w8)
            try:
                assert _lib.query("scan_conv3x3_bf16x3_instance", pyr.ref(), 256) == (2256 if w8 else 1256)
                yw = ops.conv2d(x, w, b, pyr, 3, 1, relu=True)
            finally:
                _lib.query("scan_tune", b"conv_w8", old)
            assert torch.equal(y16, yw), w8
        w128 = w[:128].contiguous(memory_format=torch.channels_last)
        ya = ops.conv2d(x, w128, b[:128], pyr, 3, 1)
        old = _lib.query("scan_tune", b"conv_tpb3", 3)
        try:
            yb = ops.conv2d(x, w128, b[:128], pyr, 3, 1)
            old2 = _lib.query("scan_tune", b"conv_wg1024", 0)
            try:
                yc = ops.conv2d(x, w128, b[:128], pyr, 3, 1)
            finally:
                _lib.query("scan_tune", b"conv_wg1024", old2)
        finally:
            _lib.query("scan_tune", b"conv_tpb3", old)
        assert torch.equal(ya, yb) and torch.equal(ya, yc)
        for l in range(pyr.n_levels):
            yl = ops.conv2d(x[pyr.row_off[l]:pyr.row_off[l + 1]].contiguous(), w, b, pyr.level(l), 3, 1, relu=True)
            assert torch.equal(yl, y16[pyr.row_off[l]:pyr.row_off[l + 1]]), l


def test_conv2d_linearity_full_size(device):
    """size-independent property at the BASELINE config size (tower layer on a 2 x 1024x2048 pyramid):
    conv(a*x1 + x2) == a*conv(x1) + conv(x2) - bias terms, and the pyramid launch equals per-level launches."""
    from scan_amd import ops
    N = 2
    sizes = [(128, 256), (64, 128), (32, 64), (16, 32), (8, 16)]
    shape = ops.PyramidShape(N, sizes)
    torch.manual_seed(0)
    x1 = torch.randn(shape.rows, 256, device=device)
    x2 = torch.randn(shape.rows, 256, device=device)
    w = (torch.randn(256, 256, 3, 3, device=device) / 48).contiguous(memory_format=torch.channels_last)
    y1 = ops.conv2d(x1, w, None, shape)
    y2 = ops.conv2d(x2, w, None, shape)
    y12 = ops.conv2d(2.0 * x1 + x2, w, None, shape)
    err = (y12 - (2.0 * y1 + y2)).abs().max().item()
    assert err < 1e-3 * y12.abs().max().item()
    for l in (0, 4):
        yl = ops.conv2d(x1[shape.row_off[l]:shape.row_off[l + 1]].contiguous(), w, None, shape.level(l))
        assert torch.equal(yl, y1[shape.row_off[l]:shape.row_off[l + 1]])
    # the split-operand matrix-core path (default: bf16x6) against the exact fp32-MFMA path at full size
    ops.CONV_MODE, keep = "fp32", ops.CONV_MODE
    try:
        yf = ops.conv2d(x1, w, None, shape)
    finally:
        ops.CONV_MODE = keep
    assert keep == "bf16x6"
    assert (yf - y1).abs().max().item() < 5e-6 * yf.abs().max().item()  # two fp32 summation orders over K = 2304


def _conv_fp64_samples(x_rows, shape, w, level, n_samples, seed):
    """fp64 CPU reference of a 3x3 / pad-1 conv (no bias) at n_samples random output pixels of one pyramid level:
    x_rows [M, Cin] fp32 rows, w [Cout, Cin, 3, 3]; returns (row indices [S], values [S, Cout] fp64)."""
    h, wd_ = shape.sizes[level]
    n = shape.n_images
    cin = w.shape[1]
    x = x_rows[shape.row_off[level]:shape.row_off[level + 1], :cin].cpu().double().view(n, h, wd_, cin)
    xp = torch.zeros(n, h + 2, wd_ + 2, cin, dtype=torch.float64)
    xp[:, 1:-1, 1:-1] = x
    rs = np.random.RandomState(seed)
    ni, yi, xi = rs.randint(0, n, n_samples), rs.randint(0, h, n_samples), rs.randint(0, wd_, n_samples)
    # border pixels are where halo handling can go wrong: force a share of the samples onto them
    yi[: n_samples // 8] = rs.choice([0, h - 1], n_samples // 8)
    xi[n_samples // 8: n_samples // 4] = rs.choice([0, wd_ - 1], n_samples // 4 - n_samples // 8)
    patches = torch.stack([xp[ni, yi + ky, xi + kx] for ky in range(3) for kx in range(3)], 1)  # [S, 9, Cin]
    wk = w.cpu().double().permute(2, 3, 1, 0).reshape(9, cin, -1)                                 # [9, Cin, Cout]
    ref = torch.einsum("stc,tco->so", patches, wk)
    rows = shape.row_off[level] + (torch.from_numpy(ni) * h + torch.from_numpy(yi)) * wd_ + torch.from_numpy(xi)
    return rows, ref


CONV_ERR_CASES = [
    # (levels, N, Cin, Cout): small CONV_CASES shapes and the layers of the bench workload at full size
    ([(8, 16)], 2, 256, 256),
    ([(16, 32), (8, 16), (4, 8), (2, 4), (1, 2)], 2, 256, 256),
    ([(8, 16), (4, 8)], 2, 268, 256),
    ([(8, 16)], 1, 264, 1024),
    ([(256, 512)], 4, 256, 256),                                     # conv3_2, 4 frames of 1024x2048
    ([(128, 256)], 4, 512, 512),                                     # conv4_2
    ([(128, 256), (64, 128), (32, 64), (16, 32), (8, 16)], 4, 256, 256),  # tower layer over the pyramid
    ([(512, 1024)], 2, 128, 128),                                    # conv2_2 (128-channel tile)
    ([(512, 1024)], 1, 64, 64),                                      # conv1_2 geometry (64-channel tile)
]


@pytest.mark.parametrize("case", CONV_ERR_CASES)
def test_conv_error_vs_fp64(device, case):
    """the three conv arithmetics against an fp64 convolution on the host (sampled output pixels, all channels; data
    gradient = the same kernel on flipped planes, weight gradient: test_wgrad_full_size_elementwise): bf16x6 -- three bf16
    pieces per operand, all 24 significand bits -- must be NO FURTHER from fp64 than the exact fp32-MFMA kernels are (its fp32
    accumulation takes 6 rounded additions per 32 input channels where an fp32 FMA chain takes 32); bf16x3 sits ~2^-17
    per product behind both."""
    from scan_amd import ops
    sizes, N, cin, cout = case
    shape = ops.PyramidShape(N, sizes)
    g = torch.Generator(device=device).manual_seed(cin * 7 + cout)
    cs = ops.pad4(cin)
    x = torch.randn((shape.rows, cs), device=device, generator=g)
    if cs != cin:
        x[:, cin:] = 0
    w = (torch.randn((cout, cin, 3, 3), device=device, generator=g) / (cin * 9) ** 0.5).contiguous(memory_format=torch.channels_last)
    errs = {}
    keep = ops.CONV_MODE
    try:
        outs = {}
        for mode in ("fp32", "bf16x6", "bf16x3"):
            ops.CONV_MODE = mode
            with torch.no_grad():
                outs[mode] = ops.conv2d(x, w, None, shape, 3, 1)[:, :cout].cpu().double()
    finally:
        ops.CONV_MODE = keep
    worst = {m: 0.0 for m in outs}
    rms = {m: 0.0 for m in outs}
    cnt = 0
    for l in range(shape.n_levels):
        ns = min(2048, 4 * shape.n_images * sizes[l][0] * sizes[l][1])
        rows, ref = _conv_fp64_samples(x, shape, w, l, ns, seed=l + 1)
        scale = float(ref.abs().max())
        for m, y in outs.items():
            d = (y[rows] - ref).abs() / scale
            worst[m] = max(worst[m], float(d.max()))
            rms[m] += float((d ** 2).sum())
        cnt += ref.numel()
    rms = {m: (v / cnt) ** 0.5 for m, v in rms.items()}
    print("conv error vs fp64 (max / rms, relative to the largest output)", case, {m: (worst[m], rms[m]) for m in outs})
    assert worst["fp32"] <= 5e-6 and worst["bf16x6"] <= 5e-6, worst
    # "no larger than the fp32-MFMA kernel's": on the rms over ~10^5..10^6 sampled outputs (stable), with 10 % slack; the
    # single worst sample within 1.5x
    assert rms["bf16x6"] <= 1.1 * rms["fp32"], rms
    assert worst["bf16x6"] <= 1.5 * worst["fp32"], worst
    assert rms["bf16x3"] <= 5e-5 and rms["bf16x3"] >= rms["bf16x6"], rms


WGRAD_FULL_CASES = [
    # (levels, N, Cin, Cout): the shapes the weight gradient is benchmarked at
    ([(256, 512)], 4, 256, 256),                                          # conv3_2
    ([(128, 256)], 4, 512, 512),                                          # conv4_2
    ([(128, 256), (64, 128), (32, 64), (16, 32), (8, 16)], 4, 256, 256),  # five-level tower pyramid
    ([(128, 256)], 4, 264, 1024),                                         # discriminator class branches at P3
    ([(128, 256), (64, 128), (32, 64), (16, 32), (8, 16)], 4, 268, 256),  # middle-head output conv (act-map share)
    ([(37, 53), (19, 27)], 3, 256, 256),                                  # ragged rows: partial last chunk of every row
]


@pytest.mark.parametrize("mode", ["bf16x6", "bf16x3"])
@pytest.mark.parametrize("case", WGRAD_FULL_CASES)
def test_wgrad_full_size_elementwise(device, case, mode, monkeypatch):
    """the weight gradient AT THE SIZES IT IS BENCHMARKED AT, element by element: the production kernel (producer /
    consumer waves, split-K slabs) against the independent fp32-MFMA weight gradient (<= 1e-4 of the largest element for
    two pieces, 2e-6 for three) and against the other split kernel (scan_tune wgrad_v6 = 0); plus the adjoint identity
    <conv(x, w), g> = <w, wgrad(x, g)> = <x, dgrad(g, w)> accumulated in fp64 (<= 2e-6 of the absolute-value scale).  A
    dropped chunk, a wrong halo column or a mis-reduced slab moves single elements by far more than either bar."""
    from scan_amd import _lib, ops
    sizes, N, cin, cout = case
    shape = ops.PyramidShape(N, sizes)
    g = torch.Generator(device=device).manual_seed(cin + cout + len(sizes))
    cs = ops.pad4(cin)
    x = torch.randn((shape.rows, cs), device=device, generator=g)
    if cs != cin:
        x[:, cin:] = 0
    gy = torch.randn((shape.rows, cout), device=device, generator=g)
    w0 = (torch.randn((cout, cin, 3, 3), device=device, generator=g) / (cin * 9) ** 0.5).contiguous(memory_format=torch.channels_last)
    b0 = torch.randn((cout,), device=device, generator=g)

    def grads(conv_mode, v6=1, tile=None):
        monkeypatch.setattr(ops, "CONV_MODE", conv_mode)
        old = _lib.query("scan_tune", b"wgrad_v6", v6)
        dflt = _lib.query("scan_tune_default", b"wgrad_tile")
        assert dflt == 2, "the shipped default is 'by piece count': three pieces take the 32 x 64 tile with the temporary accumulator"
        old_tile = _lib.query("scan_tune", b"wgrad_tile", dflt if tile is None else tile)
        try:
            xx = x.clone().requires_grad_(True)
            w = w0.clone().requires_grad_(True)
            b = b0.clone().requires_grad_(True)
            y = ops.conv2d(xx, w, b, shape, 3, 1)
            y.backward(gy)
            return y.detach(), xx.grad, w.grad, b.grad
        finally:
            _lib.query("scan_tune", b"wgrad_v6", old)
            _lib.query("scan_tune", b"wgrad_tile", old_tile)

    y, dx, dw, db = grads(mode)
    _, _, dw_other, db_other = grads(mode, v6=0)
    _, _, dw32, db32 = grads("fp32")
    scale = float(dw32.abs().max())
    # (a) every element against the independent fp32-MFMA kernel.  Both sum ~10^5..10^6 fp32 terms in different orders:
    # they agree to ~3e-6 of the largest element; one dropped 32-pixel chunk would move elements by ~1e-3 of it
    bar = 1e-4 if mode == "bf16x3" else 1e-5
    assert float((dw - dw32).abs().max()) <= bar * scale, (float((dw - dw32).abs().max()), scale)
    assert float((dw_other - dw32).abs().max()) <= bar * scale
    if mode == "bf16x3":
        assert torch.equal(dw, dw_other)  # same K order, same split-K boundaries: bit-identical slabs
    assert float((db - db32).abs().max()) <= 5e-6 * float(db32.abs().max())
    assert float((db - db_other).abs().max()) <= 5e-6 * float(db32.abs().max())
    # (b) sampled elements (16 output x 16 input channels x 9 taps) against an fp64 weight gradient computed on the device:
    # the three-piece kernel is no further from it than the exact fp32-MFMA kernel
    rs = np.random.RandomState(cin)
    oi = torch.from_numpy(rs.choice(cout, 16, replace=False)).to(device)
    ci = torch.from_numpy(rs.choice(cin, 16, replace=False)).to(device)
    ref = torch.zeros((16, 16, 3, 3), dtype=torch.float64, device=device)
    for l, (h, wd_) in enumerate(sizes):
        r0, r1 = shape.row_off[l], shape.row_off[l + 1]
        xs = x[r0:r1][:, ci].double().view(N, h, wd_, 16)
        gs = gy[r0:r1][:, oi].double().view(N, h, wd_, 16)
        xp = torch.zeros((N, h + 2, wd_ + 2, 16), dtype=torch.float64, device=device)
        xp[:, 1:-1, 1:-1] = xs
        for ky in range(3):
            for kx in range(3):
                ref[:, :, ky, kx] += torch.einsum("nyxo,nyxc->oc", gs, xp[:, ky:ky + h, kx:kx + wd_])
    def sampled_err(t):
        d = (t.double()[oi][:, ci] - ref).abs() / float(ref.abs().max())
        return float(d.max()), float((d ** 2).mean() ** 0.5)
    e, e32 = sampled_err(dw), sampled_err(dw32)
    print("wgrad error vs fp64 (max, rms)", case, mode, e, "fp32-MFMA", e32)
    if mode == "bf16x6":
        # no further from fp64 than the exact fp32-MFMA kernel: the six piece products of a 32-pixel step are summed in a
        # temporary and added to the running accumulator once (csrc/conv_wgrad.hip: TCHAIN), so a split-K slab's 8,192-pixel
        # chain rounds once per step at the accumulator's magnitude.  Measured 0.2-0.5x the fp32-MFMA kernel's rms
        # (tools/wgrad_err.py); without the temporary it is 1.0-2.1x
        assert e[0] <= 5e-6 and e[1] <= 1.1 * e32[1] and e[0] <= 1.5 * e32[0], (e, e32)
        # scan_tune wgrad_tile = 0 (the 64 x 32 consumer tile) has no temporary: the six products go straight into the running
        # accumulator -- correct to the same element bar against the fp32-MFMA kernel, an fp32 sum in another order (bar: 3x its
        # distance from fp64).  Round 6 ran the whole golden suite green on it, found it no faster in the training step
        # (profiles/r06_wgrad_tile_ab.txt) and left it a knob.
        _, _, dw_t0, _ = grads(mode, tile=0)
        assert float((dw_t0 - dw32).abs().max()) <= 1e-5 * scale
        e_t0 = sampled_err(dw_t0)
        print("   wgrad_tile = 0 (no temporary accumulator):", e_t0)
        assert e_t0[0] <= 1e-5 and e_t0[1] <= 3.0 * e32[1] and e_t0[1] >= e[1], (e_t0, e, e32)
    else:
        assert e[0] <= 1e-4, e
    # adjoint identities (bias removed from y), fp64 accumulation on the device
    yl = (y[:, :cout] - b0).double()
    lhs = float((yl * gy.double()).sum())
    via_w = float((w0.double() * dw.double()).sum())
    via_x = float((x.double() * dx.double()).sum())
    ascale = float((yl.abs() * gy.double().abs()).sum())
    assert abs(lhs - via_w) <= 2e-6 * ascale and abs(lhs - via_x) <= 2e-6 * ascale, (lhs, via_w, via_x, ascale)


@pytest.mark.parametrize("mode", ["bf16x6", "bf16x3"])
def test_conv_kernels_are_run_to_run_identical(device, mode, monkeypatch):
    """forward, data gradient and weight gradient (split-K slabs reduced in a fixed order) are order-fixed: two runs on the same
    inputs give the same bits, at the bench's tower-pyramid size (no atomics anywhere on the conv path except the GroupNorm
    sums, which are not requested here)."""
    from scan_amd import ops
    monkeypatch.setattr(ops, "CONV_MODE", mode)
    shape = ops.PyramidShape(4, [(128, 256), (64, 128), (32, 64), (16, 32), (8, 16)])
    g = torch.Generator(device=device).manual_seed(17)
    x = torch.randn((shape.rows, 256), device=device, generator=g)
    gy = torch.randn((shape.rows, 256), device=device, generator=g)
    w0 = (torch.randn((256, 256, 3, 3), device=device, generator=g) / 48).contiguous(memory_format=torch.channels_last)
    b0 = torch.randn((256,), device=device, generator=g)
    outs = []
    for _ in range(2):
        xx, w, b = x.clone().requires_grad_(True), w0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
        y = ops.conv2d(xx, w, b, shape, 3, 1, relu=True)
        y.backward(gy)
        outs.append((y.detach().clone(), xx.grad.clone(), w.grad.clone(), b.grad.clone()))
    for a, c in zip(*outs):
        assert torch.equal(a, c)


def test_shipped_library_has_no_ablation_knobs(device):
    """timing-ablation kernel instances (wrong results by construction) are not part of the shipped library: their
    scan_tune keys do not exist, so no environment variable can switch them on."""
    from scan_amd import _lib
    for key in (b"conv_exp", b"wgrad_exp", b"wgrad_v2", b"wgrad_v3", b"wgrad_v4", b"wgrad_v5", b"wgrad_il", b"wgrad_wg1024"):
        assert _lib.query("scan_tune_get", key) == _lib.TUNE_UNKNOWN, key
        assert _lib.query("scan_tune", key, 1) == _lib.TUNE_UNKNOWN, key


def test_mfma_sustained_measurement(device):
    """scan_mfma_sustained_bf16 (bench.py's roofline.board_sustained): finite positive rates below the nominal peak on random
    operands and on zeros, argument errors reported through the C ABI.  (Sanity only: how close a board gets to the peak and
    how far zeros run ahead of random operands is a measurement -- profiles/r04_mfma_peak.txt -- not a correctness bar; a
    throttled or shared board must not fail the suite.)"""
    import ctypes
    from scan_amd import _lib, ops
    tf = ctypes.c_double(0.0)
    _lib.call("scan_mfma_sustained_bf16", 0.3, 1, ctypes.byref(tf), ops._stream())
    rnd = tf.value
    _lib.call("scan_mfma_sustained_bf16", 0.3, 0, ctypes.byref(tf), ops._stream())
    zeros = tf.value
    assert np.isfinite(rnd) and np.isfinite(zeros) and 0.0 < rnd <= 2500.0 and 0.0 < zeros <= 2500.0, (rnd, zeros)
    with pytest.raises(RuntimeError):
        _lib.call("scan_mfma_sustained_bf16", 0.0, 1, ctypes.byref(tf), ops._stream())


def test_conv2d_errors(device):
    from scan_amd import ops
    shape = ops.PyramidShape(1, [(4, 4)])
    x = torch.zeros(16, 6, device=device)  # stride not a multiple of 4
    w = torch.zeros(8, 6, 3, 3, device=device)
    with pytest.raises(RuntimeError):
        ops.conv2d(x, w, None, shape)
    with pytest.raises(RuntimeError):
        ops.conv2d(torch.zeros(16, 8), torch.zeros(8, 8, 3, 3), None, shape)  # CPU tensors: no fallback


# ----------------------------------------------------------------------------- GroupNorm + ReLU
@pytest.mark.parametrize("sizes", [[(8, 16)], [(16, 32), (8, 16), (4, 8), (2, 4), (1, 2)], [(5, 7), (3, 3)]])
def test_groupnorm_relu(device, sizes):
    from scan_amd import ops
    N = 2
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(N, 256, h, w, generator=g) * 2 + 0.5 for h, w in sizes]
    gamma = 1 + 0.1 * torch.randn(256, generator=g)
    beta = 0.1 * torch.randn(256, generator=g)
    xr = [x.clone().requires_grad_(True) for x in xs]
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    yr = [F.relu(F.group_norm(x, 32, gr, br)) for x in xr]
    gys = [torch.randn(y.shape, generator=g) for y in yr]
    sum((y * gy).sum() for y, gy in zip(yr, gys)).backward()
    rows, shape = _pyr(xs, device)
    rows.requires_grad_(True)
    gd, bd = gamma.to(device).requires_grad_(True), beta.to(device).requires_grad_(True)
    y = ops.groupnorm_relu(rows, gd, bd, shape)
    for a, b in zip(_unrows(y, shape, 256), yr):
        np.testing.assert_allclose(a.numpy(), b.detach().numpy(), rtol=1e-4, atol=1e-5)
    gy_rows, _ = _pyr(gys, device)
    y.backward(gy_rows)
    for a, b in zip(_unrows(rows.grad, shape, 256), xr):
        np.testing.assert_allclose(a.numpy(), b.grad.numpy(), rtol=1e-3, atol=2e-5)
    np.testing.assert_allclose(gd.grad.cpu().numpy(), gr.grad.numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(bd.grad.cpu().numpy(), br.grad.numpy(), rtol=1e-4, atol=1e-4)


# ----------------------------------------------------------------------------- dynamic conv + softmax
@pytest.mark.parametrize("M,K", [(1, 9), (15, 9), (16, 9), (1000, 9), (4099, 9), (257, 2)])
def test_dynconv_softmax(device, M, K):
    from scan_amd import ops
    g = torch.Generator().manual_seed(M)
    feat = torch.randn(M, 256, generator=g)
    ker = torch.randn(K, 256, generator=g) / 16
    fr, kr = feat.clone().requires_grad_(True), ker.clone().requires_grad_(True)
    lr = fr @ kr.t()
    pr = lr.softmax(1)
    g1, g2 = torch.randn(M, K, generator=g), torch.randn(M, K, generator=g)
    ((lr * g1).sum() + (pr * g2).sum()).backward()
    fd, kd = feat.to(device).requires_grad_(True), ker.to(device).requires_grad_(True)
    l, p = ops.dynconv_softmax(fd, kd)
    np.testing.assert_allclose(l.detach().cpu().numpy(), lr.detach().numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(p.detach().cpu().numpy(), pr.detach().numpy(), rtol=1e-5, atol=1e-6)
    ((l * g1.to(device)).sum() + (p * g2.to(device)).sum()).backward()
    np.testing.assert_allclose(fd.grad.cpu().numpy(), fr.grad.numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(kd.grad.cpu().numpy(), kr.grad.numpy(), rtol=1e-4, atol=1e-4 * max(1.0, float(kr.grad.abs().max())))


def test_sgd_kernel(device):
    from scan_amd import ops
    torch.manual_seed(0)
    p = torch.randn(1001)
    g = torch.randn(1001)
    pr = p.clone().requires_grad_(True)
    opt = torch.optim.SGD([pr], lr=0.01, momentum=0.9, weight_decay=1e-4)
    pd, buf = p.to(device), torch.zeros(1001, device=device)
    for it in range(3):
        pr.grad = g.clone() * (it + 1)
        opt.step()
        ops.sgd_momentum_(pd, (g * (it + 1)).to(device), buf, 0.01, 1e-4, 0.9, it == 0)
    np.testing.assert_allclose(pd.cpu().numpy(), pr.detach().numpy(), rtol=1e-6, atol=1e-7)


def test_maxpool2x2(device):
    from scan_amd import ops
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 64, 12, 20, generator=g)
    x[0, :, 0, 0] = x[0, :, 0, 1]  # exact ties inside a window: gradient goes to the first maximum
    xr = x.clone().requires_grad_(True)
    yr = F.max_pool2d(xr, 2, 2)
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy)
    rows, shape = _rows(x, device)
    rows.requires_grad_(True)
    y, oshape = ops.maxpool2x2(rows, shape)
    assert oshape.sizes == [(6, 10)]
    assert torch.equal(ops.rows_to_nchw(y.detach(), oshape).contiguous().cpu(), yr.detach())
    y.backward(_rows(gy, device)[0])
    assert torch.equal(ops.rows_to_nchw(rows.grad, shape).contiguous().cpu(), xr.grad)


@pytest.mark.parametrize("mode", ["fp32", "bf16x6", "bf16x3"])
def test_deferred_relu_backward_chain(device, monkeypatch, mode):
    """conv+ReLU -> conv+ReLU -> maxpool -> conv with the ReLU backward folded into the consumers' epilogues
    (ops.conv2d relu="deferred" / mask_dx, ops.maxpool2x2 relu_input) against the plain torch chain."""
    from scan_amd import ops
    monkeypatch.setattr(ops, "CONV_MODE", mode)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 8, 24, 40, generator=g)
    ws = [torch.randn(16, 8, 3, 3, generator=g) * 0.2, torch.randn(16, 16, 3, 3, generator=g) * 0.15,
          torch.randn(12, 16, 3, 3, generator=g) * 0.15]
    bs = [torch.randn(16, generator=g) * 0.1, torch.randn(16, generator=g) * 0.1, torch.randn(12, generator=g) * 0.1]
    xr = x.clone().requires_grad_(True)
    wr = [w.clone().requires_grad_(True) for w in ws]
    br = [b.clone().requires_grad_(True) for b in bs]
    h1 = F.relu(F.conv2d(xr, wr[0], br[0], padding=1))
    h2 = F.relu(F.conv2d(h1, wr[1], br[1], padding=1))
    # keep pre-activations away from 0 so rounding cannot flip a mask bit between the two implementations
    out_r = F.conv2d(F.max_pool2d(h2, 2, 2), wr[2], br[2], padding=1)
    gy = torch.randn(out_r.shape, generator=g)
    out_r.backward(gy)
    rows, shape = _rows(x, device)
    rows.requires_grad_(True)
    wd = [w.to(device).contiguous(memory_format=torch.channels_last).requires_grad_(True) for w in ws]
    bd = [b.to(device).requires_grad_(True) for b in bs]
    a1 = ops.conv2d(rows, wd[0], bd[0], shape, 3, 1, relu="deferred")
    a2 = ops.conv2d(a1, wd[1], bd[1], shape, 3, 1, relu="deferred", mask_dx=True)
    p, pshape = ops.maxpool2x2(a2, shape, relu_input=True)
    out = ops.conv2d(p, wd[2], bd[2], pshape, 3, 1)
    np.testing.assert_allclose(ops.rows_to_nchw(out.detach(), pshape, 0, 12).cpu().numpy(), out_r.detach().numpy(),
                               rtol=2e-4, atol=2e-4)
    out.backward(_rows(gy, device, out.shape[1])[0])
    tol = dict(rtol=2e-3, atol=2e-3)
    np.testing.assert_allclose(ops.rows_to_nchw(rows.grad, shape, 0, 8).cpu().numpy(), xr.grad.numpy(), **tol)
    for i in range(3):
        np.testing.assert_allclose(wd[i].grad.cpu().numpy(), wr[i].grad.numpy(), **tol)
        np.testing.assert_allclose(bd[i].grad.cpu().numpy(), br[i].grad.numpy(), **tol)


def test_resnet_stem_pool_and_residual_join(device):
    """F.max_pool2d(x, 3, 2, 1) (resnet.py:335) and out += identity; relu_ (resnet.py:312-313)."""
    from scan_amd import ops
    g = torch.Generator().manual_seed(21)
    for (h, w) in ((12, 20), (13, 17)):
        x = torch.randn(2, 64, h, w, generator=g)
        rows, shape = _rows(x, device)
        y, oshape = ops.maxpool3x3s2(rows, shape)
        ref = F.max_pool2d(x, 3, 2, 1)
        assert oshape.sizes == [tuple(ref.shape[-2:])]
        assert torch.equal(ops.rows_to_nchw(y, oshape).contiguous().cpu(), ref)
    with pytest.raises(RuntimeError, match="frozen"):
        ops.maxpool3x3s2(rows.clone().requires_grad_(True), shape)
    a, b = torch.randn(300, 64, generator=g), torch.randn(300, 64, generator=g)
    ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    yr = F.relu(ar + br)
    gy = torch.randn(300, 64, generator=g)
    yr.backward(gy)
    ad, bd = a.to(device).requires_grad_(True), b.to(device).requires_grad_(True)
    yd = ops.add_relu(ad, bd)
    assert torch.equal(yd.detach().cpu(), yr.detach())
    yd.backward(gy.to(device))
    assert torch.equal(ad.grad.cpu(), ar.grad) and torch.equal(bd.grad.cpu(), br.grad)


@pytest.mark.parametrize("mode", ["bf16x6", "bf16x3"])
@pytest.mark.parametrize("k,stride,hw,n", [(3, 1, (24, 40), 2), (3, 1, (17, 70), 1), (7, 2, (64, 96), 2), (7, 2, (37, 75), 1)])
def test_first_layer_conv_forward(device, k, stride, hw, n, mode, monkeypatch):
    """scan_conv_smallcin_bf16x6 / _bf16x3 (frozen first layers: VGG conv1_1 3x3/1, ResNet stem 7x7/2) against fp32 torch
    and against the generic fp32-MFMA kernel."""
    from scan_amd import ops
    monkeypatch.setattr(ops, "CONV_MODE", mode)
    g = torch.Generator().manual_seed(31 + k)
    x = torch.randn(n, 3, *hw, generator=g) * 50.0  # image-scale inputs
    w = torch.randn(64, 3, k, k, generator=g) / (3 * k * k) ** 0.5
    b = torch.randn(64, generator=g)
    ref = F.relu(F.conv2d(x, w, b, stride=stride, padding=k // 2))
    rows, shape = _rows(x, device, 4)
    wd = w.to(device).contiguous(memory_format=torch.channels_last)
    ops.kernel_timer.enabled = True
    ops.kernel_timer.reset()
    try:
        y = ops.conv2d(rows, wd, b.to(device), shape, k, stride, relu=True)
        assert "conv_smallcin_" + mode in ops.kernel_timer.records  # the dedicated kernel ran
    finally:
        ops.kernel_timer.enabled = False
        ops.kernel_timer.reset()
    oshape = shape.conv_out(k, stride)
    got = ops.rows_to_nchw(y, oshape, 0, 64).cpu()
    assert got.shape == ref.shape
    scale = ref.abs().max().item()
    bar = 2e-5 if mode == "bf16x3" else 2e-6
    assert (got - ref).abs().max().item() <= bar * scale
    monkeypatch.setattr(ops, "CONV_MODE", "fp32")
    y32 = ops.conv2d(rows, wd, b.to(device), shape, k, stride, relu=True)
    assert (y - y32).abs().max().item() <= bar * scale


def _sk_in0(pts, eps, min_samples=5):
    from sklearn import cluster
    return cluster.DBSCAN(eps=eps, min_samples=min_samples).fit_predict(pts) == 0


@pytest.mark.parametrize("gemm", ["bf16x3", "fp32"])
@pytest.mark.parametrize("case", ["blobs", "chain", "all_noise", "one_blob", "duplicates", "ragged_n", "borders"])
def test_dbscan_cluster0_matches_sklearn(device, case, gemm):
    """scan_dbscan_* against sklearn.cluster.DBSCAN labels: membership of cluster 0 (all the reference's selection uses,
    rpn/fcos/loss.py:417-421) must be identical point by point -- with the pairwise-distance GEMM on the bf16x3 path (the
    default) and on the exact fp32 matrix cores; pairs inside the rounding band of either are decided in fp64."""
    from scan_amd import _lib, ops
    import zlib
    rs = np.random.RandomState(zlib.crc32(case.encode()) % 100000)
    D, eps = 256, 3.0
    if case == "blobs":  # several dense blobs + uniform noise, shuffled
        centers = rs.randn(6, D) * 4
        pts = np.concatenate([c + rs.randn(300, D) * 0.12 for c in centers] + [rs.randn(200, D) * 4])
        pts = pts[rs.permutation(len(pts))]
    elif case == "chain":  # long thin cluster: many breadth-first levels
        t = np.linspace(0, 400, 1500)[:, None]
        d = np.zeros((1, D)); d[0, 0] = 1.0
        pts = t * d + rs.randn(1500, D) * 0.05
        pts = np.concatenate([pts, rs.randn(100, D) * 50])[rs.permutation(1600)]
    elif case == "all_noise":
        pts = rs.randn(500, D) * 10
    elif case == "one_blob":
        pts = rs.randn(700, D) * 0.1
    elif case == "duplicates":  # exact duplicates (d = 0) plus points just inside / just outside eps along one axis.
        # (A pair at EXACTLY eps is a coin toss inside sklearn itself: its fp64 |x|^2 + |y|^2 - 2 x.y carries 1e-12 of
        #  rounding noise either way -- probed on the host: 57 of 200 such pairs come out as non-neighbours.)
        base = rs.randn(40, D) * 5
        pts = np.repeat(base, 8, axis=0)
        pts[::16, 0] += eps - 1e-3
        pts[8::16, 0] += eps + 1e-3
    elif case == "ragged_n":  # n not a multiple of the 128 tile / 32-bit word
        centers = rs.randn(3, D) * 3
        pts = np.concatenate([c + rs.randn(211, D) * 0.15 for c in centers] + [rs.randn(30, D) * 6])
    else:  # borders: sparse ring of non-core points around a dense core, some reachable from two clusters
        a = rs.randn(200, D) * 0.05
        b = rs.randn(200, D) * 0.05; b[:, 0] += 5.0
        ring = rs.randn(60, D); ring = ring / np.linalg.norm(ring, axis=1, keepdims=True) * 2.8
        mid = rs.randn(10, D) * 0.01; mid[:, 0] += 2.5
        pts = np.concatenate([ring[:30], a, mid, b, ring[30:] + np.eye(1, D)[0] * 5.0])
    pts = pts.astype(np.float32)
    ref = _sk_in0(pts, eps)
    old = _lib.query("scan_tune", b"dbscan_bf16x3", 1 if gemm == "bf16x3" else 0)
    try:
        got = ops.dbscan_in_cluster0(torch.from_numpy(pts).to(device), eps, 5).cpu().numpy()
    finally:
        _lib.query("scan_tune", b"dbscan_bf16x3", old)
    assert got.shape == ref.shape
    assert np.array_equal(got, ref), "cluster-0 membership differs at %d of %d points" % ((got != ref).sum(), len(ref))


@pytest.mark.parametrize("cin,cout,hw", [(64, 64, (24, 48)), (128, 128, (32, 32)), (64, 128, (18, 34))])
def test_conv_relu_pool_fused(device, cin, cout, hw):
    """scan_conv3x3_pool2_bf16x3 (frozen VGG stages): conv + bias + ReLU + 2x2 max-pool in one launch equals the two
    separate ops, for both kernel instances (Cout <= 64 / > 64) and partial tiles."""
    from scan_amd import ops
    g = torch.Generator().manual_seed(cin + cout)
    x = torch.randn(2, cin, *hw, generator=g)
    w = (torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5)
    b = torch.randn(cout, generator=g)
    ref = F.max_pool2d(F.relu(F.conv2d(x, w, b, padding=1)), 2, 2)
    rows, shape = _rows(x, device)
    wd = w.to(device).contiguous(memory_format=torch.channels_last)
    assert ops.conv_pool_fusable(rows, wd, b.to(device), shape)
    y = ops.conv2d(rows, wd, b.to(device), shape, 3, 1, relu=True, pool=True)
    pshape = ops.PyramidShape(2, [(hw[0] // 2, hw[1] // 2)])
    got = ops.rows_to_nchw(y, pshape, 0, cout).cpu()
    assert got.shape == ref.shape
    assert (got - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()
    # identical to the unfused HIP ops bit for bit (same accumulators, max commutes with the monotone epilogue)
    y2, _ = ops.maxpool2x2(ops.conv2d(rows, wd, b.to(device), shape, 3, 1, relu=True), shape)
    assert torch.equal(y, y2)
    with pytest.raises(RuntimeError, match="forward-only"):
        ops.conv2d(rows.clone().requires_grad_(True), wd, b.to(device), shape, 3, 1, relu=True, pool=True)


def test_dgrad_remainder_split_full_size(device):
    """data gradient of a 264-channel input at discriminator-P3 size (K = 512, M = 100,352): the library plans the 8 remainder
    output channels as a second launch of the 64-channel instance (scan_conv_plan: rem = 8 after a 256-channel main part) and
    scan_conv_run makes exactly those two launches -- the result equals, bit for bit, two hand-made scan_conv3x3_bf16x6 calls
    on hand-split mode-1 planes, and agrees with the independent fp32-MFMA kernel."""
    import ctypes
    from scan_amd import _lib, ops
    g = torch.Generator().manual_seed(77)
    shape = ops.PyramidShape(1, [(224, 448)])
    x = torch.randn(shape.rows, 264, generator=g).to(device).requires_grad_(True)
    w = (torch.randn(512, 264, 3, 3, generator=g) / (264 * 9) ** 0.5).to(device).contiguous(memory_format=torch.channels_last)
    gy = torch.randn(shape.rows, 512, generator=g).to(device)
    assert ops.split_pieces() == 3
    plan = _lib.ConvPlan()
    _lib.call("scan_conv_plan", 3, 9, 1, 512, 264, 512, shape.ref(), 0, ctypes.byref(plan))
    assert (plan.rem, plan.nout - plan.rem, plan.family, plan.split_mode, plan.plane_taps, plan.csw) == (8, 256, 0, 1, 9, 512)
    ops.conv2d(x, w, None, shape, 3, 1).backward(gy)
    # by hand: flipped + transposed planes [264][9][512], Nout 256 from their start, Nout 8 from row 256 on into column 256 on
    wp = ops.pack_weight(w, 264)
    planes = [torch.empty((264, 9, 512), dtype=torch.bfloat16, device=device) for _ in range(3)]
    vp = ctypes.c_void_p
    _lib.call("scan_weight_split3", vp(wp.data_ptr()), 512, 9, 264, 1, *[vp(t.data_ptr()) for t in planes], 512, None)
    hand = torch.empty((shape.rows, 264), device=device)
    for nout, first in ((256, 0), (8, 256)):
        _lib.call("scan_conv3x3_bf16x6", vp(gy.data_ptr()), shape.ref(), 512, *[vp(t.data_ptr() + first * 9 * 512 * 2) for t in planes],
                  512, None, None, vp(hand.data_ptr() + first * 4), nout, 264, 0, None)
    assert torch.equal(x.grad, hand)
    dx = x.grad.clone()
    x.grad = None
    keep = ops.CONV_MODE
    ops.CONV_MODE = "fp32"
    try:
        ops.conv2d(x, w, None, shape, 3, 1).backward(gy)
    finally:
        ops.CONV_MODE = keep
    ref = x.grad
    assert (dx - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()  # two fp32 summation orders over K = 4608


@pytest.mark.parametrize("sizes", [[(16, 32), (8, 16), (4, 8), (2, 4), (1, 2)], [(9, 21)]])
def test_groupnorm_sums_from_conv_epilogue(device, sizes):
    """scan_conv3x3_gn_bf16x3 + scan_groupnorm_stats_from_sums: the GroupNorm statistics accumulated by the conv
    epilogue give the same normalised output (and the same gradients) as the separate statistics pass."""
    from scan_amd import ops
    g = torch.Generator().manual_seed(3)
    xs = [torch.randn(2, 256, h, w, generator=g) for h, w in sizes]
    rows, shape = _pyr(xs, device)
    w = (torch.randn(256, 256, 3, 3, generator=g) / 48).to(device).contiguous(memory_format=torch.channels_last)
    b = torch.randn(256, generator=g).to(device)
    gamma = (1 + 0.1 * torch.randn(256, generator=g)).to(device)
    beta = (0.1 * torch.randn(256, generator=g)).to(device)
    outs = []
    for fused in (False, True):
        r = rows.clone().requires_grad_(True)
        wv, bv = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        gv, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        y = ops.groupnorm_relu(ops.conv2d(r, wv, bv, shape, 3, 1, gn_sums=fused), gv, bt, shape)
        assert not ops._gn_sums  # the hand-over was consumed
        (y * y).sum().backward()
        outs.append((y.detach(), r.grad, wv.grad, gv.grad, bt.grad))
    for a, c in zip(*outs):
        assert (a - c).abs().max().item() <= 2e-5 * max(1.0, c.abs().max().item())


def test_nchw_drop_in_modules(device):
    """a tower written like the reference writes it -- nn.Sequential of Conv2d(256, 256, 3, stride=1, padding=1),
    GroupNorm(32, 256), ReLU (rpn/fcos/fcos.py:25-49) -- on NCHW tensors, with scan_amd.layers classes swapped in for
    torch.nn's, plus F.conv2d-style dynamic conv + softmax (condgraph.py:619-629): outputs and every gradient against
    the same module built from torch.nn on the CPU."""
    from scan_amd import layers as L
    torch.manual_seed(11)

    def tower(conv, gn):
        return nn.Sequential(conv(256, 256, kernel_size=3, stride=1, padding=1), gn(32, 256), nn.ReLU(),
                             conv(256, 8, kernel_size=3, stride=1, padding=1))

    ref = tower(nn.Conv2d, nn.GroupNorm)
    mine = tower(L.Conv2d, L.GroupNorm).to(device)
    mine.load_state_dict(ref.state_dict())
    x = torch.randn(2, 256, 20, 28)
    xr = x.clone().requires_grad_(True)
    xm = x.to(device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    yr, ym = ref(xr), mine(xm)
    assert ym.shape == yr.shape == (2, 8, 20, 28)
    np.testing.assert_allclose(ym.detach().cpu().numpy(), yr.detach().numpy(), rtol=1e-4, atol=1e-4)
    gy = torch.randn_like(yr)
    yr.backward(gy)
    ym.backward(gy.to(device))
    np.testing.assert_allclose(xm.grad.cpu().numpy(), xr.grad.numpy(), rtol=1e-3, atol=1e-4 * float(xr.grad.abs().max()))
    for (n, pr), (_, pm) in zip(ref.named_parameters(), mine.named_parameters()):
        np.testing.assert_allclose(pm.grad.cpu().numpy(), pr.grad.numpy(), rtol=1e-3,
                                   atol=2e-4 * float(pr.grad.abs().max()), err_msg=n)
    # semantic-conditioned dynamic conv on NCHW features
    f = torch.randn(2, 256, 12, 20)
    kp = torch.randn(9, 256) * 0.1
    lg, pb = L.dynamic_conv_softmax(f.to(device), kp.to(device))
    lr = F.conv2d(f, kp.view(9, 256, 1, 1))
    np.testing.assert_allclose(lg.cpu().numpy(), lr.numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(pb.cpu().numpy(), lr.softmax(1).numpy(), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("backend", ["compiled", "python"])
def test_nchw_modules_followed_by_inplace_relu(device, backend):
    """the reference follows its convolutions with nn.ReLU(inplace=True) (backbone/mmdetection/vgg.py:29,
    modeling/make_layers.py:74,117) and GroupNorm with an in-place ReLU in the towers written with make_conv3x3: the drop-in
    modules' outputs must be tensors an in-place op may modify on BOTH operator backends (the C++ nodes return row matrices,
    the NCHW view is taken outside apply()).  Outputs and gradients against torch.nn on the CPU; GroupNorm(16, C) and
    affine=False are refused instead of silently normalised over 32 groups."""
    import importlib
    import scan_amd.layers as L
    old = os.environ.get("SCAN_OPS_BACKEND")
    try:
        if backend == "python":
            os.environ["SCAN_OPS_BACKEND"] = "python"
        else:
            os.environ.pop("SCAN_OPS_BACKEND", None)
        L = importlib.reload(L)
        assert L.OPS_BACKEND == backend
        torch.manual_seed(3)

        def block(conv, gn):
            return nn.Sequential(conv(64, 256, kernel_size=3, stride=1, padding=1), nn.ReLU(inplace=True),
                                 conv(256, 256, kernel_size=1), gn(32, 256), nn.ReLU(inplace=True),
                                 conv(256, 5, kernel_size=3, stride=1, padding=1), nn.ReLU(inplace=True))

        ref, mine = block(nn.Conv2d, nn.GroupNorm), block(L.Conv2d, L.GroupNorm).to(device)
        mine.load_state_dict(ref.state_dict())
        x = torch.randn(2, 64, 12, 20)
        xr = x.clone().requires_grad_(True)
        xm = x.to(device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        yr, ym = ref(xr), mine(xm)
        np.testing.assert_allclose(ym.detach().cpu().numpy(), yr.detach().numpy(), rtol=1e-4, atol=1e-4)
        gy = torch.randn_like(yr)
        yr.backward(gy)
        ym.backward(gy.to(device))
        np.testing.assert_allclose(xm.grad.cpu().numpy(), xr.grad.numpy(), rtol=1e-3, atol=2e-4 * float(xr.grad.abs().max()))
        for (n, pr), (_, pm) in zip(ref.named_parameters(), mine.named_parameters()):
            np.testing.assert_allclose(pm.grad.cpu().numpy(), pr.grad.numpy(), rtol=1e-3,
                                       atol=2e-4 * float(pr.grad.abs().max()), err_msg=n)
        with pytest.raises(RuntimeError):
            L.GroupNorm(16, 256).to(device)(xm.new_zeros(1, 256, 4, 4))
        with pytest.raises(RuntimeError):
            L.GroupNorm(32, 256, affine=False).to(device)(xm.new_zeros(1, 256, 4, 4))
    finally:
        if old is None:
            os.environ.pop("SCAN_OPS_BACKEND", None)
        else:
            os.environ["SCAN_OPS_BACKEND"] = old
        importlib.reload(L)


def test_compiled_ops_weight_plane_cache_follows_parameter_updates(device):
    """scan_ops._ops keeps the three bf16 planes of a weight across calls (a reference-shaped graph calls one conv once per
    pyramid level).  They must be re-split whenever the parameter changed: an in-place torch update (what torch.optim.SGD and
    load_state_dict do: the version counter moves), and an update that bypasses torch followed by
    ops.invalidate_weight_planes() (what the engine's fused SGD does)."""
    from scan_amd import layers as L
    from scan_amd import ops
    if L.OPS_BACKEND != "compiled":
        pytest.skip("scan_ops._ops not built")
    torch.manual_seed(2)
    conv = L.Conv2d(256, 256, 3, 1, 1).to(device)
    conv.weight.data = conv.weight.data.contiguous(memory_format=torch.channels_last)
    x = torch.randn(1, 256, 16, 24, device=device).contiguous(memory_format=torch.channels_last)

    def fresh():  # the Python path splits on every call outside a weight epoch
        rows, shape, _ = L._to_rows(x)
        ops.invalidate_weight_planes()
        return L._to_nchw(ops.conv2d(rows, conv.weight, conv.bias, shape, 3, 1), shape, 256)

    L._ops.invalidate_weight_cache()
    y1 = conv(x)
    n1 = L._ops.weight_cache_size()
    assert n1 >= 1 and torch.equal(y1, fresh())
    assert torch.equal(conv(x), y1) and L._ops.weight_cache_size() == n1  # second call: served from the cache
    with torch.no_grad():
        conv.weight.mul_(1.5)  # torch in-place: version counter moves
    y2 = conv(x)
    assert torch.equal(y2, fresh()) and not torch.equal(y2, y1)
    # an update behind torch's back (raw pointer, like scan_sgd_momentum_multi on the flat buffers) + the invalidation call
    w = conv.weight.detach()
    ops.call("scan_scale", ops._ptr(w), 0.5, ops._ptr(w), w.numel(), ops._stream())
    ops.invalidate_weight_planes()
    assert L._ops.weight_cache_size() == 0
    y3 = conv(x)
    assert torch.equal(y3, fresh()) and not torch.equal(y3, y2)
    # backward through cached planes: same gradients as the Python path
    xg = x.clone().requires_grad_(True)
    conv(xg).square().sum().backward()
    gx, gw = xg.grad.clone(), conv.weight.grad.clone()
    conv.weight.grad = None
    xg2 = x.clone().requires_grad_(True)
    rows, shape, _ = L._to_rows(xg2)
    ops.invalidate_weight_planes()
    L._to_nchw(ops.conv2d(rows, conv.weight, conv.bias, shape, 3, 1), shape, 256).square().sum().backward()
    assert torch.equal(gx, xg2.grad) and torch.equal(gw, conv.weight.grad)


def test_compiled_ops_cpp_autograd_equals_python_path_and_torch(device):
    """scan_amd/ext/scan_ops/_ops (scan_amd/csrc/scan_ops_ext.cpp): conv2d, conv3x3_gn_relu, group_norm_relu and
    dynamic_conv_softmax as torch::autograd::Function nodes in C++ on the C ABI.  Same kernels as the Python autograd path of
    scan_amd.ops -> outputs and every gradient are bit-identical to it; and both agree with torch.nn on the CPU.  Cases: the
    tower block (rpn/fcos/fcos.py:36-49), a 1x1 lateral with stride 1 and 2 (backbone/fpn.py:52-66, resnet), 3x3 / stride 2
    (P6 / P7, fpn.py:118-130), a 265-channel input (head_out, condgraph.py:86-106), an 8-channel head without bias."""
    from scan_amd import layers as L
    from scan_amd import ops
    assert L.OPS_BACKEND == "compiled", "scan_amd/ext/scan_ops/_ops is missing: __graft_entry__.build() builds it"
    _ops = L._ops
    torch.manual_seed(5)

    def py_conv(x, w, b, k, s, relu):
        rows, shape, _ = L._to_rows(x)
        y = ops.conv2d(rows, w.contiguous(memory_format=torch.channels_last), b, shape, k, s, relu=relu)
        return L._to_nchw(y, shape.conv_out(k, s), w.shape[0])

    for (cin, cout, k, s, relu, bias, hw) in [(256, 256, 3, 1, True, True, (20, 28)), (512, 256, 1, 1, False, True, (9, 13)),
                                              (256, 128, 1, 2, True, True, (11, 15)), (256, 256, 3, 2, False, True, (7, 9)),
                                              (265, 256, 3, 1, True, True, (16, 24)), (256, 8, 3, 1, False, False, (8, 16))]:
        x = torch.randn(2, cin, *hw)
        w = torch.randn(cout, cin, k, k) * (2.0 / (cin * k * k)) ** 0.5
        b = torch.randn(cout) * 0.1 if bias else None
        gy = None
        res = []
        for path in ("cpp", "py", "cpu"):
            dev = "cpu" if path == "cpu" else device
            xx = x.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
            ww = w.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
            bb = b.to(dev).requires_grad_(True) if bias else None
            if path == "cpp":
                y = _ops.conv2d(xx, ww, bb, s, relu)
            elif path == "py":
                y = py_conv(xx, ww, bb, k, s, relu)
            else:
                y = F.conv2d(xx, ww, bb, s, k // 2)
                y = y.relu() if relu else y
            if gy is None:
                gy = torch.randn(*y.shape)
            y.backward(gy.to(dev))
            res.append((y.detach().cpu(), xx.grad.cpu(), ww.grad.cpu(), bb.grad.cpu() if bias else None))
        (yc, dxc, dwc, dbc), (yp, dxp, dwp, dbp), (yr, dxr, dwr, dbr) = res
        tag = (cin, cout, k, s)
        assert torch.equal(yc, yp) and torch.equal(dxc, dxp) and torch.equal(dwc, dwp), tag
        assert dbc is None or torch.equal(dbc, dbp), tag
        np.testing.assert_allclose(yc.numpy(), yr.numpy(), rtol=1e-4, atol=1e-4, err_msg=str(tag))
        np.testing.assert_allclose(dxc.numpy(), dxr.numpy(), rtol=1e-3, atol=1e-4 * float(dxr.abs().max()), err_msg=str(tag))
        np.testing.assert_allclose(dwc.numpy(), dwr.numpy(), rtol=1e-3, atol=2e-4 * float(dwr.abs().max()), err_msg=str(tag))
        if bias:
            np.testing.assert_allclose(dbc.numpy(), dbr.numpy(), rtol=1e-3, atol=2e-4 * float(dbr.abs().max()), err_msg=str(tag))

    # the tower block as ONE operator, against [Conv2d, GroupNorm, ReLU] from torch.nn and against the unfused compiled pair
    conv, gn = nn.Conv2d(256, 256, 3, 1, 1), nn.GroupNorm(32, 256)
    with torch.no_grad():
        gn.weight.uniform_(0.5, 1.5)
        gn.bias.normal_(0, 0.2)
    x = torch.randn(2, 256, 20, 28)
    gy = torch.randn(2, 256, 20, 28)
    xr = x.clone().requires_grad_(True)
    F.relu(gn(conv(xr))).backward(gy)
    import copy
    out = {}
    for name in ("fused", "pair", "python"):
        c, g = copy.deepcopy(conv).to(device), copy.deepcopy(gn).to(device)
        c.weight.data = c.weight.data.contiguous(memory_format=torch.channels_last)
        xm = x.to(device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        if name == "fused":
            y = _ops.conv3x3_gn_relu(xm, c.weight, c.bias, g.weight, g.bias, g.eps, True)
        elif name == "pair":
            y = _ops.group_norm_relu(_ops.conv2d(xm, c.weight, c.bias, 1, False), g.weight, g.bias, g.eps, True)
        else:
            rows, shape, _ = L._to_rows(xm)
            y = L._to_nchw(ops.groupnorm_relu(ops.conv2d(rows, c.weight, c.bias, shape, 3, 1, gn_sums=True), g.weight, g.bias, shape,
                                              relu=True, eps=g.eps), shape, 256)
        y.backward(gy.to(device))
        out[name] = [t.detach().cpu() for t in (y, xm.grad, c.weight.grad, c.bias.grad, g.weight.grad, g.bias.grad)]
    for a, b in zip(out["fused"], out["python"]):  # same kernels, same order: bit-identical
        assert torch.equal(a, b)
    refs = [F.relu(gn(conv(x))).detach(), xr.grad, conv.weight.grad, conv.bias.grad, gn.weight.grad, gn.bias.grad]
    for name in ("fused", "pair"):
        for i, (a, r) in enumerate(zip(out[name], refs)):
            np.testing.assert_allclose(a.numpy(), r.numpy(), rtol=1e-3, atol=3e-4 * float(r.abs().max()), err_msg="%s %d" % (name, i))
    # dynamic conv + softmax with gradients into both outputs
    f = torch.randn(2, 256, 12, 20)
    kp = torch.randn(9, 256) * 0.1
    g1, g2 = torch.randn(2, 9, 12, 20), torch.randn(2, 9, 12, 20)
    fr, kr = f.clone().requires_grad_(True), kp.clone().requires_grad_(True)
    lr = F.conv2d(fr, kr.view(9, 256, 1, 1))
    ((lr * g1).sum() + (lr.softmax(1) * g2).sum()).backward()
    got = {}
    for name in ("cpp", "py"):
        fm, km = f.to(device).contiguous(memory_format=torch.channels_last).requires_grad_(True), kp.to(device).requires_grad_(True)
        if name == "cpp":
            lg, pb = _ops.dynamic_conv_softmax(fm, km)
        else:
            rows, shape, _ = L._to_rows(fm)
            a, b = ops.dynconv_softmax(rows, km)
            lg, pb = (t.view(2, 12, 20, 9).permute(0, 3, 1, 2) for t in (a, b))
        ((lg * g1.to(device)).sum() + (pb * g2.to(device)).sum()).backward()
        got[name] = [t.detach().cpu() for t in (lg, pb, fm.grad, km.grad)]
    for a, b in zip(got["cpp"], got["py"]):
        assert torch.equal(a, b)
    np.testing.assert_allclose(got["cpp"][0].numpy(), lr.detach().numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(got["cpp"][2].numpy(), fr.grad.numpy(), rtol=1e-3, atol=1e-4 * float(fr.grad.abs().max()))
    np.testing.assert_allclose(got["cpp"][3].numpy(), kr.grad.numpy(), rtol=1e-3, atol=2e-4 * float(kr.grad.abs().max()))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        _ops.conv2d(torch.zeros(1, 4, 8, 8), torch.zeros(8, 4, 3, 3), None, 1, False)


# ----------------------------------------------------------------------------- many-tensor launches (csrc/batched.hip)
@pytest.mark.parametrize("pieces", [3, 2])
def test_weight_split_batched_equals_single_launches(device, pieces):
    """scan_weight_split_batched over a table of jobs writes bit for bit the planes scan_weight_split / scan_weight_split3
    write one weight at a time (both modes, 3x3 and 1x1, channel counts that need row padding); three pieces reassemble the
    fp32 weight EXACTLY (8 + 8 + 8 significand bits), two pieces to 2^-16."""
    from scan_amd import _lib, ops
    g = torch.Generator().manual_seed(21)
    jobs, expect, rows, off = [], [], [], 0
    for (O, T, Cs) in [(256, 9, 256), (128, 9, 64), (8, 9, 256), (256, 1, 512), (1024, 9, 264), (12, 9, 268), (64, 9, 4)]:
        w = torch.randn(O, T, Cs, generator=g).to(device)
        w[0, 0, :4] = torch.tensor([1e-30, -3.0e38, 1.0 + 2.0 ** -23, 0.0])  # tiny, huge, a one-ulp tail, zero
        for mode in (0, 1):
            nrows = O if mode == 0 else Cs
            csw = ops._round8(Cs if mode == 0 else O)
            planes = [torch.zeros((nrows, T, csw), dtype=torch.bfloat16, device=device) for _ in range(pieces)]
            exp = [torch.empty_like(planes[0]) for _ in range(pieces)]
            if pieces == 3:
                _lib.call("scan_weight_split3", ops._ptr(w), O, T, Cs, mode, *[ops._ptr(t) for t in exp], csw, ops._stream())
            else:
                _lib.call("scan_weight_split", ops._ptr(w), O, T, Cs, mode, ops._ptr(exp[0]), ops._ptr(exp[1]), csw, ops._stream())
            rows.append([w.data_ptr(), planes[0].data_ptr(), planes[1].data_ptr(), O, T, Cs, mode, nrows, csw, off,
                         planes[2].data_ptr() if pieces == 3 else 0])
            off += _lib.query("scan_weight_split_job_blocks", O, T, Cs, mode, csw)
            jobs.append((w, mode, planes))
            expect.append(exp)
    table = torch.tensor(rows, dtype=torch.int64).to(device)
    assert table.shape[1] == _lib.SPLIT_JOB_WORDS
    _lib.call("scan_weight_split_batched", ops._ptr(table), len(rows), table.shape[1], off, ops._stream())
    torch.cuda.synchronize()
    for (w, mode, planes), exp in zip(jobs, expect):
        for a, e in zip(planes, exp):
            assert torch.equal(a.view(torch.int16), e.view(torch.int16))
        total = sum(t.double() for t in planes)
        O, T, Cs = w.shape
        ref = w.double() if mode == 0 else w.double().flip(1).permute(2, 1, 0)
        got = total[:, :, :ref.shape[2]]
        if pieces == 3:
            assert torch.equal(got, ref)  # the three-piece split is exact
        else:
            assert float(((got - ref).abs() / ref.abs().clamp_min(1e-30)).max()) <= 2.0 ** -16
        assert float(total[:, :, ref.shape[2]:].abs().sum()) == 0  # row padding
    with pytest.raises(RuntimeError):
        _lib.call("scan_weight_split_batched", ops._ptr(table), 0, table.shape[1], off, ops._stream())
    with pytest.raises(RuntimeError, match="records of 10 words"):  # a table of the round-3 layout is refused, not misread
        _lib.call("scan_weight_split_batched", ops._ptr(table), len(rows), 10, off, ops._stream())


def test_split_plan_resplits_after_parameter_update(device):
    """ops.SplitPlan: the second begin_weight_epoch re-splits every recorded weight in one launch, from the CURRENT
    parameter values, and the conv that follows uses those planes (same output as without a plan)."""
    from scan_amd import ops
    g = torch.Generator().manual_seed(22)
    x, shape = _rows(torch.randn(2, 64, 24, 40, generator=g), device)
    w = (torch.randn(64, 64, 3, 3, generator=g) / 24).to(device).contiguous(memory_format=torch.channels_last)
    w.requires_grad_(True)
    w._scan_flat = True
    plan = ops.SplitPlan()
    try:
        ops.begin_weight_epoch(plan)
        xr = x.clone().requires_grad_(True)
        y0 = ops.conv2d(xr, w, None, shape)
        y0.sum().backward()
        assert len(plan.jobs) == 2  # forward and data-gradient planes of the one weight
        with torch.no_grad():
            w.mul_(-0.5)
        ops.begin_weight_epoch(plan)
        assert len(ops._split_cache) == 2  # both planes are ready before any conv ran
        with torch.no_grad():
            y1 = ops.conv2d(x, w, None, shape)
        assert len(plan.jobs) == 2 and not plan.dirty
    finally:
        ops.invalidate_weight_planes()
    with torch.no_grad():
        y2 = ops.conv2d(x, w, None, shape)  # no plan, no cache
    assert torch.equal(y1, y2)
    y0 = y0.detach()
    assert (y1 + 0.5 * y0).abs().max().item() <= 1e-5 * y0.abs().max().item()
    del w, xr
    ops.begin_weight_epoch(plan)  # the parameter died: its jobs are dropped, nothing is launched on freed memory
    assert not plan.jobs
    ops.invalidate_weight_planes()


def test_sgd_multi_equals_single_launches(device):
    from scan_amd import ops
    torch.manual_seed(3)
    specs = [(100003, 0.01, 5e-4, False), (7, 0.02, 0.0, False), (4096, 0.003, 1e-4, True), (0, 0.1, 0.0, False),
             (250000, 0.01, 5e-4, True)] * 8  # 40 segments: more than one launch's table
    segs, refs = [], []
    for n, lr, wd, first in specs:
        p, g, m = torch.randn(n, device=device), torch.randn(n, device=device), torch.randn(n, device=device)
        pr, mr = p.clone(), m.clone()
        if n:
            ops.sgd_momentum_(pr, g, mr, lr, wd, 0.9, first)
        segs.append((p, g, m, lr, wd, first))
        refs.append((pr, mr))
    ops.sgd_momentum_multi_(segs, 0.9)
    for (p, g, m, *_), (pr, mr) in zip(segs, refs):
        assert torch.equal(p, pr) and torch.equal(m, mr)


@pytest.mark.parametrize("cf,channels_last", [(8, True), (8, False), (1, True)])
def test_cka_stacked_weights_equal_torch_construction(device, cf, channels_last):
    """ops.cka_stacked_weights (one launch each way) against the stack / slice / eye / cat construction it replaces:
    same stacked weights, same parameter gradients -- returned to autograd and accumulated into flat buffers."""
    from scan_amd import ops
    from scan_amd.modeling.discriminator import FCOSDiscriminator_con
    torch.manual_seed(31)
    dis = FCOSDiscriminator_con(num_convs=1, in_channels=256, num_classes=cf + 1).to(device)
    blocks = [getattr(dis, "classifier_cls_%d" % c) for c in range(cf)]
    for b in blocks:
        for m in (b[0], b[2]):
            nn.init.normal_(m.weight, std=0.1)
            nn.init.normal_(m.bias, std=0.1)
            if not channels_last:
                m.weight.data = m.weight.data.contiguous()
    cs1 = ops.pad4(256 + cf)
    w1, b1, w2, b2 = ops.cka_stacked_weights([(b[0], b[2]) for b in blocks], 256, 128, cs1)
    rw1, rb1, rw2, rb2 = dis._stacked_weights_torch()
    assert w1.shape == (cf * 128, cs1, 3, 3) and w1.permute(0, 2, 3, 1).is_contiguous()
    assert torch.equal(w1[:, :256 + cf], rw1) and float(w1[:, 256 + cf:].abs().sum()) == 0
    assert torch.equal(b1, rb1) and torch.equal(w2, rw2) and torch.equal(b2, rb2)
    cot = [torch.randn_like(t) for t in (w1, b1, w2, b2)]
    params = [p for b in blocks for p in (b[0].weight, b[0].bias, b[2].weight, b[2].bias)]
    ref = torch.autograd.grad([rw1, rb1, rw2, rb2], params, [cot[0][:, :256 + cf], cot[1], cot[2], cot[3]])
    got = torch.autograd.grad([w1, b1, w2, b2], params, cot)
    for a, r in zip(got, ref):
        assert torch.equal(a, r)
    # parameters living in flat buffers: the backward adds into .grad and hands autograd nothing
    for p in params:
        p.grad = torch.ones_like(p)
        p._scan_flat = True
    w1, b1, w2, b2 = ops.cka_stacked_weights([(b[0], b[2]) for b in blocks], 256, 128, cs1)
    torch.autograd.backward([w1, b1, w2, b2], cot)
    for p, r in zip(params, ref):
        assert torch.equal(p.grad, 1 + r)


@pytest.fixture(params=[0, 1], ids=["fma", "mfma"])
def gconv_kernels(request):
    """both implementations of the grouped class-branch conv (scan_tune "gconv_mfma")"""
    from scan_amd import _lib
    old = _lib.query("scan_tune", b"gconv_mfma", request.param)
    assert old >= 0
    yield request.param
    _lib.query("scan_tune", b"gconv_mfma", old)


@pytest.mark.parametrize("G,sizes", [(8, [(16, 24), (8, 12), (3, 5)]), (8, [(40, 64)]), (1, [(12, 20), (5, 7)]), (2, [(9, 9)])])
def test_grouped_conv_to_one_channel_per_group(device, G, sizes, gconv_kernels):
    """scan_gconv3x3_to1_*: the class branches' second conv (nn.Conv2d(128, 1, 3, padding=1) per class, reference
    fcos_head_discriminator_con.py:44-62) for all classes at once, against F.conv2d(groups=G) on the CPU -- forward,
    the ReLU-masked data gradient, the weight gradient (diagonal blocks only) and the bias gradient."""
    from scan_amd import ops
    g = torch.Generator().manual_seed(41 + G)
    N, gc = 2, G * 128
    xs = [torch.relu(torch.randn(N, gc, h, w, generator=g)) for h, w in sizes]
    wg = torch.randn(G, 128, 3, 3, generator=g) / 30
    bg = torch.randn(G, generator=g)
    # stacked weight: the per-group weights on the diagonal blocks, junk elsewhere (must be ignored)
    ws = torch.randn(G, gc, 3, 3, generator=g)
    for c in range(G):
        ws[c, c * 128:(c + 1) * 128] = wg[c]
    rows, shape = _pyr(xs, device)
    rows.requires_grad_(True)
    wd = ws.to(device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    bd = bg.to(device).requires_grad_(True)
    y = ops.gconv3x3_to1(rows, wd, bd, shape, G, mask_dx=True)
    assert y.shape == (shape.rows, ops.pad4(G)) and float(y[:, G:].abs().sum()) == 0
    gys = [torch.randn(N, G, h, w, generator=g) for h, w in sizes]
    gy_rows, _ = _pyr([F.pad(t, (0, 0, 0, 0, 0, ops.pad4(G) - G)) for t in gys], device)
    y.backward(gy_rows)
    wr, br = wg.clone().requires_grad_(True), bg.clone().requires_grad_(True)
    dx_ref = []
    for l, x in enumerate(xs):
        xr = x.clone().requires_grad_(True)
        yr = F.conv2d(xr, wr, br, padding=1, groups=G)
        got = ops.rows_to_nchw(y.detach(), shape, l, G).cpu()
        np.testing.assert_allclose(got.numpy(), yr.detach().numpy(), rtol=1e-4, atol=1e-5)
        yr.backward(gys[l])
        dx_ref.append(xr.grad * (x > 0))  # the producer's deferred ReLU: the consumer masks its dx
    for l, r in enumerate(dx_ref):
        got = ops.rows_to_nchw(rows.grad, shape, l, gc).cpu()
        np.testing.assert_allclose(got.numpy(), r.numpy(), rtol=1e-4, atol=1e-5)
    dw = wd.grad.cpu()
    for c in range(G):
        np.testing.assert_allclose(dw[c, c * 128:(c + 1) * 128].numpy(), wr.grad[c].numpy(), rtol=2e-4,
                                   atol=2e-5 * float(wr.grad.abs().max()))
        off = torch.cat([dw[c, :c * 128], dw[c, (c + 1) * 128:]], 0)
        assert float(off.abs().sum()) == 0  # exact zeros off the diagonal
    np.testing.assert_allclose(bd.grad.cpu().numpy(), br.grad.numpy(), rtol=2e-4, atol=1e-4)
    # the C entry points that take the mask from x itself / apply none, against the bit-mask path above
    from scan_amd import _lib
    P, st = ops._ptr, ops._stream()
    wsb = torch.empty((_lib.query("scan_gconv3x3_to1_ws_floats", shape.ref(), G, 128),), device=device)
    wpk = wd.detach().permute(0, 2, 3, 1).contiguous()
    xr_, gyr = rows.detach(), gy_rows.contiguous()
    dx1, dx0, dwb = torch.empty_like(xr_), torch.empty_like(xr_), torch.zeros_like(wpk)
    _lib.call("scan_gconv3x3_to1_backward", P(xr_), P(gyr), ops.pad4(G), shape.ref(), G, 128, P(wpk), 1, P(dx1), P(dwb), 0,
              P(wsb), st)
    _lib.call("scan_gconv3x3_to1_dgrad", P(gyr), ops.pad4(G), shape.ref(), G, 128, P(wpk), None, P(dx0), st)
    assert (dx1 - rows.grad).abs().max().item() <= 1e-5 * max(1.0, rows.grad.abs().max().item())
    assert (dx0 * (xr_ > 0) - rows.grad).abs().max().item() <= 1e-5 * max(1.0, rows.grad.abs().max().item())
    assert (dwb.view(G, 3, 3, gc).permute(0, 3, 1, 2) - wd.grad).abs().max().item() <= 1e-5 * max(1.0, wd.grad.abs().max().item())


def test_discriminator_grouped_branch_equals_dense_branch(device):
    """FCOSDiscriminator_con with the grouped second conv and the one-launch weight stacking against the dense
    block-diagonal conv and the torch construction: same loss, same gradients (bf16x3 vs fp32-FMA rounding apart)."""
    from scan_amd import ops
    from scan_amd.modeling.discriminator import FCOSDiscriminator_con
    torch.manual_seed(5)
    dis = FCOSDiscriminator_con(num_convs=2, in_channels=256, num_classes=9).to(device)
    for m in dis.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.normal_(m.weight, std=0.05)
    shape = ops.PyramidShape(2, [(24, 40)])
    feat = torch.randn(shape.rows, 256, device=device)
    act = torch.softmax(torch.randn(shape.rows, 9, device=device), 1)
    res = []
    for flag in (True, False):
        ops.GROUPED_CLS = ops.BATCHED = flag
        try:
            f = feat.clone().requires_grad_(True)
            dis.zero_grad()
            ls, lt = dis.forward_pair(f, act, shape, 1)
            (ls + 2 * lt).backward()
            res.append([ls.detach(), lt.detach(), f.grad] + [p.grad.clone() for p in dis.parameters()])
        finally:
            ops.GROUPED_CLS = ops.BATCHED = True
    for a, b in zip(*res):
        assert (a - b).abs().max().item() <= 2e-4 * max(b.abs().max().item(), 1e-6), (a.shape, (a - b).abs().max().item())


def test_grouped_conv_adjoint_identities_full_size(device, gconv_kernels):
    """size-independent properties at the bench size (P3, 4 frames, 8 classes): the data gradient is the adjoint of the
    forward map in x, the weight gradient its adjoint in w -- <conv(x, w), g> = <x, dgrad(g, w)> = <w, wgrad(x, g)>
    (bias off), in fp64 on the host from fp32 device results."""
    from scan_amd import ops
    g = torch.Generator(device=device).manual_seed(9)
    G, shape = 8, ops.PyramidShape(4, [(128, 256)])
    x = torch.randn((shape.rows, G * 128), device=device, generator=g).requires_grad_(True)
    w = torch.zeros((G, G * 128, 3, 3), device=device)
    for c in range(G):
        w[c, c * 128:(c + 1) * 128] = torch.randn((128, 3, 3), device=device, generator=g) / 30
    w = w.contiguous(memory_format=torch.channels_last).requires_grad_(True)
    gy = torch.randn((shape.rows, 8), device=device, generator=g)
    y = ops.gconv3x3_to1(x, w, None, shape, G, mask_dx=False)
    y.backward(gy)
    lhs = float((y.detach().double() * gy.double()).sum())
    via_x = float((x.detach().double() * x.grad.double()).sum())
    via_w = float((w.detach().double() * w.grad.double()).sum())
    scale = float((y.detach().double().abs() * gy.double().abs()).sum())
    assert abs(lhs - via_x) <= 2e-6 * scale and abs(lhs - via_w) <= 2e-6 * scale, (lhs, via_x, via_w, scale)


def test_new_entry_points_reject_bad_arguments(device):
    """error behaviour of the round-2 entry points: a non-zero return with a message (RuntimeError on the Python side),
    never a launch on bad geometry"""
    from scan_amd import _lib, ops
    P, st = ops._ptr, ops._stream()
    shape = ops.PyramidShape(1, [(4, 4)])
    x = torch.zeros((16, 3 * 128), device=device)
    w = torch.zeros((3, 9, 3 * 128), device=device)
    y = torch.zeros((16, 4), device=device)
    ws = torch.zeros((1 << 16,), device=device)
    with pytest.raises(RuntimeError, match="G=3"):
        _lib.call("scan_gconv3x3_to1_forward", P(x), shape.ref(), 3, 128, P(w), None, P(y), 4, P(ws), st)
    with pytest.raises(RuntimeError, match="128 channels per group"):
        _lib.call("scan_gconv3x3_to1_forward", P(x), shape.ref(), 2, 64, P(w), None, P(y), 4, P(ws), st)
    with pytest.raises(RuntimeError, match="Ns"):
        _lib.call("scan_gconv3x3_to1_forward", P(x), shape.ref(), 2, 128, P(w), None, P(y), 1, P(ws), st)
    with pytest.raises(RuntimeError, match="null"):
        _lib.call("scan_gconv3x3_to1_backward", None, P(y), 4, shape.ref(), 2, 128, P(w), 1, P(x), P(w), 0, P(ws), st)
    br = (_lib.CkaBranch * 17)()
    with pytest.raises(RuntimeError, match="Cf=17"):
        _lib.call("scan_cka_stack_weights", br, 17, 256, 128, 1, 1, 1, 1, 1, 276, 17 * 128, P(w), P(w), P(w), P(w), st)
    br1 = (_lib.CkaBranch * 1)()
    with pytest.raises(RuntimeError, match="null pointer in branch 0"):
        _lib.call("scan_cka_stack_weights", br1, 1, 256, 128, 1, 1, 1, 1, 1, 260, 128, P(w), P(w), P(w), P(w), st)
    seg = (_lib.SgdSegment * 1)()
    with pytest.raises(RuntimeError, match="n_segs=0"):
        _lib.call("scan_sgd_momentum_multi", seg, 0, 0.9, st)
    seg[0].n = 8
    with pytest.raises(RuntimeError, match="null pointer in segment 0"):
        _lib.call("scan_sgd_momentum_multi", seg, 1, 0.9, st)
    with pytest.raises(RuntimeError, match="from_sums"):
        _lib.call("scan_groupnorm_relu_forward_from_sums", P(x), shape.ref(), 256, 32, None, 1e-5, P(x), P(x), 1, P(x), P(x), st)
    assert _lib.query("scan_tune", b"no_such_knob", 1) == _lib.TUNE_UNKNOWN


# ----------------------------------------------------------------------------- ground-truth plan (csrc/targets.hip)
@pytest.mark.parametrize("case", ["bench_like", "crowded_small_level", "one_box", "ragged_counts"])
def test_target_plan_kernels_equal_torch_plan(device, case):
    """scan_fcos_assign / _compact / _nodes against the torch spelling of the plan (modeling/fcos.py: assign_targets,
    source_node_index, centerness_targets -- the functions the CPU tests pin against the reference's label maps and node
    lists): labels, node index and node labels, positive rows bit-identical; regression and centerness targets of the
    positives bit-identical.  Cases: the bench geometry; boxes covering most of a small level (n_pos > n_neg on it, every
    background row taken); a single box; images with different box counts (padded slots must not be read)."""
    from scan_amd import synth
    from scan_amd.modeling import fcos
    g = torch.Generator().manual_seed(5)
    if case == "bench_like":
        H, W, N = 512, 1024, 2
        targets = synth.synth_targets(N, H, W, 8, 12, 4321)
    elif case == "crowded_small_level":
        H, W, N = 128, 256, 2
        big = torch.tensor([[2.0, 2.0, W - 3.0, H - 3.0], [10.0, 8.0, W - 20.0, H - 9.0]])
        targets = [(big.clone(), torch.tensor([3, 5])), (big[:1].clone(), torch.tensor([1]))]
    elif case == "one_box":
        H, W, N = 96, 160, 1
        targets = [(torch.tensor([[20.0, 16.0, 90.0, 70.0]]), torch.tensor([2]))]
    else:
        H, W, N = 256, 256, 3
        targets = []
        for n, k in enumerate((1, 7, 3)):
            xy = torch.rand(k, 2, generator=g) * 150
            wh = torch.rand(k, 2, generator=g) * 100 + 8
            targets.append((torch.cat([xy, xy + wh], 1), torch.randint(1, 9, (k,), generator=g)))
    targets = [(b.to(device), l.to(device)) for b, l in targets]
    shape = __import__("scan_amd.ops", fromlist=["PyramidShape"]).PyramidShape(
        N, [((H + s - 1) // s, (W + s - 1) // s) for s in fcos.FPN_STRIDES])
    dev_plan = fcos._build_plan_device(shape, targets, device)
    fcos.DEVICE_PLAN = False
    try:
        ref = fcos._build_plan(shape, targets, device)
    finally:
        fcos.DEVICE_PLAN = True
    torch.cuda.synchronize()
    assert torch.equal(dev_plan.labels, ref.labels) and torch.equal(dev_plan.labels_i32, ref.labels_i32)
    assert dev_plan.n_pos == ref.n_pos and dev_plan.n_pos > 0
    assert torch.equal(dev_plan.pos_inds, ref.pos_inds)
    assert torch.equal(dev_plan.node_index, ref.node_index), (dev_plan.node_index.shape, ref.node_index.shape)
    assert torch.equal(dev_plan.node_labels, ref.node_labels)
    assert torch.equal(dev_plan.reg_pos, ref.reg_pos)
    assert torch.equal(dev_plan.reg_targets[ref.pos_inds], ref.reg_targets[ref.pos_inds])
    assert torch.equal(dev_plan.ctr_pos.view(torch.int32), ref.ctr_pos.view(torch.int32))
    if case == "crowded_small_level":  # the branch "more positives than background rows" was really taken
        lab = ref.labels
        per_level = [(int((lab[shape.row_off[l]:shape.row_off[l + 1]] > 0).sum()), shape.row_off[l + 1] - shape.row_off[l])
                     for l in range(shape.n_levels)]
        assert any(p > r - p for p, r in per_level), per_level


# ----------------------------------------------------------------------------- in-place assembly / strided GroupNorm / FPN join
def test_upsample2x_add_and_backward(device):
    """ops.upsample2x_add = lateral + F.interpolate(coarse, scale_factor=2, 'nearest') (reference backbone/fpn.py:62-75);
    backward: the gradient itself for the lateral, its 2x2 window sums for the coarse map."""
    import torch.nn.functional as F
    from scan_amd import ops
    g = torch.Generator().manual_seed(31)
    n, h, w, C = 2, 5, 7, 256
    lat = torch.randn(n, C, 2 * h, 2 * w, generator=g, requires_grad=True)
    coarse = torch.randn(n, C, h, w, generator=g, requires_grad=True)
    ref = lat + F.interpolate(coarse, scale_factor=2, mode="nearest")
    up = torch.randn(n, C, 2 * h, 2 * w, generator=g)
    ref.backward(up)
    lr, ls = ops.nchw_to_rows(lat.detach().to(device))
    cr, cs = ops.nchw_to_rows(coarse.detach().to(device))
    lr.requires_grad_(True)
    cr.requires_grad_(True)
    y = ops.upsample2x_add(lr, cr, cs)
    y.backward(ops.nchw_to_rows(up.to(device))[0])
    assert torch.equal(ops.rows_to_nchw(y.detach(), ls).cpu(), ref.detach())
    assert torch.equal(ops.rows_to_nchw(lr.grad, ls).cpu(), lat.grad)
    np.testing.assert_allclose(ops.rows_to_nchw(cr.grad, cs).cpu().numpy(), coarse.grad.numpy(), rtol=1e-6, atol=1e-6)


def test_groupnorm_into_wider_matrix_and_cat_into(device):
    """groupnorm_relu(out_buf=...) + cat_into == torch.cat([groupnorm_relu(x), extra, 0-pad], 1), forward bit for bit and
    every gradient (the GroupNorm backward reads its column slice of the incoming gradient in place)."""
    from scan_amd import ops
    g = torch.Generator().manual_seed(32)
    shape = ops.PyramidShape(2, [(12, 20), (6, 10), (3, 5)])
    M = shape.rows
    x = torch.randn(M, 256, generator=g).to(device)
    gam, bet = (torch.rand(256, generator=g) + 0.5).to(device), torch.randn(256, generator=g).to(device)
    extra = torch.rand(M, 5, generator=g).to(device)
    w = torch.randn(M, 264, generator=g).to(device)  # weights of a scalar loss: a distinct gradient for every column
    res = []
    for in_place in (False, True):
        xs = [t.clone().requires_grad_(True) for t in (x, gam, bet, extra)]
        if in_place:
            buf = x.new_empty((M, 264))
            y = ops.groupnorm_relu(xs[0], xs[1], xs[2], shape, out_buf=buf)
            assert y.data_ptr() == buf.data_ptr() and y.stride() == (264, 1)
            cat = ops.cat_into(y, xs[3], buf)
        else:
            y = ops.groupnorm_relu(xs[0], xs[1], xs[2], shape)
            cat = torch.cat([y, xs[3], y.new_zeros(M, 3)], 1)
        (cat * w).sum().backward()
        res.append((cat.detach().clone(), [t.grad.clone() for t in xs]))
    assert torch.equal(res[0][0], res[1][0])
    for a, b in zip(res[0][1], res[1][1]):
        assert torch.allclose(a, b, rtol=1e-6, atol=1e-6), (a - b).abs().max().item()


def test_split_levels_grl_equals_split_then_grl(device):
    from scan_amd import ops
    g = torch.Generator().manual_seed(33)
    shape = ops.PyramidShape(2, [(8, 12), (4, 6), (2, 3)])
    rows = torch.randn(shape.rows, 12, generator=g).to(device)
    lams = [0.02, 0.1, 0.5]
    ups = [torch.randn(shape.row_off[l + 1] - shape.row_off[l], 12, generator=g).to(device) for l in range(3)]
    grads = []
    for fused in (False, True):
        r = rows.clone().requires_grad_(True)
        if fused:
            parts = ops.split_levels_grl(r, shape, lams)
        else:
            parts = [ops.grad_reverse(p, lam) for p, lam in zip(ops.split_levels(r, shape), lams)]
        for p, ref in zip(parts, ops.split_levels(rows, shape)):
            assert torch.equal(p.detach(), ref)
        sum((p * u).sum() for p, u in zip(parts[:2], ups[:2])).backward()  # level 2 unused: its rows get zeros
        grads.append(r.grad.clone())
    assert torch.equal(grads[0], grads[1])
    assert float(grads[1][shape.row_off[2]:].abs().sum()) == 0.0


@pytest.mark.parametrize("K,T", [(9, 3), (2, 3), (5, 2), (9, 1)])
def test_cond_rnn_fused_equals_torch_loop(device, K, T):
    """scan_cond_rnn_forward / _backward (paradigm -> 2-layer tanh RNN -> (T, 1) conv -> kernels [K, 256], reference
    condgraph.py:313-319) against the torch loop GRAPHModule.get_conded_weight spells out: values and the gradients of
    all ten parameters."""
    from scan_amd import ops
    from scan_amd.modeling import condgraph
    torch.manual_seed(100 * K + T)
    m = condgraph.GRAPHModule(256, K, proto_iter=T).to(device)
    with torch.no_grad():
        m.prototype.copy_(torch.randn(K, 256, T, device=device))
        for p in list(m.cond_rnn.parameters()) + list(m.cond_nx1.parameters()):
            p.copy_(torch.randn_like(p) * 0.05)
    params = list(m.cond_rnn.parameters()) + list(m.cond_nx1.parameters())
    dk = torch.randn(K, 256, device=device)
    res = {}
    for fused in (True, False):
        keep = ops.COND_RNN_FUSED
        ops.COND_RNN_FUSED = fused
        try:
            for p in params:
                p.grad = None
            ker = m.get_conded_weight()
            ker.backward(dk)
            res[fused] = (ker.detach().clone(), [p.grad.clone() for p in params])
        finally:
            ops.COND_RNN_FUSED = keep
    assert torch.allclose(res[True][0], res[False][0], rtol=1e-4, atol=1e-5)
    for (name, _), a, b in zip(list(m.cond_rnn.named_parameters()) + list(m.cond_nx1.named_parameters()), res[True][1], res[False][1]):
        scale = max(1.0, float(b.abs().max()))
        assert torch.allclose(a, b, rtol=1e-4, atol=2e-5 * scale), (name, float((a - b).abs().max()), scale)


def test_zero_pool_slices_are_cleared_every_epoch(device):
    """GroupNorm workspaces come from ops' pool: zero when handed out, again zero after the next begin_weight_epoch even if a
    kernel left sums in them, fresh (library-cleared) allocations outside an epoch or when the pool is exhausted."""
    from scan_amd import ops
    ops.begin_weight_epoch(None, device)
    try:
        a, cleared = ops._ws_f64(1000, device)
        assert cleared and float(a.abs().sum()) == 0.0
        a.fill_(3.0)
        b, cleared_b = ops._ws_f64(70, device)
        assert cleared_b and float(b.abs().sum()) == 0.0 and b.data_ptr() != a.data_ptr()
        z = ops._zeros_f32(18, device)
        z.fill_(1.0)
        ops.begin_weight_epoch(None, device)
        a2, _ = ops._ws_f64(1000, device)
        assert a2.data_ptr() == a.data_ptr() and float(a2.abs().sum()) == 0.0
        z2 = ops._zeros_f32(18, device)
        assert float(z2.abs().sum()) == 0.0 and float(z.sum()) == 18.0  # last epoch's loss accumulators are left alone
        big, cleared_big = ops._ws_f64(ops._ZERO_POOL_DOUBLES + 1, device)
        assert not cleared_big
    finally:
        ops.invalidate_weight_planes()
    c, cleared_c = ops._ws_f64(10, device)
    assert not cleared_c  # outside an epoch: the library call clears its workspace itself


@pytest.mark.parametrize("C,i0,i1", [(256, 0, 2), (9, 2, 4), (12, 1, 2), (8, 0, 4)])
def test_take_images_backward_one_pass(device, C, i0, i1):
    """ops.take_images: the sub-pyramid of images [i0, i1) and its gradient (scan_take_images_backward: copied rows, zeros
    elsewhere, one launch) against the slice-by-slice torch spelling."""
    from scan_amd import ops
    shape = ops.PyramidShape(4, [(16, 24), (8, 12), (4, 6), (2, 3), (1, 2)])
    torch.manual_seed(C + i0)
    x = torch.randn(shape.rows, C, device=device, requires_grad=True)
    y, sub = ops.take_images(x, shape, i0, i1)
    parts = [x[shape.row_off[l] + i0 * h * w:shape.row_off[l] + i1 * h * w] for l, (h, w) in enumerate(shape.sizes)]
    ref = torch.cat(parts, 0)
    assert sub.n_images == i1 - i0 and torch.equal(y.detach(), ref.detach())
    g = torch.randn_like(ref)
    y.backward(g)
    got = x.grad.clone()
    x.grad = None
    ref.backward(g)
    assert torch.equal(got, x.grad)


def test_round6_glue_kernels_equal_their_torch_spellings(device):
    """scan_copy_cols (F.pad of the act maps / the class-branch cat), scan_paradigm_update (condgraph.update_prototype_nx1_rnn) and
    the paired CKA loss node against the torch-tier spellings they replace."""
    from scan_amd import ops, synth
    from scan_amd.modeling import condgraph
    torch.manual_seed(9)
    # (a) pad_cols forward / backward == F.pad / its slice
    x = torch.randn(1000, 9, device=device, requires_grad=True)
    y = ops.pad_cols(x, 12)
    assert torch.equal(y, F.pad(x.detach(), (0, 3)))
    g = torch.randn(1000, 12, device=device)
    y.backward(g)
    assert torch.equal(x.grad, g[:, :9])
    # (b) cat_into: the extra columns + zero tail behind a tower output that already sits in the buffer
    buf = torch.randn(500, 268, device=device)
    keep = buf[:, :256].clone()
    yv = buf[:, :256]
    extra = torch.randn(500, 9, device=device)
    out = ops.cat_into(yv, extra[:, 1:], buf)
    assert torch.equal(out[:, :256], keep) and torch.equal(out[:, 256:264], extra[:, 1:]) and float(out[:, 264:].abs().max()) == 0.0
    # (c) the paradigm update, every counter value incl. the shifting one, with unseen classes (zero rows)
    mh_a, mh_b = condgraph.GRAPHModule(256, 9).to(device), condgraph.GRAPHModule(256, 9).to(device)
    sd = synth.middle_head_state_dict(9)
    mh_a.load_state_dict(sd)
    mh_b.load_state_dict(sd)
    for it in range(6):
        pb = torch.randn(9, 256, device=device)
        pb[(it + 2) % 9] = 0
        pb[7] = 0
        old = condgraph.FUSED_PARADIGM_UPDATE
        try:
            condgraph.FUSED_PARADIGM_UPDATE = True
            mh_a.update_prototype_nx1_rnn(pb)
            condgraph.FUSED_PARADIGM_UPDATE = False
            mh_b.update_prototype_nx1_rnn(pb)
        finally:
            condgraph.FUSED_PARADIGM_UPDATE = old
        np.testing.assert_allclose(mh_a.prototype.cpu().numpy(), mh_b.prototype.cpu().numpy(), rtol=2e-6, atol=2e-6, err_msg=str(it))
    # (d) the paired CKA loss == the two single losses on the halves, values and gradient bit for bit
    M, m, cf = 3000, 1400, 8
    logits = torch.randn(M, cf, device=device)
    act = torch.rand(M, cf + 1, device=device)
    l1 = logits.clone().requires_grad_(True)
    ls, lt = ops.cka_bce_pair(l1, act, m, cf)
    (0.3 * ls + 0.7 * lt).backward()
    l2 = logits.clone().requires_grad_(True)
    a, b = ops.split_rows2(l2, m)
    rs, rt = ops.cka_bce(a, act[:m], 1.0, cf), ops.cka_bce(b, act[m:], 0.0, cf)
    (0.3 * rs + 0.7 * rt).backward()
    assert torch.equal(ls, rs) and torch.equal(lt, rt) and torch.equal(l1.grad, l2.grad)

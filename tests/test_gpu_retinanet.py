"""RetinaNet head on the GPU: the plan kernels against the reference's fixtures (tests/golden/retinanet_*.npz), the torch
spelling and the fp64 restatement (tests/retinanet_ref.py); the smooth-L1 kernels against fp64; both losses and the
post-processor against the fixtures; the head against a torch-CPU restatement; one pass through the factory module."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import deform_ref
import retinanet_ref as R
from retinanet_ref import CASES, EDGE_CASES, edge_inputs, load_case

pytestmark = pytest.mark.gpu
CPU = torch.device("cpu")


def _inputs(gold_dir, which):
    """(N, sizes, targets, cells, bg, fg)"""
    from scan_amd.modeling import retinanet
    if which in CASES:
        f = load_case(gold_dir, which)
        return f["N"], f["sizes"], f["targets"], torch.from_numpy(f["cells"]), float(f["bg"]), float(f["fg"])
    n, sizes, targets, kw, bg, fg = edge_inputs(which)
    cells = retinanet.cell_anchors(aspect_ratios=kw.get("ratios", (0.5, 1.0, 2.0)), scales_per_octave=kw.get("scales_per_octave", 3))
    return n, sizes, targets, cells, bg, fg


@pytest.fixture(scope="module")
def references(gold_dir):
    """per input the torch spelling's plan on the CPU and the fp64 restatement's labels / matched / targets, computed once"""
    from scan_amd import ops
    from scan_amd.modeling import retinanet
    out = {}
    for which in CASES + EDGE_CASES:
        n, sizes, targets, cells, bg, fg = _inputs(gold_dir, which)
        plan = retinanet.build_plan(ops.PyramidShape(n, sizes), targets, CPU, cells=cells, bg=bg, fg=fg)
        tg = [(b.numpy(), l.numpy()) for b, l in targets]
        labels, matched, _ = R.match(n, sizes, tg, cells.numpy(), bg=bg, fg=fg)
        out[which] = (plan, labels, matched, R.targets64(n, sizes, tg, cells.numpy(), labels, matched))
    return out


# ----------------------------------------------------------------------------- 1. the plan kernels
@pytest.mark.parametrize("which", CASES + EDGE_CASES)
@pytest.mark.parametrize("host_targets", [True, False])
def test_plan_kernels_equal_reference_spelling_and_restatement(device, gold_dir, references, which, host_targets):
    from scan_amd import ops
    from scan_amd.modeling import retinanet
    n, sizes, targets, cells, bg, fg = _inputs(gold_dir, which)
    spelled, labels64, matched64, targets64 = references[which]
    shape = ops.PyramidShape(n, sizes)
    A = int(cells.shape[1])
    tg = targets if host_targets else [(b.to(device), l.to(device)) for b, l in targets]
    got = retinanet.build_plan(shape, tg, device, cells=cells, bg=bg, fg=fg)
    assert retinanet.plan_stats == {"launches": 2, "host_reads": 1}
    assert got.labels_i32.is_cuda and got.labels_i32.dtype == torch.int32 and got.labels_i32.numel() == shape.rows * A
    assert torch.equal(got.labels_i32.cpu(), spelled.labels_i32) and torch.equal(got.matched.cpu(), spelled.matched)
    assert np.array_equal(got.labels_i32.cpu().numpy(), labels64) and np.array_equal(got.matched.cpu().numpy(), matched64)
    assert got.n_pos == spelled.n_pos == int((labels64 > 0).sum())
    if which in CASES:
        f = load_case(gold_dir, which)
        assert np.array_equal(got.labels_i32.cpu().numpy(), f["labels"]) and np.array_equal(got.matched.cpu().numpy(), f["matched"])
        assert got.n_pos == int((f["labels"] > 0).sum())
    # targets_out of the smooth-L1 forward against fp64 on the positives, zero elsewhere
    reg = torch.zeros((shape.rows, 4 * A), device=device)
    t_out = torch.full((shape.rows * A, 4), 7.0, device=device)
    ops.retina_smooth_l1_loss(reg, shape, R.STRIDES, cells.to(device), got.boxes, got.labels_i32, got.matched, 0.11, targets_out=t_out)
    pos = labels64 > 0
    np.testing.assert_allclose(t_out.cpu().numpy()[pos], targets64[pos], rtol=1e-5, atol=1e-6)
    assert not t_out.cpu().numpy()[~pos].any()
    # bit-identical with the deterministic knob on (integer max and integer counter: order-independent)
    old = ops.set_deterministic(True)
    try:
        again = retinanet.build_plan(shape, tg, device, cells=cells, bg=bg, fg=fg)
    finally:
        ops.set_deterministic(old)
    assert torch.equal(got.labels_i32, again.labels_i32) and torch.equal(got.matched, again.matched) and got.n_pos == again.n_pos


def test_plan_is_cached_per_batch_and_built_on_a_side_stream(device, gold_dir):
    from scan_amd import ops
    from scan_amd.modeling import fcos, retinanet
    f = load_case(gold_dir, CASES[1])
    shape = ops.PyramidShape(f["N"], f["sizes"])
    fcos.reset_target_plan()
    side = ops.borrow_side_streams(3)[0]
    p = retinanet.target_plan(shape, f["targets"], device, side_stream=side)
    assert p.ready is not None and retinanet.target_plan(shape, f["targets"], device) is p
    torch.cuda.synchronize()
    assert np.array_equal(p.labels_i32.cpu().numpy(), f["labels"])
    fcos.reset_target_plan()
    assert retinanet.target_plan(shape, f["targets"], device) is not p


# ----------------------------------------------------------------------------- 2. smooth-L1
def _smooth_l1_case(gold_dir, kind):
    """(N, sizes, targets, cells, bg, fg, beta): 0 positives (no boxes at all), exactly 1 (A = 1; the box IS one anchor, so its
    target is exactly zero and a zero prediction has d = 0 in every precision), the 64x96 fixture's 59"""
    from scan_amd.modeling import retinanet
    if kind == "none":
        empty = (torch.zeros((0, 4)), torch.zeros((0,), dtype=torch.int64))
        return 2, R.SIZES_64x96, [empty, empty], retinanet.cell_anchors(), 0.4, 0.5
    if kind == "one":
        n, sizes, targets, kw, _, _ = edge_inputs("at_bg")
        return n, sizes, targets, retinanet.cell_anchors(aspect_ratios=(1.0,), scales_per_octave=1), 0.25, 0.9
    return _inputs(gold_dir, CASES[0])


@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("kind", ["none", "one", "fixture"])
def test_smooth_l1_value_and_gradient(device, gold_dir, kind, ordered):
    """against fp64 (tests/retinanet_ref.py): the value within 1e-5 relative, the gradient within rtol 1e-4 / atol 1e-7, with
    the module's normalisation 1 / max(1, 4 n_pos) upstream.  The predictions sit at target + e with e cycling through 0.5,
    -0.3, beta (1 - 1e-3), beta (1 + 1e-3), -beta (1 - 1e-3), -beta (1 + 1e-3), 0.05, -2, and (kind 'one') at exactly the target:
    d = 0.  bbox_reg is a column slice of a wider matrix (pitch 4 A + 4).  The ordered twin is bit-identical over two runs."""
    from scan_amd import ops
    from scan_amd.modeling import retinanet
    beta = 0.11
    n, sizes, targets, cells, bg, fg = _smooth_l1_case(gold_dir, kind)
    shape = ops.PyramidShape(n, sizes)
    A = int(cells.shape[1])
    tg = [(b.numpy(), l.numpy()) for b, l in targets]
    labels, matched, _ = R.match(n, sizes, tg, cells.numpy(), bg=bg, fg=fg)
    t64 = R.targets64(n, sizes, tg, cells.numpy(), labels, matched)
    n_pos = int((labels > 0).sum())
    assert n_pos == {"none": 0, "one": 1, "fixture": 59}[kind]
    e = np.array([0.5, -0.3, beta * (1 - 1e-3), beta * (1 + 1e-3), -beta * (1 - 1e-3), -beta * (1 + 1e-3), 0.05, -2.0])
    pred = (t64.astype(np.float32) + e[np.arange(t64.size) % 8].reshape(t64.shape).astype(np.float32))
    if kind == "one":
        assert not t64[labels > 0].any()
        pred[labels > 0] = [[0.0, beta * (1 - 1e-3), beta * (1 + 1e-3), -0.5]]
    pred = torch.from_numpy(pred.reshape(shape.rows, 4 * A))
    p64 = pred.double().requires_grad_(True)
    scale = 1.0 / max(1, 4 * n_pos)
    ref = R.smooth_l1_sum(p64.view(-1, 4), torch.from_numpy(t64), torch.from_numpy(labels > 0), beta)
    (ref * scale).backward()
    plan = retinanet.build_plan(shape, targets, device, cells=cells, bg=bg, fg=fg)
    assert plan.n_pos == n_pos
    wide = torch.zeros((shape.rows, 4 * A + 4), device=device)
    wide[:, :4 * A] = pred.to(device)
    wide.requires_grad_(True)
    old = ops.set_deterministic(ordered)
    try:
        runs = []
        for _ in range(2 if ordered else 1):
            wide.grad = None
            out = ops.retina_smooth_l1_loss(wide[:, :4 * A], shape, R.STRIDES, cells.to(device), plan.boxes, plan.labels_i32,
                                            plan.matched, beta)
            (out * scale).backward()
            runs.append((out.detach().clone(), wide.grad.clone()))
    finally:
        ops.set_deterministic(old)
    val, grad = float(runs[0][0]), runs[0][1].cpu().double()
    err = (grad[:, :4 * A] - p64.grad).abs()
    print("%s ordered=%s: value %.9g ref %.9g, worst gradient error %.3g" % (kind, ordered, val, float(ref.detach()), float(err.max())))
    assert abs(val - float(ref.detach())) <= 1e-5 * abs(float(ref.detach()))
    assert bool((err <= 1e-7 + 1e-4 * p64.grad.abs()).all())
    assert float(grad[:, 4 * A:].abs().max()) == 0.0
    neg = torch.from_numpy(np.repeat(labels <= 0, 4).reshape(shape.rows, 4 * A))
    assert float(grad[:, :4 * A][neg].abs().max() if neg.any() else 0.0) == 0.0  # written, and zero, for every other anchor
    if kind == "one":
        g = grad[:, :4 * A].reshape(-1, 4)[torch.from_numpy(labels > 0)][0]
        assert float(g[0]) == 0.0 and float(g[2]) == scale and float(g[3]) == -scale  # d = 0; above beta: sign(d)
    if ordered:
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_focal_kernels_ignore_label_minus_one(device):
    """the RetinaNet plan marks the anchors between the thresholds with -1: they must add nothing to the focal sum and get
    a gradient of exactly zero (csrc/losses.hip: focal_fwd_elem / focal_bwd_elem return 0 for a negative label)"""
    from scan_amd import ops
    g = torch.Generator().manual_seed(4)
    for C in (1, 3, 8):  # the vectorised C = 1 and C = 8 instances and the generic one
        logits = torch.randn((64, C), generator=g)
        labels = torch.randint(0, C + 1, (64,), generator=g).int()
        labels[::3] = -1
        x = logits.to(device).requires_grad_(True)
        out = ops.sigmoid_focal_loss_sum(x, labels.to(device), 2.0, 0.25)
        out.backward()
        keep = labels >= 0
        ref = R.focal_sum(logits.double()[keep], labels[keep].long(), 2.0, 0.25)
        assert abs(float(out.detach()) - float(ref)) <= 1e-5 * float(ref)
        assert float(x.grad[~keep.to(device)].abs().max()) == 0.0 and float(x.grad[keep.to(device)].abs().min()) > 0.0


# ----------------------------------------------------------------------------- 3. the module loss on the fixtures
@pytest.mark.parametrize("name", CASES)
def test_loss_computation_matches_the_reference(device, gold_dir, name):
    """both losses within 1e-4 relative, gradients w.r.t. the head outputs within rtol 1e-4 / atol 1e-7 of the reference's.  The
    head outputs are column slices of padded matrices, as the convs leave them: A * C = 9 (64x96) is no multiple of 4."""
    from scan_amd import ops
    from scan_amd.modeling import fcos, retinanet
    f = load_case(gold_dir, name)
    shape = ops.PyramidShape(f["N"], f["sizes"])
    A, C = int(f["num_anchors"]), int(f["num_classes"]) - 1
    if name == CASES[0]:
        assert (A * C) % 4 != 0
    le = retinanet.RetinaNetLossComputation(float(f["gamma"]), float(f["alpha"]), float(f["beta"]), float(f["bbox_reg_weight"]),
                                            cells=torch.from_numpy(f["cells"]), bg=float(f["bg"]), fg=float(f["fg"]))
    fcos.reset_target_plan()
    bufs = {}
    for k, cols in (("logits", A * C), ("reg", 4 * A)):
        b = torch.zeros((shape.rows, ops.pad4(cols)), device=device)
        b[:, :cols] = torch.from_numpy(f[k]).to(device)
        bufs[k] = (b.requires_grad_(True), cols)
    got = le(shape, bufs["logits"][0][:, :A * C], bufs["reg"][0][:, :4 * A], f["targets"])
    sum(got).backward()
    print(name, [float(v.detach()) for v in got], f["losses"])
    np.testing.assert_allclose([float(v.detach()) for v in got], f["losses"], rtol=1e-4)
    for k, (b, cols) in bufs.items():
        np.testing.assert_allclose(b.grad[:, :cols].cpu().numpy(), f["d_" + k], rtol=1e-4, atol=1e-7, err_msg=k)
        assert float(b.grad[:, cols:].abs().max() if b.shape[1] > cols else 0.0) == 0.0
    ignored = torch.from_numpy(f["labels"] == -1)
    assert int(ignored.sum()) > 0
    assert float(bufs["logits"][0].grad[:, :A * C].reshape(-1, C).cpu()[ignored].abs().max()) == 0.0
    assert float(bufs["reg"][0].grad[:, :4 * A].reshape(-1, 4).cpu()[ignored].abs().max()) == 0.0


# ----------------------------------------------------------------------------- 4. the post-processor
class _FixedHead(nn.Module):
    """stands in for the head: returns the fixture's head outputs whatever the features are"""

    def __init__(self, outs):
        super().__init__()
        self.outs = outs

    def forward(self, rows, shape):
        return self.outs


@pytest.mark.parametrize("name", CASES)
def test_postprocessor_candidates_and_detections(device, gold_dir, name):
    from scan_amd import config, ops
    from scan_amd.modeling import factory, retinanet
    from scan_amd.structures import BoxList
    f = load_case(gold_dir, name)
    N, C = f["N"], int(f["num_classes"]) - 1
    H, W = (int(v) for v in f["image_hw"])
    shape = ops.PyramidShape(N, f["sizes"])
    outs = tuple(torch.from_numpy(f[k]).to(device) for k in ("inf_logits", "inf_reg"))
    proc = retinanet.RetinaNetPostProcessor(float(f["inference_th"]), int(f["pre_nms_top_n"]), float(f["nms_th"]),
                                            int(f["detections_per_img"]), num_classes=C + 1, cells=torch.from_numpy(f["cells"]))
    ok, idx, lab, det, val = (t.cpu() for t in proc.select(shape, *outs, [(H, W)] * N))
    i_, c_, b_, s_ = idx[ok].numpy(), lab[ok].numpy(), det[ok].numpy(), val[ok].numpy()
    order, want = np.lexsort((c_, i_)), np.lexsort((f["cand_cls"], f["cand_idx"]))
    assert np.array_equal(i_[order], f["cand_idx"][want]) and np.array_equal(c_[order], f["cand_cls"][want])
    rb = f["cand_box"][want]
    assert (np.abs(b_[order] - rb) <= 1e-4 * np.maximum(1, np.abs(rb))).all()
    np.testing.assert_allclose(s_[order], f["cand_score"][want], rtol=1e-5)
    # final detections out of the factory module: per image equal in count and label (NMS and the kthvalue cap included)
    cfg = config.load("c2f", ["MODEL.FCOS_ON", False, "MODEL.RETINANET_ON", True, "MODEL.RETINANET.NUM_CLASSES", C + 1,
                              "MODEL.RETINANET.PRE_NMS_TOP_N", int(f["pre_nms_top_n"]), "TEST.DETECTIONS_PER_IMG",
                              int(f["detections_per_img"])])
    m = factory.build_rpn(cfg, 256).to(device)
    assert np.array_equal(m.cells.numpy(), f["cells"])
    m.head = _FixedHead(outs)
    m.eval()
    feats = ops.PyramidLevels(torch.zeros((shape.rows, 256), device=device), shape)
    with torch.no_grad():
        dets, losses, maps = m(torch.zeros((N, 3, H, W), device=device), feats, act_maps=feats)
    assert losses == {} and maps is None and len(dets) == N
    o = 0
    for d, k in zip(dets, f["det_count"]):
        assert isinstance(d, BoxList) and d.mode == "xyxy" and d.size == (W, H) and set(d.fields()) == {"scores", "labels"}
        assert len(d.bbox) == int(k)
        l, s, b = d.get_field("labels").cpu().numpy(), d.get_field("scores").cpu().numpy(), d.bbox.cpu().numpy()
        rl, rs, rbx = f["det_label"][o:o + k], f["det_score"][o:o + k], f["det_box"][o:o + k]
        assert np.array_equal(np.sort(l), np.sort(rl))
        a, r = np.lexsort((-s, l)), np.lexsort((-rs, rl))  # same detections: by label, then score
        assert np.array_equal(l[a], rl[r])
        np.testing.assert_allclose(s[a], rs[r], rtol=1e-5)
        assert (np.abs(b[a] - rbx[r]) <= 1e-4 * np.maximum(1, np.abs(rbx[r]))).all()
        o += int(k)


# ----------------------------------------------------------------------------- 5. the head
def test_head_matches_torch_cpu_restatement(device):
    """RetinaNetHead (two tower convs, A = 3, two classes: A * C = 6 is no multiple of 4) against F.conv2d + ReLU in fp64 on the
    CPU at the conv bars of test_conv2d_fwd_bwd for the active conv mode"""
    from scan_amd import ops
    from scan_amd.modeling import retinanet
    torch.manual_seed(31)
    head = retinanet.RetinaNetHead(3, num_anchors=3, num_convs=2, prior_prob=0.01)
    assert [k for k, _ in head.cls_tower.named_parameters()] == ["0.weight", "0.bias", "2.weight", "2.bias"]
    for p in head.parameters():  # the initialisation (std 0.01, zero biases) would leave most of the arithmetic untested
        if p.dim() == 4:
            nn.init.normal_(p, std=(2.0 / (p.shape[1] * 9)) ** 0.5)
        else:
            nn.init.normal_(p, std=0.2)
    n, sizes = 2, [(6, 7), (3, 4), (2, 2), (1, 2), (1, 1)]
    shape = ops.PyramidShape(n, sizes)
    x = torch.randn(shape.rows, 256)
    P = {k: v.detach().clone().double().requires_grad_(True) for k, v in head.state_dict().items()}
    x64 = x.double().requires_grad_(True)

    def conv_rows(rows, w, b, relu):
        outs = []
        for l, (h, wd) in enumerate(sizes):
            xl = rows[shape.row_off[l]:shape.row_off[l + 1]].view(n, h, wd, 256).permute(0, 3, 1, 2)
            y = F.conv2d(xl, w, b, padding=1)
            outs.append((F.relu(y) if relu else y).permute(0, 2, 3, 1).reshape(n * h * wd, -1))
        return torch.cat(outs, 0)

    def branch(tower, last):
        r = x64
        for i in (0, 2):
            r = conv_rows(r, P["%s.%d.weight" % (tower, i)], P["%s.%d.bias" % (tower, i)], True)
        return conv_rows(r, P[last + ".weight"], P[last + ".bias"], False)

    ref_logits, ref_reg = branch("cls_tower", "cls_logits"), branch("bbox_tower", "bbox_pred")
    g = torch.Generator().manual_seed(5)
    gys = [torch.randn(t.shape, generator=g, dtype=torch.float64) for t in (ref_logits, ref_reg)]
    ((ref_logits * gys[0]).sum() + (ref_reg * gys[1]).sum()).backward()

    head.to(device)
    for p in head.parameters():
        if p.dim() == 4:
            p.data = p.data.contiguous(memory_format=torch.channels_last)
    xd = x.to(device).requires_grad_(True)
    logits, reg = head(xd, shape)
    assert logits.shape == (shape.rows, 6) and reg.shape == (shape.rows, 12) and logits.stride(0) == 8
    tol = deform_ref.bar(ops.CONV_MODE)
    deform_ref.assert_within(logits, ref_logits, tol, "logits")
    deform_ref.assert_within(reg, ref_reg, tol, "bbox_reg")
    ((logits * gys[0].float().to(device)).sum() + (reg * gys[1].float().to(device)).sum()).backward()
    deform_ref.assert_within(xd.grad, x64.grad, tol, "dx")
    for k, p in head.named_parameters():
        deform_ref.assert_within(p.grad, P[k].grad, tol, k)


# ----------------------------------------------------------------------------- 6. the factory module
def test_factory_module_forward_backward_reaches_every_parameter(device):
    from scan_amd import config, ops
    from scan_amd.modeling import factory, fcos, retinanet
    from scan_amd.structures import BoxList
    torch.manual_seed(7)
    cfg = config.load("c2f", ["MODEL.FCOS_ON", False, "MODEL.RETINANET_ON", True, "MODEL.RETINANET.NUM_CLASSES", 3,
                              "MODEL.RETINANET.NUM_CONVS", 1])
    m = factory.build_rpn(cfg, 256).to(device)
    m.train()
    H, W, N = 64, 96, 2
    shape = ops.PyramidShape(N, R.SIZES_64x96)
    feats = ops.PyramidLevels(torch.randn((shape.rows, 256), device=device), shape)
    targets = []
    for b, l in (([[20.3, 10.2, 70.6, 50.7], [4.1, 8.4, 36.3, 40.8]], [1, 2]), ([[30.4, 20.3, 59.7, 44.2]], [2])):
        t = BoxList(torch.tensor(b), (W, H), mode="xyxy")
        t.add_field("labels", torch.tensor(l))
        targets.append(t)
    fcos.reset_target_plan()
    retinanet.plan_stats.update(launches=0, host_reads=0)
    dets, losses, maps = m(torch.zeros((N, 3, H, W), device=device), feats, targets=targets)
    assert dets is None and maps is None and set(losses) == {"loss_retina_cls", "loss_retina_reg"}
    assert retinanet.plan_stats["host_reads"] <= 1 and retinanet.plan_stats["launches"] == 2
    sum(losses.values()).backward()
    assert all(bool(torch.isfinite(v.detach())) and float(v.detach()) > 0 for v in losses.values()), losses
    for k, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k
    # with return_maps the same losses and the two score maps
    fcos.reset_target_plan()
    _, again, maps = m(torch.zeros((N, 3, H, W), device=device), feats, targets=targets, return_maps=True)
    assert set(maps) == {"box_cls", "box_regression"} and maps["box_cls"][0].shape == (N, 18, 8, 12)
    np.testing.assert_allclose([float(again[k]) for k in sorted(again)], [float(losses[k]) for k in sorted(losses)], rtol=1e-5)

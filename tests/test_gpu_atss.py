"""ATSS head on the GPU: the plan kernels against the torch spelling, the GIoU loss against the fp64 restatement, the module
loss and the post-processor against the reference's fixtures (tests/golden/atss_*.npz), the head against a torch-CPU
restatement, one Trainer iteration."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import atss_ref as R
import deform_ref
from atss_ref import CASES, SIZES_128x256, giou_inputs, load_case, tie_inputs

pytestmark = pytest.mark.gpu
CPU = torch.device("cpu")


# ----------------------------------------------------------------------------- 1. the plan kernels
def _plan_inputs(gold_dir, which):
    if which in CASES:
        f = load_case(gold_dir, which)
        return f["N"], f["sizes"], f["targets"]
    if which == "ties":
        sizes, targets = tie_inputs()
        return 2, sizes, targets
    if which == "ng0":  # one image without boxes
        return 2, SIZES_128x256, [(torch.zeros((0, 4)), torch.zeros((0,), dtype=torch.int64)),
                                  (torch.tensor([[40.3, 30.2, 150.6, 100.7], [52.1, 24.4, 160.3, 110.8]]), torch.tensor([1, 2]))]
    if which == "g1":
        return 1, [(8, 12), (4, 6), (2, 3), (1, 2), (1, 1)], [(torch.tensor([[20.3, 10.2, 70.6, 50.7]]), torch.tensor([1]))]
    assert which == "random50"
    g = torch.Generator().manual_seed(50)
    xy = torch.rand(50, 2, generator=g) * torch.tensor([230., 110.])
    wh = 4 + torch.rand(50, 2, generator=g) * torch.tensor([120., 90.])
    b = torch.cat([xy, torch.min(xy + wh, torch.tensor([255.5, 127.5]))], 1)
    return 1, SIZES_128x256, [(b, torch.randint(1, 3, (50,), generator=g))]


@pytest.fixture(scope="module")
def spelled_plans(gold_dir):
    """the torch spelling's plan of every input, on the CPU, computed once"""
    from scan_amd import ops
    from scan_amd.modeling import atss
    out = {}
    for which in CASES + ("ties", "ng0", "g1", "random50"):
        n, sizes, targets = _plan_inputs(gold_dir, which)
        out[which] = (n, sizes, targets, atss.build_plan(ops.PyramidShape(n, sizes), targets, CPU))
    return out


@pytest.mark.parametrize("which", CASES + ("ties", "ng0", "g1", "random50"))
@pytest.mark.parametrize("host_targets", [True, False])
def test_plan_kernels_equal_the_torch_spelling(device, spelled_plans, which, host_targets):
    from scan_amd import ops
    from scan_amd.modeling import atss
    n, sizes, targets, ref = spelled_plans[which]
    shape = ops.PyramidShape(n, sizes)
    tg = targets if host_targets else [(b.to(device), l.to(device)) for b, l in targets]
    got = atss.build_plan(shape, tg, device)
    assert atss.plan_stats == {"launches": 4 + (1 if ref.n_pos else 0), "host_reads": 1}
    assert got.labels.is_cuda and torch.equal(got.labels.cpu(), ref.labels)
    assert torch.equal(got.labels_i32.cpu(), ref.labels.int())
    assert torch.equal(got.matched.cpu(), ref.matched)
    assert got.n_pos == ref.n_pos and torch.equal(got.pos_inds.cpu(), ref.pos_inds)
    counts = [int((ref.labels[shape.row_off[l]:shape.row_off[l + 1]] > 0).sum()) for l in range(shape.n_levels)]
    assert [int((got.labels[shape.row_off[l]:shape.row_off[l + 1]] > 0).sum()) for l in range(shape.n_levels)] == counts
    # targets against fp64 (log / exp are within a few ulp; 5 * log(ratio) near ratio 1 has an absolute error of ~5 ulp of 1)
    _, matched64, _ = R.assign(n, sizes, targets)
    assert torch.equal(matched64, ref.matched.long())
    anchors = R.row_anchors(n, sizes)[ref.pos_inds]
    off = R.row_offsets(n, sizes)
    img = torch.tensor([next((int(r) - off[l]) // (h * w) for l, (h, w) in enumerate(sizes) if off[l] <= int(r) < off[l + 1])
                        for r in ref.pos_inds], dtype=torch.int64)
    G = max(1, max(int(b.shape[0]) for b, _ in targets))
    boxes = torch.zeros((n, G, 4), dtype=torch.float64)
    for i, (b, _) in enumerate(targets):
        boxes[i, :b.shape[0]] = b.double()
    reg64 = R.encode(boxes[img, matched64[ref.pos_inds]], anchors)
    np.testing.assert_allclose(got.reg_pos.cpu().numpy(), reg64.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(got.ctr_pos.cpu().numpy(), R.centerness(reg64, anchors).numpy(), rtol=1e-5, atol=1e-6)
    # two runs are bit-identical, with the deterministic knob off and on (integer max: order-independent)
    old = ops.set_deterministic(True)
    try:
        again = atss.build_plan(shape, tg, device)
    finally:
        ops.set_deterministic(old)
    for name in ("labels", "matched", "pos_inds", "reg_pos", "ctr_pos"):
        assert torch.equal(getattr(got, name), getattr(again, name)), name


def test_plan_is_cached_per_batch_and_built_on_a_side_stream(device, gold_dir):
    from scan_amd import ops
    from scan_amd.modeling import atss, fcos
    f = load_case(gold_dir, CASES[1])
    shape = ops.PyramidShape(f["N"], f["sizes"])
    fcos.reset_target_plan()
    side = ops.borrow_side_streams(3)[0]
    p = atss.target_plan(shape, f["targets"], device, side_stream=side)
    assert p.ready is not None and atss.target_plan(shape, f["targets"], device) is p
    torch.cuda.synchronize()
    assert np.array_equal(p.labels.cpu().numpy(), f["labels"])
    fcos.reset_target_plan()  # the Trainer's per-iteration reset covers this cache too
    assert atss.target_plan(shape, f["targets"], device) is not p


# ----------------------------------------------------------------------------- 2. GIoU loss
WIDER_GRADIENT_BAR = {(4097, "generic")}  # see the docstring below


@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("kind", ["generic", "clamp", "disjoint", "flipped"])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 4097])
def test_giou_loss_value_and_gradient(device, P, kind, ordered):
    """against tests/atss_ref.py in fp64 at the bars tests/test_gpu_losses.py holds the IoU loss to: value within 1e-5 |ref|,
    gradient rtol 1e-4 / atol 1e-7.  The ordered twin (deterministic mode) is held to the same bars and is bit-identical over
    two runs.

    One case has a wider gradient bar, derived and not picked: P = 4097 / generic.  Its row 1085 decodes to a prediction and a
    target whose y2 differ by 1.6e-5, one fp32 ulp at 297 px, so any fp32 evaluation may route the gradient of the
    intersection's min and the enclosure's max to the other argument.  The reference's own formula in fp32 torch on the CPU is
    off by 8.34e-5 there (834 x the bar; every other element of every case stays inside it), the kernel by 7.1e-5 (709 x).  For
    that case the absolute part of the bar is 4 x the fp32-torch worst error, computed here on the same inputs (3.3e-4); the
    figures are in profiles/r16_atss.txt."""
    from scan_amd import ops
    pred, target, rows, weight = giou_inputs(P, kind)
    shape = ops.PyramidShape(2, SIZES_128x256)
    anchors = R.row_anchors(2, SIZES_128x256)[rows]
    p64 = pred.double().requires_grad_(True)
    num, den = R.giou_loss(p64, target.double(), anchors, weight.double())
    ref = num / den
    (3.0 * ref).backward()
    if kind == "disjoint":
        assert bool((R.giou_losses(p64.detach(), target.double(), anchors) > 1.0).all())  # GIoU < 0: no intersection
    if kind == "flipped":
        d = R.decode(p64.detach(), anchors)
        assert bool(((d[:, 2] < d[:, 0]) | (d[:, 3] < d[:, 1])).any())
    # what the reference's own formula gives in fp32 torch on the CPU, for the record
    p32 = pred.clone().requires_grad_(True)
    n32, d32 = R.giou_loss(p32, target, anchors.float(), weight)
    (3.0 * n32 / d32).backward()
    pd = pred.to(device).requires_grad_(True)
    old = ops.set_deterministic(ordered)
    try:
        runs = []
        for _ in range(2 if ordered else 1):
            pd.grad = None
            out = ops.atss_giou_loss(pd, target.to(device), rows.to(device), weight.to(device), shape, R.STRIDES, R.SIZES)
            (3.0 * out).backward()
            runs.append((out.detach().clone(), pd.grad.clone()))
    finally:
        ops.set_deterministic(old)
    val, grad = float(runs[0][0]), runs[0][1].cpu().double()
    err = (grad - p64.grad).abs()
    err32 = (p32.grad.double() - p64.grad).abs()
    atol = 4 * float(err32.max()) if (P, kind) in WIDER_GRADIENT_BAR else 1e-7
    bar = 1e-7 + 1e-4 * p64.grad.abs()
    print("P=%d %s: worst absolute gradient error %.3g (fp32 torch %.3g), atol %.3g" % (P, kind, float(err.max()),
                                                                                        float(err32.max()), atol))
    print("P=%d %s ordered=%s: value rel err %.3g (fp32 torch %.3g); gradient worst err / bar %.3g (fp32 torch %.3g)"
          % (P, kind, ordered, abs(val - float(ref)) / abs(float(ref)), abs(float(n32 / d32) - float(ref)) / abs(float(ref)),
             float((err / bar).max()), float((err32 / bar).max())))
    assert abs(val - float(ref)) <= 1e-5 * abs(float(ref))
    assert bool((err <= atol + 1e-4 * p64.grad.abs()).all())
    if ordered:
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


# ----------------------------------------------------------------------------- 3. the module loss on the fixtures
@pytest.mark.parametrize("mode", ["fp32", "bf16x6"])
@pytest.mark.parametrize("name", CASES)
def test_loss_computation_matches_the_reference(device, gold_dir, name, mode, monkeypatch):
    """the three losses within 1e-4 relative (the project's loss bar), gradients w.r.t. the head outputs within rtol 1e-4 /
    atol 1e-7 of the reference's; the loss path has no conv, so both conv modes must pass alike"""
    from scan_amd import ops
    from scan_amd.modeling import atss, fcos
    monkeypatch.setattr(ops, "CONV_MODE", mode)
    f = load_case(gold_dir, name)
    shape = ops.PyramidShape(f["N"], f["sizes"])
    le = atss.ATSSLossComputation(float(f["gamma"]), float(f["alpha"]), float(f["reg_loss_weight"]),
                                  sizes=[float(a) for a in f["anchor_sizes"]], topk=int(f["topk"]))
    fcos.reset_target_plan()
    outs = {k: torch.from_numpy(f[k]).to(device).requires_grad_(True) for k in ("logits", "reg", "ctr")}
    got = le(shape, outs["logits"], outs["reg"], outs["ctr"], f["targets"])
    sum(got).backward()
    print(name, mode, [float(v) for v in got], f["losses"])
    np.testing.assert_allclose([float(v) for v in got], f["losses"], rtol=1e-4)
    for k in ("logits", "reg", "ctr"):
        np.testing.assert_allclose(outs[k].grad.cpu().numpy(), f["d_" + k], rtol=1e-4, atol=1e-7, err_msg=k)


def test_loss_without_positives_takes_the_sum_fallbacks(device):
    from scan_amd import ops
    from scan_amd.modeling import atss, fcos
    shape = ops.PyramidShape(1, [(8, 12), (4, 6), (2, 3), (1, 2), (1, 1)])
    tg = [(torch.tensor([[17.3, 9.2, 19.1, 11.4]]), torch.tensor([1]))]  # no anchor centre inside: no positives
    fcos.reset_target_plan()
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(shape.rows, 2, generator=g) - 2).to(device).requires_grad_(True)
    reg = torch.randn(shape.rows, 4, generator=g).to(device).requires_grad_(True)
    ctr = torch.randn(shape.rows, generator=g).to(device).requires_grad_(True)
    lc, lr, lctr = atss.ATSSLossComputation(2.0, 0.25)(shape, logits, reg, ctr, tg)
    ref = R.focal_sum(logits.detach().cpu().double(), torch.zeros(shape.rows, dtype=torch.int64), 2.0, 0.25)
    assert abs(float(lc) - float(ref)) <= 1e-4 * float(ref) and float(lr) == 0.0 and float(lctr) == 0.0
    (lc + lr + lctr).backward()
    assert float(reg.grad.abs().max()) == 0.0 and float(ctr.grad.abs().max()) == 0.0


# ----------------------------------------------------------------------------- 4. the head
@pytest.mark.parametrize("dcn", [False, True])
def test_head_matches_torch_cpu_restatement(device, dcn):
    """ATSSHead (two tower convs; the last one deformable with ``dcn``) against F.conv2d / group_norm in fp64 on the CPU at the
    conv bars of test_conv2d_fwd_bwd; its outputs then feed an in-place ReLU"""
    from scan_amd import ops
    from scan_amd.modeling import atss
    torch.manual_seed(21 + dcn)
    head = atss.ATSSHead(3, num_convs=2, prior_prob=0.01, use_dcn_in_tower=dcn)
    for p in head.parameters():  # the initialisation (std 0.01, zero biases) would leave most of the arithmetic untested
        if p.dim() == 4:
            nn.init.normal_(p, std=(2.0 / (p.shape[1] * 9)) ** 0.5)
        elif p.dim() == 1 and p.numel() > 1:
            nn.init.normal_(p, std=0.2)
    for l, s in enumerate(head.scales):
        nn.init.constant_(s.scale, 0.5 + 0.25 * l)
    if dcn:
        for tower in (head.cls_tower, head.bbox_tower):
            nn.init.normal_(tower[3].offset.weight, std=0.01)
    n, sizes = 2, [(6, 7), (3, 4), (2, 2), (1, 2), (1, 1)]
    shape = ops.PyramidShape(n, sizes)
    x = torch.randn(shape.rows, 256)
    P = {k: v.detach().clone().double().requires_grad_(True) for k, v in head.state_dict().items()}
    x64 = x.double().requires_grad_(True)

    def tower(name, rows):
        for i in range(2):
            pre = "%s.%d." % (name, 3 * i)
            outs = []
            for l, (h, w) in enumerate(sizes):
                xl = rows[shape.row_off[l]:shape.row_off[l + 1]]
                nchw = xl.view(n, h, w, 256).permute(0, 3, 1, 2)
                if dcn and i == 1:
                    om = F.conv2d(nchw, P[pre + "offset.weight"], P[pre + "offset.bias"], padding=1)
                    om = om.permute(0, 2, 3, 1).reshape(n * h * w, -1)
                    y = deform_ref.deform_conv(xl, om[:, :18], om[:, 18:27].sigmoid(), P[pre + "conv.weight"],
                                               P[pre + "conv.bias"], n, ((h, w),)).view(n, h, w, 256).permute(0, 3, 1, 2)
                else:
                    y = F.conv2d(nchw, P[pre + "weight"], P[pre + "bias"], padding=1)
                gn = "%s.%d." % (name, 3 * i + 1)
                y = F.relu(F.group_norm(y, 32, P[gn + "weight"], P[gn + "bias"], 1e-5))
                outs.append(y.permute(0, 2, 3, 1).reshape(n * h * w, 256))
            rows = torch.cat(outs, 0)
        return rows

    def conv_rows(rows, w, b):
        outs = []
        for l, (h, wd) in enumerate(sizes):
            xl = rows[shape.row_off[l]:shape.row_off[l + 1]].view(n, h, wd, 256).permute(0, 3, 1, 2)
            outs.append(F.conv2d(xl, w, b, padding=1).permute(0, 2, 3, 1).reshape(n * h * wd, -1))
        return torch.cat(outs, 0)

    ct, bt = tower("cls_tower", x64), tower("bbox_tower", x64)
    ref_logits = conv_rows(ct, P["cls_logits.weight"], P["cls_logits.bias"])
    scale = torch.cat([P["scales.%d.scale" % l].expand(shape.row_off[l + 1] - shape.row_off[l]) for l in range(5)])
    ref_reg = conv_rows(bt, P["bbox_pred.weight"], P["bbox_pred.bias"]) * scale[:, None]  # no exp
    ref_ctr = conv_rows(bt, P["centerness.weight"], P["centerness.bias"])[:, 0]
    g = torch.Generator().manual_seed(5)
    gys = [torch.randn(t.shape, generator=g, dtype=torch.float64) for t in (ref_logits, ref_reg, ref_ctr)]
    gys[1] = gys[1] * (ref_reg.detach().abs() > 1e-3)  # the in-place ReLU behind bbox_reg: keep clear of its kink
    (ref_logits * gys[0]).sum().add((F.relu(ref_reg) * gys[1]).sum()).add((ref_ctr * gys[2]).sum()).backward()

    head.to(device)
    for p in head.parameters():
        if p.dim() == 4:
            p.data = p.data.contiguous(memory_format=torch.channels_last)
    xd = x.to(device).requires_grad_(True)
    logits, reg, ctr = head(xd, shape)
    assert logits.shape == (shape.rows, 2) and reg.shape == (shape.rows, 4) and ctr.shape == (shape.rows,)
    tol = deform_ref.bar(ops.CONV_MODE)
    deform_ref.assert_within(logits, ref_logits, tol, "logits")
    deform_ref.assert_within(reg, ref_reg, tol, "bbox_reg")
    deform_ref.assert_within(ctr, ref_ctr, tol, "centerness")
    reg = nn.ReLU(inplace=True)(reg)  # an in-place consumer may overwrite the head's output
    ((logits * gys[0].float().to(device)).sum() + (reg * gys[1].float().to(device)).sum()
     + (ctr * gys[2].float().to(device)).sum()).backward()
    deform_ref.assert_within(xd.grad, x64.grad, tol, "dx")
    for k, p in head.named_parameters():
        deform_ref.assert_within(p.grad, P[k].grad, tol, k)


# ----------------------------------------------------------------------------- 5. the post-processor
class _FixedHead(nn.Module):
    """stands in for the head: returns the fixture's head outputs whatever the features are"""

    def __init__(self, outs):
        super().__init__()
        self.outs = outs

    def forward(self, rows, shape, need_cls=True):
        return self.outs


@pytest.mark.parametrize("name", CASES)
def test_postprocessor_candidates_and_detections(device, gold_dir, name):
    from scan_amd import ops
    from scan_amd.modeling import atss, factory
    from scan_amd.structures import BoxList
    f = load_case(gold_dir, name)
    N, C = f["N"], int(f["num_classes"]) - 1
    H, W = (int(v) for v in f["image_hw"])
    shape = ops.PyramidShape(N, f["sizes"])
    outs = tuple(torch.from_numpy(f[k]).to(device) for k in ("inf_logits", "inf_reg", "inf_ctr"))
    proc = atss.ATSSPostProcessor(num_classes=C + 1, sizes=[float(a) for a in f["anchor_sizes"]])
    proc.deferred = True
    pend = proc._select(shape, *outs, [(H, W)] * N)
    proc.deferred = False
    torch.cuda.synchronize()
    ok = pend.ok.cpu()
    rows, cls = pend.rows.cpu()[ok], pend.lab.cpu()[ok]
    box, score = pend.det.cpu()[ok], torch.sqrt(pend.val.cpu()[ok])
    order = np.lexsort((cls.numpy(), rows.numpy()))
    want = np.lexsort((f["cand_cls"], f["cand_row"]))
    assert np.array_equal(rows.numpy()[order], f["cand_row"][want]) and np.array_equal(cls.numpy()[order], f["cand_cls"][want])
    rb = f["cand_box"][want]
    assert (np.abs(box.numpy()[order] - rb) <= 1e-4 * np.maximum(1, np.abs(rb))).all()
    np.testing.assert_allclose(score.numpy()[order], f["cand_score"][want], rtol=1e-5)
    per_image = [int(v) for v in ok.sum(1)]
    # final detections out of the factory module
    from scan_amd import config
    cfg = config.load("c2f", ["MODEL.ATSS_ON", True, "MODEL.ATSS.NUM_CLASSES", C + 1, "TEST.DETECTIONS_PER_IMG", 20])
    m = factory.build_rpn(cfg, 256).to(device)
    m.head = _FixedHead(outs)
    m.eval()
    feats = ops.PyramidLevels(torch.zeros((shape.rows, 256), device=device), shape)
    with torch.no_grad():
        dets, losses, maps = m(torch.zeros((N, 3, H, W), device=device), feats, act_maps=feats)
    assert losses == {} and maps is None and len(dets) == N
    for d, k in zip(dets, per_image):
        assert isinstance(d, BoxList) and d.mode == "xyxy" and d.size == (W, H) and set(d.fields()) == {"scores", "labels"}
        b, s, l = d.bbox.cpu(), d.get_field("scores").cpu(), d.get_field("labels").cpu()
        assert 0 < len(b) <= 20 and len(b) < k  # NMS and the per-image cap did suppress
        assert bool((b[:, 0] >= 0).all() and (b[:, 1] >= 0).all() and (b[:, 2] <= W - 1).all() and (b[:, 3] <= H - 1).all())
        assert bool(((s > 0) & (s <= 1)).all()) and bool(((l >= 1) & (l <= C)).all())
    # before the cap: NMS alone suppresses
    proc2 = atss.ATSSPostProcessor(num_classes=C + 1, fpn_post_nms_top_n=0, sizes=[float(a) for a in f["anchor_sizes"]])
    for (b, s, l), k in zip(proc2(shape, *outs, [(H, W)] * N), per_image):
        assert 0 < len(s) < k


# ----------------------------------------------------------------------------- 6. the Trainer
def test_trainer_iteration_on_the_atss_head(device):
    """One iteration of engine.Trainer on build_model(3, rpn="atss") at 128x256.  A level's Scale parameter has a gradient only
    when the level has a positive, and with the default anchor sizes (64 ... 1024) no box of a 128x256 image is positive on P6 / P7
    (their IoU with a 512 / 1024 px anchor is below every box's threshold): the anchor sizes are set to (16, 32, 64, 96, 128)
    and the boxes chosen so that all five levels have positives, which is asserted, so that EVERY head parameter must move."""
    from scan_amd import engine, ops, synth
    from scan_amd.modeling import atss, fcos
    torch.manual_seed(9)
    sizes = (16., 32., 64., 96., 128.)
    base_keys = set(engine.build_model(3, device=CPU))
    model = engine.build_model(3, device=device, attn_dropout=0.0, rpn="atss", atss_settings={"anchor_sizes": sizes})
    assert set(model) == base_keys and isinstance(model["fcos"], atss.ATSSModule)
    H, W, N = 128, 256, 2
    targets = [(torch.tensor([[10.3, 12.2, 26.7, 30.1], [60.5, 40.5, 92.2, 75.3], [120.2, 20.1, 190.7, 88.3]]), torch.tensor([1, 2, 1])),
               (torch.tensor([[130.3, 2.2, 250.7, 124.1], [50.2, 10.3, 140.9, 110.6], [200.3, 90.2, 212.7, 101.1]]),
                torch.tensor([2, 1, 2]))]
    shape = ops.PyramidShape(N, SIZES_128x256)
    plan = atss.build_plan(shape, targets, CPU, sizes=sizes)
    assert all(int((plan.labels[shape.row_off[l]:shape.row_off[l + 1]] > 0).sum()) > 0 for l in range(5))
    imgs_s, imgs_t = synth.synth_images(N, H, W, 1234).to(device), synth.synth_images(N, H, W, 2234).to(device)
    trainer = engine.Trainer(model)
    before = {k: v.detach().clone() for k, v in model["fcos"].named_parameters()}
    seen = {}
    h1 = model["fcos"].register_forward_pre_hook(lambda m, args: seen.update(shape=args[2]))
    h2 = model["fcos"].head.register_forward_hook(lambda m, args, out: seen.update(out=[t.detach().clone() for t in out]))
    losses = trainer.step(imgs_s, targets, imgs_t)
    h1.remove()
    h2.remove()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v.detach()).all()) for v in losses.values()), losses
    got = [float(losses[k]) for k in ("loss_cls_gs", "loss_reg_gs", "loss_centerness_gs")]
    # the module-level computation on the head outputs of that iteration (sums end in float atomics: ~1e-7 between two runs)
    fcos.reset_target_plan()
    want = [float(v) for v in model["fcos"].loss_evaluator(seen["shape"], *seen["out"], targets)]
    print("trainer", got, "module", want)
    np.testing.assert_allclose(got, want, rtol=1e-5)
    assert all(w > 0 for w in want)
    for k, p in model["fcos"].named_parameters():
        assert bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), before[k]), k

"""Region-proposal network on the GPU: labels, sampler, loss and proposal decode of csrc/rpn.hip against the reference's fixtures
(tests/golden/rpn_*.npz) and the fp64 / integer restatement (tests/rpn_ref.py); the head against a torch-CPU restatement; the
factory module's proposals in train and test mode, and through the Pooler."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import deform_ref
import retinanet_ref as R
import rpn_ref as P
from rpn_ref import CASES, load_case

pytestmark = pytest.mark.gpu
BOX_TOL = 1e-4  # |box - ref| <= BOX_TOL * max(1, |ref|): test_gpu_retinanet.py's bar for decoded candidates
SAMPLE_BLOCK = 256  # RPN_SAMPLE_BLOCK of csrc/rpn.hip: one workgroup strides over an image's anchors; there is no grid cap


def _label_inputs(gold_dir, which):
    """(N, sizes, boxes per image, cells [L, A, 4] fp32 numpy, image (h, w) per image, bg, fg, straddle)"""
    f = load_case(gold_dir, CASES[0] if which in ("empty_image", "no_straddle", "far_box") else which)
    N, sizes, boxes, hw, thr = f["N"], f["sizes"], f["box_lists"], f["image_hw"], float(f["straddle_thresh"])
    if which == "empty_image":
        boxes = [np.zeros((0, 4), np.float32), boxes[0]]
    elif which == "no_straddle":
        thr = -1.0
    elif which == "far_box":  # the second box overlaps no anchor: its maximum is 0, which every anchor that misses it equals
        N, boxes, hw = 1, [np.array([[20.3, 10.2, 50.6, 40.7], [5000.5, 5000.5, 5010.5, 5010.5]], np.float32)], hw[:1]
    return N, sizes, boxes, f["cells"], hw, float(f["bg"]), float(f["fg"]), thr


LABEL_CASES = CASES + ("empty_image", "no_straddle", "far_box")


@pytest.fixture(scope="module")
def references(gold_dir):
    """per label input the restatement's labels / matched / visibility and the image of every anchor, computed once"""
    out = {}
    for which in LABEL_CASES:
        N, sizes, boxes, cells, hw, bg, fg, thr = _label_inputs(gold_dir, which)
        lab, matched, _, vis = P.labels(N, sizes, boxes, cells, hw, bg, fg, thr)
        out[which] = (lab, matched, vis, R.anchors_in_order(N, sizes, cells)[1])
    return out


def _loss_evaluator(gold_dir, which, **kw):
    from scan_amd import ops
    from scan_amd.modeling import rpn
    N, sizes, boxes, cells, hw, bg, fg, thr = _label_inputs(gold_dir, which)
    le = rpn.RPNLossComputation(cells=torch.from_numpy(cells), bg=bg, fg=fg, straddle_thresh=thr, **kw)
    targets = [(torch.from_numpy(np.ascontiguousarray(b)), torch.ones(len(b), dtype=torch.int64)) for b in boxes]
    return le, ops.PyramidShape(N, sizes), targets, hw


# ----------------------------------------------------------------------------- 1. labels
@pytest.mark.parametrize("which", LABEL_CASES)
def test_labels_equal_the_fixtures_and_the_restatement(device, gold_dir, references, which):
    lab, matched, vis, img = references[which]
    le, shape, targets, hw = _loss_evaluator(gold_dir, which)
    got_l, got_m, boxes = le.labels(shape, targets, hw, device)
    assert got_l.dtype == torch.int32 and got_l.numel() == lab.size and boxes.shape[0] == shape.n_images
    assert np.array_equal(got_l.cpu().numpy(), lab) and np.array_equal(got_m.cpu().numpy(), matched)
    if which in CASES:
        f = load_case(gold_dir, which)
        assert np.array_equal(got_l.cpu().numpy(), f["labels"]) and np.array_equal(got_m.cpu().numpy(), f["matched"])
        assert int((~vis).sum()) > 0 and (lab[~vis] == -1).all()
    if which == "empty_image":
        assert (lab[(img == 0) & vis] == 0).all() and (lab[(img == 0) & ~vis] == -1).all() and (lab[img == 1] == 1).any()
    if which == "no_straddle":
        assert vis.all() and (lab == 1).sum() > (references[CASES[0]][0] == 1).sum()  # the hidden positives are back
    if which == "far_box":
        assert (lab[vis] == 1).all() and (lab[~vis] == -1).all()  # the literal low-quality rule: every anchor ties at 0


# ----------------------------------------------------------------------------- 2. the sampler
def _synthetic_labels(N, sizes, A, kind):
    n = R.row_offsets(N, sizes)[-1] * A
    rs = np.random.RandomState(5)
    if kind == "all_ignored":
        return np.full(n, -1, np.int32)
    if kind == "few_negatives":  # 3 negatives per image at most: fewer than B - num_pos
        lab = np.where(rs.rand(n) < 0.02, 1, -1).astype(np.int32)
        lab[rs.choice(n, 5, replace=False)] = 0
        return lab
    return rs.choice([-1, 0, 1], size=n, p=[0.2, 0.6, 0.2]).astype(np.int32)


@pytest.mark.parametrize("case", ["fixture_small", "fixture_wide", "ties", "equal_keys", "all_ignored", "few_negatives", "big_batch"])
def test_sampler_equals_the_restatement(device, gold_dir, references, case):
    """sampled bytes and counters equal tests/rpn_ref.py exactly, and two calls give the same bytes.  fixture_wide / ties / ...
    run on the 128x256 pyramid: 2046 anchors per image, eight rounds of a SAMPLE_BLOCK-wide workgroup (the launch has no
    other cap: 2 N workgroups).  ties: keys in 0..3, so the key select ends inside a group of equal keys and the ordinal select
    decides; equal_keys: decided by index alone."""
    from scan_amd import ops
    f = load_case(gold_dir, CASES[0] if case in ("fixture_small", "big_batch") else CASES[1])
    N, sizes, A = f["N"], f["sizes"], int(f["num_anchors"])
    shape = ops.PyramidShape(N, sizes)
    img = R.anchors_in_order(N, sizes, f["cells"])[1]
    lab = references[CASES[0] if case in ("fixture_small", "big_batch") else CASES[1]][0].astype(np.int32)
    B, frac, keys, seeds = int(f["batch_size_per_image"]), float(f["positive_fraction"]), None, (0, 1, 0xfffffffe)
    if case in ("ties", "equal_keys", "all_ignored", "few_negatives"):
        lab = _synthetic_labels(N, sizes, A, case)
        B, seeds = 256, (3,)
    if case == "ties":
        keys = np.random.RandomState(6).randint(0, 4, lab.size).astype(np.int32)
    if case == "equal_keys":
        keys = np.full(lab.size, 0x7fffffff, np.int32)
    if case == "big_batch":
        B = 1000
        assert lab.size // N < B
    if case != "fixture_small":
        assert lab.size // N > SAMPLE_BLOCK or case == "big_batch"
    lab_d = torch.from_numpy(lab).to(device)
    keys_d = None if keys is None else torch.from_numpy(keys).to(device)
    for seed in seeds:
        want, want_counts = P.sample(lab, img, N, B, frac, seed, keys)
        got, counts = ops.rpn_sample(shape, A, lab_d, B, frac, seed, keys_d)
        again, _ = ops.rpn_sample(shape, A, lab_d, B, frac, seed, keys_d)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), (case, seed)
        assert np.array_equal(counts.cpu().numpy(), want_counts) and torch.equal(got, again)
    if case == "all_ignored":
        assert not want.any() and not want_counts.any()
    if case == "few_negatives":
        assert (want_counts[:, 1] < B - want_counts[:, 0]).all() and want_counts[:, 1].sum() == 5
    if case == "big_batch":
        assert np.array_equal(want != 0, lab >= 0)  # everything that is not ignored is taken... up to int(B frac) positives
    if case == "ties":
        assert (want_counts[:, 0] == 128).all()


# ----------------------------------------------------------------------------- 3. the loss
def _wide(f, shape, device, obj_key="obj", reg_key="reg"):
    """the head's layout: one padded matrix [M, pad4(5 A)], bbox_reg in columns [0, 4 A), objectness in [4 A, 5 A)"""
    from scan_amd import ops
    A = int(f["num_anchors"])
    wide = torch.zeros((shape.rows, ops.pad4(5 * A)), device=device)
    wide[:, :4 * A] = torch.from_numpy(f[reg_key]).to(device)
    wide[:, 4 * A:5 * A] = torch.from_numpy(f[obj_key]).to(device)
    return wide.requires_grad_(True), A


@pytest.mark.parametrize("name", CASES)
def test_loss_matches_the_reference_with_its_own_sample(device, gold_dir, references, name):
    """with the reference's sampled masks: both losses within rtol 1e-4 of the reference and 1e-5 of the fp64 restatement,
    gradients within rtol 1e-4 / atol 1e-7, encoded targets within rtol 1e-5 / atol 1e-6; the gradient is exactly zero at every
    unsampled anchor and in the padding column; the head outputs are read in place through the pitch of the padded matrix."""
    from scan_amd import ops
    from scan_amd.modeling import retinanet
    f = load_case(gold_dir, name)
    le, shape, targets, hw = _loss_evaluator(gold_dir, name)
    wide, A = _wide(f, shape, device)
    assert wide.shape[1] > 5 * A
    lo, lr = le(shape, wide[:, 4 * A:5 * A], wide[:, :4 * A], targets, hw, sampled=torch.from_numpy(f["sampled"]))
    (lo + lr).backward()
    got = [float(lo.detach()), float(lr.detach())]
    lab, matched = references[name][:2]
    t64 = P.targets64(f["N"], f["sizes"], f["box_lists"], f["cells"], matched)
    n = int((f["sampled"] != 0).sum())
    r0, r1 = P.loss_sums(torch.from_numpy(f["obj"]).double().reshape(-1), torch.from_numpy(f["reg"]).double().reshape(-1, 4),
                         f["sampled"], t64, 1.0 / 9)
    print(name, got, f["losses"], float(r0) / n, float(r1) / n)
    np.testing.assert_allclose(got, f["losses"], rtol=1e-4)
    np.testing.assert_allclose(got, [float(r0) / n, float(r1) / n], rtol=1e-5)
    g = wide.grad.cpu().numpy()
    np.testing.assert_allclose(g[:, 4 * A:5 * A], f["d_obj"], rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(g[:, :4 * A], f["d_reg"], rtol=1e-4, atol=1e-7)
    assert not g[:, 5 * A:].any()
    assert not g[:, 4 * A:5 * A].reshape(-1)[f["sampled"] == 0].any() and not g[:, :4 * A].reshape(-1, 4)[f["sampled"] != 1].any()
    assert g[:, 4 * A:5 * A].reshape(-1)[f["sampled"] != 0].all()
    # the encoded targets of the sampled positives, zero elsewhere
    labels, matched_d, boxes = le.labels(shape, targets, hw, device)
    t_out = torch.full((shape.rows * A, 4), 7.0, device=device)
    ops.rpn_loss(wide[:, 4 * A:5 * A].detach(), wide[:, :4 * A].detach(), shape, R.STRIDES, retinanet.device_cells(le.cells, device),
                 boxes, matched_d, torch.from_numpy(f["sampled"]).to(device), 1.0 / 9, targets_out=t_out)
    pos = f["sampled"] == 1
    np.testing.assert_allclose(t_out.cpu().numpy()[pos], t64[pos], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(t_out.cpu().numpy()[pos], f["reg_targets"][pos], rtol=1e-5, atol=1e-6)
    assert not t_out.cpu().numpy()[~pos].any()


def test_loss_ordered_twin_is_reproducible_and_close(device, gold_dir):
    from scan_amd import ops
    f = load_case(gold_dir, CASES[1])
    le, shape, targets, hw = _loss_evaluator(gold_dir, CASES[1])
    wide, A = _wide(f, shape, device)
    s = torch.from_numpy(f["sampled"])
    runs = {}
    for ordered in (False, True, True):
        old = ops.set_deterministic(ordered)
        try:
            wide.grad = None
            lo, lr = le(shape, wide[:, 4 * A:5 * A], wide[:, :4 * A], targets, hw, sampled=s)
            (lo + lr).backward()
            runs.setdefault(ordered, []).append((torch.stack((lo, lr)).detach().clone(), wide.grad.clone()))
        finally:
            ops.set_deterministic(old)
    (a, ga), (b, gb) = runs[True]
    assert torch.equal(a, b) and torch.equal(ga, gb)
    np.testing.assert_allclose(a.cpu().numpy(), runs[False][0][0].cpu().numpy(), rtol=1e-5)
    assert ops.query("scan_rpn_loss_ordered_ws_floats", shape.rows * A) == 2 * ((shape.rows * A + 2047) // 2048)


def test_loss_extreme_logits_and_empty_sample(device, gold_dir):
    """logits of +-80 on sampled anchors: finite values equal to fp64 within 1e-5, finite gradients; an empty sample: both
    losses exactly 0, gradients exactly 0, no NaN"""
    f = load_case(gold_dir, CASES[0])
    le, shape, targets, hw = _loss_evaluator(gold_dir, CASES[0])
    obj = f["obj"].copy().reshape(-1)
    taken = np.nonzero(f["sampled"])[0]
    obj[taken[0::2]], obj[taken[1::2]] = 80.0, -80.0
    g = dict(f, obj=obj.reshape(f["obj"].shape))
    wide, A = _wide(g, shape, device)
    lo, lr = le(shape, wide[:, 4 * A:5 * A], wide[:, :4 * A], targets, hw, sampled=torch.from_numpy(f["sampled"]))
    (lo + lr).backward()
    t64 = P.targets64(f["N"], f["sizes"], f["box_lists"], f["cells"], f["matched"].astype(np.int64))
    r0, _ = P.loss_sums(torch.from_numpy(obj).double(), torch.from_numpy(f["reg"]).double().reshape(-1, 4), f["sampled"], t64, 1.0 / 9)
    n = int((f["sampled"] != 0).sum())
    assert np.isfinite(float(lo)) and abs(float(lo) - float(r0) / n) <= 1e-5 * float(r0) / n and float(lo) > 1.0
    assert bool(torch.isfinite(wide.grad).all())
    wide.grad = None
    lo, lr = le(shape, wide[:, 4 * A:5 * A], wide[:, :4 * A], targets, hw, sampled=torch.zeros(f["sampled"].size, dtype=torch.uint8))
    (lo + lr).backward()
    assert float(lo) == 0.0 and float(lr) == 0.0 and float(wide.grad.abs().max()) == 0.0


def test_loss_draws_its_own_sample_with_one_host_read(device, gold_dir, references):
    """without the override: the sample is the restatement's for the evaluator's seed and call counter, the losses are the
    fp64 restatement's on that sample; plan_stats records the four launches and the one host read the Python side issues
    (its own count, not an observation of the device)"""
    from scan_amd.modeling import rpn
    f = load_case(gold_dir, CASES[1])
    B, frac = int(f["batch_size_per_image"]), float(f["positive_fraction"])
    le, shape, targets, hw = _loss_evaluator(gold_dir, CASES[1], batch_size_per_image=B, positive_fraction=frac, seed=11)
    wide, A = _wide(f, shape, device)
    lab, matched, _, img = references[CASES[1]]
    t64 = P.targets64(f["N"], f["sizes"], f["box_lists"], f["cells"], matched)
    seen = []
    for call in range(2):
        lo, lr = le(shape, wide[:, 4 * A:5 * A], wide[:, :4 * A], targets, hw)
        assert rpn.plan_stats == {"launches": 4, "host_reads": 1}
        s, counts = P.sample(lab, img, f["N"], B, frac, (11 + 0x9E3779B9 * call) & 0xffffffff)
        n = int(counts.sum())
        r0, r1 = P.loss_sums(torch.from_numpy(f["obj"]).double().reshape(-1), torch.from_numpy(f["reg"]).double().reshape(-1, 4), s,
                             t64, 1.0 / 9)
        np.testing.assert_allclose([float(lo.detach()), float(lr.detach())], [float(r0) / n, float(r1) / n], rtol=1e-5)
        seen.append(s)
    assert not np.array_equal(seen[0], seen[1])  # the counter moves the key


# ----------------------------------------------------------------------------- 4. the proposal decode
@pytest.mark.parametrize("name", CASES)
def test_decode_against_the_restatement_and_the_reference(device, gold_dir, name):
    """keep flags and clipped coordinates exactly the fp64 restatement's, boxes within BOX_TOL of it and of the reference's;
    the fixture holds a candidate with dw = 6 (above the clamp log(1000 / 16)) and one with dw = dh = -6.  bbox_reg is read
    through the pitch of the padded head output.  An index outside its level gives a zero box and keep 0."""
    from scan_amd import ops
    from scan_amd.modeling import rpn
    f = load_case(gold_dir, name)
    shape = ops.PyramidShape(f["N"], f["sizes"])
    wide, A = _wide(f, shape, device, "inf_obj", "inf_reg")
    wide = wide.detach()
    cells, ks = torch.from_numpy(f["cells"]).to(device), [int(k) for k in f["topk_k"]]
    hw_d = rpn.device_image_hw(f["image_hw"], device)
    idx = torch.from_numpy(f["topk_idx"]).to(device)
    boxes, keep = ops.rpn_decode_proposals(wide[:, :4 * A], shape, R.STRIDES, cells, idx, ks, hw_d, float(f["min_size"]))
    topk = list(np.split(f["topk_idx"], np.cumsum(ks)[:-1], axis=1))
    _, deltas, anchors, hw = P.candidate_geometry(topk, f["N"], f["sizes"], A, f["cells"], f["inf_reg"], f["image_hw"])
    want, want_keep = P.decode(deltas.reshape(-1, 4), anchors.reshape(-1, 4), hw.reshape(-1, 2), float(f["min_size"]))
    assert float(deltas[..., 2].max()) > P.CLIP
    got = boxes.cpu().numpy().reshape(-1, 4).astype(np.float64)
    assert np.array_equal(keep.cpu().numpy().reshape(-1).astype(bool), want_keep)
    if name == CASES[0]:
        assert not want_keep.all()
    H, W = f["image_hw"][0]
    hi = np.array([W - 1, H - 1, W - 1, H - 1], np.float64)
    clipped = (want == 0) | (want == hi)
    assert clipped.any() and np.array_equal(got[clipped], want[clipped])
    print(name, "worst box error", float(np.abs(got - want).max()))
    assert (np.abs(got - want) <= BOX_TOL * np.maximum(1, np.abs(want))).all()
    ref = f["topk_box"].reshape(-1, 4)
    assert (np.abs(got - ref) <= BOX_TOL * np.maximum(1, np.abs(ref))).all()
    bad = idx.clone()
    bad[0, 0], bad[0, ks[0]] = -1, f["sizes"][1][0] * f["sizes"][1][1] * A
    b2, k2 = ops.rpn_decode_proposals(wide[:, :4 * A], shape, R.STRIDES, cells, bad, ks, hw_d, 0.0)
    assert not b2[0, 0].any() and not b2[0, ks[0]].any() and int(k2[0, 0]) == 0 and int(k2[0, ks[0]]) == 0
    assert torch.equal(b2[1], boxes[1])


# ----------------------------------------------------------------------------- 5. the head
def test_head_matches_torch_cpu_restatement(device):
    """RPNHead (A = 3: the stacked 1x1 launch has 15 output columns) against F.conv2d + ReLU in fp64 on the CPU at the conv bars of
    test_conv2d_fwd_bwd for the active conv mode; the two outputs are column slices of one padded matrix"""
    from scan_amd import ops
    from scan_amd.modeling import rpn
    torch.manual_seed(33)
    head = rpn.RPNHead(256, 3)
    assert [k for k, _ in head.named_parameters()] == ["conv.weight", "conv.bias", "cls_logits.weight", "cls_logits.bias",
                                                       "bbox_pred.weight", "bbox_pred.bias"]
    for p in head.parameters():  # the initialisation (std 0.01, zero biases) would leave most of the arithmetic untested
        if p.dim() == 4:
            nn.init.normal_(p, std=(2.0 / (p.shape[1] * p.shape[2] * p.shape[3])) ** 0.5)
        else:
            nn.init.normal_(p, std=0.2)
    n, sizes = 2, [(6, 7), (3, 4), (2, 2), (1, 2), (1, 1)]
    shape = ops.PyramidShape(n, sizes)
    x = torch.randn(shape.rows, 256)
    Pm = {k: v.detach().clone().double().requires_grad_(True) for k, v in head.state_dict().items()}
    x64 = x.double().requires_grad_(True)

    def conv_rows(rows, w, b, relu, pad):
        outs = []
        for l, (h, wd) in enumerate(sizes):
            xl = rows[shape.row_off[l]:shape.row_off[l + 1]].view(n, h, wd, 256).permute(0, 3, 1, 2)
            y = F.conv2d(xl, w, b, padding=pad)
            outs.append((F.relu(y) if relu else y).permute(0, 2, 3, 1).reshape(n * h * wd, -1))
        return torch.cat(outs, 0)

    t = conv_rows(x64, Pm["conv.weight"], Pm["conv.bias"], True, 1)
    ref_obj = conv_rows(t, Pm["cls_logits.weight"], Pm["cls_logits.bias"], False, 0)
    ref_reg = conv_rows(t, Pm["bbox_pred.weight"], Pm["bbox_pred.bias"], False, 0)
    g = torch.Generator().manual_seed(5)
    gys = [torch.randn(t_.shape, generator=g, dtype=torch.float64) for t_ in (ref_obj, ref_reg)]
    ((ref_obj * gys[0]).sum() + (ref_reg * gys[1]).sum()).backward()
    head.to(device)
    for p in head.parameters():
        if p.dim() == 4:
            p.data = p.data.contiguous(memory_format=torch.channels_last)
    xd = x.to(device).requires_grad_(True)
    obj, reg = head(xd, shape)
    assert obj.shape == (shape.rows, 3) and reg.shape == (shape.rows, 12) and obj.stride(0) == reg.stride(0) == 16
    assert reg.data_ptr() % 16 == 0
    tol = deform_ref.bar(ops.CONV_MODE)
    deform_ref.assert_within(obj, ref_obj, tol, "objectness")
    deform_ref.assert_within(reg, ref_reg, tol, "bbox_reg")
    ((obj * gys[0].float().to(device)).sum() + (reg * gys[1].float().to(device)).sum()).backward()
    deform_ref.assert_within(xd.grad, x64.grad, tol, "dx")
    for k, p in head.named_parameters():
        deform_ref.assert_within(p.grad, Pm[k].grad, tol, k)


# ----------------------------------------------------------------------------- 6. the module
class _FixedHead(nn.Module):
    """stands in for the head: returns the fixture's head outputs whatever the features are"""

    def __init__(self, outs):
        super().__init__()
        self.outs = outs

    def forward(self, rows, shape):
        return self.outs


def _fixture_module(f, device, *opts):
    from scan_amd import config
    from scan_amd.modeling import factory
    n = int(f["pre_nms_top_n"])
    cfg = config.load("c2f", ["MODEL.FCOS_ON", False, "MODEL.RPN_ONLY", False, "MODEL.RPN.USE_FPN", True,
                              "MODEL.RPN.BATCH_SIZE_PER_IMAGE", int(f["batch_size_per_image"]),
                              "MODEL.RPN.PRE_NMS_TOP_N_TRAIN", n, "MODEL.RPN.PRE_NMS_TOP_N_TEST", n,
                              "MODEL.RPN.POST_NMS_TOP_N_TRAIN", int(f["post_nms_top_n"]),
                              "MODEL.RPN.POST_NMS_TOP_N_TEST", int(f["post_nms_top_n"]),
                              "MODEL.RPN.FPN_POST_NMS_TOP_N_TRAIN", int(f["fpn_post_nms_top_n"]),
                              "MODEL.RPN.FPN_POST_NMS_TOP_N_TEST", int(f["fpn_post_nms_top_n"]),
                              "MODEL.RPN.NMS_THRESH", float(f["nms_thresh"]), "MODEL.RPN.MIN_SIZE", int(f["min_size"])] + list(opts))
    m = factory.build_rpn(cfg, 256).to(device)
    assert np.array_equal(m.cells.numpy(), f["cells"])
    return m


def _boxlist_targets(f):
    from scan_amd.structures import BoxList
    H, W = f["image_hw"][0]
    out = []
    for b in f["box_lists"]:
        t = BoxList(torch.from_numpy(np.ascontiguousarray(b)), (W, H), mode="xyxy")
        t.add_field("labels", torch.ones(len(b), dtype=torch.int64))
        out.append(t)
    return out


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("mode", ["train", "test"])
def test_module_proposals_equal_the_reference(device, gold_dir, name, mode):
    """the same kept candidates in the same order (train: level-major after the batch-wide top-n, the ground truth appended;
    test: by falling objectness per image), boxes within BOX_TOL, scores within rtol 1e-5"""
    from scan_amd import ops
    from scan_amd.structures import BoxList
    f = load_case(gold_dir, name)
    N = f["N"]
    H, W = f["image_hw"][0]
    shape = ops.PyramidShape(N, f["sizes"])
    m = _fixture_module(f, device)
    outs = (torch.from_numpy(f["inf_obj"]).to(device), torch.from_numpy(f["inf_reg"]).to(device))
    m.head = _FixedHead(outs)
    m.train(mode == "train")
    feats = ops.PyramidLevels(torch.zeros((shape.rows, 256), device=device), shape)
    images = torch.zeros((N, 3, H, W), device=device)
    targets = _boxlist_targets(f)
    if mode == "train":
        props, losses = m(images, feats, targets)
        assert set(losses) == {"loss_objectness", "loss_rpn_box_reg"} and all(bool(torch.isfinite(v)) for v in losses.values())
        sel = m.box_selector_train
        _, idx = sel(shape, *outs, f["image_hw"], [(t.bbox, None) for t in targets], return_indices=True)
    else:
        with torch.no_grad():
            props, losses = m(images, feats)
        assert losses == {}
        _, idx = m.box_selector_test(shape, *outs, f["image_hw"], return_indices=True)
    o = 0
    for n, (p, k) in enumerate(zip(props, f[mode + "_count"])):
        k = int(k)
        assert isinstance(p, BoxList) and p.mode == "xyxy" and p.size == (W, H) and p.fields() == ["objectness"] and len(p) == k
        assert np.array_equal(idx[n].cpu().numpy(), f[mode + "_idx"][o:o + k])
        rb, rs = f[mode + "_box"][o:o + k], f[mode + "_score"][o:o + k]
        assert (np.abs(p.bbox.cpu().numpy() - rb) <= BOX_TOL * np.maximum(1, np.abs(rb))).all()
        np.testing.assert_allclose(p.get_field("objectness").cpu().numpy(), rs, rtol=1e-5)
        if mode == "train":
            g = int(f["ng"][n])
            assert (f["train_idx"][o + k - g:o + k] == -1).all() and np.array_equal(p.bbox.cpu().numpy()[k - g:], f["box_lists"][n])
        o += k


def test_rpn_only_sorts_and_proposals_feed_the_pooler(device, gold_dir):
    from scan_amd import ops
    from scan_amd.modeling.poolers import Pooler
    f = load_case(gold_dir, CASES[1])
    N = f["N"]
    H, W = f["image_hw"][0]
    shape = ops.PyramidShape(N, f["sizes"])
    outs = (torch.from_numpy(f["inf_obj"]).to(device), torch.from_numpy(f["inf_reg"]).to(device))
    torch.manual_seed(9)
    feats = ops.PyramidLevels(torch.randn((shape.rows, 256), device=device), shape)
    images = torch.zeros((N, 3, H, W), device=device)
    m = _fixture_module(f, device, "MODEL.RPN_ONLY", True)
    m.head = _FixedHead(outs)
    m.train()
    boxes, losses = m(images, feats, _boxlist_targets(f))
    assert boxes is None and set(losses) == {"loss_objectness", "loss_rpn_box_reg"}
    m.eval()
    with torch.no_grad():
        props, _ = m(images, feats)
    for p, k in zip(props, f["test_count"]):
        s = p.get_field("objectness")
        assert len(p) == int(k) and bool((s[1:] <= s[:-1]).all())
    pooler = Pooler((7, 7), tuple(1.0 / s for s in R.STRIDES), 2)
    y = pooler(list(feats), props)
    assert y.shape == (sum(len(p) for p in props), 256, 7, 7) and bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0


def test_factory_module_forward_backward_reaches_every_parameter(device, gold_dir):
    from scan_amd import ops
    from scan_amd.modeling import rpn
    f = load_case(gold_dir, CASES[0])
    N = f["N"]
    H, W = f["image_hw"][0]
    shape = ops.PyramidShape(N, f["sizes"])
    torch.manual_seed(7)
    m = _fixture_module(f, device)
    m.train()
    feats = ops.PyramidLevels(torch.randn((shape.rows, 256), device=device), shape)
    rpn.plan_stats.update(launches=0, host_reads=0)
    props, losses = m(torch.zeros((N, 3, H, W), device=device), feats, _boxlist_targets(f))
    assert rpn.plan_stats == {"launches": 4, "host_reads": 1}
    assert len(props) == N and all(p.has_field("objectness") and len(p) > int(g) for p, g in zip(props, f["ng"]))
    sum(losses.values()).backward()
    assert all(bool(torch.isfinite(v.detach())) and float(v.detach()) > 0 for v in losses.values()), losses
    for k, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k

"""Fast R-CNN box head on the GPU: matcher, sampler on the padded layout, gather, fused loss with its ordered twin, decode and
post-processor of csrc/roi_box.hip against the reference's fixtures (tests/golden/roi_box_*.npz) and the fp64 / integer
restatement (tests/roi_box_ref.py); the linear layers against fp64 F.linear within the 1x1 convolutions' bound
(tests/conv1x1_ref.py); the modules of modeling/roi_box_head.py and factory.GeneralizedRCNN."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv1x1_ref as C1
import roi_box_ref as B
from roi_box_ref import CASES, load_case

pytestmark = pytest.mark.gpu
BOX_TOL = 1e-4  # |box - ref| <= BOX_TOL * max(1, |ref|): test_gpu_rpn.py's bar for decoded boxes


def _dev(f, dev, *names):
    return [torch.from_numpy(np.ascontiguousarray(f[k])).to(dev) for k in names]


def _match(dev, props, n_props, boxes, glab, ng, bg, fg):
    from scan_amd import ops
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (props, n_props, boxes, glab, ng)]
    lab, matched = ops.roi_box_match(*t, bg, fg)
    return lab.cpu().numpy(), matched.cpu().numpy()


def _boxes_close(got, ref):
    return (np.abs(got - ref) <= BOX_TOL * np.maximum(1.0, np.abs(ref))).all()


@pytest.fixture(scope="module")
def cases(gold_dir):
    """per fixture the stored arrays and the restatement's labels / matched, computed once"""
    out = {}
    for name in CASES:
        f = load_case(gold_dir, name)
        lab, matched, _ = B.match(f["props"], f["np"], f["boxes"], f["glabels"], f["ng"], float(f["bg"]), float(f["fg"]))
        f["r_labels"], f["r_matched"] = lab, matched
        out[name] = f
    return out


# ----------------------------------------------------------------------------- 1. match
@pytest.mark.parametrize("name", CASES)
def test_match_equals_the_fixtures_and_the_restatement(device, cases, name):
    f = cases[name]
    lab, matched = _match(device, f["props"], f["np"], f["boxes"], f["glabels"], f["ng"], float(f["bg"]), float(f["fg"]))
    assert lab.dtype == np.int32 and np.array_equal(lab, f["labels"]) and np.array_equal(matched, f["matched"])
    assert np.array_equal(lab, f["r_labels"]) and np.array_equal(matched, f["r_matched"])
    pad = (np.arange(f["P"])[None] >= f["np"][:, None]).reshape(-1)
    assert pad.any() and (lab[pad] == -1).all() and (matched[pad] == 0).all()


@pytest.mark.parametrize("P, G", [(1, 1), (257, 40), (1025, 1), (1025, 40)])
def test_match_synthetic_sizes_and_empty_images(device, P, G):
    """three images: image 0 has no box (every real proposal is background), image 1 no proposal, image 2 both"""
    rs = np.random.RandomState(P + G)
    xy = rs.uniform(0, 200, (3, P, 2))
    props = np.concatenate([xy, xy + rs.uniform(4, 90, (3, P, 2))], 2).astype(np.float32)
    gxy = rs.uniform(0, 200, (3, G, 2))
    boxes = np.concatenate([gxy, gxy + rs.uniform(10, 90, (3, G, 2))], 2).astype(np.float32)
    glab = rs.randint(1, 81, (3, G)).astype(np.int64)
    n_props, ng = np.array([P, 0, max(P - 3, 1)], np.int32), np.array([0, G, G], np.int32)
    lab, matched = _match(device, props, n_props, boxes, glab, ng, 0.3, 0.5)
    want_l, want_m, _ = B.match(props, n_props, boxes, glab, ng, 0.3, 0.5)
    assert np.array_equal(lab, want_l) and np.array_equal(matched, want_m)
    lab = lab.reshape(3, P)
    assert (lab[0] == 0).all() and (lab[1] == -1).all() and (lab[2, n_props[2]:] == -1).all()
    if P > 1:
        assert (lab[2] > 0).any() or G == 1


def test_match_ties_and_threshold_equalities(device):
    """two identical boxes: the smaller index wins.  Box [0, 0, 9, 9] against proposal [0, 0, 9, 4]: IoU exactly 0.5 with +1
    extents (50 / 100) -- positive at FG 0.5, and not background at BG 0.5."""
    props = np.array([[[0, 0, 9, 4], [1.5, 1.5, 8.5, 8.5]]], np.float32)
    boxes = np.array([[[0, 0, 9, 9], [0, 0, 9, 9]]], np.float32)
    glab = np.array([[7, 3]], np.int64)
    one, two = np.array([2], np.int32), np.array([2], np.int32)
    lab, matched = _match(device, props, one, boxes, glab, two, 0.5, 0.5)
    assert lab.tolist() == [7, 7] and matched.tolist() == [0, 0]
    lab, _ = _match(device, props, one, boxes, glab, two, 0.5, 0.6)
    assert lab.tolist()[0] == -1  # between: not background at BG 0.5
    lab, _ = _match(device, props, one, boxes, glab, two, 0.6, 0.6)
    assert lab.tolist()[0] == 0
    lab, matched = _match(device, props, one, boxes[:, ::-1].copy(), glab, two, 0.5, 0.5)
    assert matched.tolist() == [0, 0]


# ----------------------------------------------------------------------------- 2. sampler through the padded layout
@pytest.mark.parametrize("case", list(CASES) + ["ties", "wide"])
def test_sampler_on_the_padded_layout_equals_the_restatement(device, cases, case):
    from scan_amd import ops
    if case in CASES:
        f = cases[case]
        N, P, lab = f["N"], f["P"], f["labels"].astype(np.int32)
        batch, frac, keys, seeds = int(f["batch_size_per_image"]), float(f["positive_fraction"]), None, (0, 7, 0xfffffffe)
    else:
        N, P, batch, frac, seeds = 3, 700, 64, 0.25, (3,)
        rs = np.random.RandomState(11)
        lab = rs.choice([-1, 0, 1, 5], size=N * P, p=[0.2, 0.5, 0.15, 0.15]).astype(np.int32)
        lab.reshape(N, P)[:, 650:] = -1  # padding
        lab.reshape(N, P)[1] = -1  # an image without proposals
        keys = rs.randint(0, 4, N * P).astype(np.int32) if case == "ties" else None
    shape = ops.PyramidShape(N, [(P, 1)])
    lab_d = torch.from_numpy(lab).to(device)
    keys_d = None if keys is None else torch.from_numpy(keys).to(device)
    for seed in seeds:
        want, want_counts = B.sample(lab, N, P, batch, frac, seed, keys)
        got, counts = ops.rpn_sample(shape, 1, lab_d, batch, frac, seed, keys_d)
        again, _ = ops.rpn_sample(shape, 1, lab_d, batch, frac, seed, keys_d)
        got = got.cpu().numpy()
        assert np.array_equal(got, want) and np.array_equal(counts.cpu().numpy(), want_counts), (case, seed)
        assert np.array_equal(again.cpu().numpy(), got)
        assert (got[lab < 0] == 0).all()  # padding and between-thresholds rows are never drawn


# ----------------------------------------------------------------------------- 3. gather
def _gather(dev, props, boxes, labels, matched, sampled, counts, R, weights):
    from scan_amd import ops
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (props, boxes, labels.astype(np.int32),
                                                                      matched.astype(np.int32), sampled, counts)]
    return ops.roi_box_gather(*t, R, weights)


@pytest.mark.parametrize("name", CASES)
def test_gather_equals_the_fixtures_and_the_restatement(device, cases, name):
    f = cases[name]
    w = tuple(float(v) for v in f["weights"])
    rois, lab, tg, src, counts = B.gather(f["props"], f["boxes"], f["labels"], f["matched"], f["sampled"].reshape(f["N"], f["P"]), w)
    R = rois.shape[0]
    assert R == int(f["sub_count"].sum())
    g_rois, g_lab, g_tg, g_src = _gather(device, f["props"], f["boxes"], f["labels"], f["matched"], f["sampled"], counts, R, w)
    assert np.array_equal(g_rois.cpu().numpy(), rois) and np.array_equal(g_src.cpu().numpy(), src)
    assert g_lab.dtype == torch.int32 and np.array_equal(g_lab.cpu().numpy(), lab)
    assert np.allclose(g_tg.cpu().numpy(), tg, rtol=1e-5, atol=1e-6)
    # the reference's own subsample: boxes and labels exactly, targets where the reference uses them (label > 0)
    assert np.array_equal(rois[:, 1:], f["sub_box"]) and np.array_equal(lab, f["sub_labels"])
    pos = f["sub_labels"] > 0
    assert pos.any() and np.allclose(g_tg.cpu().numpy()[pos], f["sub_targets"][pos], rtol=1e-5, atol=1e-6)
    assert (g_tg.cpu().numpy()[~pos] == 0).all()


@pytest.mark.parametrize("P", [5, 257, 1025])
def test_gather_offsets_skip_an_empty_image_and_stop_at_R(device, P):
    """N = 3 with nothing sampled in the middle image; the outputs are views into larger buffers filled with a guard pattern:
    nothing is written at or beyond row R, also when R is smaller than the counts say"""
    from scan_amd import ops
    rs = np.random.RandomState(P)
    N, G = 3, 2
    xy = rs.uniform(0, 100, (N, P, 2))
    props = np.concatenate([xy, xy + rs.uniform(4, 50, (N, P, 2))], 2).astype(np.float32)
    boxes = np.array([[[10.5, 10.5, 60.5, 60.5], [30.5, 20.5, 90.5, 70.5]]] * N, np.float32)
    labels = rs.choice([0, 3, 9], size=(N, P)).astype(np.int32)
    matched = np.where(labels > 0, rs.randint(0, G, (N, P)), 0).astype(np.int32)
    sampled = np.where(rs.rand(N, P) < 0.4, np.where(labels > 0, 1, 2), 0).astype(np.uint8)
    sampled[1] = 0
    sampled[0, P - 1] = 2 if labels[0, P - 1] == 0 else 1
    rois, lab, tg, src, counts = B.gather(props, boxes, labels, matched, sampled)
    R = rois.shape[0]
    assert counts[1].sum() == 0 and counts[2].sum() > 0
    g = _gather(device, props, boxes, labels.reshape(-1), matched.reshape(-1), sampled.reshape(-1), counts, R, B.WEIGHTS)
    assert np.array_equal(g[0].cpu().numpy(), rois) and np.array_equal(g[1].cpu().numpy(), lab)
    assert np.array_equal(g[3].cpu().numpy(), src) and np.allclose(g[2].cpu().numpy(), tg, rtol=1e-5, atol=1e-6)
    # the library call on guarded buffers, R two rows short of what the counts say
    short, extra = max(R - 2, 0), 8
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in
         (props, boxes, labels.reshape(-1), matched.reshape(-1), sampled.reshape(-1), counts)]
    bufs = [torch.full((R + extra, 5), -7.0, device=device), torch.full((R + extra,), -7, dtype=torch.int32, device=device),
            torch.full((R + extra, 4), -7.0, device=device), torch.full((R + extra,), -7, dtype=torch.int32, device=device)]
    ops.call("scan_roi_box_gather", ops._ptr(t[0]), N, P, ops._ptr(t[1]), G, ops._ptr(t[2]), ops._ptr(t[3]), ops._ptr(t[4]),
             ops._ptr(t[5]), *B.WEIGHTS, short, *[ops._ptr(b) for b in bufs], ops._stream())
    for b, want in zip(bufs, (rois, lab, tg, src)):
        b = b.cpu().numpy()
        assert (b[short:] == -7).all()
        assert np.allclose(b[:short], want[:short], rtol=1e-5, atol=1e-6)


# ----------------------------------------------------------------------------- 4. loss
def _loss(dev, cls, reg, labels, targets, pitch_pad=0):
    """-> (loss_classifier, loss_box_reg, d_cls, d_reg) of ops.roi_box_loss divided by R.  pitch_pad > 0: both head outputs are
    column slices of one wider matrix (box_regression first, as the predictor's stacked launch lays them out)"""
    from scan_amd import ops
    R, C = cls.shape
    nr = reg.shape[1]
    if pitch_pad:
        wide = torch.zeros((R, (nr + C + 3) // 4 * 4 + pitch_pad), device=dev)  # the pitch stays a multiple of 4
        wide[:, :nr], wide[:, nr:nr + C] = torch.from_numpy(reg), torch.from_numpy(cls)
        wide.requires_grad_(True)
        c, r = wide[:, nr:nr + C], wide[:, :nr]
    else:
        c, r = torch.from_numpy(cls).to(dev).requires_grad_(True), torch.from_numpy(reg).to(dev).requires_grad_(True)
    out = ops.roi_box_loss(c, r, torch.from_numpy(labels.astype(np.int32)).to(dev), torch.from_numpy(targets.astype(np.float32)).to(dev))
    out = out / max(R, 1)
    (out[0] + out[1]).backward()
    if pitch_pad:
        g = wide.grad.cpu().numpy()
        assert (g[:, nr + C:] == 0).all()
        return float(out[0].detach()), float(out[1].detach()), g[:, nr:nr + C], g[:, :nr]
    return float(out[0].detach()), float(out[1].detach()), c.grad.cpu().numpy(), r.grad.cpu().numpy()


def _check_loss(got, want, labels, C, agnostic):
    lc, lb, dc, dr = got
    wc, wb, wdc, wdr = want
    assert abs(lc - wc) <= 1e-5 * abs(wc) and abs(lb - wb) <= 1e-5 * max(abs(wb), 1e-30)
    assert np.allclose(dc, wdc, rtol=1e-4, atol=1e-7) and np.allclose(dr, wdr, rtol=1e-4, atol=1e-7)
    own = np.zeros(dr.shape, bool)  # every regression column that is not the label's own has gradient exactly zero
    for r, l in enumerate(labels):
        if l > 0:
            c0 = 4 if agnostic else 4 * int(l)
            own[r, c0:c0 + 4] = True
    assert (dr[~own] == 0).all()


@pytest.mark.parametrize("name", CASES)
def test_loss_with_the_references_sample(device, cases, name):
    f = cases[name]
    got = _loss(device, f["cls"], f["reg"], f["sub_labels"], f["sub_targets"])
    want = B.losses_and_grads(f["cls"], f["reg"], f["sub_labels"], f["sub_targets"].astype(np.float64), f["agnostic"])
    _check_loss(got, want, f["sub_labels"], f["C"], f["agnostic"])
    assert abs(got[0] - f["losses"][0]) <= 1e-4 * f["losses"][0] and abs(got[1] - f["losses"][1]) <= 1e-4 * f["losses"][1]
    assert np.allclose(got[2], f["d_cls"], rtol=1e-4, atol=1e-7) and np.allclose(got[3], f["d_reg"], rtol=1e-4, atol=1e-7)
    wide = _loss(device, f["cls"], f["reg"], f["sub_labels"], f["sub_targets"], pitch_pad=12)  # slices of the stacked launch
    assert wide[:2] == got[:2] and np.array_equal(wide[2], got[2]) and np.array_equal(wide[3], got[3])


@pytest.mark.parametrize("C, R, agnostic", [(2, 1, False), (2, 33, True), (9, 257, False), (81, 33, False), (81, 257, True),
                                            (200, 1, False), (200, 257, False), (200, 33, True)])
def test_loss_against_fp64_over_class_and_row_counts(device, C, R, agnostic):
    rs = np.random.RandomState(C * 1000 + R)
    cls = rs.randn(R, C).astype(np.float32) * 2
    reg = rs.randn(R, 8 if agnostic else 4 * C).astype(np.float32)
    labels = np.where(rs.rand(R) < 0.5, rs.randint(1, C, R), 0).astype(np.int64)
    labels[0] = C - 1
    # |d| on both sides of beta = 1 and at least 0.05: fp32 forms d = x - t with an absolute error of up to 2^-24 max(|x|, |t|),
    # which the quadratic branch turns into a relative error of 2^-23 max(|x|, |t|) / |d| of the term -- the 1e-5 bar on a sum of
    # four terms (R = 1) is a statement about the kernel only while no term is a cancellation
    own = np.stack([reg[r, (4 if agnostic else 4 * int(l)):(4 if agnostic else 4 * int(l)) + 4] for r, l in enumerate(labels)])
    targets = (own - rs.choice([-1.0, 1.0], (R, 4)) * rs.uniform(0.05, 2.5, (R, 4))).astype(np.float32)
    got = _loss(device, cls, reg, labels, targets)
    _check_loss(got, B.losses_and_grads(cls, reg, labels, targets.astype(np.float64), agnostic), labels, C, agnostic)


def test_loss_extreme_logits_and_no_rows(device):
    from scan_amd import ops
    rs = np.random.RandomState(4)
    R, C = 33, 81
    cls = rs.choice([-80.0, 80.0, 0.0], size=(R, C)).astype(np.float32)
    reg = rs.randn(R, 4 * C).astype(np.float32)
    labels = rs.randint(0, C, R).astype(np.int64)
    targets = rs.randn(R, 4).astype(np.float32)
    got = _loss(device, cls, reg, labels, targets)
    assert np.isfinite(got[0]) and np.isfinite(got[2]).all()
    _check_loss(got, B.losses_and_grads(cls, reg, labels, targets.astype(np.float64)), labels, C, False)
    empty = _loss(device, np.zeros((0, C), np.float32), np.zeros((0, 4 * C), np.float32), np.zeros((0,), np.int64),
                  np.zeros((0, 4), np.float32))
    assert empty[0] == 0.0 and empty[1] == 0.0 and empty[2].shape == (0, C) and empty[3].shape == (0, 4 * C)
    prev = ops.set_deterministic(True)
    try:
        empty = _loss(device, np.zeros((0, C), np.float32), np.zeros((0, 4 * C), np.float32), np.zeros((0,), np.int64),
                      np.zeros((0, 4), np.float32))
    finally:
        ops.set_deterministic(prev)
    assert empty[0] == 0.0 and empty[1] == 0.0


# ----------------------------------------------------------------------------- 5. ordered twin
def test_ordered_twin_is_byte_identical_and_selected_by_deterministic(device, monkeypatch):
    from scan_amd import ops
    rs = np.random.RandomState(8)
    R, C = 2100, 81  # 66 blocks: the per-block slots matter
    cls = torch.from_numpy(rs.randn(R, C).astype(np.float32)).to(device)
    reg = torch.from_numpy(rs.randn(R, 4 * C).astype(np.float32)).to(device)
    labels = torch.from_numpy(rs.randint(0, C, R).astype(np.int32)).to(device)
    targets = torch.from_numpy(rs.randn(R, 4).astype(np.float32)).to(device)
    atomic = ops.roi_box_loss(cls, reg, labels, targets).cpu().numpy()
    called = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (called.append(name), real(name, *a))[1])
    prev = ops.set_deterministic(True)
    try:
        one = ops.roi_box_loss(cls, reg, labels, targets).cpu().numpy()
        two = ops.roi_box_loss(cls, reg, labels, targets).cpu().numpy()
    finally:
        ops.set_deterministic(prev)
    assert called == ["scan_roi_box_loss_forward_ordered"] * 2
    assert one.tobytes() == two.tobytes()
    assert np.allclose(one, atomic, rtol=1e-5, atol=0)


# ----------------------------------------------------------------------------- 6. decode
@pytest.mark.parametrize("name", CASES)
def test_decode_equals_the_fixtures_and_the_restatement(device, cases, name):
    from scan_amd import ops
    f = cases[name]
    w, thr = tuple(float(v) for v in f["weights"]), float(f["score_thresh"])
    rois = f["inf_rois"].copy()
    rois = np.concatenate([rois, rois[:2]], 0)
    rois[-2, 0], rois[-1, 0] = f["N"], -1  # image indices out of range
    cls, reg = np.concatenate([f["inf_cls"], f["inf_cls"][:2]], 0), np.concatenate([f["inf_reg"], f["inf_reg"][:2]], 0)
    hw = torch.tensor(f["image_hw"], dtype=torch.int32, device=device)
    scores, boxes, cand = ops.roi_box_decode(*[torch.from_numpy(a).to(device) for a in (cls, reg, rois)], hw, w, thr)
    scores, boxes, cand = scores.cpu().numpy(), boxes.cpu().numpy(), cand.cpu().numpy()
    r_scores, r_boxes, r_cand, dw, raw = B.decode_all(cls, reg, rois, f["image_hw"], w, thr)
    assert (dw > B.CLIP).any() and (raw[:-2] != r_boxes[:-2]).any()  # the clamp and the clip are exercised
    assert np.array_equal(cand.astype(bool), r_cand)
    assert np.allclose(scores, r_scores, rtol=1e-5, atol=0) and _boxes_close(boxes, r_boxes)
    assert np.allclose(scores[:-2], f["ref_scores"], rtol=1e-5, atol=0) and _boxes_close(boxes[:-2], f["ref_boxes"])
    assert (scores[-2:] == 0).all() and (boxes[-2:] == 0).all() and (cand[-2:] == 0).all()


# ----------------------------------------------------------------------------- 7. post-processor
def _proposal_lists(f, dev, objectness=False):
    from scan_amd.structures import BoxList
    H, W = f["image_hw"][0]
    out = []
    for n in range(f["N"]):
        b = BoxList(torch.from_numpy(f["props"][n, :int(f["np"][n])].copy()).to(dev), (W, H), mode="xyxy")
        if objectness:
            b.add_field("objectness", torch.arange(len(b), dtype=torch.float32, device=dev))
        out.append(b)
    return out


def _check_detections(f, dets):
    assert [len(d) for d in dets] == f["det_count"].tolist()
    assert max(f["det_before_cap"]) > int(f["detections_per_img"]) >= max(f["det_count"])  # the cap binds in one image
    assert np.array_equal(torch.cat([d.get_field("labels") for d in dets]).cpu().numpy(), f["det_label"])
    assert np.allclose(torch.cat([d.get_field("scores") for d in dets]).cpu().numpy(), f["det_score"], rtol=1e-5, atol=0)
    assert _boxes_close(torch.cat([d.bbox for d in dets]).cpu().numpy(), f["det_box"])


@pytest.mark.parametrize("name", CASES)
def test_post_processor_equals_the_reference(device, cases, name):
    from scan_amd.modeling import roi_box_head as rb
    f = cases[name]
    pp = rb.PostProcessor(float(f["score_thresh"]), float(f["nms"]), int(f["detections_per_img"]),
                          tuple(float(v) for v in f["weights"]), f["agnostic"])
    dets = pp(tuple(_dev(f, device, "inf_cls", "inf_reg")), _proposal_lists(f, device))
    _check_detections(f, dets)
    assert dets[0].get_field("labels").dtype == torch.int64


@pytest.mark.parametrize("name", CASES[:2])
def test_box_head_eval_on_the_fixture_logits(device, cases, name, monkeypatch):
    """ROIBoxHead.eval() with the predictor's outputs replaced by the fixture's: the reference's detections"""
    from scan_amd.modeling import roi_box_head as rb
    f = cases[name]
    cfg = dict(rb.DEFAULT_SETTINGS, num_classes=f["C"], cls_agnostic_bbox_reg=f["agnostic"], mlp_head_dim=32, pooler_resolution=3,
               detections_per_img=int(f["detections_per_img"]), score_thresh=float(f["score_thresh"]), nms=float(f["nms"]))
    head = rb.ROIBoxHead(cfg, in_channels=8).to(device).eval()
    cls, reg = _dev(f, device, "inf_cls", "inf_reg")
    monkeypatch.setattr(head.predictor, "forward", lambda x: (cls, reg))
    H, W = f["image_hw"][0]
    feats = [torch.randn(f["N"], 8, -(-H // s), -(-W // s), device=device) for s in (8, 16, 32, 64, 128)]
    x, dets, losses = head(feats, _proposal_lists(f, device))
    assert losses == {} and tuple(x.shape) == (cls.shape[0], 32)
    _check_detections(f, dets)


# ----------------------------------------------------------------------------- 8. the linear layers
def _linear_case(device, R, K, D, seed):
    """linear_rows forward + backward against fp64 F.linear; -> the worst ratio to the bound of every result"""
    from scan_amd import ops
    from scan_amd.modeling import roi_box_head as rb
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, K, generator=g)
    w = torch.randn(D, K, generator=g) * 0.05
    b = torch.randn(D, generator=g)
    dy = torch.randn(R, D, generator=g)
    xd, wd, bd = (t.to(device).requires_grad_(True) for t in (x, w, b))
    y = rb.linear_rows(xd, wd, bd)
    assert tuple(y.shape) == (R, ops.pad4(D))
    y[:, :D].backward(dy.to(device))
    x6, w6, b6 = (t.double().requires_grad_(True) for t in (x, w, b))
    F.linear(x6, w6, b6).backward(dy.double())
    mode = ops.CONV_MODE
    ax, aw, ady = x.double().abs(), w.double().abs(), dy.double().abs()
    ratios = {
        "forward": C1.worst_ratio(y[:, :D].detach().cpu().numpy(), F.linear(x6, w6, b6).detach().numpy(),
                                  C1.bound_factor(mode, K) * (ax @ aw.t() + b.double().abs()).numpy()),
        "dx": C1.worst_ratio(xd.grad.cpu().numpy(), x6.grad.numpy(), C1.bound_factor(mode, D) * (ady @ aw).numpy()),
        "dw": C1.worst_ratio(wd.grad.cpu().numpy(), w6.grad.numpy(), C1.bound_factor(mode, R) * (ady.t() @ ax).numpy()),
        "db": C1.worst_ratio(bd.grad.cpu().numpy(), b6.grad.numpy(), C1.bound_factor(mode, R, colsum=True) * ady.sum(0).numpy()),
    }
    print("linear_rows R=%d K=%d D=%d %s: %s" % (R, K, D, mode, {k: round(v, 4) for k, v in ratios.items()}))
    return ratios


def test_linear_real_fc6_shape(device):
    """12544 -> 1024 at R = 64: the 1x1 kernels at a reduction length and a weight-gradient size they are not run at elsewhere"""
    ratios = _linear_case(device, 64, 12544, 1024, 1)
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("R", [1, 5, 300])
def test_extractor_and_predictor_against_fp64_linear(device, R):
    """8 input channels, resolution 3, MLP 32: every linear layer within the 1x1 convolutions' bound, fc6's permuted columns and
    the predictor's stacked launch included"""
    from scan_amd.modeling import roi_box_head as rb
    for K, D, seed in ((72, 32, R), (32, 32, R + 1), (32, 9 + 36, R + 2)):
        ratios = _linear_case(device, R, K, D, seed)
        assert max(ratios.values()) <= 1.0, (K, D, ratios)
    torch.manual_seed(R)
    fe = rb.FPN2MLPFeatureExtractor(8, 3, (0.125, 0.0625), 2, 32).to(device)
    pr = rb.FPNPredictor(32, 9).to(device)
    for p in list(fe.parameters()) + list(pr.parameters()):
        p.data.normal_(0, 0.3)
    pooled = torch.randn(R, 3, 3, 8, device=device)
    logits, deltas = pr(fe.mlp(pooled.reshape(R, -1), 8))
    assert tuple(logits.shape) == (R, 9) and tuple(deltas.shape) == (R, 36) and deltas.data_ptr() % 16 == 0
    (logits.sum() + deltas.sum()).backward()
    p6 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in list(fe.named_parameters()) + list(pr.named_parameters())}
    flat = pooled.cpu().double().permute(0, 3, 1, 2).reshape(R, -1)  # the reference's channel-major view of the pooled ROI
    h = F.relu(F.linear(F.relu(F.linear(flat, p6["fc6.weight"], p6["fc6.bias"])), p6["fc7.weight"], p6["fc7.bias"]))
    l6, d6 = F.linear(h, p6["cls_score.weight"], p6["cls_score.bias"]), F.linear(h, p6["bbox_pred.weight"], p6["bbox_pred.bias"])
    (l6.sum() + d6.sum()).backward()
    assert np.allclose(logits.detach().cpu().numpy(), l6.detach().numpy(), rtol=1e-4, atol=1e-4)
    assert np.allclose(deltas.detach().cpu().numpy(), d6.detach().numpy(), rtol=1e-4, atol=1e-4)
    for k, v in list(fe.named_parameters()) + list(pr.named_parameters()):
        assert v.grad is not None and np.allclose(v.grad.cpu().numpy(), p6[k].grad.numpy(), rtol=1e-3, atol=1e-3), k


# ----------------------------------------------------------------------------- 9. modules
@pytest.mark.parametrize("name", CASES[:2])
def test_box_head_training_step(device, cases, name):
    from scan_amd.modeling import roi_box_head as rb
    f = cases[name]
    cfg = dict(rb.DEFAULT_SETTINGS, num_classes=f["C"], cls_agnostic_bbox_reg=f["agnostic"], mlp_head_dim=32, pooler_resolution=3,
               bg_iou_threshold=float(f["bg"]), fg_iou_threshold=float(f["fg"]), batch_size_per_image=int(f["batch_size_per_image"]),
               positive_fraction=float(f["positive_fraction"]))
    torch.manual_seed(0)
    head = rb.ROIBoxHead(cfg, in_channels=8).to(device).train()
    H, W = f["image_hw"][0]
    feats = [torch.randn(f["N"], 8, -(-H // s), -(-W // s), device=device, requires_grad=True) for s in (8, 16, 32, 64, 128)]
    targets = [(torch.from_numpy(f["boxes"][n, :int(f["ng"][n])].copy()), torch.from_numpy(f["glabels"][n, :int(f["ng"][n])].copy()))
               for n in range(f["N"])]
    x, props, losses = head(feats, _proposal_lists(f, device, objectness=True), targets)
    assert rb.plan_stats == {"launches": 3, "host_reads": 1}
    assert sorted(losses) == ["loss_box_reg", "loss_classifier"] and all(torch.isfinite(v) for v in losses.values())
    sum(losses.values()).backward()
    for k, p in head.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    assert feats[0].grad is not None
    batch = int(f["batch_size_per_image"])
    assert [len(p) for p in props] == [min(batch, int(v)) for v in f["np"]] or f["bg"] != f["fg"]
    assert sum(len(p) for p in props) == x.shape[0]
    # fed the reference's own masks: its subsampled proposals, labels and targets
    le = head.loss_evaluator
    sub = le.subsample(_proposal_lists(f, device, objectness=True), targets, sampled=torch.from_numpy(f["sampled"].reshape(f["N"], f["P"])))
    assert [len(s) for s in sub] == f["sub_count"].tolist()
    assert np.array_equal(torch.cat([s.bbox for s in sub]).cpu().numpy(), f["sub_box"])
    lab = torch.cat([s.get_field("labels") for s in sub])
    assert lab.dtype == torch.int64 and np.array_equal(lab.cpu().numpy(), f["sub_labels"])
    pos = f["sub_labels"] > 0
    tg = torch.cat([s.get_field("regression_targets") for s in sub]).cpu().numpy()
    assert np.allclose(tg[pos], f["sub_targets"][pos], rtol=1e-5, atol=1e-6)
    assert np.array_equal(torch.cat([s.get_field("objectness") for s in sub]).cpu().numpy(), le.src.cpu().numpy().astype(np.float32))
    lc, lb = le(*_dev(f, device, "cls", "reg"))
    assert abs(float(lc) - f["losses"][0]) <= 1e-4 * f["losses"][0] and abs(float(lb) - f["losses"][1]) <= 1e-4 * f["losses"][1]


def _rcnn_cfg():
    from scan_amd import config
    return config.load("c2f", ["MODEL.FCOS_ON", False, "MODEL.RPN_ONLY", False, "MODEL.ATSS_ON", False, "MODEL.RETINANET_ON", False,
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
                         "MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM", 64])


def test_generalized_rcnn_trains_and_detects(device, gold_dir):
    from scan_amd.modeling import factory
    from scan_amd.structures import BoxList
    with open(os.path.join(gold_dir, "roi_box_keys.json")) as fh:
        ref_keys = json.load(fh)["state_dict"]
    torch.manual_seed(0)
    model = factory.build_detection_model(_rcnn_cfg()).to(device).train()
    assert {k[len("roi_heads.box."):] for k in model.state_dict() if k.startswith("roi_heads.box.")} == set(ref_keys)
    images = torch.randn(2, 3, 64, 96, device=device)
    targets = []
    for b, l in (([[6.3, 5.2, 40.6, 37.7], [48.4, 8.6, 88.3, 44.8]], [3, 8]), ([[30.4, 12.3, 70.7, 50.2]], [5])):
        t = BoxList(torch.tensor(b), (96, 64), mode="xyxy")
        t.add_field("labels", torch.tensor(l))
        targets.append(t)
    losses = model(images, targets)
    assert sorted(losses) == ["loss_box_reg", "loss_classifier", "loss_objectness", "loss_rpn_box_reg"]
    assert all(torch.isfinite(v) for v in losses.values())
    sum(losses.values()).backward()
    missing = [k for k, p in model.named_parameters() if p.requires_grad and p.grad is None]
    assert not missing, missing
    model.eval()
    with torch.no_grad():
        dets = model(images)
    assert len(dets) == 2
    for d in dets:
        assert len(d) <= 10 + 1 and d.has_field("scores") and d.has_field("labels") and d.bbox.shape[1] == 4
        assert d.get_field("labels").dtype == torch.int64 and (d.get_field("labels") >= 1).all()

"""Writes tests/golden/roi_box_*.npz and tests/golden/roi_box_keys.json: inputs and the REFERENCE's answers for the Fast R-CNN box
head (labels, matched boxes and encoded targets of every proposal, the sampler's masks under a fixed torch.manual_seed, the
subsampled proposals, both losses with their gradients, the test-time scores and decoded boxes, the final detections) and the
state_dict keys and shapes of the reference's ROIBoxHead built with FPN2MLPFeatureExtractor / FPNPredictor.  Runs on a CPU machine
that has the reference checkout (oracle/ref_harness.py); the fixtures hold data only.

    python tools/make_roi_box_golden.py

It runs the reference's own make_roi_box_loss_evaluator (prepare_targets, the sampler, subsample, __call__ with autograd) and
make_roi_box_post_processor (softmax, BoxCoder.decode, clip_to_image, the per-class boxlist_nms -- plain nms, which the harness
provides on the CPU -- and the kthvalue cap).

Fixture conditions, asserted here (tests/roi_box_ref.py: check_match_conditions, check_post_conditions) and re-asserted by
tests/test_roi_box_host.py from the stored inputs:
  * ground-truth coordinates are non-integer; no IoU of any (proposal, box) pair is within 1e-6 of BG or FG; no proposal's best IoU
    is within 1e-6 of its second best
  * one image has more positives than int(BATCH_SIZE_PER_IMAGE * POSITIVE_FRACTION) and one fewer; one image has fewer real
    proposals than BATCH_SIZE_PER_IMAGE; positives come from at least three classes; the band case has a between-thresholds proposal
  * no score is within 1e-6 of SCORE_THRESH; no two candidates of an image and class have scores within 1e-6; no same-class
    candidate pair has an IoU within 1e-6 of NMS; NMS removes at least one box per image; DETECTIONS_PER_IMG binds in one image and
    not in the other, and the k-th score is more than 1e-6 above the next; a decoded box is clipped and one has dw above the clamp
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_harness  # noqa: E402
import roi_box_ref as B  # noqa: E402

BATCH, FRAC, SCORE_THRESH, NMS, DETS = 16, 0.25, 0.05, 0.5, 10

BOXES_64x96 = [[[6.3, 5.2, 40.6, 37.7], [48.4, 8.6, 88.3, 44.8], [20.2, 36.1, 60.7, 60.3]], [[30.4, 12.3, 70.7, 50.2]]]
BOXES_128x256 = [[[12.3, 10.2, 80.6, 75.7], [96.4, 16.6, 176.3, 88.8], [150.2, 60.1, 240.7, 120.3]], [[60.4, 24.3, 140.7, 100.2]]]
CASES = {
    "roi_box_64x96": dict(image_hw=(64, 96), seed=41, C=9, bg=0.5, fg=0.5, agnostic=False, boxes=BOXES_64x96,
                          labels=[[3, 8, 1], [5]], n_jitter=(7, 2), n_bg=(11, 10)),
    "roi_box_band_64x96": dict(image_hw=(64, 96), seed=42, C=9, bg=0.3, fg=0.6, agnostic=True, boxes=BOXES_64x96,
                               labels=[[3, 8, 1], [5]], n_jitter=(7, 2), n_bg=(11, 10)),
    "roi_box_c81_128x256": dict(image_hw=(128, 256), seed=43, C=81, bg=0.5, fg=0.5, agnostic=False, boxes=BOXES_128x256,
                                labels=[[80, 17, 64], [2]], n_jitter=(7, 2), n_bg=(11, 10)),
}


def make_proposals(c, rs):
    """per image: jittered copies of every box (from a tight fit to a loose one), background boxes, then the ground truth itself
    (the RPN appends it in training)"""
    H, W = c["image_hw"]
    out = []
    for n, gt in enumerate(c["boxes"]):
        gt = np.array(gt, np.float32)
        rows = []
        for b in gt:
            w, h = b[2] - b[0], b[3] - b[1]
            for k in range(c["n_jitter"][n]):
                amp = 0.04 + 0.09 * k  # k = 0: nearly the box; the last ones fall below 0.3
                d = rs.uniform(-amp, amp, 4) * np.array([w, h, w, h])
                rows.append(np.clip(b + d, 0, [W - 1, H - 1, W - 1, H - 1]))
        for _ in range(c["n_bg"][n]):
            x, y = rs.uniform(0, W - 12), rs.uniform(0, H - 12)
            rows.append([x, y, min(x + rs.uniform(8, W / 3), W - 1), min(y + rs.uniform(8, H / 3), H - 1)])
        rows = np.array(rows, np.float32)[rs.permutation(len(rows))]
        out.append(np.concatenate([np.round(rows, 2).astype(np.float32), gt], 0))
    return out


def make_case(name, c, write=True):
    from fcos_core.modeling.roi_heads.box_head.inference import make_roi_box_post_processor
    from fcos_core.modeling.roi_heads.box_head.loss import make_roi_box_loss_evaluator
    from fcos_core.structures.bounding_box import BoxList
    H, W = c["image_hw"]
    N, C = len(c["boxes"]), c["C"]
    Cr = 2 if c["agnostic"] else C
    cfg = ref_harness.make_cfg(["MODEL.ROI_HEADS.USE_FPN", True, "MODEL.ROI_HEADS.BG_IOU_THRESHOLD", c["bg"],
                                "MODEL.ROI_HEADS.FG_IOU_THRESHOLD", c["fg"], "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", BATCH,
                                "MODEL.ROI_HEADS.POSITIVE_FRACTION", FRAC, "MODEL.ROI_HEADS.SCORE_THRESH", SCORE_THRESH,
                                "MODEL.ROI_HEADS.NMS", NMS, "MODEL.ROI_HEADS.DETECTIONS_PER_IMG", DETS,
                                "MODEL.ROI_BOX_HEAD.NUM_CLASSES", C, "MODEL.CLS_AGNOSTIC_BBOX_REG", c["agnostic"]])
    weights = tuple(float(w) for w in cfg.MODEL.ROI_HEADS.BBOX_REG_WEIGHTS)
    rs = np.random.RandomState(c["seed"])
    g = torch.Generator().manual_seed(c["seed"])
    per_image = make_proposals(c, rs)
    props, n_props = B.pad(per_image)
    boxes, ng = B.pad(c["boxes"])
    glab, _ = B.pad(c["labels"], width=0, dtype=np.int64)
    Pn = props.shape[1]

    def proposal_lists():
        out = []
        for p in per_image:
            bl = BoxList(torch.from_numpy(p.copy()), (W, H), mode="xyxy")
            bl.add_field("objectness", torch.ones(len(p)))
            out.append(bl)
        return out

    targets = ref_harness.make_targets(c["boxes"], c["labels"], (H, W))
    le = make_roi_box_loss_evaluator(cfg)
    # ---- training: labels and targets of every proposal, the sampler's draw, the subsampled proposals, the losses
    lab_im, reg_im = le.prepare_targets(proposal_lists(), targets)
    idx_im = [le.match_targets_to_proposals(p, t).get_field("matched_idxs") for p, t in zip(proposal_lists(), targets)]
    torch.manual_seed(c["seed"])
    pos_im, neg_im = le.fg_bg_sampler(lab_im)
    torch.manual_seed(c["seed"])  # the sampler is the only consumer of the generator: the same draw
    sub = le.subsample(proposal_lists(), targets)
    labels = np.full((N, Pn), -1, np.int32)
    matched = np.zeros((N, Pn), np.int32)
    reg_all = np.zeros((N, Pn, 4), np.float32)
    sampled = np.zeros((N, Pn), np.uint8)
    for n in range(N):
        k = int(n_props[n])
        labels[n, :k] = lab_im[n].numpy()
        matched[n, :k] = np.where(lab_im[n].numpy() > 0, idx_im[n].clamp(min=0).numpy(), 0)
        reg_all[n, :k] = reg_im[n].numpy()
        sampled[n, :k] = pos_im[n].numpy().astype(np.uint8) + 2 * neg_im[n].numpy().astype(np.uint8)
        assert np.array_equal(sub[n].bbox.numpy(), per_image[n][np.nonzero(sampled[n, :k])[0]]), (name, "subsample order")
    Rn = sum(len(s) for s in sub)
    cls = torch.randn(Rn, C, generator=g).requires_grad_(True)
    reg = (torch.randn(Rn, 4 * Cr, generator=g) * 0.5).requires_grad_(True)
    lc, lb = le([cls], [reg])
    (lc + lb).backward()

    # the restatement's view of the same inputs: the conditions that make the reference unambiguous
    r_labels, r_matched, ious = B.match(props, n_props, boxes, glab, ng, c["bg"], c["fg"])
    f = dict(N=N, P=Pn, boxes=boxes, ng=ng, np=n_props, bg=c["bg"], fg=c["fg"], batch_size_per_image=BATCH, positive_fraction=FRAC)
    n_pos = B.check_match_conditions(f, ious, r_labels)
    assert np.array_equal(r_labels, labels.reshape(-1)) and np.array_equal(r_matched, matched.reshape(-1)), (name, "restatement disagrees")
    for n in range(N):
        lab = labels[n, :int(n_props[n])]
        num_pos = min(int((lab > 0).sum()), int(BATCH * FRAC))
        assert int((sampled[n] == 1).sum()) == num_pos and int((sampled[n] == 2).sum()) == min(int((lab == 0).sum()), BATCH - num_pos)

    # ---- inference on every proposal: image 0 gives every ROI one strong class, image 1 only the ROIs on its box
    rois = np.concatenate([np.concatenate([np.full((len(p), 1), n, np.float32), p], 1) for n, p in enumerate(per_image)], 0)
    Ri = rois.shape[0]
    inf_cls = torch.randn(Ri, C, generator=g) * 0.5
    inf_reg = torch.randn(Ri, 4 * Cr, generator=g) * 0.5
    inf_cls[:, 0] += 5.0
    img = rois[:, 0].astype(np.int64)
    lab_flat = [labels[n, :int(n_props[n])] for n in range(N)]
    strong = []
    for r in range(Ri):
        own = int(np.concatenate(lab_flat)[r])
        if img[r] == 0:
            j = own if own > 0 else int(torch.randint(1, C, (1,), generator=g))
        else:
            j = own if own > 0 else 0
        if j > 0:
            inf_cls[r, j] += 3.0 + 3.0 * float(torch.rand(1, generator=g))
        strong.append(j)
    first = int(np.nonzero(np.array(strong) > 0)[0][0])
    inf_reg.view(Ri, Cr, 4)[first, 1 if c["agnostic"] else strong[first], 2] = 6.0 * weights[2]  # dw above the clamp
    pp = make_roi_box_post_processor(cfg)
    with torch.no_grad():
        dets = pp((inf_cls, inf_reg), proposal_lists())
        prob = torch.softmax(inf_cls, -1)
        dec = pp.box_coder.decode((inf_reg[:, -4:] if c["agnostic"] else inf_reg).view(Ri, -1), torch.from_numpy(rois[:, 1:].copy()))
        if c["agnostic"]:
            dec = dec.repeat(1, C)
        ref_boxes = BoxList(dec.reshape(-1, 4), (W, H), mode="xyxy").clip_to_image(remove_empty=False).bbox.reshape(Ri, C, 4)
    scores, dboxes, cand, dw, raw = B.decode_all(inf_cls.numpy(), inf_reg.numpy(), rois, [(H, W)] * N, weights, SCORE_THRESH)
    before = B.check_post_conditions(dict(N=N, score_thresh=SCORE_THRESH, nms=NMS, detections_per_img=DETS, inf_rois=rois),
                                     scores, dboxes, cand, dw, raw)
    mine = B.postprocess(scores, dboxes, cand, rois, N, NMS, DETS)
    for n in range(N):
        assert np.array_equal(mine[n][1], dets[n].get_field("labels").numpy()), (name, "restatement's detections disagree", n)
        assert np.allclose(dboxes[mine[n][0], mine[n][1]], dets[n].bbox.numpy(), atol=1e-3)
    out = dict(
        image_hw_one=np.array([H, W]), num_classes=np.array(C), cls_agnostic=np.array(c["agnostic"]), bg=np.array(c["bg"]),
        fg=np.array(c["fg"]), batch_size_per_image=np.array(BATCH), positive_fraction=np.array(FRAC),
        weights=np.array(weights, np.float64), score_thresh=np.array(SCORE_THRESH), nms=np.array(NMS),
        detections_per_img=np.array(DETS), seed=np.array(c["seed"]),
        props=props, np=n_props, boxes=boxes, glabels=glab, ng=ng, labels=labels.reshape(-1), matched=matched.reshape(-1),
        reg_targets_all=reg_all.reshape(-1, 4), sampled=sampled.reshape(-1), n_pos=np.array(n_pos),
        sub_count=np.array([len(s) for s in sub]), sub_box=torch.cat([s.bbox for s in sub]).numpy(),
        sub_labels=torch.cat([s.get_field("labels") for s in sub]).numpy(),
        sub_targets=torch.cat([s.get_field("regression_targets") for s in sub]).numpy(),
        cls=cls.detach().numpy(), reg=reg.detach().numpy(), losses=np.array([float(lc.detach()), float(lb.detach())], np.float64),
        d_cls=cls.grad.numpy(), d_reg=reg.grad.numpy(),
        inf_rois=rois, inf_cls=inf_cls.numpy(), inf_reg=inf_reg.numpy(), ref_scores=prob.numpy(), ref_boxes=ref_boxes.numpy(),
        det_before_cap=np.array(before), det_count=np.array([len(d) for d in dets]),
        det_box=torch.cat([d.bbox for d in dets]).numpy(), det_score=torch.cat([d.get_field("scores") for d in dets]).numpy(),
        det_label=torch.cat([d.get_field("labels") for d in dets]).numpy())
    if write:
        path = os.path.join(ROOT, "tests", "golden", name + ".npz")
        np.savez_compressed(path, **out)
        print("%s: proposals=%s positives per image=%s sampled=%s losses=%s detections before the cap=%s after=%s -> %d bytes"
              % (name, n_props.tolist(), n_pos, out["sub_count"].tolist(), out["losses"], before, out["det_count"].tolist(),
                 os.path.getsize(path)))
    return out


def write_keys():
    """the reference's ROIBoxHead with the FPN extractor and predictor: state_dict keys and shapes"""
    from fcos_core.modeling.roi_heads.box_head.box_head import build_roi_box_head
    cfg = ref_harness.make_cfg(["MODEL.ROI_HEADS.USE_FPN", True, "MODEL.ROI_BOX_HEAD.FEATURE_EXTRACTOR", "FPN2MLPFeatureExtractor",
                                "MODEL.ROI_BOX_HEAD.PREDICTOR", "FPNPredictor", "MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION", 7,
                                "MODEL.ROI_BOX_HEAD.POOLER_SCALES", (0.125, 0.0625, 0.03125, 0.015625),
                                "MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO", 2, "MODEL.ROI_BOX_HEAD.NUM_CLASSES", 81])
    head = build_roi_box_head(cfg, 256)
    keys = {k: list(v.shape) for k, v in head.state_dict().items()}
    path = os.path.join(ROOT, "tests", "golden", "roi_box_keys.json")
    with open(path, "w") as f:
        json.dump({"in_channels": 256, "resolution": 7, "mlp_head_dim": 1024, "num_classes": 81, "state_dict": keys}, f, indent=1,
                  sort_keys=True)
        f.write("\n")
    print("roi_box_keys.json:", sorted(keys))


if __name__ == "__main__":
    ref_harness.setup()
    for name, c in CASES.items():
        make_case(name, c)
    write_keys()

"""Writes tests/golden/roi_mask_*.npz and tests/golden/roi_mask_keys.json: inputs and the REFERENCE's answers for the Mask R-CNN
mask head in binary-mask mode (the positives of the box head's sample with the ground-truth index its loss re-matches, the M x M
mask targets, the loss with its gradient, the test-time probabilities and the pasted masks) and the state_dict keys and shapes of
the reference's ROIMaskHead.  Runs on a CPU machine that has the reference checkout (oracle/ref_harness.py); the fixtures hold
data only.

    python tools/make_roi_mask_golden.py

It runs the reference's own make_roi_box_loss_evaluator (for the sample), keep_only_positive_boxes, make_roi_mask_loss_evaluator
(prepare_targets, __call__ under autograd), MaskPostProcessor and Masker.  The cases take the boxes, labels and proposal
construction of tools/make_roi_box_golden.py and add, per image size, one narrow ground-truth box at the right border and four
hand-placed positive proposals; the masks are ellipses and unions of two rectangles inside their boxes.  Logits are not stored:
tests/roi_mask_ref.make_logits reproduces them from the stored seed.  The archive is written with fixed zip timestamps, so a rerun
gives the same bytes.

Fixture conditions, asserted here (tests/roi_mask_ref.py: check_target_conditions, check_paste_conditions) and re-asserted by
tests/test_roi_mask_host.py from the stored inputs:
  * positive proposals include coordinates ending in .5 with an even and with an odd integer part; one crop touches each image
    border; one crop is 1 pixel wide; one image has a single ground-truth box; no mask leaves or fills its box
  * the ground-truth index the reference's mask loss re-matches equals the box plan's at every positive
  * the reference's target is never 1 where the integer rule gives 0; the two differ only where the rule gives 1 (the
    reference's fp32 rounding zeros), at fewer than 10 % of the rule's ones per case and at more than zero pixels in some case
  * no fp64 interpolated value of the paste is within 1e-5 of the threshold; no expanded box coordinate is within 1e-4 of an
    integer; an expanded box leaves the image on each side and one has a negative coordinate; one box is narrower than 2 pixels
"""
import io
import json
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import ref_harness  # noqa: E402
import make_roi_box_golden as BG  # noqa: E402
import roi_box_ref as B  # noqa: E402
import roi_mask_ref as R  # noqa: E402

BATCH, FRAC, THRESH = 64, 0.5, 0.5  # every positive of the cases is sampled

# per image size: the narrow box added to image 0 and the hand-placed positives of image 0 (left + top border with both .5
# parities, right border, bottom border, the 1-pixel-wide crop)
EXTRA = {
    (64, 96): dict(box=[94.2, 50.2, 95.3, 62.4],
                   props=[[0.0, 0.0, 42.5, 39.5], [47.5, 7.5, 95.5, 45.5], [19.5, 35.5, 61.5, 63.5], [94.6, 50.5, 95.4, 62.5]],
                   dets=[[[-3.2, 10.3, 20.7, 40.6], [70.3, -2.4, 99.2, 30.7], [30.2, 40.3, 60.8, 70.9], [50.3, 20.2, 51.1, 30.6],
                          [10.4, 8.3, 44.7, 36.2], [60.2, 30.6, 61.9, 31.7]], [[28.3, 10.7, 72.6, 52.4], [5.2, 3.3, 9.7, 60.4]]]),
    (128, 256): dict(box=[254.2, 90.2, 255.3, 110.4],
                     props=[[0.0, 0.0, 82.5, 77.5], [149.5, 59.5, 255.5, 121.5], [148.5, 58.5, 242.5, 127.5],
                            [254.6, 90.5, 255.4, 110.5]],
                     dets=[[[-6.2, 20.3, 40.7, 80.6], [200.3, -4.4, 259.2, 60.7], [60.2, 80.3, 120.8, 134.9],
                            [100.3, 40.2, 101.1, 60.6], [20.4, 16.3, 88.7, 72.2]], [[58.3, 20.7, 144.6, 104.4]]]),
}
CASES = {
    "roi_mask_64x96": dict(base="roi_box_64x96", extra_label=2, M=28, predictor="MaskRCNNC4Predictor", logit_seed=141, inf_seed=241),
    "roi_mask_m14_64x96": dict(base="roi_box_64x96", extra_label=2, M=14, predictor="MaskRCNNConv1x1Predictor", logit_seed=142,
                               inf_seed=242),
    "roi_mask_c81_128x256": dict(base="roi_box_c81_128x256", extra_label=33, M=28, predictor="MaskRCNNC4Predictor", logit_seed=143,
                                 inf_seed=246),
}


def save_npz(path, arrays):
    """np.savez_compressed with fixed zip timestamps: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in arrays:
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def make_masks(boxes, H, W):
    """per box an ellipse (even index) or a union of two rectangles (odd index) inside it, not filling it"""
    ys, xs = np.mgrid[0:H, 0:W]
    out = np.zeros((len(boxes), H, W), np.uint8)
    for g, (x0, y0, x1, y1) in enumerate(boxes):
        w, h = x1 - x0, y1 - y0
        if w < 4:  # the narrow box: one column, short of the box's ends
            out[g] = (xs == int(np.ceil(x0))) & (ys >= y0 + 0.2 * h) & (ys <= y1 - 0.2 * h)
        elif g % 2 == 0:
            out[g] = ((xs - (x0 + x1) / 2) / (0.45 * w)) ** 2 + ((ys - (y0 + y1) / 2) / (0.45 * h)) ** 2 <= 1
        else:
            a = (xs >= x0 + 0.1 * w) & (xs <= x0 + 0.6 * w) & (ys >= y0 + 0.1 * h) & (ys <= y0 + 0.9 * h)
            b = (xs >= x0 + 0.3 * w) & (xs <= x0 + 0.9 * w) & (ys >= y0 + 0.3 * h) & (ys <= y0 + 0.6 * h)
            out[g] = a | b
    return out


def make_case(name, c, write=True):
    from fcos_core.modeling.roi_heads.box_head.loss import make_roi_box_loss_evaluator
    from fcos_core.modeling.roi_heads.mask_head.inference import make_roi_mask_post_processor
    from fcos_core.modeling.roi_heads.mask_head.loss import make_roi_mask_loss_evaluator
    from fcos_core.modeling.roi_heads.mask_head.mask_head import keep_only_positive_boxes
    from fcos_core.structures.bounding_box import BoxList
    from fcos_core.structures.segmentation_mask import SegmentationMask
    base = BG.CASES[c["base"]]
    H, W = base["image_hw"]
    ex = EXTRA[(H, W)]
    C, M, seed = base["C"], c["M"], base["seed"]
    gt_boxes = [list(base["boxes"][0]) + [ex["box"]]] + [list(b) for b in base["boxes"][1:]]
    gt_labels = [list(base["labels"][0]) + [c["extra_label"]]] + [list(l) for l in base["labels"][1:]]
    N = len(gt_boxes)
    cfg = ref_harness.make_cfg(["MODEL.ROI_HEADS.USE_FPN", True, "MODEL.ROI_HEADS.BG_IOU_THRESHOLD", base["bg"],
                                "MODEL.ROI_HEADS.FG_IOU_THRESHOLD", base["fg"], "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", BATCH,
                                "MODEL.ROI_HEADS.POSITIVE_FRACTION", FRAC, "MODEL.ROI_BOX_HEAD.NUM_CLASSES", C, "MODEL.MASK_ON", True,
                                "MODEL.ROI_MASK_HEAD.RESOLUTION", M, "MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS", True,
                                "MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS_THRESHOLD", THRESH])
    per_image = BG.make_proposals(base, np.random.RandomState(seed))
    per_image[0] = np.concatenate([per_image[0], np.array(ex["props"], np.float32), np.array([ex["box"]], np.float32)], 0)
    props, n_props = B.pad(per_image)
    boxes, ng = B.pad(gt_boxes)
    glab, _ = B.pad(gt_labels, width=0, dtype=np.int64)
    Pn = props.shape[1]
    masks_im = [make_masks(b, H, W) for b in gt_boxes]
    flat, moff, mhw = R.pack_masks(masks_im)

    def proposal_lists():
        return [BoxList(torch.from_numpy(p.copy()), (W, H), mode="xyxy") for p in per_image]

    targets = ref_harness.make_targets(gt_boxes, gt_labels, (H, W))
    for t, m in zip(targets, masks_im):
        t.add_field("masks", SegmentationMask(torch.from_numpy(m.copy()), (W, H), mode="mask"))
    # ---- the box head's sample (the reference's draw), then the mask head's view of it
    le = make_roi_box_loss_evaluator(cfg)
    lab_im, _ = le.prepare_targets(proposal_lists(), targets)
    torch.manual_seed(seed)
    pos_im, neg_im = le.fg_bg_sampler(lab_im)
    torch.manual_seed(seed)
    sub = le.subsample(proposal_lists(), targets)
    sampled = np.zeros((N, Pn), np.uint8)
    for n in range(N):
        k = int(n_props[n])
        sampled[n, :k] = pos_im[n].numpy().astype(np.uint8) + 2 * neg_im[n].numpy().astype(np.uint8)
        assert int((sampled[n] == 1).sum()) == int((lab_im[n] > 0).sum()), (name, "a positive was not sampled")
    r_labels, r_matched, ious = B.match(props, n_props, boxes, glab, ng, base["bg"], base["fg"])
    for q in ious:
        assert ((np.abs(q - base["bg"]) > 1e-6) & (np.abs(q - base["fg"]) > 1e-6)).all(), "an IoU within 1e-6 of a threshold"
    rois, sub_labels, _, src, _ = B.gather(props, boxes, r_labels, r_matched, sampled)
    assert np.array_equal(rois[:, 1:], torch.cat([s.bbox for s in sub]).numpy()), (name, "subsample order")
    assert np.array_equal(sub_labels, torch.cat([s.get_field("labels") for s in sub]).numpy()), (name, "subsample labels")
    pos_rows, pos_rois, pos_labels, pos_gt = R.positives(sub_labels, rois, src, r_matched, Pn)
    pos, _ = keep_only_positive_boxes(sub)
    me = make_roi_mask_loss_evaluator(cfg)
    ref_gt = torch.cat([me.match_targets_to_proposals(p, t).get_field("matched_idxs") for p, t in zip(pos, targets)]).numpy()
    assert np.array_equal(ref_gt, pos_gt), (name, "the mask loss's re-match differs from the box plan's matched")
    assert np.array_equal(torch.cat([p.bbox for p in pos]).numpy(), pos_rois[:, 1:])
    ref_labels, ref_masks = me.prepare_targets(pos, targets)
    assert np.array_equal(torch.cat(ref_labels).numpy(), pos_labels)
    ref_targets = torch.cat(ref_masks, 0).numpy()
    Rp = ref_targets.shape[0]
    assert set(np.unique(ref_targets)) <= {0.0, 1.0} and ref_targets.shape == (Rp, M, M)
    ref_targets = ref_targets.astype(np.uint8)
    rule = R.targets_rule(masks_im, pos_rois, pos_gt, M)
    f = dict(H=H, W=W, pos_rois=pos_rois, ng=ng, boxes=boxes, masks_per_image=masks_im)
    n_diff, n_ones = R.check_target_conditions(f, rule, ref_targets)
    fp32 = np.stack([R.target_fp32(masks_im[int(r[0])][int(g)], r[1:], M) for r, g in zip(pos_rois, pos_gt)])
    assert (rule >= fp32).all()
    # ---- loss and gradient on the reference's own targets
    logits = torch.from_numpy(R.make_logits(c["logit_seed"], Rp, C, M)).requires_grad_(True)
    loss = me(pos, logits, targets)
    loss.backward()
    d = logits.grad.numpy()
    own = np.zeros(d.shape, bool)
    own[np.arange(Rp), pos_labels] = True
    assert (d[~own] == 0).all()
    d_label = d[np.arange(Rp), pos_labels]
    # ---- inference: hand-placed detections, the reference's probabilities and pasted masks
    det_box = [np.array(b, np.float32).reshape(-1, 4) for b in ex["dets"]]
    K = sum(len(b) for b in det_box)
    rs = np.random.RandomState(c["inf_seed"])
    det_label = rs.randint(1, C, K).astype(np.int64)
    inf_logits = torch.from_numpy(R.make_logits(c["inf_seed"], K, C, M, scale=3.0))
    dets, k0 = [], 0
    for b in det_box:
        bl = BoxList(torch.from_numpy(b.copy()), (W, H), mode="xyxy")
        bl.add_field("labels", torch.from_numpy(det_label[k0:k0 + len(b)].copy()))
        dets.append(bl)
        k0 += len(b)
    with torch.no_grad():
        pasted = make_roi_mask_post_processor(cfg)(inf_logits, dets)
        cfg.MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS = False
        probs = make_roi_mask_post_processor(cfg)(inf_logits, dets)
    ref_prob = torch.cat([p.get_field("mask") for p in probs]).numpy()
    ref_paste = torch.cat([p.get_field("mask") for p in pasted]).numpy()
    assert ref_prob.shape == (K, 1, M, M) and ref_paste.shape == (K, 1, H, W) and ref_paste.dtype == np.uint8
    fp = dict(H=H, W=W, M=M, K=K, thresh=THRESH, det_box=np.concatenate(det_box, 0))
    mine = R.check_paste_conditions(fp, R.sigmoid(inf_logits.numpy()[np.arange(K), det_label]))
    assert np.array_equal(mine, ref_paste[:, 0]), (name, "the restatement's paste differs", int((mine != ref_paste[:, 0]).sum()))
    # ---- SegmentationMask binary mode: crop / resize / transpose of image 0's masks
    seg = SegmentationMask(torch.from_numpy(masks_im[0].copy()), (W, H), mode="mask")
    seg_box = np.array(ex["props"][2], np.float32)
    crop = seg.crop(torch.from_numpy(seg_box))
    seg_resized = crop.resize((20, 12)).get_mask_tensor().numpy()
    out = dict(
        image_hw_one=np.array([H, W]), num_classes=np.array(C), resolution=np.array(M), predictor=np.array(c["predictor"]),
        bg=np.array(base["bg"]), fg=np.array(base["fg"]), batch_size_per_image=np.array(BATCH), positive_fraction=np.array(FRAC),
        thresh=np.array(THRESH), seed=np.array(seed), logit_seed=np.array(c["logit_seed"]), inf_seed=np.array(c["inf_seed"]),
        props=props, np=n_props, boxes=boxes, glabels=glab, ng=ng, sampled=sampled.reshape(-1), masks_bits=R.bits(flat), moff=moff,
        mhw=mhw, sub_count=np.array([len(s) for s in sub]), sub_labels=sub_labels, sub_rois=rois, sub_src=src,
        matched=r_matched.astype(np.int32), pos_rows=pos_rows, pos_rois=pos_rois, pos_labels=pos_labels, pos_gt=pos_gt,
        ref_targets_bits=R.bits(ref_targets), n_rounding=np.array(n_diff), n_rule_ones=np.array(n_ones),
        loss=np.array(float(loss.detach()), np.float64), d_label=d_label.astype(np.float32),
        det_count=np.array([len(b) for b in det_box]), det_box=np.concatenate(det_box, 0), det_label=det_label,
        ref_prob=ref_prob, ref_paste_bits=R.bits(ref_paste),
        seg_box=seg_box, seg_crop_size=np.array(crop.size), seg_crop_bits=R.bits(crop.get_mask_tensor().numpy()),
        seg_resize_bits=R.bits(seg_resized), seg_flip_bits=R.bits(seg.transpose(0).get_mask_tensor().numpy()))
    if write:
        path = os.path.join(ROOT, "tests", "golden", name + ".npz")
        save_npz(path, out)
        print("%s: proposals=%s sampled=%s positives=%d rule ones=%d rounding zeros of the reference=%d loss=%.6f detections=%s "
              "-> %d bytes" % (name, n_props.tolist(), out["sub_count"].tolist(), Rp, n_ones, n_diff, float(out["loss"]),
                               out["det_count"].tolist(), os.path.getsize(path)))
    return out


def write_keys():
    """the reference's ROIMaskHead with the FPN extractor and either predictor: state_dict keys and shapes"""
    from fcos_core.modeling.roi_heads.mask_head.mask_head import build_roi_mask_head
    keys = {}
    for pred, res in (("MaskRCNNC4Predictor", 28), ("MaskRCNNConv1x1Predictor", 14)):
        cfg = ref_harness.make_cfg(["MODEL.MASK_ON", True, "MODEL.ROI_HEADS.USE_FPN", True, "MODEL.ROI_BOX_HEAD.NUM_CLASSES", 81,
                                    "MODEL.ROI_MASK_HEAD.FEATURE_EXTRACTOR", "MaskRCNNFPNFeatureExtractor",
                                    "MODEL.ROI_MASK_HEAD.PREDICTOR", pred, "MODEL.ROI_MASK_HEAD.POOLER_RESOLUTION", 14,
                                    "MODEL.ROI_MASK_HEAD.POOLER_SCALES", (0.125, 0.0625, 0.03125, 0.015625),
                                    "MODEL.ROI_MASK_HEAD.POOLER_SAMPLING_RATIO", 2, "MODEL.ROI_MASK_HEAD.RESOLUTION", res,
                                    "MODEL.ROI_MASK_HEAD.SHARE_BOX_FEATURE_EXTRACTOR", False])
        head = build_roi_mask_head(cfg, 256)
        keys[pred] = {k: list(v.shape) for k, v in head.state_dict().items()}
    path = os.path.join(ROOT, "tests", "golden", "roi_mask_keys.json")
    with open(path, "w") as f:
        json.dump({"in_channels": 256, "pooler_resolution": 14, "num_classes": 81, "state_dict": keys}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("roi_mask_keys.json:", {k: sorted(v) for k, v in keys.items()})


if __name__ == "__main__":
    ref_harness.setup()
    total = 0
    for name, c in CASES.items():
        total += int(make_case(name, c)["n_rounding"])
    assert total > 0, "no case exercises the reference's rounding zeros"
    write_keys()

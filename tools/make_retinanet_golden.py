"""Writes tests/golden/retinanet_*.npz: inputs and the REFERENCE's answers for the RetinaNet head (cell anchors, labels, matched
boxes, regression targets, the two losses with their gradients, pre-NMS candidates, final detections).  Runs on a CPU machine
that has the reference checkout (oracle/ref_harness.py); the fixtures hold data only.

    python tools/make_retinanet_golden.py

It runs the reference's own make_anchor_generator_retinanet, RetinaNetLossComputation.prepare_targets / __call__ (autograd) and
RetinaNetPostProcessor.forward, select_over_all_levels included (its boxlist_nms is plain nms, which the harness provides on
the CPU).

Fixture conditions, asserted here and re-asserted by tests/test_retinanet_host.py from the stored inputs:
  * box coordinates are non-integer; no anchor has two boxes within 1e-6 IoU of its maximum (torch.max's choice is then the only
    one); every box overlaps some anchor
  * every case has an anchor in [BG, FG), an anchor that is positive only through the low-quality rule and a box whose best IoU
    is below BG
  * inference: no two candidate scores of an image lie within 1e-6 of each other, none within 1e-6 of INFERENCE_TH, and
    PRE_NMS_TOP_N binds on the finest level
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
np.float = float  # rpn/anchor_generator.py:251 (numpy < 1.20 spelling)

from oracle import ref_harness  # noqa: E402
import retinanet_ref as R  # noqa: E402

BG, FG, TH, TOP_N, DETS = 0.4, 0.5, 0.05, 50, 20

CASES = {
    "retinanet_64x96": dict(
        image_hw=(64, 96), num_classes=2, seed=21,
        boxes=[[[20.3, 10.2, 70.6, 50.7], [24.1, 8.4, 76.3, 55.8], [17.3, 9.2, 19.1, 11.4]], [[0.4, 20.3, 9.7, 44.2]]],
        labels=[[1, 1, 1], [1]]),
    "retinanet_128x256": dict(
        image_hw=(128, 256), num_classes=3, seed=22,
        boxes=[[[40.3, 30.2, 150.6, 100.7], [52.1, 24.4, 160.3, 110.8], [97.3, 9.2, 99.1, 11.4]], [[243.4, 50.3, 255.3, 90.2]]],
        labels=[[1, 2, 1], [2]]),
}


def make_case(name, c):
    from fcos_core.modeling.box_coder import BoxCoder
    from fcos_core.modeling.rpn.anchor_generator import make_anchor_generator_retinanet
    from fcos_core.modeling.rpn.retinanet.inference import make_retinanet_postprocessor
    from fcos_core.modeling.rpn.retinanet.loss import make_retinanet_loss_evaluator
    from fcos_core.modeling.rpn.utils import permute_and_flatten
    from fcos_core.structures.boxlist_ops import cat_boxlist
    H, W = c["image_hw"]
    N, C = len(c["boxes"]), c["num_classes"] - 1
    sizes = [(-(-H // s), -(-W // s)) for s in R.STRIDES]
    off = R.row_offsets(N, sizes)
    M = off[-1]
    cfg = ref_harness.make_cfg(["MODEL.RETINANET_ON", True, "MODEL.RETINANET.NUM_CLASSES", c["num_classes"],
                                "MODEL.RETINANET.BG_IOU_THRESHOLD", BG, "MODEL.RETINANET.FG_IOU_THRESHOLD", FG,
                                "MODEL.RETINANET.INFERENCE_TH", TH, "MODEL.RETINANET.PRE_NMS_TOP_N", TOP_N,
                                "TEST.DETECTIONS_PER_IMG", DETS])
    Rn = cfg.MODEL.RETINANET
    A = len(Rn.ASPECT_RATIOS) * Rn.SCALES_PER_OCTAVE
    g = torch.Generator().manual_seed(c["seed"])
    rows = {"logits": torch.randn(M, A * C, generator=g) - 2.0, "reg": torch.randn(M, A * 4, generator=g) * 0.5}
    for t in rows.values():
        t.requires_grad_(True)

    def levels(t):  # row matrix -> the reference's per-level [N, c, h, w]
        return [t[off[l]:off[l + 1]].view(N, h, w, t.shape[1]).permute(0, 3, 1, 2) for l, (h, w) in enumerate(sizes)]

    def to_index_order(per_image):  # per image [anchors, ...] (level-major within the image) -> (level, image, y, x, a)
        out = []
        for l, (h, w) in enumerate(sizes):
            a0 = sum(hh * ww for hh, ww in sizes[:l]) * A
            out += [p[a0:a0 + h * w * A] for p in per_image]
        return torch.cat(out, 0)

    images = types.SimpleNamespace(image_sizes=[(H, W)] * N)
    gen = make_anchor_generator_retinanet(cfg)
    anchors = gen(images, levels(rows["logits"]))
    cells = torch.stack([b for b in gen.cell_anchors], 0)  # [L, A, 4] fp32
    one = ref_harness.make_cfg(["MODEL.RETINANET.ASPECT_RATIOS", (1.0,), "MODEL.RETINANET.SCALES_PER_OCTAVE", 1])
    cells_a1 = torch.stack([b for b in make_anchor_generator_retinanet(one).cell_anchors], 0)  # A = 1
    targets = ref_harness.make_targets(c["boxes"], c["labels"], (H, W))
    coder = BoxCoder(weights=(10., 10., 5., 5.))
    le = make_retinanet_loss_evaluator(cfg, coder)
    le.box_cls_loss_func.gamma, le.box_cls_loss_func.alpha = [Rn.LOSS_GAMMA], [Rn.LOSS_ALPHA]  # sigmoid_focal_loss_cpu indexes them
    cat_anchors = [cat_boxlist(a) for a in anchors]
    lab_im, reg_im = le.prepare_targets(cat_anchors, targets)
    idx_im = [le.match_targets_to_anchors(a, t, le.copied_fields).get_field("matched_idxs") for a, t in zip(cat_anchors, targets)]
    labels = to_index_order(lab_im).to(torch.int64)
    matched = torch.where(labels > 0, to_index_order(idx_im).clamp(min=0), torch.zeros_like(labels))
    reg_t = to_index_order(reg_im)
    anchors_all = to_index_order([a.bbox for a in cat_anchors])
    lc, lr = le(anchors, levels(rows["logits"]), levels(rows["reg"]), targets)
    (lc + lr).backward()

    # the restatement's view of the same inputs: the conditions that make the reference unambiguous
    tg = [(np.array(b, np.float32), np.array(l)) for b, l in zip(c["boxes"], c["labels"])]
    for b, _ in tg:
        assert (b != np.round(b)).all(), (name, "integer coordinate")
    r_labels, r_matched, ious = R.match(N, sizes, tg, cells.numpy(), bg=BG, fg=FG)
    img = R.anchors_in_order(N, sizes, cells.numpy())[1]
    stats = R.check_case_conditions(ious, [r_labels[img == n] for n in range(N)], BG, FG)
    assert np.array_equal(r_labels, labels.numpy()) and np.array_equal(r_matched, matched.numpy()), (name, "restatement disagrees")
    assert np.array_equal(R.anchors_in_order(N, sizes, cells.numpy(), dtype=np.float32)[0], anchors_all.numpy())

    # inference: a class bias that makes a good part of the (anchor, class) pairs candidates; small deltas so that neighbouring
    # anchors' boxes overlap and NMS suppresses
    inf = {"logits": torch.randn(M, A * C, generator=g) * 1.5 - 3.0, "reg": torch.randn(M, A * 4, generator=g) * 0.3}
    pp = make_retinanet_postprocessor(cfg, coder, is_train=False)
    pp.eval()
    cand = {k: [] for k in ("idx", "cls", "box", "score")}
    per_image_scores = [[] for _ in range(N)]
    with torch.no_grad():
        for l, (h, w) in enumerate(sizes):
            res = pp.forward_for_single_feature_map([a[l] for a in anchors], levels(inf["logits"])[l], levels(inf["reg"])[l])
            # the scores as the reference forms them (same memory layout into sigmoid: the same bits)
            probs = permute_and_flatten(levels(inf["logits"])[l], N, A, C, h, w).sigmoid()
            for n, bl in enumerate(res):
                prob = probs[n]
                assert ((prob - TH).abs() > 1e-6).all(), (name, "a score within 1e-6 of INFERENCE_TH")
                nz = torch.nonzero(prob > TH)
                sc = prob[nz[:, 0], nz[:, 1]]
                assert len(bl) == min(nz.shape[0], TOP_N), (name, l, n, len(bl), nz.shape[0])
                if l == 0:
                    assert nz.shape[0] > TOP_N, (name, "PRE_NMS_TOP_N does not bind on level 0", nz.shape[0])
                got = bl.get_field("scores")
                assert got.unique().numel() == got.numel()
                pos_of = {s_: i for i, s_ in enumerate(got.tolist())}  # the reference returns its top-k as an unordered set
                keep = torch.tensor([i for i, s_ in enumerate(sc.tolist()) if s_ in pos_of], dtype=torch.int64)
                assert keep.numel() == len(bl), (name, l, n, keep.numel(), len(bl))
                if len(bl):
                    assert float(sc[keep].min()) >= float(torch.sort(sc)[0][-len(bl)])
                ref_i = torch.tensor([pos_of[s_] for s_ in sc[keep].tolist()], dtype=torch.int64)
                assert torch.equal(nz[keep, 1] + 1, bl.get_field("labels")[ref_i])
                a = keep  # candidates in (anchor, class) order
                cand["idx"].append((off[l] + n * h * w) * A + nz[a, 0])
                cand["cls"].append(nz[a, 1] + 1)
                cand["box"].append(bl.bbox[ref_i])
                cand["score"].append(got[ref_i])
                per_image_scores[n].append(got)
        for n in range(N):
            s = torch.sort(torch.cat(per_image_scores[n]))[0]
            assert (s[1:] - s[:-1] > 1e-6).all(), (name, "two candidate scores within 1e-6")
        dets = pp(anchors, levels(inf["logits"]), levels(inf["reg"]))
    G = max(len(b) for b in c["boxes"])
    boxes = np.zeros((N, G, 4), np.float32)
    glabels = np.zeros((N, G), np.int64)
    for n, (b, l) in enumerate(zip(c["boxes"], c["labels"])):
        boxes[n, :len(b)], glabels[n, :len(b)] = b, l
    out = dict(
        image_hw=np.array([H, W]), sizes=np.array(sizes), num_classes=np.array(c["num_classes"]), num_anchors=np.array(A),
        gamma=np.array(Rn.LOSS_GAMMA), alpha=np.array(Rn.LOSS_ALPHA), beta=np.array(Rn.BBOX_REG_BETA),
        bbox_reg_weight=np.array(Rn.BBOX_REG_WEIGHT), bg=np.array(BG), fg=np.array(FG), inference_th=np.array(TH),
        pre_nms_top_n=np.array(TOP_N), nms_th=np.array(Rn.NMS_TH), detections_per_img=np.array(DETS),
        anchor_sizes=np.array(Rn.ANCHOR_SIZES, np.float32), aspect_ratios=np.array(Rn.ASPECT_RATIOS, np.float64),
        octave=np.array(Rn.OCTAVE), scales_per_octave=np.array(Rn.SCALES_PER_OCTAVE), cells=cells.numpy(),
        cells_a1=cells_a1.numpy(),
        boxes=boxes, glabels=glabels, ng=np.array([len(b) for b in c["boxes"]], np.int32), stats=np.array(stats),
        logits=rows["logits"].detach().numpy(), reg=rows["reg"].detach().numpy(),
        labels=labels.numpy().astype(np.int32), matched=matched.numpy().astype(np.int32), reg_targets=reg_t.numpy(),
        losses=np.array([float(lc.detach()), float(lr.detach())], np.float64),
        d_logits=rows["logits"].grad.numpy(), d_reg=rows["reg"].grad.numpy(),
        inf_logits=inf["logits"].numpy(), inf_reg=inf["reg"].numpy(),
        cand_idx=torch.cat(cand["idx"]).numpy(), cand_cls=torch.cat(cand["cls"]).numpy(),
        cand_box=torch.cat(cand["box"]).numpy(), cand_score=torch.cat(cand["score"]).numpy(),
        det_count=np.array([len(d) for d in dets]),
        det_box=torch.cat([d.bbox for d in dets]).numpy(), det_score=torch.cat([d.get_field("scores") for d in dets]).numpy(),
        det_label=torch.cat([d.get_field("labels") for d in dets]).numpy())
    path = os.path.join(ROOT, "tests", "golden", name + ".npz")
    np.savez_compressed(path, **out)
    print("%s: anchors=%d positives=%d (between, low-quality, weak boxes)=%s candidates=%d detections=%s losses=%s -> %d bytes"
          % (name, M * A, int((labels > 0).sum()), stats, out["cand_idx"].size, out["det_count"], out["losses"],
             os.path.getsize(path)))


if __name__ == "__main__":
    ref_harness.setup()
    for name, c in CASES.items():
        make_case(name, c)

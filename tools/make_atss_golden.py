"""Writes tests/golden/atss_*.npz: inputs and the REFERENCE's answers for the ATSS head (anchors, labels, encoded targets,
centerness targets, the three losses with their gradients, pre-NMS candidates).  Runs on a CPU machine that has the reference
checkout (oracle/ref_harness.py); the fixtures hold data only.

    python tools/make_atss_golden.py

It runs the reference's own make_anchor_generator_atss, ATSSLossComputation.prepare_targets / __call__ (autograd) and
ATSSPostProcessor.forward_for_single_feature_map.  The reference's ml_nms has no CPU build: the fixtures stop before NMS.

Fixture conditions, asserted here and re-asserted by tests/test_atss_host.py from the stored inputs -- under them the
reference's assignment does not depend on how torch.topk / torch.max break ties, nor on rounding in the threshold:
  * box coordinates are non-integer
  * for every (box, level) the k-th and (k+1)-th smallest distances differ
  * no candidate's IoU lies within 1e-5 of its box's threshold
  * no anchor sees two positive IoUs within 1e-5 of each other
and every case has a box whose centre is within one stride of the image border, a box with no positives and at least one
anchor that is positive for two boxes.
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
import atss_ref  # noqa: E402

GAMMA, ALPHA, TOPK, REG_W = 2.0, 0.25, 9, 2.0

CASES = {
    "atss_64x96": dict(
        image_hw=(64, 96), num_classes=2, seed=11,
        boxes=[[[20.3, 10.2, 70.6, 50.7], [24.1, 8.4, 76.3, 55.8], [17.3, 9.2, 19.1, 11.4]], [[0.4, 20.3, 9.7, 44.2]]],
        labels=[[1, 1, 1], [1]]),
    "atss_128x256": dict(
        image_hw=(128, 256), num_classes=3, seed=12,
        boxes=[[[40.3, 30.2, 150.6, 100.7], [52.1, 24.4, 160.3, 110.8], [97.3, 9.2, 99.1, 11.4]], [[243.4, 50.3, 255.3, 90.2]]],
        labels=[[1, 2, 1], [2]]),
}


def check_conditions(name, c, sizes, details, labels):
    """the fixture conditions (module docstring) on the fp64 restatement's details"""
    H, W = c["image_hw"]
    contested, border, empty = 0, False, False
    for n, d in enumerate(details):
        b = torch.tensor(c["boxes"][n], dtype=torch.float64)
        assert (b != b.round()).all(), (name, "integer coordinate")
        assert (d["dist_gap"] > 0).all(), (name, "k-th and (k+1)-th distance tie", d["dist_gap"])
        assert ((d["cand_iou"] - d["thr"][None]).abs() > 1e-5).all(), (name, "candidate IoU at the threshold")
        cx, cy = (b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2
        border |= bool(((cx < 8) | (cy < 8) | (cx > W - 8) | (cy > H - 8)).any())
        empty |= bool((~d["pos"].any(0)).any())
        seen = {}
        for g in range(b.shape[0]):
            for r, v in zip(d["cand_row"][d["pos"][:, g], g].tolist(), d["cand_iou"][d["pos"][:, g], g].tolist()):
                seen.setdefault(r, []).append(v)
        for r, vs in seen.items():
            if len(vs) > 1:
                contested += 1
                vs = sorted(vs)
                assert min(b_ - a_ for a_, b_ in zip(vs, vs[1:])) > 1e-5, (name, "two equal positive IoUs on row", r)
    assert contested > 0, (name, "no anchor is positive for two boxes")
    assert border, (name, "no box centre within one stride of the border")
    assert empty, (name, "no box without positives")
    return contested


def make_case(name, c):
    from fcos_core.modeling.rpn.anchor_generator import make_anchor_generator_atss
    from fcos_core.modeling.rpn.atss.atss import BoxCoder
    from fcos_core.modeling.rpn.atss.inference import make_atss_postprocessor
    from fcos_core.modeling.rpn.atss.loss import ATSSLossComputation
    from fcos_core.structures.boxlist_ops import cat_boxlist
    H, W = c["image_hw"]
    N, C = len(c["boxes"]), c["num_classes"] - 1
    sizes = [(-(-H // s), -(-W // s)) for s in atss_ref.STRIDES]
    off = atss_ref.row_offsets(N, sizes)
    M = off[-1]
    cfg = ref_harness.make_cfg(["MODEL.ATSS_ON", True, "MODEL.ATSS.NUM_CLASSES", c["num_classes"], "MODEL.ATSS.TOPK", TOPK,
                                "MODEL.ATSS.REG_LOSS_WEIGHT", REG_W, "MODEL.ATSS.POSITIVE_TYPE", "ATSS",
                                "MODEL.ATSS.REGRESSION_TYPE", "BOX", "MODEL.ATSS.INFERENCE_TH", 0.05,
                                "MODEL.ATSS.PRE_NMS_TOP_N", 1000])
    g = torch.Generator().manual_seed(c["seed"])
    rows = {"logits": torch.randn(M, C, generator=g) - 2.0, "reg": torch.randn(M, 4, generator=g) * 0.5,
            "ctr": torch.randn(M, 1, generator=g)}
    for t in rows.values():
        t.requires_grad_(True)

    def levels(t):  # row matrix -> the reference's per-level [N, c, h, w]
        return [t[off[l]:off[l + 1]].view(N, h, w, t.shape[1]).permute(0, 3, 1, 2) for l, (h, w) in enumerate(sizes)]

    def to_rows(per_image):  # per image [A, ...] (level-major within the image) -> pyramid row order
        out = []
        for l, (h, w) in enumerate(sizes):
            a0 = sum(hh * ww for hh, ww in sizes[:l])
            out += [p[a0:a0 + h * w] for p in per_image]
        return torch.cat(out, 0)

    images = types.SimpleNamespace(image_sizes=[(H, W)] * N)
    anchors = make_anchor_generator_atss(cfg)(images, levels(rows["logits"]))
    targets = ref_harness.make_targets(c["boxes"], c["labels"], (H, W))
    coder = BoxCoder(cfg)
    le = ATSSLossComputation(cfg, coder)
    le.cls_loss_func.gamma, le.cls_loss_func.alpha = [GAMMA], [ALPHA]  # sigmoid_focal_loss_cpu indexes them
    lab_im, reg_im = le.prepare_targets(targets, anchors)
    anchors_rows = to_rows([cat_boxlist(a).bbox for a in anchors])
    labels, reg_t = to_rows(lab_im), to_rows(reg_im)
    pos_inds = torch.nonzero(labels > 0).squeeze(1)
    ctr_pos = le.compute_centerness_targets(reg_t[pos_inds], anchors_rows[pos_inds])
    lc, lr, lctr = le(levels(rows["logits"]), levels(rows["reg"]), levels(rows["ctr"]), targets, anchors)
    (lc + lr + lctr).backward()

    # the restatement's view of the same inputs: the conditions that make the reference unambiguous
    tg = [(torch.tensor(b, dtype=torch.float32), torch.tensor(l)) for b, l in zip(c["boxes"], c["labels"])]
    ref_labels, ref_matched, details = atss_ref.assign(N, sizes, tg, topk=TOPK)
    contested = check_conditions(name, c, sizes, details, ref_labels)
    assert torch.equal(ref_labels, labels), (name, "restatement and reference disagree on labels")

    # inference: shifted class bias so that a good part of the (row, class) pairs are candidates; small deltas so that
    # neighbouring anchors' boxes overlap and NMS suppresses
    inf = {"logits": torch.randn(M, C, generator=g) * 1.5 - 2.5, "reg": torch.randn(M, 4, generator=g) * 0.3,
           "ctr": torch.randn(M, 1, generator=g)}
    pp = make_atss_postprocessor(cfg, coder)
    cand = {k: [] for k in ("row", "cls", "box", "score")}
    with torch.no_grad():
        for l, (h, w) in enumerate(sizes):
            res = pp.forward_for_single_feature_map(levels(inf["logits"])[l], levels(inf["reg"])[l], levels(inf["ctr"])[l],
                                                    [a[l] for a in anchors])
            prob = levels(inf["logits"])[l].sigmoid()
            for n, bl in enumerate(res):
                # the reference returns no row: (location, class) of its candidates = nonzero(prob > th) (pre_nms_top_n does not
                # bind), matched to its output by score
                nz = torch.nonzero(prob[n].permute(1, 2, 0).reshape(h * w, C) > 0.05)
                assert len(bl) == nz.shape[0] < 1000, (name, l, n, len(bl), nz.shape[0])
                sc = torch.sqrt(prob[n].permute(1, 2, 0).reshape(h * w, C)[nz[:, 0], nz[:, 1]] *
                                levels(inf["ctr"])[l][n, 0].reshape(-1).sigmoid()[nz[:, 0]])
                a, b = torch.argsort(sc), torch.argsort(bl.get_field("scores"))
                assert torch.equal(sc[a], bl.get_field("scores")[b]) and sc.unique().numel() == sc.numel()
                assert torch.equal(nz[a, 1] + 1, bl.get_field("labels")[b])
                inv = torch.empty_like(a)
                inv[a] = b  # reference entry of candidate i
                cand["row"].append(off[l] + n * h * w + nz[:, 0])
                cand["cls"].append(nz[:, 1] + 1)
                cand["box"].append(bl.bbox[inv])
                cand["score"].append(bl.get_field("scores")[inv])
    G = max(len(b) for b in c["boxes"])
    boxes = np.zeros((N, G, 4), np.float32)
    glabels = np.zeros((N, G), np.int64)
    for n, (b, l) in enumerate(zip(c["boxes"], c["labels"])):
        boxes[n, :len(b)], glabels[n, :len(b)] = b, l
    out = dict(
        image_hw=np.array([H, W]), sizes=np.array(sizes), num_classes=np.array(c["num_classes"]), topk=np.array(TOPK),
        gamma=np.array(GAMMA), alpha=np.array(ALPHA), reg_loss_weight=np.array(REG_W),
        anchor_sizes=np.array(cfg.MODEL.ATSS.ANCHOR_SIZES, np.float32), boxes=boxes, glabels=glabels,
        ng=np.array([len(b) for b in c["boxes"]], np.int32), contested=np.array(contested),
        logits=rows["logits"].detach().numpy(), reg=rows["reg"].detach().numpy(), ctr=rows["ctr"].detach().numpy()[:, 0],
        anchors=anchors_rows.numpy(), labels=labels.numpy(), pos_inds=pos_inds.numpy(), reg_pos=reg_t[pos_inds].numpy(),
        ctr_pos=ctr_pos.numpy(), losses=np.array([float(lc.detach()), float(lr.detach()), float(lctr.detach())], np.float64),
        d_logits=rows["logits"].grad.numpy(), d_reg=rows["reg"].grad.numpy(), d_ctr=rows["ctr"].grad.numpy()[:, 0],
        inf_logits=inf["logits"].numpy(), inf_reg=inf["reg"].numpy(), inf_ctr=inf["ctr"].numpy()[:, 0],
        cand_row=torch.cat(cand["row"]).numpy(), cand_cls=torch.cat(cand["cls"]).numpy(),
        cand_box=torch.cat(cand["box"]).numpy(), cand_score=torch.cat(cand["score"]).numpy())
    path = os.path.join(ROOT, "tests", "golden", name + ".npz")
    np.savez_compressed(path, **out)
    print("%s: M=%d positives=%d contested=%d candidates=%d losses=%s -> %d bytes"
          % (name, M, pos_inds.numel(), contested, out["cand_row"].size, out["losses"], os.path.getsize(path)))


if __name__ == "__main__":
    ref_harness.setup()
    for name, c in CASES.items():
        make_case(name, c)

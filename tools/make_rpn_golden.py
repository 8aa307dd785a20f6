"""Writes tests/golden/rpn_*.npz: inputs and the REFERENCE's answers for the region-proposal network (cell anchors, visibility,
labels, matched boxes, encoded targets, the sampler's masks under a fixed torch.manual_seed, the two losses with their gradients,
per-level top-k candidates with decoded and clipped boxes, final proposals in train and test mode).  Runs on a CPU machine that
has the reference checkout (oracle/ref_harness.py); the fixtures hold data only.

    python tools/make_rpn_golden.py

It runs the reference's own make_anchor_generator, make_rpn_loss_evaluator (prepare_targets, the sampler, __call__ with autograd)
and make_rpn_postprocessor for train and test (BoxCoder.decode, clip_to_image, remove_small_boxes, boxlist_nms -- plain nms,
which the harness provides on the CPU -- select_over_all_levels and add_gt_proposals).

Fixture conditions, asserted here and re-asserted by tests/test_rpn_host.py from the stored inputs:
  * box coordinates are non-integer; no IoU of any (box, anchor) pair is within 1e-6 of 0.3 or of 0.7, and no anchor's best IoU
    is within 1e-6 of a second box's IoU
  * every case has an invisible anchor that would otherwise be positive, a between-thresholds anchor, a low-quality-only
    positive, one image with more and one with fewer positives than int(BATCH_SIZE_PER_IMAGE * POSITIVE_FRACTION)
  * no two objectness scores of an image lie within 1e-6 of each other; PRE_NMS_TOP_N binds on the finest level; MIN_SIZE (2 in
    the first case) removes at least one box; NMS removes at least one box per image; one candidate has dw above the clamp
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
import rpn_ref as P  # noqa: E402

BG, FG, BATCH, FRAC, TOP_N, POST_N, FPN_N, NMS = 0.3, 0.7, 16, 0.5, 50, 30, 40, 0.7

# boxes: image 0 holds more than int(BATCH * FRAC) boxes that each sit on one visible anchor, one box on an anchor that leaves
# the image and one thin box no anchor reaches FG on; image 1 holds two
CASES = {
    "rpn_64x96": dict(
        image_hw=(64, 96), seed=31, min_size=2,
        boxes=[[[4.3, 4.2, 34.6, 35.7], [20.4, 4.6, 51.3, 34.8], [36.2, 4.1, 66.7, 35.3], [52.6, 4.4, 82.2, 34.9],
                [60.3, 5.2, 91.1, 35.6], [4.7, 28.3, 35.2, 59.4], [20.2, 28.6, 50.8, 58.7], [36.5, 27.9, 67.4, 59.1],
                [52.1, 28.4, 83.3, 58.8], [62.4, 27.6, 91.7, 58.2], [8.3, 10.4, 70.6, 52.7], [40.3, 2.2, 48.6, 61.7]],
               [[12.4, 12.3, 42.7, 43.2], [50.3, 20.6, 90.6, 45.1]]]),
    "rpn_128x256": dict(
        image_hw=(128, 256), seed=32, min_size=0,
        boxes=[[[4.3, 4.2, 34.6, 35.7], [36.4, 4.6, 67.3, 34.8], [68.2, 4.1, 98.7, 35.3], [100.6, 4.4, 130.2, 34.9],
                [132.3, 5.2, 163.1, 35.6], [164.7, 4.3, 195.2, 35.4], [20.2, 44.6, 50.8, 74.7], [60.5, 43.9, 91.4, 75.1],
                [100.1, 60.4, 163.3, 122.8], [180.4, 50.6, 242.7, 113.2], [-20.3, 30.4, 100.6, 95.7], [140.3, 2.2, 150.6, 121.7]],
               [[28.4, 28.3, 58.7, 59.2], [150.3, 40.6, 214.6, 101.1]]]),
}


def make_case(name, c):
    from fcos_core.modeling.box_coder import BoxCoder
    from fcos_core.modeling.rpn.anchor_generator import make_anchor_generator
    from fcos_core.modeling.rpn.inference import make_rpn_postprocessor
    from fcos_core.modeling.rpn.loss import make_rpn_loss_evaluator
    from fcos_core.modeling.rpn.utils import permute_and_flatten
    from fcos_core.structures.bounding_box import BoxList
    from fcos_core.structures.boxlist_ops import cat_boxlist
    H, W = c["image_hw"]
    N = len(c["boxes"])
    sizes = [(-(-H // s), -(-W // s)) for s in R.STRIDES]
    off = R.row_offsets(N, sizes)
    M = off[-1]
    cfg = ref_harness.make_cfg(["MODEL.RPN.USE_FPN", True, "MODEL.RPN.ANCHOR_STRIDE", R.STRIDES, "MODEL.RPN.BG_IOU_THRESHOLD", BG,
                                "MODEL.RPN.FG_IOU_THRESHOLD", FG, "MODEL.RPN.BATCH_SIZE_PER_IMAGE", BATCH,
                                "MODEL.RPN.POSITIVE_FRACTION", FRAC, "MODEL.RPN.PRE_NMS_TOP_N_TRAIN", TOP_N,
                                "MODEL.RPN.PRE_NMS_TOP_N_TEST", TOP_N, "MODEL.RPN.POST_NMS_TOP_N_TRAIN", POST_N,
                                "MODEL.RPN.POST_NMS_TOP_N_TEST", POST_N, "MODEL.RPN.FPN_POST_NMS_TOP_N_TRAIN", FPN_N,
                                "MODEL.RPN.FPN_POST_NMS_TOP_N_TEST", FPN_N, "MODEL.RPN.NMS_THRESH", NMS,
                                "MODEL.RPN.MIN_SIZE", c["min_size"]])
    Rp = cfg.MODEL.RPN
    A = len(Rp.ASPECT_RATIOS)
    g = torch.Generator().manual_seed(c["seed"])
    rows = {"obj": torch.randn(M, A, generator=g), "reg": torch.randn(M, A * 4, generator=g) * 0.5}
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
    gen = make_anchor_generator(cfg)
    anchors = gen(images, levels(rows["obj"]))
    cells = torch.stack([b for b in gen.cell_anchors], 0)  # [L, A, 4] fp32
    targets = ref_harness.make_targets(c["boxes"], [[1] * len(b) for b in c["boxes"]], (H, W))
    coder = BoxCoder(weights=(1.0, 1.0, 1.0, 1.0))
    le = make_rpn_loss_evaluator(cfg, coder)
    cat_anchors = [cat_boxlist(a) for a in anchors]
    lab_im, reg_im = le.prepare_targets(cat_anchors, targets)
    idx_im = [le.match_targets_to_anchors(a, t, le.copied_fields).get_field("matched_idxs") for a, t in zip(cat_anchors, targets)]
    labels = to_index_order(lab_im).to(torch.int64)
    matched = torch.where(labels > 0, to_index_order(idx_im).clamp(min=0), torch.zeros_like(labels))
    matched_all = to_index_order(idx_im).clamp(min=0)
    reg_t = to_index_order(reg_im)
    vis = to_index_order([a.get_field("visibility") for a in cat_anchors]).bool()
    anchors_all = to_index_order([a.bbox for a in cat_anchors])
    torch.manual_seed(c["seed"])
    pos_im, neg_im = le.fg_bg_sampler(lab_im)
    sampled = (to_index_order(pos_im).to(torch.uint8) + 2 * to_index_order(neg_im).to(torch.uint8))
    torch.manual_seed(c["seed"])  # the sampler is the only consumer of the generator: the same draw
    lo, lr = le(anchors, levels(rows["obj"]), levels(rows["reg"]), targets)
    (lo + lr).backward()

    # the restatement's view of the same inputs: the conditions that make the reference unambiguous
    for b in c["boxes"]:
        b = np.array(b, np.float32)
        assert (b != np.round(b)).all(), (name, "integer coordinate")
    r_labels, r_matched, ious, r_vis = P.labels(N, sizes, c["boxes"], cells.numpy(), [(H, W)] * N, BG, FG, float(Rp.STRADDLE_THRESH))
    img = R.anchors_in_order(N, sizes, cells.numpy())[1]
    stats = P.check_label_conditions(ious, r_labels, r_vis, img, N, BG, FG, BATCH, FRAC)
    assert np.array_equal(r_vis, vis.numpy()), (name, "visibility disagrees")
    assert np.array_equal(r_labels, labels.numpy()) and np.array_equal(r_matched, matched.numpy()), (name, "restatement disagrees")
    assert np.array_equal(R.anchors_in_order(N, sizes, cells.numpy(), dtype=np.float32)[0], anchors_all.numpy())
    s_np = sampled.numpy()
    for n in range(N):
        own = img == n
        n_p, n_n = int((r_labels[own] == 1).sum()), int((r_labels[own] == 0).sum())
        assert int((s_np[own] == 1).sum()) == min(n_p, int(BATCH * FRAC))
        assert int((s_np[own] == 2).sum()) == min(n_n, BATCH - int((s_np[own] == 1).sum()))

    # inference: per image distinct, well separated logits; small deltas so that neighbouring anchors' boxes overlap and NMS
    # suppresses; in image 0 the best anchor of the finest level shrinks to nothing (dw = dh = -6) and the second best has
    # dw = 6, above the clamp
    n_img = M * A // N
    inf_obj = torch.empty(M, A)
    flat = inf_obj.view(-1)
    _, img_t = R.anchors_in_order(N, sizes, cells.numpy())
    for n in range(N):
        vals = torch.linspace(-4.0, 2.0, n_img)[torch.randperm(n_img, generator=g)]
        flat[torch.from_numpy(img_t == n)] = vals
    inf_reg = torch.randn(M, A * 4, generator=g) * 0.3
    lvl0 = inf_obj[:sizes[0][0] * sizes[0][1]].reshape(-1)  # image 0, level 0
    best = torch.argsort(lvl0, descending=True)[:2]
    inf_reg.view(-1, 4)[best[0], 2:] = -6.0
    inf_reg.view(-1, 4)[best[1], 2] = 6.0
    inf = {"obj": inf_obj, "reg": inf_reg}
    score_of = []  # per image {score: global anchor index}
    topk_idx, topk_box, topk_score = [], [], []
    with torch.no_grad():
        probs = [permute_and_flatten(o, N, A, 1, h, w).view(N, -1).sigmoid() for o, (h, w) in zip(levels(inf["obj"]), sizes)]
        for n in range(N):
            d = {}
            for l, (h, w) in enumerate(sizes):
                for j, s_ in enumerate(probs[l][n].tolist()):
                    d[s_] = (off[l] + n * h * w) * A + j
            assert len(d) == n_img
            s = np.sort(np.array(list(d), np.float64))
            assert (s[1:] - s[:-1] > 1e-6).all(), (name, "two objectness scores within 1e-6")
            score_of.append(d)
        removed_small = 0
        for l, (h, w) in enumerate(sizes):
            k = min(TOP_N, h * w * A)
            if l == 0:
                assert h * w * A > TOP_N, (name, "PRE_NMS_TOP_N does not bind on level 0")
            val, idx = probs[l].topk(k, dim=1, sorted=True)
            regs = permute_and_flatten(levels(inf["reg"])[l], N, A, 4, h, w)
            bidx = torch.arange(N)[:, None]
            anc = torch.cat([a[l].bbox for a in anchors], 0).reshape(N, -1, 4)[bidx, idx]
            dec = coder.decode(regs[bidx, idx].view(-1, 4), anc.view(-1, 4)).view(N, -1, 4)
            clipped = []
            for n in range(N):
                bl = BoxList(dec[n].clone(), (W, H), mode="xyxy").clip_to_image(remove_empty=False)
                clipped.append(bl.bbox)
                ws, hs = bl.bbox[:, 2] - bl.bbox[:, 0] + 1, bl.bbox[:, 3] - bl.bbox[:, 1] + 1
                removed_small += int(((ws < c["min_size"]) | (hs < c["min_size"])).sum())
            topk_idx.append(idx)
            topk_score.append(val)
            topk_box.append(torch.stack(clipped, 0))
        if c["min_size"] > 0:
            assert removed_small > 0, (name, "MIN_SIZE removes nothing")
        assert float(inf_reg.view(-1, 4)[:, 2].max()) > P.CLIP
        out_modes = {}
        for mode, is_train in (("train", True), ("test", False)):
            pp = make_rpn_postprocessor(cfg, coder, is_train=is_train)
            pp.train(is_train)
            single = [pp.forward_for_single_feature_map([a[l] for a in anchors], levels(inf["obj"])[l], levels(inf["reg"])[l])
                      for l in range(len(sizes))]
            if is_train:
                for n in range(N):  # NMS removes at least one box per image
                    kept = sum(len(single[l][n]) for l in range(len(sizes)))
                    alive = sum(int(((tb[n][:, 2] - tb[n][:, 0] + 1 >= c["min_size"])
                                     & (tb[n][:, 3] - tb[n][:, 1] + 1 >= c["min_size"])).sum()) for tb in topk_box)
                    assert kept < alive, (name, "NMS removes nothing in image %d" % n, kept, alive)
            props = pp(anchors, levels(inf["obj"]), levels(inf["reg"]), targets if is_train else None)
            idx_out = []
            for n, p in enumerate(props):
                sc = p.get_field("objectness").tolist()
                n_gt = len(c["boxes"][n]) if is_train else 0
                own = [score_of[n][s_] for s_ in sc[:len(sc) - n_gt]] + [-1] * n_gt
                idx_out.append(torch.tensor(own, dtype=torch.int64))
            out_modes[mode] = dict(count=np.array([len(p) for p in props]), idx=torch.cat(idx_out).numpy(),
                                   box=torch.cat([p.bbox for p in props]).numpy(),
                                   score=torch.cat([p.get_field("objectness") for p in props]).numpy())
    G = max(len(b) for b in c["boxes"])
    boxes = np.zeros((N, G, 4), np.float32)
    for n, b in enumerate(c["boxes"]):
        boxes[n, :len(b)] = b
    out = dict(
        image_hw_one=np.array([H, W]), sizes=np.array(sizes), num_anchors=np.array(A), bg=np.array(BG), fg=np.array(FG),
        straddle_thresh=np.array(float(Rp.STRADDLE_THRESH)), batch_size_per_image=np.array(BATCH), positive_fraction=np.array(FRAC),
        pre_nms_top_n=np.array(TOP_N), post_nms_top_n=np.array(POST_N), fpn_post_nms_top_n=np.array(FPN_N), nms_thresh=np.array(NMS),
        min_size=np.array(c["min_size"]), anchor_sizes=np.array(Rp.ANCHOR_SIZES, np.float32),
        aspect_ratios=np.array(Rp.ASPECT_RATIOS, np.float64), cells=cells.numpy(), boxes=boxes,
        ng=np.array([len(b) for b in c["boxes"]], np.int32), stats=np.array(stats[:3]), n_pos=np.array(stats[3]),
        obj=rows["obj"].detach().numpy(), reg=rows["reg"].detach().numpy(), visibility=vis.numpy(),
        labels=labels.numpy().astype(np.int32), matched=matched.numpy().astype(np.int32),
        matched_all=matched_all.numpy().astype(np.int32), reg_targets=reg_t.numpy(), sampled=s_np,
        losses=np.array([float(lo.detach()), float(lr.detach())], np.float64),
        d_obj=rows["obj"].grad.numpy(), d_reg=rows["reg"].grad.numpy(),
        inf_obj=inf["obj"].numpy(), inf_reg=inf["reg"].numpy(),
        topk_idx=torch.cat(topk_idx, 1).numpy(), topk_box=torch.cat(topk_box, 1).numpy(), topk_score=torch.cat(topk_score, 1).numpy(),
        topk_k=np.array([t.shape[1] for t in topk_idx]))
    for mode, d in out_modes.items():
        for k, v in d.items():
            out["%s_%s" % (mode, k)] = v
    path = os.path.join(ROOT, "tests", "golden", name + ".npz")
    np.savez_compressed(path, **out)
    print("%s: anchors=%d (hidden, between, low-quality)=%s positives per image=%s losses=%s proposals train=%s test=%s -> %d bytes"
          % (name, M * A, stats[:3], stats[3], out["losses"], out["train_count"], out["test_count"], os.path.getsize(path)))


if __name__ == "__main__":
    ref_harness.setup()
    for name, c in CASES.items():
        make_case(name, c)

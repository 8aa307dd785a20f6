"""fp64 / torch-CPU restatement of the ATSS head's definitions (csrc/atss.hip, modeling/atss.py): anchors, the assignment
with its tie rules (stable sort), the box coder, centerness targets, the GIoU loss, the three losses and the candidate
selection of the post-processor.  Independent of scan_amd: only torch (numpy to load the fixtures).  Distances are formed in fp32 operation by operation,
as the definition says (they only order anchors); everything else is fp64."""
import math
import os

import numpy as np
import torch

STRIDES = (8, 16, 32, 64, 128)
SIZES = (64, 128, 256, 512, 1024)
CLIP = math.log(1000. / 16)


def row_offsets(n_images, sizes):
    off = [0]
    for h, w in sizes:
        off.append(off[-1] + n_images * h * w)
    return off


def level_anchors(sizes, strides=STRIDES, anchor_sizes=SIZES, dtype=torch.float64):
    """per level [h * w, 4] xyxy, x fastest: centre (x * s + (s - 1) / 2, y * s + (s - 1) / 2), corners -/+ (a - 1) / 2"""
    out = []
    for (h, w), s, a in zip(sizes, strides, anchor_sizes):
        ys, xs = torch.meshgrid(torch.arange(h, dtype=dtype), torch.arange(w, dtype=dtype), indexing="ij")
        cx, cy = xs.reshape(-1) * s + (s - 1) / 2, ys.reshape(-1) * s + (s - 1) / 2
        half = (a - 1) / 2
        out.append(torch.stack([cx - half, cy - half, cx + half, cy + half], 1))
    return out


def row_anchors(n_images, sizes, strides=STRIDES, anchor_sizes=SIZES, dtype=torch.float64):
    return torch.cat([a.repeat(n_images, 1) for a in level_anchors(sizes, strides, anchor_sizes, dtype)], 0)


def iou_plus1(a, b):
    """boxlist_iou with the +1 widths: a [A, 4], b [G, 4] -> [A, G]"""
    area_a = (a[:, 2] - a[:, 0] + 1) * (a[:, 3] - a[:, 1] + 1)
    area_b = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    w = (torch.min(a[:, None, 2], b[None, :, 2]) - torch.max(a[:, None, 0], b[None, :, 0]) + 1).clamp(min=0)
    h = (torch.min(a[:, None, 3], b[None, :, 3]) - torch.max(a[:, None, 1], b[None, :, 1]) + 1).clamp(min=0)
    inter = w * h
    return inter / (area_a[:, None] + area_b[None] - inter)


def assign(n_images, sizes, targets, strides=STRIDES, anchor_sizes=SIZES, topk=9):
    """targets: per image (boxes [G, 4], labels [G]).  Returns labels [M] int64, matched [M] int64 (0 where background) in
    pyramid row order and, per image, the details the fixture conditions are stated on:
      dist_gap [G, L]   (k+1)-th minus k-th smallest distance of each level (inf where the level has <= k anchors)
      cand_iou [K, G], thr [G], pos [K, G] (positive candidates), cand_row [K, G]"""
    off = row_offsets(n_images, sizes)
    M = off[-1]
    labels = torch.zeros(M, dtype=torch.int64)
    matched = torch.zeros(M, dtype=torch.int64)
    anc64 = level_anchors(sizes, strides, anchor_sizes)
    anc32 = level_anchors(sizes, strides, anchor_sizes, torch.float32)
    details = []
    for n, (boxes, lab) in enumerate(targets):
        G = int(boxes.shape[0])
        if G == 0:
            details.append(None)
            continue
        b32 = boxes.to(torch.float32)
        b64 = b32.double()
        gcx32, gcy32 = (b32[:, 2] + b32[:, 0]) / 2, (b32[:, 3] + b32[:, 1]) / 2
        rows, ious, inside, gaps = [], [], [], []
        for l, (a64, a32) in enumerate(zip(anc64, anc32)):
            hw = a64.shape[0]
            dx = (a32[:, 2] + a32[:, 0])[:, None] / 2 - gcx32[None]
            dy = (a32[:, 3] + a32[:, 1])[:, None] / 2 - gcy32[None]
            dist = (dx * dx + dy * dy).sqrt()  # fp32, every operation rounded on its own
            sd, order = torch.sort(dist, dim=0, stable=True)  # equal distances: smaller row first
            k = min(topk, hw)
            gaps.append(sd[k] - sd[k - 1] if hw > k else torch.full((G,), float("inf")))
            idx = order[:k]
            rows.append(off[l] + n * hw + idx)
            ious.append(torch.gather(iou_plus1(a64, b64), 0, idx))
            cx, cy = (a64[:, 2] + a64[:, 0]) / 2, (a64[:, 3] + a64[:, 1]) / 2
            ltrb = torch.stack([cx[idx] - b64[None, :, 0], cy[idx] - b64[None, :, 1], b64[None, :, 2] - cx[idx],
                                b64[None, :, 3] - cy[idx]], 0)
            inside.append(ltrb.min(0)[0] > 0.01)
        rows, ious, inside = torch.cat(rows, 0), torch.cat(ious, 0), torch.cat(inside, 0)
        thr = ious.mean(0) + ious.std(0)  # unbiased
        pos = (ious >= thr[None]) & inside
        best = torch.full((M,), -1.0, dtype=torch.float64)
        for g in range(G):  # ascending g with a strict >: equal IoUs keep the smaller box index
            r = rows[pos[:, g], g]
            better = ious[pos[:, g], g] > best[r]
            best[r[better]] = ious[pos[:, g], g][better]
            labels[r[better]] = int(lab[g])
            matched[r[better]] = g
        details.append(dict(dist_gap=torch.stack(gaps, 1), cand_iou=ious, thr=thr, pos=pos, cand_row=rows))
    return labels, matched, details


def encode(gt, anchors):
    ew, eh = anchors[:, 2] - anchors[:, 0] + 1, anchors[:, 3] - anchors[:, 1] + 1
    ecx, ecy = (anchors[:, 2] + anchors[:, 0]) / 2, (anchors[:, 3] + anchors[:, 1]) / 2
    gw, gh = gt[:, 2] - gt[:, 0] + 1, gt[:, 3] - gt[:, 1] + 1
    gcx, gcy = (gt[:, 2] + gt[:, 0]) / 2, (gt[:, 3] + gt[:, 1]) / 2
    return torch.stack([10 * (gcx - ecx) / ew, 10 * (gcy - ecy) / eh, 5 * torch.log(gw / ew), 5 * torch.log(gh / eh)], 1)


def decode(deltas, anchors):
    w, h = anchors[:, 2] - anchors[:, 0] + 1, anchors[:, 3] - anchors[:, 1] + 1
    cx, cy = (anchors[:, 2] + anchors[:, 0]) / 2, (anchors[:, 3] + anchors[:, 1]) / 2
    dw, dh = torch.clamp(deltas[:, 2] / 5, max=CLIP), torch.clamp(deltas[:, 3] / 5, max=CLIP)
    pcx, pcy = deltas[:, 0] / 10 * w + cx, deltas[:, 1] / 10 * h + cy
    pw, ph = torch.exp(dw) * w, torch.exp(dh) * h
    return torch.stack([pcx - 0.5 * (pw - 1), pcy - 0.5 * (ph - 1), pcx + 0.5 * (pw - 1), pcy + 0.5 * (ph - 1)], 1)


def centerness(reg, anchors):
    g = decode(reg, anchors)
    cx, cy = (anchors[:, 2] + anchors[:, 0]) / 2, (anchors[:, 3] + anchors[:, 1]) / 2
    l, t, r, b = cx - g[:, 0], cy - g[:, 1], g[:, 2] - cx, g[:, 3] - cy
    return torch.sqrt((torch.min(l, r) / torch.max(l, r)) * (torch.min(t, b) / torch.max(t, b)))


def giou_losses(pred, target, anchors):
    """1 - GIoU per row (reference loss.py:64-99); works in the dtype of its inputs, differentiable in pred"""
    p = decode(pred, anchors)
    px1, py1 = p[:, 0], p[:, 1]
    px2, py2 = torch.max(px1, p[:, 2]), torch.max(py1, p[:, 3])
    pa = (px2 - px1) * (py2 - py1)
    t = decode(target, anchors)
    ta = (t[:, 2] - t[:, 0]) * (t[:, 3] - t[:, 1])
    ix1, iy1 = torch.max(px1, t[:, 0]), torch.max(py1, t[:, 1])
    ix2, iy2 = torch.min(px2, t[:, 2]), torch.min(py2, t[:, 3])
    mask = (iy2 > iy1) & (ix2 > ix1)
    inter = torch.where(mask, (ix2 - ix1) * (iy2 - iy1), torch.zeros_like(pa))
    ex1, ey1 = torch.min(px1, t[:, 0]), torch.min(py1, t[:, 1])
    ex2, ey2 = torch.max(px2, t[:, 2]), torch.max(py2, t[:, 3])
    enc = (ex2 - ex1) * (ey2 - ey1) + 1e-7
    union = pa + ta - inter + 1e-7
    return 1 - (inter / union - (enc - union) / enc)


def giou_loss(pred, target, anchors, weight):
    """(sum(w * (1 - GIoU)), sum(w))"""
    return (giou_losses(pred, target, anchors) * weight).sum(), weight.sum()


def focal_sum(logits, labels, gamma, alpha):
    """sigmoid focal loss summed (layers/sigmoid_focal_loss.py: sigmoid_focal_loss_cpu); labels [M] in 0..C"""
    C = logits.shape[1]
    cls = torch.arange(1, C + 1, dtype=labels.dtype)[None]
    t = labels[:, None]
    p = torch.sigmoid(logits)
    term1 = (1 - p) ** gamma * torch.log(p)
    term2 = p ** gamma * torch.log(1 - p)
    return (-(t == cls).to(logits.dtype) * term1 * alpha - ((t != cls) & (t >= 0)).to(logits.dtype) * term2 * (1 - alpha)).sum()


def losses(logits, reg, ctr, labels, reg_pos, ctr_pos, pos_inds, anchors, gamma, alpha, reg_loss_weight):
    """the three ATSS losses (reference loss.py:374-403, one rank); all inputs fp64"""
    n_pos = int(pos_inds.numel())
    cls_loss = focal_sum(logits, labels, gamma, alpha) / max(n_pos, 1)
    if n_pos == 0:
        return cls_loss, reg[pos_inds].sum() * reg_loss_weight, ctr[pos_inds].sum()
    num, den = giou_loss(reg[pos_inds], reg_pos, anchors[pos_inds], ctr_pos)
    bce = torch.nn.functional.binary_cross_entropy_with_logits(ctr[pos_inds], ctr_pos, reduction="sum")
    return cls_loss, num / den * reg_loss_weight, bce / max(n_pos, 1)


def candidates(n_images, sizes, logits, reg, ctr, image_sizes, anchors, pre_nms_thresh=0.05):
    """pre-NMS candidates of the post-processor (reference inference.py:35-82 with pre_nms_top_n not binding): every (row, class)
    with sigmoid(logit) > pre_nms_thresh; returns rows [K], classes [K] (1-based), boxes [K, 4] clipped to the image, scores [K]
    = sqrt(probability x centerness), in (row, class) order"""
    off = row_offsets(n_images, sizes)
    prob = torch.sigmoid(logits)
    rc = torch.nonzero(prob > pre_nms_thresh)
    rows, cls = rc[:, 0], rc[:, 1]
    score = torch.sqrt(prob[rows, cls] * torch.sigmoid(ctr)[rows])
    boxes = decode(reg[rows], anchors[rows])
    img = torch.zeros_like(rows)
    for l, (h, w) in enumerate(sizes):
        m = (rows >= off[l]) & (rows < off[l + 1])
        img[m] = (rows[m] - off[l]) // (h * w)
    lim = torch.tensor([[w - 1, h - 1, w - 1, h - 1] for h, w in image_sizes], dtype=boxes.dtype)[img]
    boxes = torch.min(boxes.clamp(min=0), lim)
    return rows, cls + 1, boxes, score


# ----------------------------------------------------------------------------- shared test inputs
CASES = ("atss_64x96", "atss_128x256")


def load_case(gold_dir, name):
    z = np.load(os.path.join(gold_dir, name + ".npz"))
    f = {k: z[k] for k in z.files}
    f["sizes"] = [tuple(int(v) for v in s) for s in f["sizes"]]
    f["N"] = int(f["boxes"].shape[0])
    f["targets"] = [(torch.from_numpy(f["boxes"][n, :g]), torch.from_numpy(f["glabels"][n, :g])) for n, g in enumerate(f["ng"])]
    return f


def tie_inputs():
    """integer-coordinate boxes at 128x256 whose centres sit on cell corners / edges: equidistant anchors at the topk boundary"""
    sizes = [(16, 32), (8, 16), (4, 8), (2, 4), (1, 2)]
    boxes = [torch.tensor([[32., 16., 96., 80.], [100., 40., 180., 104.], [8., 8., 24., 56.]]),
             torch.tensor([[120., 56., 200., 120.], [16., 64., 48., 96.]])]
    labels = [torch.tensor([1, 2, 1]), torch.tensor([2, 1])]
    return sizes, list(zip(boxes, labels))


SIZES_128x256 = [(16, 32), (8, 16), (4, 8), (2, 4), (1, 2)]


def giou_inputs(P, kind):
    """pred, target [P, 4] deltas, rows [P] of the 128x256 pyramid with two images, weight [P] for the GIoU tests"""
    g = torch.Generator().manual_seed(1000 * P + len(kind))
    M = 2 * sum(h * w for h, w in SIZES_128x256)
    rows = torch.randint(0, M, (P,), generator=g)
    target = torch.randn(P, 4, generator=g) * torch.tensor([1.5, 1.5, 2.0, 2.0])
    pred = target + torch.randn(P, 4, generator=g) * torch.tensor([1.0, 1.0, 1.5, 1.5])
    if kind == "clamp":  # dw, dh past log(1000 / 16) = 4.135 -> deltas past 20.7 (every second row)
        pred[::2, 2:] = 21.0 + torch.rand(pred[::2, 2:].shape, generator=g) * 4
    elif kind == "disjoint":  # centres three to five anchor widths apart: zero intersection
        pred[:, :2] = target[:, :2] + 40.0 * torch.where(torch.rand(P, 2, generator=g) > 0.5, 1.0, -1.0)
        pred[:, 2:], target[:, 2:] = pred[:, 2:].clamp(max=2.0), target[:, 2:].clamp(max=2.0)
    elif kind == "flipped":  # exp(dw) * w < 1: x2 < x1 before the max (w >= 64: dw < -4.16 -> delta < -20.8)
        pred[::2, 2] = -40.0 - torch.rand(pred[::2, 2].shape, generator=g) * 5
        pred[1::2, 3] = -40.0 - torch.rand(pred[1::2, 3].shape, generator=g) * 5
    else:
        assert kind == "generic"
    return pred, target, rows, 0.05 + torch.rand(P, generator=g)

"""fp64 / integer numpy restatement of the region-proposal network's device work: visibility and the 0 / 1 / -1 labels, the
sampler's key mix and selection rule, BoxCoder.encode / decode with weights 1, the sampled BCE + smooth-L1 loss and the proposal
decode -- written from the reference's definitions (rpn/anchor_generator.py, rpn/loss.py, rpn/inference.py, modeling/matcher.py,
modeling/box_coder.py, modeling/balanced_positive_negative_sampler.py) and from the rule stated in include/scan_hip.h, not from
the project's kernels.  Anchors, IoU and the matcher are tests/retinanet_ref.py's (the RPN uses the same ones with every box
label 1)."""
import math
import os

import numpy as np
import torch

import retinanet_ref as R

STRIDES = R.STRIDES
SIZES = R.SIZES
RATIOS = (0.5, 1.0, 2.0)
CASES = ("rpn_64x96", "rpn_128x256")
CLIP = math.log(1000.0 / 16)


def cell_anchors(ratios=RATIOS, sizes=SIZES):
    """[L][A][4] fp64: one size per level, ratio-major"""
    return R.cell_anchors(STRIDES, sizes, ratios, 2.0, 1)


def visibility(n_images, sizes, cells, image_hw, thr):
    """bool [M * A]: the anchor lies inside its image widened by thr on every side; thr < 0: everything is visible"""
    a, img = R.anchors_in_order(n_images, sizes, cells, dtype=np.float32)
    if thr < 0:
        return np.ones(a.shape[0], bool)
    hw = np.asarray(image_hw, dtype=np.float32).reshape(-1, 2)[img]
    t = np.float32(thr)
    return (a[:, 0] >= -t) & (a[:, 1] >= -t) & (a[:, 2] < hw[:, 1] + t) & (a[:, 3] < hw[:, 0] + t)


def labels(n_images, sizes, boxes_per_image, cells, image_hw, bg=0.3, fg=0.7, thr=0.0):
    """labels [M * A] in {1, 0, -1}, matched [M * A], per image the fp32 IoU matrix [G, n], visibility [M * A].  The matcher with
    every box label 1 (all anchors take part in the per-box maxima), then -1 wherever the anchor is not visible."""
    tg = [(np.asarray(b, np.float32).reshape(-1, 4), np.ones(len(b), np.int64)) for b in boxes_per_image]
    lab, matched, ious = R.match(n_images, sizes, tg, cells, bg=bg, fg=fg)
    vis = visibility(n_images, sizes, cells, image_hw, thr)
    lab = np.where(vis, lab, -1)
    return lab, np.where(lab > 0, matched, 0), ious, vis


# ----------------------------------------------------------------------------- sampler
def fmix32(x):
    x = np.asarray(x, dtype=np.uint64) & 0xffffffff
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xffffffff
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xffffffff
    x ^= x >> 16
    return x


def sample_key(seed, image, index):
    """the 32-bit key of (seed, image, anchor index): fmix32(fmix32(seed ^ (0x9E3779B9 (image + 1))) ^ index), mod 2^32"""
    first = fmix32(np.uint64(seed & 0xffffffff) ^ np.uint64((0x9E3779B9 * (int(image) + 1)) & 0xffffffff))
    return fmix32(first ^ (np.asarray(index, dtype=np.uint64) & 0xffffffff))


def sample(lab, img, n_images, batch, frac, seed=0, keys=None):
    """sampled uint8 [M * A] (1 / 2 / 0) and counts [N, 2]: per image the min(#positives, int(batch frac)) positives and then
    the min(#negatives, batch - num_pos) negatives with the smallest (key, anchor index) pairs"""
    out = np.zeros(lab.shape[0], np.uint8)
    counts = np.zeros((n_images, 2), np.int32)
    for n in range(n_images):
        own = np.nonzero(img == n)[0]
        k = sample_key(seed, n, own) if keys is None else np.asarray(keys, dtype=np.uint64)[own] & 0xffffffff
        pos, neg = lab[own] >= 1, lab[own] == 0
        num_pos = min(int(pos.sum()), int(batch * frac))
        num_neg = min(int(neg.sum()), batch - num_pos)
        for mask, num, mark in ((pos, num_pos, 1), (neg, num_neg, 2)):
            cand = own[mask]
            order = np.lexsort((cand, k[mask]))  # by key, then by anchor index
            out[cand[order[:num]]] = mark
        counts[n] = num_pos, num_neg
    return out, counts


# ----------------------------------------------------------------------------- box coder, weights (1, 1, 1, 1)
def encode(gt, anchors):
    ew, eh = anchors[:, 2] - anchors[:, 0] + 1, anchors[:, 3] - anchors[:, 1] + 1
    ecx, ecy = anchors[:, 0] + 0.5 * ew, anchors[:, 1] + 0.5 * eh
    gw, gh = gt[:, 2] - gt[:, 0] + 1, gt[:, 3] - gt[:, 1] + 1
    gcx, gcy = gt[:, 0] + 0.5 * gw, gt[:, 1] + 0.5 * gh
    return np.stack([(gcx - ecx) / ew, (gcy - ecy) / eh, np.log(gw / ew), np.log(gh / eh)], 1)


def targets64(n_images, sizes, boxes_per_image, cells, matched):
    """[M * A, 4] fp64: encode(matched box, anchor) of EVERY anchor (the reference encodes all of them, clamped match 0)"""
    anchors, img = R.anchors_in_order(n_images, sizes, cells)
    G = max(1, max(len(b) for b in boxes_per_image))
    boxes = np.zeros((n_images, G, 4))
    boxes[:, :, 2:] = 1.0  # padding boxes: never selected where a label is positive
    for n, b in enumerate(boxes_per_image):
        boxes[n, :len(b)] = np.asarray(b, np.float32).reshape(-1, 4)
    return encode(boxes[img, matched], anchors)


def decode(deltas, anchors, image_hw_of, min_size):
    """fp64: deltas / anchors [n, 4], image_hw_of [n, 2] -> clipped boxes [n, 4], keep [n]"""
    w, h = anchors[:, 2] - anchors[:, 0] + 1, anchors[:, 3] - anchors[:, 1] + 1
    cx, cy = anchors[:, 0] + 0.5 * w, anchors[:, 1] + 0.5 * h
    dw, dh = np.minimum(deltas[:, 2], CLIP), np.minimum(deltas[:, 3], CLIP)
    pcx, pcy = deltas[:, 0] * w + cx, deltas[:, 1] * h + cy
    pw, ph = np.exp(dw) * w, np.exp(dh) * h
    b = np.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw - 1, pcy + 0.5 * ph - 1], 1)
    hi = np.stack([image_hw_of[:, 1] - 1, image_hw_of[:, 0] - 1] * 2, 1).astype(np.float64)
    b = np.minimum(np.maximum(b, 0.0), hi)
    keep = (b[:, 2] - b[:, 0] + 1 >= min_size) & (b[:, 3] - b[:, 1] + 1 >= min_size)
    return b, keep


def topk_per_level(obj, n_images, sizes, A, k_max):
    """obj [M, A] logits -> per level [N, k] anchor indices within the image's level, by falling score (sigmoid is monotone;
    the fixtures' scores are distinct)"""
    off = R.row_offsets(n_images, sizes)
    out = []
    for l, (h, w) in enumerate(sizes):
        flat = np.asarray(obj[off[l]:off[l + 1]], np.float64).reshape(n_images, h * w * A)
        out.append(np.argsort(-flat, axis=1, kind="stable")[:, :min(k_max, h * w * A)])
    return out


def candidate_geometry(topk, n_images, sizes, A, cells, reg, image_hw):
    """for the candidates of topk_per_level side by side: global anchor index [N, K], deltas [N, K, 4], anchors [N, K, 4] fp64,
    image sizes [N, K, 2]"""
    off = R.row_offsets(n_images, sizes)
    anchors, _ = R.anchors_in_order(n_images, sizes, cells)
    reg = np.asarray(reg, np.float64).reshape(-1, 4)
    glob = np.concatenate([(off[l] + np.arange(n_images)[:, None] * h * w) * A + topk[l] for l, (h, w) in enumerate(sizes)], 1)
    hw = np.broadcast_to(np.asarray(image_hw, np.float64).reshape(n_images, 1, 2), glob.shape + (2,))
    return glob, reg[glob], anchors[glob], hw


# ----------------------------------------------------------------------------- loss (torch fp64, autograd)
def loss_sums(obj, reg, sampled, targets, beta):
    """obj [M * A], reg [M * A, 4] fp64 torch, sampled uint8 numpy, targets [M * A, 4] fp64 numpy ->
    (sum of BCE-with-logits over the sampled anchors, sum of smooth-L1 over the sampled positives)"""
    s = torch.from_numpy(sampled.astype(np.int64))
    y = (s == 1).double()
    bce = (obj.clamp(min=0) - obj * y + torch.log1p(torch.exp(-obj.abs()))) * (s != 0)
    n = (reg - torch.from_numpy(targets)).abs()
    sl1 = torch.where(n < beta, 0.5 * n * n / beta, n - 0.5 * beta) * (s == 1)[:, None]
    return bce.sum(), sl1.sum()


def greedy_nms(boxes, scores, thr):
    """indices kept by greedy NMS in falling score order: a box goes when its +1 IoU with a kept box is >= thr (the reference's
    CPU rule, csrc/cpu/nms_cpu.cpp)"""
    boxes = np.asarray(boxes, np.float64)
    area = (boxes[:, 2] - boxes[:, 0] + 1) * (boxes[:, 3] - boxes[:, 1] + 1)
    kept = []
    for i in np.argsort(-np.asarray(scores, np.float64), kind="stable"):
        ok = True
        for j in kept:
            w = max(min(boxes[i, 2], boxes[j, 2]) - max(boxes[i, 0], boxes[j, 0]) + 1, 0.0)
            h = max(min(boxes[i, 3], boxes[j, 3]) - max(boxes[i, 1], boxes[j, 1]) + 1, 0.0)
            if w * h / (area[i] + area[j] - w * h) >= thr:
                ok = False
                break
        if ok:
            kept.append(int(i))
    return kept


def load_case(gold_dir, name):
    z = np.load(os.path.join(gold_dir, name + ".npz"))
    f = {k: z[k] for k in z.files}
    f["sizes"] = [tuple(int(v) for v in s) for s in f["sizes"]]
    f["N"] = int(f["boxes"].shape[0])
    f["box_lists"] = [f["boxes"][n, :g] for n, g in enumerate(f["ng"])]
    f["targets"] = [(torch.from_numpy(b.copy()), torch.ones(len(b), dtype=torch.int64)) for b in f["box_lists"]]
    f["image_hw"] = [tuple(int(v) for v in f["image_hw_one"])] * f["N"]
    return f


def check_label_conditions(ious, lab, vis, img, n_images, bg, fg, batch, frac):
    """the fixture conditions on the labels (tools/make_rpn_golden.py): no IoU of any (box, anchor) pair within 1e-6 of bg or of
    fg, no anchor's best IoU within 1e-6 of a second box's IoU; an invisible anchor that would otherwise be positive, a between-thresholds anchor, a low-quality-only
    positive; one image with more and one with fewer positives than int(batch frac)"""
    hidden = between = lowq = 0
    n_pos = []
    for n in range(n_images):
        q = ious[n].astype(np.float64)
        own = img == n
        top = np.sort(q, 0)[::-1]
        assert ((np.abs(q - bg) > 1e-6) & (np.abs(q - fg) > 1e-6)).all(), "an IoU within 1e-6 of a threshold"
        if q.shape[0] > 1:
            assert ((top[0] - top[1] > 1e-6) | (top[0] == 0)).all(), "two boxes within 1e-6 of an anchor's maximum"
        low = (q == q.max(1)[:, None]).any(0)
        would = (top[0] >= fg) | low
        hidden += int((would & ~vis[own]).sum())
        between += int(((top[0] >= bg) & (top[0] < fg) & ~low & vis[own]).sum())
        lowq += int(((top[0] < fg) & low & vis[own] & (lab[own] == 1)).sum())
        n_pos.append(int((lab[own] == 1).sum()))
    cap = int(batch * frac)
    assert hidden > 0 and between > 0 and lowq > 0, (hidden, between, lowq)
    assert max(n_pos) > cap and 0 < min(n_pos) < cap, (n_pos, cap)
    return hidden, between, lowq, n_pos

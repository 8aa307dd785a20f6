"""fp64 / integer numpy restatement of the Fast R-CNN box head's device work: the proposals' matcher (no low-quality rule) and its
0 / -1 / class labels, BoxCoder.encode / decode with weights, the sampler's rule on the padded layout, the gather order, the
cross-entropy + class-specific smooth-L1 loss with its gradients, the test-time softmax + decode and the post-processor --
written from the reference's definitions (roi_heads/box_head/loss.py, inference.py, modeling/matcher.py, modeling/box_coder.py,
modeling/balanced_positive_negative_sampler.py) and from the rules stated in include/scan_hip.h, not from the project's kernels.
The IoU is tests/retinanet_ref.py's, the sampler's key and selection rule and the greedy NMS are tests/rpn_ref.py's."""
import math
import os

import numpy as np
import torch

import retinanet_ref as R
import rpn_ref as P

CASES = ("roi_box_64x96", "roi_box_band_64x96", "roi_box_c81_128x256")
CLIP = math.log(1000.0 / 16)
WEIGHTS = (10.0, 10.0, 5.0, 5.0)


# ----------------------------------------------------------------------------- padded layout
def pad(per_image, width=4, dtype=np.float32, fill=0):
    """list of [k_n, width] (or [k_n]) arrays -> ([N, max k, width], counts int32 [N]); at least one column"""
    K = max(1, max(len(a) for a in per_image))
    shape = (len(per_image), K) + ((width,) if width else ())
    out = np.full(shape, fill, dtype)
    for n, a in enumerate(per_image):
        if len(a):
            out[n, :len(a)] = np.asarray(a, dtype).reshape((len(a),) + shape[2:])
    return out, np.array([len(a) for a in per_image], np.int32)


# ----------------------------------------------------------------------------- matcher
def match(props, n_props, boxes, glab, ng, bg, fg):
    """props [N, P, 4] fp32, boxes [N, G, 4] fp32, glab [N, G] -> labels [N * P] (0 / -1 / class; -1 on padding), matched
    [N * P] (0 where label <= 0), per image the fp32 IoU matrix [ng, np].  Equal IoUs: the smaller box index (argmax's first)."""
    N, Pn = props.shape[:2]
    labels = np.full((N, Pn), -1, np.int64)
    matched = np.zeros((N, Pn), np.int64)
    ious = []
    for n in range(N):
        k, g = int(n_props[n]), int(ng[n])
        if g == 0 or k == 0:
            ious.append(np.zeros((g, k), np.float32))
            labels[n, :k] = 0
            continue
        q = R.iou_plus1(np.asarray(boxes[n, :g], np.float32), np.asarray(props[n, :k], np.float32))
        ious.append(q)
        best, arg = q.max(0), q.argmax(0)
        lb = np.where(best < np.float32(bg), 0, np.where(best < np.float32(fg), -1, np.asarray(glab[n])[arg]))
        labels[n, :k] = lb
        matched[n, :k] = np.where(lb > 0, arg, 0)
    return labels.reshape(-1), matched.reshape(-1), ious


# ----------------------------------------------------------------------------- box coder
def encode(gt, ex, weights=WEIGHTS):
    gt, ex = np.asarray(gt, np.float64), np.asarray(ex, np.float64)
    ew, eh = ex[:, 2] - ex[:, 0] + 1, ex[:, 3] - ex[:, 1] + 1
    ecx, ecy = ex[:, 0] + 0.5 * ew, ex[:, 1] + 0.5 * eh
    gw, gh = gt[:, 2] - gt[:, 0] + 1, gt[:, 3] - gt[:, 1] + 1
    gcx, gcy = gt[:, 0] + 0.5 * gw, gt[:, 1] + 0.5 * gh
    wx, wy, ww, wh = weights
    return np.stack([wx * (gcx - ecx) / ew, wy * (gcy - ecy) / eh, ww * np.log(gw / ew), wh * np.log(gh / eh)], 1)


def decode(deltas, rois, image_hw_of, weights=WEIGHTS):
    """fp64: deltas [R, K, 4], rois [R, 4], image_hw_of [R, 2] -> boxes [R, K, 4] clipped to the image, and the unclamped dw"""
    deltas, rois = np.asarray(deltas, np.float64), np.asarray(rois, np.float64)
    w, h = (rois[:, 2] - rois[:, 0] + 1)[:, None], (rois[:, 3] - rois[:, 1] + 1)[:, None]
    cx, cy = rois[:, 0:1] + 0.5 * w, rois[:, 1:2] + 0.5 * h
    wx, wy, ww, wh = weights
    dx, dy = deltas[..., 0] / wx, deltas[..., 1] / wy
    dw, dh = np.minimum(deltas[..., 2] / ww, CLIP), np.minimum(deltas[..., 3] / wh, CLIP)
    pcx, pcy = dx * w + cx, dy * h + cy
    pw, ph = np.exp(dw) * w, np.exp(dh) * h
    raw = np.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw - 1, pcy + 0.5 * ph - 1], -1)
    hw = np.asarray(image_hw_of, np.float64)
    hi = np.stack([hw[:, 1] - 1, hw[:, 0] - 1] * 2, 1)[:, None, :]
    return np.minimum(np.maximum(raw, 0.0), hi), raw


# ----------------------------------------------------------------------------- sampler and gather
def sample(labels, N, Pn, batch, frac, seed=0, keys=None):
    """the sampler's rule (tests/rpn_ref.py) on the padded layout: image n owns indices [n P, (n + 1) P), key index i = n P + p"""
    img = np.repeat(np.arange(N), Pn)
    return P.sample(np.asarray(labels), img, N, batch, frac, seed=seed, keys=keys)


def gather(props, boxes, labels, matched, sampled, weights=WEIGHTS):
    """-> rois [R, 5] fp32, labels [R], reg_targets [R, 4] fp64 (zero where label <= 0), src [R], counts [N, 2]: the sampled
    proposals image by image, by ascending index within the image"""
    N, Pn = props.shape[:2]
    s = np.asarray(sampled).reshape(N, Pn)
    lab_in, m_in = np.asarray(labels).reshape(N, Pn), np.asarray(matched).reshape(N, Pn)
    rois, labs, tg, src = [], [], [], []
    for n in range(N):
        idx = np.nonzero(s[n])[0]
        lab = np.where((s[n, idx] == 1) & (lab_in[n, idx] > 0), lab_in[n, idx], 0)
        t = np.zeros((idx.size, 4))
        pos = lab > 0
        if pos.any():
            t[pos] = encode(boxes[n][m_in[n, idx[pos]]], props[n, idx[pos]], weights)
        rois.append(np.concatenate([np.full((idx.size, 1), n, np.float32), np.asarray(props[n, idx], np.float32)], 1))
        labs.append(lab)
        tg.append(t)
        src.append(idx)
    counts = np.stack([(s == 1).sum(1), (s == 2).sum(1)], 1).astype(np.int32)
    return (np.concatenate(rois, 0).astype(np.float32), np.concatenate(labs).astype(np.int64), np.concatenate(tg, 0),
            np.concatenate(src).astype(np.int64), counts)


# ----------------------------------------------------------------------------- loss (torch fp64, autograd)
def reg_columns(labels, C, agnostic):
    """[R, 4] int64: the regression columns of every row's label (class-agnostic: 4..7)"""
    base = torch.full_like(labels, 4) if agnostic else 4 * labels
    return base[:, None] + torch.arange(4)


def loss_sums(cls, reg, labels, targets, agnostic=False):
    """cls [R, C], reg [R, 4 Cr] fp64 torch, labels int64 [R] numpy, targets [R, 4] fp64 numpy -> (sum of the cross-entropy
    over the rows, sum of smooth-L1 (beta 1) over the positives' own columns)"""
    lab = torch.from_numpy(np.asarray(labels, np.int64))
    if lab.numel() == 0:
        return cls.sum() * 0, reg.sum() * 0
    m = cls.max(1, keepdim=True)[0].detach()
    ce = (torch.log(torch.exp(cls - m).sum(1)) + m[:, 0] - cls.gather(1, lab[:, None])[:, 0]).sum()
    pred = reg.gather(1, reg_columns(lab.clamp(min=0), cls.shape[1], agnostic))
    n = (pred - torch.from_numpy(np.asarray(targets, np.float64))).abs()
    sl1 = (torch.where(n < 1.0, 0.5 * n * n, n - 0.5) * (lab > 0)[:, None]).sum()
    return ce, sl1


def losses_and_grads(cls, reg, labels, targets, agnostic=False):
    """numpy in -> (loss_classifier, loss_box_reg) fp64 (both divided by R) and the gradients of their sum"""
    c = torch.from_numpy(np.asarray(cls, np.float64)).requires_grad_(True)
    r = torch.from_numpy(np.asarray(reg, np.float64)).requires_grad_(True)
    ce, sl1 = loss_sums(c, r, labels, targets, agnostic)
    Rn = max(len(labels), 1)
    ((ce + sl1) / Rn).backward()
    return float(ce.detach()) / Rn, float(sl1.detach()) / Rn, c.grad.numpy(), r.grad.numpy()


# ----------------------------------------------------------------------------- inference
def softmax64(x):
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def decode_all(cls, reg, rois, image_hw, weights=WEIGHTS, score_thresh=0.05):
    """-> scores [R, C], boxes [R, C, 4] fp64, cand bool [R, C], the unclamped dw [R, C], the unclipped boxes; a ROI whose image
    index is out of range gives zeros"""
    cls, reg, rois = np.asarray(cls, np.float64), np.asarray(reg, np.float64), np.asarray(rois, np.float64)
    Rn, C = cls.shape
    hw = np.asarray(image_hw, np.float64).reshape(-1, 2)
    img = rois[:, 0].astype(np.int64)
    ok = (rois[:, 0] >= 0) & (rois[:, 0] < hw.shape[0])
    d = reg.reshape(Rn, -1, 4)
    if d.shape[1] != C:  # class-agnostic: the last four columns for every class
        d = np.repeat(d[:, -1:], C, 1)
    boxes, raw = decode(d, rois[:, 1:], hw[np.where(ok, img, 0)], weights)
    scores = softmax64(cls)
    cand = scores > score_thresh
    cand[:, 0] = False
    dw = d[..., 2] / weights[2]
    scores[~ok], boxes[~ok], cand[~ok] = 0.0, 0.0, False
    return scores, boxes, cand, dw, raw


def postprocess(scores, boxes, cand, rois, N, nms_thr, detections_per_img):
    """-> per image (row index [k], class [k]) of the detections in the reference's order: class ascending and, within a class,
    ascending ROI index -- the reference's nms returns the kept indices sorted (csrc/cpu/nms_cpu.cpp:62, csrc/cuda/nms.cu:126),
    not by score.  Greedy NMS per class, then the kthvalue cap with >=: ties at the k-th score all stay."""
    out = []
    for n in range(N):
        rows, cls = np.nonzero(cand & (np.asarray(rois)[:, 0] == n)[:, None])
        det_r, det_c = [], []
        for j in np.unique(cls):
            sel = rows[cls == j]
            kept = sorted(P.greedy_nms(boxes[sel, j], scores[sel, j], nms_thr))
            det_r += [int(sel[k]) for k in kept]
            det_c += [int(j)] * len(kept)
        det_r, det_c = np.array(det_r, np.int64), np.array(det_c, np.int64)
        if 0 < detections_per_img < det_r.size:
            sc = scores[det_r, det_c]
            kth = np.sort(sc)[det_r.size - detections_per_img]
            keep = sc >= kth
            det_r, det_c = det_r[keep], det_c[keep]
        out.append((det_r, det_c))
    return out


# ----------------------------------------------------------------------------- fixtures
def load_case(gold_dir, name):
    z = np.load(os.path.join(gold_dir, name + ".npz"))
    f = {k: z[k] for k in z.files}
    f["N"] = int(f["boxes"].shape[0])
    f["P"] = int(f["props"].shape[1])
    f["C"] = int(f["num_classes"])
    f["agnostic"] = bool(f["cls_agnostic"])
    f["image_hw"] = [tuple(int(v) for v in f["image_hw_one"])] * f["N"]
    return f


def check_match_conditions(f, ious, labels):
    """the fixture conditions on the matcher and the sampler (tools/make_roi_box_golden.py)"""
    bg, fg, batch, frac = float(f["bg"]), float(f["fg"]), int(f["batch_size_per_image"]), float(f["positive_fraction"])
    N, Pn = f["N"], f["P"]
    b = f["boxes"]
    for n in range(N):
        g = b[n, :int(f["ng"][n])]
        assert (g != np.round(g)).all(), "an integer ground-truth coordinate"
        q = ious[n].astype(np.float64)
        assert ((np.abs(q - bg) > 1e-6) & (np.abs(q - fg) > 1e-6)).all(), "an IoU within 1e-6 of a threshold"
        if q.shape[0] > 1:
            top = np.sort(q, 0)[::-1]
            assert ((top[0] - top[1] > 1e-6) | (top[0] == 0)).all(), "two boxes within 1e-6 of a proposal's maximum"
    lab = np.asarray(labels).reshape(N, Pn)
    n_pos = [int((lab[n] > 0).sum()) for n in range(N)]
    cap = int(batch * frac)
    assert max(n_pos) > cap and min(n_pos) < cap, (n_pos, cap)
    assert min(int(v) for v in f["np"]) < batch, "every image has at least BATCH_SIZE_PER_IMAGE proposals"
    assert np.unique(lab[lab > 0]).size >= 3, "positives of fewer than three classes"
    if bg < fg:
        real = np.arange(Pn)[None] < np.asarray(f["np"])[:, None]
        assert (lab[real] == -1).any(), "no between-thresholds proposal"
    return n_pos


def check_post_conditions(f, scores, boxes, cand, dw, raw):
    """the fixture conditions on the post-processor; -> detections per image before the cap"""
    thr, nms_thr, cap = float(f["score_thresh"]), float(f["nms"]), int(f["detections_per_img"])
    rois = f["inf_rois"]
    assert (np.abs(scores[:, 1:] - thr) > 1e-6).all(), "a score within 1e-6 of SCORE_THRESH"
    assert (dw > CLIP).any(), "no dw above the clamp"
    assert (raw != boxes).any(), "no decoded box is clipped"
    before, bound = [], []
    for n in range(f["N"]):
        own = rois[:, 0] == n
        removed, kept_scores = 0, []
        for j in range(1, scores.shape[1]):
            sel = np.nonzero(cand[:, j] & own)[0]
            if sel.size == 0:
                continue
            s = np.sort(scores[sel, j])
            assert (s[1:] - s[:-1] > 1e-6).all(), "two candidates of one image and class within 1e-6"
            q = R.iou_plus1(boxes[sel, j], boxes[sel, j])
            assert (np.abs(q[np.triu_indices(sel.size, 1)] - nms_thr) > 1e-6).all(), "a same-class IoU within 1e-6 of NMS"
            kept = P.greedy_nms(boxes[sel, j], scores[sel, j], nms_thr)
            removed += sel.size - len(kept)
            kept_scores += [scores[sel[k], j] for k in kept]
        assert removed > 0, "NMS removes nothing in image %d" % n
        before.append(len(kept_scores))
        bound.append(len(kept_scores) > cap)
        if len(kept_scores) > cap:
            s = np.sort(np.array(kept_scores))[::-1]
            assert s[cap - 1] - s[cap] > 1e-6, "the k-th score is within 1e-6 of the next"
    assert any(bound) and not all(bound), ("DETECTIONS_PER_IMG must bind in one image and not in the other", before, cap)
    return before

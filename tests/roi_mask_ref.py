"""fp64 / integer numpy restatement of the Mask R-CNN mask head's device work: the compaction of the positive rows, the crop rule
of BinaryMaskList.crop, the mask target as the exact value of the reference's bilinear resize + truncation decided in integers
(and, for comparison, the same expression evaluated in fp32 the way torch does), the binary cross-entropy with its gradient, the
sigmoid, and Masker's paste with the reference's fp32 box expansion restated separately -- written from the reference's
definitions (roi_heads/mask_head/loss.py, inference.py, structures/segmentation_mask.py) and from the rules stated in
include/scan_hip.h, not from the project's kernels."""
import os

import numpy as np

CASES = ("roi_mask_64x96", "roi_mask_m14_64x96", "roi_mask_c81_128x256")
ROUNDING_CAP = 0.10  # the reference's fp32 rounding zeros: below this share of the rule's ones in every case


# ----------------------------------------------------------------------------- masks layout
def pack_masks(per_image):
    """list of uint8 [G_n, h_n, w_n] -> (flat uint8, moff int64 [N + 1], mhw int32 [N, 2]): image after image, no padding"""
    off = [0]
    for m in per_image:
        off.append(off[-1] + m.size)
    flat = np.concatenate([np.asarray(m, np.uint8).reshape(-1) for m in per_image]) if per_image else np.zeros((0,), np.uint8)
    return flat, np.array(off, np.int64), np.array([m.shape[1:] for m in per_image], np.int32).reshape(-1, 2)


def unpack_masks(flat, moff, mhw):
    out = []
    for n in range(len(mhw)):
        h, w = int(mhw[n][0]), int(mhw[n][1])
        out.append(np.asarray(flat[int(moff[n]):int(moff[n + 1])]).reshape(-1, h, w))
    return out


# ----------------------------------------------------------------------------- positives
def positives(labels, rois, src, matched, P):
    """-> pos_rows, pos_rois, pos_labels, pos_gt: the rows with label > 0 in row order, numpy.nonzero's"""
    labels = np.asarray(labels)
    rows = np.nonzero(labels > 0)[0]
    img = np.asarray(rois)[rows, 0].astype(np.int64)
    return rows, np.asarray(rois)[rows], labels[rows], np.asarray(matched)[img * P + np.asarray(src)[rows]]


# ----------------------------------------------------------------------------- targets
def crop_box(box, w, h):
    """BinaryMaskList.crop (segmentation_mask.py:89-108) -> xmin, ymin, xmax, ymax; Python's round is half-to-even"""
    xmin, ymin, xmax, ymax = [round(float(np.float32(b))) for b in box]
    xmin, ymin = min(max(xmin, 0), w - 1), min(max(ymin, 0), h - 1)
    xmax, ymax = min(max(xmax, 0), w), min(max(ymax, 0), h)
    return xmin, ymin, max(xmax, xmin + 1), max(ymax, ymin + 1)


def axis_rule(n, M):
    """per output index d of M along a crop axis of length n: first neighbour, second neighbour, whether the second takes part
    (has a nonzero exact weight): the source coordinate ((2 d + 1) n - M) / (2 M), clamped at 0, in integers"""
    d = np.arange(M, dtype=np.int64)
    num = np.maximum((2 * d + 1) * n - M, 0)
    i0 = num // (2 * M)
    return i0, np.minimum(i0 + 1, n - 1), (num % (2 * M)) != 0


def target_rule(mask, box, M):
    """mask uint8 [h, w] of 0 / 1, box xyxy -> uint8 [M, M]: 1 iff every neighbour with a nonzero exact weight is 1, which is the
    exact value of the bilinear (align_corners=False) sum of 0 / 1 pixels truncated to uint8"""
    h, w = mask.shape
    xmin, ymin, xmax, ymax = crop_box(box, w, h)
    c = np.asarray(mask[ymin:ymax, xmin:xmax]) != 0
    x0, x1, sx = axis_rule(xmax - xmin, M)
    y0, y1, sy = axis_rule(ymax - ymin, M)
    out = c[y0][:, x0]
    out = out & (c[y0][:, x1] | ~sx[None, :])
    out = out & (c[y1][:, x0] | ~sy[:, None])
    out = out & (c[y1][:, x1] | ~(sy[:, None] & sx[None, :]))
    return out.astype(np.uint8)


def _axis_fp32(n, M):
    scale = np.float32(n) / np.float32(M)
    s = np.maximum(scale * (np.arange(M, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5), np.float32(0))
    i0 = np.minimum(s.astype(np.int64), n - 1)
    l1 = (s - i0.astype(np.float32)).astype(np.float32)
    return i0, np.minimum(i0 + 1, n - 1), np.float32(1) - l1, l1


def target_fp32(mask, box, M):
    """the reference's expression in fp32, operation by operation the way torch's bilinear kernel states it (scale = in / out,
    source = scale (d + 0.5) - 0.5 clamped at 0, the two lambdas, rows combined after columns), truncated to uint8: what can
    round an exact 1 down to 0"""
    h, w = mask.shape
    xmin, ymin, xmax, ymax = crop_box(box, w, h)
    c = np.asarray(mask[ymin:ymax, xmin:xmax]).astype(np.float32)
    x0, x1, a0, a1 = _axis_fp32(xmax - xmin, M)
    y0, y1, b0, b1 = _axis_fp32(ymax - ymin, M)
    top = a0[None] * c[y0][:, x0] + a1[None] * c[y0][:, x1]
    bot = a0[None] * c[y1][:, x0] + a1[None] * c[y1][:, x1]
    return (b0[:, None] * top + b1[:, None] * bot).astype(np.float32).astype(np.uint8)


def targets_rule(masks_per_image, pos_rois, pos_gt, M):
    out = np.zeros((len(pos_rois), M, M), np.uint8)
    for r, (roi, g) in enumerate(zip(pos_rois, pos_gt)):
        out[r] = target_rule(masks_per_image[int(roi[0])][int(g)], roi[1:], M)
    return out


# ----------------------------------------------------------------------------- loss
def make_logits(seed, K, C, M, scale=2.0):
    """fp32 [K, C, M, M]: numpy's legacy generator, the same values wherever it runs (the fixtures store a seed, not the logits)"""
    return (np.random.RandomState(int(seed)).standard_normal((K, C, M, M)) * scale).astype(np.float32)


def logits_rows(logits, cs=None):
    """[K, C, M, M] -> the conv output rows [K * M * M, Cs], zero-padded columns C..Cs"""
    K, C, M, _ = logits.shape
    cs = cs or (C + 3) // 4 * 4
    rows = np.zeros((K * M * M, cs), np.float32)
    rows[:, :C] = logits.transpose(0, 2, 3, 1).reshape(-1, C)
    return rows


def bce(x, t):
    """fp64: x, t [Rp, M, M] (the label's channel, the targets) -> (mean loss, d loss / d x)"""
    x, t = np.asarray(x, np.float64), np.asarray(t, np.float64)
    if x.size == 0:
        return 0.0, np.zeros(x.shape)
    loss = np.maximum(x, 0) - x * t + np.log1p(np.exp(-np.abs(x)))
    sig = np.where(x >= 0, 1 / (1 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1 + np.exp(-np.abs(x))))
    return float(loss.mean()), (sig - t) / x.size


def sigmoid(x):
    x = np.asarray(x, np.float64)
    z = np.exp(-np.abs(x))
    return np.where(x >= 0, 1 / (1 + z), z / (1 + z))


# ----------------------------------------------------------------------------- paste
def expand_box_fp32(box, M):
    """expand_boxes (inference.py:91-105) by (M + 2) / M operation by operation in fp32 -> the four expanded fp32 coordinates
    (x0, y0, x1, y1); .to(torch.int32) then truncates them toward zero"""
    b = np.asarray(box, np.float32)
    scale = np.float32(float(M + 2) / M)
    half = np.float32(0.5)
    wh, hh = (b[2] - b[0]) * half * scale, (b[3] - b[1]) * half * scale
    xc, yc = (b[2] + b[0]) * half, (b[3] + b[1]) * half
    return np.array([xc - wh, yc - hh, xc + wh, yc + hh], np.float32)


def _paste_axis(n_out, n_in):
    s = np.maximum((n_in / n_out) * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5, 0.0)
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    l1 = s - i0
    return i0, np.minimum(i0 + 1, n_in - 1), 1 - l1, l1


def paste(prob, box, H, W, thresh=0.5):
    """prob [M, M], box xyxy -> (uint8 [H, W], the fp64 interpolated values inside the pasted window): paste_mask_in_image
    (inference.py:118-151) with padding 1, the interpolation in fp64"""
    M = prob.shape[0]
    x0, y0, x1, y1 = [int(np.trunc(v)) for v in expand_box_fp32(box, M)]
    w, h = max(x1 - x0 + 1, 1), max(y1 - y0 + 1, 1)
    pad = np.zeros((M + 2, M + 2))
    pad[1:-1, 1:-1] = prob
    ix0, ix1, a0, a1 = _paste_axis(w, M + 2)
    iy0, iy1, b0, b1 = _paste_axis(h, M + 2)
    top = a0[None] * pad[iy0][:, ix0] + a1[None] * pad[iy0][:, ix1]
    bot = a0[None] * pad[iy1][:, ix0] + a1[None] * pad[iy1][:, ix1]
    val = b0[:, None] * top + b1[:, None] * bot
    out = np.zeros((H, W), np.uint8)
    xa, xb, ya, yb = max(x0, 0), min(x1 + 1, W), max(y0, 0), min(y1 + 1, H)
    if xb <= xa or yb <= ya:
        return out, np.zeros((0,))
    win = val[ya - y0:yb - y0, xa - x0:xb - x0]
    out[ya:yb, xa:xb] = win > thresh
    return out, win.reshape(-1)


# ----------------------------------------------------------------------------- fixtures
def bits(a):
    return np.packbits(np.asarray(a, np.uint8).reshape(-1))


def unbits(b, shape):
    n = int(np.prod(shape))
    return np.unpackbits(np.asarray(b, np.uint8))[:n].reshape(shape)


def load_case(gold_dir, name):
    z = np.load(os.path.join(gold_dir, name + ".npz"))
    f = {k: z[k] for k in z.files}
    f["N"], f["P"], f["C"], f["M"] = int(f["boxes"].shape[0]), int(f["props"].shape[1]), int(f["num_classes"]), int(f["resolution"])
    f["predictor"] = str(f["predictor"])
    f["H"], f["W"] = (int(v) for v in f["image_hw_one"])
    f["masks"] = unbits(f["masks_bits"], (int(f["moff"][-1]),))
    f["masks_per_image"] = unpack_masks(f["masks"], f["moff"], f["mhw"])
    Rp, M = int(f["pos_rows"].shape[0]), f["M"]
    f["Rp"] = Rp
    f["ref_targets"] = unbits(f["ref_targets_bits"], (Rp, M, M))
    K = int(f["det_box"].shape[0])
    f["K"] = K
    f["ref_paste"] = unbits(f["ref_paste_bits"], (K, f["H"], f["W"]))
    return f


def check_target_conditions(f, rule, ref):
    """the fixture conditions on the targets (tools/make_roi_mask_golden.py); rule / ref: uint8 [Rp, M, M] of the integer rule and
    of the reference -> (pixels where they differ, the rule's ones)"""
    H, W = f["H"], f["W"]
    pos = f["pos_rois"][:, 1:]
    frac_half = np.abs(pos - np.floor(pos) - 0.5) < 1e-6
    ipart = np.floor(pos).astype(np.int64)
    assert (frac_half & (ipart % 2 == 0)).any() and (frac_half & (ipart % 2 == 1)).any(), "no .5 coordinate of each parity"
    crops = np.array([crop_box(b, W, H) for b in pos])
    assert (crops[:, 0] == 0).any() and (crops[:, 1] == 0).any() and (crops[:, 2] == W).any() and (crops[:, 3] == H).any(), \
        "no crop touches each image border"
    assert (crops[:, 2] - crops[:, 0] == 1).any(), "no crop is 1 pixel wide"
    assert (np.asarray(f["ng"]) == 1).any(), "no image with a single ground-truth box"
    for n, m in enumerate(f["masks_per_image"]):
        b = f["boxes"][n]
        for g in range(m.shape[0]):
            ys, xs = np.nonzero(m[g])
            assert ys.size and xs.min() >= np.floor(b[g, 0]) and xs.max() <= np.ceil(b[g, 2]) and ys.min() >= np.floor(b[g, 1]) \
                and ys.max() <= np.ceil(b[g, 3]), "a mask leaves its box"
            full = (np.ceil(b[g, 2]) - np.floor(b[g, 0]) + 1) * (np.ceil(b[g, 3]) - np.floor(b[g, 1]) + 1)
            assert ys.size < full, "a mask fills its box"
    assert (rule >= ref).all(), "the reference writes 1 where the exact value is below 1"
    diff = int((rule != ref).sum())
    ones = int(rule.sum())
    assert (rule[rule != ref] == 1).all() and diff < ROUNDING_CAP * ones, (diff, ones)
    return diff, ones


def check_paste_conditions(f, prob):
    """the fixture conditions on the paste; prob fp64 [K, M, M] -> the restatement's pasted masks uint8 [K, H, W]"""
    H, W, M, thr = f["H"], f["W"], f["M"], float(f["thresh"])
    out = np.zeros((f["K"], H, W), np.uint8)
    exp = np.array([expand_box_fp32(b, M) for b in f["det_box"]], np.float64)
    assert (np.abs(exp - np.round(exp)) > 1e-4).all(), "an expanded coordinate within 1e-4 of an integer"
    assert (exp[:, 0] < 0).any() and (exp[:, 1] < 0).any() and (exp[:, 2] > W).any() and (exp[:, 3] > H).any(), \
        "no expanded box leaves the image on each side"
    assert (np.trunc(exp[:, :2]) < 0).any(), "no negative expanded coordinate"
    assert (f["det_box"][:, 2] - f["det_box"][:, 0] < 2).any(), "no box narrower than 2 pixels"
    for k in range(f["K"]):
        out[k], val = paste(prob[k], f["det_box"][k], H, W, thr)
        assert val.size == 0 or np.abs(val - thr).min() > 1e-5, "an interpolated value within 1e-5 of the threshold"
    return out

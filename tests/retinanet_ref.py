"""fp64 / numpy restatement of the RetinaNet head's ground-truth side: cell anchors, anchors in index order, +1 IoU, the
IoU-threshold matcher with low-quality matches, BoxCoder.encode and the smooth-L1 loss -- written from the reference's
definitions (rpn/anchor_generator.py, modeling/matcher.py, modeling/box_coder.py, layers/smooth_l1_loss.py), not from the
project's kernels.  The IoU alone is ALSO available in fp32 (``dtype=np.float32``): the matcher compares IoUs for equality,
which only means something in the precision the reference computes them in; numpy's fp32 operations round one by one like
torch's.  Test inputs for the tie / edge cases live here too."""
import os

import numpy as np
import torch

STRIDES = (8, 16, 32, 64, 128)
SIZES = (32, 64, 128, 256, 512)
CASES = ("retinanet_64x96", "retinanet_128x256")
SIZES_64x96 = [(8, 12), (4, 6), (2, 3), (1, 2), (1, 1)]
SIZES_128x256 = [(16, 32), (8, 16), (4, 8), (2, 4), (1, 2)]


def cell_anchors(strides=STRIDES, sizes=SIZES, ratios=(0.5, 1.0, 2.0), octave=2.0, scales_per_octave=3):
    """[L][A][4] fp64: per level, for each ratio (outer) and octave step (inner) a box about the centre of the first cell"""
    out = []
    for s, size in zip(strides, sizes):
        c = (s - 1) / 2.0
        level = []
        for r in ratios:
            w = np.round(np.sqrt(s * s / r))
            h = np.round(w * r)
            for k in range(scales_per_octave):
                f = size * octave ** (k / float(scales_per_octave)) / s
                level.append([c - 0.5 * (w * f - 1), c - 0.5 * (h * f - 1), c + 0.5 * (w * f - 1), c + 0.5 * (h * f - 1)])
        out.append(level)
    return np.array(out, dtype=np.float64)


def row_offsets(n_images, sizes):
    off = [0]
    for h, w in sizes:
        off.append(off[-1] + n_images * h * w)
    return off


def anchors_in_order(n_images, sizes, cells, strides=STRIDES, dtype=np.float64):
    """[M * A, 4] (level, image, y, x, a) and the image of every anchor; cells are rounded to fp32 first, as the reference's"""
    cells = np.asarray(cells, dtype=np.float32).astype(dtype)
    out, img = [], []
    for l, ((h, w), s) in enumerate(zip(sizes, strides)):
        ys, xs = np.meshgrid(np.arange(h) * s, np.arange(w) * s, indexing="ij")
        sh = np.stack([xs.reshape(-1), ys.reshape(-1), xs.reshape(-1), ys.reshape(-1)], 1).astype(dtype)
        a = (sh[:, None, :] + cells[l][None]).reshape(-1, 4)
        for n in range(n_images):
            out.append(a)
            img.append(np.full(a.shape[0], n))
    return np.concatenate(out, 0), np.concatenate(img, 0)


def iou_plus1(boxes, anchors):
    """[G, n]; the dtype of the inputs is the dtype of every operation"""
    one = boxes.dtype.type(1)
    a1 = (boxes[:, 2] - boxes[:, 0] + one) * (boxes[:, 3] - boxes[:, 1] + one)
    a2 = (anchors[:, 2] - anchors[:, 0] + one) * (anchors[:, 3] - anchors[:, 1] + one)
    w = np.maximum(np.minimum(boxes[:, None, 2], anchors[None, :, 2]) - np.maximum(boxes[:, None, 0], anchors[None, :, 0]) + one, 0)
    h = np.maximum(np.minimum(boxes[:, None, 3], anchors[None, :, 3]) - np.maximum(boxes[:, None, 1], anchors[None, :, 1]) + one, 0)
    inter = w * h
    return inter / (a1[:, None] + a2[None] - inter)


def match(n_images, sizes, targets, cells, strides=STRIDES, bg=0.4, fg=0.5, dtype=np.float32):
    """labels [M * A] (0 / -1 / class), matched [M * A] (0 where label <= 0) and per image the IoU matrix.  For each anchor:
    best box (first of equals); below bg -> 0, below fg -> -1; then every anchor that attains some box's row maximum is given
    its own best box back."""
    anchors, img = anchors_in_order(n_images, sizes, cells, strides, dtype)
    labels = np.zeros(anchors.shape[0], np.int64)
    matched = np.zeros(anchors.shape[0], np.int64)
    ious = []
    for n, (b, lab) in enumerate(targets):
        b, lab = np.asarray(b, dtype=np.float32).astype(dtype), np.asarray(lab)
        sel = np.nonzero(img == n)[0]
        if b.shape[0] == 0:
            ious.append(np.zeros((0, sel.size), dtype))
            continue
        q = iou_plus1(b, anchors[sel])
        ious.append(q)
        best, arg = q.max(0), q.argmax(0)
        lb = np.where(best < dtype(bg), 0, np.where(best < dtype(fg), -1, lab[arg]))
        low = (q == q.max(1)[:, None]).any(0)
        lb = np.where(low, lab[arg], lb)
        labels[sel] = lb
        matched[sel] = np.where(lb > 0, arg, 0)
    return labels, matched, ious


def encode(gt, anchors):
    ew, eh = anchors[:, 2] - anchors[:, 0] + 1, anchors[:, 3] - anchors[:, 1] + 1
    ecx, ecy = anchors[:, 0] + 0.5 * ew, anchors[:, 1] + 0.5 * eh
    gw, gh = gt[:, 2] - gt[:, 0] + 1, gt[:, 3] - gt[:, 1] + 1
    gcx, gcy = gt[:, 0] + 0.5 * gw, gt[:, 1] + 0.5 * gh
    return np.stack([10 * (gcx - ecx) / ew, 10 * (gcy - ecy) / eh, 5 * np.log(gw / ew), 5 * np.log(gh / eh)], 1)


def targets64(n_images, sizes, targets, cells, labels, matched, strides=STRIDES):
    """[M * A, 4] fp64 regression targets, zero where label <= 0"""
    anchors, img = anchors_in_order(n_images, sizes, cells, strides)
    G = max(1, max(len(b) for b, _ in targets))
    boxes = np.zeros((n_images, G, 4))
    for n, (b, _) in enumerate(targets):
        boxes[n, :len(b)] = np.asarray(b, dtype=np.float32)
    t = encode(boxes[img, matched], anchors)
    return np.where((labels > 0)[:, None], t, 0.0)


def smooth_l1_sum(pred, target, pos, beta):
    """torch fp64 (autograd): sum over the positive anchors' four elements"""
    n = (pred - target).abs()
    return (torch.where(n < beta, 0.5 * n * n / beta, n - 0.5 * beta) * pos[:, None]).sum()


def focal_sum(logits, labels, gamma, alpha):
    """layers/sigmoid_focal_loss.py: sigmoid_focal_loss_cpu, fp64; labels < 0 match no class and are masked out"""
    C = logits.shape[1]
    cls = torch.arange(1, C + 1, dtype=labels.dtype)[None]
    t = labels[:, None]
    p = torch.sigmoid(logits)
    pos = -(1 - p) ** gamma * torch.log(p) * alpha
    neg = -p ** gamma * torch.log(1 - p) * (1 - alpha)
    return (pos * (t == cls) + neg * ((t != cls) & (t >= 0))).sum()


def load_case(gold_dir, name):
    z = np.load(os.path.join(gold_dir, name + ".npz"))
    f = {k: z[k] for k in z.files}
    f["sizes"] = [tuple(int(v) for v in s) for s in f["sizes"]]
    f["N"] = int(f["boxes"].shape[0])
    f["targets"] = [(torch.from_numpy(f["boxes"][n, :g]), torch.from_numpy(f["glabels"][n, :g])) for n, g in enumerate(f["ng"])]
    return f


def check_case_conditions(ious, labels_per_image, bg, fg):
    """the fixture conditions (tools/make_retinanet_golden.py) on fp32 IoU matrices [G, n] of every image: no anchor has two
    boxes within 1e-6 of its maximum; every box overlaps some anchor; there is an anchor in [bg, fg), an anchor positive only
    through the low-quality rule and a box whose best IoU is below bg"""
    between = lowq = weak = 0
    for q, lab in zip(ious, labels_per_image):
        q = q.astype(np.float64)
        top = np.sort(q, 0)[::-1]
        if q.shape[0] > 1:
            assert ((top[0] - top[1] > 1e-6) | (top[0] == 0)).all(), "two boxes within 1e-6 of an anchor's maximum"
        assert (q.max(1) > 0).all(), "a box overlaps no anchor"
        best = q.max(0)
        between += int(((best >= bg) & (best < fg) & (lab == -1)).sum())
        lowq += int(((best < fg) & (lab > 0)).sum())
        weak += int((q.max(1) < bg).sum())
    assert between > 0 and lowq > 0 and weak > 0, (between, lowq, weak)
    return between, lowq, weak


# ----------------------------------------------------------------------------- tie / edge inputs
def edge_inputs(which):
    """(N, sizes, targets, cell kwargs, bg, fg) of the constructed cases; A = 1 uses ratio 1 and one scale: square anchors of
    side `size` with integer corners (level 0: centre 3.5 -/+ 15.5)"""
    one = dict(ratios=(1.0,), scales_per_octave=1)
    if which == "centred_tie":
        # A = 1, level-0 anchors of side 32 at stride 8: x1 = 3.5 - 15.5 + 8 x.  An integer box centred between two locations
        # (x = 1 and x = 2: centres 11.5 and 19.5, box centre 15.5) has the same IoU with both
        return 1, SIZES_64x96, [(torch.tensor([[2., 4., 29., 35.]]), torch.tensor([1]))], one, 0.4, 0.5
    if which == "duplicate":
        b = [[20.3, 10.2, 70.6, 50.7], [20.3, 10.2, 70.6, 50.7], [50.2, 20.1, 90.4, 60.3]]
        return 1, SIZES_64x96, [(torch.tensor(b), torch.tensor([2, 1, 1]))], {}, 0.4, 0.5
    if which in ("at_fg", "at_bg"):
        # A = 1: level 0 has side-32 anchors (-12 + 8 x, ..., 19 + 8 x), area 1024; level 1 side-64 anchors (-24 + 16 x, ...,
        # 39 + 16 x), area 4096.  The box IS the level-0 anchor of location (1, 1): (-4, -4, 27, 27), its own maximum (IoU 1),
        # and lies inside the level-1 anchors of locations (0, 0), (1, 0), (0, 1), (1, 1): IoU = 1024 / 4096 = 0.25 exactly, not
        # the box's maximum.  at_fg: fg = 0.25, those anchors are positive by the threshold; at_bg: bg = 0.25, they are -1
        bg, fg = (0.125, 0.25) if which == "at_fg" else (0.25, 0.5)
        return 1, SIZES_64x96, [(torch.tensor([[-4., -4., 27., 27.]]), torch.tensor([2]))], one, bg, fg
    if which == "empty_image":
        b = [[10.3, 12.2, 40.6, 50.7], [30.1, 5.4, 76.3, 45.8], [0.4, 20.3, 19.7, 44.2], [60.2, 30.3, 95.1, 63.4],
             [45.5, 2.5, 60.25, 20.75]]
        return 2, SIZES_64x96, [(torch.zeros((0, 4)), torch.zeros((0,), dtype=torch.int64)),
                                (torch.tensor(b), torch.tensor([1, 2, 1, 2, 1]))], {}, 0.4, 0.5
    if which == "far_box":
        # the second box overlaps no anchor: its maximum is 0, which every anchor that misses it equals
        b = [[20.3, 10.2, 70.6, 50.7], [5000.5, 5000.5, 5010.5, 5010.5]]
        return 1, SIZES_64x96, [(torch.tensor(b), torch.tensor([1, 2]))], {}, 0.4, 0.5
    if which == "a1":
        b = [[20.3, 10.2, 50.6, 40.7], [60.1, 30.4, 90.3, 60.8]]
        return 2, SIZES_64x96, [(torch.tensor(b), torch.tensor([1, 2])), (torch.tensor(b[:1]), torch.tensor([2]))], one, 0.4, 0.5
    assert which == "a3"
    b = [[20.3, 10.2, 50.6, 40.7], [60.1, 30.4, 90.3, 60.8]]
    return 2, SIZES_64x96, [(torch.tensor(b), torch.tensor([1, 2])), (torch.tensor(b[1:]), torch.tensor([1]))], \
        dict(scales_per_octave=1), 0.4, 0.5


EDGE_CASES = ("centred_tie", "duplicate", "at_fg", "at_bg","empty_image", "far_box", "a1", "a3")

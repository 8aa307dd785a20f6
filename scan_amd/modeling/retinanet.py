"""RetinaNet head, ground-truth plan, loss and post-processor on pyramid activations.

Mirrors the reference's fcos_core/modeling/rpn/retinanet/{retinanet.py, loss.py, inference.py} with modeling/matcher.py,
modeling/box_coder.py and rpn/anchor_generator.py.  A = len(ASPECT_RATIOS) * SCALES_PER_OCTAVE anchors per location (1..16):
pyramid row m = (level, image, y, x) holds the anchors cell[level][a] + (x s, y s, x s, y s), a < A.  A head output row [A * C] is
A anchors of C classes (the reference's permute_and_flatten makes the channel a * C + c), so a [M, A * C] matrix viewed as
[M * A, C] is in the reference's anchor order level by level, and anchor index i = m * A + a throughout.  No [M * A, 4] anchor
tensor is stored for training: the kernels of csrc/retina.hip form each anchor from its row and the [L, A, 4] cell table.

Conv outputs have padded row pitches (ops.pad4).  bbox_reg ([M, 4 A]) is read by the smooth-L1 kernels in place through its
pitch; the focal kernels take a contiguous [M * A, C] matrix, which is a view of the logits when A * C is a multiple of 4 and a
COPY of their first A * C columns otherwise (autograd returns the gradient through the slice).

``assign_targets`` is the torch spelling of the assignment, on any device; the kernels are held equal to it.
"""
import math

import numpy as np
import torch
from torch import nn

from .. import ops
from ..layers import SigmoidFocalLoss
from . import fcos as fcos_mod
from .backbone import conv_holder

ANCHOR_STRIDES = (8, 16, 32, 64, 128)
ANCHOR_SIZES = (32, 64, 128, 256, 512)
BBOX_XFORM_CLIP = math.log(1000. / 16)  # box_coder.py:13
MAX_ANCHORS = 16  # RETINA_MAX_A of csrc/retina.hip

# config.retinanet_settings(cfg) keys with the reference's defaults (config/defaults.py:415-470)
DEFAULT_SETTINGS = dict(num_classes=81, anchor_sizes=ANCHOR_SIZES, anchor_strides=ANCHOR_STRIDES, aspect_ratios=(0.5, 1.0, 2.0),
                        octave=2.0, scales_per_octave=3, num_convs=4, bbox_reg_weight=4.0, bbox_reg_beta=0.11,
                        pre_nms_top_n=1000, fg_iou_threshold=0.5, bg_iou_threshold=0.4, loss_alpha=0.25, loss_gamma=2.0,
                        prior_prob=0.01, inference_th=0.05, nms_th=0.4, detections_per_img=100)


# ----------------------------------------------------------------------------- anchors
def cell_anchors(strides=ANCHOR_STRIDES, sizes=ANCHOR_SIZES, aspect_ratios=(0.5, 1.0, 2.0), octave=2.0, scales_per_octave=3):
    """[L, A, 4] fp32 xyxy: the anchors of the cell at the origin of every level, ratio-major, scale-minor (reference
    rpn/anchor_generator.py:146-166, 242-320).  fp64 numpy, rounded to fp32 at the end.  Per level of stride s the window
    (0, 0, s - 1, s - 1) is reshaped per ratio r to w = round(sqrt(s * s / r)), h = round(w * r) about its centre (s - 1) / 2,
    then scaled per octave step k by size * octave ** (k / scales_per_octave) / s."""
    ratios = np.array(aspect_ratios, dtype=np.float64)
    out = []
    for s, size in zip(strides, sizes):
        scales = np.array([octave ** (k / float(scales_per_octave)) * size for k in range(scales_per_octave)], dtype=np.float64) / s
        ctr = 0.5 * (float(s) - 1)
        ws = np.round(np.sqrt(float(s) * float(s) / ratios))
        hs = np.round(ws * ratios)
        level = []
        for w, h in zip(ws, hs):
            # the ratio anchor's own extent and centre, re-derived from its corners as the reference does
            x1, y1, x2, y2 = ctr - 0.5 * (w - 1), ctr - 0.5 * (h - 1), ctr + 0.5 * (w - 1), ctr + 0.5 * (h - 1)
            aw, ah = x2 - x1 + 1, y2 - y1 + 1
            cx, cy = x1 + 0.5 * (aw - 1), y1 + 0.5 * (ah - 1)
            sw, sh = aw * scales, ah * scales
            level.append(np.stack([cx - 0.5 * (sw - 1), cy - 0.5 * (sh - 1), cx + 0.5 * (sw - 1), cy + 0.5 * (sh - 1)], 1))
        out.append(np.concatenate(level, 0))
    return torch.from_numpy(np.stack(out, 0)).float()


def level_anchors(shape, cells, strides=ANCHOR_STRIDES):
    """per level the anchors [h * w * A, 4] of one image: location-major (x fastest), anchor-minor; on cells' device"""
    out = []
    for (h, w), s, c in zip(shape.sizes, strides, cells):
        xs = torch.arange(0, w * s, step=s, dtype=torch.float32, device=cells.device)
        ys = torch.arange(0, h * s, step=s, dtype=torch.float32, device=cells.device)
        sy, sx = torch.meshgrid(ys, xs, indexing="ij")
        sx, sy = sx.reshape(-1), sy.reshape(-1)
        shifts = torch.stack((sx, sy, sx, sy), dim=1)
        out.append((shifts.view(-1, 1, 4) + c.view(1, -1, 4)).reshape(-1, 4))
    return out


def all_anchors(shape, cells, strides=ANCHOR_STRIDES):
    """[M * A, 4]: the anchor of every index i = m * A + a (tests and tools; the product never builds it)"""
    return torch.cat([a.repeat(shape.n_images, 1) for a in level_anchors(shape, cells, strides)], 0)


def box_iou(boxes, anchors):
    """structures/boxlist_ops.py: boxlist_iou -> [G, n]"""
    area1 = (boxes[:, 2] - boxes[:, 0] + 1) * (boxes[:, 3] - boxes[:, 1] + 1)
    area2 = (anchors[:, 2] - anchors[:, 0] + 1) * (anchors[:, 3] - anchors[:, 1] + 1)
    lt = torch.max(boxes[:, None, :2], anchors[:, :2])
    rb = torch.min(boxes[:, None, 2:], anchors[:, 2:])
    wh = (rb - lt + 1).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    return inter / (area1[:, None] + area2 - inter)


def encode(gt, anchors):
    """BoxCoder.encode, weights (10, 10, 5, 5) (box_coder.py:22-50)"""
    ew = anchors[:, 2] - anchors[:, 0] + 1
    eh = anchors[:, 3] - anchors[:, 1] + 1
    ecx = anchors[:, 0] + 0.5 * ew
    ecy = anchors[:, 1] + 0.5 * eh
    gw = gt[:, 2] - gt[:, 0] + 1
    gh = gt[:, 3] - gt[:, 1] + 1
    gcx = gt[:, 0] + 0.5 * gw
    gcy = gt[:, 1] + 0.5 * gh
    return torch.stack((10. * (gcx - ecx) / ew, 10. * (gcy - ecy) / eh, 5. * torch.log(gw / ew), 5. * torch.log(gh / eh)), dim=1)


def decode(deltas, anchors):
    """BoxCoder.decode (box_coder.py:52-95); deltas / anchors [..., 4]"""
    w = anchors[..., 2] - anchors[..., 0] + 1
    h = anchors[..., 3] - anchors[..., 1] + 1
    cx = anchors[..., 0] + 0.5 * w
    cy = anchors[..., 1] + 0.5 * h
    dw = torch.clamp(deltas[..., 2] / 5., max=BBOX_XFORM_CLIP)
    dh = torch.clamp(deltas[..., 3] / 5., max=BBOX_XFORM_CLIP)
    pcx = deltas[..., 0] / 10. * w + cx
    pcy = deltas[..., 1] / 10. * h + cy
    pw = torch.exp(dw) * w
    ph = torch.exp(dh) * h
    return torch.stack((pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw - 1, pcy + 0.5 * ph - 1), dim=-1)


def assign_targets(shape, targets, cells, strides=ANCHOR_STRIDES, bg=0.4, fg=0.5):
    """The Matcher with allow_low_quality_matches (matcher.py:42-112 through rpn/loss.py:42-89) in torch: labels [M * A] int32
    (0 background, -1 between the thresholds, else the class) and matched box [M * A] int32 (0 where label <= 0), in anchor
    order i = m * A + a.  torch.max over the boxes returns the first of equal IoUs on the CPU: the smaller box index, the
    kernels' rule.  An image without boxes is all background (the reference raises)."""
    A = int(cells.shape[1])
    dev = cells.device
    labels = torch.zeros((shape.rows * A,), dtype=torch.int32, device=dev)
    matched = torch.zeros((shape.rows * A,), dtype=torch.int32, device=dev)
    per_level = level_anchors(shape, cells, strides)
    anchors = torch.cat(per_level, 0)
    for n, (boxes, lab) in enumerate(targets):
        if int(boxes.shape[0]) == 0:
            continue
        boxes = boxes.to(device=dev, dtype=torch.float32)
        lab = lab.to(device=dev, dtype=torch.int64)
        q = box_iou(boxes, anchors)  # [G, anchors of one image]
        vals, arg = q.max(dim=0)
        m = arg.clone()
        m[vals < bg] = -1
        m[(vals >= bg) & (vals < fg)] = -2
        low = (q == q.max(dim=1)[0][:, None]).any(dim=0)
        m[low] = arg[low]
        lab_n = torch.where(m >= 0, lab[m.clamp(min=0)], torch.where(m == -1, 0, -1)).to(torch.int32)
        mat_n = torch.where(lab_n > 0, m.clamp(min=0), 0).to(torch.int32)
        a0 = 0
        for l, pl in enumerate(per_level):
            k = pl.shape[0]
            i0 = (shape.row_off[l] + n * (k // A)) * A
            labels[i0:i0 + k] = lab_n[a0:a0 + k]
            matched[i0:i0 + k] = mat_n[a0:a0 + k]
            a0 += k
    return labels, matched


# ----------------------------------------------------------------------------- the plan
class RetinaTargetPlan:
    """What the RetinaNet losses derive from the ground truth alone: the label and matched box of every anchor and the number
    of positives, with the packed boxes the smooth-L1 kernels encode against.  Built once per batch (fcos.target_plan's cache
    and side-stream protocol)."""
    __slots__ = ("key", "targets", "labels_i32", "matched", "n_pos", "boxes", "ready")


_plan = [None]
fcos_mod._plan_caches.append(_plan)
DEVICE_PLAN = True  # False: the torch spelling also on the GPU (cross-checks)
plan_stats = {"launches": 0, "host_reads": 0}  # of the most recent device plan (tools/retinanet_bench.py records them)
_cells_on = {}  # (geometry, device) -> the cell table there


def device_cells(cells, device):
    key = (tuple(cells.reshape(-1).tolist()), tuple(cells.shape), str(device))
    t = _cells_on.get(key)
    if t is None:
        t = _cells_on[key] = cells.to(device).contiguous()
    return t


def _check_geometry(shape, strides, cells):
    if not (len(strides) == cells.shape[0] == shape.n_levels):
        raise ValueError("RetinaNet: %d ANCHOR_STRIDES / %d levels of cell anchors for a pyramid of %d levels"
                         % (len(strides), cells.shape[0], shape.n_levels))
    if not 1 <= cells.shape[1] <= MAX_ANCHORS:
        raise ValueError("RetinaNet: %d anchors per location; the kernels are built for 1..%d" % (cells.shape[1], MAX_ANCHORS))


def _build_plan_device(shape, targets, device, strides, cells, bg, fg):
    """csrc/retina.hip: two memsets and two launches whatever N, G, A and the level count are, and ONE host read (the positive
    count)."""
    p = RetinaTargetPlan()
    p.ready = None
    p.boxes, glab, ng, _ = fcos_mod.upload_ground_truth(shape.n_images, targets, device)
    p.labels_i32, p.matched, n_pos = ops.retina_match(shape, strides, device_cells(cells, device), p.boxes, glab, ng, bg, fg)
    p.n_pos = int(n_pos.item())  # the one host round trip of the plan
    plan_stats.update(launches=2, host_reads=1)
    return p


def build_plan(shape, targets, device, strides=ANCHOR_STRIDES, cells=None, bg=0.4, fg=0.5):
    cells = cell_anchors() if cells is None else cells
    _check_geometry(shape, strides, cells)
    if DEVICE_PLAN and device.type == "cuda" and targets:
        return _build_plan_device(shape, targets, device, strides, cells, bg, fg)
    p = RetinaTargetPlan()
    p.ready = None
    p.labels_i32, p.matched = assign_targets(shape, targets, cells.to(device), strides, bg, fg)
    p.n_pos = int((p.labels_i32 > 0).sum())
    p.boxes = fcos_mod.pack_boxes(shape.n_images, targets, device)
    return p


def target_plan(shape, targets, device, strides=ANCHOR_STRIDES, cells=None, bg=0.4, fg=0.5, side_stream=None, after=None):
    """The RetinaTargetPlan of (shape, targets), cached for the current batch; with ``side_stream`` built there."""
    return fcos_mod.target_plan(shape, targets, device, side_stream=side_stream, after=after, cache=_plan,
                                build=lambda sh, tg, dev: build_plan(sh, tg, dev, strides, cells, bg, fg))


def regression_targets(shape, plan, cells, strides=ANCHOR_STRIDES):
    """[M * A, 4]: encode(matched box, anchor) of every anchor in torch (zero where label <= 0), formed in fp64 and rounded once
    as the kernel does; cross-checks only"""
    dev = plan.labels_i32.device
    A = int(cells.shape[1])
    anchors = all_anchors(shape, cells.to(dev), strides).double()
    hw = torch.tensor([h * w for h, w in shape.sizes], device=dev)
    off = torch.tensor(shape.row_off[:-1], device=dev)
    rows = torch.div(torch.arange(shape.rows * A, device=dev), A, rounding_mode="floor")
    lvl = torch.bucketize(rows, torch.tensor(shape.row_off[1:], device=dev), right=True)
    img = torch.div(rows - off[lvl], hw[lvl], rounding_mode="floor")
    t = encode(plan.boxes[img, plan.matched.long()].double(), anchors).float()
    return torch.where((plan.labels_i32 > 0)[:, None], t, torch.zeros_like(t))


# ----------------------------------------------------------------------------- head, loss, post-processor
class RetinaNetHead(nn.Module):
    """reference retinanet.py:13-85: cls_tower.{0,2,4,6} / bbox_tower.{0,2,4,6} conv3x3 + ReLU (no GroupNorm), cls_logits
    256 -> A * (NUM_CLASSES - 1), bbox_pred 256 -> A * 4; normal std 0.01, zero biases, PRIOR_PROB bias on cls_logits."""

    def __init__(self, num_classes=81, num_anchors=9, num_convs=4, prior_prob=0.01):
        super().__init__()
        self.num_fg, self.num_anchors, self.num_convs = num_classes - 1, num_anchors, num_convs

        def tower():
            layers = []
            for _ in range(num_convs):
                layers += [conv_holder(256, 256, 3), nn.ReLU()]
            return nn.Sequential(*layers)

        self.cls_tower = tower()
        self.bbox_tower = tower()
        self.cls_logits = conv_holder(256, num_anchors * self.num_fg, 3)
        self.bbox_pred = conv_holder(256, num_anchors * 4, 3)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, std=0.01)
                nn.init.constant_(m.bias, 0)
        nn.init.constant_(self.cls_logits.bias, -math.log((1 - prior_prob) / prior_prob))

    def forward(self, rows, shape):
        """-> logits [M, A * C] and bbox_reg [M, A * 4]: column slices of the convs' padded outputs"""
        ct = bt = rows
        for i in range(self.num_convs):
            ct = ops.conv2d(ct, self.cls_tower[2 * i].weight, self.cls_tower[2 * i].bias, shape, 3, 1, relu=True)
            bt = ops.conv2d(bt, self.bbox_tower[2 * i].weight, self.bbox_tower[2 * i].bias, shape, 3, 1, relu=True)
        logits = ops.conv2d(ct, self.cls_logits.weight, self.cls_logits.bias, shape, 3, 1)[:, :self.num_anchors * self.num_fg]
        reg = ops.conv2d(bt, self.bbox_pred.weight, self.bbox_pred.bias, shape, 3, 1)[:, :self.num_anchors * 4]
        return logits, reg


class RetinaNetLossComputation:
    """reference rpn/retinanet/loss.py:43-80 on one rank: loss_retina_cls = focal sum / (n_pos + N) over all anchors (label -1
    anchors contribute nothing: the focal kernels skip negative labels, csrc/losses.hip focal_fwd_elem / focal_bwd_elem),
    loss_retina_reg = smooth-L1 sum over the positives / max(1, n_pos * BBOX_REG_WEIGHT)."""

    def __init__(self, gamma=2.0, alpha=0.25, beta=0.11, regress_norm=4.0, strides=ANCHOR_STRIDES, cells=None, bg=0.4, fg=0.5):
        self.cls_loss_func = SigmoidFocalLoss(gamma, alpha)
        self.beta, self.regress_norm = float(beta), float(regress_norm)
        self.strides = tuple(strides)
        self.cells = cell_anchors() if cells is None else cells
        self.bg, self.fg = float(bg), float(fg)

    def plan(self, shape, targets, device, side_stream=None, after=None):
        return target_plan(shape, targets, device, self.strides, self.cells, self.bg, self.fg, side_stream, after)

    def __call__(self, shape, box_cls, box_regression, targets):
        plan = self.plan(shape, targets, box_cls.device)
        A = int(self.cells.shape[1])
        C = box_cls.shape[1] // A
        cls_loss = self.cls_loss_func(box_cls.contiguous().view(shape.rows * A, C), plan.labels_i32) / (plan.n_pos + shape.n_images)
        reg_loss = ops.retina_smooth_l1_loss(box_regression, shape, self.strides, device_cells(self.cells, box_cls.device),
                                             plan.boxes, plan.labels_i32, plan.matched, self.beta)
        return cls_loss, reg_loss / max(1, plan.n_pos * self.regress_norm)


class RetinaNetPostProcessor:
    """reference rpn/retinanet/inference.py:59-174: per level the candidates sigmoid(cls) > INFERENCE_TH over (row, anchor,
    class), the top PRE_NMS_TOP_N of them per image, decoded against the candidate's anchor and clipped; over all levels
    per-class NMS at NMS_TH (one class-aware launch per image, ops.nms_by_label) and the DETECTIONS_PER_IMG cap by kthvalue.
    Batched like FCOSPostProcessor._select: one top-k per level over all images."""

    def __init__(self, pre_nms_thresh=0.05, pre_nms_top_n=1000, nms_thresh=0.4, fpn_post_nms_top_n=100, min_size=0,
                 num_classes=81, strides=ANCHOR_STRIDES, cells=None):
        self.pre_nms_thresh, self.pre_nms_top_n, self.nms_thresh = pre_nms_thresh, pre_nms_top_n, nms_thresh
        self.fpn_post_nms_top_n, self.min_size, self.num_classes = fpn_post_nms_top_n, min_size, num_classes
        self.strides = tuple(strides)
        self.cells = cell_anchors() if cells is None else cells

    def select(self, shape, box_cls, box_regression, image_sizes):
        """-> ok [N, K] bool, anchor index [N, K] (i = m * A + a), label [N, K], boxes [N, K, 4], scores [N, K]: the
        candidates of every level side by side, in (row, anchor, class) order within a level"""
        N, dev = shape.n_images, box_cls.device
        A = int(self.cells.shape[1])
        C = box_cls.shape[1] // A
        anchors = level_anchors(shape, device_cells(self.cells, dev), self.strides)
        prob = box_cls.sigmoid()
        score = torch.where(prob > self.pre_nms_thresh, prob, prob.new_full((), -1.0))
        s_val, s_cls, s_idx, s_anc, s_reg = [], [], [], [], []
        for l in range(shape.n_levels):
            r0, r1 = shape.row_off[l], shape.row_off[l + 1]
            hw = (r1 - r0) // N
            flat = score[r0:r1].reshape(N, hw * A * C)
            k = min(self.pre_nms_top_n, hw * A * C)
            val, idx = flat.topk(k, dim=1, sorted=False)
            idx, perm = torch.sort(torch.where(val > 0, idx, idx.new_full((), hw * A * C)), dim=1)
            val = val.gather(1, perm)
            loc = torch.div(idx, C, rounding_mode="floor").clamp(max=hw * A - 1)  # anchor within the image's level
            s_val.append(val)
            s_cls.append(idx % C + 1)
            glob = (r0 + torch.arange(N, device=dev)[:, None] * hw) * A + loc
            s_idx.append(glob)
            s_anc.append(anchors[l][loc])
            s_reg.append(box_regression[r0:r1].reshape(N, hw * A, 4).gather(1, loc[..., None].expand(-1, -1, 4)))
        val, lab, idx = torch.cat(s_val, 1), torch.cat(s_cls, 1), torch.cat(s_idx, 1)
        det = decode(torch.cat(s_reg, 1), torch.cat(s_anc, 1))
        lim = torch.tensor([[w - 1, h - 1, w - 1, h - 1] for h, w in image_sizes], dtype=det.dtype).to(dev)
        det = torch.minimum(det.clamp(min=0), lim[:, None, :])
        ws, hs = det[..., 2] - det[..., 0] + 1, det[..., 3] - det[..., 1] + 1
        ok = (val > 0) & (ws >= self.min_size) & (hs >= self.min_size)
        return ok, idx, lab, det, val

    def __call__(self, shape, box_cls, box_regression, image_sizes):
        """per image (boxes [k, 4], scores [k], labels [k]), class-major"""
        ok, _, lab, det, val = self.select(shape, box_cls, box_regression, image_sizes)
        results = []
        for i in range(shape.n_images):
            sel = torch.nonzero(ok[i]).squeeze(1)
            boxes, scores, labels = det[i][sel], val[i][sel], lab[i][sel]
            keep = ops.nms_by_label(boxes, scores, labels, self.nms_thresh).to(boxes.device)
            keep = keep[torch.argsort(labels[keep], stable=True)]
            rb, rs, rl = boxes[keep], scores[keep], labels[keep]
            n = len(rs)
            if n > self.fpn_post_nms_top_n > 0:
                th, _ = torch.kthvalue(rs, n - self.fpn_post_nms_top_n + 1)
                k = torch.nonzero(rs >= th).squeeze(1)
                rb, rs, rl = rb[k], rs[k], rl[k]
            results.append((rb, rs, rl))
        return results


class RetinaNetModule(nn.Module):
    """model["fcos"] with the RetinaNet head (reference retinanet.py:88-152).  cfg: a config.retinanet_settings dict (or None:
    DEFAULT_SETTINGS with ``num_classes``)."""

    def __init__(self, num_classes=None, cfg=None):
        super().__init__()
        c = dict(DEFAULT_SETTINGS)
        c.update(cfg or {})
        if num_classes is not None:
            c["num_classes"] = num_classes
        strides = tuple(c["anchor_strides"])
        A = len(c["aspect_ratios"]) * int(c["scales_per_octave"])
        if strides != ANCHOR_STRIDES:
            raise ValueError("MODEL.RETINANET.ANCHOR_STRIDES %r: the pyramid has strides %r" % (strides, ANCHOR_STRIDES))
        if len(c["anchor_sizes"]) != len(strides):
            raise ValueError("MODEL.RETINANET.ANCHOR_SIZES %r: one size per level" % (c["anchor_sizes"],))
        if not 1 <= A <= MAX_ANCHORS:
            raise ValueError("MODEL.RETINANET.ASPECT_RATIOS x SCALES_PER_OCTAVE = %d anchors: 1..%d are built" % (A, MAX_ANCHORS))
        if not 2 <= c["num_classes"] <= 32:
            raise ValueError("MODEL.RETINANET.NUM_CLASSES=%d (background included): 2..32 are built" % c["num_classes"])
        self.settings = c
        self.cells = cell_anchors(strides, c["anchor_sizes"], c["aspect_ratios"], c["octave"], c["scales_per_octave"])
        # the reference's anchor_generator.cell_anchors.<level> buffers, so that its checkpoints load key for key; the kernels
        # read self.cells, which the settings alone determine
        self.anchor_generator = nn.Module()
        self.anchor_generator.cell_anchors = nn.Module()
        for l, cell in enumerate(self.cells):
            self.anchor_generator.cell_anchors.register_buffer(str(l), cell.clone())
        self.head = RetinaNetHead(c["num_classes"], A, c["num_convs"], c["prior_prob"])
        self.loss_evaluator = RetinaNetLossComputation(c["loss_gamma"], c["loss_alpha"], c["bbox_reg_beta"], c["bbox_reg_weight"],
                                                       strides, self.cells, c["bg_iou_threshold"], c["fg_iou_threshold"])
        self.box_selector_test = RetinaNetPostProcessor(
            pre_nms_thresh=c["inference_th"], pre_nms_top_n=c["pre_nms_top_n"], nms_thresh=c["nms_th"],
            fpn_post_nms_top_n=c["detections_per_img"], min_size=0, num_classes=c["num_classes"], strides=strides, cells=self.cells)
        self.mode = "common"

    def forward(self, image_sizes, rows, shape, targets=None, act_maps=None):
        """as ATSSModule.forward; act_maps is accepted and ignored"""
        if self.training:
            if targets is None:
                return None, {"zero": rows.new_zeros(())}
            if rows.is_cuda:  # the plan's host read hides behind the head's convolutions
                self.loss_evaluator.plan(shape, targets, rows.device, side_stream=ops.borrow_side_streams(3)[0],
                                         after=fcos_mod._event_if_device(targets))
            logits, reg = self.head(rows, shape)
            lc, lr = self.loss_evaluator(shape, logits, reg, targets)
            return None, {"loss_retina_cls": lc, "loss_retina_reg": lr}
        logits, reg = self.head(rows, shape)
        return self.box_selector_test(shape, logits, reg, image_sizes), {}


def build_retinanet(cfg=None, num_classes=None):
    """reference rpn/rpn.py:201 build_rpn(cfg, in_channels) for RETINANET_ON; cfg: a config.retinanet_settings dict or None."""
    return RetinaNetModule(num_classes, cfg)

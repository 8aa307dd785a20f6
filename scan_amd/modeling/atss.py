"""ATSS head, ground-truth plan, loss and post-processor on pyramid activations.

Mirrors the reference's fcos_core/modeling/rpn/atss/{atss.py, loss.py, inference.py} for the configuration its yaml selects
(configs/epm/da_ga_sim10k_VGG_16_FPN_4x_atss.yaml): POSITIVE_TYPE 'ATSS', REGRESSION_TYPE 'BOX', one anchor per location.
With one anchor per location the anchors of a level are the rows of that level, so everything stays on [M, C] row matrices:
the anchor of row (level l, y, x) has centre (x * s + (s - 1) / 2, y * s + (s - 1) / 2) and corners centre -/+ (a - 1) / 2
(rpn/anchor_generator.py:168-188, 241-300 with ratio 1.0 and one scale) and is computed where it is needed, never stored.

The assignment (loss.py:159-218) -- with this project's tie rules where the reference leaves the choice to torch.topk /
torch.max -- is stated in csrc/atss.hip; ``assign_targets`` below is its torch spelling and the kernels are held equal to it.
"""
import math

import torch
from torch import nn

from .. import ops
from ..layers import SigmoidFocalLoss
from . import fcos as fcos_mod
from .fcos import FCOSHead, FCOSPostProcessor

ANCHOR_STRIDES = (8, 16, 32, 64, 128)
ANCHOR_SIZES = (64, 128, 256, 512, 1024)
BBOX_XFORM_CLIP = math.log(1000. / 16)  # atss.py:84-85
MAX_TOPK = 64  # ATSS_MAX_TOPK of csrc/atss.hip

# config.atss_settings(cfg) keys with the reference's defaults (config/defaults.py:287-333)
DEFAULT_SETTINGS = dict(num_classes=81, anchor_sizes=ANCHOR_SIZES, anchor_strides=ANCHOR_STRIDES, num_convs=4,
                        dcn_in_tower=False, loss_alpha=0.25, loss_gamma=5.0, topk=9, reg_loss_weight=2.0, prior_prob=0.01,
                        inference_th=0.05, nms_th=0.6, pre_nms_top_n=1000, detections_per_img=100)


def level_anchors(shape, device, strides=ANCHOR_STRIDES, sizes=ANCHOR_SIZES):
    """per level the anchors [h * w, 4] xyxy of one image, x fastest"""
    out = []
    for (h, w), s, a in zip(shape.sizes, strides, sizes):
        xs = torch.arange(0, w * s, step=s, dtype=torch.float32, device=device) + (s - 1) / 2
        ys = torch.arange(0, h * s, step=s, dtype=torch.float32, device=device) + (s - 1) / 2
        cy, cx = torch.meshgrid(ys, xs, indexing="ij")
        cx, cy, half = cx.reshape(-1), cy.reshape(-1), (a - 1) / 2
        out.append(torch.stack((cx - half, cy - half, cx + half, cy + half), dim=1))
    return out


def row_anchors(shape, device, strides=ANCHOR_STRIDES, sizes=ANCHOR_SIZES):
    """the anchors of all pyramid rows [M, 4] (level-major, image, y, x)"""
    return torch.cat([a.repeat(shape.n_images, 1) for a in level_anchors(shape, device, strides, sizes)], 0)


def encode(gt, anchors):
    """BoxCoder.encode, REGRESSION_TYPE 'BOX' (atss.py:33-50)"""
    ew = anchors[:, 2] - anchors[:, 0] + 1
    eh = anchors[:, 3] - anchors[:, 1] + 1
    ecx = (anchors[:, 2] + anchors[:, 0]) / 2
    ecy = (anchors[:, 3] + anchors[:, 1]) / 2
    gw = gt[:, 2] - gt[:, 0] + 1
    gh = gt[:, 3] - gt[:, 1] + 1
    gcx = (gt[:, 2] + gt[:, 0]) / 2
    gcy = (gt[:, 3] + gt[:, 1]) / 2
    return torch.stack((10. * (gcx - ecx) / ew, 10. * (gcy - ecy) / eh, 5. * torch.log(gw / ew), 5. * torch.log(gh / eh)), dim=1)


def decode(deltas, anchors):
    """BoxCoder.decode, REGRESSION_TYPE 'BOX' (atss.py:68-97); deltas / anchors [..., 4]"""
    w = anchors[..., 2] - anchors[..., 0] + 1
    h = anchors[..., 3] - anchors[..., 1] + 1
    cx = (anchors[..., 2] + anchors[..., 0]) / 2
    cy = (anchors[..., 3] + anchors[..., 1]) / 2
    dw = torch.clamp(deltas[..., 2] / 5., max=BBOX_XFORM_CLIP)
    dh = torch.clamp(deltas[..., 3] / 5., max=BBOX_XFORM_CLIP)
    pcx = deltas[..., 0] / 10. * w + cx
    pcy = deltas[..., 1] / 10. * h + cy
    pw = torch.exp(dw) * w
    ph = torch.exp(dh) * h
    return torch.stack((pcx - 0.5 * (pw - 1), pcy - 0.5 * (ph - 1), pcx + 0.5 * (pw - 1), pcy + 0.5 * (ph - 1)), dim=-1)


def centerness_targets(reg, anchors):
    """reference loss.py:360-373: centerness of decode(reg) against the anchor centre"""
    gts = decode(reg, anchors)
    cx = (anchors[:, 2] + anchors[:, 0]) / 2
    cy = (anchors[:, 3] + anchors[:, 1]) / 2
    lr = torch.stack([cx - gts[:, 0], gts[:, 2] - cx], dim=1)
    tb = torch.stack([cy - gts[:, 1], gts[:, 3] - cy], dim=1)
    return torch.sqrt((lr.min(dim=-1)[0] / lr.max(dim=-1)[0]) * (tb.min(dim=-1)[0] / tb.max(dim=-1)[0]))


def assign_targets(shape, targets, device, strides=ANCHOR_STRIDES, sizes=ANCHOR_SIZES, topk=9):
    """The ATSS assignment (the definition in csrc/atss.hip, reference loss.py:159-218) in torch: labels [M] int64 and matched
    box index [M] int32 (0 where background) in pyramid row order.  Ties as the kernels break them: a stable sort puts equal
    distances in row order, and the contested-anchor vote is the same integer max of (IoU bits << 32) | ~g."""
    N, M = shape.n_images, shape.rows
    labels = torch.zeros((M,), dtype=torch.int64, device=device)
    matched = torch.zeros((M,), dtype=torch.int32, device=device)
    anchors = level_anchors(shape, device, strides, sizes)
    for n, (boxes, lab) in enumerate(targets):
        G = int(boxes.shape[0])
        if G == 0:
            continue
        boxes = boxes.to(device=device, dtype=torch.float32)
        lab = lab.to(device=device, dtype=torch.int64)
        gcx = (boxes[:, 2] + boxes[:, 0]) / 2.0
        gcy = (boxes[:, 3] + boxes[:, 1]) / 2.0
        area_g = (boxes[:, 2] - boxes[:, 0] + 1) * (boxes[:, 3] - boxes[:, 1] + 1)
        c_row, c_iou, c_in = [], [], []
        for l, a in enumerate(anchors):
            hw = a.shape[0]
            acx = (a[:, 2] + a[:, 0]) / 2.0
            acy = (a[:, 3] + a[:, 1]) / 2.0
            dx = acx[:, None] - gcx[None]
            dy = acy[:, None] - gcy[None]
            dist = (dx * dx + dy * dy).sqrt()
            idx = torch.sort(dist, dim=0, stable=True)[1][:min(topk, hw)]  # [k, G]
            ca = a[idx]  # [k, G, 4]
            area_a = (ca[..., 2] - ca[..., 0] + 1) * (ca[..., 3] - ca[..., 1] + 1)
            iw = (torch.min(ca[..., 2], boxes[None, :, 2]) - torch.max(ca[..., 0], boxes[None, :, 0]) + 1).clamp(min=0)
            ih = (torch.min(ca[..., 3], boxes[None, :, 3]) - torch.max(ca[..., 1], boxes[None, :, 1]) + 1).clamp(min=0)
            inter = iw * ih
            c_iou.append(inter / (area_a + area_g[None] - inter))
            ccx, ccy = acx[idx], acy[idx]
            ltrb = torch.stack([ccx - boxes[None, :, 0], ccy - boxes[None, :, 1], boxes[None, :, 2] - ccx,
                                boxes[None, :, 3] - ccy], dim=0)
            c_in.append(ltrb.min(dim=0)[0] > 0.01)
            c_row.append(shape.row_off[l] + n * hw + idx)
        c_row, c_iou, c_in = torch.cat(c_row, 0), torch.cat(c_iou, 0), torch.cat(c_in, 0)  # [K, G]
        iou64 = c_iou.double()
        thr = (iou64.mean(0) + iou64.std(0)).float()  # fp64 sums, one rounding; one candidate: NaN, no positives
        pos = (c_iou >= thr[None]) & c_in
        g_idx = torch.arange(G, device=device, dtype=torch.int64)[None].expand_as(c_row)
        key = (c_iou.view(torch.int32).to(torch.int64) << 32) | (0xffffffff - g_idx)
        row_key = torch.zeros((M,), dtype=torch.int64, device=device)
        row_key.scatter_reduce_(0, c_row[pos], key[pos], "amax")
        hit = row_key != 0
        g_of = (0xffffffff - (row_key & 0xffffffff)).clamp(max=G - 1)
        labels = torch.where(hit, lab[g_of], labels)
        matched = torch.where(hit, g_of.to(torch.int32), matched)
    matched = torch.where(labels > 0, matched, torch.zeros_like(matched))
    return labels, matched


class ATSSTargetPlan:
    """What the ATSS losses derive from the ground truth alone: labels (and the int32 copy the focal kernel takes), the matched
    box of every row, the positive rows with their encoded regression targets and centerness targets.  Built once per batch
    (fcos.target_plan's cache and side-stream protocol)."""
    __slots__ = ("key", "targets", "labels", "labels_i32", "matched", "pos_inds", "n_pos", "reg_pos", "ctr_pos", "ready")


_plan = [None]
fcos_mod._plan_caches.append(_plan)
DEVICE_PLAN = True  # False: the torch spelling also on the GPU (cross-checks)
plan_stats = {"launches": 0, "host_reads": 0}  # of the most recent device plan (tools/atss_bench.py records them)


def _check_geometry(shape, strides, sizes, topk):
    if not (len(strides) == len(sizes) == shape.n_levels):
        raise ValueError("ATSS: %d ANCHOR_STRIDES / %d ANCHOR_SIZES for a pyramid of %d levels"
                         % (len(strides), len(sizes), shape.n_levels))
    if not 1 <= topk <= MAX_TOPK:
        raise ValueError("MODEL.ATSS.TOPK=%d: the kernels are built for 1..%d" % (topk, MAX_TOPK))


def _build_plan_device(shape, targets, device, strides, sizes, topk):
    """csrc/atss.hip: two memsets and five launches (candidates, vote, labels, scan_fcos_compact, targets) whatever N, G and the
    level count are, and ONE host read (the per-level positive counts)."""
    p = ATSSTargetPlan()
    p.ready = None
    boxes, glab, ng, _ = fcos_mod.upload_ground_truth(shape.n_images, targets, device)
    p.labels, p.labels_i32, p.matched, level_pos, pos_list, _ = ops.atss_assign(shape, strides, sizes, topk, boxes, glab, ng)
    counts = level_pos[:shape.n_levels].tolist()  # the one host round trip of the plan
    p.n_pos = int(sum(counts))
    p.pos_inds, p.reg_pos, p.ctr_pos = ops.atss_targets(shape, strides, sizes, counts, boxes, p.matched, pos_list)
    plan_stats.update(launches=4 + (1 if p.n_pos else 0), host_reads=1)
    return p


def build_plan(shape, targets, device, strides=ANCHOR_STRIDES, sizes=ANCHOR_SIZES, topk=9):
    _check_geometry(shape, strides, sizes, topk)
    if DEVICE_PLAN and device.type == "cuda" and targets:
        return _build_plan_device(shape, targets, device, strides, sizes, topk)
    p = ATSSTargetPlan()
    p.ready = None
    p.labels, p.matched = assign_targets(shape, targets, device, strides, sizes, topk)
    p.labels_i32 = p.labels.int()
    p.pos_inds = torch.nonzero(p.labels > 0).squeeze(1)
    p.n_pos = p.pos_inds.numel()
    hw = torch.tensor([h * w for h, w in shape.sizes], device=device)
    off = torch.tensor(shape.row_off[:-1], device=device)
    lvl = torch.bucketize(p.pos_inds, torch.tensor(shape.row_off[1:], device=device), right=True)
    img = torch.div(p.pos_inds - off[lvl], hw[lvl], rounding_mode="floor")
    boxes = fcos_mod.pack_boxes(shape.n_images, targets, device)
    # targets in fp64, rounded once (as the kernel forms them: see scan_atss_targets in csrc/atss.hip)
    anchors = row_anchors(shape, device, strides, sizes)[p.pos_inds].double()
    reg = encode(boxes[img, p.matched[p.pos_inds].long()].double(), anchors)
    p.reg_pos, p.ctr_pos = reg.float(), centerness_targets(reg, anchors).float()
    return p


def target_plan(shape, targets, device, strides=ANCHOR_STRIDES, sizes=ANCHOR_SIZES, topk=9, side_stream=None, after=None):
    """The ATSSTargetPlan of (shape, targets), cached for the current batch; with ``side_stream`` built there."""
    return fcos_mod.target_plan(shape, targets, device, side_stream=side_stream, after=after, cache=_plan,
                                build=lambda sh, tg, dev: build_plan(sh, tg, dev, strides, sizes, topk))


class ATSSHead(FCOSHead):
    """reference atss.py:100-191 with one anchor per location and REGRESSION_TYPE 'BOX': the FCOS head's modules under the same
    names (cls_tower.N, bbox_tower.N, cls_logits, bbox_pred, centerness, scales.L.scale), same initialisation (normal std 0.01,
    PRIOR_PROB bias on cls_logits); bbox_reg = scale_l * bbox_pred, no exp."""
    exp_reg = False

    def __init__(self, num_classes=81, num_convs=4, prior_prob=0.01, use_dcn_in_tower=False):
        super().__init__(num_classes, num_convs, prior_prob, use_dcn_in_tower)


class ATSSLossComputation:
    """reference loss.py:374-403 on one rank: focal sum / max(n_pos, 1), REG_LOSS_WEIGHT * GIoU sum / sum of the centerness
    targets, centerness BCE sum / max(n_pos, 1); without positives the two .sum() fallbacks."""

    def __init__(self, gamma=5.0, alpha=0.25, reg_loss_weight=2.0, strides=ANCHOR_STRIDES, sizes=ANCHOR_SIZES, topk=9):
        self.cls_loss_func = SigmoidFocalLoss(gamma, alpha)
        self.reg_loss_weight = reg_loss_weight
        self.strides, self.sizes, self.topk = tuple(strides), tuple(sizes), int(topk)

    def plan(self, shape, targets, device, side_stream=None, after=None):
        return target_plan(shape, targets, device, self.strides, self.sizes, self.topk, side_stream, after)

    def __call__(self, shape, box_cls, box_regression, centerness, targets):
        plan = self.plan(shape, targets, box_cls.device)
        cls_loss = self.cls_loss_func(box_cls.contiguous(), plan.labels_i32) / max(plan.n_pos, 1)
        box_regression = box_regression[plan.pos_inds]
        centerness = centerness[plan.pos_inds]
        if plan.n_pos > 0:
            reg_loss = ops.atss_giou_loss(box_regression, plan.reg_pos, plan.pos_inds, plan.ctr_pos, shape, self.strides,
                                          self.sizes)
            ctr_loss = ops.bce_with_logits_mean(centerness, plan.ctr_pos)  # sum / n_pos
        else:
            reg_loss = box_regression.sum()
            ctr_loss = centerness.sum()
        return cls_loss, reg_loss * self.reg_loss_weight, ctr_loss


class ATSSPostProcessor(FCOSPostProcessor):
    """reference inference.py:11-124: the FCOS selection (threshold on the class probability, ranking by probability x
    centerness, scores = the square root, per-class NMS on the device) with boxes = BoxCoder.decode(deltas, anchor of the row).
    Plain logits only."""

    def __init__(self, pre_nms_thresh=0.05, pre_nms_top_n=1000, nms_thresh=0.6, fpn_post_nms_top_n=100, min_size=0,
                 num_classes=81, strides=ANCHOR_STRIDES, sizes=ANCHOR_SIZES):
        super().__init__(pre_nms_thresh, pre_nms_top_n, nms_thresh, fpn_post_nms_top_n, min_size, num_classes, mode="common")
        self.strides, self.sizes = tuple(strides), tuple(sizes)

    def _level_points(self, shape, dev):
        return level_anchors(shape, dev, self.strides, self.sizes)

    def _decode(self, anchors, deltas):
        return decode(deltas, anchors)


class ATSSModule(nn.Module):
    """model["fcos"] with the ATSS head (reference atss.py:194-270; the reference keeps that dictionary key whichever head
    build_rpn returns).  cfg: a config.atss_settings dict (or None: DEFAULT_SETTINGS with ``num_classes``)."""

    def __init__(self, num_classes=None, cfg=None):
        super().__init__()
        c = dict(DEFAULT_SETTINGS)
        c.update(cfg or {})
        if num_classes is not None:
            c["num_classes"] = num_classes
        strides, sizes = tuple(c["anchor_strides"]), tuple(c["anchor_sizes"])
        if strides != ANCHOR_STRIDES:
            raise ValueError("MODEL.ATSS.ANCHOR_STRIDES %r: the pyramid has strides %r" % (strides, ANCHOR_STRIDES))
        if len(sizes) != len(strides) or any(a < 1 for a in sizes):
            raise ValueError("MODEL.ATSS.ANCHOR_SIZES %r: one size >= 1 per level" % (sizes,))
        if not 1 <= int(c["topk"]) <= MAX_TOPK:
            raise ValueError("MODEL.ATSS.TOPK=%r: the kernels are built for 1..%d" % (c["topk"], MAX_TOPK))
        if not 2 <= c["num_classes"] <= 32:
            raise ValueError("MODEL.ATSS.NUM_CLASSES=%d (background included): 2..32 are built" % c["num_classes"])
        self.settings = c
        self.head = ATSSHead(c["num_classes"], c["num_convs"], c["prior_prob"], use_dcn_in_tower=bool(c["dcn_in_tower"]))
        self.loss_evaluator = ATSSLossComputation(c["loss_gamma"], c["loss_alpha"], c["reg_loss_weight"], strides, sizes,
                                                  c["topk"])
        self.box_selector_test = ATSSPostProcessor(
            pre_nms_thresh=c["inference_th"], pre_nms_top_n=c["pre_nms_top_n"], nms_thresh=c["nms_th"],
            fpn_post_nms_top_n=c["detections_per_img"], min_size=0, num_classes=c["num_classes"], strides=strides, sizes=sizes)
        self.mode = "common"

    def forward(self, image_sizes, rows, shape, targets=None, act_maps=None):
        """as FCOSModule.forward; act_maps is accepted and ignored (the ATSS head scores with its own logits only)"""
        if self.training:
            if targets is None:
                return None, {"zero": rows.new_zeros(())}
            if rows.is_cuda:  # the plan's host read hides behind the head's convolutions
                self.loss_evaluator.plan(shape, targets, rows.device, side_stream=ops.borrow_side_streams(3)[0],
                                         after=fcos_mod._event_if_device(targets))
            logits, reg, ctr = self.head(rows, shape)
            lc, lr, lctr = self.loss_evaluator(shape, logits, reg, ctr, targets)
            return None, {"loss_cls": lc, "loss_reg": lr, "loss_centerness": lctr}
        logits, reg, ctr = self.head(rows, shape)
        return self.box_selector_test(shape, logits, reg, ctr, image_sizes), {}


def build_atss(cfg=None, num_classes=None):
    """reference rpn/rpn.py:201 build_rpn(cfg, in_channels) for ATSS_ON; cfg: a config.atss_settings dict or None."""
    return ATSSModule(num_classes, cfg)

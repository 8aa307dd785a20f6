"""Fast R-CNN box head on pyramid activations: feature extractor, predictor, sampling loss, post-processor and module.

Mirrors the reference's fcos_core/modeling/roi_heads/box_head/{box_head.py, loss.py, inference.py, roi_box_feature_extractors.py,
roi_box_predictors.py} and roi_heads/roi_heads.py for the FPN spelling (FPN2MLPFeatureExtractor + FPNPredictor), with
modeling/matcher.py (no low-quality rule), modeling/balanced_positive_negative_sampler.py and modeling/box_coder.py.

Per training step, all on the device (csrc/roi_box.hip): the proposals of the batch are padded to [N, P, 4] as the ground truth
is; ONE launch matches them (ops.roi_box_match), ONE launch samples (ops.rpn_sample on a one-level P x 1 pyramid with A = 1),
ONE host read fetches the per-image counts, and ONE launch gathers the sampled proposals with their labels and encoded targets in
the reference's order (ops.roi_box_gather).  The loss is one fused launch over the sampled rows (ops.roi_box_loss), one more for
its backward.  As in modeling/rpn.py the sampler is a keyed selection -- the same distribution of samples as the reference's
nonzero + randperm, not the same samples -- so ``subsample`` takes a ``sampled=`` override through which the tests feed the
reference's own masks.

At test time one launch forms the softmax, decodes every (ROI, class) box, clips it and applies the score threshold
(ops.roi_box_decode); per image one ops.nms_by_label launch with the class as the label replaces the reference's loop over
classes, then the kthvalue cap.

The linear layers (fc6, fc7, cls_score + bbox_pred) are nn.Linear-shaped parameters under the reference's names, run as 1x1
convolutions through ops.conv2d on a one-level pyramid of R x 1 rows: the CONV_MODE arithmetic of every other layer.
"""
import torch
from torch import nn

from .. import config, ops
from ..structures import BoxList
from . import fcos as fcos_mod
from . import rpn as rpn_mod
from .poolers import Pooler

plan_stats = {"launches": 0, "host_reads": 0}  # what the Python side ISSUED for the most recent subsample (counted here, not observed)


def _default_cfg():
    return config.roi_box_settings(config.Cfg({"MODEL": {
        "ROI_HEADS": {"USE_FPN": True},
        "ROI_BOX_HEAD": {"FEATURE_EXTRACTOR": "FPN2MLPFeatureExtractor", "PREDICTOR": "FPNPredictor", "POOLER_RESOLUTION": 7,
                         "POOLER_SCALES": (0.125, 0.0625, 0.03125, 0.015625), "POOLER_SAMPLING_RATIO": 2}}}))


# config.roi_box_settings of the reference's Faster R-CNN FPN yamls' ROI_HEADS / ROI_BOX_HEAD blocks (e2e_faster_rcnn_R_50_FPN_1x)
DEFAULT_SETTINGS = _default_cfg()


def linear_rows(x, weight, bias, relu=False):
    """y [R, pad4(D)] = x [R, K] @ weight[D, K]^T + bias (+ ReLU) as a 1x1 convolution on the one-level pyramid of R x 1 rows;
    K a multiple of 4, x contiguous.  Columns D.. of y are zero."""
    R, K = x.shape
    D = weight.shape[0]
    if weight.shape[1] != K or K % 4:
        raise ValueError("linear_rows: x %r for a weight %r (K must match and be a multiple of 4)" % (tuple(x.shape), tuple(weight.shape)))
    if R == 0:  # nothing to launch; the empty result still reaches every parameter
        return x.new_zeros((0, ops.pad4(D))) + (weight[:1, :1].sum() + bias[:1].sum() + x.sum()) * 0
    return ops.conv2d(x, weight.reshape(D, K, 1, 1), bias, ops.PyramidShape(1, [(R, 1)]), 1, 1, relu=relu)


def rois_of(boxlists):
    """list[BoxList] -> [R, 5] fp32 (image index, xyxy box), the images in order"""
    parts = []
    for i, b in enumerate(boxlists):
        box = b.convert("xyxy").bbox.float().reshape(-1, 4)
        parts.append(torch.cat((torch.full((box.shape[0], 1), float(i), dtype=torch.float32, device=box.device), box), 1))
    return torch.cat(parts, 0).contiguous()


# ----------------------------------------------------------------------------- feature extractor and predictor
class FPN2MLPFeatureExtractor(nn.Module):
    """reference roi_box_feature_extractors.py:49-81: pooler, fc6, fc7 (make_fc: kaiming_uniform_(a=1), zero bias).  fc6.weight
    keeps the reference's [D, C * PH * PW] channel-major columns; the pooled rows are (PH, PW, Cs) channel-last, so the columns
    are permuted at call time, under autograd."""

    def __init__(self, in_channels=256, resolution=7, scales=(0.125, 0.0625, 0.03125, 0.015625), sampling_ratio=2,
                 representation_size=1024):
        super().__init__()
        self.in_channels, self.resolution = int(in_channels), int(resolution)
        self.pooler = Pooler(output_size=(resolution, resolution), scales=scales, sampling_ratio=sampling_ratio)
        self.fc6 = nn.Linear(in_channels * resolution ** 2, representation_size)
        self.fc7 = nn.Linear(representation_size, representation_size)
        for fc in (self.fc6, self.fc7):
            nn.init.kaiming_uniform_(fc.weight, a=1)
            nn.init.constant_(fc.bias, 0)
        self.out_channels = representation_size

    def pooled_rows(self, x, rois):
        """x: the pyramid's levels (a PyramidLevels is taken as the rows it is; any other list is packed) -> [R, PH, PW, Cs]
        channel-last.  Only the first len(POOLER_SCALES) levels are pooled (the reference's zip(x, self.poolers))."""
        p = self.pooler
        k = len(p.scales)
        if len(x) < k:
            raise RuntimeError("FPN2MLPFeatureExtractor: %d feature levels for %d pooler scales" % (len(x), k))
        if isinstance(x, ops.PyramidLevels) and len(x) > k:
            rows, shape = ops.pack_levels(x)
            rows, shape = rows[:shape.row_off[k]], ops.PyramidShape(shape.n_images, shape.sizes[:k])  # level-major: a prefix
        else:
            rows, shape = ops.pack_levels(x if len(x) == k else list(x)[:k])
        levels = None
        if k > 1:
            m = p.map_levels
            levels = ops.roi_levels(rois, m.k_min, m.k_max, m.s0, m.lvl0, m.eps)
        return ops.roi_align(rows, shape, rois, p.output_size, p.scales, p.sampling_ratio, levels=levels, c=x[0].shape[1])

    def fc6_weight_rows(self, cs):
        """fc6.weight [D, C * PH * PW] -> [D, PH * PW * Cs]: the column order of the pooled rows"""
        D, C, r = self.fc6.weight.shape[0], self.in_channels, self.resolution
        w = self.fc6.weight.view(D, C, r, r).permute(0, 2, 3, 1)
        if cs != C:
            w = nn.functional.pad(w, (0, cs - C))
        return w.reshape(D, r * r * cs)

    def forward(self, x, rois):
        """rois: [R, 5] (image index, box) or list[BoxList] -> [R, representation_size]"""
        if not torch.is_tensor(rois):
            rois = rois_of(rois)
        if x[0].shape[1] != self.in_channels:
            raise RuntimeError("FPN2MLPFeatureExtractor: %d feature channels, built for %d" % (x[0].shape[1], self.in_channels))
        y = self.pooled_rows(x, rois)
        return self.mlp(y.reshape(y.shape[0], -1), y.shape[3])

    def mlp(self, flat, cs):
        """flat [R, PH * PW * Cs] pooled rows -> relu(fc7(relu(fc6)))"""
        h = linear_rows(flat, self.fc6_weight_rows(cs), self.fc6.bias, relu=True)
        D = self.out_channels
        if h.shape[1] != D:
            h = h[:, :D].contiguous()
        return linear_rows(h, self.fc7.weight, self.fc7.bias, relu=True)[:, :D]


class FPNPredictor(nn.Module):
    """reference roi_box_predictors.py:34-58: cls_score (std 0.01) and bbox_pred (std 0.001), zero biases.  The two layers run as
    ONE launch over their stacked weights (bbox_pred first, so that its columns start 16-byte aligned, as RPNHead does); the
    outputs are column slices of that launch's rows, which the loss and the decode read in place through the pitch."""

    def __init__(self, in_channels=1024, num_classes=81, cls_agnostic_bbox_reg=False):
        super().__init__()
        self.num_classes = int(num_classes)
        self.num_bbox_reg_classes = 2 if cls_agnostic_bbox_reg else self.num_classes
        self.cls_score = nn.Linear(in_channels, self.num_classes)
        self.bbox_pred = nn.Linear(in_channels, self.num_bbox_reg_classes * 4)
        nn.init.normal_(self.bbox_pred.weight, std=0.001)
        nn.init.normal_(self.cls_score.weight, std=0.01)
        for l in (self.cls_score, self.bbox_pred):
            nn.init.constant_(l.bias, 0)

    def forward(self, x):
        """x [R, in_channels] -> class_logits [R, C], box_regression [R, 4 Cr]"""
        if x.dim() == 4:
            x = x.reshape(x.shape[0], -1)
        if not x.is_contiguous():
            x = x.contiguous()
        nr = 4 * self.num_bbox_reg_classes
        w = torch.cat((self.bbox_pred.weight, self.cls_score.weight), 0)
        b = torch.cat((self.bbox_pred.bias, self.cls_score.bias), 0)
        y = linear_rows(x, w, b)
        return y[:, nr:nr + self.num_classes], y[:, :nr]


# ----------------------------------------------------------------------------- loss
class FastRCNNLossComputation:
    """reference roi_heads/box_head/loss.py:15-167 on one rank.  ``seed`` keys the sampler as in RPNLossComputation: every
    subsample advances a counter that is mixed into it."""

    def __init__(self, bg=0.5, fg=0.5, batch_size_per_image=512, positive_fraction=0.25, weights=(10., 10., 5., 5.),
                 cls_agnostic=False, seed=0):
        if float(bg) > float(fg):
            raise ValueError("FastRCNNLossComputation: bg %r above fg %r" % (bg, fg))
        self.bg, self.fg = float(bg), float(fg)
        self.batch_size_per_image, self.positive_fraction = int(batch_size_per_image), float(positive_fraction)
        self.weights = tuple(float(w) for w in weights)
        self.cls_agnostic = bool(cls_agnostic)
        self.seed, self.calls = int(seed), 0
        self.rois = self.labels = self.reg_targets = self.src = self.matched = self.padded = None
        self.n_positive = 0

    next_seed = rpn_mod.RPNLossComputation.next_seed

    def subsample(self, proposals, targets, sampled=None):
        """proposals list[BoxList], targets [(boxes [g, 4], labels [g])] or list[BoxList] per image -> the sampled proposals per
        image as BoxLists with ``labels`` (int64), ``regression_targets`` and, if the proposals carry it, ``objectness``.  The
        flat rois [R, 5] / labels int32 [R] / reg_targets [R, 4] / src stay on the evaluator for the pooler and the loss.
        sampled (uint8 [N, P], 1 positive / 2 negative / 0): use this sample instead of drawing one."""
        N = len(proposals)
        if N < 1 or len(targets) != N:
            raise ValueError("FastRCNNLossComputation: %d proposal lists for %d targets" % (N, len(targets)))
        if isinstance(targets[0], BoxList):
            targets = [(t.convert("xyxy").bbox, t.get_field("labels")) for t in targets]
        dev = proposals[0].bbox.device
        counts_p = [len(p) for p in proposals]
        P = max(1, max(counts_p))
        props = torch.zeros((N, P, 4), dtype=torch.float32, device=dev)
        for n, p in enumerate(proposals):
            if counts_p[n]:
                props[n, :counts_p[n]] = p.convert("xyxy").bbox.float()
        n_props = torch.tensor(counts_p, dtype=torch.int32).to(dev)
        boxes, glab, ng, _ = fcos_mod.upload_ground_truth(N, targets, dev)
        labels, matched = ops.roi_box_match(props, n_props, boxes, glab, ng, self.bg, self.fg)
        launches = 1
        if sampled is None:
            sampled, counts = ops.rpn_sample(ops.PyramidShape(N, [(P, 1)]), 1, labels, self.batch_size_per_image,
                                             self.positive_fraction, self.next_seed())
            launches += 1
        else:
            sampled = sampled.to(device=dev, dtype=torch.uint8).reshape(N, P).contiguous()
            counts = torch.stack(((sampled == 1).sum(1), (sampled == 2).sum(1)), 1).to(torch.int32).contiguous()
            sampled = sampled.reshape(-1)
        counts_h = counts.tolist()  # the one host round trip
        per_image = [int(c[0]) + int(c[1]) for c in counts_h]
        R = int(sum(per_image))
        # what the mask head's plan reads (modeling/roi_mask_head.py): the match of every padded proposal and the sampled positives
        self.matched, self.padded, self.n_positive = matched, (N, P), sum(int(c[0]) for c in counts_h)
        self.rois, self.labels, self.reg_targets, self.src = ops.roi_box_gather(props, boxes, labels, matched, sampled, counts, R,
                                                                                 self.weights)
        plan_stats.update(launches=launches + 1, host_reads=1)
        out, r0 = [], 0
        for n, p in enumerate(proposals):
            r1 = r0 + int(per_image[n])
            bl = BoxList(self.rois[r0:r1, 1:], p.size, mode="xyxy")
            if p.has_field("objectness"):
                bl.add_field("objectness", p.get_field("objectness")[self.src[r0:r1].long()])
            bl.add_field("labels", self.labels[r0:r1].long())
            bl.add_field("regression_targets", self.reg_targets[r0:r1])
            out.append(bl)
            r0 = r1
        self._proposals = out
        return out

    def __call__(self, class_logits, box_regression):
        """class_logits [R, C], box_regression [R, 4 C] or [R, 8] (or one-element lists of them; column slices are read in
        place) -> (loss_classifier, loss_box_reg), both divided by R"""
        if self.rois is None:
            raise RuntimeError("subsample needs to be called before")
        if isinstance(class_logits, (list, tuple)):
            class_logits = class_logits[0] if len(class_logits) == 1 else torch.cat(list(class_logits), 0)
        if isinstance(box_regression, (list, tuple)):
            box_regression = box_regression[0] if len(box_regression) == 1 else torch.cat(list(box_regression), 0)
        want = 8 if self.cls_agnostic else 4 * class_logits.shape[1]
        if box_regression.shape[1] != want:
            raise ValueError("FastRCNNLossComputation: box_regression has %d columns, %d expected (cls_agnostic=%s)"
                             % (box_regression.shape[1], want, self.cls_agnostic))
        out = ops.roi_box_loss(class_logits, box_regression, self.labels, self.reg_targets)
        out = out / max(int(self.labels.shape[0]), 1)  # no sampled row: both losses 0
        return out[0], out[1]


# ----------------------------------------------------------------------------- post-processor
class PostProcessor(nn.Module):
    """reference roi_heads/box_head/inference.py:12-146.  The detections of an image come out in the reference's order: class
    ascending and, within a class, in the order of the ROIs (the reference's nms returns the kept indices sorted)."""

    def __init__(self, score_thresh=0.05, nms=0.5, detections_per_img=100, weights=(10., 10., 5., 5.), cls_agnostic=False):
        super().__init__()
        self.score_thresh, self.nms, self.detections_per_img = float(score_thresh), float(nms), int(detections_per_img)
        self.weights = tuple(float(w) for w in weights)
        self.cls_agnostic = bool(cls_agnostic)

    def forward(self, x, boxes):
        """x = (class_logits [R, C], box_regression), boxes list[BoxList] (R boxes in all) -> list[BoxList] with fields
        ``scores`` and ``labels``, clipped to the image, empty boxes kept"""
        class_logits, box_regression = x
        dev = class_logits.device
        rois = rois_of(boxes)
        hw = rpn_mod.device_image_hw([(b.size[1], b.size[0]) for b in boxes], dev)
        scores, dec, cand = ops.roi_box_decode(class_logits, box_regression, rois, hw, self.weights, self.score_thresh)
        out, r0 = [], 0
        for b in boxes:
            r1 = r0 + len(b)
            cls, row = torch.nonzero(cand[r0:r1].t(), as_tuple=True)  # class-major, the ROIs in order within a class
            bx, sc = dec[r0:r1][row, cls], scores[r0:r1][row, cls]
            kept = ops.nms_by_label(bx, sc, cls, self.nms).to(dev)  # ascending: the same order
            bx, sc, cls = bx[kept], sc[kept], cls[kept]
            n = int(sc.shape[0])
            if n > self.detections_per_img > 0:
                kth = torch.kthvalue(sc, n - self.detections_per_img + 1)[0]
                keep = torch.nonzero(sc >= kth).squeeze(1)  # ties at the k-th score all stay
                bx, sc, cls = bx[keep], sc[keep], cls[keep]
            res = BoxList(bx, b.size, mode="xyxy")
            res.add_field("scores", sc)
            res.add_field("labels", cls.to(torch.int64))
            out.append(res)
            r0 = r1
        return out


# ----------------------------------------------------------------------------- modules
class ROIBoxHead(nn.Module):
    """reference box_head.py:11-62.  cfg: a config.roi_box_settings dict (or None: DEFAULT_SETTINGS)."""

    def __init__(self, cfg=None, in_channels=256, seed=0):
        super().__init__()
        c = dict(DEFAULT_SETTINGS)
        c.update(cfg or {})
        self.settings = c
        self.feature_extractor = FPN2MLPFeatureExtractor(in_channels, c["pooler_resolution"], c["pooler_scales"],
                                                         c["pooler_sampling_ratio"], c["mlp_head_dim"])
        self.predictor = FPNPredictor(self.feature_extractor.out_channels, c["num_classes"], c["cls_agnostic_bbox_reg"])
        self.post_processor = PostProcessor(c["score_thresh"], c["nms"], c["detections_per_img"], c["bbox_reg_weights"],
                                            c["cls_agnostic_bbox_reg"])
        self.loss_evaluator = FastRCNNLossComputation(c["bg_iou_threshold"], c["fg_iou_threshold"], c["batch_size_per_image"],
                                                      c["positive_fraction"], c["bbox_reg_weights"], c["cls_agnostic_bbox_reg"],
                                                      seed=seed)

    def forward(self, features, proposals, targets=None, sampled=None):
        """features: the pyramid's levels, proposals list[BoxList], targets per image -> (x, proposals | detections, losses):
        training returns the subsampled proposals and {"loss_classifier", "loss_box_reg"}, eval the detections and {}"""
        if self.training:
            if targets is None:
                raise ValueError("ROIBoxHead: training needs targets")
            with torch.no_grad():
                proposals = self.loss_evaluator.subsample(proposals, targets, sampled=sampled)
            rois = self.loss_evaluator.rois
        else:
            rois = rois_of(proposals)
        x = self.feature_extractor(features, rois)
        class_logits, box_regression = self.predictor(x)
        if not self.training:
            with torch.no_grad():
                return x, self.post_processor((class_logits, box_regression), proposals), {}
        lc, lb = self.loss_evaluator(class_logits, box_regression)
        return x, proposals, {"loss_classifier": lc, "loss_box_reg": lb}


class CombinedROIHeads(nn.ModuleDict):
    """reference roi_heads.py:9-55 with the box head and, under MODEL.MASK_ON, the mask head (modeling/roi_mask_head.py; the
    keypoint head is not built).  In training the mask head reads the box head's plan, so it adds no host read to the box head's."""

    def forward(self, features, proposals, targets=None, sampled=None):
        """sampled: the box head's ``sampled=`` override (ROIBoxHead.forward), training only"""
        x, detections, losses = self.box(features, proposals, targets, **({} if sampled is None else {"sampled": sampled}))
        losses = dict(losses)
        if "mask" in self:
            x, detections, loss_mask = self.mask(features, detections, targets,
                                                 plan=self.box.loss_evaluator if self.training else None)
            losses.update(loss_mask)
        return x, detections, losses

"""Mask R-CNN mask head on pyramid activations, binary-mask mode: feature extractor, predictors, loss, post-processor, Masker and
module.

Mirrors the reference's fcos_core/modeling/roi_heads/mask_head/{mask_head.py, loss.py, inference.py,
roi_mask_feature_extractors.py, roi_mask_predictors.py} for MaskRCNNFPNFeatureExtractor with MaskRCNNC4Predictor or
MaskRCNNConv1x1Predictor, and the ``mask`` entry of roi_heads/roi_heads.py.

Per training step, all on the device (csrc/roi_mask.hip): ONE launch compacts the positive rows of the box head's sampled plan
with their ROIs, labels and matched ground-truth index (ops.roi_mask_positives -- the reference's keep_only_positive_boxes and
the re-match of its loss; its Matcher has the box head's thresholds and no low-quality rule, so the box plan's ``matched`` is
what it recomputes), ONE launch writes the M x M targets of every positive (ops.roi_mask_targets -- the reference's per-proposal
crop / resize / upload loop on the CPU).  Inside CombinedROIHeads the number of positives comes from the counts the box head
already read, so the mask head adds no host read; called on its own it matches the proposals itself (one more launch) and reads
the number of positives once.  The loss is one launch over the label's channel of the logits rows, one more for its backward.

The pooled rows of ops.roi_align are (PH, PW, Cs) channel-last: the rows of PyramidShape(R, [(P, P)]), so mask_fcn1..4 run on them
through ops.conv2d without a repack.  conv5_mask (2x2 / stride-2 transposed conv) runs as ONE 1x1 convolution onto 4 D columns
(kh, kw, D) + ReLU, followed by a pixel shuffle of the rows onto PyramidShape(R, [(2 P, 2 P)]) under autograd.

At test time one launch forms the sigmoid of the predicted class's channel (ops.roi_mask_prob) and, under POSTPROCESS_MASKS, one
launch per image pastes the masks into the image (ops.roi_mask_paste -- the reference's per-detection interpolate / threshold /
paste loop on the CPU).
"""
import torch
from torch import nn

from .. import config, ops
from ..structures import BoxList, SegmentationMask
from . import fcos as fcos_mod
from .poolers import Pooler
from .roi_box_head import FPN2MLPFeatureExtractor, rois_of

plan_stats = {"launches": 0, "host_reads": 0}  # what the Python side ISSUED for the most recent mask plan (counted here, not observed)


def _default_cfg():
    return config.roi_mask_settings(config.Cfg({"MODEL": {"ROI_MASK_HEAD": {
        "FEATURE_EXTRACTOR": "MaskRCNNFPNFeatureExtractor", "PREDICTOR": "MaskRCNNC4Predictor", "POOLER_RESOLUTION": 14,
        "POOLER_SCALES": (0.125, 0.0625, 0.03125, 0.015625), "POOLER_SAMPLING_RATIO": 2, "RESOLUTION": 28,
        "SHARE_BOX_FEATURE_EXTRACTOR": False}}}))


# config.roi_mask_settings of the reference's Mask R-CNN FPN yamls' ROI_MASK_HEAD block (e2e_mask_rcnn_R_50_FPN_1x)
DEFAULT_SETTINGS = _default_cfg()


def _msra_(module):
    nn.init.kaiming_normal_(module.weight, mode="fan_out", nonlinearity="relu")
    nn.init.constant_(module.bias, 0)
    return module


def _rows_dependency(x, *params):
    """an empty batch: nothing to launch, and a zero that still reaches the input and every parameter"""
    return (x.sum() + sum(p.reshape(-1)[:1].sum() for p in params)) * 0


# ----------------------------------------------------------------------------- feature extractor and predictors
class MaskRCNNFPNFeatureExtractor(nn.Module):
    """reference roi_mask_feature_extractors.py:16-66: pooler, mask_fcn1..n (3x3 conv + ReLU; kaiming_normal_(fan_out, relu),
    zero bias).  forward returns the rows [R * P * P, pad4(D)] of PyramidShape(R, [(P, P)])."""

    def __init__(self, in_channels=256, resolution=14, scales=(0.125, 0.0625, 0.03125, 0.015625), sampling_ratio=2,
                 conv_layers=(256, 256, 256, 256)):
        super().__init__()
        self.in_channels, self.resolution = int(in_channels), int(resolution)
        self.pooler = Pooler(output_size=(resolution, resolution), scales=scales, sampling_ratio=sampling_ratio)
        self.blocks, c = [], self.in_channels
        for i, d in enumerate(conv_layers, 1):
            name = "mask_fcn%d" % i
            self.add_module(name, _msra_(nn.Conv2d(c, int(d), 3, stride=1, padding=1)))
            self.blocks.append(name)
            c = int(d)
        self.out_channels = c

    pooled_rows = FPN2MLPFeatureExtractor.pooled_rows

    def shape(self, R):
        return ops.PyramidShape(R, [(self.resolution, self.resolution)])

    def forward(self, x, rois):
        """rois: [R, 5] (image index, box) or list[BoxList] -> rows [R * P * P, pad4(out_channels)]"""
        if not torch.is_tensor(rois):
            rois = rois_of(rois)
        if x[0].shape[1] != self.in_channels:
            raise RuntimeError("MaskRCNNFPNFeatureExtractor: %d feature channels, built for %d" % (x[0].shape[1], self.in_channels))
        R, layers = int(rois.shape[0]), [getattr(self, n) for n in self.blocks]
        if R == 0:
            dep = _rows_dependency(x[0], *[p for l in layers for p in l.parameters()])
            return x[0].new_zeros((0, ops.pad4(self.out_channels))) + dep
        y = self.pooled_rows(x, rois)  # [R, P, P, Cs]
        return self.convs(y.reshape(-1, y.shape[3]), R)

    def convs(self, rows, R):
        shape = self.shape(R)
        for name in self.blocks:
            l = getattr(self, name)
            rows = ops.conv2d(rows, l.weight, l.bias, shape, 3, 1, relu=True)
        return rows

    def as_nchw(self, rows):
        """the rows as the reference's [R, D, P, P] (a channels-last view)"""
        P = self.resolution
        return rows.view(-1, P, P, rows.shape[1]).permute(0, 3, 1, 2)[:, :self.out_channels]


class _MaskPredictor(nn.Module):
    def logits(self, rows, shape):
        l = self.mask_fcn_logits
        if rows.shape[0] == 0:
            return rows.new_zeros((0, ops.pad4(self.num_classes))) + _rows_dependency(rows, l.weight, l.bias)
        return ops.conv2d(rows, l.weight, l.bias, shape, 1, 1)


class MaskRCNNC4Predictor(_MaskPredictor):
    """reference roi_mask_predictors.py:10-33: conv5_mask (2x2 / stride-2 transposed conv) + ReLU, mask_fcn_logits (1x1).
    conv5_mask.weight keeps the reference's [Cin, D, 2, 2]; it is regrouped to the [4 D, Cin] rows (kh, kw, D) of a 1x1
    convolution at call time, under autograd, with the bias repeated four times -- ReLU commutes with the pixel shuffle that
    follows.  forward: rows of PyramidShape(R, [(P, P)]) -> logits rows [R * 2P * 2P, pad4(C)]."""

    def __init__(self, in_channels=256, dim_reduced=256, num_classes=81):
        super().__init__()
        self.num_classes, self.dim_reduced, self.upscale = int(num_classes), int(dim_reduced), 2
        self.conv5_mask = _msra_(nn.ConvTranspose2d(in_channels, self.dim_reduced, 2, 2, 0))
        self.mask_fcn_logits = _msra_(nn.Conv2d(self.dim_reduced, self.num_classes, 1, 1, 0))

    def upsampled(self, rows, shape):
        """rows [R * P * P, Cs] -> relu(conv5_mask) as rows [R * 2P * 2P, pad4(D)] of PyramidShape(R, [(2 P, 2 P)])"""
        D, R, (P, Pw) = self.dim_reduced, shape.n_images, shape.sizes[0]
        w = self.conv5_mask.weight.permute(2, 3, 1, 0).reshape(4 * D, -1, 1, 1)
        y = ops.conv2d(rows, w, self.conv5_mask.bias.repeat(4), shape, 1, 1, relu=True)
        y = y[:, :4 * D].reshape(R, P, Pw, 2, 2, D).permute(0, 1, 3, 2, 4, 5).reshape(R * 2 * P * 2 * Pw, D)
        if D % 4:
            y = nn.functional.pad(y, (0, ops.pad4(D) - D))
        return y, ops.PyramidShape(R, [(2 * P, 2 * Pw)])

    def forward(self, rows, shape):
        if rows.shape[0] == 0:
            dep = _rows_dependency(rows, self.conv5_mask.weight, self.conv5_mask.bias)
            return self.logits(rows.new_zeros((0, ops.pad4(self.dim_reduced))) + dep, shape)
        y, up = self.upsampled(rows, shape)
        return self.logits(y, up)


class MaskRCNNConv1x1Predictor(_MaskPredictor):
    """reference roi_mask_predictors.py:36-56: mask_fcn_logits (1x1) alone; logits rows [R * P * P, pad4(C)]"""

    def __init__(self, in_channels=256, num_classes=81):
        super().__init__()
        self.num_classes, self.upscale = int(num_classes), 1
        self.mask_fcn_logits = _msra_(nn.Conv2d(in_channels, self.num_classes, 1, 1, 0))

    def forward(self, rows, shape):
        return self.logits(rows, shape)


# ----------------------------------------------------------------------------- ground-truth masks
def target_masks(target):
    """one image's target -> its masks uint8 [G, h, w] (CPU or device): a BoxList with a ``masks`` field (a SegmentationMask in
    binary-mask mode, or the tensor itself), or a (boxes, labels, masks) tuple"""
    m = target.get_field("masks") if isinstance(target, BoxList) else (target[2] if len(target) > 2 else None)
    if isinstance(m, SegmentationMask):
        m = m.instances.masks
    if not torch.is_tensor(m) or m.dim() != 3:
        raise ValueError("the mask head needs binary masks [G, h, w] per image (a 'masks' field holding a SegmentationMask of "
                         "mode='mask'); polygon masks are not built")
    return m


def upload_masks(targets, device):
    """-> (masks uint8 flat, moff int64 [N + 1], mhw int32 [N, 2]) on the device: the layout of include/scan_hip.h, the images'
    masks back to back without padding.  The offsets come from the shapes: no device value is read."""
    ms = [target_masks(t) for t in targets]
    off, hw = [0], []
    for m in ms:
        off.append(off[-1] + int(m.numel()))
        hw.append((int(m.shape[1]), int(m.shape[2])))
    flat = torch.cat([(m if m.dtype == torch.uint8 else (m != 0).to(torch.uint8)).reshape(-1) for m in ms]).to(device)
    return flat, torch.tensor(off, dtype=torch.int64).to(device), torch.tensor(hw, dtype=torch.int32).reshape(-1, 2).to(device)


# ----------------------------------------------------------------------------- loss
class MaskRCNNLossComputation:
    """reference roi_heads/mask_head/loss.py:45-128.  ``plan_from_box`` / ``plan`` leave the positives (pos_rows, pos_rois,
    pos_labels, pos_gt) and their targets [Rp, M, M] on the evaluator; ``__call__`` is the loss on the logits rows."""

    def __init__(self, bg=0.5, fg=0.5, discretization_size=28):
        if float(bg) > float(fg):
            raise ValueError("MaskRCNNLossComputation: bg %r above fg %r" % (bg, fg))
        self.bg, self.fg, self.discretization_size = float(bg), float(fg), int(discretization_size)
        self.pos_rows = self.pos_rois = self.pos_labels = self.pos_gt = self.targets = None

    def _finish(self, labels, rois, src, matched, N, P, Rp, targets, launches, host_reads):
        self.pos_rows, self.pos_rois, self.pos_labels, self.pos_gt = ops.roi_mask_positives(labels, rois, src, matched, N, P, Rp)
        masks, moff, mhw = upload_masks(targets, rois.device)
        self.targets = ops.roi_mask_targets(self.pos_rois, self.pos_gt, masks, moff, mhw, self.discretization_size)
        plan_stats.update(launches=launches + 2, host_reads=host_reads)
        return self.pos_rois

    def plan_from_box(self, box_plan, targets):
        """box_plan: the box head's FastRCNNLossComputation after its subsample -- no launch but the two, no host read"""
        if box_plan.rois is None or box_plan.matched is None:
            raise RuntimeError("the box head's subsample needs to be called before")
        N, P = box_plan.padded
        if len(targets) != N:
            raise ValueError("MaskRCNNLossComputation: %d targets for the box plan's %d images" % (len(targets), N))
        return self._finish(box_plan.labels, box_plan.rois, box_plan.src, box_plan.matched, N, P, box_plan.n_positive, targets, 0, 0)

    def plan(self, proposals, targets):
        """proposals list[BoxList] with a ``labels`` field (the box head's subsampled proposals), targets list[BoxList] with
        ``labels`` and ``masks``: the proposals are matched here (one launch) and the number of positives is read once"""
        N = len(proposals)
        if N < 1 or len(targets) != N:
            raise ValueError("MaskRCNNLossComputation: %d proposal lists for %d targets" % (N, len(targets)))
        dev = proposals[0].bbox.device
        counts = [len(p) for p in proposals]
        P = max(1, max(counts))
        props = torch.zeros((N, P, 4), dtype=torch.float32, device=dev)
        for n, p in enumerate(proposals):
            if counts[n]:
                props[n, :counts[n]] = p.convert("xyxy").bbox.float()
        tt = [(t.convert("xyxy").bbox, t.get_field("labels")) if isinstance(t, BoxList) else (t[0], t[1]) for t in targets]
        boxes, glab, ng, _ = fcos_mod.upload_ground_truth(N, tt, dev)
        _, matched = ops.roi_box_match(props, torch.tensor(counts, dtype=torch.int32).to(dev), boxes, glab, ng, self.bg, self.fg)
        labels = torch.cat([p.get_field("labels").to(device=dev, dtype=torch.int32) for p in proposals]).contiguous()
        src = torch.cat([torch.arange(c, dtype=torch.int32) for c in counts]).to(dev)
        Rp = int((labels > 0).sum())  # the one host round trip of the stand-alone call
        return self._finish(labels, rois_of(proposals), src, matched, N, P, Rp, targets, 1, 1)

    def __call__(self, mask_logits, num_classes=None):
        """mask_logits: the logits rows [Rp * M * M, Cs] of the planned positives -> loss_mask"""
        if self.targets is None:
            raise RuntimeError("plan / plan_from_box needs to be called before")
        return ops.roi_mask_loss(mask_logits, self.pos_labels, self.targets, num_classes)


# ----------------------------------------------------------------------------- post-processor
class Masker:
    """reference mask_head/inference.py:154-194: pastes the masks of every image at their boxes, one launch per image"""

    def __init__(self, threshold=0.5, padding=1):
        if int(padding) != 1:
            raise ValueError("Masker: padding %r is not built (only 1)" % (padding,))
        if not float(threshold) >= 0:
            raise ValueError("Masker: threshold %r below 0 (the reference's mask * 255 debugging mode) is not built" % (threshold,))
        self.threshold, self.padding = float(threshold), 1

    def forward_single_image(self, masks, boxes):
        """masks [K, 1, M, M], boxes a BoxList of K boxes -> uint8 [K, 1, H, W] (K = 0: an empty [0, 1, M, M])"""
        boxes = boxes.convert("xyxy")
        im_w, im_h = boxes.size
        return ops.roi_mask_paste(masks.contiguous(), boxes.bbox.float().contiguous(), (im_h, im_w), self.threshold)

    def __call__(self, masks, boxes):
        if isinstance(boxes, BoxList):
            boxes = [boxes]
        if len(boxes) != len(masks):
            raise ValueError("Masker: %d mask sets for %d box lists" % (len(masks), len(boxes)))
        out = []
        for m, b in zip(masks, boxes):
            if m.shape[0] != len(b):
                raise ValueError("Masker: %d masks for %d boxes" % (m.shape[0], len(b)))
            out.append(self.forward_single_image(m, b))
        return out


class MaskPostProcessor(nn.Module):
    """reference mask_head/inference.py:12-62.  x: the logits rows [K * M * M, Cs] (``resolution`` gives M) or the reference's
    [K, C, M, M]; boxes list[BoxList] with ``labels`` -> list[BoxList] with the boxes' fields and ``mask`` [K_n, 1, M, M]
    probabilities, or with a masker uint8 [K_n, 1, H, W]."""

    def __init__(self, masker=None, resolution=28, num_classes=None):
        super().__init__()
        self.masker, self.resolution, self.num_classes = masker, int(resolution), num_classes

    def forward(self, x, boxes):
        M, C = self.resolution, self.num_classes
        if x.dim() == 4:
            M, C = int(x.shape[2]), int(x.shape[1])
            x = x.permute(0, 2, 3, 1).reshape(-1, C).contiguous()
        labels = torch.cat([b.get_field("labels") for b in boxes])
        prob = ops.roi_mask_prob(x, labels, M, C)
        prob = prob.split([len(b) for b in boxes], dim=0)
        if self.masker:
            prob = self.masker(prob, boxes)
        out = []
        for p, b in zip(prob, boxes):
            r = BoxList(b.bbox, b.size, mode=b.mode).convert("xyxy")
            for f in b.fields():
                r.add_field(f, b.get_field(f))
            r.add_field("mask", p)
            out.append(r)
        return out


class MaskPostProcessorCOCOFormat(MaskPostProcessor):
    """reference mask_head/inference.py:65-88 encodes the pasted masks through pycocotools: not built"""

    def __init__(self, *args, **kwargs):
        raise ValueError("MaskPostProcessorCOCOFormat is not built: its run-length encoding goes through pycocotools")


# ----------------------------------------------------------------------------- module
class ROIMaskHead(nn.Module):
    """reference mask_head.py:35-79.  cfg: a config.roi_mask_settings dict (or None: DEFAULT_SETTINGS)."""

    def __init__(self, cfg=None, in_channels=256):
        super().__init__()
        c = dict(DEFAULT_SETTINGS)
        c.update(cfg or {})
        self.settings = c
        self.feature_extractor = MaskRCNNFPNFeatureExtractor(in_channels, c["pooler_resolution"], c["pooler_scales"],
                                                             c["pooler_sampling_ratio"], c["conv_layers"])
        D = self.feature_extractor.out_channels
        if c["predictor"] == "MaskRCNNC4Predictor":
            self.predictor = MaskRCNNC4Predictor(D, c["conv_layers"][-1], c["num_classes"])
        elif c["predictor"] == "MaskRCNNConv1x1Predictor":
            self.predictor = MaskRCNNConv1x1Predictor(D, c["num_classes"])
        else:
            raise ValueError("ROIMaskHead: predictor %r is not built" % (c["predictor"],))
        if c["resolution"] != self.predictor.upscale * c["pooler_resolution"]:
            raise ValueError("ROIMaskHead: resolution %d from a pooler of %d through %s" % (c["resolution"], c["pooler_resolution"],
                                                                                           c["predictor"]))
        masker = Masker(c["postprocess_masks_threshold"], 1) if c["postprocess_masks"] else None
        self.post_processor = MaskPostProcessor(masker, c["resolution"], c["num_classes"])
        self.loss_evaluator = MaskRCNNLossComputation(c["bg_iou_threshold"], c["fg_iou_threshold"], c["resolution"])

    def forward(self, features, proposals, targets=None, plan=None):
        """features: the pyramid's levels; proposals list[BoxList] with ``labels`` (training: the box head's subsampled
        proposals, eval: its detections); targets list[BoxList] with ``labels`` and ``masks``; plan: the box head's loss
        evaluator after its subsample (CombinedROIHeads passes it: no host read) -> (x, proposals | detections with ``mask``,
        losses): training returns the proposals as they came and {"loss_mask"}, eval {}"""
        fe = self.feature_extractor
        if self.training:
            if targets is None:
                raise ValueError("ROIMaskHead: training needs targets")
            le = self.loss_evaluator
            with torch.no_grad():
                rois = le.plan_from_box(plan, targets) if plan is not None else le.plan(proposals, targets)
        else:
            rois = rois_of(proposals)
        rows = fe(features, rois)
        logits = self.predictor(rows, fe.shape(int(rois.shape[0])))
        x = fe.as_nchw(rows)
        if not self.training:
            with torch.no_grad():
                return x, self.post_processor(logits, proposals), {}
        return x, proposals, {"loss_mask": self.loss_evaluator(logits, self.settings["num_classes"])}

"""Region-proposal network on pyramid activations: head, fg / bg sampling loss, proposal selection and module.

Mirrors the reference's fcos_core/modeling/rpn/{rpn.py, loss.py, inference.py} with rpn/anchor_generator.py,
modeling/balanced_positive_negative_sampler.py, modeling/matcher.py and modeling/box_coder.py, for the FPN spelling
(MODEL.RPN.USE_FPN True) on the P3..P7 pyramid.  A = len(ASPECT_RATIOS) anchors per location, laid out as in
modeling/retinanet.py: anchor index i = m * A + a of pyramid row m = (level, image, y, x), which is the reference's order level by
level.  No [M * A, 4] anchor tensor is stored: the kernels of csrc/rpn.hip form each anchor from its row and the [L, A, 4] cell
table.

Per training step, all on the device: the labels of every anchor (the RetinaNet matcher's two launches with every box label 1
at BG / FG_IOU_THRESHOLD, then the visibility launch), the balanced sampler (one launch for all images, ops.rpn_sample), the fused
objectness BCE + smooth-L1 loss over all anchors (one launch, one more for the backward) and ONE host read: the sampled count
both losses are divided by.  The sampler replaces the reference's per-image nonzero + randperm by a keyed selection (the
smallest keys of an integer mix of seed, image and anchor index): the same distribution of samples, not the same samples, so
``RPNLossComputation.__call__`` takes a ``sampled=`` override through which the tests feed the reference's own sample.

Proposal selection follows rpn/inference.py: per level and image the top PRE_NMS_TOP_N sigmoid scores (torch.topk on the
device over a view), one ops.rpn_decode_proposals launch that gathers, decodes, clips and flags small boxes for all levels and
images, per image one NMS launch with the level as the label, the POST_NMS_TOP_N cap per level, then the FPN-wide top-n.
"""
import torch
from torch import nn

from .. import config, ops
from ..structures import BoxList
from . import fcos as fcos_mod
from . import retinanet
from .backbone import conv_holder

ANCHOR_STRIDES = retinanet.ANCHOR_STRIDES
ANCHOR_SIZES = retinanet.ANCHOR_SIZES

# config.rpn_settings of a cfg without a MODEL.RPN block: config.RPN_DEFAULTS, flat
DEFAULT_SETTINGS = config.rpn_settings(config.Cfg({"MODEL": {}}))

plan_stats = {"launches": 0, "host_reads": 0}  # what the Python side ISSUED for the most recent labels + sampler (counted here, not observed)
_hw_on = {}  # (image sizes, device) -> the [N, 2] int32 table there


def cell_anchors(strides=ANCHOR_STRIDES, sizes=ANCHOR_SIZES, aspect_ratios=(0.5, 1.0, 2.0)):
    """[L, A, 4]: one size per level, ratio-major (reference rpn/anchor_generator.py:40-67 for an FPN)"""
    return retinanet.cell_anchors(strides, sizes, aspect_ratios, octave=2.0, scales_per_octave=1)


def device_image_hw(image_sizes, device):
    """[N, 2] int32 (height, width) on ``device``, uploaded once per distinct list"""
    key = (tuple((int(h), int(w)) for h, w in image_sizes), str(device))
    t = _hw_on.get(key)
    if t is None:
        if len(_hw_on) > 64:
            _hw_on.clear()
        t = _hw_on[key] = torch.tensor(key[0], dtype=torch.int32).reshape(-1, 2).to(device)
    return t


# ----------------------------------------------------------------------------- head
class RPNHead(nn.Module):
    """reference rpn.py:75-108 (SingleConvRPNHead): conv 3x3 + ReLU, cls_logits 1x1 -> A, bbox_pred 1x1 -> 4 A; normal std 0.01,
    zero biases.  The two 1x1 convs run as ONE launch over their stacked [5 A, 256] weights (bbox_pred first, so that its
    columns start 16-byte aligned) and the outputs are column slices of that launch's padded rows; the parameters and their
    state_dict keys stay the reference's."""

    def __init__(self, in_channels=256, num_anchors=3):
        super().__init__()
        self.num_anchors = num_anchors
        self.conv = conv_holder(in_channels, in_channels, 3)
        self.cls_logits = conv_holder(in_channels, num_anchors, 1)
        self.bbox_pred = conv_holder(in_channels, num_anchors * 4, 1)
        for m in (self.conv, self.cls_logits, self.bbox_pred):
            nn.init.normal_(m.weight, std=0.01)
            nn.init.constant_(m.bias, 0)

    def forward(self, rows, shape):
        """-> objectness [M, A] and bbox_reg [M, 4 A]"""
        A = self.num_anchors
        t = ops.conv2d(rows, self.conv.weight, self.conv.bias, shape, 3, 1, relu=True)
        w = torch.cat((self.bbox_pred.weight, self.cls_logits.weight), 0).contiguous(memory_format=torch.channels_last)
        b = torch.cat((self.bbox_pred.bias, self.cls_logits.bias), 0)
        y = ops.conv2d(t, w, b, shape, 1, 1)
        return y[:, 4 * A:5 * A], y[:, :4 * A]


# ----------------------------------------------------------------------------- loss
class RPNLossComputation:
    """reference rpn/loss.py:21-131 on one rank.  loss_objectness = BCE-with-logits over the sampled anchors (mean),
    loss_rpn_box_reg = smooth-L1 (beta 1 / 9) over the sampled positives / the sampled count.  ``seed`` keys the sampler; every
    call advances a counter that is mixed into it, so successive steps draw different samples and two runs from one seed draw
    the same ones."""

    def __init__(self, strides=ANCHOR_STRIDES, cells=None, bg=0.3, fg=0.7, straddle_thresh=0.0, batch_size_per_image=256,
                 positive_fraction=0.5, beta=1.0 / 9, seed=0):
        self.strides = tuple(strides)
        self.cells = cell_anchors() if cells is None else cells
        self.bg, self.fg, self.straddle_thresh = float(bg), float(fg), float(straddle_thresh)
        self.batch_size_per_image, self.positive_fraction = int(batch_size_per_image), float(positive_fraction)
        self.beta = float(beta)
        self.seed, self.calls = int(seed), 0

    def labels(self, shape, targets, image_sizes, device):
        """-> labels_i32 [M * A], matched [M * A], boxes [N, G, 4] on ``device``"""
        retinanet._check_geometry(shape, self.strides, self.cells)
        boxes, _, ng, _ = fcos_mod.upload_ground_truth(shape.n_images, targets, device)
        labels, matched = ops.rpn_labels(shape, self.strides, retinanet.device_cells(self.cells, device), boxes, ng,
                                         device_image_hw(image_sizes, device), self.bg, self.fg, self.straddle_thresh)
        return labels, matched, boxes

    def next_seed(self):
        s = (self.seed + 0x9E3779B9 * self.calls) & 0xffffffff
        self.calls += 1
        return s

    def __call__(self, shape, objectness, box_regression, targets, image_sizes, sampled=None):
        """objectness [M, A], box_regression [M, 4 A] (column slices are read in place), targets [(boxes, labels)] per image.
        sampled (uint8 [M * A], 1 positive / 2 negative / 0): use this sample instead of drawing one."""
        dev = objectness.device
        A = int(self.cells.shape[1])
        labels, matched, boxes = self.labels(shape, targets, image_sizes, dev)
        launches = 2 + (self.straddle_thresh >= 0)
        if sampled is None:
            sampled, counts = ops.rpn_sample(shape, A, labels, self.batch_size_per_image, self.positive_fraction, self.next_seed())
            n = int(counts.sum().item())  # the one host round trip
            launches += 1
        else:
            sampled = sampled.to(device=dev, dtype=torch.uint8).contiguous()
            n = int((sampled != 0).sum().item())
        plan_stats.update(launches=launches, host_reads=1)
        out = ops.rpn_loss(objectness, box_regression, shape, self.strides, retinanet.device_cells(self.cells, dev), boxes, matched,
                           sampled, self.beta)
        out = out / max(n, 1)  # an empty sample: both losses 0 (the reference divides by zero)
        return out[0], out[1]


# ----------------------------------------------------------------------------- proposals
class RPNPostProcessor:
    """reference rpn/inference.py:13-179.  ``training`` selects select_over_all_levels' rule: True is ONE top-n over the whole
    batch (and the ground truth is appended when targets are given), False is a sorted top-n per image."""

    def __init__(self, pre_nms_top_n, post_nms_top_n, nms_thresh, min_size, fpn_post_nms_top_n=None, strides=ANCHOR_STRIDES,
                 cells=None, training=False):
        self.pre_nms_top_n, self.post_nms_top_n = int(pre_nms_top_n), int(post_nms_top_n)
        self.nms_thresh, self.min_size = float(nms_thresh), float(min_size)
        self.fpn_post_nms_top_n = int(post_nms_top_n if fpn_post_nms_top_n is None else fpn_post_nms_top_n)
        self.strides = tuple(strides)
        self.cells = cell_anchors() if cells is None else cells
        self.training = training

    def candidates(self, shape, objectness, box_regression, image_sizes):
        """-> scores [N, K], anchor index [N, K] (i = m * A + a), level [K], boxes [N, K, 4], keep [N, K] uint8: the top
        PRE_NMS_TOP_N of every level side by side, by falling score within a level"""
        N, dev = shape.n_images, objectness.device
        A = int(self.cells.shape[1])
        prob = objectness.sigmoid()
        vals, idxs, glob, ks = [], [], [], []
        for l in range(shape.n_levels):
            r0, r1 = shape.row_off[l], shape.row_off[l + 1]
            n_l = (r1 - r0) // N * A
            k = min(self.pre_nms_top_n, n_l)
            val, idx = prob[r0:r1].reshape(N, n_l).topk(k, dim=1, sorted=True)
            vals.append(val)
            idxs.append(idx)
            glob.append(r0 * A + torch.arange(N, device=dev)[:, None] * n_l + idx)
            ks.append(k)
        idx = torch.cat(idxs, 1).contiguous()
        boxes, keep = ops.rpn_decode_proposals(box_regression, shape, self.strides, retinanet.device_cells(self.cells, dev), idx, ks,
                                               device_image_hw(image_sizes, dev), self.min_size)
        level = torch.repeat_interleave(torch.arange(shape.n_levels, device=dev), torch.tensor(ks, device=dev))
        return torch.cat(vals, 1), torch.cat(glob, 1), level, boxes, keep

    def __call__(self, shape, objectness, box_regression, image_sizes, targets=None, return_indices=False):
        """-> list[BoxList] with field "objectness"; with return_indices also per image the anchor index of every proposal
        (-1 for an appended ground-truth box)"""
        N, dev = shape.n_images, objectness.device
        scores, glob, level, boxes, keep = self.candidates(shape, objectness, box_regression, image_sizes)
        per_image = []
        for i in range(N):
            sel = torch.nonzero(keep[i]).squeeze(1)
            b, s, lv, g = boxes[i][sel], scores[i][sel], level[sel], glob[i][sel]
            kept = ops.nms_by_label(b, s, lv, self.nms_thresh).to(dev)  # ascending: level-major, falling score within a level
            lk = lv[kept]
            rank = torch.arange(kept.numel(), device=dev) - torch.searchsorted(lk, lk)  # position within its level
            kept = kept[rank < self.post_nms_top_n]
            per_image.append((b[kept], s[kept], g[kept]))
        if shape.n_levels > 1:
            if self.training:
                every = torch.cat([s for _, s, _ in per_image], 0)
                top = torch.topk(every, min(self.fpn_post_nms_top_n, every.numel()), dim=0, sorted=True)[1]
                mask = torch.zeros_like(every, dtype=torch.bool)
                mask[top] = True
                masks = mask.split([s.numel() for _, s, _ in per_image])
                per_image = [(b[m], s[m], g[m]) for (b, s, g), m in zip(per_image, masks)]
            else:
                out = []
                for b, s, g in per_image:
                    top = torch.topk(s, min(self.fpn_post_nms_top_n, s.numel()), dim=0, sorted=True)[1]
                    out.append((b[top], s[top], g[top]))
                per_image = out
        result, indices = [], []
        for i, ((b, s, g), (h, w)) in enumerate(zip(per_image, image_sizes)):
            if self.training and targets is not None:  # add_gt_proposals
                gt = targets[i][0].to(device=dev, dtype=torch.float32).reshape(-1, 4)
                b = torch.cat((b, gt), 0)
                s = torch.cat((s, torch.ones((gt.shape[0],), device=dev)), 0)
                g = torch.cat((g, torch.full((gt.shape[0],), -1, dtype=g.dtype, device=dev)), 0)
            bl = BoxList(b, (int(w), int(h)), mode="xyxy")
            bl.add_field("objectness", s)
            result.append(bl)
            indices.append(g)
        return (result, indices) if return_indices else result


# ----------------------------------------------------------------------------- module
class RPNModule(nn.Module):
    """reference rpn.py:111-198.  cfg: a config.rpn_settings dict (or None: DEFAULT_SETTINGS)."""

    def __init__(self, cfg=None, seed=0):
        super().__init__()
        c = dict(DEFAULT_SETTINGS)
        c.update(cfg or {})
        strides = tuple(c["anchor_strides"])
        A = len(c["aspect_ratios"])  # config.rpn_settings has refused what is not built; the kernels check the geometry again
        self.settings = c
        self.cells = cell_anchors(strides, c["anchor_sizes"], c["aspect_ratios"])
        # the reference's anchor_generator.cell_anchors.<level> buffers, so that its checkpoints load key for key; the kernels
        # read self.cells, which the settings alone determine
        self.anchor_generator = nn.Module()
        self.anchor_generator.cell_anchors = nn.Module()
        for l, cell in enumerate(self.cells):
            self.anchor_generator.cell_anchors.register_buffer(str(l), cell.clone())
        self.head = RPNHead(256, A)
        self.loss_evaluator = RPNLossComputation(strides, self.cells, c["bg_iou_threshold"], c["fg_iou_threshold"],
                                                 c["straddle_thresh"], c["batch_size_per_image"], c["positive_fraction"], seed=seed)
        common = dict(nms_thresh=c["nms_thresh"], min_size=c["min_size"], strides=strides, cells=self.cells)
        self.box_selector_train = RPNPostProcessor(c["pre_nms_top_n_train"], c["post_nms_top_n_train"],
                                                   fpn_post_nms_top_n=c["fpn_post_nms_top_n_train"], training=True, **common)
        self.box_selector_test = RPNPostProcessor(c["pre_nms_top_n_test"], c["post_nms_top_n_test"],
                                                  fpn_post_nms_top_n=c["fpn_post_nms_top_n_test"], training=False, **common)
        self.rpn_only = bool(c["rpn_only"])

    def forward(self, image_sizes, rows, shape, targets=None):
        """image_sizes [(h, w)] unpadded, rows [M, 256] of the pyramid ``shape``, targets [(boxes [g, 4], labels [g])] per image
        -> (list[BoxList] with field "objectness" | None, losses).  Training: the proposals of box_selector_train (ground truth
        appended) and {"loss_objectness", "loss_rpn_box_reg"}; with MODEL.RPN_ONLY the boxes are None -- the reference returns its
        anchor lists there, which nothing consumes, and there is no anchor tensor here.  Eval: the proposals of
        box_selector_test and {}; with MODEL.RPN_ONLY sorted by falling objectness."""
        if self.training and targets is None:
            raise ValueError("RPNModule: training needs targets")
        objectness, reg = self.head(rows, shape)
        if self.training:
            boxes = None
            if not self.rpn_only:
                with torch.no_grad():
                    boxes = self.box_selector_train(shape, objectness.detach(), reg.detach(), image_sizes, targets)
            lo, lr = self.loss_evaluator(shape, objectness, reg, targets, image_sizes)
            return boxes, {"loss_objectness": lo, "loss_rpn_box_reg": lr}
        with torch.no_grad():
            boxes = self.box_selector_test(shape, objectness, reg, image_sizes)
            if self.rpn_only:
                boxes = [b[b.get_field("objectness").sort(descending=True)[1]] for b in boxes]
        return boxes, {}

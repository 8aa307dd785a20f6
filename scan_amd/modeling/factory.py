"""The reference's module factories and call signatures on the pyramid path.

A reference training script builds its sub-models with ``build_backbone(cfg)`` (modeling/backbone/backbone.py:21-44),
``build_rpn(cfg, in_channels)`` / ``build_middle_head(cfg, in_channels)`` (modeling/rpn/rpn.py:201-218) and one
``FCOSDiscriminator_con`` per level (tools/train_net_da.py:223-274), and drives them through ``foward_detector``
(engine/trainer.py:20-72): NCHW level lists between the modules, ``list[BoxList]`` targets in, ``list[BoxList]`` detections
out.  The builders here take the same yacs-shaped cfg (``config.load(...)``) and return modules with those signatures --

    backbone(images_tensor)                                                      -> features
    middle_head(images, features, targets, return_maps, mode, forward_target)    -> (features, loss_graph, act_loss, act_maps)
    fcos(images, features, targets, return_maps, act_maps)                       -> (proposals, losses, score_maps)
    dis(feature, target, act_maps, domain)                                       -> loss

-- that are thin subclasses of the engine's modules: same parameters, same ``state_dict`` keys (checkpoints and
``engine.load_state_dicts`` work on them), only ``forward`` differs.  Every level list they return is an ``ops.PyramidLevels``:
channels_last NCHW views of ONE [M, C] row matrix.  A module that is handed such a list back takes the matrix itself
(``ops.pack_levels``: no copy, no launch) and runs the engine's one-launch-per-layer implementation on it; a level list from
anywhere else (a foreign backbone, any layout) is packed into a row matrix by one launch of csrc/pyramid_pack.hip, whose
backward returns the gradient in the caller's layout.  Unlike ``scan_amd.surface`` nothing here runs once per level.
"""
import torch

from .. import config, ops
from ..structures import BoxList, to_image_list
from . import discriminator, fcos as fcos_mod
from .atss import ATSSModule
from .backbone import VGG16FPN
from .condgraph import GRAPHModule
from .discriminator import FCOSDiscriminator_con
from .fcos import FCOSModule
from .resnet import ResNetFPNBackbone
from .retinanet import RetinaNetModule
from .roi_box_head import CombinedROIHeads, ROIBoxHead
from .roi_mask_head import ROIMaskHead
from .rpn import RPNModule

LEVELS = ("P3", "P4", "P5", "P6", "P7")
DIS_ORDER = ("P7", "P6", "P5", "P4", "P3")  # order the reference builds them in (tools/train_net_da.py:223-274)
CONV_BODIES = ("VGG-16-FPN-RETINANET", "R-50-FPN-RETINANET", "R-101-FPN-RETINANET")


def _channels_last_(module):
    """4-D parameters stored channels_last, as engine.build_model leaves them (the kernels read [Cout][k*k][Cin] in place)"""
    for p in module.parameters():
        if p.dim() == 4:
            p.data = p.data.contiguous(memory_format=torch.channels_last)
    return module


_targets_seen = [None, None]


def target_tuples(targets):
    """list[BoxList] (boxes read in xyxy, labels from the "labels" field) -> the (boxes, labels) tuples the ground-truth plan
    consumes; tuples pass through.  The same list object maps to the same result object, so the middle head and the FCOS head of
    one iteration share one plan (modeling/fcos.py: target_plan is keyed by the list's identity)."""
    if not targets or not isinstance(targets[0], BoxList):
        return targets
    if _targets_seen[0] is targets:
        return _targets_seen[1]
    out = [(t.convert("xyxy").bbox, t.get_field("labels")) for t in targets]
    _targets_seen[:] = [targets, out]
    return out


def _rows_exact(levels, c=None):
    """(rows [M, c] contiguous, PyramidShape) of a level list: its own matrix when it is an intact PyramidLevels, one pack launch
    otherwise (padding columns, present when c is no multiple of 4, are dropped again)"""
    rows, shape = ops.pack_levels(levels)
    c = levels[0].shape[1] if c is None else c
    if rows.shape[1] != c:
        rows = rows[:, :c].contiguous()
    return rows, shape


class _BackboneForward:
    def forward(self, images, rows=None, shape=None):
        """images [N, 3, H, W] (or an ImageList) -> PyramidLevels of P3..P7"""
        if hasattr(images, "tensors"):
            images = images.tensors
        return ops.PyramidLevels(*super().forward(images, rows, shape))


class VGG16FPNBackbone(_BackboneForward, VGG16FPN):
    pass


class ResNetFPNRetinaBackbone(_BackboneForward, ResNetFPNBackbone):
    pass


def build_backbone(cfg):
    """reference modeling/backbone/backbone.py:21-44,76-80: the registry entry MODEL.BACKBONE.CONV_BODY names."""
    body = str(cfg.MODEL.BACKBONE.CONV_BODY)
    if body == "VGG-16-FPN-RETINANET":
        m = VGG16FPNBackbone()
    elif body in ("R-50-FPN-RETINANET", "R-101-FPN-RETINANET"):
        m = ResNetFPNRetinaBackbone(body[:-len("-FPN-RETINANET")], int(cfg.MODEL.BACKBONE.FREEZE_CONV_BODY_AT))
    else:
        raise ValueError("MODEL.BACKBONE.CONV_BODY %r is not built (one of %s)" % (body, ", ".join(CONV_BODIES)))
    return _channels_last_(m)


class GRAPHModuleNCHW(GRAPHModule):
    """GRAPHModule.forward of the reference (rpn/fcos/condgraph.py:547-556)."""

    def forward(self, images, features, targets=None, return_maps=False, mode="source", forward_target=False):
        """-> (features, (node_loss, consistency_loss) | None, act_loss | None, act_maps); both lists are PyramidLevels.  The act
        maps are returned whatever ``return_maps`` says, like the reference's three branches do (:445, :527, :545)."""
        rows, shape = ops.pack_levels(features)
        targets = target_tuples(targets)
        if self.training and targets and mode == "source" and rows.is_cuda:
            # the ground-truth plan on the side stream engine.forward_detector builds it on: its host round trip then waits for
            # three small kernels, not for the backbone convolutions queued in front of this call
            after = None
            if any(b.is_cuda or l.is_cuda for b, l in targets):
                after = torch.cuda.Event()
                after.record(torch.cuda.current_stream())
            fcos_mod.target_plan(shape, targets, rows.device, side_stream=ops.borrow_side_streams(3)[0], after=after)
        out, loss_graph, act_loss, maps = super().forward(rows, shape, targets=targets, mode=mode, forward_target=forward_target)
        return ops.PyramidLevels(out, shape), loss_graph, act_loss, ops.PyramidLevels(maps, shape)


def build_middle_head(cfg, in_channels):
    """reference modeling/rpn/rpn.py:215-218."""
    if not cfg.MODEL.MIDDLE_HEAD.CONDGRAPH_ON:
        raise ValueError("MODEL.MIDDLE_HEAD.CONDGRAPH_ON is False: no other middle head is built")
    s = config.settings(cfg)
    if s["num_convs_in"] != 2 or s["num_convs_out"] != 1:
        raise ValueError("MODEL.MIDDLE_HEAD.NUM_CONVS_IN/OUT other than 2/1 are not built")
    # the same construction as condgraph.build_condgraph(settings, in_channels) (rpn/fcos/condgraph.py:127-253)
    m = GRAPHModuleNCHW(in_channels, s["num_classes"], proto_iter=s["proto_iter"], transfer_cfg=s["transfer_cfg"],
                        dbscan_eps=s["dbscan_eps"], dbscan_thr=s["dbscan_thr"])
    m.lamda1, m.lamda2 = s["gcn_loss_weight"], s["act_loss_weight"]
    m.lamda3, m.lamda4 = s["con_loss_weight"], s["gcn_loss_weight_tg"]
    return _channels_last_(m)


class _RpnForwardNCHW:
    """the reference's dense-head call (rpn/fcos/fcos.py:144-232, rpn/atss/atss.py:205-270) over an engine module that has
    head / loss_evaluator / box_selector_test and forward(image_sizes, rows, shape, targets, act_maps)"""

    def forward(self, images, features, targets=None, return_maps=False, act_maps=None):
        """training: (None, losses, score_maps | None) -- score_maps = {"box_cls", "box_regression", "centerness"} as
        PyramidLevels when ``return_maps``; without targets the loss dict is the reference's {"zero": 0} (:215-220) and the head
        only runs when its maps are asked for.  eval: (list[BoxList] with fields "scores" and "labels", clipped to
        images.image_sizes, {}, None)."""
        il = to_image_list(images)
        rows, shape = ops.pack_levels(features)
        targets = target_tuples(targets)
        if not self.training:
            maps = _rows_exact(act_maps)[0] if act_maps is not None and self.mode != "common" else None  # 'common' scores alone
            dets, _ = super().forward(il.image_sizes, rows, shape, act_maps=maps)
            boxlists = []
            for (boxes, scores, labels), (h, w) in zip(dets, il.image_sizes):
                b = BoxList(boxes, (int(w), int(h)), mode="xyxy")
                b.add_field("scores", scores)
                b.add_field("labels", labels)
                boxlists.append(b)
            return boxlists, {}, None
        if not return_maps:
            return super().forward(il.image_sizes, rows, shape, targets=targets) + (None,)
        logits, reg, ctr = self.head(rows, shape)
        if targets is None:
            losses = {"zero": rows.new_zeros(())}
        else:
            lc, lr, lctr = self.loss_evaluator(shape, logits, reg, ctr, targets)
            losses = {"loss_cls": lc, "loss_reg": lr, "loss_centerness": lctr}
        score_maps = {"box_cls": ops.PyramidLevels(logits, shape), "box_regression": ops.PyramidLevels(reg, shape),
                      "centerness": ops.PyramidLevels(ctr[:, None], shape)}
        return None, losses, score_maps


class FCOSModuleNCHW(_RpnForwardNCHW, FCOSModule):
    """FCOSModule.forward of the reference (rpn/fcos/fcos.py:144-232)."""


class ATSSModuleNCHW(_RpnForwardNCHW, ATSSModule):
    """ATSSModule.forward of the reference (rpn/atss/atss.py:205-270) with the ``act_maps`` argument foward_detector passes
    (engine/trainer.py:20-72): accepted and ignored.  The reference's own ATSSModule.forward lacks it and cannot be called
    by that function."""


class RetinaNetModuleNCHW(_RpnForwardNCHW, RetinaNetModule):
    """RetinaNetModule.forward of the reference (rpn/retinanet/retinanet.py:112-148) with the ``return_maps`` / ``act_maps``
    arguments foward_detector passes (engine/trainer.py:20-72), which the reference's own forward lacks.  Two losses
    (loss_retina_cls, loss_retina_reg) and no centerness: score_maps = {"box_cls", "box_regression"}."""

    def forward(self, images, features, targets=None, return_maps=False, act_maps=None):
        if not self.training or not return_maps:
            return super().forward(images, features, targets, return_maps, act_maps)
        rows, shape = ops.pack_levels(features)
        targets = target_tuples(targets)
        logits, reg = self.head(rows, shape)
        if targets is None:
            losses = {"zero": rows.new_zeros(())}
        else:
            lc, lr = self.loss_evaluator(shape, logits, reg, targets)
            losses = {"loss_retina_cls": lc, "loss_retina_reg": lr}
        return None, losses, {"box_cls": ops.PyramidLevels(logits, shape), "box_regression": ops.PyramidLevels(reg, shape)}


class RPNModuleNCHW(RPNModule):
    """RPNModule.forward of the reference (rpn/rpn.py:142-198): (images, features, targets) -> (list[BoxList] with field
    "objectness" | None, losses).  With MODEL.RPN_ONLY in training the boxes are None (the reference returns its anchor lists;
    there is no anchor tensor here)."""

    def forward(self, images, features, targets=None):
        il = to_image_list(images)
        rows, shape = ops.pack_levels(features)
        return super().forward(il.image_sizes, rows, shape, targets=target_tuples(targets))


def build_rpn(cfg, in_channels):
    """reference modeling/rpn/rpn.py:201-212: ATSS_ON -> the ATSS head, else FCOS_ON -> the FCOS head, else RETINANET_ON -> the
    RetinaNet head, else the region-proposal network -- built only when the cfg itself carries a MODEL.RPN block (the shipped
    yamls carry none, and config.RPN_DEFAULTS stays out of config.DEFAULTS)."""
    if in_channels != 256:
        raise ValueError("the dense heads are built for 256 input channels, got %d" % in_channels)
    if cfg.MODEL.get("ATSS_ON", False):
        return _channels_last_(ATSSModuleNCHW(cfg=config.atss_settings(cfg)))
    if not cfg.MODEL.get("FCOS_ON", False):
        if cfg.MODEL.get("RETINANET_ON", False):
            return _channels_last_(RetinaNetModuleNCHW(cfg=config.retinanet_settings(cfg)))
        if isinstance(cfg.MODEL.get("RPN"), dict):
            return _channels_last_(RPNModuleNCHW(cfg=config.rpn_settings(cfg)))
        raise ValueError("MODEL.ATSS_ON, MODEL.FCOS_ON and MODEL.RETINANET_ON are False and the cfg has no MODEL.RPN block: those "
                         "three heads are built, and a MODEL.RPN block selects the RPN")
    if not cfg.MODEL.MIDDLE_HEAD.CONDGRAPH_ON:  # the EPM baseline: the plain head, centerness where MODEL.FCOS.REG_CTR_ON puts it
        h = config.epm_settings(cfg)["head"]
        return _channels_last_(FCOSModuleNCHW(h["num_classes"], h["test_mode"], h))
    s = config.settings(cfg)
    return _channels_last_(FCOSModuleNCHW(s["num_classes"], s["test_mode"], s))


def build_roi_heads(cfg, in_channels):
    """reference modeling/roi_heads/roi_heads.py:58-76: [] under MODEL.RETINANET_ON or MODEL.RPN_ONLY, else the combined heads
    whose ``box`` entry is the Fast R-CNN box head (state_dict keys roi_heads.box. ...) -- built only when the cfg itself carries
    a MODEL.ROI_BOX_HEAD block (the shipped yamls carry none, and config.ROI_BOX_HEAD_DEFAULTS stays out of config.DEFAULTS) --
    and, under MODEL.MASK_ON with a MODEL.ROI_MASK_HEAD block, whose ``mask`` entry is the Mask R-CNN mask head in binary-mask
    mode (config.roi_mask_settings).  The keypoint head is not built: MODEL.KEYPOINT_ON is refused."""
    if cfg.MODEL.get("RETINANET_ON", False) or cfg.MODEL.get("RPN_ONLY", False):
        return []
    if not isinstance(cfg.MODEL.get("ROI_BOX_HEAD"), dict):
        raise ValueError("the cfg has no MODEL.ROI_BOX_HEAD block: a MODEL.ROI_BOX_HEAD block selects the box head")
    if in_channels != 256:
        raise ValueError("the box head is built for 256 input channels, got %d" % in_channels)
    heads = [("box", ROIBoxHead(config.roi_box_settings(cfg), in_channels))]
    if cfg.MODEL.get("MASK_ON", False):
        heads.append(("mask", ROIMaskHead(config.roi_mask_settings(cfg), in_channels)))
    return CombinedROIHeads(dict(heads))


class GeneralizedRCNN(torch.nn.Module):
    """reference modeling/detector/generalized_rcnn.py:16-70: backbone, rpn, roi_heads.  The middle head (the conditional graph
    module) belongs to the FCOS path and is refused here by name."""

    def __init__(self, cfg):
        super().__init__()
        if cfg.MODEL.get("MIDDLE_HEAD", {}).get("CONDGRAPH_ON", False) and isinstance(cfg.MODEL.get("RPN"), dict) \
                and not (cfg.MODEL.get("FCOS_ON", False) or cfg.MODEL.get("ATSS_ON", False) or cfg.MODEL.get("RETINANET_ON", False)):
            raise ValueError("MODEL.MIDDLE_HEAD.CONDGRAPH_ON True with the region-proposal network is not built (set it to False)")
        self.backbone = build_backbone(cfg)
        self.rpn = build_rpn(cfg, self.backbone.out_channels)
        roi_heads = build_roi_heads(cfg, self.backbone.out_channels)
        self.roi_heads = roi_heads if roi_heads else None

    def forward(self, images, targets=None):
        """images [N, 3, H, W] (or an ImageList), targets list[BoxList] -> the loss dict in training, list[BoxList] detections
        (the RPN's proposals without roi_heads) in eval"""
        if self.training and targets is None:
            raise ValueError("In training mode, targets should be passed")
        images = to_image_list(images)
        features = self.backbone(images.tensors)
        proposals, proposal_losses = self.rpn(images, features, targets)[:2]
        if self.roi_heads is not None:
            # the mask head reads the masks from the targets' ``masks`` field: the BoxLists go through as they are
            heads_targets = targets if "mask" in self.roi_heads else target_tuples(targets)
            _, result, detector_losses = self.roi_heads(features, proposals, heads_targets)
        else:
            result, detector_losses = proposals, {}
        if self.training:
            losses = dict(detector_losses)
            losses.update(proposal_losses)
            return losses
        return result


def build_detection_model(cfg):
    """reference modeling/detector/detectors.py: META_ARCHITECTURE GeneralizedRCNN"""
    arch = str(cfg.MODEL.get("META_ARCHITECTURE", "GeneralizedRCNN"))
    if arch != "GeneralizedRCNN":
        raise ValueError("MODEL.META_ARCHITECTURE %r is not built (only 'GeneralizedRCNN')" % arch)
    return _channels_last_(GeneralizedRCNN(cfg))


class FCOSDiscriminatorNCHW(FCOSDiscriminator_con):
    """FCOSDiscriminator_con.forward of the reference (discriminator/fcos_head_discriminator_con.py:92-126) on ONE level."""

    def forward(self, feature, target, act_maps=None, domain="source", shape=None):
        """feature [N, 256, h, w], act_maps [N, K, h, w].  Level views of a PyramidLevels are taken as the rows they are (no
        copy); anything else goes through the pack kernel."""
        if shape is not None:  # the engine's own call: rows of one level
            return super().forward(feature, target, act_maps, domain=domain, shape=shape)
        frows, shape = _level_rows(feature)
        arows, _ = _level_rows(act_maps)
        return super().forward(frows, target, arows, domain=domain, shape=shape)


# the name a reference script constructs its discriminators by (tools/train_net_da.py:223-274): same keyword arguments
FCOSDiscriminator_con = FCOSDiscriminatorNCHW


class FCOSDiscriminatorGANCHW(discriminator.FCOSDiscriminator):
    """FCOSDiscriminator.forward of the reference (discriminator/fcos_head_discriminator.py:57-74) on ONE level."""

    def forward(self, feature, target, domain="source", shape=None):
        """feature [N, 256, h, w] (or, with ``shape``, the engine's rows of one level)"""
        if shape is not None:
            return super().forward(feature, target, domain=domain, shape=shape)
        frows, shape = _level_rows(feature)
        return super().forward(frows, target, domain=domain, shape=shape)


class FCOSDiscriminatorCANCHW(discriminator.FCOSDiscriminator_CA):
    """FCOSDiscriminator_CA.forward of the reference (discriminator/fcos_head_discriminator_CA.py:56-124) on ONE level."""

    def forward(self, feature, target, score_map=None, domain="source", shape=None):
        """feature [N, 256, h, w], score_map {"box_cls": [N, C, h, w], "centerness": [N, 1, h, w]} of that level"""
        if shape is not None:
            return super().forward(feature, target, score_map, domain=domain, shape=shape)
        frows, shape = _level_rows(feature)
        maps = {"box_cls": _level_rows(score_map["box_cls"])[0], "centerness": _level_rows(score_map["centerness"])[0]}
        return super().forward(frows, target, maps, domain=domain, shape=shape)


# the names a reference script constructs the EPM discriminators by (tools/train_net_da.py:100-220): same keyword arguments
FCOSDiscriminator = FCOSDiscriminatorGANCHW
FCOSDiscriminator_CA = FCOSDiscriminatorCANCHW


def _level_rows(t):
    """one [N, C, h, w] level -> ([N*h*w, C] rows, its PyramidShape): a view when the level is dense channels_last"""
    n, c, h, w = t.shape
    nhwc = t.permute(0, 2, 3, 1)
    if nhwc.is_contiguous():
        return nhwc.view(n * h * w, c), ops.PyramidShape(n, [(h, w)])
    return _rows_exact([t], c)


def build_discriminators(cfg):
    """{"dis_P7_CON": ..., ..., "dis_P3_CON": ...} for the levels MODEL.ADV.USE_DIS_<level>_CON switches on, with the level's
    CON_NUM_SHARED_CONV_<level> tower convs and GRL_WEIGHT_<level> (reference tools/train_net_da.py:223-274).  Without
    USE_DIS_CON: the EPM baseline's {"dis_P7": ..., "dis_P3": ..., "dis_P7_CA": ..., "dis_P3_CA": ...} for the levels
    MODEL.ADV.USE_DIS_<level> switches on -- the GA discriminators when USE_DIS_GLOBAL, then the CA ones when
    USE_DIS_CENTER_AWARE (:69-131); nothing when neither is set."""
    A = cfg.MODEL.ADV
    if not A.USE_DIS_CON:
        if not (A.get("USE_DIS_GLOBAL", False) or A.get("USE_DIS_CENTER_AWARE", False)):
            return {}
        s = config.epm_settings(cfg)
        out = {}
        used = [lvl for lvl in DIS_ORDER if s["use_dis"][lvl]]
        if s["use_dis_global"]:
            for lvl in used:
                out["dis_%s" % lvl] = _channels_last_(FCOSDiscriminatorGANCHW(
                    patch_stride=A.PATCH_STRIDE, num_convs=s["dis_num_convs"][lvl], grad_reverse_lambda=s["grl_weight"][lvl],
                    grl_applied_domain=str(A.GRL_APPLIED_DOMAIN)))
        if s["use_dis_center_aware"]:
            for lvl in used:
                out["dis_%s_CA" % lvl] = _channels_last_(FCOSDiscriminatorCANCHW(
                    num_convs=s["ca_dis_num_convs"][lvl], grad_reverse_lambda=s["ca_grl_weight"][lvl],
                    center_aware_weight=s["center_aware_weight"], center_aware_type=s["center_aware_type"],
                    grl_applied_domain=str(A.GRL_APPLIED_DOMAIN)))
        return out
    s = config.settings(cfg)
    out = {}
    for lvl in DIS_ORDER:
        if A["USE_DIS_%s_CON" % lvl]:
            out["dis_%s_CON" % lvl] = _channels_last_(FCOSDiscriminatorNCHW(
                with_GA=bool(A.CON_WITH_GA), fusion_cfg=str(A.CON_FUSUIN_CFG), num_convs=s["dis_num_convs"][lvl],
                in_channels=256, num_classes=s["num_classes"], grad_reverse_lambda=s["grl_weight"][lvl],
                grl_applied_domain=str(A.GRL_APPLIED_DOMAIN), patch_stride=A.PATCH_STRIDE))
    return out


def build_model(cfg, device="cuda"):
    """the reference's MODEL dict (tools/train_net_da.py:43-48,223-274) out of the factories above, moved to ``device``; without
    MODEL.MIDDLE_HEAD.CONDGRAPH_ON there is no "middle_head" entry (:43-48)"""
    backbone = build_backbone(cfg)
    model = {"backbone": backbone}
    if cfg.MODEL.MIDDLE_HEAD.CONDGRAPH_ON:
        model["middle_head"] = build_middle_head(cfg, backbone.out_channels)
    model["fcos"] = build_rpn(cfg, backbone.out_channels)
    model.update(build_discriminators(cfg))
    for m in model.values():
        m.to(device)
    return model

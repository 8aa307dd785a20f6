"""Conditional Kernel-guided Alignment (CKA) discriminator on one pyramid level.

Mirrors the reference's FCOSDiscriminator_con (fcos_core/modeling/discriminator/
fcos_head_discriminator_con.py:12-126) for the shipped setting (fusion 'concat', GRL on both
inputs, use_bg False, num_classes > 1) with the reference's parameter names
(dis_tower.N, classifier_cls_C.{0,2}).

MI355X restructuring (same arithmetic, fewer and fatter launches): the reference runs, per
foreground class c, cat(x, act[c+1]) -> conv3x3 257->128 -> ReLU -> conv3x3 128->1.  All
classes read the same x, so the 8 first convs are ONE implicit GEMM with 8*128 output channels
over cat(x, act[1:]) (the per-class act channel enters through a block-diagonal weight
slice), and the 8 second convs are ONE skinny conv 1024 -> 8 with a block-diagonal weight.
The class-weighted BCE of all classes is one wavefront-reduction kernel.  With ops.CLS_SPLIT (default) the first GEMM runs on
the 256 feature channels alone and each class's act channel is added in registers by the kernel of the second conv.

Beside it the two discriminators of the EPM baseline (the reference's configs/epm/*.yaml): FCOSDiscriminator (global
alignment, fcos_head_discriminator.py:11-74) and FCOSDiscriminator_CA (centre-aware, fcos_head_discriminator_CA.py:7-124),
on the same towers; the centre-aware map and its row scaling are csrc/center_aware.hip.
"""
import torch
from torch import nn

from .. import ops
from ..layers import GradientReversal
from .backbone import conv_holder
from .fcos import make_tower, run_tower


def _check_epm_keywords(name, grl_applied_domain, patch_stride=None, center_aware_type=None):
    """the EPM discriminators are built for the setting of the reference's configs/epm/*.yaml; anything else names its key"""
    if grl_applied_domain != "both":
        raise ValueError("%s: grl_applied_domain %r is not built (MODEL.ADV.GRL_APPLIED_DOMAIN: only 'both')"
                         % (name, grl_applied_domain))
    if patch_stride is not None:
        raise ValueError("%s: patch_stride %r is not built (MODEL.ADV.PATCH_STRIDE: only None)" % (name, patch_stride))
    if center_aware_type is not None and center_aware_type not in ("ca_feature", "ca_loss"):
        raise ValueError("%s: center_aware_type %r is not built (MODEL.ADV.CENTER_AWARE_TYPE: 'ca_feature' or 'ca_loss')"
                         % (name, center_aware_type))


class FCOSDiscriminator(nn.Module):
    """Global-alignment (GA) discriminator of the EPM baseline on one pyramid level (reference discriminator/
    fcos_head_discriminator.py:11-74): GRL -> num_convs x [conv3x3, GroupNorm(32), ReLU] -> conv3x3 256 -> 1 -> mean BCE against
    the domain label.  Parameter names are the reference's (dis_tower.{0,1,3,4,...}, cls_logits)."""

    def __init__(self, num_convs=2, in_channels=256, grad_reverse_lambda=-1.0, grl_applied_domain="both", patch_stride=None):
        super().__init__()
        _check_epm_keywords(type(self).__name__, grl_applied_domain, patch_stride)
        if num_convs < 0 or in_channels != 256:
            raise ValueError("%s: num_convs %r >= 0 on 256 input channels is what is built (in_channels %r)"
                             % (type(self).__name__, num_convs, in_channels))
        self.num_convs = num_convs
        self.in_channels = in_channels
        self.dis_tower = make_tower(num_convs, in_channels)
        self.cls_logits = conv_holder(in_channels, 1, 3)
        for modules in (self.dis_tower, self.cls_logits):  # reference :44-48
            for m in modules.modules():
                if isinstance(m, nn.Conv2d):
                    nn.init.normal_(m.weight, std=0.01)
                    nn.init.constant_(m.bias, 0)
        self.grad_reverse = GradientReversal(grad_reverse_lambda)
        self.grl_applied_domain = grl_applied_domain

    def _logits(self, feature, shape):
        """[M_l] domain logits; the 256 -> 1 conv is the skinny dense conv the FCOS head's centerness uses"""
        x = run_tower(self.dis_tower, feature, shape, self.num_convs)
        return ops.conv2d(x, self.cls_logits.weight, self.cls_logits.bias, shape, 3, 1)[:, 0]

    def forward(self, feature, target, domain="source", shape=None):
        """feature [M_l, 256] rows of ONE level; shape = that level's PyramidShape."""
        assert target in (0, 1, 0.1, 0.9) and domain in ("source", "target")
        return ops.bce_with_logits_const_mean(self._logits(self.grad_reverse(feature), shape), target)

    def forward_pair(self, feature, shape, n_src, grl_applied=False):
        """source frames [0, n_src) and target frames [n_src, N) of one level in ONE pass through the tower; the source loss
        (label 1.0) is taken on the first n_src images' rows, the target loss (label 0.0) on the rest.  Same values and gradients
        as forward(.., 1.0, 'source') + forward(.., 0.0, 'target') (reference trainer.py:316-318, 359-362).  grl_applied: the
        caller already put the feature behind this module's GRL (ops.split_levels_grl)."""
        if not grl_applied:
            feature = self.grad_reverse(feature)
        (h, w) = shape.sizes[0]
        ls, lt = ops.split_rows2(self._logits(feature, shape), n_src * h * w)
        return ops.bce_with_logits_const_mean(ls, 1.0), ops.bce_with_logits_const_mean(lt, 0.0)


class FCOSDiscriminator_CA(FCOSDiscriminator):
    """Centre-aware (CA) discriminator of the EPM baseline on one level (reference discriminator/
    fcos_head_discriminator_CA.py:7-124).  The map atten = sigmoid(w * max_c sigmoid(cls) * sigmoid(ctr)) of the head's detached
    outputs multiplies the feature in front of the GRL ('ca_feature') or weights the per-location BCE ('ca_loss')."""

    def __init__(self, num_convs=2, in_channels=256, grad_reverse_lambda=-1.0, center_aware_weight=0.0,
                 center_aware_type="ca_loss", grl_applied_domain="both"):
        _check_epm_keywords(type(self).__name__, grl_applied_domain, None, center_aware_type)
        super().__init__(num_convs, in_channels, grad_reverse_lambda, grl_applied_domain)
        self.center_aware_weight = center_aware_weight
        self.center_aware_type = center_aware_type

    def atten_map(self, score_map):
        """score_map {"box_cls": [M_l, C] rows, "centerness": [M_l] or [M_l, 1]} of this level -> atten [M_l], no gradient"""
        cls = score_map["box_cls"]
        return ops.center_aware_map(cls, score_map["centerness"], cls.shape[1], self.center_aware_weight)

    def _input(self, feature, atten, shape):
        """the feature behind this module's GRL: attention-scaled for 'ca_feature' (reference :93), as it is for 'ca_loss'"""
        if self.center_aware_type == "ca_feature":
            return ops.center_aware_split_levels_grl(feature, atten, shape, [self.grad_reverse.lambda_])[0]
        return self.grad_reverse(feature)

    def _loss(self, logits, atten, target):
        return ops.bce_with_logits_const_mean(logits, target, atten if self.center_aware_type == "ca_loss" else None)

    def forward(self, feature, target, score_map=None, domain="source", shape=None):
        assert target in (0, 1, 0.1, 0.9) and domain in ("source", "target")
        atten = self.atten_map(score_map)
        return self._loss(self._logits(self._input(feature, atten, shape), shape), atten, target)

    def forward_pair(self, feature, atten, shape, n_src, grl_applied=False):
        """FCOSDiscriminator.forward_pair with this level's map atten [M_l] (ops.center_aware_map, or atten_map).  grl_applied:
        the caller already formed this module's input (ops.center_aware_split_levels_grl with the map for 'ca_feature',
        without it for 'ca_loss')."""
        if not grl_applied:
            feature = self._input(feature, atten, shape)
        (h, w) = shape.sizes[0]
        m = n_src * h * w
        ls, lt = ops.split_rows2(self._logits(feature, shape), m)
        return self._loss(ls, atten[:m], 1.0), self._loss(lt, atten[m:], 0.0)


class FCOSDiscriminator_con(nn.Module):
    def __init__(self, with_GA=False, fusion_cfg="concat", num_convs=4, in_channels=256, num_classes=9,
                 grad_reverse_lambda=0.02, grl_applied_domain="both", patch_stride=None, cfg=None):
        super().__init__()
        assert fusion_cfg == "concat" and grl_applied_domain == "both" and patch_stride is None and num_classes >= 2, \
            "only the configuration the SCAN yamls use is built"
        self.num_convs = num_convs
        self.in_channels = in_channels
        self.num_classes = num_classes - 1  # use_bg False
        self.dis_tower = make_tower(num_convs, in_channels)
        for c in range(self.num_classes):
            self.add_module("classifier_cls_%d" % c, nn.Sequential(
                conv_holder(in_channels + 1, 128, 3), nn.ReLU(), conv_holder(128, 1, 3)))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, std=0.01)
                nn.init.constant_(m.bias, 0)
        self.grad_reverse = GradientReversal(grad_reverse_lambda)

    def _stacked_weights_torch(self):
        """the stacked weights spelled out in torch ops (what ops.cka_stacked_weights computes in one launch); kept as
        the readable definition and for the test that compares the two"""
        Cf, C = self.num_classes, self.in_channels
        blocks = [getattr(self, "classifier_cls_%d" % c) for c in range(Cf)]
        w0 = torch.stack([b[0].weight for b in blocks], 0)  # [Cf,128,C+1,3,3]
        main = w0[:, :, :C].reshape(Cf * 128, C, 3, 3)
        extra = w0[:, :, C]  # [Cf,128,3,3]: the act-map input channel of each class
        eye = torch.eye(Cf, device=w0.device, dtype=w0.dtype)
        blk = (extra[:, :, None] * eye[:, None, :, None, None]).reshape(Cf * 128, Cf, 3, 3)
        w1 = torch.cat([main, blk], 1)  # [Cf*128, C+Cf, 3, 3]
        b1 = torch.cat([b[0].bias for b in blocks], 0)
        w2s = torch.stack([b[2].weight[0] for b in blocks], 0)  # [Cf,128,3,3]
        w2 = (w2s[:, None] * eye[:, :, None, None, None]).reshape(Cf, Cf * 128, 3, 3)
        b2 = torch.cat([b[2].bias for b in blocks], 0)
        return w1, b1, w2, b2

    def _logits(self, feature, act_maps, shape, grl_applied=False):
        Cf = self.num_classes
        if not grl_applied:  # the caller already put both inputs behind this module's GRL (ops.split_levels_grl)
            feature = self.grad_reverse(feature)
            act_maps = self.grad_reverse(act_maps)
        blocks = [getattr(self, "classifier_cls_%d" % c) for c in range(Cf)]
        if ops.CLS_SPLIT and ops.BATCHED and ops.GROUPED_CLS and ops.cls_split_supported(Cf):
            # the first convs as ONE dense conv on the 256 feature channels (no cat, no pad columns); each class's act-map
            # channel -- 72 multiply-adds per pixel and class -- is added in registers by the grouped conv that reads h.
            # h is stored before its ReLU (the grouped conv applies it to h + act term and masks dh by it).
            x = run_tower(self.dis_tower, feature, shape, self.num_convs)
            wm, e, b1, w2, b2 = ops.cka_stacked_weights_split([(b[0], b[2]) for b in blocks], self.in_channels, 128)
            h = ops.conv2d(x, wm, b1, shape, 3, 1)
            return ops.gconv3x3_to1_act(h, w2, b2, act_maps, e, shape, Cf, 1)[:, :Cf], act_maps
        # cat([x, act[1:]], 1) (reference :104-118) without copying x: the tower's last GroupNorm writes into the first
        # 256 columns of the [M, pad4(256 + Cf)] class-branch input, only the Cf act columns are copied behind them, and
        # the backward hands the GroupNorm its column slice of the conv's data gradient in place
        cs1 = ops.pad4(self.in_channels + Cf)
        if ops.CAT_IN_PLACE and self.num_convs > 0:
            buf = feature.new_empty((feature.shape[0], cs1))
            x = run_tower(self.dis_tower, feature, shape, self.num_convs, out_buf=buf)
            xcat = ops.cat_into(x, act_maps[:, 1:], buf)
        else:
            x = run_tower(self.dis_tower, feature, shape, self.num_convs)
            xcat = torch.cat([x, act_maps[:, 1:]], 1)  # [M, 256 + Cf]; 264 is a multiple of 4
            if cs1 != xcat.shape[1]:
                xcat = torch.nn.functional.pad(xcat, (0, cs1 - xcat.shape[1]))
        if ops.BATCHED and Cf <= ops.CKA_STACK_MAX:  # the one-launch stacking takes 16 branches; more: the torch spelling
            w1, b1, w2, b2 = ops.cka_stacked_weights([(b[0], b[2]) for b in blocks], self.in_channels, 128,
                                                     xcat.shape[1])
        else:
            w1, b1, w2, b2 = self._stacked_weights_torch()
        h = ops.conv2d(xcat, w1, b1, shape, 3, 1, relu="deferred")  # its only consumer masks dx by (h > 0)
        if ops.GROUPED_CLS and 1 <= Cf <= ops.gconv_max_groups():
            # one output channel per class from that class's 128 hidden channels: an HBM-bound grouped kernel instead of
            # a dense conv over the block-diagonal weight (64x the useful multiply-adds)
            if not w2.permute(0, 2, 3, 1).is_contiguous():  # the torch-stacked weight (more than 16 branches)
                w2 = w2.contiguous(memory_format=torch.channels_last)
            return ops.gconv3x3_to1(h, w2, b2, shape, Cf, mask_dx=True)[:, :Cf], act_maps
        return ops.conv2d(h, w2, b2, shape, 3, 1, mask_dx=True)[:, :Cf], act_maps

    def _loss(self, logits, act_maps, target):
        Cf = self.num_classes
        if Cf == 1:
            # single foreground class (Sim10k / KITTI): plain mean BCE, no act-map weight (reference :122-123)
            logits = logits.reshape(-1)
            return ops.bce_with_logits_mean(logits, torch.full_like(logits, float(target)))
        return ops.cka_bce(logits, act_maps.detach(), float(target), Cf)

    def forward(self, feature, target, act_maps=None, domain="source", shape=None):
        """feature [M_l,256], act_maps [M_l,K] rows of ONE level; shape = that level's PyramidShape."""
        assert target in (0, 1, 0.1, 0.9) and domain in ("source", "target")
        logits, act_maps = self._logits(feature, act_maps, shape)
        return self._loss(logits, act_maps, target)

    def forward_pair(self, feature, act_maps, shape, n_src, grl_applied=False):
        """source frames [0, n_src) and target frames [n_src, N) of one level in ONE pass through the tower and the
        class branches; the two domain losses (labels 1.0 / 0.0, each with its own act-map normaliser) are taken on
        the two halves of the rows.  Same values and gradients as forward(.., 1.0, 'source') + forward(.., 0.0,
        'target') (reference trainer.py:314-333, 373-376)."""
        logits, act_maps = self._logits(feature, act_maps, shape, grl_applied)
        (h, w) = shape.sizes[0]
        m = n_src * h * w
        if self.num_classes > 1 and 0 < m < logits.shape[0]:
            # both domain losses as one node: its backward writes the two halves of ONE gradient buffer (ops.cka_bce_pair)
            return ops.cka_bce_pair(logits, act_maps.detach(), m, self.num_classes)
        ls, lt = ops.split_rows2(logits, m)  # one gradient buffer in the backward instead of two zero-filled ones + an add
        return self._loss(ls, act_maps[:m], 1.0), self._loss(lt, act_maps[m:], 0.0)

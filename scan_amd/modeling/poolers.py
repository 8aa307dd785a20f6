"""Region poolers of the reference's two-stage heads (reference modeling/poolers.py:11-133): LevelMapper, Pooler and
make_pooler with the same signatures.  The reference loops over the levels with a ``nonzero`` each and one ROIAlign launch per
level (:116-119); here the levels are packed into one row matrix (ops.pack_levels, csrc/pyramid_pack.hip), the level of every
ROI is computed on the device (ops.roi_levels) and ONE ops.roi_align launch pools all of them (csrc/roi.hip): no host read."""
import torch
from torch import nn

from .. import config, ops
from ..layers import ROIAlign


class LevelMapper(object):
    """reference modeling/poolers.py:11-42: the FPN paper's Eqn. (1) level of every box of a list of BoxLists, as int64
    indices into the pooler's levels.  GPU boxes go through ops.roi_levels, host boxes through the same fp32 formula in torch."""

    def __init__(self, k_min, k_max, canonical_scale=224, canonical_level=4, eps=1e-6):
        self.k_min = k_min
        self.k_max = k_max
        self.s0 = canonical_scale
        self.lvl0 = canonical_level
        self.eps = eps

    def __call__(self, boxlists):
        boxes = torch.cat([b.convert("xyxy").bbox for b in boxlists], dim=0)
        if boxes.is_cuda:
            return ops.roi_levels(boxes.float(), self.k_min, self.k_max, self.s0, self.lvl0, self.eps).long()
        s = torch.sqrt((boxes[:, 2] - boxes[:, 0] + 1) * (boxes[:, 3] - boxes[:, 1] + 1))
        target_lvls = torch.floor(self.lvl0 + torch.log2(s / self.s0 + self.eps))
        target_lvls = torch.clamp(target_lvls, min=self.k_min, max=self.k_max)
        return target_lvls.to(torch.int64) - int(self.k_min)


class Pooler(nn.Module):
    """reference modeling/poolers.py:45-121: Pooler(output_size, scales, sampling_ratio); forward(x: list of NCHW levels,
    boxes: list of BoxList) -> contiguous NCHW [K, C, PH, PW], the ROIs in the order of the concatenated box lists."""

    def __init__(self, output_size, scales, sampling_ratio):
        super().__init__()
        # kept for the reference's module tree and repr; the levels are pooled together in forward
        self.poolers = nn.ModuleList([ROIAlign(output_size, spatial_scale=s, sampling_ratio=sampling_ratio) for s in scales])
        self.output_size = output_size
        self.scales = tuple(float(s) for s in scales)
        self.sampling_ratio = sampling_ratio
        lvl_min = -torch.log2(torch.tensor(scales[0], dtype=torch.float32)).item()
        lvl_max = -torch.log2(torch.tensor(scales[-1], dtype=torch.float32)).item()
        self.map_levels = LevelMapper(lvl_min, lvl_max)

    def convert_to_roi_format(self, boxes):
        concat_boxes = torch.cat([b.convert("xyxy").bbox for b in boxes], dim=0)
        device, dtype = concat_boxes.device, concat_boxes.dtype
        ids = torch.cat([torch.full((len(b), 1), i, dtype=dtype, device=device) for i, b in enumerate(boxes)], dim=0)
        return torch.cat([ids, concat_boxes], dim=1)

    def forward(self, x, boxes):
        if len(x) != len(self.scales):
            raise RuntimeError("Pooler: %d feature levels for %d scales" % (len(x), len(self.scales)))
        rois = self.convert_to_roi_format(boxes).float()
        c = x[0].shape[1]
        rows, shape = ops.pack_levels(x)
        levels = None
        if len(self.scales) > 1:
            m = self.map_levels
            levels = ops.roi_levels(rois, m.k_min, m.k_max, m.s0, m.lvl0, m.eps)
        y = ops.roi_align(rows, shape, rois, self.output_size, self.scales, self.sampling_ratio, levels=levels, c=c)
        return y[..., :c].permute(0, 3, 1, 2).contiguous()


def make_pooler(cfg, head_name):
    """reference modeling/poolers.py:124-133; MODEL[head_name] is read over config.POOLER_DEFAULTS"""
    resolution, scales, sampling_ratio = config.pooler_settings(cfg, head_name)
    return Pooler(output_size=(resolution, resolution), scales=scales, sampling_ratio=sampling_ratio)

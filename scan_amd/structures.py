"""Batch and box containers of the reference's interface: ImageList (fcos_core/structures/image_list.py:8-72) and BoxList with
its helpers (structures/bounding_box.py:9-266, structures/boxlist_ops.py), further down.

The reference collator hands the detector an ImageList: images of different sizes zero-padded at the bottom /
right to a common size that is a multiple of SIZE_DIVISIBILITY (32), plus the true (h, w) of every image, which
inference uses to clip boxes (structures/bounding_box.py:214-224).  The pyramid layout needs nothing else:
padding pixels are ordinary zero-valued pixels of the batch tensor."""
import math

import torch


class ImageList:
    def __init__(self, tensors, image_sizes):
        self.tensors = tensors
        self.image_sizes = [tuple(int(v) for v in s) for s in image_sizes]

    def to(self, *args, **kwargs):
        return ImageList(self.tensors.to(*args, **kwargs), self.image_sizes)


def to_image_list(tensors, size_divisible=0):
    """ImageList | Tensor [N,3,H,W] or [3,H,W] | list of [3,h_i,w_i] -> ImageList."""
    if isinstance(tensors, ImageList):
        return tensors
    if isinstance(tensors, torch.Tensor):
        if size_divisible > 0:
            tensors = [tensors] if tensors.dim() == 3 else list(tensors)
        else:
            if tensors.dim() == 3:
                tensors = tensors[None]
            if tensors.dim() != 4:
                raise ValueError("to_image_list: expected a [N,3,H,W] or [3,H,W] tensor")
            return ImageList(tensors, [t.shape[-2:] for t in tensors])
    if not isinstance(tensors, (list, tuple)):
        raise TypeError("Unsupported type for to_image_list: %s" % type(tensors))
    c = tensors[0].shape[0]
    h = max(t.shape[1] for t in tensors)
    w = max(t.shape[2] for t in tensors)
    if size_divisible > 0:
        h = int(math.ceil(h / size_divisible) * size_divisible)
        w = int(math.ceil(w / size_divisible) * size_divisible)
    batch = tensors[0].new_zeros((len(tensors), c, h, w))
    for t, dst in zip(tensors, batch):
        dst[:, :t.shape[1], :t.shape[2]].copy_(t)
    return ImageList(batch, [t.shape[-2:] for t in tensors])


# ----------------------------------------------------------------------------- BoxList
FLIP_LEFT_RIGHT = 0
FLIP_TOP_BOTTOM = 1
_MODES = ("xyxy", "xywh")


class BoxList:
    """The boxes of ONE image with per-box extra fields (reference fcos_core/structures/bounding_box.py:9-266): what the
    reference's data pipeline hands the detector as ``targets`` and what its post-processor returns as detections.

    bbox [n, 4] fp32, size = (image width, image height), mode "xyxy" or "xywh".  Pixel-index convention of the reference
    (its TO_REMOVE = 1): a box covering pixels x0..x1 has width x1 - x0 + 1, so xywh <-> xyxy, area, the left-right flip and
    the clipping bound all carry that 1.  Plain torch ops on either device: nothing here is on the hot path."""

    def __init__(self, bbox, image_size, mode="xyxy"):
        dev = bbox.device if isinstance(bbox, torch.Tensor) else torch.device("cpu")
        bbox = torch.as_tensor(bbox, dtype=torch.float32, device=dev)
        if bbox.dim() != 2 or bbox.shape[-1] != 4:
            raise ValueError("BoxList: bbox must be [n, 4], got %s" % (tuple(bbox.shape),))
        if mode not in _MODES:
            raise ValueError("BoxList: mode must be 'xyxy' or 'xywh', got %r" % (mode,))
        self.bbox, self.size, self.mode = bbox, tuple(image_size), mode
        self.extra_fields = {}

    # ---- extra fields
    def add_field(self, field, field_data):
        self.extra_fields[field] = field_data

    def get_field(self, field):
        return self.extra_fields[field]

    def has_field(self, field):
        return field in self.extra_fields

    def fields(self):
        return list(self.extra_fields)

    def copy_with_fields(self, fields, skip_missing=False):
        out = BoxList(self.bbox, self.size, self.mode)
        for f in fields if isinstance(fields, (list, tuple)) else [fields]:
            if self.has_field(f):
                out.add_field(f, self.get_field(f))
            elif not skip_missing:
                raise KeyError("Field '%s' not found in %r" % (f, self))
        return out

    def _derived(self, bbox, size, mode, field_op=None):
        """a new BoxList carrying this one's fields; non-tensor fields (masks, keypoints) follow the geometry through field_op"""
        out = BoxList(bbox, size, mode)
        for k, v in self.extra_fields.items():
            if field_op is not None and not isinstance(v, torch.Tensor):
                v = field_op(v)
            out.add_field(k, v)
        return out

    # ---- geometry
    def _xyxy(self):
        """the four corner columns, each [n, 1]"""
        a, b, c, d = self.bbox.split(1, dim=-1)
        if self.mode == "xyxy":
            return a, b, c, d
        return a, b, a + (c - 1).clamp(min=0), b + (d - 1).clamp(min=0)

    def convert(self, mode):
        if mode not in _MODES:
            raise ValueError("BoxList: mode must be 'xyxy' or 'xywh', got %r" % (mode,))
        if mode == self.mode:
            return self
        x0, y0, x1, y1 = self._xyxy()
        cols = (x0, y0, x1, y1) if mode == "xyxy" else (x0, y0, x1 - x0 + 1, y1 - y0 + 1)
        return self._derived(torch.cat(cols, -1), self.size, mode)

    def resize(self, size, *args, **kwargs):
        """the boxes of the image scaled to ``size`` = (width, height)"""
        size = tuple(size)
        rw, rh = (float(s) / float(o) for s, o in zip(size, self.size))
        op = lambda v: v.resize(size, *args, **kwargs)
        if rw == rh:  # one ratio: every column scales alike, in either mode
            return self._derived(self.bbox * rw, size, self.mode, op)
        x0, y0, x1, y1 = self._xyxy()
        return self._derived(torch.cat((x0 * rw, y0 * rh, x1 * rw, y1 * rh), -1), size, "xyxy", op).convert(self.mode)

    def transpose(self, method):
        """FLIP_LEFT_RIGHT or FLIP_TOP_BOTTOM (the reference flips columns as pixel indices, rows as coordinates)"""
        if method not in (FLIP_LEFT_RIGHT, FLIP_TOP_BOTTOM):
            raise NotImplementedError("Only FLIP_LEFT_RIGHT and FLIP_TOP_BOTTOM implemented")
        width, height = self.size
        x0, y0, x1, y1 = self._xyxy()
        if method == FLIP_LEFT_RIGHT:
            cols = (width - x1 - 1, y0, width - x0 - 1, y1)
        else:
            cols = (x0, height - y1, x1, height - y0)
        return self._derived(torch.cat(cols, -1), self.size, "xyxy", lambda v: v.transpose(method)).convert(self.mode)

    def clip_to_image(self, remove_empty=True):
        """clamps the four columns IN PLACE to [0, width - 1] / [0, height - 1]; remove_empty drops boxes with x1 <= x0 or y1 <= y0"""
        w, h = self.size
        for col, hi in ((0, w - 1), (1, h - 1), (2, w - 1), (3, h - 1)):
            self.bbox[:, col].clamp_(min=0, max=hi)
        if remove_empty:
            b = self.bbox
            return self[(b[:, 3] > b[:, 1]) & (b[:, 2] > b[:, 0])]
        return self

    def area(self):
        b = self.bbox
        if self.mode == "xyxy":
            return (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
        return b[:, 2] * b[:, 3]

    # ---- container
    def to(self, device):
        out = BoxList(self.bbox.to(device), self.size, self.mode)
        for k, v in self.extra_fields.items():
            out.add_field(k, v.to(device) if hasattr(v, "to") else v)
        return out

    def __getitem__(self, item):
        out = BoxList(self.bbox[item], self.size, self.mode)
        for k, v in self.extra_fields.items():
            out.add_field(k, v[item])
        return out

    def __len__(self):
        return self.bbox.shape[0]

    def __repr__(self):
        return "BoxList(num_boxes=%d, image_width=%s, image_height=%s, mode=%s)" % (len(self), self.size[0], self.size[1],
                                                                                  self.mode)


# ----------------------------------------------------------------------------- SegmentationMask (binary-mask mode)
class BinaryMaskList:
    """The binary masks of ONE image's objects (reference structures/segmentation_mask.py:33-172): masks uint8 [n, H, W],
    size = (image width, image height).  Plain torch ops: the head's targets are made on the device from the masks themselves
    (ops.roi_mask_targets), not through crop / resize."""

    def __init__(self, masks, size):
        if isinstance(masks, BinaryMaskList):
            masks = masks.masks
        elif isinstance(masks, (list, tuple)):
            if not masks or not all(isinstance(m, torch.Tensor) for m in masks):
                raise ValueError("BinaryMaskList: a list of masks must hold [H, W] tensors (RLE dicts are not built)")
            masks = torch.stack(list(masks), 0)
        elif not isinstance(masks, torch.Tensor):
            raise ValueError("BinaryMaskList: masks must be a tensor, a list of tensors or a BinaryMaskList, got %s" % type(masks))
        masks = masks.clone()
        if masks.dim() == 2:
            masks = masks[None]
        size = tuple(int(s) for s in size)
        if masks.dim() != 3 or tuple(masks.shape[1:]) != (size[1], size[0]):
            raise ValueError("BinaryMaskList: masks %r for an image of (width, height) %r" % (tuple(masks.shape), size))
        self.masks, self.size = masks, size

    def transpose(self, method):
        if method not in (FLIP_LEFT_RIGHT, FLIP_TOP_BOTTOM):
            raise NotImplementedError("Only FLIP_LEFT_RIGHT and FLIP_TOP_BOTTOM implemented")
        return BinaryMaskList(self.masks.flip(1 if method == FLIP_TOP_BOTTOM else 2), self.size)

    def crop(self, box):
        """box xyxy: every coordinate rounded half-to-even (Python's round), the minima clamped into the image, the maxima to its
        far edge, at least one pixel each way"""
        width, height = self.size
        xmin, ymin, xmax, ymax = [round(float(b)) for b in box]
        xmin, ymin = min(max(xmin, 0), width - 1), min(max(ymin, 0), height - 1)
        xmax, ymax = min(max(xmax, 0), width), min(max(ymax, 0), height)
        xmax, ymax = max(xmax, xmin + 1), max(ymax, ymin + 1)
        return BinaryMaskList(self.masks[:, ymin:ymax, xmin:xmax], (xmax - xmin, ymax - ymin))

    def resize(self, size):
        """bilinear (align_corners=False) in fp32, cast back to the masks' dtype as the reference does"""
        width, height = (int(size), int(size)) if isinstance(size, (int, float)) else (int(s) for s in size)
        if width < 1 or height < 1:
            raise ValueError("BinaryMaskList.resize: size %r" % (size,))
        m = torch.nn.functional.interpolate(self.masks[None].float(), size=(height, width), mode="bilinear", align_corners=False)
        return BinaryMaskList(m[0].type_as(self.masks), (width, height))

    def to(self, *args, **kwargs):
        return self

    def __len__(self):
        return self.masks.shape[0]

    def __getitem__(self, index):
        if isinstance(index, torch.Tensor):
            index = index.to(self.masks.device)
        return BinaryMaskList(self.masks[index], self.size)

    def __iter__(self):
        return iter(self.masks)

    def __repr__(self):
        return "BinaryMaskList(num_instances=%d, image_width=%d, image_height=%d)" % (len(self), self.size[0], self.size[1])


class SegmentationMask:
    """reference structures/segmentation_mask.py:437-533 in mode "mask" (the ``masks`` field of a target BoxList).  Polygon
    mode rasterises through pycocotools and is not built: mode="poly" raises, so ``mode`` must be given."""

    def __init__(self, instances, size, mode="poly"):
        if mode != "mask":
            raise ValueError("SegmentationMask: mode %r is not built (only mode='mask', binary masks [n, H, W])" % (mode,))
        if isinstance(instances, SegmentationMask):
            instances = instances.instances
        self.instances = BinaryMaskList(instances, size)
        self.mode, self.size = mode, self.instances.size

    def transpose(self, method):
        return SegmentationMask(self.instances.transpose(method), self.size, self.mode)

    def crop(self, box):
        c = self.instances.crop(box)
        return SegmentationMask(c, c.size, self.mode)

    def resize(self, size, *args, **kwargs):
        r = self.instances.resize(size)
        return SegmentationMask(r, r.size, self.mode)

    def to(self, *args, **kwargs):
        return self

    def convert(self, mode):
        if mode != "mask":
            raise ValueError("SegmentationMask.convert: mode %r is not built (only 'mask')" % (mode,))
        return self

    def get_mask_tensor(self):
        return self.instances.masks.squeeze(0)

    def __len__(self):
        return len(self.instances)

    def __getitem__(self, item):
        return SegmentationMask(self.instances[item], self.size, self.mode)

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def __repr__(self):
        return "SegmentationMask(num_instances=%d, image_width=%d, image_height=%d, mode=%s)" % (len(self), self.size[0],
                                                                                                 self.size[1], self.mode)


def cat_boxlist(bboxes):
    """list of BoxList of one image size, mode and field set -> one BoxList (reference structures/boxlist_ops.py:127-153)"""
    if not isinstance(bboxes, (list, tuple)) or not bboxes or not all(isinstance(b, BoxList) for b in bboxes):
        raise TypeError("cat_boxlist: a non-empty list of BoxList is needed")
    first = bboxes[0]
    if any(b.size != first.size or b.mode != first.mode or set(b.fields()) != set(first.fields()) for b in bboxes):
        raise ValueError("cat_boxlist: image size, mode and fields must agree")
    out = BoxList(torch.cat([b.bbox for b in bboxes], 0), first.size, first.mode)
    for f in first.fields():
        out.add_field(f, torch.cat([b.get_field(f) for b in bboxes], 0))
    return out


def remove_small_boxes(boxlist, min_size):
    """keeps the boxes whose width AND height (pixel counts, the + 1 included) are >= min_size (boxlist_ops.py:59-73)"""
    wh = boxlist.convert("xywh").bbox
    return boxlist[((wh[:, 2] >= min_size) & (wh[:, 3] >= min_size)).nonzero().squeeze(1)]

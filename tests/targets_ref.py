"""Oracle and input cases of the ground-truth plan tests (a helper module, not a conftest): numpy only in the arithmetic, and
nothing here imports scan_amd.  tests/test_targets_host.py pins it on the CPU against the torch spelling (modeling/fcos.py:
assign_targets, source_node_index, centerness_targets) and the reference's label maps; tests/test_gpu_targets.py holds the three
kernels of scan_amd/csrc/targets.hip (scan_fcos_assign / _compact / _nodes) to it bit for bit.

The operation.  Rows are pyramid rows (level-major, image, y, x).  The location of row (l, n, y, x) is
(x s + s // 2, y s + s // 2) with s = strides[l], exact in fp32.  For a row of image n and each of that image's ng[n] boxes
(x0, y0, x1, y1), IN BOX ORDER, in fp32 with every operation rounded on its own:
    l = xs - x0,  t = ys - y0,  r = x1 - xs,  b = y1 - ys,   mn = min(l, t, r, b),   mx = max(l, t, r, b)
    cost = (x1 - x0 + 1) (y1 - y0 + 1)   when  mn > 0  and  lo <= mx <= hi       (lo, hi) = soi[level of the row]
         = 1e8                            otherwise
    winner = the FIRST box index at which the cost is the row's minimum
    label  = 0 when that minimum is 1e8 or the image has no box, else the winner's label
    reg    = the winner's (l, t, r, b) on EVERY row -- box 0's when nothing qualifies, (0, 0, 0, 0) when the image has no box
The three comparisons are what the cases below sit on: ``mn > 0`` is strict (a location on a box edge is outside), the size
range is inclusive at both ends (a side of exactly 64, 128, 256 or 512 is cared for by two adjacent levels) and among equal
costs the first box wins.

What the reference does there (fcos_core/modeling/rpn/fcos/loss.py:40-126).  ``is_in_boxes = reg.min(dim=2)[0] > 0`` and
``(max >= soi[:, [0]]) & (max <= soi[:, [1]])`` are the same strict / inclusive comparisons; the areas of boxes that fail
either are overwritten with INF = 100000000 and ``locations_to_gt_area.min(dim=1)`` picks the box, labels where the minimum
``== INF`` become 0, and the regression targets are gathered with the picked index on every row (box 0's where all are INF,
since every cost is equal there).  The index ``Tensor.min(dim)`` returns among EQUAL values is not specified by torch; its CPU
kernel returns the first, and that is the rule this project fixed (the torch spelling runs on the CPU in the tests that pin it
to the reference's label maps).  The reference cannot take an image without boxes (``min`` over an empty dimension raises);
label 0 and zero targets there are this library's.

Compaction: per level, the rows with label > 0 in row order and the rows with label <= 0 in row order.  Node sampling
(loss.py:428-463): per level with np_ positives and nn background rows, ``floor(linspace(0, nn - 2, np_))`` (fp64, as numpy
forms it) of the background list when np_ <= nn, else all of it; the order is every level's picked background rows, then every
level's positives.  Centerness target (loss.py:128-133) of a positive: sqrt((min(l, r) / max(l, r)) (min(t, b) / max(t, b))),
fp32, each operation rounded on its own.
"""
import functools

import numpy as np

F32 = np.float32
INF = 100000000  # exactly representable in fp32
STRIDES = (8, 16, 32, 64, 128)
SOI = ((-1, 64), (64, 128), (128, 256), (256, 512), (512, INF))


class Shape:
    """the level table of a pyramid: n_images, sizes, row_off (what scan_amd.ops.PyramidShape carries)"""

    def __init__(self, n_images, sizes):
        self.n_images = int(n_images)
        self.sizes = [(int(h), int(w)) for h, w in sizes]
        self.row_off = [0]
        for h, w in self.sizes:
            self.row_off.append(self.row_off[-1] + self.n_images * h * w)
        self.rows = self.row_off[-1]
        self.n_levels = len(self.sizes)


def pyramid_sizes(H, W, n_levels=5):
    return [(H // s, W // s) for s in STRIDES[:n_levels]]


# ----------------------------------------------------------------------------- the oracle
def locations(sizes, strides):
    """per level [h w, 2] fp32 (x, y), x fastest: x * s + s // 2"""
    out = []
    for (h, w), s in zip(sizes, strides):
        xs = (np.arange(w, dtype=np.int64) * s + s // 2).astype(F32)
        ys = (np.arange(h, dtype=np.int64) * s + s // 2).astype(F32)
        out.append(np.stack([np.tile(xs, h), np.repeat(ys, w)], 1))
    return out


def _candidates(sizes, N, boxes, ng, strides, soi):
    """for every (level, image) with at least one box: (level, image, first row, l / t / r / b [hw, g, 4], mn, mx, cost [hw, g],
    qualifies [hw, g]) -- the boxes in their own order along axis 1, fp32 throughout"""
    boxes = np.asarray(boxes, dtype=F32)
    shape = Shape(N, sizes)
    locs = locations(sizes, strides)
    for l, (h, w) in enumerate(sizes):
        lo, hi = F32(soi[l][0]), F32(soi[l][1])
        xs, ys = locs[l][:, 0], locs[l][:, 1]
        for n in range(N):
            g = int(ng[n])
            if g == 0:
                continue
            b = boxes[n, :g]
            ltrb = np.empty((h * w, g, 4), dtype=F32)
            cost = np.empty((h * w, g), dtype=F32)
            for k in range(g):  # box by box, in the image's order
                ltrb[:, k, 0] = xs - b[k, 0]
                ltrb[:, k, 1] = ys - b[k, 1]
                ltrb[:, k, 2] = b[k, 2] - xs
                ltrb[:, k, 3] = b[k, 3] - ys
            mn, mx = ltrb.min(2), ltrb.max(2)
            ok = (mn > F32(0)) & (mx >= lo) & (mx <= hi)
            for k in range(g):
                area = F32(F32(F32(b[k, 2] - b[k, 0]) + F32(1)) * F32(F32(b[k, 3] - b[k, 1]) + F32(1)))
                cost[:, k] = np.where(ok[:, k], area, F32(INF))
            yield l, n, shape.row_off[l] + n * h * w, ltrb, mn, mx, cost, ok


def assign(sizes, N, boxes, glabels, ng, strides=STRIDES, soi=SOI):
    """-> labels [M] int64, reg [M, 4] fp32, level_pos [L] (positives per level).  boxes [N, G, 4] xyxy, glabels [N, G], ng [N];
    slots g >= ng[n] are never looked at."""
    shape = Shape(N, sizes)
    glabels = np.asarray(glabels, dtype=np.int64)
    labels = np.zeros((shape.rows,), dtype=np.int64)
    reg = np.zeros((shape.rows, 4), dtype=F32)
    for l, n, r0, ltrb, mn, mx, cost, ok in _candidates(sizes, N, boxes, ng, strides, soi):
        rows, g = cost.shape
        least = cost.min(1)
        winner = np.full((rows,), -1, dtype=np.int64)
        for k in range(g - 1, -1, -1):  # the smallest index that reaches the minimum is written last
            winner[cost[:, k] == least] = k
        assert (winner >= 0).all()
        labels[r0:r0 + rows] = np.where(least == F32(INF), 0, glabels[n, winner])
        reg[r0:r0 + rows] = ltrb[np.arange(rows), winner]
    level_pos = np.array([int((labels[shape.row_off[l]:shape.row_off[l + 1]] > 0).sum()) for l in range(shape.n_levels)],
                         dtype=np.int64)
    return labels, reg, level_pos


def edge_counts(sizes, N, boxes, ng, strides=STRIDES, soi=SOI):
    """how often the inputs sit ON the three comparisons: rows where more than one qualifying box shares the minimum cost;
    (row, box) pairs with the location strictly inside the box and mx == lo or mx == hi (there the size comparison alone
    decides); pairs with mn == 0, and those of them whose mx is in the level's range (there ``mn > 0`` alone decides)"""
    c = {"tie_rows": int(tie_rows(sizes, N, boxes, ng, strides, soi).sum()), "mx_eq_lo": 0, "mx_eq_hi": 0, "mn_eq_0": 0,
         "mn_eq_0_in_range": 0}
    for l, n, r0, ltrb, mn, mx, cost, ok in _candidates(sizes, N, boxes, ng, strides, soi):
        lo, hi = F32(soi[l][0]), F32(soi[l][1])
        c["mx_eq_lo"] += int(((mn > 0) & (mx == lo)).sum())
        c["mx_eq_hi"] += int(((mn > 0) & (mx == hi)).sum())
        c["mn_eq_0"] += int((mn == 0).sum())
        c["mn_eq_0_in_range"] += int(((mn == 0) & (mx >= lo) & (mx <= hi)).sum())
    return c


def tie_rows(sizes, N, boxes, ng, strides=STRIDES, soi=SOI):
    """boolean [M]: rows where more than one qualifying box shares the minimum cost"""
    out = np.zeros((Shape(N, sizes).rows,), dtype=bool)
    for l, n, r0, ltrb, mn, mx, cost, ok in _candidates(sizes, N, boxes, ng, strides, soi):
        least = cost.min(1)
        out[r0:r0 + len(least)] = (least != F32(INF)) & ((cost == least[:, None]).sum(1) > 1)
    return out


def compact(labels, row_off):
    """per level (rows with label > 0, rows with label <= 0), each in row order, as pyramid row indices"""
    out = []
    for l in range(len(row_off) - 1):
        rows = np.arange(row_off[l], row_off[l + 1], dtype=np.int64)
        lab = np.asarray(labels[row_off[l]:row_off[l + 1]])
        out.append((rows[lab > 0], rows[lab <= 0]))
    return out


def pick(np_, nn):
    """indices into a level's background list: floor(linspace(0, nn - 2, np_)) when np_ <= nn, else all of it"""
    if np_ <= nn:
        return np.floor(np.linspace(0, nn - 2, np_)).astype(np.int64)
    return np.arange(nn, dtype=np.int64)


def centerness(reg):
    reg = np.asarray(reg, dtype=F32)
    lr = np.minimum(reg[:, 0], reg[:, 2]) / np.maximum(reg[:, 0], reg[:, 2])
    tb = np.minimum(reg[:, 1], reg[:, 3]) / np.maximum(reg[:, 1], reg[:, 3])
    out = np.sqrt(lr * tb)
    assert out.dtype == F32
    return out


def nodes(labels, reg, row_off):
    """-> dict(node_index, node_labels, pos_inds, reg_pos, ctr_pos, level_pos); order [all picked negatives level by level, all
    positives level by level]"""
    labels = np.asarray(labels, dtype=np.int64)
    lists = compact(labels, row_off)
    neg = [n[pick(len(p), len(n))] for p, n in lists]
    pos_inds = np.concatenate([p for p, _ in lists]) if lists else np.zeros((0,), dtype=np.int64)
    neg = np.concatenate(neg)
    reg_pos = np.asarray(reg, dtype=F32)[pos_inds]
    return {"node_index": np.concatenate([neg, pos_inds]),
            "node_labels": np.concatenate([np.zeros((len(neg),), dtype=np.int64), labels[pos_inds]]),
            "pos_inds": pos_inds, "reg_pos": reg_pos, "ctr_pos": centerness(reg_pos),
            "level_pos": np.array([len(p) for p, _ in lists], dtype=np.int64)}


# ----------------------------------------------------------------------------- the cases
class Case:
    """inputs of one batch: per-image (boxes [g, 4] fp32, labels [g] int64) and the same padded to G slots per image (``fill``:
    what the slots past an image's count hold), with the oracle's outputs and the property counts measured on them"""

    def __init__(self, name, H, W, targets, n_levels=5, G=None, pad_box=0.0, pad_label=0):
        self.name, self.H, self.W = name, H, W
        self.sizes = pyramid_sizes(H, W, n_levels)
        self.strides, self.soi = STRIDES[:n_levels], SOI[:n_levels]
        self.targets = [(np.asarray(b, dtype=F32).reshape(-1, 4), np.asarray(l, dtype=np.int64).reshape(-1)) for b, l in targets]
        self.N = len(self.targets)
        self.shape = Shape(self.N, self.sizes)
        self.ng = np.array([len(b) for b, _ in self.targets], dtype=np.int32)
        self.G = int(G or max(1, self.ng.max()))
        self.boxes = np.full((self.N, self.G, 4), pad_box, dtype=F32)
        self.glabels = np.full((self.N, self.G), pad_label, dtype=np.int64)
        for n, (b, l) in enumerate(self.targets):
            self.boxes[n, :len(b)] = b
            self.glabels[n, :len(b)] = l
        self.labels, self.reg, self.level_pos = assign(self.sizes, self.N, self.boxes, self.glabels, self.ng, self.strides, self.soi)
        self.nodes = nodes(self.labels, self.reg, self.shape.row_off)
        self.counts = edge_counts(self.sizes, self.N, self.boxes, self.ng, self.strides, self.soi)
        self.counts["level_pos"] = [int(v) for v in self.level_pos]
        self.counts["n_nodes"] = int(len(self.nodes["node_index"]))
        self.all_images_have_boxes = bool((self.ng > 0).all())

    def torch_targets(self, device=None):
        """[(boxes, labels)] as torch tensors, on the host unless a device is given"""
        import torch
        return [(torch.from_numpy(b.copy()).to(device or "cpu"), torch.from_numpy(l.copy()).to(device or "cpu"))
                for b, l in self.targets]


TIE_BOXES = [[20, 16, 100, 80], [20, 16, 100, 80], [36, 8, 100, 88], [24, 20, 104, 84]]  # all of area 81 x 65, the first two equal
TIE_LABELS = [2, 5, 7, 3]
GRID_SEED = 7


def integer_grid_targets(n_images=2, per_image=6, H=128, W=256, seed=GRID_SEED):
    """corners on multiples of 4, the way annotation files have them: x0, y0 in 4 [0, 24), w, h in 4 [2, 40), clamped to the image"""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n_images):
        xy = 4 * rs.randint(0, 24, (per_image, 2))
        wh = 4 * rs.randint(2, 40, (per_image, 2))
        b = np.concatenate([xy, np.minimum(xy + wh, [W, H])], 1).astype(F32)
        out.append((b, rs.randint(1, 9, (per_image,))))
    return out


def _build(name):
    if name == "ties":
        return Case(name, 128, 256, [(TIE_BOXES, TIE_LABELS)])
    if name == "ties_reversed":
        return Case(name, 128, 256, [(TIE_BOXES[::-1], TIE_LABELS[::-1])])
    if name == "integer_grid":
        return Case(name, 128, 256, integer_grid_targets())
    if name == "zero_positives":  # no location centre lies strictly inside either box
        return Case(name, 128, 256, [([[5, 5, 7, 7], [13, 21, 19, 27]], [1, 2])])
    if name == "one_positive":
        return Case(name, 128, 256, [([[1, 1, 7, 7]], [4])])
    if name == "covers_everything":
        return Case(name, 128, 256, [([[-600, -600, 900, 800]], [6])])
    if name == "ragged_with_empty_image":  # ng = [4, 0, 1] in G = 7 slots; what lies past an image's count must never be read
        return Case(name, 128, 256, [(TIE_BOXES, TIE_LABELS), (np.zeros((0, 4)), np.zeros((0,))), ([[40, 24, 200, 120]], [8])],
                    G=7, pad_box=np.nan, pad_label=999)
    if name == "few_levels_1":
        return Case(name, 128, 256, integer_grid_targets(), n_levels=1)
    if name == "few_levels_3":
        return Case(name, 128, 256, integer_grid_targets(), n_levels=3)
    raise KeyError(name)


CASES = ("ties", "ties_reversed", "integer_grid", "zero_positives", "one_positive", "covers_everything",
         "ragged_with_empty_image", "few_levels_1", "few_levels_3")
PLAN_CASES = tuple(c for c in CASES if c != "ragged_with_empty_image")  # every image has a box: the torch spelling can take them


@functools.lru_cache(maxsize=None)
def case(name):
    """built once per process and shared; treat what it returns as read-only"""
    return _build(name)


def case_from_targets(name, H, W, targets, n_levels=5):
    """a Case of torch or numpy (boxes, labels) pairs"""
    return Case(name, H, W, [(np.asarray(b, dtype=F32), np.asarray(l, dtype=np.int64)) for b, l in targets], n_levels)


# ----------------------------------------------------------------------------- synthetic label vectors (compaction, node sampling)
LEVEL_SIZES = {1: (1, 1), 2: (1, 2), 63: (7, 9), 64: (8, 8), 65: (5, 13), 1023: (31, 33), 1024: (32, 32), 1025: (25, 41),
               2049: (3, 683)}
LABEL_PYRAMIDS = ((1, 2, 63, 64, 65), (1023, 1024, 1025, 2049, 2), (2049, 1, 1025, 64, 1024), (65, 1023, 63), (2049,))
PATTERNS = ("all_background", "all_positive", "first_row", "last_row", "row_63", "row_64", "row_1023", "row_1024",
            "one_background", "alternating_from_1", "alternating_from_0", "half_minus", "random_10_percent")


def level_labels(rows, pattern, rs):
    """labels [rows] of one level.  A single-row pattern whose row the level does not have leaves the level all background (an
    empty level between others); alternating_from_1 has np == nn on an even level and np == nn - 1 on an odd one,
    alternating_from_0 np == nn + 1 on an odd one; half_minus is np == nn - 1 (odd) or nn - 2 (even) with the positives first."""
    pos = np.zeros((rows,), dtype=bool)
    if pattern == "all_positive":
        pos[:] = True
    elif pattern == "first_row":
        pos[0] = True
    elif pattern == "last_row":
        pos[rows - 1] = True
    elif pattern.startswith("row_"):
        k = int(pattern[4:])
        if k < rows:
            pos[k] = True
    elif pattern == "one_background":
        pos[:] = True
        pos[rows // 2] = False
    elif pattern == "alternating_from_1":
        pos[1::2] = True
    elif pattern == "alternating_from_0":
        pos[0::2] = True
    elif pattern == "half_minus":
        pos[:(rows - 1) // 2] = True
    elif pattern == "random_10_percent":
        pos = rs.rand(rows) < 0.1
    else:
        assert pattern == "all_background", pattern
    return np.where(pos, rs.randint(1, 9, (rows,)), 0).astype(np.int64)


def label_cases():
    """[(sizes of a one-image pyramid, labels [M], reg [M, 4] with positive entries, per-level pattern names)]: every pyramid of
    LABEL_PYRAMIDS with every rotation of PATTERNS over its levels (level i of rotation k has pattern (k + 3 i) mod 13, so every
    level meets every pattern and neighbouring levels differ), and one pyramid that is all background"""
    rs = np.random.RandomState(11)
    out = []
    for pyr in LABEL_PYRAMIDS:
        for k in range(len(PATTERNS)):
            names = [PATTERNS[(k + 3 * i) % len(PATTERNS)] for i in range(len(pyr))]
            labels = np.concatenate([level_labels(r, p, rs) for r, p in zip(pyr, names)])
            reg = rs.uniform(0.5, 100.0, (len(labels), 4)).astype(F32)
            out.append(([LEVEL_SIZES[r] for r in pyr], labels, reg, names))
    pyr = (65, 1, 1025)
    out.append(([LEVEL_SIZES[r] for r in pyr], np.zeros((sum(pyr),), dtype=np.int64),
                rs.uniform(0.5, 100.0, (sum(pyr), 4)).astype(F32), ["all_background"] * 3))
    return out

"""ROIAlign / ROIPool / LevelMapper / Pooler on the GPU (csrc/roi.hip) against the restatement of tests/roi_ref.py.

Shapes are the smallest at which the kernels can still go wrong: N = 2, a three-level pyramid 13x17 / 7x9 / 4x5 with scales
1/4, 1/8, 1/16, C in {3, 4, 68, 256} at the natural and at a larger pitch, pooled sizes (1, 1), (2, 3), (7, 7), sampling_ratio
0..3, K in {0, 1, 65, 257}.  257 ROIs of 7 x 7 bins are 12,593 (ROI, bin) items, more than the 8,192 waves of the forward
launches' grid cap; the gradients give one wave to a row of dx, and a 2 x 100 x 60 map has 12,000 of them.

The error bounds are derived from the operation counts in roi_ref (align_forward_bound, align_backward_bound,
pool_backward_bound: gamma(n) = n u / (1 - n u), u = 2^-24, n = the number of roundings a term can pass through), relative
to the sums of absolute terms the restatement computes next to the values -- never from what the kernels return.

    forward   4 products + 3 sums per sample, g_h g_w additions (the first one exact), one division:  gamma(g_h g_w + 5)
    backward  a product and a quotient per contribution, m additions (the first one exact):            gamma(m + 2)

Sample positions, weights and cells are compared bit for bit (scan_roi_align_samples), ROIPool values and argmax exactly.
The worst measured ratios to the bounds are printed (python -m pytest -s) and recorded by tools/roi_bench.py."""
import functools
import importlib
import json
import os
import sys

import numpy as np
import pytest
import torch

import roi_ref as R
from scan_amd import _C as C_ctypes, layers, ops
from scan_amd.modeling import poolers
from scan_amd.structures import BoxList

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SIZES_P = [(1, 1), (2, 3), (7, 7)]
RATIOS = [0, 1, 2, 3]
CHANNELS = [(3, 4), (4, 4), (68, 68), (256, 256), (3, 8), (68, 72)]  # (C, Cs): the natural pitch and a larger one
K_ALL = 257


def _shape(sizes=R.SIZES):
    return ops.PyramidShape(R.N_IMAGES, list(sizes))


@functools.lru_cache(maxsize=None)
def _rois(K):
    rois, lv = R.make_rois(K)
    return rois, lv, rois.tolist(), lv.tolist()


@functools.lru_cache(maxsize=None)
def _x(C, kind="randn"):
    x = R.make_rows(C, 7 + C)
    if kind == "ties":
        x = torch.round(x * 1.5)  # few distinct values: equal maxima inside most bins
    elif kind == "negative":
        x = -x.abs() - 1.0
    return x


def _padded(x, Cs, fill=7.5):
    """rows [M, Cs] on the device whose padding columns hold garbage the kernels must not read into their results"""
    out = torch.full((x.shape[0], Cs), fill)
    out[:, :x.shape[1]] = x
    return out.to(DEV)


@functools.lru_cache(maxsize=None)
def _align_ref(C, size, sr, K):
    _, _, rl, ll = _rois(K)
    return R.roi_align(_x(C), rl, ll, size[0], size[1], sr)


def _report(what, ratio):
    print("\n[roi] %s: worst |error| / bound = %.3f" % (what, ratio))


# ----------------------------------------------------------------------------- LevelMapper
def test_device_levels_equal_the_references(gold_dir):
    gold = json.load(open(os.path.join(gold_dir, "roi_levels.json")))
    for name, c in gold.items():
        boxes = torch.tensor(c["boxes"], dtype=torch.float64).float()
        lv = ops.roi_levels(boxes.to(DEV), c["k_min"], c["k_max"])
        assert lv.dtype == torch.int32 and lv.cpu().tolist() == c["levels"], name
        rois = torch.cat([torch.zeros(len(boxes), 1), boxes], 1).to(DEV)  # the [K, 5] form
        assert ops.roi_levels(rois, c["k_min"], c["k_max"]).cpu().tolist() == c["levels"], name
        lists = [BoxList(boxes[:c["split"]].to(DEV), (4096, 4096)), BoxList(boxes[c["split"]:].to(DEV), (4096, 4096))]
        got = poolers.LevelMapper(c["k_min"], c["k_max"])(lists)
        assert got.dtype == torch.int64 and got.cpu().tolist() == c["levels"], name
    assert ops.roi_levels(torch.zeros(0, 5, device=DEV), 2, 5).shape == (0,)


# ----------------------------------------------------------------------------- ROIAlign forward
@pytest.mark.parametrize("sr", RATIOS)
@pytest.mark.parametrize("size", SIZES_P)
def test_align_samples_bit_equal(size, sr):
    """positions, grids, weights and cells of every sample of every ROI, bit for bit"""
    rois, lv, rl, ll = _rois(K_ALL)
    refs = [R.align_samples(rl[k], ll[k], size[0], size[1], sr) for k in range(K_ALL)]
    gmax = max(max(s["g"]) for s in refs if s is not None)
    grid, pos, wgt, cell = [t.cpu().numpy() for t in ops.roi_align_samples(_shape(), rois.to(DEV), size, R.SCALES, sr, gmax,
                                                                           levels=lv.to(DEV))]
    seen = set()
    for k, s in enumerate(refs):
        if s is None:
            assert grid[k].tolist() == [0, 0] and not wgt[k].any() and (cell[k] == -1).all()
            continue
        gh, gw = s["g"]
        assert grid[k].tolist() == [gh, gw], k
        H = R.SIZES[ll[k]][0]
        py = pos[k, :, 0, :gh, 0, 0].reshape(-1)  # [PH, gh]
        px = pos[k, 0, :, 0, :gw, 1].reshape(-1)
        assert np.array_equal(py.view(np.int32), s["pos_y"].view(np.int32)), k
        assert np.array_equal(px.view(np.int32), s["pos_x"].view(np.int32)), k
        w = wgt[k, :, :, :gh, :gw].transpose(4, 0, 2, 1, 3).reshape(4, size[0] * gh, size[1] * gw)
        c = cell[k, :, :, :gh, :gw].transpose(4, 0, 2, 1, 3).reshape(4, size[0] * gh, size[1] * gw)
        assert np.array_equal(w.view(np.int32), s["w"].view(np.int32)), k
        assert np.array_equal(c, s["cell"]), k
        assert not wgt[k, :, :, gh:].any() and not wgt[k, :, :, :, gw:].any()
        if (py == H).any():
            seen.add("y == H")
        if ((py > -1) & (py <= 0)).any():
            seen.add("(-1, 0]")
        if (py == -1).any():
            seen.add("y == -1")
        if not s["live"].any():
            seen.add("all outside")
        if max(gh, gw) > 8:
            seen.add("grid > 8")
    assert {"(-1, 0]", "all outside"} <= seen
    if size == (1, 1) and sr == 1:
        assert {"y == H", "y == -1"} <= seen  # the hand-made border ROIs of roi_ref.special_rois
    if size == (1, 1) and sr == 0:
        assert "grid > 8" in seen  # the whole map and the ROI beyond it: the cut walk of a large adaptive grid


@pytest.mark.parametrize("sr", RATIOS)
@pytest.mark.parametrize("size", SIZES_P)
def test_align_forward(size, sr):
    C, Cs = CHANNELS[(SIZES_P.index(size) * len(RATIOS) + sr) % len(CHANNELS)]
    _check_align_forward(C, Cs, size, sr, K_ALL)


@pytest.mark.parametrize("C,Cs", CHANNELS)
def test_align_forward_every_channel_count(C, Cs):
    _check_align_forward(C, Cs, (2, 3), 2, 65)


@pytest.mark.parametrize("K", [0, 1, 65])
def test_align_forward_roi_counts(K):
    _check_align_forward(68, 68, (7, 7), 0, K)


def _check_align_forward(C, Cs, size, sr, K):
    rois, lv, _, _ = _rois(K)
    y = ops.roi_align(_padded(_x(C), Cs), _shape(), rois.to(DEV), size, R.SCALES, sr, levels=lv.to(DEV), c=C)
    assert tuple(y.shape) == (K, size[0], size[1], Cs) and y.is_contiguous()
    if K == 0:
        return
    ref = _align_ref(C, size, sr, K)
    y = y.cpu()
    assert float(y[..., C:].abs().max()) == 0.0 if Cs > C else True  # padding columns are written as zeros
    err = (y[..., :C].double() - ref["y"]).abs()
    bound = R.align_forward_bound(ref)
    _report("align forward C=%d Cs=%d %s sr=%d K=%d" % (C, Cs, size, sr, K), float((err / bound).max()))
    assert bool((err <= bound).all())
    for k in np.nonzero(ref["terms"] == 0)[0]:  # image -1 / N, level outside the pyramid
        assert float(y[k].abs().max()) == 0.0


# ----------------------------------------------------------------------------- ROIPool forward
@pytest.mark.parametrize("kind", ["randn", "ties", "negative"])
@pytest.mark.parametrize("size", SIZES_P)
def test_pool_forward_exact(size, kind):
    C, Cs = CHANNELS[(SIZES_P.index(size) * 3 + ["randn", "ties", "negative"].index(kind)) % len(CHANNELS)]
    rois, lv, rl, ll = _rois(K_ALL)
    x = _x(C, kind)
    y, am = ops.roi_pool(_padded(x, Cs), _shape(), rois.to(DEV), size, R.SCALES, levels=lv.to(DEV), c=C, return_argmax=True)
    ry, ram = R.roi_pool(x, rl, ll, size[0], size[1])
    assert am.dtype == torch.int32 and tuple(am.shape) == (K_ALL, size[0], size[1], Cs)
    assert torch.equal(y.cpu()[..., :C], ry) and torch.equal(am.cpu()[..., :C], ram)
    if Cs > C:
        assert float(y.cpu()[..., C:].abs().max()) == 0.0 and bool((am.cpu()[..., C:] == -1).all())
    assert bool((ram == -1).any()) and bool((ram >= 0).any())  # empty bins and pooled ones both occur
    if kind == "ties":  # equal maxima inside one bin do occur (the whole-map ROI at (1, 1): one bin over image 0 of level 0),
        H, W = R.SIZES[0]  # and the first in scan order was kept (the equality above)
        img = x[:H * W].view(H * W, C)
        assert int((img == img.amax(dim=0)).sum(dim=0).max()) > 1
    if kind == "negative":
        assert bool((ry[ram >= 0] < 0).all()) and bool((ry[ram == -1] == 0).all())


@pytest.mark.parametrize("K", [0, 1, 65])
def test_pool_forward_roi_counts(K):
    rois, lv, rl, ll = _rois(K)
    x = _x(4)
    y, am = ops.roi_pool(x.to(DEV), _shape(), rois.to(DEV), (2, 3), R.SCALES, levels=lv.to(DEV), return_argmax=True)
    assert tuple(y.shape) == (K, 2, 3, 4)
    if K:
        ry, ram = R.roi_pool(x, rl, ll, 2, 3)
        assert torch.equal(y.cpu(), ry) and torch.equal(am.cpu(), ram)


# ----------------------------------------------------------------------------- gradients
@pytest.mark.parametrize("sr", RATIOS)
def test_align_backward_bound_adjoint_and_reproducible(sr):
    """257 ROIs, 64 of them jittered around one box (they overlap on the same cells): the per-destination sums against fp64,
    the adjoint identity <roi_align(x), dy> = <x, backward(dy)>, and two runs byte for byte under set_deterministic(True)"""
    size = {0: (1, 1), 1: (2, 3), 2: (7, 7), 3: (7, 7)}[sr]  # (1, 1) adaptive: grids of 13 x 17 and 30 x 33, the cut walk
    C, Cs = CHANNELS[sr + 1]
    rois, lv, rl, ll = _rois(K_ALL)
    x = _x(C)
    dy = torch.randn(K_ALL, size[0], size[1], Cs, generator=torch.Generator().manual_seed(sr))
    was = ops.set_deterministic(True)
    try:
        runs = []
        for _ in range(2):
            xd = _padded(x, Cs).requires_grad_(True)
            y = ops.roi_align(xd, _shape(), rois.to(DEV), size, R.SCALES, sr, levels=lv.to(DEV), c=C)
            y.backward(dy.to(DEV))
            runs.append(xd.grad.cpu())
    finally:
        ops.set_deterministic(was)
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))
    dx = runs[0]
    if Cs > C:
        assert float(dx[:, C:].abs().max()) == 0.0
    ref = R.roi_align_backward(dy[..., :C], rl, ll, size[0], size[1], sr)
    assert int(ref["terms"].max()) >= 64  # the jittered ROIs do pile up on single rows
    err = (dx[:, :C].double() - ref["dx"]).abs()
    bound = R.align_backward_bound(ref)
    _report("align backward C=%d %s sr=%d" % (C, size, sr), float((err / bound).max()))
    assert bool((err <= bound).all())
    # adjoint: both sides from the kernels' fp32 outputs, summed in fp64; they differ by at most the two bounds weighted by
    # the other factor
    fwd = _align_ref(C, size, sr, K_ALL)
    lhs = float((y.detach().cpu()[..., :C].double() * dy[..., :C].double()).sum())
    rhs = float((x.double() * dx[:, :C].double()).sum())
    slack = float((R.align_forward_bound(fwd) * dy[..., :C].double().abs()).sum() + (bound * x.double().abs()).sum())
    _report("align adjoint %s sr=%d" % (size, sr), abs(lhs - rhs) / slack)
    assert abs(lhs - rhs) <= slack


@pytest.mark.parametrize("size", SIZES_P)
def test_pool_backward_bound_and_reproducible(size):
    C, Cs = CHANNELS[SIZES_P.index(size) + 3]
    rois, lv, rl, ll = _rois(K_ALL)
    x = _x(C, "ties")
    dy = torch.randn(K_ALL, size[0], size[1], Cs, generator=torch.Generator().manual_seed(5))
    was = ops.set_deterministic(True)
    try:
        runs = []
        for _ in range(2):
            xd = _padded(x, Cs).requires_grad_(True)
            y, am = ops.roi_pool(xd, _shape(), rois.to(DEV), size, R.SCALES, levels=lv.to(DEV), c=C, return_argmax=True)
            y.backward(dy.to(DEV))
            runs.append(xd.grad.cpu())
    finally:
        ops.set_deterministic(was)
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))
    ref = R.roi_pool_backward(dy[..., :C], am.cpu()[..., :C], rl, ll)
    assert int(ref["terms"].max()) >= 4  # overlapping ROIs name the same cell
    err = (runs[0][:, :C].double() - ref["dx"]).abs()
    bound = R.pool_backward_bound(ref)
    _report("pool backward C=%d %s" % (C, size), float((err / bound.clamp_min(1e-300)).max()))
    assert bool((err <= bound).all())
    if Cs > C:
        assert float(runs[0][:, C:].abs().max()) == 0.0


def test_gradients_past_the_grid_bound():
    """one wave per row of dx: 2 x 100 x 60 = 12,000 rows exceed the 8,192 waves of a capped grid"""
    sizes, scales, C = ((100, 60),), (0.5,), 4
    rs = np.random.RandomState(3)
    rl = [(int(rs.randint(0, 2)), float(a), float(b), float(a + w), float(b + h))
          for a, b, w, h in zip(rs.uniform(-10, 110, 24), rs.uniform(-10, 190, 24), rs.uniform(2, 90, 24), rs.uniform(2, 150, 24))]
    ll = [0] * len(rl)
    rois = torch.tensor(rl, dtype=torch.float32)
    rl = rois.tolist()
    shape = ops.PyramidShape(2, list(sizes))
    assert shape.rows > 8192
    x = R.make_rows(C, 11, 2, sizes)
    dy = torch.randn(len(rl), 3, 2, C, generator=torch.Generator().manual_seed(1))
    for sr in (0, 2):
        xd = x.to(DEV).requires_grad_(True)
        ops.roi_align(xd, shape, rois.to(DEV), (3, 2), scales, sr).backward(dy.to(DEV))
        ref = R.roi_align_backward(dy, rl, ll, 3, 2, sr, 2, sizes, scales)
        err = (xd.grad.cpu().double() - ref["dx"]).abs()
        assert bool((err <= R.align_backward_bound(ref)).all())
    xd = x.to(DEV).requires_grad_(True)
    y, am = ops.roi_pool(xd, shape, rois.to(DEV), (3, 2), scales, return_argmax=True)
    y.backward(dy.to(DEV))
    ry, ram = R.roi_pool(x, rl, ll, 3, 2, 2, sizes, scales)
    assert torch.equal(y.detach().cpu(), ry) and torch.equal(am.cpu(), ram)
    ref = R.roi_pool_backward(dy, ram, rl, ll, 2, sizes)
    assert bool(((xd.grad.cpu().double() - ref["dx"]).abs() <= R.pool_backward_bound(ref)).all())


# ----------------------------------------------------------------------------- pitch and alignment
def test_rows_as_a_slice_at_an_aligned_offset():
    """a row matrix that starts 3 rows into a larger allocation (3 * 72 * 4 bytes: 16-byte aligned, not 256-byte)"""
    C, Cs, size, sr = 68, 72, (2, 3), 2
    rois, lv, rl, ll = _rois(65)
    x = _x(C)
    big = torch.full((x.shape[0] + 3, Cs), -2.5, device=DEV)
    big[3:, :C] = x.to(DEV)
    rows = big[3:]
    assert rows.data_ptr() % 16 == 0 and rows.data_ptr() != big.data_ptr() and rows.is_contiguous()
    base = ops.roi_align(_padded(x, Cs), _shape(), rois.to(DEV), size, R.SCALES, sr, levels=lv.to(DEV), c=C)
    assert torch.equal(ops.roi_align(rows, _shape(), rois.to(DEV), size, R.SCALES, sr, levels=lv.to(DEV), c=C), base)
    py, pa = ops.roi_pool(_padded(x, Cs), _shape(), rois.to(DEV), size, R.SCALES, levels=lv.to(DEV), c=C, return_argmax=True)
    qy, qa = ops.roi_pool(rows, _shape(), rois.to(DEV), size, R.SCALES, levels=lv.to(DEV), c=C, return_argmax=True)
    assert torch.equal(py, qy) and torch.equal(pa, qa)
    # the gradient as a slice of a larger buffer is torch's business; the kernels are given the aligned slice of dy
    dyb = torch.randn(65 * 6 + 2, Cs, generator=torch.Generator().manual_seed(2)).to(DEV)
    dy = dyb[2:].view(65, 2, 3, Cs)
    sc = (ops.ctypes.c_float * 3)(*R.SCALES)
    dx = [torch.empty(_shape().rows + 1, Cs, device=DEV)[1:] for _ in range(2)]
    shape, rd, ld = _shape(), rois.to(DEV), lv.to(DEV)
    for out, g in zip(dx, (dy, dy.clone())):
        ops.call("scan_roi_align_backward", ops._ptr(g), shape.ref(), C, Cs, ops._ptr(rd), ops._ptr(ld), sc, 65, 2, 3, sr,
                 ops._ptr(out), ops._stream())
    assert torch.equal(dx[0], dx[1])


# ----------------------------------------------------------------------------- Pooler and the _C bindings
def _levels_nchw(C, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(R.N_IMAGES, C, h, w, generator=g) for h, w in R.SIZES]


def test_pooler_equals_the_per_level_loop(gold_dir):
    """reference modeling/poolers.py:91-121 restated on layers.ROIAlign: a nonzero and one ROIAlign per level; the one-launch
    Pooler gives the same bits, forward and backward, with the levels the reference's LevelMapper gives"""
    C = 6
    gold = json.load(open(os.path.join(gold_dir, "roi_levels.json")))["p2_p4"]
    gb = torch.tensor(gold["boxes"], dtype=torch.float64).float()
    rois, _, _, _ = _rois(100)
    b0 = torch.cat([rois[rois[:, 0] != 1][:, 1:], gb[:gold["split"]]])
    b1 = torch.cat([rois[rois[:, 0] == 1][:, 1:], gb[gold["split"]:]])
    boxes = [BoxList(b0.to(DEV), (68, 52)), BoxList(b1.to(DEV), (68, 52))]
    pooler = poolers.Pooler((7, 7), R.SCALES, 2)
    feats = [f.to(DEV).requires_grad_(True) for f in _levels_nchw(C)]
    out = pooler(feats, boxes)
    K = len(b0) + len(b1)
    assert tuple(out.shape) == (K, C, 7, 7) and out.is_contiguous()
    levels = pooler.map_levels(boxes)
    expect = R.level_mapper(torch.cat([b0, b1]), 2.0, 4.0)
    assert levels.cpu().tolist() == expect.tolist() and set(expect.tolist()) == {0, 1, 2}
    n0 = len(b0) - gold["split"]
    assert levels.cpu().tolist()[n0:len(b0)] == gold["levels"][:gold["split"]]  # the reference's own answers
    loop_feats = [f.detach().clone().requires_grad_(True) for f in feats]
    rois_all = pooler.convert_to_roi_format(boxes)
    result = torch.zeros((K, C, 7, 7), device=DEV)
    for level, (f, p) in enumerate(zip(loop_feats, pooler.poolers)):
        idx = torch.nonzero(levels == level).squeeze(1)
        result[idx] = p(f, rois_all[idx])
    assert torch.equal(out, result)
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(4)).to(DEV)
    out.backward(g)
    result.backward(g)
    for a, b in zip(feats, loop_feats):
        assert torch.equal(a.grad, b.grad)
    single = poolers.Pooler((2, 3), (0.25,), 0)
    assert torch.equal(single([feats[0].detach()], boxes), layers.ROIAlign((2, 3), 0.25, 0)(feats[0].detach(), rois_all))


def _compiled_C():
    try:
        import pybind11  # noqa: F401
    except ImportError:
        pytest.skip("pybind11 not importable: compiled extension modules are not built in this environment")
    ext = os.path.join(ROOT, "scan_amd", "ext")
    if ext not in sys.path:
        sys.path.insert(0, ext)
    return importlib.import_module("fcos_core._C")


@pytest.mark.parametrize("which", ["ctypes", "compiled"])
@pytest.mark.parametrize("C", [3, 8])
def test_C_bindings_equal_the_ops(which, C):
    """all four functions with the reference's positional arguments on NCHW GPU tensors: the ops' bits, contiguous NCHW"""
    _C = C_ctypes if which == "ctypes" else _compiled_C()
    H, W = R.SIZES[0]
    x = _levels_nchw(C)[0].to(DEV)
    rois = torch.tensor([r for r, l, _ in R.special_rois() if l == 0], dtype=torch.float32).to(DEV)
    K = len(rois)
    rows, shape = ops.nchw_to_rows(x)
    nchw = lambda t: t[..., :C].permute(0, 3, 1, 2).contiguous()
    y = _C.roi_align_forward(x, rois, 0.25, 2, 3, 2)
    assert y.is_contiguous() and torch.equal(y, nchw(ops.roi_align(rows, shape, rois, (2, 3), (0.25,), 2, c=C)))
    g = torch.randn(K, C, 2, 3, generator=torch.Generator().manual_seed(C)).to(DEV)
    rd = rows.clone().requires_grad_(True)
    ops.roi_align(rd, shape, rois, (2, 3), (0.25,), 2, c=C).backward(
        torch.nn.functional.pad(g.permute(0, 2, 3, 1), (0, rows.shape[1] - C)).contiguous())
    dx = _C.roi_align_backward(g, rois, 0.25, 2, 3, R.N_IMAGES, C, H, W, 2)
    assert tuple(dx.shape) == (R.N_IMAGES, C, H, W) and dx.is_contiguous()
    assert torch.equal(dx, rd.grad.view(R.N_IMAGES, H, W, -1)[..., :C].permute(0, 3, 1, 2))
    py, pa = _C.roi_pool_forward(x, rois, 0.25, 2, 3)
    oy, oa = ops.roi_pool(rows, shape, rois, (2, 3), (0.25,), c=C, return_argmax=True)
    assert pa.dtype == torch.int32 and tuple(pa.shape) == (K, C, 2, 3) and py.is_contiguous() and pa.is_contiguous()
    assert torch.equal(py, nchw(oy)) and torch.equal(pa, nchw(oa))
    rd = rows.clone().requires_grad_(True)
    ops.roi_pool(rd, shape, rois, (2, 3), (0.25,), c=C).backward(
        torch.nn.functional.pad(g.permute(0, 2, 3, 1), (0, rows.shape[1] - C)).contiguous())
    dx = _C.roi_pool_backward(g, x, rois, pa, 0.25, 2, 3, R.N_IMAGES, C, H, W)
    assert torch.equal(dx, rd.grad.view(R.N_IMAGES, H, W, -1)[..., :C].permute(0, 3, 1, 2))
    # the drop-in layers on the same tensors
    assert torch.equal(layers.ROIAlign((2, 3), 0.25, 2)(x, rois), y) and torch.equal(layers.ROIPool((2, 3), 0.25)(x, rois), py)
    assert torch.equal(layers.roi_align(x, rois, (2, 3), 0.25, 2), y) and torch.equal(layers.roi_pool(x, rois, (2, 3), 0.25), py)
    e = _C.roi_align_forward(x, rois[:0], 0.25, 2, 3, 2)
    assert tuple(e.shape) == (0, C, 2, 3)

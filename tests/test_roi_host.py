"""Region pooling (ROIAlign / ROIPool / Pooler), everything that needs no GPU: the CPU roi_align_forward of both _C bindings
against the restatement of tests/roi_ref.py, the restatement's LevelMapper against the reference's own levels
(tests/golden/roi_levels.json), the layers / poolers surface, the pooler defaults, the new C-ABI symbols and their argument
checks, and the CPU refusals."""
import ctypes
import importlib
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import roi_ref as R
from scan_amd import _C as C_ctypes, _lib, config, layers, ops
from scan_amd.modeling import poolers
from scan_amd.structures import BoxList

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("scan_roi_levels", "scan_roi_align_forward", "scan_roi_align_backward", "scan_roi_align_samples",
           "scan_roi_pool_forward", "scan_roi_pool_backward")


def _compiled_C():
    try:
        import pybind11  # noqa: F401
    except ImportError:
        pytest.skip("pybind11 not importable: compiled extension modules are not built in this environment")
    ext = os.path.join(ROOT, "scan_amd", "ext")
    if ext not in sys.path:
        sys.path.insert(0, ext)
    return importlib.import_module("fcos_core._C")


def _binding(which):
    return C_ctypes if which == "ctypes" else _compiled_C()


BINDINGS = ["ctypes", "compiled"]


# ----------------------------------------------------------------------------- the restatement itself
def test_restatement_on_hand_computed_samples():
    """(1, 1) bins, sampling_ratio 1 on level 0 (13 x 17, scale 1/4): the sample positions named in roi_ref.special_rois"""
    s = R.align_samples((0, -6.0, -6.0, 2.0, 2.0), 0, 1, 1, 1)
    assert s["pos_y"][0] == -0.5 and s["pos_x"][0] == -0.5 and bool(s["live"][0, 0])
    assert s["cell"][:, 0, 0].tolist() == [0, 1, 17, 18] and s["w"][:, 0, 0].tolist() == [1.0, 0.0, 0.0, 0.0]  # clamped to 0
    s = R.align_samples((0, -8.0, -8.0, 0.0, 0.0), 0, 1, 1, 1)
    assert s["pos_y"][0] == -1.0 and bool(s["live"][0, 0])  # exactly -1 is still inside
    s = R.align_samples((0, 64.0, 48.0, 72.0, 56.0), 0, 1, 1, 1)
    assert s["pos_y"][0] == 13.0 and s["pos_x"][0] == 17.0 and bool(s["live"][0, 0])  # y == H, x == W
    assert s["cell"][:, 0, 0].tolist() == [12 * 17 + 16] * 4 and s["w"][:, 0, 0].tolist() == [1.0, 0.0, 0.0, 0.0]
    s = R.align_samples((0, 30.0, 30.0, 10.0, 10.0), 0, 2, 3, 0)
    assert s["g"] == (1, 1)  # x2 < x1: forced to 1 x 1, adaptive grid ceil(1 / 2) = 1
    assert R.align_samples((0, 0.0, 0.0, 68.0, 52.0), 0, 1, 1, 0)["g"] == (13, 17)
    assert not R.align_samples((0, 500.0, 500.0, 600.0, 600.0), 0, 2, 3, 2)["live"].any()
    for roi, lv in (((-1, 8.0, 8.0, 40.0, 36.0), 0), ((2, 8.0, 8.0, 40.0, 36.0), 0), ((0, 8.0, 8.0, 40.0, 36.0), 3),
                    ((0, 8.0, 8.0, 40.0, 36.0), -1)):
        assert R.align_samples(roi, lv, 2, 3, 2) is None
    # a constant map pools to the constant wherever every sample is inside; the gradient of a sum is the adjoint
    x = torch.ones(R.row_offsets(R.N_IMAGES, R.SIZES)[-1], 3)
    y = R.roi_align(x, [(0, 9.0, 7.0, 41.0, 33.0)], [0], 2, 3, 2)["y"]
    np.testing.assert_allclose(y.numpy(), 1.0, rtol=0, atol=1e-6)


def test_restatement_adjoint_and_pool_rules():
    rois, lv = R.make_rois(40)
    x = R.make_rows(5, 1).double()
    g = torch.Generator().manual_seed(2)
    dy = torch.randn(40, 2, 3, 5, generator=g, dtype=torch.float64)
    for sr in (0, 2):
        y = R.roi_align(x, rois.tolist(), lv.tolist(), 2, 3, sr)["y"]
        dx = R.roi_align_backward(dy, rois.tolist(), lv.tolist(), 2, 3, sr)["dx"]
        assert abs(float((y * dy).sum()) - float((x * dx).sum())) <= 1e-9 * float((y * dy).abs().sum())
    # ROIPool: ties keep the first cell in scan order, an all-negative map keeps its maxima, empty bins give 0 / -1
    xc = torch.full((R.row_offsets(R.N_IMAGES, R.SIZES)[-1], 2), -3.0)
    y, am = R.roi_pool(xc, [(0, 8.0, 8.0, 32.0, 32.0), (0, 60.0, 44.0, 90.0, 70.0)], [0, 0], 7, 7)
    assert bool((y[0] == -3.0).all()) and am[0, 0, 0].tolist() == [2 * 17 + 2] * 2 and am[0, 6, 6].tolist() == [8 * 17 + 8] * 2
    assert bool((am[1] == -1).any()) and bool((y[1][am[1] == -1] == 0).all()) and bool((y[1][am[1] >= 0] == -3.0).all())
    hb, wb = R.pool_bins((0, 8.0, 8.0, 32.0, 32.0), 0.25, 7, 7, 13, 17)
    assert hb == [(2 + i, 3 + i) for i in range(7)] and wb == hb  # bin edges exactly on integers
    d = R.roi_pool_backward(torch.ones(2, 7, 7, 2), am, [(0, 8.0, 8.0, 32.0, 32.0), (0, 60.0, 44.0, 90.0, 70.0)], [0, 0])
    assert float(d["dx"].sum()) == float((am >= 0).sum())


def test_restatement_reproduces_the_reference_levels(gold_dir):
    gold = json.load(open(os.path.join(gold_dir, "roi_levels.json")))
    assert set(gold) == {"p2_p4", "p2_p5", "p3_p7", "single"}
    for name, c in gold.items():
        boxes = torch.tensor(c["boxes"], dtype=torch.float64).float()
        assert boxes.double().tolist() == c["boxes"], name  # stored exactly
        side = torch.sqrt((boxes[:, 2] - boxes[:, 0] + 1) * (boxes[:, 3] - boxes[:, 1] + 1))
        for v in (112.0, 224.0, 448.0):
            assert bool((side == v).any()), (name, v)
        assert R.level_mapper(boxes, c["k_min"], c["k_max"]).tolist() == c["levels"], name
        # the host path of the drop-in LevelMapper, on the two box lists the fixture was made from
        lists = [BoxList(boxes[:c["split"]], (4096, 4096), mode="xyxy"), BoxList(boxes[c["split"]:], (4096, 4096), mode="xyxy")]
        assert poolers.LevelMapper(c["k_min"], c["k_max"])(lists).tolist() == c["levels"], name


# ----------------------------------------------------------------------------- CPU roi_align_forward of both bindings
def _nchw_case(C, dtype):
    H, W = R.SIZES[0]
    x = torch.randn(R.N_IMAGES, C, H, W, generator=torch.Generator().manual_seed(C), dtype=torch.float64).to(dtype)
    rois = torch.tensor([r for r, l, _ in R.special_rois() if l == 0], dtype=dtype)
    rows = x.permute(0, 2, 3, 1).reshape(-1, C)
    return x, rois, rows


@pytest.mark.parametrize("which", BINDINGS)
@pytest.mark.parametrize("size,sr", [((1, 1), 1), ((1, 1), 0), ((2, 3), 0), ((2, 3), 2), ((7, 7), 3), ((7, 7), 1)])
def test_cpu_roi_align_forward_matches_the_restatement(which, size, sr):
    """fp32: the same fp32 weights, values accumulated in fp32 in the source's order -- against the fp64 sums under the bound
    derived in tests/test_gpu_roi.py (4 products + 3 sums per sample, g_h g_w additions, one division), relative to the sum
    of |w v|.  The special ROIs sit on level 0; image -1 and N give zeros."""
    _C = _binding(which)
    x, rois, rows = _nchw_case(3, torch.float32)
    y = _C.roi_align_forward(x, rois, R.SCALES[0], size[0], size[1], sr)
    assert tuple(y.shape) == (len(rois), 3, size[0], size[1]) and y.dtype == torch.float32 and y.is_contiguous()
    ref = R.roi_align(rows, rois.tolist(), [0] * len(rois), size[0], size[1], sr, sizes=R.SIZES[:1], scales=R.SCALES[:1])
    bound = R.align_forward_bound(ref)
    err = (y.permute(0, 2, 3, 1).double() - ref["y"]).abs()
    assert bool((err <= bound).all()), float((err / bound).max())
    what = [w for _, l, w in R.special_rois() if l == 0]
    for k, w in enumerate(what):
        if w in ("outside", "image -1", "image N"):
            assert float(y[k].abs().max()) == 0.0, w


@pytest.mark.parametrize("which", BINDINGS)
def test_cpu_roi_align_forward_double_and_empty(which):
    _C = _binding(which)
    x, rois, rows = _nchw_case(4, torch.float64)
    y = _C.roi_align_forward(x, rois, 0.25, 2, 3, 2)
    assert y.dtype == torch.float64
    # positions in fp64 here, in fp32 in the restatement.  An fp32 position below 2^5 = 32 (the largest sample of these ROIs is
    # under 18.5 + 8) carries at most 4 roundings of half an ulp 2^-19 each, so a sample moves by at most 2^-18 per axis;
    # bilinear interpolation is continuous and piecewise linear with slope at most max - min of the map per axis, and an
    # average of samples moves by no more than its samples: |dy| <= 2 * 2^-18 * (max - min)
    ref = R.roi_align(rows, rois.tolist(), [0] * len(rois), 2, 3, 2, sizes=R.SIZES[:1], scales=R.SCALES[:1])
    tol = 2 * 2.0 ** -18 * float(x.max() - x.min())
    np.testing.assert_allclose(y.permute(0, 2, 3, 1).numpy(), ref["y"].numpy(), rtol=0, atol=tol)
    e = _C.roi_align_forward(x, rois[:0], 0.25, 2, 3, 2)
    assert tuple(e.shape) == (0, 4, 2, 3)


@pytest.mark.parametrize("which", BINDINGS)
def test_cpu_refusals_and_argument_counts(which):
    """csrc/ROIAlign.h:44, csrc/ROIPool.h:24,46: the other three are not implemented on the CPU; a wrong argument count is a
    RuntimeError that names the arguments"""
    _C = _binding(which)
    x, rois = torch.zeros(1, 4, 5, 5), torch.zeros(2, 5)
    g, am = torch.zeros(2, 4, 2, 2), torch.zeros(2, 4, 2, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        _C.roi_align_backward(g, rois, 0.25, 2, 2, 1, 4, 5, 5, 2)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        _C.roi_pool_forward(x, rois, 0.25, 2, 2)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        _C.roi_pool_backward(g, x, rois, am, 0.25, 2, 2, 1, 4, 5, 5)
    for name, word in (("roi_align_forward", "sampling_ratio"), ("roi_align_backward", "batch_size"),
                       ("roi_pool_forward", "pooled_width"), ("roi_pool_backward", "argmax")):
        with pytest.raises(RuntimeError, match=word):
            getattr(_C, name)()
        with pytest.raises(RuntimeError, match=word):
            getattr(_C, name)(x, rois)


# ----------------------------------------------------------------------------- layers / poolers surface
def test_layers_surface_matches_the_reference():
    """reference layers/roi_align.py:11-68, layers/roi_pool.py:11-63: constructor and forward arguments, __repr__"""
    for name in ("ROIAlign", "roi_align", "ROIPool", "roi_pool"):
        assert hasattr(layers, name), name
    assert list(inspect.signature(layers.ROIAlign.__init__).parameters) == ["self", "output_size", "spatial_scale", "sampling_ratio"]
    assert list(inspect.signature(layers.ROIAlign.forward).parameters) == ["self", "input", "rois"]
    assert list(inspect.signature(layers.ROIPool.__init__).parameters) == ["self", "output_size", "spatial_scale"]
    assert list(inspect.signature(layers.ROIPool.forward).parameters) == ["self", "input", "rois"]
    assert list(inspect.signature(layers.roi_align).parameters) == ["input", "roi", "output_size", "spatial_scale", "sampling_ratio"]
    assert list(inspect.signature(layers.roi_pool).parameters) == ["input", "roi", "output_size", "spatial_scale"]
    assert repr(layers.ROIAlign((7, 7), 0.25, 2)) == "ROIAlign(output_size=(7, 7), spatial_scale=0.25, sampling_ratio=2)"
    assert repr(layers.ROIPool((7, 7), 0.0625)) == "ROIPool(output_size=(7, 7), spatial_scale=0.0625)"
    with pytest.raises(RuntimeError, match="GPU"):
        layers.ROIAlign((2, 2), 0.25, 2)(torch.zeros(1, 4, 5, 5), torch.zeros(1, 5))
    with pytest.raises(RuntimeError, match="GPU"):
        layers.ROIPool((2, 2), 0.25)(torch.zeros(1, 4, 5, 5), torch.zeros(1, 5))


def test_pooler_surface_and_defaults(gold_dir):
    """reference modeling/poolers.py:45-133: Pooler(output_size, scales, sampling_ratio), forward(x, boxes), one ROIAlign per
    scale in .poolers, the level range from the first and last scale; make_pooler reads MODEL[head_name] over the reference's
    defaults (defaults.py:214-216), which live outside config.DEFAULTS"""
    assert list(inspect.signature(poolers.Pooler.__init__).parameters) == ["self", "output_size", "scales", "sampling_ratio"]
    assert list(inspect.signature(poolers.Pooler.forward).parameters) == ["self", "x", "boxes"]
    assert list(inspect.signature(poolers.make_pooler).parameters) == ["cfg", "head_name"]
    assert list(inspect.signature(poolers.LevelMapper.__init__).parameters) == ["self", "k_min", "k_max", "canonical_scale",
                                                                               "canonical_level", "eps"]
    p = poolers.Pooler((7, 7), (0.25, 0.125, 0.0625, 0.03125), 2)
    assert [repr(m) for m in p.poolers] == ["ROIAlign(output_size=(7, 7), spatial_scale=%s, sampling_ratio=2)" % s
                                            for s in (0.25, 0.125, 0.0625, 0.03125)]
    assert (p.map_levels.k_min, p.map_levels.k_max, p.map_levels.s0, p.map_levels.lvl0, p.map_levels.eps) == (2.0, 5.0, 224, 4, 1e-6)
    boxes = [BoxList(torch.tensor([[1.0, 2.0, 3.0, 4.0]]), (10, 10)), BoxList(torch.tensor([[5.0, 6.0, 7.0, 8.0]] * 2), (10, 10))]
    assert p.convert_to_roi_format(boxes).tolist() == [[0.0, 1.0, 2.0, 3.0, 4.0], [1.0, 5.0, 6.0, 7.0, 8.0], [1.0, 5.0, 6.0, 7.0, 8.0]]
    assert config.POOLER_DEFAULTS == {"POOLER_RESOLUTION": 14, "POOLER_SAMPLING_RATIO": 0, "POOLER_SCALES": (1.0 / 16,)}
    cfg = config.load("c2f")
    d = poolers.make_pooler(cfg, "ROI_BOX_HEAD")
    assert d.output_size == (14, 14) and d.scales == (0.0625,) and d.sampling_ratio == 0 and len(d.poolers) == 1
    cfg = config.load("c2f", ["MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION", 7, "MODEL.ROI_BOX_HEAD.POOLER_SCALES", "(0.25, 0.125)",
                              "MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO", 2])
    d = poolers.make_pooler(cfg, "ROI_BOX_HEAD")
    assert d.output_size == (7, 7) and d.scales == (0.25, 0.125) and d.sampling_ratio == 2
    cfg = config.load("c2f")
    cfg.MODEL["ROI_MASK_HEAD"] = config.Cfg({"POOLER_RESOLUTION": 28, "POOLER_SCALES": [0.25, 0.125, 0.0625], "OTHER": 1})
    d = poolers.make_pooler(cfg, "ROI_MASK_HEAD")
    assert d.output_size == (28, 28) and d.scales == (0.25, 0.125, 0.0625) and d.sampling_ratio == 0
    # the shipped experiments are untouched: no new key in DEFAULTS, the hot-path views equal the committed fixtures
    assert not any(k.startswith("ROI_") for k in config.DEFAULTS["MODEL"])
    for name in ("c2f", "s2c", "k2c"):
        gold = json.load(open(os.path.join(gold_dir, "cfg_%s.json" % name)))["cfg"]
        assert config.hot_path_view(config.load(name)) == gold


def test_ops_refuse_cpu_tensors_and_wrong_geometry():
    shape = ops.PyramidShape(1, [(4, 4)])
    rows, rois = torch.zeros(16, 4), torch.zeros(2, 5)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.roi_align(rows, shape, rois, (2, 2), (0.25,), 2)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.roi_pool(rows, shape, rois, (2, 2), (0.25,))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.roi_levels(rois, 2, 5)


# ----------------------------------------------------------------------------- C ABI
def test_symbols_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "scan_hip.h")).read()
    declared = set(re.findall(r"\b(scan_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(L, name), name
    assert L.scan_abi_version() == 1
    mk = open(os.path.join(ROOT, "scan_amd", "csrc", "Makefile")).read()
    assert "build/roi.o" in mk and re.search(r"build/roi\.o:.*\n(?:\t.*\n)*\t.*-ffp-contract=off", mk)


def test_arguments_validated_without_device():
    d = ops.PyramidShape(2, [(4, 4), (2, 2)])
    p = ctypes.c_void_p(64)
    sc = (ctypes.c_float * 2)(0.25, 0.125)
    common = (("d", d.ref()), ("C", 4), ("Cs", 4), ("rois", p), ("levels", p), ("scales", sc), ("K", 3), ("PH", 2), ("PW", 2))

    def caller(name, head, tail):
        order = head + common + tail + (("stream", None),)
        return lambda **kw: _lib.call(name, *[kw.get(k, v) for k, v in order])

    afwd = caller("scan_roi_align_forward", (("x", p),), (("sr", 2), ("y", p)))
    abwd = caller("scan_roi_align_backward", (("dy", p),), (("sr", 2), ("dx", p)))
    pfwd = caller("scan_roi_pool_forward", (("x", p),), (("y", p), ("argmax", p)))
    pbwd = caller("scan_roi_pool_backward", (("dy", p), ("argmax", p)), (("dx", p),))
    for fn in (afwd, abwd, pfwd, pbwd):
        for ptr in ("d", "rois", "scales"):
            with pytest.raises(RuntimeError, match="null"):
                fn(**{ptr: None})
        with pytest.raises(RuntimeError, match="Cs"):
            fn(Cs=6)
        with pytest.raises(RuntimeError, match="C=5"):
            fn(C=5)
        with pytest.raises(RuntimeError, match="pooled size"):
            fn(PH=0)
        with pytest.raises(RuntimeError, match="pooled size"):
            fn(PW=-1)
        with pytest.raises(RuntimeError, match="K="):
            fn(K=-1)
        with pytest.raises(RuntimeError, match="2\\^31"):
            fn(K=(1 << 31) // 4 + 1)
        bad = ops.PyramidShape(1, [(2, 2)])
        bad.desc.n_levels = 6
        with pytest.raises(RuntimeError, match="bad pyramid"):
            fn(d=bad.ref())
        bad = ops.PyramidShape(1, [(2, 2)])
        bad.desc.row_off[1] = 5  # not n_images * h * w
        with pytest.raises(RuntimeError, match="bad pyramid"):
            fn(d=bad.ref())
        big = ops.PyramidShape(2, [(32768, 32768)])  # M = 2^31
        with pytest.raises(RuntimeError, match="2\\^31"):
            fn(d=big.ref(), scales=(ctypes.c_float * 1)(1.0))
    for fn, ptrs in ((afwd, ("x", "y")), (abwd, ("dy", "dx")), (pfwd, ("x", "y", "argmax")), (pbwd, ("dy", "argmax", "dx"))):
        for ptr in ptrs:
            with pytest.raises(RuntimeError, match="null"):
                fn(**{ptr: None})
            with pytest.raises(RuntimeError, match="aligned"):
                fn(**{ptr: ctypes.c_void_p(68)})
    for fn in (afwd, abwd):
        with pytest.raises(RuntimeError, match="sampling_ratio"):
            fn(sr=1 << 20)
    # K == 0: legal, returns before any launch (no device here), whatever the data pointers are
    assert afwd(K=0, x=None, y=None, rois=None) is None and pfwd(K=0, x=None, y=None, argmax=None, rois=None) is None
    lev = lambda **kw: _lib.call("scan_roi_levels", *[kw.get(k, v) for k, v in (
        ("boxes", p), ("ld", 5), ("K", 3), ("k_min", 2.0), ("k_max", 5.0), ("s0", 224.0), ("lvl0", 4.0), ("eps", 1e-6), ("levels", p),
        ("stream", None))])
    for ptr in ("boxes", "levels"):
        with pytest.raises(RuntimeError, match="null"):
            lev(**{ptr: None})
    with pytest.raises(RuntimeError, match="ld"):
        lev(ld=3)
    with pytest.raises(RuntimeError, match="k_min"):
        lev(k_min=6.0)
    with pytest.raises(RuntimeError, match="k_min"):
        lev(k_min=2.5)
    assert lev(K=0, boxes=None, levels=None) is None
    smp = lambda **kw: _lib.call("scan_roi_align_samples", *[kw.get(k, v) for k, v in (
        ("d", d.ref()), ("rois", p), ("levels", p), ("scales", sc), ("K", 3), ("PH", 2), ("PW", 2), ("sr", 0), ("gmax", 4),
        ("grid", p), ("pos", p), ("wgt", p), ("cell", p), ("stream", None))])
    for ptr in ("grid", "pos", "wgt", "cell", "rois", "d"):
        with pytest.raises(RuntimeError, match="null"):
            smp(**{ptr: None})
    with pytest.raises(RuntimeError, match="gmax"):
        smp(gmax=0)

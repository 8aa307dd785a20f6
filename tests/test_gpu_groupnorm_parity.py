"""GPU tests of the GroupNorm(32) + ReLU kernels (scan_amd/csrc/groupnorm.hip) and of the GroupNorm-sum epilogues of the 3x3
convs (conv_fwd.hip direct and Winograd, conv_gen1.hip) against the float64 oracle and the rounding bars of
tests/groupnorm_ref.py (derived there; tests/test_groupnorm_host.py shows on the CPU that the kernels' arithmetic reaches at
most half of them and that fp32 squares in the group sums do not).  Every element is compared, nothing is excluded.

The library is called through ctypes as tests/test_gpu_groupnorm_plan.py calls it, so the (mean, rstd) table is visible.
Inputs: nine (offset, sd) cases in which every (level, image, group) has its own offset and scale, on five small pyramids of
N = 2 images (groupnorm_ref.CASES / PYRAMIDS).  Each test prints its figures (largest error / bar) before it asserts them."""
import ctypes
import types

import numpy as np
import pytest
import torch

import groupnorm_ref as R

pytestmark = pytest.mark.gpu

C, G, EPS, WIDE = R.C, R.G, R.EPS, R.WIDE
SOURCES = ("x_atomic", "x_ordered", "sums", "sums_final")
SENTINEL = -7.5   # what the columns past C of a wider y hold before and after

_dev_cache = {}


def _dev(device, name, pyramid):
    """the case's arrays on the device, made once and never written"""
    key = (name, pyramid)
    if key not in _dev_cache:
        from scan_amd import ops
        c = R.case(name, pyramid)
        up = lambda a: torch.from_numpy(np.array(a)).to(device)
        d = types.SimpleNamespace(ref=c, shape=ops.PyramidShape(R.N, R.PYRAMIDS[pyramid]), x=up(c.x), gamma=up(c.gamma), beta=up(c.beta),
                                  dy=up(c.dy), dy_wide=up(c.dy_wide), fill=up(c.fill), sums=up(c.sums).reshape(-1, 2).contiguous())
        assert d.shape.row_off == c.shape.row_off and d.sums.dtype == torch.float64
        _dev_cache[key] = d
    return _dev_cache[key]


def _p(t):
    from scan_amd import ops
    return ops._ptr(t)


def _call(name, *args):
    from scan_amd import _lib, ops
    _lib.call(name, *args, ops._stream())


def _plan(shape, source):
    """a plan made with the deterministic knob as the source asks; the run functions launch what it says"""
    from scan_amd import _lib, ops
    det = source == "x_ordered"
    flags = {"sums": _lib.GN_SUMS, "sums_final": _lib.GN_SUMS | _lib.GN_SEPARATE_FINAL}.get(source, 0)
    old = ops.set_deterministic(det)
    try:
        plan = _lib.GroupNormPlan()
        _lib.call("scan_groupnorm_plan", shape.ref(), C, G, flags, ctypes.byref(plan))
    finally:
        ops.set_deterministic(old)
    want = {"sums": _lib.GN_FROM_SUMS, "sums_final": _lib.GN_FROM_SUMS_FINAL}.get(source, _lib.GN_FROM_X)
    assert (plan.ordered, plan.source) == (int(det), want)
    return plan


def _forward(d, plan, ld, relu):
    """y as the first C columns of a [M, ld] matrix: those poisoned, the others at SENTINEL; a poisoned statistics table"""
    from scan_amd import _lib
    y = torch.full((d.shape.rows, ld), SENTINEL, device=d.x.device)
    y[:, :C] = float("nan")
    stats = torch.full((plan.stats_floats,), float("nan"), device=d.x.device)
    from_x = plan.source == _lib.GN_FROM_X
    ws = torch.empty(plan.fwd_ws_doubles, dtype=torch.float64, device=d.x.device) if from_x else None
    sums = None if from_x else d.sums.clone()
    _call("scan_groupnorm_run_forward", ctypes.byref(plan), _p(d.x), d.shape.ref(), _p(sums), EPS, _p(d.gamma), _p(d.beta), relu,
          _p(y), ld, _p(stats), _p(ws))
    if sums is not None:
        assert torch.equal(sums, d.sums)
    return y, stats


def _backward(d, plan, stats, lddy, relu, accumulate, cleared):
    dx = torch.full_like(d.x, float("nan"))
    dg, db = (d.fill[0].clone(), d.fill[1].clone()) if accumulate else (torch.full_like(d.gamma, float("nan")), torch.full_like(d.beta, float("nan")))
    ws = torch.empty(plan.bwd_ws_doubles, dtype=torch.float64, device=d.x.device)
    if cleared:
        ws.zero_()
    _call("scan_groupnorm_run_backward", ctypes.byref(plan), _p(d.x), _p(d.beta), _p(d.dy_wide if lddy == WIDE else d.dy), lddy,
          d.shape.ref(), _p(stats), _p(d.gamma), relu, _p(dx), _p(dg), _p(db), accumulate, _p(ws), int(cleared))
    return dx, dg, db


def _np(t):
    return t.detach().cpu().numpy()


def _check(what, fig):
    print("%s: %s" % (what, " ".join("%s %.3g" % kv for kv in sorted(fig.items()))))
    assert all(v <= 1.0 for v in fig.values()), (what, fig)


# ----------------------------------------------------------------------------- statistics and forward
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("pyramid", sorted(R.PYRAMIDS))
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_statistics_and_forward(device, name, pyramid, source):
    """the (mean, rstd) table and y inside the bars from every statistics source (the two sums sources are fed the float64
    sums of the slots), with and without the ReLU; on one pyramid also into the first 256 columns of a 264-column matrix"""
    d = _dev(device, name, pyramid)
    plan = _plan(d.shape, source)
    for relu in (1, 0):
        fwd = d.ref.fwd[relu]
        for ld in ((C, WIDE) if pyramid == R.ONE_PYRAMID else (C,)):
            y, stats = _forward(d, plan, ld, relu)
            fig = dict(zip(("mean", "rstd"), R.stats_ratios(_np(stats), fwd)))
            fig["y"] = R.ratio(_np(y[:, :C]), fwd.y, fwd.tol_y())
            _check("%s %s %s relu=%d ld=%d" % (name, pyramid, source, relu, ld), fig)
            assert bool((y[:, C:] == SENTINEL).all())   # the other columns of the wider matrix stay untouched


# ----------------------------------------------------------------------------- backward
@pytest.mark.parametrize("ordered", [0, 1])
@pytest.mark.parametrize("pyramid", sorted(R.PYRAMIDS))
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_backward(device, name, pyramid, ordered):
    """dx, dgamma, dbeta inside the bars, atomic and ordered, from the table the device forward wrote.  The mask handed to the
    oracle is y > 0 of that forward: the backward kernels recompute exactly this predicate from x, so no element is excluded.
    On one pyramid: accumulate on and off, the workspace arriving cleared or not, and dy as columns of a 264-column matrix"""
    d = _dev(device, name, pyramid)
    plan = _plan(d.shape, "x_ordered" if ordered else "x_atomic")
    variants = [(0, False, C)]
    if pyramid == R.ONE_PYRAMID:
        variants += [(1, False, C), (0, True, C), (1, True, C), (0, False, WIDE), (1, True, WIDE)]
    for relu in (1, 0):
        y, stats = _forward(d, plan, C, relu)
        fwd = d.ref.fwd[relu]
        assert bool(torch.isfinite(stats).all())
        for accumulate, cleared, lddy in variants:
            bwd = R.Backward(fwd, d.ref.dy_wide[:, :C], _np(y) > 0 if relu else None)
            dx, dg, db = _backward(d, plan, stats, lddy, relu, accumulate, cleared)
            assert bool(torch.isfinite(dx).all())   # it went in as NaN
            fill = d.ref.fill.astype(np.float64) if accumulate else np.zeros((2, C))
            fig = {"dx": R.ratio(_np(dx), bwd.dx, bwd.tol_dx()),
                   "dgamma": R.ratio(_np(dg), bwd.dgamma + fill[0], bwd.tol_dgamma(fill[0] if accumulate else None)),
                   "dbeta": R.ratio(_np(db), bwd.dbeta + fill[1], bwd.tol_dbeta(fill[1] if accumulate else None))}
            _check("%s %s ordered=%d relu=%d accumulate=%d cleared=%d lddy=%d" % (name, pyramid, ordered, relu, accumulate, cleared, lddy), fig)


# ----------------------------------------------------------------------------- the conv epilogues' sums
# (CONV_MODE, knob, value): the Winograd epilogue, the direct epilogue with three pieces, with two, and conv_gen1.hip's
EPILOGUES = [("bf16x6", "conv_wino", 1), ("bf16x6", "conv_wino", 0), ("bf16x3", "conv_v2", 1), ("bf16x3", "conv_v2", 0)]


@pytest.mark.parametrize("mode,knob,value", EPILOGUES)
@pytest.mark.parametrize("pyramid", ["ragged_three_levels", "one_pixel"])
@pytest.mark.parametrize("off", [0, 10, 100, 1000])
def test_conv_epilogue_sums(device, off, pyramid, mode, knob, value):
    """a 256 -> 256 3x3 conv with gn_sums: the sums its epilogue leaves against float64 sums over the device's OWN output (the
    conv's split-operand error is not under test), then groupnorm_relu on that output against the oracle of the same output.
    x = 100 randn and w = randn / 4800 give outputs of standard deviation about 1 (a third of that where a pixel sees one
    tap), the bias is off (1 + g / 32) per group: |mean| / std up to a few thousand, where float64 sums still leave the
    variance exact to 1e-8.  Bar of a sum: every element enters as a double, so cnt additions in any order and one rounding
    of a square, granted twice over (the reference's own sum): 2 cnt 2^-53 of the sum of magnitudes"""
    from scan_amd import _lib, ops
    shape = ops.PyramidShape(R.N, R.PYRAMIDS[pyramid])
    g = torch.Generator().manual_seed(17 + off)
    x = (100 * torch.randn(shape.rows, C, generator=g)).to(device)
    w = (torch.randn(C, C, 3, 3, generator=g) / 4800).to(device).contiguous(memory_format=torch.channels_last)
    b = (off * (1 + torch.arange(G) / G)).repeat_interleave(R.CPG).to(device)
    gamma = (1 + 0.1 * torch.randn(C, generator=g)).to(device)
    beta = (0.1 * torch.randn(C, generator=g)).to(device)
    keep_mode, ops.CONV_MODE = ops.CONV_MODE, mode
    old = _lib.query("scan_tune", knob.encode(), value)
    try:
        with torch.no_grad():
            y = ops.conv2d(x, w, b, shape, 3, 1, gn_sums=True)
        sums = ops._gn_sums.get(y.data_ptr())
        assert sums is not None and sums.dtype == torch.float64
        n = shape.n_levels * R.N * G * 2
        got = _np(sums.reshape(-1)[:n]).reshape(-1, G, 2).copy()
        out = ops.groupnorm_relu(y.requires_grad_(True), gamma, beta, shape)
        assert not ops._gn_sums   # the hand-over was consumed: the statistics below come from the epilogue's sums
        stats = out.grad_fn.saved_tensors[3]   # _GroupNormReLU saves (x, beta, gamma, stats): hold the position to its shape
        assert stats.dtype == torch.float32 and tuple(stats.shape) == (shape.n_levels * R.N * G * 2,)
    finally:
        _lib.query("scan_tune", knob.encode(), old)
        ops.CONV_MODE = keep_mode
    yh = _np(y)
    assert np.isfinite(yh).all()
    y64 = yh.astype(np.float64)
    exp, mag = R.group_sums(yh, shape), R.group_sums(np.abs(yh), shape)
    cnt = np.array([rows.stop - rows.start for _, _, _, rows in R.slots(shape)], np.float64)[:, None] * R.CPG
    fig = {"sum": R.ratio(got[..., 0], exp[..., 0], 2 * cnt * 2.0 ** -53 * mag[..., 0]),
           "sumsq": R.ratio(got[..., 1], exp[..., 1], 2 * cnt * 2.0 ** -53 * mag[..., 1])}
    fwd = R.Forward(yh, _np(gamma), _np(beta), shape, relu=True)
    fig["mean"], fig["rstd"] = R.stats_ratios(_np(stats), fwd)
    fig["y"] = R.ratio(_np(out), fwd.y, fwd.tol_y())
    spread = np.abs(fwd.mean) * np.sqrt(1.0 / np.maximum(fwd.var, 1e-300))
    print("|mean| / std up to %.3g, |y| up to %.3g" % (spread.max(), np.abs(y64).max()))
    _check("off=%d %s %s %s=%d" % (off, pyramid, mode, knob, value), fig)

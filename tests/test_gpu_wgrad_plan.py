"""scan_conv_wgrad_plan + scan_conv_wgrad_run (csrc/conv_api.hip) against the older entry points called under the same knobs:
dw and db bit for bit (torch.equal, no tolerance anywhere) -- the dispatcher launches the same kernels on the same split-K cut.

(A) 3x3 on a ragged shape: 136 input channels (a thin last channel tile), 72 output channels (a partial output tile), odd
    heights (row-pair chunks with a lone last row), widths below one K chunk; both piece counts, the four kernel variants, with
    and without db, accumulating.  (B) 3x3 on whole tiles.  (C) 1x1, stride 1 and 2.  (D) the generic family against
    scan_conv2d_wgrad followed by scan_colsum.  (E) the knobs moved between plan and run: the planned launch runs, inside the
    planned workspace.  (F) ops.conv2d's backward and the compiled operator's against the older symbols.
Every run of a plan gets a workspace with NaN behind plan.ws_floats, which must still be NaN afterwards."""
import contextlib
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

A_LEVELS, A_N, A_CS, A_COUT = [(13, 20), (7, 10)], 2, 136, 72
KNOB_SETS = {"default": {}, "wino0": {"wgrad_wino": 0}, "tile0": {"wgrad_tile": 0}, "v4": {"wgrad_v6": 0}}
PAD = 4096  # floats of NaN behind the planned workspace


@contextlib.contextmanager
def tuned(**knobs):
    from scan_amd import _lib
    old = {k: _lib.query("scan_tune", k.encode(), v) for k, v in knobs.items()}
    try:
        yield
    finally:
        for k, v in old.items():
            _lib.query("scan_tune", k.encode(), v)


def _inputs(device, xd, yd, cs, cout_s, seed):
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn((xd.rows, cs), device=device, generator=g)
    dy = torch.randn((yd.rows, cout_s), device=device, generator=g)
    return x, dy


def _outputs(device, cout, taps, cs, preset, seed=77):
    """(dw, db) to write into: NaN, or preset values to accumulate into (the same ones for every seed given)"""
    if not preset:
        return torch.full((cout, taps, cs), float("nan"), device=device), torch.full((cout,), float("nan"), device=device)
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randn((cout, taps, cs), device=device, generator=g), torch.randn((cout,), device=device, generator=g)


def make_plan(pieces, ksize, stride, cs, cout, xd, yd):
    from scan_amd import _lib
    plan = _lib.WgradPlan()
    _lib.call("scan_conv_wgrad_plan", pieces, ksize, stride, cs, cout, xd.ref(), yd.ref(), ctypes.byref(plan))
    return plan


def run_plan(plan, x, xd, dy, yd, cout_s, dw, db, accumulate):
    from scan_amd import _lib, ops
    ws = torch.full((plan.ws_floats + PAD,), float("nan"), device=x.device)
    _lib.call("scan_conv_wgrad_run", ctypes.byref(plan), ops._ptr(x), xd.ref(), plan.Cs, ops._ptr(dy), yd.ref(), plan.Cout, cout_s,
              ops._ptr(dw), ops._ptr(db) if db is not None else None, accumulate, ops._ptr(ws), ops._stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[plan.ws_floats:]).all()), "the launch wrote behind plan.ws_floats"
    return dw, db


def run_old(pieces, ksize, stride, x, xd, dy, yd, cs, cout, cout_s, dw, db, accumulate):
    """the entry points of before the dispatcher, under the current knobs; generic: scan_conv2d_wgrad, then scan_colsum"""
    from scan_amd import _lib, ops
    sfx = {2: "bf16x3", 3: "bf16x6"}.get(pieces)
    st, dbp = ops._stream(), (ops._ptr(db) if db is not None else None)
    if pieces and ksize == 3 and stride == 1:
        ws = torch.empty((_lib.query("scan_conv3x3_wgrad_%s_ws_floats" % sfx, xd.ref(), cs, cout),), device=x.device)
        _lib.call("scan_conv3x3_wgrad_" + sfx, ops._ptr(x), xd.ref(), cs, ops._ptr(dy), cout, cout_s, ops._ptr(dw), dbp, accumulate & 1,
                  ops._ptr(ws), st)
    elif pieces and ksize == 1:
        ws = torch.empty((_lib.query("scan_conv1x1_wgrad_%s_ws_floats" % sfx, yd.ref(), cs, cout),), device=x.device)
        _lib.call("scan_conv1x1_wgrad_" + sfx, ops._ptr(x), xd.ref(), cs, ops._ptr(dy), yd.ref(), cout, cout_s, stride, ops._ptr(dw), dbp,
                  accumulate & 1, ops._ptr(ws), st)
    else:
        ws = torch.empty((_lib.query("scan_conv2d_wgrad_ws_floats", yd.ref(), cs, cout, ksize),), device=x.device)
        _lib.call("scan_conv2d_wgrad", ops._ptr(x), xd.ref(), cs, ops._ptr(dy), yd.ref(), cout, cout_s, ksize, stride, ops._ptr(dw),
                  accumulate & 1, ops._ptr(ws), st)
        if db is not None:
            cws = torch.empty((_lib.query("scan_colsum_ws_floats", yd.rows, cout),), device=x.device)
            _lib.call("scan_colsum", ops._ptr(dy), yd.rows, cout, cout_s, dbp, accumulate >> 1, ops._ptr(cws), st)
    torch.cuda.synchronize()
    return dw, db


def both(device, pieces, ksize, stride, xd, cs, cout, cout_s, with_db=True, accumulate=0, seed=1):
    """plan + run and the older entry point on the same inputs -> ((dw, db), (dw, db), plan)"""
    yd = xd.conv_out(ksize, stride)
    x, dy = _inputs(device, xd, yd, cs, cout_s, seed)
    res = []
    plan = make_plan(pieces, ksize, stride, cs, cout, xd, yd)
    for new in (True, False):
        dw, db = _outputs(device, cout, ksize * ksize, cs, accumulate != 0)
        if accumulate == 1:  # flat dw, fresh db
            db.fill_(float("nan"))
        if not with_db:
            db = None
        res.append(run_plan(plan, x, xd, dy, yd, cout_s, dw, db, accumulate) if new else
                   run_old(pieces, ksize, stride, x, xd, dy, yd, cs, cout, cout_s, dw, db, accumulate))
    return res[0], res[1], plan


def same(a, b):
    assert bool(torch.isfinite(a[0]).all()) and torch.equal(a[0], b[0])
    assert (a[1] is None and b[1] is None) or (bool(torch.isfinite(a[1]).all()) and torch.equal(a[1], b[1]))


@pytest.mark.parametrize("mode", ["db", "no_db", "accumulate"])
@pytest.mark.parametrize("knobs", sorted(KNOB_SETS))
@pytest.mark.parametrize("pieces", [3, 2])
def test_a_3x3_ragged(device, pieces, knobs, mode):
    from scan_amd import _lib, ops
    with tuned(**KNOB_SETS[knobs]):
        new, old, plan = both(device, pieces, 3, 1, ops.PyramidShape(A_N, A_LEVELS), A_CS, A_COUT, A_COUT, with_db=mode != "no_db",
                              accumulate=3 if mode == "accumulate" else 0)
    want = {"default": _lib.WGRAD_V6_32X64_WINO if pieces == 3 else _lib.WGRAD_V6_64X32,
            "wino0": _lib.WGRAD_V6_32X64 if pieces == 3 else _lib.WGRAD_V6_64X32, "tile0": _lib.WGRAD_V6_64X32, "v4": _lib.WGRAD_V4}[knobs]
    assert (plan.family, plan.variant, plan.c_tiles) == (_lib.WGRAD_SPLIT3X3, want, 2)
    same(new, old)


def test_b_3x3_whole_tiles(device):
    from scan_amd import _lib, ops
    new, old, plan = both(device, 3, 3, 1, ops.PyramidShape(1, [(16, 64)]), 256, 256, 256)
    assert plan.variant == _lib.WGRAD_V6_32X64_WINO and plan.slab_taps == 12
    same(new, old)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("pieces", [3, 2])
def test_c_1x1(device, pieces, stride):
    from scan_amd import _lib, ops
    new, old, plan = both(device, pieces, 1, stride, ops.PyramidShape(A_N, A_LEVELS), 72, 136, 136)
    assert (plan.family, plan.variant, plan.stride, plan.slab_taps) == (_lib.WGRAD_SPLIT1X1, _lib.WGRAD_V4, stride, 1)
    same(new, old)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("case", ["fp32_3x3", "bf16x6_3x3_s2", "7x7_s2_cs4"])
def test_d_generic(device, case, accumulate):
    from scan_amd import _lib, ops
    pieces, ksize, stride, xd, cs, cout = {"fp32_3x3": (0, 3, 1, ops.PyramidShape(A_N, A_LEVELS), A_CS, A_COUT),
                                           "bf16x6_3x3_s2": (3, 3, 2, ops.PyramidShape(A_N, A_LEVELS), A_CS, A_COUT),
                                           "7x7_s2_cs4": (3, 7, 2, ops.PyramidShape(2, [(32, 48)]), 4, 64)}[case]
    new, old, plan = both(device, pieces, ksize, stride, xd, cs, cout, cout, accumulate=accumulate)
    assert (plan.family, plan.variant, plan.fused_db) == (_lib.WGRAD_GENERIC, _lib.WGRAD_FP32, 0)
    same(new, old)


def test_e_knobs_moved_after_planning(device):
    """the soundness the plan buys: planned under wgrad_wino = 1, run after wgrad_wino = 0 and wgrad_wgs = 512 -- the planned
    (Winograd) launch runs, in the planned workspace; the older query + launch pair would have sized 12-tap slabs as 9-tap ones"""
    from scan_amd import _lib, ops
    xd = ops.PyramidShape(A_N, A_LEVELS)
    x, dy = _inputs(device, xd, xd, A_CS, A_COUT, 5)
    with tuned(wgrad_wino=1):
        plan = make_plan(3, 3, 1, A_CS, A_COUT, xd, xd)
        assert plan.variant == _lib.WGRAD_V6_32X64_WINO
        left = run_plan(plan, x, xd, dy, xd, A_COUT, *_outputs(device, A_COUT, 9, A_CS, False), 0)
        with tuned(wgrad_wino=0):
            with tuned(wgrad_wgs=512):
                assert _lib.query("scan_conv3x3_wgrad_bf16x6_ws_floats", xd.ref(), A_CS, A_COUT) != plan.ws_floats
                moved = run_plan(plan, x, xd, dy, xd, A_COUT, *_outputs(device, A_COUT, 9, A_CS, False), 0)
    same(moved, left)


@pytest.mark.parametrize("ksize,stride,cin,cout", [(3, 1, A_CS, A_COUT), (1, 2, 72, 136)])
def test_f_bindings(device, ksize, stride, cin, cout):
    """ops.conv2d's backward on the whole pyramid, and the compiled operator's on each of its levels (it takes one NCHW level per
    call), against the older symbols on the same rows"""
    from scan_amd import layers as L
    from scan_amd import ops
    assert L.OPS_BACKEND == "compiled"
    g = torch.Generator().manual_seed(11)
    w = (torch.randn(cout, cin, ksize, ksize, generator=g) * 0.05).to(device).contiguous(memory_format=torch.channels_last)
    b = torch.randn(cout, generator=g).to(device)

    def old(x, xd, dy):
        dw, db = run_old(3, ksize, stride, x, xd, dy, xd.conv_out(ksize, stride), cin, cout, cout, *_outputs(device, cout, ksize * ksize, cin, False), 0)
        return ops.unpack_weight_grad(dw, w), db

    xd = ops.PyramidShape(A_N, A_LEVELS)
    x, dy = _inputs(device, xd, xd.conv_out(ksize, stride), cin, cout, 13)
    ww, bb = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ops.conv2d(x, ww, bb, xd, ksize, stride).backward(dy)
    torch.cuda.synchronize()
    same((ww.grad, bb.grad), old(x, xd, dy))
    for h, w_ in A_LEVELS:
        one = ops.PyramidShape(A_N, [(h, w_)])
        x, dy = _inputs(device, one, one.conv_out(ksize, stride), cin, cout, 17 + h)
        (ho, wo), = one.conv_out(ksize, stride).sizes
        xx = x.view(A_N, h, w_, cin).permute(0, 3, 1, 2)  # channels_last NCHW views of the same rows
        ww, bb = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        L._ops.conv2d(xx, ww, bb, stride, False).backward(dy.view(A_N, ho, wo, cout).permute(0, 3, 1, 2))
        torch.cuda.synchronize()
        same((ww.grad, bb.grad), old(x, one, dy))

"""The 1x1 convolutions -- forward, the two stride maps, data gradient, weight and bias gradient -- on every instance `pick1x1`
(csrc/conv_fwd.hip) can choose and in the three arithmetics, against the host oracle of tests/conv1x1_ref.py (numpy, float64 and
int64; pinned on the CPU by tests/test_conv1x1_host.py).

(1) Exact probes, no tolerance.  Inputs, weights, bias and dY are integers in [-8, 8]: each is one bf16 piece (the later pieces
    are zero), every product is an integer of magnitude <= 64 and every partial sum an integer below 2^24, so fp32, bf16x6 and
    bf16x3, in any summation order, must return the int64 result bit for bit.  The bound is written next to each case: 64 Cin + 8
    for the forward, 64 Cout for the data gradient, 64 rows + 8 for the weight gradient.  The weight-gradient cases keep
    rows * 64 < 2^24 (the largest pyramid has 32,736 rows: 2,095,104); the value range is not narrowed anywhere.
    Every case asserts the instance id scan_conv1x1_bf16x6_instance / scan_conv_plan report for it.
(2) Error against float64 on random, post-ReLU and large-dynamic-range data: the project's bars (test_conv_error_vs_fp64,
    test_wgrad_full_size_elementwise part (b), test_gpu_wgrad_winograd.py) where Cin >= 64, and for every element and every Cin
    the pointwise bound |got - ref| <= B S of conv1x1_ref's docstring: S = the sum of the absolute values of the element's terms,
    B = gamma(terms) with one ulp (2^-23) per addition, terms = K32 + 1 (fp32), 6 K32 + 1 (three pieces, + 3 * 2^-23 for the
    dropped piece products), 3 K32 + 1 (two pieces, + 2^-15), K32 = the reduction length rounded up to 32 (Cin; the dY channels
    for the data gradient; the dY rows for dw; rows + 1 terms for db).  B is derived there, not measured; the worst measured
    err / (B S) of every case is printed.

The output of a C-ABI launch lives in a buffer of SENTINEL with a margin on both sides; the live columns hold NaN before the call
(all of them must be written), the padding columns (Ns > Nout) hold the zeros the library's callers put there (scan_amd/ops.py,
csrc/scan_ops_ext.cpp: the kernels store whole float4 groups of live channels and nothing else) and must come back exactly zero."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import conv1x1_ref as R

pytestmark = pytest.mark.gpu

PYR = (2, [(12, 20), (6, 10)])                                    # two images, partial pixel tiles on both levels
ODD = (2, [(13, 21), (7, 11)])                                    # odd sizes: the stride maps' last row and column
FIVE = (2, [(9, 14), (5, 7), (3, 4), (1, 2), (1, 1)])             # SCAN_MAX_LEVELS levels, ending in a pair and a single pixel
WIDE = (3, [(64, 128), (32, 64), (16, 32), (8, 16), (4, 8)])      # 132 pixel tiles of 16 x 16: rounds 2 against 2 -> the 256-channel tile
WIDE2 = (3, [(128, 256), (64, 128), (32, 64), (16, 32), (8, 16)])  # its stride-2 source: conv_out(1, 2) is WIDE
RAGGED = (1, [(33, 673)])                                         # one ragged level, 3 x 43 = 129 tiles
SENTINEL, MARGIN, PAD = -777.25, 1024, 4096

# (CONV_MODE, knobs): every arithmetic, the independent two-piece kernel of conv_gen1.hip, every value of the 1x1 knob
CONFIGS = [("fp32", {}), ("bf16x6", {"conv1x1": 3}), ("bf16x6", {"conv1x1": 0}), ("bf16x6", {"conv1x1": 1}), ("bf16x6", {"conv1x1": 2}),
           ("bf16x3", {"conv_v2": 1}), ("bf16x3", {"conv_v2": 0})]
DEFAULTS = [("fp32", {}), ("bf16x6", {}), ("bf16x3", {})]


@contextlib.contextmanager
def tuned(**knobs):
    from scan_amd import _lib
    old = {k: _lib.query("scan_tune", k.encode(), v) for k, v in knobs.items()}
    try:
        yield
    finally:
        for k, v in old.items():
            _lib.query("scan_tune", k.encode(), v)


@contextlib.contextmanager
def conv_mode(mode):
    from scan_amd import ops
    keep, ops.CONV_MODE = ops.CONV_MODE, mode
    try:
        yield
    finally:
        ops.CONV_MODE = keep


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _round(c, m):
    return (c + m - 1) // m * m


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)


def _exact(got, ref, what):
    """got (device, fp32) == the int64 reference, bit for bit; NaN never passes"""
    assert int(np.abs(ref).max(initial=0)) < 2 ** 24, what
    want = _dev(ref, got.device)
    if not torch.equal(got, want):
        pytest.fail("%s: %s" % (what, R.first_mismatch(got.cpu().numpy(), ref.astype(np.float32))))


class Guarded:
    """rows x ns floats inside a buffer of SENTINEL with MARGIN floats in front and behind (tests/test_gpu_cond_rnn.py); the
    first `live` columns hold `fill` (NaN: to be written), the padding columns the zeros the library's callers provide"""

    def __init__(self, device, rows, ns, live, fill=float("nan")):
        self.buf = torch.full((rows * ns + 2 * MARGIN,), SENTINEL, dtype=torch.float32, device=device)
        self.block = self.buf[MARGIN:MARGIN + rows * ns].view(rows, ns)
        self.block[:, live:] = 0
        self.block[:, :live] = fill
        self.live = live

    def check(self, what):
        torch.cuda.synchronize()
        n = self.block.numel()
        assert bool((self.buf[:MARGIN] == SENTINEL).all()) and bool((self.buf[MARGIN + n:] == SENTINEL).all()), what + ": wrote outside the buffer"
        assert bool((self.block[:, self.live:] == 0).all()), what + ": padding columns are not exactly zero"
        return self.block[:, :self.live]


def _instance(yd, nout, csw):
    from scan_amd import _lib
    return _lib.query("scan_conv1x1_bf16x6_instance", yd.ref(), nout, csw)


def _dgrad_instance(xd, cin, cout, cout_s):
    """the instance scan_conv_plan reports for the data gradient of a cin -> cout conv whose dX lies on xd"""
    from scan_amd import _lib
    plan = _lib.ConvPlan()
    _lib.call("scan_conv_plan", 3, 1, 1, cout, cin, cout_s, xd.ref(), 0, ctypes.byref(plan))
    assert (plan.family, plan.nout, plan.csw) == (2, cin, _round(max(cout, cout_s), 8))
    return plan.instance


def _under(inst, knob):
    """the id an instance of the default knob (3) becomes under scan_tune conv1x1 = knob: bit 0 off -> register staging (128),
    bit 1 off -> no 256-channel tile"""
    if inst in (1128, 1256) and not knob & 1:
        return 128
    return 1128 if inst == 1256 and not knob & 2 else inst


def _step(mode, knobs, x, w, b, shape, stride, dy=None, relu=False, mask_dx=False, cout_s=None):
    """ops.conv2d forward (and backward from dy) under one configuration -> y, dx, dw [Cout, Cin], db"""
    from scan_amd import ops
    with conv_mode(mode), tuned(**knobs):
        if dy is None:
            with torch.no_grad():
                y = ops.conv2d(x, w, b, shape, 1, stride, relu=relu, cout_s=cout_s)
            torch.cuda.synchronize()
            return y, None, None, None
        xx, ww = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        bb = b.clone().requires_grad_(True) if b is not None else None
        y = ops.conv2d(xx, ww, bb, shape, 1, stride, relu=relu, mask_dx=mask_dx, cout_s=cout_s)
        y.backward(dy)
        torch.cuda.synchronize()
        return y.detach(), xx.grad, ww.grad.reshape(ww.shape[0], ww.shape[1]), bb.grad if bb is not None else None


# ============================================================================= (1) exact probes
# id: (pyramid, Cin, Cout, stride, forward instance, data-gradient instance) under the default knobs.
# |y| <= 64 Cin + 8, |dx| <= 64 Cout, |dw| <= 64 rows(yd) -- all below 2^24 = 16,777,216
EXACT = {
    "c4_n40": (PYR, 4, 40, 1, 64, 64),               # one K chunk with a 4-channel tail.  y 264, dx 2,560, dw 38,400
    "c32_n64": (PYR, 32, 64, 1, 64, 64),             # a whole chunk, a whole 64-channel tile.  y 2,056, dx 4,096, dw 38,400
    "c36_n72_s1": (ODD, 36, 72, 1, 128, 64),         # Csw = 40: register staging.  y 2,312, dx 4,608, dw 44,800
    "c36_n72_s2": (ODD, 36, 72, 2, 128, 64),         # maps 1 and 2 on odd sizes.  dw 12,928
    "c36_n136_s2": (ODD, 36, 136, 2, 128, 64),       # two 128-channel tiles, the second with 8 rows.  dx 8,704
    "c64_n128_s1": (ODD, 64, 128, 1, 1128, 64),      # LDS-DMA weights, whole tile.  y 4,104, dx 8,192, dw 44,800
    "c64_n128_s2": (ODD, 64, 128, 2, 1128, 64),
    "c64_n200_s1": (FIVE, 64, 200, 1, 1128, 64),     # 72 live rows in the last tile: the DMA reads past the plane.  dx 12,800, dw 22,528
    "c64_n200_s2": (FIVE, 64, 200, 2, 1128, 64),     # five levels through both stride maps: (1, 2) -> (1, 1), (1, 1) -> (1, 1)
    "c68_n136": (PYR, 68, 136, 1, 128, 128),         # Csw = 72, a 4-channel tail in the third chunk; dgrad Nout = 68 on Csw = 136
    "c512_n128": (PYR, 512, 128, 1, 1128, 1128),     # 16 chunks.  y 32,776; dgrad Nout = 512 on Csw = 128
    "wide_c64_n256_s1": (WIDE, 64, 256, 1, 1256, 64),    # 132 tiles: the 256-channel tile.  32,736 rows: dw 2,095,104
    "wide_c64_n256_s2": (WIDE2, 64, 256, 2, 1256, 64),   # the same output pyramid through map 1 (130,944 source rows)
    "wide_c256_n64_s2": (WIDE, 256, 64, 2, 64, 1256),    # data gradient on the 256-channel tile through map 2.  y 16,392
    "ragged_c64_n256": (RAGGED, 64, 256, 1, 1256, 64),   # 3 x 43 = 129 tiles of one ragged level.  22,209 rows: dw 1,421,376
}


@pytest.mark.parametrize("case", sorted(EXACT))
def test_exact_forward_dgrad_wgrad(device, case):
    """ops.conv2d forward + backward == int64 in every configuration (so the seven are bit-equal to each other: conv1x1 = 0..3,
    conv_v2 = 0); on the small pyramids a second pass with the ReLU epilogue and the deferred-ReLU mask on dX; on multi-level
    pyramids one level launched alone equals its rows of the pyramid launch."""
    from scan_amd import _lib, ops
    (n, sizes), cin, cout, stride, inst_f, inst_d = EXACT[case]
    xd = ops.PyramidShape(n, sizes)
    yd = xd.conv_out(1, stride)
    assert 64 * cin + 8 < 2 ** 24 and 64 * cout < 2 ** 24 and 64 * yd.rows + 8 < 2 ** 24
    assert _lib.query("scan_tune_default", b"conv1x1") == 3
    rs = np.random.RandomState(cin * 1000 + cout + stride)
    xh, wh, bh, dyh = R.int_inputs(rs, xd.rows, cin), R.int_inputs(rs, cout, cin), R.int_inputs(rs, cout), R.int_inputs(rs, yd.rows, cout)
    x, b, dy = _dev(xh, device), _dev(bh, device), _dev(dyh, device)
    w = _dev(wh, device).reshape(cout, cin, 1, 1)
    passes = [(False, False)] + ([(True, True)] if xd.rows < 5000 else [])
    for relu, mask_dx in passes:
        y_ref = R.forward(xh, wh, bh, xd, yd, stride - 1, relu=relu, dtype=R.I64)
        dye = dyh * (y_ref > 0) if relu else dyh
        dx_ref = R.forward(dye, wh.T, None, yd, xd, 0 if stride == 1 else 2, mask=xh if mask_dx else None, dtype=R.I64)
        dw_ref, db_ref = R.wgrad(xh, dye, xd, yd, stride, dtype=R.I64)
        if not relu:
            assert np.abs(y_ref).max() > 8 and np.abs(dx_ref).max() > 0 and np.abs(dw_ref).max() > 0
        for mode, knobs in CONFIGS:
            what = "%s %s %s relu=%d" % (case, mode, knobs, relu)
            with tuned(**knobs):
                if mode == "bf16x6":
                    k = knobs["conv1x1"]
                    assert _instance(yd, cout, _round(cin, 8)) == _under(inst_f, k), what
                    assert _dgrad_instance(xd, cin, cout, cout) == _under(inst_d, k), what
            y, dx, dw, db = _step(mode, knobs, x, w, b, xd, stride, dy, relu=relu, mask_dx=mask_dx)
            _exact(y, y_ref, what + " y")
            _exact(dx, dx_ref, what + " dx")
            _exact(dw, dw_ref, what + " dw")
            _exact(db, db_ref, what + " db")
            if xd.n_levels > 1 and not relu:
                l = xd.n_levels - 1
                yl, _, _, _ = _step(mode, knobs, x[xd.row_off[l]:xd.row_off[l + 1]].contiguous(), w, b, xd.level(l), stride)
                assert torch.equal(yl, y[yd.row_off[l]:yd.row_off[l + 1]]), what + " level %d alone" % l


def _planes(pieces, wp, dgrad, cs_src):
    """scan_weight_split / scan_weight_split3 planes of wp [O, 1, Cs_w] with the mode and the row length written out: forward
    [O][1][round8(Cs_w)], data gradient [Cs_w][1][round8(max(O, Cs_src))] -> (planes, Csw, Nout)"""
    from scan_amd import _lib
    O, T, cs_w = wp.shape
    rows, csw = (cs_w, _round(max(O, cs_src), 8)) if dgrad else (O, _round(cs_w, 8))
    planes = [torch.empty((rows, 1, csw), dtype=torch.bfloat16, device=wp.device) for _ in range(pieces)]
    _lib.call("scan_weight_split3" if pieces == 3 else "scan_weight_split", _p(wp), O, 1, cs_w, dgrad, *[_p(t) for t in planes], csw, None)
    return planes, csw, rows


def _capi(pieces, x, xd, yd, cmap, planes, csw, nout, bias, mask, relu, ns, what):
    """scan_conv1x1_bf16x6 / _bf16x3 into a guarded buffer -> the live columns"""
    from scan_amd import _lib
    g = Guarded(x.device, yd.rows, ns, nout)
    _lib.call("scan_conv1x1_bf16x6" if pieces == 3 else "scan_conv1x1_bf16x3", _p(x), xd.ref(), x.shape[1], *[_p(t) for t in planes], csw,
              _p(bias), _p(mask), _p(g.block), yd.ref(), nout, ns, relu, cmap, None)
    return g.check(what)


CAPI_CONFIGS = [(3, {"conv1x1": 3}), (3, {"conv1x1": 0}), (2, {"conv_v2": 1}), (2, {"conv_v2": 0})]
# (Cin, Nout, Ns > Nout, instance under conv1x1 = 3): |y| <= 64 Cin + 8 = 2,312 / 4,104
EPILOGUE_CHANNELS = {"c36_n72_ns80": (36, 72, 80, 128), "c64_n200_ns208": (64, 200, 208, 1128)}


@pytest.mark.parametrize("cmap", [0, 1, 2])
@pytest.mark.parametrize("chans", sorted(EPILOGUE_CHANNELS))
def test_exact_epilogues_capi(device, chans, cmap):
    """check1x1 (csrc/conv_api.hip) accepts bias, ReLU and the mask in every combination on every map (ops.py uses the mask on
    maps 0 and 2): all eight per map, three and two pieces, LDS-DMA and register staging, conv_gen1.hip -- each into a NaN-filled
    buffer with Ns > Nout and a sentinel margin.  On map 2 a bias reaches the odd coordinates too (src = the zero row)."""
    from scan_amd import ops
    cin, nout, ns, inst = EPILOGUE_CHANNELS[chans]
    fine = ops.PyramidShape(*ODD)
    coarse = fine.conv_out(1, 2)
    xd, yd = {0: (fine, fine), 1: (fine, coarse), 2: (coarse, fine)}[cmap]
    rs = np.random.RandomState(cin + nout + cmap)
    xh, wh, bh = R.int_inputs(rs, xd.rows, cin), R.int_inputs(rs, nout, cin), R.int_inputs(rs, nout)
    mh = R.int_inputs(rs, yd.rows, ns)
    x, wp, bias, mask = _dev(xh, device), _dev(wh, device).reshape(nout, 1, cin), _dev(bh, device), _dev(mh, device)
    for pieces, knobs in CAPI_CONFIGS:
        with tuned(**knobs):
            if pieces == 3:
                assert _instance(yd, nout, _round(cin, 8)) == _under(inst, knobs["conv1x1"])
            planes, csw, rows = _planes(pieces, wp, 0, cin)
            for use_b in (True, False):
                for relu in (0, 1):
                    for use_m in (False, True):
                        what = "%s map %d pieces %d %s bias=%d relu=%d mask=%d" % (chans, cmap, pieces, knobs, use_b, relu, use_m)
                        y = _capi(pieces, x, xd, yd, cmap, planes, csw, nout, bias if use_b else None, mask if use_m else None, relu, ns, what)
                        ref = R.forward(xh, wh, bh if use_b else None, xd, yd, cmap, relu=bool(relu),
                                        mask=mh[:, :nout] if use_m else None, dtype=R.I64)
                        _exact(y, ref, what)


def test_capi_two_pieces_unaligned_pitch_and_refusals(device):
    """Accepted: two pieces with a row pitch that is no multiple of 4 (Ns = 73) -- the launch falls back to conv_gen1.hip's scalar
    stores.  Refused with a RuntimeError: the same pitch or a misaligned y / mask with three pieces, map 3, pyramids that do not
    match the map, Ns < Nout, Cs % 4 != 0, Csw < Cs, a missing third plane, differing level counts; in ops.conv2d a 1x1 conv with
    the fused pool or with out= of another width; in scan_conv_run a 1x1 plan with the 3x3 epilogue flags."""
    from scan_amd import _lib, ops
    fine = ops.PyramidShape(*ODD)
    coarse = fine.conv_out(1, 2)
    cin, nout = 36, 72
    rs = np.random.RandomState(3)
    xh, wh, bh, mh = R.int_inputs(rs, fine.rows, cin), R.int_inputs(rs, nout, cin), R.int_inputs(rs, nout), R.int_inputs(rs, fine.rows, 73)
    x, wp, bias, mask = _dev(xh, device), _dev(wh, device).reshape(nout, 1, cin), _dev(bh, device), _dev(mh, device)
    for cmap, (xd, yd) in {0: (fine, fine), 1: (fine, coarse)}.items():
        planes, csw, _ = _planes(2, wp, 0, cin)
        y = _capi(2, x, xd, yd, cmap, planes, csw, nout, bias, mask[:yd.rows].contiguous(), 1, 73, "two pieces, Ns = 73, map %d" % cmap)
        _exact(y, R.forward(xh, wh, bh, xd, yd, cmap, relu=True, mask=mh[:yd.rows, :nout], dtype=R.I64), "two pieces, Ns = 73, map %d" % cmap)
    p3, csw, _ = _planes(3, wp, 0, cin)
    p2, _, _ = _planes(2, wp, 0, cin)
    out = torch.zeros((fine.rows * 80 + 8,), device=device)

    def refused(pieces=3, xx=x, xd=fine, yd=fine, planes=p3, csw=csw, mask=None, y=out, nout=nout, ns=80, cmap=0, cs=cin):
        with pytest.raises(RuntimeError):
            _lib.call("scan_conv1x1_bf16x6" if pieces == 3 else "scan_conv1x1_bf16x3", _p(xx), xd.ref(), cs, *[_p(t) for t in planes], csw,
                      _p(bias), _p(mask), _p(y), yd.ref(), nout, ns, 0, cmap, None)

    refused(ns=73)                                   # three pieces store float4
    refused(y=out[1:])                               # y not 16-byte aligned
    refused(mask=out[1:])                            # mask not 16-byte aligned
    refused(cmap=3)
    refused(cmap=1)                                  # yd is not ceil(xd / 2)
    refused(cmap=2, xd=fine, yd=coarse)              # map 2 takes the coarse pyramid in, the fine one out
    refused(cmap=0, yd=coarse)
    refused(ns=68)                                   # Ns < Nout
    refused(cs=38)                                   # Cs % 4
    refused(csw=32)                                  # Csw < Cs
    refused(csw=36)                                  # Csw % 8
    refused(planes=p2 + [None])                      # no third plane
    refused(pieces=2, planes=[p2[0], None])
    refused(yd=ops.PyramidShape(2, [(13, 21)]))      # level counts differ
    w4 = wp.reshape(nout, cin, 1, 1)
    with torch.no_grad():
        with pytest.raises(RuntimeError):
            ops.conv2d(x, w4, bias, fine, 1, 1, pool=True)
        with pytest.raises(RuntimeError):
            ops.conv2d(x, w4, bias, fine, 1, 1, cout_s=80, out=torch.empty((fine.rows, 80), device=device))
    plan = _lib.ConvPlan()
    _lib.call("scan_conv_plan", 3, 1, 0, nout, cin, cin, fine.ref(), _lib.CONV_SUMS, ctypes.byref(plan))
    ws = torch.zeros((fine.n_levels * 2 * 64,), dtype=torch.float64, device=device)
    with pytest.raises(RuntimeError):
        _lib.call("scan_conv_run", ctypes.byref(plan), _p(x), fine.ref(), cin, *[_p(t) for t in p3], _p(bias), None, _p(out), fine.ref(), 80,
                  0, 0, _p(ws), 1, None)
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0             # no refused call launched anything


# (Cs, Cout): dw rows 136 / 40 / 256; Cout_s = Cout + 4.  rows = 700 (stride 1) or 202 (stride 2): |dw| <= 64 * 700 + 8 = 44,808
WGRAD_CHANNELS = [(72, 136), (36, 40), (256, 256)]


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("cs,cout", WGRAD_CHANNELS)
@pytest.mark.parametrize("pieces", [3, 2])
def test_exact_wgrad_capi(device, pieces, cs, cout, stride):
    """scan_conv1x1_wgrad_bf16x6 / _bf16x3 and scan_conv_wgrad_plan + _run: with and without db, fresh (dw and db start as NaN) and
    accumulating into integers, Cout_s > Cout with nonzero padding columns in dY that must not be read, dw inside a sentinel margin,
    NaN behind the planned length of the workspace.  rows * 64 + 8 < 2^24 (above): the value range stays [-8, 8]."""
    from scan_amd import _lib, ops
    xd = ops.PyramidShape(*ODD)
    yd = xd.conv_out(1, stride)
    cout_s = cout + 4
    rs = np.random.RandomState(cs + cout + stride)
    xh, dyh = R.int_inputs(rs, xd.rows, cs), R.int_inputs(rs, yd.rows, cout_s)
    dyh[:, cout:] = 5
    dw0h, db0h = R.int_inputs(rs, cout, cs), R.int_inputs(rs, cout)
    x, dy = _dev(xh, device), _dev(dyh, device)
    sfx = "bf16x6" if pieces == 3 else "bf16x3"
    plan = _lib.WgradPlan()
    _lib.call("scan_conv_wgrad_plan", pieces, 1, stride, cs, cout, xd.ref(), yd.ref(), ctypes.byref(plan))
    assert (plan.family, plan.variant, plan.stride, plan.slab_taps, plan.Cs, plan.Cout) == (_lib.WGRAD_SPLIT1X1, _lib.WGRAD_V4, stride, 1, cs, cout)
    old_floats = _lib.query("scan_conv1x1_wgrad_%s_ws_floats" % sfx, yd.ref(), cs, cout)
    for planned in (True, False):
        for with_db in (True, False):
            for acc in (0, 1):
                what = "wgrad %s Cs=%d Cout=%d stride=%d planned=%d db=%d accumulate=%d" % (sfx, cs, cout, stride, planned, with_db, acc)
                g = Guarded(device, cout, cs, cs, fill=_dev(dw0h, device) if acc else float("nan"))
                db = (_dev(db0h, device) if acc else torch.full((cout,), float("nan"), device=device)) if with_db else None
                n_ws = plan.ws_floats if planned else old_floats
                ws = torch.full((n_ws + PAD,), float("nan"), device=device)
                if planned:
                    _lib.call("scan_conv_wgrad_run", ctypes.byref(plan), _p(x), xd.ref(), cs, _p(dy), yd.ref(), cout, cout_s, _p(g.block),
                              _p(db), 3 * acc if with_db else acc, _p(ws), None)
                else:
                    _lib.call("scan_conv1x1_wgrad_" + sfx, _p(x), xd.ref(), cs, _p(dy), yd.ref(), cout, cout_s, stride, _p(g.block), _p(db),
                              acc, _p(ws), None)
                dw = g.check(what)
                assert bool(torch.isnan(ws[n_ws:]).all()), what + ": wrote behind the workspace"
                dw_ref, db_ref = R.wgrad(xh, dyh[:, :cout], xd, yd, stride, dw0h if acc else None, db0h if acc else None, dtype=R.I64)
                _exact(dw, dw_ref, what + " dw")
                if with_db:
                    _exact(db, db_ref, what + " db")


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("cin,cout", [(36, 72), (64, 200)])
def test_bindings_equal_capi(device, cin, cout, stride):
    """ops.conv2d(..., 1, stride) on the pyramid and the compiled operator (csrc/scan_ops_ext.cpp) on one level, forward and
    backward, against the C-ABI entry points on hand-split planes: random data, bit for bit"""
    from scan_amd import _lib, ops
    from scan_amd import layers as L
    assert L.OPS_BACKEND == "compiled"
    g = torch.Generator().manual_seed(cin + cout + stride)
    w = (torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5).to(device)
    b = torch.randn(cout, generator=g).to(device)

    def capi(x, xd, dy):
        yd = xd.conv_out(1, stride)
        wp = w.reshape(cout, 1, cin)
        planes, csw, _ = _planes(3, wp, 0, cin)
        y = _capi(3, x, xd, yd, stride - 1, planes, csw, cout, b, None, 0, cout, "forward")
        planes, csw, _ = _planes(3, wp, 1, cout)
        dx = _capi(3, dy, yd, xd, 0 if stride == 1 else 2, planes, csw, cin, None, None, 0, cin, "dgrad")
        dw = torch.full((cout, 1, cin), float("nan"), device=device)
        db = torch.full((cout,), float("nan"), device=device)
        ws = torch.empty((_lib.query("scan_conv1x1_wgrad_bf16x6_ws_floats", yd.ref(), cin, cout),), device=device)
        _lib.call("scan_conv1x1_wgrad_bf16x6", _p(x), xd.ref(), cin, _p(dy), yd.ref(), cout, cout, stride, _p(dw), _p(db), 0, _p(ws), None)
        torch.cuda.synchronize()
        return y, dx, dw.reshape(cout, cin), db

    def same(got, want, what):
        for a, c, name in zip(got, want, ("y", "dx", "dw", "db")):
            assert bool(torch.isfinite(c).all()) and torch.equal(a, c), "%s %s" % (what, name)

    xd = ops.PyramidShape(*ODD)
    yd = xd.conv_out(1, stride)
    x = torch.randn(xd.rows, cin, generator=g).to(device)
    dy = torch.randn(yd.rows, cout, generator=g).to(device)
    same(_step("bf16x6", {}, x, w, b, xd, stride, dy), capi(x, xd, dy), "ops.conv2d")
    n, (h, wd) = ODD[0], ODD[1][0]
    one = ops.PyramidShape(n, [(h, wd)])
    (ho, wo), = one.conv_out(1, stride).sizes
    x1, dy1 = x[:one.rows].contiguous(), dy[:n * ho * wo].contiguous()
    ww, bb = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    xx = x1.view(n, h, wd, cin).permute(0, 3, 1, 2).requires_grad_(True)   # channels_last NCHW views of the same rows
    y = L._ops.conv2d(xx, ww, bb, stride, False)
    y.backward(dy1.view(n, ho, wo, cout).permute(0, 3, 1, 2))
    torch.cuda.synchronize()
    got = (y.detach().permute(0, 2, 3, 1).reshape(-1, cout), xx.grad.permute(0, 2, 3, 1).reshape(-1, cin), ww.grad.reshape(cout, cin), bb.grad)
    same(got, capi(x1, one, dy1), "compiled operator")


# ============================================================================= (2) error against float64
def _float_inputs(device, xd, yd, cin, cout, kind, seed):
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn((xd.rows, cin), device=device, generator=g)
    if kind == "relu":        # post-ReLU: half the inputs exactly zero
        x = x.clamp_min(0)
    elif kind == "range":     # values over 2^-20 .. 2^20 (the "range" kind of tests/test_gpu_winograd.py)
        x = x * torch.exp2(torch.randint(-20, 21, x.shape, device=device, generator=g).float())
    w = torch.randn((cout, cin, 1, 1), device=device, generator=g) / cin ** 0.5
    b = torch.randn((cout,), device=device, generator=g)
    dy = torch.randn((yd.rows, cout), device=device, generator=g)
    return x, w, b, dy


def _rel(got, ref):
    """(worst, rms) of |got - ref| relative to the largest |ref|"""
    d = np.abs(got.astype(np.float64) - ref) / np.abs(ref).max()
    return float(d.max()), float(np.sqrt((d ** 2).mean()))


def _project_bars(rel, what, wgrad=False):
    """rel: mode -> (worst, rms) relative to the largest element.  Forward / data gradient: the bars of test_conv_error_vs_fp64
    (three pieces: worst <= 5e-6, rms <= 1.1x and worst <= 1.5x the fp32-MFMA kernel's; two pieces: rms <= 5e-5 and not below three).
    Weight gradient: worst <= 5e-6 for three pieces, <= 1e-4 for two (test_wgrad_full_size_elementwise part (b),
    tests/test_gpu_wgrad_winograd.py; the 1x1 weight gradient runs conv_wgrad_v4_kernel, which like scan_tune wgrad_tile = 0 there
    has no temporary accumulator, so the ratio to the fp32-MFMA kernel is printed, not barred)"""
    (w32, r32), (w6, r6), (w3, r3) = rel["fp32"], rel["bf16x6"], rel["bf16x3"]
    assert w6 <= 5e-6, (what, rel)
    if wgrad:
        assert w3 <= 1e-4, (what, rel)
        return
    assert r6 <= 1.1 * r32, (what, rel)
    assert w6 <= 1.5 * w32, (what, rel)
    assert r3 <= 5e-5 and r3 >= r6, (what, rel)


# id: (pyramid, Cin, Cout, stride, forward instance under the default knobs, kinds)
ALL_KINDS = ("randn", "relu", "range")
ERROR = {
    "c4_n40": (PYR, 4, 40, 1, 64, ("randn",)),            # below Cin 64: the pointwise bound only
    "c36_n72_s2": (ODD, 36, 72, 2, 128, ("randn",)),
    "c64_n128_s1": (ODD, 64, 128, 1, 1128, ALL_KINDS),
    "c64_n128_s2": (ODD, 64, 128, 2, 1128, ALL_KINDS),
    "c64_n200_s1": (FIVE, 64, 200, 1, 1128, ALL_KINDS),
    "c64_n200_s2": (FIVE, 64, 200, 2, 1128, ALL_KINDS),
    "c68_n136": (PYR, 68, 136, 1, 128, ALL_KINDS),
    "c512_n128": (PYR, 512, 128, 1, 1128, ALL_KINDS),
    "wide_c64_n256_s1": (WIDE, 64, 256, 1, 1256, ALL_KINDS),
    "wide_c64_n256_s2": (WIDE2, 64, 256, 2, 1256, ALL_KINDS),
    "wide_c256_n64_s2": (WIDE, 256, 64, 2, 64, ALL_KINDS),
    "ragged_c64_n256": (RAGGED, 64, 256, 1, 1256, ALL_KINDS),
}


@pytest.mark.parametrize("case,kind", [(c, k) for c in sorted(ERROR) for k in ERROR[c][5]])
def test_error_vs_fp64(device, case, kind):
    """y, dx, dw, db of ops.conv2d in the three arithmetics against float64 from the same fp32 arrays: the pointwise bound for every
    element (docstring of the module; the ratio printed is the worst err / (B S), which must be <= 1), the project's bars where
    Cin >= 64.  "relu": the ReLU epilogue in the forward and the deferred-ReLU mask on dX; outputs within 1e-3 of zero get no dY, so a
    mask flipped by rounding cannot enter (as test_conv2d_fwd_bwd does).

    Measured on an MI355X, worst err / (B S) over all cases (y, dx, dw, db): bf16x6 0.0073, 0.0022, 0.0024, 0.0038; fp32 0.093,
    0.043, 0.036, 0.0096; bf16x3 0.42, 0.15, 0.22, 0.0038 -- evidence, not bars.

    What this test found: without the per-chunk temporary accumulator of the three-piece 1x1 instances (csrc/conv_fwd.hip,
    mma_pieces TEMP) four "relu" cases missed the bar "rms <= 1.1x the fp32-MFMA kernel's" -- c512_n128 y 1.12x, c64_n200_s1 dx
    1.14x, ragged_c64_n256 dx 1.15x, wide_c64_n256_s1 dx 1.15x (dense data 0.80x - 0.83x): zero operands make steps of an fp32
    fma chain exact, while six MFMA results per 32-channel chunk were rounded at the running accumulator's magnitude whatever the
    data held.  With the temporary the same four sit at 0.35x, 0.41x, 0.36x, 0.36x."""
    from scan_amd import ops
    (n, sizes), cin, cout, stride, inst, _ = ERROR[case]
    xd = ops.PyramidShape(n, sizes)
    yd = xd.conv_out(1, stride)
    assert _instance(yd, cout, _round(cin, 8)) == inst
    relu = kind == "relu"
    x, w, b, dy = _float_inputs(device, xd, yd, cin, cout, kind, seed=cin * 7 + cout + stride)
    xh, wh, bh = x.cpu().numpy(), w.reshape(cout, cin).cpu().numpy(), b.cpu().numpy()
    cmap_d = 0 if stride == 1 else 2
    pre = R.forward(xh, wh, bh, xd, yd, stride - 1)
    if relu:
        dy = dy * torch.from_numpy(np.abs(pre) > 1e-3).to(device)
    dyh = dy.cpu().numpy()
    dye = dyh * (pre > 0) if relu else dyh
    ref = {"y": np.maximum(pre, 0) if relu else pre,
           "dx": R.forward(dye, wh.T, None, yd, xd, cmap_d, mask=xh if relu else None)}
    ref["dw"], ref["db"] = R.wgrad(xh, dye, xd, yd, stride)
    S = {"y": R.forward_abs(xh, wh, bh, xd, yd, stride - 1), "dx": R.forward_abs(dye, wh.T, None, yd, xd, cmap_d)}
    S["dw"], S["db"] = R.wgrad_abs(xh, dye, xd, yd, stride)
    K = {"y": cin, "dx": cout, "dw": yd.rows, "db": yd.rows}
    rel = {name: {} for name in ref}
    ratios = {}
    for mode, knobs in DEFAULTS:
        got = dict(zip(("y", "dx", "dw", "db"), _step(mode, knobs, x, w, b, xd, stride, dy, relu=relu, mask_dx=relu)))
        for name in ("y", "dx", "dw", "db"):
            gh = got[name].cpu().numpy()
            ratios[mode, name] = R.worst_ratio(gh, ref[name], R.bound_factor(mode, K[name], colsum=name == "db") * S[name])
            rel[name][mode] = _rel(gh, ref[name])
    print("conv1x1 err/(B S) %s %s:" % (case, kind), " ".join("%s/%s=%.4f" % (m, nm, r) for (m, nm), r in sorted(ratios.items())))
    print("   relative to the largest (worst, rms):", {nm: {m: "%.2e %.2e" % v for m, v in r.items()} for nm, r in rel.items()})
    assert max(ratios.values()) <= 1.0, ratios
    if cin >= 64:
        _project_bars(rel["y"], case + " y")
        _project_bars(rel["dx"], case + " dx")
        _project_bars(rel["dw"], case + " dw", wgrad=True)
        assert rel["db"]["bf16x6"][0] <= 5e-6 and rel["db"]["bf16x3"][0] <= 5e-6, rel["db"]


# one full-size row per instance: 1x1 convs of the ResNet-50 body and the FPN laterals at the bench shape (4 frames of 1024 x 2048,
# tools/conv_bench.py SHAPES_1X1).  id: (frames, level, Cin, Cout, knobs, forward instance)
FULL = {
    "layer1_conv1_256_64": (4, (256, 512), 256, 64, {}, 64),
    "layer2_conv1_512_128_registers": (4, (128, 256), 512, 128, {"conv1x1": 0}, 128),
    "layer2_conv1_512_128": (4, (128, 256), 512, 128, {}, 1128),
    "layer3_conv3_256_1024": (4, (64, 128), 256, 1024, {}, 1256),
}


@pytest.mark.parametrize("case", sorted(FULL))
def test_error_vs_fp64_full_size_sampled(device, case):
    """forward and data gradient at full size; 2,048 sampled pixels (corners and borders forced in), all channels, are copied to the
    host and held to the same pointwise bound and project bars"""
    from scan_amd import ops
    n, (h, wd), cin, cout, knobs, inst = FULL[case]
    xd = ops.PyramidShape(n, [(h, wd)])
    with tuned(**knobs):
        assert _instance(xd, cout, cin) == inst
    g = torch.Generator(device=device).manual_seed(cin + cout)
    x = torch.randn((xd.rows, cin), device=device, generator=g)
    w = torch.randn((cout, cin, 1, 1), device=device, generator=g) / cin ** 0.5
    b = torch.randn((cout,), device=device, generator=g)
    dy = torch.randn((xd.rows, cout), device=device, generator=g)
    rs = np.random.RandomState(cin)
    rows = rs.randint(0, xd.rows, 2048)
    rows[:8] = [0, wd - 1, (h - 1) * wd, h * wd - 1, h * wd, xd.rows - wd, xd.rows - 1, xd.rows - h * wd]
    rows_d = torch.from_numpy(rows).to(device)
    xs, dys = x[rows_d].cpu().numpy(), dy[rows_d].cpu().numpy()
    wh, bh = w.reshape(cout, cin).cpu().numpy(), b.cpu().numpy()
    one = R.Shape(1, [(1, 2048)])
    ref = {"y": R.forward(xs, wh, bh, one, one, 0), "dx": R.forward(dys, wh.T, None, one, one, 0)}
    S = {"y": R.forward_abs(xs, wh, bh, one, one, 0), "dx": R.forward_abs(dys, wh.T, None, one, one, 0)}
    K = {"y": cin, "dx": cout}
    rel, ratios = {"y": {}, "dx": {}}, {}
    for mode, _ in DEFAULTS:
        with conv_mode(mode), tuned(**knobs):
            xx = x.requires_grad_(True)
            y = ops.conv2d(xx, w, b, xd, 1, 1)
            y.backward(dy)
            got = {"y": y.detach()[rows_d].cpu().numpy(), "dx": xx.grad[rows_d].cpu().numpy()}
            xx.grad = None
            del y
        for name in ("y", "dx"):
            ratios[mode, name] = R.worst_ratio(got[name], ref[name], R.bound_factor(mode, K[name]) * S[name])
            rel[name][mode] = _rel(got[name], ref[name])
    print("conv1x1 full size err/(B S) %s:" % case, " ".join("%s/%s=%.4f" % (m, nm, r) for (m, nm), r in sorted(ratios.items())))
    print("   relative to the largest (worst, rms):", {nm: {m: "%.2e %.2e" % v for m, v in r.items()} for nm, r in rel.items()})
    assert max(ratios.values()) <= 1.0, ratios
    _project_bars(rel["y"], case + " y")
    _project_bars(rel["dx"], case + " dx")

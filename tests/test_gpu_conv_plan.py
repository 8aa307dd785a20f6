"""The conv dispatcher of the library (scan_conv_plan / scan_conv_weight_split / scan_conv_run, csrc/conv_api.hip) against the
single-launch entry points it chooses among: for every kernel family, epilogue and stride map, scan_conv_run on planes from
scan_conv_weight_split must equal BIT FOR BIT the named entry point on planes from scan_weight_split / scan_weight_split3 that
the test splits by hand (mode and row length written out here, not read from the plan).  Same kernel, same planes, same launch:
there is no rounding to allow for.  Only the GroupNorm sums leave their workgroups as fp64 atomics, whose order is not fixed; they
are compared within the fp64 reordering bound worked out in _sums_bound."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

PYR = [(12, 20), (6, 10)]     # two images on a two-level pyramid: partial pixel tiles on both levels
ODD = [(13, 21), (7, 11)]     # odd sizes for the stride-2 1x1 maps
N = 2
DIRECT, WINO, ONE = 0, 1, 2   # SCAN_CONV_DIRECT3X3 / SCAN_CONV_WINO3X3 / SCAN_CONV_1X1


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _rand(g, device, *shape):
    return torch.randn(*shape, generator=g).to(device)


def _round(c, m):
    return (c + m - 1) // m * m


class _Wino:
    """scan_tune "conv_wino" for the duration of a case"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        from scan_amd import _lib
        self.old = _lib.query("scan_tune", b"conv_wino", self.value)

    def __exit__(self, *exc):
        from scan_amd import _lib
        _lib.query("scan_tune", b"conv_wino", self.old)


def _planned(pieces, dgrad, wp, x, xd, bias, mask, yd, rows_out, relu=0, cmap=0, flags=0, ws=None, clear=0):
    """(plan, y) of scan_conv_run on planes from scan_conv_weight_split"""
    from scan_amd import _lib
    O, T, cs_w = wp.shape
    plan = _lib.ConvPlan()
    _lib.call("scan_conv_plan", pieces, T, dgrad, O, cs_w, x.shape[1], yd.ref(), flags, ctypes.byref(plan))
    planes = [torch.empty((plan.plane_rows, plan.plane_taps, plan.csw), dtype=torch.bfloat16, device=x.device) for _ in range(pieces)]
    _lib.call("scan_conv_weight_split", ctypes.byref(plan), _p(wp), *[_p(t) for t in planes], *[None] * (3 - pieces), None)
    y = torch.zeros((rows_out, plan.nout), device=x.device)
    _lib.call("scan_conv_run", ctypes.byref(plan), _p(x), xd.ref(), x.shape[1], *[_p(t) for t in planes], *[None] * (3 - pieces),
              _p(bias), _p(mask), _p(y), yd.ref(), plan.nout, relu, cmap, _p(ws), clear, None)
    return plan, y


def _legacy_planes(pieces, dgrad, wino, wp, cs_src):
    """planes by scan_weight_split / scan_weight_split3 with the mode and row length spelled out: 3x3 rows are padded to 32
    channels, 1x1 rows to 8; forward [O][T][round(Cs_w)], dgrad [Cs_w][T][round(max(O, Cs_src))]; Winograd: mode + 2, 12 taps"""
    from scan_amd import _lib
    O, T, cs_w = wp.shape
    m = 32 if T == 9 else 8
    rows, csw = (cs_w, _round(max(O, cs_src), m)) if dgrad else (O, _round(cs_w, m))
    mode = dgrad + (2 if wino else 0)
    planes = [torch.empty((rows, 12 if wino else T, csw), dtype=torch.bfloat16, device=wp.device) for _ in range(pieces)]
    if pieces == 3:
        _lib.call("scan_weight_split3", _p(wp), O, T, cs_w, mode, *[_p(t) for t in planes], csw, None)
    else:
        _lib.call("scan_weight_split", _p(wp), O, T, cs_w, mode, *[_p(t) for t in planes], csw, None)
    return planes, csw, (cs_w if dgrad else O)


def _legacy3x3(pieces, dgrad, wino, wp, x, d, bias, mask, relu=0):
    """scan_conv3x3_wino_bf16x6 (wino) or scan_conv3x3_bf16x3 / _bf16x6 on hand-split planes"""
    from scan_amd import _lib
    planes, csw, nout = _legacy_planes(pieces, dgrad, wino, wp, x.shape[1])
    y = torch.zeros((d.rows, nout), device=x.device)
    head = (_p(x), d.ref(), x.shape[1], *[_p(t) for t in planes], csw, _p(bias), _p(mask), _p(y), nout, nout, relu)
    if wino:
        _lib.call("scan_conv3x3_wino_bf16x6", *head, None, 0, None)
    else:
        _lib.call("scan_conv3x3_bf16x6" if pieces == 3 else "scan_conv3x3_bf16x3", *head, None)
    return y


def _case(device, cin, cout, sizes=PYR, seed=0):
    from scan_amd import ops
    g = torch.Generator().manual_seed(1000 * cin + cout + seed)
    d = ops.PyramidShape(N, sizes)
    return (d, _rand(g, device, d.rows, cin), _rand(g, device, cout, 9, cin) / (9 * cin) ** 0.5, _rand(g, device, cout),
            _rand(g, device, d.rows, cout))


@pytest.mark.parametrize("pieces", [3, 2])
@pytest.mark.parametrize("conv_wino", [1, 0])
def test_conv3x3_forward_and_dgrad(device, pieces, conv_wino):
    """Cin 36 -> Cout 72.  Forward: Nout = 72 > 64 and no tile multiple -- the Winograd instance with three pieces and conv_wino on,
    the direct kernel otherwise.  Data gradient: Nout = 36 <= 64 is always direct; the gradient of the 72 -> 36 conv (Nout = 72)
    takes Winograd again."""
    d, x, wp, bias, dy = _case(device, 36, 72)
    with _Wino(conv_wino):
        wino = pieces == 3 and conv_wino == 1
        plan, y = _planned(pieces, 0, wp, x, d, bias, None, d, d.rows)
        assert (plan.family, plan.split_mode, plan.plane_taps, plan.csw, plan.rem) == ((WINO, 2, 12, 64, 0) if wino else (DIRECT, 0, 9, 64, 0))
        assert torch.equal(y, _legacy3x3(pieces, 0, wino, wp, x, d, bias, None))
        plan, dx = _planned(pieces, 1, wp, dy, d, None, None, d, d.rows)
        assert (plan.family, plan.split_mode, plan.nout, plan.csw) == (DIRECT, 1, 36, 96)
        assert torch.equal(dx, _legacy3x3(pieces, 1, False, wp, dy, d, None, None))
        d2, x2, wp2, _, dy2 = _case(device, 72, 36)
        plan, dx2 = _planned(pieces, 1, wp2, dy2, d2, None, None, d2, d2.rows)
        assert (plan.family, plan.split_mode, plan.nout, plan.csw) == ((WINO, 3, 72, 64) if wino else (DIRECT, 1, 72, 64))
        assert torch.equal(dx2, _legacy3x3(pieces, 1, wino, wp2, dy2, d2, None, None))
        assert float(y.abs().max()) > 0 and float(dx.abs().max()) > 0 and float(dx2.abs().max()) > 0


@pytest.mark.parametrize("pieces", [3, 2])
def test_conv3x3_cout8_is_direct(device, pieces):
    d, x, wp, bias, _ = _case(device, 36, 8)
    plan, y = _planned(pieces, 0, wp, x, d, bias, None, d, d.rows)
    assert (plan.family, plan.split_mode, plan.plane_taps, plan.rem) == (DIRECT, 0, 9, 0)
    assert torch.equal(y, _legacy3x3(pieces, 0, False, wp, x, d, bias, None))


@pytest.mark.parametrize("pieces", [3, 2])
def test_conv3x3_relu_and_mask(device, pieces):
    """ReLU in the epilogue and the deferred-ReLU mask of a data gradient (y = 0 where mask <= 0), both at once"""
    d, x, wp, bias, mask = _case(device, 36, 72)
    plan, y = _planned(pieces, 0, wp, x, d, bias, mask, d, d.rows, relu=1)
    assert plan.family == (WINO if pieces == 3 else DIRECT)
    ref = _legacy3x3(pieces, 0, pieces == 3, wp, x, d, bias, mask, relu=1)
    assert torch.equal(y, ref)
    assert bool((y[mask <= 0] == 0).all()) and float(y.min()) == 0.0 and float(y.max()) > 0


def _sums_bound(y, d, passes):
    """Bound on the difference of two fp64 accumulations of the same addends in another order, per (level, image, group): every
    addend is y or y * y of one of the 8 channels of a group at one pixel -- at most K = pixels * 8 per pass -- and a chain of K fp64
    additions is off by at most K * 2^-53 * sum |addend|; two such chains differ by at most twice that.  -> [levels * N * 32, 2]"""
    out = []
    for l, (h, w) in enumerate(d.sizes):
        for i in range(d.n_images):
            blk = y[d.row_off[l] + i * h * w:d.row_off[l] + (i + 1) * h * w].double().reshape(h * w, 32, 8)
            k = passes * h * w * 8
            out.append(torch.stack([blk.abs().sum((0, 2)), (blk * blk).sum((0, 2))], 1) * (2 * passes * k * 2.0 ** -53))
    return torch.cat(out)


@pytest.mark.parametrize("pieces", [3, 2])
def test_conv3x3_groupnorm_sums_clear_then_accumulate(device, pieces):
    """Cin 36 -> 256 with GroupNorm sums: clear = 1, then clear = 0 into the same workspace (the sums double).  Three pieces:
    scan_conv3x3_wino_bf16x6 with a workspace; two: scan_conv3x3_gn_bf16x3, then scan_conv3x3_gn_acc_bf16x3."""
    from scan_amd import _lib
    d, x, wp, bias, _ = _case(device, 36, 256)
    n_ws = d.n_levels * N * 32 * 2
    ws = torch.full((n_ws,), 7.0, dtype=torch.float64, device=device)  # clear = 1 must not care what is there
    ref_ws = torch.full((n_ws,), -3.0, dtype=torch.float64, device=device)
    planes, csw, nout = _legacy_planes(pieces, 0, pieces == 3, wp, 36)
    for clear in (1, 0):
        plan, y = _planned(pieces, 0, wp, x, d, bias, None, d, d.rows, flags=_lib.CONV_SUMS, ws=ws, clear=clear)
        assert (plan.family, plan.instance if pieces == 3 else 0) == ((WINO, 3128) if pieces == 3 else (DIRECT, 0))
        ref = torch.zeros((d.rows, 256), device=device)
        if pieces == 3:
            _lib.call("scan_conv3x3_wino_bf16x6", _p(x), d.ref(), 36, *[_p(t) for t in planes], csw, _p(bias), None, _p(ref), 256,
                      256, 0, _p(ref_ws), clear, None)
        else:
            _lib.call("scan_conv3x3_gn_bf16x3" if clear else "scan_conv3x3_gn_acc_bf16x3", _p(x), d.ref(), 36,
                      *[_p(t) for t in planes], csw, _p(bias), _p(ref), 256, 256, _p(ref_ws), None)
        assert torch.equal(y, ref)
        passes = 1 if clear else 2
        diff = (ws - ref_ws).abs().reshape(-1, 2)
        print("sums: pass %d, largest difference %.3e, smallest bound %.3e" % (passes, float(diff.max()),
                                                                                 float(_sums_bound(y, d, passes).min())))
        assert bool((diff <= _sums_bound(y, d, passes)).all())
    # and they are the sums: (level 0, image 0) holds twice one pass over its 240 pixels.  A coarse bar, three roundings of
    # 2^-24 on sums of at most sum |addend|: the epilogue widens every element before it adds or squares it, and
    # tests/test_gpu_groupnorm_parity.py holds these sums to 2^-53 bars
    blk = y[:240].double().reshape(240, 32, 8)
    once = torch.stack([blk.sum((0, 2)), (blk * blk).sum((0, 2))], 1)
    mag = torch.stack([blk.abs().sum((0, 2)), (blk * blk).sum((0, 2))], 1)
    assert bool(((ws.reshape(-1, 32, 2)[0] - 2 * once).abs() <= 2 * 4 * 2.0 ** -24 * mag).all())


@pytest.mark.parametrize("pieces,conv_wino", [(3, 1), (3, 0), (2, 1)])
def test_conv3x3_fused_pool(device, pieces, conv_wino):
    """conv + bias + ReLU + 2x2 max-pool on one level (12, 20): the Winograd instance with relu bit 1, or scan_conv3x3_pool2_*"""
    from scan_amd import _lib, ops
    d, x, wp, bias, _ = _case(device, 36, 72, sizes=[(12, 20)])
    rows_out = N * 6 * 10
    with _Wino(conv_wino):
        wino = pieces == 3 and conv_wino == 1
        plan, y = _planned(pieces, 0, wp, x, d, bias, None, d, rows_out, relu=1, flags=_lib.CONV_POOL)
        assert plan.family == (WINO if wino else DIRECT)
        planes, csw, nout = _legacy_planes(pieces, 0, wino, wp, 36)
        ref = torch.zeros((rows_out, 72), device=device)
        if wino:
            _lib.call("scan_conv3x3_wino_bf16x6", _p(x), d.ref(), 36, *[_p(t) for t in planes], csw, _p(bias), None, _p(ref), 72, 72,
                      1 | 2, None, 0, None)
        else:
            _lib.call("scan_conv3x3_pool2_bf16x6" if pieces == 3 else "scan_conv3x3_pool2_bf16x3", _p(x), d.ref(), 36,
                      *[_p(t) for t in planes], csw, _p(bias), _p(ref), 72, 72, 1, None)
    assert torch.equal(y, ref) and float(y.max()) > 0
    pooled, _ = ops.maxpool2x2(_legacy3x3(pieces, 0, False, wp, x, d, bias, None, relu=1), d)
    if not wino:  # the direct kernel's pool is its own unfused output pooled, bit for bit
        assert torch.equal(y, pooled)


def _legacy1x1(pieces, dgrad, wp, x, xd, bias, yd, cmap):
    from scan_amd import _lib
    planes, csw, nout = _legacy_planes(pieces, dgrad, False, wp, x.shape[1])
    y = torch.zeros((yd.rows, nout), device=x.device)
    _lib.call("scan_conv1x1_bf16x6" if pieces == 3 else "scan_conv1x1_bf16x3", _p(x), xd.ref(), x.shape[1], *[_p(t) for t in planes],
              csw, _p(bias), None, _p(y), yd.ref(), nout, nout, 0, cmap, None)
    return y


@pytest.mark.parametrize("pieces", [3, 2])
def test_conv1x1_stride1(device, pieces):
    from scan_amd import ops
    g = torch.Generator().manual_seed(11)
    d = ops.PyramidShape(N, PYR)
    x, wp, bias = _rand(g, device, d.rows, 36), _rand(g, device, 72, 1, 36) / 6, _rand(g, device, 72)
    plan, y = _planned(pieces, 0, wp, x, d, bias, None, d, d.rows)
    assert (plan.family, plan.split_mode, plan.plane_taps, plan.csw) == (ONE, 0, 1, 40)
    assert torch.equal(y, _legacy1x1(pieces, 0, wp, x, d, bias, d, 0)) and float(y.abs().max()) > 0
    dy = _rand(g, device, d.rows, 72)
    plan, dx = _planned(pieces, 1, wp, dy, d, None, None, d, d.rows)
    assert (plan.family, plan.split_mode, plan.nout, plan.csw) == (ONE, 1, 36, 72)
    assert torch.equal(dx, _legacy1x1(pieces, 1, wp, dy, d, None, d, 0)) and float(dx.abs().max()) > 0


@pytest.mark.parametrize("pieces", [3, 2])
def test_conv1x1_stride2_forward_and_dgrad(device, pieces):
    """map 1: y on the coarse pyramid ceil(size / 2); map 2: dX on the fine pyramid, zero where a coordinate is odd"""
    from scan_amd import ops
    g = torch.Generator().manual_seed(12)
    fine = ops.PyramidShape(N, ODD)
    coarse = fine.conv_out(1, 2)
    assert coarse.sizes == [(7, 11), (4, 6)]
    x, wp, bias = _rand(g, device, fine.rows, 36), _rand(g, device, 72, 1, 36) / 6, _rand(g, device, 72)
    plan, y = _planned(pieces, 0, wp, x, fine, bias, None, coarse, coarse.rows, cmap=1)
    assert plan.family == ONE
    assert torch.equal(y, _legacy1x1(pieces, 0, wp, x, fine, bias, coarse, 1)) and float(y.abs().max()) > 0
    dy = _rand(g, device, coarse.rows, 72)
    plan, dx = _planned(pieces, 1, wp, dy, coarse, None, None, fine, fine.rows, cmap=2)
    assert (plan.family, plan.split_mode, plan.nout) == (ONE, 1, 36)
    assert torch.equal(dx, _legacy1x1(pieces, 1, wp, dy, coarse, None, fine, 2))
    lvl0 = dx[:N * 13 * 21].reshape(N, 13, 21, 36)
    assert float(lvl0[:, 1::2].abs().max()) == 0.0 and float(lvl0[:, :, 1::2].abs().max()) == 0.0 and float(lvl0[:, ::2, ::2].abs().max()) > 0

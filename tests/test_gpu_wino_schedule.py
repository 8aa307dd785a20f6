"""The two schedules of the Winograd F(2,3) 3x3 instance (csrc/conv_fwd.hip, scan_tune "wino_tpb"): 2 (default) = the patch
staged in component pairs, two weight taps per barrier interval; 1 = one tap per interval.  Every accumulator sees the same
products in the same order under both, so every output must agree BIT FOR BIT: forward and data gradient, bias, ReLU, the
deferred-ReLU mask, the fused 2x2 pool, odd and non-multiple-of-16 sizes, a five-level pyramid launch, Cout that does not fill
128-channel tiles (192, and the 264 -> 1024 class-branch shape), 2 / 8 / 16 K chunks (Cin 64 / 256 / 512), through ops and
through the compiled conv2d operator.  The GroupNorm sums of the epilogue leave each workgroup as one fp64 atomic pair, so
their order across workgroups is not fixed: outputs bit-equal, sums equal to 1e-12 relative (fp64 reordering of at most a few
thousand addends; far below any fp32 effect)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (levels, N, Cin, Cout)
CASES = [
    ([(37, 53)], 1, 64, 192),                 # 2 K chunks, Cout = 128 + 64
    ([(21, 45)], 2, 256, 256),                # 8 chunks, odd sizes
    ([(16, 32)], 1, 512, 512),                # 16 chunks, whole tiles
    ([(84, 167)], 1, 128, 128),               # not multiples of 16
    ([(19, 27)], 1, 264, 1024),               # class branch: ragged last chunk of the input, eight channel tiles
    ([(40, 56), (20, 28), (10, 14), (5, 7), (3, 4)], 2, 256, 256),  # five-level pyramid launch
]


def _tune(key, value):
    from scan_amd import _lib
    return _lib.query("scan_tune", key.encode(), value)


def _both(fn):
    """fn() under wino_tpb = 1 and = 2 (bf16x6, Winograd on)"""
    from scan_amd import ops
    keep = ops.CONV_MODE
    ops.CONV_MODE = "bf16x6"
    old_w = _tune("conv_wino", 1)
    res = []
    try:
        for tpb in (1, 2):
            old = _tune("wino_tpb", tpb)
            try:
                res.append(fn())
            finally:
                _tune("wino_tpb", old)
    finally:
        _tune("conv_wino", old_w)
        ops.CONV_MODE = keep
    return res


def _inputs(device, case, seed):
    from scan_amd import ops
    sizes, n, cin, cout = case
    shape = ops.PyramidShape(n, sizes)
    g = torch.Generator(device=device).manual_seed(seed)
    cs = ops.pad4(cin)
    x = torch.randn((shape.rows, cs), device=device, generator=g)
    if cs != cin:
        x[:, cin:] = 0
    w = (torch.randn((cout, cin, 3, 3), device=device, generator=g) / (cin * 9) ** 0.5).contiguous(memory_format=torch.channels_last)
    b = torch.randn((cout,), device=device, generator=g)
    return shape, x, w, b


def test_wino_tpb_defaults(device):
    from scan_amd import _lib
    assert _lib.query("scan_tune_default", b"wino_tpb") == 2
    assert _lib.query("scan_tune_get", b"wino_tpb") == 2
    assert _lib.query("scan_tune_default", b"conv_wino") == 1


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_wino_tpb_forward_bit_equal(device, case, relu):
    from scan_amd import _lib, ops
    shape, x, w, b = _inputs(device, case, seed=case[2] + case[3])
    assert _lib.query("scan_conv3x3_bf16x6_wino", case[3], ops._round32(ops.pad4(case[2]))) == 1

    def fwd():
        with torch.no_grad():
            return ops.conv2d(x, w, b if relu else None, shape, 3, 1, relu=relu).clone()
    y1, y2 = _both(fwd)
    assert float(y1.abs().max()) > 0
    assert torch.equal(y1, y2)


@pytest.mark.parametrize("mask_dx", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_wino_tpb_dgrad_bit_equal(device, case, mask_dx):
    """data gradient (the same kernel on dY with the mode-3 planes); mask_dx: x is a deferred-ReLU output and the epilogue
    applies its mask"""
    from scan_amd import ops
    shape, x, w, b = _inputs(device, case, seed=3 * case[2] + case[3])
    cout = case[3]
    if mask_dx:
        x = x.clamp_min(0)
    gy = torch.randn((shape.rows, cout), device=device, generator=torch.Generator(device=device).manual_seed(7))

    def bwd():
        xx = x.clone().requires_grad_(True)
        y = ops.conv2d(xx, w, b, shape, 3, 1, mask_dx=mask_dx)
        y[:, :cout].backward(gy)
        return xx.grad.detach().clone()
    d1, d2 = _both(bwd)
    assert float(d1.abs().max()) > 0
    assert torch.equal(d1, d2)


@pytest.mark.parametrize("case", [([(36, 52)], 2, 128, 128), ([(18, 70)], 1, 256, 192)])
def test_wino_tpb_fused_pool_bit_equal(device, case):
    from scan_amd import ops
    shape, x, w, b = _inputs(device, case, seed=5)

    def fwd():
        with torch.no_grad():
            return ops.conv2d(x, w, b, shape, 3, 1, relu=True, pool=True).clone()
    y1, y2 = _both(fwd)
    h, w_ = case[0][0]
    assert y1.shape[0] == case[1] * (h // 2) * (w_ // 2) and float(y1.abs().max()) > 0
    assert torch.equal(y1, y2)


def test_wino_tpb_groupnorm_sums(device):
    from scan_amd import ops
    case = ([(37, 53), (19, 27), (9, 13)], 2, 256, 256)
    shape, x, w, b = _inputs(device, case, seed=11)

    def fwd():
        with torch.no_grad():
            y = ops.conv2d(x, w, b, shape, 3, 1, gn_sums=True)
            sums = ops._gn_sums.get(y.data_ptr())
            assert sums is not None
            return y.clone(), sums.clone()
    (y1, s1), (y2, s2) = _both(fwd)
    assert torch.equal(y1, y2)
    n = shape.n_levels * shape.n_images * 32 * 2
    a, c = s1.reshape(-1)[:n].double(), s2.reshape(-1)[:n].double()
    rel = float(((a - c).abs() / a.abs().clamp_min(1e-300)).max())
    print("GroupNorm sums, worst relative difference between the schedules: %.3e" % rel)
    assert float(a.abs().min()) > 0
    assert rel <= 1e-12


def test_wino_tpb_compiled_operator_bit_equal(device):
    """the drop-in conv2d operator (csrc/scan_ops_ext.cpp) launches through the same library entry and follows the knob:
    forward and input gradient bit-equal between the schedules, and equal to the ops path"""
    from scan_amd import layers as L
    from scan_amd import ops
    assert L.OPS_BACKEND == "compiled"
    torch.manual_seed(3)
    for cin, cout, hw in [(256, 256, (21, 45)), (64, 192, (19, 37))]:
        x = torch.randn(2, cin, *hw)
        w = torch.randn(cout, cin, 3, 3) * (2.0 / (cin * 9)) ** 0.5
        b = torch.randn(cout) * 0.1
        gy = torch.randn(2, cout, *hw).to(device)

        def run(path):
            xx = x.to(device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
            ww = w.to(device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
            bb = b.to(device).requires_grad_(True)
            if path == "cpp":
                y = L._ops.conv2d(xx, ww, bb, 1, False)
            else:
                rows, shape, _ = L._to_rows(xx)
                y = L._to_nchw(ops.conv2d(rows, ww, bb, shape, 3, 1, relu=False), shape.conv_out(3, 1), cout)
            y.backward(gy)
            return y.detach().clone(), xx.grad.detach().clone()
        (y1, g1), (y2, g2) = _both(lambda: run("cpp"))
        assert torch.equal(y1, y2) and torch.equal(g1, g2), (cin, cout)
        (yp, gp), _ = _both(lambda: run("py"))
        assert torch.equal(y1, yp) and torch.equal(g1, gp), (cin, cout)

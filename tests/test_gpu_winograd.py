"""The Winograd F(2,3) instance of the three-piece 3x3 convs (scan_tune "conv_wino" = 1, csrc/conv_fwd.hip WINO) against
an fp64 convolution, next to the direct kernels (conv_wino = 0) and the exact fp32-MFMA kernels: forward and data gradient,
odd widths (the last output pair straddles the right edge), ragged input and output channel counts, every epilogue the
instance serves (bias, ReLU, the ReLU mask of a data gradient, GroupNorm sums), sparse post-ReLU and large-dynamic-range
inputs.  Bars as tests/test_gpu_kernels.py::test_conv_error_vs_fp64: worst <= 5e-6 of the largest output, rms <= 1.1x and
worst <= 1.5x those of the fp32-MFMA kernel."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (levels, N, Cin, Cout)
CASES = [
    ([(9, 13)], 2, 256, 256),
    ([(37, 53)], 1, 268, 200),             # ragged K chunk, ragged output-channel tile
    ([(84, 167)], 1, 128, 128),
    ([(37, 53), (19, 27), (9, 13)], 2, 256, 256),
]


def _tune(key, value):
    from scan_amd import _lib
    return _lib.query("scan_tune", key.encode(), value)


def _to_nchw(rows, shape, l, c):
    h, w = shape.sizes[l]
    return rows[shape.row_off[l]:shape.row_off[l + 1], :c].reshape(shape.n_images, h, w, c).permute(0, 3, 1, 2)


def _conv64(x_rows, shape, w, c_in):
    """fp64 3x3 / pad-1 conv of every level: rows [M, Cout] fp64 on the host"""
    w64 = w.detach().cpu().double()
    out = []
    for l in range(shape.n_levels):
        xl = _to_nchw(x_rows.detach().cpu().double(), shape, l, c_in)
        out.append(F.conv2d(xl, w64, padding=1).permute(0, 2, 3, 1).reshape(-1, w64.shape[0]))
    return torch.cat(out, 0)


def _errs(y, ref):
    scale = float(ref.abs().max())
    d = (y.detach().cpu().double() - ref).abs() / scale
    return float(d.max()), float((d ** 2).mean()) ** 0.5


def _check(outs, ref):
    e = {m: _errs(y, ref) for m, y in outs.items()}
    print("worst / rms vs fp64", e)
    assert e["wino"][0] <= 5e-6, e
    assert e["wino"][1] <= 1.1 * e["fp32"][1], e
    assert e["wino"][0] <= 1.5 * e["fp32"][0], e


def _run(mode, wino, fn):
    from scan_amd import ops
    keep = ops.CONV_MODE
    ops.CONV_MODE = mode
    old = _tune("conv_wino", wino)
    try:
        return fn()
    finally:
        _tune("conv_wino", old)
        ops.CONV_MODE = keep


def _inputs(device, case, kind, seed):
    from scan_amd import ops
    sizes, n, cin, cout = case
    shape = ops.PyramidShape(n, sizes)
    g = torch.Generator(device=device).manual_seed(seed)
    cs = ops.pad4(cin)
    x = torch.randn((shape.rows, cs), device=device, generator=g)
    if kind == "relu":        # post-ReLU: half the inputs exactly zero
        x = x.clamp_min(0)
    elif kind == "range":     # values over 2^-20 .. 2^20
        x = x * torch.exp2(torch.randint(-20, 21, x.shape, device=device, generator=g).float())
    if cs != cin:
        x[:, cin:] = 0
    w = (torch.randn((cout, cin, 3, 3), device=device, generator=g) / (cin * 9) ** 0.5).contiguous(memory_format=torch.channels_last)
    b = torch.randn((cout,), device=device, generator=g)
    return shape, x, w, b


def test_wino_is_default_and_eligible(device):
    from scan_amd import _lib
    assert _lib.query("scan_tune_default", b"conv_wino") == 1
    assert _lib.query("scan_conv3x3_bf16x6_wino", 256, 256) == 1
    assert _lib.query("scan_conv3x3_bf16x6_wino", 64, 256) == 0   # the 64-channel instances stay direct
    old = _tune("conv_wino", 0)
    try:
        assert _lib.query("scan_conv3x3_bf16x6_wino", 256, 256) == 0
    finally:
        _tune("conv_wino", old)


@pytest.mark.parametrize("kind", ["randn", "relu", "range"])
@pytest.mark.parametrize("case", CASES)
def test_wino_forward_vs_fp64(device, case, kind):
    """forward with bias (and ReLU for the sparse input): wino against fp64, beside the direct kernel and fp32-MFMA"""
    from scan_amd import ops
    shape, x, w, b = _inputs(device, case, kind, seed=case[2] + case[3] + len(kind))
    cout = case[3]
    relu = kind == "relu"

    def fwd():
        with torch.no_grad():
            return ops.conv2d(x, w, b, shape, 3, 1, relu=relu)[:, :cout]
    outs = {"wino": _run("bf16x6", 1, fwd), "direct": _run("bf16x6", 0, fwd), "fp32": _run("fp32", 1, fwd)}
    ref = _conv64(x, shape, w, case[2]) + b.cpu().double()
    if relu:
        ref = ref.clamp_min(0)
    _check(outs, ref)
    # the level alone equals its rows of the pyramid launch bit for bit
    if shape.n_levels > 1:
        l = shape.n_levels - 1
        xl = x[shape.row_off[l]:shape.row_off[l + 1]].contiguous()

        def lvl():
            with torch.no_grad():
                return ops.conv2d(xl, w, b, shape.level(l), 3, 1, relu=relu)[:, :cout]
        assert torch.equal(_run("bf16x6", 1, lvl), outs["wino"][shape.row_off[l]:shape.row_off[l + 1]])


@pytest.mark.parametrize("kind", ["randn", "relu"])
@pytest.mark.parametrize("case", CASES)
def test_wino_dgrad_vs_fp64(device, case, kind):
    """data gradient (the forward kernel on dY with the mode-3 planes); kind "relu": x is a deferred-ReLU output, the
    epilogue applies the ReLU mask"""
    from scan_amd import ops
    shape, x, w, b = _inputs(device, case, kind, seed=3 * case[2] + case[3] + len(kind))
    cin, cout = case[2], case[3]
    gy = torch.randn((shape.rows, cout), device=device, generator=torch.Generator(device=device).manual_seed(7))
    mask_dx = kind == "relu"

    def bwd():
        xx = x.clone().requires_grad_(True)
        y = ops.conv2d(xx, w, b, shape, 3, 1, mask_dx=mask_dx)
        y[:, :cout].backward(gy)
        return xx.grad[:, :cin].detach()
    outs = {"wino": _run("bf16x6", 1, bwd), "direct": _run("bf16x6", 0, bwd), "fp32": _run("fp32", 1, bwd)}
    wt = w.detach().flip(2, 3).transpose(0, 1).contiguous()
    ref = _conv64(gy, shape, wt, cout)
    if mask_dx:
        ref = ref * (x[:, :cin].cpu() > 0).double()
    _check(outs, ref)


@pytest.mark.parametrize("O,Cs", [(256, 256), (200, 268), (1024, 264)])
def test_wino_planes_batched_equal_single_launches(device, O, Cs):
    """split modes 2 / 3 through scan_weight_split_batched (one launch per training iteration) equal the per-weight
    scan_weight_split3 planes bit for bit, and mode 2 equals G applied to the fp32 weights in fp64, rounded once"""
    from scan_amd import _lib, ops
    g = torch.Generator(device=device).manual_seed(O + Cs)
    wp = torch.randn((O, 9, Cs), device=device, generator=g)
    rows_off, jobs, single, batched = 0, [], [], []
    for mode in (2, 3):
        rows = O if mode == 2 else Cs
        csw = ops._round32(Cs if mode == 2 else O)
        one = [torch.empty((rows, 12, csw), dtype=torch.bfloat16, device=device) for _ in range(3)]
        ops.call("scan_weight_split3", ops._ptr(wp), O, 9, Cs, mode, *[ops._ptr(t) for t in one], csw, ops._stream())
        many = [torch.full((rows, 12, csw), 7.0, dtype=torch.bfloat16, device=device) for _ in range(3)]
        jobs.append([wp.data_ptr(), many[0].data_ptr(), many[1].data_ptr(), O, 9, Cs, mode, rows, csw, rows_off, many[2].data_ptr()])
        rows_off += ops.query("scan_weight_split_job_blocks", O, 9, Cs, mode, csw)
        single.append(one)
        batched.append(many)
    table = torch.tensor(jobs, dtype=torch.int64).to(device)
    ops.call("scan_weight_split_batched", ops._ptr(table), len(jobs), _lib.SPLIT_JOB_WORDS, rows_off, ops._stream())
    for one, many in zip(single, batched):
        for a, b in zip(one, many):
            assert torch.equal(a, b)
    # mode 2 against the transform on the host
    G = torch.tensor([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=torch.float64)
    ref = torch.einsum("jk,oykc->ojyc", G, wp.cpu().double().view(O, 3, 3, Cs)).reshape(O, 12, Cs).float()
    got = sum(p.float() for p in reversed(single[0])).cpu()[:, :, :Cs]
    assert torch.equal(got, ref)


def test_wino_groupnorm_sums(device):
    """the GroupNorm-sum epilogue: the per-(level, image, group) sums equal fp64 sums over the kernel's own output, and
    the output matches the direct kernel's at rounding scale"""
    from scan_amd import ops
    case = ([(37, 53), (19, 27)], 2, 256, 256)
    shape, x, w, b = _inputs(device, case, "randn", seed=11)

    def fwd():
        with torch.no_grad():
            y = ops.conv2d(x, w, b, shape, 3, 1, gn_sums=True)
            sums = ops._gn_sums.get(y.data_ptr())
            return y, (sums.clone() if sums is not None else None)
    (y1, s1), (y0, s0) = _run("bf16x6", 1, fwd), _run("bf16x6", 0, fwd)
    assert s1 is not None and s0 is not None
    assert float((y1 - y0).abs().max()) <= 5e-6 * float(y0.abs().max())
    yd = y1.double()
    exp = []
    for l in range(shape.n_levels):
        yl = yd[shape.row_off[l]:shape.row_off[l + 1]].reshape(shape.n_images, -1, 32, 8)
        exp.append(torch.stack([yl.sum((1, 3)), (yl * yl).sum((1, 3))], -1))
    exp = torch.stack(exp, 0).reshape(-1)
    got = s1.reshape(-1)[:exp.numel()]
    assert torch.allclose(got, exp, rtol=1e-9, atol=1e-9 * float(exp.abs().max())), float((got - exp).abs().max())

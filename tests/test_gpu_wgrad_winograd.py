"""The Winograd F(2,3)-across-rows instance of the three-piece 3x3 weight gradient (scan_tune "wgrad_wino" = 1,
csrc/conv_wgrad.hip WINO + slab_bias_reduce_wino_kernel) through the C ABI: against an fp64 weight gradient on sampled
elements (worst <= 5e-6 of the largest, the bar of test_gpu_kernels.py::test_wgrad_full_size_elementwise part (b)), against
the direct path (wgrad_wino = 0) element by element (<= 1e-5 of the largest, that test's part (a)), the bias gradient against
fp64 column sums (<= 5e-6).  Shapes: heights 1 and 3 and other odd heights (the last pair of an image has no second row),
widths that are no multiple of the 32-pixel chunk, pyramids whose levels have odd heights, several images (a pair never
straddles two), ragged channel counts including 264 -> 1024 and an output count that is no multiple of 4 (Cout_s > Cout, the
padding columns of dY hold junk).  accumulate = 1, bias on and off, and the compiled operator against the Python path bit for
bit.

wgrad_wino = 0 must give the direct kernel's gradients bit for bit: tests/golden/wgrad_direct_parent.npz holds dW and db of three
small shapes computed by the build before the Winograd form existed, on inputs drawn from a seeded CPU generator
(test_wgrad_wino_off_reproduces_the_direct_build); the knob's workspace contract, run-to-run bits and the compiled operator are
pinned beside it."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_direct_parent.npz")

# (levels, N, Cin, Cout)
CASES = [
    ([(1, 40)], 2, 256, 256),                                          # H = 1: every pair is a single row
    ([(3, 33)], 3, 256, 256),                                          # H = 3, one pixel into the second chunk
    ([(37, 53), (19, 27), (9, 13)], 2, 256, 256),                      # odd heights on every level
    ([(16, 32), (8, 16), (4, 8), (2, 4), (1, 2)], 2, 264, 1024),       # class branches; levels down to H = 1
    ([(21, 45)], 2, 268, 200),                                         # ragged input and output channel tiles
    ([(12, 70)], 3, 130, 5),                                           # Cout_s = 8 > Cout = 5
    ([(64, 128), (32, 64)], 4, 256, 256),                              # chains of a few hundred chunks per split
]


# (levels, N, Cin, Cout, post-ReLU x) of the recorded direct-path gradients: odd heights over two levels, H = 3 with Cout_s > Cout,
# and two input-channel tiles with 64 split-K slabs
PARENT_CASES = [
    ([(37, 53), (19, 27)], 2, 40, 32, True),
    ([(3, 33)], 3, 130, 5, False),
    ([(64, 128)], 2, 136, 24, True),
]


def parent_case_inputs(i, device):
    """inputs of PARENT_CASES[i] from a seeded CPU generator (the same values on every machine)"""
    from scan_amd import ops
    sizes, n, cin, cout, relu = PARENT_CASES[i]
    shape = ops.PyramidShape(n, sizes)
    g = torch.Generator().manual_seed(1000 + i)
    cs, ns = ops.pad4(cin), ops.pad4(cout)
    x = torch.randn((shape.rows, cs), generator=g)
    if relu:
        x = x.clamp_min(0)
    x[:, cin:] = 0
    gy = torch.randn((shape.rows, ns), generator=g)
    return shape, x.to(device), gy.to(device), cs, ns


def _tune(key, value):
    from scan_amd import _lib
    return _lib.query("scan_tune", key.encode(), value)


def _inputs(device, case, seed):
    from scan_amd import ops
    sizes, n, cin, cout = case
    shape = ops.PyramidShape(n, sizes)
    g = torch.Generator(device=device).manual_seed(seed)
    cs, ns = ops.pad4(cin), ops.pad4(cout)
    x = torch.randn((shape.rows, cs), device=device, generator=g)
    if cs != cin:
        x[:, cin:] = 0
    gy = torch.randn((shape.rows, ns), device=device, generator=g)  # columns cout.. are junk the kernel must not use
    return shape, x, gy, cs, ns


def _wgrad(shape, x, gy, cs, cout, ns, wino, bias=True, into=None):
    """scan_conv3x3_wgrad_bf16x6 under wgrad_wino = wino; into = (dw, db): accumulate into copies of them"""
    from scan_amd import _lib, ops
    old = _tune("wgrad_wino", wino)
    try:
        ws = torch.empty((_lib.query("scan_conv3x3_wgrad_bf16x6_ws_floats", shape.ref(), cs, cout),), device=x.device)
        dw = into[0].clone() if into else torch.full((cout, 9, cs), float("nan"), device=x.device)
        db = (into[1].clone() if into else torch.full((cout,), float("nan"), device=x.device)) if bias else None
        _lib.call("scan_conv3x3_wgrad_bf16x6", ops._ptr(x), shape.ref(), cs, ops._ptr(gy), cout, ns, ops._ptr(dw),
                  ops._ptr(db) if bias else None, int(into is not None), ops._ptr(ws), ops._stream())
        torch.cuda.synchronize()
        return dw, db
    finally:
        _tune("wgrad_wino", old)


def _ref64(shape, x, gy, cin, cout, seed):
    """fp64 weight gradient of up to 16 x 16 sampled (o, c) on the device: [o, ky, kx, c], and the indices"""
    rs = np.random.RandomState(seed)
    oi = torch.from_numpy(rs.choice(cout, min(16, cout), replace=False)).to(x.device)
    ci = torch.from_numpy(rs.choice(cin, 16, replace=False)).to(x.device)
    ref = torch.zeros((len(oi), 3, 3, 16), dtype=torch.float64, device=x.device)
    n = shape.n_images
    for l, (h, w) in enumerate(shape.sizes):
        r0, r1 = shape.row_off[l], shape.row_off[l + 1]
        xs = x[r0:r1][:, ci].double().view(n, h, w, 16)
        gs = gy[r0:r1][:, oi].double().view(n, h, w, len(oi))
        xp = torch.zeros((n, h + 2, w + 2, 16), dtype=torch.float64, device=x.device)
        xp[:, 1:-1, 1:-1] = xs
        for ky in range(3):
            for kx in range(3):
                ref[:, ky, kx] += torch.einsum("nyxo,nyxc->oc", gs, xp[:, ky:ky + h, kx:kx + w])
    return ref, oi, ci


def test_wgrad_wino_is_default_and_sizes_its_workspace(device):
    from scan_amd import _lib, ops
    assert _lib.query("scan_tune_default", b"wgrad_wino") == 1
    shape = ops.PyramidShape(4, [(256, 512)])  # conv3_x: 16,384 row chunks -> 64 slabs of 9 taps; 8,192 pair chunks -> 48 of 12
    sizes = {}
    for wino in (0, 1):
        old = _tune("wgrad_wino", wino)
        try:
            sizes[wino] = _lib.query("scan_conv3x3_wgrad_bf16x6_ws_floats", shape.ref(), 256, 256)
            two = _lib.query("scan_conv3x3_wgrad_bf16x3_ws_floats", shape.ref(), 256, 256)
        finally:
            _tune("wgrad_wino", old)
        sizes["bf16x3", wino] = two
    assert sizes[0] == 64 * 256 * 9 * 256 + 64 * 256
    assert sizes[1] == 48 * 256 * 12 * 256 + 48 * 256
    assert sizes["bf16x3", 0] == sizes["bf16x3", 1]  # two pieces stay direct
    # wgrad_v6 = 0 and wgrad_tile = 0 keep their direct kernels whatever wgrad_wino says
    for key in ("wgrad_v6", "wgrad_tile"):
        old = _tune(key, 0)
        try:
            a = _lib.query("scan_conv3x3_wgrad_bf16x6_ws_floats", shape.ref(), 256, 256)
            o2 = _tune("wgrad_wino", 0)
            b = _lib.query("scan_conv3x3_wgrad_bf16x6_ws_floats", shape.ref(), 256, 256)
            _tune("wgrad_wino", o2)
        finally:
            _tune(key, old)
        assert a == b, key


@pytest.mark.parametrize("i", range(len(PARENT_CASES)))
def test_wgrad_wino_off_reproduces_the_direct_build(device, i):
    shape, x, gy, cs, ns = parent_case_inputs(i, device)
    cout = PARENT_CASES[i][3]
    dw, db = _wgrad(shape, x, gy, cs, cout, ns, 0)
    gold = np.load(GOLDEN)
    assert torch.equal(dw.cpu(), torch.from_numpy(gold["dw_%d" % i])), float((dw.cpu() - torch.from_numpy(gold["dw_%d" % i])).abs().max())
    assert torch.equal(db.cpu(), torch.from_numpy(gold["db_%d" % i]))
    # and the Winograd form on the same inputs sits within the element bar of it
    dw1, _ = _wgrad(shape, x, gy, cs, cout, ns, 1)
    assert float((dw1 - dw).abs().max()) <= 1e-5 * float(dw.abs().max())


@pytest.mark.parametrize("case", CASES)
def test_wgrad_wino_vs_fp64_and_direct(device, case):
    sizes, n, cin, cout = case
    shape, x, gy, cs, ns = _inputs(device, case, seed=cin + 3 * cout + len(sizes))
    dw1, db1 = _wgrad(shape, x, gy, cs, cout, ns, 1)
    dw0, db0 = _wgrad(shape, x, gy, cs, cout, ns, 0)
    assert bool(torch.isfinite(dw1).all()) and bool(torch.isfinite(db1).all())  # every element written (outputs start as NaN)
    if cs != cin:
        assert float(dw1[:, :, cin:].abs().max()) == 0.0
    scale = float(dw0.abs().max())
    d01 = float((dw1 - dw0).abs().max())
    ref, oi, ci = _ref64(shape, x, gy, cin, cout, seed=cin)
    rmax = float(ref.abs().max())

    def err(dw):
        d = (dw.view(cout, 3, 3, cs).double()[oi][:, :, :, ci] - ref).abs() / rmax
        return float(d.max()), float((d ** 2).mean() ** 0.5)
    e1, e0 = err(dw1), err(dw0)
    bref = gy[:, :cout].double().sum(0)
    eb1 = float((db1.double() - bref).abs().max()) / float(bref.abs().max())
    print("wgrad wino vs fp64 (max, rms)", case, e1, "direct", e0, "| wino - direct: %.3e of the largest | bias %.3e" % (d01 / scale, eb1))
    assert e1[0] <= 5e-6, (e1, e0)
    # rms against the direct form's: the Winograd operands carry one fp32 rounding each that direct operands do not, which
    # is the larger share of the error the shorter the chain.  The host emulation (tools/wino_numerics.py emulate_wgrad) puts the
    # ratio at 2.02 on 64-pixel chains, 1.44 at 256, 1.10 at 1,024 and 0.94-1.11 at the bench's 5,461: 2.1x bounds every case here
    assert e1[1] <= 2.1 * e0[1], (e1, e0)
    assert d01 <= 1e-5 * scale, (d01, scale)
    assert eb1 <= 5e-6, eb1
    assert float((db1 - db0).abs().max()) <= 5e-6 * float(bref.abs().max())


@pytest.mark.parametrize("wino", [1, 0])
def test_wgrad_wino_accumulate_bias_off_and_rerun(device, wino):
    case = ([(37, 53), (19, 27)], 2, 268, 200)
    sizes, n, cin, cout = case
    shape, x, gy, cs, ns = _inputs(device, case, seed=5)
    dw, db = _wgrad(shape, x, gy, cs, cout, ns, wino)
    dw_again, db_again = _wgrad(shape, x, gy, cs, cout, ns, wino)
    assert torch.equal(dw, dw_again) and torch.equal(db, db_again)      # fixed order: the same bits from run to run
    dw_nb, none = _wgrad(shape, x, gy, cs, cout, ns, wino, bias=False)
    assert none is None and torch.equal(dw, dw_nb)                      # the bias ride-along does not touch dW
    g = torch.Generator(device=device).manual_seed(9)
    dw_init = torch.randn((cout, 9, cs), device=device, generator=g)
    db_init = torch.randn((cout,), device=device, generator=g)
    dw_acc, db_acc = _wgrad(shape, x, gy, cs, cout, ns, wino, into=(dw_init, db_init))
    assert torch.equal(dw_acc, dw + dw_init) and torch.equal(db_acc, db + db_init)


@pytest.mark.parametrize("wino", [1, 0])
def test_wgrad_wino_compiled_operator_equals_python_path(device, wino):
    """the drop-in operator (csrc/scan_ops_ext.cpp) sizes its workspace through the library and lands on the same kernel:
    same bits as the Python autograd path, odd height and width, Cout_s > Cout"""
    from scan_amd import layers as L
    from scan_amd import ops
    assert L.OPS_BACKEND == "compiled"
    torch.manual_seed(3)
    old = _tune("wgrad_wino", wino)
    try:
        for cin, cout, hw in [(256, 256, (21, 45)), (264, 6, (9, 37))]:
            x = torch.randn(2, cin, *hw)
            w = torch.randn(cout, cin, 3, 3) * (2.0 / (cin * 9)) ** 0.5
            b = torch.randn(cout) * 0.1
            gy = torch.randn(2, cout, *hw).to(device)
            res = []
            for path in ("cpp", "py"):
                xx = x.to(device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
                ww = w.to(device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
                bb = b.to(device).requires_grad_(True)
                if path == "cpp":
                    y = L._ops.conv2d(xx, ww, bb, 1, False)
                else:
                    rows, shape, _ = L._to_rows(xx)
                    y = L._to_nchw(ops.conv2d(rows, ww, bb, shape, 3, 1, relu=False), shape.conv_out(3, 1), cout)
                y.backward(gy)
                res.append((ww.grad.clone(), bb.grad.clone()))
            assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), (cin, cout, wino)
    finally:
        _tune("wgrad_wino", old)

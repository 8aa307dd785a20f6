"""GPU tests of the HBM-bound kernels of scan_amd/csrc/pointwise.hip, of scan_sgd_momentum_multi (batched.hip) and of
scan_relu_backward against the references of tests/pointwise_ref.py (pinned on the CPU by tests/test_pointwise_host.py): past
the grid cap of 2048 blocks x 256 threads = 524 288 work items (a float4 each for the vector kernels), where the grid-stride
loops take their second trip; at the smallest legal shapes and the n & 3 tails; on pointers that are 4-byte but not 16-byte
aligned; and on the inputs only some data reaches (pooling ties, all-negative maps, fresh prototypes).

Bars.  scale, add + ReLU, the ReLU backward, both pools, the FPN join and its backward, the take_images gradient and the column
copy are exact in fp32: torch.equal against the fp32 reference (alpha = +-0 on the bits).  SGD: rtol 1e-6 / atol 1e-7 against
float64 after three steps, the bar of test_sgd_kernel.  Paradigm update: rtol 2e-6 / atol 2e-6 against float64, the bar of
test_round6_glue_kernels_equal_their_torch_spellings -- the fp32 torch spelling of the update is within 0.06 of that bar on every
input used here (test_pointwise_host.py asserts <= 0.5), so no case needs a bar of its own.

Every output a test allocates itself is a view into a larger buffer of SENTINEL with a margin in front and behind, handed to
the library by _lib.call; the margins are checked after the call.  Where ops.* reaches the kernel, the values are checked that
way too.  Shapes are the smallest that reach the named path; the largest tensor is 37.7 MB."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import pointwise_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
MARGIN = 64                 # floats: a multiple of 4, so a view behind it is as aligned as the allocation
CAP = 2048 * 256            # work items of one trip of a grid-stride loop (grid_for in csrc/common.h)


# ----------------------------------------------------------------------------- plumbing
class Guarded:
    """n floats inside a buffer of SENTINEL, MARGIN (+ lead) floats in front and MARGIN behind; lead = 1..3: not 16-byte aligned"""

    def __init__(self, n, device, lead=0, init=None):
        self.lo, self.n = MARGIN + lead, int(n)
        self.buf = torch.full((self.lo + self.n + MARGIN,), SENTINEL, dtype=torch.float32, device=device)
        self.v = self.buf[self.lo:self.lo + self.n]
        assert self.v.data_ptr() % 16 == 4 * (lead % 4)
        if init is not None:
            self.v.copy_(torch.as_tensor(init).reshape(-1))

    def intact(self):
        return bool((self.buf[:self.lo] == SENTINEL).all()) and bool((self.buf[self.lo + self.n:] == SENTINEL).all())

    def untouched(self):
        return bool((self.buf == SENTINEL).all())


def _dev(a, device, lead=0):
    """a contiguous device copy of a numpy array, `lead` floats off 16-byte alignment"""
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a)
    if lead == 0:
        v = t.to(device)
        assert v.numel() == 0 or v.data_ptr() % 16 == 0
        return v
    return Guarded(a.size, device, lead, t).v.view(a.shape)


def _eq(t, ref):
    """value equality of a device tensor and a numpy reference, shape apart"""
    return torch.equal(t.detach().cpu().reshape(-1), torch.from_numpy(np.ascontiguousarray(ref)).reshape(-1))


def _bits(t, ref):
    return torch.equal(t.detach().cpu().reshape(-1).view(torch.int32), torch.from_numpy(np.ascontiguousarray(ref)).reshape(-1).view(torch.int32))


def _lib_ops():
    from scan_amd import _lib, ops
    return _lib, ops, ops._ptr, ops._stream()


@functools.lru_cache(maxsize=None)
def _randn(seed, *shape):
    return np.random.RandomState(seed).standard_normal(shape).astype(np.float32)


# ============================================================================= 1. scale, add + ReLU, ReLU backward
def _flat_case(device, n, alpha, leads=(0, 0, 0)):
    """scan_scale (out of place and in place), scan_add_relu and scan_relu_backward on n floats into guarded outputs; leads = the
    misalignment in floats of (first input, second input, output)"""
    _lib, ops, P, st = _lib_ops()
    a, b, dy = _randn(11, n), _randn(12, n), _randn(13, n)
    b = b.copy()
    b[::5] = -a[::5]  # sums of exactly zero: the ReLU's boundary
    ad, bd, dyd = _dev(a, device, leads[0]), _dev(b, device, leads[1]), _dev(dy, device, leads[0])
    y = Guarded(n, device, leads[2])
    _lib.call("scan_scale", P(ad), alpha, P(y.v), n, st)
    assert _bits(y.v, R.scale(a, alpha)) and y.intact(), ("scale", n, alpha, leads)
    z = Guarded(n, device, leads[2], a)
    _lib.call("scan_scale", P(z.v), alpha, P(z.v), n, st)  # x == y, as the weight-plane cache test uses it
    assert _bits(z.v, R.scale(a, alpha)) and z.intact(), ("scale in place", n, alpha, leads)
    s = Guarded(n, device, leads[2])
    _lib.call("scan_add_relu", P(ad), P(bd), P(s.v), n, st)
    ref = R.add_relu(a, b)
    assert _eq(s.v, ref) and s.intact(), ("add_relu", n, leads)
    r = Guarded(n, device, leads[2])
    _lib.call("scan_relu_backward", P(dyd), P(bd if leads[1] else _dev(ref, device)), P(r.v), n, st)
    assert _eq(r.v, R.relu_backward(dy, b if leads[1] else ref)) and r.intact(), ("relu_backward", n, leads)


@pytest.mark.parametrize("r", [0, 1, 2, 3])
def test_flat_kernels_past_the_grid_cap(device, r):
    """n = 4 * 524 288 + 4 * 300 + r: 300 float4s on the second trip and an n & 3 tail of r; through ops.grad_reverse and
    ops.add_relu (values and both gradients) and into guarded buffers"""
    _lib, ops, P, st = _lib_ops()
    n = 4 * CAP + 4 * 300 + r
    _flat_case(device, n, -0.02)
    a, b, dy = _randn(11, n), _randn(12, n), _randn(13, n)
    xd = _dev(a, device).requires_grad_(True)
    y = ops.grad_reverse(xd, 0.02)
    assert _eq(y, a)
    y.backward(_dev(dy, device))
    assert _bits(xd.grad, R.scale(dy, -0.02))
    ad, bd = _dev(a, device).requires_grad_(True), _dev(b, device).requires_grad_(True)
    s = ops.add_relu(ad, bd)
    ref = R.add_relu(a, b)
    assert _eq(s, ref)
    s.backward(_dev(dy, device))
    assert _eq(ad.grad, R.relu_backward(dy, ref)) and _eq(bd.grad, R.relu_backward(dy, ref))


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 1023])
@pytest.mark.parametrize("alpha", [0.5, 0.0, -0.0])
def test_flat_kernels_smallest_sizes_and_tails(device, n, alpha):
    """n < 4: the tail alone; 4, 5, 7, 1023: float4s plus every tail length.  alpha = 0 and -0.0: signed zeros, compared on bits"""
    _flat_case(device, n, alpha)


@pytest.mark.parametrize("n", [1, 6, 1023, CAP + 1001])
@pytest.mark.parametrize("leads", [(1, 0, 0), (0, 0, 3), (1, 1, 1), (3, 1, 2), (0, 3, 0)])
def test_flat_kernels_on_pointers_off_16_byte_alignment(device, n, leads):
    """a flat buffer entered one and three floats late, on the input side, the output side and both: the launchers take the
    one-float-per-lane kernels (n = 524 288 + 1001: their second trip), bit-identical to the float4 ones"""
    _flat_case(device, n, -0.1, leads)


def test_grl_on_a_nine_column_pyramid(device):
    """ops.split_levels_grl and ops.grad_reverse on [M, 9] rows of the pyramid [(5, 7), (3, 3), (2, 1)], N = 1: level 1 starts
    35 * 9 floats into the gradient matrix, 4-byte but not 16-byte aligned.  Bit-exact against -lam * g."""
    _lib, ops, P, st = _lib_ops()
    shape = ops.PyramidShape(1, [(5, 7), (3, 3), (2, 1)])
    assert (shape.row_off[1] * 9) % 4 != 0
    lams = [0.02, 0.1, 0.5]
    x = _randn(21, shape.rows, 9)
    ups = [_randn(22 + l, shape.row_off[l + 1] - shape.row_off[l], 9) for l in range(3)]
    xd = _dev(x, device).requires_grad_(True)
    parts = ops.split_levels_grl(xd, shape, lams)
    for l, p in enumerate(parts):
        assert _eq(p, x[shape.row_off[l]:shape.row_off[l + 1]])
    torch.autograd.backward(list(parts), [_dev(u, device) for u in ups])
    assert _bits(xd.grad, np.concatenate([R.scale(u, -lam) for u, lam in zip(ups, lams)], 0))
    # the gradient matrix itself guarded: every level scaled straight into its row range, as _SplitLevelsGRL.backward does
    out = Guarded(shape.rows * 9, device)
    for l, (u, lam) in enumerate(zip(ups, lams)):
        part = out.v[shape.row_off[l] * 9:shape.row_off[l + 1] * 9]
        _lib.call("scan_scale", P(_dev(u, device)), -lam, P(part), u.size, st)
    assert _bits(out.v, np.concatenate([R.scale(u, -lam) for u, lam in zip(ups, lams)], 0)) and out.intact()
    # grad_reverse behind a level view, and with an upstream gradient that is itself such a view
    for lead in (1, 3):
        xd = _dev(x, device).requires_grad_(True)
        lvl = xd[shape.row_off[1]:shape.row_off[2]]
        ops.grad_reverse(lvl, 0.1).backward(_dev(ups[1], device, lead))
        ref = np.zeros_like(x)
        ref[shape.row_off[1]:shape.row_off[2]] = R.scale(ups[1], -0.1)
        assert _bits(xd.grad, ref), lead


def test_add_relu_on_views_off_16_byte_alignment(device):
    """ops.add_relu on row ranges of [M, 9] matrices and an upstream gradient entered late: values and both gradients"""
    _lib, ops, P, st = _lib_ops()
    a, b, dy = _randn(31, 46, 9), _randn(32, 46, 9), _randn(33, 9, 9)
    ref = R.add_relu(a[35:44], b[35:44])
    for lead in (1, 3):
        ad, bd = _dev(a, device).requires_grad_(True), _dev(b, device, lead).requires_grad_(True)
        y = ops.add_relu(ad[35:44], bd[35:44])
        assert _eq(y, ref)
        y.backward(_dev(dy, device, lead))
        want = np.zeros_like(a)
        want[35:44] = R.relu_backward(dy, ref)
        assert _eq(ad.grad, want) and _eq(bd.grad, want), lead


# ============================================================================= 2. SGD
SGD_RTOL, SGD_ATOL = 1e-6, 1e-7


@pytest.mark.parametrize("n", [1, CAP + 1001])
@pytest.mark.parametrize("wd,momentum", [(1e-4, 0.9), (0.0, 0.9), (5e-4, 0.0)])
def test_sgd_three_steps_against_float64(device, n, wd, momentum):
    """scan_sgd_momentum through ops.sgd_momentum_ on guarded p and buf (n = 524 288 + 1001: a second trip of 1001), three steps
    against the float64 recurrence; buf holds NaN before the first step, which must not read it"""
    _lib, ops, P, st = _lib_ops()
    lr = float(np.float32(0.01))
    wd, momentum = float(np.float32(wd)), float(np.float32(momentum))
    p0, g = _randn(41, n), _randn(42, n)
    p, buf = Guarded(n, device, 0, p0), Guarded(n, device, 0, np.full(n, np.nan, np.float32))
    rp, rb = p0.astype(np.float64), None
    for it in range(3):
        gi = (g * np.float32(it + 1)).astype(np.float32)
        ops.sgd_momentum_(p.v, _dev(gi, device), buf.v, lr, wd, momentum, it == 0)
        rp, rb = R.sgd_step(rp, gi, rb, lr, wd, momentum, it == 0)
        assert bool(torch.isfinite(buf.v).all()), it
    err = np.abs(p.v.cpu().numpy() - rp) / (SGD_ATOL + SGD_RTOL * np.abs(rp))
    print("sgd n=%d wd=%g momentum=%g: worst |err| / (atol + rtol |ref|) = %.3g" % (n, wd, momentum, err.max()))
    np.testing.assert_allclose(p.v.cpu().numpy(), rp, rtol=SGD_RTOL, atol=SGD_ATOL)
    np.testing.assert_allclose(buf.v.cpu().numpy(), rb, rtol=SGD_RTOL, atol=SGD_ATOL)
    assert p.intact() and buf.intact()


def _sgd_segments(device, lengths):
    """[(Guarded p, g, Guarded buf, lr, wd, first)] and the single-launch results (p, buf) of each"""
    _lib, ops, P, st = _lib_ops()
    segs, refs = [], []
    for i, n in enumerate(lengths):
        lr, wd, first = (0.01, 0.02, 0.003)[i % 3], (5e-4, 0.0, 1e-4)[i % 3], i % 2 == 1
        p0, g, m0 = _randn(50 + i, n), _randn(150 + i, n), _randn(250 + i, n)
        if first:
            m0 = np.full(n, np.nan, np.float32)
        gd = _dev(g, device)
        pr, mr = _dev(p0, device), _dev(m0, device)
        if n:
            ops.sgd_momentum_(pr, gd, mr, lr, wd, 0.9, first)
        segs.append((Guarded(n, device, 0, p0), gd, Guarded(n, device, 0, m0), lr, wd, first))
        refs.append((pr, mr))
    return segs, refs


def _sgd_check(segs, refs):
    for i, ((p, _, m, *_), (pr, mr)) in enumerate(zip(segs, refs)):
        assert torch.equal(p.v, pr) and torch.equal(m.v, mr), i
        assert p.intact() and m.intact(), i


def test_sgd_multi_block_boundaries_and_a_full_table(device):
    """scan_sgd_momentum_multi, one library call with exactly 32 table entries: segments of 1, 4095, 4096 and 4097 elements (one
    block of 4096 short by one, exact, and one element into a second block) with zero-length segments between them; every p and
    buf a guarded view.  Bit-identical to one scan_sgd_momentum launch per segment."""
    _lib, ops, P, st = _lib_ops()
    lengths = [1, 0, 4095, 0, 0, 4096, 0, 4097] * 4
    assert len(lengths) == _lib.SGD_MAX_SEGMENTS
    segs, refs = _sgd_segments(device, lengths)
    arr = (_lib.SgdSegment * len(segs))()
    for a, (p, g, m, lr, wd, first) in zip(arr, segs):
        if p.n:  # a zero-length segment carries null pointers: it is skipped before they are looked at
            a.p, a.g, a.buf = p.v.data_ptr(), g.data_ptr(), m.v.data_ptr()
        a.n, a.lr, a.wd, a.first_step, a.reserved = p.n, lr, wd, int(first), 0
    _lib.call("scan_sgd_momentum_multi", arr, len(segs), 0.9, st)
    _sgd_check(segs, refs)


def test_sgd_multi_thirty_three_segments_through_ops(device):
    """ops.sgd_momentum_multi_ with 33 non-empty segments: a full table and a second call with one"""
    _lib, ops, P, st = _lib_ops()
    lengths = ([1, 4095, 4096, 4097, 7] * 7)[:33]
    segs, refs = _sgd_segments(device, lengths)
    ops.sgd_momentum_multi_([(p.v, g, m.v, lr, wd, first) for p, g, m, lr, wd, first in segs], 0.9)
    _sgd_check(segs, refs)


# ============================================================================= 3. 2x2 max pooling
def _pool2_case(device, x, gy, relu_input):
    """ops.maxpool2x2 forward and backward against the reference, then the same two launches into guarded buffers"""
    _lib, ops, P, st = _lib_ops()
    N, H, W, C = x.shape
    ref_y, ref_dx = R.maxpool2x2(x), R.maxpool2x2_backward(x, gy, relu_input)
    shape = ops.PyramidShape(N, [(H, W)])
    xd = _dev(R.rows(x), device).requires_grad_(True)
    y, oshape = ops.maxpool2x2(xd, shape, relu_input=relu_input)
    assert oshape.sizes == [(H // 2, W // 2)] and _eq(y, ref_y)
    gyd = _dev(R.rows(gy), device)
    y.backward(gyd)
    assert _eq(xd.grad, ref_dx)
    yg, dxg = Guarded(ref_y.size, device), Guarded(x.size, device)
    _lib.call("scan_maxpool2x2_forward", P(xd), N, H, W, C, P(yg.v), st)
    _lib.call("scan_maxpool2x2_backward", P(xd), P(yg.v), P(gyd), N, H, W, C, P(dxg.v), int(relu_input), st)
    assert _eq(yg.v, ref_y) and yg.intact() and _eq(dxg.v, ref_dx) and dxg.intact()
    return ref_dx


@pytest.mark.parametrize("relu_input", [False, True])
@pytest.mark.parametrize("shape", [(1, 2, 2, 4), (2, 6, 10, 8), (3, 96, 128, 256)])
def test_maxpool2x2(device, shape, relu_input):
    """the smallest legal map; a small one with several windows per row; N = 3, H = 96, W = 128, C = 256 = 589 824 float4s, whose
    second trip lies in image 2.  relu_input: x is a ReLU output (a sixteenth of its windows are exactly zero)"""
    x = _randn(61, *shape)
    if relu_input:
        x = np.maximum(x, 0)
    gy = _randn(62, shape[0], shape[1] // 2, shape[2] // 2, shape[3])
    _pool2_case(device, x, gy, relu_input)


@pytest.mark.parametrize("relu_input", [False, True])
def test_maxpool2x2_backward_ties_built_by_hand(device, relu_input):
    """ties at (0,1), (1,2), (2,3), (1,3), (0,3), four equal values, -0.0 against +0.0, a block of windows of exact zeros: the
    gradient goes to the first maximum in window order; relu_input: pool_backward(dy) * (x > 0), so zero windows get nothing"""
    C = 8
    x = R.tie_map(C)
    nw = len(R.TIE_WINDOWS)
    gy = (1 + np.arange(nw * C, dtype=np.float32)).reshape(1, 1, nw, C)
    dx = _pool2_case(device, x, gy, relu_input)
    for i, (vals, pos) in enumerate(R.TIE_WINDOWS):  # the reference is what the table says (also pinned on the CPU)
        live = not relu_input or max(vals) > 0
        assert np.array_equal(dx[0, pos >> 1, 2 * i + (pos & 1)], gy[0, 0, i] if live else np.zeros(C, np.float32)), (i, vals)


# ============================================================================= 4. 3x3 / stride 2 / pad 1 max pooling
@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (1, 2, 3, 4), (2, 13, 17, 8), (3, 95, 127, 256)])
def test_maxpool3x3s2(device, shape, negative):
    """1x1 and 2x3 maps (every window cut by the border), odd sizes, and N = 3, H = 95, W = 127, C = 256 = 589 824 float4s.
    negative: -|randn| - 1 everywhere -- padding that contributed 0 instead of -inf would win every border window"""
    _lib, ops, P, st = _lib_ops()
    N, H, W, C = shape
    x = _randn(71, *shape)
    if negative:
        x = -np.abs(x) - 1
    ref = R.maxpool3x3s2(x)
    assert not negative or (ref < 0).all()
    xd = _dev(R.rows(x), device)
    y, oshape = ops.maxpool3x3s2(xd, ops.PyramidShape(N, [(H, W)]))
    assert oshape.sizes == [ref.shape[1:3]] and _eq(y, ref)
    yg = Guarded(ref.size, device)
    _lib.call("scan_maxpool3x3s2_forward", P(xd), N, H, W, C, P(yg.v), st)
    assert _eq(yg.v, ref) and yg.intact()


# ============================================================================= 5. FPN join
@pytest.mark.parametrize("n,h,w,C", [(1, 1, 1, 4), (2, 5, 7, 8), (3, 24, 32, 256), (3, 48, 64, 256)])
def test_upsample2x_add_and_downsample2x_sum(device, n, h, w, C):
    """h = w = 1; a small odd map; N = 3, h = 24, w = 32, C = 256: 589 824 float4s of the join; N = 3, h = 48, w = 64: 589 824
    float4s of its backward.  The backward's window sums in the documented association (g00 + g01) + (g10 + g11): torch.equal"""
    _lib, ops, P, st = _lib_ops()
    lat, coarse, up = _randn(81, n, 2 * h, 2 * w, C), _randn(82, n, h, w, C), _randn(83, n, 2 * h, 2 * w, C)
    ref_y, ref_d = R.upsample2x_add(lat, coarse), R.downsample2x_sum(up)
    ld, cd = _dev(R.rows(lat), device).requires_grad_(True), _dev(R.rows(coarse), device).requires_grad_(True)
    y = ops.upsample2x_add(ld, cd, ops.PyramidShape(n, [(h, w)]))
    assert _eq(y, ref_y)
    upd = _dev(R.rows(up), device)
    y.backward(upd)
    assert _eq(ld.grad, up) and _eq(cd.grad, ref_d)
    yg, dg = Guarded(lat.size, device), Guarded(coarse.size, device)
    _lib.call("scan_upsample2x_add", P(ld), P(cd), n, h, w, C, P(yg.v), st)
    _lib.call("scan_downsample2x_sum", P(upd), n, h, w, C, P(dg.v), st)
    assert _eq(yg.v, ref_y) and yg.intact() and _eq(dg.v, ref_d) and dg.intact()


def test_nhwc_launchers_reject_pointers_off_16_byte_alignment(device):
    """the float4 kernels of the pools and the join: a view entered one float late is an argument error naming the operands, and
    nothing is launched (the outputs keep their sentinel)"""
    _lib, ops, P, st = _lib_ops()
    N, H, W, C = 1, 4, 4, 4
    ok = Guarded(N * H * W * C, device, 0, _randn(91, N * H * W * C))
    off = Guarded(N * H * W * C, device, 1, _randn(91, N * H * W * C))
    out, out_off = Guarded(N * H * W * C, device), Guarded(N * H * W * C, device, 1)
    calls = [
        ("scan_maxpool2x2_forward", (P(off.v), N, H, W, C, P(out.v), st), "x and y"),
        ("scan_maxpool2x2_forward", (P(ok.v), N, H, W, C, P(out_off.v), st), "x and y"),
        ("scan_maxpool2x2_backward", (P(ok.v), P(ok.v), P(off.v), N, H, W, C, P(out.v), 0, st), "x, y, dy and dx"),
        ("scan_maxpool2x2_backward", (P(ok.v), P(ok.v), P(ok.v), N, H, W, C, P(out_off.v), 1, st), "x, y, dy and dx"),
        ("scan_maxpool3x3s2_forward", (P(off.v), N, H, W, C, P(out.v), st), "x and y"),
        ("scan_maxpool3x3s2_forward", (P(ok.v), N, H, W, C, P(out_off.v), st), "x and y"),
        ("scan_upsample2x_add", (P(ok.v), P(off.v), N, H // 2, W // 2, C, P(out.v), st), "lat, coarse and y"),
        ("scan_upsample2x_add", (P(off.v), P(ok.v), N, H // 2, W // 2, C, P(out.v), st), "lat, coarse and y"),
        ("scan_upsample2x_add", (P(ok.v), P(ok.v), N, H // 2, W // 2, C, P(out_off.v), st), "lat, coarse and y"),
        ("scan_downsample2x_sum", (P(off.v), N, H // 2, W // 2, C, P(out.v), st), "g and d"),
        ("scan_downsample2x_sum", (P(ok.v), N, H // 2, W // 2, C, P(out_off.v), st), "g and d"),
    ]
    for name, args, operands in calls:
        with pytest.raises(RuntimeError, match=r"%s: %s must be 16-byte aligned" % (name[5:], operands)):
            _lib.call(name, *args)
        assert _lib.query(name, *args) == -1
    torch.cuda.synchronize()
    assert out.untouched() and out_off.untouched()


# ============================================================================= 6. take_images
TAKE_SIZES = [(16, 24), (8, 12), (4, 6), (2, 3), (1, 2)]  # the pyramid of test_take_images_backward_one_pass, 5 images here


@pytest.mark.parametrize("C", [1, 9, 256])
def test_take_images_backward_of_five_images(device, C):
    """images 1..4 of 5: rows of images 0 and 4 of every level are zero, the others copied.  C = 256: 2560 rows x 256 = 655 360
    elements, a second trip that decodes rows of the last levels; C = 1 and C = 9: rows that are no multiple of anything"""
    _lib, ops, P, st = _lib_ops()
    n, i0, i1 = 5, 1, 4
    shape = ops.PyramidShape(n, TAKE_SIZES)
    x = _randn(101, shape.rows, C)
    sub = R.take_images(x, n, TAKE_SIZES, i0, i1)
    g = _randn(102, *sub.shape)
    ref = R.take_images_backward(g, n, TAKE_SIZES, i0, i1)
    xd = _dev(x, device).requires_grad_(True)
    y, sshape = ops.take_images(xd, shape, i0, i1)
    assert sshape.n_images == i1 - i0 and _eq(y, sub)
    gd = _dev(g, device)
    y.backward(gd)
    assert _eq(xd.grad, ref)
    out = Guarded(ref.size, device)
    _lib.call("scan_take_images_backward", P(gd), shape.ref(), i0, i1, C, P(out.v), st)
    assert _eq(out.v, ref) and out.intact()


# ============================================================================= 7. column block copy
def _copy_cols_case(device, M, ld_src, sc0, ld_dst, dc0, ncols, ztail):
    """src [M, ld_src] read from column sc0, dst [M, ld_dst] (all SENTINEL, guarded) entered at column dc0"""
    _lib, ops, P, st = _lib_ops()
    src = _randn(111, M, ld_src)
    sd = _dev(src, device)
    dst = Guarded(M * ld_dst, device)
    _lib.call("scan_copy_cols", ctypes.c_void_p(sd.data_ptr() + 4 * sc0), ld_src, ctypes.c_void_p(dst.v.data_ptr() + 4 * dc0), ld_dst,
              M, ncols, ztail, st)
    ref = np.full((M, ld_dst), SENTINEL, np.float32)
    ref[:, dc0:] = R.copy_cols(src[:, sc0:], ref[:, dc0:], ncols, ztail)
    assert (ref[:, :dc0] == SENTINEL).all() and (ref[:, dc0 + ncols + ztail:] == SENTINEL).all()
    assert _eq(dst.v, ref) and dst.intact(), (M, ld_src, sc0, ld_dst, dc0, ncols, ztail)


@pytest.mark.parametrize("M,ld_src,sc0,ld_dst,dc0,ncols,ztail", [
    (50000, 9, 0, 12, 0, 9, 3),   # the act-map pad at 600 000 elements: a second trip
    (1000, 9, 1, 268, 256, 8, 4),  # cat_into: the source a column slice (ld_src > ncols), the destination entered at column 256
    (37, 12, 0, 9, 0, 9, 0),       # the pad's backward: ztail = 0
    (37, 5, 0, 16, 3, 0, 7),       # ncols = 0: zeros only
    (1, 9, 2, 12, 1, 5, 2),        # M = 1
    (50000, 12, 0, 9, 0, 9, 0),    # the backward at the large size: 450 000 elements, one trip, rows of 9
])
def test_copy_cols(device, M, ld_src, sc0, ld_dst, dc0, ncols, ztail):
    """the columns of dst outside the written block keep the sentinel, and so do the margins"""
    _copy_cols_case(device, M, ld_src, sc0, ld_dst, dc0, ncols, ztail)


def test_pad_cols_past_the_grid_cap_through_ops(device):
    _lib, ops, P, st = _lib_ops()
    x, g = _randn(121, 50000, 9), _randn(122, 50000, 12)
    xd = _dev(x, device).requires_grad_(True)
    y = ops.pad_cols(xd, 12)
    assert _eq(y, R.copy_cols(x, np.ones((50000, 12), np.float32), 9, 3))
    y.backward(_dev(g, device))
    assert _eq(xd.grad, g[:, :9])


# ============================================================================= 8. paradigm update
PARADIGM_RTOL = PARADIGM_ATOL = 2e-6


@pytest.mark.parametrize("K,C,T", R.PARADIGM_SHAPES)
def test_paradigm_update_against_float64(device, K, C, T):
    """scan_paradigm_update in place on a guarded P, every counter value it = 0..T (it == T shifts the slots), for K = 2, 9, 32,
    C off and on a multiple of 256 up to 1024, T = 1..3.  Every input holds an all-zero current row (norm clamped to 1e-8: the
    result is pb, not NaN), an all-zero batch row, the batch row [1, -1, 0, ...] (sums to exactly 0: class not seen) and a batch
    row equal to the current row (m = 1).  Bar: rtol 2e-6 / atol 2e-6 against float64; the fp32 torch spelling of the update is
    within 0.06 of it on these inputs (measured by test_pointwise_host.py), a factor 16 to spare where 2 is asked for."""
    _lib, ops, P_, st = _lib_ops()
    worst = 0.0
    for it in range(T + 1):
        for P, pb, where in R.paradigm_cases(K, C, T, it):
            ref = R.paradigm_update(P, pb, it)
            Pd = Guarded(P.size, device, 0, P)
            _lib.call("scan_paradigm_update", P_(Pd.v), P_(_dev(pb, device)), K, C, T, it, st)
            got = Pd.v.cpu().numpy().reshape(P.shape)
            assert np.isfinite(got).all(), (it, where)
            worst = max(worst, float((np.abs(got - ref) / (PARADIGM_ATOL + PARADIGM_RTOL * np.abs(ref))).max()))
            np.testing.assert_allclose(got, ref, rtol=PARADIGM_RTOL, atol=PARADIGM_ATOL, err_msg="it=%d %r" % (it, where))
            slot = it - 1 if it == T else it
            for edge, k in where.items():  # rows the update must leave, or set, exactly
                if edge in ("zero_batch", "plus_minus_one"):
                    assert np.array_equal(got[k, :, slot], P[k, :, slot]), (it, edge)
                elif edge == "zero_current":
                    assert np.array_equal(got[k, :, slot], pb[k]), (it, edge)
            assert Pd.intact(), it
    print("paradigm update (K, C, T) = (%d, %d, %d): worst |err| / (atol + rtol |ref|) = %.3g" % (K, C, T, worst))

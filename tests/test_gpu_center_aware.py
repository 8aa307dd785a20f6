"""The two centre-aware kernels (csrc/center_aware.hip) on the GPU: scan_center_aware_map against the fp64 restatement of
tests/epm_ref.py within a bound derived from the kernel's operations, scan_row_scale_levels bit for bit against the fp32
products it is defined as, both through the C ABI (pitches, padding columns, the level-pointer form) and through ops.*
(autograd), and byte-identical repeats in both settings of the deterministic switch."""
import ctypes

import pytest
import torch

import epm_ref

pytestmark = pytest.mark.gpu

STRIDES = (8, 16, 32, 64, 128)
LAMS = (0.02, 0.05, 0.1, 0.3, 0.7)  # one gradient-reversal strength per level, all different


def _pyramid(H, W, N):
    from scan_amd import ops
    return ops.PyramidShape(N, [(-(-H // s), -(-W // s)) for s in STRIDES])


def _map(device, cls, C, ctr_col, weight):
    """C ABI: cls [M, Cs] as given (padding columns and all), centerness = column 4 of an [M, 8] matrix (its place in the head's
    bbox / centerness conv), output pre-filled with NaN"""
    from scan_amd import ops
    M, Cs = cls.shape
    ctr8 = torch.full((M, 8), float("nan"))
    ctr8[:, 4] = ctr_col
    cd, td = cls.to(device), ctr8.to(device)
    out = torch.full((M,), float("nan"), device=device)
    ops.call("scan_center_aware_map", ops._ptr(cd), Cs, C, ops._ptr(td[:, 4]), 8, float(weight), M, ops._ptr(out), ops._stream())
    return out.cpu()


# ----------------------------------------------------------------------------- the map
@pytest.mark.parametrize("C,Cs", [(1, 4), (3, 4), (8, 12)])
@pytest.mark.parametrize("weight", [20.0, 1.0])
def test_map_error_bound(device, C, Cs, weight):
    """387 rows (the pyramid of three 64x96 frames: levels start at rows 288, 360, 378 -- inside a wave -- and 384; the last
    wave holds 3 rows), garbage (1e30, which would win any maximum) in the padding columns.

    Bound, from the kernel's operations, with u = 2^-24 (half an ulp of 1):
      s(x) = 1 / (1 + expf(-x)):  expf is within 1 ulp (relative 2u); its error enters 1 + e damped by e / (1 + e) < 1; the add
                                  rounds (u); the IEEE division rounds (u)                         -> relative error <= 4u
      p = s(max_c x_c), q = s(ctr): 4u each (the maximum of the logits is exact, and sigmoid is increasing)
      t = w * p * q: two roundings                                                                 -> relative error <= 10u
      a = s(t): d a / a = (1 - a) t * (d t / t), and t (1 - s(t)) <= 0.2785 for t >= 0            -> 2.8u from t, + 4u of its own
    so |a - exact| <= 6.8u * a, and a lies in [1/2, 1) for w >= 0, where one ulp is u: the kernel is within 7 ulps; the test
    allows 8 (the fp64 restatement's own rounding is 2^-53)."""
    shape = _pyramid(64, 96, 3)
    M = shape.rows
    assert M == 387 and shape.row_off == [0, 288, 360, 378, 384, 387]
    g = torch.Generator().manual_seed(100 * C + int(weight))
    cls = torch.full((M, Cs), 1e30)
    cls[:, :C] = torch.randn(M, C, generator=g) * 3.0
    ctr = torch.randn(M, generator=g) * 2.0
    got = _map(device, cls, C, ctr, weight)
    ref = epm_ref.center_aware_map(cls[:, :C], ctr, weight)
    err = (got.double() - ref).abs() / 2.0 ** -24
    fp32 = (epm_ref.center_aware_map_fp32(cls[:, :C], ctr, weight).double() - ref).abs() / 2.0 ** -24
    print("center_aware_map C=%d w=%g: worst error %.2f ulp (fp32 torch expressions on the CPU: %.2f ulp)"
          % (C, weight, float(err.max()), float(fp32.max())))
    assert bool(torch.isfinite(got).all()) and float(err.max()) <= 8.0


def test_map_special_inputs(device):
    shape = _pyramid(64, 96, 3)
    M = shape.rows
    g = torch.Generator().manual_seed(7)
    # all-negative logits: a zero padding column entering the maximum would raise it to 0
    cls = torch.zeros(M, 4)
    cls[:, :3] = -1.0 - torch.randn(M, 3, generator=g).abs() * 4.0
    ctr = torch.randn(M, generator=g)
    got = _map(device, cls, 3, ctr, 20.0)
    ref = epm_ref.center_aware_map(cls[:, :3], ctr, 20.0)
    assert float((got.double() - ref).abs().max()) <= 8 * 2.0 ** -24
    wrong = epm_ref.center_aware_map(cls, ctr, 20.0)  # what the zero column would give
    assert float((wrong - ref).abs().max()) > 1e-2  # the case can tell the two apart
    # logits and centerness at +-90: finite, and what the formula gives
    cls = torch.full((M, 4), float("nan"))
    cls[:, :3] = torch.where(torch.rand(M, 3, generator=g) < 0.5, -90.0, 90.0)
    ctr = torch.where(torch.rand(M, generator=g) < 0.5, -90.0, 90.0)
    got = _map(device, cls, 3, ctr, 20.0)
    assert bool(torch.isfinite(got).all())
    assert float((got.double() - epm_ref.center_aware_map(cls[:, :3], ctr, 20.0)).abs().max()) <= 8 * 2.0 ** -24
    # weight 0: sigmoid(0) = 1 / (1 + 1) exactly
    got = _map(device, cls, 3, ctr, 0.0)
    assert torch.equal(got, torch.full((M,), 0.5))


def test_map_op_takes_the_heads_slices(device):
    """ops.center_aware_map on the column slices the head returns ([:, :C] of the padded conv output, a column of the 8-wide
    bbox / centerness conv): no copy needed, same bits as the C ABI on the same storage; no gradient flows"""
    from scan_amd import ops
    M, C = 387, 3
    g = torch.Generator().manual_seed(11)
    cls4 = torch.randn(M, 4, generator=g)
    cls4[:, 3] = 1e30
    out8 = torch.randn(M, 8, generator=g)
    cd, od = cls4.to(device).requires_grad_(True), out8.to(device).requires_grad_(True)
    a = ops.center_aware_map(cd[:, :C], od[:, 4], C, 20.0)
    assert not a.requires_grad and a.shape == (M,)
    assert torch.equal(a.cpu(), _map(device, cls4, C, out8[:, 4], 20.0))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.center_aware_map(cls4[:, :C], out8[:, 4], C, 20.0)


# ----------------------------------------------------------------------------- the row scale
def _row_scale(device, shape, x, ldx, a, s, C, ldy, levels=None):
    from scan_amd import ops
    xd = x.to(device)
    ad = a.to(device) if a is not None else None
    y = torch.full((shape.rows, ldy), -7.0, device=device)
    sv = (ctypes.c_float * shape.n_levels)(*s)
    if levels is None:
        ops.call("scan_row_scale_levels", ops._ptr(xd), ldx, ops._ptr(ad), sv, shape.ref(), C, ops._ptr(y), ldy, ops._stream())
    else:
        parts = [xd[shape.row_off[l]:shape.row_off[l + 1]].clone() if l in levels else None for l in range(shape.n_levels)]
        ptrs = (ctypes.c_void_p * shape.n_levels)(*[p.data_ptr() if p is not None else None for p in parts])
        ops.call("scan_row_scale_levels_ptrs", ptrs, ldx, ops._ptr(ad), sv, shape.ref(), C, ops._ptr(y), ldy, ops._stream())
        torch.cuda.synchronize()
    return y.cpu()


def _level_factor(shape, s):
    return torch.cat([torch.full((shape.row_off[l + 1] - shape.row_off[l],), v, dtype=torch.float32) for l, v in enumerate(s)])


@pytest.mark.parametrize("C,ldx,ldy", [(256, 256, 256), (8, 12, 16), (4, 4, 8)])
@pytest.mark.parametrize("with_a", [True, False])
def test_row_scale_bits(device, C, ldx, ldy, with_a):
    """forward (s = 1): the fp32 product a * x, one rounding; backward (s_l = -lambda_l): fl(fl(-lambda_l * a) * dy), the
    association include/scan_hip.h states; a == NULL: fl(s_l * x).  Pitches larger than C on both sides: the padding columns of
    x (NaN) are never read, those of y keep what was there."""
    shape = _pyramid(64, 96, 3)
    M = shape.rows
    g = torch.Generator().manual_seed(C + ldx)
    x = torch.full((M, ldx), float("nan"))
    x[:, :C] = torch.randn(M, C, generator=g)
    a = torch.rand(M, generator=g) * 0.5 + 0.5 if with_a else None
    for s in ([1.0] * 5, [-v for v in LAMS]):
        got = _row_scale(device, shape, x, ldx, a, s, C, ldy)
        f = _level_factor(shape, s)
        if a is not None:
            f = f * a  # one rounding (exact for s = 1)
        want = f[:, None] * x[:, :C]
        assert torch.equal(got[:, :C], want), (s, float((got[:, :C] - want).abs().max()))
        assert bool((got[:, C:] == -7.0).all())


def test_row_scale_level_pointers_and_missing_levels(device):
    shape = _pyramid(64, 96, 3)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(shape.rows, 256, generator=g)
    a = torch.rand(shape.rows, generator=g)
    s = [-v for v in LAMS]
    got = _row_scale(device, shape, x, 256, a, s, 256, 256, levels=(0, 2, 4))
    want = (_level_factor(shape, s) * a)[:, None] * x
    for l in range(5):
        r0, r1 = shape.row_off[l], shape.row_off[l + 1]
        assert torch.equal(got[r0:r1], want[r0:r1] if l in (0, 2, 4) else torch.zeros(r1 - r0, 256)), l


def test_row_scale_more_rows_than_one_grid_pass(device):
    """the grid is capped at 2048 blocks of 256 lanes, one float4 each: 8192 rows of 256 channels per pass; two 512x768 frames
    are 16368 rows"""
    shape = _pyramid(512, 768, 2)
    assert shape.rows == 16368 > 8192
    g = torch.Generator().manual_seed(9)
    x = torch.randn(shape.rows, 256, generator=g)
    a = torch.rand(shape.rows, generator=g)
    s = [-v for v in LAMS]
    got = _row_scale(device, shape, x, 256, a, s, 256, 256)
    assert torch.equal(got, (_level_factor(shape, s) * a)[:, None] * x)


def test_row_scale_rejects_bad_layouts(device):
    from scan_amd import ops
    shape = _pyramid(64, 96, 1)
    x = torch.zeros(shape.rows, 8, device=device)
    y = torch.zeros(shape.rows, 8, device=device)
    s = (ctypes.c_float * 5)(*[1.0] * 5)
    for C, ldx in ((6, 8), (8, 4), (8, 10)):
        with pytest.raises(RuntimeError, match="row_scale_levels"):
            ops.call("scan_row_scale_levels", ops._ptr(x), ldx, None, s, shape.ref(), C, ops._ptr(y), 8, ops._stream())
    with pytest.raises(RuntimeError, match="aligned"):
        ops.call("scan_row_scale_levels", ctypes.c_void_p(x.data_ptr() + 4), 8, None, s, shape.ref(), 8, ops._ptr(y), 8, ops._stream())


def test_split_levels_grl_op(device):
    """ops.center_aware_split_levels_grl: level views of atten * rows; the backward puts -lambda_l * atten * g_l into the rows of
    one matrix (levels without a gradient: zeros).  With atten None the values of ops.split_levels_grl."""
    from scan_amd import ops
    shape = _pyramid(64, 96, 3)
    g = torch.Generator().manual_seed(21)
    x = torch.randn(shape.rows, 256, generator=g)
    a = torch.rand(shape.rows, generator=g)
    gy = torch.randn(shape.rows, 256, generator=g)
    for atten in (a, None):
        xd = x.to(device).requires_grad_(True)
        ad = atten.to(device) if atten is not None else None
        levels = ops.center_aware_split_levels_grl(xd, ad, shape, LAMS)
        assert len(levels) == 5
        want = x if atten is None else a[:, None] * x
        assert torch.equal(torch.cat([t.detach().cpu() for t in levels]), want)
        used = (0, 1, 3)  # P5 and P7 get no gradient
        sum((levels[l] * gy[shape.row_off[l]:shape.row_off[l + 1]].to(device)).sum() for l in used).backward()
        f = _level_factor(shape, [-v for v in LAMS])
        if atten is not None:
            f = f * a
        wantg = f[:, None] * gy
        for l in range(5):
            r0, r1 = shape.row_off[l], shape.row_off[l + 1]
            assert torch.equal(xd.grad[r0:r1].cpu(), wantg[r0:r1] if l in used else torch.zeros(r1 - r0, 256)), l
    ref = ops.split_levels_grl(x.to(device).requires_grad_(True), shape, LAMS)
    assert all(torch.equal(p, q) for p, q in zip(ref, levels))


def test_weighted_bce_const_mean(device):
    """ops.bce_with_logits_const_mean: mean_m w_m bce(z_m, t) (the 'ca_loss' form) and its gradient against fp64, in both settings
    of the deterministic switch (the ordered twin through ops._call_reduction)"""
    from scan_amd import ops
    g = torch.Generator().manual_seed(33)
    for M in (387, 5000):
        z = torch.randn(M, generator=g) * 3.0
        w = torch.rand(M, generator=g)
        for t in (1.0, 0.0, 0.9):
            for weight in (w, None):
                zr = z.double().requires_grad_(True)
                lr = ((w.double() if weight is not None else 1.0) * epm_ref.bce(zr, t)).mean()
                lr.backward()
                for det in (False, True):
                    old = ops.set_deterministic(det)
                    try:
                        zd = z.to(device).requires_grad_(True)
                        l = ops.bce_with_logits_const_mean(zd, t, weight.to(device) if weight is not None else None)
                        l.backward()
                    finally:
                        ops.set_deterministic(old)
                    assert abs(float(l.detach()) - float(lr.detach())) <= 1e-5 * abs(float(lr.detach())), (M, t, det)
                    assert float((zd.grad.cpu().double() - zr.grad).abs().max()) <= 1e-6 / M * 10, (M, t, det)


# ----------------------------------------------------------------------------- determinism
def test_repeats_are_byte_identical(device):
    from scan_amd import ops
    shape = _pyramid(64, 96, 3)
    g = torch.Generator().manual_seed(77)
    cls = torch.randn(shape.rows, 4, generator=g).to(device)
    ctr = torch.randn(shape.rows, generator=g).to(device)
    x = torch.randn(shape.rows, 256, generator=g).to(device)
    gy = torch.randn(shape.rows, 256, generator=g).to(device)
    runs = []
    for det in (False, True, False, True):
        old = ops.set_deterministic(det)
        try:
            a = ops.center_aware_map(cls[:, :3], ctr, 3, 20.0)
            xd = x.clone().requires_grad_(True)
            levels = ops.center_aware_split_levels_grl(xd, a, shape, LAMS)
            torch.cat(levels).backward(gy)
            runs.append((a.cpu(), torch.cat([t.detach() for t in levels]).cpu(), xd.grad.cpu()))
        finally:
            ops.set_deterministic(old)
    for r in runs[1:]:
        assert all(torch.equal(p, q) for p, q in zip(runs[0], r))

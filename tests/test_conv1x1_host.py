"""The 1x1 convolution oracle of tests/conv1x1_ref.py, everything that needs no GPU: (a) forward, data gradient, weight and bias
gradient against F.conv2d(..., stride=s) and its autograd in float64, on odd sizes, for the three stride maps; the int64 path
against the float64 one on integer inputs; (b) the sums of absolute terms and the bound factors; (c) the comparators are
sensitive: a reference corrupted by one row, one column, or with the (y, x) parity of map 2 swapped is flagged, by the exact
comparator and by the bound comparator."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv1x1_ref as R

N = 2
SIZES = [(13, 21), (7, 11), (1, 1), (1, 2)]   # odd sizes, a single pixel, a single pair
CIN, COUT = 12, 20


def _case(seed, integer=False):
    rs = np.random.RandomState(seed)
    xd = R.Shape(N, SIZES)
    if integer:
        return xd, R.int_inputs(rs, xd.rows, CIN), R.int_inputs(rs, COUT, CIN), R.int_inputs(rs, COUT)
    return xd, rs.randn(xd.rows, CIN).astype(np.float32), rs.randn(COUT, CIN).astype(np.float32), rs.randn(COUT).astype(np.float32)


def _nchw(rows, shape, lvl):
    h, w = shape.sizes[lvl]
    t = torch.from_numpy(np.ascontiguousarray(rows[shape.row_off[lvl]:shape.row_off[lvl + 1]]))
    return t.reshape(shape.n_images, h, w, -1).permute(0, 3, 1, 2)


def _rows(levels):
    return np.concatenate([t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).detach().numpy() for t in levels])


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("stride", [1, 2])
def test_oracle_is_float64_conv2d_and_autograd(stride, relu):
    """forward = map 0 / 1, data gradient = map 0 / 2 on the transposed weight, weight and bias gradient at both strides"""
    xd, x, w, b = _case(stride)
    yd = xd.conv_out(1, stride)
    rs = np.random.RandomState(7)
    dy = rs.randn(yd.rows, COUT)
    wt, bt = torch.from_numpy(w).double().requires_grad_(True), torch.from_numpy(b).double().requires_grad_(True)
    xs = [_nchw(x.astype(np.float64), xd, l).clone().requires_grad_(True) for l in range(xd.n_levels)]
    ys = [F.conv2d(t, wt[:, :, None, None], bt, stride=stride) for t in xs]
    if relu:
        ys = [F.relu(t) for t in ys]
    assert [tuple(t.shape[2:]) for t in ys] == yd.sizes
    y = R.forward(x, w, b, xd, yd, stride - 1, relu=relu)
    np.testing.assert_allclose(y, _rows(ys), rtol=0, atol=1e-13)
    sum((t * _nchw(dy, yd, l)).sum() for l, t in enumerate(ys)).backward()
    dye = dy * (y > 0) if relu else dy
    dx = R.forward(dye, w.T, None, yd, xd, 0 if stride == 1 else 2)
    np.testing.assert_allclose(dx, _rows([t.grad for t in xs]), rtol=0, atol=1e-13)
    dw, db = R.wgrad(x, dye, xd, yd, stride)
    np.testing.assert_allclose(dw, wt.grad.numpy(), rtol=0, atol=1e-11)
    np.testing.assert_allclose(db, bt.grad.numpy(), rtol=0, atol=1e-11)
    # accumulating adds the old values once
    dw0, db0 = rs.randn(COUT, CIN), rs.randn(COUT)
    dwa, dba = R.wgrad(x, dye, xd, yd, stride, dw0, db0)
    np.testing.assert_allclose(dwa, dw + dw0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(dba, db + db0, rtol=0, atol=1e-12)


def test_map2_is_zero_where_a_coordinate_is_odd_and_mask_zeroes():
    xd, _, w, _ = _case(3)
    cd = xd.conv_out(1, 2)
    rs = np.random.RandomState(9)
    dy = rs.randn(cd.rows, COUT)
    mask = rs.randn(xd.rows, CIN)
    dx = R.forward(dy, w.T, None, cd, xd, 2)
    dxm = R.forward(dy, w.T, None, cd, xd, 2, mask=mask)
    for l, (h, wd) in enumerate(xd.sizes):
        lv = dx[xd.row_off[l]:xd.row_off[l + 1]].reshape(N, h, wd, CIN)
        assert not lv[:, 1::2].any() and not lv[:, :, 1::2].any() and lv[:, ::2, ::2].all()
    assert np.array_equal(dxm, np.where(mask > 0, dx, 0)) and (dxm != dx).any()


@pytest.mark.parametrize("cmap", [0, 1, 2])
def test_int64_path_equals_float64_on_integers(cmap):
    """integers in [-8, 8]: |product| <= 64, |sum| <= 64 Cin + 8 < 2^24 -- int64 and float64 agree exactly, and float32 holds it"""
    fine, x, w, b = _case(5, integer=True)
    coarse = fine.conv_out(1, 2)
    xd, yd = {0: (fine, fine), 1: (fine, coarse), 2: (coarse, fine)}[cmap]
    x = x[:xd.rows]
    for relu in (False, True):
        yi = R.forward(x, w, b, xd, yd, cmap, relu=relu, dtype=R.I64)
        yf = R.forward(x, w, b, xd, yd, cmap, relu=relu)
        assert yi.dtype == np.int64 and np.array_equal(yi, yf) and np.array_equal(yi.astype(np.float32), yi)
        assert np.abs(yi).max() <= 64 * CIN + 8
    if cmap < 2:
        dy = R.int_inputs(np.random.RandomState(6), yd.rows, COUT)
        dwi, dbi = R.wgrad(x, dy, xd, yd, cmap + 1, dtype=R.I64)
        dwf, dbf = R.wgrad(x, dy, xd, yd, cmap + 1)
        assert np.array_equal(dwi, dwf) and np.array_equal(dbi, dbf) and np.abs(dwi).max() <= 64 * yd.rows < 2 ** 24
        assert R.first_mismatch(dwi.astype(np.float32), dwi) is None


def test_abs_sums_and_bound_factors():
    xd, x, w, b = _case(8)
    yd = xd.conv_out(1, 2)
    s = R.forward_abs(x, w, b, xd, yd, 1)
    assert np.array_equal(s, R.forward(np.abs(x), np.abs(w), np.abs(b), xd, yd, 1)) and (s >= np.abs(R.forward(x, w, b, xd, yd, 1))).all()
    dy = np.random.RandomState(1).randn(yd.rows, COUT)
    sw, sb = R.wgrad_abs(x, dy, xd, yd, 2, dw0=-np.ones((COUT, CIN)))
    dw, db = R.wgrad(x, dy, xd, yd, 2, dw0=-np.ones((COUT, CIN)))
    assert (sw >= np.abs(dw)).all() and (sb >= np.abs(db)).all() and sw.min() >= 1.0
    u = 2.0 ** -23
    # terms: fp32 K32 + 1, three pieces 6 K32 + 1 (+ 3 u), two pieces 3 K32 + 1 (+ 2^-15); Cin 36 rounds up to 64
    assert R.bound_factor("fp32", 36) == pytest.approx(65 * u, rel=1e-4)
    assert R.bound_factor("bf16x6", 36) == pytest.approx((6 * 64 + 1 + 3) * u, rel=1e-4)
    assert R.bound_factor("bf16x3", 64) == pytest.approx((3 * 64 + 1) * u + 2.0 ** -15, rel=1e-4)
    assert R.bound_factor("bf16x6", 100, colsum=True) == pytest.approx(101 * u, rel=1e-4)
    assert R.bound_factor("bf16x6", 32736) > 6 * 32736 * u   # the gamma form, not its first order


# ----------------------------------------------------------------------------- (c) the comparators have teeth
def _corruptions(ref, yd):
    """name -> a copy of ref with one row / one column moved by the smallest amount the data has (one unit on integer data)"""
    row = ref.copy()
    row[yd.row_off[1] + 3] += 1
    col = ref.copy()
    col[:, ref.shape[1] - 1] += 1
    last = ref.copy()
    last[-1, 0] -= 1
    return {"one_row": row, "one_column": col, "last_row_one_element": last}


def _swapped_parity(fine, coarse, dy, w):
    """map 2 with y and x swapped in the parity test's placement: level by level, the rows of (y even, x even) moved to the
    transposed parity class where the level is not a single row or column, otherwise shifted by one pixel"""
    good = R.forward(dy, w.T, None, coarse, fine, 2, dtype=R.I64)
    bad = good.copy()
    for l, (h, wd) in enumerate(fine.sizes):
        lv = good[fine.row_off[l]:fine.row_off[l + 1]].reshape(N, h, wd, -1)
        if h * wd == 1:
            continue
        bad[fine.row_off[l]:fine.row_off[l + 1]] = np.roll(lv, 1, axis=2 if wd > 1 else 1).reshape(-1, lv.shape[-1])
    return good, bad


def test_exact_comparator_flags_corrupted_references():
    fine, x, w, b = _case(11, integer=True)
    coarse = fine.conv_out(1, 2)
    for cmap, (xd, yd) in {0: (fine, fine), 1: (fine, coarse)}.items():
        ref = R.forward(x, w, b, xd, yd, cmap, dtype=R.I64)
        assert R.first_mismatch(ref.astype(np.float32), ref) is None
        for name, bad in _corruptions(ref, yd).items():
            assert R.first_mismatch(ref.astype(np.float32), bad) is not None, (cmap, name)
    dy = R.int_inputs(np.random.RandomState(12), coarse.rows, COUT)
    good, bad = _swapped_parity(fine, coarse, dy, w)
    assert R.first_mismatch(good.astype(np.float32), good) is None
    assert R.first_mismatch(good.astype(np.float32), bad) is not None
    # every level with more than one pixel is flagged on its own: the (1, 2) level too
    for l in (0, 1, 3):
        r0, r1 = fine.row_off[l], fine.row_off[l + 1]
        assert R.first_mismatch(good[r0:r1], bad[r0:r1]) is not None, l
    # a weight gradient that skipped one row of dY, or took stride 1 for stride 2
    dwi, dbi = R.wgrad(x, dy, fine, coarse, 2, dtype=R.I64)
    dy1 = dy.copy()
    dy1[coarse.rows - 1] = 0
    dw1, db1 = R.wgrad(x, dy1, fine, coarse, 2, dtype=R.I64)
    assert R.first_mismatch(dwi, dw1) is not None and R.first_mismatch(dbi, db1) is not None


@pytest.mark.parametrize("mode", ["fp32", "bf16x6", "bf16x3"])
def test_bound_comparator_flags_corrupted_references(mode):
    """float data: a float32 evaluation of the reference sits inside B S (ratio well below 1), the corrupted references -- one
    row or column off by 1e-3 of the data's scale, the swapped parity -- sit far outside"""
    fine, x, w, b = _case(13)
    coarse = fine.conv_out(1, 2)
    B = R.bound_factor(mode, CIN)
    for cmap, (xd, yd) in {0: (fine, fine), 1: (fine, coarse)}.items():
        ref = R.forward(x, w, b, xd, yd, cmap)
        S = R.forward_abs(x, w, b, xd, yd, cmap)
        got = (R.gather(x, xd, yd, cmap) @ w.T + b).astype(np.float32)   # an fp32 evaluation: one of the orders B allows
        assert R.worst_ratio(got, ref, B * S) < 1.0
        for name, bad in _corruptions(ref * 1e3, yd).items():
            assert R.worst_ratio(got, bad / 1e3, B * S) > 1.0, (cmap, name)
    dy = np.random.RandomState(14).randn(coarse.rows, COUT).astype(np.float32)
    ref = R.forward(dy, w.T, None, coarse, fine, 2)
    S = R.forward_abs(dy, w.T, None, coarse, fine, 2)
    Bd = R.bound_factor(mode, COUT)
    got = (R.gather(dy, coarse, fine, 2) @ w).astype(np.float32)
    assert R.worst_ratio(got, ref, Bd * S) < 1.0
    bad = ref.copy()
    for l, (h, wd) in enumerate(fine.sizes):
        if h * wd > 1:
            lv = ref[fine.row_off[l]:fine.row_off[l + 1]].reshape(N, h, wd, -1)
            bad[fine.row_off[l]:fine.row_off[l + 1]] = np.roll(lv, 1, axis=2 if wd > 1 else 1).reshape(-1, lv.shape[-1])
    assert R.worst_ratio(got, bad, Bd * S) == float("inf")   # a nonzero where the bound is zero, and a zero where a value belongs
    nan = got.copy()
    nan[0, 0] = np.nan
    assert R.worst_ratio(nan, ref, Bd * S) == float("inf")
    # weight and bias gradient
    dw, db = R.wgrad(x, dy, fine, coarse, 2)
    sw, sb = R.wgrad_abs(x, dy, fine, coarse, 2)
    Bw, Bb = R.bound_factor(mode, coarse.rows), R.bound_factor(mode, coarse.rows, colsum=True)
    g32 = R.gather(x, fine, coarse, 1)
    assert R.worst_ratio((dy.T @ g32).astype(np.float32), dw, Bw * sw) < 1.0
    assert R.worst_ratio(dy.sum(0, dtype=np.float32), db, Bb * sb) < 1.0
    dy1 = dy.copy()
    dy1[coarse.rows - 1] = 0
    dw1, db1 = R.wgrad(x, dy1, fine, coarse, 2)
    assert R.worst_ratio((dy.T @ g32).astype(np.float32), dw1, Bw * sw) > 1.0
    assert R.worst_ratio(dy.sum(0, dtype=np.float32), db1, Bb * sb) > 1.0

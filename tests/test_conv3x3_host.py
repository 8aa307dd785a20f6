"""The 3x3 convolution oracle of tests/conv3x3_ref.py, everything that needs no GPU: (a) forward (stride 1 and 2), data gradient,
pool and GroupNorm sums against torch in float64 on every pyramid tests/test_gpu_conv3x3_parity.py uses; the int64 path against
the float64 one on integer data; (b) the integer data of the smallest case tells the errors a 3x3 kernel can make apart: ky and
kx swapped, a tap dropped, the halo taken from the neighbouring image or level instead of zero, the flip omitted in the data
gradient, the last column of an odd width duplicated -- each corrupted oracle differs from the true one, before any GPU is
involved; (c) the Winograd identity and its sum of absolute terms, the bound factors and the comparator."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv3x3_ref as R

FIVE = (2, [(9, 13), (5, 7), (3, 4), (1, 2), (1, 1)])   # the smallest case of the GPU file
PYRAMIDS = {"five": FIVE, "row": (2, [(1, 37)]), "column": (2, [(37, 1)]), "past_tile": (2, [(17, 33)]), "tile": (2, [(16, 16)]),
            "c1064": (1, [(48, 64)]), "c2064": (1, [(32, 48)])}
CIN, COUT = 4, 5


def _nchw(rows, shape, lvl):
    h, w = shape.sizes[lvl]
    t = torch.from_numpy(np.ascontiguousarray(rows[shape.row_off[lvl]:shape.row_off[lvl + 1]]))
    return t.reshape(shape.n_images, h, w, -1).permute(0, 3, 1, 2)


def _rows(levels):
    return np.concatenate([t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).detach().numpy() for t in levels])


def _int_case(seed=0, pyr=FIVE):
    rs = np.random.RandomState(seed)
    d = R.Shape(*pyr)
    return d, R.int_inputs(rs, d.rows, CIN), R.int_inputs(rs, COUT, CIN, 3, 3), R.int_inputs(rs, COUT), R.int_inputs(rs, d.rows, COUT)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("name", sorted(PYRAMIDS))
def test_oracle_is_float64_conv2d_and_autograd(name, stride):
    d = R.Shape(*PYRAMIDS[name])
    yd = d.conv_out(3, stride)
    rs = np.random.RandomState(len(name) + stride)
    x, w, b = rs.randn(d.rows, CIN), rs.randn(COUT, CIN, 3, 3), rs.randn(COUT)
    dy = rs.randn(yd.rows, COUT)
    wt, bt = torch.from_numpy(w).requires_grad_(True), torch.from_numpy(b).requires_grad_(True)
    xs = [_nchw(x, d, l).clone().requires_grad_(True) for l in range(d.n_levels)]
    ys = [F.conv2d(t, wt, bt, stride=stride, padding=1) for t in xs]
    assert [tuple(t.shape[2:]) for t in ys] == yd.sizes
    y = R.forward(x, w, b, d, stride)
    np.testing.assert_allclose(y, _rows(ys), rtol=0, atol=1e-12)
    np.testing.assert_allclose(R.forward(x, w, b, d, stride, relu=True), _rows([F.relu(t) for t in ys]), rtol=0, atol=1e-12)
    sum((t * _nchw(dy, yd, l)).sum() for l, t in enumerate(ys)).backward()
    dx = _rows([t.grad for t in xs])
    np.testing.assert_allclose(R.dgrad(dy, w, d, stride), dx, rtol=0, atol=1e-12)
    if stride == 1:
        np.testing.assert_allclose(R.forward(dy, R.dgrad_weight(w), None, d), dx, rtol=0, atol=1e-12)
        mask = rs.randn(d.rows, CIN)
        assert np.array_equal(R.forward(dy, R.dgrad_weight(w), None, d, mask=mask), np.where(mask > 0, R.forward(dy, R.dgrad_weight(w), None, d), 0))
        # S bounds |y| and is the conv of the absolute values
        s = R.forward_abs(x, w, b, d)
        assert (s >= np.abs(y) - 1e-12).all() and np.array_equal(s, R.forward(np.abs(x), np.abs(w), np.abs(b), d))


def test_pool2_and_gn_sums_are_torchs():
    d = R.Shape(2, [(12, 20)])
    rs = np.random.RandomState(1)
    y = rs.randn(d.rows, 16)
    want = F.max_pool2d(_nchw(y, d, 0), 2)
    assert np.array_equal(R.pool2(y, d), _rows([want]))
    d = R.Shape(*FIVE)
    y = R.int_inputs(rs, d.rows, 256).astype(np.int64)
    s = R.gn_sums(y, d).reshape(d.n_levels, d.n_images, 32, 2)
    assert s.dtype == np.int64
    for l in range(d.n_levels):
        t = _nchw(y, d, l).reshape(d.n_images, 32, 8, -1)
        assert np.array_equal(s[l, :, :, 0], t.sum((2, 3)).numpy()) and np.array_equal(s[l, :, :, 1], (t * t).sum((2, 3)).numpy())


@pytest.mark.parametrize("stride", [1, 2])
def test_int64_path_equals_float64_on_integers(stride):
    """integers in [-8, 8]: |y| <= 64 * 9 * Cin + 8, |dx| <= 64 * 9 * Cout, below 2^24 -- int64 and float64 agree, float32 holds it"""
    d, x, w, b, _ = _int_case(5)
    yd = d.conv_out(3, stride)
    dy = R.int_inputs(np.random.RandomState(6), yd.rows, COUT)
    for relu in (False, True):
        yi = R.forward(x, w, b, d, stride, relu=relu, dtype=R.I64)
        assert yi.dtype == np.int64 and np.array_equal(yi, R.forward(x, w, b, d, stride, relu=relu)) and np.array_equal(yi.astype(np.float32), yi)
        assert np.abs(yi).max() <= 64 * 9 * CIN + 8
    di = R.dgrad(dy, w, d, stride, dtype=R.I64)
    assert di.dtype == np.int64 and np.array_equal(di, R.dgrad(dy, w, d, stride)) and np.abs(di).max() <= 64 * 9 * COUT
    if stride == 1:
        assert np.array_equal(di, R.forward(dy, R.dgrad_weight(w), None, d, dtype=R.I64))
    with pytest.raises(AssertionError):
        R.forward(x + 0.5, w, b, d, dtype=R.I64)


# ----------------------------------------------------------------------------- (b) the data tells the errors apart
def _unbounded(shape, keep):
    """tap rows of a kernel that computes row + (ky - 1) W + (kx - 1) and forgets a bounds test.  keep = "image": the y test is
    missing, the halo above / below an image is the neighbouring image's row (inside the level); "level": the test against the
    level is missing too, the halo comes from the neighbouring level (inside the buffer); the x test is kept in both."""
    good = R.tap_rows(shape)
    bad = good.copy()
    for l, (h, w) in enumerate(shape.sizes):
        r0, r1 = shape.row_off[l], shape.row_off[l + 1]
        lo, hi = (r0, r1) if keep == "image" else (0, shape.rows)
        r = np.arange(r0, r1)
        x = (r - r0) % w
        for ky in range(3):
            for kx in range(3):
                src = r + (ky - 1) * w + (kx - 1)
                ok = (x + kx - 1 >= 0) & (x + kx - 1 < w) & (src >= lo) & (src < hi)
                bad[r0:r1, ky * 3 + kx] = np.where(ok, src, -1)
    return good, bad


def _corrupted(d, x, w, b, dy, dtype=R.I64):
    """name -> (true result, result of the corrupted oracle)"""
    y = R.forward(x, w, b, d, dtype=dtype)
    dx = R.forward(dy, R.dgrad_weight(w), None, d, dtype=dtype)
    out = {"ky_kx_swapped": (y, R.forward(x, w.transpose(0, 1, 3, 2), b, d, dtype=dtype))}
    for t in (0, 4, 8):
        w1 = w.copy()
        w1[:, :, t // 3, t % 3] = 0
        out["tap_%d_dropped" % t] = (y, R.forward(x, w1, b, d, dtype=dtype))
    for keep in ("image", "level"):
        good, bad = _unbounded(d, keep)
        assert (good != bad).any()
        out["halo_from_neighbouring_" + keep] = (y, R.forward(x, w, b, d, dtype=dtype, idx=bad))
    out["flip_omitted"] = (dx, R.forward(dy, w.transpose(1, 0, 2, 3), None, d, dtype=dtype))
    dup = R.tap_rows(d)
    for l, (h, wd) in enumerate(d.sizes):
        if wd % 2 == 1:   # the column right of the last one reads the last one again
            r0, r1 = d.row_off[l], d.row_off[l + 1]
            last = (np.arange(r0, r1) - r0) % wd == wd - 1
            for ky in range(3):
                dup[r0:r1, ky * 3 + 2] = np.where(last, dup[r0:r1, ky * 3 + 1], dup[r0:r1, ky * 3 + 2])
    out["last_odd_column_duplicated"] = (y, R.forward(x, w, b, d, dtype=dtype, idx=dup))
    return out


def test_integer_data_of_the_smallest_case_detects_every_corruption():
    d, x, w, b, dy = _int_case(11)
    for name, (good, bad) in _corrupted(d, x, w, b, dy).items():
        assert R.first_mismatch(good.astype(np.float32), good) is None
        assert R.first_mismatch(good.astype(np.float32), bad) is not None, name
    # the halo corruptions are seen where they act: "image" on every level with more than one row or image boundary, "level" at
    # the first and last rows of the inner levels
    y = R.forward(x, w, b, d, dtype=R.I64)
    _, bad = _unbounded(d, "image")
    yb = R.forward(x, w, b, d, dtype=R.I64, idx=bad)
    for l in range(d.n_levels):
        r0, r1 = d.row_off[l], d.row_off[l + 1]
        assert R.first_mismatch(y[r0:r1], yb[r0:r1]) is not None, l    # two images per level: every level has an inner boundary
    _, bad = _unbounded(d, "level")
    yl = R.forward(x, w, b, d, dtype=R.I64, idx=bad)
    for l in range(d.n_levels):
        r0, r1 = d.row_off[l], d.row_off[l + 1]
        assert R.first_mismatch(yb[r0:r1], yl[r0:r1]) is not None, l   # ... and reads its neighbour level(s) on top of that


def test_bound_comparator_detects_every_corruption():
    """float data: an fp32 evaluation of the oracle sits inside B S in every arithmetic's bound, each corrupted oracle far outside"""
    d = R.Shape(*FIVE)
    rs = np.random.RandomState(13)
    x, w, b, dy = (rs.randn(d.rows, CIN).astype(np.float32), rs.randn(COUT, CIN, 3, 3).astype(np.float32), rs.randn(COUT).astype(np.float32),
                   rs.randn(d.rows, COUT).astype(np.float32))
    got_y = R.forward(x, w, b, d, dtype=np.float32)
    got_dx = R.forward(dy, R.dgrad_weight(w), None, d, dtype=np.float32)
    S = {"y": R.forward_abs(x, w, b, d), "dx": R.forward_abs(dy, R.dgrad_weight(w), None, d)}
    ref = {"y": R.forward(x, w, b, d), "dx": R.forward(dy, R.dgrad_weight(w), None, d)}
    for mode in ("fp32", "bf16x6", "bf16x3"):
        assert R.worst_ratio(got_y, ref["y"], R.bound_factor(mode, CIN) * S["y"]) < 1.0
        assert R.worst_ratio(got_dx, ref["dx"], R.bound_factor(mode, COUT) * S["dx"]) < 1.0
    for name, (good, bad) in _corrupted(d, x.astype(np.float64), w.astype(np.float64), b.astype(np.float64), dy.astype(np.float64), R.F64).items():
        which, got, k = ("dx", got_dx, COUT) if name == "flip_omitted" else ("y", got_y, CIN)
        np.testing.assert_allclose(good, ref[which], rtol=0, atol=1e-12)
        assert R.worst_ratio(got, bad, R.bound_factor("bf16x3", k) * S[which]) > 1.0, name


# ----------------------------------------------------------------------------- (c) Winograd, bound factors, comparator
def test_winograd_terms_sum_to_the_conv_and_are_bounded_by_their_abs_sum():
    """the F(2,3) arithmetic of the docstring, evaluated the way the kernel does it (fp32 transforms, fp32 sums), lies inside
    B_w S_w of the float64 oracle; S_w >= |y|; on integer data the transforms are exact: multiples of 1/2 up to 12, integers up to 16"""
    d = R.Shape(2, [(9, 13), (5, 7), (1, 2), (1, 1)])
    rs = np.random.RandomState(21)
    for integer in (False, True):
        if integer:
            x, w, b = R.int_inputs(rs, d.rows, CIN), R.int_inputs(rs, COUT, CIN, 3, 3), R.int_inputs(rs, COUT)
        else:
            x, w, b = rs.randn(d.rows, CIN).astype(np.float32), rs.randn(COUT, CIN, 3, 3).astype(np.float32), rs.randn(COUT).astype(np.float32)
        xcol = np.concatenate([np.tile(np.arange(wd), d.n_images * h) for h, wd in d.sizes])
        odd = (xcol & 1).astype(bool)[:, None]
        m = [np.zeros((d.rows, COUT), dtype=np.float32) for _ in range(4)]
        vmax = umax = 0.0
        for ky in range(3):
            dk = [R.take(x, R.shifted_rows(d, ky - 1, lambda xx, k=k: k - 1 - (xx & 1))) for k in range(4)]
            v = [dk[0] - dk[2], dk[1] + dk[2], dk[2] - dk[1], dk[1] - dk[3]]                  # float32
            g = w[:, :, ky, :].astype(np.float64)
            u = [g[..., 0], 0.5 * (g[..., 0] + g[..., 1] + g[..., 2]), 0.5 * (g[..., 0] - g[..., 1] + g[..., 2]), g[..., 2]]
            for j in range(4):
                m[j] += v[j] @ u[j].astype(np.float32).T
                vmax, umax = max(vmax, float(np.abs(v[j]).max())), max(umax, float(np.abs(u[j]).max()))
                if integer:
                    assert np.array_equal(2 * u[j], np.rint(2 * u[j]))
        got = np.where(odd, (m[1] - m[2]) - m[3], m[0] + (m[1] + m[2])) + b
        ref = R.forward(x, w, b, d)
        sw = R.forward_abs_wino(x, w, b, d)
        assert (sw >= np.abs(ref) * (1 - 1e-12)).all()
        if integer:
            assert vmax <= 16 and umax <= 12 and np.array_equal(got, ref)
            assert 2 * 12 * 16 * 3 * 512 < 2 ** 24      # units of 1/2, Cin = 512
        else:
            assert R.worst_ratio(got, ref, R.bound_factor("bf16x6", CIN, "wino") * sw) < 1.0
            ratio = float((sw / R.forward_abs(x, w, b, d)).mean())
            assert ratio > 1.0, ratio     # S_w is another sum than S, and the larger one on dense data


def test_bound_factors_and_comparator():
    u = 2.0 ** -23
    # K32 = 9 * round32(Cin): Cin 36 rounds up to 64
    assert R.bound_factor("fp32", 36) == pytest.approx((576 + 1) * u, rel=1e-3)
    assert R.bound_factor("bf16x6", 36) == pytest.approx((6 * 576 + 1 + 3) * u, rel=1e-3)
    assert R.bound_factor("bf16x3", 64) == pytest.approx((3 * 576 + 1) * u + 2.0 ** -15, rel=1e-3)
    assert R.bound_factor("bf16x6", 64, "wino") == pytest.approx((6 * 576 + 1 + 5) * u, rel=1e-3)
    assert R.bound_factor("bf16x6", 512) > 6 * 9 * 512 * u          # the gamma form, not its first order
    assert R.bound_factor("bf16x6", 36, "wino") > R.bound_factor("bf16x6", 36)
    with pytest.raises(AssertionError):
        R.bound_factor("bf16x3", 64, "wino")                         # two pieces never run the Winograd instance
    ref = np.array([[1.0, 2.0], [3.0, 0.0]])
    assert R.worst_ratio(ref, ref, np.zeros_like(ref)) == 0.0
    off = ref.copy()
    off[1, 1] = 1e-30
    assert R.worst_ratio(off, ref, np.zeros_like(ref)) == float("inf")   # a bound of 0 demands equality
    assert R.worst_ratio(off, ref, np.full_like(ref, 2e-30)) == pytest.approx(0.5)
    nan = ref.copy()
    nan[0, 0] = np.nan
    assert R.worst_ratio(nan, ref, np.ones_like(ref)) == float("inf")
    assert R.worst_ratio(np.full_like(ref, np.inf), ref, np.ones_like(ref)) == float("inf")

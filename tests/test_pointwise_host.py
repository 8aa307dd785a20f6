"""The references of tests/pointwise_ref.py against the torch CPU ops the kernels replace, so that the oracle of
tests/test_gpu_pointwise.py and tests/test_gpu_cond_rnn.py is itself pinned on a machine without a GPU.  Needs no
libscan_hip.so.  Also measured here, on the inputs the GPU tests use: how far a plain fp32 evaluation of the paradigm update and
of the cond RNN is from float64 -- the GPU tests' bars rest on these figures."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import pointwise_ref as R


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


# ----------------------------------------------------------------------------- flat kernels
def test_scale_add_relu_and_relu_backward():
    g = _gen(1)
    a, b, dy = (torch.randn(1023, generator=g) for _ in range(3))
    a[::7] = -b[::7]  # sums of exactly zero
    for alpha in (-0.02, 0.5, 0.0, -0.0):
        ref = a * torch.tensor(alpha, dtype=torch.float32)
        assert np.array_equal(R.scale(a.numpy(), alpha).view(np.int32), ref.numpy().view(np.int32)), alpha
    ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = F.relu(ar + br)
    y.backward(dy)
    assert np.array_equal(R.add_relu(a.numpy(), b.numpy()), y.detach().numpy())
    assert np.array_equal(R.relu_backward(dy.numpy(), y.detach().numpy()), ar.grad.numpy())
    assert np.array_equal(ar.grad.numpy(), br.grad.numpy())


@pytest.mark.parametrize("wd,momentum", [(1e-4, 0.9), (0.0, 0.9), (5e-4, 0.0)])
def test_sgd_is_torch_optim_sgd(wd, momentum):
    g = _gen(2)
    p0 = torch.randn(257, generator=g, dtype=torch.float64)
    grad = torch.randn(257, generator=g, dtype=torch.float64)
    pr = p0.clone().requires_grad_(True)
    opt = torch.optim.SGD([pr], lr=0.01, momentum=momentum, weight_decay=wd)
    p, buf = p0.numpy(), np.full(257, np.nan)  # the first step must not read the buffer
    for it in range(3):
        pr.grad = grad * (it + 1)
        opt.step()
        p, buf = R.sgd_step(p, grad.numpy() * (it + 1), buf, 0.01, wd, momentum, it == 0)
    np.testing.assert_allclose(p, pr.detach().numpy(), rtol=1e-13, atol=1e-15)
    assert np.isfinite(buf).all()


# ----------------------------------------------------------------------------- the pools
@pytest.mark.parametrize("shape", [(1, 2, 2, 4), (2, 12, 20, 8), (3, 6, 4, 5)])
def test_maxpool2x2_and_backward(shape):
    g = _gen(3)
    x = torch.randn(*shape, generator=g)
    x[0, 0, 0] = x[0, 0, 1]  # a tie inside a window
    xr = _nchw(x.numpy()).clone().requires_grad_(True)
    yr = F.max_pool2d(xr, 2, 2)
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy)
    assert np.array_equal(R.maxpool2x2(x.numpy()), _nhwc(yr.detach()))
    assert np.array_equal(R.maxpool2x2_backward(x.numpy(), _nhwc(gy)), _nhwc(xr.grad))


@pytest.mark.parametrize("relu_input", [False, True])
def test_maxpool2x2_backward_ties_by_hand(relu_input):
    """every hand-built window: the gradient lands where TIE_WINDOWS says, and where torch's autograd puts it -- behind a ReLU
    (x = relu(z), gradient with respect to z) for relu_input"""
    C = 4
    x = R.tie_map(C)
    nw = len(R.TIE_WINDOWS)
    gy = np.arange(1, nw * C + 1, dtype=np.float32).reshape(1, 1, nw, C)
    dx = R.maxpool2x2_backward(x, gy, relu_input)
    for i, (vals, pos) in enumerate(R.TIE_WINDOWS):
        live = not relu_input or max(vals) > 0
        for p in range(4):
            want = gy[0, 0, i] if (p == pos and live) else np.zeros(C, np.float32)
            assert np.array_equal(dx[0, p >> 1, 2 * i + (p & 1)], want), (i, vals, p)
    if relu_input:
        x = np.maximum(x, 0)  # what a ReLU in front hands the pool; z = the map itself
        z = _nchw(R.tie_map(C)).clone().requires_grad_(True)
        F.max_pool2d(F.relu(z), 2, 2).backward(_nchw(gy))
        assert np.array_equal(R.maxpool2x2_backward(x, gy, True), _nhwc(z.grad))
    else:
        z = _nchw(x).clone().requires_grad_(True)
        F.max_pool2d(z, 2, 2).backward(_nchw(gy))
        assert np.array_equal(dx, _nhwc(z.grad))


@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (1, 2, 3, 4), (2, 12, 20, 8), (2, 13, 17, 4), (1, 95, 127, 4)])
def test_maxpool3x3s2(shape):
    g = _gen(4)
    for x in (torch.randn(*shape, generator=g), -torch.randn(*shape, generator=g).abs() - 1):
        ref = F.max_pool2d(_nchw(x.numpy()), 3, 2, 1)
        got = R.maxpool3x3s2(x.numpy())
        assert got.shape[1:3] == tuple(ref.shape[-2:]) and np.array_equal(got, _nhwc(ref))
    assert (got < 0).all()  # the negative map: no padding value leaked in


# ----------------------------------------------------------------------------- FPN join
@pytest.mark.parametrize("n,h,w,C", [(1, 1, 1, 4), (2, 5, 7, 8)])
def test_upsample2x_add_and_downsample2x_sum(n, h, w, C):
    g = _gen(5)
    lat = torch.randn(n, C, 2 * h, 2 * w, generator=g, requires_grad=True)
    coarse = torch.randn(n, C, h, w, generator=g, requires_grad=True)
    y = lat + F.interpolate(coarse, scale_factor=2, mode="nearest")
    up = torch.randn(y.shape, generator=g)
    y.backward(up)
    assert np.array_equal(R.upsample2x_add(_nhwc(lat.detach()), _nhwc(coarse.detach())), _nhwc(y.detach()))
    d = R.downsample2x_sum(_nhwc(up))
    # torch adds the four window values in an order of its own: equal up to the rounding of two fp32 additions ...
    np.testing.assert_allclose(d, _nhwc(coarse.grad), rtol=1e-6, atol=1e-6)
    # ... and bit for bit in float64 terms on integers, where every order is exact
    ints = torch.randint(-1000, 1000, y.shape, generator=g).float()
    coarse.grad = None
    (lat + F.interpolate(coarse, scale_factor=2, mode="nearest")).backward(ints)
    assert np.array_equal(R.downsample2x_sum(_nhwc(ints)), _nhwc(coarse.grad))
    # the documented association, element by element
    u = _nhwc(up)
    want = (u[0, 0, 0] + u[0, 0, 1]) + (u[0, 1, 0] + u[0, 1, 1])
    assert np.array_equal(d[0, 0, 0], want)


# ----------------------------------------------------------------------------- pyramids and columns
@pytest.mark.parametrize("C,i0,i1", [(1, 1, 4), (9, 1, 4), (8, 0, 2)])
def test_take_images_and_backward(C, i0, i1):
    n, sizes = 5, [(4, 6), (2, 3), (1, 2)]
    ro = R.row_offsets(n, sizes)
    x = torch.randn(ro[-1], C, generator=_gen(6), requires_grad=True)
    parts = [x[ro[l] + i0 * h * w:ro[l] + i1 * h * w] for l, (h, w) in enumerate(sizes)]
    ref = torch.cat(parts, 0)
    assert np.array_equal(R.take_images(x.detach().numpy(), n, sizes, i0, i1), ref.detach().numpy())
    gy = torch.randn(ref.shape, generator=_gen(7))
    ref.backward(gy)
    assert np.array_equal(R.take_images_backward(gy.numpy(), n, sizes, i0, i1), x.grad.numpy())


def test_copy_cols_is_pad_and_slice():
    g = _gen(8)
    x = torch.randn(37, 9, generator=g)
    junk = torch.randn(37, 12, generator=g).numpy()
    assert np.array_equal(R.copy_cols(x.numpy(), junk, 9, 3), F.pad(x, (0, 3)).numpy())
    gy = torch.randn(37, 12, generator=g)
    assert np.array_equal(R.copy_cols(gy.numpy(), np.zeros((37, 9), np.float32), 9, 0), gy[:, :9].numpy())
    wide = torch.randn(37, 20, generator=g).numpy()  # entered at column 5: 4 copied, 2 zeroed, the rest kept
    out = wide.copy()
    out[:, 5:] = R.copy_cols(x.numpy()[:, 2:], wide[:, 5:], 4, 2)
    assert np.array_equal(out[:, 5:9], x.numpy()[:, 2:6]) and not out[:, 9:11].any()
    assert np.array_equal(out[:, :5], wide[:, :5]) and np.array_equal(out[:, 11:], wide[:, 11:])


# ----------------------------------------------------------------------------- paradigm update
PARADIGM_RTOL = PARADIGM_ATOL = 2e-6  # the bar tests/test_gpu_kernels.py holds scan_paradigm_update to


@pytest.mark.parametrize("K,C,T", R.PARADIGM_SHAPES)
def test_paradigm_update_reference_and_fp32_margin(K, C, T):
    """float64: the reference equals the F.cosine_similarity spelling of condgraph.update_prototype_nx1_rnn, and the four edges
    come out as stated.  fp32: that spelling stays within HALF of rtol 2e-6 / atol 2e-6 of the float64 reference on every input
    of the GPU test, so the GPU test may hold the kernel to that bar against float64."""
    worst = 0.0
    seen = set()
    for it in range(T + 1):
        slot = it - 1 if it == T else it
        for P, pb, where in R.paradigm_cases(K, C, T, it):
            seen |= set(where)
            ref = R.paradigm_update(P, pb, it)
            t64 = R.paradigm_update_torch(torch.from_numpy(P).double(), torch.from_numpy(pb).double(), it).numpy()
            np.testing.assert_allclose(ref, t64, rtol=1e-12, atol=1e-13)
            old = P.astype(np.float64)
            for edge, k in where.items():
                if edge == "zero_current":
                    np.testing.assert_allclose(ref[k, :, slot], pb[k], rtol=0, atol=0)
                elif edge in ("zero_batch", "plus_minus_one"):
                    assert np.array_equal(ref[k, :, slot], old[k, :, slot])
                else:
                    np.testing.assert_allclose(ref[k, :, slot], old[k, :, slot], rtol=1e-12)
            if it == T and T > 1:
                assert np.array_equal(ref[:, :, :T - 1], old[:, :, 1:])
            t32 = R.paradigm_update_torch(torch.from_numpy(P), torch.from_numpy(pb), it).numpy()
            worst = max(worst, float((np.abs(t32 - ref) / (PARADIGM_ATOL + PARADIGM_RTOL * np.abs(ref))).max()))
    print("paradigm update (K, C, T) = (%d, %d, %d): fp32 torch spelling, worst |err| / (atol + rtol |ref|) = %.3g" % (K, C, T, worst))
    assert seen == set(R.PARADIGM_EDGES)
    assert worst <= 0.5, worst


# ----------------------------------------------------------------------------- cond RNN
COND_V = (1e-4, 1e-5)  # rtol, atol / max(1, max |ref|): the bars of test_cond_rnn_fused_equals_torch_loop
COND_G = (1e-4, 2e-5)


def _ratio(got, ref, rtol, atol):
    ref = ref.double()
    a = atol * max(1.0, float(ref.abs().max()))
    return float(((got.double() - ref).abs() / (a + rtol * ref.abs())).max())


@pytest.mark.parametrize("K,T,scale", R.COND_RNN_CASES)
def test_cond_rnn_loop_is_nn_rnn_plus_conv(K, T, scale):
    """float64: the loop equals nn.RNN(256, 512, 2, tanh) followed by Conv2d(512, 256, (T, 1)) as
    GRAPHModule.get_conded_weight spells it, values, states and all ten gradients.  fp32: the same loop stays within a quarter of
    the GPU test's bars of the float64 one, so those bars can be held against float64."""
    x, weights, dk = R.cond_rnn_inputs(K, T, scale)
    ker, h0, h1, grads = R.cond_rnn(x, weights, dk)
    rnn = nn.RNN(256, 512, 2, nonlinearity="tanh").double()
    conv = nn.Conv2d(512, 256, (T, 1)).double()
    names = ["%s_l%d" % (n, l) for l in (0, 1) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    params = [getattr(rnn, n) for n in names] + [conv.weight, conv.bias]
    with torch.no_grad():
        for p, w in zip(params, weights):
            p.copy_(w.double().view(p.shape))
    seq, _ = rnn(x.double())  # [T, K, 512]
    out = conv(seq.permute(1, 2, 0).unsqueeze(-1)).reshape(K, 256)
    (out * dk.double()).sum().backward()
    tol = dict(rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(ker.numpy(), out.detach().numpy(), **tol)
    np.testing.assert_allclose(h1.numpy(), seq.detach().numpy(), **tol)
    for name, p, gr in zip(R.COND_RNN_NAMES, params, grads):
        ref = p.grad if p.grad is not None else torch.zeros_like(p)
        np.testing.assert_allclose(gr.numpy(), ref.view(gr.shape).numpy(), err_msg=name, **tol)
    if T == 1:
        assert not grads[1].any() and not grads[5].any()  # no recurrent step: zero gradients, still written
    k32, a32, b32, g32 = R.cond_rnn(x, weights, dk, dtype=torch.float32)
    worst = max([_ratio(k32, ker, *COND_V), _ratio(a32, h0, *COND_V), _ratio(b32, h1, *COND_V)]
                + [_ratio(a, b, *COND_G) for a, b in zip(g32, grads)])
    sat = float((torch.cat([h0, h1]).abs() > 0.99).double().mean())
    print("cond RNN K=%d T=%d scale=%g: fp32 loop worst err / bar = %.3g; share of |h| > 0.99 = %.3f" % (K, T, scale, worst, sat))
    assert worst <= 0.25, worst
    if scale == 0.1:
        assert sat >= 0.2, sat  # the case that drives 1 - h^2 towards cancellation

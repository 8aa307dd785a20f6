"""GPU tests of scan_amd/csrc/condrnn.hip: scan_cond_rnn_forward / _backward called directly on buffers the test owns, against
the float64 loop of tests/pointwise_ref.py (pinned against nn.RNN + Conv2d on the CPU by tests/test_pointwise_host.py): the
kernels [K, 256], the states h0 and h1, and all ten gradients.

Bars: the ones test_cond_rnn_fused_equals_torch_loop holds the kernels to against fp32 torch on the GPU, here against float64 --
values rtol 1e-4, atol 1e-5 * max(1, max |ref|); gradients rtol 1e-4, atol 2e-5 * max(1, max |ref|).  A plain fp32 torch loop
stays within 0.14 of them on every case (test_pointwise_host.py asserts <= 0.25).  Weight scale 0.1 puts a quarter of the hidden
units above |h| = 0.99, where 1 - h^2 loses its digits; at 0.3 a fp32 loop no longer meets these bars, so that is no case.

Every buffer the library writes is a view into a larger buffer of SENTINEL; what it is to fill holds NaN before the call."""
import ctypes

import numpy as np
import pytest
import torch

import pointwise_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
MARGIN = 64
V_RTOL, V_ATOL = 1e-4, 1e-5
G_RTOL, G_ATOL = 1e-4, 2e-5


class Guarded:
    """n floats of `fill` inside a buffer of SENTINEL with MARGIN floats in front and behind"""

    def __init__(self, n, device, fill=float("nan")):
        self.n = int(n)
        self.buf = torch.full((self.n + 2 * MARGIN,), SENTINEL, dtype=torch.float32, device=device)
        self.v = self.buf[MARGIN:MARGIN + self.n]
        self.v.fill_(fill)

    def intact(self):
        return bool((self.buf[:MARGIN] == SENTINEL).all()) and bool((self.buf[MARGIN + self.n:] == SENTINEL).all())


def _check(name, got, ref, rtol, atol):
    ref = ref.double().reshape(-1)
    got = got.detach().cpu().double().reshape(-1)
    a = atol * max(1.0, float(ref.abs().max()))
    ratio = float(((got - ref).abs() / (a + rtol * ref.abs())).max())
    assert bool(torch.isfinite(got).all()), name
    assert ratio <= 1.0, (name, ratio)
    return ratio


@pytest.mark.parametrize("K,T,scale", R.COND_RNN_CASES)
def test_cond_rnn_against_float64(device, K, T, scale):
    """K = 1 and T = 1 (no recurrent step: the recurrent weights' gradients are zeros, still written), K = 2, the full K = 9 /
    T = 3, and weight scale 0.1 (tanh near saturation).  h0 / h1 are allocated for T = 3, K = 9: only the first T * K * 512
    floats may change.  Forward twice and backward twice -- the second backward on the workspace the first one left -- are
    bit-identical: fixed summation order, and nothing is read from ws, h0 or h1 that the call did not write itself."""
    from scan_amd import _lib, ops
    P, st = ops._ptr, ops._stream()
    x, weights, dk = R.cond_rnn_inputs(K, T, scale)
    ker, h0, h1, grads = R.cond_rnn(x, weights, dk)
    xd, dkd = x.to(device).contiguous(), dk.to(device).contiguous()
    wd = [w.to(device).contiguous() for w in weights]
    wptr = (ctypes.c_void_p * 10)(*[w.data_ptr() for w in wd])
    used, full = T * K * 512, 3 * 9 * 512
    ws_n = _lib.query("scan_cond_rnn_ws_floats")
    assert ws_n == 3 * 3 * 9 * 512

    def forward():
        h0g, h1g, kg = Guarded(full, device), Guarded(full, device), Guarded(K * 256, device)
        _lib.call("scan_cond_rnn_forward", P(xd), K, T, wptr, P(h0g.v), P(h1g.v), P(kg.v), st)
        for name, g_ in (("h0", h0g), ("h1", h1g)):
            assert bool(torch.isnan(g_.v[used:]).all()), name + ": written past T * K * 512 floats"
            assert g_.intact(), name
        assert kg.intact()
        return h0g, h1g, kg

    h0g, h1g, kg = forward()
    worst_v = max(_check("kernels", kg.v, ker, V_RTOL, V_ATOL), _check("h0", h0g.v[:used], h0, V_RTOL, V_ATOL),
                  _check("h1", h1g.v[:used], h1, V_RTOL, V_ATOL))
    h0b, h1b, kb = forward()
    assert torch.equal(kg.v, kb.v) and torch.equal(h0g.v[:used], h0b.v[:used]) and torch.equal(h1g.v[:used], h1b.v[:used])

    ws = Guarded(ws_n, device)

    def backward():
        gg = [Guarded(w.numel(), device) for w in wd]
        gptr = (ctypes.c_void_p * 10)(*[g_.v.data_ptr() for g_ in gg])
        _lib.call("scan_cond_rnn_backward", P(xd), K, T, wptr, P(h0g.v), P(h1g.v), P(dkd), gptr, P(ws.v), st)
        for name, g_ in zip(R.COND_RNN_NAMES, gg):
            assert not bool(torch.isnan(g_.v).any()), "gradient of %s not fully overwritten" % name
            assert g_.intact(), name
        assert ws.intact()
        return gg

    g1 = backward()
    worst_g = max(_check(name, g_.v, ref, G_RTOL, G_ATOL) for name, g_, ref in zip(R.COND_RNN_NAMES, g1, grads))
    g2 = backward()  # ws now holds the first call's dS / dA0 / dA1
    for name, a, b in zip(R.COND_RNN_NAMES, g1, g2):
        assert torch.equal(a.v, b.v), name
    if T == 1:
        assert not bool(g1[1].v.any()) and not bool(g1[5].v.any())
    print("cond RNN K=%d T=%d scale=%g: worst err / bar: values %.3g, gradients %.3g" % (K, T, scale, worst_v, worst_g))


def test_cond_rnn_argument_checks(device):
    """K = 0, K = 10, T = 0, T = 4: -1 with cr_check's message before anything is launched; the outputs keep their NaN"""
    from scan_amd import _lib, ops
    P, st = ops._ptr, ops._stream()
    x, weights, dk = R.cond_rnn_inputs(1, 1, 0.05)
    buf = torch.zeros(3 * 10 * 512, device=device)
    wd = [w.to(device).contiguous() for w in weights]
    wptr = (ctypes.c_void_p * 10)(*[w.data_ptr() for w in wd])
    out = Guarded(3 * 10 * 512, device)
    gptr = (ctypes.c_void_p * 10)(*[out.v.data_ptr()] * 10)
    for K, T in ((0, 1), (10, 1), (1, 0), (1, 4)):
        msg = r"K=%d \(<= 9\), T=%d \(<= 3\)" % (K, T)
        with pytest.raises(RuntimeError, match="cond_rnn_forward: " + msg):
            _lib.call("scan_cond_rnn_forward", P(buf), K, T, wptr, P(out.v), P(out.v), P(out.v), st)
        with pytest.raises(RuntimeError, match="cond_rnn_backward: " + msg):
            _lib.call("scan_cond_rnn_backward", P(buf), K, T, wptr, P(buf), P(buf), P(buf), gptr, P(out.v), st)
        assert _lib.query("scan_cond_rnn_forward", P(buf), K, T, wptr, P(out.v), P(out.v), P(out.v), st) == -1
        assert _lib.query("scan_cond_rnn_backward", P(buf), K, T, wptr, P(buf), P(buf), P(buf), gptr, P(out.v), st) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.v).all()) and out.intact()

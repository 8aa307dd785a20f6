"""GPU tests of the five loss families of scan_amd/csrc/losses.hip -- sigmoid focal, IoU, BCE-with-logits, CKA class-weighted
BCE, softmax focal -- on every dispatch path and numeric edge, each against a float64 torch-CPU computation of the reference's
formula: the value AND every gradient element, with the atomic and the ordered (scan_tune "deterministic") reductions.

The bars are the ones tests/test_gpu_kernels.py and tests/test_gpu_deterministic.py already hold each op to:

    op                  value                       gradient
    sigmoid focal sum   1e-4 * max(1, |ref|)        rtol 1e-5 / atol 1e-7   (element losses: rtol 1e-5 / atol 1e-7)
    IoU                 1e-5 * |ref|                rtol 1e-4 / atol 1e-7
    BCE                 1e-6 * max(1, |ref|)        rtol 1e-5 / atol 1e-9
    CKA                 1e-5 * |ref|                rtol 1e-4 / atol 1e-9
    softmax focal       1e-5 * |ref|                rtol 1e-4 / atol 1e-8

Which kernel / instance / in-kernel path a test id reaches is said at its parametrisation.  Shapes are the smallest that reach
the path; the two large cases (softmax focal grid-stride loops, the 512-block cap of the float4 BCE kernel) need their size."""
import contextlib
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

MODES = (False, True)  # atomic / ordered reductions
SENTINEL = -777.25


# ----------------------------------------------------------------------------- plumbing
@contextlib.contextmanager
def deterministic(flag):
    from scan_amd import ops
    old = ops.set_deterministic(flag)
    try:
        yield
    finally:
        ops.set_deterministic(old)


@contextlib.contextmanager
def reduce_blocks(value):
    from scan_amd import _lib
    old = _lib.query("scan_tune", b"reduce_blocks", value)
    try:
        yield
    finally:
        _lib.query("scan_tune", b"reduce_blocks", old)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _offset_copy(t, device, lead):
    """a contiguous device copy of t that starts `lead` elements into its allocation: lead = one row is the ``buf[1:]`` view of a
    buffer with one more row, lead = 1 a flat buffer entered one element late.  Never 16-byte aligned for the shapes used here."""
    buf = torch.empty(t.numel() + lead, dtype=t.dtype, device=device)
    v = buf[lead:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0, (t.shape, lead)
    return v


def _aligned(t, device):
    v = t.to(device).contiguous()
    assert v.numel() == 0 or v.data_ptr() % 16 == 0
    return v


class Case:
    """run() -> (value, gradient) on the GPU from fresh leaves; the float64 value and gradient; the op's bars"""

    def __init__(self, name, run, ref_v, ref_g, vbar, rtol, atol):
        self.name, self.run, self.ref_v, self.ref_g, self.vbar, self.rtol, self.atol = name, run, float(ref_v), ref_g, vbar, rtol, atol


def _check(case, modes=MODES):
    out = {}
    for ordered in modes:
        with deterministic(ordered):
            v, g = case.run()
        v, g = float(v), g.detach().cpu()
        err = (g.double() - case.ref_g).abs()
        print("%s %s: value %.9g fp64 %.9g |diff| %.3g bar %.3g; gradient worst |err| / (atol + rtol |ref|) = %.3g"
              % (case.name, "ordered" if ordered else "atomic", v, case.ref_v, abs(v - case.ref_v), case.vbar,
                 (err / (case.atol + case.rtol * case.ref_g.abs())).max().item() if err.numel() else 0.0))
        assert math.isfinite(v) and bool(torch.isfinite(g).all())
        assert abs(v - case.ref_v) <= case.vbar, (case.name, ordered, v, case.ref_v)
        np.testing.assert_allclose(g.numpy(), case.ref_g.numpy(), rtol=case.rtol, atol=case.atol)
        out[ordered] = (v, g)
    return out


# ============================================================================= 1. sigmoid focal
def _focal_elem64(x, t, gamma, alpha):
    """the reference's element losses (csrc/cuda/SigmoidFocalLoss_cuda.cu:20-58) in float64; 1 - p as sigmoid(-x)"""
    C = x.shape[1]
    cls = torch.arange(1, C + 1).view(1, C)
    tt = t.long().view(-1, 1)
    pos = -(torch.sigmoid(-x) ** gamma) * F.logsigmoid(x) * alpha
    neg = -(torch.sigmoid(x) ** gamma) * F.logsigmoid(-x) * (1 - alpha)
    return torch.where(tt == cls, pos, neg) * (tt >= 0)


def _focal_inputs(M, C, seed):
    """randn * 3 with the leading rows a ramp over [-80, 80]; targets in [-1, C]: ignored rows (-1), rows with no positive (0)"""
    g = _gen(seed)
    x = torch.randn(M, C, generator=g) * 3
    rows = max(1, min(M, 128 // C))
    x[:rows] = torch.linspace(-80, 80, rows * C).view(rows, C)
    t = torch.randint(-1, C + 1, (M,), generator=g).to(torch.int32)
    t[:4] = torch.tensor([-1, 0, 1, C], dtype=torch.int32)[:M]
    assert (t == -1).any() and (t == 0).any() and (t > 0).any()
    return x, t


# id: (M, C, what starts 4 bytes into its allocation) -> focal_fwd_kernel / focal_bwd_kernel instance <CT, G2> and load form
FOCAL_CASES = {
    "c8": (1024, 8, ""),                       # <8, .>, float4
    "c1": (1024, 1, ""),                       # <1, .>, float4 logits + int4 targets
    "c1_tail": (1023, 1, ""),                  # <0, .>, scalar (total % 4 != 0)
    "c1_offset_views": (1024, 1, "both"),      # x[1:], t[1:] of 1,025 rows: <0, .>, scalar
    "c1_offset_targets": (1024, 1, "targets"),  # aligned logits, t[1:]: <0, .>, float4 logits + scalar targets
    "c3": (333, 3, ""),                        # <0, .>, scalar (999 elements)
    "c20": (4, 20, ""),                        # <0, .>, float4, rows change inside a float4
}


def _focal_device(x, t, mis, device):
    xd = _offset_copy(x, device, x.shape[1]) if mis == "both" else _aligned(x, device)
    td = _offset_copy(t, device, 1) if mis in ("both", "targets") else _aligned(t, device)
    return xd, td


@pytest.mark.parametrize("alpha", [0.25, 0.5])
@pytest.mark.parametrize("gamma", [2.0, 1.5, 3.0])  # G2 = true / the powf instances
@pytest.mark.parametrize("case", list(FOCAL_CASES))
def test_sigmoid_focal(device, case, gamma, alpha):
    """ops.sigmoid_focal_loss_sum (value + gradient, both modes) and _C.sigmoid_focalloss_forward / _backward (element losses,
    gradient under a random upstream) against float64, |x| <= 80"""
    from scan_amd import _C, ops
    M, C, mis = FOCAL_CASES[case]
    x, t = _focal_inputs(M, C, 100 + M + C)
    x64 = x.double().requires_grad_(True)
    elem64 = _focal_elem64(x64, t, gamma, alpha)
    g1 = torch.autograd.grad(elem64.sum(), x64)[0]  # element-wise op: the gradient under any upstream u is u * g1
    elem64 = elem64.detach()
    ref = elem64.sum().item()
    xd, td = _focal_device(x, t, mis, device)
    ignored = (t < 0)

    def run():
        leaf = xd.detach().requires_grad_(True)
        assert leaf.data_ptr() == xd.data_ptr()
        loss = ops.sigmoid_focal_loss_sum(leaf, td, gamma, alpha)
        (loss * 0.5).backward()
        return loss.detach(), leaf.grad

    got = _check(Case("focal %s g=%g a=%g" % (case, gamma, alpha), run, ref, 0.5 * g1, 1e-4 * max(1.0, abs(ref)), 1e-5, 1e-7))
    for _, g in got.values():
        assert bool((g[ignored] == 0).all())
    # the drop-in pair
    l = _C.sigmoid_focalloss_forward(xd, td, C, gamma, alpha).cpu()
    np.testing.assert_allclose(l.numpy(), elem64.numpy(), rtol=1e-5, atol=1e-7)
    assert bool((l[ignored] == 0).all())
    up = torch.rand(M, C, generator=_gen(7)) + 0.5
    d = _C.sigmoid_focalloss_backward(xd, td, up.to(device), C, gamma, alpha).cpu()
    np.testing.assert_allclose(d.numpy(), (up.double() * g1).numpy(), rtol=1e-5, atol=1e-7)
    assert bool((d[ignored] == 0).all())


@pytest.mark.parametrize("gamma", [2.0, 1.5, 3.0])
def test_sigmoid_focal_beyond_the_float_range_of_exp(device, gamma):
    """|x| in {88, 100, 104}: exp(-|x|) is denormal or flushed, the positive term sits on the log(FLT_MIN) = -87.33654 clamp of the
    reference's CUDA formula.  float64 has no such clamp, so the yardstick is that formula in floats (oracle.coracle), every
    value as a positive and as a negative; finite everywhere."""
    from oracle import coracle
    from scan_amd import _C
    vals = torch.tensor([88.0, -88.0, 100.0, -100.0, 104.0, -104.0])
    x = vals.repeat(2).view(12, 1).expand(12, 2).contiguous()
    x = torch.cat([x, vals[:2].view(1, 2)])
    t = torch.tensor([1] * 6 + [2] * 6 + [-1], dtype=torch.int32)
    up = torch.rand(13, 2, generator=_gen(8)) + 0.5
    xd, td = x.to(device), t.to(device)
    l = _C.sigmoid_focalloss_forward(xd, td, 2, gamma, 0.25).cpu().numpy()
    d = _C.sigmoid_focalloss_backward(xd, td, up.to(device), 2, gamma, 0.25).cpu().numpy()
    assert np.isfinite(l).all() and np.isfinite(d).all()
    np.testing.assert_allclose(l, coracle.sigmoid_focal_fwd(x.numpy(), t.numpy(), gamma, 0.25), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(d, coracle.sigmoid_focal_bwd(x.numpy(), t.numpy(), up.numpy(), gamma, 0.25), rtol=1e-5, atol=1e-7)
    assert (l[12] == 0).all() and (d[12] == 0).all()


@pytest.mark.parametrize("gamma", [2.0, 1.5])
@pytest.mark.parametrize("case", ["c8", "c1", "c1_tail", "c1_offset_views"])
def test_sigmoid_focal_abi_losses_with_sum_and_scalar_upstream(device, case, gamma):
    """the C ABI directly: `losses` and `loss_sum` from ONE call (the sum is the sum of the elements it returned), the ordered
    twin likewise and with the same elements; d_losses = NULL with d_scale = 0.5 equals an explicit array of 0.5"""
    from scan_amd import _lib, ops
    P, st = ops._ptr, ops._stream
    M, C, mis = FOCAL_CASES[case]
    x, t = _focal_inputs(M, C, 100 + M + C)
    xd, td = _focal_device(x, t, mis, device)
    ref = _focal_elem64(x.double(), t, gamma, 0.25)
    losses, s = torch.full((M, C), SENTINEL, device=device), torch.zeros(1, device=device)
    _lib.call("scan_sigmoid_focal_loss_forward", P(xd), P(td), M, C, gamma, 0.25, P(losses), P(s), st())
    np.testing.assert_allclose(losses.cpu().numpy(), ref.numpy(), rtol=1e-5, atol=1e-7)
    own = losses.double().sum().item()
    assert abs(s.item() - own) <= 1e-4 * max(1.0, abs(own)), (s.item(), own)
    losses_o, s_o = torch.full((M, C), SENTINEL, device=device), torch.full((1,), SENTINEL, device=device)
    ws = torch.empty(_lib.query("scan_sigmoid_focal_loss_ordered_ws_floats", M, C), device=device)
    _lib.call("scan_sigmoid_focal_loss_forward_ordered", P(xd), P(td), M, C, gamma, 0.25, P(losses_o), P(s_o), P(ws), st())
    assert torch.equal(losses_o, losses)
    assert abs(s_o.item() - own) <= 1e-4 * max(1.0, abs(own)), (s_o.item(), own)
    d_scalar, d_array = torch.full((M, C), SENTINEL, device=device), torch.full((M, C), SENTINEL, device=device)
    half = torch.full((M, C), 0.5, device=device)
    _lib.call("scan_sigmoid_focal_loss_backward", P(xd), P(td), None, 0.5, M, C, gamma, 0.25, P(d_scalar), st())
    _lib.call("scan_sigmoid_focal_loss_backward", P(xd), P(td), P(half), 1.0, M, C, gamma, 0.25, P(d_array), st())
    assert torch.equal(d_scalar, d_array) and not bool((d_scalar == SENTINEL).any())


# ============================================================================= 2. IoU
def _iou64(pred, target, weight):
    """layers/iou_loss.py:5-36 in float64, with its rule: the weighted mean only for a weight that sums to more than 0"""
    p, t = pred, target.double()
    ta = (t[:, 0] + t[:, 2]) * (t[:, 1] + t[:, 3])
    pa = (p[:, 0] + p[:, 2]) * (p[:, 1] + p[:, 3])
    wi = torch.min(p[:, 0], t[:, 0]) + torch.min(p[:, 2], t[:, 2])
    hi = torch.min(p[:, 3], t[:, 3]) + torch.min(p[:, 1], t[:, 1])
    inter = wi * hi
    loss = -torch.log((inter + 1.0) / (ta + pa - inter + 1.0))
    if weight is not None and weight.double().sum() > 0:
        return (loss * weight.double()).sum() / weight.double().sum()
    return loss.mean()


def _iou_inputs(P, seed):
    """ordinary boxes rand * 10 + 0.1 and, from P = 450 on, 200 large (pred = exp(randn * 2 + 3) against target = rand * 600 + 1),
    100 tiny (rand * 1e-3), 100 rows with one component tied (each of the four in turn) and 50 rows with all four tied; smaller
    P hold the same kinds in the same proportions"""
    g = _gen(seed)
    p, t = torch.rand(P, 4, generator=g) * 10 + 0.1, torch.rand(P, 4, generator=g) * 10 + 0.1
    n_large, n_tiny, n_tie1, n_tie4 = [k if P >= 450 else P * k // 450 for k in (200, 100, 100, 50)]
    a = 0
    p[a:a + n_large] = torch.exp(torch.randn(n_large, 4, generator=g) * 2 + 3)
    t[a:a + n_large] = torch.rand(n_large, 4, generator=g) * 600 + 1
    a += n_large
    p[a:a + n_tiny] = torch.rand(n_tiny, 4, generator=g) * 1e-3
    a += n_tiny
    for i in range(a, a + n_tie1):
        t[i, i % 4] = p[i, i % 4]
    a += n_tie1
    t[a:a + n_tie4] = p[a:a + n_tie4]
    return p, t, torch.rand(P, generator=g) + 0.01


# P: 1 row; 255 / 257 around one wave-multiple workgroup; 2,049 and 5,000: 2 and 3 workgroups of iou_fwd_kernel
# weight: the weighted mean; none; all zero and a single positive entry -- the reference's `weight.sum() > 0` rule both ways
@pytest.mark.parametrize("weight", ["weighted", "none", "zero", "one_positive"])
@pytest.mark.parametrize("P", [1, 255, 257, 2049, 5000])
def test_iou_loss(device, P, weight):
    """ops.iou_loss, value and gradient, both modes: large, tiny and tied boxes (torch.min's backward splits a tie 0.5 / 0.5 --
    the float64 reference is that backward); a weight that sums to 0 gives the plain mean and ITS gradient, not 0 / 0"""
    from scan_amd import ops
    p, t, w = _iou_inputs(P, 200 + P)
    if weight == "none":
        w = None
    elif weight == "zero":
        w = torch.zeros(P)
    elif weight == "one_positive":
        w = torch.zeros(P)
        w[P // 3] = 0.7
    p64 = p.double().requires_grad_(True)
    ref = _iou64(p64, t, w)
    ref.backward()
    pd, td, wd = p.to(device), t.to(device), (w.to(device) if w is not None else None)

    def run():
        leaf = pd.detach().requires_grad_(True)
        loss = ops.iou_loss(leaf, td, wd)
        loss.backward()
        return loss.detach(), leaf.grad

    _check(Case("iou P=%d %s" % (P, weight), run, ref.item(), p64.grad, 1e-5 * abs(ref.item()), 1e-4, 1e-7))


def test_iou_layer_zero_weight(device):
    """the drop-in module, the reference's call: IOULoss()(pred, target, weight) with a weight of zeros is the plain mean"""
    from scan_amd.layers import IOULoss
    p, t, _ = _iou_inputs(257, 457)
    p64 = p.double().requires_grad_(True)
    ref = _iou64(p64, t, None)
    ref.backward()
    leaf = p.to(device).requires_grad_(True)
    loss = IOULoss()(leaf, t.to(device), torch.zeros(257, device=device))
    loss.backward()
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item())
    np.testing.assert_allclose(leaf.grad.cpu().numpy(), p64.grad.numpy(), rtol=1e-4, atol=1e-7)


# ============================================================================= 3. BCE with logits
def _bce_inputs(M, seed):
    """randn * 3, the first 64 a ramp over [-100, 100] with exact targets 0 / 1 in turn (so each end meets both), others rand"""
    g = _gen(seed)
    x, t = torch.randn(M, generator=g) * 3, torch.rand(M, generator=g)
    n = min(64, M)
    x[:n] = torch.linspace(-100, 100, 64)[:n]
    t[:n] = (torch.arange(n) % 2).float()
    return x, t


# id: (M, logits one float into their allocation) -> bce_fwd_kernel<VEC>
BCE_CASES = {
    "m1": (1, False),             # <false>
    "m4095": (4095, False),       # <false>, below the M >= 4096 threshold
    "m4096": (4096, False),       # <true>, no tail
    "m4097": (4097, False),       # <true>, tail of 1
    "m4099": (4099, False),       # <true>, tail of 3
    "m4096_offset_view": (4096, True),  # x[1:] of 4,097: <false> by the alignment check
}


@pytest.mark.parametrize("case", list(BCE_CASES))
def test_bce_logits_mean(device, case):
    from scan_amd import ops
    M, mis = BCE_CASES[case]
    x, t = _bce_inputs(M, 300 + M)
    x64 = x.double().requires_grad_(True)
    ref = F.binary_cross_entropy_with_logits(x64, t.double())
    ref.backward()
    xd, td = (_offset_copy(x, device, 1) if mis else _aligned(x, device)), _aligned(t, device)

    def run():
        leaf = xd.detach().requires_grad_(True)
        assert leaf.data_ptr() == xd.data_ptr()
        loss = ops.bce_with_logits_mean(leaf, td)
        loss.backward()
        return loss.detach(), leaf.grad

    _check(Case("bce " + case, run, ref.item(), x64.grad, 1e-6 * max(1.0, abs(ref.item())), 1e-5, 1e-9))


def _bce_abi(device, x, t, const_target, w_mat, w_col):
    """scan_bce_logits_forward / _forward_ordered / _backward as the C ABI has them: out2 = {sum l w, sum w}; t = None: const_target;
    w_mat [M, ncol]: its column w_col is the weight (w_stride = ncol); checked against float64 (sums: reduction="sum" and weight.sum())"""
    from scan_amd import _lib, ops
    P, st = ops._ptr, ops._stream
    M = x.numel()
    t64 = t.double() if t is not None else torch.full((M,), const_target, dtype=torch.float64)
    w64 = w_mat[:, w_col].double() if w_mat is not None else None
    x64 = x.double().requires_grad_(True)
    num = F.binary_cross_entropy_with_logits(x64, t64, weight=w64, reduction="sum")
    den = w64.sum().item() if w64 is not None else float(M)
    # the upstream the ops hand the backward: 1 / den, the gradient of the (weighted) mean -- the scale the op's absolute bar of
    # 1e-9 is meant at (sigmoid(x) - t in floats carries half an ulp of 1 = 3e-8 wherever sigmoid(x) is near 1)
    gscale = 1.0 / den
    (num * gscale).backward()
    xd, td = _aligned(x, device), (_aligned(t, device) if t is not None else None)
    wd = _aligned(w_mat, device) if w_mat is not None else None
    wp = P(wd[:, w_col]) if wd is not None else None  # for a one-column matrix: a unit-stride, 16-byte aligned vector
    ws_ = w_mat.shape[1] if w_mat is not None else 0
    args = (P(xd), P(td), float(const_target), wp, ws_, M)
    out = torch.zeros(2, device=device)
    _lib.call("scan_bce_logits_forward", *args, P(out), st())
    out_o = torch.full((2,), SENTINEL, device=device)
    ws = torch.empty(_lib.query("scan_bce_logits_ordered_ws_floats", M), device=device)
    _lib.call("scan_bce_logits_forward_ordered", *args, P(out_o), P(ws), st())
    for o in (out, out_o):
        print("bce abi: num %.9g fp64 %.9g den %.9g fp64 %.9g" % (o[0].item(), num.item(), o[1].item(), den))
        assert abs(o[0].item() - num.item()) <= 1e-6 * max(1.0, abs(num.item()))
        assert abs(o[1].item() - den) <= 1e-6 * max(1.0, abs(den))
    d = torch.full((M,), SENTINEL, device=device)
    _lib.call("scan_bce_logits_backward", *args, P(torch.full((1,), gscale, device=device)), P(d), st())
    np.testing.assert_allclose(d.cpu().numpy(), x64.grad.numpy(), rtol=1e-5, atol=1e-9)


# M = 4,099 (the float4 kernel with a tail of 3 wherever its conditions hold)
# weight: none; w_stride = 1: float4 weights, bce_fwd_kernel<true>; w_stride = 9: column 3 of an [M, 9] matrix, <false>
# targets: an array, or NULL with const_target 0 / 1
@pytest.mark.parametrize("targets", ["array", 0.0, 1.0])
@pytest.mark.parametrize("w_stride", [0, 1, 9])
def test_bce_logits_abi_weight_stride_and_const_target(device, w_stride, targets):
    M = 4099
    x, t = _bce_inputs(M, 350)
    w_mat = torch.rand(M, w_stride, generator=_gen(351)) + 0.01 if w_stride else None
    const = 0.0 if targets == "array" else targets
    _bce_abi(device, x, t if targets == "array" else None, const, w_mat, 3 if w_stride == 9 else 0)


def test_bce_logits_float4_block_cap(device):
    """M = 513 * 8192 + 5: grid_reduce asks for 514 workgroups, bce_fwd_kernel<true> gets min(512, .) and its threads 9 trips
    of the float4 loop (every smaller test: at most 8), then the tail of 1"""
    from scan_amd import ops
    M = 513 * 8192 + 5
    g = _gen(360)
    x, t = torch.randn(M, generator=g) * 3, torch.rand(M, generator=g)
    x64 = x.double().requires_grad_(True)
    ref = F.binary_cross_entropy_with_logits(x64, t.double())
    ref.backward()
    xd, td = _aligned(x, device), _aligned(t, device)

    def run():
        leaf = xd.detach().requires_grad_(True)
        loss = ops.bce_with_logits_mean(leaf, td)
        loss.backward()
        return loss.detach(), leaf.grad

    _check(Case("bce cap", run, ref.item(), x64.grad, 1e-6 * max(1.0, abs(ref.item())), 1e-5, 1e-9))


# ============================================================================= 4. CKA class-weighted BCE
def _cka64(x, act, target, cf):
    a = act.double()
    ref = 0
    for c in range(cf):
        w = a[:, c + 1]
        ref = ref + F.binary_cross_entropy_with_logits(x[:, c], torch.full_like(x[:, c], target), weight=w,
                                                       reduction="sum") / w.sum() / cf
    return ref


def _cka_inputs(M, cf, seed):
    """logits randn * 2 with a row at +60 and (from two rows on) one at -60; act-map rows softmax(randn)"""
    g = _gen(seed)
    logits = torch.randn(M, cf, generator=g) * 2
    logits[0] = 60.0
    if M > 1:
        logits[M // 2] = -60.0
    return logits, torch.softmax(torch.randn(M, cf + 1, generator=g), 1)


def _cka_case(device, name, logits, act, target, cf, ld=None):
    from scan_amd import ops
    l64 = logits.double().requires_grad_(True)
    ref = _cka64(l64, act, target, cf)
    ref.backward()
    ld = _aligned(logits, device) if ld is None else ld
    ad = _aligned(act, device)

    def run():
        leaf = ld.detach().requires_grad_(True)
        assert leaf.data_ptr() == ld.data_ptr()
        loss = ops.cka_bce(leaf, ad, target, cf)
        loss.backward()
        return loss.detach(), leaf.grad

    return _check(Case(name, run, ref.item(), l64.grad, 1e-5 * abs(ref.item()), 1e-4, 1e-9))


# Cf = 8: cka_fwd8_kernel (M = 127 / 128 / 129: 254 / 256 / 258 float4 around one workgroup's threads; 1,025: two trips);
# Cf = 1 and 31: cka_fwd_kernel, the smallest and (with CKA_MAXC = 32) nearly the largest class count
@pytest.mark.parametrize("M", [1, 127, 128, 129, 1025])
@pytest.mark.parametrize("cf", [1, 8, 31])
def test_cka_bce(device, cf, M):
    logits, act = _cka_inputs(M, cf, 400 + 40 * cf + M)
    for target in (1.0, 0.0):
        _cka_case(device, "cka cf=%d M=%d t=%g" % (cf, M, target), logits, act, target, cf)


def test_cka_bce_cf8_offset_view_takes_the_generic_kernel(device):
    """Cf = 8 on a view one float into a flat buffer: cka_is8 is false, cka_fwd_kernel runs with Cf = 8.  Against float64, and
    the same value as the aligned call within the bar."""
    M, cf = 1025, 8
    logits, act = _cka_inputs(M, cf, 480)
    for target in (1.0, 0.0):
        al = _cka_case(device, "cka8 aligned t=%g" % target, logits, act, target, cf)
        off = _cka_case(device, "cka8 offset t=%g" % target, logits, act, target, cf, ld=_offset_copy(logits, device, 1))
        for ordered in MODES:
            assert abs(al[ordered][0] - off[ordered][0]) <= 1e-5 * abs(al[ordered][0])
            np.testing.assert_allclose(off[ordered][1].numpy(), al[ordered][1].numpy(), rtol=1e-4, atol=1e-9)


@pytest.mark.parametrize("cf", [8, 31])
def test_cka_bce_pair_odd_split(device, cf):
    """ops.cka_bce_pair with an odd m: rows [0, m) against 1, rows [m, M) against 0, one gradient buffer"""
    from scan_amd import ops
    M, m = 1025, 513
    logits, act = _cka_inputs(M, cf, 490 + cf)
    l64 = logits.double().requires_grad_(True)
    rs, rt = _cka64(l64[:m], act[:m], 1.0, cf), _cka64(l64[m:], act[m:], 0.0, cf)
    (rs + 2 * rt).backward()
    ld, ad = _aligned(logits, device), _aligned(act, device)
    for ordered in MODES:
        leaf = ld.detach().requires_grad_(True)
        with deterministic(ordered):
            ls, lt = ops.cka_bce_pair(leaf, ad, m, cf)
            (ls + 2 * lt).backward()
        print("cka pair cf=%d: %.9g %.9g fp64 %.9g %.9g" % (cf, ls.item(), lt.item(), rs.item(), rt.item()))
        assert abs(ls.item() - rs.item()) <= 1e-5 * abs(rs.item()) and abs(lt.item() - rt.item()) <= 1e-5 * abs(rt.item())
        np.testing.assert_allclose(leaf.grad.cpu().numpy(), l64.grad.numpy(), rtol=1e-4, atol=1e-9)


@pytest.mark.parametrize("cf", [1, 8, 31])
def test_cka_bce_abi_sums_and_per_class_coefficients(device, cf):
    """scan_cka_bce_forward (the 2 Cf sums, no loss) with its ordered twin, and scan_cka_bce_backward with explicit per-class
    coefficients g[c]:  d_logits[m, c] = g[c] act[m, c + 1] (sigmoid(x) - t)"""
    from scan_amd import _lib, ops
    P, st = ops._ptr, ops._stream
    M = 129
    logits, act = _cka_inputs(M, cf, 495 + cf)
    # coefficients at the scale the layer hands over, g / (Cf den_c), times a factor per class
    coef = ((torch.rand(cf, generator=_gen(496)) + 0.5) / (cf * act[:, 1:].double().sum(0))).float()
    ld, ad = _aligned(logits, device), _aligned(act, device)
    for target in (1.0, 0.0):
        l64 = logits.double().requires_grad_(True)
        sums = []
        for c in range(cf):
            w = act[:, c + 1].double()
            sums += [F.binary_cross_entropy_with_logits(l64[:, c], torch.full((M,), target, dtype=torch.float64), weight=w,
                                                        reduction="sum"), w.sum()]
        sum(s * k for s, k in zip(sums[0::2], coef.double())).backward()
        ref = torch.stack([s.detach() for s in sums])
        out = torch.zeros(2 * cf, device=device)
        _lib.call("scan_cka_bce_forward", P(ld), P(ad), M, cf, target, P(out), st())
        out_o = torch.full((2 * cf,), SENTINEL, device=device)
        ws = torch.empty(_lib.query("scan_cka_bce_ordered_ws_floats", M, cf), device=device)
        _lib.call("scan_cka_bce_forward_ordered", P(ld), P(ad), M, cf, target, P(out_o), P(ws), st())
        for o in (out, out_o):
            assert bool(((o.cpu().double() - ref).abs() <= 1e-5 * ref.abs()).all()), (o, ref)
        d = torch.full((M, cf), SENTINEL, device=device)
        _lib.call("scan_cka_bce_backward", P(ld), P(ad), M, cf, target, P(coef.to(device)), P(d), st())
        np.testing.assert_allclose(d.cpu().numpy(), l64.grad.numpy(), rtol=1e-4, atol=1e-9)


# ============================================================================= 5. softmax focal
CLAMP = 1e-15


def _sfl64(z, lab, gamma):
    """layers/sigmoid_focal_loss_wbg.py:38-64 in float64"""
    p = torch.softmax(z, 1).gather(1, lab.view(-1, 1)).squeeze(1).clamp(min=CLAMP)
    return (-((1 - p) ** gamma) * torch.log(p)).mean()


def _sfl_inputs(M, K, seed):
    """z = randn * 2; the first n = min(50, M // 4) rows x 10, as many all-zero rows.  Of the x 10 rows the first third is labelled
    with its largest logit (p == 1 in floats, or 1 - p in the series branch), the second with its smallest (far below the 1e-15
    clamp), the rest at random.  The clamp is a jump in the gradient: a row whose label probability lies within a factor e of
    it may land on either side in floats, so such rows are zeroed -- at most 1 % of M (the tests assert the share returned
    here); a draw with more is replaced by the next seed."""
    for attempt in range(16):
        g = _gen(seed + 7919 * attempt)
        z = torch.randn(M, K, generator=g) * 2
        lab = torch.randint(0, K, (M,), generator=g)
        n = min(50, M // 4)
        z[:n] *= 10
        z[n:2 * n] = 0
        lab[:n // 3] = z[:n // 3].argmax(1)
        lab[n // 3:2 * (n // 3)] = z[n // 3:2 * (n // 3)].argmin(1)
        p = torch.softmax(z.double(), 1).gather(1, lab.view(-1, 1)).squeeze(1)
        near = (p > CLAMP / math.e) & (p < CLAMP * math.e)
        if int(near.sum()) <= 0.01 * M:
            break
    z[near] = 0
    p = torch.softmax(z.double(), 1).gather(1, lab.view(-1, 1)).squeeze(1)
    return z, lab, int(near.sum()), p


def _sfl_case(device, name, z, lab, gamma, zd=None):
    from scan_amd import ops
    z64 = z.double().requires_grad_(True)
    ref = _sfl64(z64, lab, gamma)
    ref.backward()
    zd = _aligned(z, device) if zd is None else zd
    labd = lab.to(device)

    def run():
        leaf = zd.detach().requires_grad_(True)
        assert leaf.data_ptr() == zd.data_ptr()
        loss = ops.softmax_focal_loss_mean(leaf, labd, gamma)
        loss.backward()
        return loss.detach(), leaf.grad

    return _check(Case(name, run, ref.item(), z64.grad, 1e-5 * abs(ref.item()), 1e-4, 1e-8))


# K: 2 (a shipped config), 9, 16 (the last of sfl_kernel<., ., 16>), 17 and 32 (sfl_kernel<., ., 32>: first and last)
# M: around the 64-row wave batch (63 / 64 / 65, 129) and the 512-row workgroup iteration (511 / 513); 1,000: two workgroups
# gamma: 2 (squares) and 1.5 (the powf branches, forward and backward)
@pytest.mark.parametrize("gamma", [2.0, 1.5])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 129, 511, 513, 1000])
@pytest.mark.parametrize("K", [2, 9, 16, 17, 32])
def test_softmax_focal(device, K, M, gamma):
    z, lab, n_near, p = _sfl_inputs(M, K, 500 + 37 * K + M)
    assert n_near <= 0.01 * M, n_near
    clamped = p < CLAMP
    if M == 1000:  # the edges are really there: rows under the clamp, rows whose p is 1 in floats, rows in the series branch
        assert int(clamped.sum()) >= 2 and int((p.float() == 1).sum()) >= 2
        assert int(((1 - p < 2.0 ** -7) & (p.float() < 1)).sum()) >= 2
    got = _sfl_case(device, "sfl K=%d M=%d g=%g" % (K, M, gamma), z, lab, gamma)
    for _, g in got.values():  # below the clamp: the constant -log(1e-15) (1 - 1e-15)^gamma (in the value), NO gradient
        assert bool((g[clamped] == 0).all())


@pytest.mark.parametrize("K", [9, 17])
def test_softmax_focal_offset_views(device, K):
    """z[1:] of M + 1 rows (36 / 68 bytes in): vec_ok is false, the scalar loads.  ops allocates the gradient itself (aligned), so
    the scalar stores (st_ok false) are reached through the C ABI with a gradient buffer entered one row late."""
    from scan_amd import _lib, ops
    M, gamma = 129, 2.0
    z, lab, n_near, _ = _sfl_inputs(M, K, 560 + K)
    assert n_near <= 0.01 * M
    zd = _offset_copy(z, device, K)
    got = _sfl_case(device, "sfl offset K=%d" % K, z, lab, gamma, zd=zd)
    buf = torch.full(((M + 1) * K,), SENTINEL, device=device)
    d = buf[K:].view(M, K)
    assert d.data_ptr() % 16 != 0
    _lib.call("scan_softmax_focal_backward", ops._ptr(zd), ops._ptr(lab.to(device)), M, K, gamma, 1.0 / M, ops._ptr(d), ops._stream())
    assert torch.equal(d.cpu(), got[False][1])  # same arithmetic, another store form
    assert bool((buf[:K] == SENTINEL).all())


def test_softmax_focal_grid_stride(device):
    """K = 2, M = 512 * 4096 + 577 rows (17 MB of logits): more 512-row iterations than the forward's 2,048 and the backward's
    4,096 workgroups, so both grid-stride loops take a second trip"""
    K, M = 2, 512 * 4096 + 577
    g = _gen(570)
    z = torch.randn(M, K, generator=g) * 2
    lab = torch.randint(0, K, (M,), generator=g)
    _sfl_case(device, "sfl grid-stride", z, lab, 2.0)


# ============================================================================= 6. scan_tune "reduce_blocks"
def _family_case(device, family):
    """one case per family at M = 40,000 rows (40 / 20 / 5 / 40 / 79 workgroups at the default cap of 2,048)"""
    from scan_amd import ops
    M = 40000
    if family == "focal":
        x, t = _focal_inputs(M, 8, 601)
        x64 = x.double().requires_grad_(True)
        ref = _focal_elem64(x64, t, 2.0, 0.25).sum()
        xd, td = _aligned(x, device), _aligned(t, device)
        fn, bars = (lambda leaf: ops.sigmoid_focal_loss_sum(leaf, td, 2.0, 0.25)), (1e-4 * max(1.0, abs(ref.item())), 1e-5, 1e-7)
    elif family == "iou":
        x, t, w = _iou_inputs(M, 602)
        x64 = x.double().requires_grad_(True)
        ref = _iou64(x64, t, w)
        xd, td, wd = _aligned(x, device), _aligned(t, device), _aligned(w, device)
        fn, bars = (lambda leaf: ops.iou_loss(leaf, td, wd)), (1e-5 * abs(ref.item()), 1e-4, 1e-7)
    elif family == "bce":
        x, t = _bce_inputs(M, 603)
        x64 = x.double().requires_grad_(True)
        ref = F.binary_cross_entropy_with_logits(x64, t.double())
        xd, td = _aligned(x, device), _aligned(t, device)
        fn, bars = (lambda leaf: ops.bce_with_logits_mean(leaf, td)), (1e-6 * max(1.0, abs(ref.item())), 1e-5, 1e-9)
    elif family in ("cka8", "cka3"):
        cf = int(family[3:])
        x, act = _cka_inputs(M, cf, 604)
        x64 = x.double().requires_grad_(True)
        ref = _cka64(x64, act, 1.0, cf)
        xd, ad = _aligned(x, device), _aligned(act, device)
        fn, bars = (lambda leaf: ops.cka_bce(leaf, ad, 1.0, cf)), (1e-5 * abs(ref.item()), 1e-4, 1e-9)
    else:
        x, lab, _, _ = _sfl_inputs(M, 9, 605)
        x64 = x.double().requires_grad_(True)
        ref = _sfl64(x64, lab, 2.0)
        xd, labd = _aligned(x, device), lab.to(device)
        fn, bars = (lambda leaf: ops.softmax_focal_loss_mean(leaf, labd, 2.0)), (1e-5 * abs(ref.item()), 1e-4, 1e-8)
    ref.backward()

    def run():
        leaf = xd.detach().requires_grad_(True)
        loss = fn(leaf)
        loss.backward()
        return loss.detach(), leaf.grad

    return Case(family, run, ref.item(), x64.grad, *bars)


# cap 1: one workgroup, hundreds of trips per thread; cap 3: three for focal / BCE / the generic CKA kernel (the `g > cap` branch
# of grid_reduce), 3 / 2 = 1 for the `light` kernels (IoU, CKA-8).  The softmax focal grid does not follow the knob: it rides along.
@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("family", ["focal", "iou", "bce", "cka8", "cka3", "sfl"])
def test_reduce_blocks_cap(device, family, cap):
    case = _family_case(device, family)
    case.name = "%s reduce_blocks=%d" % (family, cap)
    with reduce_blocks(cap):
        first = _check(case)
        with deterministic(True):
            v, g = case.run()
        assert float(v) == first[True][0] and torch.equal(g.cpu(), first[True][1])  # ordered: the same bits every call


# ============================================================================= 7. M = 0
def test_zero_rows_return_ok_and_touch_nothing(device):
    """every loss entry point with M = 0: returns 0 (success), leaves its outputs alone, launches nothing -- no error is pending
    afterwards.  (scan_cka_bce_forward_loss[_ordered] ask for at least one row by contract: the loss is a ratio of sums.)"""
    from scan_amd import _lib, ops
    P, st = ops._ptr, ops._stream
    L = _lib.lib()
    out = torch.full((64,), SENTINEL, device=device)
    ws = torch.full((64,), SENTINEL, device=device)
    e = torch.empty(0, device=device)
    o, w, z = P(out), P(ws), P(e)
    calls = [
        ("scan_sigmoid_focal_loss_forward", (z, z, 0, 8, 2.0, 0.25, o, o, st())),
        ("scan_sigmoid_focal_loss_forward_ordered", (z, z, 0, 8, 2.0, 0.25, o, o, w, st())),
        ("scan_sigmoid_focal_loss_backward", (z, z, z, 1.0, 0, 8, 2.0, 0.25, o, st())),
        ("scan_iou_loss_forward", (z, z, z, 0, o, st())),
        ("scan_iou_loss_forward_ordered", (z, z, z, 0, o, w, st())),
        ("scan_iou_loss_backward", (z, z, z, 0, o, o, st())),
        ("scan_bce_logits_forward", (z, z, 0.0, z, 1, 0, o, st())),
        ("scan_bce_logits_forward_ordered", (z, z, 0.0, z, 1, 0, o, w, st())),
        ("scan_bce_logits_backward", (z, z, 0.0, z, 1, 0, o, o, st())),
        ("scan_cka_bce_forward", (z, z, 0, 8, 1.0, o, st())),
        ("scan_cka_bce_forward_ordered", (z, z, 0, 8, 1.0, o, w, st())),
        ("scan_cka_bce_backward", (z, z, 0, 8, 1.0, o, o, st())),
        ("scan_cka_bce_backward_loss", (z, z, 0, 8, 1.0, o, o, o, st())),
        ("scan_softmax_focal_forward", (z, z, 0, 9, 2.0, o, st())),
        ("scan_softmax_focal_forward_ordered", (z, z, 0, 9, 2.0, o, w, st())),
        ("scan_softmax_focal_backward", (z, z, 0, 9, 2.0, 1.0, o, st())),
    ]
    for name, args in calls:
        assert getattr(L, name)(*args) == 0, (name, L.scan_last_error())
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((ws == SENTINEL).all())
    # a real launch right behind them goes through the library's own pending-error check
    x, y = torch.arange(8, dtype=torch.float32, device=device), torch.empty(8, device=device)
    _lib.call("scan_scale", P(x), 2.0, P(y), 8, st())
    assert torch.equal(y, 2 * x)

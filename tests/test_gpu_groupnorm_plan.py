"""GPU tests of scan_groupnorm_plan / scan_groupnorm_run_forward / scan_groupnorm_run_backward (include/scan_hip.h) against the
older GroupNorm entry points they replace in the bindings: same inputs, same stream.

Where the old result is itself reproducible -- the ordered statistics and backward, the apply launch on given statistics, the
forward from one conv-epilogue sums buffer -- plan + run must give the same bits.  The atomic statistics and the atomic backward
add fp64 partials in an order that is not fixed, two runs of the old entry points need not agree in the last bit, so there the
comparison is at the bars of test_groupnorm_relu (tests/test_gpu_kernels.py).

Shapes: C = 256 (the one built channel count), 2 images.  [(20, 13), (3, 5)]: 260 rows = two 256-row blocks with a 4-row tail,
15 rows = less than one block, and a second level (cross-level block offsets).  [(16, 16)]: a level that fills exactly one block."""
import ctypes
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

C, G, EPS, N, WIDE = 256, 32, 1e-5, 2, 264
PYRAMIDS = {"ragged_two_levels": [(20, 13), (3, 5)], "one_exact_block": [(16, 16)]}


@pytest.fixture(scope="module", params=sorted(PYRAMIDS))
def case(request, device):
    """inputs made once per pyramid and never written: x, dy as the first C columns of a [M, 264] matrix and as a matrix of
    its own, gamma / beta, the fp64 (sum, sum of squares) per (level, image, group) a conv epilogue would have left, and the
    (mean, rstd) table of the ordered statistics kernel (reproducible: what every backward below reads)"""
    from scan_amd import ops
    shape = ops.PyramidShape(N, PYRAMIDS[request.param])
    g = torch.Generator().manual_seed(5)
    x = torch.randn(shape.rows, C, generator=g) * 2 + 0.5
    x64 = x.double()
    sums = []
    for lvl, (h, w) in enumerate(shape.sizes):
        for n in range(N):
            r = x64[shape.row_off[lvl] + n * h * w:shape.row_off[lvl] + (n + 1) * h * w].reshape(h * w, G, C // G)
            sums.append(torch.stack([r.sum((0, 2)), (r * r).sum((0, 2))], 1))
    c = types.SimpleNamespace(shape=shape, x=x.to(device), dy_wide=torch.randn(shape.rows, WIDE, generator=g).to(device),
                              gamma=(1 + 0.1 * torch.randn(C, generator=g)).to(device),
                              beta=(0.1 * torch.randn(C, generator=g)).to(device), sums=torch.cat(sums).contiguous().to(device),
                              fill=torch.randn(2, C, generator=g).to(device))
    c.dy = c.dy_wide[:, :C].contiguous()
    assert c.sums.shape == (shape.n_levels * N * G, 2) and c.sums.dtype == torch.float64
    c.stats = _old_forward(c, True, C)[1]
    return c


def _p(t):
    from scan_amd import ops
    return ops._ptr(t)


def _call(name, *args):
    from scan_amd import _lib, ops
    _lib.call(name, *args, ops._stream())


def _plan(shape, det, flags=0):
    """a plan made with the knob at `det`; the run functions launch what it says whatever the knob says by then"""
    from scan_amd import _lib, ops
    old = ops.set_deterministic(det)
    try:
        plan = _lib.GroupNormPlan()
        _lib.call("scan_groupnorm_plan", shape.ref(), C, G, flags, ctypes.byref(plan))
    finally:
        ops.set_deterministic(old)
    assert plan.ordered == int(det)
    return plan


def _out(c, ld):
    """y as the first C columns of a zeroed [M, ld] matrix, and a poisoned statistics table"""
    return torch.zeros(c.shape.rows, ld, device=c.x.device), torch.full((c.shape.n_levels * N * G * 2,), float("nan"), device=c.x.device)


def _old_ws(c, ordered):
    from scan_amd import _lib
    n = _lib.query("scan_groupnorm_ordered_ws_floats" if ordered else "scan_groupnorm_ws_floats", c.shape.ref(), C, G)
    return torch.empty(n // 2, dtype=torch.float64, device=c.x.device)


def _old_forward(c, ordered, ld, relu=1):
    """the statistics kernels on x, then the apply launch"""
    y, stats = _out(c, ld)
    _call("scan_groupnorm_stats_ordered" if ordered else "scan_groupnorm_stats", _p(c.x), c.shape.ref(), C, G, EPS, _p(stats),
          _p(_old_ws(c, ordered)))
    _call("scan_groupnorm_relu_forward_ld", _p(c.x), c.shape.ref(), C, G, _p(stats), _p(c.gamma), _p(c.beta), relu, _p(y), ld)
    return y, stats


def _old_forward_from_sums(c, separate, ld):
    y, stats = _out(c, ld)
    sums = c.sums.clone()
    if separate:
        _call("scan_groupnorm_stats_from_sums", _p(sums), c.shape.ref(), C, G, EPS, _p(stats))
        _call("scan_groupnorm_relu_forward_ld", _p(c.x), c.shape.ref(), C, G, _p(stats), _p(c.gamma), _p(c.beta), 1, _p(y), ld)
    else:
        _call("scan_groupnorm_relu_forward_from_sums_ld", _p(c.x), c.shape.ref(), C, G, _p(sums), EPS, _p(c.gamma), _p(c.beta), 1,
              _p(y), ld, _p(stats))
    assert torch.equal(sums, c.sums)
    return y, stats


def _new_forward(c, plan, ld, sums=None, relu=1):
    from scan_amd import _lib
    y, stats = _out(c, ld)
    assert plan.stats_floats == stats.numel()
    ws = torch.empty(plan.fwd_ws_doubles, dtype=torch.float64, device=c.x.device) if plan.source == _lib.GN_FROM_X else None
    _call("scan_groupnorm_run_forward", ctypes.byref(plan), _p(c.x), c.shape.ref(), _p(sums), EPS, _p(c.gamma), _p(c.beta), relu,
          _p(y), ld, _p(stats), _p(ws))
    return y, stats


def _grads(c, accumulate):
    """dx poisoned; dgamma / dbeta pre-filled where the call adds to them"""
    dx = torch.full_like(c.x, float("nan"))
    dg, db = (c.fill[0].clone(), c.fill[1].clone()) if accumulate else (torch.full_like(c.gamma, float("nan")), torch.full_like(c.beta, float("nan")))
    return dx, dg, db


def _old_backward(c, ordered, ld, accumulate, relu=1, cleared=False):
    dx, dg, db = _grads(c, accumulate)
    ws = _old_ws(c, ordered)
    if cleared:
        ws.zero_()
    _call("scan_groupnorm_relu_backward_ld_ordered" if ordered else "scan_groupnorm_relu_backward_ld", _p(c.x), _p(c.beta),
          _p(c.dy_wide if ld == WIDE else c.dy), ld, c.shape.ref(), C, G, _p(c.stats), _p(c.gamma), relu, _p(dx), _p(dg), _p(db),
          accumulate | (2 if cleared else 0), _p(ws))
    return dx, dg, db


def _new_backward(c, plan, ld, accumulate, relu=1, cleared=False):
    dx, dg, db = _grads(c, accumulate)
    ws = torch.empty(plan.bwd_ws_doubles, dtype=torch.float64, device=c.x.device)
    if cleared:
        ws.zero_()
    _call("scan_groupnorm_run_backward", ctypes.byref(plan), _p(c.x), _p(c.beta), _p(c.dy_wide if ld == WIDE else c.dy), ld,
          c.shape.ref(), _p(c.stats), _p(c.gamma), relu, _p(dx), _p(dg), _p(db), accumulate, _p(ws), int(cleared))
    return dx, dg, db


def _same_y(new, old, ld):
    assert torch.equal(new[1], old[1]) and not torch.isnan(new[1]).any()  # the (mean, rstd) table
    assert torch.equal(new[0], old[0])
    assert not new[0][:, C:].any() and new[0][:, :C].any()  # the other columns of the wider matrix stay zero


# ----------------------------------------------------------------------------- (a) reproducible: the same bits
@pytest.mark.parametrize("ld", [C, WIDE])
@pytest.mark.parametrize("relu", [1, 0])
def test_ordered_statistics_and_apply_equal_the_old_entry_points(case, ld, relu):
    from scan_amd import _lib
    plan = _plan(case.shape, True, _lib.GN_SUMS)  # sums offered in deterministic mode: not taken
    assert plan.source == _lib.GN_FROM_X
    _same_y(_new_forward(case, plan, ld, sums=case.sums.clone(), relu=relu), _old_forward(case, True, ld, relu), ld)
    assert torch.equal(_new_forward(case, _plan(case.shape, True), ld, relu=relu)[0], _old_forward(case, True, ld, relu)[0])


@pytest.mark.parametrize("ld", [C, WIDE])
@pytest.mark.parametrize("separate", [False, True])
def test_forward_from_sums_equals_the_old_entry_points(case, separate, ld):
    from scan_amd import _lib
    plan = _plan(case.shape, False, _lib.GN_SUMS | (_lib.GN_SEPARATE_FINAL if separate else 0))
    assert plan.source == (_lib.GN_FROM_SUMS_FINAL if separate else _lib.GN_FROM_SUMS)
    sums = case.sums.clone()
    _same_y(_new_forward(case, plan, ld, sums=sums), _old_forward_from_sums(case, separate, ld), ld)
    assert torch.equal(sums, case.sums)
    # the two forms finalise with the same arithmetic (gn_stats_final_kernel's, restated in gn_apply_kernel)
    assert torch.equal(_old_forward_from_sums(case, True, ld)[1], _old_forward_from_sums(case, False, ld)[1])


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("ld", [C, WIDE])
@pytest.mark.parametrize("relu", [1, 0])
def test_ordered_backward_equals_the_old_entry_point(case, relu, ld, accumulate):
    plan = _plan(case.shape, True)
    new = _new_backward(case, plan, ld, accumulate, relu, cleared=bool(accumulate))  # ws_cleared is ignored by an ordered plan
    old = _old_backward(case, True, ld, accumulate, relu)
    for a, b in zip(new, old):
        assert torch.equal(a, b) and not torch.isnan(a).any()
    if accumulate:  # added to what was there
        fresh = _new_backward(case, plan, ld, 0, relu)
        np.testing.assert_allclose((new[1] - case.fill[0]).cpu().numpy(), fresh[1].cpu().numpy(), rtol=1e-5, atol=1e-5)


# ----------------------------------------------------------------------------- (b) atomic: the bars of test_groupnorm_relu
@pytest.mark.parametrize("ld", [C, WIDE])
def test_atomic_statistics_match_the_old_entry_points(case, ld):
    from scan_amd import _lib
    plan = _plan(case.shape, False)
    assert (plan.ordered, plan.source) == (0, _lib.GN_FROM_X)
    new, old = _new_forward(case, plan, ld), _old_forward(case, False, ld)
    np.testing.assert_allclose(new[0].cpu().numpy(), old[0].cpu().numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(new[1].cpu().numpy(), old[1].cpu().numpy(), rtol=1e-4, atol=1e-5)
    assert not new[0][:, C:].any()
    # one launch's sums per accumulator on these shapes where a (level, image) is one block: then the bits agree too
    if case.shape.sizes == [(16, 16)]:
        _same_y(new, old, ld)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("cleared", [False, True])
@pytest.mark.parametrize("ld", [C, WIDE])
def test_atomic_backward_matches_the_old_entry_point(case, ld, cleared, accumulate):
    plan = _plan(case.shape, False)
    new = _new_backward(case, plan, ld, accumulate, cleared=cleared)
    old = _old_backward(case, False, ld, accumulate, cleared=cleared)
    np.testing.assert_allclose(new[0].cpu().numpy(), old[0].cpu().numpy(), rtol=1e-3, atol=2e-5)
    np.testing.assert_allclose(new[1].cpu().numpy(), old[1].cpu().numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(new[2].cpu().numpy(), old[2].cpu().numpy(), rtol=1e-4, atol=1e-4)
    ordered = _old_backward(case, True, ld, accumulate)  # and both against the ordered sums
    np.testing.assert_allclose(new[0].cpu().numpy(), ordered[0].cpu().numpy(), rtol=1e-3, atol=2e-5)
    np.testing.assert_allclose(new[1].cpu().numpy(), ordered[1].cpu().numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(new[2].cpu().numpy(), ordered[2].cpu().numpy(), rtol=1e-4, atol=1e-4)


# ----------------------------------------------------------------------------- (c) the two bindings
def test_bindings_agree_bit_for_bit_in_deterministic_mode(device):
    """ops.groupnorm_relu against the compiled _ops.group_norm_relu on level 0 of the first pyramid, forward and backward, as
    test_compiled_group_norm_relu_ordered_equals_python_path (tests/test_gpu_deterministic.py) compares them on a large level"""
    from scan_amd import layers as L
    from scan_amd import ops
    assert L.OPS_BACKEND == "compiled"
    h, w = PYRAMIDS["ragged_two_levels"][0]
    torch.manual_seed(8)
    x, gy = torch.randn(N, C, h, w), torch.randn(N, C, h, w)
    gamma, beta = torch.rand(C) + 0.5, torch.randn(C) * 0.2
    out = []
    old = ops.set_deterministic(True)
    try:
        for path in ("cpp", "py"):
            xm = x.to(device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
            gd, bd = gamma.to(device).requires_grad_(True), beta.to(device).requires_grad_(True)
            if path == "cpp":
                y = L._ops.group_norm_relu(xm, gd, bd, 1e-5, True)
            else:
                rows, shape, c = L._to_rows(xm)
                y = L._to_nchw(ops.groupnorm_relu(rows, gd, bd, shape, relu=True, eps=1e-5), shape, c)
            y.backward(gy.to(device))
            out.append((y.detach(), xm.grad, gd.grad, bd.grad))
    finally:
        ops.set_deterministic(old)
    for a, b in zip(*out):
        assert torch.equal(a, b) and not torch.isnan(a).any()

"""GPU tests of the deterministic mode (scan_tune "deterministic"): with the knob on, every
order-dependent reduction of the training step runs as an ordered two-stage sum, so repeated calls -- and whole training
steps, serial or overlapped on side streams -- end with the same bits.

Kernel level, per op: (a) 20 calls on the same inputs are torch.equal in the value and every gradient, (d) one of them while
an unrelated elementwise op keeps a side stream busy; (b) the value agrees with the default (atomic) path and (c) with a
float64 torch computation within the bar tests/test_gpu_kernels.py holds that op to (quoted at each use).  Shapes: at least 16
reducing workgroups (one per 2,048 work items), plus one row and exactly one workgroup (every slot of the workspace must be
written whatever the grid)."""
import contextlib
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

REPEATS = 20
BUSY_AT = 7  # the repeat that runs beside a busy side stream


@contextlib.contextmanager
def deterministic(flag):
    from scan_amd import ops
    old = ops.set_deterministic(flag)
    try:
        yield
    finally:
        ops.set_deterministic(old)


_busy_state = {}


@contextlib.contextmanager
def busy_side_stream(device):
    """a large elementwise op queued on a side stream: the call inside the block shares the GPU with it, which moves the
    order its workgroups are placed and finish in"""
    if "buf" not in _busy_state:
        _busy_state["buf"] = torch.ones(1 << 25, device=device)
        _busy_state["stream"] = torch.cuda.Stream(device)
    side = _busy_state["stream"]
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        for _ in range(6):
            _busy_state["buf"].mul_(1.0)
    try:
        yield
    finally:
        torch.cuda.current_stream(device).wait_stream(side)


def _repeat_equal(device, run, repeats=REPEATS):
    """run() -> tuple of tensors; `repeats` calls under the knob, one beside a busy side stream, all bit-identical"""
    first = None
    with deterministic(True):
        for i in range(repeats):
            with (busy_side_stream(device) if i == min(BUSY_AT, repeats - 1) else contextlib.nullcontext()):
                out = [t.detach().clone() for t in run()]
            if first is None:
                first = out
            else:
                for k, (a, b) in enumerate(zip(first, out)):
                    assert torch.equal(a, b), "call %d, output %d: max diff %g" % (i, k, (a - b).abs().max().item())
    with deterministic(False):
        default = [t.detach().clone() for t in run()]
    return first, default


def _leaf(t, device):
    return t.to(device).requires_grad_(True)


# M = 40,000 rows x 8 classes: 40 / 20 / 40 / 40 / 20 / 79 workgroups for focal / IoU / BCE / CKA-8 / CKA-3 / softmax focal;
# 1,024 rows: exactly one workgroup for the focal and the CKA-8 kernels; 1 row
SIZES = [40000, 1024, 1]


def _repeats_for(M):
    return REPEATS if M == SIZES[0] else 3


# ----------------------------------------------------------------------------- float64 references
def _focal_sum64(x, t, gamma, alpha):
    x = x.double()
    C = x.shape[1]
    cls = torch.arange(1, C + 1).view(1, C)
    tt = t.long().view(-1, 1)
    logp, log1mp = F.logsigmoid(x), F.logsigmoid(-x)
    p = torch.sigmoid(x)
    pos = -((1 - p) ** gamma) * logp * alpha
    neg = -(p ** gamma) * log1mp * (1 - alpha)
    loss = torch.where(tt == cls, pos, neg) * (tt >= 0)
    return loss.sum()


def _iou64(pred, target, weight):
    p, t = pred.double(), target.double()
    ta = (t[:, 0] + t[:, 2]) * (t[:, 1] + t[:, 3])
    pa = (p[:, 0] + p[:, 2]) * (p[:, 1] + p[:, 3])
    wi = torch.min(p[:, 0], t[:, 0]) + torch.min(p[:, 2], t[:, 2])
    hi = torch.min(p[:, 3], t[:, 3]) + torch.min(p[:, 1], t[:, 1])
    inter = wi * hi
    loss = -torch.log((inter + 1.0) / (ta + pa - inter + 1.0))
    w = weight.double()
    return (loss * w).sum() / w.sum()


def _cka64(logits, act, target, cf):
    x, a = logits.double(), act.double()
    ref = 0
    for c in range(cf):
        w = a[:, c + 1]
        ref = ref + F.binary_cross_entropy_with_logits(x[:, c], torch.full_like(x[:, c], target), weight=w,
                                                       reduction="sum") / w.sum() / cf
    return ref


def _sfl64(z, lab, gamma):
    p = torch.softmax(z.double(), 1).gather(1, lab.view(-1, 1)).squeeze(1).clamp(min=1e-15)
    return (-((1 - p) ** gamma) * torch.log(p)).mean()


# ----------------------------------------------------------------------------- losses
@pytest.mark.parametrize("M", SIZES)
def test_sigmoid_focal_sum_ordered(device, M):
    from scan_amd import ops
    g = torch.Generator().manual_seed(10 + M)
    x = torch.randn(M, 8, generator=g) * 3
    t = torch.randint(-1, 9, (M,), generator=g).to(torch.int32)
    xd, td = _leaf(x, device), t.to(device)

    def run():
        xd.grad = None
        loss = ops.sigmoid_focal_loss_sum(xd, td, 2.0, 0.25)
        (loss * 0.5).backward()
        return loss, xd.grad

    (v, dx), (v0, dx0) = _repeat_equal(device, run, _repeats_for(M))
    ref = _focal_sum64(x, t, 2.0, 0.25).item()
    # test_sigmoid_focal_layer_sum_and_tail: abs(loss - ref) <= 1e-4 * max(1.0, abs(ref)); gradient rtol 1e-5 / atol 1e-7
    bar = 1e-4 * max(1.0, abs(ref))
    print("focal M=%d ordered %.9g default %.9g fp64 %.9g" % (M, v.item(), v0.item(), ref))
    assert abs(v.item() - v0.item()) <= bar and abs(v.item() - ref) <= bar
    np.testing.assert_allclose(dx.cpu().numpy(), dx0.cpu().numpy(), rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("M", SIZES)
def test_iou_loss_ordered(device, M):
    from scan_amd import ops
    g = torch.Generator().manual_seed(20 + M)
    pred, target = torch.rand(M, 4, generator=g) * 10 + 0.1, torch.rand(M, 4, generator=g) * 10 + 0.1
    w = torch.rand(M, generator=g) + 0.01
    pd, tg, wd = _leaf(pred, device), target.to(device), w.to(device)

    def run():
        pd.grad = None
        loss = ops.iou_loss(pd, tg, wd)
        loss.backward()
        return loss, pd.grad

    (v, dp), (v0, dp0) = _repeat_equal(device, run, _repeats_for(M))
    ref = _iou64(pred, target, w).item()
    print("iou M=%d ordered %.9g default %.9g fp64 %.9g" % (M, v.item(), v0.item(), ref))
    # test_iou_loss_golden: abs(l - ref) <= 1e-5 * abs(ref); gradient rtol 1e-4 / atol 1e-7
    assert abs(v.item() - v0.item()) <= 1e-5 * abs(ref) and abs(v.item() - ref) <= 1e-5 * abs(ref)
    np.testing.assert_allclose(dp.cpu().numpy(), dp0.cpu().numpy(), rtol=1e-4, atol=1e-7)


@pytest.mark.parametrize("M", [40000 * 8, 4000, 1])  # 40 workgroups of the float4 form; 2 of the scalar form (M < 4,096); one row
def test_bce_logits_mean_ordered(device, M):
    from scan_amd import ops
    g = torch.Generator().manual_seed(30 + M % 97)
    x, t = torch.randn(M, generator=g) * 3, torch.rand(M, generator=g)
    xd, td = _leaf(x, device), t.to(device)

    def run():
        xd.grad = None
        loss = ops.bce_with_logits_mean(xd, td)
        loss.backward()
        return loss, xd.grad

    (v, dx), (v0, _) = _repeat_equal(device, run, REPEATS if M > 100000 else 3)
    x64 = x.double().requires_grad_(True)
    ref = F.binary_cross_entropy_with_logits(x64, t.double())
    ref.backward()
    print("bce M=%d ordered %.9g default %.9g fp64 %.9g" % (M, v.item(), v0.item(), ref.item()))
    # test_bce_and_cka: abs(l - ref) < 1e-6 * max(1, abs(ref)); gradient rtol 1e-5 / atol 1e-9
    bar = 1e-6 * max(1.0, abs(ref.item()))
    assert abs(v.item() - v0.item()) < bar and abs(v.item() - ref.item()) < bar
    np.testing.assert_allclose(dx.cpu().numpy(), x64.grad.float().numpy(), rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("cf", [8, 3])  # cka_fwd8_kernel / the generic kernel
def test_cka_bce_ordered(device, M, cf):
    from scan_amd import ops
    g = torch.Generator().manual_seed(40 + M + cf)
    logits = torch.randn(M, cf, generator=g) * 2
    act = torch.softmax(torch.randn(M, cf + 1, generator=g), 1)
    ad = act.to(device)
    for target in (1.0, 0.0):
        ld = _leaf(logits, device)

        def run():
            ld.grad = None
            loss = ops.cka_bce(ld, ad, target, cf)
            loss.backward()
            return loss, ld.grad

        (v, dl), (v0, _) = _repeat_equal(device, run, _repeats_for(M) if target == 1.0 else 3)
        l64 = logits.double().requires_grad_(True)
        ref = _cka64(l64, act, target, cf)
        ref.backward()
        print("cka M=%d cf=%d t=%g ordered %.9g default %.9g fp64 %.9g" % (M, cf, target, v.item(), v0.item(), ref.item()))
        # test_bce_and_cka: abs(l - ref) < 1e-5 * abs(ref); gradient rtol 1e-4 / atol 1e-9
        assert abs(v.item() - v0.item()) < 1e-5 * abs(ref.item()) and abs(v.item() - ref.item()) < 1e-5 * abs(ref.item())
        np.testing.assert_allclose(dl.cpu().numpy(), l64.grad.float().numpy(), rtol=1e-4, atol=1e-9)


def test_cka_bce_pair_ordered_equals_the_two_halves(device):
    """_CkaBcePair under the knob: the same two ordered launches as _CkaBce on the two halves, bit for bit"""
    from scan_amd import ops
    g = torch.Generator().manual_seed(45)
    M, m, cf = 40000, 26000, 8
    logits = torch.randn(M, cf, generator=g) * 2
    ad = torch.softmax(torch.randn(M, cf + 1, generator=g), 1).to(device)
    lp, lh = _leaf(logits, device), _leaf(logits, device)
    with deterministic(True):
        ps, pt = ops.cka_bce_pair(lp, ad, m, cf)
        (ps + 2 * pt).backward()
        hs = ops.cka_bce(lh[:m], ad[:m], 1.0, cf)
        ht = ops.cka_bce(lh[m:], ad[m:], 0.0, cf)
        (hs + 2 * ht).backward()
    assert torch.equal(ps, hs) and torch.equal(pt, ht) and torch.equal(lp.grad, lh.grad)


@pytest.mark.parametrize("M", SIZES)
def test_softmax_focal_mean_ordered(device, M):
    from scan_amd import ops
    g = torch.Generator().manual_seed(50 + M)
    z = torch.randn(M, 9, generator=g) * 2
    lab = torch.randint(0, 9, (M,), generator=g)
    zd, labd = _leaf(z, device), lab.to(device)

    def run():
        zd.grad = None
        loss = ops.softmax_focal_loss_mean(zd, labd, 2.0)
        loss.backward()
        return loss, zd.grad

    (v, dz), (v0, dz0) = _repeat_equal(device, run, _repeats_for(M))
    ref = _sfl64(z, lab, 2.0).item()
    print("sfl M=%d ordered %.9g default %.9g fp64 %.9g" % (M, v.item(), v0.item(), ref))
    # test_softmax_focal_golden: abs(l - ref) <= 1e-5 * abs(ref); gradient rtol 1e-4 / atol 1e-8
    assert abs(v.item() - v0.item()) <= 1e-5 * abs(ref) and abs(v.item() - ref) <= 1e-5 * abs(ref)
    np.testing.assert_allclose(dz.cpu().numpy(), dz0.cpu().numpy(), rtol=1e-4, atol=1e-8)


# ----------------------------------------------------------------------------- GroupNorm + ReLU
def _pyr(levels, dev):
    from scan_amd import ops
    rows, sizes = [], []
    for x in levels:
        r, s = ops.nchw_to_rows(x.to(dev), None)
        rows.append(r)
        sizes.append(s.sizes[0])
    return torch.cat(rows, 0).contiguous(), ops.PyramidShape(levels[0].shape[0], sizes)


def _unrows(rows, shape, c):
    from scan_amd import ops
    return [ops.rows_to_nchw(rows.detach(), shape, l, c).contiguous().cpu() for l in range(shape.n_levels)]


# two images; 64x96 = 24 whole 256-row chunks per image beside a one-chunk level (50 workgroups); 33x17 = 561 rows = two
# chunks and a ragged third of 49 rows, beside a one-chunk level; a pyramid that is ONE workgroup (one image, 5x7)
@pytest.mark.parametrize("N,sizes", [(2, [(64, 96), (7, 5)]), (2, [(33, 17), (5, 7)]), (1, [(5, 7)])])
def test_groupnorm_relu_ordered(device, N, sizes):
    from scan_amd import ops
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(N, 256, h, w, generator=g) * 2 + 0.5 for h, w in sizes]
    gamma = 1 + 0.1 * torch.randn(256, generator=g)
    beta = 0.1 * torch.randn(256, generator=g)
    gys = [torch.randn(x.shape, generator=g) for x in xs]
    rows, shape = _pyr(xs, device)
    rows.requires_grad_(True)
    gy_rows, _ = _pyr(gys, device)
    gd, bd = _leaf(gamma, device), _leaf(beta, device)

    def run():
        rows.grad = gd.grad = bd.grad = None
        y = ops.groupnorm_relu(rows, gd, bd, shape)
        y.backward(gy_rows)
        return y, rows.grad, gd.grad, bd.grad

    (y, dx, dg, db), (y0, dx0, dg0, db0) = _repeat_equal(device, run, REPEATS if sizes[0] == (64, 96) else 3)
    x64 = [x.double().requires_grad_(True) for x in xs]
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y64 = [F.relu(F.group_norm(x, 32, g64, b64)) for x in x64]
    sum((a * gy.double()).sum() for a, gy in zip(y64, gys)).backward()
    # test_groupnorm_relu: y rtol 1e-4 / atol 1e-5; dx rtol 1e-3 / atol 2e-5; dgamma, dbeta rtol 1e-4 / atol 1e-4
    for got, other in ((y, y0), (dx, dx0)):
        tol = dict(rtol=1e-4, atol=1e-5) if got is y else dict(rtol=1e-3, atol=2e-5)
        for a, b in zip(_unrows(got, shape, 256), _unrows(other, shape, 256)):
            np.testing.assert_allclose(a.numpy(), b.numpy(), **tol)
    for a, b in zip(_unrows(y, shape, 256), y64):
        np.testing.assert_allclose(a.numpy(), b.detach().float().numpy(), rtol=1e-4, atol=1e-5)
    for a, b in zip(_unrows(dx, shape, 256), x64):
        np.testing.assert_allclose(a.numpy(), b.grad.float().numpy(), rtol=1e-3, atol=2e-5)
    for got, other, ref in ((dg, dg0, g64.grad), (db, db0, b64.grad)):
        np.testing.assert_allclose(got.cpu().numpy(), other.cpu().numpy(), rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(got.cpu().numpy(), ref.float().numpy(), rtol=1e-4, atol=1e-4)


def test_groupnorm_ordered_accumulates_into_existing_gradients(device):
    """accumulate bit 0 of the ordered backward (the flat-gradient-buffer path of the trainer): dgamma / dbeta are added to"""
    from scan_amd import _lib, ops
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 256, 20, 30, generator=g)
    rows, shape = _pyr([x], device)
    gy = torch.randn(rows.shape, generator=g).to(device)
    gamma, beta = (1 + 0.1 * torch.randn(256, generator=g)).to(device), (0.1 * torch.randn(256, generator=g)).to(device)
    P, st = ops._ptr, ops._stream
    stats = torch.empty(2 * 32 * 2, device=device)
    ws = torch.empty(_lib.query("scan_groupnorm_ordered_ws_floats", shape.ref(), 256, 32) // 2 + 1, dtype=torch.float64, device=device)
    _lib.call("scan_groupnorm_stats_ordered", P(rows), shape.ref(), 256, 32, 1e-5, P(stats), P(ws), st())
    out = []
    for acc in (0, 1):
        dx, dg, db = torch.empty_like(rows), torch.full((256,), 3.0, device=device), torch.full((256,), -2.0, device=device)
        _lib.call("scan_groupnorm_relu_backward_ordered", P(rows), P(beta), P(gy), shape.ref(), 256, 32, P(stats), P(gamma), 1, P(dx),
                  P(dg), P(db), acc, P(ws), st())
        out.append((dx, dg, db))
    assert torch.equal(out[0][0], out[1][0])
    assert torch.equal(out[1][1], out[0][1] + 3.0) and torch.equal(out[1][2], out[0][2] - 2.0)


# ----------------------------------------------------------------------------- conv3x3 + GroupNorm + ReLU, compiled path
@pytest.fixture(scope="module")
def tower_case():
    """the tower block on 4 images of 32x32 (16 GroupNorm workgroups) with its float64 torch.nn result, computed once"""
    torch.manual_seed(7)
    conv, gn = torch.nn.Conv2d(256, 256, 3, 1, 1), torch.nn.GroupNorm(32, 256)
    with torch.no_grad():
        gn.weight.uniform_(0.5, 1.5)
        gn.bias.normal_(0, 0.2)
    x, gy = torch.randn(4, 256, 32, 32), torch.randn(4, 256, 32, 32)
    c64, g64 = copy.deepcopy(conv).double(), copy.deepcopy(gn).double()
    x64 = x.double().requires_grad_(True)
    y64 = F.relu(g64(c64(x64)))
    y64.backward(gy.double())
    refs = [t.detach().float() for t in (y64, x64.grad, c64.weight.grad, c64.bias.grad, g64.weight.grad, g64.bias.grad)]
    return conv, gn, x, gy, refs


def _tower(device, case, path):
    from scan_amd import layers as L
    from scan_amd import ops
    conv, gn, x, gy, _ = case
    c, g = copy.deepcopy(conv).to(device), copy.deepcopy(gn).to(device)
    c.weight.data = c.weight.data.contiguous(memory_format=torch.channels_last)
    xm = x.to(device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    if path == "fused":
        y = L._ops.conv3x3_gn_relu(xm, c.weight, c.bias, g.weight, g.bias, g.eps, True)
    elif path == "pair":
        y = L._ops.group_norm_relu(L._ops.conv2d(xm, c.weight, c.bias, 1, False), g.weight, g.bias, g.eps, True)
    else:
        rows, shape, _ = L._to_rows(xm)
        y = L._to_nchw(ops.groupnorm_relu(ops.conv2d(rows, c.weight, c.bias, shape, 3, 1, gn_sums=True), g.weight, g.bias, shape,
                                          relu=True, eps=g.eps), shape, 256)
    y.backward(gy.to(device))
    return [t.detach() for t in (y, xm.grad, c.weight.grad, c.bias.grad, g.weight.grad, g.bias.grad)]


def test_conv3x3_gn_relu_ordered(device, tower_case):
    """the fused tower block under the knob: no epilogue sums, statistics from the ordered kernel.  The compiled operator, the
    compiled unfused pair and the Python path are bit-identical to each other (what test_compiled_ops_cpp_autograd_equals_python_
    path_and_torch asserts for the default) and repeatable; against the default and float64 torch.nn they keep that test's
    bar: rtol 1e-3, atol 3e-4 * max |reference|."""
    from scan_amd import layers as L
    assert L.OPS_BACKEND == "compiled", "scan_amd/ext/scan_ops/_ops is missing: __graft_entry__.build() builds it"
    first, default = _repeat_equal(device, lambda: _tower(device, tower_case, "fused"), REPEATS)
    with deterministic(True):
        pair, python = _tower(device, tower_case, "pair"), _tower(device, tower_case, "python")
    for a, b, c in zip(first, pair, python):
        assert torch.equal(a, b) and torch.equal(a, c)
    for i, (a, d, r) in enumerate(zip(first, default, tower_case[4])):
        tol = dict(rtol=1e-3, atol=3e-4 * float(r.abs().max()), err_msg=str(i))
        np.testing.assert_allclose(a.cpu().numpy(), d.cpu().numpy(), **tol)
        np.testing.assert_allclose(a.cpu().numpy(), r.numpy(), **tol)


def test_compiled_group_norm_relu_ordered_equals_python_path(device):
    from scan_amd import layers as L
    from scan_amd import ops
    assert L.OPS_BACKEND == "compiled"
    torch.manual_seed(8)
    x, gy = torch.randn(2, 256, 64, 96), torch.randn(2, 256, 64, 96)
    gamma, beta = torch.rand(256) + 0.5, torch.randn(256) * 0.2
    out = []
    with deterministic(True):
        for path in ("cpp", "py"):
            xm = x.to(device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
            gd, bd = _leaf(gamma, device), _leaf(beta, device)
            if path == "cpp":
                y = L._ops.group_norm_relu(xm, gd, bd, 1e-5, True)
            else:
                rows, shape, c = L._to_rows(xm)
                y = L._to_nchw(ops.groupnorm_relu(rows, gd, bd, shape, relu=True, eps=1e-5), shape, c)
            y.backward(gy.to(device))
            out.append((y.detach(), xm.grad, gd.grad, bd.grad))
    for a, b in zip(*out):
        assert torch.equal(a, b)


# ----------------------------------------------------------------------------- a whole training step
def _two_iterations(device, overlap):
    """the run of test_stream_overlap_is_race_free: 2 + 2 frames of 256x512, procedural weights, two iterations"""
    from scan_amd import engine, synth
    model = engine.build_model(9, device=device, attn_dropout=0.0)
    engine.load_procedural_weights(model)
    trainer = engine.Trainer(model)
    if not overlap:
        trainer.dis_streams = {}
        trainer.overlap_target = False
    imgs_s = synth.synth_images(2, 256, 512, 11).to(device)
    imgs_t = synth.synth_images(2, 256, 512, 12).to(device)
    tg = synth.synth_targets(2, 256, 512, 8, 8, 13)
    for _ in range(2):
        losses = trainer.step(imgs_s, tg, imgs_t)
    torch.cuda.synchronize()
    return {k: g.flat_p.clone() for k, g in trainer.groups.items()}, {k: float(v.detach()) if torch.is_tensor(v) else float(v) for k, v in losses.items()}


@pytest.fixture(scope="module")
def step_runs(device):
    """two serial and two overlapped runs under the knob and one default run, shared by the tests below"""
    runs = {}
    with deterministic(True):
        for name, overlap in (("serial_a", False), ("serial_b", False), ("overlap_a", True), ("overlap_b", True)):
            runs[name] = _two_iterations(device, overlap)
    with deterministic(False):
        runs["default"] = _two_iterations(device, False)
    return runs


def _assert_same_parameters(a, b, what):
    assert a[0].keys() == b[0].keys()
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]), "%s: group %s differs by %g" % (what, k, (a[0][k] - b[0][k]).abs().max().item())
    assert a[1] == b[1], what


def test_step_serial_runs_are_bit_identical(step_runs):
    _assert_same_parameters(step_runs["serial_a"], step_runs["serial_b"], "serial vs serial")


def test_step_overlapped_runs_are_bit_identical(step_runs):
    _assert_same_parameters(step_runs["overlap_a"], step_runs["overlap_b"], "overlapped vs overlapped")


def test_step_serial_equals_overlapped_bit_for_bit(step_runs):
    """with the reduction order fixed, the side-stream schedule has no excuse left: any difference is a missed dependency"""
    _assert_same_parameters(step_runs["serial_a"], step_runs["overlap_a"], "serial vs overlapped")


def test_step_losses_agree_with_the_default_path(step_runs):
    """the mode changes summation orders only: the losses of the second iteration agree with a default run within 1e-5
    relative (the default's own run-to-run noise, 3e-7 in the parameters, amplified by nothing)"""
    det, dflt = step_runs["serial_a"][1], step_runs["default"][1]
    assert det.keys() == dflt.keys() and len(det) == 16, sorted(det)
    for k, ref in dflt.items():
        print("%s deterministic %.9g default %.9g" % (k, det[k], ref))
        assert abs(det[k] - ref) <= 1e-5 * abs(ref), (k, det[k], ref)

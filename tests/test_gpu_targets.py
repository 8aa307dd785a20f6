"""The ground-truth plan kernels (scan_amd/csrc/targets.hip: scan_fcos_assign / _compact / _nodes) against the host oracle of
tests/targets_ref.py, bit for bit: at ties, at the boundary equalities, without positives, with an image without boxes, on short
pyramids, through both upload paths, and with every output followed by guard elements that must stay as they were."""
import ctypes

import numpy as np
import pytest
import torch

import atss_ref
import targets_ref as R

pytestmark = pytest.mark.gpu
GUARD = 64


def _guarded(n, dtype, fill, device):
    """a buffer of n elements followed by GUARD more, all holding ``fill``"""
    return torch.full((n + GUARD,), fill, dtype=dtype, device=device)


def _bits(t):
    t = t.cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(got, want):
    """bit-identical (fp32 compared as int32 words: NaN == NaN, -0 != 0)"""
    got, want = _bits(got), _bits(want)
    return got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want)


def _untouched(buf, n, fill):
    return _same(buf[n:], torch.full((GUARD,), fill, dtype=buf.dtype))


def _shape(case):
    from scan_amd import ops
    return ops.PyramidShape(case.N, case.sizes)


# ----------------------------------------------------------------------------- 1. scan_fcos_assign through the C ABI
@pytest.mark.parametrize("name", R.CASES)
def test_assign_c_abi(device, name):
    from scan_amd import ops
    c = R.case(name)
    shape, M, L = _shape(c), c.shape.rows, c.shape.n_levels
    boxes = torch.from_numpy(c.boxes).to(device)
    glab = torch.from_numpy(c.glabels).to(device)
    ng = torch.from_numpy(c.ng).to(device)
    labels = _guarded(M, torch.int64, -7, device)
    labels_i32 = _guarded(M, torch.int32, -7, device)
    reg = _guarded(4 * M, torch.float32, float("nan"), device)
    level_pos = _guarded(5, torch.int32, 12345, device)  # [SCAN_MAX_LEVELS] counters whatever the pyramid's depth
    strides = (ctypes.c_int32 * L)(*c.strides)
    soi = (ctypes.c_float * (2 * L))(*[float(v) for pair in c.soi for v in pair])
    ops.call("scan_fcos_assign", shape.ref(), strides, soi, ops._ptr(boxes), ops._ptr(glab), ops._ptr(ng), c.G, ops._ptr(labels),
             ops._ptr(labels_i32), ops._ptr(reg), ops._ptr(level_pos), ops._stream())
    torch.cuda.synchronize()
    assert _untouched(labels, M, -7) and _untouched(labels_i32, M, -7) and _untouched(reg, 4 * M, float("nan"))
    assert _untouched(level_pos, 5, 12345)
    assert _same(labels[:M], c.labels)
    assert _same(labels_i32[:M], c.labels.astype(np.int32))
    assert _same(reg[:4 * M].view(M, 4), c.reg)  # every row, background rows too
    assert level_pos[:L].tolist() == c.counts["level_pos"]
    if name == "ragged_with_empty_image":
        assert not bool((labels[:M] == 999).any()) and not bool(torch.isnan(reg[:4 * M]).any())  # no padded slot was read
        for l, (h, w) in enumerate(c.sizes):  # the image without boxes
            r0 = shape.row_off[l] + h * w
            assert not bool(labels[r0:r0 + h * w].any()) and _same(reg[4 * r0:4 * (r0 + h * w)], np.zeros((4 * h * w,), np.float32))


# ----------------------------------------------------------------------------- 2. compaction and node sampling on written labels
def test_compact_and_nodes_synthetic_labels(device):
    from scan_amd import ops
    st = ops._stream()
    for sizes, lab_h, reg_h, names in R.label_cases():
        shape = ops.PyramidShape(1, sizes)
        M, L = shape.rows, shape.n_levels
        labels = torch.from_numpy(lab_h).to(device)
        reg = torch.from_numpy(reg_h).to(device)
        pos_list = _guarded(M, torch.int32, -1, device)
        neg_list = _guarded(M, torch.int32, -1, device)
        ops.call("scan_fcos_compact", shape.ref(), ops._ptr(labels), ops._ptr(pos_list), ops._ptr(neg_list), st)
        want_pos = np.full((M + GUARD,), -1, dtype=np.int32)
        want_neg = np.full((M + GUARD,), -1, dtype=np.int32)
        for l, (p, n) in enumerate(R.compact(lab_h, shape.row_off)):
            want_pos[shape.row_off[l]:shape.row_off[l] + len(p)] = p
            want_neg[shape.row_off[l]:shape.row_off[l] + len(n)] = n
        assert _same(pos_list, want_pos), (sizes, names)  # the lists, and -1 everywhere else (guards included)
        assert _same(neg_list, want_neg), (sizes, names)
        want = R.nodes(lab_h, reg_h, shape.row_off)
        counts = (ctypes.c_int32 * L)(*[int(v) for v in want["level_pos"]])
        n_nodes, n_pos = len(want["node_index"]), len(want["pos_inds"])
        assert ops.query("scan_fcos_nodes_count", shape.ref(), counts) == n_nodes
        if n_nodes == 0:  # the kernel returns before it looks at its outputs
            ops.call("scan_fcos_nodes", shape.ref(), counts, ops._ptr(labels), ops._ptr(reg), ops._ptr(pos_list), ops._ptr(neg_list),
                     None, None, None, None, None, st)
            continue
        node_index = _guarded(n_nodes, torch.int64, -3, device)
        node_labels = _guarded(n_nodes, torch.int64, -3, device)
        pos_inds = _guarded(n_pos, torch.int64, -3, device)
        reg_pos = _guarded(4 * n_pos, torch.float32, float("nan"), device)
        ctr_pos = _guarded(n_pos, torch.float32, float("nan"), device)
        ops.call("scan_fcos_nodes", shape.ref(), counts, ops._ptr(labels), ops._ptr(reg), ops._ptr(pos_list), ops._ptr(neg_list),
                 ops._ptr(node_index), ops._ptr(node_labels), ops._ptr(pos_inds), ops._ptr(reg_pos), ops._ptr(ctr_pos), st)
        torch.cuda.synchronize()
        assert _untouched(node_index, n_nodes, -3) and _untouched(node_labels, n_nodes, -3) and _untouched(pos_inds, n_pos, -3)
        assert _untouched(reg_pos, 4 * n_pos, float("nan")) and _untouched(ctr_pos, n_pos, float("nan"))
        assert _same(node_index[:n_nodes], want["node_index"]), (sizes, names)
        assert _same(node_labels[:n_nodes], want["node_labels"]), (sizes, names)
        assert _same(pos_inds[:n_pos], want["pos_inds"]), (sizes, names)
        assert _same(reg_pos[:4 * n_pos].view(n_pos, 4), want["reg_pos"]), (sizes, names)
        assert _same(ctr_pos[:n_pos], want["ctr_pos"]), (sizes, names)


# ----------------------------------------------------------------------------- 3. the plan, through both upload paths
PLAN_FIELDS = ("labels", "labels_i32", "reg_targets", "pos_inds", "reg_pos", "ctr_pos", "node_index", "node_labels")


def _assert_plan_is_the_oracle(plan, c):
    assert _same(plan.labels, c.labels) and _same(plan.labels_i32, c.labels.astype(np.int32))
    assert _same(plan.reg_targets, c.reg)
    assert plan.n_pos == sum(c.counts["level_pos"])
    for k in ("pos_inds", "reg_pos", "node_index", "node_labels"):
        assert _same(getattr(plan, k), c.nodes[k]), k
    assert (plan.ctr_pos is None) == (plan.n_pos == 0)
    if plan.n_pos:
        assert _same(plan.ctr_pos, c.nodes["ctr_pos"])


def _assert_plans_identical(a, b):
    assert a.n_pos == b.n_pos
    for k in PLAN_FIELDS:
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None and y is None) or _same(x, y), k


@pytest.mark.parametrize("name", R.PLAN_CASES)
def test_plan_on_edge_cases(device, name):
    from scan_amd.modeling import fcos
    c = R.case(name)
    on_device = fcos._build_plan_device(_shape(c), c.torch_targets(device), device)
    from_host = fcos._build_plan_device(_shape(c), c.torch_targets(), device)  # pinned staging buffers, G padded to a power of two
    torch.cuda.synchronize()
    _assert_plan_is_the_oracle(on_device, c)
    _assert_plan_is_the_oracle(from_host, c)
    _assert_plans_identical(on_device, from_host)


def test_staging_grows_and_is_rezeroed(device):
    """host targets of one batch size: 3 boxes per image (buffers of 16 slots), then 20 (re-allocated at 32), then the first
    batch again in the grown buffers, whose slots 3..19 held the second batch's boxes"""
    from scan_amd.modeling import fcos
    small = R.case_from_targets("small", 128, 256, [(b[:3], l[:3]) for b, l in R.integer_grid_targets(2, 6)])
    large = R.case_from_targets("large", 128, 256, R.integer_grid_targets(2, 20, seed=8))
    assert list(small.ng) == [3, 3] and list(large.ng) == [20, 20] and sum(large.counts["level_pos"]) > sum(small.counts["level_pos"]) > 0
    key = (2, str(device))
    fcos._plan_staging.pop(key, None)
    try:
        plans = []
        for c, slots in ((small, 16), (large, 32), (small, 32)):
            plans.append(fcos._build_plan_device(_shape(c), c.torch_targets(), device))
            torch.cuda.synchronize()
            assert fcos._plan_staging[key][0].shape == (2, slots, 4) and fcos._plan_staging[key][0].is_pinned()
            _assert_plan_is_the_oracle(plans[-1], c)
        _assert_plans_identical(plans[0], plans[2])
    finally:
        fcos._plan_staging.pop(key, None)


# ----------------------------------------------------------------------------- 4. the loss without a positive location
def test_fcos_loss_without_positives(device):
    """the FCOS twin of test_gpu_atss.py::test_loss_without_positives_takes_the_sum_fallbacks (modeling/fcos.py: the branch of
    FCOSLossComputation for n_pos == 0): class loss = the fp64 focal sum over all-background labels / (0 + N) within the 1e-4
    relative bound of that test, the other two losses and their gradients exactly zero"""
    from scan_amd.modeling import fcos
    c = R.case("zero_positives")
    assert sum(c.counts["level_pos"]) == 0
    shape, M, C = _shape(c), c.shape.rows, 8
    fcos.reset_target_plan()
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(M, C, generator=g) - 2).to(device).requires_grad_(True)
    reg = torch.randn(M, 4, generator=g).exp().to(device).requires_grad_(True)
    ctr = torch.randn(M, generator=g).to(device).requires_grad_(True)
    try:
        lc, lr, lctr = fcos.FCOSLossComputation()(shape, logits, reg, ctr, c.torch_targets())
        ref = float(atss_ref.focal_sum(logits.detach().cpu().double(), torch.zeros(M, dtype=torch.int64), 2.0, 0.25)) / (0 + c.N)
        got = float(lc.detach())
        print("class loss %.9g, fp64 %.9g, relative error %.3g" % (got, ref, abs(got - ref) / ref))
        assert abs(got - ref) <= 1e-4 * ref
        assert float(lr.detach()) == 0.0 and float(lctr.detach()) == 0.0
        (lc + lr + lctr).backward()
    finally:
        fcos.reset_target_plan()
    assert float(reg.grad.abs().max()) == 0.0 and float(ctr.grad.abs().max()) == 0.0
    assert bool(torch.isfinite(logits.grad).all()) and float(logits.grad.abs().max()) > 0.0

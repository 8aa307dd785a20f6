"""CPU tests (no GPU) of the deterministic mode's C ABI: the scan_tune knob "deterministic" and the *_ordered entry points
(include/scan_hip.h).  The kernels themselves are tested on the GPU in tests/test_gpu_deterministic.py."""
import os
import re

from scan_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ORDERED = ["scan_sigmoid_focal_loss_forward_ordered", "scan_iou_loss_forward_ordered", "scan_bce_logits_forward_ordered",
           "scan_cka_bce_forward_ordered", "scan_cka_bce_forward_loss_ordered", "scan_softmax_focal_forward_ordered",
           "scan_groupnorm_stats_ordered", "scan_groupnorm_relu_backward_ordered", "scan_groupnorm_relu_backward_ld_ordered"]


def test_library_exports_every_ordered_symbol_the_header_declares():
    hdr = open(os.path.join(ROOT, "include", "scan_hip.h")).read()
    declared = sorted(n for n in set(re.findall(r"\b(scan_[a-z0-9_]+)\s*\(", hdr)) if "_ordered" in n)
    assert set(ORDERED) <= set(declared), set(ORDERED) - set(declared)
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name), "libscan_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES, name
    # every ordered entry point has a workspace-size query, as the header's other workspace-taking entry points have
    for q in ("scan_sigmoid_focal_loss_ordered_ws_floats", "scan_iou_loss_ordered_ws_floats", "scan_bce_logits_ordered_ws_floats",
              "scan_cka_bce_ordered_ws_floats", "scan_softmax_focal_ordered_ws_floats", "scan_groupnorm_ordered_ws_floats"):
        assert q in declared, q


def test_deterministic_knob_defaults_to_off_and_round_trips():
    L = _lib.lib()
    assert L.scan_tune_default(b"deterministic") == 0
    old = L.scan_tune_get(b"deterministic")
    assert old != _lib.TUNE_UNKNOWN
    try:
        assert L.scan_tune(b"deterministic", 1) == old
        assert L.scan_tune_get(b"deterministic") == 1
        assert _lib.lib_identity()["scan_tune_non_default"].get("deterministic") == 1  # what bench.py stamps into its line
        assert L.scan_tune(b"deterministic", 0) == 1
        assert L.scan_tune_get(b"deterministic") == 0
        assert L.scan_tune_default(b"deterministic") == 0  # the default is what the library was built with, not the last value
    finally:
        L.scan_tune(b"deterministic", old)


def test_ops_reads_the_library_knob_at_call_time():
    """ops.deterministic() / ops.set_deterministic() are views of the library's knob, not a copy taken at import"""
    from scan_amd import ops
    L = _lib.lib()
    old = L.scan_tune_get(b"deterministic")
    try:
        L.scan_tune(b"deterministic", 0)
        assert ops.deterministic() is False
        assert ops.set_deterministic(True) is False and L.scan_tune_get(b"deterministic") == 1 and ops.deterministic() is True
        L.scan_tune(b"deterministic", 0)  # behind ops' back
        assert ops.deterministic() is False
        assert ops.set_deterministic(True) is False and ops.set_deterministic(False) is True
    finally:
        L.scan_tune(b"deterministic", old)


def test_ordered_workspace_sizes_cover_the_launch_grids():
    """one slot per workgroup and output column, under the current "reduce_blocks" (grid_reduce: one workgroup per 2,048 work
    items, capped), never zero for a non-empty input"""
    L = _lib.lib()
    assert L.scan_tune_get(b"reduce_blocks") == 2048
    assert L.scan_sigmoid_focal_loss_ordered_ws_floats(40000, 8) == 40  # 80,000 float4
    assert L.scan_sigmoid_focal_loss_ordered_ws_floats(1, 8) == 1
    assert L.scan_sigmoid_focal_loss_ordered_ws_floats(1 << 24, 8) == 2048
    assert L.scan_iou_loss_ordered_ws_floats(40000) == 2 * 20
    assert L.scan_iou_loss_ordered_ws_floats(1 << 24) == 2 * 1024  # a "light" kernel: half the cap
    assert L.scan_bce_logits_ordered_ws_floats(320000) == 2 * 157
    assert L.scan_cka_bce_ordered_ws_floats(40000, 8) == 16 * 40  # the float4 form: 80,000 half rows
    assert L.scan_cka_bce_ordered_ws_floats(40000, 3) == 6 * 20
    assert L.scan_softmax_focal_ordered_ws_floats(40000) == 79  # 512 rows per workgroup iteration
    assert L.scan_softmax_focal_ordered_ws_floats(1) == 1
    # the queries follow the knob: the cap itself, half of it for the "light" kernels, each clamped to one workgroup
    for cap, focal, iou, bce, cka8, cka3 in ((2, 2, 2 * 1, 2 * 2, 16 * 2, 6 * 2), (0, 1, 2 * 1, 2 * 1, 16 * 1, 6 * 1)):
        old = L.scan_tune(b"reduce_blocks", cap)
        try:
            assert L.scan_sigmoid_focal_loss_ordered_ws_floats(1 << 24, 8) == focal
            assert L.scan_iou_loss_ordered_ws_floats(1 << 24) == iou
            assert L.scan_bce_logits_ordered_ws_floats(320000) == bce
            assert L.scan_cka_bce_ordered_ws_floats(40000, 8) == cka8  # the larger of the generic and the light float4 grid
            assert L.scan_cka_bce_ordered_ws_floats(40000, 3) == cka3
            assert L.scan_softmax_focal_ordered_ws_floats(40000) == 79  # the knob does not reach this kernel's grid
        finally:
            L.scan_tune(b"reduce_blocks", old)
    assert L.scan_tune_get(b"reduce_blocks") == 2048
    d = _lib.PyramidDesc()
    d.n_levels, d.n_images = 2, 2
    d.h[0], d.w[0], d.h[1], d.w[1] = 64, 96, 7, 5
    d.row_off[0], d.row_off[1], d.row_off[2] = 0, 2 * 64 * 96, 2 * 64 * 96 + 2 * 35
    nblk = 2 * 24 + 2 * 1  # 256-row chunks
    assert L.scan_groupnorm_ordered_ws_floats(d, 256, 32) == 2 * (nblk * 32 * 2 + nblk * 256 * 2)


def test_ordered_entry_points_validate_arguments_without_a_device():
    L = _lib.lib()
    assert L.scan_sigmoid_focal_loss_forward_ordered(None, None, 4, 8, 2.0, 0.25, None, None, None, None) == -1
    assert b"loss_sum and ws" in L.scan_last_error()
    assert L.scan_iou_loss_forward_ordered(None, None, None, 4, None, None, None) == -1
    assert L.scan_bce_logits_forward_ordered(None, None, 0.0, None, 0, 4, None, None, None) == -1
    assert L.scan_cka_bce_forward_loss_ordered(None, None, 0, 8, 1.0, None, None, None) == -1
    assert L.scan_softmax_focal_forward_ordered(None, None, 4, 17, 2.0, None, None, None) == -1
    d = _lib.PyramidDesc()
    d.n_levels, d.n_images = 1, 1
    d.h[0], d.w[0] = 4, 4
    d.row_off[1] = 16
    assert L.scan_groupnorm_stats_ordered(None, d, 128, 32, 1e-5, None, None, None) == -1
    assert b"C=256" in L.scan_last_error()
    assert L.scan_groupnorm_relu_backward_ordered(None, None, None, d, 256, 32, None, None, 1, None, None, None, 0, None, None) == -1

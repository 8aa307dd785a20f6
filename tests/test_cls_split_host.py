"""Host arithmetic behind ops.CLS_SPLIT (no GPU): the plans the library makes for the three launches of the class branches'
first conv on 256 feature channels at the headline size (P3, 4 frames = 131,072 rows), set against the plans of the dense
264-channel conv over cat(x, act[1:]) it replaces, and the ABI of the new entry points."""
import ctypes
import os

from scan_amd import _lib, ops

ROWS = ops.PyramidShape(4, [(128, 256)])
WINO = 1  # SCAN_CONV_WINO3X3


def _conv_plan(dgrad, cs):
    p = _lib.ConvPlan()
    _lib.call("scan_conv_plan", 3, 9, dgrad, 1024, cs, 1024 if dgrad else cs, ROWS.ref(), 0, ctypes.byref(p))
    return p


def _wgrad_plan(cs):
    w = _lib.WgradPlan()
    _lib.call("scan_conv_wgrad_plan", 3, 3, 1, cs, 1024, ROWS.ref(), ROWS.ref(), ctypes.byref(w))
    return w


def test_main_conv_plans_on_256_channels():
    assert ROWS.rows == 131072
    fwd, dgrad, wgrad = _conv_plan(0, 256), _conv_plan(1, 256), _wgrad_plan(256)
    assert fwd.family == WINO and fwd.csw == 256
    assert dgrad.family == WINO and dgrad.nout == 256 and dgrad.rem == 0
    assert wgrad.c_tiles == 2


def test_dense_264_channel_plans_pay_a_whole_extra_tile():
    """what the split removes: a ninth 32-channel chunk forward, the remainder rule (direct kernel + a remainder launch) in the
    data gradient, a third channel tile in the weight gradient"""
    fwd, dgrad, wgrad = _conv_plan(0, 264), _conv_plan(1, 264), _wgrad_plan(264)
    assert fwd.csw == 288
    assert dgrad.family != WINO and dgrad.rem == 8
    assert wgrad.c_tiles == 3


def test_new_entry_points_are_declared_and_exported():
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "scan_hip.h")).read()
    L = _lib.lib()
    for name in ("scan_cka_stack_weights_split", "scan_cka_unstack_grads_split", "scan_gconv3x3_to1_act_ws_floats",
                 "scan_gconv3x3_to1_act_forward", "scan_gconv3x3_to1_act_backward", "scan_gconv3x3_to1_act_grads",
                 "scan_gconv3x3_to1_act_backward_all"):
        assert name + "(" in hdr and name in _lib.SIGNATURES and hasattr(L, name), name


def test_gconv_workspace_sizes():
    """tap sums [M][G][9]; a slab = 1024 partials + 32 run sums of 9 * G * 128.  The plain entry points use one or the other,
    scan_gconv3x3_to1_act_backward_all the tap sums and two slabs at once."""
    slab = 1056 * 9 * 128
    for shape in (ops.PyramidShape(2, [(17, 17)]), ops.PyramidShape(2, [(5, 7), (3, 4)]), ROWS):
        M = shape.rows
        for G in (1, 8, 31):
            assert _lib.query("scan_gconv3x3_to1_ws_floats", shape.ref(), G, 128) == max(9 * M * G, slab * G), (M, G)
            assert _lib.query("scan_gconv3x3_to1_act_ws_floats", shape.ref(), G, 128) == 9 * M * G + 2 * slab * G, (M, G)

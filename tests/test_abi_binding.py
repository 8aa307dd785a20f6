"""The ctypes binding is derived from include/scan_hip.h (scan_amd/_lib.py): struct layouts against the compiler, one pinned
signature of every kind, the constants, the parser's refusals, and the argument checks of the head-plan wrappers in scan_amd/ops.py.
No device."""
import ctypes
import os
import subprocess

import pytest
import torch

from scan_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"scan_pyramid_t": _lib.PyramidDesc, "scan_sgd_segment_t": _lib.SgdSegment, "scan_cka_branch_t": _lib.CkaBranch,
           "scan_level_t": _lib.LevelDesc, "scan_conv_plan_t": _lib.ConvPlan, "scan_conv_wgrad_plan_t": _lib.WgradPlan,
           "scan_groupnorm_plan_t": _lib.GroupNormPlan}


# ----------------------------------------------------------------------------- 1. struct layout against the compiler
@pytest.mark.parametrize("c_name", sorted(STRUCTS))
def test_struct_layout_is_the_compilers(c_name, tmp_path):
    cls = STRUCTS[c_name]
    assert cls.__doc__ == c_name and len(cls._fields_) > 0
    lines = ['#include <cstddef>', '#include "scan_hip.h"',
             'static_assert(sizeof(%s) == %d, "sizeof %s");' % (c_name, ctypes.sizeof(cls), c_name)]
    for field, t in cls._fields_:
        lines.append('static_assert(offsetof(%s, %s) == %d, "offsetof %s.%s");'
                     % (c_name, field, getattr(cls, field).offset, c_name, field))
        lines.append('static_assert(sizeof(((%s*)0)->%s) == %d, "sizeof %s.%s");' % (c_name, field, ctypes.sizeof(t), c_name, field))
    src = tmp_path / (c_name + ".cpp")
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ----------------------------------------------------------------------------- 2. pinned signatures
i32, i64, u32, f32, f64, vp, cp = (ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_float, ctypes.c_double,
                                   ctypes.c_void_p, ctypes.c_char_p)
PD, CP, WP, GP = (ctypes.POINTER(c) for c in (_lib.PyramidDesc, _lib.ConvPlan, _lib.WgradPlan, _lib.GroupNormPlan))
SEG, BR, LV = (ctypes.POINTER(c) for c in (_lib.SgdSegment, _lib.CkaBranch, _lib.LevelDesc))
PINNED = {
    "scan_last_error": (cp, []),
    "scan_tune": (ctypes.c_int, [cp, ctypes.c_int]),
    "scan_nms_ws_bytes": (i64, [i64]),
    "scan_rpn_sample": (ctypes.c_int, [PD, i32, vp, i32, i32, u32, vp, vp, vp, vp]),
    "scan_mfma_sustained_bf16": (ctypes.c_int, [f64, i32, vp, vp]),
    "scan_conv_run": (ctypes.c_int, [CP, vp, PD, i32, vp, vp, vp, vp, vp, vp, PD, i32, i32, i32, vp, i32, vp]),
    "scan_conv_wgrad_plan": (ctypes.c_int, [i32, i32, i32, i32, i32, PD, PD, WP]),
    "scan_groupnorm_plan": (ctypes.c_int, [PD, i32, i32, i32, GP]),
    "scan_sgd_momentum_multi": (ctypes.c_int, [SEG, i32, f32, vp]),
    "scan_cka_stack_weights": (ctypes.c_int, [BR, i32, i32, i32, i64, i64, i64, i64, i64, i32, i32, vp, vp, vp, vp, vp]),
    "scan_pyramid_pack": (ctypes.c_int, [LV, i32, i32, i32, vp, i32, vp]),
    "scan_roi_align_forward": (ctypes.c_int, [vp, PD, i32, i32, vp, vp, vp, i64, i32, i32, i32, vp, vp]),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_signature(name):
    res, args = _lib.SIGNATURES[name]
    assert res is PINNED[name][0], (name, res)
    assert len(args) == len(PINNED[name][1]) and all(a is b for a, b in zip(args, PINNED[name][1])), (name, args)


# ----------------------------------------------------------------------------- 3. constants
def test_constants_come_from_the_header():
    assert _lib.TUNE_UNKNOWN == -2 ** 31
    assert _lib.MAX_LEVELS == 5
    assert _lib.NMS_MAX == 262144
    assert (_lib.WGRAD_FP32, _lib.WGRAD_V4, _lib.WGRAD_V6_64X32, _lib.WGRAD_V6_32X64, _lib.WGRAD_V6_32X64_WINO) == (0, 1, 2, 3, 4)
    assert len(_lib.PyramidDesc().row_off) == 6
    assert not hasattr(_lib, "HIP_H")  # the include guard is no constant


# ----------------------------------------------------------------------------- 4. the parser refuses what it does not know
T_STRUCT = "typedef struct { int32_t a, b[SCAN_N + 1]; const float* p; } scan_t_t;\n"


def test_parser_on_a_small_header():
    consts, structs, sigs = _lib._parse_header(
        "#ifndef SCAN_HIP_H\n#define SCAN_HIP_H\n#define SCAN_N (2 * 3 - 1) /* five */\n" + T_STRUCT
        + "const char* scan_a(void);\nint64_t scan_b(const scan_t_t* t, const int32_t* v,\n  uint32_t k, double x);\n#endif\n",
        {"scan_t_t": "T"})
    assert consts == {"SCAN_N": 5}
    assert [(n, ctypes.sizeof(t)) for n, t in structs["T"]._fields_] == [("a", 4), ("b", 24), ("p", 8)]
    assert sigs == {"scan_a": (cp, []), "scan_b": (i64, [ctypes.POINTER(structs["T"]), vp, u32, f64])}


@pytest.mark.parametrize("text, names, offending", [
    ("int scan_f(const float* x, size_t n);", {}, "size_t n"),
    ("typedef struct { int32_t a; unsigned long b; } scan_t_t;", {"scan_t_t": "T"}, "unsigned long b"),
    ("int scan_f(void (*done)(int), int32_t n);", {}, "(*done)"),
    ("int scan_f(int32_t n) { return n; }", {}, "scan_f"),
    ("#define SCAN_N 5\nint scan_f(int32_t n);", {"scan_t_t": "T"}, "scan_t_t"),
    ("#define SCAN_EPS 1e-5f\n", {}, "1e-5f"),
    ("typedef struct { int32_t a[SCAN_UNSET]; } scan_t_t;", {"scan_t_t": "T"}, "SCAN_UNSET"),
])
def test_parser_fails_loudly(text, names, offending):
    with pytest.raises(ValueError) as e:
        _lib._parse_header(text, names)
    assert offending in str(e.value)


# ----------------------------------------------------------------------------- 5. the head-plan wrappers check before they call
SHAPE = ops.PyramidShape(2, [(8, 12), (4, 6)])


def _ground_truth(G=3):
    return (torch.zeros((2, G, 4)), torch.zeros((2, G), dtype=torch.int64), torch.full((2,), G, dtype=torch.int32))


def _refusals():
    M = SHAPE.rows
    boxes, glab, ng = _ground_truth()
    cells = torch.zeros((2, 3, 4))
    lab64, i32v, reg = torch.zeros((M,), dtype=torch.int64), torch.zeros((M,), dtype=torch.int32), torch.zeros((M, 4))
    soi = ((-1, 64), (64, 128))
    return [
        ("fcos_assign strides", lambda: ops.fcos_assign(SHAPE, (8, 16, 32), soi, boxes, glab, ng)),
        ("fcos_assign sizes of interest", lambda: ops.fcos_assign(SHAPE, (8, 16), soi[:1], boxes, glab, ng)),
        ("fcos_assign labels", lambda: ops.fcos_assign(SHAPE, (8, 16), soi, boxes, glab.int(), ng)),
        ("fcos_nodes counts", lambda: ops.fcos_nodes(SHAPE, [1, 2, 3], lab64, reg, i32v, i32v)),
        ("fcos_nodes count range", lambda: ops.fcos_nodes(SHAPE, [1, 2 * 4 * 6 + 1], lab64, reg, i32v, i32v)),
        ("fcos_nodes labels", lambda: ops.fcos_nodes(SHAPE, [1, 2], i32v, reg, i32v, i32v)),
        ("atss_assign sizes", lambda: ops.atss_assign(SHAPE, (8, 16), (64.,), 9, boxes, glab, ng)),
        ("atss_assign ng", lambda: ops.atss_assign(SHAPE, (8, 16), (64., 128.), 9, boxes, glab, ng.long())),
        ("atss_targets counts", lambda: ops.atss_targets(SHAPE, (8, 16), (64., 128.), [1], boxes, i32v, i32v)),
        ("atss_targets matched", lambda: ops.atss_targets(SHAPE, (8, 16), (64., 128.), [1, 2], boxes, lab64, i32v)),
        ("retina_match strides", lambda: ops.retina_match(SHAPE, (8,), cells, boxes, glab, ng, 0.4, 0.5)),
        ("retina_match labels", lambda: ops.retina_match(SHAPE, (8, 16), cells, boxes, glab.int(), ng, 0.4, 0.5)),
        ("retina_match thresholds", lambda: ops.retina_match(SHAPE, (8, 16), cells, boxes, glab, ng, 0.6, 0.5)),
        ("rpn_labels boxes", lambda: ops.rpn_labels(SHAPE, (8, 16), cells, boxes[:, :, :3], ng,
                                                    torch.zeros((2, 2), dtype=torch.int32), 0.3, 0.7, 0.0)),
        ("paradigm_update_ pb", lambda: ops.paradigm_update_(torch.zeros((9, 256, 5)), torch.zeros((9, 255)), 0)),
        ("paradigm_update_ it", lambda: ops.paradigm_update_(torch.zeros((9, 256, 5)), torch.zeros((9, 256)), 6)),
    ]


@pytest.mark.parametrize("case", [name for name, _ in _refusals()])
def test_wrapper_refuses_before_any_library_call(case, monkeypatch):
    def no_call(name, *args):
        pytest.fail("%s reached the library (%s)" % (case, name))
    monkeypatch.setattr(ops, "call", no_call)
    monkeypatch.setattr(ops, "query", no_call)
    with pytest.raises(ValueError, match=case.split()[0]):
        dict(_refusals())[case]()


def test_level_table_checks_its_length():
    assert list(ops._level_table("t", SHAPE, ctypes.c_int32, (8, 16), "strides")) == [8, 16]
    assert list(ops._level_table("t", SHAPE, ctypes.c_float, (-1, 64, 64, 128), "sizes of interest", per_level=2)) == [-1., 64., 64., 128.]
    with pytest.raises(ValueError, match="t: 3 strides for a pyramid of 2 levels"):
        ops._level_table("t", SHAPE, ctypes.c_int32, (8, 16, 32), "strides")

"""Class counts beyond the two shipped label sets, the parts that need no GPU: the reference fixtures at K = 8 / 21 and the
declarations of the two limits."""
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("K", [8, 21])
def test_step_fixtures_at_other_class_counts_load(gold_dir, K):
    name = "step_k%d_128x256" % K
    gold = json.load(open(os.path.join(gold_dir, name + ".json")))
    base = json.load(open(os.path.join(gold_dir, "step_128x256.json")))
    assert gold["num_classes"] == K and (gold["H"], gold["W"], gold["N"]) == (128, 256, 2)
    assert len(base["losses"]) == 16 and set(gold["losses"]) == set(base["losses"])
    assert all(np.isfinite(v) for v in gold["losses"].values())
    for mk in ("backbone", "fcos", "middle_head") + tuple("dis_P%d_CON" % l for l in range(3, 8)):
        assert gold["grad_digest"][mk], mk
    # one class branch per foreground class
    assert "classifier_cls_%d.2.weight" % (K - 2) in gold["grad_digest"]["dis_P3_CON"]
    assert "classifier_cls_%d.2.weight" % (K - 1) not in gold["grad_digest"]["dis_P3_CON"]
    g = np.load(os.path.join(gold_dir, name + ".npz"))
    assert g["prototype_after"].shape == (K, 256, 3) and g["kernels"].shape == (K, 256)
    assert int(g["node_labels"].max()) <= K - 1


def test_class_count_limits_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "scan_hip.h")).read()
    assert re.search(r"int32_t\s+scan_dynconv_max_classes\(void\);", hdr)
    assert re.search(r"int32_t\s+scan_gconv3x3_to1_max_groups\(void\);", hdr)
    for nm in ("forward", "dgrad", "wgrad", "backward"):
        assert re.search(r"int\s+scan_gconv3x3_to1_any_%s\(" % nm, hdr), nm
    from scan_amd import _lib
    assert _lib.query("scan_dynconv_max_classes") == 32
    assert _lib.query("scan_gconv3x3_to1_max_groups") == 31
    assert _lib.query("scan_tune_get", b"dynconv_generic") == 0 == _lib.query("scan_tune_default", b"dynconv_generic")
    # refused before any device is touched, the range in the message
    for K in (1, 33):
        with pytest.raises(RuntimeError, match=r"only K in 2\.\.32 is built \(got %d\)" % K):
            _lib.call("scan_dynconv_softmax_forward", None, None, 10, 256, K, None, None, None)


def test_gconv_caps_follow_the_group_count_and_the_knob():
    """scan_gconv3x3_to1_caps: 0 for what the entry points refuse, else runnable (1) | lane-mapped (2, G in 1, 2, 4, 8) |
    bit-mask forward / backward taken now (4, lane-mapped and gconv_mfma = 1) | act-term kernels available now (8,
    lane-mapped and gconv_mfma = 0); the knob is read and left alone"""
    hdr = open(os.path.join(ROOT, "include", "scan_hip.h")).read()
    assert re.search(r"int32_t\s+scan_gconv3x3_to1_caps\(int32_t G, int32_t Cg\);", hdr)
    for name, bit in (("RUNS", 1), ("LANE_MAPPED", 2), ("BITS", 4), ("ACT", 8)):
        assert re.search(r"#define\s+SCAN_GCONV_%s\s+%d\b" % (name, bit), hdr), name
    from scan_amd import _lib, ops
    assert (ops.GCONV_BITS, ops.GCONV_ACT) == (4, 8)
    gmax = _lib.query("scan_gconv3x3_to1_max_groups")
    old = _lib.query("scan_tune_get", b"gconv_mfma")
    try:
        for knob in (0, 1):
            _lib.query("scan_tune", b"gconv_mfma", knob)
            for G in range(0, 33):
                want = 0
                if 1 <= G <= gmax:
                    want = 1 | ((2 | (4 if knob == 1 else 8)) if G in (1, 2, 4, 8) else 0)
                assert _lib.query("scan_gconv3x3_to1_caps", G, 128) == want, (knob, G)
                assert bool(_lib.query("scan_gconv3x3_to1_caps", G, 128) & 1) == (1 <= G <= gmax)
                assert ops.cls_split_supported(G) == (G in (1, 2, 4, 8) and knob == 0)
            assert _lib.query("scan_gconv3x3_to1_caps", 2, 64) == 0
            assert _lib.query("scan_tune_get", b"gconv_mfma") == knob
    finally:
        _lib.query("scan_tune", b"gconv_mfma", old)

"""ATSS head, everything that needs no GPU: the fp64 restatement (tests/atss_ref.py) against the reference's fixtures
(tests/golden/atss_*.npz, written by tools/make_atss_golden.py), the torch spelling of the assignment (modeling/atss.py) against
both, the tie rules, the anchor formula, build_rpn / config / engine surface and the argument checks of the new entry points."""
import os

import numpy as np
import pytest
import torch

import atss_ref as R
from atss_ref import CASES, load_case, tie_inputs
from scan_amd import _lib, config, ops
from scan_amd.modeling import atss, factory

CPU = torch.device("cpu")


@pytest.mark.parametrize("name", CASES)
def test_fixture_conditions_hold(gold_dir, name):
    """what makes the reference's answer independent of torch.topk / torch.max tie-breaking and of threshold rounding"""
    f = load_case(gold_dir, name)
    H, W = (int(v) for v in f["image_hw"])
    _, _, details = R.assign(f["N"], f["sizes"], f["targets"], topk=int(f["topk"]))
    contested = border = empty = 0
    for (b, _), d in zip(f["targets"], details):
        assert (b != b.round()).all()
        assert (d["dist_gap"] > 0).all()
        assert ((d["cand_iou"] - d["thr"][None]).abs() > 1e-5).all()
        cx, cy = (b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2
        border += int(((cx < 8) | (cy < 8) | (cx > W - 8) | (cy > H - 8)).sum())
        empty += int((~d["pos"].any(0)).sum())
        seen = {}
        for g in range(b.shape[0]):
            for r, v in zip(d["cand_row"][d["pos"][:, g], g].tolist(), d["cand_iou"][d["pos"][:, g], g].tolist()):
                seen.setdefault(r, []).append(v)
        for vs in seen.values():
            if len(vs) > 1:
                contested += 1
                assert np.diff(sorted(vs)).min() > 1e-5
    assert contested == int(f["contested"]) > 0 and border > 0 and empty > 0
    assert sorted(int(g) for g in f["ng"]) == [1, 3]


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(gold_dir, name):
    f = load_case(gold_dir, name)
    labels, matched, _ = R.assign(f["N"], f["sizes"], f["targets"], topk=int(f["topk"]))
    assert np.array_equal(labels.numpy(), f["labels"])  # exact, no allowance
    pos = torch.nonzero(labels > 0).squeeze(1)
    assert np.array_equal(pos.numpy(), f["pos_inds"])
    anchors = R.row_anchors(f["N"], f["sizes"], anchor_sizes=[float(a) for a in f["anchor_sizes"]])
    off = R.row_offsets(f["N"], f["sizes"])
    img = torch.tensor([next((int(r) - off[l]) // (h * w) for l, (h, w) in enumerate(f["sizes"]) if off[l] <= int(r) < off[l + 1])
                        for r in pos])
    boxes = torch.from_numpy(f["boxes"]).double()[img, matched[pos]]
    reg_pos = R.encode(boxes, anchors[pos])
    np.testing.assert_allclose(reg_pos.numpy(), f["reg_pos"], rtol=1e-5, atol=1e-6)
    ctr_pos = R.centerness(reg_pos, anchors[pos])
    np.testing.assert_allclose(ctr_pos.numpy(), f["ctr_pos"], rtol=1e-5)
    got = R.losses(torch.from_numpy(f["logits"]).double(), torch.from_numpy(f["reg"]).double(),
                   torch.from_numpy(f["ctr"]).double(), labels, reg_pos, ctr_pos, pos, anchors, float(f["gamma"]),
                   float(f["alpha"]), float(f["reg_loss_weight"]))
    np.testing.assert_allclose([float(v) for v in got], f["losses"], rtol=1e-5)
    rows, cls, cbox, score = R.candidates(f["N"], f["sizes"], torch.from_numpy(f["inf_logits"]).double(),
                                          torch.from_numpy(f["inf_reg"]).double(), torch.from_numpy(f["inf_ctr"]).double(),
                                          [tuple(f["image_hw"])] * f["N"], anchors)
    ours = sorted(zip(rows.tolist(), cls.tolist()))
    assert ours == sorted(zip(f["cand_row"].tolist(), f["cand_cls"].tolist()))
    order = np.lexsort((f["cand_cls"], f["cand_row"]))
    np.testing.assert_allclose(score.numpy(), f["cand_score"][order], rtol=1e-5)
    assert (np.abs(cbox.numpy() - f["cand_box"][order]) <= 1e-4 * np.maximum(1, np.abs(f["cand_box"][order]))).all()


@pytest.mark.parametrize("name", CASES)
def test_anchor_formula_is_bit_equal_to_the_generator(gold_dir, name):
    f = load_case(gold_dir, name)
    shape = ops.PyramidShape(f["N"], f["sizes"])
    ours = atss.row_anchors(shape, CPU, sizes=[float(a) for a in f["anchor_sizes"]])
    assert ours.dtype == torch.float32 and np.array_equal(ours.numpy(), f["anchors"])
    assert np.array_equal(R.row_anchors(f["N"], f["sizes"], dtype=torch.float32).numpy(), f["anchors"])
    # two spot values of the generator (sizes 64 and 1024): the first P3 anchor, the P7 anchor
    a = atss.level_anchors(ops.PyramidShape(1, [(1, 1)] * 5), CPU)
    assert a[0][0].tolist() == [-28., -28., 35., 35.] and a[4][0].tolist() == [-448., -448., 575., 575.]


@pytest.mark.parametrize("name", CASES)
def test_torch_spelling_reproduces_the_reference_labels(gold_dir, name):
    f = load_case(gold_dir, name)
    shape = ops.PyramidShape(f["N"], f["sizes"])
    plan = atss.build_plan(shape, f["targets"], CPU, topk=int(f["topk"]))
    assert np.array_equal(plan.labels.numpy(), f["labels"])
    assert np.array_equal(plan.pos_inds.numpy(), f["pos_inds"]) and plan.n_pos == len(f["pos_inds"])
    _, matched, _ = R.assign(f["N"], f["sizes"], f["targets"], topk=int(f["topk"]))
    assert torch.equal(plan.matched.long(), matched)
    np.testing.assert_allclose(plan.reg_pos.numpy(), f["reg_pos"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(plan.ctr_pos.numpy(), f["ctr_pos"], rtol=1e-5, atol=1e-6)


def test_tie_rule_equal_distances_go_to_the_smaller_row():
    """integer boxes whose centres are equidistant from several anchors at the topk boundary: the torch spelling gives the
    restatement's stable-sort answer (the reference is not consulted: torch.topk promises no order among equals)"""
    sizes, targets = tie_inputs()
    labels, matched, details = R.assign(2, sizes, targets, topk=9)
    assert sum(int((d["dist_gap"] == 0).sum()) for d in details) > 0, "the inputs must have boundary ties"
    plan = atss.build_plan(ops.PyramidShape(2, sizes), targets, CPU, topk=9)
    assert torch.equal(plan.labels, labels) and torch.equal(plan.matched.long(), matched)
    assert plan.n_pos > 0


def test_contested_anchor_ties_go_to_the_smaller_box_index():
    """two identical boxes with different labels: every positive anchor sees two equal IoUs and takes box 0"""
    sizes = [(8, 12), (4, 6), (2, 3), (1, 2), (1, 1)]
    b = torch.tensor([[20.3, 10.2, 70.6, 50.7], [20.3, 10.2, 70.6, 50.7]])
    plan = atss.build_plan(ops.PyramidShape(1, sizes), [(b, torch.tensor([2, 1]))], CPU)
    assert plan.n_pos > 0 and set(plan.labels[plan.pos_inds].tolist()) == {2} and int(plan.matched.max()) == 0
    labels, matched, _ = R.assign(1, sizes, [(b, torch.tensor([2, 1]))])
    assert torch.equal(plan.labels, labels)


def test_image_without_boxes_is_all_background():
    sizes = [(8, 12), (4, 6), (2, 3), (1, 2), (1, 1)]
    tg = [(torch.zeros((0, 4)), torch.zeros((0,), dtype=torch.int64)), (torch.tensor([[20.3, 10.2, 70.6, 50.7]]), torch.tensor([1]))]
    shape = ops.PyramidShape(2, sizes)
    plan = atss.build_plan(shape, tg, CPU)
    hw0 = 8 * 12
    assert int(plan.labels[:hw0].sum()) == 0 and int(plan.labels[hw0:2 * hw0].sum()) > 0
    none = atss.build_plan(shape, [tg[0], tg[0]], CPU)
    assert none.n_pos == 0 and none.reg_pos.shape == (0, 4)


# ----------------------------------------------------------------------------- modules, config, factory
def atss_cfg(*opts):
    return config.load("c2f", ["MODEL.ATSS_ON", True, "MODEL.ATSS.NUM_CLASSES", 3] + list(opts))


def test_build_rpn_atss_state_dict_and_initial_values():
    torch.manual_seed(0)
    m = factory.build_rpn(atss_cfg("MODEL.ATSS.PRIOR_PROB", 0.02), 256)
    assert isinstance(m, factory.ATSSModuleNCHW) and isinstance(m, atss.ATSSModule)
    keys = set(m.state_dict())
    want = {"head.cls_logits.weight", "head.cls_logits.bias", "head.bbox_pred.weight", "head.bbox_pred.bias",
            "head.centerness.weight", "head.centerness.bias"}
    want |= {"head.scales.%d.scale" % l for l in range(5)}
    for tower in ("cls_tower", "bbox_tower"):
        for i in range(4):
            want |= {"head.%s.%d.%s" % (tower, 3 * i + j, p) for j in (0, 1) for p in ("weight", "bias")}
    assert keys == want
    sd = m.state_dict()
    assert sd["head.cls_logits.weight"].shape == (2, 256, 3, 3) and sd["head.bbox_pred.weight"].shape == (4, 256, 3, 3)
    assert torch.allclose(sd["head.cls_logits.bias"], torch.full((2,), -float(np.log((1 - 0.02) / 0.02))))
    assert float(sd["head.bbox_pred.bias"].abs().max()) == 0 and float(sd["head.cls_tower.0.bias"].abs().max()) == 0
    assert abs(float(sd["head.cls_tower.0.weight"].std()) - 0.01) < 5e-4
    assert all(float(sd["head.scales.%d.scale" % l]) == 1.0 for l in range(5))
    assert m.head.exp_reg is False
    # the tower switch: the last conv of both towers is a DFConv2d in the same slot
    d = factory.build_rpn(atss_cfg("MODEL.ATSS.USE_DCN_IN_TOWER", True, "MODEL.ATSS.NUM_CONVS", 2), 256)
    assert any(k.startswith("head.cls_tower.3.offset.") for k in d.state_dict())
    assert not any(k.startswith("head.cls_tower.6.") for k in d.state_dict())
    # ATSS_ON wins over FCOS_ON, as in the reference's build_rpn; neither: an error naming both
    assert isinstance(factory.build_rpn(atss_cfg("MODEL.FCOS_ON", True), 256), atss.ATSSModule)
    with pytest.raises(ValueError, match="ATSS_ON"):
        factory.build_rpn(config.load("c2f", ["MODEL.FCOS_ON", False]), 256)


def test_atss_settings_defaults_are_the_references():
    assert config.ATSS_DEFAULTS["NUM_CLASSES"] == 81  # the reference's default; outside what the kernels are built for
    s = config.atss_settings(config.load("c2f", ["MODEL.ATSS.NUM_CLASSES", 9]))
    assert s == dict(atss.DEFAULT_SETTINGS, num_classes=9, anchor_sizes=tuple(float(a) for a in atss.ANCHOR_SIZES))
    assert s["loss_gamma"] == 5.0 and s["topk"] == 9 and s["reg_loss_weight"] == 2.0


@pytest.mark.parametrize("key,value", [
    ("POSITIVE_TYPE", "SSC"), ("POSITIVE_TYPE", "IoU"), ("POSITIVE_TYPE", "TOPK"), ("POSITIVE_TYPE", "ADAPT_ATSS"),
    ("REGRESSION_TYPE", "POINT"), ("ASPECT_RATIOS", (0.5, 1.0, 2.0)), ("SCALES_PER_OCTAVE", 3),
    ("ANCHOR_STRIDES", (4, 8, 16, 32, 64)), ("ANCHOR_SIZES", (64, 128, 256)), ("TOPK", 0), ("TOPK", 65), ("NUM_CLASSES", 1),
    ("NUM_CLASSES", 81), ("NUM_CONVS", 0)])
def test_every_unsupported_value_raises_naming_its_key(key, value):
    with pytest.raises(ValueError, match="MODEL.ATSS." + key):
        factory.build_rpn(config.load("c2f", ["MODEL.ATSS_ON", True, "MODEL.ATSS.NUM_CLASSES", 3, "MODEL.ATSS." + key, value]), 256)


def test_reference_atss_yaml_loads_and_shipped_views_are_unchanged(gold_dir):
    import json
    cfg = config.load(os.path.join(gold_dir, "reference_yaml", "da_ga_sim10k_VGG_16_FPN_4x_atss.yaml"))
    assert cfg.MODEL.ATSS_ON is True
    s = config.atss_settings(cfg)
    assert s["num_classes"] == 2 and s["topk"] == 9 and s["anchor_sizes"] == (64., 128., 256., 512., 1024.)
    assert s["dcn_in_tower"] is False and s["detections_per_img"] == 100
    m = factory.build_rpn(cfg, 256)
    assert m.head.cls_logits.weight.shape[0] == 1
    assert "ATSS" not in config.DEFAULTS["MODEL"] and "ATSS_ON" not in config.DEFAULTS["MODEL"]
    for name in ("c2f", "s2c", "k2c"):
        gold = json.load(open(os.path.join(gold_dir, "cfg_%s.json" % name)))["cfg"]
        assert config.hot_path_view(config.load(name)) == gold


def test_engine_build_model_keyword():
    from scan_amd import engine
    base = engine.build_model(3, device="cpu")
    a = engine.build_model(3, device="cpu", rpn="atss")
    assert set(base) == set(a) == {"backbone", "middle_head", "fcos"} | {"dis_%s_CON" % l for l in engine.LEVELS}
    assert type(base["fcos"]).__name__ == "FCOSModule" and isinstance(a["fcos"], atss.ATSSModule)
    assert a["fcos"].head.cls_logits.weight.shape[0] == 2 and set(a["fcos"].state_dict()) == set(base["fcos"].state_dict())
    with pytest.raises(ValueError, match="rpn"):
        engine.build_model(3, device="cpu", rpn="retinanet")
    with pytest.raises(ValueError, match="distributed"):
        engine.Trainer(a, distributed=True)


def test_module_without_targets_returns_the_zero_loss():
    m = atss.ATSSModule(3)
    m.train()
    rows = torch.zeros((4, 256))
    out = m(None, rows, ops.PyramidShape(1, [(2, 2)]), targets=None, act_maps=object())
    assert out[0] is None and list(out[1]) == ["zero"] and float(out[1]["zero"]) == 0.0


# ----------------------------------------------------------------------------- C ABI without a device
def _desc(n=1, sizes=((4, 4), (2, 2))):
    return ops.PyramidShape(n, sizes)


def test_new_symbols_are_exported_and_declared():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "scan_hip.h")).read()
    L = _lib.lib()
    for name in ("scan_atss_assign_ws_bytes", "scan_atss_assign", "scan_atss_targets", "scan_atss_giou_forward",
                 "scan_atss_giou_ordered_ws_floats", "scan_atss_giou_forward_ordered", "scan_atss_giou_backward"):
        assert name in hdr and name in _lib.SIGNATURES and hasattr(L, name)
    assert "rpn/atss/loss.py:159-218, 354, 360-373" in hdr


def test_entry_points_validate_arguments_without_a_device():
    import ctypes
    L = _lib.lib()
    sh = _desc()
    st = (ctypes.c_int32 * 2)(8, 16)
    sz = (ctypes.c_float * 2)(64., 128.)
    one = ctypes.c_void_p(16)  # non-null, aligned; never dereferenced: every call below fails validation first
    assert L.scan_atss_assign_ws_bytes(sh.ref(), 3, 9) == 8 * sh.rows + 8 * (1 * 3 * 2 * 9)
    assert L.scan_atss_assign_ws_bytes(sh.ref(), 0, 9) == -1 and L.scan_atss_assign_ws_bytes(sh.ref(), 3, 65) == -1
    assert L.scan_atss_assign(None, st, sz, one, one, one, 3, 9, one, one, one, one, one, None) == -1
    assert b"bad pyramid" in L.scan_last_error()
    assert L.scan_atss_assign(sh.ref(), st, sz, None, one, one, 3, 9, one, one, one, one, one, None) == -1
    assert b"null pointer" in L.scan_last_error()
    assert L.scan_atss_assign(sh.ref(), st, sz, one, one, one, 3, 0, one, one, one, one, one, None) == -1
    assert b"topk=0" in L.scan_last_error()
    assert L.scan_atss_assign(sh.ref(), st, sz, one, one, one, 0, 9, one, one, one, one, one, None) == -1
    assert L.scan_atss_assign(sh.ref(), st, sz, ctypes.c_void_p(20), one, one, 3, 9, one, one, one, one, one, None) == -1
    assert b"aligned" in L.scan_last_error()
    bad = (ctypes.c_int32 * 2)(8, 0)
    assert L.scan_atss_assign(sh.ref(), bad, sz, one, one, one, 3, 9, one, one, one, one, one, None) == -1
    assert b"stride 0" in L.scan_last_error()
    broken = ops.PyramidShape(1, [(4, 4)])
    broken.desc.row_off[1] = 15
    assert L.scan_atss_assign(broken.ref(), st, sz, one, one, one, 3, 9, one, one, one, one, one, None) == -1
    assert b"inconsistent" in L.scan_last_error()
    cnt = (ctypes.c_int32 * 2)(17, 0)
    assert L.scan_atss_targets(sh.ref(), st, sz, cnt, one, 3, one, one, one, one, one, None) == -1
    assert b"17 positives of 16 rows" in L.scan_last_error()
    assert L.scan_atss_targets(sh.ref(), st, sz, None, one, 3, one, one, one, one, one, None) == -1
    zero = (ctypes.c_int32 * 2)(0, 0)
    assert L.scan_atss_targets(sh.ref(), st, sz, zero, one, 3, one, one, None, None, None, None) == 0  # nothing to write
    for fn, tail in (("scan_atss_giou_forward", (one, None)), ("scan_atss_giou_forward_ordered", (one, one, None)),
                     ("scan_atss_giou_backward", (one, one, None))):
        f = getattr(L, fn)
        assert f(sh.ref(), st, sz, one, one, one, one, -1, *tail) == -1
        assert f(sh.ref(), st, sz, one, one, one, one, 0, *tail) == 0  # P = 0: nothing to do
        assert f(sh.ref(), st, sz, None, one, one, one, 4, *tail) == -1 and b"null input" in L.scan_last_error()
        assert f(sh.ref(), st, sz, ctypes.c_void_p(20), one, one, one, 4, *tail) == -1 and b"aligned" in L.scan_last_error()
        assert f(sh.ref(), None, sz, one, one, one, one, 4, *tail) == -1
    assert L.scan_atss_giou_forward(sh.ref(), st, sz, one, one, one, one, 4, None, None) == -1
    assert L.scan_atss_giou_forward_ordered(sh.ref(), st, sz, one, one, one, one, 4, one, None, None) == -1
    assert L.scan_atss_giou_backward(sh.ref(), st, sz, one, one, one, one, 4, None, one, None) == -1
    assert L.scan_atss_giou_ordered_ws_floats(1) == 2 and L.scan_atss_giou_ordered_ws_floats(4097) == 6
    assert L.scan_atss_giou_ordered_ws_floats(1 << 24) == 512


def test_ops_wrapper_refuses_cpu_tensors_and_wrong_geometry():
    sh = _desc()
    p = torch.zeros((2, 4))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.atss_giou_loss(p, p, torch.zeros(2, dtype=torch.int64), torch.ones(2), sh, (8, 16), (64., 128.))
    with pytest.raises(ValueError, match="strides"):
        ops.atss_giou_loss(p, p, torch.zeros(2, dtype=torch.int64), torch.ones(2), sh, (8,), (64.,))

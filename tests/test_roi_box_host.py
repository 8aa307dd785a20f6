"""Fast R-CNN box head without a device: the fixtures' conditions re-asserted from the stored inputs, the numpy restatement
(tests/roi_box_ref.py) against the reference's answers in tests/golden/roi_box_*.npz, config.roi_box_settings, the factories, the
wrappers' argument checks and the state_dict keys."""
import json
import os

import numpy as np
import pytest
import torch

import roi_box_ref as B
from roi_box_ref import CASES, load_case
from scan_amd import _lib, config, ops
from scan_amd.modeling import factory, roi_box_head as rb


@pytest.fixture(scope="module")
def cases(gold_dir):
    out = {}
    for name in CASES:
        f = load_case(gold_dir, name)
        f["r"] = B.match(f["props"], f["np"], f["boxes"], f["glabels"], f["ng"], float(f["bg"]), float(f["fg"]))
        out[name] = f
    return out


# ----------------------------------------------------------------------------- fixtures and restatement
@pytest.mark.parametrize("name", CASES)
def test_fixture_conditions_and_plan(cases, name):
    f = cases[name]
    lab, matched, ious = f["r"]
    n_pos = B.check_match_conditions(f, ious, lab)
    assert n_pos == f["n_pos"].tolist()
    assert np.array_equal(lab, f["labels"]) and np.array_equal(matched, f["matched"])
    assert (f["bg"] < f["fg"]) == (name == "roi_box_band_64x96") and f["agnostic"] == (name == "roi_box_band_64x96")
    if name == "roi_box_c81_128x256":
        assert f["C"] == 81 and 80 in f["labels"]
    N, P, batch, frac = f["N"], f["P"], int(f["batch_size_per_image"]), float(f["positive_fraction"])
    s = f["sampled"].reshape(N, P)
    for n in range(N):  # the reference's draw has the counts of the sampler's rule
        own = lab.reshape(N, P)[n]
        num_pos = min(int((own > 0).sum()), int(batch * frac))
        assert int((s[n] == 1).sum()) == num_pos and int((s[n] == 2).sum()) == min(int((own == 0).sum()), batch - num_pos)
        assert (own[s[n] == 1] > 0).all() and (own[s[n] == 2] == 0).all()
    mine, counts = B.sample(lab, N, P, batch, frac, seed=5)  # the keyed rule draws as many, and never padding
    assert np.array_equal(counts, np.stack([(s == 1).sum(1), (s == 2).sum(1)], 1)) and (mine[lab < 0] == 0).all()


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_references_subsample_and_loss(cases, name):
    f = cases[name]
    w = tuple(float(v) for v in f["weights"])
    rois, lab, tg, src, counts = B.gather(f["props"], f["boxes"], f["labels"], f["matched"], f["sampled"].reshape(f["N"], f["P"]), w)
    assert counts.sum(1).tolist() == f["sub_count"].tolist()
    assert np.array_equal(rois[:, 1:], f["sub_box"]) and np.array_equal(lab, f["sub_labels"])
    pos = lab > 0
    assert np.allclose(tg[pos], f["sub_targets"][pos], rtol=1e-5, atol=1e-6) and (tg[~pos] == 0).all()
    lc, lb, dc, dr = B.losses_and_grads(f["cls"], f["reg"], f["sub_labels"], f["sub_targets"].astype(np.float64), f["agnostic"])
    assert abs(lc - f["losses"][0]) <= 1e-4 * f["losses"][0] and abs(lb - f["losses"][1]) <= 1e-4 * f["losses"][1]
    assert np.allclose(dc, f["d_cls"], rtol=1e-4, atol=1e-7) and np.allclose(dr, f["d_reg"], rtol=1e-4, atol=1e-7)


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_references_detections(cases, name):
    f = cases[name]
    w = tuple(float(v) for v in f["weights"])
    scores, boxes, cand, dw, raw = B.decode_all(f["inf_cls"], f["inf_reg"], f["inf_rois"], f["image_hw"], w, float(f["score_thresh"]))
    before = B.check_post_conditions(f, scores, boxes, cand, dw, raw)
    assert before == f["det_before_cap"].tolist()
    assert np.allclose(scores, f["ref_scores"], rtol=1e-5, atol=0)
    assert (np.abs(boxes - f["ref_boxes"]) <= 1e-4 * np.maximum(1, np.abs(f["ref_boxes"]))).all()
    dets = B.postprocess(scores, boxes, cand, f["inf_rois"], f["N"], float(f["nms"]), int(f["detections_per_img"]))
    assert [len(r) for r, _ in dets] == f["det_count"].tolist()
    rows, cls = np.concatenate([r for r, _ in dets]), np.concatenate([c for _, c in dets])
    assert np.array_equal(cls, f["det_label"])
    assert np.allclose(scores[rows, cls], f["det_score"], rtol=1e-5, atol=0)
    assert (np.abs(boxes[rows, cls] - f["det_box"]) <= 1e-4 * np.maximum(1, np.abs(f["det_box"]))).all()


# ----------------------------------------------------------------------------- config and factories
def _cfg(*extra):
    return config.load("c2f", ["MODEL.FCOS_ON", False, "MODEL.RPN_ONLY", False, "MODEL.MIDDLE_HEAD.CONDGRAPH_ON", False,
                               "MODEL.RPN.USE_FPN", True, "MODEL.ROI_HEADS.USE_FPN", True,
                               "MODEL.ROI_BOX_HEAD.FEATURE_EXTRACTOR", "FPN2MLPFeatureExtractor",
                               "MODEL.ROI_BOX_HEAD.PREDICTOR", "FPNPredictor", "MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION", 7,
                               "MODEL.ROI_BOX_HEAD.POOLER_SCALES", (0.125, 0.0625, 0.03125, 0.015625),
                               "MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO", 2] + list(extra))


def test_defaults_are_the_references_and_stay_out_of_DEFAULTS():
    assert config.ROI_HEADS_DEFAULTS == {
        "USE_FPN": False, "FG_IOU_THRESHOLD": 0.5, "BG_IOU_THRESHOLD": 0.5, "BBOX_REG_WEIGHTS": (10., 10., 5., 5.),
        "BATCH_SIZE_PER_IMAGE": 512, "POSITIVE_FRACTION": 0.25, "SCORE_THRESH": 0.05, "NMS": 0.5, "DETECTIONS_PER_IMG": 100}
    assert config.ROI_BOX_HEAD_DEFAULTS["FEATURE_EXTRACTOR"] == "ResNet50Conv5ROIFeatureExtractor"
    assert config.ROI_BOX_HEAD_DEFAULTS["NUM_CLASSES"] == 81 and config.ROI_BOX_HEAD_DEFAULTS["MLP_HEAD_DIM"] == 1024
    assert "ROI_HEADS" not in config.DEFAULTS["MODEL"] and "ROI_BOX_HEAD" not in config.DEFAULTS["MODEL"]


def test_settings_accept_the_references_yaml_keys():
    s = config.roi_box_settings(_cfg("MODEL.ROI_BOX_HEAD.NUM_CLASSES", 9, "MODEL.CLS_AGNOSTIC_BBOX_REG", True,
                                     "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", 256, "MODEL.ROI_HEADS.BG_IOU_THRESHOLD", 0.3))
    assert s["num_classes"] == 9 and s["cls_agnostic_bbox_reg"] and s["batch_size_per_image"] == 256
    assert s["bg_iou_threshold"] == 0.3 and s["fg_iou_threshold"] == 0.5 and s["bbox_reg_weights"] == (10., 10., 5., 5.)
    assert s["pooler_scales"] == (0.125, 0.0625, 0.03125, 0.015625) and s["pooler_resolution"] == 7 and s["mlp_head_dim"] == 1024
    assert config.roi_box_settings(_cfg("MODEL.ROI_BOX_HEAD.POOLER_SCALES", (0.125,)))["pooler_scales"] == (0.125,)


@pytest.mark.parametrize("key, extra", [
    ("MODEL.ROI_BOX_HEAD.FEATURE_EXTRACTOR", ["MODEL.ROI_BOX_HEAD.FEATURE_EXTRACTOR", "ResNet50Conv5ROIFeatureExtractor"]),
    ("MODEL.ROI_BOX_HEAD.FEATURE_EXTRACTOR", ["MODEL.ROI_BOX_HEAD.FEATURE_EXTRACTOR", "FPNXconv1fcFeatureExtractor"]),
    ("MODEL.ROI_BOX_HEAD.PREDICTOR", ["MODEL.ROI_BOX_HEAD.PREDICTOR", "FastRCNNPredictor"]),
    ("MODEL.ROI_BOX_HEAD.USE_GN", ["MODEL.ROI_BOX_HEAD.USE_GN", True]),
    ("MODEL.MASK_ON", ["MODEL.MASK_ON", True]),
    ("MODEL.KEYPOINT_ON", ["MODEL.KEYPOINT_ON", True]),
    ("MODEL.ROI_HEADS.USE_FPN", ["MODEL.ROI_HEADS.USE_FPN", False]),
    ("MODEL.ROI_BOX_HEAD.POOLER_SCALES", ["MODEL.ROI_BOX_HEAD.POOLER_SCALES", (0.0625,)]),
    ("MODEL.ROI_BOX_HEAD.POOLER_SCALES", ["MODEL.ROI_BOX_HEAD.POOLER_SCALES", (0.25, 0.125)]),
    ("MODEL.ROI_HEADS.BG_IOU_THRESHOLD", ["MODEL.ROI_HEADS.BG_IOU_THRESHOLD", 0.6]),
])
def test_settings_refuse_what_is_not_built_by_name(key, extra):
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        config.roi_box_settings(_cfg(*extra))


def test_the_references_defaults_must_be_overridden_explicitly():
    cfg = config.load("c2f", ["MODEL.ROI_HEADS.USE_FPN", True, "MODEL.ROI_BOX_HEAD.NUM_CLASSES", 9])
    with pytest.raises(ValueError, match="FEATURE_EXTRACTOR"):
        config.roi_box_settings(cfg)


def test_build_roi_heads():
    assert factory.build_roi_heads(_cfg("MODEL.RETINANET_ON", True), 256) == []
    assert factory.build_roi_heads(_cfg("MODEL.RPN_ONLY", True), 256) == []
    with pytest.raises(ValueError, match="ROI_BOX_HEAD"):
        factory.build_roi_heads(config.load("c2f", ["MODEL.RPN_ONLY", False]), 256)
    heads = factory.build_roi_heads(_cfg("MODEL.ROI_BOX_HEAD.NUM_CLASSES", 9, "MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM", 64), 256)
    assert isinstance(heads, rb.CombinedROIHeads) and isinstance(heads.box, rb.ROIBoxHead)
    assert all(k.startswith("box.") for k in heads.state_dict())


def test_generalized_rcnn_refuses_the_middle_head_and_trainers_refuse_the_rpn():
    from scan_amd import engine, epm
    with pytest.raises(ValueError, match="MIDDLE_HEAD.CONDGRAPH_ON"):
        factory.GeneralizedRCNN(_cfg("MODEL.MIDDLE_HEAD.CONDGRAPH_ON", True))
    with pytest.raises(ValueError, match="META_ARCHITECTURE"):
        factory.build_detection_model(_cfg("MODEL.META_ARCHITECTURE", "Other"))
    for build in (engine.build_model, epm.build_model):
        with pytest.raises((ValueError, TypeError)):
            build(9, device="cpu", rpn="rpn")


def test_state_dict_keys_and_shapes_are_the_references(gold_dir):
    with open(os.path.join(gold_dir, "roi_box_keys.json")) as fh:
        ref = json.load(fh)
    head = rb.ROIBoxHead(dict(rb.DEFAULT_SETTINGS, num_classes=ref["num_classes"], mlp_head_dim=ref["mlp_head_dim"],
                              pooler_resolution=ref["resolution"]), in_channels=ref["in_channels"])
    assert {k: list(v.shape) for k, v in head.state_dict().items()} == ref["state_dict"]
    head.load_state_dict({k: torch.zeros(s) for k, s in ref["state_dict"].items()}, strict=True)
    model = factory.build_detection_model(_cfg("MODEL.ROI_BOX_HEAD.NUM_CLASSES", 81))
    assert {k[len("roi_heads.box."):] for k in model.state_dict() if k.startswith("roi_heads.")} == set(ref["state_dict"])
    agn = rb.ROIBoxHead(dict(rb.DEFAULT_SETTINGS, cls_agnostic_bbox_reg=True, mlp_head_dim=32, pooler_resolution=3), in_channels=8)
    assert tuple(agn.predictor.bbox_pred.weight.shape) == (8, 32)


def test_initialisers_and_fc6_column_order():
    torch.manual_seed(0)
    fe, pr = rb.FPN2MLPFeatureExtractor(8, 3, (0.125, 0.0625), 2, 32), rb.FPNPredictor(1024, 81)
    assert float(fe.fc6.bias.abs().max()) == 0 and float(pr.cls_score.bias.abs().max()) == 0
    bound = (3.0 / 72) ** 0.5  # kaiming_uniform_(a=1): gain 1, fan_in 72
    assert float(fe.fc6.weight.abs().max()) <= bound and float(fe.fc6.weight.abs().max()) > 0.9 * bound
    assert abs(float(pr.cls_score.weight.std()) - 0.01) < 1e-3 and abs(float(pr.bbox_pred.weight.std()) - 0.001) < 1e-4
    # pooled rows are (PH, PW, Cs): the permuted weight applied to them equals fc6 on the reference's channel-major view
    y = torch.randn(5, 3, 3, 8)
    want = torch.nn.functional.linear(y.permute(0, 3, 1, 2).reshape(5, -1), fe.fc6.weight)
    assert torch.allclose(torch.nn.functional.linear(y.reshape(5, -1), fe.fc6_weight_rows(8)), want, atol=1e-6)
    y12 = torch.nn.functional.pad(y, (0, 4))  # a row pitch wider than C: zero weight columns
    assert torch.allclose(torch.nn.functional.linear(y12.reshape(5, -1), fe.fc6_weight_rows(12)), want, atol=1e-6)


# ----------------------------------------------------------------------------- the wrappers check before they call
def _refusals():
    props, n_props = torch.zeros((2, 6, 4)), torch.full((2,), 6, dtype=torch.int32)
    boxes, glab, ng = torch.zeros((2, 3, 4)), torch.zeros((2, 3), dtype=torch.int64), torch.full((2,), 3, dtype=torch.int32)
    i32v, u8v, counts = torch.zeros((12,), dtype=torch.int32), torch.zeros((12,), dtype=torch.uint8), torch.zeros((2, 2), dtype=torch.int32)
    cls, reg, lab, tg = torch.zeros((5, 9)), torch.zeros((5, 36)), torch.zeros((5,), dtype=torch.int32), torch.zeros((5, 4))
    rois, hw = torch.zeros((5, 5)), torch.zeros((2, 2), dtype=torch.int32)
    return [
        ("roi_box_match proposals", lambda: ops.roi_box_match(props[:, :, :3], n_props, boxes, glab, ng, 0.5, 0.5)),
        ("roi_box_match dtype", lambda: ops.roi_box_match(props.double(), n_props, boxes, glab, ng, 0.5, 0.5)),
        ("roi_box_match counts", lambda: ops.roi_box_match(props, n_props.long(), boxes, glab, ng, 0.5, 0.5)),
        ("roi_box_match labels", lambda: ops.roi_box_match(props, n_props, boxes, glab.int(), ng, 0.5, 0.5)),
        ("roi_box_match images", lambda: ops.roi_box_match(props, n_props, boxes[:1], glab[:1], ng[:1], 0.5, 0.5)),
        ("roi_box_match thresholds", lambda: ops.roi_box_match(props, n_props, boxes, glab, ng, 0.6, 0.5)),
        ("roi_box_gather sampled", lambda: ops.roi_box_gather(props, boxes, i32v, i32v, u8v[:11], counts, 4)),
        ("roi_box_gather matched", lambda: ops.roi_box_gather(props, boxes, i32v, i32v.long(), u8v, counts, 4)),
        ("roi_box_gather counts", lambda: ops.roi_box_gather(props, boxes, i32v, i32v, u8v, counts[:1], 4)),
        ("roi_box_gather R", lambda: ops.roi_box_gather(props, boxes, i32v, i32v, u8v, counts, 13)),
        ("roi_box_gather weights", lambda: ops.roi_box_gather(props, boxes, i32v, i32v, u8v, counts, 4, (10., 10., 5.))),
        ("roi_box_gather weights sign", lambda: ops.roi_box_gather(props, boxes, i32v, i32v, u8v, counts, 4, (10., 10., 5., 0.))),
        ("roi_box_loss C", lambda: ops.roi_box_loss(cls[:, :1], reg[:, :4], lab, tg)),
        ("roi_box_loss Cr", lambda: ops.roi_box_loss(cls, reg[:, :32], lab, tg)),
        ("roi_box_loss rows", lambda: ops.roi_box_loss(cls, reg[:4], lab, tg)),
        ("roi_box_loss labels", lambda: ops.roi_box_loss(cls, reg, lab.long(), tg)),
        ("roi_box_loss targets", lambda: ops.roi_box_loss(cls, reg, lab, tg[:, :3])),
        ("roi_box_loss pitch", lambda: ops.roi_box_loss(cls, torch.zeros((5, 38))[:, 1:37], lab, tg)),
        ("roi_box_loss columns", lambda: ops.roi_box_loss(cls.t().contiguous().t(), reg, lab, tg)),
        ("roi_box_decode rois", lambda: ops.roi_box_decode(cls, reg, rois[:, :4], hw)),
        ("roi_box_decode image_hw", lambda: ops.roi_box_decode(cls, reg, rois, hw.long())),
        ("roi_box_decode Cr", lambda: ops.roi_box_decode(cls, reg[:, :12], rois, hw)),
        ("roi_box_decode weights", lambda: ops.roi_box_decode(cls, reg, rois, hw, (1., 1., -1., 1.))),
    ]


@pytest.mark.parametrize("case", [name for name, _ in _refusals()])
def test_wrapper_refuses_before_any_library_call(case, monkeypatch):
    def no_call(name, *args):
        pytest.fail("%s reached the library (%s)" % (case, name))
    monkeypatch.setattr(ops, "call", no_call)
    monkeypatch.setattr(ops, "query", no_call)
    with pytest.raises(ValueError, match=case.split()[0]):
        dict(_refusals())[case]()


def test_agnostic_accepts_eight_columns_and_the_binding_has_the_entry_points(monkeypatch):
    assert ops._roi_box_head_outputs("t", torch.zeros((5, 9)), torch.zeros((5, 8))) == (5, 9, 2)
    assert ops._roi_box_head_outputs("t", torch.zeros((0, 2)), torch.zeros((0, 8))) == (0, 2, 2)  # C = 2: 4 C = 8 either way
    i32, i64, f32, vp = _lib.ctypes.c_int32, _lib.ctypes.c_int64, _lib.ctypes.c_float, _lib.ctypes.c_void_p
    assert _lib.SIGNATURES["scan_roi_box_match"] == (_lib.ctypes.c_int, [vp, vp, i32, i32, vp, vp, vp, i32, f32, f32, vp, vp, vp])
    assert _lib.SIGNATURES["scan_roi_box_loss_ordered_ws_floats"] == (i64, [i64])
    assert _lib.SIGNATURES["scan_roi_box_loss_forward_ordered"][1] == [vp, i64, vp, i64, i32, i32, i32, vp, vp, vp, vp, vp]
    for name in ("scan_roi_box_gather", "scan_roi_box_loss_forward", "scan_roi_box_loss_backward", "scan_roi_box_decode"):
        assert name in _lib.SIGNATURES
    with pytest.raises(ValueError, match="bg"):
        rb.FastRCNNLossComputation(bg=0.6, fg=0.5)
    le = rb.FastRCNNLossComputation()
    with pytest.raises(RuntimeError, match="subsample"):
        le(torch.zeros((1, 9)), torch.zeros((1, 36)))

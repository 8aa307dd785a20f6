"""Mask R-CNN mask head without a device: the fixtures' conditions re-asserted from the stored inputs, the numpy restatement
(tests/roi_mask_ref.py) against the reference's answers in tests/golden/roi_mask_*.npz, config.roi_mask_settings, the factories,
SegmentationMask in binary-mask mode, the wrappers' argument checks and the state_dict keys."""
import json
import os

import numpy as np
import pytest
import torch

import roi_box_ref as B
import roi_mask_ref as R
from roi_mask_ref import CASES, load_case
from scan_amd import _lib, config, ops
from scan_amd.modeling import factory, roi_box_head as rb, roi_mask_head as rm
from scan_amd.structures import BinaryMaskList, BoxList, SegmentationMask


@pytest.fixture(scope="module")
def cases(gold_dir):
    out = {}
    for name in CASES:
        f = load_case(gold_dir, name)
        f["rule"] = R.targets_rule(f["masks_per_image"], f["pos_rois"], f["pos_gt"], f["M"])
        out[name] = f
    return out


# ----------------------------------------------------------------------------- fixtures and restatement
@pytest.mark.parametrize("name", CASES)
def test_fixture_conditions_and_positives(cases, name):
    f = cases[name]
    diff, ones = R.check_target_conditions(f, f["rule"], f["ref_targets"])
    assert diff == int(f["n_rounding"]) and ones == int(f["n_rule_ones"])
    assert f["predictor"] == ("MaskRCNNConv1x1Predictor" if name == "roi_mask_m14_64x96" else "MaskRCNNC4Predictor")
    assert f["M"] == (14 if name == "roi_mask_m14_64x96" else 28) and f["C"] == (81 if name == "roi_mask_c81_128x256" else 9)
    # the box plan of the stored inputs: its matched index at the positives is what the reference's mask loss re-matched
    lab, matched, _ = B.match(f["props"], f["np"], f["boxes"], f["glabels"], f["ng"], float(f["bg"]), float(f["fg"]))
    rois, sub_labels, _, src, counts = B.gather(f["props"], f["boxes"], lab, matched, f["sampled"].reshape(f["N"], f["P"]))
    assert np.array_equal(rois, f["sub_rois"]) and np.array_equal(sub_labels, f["sub_labels"]) and np.array_equal(src, f["sub_src"])
    assert np.array_equal(matched, f["matched"])
    rows, pos_rois, pos_labels, pos_gt = R.positives(sub_labels, rois, src, matched, f["P"])
    assert np.array_equal(rows, f["pos_rows"]) and np.array_equal(pos_rois, f["pos_rois"])
    assert np.array_equal(pos_labels, f["pos_labels"]) and np.array_equal(pos_gt, f["pos_gt"])
    assert int(counts[:, 0].sum()) == f["Rp"]  # every sampled positive is a positive row: Rp comes from the counts


def test_the_deviation_is_exercised(cases):
    assert sum(int(f["n_rounding"]) for f in cases.values()) > 0


@pytest.mark.parametrize("name", CASES)
def test_fp32_evaluation_only_loses_ones(cases, name):
    """the reference's expression evaluated in fp32 never writes a 1 the exact value does not have"""
    f = cases[name]
    fp32 = np.stack([R.target_fp32(f["masks_per_image"][int(r[0])][int(g)], r[1:], f["M"]) for r, g in zip(f["pos_rois"], f["pos_gt"])])
    assert (f["rule"] >= fp32).all()


def test_all_ones_crops_stay_all_ones_under_the_rule():
    for n in (1, 2, 13, 27, 28, 29, 59):
        m = np.ones((n, 31), np.uint8)
        assert R.target_rule(m, [0, 0, 31, n], 28).all() and R.target_rule(m, [0, 0, 31, n], 14).all()
    m = np.zeros((9, 9), np.uint8)
    m[4, 4] = 1
    t = R.target_rule(m, [0, 0, 9, 9], 9)  # identity resize: the one pixel alone
    assert t.sum() == 1 and t[4, 4] == 1


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_references_loss_and_gradient(cases, name):
    f = cases[name]
    Rp, C, M = f["Rp"], f["C"], f["M"]
    x = R.make_logits(f["logit_seed"], Rp, C, M)[np.arange(Rp), f["pos_labels"]]
    loss, d = R.bce(x, f["ref_targets"])
    assert abs(loss - float(f["loss"])) <= 1e-4 * float(f["loss"])
    assert np.allclose(d, f["d_label"], rtol=1e-4, atol=1e-7)


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_references_probabilities_and_paste(cases, name):
    f = cases[name]
    K, C, M = f["K"], f["C"], f["M"]
    x = R.make_logits(f["inf_seed"], K, C, M, scale=3.0)[np.arange(K), f["det_label"]]
    p = R.sigmoid(x)
    assert np.allclose(p, f["ref_prob"][:, 0], rtol=1e-5, atol=0)
    mine = R.check_paste_conditions(f, p)
    assert np.array_equal(mine, f["ref_paste"]) and f["ref_paste"].any()


# ----------------------------------------------------------------------------- config and factories
def _cfg(*extra):
    return config.load("c2f", ["MODEL.FCOS_ON", False, "MODEL.RPN_ONLY", False, "MODEL.MIDDLE_HEAD.CONDGRAPH_ON", False,
                               "MODEL.RPN.USE_FPN", True, "MODEL.ROI_HEADS.USE_FPN", True,
                               "MODEL.ROI_BOX_HEAD.FEATURE_EXTRACTOR", "FPN2MLPFeatureExtractor",
                               "MODEL.ROI_BOX_HEAD.PREDICTOR", "FPNPredictor", "MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION", 7,
                               "MODEL.ROI_BOX_HEAD.POOLER_SCALES", (0.125, 0.0625, 0.03125, 0.015625),
                               "MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO", 2, "MODEL.MASK_ON", True,
                               "MODEL.ROI_MASK_HEAD.FEATURE_EXTRACTOR", "MaskRCNNFPNFeatureExtractor",
                               "MODEL.ROI_MASK_HEAD.PREDICTOR", "MaskRCNNC4Predictor", "MODEL.ROI_MASK_HEAD.POOLER_RESOLUTION", 14,
                               "MODEL.ROI_MASK_HEAD.POOLER_SCALES", (0.125, 0.0625, 0.03125, 0.015625),
                               "MODEL.ROI_MASK_HEAD.POOLER_SAMPLING_RATIO", 2, "MODEL.ROI_MASK_HEAD.RESOLUTION", 28,
                               "MODEL.ROI_MASK_HEAD.SHARE_BOX_FEATURE_EXTRACTOR", False] + list(extra))


def test_roi_mask_settings():
    """accepts the keys of the reference's Mask R-CNN FPN yamls (e2e_mask_rcnn_R_50_FPN_1x.yaml) and lets roi_box_settings through"""
    cfg = _cfg("MODEL.ROI_BOX_HEAD.NUM_CLASSES", 9, "MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS", True)
    s = config.roi_mask_settings(cfg)
    assert s["predictor"] == "MaskRCNNC4Predictor" and s["resolution"] == 28 and s["pooler_resolution"] == 14
    assert s["pooler_scales"] == (0.125, 0.0625, 0.03125, 0.015625) and s["pooler_sampling_ratio"] == 2
    assert s["conv_layers"] == (256, 256, 256, 256) and s["num_classes"] == 9 and s["postprocess_masks"]
    assert s["postprocess_masks_threshold"] == 0.5 and s["fg_iou_threshold"] == 0.5 and s["bg_iou_threshold"] == 0.5
    assert config.roi_box_settings(cfg)["num_classes"] == 9  # MASK_ON with the block present passes the box head's view
    s = config.roi_mask_settings(_cfg("MODEL.ROI_MASK_HEAD.PREDICTOR", "MaskRCNNConv1x1Predictor", "MODEL.ROI_MASK_HEAD.RESOLUTION", 14,
                                      "MODEL.ROI_MASK_HEAD.POOLER_SCALES", (0.125,)))
    assert s["predictor"] == "MaskRCNNConv1x1Predictor" and s["resolution"] == 14 and s["pooler_scales"] == (0.125,)


@pytest.mark.parametrize("key, extra", [
    ("MODEL.ROI_MASK_HEAD.FEATURE_EXTRACTOR", ["MODEL.ROI_MASK_HEAD.FEATURE_EXTRACTOR", "ResNet50Conv5ROIFeatureExtractor"]),
    ("MODEL.ROI_MASK_HEAD.PREDICTOR", ["MODEL.ROI_MASK_HEAD.PREDICTOR", "Other"]),
    ("MODEL.ROI_MASK_HEAD.SHARE_BOX_FEATURE_EXTRACTOR", ["MODEL.ROI_MASK_HEAD.SHARE_BOX_FEATURE_EXTRACTOR", True]),
    ("MODEL.ROI_MASK_HEAD.USE_GN", ["MODEL.ROI_MASK_HEAD.USE_GN", True]),
    ("MODEL.ROI_MASK_HEAD.DILATION", ["MODEL.ROI_MASK_HEAD.DILATION", 2]),
    ("MODEL.ROI_MASK_HEAD.POOLER_SCALES", ["MODEL.ROI_MASK_HEAD.POOLER_SCALES", (0.0625,)]),
    ("MODEL.ROI_MASK_HEAD.POOLER_SCALES", ["MODEL.ROI_MASK_HEAD.POOLER_SCALES", (0.25, 0.125)]),
    ("MODEL.ROI_MASK_HEAD.RESOLUTION", ["MODEL.ROI_MASK_HEAD.RESOLUTION", 14]),
    ("MODEL.ROI_MASK_HEAD.RESOLUTION", ["MODEL.ROI_MASK_HEAD.PREDICTOR", "MaskRCNNConv1x1Predictor"]),
    ("MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS_THRESHOLD", ["MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS_THRESHOLD", -1.0]),
    ("MODEL.KEYPOINT_ON", ["MODEL.KEYPOINT_ON", True]),
])
def test_mask_settings_refuse_what_is_not_built_by_name(key, extra):
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        config.roi_mask_settings(_cfg(*extra))


def test_the_references_mask_defaults_must_be_overridden_and_the_block_must_be_there():
    assert config.ROI_MASK_HEAD_DEFAULTS == {
        "FEATURE_EXTRACTOR": "ResNet50Conv5ROIFeatureExtractor", "PREDICTOR": "MaskRCNNC4Predictor", "POOLER_RESOLUTION": 14,
        "POOLER_SAMPLING_RATIO": 0, "POOLER_SCALES": (1.0 / 16,), "MLP_HEAD_DIM": 1024, "CONV_LAYERS": (256, 256, 256, 256),
        "RESOLUTION": 14, "SHARE_BOX_FEATURE_EXTRACTOR": True, "POSTPROCESS_MASKS": False, "POSTPROCESS_MASKS_THRESHOLD": 0.5,
        "DILATION": 1, "USE_GN": False}
    assert "ROI_MASK_HEAD" not in config.DEFAULTS["MODEL"]
    base = ["MODEL.ROI_HEADS.USE_FPN", True, "MODEL.MASK_ON", True, "MODEL.ROI_MASK_HEAD.RESOLUTION", 28]
    with pytest.raises(ValueError, match="FEATURE_EXTRACTOR"):
        config.roi_mask_settings(config.load("c2f", base))
    with pytest.raises(ValueError, match="SHARE_BOX_FEATURE_EXTRACTOR"):
        config.roi_mask_settings(config.load("c2f", base + ["MODEL.ROI_MASK_HEAD.FEATURE_EXTRACTOR", "MaskRCNNFPNFeatureExtractor"]))
    no_block = config.load("c2f", ["MODEL.MASK_ON", True])
    with pytest.raises(ValueError, match=r"MODEL\.ROI_MASK_HEAD"):
        config.roi_mask_settings(no_block)
    with pytest.raises(ValueError, match=r"MODEL\.MASK_ON.*ROI_MASK_HEAD block"):
        config.roi_box_settings(no_block)


def test_build_roi_heads_and_state_dict_keys(gold_dir):
    with open(os.path.join(gold_dir, "roi_mask_keys.json")) as fh:
        ref = json.load(fh)
    heads = factory.build_roi_heads(_cfg("MODEL.ROI_BOX_HEAD.NUM_CLASSES", 81, "MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM", 64), 256)
    assert isinstance(heads, rb.CombinedROIHeads) and list(heads.keys()) == ["box", "mask"] and isinstance(heads.mask, rm.ROIMaskHead)
    keys = ref["state_dict"]["MaskRCNNC4Predictor"]
    assert {k[len("mask."):]: list(v.shape) for k, v in heads.state_dict().items() if k.startswith("mask.")} == keys
    heads.mask.load_state_dict({k: torch.zeros(s) for k, s in keys.items()}, strict=True)
    one = rm.ROIMaskHead(dict(rm.DEFAULT_SETTINGS, predictor="MaskRCNNConv1x1Predictor", resolution=14))
    assert {k: list(v.shape) for k, v in one.state_dict().items()} == ref["state_dict"]["MaskRCNNConv1x1Predictor"]
    box_only = factory.build_roi_heads(_cfg("MODEL.MASK_ON", False), 256)
    assert list(box_only.keys()) == ["box"]
    with pytest.raises(ValueError, match="resolution"):
        rm.ROIMaskHead(dict(rm.DEFAULT_SETTINGS, resolution=14))


def test_initialisers_and_the_transposed_conv_as_a_1x1_conv():
    torch.manual_seed(0)
    fe, pr = rm.MaskRCNNFPNFeatureExtractor(), rm.MaskRCNNC4Predictor(256, 256, 81)
    assert float(fe.mask_fcn1.bias.detach().abs().max()) == 0 and float(pr.conv5_mask.bias.detach().abs().max()) == 0
    assert abs(float(fe.mask_fcn1.weight.std()) - (2.0 / (256 * 9)) ** 0.5) < 1e-3  # kaiming_normal_(fan_out, relu)
    assert abs(float(pr.mask_fcn_logits.weight.std()) - (2.0 / 81) ** 0.5) < 2e-2
    # the regrouped weight on (P, P, C) rows followed by the pixel shuffle equals F.conv_transpose2d
    small = rm.MaskRCNNC4Predictor(8, 4, 3)
    small.conv5_mask.bias.data.normal_()
    x = torch.randn(2, 8, 3, 3)
    want = torch.relu(torch.nn.functional.conv_transpose2d(x, small.conv5_mask.weight, small.conv5_mask.bias, stride=2))
    w = small.conv5_mask.weight.permute(2, 3, 1, 0).reshape(16, 8)
    y = torch.relu(x.permute(0, 2, 3, 1).reshape(-1, 8) @ w.t() + small.conv5_mask.bias.repeat(4))
    y = y.reshape(2, 3, 3, 2, 2, 4).permute(0, 1, 3, 2, 4, 5).reshape(2, 6, 6, 4).permute(0, 3, 1, 2)
    assert torch.allclose(y, want, atol=1e-5)


# ----------------------------------------------------------------------------- SegmentationMask, binary mode
def test_segmentation_mask_binary_mode_equals_the_reference(cases):
    f = cases["roi_mask_64x96"]
    H, W = f["H"], f["W"]
    m0 = torch.from_numpy(f["masks_per_image"][0].copy())
    seg = SegmentationMask(m0, (W, H), mode="mask")
    assert len(seg) == m0.shape[0] and seg.size == (W, H) and seg.to("cpu") is seg
    crop = seg.crop(torch.from_numpy(f["seg_box"]))
    assert crop.size == tuple(int(v) for v in f["seg_crop_size"])
    G, (cw, ch) = len(seg), crop.size
    assert np.array_equal(crop.get_mask_tensor().numpy(), R.unbits(f["seg_crop_bits"], (G, ch, cw)))
    assert np.array_equal(crop.resize((20, 12)).get_mask_tensor().numpy(), R.unbits(f["seg_resize_bits"], (G, 12, 20)))
    assert np.array_equal(seg.transpose(0).get_mask_tensor().numpy(), R.unbits(f["seg_flip_bits"], (G, H, W)))
    assert np.array_equal(seg.transpose(1).get_mask_tensor().numpy(), m0.numpy()[:, ::-1])
    assert len(seg[torch.tensor([2, 0])]) == 2 and tuple(seg[1].get_mask_tensor().shape) == (H, W)
    assert np.array_equal(seg[torch.tensor([2, 0])].get_mask_tensor().numpy(), m0.numpy()[[2, 0]])
    x0, y0, x1, y1 = R.crop_box(f["seg_box"], W, H)
    assert (x1 - x0, y1 - y0) == crop.size
    m0[0, 0, 0] = 1 - m0[0, 0, 0]  # the list holds a copy
    assert not np.array_equal(seg.get_mask_tensor().numpy(), m0.numpy())


def test_segmentation_mask_refuses_polygons_and_boxlist_carries_the_field():
    with pytest.raises(ValueError, match="mode"):
        SegmentationMask([[[0.0, 0.0, 4.0, 0.0, 4.0, 4.0]]], (8, 8), mode="poly")
    with pytest.raises(ValueError, match="mode"):
        SegmentationMask([[[0.0, 0.0, 4.0, 0.0, 4.0, 4.0]]], (8, 8))  # the reference's default is polygons
    with pytest.raises(ValueError, match="masks"):
        BinaryMaskList(torch.zeros((2, 5, 8)), (5, 8))  # size is width-first
    m = torch.zeros((2, 6, 8), dtype=torch.uint8)
    m[0, 1:3, 2:5], m[1, 4, 7] = 1, 1
    b = BoxList(torch.tensor([[2., 1., 4., 2.], [7., 4., 7., 4.]]), (8, 6))
    b.add_field("masks", SegmentationMask(m, (8, 6), mode="mask"))
    b.add_field("labels", torch.tensor([1, 2]))
    flipped = b.transpose(0).get_field("masks")
    assert np.array_equal(flipped.get_mask_tensor().numpy(), m.numpy()[:, :, ::-1])
    assert b.resize((16, 12)).get_field("masks").size == (16, 12)
    assert len(b[torch.tensor([1])].get_field("masks")) == 1 and b.to("cpu").get_field("masks").mode == "mask"
    flat, moff, mhw = rm.upload_masks([b, (b.bbox, b.get_field("labels"), m[:1, :4, :4])], "cpu")
    assert moff.tolist() == [0, 96, 112] and mhw.tolist() == [[6, 8], [4, 4]] and flat.dtype == torch.uint8 and flat.numel() == 112
    with pytest.raises(ValueError, match="masks"):
        rm.upload_masks([(b.bbox, b.get_field("labels"))], "cpu")


# ----------------------------------------------------------------------------- the wrappers check before they call
def _refusals():
    lab, rois, src = torch.zeros((5,), dtype=torch.int32), torch.zeros((5, 5)), torch.zeros((5,), dtype=torch.int32)
    matched = torch.zeros((12,), dtype=torch.int32)
    masks, moff, mhw = torch.zeros((96,), dtype=torch.uint8), torch.zeros((3,), dtype=torch.int64), torch.zeros((2, 2), dtype=torch.int32)
    gt = torch.zeros((5,), dtype=torch.int32)
    logits, tg = torch.zeros((5 * 16, 12)), torch.zeros((5, 4, 4))
    prob, boxes = torch.zeros((5, 1, 4, 4)), torch.zeros((5, 4))
    return [
        ("roi_mask_positives labels", lambda: ops.roi_mask_positives(lab.long(), rois, src, matched, 2, 6, 3)),
        ("roi_mask_positives rois", lambda: ops.roi_mask_positives(lab, rois[:, :4], src, matched, 2, 6, 3)),
        ("roi_mask_positives src", lambda: ops.roi_mask_positives(lab, rois, src[:4], matched, 2, 6, 3)),
        ("roi_mask_positives matched", lambda: ops.roi_mask_positives(lab, rois, src, matched[:11], 2, 6, 3)),
        ("roi_mask_positives Rp", lambda: ops.roi_mask_positives(lab, rois, src, matched, 2, 6, 6)),
        ("roi_mask_targets rois", lambda: ops.roi_mask_targets(rois.double(), gt, masks, moff, mhw, 4)),
        ("roi_mask_targets pos_gt", lambda: ops.roi_mask_targets(rois, gt.long(), masks, moff, mhw, 4)),
        ("roi_mask_targets masks", lambda: ops.roi_mask_targets(rois, gt, masks.float(), moff, mhw, 4)),
        ("roi_mask_targets moff", lambda: ops.roi_mask_targets(rois, gt, masks, moff[:2], mhw, 4)),
        ("roi_mask_targets mhw", lambda: ops.roi_mask_targets(rois, gt, masks, moff, mhw.long(), 4)),
        ("roi_mask_targets M", lambda: ops.roi_mask_targets(rois, gt, masks, moff, mhw, 0)),
        ("roi_mask_loss targets", lambda: ops.roi_mask_loss(logits, lab, tg[:, :, :3])),
        ("roi_mask_loss logits", lambda: ops.roi_mask_loss(logits[:79], lab, tg)),
        ("roi_mask_loss labels", lambda: ops.roi_mask_loss(logits, lab.long(), tg)),
        ("roi_mask_loss C", lambda: ops.roi_mask_loss(logits, lab, tg, 13)),
        ("roi_mask_loss rows", lambda: ops.roi_mask_loss(torch.zeros((12, 80)).t(), lab, tg)),
        ("roi_mask_prob labels", lambda: ops.roi_mask_prob(logits, lab.float(), 4)),
        ("roi_mask_prob logits", lambda: ops.roi_mask_prob(logits, lab[:4], 4)),
        ("roi_mask_paste thresh", lambda: ops.roi_mask_paste(prob, boxes, (8, 8), -1.0)),
        ("roi_mask_paste prob", lambda: ops.roi_mask_paste(prob[:, 0], boxes, (8, 8))),
        ("roi_mask_paste boxes", lambda: ops.roi_mask_paste(prob, boxes[:4], (8, 8))),
        ("roi_mask_paste image_hw", lambda: ops.roi_mask_paste(prob, boxes, (0, 8))),
    ]


@pytest.mark.parametrize("case", [name for name, _ in _refusals()])
def test_wrapper_refuses_before_any_library_call(case, monkeypatch):
    def no_call(name, *args):
        pytest.fail("%s reached the library (%s)" % (case, name))
    monkeypatch.setattr(ops, "call", no_call)
    monkeypatch.setattr(ops, "query", no_call)
    with pytest.raises(ValueError, match=case.split()[0]):
        dict(_refusals())[case]()


def test_cpu_tensors_are_refused_and_the_binding_has_the_entry_points():
    with pytest.raises(RuntimeError, match="GPU"):
        ops.roi_mask_prob(torch.zeros((16, 4)), torch.zeros((1,), dtype=torch.int64), 4)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.roi_mask_loss(torch.zeros((0, 4)), torch.zeros((0,), dtype=torch.int32), torch.zeros((0, 4, 4)))
    i32, i64, f32, vp = _lib.ctypes.c_int32, _lib.ctypes.c_int64, _lib.ctypes.c_float, _lib.ctypes.c_void_p
    assert _lib.SIGNATURES["scan_roi_mask_positives"] == (_lib.ctypes.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp])
    assert _lib.SIGNATURES["scan_roi_mask_targets"][1] == [vp, vp, i32, vp, i64, vp, vp, i32, i32, vp, vp]
    assert _lib.SIGNATURES["scan_roi_mask_loss_ordered_ws_floats"] == (i64, [i64])
    assert _lib.SIGNATURES["scan_roi_mask_loss_forward_ordered"][1] == [vp, i64, i32, i32, i32, vp, vp, vp, vp, vp]
    assert _lib.SIGNATURES["scan_roi_mask_paste"][1] == [vp, vp, i32, i32, i32, i32, f32, vp, vp]
    for name in ("scan_roi_mask_loss_forward", "scan_roi_mask_loss_backward", "scan_roi_mask_prob"):
        assert name in _lib.SIGNATURES
    with pytest.raises(ValueError, match="pycocotools"):
        rm.MaskPostProcessorCOCOFormat()
    with pytest.raises(ValueError, match="threshold"):
        rm.Masker(threshold=-1)
    with pytest.raises(ValueError, match="bg"):
        rm.MaskRCNNLossComputation(bg=0.6, fg=0.5)
    with pytest.raises(RuntimeError, match="plan"):
        rm.MaskRCNNLossComputation()(torch.zeros((16, 4)))

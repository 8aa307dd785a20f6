"""Region-proposal network without a device: the fp64 / integer restatement (tests/rpn_ref.py) against the reference's fixtures
(tests/golden/rpn_*.npz, tools/make_rpn_golden.py), the sampler's rule, config.rpn_settings, factory.build_rpn and the C ABI's
argument checks."""
import ctypes
import os

import numpy as np
import pytest
import torch

import retinanet_ref as R
import rpn_ref as P
from rpn_ref import CASES, load_case
from scan_amd import _lib, config, ops
from scan_amd.modeling import factory, rpn

BOX_TOL = 1e-4  # |box - ref| <= BOX_TOL * max(1, |ref|): test_gpu_retinanet.py's bar for decoded candidates


def rpn_cfg(*opts):
    return config.load("c2f", ["MODEL.FCOS_ON", False, "MODEL.RPN.USE_FPN", True] + list(opts))


@pytest.fixture(scope="module")
def restated(gold_dir):
    """per case the fixture and the restatement's labels / matched / IoUs / visibility / image of every anchor, computed once"""
    out = {}
    for name in CASES:
        f = load_case(gold_dir, name)
        lab, matched, ious, vis = P.labels(f["N"], f["sizes"], f["box_lists"], f["cells"], f["image_hw"], float(f["bg"]),
                                           float(f["fg"]), float(f["straddle_thresh"]))
        img = R.anchors_in_order(f["N"], f["sizes"], f["cells"])[1]
        out[name] = (f, lab, matched, ious, vis, img)
    return out


# ----------------------------------------------------------------------------- 1. the restatement against the fixtures
@pytest.mark.parametrize("name", CASES)
def test_fixture_conditions_hold(restated, name):
    f, lab, _, ious, vis, img = restated[name]
    for b in f["box_lists"]:
        assert (b != np.round(b)).all()
    stats = P.check_label_conditions(ious, lab, vis, img, f["N"], float(f["bg"]), float(f["fg"]), int(f["batch_size_per_image"]),
                                     float(f["positive_fraction"]))
    assert tuple(stats[:3]) == tuple(f["stats"]) and list(stats[3]) == list(f["n_pos"])
    A, N = int(f["num_anchors"]), f["N"]
    assert {"rpn_64x96": 387, "rpn_128x256": 2046}[name] == lab.size // N
    score = 1.0 / (1.0 + np.exp(-f["inf_obj"].astype(np.float64).reshape(-1)))
    for n in range(N):
        s = np.sort(score[img == n])
        assert (s[1:] - s[:-1] > 1e-6).all()
    h, w = f["sizes"][0]
    assert h * w * A > int(f["pre_nms_top_n"]) == int(f["topk_k"][0])
    ws, hs = f["topk_box"][..., 2] - f["topk_box"][..., 0] + 1, f["topk_box"][..., 3] - f["topk_box"][..., 1] + 1
    alive = (ws >= float(f["min_size"])) & (hs >= float(f["min_size"]))
    if name == CASES[0]:
        assert float(f["min_size"]) == 2 and int((~alive).sum()) > 0
    assert float(f["inf_reg"].reshape(-1, 4)[:, 2].max()) > P.CLIP
    # NMS removes at least one box per image: a greedy NMS per (image, level) over the stored live candidates keeps fewer
    off = np.concatenate([[0], np.cumsum(f["topk_k"])])
    for n in range(N):
        n_alive = n_kept = 0
        for l in range(len(f["topk_k"])):
            cols = np.arange(off[l], off[l + 1])[alive[n, off[l]:off[l + 1]]]
            n_alive += cols.size
            n_kept += len(P.greedy_nms(f["topk_box"][n, cols], f["topk_score"][n, cols], float(f["nms_thresh"])))
        assert n_kept < n_alive, (name, n, n_kept, n_alive)


@pytest.mark.parametrize("name", CASES)
def test_restated_labels_visibility_and_targets_equal_the_reference(restated, name):
    f, lab, matched, _, vis, _ = restated[name]
    assert np.array_equal(vis, f["visibility"]) and np.array_equal(lab, f["labels"]) and np.array_equal(matched, f["matched"])
    assert np.array_equal(f["cells"], P.cell_anchors().astype(np.float32))
    t = P.targets64(f["N"], f["sizes"], f["box_lists"], f["cells"], f["matched_all"])
    np.testing.assert_allclose(t, f["reg_targets"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name", CASES)
def test_restated_loss_equals_the_reference(restated, name):
    f, lab, matched, _, _, _ = restated[name]
    s = f["sampled"]
    assert not (s[lab != 1] == 1).any() and not (s[lab != 0] == 2).any()
    t = P.targets64(f["N"], f["sizes"], f["box_lists"], f["cells"], matched)
    obj = torch.from_numpy(f["obj"]).double().reshape(-1).requires_grad_(True)
    reg = torch.from_numpy(f["reg"]).double().reshape(-1, 4).requires_grad_(True)
    bce, sl1 = P.loss_sums(obj, reg, s, t, 1.0 / 9)
    n = int((s != 0).sum())
    ((bce + sl1) / n).backward()
    np.testing.assert_allclose([float(bce.detach()) / n, float(sl1.detach()) / n], f["losses"], rtol=1e-4)
    np.testing.assert_allclose(obj.grad.numpy().reshape(f["d_obj"].shape), f["d_obj"], rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(reg.grad.numpy().reshape(f["d_reg"].shape), f["d_reg"], rtol=1e-4, atol=1e-7)


@pytest.mark.parametrize("name", CASES)
def test_restated_topk_and_decode_equal_the_reference(restated, name):
    f = restated[name][0]
    A = int(f["num_anchors"])
    topk = P.topk_per_level(f["inf_obj"], f["N"], f["sizes"], A, int(f["pre_nms_top_n"]))
    assert np.array_equal(np.concatenate(topk, 1), f["topk_idx"]) and [t.shape[1] for t in topk] == list(f["topk_k"])
    _, deltas, anchors, hw = P.candidate_geometry(topk, f["N"], f["sizes"], A, f["cells"], f["inf_reg"], f["image_hw"])
    boxes, keep = P.decode(deltas.reshape(-1, 4), anchors.reshape(-1, 4), hw.reshape(-1, 2), float(f["min_size"]))
    ref = f["topk_box"].reshape(-1, 4)
    assert (np.abs(boxes - ref) <= BOX_TOL * np.maximum(1, np.abs(ref))).all()
    ws, hs = ref[:, 2] - ref[:, 0] + 1, ref[:, 3] - ref[:, 1] + 1
    assert np.array_equal(keep, (ws >= float(f["min_size"])) & (hs >= float(f["min_size"])))


# ----------------------------------------------------------------------------- 2. the sampler's rule
def test_sample_key_is_the_stated_mix():
    """the key of three (seed, image, anchor index) triples as literal values (evaluated once by hand from the formula in
    include/scan_hip.h), and against a second spelling of the mix in Python integers; the GPU test holds the kernel to the same
    function"""
    def fmix(x):
        x ^= x >> 16
        x = x * 0x85EBCA6B & 0xffffffff
        x ^= x >> 13
        x = x * 0xC2B2AE35 & 0xffffffff
        return x ^ (x >> 16)
    for seed, n, i, literal in ((0x0, 0, 0, 0xAA3E5B61), (0x7, 1, 386, 0x966F1168), (0xdeadbeef, 3, 123456, 0x99C2179D)):
        want = fmix(fmix(seed ^ (0x9E3779B9 * (n + 1) & 0xffffffff)) ^ i)
        assert int(P.sample_key(seed, n, np.array([i]))[0]) == want == literal


def test_restated_sampler_counts_subset_and_coverage(restated):
    f, lab, _, _, _, img = restated[CASES[0]]
    B, frac = int(f["batch_size_per_image"]), float(f["positive_fraction"])
    for seed in (0, 1, 12345):
        s, counts = P.sample(lab, img, f["N"], B, frac, seed)
        for n in range(f["N"]):
            own = img == n
            n_p, n_n = int((lab[own] >= 1).sum()), int((lab[own] == 0).sum())
            assert counts[n, 0] == min(n_p, int(B * frac)) == int((s[own] == 1).sum())
            assert counts[n, 1] == min(n_n, B - counts[n, 0]) == int((s[own] == 2).sum())
        assert (lab[s == 1] >= 1).all() and (lab[s == 2] == 0).all()
    # 12 positives, choose 4: over 64 seeds every positive is chosen at least once and none always
    lab12 = np.full(40, -1, np.int64)
    lab12[3:39:3] = 1
    assert int((lab12 == 1).sum()) == 12
    times = np.zeros(40, int)
    for seed in range(64):
        s, counts = P.sample(lab12, np.zeros(40, int), 1, 8, 0.5, seed)
        assert counts.tolist() == [[4, 0]]
        times += s == 1
    assert (times[lab12 == 1] > 0).all() and (times[lab12 == 1] < 64).all() and not times[lab12 != 1].any()
    # equal keys: the smallest anchor indices
    s, _ = P.sample(lab12, np.zeros(40, int), 1, 8, 0.5, keys=np.full(40, 5))
    assert np.nonzero(s)[0].tolist() == [3, 6, 9, 12]


# ----------------------------------------------------------------------------- 3. settings and the factory
REFERENCE_DEFAULTS = {  # the reference's MODEL.RPN block (config/defaults.py)
    "USE_FPN": False, "ANCHOR_SIZES": (32, 64, 128, 256, 512), "ANCHOR_STRIDE": (16,), "ASPECT_RATIOS": (0.5, 1.0, 2.0),
    "STRADDLE_THRESH": 0, "FG_IOU_THRESHOLD": 0.7, "BG_IOU_THRESHOLD": 0.3, "BATCH_SIZE_PER_IMAGE": 256, "POSITIVE_FRACTION": 0.5,
    "PRE_NMS_TOP_N_TRAIN": 12000, "PRE_NMS_TOP_N_TEST": 6000, "POST_NMS_TOP_N_TRAIN": 2000, "POST_NMS_TOP_N_TEST": 1000,
    "NMS_THRESH": 0.7, "MIN_SIZE": 0, "FPN_POST_NMS_TOP_N_TRAIN": 2000, "FPN_POST_NMS_TOP_N_TEST": 2000,
    "RPN_HEAD": "SingleConvRPNHead"}


def test_rpn_defaults_are_the_references_apart_from_the_pyramid():
    want = dict(REFERENCE_DEFAULTS, USE_FPN=True, ANCHOR_STRIDE=(8, 16, 32, 64, 128))
    assert config.RPN_DEFAULTS == want
    assert "RPN" not in config.DEFAULTS["MODEL"]
    assert config.rpn_settings(rpn_cfg("MODEL.RPN_ONLY", False)) == rpn.DEFAULT_SETTINGS
    s = config.rpn_settings(rpn_cfg("MODEL.RPN.MIN_SIZE", 2))  # the shipped yamls set MODEL.RPN_ONLY, as the reference's FCOS ones
    assert s["rpn_only"] is True and s["min_size"] == 2.0


@pytest.mark.parametrize("opts, key", [
    (["MODEL.RPN.USE_FPN", False], "USE_FPN"),
    (["MODEL.RPN.ANCHOR_STRIDE", (16,)], "ANCHOR_STRIDE"),
    (["MODEL.RPN.ANCHOR_STRIDE", (4, 8, 16, 32, 64)], "ANCHOR_STRIDE"),
    (["MODEL.RPN.ANCHOR_SIZES", (32, 64, 128)], "ANCHOR_SIZES"),
    (["MODEL.RPN.ANCHOR_SIZES", ((32, 48), 64, 128, 256, 512)], "ANCHOR_SIZES"),
    (["MODEL.RPN.ASPECT_RATIOS", ()], "ASPECT_RATIOS"),
    (["MODEL.RPN.ASPECT_RATIOS", tuple(0.1 * k for k in range(1, 18))], "ASPECT_RATIOS"),
    (["MODEL.RPN.RPN_HEAD", "SingleConvRPNHead_1"], "RPN_HEAD"),
    (["MODEL.RPN.BG_IOU_THRESHOLD", 0.8], "BG_IOU_THRESHOLD"),
    (["MODEL.RPN.BATCH_SIZE_PER_IMAGE", 0], "BATCH_SIZE_PER_IMAGE"),
    (["MODEL.RPN.POSITIVE_FRACTION", 0.0], "POSITIVE_FRACTION"),
    (["MODEL.RPN.POSITIVE_FRACTION", 1.5], "POSITIVE_FRACTION"),
    (["MODEL.RPN.PRE_NMS_TOP_N_TRAIN", 0], "PRE_NMS_TOP_N_TRAIN"),
])
def test_rpn_settings_refusals_name_their_key(opts, key):
    with pytest.raises(ValueError, match="MODEL.RPN." + key):
        config.rpn_settings(rpn_cfg(*opts))
    with pytest.raises(ValueError, match="MODEL.RPN." + key):
        factory.build_rpn(rpn_cfg(*opts), 256)


def test_build_rpn_returns_the_module_with_the_references_keys(gold_dir):
    torch.manual_seed(3)
    m = factory.build_rpn(rpn_cfg(), 256)
    assert isinstance(m, factory.RPNModuleNCHW) and isinstance(m, rpn.RPNModule)
    want = {"head.%s.%s" % (c, p) for c in ("conv", "cls_logits", "bbox_pred") for p in ("weight", "bias")}
    want |= {"anchor_generator.cell_anchors.%d" % l for l in range(5)}  # the reference's BufferList
    sd = m.state_dict()
    assert set(sd) == want
    assert sd["head.conv.weight"].shape == (256, 256, 3, 3) and sd["head.cls_logits.weight"].shape == (3, 256, 1, 1)
    assert sd["head.bbox_pred.weight"].shape == (12, 256, 1, 1)
    for c in ("conv", "cls_logits", "bbox_pred"):
        assert float(sd["head.%s.bias" % c].abs().max()) == 0
    assert abs(float(sd["head.conv.weight"].std()) - 0.01) < 5e-4 and abs(float(sd["head.bbox_pred.weight"].std()) - 0.01) < 1e-3
    cells = load_case(gold_dir, CASES[0])["cells"]
    for l in range(5):
        assert np.array_equal(sd["anchor_generator.cell_anchors.%d" % l].numpy(), cells[l])
    assert m.box_selector_train.training and not m.box_selector_test.training
    assert m.box_selector_train.pre_nms_top_n == 12000 and m.box_selector_test.pre_nms_top_n == 6000
    a1 = factory.build_rpn(rpn_cfg("MODEL.RPN.ASPECT_RATIOS", (1.0,)), 256)
    assert a1.state_dict()["head.bbox_pred.weight"].shape[0] == 4 and a1.cells.shape == (5, 1, 4)
    # the reference's order: the dense heads first
    assert type(factory.build_rpn(config.load("c2f", ["MODEL.RPN.USE_FPN", True]), 256)).__name__ == "FCOSModuleNCHW"


def test_without_an_rpn_block_build_rpn_still_raises():
    with pytest.raises(ValueError, match="ATSS_ON.*FCOS_ON.*RETINANET_ON.*MODEL.RPN block"):
        factory.build_rpn(config.load("c2f", ["MODEL.FCOS_ON", False]), 256)
    with pytest.raises(ValueError, match="256 input channels"):
        factory.build_rpn(rpn_cfg(), 512)


def test_trainer_integration_is_still_refused():
    from scan_amd import engine, epm
    with pytest.raises(ValueError, match="rpn"):
        engine.build_model(3, device="cpu", rpn="rpn")
    with pytest.raises(ValueError, match="rpn"):
        epm.build_model(3, rpn="rpn", device="cpu")


def test_training_without_targets_is_refused():
    m = rpn.RPNModule()
    m.train()
    with pytest.raises(ValueError, match="targets"):
        m([(16, 16)], torch.zeros((4, 256)), ops.PyramidShape(1, [(2, 2)]), targets=None)


# ----------------------------------------------------------------------------- 4. C ABI without a device
NAMES = ("scan_rpn_visibility", "scan_rpn_sample", "scan_rpn_loss_forward", "scan_rpn_loss_ordered_ws_floats",
         "scan_rpn_loss_forward_ordered", "scan_rpn_loss_backward", "scan_rpn_decode")


def test_new_symbols_are_exported_and_declared():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "scan_hip.h")).read()
    L = _lib.lib()
    for name in NAMES:
        assert name in hdr and name in _lib.SIGNATURES and hasattr(L, name)
    assert "0x9E3779B9" in hdr and "0x85EBCA6B" in hdr and "0xC2B2AE35" in hdr  # the key mix is written out


def test_entry_points_validate_arguments_without_a_device():
    L = _lib.lib()
    sh = ops.PyramidShape(1, ((4, 4), (2, 2)))
    st = (ctypes.c_int32 * 2)(8, 16)
    one = ctypes.c_void_p(16)  # non-null, aligned; never dereferenced: every call below fails validation first

    def vis(d=sh.ref(), strides=st, cells=one, A=3, hw=one, lab=one, mat=one):
        return L.scan_rpn_visibility(d, strides, cells, A, hw, 0.0, lab, mat, None)

    assert vis(d=None) == -1 and b"bad pyramid" in L.scan_last_error()
    assert vis(hw=None) == -1 and b"null pointer" in L.scan_last_error()
    assert vis(lab=None) == -1 and vis(mat=None) == -1 and vis(cells=None) == -1 and vis(A=17) == -1

    def smp(d=sh.ref(), A=3, lab=one, batch=16, cap=8, out=one, cnt=one):
        return L.scan_rpn_sample(d, A, lab, batch, cap, 0, None, out, cnt, None)

    assert smp(d=None) == -1 and b"bad pyramid" in L.scan_last_error()
    assert smp(A=0) == -1 and b"A=0" in L.scan_last_error()
    assert smp(lab=None) == -1 and smp(out=None) == -1 and smp(cnt=None) == -1 and b"null pointer" in L.scan_last_error()
    assert smp(batch=0) == -1 and b"batch_size_per_image=0" in L.scan_last_error()
    assert smp(cap=17) == -1 and b"max_positives=17" in L.scan_last_error()
    assert smp(cap=-1) == -1

    def common(fn, tail, d=sh.ref(), strides=st, cells=one, A=3, boxes=one, G=2, mat=one, smp_=one, obj=one, ldo=4, reg=one, ld=12,
               beta=1.0 / 9):
        return getattr(L, fn)(d, strides, cells, A, boxes, G, mat, smp_, obj, ldo, reg, ld, beta, *tail)

    for fn, tail in (("scan_rpn_loss_forward", (None, one, None)), ("scan_rpn_loss_forward_ordered", (None, one, one, None)),
                     ("scan_rpn_loss_backward", (one, one, 3, one, 12, None))):
        assert common(fn, tail, d=None) == -1 and b"bad pyramid" in L.scan_last_error()
        assert common(fn, tail, reg=None) == -1 and b"null input" in L.scan_last_error()
        assert common(fn, tail, obj=None) == -1 and common(fn, tail, smp_=None) == -1 and common(fn, tail, mat=None) == -1
        assert common(fn, tail, reg=ctypes.c_void_p(20)) == -1 and b"aligned" in L.scan_last_error()
        assert common(fn, tail, ld=11) == -1 and b"row pitch 11" in L.scan_last_error()
        assert common(fn, tail, ldo=2) == -1 and b"row pitch 2" in L.scan_last_error()
        assert common(fn, tail, beta=0.0) == -1 and b"beta" in L.scan_last_error()
        assert common(fn, tail, A=17) == -1 and common(fn, tail, G=0) == -1
    assert common("scan_rpn_loss_forward", (None, None, None)) == -1 and b"null output" in L.scan_last_error()
    assert common("scan_rpn_loss_forward_ordered", (None, one, None, None)) == -1
    assert common("scan_rpn_loss_forward", (ctypes.c_void_p(20), one, None)) == -1 and b"targets_out" in L.scan_last_error()
    assert common("scan_rpn_loss_backward", (None, one, 3, one, 12, None)) == -1
    assert common("scan_rpn_loss_backward", (one, one, 2, one, 12, None)) == -1 and b"pitch" in L.scan_last_error()
    assert L.scan_rpn_loss_ordered_ws_floats(1) == 2 and L.scan_rpn_loss_ordered_ws_floats(4097) == 6

    koff = (ctypes.c_int32 * 3)(0, 10, 14)

    def dec(d=sh.ref(), strides=st, cells=one, A=3, reg=one, ld=12, idx=one, k=koff, hw=one, boxes=one, keep=one):
        return L.scan_rpn_decode(d, strides, cells, A, reg, ld, idx, k, hw, 0.0, boxes, keep, None)

    assert dec(d=None) == -1 and dec(reg=None) == -1 and b"null pointer" in L.scan_last_error()
    assert dec(idx=None) == -1 and dec(k=None) == -1 and dec(hw=None) == -1 and dec(boxes=None) == -1 and dec(keep=None) == -1
    assert dec(ld=10) == -1 and b"row pitch 10" in L.scan_last_error()
    assert dec(reg=ctypes.c_void_p(20)) == -1 and b"aligned" in L.scan_last_error()
    assert dec(k=(ctypes.c_int32 * 3)(1, 10, 14)) == -1 and b"k_off[0]=1" in L.scan_last_error()
    assert dec(k=(ctypes.c_int32 * 3)(0, 10, 23)) == -1 and b"level 1 has 13 candidates" in L.scan_last_error()
    assert dec(k=(ctypes.c_int32 * 3)(0, 10, 9)) == -1


def test_ops_wrappers_refuse_cpu_tensors_and_wrong_arguments():
    sh = ops.PyramidShape(1, ((4, 4), (2, 2)))
    cells = rpn.cell_anchors((8, 16), (32, 64))
    n = sh.rows * 3
    i32 = torch.zeros((n,), dtype=torch.int32)
    u8 = torch.zeros((n,), dtype=torch.uint8)
    boxes = torch.zeros((1, 1, 4))
    hw = torch.tensor([[32, 32]], dtype=torch.int32)
    obj, reg = torch.zeros((sh.rows, 3)), torch.zeros((sh.rows, 12))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.rpn_loss(obj, reg, sh, (8, 16), cells, boxes, i32, u8, 1.0 / 9)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.rpn_sample(sh, 3, i32, 16, 0.5)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.rpn_labels(sh, (8, 16), cells, boxes, torch.zeros((1,), dtype=torch.int32), hw, 0.3, 0.7, 0.0)
    with pytest.raises(ValueError, match="strides"):
        ops.rpn_loss(obj, reg, sh, (8,), cells, boxes, i32, u8, 1.0 / 9)
    with pytest.raises(ValueError, match="objectness"):
        ops.rpn_loss(reg, reg, sh, (8, 16), cells, boxes, i32, u8, 1.0 / 9)
    with pytest.raises(ValueError, match="bbox_reg"):
        ops.rpn_loss(obj, obj, sh, (8, 16), cells, boxes, i32, u8, 1.0 / 9)
    with pytest.raises(ValueError, match="matched"):
        ops.rpn_loss(obj, reg, sh, (8, 16), cells, boxes, i32.long(), u8, 1.0 / 9)
    with pytest.raises(ValueError, match="sampled"):
        ops.rpn_loss(obj, reg, sh, (8, 16), cells, boxes, i32, i32, 1.0 / 9)
    with pytest.raises(ValueError, match="beta"):
        ops.rpn_loss(obj, reg, sh, (8, 16), cells, boxes, i32, u8, 0.0)
    with pytest.raises(ValueError, match="labels_i32"):
        ops.rpn_sample(sh, 3, i32[:-1], 16, 0.5)
    with pytest.raises(ValueError, match="batch_size_per_image"):
        ops.rpn_sample(sh, 3, i32, 0, 0.5)
    with pytest.raises(ValueError, match="positive_fraction"):
        ops.rpn_sample(sh, 3, i32, 16, 0.0)
    with pytest.raises(ValueError, match="keys"):
        ops.rpn_sample(sh, 3, i32, 16, 0.5, keys=torch.zeros((n,), dtype=torch.int64))
    with pytest.raises(ValueError, match="image_hw"):
        ops.rpn_labels(sh, (8, 16), cells, boxes, torch.zeros((1,), dtype=torch.int32), hw.long(), 0.3, 0.7, 0.0)
    with pytest.raises(ValueError, match="bg_thr"):
        ops.rpn_labels(sh, (8, 16), cells, boxes, torch.zeros((1,), dtype=torch.int32), hw, 0.8, 0.7, 0.0)
    with pytest.raises(ValueError, match="ks"):
        ops.rpn_decode_proposals(reg, sh, (8, 16), cells, torch.zeros((1, 60), dtype=torch.int64), (49, 11), hw)
    with pytest.raises(ValueError, match="topk_idx"):
        ops.rpn_decode_proposals(reg, sh, (8, 16), cells, torch.zeros((1, 59), dtype=torch.int64), (48, 12), hw)

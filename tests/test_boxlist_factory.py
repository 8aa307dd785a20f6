"""CPU tests (no GPU): BoxList / cat_boxlist / remove_small_boxes against hand-computed answers (reference
structures/bounding_box.py:9-266, structures/boxlist_ops.py, TO_REMOVE = 1 convention), the reference-shaped module factories
(scan_amd/modeling/factory.py) built from the three shipped yamls with the engine's state_dict keys, and the C ABI of the
pyramid pack / unpack kernels (exported, argument validation without a device)."""
import ctypes

import pytest
import torch

from scan_amd import _lib, config, engine, ops
from scan_amd.modeling import factory
from scan_amd.structures import FLIP_LEFT_RIGHT, FLIP_TOP_BOTTOM, BoxList, cat_boxlist, remove_small_boxes


def _boxes():
    # image 20 wide, 10 high
    b = BoxList([[2.0, 1.0, 5.0, 3.0], [0.0, 0.0, 19.0, 9.0], [4.0, 4.0, 4.0, 4.0]], (20, 10), "xyxy")
    b.add_field("labels", torch.tensor([3, 1, 2]))
    b.add_field("scores", torch.tensor([0.5, 0.25, 0.125]))
    return b


def test_boxlist_construction_and_fields():
    b = _boxes()
    assert len(b) == 3 and b.size == (20, 10) and b.mode == "xyxy" and b.bbox.dtype == torch.float32
    assert b.has_field("labels") and not b.has_field("masks") and sorted(b.fields()) == ["labels", "scores"]
    c = b.copy_with_fields("labels")
    assert c.fields() == ["labels"] and c.bbox is b.bbox
    assert b.copy_with_fields(["labels", "nope"], skip_missing=True).fields() == ["labels"]
    with pytest.raises(KeyError):
        b.copy_with_fields(["nope"])
    with pytest.raises(ValueError):
        BoxList(torch.zeros(3, 5), (4, 4))
    with pytest.raises(ValueError):
        BoxList(torch.zeros(3, 4), (4, 4), "cxcywh")
    assert len(BoxList(torch.zeros(0, 4), (4, 4))) == 0


def test_boxlist_convert_round_trip():
    b = _boxes()
    w = b.convert("xywh")
    # width = x1 - x0 + 1: the box covering pixel 4 alone is 1 x 1
    assert w.mode == "xywh" and w.bbox.tolist() == [[2, 1, 4, 3], [0, 0, 20, 10], [4, 4, 1, 1]]
    assert w.get_field("labels") is b.get_field("labels")
    back = w.convert("xyxy")
    assert back.mode == "xyxy" and torch.equal(back.bbox, b.bbox)
    assert b.convert("xyxy") is b
    with pytest.raises(ValueError):
        b.convert("polygon")


def test_boxlist_resize():
    b = _boxes()
    r = b.resize((40, 20))  # one ratio: plain scaling
    assert r.size == (40, 20) and r.bbox.tolist() == [[4, 2, 10, 6], [0, 0, 38, 18], [8, 8, 8, 8]]
    assert torch.equal(r.get_field("scores"), b.get_field("scores"))
    r = b.resize((10, 20))  # x halves, y doubles
    assert r.size == (10, 20) and r.mode == "xyxy" and r.bbox.tolist() == [[1, 2, 2.5, 6], [0, 0, 9.5, 18], [2, 8, 2, 8]]
    r = b.convert("xywh").resize((10, 20))  # through xyxy and back: w = 2.5 - 1 + 1
    assert r.mode == "xywh" and r.bbox.tolist() == [[1, 2, 2.5, 5], [0, 0, 10.5, 19], [2, 8, 1, 1]]


def test_boxlist_flips():
    b = _boxes()
    lr = b.transpose(FLIP_LEFT_RIGHT)  # columns are pixel indices: x' = 20 - x - 1
    assert lr.bbox.tolist() == [[14, 1, 17, 3], [0, 0, 19, 9], [15, 4, 15, 4]] and lr.size == (20, 10)
    tb = b.transpose(FLIP_TOP_BOTTOM)  # rows are coordinates: y' = 10 - y
    assert tb.bbox.tolist() == [[2, 7, 5, 9], [0, 1, 19, 10], [4, 6, 4, 6]]
    assert torch.equal(lr.transpose(FLIP_LEFT_RIGHT).bbox, b.bbox)
    assert lr.get_field("labels").tolist() == [3, 1, 2]
    with pytest.raises(NotImplementedError):
        b.transpose(2)


def test_boxlist_clip_area_index():
    b = BoxList([[-3.0, -2.0, 25.0, 4.0], [21.0, 2.0, 30.0, 5.0], [3.0, 12.0, 6.0, 15.0], [1.0, 1.0, 2.0, 3.0]], (20, 10))
    b.add_field("labels", torch.tensor([1, 2, 3, 4]))
    kept = b.clip_to_image(remove_empty=False)
    assert kept is b and b.bbox.tolist() == [[0, 0, 19, 4], [19, 2, 19, 5], [3, 9, 6, 9], [1, 1, 2, 3]]
    c = BoxList([[-3.0, -2.0, 25.0, 4.0], [21.0, 2.0, 30.0, 5.0], [3.0, 12.0, 6.0, 15.0], [1.0, 1.0, 2.0, 3.0]], (20, 10))
    c.add_field("labels", torch.tensor([1, 2, 3, 4]))
    c = c.clip_to_image(remove_empty=True)  # boxes 1 (x1 == x0) and 2 (y1 == y0) collapse
    assert c.bbox.tolist() == [[0, 0, 19, 4], [1, 1, 2, 3]] and c.get_field("labels").tolist() == [1, 4]
    assert c.area().tolist() == [100.0, 6.0] and c.convert("xywh").area().tolist() == [100.0, 6.0]
    m = b[torch.tensor([True, False, False, True])]
    assert m.bbox.tolist() == [[0, 0, 19, 4], [1, 1, 2, 3]] and m.get_field("labels").tolist() == [1, 4] and m.size == (20, 10)
    i = b[torch.tensor([3, 0])]
    assert i.get_field("labels").tolist() == [4, 1] and i.bbox[0].tolist() == [1, 1, 2, 3]
    assert b.to("cpu").get_field("labels").tolist() == [1, 2, 3, 4]


def test_cat_boxlist_and_remove_small_boxes():
    a, b = _boxes(), _boxes()[torch.tensor([2, 0])]
    c = cat_boxlist([a, b])
    assert len(c) == 5 and c.size == (20, 10) and c.mode == "xyxy"
    assert c.get_field("labels").tolist() == [3, 1, 2, 2, 3] and c.bbox[3].tolist() == [4, 4, 4, 4]
    with pytest.raises(ValueError):
        cat_boxlist([a, BoxList(torch.zeros(1, 4), (20, 10))])  # field sets differ
    with pytest.raises(ValueError):
        cat_boxlist([a.copy_with_fields([]), BoxList(torch.zeros(1, 4), (10, 10))])  # image sizes differ
    # sides in pixels: 4 x 3, 20 x 10, 1 x 1
    assert remove_small_boxes(a, 1).get_field("labels").tolist() == [3, 1, 2]
    assert remove_small_boxes(a, 3).get_field("labels").tolist() == [3, 1]
    assert remove_small_boxes(a, 4).get_field("labels").tolist() == [1]
    assert len(remove_small_boxes(a, 21)) == 0


@pytest.mark.parametrize("name", ["c2f", "s2c", "k2c"])
def test_factories_build_from_shipped_yaml_with_engine_state_dict_keys(name):
    cfg = config.load(name)
    backbone = factory.build_backbone(cfg)
    assert backbone.out_channels == 256
    model = {"backbone": backbone, "middle_head": factory.build_middle_head(cfg, backbone.out_channels),
             "fcos": factory.build_rpn(cfg, backbone.out_channels)}
    dis = factory.build_discriminators(cfg)
    assert list(dis) == ["dis_%s_CON" % l for l in ("P7", "P6", "P5", "P4", "P3")]
    model.update(dis)
    eng = engine.build_model(device="cpu", settings=config.settings(cfg))
    assert set(model) == set(eng)
    for k, m in model.items():
        assert isinstance(m, type(eng[k])) and type(m) is not type(eng[k])  # a subclass: only forward differs
        assert list(m.state_dict()) == list(eng[k].state_dict()), k
        for (n1, p1), (n2, p2) in zip(m.named_parameters(), eng[k].named_parameters()):
            assert n1 == n2 and p1.shape == p2.shape and p1.stride() == p2.stride() and p1.requires_grad == p2.requires_grad
    for lvl in ("P3", "P7"):
        d = model["dis_%s_CON" % lvl]
        assert d.grad_reverse.lambda_ == cfg.MODEL.ADV["GRL_WEIGHT_%s" % lvl]
        assert d.num_convs == cfg.MODEL.ADV["CON_NUM_SHARED_CONV_%s" % lvl]
    assert model["fcos"].head.num_fg == cfg.MODEL.FCOS.NUM_CLASSES - 1 and model["fcos"].mode == cfg.TEST.MODE
    # the engine's loader takes them (same keys, same shapes)
    engine.load_state_dicts({"fcos": model["fcos"]}, {"fcos": eng["fcos"].state_dict()})


def test_factories_honour_the_cfg_switches():
    for body in ("R-50-FPN-RETINANET", "R-101-FPN-RETINANET"):
        cfg = config.load("k2c", ["MODEL.BACKBONE.CONV_BODY", body])
        bb = factory.build_backbone(cfg)
        ref = engine.build_model(device="cpu", settings=config.settings(cfg))["backbone"]
        assert list(bb.state_dict()) == list(ref.state_dict()) and bb.out_channels == 256
    with pytest.raises(ValueError, match="CONV_BODY"):
        factory.build_backbone(config.load("c2f", ["MODEL.BACKBONE.CONV_BODY", "R-50-C4"]))
    with pytest.raises(ValueError, match="FCOS_ON"):
        factory.build_rpn(config.load("c2f", ["MODEL.FCOS_ON", False]), 256)
    with pytest.raises(ValueError, match="CONDGRAPH_ON"):
        factory.build_middle_head(config.load("c2f", ["MODEL.MIDDLE_HEAD.CONDGRAPH_ON", False]), 256)
    cfg = config.load("c2f", ["MODEL.ADV.USE_DIS_P5_CON", False])
    cfg.MODEL.ADV.GRL_WEIGHT_P4 = 0.5
    with pytest.raises(ValueError):  # the settings view still refuses what the path does not build
        factory.build_discriminators(cfg)


def test_target_tuples_from_boxlists():
    t = BoxList([[1.0, 2.0, 4.0, 6.0]], (32, 16), "xyxy").convert("xywh")
    t.add_field("labels", torch.tensor([5]))
    targets = [t]
    out = factory.target_tuples(targets)
    assert out[0][0].tolist() == [[1, 2, 4, 6]] and out[0][1].tolist() == [5]
    assert factory.target_tuples(targets) is out  # one plan per batch: the same list maps to the same object
    tup = [(torch.zeros(1, 4), torch.ones(1, dtype=torch.int64))]
    assert factory.target_tuples(tup) is tup and factory.target_tuples(None) is None


def test_pack_symbols_exported_and_arguments_validated_without_device():
    L = _lib.lib()
    assert hasattr(L, "scan_pyramid_pack") and hasattr(L, "scan_pyramid_unpack")
    assert {"scan_pyramid_pack", "scan_pyramid_unpack"} <= set(_lib.SIGNATURES)
    lv = (_lib.LevelDesc * 9)()
    for d in lv:
        d.data, d.h, d.w, d.sn, d.sc, d.sy, d.sx = 64, 2, 2, 16, 4, 2, 1
    rows = ctypes.c_void_p(64)
    with pytest.raises(RuntimeError, match="Cs"):
        _lib.call("scan_pyramid_pack", lv, 1, 1, 5, rows, 4, None)
    with pytest.raises(RuntimeError, match="Cs"):
        _lib.call("scan_pyramid_unpack", rows, 6, lv, 1, 1, 5, None)
    with pytest.raises(RuntimeError, match="n_levels"):
        _lib.call("scan_pyramid_pack", lv, 9, 1, 4, rows, 4, None)
    with pytest.raises(RuntimeError, match="n_levels"):
        _lib.call("scan_pyramid_unpack", rows, 4, lv, 0, 1, 4, None)
    with pytest.raises(RuntimeError, match="null"):
        _lib.call("scan_pyramid_pack", lv, 2, 1, 4, None, 4, None)
    with pytest.raises(RuntimeError, match="null"):
        _lib.call("scan_pyramid_pack", None, 2, 1, 4, rows, 4, None)
    lv[1].data = None
    with pytest.raises(RuntimeError, match="level 1: null"):
        _lib.call("scan_pyramid_unpack", rows, 4, lv, 2, 1, 4, None)


def test_pack_ops_refuse_cpu_tensors():
    x = [torch.zeros(1, 4, 2, 2)]
    with pytest.raises(RuntimeError, match="GPU"):
        ops.pack_levels(x)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.unpack_levels(torch.zeros(4, 4), ops.PyramidShape(1, [(2, 2)]), 4)
    lv = ops.PyramidLevels(torch.zeros(6, 4), ops.PyramidShape(1, [(2, 2), (1, 2)]))
    assert [tuple(t.shape) for t in lv] == [(1, 4, 2, 2), (1, 4, 1, 2)] and lv.intact()
    with pytest.raises(RuntimeError, match="GPU"):
        ops.pack_levels(lv)
    lv[0], lv[1] = lv[1], lv[0]
    assert not lv.intact()

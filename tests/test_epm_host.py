"""Host-side contract of the EPM baseline (no GPU): the config view, the factories, the module parameter layout, what raises,
and the map's torch spelling against the fp64 restatement and the reference-written module fixture."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

import epm_ref
from scan_amd import config, epm, synth
from scan_amd.modeling import discriminator, factory

LEVELS = ("P3", "P4", "P5", "P6", "P7")
DIS_ORDER = ("P7", "P6", "P5", "P4", "P3")
YAMLS = ("da_ga_ca_cityscapes_VGG_16_FPN_4x.yaml", "da_ga_sim10k_VGG_16_FPN_4x_atss.yaml", "da_ga_cityscapes_VGG_16_FPN_4x.yaml")


def _yaml(gold_dir, name):
    return os.path.join(gold_dir, "reference_yaml", name)


@pytest.mark.parametrize("name", YAMLS)
def test_reference_yaml_loads_and_settings_equal_it(gold_dir, name):
    raw = yaml.safe_load(open(_yaml(gold_dir, name)))
    given = raw["MODEL"]["ADV"]
    adv = lambda k: given.get(k, config.EPM_ADV_DEFAULTS[k])  # a key the yaml leaves out keeps the reference's default
    cfg = config.load(_yaml(gold_dir, name))
    s = config.epm_settings(cfg)
    assert s["use_dis_global"] == adv("USE_DIS_GLOBAL") and s["use_dis_center_aware"] == adv("USE_DIS_CENTER_AWARE")
    assert s["center_aware_weight"] == adv("CENTER_AWARE_WEIGHT") and s["center_aware_type"] == adv("CENTER_AWARE_TYPE")
    assert s["ga_dis_lambda"] == adv("GA_DIS_LAMBDA") and s["ca_dis_lambda"] == adv("CA_DIS_LAMBDA")
    for l in LEVELS:
        assert s["use_dis"][l] == adv("USE_DIS_%s" % l)
        assert s["dis_num_convs"][l] == adv("DIS_%s_NUM_CONVS" % l) and s["ca_dis_num_convs"][l] == adv("CA_DIS_%s_NUM_CONVS" % l)
        assert s["grl_weight"][l] == adv("GRL_WEIGHT_%s" % l) and s["ca_grl_weight"][l] == adv("CA_GRL_WEIGHT_%s" % l)
    assert s["rpn"] == ("atss" if raw["MODEL"].get("ATSS_ON") else "fcos")
    assert s["num_classes"] == raw["MODEL"]["ATSS" if s["rpn"] == "atss" else "FCOS"]["NUM_CLASSES"]
    assert s["conv_body"] == raw["MODEL"]["BACKBONE"]["CONV_BODY"]
    if s["rpn"] == "fcos":
        assert s["head"]["reg_ctr_on"] is False  # the yaml leaves the reference's default: centerness on the class tower
    assert s["solver"]["dis"]["lr"] == raw["SOLVER"]["DIS"]["BASE_LR"] and s["solver"]["dis"]["steps"] == (120000, 160000)
    assert s["solver"]["backbone"]["wd"] == raw["SOLVER"]["WEIGHT_DECAY"]
    with pytest.raises(ValueError):  # the SCAN view still refuses them
        config.settings(cfg)


def test_defaults_stay_out_of_the_shipped_views(gold_dir):
    new = set(config.EPM_ADV_DEFAULTS) - set(config.DEFAULTS["MODEL"]["ADV"])  # GRL_WEIGHT_Px is shared with the CKA view
    assert new == set(k for k in config.EPM_ADV_DEFAULTS if not k.startswith("GRL_WEIGHT_"))
    assert "USE_DIS_GLOBAL" not in config.DEFAULTS["MODEL"]["ADV"] and "CA_DIS_LAMBDA" not in config.DEFAULTS["MODEL"]["ADV"]
    assert config.EPM_ADV_DEFAULTS["CENTER_AWARE_WEIGHT"] == 20 and config.EPM_ADV_DEFAULTS["CENTER_AWARE_TYPE"] == "ca_feature"
    assert config.EPM_ADV_DEFAULTS["GA_DIS_LAMBDA"] == 0.01 and config.EPM_ADV_DEFAULTS["CA_DIS_LAMBDA"] == 0.1
    assert all(config.EPM_ADV_DEFAULTS["DIS_%s_NUM_CONVS" % l] == 4 and config.EPM_ADV_DEFAULTS["CA_GRL_WEIGHT_%s" % l] == 0.1
               for l in LEVELS)
    for name in ("c2f", "s2c", "k2c"):
        gold = json.load(open(os.path.join(gold_dir, "cfg_%s.json" % name)))["cfg"]
        assert config.hot_path_view(config.load(name)) == gold
        with pytest.raises(ValueError, match="CONDGRAPH_ON"):  # a SCAN config is no EPM config
            config.epm_settings(config.load(name))


def test_state_dict_layout_equals_the_references(gold_dir):
    z = np.load(os.path.join(gold_dir, "epm_dis_modules.npz"))
    keys, shapes = [str(k) for k in z["state_dict_keys"]], json.loads(str(z["state_dict_shapes"]))
    n = int(z["num_convs"])
    for cls in (discriminator.FCOSDiscriminator, discriminator.FCOSDiscriminator_CA, factory.FCOSDiscriminator, factory.FCOSDiscriminator_CA):
        m = cls(num_convs=n, grad_reverse_lambda=0.02)
        sd = m.state_dict()
        assert list(sd) == keys and [list(v.shape) for v in sd.values()] == shapes, cls
        assert float(m.cls_logits.bias.detach().abs().max()) == 0.0 and 0.005 < float(m.dis_tower[0].weight.detach().std()) < 0.02  # init :44-48
    assert list(discriminator.FCOSDiscriminator(num_convs=0).state_dict()) == ["cls_logits.weight", "cls_logits.bias"]
    sd = synth.epm_discriminator_state_dict("dis_P5", n)
    assert list(sd) == keys


def test_build_discriminators_and_build_model_key_order(gold_dir):
    cfg = config.load(_yaml(gold_dir, YAMLS[0]))
    want = ["dis_%s" % l for l in DIS_ORDER] + ["dis_%s_CA" % l for l in DIS_ORDER]
    dis = factory.build_discriminators(cfg)
    assert list(dis) == want
    assert isinstance(dis["dis_P3"], discriminator.FCOSDiscriminator) and isinstance(dis["dis_P3_CA"], discriminator.FCOSDiscriminator_CA)
    assert dis["dis_P4"].grad_reverse.lambda_ == 0.02 and dis["dis_P4_CA"].center_aware_weight == 20
    cfg2 = config.load(_yaml(gold_dir, YAMLS[0]), ["MODEL.ADV.USE_DIS_P5", False, "MODEL.ADV.DIS_P3_NUM_CONVS", 1])
    dis2 = factory.build_discriminators(cfg2)
    assert list(dis2) == [k for k in want if "P5" not in k] and dis2["dis_P3"].num_convs == 1
    assert list(factory.build_discriminators(config.load(_yaml(gold_dir, YAMLS[1])))) == want[:5]
    assert factory.build_discriminators(config.load("c2f", ["MODEL.ADV.USE_DIS_CON", False])) == {}
    model = factory.build_model(cfg, device="cpu")
    assert list(model) == ["backbone", "fcos"] + want  # no middle head without CONDGRAPH_ON (tools/train_net_da.py:43-48)
    assert model["fcos"].head.reg_ctr_on is False and model["fcos"].mode == "common"
    with pytest.raises(ValueError, match="CONDGRAPH_ON"):
        factory.build_middle_head(cfg, 256)
    with pytest.raises(ValueError, match="CONDGRAPH_ON"):
        factory.build_middle_head(config.load("c2f", ["MODEL.MIDDLE_HEAD.CONDGRAPH_ON", False]), 256)


@pytest.mark.parametrize("opts,key", [
    (["MODEL.ADV.GRL_APPLIED_DOMAIN", "target"], "GRL_APPLIED_DOMAIN"),
    (["MODEL.ADV.PATCH_STRIDE", 2], "PATCH_STRIDE"),
    (["MODEL.ADV.CENTER_AWARE_TYPE", "focal"], "CENTER_AWARE_TYPE"),
    (["MODEL.ADV.USE_DIS_CON", True], "USE_DIS_CON"),
    (["MODEL.MIDDLE_HEAD.CONDGRAPH_ON", True], "CONDGRAPH_ON"),
    (["MODEL.ADV.USE_DIS_OUT", True], "USE_DIS_OUT"),
    (["MODEL.ADV.USE_DIS_GLOBAL", False, "MODEL.ADV.USE_DIS_CENTER_AWARE", False], "USE_DIS_GLOBAL"),
    (["MODEL.ADV.DIS_P4_NUM_CONVS", -1], "DIS_P4_NUM_CONVS"),
    (["TEST.MODE", "precision"], "TEST.MODE"),
    (["MODEL.RETINANET.USE_C5", True], "USE_C5"),
    (["MODEL.FCOS_ON", False], "FCOS_ON"),
])
def test_unbuilt_settings_raise_and_name_their_key(gold_dir, opts, key):
    with pytest.raises(ValueError, match=key):
        config.epm_settings(config.load(_yaml(gold_dir, YAMLS[0]), opts))


def test_unbuilt_module_keywords_raise_and_name_their_key():
    for cls in (discriminator.FCOSDiscriminator, discriminator.FCOSDiscriminator_CA):
        with pytest.raises(ValueError, match="GRL_APPLIED_DOMAIN"):
            cls(grl_applied_domain="target")
        with pytest.raises(ValueError, match="num_convs"):
            cls(num_convs=-1)
    with pytest.raises(ValueError, match="PATCH_STRIDE"):
        discriminator.FCOSDiscriminator(patch_stride=2)
    with pytest.raises(ValueError, match="CENTER_AWARE_TYPE"):
        discriminator.FCOSDiscriminator_CA(center_aware_type="focal")
    for t in ("ca_feature", "ca_loss"):
        assert discriminator.FCOSDiscriminator_CA(center_aware_type=t, center_aware_weight=20).center_aware_type == t


def test_epm_build_model_key_sets_and_trainer_refusals():
    ga = epm.build_model(4, device="cpu")
    assert list(ga) == ["backbone", "fcos"] + ["dis_%s" % l for l in DIS_ORDER]
    both = epm.build_model(4, adv=("ga", "ca"), device="cpu")
    assert list(both) == list(ga) + ["dis_%s_CA" % l for l in DIS_ORDER]
    assert both["fcos"].head.num_fg == 3 and both["fcos"].head.reg_ctr_on is False
    from scan_amd.modeling.atss import ATSSModule
    atss = epm.build_model(2, rpn="atss", device="cpu")
    assert isinstance(atss["fcos"], ATSSModule) and list(atss) == list(ga)
    epm.load_procedural_weights(both)
    sds = synth.epm_state_dicts(4, ("ga", "ca"))
    assert set(sds) == set(both)
    assert torch.equal(both["dis_P3_CA"].cls_logits.weight.detach(), sds["dis_P3_CA"]["cls_logits.weight"])
    assert not torch.equal(sds["dis_P3_CA"]["cls_logits.weight"], sds["dis_P3"]["cls_logits.weight"])
    with pytest.raises(ValueError, match="rpn"):
        epm.build_model(4, rpn="retinanet", device="cpu")
    with pytest.raises(ValueError, match="adv"):
        epm.build_model(4, adv=("out",), device="cpu")
    with pytest.raises(ValueError, match="distributed"):
        epm.EPMTrainer(ga, distributed=True)
    with pytest.raises(ValueError, match="discriminator"):
        epm.EPMTrainer({k: v for k, v in ga.items() if not k.startswith("dis_")})
    tr = epm.EPMTrainer(both)
    assert set(tr.groups) == set(both) and tr.ga_dis_lambda == 0.01 and tr.ca_dis_lambda == 0.1
    assert tr.groups["dis_P3"].lr == tr.settings["solver"]["dis"]["lr"] and tr.groups["fcos"].lr == tr.settings["solver"]["fcos"]["lr"]


def test_map_torch_spelling_agrees_with_restatement_and_fixture(gold_dir):
    """sigmoid(w * max_c sigmoid(cls) * sigmoid(ctr)) in fp32 torch ops against the fp64 restatement (a few ulps of [1/2, 1)) and
    against the maps stored beside the reference modules' answers"""
    z = np.load(os.path.join(gold_dir, "epm_dis_modules.npz"))
    ctr = torch.from_numpy(z["centerness"])[:, 0]
    for fg, w in ((3, 20), (1, 20), (3, 0)):
        cls = torch.from_numpy(z["box_cls_c%d" % fg]).permute(0, 2, 3, 1)
        a32 = torch.sigmoid(float(w) * torch.sigmoid(cls).amax(-1) * torch.sigmoid(ctr))
        a64 = epm_ref.center_aware_map(cls, ctr, w)
        assert float((a32.double() - a64).abs().max()) <= 8 * 2.0 ** -24
        assert float((torch.from_numpy(z["atten_c%d_w%d" % (fg, w)]).double() - a64).abs().max()) <= 8 * 2.0 ** -24
        if w == 0:
            assert torch.equal(a32, torch.full_like(a32, 0.5))


def test_restatement_agrees_with_the_module_fixture(gold_dir):
    """tests/epm_ref.py (fp64, from the formulas) against the reference modules' fp32 answers: losses to 1e-6, d loss / d feature
    to 1e-4 of its largest element"""
    z = np.load(os.path.join(gold_dir, "epm_dis_modules.npz"))
    n, lam = int(z["num_convs"]), float(z["grad_reverse_lambda"])
    feature, ctr = torch.from_numpy(z["feature"]), torch.from_numpy(z["centerness"])
    for c in json.loads(str(z["cases"])):
        sd = synth.epm_discriminator_state_dict("dis_P5" if c["kind"] == "ga" else "dis_P5_CA", n)
        cls = torch.from_numpy(z["box_cls_c%d" % c["fg"]]) if c["kind"] != "ga" else None
        loss, dx = epm_ref.discriminator(feature, sd, n, c["target"], lam, c["kind"], cls, ctr, c["weight"])
        ref = float(z[c["name"] + "/loss"])
        assert abs(float(loss) - ref) <= 1e-6 * abs(ref), c
        if c["full"]:
            g = torch.from_numpy(z[c["name"] + "/d_feature"]).double()
            assert float((dx - g).abs().max()) <= 1e-4 * float(g.abs().max()), c

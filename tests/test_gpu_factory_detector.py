"""GPU parity of the reference-shaped modules (scan_amd/modeling/factory.py): the reference's ``foward_detector``
(engine/trainer.py:20-72) and its three-phase DA iteration (:284-383) restated here in call shape, run on the factories'
modules with ``to_image_list`` images and ``BoxList`` targets, against the reference's fixture (tests/golden/step_128x256.json),
against ``engine.Trainer.step`` on the same weights, and -- in eval mode -- against ``engine.forward_detector``'s detections.

The bars are those of tests/test_gpu_model.py::test_surface_step_matches_engine_and_reference: losses within LOSS_RTOL of the
fixture and within 2e-5 of the engine's, the eight named gradient digests within 2e-3."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-4  # tests/test_gpu_model.py
LAYERS = ("P7", "P6", "P5", "P4", "P3")  # used_feature_layers in the order the reference iterates them
MAP = {"P3": 0, "P4": 1, "P5": 2, "P6": 3, "P7": 4}
DIGESTS = (("backbone", "body.features.28.weight"), ("backbone", "fpn.fpn_inner3.weight"),
           ("fcos", "head.cls_tower.0.weight"), ("fcos", "head.bbox_pred.weight"),
           ("middle_head", "head_out.middle_tower.0.weight"), ("middle_head", "head_in.middle_tower.1.weight"),
           ("dis_P3_CON", "classifier_cls_0.0.weight"), ("dis_P5_CON", "dis_tower.0.weight"))


def _digest(g):
    flat = g.detach().double().reshape(-1).cpu()
    return [flat.sum().item(), flat.abs().sum().item()]


def _cfg(gold_dir):
    """the reference's merged cfg as the fixture holds it (the hot-path keys) + FCOS_ON, which its yaml sets"""
    from scan_amd import config
    cfg = config.Cfg(json.load(open(os.path.join(gold_dir, "cfg_c2f.json")))["cfg"])
    cfg.MODEL.FCOS_ON = True
    return cfg


class ForeignBackbone(torch.nn.Module):
    """a backbone that is not ours: the same features, handed over as a plain list of NCHW-contiguous tensors"""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x):
        return [f.contiguous() for f in self.inner(x)]


def foward_detector(cfg, model, images, targets=None, return_maps=True, mode="source", forward_target=False):
    """reference engine/trainer.py:20-72, call for call"""
    from scan_amd.structures import to_image_list
    with_middle_head = cfg.MODEL.MIDDLE_HEAD.CONDGRAPH_ON
    model_backbone, model_fcos = model["backbone"], model["fcos"]
    images = to_image_list(images)
    features = model_backbone(images.tensors)
    losses = {}
    assert with_middle_head
    features, loss_graph, loss_act_map, return_act_maps = model["middle_head"](
        images, features, targets=targets, return_maps=return_maps, mode=mode, forward_target=forward_target)
    if loss_graph is not None:
        node_loss, consistency_loss = loss_graph
        if consistency_loss is not None and not (isinstance(consistency_loss, (int, float)) and consistency_loss == 0):
            losses["consistency_loss"] = consistency_loss
        if node_loss is not None:
            losses["node_loss"] = node_loss
    if loss_act_map is not None:
        losses["act_loss"] = loss_act_map
    proposals, proposal_losses, score_maps = model_fcos(images, features, targets=targets, return_maps=return_maps,
                                                        act_maps=return_act_maps)
    f = {layer: features[MAP[layer]] for layer in MAP}
    if return_act_maps:
        return_act_maps = {layer: return_act_maps[MAP[layer]] for layer in MAP}
    if model_fcos.training:
        if not targets:
            assert len(proposal_losses) == 1 and proposal_losses["zero"] == 0
        losses.update(proposal_losses)
        return losses, f, return_act_maps
    return proposals


def da_iteration(cfg, model, images_s, targets_s, images_t):
    """reference engine/trainer.py:284-383: (1) generator on source, backward with the graph retained, (2) discriminators on
    source, backward, (3) target pass + discriminators on target, backward.  Gradients accumulate in .grad; no optimizer step."""
    lam = cfg.MODEL.ADV.CON_DIS_LAMBDA
    source_label, target_label = 1.0, 0.0
    out = {}
    for m in model.values():
        m.train()
        m.zero_grad(set_to_none=True)
    loss_dict, features_s, score_maps_s = foward_detector(cfg, model, images_s, targets=targets_s, return_maps=True,
                                                          mode="source")
    loss_dict = {k + "_gs": v for k, v in loss_dict.items()}
    sum(loss_dict.values()).backward(retain_graph=True)
    out.update(loss_dict)
    loss_dict = {}
    for layer in LAYERS:
        loss_dict["loss_adv_%s_CON_ds" % layer] = lam * model["dis_%s_CON" % layer](
            features_s[layer], source_label, score_maps_s[layer], domain="source")
    sum(loss_dict.values()).backward()
    out.update(loss_dict)
    del loss_dict, features_s, score_maps_s
    loss_dict, features_t, score_maps_t = foward_detector(cfg, model, images_t, return_maps=True, mode="target",
                                                          forward_target=False)
    loss_dict = {k + "_gt": v for k, v in loss_dict.items()}
    for layer in LAYERS:
        loss_dict["loss_adv_%s_CON_dt" % layer] = lam * model["dis_%s_CON" % layer](
            features_t[layer], target_label, score_maps_t[layer], domain="target")
    sum(loss_dict.values()).backward()
    out.update(loss_dict)
    return out


@pytest.fixture(scope="module")
def setup(device, gold_dir):
    """gold, cfg, inputs, the engine's losses (Trainer.step, lr 0) and the factory-built model with the same weights"""
    from scan_amd import engine, synth
    from scan_amd.modeling import factory
    from scan_amd.structures import BoxList, to_image_list
    gold = json.load(open(os.path.join(gold_dir, "step_128x256.json")))
    H, W, N = gold["H"], gold["W"], gold["N"]
    imgs_s = synth.synth_images(N, H, W, gold["seeds"]["src"]).to(device)
    imgs_t = synth.synth_images(N, H, W, gold["seeds"]["tgt"]).to(device)
    tg = synth.synth_targets(N, H, W, 8, 12, gold["seeds"]["boxes"])
    emodel = engine.build_model(9, device=device, attn_dropout=0.0)
    engine.load_procedural_weights(emodel)
    eng = {k: float(v) for k, v in engine.Trainer(emodel, base_lr=0.0).step(imgs_s, tg, imgs_t).items()}
    del emodel
    cfg = _cfg(gold_dir)
    model = factory.build_model(cfg, device=device)
    model["middle_head"].multihead_attn.dropout.p = 0.0
    model["middle_head"].multihead_attn.attn_dropout.p = 0.0
    targets = []
    for boxes, labels in tg:
        t = BoxList(boxes, (W, H), mode="xyxy")
        t.add_field("labels", labels)
        targets.append(t)
    return dict(gold=gold, cfg=cfg, eng=eng, model=model, targets=targets, tg=tg,
                images_s=to_image_list(imgs_s), images_t=to_image_list(imgs_t))


def _reset(model):
    from scan_amd import engine
    engine.load_procedural_weights(model)
    model["middle_head"].counter_rnn.counter = -1


def _run(s, model):
    _reset(s["model"])
    out = {k: float(v) for k, v in da_iteration(s["cfg"], model, s["images_s"], s["targets"], s["images_t"]).items()}
    torch.cuda.synchronize()
    return out


def _check_digests(gold, model, names):
    for mk, name_ in names:
        ref = gold["grad_digest"][mk][name_]
        mine = _digest(dict(model[mk].named_parameters())[name_].grad)
        print("digest %s/%s: mine %r ref %r" % (mk, name_, mine, ref[:2]))
        assert abs(mine[1] - ref[1]) <= 2e-3 * ref[1] and abs(mine[0] - ref[0]) <= 2e-3 * ref[1], (mk, name_, mine, ref[:2])


@pytest.fixture(scope="module")
def own_backbone_losses(setup):
    return _run(setup, setup["model"])


def test_reference_loop_on_factory_modules_matches_fixture_and_engine(setup, own_backbone_losses):
    gold, eng, out = setup["gold"], setup["eng"], own_backbone_losses
    assert len(gold["losses"]) == 16 and set(gold["losses"]) <= set(out)
    for k, ref in gold["losses"].items():
        print("%s: factory %.9g engine %.9g fixture %.9g" % (k, out[k], eng[k], ref))
    for k, ref in gold["losses"].items():
        assert abs(out[k] - ref) <= LOSS_RTOL * abs(ref) if ref != 0.0 else out[k] == 0.0, (k, out[k], ref)
        assert abs(out[k] - eng[k]) <= 2e-5 * max(abs(eng[k]), 1e-6), (k, out[k], eng[k])
    _check_digests(gold, setup["model"], DIGESTS)


def test_levels_travel_between_the_modules_without_a_copy(setup):
    from scan_amd import ops
    from scan_amd.modeling import factory
    model = setup["model"]
    for m in model.values():
        m.eval()
    with torch.no_grad():
        feats = model["backbone"](setup["images_s"].tensors)
        assert isinstance(feats, ops.PyramidLevels) and len(feats) == 5 and feats.intact()
        assert all(f.shape[1] == 256 and f.is_contiguous(memory_format=torch.channels_last) for f in feats)
        rows, shape = ops.pack_levels(feats)
        assert rows.data_ptr() == feats.rows.data_ptr() == feats[0].data_ptr()
        out, _, _, maps = model["middle_head"](setup["images_s"], feats)
        assert isinstance(out, ops.PyramidLevels) and isinstance(maps, ops.PyramidLevels) and maps[0].shape[1] == 9
        # a level view is taken by the discriminator as the rows it is: same storage
        r, lshape = factory._level_rows(out[2])
        assert r.data_ptr() == out[2].data_ptr() and tuple(r.shape) == (shape.row_off[3] - shape.row_off[2], 256)
        a, _ = factory._level_rows(maps[2])
        assert a.data_ptr() == maps[2].data_ptr() and a.shape[1] == 9 and lshape == shape.level(2)


def test_foreign_backbone_goes_through_the_pack_kernel(setup, own_backbone_losses):
    """the middle head is fed a plain list of NCHW-contiguous clones: pack kernel forward, unpack kernel backward"""
    gold, model = setup["gold"], dict(setup["model"])
    model["backbone"] = ForeignBackbone(setup["model"]["backbone"])
    out = _run(setup, model)
    for k, v in own_backbone_losses.items():
        print("%s: foreign %.9g own %.9g" % (k, out[k], v))
    for k, v in own_backbone_losses.items():
        assert abs(out[k] - v) <= 2e-5 * max(abs(v), 1e-6), (k, out[k], v)
    model["backbone"] = setup["model"]["backbone"]
    _check_digests(gold, model, [d for d in DIGESTS if d[0] == "backbone"])


@pytest.mark.parametrize("mode", ["common", "precision", "light"])
def test_eval_returns_the_engine_s_detections_as_boxlists(setup, device, mode):
    from scan_amd import engine, synth
    from scan_amd.modeling import factory
    from scan_amd.structures import BoxList, to_image_list
    cfg = setup["cfg"].clone()
    cfg.TEST.MODE = mode
    sds = synth.shifted_state_dicts(9)  # weights with which every test mode returns detections (tests/test_gpu_model.py)
    model = factory.build_model(cfg, device=device)
    emodel = engine.build_model(device=device, settings=dict(engine.CONFIGS["c2f"], test_mode=mode))
    engine.load_state_dicts(model, sds)
    engine.load_state_dicts(emodel, sds)
    # a ragged batch: boxes are clipped to each image's own size
    imgs = to_image_list([t.to(device) for t in synth.synth_image_list([(120, 250), (128, 256)], 3234)], 32)
    want = engine.inference(emodel, imgs)
    for m in model.values():
        m.eval()
    with torch.no_grad():
        got = foward_detector(cfg, model, imgs, targets=None, return_maps=False)
    assert len(got) == len(want) == 2 and sum(len(b) for b in got) > 0
    for b, (boxes, scores, labels), (h, w) in zip(got, want, imgs.image_sizes):
        assert isinstance(b, BoxList) and b.mode == "xyxy" and b.size == (w, h) and sorted(b.fields()) == ["labels", "scores"]
        assert torch.equal(b.bbox, boxes) and torch.equal(b.get_field("scores"), scores)
        assert torch.equal(b.get_field("labels"), labels)
        assert len(b) == 0 or (b.bbox[:, 2].max() <= w - 1 and b.bbox[:, 3].max() <= h - 1)

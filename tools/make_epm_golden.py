"""Writes the EPM-baseline fixtures under tests/golden/: the REFERENCE's answers for its GA / CA discriminator modules
(epm_dis_modules.npz) and for one full adaptation iteration without a middle head (epm_ga_64x96, epm_ga_ca_64x96,
epm_ga_atss_64x96: .json).  Runs on a CPU machine that has the reference checkout (oracle/ref_harness.py); the fixtures hold
data only.

    python tools/make_epm_golden.py

What is run: the reference's own FCOSDiscriminator / FCOSDiscriminator_CA (autograd), build_backbone / build_rpn, and the
adaptation loop of engine/trainer.py:266-386 restated call for call (importing that file pulls the data loaders) with
CONDGRAPH_ON False.  The loop's CA branch cannot run as it stands (it indexes the ``None`` foward_detector returns for the act
maps, and the head groups its score maps by type, not by level): the CA fixture calls the CA modules with each level's
{"box_cls", "centerness"}, detached, in the loop's order and with the loop's weights.

The ATSS fixture uses the boxes of tools/make_atss_golden.py's atss_64x96 case and re-asserts that generator's tie-free
conditions, so the reference's assignment does not depend on how torch.topk / torch.max break ties.

A 256 -> 256 tower conv's weight gradient is 590 K floats; the module fixture keeps every parameter gradient in full except
those, of which it keeps every SAMPLE_STRIDE-th element beside the sum and the abs-sum (committed files stay under 1 MiB).
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
np.float = float  # rpn/anchor_generator.py:251 (numpy < 1.20 spelling)

from oracle import ref_harness  # noqa: E402
from scan_amd import synth  # noqa: E402
import epm_ref  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
LEVELS = ("P3", "P4", "P5", "P6", "P7")
DIS_ORDER = ("P7", "P6", "P5", "P4", "P3")
SAMPLE_STRIDE = 251
MODULE_CONVS, MODULE_LAMBDA = 2, 0.02

# (name, kind, target, foreground classes, CENTER_AWARE_WEIGHT, keep d_feature in full)
MODULE_CASES = [
    ("ga_t1", "ga", 1.0, 0, 0, True), ("ga_t0", "ga", 0.0, 0, 0, False),
    ("caf_t1_c3_w20", "ca_feature", 1.0, 3, 20, True), ("caf_t0_c1_w20", "ca_feature", 0.0, 1, 20, True),
    ("cal_t1_c1_w20", "ca_loss", 1.0, 1, 20, False), ("cal_t0_c3_w20", "ca_loss", 0.0, 3, 20, True),
    ("caf_t0_c3_w0", "ca_feature", 0.0, 3, 0, False), ("cal_t1_c3_w0", "ca_loss", 1.0, 3, 0, False),
]


def digest(g):
    flat = g.detach().double().reshape(-1)
    idx = torch.linspace(0, flat.numel() - 1, 8).long()
    return [flat.sum().item(), flat.abs().sum().item()] + flat[idx].tolist()


def grad_digest(named):
    return {k: digest(p.grad) for k, p in named if p.grad is not None}


def module_inputs():
    g = torch.Generator().manual_seed(2024)
    N, h, w = 2, 6, 10
    return dict(feature=torch.randn(N, 256, h, w, generator=g),
                box_cls_c3=torch.randn(N, 3, h, w, generator=g) * 2.0 - 1.0, box_cls_c1=torch.randn(N, 1, h, w, generator=g) * 2.0 - 1.0,
                centerness=torch.randn(N, 1, h, w, generator=g) * 1.5)


def make_modules():
    from fcos_core.modeling.discriminator.fcos_head_discriminator import FCOSDiscriminator
    from fcos_core.modeling.discriminator.fcos_head_discriminator_CA import FCOSDiscriminator_CA
    inp = module_inputs()
    out = {k: v.numpy() for k, v in inp.items()}
    out["num_convs"], out["grad_reverse_lambda"], out["sample_stride"] = np.array(MODULE_CONVS), np.array(MODULE_LAMBDA), np.array(SAMPLE_STRIDE)
    out["cases"] = np.array(json.dumps([dict(name=n, kind=k, target=t, fg=c, weight=w, full=f) for n, k, t, c, w, f in MODULE_CASES]))
    keys = None
    for name, kind, target, fg, weight, full in MODULE_CASES:
        if kind == "ga":
            dis = FCOSDiscriminator(num_convs=MODULE_CONVS, grad_reverse_lambda=MODULE_LAMBDA, grl_applied_domain="both")
            sd = synth.epm_discriminator_state_dict("dis_P5", MODULE_CONVS)
        else:
            dis = FCOSDiscriminator_CA(num_convs=MODULE_CONVS, grad_reverse_lambda=MODULE_LAMBDA, center_aware_weight=weight,
                                       center_aware_type=kind, grl_applied_domain="both")
            sd = synth.epm_discriminator_state_dict("dis_P5_CA", MODULE_CONVS)
        missing, unexpected = dis.load_state_dict(sd, strict=False)
        assert not missing and not unexpected, (missing, unexpected)
        this = [(k, tuple(v.shape)) for k, v in dis.state_dict().items()]
        assert keys is None or keys == this  # both modules hold the same parameters
        keys = this
        x = inp["feature"].clone().requires_grad_(True)
        domain = "source" if target == 1.0 else "target"
        if kind == "ga":
            loss = dis(x, target, domain=domain)
        else:
            maps = {"box_cls": inp["box_cls_c%d" % fg], "centerness": inp["centerness"]}
            loss = dis(x, target, maps, domain=domain)
            if ("atten_c%d_w%d" % (fg, weight)) not in out:  # the map's formula in fp32 torch ops on the CPU (the module keeps
                # its own in a local); the module's loss and gradients above pin it
                out["atten_c%d_w%d" % (fg, weight)] = epm_ref.center_aware_map_fp32(
                    maps["box_cls"].permute(0, 2, 3, 1), maps["centerness"][:, 0], weight).numpy()
        loss.backward()
        r_loss, r_dx = epm_ref.discriminator(inp["feature"], sd, MODULE_CONVS, target, MODULE_LAMBDA, kind,
                                             maps["box_cls"] if kind != "ga" else None, inp["centerness"], weight)
        loss = loss.detach()
        assert abs(float(r_loss) - float(loss)) <= 1e-5 * abs(float(loss)), (name, float(r_loss), float(loss))
        assert float((r_dx - x.grad.double()).abs().max()) <= 1e-4 * float(x.grad.abs().max()), name
        out[name + "/loss"] = np.array(float(loss), np.float64)
        out[name + "/d_feature_digest"] = np.array(digest(x.grad))
        if full:
            out[name + "/d_feature"] = x.grad.numpy()
        for k, p in dis.named_parameters():
            g = p.grad
            if g.numel() > 100000:
                out["%s/grad_sample/%s" % (name, k)] = g.reshape(-1)[::SAMPLE_STRIDE].numpy().copy()
                out["%s/grad_digest/%s" % (name, k)] = np.array(digest(g))
            else:
                out["%s/grad/%s" % (name, k)] = g.numpy().copy()
        print("%-16s loss %.7f  |d_feature| max %.3e  (fp64 restatement: loss rel %.1e)"
              % (name, float(loss), float(x.grad.abs().max()), abs(float(r_loss) - float(loss)) / abs(float(loss))))
    out["state_dict_keys"] = np.array([k for k, _ in keys])
    out["state_dict_shapes"] = np.array(json.dumps([list(s) for _, s in keys]))
    path = os.path.join(GOLD, "epm_dis_modules.npz")
    np.savez_compressed(path, **out)
    print("epm_dis_modules.npz: %d bytes" % os.path.getsize(path))
    assert os.path.getsize(path) < (1 << 20)


# ----------------------------------------------------------------------------- one adaptation iteration
def build_reference_model(cfg, adv):
    from fcos_core.modeling.backbone import build_backbone
    from fcos_core.modeling.discriminator.fcos_head_discriminator import FCOSDiscriminator
    from fcos_core.modeling.discriminator.fcos_head_discriminator_CA import FCOSDiscriminator_CA
    from fcos_core.modeling.rpn.rpn import build_rpn
    A = cfg.MODEL.ADV
    model = {"backbone": build_backbone(cfg), "fcos": build_rpn(cfg, 256)}
    for lvl in DIS_ORDER:  # tools/train_net_da.py:69-99
        model["dis_%s" % lvl] = FCOSDiscriminator(
            patch_stride=A.PATCH_STRIDE, num_convs=A["DIS_%s_NUM_CONVS" % lvl], grad_reverse_lambda=A["GRL_WEIGHT_%s" % lvl],
            grl_applied_domain=A.GRL_APPLIED_DOMAIN)
    if "ca" in adv:
        for lvl in DIS_ORDER:  # :100-131
            model["dis_%s_CA" % lvl] = FCOSDiscriminator_CA(
                num_convs=A["CA_DIS_%s_NUM_CONVS" % lvl], grad_reverse_lambda=A["CA_GRL_WEIGHT_%s" % lvl],
                center_aware_weight=A.CENTER_AWARE_WEIGHT, center_aware_type=A.CENTER_AWARE_TYPE,
                grl_applied_domain=A.GRL_APPLIED_DOMAIN)
    lf = model["fcos"].loss_evaluator.cls_loss_func  # sigmoid_focal_loss_cpu indexes gamma / alpha
    lf.gamma, lf.alpha = [lf.gamma], [lf.alpha]
    return model


def forward_detector(cfg, model, images, targets=None):
    """engine/trainer.py:20-72 with with_middle_head False; the third value is the head's score maps (the reference returns the
    act maps there: None)"""
    from fcos_core.structures.image_list import to_image_list
    images = to_image_list(images)
    features = model["backbone"](images.tensors)
    if cfg.MODEL.ATSS_ON:  # the reference's ATSSModule.forward has no act_maps argument
        _, losses, score_maps = model["fcos"](images, features, targets=targets, return_maps=True)
    else:
        _, losses, score_maps = model["fcos"](images, features, targets=targets, return_maps=True, act_maps=None)
    return losses, dict(zip(LEVELS, features)), score_maps


def da_iteration(cfg, model, images_s, targets_s, images_t, adv):
    """engine/trainer.py:266-386 for USE_DIS_GLOBAL (/ USE_DIS_CENTER_AWARE), without optimizers"""
    A = cfg.MODEL.ADV
    out = {}
    for m in model.values():
        m.train()
        m.zero_grad()
    loss_dict, feat_s, maps_s = forward_detector(cfg, model, images_s, targets_s)
    loss_dict = {k + "_gs": v for k, v in loss_dict.items()}
    sum(loss_dict.values()).backward(retain_graph=True)
    out.update({k: float(v) for k, v in loss_dict.items()})

    def adversarial(feats, maps, label, domain, tag):
        ld = {}
        for lvl in DIS_ORDER:
            i = LEVELS.index(lvl)
            ld["loss_adv_%s_%s" % (lvl, tag)] = A.GA_DIS_LAMBDA * model["dis_%s" % lvl](feats[lvl], label, domain=domain)
            if "ca" in adv:
                sm = {"box_cls": maps["box_cls"][i].detach(), "centerness": maps["centerness"][i].detach()}
                ld["loss_adv_%s_CA_%s" % (lvl, tag)] = A.CA_DIS_LAMBDA * model["dis_%s_CA" % lvl](feats[lvl], label, sm, domain=domain)
        return ld

    ld = adversarial(feat_s, maps_s, 1.0, "source", "ds")
    sum(ld.values()).backward()
    out.update({k: float(v) for k, v in ld.items()})
    loss_dict, feat_t, maps_t = forward_detector(cfg, model, images_t, None)
    ld = {k + "_gt": v for k, v in loss_dict.items()}
    ld.update(adversarial(feat_t, maps_t, 0.0, "target", "dt"))
    sum(ld.values()).backward()
    out.update({k: float(v) for k, v in ld.items()})
    return out


def make_step(name, rpn, adv, K, H=64, W=96, N=2):
    yaml_name = {"fcos": "../epm/da_ga_ca_cityscapes_VGG_16_FPN_4x.yaml" if "ca" in adv else "../epm/da_ga_cityscapes_VGG_16_FPN_4x.yaml",
                 "atss": "../epm/da_ga_sim10k_VGG_16_FPN_4x_atss.yaml"}[rpn]
    extra = ["MODEL.FCOS.NUM_CLASSES", K] + (["MODEL.ATSS.NUM_CLASSES", K] if rpn == "atss" else [])
    cfg = ref_harness.make_cfg(extra, yaml_name=yaml_name)
    assert bool(cfg.MODEL.ATSS_ON) == (rpn == "atss") and not cfg.MODEL.MIDDLE_HEAD.CONDGRAPH_ON
    assert bool(cfg.MODEL.ADV.USE_DIS_CENTER_AWARE) == ("ca" in adv) and cfg.MODEL.ADV.USE_DIS_GLOBAL
    model = build_reference_model(cfg, adv)
    sds = synth.epm_state_dicts(K, adv)
    for k, m in model.items():
        missing, unexpected = m.load_state_dict(sds[k], strict=False)
        missing = [n for n in missing if not n.startswith("anchor_generator.")]  # the ATSS module's anchor buffers: no parameters
        assert not missing and not unexpected, (k, missing, unexpected)
    imgs_s, imgs_t = synth.synth_images(N, H, W, 1234), synth.synth_images(N, H, W, 2234)
    rec = {"H": H, "W": W, "N": N, "num_classes": K, "rpn": rpn, "adv": list(adv), "seeds": {"src": 1234, "tgt": 2234}}
    if rpn == "atss":
        import atss_ref
        import make_atss_golden
        c = make_atss_golden.CASES["atss_64x96"]
        assert c["image_hw"] == (H, W) and c["num_classes"] == K and len(c["boxes"]) == N
        tg = [(torch.tensor(b, dtype=torch.float32), torch.tensor(l)) for b, l in zip(c["boxes"], c["labels"])]
        sizes = [(-(-H // s), -(-W // s)) for s in atss_ref.STRIDES]
        ref_labels, _, details = atss_ref.assign(N, sizes, tg, topk=int(cfg.MODEL.ATSS.TOPK))
        rec["contested"] = int(make_atss_golden.check_conditions(name, c, sizes, details, ref_labels))  # the tie-free conditions
        rec["boxes"], rec["labels"] = c["boxes"], c["labels"]
    else:
        tg = synth.synth_targets(N, H, W, K - 1, 6, 4321)
        rec["seeds"]["boxes"], rec["boxes_per_img"] = 4321, 6
    targets = ref_harness.make_targets([b for b, _ in tg], [l for _, l in tg], (H, W))
    rec["losses"] = da_iteration(cfg, model, imgs_s, targets, imgs_t, adv)
    rec["grad_digest"] = {mk: grad_digest(m.named_parameters()) for mk, m in model.items()}
    with open(os.path.join(GOLD, name + ".json"), "w") as f:
        json.dump(rec, f)
    print(name, {k: round(v, 6) for k, v in rec["losses"].items()})


if __name__ == "__main__":
    ref_harness.setup()
    todo = sys.argv[1:] or ["modules", "epm_ga_64x96", "epm_ga_ca_64x96", "epm_ga_atss_64x96"]
    if "modules" in todo:
        make_modules()
    if "epm_ga_64x96" in todo:
        make_step("epm_ga_64x96", "fcos", ("ga",), 4)
    if "epm_ga_ca_64x96" in todo:
        make_step("epm_ga_ca_64x96", "fcos", ("ga", "ca"), 4)
    if "epm_ga_atss_64x96" in todo:
        make_step("epm_ga_atss_64x96", "atss", ("ga",), 2)

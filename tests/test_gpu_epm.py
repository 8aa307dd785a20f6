"""The EPM baseline on the GPU against the reference's answers (tools/make_epm_golden.py): the GA / CA discriminator modules
(tests/golden/epm_dis_modules.npz), forward_pair against the two single-domain calls, one full adaptation iteration of
epm.EPMTrainer for GA, GA + CA and GA on the ATSS head (epm_*_64x96.json), bit-reproducible steps in deterministic mode, and
eval-mode forward_detector."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-4  # the project's loss contract
DIGEST_BAR = 2e-3  # every gradient digest, the VGG configs' bar (tests/test_gpu_model.py)
MODES = ("fp32", "bf16x6")
STEP_FIXTURES = ("epm_ga_64x96", "epm_ga_ca_64x96", "epm_ga_atss_64x96")


def _digest(g):
    flat = g.detach().double().reshape(-1).cpu()
    idx = torch.linspace(0, flat.numel() - 1, 8).long()
    return [flat.sum().item(), flat.abs().sum().item()] + flat[idx].tolist()


def _conv_bar(mode):
    """tests/test_gpu_kernels.py::test_conv2d_fwd_bwd: rtol 1e-4, atol tol * max(1, max |ref|)"""
    return 1e-4 if mode == "bf16x3" else 2e-5


def _close(mine, ref, tol, what):
    """test_conv2d_fwd_bwd's bar, and -- these gradients are ~1e-5, far below the bar's floor of max(1, .) -- the same bar without
    the floor, widened 5x for the chain it crosses here (three convs and two GroupNorms, forward and backward, where the conv test
    crosses one conv): |mine - ref| <= 1e-4 |ref| + 5 tol max |ref|"""
    mine, ref = np.asarray(mine, np.float64), np.asarray(ref, np.float64)
    scale = float(np.abs(ref).max())
    np.testing.assert_allclose(mine, ref, rtol=1e-4, atol=tol * max(1.0, scale), err_msg=what)
    err = np.abs(mine - ref) - 1e-4 * np.abs(ref)
    assert float(err.max()) <= 5 * tol * scale, (what, float(err.max()), scale)


def _rows(t, device):
    """[N, C, h, w] -> [N h w, C] rows on the device"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous().to(device)


def _module(kind, n, lam, weight, device):
    from scan_amd import synth
    from scan_amd.modeling import discriminator
    if kind == "ga":
        m = discriminator.FCOSDiscriminator(num_convs=n, grad_reverse_lambda=lam)
        m.load_state_dict(synth.epm_discriminator_state_dict("dis_P5", n))
    else:
        m = discriminator.FCOSDiscriminator_CA(num_convs=n, grad_reverse_lambda=lam, center_aware_weight=weight, center_aware_type=kind)
        m.load_state_dict(synth.epm_discriminator_state_dict("dis_P5_CA", n))
    m.to(device)
    for p in m.parameters():
        if p.dim() == 4:
            p.data = p.data.contiguous(memory_format=torch.channels_last)
    return m


# ----------------------------------------------------------------------------- 1. the modules against the reference's
@pytest.mark.parametrize("mode", MODES)
def test_modules_match_reference(device, gold_dir, mode, monkeypatch):
    from scan_amd import ops
    monkeypatch.setattr(ops, "CONV_MODE", mode)
    tol = _conv_bar(mode)
    z = np.load(os.path.join(gold_dir, "epm_dis_modules.npz"))
    n, lam, stride = int(z["num_convs"]), float(z["grad_reverse_lambda"]), int(z["sample_stride"])
    feature = torch.from_numpy(z["feature"])
    N, _, h, w = feature.shape
    shape = ops.PyramidShape(N, [(h, w)])
    for c in json.loads(str(z["cases"])):
        name = c["name"]
        m = _module(c["kind"], n, lam, c["weight"], device)
        x = _rows(feature, device).requires_grad_(True)
        domain = "source" if c["target"] == 1.0 else "target"
        if c["kind"] == "ga":
            loss = m(x, c["target"], domain=domain, shape=shape)
        else:
            # the score maps as the head hands them over: class logits in the first C columns of a 4-wide conv output (garbage
            # behind them), centerness as a column of an 8-wide one
            cls = torch.full((x.shape[0], 4), 1e30, device=device)
            cls[:, :c["fg"]] = _rows(torch.from_numpy(z["box_cls_c%d" % c["fg"]]), device)
            ctr = torch.full((x.shape[0], 8), float("nan"), device=device)
            ctr[:, 4] = _rows(torch.from_numpy(z["centerness"]), device)[:, 0]
            loss = m(x, c["target"], {"box_cls": cls[:, :c["fg"]], "centerness": ctr[:, 4]}, domain=domain, shape=shape)
        loss.backward()
        loss = loss.detach()
        ref = float(z[name + "/loss"])
        print("%s %s: loss %.7f (reference %.7f)" % (mode, name, float(loss), ref))
        assert abs(float(loss) - ref) <= LOSS_RTOL * abs(ref), (mode, name, float(loss), ref)
        dref = z[name + "/d_feature_digest"]
        mine = _digest(x.grad)
        assert max(abs(mine[0] - dref[0]), abs(mine[1] - dref[1])) <= 1e-3 * dref[1], (mode, name, mine[:2], dref[:2])
        if c["full"]:
            _close(x.grad.cpu().numpy(), _rows(torch.from_numpy(z[name + "/d_feature"]), "cpu").numpy(), tol, (mode, name, "d_feature"))
        for k, p in m.named_parameters():
            if name + "/grad/" + k in z.files:
                btol = 2e-5 if k.endswith("bias") else tol
                _close(p.grad.cpu().numpy(), z[name + "/grad/" + k], btol, (mode, name, k))
            else:
                _close(p.grad.cpu().reshape(-1)[::stride].numpy(), z["%s/grad_sample/%s" % (name, k)], tol, (mode, name, k))
                dref, mine = z["%s/grad_digest/%s" % (name, k)], _digest(p.grad)
                assert max(abs(mine[0] - dref[0]), abs(mine[1] - dref[1])) <= 1e-3 * dref[1], (mode, name, k, mine[:2], dref[:2])


# ----------------------------------------------------------------------------- 2. forward_pair == the two single-domain calls
@pytest.mark.parametrize("kind", ["ga", "ca_feature", "ca_loss"])
def test_forward_pair_equals_the_two_calls(device, kind):
    """values and every gradient; the two schedules sum the same products in another order (one weight-gradient launch over both
    images against two launches added by autograd): 1e-5 of the largest element"""
    from scan_amd import ops
    g = torch.Generator().manual_seed(3)
    N, h, w, C = 2, 6, 10, 3
    feature = torch.randn(N, 256, h, w, generator=g)
    cls = _rows(torch.randn(N, C, h, w, generator=g) * 2.0, device)
    ctr = _rows(torch.randn(N, 1, h, w, generator=g), device)[:, 0]
    full, one = ops.PyramidShape(N, [(h, w)]), ops.PyramidShape(1, [(h, w)])
    m = _module(kind, 2, 0.1, 20.0, device)
    hw = h * w
    res = []
    for paired in (True, False):
        m.zero_grad()
        x = _rows(feature, device).requires_grad_(True)
        if paired:
            if kind == "ga":
                ls, lt = m.forward_pair(x, full, 1)
            else:
                ls, lt = m.forward_pair(x, ops.center_aware_map(cls, ctr, C, 20.0), full, 1)
        elif kind == "ga":
            ls, lt = m(x[:hw], 1.0, domain="source", shape=one), m(x[hw:], 0.0, domain="target", shape=one)
        else:
            ls = m(x[:hw], 1.0, {"box_cls": cls[:hw], "centerness": ctr[:hw]}, domain="source", shape=one)
            lt = m(x[hw:], 0.0, {"box_cls": cls[hw:], "centerness": ctr[hw:]}, domain="target", shape=one)
        (ls + 0.5 * lt).backward()
        res.append((float(ls.detach()), float(lt.detach()), x.grad.cpu(), {k: p.grad.cpu().clone() for k, p in m.named_parameters()}))
    a, b = res
    assert abs(a[0] - b[0]) <= 1e-6 * abs(b[0]) and abs(a[1] - b[1]) <= 1e-6 * abs(b[1])
    assert float((a[2] - b[2]).abs().max()) <= 1e-5 * float(b[2].abs().max())
    for k in a[3]:
        assert float((a[3][k] - b[3][k]).abs().max()) <= 1e-5 * float(b[3][k].abs().max()), k


# ----------------------------------------------------------------------------- 3. one iteration against the reference's loop
def _step_inputs(gold, device):
    from scan_amd import synth
    H, W, N = gold["H"], gold["W"], gold["N"]
    imgs_s = synth.synth_images(N, H, W, gold["seeds"]["src"]).to(device)
    imgs_t = synth.synth_images(N, H, W, gold["seeds"]["tgt"]).to(device)
    if "boxes" in gold:
        tg = [(torch.tensor(b, dtype=torch.float32), torch.tensor(l)) for b, l in zip(gold["boxes"], gold["labels"])]
    else:
        tg = synth.synth_targets(N, H, W, gold["num_classes"] - 1, gold["boxes_per_img"], gold["seeds"]["boxes"])
    return imgs_s, tg, imgs_t


def _settings(gold):
    """the reference yaml the fixture was generated from (stored byte for byte under tests/golden/reference_yaml/), with the
    fixture's class count"""
    from scan_amd import config
    name = "da_ga_sim10k_VGG_16_FPN_4x_atss.yaml" if gold["rpn"] == "atss" else \
        "da_ga_ca_cityscapes_VGG_16_FPN_4x.yaml" if "ca" in gold["adv"] else "da_ga_cityscapes_VGG_16_FPN_4x.yaml"
    path = os.path.join(os.path.dirname(__file__), "golden", "reference_yaml", name)
    return config.epm_settings(config.load(path, ["MODEL.%s.NUM_CLASSES" % gold["rpn"].upper(), gold["num_classes"]]))


def _run_step(gold, device, paired=True):
    from scan_amd import epm
    s = _settings(gold)
    model = epm.build_model(settings=s, device=device)
    epm.load_procedural_weights(model)
    trainer = epm.EPMTrainer(model, settings=s)
    trainer.paired = paired
    for g in trainer.groups.values():  # the gradients are read after the step: keep the parameters where they are
        g.lr = 0.0
    imgs_s, tg, imgs_t = _step_inputs(gold, device)
    losses = {k: float(v.detach()) for k, v in trainer.step(imgs_s, tg, imgs_t).items()}
    torch.cuda.synchronize()
    return model, losses


def _check_step(gold, model, losses, tag):
    assert set(losses) == set(gold["losses"]), (tag, sorted(set(losses) ^ set(gold["losses"])))
    for k, ref in gold["losses"].items():
        print("%s %-22s %.7f (reference %.7f)" % (tag, k, losses[k], ref))
        assert (losses[k] == 0.0) if ref == 0.0 else abs(losses[k] - ref) <= LOSS_RTOL * abs(ref), (tag, k, losses[k], ref)
    errs = []
    for mk, m in model.items():
        for name, p in m.named_parameters():
            ref = gold["grad_digest"][mk].get(name)
            if ref is None:
                assert not p.requires_grad, (tag, mk, name)
                continue
            mine = _digest(p.grad)
            if ref[1] / p.numel() < 1e-7:  # a gradient that is zero up to rounding (a level's Scale without positives)
                assert mine[1] / p.numel() < 1e-6, (tag, mk, name, mine[1])
                continue
            errs.append((max(abs(mine[1] - ref[1]), abs(mine[0] - ref[0])) / max(ref[1], 1e-3), mk + "/" + name))
    errs.sort(reverse=True)
    print("%s: %d gradient digests, worst (sum / abs-sum, relative to abs-sum): %s"
          % (tag, len(errs), ", ".join("%.2e %s" % e for e in errs[:5])))
    assert errs and errs[0][0] <= DIGEST_BAR, (tag, errs[:5])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fixture", STEP_FIXTURES)
def test_step_matches_reference(device, gold_dir, fixture, mode, monkeypatch):
    """one iteration (2 source + 2 target frames at 64x96, VGG body, procedural weights) as ONE pyramid and one backward against
    the reference's three backward calls: every loss within 1e-4, every gradient digest within 2e-3"""
    from scan_amd import ops
    monkeypatch.setattr(ops, "CONV_MODE", mode)
    gold = json.load(open(os.path.join(gold_dir, fixture + ".json")))
    model, losses = _run_step(gold, device)
    _check_step(gold, model, losses, "%s %s" % (fixture, mode))


def test_two_pass_step_matches_reference(device, gold_dir):
    """the schedule for batches whose padded shapes differ (source pass, target pass, one backward) on the GA + CA fixture"""
    gold = json.load(open(os.path.join(gold_dir, "epm_ga_ca_64x96.json")))
    model, losses = _run_step(gold, device, paired=False)
    _check_step(gold, model, losses, "epm_ga_ca_64x96 two-pass")


# ----------------------------------------------------------------------------- 4. deterministic mode
def test_two_seeded_steps_are_bit_reproducible(device, gold_dir):
    """scan_tune deterministic = 1 (SCAN_TUNE=deterministic=1): two runs of two steps from the same weights and batches end with
    the same bits in every loss and every parameter"""
    from scan_amd import epm, ops, synth
    gold = json.load(open(os.path.join(gold_dir, "epm_ga_ca_64x96.json")))
    old = ops.set_deterministic(True)
    try:
        runs = []
        for _ in range(2):
            s = _settings(gold)
            model = epm.build_model(settings=s, device=device)
            epm.load_procedural_weights(model)
            trainer = epm.EPMTrainer(model, settings=s)
            out = []
            for it in range(2):
                imgs_s = synth.synth_images(2, 64, 96, 1234 + 17 * it).to(device)
                imgs_t = synth.synth_images(2, 64, 96, 2234 + 17 * it).to(device)
                tg = synth.synth_targets(2, 64, 96, gold["num_classes"] - 1, 6, 4321 + 17 * it)
                losses = trainer.step(imgs_s, tg, imgs_t)
                out.append({k: v.detach().cpu().clone() for k, v in losses.items()})
            torch.cuda.synchronize()
            runs.append((out, {mk: [p.detach().cpu().clone() for p in m.parameters()] for mk, m in model.items()}))
    finally:
        ops.set_deterministic(old)
    (la, pa), (lb, pb) = runs
    for a, b in zip(la, lb):
        assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    moved = 0
    for mk in pa:
        for p, q in zip(pa[mk], pb[mk]):
            assert torch.equal(p, q), mk
        moved += mk.startswith("dis_")
    sd = synth.epm_state_dicts(gold["num_classes"], ("ga", "ca"))
    assert not torch.equal(pa["dis_P3_CA"][0], sd["dis_P3_CA"]["dis_tower.0.weight"])  # the steps did train
    assert moved == 10


# ----------------------------------------------------------------------------- 5. eval mode
@pytest.mark.parametrize("rpn", ["fcos", "atss"])
def test_eval_forward_detector_is_the_heads_own_answer(device, rpn):
    from scan_amd import engine, epm, ops, synth
    K = 4 if rpn == "fcos" else 2
    model = epm.build_model(K, rpn=rpn, device=device)
    sds = synth.epm_state_dicts(K, ("ga",))
    sds["fcos"]["head.cls_logits.bias"] = sds["fcos"]["head.cls_logits.bias"] + synth.INF2_SHIFT["cls_bias"]
    engine.load_state_dicts(model, sds)
    for m in model.values():
        m.eval()
    images = synth.synth_images(2, 64, 96, 99).to(device)
    with torch.no_grad():
        dets = epm.forward_detector(model, images)
        rows, shape = model["backbone"](images)
        want, _ = model["fcos"]([(64, 96)] * 2, rows, shape)
    assert len(dets) == len(want) == 2 and sum(len(d[1]) for d in dets) > 0
    for d, w_ in zip(dets, want):
        assert all(torch.equal(a, b) for a, b in zip(d, w_))
    ops.invalidate_weight_planes()

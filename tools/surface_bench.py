#!/usr/bin/env python
"""What the drop-in operator surface costs beside the engine: the SAME DA iteration through scan_amd.surface (NCHW tensors, one
module call per level, scan_amd.layers on the C++ autograd operators -- the call shape of the reference's module files) and
through scan_amd.engine (one row matrix per pyramid, one launch per layer), ms/step and kernel launches/step, plus a per-operator
table: one layer's forward + backward through layers.Conv2d per level vs ops.conv2d on the pyramid, layout conversions counted.

    python tools/surface_bench.py [--steps 5]          (also: bench.py's `drop_in` leg calls measure())
    python tools/surface_bench.py --factory [--out profiles/<file>.json]
        the third path: the reference's foward_detector / three-phase loop on the modules of scan_amd.modeling.factory
        (reference signatures outside, the engine's pyramid graph inside), timed in the same process in alternating blocks
        with Trainer.step and SurfaceTrainer.step, + the achieved bandwidth of the pyramid pack kernel
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def count_launches(fn):
    """GPU kernel launches of one call of fn (torch profiler, device activities)"""
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = 0
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA and not e.name.startswith(("Memcpy", "Memset")):
            n += 1
    return n


def op_table(dev, reps=5):
    """forward + backward of one layer: engine call (ops.conv2d on the pyramid rows) vs surface calls (layers.Conv2d per level on
    NCHW channels_last tensors, to-rows / to-NCHW views and the per-call weight split included)"""
    import torch
    from scan_amd import layers as L
    from scan_amd import ops
    cases = [("tower 3x3 256->256, P3..P7, 4 frames", 4, [(128, 256), (64, 128), (32, 64), (16, 32), (8, 16)], 256, 256, 3),
             ("conv4_x 3x3 512->512 @128x256, 4 frames", 4, [(128, 256)], 512, 512, 3),
             ("FPN lateral 1x1 512->256 @128x256, 4 frames", 4, [(128, 256)], 512, 256, 1),
             ("head 3x3 256->8, P3..P7, 2 frames", 2, [(128, 256), (64, 128), (32, 64), (16, 32), (8, 16)], 256, 8, 3)]
    out = []
    for name, n, sizes, cin, cout, k in cases:
        shape = ops.PyramidShape(n, sizes)
        g = torch.Generator(device=dev).manual_seed(1)
        conv = L.Conv2d(cin, cout, k, 1, k // 2).to(dev)
        conv.weight.data = conv.weight.data.contiguous(memory_format=torch.channels_last)
        rows = torch.randn((shape.rows, cin), device=dev, generator=g).requires_grad_(True)
        lv = [rows.detach()[shape.row_off[l]:shape.row_off[l + 1]].view(n, h, w, cin).permute(0, 3, 1, 2).requires_grad_(True)
              for l, (h, w) in enumerate(sizes)]

        def engine():
            ops.invalidate_weight_planes()
            ops.begin_weight_epoch()
            y = ops.conv2d(rows, conv.weight, conv.bias, shape, k, 1)
            y.backward(y.detach())

        def surface():
            ys = [conv(x) for x in lv]
            torch.autograd.backward(ys, [y.detach() for y in ys])

        rec = {"op": name, "calls_surface": len(sizes)}
        for tag, fn in (("engine", engine), ("surface", surface)):
            fn()
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.time()
            s.record()
            for _ in range(reps):
                fn()
            e.record()
            torch.cuda.synchronize()
            rec[tag + "_us"] = round(s.elapsed_time(e) * 1e3 / reps, 1)
            rec[tag + "_host_us"] = round((time.time() - t0) * 1e6 / reps, 1)
            rec[tag + "_launches"] = count_launches(fn)
        rec["ratio"] = round(rec["surface_us"] / rec["engine_us"], 3)
        out.append(rec)
    return out


def measure(trainer, imgs_s, tg, imgs_t, steps=5, with_ops=True):
    """trainer: an engine.Trainer whose model is then ADOPTED by the surface (scan_amd.surface.adopt re-classes its Conv2d /
    GroupNorm modules; the engine path ignores module classes, so the trainer keeps working).  imgs_*: ImageList or NCHW."""
    import torch
    from scan_amd import layers as L
    from scan_amd import surface
    xs = imgs_s.tensors if hasattr(imgs_s, "tensors") else imgs_s
    xt = imgs_t.tensors if hasattr(imgs_t, "tensors") else imgs_t
    st = surface.SurfaceTrainer(trainer)
    for _ in range(2):
        losses = st.step(xs, tg, xt)
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(steps):
        losses = st.step(xs, tg, xt)
    torch.cuda.synchronize()
    ms = (time.time() - t0) / steps * 1e3
    rec = {"ms_per_step": round(ms, 2), "steps": steps, "ops_backend": L.OPS_BACKEND,
           "losses_finite": all(bool(torch.isfinite(v)) for v in losses.values()),
           "launches_per_step": count_launches(lambda: st.step(xs, tg, xt)),
           "graph": "scan_amd.surface: NCHW, one module call per level, layers.Conv2d / GroupNorm / dynamic_conv_softmax on "
                    "scan_ops._ops, three-phase schedule, no side streams"}
    rec["engine_launches_per_step"] = count_launches(lambda: trainer.step(imgs_s, tg, imgs_t))
    if with_ops:
        rec["per_op"] = op_table(xs.device)
    return rec


LEVELS = ("P3", "P4", "P5", "P6", "P7")


class FactoryLoop:
    """One DA iteration in the reference's call shape (engine/trainer.py:20-72 foward_detector, :284-383 the three phases, :418-424
    the optimizer steps) on the modules scan_amd.modeling.factory builds.  Gradient buffers, optimizer and schedule are an
    engine.Trainer's on the same modules (as scan_amd.surface.SurfaceTrainer does): the forward / backward graph is what is timed.
    verbatim=True: the reference's three backward calls (the source graph is walked twice, trainer.py:299,343);
    False: source losses and source adversarial losses in one backward."""

    def __init__(self, cfg, model, trainer, verbatim=True, return_maps=True, foreign=False):
        self.cfg, self.model, self.trainer = cfg, model, trainer
        self.verbatim, self.return_maps, self.foreign = verbatim, return_maps, foreign

    def foward_detector(self, images, targets=None, return_maps=True, mode="source", forward_target=False):
        from scan_amd.structures import to_image_list
        model = self.model
        images = to_image_list(images)
        features = model["backbone"](images.tensors)
        if self.foreign:  # a backbone that is not ours: plain list, NCHW-contiguous
            features = [f.contiguous() for f in features]
        losses = {}
        features, loss_graph, loss_act_map, act_maps = model["middle_head"](
            images, features, targets=targets, return_maps=return_maps, mode=mode, forward_target=forward_target)
        if loss_graph is not None:
            node_loss, consistency_loss = loss_graph
            if consistency_loss is not None and not (isinstance(consistency_loss, (int, float)) and consistency_loss == 0):
                losses["consistency_loss"] = consistency_loss
            if node_loss is not None:
                losses["node_loss"] = node_loss
        if loss_act_map is not None:
            losses["act_loss"] = loss_act_map
        _, proposal_losses, _ = model["fcos"](images, features, targets=targets, return_maps=return_maps, act_maps=act_maps)
        losses.update(proposal_losses)
        return losses, dict(zip(LEVELS, features)), dict(zip(LEVELS, act_maps))

    def _adv(self, feats, maps, label, domain, tag):
        lam = self.cfg.MODEL.ADV.CON_DIS_LAMBDA
        return {"loss_adv_%s_CON_%s" % (l, tag): lam * self.model["dis_%s_CON" % l](feats[l], label, maps[l], domain=domain)
                for l in reversed(LEVELS)}

    def step(self, images_s, targets_s, images_t):
        from scan_amd import ops
        from scan_amd.modeling import fcos as fcos_mod
        tr = self.trainer
        for m in self.model.values():
            m.train()
        ops.begin_weight_epoch(tr._split_plan, tr.device)
        fcos_mod.reset_target_plan()
        tr.grad_arena.zero_()  # optimizer[k].zero_grad() of every sub-model
        loss_dict, feats, maps = self.foward_detector(images_s, targets_s, self.return_maps, "source")
        out = {k + "_gs": v for k, v in loss_dict.items()}
        if self.verbatim:
            sum(out.values()).backward(retain_graph=True)
            ld = self._adv(feats, maps, 1.0, "source", "ds")
            sum(ld.values()).backward()
        else:
            ld = self._adv(feats, maps, 1.0, "source", "ds")
            (sum(out.values()) + sum(ld.values())).backward()
        out.update(ld)
        del feats, maps, ld
        loss_dict, feats, maps = self.foward_detector(images_t, None, self.return_maps, "target")
        lt = {k + "_gt": v for k, v in loss_dict.items()}
        lt.update(self._adv(feats, maps, 0.0, "target", "dt"))
        sum(v for k, v in lt.items() if k != "zero_gt").backward()
        out.update(lt)
        tr._join_streams()
        tr._optimizer_step()
        return out


def pack_bandwidth(dev, n=4, sizes=((128, 256), (64, 128), (32, 64), (16, 32), (8, 16)), c=256, reps=20):
    """achieved GB/s (bytes read + bytes written over the launch time) of ops.pack_levels at the bench pyramid, per source
    layout, beside the streaming read + write kernel of tools/pointwise_roofline.py (grl_scale) on the same device"""
    import torch
    from scan_amd import ops
    import pointwise_roofline
    out = {"n_images": n, "sizes": [list(s) for s in sizes], "C": c}
    g = torch.Generator(device=dev).manual_seed(0)
    base = [torch.randn((n, c, h, w), device=dev, generator=g) for h, w in sizes]
    m = sum(n * h * w for h, w in sizes)
    out["M"], out["bytes"] = m, 2 * 4 * m * c
    for tag, lv in (("nchw", base), ("channels_last", [t.contiguous(memory_format=torch.channels_last) for t in base])):
        rows, shape = ops.pack_levels(lv)
        us = pointwise_roofline._time(lambda: ops.pack_levels(lv), reps, torch)
        us_un = pointwise_roofline._time(lambda: ops.unpack_levels(rows, shape, c, torch.contiguous_format if tag == "nchw"
                                                                  else torch.channels_last), reps, torch)
        out[tag] = {"pack_us": round(us, 2), "pack_GBps": round(out["bytes"] / us * 1e-3, 1),
                    "unpack_us": round(us_un, 2), "unpack_GBps": round(out["bytes"] / us_un * 1e-3, 1)}
    out["fits_llc"] = bool(out["bytes"] < 256e6)
    out["pointwise_roofline"] = [r for r in pointwise_roofline.measure(dev, sizes=(pointwise_roofline.M_CFG5,), reps=reps,
                                                                       only={"grl_scale", "groupnorm_relu_apply"})]
    return out


def measure_factory(dev, H, W, B, steps, rounds=3):
    """engine / factory (reference loop verbatim; one source backward; foreign backbone) / surface, alternating blocks of
    ``steps`` iterations in one process, ``rounds`` times: ms/step per block, and kernel launches per step."""
    import torch
    from scan_amd import config, engine, surface, synth
    from scan_amd.modeling import factory
    from scan_amd.structures import BoxList
    cfg = config.load("c2f")
    mcfg = config.settings(cfg)
    K = mcfg["num_classes"]
    imgs_s = engine.to_image_list([t.to(dev) for t in synth.synth_image_list([(H, W)] * B, 1234)], 32)
    imgs_t = engine.to_image_list([t.to(dev) for t in synth.synth_image_list([(H, W)] * B, 2234)], 32)
    tg = synth.synth_targets(B, H, W, K - 1, 12, 4321)
    targets = []
    for boxes, labels in tg:
        t = BoxList(boxes, (W, H))
        t.add_field("labels", labels)
        targets.append(t)
    emodel = engine.build_model(device=dev, settings=mcfg)
    engine.load_procedural_weights(emodel, K, mcfg["conv_body"])
    etr = engine.Trainer(emodel, settings=mcfg)
    fmodel = factory.build_model(cfg, device=dev)
    engine.load_procedural_weights(fmodel, K, mcfg["conv_body"])
    ftr = engine.Trainer(fmodel, settings=mcfg)
    smodel = engine.build_model(device=dev, settings=mcfg)
    engine.load_procedural_weights(smodel, K, mcfg["conv_body"])
    st = surface.SurfaceTrainer(engine.Trainer(smodel, settings=mcfg))
    legs = {
        "engine": lambda: etr.step(imgs_s, tg, imgs_t),
        "factory_reference_loop": FactoryLoop(cfg, fmodel, ftr, verbatim=True).step,
        "factory_one_source_backward": FactoryLoop(cfg, fmodel, ftr, verbatim=False).step,
        "factory_foreign_backbone": FactoryLoop(cfg, fmodel, ftr, verbatim=False, foreign=True).step,
        "surface": lambda: st.step(imgs_s.tensors, tg, imgs_t.tensors),
    }
    call = {k: (v if k in ("engine", "surface") else (lambda f=v: f(imgs_s, targets, imgs_t))) for k, v in legs.items()}
    rec = {"workload": {"H": H, "W": W, "frames": "%d+%d" % (B, B), "cfg": "c2f", "conv_mode": "bf16x6"}, "steps_per_block": steps,
           "rounds": rounds, "legs": {k: {"ms_per_step_blocks": []} for k in call}}
    for fn in call.values():
        for _ in range(2):
            losses = fn()
        torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in call.items():
            torch.cuda.synchronize()
            t0 = time.time()
            for _ in range(steps):
                losses = fn()
            torch.cuda.synchronize()
            rec["legs"][k]["ms_per_step_blocks"].append(round((time.time() - t0) / steps * 1e3, 2))
            rec["legs"][k]["losses_finite"] = all(bool(torch.isfinite(v)) for v in losses.values())
    for k, fn in call.items():
        b = sorted(rec["legs"][k]["ms_per_step_blocks"])
        rec["legs"][k]["ms_per_step_median"] = b[len(b) // 2]
        rec["legs"][k]["launches_per_step"] = count_launches(fn)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--factory", action="store_true", help="engine / factory / surface in alternating blocks + pack bandwidth")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.factory:
        import torch
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        dev = torch.device("cuda", 0)
        rec = measure_factory(dev, a.height, a.width, 2, a.steps, a.rounds)
        rec["pack_kernel"] = pack_bandwidth(dev)
        line = json.dumps(rec)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(rec, indent=1) + "\n")
        return
    import torch
    from scan_amd import engine, synth
    dev = torch.device("cuda", 0)
    mcfg = engine.CONFIGS["c2f"]
    model = engine.build_model(device=dev, settings=mcfg)
    engine.load_procedural_weights(model, mcfg["num_classes"], mcfg["conv_body"])
    trainer = engine.Trainer(model, settings=mcfg)
    H, W, B = a.height, a.width, 2
    imgs_s = engine.to_image_list([t.to(dev) for t in synth.synth_image_list([(H, W)] * B, 1234)], 32)
    imgs_t = engine.to_image_list([t.to(dev) for t in synth.synth_image_list([(H, W)] * B, 2234)], 32)
    tg = synth.synth_targets(B, H, W, mcfg["num_classes"] - 1, 12, 4321)
    for _ in range(3):
        trainer.step(imgs_s, tg, imgs_t)
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(a.steps):
        trainer.step(imgs_s, tg, imgs_t)
    torch.cuda.synchronize()
    eng = (time.time() - t0) / a.steps * 1e3
    rec = measure(trainer, imgs_s, tg, imgs_t, a.steps)
    rec["engine_ms_per_step"] = round(eng, 2)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

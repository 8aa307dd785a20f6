"""The EPM baseline on the pyramid path: plain FCOS (or ATSS) without a middle head, one global-alignment (GA) discriminator
per pyramid level, optionally a centre-aware (CA) one beside it.

Mirrors the reference's own loop for that setting -- ``foward_detector`` with MODEL.MIDDLE_HEAD.CONDGRAPH_ON False
(fcos_core/engine/trainer.py:20-72) and the USE_DIS_GLOBAL / USE_DIS_CENTER_AWARE branches of the DA iteration
(trainer.py:245-386, tools/train_net_da.py:69-135) -- next to ``engine``, which holds the SCAN step.  ``engine.Trainer`` is not
involved: this file has its own, much smaller iteration (no middle head, no act maps, no data parallelism).

What is pinned to what: the GA step to the reference's loop as it stands.  The reference's CA branch
cannot run there -- without a middle head ``foward_detector`` hands back ``None`` where the loop expects the head's score maps,
and the head groups its maps by type, not by level (rpn/fcos/fcos.py:199-203 against trainer.py:321-325) -- so the CA step is
pinned to the reference's MODULE called with each level's {"box_cls", "centerness"} in the loop's order.
"""
import torch
import torch.distributed as dist

from . import config, ops, synth
from .engine import DIS_ORDER, LEVELS, FlatGroup, _padded_shape, _plan_stream, warmup_factor
from .modeling import fcos as fcos_mod
from .modeling.atss import ATSSModule, build_atss
from .modeling.backbone import build_backbone
from .modeling.discriminator import FCOSDiscriminator, FCOSDiscriminator_CA
from .modeling.fcos import FCOSModule, _event_if_device
from .modeling.resnet import build_resnet_fpn_backbone
from .structures import to_image_list

ADV_KINDS = ("ga", "ca")


def default_settings(num_classes=9, rpn="fcos", adv=("ga",), conv_body="VGG-16-FPN-RETINANET", opts=()):
    """config.epm_settings of the reference's defaults with what configs/epm/*.yaml all set: the dense head on P3..P7 of a
    RetinaNet-style FPN body, discriminators on every level.  opts: further KEY VALUE pairs (reference CLI style)."""
    if rpn not in ("fcos", "atss"):
        raise ValueError("rpn=%r: 'fcos' or 'atss'" % (rpn,))
    adv = tuple(adv)
    if not adv or any(a not in ADV_KINDS for a in adv):
        raise ValueError("adv=%r: a non-empty selection of %r" % (adv, ADV_KINDS))
    cfg = config.defaults()
    lst = ["MODEL.BACKBONE.CONV_BODY", conv_body, "MODEL.RETINANET.USE_C5", False, "MODEL.ADV.USE_DIS_GLOBAL", "ga" in adv,
           "MODEL.ADV.USE_DIS_CENTER_AWARE", "ca" in adv]
    for lvl in LEVELS:
        lst += ["MODEL.ADV.USE_DIS_%s" % lvl, True]
    lst += ["MODEL.ATSS_ON", True, "MODEL.ATSS.NUM_CLASSES", num_classes] if rpn == "atss" else \
        ["MODEL.FCOS_ON", True, "MODEL.FCOS.NUM_CLASSES", num_classes]
    cfg.merge_from_list(lst + list(opts))
    return config.epm_settings(cfg)


def build_model(num_classes=9, rpn="fcos", adv=("ga",), settings=None, device="cuda", conv_body="VGG-16-FPN-RETINANET"):
    """{"backbone", "fcos", "dis_P7" .. "dis_P3"[, "dis_P7_CA" .. "dis_P3_CA"]} like tools/train_net_da.py:43-48, 69-131 with
    CONDGRAPH_ON False.  settings: a config.epm_settings(cfg) dict; it overrides the other keywords."""
    s = settings if settings is not None else default_settings(num_classes, rpn, adv, conv_body)
    body = s["conv_body"]
    if body == "VGG-16-FPN-RETINANET":
        backbone = build_backbone()
    elif body in ("R-50-FPN-RETINANET", "R-101-FPN-RETINANET"):
        backbone = build_resnet_fpn_backbone(body[:-len("-FPN-RETINANET")])
    else:
        raise ValueError("conv_body %r is not built" % body)
    model = {"backbone": backbone,
             "fcos": build_atss(s["head"]) if s["rpn"] == "atss" else FCOSModule(s["num_classes"], "common", s["head"])}
    used = [lvl for lvl in DIS_ORDER if s["use_dis"][lvl]]
    if s["use_dis_global"]:
        for lvl in used:
            model["dis_%s" % lvl] = FCOSDiscriminator(num_convs=s["dis_num_convs"][lvl], grad_reverse_lambda=s["grl_weight"][lvl])
    if s["use_dis_center_aware"]:
        for lvl in used:
            model["dis_%s_CA" % lvl] = FCOSDiscriminator_CA(
                num_convs=s["ca_dis_num_convs"][lvl], grad_reverse_lambda=s["ca_grl_weight"][lvl],
                center_aware_weight=s["center_aware_weight"], center_aware_type=s["center_aware_type"])
    for m in model.values():
        m.to(device)
        for p in m.parameters():
            if p.dim() == 4:
                p.data = p.data.contiguous(memory_format=torch.channels_last)
    return model


def model_adv(model):
    """which discriminator families a model dict holds: a selection of ("ga", "ca")"""
    ga = any(k.startswith("dis_") and not k.endswith("_CA") for k in model)
    return tuple(a for a, on in zip(ADV_KINDS, (ga, any(k.endswith("_CA") for k in model))) if on)


def load_procedural_weights(model):
    """synth.epm_state_dicts for the model's head size and towers"""
    from .engine import load_state_dicts
    convs = lambda sfx: {lvl: model["dis_%s%s" % (lvl, sfx)].num_convs for lvl in LEVELS if "dis_%s%s" % (lvl, sfx) in model}
    sds = synth.epm_state_dicts(model["fcos"].head.num_fg + 1, model_adv(model), dis_num_convs=convs(""), ca_dis_num_convs=convs("_CA"))
    load_state_dicts(model, {k: sds[k] for k in model})


# ----------------------------------------------------------------------------- forward
def _head_train(fcos, rows, shape, targets):
    """the dense head in training mode on ``rows`` -> (losses, class logits [M, C], centerness [M]); without targets the loss
    dict is the reference's {"zero": 0} (rpn/fcos/fcos.py:215-220)"""
    if targets and isinstance(fcos, ATSSModule) and rows.is_cuda:  # the ATSS plan's host read hides behind the head's convolutions
        fcos.loss_evaluator.plan(shape, targets, rows.device, side_stream=_plan_stream(rows.device), after=_event_if_device(targets))
    if not targets:  # the target pass: the maps alone (its loss is identically zero, and so are its gradients)
        with torch.no_grad():
            logits, _, ctr = fcos.head(rows, shape)
        return {"zero": rows.new_zeros(())}, logits, ctr
    logits, reg, ctr = fcos.head(rows, shape)
    lc, lr, lctr = fcos.loss_evaluator(shape, logits, reg, ctr, targets)
    return {"loss_cls": lc, "loss_reg": lr, "loss_centerness": lctr}, logits, ctr


def _forward_rows(model, images, targets, mode, return_maps):
    """backbone + head of one pass -> (il, rows, shape, losses, logits, ctr); logits / ctr are None when the head did not run"""
    il = to_image_list(images)
    in_rows = getattr(il, "rows", None)
    dev = in_rows.device if in_rows is not None else il.tensors.device
    fcos = model["fcos"]
    plan_here = bool(targets) and mode == "source" and fcos.training and dev.type == "cuda" and isinstance(fcos, FCOSModule)
    if plan_here:
        inputs_ready = torch.cuda.Event()
        inputs_ready.record(torch.cuda.current_stream())
    rows, shape = model["backbone"](il.tensors, in_rows, getattr(il, "shape", None))
    if plan_here:  # the ground-truth plan on the side stream while the backbone is queued, as engine.forward_detector does
        fcos_mod.target_plan(shape, targets, dev, side_stream=_plan_stream(dev), after=inputs_ready)
    if not fcos.training:
        return il, rows, shape, None, None, None
    if targets or return_maps:
        losses, logits, ctr = _head_train(fcos, rows, shape, targets)
        return il, rows, shape, losses, logits, ctr
    return il, rows, shape, {"zero": rows.new_zeros(())}, None, None


def forward_detector(model, images, targets=None, mode="source", return_maps=False):
    """reference engine/trainer.py:20-72 with with_middle_head False: backbone, then the dense head on the backbone's rows (the
    head ignores ``act_maps``, rpn/fcos/fcos.py:89-114, and TEST.MODE 'common' scores with its own logits alone).
    Training: (losses, features {P3..P7: rows}, score_maps, shape) -- score_maps is the reference's ``None`` unless
    ``return_maps``, then {level: {"box_cls": [M_l, C], "centerness": [M_l, 1]}}, what the CA discriminators take; in the
    target pass (no targets) the head only runs when its maps are asked for.  Eval: detections."""
    il, rows, shape, losses, logits, ctr = _forward_rows(model, images, targets, mode, return_maps)
    if losses is None:
        return model["fcos"](il.image_sizes, rows, shape)[0]
    maps = None
    if return_maps:
        maps = {lvl: {"box_cls": c, "centerness": t} for lvl, c, t in
                zip(LEVELS, ops.split_levels(logits, shape), ops.split_levels(ctr[:, None], shape))}
    return losses, dict(zip(LEVELS, ops.split_levels(rows, shape))), maps, shape


def _interleave_images(a, shape_a, b, shape_b):
    """rows of two sub-batches of one pyramid (a: the first images, b: the rest; both level-major) -> the rows of the whole"""
    parts = []
    for l in range(shape_a.n_levels):
        parts += [a[shape_a.row_off[l]:shape_a.row_off[l + 1]], b[shape_b.row_off[l]:shape_b.row_off[l + 1]]]
    return torch.cat(parts, 0)


# ----------------------------------------------------------------------------- the iteration
class EPMTrainer:
    """One process, one GPU: the DA iteration of trainer.py:266-424 for GA (/ CA) discriminators on the plain head, then one
    fused-SGD step per sub-model (engine.FlatGroup; the discriminators take SOLVER.DIS).

    The objective is sum(head losses) + GA_DIS_LAMBDA * sum(GA terms) + CA_DIS_LAMBDA * sum(CA terms).  The reference calls
    backward three times (source head losses, source adversarial terms, target adversarial terms; :299, :343, :385) into the
    same .grad; gradients are linear in the loss, so ONE backward of the sum leaves the same accumulated gradients -- the argument
    engine.Trainer.step makes for the SCAN iteration."""

    def __init__(self, model, settings=None, base_lr=None, distributed=False):
        if distributed or (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            raise ValueError("a distributed EPMTrainer is not built (one process, one GPU; engine.Trainer holds the data-parallel step)")
        self.model = model
        adv = model_adv(model)
        if not adv:
            raise ValueError("the model holds no dis_P* / dis_P*_CA discriminator (epm.build_model)")
        if settings is None:
            settings = default_settings(model["fcos"].head.num_fg + 1, "atss" if isinstance(model["fcos"], ATSSModule) else "fcos", adv)
        self.settings = settings
        self.ga_dis_lambda, self.ca_dis_lambda = settings["ga_dis_lambda"], settings["ca_dis_lambda"]
        self.ga_levels = [lvl for lvl in DIS_ORDER if "dis_%s" % lvl in model]
        self.ca_levels = [lvl for lvl in DIS_ORDER if "dis_%s_CA" % lvl in model]
        self.device = next(model["backbone"].parameters()).device
        # one gradient arena for all sub-models (one fill per iteration), every base 256-byte aligned for the float4 kernels
        sizes = {k: FlatGroup.numel(m) for k, m in model.items()}
        pad = lambda n: (n + 63) // 64 * 64
        self.grad_arena = torch.zeros(sum(pad(n) for n in sizes.values()), device=self.device)
        self.groups, self.sched, off = {}, {}, 0
        for k, m in model.items():
            sv = settings["solver"]["dis" if k.startswith("dis_") else k]
            self.groups[k] = FlatGroup(m, sv["lr"] if base_lr is None else base_lr, sv["bias_lr_factor"], sv["wd"], sv["wd_bias"],
                                       sv["momentum"], flat_g=self.grad_arena[off:off + sizes[k]])
            self.sched[k] = dict(warmup_iters=sv["warmup_iters"], factor=sv["warmup_factor"], steps=sv["steps"],
                                 gamma=sv["gamma"], method=sv["warmup_method"])
            off += pad(sizes[k])
        self.iteration = 0
        self._split_plan = ops.SplitPlan()
        self.paired = True

    def _begin(self):
        ops.begin_weight_epoch(self._split_plan, self.device)
        fcos_mod.reset_target_plan()
        for m in self.model.values():
            if not m.training:
                m.train()
        self.grad_arena.zero_()

    def _lams(self, sfx):
        """the GRL strength of every level's discriminator of one family (0 for a level without one: its gradient is dropped)"""
        return [self.model["dis_%s%s" % (lvl, sfx)].grad_reverse.lambda_ if "dis_%s%s" % (lvl, sfx) in self.model else 0.0
                for lvl in LEVELS]

    def _adversarial(self, feats, logits, ctr, shape, n_src, tags):
        """the GA / CA terms of a pyramid whose first n_src images are source frames (n_src = N: source only, 0: target only)
        -> {loss name: (raw loss, lambda)}.  logits / ctr: the head's detached outputs on the same rows (CA only)."""
        model, out = self.model, {}
        N = shape.n_images

        def emit(fmt, lvl, lam, pair):
            if 0 < n_src < N:
                out[fmt % (lvl, "ds")], out[fmt % (lvl, "dt")] = (pair[0], lam), (pair[1], lam)
            else:  # one domain only: all rows are one half
                out[fmt % (lvl, tags)] = (pair[0] if n_src == N else pair[1], lam)

        if self.ga_levels:
            f = ops.split_levels_grl(feats, shape, self._lams(""))
            for lvl in self.ga_levels:
                i = LEVELS.index(lvl)
                emit("loss_adv_%s_%s", lvl, self.ga_dis_lambda,
                     self._pair(model["dis_%s" % lvl], (f[i],), shape.level(i), n_src, N))
        if self.ca_levels:
            first = model["dis_%s_CA" % self.ca_levels[0]]
            # the map once for the pyramid (every CA discriminator is built with the same CENTER_AWARE_WEIGHT / TYPE)
            atten = ops.center_aware_map(logits, ctr, logits.shape[1], first.center_aware_weight)
            a = [atten[shape.row_off[l]:shape.row_off[l + 1]] for l in range(shape.n_levels)]
            f = ops.center_aware_split_levels_grl(feats, atten if first.center_aware_type == "ca_feature" else None, shape,
                                                  self._lams("_CA"))
            for lvl in self.ca_levels:
                i = LEVELS.index(lvl)
                emit("loss_adv_%s_CA_%s", lvl, self.ca_dis_lambda,
                     self._pair(model["dis_%s_CA" % lvl], (f[i], a[i]), shape.level(i), n_src, N))
        return out

    @staticmethod
    def _pair(dis, args, shape_l, n_src, N):
        """forward_pair, also for a pyramid of one domain (an empty half has no loss: its slot is None)"""
        if 0 < n_src < N:
            return dis.forward_pair(*args, shape_l, n_src, grl_applied=True)
        label = 1.0 if n_src == N else 0.0
        logits = dis._logits(args[0], shape_l)
        loss = dis._loss(logits, args[1], label) if len(args) == 2 else ops.bce_with_logits_const_mean(logits, label)
        return (loss, None) if n_src == N else (None, loss)

    def _backward(self, terms):
        roots = [t for t, _ in terms if t.requires_grad]
        seeds = [torch.full((), float(w), device=t.device) for t, w in terms if t.requires_grad]
        torch.autograd.backward(roots, seeds)

    def _optimizer_step(self):
        moms = {g.momentum for g in self.groups.values()}
        segs = []
        for k, g in self.groups.items():
            segs.extend(g.segments(warmup_factor(self.iteration, **self.sched[k])))
            g.first = False
        mom = moms.pop()
        assert not moms, "one momentum for all sub-models (SOLVER.MOMENTUM)"
        ops.sgd_momentum_multi_(segs, mom)
        self.iteration += 1
        ops.invalidate_weight_planes()

    def _finish(self, losses, adv):
        """backward of the objective, the optimizer step, and the reported dict (adversarial terms as lambda * loss)"""
        self._backward([(v, 1.0) for v in losses.values()] + list(adv.values()))
        for k, (v, lam) in adv.items():
            losses[k] = v.detach() * lam
        self._optimizer_step()
        return losses

    def step(self, images_s, targets_s, images_t):
        """One DA iteration; returns the loss dict (0-dim GPU tensors, the reference's key names)."""
        il_s, il_t = to_image_list(images_s), to_image_list(images_t)
        if self.paired and _padded_shape(il_s) == _padded_shape(il_t):
            return self.step_paired(il_s, targets_s, il_t)
        return self.step_two_pass(il_s, targets_s, il_t)

    def step_paired(self, il_s, targets_s, il_t):
        """source and target frames as ONE pyramid through the backbone and the discriminators (frames [0, B) source, [B, 2B)
        target), as engine.Trainer.step_paired; the head sees the source rows (and, for the CA map, the target rows without a
        graph)."""
        model = self.model
        self._begin()
        B = len(il_s.image_sizes)
        fcos = model["fcos"]
        inputs_ready = torch.cuda.Event()
        inputs_ready.record(torch.cuda.current_stream())
        if getattr(il_s, "rows", None) is not None and getattr(il_t, "rows", None) is not None:
            rows, shape = model["backbone"](None, torch.cat([il_s.rows, il_t.rows], 0), ops.PyramidShape(2 * B, il_s.shape.sizes))
        else:
            rows, shape = model["backbone"](torch.cat([il_s.tensors, il_t.tensors], 0))
        shape_src = ops.PyramidShape(B, shape.sizes)
        if isinstance(fcos, FCOSModule):
            fcos_mod.target_plan(shape_src, targets_s, rows.device, side_stream=_plan_stream(rows.device), after=inputs_ready)
        src_rows, _ = ops.take_images(rows, shape, 0, B)
        head_losses, logits_s, ctr_s = _head_train(fcos, src_rows, shape_src, targets_s)
        losses = {k + "_gs": v for k, v in head_losses.items()}
        logits = ctr = None
        if self.ca_levels:
            with torch.no_grad():  # the target pass of the head yields its score maps and an identically-zero loss (:215-220)
                tgt_rows, shape_tgt = ops.take_images(rows, shape, B, 2 * B)
                logits_t, _, ctr_t = fcos.head(tgt_rows, shape_tgt)
                logits = _interleave_images(logits_s.detach(), shape_src, logits_t, shape_tgt)
                ctr = _interleave_images(ctr_s.detach(), shape_src, ctr_t, shape_tgt)
        adv = self._adversarial(rows, logits, ctr, shape, B, None)
        losses = self._finish(losses, adv)
        losses["zero_gt"] = rows.new_zeros(())
        return losses

    def step_two_pass(self, il_s, targets_s, il_t):
        """the reference's schedule for batches of different padded sizes: source pass + source terms, target pass + target
        terms, one backward of everything"""
        self._begin()
        want = bool(self.ca_levels)
        losses, adv = {}, {}
        for il, targets, tag in ((il_s, targets_s, "s"), (il_t, None, "t")):
            _, rows, shape, ld, logits, ctr = _forward_rows(self.model, il, targets, "source" if targets else "target", want)
            losses.update({k + "_g" + tag: v for k, v in ld.items()})
            if want:
                logits, ctr = logits.detach(), ctr.detach()
            adv.update(self._adversarial(rows, logits, ctr, shape, shape.n_images if targets else 0, "d" + tag))
        return self._finish(losses, adv)

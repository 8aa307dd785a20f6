#!/usr/bin/env python
"""The region-proposal network's own kernels on the bench pyramid (N = 4 frames of 1024 x 2048: P3..P7 = 128x256 ... 8x16,
M = 174,592 rows, A = 3 anchors per row: 523,776 anchors, about 30 boxes per image):

    labels + sampler   RPNLossComputation.labels (csrc/retina.hip's two matcher launches + csrc/rpn.hip's visibility launch) and
                       ops.rpn_sample with the read of its counters, from host ground truth through the pinned staging buffers,
                       beside the RetinaNet plan (modeling.retinanet.build_plan, A = 3 too) in the same run, alternating; host
                       clock around a call that ends in a synchronise; launches and host reads as the Python side issues them
    loss               scan_rpn_loss_forward / _forward_ordered / _backward over ALL anchors (no compaction); device events;
                       beside ops.add_relu on a matrix of d_reg's size (2 reads + 1 write) as the streaming yardstick
    proposals          the gather / decode / clip / small-box step at PRE_NMS_TOP_N_TRAIN = 12000 (K = 12000 + 8192 + 2048 +
                       512 + 128 candidates per image): ops.rpn_decode_proposals against the torch spelling of the same step in
                       the same run; device events; and the whole box_selector_train call by the host clock

There is no pass / fail number -- nothing comparable existed before this head.  Median of three rounds.

    python tools/rpn_bench.py [--out profiles/rNN_rpn.txt] [--reps 20]

Without --out the next free profiles/rNN_rpn.txt is written.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import ctypes
import glob
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from atss_bench import SIZES, bench_targets  # noqa: E402


def next_profile():
    taken = [int(m.group(1)) for m in (re.match(r"r(\d+)_", os.path.basename(p)) for p in glob.glob(os.path.join(ROOT, "profiles", "r*_*")))
             if m]
    return os.path.join(ROOT, "profiles", "r%02d_rpn.txt" % (max(taken, default=0) + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--boxes", type=int, default=30)
    a = ap.parse_args()
    import torch
    from scan_amd import _lib, ops
    from scan_amd.modeling import retinanet, rpn
    if not torch.cuda.is_available():
        raise SystemExit("rpn_bench: no GPU; the numbers are unmeasured")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    H, W = 1024, 2048
    shape = ops.PyramidShape(a.images, SIZES)
    targets = bench_targets(torch, a.images, a.boxes, H, W)
    image_hw = [(H, W)] * a.images
    cells = rpn.cell_anchors()
    A = int(cells.shape[1])
    n_anchors = shape.rows * A
    say("# RPN kernels on the bench pyramid: N=%d, levels %s, M=%d rows, A=%d: %d anchors, boxes per image %s, %d repetitions per "
        "figure, median of three rounds" % (a.images, SIZES, shape.rows, A, n_anchors, [int(b.shape[0]) for b, _ in targets], a.reps))
    say("# library: %s" % _lib.lib_identity())

    def host_ms(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        return ts[len(ts) // 2]

    def event_ms(fn):
        for _ in range(3):
            fn()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for _ in range(a.reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.reps

    def rounds(fns, clock):
        """{name: [three figures]} with the candidates alternating, so that a drift of the box hits all of them"""
        out = {k: [] for k in fns}
        for _ in range(3):
            for k, fn in fns.items():
                out[k].append(clock(fn))
        return out

    def show(name, v, note=""):
        say("  %-28s %9.4f ms   (rounds %s)%s" % (name, sorted(v)[1], " ".join("%.4f" % x for x in v), note))

    le = rpn.RPNLossComputation(cells=cells, seed=1)

    def labels_and_sample():
        labels, matched, boxes = le.labels(shape, targets, image_hw, dev)
        sampled, counts = ops.rpn_sample(shape, A, labels, le.batch_size_per_image, le.positive_fraction, le.next_seed())
        return labels, matched, boxes, sampled, int(counts.sum().item())

    say("")
    say("labels + sampler from host ground truth, host clock incl. upload and the host read; the RetinaNet plan with the same cells")
    r = rounds({"rpn labels + sampler": labels_and_sample,
                "retinanet plan (A = 3)": lambda: retinanet.build_plan(shape, targets, dev, cells=cells, bg=0.3, fg=0.7)}, host_ms)
    for k, v in r.items():
        show(k, v)
    labels, matched, boxes, sampled, n_sampled = labels_and_sample()
    say("  as issued by the Python side (counted there, not observed on the device): rpn 4 kernel launches (matcher 2, visibility 1, "
        "sampler 1) + 2 memsets, 1 host read (the counters); RetinaNet plan: "
        "%d launches + 2 memsets, %d host read" % (retinanet.plan_stats["launches"], retinanet.plan_stats["host_reads"]))
    say("  labels: %d positive, %d negative, %d ignored of %d; sampled %d (%d positive)"
        % (int((labels == 1).sum()), int((labels == 0).sum()), int((labels < 0).sum()), n_anchors, n_sampled, int((sampled == 1).sum())))

    say("")
    say("loss over all %d anchors (device events, ms per launch)" % n_anchors)
    P_, st = ops._ptr, ops._stream
    g = torch.Generator(device=dev).manual_seed(1)
    wide = torch.randn((shape.rows, ops.pad4(5 * A)), device=dev, generator=g)
    reg, obj = wide[:, :4 * A], wide[:, 4 * A:5 * A]
    out, gn = torch.zeros(2, device=dev), torch.ones(2, device=dev)
    d_obj, d_reg = torch.empty((shape.rows, A), device=dev), torch.empty((shape.rows, 4 * A), device=dev)
    ws = torch.empty((max(1, ops.query("scan_rpn_loss_ordered_ws_floats", n_anchors)),), device=dev)
    dcells = retinanet.device_cells(cells, dev)
    geo = (shape.ref(), (ctypes.c_int32 * 5)(*rpn.ANCHOR_STRIDES), P_(dcells), A, P_(boxes), boxes.shape[1], P_(matched), P_(sampled),
           P_(obj), wide.shape[1], P_(reg), wide.shape[1], 1.0 / 9)
    other = torch.randn_like(d_reg)
    r = rounds({"forward": lambda: ops.call("scan_rpn_loss_forward", *geo, None, P_(out), st()),
                "forward, ordered (2 launches)": lambda: ops.call("scan_rpn_loss_forward_ordered", *geo, None, P_(out), P_(ws), st()),
                "backward": lambda: ops.call("scan_rpn_loss_backward", *geo, P_(gn), P_(d_obj), A, P_(d_reg), 4 * A, st()),
                "add_relu [%d, %d], same run" % tuple(d_reg.shape): lambda: ops.add_relu(d_reg, other)}, event_ms)
    for k, v in r.items():
        show(k, v)

    say("")
    sel = rpn.RPNPostProcessor(12000, 2000, 0.7, 0, 2000, cells=cells, training=True)
    prob = obj.sigmoid()
    ks, idxs = [], []
    for l in range(shape.n_levels):
        r0, r1 = shape.row_off[l], shape.row_off[l + 1]
        n_l = (r1 - r0) // a.images * A
        ks.append(min(12000, n_l))
        idxs.append(prob[r0:r1].reshape(a.images, n_l).topk(ks[-1], dim=1, sorted=True)[1])
    idx = torch.cat(idxs, 1).contiguous()
    hw_d = rpn.device_image_hw(image_hw, dev)
    anchors = retinanet.level_anchors(shape, dcells, rpn.ANCHOR_STRIDES)
    lim = torch.tensor([[w - 1, h - 1, w - 1, h - 1] for h, w in image_hw], dtype=torch.float32, device=dev)

    def torch_spelling():
        regs, ancs = [], []
        for l in range(shape.n_levels):
            r0, r1 = shape.row_off[l], shape.row_off[l + 1]
            n_l = (r1 - r0) // a.images * A
            regs.append(reg[r0:r1].reshape(a.images, n_l, 4).gather(1, idxs[l][..., None].expand(-1, -1, 4)))
            ancs.append(anchors[l][idxs[l]])
        t, an = torch.cat(regs, 1), torch.cat(ancs, 1)
        w_, h_ = an[..., 2] - an[..., 0] + 1, an[..., 3] - an[..., 1] + 1
        cx, cy = an[..., 0] + 0.5 * w_, an[..., 1] + 0.5 * h_
        dw, dh = t[..., 2].clamp(max=retinanet.BBOX_XFORM_CLIP), t[..., 3].clamp(max=retinanet.BBOX_XFORM_CLIP)
        pcx, pcy, pw, ph = t[..., 0] * w_ + cx, t[..., 1] * h_ + cy, torch.exp(dw) * w_, torch.exp(dh) * h_
        b = torch.stack((pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw - 1, pcy + 0.5 * ph - 1), -1)
        b = torch.minimum(b.clamp(min=0), lim[:, None, :])
        return b, ((b[..., 2] - b[..., 0] + 1 >= 0) & (b[..., 3] - b[..., 1] + 1 >= 0)).to(torch.uint8)

    say("proposal decode at PRE_NMS_TOP_N_TRAIN = 12000: K = %d candidates per image (device events, ms per call)" % sum(ks))
    r = rounds({"scan_rpn_decode (1 launch)": lambda: ops.rpn_decode_proposals(reg, shape, rpn.ANCHOR_STRIDES, dcells, idx, ks, hw_d, 0),
                "torch spelling": torch_spelling}, event_ms)
    for k, v in r.items():
        show(k, v)
    b_k, k_k = ops.rpn_decode_proposals(reg, shape, rpn.ANCHOR_STRIDES, dcells, idx, ks, hw_d, 0)
    b_t, k_t = torch_spelling()
    say("  kernel against the torch spelling on this input: worst |box difference| %.3g, keep flags equal %s"
        % (float((b_k - b_t).abs().max()), torch.equal(k_k, k_t)))
    r = rounds({"box_selector_train, whole call": lambda: sel(shape, obj, reg, image_hw, targets)}, host_ms)
    show("box_selector_train, whole call", r["box_selector_train, whole call"],
         "   host clock: top-k per level, decode, one NMS launch + host read per image, batch-wide top-n, ground truth")
    path = a.out or next_profile()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", path)


if __name__ == "__main__":
    main()

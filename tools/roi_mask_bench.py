#!/usr/bin/env python
"""The Mask R-CNN mask head's own kernels at the box head's bench plan (N = 4 frames of 1024 x 2048, about 2000 proposals plus
about 30 ground-truth boxes per image, BATCH_SIZE_PER_IMAGE 512, C = 9 and 81, pooler 14, masks of 28 x 28):

    plan       MaskRCNNLossComputation.plan_from_box on the box head's subsample: the masks' layout, ops.roi_mask_positives,
               ops.roi_mask_targets, no host read; host clock around a call that ends in a synchronise, with the two launches'
               device-event time beside it.  Baseline: the same targets the reference's way on the CPU -- the per-proposal crop /
               F.interpolate / cast loop of project_masks_on_boxes, restated here
    loss       scan_roi_mask_loss_forward / _forward_ordered / _backward over the Rp positives; device events
    prob       scan_roi_mask_prob at K = 400
    paste      scan_roi_mask_paste at K = 100 per image; baseline: the per-detection interpolate / threshold / paste loop of
               Masker.forward_single_image on the CPU, restated here
    convs      mask_fcn1..4 (3x3, 256 -> 256 on 14 x 14 ROI images), conv5_mask (the 4 D-column 1x1 conv + shuffle) and
               mask_fcn_logits (256 -> C on 28 x 28), forward and forward + backward, beside the torch operators in the same run

There is no pass / fail number -- nothing comparable existed before this head.  Median of three rounds.

    python tools/roi_mask_bench.py [--out profiles/rNN_roi_mask.txt] [--reps 20]

Without --out the next free profiles/rNN_roi_mask.txt is written.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from atss_bench import bench_targets  # noqa: E402
from rpn_bench import next_profile  # noqa: E402


def cpu_targets(torch, masks, rois, gt, M):
    """project_masks_on_boxes (reference mask_head/loss.py:11-42) on CPU tensors: per positive crop, resize, cast, then stack"""
    out = []
    for roi, g in zip(rois.tolist(), gt.tolist()):
        m = masks[int(roi[0])][g]
        h, w = m.shape
        xmin, ymin, xmax, ymax = [round(float(b)) for b in roi[1:]]
        xmin, ymin = min(max(xmin, 0), w - 1), min(max(ymin, 0), h - 1)
        xmax, ymax = max(min(max(xmax, 0), w), xmin + 1), max(min(max(ymax, 0), h), ymin + 1)
        c = m[ymin:ymax, xmin:xmax]
        r = torch.nn.functional.interpolate(c[None, None].float(), size=(M, M), mode="bilinear", align_corners=False)[0, 0]
        out.append(r.type_as(m))
    return torch.stack(out, 0).to(dtype=torch.float32)


def cpu_paste(torch, prob, boxes, H, W, thresh=0.5):
    """Masker.forward_single_image (reference mask_head/inference.py:118-172) on CPU tensors, padding 1"""
    M = prob.shape[-1]
    scale = float(M + 2) / M
    res = []
    for mask, box in zip(prob, boxes):
        pad = mask.new_zeros((M + 2, M + 2))
        pad[1:-1, 1:-1] = mask[0]
        wh, hh = (box[2] - box[0]) * .5 * scale, (box[3] - box[1]) * .5 * scale
        xc, yc = (box[2] + box[0]) * .5, (box[3] + box[1]) * .5
        b = torch.stack((xc - wh, yc - hh, xc + wh, yc + hh)).to(torch.int32)
        w, h = max(int(b[2] - b[0] + 1), 1), max(int(b[3] - b[1] + 1), 1)
        m = torch.nn.functional.interpolate(pad[None, None], size=(h, w), mode="bilinear", align_corners=False)[0, 0] > thresh
        im = torch.zeros((H, W), dtype=torch.uint8)
        x0, x1, y0, y1 = max(int(b[0]), 0), min(int(b[2]) + 1, W), max(int(b[1]), 0), min(int(b[3]) + 1, H)
        if x1 > x0 and y1 > y0:
            im[y0:y1, x0:x1] = m[y0 - int(b[1]):y1 - int(b[1]), x0 - int(b[0]):x1 - int(b[0])]
        res.append(im)
    return torch.stack(res, 0)[:, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--boxes", type=int, default=30)
    ap.add_argument("--proposals", type=int, default=2000)
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from scan_amd import _lib, ops
    from scan_amd.modeling import roi_box_head as rb, roi_mask_head as rm
    from scan_amd.structures import BoxList
    if not torch.cuda.is_available():
        raise SystemExit("roi_mask_bench: no GPU; the numbers are unmeasured")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def rounds(one):
        v = sorted(one() for _ in range(3))
        return v[1]

    def host_ms(fn, reps=None):
        def one():
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(reps or a.reps):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            return sorted(ts)[len(ts) // 2]
        return rounds(one)

    def event_us(fn):
        def one():
            for _ in range(3):
                fn()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            for _ in range(a.reps):
                fn()
            e.record()
            torch.cuda.synchronize()
            return s.elapsed_time(e) * 1e3 / a.reps
        return rounds(one)

    H, W, N, M, P = 1024, 2048, a.images, 28, 14
    targets = bench_targets(torch, N, a.boxes, H, W)
    g = torch.Generator().manual_seed(23)
    proposals, masks_cpu = [], []
    ys, xs = torch.arange(H)[:, None].float(), torch.arange(W)[None, :].float()
    for b, _ in targets:  # the box bench's proposals; an ellipse inside every ground-truth box as its mask
        k = a.proposals
        near = b[torch.randint(0, b.shape[0], (k // 4,), generator=g)].float() + torch.randn(k // 4, 4, generator=g) * 6
        xy = torch.rand(k - k // 4, 2, generator=g) * torch.tensor([W - 64.0, H - 64.0])
        far = torch.cat((xy, xy + 16 + torch.rand(k - k // 4, 2, generator=g) * 240), 1)
        box = torch.cat((near, far, b.float()), 0)
        box[:, 2:] = torch.maximum(box[:, 2:], box[:, :2] + 1)
        proposals.append(BoxList(box.to(dev), (W, H), mode="xyxy"))
        m = torch.stack([(((xs - (x0 + x1) / 2) / (0.45 * (x1 - x0))) ** 2 + ((ys - (y0 + y1) / 2) / (0.45 * (y1 - y0))) ** 2 <= 1)
                         for x0, y0, x1, y1 in b.tolist()]).to(torch.uint8)
        masks_cpu.append(m)
    masks_dev = [m.to(dev) for m in masks_cpu]
    mask_targets = [(b, l, m) for (b, l), m in zip(targets, masks_dev)]
    say("# mask head kernels: N=%d, proposals per image %s, boxes per image %s, BATCH_SIZE_PER_IMAGE 512, pooler %d, masks %d x %d, "
        "%d repetitions per figure, median of three rounds" % (N, [len(p) for p in proposals], [int(b.shape[0]) for b, _ in targets],
                                                                P, M, M, a.reps))
    say("# library: %s" % _lib.lib_identity())

    box = rb.FastRCNNLossComputation(batch_size_per_image=512)
    box.subsample(proposals, targets)
    le = rm.MaskRCNNLossComputation(0.5, 0.5, M)
    plan_ms = host_ms(lambda: le.plan_from_box(box, mask_targets))
    stats = dict(rm.plan_stats)
    Rp = int(le.pos_labels.shape[0])
    flat, moff, mhw = rm.upload_masks(mask_targets, dev)
    two_us = event_us(lambda: (ops.roi_mask_positives(box.labels, box.rois, box.src, box.matched, N, box.padded[1], Rp),
                               ops.roi_mask_targets(le.pos_rois, le.pos_gt, flat, moff, mhw, M)))
    rois_c, gt_c = le.pos_rois.cpu(), le.pos_gt.cpu()
    t0 = time.perf_counter()
    ref_t = cpu_targets(torch, masks_cpu, rois_c, gt_c, M).to(dev)
    torch.cuda.synchronize()
    cpu_ms = (time.perf_counter() - t0) * 1e3
    got_t = le.targets
    say("plan (masks' layout on device-resident masks, positives, targets): %.3f ms host clock; %s; the two launches %.1f us on the "
        "device; R = %d, Rp = %d.  The reference's per-proposal crop / interpolate / upload loop on the CPU: %.1f ms (one run); its "
        "targets are a subset of the device's: %s, %d of %d ones differ"
        % (plan_ms, stats, two_us, box.labels.shape[0], Rp, cpu_ms, bool((got_t >= ref_t).all()), int((got_t != ref_t).sum()),
           int(got_t.sum())))

    for C in (9, 81):
        cs = ops.pad4(C)
        labels = torch.randint(1, C, (Rp,), device=dev, dtype=torch.int32)
        rows = torch.randn(Rp * M * M, cs, device=dev, requires_grad=True)
        fwd = event_us(lambda: ops.roi_mask_loss(rows, labels, le.targets, C))
        prev = ops.set_deterministic(True)
        try:
            ordered = event_us(lambda: ops.roi_mask_loss(rows, labels, le.targets, C))
        finally:
            ops.set_deterministic(prev)
        out = ops.roi_mask_loss(rows, labels, le.targets, C)
        bwd = event_us(lambda: torch.autograd.grad(out, (rows,), retain_graph=True))
        m1, m2 = torch.randn(Rp * M * M, cs, device=dev), torch.randn(Rp * M * M, cs, device=dev)
        one = torch.empty((1,), device=dev)
        one_wg = event_us(lambda: ops.call("scan_roi_mask_loss_forward", ops._ptr(rows), cs, Rp, M, C, ops._ptr(labels),
                                           ops._ptr(le.targets), ops._ptr(one), ops._stream()))
        small = ops.ROI_MASK_LOSS_ONE_LAUNCH_ELEMS // (M * M)
        one_small = event_us(lambda: ops.call("scan_roi_mask_loss_forward", ops._ptr(rows), cs, small, M, C, ops._ptr(labels),
                                              ops._ptr(le.targets), ops._ptr(one), ops._stream()))
        ws = torch.empty((256,), device=dev)
        two_small = event_us(lambda: ops.call("scan_roi_mask_loss_forward_ordered", ops._ptr(rows), cs, small, M, C, ops._ptr(labels),
                                              ops._ptr(le.targets), ops._ptr(one), ops._ptr(ws), ops._stream()))
        say("loss C=%d, Rp=%d (%d elements, rows of %d columns): forward %.1f us, in deterministic mode %.1f us (both the slots + "
            "ordered sum, two launches, at this size), backward %.1f us (through autograd); add_relu on the rows: %.1f us.  The "
            "library's one-workgroup entry alone: %.1f us here; at Rp=%d (%d elements) %.1f us against %.1f us for the two launches"
            % (C, Rp, Rp * M * M, cs, fwd, ordered, bwd, event_us(lambda: ops.add_relu(m1, m2)), one_wg, small, small * M * M,
               one_small, two_small))
        K = 400
        krows, klab = torch.randn(K * M * M, cs, device=dev), torch.randint(1, C, (K,), device=dev)
        say("prob C=%d, K=%d: %.1f us" % (C, K, event_us(lambda: ops.roi_mask_prob(krows, klab, M, C))))
    K = 100
    prob = torch.rand(K, 1, M, M, device=dev)
    xy = torch.rand(K, 2, generator=g) * torch.tensor([W - 300.0, H - 300.0])
    dbox = torch.cat((xy, xy + 20 + torch.rand(K, 2, generator=g) * 280), 1)
    dbox_d = dbox.to(dev)
    paste_us = event_us(lambda: ops.roi_mask_paste(prob, dbox_d, (H, W)))
    prob_c = prob.cpu()
    t0 = time.perf_counter()
    ref_p = cpu_paste(torch, prob_c, dbox, H, W)
    cpu_paste_ms = (time.perf_counter() - t0) * 1e3
    same = int((ops.roi_mask_paste(prob, dbox_d, (H, W)).cpu() != ref_p).sum())
    say("paste K=%d on %d x %d: %.1f us per image (one launch, %d bytes written).  The reference's per-detection loop on the CPU: "
        "%.1f ms (one run); pixels that differ: %d" % (K, H, W, paste_us, K * H * W, cpu_paste_ms, same))

    shape = ops.PyramidShape(Rp, [(P, P)])
    up = ops.PyramidShape(Rp, [(2 * P, 2 * P)])

    def both(f, ts, dy):
        for t in ts:
            t.grad = None
        f().backward(dy)

    def nchw(t, s):
        return t.detach().view(Rp, s, s, -1).permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last).requires_grad_(True)

    x = torch.randn(shape.rows, 256, device=dev, requires_grad=True)
    w3 = (torch.randn(256, 256, 3, 3, device=dev) * 0.02).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    b3 = torch.zeros(256, device=dev, requires_grad=True)
    dy = torch.randn(shape.rows, 256, device=dev)
    xn, dyn = nchw(x, P), nchw(dy, P).detach()
    say("mask_fcn 3x3 256 -> 256 at Rp=%d on %d x %d (%s), one of the four: forward %.1f us, forward + backward %.1f us; F.conv2d "
        "(channels_last): forward %.1f us, forward + backward %.1f us"
        % (Rp, P, P, ops.CONV_MODE, event_us(lambda: ops.conv2d(x.detach(), w3.detach(), b3.detach(), shape, 3, 1, relu=True)),
           event_us(lambda: both(lambda: ops.conv2d(x, w3, b3, shape, 3, 1, relu=True), (x, w3, b3), dy)),
           event_us(lambda: F.relu(F.conv2d(xn.detach(), w3.detach(), b3.detach(), padding=1))),
           event_us(lambda: both(lambda: F.relu(F.conv2d(xn, w3, b3, padding=1)), (xn, w3, b3), dyn))))
    pr = rm.MaskRCNNC4Predictor(256, 256, 81).to(dev)
    dyu = torch.randn(up.rows, 256, device=dev)
    dyun = nchw(dyu, 2 * P).detach()
    w5, b5 = pr.conv5_mask.weight, pr.conv5_mask.bias
    say("conv5_mask 256 -> 4 x 256 columns + shuffle at Rp=%d: forward %.1f us, forward + backward %.1f us; F.conv_transpose2d: "
        "forward %.1f us, forward + backward %.1f us"
        % (Rp, event_us(lambda: pr.upsampled(x.detach(), shape)[0]),
           event_us(lambda: both(lambda: pr.upsampled(x, shape)[0], (x, w5, b5), dyu)),
           event_us(lambda: F.relu(F.conv_transpose2d(xn.detach(), w5.detach(), b5.detach(), stride=2))),
           event_us(lambda: both(lambda: F.relu(F.conv_transpose2d(xn, w5, b5, stride=2)), (xn, w5, b5), dyun))))
    for C in (9, 81):
        pc = rm.MaskRCNNC4Predictor(256, 256, C).to(dev)
        wl, bl = pc.mask_fcn_logits.weight, pc.mask_fcn_logits.bias
        u = torch.randn(up.rows, 256, device=dev, requires_grad=True)
        un = nchw(u, 2 * P)
        dl = torch.randn(up.rows, ops.pad4(C), device=dev)
        dln = nchw(dl[:, :C].contiguous(), 2 * P).detach()
        say("mask_fcn_logits 256 -> %d at Rp=%d on %d x %d: forward %.1f us, forward + backward %.1f us; F.conv2d: forward %.1f us, "
            "forward + backward %.1f us"
            % (C, Rp, 2 * P, 2 * P, event_us(lambda: pc.logits(u.detach(), up)), event_us(lambda: both(lambda: pc.logits(u, up), (u, wl, bl), dl)),
               event_us(lambda: F.conv2d(un.detach(), wl.detach(), bl.detach())),
               event_us(lambda: both(lambda: F.conv2d(un, wl, bl), (un, wl, bl), dln))))
    out = a.out or next_profile().replace("_rpn.txt", "_roi_mask.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()

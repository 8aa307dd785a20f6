#!/usr/bin/env python
"""The Fast R-CNN box head's own kernels at the bench workload's size (N = 4 frames of 1024 x 2048, about 2000 proposals plus about
30 ground-truth boxes per image, BATCH_SIZE_PER_IMAGE 512, C = 9 and 81):

    plan       FastRCNNLossComputation.subsample: pad + upload, ops.roi_box_match, ops.rpn_sample on the padded layout, the one
               host read, ops.roi_box_gather; host clock around a call that ends in a synchronise
    loss       scan_roi_box_loss_forward / _forward_ordered / _backward over the R sampled rows, and scan_roi_box_decode over
               R = 4000 test-time rows; device events; each beside ops.add_relu on a matrix of the same size (2 reads + 1 write)
               as the launch-length yardstick
    fc6 / fc7  modeling.roi_box_head.linear_rows (the 1x1 convolutions of ops.conv2d) forward and forward + backward beside
               torch.nn.functional.linear in the same run, with the weight gradient's plan.ws_floats

There is no pass / fail number -- nothing comparable existed before this head.  Median of three rounds.

    python tools/roi_box_bench.py [--out profiles/rNN_roi_box.txt] [--reps 20]

Without --out the next free profiles/rNN_roi_box.txt is written.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from atss_bench import bench_targets  # noqa: E402
from rpn_bench import next_profile  # noqa: E402


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
    from scan_amd.modeling import roi_box_head as rb
    from scan_amd.structures import BoxList
    if not torch.cuda.is_available():
        raise SystemExit("roi_box_bench: no GPU; the numbers are unmeasured")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def rounds(one):
        v = sorted(one() for _ in range(3))
        return v[1]

    def host_ms(fn):
        def one():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.reps):
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

    H, W, N = 1024, 2048, a.images
    targets = bench_targets(torch, N, a.boxes, H, W)
    g = torch.Generator().manual_seed(23)
    proposals = []
    for b, _ in targets:  # jittered copies of the boxes, background boxes, then the ground truth itself (as the RPN appends it)
        k = a.proposals
        near = b[torch.randint(0, b.shape[0], (k // 4,), generator=g)].float() + torch.randn(k // 4, 4, generator=g) * 6
        xy = torch.rand(k - k // 4, 2, generator=g) * torch.tensor([W - 64.0, H - 64.0])
        far = torch.cat((xy, xy + 16 + torch.rand(k - k // 4, 2, generator=g) * 240), 1)
        box = torch.cat((near, far, b.float()), 0)
        box[:, 2:] = torch.maximum(box[:, 2:], box[:, :2] + 1)
        bl = BoxList(box.to(dev), (W, H), mode="xyxy")
        bl.add_field("objectness", torch.ones(box.shape[0], device=dev))
        proposals.append(bl)
    say("# box head kernels: N=%d, proposals per image %s, boxes per image %s, BATCH_SIZE_PER_IMAGE 512, %d repetitions per figure, "
        "median of three rounds" % (N, [len(p) for p in proposals], [int(b.shape[0]) for b, _ in targets], a.reps))
    say("# library: %s" % _lib.lib_identity())

    le = rb.FastRCNNLossComputation(batch_size_per_image=512)
    say("plan (pad + upload, match, sample, host read, gather): %.3f ms host clock; %s; R = %d, positives %d"
        % (host_ms(lambda: le.subsample(proposals, targets)), rb.plan_stats, le.labels.shape[0], int((le.labels > 0).sum())))
    R = int(le.labels.shape[0])
    for C in (9, 81):
        labels = torch.where(le.labels > 0, torch.randint(1, C, (R,), device=dev, dtype=torch.int32), torch.zeros_like(le.labels))
        cls = torch.randn(R, C, device=dev, requires_grad=True)
        reg = torch.randn(R, 4 * C, device=dev, requires_grad=True)
        fwd = event_us(lambda: ops.roi_box_loss(cls, reg, labels, le.reg_targets))
        prev = ops.set_deterministic(True)
        try:
            ordered = event_us(lambda: ops.roi_box_loss(cls, reg, labels, le.reg_targets))
        finally:
            ops.set_deterministic(prev)
        out = ops.roi_box_loss(cls, reg, labels, le.reg_targets)
        g2 = torch.ones(2, device=dev)
        bwd = event_us(lambda: torch.autograd.grad(out, (cls, reg), g2, retain_graph=True))
        m1, m2 = torch.randn(R, 4 * C, device=dev), torch.randn(R, 4 * C, device=dev)
        say("loss C=%d, R=%d: forward %.1f us, ordered twin %.1f us (two launches), backward %.1f us (through autograd); add_relu on "
            "[R, 4 C]: %.1f us" % (C, R, fwd, ordered, bwd, event_us(lambda: ops.add_relu(m1, m2))))
        Rt = 4000
        rois = torch.cat([torch.cat((torch.full((len(p), 1), float(i), device=dev), p.bbox), 1) for i, p in enumerate(proposals)])[:Rt]
        rois = rois.contiguous()
        tc, tr = torch.randn(Rt, C, device=dev), torch.randn(Rt, 4 * C, device=dev)
        hw = torch.tensor([[H, W]] * N, dtype=torch.int32, device=dev)
        d1, d2 = torch.randn(Rt, 4 * C, device=dev), torch.randn(Rt, 4 * C, device=dev)
        say("decode C=%d, R=%d: %.1f us; add_relu on [R, 4 C]: %.1f us"
            % (C, Rt, event_us(lambda: ops.roi_box_decode(tc, tr, rois, hw)), event_us(lambda: ops.add_relu(d1, d2))))
    for name, K, D in (("fc6", 12544, 1024), ("fc7", 1024, 1024)):
        x = torch.randn(R, K, device=dev, requires_grad=True)
        w = (torch.randn(D, K, device=dev) * 0.01).requires_grad_(True)
        b = torch.zeros(D, device=dev, requires_grad=True)
        dy = torch.randn(R, D, device=dev)
        shape = ops.PyramidShape(1, [(R, 1)])
        plan = _lib.WgradPlan()
        _lib.call("scan_conv_wgrad_plan", ops.split_pieces(), 1, 1, K, D, shape.ref(), shape.ref(), ctypes.byref(plan))

        def both(f):
            for t in (x, w, b):
                t.grad = None
            f(x, w, b).backward(dy)
        say("%s %d -> %d at R=%d (%s): forward %.1f us, forward + backward %.1f us, plan.ws_floats %d; F.linear: forward %.1f us, "
            "forward + backward %.1f us"
            % (name, K, D, R, ops.CONV_MODE, event_us(lambda: rb.linear_rows(x.detach(), w.detach(), b.detach(), relu=True)),
               event_us(lambda: both(lambda x_, w_, b_: rb.linear_rows(x_, w_, b_, relu=True))), plan.ws_floats,
               event_us(lambda: F.relu(F.linear(x.detach(), w.detach(), b.detach()))),
               event_us(lambda: both(lambda x_, w_, b_: F.relu(F.linear(x_, w_, b_))))))
    out = a.out or next_profile().replace("_rpn.txt", "_roi_box.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()

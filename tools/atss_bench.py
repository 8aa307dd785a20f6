#!/usr/bin/env python
"""The ATSS head's own kernels on the bench pyramid (N = 4 frames of 1024 x 2048: P3..P7 = 128x256 ... 8x16, M = 174,592 rows,
about 30 boxes per image):

    plan        modeling.atss.build_plan (csrc/atss.hip: candidates, vote, labels, compaction, targets + the one host read),
                beside the FCOS plan (modeling.fcos._build_plan, csrc/targets.hip) on the same box in the same run, both from
                host ground truth through the pinned staging buffers; host clock around a call that ends in a synchronise
    GIoU        scan_atss_giou_forward / _forward_ordered / _backward on the plan's positives and, for a rate that is not all
                launch overhead, on P = 2^20 rows; device events; GB/s of ALGORITHMIC bytes (pred, target, weight and the row
                index read once: 44 B per box forward; + d_pred written: 60 B backward)
    counts      launches and host reads of one plan (what the Python side issues; they do not grow with N, G or the levels)
    fp32 error  of the reference's GIoU formula in fp32 torch on the CPU against fp64, on the inputs of tests/test_gpu_atss.py
                (the figure a wider gradient bar would have to be derived from; no test needed one)

There is no pass / fail number -- nothing comparable existed before this head.

    python tools/atss_bench.py [--out profiles/r16_atss.txt] [--reps 20]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SIZES = [(128, 256), (64, 128), (32, 64), (16, 32), (8, 16)]


def bench_targets(torch, n_images, boxes_per_image, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n_images):
        k = boxes_per_image + int(torch.randint(-4, 5, (1,), generator=g))
        xy = torch.rand(k, 2, generator=g) * torch.tensor([W * 0.9, H * 0.9])
        wh = 12 + torch.rand(k, 2, generator=g) ** 2 * torch.tensor([W * 0.4, H * 0.5])
        b = torch.cat([xy, torch.min(xy + wh, torch.tensor([W - 0.5, H - 0.5]))], 1)
        out.append((b, torch.randint(1, 9, (k,), generator=g)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--boxes", type=int, default=30)
    a = ap.parse_args()
    import torch
    import atss_ref as R
    from scan_amd import _lib, ops
    from scan_amd.modeling import atss, fcos
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    shape = ops.PyramidShape(a.images, SIZES)
    targets = bench_targets(torch, a.images, a.boxes, 1024, 2048)
    say("# ATSS head kernels on the bench pyramid: N=%d, levels %s, M=%d rows, boxes per image %s, %d repetitions per figure"
        % (a.images, SIZES, shape.rows, [int(b.shape[0]) for b, _ in targets], a.reps))
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
        return ts[len(ts) // 2], ts[0], ts[-1]

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

    # the two plans alternate, so that a drift of the box hits both
    res = {"atss": [], "fcos": []}
    for _ in range(3):
        res["atss"].append(host_ms(lambda: atss.build_plan(shape, targets, dev)))
        res["fcos"].append(host_ms(lambda: fcos._build_plan(shape, targets, dev)))
    plan = atss.build_plan(shape, targets, dev)
    fplan = fcos._build_plan(shape, targets, dev)
    say("")
    say("ground-truth plan, host clock incl. upload and the host read (median / min / max ms per call; three alternating rounds)")
    for name in ("atss", "fcos"):
        for i, (med, lo, hi) in enumerate(res[name]):
            say("  %-5s round %d   %8.3f / %8.3f / %8.3f" % (name, i, med, lo, hi))
    say("  positives: ATSS %d, FCOS %d" % (plan.n_pos, fplan.n_pos))
    say("  one ATSS plan: %d kernel launches + 2 memsets, %d host read (FCOS: 3 launches + 1 memset, 1 host read)"
        % (atss.plan_stats["launches"], atss.plan_stats["host_reads"]))
    spelled = atss.build_plan(shape, targets, torch.device("cpu"))
    say("  kernels equal the torch spelling on this input: labels %s, matched %s, pos_inds %s"
        % (torch.equal(plan.labels.cpu(), spelled.labels), torch.equal(plan.matched.cpu(), spelled.matched),
           torch.equal(plan.pos_inds.cpu(), spelled.pos_inds)))

    say("")
    say("GIoU loss on anchor deltas (device events, ms per launch; GB/s of algorithmic bytes: 44 B / box forward, 60 B backward)")
    P_, st = ops._ptr, ops._stream
    import ctypes
    strides_h = (ctypes.c_int32 * 5)(*atss.ANCHOR_STRIDES)
    sizes_h = (ctypes.c_float * 5)(*[float(s) for s in atss.ANCHOR_SIZES])
    g = torch.Generator(device=dev).manual_seed(1)
    for label, P in (("plan positives", plan.n_pos), ("2^20 rows", 1 << 20)):
        if P == plan.n_pos:
            rows, target, weight = plan.pos_inds, plan.reg_pos, plan.ctr_pos
        else:
            rows = torch.randint(0, shape.rows, (P,), device=dev, generator=g)
            target = torch.randn((P, 4), device=dev, generator=g)
            weight = torch.rand((P,), device=dev, generator=g) + 0.05
        pred = target + 0.5 * torch.randn((P, 4), device=dev, generator=g)
        out, d, gn = torch.zeros(2, device=dev), torch.empty_like(pred), torch.ones(1, device=dev)
        ws = torch.empty((max(1, ops.query("scan_atss_giou_ordered_ws_floats", P)),), device=dev)
        geo = (shape.ref(), strides_h, sizes_h, P_(pred), P_(target), P_(rows), P_(weight), P)
        t_f = event_ms(lambda: ops.call("scan_atss_giou_forward", *geo, P_(out), st()))
        t_o = event_ms(lambda: ops.call("scan_atss_giou_forward_ordered", *geo, P_(out), P_(ws), st()))
        t_b = event_ms(lambda: ops.call("scan_atss_giou_backward", *geo, P_(gn), P_(d), st()))
        say("  P = %-8d (%s)" % (P, label))
        say("    forward            %9.4f ms   %8.1f GB/s" % (t_f, 44.0 * P / t_f * 1e-6))
        say("    forward, ordered   %9.4f ms   %8.1f GB/s   (two launches)" % (t_o, 44.0 * P / t_o * 1e-6))
        say("    backward           %9.4f ms   %8.1f GB/s" % (t_b, 60.0 * P / t_b * 1e-6))

    say("")
    say("fp32 error of the reference's GIoU formula (torch CPU fp32 against fp64) on the inputs of tests/test_gpu_atss.py,")
    say("in units of the gradient bar (1e-7 + 1e-4 |ref|) and of the value bar (1e-5 |ref|); worst over P in 1, 63, 64, 65, 4097")
    for kind in ("generic", "clamp", "disjoint", "flipped"):
        wg = wv = 0.0
        for P in (1, 63, 64, 65, 4097):
            pred, target, rows, weight = R.giou_inputs(P, kind)
            anchors = R.row_anchors(2, R.SIZES_128x256)[rows]
            p64 = pred.double().requires_grad_(True)
            n64, d64 = R.giou_loss(p64, target.double(), anchors, weight.double())
            (3.0 * n64 / d64).backward()
            p32 = pred.clone().requires_grad_(True)
            n32, d32 = R.giou_loss(p32, target, anchors.float(), weight)
            (3.0 * n32 / d32).backward()
            wg = max(wg, float(((p32.grad.double() - p64.grad).abs() / (1e-7 + 1e-4 * p64.grad.abs())).max()))
            wv = max(wv, abs(float(n32 / d32) - float(n64 / d64)) / (1e-5 * abs(float(n64 / d64))))
        say("  %-9s gradient %.3g x bar, value %.3g x bar" % (kind, wg, wv))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

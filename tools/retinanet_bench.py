#!/usr/bin/env python
"""The RetinaNet head's own kernels on the bench pyramid (N = 4 frames of 1024 x 2048: P3..P7 = 128x256 ... 8x16, M = 174,592
rows, A = 9 anchors per row: 1,571,328 anchors, about 30 boxes per image):

    plan        modeling.retinanet.build_plan (csrc/retina.hip: two passes over all anchors x the image's boxes + the one host
                read), beside the ATSS plan (modeling.atss.build_plan) on the same box in the same run, alternating, both from
                host ground truth through the pinned staging buffers; host clock around a call that ends in a synchronise
    smooth-L1   scan_retina_smooth_l1_forward / _forward_ordered / _backward over ALL anchors (no compaction); device events;
                GB/s of ALGORITHMIC bytes: labels 4 B per anchor forward (+ 4 B matched + 16 B prediction + 16 B box per
                positive, a few thousand: left out), + 16 B d_pred written per anchor backward.  In the same run a streaming
                kernel of the library over a matrix of the size of d_pred (ops.add_relu: 2 reads + 1 write) as the yardstick
    counts      launches and host reads of one plan (what the Python side issues; they do not grow with N, G, A or the levels)

There is no pass / fail number -- nothing comparable existed before this head.

    python tools/retinanet_bench.py [--out profiles/rNN_retinanet.txt] [--reps 20]

Without --out the next free profiles/rNN_retinanet.txt is written.  Needs a GPU: there is no CPU fallback.
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
    return os.path.join(ROOT, "profiles", "r%02d_retinanet.txt" % (max(taken, default=0) + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--boxes", type=int, default=30)
    a = ap.parse_args()
    import torch
    from scan_amd import _lib, ops
    from scan_amd.modeling import atss, retinanet
    if not torch.cuda.is_available():
        raise SystemExit("retinanet_bench: no GPU; the numbers are unmeasured")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    shape = ops.PyramidShape(a.images, SIZES)
    targets = bench_targets(torch, a.images, a.boxes, 1024, 2048)
    cells = retinanet.cell_anchors()
    A = int(cells.shape[1])
    n_anchors = shape.rows * A
    say("# RetinaNet head kernels on the bench pyramid: N=%d, levels %s, M=%d rows, A=%d: %d anchors, boxes per image %s, "
        "%d repetitions per figure" % (a.images, SIZES, shape.rows, A, n_anchors, [int(b.shape[0]) for b, _ in targets], a.reps))
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

    res = {"retinanet": [], "atss": []}
    for _ in range(3):  # the two plans alternate, so that a drift of the box hits both
        res["retinanet"].append(host_ms(lambda: retinanet.build_plan(shape, targets, dev, cells=cells)))
        res["atss"].append(host_ms(lambda: atss.build_plan(shape, targets, dev)))
    plan = retinanet.build_plan(shape, targets, dev, cells=cells)
    aplan = atss.build_plan(shape, targets, dev)
    say("")
    say("ground-truth plan, host clock incl. upload and the host read (median / min / max ms per call; three alternating rounds)")
    for name in ("retinanet", "atss"):
        for i, (med, lo, hi) in enumerate(res[name]):
            say("  %-9s round %d   %8.3f / %8.3f / %8.3f" % (name, i, med, lo, hi))
    say("  positives: RetinaNet %d of %d anchors (label -1: %d), ATSS %d of %d rows"
        % (plan.n_pos, n_anchors, int((plan.labels_i32 == -1).sum()), aplan.n_pos, shape.rows))
    say("  one RetinaNet plan: %d kernel launches + 2 memsets, %d host read (ATSS: %d launches + 2 memsets, %d host read)"
        % (retinanet.plan_stats["launches"], retinanet.plan_stats["host_reads"], atss.plan_stats["launches"],
           atss.plan_stats["host_reads"]))
    spelled = retinanet.build_plan(shape, targets, torch.device("cpu"), cells=cells)
    say("  kernels equal the torch spelling on this input: labels %s, matched %s, n_pos %s"
        % (torch.equal(plan.labels_i32.cpu(), spelled.labels_i32), torch.equal(plan.matched.cpu(), spelled.matched),
           plan.n_pos == spelled.n_pos))

    say("")
    say("smooth-L1 over all %d anchors (device events, ms per launch; GB/s of algorithmic bytes: 4 B / anchor forward, 20 B backward)"
        % n_anchors)
    P_, st = ops._ptr, ops._stream
    g = torch.Generator(device=dev).manual_seed(1)
    reg = torch.randn((shape.rows, 4 * A), device=dev, generator=g)
    out, d, gn = torch.zeros(1, device=dev), torch.empty_like(reg), torch.ones(1, device=dev)
    ws = torch.empty((max(1, ops.query("scan_retina_smooth_l1_ordered_ws_floats", n_anchors)),), device=dev)
    dcells = retinanet.device_cells(cells, dev)
    geo = (shape.ref(), (ctypes.c_int32 * 5)(*retinanet.ANCHOR_STRIDES), P_(dcells), A, P_(plan.boxes), plan.boxes.shape[1],
           P_(plan.labels_i32), P_(plan.matched), P_(reg), 4 * A, 0.11)
    other = torch.randn_like(reg)
    t_f = event_ms(lambda: ops.call("scan_retina_smooth_l1_forward", *geo, None, P_(out), st()))
    t_o = event_ms(lambda: ops.call("scan_retina_smooth_l1_forward_ordered", *geo, None, P_(out), P_(ws), st()))
    t_b = event_ms(lambda: ops.call("scan_retina_smooth_l1_backward", *geo, P_(gn), P_(d), 4 * A, st()))
    t_s = event_ms(lambda: ops.add_relu(reg, other))
    say("  forward            %9.4f ms   %8.1f GB/s" % (t_f, 4.0 * n_anchors / t_f * 1e-6))
    say("  forward, ordered   %9.4f ms   %8.1f GB/s   (two launches)" % (t_o, 4.0 * n_anchors / t_o * 1e-6))
    say("  backward           %9.4f ms   %8.1f GB/s" % (t_b, 20.0 * n_anchors / t_b * 1e-6))
    say("  add_relu, same run %9.4f ms   %8.1f GB/s   (streaming yardstick: [%d, %d] fp32, 2 reads + 1 write, incl. torch's "
        "allocation of the output)" % (t_s, 12.0 * reg.numel() / t_s * 1e-6, reg.shape[0], reg.shape[1]))
    path = a.out or next_profile()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", path)


if __name__ == "__main__":
    main()

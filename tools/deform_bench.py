#!/usr/bin/env python
"""Deformable convolution (DCNv2) on the bench pyramid, step by step (N = 4 frames of 1024 x 2048: P3..P7 = 128x256 ... 8x16,
M = 174,592 rows; C = 256 -> 256, modulated): time per launch of

    sample forward     scan_deform_sample_forward: x read, cols [M, 9 * 256] written
    contraction        the 1x1 conv over cols (ops.conv2d, K = 2304) -- forward, then data + weight gradient
    sample backward    scan_deform_sample_backward: x and dcols read; doffset, dmask and the (key, weight) entries written
    sort               torch.sort(keys, stable=True) + searchsorted: the inverted index of the data gradient
    gather             scan_deform_dx_gather: dcols read through the index, dx written

with the ALGORITHMIC bytes of the memory-bound steps (what each must read and write once; the four corner rows of a tap
overlap its neighbours' and are counted once as x) over the time, beside the HBM rate tools/pointwise_roofline.py measures
on the same box in the same process (grl_scale: a read + write stream; groupnorm_relu_apply: the 256-channel row pass).  For
scale: the plain 3x3 tower conv of the same shape, forward and data + weight gradient, and the whole op through
ops.deform_conv2d.  There is no pass / fail number -- nothing comparable existed before this op.

    python tools/deform_bench.py [--out profiles/r15_deform_conv.txt] [--reps 5] [--mode bf16x6]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

SIZES = [(128, 256), (64, 128), (32, 64), (16, 32), (8, 16)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--mode", default="bf16x6", choices=["bf16x6", "bf16x3", "fp32"])
    a = ap.parse_args()
    import torch
    import pointwise_roofline
    from scan_amd import _lib, ops
    dev = torch.device("cuda:0")
    ops.CONV_MODE = a.mode
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def ms(fn):
        return pointwise_roofline._time(fn, a.reps, torch) * 1e-3

    hbm = {r["kernel"]: r for r in pointwise_roofline.measure(dev, sizes=(1 << 22,), reps=a.reps,
                                                               only={"grl_scale", "groupnorm_relu_apply"})}
    torch.cuda.empty_cache()
    shape = ops.PyramidShape(a.images, SIZES)
    M, C, O = shape.rows, 256, 256
    say("# deformable conv v2 on the bench pyramid: N=%d, levels %s, M=%d rows, C=%d -> O=%d, CONV_MODE=%s, %d launches per figure"
        % (a.images, SIZES, M, C, O, a.mode, a.reps))
    say("# library: %s" % _lib.lib_identity())
    say("# HBM rate of this box (tools/pointwise_roofline.py, M = 2^22): " + ", ".join(
        "%s %.0f GB/s" % (k, r["GBps"]) for k, r in hbm.items()))
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((M, C), device=dev, generator=g)
    om = torch.empty((M, 28), device=dev)
    om[:, :18] = torch.rand((M, 18), device=dev, generator=g) * 5 - 2.5
    om[:, 18:] = torch.sigmoid(torch.randn((M, 10), device=dev, generator=g))
    mask = om[:, 18:27]
    w = (torch.randn((O, C, 3, 3), device=dev, generator=g) / (9 * C) ** 0.5).contiguous(memory_format=torch.channels_last)
    b = torch.randn((O,), device=dev, generator=g)
    gy = torch.randn((M, O), device=dev, generator=g)
    P, st = ops._ptr, ops._stream
    fl = 2.0 * M * O * 9 * C

    def mem(name, t, nbytes, what):
        say("%-34s %9.3f ms   %7.1f GB/s   (%s)" % (name, t, nbytes / t * 1e-6, what))

    def mma(name, t, flops):
        say("%-34s %9.3f ms   %7.1f TFLOP/s" % (name, t, flops / t * 1e-9))

    cols = torch.empty((M, 9 * C), device=dev)
    t = ms(lambda: _lib.call("scan_deform_sample_forward", P(x), shape.ref(), C, C, P(om), 28, P(mask), 28, P(cols), st()))
    mem("sample forward", t, 4.0 * M * (C + 27 + 9 * C), "x + offsets + mask read, cols written")
    w1 = w.permute(0, 2, 3, 1).reshape(O, 9 * C, 1, 1).requires_grad_(True)
    bl = b.clone().requires_grad_(True)
    with torch.no_grad():
        mma("contraction forward (1x1, K=2304)", ms(lambda: ops.conv2d(cols, w1, bl, shape, 1, 1)), fl)
    cl = cols.requires_grad_(True)
    y = ops.conv2d(cl, w1, bl, shape, 1, 1)
    mma("contraction dgrad + wgrad", ms(lambda: torch.autograd.grad(y, [cl, w1, bl], gy, retain_graph=True)), 2 * fl)
    dcols = torch.autograd.grad(y, [cl], gy)[0].contiguous()
    del y, cl
    cols = None
    torch.cuda.empty_cache()
    doff, dmask = torch.empty((M, 28), device=dev), torch.empty((M, 9), device=dev)
    keys, wgts = torch.empty((36 * M,), dtype=torch.int32, device=dev), torch.empty((36 * M,), device=dev)
    t = ms(lambda: _lib.call("scan_deform_sample_backward", P(x), shape.ref(), C, C, P(dcols), P(om), 28, P(mask), 28, P(doff), 28,
                             P(dmask), 9, P(keys), P(wgts), st()))
    mem("sample backward", t, 4.0 * M * (C + 9 * C + 27 + 28 + 9 + 72), "x + dcols + offsets + mask read; doffset, dmask, entries written")
    rows = torch.arange(M + 1, dtype=torch.int32, device=dev)
    t_sort = ms(lambda: torch.sort(keys, stable=True))
    skeys, perm = torch.sort(keys, stable=True)
    t_seg = ms(lambda: torch.searchsorted(skeys, rows))
    seg = torch.searchsorted(skeys, rows)
    say("%-34s %9.3f ms   %7.1f M entries/s   (torch.sort stable, int32 keys; + searchsorted %.3f ms)"
        % ("sort (%d entries)" % (36 * M), t_sort, 36 * M / t_sort * 1e-3, t_seg))
    per = (seg[1:] - seg[:-1]).float()
    say("#   entries per destination row: median %.0f, max %.0f; %.1f %% of the entries have no destination"
        % (float(per.median()), float(per.max()), 100.0 * float((keys == M).float().mean())))
    dx = torch.empty_like(x)
    t = ms(lambda: _lib.call("scan_deform_dx_gather", P(dcols), P(perm), P(seg), P(wgts), M, C, C, P(dx), st()))
    mem("gather (dx)", t, 4.0 * M * (9 * C + C) + 36.0 * M * 12, "dcols + index + weights read, dx written")
    del dcols, keys, wgts, skeys, perm, seg, dx, doff, dmask
    torch.cuda.empty_cache()
    # the whole op, and the plain 3x3 tower conv of the same shape for scale
    xl, wl = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    oml = om.clone().requires_grad_(True)
    with torch.no_grad():
        t_f = ms(lambda: ops.deform_conv2d(xl, oml, oml[:, 18:27], wl, bl, shape))
    say("%-34s %9.3f ms" % ("ops.deform_conv2d forward", t_f))
    yd = ops.deform_conv2d(xl, oml, oml[:, 18:27], wl, bl, shape)
    say("%-34s %9.3f ms" % ("ops.deform_conv2d backward",
                            ms(lambda: torch.autograd.grad(yd, [xl, oml, wl, bl], gy, retain_graph=True))))
    del yd
    torch.cuda.empty_cache()
    with torch.no_grad():
        mma("plain conv3x3 forward", ms(lambda: ops.conv2d(xl, wl, bl, shape, 3, 1)), fl)
    yp = ops.conv2d(xl, wl, bl, shape, 3, 1)
    mma("plain conv3x3 dgrad + wgrad", ms(lambda: torch.autograd.grad(yp, [xl, wl, bl], gy, retain_graph=True)), 2 * fl)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

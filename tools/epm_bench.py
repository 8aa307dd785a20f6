#!/usr/bin/env python
"""The EPM baseline on the bench pyramid (2 source + 2 target frames of 1024 x 2048: P3..P7 = 128x256 ... 8x16, M = 174,592
rows of the paired pyramid):

    step      epm.EPMTrainer.step for GA and for GA + CA ('ca_feature') beside engine.Trainer.step (the SCAN step) in the same
              process, the three alternating over several rounds so that a drift of the box hits all of them; host clock around
              a window of steps that ends in a synchronise, ms per step
    kernels   scan_center_aware_map (C = 8 of Cs = 8 class columns, centerness as a column of an 8-wide matrix) and
              scan_row_scale_levels (256 channels, forward s = 1 and backward s_l = -lambda_l through the level-pointer form) on
              those rows; device events; GB/s of ALGORITHMIC bytes (map: the class rows and the centerness read, the map written;
              row scale: x read, y written, the map read) beside scan_scale -- a plain float4 stream -- on as many elements
    error     of the map kernel against fp64, beside the fp32 torch expressions on the CPU, in ulps of [1/2, 1)

There is no pass / fail number -- nothing comparable existed before.

    python tools/epm_bench.py [--out profiles/r17_epm.txt] [--steps 10] [--rounds 2] [--reps 50]
"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SIZES = [(128, 256), (64, 128), (32, 64), (16, 32), (8, 16)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--skip-steps", action="store_true")
    a = ap.parse_args()
    import torch
    import epm_ref
    from scan_amd import _lib, engine, epm, ops, synth
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    H, W, B = a.height, a.width, 2
    say("# EPM baseline on the bench pyramid: %d + %d frames of %d x %d, conv mode %s" % (B, B, H, W, ops.CONV_MODE))
    say("# library: %s" % _lib.lib_identity())

    if not a.skip_steps:
        imgs_s, imgs_t = synth.synth_images(B, H, W, 1234).to(dev), synth.synth_images(B, H, W, 2234).to(dev)
        tg = synth.synth_targets(B, H, W, 8, 12, 4321)

        def make(kind):
            if kind == "scan":
                model = engine.build_model(9, device=dev, attn_dropout=0.0)
                engine.load_procedural_weights(model)
                tr = engine.Trainer(model)
            else:
                model = epm.build_model(9, adv=("ga",) if kind == "ga" else ("ga", "ca"), device=dev)
                epm.load_procedural_weights(model)
                tr = epm.EPMTrainer(model)
            return tr

        kinds = ("scan", "ga", "ga+ca")
        trainers = {k: make(k) for k in kinds}
        for k in kinds:  # every shape the timed windows use
            for _ in range(3):
                trainers[k].step(imgs_s, tg, imgs_t)
        torch.cuda.synchronize()
        res = {k: [] for k in kinds}
        for _ in range(a.rounds):
            for k in kinds:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    trainers[k].step(imgs_s, tg, imgs_t)
                torch.cuda.synchronize()
                res[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
        say("")
        say("one adaptation iteration, ms per step (host clock around %d steps ending in a synchronise; %d alternating rounds)"
            % (a.steps, a.rounds))
        for k in kinds:
            say("  %-6s %s" % (k, "  ".join("%8.2f" % v for v in res[k])))
        del trainers
        torch.cuda.empty_cache()

    def event_ms(fn):
        for _ in range(5):
            fn()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for _ in range(a.reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.reps

    shape = ops.PyramidShape(2 * B, SIZES if (H, W) == (1024, 2048) else [(-(-H // s), -(-W // s)) for s in (8, 16, 32, 64, 128)])
    M, C = shape.rows, 256
    P_, st = ops._ptr, ops._stream
    g = torch.Generator(device=dev).manual_seed(1)
    cls = torch.randn((M, 8), device=dev, generator=g) * 3.0
    out8 = torch.randn((M, 8), device=dev, generator=g)
    atten = torch.empty((M,), device=dev)
    x = torch.randn((M, C), device=dev, generator=g)
    y = torch.empty_like(x)
    ones = (ctypes.c_float * 5)(*[1.0] * 5)
    lams = (ctypes.c_float * 5)(*[-0.02] * 5)
    parts = [x[shape.row_off[l]:shape.row_off[l + 1]].clone() for l in range(5)]
    ptrs = (ctypes.c_void_p * 5)(*[p.data_ptr() for p in parts])
    say("")
    say("kernels on M = %d rows (device events over %d launches, ms per launch; GB/s of algorithmic bytes)" % (M, a.reps))
    # the three alternate twice, so that a drift of the box shows
    for rnd in range(2):
        t_map = event_ms(lambda: ops.call("scan_center_aware_map", P_(cls), 8, 8, P_(out8[:, 4]), 8, 20.0, M, P_(atten), st()))
        t_fwd = event_ms(lambda: ops.call("scan_row_scale_levels", P_(x), C, P_(atten), ones, shape.ref(), C, P_(y), C, st()))
        t_bwd = event_ms(lambda: ops.call("scan_row_scale_levels_ptrs", ptrs, C, P_(atten), lams, shape.ref(), C, P_(y), C, st()))
        t_str = event_ms(lambda: ops.call("scan_scale", P_(x), -0.02, P_(y), M * C, st()))
        b_map, b_rs, b_str = M * (8 + 1 + 1) * 4.0, M * (2 * C + 1) * 4.0, M * 2 * C * 4.0
        say("  round %d" % rnd)
        say("    scan_center_aware_map           %9.4f ms   %8.1f GB/s   (%.1f MB)" % (t_map, b_map / t_map * 1e-6, b_map * 1e-6))
        say("    scan_row_scale_levels   s = 1   %9.4f ms   %8.1f GB/s   (%.1f MB)" % (t_fwd, b_rs / t_fwd * 1e-6, b_rs * 1e-6))
        say("    scan_row_scale_levels_ptrs -lam %9.4f ms   %8.1f GB/s" % (t_bwd, b_rs / t_bwd * 1e-6))
        say("    scan_scale (plain stream)       %9.4f ms   %8.1f GB/s   (%.1f MB)" % (t_str, b_str / t_str * 1e-6, b_str * 1e-6))

    ref = epm_ref.center_aware_map(cls.cpu(), out8[:, 4].cpu(), 20.0)
    ops.call("scan_center_aware_map", P_(cls), 8, 8, P_(out8[:, 4]), 8, 20.0, M, P_(atten), st())
    e_k = float((atten.cpu().double() - ref).abs().max()) / 2.0 ** -24
    e_t = float((epm_ref.center_aware_map_fp32(cls.cpu(), out8[:, 4].cpu(), 20.0).double() - ref).abs().max()) / 2.0 ** -24
    say("")
    say("map against fp64 on those rows, worst error in ulps of [1/2, 1): kernel %.2f, fp32 torch expressions on the CPU %.2f"
        % (e_k, e_t))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

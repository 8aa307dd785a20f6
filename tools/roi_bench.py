#!/usr/bin/env python
"""Region pooling on the bench pyramid (2 frames of 1024 x 2048: P3..P7 = 128x256 ... 8x16, M = 87,296 rows, C = 256), 512
ROIs per image with log-uniform sizes so that every level is used, 7 x 7 bins, sampling_ratio 2:

    kernels   scan_roi_align_forward / _backward and scan_roi_pool_forward / _backward on the row matrix, device events, the
              median of several alternating rounds; ALGORITHMIC bytes (what the operation must move once: the rows a ROI's
              samples or windows touch counted once per (ROI, bin), the pooled tensor, the gradient rows) and the rate they
              give, beside scan_scale -- a plain float4 stream -- on the M x C elements in the same run
    pooler    modeling.poolers.Pooler (one pack + one level-mapper launch + one pooling launch) against the same work done
              level by level through layers.ROIAlign (the reference's loop, modeling/poolers.py:116-119), same process,
              alternating; host clock around a window that ends in a synchronise; forward, and forward + backward
    error     worst |error| / bound of the forward and of the gradients on the cases of tests/test_gpu_roi.py (bounds derived
              from the operation counts in tests/roi_ref.py)

Only the per-destination form of the gradients exists (csrc/roi.hip); a float-atomic form was not built and not measured.
There is no pass / fail number -- nothing comparable existed before.

    python tools/roi_bench.py [--out profiles/r18_roi.txt] [--reps 30] [--rounds 5]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SIZES = [(128, 256), (64, 128), (32, 64), (16, 32), (8, 16)]
SCALES = [1 / 8, 1 / 16, 1 / 32, 1 / 64, 1 / 128]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rois", type=int, default=512)
    ap.add_argument("--skip-error", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    from scan_amd import _lib, ops
    from scan_amd.modeling import poolers
    from scan_amd.structures import BoxList
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    N, C, PH, PW, SR, Himg, Wimg = 2, 256, 7, 7, 2, 1024, 2048
    shape = ops.PyramidShape(N, SIZES)
    M, K = shape.rows, N * a.rois
    rs = np.random.RandomState(0)
    per_image = []
    for n in range(N):
        # log-uniform sqrt(area) from 16 to 2400 pixels: P7 starts at 1792, more than a 1024 x 2048 image holds, so the boxes
        # are proposals before clipping (centres inside the image) -- every level is used
        side = np.exp(rs.uniform(np.log(16), np.log(2400), a.rois))
        ar = np.exp(rs.uniform(np.log(0.5), np.log(2.0), a.rois))
        w, h = side * np.sqrt(ar), side / np.sqrt(ar)
        cx, cy = rs.uniform(0, Wimg, a.rois), rs.uniform(0, Himg, a.rois)
        b = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)
        per_image.append(torch.tensor(b, dtype=torch.float32))
    boxes = [BoxList(b.to(dev), (Wimg, Himg)) for b in per_image]
    pooler = poolers.Pooler((PH, PW), SCALES, SR)
    rois = pooler.convert_to_roi_format(boxes).float().contiguous()
    m = pooler.map_levels
    levels = ops.roi_levels(rois, m.k_min, m.k_max)
    per_level = torch.bincount(levels.long(), minlength=5).cpu().tolist()
    say("# region pooling on the bench pyramid: %d frames of %d x %d, M = %d rows, C = %d, K = %d ROIs, %d x %d bins, "
        "sampling_ratio %d" % (N, Himg, Wimg, M, C, K, PH, PW, SR))
    say("# ROIs per level P3..P7: %s" % per_level)
    say("# library: %s" % _lib.lib_identity())

    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((M, C), device=dev, generator=g)
    y = torch.empty((K, PH, PW, C), device=dev)
    am = torch.empty((K, PH, PW, C), device=dev, dtype=torch.int32)
    dy = torch.randn((K, PH, PW, C), device=dev, generator=g)
    dx = torch.empty((M, C), device=dev)
    x2 = torch.empty_like(x)
    sc = (ctypes.c_float * 5)(*SCALES)
    P_, st = ops._ptr, ops._stream

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

    kern = {
        "roi_align_forward": lambda: ops.call("scan_roi_align_forward", P_(x), shape.ref(), C, C, P_(rois), P_(levels), sc, K, PH, PW,
                                              SR, P_(y), st()),
        "roi_align_backward": lambda: ops.call("scan_roi_align_backward", P_(dy), shape.ref(), C, C, P_(rois), P_(levels), sc, K, PH,
                                               PW, SR, P_(dx), st()),
        "roi_pool_forward": lambda: ops.call("scan_roi_pool_forward", P_(x), shape.ref(), C, C, P_(rois), P_(levels), sc, K, PH, PW,
                                             P_(y), P_(am), st()),
        "roi_pool_backward": lambda: ops.call("scan_roi_pool_backward", P_(dy), P_(am), shape.ref(), C, C, P_(rois), P_(levels), sc, K,
                                              PH, PW, P_(dx), st()),
        "scan_scale (stream)": lambda: ops.call("scan_scale", P_(x), -0.02, P_(x2), M * C, st()),
    }
    # algorithmic bytes, from the geometry the kernels themselves report / the restatement's rules
    grid, pos, wgt, cell = ops.roi_align_samples(shape, rois, (PH, PW), SCALES, SR, SR, levels=levels)
    live_corners = int((cell >= 0).sum())
    # distinct rows per (ROI, bin): at most 4 * SR * SR, fewer where samples share cells
    c_sorted = torch.sort(cell.view(K * PH * PW, -1), dim=1).values
    distinct = int(((c_sorted[:, 1:] != c_sorted[:, :-1]) & (c_sorted[:, 1:] >= 0)).sum() + (c_sorted[:, 0] >= 0).sum())
    kern["roi_pool_forward"]()
    torch.cuda.synchronize()
    out_b = K * PH * PW * C * 4.0
    bytes_ = {
        "roi_align_forward": distinct * C * 4.0 + out_b,
        "roi_align_backward": out_b + M * C * 4.0,      # dy read once, every row of dx written
        "roi_pool_forward": None,                        # filled below from the windows
        "roi_pool_backward": 2 * out_b + M * C * 4.0,   # dy and argmax read once, dx written
        "scan_scale (stream)": 2.0 * M * C * 4.0,
    }
    import roi_ref
    win = 0
    rl, ll = rois.cpu().tolist(), levels.cpu().tolist()
    for k in range(K):
        hb, wb = roi_ref.pool_bins(rl[k], SCALES[ll[k]], PH, PW, *SIZES[ll[k]])
        win += sum(max(he - hs, 0) for hs, he in hb) * sum(max(we - ws, 0) for ws, we in wb)
    bytes_["roi_pool_forward"] = win * C * 4.0 + 2 * out_b
    say("")
    say("kernels (device events over %d launches, ms per launch; median [min .. max] of %d alternating rounds; GB/s of "
        "algorithmic bytes at the median)" % (a.reps, a.rounds))
    say("  ROIAlign: %d live (sample, corner) rows requested, %d distinct per (ROI, bin); ROIPool windows hold %d cells"
        % (live_corners, distinct, win))
    res = {k: [] for k in kern}
    for _ in range(a.rounds):
        for k, fn in kern.items():
            res[k].append(event_ms(fn))
    for k in kern:
        med = statistics.median(res[k])
        say("    %-22s %9.4f ms  [%.4f .. %.4f]   %8.1f GB/s   (%.1f MB)"
            % (k, med, min(res[k]), max(res[k]), bytes_[k] / med * 1e-6, bytes_[k] * 1e-6))

    # ---- the one-launch pooler against the per-level loop
    feats = [torch.randn((N, C, h, w), device=dev, generator=g).contiguous(memory_format=torch.channels_last) for h, w in SIZES]
    gout = torch.randn((K, C, PH, PW), device=dev, generator=g)

    def loop_pooler(fs):
        lv = pooler.map_levels(boxes)
        result = torch.zeros((K, C, PH, PW), device=dev)
        for level, (f, p) in enumerate(zip(fs, pooler.poolers)):
            idx = torch.nonzero(lv == level).squeeze(1)
            result[idx] = p(f, rois[idx])
        return result

    def fwd(fn):
        with torch.no_grad():
            fn(feats)

    def fwd_bwd(fn):
        fs = [f.detach().requires_grad_(True) for f in feats]
        fn(fs).backward(gout)

    def window_ms(run, fn, steps=10):
        for _ in range(3):
            run(fn)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            run(fn)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    same = torch.equal(pooler(feats, boxes), loop_pooler(feats))
    say("")
    say("Pooler on five NCHW (channels_last) levels, ms per call (host clock around 10 calls ending in a synchronise; median "
        "[min .. max] of %d alternating rounds); outputs bit-identical: %s" % (a.rounds, same))
    forms = (("one launch (Pooler)", lambda fs: pooler(fs, boxes)), ("per-level loop", loop_pooler))
    for label, run in (("forward", fwd), ("forward + backward", fwd_bwd)):
        r = {n: [] for n, _ in forms}
        for _ in range(a.rounds):
            for n, fn in forms:
                r[n].append(window_ms(run, fn))
        for n, _ in forms:
            say("    %-20s %-20s %9.3f ms  [%.3f .. %.3f]" % (label, n, statistics.median(r[n]), min(r[n]), max(r[n])))

    if not a.skip_error:
        import roi_ref as R
        say("")
        say("worst |error| / bound on the test pyramid (13x17 / 7x9 / 4x5, 257 ROIs; bounds from the operation counts, "
            "tests/roi_ref.py)")
        rr, lv = R.make_rois(257)
        rl, ll = rr.tolist(), lv.tolist()
        tshape = ops.PyramidShape(R.N_IMAGES, list(R.SIZES))
        worst = {"align forward": 0.0, "align backward": 0.0, "pool backward": 0.0}
        for size in ((1, 1), (2, 3), (7, 7)):
            for sr in (0, 1, 2, 3):
                xs = R.make_rows(8, 3)
                xd = xs.to(dev).requires_grad_(True)
                yy = ops.roi_align(xd, tshape, rr.to(dev), size, R.SCALES, sr, levels=lv.to(dev))
                gy = torch.randn(yy.shape, generator=torch.Generator().manual_seed(sr))
                yy.backward(gy.to(dev))
                f = R.roi_align(xs, rl, ll, size[0], size[1], sr)
                b = R.roi_align_backward(gy, rl, ll, size[0], size[1], sr)
                worst["align forward"] = max(worst["align forward"],
                                             float(((yy.detach().cpu().double() - f["y"]).abs() / R.align_forward_bound(f)).max()))
                worst["align backward"] = max(worst["align backward"],
                                              float(((xd.grad.cpu().double() - b["dx"]).abs() / R.align_backward_bound(b)).max()))
            xs = torch.round(R.make_rows(8, 4) * 1.5)
            xd = xs.to(dev).requires_grad_(True)
            yy, aa = ops.roi_pool(xd, tshape, rr.to(dev), size, R.SCALES, levels=lv.to(dev), return_argmax=True)
            gy = torch.randn(yy.shape, generator=torch.Generator().manual_seed(9))
            yy.backward(gy.to(dev))
            ry, ra = R.roi_pool(xs, rl, ll, size[0], size[1])
            assert torch.equal(yy.detach().cpu(), ry) and torch.equal(aa.cpu(), ra), "ROIPool forward is exact"
            b = R.roi_pool_backward(gy, ra, rl, ll)
            worst["pool backward"] = max(worst["pool backward"],
                                         float(((xd.grad.cpu().double() - b["dx"]).abs() / R.pool_backward_bound(b).clamp_min(1e-300)).max()))
        for k, v in worst.items():
            say("    %-16s %.3f" % (k, v))
        say("    pool forward     exact (values and argmax equal)")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

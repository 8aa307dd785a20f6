"""Generic class-count kernels next to what they stand beside, at the bench workload's pyramid (4 frames of 1024x2048:
174592 rows): (a) dynamic conv + softmax forward and backward at K = 9, the <9> instances against the generic kernels
(scan_tune "dynconv_generic"), and the generic kernels at K = 8 / 21 / 32; (b) the class-branch output conv at Cf = 7,
generic grouped kernels against the dense conv over the block-diagonal weight.  HIP events, warm, median of 21 launches.

    python tools/class_count_bench.py
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scan_amd import _lib, ops  # noqa: E402

dev = torch.device("cuda", 0)
SIZES = [(128, 256), (64, 128), (32, 64), (16, 32), (8, 16)]
REPS = 21


def timed(fwd, bwd):
    """median ms of fwd() and of bwd(y) over REPS launches after 3 warm ones"""
    tf, tb = [], []
    for i in range(3 + REPS):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        y = fwd()
        e[1].record()
        bwd(y)
        e[2].record()
        torch.cuda.synchronize()
        if i >= 3:
            tf.append(e[0].elapsed_time(e[1]))
            tb.append(e[1].elapsed_time(e[2]))
    return statistics.median(tf), statistics.median(tb)


def dynconv(K, generic):
    M = 4 * sum(h * w for h, w in SIZES)
    feat = torch.randn(M, 256, device=dev).requires_grad_(True)
    ker = (torch.randn(K, 256, device=dev) / 16).requires_grad_(True)
    g1, g2 = torch.randn(M, K, device=dev), torch.randn(M, K, device=dev)
    old = _lib.query("scan_tune", b"dynconv_generic", int(generic))
    try:
        f, b = timed(lambda: ops.dynconv_softmax(feat, ker), lambda y: torch.autograd.backward(y, (g1, g2)))
    finally:
        _lib.query("scan_tune", b"dynconv_generic", old)
    print("dynconv M=%d K=%-2d %-11s fwd %.3f ms  bwd %.3f ms" % (M, K, "generic" if generic else "specialised", f, b))


def class_branch(G):
    shape = ops.PyramidShape(4, SIZES)
    x = torch.relu(torch.randn(shape.rows, G * 128, device=dev))
    ws = torch.zeros(G, G * 128, 3, 3, device=dev)
    for c in range(G):
        ws[c, c * 128:(c + 1) * 128] = torch.randn(128, 3, 3, device=dev) / 30
    ws = ws.contiguous(memory_format=torch.channels_last)
    bias = torch.randn(G, device=dev)
    for name, fn in (("grouped", lambda xx, ww: ops.gconv3x3_to1(xx, ww, bias, shape, G, mask_dx=True)),
                     ("dense", lambda xx, ww: ops.conv2d(xx, ww, bias, shape, 3, 1, mask_dx=True))):
        xx, ww = x.clone().requires_grad_(True), ws.clone().requires_grad_(True)
        gy = torch.ones((shape.rows, ops.pad4(G)), device=dev)
        f, b = timed(lambda: fn(xx, ww), lambda y: y.backward(gy))
        print("class branch rows=%d G=%-2d %-8s fwd %.3f ms  bwd %.3f ms" % (shape.rows, G, name, f, b))


if __name__ == "__main__":
    print(_lib.lib_identity())
    dynconv(9, False)
    dynconv(9, True)
    for K in (8, 21, 32):
        dynconv(K, True)
    class_branch(7)
    class_branch(8)

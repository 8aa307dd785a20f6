#!/usr/bin/env python
"""Host emulation of the rounding of three 3x3 conv arithmetics against fp64, at the shapes of CONV_ERR_CASES
(tests/test_gpu_kernels.py), for the 1-D Winograd F(2,3) path of the bf16x6 kernels (csrc/conv_fwd.hip, conv_wino):

    direct    bf16x6 as conv_split_kernel runs it: both operands cut into three bf16 pieces (exact), per (32-channel chunk,
              tap) six piece products, each summed exactly over its 32 channels and added to the fp32 accumulator with ONE
              rounding (the model of one v_mfma_f32_16x16x32_bf16), smallest terms first
    wino      the same on the Winograd operands: U = B^T d in fp32 (one rounding per value), Gg in fp64 rounded once to fp32,
              both split exactly; four accumulators m_j over (chunk, ky); y0 = m0 + (m1 + m2), y1 = (m1 - m2) - m3 in fp32
    fp32      an fp32 FMA chain in the fp32-MFMA kernel's K order (tap-major, channels inside)

Samples are output PAIRS (x, x + 1) of one output channel; inputs ~ N(0, 1), weights ~ N(0, 1) / sqrt(9 Cin) as in the
GPU test.  Prints per case the rms and worst error relative to the largest sampled output, and the ratios to fp32.

    python tools/wino_numerics.py [--samples 4096] [--seed 0]

--wgrad: the same question for the 3x3 WEIGHT gradient with F(2,3) applied across rows (csrc/conv_wgrad.hip, wgrad_wino), see
emulate_wgrad.  profiles/r08_wgrad_wino_numerics.txt is its output; tests/test_wgrad_wino_numerics.py pins it.
"""
import argparse

import numpy as np
import torch

# F(2,3):  y = A^T [ (G g) * (B^T d) ]
BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64)
G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=np.float64)
AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64)

# Cin of the CONV_ERR_CASES shapes (the K length is what sets the accumulation error; pixel geometry does not enter)
CASES = [256, 268, 264, 512, 128]


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def split3(a):
    """exact three-piece bf16 split of fp32 values (conv_split.h split1_np<3>), as fp64 arrays"""
    r = torch.from_numpy(np.asarray(a, dtype=np.float32))
    out = []
    for _ in range(3):
        q = r.to(torch.bfloat16).to(torch.float32)
        out.append(q.double().numpy())
        r = r - q
    return out


def mma_acc(acc, wp, xp):
    """one (chunk, tap) of mma_pieces<3>: x0 w2, x1 w1, x2 w0, x0 w1, x1 w0, x0 w0 -- each 32-channel product sum exact,
    one fp32 rounding per MFMA.  wp, xp: three pieces [S, 32]"""
    for s in (2, 1, 0):
        for i in range(s + 1):
            acc = f32(acc + (wp[i] * xp[s - i]).sum(-1))
    return acc


def emulate(cin, n, seed):
    rs = np.random.RandomState(seed)
    cs = (cin + 31) // 32 * 32
    d = np.zeros((n, 3, 4, cs), np.float32)   # [S, ky, halo column, channel]: input window of one output pair
    g = np.zeros((n, 3, 3, cs), np.float32)   # [S, ky, kx, channel]: the weights of one output channel
    d[..., :cin] = rs.standard_normal((n, 3, 4, cin))
    g[..., :cin] = rs.standard_normal((n, 3, 3, cin)) / np.sqrt(9 * cin)
    d64, g64 = d.astype(np.float64), g.astype(np.float64)
    ref = np.stack([np.einsum("skc,skc->s", d64[:, :, e:e + 3].reshape(n, 9, cs), g64.reshape(n, 9, cs)) for e in (0, 1)], 1)

    # fp32 FMA chain, tap-major
    y32 = np.zeros((n, 2))
    for e in (0, 1):
        acc = np.zeros(n)
        for ky in range(3):
            for kx in range(3):
                for c in range(cin):
                    acc = f32(acc + d64[:, ky, e + kx, c] * g64[:, ky, kx, c])
        y32[:, e] = acc

    # direct bf16x6: chunk-major, then the nine taps
    ydir = np.zeros((n, 2))
    for e in (0, 1):
        acc = np.zeros(n)
        for c0 in range(0, cs, 32):
            for ky in range(3):
                for kx in range(3):
                    acc = mma_acc(acc, split3(g[:, ky, kx, c0:c0 + 32]), split3(d[:, ky, e + kx, c0:c0 + 32]))
        ydir[:, e] = acc

    # Winograd F(2,3) along x: U_j = (B^T d)_j in fp32, V_j = (G g)_j in fp64 -> fp32; accumulators in the kernel's
    # (chunk, j, ky) order -- each m_j only sees its own (chunk, ky) sequence
    U = f32(np.einsum("jk,sykc->syjc", BT, d64))   # [S, ky, j, c]
    V = f32(np.einsum("jk,sykc->syjc", G, g64))
    m = np.zeros((n, 4))
    for c0 in range(0, cs, 32):
        for j in range(4):
            for ky in range(3):
                m[:, j] = mma_acc(m[:, j], split3(V[:, ky, j, c0:c0 + 32]), split3(U[:, ky, j, c0:c0 + 32]))
    ywin = np.stack([f32(m[:, 0] + f32(m[:, 1] + m[:, 2])), f32(f32(m[:, 1] - m[:, 2]) - m[:, 3])], 1)

    scale = np.abs(ref).max()
    res = {}
    for name, y in (("fp32", y32), ("direct", ydir), ("wino", ywin)):
        e = np.abs(y - ref) / scale
        res[name] = (float(np.sqrt((e ** 2).mean())), float(e.max()))
    return res


# ---- weight gradient, F(2,3) across rows -------------------------------------------------------------------------------
# One sample is one (o, c, kx) of one image: dY column e[y][x] and X column d[y][x] (rows -1 and H are zero padding), and
# the three gradients dW[ky] = sum_{y, x} e[y][x] d[y + ky - 1][x].  K runs over 32-pixel chunks of a row (direct) or of a
# row pair (Winograd), split into slabs of `cps` chunks as wgrad_plan does; the slabs are summed in fp64.
WGRAD_CLASSES = ("gauss", "relu_sparse", "relu_smooth_sparse")
WGRAD_GEOM = dict(H=64, W=512, cps_direct=256, cps_wino=171, fp32_chain=9376)  # conv3_x chains: 64 / 48 / 56 splits of 4 x 256 x 512


def wgrad_inputs(cls, n, H, W, rs):
    e = rs.standard_normal((n, H, W)).astype(np.float32)
    d = rs.standard_normal((n, H, W)).astype(np.float32)
    if cls != "gauss":
        # post-ReLU activations, and a gradient that is zero on nine pixels of ten
        if cls == "relu_smooth_sparse":  # neighbouring rows nearly equal: d2 - d1 cancels, d1 + d2 does not
            base = rs.standard_normal((n, 1, W)).astype(np.float32)
            d = base + 0.1 * d
        d = np.maximum(d, 0).astype(np.float32)
        e = (e * (rs.random_sample((n, H, W)) < 0.1)).astype(np.float32)
    return e, d


def tchain(ap, bp, cps):
    """split-K slabs of the three-piece kernels with the per-step temporary (wgrad_mma_v6_pipe): ap, bp [n, chunks, 32] fp32
    operands; per chunk the six piece products (32-term sums exact, one rounding per MFMA) are summed from zero, smallest
    first, and the temporary is added to the fp32 running sum once.  Returns the fp64 sum of the fp32 slabs."""
    a3, b3 = split3(ap), split3(bp)
    prods = [(a3[i] * b3[s - i]).sum(-1) for s in (2, 1, 0) for i in range(s, -1, -1)]  # [n, chunks] each, exact
    n, chunks = prods[0].shape
    total = np.zeros(n)
    for c0 in range(0, chunks, cps):
        acc = np.zeros(n)
        for k in range(c0, min(c0 + cps, chunks)):
            tmp = np.zeros(n)
            for p in prods:
                tmp = f32(tmp + p[:, k])
            acc = f32(acc + tmp)
        total += acc
    return total


def emulate_wgrad(cls, n, seed, H=None, W=None, cps_direct=None, cps_wino=None, fp32_chain=None):
    geo = dict(WGRAD_GEOM)
    geo.update({k: v for k, v in dict(H=H, W=W, cps_direct=cps_direct, cps_wino=cps_wino, fp32_chain=fp32_chain).items() if v})
    H, W = geo["H"], geo["W"]
    assert H % 2 == 0 and W % 32 == 0
    rs = np.random.RandomState(seed)
    e, d = wgrad_inputs(cls, n, H, W, rs)
    dp = np.zeros((n, H + 2, W), np.float32)   # row y of the image is dp[:, y + 1]
    dp[:, 1:-1] = d
    e64, dp64 = e.astype(np.float64), dp.astype(np.float64)
    ref = np.stack([(e64 * dp64[:, ky:ky + H]).sum((1, 2)) for ky in range(3)], 1)

    # fp32 FMA chain over the pixels in memory order, split-K as the fp32-MFMA kernel plans it
    y32 = np.zeros((n, 3))
    for ky in range(3):
        ef, df = e64.reshape(n, -1), dp64[:, ky:ky + H].reshape(n, -1)
        for p0 in range(0, H * W, geo["fp32_chain"]):
            acc = np.zeros(n)
            for p in range(p0, min(p0 + geo["fp32_chain"], H * W)):
                acc = f32(acc + ef[:, p] * df[:, p])
            y32[:, ky] += acc
    y32 = f32(y32)

    # today's direct kernel: chunks walk rows, 32 pixels each
    ydir = f32(np.stack([tchain(e.reshape(n, -1, 32), dp[:, ky:ky + H].reshape(n, -1, 32), geo["cps_direct"])
                         for ky in range(3)], 1))

    # F(2,3) across rows: A e and B^T d in fp32 (one rounding per value), four component chains over row pairs, G^T on the
    # fp64 slab sums, one rounding to fp32
    e0, e1 = e64[:, 0::2], e64[:, 1::2]
    d0, d1, d2, d3 = (dp64[:, i:i + H:2] for i in range(4))
    comps = ((e0, d0 - d2), (e0 + e1, d1 + d2), (e0 - e1, d2 - d1), (-e1, d1 - d3))
    M = [tchain(f32(a).astype(np.float32).reshape(n, -1, 32), f32(b).astype(np.float32).reshape(n, -1, 32), geo["cps_wino"])
         for a, b in comps]
    ywin = f32(np.stack([M[0] + 0.5 * (M[1] + M[2]), 0.5 * (M[1] - M[2]), M[3] + 0.5 * (M[1] + M[2])], 1))

    scale = np.abs(ref).max()
    res = {}
    for name, y in (("fp32", y32), ("direct", ydir), ("wino", ywin)):
        err = np.abs(y - ref) / scale
        res[name] = (float(np.sqrt((err ** 2).mean())), float(err.max()))
    return res


def wgrad_table(samples, seed, classes=WGRAD_CLASSES, **geo):
    lines = []
    for cls in classes:
        i = WGRAD_CLASSES.index(cls)
        r = emulate_wgrad(cls, samples, seed + i, **geo)
        lines.append("%-19s rms fp32 %.3e direct %.3e wino %.3e | max fp32 %.3e direct %.3e wino %.3e | wino/fp32 rms %.3f max %.3f"
                     % (cls, r["fp32"][0], r["direct"][0], r["wino"][0], r["fp32"][1], r["direct"][1], r["wino"][1],
                        r["wino"][0] / r["fp32"][0], r["wino"][1] / r["fp32"][1]))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--wgrad", action="store_true", help="weight gradient, F(2,3) across rows")
    a = ap.parse_args()
    if a.wgrad:
        print("# 3x3 weight gradient, distance from fp64 relative to the largest sampled element; %d samples x 3 ky, geometry %s"
              % (a.samples, WGRAD_GEOM))
        for line in wgrad_table(a.samples, a.seed):
            print(line)
        return
    for cin in CASES:
        r = emulate(cin, a.samples, a.seed + cin)
        print("Cin %4d  rms fp32 %.3e direct %.3e wino %.3e | rms ratio direct %.3f wino %.3f | worst ratio direct %.3f wino %.3f"
              % (cin, r["fp32"][0], r["direct"][0], r["wino"][0], r["direct"][0] / r["fp32"][0], r["wino"][0] / r["fp32"][0],
                 r["direct"][1] / r["fp32"][1], r["wino"][1] / r["fp32"][1]))


if __name__ == "__main__":
    main()

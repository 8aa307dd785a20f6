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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    for cin in CASES:
        r = emulate(cin, a.samples, a.seed + cin)
        print("Cin %4d  rms fp32 %.3e direct %.3e wino %.3e | rms ratio direct %.3f wino %.3f | worst ratio direct %.3f wino %.3f"
              % (cin, r["fp32"][0], r["direct"][0], r["wino"][0], r["direct"][0] / r["fp32"][0], r["wino"][0] / r["fp32"][0],
                 r["direct"][1] / r["fp32"][1], r["wino"][1] / r["fp32"][1]))


if __name__ == "__main__":
    main()

"""Oracle and shared inputs of the deformable-convolution tests (a helper module, not a conftest).

The reference has no arithmetic for DFConv2d (layers/misc.py:113-184 imports an absent package), so the oracle is the
DCNv2 definition the kernels document (include/scan_hip.h: scan_deform_sample_forward), written in differentiable torch:

  h = float(y - 1 + i) + off[m, 2k],  w = float(x - 1 + j) + off[m, 2k + 1]     one fp32 add each, then promoted
  val = 0 when h <= -1 or w <= -1 or h >= H or w >= W, otherwise bilinear on the cell floor selects, outside corners zero
  cols[m, k, c] = mask[m, k] * val[c];   y[m, o] = b[o] + sum_{k, c} W[o, c, i, j] * cols[m, k, c]

floor is detached, so autograd of this function gives the gradients the kernels implement (at integer positions: of the cell
floor selects).  ``dtype`` is torch.float64 for the oracle proper; torch.float32 evaluates the same formulas in fp32.
"""
import functools
import math

import torch

N_IMAGES = 2
SIZES = ((9, 15), (5, 7), (1, 2))  # rows per level that are no multiple of anything, and a level smaller than the kernel
CHANNELS = ((4, 8), (6, 5), (72, 40), (256, 256))  # (C, O)
FAMILIES = ("zeros", "integers", "fractional", "edges")


def row_offsets(n_images, sizes):
    off = [0]
    for h, w in sizes:
        off.append(off[-1] + n_images * h * w)
    return off


def sample(x, off, mask, n_images, sizes, dtype=torch.float64):
    """x [M, C], off [M, 18] (fp32-representable values), mask [M, 9] or None -> (cols [M, 9, C], S [M, 9, C]) with
    S = |mask| * sum_corners weight * |x|, the magnitude the sampling bound is stated in."""
    x, off = x.to(dtype), off.to(dtype)
    mask = mask.to(dtype) if mask is not None else None
    ro = row_offsets(n_images, sizes)
    cols, mags = [], []
    for l, (H, W) in enumerate(sizes):
        xl = x[ro[l]:ro[l + 1]]
        ol = off[ro[l]:ro[l + 1]].view(n_images, H, W, 18)
        ys = torch.arange(H).view(1, H, 1).expand(n_images, H, W)
        xs = torch.arange(W).view(1, 1, W).expand(n_images, H, W)
        ns = torch.arange(n_images).view(n_images, 1, 1).expand(n_images, H, W)
        lc, lm = [], []
        for k in range(9):
            i, j = divmod(k, 3)
            pos = []
            for base, o in (((ys - 1 + i), ol[..., 2 * k]), ((xs - 1 + j), ol[..., 2 * k + 1])):
                p32 = base.to(torch.float32) + o.detach().to(torch.float32)  # the one fp32 add
                pos.append(p32.to(dtype) + (o - o.detach()))                 # that value, derivative 1 w.r.t. the offset
            h, w = pos
            live = (h > -1) & (w > -1) & (h < H) & (w < W)
            h, w = torch.where(live, h, torch.zeros_like(h)), torch.where(live, w, torch.zeros_like(w))
            fh, fw = torch.floor(h).detach(), torch.floor(w).detach()
            lh, lw = h - fh, w - fw
            h0, w0 = fh.long(), fw.long()
            val = mag = 0
            for dh, dw, wt in ((0, 0, (1 - lh) * (1 - lw)), (0, 1, (1 - lh) * lw), (1, 0, lh * (1 - lw)), (1, 1, lh * lw)):
                hh, ww = h0 + dh, w0 + dw
                ok = live & (hh >= 0) & (hh < H) & (ww >= 0) & (ww < W)
                idx = (ns * H + hh.clamp(0, H - 1)) * W + ww.clamp(0, W - 1)
                v = xl[idx.reshape(-1)].view(n_images, H, W, -1)
                wt = torch.where(ok, wt, torch.zeros_like(wt))[..., None]
                val = val + wt * v
                mag = mag + wt.detach() * v.detach().abs()
            lc.append(val.reshape(n_images * H * W, -1))
            lm.append(mag.reshape(n_images * H * W, -1))
        cols.append(torch.stack(lc, 1))
        mags.append(torch.stack(lm, 1))
    cols, mags = torch.cat(cols, 0), torch.cat(mags, 0)
    if mask is not None:
        cols, mags = cols * mask[:, :, None], mags * mask.detach().abs()[:, :, None]
    return cols, mags


def deform_conv(x, off, mask, weight, bias, n_images, sizes, dtype=torch.float64):
    """-> y [M, O]; weight [O, C, 3, 3], bias [O] or None"""
    cols, _ = sample(x, off, mask, n_images, sizes, dtype)
    w = weight.to(dtype).permute(0, 2, 3, 1).reshape(weight.shape[0], -1)
    y = cols.reshape(cols.shape[0], -1) @ w.t()
    return y + bias.to(dtype) if bias is not None else y


def _edge_offsets(n_images, sizes, g):
    """samples exactly on -1, 0, size - 1, size, inside (-1, 0) and (size - 1, size), and at +-1e6 and +-1e30, in both
    coordinates, mixed with in-range fractional ones so that every combination of a live and a skipped coordinate occurs"""
    out = []
    for H, W in sizes:
        o = torch.zeros(n_images, H, W, 18)
        ys = torch.arange(H).view(1, H, 1).expand(n_images, H, W).float()
        xs = torch.arange(W).view(1, 1, W).expand(n_images, H, W).float()
        e = torch.arange(n_images * H * W).view(n_images, H, W)
        frac = torch.rand(n_images, H, W, 18, generator=g)
        for k in range(9):
            i, j = divmod(k, 3)
            for col, base, size, sel in ((2 * k, ys - 1 + i, H, (e * 9 + k) % 13), (2 * k + 1, xs - 1 + j, W, (e * 9 + k) * 5 % 13 + e // 13 % 2)):
                sel = sel % 13
                f = frac[..., col]
                target = [-1.0 + 0 * f, 0 * f, size - 1.0 + 0 * f, size + 0 * f, -1 + f * 0.875 + 0.0625, size - 1 + f * 0.875 + 0.0625,
                          f * (size - 1), f * (size - 1), f * (size - 1)]
                v = torch.zeros_like(f)
                for s, t in enumerate(target):
                    v = torch.where(sel == s, t - base, v)  # small exact values: base + (t - base) == t in fp32 for the exact targets
                for s, big in zip((9, 10, 11, 12), (1e6, -1e6, 1e30, -1e30)):
                    v = torch.where(sel == s, torch.full_like(f, big), v)
                o[..., col] = v
        out.append(o.reshape(-1, 18))
    return torch.cat(out, 0)


@functools.lru_cache(maxsize=None)
def case(C, O, family, with_mask):
    """the shared inputs of one parametrisation (CPU fp32 tensors; treat them as read-only):
    x [M, C] ~ N(0, 1), off [M, 18], mask [M, 9] = sigmoid(N(0, 1)) or None, weight [O, C, 3, 3] ~ N(0, 1) / sqrt(9 C), bias [O],
    gy [M, O] ~ N(0, 1) the upstream gradient"""
    import zlib
    g = torch.Generator().manual_seed(zlib.crc32(repr((C, O, family, with_mask)).encode()))
    M = row_offsets(N_IMAGES, SIZES)[-1]
    x = torch.randn(M, C, generator=g)
    if family == "zeros":
        off = torch.zeros(M, 18)
    elif family == "integers":
        off = torch.randint(-3, 4, (M, 18), generator=g).float()
    elif family == "fractional":
        off = torch.rand(M, 18, generator=g) * 5 - 2.5
    elif family == "edges":
        off = _edge_offsets(N_IMAGES, SIZES, g)
    else:
        raise ValueError(family)
    mask = torch.sigmoid(torch.randn(M, 9, generator=g)) if with_mask else None
    weight = torch.randn(O, C, 3, 3, generator=g) / math.sqrt(9 * C)
    bias = torch.randn(O, generator=g)
    gy = torch.randn(M, O, generator=g)
    return x, off, mask, weight, bias, gy


@functools.lru_cache(maxsize=None)
def reference(C, O, family, with_mask, dtype=torch.float64):
    """y and every gradient of sum(y * gy) for case(...), computed once: dict of detached tensors in ``dtype``"""
    x, off, mask, weight, bias, gy = case(C, O, family, with_mask)
    leaves = [t.to(dtype).requires_grad_(True) if t is not None else None for t in (x, off, mask, weight, bias)]
    y = deform_conv(*leaves, N_IMAGES, SIZES, dtype)
    (y * gy.to(dtype)).sum().backward()
    out = {"y": y.detach()}
    for name, t in zip(("dx", "doff", "dmask", "dw", "db"), leaves):
        out[name] = t.grad if t is not None else None
    return out


def bar(mode):
    """the bars of tests/test_gpu_kernels.py::test_conv2d_fwd_bwd: rtol 1e-4, atol = tol * max(1, max |ref|)"""
    return 1e-4 if mode == "bf16x3" else 2e-5


def assert_within(got, ref, tol, what):
    """|got - ref| <= tol * max(1, max |ref|) + 1e-4 * |ref| on every element; prints the figure before it asserts"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "%s: not finite" % what
    atol = tol * max(1.0, float(ref.abs().max()))
    excess = ((got - ref).abs() - 1e-4 * ref.abs()) / atol
    worst = float(excess.max()) if excess.numel() else 0.0
    print("%s: worst (|err| - rtol |ref|) / atol = %.3g (atol %.3g)" % (what, worst, atol))
    assert worst <= 1.0, "%s: %.3g x the bar" % (what, worst)

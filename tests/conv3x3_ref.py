"""Oracle and bound helpers of the 3x3 convolution tests (a helper module, not a conftest): numpy only, nothing here imports
scan_amd.  tests/test_conv3x3_host.py pins it on the CPU against F.conv2d(..., padding=1) in float64;
tests/test_gpu_conv3x3_parity.py holds the 3x3 forward and data-gradient kernels (csrc/conv_fwd.hip, conv_gen1.hip, conv_mfma.hip
through csrc/conv_api.hip) to it.  Shape, the comparators and the integer data are tests/conv1x1_ref.py's.

The operation, on pyramid rows.  ``shape`` is anything with n_images, sizes and row_off; row (level l, image i, y, x) =
row_off[l] + (i H_l + y) W_l + x.  With w [O, C, 3, 3], b [O] or None, stride s (1 or 2), pad 1:

    y[(l, i, y, x)] = sum over (ky, kx, c) of x_rows[(l, i, s y + ky - 1, s x + kx - 1), c] w[o, c, ky, kx] + b[o]

where a source pixel outside [0, H_l) x [0, W_l) is the ZERO row -- at every border of every level and image, although the rows
of the neighbouring image or level are adjacent in memory -- then the optional ReLU, then the optional deferred-ReLU mask (y = 0
where mask <= 0).  It is written as nine shifted gathers (``tap_rows``) and one matmul per tap, no pixel loop.  The data gradient
of a stride-1 conv is the same operation on dY with the flipped and transposed weight (``dgrad_weight``); ``dgrad`` is the general
transpose (scatter) for stride 2.  Every function computes in the dtype it is given: float64 for the error tests, int64 for the
exact probes (integer inputs; products are taken in float64 after a check that they fit 2^53, as conv1x1_ref._matmul does).

The pointwise bound |result - float64 result| <= B S, ``bound_factor(mode, cin, family)`` and the two sums S.

family "direct" (conv_split_kernel without WINO, conv_gen1.hip, the fp32-MFMA kernels of conv_mfma.hip).  S = ``forward_abs`` =
sum |x| |w| + |b|, the sum of the absolute values of every term of the element.  As in conv1x1_ref: an element is a sum of
``terms`` numbers that are each exact in fp32 (a product of two bf16 pieces; the bias) -- or, in fp32 mode, fp32 products an fma
never rounds on their own; any summation order takes terms - 1 additions, each loses at most one ulp (2^-23) of its partial sum,
every partial sum is at most S (1 + 2^-23)^terms: B = gamma(terms) = terms 2^-23 / (1 - terms 2^-23), plus what the arithmetic
drops.  With K32 = 9 * round32(Cin) (nine taps, K chunks of 32 channels; Cin is the dY channel count for a data gradient):
    fp32      terms = K32 + 1
    bf16x6    terms = 6 K32 + 1,  + 3 * 2^-23 for the three dropped piece products (include/scan_hip.h's figure)
    bf16x3    terms = 3 K32 + 1,  + 2^-15 for what two pieces drop

family "wino" (three pieces, conv_split_kernel<..., WINO>: 1-D Winograd F(2,3) along x).  The kernel's arithmetic, read from
csrc/conv_fwd.hip (store_a, wino_mma, the epilogue) and csrc/conv_split.h (wino_g): output columns come in pairs (x0, x0 + 1), x0
even in level coordinates (tiles start at multiples of 16); with d_k = x_rows[(l, i, y + ky - 1, x0 - 1 + k)], k = 0..3, and
(g0, g1, g2) = w[o, c, ky, 0..2]:
    V0 = d0 - d2,  V1 = d1 + d2,  V2 = d2 - d1,  V3 = d1 - d3            one fp32 subtraction or addition each (store_a)
    U0 = g0,  U1 = (g0 + g1 + g2) / 2,  U2 = (g0 - g1 + g2) / 2,  U3 = g2  in fp64, rounded once to fp32 (wino_g)
    m_j = sum over (c, ky) of U_j V_j                                     six piece products per product, fp32 accumulators
    y(x0) = m0 + (m1 + m2) + b,   y(x0 + 1) = (m1 - m2) - m3 + b          (exactly the conv in real arithmetic)
So an element is again a sum of exact fp32 numbers, the piece products of three of the four m_j and the bias:
3 accumulators x 3 ky x round32(Cin) x 6 = 6 K32 of them, terms = 6 K32 + 1 -- the count of the direct kernel -- but the numbers
are other numbers, and S must be the sum of THEIR absolute values.  Errors, each relative to Ubar_j |V_j| where
Ubar_0 = |g0|, Ubar_1 = Ubar_2 = (|g0| + |g1| + |g2|) / 2, Ubar_3 = |g2| (>= |U_j|: the fp64 sum behind U_j errs by 2^-52 of
the sum of ITS absolute terms, which is why the bound is taken on Ubar and not on |U_j|):
    U_j rounded to fp32            <= 2^-23 Ubar_j        (half an ulp and the fp64 error; one ulp is allowed)
    V_j one fp32 addition          <= 2^-23 |V_j|         (relative to the result: fl(a - b) = (a - b)(1 + delta))
    dropped piece products         <= 3 * 2^-23
    summation, terms - 1 additions <= gamma(terms)
and second-order products of these are covered by a factor (1 + 2^-20):
    S_w(x0)     = sum over (c, ky) of Ubar_0 |V0| + Ubar_1 |V1| + Ubar_2 |V2|  + |b|      (``forward_abs_wino``)
    S_w(x0 + 1) = sum over (c, ky) of Ubar_1 |V1| + Ubar_2 |V2| + Ubar_3 |V3|  + |b|
    B_w = (gamma(6 K32 + 1) + 5 * 2^-23) (1 + 2^-20)
Nothing in it is measured.  S_w is not S: |V1| <= |d1| + |d2| pairs every weight of the row with both middle pixels, so S_w can
be larger than S (about 2 S on Gaussian data) and the Winograd instance is allowed that much more than the direct kernel; the
tests print both ratios.

On integer data in [-8, 8] the Winograd instance is exact as well: V_j are integers of magnitude <= 16, U_j multiples of 1/2 of
magnitude <= 12, both one bf16 piece; |m_j| <= 12 * 16 * 3 Cin = 576 Cin, in units of 1/2 below 2^24 up to Cin = 14,563, and
the three-term output transform stays in the same range.
"""
import numpy as np

from conv1x1_ref import F64, I64, U, _matmul, first_mismatch, int_inputs, round32, worst_ratio  # noqa: F401  (re-exported)
from conv1x1_ref import Shape as _Shape


class Shape(_Shape):
    """scan_amd.ops.PyramidShape without the library; conv_out for the 3x3 / pad-1 conv"""

    def conv_out(self, ksize, stride):
        assert ksize == 3
        return Shape(self.n_images, [((h - 1) // stride + 1, (w - 1) // stride + 1) for h, w in self.sizes])

    def level(self, l):
        return Shape(self.n_images, [self.sizes[l]])


def out_sizes(shape, stride):
    return [((h - 1) // stride + 1, (w - 1) // stride + 1) for h, w in shape.sizes]


def out_offsets(shape, stride):
    off = [0]
    for h, w in out_sizes(shape, stride):
        off.append(off[-1] + shape.n_images * h * w)
    return off


def shifted_rows(shape, dy, dx, stride=1):
    """int64 [output rows]: the row of ``shape`` that output pixel (l, i, y, x) reads at (stride y + dy, stride x + dx), -1 (the zero
    row) where that lies outside the level's image.  dx may be a function of the array of x coordinates (pair_pixels)."""
    off = out_offsets(shape, stride)
    out = np.full((off[-1],), -1, dtype=I64)
    for l, ((h, w), (ho, wo)) in enumerate(zip(shape.sizes, out_sizes(shape, stride))):
        i, y, x = np.meshgrid(np.arange(shape.n_images), np.arange(ho), np.arange(wo), indexing="ij")
        sy, sx = stride * y + dy, stride * x + (dx if np.isscalar(dx) else np.asarray(dx(x)))
        ok = (sy >= 0) & (sy < h) & (sx >= 0) & (sx < w)
        out[off[l]:off[l + 1]] = np.where(ok, shape.row_off[l] + (i * h + sy) * w + sx, -1).reshape(-1)
    return out


def tap_rows(shape, stride=1):
    """int64 [output rows, 9]: column ky * 3 + kx = the source row of that tap, -1 for the zero row"""
    return np.stack([shifted_rows(shape, ky - 1, kx - 1, stride) for ky in range(3) for kx in range(3)], 1)


def take(x, idx):
    """x[idx] with the zero row where idx < 0, in x's dtype"""
    g = x[np.maximum(idx, 0)]
    g[idx < 0] = 0
    return g


def forward(x, w, b, shape, stride=1, relu=False, mask=None, dtype=F64, idx=None):
    """y [output rows, O] in ``dtype`` (float64 or int64): x [shape.rows, C], w [O, C, 3, 3], b [O] or None, mask [output rows, O]
    or None.  idx: tap_rows(shape, stride) (tests/test_conv3x3_host.py passes corrupted ones)"""
    x, w = np.asarray(x), np.asarray(w)
    assert x.shape[0] == shape.rows and w.shape[1:] == (x.shape[1], 3, 3), (x.shape, w.shape, shape.rows)
    idx = tap_rows(shape, stride) if idx is None else idx
    y = np.zeros((idx.shape[0], w.shape[0]), dtype=dtype)
    for t in range(9):
        y += _matmul(take(x, idx[:, t]), w[:, :, t // 3, t % 3].T, dtype)
    if b is not None:
        y = y + np.asarray(b).astype(dtype)
    if relu:
        y = np.maximum(y, 0)
    if mask is not None:
        y = np.where(np.asarray(mask) > 0, y, 0)
    return y


def dgrad_weight(w):
    """[C, O, 3, 3]: the weight whose stride-1 forward on dY is the data gradient (flip both kernel axes, swap the channel axes)"""
    return np.ascontiguousarray(np.asarray(w)[:, :, ::-1, ::-1].transpose(1, 0, 2, 3))


def dgrad(dy, w, shape, stride=1, mask=None, dtype=F64):
    """dx [shape.rows, C]: the transpose of forward(., w, None, shape, stride) applied to dy [output rows, O] -- every tap's
    contribution scattered back to its source row (a tap's source rows are distinct, so a fancy-index add is exact).  At stride 1
    it equals forward(dy, dgrad_weight(w), None, shape), which tests/test_conv3x3_host.py checks."""
    dy, w = np.asarray(dy), np.asarray(w)
    idx = tap_rows(shape, stride)
    dx = np.zeros((shape.rows, w.shape[1]), dtype=dtype)
    for t in range(9):
        src = idx[:, t]
        live = src >= 0
        dx[src[live]] += _matmul(dy[live], w[:, :, t // 3, t % 3], dtype)
    if mask is not None:
        dx = np.where(np.asarray(mask) > 0, dx, 0)
    return dx


def forward_abs(x, w, b, shape, stride=1):
    """S [output rows, O] = sum |x| |w| + |b|, float64"""
    return forward(np.abs(np.asarray(x).astype(F64)), np.abs(np.asarray(w).astype(F64)), None if b is None else np.abs(np.asarray(b).astype(F64)),
                   shape, stride)


def wino_abs(d, odd, w, b):
    """S_w of the module docstring from the pixels themselves: d[ky][k] [R, C] = the pixel at (y + ky - 1, x0 - 1 + k) of every
    output element's pair (zero outside the image), odd [R] = the element is the pair's second column; float64 [R, O]"""
    w = np.abs(np.asarray(w).astype(F64))
    odd = np.asarray(odd).astype(bool)[:, None]
    s = 0.0
    for ky in range(3):
        dk = [np.asarray(t).astype(F64) for t in d[ky]]
        v = [np.abs(dk[0] - dk[2]), np.abs(dk[1] + dk[2]), np.abs(dk[2] - dk[1]), np.abs(dk[1] - dk[3])]
        g0, g1, g2 = w[:, :, ky, 0], w[:, :, ky, 1], w[:, :, ky, 2]
        half = 0.5 * (g0 + g1 + g2)
        m = [v[j] @ u.T for j, u in enumerate((g0, half, half, g2))]
        s = s + m[1] + m[2] + np.where(odd, m[3], m[0])
    return s if b is None else s + np.abs(np.asarray(b).astype(F64))


def pair_pixels(x, shape, ky):
    """[d_0 .. d_3] of wino_abs for every row of ``shape``: column x0 - 1 + k of row y + ky - 1, x0 = x - (x & 1)"""
    return [take(x, shifted_rows(shape, ky - 1, lambda xx, k=k: k - 1 - (xx & 1))) for k in range(4)]


def x_is_odd(shape):
    return np.concatenate([np.tile(np.arange(wd) & 1, shape.n_images * h) for h, wd in shape.sizes]).astype(bool)


def forward_abs_wino(x, w, b, shape):
    """S_w [rows, O] of the module docstring: the sum of Ubar_j |V_j| over the three Winograd components an output column uses
    (0, 1, 2 on even x, 1, 2, 3 on odd x), channels and ky, + |b|; float64"""
    x = np.asarray(x).astype(F64)
    return wino_abs([pair_pixels(x, shape, ky) for ky in range(3)], x_is_odd(shape), w, b)


def wgrad(x, dy, shape, stride=1, dtype=F64):
    """(dw [O, C, 3, 3], db [O]) in ``dtype``: dw[o, c, ky, kx] = sum over output rows of dy[r, o] x[tap row, c]"""
    x, dy = np.asarray(x), np.asarray(dy)
    idx = tap_rows(shape, stride)
    dw = np.stack([_matmul(dy.T, take(x, idx[:, t]), dtype) for t in range(9)], -1).reshape(dy.shape[1], x.shape[1], 3, 3)
    return dw, dy.astype(dtype).sum(0)


def pool2(y, shape):
    """2x2 / stride-2 max over an even-sized single level: [n H/2 W/2, C] in y's dtype"""
    assert shape.n_levels == 1 and shape.sizes[0][0] % 2 == 0 and shape.sizes[0][1] % 2 == 0
    (h, w), n = shape.sizes[0], shape.n_images
    return np.asarray(y).reshape(n, h // 2, 2, w // 2, 2, -1).max(axis=(2, 4)).reshape(n * (h // 2) * (w // 2), -1)


def gn_sums(y, shape):
    """[n_levels * n_images * C / 8, 2] in y's dtype: sum and sum of squares of y per (level, image, group of 8 channels), in the
    order of the workspace of scan_conv3x3_gn_* ((level * n_images + image) * 32 + group) * 2 for C = 256"""
    y = np.asarray(y)
    out = []
    for l, (h, w) in enumerate(shape.sizes):
        blk = y[shape.row_off[l]:shape.row_off[l + 1]].reshape(shape.n_images, h * w, y.shape[1] // 8, 8)
        out.append(np.stack([blk.sum(axis=(1, 3)), (blk * blk).sum(axis=(1, 3))], -1).reshape(-1, 2))
    return np.concatenate(out)


def bound_factor(mode, cin, family="direct"):
    """B of the module docstring for a 3x3 conv over ``cin`` input channels (the dY channels for a data gradient) in ``mode``
    ("fp32", "bf16x6", "bf16x3"); family "direct" goes with forward_abs, "wino" (bf16x6 only) with forward_abs_wino"""
    k32 = 9 * round32(cin)
    per, extra = {"fp32": (1, 0.0), "bf16x6": (6, 3 * U), "bf16x3": (3, 2.0 ** -15)}[mode]
    terms = per * k32 + 1
    assert terms * U < 0.5
    gamma = terms * U / (1.0 - terms * U)
    if family == "direct":
        return gamma + extra
    assert family == "wino" and mode == "bf16x6", (family, mode)
    return (gamma + 5 * U) * (1.0 + 2.0 ** -20)

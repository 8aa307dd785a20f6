"""Oracle, bound helpers and comparator of the 1x1 convolution tests (a helper module, not a conftest): numpy only, nothing here
imports scan_amd.  tests/test_conv1x1_host.py pins it on the CPU against F.conv2d in float64; tests/test_gpu_conv1x1_parity.py
holds the 1x1 kernels (csrc/conv_fwd.hip, conv_gen1.hip, conv_wgrad.hip, conv_mfma.hip through csrc/conv_api.hip) to it.

The operation, on pyramid rows.  ``shape`` is anything with n_images, sizes and row_off (scan_amd.ops.PyramidShape; ``Shape``
below on the CPU); row (level l, image i, y, x) = row_off[l] + (i H_l + y) W_l + x.  With w [O, C], b [O] or None:

    y[r] = src(r) w^T + b   (then the optional ReLU, then the optional deferred-ReLU mask: y = 0 where mask <= 0)

and src(r) is what scan_conv1x1_*'s ``map`` says (csrc/conv_api.hip):
    map 0   the same pyramid in and out:                     src(l, i, y, x) = x_rows[(l, i, y, x)]
    map 1   forward of a stride-2 conv, yd = ceil(xd / 2):   src(l, i, y, x) = x_rows[(l, i, 2 y, 2 x)]   (xd: the FINE pyramid)
    map 2   data gradient of a stride-2 conv, xd = ceil(yd / 2) (xd: the COARSE pyramid of dY, yd: the fine one of dX):
            src(l, i, y, x) = x_rows[(l, i, y / 2, x / 2)] where y and x are both even, the zero row elsewhere -- so without a
            bias the output is zero where a coordinate is odd.
Weight and bias gradient of a stride-s conv (s = 1, 2), x on xd, dy on yd = ceil(xd / s):
    dw[o, c] (+)= sum_r dy[r, o] x_rows[src_s(r), c],     db[o] (+)= sum_r dy[r, o]         (src_1 = map 0, src_2 = map 1)

Every function computes in the dtype it is given: float64 for the error tests, int64 for the exact probes (integer inputs).

The pointwise bound |result - float64 result| <= B S.  S is the sum of the absolute values of every term of the element
(``forward_abs`` / ``wgrad_abs``: sum |src| |w| + |b|, sum |dy| |src| (+ |dw before|), sum |dy| (+ |db before|)).  B counts
roundings, it is not measured.  An element is a sum of ``terms`` numbers that are each exact in fp32 (a product of two bf16
pieces; the bias or the value accumulated into) -- or, in fp32 mode, fp32 products that an fma never rounds on their own.  Any
order of summation, the split-K slabs of the weight gradient included, takes terms - 1 additions; each loses at most one ulp of
its partial sum, 2^-23 of it -- one ulp, not half, so an adder that truncates inside the matrix core is allowed -- and every
partial sum is at most S (1 + 2^-23)^terms.  That is the textbook gamma = terms 2^-23 / (1 - terms 2^-23) >= (1 + 2^-23)^terms - 1.
    fp32      terms = K32 + 1              (K32: the reduction length rounded up to the 32-wide K chunk, + the bias / old value)
    bf16x6    terms = 6 K32 + 1,  + 3 * 2^-23 for the three dropped piece products x1 w2, x2 w1, x2 w2: 2^-23 of the product
              each is the figure include/scan_hip.h states (pieces rounded to nearest leave |x1| <= 2^-9 |x|, |x2| <= 2^-18 |x|,
              so the three are in fact below 2^-25 |x w| together; csrc/conv_split.h)
    bf16x3    terms = 3 K32 + 1,  + 2^-15 for what two pieces drop (x = p0 + p1 + r with |r| <= 2^-18 |x|: the product loses
              p1 q1 + r w + x r' <= 3 * 2^-18 (1 + 2^-8) |x w| < 2^-16; 2^-15 is the round figure above it)
K is Cin for the forward, the dY channel count for the data gradient, the dY rows for dw and db (db: terms = rows + 1 in every
mode, a plain fp32 column sum).
"""
import numpy as np

F64, I64 = np.float64, np.int64
U = 2.0 ** -23


class Shape:
    """scan_amd.ops.PyramidShape without the library"""

    def __init__(self, n_images, sizes):
        self.n_images = int(n_images)
        self.sizes = [(int(h), int(w)) for h, w in sizes]
        self.row_off = [0]
        for h, w in self.sizes:
            self.row_off.append(self.row_off[-1] + self.n_images * h * w)

    @property
    def rows(self):
        return self.row_off[-1]

    @property
    def n_levels(self):
        return len(self.sizes)

    def conv_out(self, ksize, stride):
        assert ksize == 1
        return Shape(self.n_images, [((h - 1) // stride + 1, (w - 1) // stride + 1) for h, w in self.sizes])


def source_rows(xd, yd, cmap):
    """int64 [yd.rows]: the row of the input pyramid xd that output row r reads under ``cmap``, -1 for the zero row"""
    assert xd.n_images == yd.n_images and xd.n_levels == yd.n_levels
    out = np.full((yd.rows,), -1, dtype=I64)
    for l, ((ho, wo), (hi, wi)) in enumerate(zip(yd.sizes, xd.sizes)):
        if cmap == 0:
            assert (ho, wo) == (hi, wi)
        elif cmap == 1:
            assert (ho, wo) == ((hi - 1) // 2 + 1, (wi - 1) // 2 + 1)
        else:
            assert cmap == 2 and (hi, wi) == ((ho - 1) // 2 + 1, (wo - 1) // 2 + 1)
        i, y, x = np.meshgrid(np.arange(yd.n_images), np.arange(ho), np.arange(wo), indexing="ij")
        if cmap == 0:
            src = (i * hi + y) * wi + x
        elif cmap == 1:
            src = (i * hi + 2 * y) * wi + 2 * x
        else:
            src = np.where((y % 2 == 0) & (x % 2 == 0), (i * hi + y // 2) * wi + x // 2, -1 - xd.row_off[l])
        out[yd.row_off[l]:yd.row_off[l + 1]] = (xd.row_off[l] + src).reshape(-1)
    return out


def gather(x, xd, yd, cmap):
    """[yd.rows, C]: src(r) of every output row, in x's dtype"""
    idx = source_rows(xd, yd, cmap)
    g = x[np.maximum(idx, 0)]
    g[idx < 0] = 0
    return g


def _matmul(a, b, dtype):
    """a @ b in ``dtype``.  int64: the product is taken in float64 (BLAS; numpy's integer matmul is a plain loop) and is exact
    there -- every partial sum of the integer data is below 2^53, which is checked on max |a| max |b| K"""
    if dtype != I64:
        return a.astype(dtype) @ b.astype(dtype)
    assert np.all(a == np.rint(a)) and np.all(b == np.rint(b)), "int64 path: integer data only"
    a, b = a.astype(F64), b.astype(F64)
    assert float(np.abs(a).max(initial=0)) * float(np.abs(b).max(initial=0)) * a.shape[1] < 2.0 ** 53
    return np.rint(a @ b).astype(I64)


def forward(x, w, b, xd, yd, cmap, relu=False, mask=None, dtype=F64):
    """y [yd.rows, O] in ``dtype`` (float64 or int64): x [xd.rows, C], w [O, C], b [O] or None, mask [yd.rows, O] or None"""
    y = _matmul(gather(np.asarray(x), xd, yd, cmap), np.asarray(w).T, dtype)
    if b is not None:
        y = y + np.asarray(b).astype(dtype)
    if relu:
        y = np.maximum(y, 0)
    if mask is not None:
        y = np.where(np.asarray(mask) > 0, y, 0)
    return y


def forward_abs(x, w, b, xd, yd, cmap):
    """S [yd.rows, O] = sum_c |src| |w| + |b|, float64"""
    s = gather(np.abs(np.asarray(x).astype(F64)), xd, yd, cmap) @ np.abs(np.asarray(w).astype(F64)).T
    return s if b is None else s + np.abs(np.asarray(b).astype(F64))


def wgrad(x, dy, xd, yd, stride, dw0=None, db0=None, dtype=F64):
    """(dw [O, C], db [O]) in ``dtype``; dw0 / db0: the values accumulated into (None: a fresh result)"""
    dw = _matmul(np.asarray(dy).T, gather(np.asarray(x), xd, yd, stride - 1), dtype)
    db = np.asarray(dy).astype(dtype).sum(0)
    if dw0 is not None:
        dw = dw + np.asarray(dw0).astype(dtype)
    if db0 is not None:
        db = db + np.asarray(db0).astype(dtype)
    return dw, db


def wgrad_abs(x, dy, xd, yd, stride, dw0=None, db0=None):
    """(S_dw [O, C], S_db [O]): the sums of absolute terms behind wgrad(), float64"""
    return wgrad(np.abs(np.asarray(x).astype(F64)), np.abs(np.asarray(dy).astype(F64)), xd, yd, stride,
                 None if dw0 is None else np.abs(dw0), None if db0 is None else np.abs(db0))


def round32(k):
    return (int(k) + 31) // 32 * 32


def bound_factor(mode, k, colsum=False):
    """B of the module docstring for a reduction over k values (channels or rows) in ``mode`` ("fp32", "bf16x6", "bf16x3");
    colsum: the bias gradient, a plain fp32 sum of k values in every mode"""
    if colsum:
        terms, extra = k + 1, 0.0
    else:
        per, extra = {"fp32": (1, 0.0), "bf16x6": (6, 3 * U), "bf16x3": (3, 2.0 ** -15)}[mode]
        terms = per * round32(k) + 1
    assert terms * U < 0.5
    return terms * U / (1.0 - terms * U) + extra


def worst_ratio(got, ref, bound):
    """max over elements of |got - ref| / bound (float64); an element with bound 0 must be exact (ratio inf otherwise).
    NaN anywhere in ``got`` is inf."""
    got, ref, bound = np.asarray(got).astype(F64), np.asarray(ref).astype(F64), np.asarray(bound).astype(F64)
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    err = np.abs(got - ref)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max())


def first_mismatch(got, ref):
    """None when got == ref everywhere (exact probes), else a short description of the first differing element"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    bad = np.argwhere(~(got == ref))
    if len(bad) == 0:
        return None
    at = tuple(int(v) for v in bad[0])
    return "%d of %d elements differ, first at %s: got %r, want %r" % (len(bad), got.size, at, got[at].item(), ref[at].item())


def int_inputs(rs, *shape, lo=-8, hi=8):
    """integers in [lo, hi] as float32: each is one bf16 piece (the later pieces are zero), every product is an integer of at
    most 64 in magnitude"""
    return rs.randint(lo, hi + 1, size=shape).astype(np.float32)

"""Oracle, input cases and error bars of the GroupNorm(32) + ReLU tests (a helper module, not a conftest): numpy only, nothing
here imports scan_amd.  tests/test_groupnorm_host.py pins it on the CPU, tests/test_gpu_groupnorm_parity.py measures the kernels
of scan_amd/csrc/groupnorm.hip and the GroupNorm-sum epilogues of the 3x3 convs against it.

The operation, on pyramid rows x [M, 256] with G = 32 groups of 8 channels.  ``shape`` is anything with n_images, sizes and
row_off (scan_amd.ops.PyramidShape; ``Shape`` below on the CPU).  Per (level, image, group), over the H W x 8 elements of the slot:
    mean,  var (biased),  rstd = 1 / sqrt(var + float32(eps));     xhat = (x - mean) rstd,   y = xhat gamma + beta (+ ReLU).
Backward from dy and an explicit boolean mask (all true without the ReLU):
    g = dy mask,  a = g gamma,  S1 = mean_slot(a),  S2 = mean_slot(a xhat),  dx = rstd (a - S1 - xhat S2),
    dgamma = sum_rows g xhat,  dbeta = sum_rows g.
Everything is float64 from exactly the fp32 arrays the kernels receive; the variance is the two-pass one.

The bars.  u = 2^-24, kappa = 1 + |mean| rstd per slot, A = the largest |a| of the slot:
    statistics   |mean_k - mean| <= u |mean|,   |rstd_k / rstd - 1| <= 2 u
    tol_y      = 2 u [(|mean| rstd + 4 |xhat|) |gamma| + 2 |y before the ReLU|]     (the ReLU is 1-Lipschitz: it holds for y too)
    tol_dx     = 8 u rstd [A (1 + |xhat|)^2 + kappa (|S2| + |xhat| |S1|)]
    tol_dgamma = 32 u (sum |g| (kappa + |xhat|) + |dgamma|)
    tol_dbeta  = 32 u sum |g|                                                       (accumulate: + u |fill| on both)
They are rounding bounds of the kernels' operation order: mean and rstd are fp64 results rounded once to fp32 (rstd a second time
through the fp64 sqrt and division: 2 u); xhat = fl(fl(x - mean_k) rstd_k) carries u |mean| rstd from the mean, u |xhat| from the
subtraction, 2 u |xhat| from rstd_k, u |xhat| from the product, then one fma: u [(|mean| rstd + 4 |xhat|) |gamma| + |y|] to first
order, doubled.  dgamma / dbeta are fp32 chains of the rows one thread owns in a 256-row block before the fp64 folding over waves
and blocks; roundings of a chain do not line up, and the emulation below reaches about 1 / 32 of those two bars, 0.50 of
tol_y (all but the whole of its first-order bound: the factor 2 is the margin) and 0.38 of tol_dx.

The statistics bar needs the group sums to be exact to far below u, which is what widening every element before it is added or
squared gives for |mean| / std <= 1000 (the nominal offset / sd of the cases; the fp64 cancellation in q / cnt - mean^2 costs
the variance about (mean / std)^2 2^-53) and |x| up to the fp64 square range.  ``emulate_stats(widened=False)`` squares and
four-sums in fp32 and only then goes on in fp64 -- the spelling the kernels must not have -- and breaks the rstd bar from
mean / std = 10 on.
"""
import functools

import numpy as np

F32, F64 = np.float32, np.float64
C, G, CPG = 256, 32, 8
N = 2
EPS = 1e-5
U = 2.0 ** -24
WIDE = 264
RPB = 256        # GN_RPB: rows per block
GN_REP = 8

# (offset, sd)
CASES = {
    "friendly": (0.5, 2.0),
    "off10": (10.0, 1.0),
    "off100": (100.0, 1.0),
    "off1000": (1000.0, 1.0),
    "narrow": (30.0, 0.03),
    "small": (0.0, 1e-3),
    "negoff": (-300.0, 0.5),
    "const": (5.0, 0.0),
    "huge": (0.0, 1e20),
}
# where fp32 squares and four-sums must fail the rstd bar: the GPU statistics tests have teeth there
BROKEN_BEFORE = ("off10", "off100", "off1000", "narrow", "huge")

PYRAMIDS = {
    "one_pixel": [(1, 1)],                                     # 8 elements per group
    "ragged_three_levels": [(20, 13), (3, 5), (1, 2)],         # 260 rows = 256 + a 4-row tail; levels under 16 rows; level offsets
    "one_exact_block": [(16, 16)],
    "past_the_replicas": [(33, 32)],                           # 5 chunks per image, 10 blocks > GN_REP; the ordered chunk loop
    "five_tiny_levels": [(3, 3), (2, 3), (2, 2), (1, 2), (1, 1)],   # SCAN_MAX_LEVELS
}
ONE_PYRAMID = "ragged_three_levels"   # where the row-stride, accumulate and ws_cleared variants run


class Shape:
    """the fields of scan_amd.ops.PyramidShape the oracle reads"""

    def __init__(self, n_images, sizes):
        self.n_images, self.sizes, self.row_off = int(n_images), [(int(h), int(w)) for h, w in sizes], [0]
        for h, w in self.sizes:
            self.row_off.append(self.row_off[-1] + self.n_images * h * w)
        self.rows, self.n_levels = self.row_off[-1], len(self.sizes)


def slots(shape):
    """(il, level, image, row slice) of every (level, image), il = level * N + image: the order of the statistics table"""
    for lvl, (h, w) in enumerate(shape.sizes):
        for n in range(shape.n_images):
            r0 = shape.row_off[lvl] + n * h * w
            yield lvl * shape.n_images + n, lvl, n, slice(r0, r0 + h * w)


def blocks(shape):
    return sum(shape.n_images * ((h * w + RPB - 1) // RPB) for h, w in shape.sizes)


def expand(shape, t):
    """[IL, G] per-slot values -> [M, C] per element"""
    out = np.empty((shape.row_off[-1], C), np.asarray(t).dtype)
    for il, _, _, rows in slots(shape):
        out[rows] = np.repeat(t[il], CPG)[None, :]
    return out


# ----------------------------------------------------------------------------- inputs
def inputs(case, shape, seed=0):
    """(x [M, 256], gamma, beta, dy [M, 264], fill [2, 256]) as fp32 numpy arrays, seeded.  Every (level, image, group) has its
    own offset off (1 + g / 32) (-1)^n and its own scale sd (1 + l / 2), so a statistic taken from a neighbouring slot cannot
    pass; the larger scale on the higher levels keeps |mean| / std at or under the case's offset / sd there"""
    off, sd = CASES[case]
    rs = np.random.RandomState(1000 * sorted(CASES).index(case) + 7 * shape.row_off[-1] + seed)
    x = np.empty((shape.row_off[-1], C), F64)
    grp = np.repeat(1.0 + np.arange(G) / G, CPG)
    for _, lvl, n, rows in slots(shape):
        x[rows] = off * grp[None, :] * (-1.0) ** n + sd * (1.0 + 0.5 * lvl) * rs.standard_normal((rows.stop - rows.start, C))
    gamma = (1.0 + 0.1 * rs.standard_normal(C)).astype(F32)
    beta = (0.1 * rs.standard_normal(C)).astype(F32)
    dy = rs.standard_normal((shape.row_off[-1], WIDE)).astype(F32)
    fill = rs.standard_normal((2, C)).astype(F32)
    return x.astype(F32), gamma, beta, dy, fill


def group_sums(x, shape):
    """fp64 (sum, sum of squares) per (level, image, group), [IL, G, 2]: what a conv epilogue leaves behind"""
    x64 = np.asarray(x, F64)
    out = np.empty((shape.n_levels * shape.n_images, G, 2), F64)
    for il, _, _, rows in slots(shape):
        r = x64[rows].reshape(-1, G, CPG)
        out[il, :, 0], out[il, :, 1] = r.sum((0, 2)), (r * r).sum((0, 2))
    return out


# ----------------------------------------------------------------------------- float64 oracle
class Forward:
    """mean, var, rstd [IL, G]; xhat, ypre (before the ReLU), y [M, C]; and the per-element spreads mean_e, rstd_e"""

    def __init__(self, x, gamma, beta, shape, relu=True, eps=EPS):
        x64 = np.asarray(x, F64)
        il_n = shape.n_levels * shape.n_images
        self.shape, self.relu = shape, bool(relu)
        self.gamma, self.beta = np.asarray(gamma, F64), np.asarray(beta, F64)
        self.mean, self.var = np.empty((il_n, G), F64), np.empty((il_n, G), F64)
        for il, _, _, rows in slots(shape):
            r = x64[rows].reshape(-1, G, CPG)
            m = r.mean((0, 2))
            self.mean[il], self.var[il] = m, ((r - m[None, :, None]) ** 2).mean((0, 2))
        self.rstd = 1.0 / np.sqrt(self.var + F64(F32(eps)))
        self.mean_e, self.rstd_e = expand(shape, self.mean), expand(shape, self.rstd)
        self.xhat = (x64 - self.mean_e) * self.rstd_e
        self.ypre = self.xhat * self.gamma[None, :] + self.beta[None, :]
        self.y = np.maximum(self.ypre, 0.0) if relu else self.ypre

    def tol_mean(self):
        return U * np.abs(self.mean)

    def tol_rstd(self):
        return 2 * U * self.rstd

    def tol_y(self):
        return 2 * U * ((np.abs(self.mean_e) * self.rstd_e + 4 * np.abs(self.xhat)) * np.abs(self.gamma)[None, :] + 2 * np.abs(self.ypre))


class Backward:
    """dx [M, C], dgamma, dbeta [C] of a Forward, from dy [M, C] and a boolean mask [M, C] (None: all true)"""

    def __init__(self, fwd, dy, mask=None):
        shape = fwd.shape
        g = np.asarray(dy, F64) if mask is None else np.asarray(dy, F64) * np.asarray(mask, bool)
        a = g * fwd.gamma[None, :]
        il_n = shape.n_levels * shape.n_images
        S1, S2, A = np.empty((il_n, G), F64), np.empty((il_n, G), F64), np.empty((il_n, G), F64)
        for il, _, _, rows in slots(shape):
            ar, hr = a[rows].reshape(-1, G, CPG), fwd.xhat[rows].reshape(-1, G, CPG)
            S1[il], S2[il], A[il] = ar.mean((0, 2)), (ar * hr).mean((0, 2)), np.abs(ar).max((0, 2))
        self.fwd, self.g, self.S1, self.S2, self.A = fwd, g, S1, S2, A
        self.S1_e, self.S2_e, self.A_e = expand(shape, S1), expand(shape, S2), expand(shape, A)
        self.dx = fwd.rstd_e * (a - self.S1_e - fwd.xhat * self.S2_e)
        self.dgamma, self.dbeta = (g * fwd.xhat).sum(0), g.sum(0)

    def tol_dx(self):
        f, h = self.fwd, np.abs(self.fwd.xhat)
        kappa = 1.0 + np.abs(f.mean_e) * f.rstd_e
        return 8 * U * f.rstd_e * (self.A_e * (1.0 + h) ** 2 + kappa * (np.abs(self.S2_e) + h * np.abs(self.S1_e)))

    def tol_dgamma(self, fill=None):
        f = self.fwd
        kappa = 1.0 + np.abs(f.mean_e) * f.rstd_e
        t = 32 * U * ((np.abs(self.g) * (kappa + np.abs(f.xhat))).sum(0) + np.abs(self.dgamma))
        return t if fill is None else t + U * np.abs(np.asarray(fill, F64))

    def tol_dbeta(self, fill=None):
        t = 32 * U * np.abs(self.g).sum(0)
        return t if fill is None else t + U * np.abs(np.asarray(fill, F64))


def ratio(got, ref, tol):
    """largest |got - ref| / tol over every element; an error of 0 under a bar of 0 counts 0, a non-finite value inf"""
    got, ref, tol = np.asarray(got, F64), np.asarray(ref, F64), np.asarray(tol, F64)
    assert got.shape == ref.shape == tol.shape, (got.shape, ref.shape, tol.shape)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.divide(err, tol, out=np.zeros_like(err), where=err != 0)
    m = float(r.max()) if r.size else 0.0
    return m if np.isfinite(m) else float("inf")


def stats_ratios(table, fwd):
    """(mean, rstd) ratios of a [IL * G * 2] device table against a Forward"""
    t = np.asarray(table, F64).reshape(-1, G, 2)
    return ratio(t[..., 0], fwd.mean, fwd.tol_mean()), ratio(t[..., 1], fwd.rstd, fwd.tol_rstd())


# ----------------------------------------------------------------------------- fp32 emulation of the kernels' arithmetic
def _finalize(s, q, cnt, eps):
    """gn_stats_final_kernel: fp64 from the sums to one rounding of mean and of rstd"""
    with np.errstate(all="ignore"):
        mean = s / cnt
        var = np.maximum(q / cnt - mean * mean, 0.0)
        return mean.astype(F32), (1.0 / np.sqrt(var + F64(F32(eps)))).astype(F32)


def emulate_stats(x, shape, widened=True, eps=EPS):
    """the (mean, rstd) table [IL, G, 2] in fp32.  widened: every element enters both sums as a double.  Not widened: the four
    channels of a lane are squared and summed in fp32 first, (x0 x0 + x1 x1) + (x2 x2 + x3 x3), and only then widened"""
    x = np.asarray(x, F32)
    out = np.empty((shape.n_levels * shape.n_images, G, 2), F32)
    for il, _, _, rows in slots(shape):
        with np.errstate(all="ignore"):
            if widened:
                r = x[rows].astype(F64).reshape(-1, G, CPG)
                s, q = r.sum((0, 2)), (r * r).sum((0, 2))
            else:
                r = x[rows].reshape(-1, G, 2, 4)
                s4 = (r[..., 0] + r[..., 1]) + (r[..., 2] + r[..., 3])
                q4 = (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + (r[..., 2] * r[..., 2] + r[..., 3] * r[..., 3])
                assert s4.dtype == F32 and q4.dtype == F32
                s, q = s4.astype(F64).sum((0, 2)), q4.astype(F64).sum((0, 2))
        out[il, :, 0], out[il, :, 1] = _finalize(s, q, F64(r.shape[0] * CPG), eps)
    return out


def _fma32(a, b, c):
    """fl32(a b + c) for fp32 a, b, c: the product is exact in fp64; the fp64 sum's own rounding is 2^-29 of fp32's"""
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def emulate_forward(x, table, gamma, beta, shape, relu=True):
    """gn_affine in fp32: fma(fl(fl(x - mean) rstd), gamma, beta); returns (y, y before the ReLU)"""
    x = np.asarray(x, F32)
    mean, rstd = expand(shape, table[..., 0]), expand(shape, table[..., 1])
    h = (x - mean) * rstd
    assert h.dtype == F32
    ypre = _fma32(h, np.broadcast_to(np.asarray(gamma, F32), h.shape), np.broadcast_to(np.asarray(beta, F32), h.shape))
    return (np.maximum(ypre, F32(0)) if relu else ypre), ypre


def emulate_backward(x, dy, table, gamma, beta, shape, relu=True):
    """gn_bwd_reduce_kernel + gn_bwd_apply_kernel in fp32: (dx, dgamma, dbeta, mask).  A thread adds g xhat and g over its
    rows of a 256-row block (wave w owns rows w, w + 4, ...) in an fp32 chain; waves and blocks are folded in fp64.  The group
    sums add a lane's four products in fp32 and go on in fp64.  S1, S2 are rounded to fp32 and scaled by fl(1 / cnt)"""
    x, dy = np.asarray(x, F32), np.asarray(dy, F32)
    ga = np.broadcast_to(np.asarray(gamma, F32), x.shape)
    mean, rstd = expand(shape, table[..., 0]), expand(shape, table[..., 1])
    h = (x - mean) * rstd
    mask = _fma32(h, ga, np.broadcast_to(np.asarray(beta, F32), x.shape)) > 0 if relu else np.ones(x.shape, bool)
    gg = np.where(mask, dy, F32(0))
    a = gg * ga
    ah = a * h
    assert a.dtype == F32 and ah.dtype == F32
    dgam, dbet = np.zeros(C, F64), np.zeros(C, F64)
    il_n = shape.n_levels * shape.n_images
    S1, S2 = np.empty((il_n, G), F32), np.empty((il_n, G), F32)
    for il, _, _, rows in slots(shape):
        hw = rows.stop - rows.start
        for b0 in range(rows.start, rows.stop, RPB):
            for w in range(4):
                dg, db = np.zeros(C, F32), np.zeros(C, F32)
                for r in range(b0 + w, min(b0 + RPB, rows.stop), 4):
                    dg = dg + gg[r] * h[r]
                    db = db + gg[r]
                dgam += dg.astype(F64)
                dbet += db.astype(F64)
        a4, ah4 = a[rows].reshape(-1, G, 2, 4), ah[rows].reshape(-1, G, 2, 4)
        s1 = ((a4[..., 0] + a4[..., 1]) + (a4[..., 2] + a4[..., 3])).astype(F64).sum((0, 2))
        s2 = ((ah4[..., 0] + ah4[..., 1]) + (ah4[..., 2] + ah4[..., 3])).astype(F64).sum((0, 2))
        inv_cnt = F32(1.0) / F32(hw * CPG)
        S1[il], S2[il] = s1.astype(F32) * inv_cnt, s2.astype(F32) * inv_cnt
    S1e, S2e = expand(shape, S1), expand(shape, S2)
    dx = rstd * (a - (S1e + h * S2e))
    assert dx.dtype == F32
    return dx, dgam.astype(F32), dbet.astype(F32), mask


# ----------------------------------------------------------------------------- shared, read-only cases
class Case:
    """inputs of (case, pyramid) and their float64 forward, ReLU on and off; never written after construction"""

    def __init__(self, case, pyramid, shape=None):
        self.case, self.pyramid = case, pyramid
        self.shape = shape if shape is not None else Shape(N, PYRAMIDS[pyramid])
        self.x, self.gamma, self.beta, self.dy_wide, self.fill = inputs(case, self.shape)
        self.dy = np.ascontiguousarray(self.dy_wide[:, :C])
        self.sums = group_sums(self.x, self.shape)
        self.fwd = {r: Forward(self.x, self.gamma, self.beta, self.shape, relu=bool(r)) for r in (0, 1)}
        for a in (self.x, self.gamma, self.beta, self.dy_wide, self.dy, self.fill, self.sums):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def case(name, pyramid):
    return Case(name, pyramid)

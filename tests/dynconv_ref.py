"""Oracle, input families and error bars of the dynamic conv + softmax tests (a helper module, not a conftest): numpy and
torch-CPU only, nothing here imports scan_amd._lib.  tests/test_dynconv_host.py pins it on the CPU, tests/test_gpu_dynconv.py
measures the kernels of scan_amd/csrc/dynconv.hip against it.

The operation.  feat [M, 256] x kernels [K, 256]^T -> logits z [M, K]; p = softmax(z, 1).  Backward, from the gradients dl
(at the logits) and dp (at the probabilities), either of which may be absent:
    dot_m = sum_j p_mj dp_mj,   dz = dl + p (dp - dot),   d_feat = dz @ kernels,   d_kernels = dz^T @ feat.
``forward`` / ``backward`` evaluate this in float64 from exactly the fp32 arrays the kernels receive -- the backward from the
fp32-rounded reference probabilities, which is what the GPU test hands to scan_dynconv_softmax_backward, so both sides start from
identical inputs.

Tier A: worst-case bars, u = 2^-24 (fp32 round to nearest), every element, nothing excluded.  The counts are roundings read off
dynconv.hip, to first order in u:
  logits     |err| <= 320 u S,  S_mk = sum_c |f_mc| |k_kc|.  A 256-term dot product accumulated in any order, fused or not, puts
             at most 256 roundings on a term (its product, then at most 255 additions): 256 u S.  The 64 chained
             v_mfma_f32_16x16x4_f32 of a tile may each add their four products before they meet the accumulator: one more
             rounding per MFMA boundary, 64.
  probs      |err| <= p (4 Bz + (K + 8) 2^-23),  Bz = the largest logit bar of the row.  p_k = 1 / sum_j exp(z_j - z_k): logits
             off by Bz each move an exponent by 2 Bz, p by the factor exp(2 Bz); the rounding of z - mx is at most
             u |z - mx| <= 2 u max S, far inside the second 2 Bz.  Then expf (1 ulp = 2 u) on the numerator and on the
             denominator, at most 5 additions on the way through the denominator (one per class tile, four xor-shuffles; a
             sequential sum of K terms: K - 1), one division: (2 + 2 + 5 + 1) u = 5 2^-23 <= (K + 8) 2^-23.  Where the float64
             p is below 2^-126 the fp32 result is subnormal or zero and has no relative accuracy: there 0 <= got <= 2^-126.
  dz         |err| <= (K + 8) u Dz,  Dz = |dl| + p (|dp| + sum_j p_j |dp_j|).  The products p dp (1), the shuffle tree of dot
             (<= 5; a sequential chain: K - 1), dp - dot (1), p (..) (1), + dl (1): at most 9 <= K + 8 on any term in the
             kernels, K + 3 in a sequential chain.
  d_feat     |err| <= (2 K + 10) u sum_k Dz_mk |w_kc|: the K + 8 of dz, K multiply-adds of the chain over the classes (the
             zero rows K..KP-1 of the generic kernel add exact zeros), 2 spare.
  d_kernels  |err| <= (K + 8 + L) u sum_m Dz_mk |f_mc|,  L = the longest fp32 addition chain an element passes through
             (``dker_chain_length``): the rows a lane accumulates, the 4 wave partials of a workgroup in the <K> instances, the
             dc_bwd_blocks(M) workgroup partials in dynconv_reduce_kernel.  A sum of M terms in ANY order has L <= M, which is
             the L the host test grants torch and the sequential spelling.

Tier B: drift.  ``fp32_chain_*`` spell the same formulas as naive sequential fp32 loops with one rounding per operation (logits: a
256-step chain over the channels; d_kernels: one chain over all rows in order).  ``yardstick`` is the largest error of that
spelling against the float64 reference in units of u x the tier-A scale (probs: as a fraction of the tier-A bar, which has two
terms); a kernel must stay within TIER_B_MARGIN = 4 times it on the same inputs.  Two summation orders move the maximum of a
rounding random walk over up to 4e6 elements by small factors; a lost operand moves it by about 1e4 units.
"""
import functools

import numpy as np
import torch

F32, F64 = np.float32, np.float64
C = 256
U = 2.0 ** -24
TINY = 2.0 ** -126          # smallest normal fp32
TIER_B_MARGIN = 4.0

EXTREMES = ("offset_hi", "offset_lo", "gap", "ties")
FAMILIES = ("standard",) + EXTREMES

# (K, scan_tune "dynconv_generic"): the <K> instances; the same K on the generic kernels; one class tile (5, 16); two tiles (17),
# the last exact 8-row chunk of the generic backward (24), its 6-row chunk with padded classes (25, 31) and without (32)
DISPATCH = ((9, 0), (2, 0), (9, 1), (2, 1), (5, 0), (16, 0), (17, 0), (24, 0), (25, 0), (31, 0), (32, 0))
# 8192 full 16-row groups = one trip of the forward's 2048 x 4 waves, one more full group and a 1-row tail: the smallest M whose
# second trip and ragged tail land on different waves; the backward is past its 512 workgroups too
CAP_M, CAP_DISPATCH = 131089, ((9, 0), (2, 0), (5, 0), (17, 0))
EDGE_MS = (3, 4, 5, 6, 7, 8, 9, 12, 13, 63, 64, 65)   # around the row chunks of 4 (<K>), 6 and 8 (generic) and the 16-row group
EXTREME_M, EXTREME_DISPATCH = 37, ((9, 0), (2, 0), (5, 0), (17, 0), (31, 0))
BRANCH_M, BRANCH_DISPATCH = 65, ((9, 0), (2, 0), (9, 1), (2, 1), (5, 0), (25, 0))
BRANCHES = ((True, False), (False, True), (True, True), (False, False))   # (dl given, dp given)


# ----------------------------------------------------------------------------- inputs
def coefficients(family, K):
    """c_k of the extreme families (kernels_k = c_k u, float64 here)"""
    k = np.arange(K, dtype=F64)
    if family == "offset_hi":    # s = 16: logits 80 .. 86, exp(86) = 2e37 is a factor 15 below the largest fp32
        return 5.375 - 0.375 * k / (K - 1)
    if family == "offset_lo":    # s = 1: -60 .. -62.5, s = 16: -960 .. -1000
        return -60.0 - 2.5 * k / (K - 1)
    if family == "gap":          # the last real class leads by 10 s, up to 160; the others within +-0.3 s
        c = -0.3 + 0.6 * k / max(K - 2, 1)
        c[K - 1] = 10.0
        return c
    if family == "ties":         # three values in turn; the last real class takes the value of the first
        c = np.array([1.0, -0.5, 0.25])[np.arange(K) % 3]
        c[K - 1] = c[0]
        return c
    raise ValueError(family)


def tie_groups(K):
    """the classes of the ``ties`` family whose kernel rows are bit-identical, groups of two or more"""
    c = coefficients("ties", K)
    groups = [np.flatnonzero(c == v).tolist() for v in np.unique(c)]
    return [g for g in groups if len(g) > 1]


def inputs(family, M, K):
    """(feat [M, 256], kernels [K, 256], dl [M, K], dp [M, K]) as fp32 numpy arrays, seeded.  ``standard`` is the construction
    of test_dynconv_softmax (tests/test_gpu_kernels.py).  The extreme families: feat_m = s_m u + 0.01 noise, kernels_k = c_k u
    with u a unit vector and s_m = 1 + m % 16, so z_mk = c_k (s_m + 0.01 noise . u) is under control."""
    if family == "standard":
        g = torch.Generator().manual_seed(M)
        feat = torch.randn(M, C, generator=g)
        ker = torch.randn(K, C, generator=g) / 16
        g1, g2 = torch.randn(M, K, generator=g), torch.randn(M, K, generator=g)
        return feat.numpy(), ker.numpy(), g1.numpy(), g2.numpy()
    g = torch.Generator().manual_seed(100003 * (1 + EXTREMES.index(family)) + 1009 * K + M)
    u = torch.randn(C, generator=g, dtype=torch.float64).numpy()
    u = (u / np.sqrt((u * u).sum())).astype(F32)
    s = (1 + np.arange(M) % 16).astype(F32)
    noise = torch.randn(M, C, generator=g).numpy()
    feat = (s[:, None] * u[None, :] + F32(0.01) * noise).astype(F32)
    ker = (coefficients(family, K).astype(F32)[:, None] * u[None, :]).astype(F32)
    dl, dp = torch.randn(M, K, generator=g).numpy(), torch.randn(M, K, generator=g).numpy()
    return feat, ker, dl, dp


# ----------------------------------------------------------------------------- float64 oracle
def _row_blocks(M, n=8192):
    """feat goes to float64 a block of rows at a time (a whole copy at M = 131089 is 268 MB)"""
    return [slice(m, min(m + n, M)) for m in range(0, M, n)]


def forward(feat, ker):
    """(z, p, S) in float64: logits, softmax, S_mk = sum_c |f_mc| |k_kc|"""
    k = np.asarray(ker, F64)
    z, S = np.empty((len(feat), len(k)), F64), np.empty((len(feat), len(k)), F64)
    for rows in _row_blocks(len(feat)):
        f = np.asarray(feat[rows], F64)
        z[rows], S[rows] = f @ k.T, np.abs(f) @ np.abs(k).T
    e = np.exp(z - z.max(1, keepdims=True))
    return z, e / e.sum(1, keepdims=True), S


def backward(feat, ker, probs32, dl, dp):
    """float64 from the fp32 arrays the kernel receives; dl / dp may be None.  Returns a dict: dz, d_feat, d_ker and the scales
    Dz = |dl| + p (|dp| + sum_j p_j |dp_j|), Sf = Dz @ |ker|, Sk = Dz^T @ |feat|"""
    k, p = np.asarray(ker, F64), np.asarray(probs32, F64)
    zero = np.zeros(p.shape, F64)
    a = zero if dl is None else np.asarray(dl, F64)
    if dp is None:
        dz, Dz = a.copy(), np.abs(a)
    else:
        b = np.asarray(dp, F64)
        dz = a + p * (b - (p * b).sum(1, keepdims=True))
        Dz = np.abs(a) + p * (np.abs(b) + (p * np.abs(b)).sum(1, keepdims=True))
    d_ker, Sk = np.zeros(k.shape, F64), np.zeros(k.shape, F64)
    for rows in _row_blocks(len(feat)):
        f = np.asarray(feat[rows], F64)
        d_ker += dz[rows].T @ f
        Sk += Dz[rows].T @ np.abs(f)
    return {"dz": dz, "d_feat": dz @ k, "d_ker": d_ker, "Dz": Dz, "Sf": Dz @ np.abs(k), "Sk": Sk}


# ----------------------------------------------------------------------------- naive sequential fp32 spellings
def fp32_chain_logits(feat, ker):
    """acc <- acc + f_c k_c for c = 0 .. 255: a product and an addition, each rounded to fp32"""
    ft, kt = np.ascontiguousarray(np.asarray(feat, F32).T), np.ascontiguousarray(np.asarray(ker, F32).T)
    acc = np.zeros((ft.shape[1], kt.shape[1]), F32)
    tmp = np.empty_like(acc)
    for c in range(C):
        np.multiply(ft[c][:, None], kt[c][None, :], out=tmp)
        np.add(acc, tmp, out=acc)
    return acc


def fp32_chain_probs(z32):
    """max-subtracted softmax with a sequential denominator"""
    z32 = np.asarray(z32, F32)
    e = np.exp(z32 - z32.max(1, keepdims=True))
    den = e[:, 0].copy()
    for k in range(1, e.shape[1]):
        den = den + e[:, k]
    return e / den[:, None]


def fp32_naive_probs(z32):
    """exp(z) / sum exp(z) without the max subtraction: what the extreme families are built to break"""
    with np.errstate(all="ignore"):
        e = np.exp(np.asarray(z32, F32))
        return e / e.sum(1, dtype=F32, keepdims=True)


def fp32_chain_dz(probs32, dl, dp):
    p = np.asarray(probs32, F32)
    if dp is None:
        return np.zeros(p.shape, F32) if dl is None else np.array(dl, F32)
    dp = np.asarray(dp, F32)
    dot = p[:, 0] * dp[:, 0]
    for k in range(1, p.shape[1]):
        dot = dot + p[:, k] * dp[:, k]
    dz = p * (dp - dot[:, None])
    return dz if dl is None else np.asarray(dl, F32) + dz


def fp32_chain_dfeat(dz32, ker):
    dz32, ker = np.asarray(dz32, F32), np.asarray(ker, F32)
    o = np.zeros((dz32.shape[0], C), F32)
    tmp = np.empty_like(o)
    for k in range(ker.shape[0]):
        np.multiply(dz32[:, k:k + 1], ker[k][None, :], out=tmp)
        np.add(o, tmp, out=o)
    return o


def fp32_chain_dker(dz32, feat):
    """one chain over all rows in order: acc <- acc + dz_m (x) f_m, the product and the addition each rounded to fp32"""
    dz32, feat = np.asarray(dz32, F32), np.asarray(feat, F32)
    acc = np.zeros((dz32.shape[1], C), F32)
    tmp = np.empty_like(acc)
    for m in range(feat.shape[0]):
        np.multiply(dz32[m][:, None], feat[m][None, :], out=tmp)
        np.add(acc, tmp, out=acc)
    return acc


def torch_fp32(feat, ker, probs32, dl, dp):
    """the same formulas as torch-CPU fp32 operators (matmul, softmax): (z, p, d_feat, d_ker)"""
    f, k, p = torch.from_numpy(np.asarray(feat, F32)), torch.from_numpy(np.asarray(ker, F32)), torch.from_numpy(np.asarray(probs32, F32))
    z = f @ k.t()
    dz = torch.zeros_like(p) if dl is None else torch.from_numpy(np.asarray(dl, F32)).clone()
    if dp is not None:
        b = torch.from_numpy(np.asarray(dp, F32))
        dz = dz + p * (b - (p * b).sum(1, keepdim=True))
    return z.numpy(), z.softmax(1).numpy(), (dz @ k).numpy(), (dz.t() @ f).numpy()


# ----------------------------------------------------------------------------- the launch arithmetic of dynconv.hip
def bwd_blocks(M):
    """dc_bwd_blocks: workgroups of the backward = partials dynconv_reduce_kernel adds"""
    return max(1, min(512, (M + 63) // 64))


def specialised(K, generic_knob=False):
    return K in (2, 9) and not generic_knob


def dker_chain_length(M, K, generic_knob=False):
    """L of the d_kernels bar.  <K> instances: a wave takes every (4 nb)-th chunk of 4 rows, then 4 wave partials, then nb
    workgroup partials.  Generic: a workgroup takes every nb-th chunk of 8 rows (6 from K = 25), then nb partials."""
    nb = bwd_blocks(M)
    if specialised(K, generic_knob):
        chunks = (M + 3) // 4
        return 4 * ((chunks + 4 * nb - 1) // (4 * nb)) + 4 + nb
    gr = 6 if K > 24 else 8
    chunks = (M + gr - 1) // gr
    return gr * ((chunks + nb - 1) // nb) + nb


# ----------------------------------------------------------------------------- bars
def bound_logits(S):
    return 320 * U * S


def bound_probs(p, S, K):
    return p * (4 * bound_logits(S).max(1, keepdims=True) + (K + 8) * 2 * U)


def _ratio(got, ref, bound):
    """largest |got - ref| / bound; an error of 0 under a bound of 0 counts 0, a non-finite value inf"""
    assert np.shape(got) == np.shape(ref) == np.shape(bound), (np.shape(got), np.shape(ref), np.shape(bound))
    err = np.abs(np.subtract(got, ref, dtype=F64))       # NaN / inf in got stay NaN / inf down to the maximum
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.divide(err, bound, out=np.zeros_like(err), where=err != 0)
    m = float(r.max()) if r.size else 0.0
    return m if np.isfinite(m) else float("inf")


def ratio_probs(got, p, S, K):
    """as _ratio against bound_probs; where the float64 p < 2^-126 the element passes with 0 <= got <= 2^-126 instead"""
    got = np.asarray(got, F64)
    tiny = p < TINY
    ok_tiny = (got >= 0) & (got <= TINY)                 # False for NaN
    if not ok_tiny[tiny].all():
        return float("inf")
    return _ratio(np.where(tiny, p, got), p, bound_probs(p, S, K))


class Case:
    """inputs of (family, M, K), their float64 results and the tier-A ratios (largest error / bar) of any candidate"""

    def __init__(self, family, M, K, dl=True, dp=True):
        self.family, self.M, self.K = family, M, K
        self.feat, self.ker, dl_, dp_ = inputs(family, M, K)
        self.dl, self.dp = (dl_ if dl else None), (dp_ if dp else None)
        self.z, self.p, self.S = forward(self.feat, self.ker)
        self.p32 = self.p.astype(F32)
        self.bwd = backward(self.feat, self.ker, self.p32, self.dl, self.dp)

    def figures(self, z=None, p=None, dz=None, d_feat=None, d_ker=None):
        """the largest error of each candidate given, in units of u x its tier-A scale (probs: as a fraction of its bar).
        Tier A: figure <= counts(K, L)[quantity]; tier B: figure <= TIER_B_MARGIN x yardstick(...)[quantity]"""
        out = {}
        if z is not None:
            out["logits"] = _ratio(z, self.z, U * self.S)
        if p is not None:
            out["probs"] = ratio_probs(p, self.p, self.S, self.K)
        if dz is not None:
            out["dz"] = _ratio(dz, self.bwd["dz"], U * self.bwd["Dz"])
        if d_feat is not None:
            out["d_feat"] = _ratio(d_feat, self.bwd["d_feat"], U * self.bwd["Sf"])
        if d_ker is not None:
            out["d_ker"] = _ratio(d_ker, self.bwd["d_ker"], U * self.bwd["Sk"])
        return out

    def chain(self):
        """the fp32_chain_* results: (z, p, dz, d_feat, d_ker)"""
        z = fp32_chain_logits(self.feat, self.ker)
        dz = fp32_chain_dz(self.p32, self.dl, self.dp)
        return z, fp32_chain_probs(z), dz, fp32_chain_dfeat(dz, self.ker), fp32_chain_dker(dz, self.feat)


def counts(K, L):
    """the tier-A bars in the units of Case.figures (the module docstring derives them)"""
    return {"logits": 320.0, "probs": 1.0, "dz": K + 8.0, "d_feat": 2 * K + 10.0, "d_ker": K + 8.0 + L}


def over_tier_a(fig, K, L):
    """the quantities of ``fig`` that are outside tier A: empty passes"""
    bar = counts(K, L)
    return {q: (v, bar[q]) for q, v in fig.items() if not v <= bar[q]}


def over_tier_b(fig, yard):
    return {q: (v, yard[q]) for q, v in fig.items() if not v <= TIER_B_MARGIN * yard[q]}


@functools.lru_cache(maxsize=2)
def case(family, M, K, dl=True, dp=True):
    """shared, read-only; the cache is small because a case at M = 131089 holds about 1 GB of float64 references"""
    return Case(family, M, K, dl, dp)


@functools.lru_cache(maxsize=None)
def yardstick(family, M, K):
    """tier-B yardstick: the figures of the fp32_chain_* spelling against the float64 reference, measured here on the CPU and
    never against a kernel: {"logits", "probs", "dz", "d_feat", "d_ker"}"""
    c = case(family, M, K)
    return c.figures(*c.chain())

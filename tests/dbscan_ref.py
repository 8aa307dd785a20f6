"""fp64 restatement of what scan_dbscan_* (csrc/dbscan.hip) computes, and the point generators the host and GPU tests share.
Independent of scan_amd and of sklearn: numpy only.

The definition (sklearn/cluster/_dbscan_inner.pyx, restated in dbscan.hip's header): two points are neighbours when their
squared distance is <= eps^2 (a point is its own neighbour); a point is core when it has >= min_samples neighbours; points are
visited in index order and the first core point opens cluster 0, which grows through core points and takes every non-core
point next to one of its core points.  eps is rounded to fp32 and squared in double, as the library does."""
import functools

import numpy as np


def eps2_of(eps):
    return float(np.float32(eps)) ** 2


def sq_dists(pts, eps):
    """[n, n] fp64 squared distances.  The Gram form |a|^2 + |b|^2 - 2 a.b carries ~D 2^-53 (|a|^2 + |b|^2) of rounding, which
    at |p|^2 ~ 1e8 is larger than the gaps to eps^2 that have to be resolved: every pair whose Gram value lies within
    1e-9 (|a|^2 + |b|^2) + 1e-12 of eps^2 is recomputed as sum (a - b)^2 (exact differences of fp32 values, ~D 2^-53 RELATIVE)."""
    p = np.asarray(pts, dtype=np.float64)
    e2 = eps2_of(eps)
    s = (p * p).sum(1)
    ss = s[:, None] + s[None, :]
    d2 = ss - 2.0 * (p @ p.T)
    near = np.abs(d2 - e2) <= 1e-9 * ss + 1e-12
    ii, jj = np.nonzero(np.triu(near, 1))
    for c in range(0, len(ii), 16384):
        a, b = ii[c:c + 16384], jj[c:c + 16384]
        df = p[a] - p[b]
        e = (df * df).sum(1)
        d2[a, b] = e
        d2[b, a] = e
    np.fill_diagonal(d2, 0.0)
    return d2


def adjacency(pts, eps):
    """[n, n] bool, symmetric, True on the diagonal"""
    return sq_dists(pts, eps) <= eps2_of(eps)


def min_gap(pts, eps, d2=None):
    """smallest non-zero |d2 - eps^2| over all pairs i < j.  Pairs whose difference vector has a single non-zero component are
    left out: their d2 is one exact product in any summation order (the exactly-at-eps cases are made of them).  inf when no
    pair is left."""
    p = np.asarray(pts, dtype=np.float64)
    e2 = eps2_of(eps)
    n = len(p)
    iu, ju = np.triu_indices(n, 1)
    gap = np.abs((sq_dists(pts, eps) if d2 is None else d2)[iu, ju] - e2)
    k = min(2048, len(gap))
    if k == 0:
        return np.inf
    for cand in (np.argpartition(gap, k - 1)[:k], None):
        order = np.argsort(gap) if cand is None else cand[np.argsort(gap[cand])]
        for c in range(0, len(order), 16384):
            o = order[c:c + 16384]
            ok = (gap[o] > 0.0) & ((p[iu[o]] != p[ju[o]]).sum(1) > 1)
            if ok.any():
                return float(gap[o][np.argmax(ok)])
    return np.inf


def counts(adj):
    return adj.sum(1).astype(np.int64)


def first_core(adj, min_samples):
    c = np.nonzero(counts(adj) >= min_samples)[0]
    return int(c[0]) if len(c) else len(adj)


def cluster0(adj, min_samples):
    """bool [n]: the core-core connected component of first_core, plus every non-core point adjacent to one of its core points"""
    n = len(adj)
    core = counts(adj) >= min_samples
    f = first_core(adj, min_samples)
    seen = np.zeros(n, dtype=bool)
    if f >= n:
        return seen
    seen[f] = True
    front = np.array([f])
    while len(front):
        reach = adj[front].any(0) & core & ~seen
        seen |= reach
        front = np.nonzero(reach)[0]
    return seen | (~core & adj[:, seen].any(1))


def solve(pts, eps, min_samples):
    """(counts, first_core, cluster0) of one input"""
    adj = adjacency(pts, eps)
    return counts(adj), first_core(adj, min_samples), cluster0(adj, min_samples)


# ----------------------------------------------------------------------------- generators (all return fp32 [n, D])
def real_like(n, D=256, seed=0, scale=2.0):
    """what the workload clusters: non-negative, half-sparse pixel features (relu of a Gaussian, times scale), each used by up to
    8 class entries with its own activation in (0.05, 1] -- points on rays out of the origin, piled up near it; shuffled"""
    rs = np.random.RandomState(seed)
    feat = np.maximum(rs.randn((n + 7) // 8, D), 0.0) * scale
    act = 0.05 + 0.95 * (1.0 - rs.rand(n))
    pts = feat[np.arange(n) // 8] * act[:, None]
    return pts[rs.permutation(n)].astype(np.float32)


def noise_then_blob(n_noise, n_blob, D=256, seed=0):
    """n_noise mutually isolated points (no core among them), then a dense blob: the first core point is index n_noise"""
    rs = np.random.RandomState(seed)
    noise = rs.randn(n_noise, D) * 10.0
    blob = rs.randn(1, D) * 4.0 + rs.randn(n_blob, D) * 0.1
    return np.concatenate([noise, blob]).astype(np.float32)


def chain(n_chain, n_noise, D=256, seed=0):
    """the thin chain of tests/test_gpu_kernels.py::test_dbscan_cluster0_matches_sklearn at the same spacing, longer; shuffled"""
    rs = np.random.RandomState(seed)
    t = np.linspace(0, 400.0 * n_chain / 1500.0, n_chain)[:, None]
    d = np.zeros((1, D))
    d[0, 0] = 1.0
    pts = t * d + rs.randn(n_chain, D) * 0.05
    pts = np.concatenate([pts, rs.randn(n_noise, D) * 50.0])
    return pts[rs.permutation(n_chain + n_noise)].astype(np.float32)


# eps per D at which roughly half of cloud()'s points are core (min_samples = 5); every value is a multiple of 1/8
CLOUD_EPS = {4: 0.75, 20: 4.125, 36: 5.75, 252: 17.75, 256: 17.25, 260: 17.875, 512: 25.125}


def cloud(n, D, seed=0, shift=0.0):
    """two Gaussian clouds whose points have their own spread in [0.5, 1.5] (dense inside, sparse outside), the second one
    moved away along every axis; + shift in every coordinate"""
    rs = np.random.RandomState(seed)
    sig = 0.5 + rs.rand(n, 1)
    pts = rs.randn(n, D) * sig
    pts[n // 2:] += 6.0
    return (pts[rs.permutation(n)] + shift).astype(np.float32)


def tiny(n, D=256, seed=0):
    """a blob of n - n // 6 points and n // 6 far ones, shuffled"""
    rs = np.random.RandomState(seed + n)
    pts = np.concatenate([rs.randn(n - n // 6, D) * 0.1, rs.randn(n // 6, D) * 10.0])
    return pts[rs.permutation(n)].astype(np.float32)


def at_eps(eps, base, pattern, D=256):
    """Groups that a pair at EXACTLY eps decides.  Coordinates 1 .. D-1 of every point start at `base`; group k sits 100 away
    on axis 2 + k and is: a centre, three companions 0.25 / 0.5 / 0.75 beside it on axis 1, and one point q that differs from
    the centre on axis 0 only -- by fp32(eps) (pattern[k] True: d2 == eps^2 in any fp64 evaluation, a neighbour) or by the next
    fp32 above it (False: not a neighbour).  q is sqrt(eps^2 + 1/16) or more from the companions.  With min_samples = 5 the
    centre is core (count 5) exactly when its q is at eps.  Returns (pts, expected counts).
    (Axis 0 itself stays near 0: around 1000 the fp32 grid is 2^-14, two values there cannot differ by one ulp of eps.)"""
    e32 = np.float32(eps)
    up = np.nextafter(e32, np.float32(np.inf))
    assert float(np.float32(np.float32(base) + np.float32(100.0))) == float(base) + 100.0
    rows, cnt = [], []
    for k, on in enumerate(pattern):
        c = np.full(D, base, dtype=np.float32)
        c[0] = 0.0
        c[2 + k] += np.float32(100.0)
        rows.append(c)
        for o in (0.25, 0.5, 0.75):
            m = c.copy()
            m[1] += np.float32(o)
            rows.append(m)
        q = c.copy()
        q[0] = e32 if on else up
        rows.append(q)
        cnt += [5 if on else 4, 4, 4, 4, 2 if on else 1]
    return np.stack(rows), np.array(cnt)


def bridge(D=8):
    """11 points on axis 0: A = {-0.25, -0.125, 0, 0.125, 2} (indices 0-4), x = 4.875 (5), B = {7.75, 9.625, 9.75, 9.875, 10}
    (6-10).  eps = 3: A and B are 5-cliques, x is within eps of A's 2 and B's 7.75 only (count 3)."""
    pts = np.zeros((11, D), dtype=np.float32)
    pts[:, 0] = [-0.25, -0.125, 0.0, 0.125, 2.0, 4.875, 7.75, 9.625, 9.75, 9.875, 10.0]
    return pts


def glue_level(seed=0, n_images=2, hw=12 * 20, K=9, C=256, zero=False):
    """one pyramid level for condgraph.dbscan_positive_rows: (feat [N * HW, C] fp32 non-negative, every pixel with its own scale -- all zero with zero=True --,
    act [N * HW, K] fp32 in [0, 1) with about a fifth of the entries at or below the 0.05 threshold, some exactly on it)"""
    rs = np.random.RandomState(seed)
    feat = (np.maximum(rs.randn(n_images * hw, C), 0.0) * (0.0 if zero else 2.0) * rs.rand(n_images * hw, 1) ** 2).astype(np.float32)
    act = (rs.rand(n_images * hw, K) ** 2).astype(np.float32)
    act[rs.rand(n_images * hw, K) < 0.02] = np.float32(0.05)
    return feat, act


def glue_points(feat, act, n_images, thr):
    """the points of PrototypeComputation.DBSCAN_batch_cpu (reference loss.py:397-423) in its order -- image, class (background
    left out), pixel -- and the pixel row of each"""
    hw = feat.shape[0] // n_images
    rows = [n * hw + p for n in range(n_images) for c in range(1, act.shape[1]) for p in range(hw) if act[n * hw + p, c] > thr]
    cls = [c for n in range(n_images) for c in range(1, act.shape[1]) for p in range(hw) if act[n * hw + p, c] > thr]
    rows, cls = np.array(rows, dtype=np.int64), np.array(cls, dtype=np.int64)
    return feat[rows] * act[rows, cls][:, None], rows


def glue_rows(feat, act, n_images, eps, thr):
    """bool [N * HW]: a pixel row is selected when any of its points is outside cluster 0 (noise -> 1, cluster 0 -> 0, other
    clusters keep their label >= 1); with no non-zero point at all every candidate is selected"""
    pts, rows = glue_points(feat, act, n_images, thr)
    out = np.zeros(feat.shape[0], dtype=bool)
    if len(pts):
        sel = ~cluster0(adjacency(pts, eps), 5) if pts.any() else np.ones(len(pts), dtype=bool)
        out[rows[sel]] = True
    return out


# ----------------------------------------------------------------------------- the cases of the host and GPU tests
# name -> (builder, eps, min_samples).  Seeds are chosen so that the precondition below holds and, for the real-like clouds, so
# that there are core points inside and outside cluster 0 (tests/test_dbscan_host.py asserts both for every case).
CASES = {
    # ceil(n / 128) * 4 adjacency words per row: 68, 72 (a second trip of the 64-lane word loops) and 136 (three trips)
    "real_2049": (lambda: real_like(2049, seed=1), 3.0, 5),
    "real_2177": (lambda: real_like(2177, seed=1), 3.0, 5),
    "real_4229": (lambda: real_like(4229, seed=1), 3.0, 5),
    # the first core point (the seed of the breadth-first search) in word 65 / in the last, ragged tile (word 68)
    "late_core": (lambda: noise_then_blob(2100, 300, seed=3), 3.0, 5),
    "late_core_ragged_tile": (lambda: noise_then_blob(2176, 40, seed=4), 3.0, 5),
    "chain_2400": (lambda: chain(2300, 100, seed=5), 3.0, 5),
    "minsamples_cloud": (lambda: cloud(700, 256, seed=7), CLOUD_EPS[256], 5),
}
for _D in (4, 20, 36, 252, 260, 512):
    CASES["cloud_D%d" % _D] = (functools.partial(cloud, 700, _D, seed=_D), CLOUD_EPS[_D], 5)
for _D, _shift in ((256, 30.0), (256, 1000.0), (36, 30.0), (36, 1000.0)):
    CASES["shift%d_D%d" % (_shift, _D)] = (functools.partial(cloud, 700, _D, seed=_D + 1, shift=_shift), CLOUD_EPS[_D], 5)
TINY_N = (1, 4, 5, 31, 32, 33, 127, 128, 129)
for _n in TINY_N:
    CASES["tiny_%d" % _n] = (functools.partial(tiny, _n), 3.0, 5)

GAP_REL = 1e-9  # precondition of every input: min_gap >= GAP_REL * eps^2


@functools.lru_cache(maxsize=None)
def reference(name, min_samples=None):
    """dict(pts, eps, min_samples, counts, first_core, in0, gap) of a case, computed once per process; the arrays are read-only"""
    build, eps, ms = CASES[name]
    if min_samples is not None:
        base = reference(name)
        adj = base["adj"]
        out = dict(base, min_samples=min_samples, first_core=first_core(adj, min_samples), in0=cluster0(adj, min_samples))
        out["in0"].setflags(write=False)
        return out
    pts = build()
    d2 = sq_dists(pts, eps)
    adj = d2 <= eps2_of(eps)
    out = dict(pts=pts, eps=eps, min_samples=ms, adj=adj, counts=counts(adj), first_core=first_core(adj, ms),
               in0=cluster0(adj, ms), gap=min_gap(pts, eps, d2))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out

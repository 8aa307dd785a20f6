"""Density clustering (scan_dbscan_*), everything that needs no GPU: the fp64 reference of tests/dbscan_ref.py against sklearn and
against hand-made known answers, the precondition that every generated input of tests/test_gpu_dbscan.py has to meet, the new
C-ABI symbol and the argument checks (which run before anything touches a device)."""
import ctypes
import os
import re

import numpy as np
import pytest

import dbscan_ref as R
from scan_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sk_in0(pts, eps, min_samples):
    from sklearn import cluster
    return cluster.DBSCAN(eps=eps, min_samples=min_samples).fit_predict(pts) == 0


# ----------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_reference_matches_sklearn_and_gap_precondition(name):
    """cluster 0 of the reference == (sklearn label == 0) point by point on every generated case of the GPU tests, and no pair
    of any case is closer to eps^2 than 1e-9 eps^2 (the kernel and the reference decide near pairs from fp64 direct sums in
    different orders, which differ by ~D 2^-52 d2 = 1e-13 d2 at D = 512: four orders of margin).  The exactly-at-eps inputs
    (R.at_eps) are NOT compared with sklearn: a pair at exactly eps is a coin toss inside sklearn itself, see the comment of
    the "duplicates" case in tests/test_gpu_kernels.py::test_dbscan_cluster0_matches_sklearn."""
    ref = R.reference(name)
    assert ref["gap"] >= R.GAP_REL * R.eps2_of(ref["eps"]), (ref["gap"], R.eps2_of(ref["eps"]))
    assert np.array_equal(ref["in0"], _sk_in0(ref["pts"], ref["eps"], ref["min_samples"]))
    assert ref["counts"].min() >= 1 and np.array_equal(ref["adj"], ref["adj"].T)


@pytest.mark.parametrize("min_samples", [1, 2, 33])
def test_reference_matches_sklearn_over_min_samples(min_samples):
    ref = R.reference("minsamples_cloud", min_samples)
    assert np.array_equal(ref["in0"], _sk_in0(ref["pts"], ref["eps"], min_samples))
    assert ref["first_core"] < len(ref["pts"])


def test_cases_exercise_what_they_are_for():
    for name in ("real_2049", "real_2177", "real_4229"):
        ref = R.reference(name)
        core = ref["counts"] >= 5
        assert (core & ref["in0"]).sum() > 50 and (core & ~ref["in0"]).sum() > 50, name
        assert (~core & ref["in0"]).any() and (~core & ~ref["in0"]).any(), name  # border points of cluster 0, and noise
    assert R.reference("late_core")["first_core"] == 2100  # word 65
    assert R.reference("late_core_ragged_tile")["first_core"] == 2176  # the 18th tile holds 40 points
    assert R.reference("late_core")["in0"].sum() == 300 and R.reference("late_core_ragged_tile")["in0"].sum() == 40
    ref = R.reference("chain_2400")
    assert ref["in0"].sum() == 2300  # the whole chain is one cluster, the 100 far points are not
    # the chain cannot be walked inside one 64-word span: consecutive links cross between words < 64 and words >= 64
    order = np.argsort(ref["pts"][ref["in0"], 0])
    hi = (np.nonzero(ref["in0"])[0][order] >> 5) >= 64
    assert (hi[1:] != hi[:-1]).sum() > 100
    for D in (4, 20, 36, 252, 260, 512):
        ref = R.reference("cloud_D%d" % D)
        core = ref["counts"] >= 5
        assert 0.3 < core.mean() < 0.7, (D, core.mean())
        assert (core & ~ref["in0"]).any() and (core & ref["in0"]).any(), D
    for name in ("shift30_D256", "shift1000_D256", "shift30_D36", "shift1000_D36"):
        ref = R.reference(name)
        core = ref["counts"] >= 5
        assert 0.2 < core.mean() < 0.8 and (core & ~ref["in0"]).any() and (core & ref["in0"]).any(), name
    # |p|^2 against eps^2: at +30 the bf16x3 band 5.9e-5 (si + sj) is comparable to eps^2, at +1000 it is beyond any d2
    r30, r1000 = R.reference("shift30_D256"), R.reference("shift1000_D256")
    s30 = (r30["pts"].astype(np.float64) ** 2).sum(1).mean()
    s1000 = (r1000["pts"].astype(np.float64) ** 2).sum(1).mean()
    assert 0.05 < 5.9e-5 * 2 * s30 / R.eps2_of(r30["eps"]) < 1
    p = r1000["pts"].astype(np.float64)
    sq = (p * p).sum(1)
    off = np.abs(R.sq_dists(r1000["pts"], r1000["eps"]) - R.eps2_of(r1000["eps"])) / (sq[:, None] + sq[None, :])
    assert off.max() < 5.9e-5  # bf16x3: every pair is decided by the fp64 re-check
    assert (off < 1.7e-5).mean() > 0.45  # fp32: every pair inside one of the two clouds, and with it every pair near eps


# ----------------------------------------------------------------------------- known answers on a handful of points
def _line(xs, D=4):
    pts = np.zeros((len(xs), D), dtype=np.float32)
    pts[:, 0] = xs
    return pts


def test_known_answer_no_core():
    c, f, m = R.solve(_line([0, 1, 2, 10, 11, 20]), 3.0, 5)
    assert c.tolist() == [3, 3, 3, 2, 2, 1] and f == 6 and not m.any()


def test_known_answer_min_samples_one():
    """every point is core: cluster 0 is the eps-connected component of point 0"""
    c, f, m = R.solve(_line([0, 50, 2.5, 52, 5, 100, 7.5]), 3.0, 1)
    assert c.tolist() == [2, 2, 3, 2, 3, 1, 2] and f == 0
    assert m.tolist() == [True, False, True, False, True, False, True]


def test_known_answer_border_before_first_core():
    """point 0 has 2 neighbours (itself and point 3): not core, but next to a core point of the first cluster"""
    xs = [0.0, 50.0, 4.0, 3.0, 3.5, 4.5, 5.0, 60.0]
    c, f, m = R.solve(_line(xs), 3.0, 5)
    assert c.tolist() == [2, 1, 5, 6, 5, 5, 5, 1] and f == 2
    assert m.tolist() == [True, False, True, True, True, True, True, False]
    assert np.array_equal(m, _sk_in0(_line(xs), 3.0, 5))


def test_known_answer_one_point_bridge():
    pts = R.bridge()
    c, f, m = R.solve(pts, 3.0, 5)
    assert c.tolist() == [5, 5, 5, 5, 6, 3, 6, 5, 5, 5, 5] and f == 0
    assert m.tolist() == [True] * 6 + [False] * 5  # A and x; x is not core, so B is not reached through it
    c3, f3, m3 = R.solve(pts, 3.0, 3)
    assert np.array_equal(c3, c) and f3 == 0 and m3.all()  # x is core now and B joins
    assert np.array_equal(m, _sk_in0(pts, 3.0, 5)) and np.array_equal(m3, _sk_in0(pts, 3.0, 3))


@pytest.mark.parametrize("eps", [3.0, 2.7])
@pytest.mark.parametrize("base", [0.0, 1000.0])
def test_known_answer_exactly_at_eps(eps, base):
    """d2 == eps^2 is a neighbour, the next fp32 distance above eps is not; eps^2 is the square of fp32(eps)"""
    pattern = (False, True, False, True)
    pts, cnt = R.at_eps(eps, base, pattern)
    c, f, m = R.solve(pts, eps, 5)
    assert np.array_equal(c, cnt) and f == 5
    assert np.array_equal(np.nonzero(m)[0], np.arange(5, 10))
    d2 = R.sq_dists(pts, eps)
    assert d2[5, 9] == R.eps2_of(eps) and d2[0, 4] > R.eps2_of(eps) and d2[0, 4] - R.eps2_of(eps) < 1e-6 * R.eps2_of(eps)
    assert R.min_gap(pts, eps) >= R.GAP_REL * R.eps2_of(eps)


def test_min_gap_leaves_out_single_component_pairs():
    pts = np.zeros((3, 4), dtype=np.float32)
    pts[1, 0] = np.nextafter(np.float32(3.0), np.float32(4.0))  # one component: left out although 1.4e-6 from eps^2
    pts[2, :2] = (2.0, 2.0)  # d2 = 8 to point 0
    assert R.min_gap(pts, 3.0) == pytest.approx(1.0)
    assert R.min_gap(pts[:2], 3.0) == np.inf


# ----------------------------------------------------------------------------- the Python glue, "host" backend
@pytest.mark.parametrize("zero", [False, True])
def test_glue_host_backend_matches_restatement(zero):
    """condgraph.dbscan_positive_rows with sklearn behind it (runs on CPU tensors) against the plain loops of R.glue_rows: the
    point order, the act > thr mask (entries exactly at thr are out), noise -> 1 and the any-class rule; the same inputs go
    through the "device" backend in tests/test_gpu_dbscan.py"""
    import torch
    from scan_amd.modeling import condgraph
    feat, act = R.glue_level(seed=11, zero=zero)
    pts, rows = R.glue_points(feat, act, 2, 0.05)
    assert (act == np.float32(0.05)).sum() > 20 and (act[:, 1:] <= 0.05).mean() > 0.1 and len(pts) > 2048
    want = R.glue_rows(feat, act, 2, 3.0, 0.05)
    if zero:
        assert want.sum() == len(np.unique(rows))
    else:
        assert R.min_gap(pts, 3.0) >= R.GAP_REL * 9.0
        assert 0.1 < want.mean() < 0.9
    old = condgraph.DBSCAN_BACKEND
    condgraph.DBSCAN_BACKEND = "host"
    try:
        got = condgraph.dbscan_positive_rows(torch.from_numpy(feat), torch.from_numpy(act), 2, 3.0, 0.05)
    finally:
        condgraph.DBSCAN_BACKEND = old
    assert got.dtype == torch.bool and np.array_equal(got.numpy(), want)


# ----------------------------------------------------------------------------- C ABI
def test_neighbor_counts_symbol_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "scan_hip.h")).read()
    declared = set(re.findall(r"\b(scan_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in ("scan_dbscan_ws_bytes", "scan_dbscan_prepare", "scan_dbscan_neighbor_counts", "scan_dbscan_bfs_step",
                 "scan_dbscan_finish"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(L, name), name


def check_arguments():
    """every scan_dbscan_* entry point names the argument it refuses (shared with the GPU test: the checks come first)"""
    p = ctypes.c_void_p(64)
    prep = lambda **kw: _lib.call("scan_dbscan_prepare", *[kw.get(k, v) for k, v in (
        ("pts", p), ("n", 8), ("D", 4), ("eps", 3.0), ("min_samples", 5), ("ws", p), ("info", p), ("stream", None))])
    for ptr in ("pts", "ws", "info"):
        with pytest.raises(RuntimeError, match=ptr + " is a null pointer"):
            prep(**{ptr: None})
    for D in (0, -4, 6, 255):
        with pytest.raises(RuntimeError, match="D=%d" % D):
            prep(D=D)
    for n in (0, -1, 1200001):
        with pytest.raises(RuntimeError, match="n=%d" % n):
            prep(n=n)
    for eps in (0.0, -1.0, float("nan")):
        with pytest.raises(RuntimeError, match="eps="):
            prep(eps=eps)
    for ms in (0, -3):
        with pytest.raises(RuntimeError, match="min_samples=%d" % ms):
            prep(min_samples=ms)
    for name, args, ptrs in (("scan_dbscan_neighbor_counts", [8, p, p, None], {1: "ws", 2: "counts"}),
                             ("scan_dbscan_bfs_step", [8, p, 0, p, None], {1: "ws", 3: "changed"}),
                             ("scan_dbscan_finish", [8, p, p, None], {1: "ws", 2: "in_cluster0"})):
        for k, nm in ptrs.items():
            with pytest.raises(RuntimeError, match=nm + " is a null pointer"):
                _lib.call(name, *[None if i == k else a for i, a in enumerate(args)])
        for n in (0, 1200001):
            with pytest.raises(RuntimeError, match="n=%d" % n):
                _lib.call(name, n, *args[1:])
    assert _lib.query("scan_dbscan_ws_bytes", 1200001) == -1 and _lib.query("scan_dbscan_ws_bytes", 0) == -1
    # bit matrix + norms + counts + four masks, nothing else of size
    n, nw = 2177, 72
    assert n * nw * 4 + n * 12 + 16 * nw <= _lib.query("scan_dbscan_ws_bytes", n) <= n * nw * 4 + n * 12 + 16 * nw + 256


def test_arguments_validated_without_device():
    check_arguments()

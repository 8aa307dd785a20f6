"""GPU tests of scan_dbscan_* (csrc/dbscan.hip) against the fp64 reference of tests/dbscan_ref.py.  Every comparison is exact:
the neighbour count of EVERY point (scan_dbscan_neighbor_counts -- one flipped adjacency bit always shows there), the lowest
core index (info[0]) and the membership of cluster 0, under both settings of scan_tune "dbscan_bf16x3", which must also agree
with each other.  tests/test_dbscan_host.py checks the reference itself (sklearn, known answers) and that no input has a pair
within 1e-9 eps^2 of eps^2 -- closer than that, two fp64 sums of the same pair in different orders could decide differently."""
import numpy as np
import pytest
import torch

import dbscan_ref as R

pytestmark = pytest.mark.gpu

GEMMS = (("bf16x3", 1), ("fp32", 0))


def _device_run(pts, eps, min_samples, device, ws=None):
    """(counts, first_core, in_cluster0) through _lib.call, in the caller's workspace if there is one"""
    from scan_amd import _lib, ops
    n, d = pts.shape
    x = torch.from_numpy(np.array(pts)).to(device)
    nbytes = _lib.query("scan_dbscan_ws_bytes", n)
    assert nbytes > 0
    if ws is None:
        ws = torch.empty((nbytes // 8 + 1,), dtype=torch.float64, device=device)
    assert ws.numel() * ws.element_size() >= nbytes
    info = torch.full((2,), -7, dtype=torch.int32, device=device)
    counts = torch.full((n,), -7, dtype=torch.int32, device=device)
    out = torch.zeros((n,), dtype=torch.uint8, device=device)
    changed = torch.zeros((1,), dtype=torch.int32, device=device)
    st = ops._stream()
    _lib.call("scan_dbscan_prepare", ops._ptr(x), n, d, float(eps), int(min_samples), ops._ptr(ws), ops._ptr(info), st)
    _lib.call("scan_dbscan_neighbor_counts", n, ops._ptr(ws), ops._ptr(counts), st)
    first = int(info[0].item())
    assert int(info[1].item()) == 0
    if first < n:
        parity = 0
        for _ in range(n + 1):  # a breadth-first search over n points has at most n levels
            _lib.call("scan_dbscan_bfs_step", n, ops._ptr(ws), parity, ops._ptr(changed), st)
            if int(changed.item()) == 0:
                break
            parity ^= 1
        else:
            raise AssertionError("the breadth-first search did not end")
        _lib.call("scan_dbscan_finish", n, ops._ptr(ws), ops._ptr(out), st)
    return counts.cpu().numpy(), first, out.bool().cpu().numpy()


def _both_gemms(pts, eps, min_samples, device, want=None):
    """run under both "dbscan_bf16x3" settings (restored afterwards) and through ops.dbscan_in_cluster0; compare everything
    with want = (counts, first_core, in0) and the two settings with each other"""
    from scan_amd import _lib, ops
    if want is None:
        want = R.solve(pts, eps, min_samples)
    got = {}
    for name, val in GEMMS:
        old = _lib.query("scan_tune", b"dbscan_bf16x3", val)
        try:
            got[name] = _device_run(pts, eps, min_samples, device)
            via_ops = ops.dbscan_in_cluster0(torch.from_numpy(np.array(pts)).to(device), eps, min_samples).cpu().numpy()
        finally:
            _lib.query("scan_tune", b"dbscan_bf16x3", old)
        c, f, m = got[name]
        bad = np.nonzero(c != want[0])[0]
        assert len(bad) == 0, "%s: neighbour counts differ at %d of %d points, first %d: %d for %d" % (
            name, len(bad), len(c), bad[0], c[bad[0]], want[0][bad[0]])
        assert f == want[1], (name, f, want[1])
        assert np.array_equal(m, want[2]), "%s: cluster-0 membership differs at %d of %d points" % (name, (m != want[2]).sum(), len(m))
        assert via_ops.dtype == np.bool_ and np.array_equal(via_ops, m), name
    a, b = got["bf16x3"], got["fp32"]
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])
    return got


def _case(name, device, min_samples=None):
    ref = R.reference(name, min_samples)
    assert ref["gap"] >= R.GAP_REL * R.eps2_of(ref["eps"])
    return _both_gemms(ref["pts"], ref["eps"], ref["min_samples"], device, (ref["counts"], ref["first_core"], ref["in0"]))


@pytest.mark.parametrize("name", ["real_2049", "real_2177", "real_4229"])
def test_word_loop_trips(device, name):
    """more than 2048 points: 68, 72 and 136 adjacency words per row, so the 64-lane word loops of the core, breadth-first and
    finish kernels take a second and a third trip; workload-like points (non-negative, sparse, piled up near the origin) with
    core points inside and outside cluster 0"""
    ref = R.reference(name)
    core = ref["counts"] >= 5
    assert (core & ref["in0"]).any() and (core & ~ref["in0"]).any()
    _case(name, device)


@pytest.mark.parametrize("name", ["late_core", "late_core_ragged_tile"])
def test_first_core_beyond_word_64(device, name):
    """the seed write and the first frontier row are in a second-trip word (index 2100), or in the last, ragged tile (2176)"""
    assert R.reference(name)["first_core"] >> 5 >= 64
    _case(name, device)


def test_chain_across_words(device):
    """a thin shuffled chain of 2300 points: hundreds of breadth-first levels that hop between first-trip and second-trip words"""
    _case("chain_2400", device)


@pytest.mark.parametrize("D", [4, 20, 36, 252, 260, 512])
def test_point_dimensions(device, D):
    """D below one 32-wide K chunk, with a zero-padded K tail, and above 256 (the band follows D there; D = 512 is a sanity check,
    random rounding errors do not approach the worst-case bound the band is sized for)"""
    _case("cloud_D%d" % D, device)


@pytest.mark.parametrize("name", ["shift30_D256", "shift1000_D256", "shift30_D36", "shift1000_D36"])
def test_far_from_the_origin(device, name):
    """|p|^2 >> eps^2: the Gram form cancels catastrophically; at +30 the re-check band is comparable to eps^2, at +1000 every
    pair that could be a neighbour is inside it and decided by the fp64 path"""
    _case(name, device)


@pytest.mark.parametrize("eps", [3.0, 2.7])
@pytest.mark.parametrize("base", [0.0, 1000.0])
def test_exactly_at_eps(device, base, eps):
    """a pair at exactly fp32(eps) is a neighbour (d2 == eps^2 bit for bit), the next fp32 above it is not: each such pair makes
    its centre core or not, so counts, first core and membership all move with it"""
    for pattern in ((False, True, False, True), (True, False, True), (False, False)):
        pts, cnt = R.at_eps(eps, base, pattern)
        want = R.solve(pts, eps, 5)
        assert np.array_equal(want[0], cnt)
        first = 5 * pattern.index(True) if True in pattern else len(pts)
        assert want[1] == first and want[2].sum() == (5 if True in pattern else 0)
        _both_gemms(pts, eps, 5, device, want)


@pytest.mark.parametrize("D", [8, 256])
def test_one_point_bridge(device, D):
    """A and B are joined only through x (3 neighbours): with min_samples = 5 x is a border point of A and B stays out, with 3 x
    is core and B joins -- the `& core` of the breadth-first step and the border rule of finish"""
    pts = R.bridge(D)
    got5 = _both_gemms(pts, 3.0, 5, device)["bf16x3"]
    assert got5[2].tolist() == [True] * 6 + [False] * 5
    got3 = _both_gemms(pts, 3.0, 3, device)["bf16x3"]
    assert got3[2].all()
    # border point with a lower index than the first core point
    perm = np.array([5, 0, 1, 2, 3, 4, 6, 7, 8, 9, 10])
    got = _both_gemms(pts[perm], 3.0, 5, device)["bf16x3"]
    assert got[1] == 1 and got[2].tolist() == [True] * 6 + [False] * 5


@pytest.mark.parametrize("min_samples", [1, 2, 5, 33, 701])
def test_min_samples_sweep(device, min_samples):
    ref = R.reference("minsamples_cloud", min_samples)
    got = _case("minsamples_cloud", device, min_samples)["bf16x3"]
    if min_samples == 1:
        assert got[1] == 0
    if min_samples == 701:  # n + 1: no core point
        assert len(ref["pts"]) == 700 and got[1] == 700 and not got[2].any()


@pytest.mark.parametrize("n", R.TINY_N)
def test_tiny_n(device, n):
    _case("tiny_%d" % n, device)


def test_dirty_and_reused_workspace(device):
    """nothing is read from the workspace before it is written: a buffer filled with 0xFF, used for n = 2177 and then for
    n = 300, gives what a fresh one gives"""
    from scan_amd import _lib
    big, small = R.reference("real_2177"), R.reference("real_2177")["pts"][:300]
    want_small = R.solve(small, 3.0, 5)
    assert want_small[1] < 300 and want_small[2].any() and not want_small[2].all()
    nbytes = _lib.query("scan_dbscan_ws_bytes", 2177)
    ws = torch.full((nbytes // 8 + 1,), float("nan"), dtype=torch.float64, device=device)
    ws.view(torch.uint8).fill_(0xFF)
    for pts, want in ((big["pts"], (big["counts"], big["first_core"], big["in0"])), (small, want_small)):
        c, f, m = _device_run(pts, 3.0, 5, device, ws)
        assert np.array_equal(c, want[0]) and f == want[1] and np.array_equal(m, want[2])


def test_run_to_run_equality(device):
    ref = R.reference("real_4229")
    a = _device_run(ref["pts"], 3.0, 5, device)
    b = _device_run(ref["pts"], 3.0, 5, device)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])


def test_argument_checks(device):
    from scan_amd import ops
    from test_dbscan_host import check_arguments
    check_arguments()
    out = ops.dbscan_in_cluster0(torch.zeros((0, 256), device=device), 3.0, 5)
    assert out.dtype == torch.bool and out.shape == (0,) and out.device.type == "cuda"
    with pytest.raises(RuntimeError, match="D=6"):
        ops.dbscan_in_cluster0(torch.zeros((8, 6), device=device), 3.0, 5)
    with pytest.raises(RuntimeError, match="eps="):
        ops.dbscan_in_cluster0(torch.zeros((8, 4), device=device), 0.0, 5)
    with pytest.raises(RuntimeError, match="min_samples=0"):
        ops.dbscan_in_cluster0(torch.zeros((8, 4), device=device), 3.0, 0)


@pytest.mark.parametrize("zero", [False, True])
def test_glue_device_equals_host(device, zero):
    """condgraph.dbscan_positive_rows on one level (N = 2, 12 x 20, K = 9, 256 channels): the "device" backend selects the rows
    its own "host" spelling (sklearn) selects, and both select what the plain restatement selects"""
    from scan_amd.modeling import condgraph
    feat, act = R.glue_level(seed=11, zero=zero)
    want = R.glue_rows(feat, act, 2, 3.0, 0.05)
    f, a = torch.from_numpy(feat).to(device), torch.from_numpy(act).to(device)
    old, got = condgraph.DBSCAN_BACKEND, {}
    try:
        for backend in ("device", "host"):
            condgraph.DBSCAN_BACKEND = backend
            got[backend] = condgraph.dbscan_positive_rows(f, a, 2, 3.0, 0.05).cpu().numpy()
    finally:
        condgraph.DBSCAN_BACKEND = old
    assert np.array_equal(got["device"], got["host"])
    assert np.array_equal(got["device"], want) and want.any() and (zero or not want.all())

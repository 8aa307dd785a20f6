"""GPU tests of the five kernels of scan_amd/csrc/dynconv.hip against the float64 oracle of tests/dynconv_ref.py (pinned on the
CPU by tests/test_dynconv_host.py): past the forward's grid cap of 2048 workgroups and the backward's of 512, around the row
chunks of 4 / 6 / 8 and the 16-row MFMA group, at logits where a softmax without max subtraction or class masking breaks, on the
d_logits / d_probs == NULL branches only the C ABI reaches, with guard rows behind every output and a poisoned workspace, with
non-finite rows inside a tile, run to run, through both bindings, and on empty input.

Bars: tier A (derived worst-case roundings) everywhere, tier B (4 x the error of the sequential fp32 spelling) past the grid
cap; both are stated and derived in dynconv_ref's docstring.  The kernels do not return dz; test 4 reads it out of d_feat with
unit-vector kernels.

Every launch goes through the C ABI into outputs with GUARD_ROWS rows of GUARD behind them (ws: WS_GUARD floats), checked after
every call.  K per dispatch: dynconv_ref.DISPATCH; a case with knob = 1 runs under scan_tune "dynconv_generic"."""
import numpy as np
import pytest
import torch

import dynconv_ref as R

pytestmark = pytest.mark.gpu

GUARD, GUARD_ROWS, WS_GUARD = 7.0, 16, 4096


def _ids(dispatch):
    return ["K%d%s" % (k, "-generic" if g else "") for k, g in dispatch]


IDS = _ids(R.DISPATCH)


# ----------------------------------------------------------------------------- plumbing
def _lib_ops():
    from scan_amd import _lib, ops
    return _lib, ops, ops._ptr, ops._stream()


def _knob():
    from scan_amd import _lib
    return _lib.query("scan_tune_get", b"dynconv_generic")


def _under_knob(generic, fn):
    """fn() with scan_tune "dynconv_generic" = 1 when asked; the knob is back at 0 whatever fn does"""
    from scan_amd import _lib
    if not generic:
        return fn()
    old = _lib.query("scan_tune", b"dynconv_generic", 1)
    try:
        assert old == 0
        return fn()
    finally:
        _lib.query("scan_tune", b"dynconv_generic", 0)


def _dev(a, device):
    if a is None or isinstance(a, torch.Tensor):
        return a
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)


def _guarded(rows, cols, device):
    return torch.full((rows + GUARD_ROWS, cols), GUARD, dtype=torch.float32, device=device)


def _intact(buf, rows):
    return bool((buf[rows:] == GUARD).all())


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _np(t):
    return t.detach().cpu().numpy()


def _forward(device, feat, ker, generic=0):
    """scan_dynconv_softmax_forward into guarded outputs: (logits [M, K], probs [M, K]) on the device"""
    _lib, ops, P, st = _lib_ops()
    fd, kd = _dev(feat, device), _dev(ker, device)
    M, K = fd.shape[0], kd.shape[0]
    lg, pr = _guarded(M, K, device), _guarded(M, K, device)
    _under_knob(generic, lambda: _lib.call("scan_dynconv_softmax_forward", P(fd), P(kd), M, R.C, K, P(lg), P(pr), st))
    torch.cuda.synchronize()
    assert _intact(lg, M) and _intact(pr, M), ("forward wrote behind row M", M, K, generic)
    return lg[:M], pr[:M]


def _backward(device, feat, ker, probs, dl, dp, generic=0, ws_fill=GUARD):
    """scan_dynconv_softmax_backward (dl / dp may be None: NULL) into guarded outputs, ws filled with ws_fill:
    (d_feat [M, 256], d_kernels [K, 256]) on the device"""
    _lib, ops, P, st = _lib_ops()
    fd, kd, pd, dld, dpd = (_dev(a, device) for a in (feat, ker, probs, dl, dp))
    M, K = fd.shape[0], kd.shape[0]
    n_ws = _lib.query("scan_dynconv_ws_floats", M, R.C, K)
    assert n_ws == R.bwd_blocks(M) * K * R.C
    ws = torch.full((n_ws + WS_GUARD,), GUARD, dtype=torch.float32, device=device)
    ws[:n_ws] = ws_fill
    df, dk = _guarded(M, R.C, device), _guarded(K, R.C, device)
    _under_knob(generic, lambda: _lib.call("scan_dynconv_softmax_backward", P(fd), P(kd), P(pd), P(dld), P(dpd), M, R.C, K, P(df),
                                           P(dk), P(ws), st))
    torch.cuda.synchronize()
    assert _intact(df, M) and _intact(dk, K) and bool((ws[n_ws:] == GUARD).all()), ("backward wrote out of bounds", M, K, generic)
    return df[:M], dk[:K]


def _fmt(fig):
    return " ".join("%s %.3g" % (q, v) for q, v in sorted(fig.items()))


def _figures(device, c, generic):
    """forward and backward of case c (the backward from the reference's fp32 probabilities): the tier-B figures of the four
    results, and the results"""
    z, p = _forward(device, c.feat, c.ker, generic)
    df, dk = _backward(device, c.feat, c.ker, c.p32, c.dl, c.dp, generic)
    return c.figures(z=_np(z), p=_np(p), d_feat=_np(df), d_ker=_np(dk)), (z, p, df, dk)


def _dz(device, c, generic):
    """dz of case c as the backward kernel forms it: with the unit vectors e_k as kernels d_feat[:, k] = dz_k 1 + exact zeros"""
    df, _ = _backward(device, c.feat, np.eye(c.K, R.C, dtype=np.float32), c.p32, c.dl, c.dp, generic)
    assert not df[:, c.K:].any()
    return df[:, :c.K]


def _tier_a(device, c, generic, what):
    fig, res = _figures(device, c, generic)
    L = R.dker_chain_length(c.M, c.K, bool(generic))
    print("%s: %s (L = %d)" % (what, _fmt(fig), L))
    assert not R.over_tier_a(fig, c.K, L), what
    return fig, res


# ----------------------------------------------------------------------------- 1. past the grid cap
@pytest.mark.parametrize("K,generic", R.CAP_DISPATCH, ids=_ids(R.CAP_DISPATCH))
def test_past_the_grid_cap(device, K, generic):
    """M = 131089 = 16 (8192 + 1) + 1: every wave of the forward's 2048 workgroups has had its group when groups 8192 (full) and
    8193 (one row) go to waves 0 and 1 on their second trip; the backward's 512 workgroups loop 17 (<K>) or 33 times.  Tiers A
    and B, and rows 0 .. 131071 carry the bits of a launch on those rows alone (one trip)"""
    M, first = R.CAP_M, 16 * 8192
    c = R.case("standard", M, K)
    fig, (z, p, _, _) = _tier_a(device, c, generic, "standard M=%d K=%d" % (M, K))
    fig["dz"] = c.figures(dz=_np(_dz(device, c, generic)))["dz"]
    yard = R.yardstick("standard", M, K)
    print("dz %.3g | yardstick (sequential fp32, CPU): %s" % (fig["dz"], _fmt(yard)))
    assert not R.over_tier_a(fig, K, R.dker_chain_length(M, K, bool(generic)))
    assert not R.over_tier_b(fig, yard)
    z1, p1 = _forward(device, c.feat[:first], c.ker, generic)
    assert _bits(z[:first], z1) and _bits(p[:first], p1)
    assert _knob() == 0


# ----------------------------------------------------------------------------- 2. chunk edges
@pytest.mark.parametrize("K,generic", R.DISPATCH, ids=IDS)
def test_chunk_edges(device, K, generic):
    """M around the backward's row chunks (4 in the <K> instances, 8 in the generic kernel, 6 from K = 25) and the forward's
    16-row group, from less than one chunk to 65 rows = two workgroups of the backward"""
    for M in R.EDGE_MS:
        _tier_a(device, R.case("standard", M, K), generic, "standard M=%d K=%d" % (M, K))
    assert _knob() == 0


# ----------------------------------------------------------------------------- 3. extremes
@pytest.mark.parametrize("K,generic", R.EXTREME_DISPATCH, ids=_ids(R.EXTREME_DISPATCH))
@pytest.mark.parametrize("family", R.EXTREMES)
def test_extreme_logits(device, family, K, generic):
    M = R.EXTREME_M
    c = R.case(family, M, K)
    _, (z, p, df, dk) = _tier_a(device, c, generic, "%s M=%d K=%d" % (family, M, K))
    z, p = _np(z), _np(p)
    assert np.isfinite(z).all() and np.isfinite(p).all() and (p >= 0).all() and (p <= 1).all()
    if family == "ties":      # bit-identical kernel rows: the same chain per class column, the same exp, the same denominator
        for g in R.tie_groups(K):
            for k in g[1:]:
                assert np.array_equal(z[:, k].view(np.int32), z[:, g[0]].view(np.int32)), (g, k)
                assert np.array_equal(p[:, k].view(np.int32), p[:, g[0]].view(np.int32)), (g, k)
    elif family == "gap":     # saturation: exact 1 for the leader, and a finite backward from exact 0 / 1 probabilities
        one = c.p[:, K - 1] == 1.0
        assert one.any() and (p[one, K - 1] == 1.0).all()
        assert np.isfinite(_np(df)).all() and np.isfinite(_np(dk)).all()
    elif family == "offset_lo":
        # every real logit is far below the 0 of a padding class lane: a 0 in the maximum makes every exp underflow, a 0 in the
        # sum adds 1 to a denominator of about 1.  sum_k p_k = (sum_k e_k) / den (1 + d): the <= 5 additions of den, 1 division
        assert (np.abs(p.astype(np.float64).sum(1) - 1.0) <= (K + 8) * 2.0 ** -23).all()
    assert _knob() == 0


# ----------------------------------------------------------------------------- 4. gradient branches
@pytest.mark.parametrize("has_dl,has_dp", R.BRANCHES, ids=["dl", "dp", "dl+dp", "none"])
@pytest.mark.parametrize("K,generic", R.BRANCH_DISPATCH, ids=_ids(R.BRANCH_DISPATCH))
def test_gradient_branches_of_the_c_abi(device, K, generic, has_dl, has_dp):
    """d_logits_in == NULL and d_probs == NULL are separate paths of both backward kernels that the autograd wrappers never
    take.  M = 65: two workgroups.  With unit-vector kernels d_feat[:, :K] IS dz (the other products are exact zeros)"""
    M = R.BRANCH_M
    c = R.case("standard", M, K, has_dl, has_dp)
    L = R.dker_chain_length(M, K, bool(generic))
    df, dk = _backward(device, c.feat, c.ker, c.p32, c.dl, c.dp, generic)
    fig = c.figures(d_feat=_np(df), d_ker=_np(dk))
    fig["dz"] = c.figures(dz=_np(_dz(device, c, generic)))["dz"]
    print("standard M=%d K=%d dl=%s dp=%s: %s" % (M, K, has_dl, has_dp, _fmt(fig)))
    assert not R.over_tier_a(fig, K, L)
    if not has_dl and not has_dp:
        assert not df.any() and not dk.any()
    assert _knob() == 0


# ----------------------------------------------------------------------------- 5. guards and the workspace
@pytest.mark.parametrize("K,generic", R.DISPATCH, ids=IDS)
def test_guards_and_poisoned_workspace(device, K, generic):
    """_forward / _backward check the 16 guard rows behind logits, probs, d_feat and d_kernels and the 4096 floats behind ws;
    a workspace of NaN gives the bits of a workspace of 7.0: the reduction reads no slot the backward has not written"""
    for M in (1, 17, 65):
        c = R.case("standard", M, K)
        _, p = _forward(device, c.feat, c.ker, generic)
        df, dk = _backward(device, c.feat, c.ker, p, c.dl, c.dp, generic)
        df_n, dk_n = _backward(device, c.feat, c.ker, p, c.dl, c.dp, generic, ws_fill=float("nan"))
        assert _bits(df, df_n) and _bits(dk, dk_n), M
        assert bool(torch.isfinite(dk_n).all())
    assert _knob() == 0


# ----------------------------------------------------------------------------- 6. containment
@pytest.mark.parametrize("K,generic", R.DISPATCH, ids=IDS)
def test_non_finite_rows_stay_in_their_rows(device, K, generic):
    """rows 18 (all NaN) and 21 (+inf in channel 100) of the group 16 .. 31: two lane quarters of one MFMA tile, one 8-row and
    one 6-row chunk of the generic backward, neighbouring 4-row chunks of the <K> instances.  Every other row of logits, probs
    and d_feat has the bits of the clean run (d_kernels sums over the rows: not asserted)"""
    M, bad = 40, [18, 21]
    c = R.case("standard", M, K)
    dirty = c.feat.copy()
    dirty[18] = np.nan
    dirty[21, 100] = np.inf
    keep = torch.tensor([m for m in range(M) if m not in bad], device=device)
    z, p = _forward(device, c.feat, c.ker, generic)
    zd, pd = _forward(device, dirty, c.ker, generic)
    assert bool(torch.isnan(zd[18]).all()) and not bool(torch.isfinite(zd[21]).any())   # the kernel did see them
    assert _bits(z[keep], zd[keep]) and _bits(p[keep], pd[keep])
    df, _ = _backward(device, c.feat, c.ker, p, c.dl, c.dp, generic)
    dfd, _ = _backward(device, dirty, c.ker, pd, c.dl, c.dp, generic)
    assert bool(torch.isfinite(df).all()) and _bits(df[keep], dfd[keep])
    assert _knob() == 0


# ----------------------------------------------------------------------------- 7. reproducibility and bindings
@pytest.mark.parametrize("K", [9, 2])
def test_specialised_kernels_are_run_to_run_identical(device, K):
    c = R.case("standard", 4099, K)
    runs = []
    for _ in range(2):
        z, p = _forward(device, c.feat, c.ker)
        runs.append((z, p) + _backward(device, c.feat, c.ker, p, c.dl, c.dp))
    assert all(_bits(a, b) for a, b in zip(*runs))
    assert _knob() == 0


def test_both_bindings_give_the_same_bits(device):
    """layers.dynamic_conv_softmax (the compiled operator with C++ autograd when it is built) against ops.dynconv_softmax (ctypes,
    Python autograd) on the same NCHW input at K = 9: logits, probs and both gradients"""
    from scan_amd import layers, ops
    g = torch.Generator().manual_seed(79)
    N, H, W, K = 2, 7, 11, 9
    x = torch.randn(N, R.C, H, W, generator=g)
    ker = torch.randn(K, R.C, generator=g) / 16
    g1, g2 = torch.randn(N, K, H, W, generator=g).to(device), torch.randn(N, K, H, W, generator=g).to(device)
    res = []
    for compiled in (True, False):
        xd, kd = x.to(device).requires_grad_(True), ker.to(device).requires_grad_(True)
        if compiled:
            l, p = layers.dynamic_conv_softmax(xd, kd)
        else:
            rows = xd.permute(0, 2, 3, 1).reshape(N * H * W, R.C)
            l, p = (t.view(N, H, W, K).permute(0, 3, 1, 2) for t in ops.dynconv_softmax(rows, kd))
        assert l.shape == (N, K, H, W) and p.shape == (N, K, H, W)
        ((l * g1).sum() + (p * g2).sum()).backward()
        res.append((l.detach(), p.detach(), xd.grad, kd.grad))
    assert all(_bits(a, b) for a, b in zip(*res))
    assert bool(res[0][2].any()) and bool(res[0][3].any())
    assert _knob() == 0


# ----------------------------------------------------------------------------- 8. empty input
@pytest.mark.parametrize("K,generic", [(9, 0), (2, 0), (9, 1), (5, 0), (32, 0)], ids=["K9", "K2", "K9-generic", "K5", "K32"])
def test_empty_input(device, K, generic):
    """M = 0 is legal in both directions: the forward returns empty tensors, the backward clears d_kernels, returns 0 and launches
    nothing (NULL feat / probs / d_feat / ws are not looked at, a guarded workspace keeps its fill); M < 0 stays an error"""
    _lib, ops, P, st = _lib_ops()
    L = _lib.lib()
    ker = torch.randn(K, R.C, device=device)
    z, p = _forward(device, torch.empty((0, R.C), device=device), ker, generic)
    assert z.shape == (0, K) and p.shape == (0, K)
    dk = _guarded(K, R.C, device)
    ws = torch.full((WS_GUARD,), GUARD, device=device)
    rc = _under_knob(generic, lambda: L.scan_dynconv_softmax_backward(None, P(ker), None, None, None, 0, R.C, K, None, P(dk), P(ws), st))
    torch.cuda.synchronize()
    assert rc == 0
    assert not dk[:K].any() and _intact(dk, K) and bool((ws == GUARD).all())
    dk.fill_(GUARD)
    rc = _under_knob(generic, lambda: L.scan_dynconv_softmax_backward(None, P(ker), None, None, None, -1, R.C, K, None, P(dk), P(ws), st))
    torch.cuda.synchronize()
    assert rc != 0 and "bad M" in L.scan_last_error().decode()
    assert L.scan_dynconv_softmax_forward(None, P(ker), -1, R.C, K, None, None, st) != 0 and "bad M" in L.scan_last_error().decode()
    assert bool((dk == GUARD).all())
    # and through autograd: an empty input differentiates into an empty d_feat and a zero d_kernels
    fd, kd = torch.empty((0, R.C), device=device, requires_grad=True), ker.clone().requires_grad_(True)
    l, q = _under_knob(generic, lambda: ops.dynconv_softmax(fd, kd))
    _under_knob(generic, lambda: (l.sum() + q.sum()).backward())
    assert fd.grad.shape == (0, R.C) and kd.grad.shape == (K, R.C) and not kd.grad.any()
    assert _knob() == 0

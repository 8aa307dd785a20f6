"""GroupNorm(32) + ReLU, everything that needs no GPU: (a) the oracle of tests/groupnorm_ref.py against torch autograd in
float64 on every pyramid of tests/test_gpu_groupnorm_parity.py; (b) an fp32 emulation of the kernels' arithmetic with the group
sums widened per element inside half of every bar on every case -- the bars are reachable; (c) the same emulation with the
squares and four-sums in fp32 outside the rstd bar exactly where the GPU tests are meant to have teeth."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import groupnorm_ref as R

# rows of a (level, image) the emulation is swept over besides the pyramids: 1, 2, 15, 260, 1024
SWEEP = {"hw_%d" % hw: R.Shape(R.N, [(1, hw)]) for hw in (2, 15, 1024)}


def _shapes():
    out = {name: R.Shape(R.N, sizes) for name, sizes in R.PYRAMIDS.items()}
    out.update(SWEEP)
    return out


SHAPES = _shapes()


# ----------------------------------------------------------------------------- (a) the oracle
def _nchw(rows, shape, lvl):
    h, w = shape.sizes[lvl]
    return rows[shape.row_off[lvl]:shape.row_off[lvl + 1]].reshape(shape.n_images, h, w, R.C).permute(0, 3, 1, 2)


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("pyramid", sorted(R.PYRAMIDS))
def test_oracle_is_float64_autograd(pyramid, relu):
    c = R.case("friendly", pyramid)
    shape = c.shape
    x = torch.from_numpy(c.x.copy()).double().requires_grad_(True)
    gamma = torch.from_numpy(c.gamma.copy()).double().requires_grad_(True)
    beta = torch.from_numpy(c.beta.copy()).double().requires_grad_(True)
    eps = float(np.float32(R.EPS))
    ys = []
    for lvl in range(shape.n_levels):
        y = F.group_norm(_nchw(x, shape, lvl), R.G, gamma, beta, eps)
        ys.append((F.relu(y) if relu else y).permute(0, 2, 3, 1).reshape(-1, R.C))
    y = torch.cat(ys, 0)
    y.backward(torch.from_numpy(c.dy.copy()).double())
    fwd = c.fwd[relu]
    np.testing.assert_allclose(fwd.y, y.detach().numpy(), rtol=1e-12, atol=1e-12)
    assert (fwd.y >= 0).all() if relu else (fwd.y < 0).any()
    bwd = R.Backward(fwd, c.dy, fwd.ypre > 0 if relu else None)
    np.testing.assert_allclose(bwd.dx, x.grad.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(bwd.dgamma, gamma.grad.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(bwd.dbeta, beta.grad.numpy(), rtol=1e-12, atol=1e-12)
    # the table: per (level, image, group), against a plain loop
    for il, lvl, n, rows in R.slots(shape):
        for g in (0, 13, 31):
            v = c.x[rows, 8 * g:8 * g + 8].astype(np.float64)
            assert abs(fwd.mean[il, g] - v.mean()) <= 1e-12 * max(1.0, abs(v.mean()))
            assert abs(fwd.rstd[il, g] - 1.0 / np.sqrt(v.var() + eps)) <= 1e-12 * fwd.rstd[il, g]


def test_cases_are_what_they_claim():
    """a statistic read from a neighbouring slot -- the next group, the other image, the next (level, image) -- is outside the
    bars in every case; const has var = 0 exactly, y = beta and a finite dx; the sums handed to the FROM_SUMS paths are the slots'"""
    for name, (off, sd) in R.CASES.items():
        c = R.case(name, "ragged_three_levels")
        fwd = c.fwd[0]
        assert np.isfinite(c.x).all() and np.isfinite(fwd.y).all() and np.isfinite(fwd.rstd).all()
        cnt = np.array([260, 260, 15, 15, 2, 2])[:, None] * 8.0
        assert c.sums.shape == fwd.mean.shape + (2,)
        np.testing.assert_allclose(c.sums[..., 0] / cnt, fwd.mean, rtol=1e-9, atol=1e-12 * np.abs(c.x).max())
        # const has no scale to vary by level: its slots of one image differ by group only
        for axis, step in ((1, 1), (0, 1)) + (((0, 2),) if sd else ()):
            wrong_mean = np.abs(np.roll(fwd.mean, step, axis) - fwd.mean) > fwd.tol_mean()
            wrong_rstd = np.abs(np.roll(fwd.rstd, step, axis) - fwd.rstd) > fwd.tol_rstd()
            assert (wrong_mean | wrong_rstd).all(), (name, axis, step)
        if sd == 0:
            assert not fwd.var.any() and not fwd.xhat.any()
            assert np.array_equal(fwd.y, np.broadcast_to(c.beta.astype(np.float64), fwd.y.shape))
            bwd = R.Backward(fwd, c.dy)
            assert np.isfinite(bwd.dx).all() and np.abs(bwd.dx).max() > 1
        else:   # |mean| / std stays at or under twice the nominal offset / sd (the factor 1 + g / 32)
            assert (np.abs(fwd.mean) * np.sqrt(1.0 / fwd.var) <= 2 * abs(off) / sd + 3).all(), name


# ----------------------------------------------------------------------------- (b) the widened arithmetic meets the bars
def _emulated_figures(c, relu, widened=True):
    """every bar's ratio for the fp32 emulation on case c"""
    shape, fwd = c.shape, c.fwd[relu]
    table = R.emulate_stats(c.x, shape, widened=widened)
    fig = dict(zip(("mean", "rstd"), R.stats_ratios(table, fwd)))
    y, _ = R.emulate_forward(c.x, table, c.gamma, c.beta, shape, relu=bool(relu))
    fig["y"] = R.ratio(y, fwd.y, fwd.tol_y())
    dx, dg, db, mask = R.emulate_backward(c.x, c.dy, table, c.gamma, c.beta, shape, relu=bool(relu))
    bwd = R.Backward(fwd, c.dy, mask if relu else None)   # the mask the emulated kernel computed, as the GPU test hands over y > 0
    fig["dx"], fig["dgamma"], fig["dbeta"] = R.ratio(dx, bwd.dx, bwd.tol_dx()), R.ratio(dg, bwd.dgamma, bwd.tol_dgamma()), \
        R.ratio(db, bwd.dbeta, bwd.tol_dbeta())
    return fig


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_widened_arithmetic_is_inside_half_of_every_bar(name):
    worst = {}
    for sname, shape in SHAPES.items():
        c = R.Case(name, sname, shape) if sname in SWEEP else R.case(name, sname)
        for relu in (1, 0):
            fig = _emulated_figures(c, relu)
            print("%s %s relu=%d: %s" % (name, sname, relu, " ".join("%s %.3f" % kv for kv in sorted(fig.items()))))
            for k, v in fig.items():
                worst[k] = max(worst.get(k, 0.0), v)
            # the two statistics bars ARE the roundings of a correctly rounded table (u |mean| is round-to-nearest itself), so
            # the table may reach them; everything computed from it stays inside half of its bar
            assert fig["mean"] <= 1.0 and fig["rstd"] <= 1.0, (name, sname, relu, fig)
            assert all(fig[k] <= 0.5 for k in ("y", "dx", "dgamma", "dbeta")), (name, sname, relu, fig)
    print("%s worst: %s" % (name, " ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


# ----------------------------------------------------------------------------- (c) the arithmetic before does not
@pytest.mark.parametrize("pyramid", sorted(R.PYRAMIDS))
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_fp32_squares_break_the_rstd_bar_where_expected(name, pyramid):
    c = R.case(name, pyramid)
    old = R.stats_ratios(R.emulate_stats(c.x, c.shape, widened=False), c.fwd[0])
    new = R.stats_ratios(R.emulate_stats(c.x, c.shape, widened=True), c.fwd[0])
    print("%s %s: rstd error / bar  fp32 squares %.3g  widened %.3g" % (name, pyramid, old[1], new[1]))
    assert new[0] <= 1.0 and new[1] <= 1.0
    if name in R.BROKEN_BEFORE:
        assert old[1] > 1.0, (name, pyramid, old)
    if name == "huge":   # the fp32 square overflowed: rstd = 0
        assert not R.emulate_stats(c.x, c.shape, widened=False)[..., 1].any()

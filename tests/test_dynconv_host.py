"""Dynamic conv + softmax, everything that needs no GPU: the oracle of tests/dynconv_ref.py against torch autograd in float64,
the input families against the properties they are built for, the plain fp32 evaluations (torch-CPU operators and the sequential
fp32_chain_* spellings) inside tier A on every family and shape tests/test_gpu_dynconv.py uses -- the reference alone passes its
own bars -- and the tier-B yardsticks, printed."""
import numpy as np
import pytest
import torch

import dynconv_ref as R


def _fmt(fig):
    return " ".join("%s %.3g" % (q, v) for q, v in sorted(fig.items()))


# ----------------------------------------------------------------------------- 1. the oracle
@pytest.mark.parametrize("family,M,K", [("standard", 37, 9), ("standard", 13, 25), ("ties", 37, 5), ("offset_hi", 20, 2)])
@pytest.mark.parametrize("has_dl,has_dp", R.BRANCHES)
def test_oracle_is_float64_autograd(family, M, K, has_dl, has_dp):
    feat, ker, dl, dp = R.inputs(family, M, K)
    f = torch.from_numpy(feat).double().requires_grad_(True)
    k = torch.from_numpy(ker).double().requires_grad_(True)
    z = f @ k.t()
    p = z.softmax(1)
    loss = 0 * z.sum()
    if has_dl:
        loss = loss + (z * torch.from_numpy(dl).double()).sum()
    if has_dp:
        loss = loss + (p * torch.from_numpy(dp).double()).sum()
    loss.backward()
    zr, pr, S = R.forward(feat, ker)
    np.testing.assert_allclose(zr, z.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(pr, p.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(S, (f.detach().abs() @ k.detach().abs().t()).numpy(), rtol=1e-12, atol=1e-12)
    assert (S >= np.abs(zr)).all()
    b = R.backward(feat, ker, pr, dl if has_dl else None, dp if has_dp else None)  # the unrounded p: the same function as autograd
    np.testing.assert_allclose(b["d_feat"], f.grad.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(b["d_ker"], k.grad.numpy(), rtol=1e-12, atol=1e-12)
    assert (b["Dz"] >= np.abs(b["dz"]) * (1 - 1e-12)).all() and (b["Sf"] >= np.abs(b["d_feat"]) * (1 - 1e-12)).all()
    assert (b["Sk"] >= np.abs(b["d_ker"]) * (1 - 1e-12)).all()
    if not has_dl and not has_dp:
        assert not b["d_feat"].any() and not b["d_ker"].any() and not b["Sf"].any()


def test_launch_arithmetic():
    """bwd_blocks / dker_chain_length restate dc_bwd_blocks and the loops of the two backward kernels"""
    assert [R.bwd_blocks(M) for M in (1, 64, 65, 32768, 32769, R.CAP_M)] == [1, 1, 2, 512, 512, 512]
    assert R.dker_chain_length(R.CAP_M, 9) == 4 * 17 + 4 + 512      # 32773 chunks of 4 over 2048 waves
    assert R.dker_chain_length(R.CAP_M, 5) == 8 * 33 + 512          # 16387 chunks of 8 over 512 workgroups
    assert R.dker_chain_length(R.CAP_M, 9, True) == 8 * 33 + 512
    assert R.dker_chain_length(65, 25) == 6 * 6 + 2 and R.dker_chain_length(65, 24) == 8 * 5 + 2
    assert R.dker_chain_length(1, 2) == 4 + 4 + 1


# ----------------------------------------------------------------------------- 2. the families
@pytest.mark.parametrize("K,_", R.EXTREME_DISPATCH)
def test_extreme_families_are_what_they_claim(K, _):
    M = R.EXTREME_M
    for family in R.EXTREMES:
        c = R.case(family, M, K)
        assert np.isfinite(c.z).all() and np.isfinite(c.p).all() and all(np.isfinite(v).all() for v in c.bwd.values())
        np.testing.assert_allclose(c.p.sum(1), 1.0, rtol=0, atol=1e-14)
        z32 = c.z.astype(np.float32)
        naive_ok = bool(np.isfinite(R.fp32_naive_probs(z32)).all())
        print("%s K=%d: logits %.1f .. %.1f, naive fp32 softmax finite: %s, p < 2^-126: %d of %d" %
              (family, K, c.z.min(), c.z.max(), naive_ok, int((c.p < R.TINY).sum()), c.p.size))
        if family == "offset_hi":
            assert 84 < c.z.max() < 88 and c.z.min() > 0
        elif family == "offset_lo":
            assert -1010 < c.z.min() < -950 and -70 < c.z.max() < -55
            assert not naive_ok                                        # exp(-60) .. exp(-1000): 0 / 0 from row s = 2 on
            assert (c.p >= R.TINY).all()                               # yet no probability underflows: the spread is 2.5 s <= 40
        elif family == "gap":
            lead = c.z[:, K - 1] - np.delete(c.z, K - 1, 1).max(1)
            assert 150 < lead.max() < 170 and 5 < lead.min() < 15
            assert not naive_ok                                        # exp(160) = inf
            sat = c.p32[:, K - 1] == 1.0
            assert sat.any() and not sat.all()                         # saturated rows and ordinary rows
            assert (np.delete(c.p, K - 1, 1)[lead > 100] < R.TINY).all() and (c.p[lead < 80] >= R.TINY).all()
            assert (np.delete(c.p32, K - 1, 1)[lead > 110] == 0).all()  # exact zeros
        else:
            groups = R.tie_groups(K)
            assert any(0 in g and K - 1 in g for g in groups)
            for g in groups:
                for k in g[1:]:
                    assert np.array_equal(c.ker[k].view(np.int32), c.ker[g[0]].view(np.int32))
            assert len({tuple(r) for r in c.ker.view(np.int32).tolist()}) == min(K - 1, 3)


def test_standard_family_is_the_construction_of_test_dynconv_softmax():
    g = torch.Generator().manual_seed(257)
    feat = torch.randn(257, 256, generator=g)
    ker = torch.randn(2, 256, generator=g) / 16
    g1, g2 = torch.randn(257, 2, generator=g), torch.randn(257, 2, generator=g)
    for a, b in zip(R.inputs("standard", 257, 2), (feat, ker, g1, g2)):
        assert np.array_equal(a, b.numpy())


# ----------------------------------------------------------------------------- 3. the reference alone passes tier A
def _plain_fp32_inside_tier_a(c, what):
    """the sequential spelling and the torch-CPU operators on the inputs of case c; L = M: a sum of M terms in any order"""
    fig = c.figures(*c.chain())
    z, p, df, dk = R.torch_fp32(c.feat, c.ker, c.p32, c.dl, c.dp)
    tfig = c.figures(z=z, p=p, d_feat=df, d_ker=dk)
    print("%s: chain %s | torch %s" % (what, _fmt(fig), _fmt(tfig)))
    assert not R.over_tier_a(fig, c.K, c.M), (what, "chain")
    assert not R.over_tier_a(tfig, c.K, c.M), (what, "torch")
    return fig


@pytest.mark.parametrize("K", sorted({k for k, _ in R.DISPATCH}))
def test_plain_fp32_inside_tier_a_at_the_chunk_edges(K):
    for M in R.EDGE_MS:
        _plain_fp32_inside_tier_a(R.case("standard", M, K), "standard M=%d K=%d" % (M, K))


@pytest.mark.parametrize("family", R.EXTREMES)
def test_plain_fp32_inside_tier_a_at_the_extremes(family):
    for K, _ in R.EXTREME_DISPATCH:
        _plain_fp32_inside_tier_a(R.case(family, R.EXTREME_M, K), "%s M=%d K=%d" % (family, R.EXTREME_M, K))


@pytest.mark.parametrize("has_dl,has_dp", R.BRANCHES)
def test_plain_fp32_inside_tier_a_on_the_gradient_branches(has_dl, has_dp):
    for K in sorted({k for k, _ in R.BRANCH_DISPATCH}):
        c = R.case("standard", R.BRANCH_M, K, has_dl, has_dp)
        fig = _plain_fp32_inside_tier_a(c, "standard M=%d K=%d dl=%s dp=%s" % (R.BRANCH_M, K, has_dl, has_dp))
        if not has_dl and not has_dp:
            assert fig["dz"] == 0 and fig["d_feat"] == 0 and fig["d_ker"] == 0


# ----------------------------------------------------------------------------- 4. past the grid cap: tier A and the yardsticks
@pytest.mark.parametrize("K,_", R.CAP_DISPATCH)
def test_tier_b_yardsticks_past_the_grid_cap(K, _):
    """the figures test_gpu_dynconv.py multiplies by TIER_B_MARGIN; they are the sequential spelling's own errors, so they are
    inside tier A (L = M) and not zero"""
    yard = R.yardstick("standard", R.CAP_M, K)
    print("yardstick standard M=%d K=%d: %s" % (R.CAP_M, K, _fmt(yard)))
    assert set(yard) == {"logits", "probs", "dz", "d_feat", "d_ker"}
    assert not R.over_tier_a(yard, K, R.CAP_M)
    assert all(v > 0 for v in yard.values())
    c = R.case("standard", R.CAP_M, K)
    z, p, df, dk = R.torch_fp32(c.feat, c.ker, c.p32, c.dl, c.dp)
    tfig = c.figures(z=z, p=p, d_feat=df, d_ker=dk)
    print("torch-CPU fp32 M=%d K=%d: %s" % (R.CAP_M, K, _fmt(tfig)))
    assert not R.over_tier_a(tfig, K, R.CAP_M)

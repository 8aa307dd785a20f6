"""The class branches with the act-map channel taken out of the dense first conv (ops.CLS_SPLIT): the grouped conv that forms
relu(h_main + act term) in registers (scan_gconv3x3_to1_act_*) against a float64 statement on the CPU, the split weight
stacking against the torch construction (bit for bit), FCOSDiscriminator_con with the split on against off, and the bit
reproducibility of its backward in deterministic mode.

Bars of the kernel-level cases.  Every compared quantity is an fp32 sum of n products, so |err| <= n * 2^-23 * sum|terms|.
sum|terms| is computed in float64 by running the same float64 statement on the absolute values of all inputs (everything is
then non-negative, the ReLU is the identity, and autograd returns exactly the sums of the absolute terms).  n per quantity,
with M = pixels of the pyramid:
    hidden value  h_main + 9 act products               10     (enters the quantities below as a relative error of its terms)
    logits        9 x 128 products + bias + hidden      9 * 128 + 1 + 10
    dh            9 products                            9
    dw2           one product per pixel + hidden        M + 10
    db2           one term per pixel                    M
    dE            one product per pixel + dh            M + 9
    da            9 x 128 products + dh                 9 * 128 + 9
The ReLU mask is discontinuous, so h_main is drawn and then pushed away from zero: where the float64 |h_main + act term| is
under 1e-3 the element gets +-2e-3 (1000 times the hidden value's rounding error).  No element is left out of a comparison."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
PYRAMIDS = {"seam": (2, [(5, 7), (3, 4)]),   # two images: row neighbours cross an image seam, partial workgroups
            "thin": (2, [(1, 1), (1, 5)])}   # one-pixel and one-row images: every tap but the centre falls outside


def _rows(levels):
    """list of NCHW tensors -> [M, C] rows (level-major, then image, y, x)"""
    return torch.cat([x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]) for x in levels], 0).contiguous()


def _statement(hm, act, ew, w2, b2, dy, G):
    """float64: per level  y = conv3x3(relu(hm + conv3x3(act[:, 1:], E; one class per group)), w2; groups) + b2  and the
    gradients of <y, dy>.  hm / act / dy: lists of NCHW levels; ew [G*128, 1, 3, 3]; w2 [G, 128, 3, 3]."""
    leaves = [t.clone().requires_grad_(True) for t in hm] + [t.clone().requires_grad_(True) for t in act]
    ew, w2, b2 = (t.clone().requires_grad_(True) for t in (ew, w2, b2))
    L = len(hm)
    ys, hs, tot = [], [], 0.0
    for l in range(L):
        hsum = leaves[l] + F.conv2d(leaves[L + l][:, 1:1 + G], ew, None, padding=1, groups=G)
        hs.append(hsum.detach())
        y = F.conv2d(torch.relu(hsum), w2, b2, padding=1, groups=G)
        ys.append(y.detach())
        tot = tot + (y * dy[l]).sum()
    grads = torch.autograd.grad(tot, leaves + [ew, w2, b2])
    return {"y": _rows(ys), "hsum": _rows(hs), "dh": _rows(grads[:L]), "da": _rows(grads[L:2 * L]), "dE": grads[2 * L],
            "dw2": grads[2 * L + 1], "db2": grads[2 * L + 2]}


@pytest.fixture(params=[True, False], ids=["one_pass", "own_pass"])
def act_grads_path(request):
    """both backward routes: d act and dE inside the kernel that produces dh (scan_gconv3x3_to1_act_backward_all, the default)
    and in a pass of their own over dh (scan_gconv3x3_to1_act_backward + scan_gconv3x3_to1_act_grads)"""
    from scan_amd import ops
    old = ops.CLS_SPLIT_FUSED
    ops.CLS_SPLIT_FUSED = request.param
    yield request.param
    ops.CLS_SPLIT_FUSED = old


@pytest.mark.parametrize("pyr", sorted(PYRAMIDS))
@pytest.mark.parametrize("G", [1, 2, 4, 8])
def test_gconv_act_kernels_against_float64(device, G, pyr, act_grads_path):
    from scan_amd import ops
    n, sizes = PYRAMIDS[pyr]
    shape = ops.PyramidShape(n, sizes)
    M, K, gc = shape.rows, G + 1, G * 128
    g = torch.Generator().manual_seed(100 * G + len(pyr))
    hm = [torch.randn(n, gc, h, w, generator=g) for h, w in sizes]
    act = [torch.softmax(2 * torch.randn(n, K, h, w, generator=g), 1) for h, w in sizes]
    ew = torch.randn(gc, 1, 3, 3, generator=g) * 0.5
    wg = torch.randn(G, 128, 3, 3, generator=g) / 30
    bg = torch.randn(G, generator=g)
    dy = [torch.randn(n, G, h, w, generator=g) for h, w in sizes]
    d64 = lambda ts: [t.double() for t in ts]  # noqa: E731
    # push the hidden values away from the ReLU's kink (see the module docstring), in fp32 so that both sides read the same h_main
    for l in range(len(sizes)):
        hsum = hm[l].double() + F.conv2d(act[l].double()[:, 1:], ew.double(), None, padding=1, groups=G)
        near = hsum.abs() < 1e-3
        hm[l] = torch.where(near, hm[l] + torch.where(hsum >= 0, 2e-3, -2e-3).float(), hm[l])
    ref = _statement(d64(hm), d64(act), ew.double(), wg.double(), bg.double(), d64(dy), G)
    assert float(ref["hsum"].abs().min()) >= 9e-4
    mag = _statement([t.abs() for t in d64(hm)], [t.abs() for t in d64(act)], ew.double().abs(), wg.double().abs(),
                     bg.double().abs(), [t.abs() for t in d64(dy)], G)

    # device side: stacked weight with junk off the diagonal blocks (must be ignored), E as [G][9][128]
    ws = torch.randn(G, gc, 3, 3, generator=g)
    for c in range(G):
        ws[c, c * 128:(c + 1) * 128] = wg[c]
    h_d = _rows(hm).to(device).requires_grad_(True)
    a_d = _rows(act).to(device).requires_grad_(True)
    e_d = ew.reshape(G, 128, 9).permute(0, 2, 1).contiguous().to(device).requires_grad_(True)
    w_d = ws.to(device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    b_d = bg.to(device).requires_grad_(True)
    y = ops.gconv3x3_to1_act(h_d, w_d, b_d, a_d, e_d, shape, G, 1)
    assert y.shape == (M, ops.pad4(G)) and float(y.detach()[:, G:].abs().sum()) == 0
    y.backward(F.pad(_rows(dy), (0, ops.pad4(G) - G)).to(device))
    dw = w_d.grad.cpu()
    got = {"y": y.detach()[:, :G].cpu(), "dh": h_d.grad.cpu(), "da": a_d.grad.cpu(),
           "dE": e_d.grad.cpu().permute(0, 2, 1).reshape(gc, 1, 3, 3),
           "dw2": torch.stack([dw[c, c * 128:(c + 1) * 128] for c in range(G)], 0), "db2": b_d.grad.cpu()}
    for c in range(G):  # off-diagonal blocks of the stacked weight gradient: exact zeros
        off = dw[c].clone()
        off[c * 128:(c + 1) * 128] = 0
        assert float(off.abs().sum()) == 0
    assert float(got["da"][:, 0].abs().sum()) == 0  # the background column takes no part
    terms = {"y": 9 * 128 + 1 + 10, "dh": 9, "dw2": M + 10, "db2": M, "dE": M + 9, "da": 9 * 128 + 9}
    worst = {}
    for k, nterms in terms.items():
        err = (got[k].double() - ref[k]).abs()
        bound = nterms * U * mag[k]
        worst[k] = (float(err.max()), float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound).all()), (k, worst[k])
    print("G=%d %s (max |err|, max err / bound):" % (G, pyr), worst)


def _branches(dis, cf):
    return [getattr(dis, "classifier_cls_%d" % c) for c in range(cf)]


@pytest.mark.parametrize("channels_last", [True, False], ids=["channels_last", "contiguous"])
@pytest.mark.parametrize("cf", [8, 1])
def test_split_stacked_weights_equal_torch_construction_bitwise(device, cf, channels_last):
    """ops.cka_stacked_weights_split against w0[:, :, :C] / w0[:, :, C] of the stacked conv0 weights: the same bits forward,
    the same bits in every parameter gradient -- returned to autograd and accumulated into flat gradient buffers."""
    from scan_amd import ops
    from scan_amd.modeling.discriminator import FCOSDiscriminator_con
    torch.manual_seed(17)
    C, H = 256, 128
    dis = FCOSDiscriminator_con(num_convs=1, in_channels=C, num_classes=cf + 1).to(device)
    blocks = _branches(dis, cf)
    for b in blocks:
        for m in (b[0], b[2]):
            nn.init.normal_(m.weight, std=0.1)
            nn.init.normal_(m.bias, std=0.1)
            if not channels_last:
                m.weight.data = m.weight.data.contiguous()
    params = [p for b in blocks for p in (b[0].weight, b[0].bias, b[2].weight, b[2].bias)]

    def torch_form():
        w0 = torch.stack([b[0].weight for b in blocks], 0)  # [Cf, H, C + 1, 3, 3]
        main = w0[:, :, :C].reshape(cf * H, C, 3, 3)
        e = w0[:, :, C].reshape(cf, H, 9).permute(0, 2, 1)  # [Cf, 9, H]
        _, b1, w2, b2 = dis._stacked_weights_torch()
        return main, e, b1, w2, b2

    got = ops.cka_stacked_weights_split([(b[0], b[2]) for b in blocks], C, H)
    ref = torch_form()
    assert got[0].shape == (cf * H, C, 3, 3) and got[0].permute(0, 2, 3, 1).is_contiguous()
    assert got[1].shape == (cf, 9, H) and got[1].is_contiguous()
    for a, r in zip(got, ref):
        assert torch.equal(a, r)
    cot = [torch.randn_like(t) for t in got]
    g_ref = torch.autograd.grad(list(ref), params, cot)
    g_got = torch.autograd.grad(list(got), params, cot)
    for a, r in zip(g_got, g_ref):
        assert torch.equal(a, r)
    for p in params:  # parameters living in flat buffers: the backward adds into .grad and hands autograd nothing
        p.grad = torch.ones_like(p)
        p._scan_flat = True
    torch.autograd.backward(list(ops.cka_stacked_weights_split([(b[0], b[2]) for b in blocks], C, H)), cot)
    for p, r in zip(params, g_ref):
        assert torch.equal(p.grad, 1 + r)


def _module_case(device, cf, seed=5):
    from scan_amd import ops
    from scan_amd.modeling.discriminator import FCOSDiscriminator_con
    torch.manual_seed(seed)
    dis = FCOSDiscriminator_con(num_convs=1, in_channels=256, num_classes=cf + 1).to(device)
    for m in dis.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.normal_(m.weight, std=0.05)
    shape = ops.PyramidShape(2, [(6, 10)])
    feat = torch.randn(shape.rows, 256, device=device)
    act = torch.softmax(torch.randn(shape.rows, cf + 1, device=device), 1)
    return dis, shape, feat, act


def _module_run(dis, shape, feat, act, flat):
    """both losses, d feature, d act and every parameter gradient of one forward_pair (1 source + 1 target frame)"""
    f, a = feat.clone().requires_grad_(True), act.clone().requires_grad_(True)
    for p in dis.parameters():
        if flat:  # parameters re-homed into flat gradient buffers: the kernels accumulate into .grad in place
            p.grad = torch.zeros_like(p)
            p._scan_flat = True
        else:
            p.grad = None
            p._scan_flat = False
    ls, lt = dis.forward_pair(f, a, shape, 1)
    (ls + 2 * lt).backward()
    return [ls.detach(), lt.detach(), f.grad, a.grad] + [p.grad.clone() for p in dis.parameters()]


@pytest.mark.parametrize("flat", [False, True], ids=["autograd", "flat_buffers"])
@pytest.mark.parametrize("cf", [8, 1])
def test_discriminator_split_branch_equals_dense_branch(device, cf, flat, act_grads_path):
    """FCOSDiscriminator_con.forward_pair with CLS_SPLIT on against off (the dense conv over cat(x, act[1:])): the bar of
    test_discriminator_grouped_branch_equals_dense_branch for the same kind of comparison, 2e-4 of the reference's max"""
    from scan_amd import ops
    dis, shape, feat, act = _module_case(device, cf)
    res = []
    old = ops.CLS_SPLIT
    try:
        for flag in (True, False):
            ops.CLS_SPLIT = flag
            res.append(_module_run(dis, shape, feat, act, flat))
    finally:
        ops.CLS_SPLIT = old
        for p in dis.parameters():
            p._scan_flat = False
    assert res[0][3] is not None and float(res[1][3].abs().max()) > 0
    for a, b in zip(*res):
        assert (a - b).abs().max().item() <= 2e-4 * max(b.abs().max().item(), 1e-6), (a.shape, (a - b).abs().max().item())


@pytest.mark.parametrize("cf", [8, 1])
def test_discriminator_split_backward_is_bit_reproducible_in_deterministic_mode(device, cf, act_grads_path):
    from scan_amd import ops
    assert ops.CLS_SPLIT
    dis, shape, feat, act = _module_case(device, cf, seed=7)
    old = ops.set_deterministic(True)
    try:
        runs = [_module_run(dis, shape, feat, act, False) for _ in range(2)]
    finally:
        ops.set_deterministic(old)
    for a, b in zip(*runs):
        assert torch.equal(a, b), (a.shape, (a - b).abs().max().item())

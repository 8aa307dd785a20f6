"""GPU tests of the pyramid pack / unpack kernels (scan_amd/csrc/pyramid_pack.hip) through ops.pack_levels / ops.unpack_levels.

The op is a copy, so every comparison is torch.equal against the reference's flatten-and-concatenate restated here
(rpn/fcos/loss.py:191-202: permute(0, 2, 3, 1).reshape(-1, C) per level, torch.cat over the levels), zero-padded to Cs.

Shapes: N = 2 with levels 9x15 (135 pixels per image, 270 per level: tile boundaries inside the level), 5x7, 3x4, 1x2, 1x1 (levels
smaller than one 64-pixel tile), C in {1, 4, 9, 66, 130} (below one float4, exactly one, not a multiple of 4, just past one and
two 64-channel tiles); and N = 1, 8x8, C = 64: exactly one tile.  Each in three source layouts: NCHW-contiguous (LDS transpose
path), channels_last (row copy, float4 when C % 4 == 0) and the channel slice x[:, 1:] of each (strided, base off 16 bytes)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

PYRAMID = (2, [(9, 15), (5, 7), (3, 4), (1, 2), (1, 1)])
CASES = [PYRAMID + (c,) for c in (1, 4, 9, 66, 130)] + [(1, [(8, 8)], 64)]
LAYOUTS = ("nchw", "channels_last", "nchw_slice", "channels_last_slice")


def _levels(n, sizes, c, layout, device, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    out = []
    for h, w in sizes:
        extra = 1 if layout.endswith("slice") else 0
        x = torch.randn((n, c + extra, h, w), generator=g).to(device)
        if layout.startswith("channels_last"):
            x = x.contiguous(memory_format=torch.channels_last)
        out.append(x[:, 1:] if extra else x)
    return out


def _flatten_ref(levels, cs):
    c = levels[0].shape[1]
    rows = torch.cat([t.permute(0, 2, 3, 1).reshape(-1, c) for t in levels], 0)
    return torch.nn.functional.pad(rows, (0, cs - c))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n,sizes,c", CASES)
def test_pack_equals_flatten_and_unpack_inverts_it(device, n, sizes, c, layout):
    from scan_amd import _lib, ops
    levels = _levels(n, sizes, c, layout, device)
    if layout == "channels_last_slice":  # channel stride 1, but the base sits one float past a 16-byte boundary
        assert all(t.stride(1) == 1 and t.data_ptr() % 16 == 4 for t in levels)
    # the default pitch pad4(C), and an explicit wider one: C + 8 (from pad4(C) where C itself is no multiple of 4)
    for cs in (ops.pad4(c), ops.pad4(c) + 8):
        rows, shape = ops.pack_levels(levels, cs=cs)
        assert shape == ops.PyramidShape(n, sizes) and tuple(rows.shape) == (shape.rows, cs)
        assert torch.equal(rows, _flatten_ref(levels, cs))
        # the kernel writes EVERY element of its destination, padding columns included: NaN-filled, nothing survives
        dst = torch.full((shape.rows, cs), float("nan"), device=device)
        _lib.call("scan_pyramid_pack", ops._level_descs(levels), len(levels), n, c, ops._ptr(dst), cs, ops._stream())
        assert torch.equal(dst, rows)
        for fmt in (torch.contiguous_format, torch.channels_last):
            back = ops.unpack_levels(rows, shape, c, fmt)
            assert all(torch.equal(b, t) for b, t in zip(back, levels))
            assert all(b.is_contiguous(memory_format=fmt) for b in back)
        # unpack into NaN-filled level tensors of the SOURCE's strides: every element of every level is written
        outs = [torch.empty_strided(t.shape, t.stride(), device=device).fill_(float("nan")) for t in levels]
        _lib.call("scan_pyramid_unpack", ops._ptr(rows), cs, ops._level_descs(outs), len(outs), n, c, ops._stream())
        assert all(torch.equal(o, t) for o, t in zip(outs, levels))


@pytest.mark.parametrize("layout", ("nchw", "channels_last", "nchw_slice"))
@pytest.mark.parametrize("c", (9, 66))
def test_pack_and_unpack_are_each_other_s_gradient(device, c, layout):
    from scan_amd import ops
    n, sizes = PYRAMID
    bases = None
    if layout != "nchw_slice":
        levels = [t.requires_grad_(True) for t in _levels(n, sizes, c, layout, device)]
    else:  # gradients flow through the slice to the full tensors
        bases = [torch.randn((n, c + 1, h, w), device=device, requires_grad=True) for h, w in sizes]
        levels = [b[:, 1:] for b in bases]
    cs = ops.pad4(c)
    rows, shape = ops.pack_levels(levels)
    g = torch.randn((shape.rows, cs), device=device, generator=torch.Generator(device=device).manual_seed(1))
    rows.backward(g)
    want = ops.unpack_levels(g, shape, c, torch.contiguous_format)
    if bases is None:
        assert all(torch.equal(t.grad, w_) for t, w_ in zip(levels, want))
    else:
        assert all(torch.equal(b.grad[:, 1:], w_) and not b.grad[:, :1].any() for b, w_ in zip(bases, want))
    # and the other way round: d unpack = pack of the level gradients, whatever their layout; padding columns get zero
    r = torch.randn((shape.rows, cs), device=device, requires_grad=True)
    outs = ops.unpack_levels(r, shape, c, torch.channels_last)
    gl = _levels(n, sizes, c, layout, device, seed=2)
    torch.autograd.backward(outs, gl)
    assert torch.equal(r.grad, _flatten_ref(gl, cs))
    # a level without a gradient counts as zeros
    r2 = torch.randn((shape.rows, cs), device=device, requires_grad=True)
    outs = ops.unpack_levels(r2, shape, c)
    outs[1].backward(gl[1])
    z = [torch.zeros_like(t) for t in gl]
    z[1] = gl[1]
    assert torch.equal(r2.grad, _flatten_ref(z, cs))


def test_pyramid_levels_fast_path_and_its_guard(device):
    from scan_amd import ops
    n, sizes = PYRAMID
    shape = ops.PyramidShape(n, sizes)
    rows = torch.randn((shape.rows, 8), device=device)
    lv = ops.PyramidLevels(rows, shape)
    assert all(t.is_contiguous(memory_format=torch.channels_last) or min(t.shape[1:]) == 1 for t in lv)
    assert torch.equal(_flatten_ref(lv, 8), rows)  # the views ARE the levels of the matrix
    got, gshape = ops.pack_levels(lv)
    assert got.data_ptr() == rows.data_ptr() and got is rows and gshape == shape  # same storage: nothing was launched
    # another row pitch than the matrix has: the kernel
    wide, _ = ops.pack_levels(lv, cs=12)
    assert wide.data_ptr() != rows.data_ptr() and torch.equal(wide, _flatten_ref(lv, 12))
    # two elements swapped: the list no longer is the matrix -> the kernel, and the rows of the list as it now stands
    lv2 = ops.PyramidLevels(rows, shape)
    lv2[0], lv2[1] = lv2[1], lv2[0]
    got2, shape2 = ops.pack_levels(lv2)
    assert got2.data_ptr() != rows.data_ptr() and shape2.sizes[:2] == [sizes[1], sizes[0]]
    assert torch.equal(got2, torch.cat([rows[shape.row_off[1]:shape.row_off[2]], rows[:shape.row_off[1]], rows[shape.row_off[2]:]], 0))
    # ... also when the swapped levels have the same size (shape alone cannot tell)
    shape_eq = ops.PyramidShape(2, [(3, 4), (3, 4)])
    rows_eq = torch.randn((shape_eq.rows, 8), device=device)
    lv_eq = ops.PyramidLevels(rows_eq, shape_eq)
    lv_eq[0], lv_eq[1] = lv_eq[1], lv_eq[0]
    got_eq, _ = ops.pack_levels(lv_eq)
    assert got_eq.data_ptr() != rows_eq.data_ptr() and torch.equal(got_eq, torch.cat([rows_eq[24:], rows_eq[:24]], 0))
    # an element replaced by a clone: same values, other storage -> the kernel, same rows
    lv3 = ops.PyramidLevels(rows, shape)
    lv3[2] = lv3[2].clone()
    got3, _ = ops.pack_levels(lv3)
    assert got3.data_ptr() != rows.data_ptr() and torch.equal(got3, rows)
    # a plain list of the very same views is not a PyramidLevels: the kernel again
    got4, _ = ops.pack_levels(list(lv))
    assert got4.data_ptr() != rows.data_ptr() and torch.equal(got4, rows)
    # the views carry the gradient back into the matrix
    r = torch.randn((shape.rows, 8), device=device, requires_grad=True)
    lvg = ops.PyramidLevels(r, shape)
    gl = _levels(n, sizes, 8, "nchw", device, seed=3)
    torch.autograd.backward(list(lvg), gl)
    assert torch.equal(r.grad, _flatten_ref(gl, 8))

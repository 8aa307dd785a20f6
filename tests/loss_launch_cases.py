"""The cases of tests/test_gpu_loss_launch.py and tools/make_loss_parent_golden.py: the loss forwards of csrc/losses.hip, the
GIoU forward / backward and the plan targets of csrc/atss.hip and the smooth-L1 forward / backward of csrc/retina.hip, called
through the C ABI on inputs drawn from a seeded CPU generator or taken from the heads' fixtures.  run(case, device)
returns the raw bits of what a call wrote.  Ordered calls get a workspace of exactly the size their *_ordered_ws_floats query
gives, filled with NaN, and NaN-filled outputs: a block count or slot stride that does not match the launch ends in NaN or in
other bits.  Atomic calls add to zeroed outputs, from ONE workgroup (at most 2,048 work items): a single atomic onto a zeroed
word is order-free, so those bits are reproducible too."""
import ctypes
import zlib

import numpy as np
import torch

NAN = float("nan")

# (id, family, ordered, reduce_blocks or None, parameters).  Workgroups of the first stage in the comments.
CASES = [
    # ---- ordered entry points: more than one workgroup, so the grid and the slot stride decide the bits
    ("focal_c8", "focal", True, None, dict(M=2100, C=8, gamma=2.0)),             # <8, true>, float4, 3
    ("focal_c1", "focal", True, None, dict(M=9000, C=1, gamma=2.0)),             # <1, true>, aligned targets, 2
    ("focal_c3", "focal", True, None, dict(M=3001, C=3, gamma=1.5)),             # generic scalar (9,003 elements), 2
    ("iou", "iou", True, None, dict(P=5000, weighted=False)),                    # 3
    ("iou_w", "iou", True, None, dict(P=5000, weighted=True)),
    ("bce_4095", "bce", True, None, dict(M=4095)),                               # scalar, under the float4 threshold, 2
    ("bce_8200", "bce", True, None, dict(M=8200, weight=1)),                     # float4, 2
    ("bce_8200_shift", "bce", True, None, dict(M=8200, shift=True)),             # logits 4 bytes in: scalar, 5
    ("bce_8200_stride2", "bce", True, None, dict(M=8200, weight=2)),             # weight of stride 2: scalar, 5
    ("cka8", "cka", True, None, dict(M=3000, Cf=8)),                             # float4 kernel, 3
    ("cka8_shift", "cka", True, None, dict(M=3000, Cf=8, shift=True)),           # generic kernel, 2
    ("cka3", "cka", True, None, dict(M=5000, Cf=3)),                             # 3
    ("cka8_loss", "cka", True, None, dict(M=3000, Cf=8, loss=True)),
    ("cka8_shift_loss", "cka", True, None, dict(M=3000, Cf=8, shift=True, loss=True)),
    ("cka3_loss", "cka", True, None, dict(M=5000, Cf=3, loss=True)),
    ("sfl_k9", "sfl", True, None, dict(M=1500, K=9)),                            # 3
    ("sfl_k20", "sfl", True, None, dict(M=700, K=20)),                           # the 32-wide instance, 2
    ("focal_c8_rb2", "focal", True, 2, dict(M=2100, C=8, gamma=2.0)),            # capped to 2
    ("iou_rb2", "iou", True, 2, dict(P=5000, weighted=True)),                    # light: half the cap, 1
    ("giou", "giou", True, None, dict(P=5000)),                                  # 3
    # ---- atomic entry points: one workgroup per family and kernel form
    ("a_focal_c8", "focal", False, None, dict(M=200, C=8, gamma=2.0)),
    ("a_focal_c1", "focal", False, None, dict(M=200, C=1, gamma=2.0)),
    ("a_focal_c3", "focal", False, None, dict(M=201, C=3, gamma=1.5)),
    ("a_focal_elem", "focal", False, None, dict(M=3001, C=3, gamma=2.0, no_sum=True)),  # losses only: grid_for, no sum
    ("a_iou_w", "iou", False, None, dict(P=200, weighted=True)),
    ("a_bce", "bce", False, None, dict(M=200, weight=2)),
    ("a_bce_vec", "bce", False, None, dict(M=4100, weight=1)),                   # float4 form: 1,025 float4
    ("a_cka8", "cka", False, None, dict(M=200, Cf=8)),
    ("a_cka8_shift", "cka", False, None, dict(M=200, Cf=8, shift=True)),
    ("a_cka3", "cka", False, None, dict(M=200, Cf=3)),
    ("a_cka8_loss", "cka", False, None, dict(M=200, Cf=8, loss=True)),           # the only block is the finishing block
    ("a_cka3_loss", "cka", False, None, dict(M=200, Cf=3, loss=True)),
    ("a_sfl_k9", "sfl", False, None, dict(M=200, K=9)),
    ("a_sfl_k20", "sfl", False, None, dict(M=200, K=20)),
    ("a_giou", "giou", False, None, dict(P=200)),
    # ---- the heads' smooth-L1 (csrc/retina.hip); new cases go at the end: the seed of a case is 7000 + its index
    ("sl1_a9", "sl1", True, None, dict(A=9)),                                    # ordered, 2,322 anchors, 2
    ("a_sl1_a3", "sl1", False, None, dict(A=3)),                                 # atomic, 774 anchors, 1
    # ---- float outputs of the heads that no sum folds: backward gradients and the ATSS plan's targets
    ("sl1_bwd_a9", "sl1_bwd", True, None, dict(A=9)),
    ("giou_bwd", "giou_bwd", True, None, dict(P=5000)),
    ("atss_targets", "atss_targets", True, None, dict()),
]
IDS = [c[0] for c in CASES]


def _shift4(t):
    """the same values in a contiguous view that starts 4 bytes into its allocation"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32).copy()


def _crc(t):
    return np.array([zlib.crc32(t.detach().cpu().contiguous().numpy().tobytes())], dtype=np.uint32)


def _out(n, ordered, device):
    return torch.full((n,), NAN, device=device) if ordered else torch.zeros(n, device=device)


def _launch(base, fwd, ordered, ws_args, device, *args):
    """base + fwd with atomics, or its *_ordered twin on a NaN workspace of exactly the queried size"""
    from scan_amd import _lib, ops
    if ordered:
        n = _lib.query(base + "_ordered_ws_floats", *ws_args)
        assert n >= 1
        ws = torch.full((n,), NAN, device=device)
        _lib.call(base + fwd + "_ordered", *args, ops._ptr(ws), ops._stream())
    else:
        _lib.call(base + fwd, *args, ops._stream())
    torch.cuda.synchronize()


def _focal(device, ordered, seed, M, C, gamma, no_sum=False):
    from scan_amd.ops import _ptr
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, C, generator=g) * 3).to(device)
    t = torch.randint(-1, C + 1, (M,), generator=g).to(torch.int32).to(device)
    assert t.data_ptr() % 16 == 0
    res = {}
    for want in ((True,) if no_sum else (False, True)):  # the sum alone, then the sum beside the element losses
        losses = torch.full((M, C), NAN, device=device) if want else None
        s = None if no_sum else _out(1, ordered, device)
        _launch("scan_sigmoid_focal_loss", "_forward", ordered, (M, C), device, _ptr(x), _ptr(t), M, C, gamma, 0.25, _ptr(losses),
                _ptr(s))
        if s is not None:
            res["sum_with_losses" if want else "sum"] = _bits(s)
        if want:
            res["losses_crc32"] = _crc(losses)
    return res


def _iou(device, ordered, seed, P, weighted):
    from scan_amd.ops import _ptr
    g = torch.Generator().manual_seed(seed)
    pred = (torch.rand(P, 4, generator=g) * 20 + 0.1).to(device)
    target = (torch.rand(P, 4, generator=g) * 20 + 0.1).to(device)
    w = (torch.rand(P, generator=g) + 0.05).to(device) if weighted else None
    out = _out(2, ordered, device)
    _launch("scan_iou_loss", "_forward", ordered, (P,), device, _ptr(pred), _ptr(target), _ptr(w), P, _ptr(out))
    return {"out2": _bits(out)}


def _bce(device, ordered, seed, M, weight=0, shift=False):
    """weight: 0 = none (and a constant target), else its stride"""
    from scan_amd.ops import _ptr
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, generator=g) * 4).to(device)
    if shift:
        x = _shift4(x)
    t = torch.rand(M, generator=g).to(device) if weight else None
    w = (torch.rand(M * weight, generator=g) + 0.05).to(device) if weight else None
    out = _out(2, ordered, device)
    _launch("scan_bce_logits", "_forward", ordered, (M,), device, _ptr(x), _ptr(t), 1.0, _ptr(w), weight, M, _ptr(out))
    return {"out2": _bits(out)}


def _cka(device, ordered, seed, M, Cf, shift=False, loss=False):
    from scan_amd.ops import _ptr
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, Cf, generator=g) * 3).to(device)
    if shift:
        x = _shift4(x)
    act = torch.softmax(torch.randn(M, Cf + 1, generator=g), 1).to(device)
    out = _out(2 * Cf + (2 if loss else 0), ordered, device)  # forward_loss: the sums, the ticket word, the loss
    if loss:
        out[2 * Cf] = 0.0  # the ordered form leaves the ticket word alone
    _launch("scan_cka_bce", "_forward_loss" if loss else "_forward", ordered, (M, Cf), device, _ptr(x), _ptr(act), M, Cf, 1.0,
            _ptr(out))
    return {"out": _bits(out)}


def _sfl(device, ordered, seed, M, K):
    from scan_amd.ops import _ptr
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(M, K, generator=g) * 2).to(device)
    lab = torch.randint(0, K, (M,), generator=g).to(device)
    out = _out(1, ordered, device)
    _launch("scan_softmax_focal", "_forward", ordered, (M,), device, _ptr(z), _ptr(lab), M, K, 2.0, _ptr(out))
    return {"sum": _bits(out)}


def _giou_inputs(device, P):
    """P rows drawn with repetition from the 1,364 rows of the 128x256 pyramid of tests/atss_ref.py with two images; the shape
    is returned too: it owns the descriptor the first argument points to"""
    import atss_ref as R
    from scan_amd import ops
    pred, target, rows, weight = (t.to(device) for t in R.giou_inputs(P, "generic"))
    shape = ops.PyramidShape(2, R.SIZES_128x256)
    geo = (shape.ref(), (ctypes.c_int32 * shape.n_levels)(*R.STRIDES), (ctypes.c_float * shape.n_levels)(*R.SIZES))
    return shape, geo + (ops._ptr(pred), ops._ptr(target), ops._ptr(rows), ops._ptr(weight), P), (pred, target, rows, weight)


def _giou(device, ordered, seed, P):
    from scan_amd.ops import _ptr
    shape, args, keep = _giou_inputs(device, P)
    out = _out(2, ordered, device)
    _launch("scan_atss_giou", "_forward", ordered, (P,), device, *args, _ptr(out))
    return {"out2": _bits(out)}


def _giou_bwd(device, ordered, seed, P):
    """the gradient of the giou case's inputs under an upstream gradient of 0.75"""
    from scan_amd import _lib
    from scan_amd.ops import _ptr, _stream
    shape, args, keep = _giou_inputs(device, P)
    g = torch.full((1,), 0.75, device=device)
    d = torch.full((P, 4), NAN, device=device)
    _lib.call("scan_atss_giou_backward", *args, _ptr(g), _ptr(d), _stream())
    torch.cuda.synchronize()
    assert torch.isfinite(d).all()
    return {"d_pred_crc32": _crc(d)}


_SL1_SEED = 7777  # sl1_a9 and sl1_bwd_a9 share their inputs


def _sl1_inputs(device, A):
    """the 64x96 pyramid of tests/retinanet_ref.py with the two images and boxes of the retinanet_64x96 fixture, A = 9 (the
    fixture's cell anchors) or 3 (one scale per octave); the plan is retinanet.build_plan's; bbox_reg is the first 4 A columns
    of a seeded [M, 4 A + 4] matrix, read in place through its pitch"""
    import os
    import retinanet_ref as R
    from scan_amd import ops
    from scan_amd.modeling import retinanet
    f = R.load_case(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"), "retinanet_64x96")
    assert f["N"] == 2 and f["sizes"] == R.SIZES_64x96
    shape = ops.PyramidShape(2, R.SIZES_64x96)
    cells = retinanet.cell_anchors() if A == 9 else retinanet.cell_anchors(scales_per_octave=1)
    assert cells.shape[1] == A
    plan = retinanet.build_plan(shape, f["targets"], device, cells=cells)
    assert plan.n_pos > 0 and int((plan.labels_i32 > 0).sum()) == plan.n_pos
    g = torch.Generator().manual_seed(_SL1_SEED + A)
    wide = torch.randn(shape.rows, 4 * A + 4, generator=g).to(device)
    cells_d = retinanet.device_cells(cells, device)
    strides = (ctypes.c_int32 * shape.n_levels)(*R.STRIDES)
    args = (shape.ref(), strides, ops._ptr(cells_d), A, ops._ptr(plan.boxes), plan.boxes.shape[1], ops._ptr(plan.labels_i32),
            ops._ptr(plan.matched), ops._ptr(wide), 4 * A + 4, 0.11)
    return shape, args, (plan, wide, cells_d)


def _sl1(device, ordered, seed, A):
    from scan_amd import _lib
    from scan_amd.ops import _ptr
    shape, args, keep = _sl1_inputs(device, A)
    n = shape.rows * A
    if ordered:
        assert _lib.query("scan_retina_smooth_l1_ordered_ws_floats", n) >= 2  # more than one workgroup
    else:
        assert n <= 2048  # one workgroup
    res = {}
    for want in (True, False):  # the sum beside the targets, then the sum alone
        tg = torch.full((n, 4), NAN, device=device) if want else None
        s = _out(1, ordered, device)
        _launch("scan_retina_smooth_l1", "_forward", ordered, (n,), device, *args, _ptr(tg), _ptr(s))
        res["sum_with_targets" if want else "sum"] = _bits(s)
        if want:
            assert torch.isfinite(tg).all()
            res["targets_crc32"] = _crc(tg)
    return res


def _sl1_bwd(device, ordered, seed, A):
    """d_pred through a pitch of 4 A + 4 under an upstream gradient of 0.75: the 4 A columns are written, the rest is not"""
    from scan_amd import _lib
    from scan_amd.ops import _ptr, _stream
    shape, args, keep = _sl1_inputs(device, A)
    g = torch.full((1,), 0.75, device=device)
    d = torch.full((shape.rows, 4 * A + 4), NAN, device=device)
    _lib.call("scan_retina_smooth_l1_backward", *args, _ptr(g), _ptr(d), 4 * A + 4, _stream())
    torch.cuda.synchronize()
    assert torch.isfinite(d[:, :4 * A]).all() and torch.isnan(d[:, 4 * A:]).all()
    assert int((d[:, :4 * A] != 0).sum()) > 0
    return {"d_pred_crc32": _crc(d[:, :4 * A])}


def _atss_targets(device, ordered, seed):
    """the float targets of modeling.atss.build_plan on the boxes of the atss_64x96 fixture"""
    import os
    import atss_ref as R
    from scan_amd import ops
    from scan_amd.modeling import atss
    f = R.load_case(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"), "atss_64x96")
    shape = ops.PyramidShape(f["N"], f["sizes"])
    plan = atss.build_plan(shape, f["targets"], device, R.STRIDES, [float(a) for a in f["anchor_sizes"]], int(f["topk"]))
    torch.cuda.synchronize()
    assert plan.n_pos > 0 and plan.reg_pos.shape == (plan.n_pos, 4) and plan.ctr_pos.shape == (plan.n_pos,)
    return {"reg_pos": _bits(plan.reg_pos).reshape(-1), "ctr_pos": _bits(plan.ctr_pos), "pos_inds_crc32": _crc(plan.pos_inds)}


_FAMILY = {"focal": _focal, "iou": _iou, "bce": _bce, "cka": _cka, "sfl": _sfl, "giou": _giou, "giou_bwd": _giou_bwd,
           "sl1": _sl1, "sl1_bwd": _sl1_bwd, "atss_targets": _atss_targets}


def run(case_id, device):
    """{name: uint32 array} -- the raw bits the calls of one case wrote"""
    from scan_amd import _lib
    i = IDS.index(case_id)
    _, family, ordered, reduce_blocks, params = CASES[i]
    old = _lib.query("scan_tune", b"reduce_blocks", reduce_blocks) if reduce_blocks is not None else None
    try:
        return _FAMILY[family](device, ordered, 7000 + i, **params)
    finally:
        if old is not None:
            _lib.query("scan_tune", b"reduce_blocks", old)

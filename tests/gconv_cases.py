"""The cases of tests/test_gpu_gconv_parent_bits.py and tools/make_gconv_parent_golden.py: every entry point of csrc/gconv.hip,
called through the C ABI on inputs drawn from a seeded CPU generator.  run(case, device) returns, per output array, the crc32
of its bytes (and the raw bits of arrays of at most 64 floats).  Outputs and the workspace (of exactly the queried size) start as
NaN, so an element a launch does not write -- or a workspace laid out differently from how it was sized -- shows; the
accumulate = 1 target starts at 0.5.  None of these paths has atomics: the bits follow from the kernels' arithmetic, the grid
and the slab order alone.

Pyramids (2 images each):
  p17  [(17, 17)], 578 rows: the lane-mapped and act slabs get 37 workgroups (18 runs of 2 and a last run of 1), the generic
       slab 40 strides (20 runs of 2) -- the smallest size at which the first reduction level adds more than one partial
  p57  [(5, 7), (3, 4)], 94 rows: partial workgroups, an image seam and a level seam"""
import zlib

import numpy as np
import torch

NAN = float("nan")
N_IMAGES = 2
PYRAMIDS = {"p17": [(17, 17)], "p57": [(5, 7), (3, 4)]}

FMA_OPS = ("any_forward", "any_backward", "any_dgrad", "any_wgrad", "act_forward", "act_backward_grads", "act_backward_all")
MFMA_OPS = ("forward", "backward", "forward_bits", "backward_bits")
GENERIC_OPS = ("any_forward", "any_backward", "any_backward_nomask", "any_dgrad", "any_wgrad")

# (id, pyramid, G, gconv_mfma, op)
CASES = []
for _p in PYRAMIDS:
    for _g in (1, 2, 4, 8):  # pixel slots 8, 4, 2, 1
        CASES += [("%s_g%d_fma_%s" % (_p, _g, op), _p, _g, 0, op) for op in FMA_OPS]
    for _g in (2, 8):
        CASES += [("%s_g%d_mfma_%s" % (_p, _g, op), _p, _g, 1, op) for op in MFMA_OPS]
    for _g in (3, 31):
        CASES += [("%s_g%d_generic_%s" % (_p, _g, op), _p, _g, 0, op) for op in GENERIC_OPS]
IDS = [c[0] for c in CASES]


def _put(res, name, t):
    a = t.detach().cpu().contiguous().numpy()
    res[name + "_crc32"] = np.array([zlib.crc32(a.tobytes())], dtype=np.uint32)
    if a.size <= 64:
        res[name] = a.reshape(-1).view(np.uint32).copy()


def run(case_id, device):
    """{name: uint32 array} -- crc words (and short arrays) of what the calls of one case wrote"""
    from scan_amd import _lib, ops
    i = IDS.index(case_id)
    _, pyr, G, mfma, op = CASES[i]
    gen = torch.Generator().manual_seed(9100 + 64 * list(PYRAMIDS).index(pyr) + G)  # one set of inputs per (pyramid, G)
    shape = ops.PyramidShape(N_IMAGES, PYRAMIDS[pyr])
    M, gc, ns, K = shape.rows, G * 128, ops.pad4(G), G + 1
    x = torch.randn(M, gc, generator=gen).to(device)  # signed: the ReLU mask cuts about half
    w = (torch.randn(G, 9, gc, generator=gen) / 30).to(device)  # junk off the diagonal blocks: never read
    bias = torch.randn(G, generator=gen).to(device)
    dy = torch.randn(M, ns, generator=gen).to(device)
    act = torch.softmax(torch.randn(M, K, generator=gen), 1).to(device)  # class g in column 1 + g
    e = (torch.randn(G, 9, 128, generator=gen) / 3).to(device)
    P, st, d = ops._ptr, ops._stream(), shape.ref()

    def nan(*size, dtype=torch.float32):
        return torch.full(size, NAN, device=device).view(dtype)

    def ws(act_layout=False):
        return nan(_lib.query("scan_gconv3x3_to1_act_ws_floats" if act_layout else "scan_gconv3x3_to1_ws_floats", d, G, 128))

    def call(name, *args):
        _lib.call("scan_gconv3x3_to1_" + name, *args, st)
        torch.cuda.synchronize()

    res = {}
    old = _lib.query("scan_tune", b"gconv_mfma", mfma)
    try:
        if op in ("any_forward", "forward"):
            y = nan(M, ns)
            call(op, P(x), d, G, 128, P(w), P(bias), P(y), ns, P(ws()))
            _put(res, "y", y)
        elif op in ("any_backward", "any_backward_nomask", "backward"):
            dx, dw = nan(M, gc), nan(G, 9, gc)
            call(op.replace("_nomask", ""), P(x), P(dy), ns, d, G, 128, P(w), int(not op.endswith("nomask")), P(dx), P(dw), 0,
                 P(ws()))
            _put(res, "dx", dx)
            _put(res, "dw", dw)
        elif op == "any_dgrad":
            dx = nan(M, gc)
            call(op, P(dy), ns, d, G, 128, P(w), None, P(dx))
            _put(res, "dx", dx)
        elif op == "any_wgrad":
            dw = torch.full((G, 9, gc), 0.5, device=device)
            call(op, P(x), P(dy), ns, d, G, 128, P(dw), 1, P(ws()))
            _put(res, "dw", dw)
        elif op in ("forward_bits", "backward_bits"):
            y, bits = nan(M, ns), nan(M * G * 4, dtype=torch.int32)
            call("forward_bits", P(x), d, G, 128, P(w), P(bias), P(y), ns, P(ws()), P(bits))
            if op == "forward_bits":
                _put(res, "y", y)
                _put(res, "bits", bits)
            else:
                dx, dw = nan(M, gc), nan(G, 9, gc)
                call(op, P(x), P(dy), ns, d, G, 128, P(w), P(bits), P(dx), P(dw), 0, P(ws()))
                _put(res, "dx", dx)
                _put(res, "dw", dw)
        elif op == "act_forward":
            y = nan(M, ns)
            call(op, P(x), d, G, 128, P(w), P(bias), P(act), K, 1, P(e), P(y), ns, P(ws(True)))
            _put(res, "y", y)
        elif op == "act_backward_grads":
            dx, dw, da, de = nan(M, gc), nan(G, 9, gc), nan(M, K), nan(G, 9, 128)
            call("act_backward", P(x), P(dy), ns, d, G, 128, P(w), P(act), K, 1, P(e), P(dx), P(dw), 0, P(ws(True)))
            call("act_grads", P(dx), d, G, 128, P(act), K, 1, P(e), P(da), K, 1, P(de), 0, P(ws(True)))
            for k, v in (("dx", dx), ("dw", dw), ("da", da), ("de", de)):
                _put(res, k, v)
        elif op == "act_backward_all":
            dx, dw, da, de = nan(M, gc), nan(G, 9, gc), nan(M, K), nan(G, 9, 128)
            call(op, P(x), P(dy), ns, d, G, 128, P(w), P(act), K, 1, P(e), P(dx), P(dw), P(da), K, 1, P(de), 0, P(ws(True)))
            for k, v in (("dx", dx), ("dw", dw), ("da", da), ("de", de)):
                _put(res, k, v)
        else:
            raise KeyError(op)
    finally:
        _lib.query("scan_tune", b"gconv_mfma", old)
    return res

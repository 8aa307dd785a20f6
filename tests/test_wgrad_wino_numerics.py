"""CPU pins of the Winograd F(2,3)-across-rows arithmetic of the three-piece 3x3 weight gradient (csrc/conv_wgrad.hip WINO,
tools/wino_numerics.py --wgrad): the component form reproduces the three row taps exactly, and the emulated rounding (fp32
transforms, three-piece split, six products smallest first in a per-step temporary, fp32 slabs, fp64 reduce with G^T) is no
further from fp64 than an fp32 FMA chain on every input class -- the gate the kernel was built against, and what
tests/test_gpu_kernels.py::test_wgrad_full_size_elementwise part (b) asks of the real kernel.  profiles/r08_wgrad_wino_numerics.txt is
the table at full chain length (1024 samples); it is re-checked here line by line."""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import wino_numerics as wn  # noqa: E402


def test_component_form_is_the_adjoint_of_f23():
    """M0..M3 and G^T as the kernel and the reduction apply them equal e0 d_ky + e1 d_(ky+1)"""
    rs = np.random.RandomState(0)
    e0, e1 = rs.standard_normal((2, 1000))
    d0, d1, d2, d3 = rs.standard_normal((4, 1000))
    m = [e0 * (d0 - d2), (e0 + e1) * (d1 + d2), (e0 - e1) * (d2 - d1), (-e1) * (d1 - d3)]
    got = [m[0] + 0.5 * (m[1] + m[2]), 0.5 * (m[1] - m[2]), m[3] + 0.5 * (m[1] + m[2])]
    ref = [e0 * d0 + e1 * d1, e0 * d1 + e1 * d2, e0 * d2 + e1 * d3]
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12)
    # the same thing from the transform matrices of the forward form: dg = G^T [(A e) .* (B^T d)]
    A = wn.AT.T
    via = wn.G.T @ ((A @ np.stack([e0, e1])) * (wn.BT @ np.stack([d0, d1, d2, d3])))
    np.testing.assert_allclose(via, ref, rtol=0, atol=1e-12)


def test_emulated_wgrad_winograd_error_not_above_fp32_chain():
    """a short run of the emulation (one slab of 128 pair chunks, 4,096 pixels, where the bench's slabs have 171): the gate on
    every input class"""
    for i, cls in enumerate(wn.WGRAD_CLASSES):
        r = wn.emulate_wgrad(cls, 96, seed=100 + i, H=16, W=512)
        assert r["wino"][0] <= r["fp32"][0] and r["wino"][1] <= r["fp32"][1], (cls, r)
        # and in the neighbourhood of today's direct arithmetic (both are a few fp32 roundings of the result)
        assert r["wino"][0] <= 1.5 * r["direct"][0], (cls, r)


def test_recorded_table_is_what_the_tool_prints():
    """the first row of profiles/r08_wgrad_wino_numerics.txt regenerated as the tool's main() does it (1024 samples, seed 0): the
    emulation is deterministic, so the figures agree to the four digits the table prints"""
    path = os.path.join(ROOT, "profiles", "r08_wgrad_wino_numerics.txt")
    row = [l for l in open(path) if l.startswith("gauss")][0]
    assert wn.wgrad_table(1024, 0, classes=("gauss",))[0] == row.rstrip("\n")


def test_recorded_table_passes_the_gate():
    path = os.path.join(ROOT, "profiles", "r08_wgrad_wino_numerics.txt")
    rows = [l for l in open(path) if not l.startswith("#") and l.strip()]
    assert [l.split()[0] for l in rows] == list(wn.WGRAD_CLASSES)
    for l in rows:
        rms = re.search(r"rms fp32 (\S+) direct (\S+) wino (\S+)", l)
        mx = re.search(r"max fp32 (\S+) direct (\S+) wino (\S+)", l)
        f32_rms, _, w_rms = map(float, rms.groups())
        f32_max, _, w_max = map(float, mx.groups())
        assert w_rms <= f32_rms and w_max <= f32_max, l

"""CPU pins of the Winograd F(2,3) arithmetic of the three-piece 3x3 convs (csrc/conv_fwd.hip WINO, tools/wino_numerics.py):
the transform matrices reproduce the direct 3-tap correlation, and the emulated rounding of the Winograd bf16x6 path stays
below that of an fp32 FMA chain (the numerics gate the kernel was built against)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import wino_numerics as wn  # noqa: E402


def test_transform_matrices_are_f23():
    np.testing.assert_array_equal(wn.BT, [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]])
    np.testing.assert_array_equal(wn.G, [[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]])
    np.testing.assert_array_equal(wn.AT, [[1, 1, 1, 0], [0, 1, -1, -1]])
    rs = np.random.RandomState(0)
    d, g = rs.standard_normal((100, 4)), rs.standard_normal((100, 3))
    y = np.einsum("jk,sk->sj", wn.AT, np.einsum("jk,sk->sj", wn.G, g) * np.einsum("jk,sk->sj", wn.BT, d))
    direct = np.stack([(d[:, 0:3] * g).sum(1), (d[:, 1:4] * g).sum(1)], 1)
    np.testing.assert_allclose(y, direct, rtol=0, atol=1e-12)


def test_emulated_winograd_error_below_fp32_chain():
    r = wn.emulate(256, 256, seed=1)
    # measured at 4096 samples on every CONV_ERR_CASES channel count: wino 0.33-0.37x, direct 0.43-0.47x of the fp32 chain
    assert r["wino"][0] <= 0.6 * r["fp32"][0], r
    assert r["wino"][0] <= 1.0 * r["direct"][0], r

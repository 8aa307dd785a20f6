"""csrc/gconv.hip shares its device helpers and the tap-sum loop between the lane-mapped and the generic kernels, has one gather
and one reduce kernel, and one host layer for the workspace layout, the slab grid, the slab reduction and the gather.
tests/golden/gconv_parent.npz holds what the build before those were folded wrote for the cases of tests/gconv_cases.py (tools/make_gconv_parent_golden.py recorded it on
an MI355X): every case must reproduce it bit for bit -- the arithmetic, the order of the additions, the grids and the slab order
are the parent's."""
import os

import numpy as np
import pytest

import gconv_cases as C

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gconv_parent.npz")


@pytest.fixture(scope="module")
def parent():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def test_golden_holds_every_case_and_no_other(parent):
    assert sorted({k.split("/")[0] for k in parent}) == sorted(C.IDS)


@pytest.mark.parametrize("case_id", C.IDS)
def test_gconv_reproduces_the_parent_build(device, parent, case_id):
    got = C.run(case_id, device)
    want = {k.split("/", 1)[1]: v for k, v in parent.items() if k.split("/")[0] == case_id}
    assert sorted(got) == sorted(want)
    for k in sorted(got):
        print("%s/%s: %s (parent %s)" % (case_id, k, got[k], want[k]))
        assert got[k].dtype == np.uint32 and np.array_equal(got[k], want[k]), (case_id, k)

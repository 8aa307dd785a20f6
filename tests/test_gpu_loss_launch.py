"""The host launch layer of the loss reductions (csrc/losses.hip, and the GIoU forward of csrc/atss.hip) picks the kernel form,
the grid and the workspace stride; the kernels' bits follow from those alone.  tests/golden/loss_sums_parent.npz holds what the
build before that layer was folded into one launcher per loss wrote for the cases of tests/loss_launch_cases.py
(tools/make_loss_parent_golden.py recorded it on an MI355X): every case must reproduce it bit for bit.  The heads' cases
(smooth-L1 of csrc/retina.hip, the GIoU backward and the plan targets of csrc/atss.hip) were recorded the same way on the build
before their select, IoU and ordered-sum helpers moved to csrc/common.h and csrc/boxes.h; every array recorded earlier came back
identical then.

Ordered entry points at the smallest shapes with more than one workgroup on every kernel form (and under reduce_blocks = 2);
atomic entry points from one workgroup, where the sum is order-free.  Atomic sums of several workgroups are not reproducible
by design: tests/test_gpu_losses.py holds them to fp64 bars in both modes."""
import os

import numpy as np
import pytest

import loss_launch_cases as L

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_sums_parent.npz")


@pytest.fixture(scope="module")
def parent():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def test_golden_holds_every_case_and_no_other(parent):
    assert sorted({k.split("/")[0] for k in parent}) == sorted(L.IDS)


@pytest.mark.parametrize("case_id", L.IDS)
def test_loss_launch_reproduces_the_parent_build(device, parent, case_id):
    got = L.run(case_id, device)
    want = {k.split("/", 1)[1]: v for k, v in parent.items() if k.split("/")[0] == case_id}
    assert sorted(got) == sorted(want)
    for k in sorted(got):
        print("%s/%s: %s (parent %s)" % (case_id, k, got[k].view(np.float32) if "crc" not in k else got[k],
                                         want[k].view(np.float32) if "crc" not in k else want[k]))
        assert got[k].dtype == np.uint32 and np.array_equal(got[k], want[k]), (case_id, k)
        assert "crc" in k or np.isfinite(got[k].view(np.float32)).all(), (case_id, k)  # an unwritten slot would have left NaN

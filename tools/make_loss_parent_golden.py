#!/usr/bin/env python3
"""Records tests/golden/loss_sums_parent.npz: the raw bits the loss forwards write for the cases of tests/loss_launch_cases.py,
on an MI355X, with the build whose bits tests/test_gpu_loss_launch.py is to pin (run it on that build, once).

    python tools/make_loss_parent_golden.py [--out tests/golden/loss_sums_parent.npz]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "loss_sums_parent.npz"))
    a = ap.parse_args()
    import torch
    import loss_launch_cases as L
    dev = torch.device("cuda:0")
    out = {}
    for cid in L.IDS:
        first, again = L.run(cid, dev), L.run(cid, dev)
        for k, v in first.items():
            assert np.array_equal(v, again[k]), "%s/%s is not reproducible on this build" % (cid, k)
            out["%s/%s" % (cid, k)] = v
            print("%s/%s" % (cid, k), v if "crc" in k else v.view(np.float32))
    np.savez_compressed(a.out, **out)
    print("%s: %d arrays of %d cases" % (a.out, len(out), len(L.IDS)))


if __name__ == "__main__":
    main()

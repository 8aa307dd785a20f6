#!/usr/bin/env python3
"""Records tests/golden/gconv_parent.npz: crc words (and short arrays) of what the grouped class-branch conv entry points write
for the cases of tests/gconv_cases.py, on an MI355X, with the build whose bits tests/test_gpu_gconv_parent_bits.py is to pin
(run it on that build, once).  Every case runs twice; two runs that differ are refused (none of these paths has atomics).

    python tools/make_gconv_parent_golden.py [--out tests/golden/gconv_parent.npz]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "gconv_parent.npz"))
    a = ap.parse_args()
    import torch
    import gconv_cases as C
    dev = torch.device("cuda:0")
    out = {}
    for cid in C.IDS:
        first, again = C.run(cid, dev), C.run(cid, dev)
        assert sorted(first) == sorted(again), cid
        for k, v in first.items():
            assert np.array_equal(v, again[k]), "%s/%s is not reproducible on this build" % (cid, k)
            out["%s/%s" % (cid, k)] = v
            print("%s/%s" % (cid, k), v if "crc" in k else v.view(np.float32))
    np.savez_compressed(a.out, **out)
    print("%s: %d arrays of %d cases" % (a.out, len(out), len(C.IDS)))


if __name__ == "__main__":
    main()

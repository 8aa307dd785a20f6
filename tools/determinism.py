"""Run-to-run reproducibility of the training step: five fresh two-iteration runs (serial, serial, overlapped, overlapped,
serial -- the shape of tests/test_gpu_model.py::test_stream_overlap_is_race_free) and, per parameter group, the number of
distinct bit patterns among their final parameters.

    python tools/determinism.py --deterministic 1     # exit status 1 if any two runs differ
    python tools/determinism.py --deterministic 0     # the default path: reports its noise, always exits 0
"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from scan_amd import engine, ops, synth  # noqa: E402


def run(dev, overlap):
    model = engine.build_model(9, device=dev, attn_dropout=0.0)
    engine.load_procedural_weights(model)
    tr = engine.Trainer(model)
    if not overlap:
        tr.dis_streams = {}
        tr.overlap_target = False
    s = synth.synth_images(2, 256, 512, 11).to(dev)
    t = synth.synth_images(2, 256, 512, 12).to(dev)
    tg = synth.synth_targets(2, 256, 512, 8, 8, 13)
    for _ in range(2):
        tr.step(s, tg, t)
    torch.cuda.synchronize()
    return {k: g.flat_p.clone() for k, g in tr.groups.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--deterministic", type=int, choices=(0, 1), default=0,
                    help="1: ordered reductions (scan_tune deterministic), any difference between runs is an error")
    args = ap.parse_args()
    dev = torch.device("cuda")
    old = ops.set_deterministic(bool(args.deterministic))
    try:
        runs = [(name, run(dev, name == "overlap")) for name in ("serial", "serial", "overlap", "overlap", "serial")]
    finally:
        ops.set_deterministic(old)
    worst = 0
    print("deterministic=%d: distinct bit patterns over %d runs (%s)" % (args.deterministic, len(runs), ", ".join(n for n, _ in runs)))
    for k in runs[0][1]:
        digests = [hashlib.sha1(r[k].cpu().numpy().tobytes()).hexdigest() for _, r in runs]
        spread = max(float((runs[0][1][k] - r[k]).abs().max()) for _, r in runs)
        n = len(set(digests))
        worst = max(worst, n)
        print("  %-14s %d   (largest difference from run 0: %.3e)" % (k, n, spread))
    if args.deterministic and worst > 1:
        print("FAIL: runs differ with the ordered reductions on")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())

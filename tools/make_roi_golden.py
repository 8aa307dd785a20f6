"""Writes tests/golden/roi_levels.json: boxes and the FPN levels the REFERENCE's own LevelMapper (modeling/poolers.py:11-42)
gives them.  Runs on a CPU machine that has the reference checkout (oracle/ref_harness.py); the fixture holds data only.

    python tools/make_roi_golden.py

Every case holds boxes whose sqrt(area) is exactly 112, 224 and 448 (the level boundaries of the canonical scale 224 at
level 4), boxes one coordinate unit to either side of them, tiny and huge boxes (clamped to k_min / k_max) and random ones.
Coordinates are stored as the exact values of their fp32 numbers."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness  # noqa: E402

CASES = (("p2_p4", (0.25, 0.125, 0.0625)), ("p2_p5", (0.25, 0.125, 0.0625, 0.03125)), ("p3_p7", (1 / 8, 1 / 16, 1 / 32, 1 / 64, 1 / 128)),
         ("single", (1 / 16,)))


def boxes_for(seed):
    rs = np.random.RandomState(seed)
    out = []
    for side in (112, 224, 448, 896):  # (x2 - x1 + 1) = side: sqrt(area) == side exactly
        for d in (-1, 0, 1):
            out.append([3.0, 5.0, 3.0 + side - 1 + d, 5.0 + side - 1 + d])
            out.append([10.0, 20.0, 10.0 + 2 * side - 1, 20.0 + side / 2 - 1 + d])  # the same area from a 4 : 1 box
    out += [[0.0, 0.0, 0.0, 0.0], [5.5, 5.5, 6.0, 6.25], [0.0, 0.0, 4000.0, 3000.0], [7.0, 7.0, 2.0, 2.0]]
    for _ in range(40):
        c = rs.uniform(0, 1000, 2)
        wh = np.exp(rs.uniform(np.log(4), np.log(1500), 2))
        out.append([c[0] - wh[0] / 2, c[1] - wh[1] / 2, c[0] + wh[0] / 2, c[1] + wh[1] / 2])
    return torch.tensor(out, dtype=torch.float32)


def main():
    ref_harness.setup()
    from fcos_core.modeling.poolers import LevelMapper
    from fcos_core.structures.bounding_box import BoxList
    cases = {}
    for i, (name, scales) in enumerate(CASES):
        # modeling/poolers.py:74-76
        k_min = -torch.log2(torch.tensor(scales[0], dtype=torch.float32)).item()
        k_max = -torch.log2(torch.tensor(scales[-1], dtype=torch.float32)).item()
        boxes = boxes_for(100 + i)
        half = len(boxes) // 2  # two box lists, as a batch of two images gives
        lists = [BoxList(boxes[:half], (4096, 4096), mode="xyxy"), BoxList(boxes[half:], (4096, 4096), mode="xyxy")]
        levels = LevelMapper(k_min, k_max)(lists)
        cases[name] = dict(scales=list(scales), k_min=k_min, k_max=k_max, split=half, boxes=boxes.double().tolist(),
                           levels=[int(v) for v in levels.tolist()])
        print(name, "k", k_min, k_max, "levels used", sorted(set(cases[name]["levels"])))
    path = os.path.join(ROOT, "tests", "golden", "roi_levels.json")
    with open(path, "w") as f:
        json.dump(cases, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

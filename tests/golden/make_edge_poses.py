"""Regenerates tests/golden/edge_poses.json: CRC32 of the CPU oracle's raybuffers (used rows, unwritten pixels as 0) and the work counters for
every frame of the edge-pose catalogue (tests/edgeposes.py).

    python tests/golden/make_edge_poses.py

Like golden.json these pin the oracle against drift and the HIP path against it (PARITY UNPINNED: the reference has no vectors of its own).
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import edgeposes as E

    out = {}
    for name, r in E.render_all().items():
        assert not r["region"], (name, r["region"])
        c = r["counters"]
        out[name] = {"rayCounts": r["rayCounts"], "crcTopDown": r["crcs"][0], "crcLeftRight": r["crcs"][1],
                     "counters": {k: c[k] for k in ("S", "E", "C", "P", "R", "lodVisits")}}
        print(name, r["rayCounts"], hex(r["crcs"][0]), hex(r["crcs"][1]))
    with open(E.FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()

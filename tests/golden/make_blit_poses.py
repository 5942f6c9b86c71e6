"""Regenerates tests/golden/blit_poses.json: for every CPU frame of the blit catalogue (tests/blitposes.py) the ray counts, the CRC32 of the image the
float32 Phase-2 rule (oraclelib.blit_reference, seam rule included) makes of the CPU oracle's raybuffers (unwritten pixels as 0, clear colour 0:
the image a GPU returns), how many pixels of it differ from the float64 rule inside that rule's margin, and how many pixels the seam rule assigned.

    python tests/golden/make_blit_poses.py

Names, counts and CRCs of this repository's own code only.
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
    import blitposes as B

    out = {}
    for name, r in B.render_all().items():
        assert r["holes"] == 0 and r["differBeyondMargin"] == 0 and r["readsUnwritten"] == 0, (name, r)
        out[name] = {"rayCounts": r["rayCounts"], "crcImage": r["crcImage"], "differInsideMargin": r["differInsideMargin"],
                     "pixels": r["pixels"], "seamRulePixels": r["seamRulePixels"]}
        print(name, r["rayCounts"], hex(r["crcImage"]), r["differInsideMargin"], r["seamRulePixels"])
    with open(B.FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Runs the bundling yardstick (tests/_bundle_ref.py) over the whole-run case of the tests and writes
tests/golden/bundle.npz.  Needs no GPU and never looks at one: nothing stored here is taken from the device.

TEST INFRASTRUCTURE ONLY:

    python tools/gen_golden_bundle.py [--out tests/golden/bundle.npz]

For each accuracy A of tests/_bundle_case.RUN_A, on the 400-node, 2 300-edge graph: the yardstick's offsets, the sha256 of
its points (the GPU test asks for the same bytes), how close its integer decisions came to their thresholds (the CPU test
demands more than 1e-9), two figures of the 300 long edges -- the mean distance from an edge's midpoint to the nearest
other midpoint, and the mean ratio of the bundled to the straight length -- and, for a device whose operations were not
all correctly rounded, the margin those figures would be held to: 4 x the largest change they show over 8 yardstick runs
whose node positions are each moved by one ulp, up or down at random.
"""
import argparse
import datetime
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "bundle.npz"))
    ap.add_argument("--perturbed", type=int, default=8)
    a = ap.parse_args()
    import _bundle_case as bc
    import _bundle_ref as br
    pos, src, dst = bc.graph()
    out = {"seed": np.int64(bc.SEED), "accuracies": np.array(bc.RUN_A, dtype=np.int64), "n_perturbed": np.int64(a.perturbed),
           "made_on": np.array(datetime.date.today().isoformat())}
    straight = br.figures(*br.run(pos, src, dst, iterations=0, smooth_passes=0), bc.LONG, pos, src, dst)
    out["straight_figures"] = np.array(straight)
    for A in bc.RUN_A:
        margins = {}
        pts, off = br.run(pos, src, dst, margins, accuracy=A)
        fig = np.array(br.figures(pts, off, bc.LONG, pos, src, dst))
        rng = np.random.default_rng(bc.SEED + A)
        change = np.zeros(2)
        for _ in range(a.perturbed):
            moved = np.nextafter(pos, np.where(rng.random(pos.shape) < 0.5, -np.inf, np.inf))
            p2, o2 = br.run(moved, src, dst, accuracy=A)
            change = np.maximum(change, np.abs(np.array(br.figures(p2, o2, bc.LONG, moved, src, dst)) - fig))
        out["offsets_%d" % A] = off
        out["sha256_%d" % A] = np.array(hashlib.sha256(np.ascontiguousarray(pts).tobytes()).hexdigest())
        out["figures_%d" % A] = fig
        out["figure_margin_%d" % A] = 4 * change
        out["margins_%d" % A] = np.array([margins["m"], margins["pixel"], margins["j"]])
        print("A = %d: %d points, longest edge %d, figures %s (straight %s), margin %s, decision margins m %.3g pixel %.3g j %.3g"
              % (A, off[-1], np.diff(off).max(), fig, np.array(straight), 4 * change, margins["m"], margins["pixel"], margins["j"]))
    np.savez(a.out, **out)
    print("->", a.out)


if __name__ == "__main__":
    sys.exit(main())

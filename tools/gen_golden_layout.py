#!/usr/bin/env python3
"""Measures, once and on the MI355X, how far one device iteration of the layout lands from one iteration of the tests'
float64 restatement, and writes tests/golden/layout.npz.

TEST INFRASTRUCTURE ONLY; needs a GPU:

    python tools/gen_golden_layout.py [--out tests/golden/layout.npz]

Every case of tests/_layout_ref.cases is stepped exactly as tests/test_layout_gpu.py steps it, with every bound on the
forces, S, T and eff asserted, so the figure is never taken from a kernel that fails them.  Stored: the case names and
seeds, the kernel geometry the sizes were chosen for, the largest |x_gpu - x_ref| / max(1, the node's step length) (or
the same for speed) over all cases and steps, and the date of the run.  The GPU test asserts 4 x that figure, and refuses
any figure that would put the bound above 1e-3.
"""
import argparse
import datetime
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "layout.npz"))
    a = ap.parse_args()
    import test_layout_gpu as t
    devs = {name: t.step_case(c) for name, c in t.CASES.items()}
    worst = max(devs.values())
    assert 0 < 4 * worst <= t.POS_BOUND_MAX, "a bound above 1e-3 would be needed: the kernel is wrong, not the tolerance"
    names = list(t.CASES)
    np.savez(a.out, case_names=np.array(names), case_seeds=np.array([t.CASES[k]["seed"] for k in names], dtype=np.int64),
             case_pos_dev=np.array([devs[k] for k in names]), i_block=np.int64(t.I_BLOCK), j_tile=np.int64(t.J_TILE),
             n_steps=np.int64(t.lref.N_STEPS), pos_dev_measured=np.float64(worst), measured_on=np.array("MI355X (gfx950)"),
             measured_date=np.array(datetime.date.today().isoformat()))
    print("pos_dev_measured = %.3g over %d cases -> %s" % (worst, len(names), a.out))


if __name__ == "__main__":
    sys.exit(main())

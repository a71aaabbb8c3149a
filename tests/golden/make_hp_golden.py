"""Generates the 50-digit fixtures tests/golden/triangulation_hp.npz and tests/golden/preint_hp.npz (needs mpmath).

Each file holds the float64 inputs of tests/test_triangulation_hp.py / tests/test_preint_hp.py, the 50-digit results of
tests/triangulation_hp.py / tests/preint_hp.py as float64 pairs (hi = the rounded value, lo = the rest) and the results of the float64
yardstick the tolerances are derived from.  The tests read the fixtures, so that they run where mpmath is not installed; where it is,
test_fixture_matches_its_generator of either module evaluates the references again and demands the same bits.

    python tests/golden/make_hp_golden.py [triangulation] [preint]      (no arguments: both)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, os.path.join(ROOT, "tests"))


def triangulation():
    import triangulation_hp as hp
    inp = hp.build_inputs()
    return {**inp, **hp.evaluate(inp)}


def preint():
    import preint_hp as hp
    from test_preint_hp import yardstick_all
    inp = hp.build_inputs()
    return {**inp, **hp.evaluate(inp), "yard": yardstick_all(inp)}


def main():
    for name, make in (("triangulation", triangulation), ("preint", preint)):
        if len(sys.argv) > 1 and name not in sys.argv[1:]:
            continue
        path = os.path.join(HERE, name + "_hp.npz")
        np.savez_compressed(path, **make())
        print("%-16s %6.1f KB" % (name, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()

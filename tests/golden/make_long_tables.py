#!/usr/bin/env python3
"""Ground truth of the exact (forward-mode) Jacobians over long wind and CA tables (tests/golden/g28_long_tables.npz) for
tests/test_exact_jac.py and tests/test_exact_aero_jac.py.

The 60-digit derivatives of make_exact_jac.py (state_truth: the defect groups) and make_exact_aero_jac.py (case_truth: the aero
path constraints) -- both take the tables from the problem -- on the LONG case of tests/table_cases.py (160 wind rows, 48 CA rows:
the bisection branch of the lookups, 1029 staged doubles) over the middle mesh (40, 65, 2), for the two decision vectors of
tests/states.py table_state(): "climb" and "knots" (nodes 4 mm and 4 cm either side of six wind knots: none ON a knot, so the fixture has no `kink` entry -- asserted).  g19 / g20 are left alone.

Needs mpmath (build container only; the tests read the .npz).  Run time: about 10 seconds on 8 cores.

Usage:  python tests/golden/make_long_tables.py"""
import os
import sys
import time
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

from mpmath import mp  # noqa: E402

import make_exact_aero_jac  # noqa: E402
import make_exact_jac  # noqa: E402

CASE, MESH, VECTORS = "LONG", "coop", ("climb", "knots")


def main():
    import exact_aero_truth
    import states
    import table_cases as TC
    mp.dps = make_exact_jac.DPS
    out = {}
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        for name in VECTORS:
            t0 = time.time()
            prob, x = states.table_state(CASE, TC.MESHES[MESH], name)
            out[name + "_x"] = x
            for k, v in make_exact_jac.state_truth(prob, x, pool).items():
                out[name + "_" + k] = v
            prob, _D, x = exact_aero_truth._with_tau(prob, x)
            nodes = exact_aero_truth.case_nodes(prob, exact_aero_truth._all_aero(prob))
            out[name + "_nodes"] = np.array(nodes, dtype=np.int32).reshape(-1, 2)
            for k, v in make_exact_aero_jac.case_truth(prob, x, nodes, pool).items():
                out[name + "_" + k] = v
            print("%s: %d defect nodes (%d kink entries), %d aero nodes (%d / %d kink entries), %.1f s" % (
                name, len(out[name + "_fv"]), int(out[name + "_kink"].sum()), len(nodes), int(out[name + "_kink_a"].sum()),
                int(out[name + "_kink_q"].sum()), time.time() - t0), flush=True)
    # no node lies on a knot (within the truth's step h = 1e-25): the fixture pins the interval 4 mm either side of a knot, it does not
    # decide which interval serves the knot itself (tests/test_table_lookups.py says so)
    assert all(int(out[name + k].sum()) == 0 for name in VECTORS for k in ("_kink", "_kink_a", "_kink_q"))
    np.savez_compressed(os.path.join(HERE, "g28_long_tables.npz"), **out)


if __name__ == "__main__":
    main()

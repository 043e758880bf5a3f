#!/usr/bin/env python3
"""Ground truth of the adjoint flight (tests/golden/g31_flight_adjoint.npz) for tests/test_flight_adjoint*.py.

Needs mpmath (the tests read the .npz) and the built library (a host-only handle gives the plan's matrices and steps).  Everything
else comes from tests/golden/g30_flight_tangent.npz alone: for each of flight_tangent_truth.FLIGHTS the stored vector x and the
per-stage F, J, Pu, Pf, verr.  The transposed recursion (flight_adjoint_truth.adjoint) runs on them in 60-digit arithmetic for the
seven functionals of flight_adjoint_truth.functionals, and the bound Eg is carried along the same run.  Stored per flight: gx [7, nvars],
gdisp [7, S, 4], Egx, Egd.  tests/test_flight_adjoint_cpu.py pins the restatement by duality against flight_tangent_truth.recursion.

Usage:  python tests/golden/make_flight_adjoint.py"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from mpmath import mp, mpf  # noqa: E402

mp.dps = 60


def M_(v):
    return mpf(float(v))


def marr(a):
    a = np.asarray(a, dtype=float)
    out = np.empty(a.shape, dtype=object)
    for i in np.ndindex(a.shape):
        out[i] = mpf(float(a[i]))
    return out


def stage_data(g):
    return {k: marr(g[k]) for k in ("F", "J", "Pu", "Pf")}


def main():
    import flight_adjoint_truth as at
    import flight_tangent_truth as tt
    import interp_truth as it
    out = {}
    for flight in tt.FLIGHTS:
        t0 = time.time()
        g = tt.load(flight)
        prob, _X, _d = tt.case(flight[0])
        mats, hs = tt.plan_tables(it.engine(prob), flight[2], flight[1])
        st = stage_data(g)
        lam = at.functionals(prob, g["x"])
        xm = marr(g["x"])
        res = {k: [] for k in ("gx", "gdisp", "Egx", "Egd")}
        for q in range(len(at.FUNCTIONALS)):
            gx, gd, Egx, Egd = at.adjoint(prob, flight[1], flight[2], xm, mats, hs, st, marr(lam[q]), value_err=g["verr"], num=M_)
            res["gx"].append(gx.astype(float))
            res["gdisp"].append(gd.astype(float))
            res["Egx"].append(Egx)
            res["Egd"].append(Egd)
        for k, v in res.items():
            out["%s_%s_k%d_%s" % (flight + (k,))] = np.array(v)
        print("%s %s k=%d: %.1f s" % (flight + (time.time() - t0,)))
    np.savez_compressed(at.G31, **out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Exact-arithmetic known answers at the degenerate states of the aerodynamic forms (tests/golden/g27_degenerate_fd.npz).

Runs in the build container (needs mpmath; NOT the reference checkout): oracle/exact_fd.py evaluates the reference's velocity RHS
and its angle of attack / dynamic pressure in 40-digit arithmetic on exactly the fp64 inputs the reference's sweeps form, and
differences them (see make_exact_fd.py and make_aero_exact_fd.py, whose keys this file keeps).  States (tests/states.py,
tests/exact_jac_truth.py), each with a short coast tail so that the aero rows apply to every aerodynamic phase:

  axis     three phases around both poles in dense air: "covered" (every position sweep takes the exact-difference form, down to
           within 2 % of its switch), "fallback" (1 m <= p <= the switch: the recomputing sweeps), "undecidable" (p < 1 m, ON the
           axis, perturbed points that cross it or land on it)
  rest     one phase at rest in calm, dense air: |v_air| = 0 exactly at three nodes, 1e-13 .. 30 m/s at the others
  corners  exact_jac_truth.corner_state: underground, on the axis, at rest

Per state:  <name>_x;  <name>_phases and <name>_p<phase>_{fc, mass, position, velocity, quaternion} like g15;  <name>_nodes and
<name>_{alpha, q, d_alpha, d_q} like g18.

Usage:  python tests/golden/make_degenerate_fd.py"""
import os
import sys
import time

import numpy as np
from mpmath import mpf

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import exact_jac_truth  # noqa: E402
import oracle  # noqa: E402
import states  # noqa: E402
from oracle import exact_fd  # noqa: E402

STATES = {"axis": states.axis_state, "rest": states.rest_state,
          "corners": lambda: states.with_coast_tail(exact_jac_truth.corner_state)}


def main():
    # At rest in the air the chain cancels v - omega x r to zero, and to 1e-13 m/s next to it: there the Earth rate has to be the
    # number the reference's C++ holds, not the decimal (exact_fd.earth_rate)
    with exact_fd.earth_rate(exact_fd.OMEGA_F64):
        out = truths()
    np.savez_compressed(os.path.join(HERE, "g27_degenerate_fd.npz"), **out)


def truths():
    out = {}
    for name, build in STATES.items():
        t0 = time.time()
        prob, x = build()
        P = oracle.Problem(prob)
        prob = dict(prob)
        prob["tau"] = [P.tau(i) for i in range(P.S)]
        phases = [i for i in range(P.S) if prob["reference_area"][i] != 0.0]
        out[name + "_x"] = x
        out[name + "_phases"] = np.array(phases, dtype=np.int32)
        for ph in phases:
            T = exact_fd.velocity_fd_truth(prob, x, ph, mpf(oracle.BARC20_CPP), with_alt_sensitivity=False)
            for key in ("fc", "mass", "position", "velocity", "quaternion"):
                out["%s_p%d_%s" % (name, ph, key)] = T[key]
        nodes = [(i, 1) for i in phases]
        A = exact_fd.aero_fd_truth(prob, x, nodes)
        out[name + "_nodes"] = np.array(nodes, dtype=np.int32)
        for k in ("alpha", "q", "d_alpha", "d_q"):
            out["%s_%s" % (name, k)] = A[k]
        print("%s: phases %s, %d aero nodes, %.1f s; all finite: %s" % (
            name, phases, len(A["alpha"]), time.time() - t0,
            all(np.isfinite(v).all() for k, v in out.items() if k.startswith(name + "_"))), flush=True)
    return out


if __name__ == "__main__":
    main()

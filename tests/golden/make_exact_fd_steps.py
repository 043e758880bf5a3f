#!/usr/bin/env python3
"""Exact-arithmetic known answers for the velocity-defect Jacobian and the aero rows over the range of position steps the
engine's difference form accepts (tests/golden/g29_exact_fd_steps.npz; tests/test_exact_fd_steps.py reads it).

Like tests/golden/make_exact_fd.py (needs mpmath; NOT the reference checkout): oracle/exact_fd.py evaluates the reference's RHS
in 40-digit arithmetic on exactly the fp64 inputs the reference's sweeps form with the problem's own dx and units, and
differences them.  Cases (tests/fd_steps.py): the all-layers, the polar, the step-scaled break state of tests/states.py and its mirror, each
at steps dx * unit_position of 1e-5 m, 1e-3 m, 0.25 m and the largest one not above 1 m by dx, and at 1 m and 1e-5 m by
unit_position with dx = 1e-8.  Per case `<state>@<step>`: the SHA-256 of the decision vector, f_c and the four blocks of
quotients as make_exact_fd.py lays them out.  The aero rows: exact_fd.aero_fd_truth of the polar state with a coasting tail at the
largest step (its 6.4 cm values are in g18_aero_exact_fd.npz).

Usage:  python tests/golden/make_exact_fd_steps.py      (about two minutes on 8 cores)"""
import multiprocessing
import os
import sys
import time

import numpy as np
from mpmath import mpf

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import fd_steps  # noqa: E402
import oracle  # noqa: E402
from oracle import exact_fd  # noqa: E402

AERO_KEYS = ("alpha", "q", "d_alpha", "d_q")


def with_tau(prob):
    P = oracle.Problem(prob)
    prob = dict(prob)
    prob["tau"] = [P.tau(i) for i in range(P.S)]     # the oracle's own LGR nodes: what the tests hand to both sides
    return prob


def velocity_case(job):
    state, label = job
    t0 = time.time()
    prob, x = fd_steps.build(state, label)
    prob = with_tau(prob)
    name = "%s@%s" % (state, label)
    T = exact_fd.velocity_fd_truth(prob, x, 0, mpf(oracle.BARC20_CPP), with_alt_sensitivity=False)
    out = {name + "_xsha": fd_steps.digest(x), name + "_phases": np.array([0], dtype=np.int32)}
    for key in ("fc", "mass", "position", "velocity", "quaternion"):
        out["%s_p0_%s" % (name, key)] = T[key]
    print("%s: %d nodes, %.1f s, max |vel/position| %.3g" % (name, len(T["fc"]), time.time() - t0, np.abs(T["position"]).max()), flush=True)
    return out


def aero_case(_):
    t0 = time.time()
    state, label = fd_steps.AERO_CASE[len("aero_"):].split("@")
    prob, x = fd_steps.build(state, label, coast_tail=True)
    prob = with_tau(prob)
    nodes = [(0, 1)]
    T = exact_fd.aero_fd_truth(prob, x, nodes)
    out = {fd_steps.AERO_CASE + "_x": x, fd_steps.AERO_CASE + "_nodes": np.array(nodes, dtype=np.int32)}
    for k in AERO_KEYS:
        out["%s_%s" % (fd_steps.AERO_CASE, k)] = T[k]
    print("%s: %d nodes, %.1f s" % (fd_steps.AERO_CASE, len(T["alpha"]), time.time() - t0), flush=True)
    return out


def run(job):
    return aero_case(job) if job is None else velocity_case(job)


def main():
    jobs = [None] + [(s, l) for s in fd_steps.STATES for l in fd_steps.STEPS]
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        parts = pool.map(run, jobs, chunksize=1)
    out = {}
    for p in parts:
        out.update(p)
    np.savez_compressed(os.path.join(HERE, "g29_exact_fd_steps.npz"), **{k: out[k] for k in sorted(out)})


if __name__ == "__main__":
    main()

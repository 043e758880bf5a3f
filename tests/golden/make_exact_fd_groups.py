#!/usr/bin/env python3
"""Exact-arithmetic known answers for the rest of the default forward-difference Jacobian (tests/golden/g21_exact_fd_groups.npz):
the velocity group of the phases WITHOUT aerodynamics, the quaternion group of the free-attitude phases, and the residuals of all
four defect groups.  g15 / g15b (make_exact_fd.py) hold the velocity group of the aerodynamic phases.

Runs in the build container (needs mpmath; NOT the reference checkout): oracle/exact_fd.py evaluates the reference's formulas
(src/pybind_dynamics.cpp:73-106, cited there line by line) in 40-digit arithmetic on exactly the fp64 inputs its sweeps form.
Per state, `<name>_x` (the decision vector, checked by the tests; for the two BASELINE.json workloads, whose vectors g15b already
holds, `<name>_x_sha256` of its bytes instead -- the generator checks that it is g15b's vector) and three phase lists:

  <name>_noair     phases with reference_area 0:  _p<i>_nfc [n, 3], _nmass [n, 3], _npos [n, 3, 3], _nquat [n, 3, 4], _ntmag, _ngmag [n]
  <name>_quat      free-attitude phases:          _p<i>_qfc [n, 4], _qquat [n, 4, 4], _qu [n, 4, 2]
  <name>_res       residual phases (on the oracle's fp64 D): _p<i>_rmass [n], _rpos [n, 3], _rvel [n, 3], _rquat [n, 4]

(last index of a sweep = perturbed component).  Deterministic: running it again rewrites the file byte for byte.

Usage:  python tests/golden/make_exact_fd_groups.py"""
import os
import sys
import time

import numpy as np
from mpmath import mpf

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import oracle  # noqa: E402
import states  # noqa: E402
from oracle import exact_fd  # noqa: E402


from exact_fd_groups_truth import BASELINE, STATES, x_digest  # noqa: E402  (the state table the tests read the fixture with)


def setup(build):
    prob, x = build()
    P = oracle.Problem(prob)
    prob = dict(prob)
    prob["tau"] = [P.tau(i) for i in range(P.S)]     # the oracle's own LGR nodes and D: what the tests hand to both sides
    return prob, x, P


def main():
    out = {}
    bc = mpf(oracle.BARC20_CPP)
    for name, (build, noair, quat, res) in STATES.items():
        prob, x, P = setup(build)
        if name in BASELINE:
            g15b = np.load(os.path.join(HERE, "g15b_exact_fd_baseline.npz"))
            assert np.array_equal(x, g15b[name + "_x"]), "the workload's decision vector is no longer g15b's"
            out[name + "_x_sha256"] = x_digest(x)
        else:
            out[name + "_x"] = x
        if noair is None:
            noair = [i for i in range(P.S) if prob["reference_area"][i] == 0.0]
        if quat is None:
            quat = [i for i in range(P.S) if not prob["attitude_hold"][i]]
        if res is None:
            res = sorted(set(noair) | set(quat))
        assert all(prob["reference_area"][i] == 0.0 for i in noair) and not any(prob["attitude_hold"][i] for i in quat)
        assert all(i in noair for i in res if prob["reference_area"][i] == 0.0)   # NoAir velocity rows read the node magnitudes
        t0 = time.time()
        for key, phases in (("noair", noair), ("quat", quat), ("res", res)):
            out["%s_%s" % (name, key)] = np.array(phases, dtype=np.int32)
        for ph in noair:
            T = exact_fd.noair_fd_truth(prob, x, ph, bc)
            for k in ("fc", "mass", "position", "quaternion", "tmag", "gmag"):
                out["%s_p%d_n%s" % (name, ph, k[:4] if k != "position" else "pos")] = T[k]
        for ph in quat:
            T = exact_fd.quat_fd_truth(prob, x, ph)
            for k in ("fc", "quaternion", "u"):
                out["%s_p%d_q%s" % (name, ph, k[:4])] = T[k]
        for ph in res:
            T = exact_fd.residual_truth(prob, x, ph, P.D(ph), bc)
            for k in ("mass", "pos", "vel", "quat"):
                out["%s_p%d_r%s" % (name, ph, k)] = T[k]
        print("%s: NoAir %s, quat %s, residuals %s: %.1f s" % (name, noair, quat, res, time.time() - t0), flush=True)
    path = os.path.join(HERE, "g21_exact_fd_groups.npz")
    np.savez_compressed(path, **out)
    print("%s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()

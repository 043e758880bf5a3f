#!/usr/bin/env python3
"""Ground truth of the aero path constraints' gradients (tests/golden/g20_exact_aero_jac.npz) for tests/test_exact_aero_jac.py.

Needs mpmath (build container only; the tests read the .npz).  The angle of attack and the dynamic pressure (src/wrapper_utils.hpp:
89-111,163-175) are composed from oracle/exact_fd.py's geodetic, atmosphere, air_velocity and quatrot on EXACT inputs -- the
normalised variables times their units in 60-digit arithmetic, without the fp64 casts of exact_fd.aero_point -- and differentiated
with respect to the normalised position (3), velocity (3) and quaternion (4) by differences with h = 1e-25: the central quotient and
both one-sided ones are kept; where the one-sided ones disagree a table knot, atmosphere layer break or clamp lies within h of the
node (`kink`), and the test holds the engine to the quotient on the side its value computation took.  The t0 / tf columns are not
stored: the air-relative velocity does not depend on the Earth angle, so their derivatives are exactly zero.

Cases (tests/exact_aero_truth.py cases()): the two constraint sets of G9 on its decision vector; every aerodynamic phase but the
last of tests/states.py's ragged, polar-dense, all-layers and layer-break states and of mixed-6x64 (whose vertical ascent has the
angle of attack near 0); the corner nodes (air at rest, exactly on the polar axis, below the polar radius).

Per case: `nodes` [R, 2] (phase, node) and per node alpha, q, d{a,q}_{c,f,b} [R, 10], kink_{a,q} [R, 10] and kappa [R]: the
conditioning (|v| + omega |r_xy| + |w|) / |v_air| of the air-relative velocity (inf where it is 0).

Usage:  python tests/golden/make_exact_aero_jac.py"""
import os
import sys
import time
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from mpmath import mp, mpf  # noqa: E402

DPS, H = 60, "1e-25"


def alpha_q(X, r_e, v_e, q, t, wind, up, uv):
    """angle of attack [rad] and dynamic pressure [Pa] at normalised (r, v), quaternion q, time t [s] (exact mpf everywhere)"""
    r = [c * up for c in r_e]
    v = [c * uv for c in v_e]
    va, h = X.air_velocity(r, v, t, wind)
    nv = mp.sqrt(va[0] ** 2 + va[1] ** 2 + va[2] ** 2)
    d = X.quatrot(X.conj(q), [mpf(1), mpf(0), mpf(0)])
    nd = mp.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2)
    qdyn = mpf("0.5") * X.atmosphere(h)[2] * nv * nv
    if nv < mpf("1e-6"):
        return mpf(0), qdyn
    c = sum((va[i] / nv) * (d[i] / nd) for i in range(3))
    return (mpf(0) if c > 1 else mp.acos(c)), qdyn


def node_truth(args):
    r, v, q, t, wt, up, uv = args
    from oracle import exact_fd as X
    mp.dps = DPS
    h = mpf(H)
    wind = [[mpf(float(a)) for a in wt[:, c]] for c in range(3)]
    up, uv = mpf(float(up)), mpf(float(uv))
    base = [mpf(float(a)) for a in list(r) + list(v) + list(q)]
    tt = mpf(t)

    def f(z):
        return alpha_q(X, z[0:3], z[3:6], z[6:10], tt, wind, up, uv)

    a0, q0 = f(base)
    # conditioning of the air-relative velocity: the magnitude of the terms that cancel in v + omega x r - w over |v_air|
    r0, v0 = [c * up for c in base[0:3]], [c * uv for c in base[3:6]]
    va, _ = X.air_velocity(r0, v0, tt, wind)
    w0 = [v0[0] + X.OMEGA * r0[1] - va[0], v0[1] - X.OMEGA * r0[0] - va[1], v0[2] - va[2]]
    s0 = mp.sqrt(sum(c * c for c in va))
    mag = mp.sqrt(sum(c * c for c in v0)) + X.OMEGA * mp.sqrt(r0[0] ** 2 + r0[1] ** 2) + mp.sqrt(sum(c * c for c in w0))
    kappa = float(mag / s0) if s0 > 0 else float("inf")
    out = np.zeros((2, 3, 10))          # [alpha / q][central, forward, backward][variable]
    for k in range(10):
        zp, zm = list(base), list(base)
        zp[k] += h
        zm[k] -= h
        fp, fm = f(zp), f(zm)
        for i, (c, p, m) in enumerate(((a0, fp[0], fm[0]), (q0, fp[1], fm[1]))):
            out[i, 0, k] = float((p - m) / (2 * h))
            out[i, 1, k] = float((p - c) / h)
            out[i, 2, k] = float((c - m) / h)
    return float(a0), float(q0), out, kappa


def case_truth(prob, x, nodes, pool):
    nn = [int(v) for v in prob["num_nodes"]]
    S, N = len(nn), sum(nn)
    M = N + S
    up, uv, ut = (float(prob["units"][k]) for k in (1, 2, 4))
    xr, xv, xq = x[M:4 * M].reshape(-1, 3), x[4 * M:7 * M].reshape(-1, 3), x[7 * M:11 * M].reshape(-1, 4)
    xt = x[11 * M + 2 * N:]
    wt = np.asarray(prob["wind_table"], dtype=np.float64)
    jobs = []
    for ph, k in nodes:
        xa = sum(nn[:ph]) + ph
        to, tf = mpf(float(xt[ph])), mpf(float(xt[ph + 1]))
        tn = to if k == 0 else mpf(float(prob["tau"][ph][k - 1])) * (tf - to) / 2 + (tf + to) / 2   # PSparams.time_nodes
        jobs.append((xr[xa + k], xv[xa + k], xq[xa + k], str(tn * mpf(ut)), wt, up, uv))
    res = pool.map(node_truth, jobs)
    J = np.array([a[2] for a in res])                # [R, 2, 3, 10]
    out = {"alpha": np.array([a[0] for a in res]), "q": np.array([a[1] for a in res]), "kappa": np.array([a[3] for a in res])}
    for i, s in enumerate("aq"):
        for j, w in enumerate("cfb"):
            out["d%s_%s" % (s, w)] = J[:, i, j]
        f, b = J[:, i, 1], J[:, i, 2]
        out["kink_" + s] = np.abs(f - b) > 1e-18 * (np.abs(f) + np.abs(b)) + 1e-300
    return out


def main():
    import exact_aero_truth
    mp.dps = DPS
    out = {}
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        for name in exact_aero_truth.CASES:
            t0 = time.time()
            prob, D, x, specs = exact_aero_truth.case(name)
            nodes = exact_aero_truth.case_nodes(prob, specs)
            out[name + "_x"] = x
            out[name + "_nodes"] = np.array(nodes, dtype=np.int32).reshape(-1, 2)
            for k, v in case_truth(prob, x, nodes, pool).items():
                out[name + "_" + k] = v
            print("%s: %d nodes, %d / %d kink entries, %.1f s" % (name, len(nodes), int(out[name + "_kink_a"].sum()),
                                                                   int(out[name + "_kink_q"].sum()), time.time() - t0), flush=True)
    np.savez_compressed(os.path.join(HERE, "g20_exact_aero_jac.npz"), **out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Ground truth of the defect Jacobian (tests/golden/g19_exact_jac.npz) for tests/test_exact_jac.py.

Needs mpmath (build container only; the tests read the .npz).  The reference's RHS is composed from the functions of
oracle/exact_fd.py (geodetic, atmosphere, interp, air_velocity, gravity, quatrot) on EXACT inputs -- the normalised variables
times their units in 60-digit arithmetic, without the fp64 casts of exact_fd.rhs_air -- and differentiated with respect to the
normalised variables by differences with h = 1e-25: the central quotient (exact to ~1e-40 here) and the forward and the backward
one are kept; where the one-sided ones disagree a table knot, atmosphere layer break or clamp lies within h of
the node (`kink`), and the test holds the engine to the quotient on the side its value computation took.  On the polar axis, where the value jumps, `Jv_conv` holds the
derivative under the engine's stated convention (the air of the axis point held along x / y).

States (tests/exact_jac_truth.py states()): the shipped example, tests/states.py's ragged, all-layers, layer-break and
polar-dense states, and the corner nodes (below the polar radius, exactly on the polar axis, at rest in the air).

Usage:  python tests/golden/make_exact_jac.py"""
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
BARC20 = "-0.484165371736e-3"        # what the engine takes for barC20 = 0 (src/gravity.cpp:18)


def _setup():
    from oracle import exact_fd
    mp.dps = DPS
    return exact_fd


def rhs(X, m_e, r_e, v_e, q, t, thrust, area, nozzle, wind, ca, units, frozen=None):
    """src/pybind_dynamics.cpp:30-71 (air) / :73-92 (area == 0) on exact inputs -> acc / unit_v.  frozen = (h, wind in ECI):
    the air of that point instead of the position's own (the engine's convention on the polar axis, where the altitude jumps)"""
    um, up, uv = units
    m = m_e * um
    r = [c * up for c in r_e]
    v = [c * uv for c in v_e]
    d = X.quatrot(X.conj(q), [mpf(1), mpf(0), mpf(0)])
    g = X.gravity(r, mpf(BARC20))
    if area == 0:
        return [((thrust * d[i]) / m + g[i]) / uv for i in range(3)]
    if frozen is None:
        va, h = X.air_velocity(r, v, t, wind)
    else:
        h, w = frozen
        va = [v[0] + X.OMEGA * r[1] - w[0], v[1] - X.OMEGA * r[0] - w[1], v[2] - w[2]]
    T, P, rho, a = X.atmosphere(h)
    vn = mp.sqrt(va[0] ** 2 + va[1] ** 2 + va[2] ** 2)
    cav = X.interp(vn / a, ca[0], ca[1])
    F = [mpf("0.5") * rho * area * cav * vn * -c for c in va]
    Tt = thrust - nozzle * P
    return [((Tt * d[i] + F[i]) / m + g[i]) / uv for i in range(3)]


def quat_rhs(q, u, uu):
    """src/pybind_dynamics.cpp:94-106"""
    oy, oz = u[0] * uu * mp.pi / 180, u[1] * uu * mp.pi / 180
    return [mpf("0.5") * (-q[2] * oy - q[3] * oz), mpf("0.5") * (q[2] * oz - q[3] * oy),
            mpf("0.5") * (q[0] * oy - q[1] * oz), mpf("0.5") * (q[0] * oz + q[1] * oy)]


def node_truth(args):
    m, r, v, q, u, t, thrust, area, nozzle, wt, ct, units, uu = args
    X = _setup()
    h = mpf(H)
    wind = [[mpf(float(a)) for a in wt[:, c]] for c in range(3)]
    ca = [[mpf(float(a)) for a in ct[:, c]] for c in range(2)]
    un = [mpf(float(a)) for a in units]
    thrust, area, nozzle = mpf(float(thrust)), mpf(float(area)), mpf(float(nozzle))
    base = [mpf(float(a)) for a in [m] + list(r) + list(v) + list(q)]
    tt = mpf(float(t))

    def f(z):
        return rhs(X, z[0], z[1:4], z[4:7], z[7:11], tt, thrust, area, nozzle, wind, ca, un)

    f0 = f(base)
    Jc, Jf, Jb = np.zeros((3, 11)), np.zeros((3, 11)), np.zeros((3, 11))
    for k in range(11):
        zp, zm = list(base), list(base)
        zp[k] += h
        zm[k] -= h
        fp, fm = f(zp), f(zm)
        for c in range(3):
            Jc[c, k] = float((fp[c] - fm[c]) / (2 * h))
            Jf[c, k] = float((fp[c] - f0[c]) / h)
            Jb[c, k] = float((f0[c] - fm[c]) / h)
    # on the polar axis the value jumps along x / y (altitude -N on the axis, the true altitude off it): the engine's convention
    # (the partials of p and of the longitude are 0) is the derivative with the air of the axis point held
    Jconv = Jc.copy()
    if base[1] == 0 and base[2] == 0 and area != 0:
        rr = [c * un[1] for c in base[1:4]]
        vv = [c * un[2] for c in base[4:7]]
        va0, h0 = X.air_velocity(rr, vv, tt, wind)
        w0 = [vv[0] + X.OMEGA * rr[1] - va0[0], vv[1] - X.OMEGA * rr[0] - va0[1], vv[2] - va0[2]]
        for k in (1, 2):
            zp, zm = list(base), list(base)
            zp[k] += h
            zm[k] -= h
            fp = rhs(X, zp[0], zp[1:4], zp[4:7], zp[7:11], tt, thrust, area, nozzle, wind, ca, un, frozen=(h0, w0))
            fm = rhs(X, zm[0], zm[1:4], zm[4:7], zm[7:11], tt, thrust, area, nozzle, wind, ca, un, frozen=(h0, w0))
            for c in range(3):
                Jconv[c, k] = float((fp[c] - fm[c]) / (2 * h))
    qb, ub = base[7:11], [mpf(float(a)) for a in u]
    uum = mpf(float(uu))
    fq0 = quat_rhs(qb, ub, uum)
    Jq = np.zeros((4, 6))
    for k in range(6):          # dq is bilinear in (q, u): the central difference is exact
        zp, zm = list(qb) + list(ub), list(qb) + list(ub)
        zp[k] += h
        zm[k] -= h
        fp, fm = quat_rhs(zp[:4], zp[4:], uum), quat_rhs(zm[:4], zm[4:], uum)
        for c in range(4):
            Jq[c, k] = float((fp[c] - fm[c]) / (2 * h))
    return [float(a) for a in f0], Jc, Jf, Jb, [float(a) for a in fq0], Jq, Jconv


def state_truth(prob, x, pool):
    nn = [int(v) for v in prob["num_nodes"]]
    S, N = len(nn), sum(nn)
    M = N + S
    um, up, uv, uu, ut = [float(a) for a in prob["units"]]
    xm, xr, xv, xq = x[:M], x[M:4 * M].reshape(-1, 3), x[4 * M:7 * M].reshape(-1, 3), x[7 * M:11 * M].reshape(-1, 4)
    xu, xt = x[11 * M:11 * M + 2 * N].reshape(-1, 2), x[11 * M + 2 * N:]
    jobs = []
    for i in range(S):
        ua = sum(nn[:i])
        xa = ua + i
        for j in range(nn[i]):
            k = xa + 1 + j
            jobs.append((xm[k], xr[k], xv[k], xq[k], xu[ua + j], xt[i], prob["thrust"][i], prob["reference_area"][i],
                         prob["nozzle_area"][i], np.asarray(prob["wind_table"]), np.asarray(prob["ca_table"]), (um, up, uv), uu))
    res = pool.map(node_truth, jobs)
    out = {"fv": np.array([a[0] for a in res]), "Jv_c": np.array([a[1] for a in res]), "Jv_f": np.array([a[2] for a in res]),
           "Jv_b": np.array([a[3] for a in res]), "fq": np.array([a[4] for a in res]), "Jq": np.array([a[5] for a in res]),
           "Jv_conv": np.array([a[6] for a in res])}
    d = np.abs(out["Jv_f"] - out["Jv_b"])
    out["kink"] = d > 1e-18 * (np.abs(out["Jv_f"]) + np.abs(out["Jv_b"])) + 1e-300
    return out


def main():
    import exact_jac_truth
    out = {}
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        for name, build in exact_jac_truth.states().items():
            t0 = time.time()
            prob, x = build()
            out[name + "_x"] = x
            for k, v in state_truth(prob, x, pool).items():
                out[name + "_" + k] = v
            print("%s: %d nodes, %d kink entries, %.1f s" % (name, len(out[name + "_fv"]), int(out[name + "_kink"].sum()),
                                                             time.time() - t0))
    np.savez_compressed(os.path.join(HERE, "g19_exact_jac.npz"), **out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""g24_mesh_truth.npz: manufactured trajectories for the collocation error estimate's convergence test (tests/test_mesh_error.py).

Two one-section problems on the example's units and tables (gelato_amd.problem "example"):
  "noair": NoAir (reference_area 0), engine on, free attitude, constant control -- a smooth right-hand side;
  "air":   reference_area 2.21, engine on, free attitude, constant control, climbing through knots of the wind and CA tables
           (piecewise linear: the right-hand side has kinks inside the section).
The true trajectory: scipy's DOP853 at rtol 1e-13 on the oracle's right-hand side (the one the defect rows impose, per second of
normalised state; the Earth angle at the normalised time), integrated knot to knot through every sample time.  For every n in NS:
x_<case>_<n> = the packed decision vector (states at tau_x = [-1, tau_n], the constant control at tau_n, t = [0, T]) and
true_<case>_<n> [n+2, 11] = the true states at sigma_0 = -1 and the flipped LGR points sigma of n + 1.  prob_<case>_* = the static
problem without num_nodes.  Needs scipy and the oracle (oracle.build()).
Deterministic: rerunning reproduces the file byte for byte.     python3 tests/golden/make_mesh_truth.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
NS = (3, 5, 8, 12, 16)


def base_prob():
    from gelato_amd import con_dynamics, problem
    pdict, unitdict, _c, _x = problem.make_problem("example")
    return dict(con_dynamics.problem_arrays(pdict, unitdict))


CASES = {
    # T seconds, thrust N, massflow kg/s, area, nozzle, m0 kg, r0 m, v0 m/s, control deg/s
    "noair": dict(T=120.0, thrust=30700.0, massflow=9.8, area=0.0, nozzle=0.0, m0=4000.0, r0=(6578137.0, 0.0, 0.0),
                  v0=(0.0, 7600.0, 900.0), u=(0.4, -0.25)),
    "air": dict(T=6.0, thrust=420000.0, massflow=140.0, area=2.21, nozzle=0.68, m0=30000.0, r0=(6378137.0 + 2000.0, 0.0, 0.0),
                v0=(400.0, 465.0, 40.0), u=(-0.3, 0.1)),
}


def problem_of(case):
    c = CASES[case]
    prob = base_prob()
    for k, v in (("thrust", c["thrust"]), ("massflow", c["massflow"]), ("reference_area", c["area"]), ("nozzle_area", c["nozzle"])):
        prob[k] = np.array([v])
    prob["engine_on"] = np.array([1], dtype=np.int32)
    prob["attitude_hold"] = np.array([0], dtype=np.int32)
    return prob


def rhs_fn(prob):
    import oracle
    um, up, uv, uu, ut = [float(v) for v in prob["units"]]
    units = np.array([um, up, uv])
    param = np.array([prob["thrust"][0], prob["massflow"][0], prob["reference_area"][0], 0.0, prob["nozzle_area"][0]])

    def f(t_norm, X, Uc):
        F = np.zeros(11)
        F[0] = -float(prob["massflow"][0]) / um
        F[1:4] = X[4:7] * (uv / up)
        if float(prob["reference_area"][0]) != 0.0:
            F[4:7] = oracle.dynamics_velocity(X[None, 0], X[None, 1:4], X[None, 4:7], X[None, 7:11], np.array([t_norm]), param,
                                              prob["wind_table"], prob["ca_table"], units)[0]
        else:
            F[4:7] = oracle.dynamics_velocity_NoAir(X[None, 0], X[None, 1:4], X[None, 7:11], param, units)[0]
        F[7:11] = oracle.dynamics_quaternion(X[None, 7:11], Uc[None, :], uu)[0]
        return F
    return f


def main():
    from scipy.integrate import solve_ivp
    from gelato_amd._lib import lib
    import ctypes as C
    out = {}
    for case in sorted(CASES):
        c = CASES[case]
        prob = problem_of(case)
        um, up, uv, uu, ut = [float(v) for v in prob["units"]]
        Tn = c["T"] / ut
        Uc = np.array(c["u"]) / uu
        f = rhs_fn(prob)
        q0 = np.array([0.9, 0.1, -0.3, 0.2])
        q0 /= np.linalg.norm(q0)
        X0 = np.concatenate([[c["m0"] / um], np.array(c["r0"]) / up, np.array(c["v0"]) / uv, q0])

        def ode(ts, X):   # seconds
            return f(ts / ut, X, Uc)
        times = {}
        for n in NS:
            tau = np.zeros(n)
            sig = np.zeros(n + 1)
            lib().gel_lgr_nodes(n, tau.ctypes.data_as(C.POINTER(C.c_double)))
            lib().gel_lgr_nodes(n + 1, sig.ctypes.data_as(C.POINTER(C.c_double)))
            times[n] = (tau, sig)
        # every sample time in seconds, integrated knot to knot from t = 0
        ts_all = sorted({0.0} | {float((z + 1) / 2 * c["T"]) for n in NS for z in np.concatenate(times[n])})
        state = {0.0: X0.copy()}
        X, t0 = X0.copy(), 0.0
        for ts in ts_all[1:]:
            sol = solve_ivp(ode, (t0, ts), X, method="DOP853", rtol=1e-13, atol=1e-16)
            assert sol.success, sol.message
            X, t0 = sol.y[:, -1].copy(), ts
            state[ts] = X.copy()
        at = lambda z: state[float((z + 1) / 2 * c["T"])]
        for n in NS:
            tau, sig = times[n]
            Xs = np.array([X0] + [at(z) for z in tau])
            M, N = n + 1, n
            x = np.concatenate([Xs[:, 0], Xs[:, 1:4].ravel(), Xs[:, 4:7].ravel(), Xs[:, 7:11].ravel(), np.tile(Uc, N), [0.0, Tn]])
            assert x.size == 11 * M + 2 * N + 2
            out["x_%s_%d" % (case, n)] = x
            out["true_%s_%d" % (case, n)] = np.array([X0] + [at(z) for z in sig])
        for k, v in prob.items():
            out["prob_%s_%s" % (case, k)] = np.asarray(v)
    out["ns"] = np.array(NS, dtype=np.int32)
    path = os.path.join(HERE, "g24_mesh_truth.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()

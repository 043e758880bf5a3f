"""Independent restatement of the explicit propagation (include/gelato_amd.h gel_propagate) for the tests:
classical RK4 in numpy with the oracle's right-hand sides (mesh_truth.rhs), the plan's OWN stage points and control matrix, and
a first-order bound carried along the trajectory -- derived from the arithmetic, not fitted:

  A   = |dF/dX| (11 x 11), forward differences of the oracle's right-hand side at the step's start
  dF  = what the two sides' right-hand sides may differ by at equal arguments: mass 0 (the same IEEE quotient); position 2u |F|
        (one product each); velocity SURVEY 8(c)'s parity 1e-12 + 1e-10 |F|; quaternion quat_rate's roundings (6u) plus the
        control samples' 2 gamma_n sum |Wu| |U| (an fma chain of n terms against a numpy dot product) through its bilinear form
  e1 = A E + dF;  e2 = A (E + S h/2 e1) + dF;  e3 = A (E + S h/2 e2) + dF;  e4 = A (E + S h e3) + dF
  E <- E + S h/6 (e1 + 2 e2 + 2 e3 + e4) + 8u |y|          (the last term: the two sides' roundings of the update itself)
The tests allow 2 E: the factor 2 covers the variation of A inside a step and the second-order terms.  u = 2^-53.

Three WRONG restatements (`mutate`) give the bound its teeth: S without unit_t, the control held at the left node's value through
an interval, and n k equal steps across the section instead of k per node interval."""
import numpy as np

import mesh_truth as mt
from mesh_truth import D2R, GROUP_COLS, U, gamma


def _lagrange(tau, z):
    """the Lagrange basis on tau at the points z (plain fp64: for the equal-steps mutation only)"""
    W = np.ones((len(z), len(tau)))
    for j in range(len(tau)):
        for m in range(len(tau)):
            if m != j:
                W[:, j] *= (z - tau[m]) / (tau[j] - tau[m])
    return W


def samples(m, Uc):
    """the control polynomial at the plan's stage points: (Us [Pp, 2], dUs [Pp, 2] = 2 gamma_n sum |Wu| |U|, 0 at a copy)"""
    n = Uc.shape[0]
    Us = m["Wu"] @ Uc
    dUs = 2 * gamma(n) * (np.abs(m["Wu"]) @ np.abs(Uc))
    c = m["copy_u"] >= 0
    Us[c] = Uc[m["copy_u"][c]]
    dUs[c] = 0.0
    return Us, dUs


def _rhs(prob, s, X, Uv, sig, to, tf):
    """F [P, 11] at states X [P, 11], controls Uv [P, 2] and points sig [P]"""
    X = np.atleast_2d(X)
    P = X.shape[0]
    return mt.rhs(prob, s, X, np.broadcast_to(Uv, (P, 2)).copy(), np.broadcast_to(sig * (tf - to) / 2 + (tf + to) / 2, (P,)).copy())


def _dF(prob, s, y, Uv, dUv, F):
    uu = float(prob["units"][3])
    d = np.zeros(11)
    d[1:4] = 2 * U * np.abs(F[1:4])
    d[4:7] = 1e-12 + 1e-10 * np.abs(F[4:7])
    if not prob["attitude_hold"][s]:
        w = np.abs(Uv) * uu * D2R
        dw = dUv * uu * D2R + 2 * U * w
        q1 = np.abs(y[7:11]).sum()
        d[7:11] = 0.5 * q1 * dw.sum() + 6 * U * 0.5 * q1 * w.sum()
    return d


def _jac_abs(prob, s, y, Uv, sig, to, tf, F0):
    """|dF/dX| by forward differences of the oracle's right-hand side (one call for the 11 perturbed states)"""
    h = 1e-7 * (1.0 + np.abs(y))
    Xp = y[None, :] + np.diag(h)
    Fp = _rhs(prob, s, Xp, Uv, sig, to, tf)
    return np.abs((Fp - F0[None, :]) / h[:, None]).T    # A[c, d] = |dF_c / dX_d|


def propagate_phase(E, plan, prob, x, s, restart=False, want_bound=True, mutate=None):
    """-> dict(y [n+1, 11], bound [n+1, 11] (2 E at every node; row 0 is 0: a copy)) of phase s for one decision vector.
    mutate: None, "no_unit_t", "hold_control" or "equal_steps" (the last fills y at the last node only; the others NaN)"""
    m = plan.matrices(s)
    k = plan.steps[s]
    X, Uc, to, tf = mt.phase_state(E, x, s)
    n = X.shape[0] - 1
    hold = bool(prob["attitude_hold"][s])
    ut = float(prob["units"][4])
    S = (tf - to) * ut / 2.0
    if mutate == "no_unit_t":
        S = (tf - to) / 2.0
    tx = np.concatenate([[-1.0], E.tau(s)])
    pts = m["pts"]
    if hold:
        Us, dUs = np.zeros((len(pts), 2)), np.zeros((len(pts), 2))
    else:
        Us, dUs = samples(m, Uc)
    hs = (tx[1:] - tx[:-1]) / k
    if mutate == "hold_control" and not hold:
        for j in range(n):
            Us[2 * k * j:2 * k * (j + 1) + (1 if j == n - 1 else 0)] = Uc[max(j - 1, 0)]
    if mutate == "equal_steps":
        pts = -1.0 + (tx[-1] + 1.0) * np.arange(2 * n * k + 1) / (2.0 * n * k)
        hs = np.full(n, (tx[-1] + 1.0) / (n * k))
        if not hold:
            Us = _lagrange(E.tau(s), pts) @ Uc
    Y = np.full((n + 1, 11), np.nan)
    Bd = np.zeros((n + 1, 11))
    Y[0] = X[0]
    y = X[0].copy()
    Eb = np.zeros(11)
    for j in range(n):
        if restart:
            y = X[j].copy()
            Eb = np.zeros(11)
        Sh = S * hs[j]
        for i in range(k):
            p = 2 * (k * j + i)
            k1 = _rhs(prob, s, y, Us[p], pts[p], to, tf)[0]
            k2 = _rhs(prob, s, y + Sh * 0.5 * k1, Us[p + 1], pts[p + 1], to, tf)[0]
            k3 = _rhs(prob, s, y + Sh * 0.5 * k2, Us[p + 1], pts[p + 1], to, tf)[0]
            k4 = _rhs(prob, s, y + Sh * k3, Us[p + 2], pts[p + 2], to, tf)[0]
            if want_bound:
                A = _jac_abs(prob, s, y, Us[p], pts[p], to, tf, k1)
                aS = abs(Sh)
                e1 = A @ Eb + _dF(prob, s, y, Us[p], dUs[p], k1)
                e2 = A @ (Eb + aS / 2 * e1) + _dF(prob, s, y, Us[p + 1], dUs[p + 1], k2)
                e3 = A @ (Eb + aS / 2 * e2) + _dF(prob, s, y, Us[p + 1], dUs[p + 1], k3)
                e4 = A @ (Eb + aS * e3) + _dF(prob, s, y, Us[p + 2], dUs[p + 2], k4)
            y = y + Sh / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)
            if want_bound:
                Eb = Eb + aS / 6 * (e1 + 2 * e2 + 2 * e3 + e4) + 8 * U * np.abs(y)
        if mutate != "equal_steps" or j == n - 1:
            Y[j + 1] = y
        Bd[j + 1] = 2 * Eb
    return {"y": Y, "bound": Bd, "X": X}


def group_err(X, Y):
    """err [4] and its per-component parts (e_c [11], den_c [11]) in the engine's normalisation"""
    den = 1.0 + np.abs(X).max(axis=0)
    ec = np.abs(Y[1:] - X[1:]).max(axis=0) / den
    return np.array([ec[a:b].max() for a, b in GROUP_COLS]), ec, den


def propagate_all(E, plan, prob, x, restart=False, want_bound=True):
    """-> (y [M, 11], bound_y [M, 11], err [S, 4], bound_err [S, 4]) of one vector, every phase"""
    ys, bs, es, bes = [], [], [], []
    for s in range(E.S):
        r = propagate_phase(E, plan, prob, x, s, restart=restart, want_bound=want_bound)
        e, ec, den = group_err(r["X"], r["y"])
        bc = r["bound"].max(axis=0) / den + 4 * U * ec
        ys.append(r["y"]); bs.append(r["bound"]); es.append(e)
        bes.append(np.array([bc[a:b].max() for a, b in GROUP_COLS]))
    return np.concatenate(ys), np.concatenate(bs), np.array(es), np.array(bes)


def unpack_y(Yv, M):
    """[M, 11] from the device's y [11 M] (the state part of x's layout)"""
    return np.concatenate([Yv[0:M, None], Yv[M:4 * M].reshape(-1, 3), Yv[4 * M:7 * M].reshape(-1, 3), Yv[7 * M:11 * M].reshape(-1, 4)],
                          axis=1)


def g24_case(g, case, n):
    prob = {k[len("prob_%s_" % case):]: g[k] for k in g if k.startswith("prob_%s_" % case)}
    prob["num_nodes"] = np.array([n], dtype=np.int32)
    return prob, g["x_%s_%d" % (case, n)]

"""Independent restatement of the collocation error estimate (include/gelato_amd.h gel_mesh_error) for the tests: numpy for the
matrix products, the oracle's dynamics_velocity / _NoAir / dynamics_quaternion for the right-hand side, and the bound every
output must meet, derived from the arithmetic (not fitted):

  X~ = Lx X, U~ = Lu U          each side rounds a dot product of k terms: |error| <= gamma_k sum |L| |X|, both sides: 2 gamma_k
  F (right-hand side)           mass: the same IEEE quotient on both sides (exact agreement); position X~_vel (unit_v/unit_p):
                                one product, plus the X~ difference; velocity: SURVEY 8(c)'s RHS parity 1e-12 + 1e-10 |F|;
                                quaternion: quat_rate's products (6 roundings) plus the X~ / U~ differences through its bilinear form
  X^ = X_0 + S I F              2 gamma_{P+1} (|X_0| + S sum_l |I_jl| |F_l|) for the two sides' sums, S sum_l |I_jl| dF_l for F's
  d = X^ - X~                   dX~ + the above + 2u |d|
  e = max |d| / (1 + max |X~|)  max_j,c (B_jc + e_c dmax_c) / (1 + max_c) + 4u e
with gamma_k = k u / (1 - k u), u = 2^-53."""
import numpy as np

U = 2.0 ** -53
GROUP_COLS = ((0, 1), (1, 4), (4, 7), (7, 11))
D2R = 0.017453292519943295769


def gamma(k):
    return k * U / (1.0 - k * U)


def phase_state(E, x, s):
    """X [n+1, 11] (mass, pos, vel, quat at the state nodes xa .. xa+n), Uc [n, 2], to, tf"""
    M, N = E.M, E.N
    nn = [int(v) for v in E.num_nodes]
    n = nn[s]
    ua = int(sum(nn[:s]))
    xa = ua + s
    xs = slice(xa, xa + n + 1)
    X = np.concatenate([x[0:M][xs, None], x[M:4 * M].reshape(-1, 3)[xs], x[4 * M:7 * M].reshape(-1, 3)[xs],
                        x[7 * M:11 * M].reshape(-1, 4)[xs]], axis=1)
    Uc = x[11 * M:11 * M + 2 * N].reshape(-1, 2)[ua:ua + n]
    t = x[11 * M + 2 * N:]
    return X, Uc, float(t[s]), float(t[s + 1])


def rhs(prob, s, Xt, Ut, tp):
    """F [P, 11] of phase s at interpolated states Xt [P, 11], controls Ut [P, 2], normalised times tp [P] (oracle)"""
    import oracle
    um, up, uv, uu, ut = [float(v) for v in prob["units"]]
    units = np.array([um, up, uv])
    P = Xt.shape[0]
    F = np.zeros((P, 11))
    F[:, 0] = (-float(prob["massflow"][s]) / um) if prob["engine_on"][s] else 0.0
    F[:, 1:4] = Xt[:, 4:7] * (uv / up)
    param = np.array([prob["thrust"][s], prob["massflow"][s], prob["reference_area"][s], 0.0, prob["nozzle_area"][s]], dtype=float)
    if float(prob["reference_area"][s]) != 0.0:
        F[:, 4:7] = oracle.dynamics_velocity(Xt[:, 0], Xt[:, 1:4], Xt[:, 4:7], Xt[:, 7:11], tp, param, prob["wind_table"],
                                             prob["ca_table"], units)
    else:
        F[:, 4:7] = oracle.dynamics_velocity_NoAir(Xt[:, 0], Xt[:, 1:4], Xt[:, 7:11], param, units)
    if not prob["attitude_hold"][s]:
        F[:, 7:11] = oracle.dynamics_quaternion(Xt[:, 7:11], Ut, uu)
    return F


def estimate(E, prob, x, s, want_bound=True):
    """-> dict(err [4], diff [P, 11], bound_err [4], bound_diff [P, 11]) of phase s for one decision vector x"""
    m = E.mesh_matrices(s)
    Lx, Lu, I, sg = m["Lx"], m["Lu"], m["I"], m["sigma"]
    X, Uc, to, tf = phase_state(E, x, s)
    n = X.shape[0] - 1
    P = n + 1
    hold = bool(prob["attitude_hold"][s])
    Xt = Lx @ X
    Ut = Lu @ Uc if not hold else np.zeros((P, 2))
    tp = sg * (tf - to) / 2 + (tf + to) / 2
    F = rhs(prob, s, Xt, Ut, tp)
    S = (tf - to) * float(prob["units"][4]) / 2.0
    Xh = X[0] + S * (I @ F)
    d = Xh - Xt
    mx = np.maximum(np.abs(Xt).max(axis=0), np.abs(X[0]))
    ec = np.abs(d).max(axis=0) / (1.0 + mx)
    err = np.array([ec[a:b].max() for a, b in GROUP_COLS])
    out = {"err": err, "diff": d, "Xt": Xt, "F": F, "S": S}
    if not want_bound:
        return out
    um, up, uv, uu, ut = [float(v) for v in prob["units"]]
    dXt = 2 * gamma(n + 1) * (np.abs(Lx) @ np.abs(X))
    dF = np.zeros_like(F)
    dF[:, 1:4] = (uv / up) * dXt[:, 4:7] + 2 * U * np.abs(F[:, 1:4])
    dF[:, 4:7] = 1e-12 + 1e-10 * np.abs(F[:, 4:7])
    if not hold:
        w = np.abs(Ut) * uu * D2R                                   # |omega_y|, |omega_z|
        dw = 2 * gamma(n) * (np.abs(Lu) @ np.abs(Uc)) * uu * D2R + 2 * U * w
        q1 = np.abs(Xt[:, 7:11]).sum(axis=1)
        dq1 = dXt[:, 7:11].sum(axis=1)
        dF[:, 7:11] = (0.5 * (dq1 * w.sum(axis=1) + q1 * dw.sum(axis=1)) + 6 * U * 0.5 * q1 * w.sum(axis=1))[:, None]
    aI = np.abs(I)
    Bd = (dXt + S * (aI @ dF) + 2 * gamma(P + 1) * (np.abs(X[0]) + S * (aI @ np.abs(F))) + 2 * U * np.abs(d))
    dmx = dXt.max(axis=0)
    Be_c = (Bd.max(axis=0) + ec * dmx) / (1.0 + mx) + 4 * U * ec
    out["bound_diff"] = Bd
    out["bound_err"] = np.array([Be_c[a:b].max() for a, b in GROUP_COLS])
    return out


def estimate_all(E, prob, x):
    """err [S, 4], diff [npts, 11], bound_err [S, 4], bound_diff [npts, 11] of one vector, every phase"""
    parts = [estimate(E, prob, x, s) for s in range(E.S)]
    return (np.array([p["err"] for p in parts]), np.concatenate([p["diff"] for p in parts]),
            np.array([p["bound_err"] for p in parts]), np.concatenate([p["bound_diff"] for p in parts]))

"""What the tangent-linear propagation's tests share (include/gelato_amd.h gel_propagate_tangent): the two cases, their
eleven seed directions, and the tangent recursion of the discrete RK4 map written once for any arithmetic -- the generator
(tests/golden/make_flight_tangent.py) runs it on mpmath numbers with 60 digits, the tests run it in fp64 on the stored per-stage
partials to evaluate WRONG restatements (`mutate`), which give the bound its teeth:

  "no_dS"           the step's own tangent dS = (dtf - dto) unit_t / 2 dropped: a knot time then moves nothing
  "no_djump"        the knots' djump dropped: the chain carries dy across every knot as it is
  "shift_factors"   the factor direction of phase s applied to phase s + 1 (phase 0 gets none)
  "no_wind_slope"   in d(wn fw) = wn dfw + fw dwn the second term dropped: the wind's change with the altitude

The recursion (F, J = dF/dX, Pu = dF/dU, Pf = dF/dfactors per stage; a = 0, Sh/2, Sh/2, Sh and da likewise from dSh = dS h):
  dyt = dy + a dF_prev + da F_prev;   dF = J dyt + Pu dU + Pf df;   dy += Sh/6 (dF1 + 2 dF2 + 2 dF3 + dF4) + dSh/6 (F1 + 2 F2 + 2 F3 + F4)
and the bound E carried along it, derived and not fitted (u = 2^-53; the tests allow 2 E):
  e(dF)  velocity rows: sum_d (1e-12 + 1e-9 |J_cd|) |dyt_d|, the same form on Pu, Pf -- the project's own contract for exactly these
         tangents, which also covers J being evaluated on the device's own trajectory;
         the other rows (constants and single products): 8u (|J| |dyt| + |Pu| |dU| + |Pf| |df|);   plus |J| e(dyt) in every row
  e(dyt) = E + |a| e(dF_prev) + |da| dF_prev, dF_prev = what the two sides' VALUES of F may differ by (propagate_truth._dF)
  E     += |Sh|/6 (e1 + 2 e2 + 2 e3 + e4) + |dSh|/6 (dF1 + 2 dF2 + 2 dF3 + dF4) + 8u |dy|;   knot: + u (|djump| + |dy + djump|)
"""
import os

import numpy as np

U = 2.0 ** -53
HERE = os.path.dirname(os.path.abspath(__file__))
G30 = os.path.join(HERE, "golden", "g30_flight_tangent.npz")
TRUTH_VEC = 1          # the vector of each case's batch whose tangents g30 holds
DIRECTIONS = ("mass0", "position0_y", "velocity0_z", "thrust_all", "massflow_phase2", "area_all", "wind_all", "knot_time", "u0_bias",
              "mass_after_drop", "dense")
# (case, plan mode, steps per node interval) of the flights g30 holds
FLIGHTS = (("example", "chain", 1), ("noair", "chain", 2), ("noair", "section", 2))
# the example over the long wind and CA tables of tests/table_cases.py (count path at 32 rows, bisection and an odd number of staged
# doubles at 160 / 48): dy and its bound alone
TABLE_FLIGHTS = (("example@EDGE32", "chain", 1), ("example@LONG", "chain", 1))
MUTATIONS = ("no_dS", "no_djump", "shift_factors", "no_wind_slope")


def sidx(M, node, c):
    """component c of state row `node` in a packed vector"""
    return node if c == 0 else (M + 3 * node + c - 1 if c < 4 else (4 * M + 3 * node + c - 4 if c < 7 else 7 * M + 4 * node + c - 7))


def state_rows(M, node):
    return np.array([sidx(M, node, c) for c in range(11)])


def case(name):
    """(prob, X [3, nvars], disp [3, S, 4]) of a case, numpy only.  "example": the shipped problem as flight_truth.flight_batch's batch
    of three (vector 1: the mass jettisoned at the stage knots).  "noair": three phases of five nodes without aerodynamics
    "example@CASE": the example over the tables of tests/table_cases.py.  (reference_area = 0), engines on, phase 0 held and phases 1, 2 free; random states that jump at every knot."""
    import flight_truth as ft
    import interp_truth as it
    if name.startswith("kinks"):   # tests/kink_flight.py: every phase starts on another branch of the right-hand side
        import kink_flight
        return kink_flight.kink_problem("ends" if name == "kinks@ENDS" else None)
    if name.startswith("example"):
        prob, x0 = it.named("example")
        if "@" in name:            # "example@CASE": over the wind and CA tables of table_cases.CASES[CASE]
            import table_cases as TC
            prob = TC.with_tables(prob, name.split("@")[1])
        E = it.engine(prob)
        X = ft.flight_batch(x0, E)
    else:
        prob = it.prob_of([5, 5, 5])
        prob["reference_area"] = np.zeros(3)
        prob["nozzle_area"] = np.zeros(3)
        E = it.engine(prob)
        X = np.stack([it.random_x(E, 40 + b) for b in range(3)])
    S = len(prob["num_nodes"])
    disp = np.stack([ft.teeth_dispersion(S) * (1.0 + 0.01 * b) for b in range(3)])
    disp[:, :, 3] = 2.0 - 0.5 * np.arange(3)[:, None]
    return prob, X, np.ascontiguousarray(disp)


def layout(prob):
    nn = [int(v) for v in prob["num_nodes"]]
    S, N = len(nn), sum(nn)
    return nn, S, N, N + S


def directions(prob, x):
    """the eleven seeds of a case at the vector x -> (dX [11, nvars], dD [11, S, 4])"""
    nn, S, N, M = layout(prob)
    nv = 11 * M + 2 * N + S + 1
    dX, dD = np.zeros((11, nv)), np.zeros((11, S, 4))
    dX[0, sidx(M, 0, 0)] = 1.0
    dX[1, sidx(M, 0, 2)] = 1.0
    dX[2, sidx(M, 0, 6)] = 1.0
    dD[3, :, 0] = 1.0
    dD[4, 2, 1] = 1.0
    dD[5, :, 2] = 1.0
    dD[6, :, 3] = 1.0
    dX[7, 11 * M + 2 * N + (2 if S > 3 else 1)] = 1.0
    free = [s for s in range(S) if not prob["attitude_hold"][s]][0]
    ua = sum(nn[:free])
    dX[8, 11 * M + 2 * (ua + np.arange(nn[free]))] = 1.0
    # the first knot across which the collocated mass drops (every knot of the noair case jumps: its first)
    xa = [sum(nn[:s]) + s for s in range(S)]
    drops = [s for s in range(1, S) if x[xa[s]] != x[xa[s] - 1]]
    drop = drops[0] if drops else 1        # (a vector whose knots are all continuous: its first knot)
    dX[9, xa[drop]] = 1.0
    rng = np.random.default_rng(30)
    dX[10] = rng.standard_normal(nv)
    dD[10] = rng.standard_normal((S, 4))
    return dX, dD


def segments(prob, mode):
    """[(phase, continues the previous segment's state)]: the order in which the flight's stages are stored"""
    S = len(prob["num_nodes"])
    return [(s, mode == "chain" and s > 0) for s in range(S)]


def steps_of(k, S):
    """k as one number of RK4 steps per node interval, or one per phase -> [S] integers"""
    if np.ndim(k) == 0:
        return [int(k)] * S
    ks = [int(v) for v in k]
    assert len(ks) == S, (ks, S)
    return ks


def recursion(prob, mode, k, x, mats, hs, st, dx, dd, mutate=None, value_err=None, num=float):
    """The tangent of the flight (chain, section or node mode, k steps per node interval: one number, or one per phase) of the vector x along the seed (dx [nvars],
    dd [S, 4]) from the per-stage data st = {"F" [T, 11], "J" [T, 11, 11], "Pu" [T, 11, 2], "Pf" [T, 11, 4], "Jw" [T, 3, 3]: the part
    of J[4:7, 1:4] that comes through the wind's slope} in stage order -> dy [M, 11] (and the bound E [M, 11] where value_err
    [T, 11] = what the values of F may differ by is given; fp64 only).  mats[s] = the plan's matrices of phase s; hs[s] its steps;
    x, dx, dd and st in the arithmetic `num` converts to (float, or mpmath.mpf with object arrays)."""
    nn, S, N, M = layout(prob)
    ks = steps_of(k, S)
    ut = num(float(prob["units"][4]))
    t0 = 11 * M + 2 * N
    dy_out = np.zeros((M, 11), dtype=object if num is not float else float)
    E_out = np.zeros((M, 11))
    T = 0
    dy = None
    Eb = np.zeros(11)
    want_E = value_err is not None
    for s, carried in segments(prob, mode):
        n, k = nn[s], ks[s]
        ua = sum(nn[:s])
        xa = ua + s
        rows0 = state_rows(M, xa)
        if carried:
            dj = dx[rows0] - dx[state_rows(M, xa - 1)]
            if mutate == "no_djump":
                dj = dj * 0
            moved = dy + dj
            if want_E:
                Eb = Eb + np.where(np.asarray(dj != 0, dtype=bool), U * (np.abs(dj.astype(float)) + np.abs(moved.astype(float))), 0.0)
            dy = moved
        else:
            dy = dx[rows0].copy()
            Eb = np.zeros(11)
        dy_out[xa] = dy
        E_out[xa] = Eb
        S_ = (x[t0 + s + 1] - x[t0 + s]) * ut / 2
        dS = (dx[t0 + s + 1] - dx[t0 + s]) * ut / 2
        if mutate == "no_dS":
            dS = dS * 0
        df = dd[s - 1] if mutate == "shift_factors" and s > 0 else (dd[s] * 0 if mutate == "shift_factors" else dd[s])
        hold = bool(prob["attitude_hold"][s])
        m = mats[s]
        du_nodes = dx[11 * M + 2 * ua:11 * M + 2 * (ua + n)].reshape(n, 2)
        for j in range(n):
            if mode == "node" and j > 0:        # every node interval starts from the collocated row: its seed, E = 0
                dy = dx[state_rows(M, xa + j)].copy()
                Eb = np.zeros(11)
            Sh = S_ * hs[s][j]
            dSh = dS * hs[s][j]
            for i in range(k):
                p = 2 * (k * j + i)
                acc = dacc = eacc = vacc = 0
                Fp = dFp = eFp = vFp = None
                for sg in range(4):
                    pp = p + ((sg + 1) >> 1)
                    a, da = ((0, 0), (Sh / 2, dSh / 2), (Sh / 2, dSh / 2), (Sh, dSh))[sg]
                    w = (1, 2, 2, 1)[sg]
                    dyt = dy if sg == 0 else dy + dFp * a + Fp * da
                    if hold:
                        dU = du_nodes[0] * 0
                    elif m["copy_u"][pp] >= 0:
                        dU = du_nodes[m["copy_u"][pp]]
                    else:
                        dU = np.array([sum(num(float(m["Wu"][pp, q])) * du_nodes[q, c] for q in range(n)) for c in range(2)], dtype=dy.dtype)
                    J = st["J"][T]
                    if mutate == "no_wind_slope":
                        J = J.copy()
                        J[4:7, 1:4] = J[4:7, 1:4] - st["Jw"][T]
                    dF = J.dot(dyt) + st["Pu"][T].dot(dU) + st["Pf"][T].dot(df)
                    F = st["F"][T]
                    if want_E:
                        aJ, aPu, aPf = np.abs(J.astype(float)), np.abs(st["Pu"][T].astype(float)), np.abs(st["Pf"][T].astype(float))
                        ayt, aU, af = np.abs(dyt.astype(float)), np.abs(dU.astype(float)), np.abs(df.astype(float))
                        eyt = Eb if sg == 0 else Eb + abs(float(a)) * eFp + abs(float(da)) * vFp
                        e = 8 * U * (aJ.dot(ayt) + aPu.dot(aU) + aPf.dot(af))
                        e[4:7] = (1e-12 + 1e-9 * aJ[4:7]).dot(ayt) + (1e-12 + 1e-9 * aPu[4:7]).dot(aU) + (1e-12 + 1e-9 * aPf[4:7]).dot(af)
                        e = e + aJ.dot(eyt)
                        eacc = eacc + w * e
                        vacc = vacc + w * value_err[T]
                        eFp, vFp = e, value_err[T]
                    acc = acc + F * w
                    dacc = dacc + dF * w
                    Fp, dFp = F, dF
                    T += 1
                dy = dy + dacc * (Sh / 6) + acc * (dSh / 6)
                if want_E:
                    Eb = Eb + abs(float(Sh)) / 6 * eacc + abs(float(dSh)) / 6 * vacc + 8 * U * np.abs(dy.astype(float))
            dy_out[xa + j + 1] = dy
            E_out[xa + j + 1] = Eb
    return (dy_out, E_out) if want_E else dy_out


def recursion_steps(flight):
    """RK4 steps of a flight (case, mode, steps per node interval: one number, or one per phase)"""
    prob, _X, _d = case(flight[0])
    nn = layout(prob)[0]
    return sum(k * n for k, n in zip(steps_of(flight[2], len(nn)), nn))


def plan_tables(E, k, mode="chain"):
    """(mats [S], hs [S]) of a plan of k steps per node interval (one number, or one per phase): the matrices as the library builds
    them and the steps as its host code forms them (one subtraction, one division)"""
    ks = steps_of(k, E.S)
    plan = E.propagation_plan(steps=ks, restart=mode)
    mats = [plan.matrices(s) for s in range(E.S)]
    plan.close()
    hs = []
    for s in range(E.S):
        tx = np.concatenate([[-1.0], E.tau(s)])
        hs.append((tx[1:] - tx[:-1]) / ks[s])
    return mats, hs


def load(flight):
    """the stored truth of one of FLIGHTS -> dict(dy [11, M, 11], dy_f, dy_b (the one-sided quotients), bound [11, M, 11] = E, and the
    per-stage data F, J, Pu, Pf, Jw, verr)"""
    g = np.load(G30)
    key = "%s_%s_k%d_" % flight
    return {name[len(key):]: g[name] for name in g.files if name.startswith(key)}


def unpack_dy(dY, M):
    """[..., M, 11] from the device's [..., 11 M]"""
    lead = dY.shape[:-1]
    return np.concatenate([dY[..., 0:M, None], dY[..., M:4 * M].reshape(lead + (M, 3)), dY[..., 4 * M:7 * M].reshape(lead + (M, 3)),
                           dY[..., 7 * M:11 * M].reshape(lead + (M, 4))], axis=-1)

"""What the tests of the wind-profile sensitivities share (include/gelato_amd.h gel_propagate_tangent_wind / gel_propagate_adjoint_wind;
DESIGN.md 3.23): the flights, the seeds on the wind table's values, the functionals, the host restatement of the row lookup
(gelato_amd/csrc/gel_wind_rows.h) and the two recursions, written once for any arithmetic -- the generator
(tests/golden/make_flight_wind.py) runs them on mpmath numbers with 80 digits, the tests run them in fp64 on the stored per-stage
partials to evaluate WRONG restatements (`mutate`), which give the bounds their teeth:

  "shift_piece"     the weights put on rows i - 1, i instead of i, i + 1 (row 0 stays row 0)
  "no_fw"           the looked-up seed not multiplied by the wind factor
  "ends_dropped"    zero instead of the end row's seed outside the table
  "theta_swapped"   the weights 1 - th and th exchanged

The map: with the altitudes x fixed, the wind a stage reads is fw (W[i] + (h - x[i]) (W[i + 1] - W[i]) / (x[i + 1] - x[i])) on the
piece x[i] < h <= x[i + 1], fw W[0] for h <= x[0], fw W[Kw - 1] for h > x[Kw - 1]: linear in W.  Along a seed dW:
  th = (h - x[i]) / (x[i + 1] - x[i]);   dw = fw (dW[i] + th (dW[i + 1] - dW[i]));   the end row's seed in a clamped end
and the tangent recursion of flight_tangent_truth.recursion gets one more forcing term per stage, Pw dw, with
Pw [11, 2] = dF / d(the scaled wind's north, east):
  dF = J dyt + Pu dU + Pf df + Pw dw
The bound E is flight_tangent_truth's, with the wind term carried in the same form as the factor term:
  velocity rows: + sum_c (1e-12 + 1e-9 |Pw_c|) |dw_c|;   the other rows: + 8u |Pw| |dw|
The adjoint is the transpose: a reversed stage's lw = Pw^T lF (lF as in flight_adjoint_truth.adjoint) goes, times fw, to rows i and
i + 1 with the weights 1 - th and th, in a clamped end wholly to the end row.  Its bound Eg, per row and component:
  e(lw) as flight_adjoint_truth's err(Pf);   Eg[row] += fw weight e(lw) + 4u |contribution|, and at the end (T + 2) u sum |contributions|
  for the T stages' read-add-write in walk order.

The flights of tests/golden/g36_flight_wind_plans.npz (PLAN_FLIGHTS; tests/golden/make_flight_wind_plans.py, tests/test_flight_wind_plans*.py)
run through the same two recursions: a node plan (every node interval restarts from the collocated row), the example under
mixed_steps.E_STEPS in chain and section mode, and the example over the two-row table.
"""
import os

import numpy as np

import flight_tangent_truth as tt
import mixed_steps as ms

U = tt.U
HERE = os.path.dirname(os.path.abspath(__file__))
G35 = os.path.join(HERE, "golden", "g35_flight_wind.npz")
TRUTH_VEC = tt.TRUTH_VEC
# (case, plan mode, steps per node interval): full per-stage data | inner checkpoints | 160 rows, the bisection path | stages
# outside the table on both sides, fw != 1
FLIGHTS = (("example", "chain", 1), ("example", "section", 2), ("example@LONG", "chain", 1), ("kinks@ENDS", "section", 1))
SEEDS = ("bump_north", "east_all", "scale", "row_first", "row_last", "dense", "mixed")
MUTATIONS = ("shift_piece", "no_fw", "ends_dropped", "theta_swapped")
NQ = 12   # the eleven terminal rows and one dense functional
# the flights of tests/golden/g36_flight_wind_plans.npz (tests/golden/make_flight_wind_plans.py; tests/test_flight_wind_plans*.py):
# a node plan (the tangent alone: the adjoint refuses node plans) | step counts that differ by phase, chain and section (inner
# checkpoints in air phases, k = 2 and k = 3) | the shortest table a handle takes: Kw = 2, one piece, both ends clamp onto its rows
G36 = os.path.join(HERE, "golden", "g36_flight_wind_plans.npz")
PLAN_FLIGHTS = {"W-node": ("example", "node", 1), "W-E-chain": ("example", "chain", ms.E_STEPS), "W-E-section": ("example", "section", ms.E_STEPS),
                "W-MIN": ("example@MIN", "chain", 1)}
PLAN_NAMES = tuple(PLAN_FLIGHTS)
PLAN_ADJOINT = ("W-E-chain", "W-E-section", "W-MIN")
PLAN_E = ("W-E-chain", "W-E-section")
# g36's counts: the bump row, air stages on the piece below / above it, air stages under / over the table with Pw != 0, air stages,
# air stages inside the table with Pw != 0, air stages of phases with k = 2 / k = 3, air stages of node intervals j >= 1
COUNTS = ("bump", "lo", "hi", "below", "above", "air", "inside", "air_k2", "air_k3", "air_j1")


def key(flight):
    return "%s_%s_k%d_" % flight


def lookup(h, alt, num=float):
    """the rows and the weight of the lookup at altitude h in the table whose altitudes are alt [Kw] -> (piece, i0, i1, th):
    gel_wind_rows.h's expression (piece as wind_ned2_centre returns it: -1 below, -2 above)"""
    Kw = len(alt)
    if h <= alt[0]:
        return -1, 0, 0, num(0.0)
    if h > alt[Kw - 1]:
        return -2, Kw - 1, Kw - 1, num(0.0)
    i = 0
    while not (alt[i] < h <= alt[i + 1]):
        i += 1
    return i, i, i + 1, (h - alt[i]) / (alt[i + 1] - alt[i])


def rows_of(piece, Kw):
    return (0, 0) if piece == -1 else ((Kw - 1, Kw - 1) if piece == -2 else (int(piece), int(piece) + 1))


def weights(piece, th, Kw, fw, mutate=None, num=float):
    """[(row, weight)]: what a stage's scaled wind takes from the table's rows (the tangent contracts the seed with it, the adjoint
    scatters along it)"""
    i0, i1 = rows_of(piece, Kw)
    f = num(1.0) if mutate == "no_fw" else fw
    if piece < 0:
        return [] if mutate == "ends_dropped" else [(i0, f)]
    if mutate == "shift_piece":
        i0, i1 = max(i0 - 1, 0), i0
    w0, w1 = (th, 1 - th) if mutate == "theta_swapped" else (1 - th, th)
    return [(i0, f * w0), (i1, f * w1)]


def on_kinks(flight):
    """every phase of tests/kink_flight.py's flights starts ON a kink of the right-hand side, where a dense dx has one-sided
    derivatives only (their conventions are g34's subject): there the mixed seed is the dense dW with the dense ddisp alone"""
    return flight[0].startswith("kinks")


def seeds(prob, x, stage_rows=None, with_dx=True):
    """the seven seeds of a case -> (dW [7, Kw, 2], dX [7, nvars], dD [7, S, 4]); stage_rows: for every air stage the rows of its
    piece (the bump goes to the row with the most adjacent stages; None: the middle row); with_dx = False: see on_kinks"""
    wt = np.asarray(prob["wind_table"], dtype=float)
    Kw = wt.shape[0]
    nn, S, N, M = tt.layout(prob)
    nv = 11 * M + 2 * N + S + 1
    dW, dX, dD = np.zeros((7, Kw, 2)), np.zeros((7, nv)), np.zeros((7, S, 4))
    dW[0, bump_row(Kw, stage_rows), 0] = 1.0
    dW[1, :, 1] = 1.0
    dW[2] = wt[:, 1:]
    dW[3, 0, :] = 1.0
    dW[4, Kw - 1, :] = 1.0
    rng = np.random.default_rng(35)
    dW[5] = rng.standard_normal((Kw, 2))
    dW[6] = dW[5]
    dX[6] = rng.standard_normal(nv) * (1.0 if with_dx else 0.0)
    dD[6] = rng.standard_normal((S, 4))
    return dW, dX, dD


def bump_row(Kw, stage_rows):
    if stage_rows is None:
        return Kw // 2
    cnt = np.zeros(Kw, dtype=int)
    for i0, i1 in stage_rows:
        if i1 != i0:
            cnt[i0] += 1
            cnt[i1] += 1
    return int(np.argmax(cnt))


def functionals(prob):
    """-> lam [12, M, 11]: the eleven terminal rows, then one dense functional"""
    nn, S, N, M = tt.layout(prob)
    lam = np.zeros((NQ, M, 11))
    for c in range(11):
        lam[c, M - 1, c] = 1.0
    lam[11] = np.random.default_rng(36).standard_normal((M, 11))
    return lam


def tangent(prob, mode, k, x, mats, hs, st, fws, dx, dd, dW, mutate=None, value_err=None, num=float):
    """flight_tangent_truth.recursion with the wind table's direction dW [Kw, 2]: st holds, besides F, J, Pu, Pf, the stages' Pw
    [T, 11, 2], piece [T] and th [T] (air [T]: whether the stage's phase reads the wind); fws [S]: the wind factors.
    -> dy [M, 11] (and E [M, 11] where value_err is given; fp64 only)"""
    nn, S, N, M = tt.layout(prob)
    ks = tt.steps_of(k, S)
    Kw = dW.shape[0]
    ut = num(float(prob["units"][4]))
    t0 = 11 * M + 2 * N
    dy_out = np.zeros((M, 11), dtype=object if num is not float else float)
    E_out = np.zeros((M, 11))
    T = 0
    dy = None
    Eb = np.zeros(11)
    want_E = value_err is not None
    for s, carried in tt.segments(prob, mode):
        n, k = nn[s], ks[s]
        ua = sum(nn[:s])
        xa = ua + s
        rows0 = tt.state_rows(M, xa)
        if carried:
            dj = dx[rows0] - dx[tt.state_rows(M, xa - 1)]
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
        df = dd[s]
        hold = bool(prob["attitude_hold"][s])
        m = mats[s]
        du_nodes = dx[11 * M + 2 * ua:11 * M + 2 * (ua + n)].reshape(n, 2)
        for j in range(n):
            if mode == "node" and j > 0:        # every node interval starts from the collocated row: its seed, E = 0
                dy = dx[tt.state_rows(M, xa + j)].copy()
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
                    dw = np.array([num(0.0), num(0.0)], dtype=dy.dtype)
                    if st["air"][T]:
                        for row, wgt in weights(int(st["piece"][T]), st["th"][T], Kw, fws[s], mutate, num):
                            dw = dw + dW[row] * wgt
                    J, Pw = st["J"][T], st["Pw"][T]
                    dF = J.dot(dyt) + st["Pu"][T].dot(dU) + st["Pf"][T].dot(df) + Pw.dot(dw)
                    F = st["F"][T]
                    if want_E:
                        fl = lambda v: np.abs(np.asarray(v, dtype=float))   # noqa: E731
                        aJ, aPu, aPf, aPw = fl(J), fl(st["Pu"][T]), fl(st["Pf"][T]), fl(Pw)
                        ayt, aU, af, aw = fl(dyt), fl(dU), fl(df), fl(dw)
                        eyt = Eb if sg == 0 else Eb + abs(float(a)) * eFp + abs(float(da)) * vFp
                        e = 8 * U * (aJ.dot(ayt) + aPu.dot(aU) + aPf.dot(af) + aPw.dot(aw))
                        e[4:7] = ((1e-12 + 1e-9 * aJ[4:7]).dot(ayt) + (1e-12 + 1e-9 * aPu[4:7]).dot(aU) + (1e-12 + 1e-9 * aPf[4:7]).dot(af)
                                  + (1e-12 + 1e-9 * aPw[4:7]).dot(aw))
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


def adjoint(prob, mode, k, x, hs, st, fws, lam, Kw, mutate=None, want_E=False, num=float):
    """The wind rows' part of the adjoint flight: flight_adjoint_truth.adjoint's backward walk of the state's multiplier, and per
    reversed stage lw = Pw^T lF scattered to the table's rows -> gW [Kw, 2] (and Eg [Kw, 2] with want_E; fp64 only)"""
    nn, S, N, M = tt.layout(prob)
    ks = tt.steps_of(k, S)
    ut = num(float(prob["units"][4]))
    t0 = 11 * M + 2 * N
    dt = object if num is not float else float
    zero = num(0.0)
    gW = np.full((Kw, 2), zero, dtype=dt)
    Eg, aG = np.zeros((Kw, 2)), np.zeros((Kw, 2))
    T0 = [4 * sum(ks[r] * nn[r] for r in range(s)) for s in range(S)]
    fl = lambda a: np.abs(np.asarray(a, dtype=float))   # noqa: E731
    lm, El = np.full(11, zero, dtype=dt), np.zeros(11)
    nst = 0
    for s in reversed(range(S)):
        n, k = nn[s], ks[s]
        xa = sum(nn[:s]) + s
        if not (mode == "chain" and s < S - 1):
            lm, El = np.full(11, zero, dtype=dt), np.zeros(11)
        lm = lm + lam[xa + n]
        if want_E:
            El = El + U * fl(lm)
        S_ = (x[t0 + s + 1] - x[t0 + s]) * ut / 2
        for j in reversed(range(n)):
            Sh = S_ * hs[s][j]
            for i in reversed(range(k)):
                Tb = T0[s] + 4 * (k * j + i)
                lacc = lm * (Sh / 6)
                e_lacc = abs(float(Sh)) / 6 * El + 2 * U * fl(lacc) if want_E else None
                lyt = e_lyt = None
                lsum, e_sum = 0, 0
                for sg in (3, 2, 1, 0):
                    a_next = (Sh / 2, Sh / 2, Sh, None)[sg]
                    w = (1, 2, 2, 1)[sg]
                    if sg == 3:
                        lF, e_lF = lacc, e_lacc
                    else:
                        lF = lacc * w + lyt * a_next
                        if want_E:
                            e_lF = w * e_lacc + abs(float(a_next)) * e_lyt + 2 * U * fl(lF)
                    J, Pw = st["J"][Tb + sg], st["Pw"][Tb + sg]
                    lyt, lw = J.T.dot(lF), Pw.T.dot(lF)
                    if want_E:
                        aF = fl(lF)
                        oth = aF.copy()
                        oth[4:7] = 0.0

                        def err(Mx):
                            aM = fl(Mx)
                            return (1e-12 + 1e-9 * aM[4:7]).T.dot(aF[4:7]) + 8 * U * aM.T.dot(oth) + aM.T.dot(e_lF)
                        e_lyt, e_lw = err(J), err(Pw)
                        e_sum = e_sum + e_lyt
                    if st["air"][Tb + sg]:
                        nst += 1
                        for row, wgt in weights(int(st["piece"][Tb + sg]), st["th"][Tb + sg], Kw, fws[s], mutate, num):
                            gW[row] = gW[row] + lw * wgt
                            if want_E:
                                c = fl(lw) * abs(float(wgt))
                                Eg[row] += abs(float(wgt)) * e_lw + 4 * U * c
                                aG[row] += c
                    lsum = lsum + lyt
                lm = lm + lsum
                if want_E:
                    El = El + e_sum + 8 * U * fl(lm)
            lm = lm + lam[xa + j]
            if want_E:
                El = El + U * fl(lm)
    return (gW, Eg + (nst + 2) * U * aG) if want_E else gW


def load(flight):
    """the stored truth of one of FLIGHTS -> dict without the flight's prefix"""
    g = np.load(G35)
    k = key(flight)
    return {name[len(k):]: g[name] for name in g.files if name.startswith(k)}


def load_plan(name):
    """the stored truth of one of PLAN_NAMES -> dict without the flight's prefix"""
    g = np.load(G36)
    k = name + "_"
    return {n[len(k):]: g[n] for n in g.files if n.startswith(k)}


def node_rows(nn):
    """(the state rows xa, xa + 1 of every phase: its start and the end of its first node interval, where a node plan and a section
    plan agree; the rows past them, where a node plan restarted from the collocated row and a section plan went on)"""
    first, later = [], []
    for s, n in enumerate(nn):
        xa = sum(nn[:s]) + s
        first += [xa, xa + 1]
        later += list(range(xa + 2, xa + n + 1))
    return np.array(first), np.array(later)


def miss_bounded(a, ref, bound):
    """the largest |a - ref| / bound over the entries that HAVE a bound: what the teeth are measured by (an entry that differs
    under a zero bound would make `miss` infinite and the teeth trivial)"""
    d = np.abs(np.asarray(a, dtype=float) - ref)
    ok = (bound > 0) & np.isfinite(d)
    return float((d[ok] / bound[ok]).max()) if ok.any() else 0.0


def miss(a, ref, bound):
    """the largest |a - ref| / bound; inf where an entry differs under a zero bound or is not finite"""
    d = np.abs(np.asarray(a, dtype=float) - ref)
    if np.any((bound == 0) & (d > 0)) or not np.all(np.isfinite(d)):
        return np.inf
    ok = bound > 0
    return float((d[ok] / bound[ok]).max()) if ok.any() else 0.0

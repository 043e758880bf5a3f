"""What the adjoint flight's tests share (include/gelato_amd.h gel_propagate_adjoint): the seven functionals and the
TRANSPOSE of flight_tangent_truth.recursion, written once for any arithmetic -- the generator (tests/golden/make_flight_adjoint.py)
runs it on mpmath numbers with 60 digits over g30's stored per-stage F, J, Pu, Pf, the tests run it in fp64 to evaluate WRONG
restatements (`mutate`), which give the bound its teeth:

  "no_gS"            the multiplier of the step S h dropped: a knot time then has no gradient
  "no_knot_minus"    at a chain knot the -l of the last node of phase s dropped
  "shift_factors"    the factor adjoint of phase s written to phase s + 1
  "copy_through_wu"  the stage points that ARE a collocation node sent through Wu as well as copied
  "no_stage4"        in lF3 = 2 lacc + Sh lyt4 the second term dropped

The recursion, walking backwards (l = the multiplier of the state; a = Sh/2, Sh/2, Sh into stages 2, 3, 4):
  lacc = Sh/6 l;  lF4 = lacc;  lF3 = 2 lacc + Sh lyt4;  lF2 = 2 lacc + Sh/2 lyt3;  lF1 = lacc + Sh/2 lyt2
  (lyt, lu, lf) = (J^T, Pu^T, Pf^T) lF;   l += lyt4 + lyt3 + lyt2 + lyt1
  gS += h (<l, acc>/6 + <lyt2, F1>/2 + <lyt3, F2>/2 + <lyt4, F3>)
and the bound Eg carried along it -- 3.20's per-stage contract transposed, no new number (u = 2^-53; the tests allow 2 Eg):
  e(J^T lF)  through the velocity rows of F: (1e-12 + 1e-9 |J_cd|)^T |lF_c|, c in 4..6 (which also covers J being
             evaluated on the device's own trajectory); through the other rows 8u |J|^T |lF|; plus |J|^T e(lF); the same on Pu, Pf
  e(lF)      = w e(lacc) + |a| e(lyt_next) + 2u |lF|;   e(lacc) = |Sh|/6 e(l) + 2u |lacc|
  e(l)      += sum e(lyt) + 8u |l|;   a lam row added: + u |l|
  e(gS)     += |h| (<e(l), |acc|>/6 + <|l|, v>/6 + <e(lyt_i), |F_i-1|> c_i + <|lyt_i|, v_i-1> c_i) + 16u |h| (sum of the |products|)
             with v = what the two sides' VALUES of F may differ by (g30's verr) and 16u = an 11-term fma chain, its scale and the sum
  controls   e(cell) = sum e(lu) + u |cell|;  e(gu_j) = sum_p |Wu_pj| e(cell_p) + (Pp + 2) u sum_p |Wu_pj cell_p|
  factors    e(gd) = sum e(lf) + (4 k n + 2) u sum |lf|        times: e(gt) = (e(gS_s-1) + e(gS_s)) unit_t/2 + 4u (|gS_s-1| + |gS_s|) unit_t/2
"""
import os

import numpy as np

import flight_tangent_truth as tt

U = tt.U
HERE = os.path.dirname(os.path.abspath(__file__))
G31 = os.path.join(HERE, "golden", "g31_flight_adjoint.npz")
FUNCTIONALS = ("terminal_mass", "terminal_x", "terminal_vz", "terminal_q1", "mid_phase2_vy", "behind_drop", "dense")
MUTATIONS = ("no_gS", "no_knot_minus", "shift_factors", "copy_through_wu", "no_stage4")
GROUPS = ("mass", "position", "velocity", "quaternion", "controls", "times", "factors")


def functionals(prob, x):
    """the seven functionals of a case at the vector x -> lam [7, M, 11] (weights on y, node by node)"""
    nn, S, N, M = tt.layout(prob)
    lam = np.zeros((7, M, 11))
    lam[0, M - 1, 0] = 1.0
    lam[1, M - 1, 1] = 1.0
    lam[2, M - 1, 6] = 1.0
    lam[3, M - 1, 8] = 1.0
    xa = [sum(nn[:s]) + s for s in range(S)]
    lam[4, xa[2] + nn[2] // 2, 5] = 1.0                      # a velocity row in the middle of phase 2
    drops = [s for s in range(1, S) if x[xa[s]] != x[xa[s] - 1]]
    drop = drops[0] if drops else 1
    lam[5, xa[drop], :] = 1.0                                 # the first node behind a stage drop: all eleven rows
    lam[6] = np.random.default_rng(31).standard_normal((M, 11))
    return lam


def pack_lam(lam):
    """[..., M, 11] -> the device's layout [..., 11 M] (like y)"""
    lead = lam.shape[:-2]
    return np.ascontiguousarray(np.concatenate([lam[..., 0], lam[..., 1:4].reshape(lead + (-1,)), lam[..., 4:7].reshape(lead + (-1,)),
                                                lam[..., 7:11].reshape(lead + (-1,))], axis=-1))


def groups(prob):
    """index sets of gx by group -> {"mass": idx, ..., "times": idx}"""
    nn, S, N, M = tt.layout(prob)
    return {"mass": np.arange(0, M), "position": np.arange(M, 4 * M), "velocity": np.arange(4 * M, 7 * M),
            "quaternion": np.arange(7 * M, 11 * M), "controls": np.arange(11 * M, 11 * M + 2 * N),
            "times": np.arange(11 * M + 2 * N, 11 * M + 2 * N + S + 1)}


def adjoint(prob, mode, k, x, mats, hs, st, lam, mutate=None, value_err=None, num=float):
    """The adjoint of the flight (chain or section mode, k steps per node interval: one number, or one per phase) of the vector x for the functional lam [M, 11] from
    the per-stage data st (flight_tangent_truth.recursion's) -> (gx [nvars], gd [S, 4]), and (Egx, Egd) behind them where value_err
    [T, 11] is given (fp64 only).  x, lam and st in the arithmetic `num` converts to."""
    nn, S, N, M = tt.layout(prob)
    nv = 11 * M + 2 * N + S + 1
    ks = tt.steps_of(k, S)
    ut = num(float(prob["units"][4]))
    t0 = 11 * M + 2 * N
    dt = object if num is not float else float
    zero = num(0.0)
    gx, gd = np.full(nv, zero, dtype=dt), np.full((S, 4), zero, dtype=dt)
    Egx, Egd = np.zeros(nv), np.zeros((S, 4))
    gS, EgS = [zero] * S, [0.0] * S
    want_E = value_err is not None
    T0 = [4 * sum(ks[r] * nn[r] for r in range(s)) for s in range(S)]
    fl = lambda a: np.abs(np.asarray(a, dtype=float))   # noqa: E731
    lm, El = np.full(11, zero, dtype=dt), np.zeros(11)
    for s in reversed(range(S)):
        n, k = nn[s], ks[s]
        ua = sum(nn[:s])
        xa = ua + s
        if not (mode == "chain" and s < S - 1):
            lm, El = np.full(11, zero, dtype=dt), np.zeros(11)
        lm = lm + lam[xa + n]
        if want_E:
            El = El + U * fl(lm)
        S_ = (x[t0 + s + 1] - x[t0 + s]) * ut / 2
        hold = bool(prob["attitude_hold"][s])
        m = mats[s]
        Pp = 2 * k * n + 1
        cell, Ecell = np.full((Pp, 2), zero, dtype=dt), np.zeros((Pp, 2))
        gf, Egf, agf = np.full(4, zero, dtype=dt), np.zeros(4), np.zeros(4)
        for j in reversed(range(n)):
            h = hs[s][j]
            Sh = S_ * h
            for i in reversed(range(k)):
                p = 2 * (k * j + i)
                Tb = T0[s] + 4 * (k * j + i)
                F = [st["F"][Tb + sg] for sg in range(4)]
                acc = F[0] + F[1] * 2 + F[2] * 2 + F[3]
                lacc = lm * (Sh / 6)
                e_lacc = abs(float(Sh)) / 6 * El + 2 * U * fl(lacc) if want_E else None
                lyt = e_lyt = None
                lsum, e_sum = 0, 0
                step = (lm * acc).sum() / 6
                e_step = (((El * fl(acc)).sum() + (fl(lm) * (value_err[Tb] + 2 * value_err[Tb + 1] + 2 * value_err[Tb + 2] + value_err[Tb + 3])).sum()) / 6
                          if want_E else 0.0)
                a_step = float(abs(step))
                for sg in (3, 2, 1, 0):
                    pp = p + ((sg + 1) >> 1)
                    a_next = (Sh / 2, Sh / 2, Sh, None)[sg]
                    w = (1, 2, 2, 1)[sg]
                    if sg == 3:
                        lF, e_lF = lacc, e_lacc
                    else:
                        lF = lacc * w if (mutate == "no_stage4" and sg == 2) else lacc * w + lyt * a_next
                        if want_E:
                            e_lF = w * e_lacc + abs(float(a_next)) * e_lyt + 2 * U * fl(lF)
                    J, Pu, Pf = st["J"][Tb + sg], st["Pu"][Tb + sg], st["Pf"][Tb + sg]
                    lyt, lu, lf = J.T.dot(lF), Pu.T.dot(lF), Pf.T.dot(lF)
                    if want_E:
                        aF = fl(lF)
                        vel, oth = np.zeros(11), aF.copy()
                        vel[4:7] = aF[4:7]
                        oth[4:7] = 0.0

                        def err(Mx):
                            aM = fl(Mx)
                            return (1e-12 + 1e-9 * aM[4:7]).T.dot(aF[4:7]) + 8 * U * aM.T.dot(oth) + aM.T.dot(e_lF)
                        e_lyt, e_lu, e_lf = err(J), err(Pu), err(Pf)
                        e_sum = e_sum + e_lyt
                        Ecell[pp] = Ecell[pp] + e_lu + U * fl(cell[pp] + lu)
                        Egf = Egf + e_lf
                        agf = agf + fl(lf)
                    cell[pp] = cell[pp] + lu
                    gf = gf + lf
                    lsum = lsum + lyt
                    if sg:
                        c = 1 if sg == 3 else num(0.5)
                        term = (lyt * F[sg - 1]).sum() * c
                        step = step + term
                        if want_E:
                            e_step += float(c) * ((e_lyt * fl(F[sg - 1])).sum() + (fl(lyt) * value_err[Tb + sg - 1]).sum())
                            a_step += float(abs(term))
                if mutate != "no_gS":
                    gS[s] = gS[s] + step * h
                lm = lm + lsum
                if want_E:
                    EgS[s] += abs(float(h)) * (e_step + 16 * U * a_step)
                    El = El + e_sum + 8 * U * fl(lm)
            lm = lm + lam[xa + j]
            if want_E:
                El = El + U * fl(lm)
        rows0 = tt.state_rows(M, xa)
        gx[rows0] = lm
        Egx[rows0] = El
        if mode == "chain" and s > 0:
            prev = tt.state_rows(M, xa - 1)
            if mutate != "no_knot_minus":
                gx[prev] = zero - lm
            Egx[prev] = El
        if not hold:
            W = m["Wu"]
            cols = [[] for _ in range(n)]
            for pp in range(Pp):
                cu = int(m["copy_u"][pp])
                if cu >= 0:
                    cols[cu].append((pp, None))
                    if mutate != "copy_through_wu":
                        continue
                for q in range(n):
                    cols[q].append((pp, num(float(W[pp, q]))))
            for q in range(n):
                for c in range(2):
                    v, e, a = zero, 0.0, 0.0
                    for pp, wq in cols[q]:
                        t = cell[pp, c] if wq is None else cell[pp, c] * wq
                        v = v + t
                        if want_E:
                            e += Ecell[pp, c] * (1.0 if wq is None else abs(float(wq)))
                            a += abs(float(t))
                    gx[11 * M + 2 * (ua + q) + c] = v
                    Egx[11 * M + 2 * (ua + q) + c] = e + (Pp + 2) * U * a
        sd = s + 1 if mutate == "shift_factors" else s
        if sd < S:
            gd[sd] = gf
        Egd[s] = Egf + (4 * k * n + 2) * U * agf
    for i in range(S + 1):
        a = gS[i - 1] if i > 0 else zero
        b = gS[i] if i < S else zero
        gx[t0 + i] = (a - b) * ut / 2
        if want_E:
            ea = (EgS[i - 1] if i > 0 else 0.0) + (EgS[i] if i < S else 0.0)
            gx_abs = abs(float(a)) + abs(float(b))
            Egx[t0 + i] = (ea + 4 * U * gx_abs) * float(ut) / 2
    return (gx, gd, Egx, Egd) if want_E else (gx, gd)


def load(flight):
    """the stored truth of one of tt.FLIGHTS -> dict(gx [7, nvars], gdisp [7, S, 4], Egx, Egd)"""
    g = np.load(G31)
    key = "%s_%s_k%d_" % flight
    return {name[len(key):]: g[name] for name in g.files if name.startswith(key)}


def miss(a, ref, bound):
    """the largest |a - ref| / bound; inf where an entry differs under a zero bound or is not finite"""
    d = np.abs(np.asarray(a, dtype=float) - ref)
    if np.any((bound == 0) & (d > 0)) or not np.all(np.isfinite(d)):
        return np.inf
    ok = bound > 0
    return float((d[ok] / bound[ok]).max()) if ok.any() else 0.0

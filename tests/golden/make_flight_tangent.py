#!/usr/bin/env python3
"""Ground truth of the tangent-linear propagation (tests/golden/g30_flight_tangent.npz) for tests/test_flight_tangent*.py.

Needs mpmath (the tests read the .npz).  The discrete RK4 map of gel_propagate_dispersed* (gelato_amd/csrc/gel_prop.h) is evaluated in
60-digit arithmetic on the fp64 inputs the device gets -- x, the factors, the tables, the units, and the plan's stage points, control
matrix and step fractions from gel_prop_matrices on a host-only handle -- with the right-hand side composed from oracle/exact_fd.py's
functions as tests/golden/make_exact_jac.py composes them, and differentiated along every seed of
tests/flight_tangent_truth.py in two ways:
  (a) differences of the WHOLE map with h = 1e-25: the central quotient, and the forward and the backward one (where they
      disagree a kink lies within h of some stage);
  (b) the tangent recursion (flight_tangent_truth.recursion) with the per-stage J = dF/dX (11 x 11) and the partials along the
      controls and the factors, themselves central differences of the right-hand side.  The bound E is carried along (b).
Stored per flight: dy (b), dy_a / dy_f / dy_b (a), bound, and the per-stage F, J, Pu, Pf, Jw (the part of J that comes through
the wind's slope: J minus J with the wind held at the stage's value), verr (propagate_truth._dF); for the flights over the long tables
(flight_tangent_truth.TABLE_FLIGHTS) dy, bound and the largest distance of the one-sided quotients alone.

Usage:  python tests/golden/make_flight_tangent.py"""
import os
import sys
import time
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

from mpmath import mp, mpf  # noqa: E402

import make_exact_jac as mj  # noqa: E402

H = "1e-25"


def M_(v):
    return mpf(float(v))


def marr(a):
    a = np.asarray(a, dtype=float)
    out = np.empty(a.shape, dtype=object)
    for i in np.ndindex(a.shape):
        out[i] = mpf(float(a[i]))
    return out


class Ctx:
    """everything a flight reads besides x and the factors, as exact mpf of the fp64 numbers the device holds"""

    def __init__(self, name, mode, k):
        """k: RK4 steps per node interval, one number or one per phase"""
        import flight_tangent_truth as tt
        import interp_truth as it
        self.X = mj._setup()
        self.name, self.mode, self.k = name, mode, k
        self.prob, self.Xb, self.disp = tt.case(name)
        self.E = it.engine(self.prob)
        self.nn, self.S, self.N, self.M = tt.layout(self.prob)
        self.ks = tt.steps_of(k, self.S)
        self.mats, self.hs = tt.plan_tables(self.E, k, mode)
        um, up, uv, uu, ut = [float(v) for v in self.prob["units"]]
        self.units = [M_(um), M_(up), M_(uv)]
        self.uu, self.ut = M_(uu), M_(ut)
        self.vp = M_(uv / up)                                                      # the plan's fp64 quotient
        self.mf_um = [M_(-float(self.prob["massflow"][s]) / um) for s in range(self.S)]   # the handle's fp64 quotient
        wt, ct = np.asarray(self.prob["wind_table"]), np.asarray(self.prob["ca_table"])
        self.wind = [[M_(a) for a in wt[:, c]] for c in range(3)]
        self.ca = [[M_(a) for a in ct[:, c]] for c in range(2)]
        self.thrust = [M_(v) for v in self.prob["thrust"]]
        self.area = [M_(v) for v in self.prob["reference_area"]]
        self.nozzle = [M_(v) for v in self.prob["nozzle_area"]]

    def rhs(self, s, z, u, f, t, wind=None):
        """F [11] of phase s at the state z, controls u, factors f and normalised time t"""
        wind = wind or self.wind
        F = [mpf(0)] * 11
        if self.prob["engine_on"][s]:
            F[0] = self.mf_um[s] * f[1]
        for c in range(3):
            F[1 + c] = z[4 + c] * self.vp
        ws = [wind[0], [w * f[3] for w in wind[1]], [w * f[3] for w in wind[2]]]
        F[4:7] = mj.rhs(self.X, z[0], z[1:4], z[4:7], z[7:11], t, self.thrust[s] * f[0], self.area[s] * f[2], self.nozzle[s], ws,
                        self.ca, self.units)
        if not self.prob["attitude_hold"][s]:
            F[7:11] = mj.quat_rhs(z[7:11], u, self.uu)
        return F

    def frozen_wind(self, s, z, t):
        """a wind table that is constant at the stage's own wind: the right-hand side without the wind's slope"""
        if self.area[s] == 0:
            return None
        r = [c * self.units[1] for c in z[1:4]]
        v = [c * self.units[2] for c in z[4:7]]
        _va, h = self.X.air_velocity(r, v, t, self.wind)
        wn, we = self.X.interp(h, self.wind[0], self.wind[1]), self.X.interp(h, self.wind[0], self.wind[2])
        return [[mpf(0), mpf(1)], [wn, wn], [we, we]]

    def fly(self, x, fac, stages=None):
        """the flight of x [nvars] under fac [S][4] -> y [M][11]; stages: a list that receives (s, z, u, t) of every stage"""
        import flight_tangent_truth as tt
        M, N = self.M, self.N
        t0 = 11 * M + 2 * N
        Y = [None] * M
        y = None
        for s, carried in tt.segments(self.prob, self.mode):
            n = self.nn[s]
            ua = sum(self.nn[:s])
            xa = ua + s
            rows = tt.state_rows(M, xa)
            if carried:
                prev = tt.state_rows(M, xa - 1)
                y = [y[c] + (x[rows[c]] - x[prev[c]]) for c in range(11)]
            else:
                y = [x[i] for i in rows]
            Y[xa] = list(y)
            to, tf = x[t0 + s], x[t0 + s + 1]
            S_ = (tf - to) * self.ut / 2
            m = self.mats[s]
            Uc = [[x[11 * M + 2 * (ua + q) + c] for c in range(2)] for q in range(n)]
            hold = bool(self.prob["attitude_hold"][s])
            for j in range(n):
                if self.mode == "node" and j > 0:
                    y = [x[i] for i in tt.state_rows(M, xa + j)]
                Sh = S_ * M_(self.hs[s][j])
                for i in range(self.ks[s]):
                    p = 2 * (self.ks[s] * j + i)
                    acc, Fp = None, None
                    for sg in range(4):
                        pp = p + ((sg + 1) >> 1)
                        a = (0, Sh / 2, Sh / 2, Sh)[sg]
                        w = (1, 2, 2, 1)[sg]
                        yt = list(y) if sg == 0 else [y[c] + a * Fp[c] for c in range(11)]
                        if hold:
                            u = [mpf(0), mpf(0)]
                        elif m["copy_u"][pp] >= 0:
                            u = Uc[m["copy_u"][pp]]
                        else:
                            u = [sum(M_(m["Wu"][pp, q]) * Uc[q][c] for q in range(n)) for c in range(2)]
                        t = M_(m["pts"][pp]) * (tf - to) / 2 + (tf + to) / 2
                        if stages is not None:
                            stages.append((s, yt, u, t))
                        Fp = self.rhs(s, yt, u, fac[s], t)
                        acc = [w * v for v in Fp] if sg == 0 else [acc[c] + w * Fp[c] for c in range(11)]
                    y = [y[c] + Sh / 6 * acc[c] for c in range(11)]
                Y[xa + j + 1] = list(y)
        return Y


_CTX = {}


def ctx_of(flight):
    if flight not in _CTX:
        _CTX[flight] = Ctx(*flight)
    return _CTX[flight]


def stage_partials(job):
    """J, Pu, Pf, Jw and F of one stage by central differences of the right-hand side"""
    flight, s, z, u, t, fac = job
    C = ctx_of(flight)
    h = mpf(H)
    F = C.rhs(s, z, u, fac, t)
    J, Pu, Pf, Jw = np.zeros((11, 11), dtype=object), np.zeros((11, 2), dtype=object), np.zeros((11, 4), dtype=object), np.zeros((3, 3), dtype=object)

    def quot(zp, up_, fp, zm, um_, fm, wind=None):
        a, b = C.rhs(s, zp, up_, fp, t, wind), C.rhs(s, zm, um_, fm, t, wind)
        return [(a[c] - b[c]) / (2 * h) for c in range(11)]

    for d in range(11):
        zp, zm = list(z), list(z)
        zp[d] += h
        zm[d] -= h
        J[:, d] = quot(zp, u, fac, zm, u, fac)
    for d in range(2):
        up_, um_ = list(u), list(u)
        up_[d] += h
        um_[d] -= h
        Pu[:, d] = quot(z, up_, fac, z, um_, fac)
    for d in range(4):
        fp, fm = list(fac), list(fac)
        fp[d] += h
        fm[d] -= h
        Pf[:, d] = quot(z, u, fp, z, u, fm)
    Jw[:, :] = mpf(0)
    wf = C.frozen_wind(s, z, t)
    if wf is not None:
        for d in range(3):
            zp, zm = list(z), list(z)
            zp[1 + d] += h
            zm[1 + d] -= h
            q = quot(zp, u, fac, zm, u, fac, wind=wf)
            for c in range(3):
                Jw[c, d] = J[4 + c, 1 + d] - q[4 + c]
    return np.array(F, dtype=object), J, Pu, Pf, Jw


def whole_map(job):
    """(a): the three quotients of the whole map along one seed"""
    flight, x, fac, dx, dd = job
    C = ctx_of(flight)
    h = mpf(H)
    xm_, fm_ = marr(x), marr(fac)
    dxm, ddm = marr(dx), marr(dd)
    y0 = C.fly(list(xm_), [list(r) for r in fm_])
    yp = C.fly(list(xm_ + h * dxm), [list(r) for r in fm_ + h * ddm])
    ym = C.fly(list(xm_ - h * dxm), [list(r) for r in fm_ - h * ddm])
    M = C.M
    c_, f_, b_ = (np.zeros((M, 11), dtype=object) for _ in range(3))
    for i in range(M):
        for c in range(11):
            c_[i, c] = (yp[i][c] - ym[i][c]) / (2 * h)
            f_[i, c] = (yp[i][c] - y0[i][c]) / h
            b_[i, c] = (y0[i][c] - ym[i][c]) / h
    return c_, f_, b_


def value_errors(C, x, fac, stages, Fs):
    """what the two sides' values of F may differ by at every stage (propagate_truth._dF, with the control samples' own bound)"""
    import flight_truth as ft
    import mesh_truth as mt
    import propagate_truth as pt
    out = np.zeros((len(stages), 11))
    dUs = {}
    for s in range(C.S):
        if not C.prob["attitude_hold"][s]:
            dUs[s] = pt.samples(C.mats[s], mt.phase_state(C.E, x, s)[1])[1]
    T = 0
    for s, _carried in __import__("flight_tangent_truth").segments(C.prob, C.mode):
        n = C.nn[s]
        pd = ft.dispersed_prob(C.prob, s, fac[s])
        for j in range(n):
            for i in range(C.ks[s]):
                p = 2 * (C.ks[s] * j + i)
                for sg in range(4):
                    pp = p + ((sg + 1) >> 1)
                    _s, z, u, _t = stages[T]
                    zf = np.array([float(v) for v in z])
                    uf = np.array([float(v) for v in u])
                    out[T] = pt._dF(pd, s, zf, uf, dUs[s][pp] if s in dUs else np.zeros(2), np.array([float(v) for v in Fs[T]]))
                    T += 1
    return out


def flight_truth(flight, pool, compact=False):
    import flight_tangent_truth as tt
    C = ctx_of(flight)
    x, fac = C.Xb[tt.TRUTH_VEC], C.disp[tt.TRUTH_VEC]
    dX, dD = tt.directions(C.prob, x)
    xm_, fm_ = marr(x), marr(fac)
    stages = []
    y = C.fly(list(xm_), [list(r) for r in fm_], stages)
    res = pool.map(stage_partials, [(flight, s, z, u, t, list(fm_[s])) for s, z, u, t in stages])
    st = {"F": np.array([r[0] for r in res]), "J": np.array([r[1] for r in res]), "Pu": np.array([r[2] for r in res]),
          "Pf": np.array([r[3] for r in res]), "Jw": np.array([r[4] for r in res])}
    verr = value_errors(C, x, fac, stages, st["F"])
    quots = pool.map(whole_map, [(flight, x, fac, dX[d], dD[d]) for d in range(11)])
    M = C.M
    out = {k: np.zeros((11, M, 11)) for k in ("dy", "dy_a", "dy_f", "dy_b", "bound")}
    ab = np.zeros(11)
    for d in range(11):
        dy, Eb = tt.recursion(C.prob, C.mode, C.k, xm_, C.mats, C.hs, st, marr(dX[d]), marr(dD[d]), value_err=verr, num=M_)
        ca, cf, cb = quots[d]
        big = max(abs(v) for v in dy.ravel())
        worst = max(abs(a - b) for a, b in zip(dy.ravel(), ca.ravel()))
        ab[d] = float(worst / big) if big != 0 else float(worst)   # (a direction that moves nothing: area and wind without air)
        out["dy"][d] = dy.astype(float)
        out["dy_a"][d], out["dy_f"][d], out["dy_b"][d] = ca.astype(float), cf.astype(float), cb.astype(float)
        out["bound"][d] = Eb
    out["ab"] = ab
    out["y"] = np.array([[float(v) for v in row] for row in y])
    out["x"], out["disp"] = x, fac
    if compact:     # dy and its bound; of (a) only how far the one-sided quotients are apart, per direction, relative to the largest entry
        out["fb"] = np.array([np.abs(out["dy_f"][d] - out["dy_b"][d]).max() / max(np.abs(out["dy"][d]).max(), 1e-300) for d in range(11)])
        for k in ("dy_a", "dy_f", "dy_b"):
            del out[k]
        return out
    for k, v in st.items():
        out[k] = v.astype(float)
    out["verr"] = verr
    return out


def main():
    import flight_tangent_truth as tt
    mj._setup()
    out = {}
    with Pool(min(16, os.cpu_count() or 1)) as pool:
        for flight in tt.FLIGHTS + tt.TABLE_FLIGHTS:
            t0 = time.time()
            r = flight_truth(flight, pool, compact=flight in tt.TABLE_FLIGHTS)
            for k, v in r.items():
                out["%s_%s_k%d_%s" % (flight + (k,))] = v
            print("%s %s k=%d: %d stages, (a) against (b) at most %.2e of a direction's largest entry, %.1f s"
                  % (flight + (4 * tt.recursion_steps(flight), r["ab"].max(), time.time() - t0)))
    np.savez_compressed(tt.G30, **out)


if __name__ == "__main__":
    main()

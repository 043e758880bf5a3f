#!/usr/bin/env python3
"""Ground truth of the wind-profile sensitivities (tests/golden/g35_flight_wind.npz) for tests/test_flight_wind*.py.

Needs mpmath (the tests read the .npz) and the built library (a host-only handle gives the plan's matrices and steps).  Built on
make_flight_tangent.py: its Ctx flies the discrete RK4 map of gel_propagate_dispersed* in 60-digit arithmetic on the fp64 inputs
the device gets, and its rhs takes a replaced wind table.  With the table's altitudes fixed the flight is a function of the table's
values W [Kw][2]; along every seed of flight_wind_truth.seeds it is differentiated in two ways:
  (a) differences of the WHOLE map, the table's values moved along the seed (and x, the factors along the mixed seed's other
      parts), h = 1e-25: central, forward and backward;
  (b) flight_wind_truth.tangent: make_flight_tangent's per-stage J, Pu, Pf and Pw = dF / d(scaled wind north, east) -- a central
      difference of the right-hand side over a table frozen at the stage's own scaled wind, factor 1 -- with the stage's
      (piece, th) of the lookup at its exact altitude.  The bound E is carried along (b).
The adjoint truth is flight_wind_truth.adjoint on the same per-stage data, for the twelve functionals, with its bound Eg.
Asserted here (and again by tests/test_flight_wind_cpu.py from what is stored): (a) against (b); forward against backward; the bump
row has stages in both adjacent pieces; the ENDS flight has air stages below and above the table with Pw != 0; duality
<lam, T_w dW> = <gW, dW> and the scaling identity (the "scale" seed's dy = the dy of ddisp[:, 3] = fw) to 1e-50.
Stored per flight: x, disp, dW, dy, bound, ab, fb, gW, Eg, dual, dy_fw, bound_fw, scale_id, counts; for the first flight the
stages' Pw, piece, th, air (its F, J, Pu, Pf, verr are g30's: the same flight of the same vector).

DIGITS: 80, not make_flight_tangent's 60.  A wind row moves the normalised state by 1e-6 .. 1e-10 per m/s, and a quotient over
h = 1e-25 leaves such an entry 60 - 25 - 6 .. 10 digits: at 60 digits (a) against (b) stands at 1e-29 .. 1e-25 of a direction's largest
entry -- the quotients' own rounding, where g30's directions of order one reach 1e-32.  At 80 digits the figure is the
truncation's, as there.

Usage:  python tests/golden/make_flight_wind.py"""
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
import make_flight_tangent as mft  # noqa: E402
from make_flight_tangent import H, M_, marr  # noqa: E402

DPS = 80


def ctx_of(flight):
    """make_flight_tangent's context (its constructor sets 60 digits), then this file's precision"""
    C = mft.ctx_of(flight)
    mp.dps = DPS
    return C


def wind_partials(job):
    """make_flight_tangent.stage_partials, and Pw [11, 2], (piece, th) and whether the stage reads the wind"""
    import flight_wind_truth as wt
    flight, s, z, u, t, fac = job
    C = ctx_of(flight)
    h = mpf(H)
    F, J, Pu, Pf, _Jw = mft.stage_partials(job)
    Pw = np.full((11, 2), mpf(0), dtype=object)
    wf = C.frozen_wind(s, z, t)
    if wf is None:
        return F, J, Pu, Pf, Pw, 0, mpf(0), 0
    one = list(fac)
    one[3] = mpf(1)
    sc = [wf[1][0] * fac[3], wf[2][0] * fac[3]]         # the stage's scaled wind
    for c in range(2):
        p, m = list(sc), list(sc)
        p[c] += h
        m[c] -= h
        a = C.rhs(s, z, u, one, t, [[mpf(0), mpf(1)], [p[0], p[0]], [p[1], p[1]]])
        b = C.rhs(s, z, u, one, t, [[mpf(0), mpf(1)], [m[0], m[0]], [m[1], m[1]]])
        for r in range(11):
            Pw[r, c] = (a[r] - b[r]) / (2 * h)
    # (the frozen table reproduces the stage's F: the value the device forms from the scaled wind)
    F0 = C.rhs(s, z, u, one, t, [[mpf(0), mpf(1)], [sc[0], sc[0]], [sc[1], sc[1]]])
    assert max(abs(F0[r] - F[r]) for r in range(11)) < mpf("1e-50")
    r_ = [c * C.units[1] for c in z[1:4]]
    v_ = [c * C.units[2] for c in z[4:7]]
    _va, alt = C.X.air_velocity(r_, v_, t, C.wind)
    piece, _i0, _i1, th = wt.lookup(alt, C.wind[0], num=M_)
    return F, J, Pu, Pf, Pw, piece, th, 1


def whole_map(job):
    """(a): the three quotients of the whole map along one seed (dW on the table's values, dx, dd)"""
    flight, x, fac, dx, dd, dW = job
    C = ctx_of(flight)
    h = mpf(H)
    xm_, fm_ = marr(x), marr(fac)
    dxm, ddm, dWm = marr(dx), marr(dd), marr(dW)
    base = C.wind

    def fly(sign):
        C.wind = [base[0], [base[1][r] + sign * h * dWm[r, 0] for r in range(len(base[0]))],
                  [base[2][r] + sign * h * dWm[r, 1] for r in range(len(base[0]))]]
        try:
            return C.fly(list(xm_ + sign * h * dxm), [list(r) for r in fm_ + sign * h * ddm])
        finally:
            C.wind = base
    y0, yp, ym = fly(0), fly(1), fly(-1)
    M = C.M
    c_, f_, b_ = (np.zeros((M, 11), dtype=object) for _ in range(3))
    for i in range(M):
        for c in range(11):
            c_[i, c] = (yp[i][c] - ym[i][c]) / (2 * h)
            f_[i, c] = (yp[i][c] - y0[i][c]) / h
            b_[i, c] = (y0[i][c] - ym[i][c]) / h
    return c_, f_, b_


def flight_truth(flight, pool, first):
    import flight_tangent_truth as tt
    import flight_wind_truth as wt
    C = ctx_of(flight)
    x, fac = C.Xb[wt.TRUTH_VEC], C.disp[wt.TRUTH_VEC]
    xm_, fm_ = marr(x), marr(fac)
    stages = []
    C.fly(list(xm_), [list(r) for r in fm_], stages)
    res = pool.map(wind_partials, [(flight, s, z, u, t, list(fm_[s])) for s, z, u, t in stages])
    st = {"F": np.array([r[0] for r in res]), "J": np.array([r[1] for r in res]), "Pu": np.array([r[2] for r in res]),
          "Pf": np.array([r[3] for r in res]), "Pw": np.array([r[4] for r in res]), "piece": np.array([r[5] for r in res]),
          "th": np.array([r[6] for r in res], dtype=object), "air": np.array([r[7] for r in res])}
    verr = mft.value_errors(C, x, fac, stages, st["F"])
    Kw = len(C.wind[0])
    air = st["air"] == 1
    stage_rows = [wt.rows_of(int(p), Kw) for p in st["piece"][air]]
    dW, dX, dD = wt.seeds(C.prob, x, stage_rows, not wt.on_kinks(flight))
    nsd = len(wt.SEEDS)
    fws = [fm_[s][3] for s in range(C.S)]
    quots = pool.map(whole_map, [(flight, x, fac, dX[d], dD[d], dW[d]) for d in range(nsd)])
    M = C.M
    out = {"dy": np.zeros((nsd, M, 11)), "bound": np.zeros((nsd, M, 11)), "ab": np.zeros(nsd), "fb": np.zeros(nsd)}
    dys = []
    for d in range(nsd):
        dy, Eb = wt.tangent(C.prob, C.mode, C.k, xm_, C.mats, C.hs, st, fws, marr(dX[d]), marr(dD[d]), marr(dW[d]), value_err=verr, num=M_)
        ca, cf, cb = quots[d]
        big = max(abs(v) for v in dy.ravel())
        big = big if big != 0 else mpf(1)       # (a row no stage touches moves nothing: the end rows of a table the flight stays inside)
        out["ab"][d] = float(max(abs(a - b) for a, b in zip(dy.ravel(), ca.ravel())) / big)
        out["fb"][d] = float(max(abs(a - b) for a, b in zip(cf.ravel(), cb.ravel())) / big)
        out["dy"][d], out["bound"][d] = dy.astype(float), Eb
        dys.append(dy)
    # the conditions that keep the tests from being vacuous
    assert out["ab"].max() < 1e-30, out["ab"]          # the level g30 reaches (its worst: 8.6e-33) with h = 1e-25
    assert out["fb"].max() < 1e-20, out["fb"]          # one-sided quotients O(h) apart: no stage within h of a breakpoint
    bump = wt.bump_row(Kw, stage_rows)
    lo = sum(1 for i0, i1 in stage_rows if i1 != i0 and i1 == bump)
    hi = sum(1 for i0, i1 in stage_rows if i1 != i0 and i0 == bump)
    nz = np.array([max(abs(v) for v in P.ravel()) > 0 for P in st["Pw"]])
    below = int(np.sum(air & (st["piece"] == -1) & nz))
    above = int(np.sum(air & (st["piece"] == -2) & nz))
    assert lo > 0 and hi > 0, (flight, bump, lo, hi)
    if flight[0] == "kinks@ENDS":
        assert below > 0 and above > 0, (below, above)
        assert any(float(f) != 1.0 for f in fws)
    out["counts"] = np.array([bump, lo, hi, below, above, int(air.sum())])
    # the adjoint, and duality against (b) for the five pure wind seeds and the dense one
    lam = wt.functionals(C.prob)
    out["gW"], out["Eg"] = np.zeros((wt.NQ, Kw, 2)), np.zeros((wt.NQ, Kw, 2))
    dual = mpf(0)
    for q in range(wt.NQ):
        lq = marr(lam[q])
        gW = wt.adjoint(C.prob, C.mode, C.k, xm_, C.hs, st, fws, lq, Kw, num=M_)
        _g, Eg = wt.adjoint(C.prob, C.mode, C.k, x, C.hs, {k: (v.astype(float) if k in ("J", "Pw", "th") else v) for k, v in st.items()},
                            [float(f) for f in fws], lam[q], Kw, want_E=True)
        out["gW"][q], out["Eg"][q] = gW.astype(float), Eg
        for d in range(6):
            lhs = sum(a * b for a, b in zip(lq.ravel(), dys[d].ravel()))
            rhs = sum(a * b for a, b in zip(gW.ravel(), marr(dW[d]).ravel()))
            scale = max(abs(lhs), abs(rhs), mpf(1))
            dual = max(dual, abs(lhs - rhs) / scale)
    assert dual < mpf("1e-50"), dual
    out["dual"] = np.array(float(dual))
    # the scaling identity: moving every row along the table's own values is moving the factor along itself
    dDs = np.zeros_like(dD[0])
    dDs[:, 3] = fac[:, 3]
    zW = np.zeros_like(dW[0])
    dyf, Ef = wt.tangent(C.prob, C.mode, C.k, xm_, C.mats, C.hs, st, fws, marr(np.zeros_like(dX[0])), marr(dDs), marr(zW), value_err=verr,
                         num=M_)
    sid = max(abs(a - b) for a, b in zip(dyf.ravel(), dys[wt.SEEDS.index("scale")].ravel()))
    assert sid < mpf("1e-50") * max(mpf(1), max(abs(v) for v in dyf.ravel())), sid
    out["scale_id"] = np.array(float(sid))
    out["dy_fw"], out["bound_fw"] = dyf.astype(float), Ef
    out["x"], out["disp"], out["dW"] = x, fac, dW
    if first:
        g30 = tt.load(flight)    # the same flight of the same vector: its F, J, Pu, Pf, verr serve the fp64 restatements
        for k_ in ("F", "J", "Pu", "Pf"):
            assert np.allclose(g30[k_], st[k_].astype(float), rtol=1e-12, atol=1e-30), k_   # (g30's quotients at 60 digits: 1e-35 absolute)
        assert np.allclose(g30["verr"], verr, rtol=1e-12, atol=0.0)
        out["Pw"], out["piece"], out["th"], out["air"] = st["Pw"].astype(float), st["piece"], st["th"].astype(float), st["air"]
    return out


def main():
    import flight_wind_truth as wt
    mj._setup()
    mp.dps = DPS
    out = {}
    with Pool(min(16, os.cpu_count() or 1)) as pool:
        for n, flight in enumerate(wt.FLIGHTS):
            t0 = time.time()
            r = flight_truth(flight, pool, n == 0)
            for k, v in r.items():
                out[wt.key(flight) + k] = v
            print("%s %s k=%d: (a) against (b) %.2e, forward against backward %.2e, duality %.2e, scale identity %.2e, "
                  "[bump row, stages below, above it, air stages under, over the table, air stages] = %s, %.1f s"
                  % (flight + (r["ab"].max(), r["fb"].max(), float(r["dual"]), float(r["scale_id"]), r["counts"].tolist(), time.time() - t0)),
                  flush=True)
    np.savez_compressed(wt.G35, **out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Ground truth of the flights whose step count differs by phase (tests/golden/g32_mixed_steps_noair.npz,
g33_mixed_steps_example.npz) for tests/test_mixed_steps*.py.

Needs mpmath and the built library (a host-only handle gives the plan's matrices).  For each flight of tests/mixed_steps.py:
  tangent   make_flight_tangent.flight_truth with the steps given per phase: dy by the recursion over the 60-digit per-stage
            partials, the whole map's three quotients, the bound E;
  adjoint   flight_adjoint_truth.adjoint in 60-digit arithmetic over the same run's per-stage F, J, Pu, Pf, rounded to fp64 as
            make_flight_adjoint.py reads them from g30, for the seven functionals, with the bound Eg;
  dual      the largest |<gx, dX> + <gdisp, dD> - <lam, dy>| / (sum of the |products|) over the 7 x 11 pairs, both sides in 60-digit
            arithmetic over those rounded partials;
  teeth     for each WRONG step assignment (mixed_steps.WRONG) the same tangent and adjoint under that assignment, and how far they
            miss 2 E / 2 Eg of the right one: teeth_dy, teeth_gx [4] and teeth = the larger of the two.
The noair flights store what g30 and g31 store per flight (Jw, identically zero without air, is left out); the example flights
dy, bound, ab, fb, y, x, disp, gx, gdisp, Egx, Egd, dual and the teeth alone.

Usage:  python tests/golden/make_flight_mixed_steps.py"""
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

import make_flight_tangent as mft  # noqa: E402
from make_flight_tangent import M_, marr  # noqa: E402

mp.dps = 60
STAGE_KEYS = ("F", "J", "Pu", "Pf")


def rounded(stf):
    """the per-stage data as exact mpf of its fp64 values"""
    st = {k: marr(stf[k]) for k in STAGE_KEYS}
    st["Jw"] = None          # (read by a mutation alone)
    return st


def tangent_job(job):
    """the recursion along one seed in 60-digit arithmetic over the rounded partials -> dy [M, 11] of mpf"""
    import flight_tangent_truth as tt
    flight, stf, x, dx, dd = job
    C = mft.ctx_of(flight)
    return tt.recursion(C.prob, C.mode, C.ks, marr(x), C.mats, C.hs, rounded(stf), marr(dx), marr(dd), num=M_)


def adjoint_job(job):
    """the transposed recursion for one functional over the rounded partials -> (gx, gd[, Egx, Egd]); the bounds where verr is given"""
    import flight_adjoint_truth as at
    flight, stf, x, lam, verr = job
    C = mft.ctx_of(flight)
    return at.adjoint(C.prob, C.mode, C.ks, marr(x), C.mats, C.hs, rounded(stf), marr(lam), value_err=verr, num=M_)


def stage_data(flight, pool):
    """the per-stage F, J, Pu, Pf of a flight's vector 1, rounded to fp64"""
    import flight_tangent_truth as tt
    C = mft.ctx_of(flight)
    x, fac = C.Xb[tt.TRUTH_VEC], C.disp[tt.TRUTH_VEC]
    xm_, fm_ = marr(x), marr(fac)
    stages = []
    C.fly(list(xm_), [list(r) for r in fm_], stages)
    res = pool.map(mft.stage_partials, [(flight, s, z, u, t, list(fm_[s])) for s, z, u, t in stages])
    return {k: np.array([r[i] for r in res]).astype(float) for i, k in enumerate(STAGE_KEYS)}


def both(flight, stf, x, dX, dD, lam, verr, pool):
    """-> (dys [11] of mpf arrays, adjoint results [7]) over the rounded partials, in one map"""
    jobs = [(tangent_job, (flight, stf, x, dX[d], dD[d])) for d in range(len(dX))]
    jobs += [(adjoint_job, (flight, stf, x, lam[q], verr)) for q in range(len(lam))]
    res = pool.map(_call, jobs)
    return res[:len(dX)], res[len(dX):]


def _call(job):
    return job[0](job[1])


def duality(dys, adj, dX, dD, lam):
    worst = mpf(0)
    for q in range(len(lam)):
        gx, gd, lm = adj[q][0], adj[q][1], marr(lam[q])
        for d in range(len(dX)):
            mx, md = marr(dX[d]), marr(dD[d])
            left = (gx * mx).sum() + (gd * md).sum()
            right = (lm * dys[d]).sum()
            scale = (abs(gx) * abs(mx)).sum() + (abs(gd) * abs(md)).sum() + (abs(lm) * abs(dys[d])).sum()
            if scale != 0:
                worst = max(worst, abs(left - right) / scale)
            else:
                assert left == right
    return float(worst)


def flight_truth(name, pool):
    import flight_adjoint_truth as at
    import flight_tangent_truth as tt
    import mixed_steps as ms
    flight = ms.CASES[name]
    full = name in ms.N_NAMES
    r = mft.flight_truth(flight, pool)
    x = r["x"]
    C = mft.ctx_of(flight)
    dX, dD = tt.directions(C.prob, x)
    lam = at.functionals(C.prob, x)
    stf = {k: r[k] for k in STAGE_KEYS}
    dys, adj = both(flight, stf, x, dX, dD, lam, r["verr"], pool)
    r["dual"] = np.array(duality(dys, adj, dX, dD, lam))
    r["gx"] = np.array([a[0].astype(float) for a in adj])
    r["gdisp"] = np.array([a[1].astype(float) for a in adj])
    r["Egx"] = np.array([a[2] for a in adj])
    r["Egd"] = np.array([a[3] for a in adj])
    teeth = np.zeros((2, len(ms.WRONG)))
    for w, how in enumerate(ms.WRONG):
        wrong = (flight[0], flight[1], ms.wrong_steps(flight[2], how))
        wdy, wadj = both(wrong, stage_data(wrong, pool), x, dX, dD, lam, None, pool)
        teeth[0, w] = max(at.miss(wdy[d].astype(float), r["dy"][d], 2 * r["bound"][d]) for d in range(len(dX)))
        teeth[1, w] = max(max(at.miss(wadj[q][0].astype(float), r["gx"][q], 2 * r["Egx"][q]),
                              at.miss(wadj[q][1].astype(float), r["gdisp"][q], 2 * r["Egd"][q])) for q in range(len(lam)))
    r["teeth_dy"], r["teeth_gx"], r["teeth"] = teeth[0], teeth[1], teeth.max(axis=0)
    del r["Jw"]
    if not full:
        r["fb"] = np.array([np.abs(r["dy_f"][d] - r["dy_b"][d]).max() / max(np.abs(r["dy"][d]).max(), 1e-300) for d in range(len(dX))])
        for k in ("dy_a", "dy_f", "dy_b", "verr") + STAGE_KEYS:
            del r[k]
    return r


def main(names=None):
    import flight_tangent_truth as tt
    import mixed_steps as ms
    out = {ms.G32: {}, ms.G33: {}}
    with Pool(min(16, os.cpu_count() or 1)) as pool:
        for name in names or ms.NAMES:
            t0 = time.time()
            r = flight_truth(name, pool)
            for k, v in r.items():
                out[ms.fixture_of(name)]["%s_%s" % (name, k)] = v
            print("%s: %d stages, (a) against (b) at most %.2e, duality %.2e, teeth %s (dy %s, gx %s), %.1f s"
                  % (name, 4 * tt.recursion_steps(ms.CASES[name]), r["ab"].max(), float(r["dual"]), np.array2string(r["teeth"], precision=3),
                     np.array2string(r["teeth_dy"], precision=3), np.array2string(r["teeth_gx"], precision=3), time.time() - t0), flush=True)
    return out


if __name__ == "__main__":
    for path, arrays in main().items():
        np.savez_compressed(path, **arrays)

#!/usr/bin/env python3
"""Ground truth of the flight whose every phase starts on another branch of the right-hand side (tests/kink_flight.py):
tests/golden/g34_flight_kinks.npz for tests/test_flight_kinks*.py.

Needs mpmath and the built library (a host-only handle gives the plan's matrices).  make_flight_tangent.py's procedure -- its Ctx,
stage_partials, whole_map and the recursion of tests/flight_tangent_truth.py are imported, not restated -- in 60-digit arithmetic
with h = 1e-25, for the three flights of kink_flight.FLIGHTS (section k = 1, node k = 1, section k = 2), 16 directions:

  per stage   J, Pu, Pf: central quotients of the right-hand side.  The ON-AXIS stage (x = y = 0) takes the convention of DESIGN 3.6
              from make_exact_jac.rhs(..., frozen=(h0, w0)) along x / y -- the air of the axis point held, the partials of p and of
              the longitude zero -- and no explicit time partial (the recursion has none).  Asserted: that block equals
              make_exact_jac.node_truth's Jv_conv of the same node (undispersed, as node_truth takes it) to the fp64 rounding of
              node_truth's output
  (a)         the whole map's central quotient against the recursion (b), on every phase without an on-axis stage; there both
              one-sided quotients agree too.  On the axis phases (b) stands alone
  one-sided   asserted per stage: the forward and the backward quotient of the right-hand side agree at every stage that is not on
              the axis, stages 2 - 4 of the axis phases included
  margins     asserted: no stage but the deliberate exact ones within 1e-9 (relative) of a layer break, 86 km, r = b, a wind or CA
              knot, |v_air| = 0 or the axis
  adjoint     gx, gdisp, Egx, Egd by flight_adjoint_truth.adjoint over the stored (rounded) per-stage data, as
              make_flight_mixed_steps.py derives them; duality against the recursion is reported (section flights; the adjoint has
              no node mode)
  teeth       dy of the section k = 1 flight under WRONG restatements of single branches (TEETH), and the factor by which each
              misses 2 E of the right truth.  Three of them change nothing on the example's tables, whose end intervals are flat
              and calm; they are evaluated on the ENDS variant of the case (kink_flight.ENDS: tables windy and sloped at their
              ends, the southern axis stage in air that carries a force, the Earth angle 0.73 rad from that of t = 0), which
              is flown as a fourth flight in section mode, k = 1, and where each must bite

Stored: for every flight dy, bound, y, x, disp, the stage states Z and their phases, the plan's pts, Wu, copy_u, hs, ab, fb, (gx, gdisp, Egx, Egd, dual); for the
section k = 1 flight also F, J, Pu, Pf, Jw, verr and the teeth.

Usage:  python tests/golden/make_flight_kinks.py"""
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
import make_flight_mixed_steps as mms  # noqa: E402
import make_flight_tangent as mft  # noqa: E402
from make_flight_tangent import M_, marr  # noqa: E402

mp.dps = 60
from kink_flight import TEETH  # noqa: E402


def on_axis(z):
    return z[1] == 0 and z[2] == 0


def axis_block(C, s, z, t, fac, t_air=None):
    """d F[4:7] / d (x, y) of an on-axis stage under the convention: make_exact_jac.rhs with the air of the axis point held
    (t_air: the time the held wind's Earth angle is taken at; the stage's own) -> [3, 2] of mpf"""
    h = mpf(mft.H)
    X = C.X
    ws = [C.wind[0], [w * fac[3] for w in C.wind[1]], [w * fac[3] for w in C.wind[2]]]
    rr = [c * C.units[1] for c in z[1:4]]
    vv = [c * C.units[2] for c in z[4:7]]
    va0, h0 = X.air_velocity(rr, vv, t if t_air is None else t_air, ws)
    w0 = [vv[0] + X.OMEGA * rr[1] - va0[0], vv[1] - X.OMEGA * rr[0] - va0[1], vv[2] - va0[2]]
    out = np.zeros((3, 2), dtype=object)
    for k in (1, 2):
        zp, zm = list(z), list(z)
        zp[k] += h
        zm[k] -= h
        f = [mj.rhs(X, zz[0], zz[1:4], zz[4:7], zz[7:11], t, C.thrust[s] * fac[0], C.area[s] * fac[2], C.nozzle[s], ws, C.ca, C.units,
                    frozen=(h0, w0)) for zz in (zp, zm)]
        for c in range(3):
            out[c, k - 1] = (f[0][c] - f[1][c]) / (2 * h)
    return out


def _extrapolating(X, tables):
    """exact_fd.interp continued with the end intervals' slopes outside the tables in `tables` (lists of abscissae, by identity)"""
    plain = X.interp

    def interp(x, xp, yp):
        if any(xp is t for t in tables) and (x <= xp[0] or x > xp[-1]):
            i = 0 if x <= xp[0] else len(xp) - 2
            return yp[i] + (x - xp[i]) / (xp[i + 1] - xp[i]) * (yp[i + 1] - yp[i])
        return plain(x, xp, yp)
    return interp


def _gravity_unclamped(X):
    def gravity(r, barC20):
        x, y, z = r
        rn = mp.sqrt(x * x + y * y + z * z)
        irx, iry, irz = x / rn, y / rn, z / rn
        s5 = mp.sqrt(mpf(5))
        P20, P20d = s5 * (3 * irz * irz - 1) / 2, s5 * 3 * irz
        g_ir = -X.MU / rn ** 2 * (1 + barC20 * (X.RA / rn) ** 2 * (3 * P20 + irz * P20d))
        g_iz = X.MU / rn ** 2 * (X.RA / rn) ** 2 * barC20 * P20d
        return [g_ir * irx, g_ir * iry, g_ir * irz + g_iz]
    return gravity


def kink_partials(job):
    """make_flight_tangent.stage_partials with the axis convention; variant: one of TEETH (a WRONG restatement) or None"""
    flight, s, z, u, t, fac, variant = job
    C = mft.ctx_of(flight)
    X = C.X
    saved = (X.interp, X.gravity, X.LMB)
    try:
        if variant == "wind_slope_outside":
            X.interp = _extrapolating(X, [C.wind[0]])
        elif variant == "ca_slope_outside":
            X.interp = _extrapolating(X, [C.ca[0]])
        elif variant == "no_gravity_clamp":
            X.gravity = _gravity_unclamped(X)
        elif variant == "neighbour_lapse":
            X.LMB = X.LMB[1:] + X.LMB[-1:]
        elif variant == "rest_from_1e-100":
            z = list(z)
            z[6] = z[6] + mpf("1e-100") / C.units[2]
        F, J, Pu, Pf, Jw = mft.stage_partials((flight, s, z, u, t, fac))
    finally:
        X.interp, X.gravity, X.LMB = saved
    if on_axis(z) and C.area[s] != 0:
        Jw[:, :] = mpf(0)           # (the frozen-wind quotient crosses the axis: read by no tooth here)
        if variant != "axis_longitude_partial":
            J[4:7, 1:3] = axis_block(C, s, z, t, fac, t_air=mpf(0) if variant == "axis_angle_t0" else None)
    if variant == "hold_rows_free" and C.prob["attitude_hold"][s]:
        for d in range(4):          # the quaternion rate is linear in q: its columns under the stage's sampled control
            e = [mpf(1) if c == d else mpf(0) for c in range(4)]
            J[7:11, 7 + d] = mj.quat_rhs(e, u, C.uu)
    return F, J, Pu, Pf, Jw


def one_sided_gap(job):
    """the largest distance of the forward and the backward quotient of the right-hand side along the 11 state components, the 2
    controls and the 4 factors at one stage, relative to the largest entry of the stage's central J, Pu, Pf"""
    flight, s, z, u, t, fac = job
    C = mft.ctx_of(flight)
    h = mpf(mft.H)
    f0 = C.rhs(s, z, u, fac, t)
    worst, big = mpf(0), mpf(0)
    for grp, n in ((0, 11), (1, 2), (2, 4)):
        for d in range(n):
            arg = [list(z), list(u), list(fac)]
            arg[grp][d] += h
            fp = C.rhs(s, arg[0], arg[1], arg[2], t)
            arg[grp][d] -= 2 * h
            fm = C.rhs(s, arg[0], arg[1], arg[2], t)
            for c in range(11):
                worst = max(worst, abs((fp[c] - f0[c]) - (f0[c] - fm[c])) / h)
                big = max(big, abs(fp[c] - fm[c]) / (2 * h))
    return float(worst / big)


def check_axis_convention(C, flight, stages):
    """the on-axis stage-1 velocity block against make_exact_jac.node_truth's Jv_conv of the same node, undispersed"""
    worst = 0.0
    for s, z, u, t in stages:
        if not (on_axis(z) and C.area[s] != 0):
            continue
        one = [mpf(1)] * 4
        blk = axis_block(C, s, z, t, one)
        zf = [float(v) for v in z]
        res = mj.node_truth((zf[0], zf[1:4], zf[4:7], zf[7:11], [float(v) for v in u], float(t), float(C.thrust[s]), float(C.area[s]),
                             float(C.nozzle[s]), np.asarray(C.prob["wind_table"]), np.asarray(C.prob["ca_table"]),
                             [float(v) for v in C.units], float(C.uu)))
        conv = res[6][:, 1:3]
        big = np.abs(res[6]).max(axis=1)
        gap = np.abs(blk.astype(float) - conv).max(axis=1) / big
        worst = max(worst, float(gap.max()))
        assert np.all(gap <= 4 * 2.0 ** -53), (s, gap)
    return worst


def hold_controls(C, x, stages):
    """the stages with the control a hold phase would sample if it were free (the tooth hold_rows_free reads it)"""
    out = []
    T = 0
    nv = 11 * C.M
    for s in range(C.S):
        n, k = C.nn[s], C.ks[s]
        ua = sum(C.nn[:s])
        m = C.mats[s]
        Uc = [[x[nv + 2 * (ua + q) + c] for c in range(2)] for q in range(n)]
        for j in range(n):
            for i in range(k):
                for sg in range(4):
                    pp = 2 * (k * j + i) + ((sg + 1) >> 1)
                    s_, z, u, t = stages[T]
                    if C.prob["attitude_hold"][s]:
                        u = Uc[m["copy_u"][pp]] if m["copy_u"][pp] >= 0 else [sum(M_(m["Wu"][pp, q]) * Uc[q][c] for q in range(n)) for c in range(2)]
                    out.append((s_, z, u, t))
                    T += 1
    return out


def flight_truth(flight, pool, full, teeth):
    import flight_adjoint_truth as at
    import flight_tangent_truth as tt
    import kink_flight as kf
    C = mft.ctx_of(flight)
    b = kf.TRUTH_VEC
    x, fac = C.Xb[b], C.disp[b]
    dX, dD = kf.directions(C.prob, x)
    lam = kf.functionals(C.prob, x)
    P = len(dX)
    xm_, fm_ = marr(x), marr(fac)
    stages = []
    y = C.fly(list(xm_), [list(r) for r in fm_], stages)
    phases = np.array([s for s, _z, _u, _t in stages])
    Z = np.array([[float(v) for v in z] for _s, z, _u, _t in stages])
    cen = kf.kink_census(C.prob, phases, Z, fac[:, 3])
    assert cen["margin"].min() > 1e-9, ("a stage within 1e-9 of a branch boundary", int(cen["margin"].argmin()), cen["margin"].min())
    axis_phase = np.array([s in kf.AXIS_PHASES for s in range(C.S)])
    assert set(phases[cen["on_axis"]]) == set(kf.AXIS_PHASES)
    conv = check_axis_convention(C, flight, stages)
    res = pool.map(kink_partials, [(flight, s, z, u, t, list(fm_[s]), None) for s, z, u, t in stages])
    # both one-sided quotients of every stage that is not on the axis agree (stages 2 - 4 of the axis phases included)
    stage_sides = pool.map(one_sided_gap, [(flight, s, z, u, t, list(fm_[s])) for (s, z, u, t), ax in zip(stages, cen["on_axis"]) if not ax])
    assert len(stage_sides) == len(stages) - 2 and max(stage_sides) < 1e-20, max(stage_sides)
    st = {k: np.array([r[i] for r in res]) for i, k in enumerate(("F", "J", "Pu", "Pf", "Jw"))}
    verr = mft.value_errors(C, x, fac, stages, st["F"])
    assert np.all(np.isfinite(verr))
    quots = pool.map(mft.whole_map, [(flight, x, fac, dX[d], dD[d]) for d in range(P)])
    M = C.M
    nn = C.nn
    smooth_rows = np.concatenate([np.full(nn[s] + 1, not axis_phase[s]) for s in range(C.S)])
    out = {k: np.zeros((P, M, 11)) for k in ("dy", "bound")}
    ab, fb = np.zeros(P), np.zeros(P)
    dys = []
    for d in range(P):
        dy, Eb = tt.recursion(C.prob, C.mode, C.k, xm_, C.mats, C.hs, st, marr(dX[d]), marr(dD[d]), value_err=verr, num=M_)
        dys.append(dy)
        ca, cf, cb = quots[d]
        big = max(abs(v) for v in dy[smooth_rows].ravel())
        worst = max(abs(a - c) for a, c in zip(dy[smooth_rows].ravel(), ca[smooth_rows].ravel()))
        sides = max(abs(a - c) for a, c in zip(cf[smooth_rows].ravel(), cb[smooth_rows].ravel()))
        ab[d] = float(worst / big) if big != 0 else float(worst)
        fb[d] = float(sides / big) if big != 0 else float(sides)
        out["dy"][d], out["bound"][d] = dy.astype(float), Eb
    assert ab.max() < 1e-28 and fb.max() < 1e-20, (ab, fb)       # (a) against (b); the one-sided quotients agree off the axis phases
    out.update({"ab": ab, "fb": fb, "conv": np.array(conv), "y": np.array([[float(v) for v in row] for row in y]), "x": x, "disp": fac,
                "Z": Z, "phases": phases, "margin": cen["margin"], "sides": np.array(max(stage_sides)),
                # the plan's tables the flight was made with (all phases have the same node count)
                "pts": np.array([m["pts"] for m in C.mats]), "Wu": np.array([m["Wu"] for m in C.mats]),
                "copy_u": np.array([m["copy_u"] for m in C.mats]), "hs": np.array(C.hs)})
    stf = {k: st[k].astype(float) for k in mms.STAGE_KEYS}
    if C.mode != "node":
        rdys, adj = mms.both(flight, stf, x, dX, dD, lam, verr, pool)
        out["dual"] = np.array(mms.duality(rdys, adj, dX, dD, lam))
        out["gx"] = np.array([a[0].astype(float) for a in adj])
        out["gdisp"] = np.array([a[1].astype(float) for a in adj])
        out["Egx"] = np.array([a[2] for a in adj])
        out["Egd"] = np.array([a[3] for a in adj])
    if full:
        for k in ("F", "J", "Pu", "Pf", "Jw"):
            out[k] = st[k].astype(float)
        out["verr"] = verr
    if teeth:
        # the teeth: the per-stage data of the stages a wrong restatement touches, then the recursion
        held = hold_controls(C, xm_, stages)
        touched = {"wind_slope_outside": cen["air"] & ((cen["wind"] == -1) | (cen["wind"] == len(C.wind[0]) - 1)),
                   "ca_slope_outside": cen["air"] & ((cen["ca"] == -1) | (cen["ca"] == len(C.ca[0]) - 1)),
                   "axis_longitude_partial": cen["on_axis"], "axis_angle_t0": cen["on_axis"], "no_gravity_clamp": cen["under"],
                   "neighbour_lapse": np.isin(np.arange(len(phases)), kf.first_stage(C.prob, C.mode, C.k)[[kf.NAMES.index("lapse"), kf.NAMES.index("isothermal")]]),
                   "rest_from_1e-100": cen["rest"],
                   "hold_rows_free": np.array([bool(C.prob["attitude_hold"][s]) for s in phases])}
        factors = np.zeros(len(teeth))
        for w, tooth in enumerate(teeth):
            idx = np.flatnonzero(touched[tooth])
            src = held if tooth == "hold_rows_free" else stages
            res_w = pool.map(kink_partials, [(flight, src[i][0], src[i][1], src[i][2], src[i][3], list(fm_[src[i][0]]), tooth) for i in idx])
            stw = {k: st[k].copy() for k in ("F", "J", "Pu", "Pf", "Jw")}
            for i, r in zip(idx, res_w):
                stw["J"][i], stw["Pu"][i], stw["Pf"][i] = r[1], r[2], r[3]
            wrong = np.zeros((P, M, 11))
            for d in range(P):
                wrong[d] = tt.recursion(C.prob, C.mode, C.k, xm_, C.mats, C.hs, stw, marr(dX[d]), marr(dD[d]), num=M_).astype(float)
            out["tooth_" + tooth] = wrong
            factors[w] = max(at.miss(wrong[d], out["dy"][d], 2 * out["bound"][d]) for d in range(P))
        out["teeth"] = factors
    return out


def main():
    import flight_tangent_truth as tt
    import kink_flight as kf
    mj._setup()
    arrays = {}
    with Pool(min(16, os.cpu_count() or 1)) as pool:
        for flight in kf.FLIGHTS + (kf.ENDS,):
            t0 = time.time()
            teeth = TEETH if flight == kf.FULL else (kf.ENDS_TEETH if flight == kf.ENDS else ())
            r = flight_truth(flight, pool, flight == kf.FULL, teeth)
            for k, v in r.items():
                arrays["%s_%s_k%d_%s" % (flight + (k,))] = v
            print("%s %s k=%d: %d stages, smallest margin %.2e, axis block against Jv_conv %.1e, (a) against (b) %.2e, one-sided %.2e (per stage %.2e), "
                  "duality %s" % (flight + (4 * tt.recursion_steps(flight), r["margin"].min(), float(r["conv"]), r["ab"].max(), r["fb"].max(), float(r["sides"]),
                                            "%.2e" % float(r["dual"]) if "dual" in r else "-")) + ", %.1f s" % (time.time() - t0), flush=True)
            if "teeth" in r:
                print("teeth, as multiples of 2 E: " + ", ".join("%s %.3g" % (n, f) for n, f in zip(teeth, r["teeth"])), flush=True)
    np.savez_compressed(kf.G34, **arrays)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Ground truth of the wind-profile sensitivities on the plans g35 does not fly (tests/golden/g36_flight_wind_plans.npz) for
tests/test_flight_wind_plans*.py.

Needs mpmath and the built library, as make_flight_wind.py, on which this is built: its ctx_of, wind_partials and whole_map, 80
digits, h = 1e-25, and flight_wind_truth.tangent / adjoint, the seven seeds and the twelve functionals.  Vector 1 of four flights
(flight_wind_truth.PLAN_FLIGHTS):

  W-node       example, node plan, k = 1                  tangent alone (the adjoint refuses node plans)
  W-E-chain    example, chain, mixed_steps.E_STEPS        tangent + adjoint: inner checkpoints in the air phases 1 (k = 3), 2 and 4 (k = 2)
  W-E-section  example, section, E_STEPS                  tangent + adjoint
  W-MIN        example@MIN, chain, k = 1                  tangent + adjoint: Kw = 2, one piece, stages over the table clamp onto row 1

(example@MIN flies finitely: asserted below; no replacement table was needed.)

Stored per flight: x, disp, dW, dy, bound, ab, fb, counts (flight_wind_truth.COUNTS) and, for the three adjoint flights, gW, Eg,
dual.  No per-stage data.  The teeth, at the same 80 digits:
  dy_rolled, gW_rolled   the two E flights under mixed_steps.wrong_steps(E_STEPS, "rolled"), same seeds and functionals
  dy_section             W-node's seeds flown on the section plan k = 1
Asserted here (and again by tests/test_flight_wind_plans_cpu.py from what is stored): (a) the whole map's central quotient against
(b) the recursion, for ALL seven seeds of every flight, within one decade of what g35 stores for the same seeds; forward against
backward quotient below 1e-20; duality <lam, T_w dW> = <gW, dW> to 1e-50; the counts (air stages in phases with k = 2 and with
k = 3; W-MIN: air stages inside its piece and over the table with Pw != 0; W-node: air stages in node intervals j >= 1); the rolled
plan's dy and gW miss 2 E / 2 Eg of the right plan by more than 1e3, and so does W-node's section restatement on the rows past each
phase's first interval (while its rows of the first interval are the node plan's); bounds finite, and where a bound is zero the
truth is exact: zero, or -- the start row of a segment under the mixed seed -- the seed's own entry of that row.

Wall time: 53 s with 8 processes for the four flights and the three teeth flights (10 + 19 + 18 + 6 s, printed per flight), so the
quotient check (a) runs on all seven seeds, not on a subset.

Usage:  python tests/golden/make_flight_wind_plans.py"""
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
from make_flight_tangent import M_, marr  # noqa: E402
import make_flight_tangent as mft  # noqa: E402
from make_flight_wind import DPS, ctx_of, whole_map, wind_partials  # noqa: E402


def stage_data(flight, pool):
    """vector 1 of a flight flown at 80 digits -> (context, x, fac, their mpf copies, the stages, the per-stage partials)"""
    import flight_wind_truth as wt
    C = ctx_of(flight)
    x, fac = C.Xb[wt.TRUTH_VEC], C.disp[wt.TRUTH_VEC]
    xm_, fm_ = marr(x), marr(fac)
    stages = []
    y = C.fly(list(xm_), [list(r) for r in fm_], stages)
    assert all(np.isfinite(float(v)) for row in y for v in row), flight
    res = pool.map(wind_partials, [(flight, s, z, u, t, list(fm_[s])) for s, z, u, t in stages])
    st = {"F": np.array([r[0] for r in res]), "J": np.array([r[1] for r in res]), "Pu": np.array([r[2] for r in res]),
          "Pf": np.array([r[3] for r in res]), "Pw": np.array([r[4] for r in res]), "piece": np.array([r[5] for r in res]),
          "th": np.array([r[6] for r in res], dtype=object), "air": np.array([r[7] for r in res])}
    return C, x, fac, xm_, fm_, stages, st


def both(C, xm_, fm_, st, dX, dD, dW, lam, adjoint):
    """-> (dy [7] of mpf arrays, gW [12] of mpf arrays | None) of the context's plan over its per-stage data"""
    import flight_wind_truth as wt
    fws = [fm_[s][3] for s in range(C.S)]
    dys = [wt.tangent(C.prob, C.mode, C.k, xm_, C.mats, C.hs, st, fws, marr(dX[d]), marr(dD[d]), marr(dW[d]), num=M_) for d in range(len(dW))]
    gWs = [wt.adjoint(C.prob, C.mode, C.k, xm_, C.hs, st, fws, marr(lam[q]), dW.shape[1], num=M_) for q in range(len(lam))] if adjoint else None
    return dys, gWs


def g35_level(seed_ids):
    """the largest (a)-against-(b) figure g35 stores over its four flights for these seeds"""
    import flight_wind_truth as wt
    return max(float(wt.load(f)["ab"][seed_ids].max()) for f in wt.FLIGHTS)


def flight_truth(name, pool):
    import flight_tangent_truth as tt
    import flight_wind_truth as wt
    import mixed_steps as ms
    flight = wt.PLAN_FLIGHTS[name]
    adjoint = name in wt.PLAN_ADJOINT
    C, x, fac, xm_, fm_, stages, st = stage_data(flight, pool)
    verr = mft.value_errors(C, x, fac, stages, st["F"])
    Kw = len(C.wind[0])
    air = st["air"] == 1
    stage_rows = [wt.rows_of(int(p), Kw) for p in st["piece"][air]]
    dW, dX, dD = wt.seeds(C.prob, x, stage_rows, True)
    lam = wt.functionals(C.prob)
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
        big = big if big != 0 else mpf(1)
        out["ab"][d] = float(max(abs(a - b) for a, b in zip(dy.ravel(), ca.ravel())) / big)
        out["fb"][d] = float(max(abs(a - b) for a, b in zip(cf.ravel(), cb.ravel())) / big)
        out["dy"][d], out["bound"][d] = dy.astype(float), Eb
        copied = marr(dX[d])[np.array([tt.state_rows(M, i) for i in range(M)])]      # (a segment's start row IS the seed's row)
        assert all(v == 0 or v == c for v, e, c in zip(dy.ravel(), Eb.ravel(), copied.ravel()) if e == 0), (name, wt.SEEDS[d])
        dys.append(dy)
    level = g35_level(np.arange(nsd))
    assert out["ab"].max() <= 10 * level, (name, out["ab"], level)
    assert out["fb"].max() < 1e-20, (name, out["fb"])
    assert np.all(np.isfinite(out["bound"]))
    # the counts that keep the tests from being vacuous
    ph = np.array([s for s, _z, _u, _t in stages])
    jj = np.concatenate([np.repeat(np.arange(C.nn[s]), 4 * C.ks[s]) for s, _c in tt.segments(C.prob, C.mode)])
    assert len(jj) == len(stages)
    kk = np.array([C.ks[s] for s in ph])
    nz = np.array([max(abs(v) for v in P.ravel()) > 0 for P in st["Pw"]])
    bump = wt.bump_row(Kw, stage_rows)
    cnt = {"bump": bump, "lo": sum(1 for i0, i1 in stage_rows if i1 != i0 and i1 == bump),
           "hi": sum(1 for i0, i1 in stage_rows if i1 != i0 and i0 == bump),
           "below": int(np.sum(air & (st["piece"] == -1) & nz)), "above": int(np.sum(air & (st["piece"] == -2) & nz)),
           "air": int(air.sum()), "inside": int(np.sum(air & (st["piece"] >= 0) & nz)),
           "air_k2": int(np.sum(air & nz & (kk == 2))), "air_k3": int(np.sum(air & nz & (kk == 3))), "air_j1": int(np.sum(air & nz & (jj >= 1)))}
    out["counts"] = np.array([cnt[k] for k in wt.COUNTS])
    if name in wt.PLAN_E:
        assert cnt["air_k2"] > 0 and cnt["air_k3"] > 0 and cnt["lo"] > 0 and cnt["hi"] > 0, cnt
    if name == "W-MIN":
        assert Kw == 2 and cnt["inside"] > 0 and cnt["above"] > 0, cnt
    if name == "W-node":
        assert cnt["air_j1"] > 0 and cnt["lo"] > 0 and cnt["hi"] > 0, cnt
    if adjoint:
        out["gW"], out["Eg"] = np.zeros((wt.NQ, Kw, 2)), np.zeros((wt.NQ, Kw, 2))
        stf = {k: (v.astype(float) if k in ("J", "Pw", "th") else v) for k, v in st.items()}
        dual = mpf(0)
        for q in range(wt.NQ):
            lq = marr(lam[q])
            gW = wt.adjoint(C.prob, C.mode, C.k, xm_, C.hs, st, fws, lq, Kw, num=M_)
            _g, Eg = wt.adjoint(C.prob, C.mode, C.k, x, C.hs, stf, [float(f) for f in fws], lam[q], Kw, want_E=True)
            out["gW"][q], out["Eg"][q] = gW.astype(float), Eg
            assert all(v == 0 for v, e in zip(gW.ravel(), Eg.ravel()) if e == 0), (name, q)
            for d in range(6):
                lhs = sum(a * b for a, b in zip(lq.ravel(), dys[d].ravel()))
                rhs = sum(a * b for a, b in zip(gW.ravel(), marr(dW[d]).ravel()))
                dual = max(dual, abs(lhs - rhs) / max(abs(lhs), abs(rhs), mpf(1)))
        assert dual < mpf("1e-50"), dual
        assert np.all(np.isfinite(out["Eg"]))
        out["dual"] = np.array(float(dual))
    # the teeth
    if name in wt.PLAN_E:
        wrong = (flight[0], flight[1], ms.wrong_steps(flight[2], "rolled"))
        Cw, _x, _f, _xm, _fm, _stages, stw = stage_data(wrong, pool)
        wdy, wgW = both(Cw, xm_, fm_, stw, dX, dD, dW, lam, True)
        out["dy_rolled"], out["gW_rolled"] = np.array([a.astype(float) for a in wdy]), np.array([a.astype(float) for a in wgW])
        t_dy = max(wt.miss_bounded(out["dy_rolled"][d], out["dy"][d], 2 * out["bound"][d]) for d in range(nsd))
        t_gw = max(wt.miss_bounded(out["gW_rolled"][q], out["gW"][q], 2 * out["Eg"][q]) for q in range(wt.NQ))
        assert t_dy > 1.0e3 and t_gw > 1.0e3, (name, t_dy, t_gw)
        out["teeth"] = np.array([t_dy, t_gw])
    if name == "W-node":
        wrong = (flight[0], "section", flight[2])
        Cw, _x, _f, _xm, _fm, _stages, stw = stage_data(wrong, pool)
        wdy, _g = both(Cw, xm_, fm_, stw, dX, dD, dW, lam, False)
        out["dy_section"] = np.array([a.astype(float) for a in wdy])
        first, later = wt.node_rows(C.nn)
        same = max(abs(a - b) for d in range(nsd) for a, b in zip(wdy[d][first].ravel(), dys[d][first].ravel()))
        assert same < mpf("1e-60"), same        # (the section plan's first interval IS the node plan's)
        t_dy = max(wt.miss_bounded(out["dy_section"][d][later], out["dy"][d][later], 2 * out["bound"][d][later]) for d in range(nsd))
        assert t_dy > 1.0e3, t_dy
        out["teeth"] = np.array([t_dy])
    out["x"], out["disp"], out["dW"] = x, fac, dW
    return out


def main():
    import flight_wind_truth as wt
    mj._setup()
    mp.dps = DPS
    out = {}
    t_all = time.time()
    with Pool(min(16, os.cpu_count() or 1)) as pool:
        for name in wt.PLAN_NAMES:
            t0 = time.time()
            r = flight_truth(name, pool)
            for k, v in r.items():
                out["%s_%s" % (name, k)] = v
            print("%s: (a) against (b) %.2e, forward against backward %.2e, duality %s, counts %s, teeth %s, %.1f s"
                  % (name, r["ab"].max(), r["fb"].max(), ("%.2e" % float(r["dual"])) if "dual" in r else "-",
                     dict(zip(wt.COUNTS, r["counts"].tolist())), np.array2string(r.get("teeth", np.zeros(0)), precision=3), time.time() - t0),
                  flush=True)
    np.savez_compressed(wt.G36, **out)
    print("%s: %d bytes, %.0f s in all" % (os.path.basename(wt.G36), os.path.getsize(wt.G36), time.time() - t_all))


if __name__ == "__main__":
    main()

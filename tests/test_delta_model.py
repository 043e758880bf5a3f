"""The series of the exact-difference position sweep, quantity by quantity (gel_rhs_parts.h pos_delta, gel_physics.h
atmosphere_delta, wind_piece, the margin of pos_centre_tail), against the chain recomputed at both points in 40-digit arithmetic
(tests/delta_model.py).  Through the Jacobian a wrong half-latitude pair or 1/p hides wherever the wind is weak; here every one
of the eight quantities a sweep hands on -- rho, P, 1/a, wn, we, sin(lat/2), cos(lat/2), 1/p -- is held to

    |dX - dX_true| <= REL[X] |dX_true| + 4 eps |X_centre|        (delta_model.tolerance)

over delta_model.inputs(): latitudes -89.9 .. 89.9 deg, -300 m .. 700 km, the three components, steps of 1e-6 m .. 1 m of either
sign, points half a step and two steps from every layer break, the 86 km branch and every wind row, and x / y sweeps around the
limit |u| = 1e-4 of the series near the polar axis.

CPU part: the numpy restatement of the device's formulas (the algorithm, without the device's arithmetic).  Its worst
|error| / tolerance per quantity with 1e-12 throughout, what gel_rhs_parts.h used to claim, over the 3109 inputs it accepts:

    rho 0.82   P 0.73   1/a 0.48   wn 7370   we 7370   sin(lat/2) 0.12   cos(lat/2) 0.088   1/p 331

The wind and 1/p need more, both only at the points 1.3 .. 22 km from the polar axis (below 80 degrees every quantity stays under
0.82, the wind and 1/p under 0.22): the wind 54 eps / cos^2(lat) and never more than 7.7e-9 -- what the terms of the altitude's
cancellation are off, which only a wind of 1e-22 m/s (a rounding residue of the example's table) has no output rounding above --
and 1/p 0.623 u^2, the u^3 term its series drops.  gel_rhs_parts.h now states twice those figures and delta_model.rel_at() holds
them as terms that vanish away from the axis (asserted: below 80 degrees the relative term of the first seven stays under
1.8e-12); with them the restatement's worst ratios are wn, we 0.50 and 1/p 0.50, the others as above.
Teeth: three mutants of the restatement, each one series term short, must break the tolerance at |dlt| = 1 m.  Worst ratios at
1e-6 m / 1 mm / 6.4 cm / 1 m:
    dp without 0.125 u^2            0.22 / 0.22 / 0.50 / 1.45  (P; rho 1.36, wn 1.01; unmutated 0.73, 0.82, 0.50).  The gap is
                                    small because the term is: it changes dp, hence every change, by 0.125 u^2 <= 1.25e-9 of itself
                                    (|u| < 1e-4 by the predicate), consistently -- the sweep of a step 1.25e-9 longer;
    uP without ee^2 / 6             0.22 / 0.22 / 0.50 / 950   (rho, P)
    dsl, dcl without dlat^2 / 2     0.22 / 69 / 4430 / 69200   (wn, we; rho, P 66 at 6.4 cm and 16100 at 1 m): this term is needed far
                                    below the reference's own 6.4 cm -- it passes at 1e-6 m only --, the other two show at 1 m alone.

GPU part (-m gpu): gel_point_eval kind 15, pos_part<CENTRE> -> pos_centre_tail -> pos_delta as the fused kernel chains them.
Measured on the MI355X, worst |error| / tolerance: rho 0.82, P 0.73, 1/a 0.48, wn 0.52, we 0.52, sin(lat/2) 0.12, cos(lat/2)
0.088, 1/p 0.50; the predicate agrees with the restatement's on all 3774 inputs."""
import numpy as np
import pytest

import delta_model as M

_CACHE = {}


def data():
    """(inputs, truth, wind table): computed once per session, shared and left unchanged"""
    if not _CACHE:
        import states
        wind = np.array(states._example_prob()["wind_table"], dtype=np.float64)
        I = M.inputs(wind)
        _CACHE["d"] = (I, M.truth(I["r"], I["kk"], I["dlt"], wind), wind)
    return _CACHE["d"]


def worst(rt, sel):
    return {n: float("%.3g" % rt[sel][:, j].max()) for j, n in enumerate(M.NAMES)}


def test_inputs_cover_what_they_promise():
    I, T, wind = data()
    n = len(I["dlt"])
    assert 3000 <= n <= 6000
    assert set(np.abs(I["dlt"])) == set(M.STEPS) and set(I["kk"]) == {0, 1, 2}
    lat = np.rad2deg(T["lat"])
    assert lat.min() < -89.8 and lat.max() > 89.8
    cen = M._centre(I["r"], wind)
    assert set(cen["k"]) == set(range(11)), "every atmosphere layer"
    # the breaks: crossings and near misses both; the limit: |u| on both sides
    g1 = I["group"] == 1
    assert (~T["same"][g1]).sum() > 100 and (T["same"][g1] & (T["clear"][g1] < 1.0)).sum() > 100
    g2 = I["group"] == 2
    assert (np.abs(T["u"][g2]) > M.U_LIMIT).sum() >= 24 and (np.abs(T["u"][g2]) < M.U_LIMIT).sum() >= 24


def test_restatement_holds_the_documented_accuracy_and_its_mutants_do_not():
    I, T, wind = data()
    cen, per, ok, margin = M.restate(I["r"], I["kk"], I["dlt"], wind)
    # the predicate: never true across a break or beyond the limits; true wherever the point is clear of both
    left = ~T["same"] | (np.abs(T["u"]) >= M.U_LIMIT) | (np.abs(T["v"]) >= M.U_LIMIT)
    assert not (ok & left).any()
    assert ok[(T["clear"] >= 2.0) & (np.abs(T["u"]) < 0.5 * M.U_LIMIT)].all()
    assert ok.sum() > 0.7 * len(ok)
    flat = M.ratios(cen, per, T, 1e-12)
    print("restatement, 1e-12 throughout:", worst(flat, ok))
    rt = M.ratios(cen, per, T)
    print("restatement, delta_model.rel_at:", worst(rt, ok))
    below80 = ok & (np.abs(T["lat"]) < np.deg2rad(80.0))
    assert M.rel_at(T)[below80][:, :7].max() <= 1.8e-12, "away from the axis the claim stays 1e-12 (1/p: where |u| is small)"
    # the exceptions are twice what the restatement needs, (|error| - 4 eps |X_c|) / |dX| - 1e-12, in their own units
    need = (np.abs((per - cen) - T["delta"]) - 4.0 * M.EPS * np.abs(T["centre"])) / (np.abs(T["delta"]) + 1e-300) - 1e-12
    assert need[ok][:, [0, 1, 2, 5, 6]].max() <= 0.0, "the other five hold 1e-12 everywhere"
    polar = (need[:, 3:5].max(axis=1) / (M.EPS / np.cos(T["lat"]) ** 2))[ok].max()
    cap = need[ok][:, 3:5].max()
    with np.errstate(divide="ignore", invalid="ignore"):
        u2 = np.where(T["u"] != 0.0, need[:, 7] / T["u"] ** 2, 0.0)[ok].max()
    print("restatement needs: wind %.3g eps / cos^2 lat and at most %.3g; 1/p %.3g u^2" % (polar, cap, u2))
    for got, have in ((polar, M.WIND_POLAR), (cap, M.WIND_CAP), (u2, M.INVP_U2)):
        assert 1.9 * got <= have <= 2.1 * got, (got, have)
    assert rt[ok].max() <= 1.0, worst(rt, ok)
    # teeth
    at = {d: ok & (np.abs(I["dlt"]) == d) for d in (1e-6, 1e-3, 0.064, 1.0)}
    for mutant, passes_at in (("dp_u2", 0.064), ("uP_e3", 0.064), ("hl2", 1e-6)):
        c2, p2, ok2, _ = M.restate(I["r"], I["kk"], I["dlt"], wind, mutant=mutant)
        r2 = M.ratios(c2, p2, T)
        print("mutant %s: 1e-6 m %s\n    1 mm %s\n    6.4 cm %s\n    1 m %s" % (
            mutant, worst(r2, at[1e-6]), worst(r2, at[1e-3]), worst(r2, at[0.064]), worst(r2, at[1.0])))
        assert r2[at[1.0]].max() > 1.0, "a series one term short must show at 1 m: " + mutant
        assert r2[at[passes_at]].max() <= 1.0, (mutant, passes_at)
    assert r2[at[0.064]].max() > 1.0, "the dlat^2 / 2 terms of dsl / dcl are needed at 6.4 cm already"


@pytest.mark.gpu
def test_device_position_sweep_against_the_truth_quantity_by_quantity():
    from gelato_amd import dynamics
    I, T, wind = data()
    out = dynamics.point_eval(15, np.column_stack([I["r"], I["kk"].astype(np.float64), I["dlt"]]), aux=wind)
    assert np.isfinite(out).all()
    cen, per, ok, margin = out[:, :8], out[:, 8:16], out[:, 16] == 1.0, out[:, 17]
    assert np.all((out[:, 16] == 0.0) | ok)
    # the centre, the values the change is taken from: 1e-10 of the value like every residual; the wind is looked up at an altitude
    # that carries the rounding of p / cos(lat) - N (fd_noise: eps (q (1 + 2 |lat tan lat|) + 6.4e6) m) times the table's steepest slope
    q = np.hypot(I["r"][:, 0], I["r"][:, 1]) / np.cos(T["lat"])
    dalt = M.EPS * (q * (1.0 + 2.0 * np.abs(T["lat"] * np.tan(T["lat"]))) + 6.4e6)
    steepest = np.abs(np.diff(wind[:, 1:], axis=0) / np.diff(wind[:, 0])[:, None]).max()
    ctol = 1e-10 * np.abs(T["centre"])
    ctol[:, 3:5] += (steepest * dalt)[:, None]
    assert np.all(np.abs(cen - T["centre"]) <= ctol), (np.abs(cen - T["centre"]) / (ctol + 1e-300)).max(axis=0)
    # the margin: the restatement's, to the rounding of the centre's altitude
    m0 = M.restate(I["r"], I["kk"], I["dlt"], wind)[3]
    assert np.all(np.abs(margin - m0) <= 1e-6 + 1e-12 * np.abs(m0)), np.abs(margin - m0).max()
    # the predicate, from the 40-digit geometry
    left = ~T["same"] | (np.abs(T["u"]) >= M.U_LIMIT) | (np.abs(T["v"]) >= M.U_LIMIT)
    assert not (ok & left).any(), "pos_delta accepted a lane whose perturbed point leaves the layer / piece / branch / limits: %s" % np.nonzero(ok & left)[0][:10]
    must = (T["clear"] >= 2.0) & (np.abs(T["u"]) < 0.5 * M.U_LIMIT)
    assert must.sum() > 0.5 * len(must) and ok[must].all(), "pos_delta refused lanes clear of every break: %s" % np.nonzero(must & ~ok)[0][:10]
    rt = M.ratios(cen, per, T)
    print("device, |error| / tolerance per quantity:", worst(rt, ok))
    for d in M.STEPS:
        print("   |dlt| = %g m: %s" % (d, worst(rt, ok & (np.abs(I["dlt"]) == d))))
    bad = np.argwhere(ok[:, None] & (rt > 1.0))
    assert len(bad) == 0, "%d (point, quantity) beyond the tolerance, worst %s; first: %s" % (len(bad), worst(rt, ok), [
        (int(i), M.NAMES[j], float(rt[i, j]), float(I["dlt"][i]), int(I["kk"][i]), float(np.rad2deg(T["lat"][i]))) for i, j in bad[:6]])

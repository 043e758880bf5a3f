"""The flight whose every phase starts on another branch of the right-hand side (tests/kink_flight.py), host
side (no GPU; host-only handles): the census of g34's three flights meets every class at stage 1 of some phase, and the smooth
flights of g30, g32 and g33 meet none of them at any stage -- the gap, written down; the conditions the truth of g34 must meet
(its inputs, (a) against (b), the margins re-evaluated in fp64, duality, finite bounds); the fp64 recursion on the stored partials;
the teeth by their stored factors; and the fixture's own |dy| against E, the check that the bound holds something at the axis."""
import numpy as np
import pytest

import flight_adjoint_truth as at
import flight_tangent_truth as tt
import interp_truth as it
import kink_flight as kf
import mixed_steps as ms


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


_CASE = {}


ALL = kf.FLIGHTS + (kf.ENDS,)


def _case(name="kinks"):
    """(prob, host-only engine, X, disp) of the case, or of its ENDS variant ("kinks@ENDS")"""
    if name not in _CASE:
        prob, X, disp = tt.case(name)
        _CASE[name] = (prob, it.engine(prob), X, disp)
    return _CASE[name]


def test_the_case_is_what_it_says():
    """x = y = 0 in the input of the two axis phases' first rows; the at-rest row's air-relative velocity is exactly zero in fp64,
    fused or not; the phase at rest flies in calm air in all three vectors; the other two vectors are off those kinks"""
    from fractions import Fraction
    prob, E, X, disp = _case()
    nn, S, N, M = tt.layout(prob)
    assert (S, set(nn), M) == (12, {3}, 48) and X.shape == (3, 11 * M + 2 * N + S + 1)
    up, uv = float(prob["units"][1]), float(prob["units"][2])
    first = [s * 4 for s in range(S)]
    x = X[kf.TRUTH_VEC]
    pos, vel = x[M:4 * M].reshape(-1, 3), x[4 * M:7 * M].reshape(-1, 3)
    for s in kf.AXIS_PHASES:
        assert pos[first[s], 0] == 0.0 and pos[first[s], 1] == 0.0 and float(prob["reference_area"][s]) != 0.0
        assert np.all(np.hypot(pos[first[s] + 1:first[s] + 4, 0], pos[first[s] + 1:first[s] + 4, 1]) * up > 1300.0)
        assert np.hypot(*X[2][M:4 * M].reshape(-1, 3)[first[s], :2]) * up == pytest.approx(5000.0)
    f = first[kf.REST_PHASE]
    r, v = pos[f] * up, vel[f] * uv
    assert (v[0] + kf.OMEGA * r[1], v[1] - kf.OMEGA * r[0], v[2]) == (0.0, 0.0, 0.0)
    assert all(Fraction(kf.OMEGA) * Fraction(r[c]) == Fraction(kf.OMEGA * r[c]) for c in (0, 1))
    assert np.all(disp[:, kf.REST_PHASE, 3] == 0.0) and np.all(np.delete(disp[:, :, 3], kf.REST_PHASE, axis=1) != 0.0)
    assert np.any(X[0][4 * M:7 * M].reshape(-1, 3)[f] != vel[f]) and np.all(X[0][M:4 * M] == x[M:4 * M] * (1.0 + 2.0 ** -10))
    air = np.asarray(prob["reference_area"]) != 0
    for key in ("engine_on", "attitude_hold"):          # thrust / engine / hold mixed over the air phases
        assert len(set(np.asarray(prob[key])[air])) == 2, key
    assert np.any(np.asarray(prob["reference_area"]) < 0) and np.any(np.asarray(prob["thrust"])[air] == 0)


@pytest.mark.parametrize("flight", ALL, ids=lambda f: "%s-%s-k%d" % f)
def test_census_meets_every_class_at_stage_one(flight):
    """every class of the table is met by stage 1 of at least one phase's first step, in all three flights and in the ENDS
    variant; counted per class"""
    prob, E, X, disp = _case(flight[0])
    g = kf.load(flight)
    assert np.array_equal(g["phases"], kf.stage_phases(prob, flight[1], flight[2]))
    c = kf.kink_census(prob, g["phases"], g["Z"], g["disp"][:, 3])
    fl = kf.class_flags(prob, g["phases"], c)[kf.first_stage(prob, flight[1], flight[2])]
    count = dict(zip(kf.CLASSES, fl.sum(axis=0)))
    print("%s %s k=%d, phases whose stage 1 is in a class: %s" % (flight + (count,)))
    assert all(v >= 1 for v in count.values()), count
    for s, name in enumerate(kf.NAMES):                 # ... and each phase meets the class it is named after
        own = name if name in kf.CLASSES else None
        assert own is None or fl[s, kf.CLASSES.index(own)], name
    # only the deliberate stages are exactly on a kink: the two axis stages and the one at rest, nowhere else in the flight
    assert c["on_axis"].sum() == 2 and c["rest"].sum() == 1


@pytest.mark.parametrize("flight", ALL, ids=lambda f: "%s-%s-k%d" % f)
def test_margins_in_fp64(flight):
    """no stage other than the deliberate exact ones lies within 1e-9 (relative) of a branch boundary -- a layer break, 86 km, r = b,
    a wind or CA knot, |v_air| = 0, the axis -- re-evaluated in fp64 from the stored stage states; the stored margins are these"""
    prob, E, X, disp = _case(flight[0])
    g = kf.load(flight)
    c = kf.kink_census(prob, g["phases"], g["Z"], g["disp"][:, 3])
    print("%s %s k=%d: smallest margin %.3g at stage %d" % (flight + (c["margin"].min(), int(c["margin"].argmin()))))
    assert c["margin"].min() > 1e-9
    assert np.allclose(c["margin"], g["margin"], rtol=1e-6)
    ax = np.isin(g["phases"], kf.AXIS_PHASES) & ~c["on_axis"]
    up = float(prob["units"][1])
    assert (np.hypot(g["Z"][ax, 1], g["Z"][ax, 2]) * up).min() > 1300.0     # stages 2 - 4 beyond pos_delta's 1276 m switch


def _smooth_flights():
    out = [("g30", f) for f in tt.FLIGHTS + tt.TABLE_FLIGHTS]
    return out + [("g32/g33", ms.CASES[n]) for n in ms.NAMES]


@pytest.mark.parametrize("src,flight", _smooth_flights(), ids=lambda v: str(v))
def test_smooth_flights_meet_none_of_it(src, flight):
    """THE GAP: over every stage of the flights g30, g32 and g33 hold (re-flown in fp64 with flight_truth's right-hand side: the
    fixtures keep no stage states) none is on the polar axis, at rest in the air, below the polar radius, above 110 km with air (the
    end of the ellipse, 110 - 120 km, the exponential) or above a wind table's last row.  What they DO meet, measured here and not
    assumed: the example's last air phase crosses 86 km and ends at 91.2 km (93.7 km over the LONG tables) -- 5 to 9 stages in the
    isothermal 86 - 91 km layer and 1 to 3 at the foot of the ellipse -- and over EDGE32 / LONG, whose wind tables begin higher, 29
    stages lie below the first row.  On the example's own table no stage leaves it.  (The NoAir flights keep their stages: they
    have no air to be in.)"""
    case, mode, steps = flight
    prob, X, disp = tt.case(case)
    E = it.engine(prob)
    plan = E.propagation_plan(steps=list(tt.steps_of(steps, E.S)), restart=mode)
    b = tt.TRUTH_VEC
    phases, Z = kf.fly_stages(E, plan, prob, X[b], disp[b], mode)
    plan.close()
    assert len(Z) == 4 * sum(k * n for k, n in zip(plan.steps, tt.layout(prob)[0])) and np.all(np.isfinite(Z))
    c = kf.kink_census(prob, phases, Z, disp[b][:, 3])
    gap = {k: int(v.sum()) for k, v in kf.gap_flags(prob, c).items()}
    print("%s %s: %d stages, of them %s; with air above 86 km %d, highest %.0f m"
          % (src, flight, len(Z), gap, int((c["air"] & c["above86"]).sum()), c["alt"][c["air"]].max() if c["air"].any() else 0.0))
    assert all(gap[k] == 0 for k in kf.GAP), gap
    assert c["alt"][c["air"]].max(initial=0.0) < 94000.0
    assert (gap["below_wind_table"] > 0) == ("@" in case), gap


@pytest.mark.parametrize("flight", ALL, ids=lambda f: "%s-%s-k%d" % f)
def test_truth_conditions(flight):
    """the stored inputs are the case's; (a) against (b) to 1e-28 of a direction's largest entry off the axis phases, where the
    one-sided quotients agree too, and per stage at every stage that is not on the axis; the axis block is make_exact_jac's
    convention; bounds finite; the 60-digit duality to 1e-30"""
    prob, E, X, disp = _case(flight[0])
    g = kf.load(flight)
    M, nv, P, Q = E.M, X.shape[1], len(kf.DIRECTIONS), len(kf.FUNCTIONALS)
    b = kf.TRUTH_VEC
    assert np.array_equal(_bits(g["x"]), _bits(X[b])) and np.array_equal(_bits(g["disp"]), _bits(disp[b]))
    assert g["dy"].shape == (P, M, 11) and g["bound"].shape == (P, M, 11) and g["y"].shape == (M, 11)
    assert np.all(np.isfinite(g["y"])) and np.all(np.isfinite(g["dy"])) and np.all(np.isfinite(g["bound"])) and np.all(g["bound"] >= 0)
    assert np.all(g["ab"] <= 1e-28) and np.all(g["fb"] <= 1e-20) and float(g["conv"]) <= 4 * tt.U and float(g["sides"]) <= 1e-20, (g["ab"], g["fb"], g["conv"], g["sides"])
    assert np.all(np.abs(g["dy"]).max(axis=(1, 2)) > 0)
    if flight[1] != "node":
        assert g["gx"].shape == (Q, nv) and g["gdisp"].shape == (Q, E.S, 4) and float(g["dual"]) <= 1e-30
        for k in ("Egx", "Egd"):
            assert np.all(np.isfinite(g[k])) and np.all(g[k] >= 0), k
        assert np.all(np.abs(g["gx"]).max(axis=1) > 0) and np.any(g["gdisp"] != 0)


def test_plan_tables_are_the_fixtures():
    """plan.matrices (stage points, control matrix, copy list) and the step fractions a host-only handle gives are, bit for bit,
    the ones the fixture was made with: the fp64 recursion below runs on them"""
    for flight in ALL:
        prob, E, X, disp = _case(flight[0])
        mats, hs = tt.plan_tables(E, flight[2], flight[1])
        g = kf.load(flight)
        assert len(g["Z"]) == 4 * sum(len(h) * flight[2] for h in hs)
        for s in range(E.S):
            assert mats[s]["pts"].shape == (2 * flight[2] * 3 + 1,)
            assert np.array_equal(_bits(mats[s]["pts"]), _bits(g["pts"][s])) and np.array_equal(_bits(mats[s]["Wu"]), _bits(g["Wu"][s])), (flight, s)
            assert np.array_equal(mats[s]["copy_u"], g["copy_u"][s]) and np.array_equal(_bits(hs[s]), _bits(g["hs"][s])), (flight, s)


def test_fp64_recursion_reproduces_dy_and_E():
    """the tangent recursion in fp64 over the stored partials of the section k = 1 flight gives the stored E bit for bit (E is an
    fp64 quantity) and dy within 2 E -- it is an fp64 implementation of the map, held to what the device is held to -- zero pattern
    included; its transpose gx, gdisp within 2 Eg"""
    prob, E, X, disp = _case()
    case, mode, k = kf.FULL
    g = kf.load(kf.FULL)
    mats, hs = tt.plan_tables(E, k, mode)
    dX, dD = kf.directions(prob, g["x"])
    lam = kf.functionals(prob, g["x"])
    worst = 0.0
    for d in range(len(dX)):
        r, Eb = tt.recursion(prob, mode, k, g["x"], mats, hs, g, dX[d], dD[d], value_err=g["verr"])
        assert np.array_equal(r != 0, g["dy"][d] != 0), kf.DIRECTIONS[d]
        assert np.allclose(Eb, g["bound"][d], rtol=1e-12, atol=0.0), kf.DIRECTIONS[d]
        worst = max(worst, at.miss(r, g["dy"][d], 2 * g["bound"][d]))
    print("fp64 tangent recursion: at most %.3g of 2 E" % worst)
    assert worst <= 1.0
    worst = 0.0
    for q in range(len(lam)):
        gx, gd = at.adjoint(prob, mode, k, g["x"], mats, hs, g, lam[q])
        assert np.array_equal(gx != 0, g["gx"][q] != 0) and np.array_equal(gd != 0, g["gdisp"][q] != 0), kf.FUNCTIONALS[q]
        worst = max(worst, at.miss(gx, g["gx"][q], 2 * g["Egx"][q]), at.miss(gd, g["gdisp"][q], 2 * g["Egd"][q]))
    print("fp64 adjoint recursion: at most %.3g of 2 Eg" % worst)
    assert worst <= 1.0


def test_fp64_duality_of_the_stored_truth():
    """<lam, dy> = <gx, dX> + <gdisp, dD> between the stored arrays, within the bounds both carry, for the 9 x 16 pairs of the two
    section flights and the ENDS variant"""
    for flight in ALL:
        prob, E, X, disp = _case(flight[0])
        if flight[1] == "node":
            continue
        g = kf.load(flight)
        dX, dD = kf.directions(prob, g["x"])
        lam = kf.functionals(prob, g["x"])
        worst = 0.0
        for q in range(len(lam)):
            for d in range(len(dX)):
                gap = abs((lam[q] * g["dy"][d]).sum() - (g["gx"][q] * dX[d]).sum() - (g["gdisp"][q] * dD[d]).sum())
                size = (np.abs(lam[q] * g["dy"][d]).sum() + np.abs(g["gx"][q] * dX[d]).sum() + np.abs(g["gdisp"][q] * dD[d]).sum())
                worst = max(worst, gap / (1e-13 * size) if size > 0 else gap)
        print("%s %s k=%d: stored duality to %.3g of 1e-13 of the products" % (flight + (worst,)))
        assert worst <= 1.0


# On the example's own tables three restatements change nothing: both tables end in flat intervals, and the axis altitude -N maps
# into the wind table's calm last interval, in air of 2e-20 kg/m^3.  They are held on the ENDS variant of the case, where each must
# bite.  rest_from_1e-100 is identically the truth under any tables (|a| a CA is C^1 with derivative 0 at rest).
BITING = ("axis_longitude_partial", "no_gravity_clamp", "neighbour_lapse", "hold_rows_free")
IDENTICAL = ("rest_from_1e-100",)


def _tooth_factors(flight, teeth):
    g = kf.load(flight)
    assert g["teeth"].shape == (len(teeth),)
    out = {}
    for w, tooth in enumerate(teeth):
        wrong = g["tooth_" + tooth]
        f = max(at.miss(wrong[d], g["dy"][d], 2 * g["bound"][d]) for d in range(len(kf.DIRECTIONS)))
        print("%s, tooth %s: %.3g of 2 E" % (flight[0], tooth, f))
        assert f == g["teeth"][w] or abs(f - g["teeth"][w]) <= 1e-12 * f, (tooth, f, g["teeth"][w])
        out[tooth] = f
    return out


def test_teeth():
    """every tooth lies outside 2 E of the right truth, by its stored factor (recomputed from the stored arrays) and by more than
    1e3: four on the case itself, the three that the example's flat, calm table ends cannot show on the ENDS variant.  The one
    restatement that is identically the truth is stored and asserted to be that, by name."""
    assert set(kf.TEETH) == set(BITING + kf.ENDS_TEETH + IDENTICAL)
    f = _tooth_factors(kf.FULL, kf.TEETH)
    assert all(f[t] > 1.0e3 for t in BITING), f
    assert all(f[t] == 0.0 for t in IDENTICAL), f
    print("on the example's tables the teeth held on ENDS have the factors %s" % {t: f[t] for t in kf.ENDS_TEETH})
    f = _tooth_factors(kf.ENDS, kf.ENDS_TEETH)
    assert all(f[t] > 1.0e3 for t in kf.ENDS_TEETH), f


def test_ends_variant_is_what_it_says():
    """the ENDS tables are windy and sloped in their first and last intervals; the truth vector's stages reach below the wind
    table's first row, above its last row (the axis stages among them) and above the CA table's last row; the southern axis stage
    has air that carries a force; the Earth angle of the axis stages is far from that of t = 0"""
    prob, E, X, disp = _case(kf.ENDS[0])
    W, Ct = np.asarray(prob["wind_table"]), np.asarray(prob["ca_table"])
    base = _case()[0]
    assert W.shape == np.asarray(base["wind_table"]).shape and Ct.shape == np.asarray(base["ca_table"]).shape
    for T in (W, Ct):
        assert np.all(np.diff(T[:, 0]) > 0) and np.all(T[1, 1:] != T[0, 1:]) and np.all(T[-1, 1:] != T[-2, 1:])
    assert np.all(W[[0, 1, -2, -1], 1:] != 0.0)
    g = kf.load(kf.ENDS)
    c = kf.kink_census(prob, g["phases"], g["Z"], g["disp"][:, 3])
    f1 = kf.first_stage(prob, kf.ENDS[1], kf.ENDS[2])
    assert c["wind"][f1[kf.NAMES.index("wind_below")]] == -1 and np.all(c["wind"][f1[list(kf.AXIS_PHASES)]] == len(W) - 1)
    assert c["wind"][f1[kf.NAMES.index("exponential")]] == len(W) - 1 and c["ca"][f1[kf.NAMES.index("ca_above")]] == len(Ct) - 1
    import oracle
    s = kf.AXIS_PHASES[1]
    assert oracle.air_density(c["h"][f1[s]]) * float(prob["reference_area"][s]) > 1e-4
    t = X[kf.TRUTH_VEC][-(E.S + 1):]
    assert np.all(kf.OMEGA * t > 0.5) and np.all(kf.OMEGA * t < 1.0)


def test_bound_holds_something_at_the_axis():
    """the reference-side check before any device run: the entries of dy whose carried bound 2 E exceeds the entry's own largest
    value over the directions -- where the bound would hold nothing.  There is none, in the axis phases or elsewhere: no entry is
    excluded from the device tests."""
    for flight in ALL:
        prob, E, X, disp = _case(flight[0])
        rows = kf.axis_rows(prob)
        g = kf.load(flight)
        big = np.abs(g["dy"]).max(axis=0)                    # [M, 11] over the directions
        loose = (2 * g["bound"]).max(axis=0) > big
        loose &= big > 0
        print("%s %s k=%d: %d entries of [M, 11] whose 2 E exceeds the entry's largest |dy|; in the axis phases %d"
              % (flight + (int(loose.sum()), int(loose[rows].sum()))))
        assert not loose.any(), np.argwhere(loose)

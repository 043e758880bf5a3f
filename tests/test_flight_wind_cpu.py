"""The wind-profile sensitivities of the flight, host side (no GPU): the stored truth g35 is not vacuous and its
bounds have teeth -- the conditions tests/golden/make_flight_wind.py asserted, re-asserted from what is stored, and the four wrong
restatements of flight_wind_truth evaluated in fp64 on the stored per-stage partials, which must leave 2 E resp. 2 Eg --; every
refusal of the new calls, of gel_prop_wind_rows and of gel_prop_adjoint_wind_info on host-only handles, each decided before a buffer is
looked at (every buffer passed is a poisoned non-NULL address); montecarlo.wind_linear_prediction; and the refusals once more in a
stand-alone program under ASan + UBSan."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import flight_tangent_truth as tt
import flight_wind_truth as wt
import interp_truth as it
import sanitized_lib
from test_wind_ensemble_cpu import members

GEL_ERR_ARG = -1
POISON = 0xDEAD0000
NUM_NODES = [2, 3, 16, 4]
NAMES = ("gel_propagate_tangent_wind", "gel_propagate_tangent_wind_device", "gel_propagate_adjoint_wind", "gel_propagate_adjoint_wind_device")


def _dp(addr):
    return C.cast(C.c_void_p(addr), C.POINTER(C.c_double)) if addr else None


# ------------------------------------------------------------------ 1. the truth is not vacuous
@pytest.mark.parametrize("flight", wt.FLIGHTS, ids=lambda f: "%s-%s-k%d" % f)
def test_conditions_of_the_truth(flight):
    g = wt.load(flight)
    prob, X, disp = tt.case(flight[0])
    assert np.array_equal(g["x"], X[wt.TRUTH_VEC]) and np.array_equal(g["disp"], disp[wt.TRUTH_VEC])
    Kw = np.asarray(prob["wind_table"]).shape[0]
    nsd = len(wt.SEEDS)
    assert g["dy"].shape == g["bound"].shape == (nsd, tt.layout(prob)[3], 11) and g["gW"].shape == g["Eg"].shape == (wt.NQ, Kw, 2)
    # (a) central against (b), relative to the direction's largest entry: g30's level (its worst direction: 8.6e-33)
    assert g["ab"].shape == (nsd,) and g["ab"].max() < 1e-30, g["ab"]
    # forward against backward: h apart, so no stage sits within h = 1e-25 of a breakpoint
    assert g["fb"].max() < 1e-20, g["fb"]
    bump, lo, hi, below, above, nair = (int(v) for v in g["counts"])
    assert lo > 0 and hi > 0 and nair > 0, g["counts"]                  # the bump row has stages in both adjacent pieces
    assert np.count_nonzero(g["dW"][0]) == 1 and g["dW"][0, bump, 0] == 1.0
    if flight[0] == "kinks@ENDS":
        assert below > 0 and above > 0, g["counts"]                     # air stages under and over the table, each with Pw != 0
        assert np.any(g["disp"][:, 3] != 1.0)
    if flight[0] == "example@LONG":
        assert Kw == 160
    assert float(g["dual"]) < 1e-50 and float(g["scale_id"]) < 1e-50    # duality and the scaling identity, in the truth's arithmetic
    # the seeds are flight_wind_truth's
    assert np.array_equal(g["dW"][2], np.asarray(prob["wind_table"])[:, 1:]) and np.all(g["dW"][1, :, 1] == 1.0)
    # every seed that moves the flight has a bound, and a seed that moves nothing has none
    for d in range(nsd):
        moved = np.abs(g["dy"][d]).max() > 0
        assert moved == (g["bound"][d].max() > 0), (flight, wt.SEEDS[d])
    assert np.abs(g["dy"][[0, 1, 2, 5, 6]]).reshape(5, -1).max(axis=1).min() > 0
    # fp64 duality of the stored arrays, within the stored bounds
    lam = wt.functionals(prob)
    for q in range(wt.NQ):
        for d in range(6):
            lhs, rhs = (lam[q] * g["dy"][d]).sum(), (g["gW"][q] * g["dW"][d]).sum()
            tol = (np.abs(lam[q]) * g["bound"][d]).sum() + (g["Eg"][q] * np.abs(g["dW"][d])).sum() + 1e-13 * (abs(lhs) + abs(rhs))
            assert abs(lhs - rhs) <= tol, (flight, q, d, lhs, rhs, tol)


def _first():
    """the first flight's per-stage data: g30's F, J, Pu, Pf, verr and g35's Pw, piece, th, air"""
    flight = wt.FLIGHTS[0]
    g, g30 = wt.load(flight), tt.load(flight)
    assert np.array_equal(g30["x"], g["x"]) and np.array_equal(g30["disp"], g["disp"])
    st = {k: g30[k] for k in ("F", "J", "Pu", "Pf")}
    st.update({k: g[k] for k in ("Pw", "piece", "th", "air")})
    prob, _X, _d = tt.case(flight[0])
    mats, hs = tt.plan_tables(it.engine(prob), flight[2], flight[1])
    return flight, g, st, g30["verr"], prob, mats, hs


def test_restatement_reproduces_the_truth_and_the_bounds():
    """flight_wind_truth.tangent / adjoint in fp64 on the stored partials land within E / Eg of the stored truth (they ARE the
    device's arithmetic up to the order of the sums), and the bound the fp64 run carries is the stored one"""
    flight, g, st, verr, prob, mats, hs = _first()
    fws = g["disp"][:, 3]
    rows = [wt.rows_of(int(p), g["dW"].shape[1]) for p in st["piece"][st["air"] == 1]]
    dW, dX, dD = wt.seeds(prob, g["x"], rows)
    assert np.array_equal(dW, g["dW"]) and wt.bump_row(dW.shape[1], rows) == int(g["counts"][0])
    for d in range(len(wt.SEEDS)):
        dy, E = wt.tangent(prob, flight[1], flight[2], g["x"], mats, hs, st, fws, dX[d], dD[d], dW[d], value_err=verr)
        assert wt.miss(dy, g["dy"][d], g["bound"][d]) <= 1.0, wt.SEEDS[d]
        assert np.allclose(E, g["bound"][d], rtol=1e-6, atol=0.0), wt.SEEDS[d]
    lam = wt.functionals(prob)
    for q in range(wt.NQ):
        gW, Eg = wt.adjoint(prob, flight[1], flight[2], g["x"], hs, st, fws, lam[q], dW.shape[1], want_E=True)
        assert wt.miss(gW, g["gW"][q], g["Eg"][q]) <= 1.0, q
        assert np.allclose(Eg, g["Eg"][q], rtol=1e-6, atol=0.0), q


@pytest.mark.parametrize("mut", wt.MUTATIONS)
def test_bounds_reject_wrong_restatements(mut):
    """each wrong restatement leaves 2 E for some seed and 2 Eg for some functional.  ends_dropped needs stages outside the table: the
    first flight stays inside it, so that one is judged on the ENDS flight's data by the device test alone and must be EXACT here"""
    flight, g, st, verr, prob, mats, hs = _first()
    fws = g["disp"][:, 3]
    Kw = g["dW"].shape[1]
    lam = wt.functionals(prob)
    worst_t = max(wt.miss(wt.tangent(prob, flight[1], flight[2], g["x"], mats, hs, st, fws, np.zeros_like(g["x"]), np.zeros((len(fws), 4)),
                                     g["dW"][d], mutate=mut), g["dy"][d], 2 * g["bound"][d]) for d in (0, 1, 2, 5))
    worst_a = max(wt.miss(wt.adjoint(prob, flight[1], flight[2], g["x"], hs, st, fws, lam[q], Kw, mutate=mut), g["gW"][q], 2 * g["Eg"][q])
                  for q in (4, 5, 6, 11))
    print("mutation %s: leaves 2 E by a factor %.3g, 2 Eg by a factor %.3g" % (mut, worst_t, worst_a))
    if mut == "ends_dropped":
        assert int(g["counts"][3]) == 0 and int(g["counts"][4]) == 0 and worst_t <= 1.0 and worst_a <= 1.0
        e = wt.load(wt.FLIGHTS[3])
        assert int(e["counts"][3]) > 0 and int(e["counts"][4]) > 0
        # the end rows alone carry those stages: with them dropped the two end-row seeds would move nothing
        assert np.abs(e["dy"][3]).max() > 2 * e["bound"][3].max() and np.abs(e["dy"][4]).max() > 2 * e["bound"][4].max()
        assert np.abs(e["gW"][:, 0]).max() > 2 * e["Eg"][:, 0].max() and np.abs(e["gW"][:, -1]).max() > 2 * e["Eg"][:, -1].max()
    else:
        assert worst_t > 1.0e3 and worst_a > 1.0e3, (mut, worst_t, worst_a)


def test_lookup_is_the_header_expression():
    """flight_wind_truth.lookup on the conventions of the value lookup: xl < h <= xu, the clamped ends, the weights"""
    alt = np.array([0.0, 1000.0, 4000.0, 9000.0])
    assert wt.lookup(-5.0, alt) == (-1, 0, 0, 0.0) and wt.lookup(0.0, alt) == (-1, 0, 0, 0.0)
    assert wt.lookup(9000.0, alt) == (2, 2, 3, 1.0) and wt.lookup(9000.5, alt) == (-2, 3, 3, 0.0)
    assert wt.lookup(1000.0, alt) == (0, 0, 1, 1.0)                         # at a breakpoint: the piece below it, as the value's
    assert wt.lookup(2500.0, alt) == (1, 1, 2, (2500.0 - 1000.0) / (4000.0 - 1000.0))
    assert wt.weights(1, 0.25, 4, 2.0) == [(1, 1.5), (2, 0.5)] and wt.weights(-2, 0.0, 4, 2.0) == [(3, 2.0)]
    assert wt.weights(-1, 0.0, 4, 2.0, "ends_dropped") == [] and wt.weights(1, 0.25, 4, 2.0, "theta_swapped") == [(1, 0.5), (2, 1.5)]
    assert wt.weights(1, 0.25, 4, 2.0, "shift_piece") == [(0, 1.5), (1, 0.5)] and wt.weights(1, 0.25, 4, 2.0, "no_fw") == [(1, 0.75), (2, 0.25)]
    text = open(os.path.join(os.path.dirname(wt.HERE), "gelato_amd", "csrc", "gel_wind_rows.h")).read()
    assert "th = (h - x[i]) / (x[i + 1] - x[i])" in text and "fma(th, dW[i + 1] - dW[i], dW[i])" in text


# ------------------------------------------------------------------ 2. the C ABI on host-only handles
def test_prototypes_in_the_header_and_bound():
    from gelato_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "gelato_amd.h")).read()
    L = _lib.lib()
    for n in NAMES:
        m = re.search(r"^int %s\(([^;]*)\);" % n, text, re.M)
        assert m, n
        assert "gel_wind_ensemble* ens" in m.group(1) and "stream" not in m.group(1), n
        fn = getattr(L, n)
        assert fn.restype is C.c_int and len(fn.argtypes) == 12, n
    assert re.search(r"gel_propagate_tangent_wind\([^;]*ddisp[^;]*dwind[^;]*ens[^;]*\by,", text)
    assert re.search(r"gel_propagate_adjoint_wind\([^;]*lam[^;]*ens[^;]*gdisp[^;]*gwind", text)
    assert len(L.gel_prop_wind_rows.argtypes) == 3 and len(L.gel_prop_adjoint_wind_info.argtypes) == 7


def _tangent(L, form, plan, B, P, shared, ens, dx=POISON, ddisp=POISON, dwind=POISON, x=POISON):
    if form == "host":
        rc = L.gel_propagate_tangent_wind(plan, B, P, shared, _dp(x), _dp(POISON), _dp(dx), _dp(ddisp), _dp(dwind), ens, _dp(POISON), _dp(POISON))
    else:
        rc = L.gel_propagate_tangent_wind_device(plan, B, P, shared, x or None, POISON, dx or None, ddisp or None, dwind or None, ens, POISON, POISON)
    return rc, (L.gel_last_error() or b"").decode()


def _adjoint(L, form, plan, B, Q, shared, ens, lam=POISON, gwind=POISON):
    if form == "host":
        rc = L.gel_propagate_adjoint_wind(plan, B, Q, shared, _dp(POISON), _dp(POISON), _dp(lam), ens, _dp(POISON), _dp(POISON), _dp(POISON),
                                          _dp(gwind))
    else:
        rc = L.gel_propagate_adjoint_wind_device(plan, B, Q, shared, POISON, POISON, lam or None, ens, POISON, POISON, POISON, gwind or None)
    return rc, (L.gel_last_error() or b"").decode()


def test_refusals_on_a_host_only_handle_touch_no_buffer():
    from gelato_amd import _lib
    L = _lib.lib()
    E, other = it.engine(it.prob_of(NUM_NODES)), it.engine(it.prob_of(NUM_NODES))
    B = 5
    ens = E.wind_ensemble(members(33, (1, 2, 3))).assign([0, -1, 2, 1, 0])
    short = E.wind_ensemble(members(33, (1, 2, 3))).assign([0, -1, 2, 1])
    foreign = other.wind_ensemble(members(33, (1, 2, 3))).assign([0, -1, 2, 1, 0])
    unassigned = E.wind_ensemble(members(2, (1,)))
    chain, section, node = (E.propagation_plan(steps=1, restart=r) for r in ("chain", "section", "node"))
    for form in ("host", "device"):
        name_t = "gel_propagate_tangent_wind" + ("_device" if form == "device" else "")
        name_a = "gel_propagate_adjoint_wind" + ("_device" if form == "device" else "")
        for plan in (chain, section, node):
            for seeds in ({}, {"dx": 0}, {"ddisp": 0}, {"dx": 0, "ddisp": 0}, {"dwind": 0}):        # any non-empty subset of the three
                rc, msg = _tangent(L, form, plan._p, B, 3, 1, ens._p, **seeds)
                assert rc == GEL_ERR_ARG and msg.startswith(name_t + ":") and "host-only" in msg, msg
            rc, msg = _tangent(L, form, plan._p, B, 3, 1, None, dx=0, ddisp=0, dwind=0)
            assert rc == GEL_ERR_ARG and msg.startswith(name_t + ":") and "all three seeds" in msg, msg
            rc, msg = _tangent(L, form, plan._p, B, 3, 0, short._p)
            assert rc == GEL_ERR_ARG and "assigned 4 vectors, the call has B = 5" in msg, msg
            rc, msg = _tangent(L, form, plan._p, B, 3, 0, foreign._p)
            assert rc == GEL_ERR_ARG and "another handle" in msg, msg
            rc, msg = _tangent(L, form, plan._p, B, 3, 0, unassigned._p)
            assert rc == GEL_ERR_ARG and "no vectors yet" in msg, msg
            rc, msg = _tangent(L, form, plan._p, B, 0, 1, short._p)                                   # the parent's rules first
            assert rc == GEL_ERR_ARG and "P < 1" in msg, msg
            rc, msg = _tangent(L, form, plan._p, B, 3, 2, short._p)
            assert rc == GEL_ERR_ARG and "shared is neither 0 nor 1" in msg, msg
            rc, msg = _tangent(L, form, plan._p, -1, 3, 1, ens._p)
            assert rc == GEL_ERR_ARG and "B < 0" in msg, msg
            rc, msg = _tangent(L, form, plan._p, 65536, 65536, 1, ens._p)
            assert rc == GEL_ERR_ARG and "2^31" in msg, msg
            rc, msg = _tangent(L, form, plan._p, B, 3, 1, ens._p, x=0)
            assert rc == GEL_ERR_ARG and "x, y or dy is NULL" in msg, msg
            rc, msg = _tangent(L, form, None, B, 3, 1, ens._p)
            assert rc == GEL_ERR_ARG and msg.startswith(name_t + ": null plan"), msg
        for plan in (chain, section):
            for gw in (POISON, 0):
                rc, msg = _adjoint(L, form, plan._p, B, 2, 1, ens._p, gwind=gw)
                assert rc == GEL_ERR_ARG and msg.startswith(name_a + ":") and "host-only" in msg, msg
            rc, msg = _adjoint(L, form, plan._p, B, 2, 1, None)
            assert rc == GEL_ERR_ARG and "host-only" in msg, msg
            rc, msg = _adjoint(L, form, plan._p, B, 2, 0, short._p)
            assert rc == GEL_ERR_ARG and "assigned 4 vectors, the call has B = 5" in msg, msg
            rc, msg = _adjoint(L, form, plan._p, B, 2, 0, foreign._p)
            assert rc == GEL_ERR_ARG and "another handle" in msg, msg
            rc, msg = _adjoint(L, form, plan._p, B, 0, 1, short._p)
            assert rc == GEL_ERR_ARG and "Q < 1" in msg, msg
            rc, msg = _adjoint(L, form, plan._p, B, 2, 1, short._p, lam=0)
            assert rc == GEL_ERR_ARG and "lam is NULL" in msg, msg
            rc, msg = _adjoint(L, form, plan._p, B, 2, 3, short._p)
            assert rc == GEL_ERR_ARG and "shared is neither 0 nor 1" in msg, msg
            rc, msg = _adjoint(L, form, plan._p, B, 1 << 24, 0, short._p)
            assert rc == GEL_ERR_ARG and "1 GB" in msg, msg
            rc, msg = _adjoint(L, form, None, B, 2, 1, ens._p)
            assert rc == GEL_ERR_ARG and msg.startswith(name_a + ": null plan"), msg
        for e in (ens, short, None):
            rc, msg = _adjoint(L, form, node._p, B, 2, 1, e._p if e else None)
            assert rc == GEL_ERR_ARG and "GEL_PROP_RESTART_NODE" in msg, msg
    # the Python layer
    X = np.zeros((B, E.nvars))
    lam = np.ones((2, 11 * E.M))
    Kg = chain.wind_rows(ens)
    assert Kg == 33 and chain.wind_rows() == E.wind_altitudes.size == 9
    with pytest.raises(_lib.GelatoAmdError, match="host-only"):
        chain.tangent(X, dwind=np.ones((3, Kg, 2)), shared=True, ensemble=ens)
    with pytest.raises(ValueError, match="dwind"):
        chain.tangent(X, dwind=np.ones((3, 9, 2)), shared=True, ensemble=ens)          # the ensemble's row count, not the handle's
    with pytest.raises(ValueError, match="at least one"):
        chain.tangent(X)
    with pytest.raises(_lib.GelatoAmdError, match="host-only"):
        chain.adjoint(X, lam, shared=True, ensemble=ens, want_wind=True)
    with pytest.raises(ValueError, match="another engine"):
        other.propagation_plan(steps=1, restart="chain").wind_rows(ens)
    for o in (chain, section, node, ens, short, foreign, unassigned):
        o.close()
    other.close()


def test_wind_rows_and_adjoint_wind_info():
    """Kg = the handle's Kw, under an ensemble the larger of the two; the workspace grows by 16 Kg bytes per lane where gwind is wanted
    and is gel_prop_adjoint_info's where it is not; the 1 GB cap counts it"""
    from gelato_amd import _lib
    L = _lib.lib()
    E, other = it.engine(it.prob_of(NUM_NODES)), it.engine(it.prob_of(NUM_NODES))
    big, small = E.wind_ensemble(members(160, (1, 2))), E.wind_ensemble(members(2, (1,)))
    foreign = other.wind_ensemble(members(33, (1,)))
    kg = C.c_int32(-1)
    info = (C.c_int64 * 4)()
    for k in (1, 3):
        plan = E.propagation_plan(steps=k, restart="chain")
        assert plan.wind_rows() == 9 and plan.wind_rows(big) == 160 and plan.wind_rows(small) == 9
        base = plan.adjoint_info(67, 2)
        for ens, Kg in ((None, 9), (big, 160), (small, 9)):
            w = plan.adjoint_info(67, 2, want_wind=True, ensemble=ens)
            assert w["wind_rows"] == Kg and w["lane_bytes"] == base["lane_bytes"] + 16 * Kg, (w, base)
            per = w["lanes_per_slab"] // 2
            assert w["lanes_per_slab"] % 128 == 0 and w["lanes_per_slab"] <= base["lanes_per_slab"] and w["slabs"] == -(-67 // per)
            assert L.gel_prop_adjoint_wind_info(plan._p, ens._p if ens else None, 67, 2, 0, 0, info) == 0
            assert [int(v) for v in info] == [base["lane_bytes"], base["lanes_per_slab"], base["slabs"], Kg]
        # refusals, with the call's name
        for call, text in ((lambda: L.gel_prop_wind_rows(None, None, C.byref(kg)), "gel_prop_wind_rows: null plan"),
                           (lambda: L.gel_prop_wind_rows(plan._p, None, None), "gel_prop_wind_rows: Kg is NULL"),
                           (lambda: L.gel_prop_wind_rows(plan._p, foreign._p, C.byref(kg)), "gel_prop_wind_rows: the wind ensemble belongs to another handle"),
                           (lambda: L.gel_prop_adjoint_wind_info(plan._p, None, 67, 2, 0, 1, None), "gel_prop_adjoint_wind_info: info is NULL"),
                           (lambda: L.gel_prop_adjoint_wind_info(None, None, 67, 2, 0, 1, info), "gel_prop_adjoint_wind_info: null plan"),
                           (lambda: L.gel_prop_adjoint_wind_info(plan._p, foreign._p, 67, 2, 0, 1, info), "gel_prop_adjoint_wind_info: the wind ensemble belongs"),
                           (lambda: L.gel_prop_adjoint_wind_info(plan._p, None, 67, 0, 0, 1, info), "gel_prop_adjoint_wind_info: Q < 1"),
                           (lambda: L.gel_prop_adjoint_wind_info(plan._p, None, -1, 2, 0, 1, info), "gel_prop_adjoint_wind_info: B < 0"),
                           (lambda: L.gel_prop_adjoint_wind_info(plan._p, None, 67, 2, 2, 1, info), "shared is neither 0 nor 1"),
                           (lambda: L.gel_prop_adjoint_wind_info(plan._p, None, 67, 1 << 24, 0, 1, info), "1 GB")):
            assert call() == GEL_ERR_ARG and text in (L.gel_last_error() or b"").decode(), text
        plan.close()
    node = E.propagation_plan(steps=1, restart="node")
    assert L.gel_prop_adjoint_wind_info(node._p, None, 67, 2, 0, 1, info) == GEL_ERR_ARG and b"GEL_PROP_RESTART_NODE" in L.gel_last_error()
    # a functional count the parent still takes, refused once the wind rows of a long member are counted
    plan = E.propagation_plan(steps=1, restart="chain")
    lane = plan.adjoint_info(1, 1)["lane_bytes"]
    Q = (1 << 30) // (64 * (lane + 16 * 160)) + 1
    assert plan.adjoint_info(1, Q)["slabs"] == 1
    with pytest.raises(_lib.GelatoAmdError, match="1 GB"):
        plan.adjoint_info(1, Q, want_wind=True, ensemble=big)
    for o in (plan, node, big, small, foreign):
        o.close()
    other.close()


# ------------------------------------------------------------------ 3. the reader
def test_wind_linear_prediction():
    from gelato_amd import montecarlo as mc
    rng = np.random.default_rng(7)
    Kw, Kg, E = 9, 12, 4
    base = np.column_stack([np.linspace(0.0, 30000.0, Kw), rng.standard_normal((Kw, 2))])
    tables = np.stack([np.column_stack([base[:, 0], rng.standard_normal((Kw, 2))]) for _ in range(E)])
    g = rng.standard_normal((3, 5, Kg, 2))
    got = mc.wind_linear_prediction(g, base, tables)
    assert got.shape == (E, 3, 5)
    for e in range(E):
        for b in range(3):
            for q in range(5):
                want = sum(g[b, q, k, c] * (tables[e, k, 1 + c] - base[k, 1 + c]) for k in range(Kw) for c in range(2))
                assert abs(got[e, b, q] - want) <= 1e-13 * (1.0 + abs(want))
    assert np.all(mc.wind_linear_prediction(g, base, base) == 0.0) and mc.wind_linear_prediction(g, base, base).shape == (1, 3, 5)
    assert mc.wind_linear_prediction(g[0, 0], base, tables).shape == (E,)
    moved = tables.copy()
    moved[2, 4, 0] += 1.0
    with pytest.raises(ValueError, match="altitudes"):
        mc.wind_linear_prediction(g, base, moved)
    with pytest.raises(ValueError, match="rows"):
        mc.wind_linear_prediction(g, base, tables[:, :-1])
    with pytest.raises(ValueError, match="gwind"):
        mc.wind_linear_prediction(g[:, :, :Kw - 1], base, tables)


# ------------------------------------------------------------------ 4. under the sanitizers
@sanitized_lib.needs_toolchain
def test_entry_points_under_asan_ubsan(tmp_path):
    """every refusal of the new calls on host-only handles, with buffers of ONE double, in a stand-alone program
    (tests/flight_wind_sanitize.c) under AddressSanitizer + UBSan + LeakSanitizer, linked against the sanitized library directly;
    nothing is preloaded and nothing is launched"""
    sanitized_lib.run_program(tmp_path, sanitized_lib.build(tmp_path), "flight_wind_sanitize")

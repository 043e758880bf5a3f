"""The wind-profile sensitivities on node plans, plans whose step count differs by phase and the two-row table, host side (no GPU;
DESIGN.md 3.23): the conditions tests/golden/make_flight_wind_plans.py asserted of g36, re-asserted from what is stored; the stored
inputs are flight_tangent_truth.case's; the plans' matrices are the uniform plans'; and gel_prop_adjoint_wind_info /
gel_prop_tangent_info report the slab counts tests/test_flight_wind_plans.py asserts on the device."""
import numpy as np
import pytest

import flight_tangent_truth as tt
import flight_wind_truth as wt
import interp_truth as it
import mixed_steps as ms
from test_mixed_steps_cpu import check_plan_matrices
from test_wind_ensemble_cpu import members

_CASE = {}


def _case(name):
    """(prob, host-only engine, X, disp) of a case"""
    if name not in _CASE:
        prob, X, disp = tt.case(name)
        _CASE[name] = (prob, it.engine(prob), X, disp)
    return _CASE[name]


def g35_level(seed_ids):
    """the largest (a)-against-(b) figure g35 stores over its four flights for these seeds: what the same generator code reaches"""
    return max(float(wt.load(f)["ab"][seed_ids].max()) for f in wt.FLIGHTS)


@pytest.mark.parametrize("name", wt.PLAN_NAMES)
def test_conditions_of_the_truth(name):
    case, mode, steps = wt.PLAN_FLIGHTS[name]
    g = wt.load_plan(name)
    prob, E, X, disp = _case(case)
    nn, S, N, M = tt.layout(prob)
    Kw = np.asarray(prob["wind_table"]).shape[0]
    nsd = len(wt.SEEDS)
    adjoint = name in wt.PLAN_ADJOINT
    # the stored inputs are the case's
    assert np.array_equal(g["x"], X[wt.TRUTH_VEC]) and np.array_equal(g["disp"], disp[wt.TRUTH_VEC])
    assert g["dy"].shape == g["bound"].shape == (nsd, M, 11)
    assert ("gW" in g) == adjoint and ("Eg" in g) == adjoint and ("dual" in g) == adjoint
    assert not any(k in g for k in ("F", "J", "Pu", "Pf", "Pw", "piece", "th"))          # no per-stage data
    # (a) central against (b), all seven seeds: within one decade of what g35 reaches for them (6.7e-44 -> 6.7e-43)
    level = g35_level(np.arange(nsd))
    print("%s: (a) against (b) %.2e (g35: %.2e), forward against backward %.2e" % (name, g["ab"].max(), level, g["fb"].max()))
    assert g["ab"].shape == (nsd,) and g["ab"].max() <= 10 * level, (g["ab"], level)
    assert g["fb"].shape == (nsd,) and g["fb"].max() < 1e-20, g["fb"]
    # the seeds are flight_wind_truth's, the bump at the stored row
    cnt = dict(zip(wt.COUNTS, (int(v) for v in g["counts"])))
    dW, dX, dD = wt.seeds(prob, g["x"])
    assert np.array_equal(g["dW"][1:], dW[1:]) and np.count_nonzero(g["dW"][0]) == 1 and g["dW"][0, cnt["bump"], 0] == 1.0
    # the counts
    assert cnt["air"] > 0 and cnt["inside"] > 0
    if name in wt.PLAN_E:
        assert tuple(steps) == ms.E_STEPS and cnt["air_k2"] > 0 and cnt["air_k3"] > 0 and cnt["lo"] > 0 and cnt["hi"] > 0, cnt
    if name == "W-MIN":
        assert Kw == 2 and cnt["inside"] > 0 and cnt["above"] > 0, cnt       # inside the one piece, and over the table with Pw != 0
    if name == "W-node":
        assert cnt["air_j1"] > 0 and cnt["lo"] > 0 and cnt["hi"] > 0, cnt    # the restart matters
    # bounds finite; where a bound is zero the truth is exact: zero, or the seed's own entry of a segment's start row
    rows = np.array([tt.state_rows(M, i) for i in range(M)])
    for d in range(nsd):
        assert np.all(np.isfinite(g["bound"][d])) and np.all(g["bound"][d] >= 0)
        z = g["bound"][d] == 0
        assert np.all((g["dy"][d][z] == 0) | (g["dy"][d][z] == dX[d][rows][z])), wt.SEEDS[d]
        assert (np.abs(g["dy"][d]).max() > 0) == (g["bound"][d].max() > 0), wt.SEEDS[d]
    assert np.abs(g["dy"][[0, 1, 2, 5, 6]]).reshape(5, -1).max(axis=1).min() > 0
    if adjoint:
        assert g["gW"].shape == g["Eg"].shape == (wt.NQ, Kw, 2) and float(g["dual"]) < 1e-50
        assert np.all(np.isfinite(g["Eg"])) and np.all(g["Eg"] >= 0) and np.all(g["gW"][g["Eg"] == 0] == 0)
        lam = wt.functionals(prob)
        for q in range(wt.NQ):          # fp64 duality of the stored arrays, within the stored bounds
            for d in range(6):
                lhs, rhs = (lam[q] * g["dy"][d]).sum(), (g["gW"][q] * g["dW"][d]).sum()
                tol = (np.abs(lam[q]) * g["bound"][d]).sum() + (g["Eg"][q] * np.abs(g["dW"][d])).sum() + 1e-13 * (abs(lhs) + abs(rhs))
                assert abs(lhs - rhs) <= tol, (name, q, d, lhs, rhs, tol)
    if name == "W-MIN":     # both rows carry stages: the end-row seeds move the flight, every functional that feels the wind has both rows
        assert np.abs(g["dy"][3]).max() > 2 * g["bound"][3].max() and np.abs(g["dy"][4]).max() > 2 * g["bound"][4].max()
        assert np.all(np.abs(g["gW"][1:7]).reshape(6, 2, 2).max(axis=2) > 0)


@pytest.mark.parametrize("name", wt.PLAN_E)
def test_teeth_rolled_steps(name):
    """the 80-digit dy and gW of the rolled step assignment miss 2 E / 2 Eg of the right plan by more than 1e3"""
    g = wt.load_plan(name)
    assert g["dy_rolled"].shape == g["dy"].shape and g["gW_rolled"].shape == g["gW"].shape
    t_dy = max(wt.miss_bounded(g["dy_rolled"][d], g["dy"][d], 2 * g["bound"][d]) for d in range(len(wt.SEEDS)))
    t_w = max(wt.miss_bounded(g["dy_rolled"][d], g["dy"][d], 2 * g["bound"][d]) for d in range(6))          # the pure wind seeds alone
    t_gw = max(wt.miss_bounded(g["gW_rolled"][q], g["gW"][q], 2 * g["Eg"][q]) for q in range(wt.NQ))
    print("%s under the rolled steps: misses 2 E by %.3g (pure wind seeds %.3g), 2 Eg by %.3g" % (name, t_dy, t_w, t_gw))
    assert t_dy > 1.0e3 and t_w > 1.0e3 and t_gw > 1.0e3
    assert np.array_equal(g["teeth"], [t_dy, t_gw])


def test_teeth_node_plan_restated_as_a_section_plan():
    """W-node's seeds flown on the section plan: the rows of every phase's first interval are the node plan's, the rows past it miss
    2 E by more than 1e3"""
    g = wt.load_plan("W-node")
    prob = _case("example")[0]
    first, later = wt.node_rows(tt.layout(prob)[0])
    assert len(first) + len(later) == tt.layout(prob)[3]
    for d in range(len(wt.SEEDS)):
        assert wt.miss(g["dy_section"][d][first], g["dy"][d][first], g["bound"][d][first]) <= 1.0, wt.SEEDS[d]
    per = [wt.miss_bounded(g["dy_section"][d][later], g["dy"][d][later], 2 * g["bound"][d][later]) for d in range(len(wt.SEEDS))]
    print("W-node restated in section mode: misses 2 E on the later rows by %s" % np.array2string(np.array(per), precision=3))
    assert max(per) > 1.0e3 and all(per[d] > 1.0e3 for d in (0, 5, 6)), per
    assert g["teeth"][0] == max(per)


@pytest.mark.parametrize("name", wt.PLAN_NAMES)
def test_plan_matrices_are_the_uniform_plans(name):
    """the node plan's, the mixed plans' and the MIN flight's matrices, asked of a host-only handle, are the uniform plans'"""
    case, mode, steps = wt.PLAN_FLIGHTS[name]
    prob, E, X, disp = _case(case)
    ks = tt.steps_of(steps, E.S)
    mats, hs = tt.plan_tables(E, ks, mode)
    check_plan_matrices(name, E, mode, ks, mats, hs)


@pytest.mark.parametrize("mode", ["chain", "section"])
def test_slab_counts_of_the_device_tests(mode, monkeypatch):
    """B = 130, P = Q = 2, per-lane seeds, on the E_STEPS plan: one slab, three with GEL_PROP_SLAB=64 -- with and without a 33-row
    ensemble (gel_prop_tangent_info, gel_prop_adjoint_wind_info; the device tests assert the same on their handles)"""
    prob, E, X, disp = _case("example")
    plan = E.propagation_plan(steps=list(ms.E_STEPS), restart=mode)
    ens = E.wind_ensemble(members(33, (1976, 12), calm_of=1))
    for slab, want in ((None, 1), ("64", 3)):
        if slab:
            monkeypatch.setenv("GEL_PROP_SLAB", slab)
        assert plan.tangent_info(130, 2, shared=False)["slabs"] == want
        for e, Kg in ((None, 9), (ens, 33)):
            info = plan.adjoint_info(130, 2, shared=False, want_wind=True, ensemble=e)
            assert info["slabs"] == want and info["wind_rows"] == Kg, (slab, info)
            assert info["lane_bytes"] == plan.adjoint_info(130, 2)["lane_bytes"] + 16 * Kg
    monkeypatch.delenv("GEL_PROP_SLAB")
    ens.close()
    plan.close()

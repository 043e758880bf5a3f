"""Plans whose step count differs by phase, host side (no GPU; host-only handles; tests/mixed_steps.py): the mixed plan's data is the
uniform plans', phase by phase; the conditions the truth of g32 and g33 must meet, as tests/test_flight_tangent_cpu.py and
tests/test_flight_adjoint_cpu.py state them for g30 and g31; and the teeth: a flight under a wrong assignment of the same step counts
is far outside the bound of the right one, in the 60-digit truth and in the fp64 value restatement."""
import numpy as np
import pytest

import flight_adjoint_truth as at
import flight_tangent_truth as tt
import flight_truth as ft
import interp_truth as it
import mixed_steps as ms


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


_CASE = {}


def _case(name):
    """(prob, host-only engine, X, disp, mode, steps, (mats, hs)) of one of ms.NAMES"""
    if name not in _CASE:
        case, mode, steps = ms.CASES[name]
        prob, X, disp = tt.case(case)
        E = it.engine(prob)
        _CASE[name] = (prob, E, X, disp, mode, steps, tt.plan_tables(E, steps, mode))
    return _CASE[name]


def check_plan_matrices(name, E, mode, steps, mats, hs):
    """for every phase s the stage points, the control matrix and the copy list of the plan with these per-phase steps are, bit for
    bit, those of the uniform plan steps = steps[s]; so are the step fractions of tt.plan_tables.  In the given mode and in the node
    mode.  (shared with tests/test_flight_wind_plans_cpu.py)"""
    uniform = {}
    for md in (mode, "node"):
        plan = E.propagation_plan(steps=list(steps), restart=md)
        assert plan.steps == list(steps)
        for s, k in enumerate(steps):
            if (md, k) not in uniform:
                p = E.propagation_plan(steps=k, restart=md)
                uniform[(md, k)] = ([p.matrices(r) for r in range(E.S)], tt.plan_tables(E, k, md)[1])
                p.close()
            um, uhs = uniform[(md, k)]
            m = plan.matrices(s)
            assert m["pts"].shape == (2 * k * int(E.num_nodes[s]) + 1,)
            for key in ("pts", "Wu"):
                assert np.array_equal(_bits(m[key]), _bits(um[s][key])), (name, md, s, key)
            assert np.array_equal(m["copy_u"], um[s]["copy_u"]), (name, md, s)
            if md == mode:
                assert np.array_equal(_bits(hs[s]), _bits(uhs[s])), (name, s)
                assert all(np.array_equal(_bits(mats[s][key]), _bits(m[key])) for key in ("pts", "Wu")) and np.array_equal(mats[s]["copy_u"], m["copy_u"])
        plan.close()


@pytest.mark.parametrize("name", ms.NAMES)
def test_plan_matrices_are_the_uniform_plans(name):
    """(a) for every phase s the stage points, the control matrix and the copy list of the mixed plan are, bit for bit, those of the
    uniform plan steps = steps[s]; so are the step fractions of tt.plan_tables.  In the flight's mode and in the node mode."""
    prob, E, X, disp, mode, steps, (mats, hs) = _case(name)
    check_plan_matrices(name, E, mode, steps, mats, hs)


@pytest.mark.parametrize("name", ms.NAMES)
def test_truth_conditions(name):
    """(b) the stored inputs are the case's; the whole map's central quotient and the recursion agree to 1e-30 of a direction's
    largest entry; the forward and the backward quotient agree, so no kink lies within h of a stage; the bounds are finite; the
    60-digit duality of the adjoint against the recursion holds to 1e-30; the teeth are stored for every wrong assignment"""
    prob, E, X, disp, mode, steps, _t = _case(name)
    g = ms.load(name)
    M, nv = tt.layout(prob)[3], X.shape[1]
    assert np.array_equal(_bits(g["x"]), _bits(X[tt.TRUTH_VEC])) and np.array_equal(_bits(g["disp"]), _bits(disp[tt.TRUTH_VEC]))
    assert g["dy"].shape == (11, M, 11) and g["bound"].shape == (11, M, 11) and g["y"].shape == (M, 11)
    assert g["gx"].shape == (7, nv) and g["Egx"].shape == (7, nv) and g["gdisp"].shape == (7, E.S, 4) and g["Egd"].shape == (7, E.S, 4)
    assert np.all(g["ab"] <= 1e-30), g["ab"]
    assert float(g["dual"]) <= 1e-30, g["dual"]
    for k in ("bound", "Egx", "Egd"):
        assert np.all(np.isfinite(g[k])) and np.all(g[k] >= 0), k
    for k in ("teeth", "teeth_dy", "teeth_gx"):
        assert g[k].shape == (len(ms.WRONG),), k
    air = name not in ms.N_NAMES
    for d, dname in enumerate(tt.DIRECTIONS):
        big = np.abs(g["dy"][d]).max()
        assert (big > 0) == (air or dname not in ("area_all", "wind_all")), dname
        if air:
            assert g["fb"][d] <= 1e-18, dname
        else:
            assert np.abs(g["dy"][d] - g["dy_a"][d]).max() <= 4 * tt.U * big, dname     # (both stored rounded to fp64)
            assert np.abs(g["dy_f"][d] - g["dy_b"][d]).max() <= 1e-18 * big + 1e-300, dname
    assert np.all(np.abs(g["gx"]).max(axis=1) > 0) and np.any(g["gdisp"] != 0)


@pytest.mark.parametrize("name", ms.N_NAMES)
def test_duality_pins_the_restatements(name):
    """(b) in 60-digit arithmetic over the stored per-stage data, for the 11 seeds and the 7 functionals:
    <gx, dX> + <gdisp, dD> = <lam, recursion(dX, dD)> to 1e-30 relative; the stored gx and gdisp are that run's, rounded"""
    import mpmath
    mpmath.mp.dps = 60
    mpf = mpmath.mpf
    num = lambda v: mpf(float(v))   # noqa: E731

    def marr(a):
        a = np.asarray(a, dtype=float)
        out = np.empty(a.shape, dtype=object)
        for i in np.ndindex(a.shape):
            out[i] = mpf(float(a[i]))
        return out

    prob, E, X, disp, mode, steps, (mats, hs) = _case(name)
    g = ms.load(name)
    st = {k: marr(g[k]) for k in ("F", "J", "Pu", "Pf")}
    xm = marr(g["x"])
    dX, dD = tt.directions(prob, g["x"])
    lam = at.functionals(prob, g["x"])
    dys = [tt.recursion(prob, mode, steps, xm, mats, hs, st, marr(dX[d]), marr(dD[d]), num=num) for d in range(11)]
    worst = mpf(0)
    for q in range(7):
        lm = marr(lam[q])
        gx, gd = at.adjoint(prob, mode, steps, xm, mats, hs, st, lm, num=num)
        assert np.array_equal(gx.astype(float), g["gx"][q]) and np.array_equal(gd.astype(float), g["gdisp"][q])
        for d in range(11):
            left = (gx * marr(dX[d])).sum() + (gd * marr(dD[d])).sum()
            right = (lm * dys[d]).sum()
            scale = (abs(gx) * abs(marr(dX[d]))).sum() + (abs(gd) * abs(marr(dD[d]))).sum() + (abs(lm) * abs(dys[d])).sum()
            if scale != 0:
                worst = max(worst, abs(left - right) / scale)
            else:
                assert left == right
    print("%s: duality to %.2e" % (name, float(worst)))
    assert worst <= mpf("1e-30")


def _tangent_mutations(mode):
    return [m for m in tt.MUTATIONS if m != "no_wind_slope" and not (m == "no_djump" and mode != "chain")]   # (no air: no wind)


def _adjoint_mutations(mode):
    return [m for m in at.MUTATIONS if not (m == "no_knot_minus" and mode != "chain")]


@pytest.mark.parametrize("name", ms.N_NAMES)
def test_fp64_restatements_inside_half_the_bound_and_mutations_outside(name):
    """(b) the tangent recursion and its transpose in fp64 over the stored partials stay within 0.5 x 2 E / 2 Eg of the truth in every
    entry, zero pattern included; every wrong restatement misses by more than 1e3"""
    prob, E, X, disp, mode, steps, (mats, hs) = _case(name)
    g = ms.load(name)
    dX, dD = tt.directions(prob, g["x"])
    lam = at.functionals(prob, g["x"])
    for mut in [None] + _tangent_mutations(mode):
        worst = 0.0
        for d in range(11):
            r = tt.recursion(prob, mode, steps, g["x"], mats, hs, g, dX[d], dD[d], mutate=mut)
            if mut is None:
                assert np.array_equal(r != 0, g["dy"][d] != 0), tt.DIRECTIONS[d]
            worst = max(worst, at.miss(r, g["dy"][d], 2 * g["bound"][d]))
        print("%s tangent, %s: at most %.3g of 2 E" % (name, mut, worst))
        assert (worst <= 0.5) if mut is None else (worst > 1.0e3), (name, mut, worst)
    for mut in [None] + _adjoint_mutations(mode):
        worst = 0.0
        for q in range(7):
            gx, gd = at.adjoint(prob, mode, steps, g["x"], mats, hs, g, lam[q], mutate=mut)
            if mut is None:
                assert np.array_equal(gx != 0, g["gx"][q] != 0) and np.array_equal(gd != 0, g["gdisp"][q] != 0), at.FUNCTIONALS[q]
            worst = max(worst, at.miss(gx, g["gx"][q], 2 * g["Egx"][q]), at.miss(gd, g["gdisp"][q], 2 * g["Egd"][q]))
        print("%s adjoint, %s: at most %.3g of 2 Eg" % (name, mut, worst))
        assert (worst <= 0.5) if mut is None else (worst > 1.0e3), (name, mut, worst)


def test_adjoint_refuses_a_section_plan_longer_than_a_chain_may_be():
    """one (vector, functional) of the adjoint walks every phase of a section plan too (the inner checkpoints are the lane's), so it
    holds a section plan to the chain's limit: the sum of steps[s] n_s at most 2^20.  The value and tangent calls keep the per-phase
    limit; 2^20 itself is accepted.  (16 phases of 8 nodes that all hold their attitude, 8192 steps each: no control samples and 720 KB
    of inner checkpoints per lane, so the 1 GB workspace cap stays out of it.)"""
    from gelato_amd import _lib
    prob = it.prob_of([8] * 16)
    prob["attitude_hold"] = np.ones(16, dtype=np.int32)
    E = it.engine(prob)
    for steps, ok in (([8192] * 16, True), ([8192] * 15 + [8193], False)):
        plan = E.propagation_plan(steps=steps, restart="section")
        assert plan.tangent_info(1, 1)["slabs"] == 1
        if ok:
            assert plan.adjoint_info(1, 1)["slabs"] == 1
        else:
            with pytest.raises(_lib.GelatoAmdError, match="2\\^20 RK4 steps in one lane"):
                plan.adjoint_info(1, 1)
            with pytest.raises(_lib.GelatoAmdError, match="2\\^20 RK4 steps in one lane"):
                plan.adjoint(np.zeros((1, E.nvars)), np.zeros((1, 1, 11 * E.M)))
        plan.close()


@pytest.mark.parametrize("name", ms.NAMES)
def test_teeth_against_wrong_step_assignments(name):
    """(c) reference against reference: the 60-digit dy and gx under each wrong assignment of the same counts miss 2 E / 2 Eg of the
    right one by more than 1e3 (the rolled one in dy AND in gx: the device test flies that plan), and so does the fp64 value flight
    ft.fly_all against the 2 E of the right plan's"""
    prob, E, X, disp, mode, steps, _t = _case(name)
    g = ms.load(name)
    print("%s: stored teeth %s (dy %s, gx %s)" % (name, g["teeth"], g["teeth_dy"], g["teeth_gx"]))
    assert np.array_equal(g["teeth"], np.maximum(g["teeth_dy"], g["teeth_gx"]))
    assert np.all(g["teeth"] > 1.0e3), g["teeth"]
    w = ms.WRONG.index("rolled")
    assert g["teeth_dy"][w] > 1.0e3 and g["teeth_gx"][w] > 1.0e3
    b = tt.TRUTH_VEC
    kw = {"chain": mode == "chain"}
    plan = E.propagation_plan(steps=list(steps), restart=mode)
    y, by, _e, _be = ft.fly_all(E, plan, prob, X[b], disp=disp[b], **kw)
    plan.close()
    assert np.all(np.isfinite(y)) and np.all(np.isfinite(by))
    for how in ms.WRONG:
        wrong = E.propagation_plan(steps=list(ms.wrong_steps(steps, how)), restart=mode)
        yw = ft.fly_all(E, wrong, prob, X[b], disp=disp[b], want_bound=False, **kw)[0]
        wrong.close()
        d = np.abs(yw - y)
        ok = np.isfinite(d) & (by > 0)
        miss = float((d[ok] / by[ok]).max())
        print("%s, value flight under the %s steps: misses 2 E by a factor %.3g" % (name, how, miss))
        assert miss > 1.0e3, (name, how, miss)

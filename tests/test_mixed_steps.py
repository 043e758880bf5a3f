"""The flight kernels on plans whose RK4 step count differs by phase (tests/mixed_steps.py).  Every
kernel forms its phase's offsets -- stage points, control samples, step fractions, the adjoint's inner checkpoints -- from the plan's
per-phase counts; with one count for all phases a wrong offset changes no result.  Here every phase's count differs from its
predecessor's:

  a  the value flight against flight_truth.fly_all within its 2 E, plain and dispersed, chain, section and node mode
  b  phase-locality, bit for bit and without a fixture: phase s of the mixed plan is phase s of the uniform plan steps = steps[s]
     (section and node mode; y, dy, and the adjoint of a functional supported on phase s), and a chain does not feel what follows
  c  the tangent against the 60-digit truth of g32 / g33 within 2 E
  d  the adjoint against it within 2 Eg, the bound's teeth around the device's values, the device's duality
  e  the device's own wrong plan (the steps rolled by one phase) far outside the bound
  f  a wind ensemble: bit for bit one engine per member
  g  the host form against the device form into poisoned buffers"""
import os
from fractions import Fraction

import numpy as np
import pytest

import flight_adjoint_truth as at
import flight_truth as ft
import flight_tangent_truth as tt
import mixed_steps as ms
import propagate_truth as pt

pytestmark = pytest.mark.gpu
B130 = 130
SEL = [tt.DIRECTIONS.index(n) for n in ("position0_y", "knot_time", "u0_bias", "dense")]    # the seeds of the bit-exact tests


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(_bits(a), _bits(b))


_CASE = {}


def _case(case):
    """(prob, engine, X [3, nvars], disp [3, S, 4], dX [3, 11, nvars], dD [3, 11, S, 4], Lam [3, 7, 11 M]) of "noair" / "example\""""
    if case not in _CASE:
        from gelato_amd import Engine
        prob, X, disp = tt.case(case)
        seeds = [tt.directions(prob, X[b]) for b in range(3)]
        Lam = np.stack([at.pack_lam(at.functionals(prob, X[b])) for b in range(3)])
        _CASE[case] = (prob, Engine(prob), X, disp, np.stack([s[0] for s in seeds]), np.stack([s[1] for s in seeds]), Lam)
    return _CASE[case]


_DEV = {}


def _device(name, how=None):
    """the device's tangent (Y, dY) and adjoint (Y, GX, GD) of the flight's batch on its plan (how: on a wrong plan of ms.WRONG)"""
    if (name, how) not in _DEV:
        case, mode, steps = ms.CASES[name]
        prob, E, X, disp, dX, dD, Lam = _case(case)
        plan = E.propagation_plan(steps=list(ms.wrong_steps(steps, how) if how else steps), restart=mode)
        Y, dY, rc = plan.tangent(X, dX=dX, dispersion=disp, ddispersion=dD)
        Y2, GX, GD, rc2 = plan.adjoint(X, Lam, dispersion=disp)
        plan.close()
        assert rc == 0 and rc2 == 0 and same(Y, Y2)
        _DEV[(name, how)] = (Y, dY, GX, GD)
    return _DEV[(name, how)]


# ------------------------------------------------------------------ a. the value flight
VALUE_FLIGHTS = [(n, ms.CASES[n][1]) for n in ms.NAMES] + [(n, "node") for n in ("N-chain", "N-section", "E-chain")]


@pytest.mark.parametrize("dispersed", [False, True], ids=["plain", "dispersed"])
@pytest.mark.parametrize("name,mode", VALUE_FLIGHTS, ids=lambda v: str(v))
def test_value_flight(name, mode, dispersed):
    """y and err of the three vectors against flight_truth.fly_all (which reads plan.steps[s] per phase) within 2 E, err as
    tests/test_flight.py checks it; mode "node": the same steps on a node-restart plan"""
    from test_flight import check_parity
    case, _mode, steps = ms.CASES[name]
    prob, E, X, disp, _dX, _dD, _L = _case(case)
    plan = E.propagation_plan(steps=list(steps), restart=mode)
    D = disp if dispersed else None
    Y, err, rc = plan.apply(X, dispersion=D)
    assert rc == 0
    kw = {"restart": "node"} if mode == "node" else {"chain": mode == "chain"}
    ref = [ft.fly_all(E, plan, prob, X[b], disp=None if D is None else D[b], **kw) for b in range(3)]
    plan.close()
    use, _last, worst = check_parity(E, Y, err, ref)
    print("share of 2 E used, %s %s %s %s: y %s err %s" % (name, mode, steps, "dispersed" if dispersed else "plain",
                                                         np.array2string(use[0], precision=3), np.array2string(use[1], precision=3)))
    assert all(wy <= 1.0 and we <= 1.0 for wy, we in worst), (name, mode, worst)


# ------------------------------------------------------------------ b. phase-locality
def _batch130(case):
    prob, E, X, disp, dX, dD, Lam = _case(case)
    idx = np.arange(B130) % 3
    return prob, E, np.ascontiguousarray(X[idx]), np.ascontiguousarray(disp[idx]), np.ascontiguousarray(dX[idx][:, SEL]), np.ascontiguousarray(dD[idx][:, SEL])


def _under_slabs(call):
    """call() once as it is and once under GEL_PROP_SLAB=64 (130 vectors: three slabs) -> the first result, the two being equal in bits"""
    out = []
    for slab in (None, "64"):
        if slab:
            os.environ["GEL_PROP_SLAB"] = slab
        try:
            out.append(call())
        finally:
            os.environ.pop("GEL_PROP_SLAB", None)
    assert all(same(u, v) for u, v in zip(out[0], out[1])), "a slab of 64 changes bits"
    return out[0]


def _fly(plan, X, D, dX, dD):
    """(y [B, M, 11], dy per-vector seeds [B, P, M, 11], dy shared seeds (vector 0's)) of a plan"""
    M = plan.M
    Y, dY, rc = plan.tangent(X, dX=dX, dispersion=D, ddispersion=dD)
    Ys, dYs, rcs = plan.tangent(X, dX=np.ascontiguousarray(dX[0]), dispersion=D, ddispersion=np.ascontiguousarray(dD[0]), shared=True)
    Y0, _e, rc0 = plan.apply(X, want_err=False, dispersion=D)
    assert rc == 0 and rcs == 0 and rc0 == 0 and same(Y, Ys) and same(Y, Y0)
    return tt.unpack_dy(Y, M), tt.unpack_dy(dY, M), tt.unpack_dy(dYs, M)


@pytest.mark.parametrize("mode", ["section", "node"])
@pytest.mark.parametrize("name", ["N-chain", "N-section", "E-chain"])
def test_phase_locality_section_and_node(name, mode):
    """without a carry a phase reads nothing of the others: the rows of phase s of y and dy (per-vector and shared seeds) from the
    mixed plan are, bit for bit, those of the uniform plan steps = steps[s].  B = 130, also in slabs of 64."""
    case, _mode, steps = ms.CASES[name]
    prob, E, X, D, dX, dD = _batch130(case)
    rows = ms.phase_rows([int(v) for v in E.num_nodes])
    plan = E.propagation_plan(steps=list(steps), restart=mode)
    got = _under_slabs(lambda: _fly(plan, X, D, dX, dD))
    plan.close()
    assert np.all(np.isfinite(got[1])) and np.any(got[1] != 0)
    for k in sorted(set(steps)):
        uni = E.propagation_plan(steps=k, restart=mode)
        ref = _fly(uni, X, D, dX, dD)
        uni.close()
        for s in [s for s in range(E.S) if steps[s] == k]:
            assert same(got[0][:, rows[s]], ref[0][:, rows[s]]), (name, mode, s, "y")
            assert same(got[1][:, :, rows[s]], ref[1][:, :, rows[s]]), (name, mode, s, "dy")
            assert same(got[2][:, :, rows[s]], ref[2][:, :, rows[s]]), (name, mode, s, "dy, shared seeds")
        for s in [s for s in range(E.S) if steps[s] != k and int(E.num_nodes[s]) > 1]:     # (and k matters: the other phases differ)
            assert not same(got[0][:, rows[s]], ref[0][:, rows[s]]), (name, mode, s)


@pytest.mark.parametrize("name", ["N-section", "E-section"])
def test_phase_locality_section_adjoint(name):
    """section plan: for a functional supported on the rows of phase s alone, gx and gdisp are, bit for bit, the uniform plan's
    steps = steps[s].  One functional per phase (Q = S), B = 130, also in slabs of 64."""
    case, mode, steps = ms.CASES[name]
    prob, E, X, D, _dX, _dD = _batch130(case)
    M, S = E.M, E.S
    rows = ms.phase_rows([int(v) for v in E.num_nodes])
    dense = np.random.default_rng(33).standard_normal((M, 11))
    lam = np.zeros((S, M, 11))
    for s in range(S):
        lam[s, rows[s]] = dense[rows[s]]
    Lam = at.pack_lam(lam)
    plan = E.propagation_plan(steps=list(steps), restart=mode)
    _Y, GX, GD = _under_slabs(lambda: plan.adjoint(X, Lam, dispersion=D, shared=True)[:3])
    plan.close()
    assert np.all(np.isfinite(GX)) and np.all(np.abs(GX).max(axis=(0, 2)) > 0)
    for k in sorted(set(steps)):
        uni = E.propagation_plan(steps=k, restart=mode)
        _Yu, GXu, GDu, rc = uni.adjoint(X, Lam, dispersion=D, shared=True)
        uni.close()
        assert rc == 0
        for s in range(S):
            if steps[s] == k:
                assert same(GX[:, s], GXu[:, s]) and same(GD[:, s], GDu[:, s]), (name, s)
            elif int(E.num_nodes[s]) > 1:
                assert not same(GX[:, s], GXu[:, s]), (name, s)


def test_section_adjoint_inner_checkpoints_have_one_user():
    """the regression case of the defect the test above found: the inner checkpoints [k_max - 1][11] are indexed by the lane
    (vector, functional) alone, and the section-mode adjoint ran one thread per (lane, phase) -- the S threads of a lane wrote and
    read the same cells at once.  A few lanes hid it (a thread read its own writes back from its CU's cache); 130 x 12 lanes on a
    UNIFORM plan of 3 steps showed it.  Now the lane's thread walks all its phases: every vector of the batch gives, bit for bit,
    what it gives alone."""
    prob, E, X, D, _dX, _dD = _batch130("example")
    M, S = E.M, E.S
    rows = ms.phase_rows([int(v) for v in E.num_nodes])
    dense = np.random.default_rng(34).standard_normal((M, 11))
    lam = np.zeros((S, M, 11))
    for s in range(S):
        lam[s, rows[s]] = dense[rows[s]]
    Lam = at.pack_lam(lam)
    plan = E.propagation_plan(steps=3, restart="section")
    Y, GX, GD, rc = plan.adjoint(X, Lam, dispersion=D, shared=True)
    assert rc == 0
    for b in (0, 1, 2):          # (the batch cycles through three vectors)
        y1, g1, d1, rc = plan.adjoint(X[b], Lam, dispersion=D[[b]], shared=True)
        assert rc == 0
        for pos in range(b, B130, 3):
            assert same(Y[pos], y1[0]) and same(GX[pos], g1[0]) and same(GD[pos], d1[0]), pos
    plan.close()


@pytest.mark.parametrize("name", ["N-chain", "E-chain"])
def test_phase_locality_chain_prefix(name):
    """chain plan: a plan that agrees with the mixed one on the phases 0..s and differs in every later one gives the same bits in
    the rows of the phases 0..s, for y and for dy (per-vector and shared seeds).  B = 130, also in slabs of 64."""
    case, mode, steps = ms.CASES[name]
    prob, E, X, D, dX, dD = _batch130(case)
    nn = [int(v) for v in E.num_nodes]
    rows = ms.phase_rows(nn)
    plan = E.propagation_plan(steps=list(steps), restart=mode)
    got = _under_slabs(lambda: _fly(plan, X, D, dX, dD))
    plan.close()
    for s in range(E.S - 1):
        other = list(steps[:s + 1]) + [k % 4 + 1 for k in steps[s + 1:]]
        p2 = E.propagation_plan(steps=other, restart=mode)
        ref = _fly(p2, X, D, dX, dD) if s % 4 else _under_slabs(lambda: _fly(p2, X, D, dX, dD))
        p2.close()
        head = slice(0, rows[s].stop)
        assert same(got[0][:, head], ref[0][:, head]), (name, s, "y")
        assert same(got[1][:, :, head], ref[1][:, :, head]) and same(got[2][:, :, head], ref[2][:, :, head]), (name, s, "dy")
        assert not same(got[0][:, head.stop:], ref[0][:, head.stop:]), (name, s)


# ------------------------------------------------------------------ c, d. against the 60-digit truth
@pytest.mark.parametrize("name", ms.NAMES)
def test_tangent_truth(name):
    """dy of vector 1 within 2 E of the fixture in every entry of all eleven directions, nothing masked, with its zero pattern"""
    case, mode, steps = ms.CASES[name]
    prob, E, X, disp, dX, dD, _L = _case(case)
    g = ms.load(name)
    Y, dY, _GX, _GD = _device(name)
    b = tt.TRUTH_VEC
    got = tt.unpack_dy(dY[b], E.M)
    assert np.abs(pt.unpack_y(Y[b], E.M) - g["y"]).max() <= 1e-9 * (1.0 + np.abs(g["y"]).max())
    use = np.zeros((11, 4))
    for d in range(11):
        assert np.array_equal(got[d] != 0, g["dy"][d] != 0), tt.DIRECTIONS[d]
        for k, (a, c) in enumerate(pt.GROUP_COLS):
            use[d, k] = at.miss(got[d][:, a:c], g["dy"][d][:, a:c], 2 * g["bound"][d][:, a:c])
    print("share of 2 E used, %s %s, per group (mass, position, velocity, quaternion): %s; per direction %s"
          % (name, steps, np.array2string(use.max(axis=0), precision=3), np.array2string(use.max(axis=1), precision=3)))
    assert np.all(use <= 1.0), (name, use)


@pytest.mark.parametrize("name", ms.NAMES)
def test_adjoint_truth(name):
    """gx and gdisp of vector 1 within 2 Eg of the fixture in every entry of the seven functionals, nothing masked, with its zero
    pattern"""
    case, mode, steps = ms.CASES[name]
    prob, E, X, disp, _dX, _dD, Lam = _case(case)
    g = ms.load(name)
    Y, _dY, GX, GD = _device(name)
    b = tt.TRUTH_VEC
    grp = at.groups(prob)
    use = np.zeros((7, 7))
    for q in range(7):
        assert np.array_equal(GX[b, q] != 0, g["gx"][q] != 0) and np.array_equal(GD[b, q] != 0, g["gdisp"][q] != 0), at.FUNCTIONALS[q]
        for k, gname in enumerate(at.GROUPS[:6]):
            i = grp[gname]
            use[q, k] = at.miss(GX[b, q][i], g["gx"][q][i], 2 * g["Egx"][q][i])
        use[q, 6] = at.miss(GD[b, q], g["gdisp"][q], 2 * g["Egd"][q])
    print("share of 2 Eg used, %s %s, per group %s: %s; per functional %s"
          % (name, steps, at.GROUPS, np.array2string(use.max(axis=0), precision=3), np.array2string(use.max(axis=1), precision=3)))
    assert np.all(use <= 1.0), (name, use)


@pytest.mark.parametrize("name", ms.N_NAMES)
def test_bounds_reject_wrong_restatements(name):
    """the same bounds, around the DEVICE's values, reject the wrong restatements evaluated from the stored per-stage partials"""
    import interp_truth as it
    case, mode, steps = ms.CASES[name]
    prob, E, X, disp, dX, dD, _L = _case(case)
    g = ms.load(name)
    _Y, dY, GX, GD = _device(name)
    b = tt.TRUTH_VEC
    got = tt.unpack_dy(dY[b], E.M)
    mats, hs = tt.plan_tables(it.engine(prob), steps, mode)
    lam = at.functionals(prob, g["x"])
    for mut in tt.MUTATIONS:
        if mut == "no_wind_slope" or (mut == "no_djump" and mode != "chain"):
            continue     # (no air: no wind; section mode: no knot is crossed)
        worst = max(at.miss(tt.recursion(prob, mode, steps, g["x"], mats, hs, g, dX[b, d], dD[b, d], mutate=mut), got[d], 2 * g["bound"][d])
                    for d in range(11))
        print("tangent mutation %s, %s: misses the bound around the device's dy by a factor %.3g" % (mut, name, worst))
        assert worst > 1.0e3, (name, mut, worst)
    for mut in at.MUTATIONS:
        if mut == "no_knot_minus" and mode != "chain":
            continue
        worst = 0.0
        for q in range(7):
            gx, gd = at.adjoint(prob, mode, steps, g["x"], mats, hs, g, lam[q], mutate=mut)
            worst = max(worst, at.miss(gx, GX[b, q], 2 * g["Egx"][q]), at.miss(gd, GD[b, q], 2 * g["Egd"][q]))
        print("adjoint mutation %s, %s: misses the bound around the device's values by a factor %.3g" % (mut, name, worst))
        assert worst > 1.0e3, (name, mut, worst)


def _exact_dot(a, b):
    """<a, b> of fp64 arrays without a rounding of the test's own"""
    a, b = np.ravel(a), np.ravel(b)
    return sum((Fraction(float(a[i])) * Fraction(float(b[i])) for i in np.flatnonzero((a != 0) & (b != 0))), Fraction(0))


@pytest.mark.parametrize("name", ms.NAMES)
def test_device_duality(name):
    """|<lam, dy_dev> - <gx_dev, dX> - <gdisp_dev, dD>| <= 2 sum |lam| E for the 7 x 11 pairs of vector 1.  The three inner products
    are formed exactly (rationals): where a functional sits on a row whose E is zero -- a section's first node, which is the seed
    itself -- the two sides must agree exactly, and a rounding of the test's own sums would be all there is to see."""
    case, mode, steps = ms.CASES[name]
    prob, E, X, disp, dX, dD, _L = _case(case)
    g = ms.load(name)
    _Y, dY, GX, GD = _device(name)
    b = tt.TRUTH_VEC
    lam = at.functionals(prob, X[b])
    dy = tt.unpack_dy(dY[b], E.M)
    worst = 0.0
    for q in range(7):
        for d in range(11):
            gap = abs(_exact_dot(lam[q], dy[d]) - _exact_dot(GX[b, q], dX[b, d]) - _exact_dot(GD[b, q], dD[b, d]))
            bound = 2 * float((np.abs(lam[q]) * g["bound"][d]).sum())
            worst = max(worst, float(gap / Fraction(bound)) if bound > 0 else (0.0 if gap == 0 else np.inf))
    print("%s %s: duality uses %.3g of 2 sum |lam| E" % (name, steps, worst))
    assert worst <= 1.0, (name, worst)


# ------------------------------------------------------------------ e. the device's own wrong plan
@pytest.mark.parametrize("name", ms.NAMES)
def test_rolled_steps_plan_is_rejected(name):
    """dy and gx of the plan whose steps are rolled by one phase -- every phase flown with its predecessor's count -- miss 2 E / 2 Eg
    of the fixture by more than 1e3, as the 60-digit truth of that plan does (the stored teeth): a kernel that took a neighbour's k
    would be seen"""
    case, mode, steps = ms.CASES[name]
    prob, E, X, disp, _dX, _dD, _L = _case(case)
    g = ms.load(name)
    _Y, dY, GX, GD = _device(name, "rolled")
    b = tt.TRUTH_VEC
    got = tt.unpack_dy(dY[b], E.M)
    miss_dy = max(at.miss(got[d], g["dy"][d], 2 * g["bound"][d]) for d in range(11))
    miss_gx = max(max(at.miss(GX[b, q], g["gx"][q], 2 * g["Egx"][q]), at.miss(GD[b, q], g["gdisp"][q], 2 * g["Egd"][q])) for q in range(7))
    w = ms.WRONG.index("rolled")
    print("%s, rolled steps %s: dy misses 2 E by %.3g (the truth of that plan: %.3g), gx misses 2 Eg by %.3g (%.3g)"
          % (name, ms.wrong_steps(steps, "rolled"), miss_dy, g["teeth_dy"][w], miss_gx, g["teeth_gx"][w]))
    assert miss_dy > 1.0e3 and miss_gx > 1.0e3, (name, miss_dy, miss_gx)


# ------------------------------------------------------------------ f. wind ensemble
def test_wind_ensemble_member_bits():
    """E-chain under K = 2 members, B = 3: apply, tangent and adjoint with ensemble= give, bit for bit, what an engine created with the
    member's wind table gives on a plan of the same steps (-1: the engine's own)"""
    from test_wind_ensemble import SEEDS, fly_checked, member_engines
    from test_wind_ensemble_cpu import members
    from test_wind_ensemble_tangent import adjoint_checked, mismatches, tangent_checked
    case, mode, steps = ms.CASES["E-chain"]
    prob, E, X, disp, dX, dD, Lam = _case(case)
    T = members(33, SEEDS[:2])
    eng = member_engines(("example", 33, 2), prob, T)
    sX, sD, sL = np.ascontiguousarray(dX[0][SEL]), np.ascontiguousarray(dD[0][SEL]), np.ascontiguousarray(Lam[0][[2, 4, 6]])
    plan = E.propagation_plan(steps=list(steps), restart=mode)
    plans = [e.propagation_plan(steps=list(steps), restart=mode) for e in eng]
    for assignment in (np.array([1, -1, 0], dtype=np.int32), np.array([0, 1, 1], dtype=np.int32)):
        ens = E.wind_ensemble(T).assign(assignment)
        calls = (lambda e, p, n: fly_checked(e, p, X, disp, n),
                 lambda e, p, n: tangent_checked(e, p, X, disp, sX, sD, True, n),
                 lambda e, p, n: adjoint_checked(e, p, X, disp, sL, True, n))
        for what, call in zip(("apply", "tangent", "adjoint"), calls):
            got = call(E, plan, ens)
            own = call(E, plan, None)
            refs = [call(e, p, None) for e, p in zip(eng, plans)]
            assert not mismatches(got, refs, own, assignment), (what, assignment)
            assert all(np.all(np.isfinite(a)) for a in got) and not same(refs[0][0], refs[1][0]), what
        ens.close()
    for p in plans + [plan]:
        p.close()


# ------------------------------------------------------------------ g. host form against device form
def test_host_form_is_device_form():
    """E-chain: tangent and adjoint through the host-buffer entry points give the bits of the device-buffer ones, which write into
    poisoned buffers and leave the row behind each output alone; status 0 everywhere"""
    from test_wind_ensemble_tangent import adjoint_checked, tangent_checked
    case, mode, steps = ms.CASES["E-chain"]
    prob, E, X, disp, dX, dD, Lam = _case(case)
    Y, dY, GX, GD = _device("E-chain")
    plan = E.propagation_plan(steps=list(steps), restart=mode)
    Yd, dYd = tangent_checked(E, plan, X, disp, dX, dD, False)
    assert same(Yd, Y) and same(dYd, dY)
    Ya, GXd, GDd = adjoint_checked(E, plan, X, disp, Lam, False)
    assert same(Ya, Y) and same(GXd, GX) and same(GDd, GD)
    sX, sD, sL = np.ascontiguousarray(dX[1]), np.ascontiguousarray(dD[1]), np.ascontiguousarray(Lam[1])
    Yh, dYh, rc = plan.tangent(X, dX=sX, dispersion=disp, ddispersion=sD, shared=True)
    Ys, dYs = tangent_checked(E, plan, X, disp, sX, sD, True)
    assert rc == 0 and same(Yh, Ys) and same(dYh, dYs) and same(dYh[1], dY[1])
    Yh, Gh, Dh, rc = plan.adjoint(X, sL, dispersion=disp, shared=True)
    Ys, Gs, Ds = adjoint_checked(E, plan, X, disp, sL, True)
    assert rc == 0 and same(Yh, Ys) and same(Gh, Gs) and same(Dh, Ds) and same(Gh[1], GX[1]) and same(Dh[1], GD[1])
    plan.close()

"""The tangent and the adjoint flight on every branch of the right-hand side (tests/kink_flight.py):
section_rhs_tangent and section_rhs_adjoint where `s2 > 0`, `inv_p > 0`, `tail.piece >= 0`, the atmosphere layer, the 86 km switch,
gravity's clamp and the CA table's clamps take the side no other device test takes.

  a  the truth of g34 (60 digits): dy within 2 E in section and node mode, k = 1, 2; gx, gdisp within 2 Eg in section mode; y is
     gel_propagate_dispersed's bit for bit; the share of the bound per class (= phase) and group is printed
  b  the stored wrong restatements of single branches are outside 2 E around the DEVICE's dy
  c  device duality over all directions and functionals, per-vector and shared seeds
  d  lanes on different branches in one wavefront: B = 130 cycling three vectors, bit for bit their one-vector calls, slabs of 64,
     a direction alone against among all
  e  linearity at the kinks: zero in, zero out; 2^-3 and 2^5 scale bit for bit
  f  under a wind ensemble: the handle's own rows and a table lying wholly above every stage, bit for bit one handle per member"""
import os
from fractions import Fraction

import numpy as np
import pytest

import flight_adjoint_truth as at
import flight_tangent_truth as tt
import kink_flight as kf
import propagate_truth as pt

pytestmark = pytest.mark.gpu
B130 = 130
PICK = (0, 1, 63, 64, 65, 129)
ALL = kf.FLIGHTS + (kf.ENDS,)            # the ENDS variant: tables windy and sloped at their ends (kink_flight.ENDS)
SECTION = [f for f in ALL if f[1] != "node"]
IDS = lambda f: "%s-%s-k%d" % f   # noqa: E731
# the teeth held on the case itself; kf.ENDS_TEETH are held on the ENDS variant (tests/test_flight_kinks_cpu.py says why)
BITING = ("axis_longitude_partial", "no_gravity_clamp", "neighbour_lapse", "hold_rows_free")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(_bits(a), _bits(b))


_CASE = {}


def _case(name="kinks"):
    """(prob, engine, X [3, nvars], disp [3, S, 4], dX [3, 16, nvars], dD [3, 16, S, 4], Lam [3, 9, 11 M]) of the case, or of its
    ENDS variant ("kinks@ENDS")"""
    if name not in _CASE:
        from gelato_amd import Engine
        prob, X, disp = tt.case(name)
        seeds = [kf.directions(prob, X[b]) for b in range(3)]
        Lam = np.stack([at.pack_lam(kf.functionals(prob, X[b])) for b in range(3)])
        _CASE[name] = (prob, Engine(prob), X, disp, np.stack([s[0] for s in seeds]), np.stack([s[1] for s in seeds]), Lam)
    return _CASE[name]


_DEV = {}


def _device(flight):
    """(Y, dY, GX, GD) of the batch of three on the flight's plan (GX, GD None in node mode: the adjoint has none); status 0, finite,
    y the value flight's bits"""
    if flight not in _DEV:
        name, mode, k = flight
        prob, E, X, disp, dX, dD, Lam = _case(name)
        plan = E.propagation_plan(steps=k, restart=mode)
        Y, dY, rc = plan.tangent(X, dX=dX, dispersion=disp, ddispersion=dD)
        Y0, _e, rc0 = plan.apply(X, want_err=False, dispersion=disp)
        assert rc == 0 and rc0 == 0 and same(Y, Y0), "y is not gel_propagate_dispersed's"
        assert np.all(np.isfinite(Y)) and np.all(np.isfinite(dY))
        GX = GD = None
        if mode != "node":
            Y2, GX, GD, rc2 = plan.adjoint(X, Lam, dispersion=disp)
            assert rc2 == 0 and same(Y, Y2) and np.all(np.isfinite(GX)) and np.all(np.isfinite(GD))
        plan.close()
        _DEV[flight] = (Y, dY, GX, GD)
    return _DEV[flight]


def _phase_rows(E):
    nn = [int(v) for v in E.num_nodes]
    return [slice(sum(nn[:s]) + s, sum(nn[:s]) + s + nn[s] + 1) for s in range(E.S)]


# ------------------------------------------------------------------ a. the truth
@pytest.mark.parametrize("flight", ALL, ids=IDS)
def test_tangent_truth(flight):
    """dy of the kink vector within 2 E of g34 in every entry of all 16 directions, nothing masked, with its zero pattern (y is
    the value flight's bit for bit: _device)"""
    prob, E, X, disp, dX, dD, _L = _case(flight[0])
    g = kf.load(flight)
    Y, dY, _GX, _GD = _device(flight)
    b = kf.TRUTH_VEC
    got = tt.unpack_dy(dY[b], E.M)
    rows = _phase_rows(E)
    use = np.zeros((E.S, 4))
    per_dir = np.zeros(len(kf.DIRECTIONS))
    for d, name in enumerate(kf.DIRECTIONS):
        assert np.array_equal(got[d] != 0, g["dy"][d] != 0), name
        for s in range(E.S):
            for k, (a, c) in enumerate(pt.GROUP_COLS):
                m = at.miss(got[d][rows[s], a:c], g["dy"][d][rows[s], a:c], 2 * g["bound"][d][rows[s], a:c])
                use[s, k] = max(use[s, k], m)
                per_dir[d] = max(per_dir[d], m)
    print("share of 2 E used, %s %s k=%d, per class (phase) x (mass, position, velocity, quaternion):" % flight)
    for s in range(E.S):
        print("  %-12s %s" % (kf.NAMES[s], np.array2string(use[s], precision=3)))
    print("  per direction %s" % np.array2string(per_dir, precision=3))
    assert np.all(use <= 1.0), (flight, use)


@pytest.mark.parametrize("flight", SECTION, ids=IDS)
def test_adjoint_truth(flight):
    """gx and gdisp of the kink vector within 2 Eg of g34 in every entry of the 9 functionals, nothing masked, with its zero pattern"""
    prob, E, X, disp, _dX, _dD, Lam = _case(flight[0])
    g = kf.load(flight)
    _Y, _dY, GX, GD = _device(flight)
    b = kf.TRUTH_VEC
    grp = at.groups(prob)
    Q = len(kf.FUNCTIONALS)
    use = np.zeros((Q, 7))
    for q in range(Q):
        assert np.array_equal(GX[b, q] != 0, g["gx"][q] != 0) and np.array_equal(GD[b, q] != 0, g["gdisp"][q] != 0), kf.FUNCTIONALS[q]
        for k, gname in enumerate(at.GROUPS[:6]):
            i = grp[gname]
            use[q, k] = at.miss(GX[b, q][i], g["gx"][q][i], 2 * g["Egx"][q][i])
        use[q, 6] = at.miss(GD[b, q], g["gdisp"][q], 2 * g["Egd"][q])
    # per class: the state rows of gx and the factor row of gdisp, phase by phase
    rows = _phase_rows(E)
    per = np.zeros(E.S)
    for s in range(E.S):
        idx = np.concatenate([tt.state_rows(E.M, r) for r in range(rows[s].start, rows[s].stop)])
        per[s] = max(max(at.miss(GX[b, q][idx], g["gx"][q][idx], 2 * g["Egx"][q][idx]),
                         at.miss(GD[b, q][s], g["gdisp"][q][s], 2 * g["Egd"][q][s])) for q in range(Q))
    print("share of 2 Eg used, %s %s k=%d, per group %s: %s" % (flight + (at.GROUPS, np.array2string(use.max(axis=0), precision=3))))
    print("  per class (phase): " + ", ".join("%s %.3g" % (kf.NAMES[s], per[s]) for s in range(E.S)))
    print("  per functional %s" % np.array2string(use.max(axis=1), precision=3))
    assert np.all(use <= 1.0), (flight, use)


# ------------------------------------------------------------------ b. teeth around the device's output
@pytest.mark.parametrize("flight", [kf.FULL, kf.ENDS], ids=IDS)
def test_bound_rejects_wrong_restatements_of_single_branches(flight):
    """every stored wrong restatement is outside 2 E around the DEVICE's dy by more than 1e3: four on the case itself; on the ENDS
    variant the end slope of the wind and of the CA table continued outside, and the on-axis longitude from the Earth angle of
    t = 0.  (The restatement that is identically the truth, rest_from_1e-100, is printed.)"""
    prob, E, X, disp, dX, dD, _L = _case(flight[0])
    g = kf.load(flight)
    _Y, dY, _GX, _GD = _device(flight)
    got = tt.unpack_dy(dY[kf.TRUTH_VEC], E.M)
    for tooth in (kf.TEETH if flight == kf.FULL else kf.ENDS_TEETH):
        f = max(at.miss(g["tooth_" + tooth][d], got[d], 2 * g["bound"][d]) for d in range(len(kf.DIRECTIONS)))
        print("%s, tooth %s: misses 2 E around the device's dy by %.3g" % (flight[0], tooth, f))
        if tooth in (BITING if flight == kf.FULL else kf.ENDS_TEETH):
            assert f > 1.0e3, (tooth, f)


# ------------------------------------------------------------------ c. device duality
def _exact_dot(a, b):
    a, b = np.ravel(a), np.ravel(b)
    return sum((Fraction(float(a[i])) * Fraction(float(b[i])) for i in np.flatnonzero((a != 0) & (b != 0))), Fraction(0))


@pytest.mark.parametrize("shared", [False, True], ids=["per-vector", "shared"])
@pytest.mark.parametrize("flight", SECTION, ids=IDS)
def test_device_duality(flight, shared):
    """|<lam, dy_dev> - <gx_dev, dX> - <gdisp_dev, dD>| <= 2 sum |lam| E + 2 sum |dX| Egx + 2 sum |dD| Egd for the 9 x 16 pairs of the
    kink vector, the inner products formed exactly: a branch transposed differently from how it was differentiated shows here"""
    name, mode, k = flight
    prob, E, X, disp, dX, dD, Lam = _case(name)
    g = kf.load(flight)
    b = kf.TRUTH_VEC
    if shared:
        plan = E.propagation_plan(steps=k, restart=mode)
        _Y, dY, rc = plan.tangent(X, dX=np.ascontiguousarray(dX[b]), dispersion=disp, ddispersion=np.ascontiguousarray(dD[b]), shared=True)
        _Y, GX, GD, rc2 = plan.adjoint(X, np.ascontiguousarray(Lam[b]), dispersion=disp, shared=True)
        plan.close()
        assert rc == 0 and rc2 == 0
        _Yp, dYp, GXp, GDp = _device(flight)
        assert same(dY[b], dYp[b]) and same(GX[b], GXp[b]) and same(GD[b], GDp[b])
    else:
        _Y, dY, GX, GD = _device(flight)
    lam = kf.functionals(prob, X[b])
    dy = tt.unpack_dy(dY[b], E.M)
    worst = 0.0
    for q in range(len(lam)):
        for d in range(len(kf.DIRECTIONS)):
            gap = abs(_exact_dot(lam[q], dy[d]) - _exact_dot(GX[b, q], dX[b, d]) - _exact_dot(GD[b, q], dD[b, d]))
            bound = 2 * float((np.abs(lam[q]) * g["bound"][d]).sum() + (np.abs(dX[b, d]) * g["Egx"][q]).sum() + (np.abs(dD[b, d]) * g["Egd"][q]).sum())
            worst = max(worst, float(gap / Fraction(bound)) if bound > 0 else (0.0 if gap == 0 else np.inf))
    print("%s %s k=%d, %s seeds: duality uses %.3g of its bound" % (flight + ("shared" if shared else "per-vector", worst)))
    assert worst <= 1.0, (flight, worst)


# ------------------------------------------------------------------ d. lanes on different branches in one wavefront
def _under_slabs(call):
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


@pytest.mark.parametrize("mode", ["section", "node"])
def test_mixed_lanes_tangent(mode):
    """B = 130 cycling the vector off every kink, the kink vector and the one off the axis: neighbouring lanes of a wavefront take
    different sides of every select.  Positions 0, 1, 63, 64, 65 and 129 give, bit for bit, their one-vector call (y, dy); the
    same in slabs of 64; direction p alone gives the bits it has among all 16."""
    prob, E, X, disp, dX, dD, _L = _case()
    idx = np.arange(B130) % 3
    plan = E.propagation_plan(steps=1, restart=mode)
    Xb, Db, dXb, dDb = (np.ascontiguousarray(a[idx]) for a in (X, disp, dX, dD))
    Y, dY = _under_slabs(lambda: plan.tangent(Xb, dX=dXb, dispersion=Db, ddispersion=dDb)[:2])
    one = [plan.tangent(X[v], dX=dX[[v]], dispersion=disp[[v]], ddispersion=dD[[v]]) for v in range(3)]
    assert all(o[2] == 0 for o in one)
    for pos in PICK:
        assert same(Y[pos], one[pos % 3][0][0]) and same(dY[pos], one[pos % 3][1][0]), pos
    assert not same(dY[0], dY[1]) and not same(dY[1], dY[2])
    for p in (1, 10, 14):
        _y, d1, rc = plan.tangent(X, dX=dX[:, [p]], dispersion=disp, ddispersion=dD[:, [p]])
        assert rc == 0 and same(d1[:, 0], dY[:3, p]), kf.DIRECTIONS[p]
    plan.close()


def test_mixed_lanes_adjoint():
    """the same batch through the section adjoint: positions 0, 1, 63, 64, 65, 129 give their one-vector call's y, gx, gdisp bit for
    bit, also in slabs of 64; functional q alone gives the bits it has among all 9"""
    prob, E, X, disp, _dX, _dD, Lam = _case()
    idx = np.arange(B130) % 3
    plan = E.propagation_plan(steps=1, restart="section")
    Xb, Db, Lb = (np.ascontiguousarray(a[idx]) for a in (X, disp, Lam))
    Y, GX, GD = _under_slabs(lambda: plan.adjoint(Xb, Lb, dispersion=Db)[:3])
    one = [plan.adjoint(X[v], Lam[[v]], dispersion=disp[[v]]) for v in range(3)]
    assert all(o[3] == 0 for o in one)
    for pos in PICK:
        v = pos % 3
        assert same(Y[pos], one[v][0][0]) and same(GX[pos], one[v][1][0]) and same(GD[pos], one[v][2][0]), pos
    assert not same(GX[0], GX[1]) and not same(GX[1], GX[2])
    for q in (2, 7, 8):
        _y, g1, d1, rc = plan.adjoint(X, Lam[:, [q]], dispersion=disp)
        assert rc == 0 and same(g1[:, 0], GX[:3, q]) and same(d1[:, 0], GD[:3, q]), kf.FUNCTIONALS[q]
    plan.close()


# ------------------------------------------------------------------ e. linearity at the kinks
@pytest.mark.parametrize("mode", ["section", "node"])
def test_linearity_tangent(mode):
    """a zero seed gives exact zeros; a seed times 2^-3 / 2^5 gives dy times 2^-3 / 2^5 bit for bit -- on the axis, at rest, below
    the polar radius and outside the tables as anywhere"""
    prob, E, X, disp, dX, dD, _L = _case()
    plan = E.propagation_plan(steps=1, restart=mode)
    _Y, dY, rc = plan.tangent(X, dX=dX, dispersion=disp, ddispersion=dD)
    _Y, d0, rc0 = plan.tangent(X, dX=np.zeros_like(dX), dispersion=disp, ddispersion=np.zeros_like(dD))
    assert rc == 0 and rc0 == 0 and not d0.any()
    for f in (2.0 ** -3, 2.0 ** 5):
        _Y, ds, rcs = plan.tangent(X, dX=dX * f, dispersion=disp, ddispersion=dD * f)
        assert rcs == 0 and same(ds, dY * f), f
    plan.close()


def test_linearity_adjoint():
    """lam = 0 gives exact zeros; lam times 2^-3 / 2^5 gives gx and gdisp times 2^-3 / 2^5 bit for bit"""
    prob, E, X, disp, _dX, _dD, Lam = _case()
    plan = E.propagation_plan(steps=1, restart="section")
    _Y, GX, GD, rc = plan.adjoint(X, Lam, dispersion=disp)
    _Y, g0, d0, rc0 = plan.adjoint(X, np.zeros_like(Lam), dispersion=disp)
    assert rc == 0 and rc0 == 0 and not g0.any() and not d0.any()
    for f in (2.0 ** -3, 2.0 ** 5):
        _Y, gs, ds, rcs = plan.adjoint(X, Lam * f, dispersion=disp)
        assert rcs == 0 and same(gs, GX * f) and same(ds, GD * f), f
    plan.close()


# ------------------------------------------------------------------ f. under a wind ensemble
def test_wind_ensemble_member_bits():
    """proptan_kernel<*, 1> and propadj_kernel<*, 1> at the kinks.  Two members of the handle's row count: its own rows, and a table
    lying wholly ABOVE every stage (its first row at 3e10 m: every lookup of that member has piece < 0 and takes the first row's
    wind, which is not calm).  The three vectors three times, the assignment -1, 0, 1 by block: every vector bit for bit what a
    handle created with its member's table returns (stated there on flights inside their tables)."""
    from test_wind_ensemble import member_engines
    from test_wind_ensemble_tangent import adjoint_checked, mismatches, tangent_checked
    prob, E, X, disp, dX, dD, Lam = _case()
    own = np.array(prob["wind_table"], dtype=np.float64)
    high = own.copy()
    high[:, 0] = 3.0e10 + 1.0e9 * np.arange(len(own))
    high[:, 1] = 20.0 - 3.0 * np.arange(len(own))
    high[:, 2] = -10.0 + 4.0 * np.arange(len(own))
    T = np.ascontiguousarray(np.stack([own, high]))
    # wholly above every stage: the geopotential altitude of the lookups of the three flown vectors, in both modes, from the fp64
    # value flight (the air stages off the axis; on it the altitude is the constant -N, 9.5e8 m of geopotential altitude)
    for mode in ("section", "node"):
        plan = E.propagation_plan(steps=1, restart=mode)
        for v in range(3):
            phases, Z = kf.fly_stages(E, plan, prob, X[v], disp[v], mode)
            c = kf.kink_census(prob, phases, Z, disp[v][:, 3])
            assert np.all(np.isfinite(Z)) and c["air"].any() and c["h"][c["air"]].max() < high[0, 0], (mode, v)
        plan.close()
    eng = member_engines(("kinks", 2), prob, T)
    idx = np.arange(9) % 3
    assignment = (np.arange(9) // 3 - 1).astype(np.int32)
    Xb, Db, dXb, dDb, Lb = (np.ascontiguousarray(a[idx]) for a in (X, disp, dX, dD, Lam))
    ens = E.wind_ensemble(T).assign(assignment)
    for mode in ("section", "node"):
        plan = E.propagation_plan(steps=1, restart=mode)
        plans = [e.propagation_plan(steps=1, restart=mode) for e in eng]
        calls = [("tangent", lambda e, p, n: tangent_checked(e, p, Xb, Db, dXb, dDb, False, n))]
        if mode == "section":
            calls.append(("adjoint", lambda e, p, n: adjoint_checked(e, p, Xb, Db, Lb, False, n)))
        for what, call in calls:
            got = call(E, plan, ens)
            mine = call(E, plan, None)
            refs = [call(e, p, None) for e, p in zip(eng, plans)]
            assert not mismatches(got, refs, mine, assignment), (mode, what)
            assert all(np.all(np.isfinite(a)) for a in got), (mode, what)
            assert all(same(a, c) for a, c in zip(refs[0], mine)) and not same(refs[1][-1], mine[-1]), (mode, what)
        for p in plans + [plan]:
            p.close()
    ens.close()

"""The wind-profile sensitivities of the flight on the device (gel_propagate_tangent_wind*, gel_propagate_adjoint_wind*; DESIGN.md
3.23), through the C ABI: dy and gwind against the 80-digit truth of tests/golden/g35_flight_wind.npz within its carried bounds
2 E / 2 Eg, duality and the scaling identity on the device within those bounds, the bit-exact properties (the parents' bits, slices,
2^k, +0.0 rows), the wind ensemble, and the Python layer.

Cases (tests/flight_wind_truth.py): batches of three with factors that differ per vector and phase; the truth holds vector 1 along
seven seeds on the table's values and for twelve functionals."""
import ctypes as C

import numpy as np
import pytest

import flight_adjoint_truth as at
import flight_tangent_truth as tt
import flight_wind_truth as wt

pytestmark = pytest.mark.gpu
IDS = lambda f: "%s-%s-k%d" % f   # noqa: E731
_dp = C.POINTER(C.c_double)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _d(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _c(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def tangent_raw(E, plan, X, disp, dX, dD, dW, shared, ens=None, form="host", status=0):
    """gel_propagate_tangent_wind[_device] itself -> (Y [B, 11 M], dY [B, P, 11 M]); form "device": torch buffers with a sentinel row
    behind each output"""
    from gelato_amd import _lib
    L = _lib.lib()
    X, disp, dX, dD, dW = (_c(a) for a in (X, disp, dX, dD, dW))
    B = X.shape[0]
    lead = dX if dX is not None else (dD if dD is not None else dW)
    P = lead.shape[0 if shared else 1]
    e = ens._p if ens is not None else None
    if form == "host":
        Y, dY = np.full((B, 11 * E.M), np.nan), np.full((B, P, 11 * E.M), np.nan)
        rc = _lib.check(L.gel_propagate_tangent_wind(plan._p, B, P, int(shared), _d(X), _d(disp), _d(dX), _d(dD), _d(dW), e, _d(Y), _d(dY)))
        assert rc == status
        return Y, dY
    import torch
    t = [None if a is None else torch.from_numpy(a).cuda() for a in (X, disp, dX, dD, dW)]
    p = [0 if a is None else a.data_ptr() for a in t]
    tY = torch.full((B + 1, 11 * E.M), -7.0, dtype=torch.float64, device="cuda")
    tdY = torch.full((B + 1, P, 11 * E.M), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    _lib.check(L.gel_propagate_tangent_wind_device(plan._p, B, P, int(shared), p[0], p[1] or None, p[2] or None, p[3] or None, p[4] or None, e,
                                                   tY.data_ptr(), tdY.data_ptr()))
    assert E.sync() == status
    Y, dY = tY.cpu().numpy(), tdY.cpu().numpy()
    assert np.all(Y[B] == -7.0) and np.all(dY[B] == -7.0), "wrote behind the batch"
    return Y[:B], dY[:B]


def adjoint_raw(E, plan, X, disp, Lam, shared, ens=None, form="host", wind=True, status=0, Kg=None):
    """gel_propagate_adjoint_wind[_device] itself -> (Y, GX [B, Q, nvars], GD [B, Q, S, 4], GW [B, Q, Kg, 2] | None)"""
    from gelato_amd import _lib
    L = _lib.lib()
    X, disp, Lam = (_c(a) for a in (X, disp, Lam))
    B = X.shape[0]
    Q = Lam.shape[0 if shared else 1]
    e = ens._p if ens is not None else None
    Kg = Kg or plan.wind_rows(ens)
    if form == "host":
        Y, GX, GD = np.full((B, 11 * E.M), np.nan), np.full((B, Q, E.nvars), np.nan), np.full((B, Q, E.S, 4), np.nan)
        GW = np.full((B, Q, Kg, 2), np.nan) if wind else None
        rc = _lib.check(L.gel_propagate_adjoint_wind(plan._p, B, Q, int(shared), _d(X), _d(disp), _d(Lam), e, _d(Y), _d(GX), _d(GD), _d(GW)))
        assert rc == status
        return Y, GX, GD, GW
    import torch
    t = [None if a is None else torch.from_numpy(a).cuda() for a in (X, disp, Lam)]
    p = [0 if a is None else a.data_ptr() for a in t]
    shapes = ((B + 1, 11 * E.M), (B + 1, Q, E.nvars), (B + 1, Q, E.S, 4), (B + 1, Q, Kg, 2))
    o = [torch.full(s, -7.0, dtype=torch.float64, device="cuda") for s in shapes]
    torch.cuda.synchronize()
    _lib.check(L.gel_propagate_adjoint_wind_device(plan._p, B, Q, int(shared), p[0], p[1] or None, p[2], e, o[0].data_ptr(), o[1].data_ptr(),
                                                   o[2].data_ptr(), o[3].data_ptr() if wind else None))
    assert E.sync() == status
    h = [a.cpu().numpy() for a in o]
    assert all(np.all(a[B] == -7.0) for a in h), "wrote behind the batch"
    return h[0][:B], h[1][:B], h[2][:B], (h[3][:B] if wind else None)


_CASE, _DEV = {}, {}


def _case(name):
    """(prob, engine, X [3, nvars], disp [3, S, 4]) of a case, shared by the tests"""
    if name not in _CASE:
        from gelato_amd import Engine
        prob, X, disp = tt.case(name)
        _CASE[name] = (prob, Engine(prob), X, disp)
    return _CASE[name]


def _seeds(flight):
    """the golden's seven seeds of a flight: (dW [7, Kw, 2], dX [7, nvars], dD [7, S, 4])"""
    prob, E, X, disp = _case(flight[0])
    _w, dX, dD = wt.seeds(prob, X[wt.TRUTH_VEC], None, not wt.on_kinks(flight))
    return wt.load(flight)["dW"], dX, dD


def _device(flight):
    """the device's results of a flight's batch of three, computed once: the seven seeds (shared) and, beside them as an eighth
    direction, the factor's own scaling direction ddisp[:, 3] = fw per vector; the twelve functionals (shared)"""
    if flight not in _DEV:
        prob, E, X, disp = _case(flight[0])
        dW, dX, dD = _seeds(flight)
        plan = E.propagation_plan(steps=flight[2], restart=flight[1])
        Y, dY = tangent_raw(E, plan, X, disp, dX, dD, dW, True)
        dDs = np.zeros((3, 1, E.S, 4))
        dDs[:, 0, :, 3] = disp[:, :, 3]
        _Y, dYs = tangent_raw(E, plan, X, disp, None, dDs, None, False)
        lam = at.pack_lam(wt.functionals(prob))
        Ya, GX, GD, GW = adjoint_raw(E, plan, X, disp, lam, True)
        plan.close()
        assert same(Ya, Y)
        _DEV[flight] = (Y, dY, dYs[:, 0], GW)
    return _DEV[flight]


# ------------------------------------------------------------------ 1. the truth
@pytest.mark.parametrize("flight", wt.FLIGHTS, ids=IDS)
def test_truth(flight):
    """dy within 2 E and gwind within 2 Eg of g35, for every seed and every functional"""
    prob, E, X, disp = _case(flight[0])
    g = wt.load(flight)
    Y, dY, _s, GW = _device(flight)
    b = wt.TRUTH_VEC
    got = tt.unpack_dy(dY[b], E.M)
    use_t = np.array([wt.miss(got[d], g["dy"][d], g["bound"][d]) for d in range(len(wt.SEEDS))])
    use_a = np.array([wt.miss(GW[b, q], g["gW"][q], g["Eg"][q]) for q in range(wt.NQ)])
    print("largest |error| / E per seed %s; / Eg per functional %s  (%s %s k=%d)"
          % ((np.array2string(use_t, precision=3), np.array2string(use_a, precision=3)) + flight))
    assert np.all(use_t <= 2.0), (flight, use_t)
    assert np.all(use_a <= 2.0), (flight, use_a)
    assert GW.shape[2] == np.asarray(prob["wind_table"]).shape[0]


@pytest.mark.parametrize("flight", wt.FLIGHTS, ids=IDS)
def test_device_duality_and_scaling_identity(flight):
    """|<lam, dy(dW)> - <gwind, dW>| <= sum |lam| 2 E + sum 2 Eg |dW| for the pure wind seeds; the "scale" seed's dy against the dy of
    ddisp[:, 3] = fw within the two directions' bounds"""
    prob, E, X, disp = _case(flight[0])
    g = wt.load(flight)
    Y, dY, dYs, GW = _device(flight)
    b = wt.TRUTH_VEC
    lam = wt.functionals(prob)
    dy = tt.unpack_dy(dY[b], E.M)
    for q in range(wt.NQ):
        for d in range(6):
            lhs, rhs = (lam[q] * dy[d]).sum(), (GW[b, q] * g["dW"][d]).sum()
            tol = (np.abs(lam[q]) * 2 * g["bound"][d]).sum() + (2 * g["Eg"][q] * np.abs(g["dW"][d])).sum()
            assert abs(lhs - rhs) <= tol, (flight, q, wt.SEEDS[d], lhs, rhs, tol)
    sc = wt.SEEDS.index("scale")
    assert np.abs(g["dy"][sc]).max() > 0
    diff = np.abs(dy[sc] - tt.unpack_dy(dYs[b], E.M))
    assert np.all(diff <= 2 * g["bound"][sc] + 2 * g["bound_fw"]), (flight, float((diff - 2 * g["bound"][sc] - 2 * g["bound_fw"]).max()))


def test_bound_rejects_wrong_restatements_around_the_device():
    """the same bounds, around the DEVICE's dy and gwind, reject the wrong restatements evaluated from the stored per-stage partials
    (first flight; ends_dropped is judged on the ENDS flight: without its end rows the device's end-row results would be zero)"""
    import interp_truth as it
    flight = wt.FLIGHTS[0]
    prob, E, X, disp = _case(flight[0])
    g, g30 = wt.load(flight), tt.load(flight)
    st = {k: g30[k] for k in ("F", "J", "Pu", "Pf")}
    st.update({k: g[k] for k in ("Pw", "piece", "th", "air")})
    mats, hs = tt.plan_tables(it.engine(prob), flight[2], flight[1])
    Y, dY, _s, GW = _device(flight)
    b = wt.TRUTH_VEC
    dy = tt.unpack_dy(dY[b], E.M)
    fws, Kw = g["disp"][:, 3], g["dW"].shape[1]
    lam = wt.functionals(prob)
    for mut in ("shift_piece", "no_fw", "theta_swapped"):
        wt_ = max(wt.miss(wt.tangent(prob, flight[1], flight[2], g["x"], mats, hs, st, fws, np.zeros_like(g["x"]), np.zeros((E.S, 4)), g["dW"][d],
                                     mutate=mut), dy[d], 2 * g["bound"][d]) for d in (0, 1, 2, 5))
        wa = max(wt.miss(wt.adjoint(prob, flight[1], flight[2], g["x"], hs, st, fws, lam[q], Kw, mutate=mut), GW[b, q], 2 * g["Eg"][q])
                 for q in (4, 5, 6, 11))
        print("mutation %s: misses 2 E around the device's dy by a factor %.3g, 2 Eg around its gwind by %.3g" % (mut, wt_, wa))
        assert wt_ > 1.0e3 and wa > 1.0e3, (mut, wt_, wa)
    ends = wt.FLIGHTS[3]
    e = wt.load(ends)
    _Y, dYe, _s, GWe = _device(ends)
    dye = tt.unpack_dy(dYe[b], _case(ends[0])[1].M)
    for d, row in ((3, 0), (4, -1)):
        assert np.any(np.abs(dye[d]) > 1.0e3 * 2 * e["bound"][d]) and np.any(np.abs(GWe[b, :, row]) > 1.0e3 * 2 * e["Eg"][:, row])


# ------------------------------------------------------------------ 2. the parents' bits
@pytest.mark.parametrize("flight", [wt.FLIGHTS[1], wt.FLIGHTS[3]], ids=IDS)
def test_parent_bits(flight):
    """dwind / gwind NULL: y, dy, gx, gdisp are the parent calls' bits; gwind wanted: y, gx, gdisp still are; dwind given and zero:
    dy is the parent's"""
    prob, E, X, disp = _case(flight[0])
    dW, dX, dD = _seeds(flight)
    lam = at.pack_lam(wt.functionals(prob))
    plan = E.propagation_plan(steps=flight[2], restart=flight[1])
    Y0, dY0, rc = plan.tangent(X, dX=dX, dispersion=disp, ddispersion=dD, shared=True)
    Ya0, GX0, GD0, rca = plan.adjoint(X, lam, dispersion=disp, shared=True)
    assert rc == 0 and rca == 0
    for form in ("host", "device"):
        Y, dY = tangent_raw(E, plan, X, disp, dX, dD, None, True, form=form)
        assert same(Y, Y0) and same(dY, dY0), form
        Y, dY = tangent_raw(E, plan, X, disp, dX, dD, np.zeros_like(dW), True, form=form)
        assert same(Y, Y0) and same(dY, dY0), form
        Y, GX, GD, GW = adjoint_raw(E, plan, X, disp, lam, True, form=form, wind=False)
        assert GW is None and same(Y, Ya0) and same(GX, GX0) and same(GD, GD0), form
        Y, GX, GD, GW = adjoint_raw(E, plan, X, disp, lam, True, form=form, wind=True)
        assert same(Y, Ya0) and same(GX, GX0) and same(GD, GD0) and np.all(np.isfinite(GW)) and np.any(GW != 0), form
    # the wind seed beside the others is their sum with it alone, within rounding of the sum: it is ONE forcing term more
    _Y, dYw = tangent_raw(E, plan, X, disp, None, None, dW, True)
    _Y, dYall = tangent_raw(E, plan, X, disp, dX, dD, dW, True)
    assert np.any(dYw != 0) and not same(dYall, dY0)
    assert np.abs(dYall - (dY0 + dYw)).max() <= 1e-9 * np.abs(dYall).max()
    plan.close()


# ------------------------------------------------------------------ 3. slices, scaling, zeros
@pytest.mark.parametrize("mode", ["chain", "section"])
def test_slices_forms_slabs_scaling(mode, monkeypatch):
    """a slice's bits depend neither on B, P / Q, its place in the batch, shared, the form of the call nor the slab size; a seed or lam
    times 2^k gives the outputs times 2^k; zero gives zeros"""
    flight = ("example", mode, 2 if mode == "section" else 1)
    prob, E, X, disp = _case("example")
    dW7, dX7, dD7 = _seeds(wt.FLIGHTS[0])
    sel = [6, 0, 5]
    dW, dX, dD = dW7[sel], dX7[sel], dD7[sel]
    lam = at.pack_lam(wt.functionals(prob))[[11, 4, 0]]
    plan = E.propagation_plan(steps=flight[2], restart=mode)
    Y, dY = tangent_raw(E, plan, X, disp, dX, dD, dW, True)
    _Y, GX, GD, GW = adjoint_raw(E, plan, X, disp, lam, True)
    # P, Q = 1; per-vector copies of the shared seeds; the device form
    for i in range(3):
        _y, d1 = tangent_raw(E, plan, X, disp, dX[[i]], dD[[i]], dW[[i]], True)
        _y, gx1, gd1, gw1 = adjoint_raw(E, plan, X, disp, lam[[i]], True)
        assert same(d1[:, 0], dY[:, i]) and same(gw1[:, 0], GW[:, i]) and same(gx1[:, 0], GX[:, i]), i
    bc = lambda a: np.broadcast_to(a, (3,) + a.shape)   # noqa: E731
    Yc, dYc = tangent_raw(E, plan, X, disp, bc(dX), bc(dD), bc(dW), False, form="device")
    _Yc, GXc, GDc, GWc = adjoint_raw(E, plan, X, disp, bc(lam), False, form="device")
    assert same(Yc, Y) and same(dYc, dY) and same(GXc, GX) and same(GDc, GD) and same(GWc, GW)
    # 67 vectors, cyclic and reversed, in one slab and in two
    idx = (np.arange(67) % 3)[::-1]
    res = []
    for slab in (None, "64"):
        if slab:
            monkeypatch.setenv("GEL_PROP_SLAB", slab)
        assert plan.adjoint_info(67, 3, shared=True, want_wind=True)["slabs"] == (2 if slab else 1)
        res.append(tangent_raw(E, plan, X[idx], disp[idx], dX, dD, dW, True, form="device" if slab else "host")
                   + adjoint_raw(E, plan, X[idx], disp[idx], lam, True, form="device" if slab else "host"))
        if slab:
            monkeypatch.delenv("GEL_PROP_SLAB")
    for r in res:
        assert same(r[1], dY[idx]) and same(r[3], GX[idx]) and same(r[4], GD[idx]) and same(r[5], GW[idx])
    # 2^k and zero
    for sc in (2.0 ** -3, 2.0 ** 7):
        _y, dYs = tangent_raw(E, plan, X, disp, dX * sc, dD * sc, dW * sc, True)
        _y, _gx, _gd, GWs = adjoint_raw(E, plan, X, disp, lam * sc, True)
        assert same(dYs, dY * sc) and same(GWs, GW * sc), sc
    _y, dYz = tangent_raw(E, plan, X, disp, None, None, np.zeros_like(dW), True)
    _y, _gx, _gd, GWz = adjoint_raw(E, plan, X, disp, np.zeros_like(lam), True)
    assert np.all(_bits(dYz) << 1 == 0) and np.all(GWz == 0.0)
    plan.close()


def test_untouched_rows_and_airless_problem():
    """rows no stage touches are +0.0: the example never reads row 0 (g35: its row_first seed moves nothing); a problem whose
    phases are all air-less gives an all-zero gwind and a zero dy for every wind seed"""
    g = wt.load(wt.FLIGHTS[0])
    assert np.all(g["dy"][wt.SEEDS.index("row_first")] == 0.0) and np.all(g["gW"][:, 0] == 0.0)
    _Y, dY, _s, GW = _device(wt.FLIGHTS[0])
    assert np.all(_bits(GW[:, :, 0]) == 0) and np.all(dY[:, wt.SEEDS.index("row_first")] == 0.0)
    feels = [1, 2, 3, 4, 5, 6, 11]         # (the terminal mass and attitude do not depend on the wind: their rows are +0.0 too)
    assert np.all(GW[:, feels, 1:3].reshape(3, len(feels), -1).any(axis=2)) and np.all(_bits(GW[:, [0, 7, 8, 9, 10]]) == 0)
    prob, E, X, disp = _case("noair")
    Kw = np.asarray(prob["wind_table"]).shape[0]
    lam = at.pack_lam(wt.functionals(prob))
    for mode in ("chain", "section"):
        plan = E.propagation_plan(steps=2, restart=mode)
        _Y, GX, _gd, GW = adjoint_raw(E, plan, X, disp, lam, True)
        assert np.all(_bits(GW) == 0) and np.any(GX != 0)
        _Y, dY = tangent_raw(E, plan, X, disp, None, None, np.random.default_rng(1).standard_normal((2, Kw, 2)), True)
        assert np.all(dY == 0.0)
        plan.close()


# ------------------------------------------------------------------ 4. the wind ensemble
def _ensemble_case(K, B=12):
    from test_wind_ensemble import CYCLE, SEEDS, example, member_engines
    from test_wind_ensemble_cpu import members
    from test_flight import dispersion
    prob, E, X67, _pd, _ud = example()
    T = members(K, SEEDS, calm_of=1)
    return prob, E, np.ascontiguousarray(X67[:B]), dispersion(67, E.S)[:B], T, member_engines(("example", K), prob, T), CYCLE[:B].copy()


@pytest.mark.parametrize("mode", ["chain", "section"])
@pytest.mark.parametrize("K", [2, 33])
def test_ensemble_member_bits(K, mode):
    """a vector with member e gets bit for bit the call on a handle created with wind_table = tables[e], -1 the call on the handle
    itself; rows at or beyond the lane's own Kw are +0.0 (K = 33 > 9: the -1 lanes; K = 2 < 9: the members' lanes) and are not read
    from the seed; the neighbours' assignment changes nothing"""
    prob, E, X, D, T, eng, cyc = _ensemble_case(K)
    B, Kown = X.shape[0], E.wind_altitudes.size
    Kg = max(K, Kown)
    rng = np.random.default_rng(K)
    dW = rng.standard_normal((2, Kg, 2))
    lam = at.pack_lam(wt.functionals(prob))[[11, 5]]
    ens = E.wind_ensemble(T).assign(cyc)
    plan = E.propagation_plan(steps=1, restart=mode)
    assert plan.wind_rows(ens) == Kg
    Y, dY = tangent_raw(E, plan, X, D, None, None, dW, True, ens, form="device")
    Ya, GX, GD, GW = adjoint_raw(E, plan, X, D, lam, True, ens, form="device")
    own_t = tangent_raw(E, plan, X, D, None, None, dW[:, :Kown], True)
    own_a = adjoint_raw(E, plan, X, D, lam, True)
    for b in range(B):
        m = int(cyc[b])
        if m < 0:
            rt, ra, Kl = own_t, own_a, Kown
        else:
            p = eng[m].propagation_plan(steps=1, restart=mode)
            rt = tangent_raw(eng[m], p, X, D, None, None, dW[:, :K], True)
            ra = adjoint_raw(eng[m], p, X, D, lam, True)
            p.close()
            Kl = K
        assert same(Y[b], rt[0][b]) and same(dY[b], rt[1][b]), (K, mode, b, m)
        assert same(GX[b], ra[1][b]) and same(GD[b], ra[2][b]) and same(GW[b, :, :Kl], ra[3][b]), (K, mode, b, m)
        assert np.all(_bits(GW[b, :, Kl:]) == 0), (K, mode, b, m)
    assert np.any(dY != 0) and np.any(GW != 0)
    # seed rows at or beyond the lane's Kw are not read: NaN there changes nothing
    Kmin = min(K, Kown)
    dWn = dW.copy()
    dWn[:, Kmin:] = np.nan
    small = (cyc < 0) if Kown < K else (cyc >= 0)
    _Y, dYn = tangent_raw(E, plan, X, D, None, None, dWn, True, ens, form="device", status=1 if not small.all() else 0)
    assert same(dYn[small], dY[small])
    # the neighbours: every other vector re-assigned
    b0 = 3
    other = np.roll(cyc, 2)
    other[b0] = cyc[b0]
    ens.assign(other)
    _Y, dYo = tangent_raw(E, plan, X, D, None, None, dW, True, ens)
    _Y, _gx, _gd, GWo = adjoint_raw(E, plan, X, D, lam, True, ens)
    assert same(dYo[b0], dY[b0]) and same(GWo[b0], GW[b0])
    plan.close()
    ens.close()


def test_ensemble_member_longer_than_any_handle_accepts():
    """Kw = 400 (a handle refuses it), B = 3: y and the parents' outputs are the ensemble calls' bits, gwind is finite, zero beyond no
    row a lane owns, the 2^k scaling holds in bits, and the device's own duality holds.  No handle exists to compare with; the
    tolerance is the per-stage contract of these tangents (1e-9 relative) on the sum of the terms' magnitudes, both
    sides summing the same per-stage products in another order, with a factor 10 for the knots and the steps between them"""
    from test_wind_ensemble import example
    from test_wind_ensemble_cpu import members
    prob, E, X67, _pd, _ud = example()
    X = np.ascontiguousarray(X67[:3])
    T = members(400, (15, 16, 17))
    ens = E.wind_ensemble(T).assign([0, 1, 2])
    plan = E.propagation_plan(steps=1, restart="chain")
    assert plan.wind_rows(ens) == 400
    lamM = wt.functionals(prob)[[11, 6]]
    lam = at.pack_lam(lamM)
    dW = np.random.default_rng(400).standard_normal((2, 400, 2))
    Y, dY = tangent_raw(E, plan, X, None, None, None, dW, True, ens)
    Ya, GX, GD, GW = adjoint_raw(E, plan, X, None, lam, True, ens)
    Yp, GXp, GDp, rc = plan.adjoint(X, lam, shared=True, ensemble=ens)
    assert same(Y, Yp) and same(Ya, Yp) and same(GX, GXp) and same(GD, GDp)
    assert np.all(np.isfinite(dY)) and np.all(np.isfinite(GW)) and np.any(GW != 0)
    dy = tt.unpack_dy(dY, E.M)
    for b in range(3):
        for q in range(2):
            for d in range(2):
                lhs, rhs = (lamM[q] * dy[b, d]).sum(), (GW[b, q] * dW[d]).sum()
                mag = np.abs(lamM[q] * dy[b, d]).sum() + np.abs(GW[b, q] * dW[d]).sum()
                assert abs(lhs - rhs) <= 1e-8 * mag, (b, q, d, lhs, rhs)
    _Y, dY7 = tangent_raw(E, plan, X, None, None, None, dW * 128.0, True, ens)
    _Y, _gx, _gd, GW7 = adjoint_raw(E, plan, X, None, lam * 128.0, True, ens)
    assert same(dY7, dY * 128.0) and same(GW7, GW * 128.0)
    plan.close()
    ens.close()


def test_status_nonfinite_gwind():
    """a non-finite gwind entry raises the handle's status like gx: lam = inf on one vector's functional"""
    from gelato_amd import _lib
    prob, E, X, disp = _case("example")
    lam = np.broadcast_to(at.pack_lam(wt.functionals(prob))[[6]], (3, 1, 11 * E.M)).copy()
    lam[2] = np.where(lam[2] != 0.0, np.inf, 0.0)
    plan = E.propagation_plan(steps=1, restart="chain")
    _Y, GX, _gd, GW = adjoint_raw(E, plan, X, disp, lam, False, status=_lib.GEL_NONFINITE)
    assert np.all(np.isfinite(GW[:2])) and not np.all(np.isfinite(GW[2]))
    _Y, _gx, _gd, GW2 = adjoint_raw(E, plan, X[:2], disp[:2], lam[:2], False)       # the next call is clean (status 0 inside)
    assert same(GW2, GW[:2])
    plan.close()


# ------------------------------------------------------------------ 5. the Python layer
def test_python_layer_against_the_raw_calls():
    from gelato_amd import propagate
    from test_wind_ensemble import example
    from test_wind_ensemble_cpu import members
    prob, E, X67, pdict, unitdict = example()
    X = np.ascontiguousarray(X67[:3])
    # PropagationPlan.tangent / adjoint
    plan = E.propagation_plan(steps=2, restart="chain")
    Kw = E.wind_altitudes.size
    dW = np.random.default_rng(5).standard_normal((3, 2, Kw, 2))
    lam = np.broadcast_to(at.pack_lam(wt.functionals(prob))[[0, 11]], (3, 2, 11 * E.M))
    Y, dY, rc = plan.tangent(X, dwind=dW)
    Yr, dYr = tangent_raw(E, plan, X, None, None, None, dW, False)
    assert rc == 0 and same(Y, Yr) and same(dY, dYr)
    Y, GX, GD, rc, GW = plan.adjoint(X, lam, want_wind=True)
    Yr, GXr, GDr, GWr = adjoint_raw(E, plan, X, None, lam, False)
    assert rc == 0 and same(GW, GWr) and same(GX, GXr) and same(GD, GDr)
    four = plan.adjoint(X, lam)
    assert len(four) == 4 and same(four[1], GX)
    # flight_gradient(wind=True): steps = 1 is a plan of 2 steps per node interval; scaled like gx
    out = propagate.flight_gradient(X, pdict, unitdict, steps=1, engine=E, wind=True)
    ref = propagate.flight_gradient(X, pdict, unitdict, steps=1, engine=E)
    assert set(out) == set(ref) | {"gwind", "wind_altitudes"} and all(same(np.asarray(out[k], dtype=float), np.asarray(ref[k], dtype=float))
                                                                      for k in ("gx", "gdisp", "y", "jacobian"))
    M = E.M
    lam11 = np.zeros((11, 11 * M))
    lam11[np.arange(11), [tt.sidx(M, M - 1, c) for c in range(11)]] = 1.0
    _Y, _gx, _gd, GWt = adjoint_raw(E, plan, X, None, lam11, True)
    u = E.units
    scale = np.array([u[0]] + [u[1]] * 3 + [u[2]] * 3 + [1.0] * 4)
    assert same(out["gwind"], GWt * scale[None, :, None, None]) and np.array_equal(out["wind_altitudes"], np.asarray(prob["wind_table"])[:, 0])
    # under an ensemble: per vector the altitudes of its member
    T = members(33, (1, 2))
    ens = E.wind_ensemble(T).assign([1, -1, 0])
    oe = propagate.flight_gradient(X, pdict, unitdict, steps=1, engine=E, ensemble=ens, wind=True)
    assert oe["gwind"].shape == (3, 11, 33, 2) and oe["wind_altitudes"].shape == (3, 33)
    assert np.array_equal(oe["wind_altitudes"][0], T[1, :, 0]) and np.array_equal(oe["wind_altitudes"][2], T[0, :, 0])
    assert np.array_equal(oe["wind_altitudes"][1, :Kw], out["wind_altitudes"]) and np.all(np.isnan(oe["wind_altitudes"][1, Kw:]))
    assert same(oe["gwind"][1, :, :Kw], out["gwind"][1]) and np.all(_bits(oe["gwind"][1, :, Kw:]) == 0)
    ens.close()
    plan.close()


def test_linear_prediction_against_flying_the_member():
    """wind_linear_prediction against flying a table that differs from the base by 1e-3 of its values.  The acceptance bound is the
    second-order remainder, estimated from the same comparison at 2e-3: the remainder is quadratic in the step, so a quarter of the
    2e-3 miss, with a factor 2 of margin -- not a fixed number"""
    from gelato_amd import Engine, montecarlo as mc, propagate
    from test_wind_ensemble import example
    prob, E, X67, pdict, unitdict = example()
    X = np.ascontiguousarray(X67[:3])
    base = np.asarray(prob["wind_table"], dtype=np.float64)
    out = propagate.flight_gradient(X, pdict, unitdict, steps=1, engine=E, wind=True)
    M = E.M
    idx = np.array([tt.sidx(M, M - 1, c) for c in range(11)])
    u = E.units
    scale = np.array([u[0]] + [u[1]] * 3 + [u[2]] * 3 + [1.0] * 4)
    y0 = out["y"][:, idx] * scale
    tables = np.stack([np.column_stack([base[:, 0], base[:, 1:] * (1.0 + eps)]) for eps in (1e-3, 2e-3)])
    pred = mc.wind_linear_prediction(out["gwind"], base, tables)            # [2, B, 11]
    miss = []
    for e in range(2):
        Em = Engine(dict(prob, wind_table=tables[e]))
        plan = Em.propagation_plan(steps=2, restart="chain")
        Ym, _err, rc = plan.apply(X, want_err=False)
        plan.close()
        Em.close()
        assert rc == 0
        miss.append(np.abs((Ym[:, idx] * scale - y0) - pred[e]))
    moved = np.abs(pred[0])
    assert np.any(moved[:, 1:7] > 0)
    # (the floor: y's own rounding in the difference of two flights, 64 ulp of the terminal value)
    floor = 64 * 2.0 ** -53 * np.abs(y0)
    print("linear prediction at 1e-3: largest miss / |change| %.3g; at 2e-3 %.3g" % (float((miss[0] / np.maximum(moved, 1e-300))[moved > 0].max()),
                                                                                  float((miss[1] / np.maximum(2 * moved, 1e-300))[moved > 0].max())))
    assert np.all(miss[0] <= 2 * (miss[1] / 4) + floor), float((miss[0] - 2 * (miss[1] / 4) - floor).max())
    assert np.all(miss[0] <= 1e-2 * moved + floor)                          # and the prediction is first order: the miss is small beside it

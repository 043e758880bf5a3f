"""The tangent and the adjoint flight under a wind ensemble on the device (gel_propagate_tangent_ensemble*,
gel_propagate_adjoint_ensemble*).

The truth is the existing single-table path, which tests/test_flight_tangent.py and tests/test_flight_adjoint.py pin to their
60-digit fixtures: a vector assigned member e must have, BIT FOR BIT, the y, dy, gx and gdisp that gel_propagate_tangent* /
gel_propagate_adjoint* return for the same x, factors and seeds / lam on an engine created with wind_table = tables[e], and a vector
assigned -1 what those calls return on the engine itself.  No comparison here carries a tolerance.

The example and its 67 vectors, the members (four tables of table_cases._wind_table and a calm one) and the assignment that cycles
-1, 0, 1, 2, 3, 4 -- every wavefront mixes all six tables -- are tests/test_wind_ensemble.py's; steps = 1.  Every call whose result is
compared is a device-form call with one sentinel row behind each output."""
import numpy as np
import pytest

import flight_tangent_truth as tt
from test_flight import _bits, dispersion
from test_wind_ensemble import B67, CYCLE, SEEDS, assigned_rows, example, fly_checked, member_engines
from test_wind_ensemble_cpu import members

pytestmark = pytest.mark.gpu
SENTINEL = -7.0
SHARED3 = [tt.DIRECTIONS.index(n) for n in ("position0_y", "knot_time", "wind_all")]   # a lift-off state, a knot time, the wind factor of every phase
PERVEC3 = [tt.DIRECTIONS.index(n) for n in ("position0_y", "mass_after_drop", "dense")]


def same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def shared_seeds(prob, x):
    """(dX [3, nvars], dD [3, S, 4]): three of flight_tangent_truth.directions' seeds, one set for every vector"""
    dX, dD = tt.directions(prob, x)
    assert np.all(dD[SHARED3[2], :, 3] != 0.0) and np.any(dX[SHARED3[0]] != 0.0) and np.any(dX[SHARED3[1]] != 0.0)
    return np.ascontiguousarray(dX[SHARED3]), np.ascontiguousarray(dD[SHARED3])


def per_vector_seeds(prob, X):
    """(dX [B, 3, nvars], dD [B, 3, S, 4]): every vector's own seeds (its own mass drop; the dense seed scaled by the vector)"""
    s = [tt.directions(prob, x) for x in X]
    dX, dD = np.stack([a[PERVEC3] for a, _d in s]), np.stack([d[PERVEC3] for _a, d in s])
    sc = 1.0 + np.arange(len(X)) / 64.0
    dX[:, 2] *= sc[:, None]
    dD[:, 2] *= sc[:, None, None]
    return np.ascontiguousarray(dX), np.ascontiguousarray(dD)


def functionals(E, x):
    """Lam [2, 11 M]: the terminal vz, and the velocity row of the first node between 5 and 10 km above the first (the windy band)"""
    M = E.M
    r = np.stack([x[M + 3 * i:M + 3 * i + 3] for i in range(M)]) * E.units[1]
    alt = np.linalg.norm(r, axis=1) - np.linalg.norm(r[0])
    inside = np.nonzero((alt > 5000.0) & (alt < 10000.0))[0]
    assert inside.size and 0 < inside[0] < M - 1, alt
    lam = np.zeros((2, 11 * M))
    lam[0, tt.sidx(M, M - 1, 6)] = 1.0
    lam[1, [tt.sidx(M, int(inside[0]), c) for c in (4, 5, 6)]] = 1.0
    return lam


def _cuda(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _ptr(t):
    return t.data_ptr() if t is not None else 0


def tangent_checked(E, plan, X, D, dX, dD, shared, ens=None, status=0, raw=False):
    """the tangent on device buffers -> (Y [B, 11 M], dY [B, P, 11 M]); the row behind each output is untouched.  raw: through the
    parent entry point gel_propagate_tangent_device itself"""
    import torch
    from gelato_amd import _lib
    B = X.shape[0]
    P = (dX if dX is not None else dD).shape[0 if shared else 1]
    t = [_cuda(a) for a in (X, D, dX, dD)]
    dY = torch.full((B + 1, 11 * E.M), SENTINEL, dtype=torch.float64, device="cuda")
    ddY = torch.full((B + 1, P, 11 * E.M), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    if raw:
        assert ens is None
        _lib.check(_lib.lib().gel_propagate_tangent_device(plan._p, B, P, int(shared), _ptr(t[0]), _ptr(t[1]) or None, _ptr(t[2]) or None,
                                                           _ptr(t[3]) or None, _ptr(dY), _ptr(ddY)))
    else:
        plan.tangent_device(B, P, _ptr(t[0]), _ptr(dY), _ptr(ddY), d_dx=_ptr(t[2]), d_dispersion=_ptr(t[1]), d_ddispersion=_ptr(t[3]),
                            shared=shared, ensemble=ens)
    assert E.sync() == status
    Y, dYh = dY.cpu().numpy(), ddY.cpu().numpy()
    assert np.all(Y[B] == SENTINEL) and np.all(dYh[B] == SENTINEL), "wrote behind the batch"
    return Y[:B], dYh[:B]


def adjoint_checked(E, plan, X, D, Lam, shared, ens=None, status=0, raw=False):
    """the adjoint flight on device buffers -> (Y [B, 11 M], GX [B, Q, nvars], GD [B, Q, S, 4]); the rows behind the outputs untouched"""
    import torch
    from gelato_amd import _lib
    B = X.shape[0]
    Q = Lam.shape[0 if shared else 1]
    t = [_cuda(a) for a in (X, D, Lam)]
    dY = torch.full((B + 1, 11 * E.M), SENTINEL, dtype=torch.float64, device="cuda")
    dG = torch.full((B + 1, Q, E.nvars), SENTINEL, dtype=torch.float64, device="cuda")
    dF = torch.full((B + 1, Q, E.S, 4), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    if raw:
        assert ens is None
        _lib.check(_lib.lib().gel_propagate_adjoint_device(plan._p, B, Q, int(shared), _ptr(t[0]), _ptr(t[1]) or None, _ptr(t[2]), _ptr(dY),
                                                           _ptr(dG), _ptr(dF)))
    else:
        plan.adjoint_device(B, Q, _ptr(t[0]), _ptr(t[2]), _ptr(dY), _ptr(dG), d_gdisp=_ptr(dF), d_dispersion=_ptr(t[1]), shared=shared,
                            ensemble=ens)
    assert E.sync() == status
    Y, G, F = dY.cpu().numpy(), dG.cpu().numpy(), dF.cpu().numpy()
    assert np.all(Y[B] == SENTINEL) and np.all(G[B] == SENTINEL) and np.all(F[B] == SENTINEL), "wrote behind the batch"
    return Y[:B], G[:B], F[:B]


def per_member(eng, mode, call):
    """call(engine, plan) on every member's engine with a plan of its own"""
    out = []
    for e in eng:
        p = e.propagation_plan(steps=1, restart=mode)
        out.append(call(e, p))
        p.close()
    return out


def mismatches(got, refs, own, assignment):
    """the vectors of which any output differs in a bit from the engine they are assigned to; got, own, refs[e]: tuples of arrays"""
    want = [assigned_rows([r[i] for r in refs], own[i], assignment) for i in range(len(got))]
    return [b for b in range(len(assignment)) if not all(same(g[b], w[b]) for g, w in zip(got, want))]


# ------------------------------------------------------------------ 1. tangent, chain
@pytest.mark.parametrize("dispersed", [False, True])
@pytest.mark.parametrize("K", [2, 33, 160])
def test_tangent_member_bits_chain(K, dispersed):
    """proptan_kernel<true, 1>: one interval, the count and the bisection on either side of lower_count's switch, the 9-row handle
    beside them; P = 3 shared seeds"""
    prob, E, X, _pd, _ud = example()
    T = members(K, SEEDS, calm_of=1)
    eng = member_engines(("example", K), prob, T)
    D = dispersion(B67, E.S) if dispersed else None
    dX, dD = shared_seeds(prob, X[0])
    ens = E.wind_ensemble(T).assign(CYCLE)
    plan = E.propagation_plan(steps=1, restart="chain")
    got = tangent_checked(E, plan, X, D, dX, dD, True, ens)
    own = tangent_checked(E, plan, X, D, dX, dD, True)
    refs = per_member(eng, "chain", lambda e, p: tangent_checked(e, p, X, D, dX, dD, True))
    bad = mismatches(got, refs, own, CYCLE)
    assert not bad, (K, dispersed, bad[:10], CYCLE[bad[:10]])
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1]))
    moved = np.abs(got[1]).max(axis=2) > 0                                    # [B, P]: the direction moves the flight
    assert np.all(moved[:, :2]) and np.all(moved[CYCLE != 4, 2]), moved       # (the wind factor's direction is zero under the calm member)
    Yv, _err = fly_checked(E, plan, X, D, ens)
    assert same(got[0], Yv)                                                   # y is gel_propagate_ensemble's
    # the wind is felt in the derivative: the same vector under two different tables differs in its bits (wind factor 0 excepted)
    for b in range(B67):
        felt = D is None or np.any(D[b, :, 3] != 0.0)
        others = [own[1][b]] + [r[1][b] for r in refs]
        mine = int(CYCLE[b]) + 1
        differ = [j for j, o in enumerate(others) if j != mine and not same(o, got[1][b])]
        if felt:
            assert len(differ) >= 4, (K, b, differ)                          # (the calm member and a table the flight never enters may coincide)
    plan.close()
    ens.close()


# ------------------------------------------------------------------ 2. tangent, section and node mode
@pytest.mark.parametrize("mode", ["section", "node"])
def test_tangent_member_bits_section_and_node(mode):
    """proptan_kernel<false, 1>, K = 33, per-vector seeds (shared = 0): a lane's vector is lane / P in every segment's workgroups"""
    prob, E, X, _pd, _ud = example()
    T = members(33, SEEDS, calm_of=1)
    eng = member_engines(("example", 33), prob, T)
    dX, dD = per_vector_seeds(prob, X)
    ens = E.wind_ensemble(T).assign(CYCLE)
    plan = E.propagation_plan(steps=1, restart=mode)
    for D in (None, dispersion(B67, E.S)):
        got = tangent_checked(E, plan, X, D, dX, dD, False, ens)
        own = tangent_checked(E, plan, X, D, dX, dD, False)
        refs = per_member(eng, mode, lambda e, p: tangent_checked(e, p, X, D, dX, dD, False))
        bad = mismatches(got, refs, own, CYCLE)
        assert not bad, (mode, D is not None, bad[:10], CYCLE[bad[:10]])
        assert np.all(np.isfinite(got[1])) and not same(refs[0][1], refs[2][1])
        Yv, _err = fly_checked(E, plan, X, D, ens)
        assert same(got[0], Yv)
    plan.close()
    ens.close()


# ------------------------------------------------------------------ 3. adjoint, chain and section
@pytest.mark.parametrize("mode", ["chain", "section"])
@pytest.mark.parametrize("K", [33, 160])
def test_adjoint_member_bits(K, mode):
    """propadj_kernel<*, 1> behind prop_kernel<true, *, 1>: dispersed, Q = 2 shared functionals"""
    prob, E, X, _pd, _ud = example()
    T = members(K, SEEDS, calm_of=1)
    eng = member_engines(("example", K), prob, T)
    D = dispersion(B67, E.S)
    Lam = functionals(E, X[0])
    ens = E.wind_ensemble(T).assign(CYCLE)
    plan = E.propagation_plan(steps=1, restart=mode)
    got = adjoint_checked(E, plan, X, D, Lam, True, ens)
    own = adjoint_checked(E, plan, X, D, Lam, True)
    refs = per_member(eng, mode, lambda e, p: adjoint_checked(e, p, X, D, Lam, True))
    bad = mismatches(got, refs, own, CYCLE)
    assert not bad, (K, mode, bad[:10], CYCLE[bad[:10]])
    assert all(np.all(np.isfinite(g)) for g in got)
    Yv, _err = fly_checked(E, plan, X, D, ens)
    assert same(got[0], Yv)                                                   # the checkpoints are the ensemble flight's
    assert not same(refs[0][1], refs[2][1]) and not same(refs[0][2][:, 1], refs[2][2][:, 1])   # the wind is felt, in the mid-flight row too
    plan.close()
    ens.close()


# ------------------------------------------------------------------ 4. forms and independence
B130 = 130
CYCLE130 = (np.arange(B130) % 6) - 1


def _forms_case():
    prob, E, X67, _pd, _ud = example()
    X = np.ascontiguousarray(X67[np.arange(B130) % B67])
    return prob, E, X, dispersion(B130, E.S), members(33, SEEDS, calm_of=1)


def test_tangent_forms_and_independence(monkeypatch):
    prob, E, X, D, T = _forms_case()
    dX, dD = shared_seeds(prob, X[0])
    ens = E.wind_ensemble(T).assign(CYCLE130)
    plan = E.propagation_plan(steps=1, restart="chain")
    Y, dY = tangent_checked(E, plan, X, D, dX, dD, True, ens)
    # slabs of 64 + 64 + 2: every slab reads ITS part of the assignment
    monkeypatch.setenv("GEL_PROP_SLAB", "64")
    assert plan.tangent_info(B130, 3, shared=True)["slabs"] == 3
    Ys, dYs = tangent_checked(E, plan, X, D, dX, dD, True, ens)
    monkeypatch.delenv("GEL_PROP_SLAB")
    assert plan.tangent_info(B130, 3, shared=True)["slabs"] == 1
    assert same(Ys, Y) and same(dYs, dY)
    # host form = device form
    Yh, dYh, rc = plan.tangent(X, dX=dX, dispersion=D, ddispersion=dD, shared=True, ensemble=ens)
    assert rc == 0 and same(Yh, Y) and same(dYh, dY)
    # shared seeds = per-vector copies of them
    Yc, dYc = tangent_checked(E, plan, X, D, np.broadcast_to(dX, (B130,) + dX.shape), np.broadcast_to(dD, (B130,) + dD.shape), False, ens)
    assert same(Yc, Y) and same(dYc, dY)
    # P = 1 is direction 0 of P = 3; a seed times 2^7
    _Y1, dY1 = tangent_checked(E, plan, X, D, dX[:1], dD[:1], True, ens)
    assert same(dY1[:, 0], dY[:, 0])
    Y7, dY7 = tangent_checked(E, plan, X, D, dX * 128.0, dD * 128.0, True, ens)
    assert same(Y7, Y) and same(dY7, dY * 128.0)
    # the batch and its assignment reversed
    rev = E.wind_ensemble(T).assign(CYCLE130[::-1])
    Yr, dYr = tangent_checked(E, plan, X[::-1], D[::-1], dX, dD, True, rev)
    assert same(Yr[::-1], Y) and same(dYr[::-1], dY)
    rev.close()
    # ensemble = None is the parent entry point; so is an assignment of -1 throughout
    Y0, dY0 = tangent_checked(E, plan, X, D, dX, dD, True, raw=True)
    Yn, dYn = tangent_checked(E, plan, X, D, dX, dD, True, None)
    assert same(Yn, Y0) and same(dYn, dY0)
    ens.assign(np.full(B130, -1))
    Ya, dYa = tangent_checked(E, plan, X, D, dX, dD, True, ens)
    assert same(Ya, Y0) and same(dYa, dY0)
    own = CYCLE130 < 0
    assert same(Y[own], Y0[own]) and same(dY[own], dY0[own]) and not same(dY[~own], dY0[~own])
    # B = 0 is valid
    ens.assign([])
    Yz, dYz, rc = plan.tangent(np.zeros((0, E.nvars)), dX=dX, shared=True, ensemble=ens)
    assert rc == 0 and Yz.shape == (0, 11 * E.M) and dYz.shape == (0, 3, 11 * E.M)
    plan.close()
    ens.close()


def test_adjoint_forms_and_independence(monkeypatch):
    prob, E, X, D, T = _forms_case()
    Lam = functionals(E, X[0])
    ens = E.wind_ensemble(T).assign(CYCLE130)
    plan = E.propagation_plan(steps=1, restart="chain")
    Y, GX, GD = adjoint_checked(E, plan, X, D, Lam, True, ens)
    monkeypatch.setenv("GEL_PROP_SLAB", "64")
    assert plan.adjoint_info(B130, 2, shared=True)["slabs"] == 3
    slabbed = adjoint_checked(E, plan, X, D, Lam, True, ens)
    monkeypatch.delenv("GEL_PROP_SLAB")
    assert plan.adjoint_info(B130, 2, shared=True)["slabs"] == 1
    assert all(same(a, b) for a, b in zip(slabbed, (Y, GX, GD)))
    Yh, GXh, GDh, rc = plan.adjoint(X, Lam, dispersion=D, shared=True, ensemble=ens)
    assert rc == 0 and same(Yh, Y) and same(GXh, GX) and same(GDh, GD)
    copies = adjoint_checked(E, plan, X, D, np.broadcast_to(Lam, (B130,) + Lam.shape), False, ens)
    assert all(same(a, b) for a, b in zip(copies, (Y, GX, GD)))
    _Y1, GX1, GD1 = adjoint_checked(E, plan, X, D, Lam[:1], True, ens)
    assert same(GX1[:, 0], GX[:, 0]) and same(GD1[:, 0], GD[:, 0])
    Y7, GX7, GD7 = adjoint_checked(E, plan, X, D, Lam * 128.0, True, ens)
    assert same(Y7, Y) and same(GX7, GX * 128.0) and same(GD7, GD * 128.0)
    rev = E.wind_ensemble(T).assign(CYCLE130[::-1])
    Yr, GXr, GDr = adjoint_checked(E, plan, X[::-1], D[::-1], Lam, True, rev)
    assert same(Yr[::-1], Y) and same(GXr[::-1], GX) and same(GDr[::-1], GD)
    rev.close()
    parent = adjoint_checked(E, plan, X, D, Lam, True, raw=True)
    none = adjoint_checked(E, plan, X, D, Lam, True, None)
    assert all(same(a, b) for a, b in zip(none, parent))
    ens.assign(np.full(B130, -1))
    all_own = adjoint_checked(E, plan, X, D, Lam, True, ens)
    assert all(same(a, b) for a, b in zip(all_own, parent))
    own = CYCLE130 < 0
    assert same(GX[own], parent[1][own]) and same(GD[own], parent[2][own]) and not same(GX[~own], parent[1][~own])
    ens.assign([])
    Yz, GXz, GDz, rc = plan.adjoint(np.zeros((0, E.nvars)), Lam, shared=True, ensemble=ens)
    assert rc == 0 and Yz.shape == (0, 11 * E.M) and GXz.shape == (0, 2, E.nvars) and GDz.shape == (0, 2, E.S, 4)
    plan.close()
    ens.close()


# ------------------------------------------------------------------ 5. beyond the handle's limit
def test_a_member_longer_than_any_handle_accepts():
    """Kw = 400 (a handle refuses it), B = 3, chain: y of both calls is gel_propagate_ensemble's, the outputs are finite, zero seeds
    and zero lam give zeros, the 2^k scaling holds in bits.  No handle exists to compare the derivatives with: they rest on the
    instantiation test 1 pins at K = 160; the row count is data, not a code path."""
    prob, E, X67, _pd, _ud = example()
    X = np.ascontiguousarray(X67[:3])
    T = members(400, (15, 16, 17))
    ens = E.wind_ensemble(T).assign([0, 1, 2])
    plan = E.propagation_plan(steps=1, restart="chain")
    dX, dD = shared_seeds(prob, X[0])
    Lam = functionals(E, X[0])
    Yv, _err = fly_checked(E, plan, X, None, ens)
    Y, dY = tangent_checked(E, plan, X, None, dX, dD, True, ens)
    Ya, GX, GD = adjoint_checked(E, plan, X, None, Lam, True, ens)
    assert same(Y, Yv) and same(Ya, Yv)
    assert all(np.all(np.isfinite(a)) for a in (Y, dY, GX, GD)) and np.any(dY != 0) and np.any(GX != 0) and np.any(GD[:, :, :, 3] != 0)
    _Y, dYz = tangent_checked(E, plan, X, None, np.zeros_like(dX), np.zeros_like(dD), True, ens)
    _Y, GXz, GDz = adjoint_checked(E, plan, X, None, np.zeros_like(Lam), True, ens)
    assert np.all(dYz == 0.0) and np.all(GXz == 0.0) and np.all(GDz == 0.0)
    for sc in (2.0 ** -3, 2.0 ** 7):
        _Y, dYs = tangent_checked(E, plan, X, None, dX * sc, dD * sc, True, ens)
        _Y, GXs, GDs = adjoint_checked(E, plan, X, None, Lam * sc, True, ens)
        assert same(dYs, dY * sc) and same(GXs, GX * sc) and same(GDs, GD * sc), sc
    plan.close()
    ens.close()


# ------------------------------------------------------------------ 6. status
def test_status_nan_member():
    """member 2 holds NaN wind entries inside the altitudes flown: its flights' y, dy, gx and gdisp are non-finite, the others keep
    the bits of the clean ensemble, gel_sync reports GEL_NONFINITE for the tangent and for the adjoint, and the next clean call
    returns 0"""
    from gelato_amd import _lib
    prob, E, X, _pd, _ud = example()
    T = members(33, SEEDS, calm_of=1)
    Tn = T.copy()
    rows = (T[2, :, 0] > 4000.0) & (T[2, :, 0] < 12000.0)                    # (tests/test_wind_ensemble.py: every ascent has nodes there)
    assert rows.sum() >= 2 and not rows[0] and not rows[-1]
    Tn[2, rows, 1] = np.nan
    D = dispersion(B67, E.S)
    D[:, :, 3] = np.where(D[:, :, 3] == 0.0, 0.5, D[:, :, 3])
    dX, dD = shared_seeds(prob, X[0])
    Lam = functionals(E, X[0])
    clean = E.wind_ensemble(T).assign(CYCLE)
    ens = E.wind_ensemble(Tn).assign(CYCLE)
    plan = E.propagation_plan(steps=1, restart="chain")
    hit = CYCLE == 2
    assert hit.sum() == 11
    t0 = tangent_checked(E, plan, X, D, dX, dD, True, clean)
    t1 = tangent_checked(E, plan, X, D, dX, dD, True, ens, status=_lib.GEL_NONFINITE)
    t2 = tangent_checked(E, plan, X, D, dX, dD, True, clean)                  # the next call is clean (status 0 inside)
    a0 = adjoint_checked(E, plan, X, D, Lam, True, clean)
    a1 = adjoint_checked(E, plan, X, D, Lam, True, ens, status=_lib.GEL_NONFINITE)
    a2 = adjoint_checked(E, plan, X, D, Lam, True, clean)
    for got, ref, again in ((t1, t0, t2), (a1, a0, a2)):
        assert all(same(g, r) for g, r in zip(again, ref))
        for g, r in zip(got, ref):
            assert same(g[~hit], r[~hit])
            flat = g[hit].reshape(11, -1) if g.ndim == 2 else g[hit].reshape(11 * g.shape[1], -1)
            assert not np.isfinite(flat).all(axis=1).any()                    # every (vector, direction / functional) slice of member 2
    for o in (plan, ens, clean):
        o.close()

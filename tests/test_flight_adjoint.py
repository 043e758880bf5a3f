"""The adjoint flight on the device (gel_propagate_adjoint*): gx and gdisp against the 60-digit truth of
tests/golden/g31_flight_adjoint.npz within its carried bound 2 Eg, the bound's teeth around the device's values, duality against the
device's own tangent on the long-table flights, the bit-exact properties, status, and propagate.flight_gradient.

Cases (tests/flight_tangent_truth.py): the shipped example (12 phases, N = 66) and a 3-phase problem without aerodynamics (n = 5), each a
batch of three with factors that differ per vector and phase; the truth holds the gradients of vector 1 for seven functionals."""
import os

import numpy as np
import pytest

import flight_adjoint_truth as at
import flight_tangent_truth as tt

pytestmark = pytest.mark.gpu
IDS = lambda f: "%s-%s-k%d" % f   # noqa: E731


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


_CASE = {}


def _case(name):
    """(prob, engine, X [3, nvars], disp [3, S, 4], Lam [3, 7, 11 M]) of a case, shared by the tests"""
    if name not in _CASE:
        from gelato_amd import Engine
        prob, X, disp = tt.case(name)
        Lam = np.stack([at.pack_lam(at.functionals(prob, X[b])) for b in range(3)])
        _CASE[name] = (prob, Engine(prob), X, disp, Lam)
    return _CASE[name]


_DEV = {}


def _device(flight):
    """the device's (Y, GX, GD) of the case's batch for the seven functionals of every vector, computed once per flight"""
    if flight not in _DEV:
        prob, E, X, disp, Lam = _case(flight[0])
        plan = E.propagation_plan(steps=flight[2], restart=flight[1])
        Y, GX, GD, rc = plan.adjoint(X, Lam, dispersion=disp)
        plan.close()
        assert rc == 0
        _DEV[flight] = (Y, GX, GD)
    return _DEV[flight]


@pytest.mark.parametrize("flight", tt.FLIGHTS, ids=IDS)
def test_truth(flight):
    """(e) gx and gdisp of vector 1 within 2 Eg of g31 in every entry, nothing masked, with g31's zero pattern; y is the flight the
    truth differentiated; the largest share of 2 Eg per group is printed"""
    import propagate_truth as pt
    prob, E, X, disp, Lam = _case(flight[0])
    g30, g31 = tt.load(flight), at.load(flight)
    Y, GX, GD = _device(flight)
    b = tt.TRUTH_VEC
    assert np.abs(pt.unpack_y(Y[b], E.M) - g30["y"]).max() <= 1e-9 * (1.0 + np.abs(g30["y"]).max())
    grp = at.groups(prob)
    use = np.zeros((7, 7))
    for q in range(7):
        assert np.array_equal(GX[b, q] != 0, g31["gx"][q] != 0) and np.array_equal(GD[b, q] != 0, g31["gdisp"][q] != 0), at.FUNCTIONALS[q]
        for k, name in enumerate(at.GROUPS[:6]):
            i = grp[name]
            use[q, k] = at.miss(GX[b, q][i], g31["gx"][q][i], 2 * g31["Egx"][q][i])
        use[q, 6] = at.miss(GD[b, q], g31["gdisp"][q], 2 * g31["Egd"][q])
    print("share of 2 Eg used, %s %s k=%d, per group %s: %s; per functional %s"
          % (flight + (at.GROUPS, np.array2string(use.max(axis=0), precision=3), np.array2string(use.max(axis=1), precision=3))))
    assert np.all(use <= 1.0), (flight, use)


@pytest.mark.parametrize("flight", tt.FLIGHTS, ids=IDS)
def test_bound_rejects_wrong_restatements(flight):
    """the same bound, around the DEVICE's values, rejects the wrong restatements evaluated from g30's per-stage partials"""
    import interp_truth as it
    prob, E, X, disp, Lam = _case(flight[0])
    g30, g31 = tt.load(flight), at.load(flight)
    _Y, GX, GD = _device(flight)
    b = tt.TRUTH_VEC
    mats, hs = tt.plan_tables(it.engine(prob), flight[2], flight[1])
    lam = at.functionals(prob, g30["x"])
    for mut in at.MUTATIONS:
        if mut == "no_knot_minus" and flight[1] != "chain":
            continue     # (section mode: no knot is crossed)
        worst = 0.0
        for q in range(7):
            gx, gd = at.adjoint(prob, flight[1], flight[2], g30["x"], mats, hs, g30, lam[q], mutate=mut)
            worst = max(worst, at.miss(gx, GX[b, q], 2 * g31["Egx"][q]), at.miss(gd, GD[b, q], 2 * g31["Egd"][q]))
        print("mutation %s, %s %s k=%d: misses the bound around the device's values by a factor %.3g" % ((mut,) + flight + (worst,)))
        assert worst > 1.0e3, (flight, mut, worst)


@pytest.mark.parametrize("flight", tt.TABLE_FLIGHTS, ids=IDS)
def test_device_duality_over_the_long_tables(flight):
    """(f) shapes the fixture does not hold: on the flights over the long wind and CA tables, with shared seeds and the seven
    functionals, |<lam, dy_dev> - <gx_dev, dX> - <gdisp_dev, dD>| <= 2 sum |lam| E with g30's bound E of that flight.  (g30 keeps no
    per-stage values for these flights, so the Eg' term of the right side is not available: the right side is the E term alone.)"""
    prob, E, X, disp, Lam = _case(flight[0])
    g = tt.load(flight)
    b = tt.TRUTH_VEC
    dX, dD = tt.directions(prob, X[b])
    plan = E.propagation_plan(steps=flight[2], restart=flight[1])
    Y, dY, rc = plan.tangent(X[[b]], dX=dX, dispersion=disp[[b]], ddispersion=dD, shared=True)
    Y2, GX, GD, rc2 = plan.adjoint(X[[b]], Lam[b], dispersion=disp[[b]], shared=True)
    plan.close()
    assert rc == 0 and rc2 == 0 and np.array_equal(_bits(Y), _bits(Y2))
    lam = at.functionals(prob, X[b])                       # [7, M, 11]
    dy = tt.unpack_dy(dY[0], E.M)                          # [11, M, 11]
    worst = 0.0
    for q in range(7):
        for d in range(11):
            left = float((lam[q] * dy[d]).sum())
            right = float(GX[0, q].dot(dX[d]) + (GD[0, q] * dD[d]).sum())
            bound = 2 * float((np.abs(lam[q]) * g["bound"][d]).sum())
            share = abs(left - right) / bound if bound > 0 else (0.0 if left == right else np.inf)
            worst = max(worst, share)
    print("%s %s k=%d: duality uses %.3g of 2 sum |lam| E" % (flight + (worst,)))
    assert worst <= 1.0, (flight, worst)


@pytest.mark.parametrize("mode", ["section", "chain"])
@pytest.mark.parametrize("name,k", [("example", 1), ("noair", 3)])
def test_bits_y_zero_scaling_factors_of_one(name, k, mode):
    """(g) y is gel_propagate_dispersed's, with and without factors; lam == 0 gives zeros; lam times 2^-3 / 2^5 gives the outputs times
    the same power bit for bit; disp == None is factors of one"""
    prob, E, X, disp, Lam = _case(name)
    plan = E.propagation_plan(steps=k, restart=mode)
    for D in (None, disp):
        Y0, _e, rc0 = plan.apply(X, want_err=False, dispersion=D)
        Y, GX, GD, rc = plan.adjoint(X, Lam, dispersion=D)
        assert rc0 == 0 and rc == 0 and np.array_equal(_bits(Y), _bits(Y0)), (name, mode, D is None)
        assert np.all(np.isfinite(GX)) and np.all(np.isfinite(GD)) and np.any(GX != 0) and np.any(GD != 0)
        Yz, GXz, GDz, rc = plan.adjoint(X, np.zeros_like(Lam), dispersion=D)
        assert rc == 0 and np.array_equal(_bits(Yz), _bits(Y0)) and np.all(GXz == 0.0) and np.all(GDz == 0.0)
        for sc in (2.0 ** -3, 2.0 ** 5):
            _Y, GXs, GDs, rc = plan.adjoint(X, Lam * sc, dispersion=D)
            assert rc == 0 and np.array_equal(_bits(GXs), _bits(GX * sc)) and np.array_equal(_bits(GDs), _bits(GD * sc)), (name, mode, sc)
    a = plan.adjoint(X, Lam)
    b = plan.adjoint(X, Lam, dispersion=np.ones_like(disp))
    assert a[3] == 0 and b[3] == 0 and all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(a[:3], b[:3]))
    # inputs the value call does not read: +0.0, bit for bit
    M = E.M
    nn = [int(v) for v in E.num_nodes]
    xa = [sum(nn[:s]) + s for s in range(E.S)]
    read = np.zeros(E.nvars, dtype=bool)
    for s in range(E.S):
        if mode == "section" or s == 0:
            read[tt.state_rows(M, xa[s])] = True
        else:
            read[tt.state_rows(M, xa[s])] = read[tt.state_rows(M, xa[s] - 1)] = True
        if not prob["attitude_hold"][s]:
            ua = sum(nn[:s])
            read[11 * M + 2 * ua:11 * M + 2 * (ua + nn[s])] = True
    read[11 * M + 2 * E.N:] = True
    assert np.all(_bits(a[1][:, :, ~read]) == 0)
    plan.close()


@pytest.mark.parametrize("mode", ["section", "chain"])
def test_bits_functional_batch_slab_buffers(mode):
    """(g) functional q alone is functional q among seven; B = 1, B = 3 and batch positions 0, 63, 64, 129 of 130; two slabs under
    GEL_PROP_SLAB=64; shared lam against per-vector copies; host buffers against device buffers, into poisoned buffers"""
    import torch
    prob, E, X, disp, Lam = _case("example")
    plan = E.propagation_plan(steps=1, restart=mode)
    Y7, GX7, GD7, rc = plan.adjoint(X, Lam, dispersion=disp)
    assert rc == 0
    for q in (0, 4, 6):
        _Y, g1, d1, rc = plan.adjoint(X, Lam[:, [q]], dispersion=disp)
        assert rc == 0 and np.array_equal(_bits(g1[:, 0]), _bits(GX7[:, q])) and np.array_equal(_bits(d1[:, 0]), _bits(GD7[:, q])), (mode, q)
    y1, g1, d1, rc = plan.adjoint(X[1], Lam[[1]], dispersion=disp[[1]])
    assert rc == 0 and np.array_equal(_bits(y1[0]), _bits(Y7[1])) and np.array_equal(_bits(g1[0]), _bits(GX7[1])) and np.array_equal(_bits(d1[0]), _bits(GD7[1]))
    # 130 vectors: cyclic copies of the three with their own functionals (three of the seven)
    sel = [6, 2, 5]
    idx = np.arange(130) % 3
    XX, DD, LL = X[idx], disp[idx], np.ascontiguousarray(Lam[idx][:, sel])
    results = []
    for slab in (None, "64"):
        if slab:
            os.environ["GEL_PROP_SLAB"] = slab
        try:
            assert plan.adjoint_info(130, 3)["slabs"] == (3 if slab else 1)
            results.append(plan.adjoint(XX, LL, dispersion=DD))
        finally:
            os.environ.pop("GEL_PROP_SLAB", None)
    (Ya, Ga, Da, rca), (Yb, Gb, Db, rcb) = results
    assert rca == 0 and rcb == 0
    assert np.array_equal(_bits(Ya), _bits(Yb)) and np.array_equal(_bits(Ga), _bits(Gb)) and np.array_equal(_bits(Da), _bits(Db))
    assert np.array_equal(_bits(Ga[:3]), _bits(GX7[:, sel])) and np.array_equal(_bits(Da[:3]), _bits(GD7[:, sel])) and np.array_equal(_bits(Ya[:3]), _bits(Y7))
    for pos in (0, 63, 64, 129):
        y1, g1, d1, rc = plan.adjoint(XX[pos], LL[[pos]], dispersion=DD[[pos]])
        assert rc == 0 and np.array_equal(_bits(y1[0]), _bits(Ya[pos])) and np.array_equal(_bits(g1[0]), _bits(Ga[pos]))
        assert np.array_equal(_bits(d1[0]), _bits(Da[pos])), (mode, pos)
    # device buffers, poisoned
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (XX, DD, LL)]
    dY = torch.full((130, 11 * E.M), -3.0, dtype=torch.float64, device="cuda")
    dG = torch.full((130, 3, E.nvars), -3.0, dtype=torch.float64, device="cuda")
    dD = torch.full((130, 3, E.S, 4), -3.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    plan.adjoint_device(130, 3, t[0].data_ptr(), t[2].data_ptr(), dY.data_ptr(), dG.data_ptr(), d_gdisp=dD.data_ptr(), d_dispersion=t[1].data_ptr())
    assert E.sync() == 0
    assert np.array_equal(_bits(dY.cpu().numpy()), _bits(Ya)) and np.array_equal(_bits(dG.cpu().numpy()), _bits(Ga))
    assert np.array_equal(_bits(dD.cpu().numpy()), _bits(Da))
    # gdisp not wanted: gx and y as before
    dG.fill_(-3.0)
    torch.cuda.synchronize()
    plan.adjoint_device(130, 3, t[0].data_ptr(), t[2].data_ptr(), dY.data_ptr(), dG.data_ptr(), d_dispersion=t[1].data_ptr())
    assert E.sync() == 0 and np.array_equal(_bits(dG.cpu().numpy()), _bits(Ga))
    # shared lam: vector 0's three for everybody, against per-vector copies; in slabs too
    sL = np.ascontiguousarray(Lam[0][sel])
    Yc, Gc, Dc, rc = plan.adjoint(XX, np.broadcast_to(sL, (130,) + sL.shape).copy(), dispersion=DD)
    assert rc == 0
    for slab in (None, "64"):
        if slab:
            os.environ["GEL_PROP_SLAB"] = slab
        try:
            Ys, Gs, Ds, rc = plan.adjoint(XX, sL, dispersion=DD, shared=True)
        finally:
            os.environ.pop("GEL_PROP_SLAB", None)
        assert rc == 0 and np.array_equal(_bits(Ys), _bits(Yc)) and np.array_equal(_bits(Gs), _bits(Gc)) and np.array_equal(_bits(Ds), _bits(Dc)), (mode, slab)
    plan.close()


def test_status_nan_lam_state_empty_batch_and_node_plan():
    """(h) a NaN in one (vector, functional)'s lam makes only that slice non-finite; a NaN state in one vector's x leaves the other
    vectors their bits; both raise GEL_NONFINITE and the next call is clean.  B = 0 succeeds.  A node-restart plan is refused."""
    from gelato_amd import _lib
    prob, E, X, disp, Lam = _case("example")
    M = E.M
    nn = [int(v) for v in E.num_nodes]
    xa = [sum(nn[:s]) + s for s in range(E.S)]
    plan = E.propagation_plan(steps=1, restart="chain")
    Q = 4
    okY, okG, okD, rc = plan.adjoint(X, Lam[:, :Q], dispersion=disp)
    assert rc == 0 and np.all(np.isfinite(okG)) and np.all(np.isfinite(okD))
    bad = Lam[:, :Q].copy()
    bad[1, 2, xa[3]] = np.nan              # the mass row of phase 3's first node
    Y, G, D, rc = plan.adjoint(X, bad, dispersion=disp)
    assert rc == _lib.GEL_NONFINITE and np.array_equal(_bits(Y), _bits(okY))
    keep = np.ones((3, Q), dtype=bool)
    keep[1, 2] = False
    assert np.array_equal(_bits(G[keep]), _bits(okG[keep])) and np.array_equal(_bits(D[keep]), _bits(okD[keep]))
    assert not np.all(np.isfinite(G[1, 2]))
    Y2, G2, D2, rc = plan.adjoint(X, Lam[:, :Q], dispersion=disp)
    assert rc == 0 and np.array_equal(_bits(G2), _bits(okG)) and np.array_equal(_bits(D2), _bits(okD)) and np.array_equal(_bits(Y2), _bits(okY))
    Xb = X.copy()
    Xb[1, M + 3 * xa[3] + 1] = np.nan      # position y of phase 3's first node of vector 1
    Y, G, D, rc = plan.adjoint(Xb, Lam[:, :Q], dispersion=disp)
    assert rc == _lib.GEL_NONFINITE
    assert np.array_equal(_bits(Y[[0, 2]]), _bits(okY[[0, 2]])) and np.array_equal(_bits(G[[0, 2]]), _bits(okG[[0, 2]]))
    assert np.array_equal(_bits(D[[0, 2]]), _bits(okD[[0, 2]]))
    Y2, G2, D2, rc = plan.adjoint(X, Lam[:, :Q], dispersion=disp)
    assert rc == 0 and np.array_equal(_bits(G2), _bits(okG))
    # B = 0
    Y0, G0, D0, rc = plan.adjoint(np.zeros((0, E.nvars)), np.zeros((0, 2, 11 * M)))
    assert rc == 0 and Y0.shape == (0, 11 * M) and G0.shape == (0, 2, E.nvars) and D0.shape == (0, 2, E.S, 4)
    Y0, G0, D0, rc = plan.adjoint(np.zeros((0, E.nvars)), np.zeros((3, 11 * M)), shared=True)
    assert rc == 0 and G0.shape == (0, 3, E.nvars)
    plan.adjoint_device(0, 1, 0, 8, 0, 0)
    assert E.sync() == 0
    plan.close()
    node = E.propagation_plan(steps=1, restart="node")
    with pytest.raises(_lib.GelatoAmdError, match="GEL_PROP_RESTART_NODE"):
        node.adjoint(X, Lam[:, :Q], dispersion=disp)
    node.close()


def test_fixture_pairs_against_the_tangent():
    """(i) where both fixtures hold a bound: the terminal functionals' entries for the unit lift-off seeds (mass, position y, velocity
    z) against the device tangent's terminal rows along those seeds, within 2 E + 2 Eg"""
    flight = tt.FLIGHTS[0]
    prob, E, X, disp, Lam = _case(flight[0])
    g30, g31 = tt.load(flight), at.load(flight)
    b = tt.TRUTH_VEC
    M = E.M
    dX, dD = tt.directions(prob, X[b])
    plan = E.propagation_plan(steps=flight[2], restart=flight[1])
    _Y, dY, rc = plan.tangent(X[[b]], dX=dX[:3], dispersion=disp[[b]], shared=True)
    plan.close()
    assert rc == 0
    dy = tt.unpack_dy(dY[0], M)
    GX = _device(flight)[1][b]
    for d, xi in enumerate((tt.sidx(M, 0, 0), tt.sidx(M, 0, 2), tt.sidx(M, 0, 6))):
        for q, c in enumerate((0, 1, 6, 8)):
            tol = 2 * g30["bound"][d][M - 1, c] + 2 * g31["Egx"][q][xi]
            assert abs(dy[d, M - 1, c] - GX[q, xi]) <= tol, (d, q, dy[d, M - 1, c], GX[q, xi], tol)


def test_flight_gradient():
    """(i) flight_gradient's terminal rows against flight_jacobian's columns (all four groups of jacobian_seeds) on the example, and
    of=("rows", mu) against mu^T (flight_jacobian's row block).  Both sides evaluate the same discrete map at 2 steps per node
    interval, K = 4 * 132 stages, each stage's partials inside the contract of DESIGN.md 3.6 (1e-9 relative, 1e-12 absolute): to
    first order the two differ by at most K (1e-9 |entry| + 1e-12 (largest entry of the functional's row)) each."""
    from gelato_amd import Engine, propagate
    prob, E0, X, disp, _L = _case("example")
    E = Engine(prob)
    M = E.M
    last = M - 1
    wrt = propagate.JACOBIAN_GROUPS
    jac = propagate.flight_jacobian(X, None, None, steps=1, wrt=wrt, dispersion=disp, engine=E)
    out = propagate.flight_gradient(X, None, None, steps=1, dispersion=disp, engine=E)
    assert out["status"] == 0 and jac["status"] == 0 and out["columns"] == jac["columns"]
    assert np.array_equal(_bits(out["y"]), _bits(jac["y"])) and np.array_equal(_bits(out["x_flown"]), _bits(jac["x_flown"]))
    assert out["functionals"] == ["terminal:%s" % n for n in ("mass", "x", "y", "z", "vx", "vy", "vz", "q0", "q1", "q2", "q3")]
    P = len(jac["columns"])
    assert out["gx"].shape == (3, 11, E.nvars) and out["gdisp"].shape == (3, 11, E.S, 4) and out["jacobian"].shape == (3, 11, P)
    ref = np.concatenate([jac["terminal"][k] for k in ("mass", "position", "velocity", "quaternion")], axis=1)      # [B, 11, P]
    K = 4 * 2 * E.N

    def close(a, r, what):
        tol = 2 * K * (1e-9 * np.abs(r) + 1e-12 * np.abs(r).max(axis=-1, keepdims=True))
        share = np.where(tol > 0, np.abs(a - r) / np.where(tol > 0, tol, 1.0), np.where(a == r, 0.0, np.inf))
        print("flight_gradient, %s: at most %.3g of the tolerance" % (what, share.max()))
        assert share.max() <= 1.0, (what, share.max())

    close(out["jacobian"], ref, "terminal against flight_jacobian")
    # the plan's own call with hand-made weights, scaled by hand
    plan = E.propagation_plan(steps=2, restart="chain")
    lam = np.zeros((11, 11 * M))
    idx = [last] + [M + 3 * last + c for c in range(3)] + [4 * M + 3 * last + c for c in range(3)] + [7 * M + 4 * last + c for c in range(4)]
    lam[np.arange(11), idx] = 1.0
    Y, GX, GD, rc = plan.adjoint(X, lam, dispersion=disp, shared=True)
    plan.close()
    um, up, uv = [float(v) for v in prob["units"][:3]]
    sc = np.array([um] + [up] * 3 + [uv] * 3 + [1.0] * 4)
    assert rc == 0 and np.array_equal(_bits(out["gx"]), _bits(GX * sc[None, :, None])) and np.array_equal(_bits(out["gdisp"]), _bits(GD * sc[None, :, None, None]))
    # a configured row table
    E.rows_configure([(last, 1.0, -1, 0.0, -0.25), (0, 1.0, last, -1.0, 0.0)], [("radius", last, 6378137.0, 1.0)])
    jac = propagate.flight_jacobian(X, None, None, steps=1, wrt=wrt, dispersion=disp, engine=E)
    mu = np.array([[1.0, 0.0, 0.0], [0.5, -2.0, 3.0]])
    out = propagate.flight_gradient(X, None, None, steps=1, of=("rows", mu), dispersion=disp, engine=E)
    assert out["status"] == 0 and out["jacobian"].shape == (3, 2, P)
    close(out["jacobian"], np.einsum("qr,brp->bqp", mu, jac["rows"]), "rows against mu^T flight_jacobian's rows")
    with pytest.raises(ValueError):
        propagate.flight_gradient(X, None, None, steps=1, of=("rows", mu), engine=E0)     # no row table
    E.close()

"""The tangent-linear propagation on the device (gel_propagate_tangent*): dy against the 60-digit truth of
tests/golden/g30_flight_tangent.npz within its carried bound 2 E, the bound's teeth around the device's dy, the bit-exact properties,
status, and propagate.flight_jacobian / montecarlo.linear_covariance.

Cases (tests/flight_tangent_truth.py): the shipped example (12 phases, N = 66) and a 3-phase problem without aerodynamics (n = 5),
each a batch of three with factors that differ per vector and phase; the truth holds the tangents of vector 1 along eleven seeds."""
import os

import numpy as np
import pytest

import flight_tangent_truth as tt
import propagate_truth as pt

pytestmark = pytest.mark.gpu
GROUPS = ("mass", "position", "velocity", "quaternion")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


_CASE = {}


def _case(name):
    """(prob, engine, X [3, nvars], disp [3, S, 4], dX [3, 11, nvars], dD [3, 11, S, 4]) of a case, shared by the tests"""
    if name not in _CASE:
        from gelato_amd import Engine
        prob, X, disp = tt.case(name)
        seeds = [tt.directions(prob, X[b]) for b in range(3)]
        _CASE[name] = (prob, Engine(prob), X, disp, np.stack([s[0] for s in seeds]), np.stack([s[1] for s in seeds]))
    return _CASE[name]


_DEV = {}


def _device_dy(flight):
    """the device's (Y, dY) of the case's batch along the eleven seeds of every vector, computed once per flight"""
    if flight not in _DEV:
        prob, E, X, disp, dX, dD = _case(flight[0])
        plan = E.propagation_plan(steps=flight[2], restart=flight[1])
        Y, dY, rc = plan.tangent(X, dX=dX, dispersion=disp, ddispersion=dD)
        plan.close()
        assert rc == 0
        _DEV[flight] = (Y, dY)
    return _DEV[flight]


def _share(got, ref, bound):
    """|got - ref| in units of the bound per entry (0 / 0 = 0, anything / 0 = inf)"""
    d = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(bound > 0, d / bound, np.where(d == 0, 0.0, np.inf))


@pytest.mark.parametrize("flight", tt.FLIGHTS, ids=lambda f: "%s-%s-k%d" % f)
def test_truth(flight):
    """dy of vector 1 within 2 E of g30 for every direction and node; y is the flight the truth differentiated"""
    prob, E, X, disp, dX, dD = _case(flight[0])
    g = tt.load(flight)
    Y, dY = _device_dy(flight)
    b = tt.TRUTH_VEC
    got = tt.unpack_dy(dY[b], E.M)
    assert np.abs(pt.unpack_y(Y[b], E.M) - g["y"]).max() <= 1e-9 * (1.0 + np.abs(g["y"]).max())
    use = np.zeros((11, 4))
    for d in range(11):
        sh = _share(got[d], g["dy"][d], 2 * g["bound"][d])
        for k, (a, c) in enumerate(pt.GROUP_COLS):
            use[d, k] = sh[:, a:c].max()
    print("share of 2 E used, %s %s k=%d, per group (mass, position, velocity, quaternion): %s; per direction %s"
          % (flight + (np.array2string(use.max(axis=0), precision=3), np.array2string(use.max(axis=1), precision=3))))
    assert np.all(use <= 1.0), (flight, use)


@pytest.mark.parametrize("flight", tt.FLIGHTS, ids=lambda f: "%s-%s-k%d" % f)
def test_bound_rejects_wrong_restatements(flight):
    """the same bound, around the DEVICE's dy, rejects the four wrong restatements evaluated from g30's per-stage partials"""
    import interp_truth as it
    prob, E, X, disp, dX, dD = _case(flight[0])
    g = tt.load(flight)
    got = tt.unpack_dy(_device_dy(flight)[1][tt.TRUTH_VEC], E.M)
    mats, hs = tt.plan_tables(it.engine(prob), flight[2], flight[1])
    for mut in tt.MUTATIONS:
        if (mut == "no_wind_slope" and flight[0] != "example") or (mut == "no_djump" and flight[1] != "chain"):
            continue     # (no air: no wind; section mode: no knot is crossed)
        worst = 0.0
        for d in range(11):
            wrong = tt.recursion(prob, flight[1], flight[2], g["x"], mats, hs, g, dX[tt.TRUTH_VEC, d], dD[tt.TRUTH_VEC, d], mutate=mut)
            worst = max(worst, float(_share(wrong, got[d], 2 * g["bound"][d]).max()))
        print("mutation %s, %s %s k=%d: misses the bound around the device's dy by a factor %.3g" % ((mut,) + flight + (worst,)))
        assert worst > 1.0e3, (flight, mut, worst)


@pytest.mark.parametrize("mode", ["section", "node", "chain"])
@pytest.mark.parametrize("name,k", [("example", 1), ("noair", 3)])
def test_bits_y_zero_seed_scaling(name, k, mode):
    """y is gel_propagate_dispersed's, with and without factors; a zero seed gives dy == 0; a seed times 2^-3 / 2^5 gives dy times
    the same power bit for bit; ddisp with disp == NULL is ddisp under factors of one"""
    prob, E, X, disp, dX, dD = _case(name)
    plan = E.propagation_plan(steps=k, restart=mode)
    for D in (None, disp):
        Y0, _e, rc0 = plan.apply(X, want_err=False, dispersion=D)
        Y, dY, rc = plan.tangent(X, dX=dX, dispersion=D, ddispersion=dD)
        assert rc0 == 0 and rc == 0 and np.array_equal(_bits(Y), _bits(Y0)), (name, mode, D is None)
        assert np.all(np.isfinite(dY)) and np.any(dY != 0)
        Yz, dYz, rc = plan.tangent(X, dX=np.zeros_like(dX), dispersion=D, ddispersion=np.zeros_like(dD))
        assert rc == 0 and np.array_equal(_bits(Yz), _bits(Y0)) and np.all(dYz == 0.0)
        for sc in (2.0 ** -3, 2.0 ** 5):
            _Y, dYs, rc = plan.tangent(X, dX=dX * sc, dispersion=D, ddispersion=dD * sc)
            assert rc == 0 and np.array_equal(_bits(dYs), _bits(dY * sc)), (name, mode, sc)
    Ya, dYa, rca = plan.tangent(X, ddispersion=dD)
    Yb, dYb, rcb = plan.tangent(X, dispersion=np.ones_like(disp), ddispersion=dD)
    assert rca == 0 and rcb == 0 and np.array_equal(_bits(Ya), _bits(Yb)) and np.array_equal(_bits(dYa), _bits(dYb))
    # one seed NULL is that seed zero
    Yc, dYc, _rc = plan.tangent(X, dX=dX, dispersion=disp)
    Yd, dYd, _rc = plan.tangent(X, dX=dX, dispersion=disp, ddispersion=np.zeros_like(dD))
    assert np.array_equal(_bits(dYc), _bits(dYd)) and np.array_equal(_bits(Yc), _bits(Yd))
    plan.close()


@pytest.mark.parametrize("mode", ["section", "chain"])
def test_bits_direction_batch_slab_buffers(mode):
    """direction p alone is the same direction among P = 5; B = 1 is batch positions 0, 63, 64, 66 of 67; one slab is
    GEL_PROP_SLAB=64; host buffers are device buffers; shared seeds are per-vector copies of them"""
    import torch
    prob, E, X, disp, dX, dD = _case("example")
    k = 1
    plan = E.propagation_plan(steps=k, restart=mode)
    P = 5
    sel = [10, 7, 3, 9, 6]
    Y5, dY5, rc = plan.tangent(X, dX=dX[:, sel], dispersion=disp, ddispersion=dD[:, sel])
    assert rc == 0
    for i, p in enumerate(sel):
        _Y, d1, rc = plan.tangent(X, dX=dX[:, [p]], dispersion=disp, ddispersion=dD[:, [p]])
        assert rc == 0 and np.array_equal(_bits(d1[:, 0]), _bits(dY5[:, i])), (mode, p)
    # 67 vectors: cyclic copies of the three with their own seeds
    idx = np.arange(67) % 3
    XX, DD, dXX, dDD = X[idx], disp[idx], dX[idx][:, sel], dD[idx][:, sel]
    results = []
    for slab in (None, "64"):
        if slab:
            os.environ["GEL_PROP_SLAB"] = slab
        try:
            assert plan.tangent_info(67, P)["slabs"] == (2 if slab else 1)
            results.append(plan.tangent(XX, dX=dXX, dispersion=DD, ddispersion=dDD))
        finally:
            os.environ.pop("GEL_PROP_SLAB", None)
    (Ya, dYa, rca), (Yb, dYb, rcb) = results
    assert rca == 0 and rcb == 0 and np.array_equal(_bits(Ya), _bits(Yb)) and np.array_equal(_bits(dYa), _bits(dYb))
    for pos in (0, 63, 64, 66):
        y1, d1, rc = plan.tangent(XX[pos], dX=dXX[[pos]], dispersion=DD[[pos]], ddispersion=dDD[[pos]])
        assert rc == 0 and np.array_equal(_bits(y1[0]), _bits(Ya[pos])) and np.array_equal(_bits(d1[0]), _bits(dYa[pos])), (mode, pos)
    assert np.array_equal(_bits(dYa[:3]), _bits(dY5)) and np.array_equal(_bits(Ya[:3]), _bits(Y5))
    # device buffers
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (XX, DD, dXX, dDD)]
    dY = torch.full((67, 11 * E.M), -3.0, dtype=torch.float64, device="cuda")
    ddY = torch.full((67, P, 11 * E.M), -3.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    plan.tangent_device(67, P, t[0].data_ptr(), dY.data_ptr(), ddY.data_ptr(), d_dx=t[2].data_ptr(), d_dispersion=t[1].data_ptr(),
                        d_ddispersion=t[3].data_ptr())
    assert E.sync() == 0
    assert np.array_equal(_bits(dY.cpu().numpy()), _bits(Ya)) and np.array_equal(_bits(ddY.cpu().numpy()), _bits(dYa))
    # shared seeds: vector 0's five for everybody, against per-vector copies; in two slabs too
    sX, sD = np.ascontiguousarray(dX[0][sel]), np.ascontiguousarray(dD[0][sel])
    cX, cD = np.broadcast_to(sX, (67,) + sX.shape).copy(), np.broadcast_to(sD, (67,) + sD.shape).copy()
    Yc, dYc, rc = plan.tangent(XX, dX=cX, dispersion=DD, ddispersion=cD)
    assert rc == 0
    for slab in (None, "64"):
        if slab:
            os.environ["GEL_PROP_SLAB"] = slab
        try:
            Ys, dYs, rc = plan.tangent(XX, dX=sX, dispersion=DD, ddispersion=sD, shared=True)
        finally:
            os.environ.pop("GEL_PROP_SLAB", None)
        assert rc == 0 and np.array_equal(_bits(Ys), _bits(Yc)) and np.array_equal(_bits(dYs), _bits(dYc)), (mode, slab)
    ddY.fill_(-3.0)
    ts = [torch.from_numpy(a).cuda() for a in (sX, sD)]
    torch.cuda.synchronize()
    plan.tangent_device(67, P, t[0].data_ptr(), dY.data_ptr(), ddY.data_ptr(), d_dx=ts[0].data_ptr(), d_dispersion=t[1].data_ptr(),
                        d_ddispersion=ts[1].data_ptr(), shared=True)
    assert E.sync() == 0 and np.array_equal(_bits(ddY.cpu().numpy()), _bits(dYc))
    plan.close()


def _knot_rows(E):
    nn = [int(v) for v in E.num_nodes]
    return [sum(nn[:s]) + s for s in range(E.S)], nn


@pytest.mark.parametrize("name,k", [("example", 1), ("noair", 3)])
def test_bits_modes_and_stitched_chain(name, k):
    """node mode's first interval is section mode's; chain phase 0 is section phase 0; the chain is S section-mode tangent calls
    stitched by the host with the carry rule applied to values and tangents"""
    prob, E, X, disp, dX, dD = _case(name)
    M = E.M
    xa, nn = _knot_rows(E)
    plans = {m: E.propagation_plan(steps=k, restart=m) for m in ("section", "node", "chain")}
    out = {m: plans[m].tangent(X, dX=dX, dispersion=disp, ddispersion=dD) for m in plans}
    assert all(o[2] == 0 for o in out.values())
    un = {m: (tt.unpack_dy(out[m][0], M), tt.unpack_dy(out[m][1], M)) for m in out}     # y [B, M, 11], dy [B, P, M, 11]
    for s in range(E.S):
        first = slice(xa[s], xa[s] + 2)
        assert np.array_equal(_bits(un["node"][0][:, first]), _bits(un["section"][0][:, first])), s
        assert np.array_equal(_bits(un["node"][1][:, :, first]), _bits(un["section"][1][:, :, first])), s
    p0 = slice(0, nn[0] + 1)
    assert np.array_equal(_bits(un["chain"][0][:, p0]), _bits(un["section"][0][:, p0]))
    assert np.array_equal(_bits(un["chain"][1][:, :, p0]), _bits(un["section"][1][:, :, p0]))
    assert not np.array_equal(_bits(un["chain"][1][:, :, nn[0] + 1:]), _bits(un["section"][1][:, :, nn[0] + 1:]))
    # the stitch: phase s flown by the section plan from the carried state and the carried tangent
    B, P = X.shape[0], dX.shape[1]
    y_end = dy_end = None
    for s in range(E.S):
        rows = tt.state_rows(M, xa[s])
        Xs, dXs = X.copy(), dX.copy()
        if s > 0:
            prev = tt.state_rows(M, xa[s] - 1)
            jump = X[:, rows] - X[:, prev]
            djump = dX[:, :, rows] - dX[:, :, prev]
            Xs[:, rows] = np.where(jump == 0.0, y_end, y_end + jump)
            dXs[:, :, rows] = np.where(djump == 0.0, dy_end, dy_end + djump)
        Yk, dYk, rc = plans["section"].tangent(Xs, dX=dXs, dispersion=disp, ddispersion=dD)
        assert rc == 0
        yk, dyk = tt.unpack_dy(Yk, M), tt.unpack_dy(dYk, M)
        ph = slice(xa[s], xa[s] + nn[s] + 1)
        assert np.array_equal(_bits(yk[:, ph]), _bits(un["chain"][0][:, ph])), (name, s)
        assert np.array_equal(_bits(dyk[:, :, ph]), _bits(un["chain"][1][:, :, ph])), (name, s)
        y_end, dy_end = yk[:, xa[s] + nn[s]], dyk[:, :, xa[s] + nn[s]]
    for p in plans.values():
        p.close()


def test_status_nan_seed_state_and_empty_batch():
    """a NaN in one (vector, direction)'s seed -- the mass row of phase 3's first node, which enters at that knot -- makes only that
    dy slice non-finite, from that node on; y and every other slice keep their bits; GEL_NONFINITE; the next call is clean.  A NaN
    state in x behaves as in tests/test_flight.py.  B = 0 succeeds."""
    from gelato_amd import _lib
    prob, E, X, disp, dX, dD = _case("example")
    M = E.M
    xa, nn = _knot_rows(E)
    plan = E.propagation_plan(steps=1, restart="chain")
    P = 4
    okY, okd, rc = plan.tangent(X, dX=dX[:, :P], dispersion=disp, ddispersion=dD[:, :P])
    assert rc == 0 and np.all(np.isfinite(okd))
    bad = dX[:, :P].copy()
    bad[1, 2, xa[3]] = np.nan
    Y, dY, rc = plan.tangent(X, dX=bad, dispersion=disp, ddispersion=dD[:, :P])
    assert rc == _lib.GEL_NONFINITE and np.array_equal(_bits(Y), _bits(okY))
    keep = np.ones((3, P), dtype=bool)
    keep[1, 2] = False
    assert np.array_equal(_bits(dY[keep]), _bits(okd[keep]))
    d, dok = tt.unpack_dy(dY[1, 2], M), tt.unpack_dy(okd[1, 2], M)
    assert np.array_equal(_bits(d[:xa[3]]), _bits(dok[:xa[3]]))
    assert not np.any(np.all(np.isfinite(d[xa[3]:]), axis=1))       # the mass from the knot on (and whatever it reaches)
    Y2, dY2, rc = plan.tangent(X, dX=dX[:, :P], dispersion=disp, ddispersion=dD[:, :P])
    assert rc == 0 and np.array_equal(_bits(dY2), _bits(okd)) and np.array_equal(_bits(Y2), _bits(okY))
    # a NaN state: position y of phase 3's first node of vector 1 (its jump into phase 3 is NaN)
    Xb = X.copy()
    Xb[1, M + 3 * xa[3] + 1] = np.nan
    Y, dY, rc = plan.tangent(Xb, dX=dX[:, :P], dispersion=disp, ddispersion=dD[:, :P])
    assert rc == _lib.GEL_NONFINITE
    assert np.array_equal(_bits(Y[[0, 2]]), _bits(okY[[0, 2]])) and np.array_equal(_bits(dY[[0, 2]]), _bits(okd[[0, 2]]))
    Yb = pt.unpack_y(Y[1], M)
    assert np.array_equal(_bits(Yb[:xa[3]]), _bits(pt.unpack_y(okY[1], M)[:xa[3]]))
    assert np.array_equal(_bits(tt.unpack_dy(dY[1], M)[:, :xa[3]]), _bits(tt.unpack_dy(okd[1], M)[:, :xa[3]]))
    assert not np.any(np.all(np.isfinite(Yb[xa[3]:]), axis=1))
    Y2, dY2, rc = plan.tangent(X, dX=dX[:, :P], dispersion=disp, ddispersion=dD[:, :P])
    assert rc == 0 and np.array_equal(_bits(dY2), _bits(okd))
    # B = 0
    Y0, d0, rc = plan.tangent(np.zeros((0, E.nvars)), dX=np.zeros((0, 2, E.nvars)))
    assert rc == 0 and Y0.shape == (0, 11 * M) and d0.shape == (0, 2, 11 * M)
    Y0, d0, rc = plan.tangent(np.zeros((0, E.nvars)), ddispersion=np.zeros((3, E.S, 4)), shared=True)
    assert rc == 0 and d0.shape == (0, 3, 11 * M)
    plan.tangent_device(0, 1, 0, 0, 0, d_dx=8)
    assert E.sync() == 0
    plan.close()


def test_flight_jacobian_and_linear_covariance():
    """terminal against dy's last row by hand; rows against con_matvec by hand; the columns against the tangent of the same unit
    seeds; linear_covariance symmetric in bits"""
    from gelato_amd import Engine, montecarlo, propagate
    prob, E0, X, disp, _dX, _dD = _case("example")
    E = Engine(prob)
    M = E.M
    last = M - 1
    E.rows_configure([(last, 1.0, -1, 0.0, -0.25), (0, 1.0, last, -1.0, 0.0)], [("radius", last, 6378137.0, 1.0)])
    wrt = ("initial", "dispersion", "times", "controls_bias")
    out = propagate.flight_jacobian(X, None, None, steps=1, wrt=wrt, dispersion=disp, engine=E)
    cols, sX, sD = propagate.jacobian_seeds(E.num_nodes, prob["attitude_hold"], wrt)
    P = len(cols)
    assert out["columns"] == cols and out["status"] == 0 and P == 11 + 4 * E.S + E.S + 1 + 2 * int(np.sum(np.asarray(prob["attitude_hold"]) == 0))
    plan = E.propagation_plan(steps=2, restart="chain")
    Y, dY, rc = plan.tangent(X, dX=sX, dispersion=disp, ddispersion=sD, shared=True)
    assert rc == 0 and np.array_equal(_bits(out["dy"]), _bits(dY)) and np.array_equal(_bits(out["y"]), _bits(Y))
    assert np.array_equal(_bits(out["x_flown"][:, :11 * M]), _bits(Y)) and np.array_equal(_bits(out["x_flown"][:, 11 * M:]), _bits(X[:, 11 * M:]))
    um, up, uv = [float(v) for v in prob["units"][:3]]
    un = tt.unpack_dy(dY, M)                                           # [B, P, M, 11]
    for key, (a, c), sc in zip(GROUPS, pt.GROUP_COLS, (um, up, uv, 1.0)):
        assert out["terminal"][key].shape == (3, c - a, P)
        for b in range(3):
            assert np.array_equal(out["terminal"][key][b], (un[b, :, -1, a:c] * sc).T), (key, b)
    # the lift-off mass moves the final mass one to one (the mass row is a constant rate); a held attitude's quaternion stays
    assert np.all(np.abs(out["terminal"]["mass"][:, 0, 0] - um) <= 1e-9 * um)
    _con, jfn, rc = E.rows_eval(out["x_flown"], want_jac=True)
    assert rc == 0 and out["rows"].shape == (3, 3, P)
    for b in range(3):
        V = np.broadcast_to(sX, (P, E.nvars)).copy()
        V[:, :11 * M] = dY[b]
        r, rc = E.con_matvec(V, jfn=np.broadcast_to(jfn[b], (P,) + jfn.shape[1:]).copy())
        assert rc == 0 and np.array_equal(_bits(out["rows"][b]), _bits(r.T)), b
    # row 0 is the final mass - 0.25: its derivative is the terminal mass's, normalised
    assert np.allclose(out["rows"][:, 0, :], out["terminal"]["mass"][:, 0, :] / um, rtol=1e-13, atol=0)
    # linear covariance of the three rows under 1 % factors and nothing else
    sg = np.array([0.01 if c.startswith("dispersion") else 0.0 for c in cols])
    C_ = montecarlo.linear_covariance(out["rows"], sg)
    assert C_.shape == (3, 3, 3) and np.array_equal(_bits(C_), _bits(np.swapaxes(C_, 1, 2))) and np.all(np.isfinite(C_))
    assert np.all(np.diagonal(C_, axis1=1, axis2=2) >= 0) and np.any(C_ != 0)
    # without a row table there is no "rows"
    out1 = propagate.flight_jacobian(E0.split_x(X[0]), None, None, steps=1, engine=E0)
    assert "rows" not in out1 and out1["dy"].shape == (1, 11 + 4 * E.S + E.S + 1, 11 * M) and out1["status"] == 0
    plan.close()
    E.close()

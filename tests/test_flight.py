"""The chained flight (GEL_PROP_CHAIN) and the dispersions (gel_propagate_dispersed*) on the device: parity with
the restatement of tests/flight_truth.py under its carried bound 2 E, the bit-exact properties, status, the bound's teeth, and
propagate.fly.

Inputs: the shipped example (12 phases, N = 66) as a batch of three -- x0 itself (every knot continuous), x0 with the mass
jettisoned at its stage knots, a perturbed vector whose every component jumps a little at every knot -- and the ragged state of
tests/states.py (three perturbed copies).  The ragged state is no trajectory: flown as one chain it leaves every physical range in
phase 1 (positions of 1e17 units), where the bound of position and velocity is as large as the values; mass and quaternion stay
meaningful there, and the device must still agree with the restatement under the same bound without a non-finite value."""
import os

import numpy as np
import pytest

import flight_truth as ft
import mesh_truth as mt
import propagate_truth as pt

pytestmark = pytest.mark.gpu
GROUPS = ("mass", "position", "velocity", "quaternion")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


_CASE = {}


def _case(name):
    """(prob, engine, X [3, nvars]) of a named problem, shared by the tests"""
    if name not in _CASE:
        import interp_truth as it
        from gelato_amd import Engine, problem
        prob, x0 = it.named(name)
        E = Engine(prob)
        _CASE[name] = (prob, E, ft.flight_batch(x0, E) if name == "example" else problem.synthetic_batch(x0, E.M, 3))
    return _CASE[name]


def dispersion(B, S, seed=5):
    """[B, S, 4]: thrust, mass flow and area distinct per (vector, phase) in [0.9, 1.1]; wind factors 0, 1, 2, different from one
    phase to the next and from one vector to the next"""
    d = 0.9 + 0.2 * np.random.default_rng(seed).random((B, S, 4))
    assert len(np.unique(d[:, :, :3])) == 3 * B * S
    d[:, :, 3] = (np.arange(B)[:, None] + np.arange(S)[None, :]) % 3
    return d


_REF = {}


def _reference(name, k, dispersed, chain):
    """the restatement of every vector of the case: a list of (y [M, 11], bound_y, err [S, 4], bound_err), computed once"""
    key = (name, k, dispersed, chain)
    if key not in _REF:
        prob, E, X = _case(name)
        plan = E.propagation_plan(steps=k, restart="chain" if chain else "section")
        D = dispersion(X.shape[0], E.S) if dispersed else None
        _REF[key] = [ft.fly_all(E, plan, prob, X[b], disp=None if D is None else D[b], chain=chain) for b in range(X.shape[0])]
        plan.close()
    return _REF[key]


def check_parity(E, Y, err, reference):
    """-> (usage [2, 4] of the bounds per group, the same of the LAST section alone, [(worst y usage, worst err usage)] per vector)"""
    use, last = np.zeros((2, 4)), np.zeros((2, 4))
    worst = []
    n_last = int(E.num_nodes[-1])
    for b, (ry, by, re, be) in enumerate(reference):
        assert np.all(np.isfinite(ry)) and np.all(np.isfinite(by)), b
        gy = np.abs(pt.unpack_y(Y[b], E.M) - ry)
        ge = np.abs(err[b] - re)
        with np.errstate(divide="ignore", invalid="ignore"):
            sy = np.where(by > 0, gy / by, np.where(gy == 0, 0.0, np.inf))
            se = np.where(be > 0, ge / be, np.where(ge == 0, 0.0, np.inf))
        for g, (a, c) in enumerate(pt.GROUP_COLS):
            use[0, g] = max(use[0, g], float(sy[:, a:c].max()))
            use[1, g] = max(use[1, g], float(se[:, g].max()))
            last[0, g] = max(last[0, g], float(sy[-n_last - 1:, a:c].max()))
            last[1, g] = max(last[1, g], float(se[-1, g]))
        worst.append((float(np.nan_to_num(sy, nan=np.inf).max()), float(np.nan_to_num(se, nan=np.inf).max())))
    return use, last, worst


CASES = [("example", 1), ("example", 3), ("ragged", 1), ("ragged", 3)]


@pytest.mark.parametrize("name,k", CASES)
def test_parity_chain(name, k):
    """y and err of the chained flight against the restatement, within 2 E"""
    prob, E, X = _case(name)
    plan = E.propagation_plan(steps=k, restart="chain")
    Y, err, rc = plan.apply(X)
    assert rc == 0
    use, last, worst = check_parity(E, Y, err, _reference(name, k, False, True))
    print("bound usage %s k=%d chain: y %s err %s; last section: y %s err %s" % (
        name, k, np.array2string(use[0], precision=3), np.array2string(use[1], precision=3),
        np.array2string(last[0], precision=3), np.array2string(last[1], precision=3)))
    assert all(wy <= 1.0 and we <= 1.0 for wy, we in worst), (name, k, worst)
    plan.close()


@pytest.mark.parametrize("mode", ["chain", "section"])
@pytest.mark.parametrize("name,k", CASES)
def test_parity_dispersed(name, k, mode):
    """the same under factors that differ per (vector, phase): thrust, mass flow, area in [0.9, 1.1], wind 0, 1, 2"""
    prob, E, X = _case(name)
    plan = E.propagation_plan(steps=k, restart=mode)
    Y, err, rc = plan.apply(X, dispersion=dispersion(X.shape[0], E.S))
    assert rc == 0
    use, last, worst = check_parity(E, Y, err, _reference(name, k, True, mode == "chain"))
    print("bound usage %s k=%d %s dispersed: y %s err %s; last section: y %s err %s" % (
        name, k, mode, np.array2string(use[0], precision=3), np.array2string(use[1], precision=3),
        np.array2string(last[0], precision=3), np.array2string(last[1], precision=3)))
    assert all(wy <= 1.0 and we <= 1.0 for wy, we in worst), (name, k, mode, worst)
    # the factors matter: the undispersed flight is elsewhere
    Y0, _e, _rc = plan.apply(X)
    assert not np.array_equal(_bits(Y0), _bits(Y))
    plan.close()


@pytest.mark.parametrize("mode", ["section", "node", "chain"])
def test_bits_ones_equal_null(mode):
    """factors of exactly 1.0 change no bit, in every mode; on device buffers too"""
    import torch
    for name in ("example", "ragged"):
        prob, E, X = _case(name)
        plan = E.propagation_plan(steps=2, restart=mode)
        Y0, e0, rc0 = plan.apply(X)
        Y1, e1, rc1 = plan.apply(X, dispersion=np.ones((X.shape[0], E.S, 4)))
        assert rc0 == 0 and rc1 == 0
        assert np.array_equal(_bits(Y0), _bits(Y1)) and np.array_equal(_bits(e0), _bits(e1)), (name, mode)
        B = X.shape[0]
        dX, dD = torch.from_numpy(X).cuda(), torch.ones((B, E.S, 4), dtype=torch.float64, device="cuda")
        dY = torch.full((B, 11 * E.M), -3.0, dtype=torch.float64, device="cuda")
        dE = torch.full((B, E.S, 4), -3.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        plan.apply_device(B, dX.data_ptr(), dY.data_ptr(), dE.data_ptr(), dD.data_ptr())
        assert E.sync() == 0
        assert np.array_equal(_bits(dY.cpu().numpy()), _bits(Y0)) and np.array_equal(_bits(dE.cpu().numpy()), _bits(e0)), (name, mode)
        plan.close()


def _knot_rows(E):
    nn = [int(v) for v in E.num_nodes]
    return [sum(nn[:s]) + s for s in range(E.S)], nn


@pytest.mark.parametrize("dispersed", [False, True], ids=["plain", "dispersed"])
def test_bits_chain_is_stitched_sections(dispersed):
    """the chain equals S section-mode calls stitched by the host: after section s the host writes fl(y_end + jump), or y_end at a
    zero jump, into the first node of section s + 1 of a working copy of x (the jump from the ORIGINAL x); chain phase 0 is the
    section mode's phase 0; node xa of phase 0 is X_0; across a continuous knot the start of s + 1 is the end of s, bit for bit,
    across a jump it is fl(y + jump)"""
    for name in ("example", "ragged"):
        prob, E, X = _case(name)
        M, S, B = E.M, E.S, X.shape[0]
        D = dispersion(B, S) if dispersed else None
        chain, sec = E.propagation_plan(steps=2, restart="chain"), E.propagation_plan(steps=2)
        Yc, ec, rc = chain.apply(X, dispersion=D)
        assert rc == 0
        xa, nn = _knot_rows(E)
        Xw = X.copy()
        Ys = np.zeros_like(Yc)
        for s in range(S):
            Y, _e, rc = sec.apply(Xw, dispersion=D)
            assert rc == 0
            for b in range(B):
                Yn, Xo, Xn = pt.unpack_y(Y[b], M), pt.unpack_y(X[b, :11 * M], M), pt.unpack_y(Xw[b, :11 * M], M)
                rows = slice(xa[s], xa[s] + nn[s] + 1)
                Yb = pt.unpack_y(Ys[b], M)
                Yb[rows] = Yn[rows]
                if s + 1 < S:
                    jump = Xo[xa[s + 1]] - Xo[xa[s + 1] - 1]
                    Xn[xa[s + 1]] = np.where(jump == 0.0, Yn[xa[s + 1] - 1], Yn[xa[s + 1] - 1] + jump)
                    Xw[b, :11 * M] = np.concatenate([Xn[:, 0], Xn[:, 1:4].ravel(), Xn[:, 4:7].ravel(), Xn[:, 7:11].ravel()])
                Ys[b] = np.concatenate([Yb[:, 0], Yb[:, 1:4].ravel(), Yb[:, 4:7].ravel(), Yb[:, 7:11].ravel()])
        assert np.array_equal(_bits(Ys), _bits(Yc)), name
        Y0, _e0, rc = sec.apply(X, dispersion=D)
        assert rc == 0
        continuous = jumps = 0
        for b in range(B):
            Yb, Y0b, Xo = pt.unpack_y(Yc[b], M), pt.unpack_y(Y0[b], M), pt.unpack_y(X[b, :11 * M], M)
            assert np.array_equal(_bits(Yb[:nn[0] + 1]), _bits(Y0b[:nn[0] + 1])), (name, b)
            assert np.array_equal(_bits(Yb[0]), _bits(Xo[0])), (name, b)
            for s in range(1, S):
                jump = Xo[xa[s]] - Xo[xa[s] - 1]
                z = jump == 0.0
                continuous += int(z.sum())
                jumps += int((~z).sum())
                assert np.array_equal(_bits(Yb[xa[s]][z]), _bits(Yb[xa[s] - 1][z])), (name, b, s)
                assert np.array_equal(_bits(Yb[xa[s]][~z]), _bits((Yb[xa[s] - 1] + jump)[~z])), (name, b, s)
        if name == "example":   # x0: 11 continuous knots; the jettisoned copy: 3 mass drops; the perturbed copy: jumps nearly everywhere
            assert continuous >= 11 * 11 + 11 * 11 - 3 and jumps >= 3 + 100, (continuous, jumps)
        chain.close()
        sec.close()


def test_bits_batch_slab_and_buffers():
    """one vector gives the same y / err alone and at positions 0, 63, 64, 66 of a batch of 67 whose other vectors and factors
    differ; with slabs of 64 vectors (two slabs) as with one; on device buffers as on host buffers"""
    import torch
    from gelato_amd import problem
    prob, E, X3 = _case("example")
    plan = E.propagation_plan(steps=2, restart="chain")
    d1 = dispersion(3, E.S)[1]
    y1, e1, rc = plan.apply(X3[1], dispersion=d1)
    assert rc == 0
    XX = problem.synthetic_batch(X3[0], E.M, 67, seed=99)
    DD = dispersion(67, E.S, seed=11)
    full = plan.info()["slab"]
    assert full >= 128
    results = []
    for slab in (None, "64"):
        if slab:
            os.environ["GEL_PROP_SLAB"] = slab
        try:
            assert plan.info()["slab"] == (64 if slab else full)
            for pos in (0, 63, 64, 66):
                Xp, Dp = XX.copy(), DD.copy()
                Xp[pos], Dp[pos] = X3[1], d1
                Y, err, rc = plan.apply(Xp, dispersion=Dp)
                assert rc == 0
                assert np.array_equal(_bits(Y[pos]), _bits(y1[0])) and np.array_equal(_bits(err[pos]), _bits(e1[0])), (slab, pos)
            results.append(plan.apply(XX, dispersion=DD))
        finally:
            os.environ.pop("GEL_PROP_SLAB", None)
    (Ya, ea, _), (Yb, eb, _) = results
    assert np.array_equal(_bits(Ya), _bits(Yb)) and np.array_equal(_bits(ea), _bits(eb))
    dX, dD = torch.from_numpy(XX).cuda(), torch.from_numpy(DD).cuda()
    dY = torch.full((67, 11 * E.M), -3.0, dtype=torch.float64, device="cuda")
    dE = torch.full((67, E.S, 4), -3.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    plan.apply_device(67, dX.data_ptr(), dY.data_ptr(), dE.data_ptr(), dD.data_ptr())
    assert E.sync() == 0
    assert np.array_equal(_bits(dY.cpu().numpy()), _bits(Ya)) and np.array_equal(_bits(dE.cpu().numpy()), _bits(ea))
    # the undispersed chain: host buffers against device buffers, err optional
    Yu, eu, rc = plan.apply(XX)
    assert rc == 0
    dY.fill_(-3.0)
    torch.cuda.synchronize()
    plan.apply_device(67, dX.data_ptr(), dY.data_ptr())
    assert E.sync() == 0
    assert np.array_equal(_bits(dY.cpu().numpy()), _bits(Yu))
    plan.close()


@pytest.mark.parametrize("what", ["state", "factor"])
def test_status_nan(what):
    """a NaN state at the first node of phase 3 of one vector (its jump into phase 3 is NaN), or a NaN thrust factor of its phase
    3: its phases >= 3 are non-finite, its phases < 3 and the other vectors keep their bits; GEL_NONFINITE; the next call is clean"""
    from gelato_amd import _lib
    prob, E, X = _case("example")
    plan = E.propagation_plan(steps=2, restart="chain")
    D = dispersion(X.shape[0], E.S)
    ok_y, ok_e, rc = plan.apply(X, dispersion=D)
    assert rc == 0 and np.all(np.isfinite(ok_y)) and np.all(np.isfinite(ok_e))
    xa, nn = _knot_rows(E)
    Xb, Db = X.copy(), D.copy()
    if what == "state":
        Xb[1, E.M + 3 * xa[3] + 1] = np.nan       # position y of phase 3's first node
    else:
        assert prob["engine_on"][3]
        Db[1, 3, 0] = np.nan
    Y, err, rc = plan.apply(Xb, dispersion=Db)
    assert rc == _lib.GEL_NONFINITE
    assert np.array_equal(_bits(Y[[0, 2]]), _bits(ok_y[[0, 2]])) and np.array_equal(_bits(err[[0, 2]]), _bits(ok_e[[0, 2]]))
    Yb, Yok = pt.unpack_y(Y[1], E.M), pt.unpack_y(ok_y[1], E.M)
    assert np.array_equal(_bits(Yb[:xa[3]]), _bits(Yok[:xa[3]])) and np.array_equal(_bits(err[1, :3]), _bits(ok_e[1, :3]))
    for s in range(3, E.S):
        rows = slice(xa[s] + (1 if (s == 3 and what == "factor") else 0), xa[s] + nn[s] + 1)
        assert not np.any(np.all(np.isfinite(Yb[rows]), axis=1)), s      # every node's state holds a non-finite value
        assert not np.all(np.isfinite(err[1, s])), s
    again_y, again_e, rc = plan.apply(X, dispersion=D)
    assert rc == 0 and np.array_equal(_bits(again_y), _bits(ok_y)) and np.array_equal(_bits(again_e), _bits(ok_e))
    plan.close()


def test_status_empty_batch():
    prob, E, X = _case("example")
    plan = E.propagation_plan(steps=1, restart="chain")
    Y0, e0, rc = plan.apply(np.zeros((0, E.nvars)), dispersion=np.zeros((0, E.S, 4)))
    assert rc == 0 and Y0.shape == (0, 11 * E.M) and e0.shape == (0, E.S, 4)
    Y0, e0, rc = plan.apply(np.zeros((0, E.nvars)))
    assert rc == 0 and Y0.shape == (0, 11 * E.M)
    plan.apply_device(0, 0, 0, 0, 0)
    assert E.sync() == 0
    plan.close()


@pytest.mark.parametrize("mutate", ["no_jump", "shift_factors", "no_wind_factor"])
def test_bound_rejects_wrong_restatements(mutate):
    """the same bound, around the device's y, rejects: the carry without the jump (on the vector with the mass drops), the factors
    of phase s applied to phase s + 1, the wind factor ignored (f = 2 in the windy phases).  tests/test_flight_cpu.py shows that
    the correct restatement and each of these differ by 1e7 .. 1e12 of 2 E."""
    prob, E, X = _case("example")
    plan = E.propagation_plan(steps=1, restart="chain")
    disp = None if mutate == "no_jump" else ft.teeth_dispersion(E.S)
    Y, _err, rc = plan.apply(X[1], dispersion=disp)
    assert rc == 0
    Yd = pt.unpack_y(Y[0], E.M)
    ry, by, _re, _be = ft.fly_all(E, plan, prob, X[1], disp=disp)
    assert np.all(np.abs(Yd - ry) <= by)
    miss = ft.mutant_miss(E, plan, prob, X[1], disp, mutate, Yd, by)
    print("mutation %s: misses the bound around the device's y by a factor %.3g" % (mutate, miss))
    assert miss > 1.0e3, (mutate, miss)
    plan.close()


def test_fly():
    """x_flown = [y | u | t]; terminal = y - x at the last state node in physical units; the row values are rows_eval(x_flown);
    the step-doubling estimate; B = 3 under dispersions"""
    from gelato_amd import Engine, propagate
    prob, E0, X = _case("example")
    E = Engine(prob)
    M = E.M
    # a small row table: the mass at the last node against a target, the mass burnt, and the radius at the last node
    last = M - 1
    E.rows_configure([(last, 1.0, -1, 0.0, -0.25), (0, 1.0, last, -1.0, 0.0)], [("radius", last, 6378137.0, 1.0)])
    D = dispersion(X.shape[0], E.S)
    out = propagate.fly(X, None, None, steps=1, dispersion=D, engine=E)
    assert out["steps"] == 2 and out["status"] == 0
    plan = E.propagation_plan(steps=2, restart="chain")
    Y, err, rc = plan.apply(X, dispersion=D)
    assert rc == 0
    assert np.array_equal(_bits(out["y"]), _bits(Y)) and np.array_equal(_bits(out["err"]), _bits(err))
    xf = out["x_flown"]
    assert xf.shape == X.shape and np.array_equal(_bits(xf[:, :11 * M]), _bits(Y)) and np.array_equal(_bits(xf[:, 11 * M:]), _bits(X[:, 11 * M:]))
    um, up, uv = [float(v) for v in prob["units"][:3]]
    for b in range(X.shape[0]):
        dy = pt.unpack_y(Y[b], M)[-1] - pt.unpack_y(X[b, :11 * M], M)[-1]
        for key, (a, c), sc in zip(GROUPS, pt.GROUP_COLS, (um, up, uv, 1.0)):
            assert out["terminal"][key].shape == (X.shape[0], c - a)
            assert np.array_equal(out["terminal"][key][b], dy[a:c] * sc), (b, key)
    # the last row of err is the terminal miss in the normalised form: at least the last node's share
    Xl = mt.phase_state(E, X[0], E.S - 1)[0]
    den = 1.0 + np.abs(Xl).max(axis=0)
    t0 = np.abs(pt.unpack_y(Y[0], M)[-1] - Xl[-1]) / den
    assert np.all(err[0, -1] >= np.array([t0[a:c].max() for a, c in pt.GROUP_COLS]))
    con, _j, rc = E.rows_eval(xf, want_jac=False)
    assert rc == 0 and np.array_equal(_bits(out["rows"]), _bits(con))
    assert np.allclose(out["rows"][:, 0], Y[:, last] - 0.25, rtol=0, atol=1e-15)
    # step doubling: the estimate is max |y_1 - y_2| / 15 under err's normalisation
    p1 = E.propagation_plan(steps=1, restart="chain")
    Y1, _e, rc = p1.apply(X, dispersion=D)
    assert rc == 0
    xa, nn = _knot_rows(E)
    s = E.S - 1
    rows = slice(xa[s], xa[s] + nn[s] + 1)
    d = np.abs(pt.unpack_y(Y1[0], M)[rows] - pt.unpack_y(Y[0], M)[rows]).max(axis=0) / den / 15.0
    assert np.allclose(out["integrator"][0, s], [d[a:c].max() for a, c in pt.GROUP_COLS], rtol=1e-15, atol=0)
    assert out["integrator"].shape == (3, E.S, 4) and np.all(np.isfinite(out["integrator"]))
    # without a row table there is no "rows"; an xdict is one vector
    out1 = propagate.fly(E0.split_x(X[0]), None, None, steps=1, engine=E0)
    assert "rows" not in out1 and out1["y"].shape == (1, 11 * M) and out1["status"] == 0
    p1.close()
    plan.close()
    E.close()

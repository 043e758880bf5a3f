"""Explicit RK4 propagation of the sections on the device (gel_propagate*): parity with an independent restatement
under a bound carried along the trajectory (tests/propagate_truth.py), the bound's teeth, truth and order on the manufactured
solution of g24, the bit-exact properties, status, and propagate.shooting_check."""
import os

import numpy as np
import pytest

import propagate_truth as pt
from conftest import load_golden

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
GROUPS = ("mass", "position", "velocity", "quaternion")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _named(name):
    import interp_truth as it
    if name == "long128":
        import states
        return states.long_state([128])
    return it.named(name)


def _engine(prob, **kw):
    from gelato_amd import Engine
    return Engine(prob, **kw)


_CASE = {}


def _case(name):
    """(prob, engine, X [3, nvars]) of a named problem, shared by the tests"""
    if name not in _CASE:
        from gelato_amd import problem
        prob, x0 = _named(name)
        E = _engine(prob)
        _CASE[name] = (prob, E, problem.synthetic_batch(x0, E.M, 3))
    return _CASE[name]


_REF = {}


def _reference(name, k, restart):
    """the restatement of every vector of the case: a list of (y [M, 11], bound_y, err [S, 4], bound_err), computed once"""
    key = (name, k, restart)
    if key not in _REF:
        prob, E, X = _case(name)
        plan = E.propagation_plan(steps=k, restart="node" if restart else "section")
        _REF[key] = [pt.propagate_all(E, plan, prob, X[b], restart=restart) for b in range(X.shape[0])]
        plan.close()
    return _REF[key]


USAGE = {}


@pytest.mark.parametrize("restart", [False, True], ids=["section", "node"])
@pytest.mark.parametrize("name,k", [("example", 1), ("example", 3), ("ragged", 1), ("ragged", 3), ("long128", 1)])
def test_parity_with_restatement(name, k, restart):
    """y and err of the device against numpy RK4 with the oracle's right-hand sides, within 2 E (propagate_truth)"""
    prob, E, X = _case(name)
    plan = E.propagation_plan(steps=k, restart="node" if restart else "section")
    use, worst = check_parity(E, plan, X, _reference(name, k, restart))
    USAGE[(name, k, restart)] = use
    print("bound usage %s k=%d %s: y %s err %s" % (name, k, "node" if restart else "section", np.array2string(use[0], precision=3),
                                                  np.array2string(use[1], precision=3)))
    assert all(wy <= 1.0 and we <= 1.0 for wy, we in worst), (name, k, restart, worst)


def check_parity(E, plan, X, reference):
    """the plan applied to X [B, nvars] against the restatement's (y, bound_y, err, bound_err) per vector -> (usage [2, 4] of the
    bounds per group, [(worst y usage, worst err usage)] per vector: the caller asserts them <= 1)"""
    Y, err, rc = plan.apply(X)
    assert rc == 0
    use = np.zeros((2, 4))
    worst = []
    for b, (ry, by, re, be) in enumerate(reference):
        gy = np.abs(pt.unpack_y(Y[b], E.M) - ry)
        ge = np.abs(err[b] - re)
        with np.errstate(divide="ignore", invalid="ignore"):
            sy = np.where(by > 0, gy / by, np.where(gy == 0, 0.0, np.inf))
            se = np.where(be > 0, ge / be, np.where(ge == 0, 0.0, np.inf))
        for g, (a, c) in enumerate(pt.GROUP_COLS):
            use[0, g] = max(use[0, g], float(sy[:, a:c].max()))
            use[1, g] = max(use[1, g], float(se[:, g].max()))
        worst.append((float(sy.max()), float(se.max())))
    return use, worst


@pytest.mark.parametrize("mutate", ["no_unit_t", "hold_control", "equal_steps"])
def test_bound_rejects_wrong_restatements(mutate):
    """the same bound, around the device's y, rejects: S without unit_t, the control held at the left node's value through an
    interval (the example's u varies), n k equal steps across the section (compared at the last node, where both arrive)"""
    prob, E, X = _case("example")
    k = 3
    plan = E.propagation_plan(steps=k)
    Y, _err, rc = plan.apply(X[0])
    assert rc == 0
    Yd = pt.unpack_y(Y[0], E.M)
    _ry, by, _re, _be = _reference("example", k, False)[0]
    nn = [int(v) for v in E.num_nodes]
    worst, r0 = 0.0, 0
    for s, n in enumerate(nn):
        if mutate == "hold_control" and prob["attitude_hold"][s]:
            r0 += n + 1
            continue
        wrong = pt.propagate_phase(E, plan, prob, X[0], s, want_bound=False, mutate=mutate)["y"]
        rows = slice(r0, r0 + n + 1)
        d = np.abs(wrong - Yd[rows])
        ok = np.isfinite(d) & (by[rows] > 0)
        worst = max(worst, float((d[ok] / by[rows][ok]).max()))
        r0 += n + 1
    print("mutation %s: misses the bound by a factor %.3g" % (mutate, worst))
    assert worst > 1.0e3, (mutate, worst)


_G24 = {}


def _g24_err(case, n, k):
    """device err [4] of g24 (its x holds the DOP853 truth at the nodes: err is RK4's own error), cached"""
    if (case, n, k) not in _G24:
        g = load_golden("g24_mesh_truth.npz")
        prob, x = pt.g24_case(g, case, n)
        E = _engine(prob)
        plan = E.propagation_plan(steps=k)
        _Y, err, rc = plan.apply(x)
        assert rc == 0
        _G24[(case, n, k)] = err[0, 0].copy()
        plan.close()
        E.close()
    return _G24[(case, n, k)]


def test_truth_and_order_on_g24():
    """NoAir, powered, free attitude: halving the step divides the position, velocity and quaternion errors by 15 .. 18 (fourth
    order); at n = 8, k = 16 every group is below 2e-11; the mass error is rounding.  (The aerodynamic case is held to parity
    only: its table kinks break the order.)"""
    for n in (3, 5, 8):
        for k in (1, 2, 4):
            a, b = _g24_err("noair", n, k), _g24_err("noair", n, 2 * k)
            print("g24 noair n=%d k=%d -> %d: ratios %s" % (n, k, 2 * k, np.array2string(a[1:] / b[1:], precision=3)))
            for g in (1, 2, 3):
                assert 15.0 <= a[g] / b[g] <= 18.0, (n, k, g, float(a[g]), float(b[g]))
            assert a[0] <= (2 * n * k + 4) * U, (n, k, float(a[0]))
    e = _g24_err("noair", 8, 16)
    print("g24 noair n=8 k=16:", e)
    assert np.all(e <= 2e-11), e


@pytest.mark.parametrize("n,k", [(5, 2), (8, 4)])
def test_parity_on_g24_air(n, k):
    g = load_golden("g24_mesh_truth.npz")
    prob, x = pt.g24_case(g, "air", n)
    E = _engine(prob)
    plan = E.propagation_plan(steps=k)
    Y, err, rc = plan.apply(x)
    assert rc == 0
    ry, by, re, be = pt.propagate_all(E, plan, prob, x)
    gy, ge = np.abs(pt.unpack_y(Y[0], E.M) - ry), np.abs(err[0] - re)
    assert np.all(gy <= by), float((gy[by > 0] / by[by > 0]).max())
    assert np.all(ge <= be), float((ge / be).max())


def test_exact_bits():
    """node xa of every phase is x's; quaternions of hold-type phases and masses of engine-off phases keep X_0's bits at every
    node; the first interval is the same in both restart modes"""
    for name in ("example", "ragged"):
        prob, E, X = _case(name)
        M = E.M
        sec, node = E.propagation_plan(steps=3), E.propagation_plan(steps=3, restart="node")
        Ys, es, rc = sec.apply(X)
        Yn, en, rc2 = node.apply(X)
        assert rc == 0 and rc2 == 0
        nn = [int(v) for v in E.num_nodes]
        for b in range(X.shape[0]):
            Xs = pt.unpack_y(X[b, :11 * M], M)
            A, Bn = pt.unpack_y(Ys[b], M), pt.unpack_y(Yn[b], M)
            xa = 0
            for s, n in enumerate(nn):
                for Yv in (A, Bn):
                    assert np.array_equal(_bits(Yv[xa]), _bits(Xs[xa])), (name, b, s)
                assert np.array_equal(_bits(A[xa + 1]), _bits(Bn[xa + 1])), (name, b, s)
                if prob["attitude_hold"][s]:
                    assert np.array_equal(_bits(A[xa:xa + n + 1, 7:]), _bits(np.tile(Xs[xa, 7:], (n + 1, 1)))), (name, b, s)
                    assert np.array_equal(_bits(Bn[xa + 1:xa + n + 1, 7:]), _bits(Xs[xa:xa + n, 7:])), (name, b, s)
                if not prob["engine_on"][s]:
                    assert np.array_equal(_bits(A[xa:xa + n + 1, 0]), _bits(np.full(n + 1, Xs[xa, 0]))), (name, b, s)
                    assert np.array_equal(_bits(Bn[xa + 1:xa + n + 1, 0]), _bits(Xs[xa:xa + n, 0])), (name, b, s)
                xa += n + 1


@pytest.mark.parametrize("restart", ["section", "node"])
def test_batch_slab_and_stream_invariance(restart):
    """one vector gives the same y / err alone and at positions 0, 63, 64, 66 of a batch of 67 whose other vectors differ; with
    slabs of 64 vectors (two slabs) as with one; on device buffers as on host buffers, also for a caller on a non-blocking stream"""
    import torch
    from gelato_amd import problem
    prob, E, X3 = _case("example")
    plan = E.propagation_plan(steps=2, restart=restart)
    y1, e1, rc = plan.apply(X3[1])
    assert rc == 0
    XX = problem.synthetic_batch(X3[0], E.M, 67, seed=99)
    full = plan.info()["slab"]
    assert full >= 128
    results = []
    for slab in (None, "64"):
        if slab:
            os.environ["GEL_PROP_SLAB"] = slab
        try:
            assert plan.info()["slab"] == (64 if slab else full)
            for pos in (0, 63, 64, 66):
                Xp = XX.copy()
                Xp[pos] = X3[1]
                Y, err, rc = plan.apply(Xp)
                assert rc == 0
                assert np.array_equal(_bits(Y[pos]), _bits(y1[0])) and np.array_equal(_bits(err[pos]), _bits(e1[0])), (slab, pos)
            results.append(plan.apply(XX))
        finally:
            os.environ.pop("GEL_PROP_SLAB", None)
    (Ya, ea, _), (Yb, eb, _) = results
    assert np.array_equal(_bits(Ya), _bits(Yb)) and np.array_equal(_bits(ea), _bits(eb))
    # device buffers (the engine's own stream): from torch's default stream, then for a caller that works on a non-blocking stream
    # of its own -- it finishes writing d_x before the call and consumes the outputs after Engine.sync()
    side = torch.cuda.Stream()
    for caller in (None, side):
        with torch.cuda.stream(caller):
            dX = torch.from_numpy(XX).cuda()
            dY = torch.full((67, 11 * E.M), -3.0, dtype=torch.float64, device="cuda")
            dE = torch.full((67, E.S, 4), -3.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        plan.apply_device(67, dX.data_ptr(), dY.data_ptr(), dE.data_ptr())
        assert E.sync() == 0
        with torch.cuda.stream(caller):
            Yd, ed = dY.cpu().numpy(), dE.cpu().numpy()
        assert np.array_equal(_bits(Yd), _bits(Ya)) and np.array_equal(_bits(ed), _bits(ea))
    # err is optional
    dY = torch.full((67, 11 * E.M), -3.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    plan.apply_device(67, dX.data_ptr(), dY.data_ptr(), 0)
    assert E.sync() == 0
    assert np.array_equal(_bits(dY.cpu().numpy()), _bits(Ya))
    Yq, eq, rc = plan.apply(XX, want_err=False)
    assert rc == 0 and eq is None and np.array_equal(_bits(Yq), _bits(Ya))


def test_status_nan_and_empty_batch():
    from gelato_amd import _lib
    prob, E, X = _case("example")
    plan = E.propagation_plan(steps=2)
    ok_y, ok_e, rc = plan.apply(X)
    assert rc == 0 and np.all(np.isfinite(ok_y)) and np.all(np.isfinite(ok_e))
    Xb = X.copy()
    xa1 = int(E.num_nodes[0]) + 1         # first state node of phase 1: the state its section starts from
    Xb[1, E.M + 3 * xa1 + 1] = np.nan     # its position y (a NaN at an interior node reaches err only: y starts from X_0)
    Y, err, rc = plan.apply(Xb)
    assert rc == _lib.GEL_NONFINITE
    assert np.array_equal(_bits(Y[[0, 2]]), _bits(ok_y[[0, 2]])) and np.array_equal(_bits(err[[0, 2]]), _bits(ok_e[[0, 2]]))
    assert not np.all(np.isfinite(Y[1])) and not np.all(np.isfinite(err[1]))
    again_y, again_e, rc = plan.apply(X)
    assert rc == 0 and np.array_equal(_bits(again_y), _bits(ok_y)) and np.array_equal(_bits(again_e), _bits(ok_e))
    # B = 0 is valid
    Y0, e0, rc = plan.apply(np.zeros((0, E.nvars)))
    assert rc == 0 and Y0.shape == (0, 11 * E.M) and e0.shape == (0, E.S, 4)
    plan.apply_device(0, 0, 0, 0)
    assert E.sync() == 0


def test_status_mass_reaches_zero():
    """a massflow so large that one vector's mass is exactly zero at the middle stages of a section's first step: 1 / m is an
    Inf, not a fault -- the call returns with the flag set, the other vectors keep their bits, the next call is clean"""
    from gelato_amd import _lib
    prob0, E0, X = _case("example")
    s = next(i for i in range(E0.S) if prob0["engine_on"][i] and not prob0["attitude_hold"][i])
    prob = dict(prob0)
    um, ut = float(prob["units"][0]), float(prob["units"][4])
    prob["massflow"] = np.array(prob["massflow"], dtype=float)
    prob["massflow"][s] = um                         # -massflow / unit_mass = -1 exactly
    E = _engine(prob)
    k = 2
    plan = E.propagation_plan(steps=k)
    ok_y, ok_e, rc = plan.apply(X)
    assert rc == 0
    nn = [int(v) for v in E.num_nodes]
    xa = sum(nn[:s]) + s
    Xz = X.copy()
    t = Xz[1, 11 * E.M + 2 * E.N:]
    S = (t[s + 1] - t[s]) * ut / 2.0
    h = (E.tau(s)[0] - (-1.0)) / k
    Xz[1, xa] = (S * h) * 0.5                        # fma(Sh / 2, k1 = -1, m) = 0 at the step's second and third stage
    assert Xz[1, xa] > 0
    Y, err, rc = plan.apply(Xz)
    assert rc == _lib.GEL_NONFINITE
    assert np.array_equal(_bits(Y[[0, 2]]), _bits(ok_y[[0, 2]])) and np.array_equal(_bits(err[[0, 2]]), _bits(ok_e[[0, 2]]))
    Yz = pt.unpack_y(Y[1], E.M)
    assert not np.all(np.isfinite(Yz[xa + 1, 4:7]))
    other = np.ones(E.M, dtype=bool)
    other[xa:xa + nn[s] + 1] = False
    assert np.array_equal(_bits(Yz[other]), _bits(pt.unpack_y(ok_y[1], E.M)[other]))   # the vector's other sections are untouched
    again_y, _e, rc = plan.apply(X)
    assert rc == 0 and np.array_equal(_bits(again_y), _bits(ok_y))


def test_shooting_check():
    from gelato_amd import problem, propagate
    g = load_golden("g24_mesh_truth.npz")
    prob, x = pt.g24_case(g, "noair", 8)
    E = _engine(prob)
    rep = propagate.shooting_check(E.split_x(x), {"num_sections": 1, "params": [{"name": "g24"}]}, None, steps=2, engine=E)
    assert len(rep) == 1 and rep[0]["steps"] == 4 and rep[0]["num_nodes"] == 8
    true = _g24_err("noair", 8, 4)
    for g_i, key in enumerate(GROUPS):
        assert rep[0][key] == true[g_i]
    for key in GROUPS[1:]:
        r = rep[0]["integrator_groups"][key] / rep[0][key]
        print("shooting_check g24 %s: step-doubling estimate / true error = %.3f" % (key, r))
        assert 0.5 <= r <= 2.0, (key, r)
    assert 0.5 <= rep[0]["integrator"] / rep[0]["max"] <= 2.0
    pdict, unitdict, _c, xdict = problem.make_problem("example")
    rep = propagate.shooting_check(xdict, pdict, unitdict, steps=2)
    assert len(rep) == 12
    for rec in rep:
        assert all(np.isfinite(rec[key]) for key in GROUPS + ("max", "integrator")), rec

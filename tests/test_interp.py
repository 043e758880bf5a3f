"""Spectral interpolation on the device (gel_interp*): the kernel against the host form bit for bit (fewer points
than lanes, several point tiles with a partial last one, n on both sides of the wavefront width, a tail group of vectors, the
n = 128 slice that decides the vectors per workgroup), batch invariance, the resident form, status, and a refined problem that
evaluates."""
import os

import numpy as np
import pytest

import interp_truth as it
from interp_truth import LD, U

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _batch(x0, M, B):
    from gelato_amd import problem
    X = problem.synthetic_batch(x0, M, min(B, 5))
    return np.tile(X, (B // X.shape[0] + 1, 1))[:B].copy()


@pytest.fixture(scope="module")
def cases():
    """name -> (device engine, destination engine (host-only), x0), built once"""
    out = {}
    for name in ("example", "mixed-6x64", "stress-12x128", "ragged"):
        prob, x0 = it.named(name)
        E = it.engine(prob, device=0)
        nn = [int(v) for v in E.num_nodes]
        out[name] = (E, it.engine(it.with_nodes(prob, it.targets(name, nn))), x0)
    return out


@pytest.mark.parametrize("name", ["example", "mixed-6x64", "stress-12x128", "ragged"])
@pytest.mark.parametrize("B", [1, 3, 37])
def test_device_equals_host_transfer(cases, name, B):
    E, Ed, x0 = cases[name]
    X = _batch(x0, E.M, B)
    plan = E.transfer_plan(Ed)
    assert plan.info()["vb"] == 4      # 13 n + 11 doubles per vector: 53.6 KB at n = 128 with four vectors
    host, rch = plan.apply_host(X)
    dev, rcd = plan.apply(X)
    assert rch == 0 and rcd == 0
    assert np.array_equal(_bits(dev), _bits(host)), (name, B, int((_bits(dev) != _bits(host)).sum()))
    plan.close()


@pytest.mark.parametrize("B", [1, 3, 37])
def test_device_equals_host_table(cases, B):
    """600 points in one phase (three point tiles, the last partial), 1 in another, 0 in a third"""
    E, _Ed, x0 = cases["mixed-6x64"]
    rng = np.random.default_rng(11)
    pts = [np.sort(np.concatenate([[-1.0, 1.0], E.tau(0)[:5], rng.uniform(-1, 1, 593)])), np.array([0.3]), np.zeros(0),
           np.linspace(-1, 1, 70), np.array([1.0, -1.0]), rng.uniform(-1, 1, 257)]
    X = _batch(x0, E.M, B)
    plan = E.interp_plan(pts)
    host, rch = plan.apply_host(X)
    dev, rcd = plan.apply(X)
    assert rch == 0 and rcd == 0 and dev.shape == (B, 600 + 1 + 70 + 2 + 257, 14)
    assert np.array_equal(_bits(dev), _bits(host))
    assert np.array_equal(_bits(dev[0, :, 0]), _bits(it.table_times(pts, E, X[0])))
    plan.close()


def test_unit_quat_device_against_host(cases):
    """with the flag the device's division and square root are held to test 7's bound, 6 u |q| against q_lin / |q_lin| in
    longdouble (q_lin: the same plan without the flag); everything else is the host's bits"""
    E, Ed, x0 = cases["example"]
    X = _batch(x0, E.M, 3)
    lin, _rc = E.transfer_plan(Ed).apply(X)
    plan = E.transfer_plan(Ed, unit_quat=True)
    dev, rc = plan.apply(X)
    host, rch = plan.apply_host(X)
    assert rc == 0 and rch == 0
    qs = it.quat_slice(Ed)
    other = np.ones(Ed.nvars, dtype=bool)
    other[qs] = False
    assert np.array_equal(_bits(dev[:, other]), _bits(host[:, other]))
    cpx = np.concatenate([plan.matrices(s)["copy_x"] >= 0 for s in range(E.S)])
    qd, ql = dev[:, qs].reshape(3, -1, 4), lin[:, qs].reshape(3, -1, 4)
    assert np.array_equal(_bits(qd[:, cpx]), _bits(ql[:, cpx]))
    qL = ql.astype(LD)
    ref = qL / np.sqrt((qL * qL).sum(axis=2, keepdims=True))
    assert np.all(np.abs(qd.astype(LD) - ref).astype(float)[:, ~cpx] <= 6 * U * np.abs(ref[:, ~cpx]).astype(float))


def test_batch_invariance(cases):
    """vector k's bits at B = 1, anywhere inside B = 37, and for 1, 2 and 4 vectors per workgroup; a repeated call into poisoned
    output gives the same bits"""
    E, Ed, x0 = cases["mixed-6x64"]
    plan = E.transfer_plan(Ed)
    X = _batch(x0, E.M, 37)
    x = X[3].copy()
    ref, rc = plan.apply(x)
    assert rc == 0
    old = os.environ.get("GEL_INTERP_VB")
    try:
        for vb in (1, 2, 4):
            os.environ["GEL_INTERP_VB"] = str(vb)
            assert plan.info()["vb"] == vb
            for pos in (0, 18, 35, 36):
                XX = X.copy()
                XX[pos] = x
                out, rc = plan.apply(XX)
                assert rc == 0 and np.array_equal(_bits(out[pos]), _bits(ref[0])), (vb, pos)
        os.environ["GEL_INTERP_VB"] = "3"      # not a form: ignored
        assert plan.info()["vb"] == 4
    finally:
        if old is None:
            os.environ.pop("GEL_INTERP_VB", None)
        else:
            os.environ["GEL_INTERP_VB"] = old
    import torch
    dX = torch.from_numpy(X).cuda()
    first = None
    for _ in range(2):
        dO = torch.full((37, Ed.nvars), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        plan.apply_resident(37, dX.data_ptr(), dO.data_ptr())
        assert E.sync() == 0
        got = dO.cpu().numpy()
        first = got if first is None else first
        assert np.array_equal(_bits(got), _bits(first))
    assert np.array_equal(_bits(first[3]), _bits(ref[0]))


@pytest.mark.parametrize("mode", ["transfer", "table"])
def test_resident_form(cases, mode):
    """device tensors in and out; the B rows are the host-buffer form's, the two rows behind them keep the poison"""
    import torch
    E, Ed, x0 = cases["example"]
    B = 7
    X = _batch(x0, E.M, B)
    plan = E.transfer_plan(Ed) if mode == "transfer" else E.interp_plan([np.linspace(-1, 1, 5 + s) for s in range(E.S)])
    want, rc = plan.apply(X)
    assert rc == 0
    w = plan.out_doubles
    dX = torch.from_numpy(X).cuda()
    dO = torch.full((B + 2, w), -7.25, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    plan.apply_resident(B, dX.data_ptr(), dO.data_ptr())
    assert E.sync() == 0
    got = dO.cpu().numpy()
    assert np.array_equal(_bits(got[:B]), _bits(want.reshape(B, w)))
    assert np.all(got[B:] == -7.25)
    plan.apply_resident(0, dX.data_ptr(), dO.data_ptr())      # B = 0: nothing is launched
    assert E.sync() == 0


def test_status_nonfinite(cases):
    import torch
    from gelato_amd import _lib
    E, Ed, x0 = cases["example"]
    plan = E.transfer_plan(Ed)
    X = _batch(x0, E.M, 5)
    ok, rc = plan.apply(X)
    assert rc == 0 and np.all(np.isfinite(ok))
    Xb = X.copy()
    Xb[2, E.M + 7] = np.nan
    out, rc = plan.apply(Xb)
    assert rc == _lib.GEL_NONFINITE
    keep = [0, 1, 3, 4]
    assert np.array_equal(_bits(out[keep]), _bits(ok[keep])) and not np.all(np.isfinite(out[2]))
    again, rc = plan.apply(X)
    assert rc == 0 and np.array_equal(_bits(again), _bits(ok))
    dX = torch.from_numpy(Xb).cuda()
    dO = torch.empty((5, Ed.nvars), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    plan.apply_resident(5, dX.data_ptr(), dO.data_ptr())
    assert E.sync() == _lib.GEL_NONFINITE
    assert np.array_equal(_bits(dO.cpu().numpy()[keep]), _bits(ok[keep]))
    assert E.sync() == 0
    dX.copy_(torch.from_numpy(X))
    torch.cuda.synchronize()
    plan.apply_resident(5, dX.data_ptr(), dO.data_ptr())
    assert E.sync() == 0 and np.array_equal(_bits(dO.cpu().numpy()), _bits(ok))


def test_refined_problem_lives():
    """estimate -> suggestion -> refined problem -> warm start: the constraint mirrors build on (xdict_new, pdict_new), the linear
    knot and initial rows read copied nodes only and keep their bits, and the residual and the estimate of the transferred
    vector on the new mesh are finite"""
    from gelato_amd import Engine, con_dynamics, con_init_terminal_knot as citk, interp, pack_x, problem
    from gelato_amd.mesh_error import collocation_error, suggest_num_nodes
    pdict, unitdict, condition, xdict = problem.make_problem("example")
    rep = collocation_error(xdict, pdict, unitdict)
    errs = sorted(r["max"] for r in rep)
    tol = float(np.sqrt(errs[len(errs) // 2 - 1] * errs[len(errs) // 2]))      # between two sections' errors: some kept, some raised
    sug = suggest_num_nodes(rep, tol, 40)
    acts = {r["action"] for r in sug}
    assert "kept" in acts and ("raised" in acts or "capped" in acts) and any(r["suggested"] > r["num_nodes"] for r in sug)
    xn, pn = interp.refine(xdict, pdict, unitdict, sug)
    for fn in (citk.equality_knot_LGR, citk.equality_init):
        a, b = fn(xdict, pdict, unitdict, condition), fn(xn, pn, unitdict, condition)
        assert np.array_equal(_bits(a), _bits(b)), fn.__name__
    ps = pn["ps_params"]
    S = pn["num_sections"]
    E = Engine(con_dynamics.problem_arrays(pn, unitdict), D=[ps.D(i) for i in range(S)], tau=[ps.tau(i) for i in range(S)])
    x = pack_x(xn)
    res, rc = E.eval_residual(x)
    assert rc == 0 and np.all(np.isfinite(res))
    err, _d, rc = E.mesh_error(x)
    assert rc == 0 and np.all(np.isfinite(err))


def test_slice_that_does_not_fit_is_refused_on_the_device_only():
    """13 n + 11 doubles of one vector must fit 64 KB of LDS: n = 629 plans with one vector per workgroup and matches the host
    form, n = 630 is refused when the plan is created; a host-only handle has no such limit"""
    from gelato_amd import _lib
    for n, fits in ((629, True), (630, False)):
        prob = it.prob_of([n, 3])
        E, Ed = it.engine(prob, device=0), it.engine(it.with_nodes(prob, [n + 1, 3]))
        if not fits:
            with pytest.raises(_lib.GelatoAmdError):
                E.transfer_plan(Ed)
            H = it.engine(prob)
            out, rc = H.transfer_plan(Ed).apply_host(it.random_x(H, 3))
            assert rc == 0 and np.all(np.isfinite(out))
            continue
        plan = E.transfer_plan(Ed)
        assert plan.info()["vb"] == 1
        X = np.stack([it.random_x(E, s) for s in range(2)])
        dev, rc = plan.apply(X)
        host, rch = plan.apply_host(X)
        assert rc == 0 and rch == 0 and np.array_equal(_bits(dev), _bits(host))

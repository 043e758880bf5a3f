"""Collocation error estimate on the device (gel_mesh_error*): parity with an independent restatement
(tests/mesh_truth.py: numpy products, the oracle's right-hand sides, a bound derived from the arithmetic), convergence on a
manufactured solution (g24), exact cases, batch invariance and status."""
import numpy as np
import pytest

import mesh_truth as mt
from conftest import load_golden

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


def _named(name):
    from gelato_amd import con_dynamics, pack_x, problem
    if name == "ragged":
        import states
        return states.ragged_state()
    pdict, unitdict, _c, xdict = problem.make_problem(name)
    return dict(con_dynamics.problem_arrays(pdict, unitdict)), pack_x(xdict)


def _engine(prob, **kw):
    from gelato_amd import Engine
    return Engine(prob, **kw)


USAGE = {}


def check_parity(E, prob, X, name):
    """gel_mesh_error of X [B, nvars] against the restatement, within its bound -> the bound's usage [2, 4]"""
    err, diff, rc = E.mesh_error(X, want_diff=True)
    assert rc == 0
    use = np.zeros((2, 4))
    for b in range(X.shape[0]):
        re, rd, be, bd = mt.estimate_all(E, prob, X[b])
        ge = np.abs(err[b] - re)
        gd = np.abs(diff[b] - rd)
        assert np.all(ge <= be), (name, b, float((ge / be).max()))
        assert np.all(gd <= bd), (name, b, float((gd / bd).max()))
        for g, (a, c) in enumerate(mt.GROUP_COLS):
            use[0, g] = max(use[0, g], float((ge / be)[:, g].max()))
            use[1, g] = max(use[1, g], float((gd / bd)[:, a:c].max()))
    return use


@pytest.mark.parametrize("name", ["example", "mixed-6x64", "stress-12x128", "ragged"])
def test_parity_with_restatement(name):
    from gelato_amd import problem
    prob, x0 = _named(name)
    E = _engine(prob)
    X = problem.synthetic_batch(x0, E.M, 3)
    use = USAGE[name] = check_parity(E, prob, X, name)
    print("bound usage %s: err %s diff %s" % (name, np.array2string(use[0], precision=3), np.array2string(use[1], precision=3)))


def _g24_case(g, case, n):
    prob = {k[len("prob_%s_" % case):]: g[k] for k in g if k.startswith("prob_%s_" % case)}
    prob["num_nodes"] = np.array([n], dtype=np.int32)
    return prob, g["x_%s_%d" % (case, n)], g["true_%s_%d" % (case, n)]


def test_convergence_manufactured_noair():
    """NoAir, powered, free attitude, constant control: the estimate falls monotonically with n, reaches 1e-10 within the listed
    n, and stays within a factor of 100 of the true interpolation error while that exceeds 1e-11"""
    g = load_golden("g24_mesh_truth.npz")
    est, ratios = [], []
    for n in [int(v) for v in g["ns"]]:
        prob, x, true = _g24_case(g, "noair", n)
        E = _engine(prob)
        err, _d, rc = E.mesh_error(x)
        assert rc == 0
        m = E.mesh_matrices(0)
        X, _u, _to, _tf = mt.phase_state(E, x, 0)
        Xt = m["Lx"] @ X
        mx = np.maximum(np.abs(Xt).max(axis=0), np.abs(X[0]))
        et = np.abs(true[1:] - Xt).max(axis=0) / (1.0 + mx)
        e_true = max(et[a:b].max() for a, b in mt.GROUP_COLS)
        e = float(err[0, 0].max())
        est.append(e)
        if e_true > 1e-11:
            ratios.append(e / e_true)
            assert 1e-2 <= e / e_true <= 1e2, (n, e, e_true)
    print("noair estimate by n:", ["%.3e" % v for v in est], "estimate / true:", ["%.3f" % r for r in ratios])
    assert all(b < a for a, b in zip(est, est[1:])), est
    assert min(est) <= 1e-10
    assert len(ratios) >= 3


def test_convergence_air_across_table_knots():
    """an aerodynamic section crossing a wind-table knot and CA-table knots: the right-hand side is piecewise smooth, the
    decrease only algebraic -- but the estimate still falls with n"""
    g = load_golden("g24_mesh_truth.npz")
    est = []
    for n in [int(v) for v in g["ns"]]:
        prob, x, _true = _g24_case(g, "air", n)
        err, _d, rc = _engine(prob).mesh_error(x)
        assert rc == 0
        est.append(float(err[0, 0].max()))
    print("air estimate by n:", ["%.3e" % v for v in est])
    assert all(b < a for a, b in zip(est, est[1:])), est
    assert est[-1] > 1e-9   # algebraic, not spectral: far above the smooth case at the same n


def test_exact_cases():
    """mass of a powered phase exactly linear at the phase's mf_um slope; mass of a coast phase and quaternion of a hold phase
    constant: the group error is rounding, below 4 (n + 3) u (sum |Lx| |X| + |X_0| + S sum |I| |F|) / (1 + max |X~|)"""
    import states
    prob, x = states.ragged_state()
    E = _engine(prob)
    nn = [int(v) for v in E.num_nodes]
    M, N = E.M, E.N
    x = x.copy()
    um, ut = float(prob["units"][0]), float(prob["units"][4])
    t = x[11 * M + 2 * N:]
    cases = []
    for s, n in enumerate(nn):
        ua = sum(nn[:s])
        xa = ua + s
        tau = np.concatenate([[-1.0], E.tau(s)])
        S = (t[s + 1] - t[s]) * ut / 2.0
        if prob["engine_on"][s]:
            mf = -float(prob["massflow"][s]) / um
            x[xa:xa + n + 1] = x[xa] + S * mf * (tau + 1.0)
            cases.append((s, 0))
        else:
            x[xa:xa + n + 1] = x[xa]
            cases.append((s, 0))
        if prob["attitude_hold"][s]:
            q = x[7 * M:11 * M].reshape(-1, 4)
            q[xa + 1:xa + n + 1] = q[xa]
            cases.append((s, 3))
    err, _d, rc = E.mesh_error(x)
    assert rc == 0
    for s, g in cases:
        n = nn[s]
        m = E.mesh_matrices(s)
        X, _u, to, tf = mt.phase_state(E, x, s)
        S = (tf - to) * ut / 2.0
        a, b = mt.GROUP_COLS[g]
        F = np.full(n + 1, (-float(prob["massflow"][s]) / um) if (g == 0 and prob["engine_on"][s]) else 0.0)
        Xt = m["Lx"] @ X[:, a:b]
        sc = np.abs(m["Lx"]) @ np.abs(X[:, a:b]) + np.abs(X[0, a:b]) + S * (np.abs(m["I"]) @ np.abs(F))[:, None]
        bound = (4 * (n + 3) * U * sc / (1.0 + np.maximum(np.abs(Xt).max(axis=0), np.abs(X[0, a:b])))).max()
        assert err[0, s, g] <= bound, (s, g, float(err[0, s, g]), float(bound))


def test_batch_invariance_and_entry_points():
    import torch
    from gelato_amd import problem
    prob, x0 = _named("example")
    E = _engine(prob)
    X = problem.synthetic_batch(x0, E.M, 7)
    ref, _d, rc = E.mesh_error(X[3])
    assert rc == 0
    for B in (1, 3, 4097):
        XX = np.tile(X, (B // 7 + 1, 1))[:B].copy()
        for pos in sorted({0, B // 2, B - 1}):
            XX[pos] = X[3]
            err, _d, rc = E.mesh_error(XX)
            assert rc == 0
            assert np.array_equal(err[pos], ref[0]), (B, pos)
    # host and device entry points, with and without the differences
    B = 4097
    XX = np.tile(X, (B // 7 + 1, 1))[:B].copy()
    eh, dh, rc = E.mesh_error(XX, want_diff=True)
    assert rc == 0
    en, _n, rc = E.mesh_error(XX)
    assert np.array_equal(eh, en)
    dX = torch.from_numpy(XX).cuda()
    de = torch.empty((B, E.S, 4), dtype=torch.float64, device="cuda")
    dd = torch.empty((B, E.mesh_npts(), 11), dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    E.mesh_error_device(B, dX.data_ptr(), de.data_ptr(), dd.data_ptr(), s)
    assert E.sync(s) == 0
    assert np.array_equal(de.cpu().numpy(), eh) and np.array_equal(dd.cpu().numpy(), dh)
    de2 = torch.empty_like(de)
    E.mesh_error_device(B, dX.data_ptr(), de2.data_ptr(), 0, s)
    assert E.sync(s) == 0
    assert np.array_equal(de2.cpu().numpy(), eh)


def test_status_nonfinite_and_host_only():
    from gelato_amd import _lib, problem
    prob, x0 = _named("example")
    E = _engine(prob)
    X = problem.synthetic_batch(x0, E.M, 5)
    ok, _d, rc = E.mesh_error(X)
    assert rc == 0 and np.all(np.isfinite(ok))
    Xb = X.copy()
    Xb[2, E.M + 7] = np.nan
    err, _d, rc = E.mesh_error(Xb)
    assert rc == _lib.GEL_NONFINITE
    keep = [0, 1, 3, 4]
    assert np.array_equal(err[keep], ok[keep])
    assert not np.all(np.isfinite(err[2]))
    # the status is cleared: the next clean call reports ok again
    again, _d, rc = E.mesh_error(X)
    assert rc == 0 and np.array_equal(again, ok)
    H = _engine(prob, device=-1)
    with pytest.raises(_lib.GelatoAmdError):
        H.mesh_error(X)

"""Explicit propagation, host side (no GPU; host-only handles): the plan's stage points, copy marks and control
matrix, the refusals, the argument checks, and the restatement of tests/propagate_truth.py against the DOP853 truth of g24 -- the
numbers the device test asserts, pinned where no GPU is needed."""
import numpy as np
import pytest

import interp_truth as it
import propagate_truth as pt
from conftest import load_golden
from interp_truth import LD, U, gamma


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


NODES = [2, 3, 16, 64]
STEPS = [1, 3, 4, 2]


def test_stage_points_copies_and_info():
    E = it.engine(it.prob_of(NODES))
    plan = E.propagation_plan(steps=STEPS)
    info = plan.info()
    assert info["S"] == 4 and info["flags"] == 0
    assert info["stage_points"] == sum(2 * k * n + 1 for n, k in zip(NODES, STEPS))
    assert info["lane_steps"] == max(k * n for n, k in zip(NODES, STEPS))
    hold = [bool(h) for h in E.prob["attitude_hold"]]
    assert info["workspace_bytes_per_vector"] == 16 * sum(2 * k * n + 1 for n, k, h in zip(NODES, STEPS, hold) if not h)
    assert info["slab"] >= 64 and info["slab"] % 64 == 0
    node_plan = E.propagation_plan(steps=STEPS, restart="node")
    assert node_plan.info()["flags"] == 1 and node_plan.info()["lane_steps"] == max(STEPS)
    for s, (n, k) in enumerate(zip(NODES, STEPS)):
        m = plan.matrices(s)
        tau = E.tau(s)
        tx = np.concatenate([[-1.0], tau])
        assert m["pts"].shape == (2 * k * n + 1,) and m["Wu"].shape == (2 * k * n + 1, n)
        # the definition, in extended precision (the library rounds it once: within one ulp of 1)
        j, q = np.divmod(np.arange(2 * k * n), 2 * k)
        want = tx[j].astype(LD) + (tx[j + 1].astype(LD) - tx[j].astype(LD)) * q.astype(LD) / LD(2 * k)
        assert np.all(np.abs(m["pts"][:-1].astype(LD) - want) <= 2.0 ** -52)
        assert np.all(np.diff(m["pts"]) > 0)
        # nodes are hit exactly
        assert np.array_equal(_bits(m["pts"][::2 * k]), _bits(tx))
        # copy_u marks exactly the collocation nodes (the first stage point, -1, is no collocation node)
        want_c = np.full(2 * k * n + 1, -1, dtype=np.int32)
        want_c[2 * k::2 * k] = np.arange(n)
        assert np.array_equal(m["copy_u"], want_c)
        assert np.array_equal(m["Wu"][want_c >= 0], np.eye(n))
        # the restart plan has the same tables
        mn = node_plan.matrices(s)
        assert all(np.array_equal(_bits(m[key]), _bits(mn[key])) for key in ("pts", "Wu")) and np.array_equal(m["copy_u"], mn["copy_u"])
    plan.close()
    node_plan.close()


def test_control_matrix_is_the_interpolation_plans():
    """Wu equals, bit for bit, the Wu of gel_interp_plan_create at the same points"""
    E = it.engine(it.prob_of(NODES))
    plan = E.propagation_plan(steps=STEPS)
    ms = [plan.matrices(s) for s in range(E.S)]
    ip = E.interp_plan([m["pts"] for m in ms])
    for s, m in enumerate(ms):
        mi = ip.matrices(s)
        assert np.array_equal(_bits(m["Wu"]), _bits(mi["Wu"])), s
        assert np.array_equal(m["copy_u"], mi["copy_u"]), s


@pytest.mark.parametrize("n,k", [(2, 1), (5, 3), (16, 4), (64, 2), (128, 1)])
def test_control_matrix_reproduces_polynomials(n, k):
    """every polynomial of degree < n is reproduced to gamma_n sum |Wu| |p| (each entry is rounded once: u |Wu|; extrapolation
    below tau_1 included)"""
    from numpy.polynomial import chebyshev as cheb
    E = it.engine(it.prob_of([n]))
    m = E.propagation_plan(steps=k).matrices(0)
    tau, z = E.tau(0).astype(LD), m["pts"].astype(LD)
    W = m["Wu"].astype(LD)
    for d in sorted({0, 1, n // 2, n - 1}):
        c = np.zeros(d + 1)
        c[d] = 1.0
        p_tau, p_z = cheb.chebval(tau, c), cheb.chebval(z, c)
        got = W @ p_tau
        sc = np.abs(W) @ np.abs(p_tau)
        assert np.all(np.abs(got - p_z) <= gamma(n) * sc + 1e-17), (n, k, d, float((np.abs(got - p_z) / sc).max() / U))


def test_refusals():
    from gelato_amd import _lib
    E = it.engine(it.prob_of([4, 1024]))
    for bad in (0, -1, [1, 0]):
        with pytest.raises(_lib.GelatoAmdError):
            E.propagation_plan(steps=bad)
    # the 2^20 cap on steps n of one section
    with pytest.raises(_lib.GelatoAmdError):
        E.propagation_plan(steps=[1, 1025])
    with pytest.raises(_lib.GelatoAmdError):
        E.propagation_plan(steps=[2 ** 18 + 1, 1])
    ok = E.propagation_plan(steps=[2 ** 10, 1])
    assert ok.info()["lane_steps"] == 4096
    # evaluation on a host-only handle: no CPU fallback
    x = it.random_x(E)
    with pytest.raises(_lib.GelatoAmdError):
        ok.apply(x)
    with pytest.raises(_lib.GelatoAmdError):
        ok.apply_device(1, 0, 0)
    ok.close()


def test_python_argument_checks():
    from gelato_amd import _lib, propagate
    E = it.engine(it.prob_of([3, 4]))
    with pytest.raises(ValueError):
        E.propagation_plan(steps=[1, 2, 3])
    with pytest.raises(ValueError):
        E.propagation_plan(steps=[[1, 2]])
    with pytest.raises(TypeError):
        E.propagation_plan(steps=1.5)
    with pytest.raises(ValueError):
        E.propagation_plan(restart="phase")
    plan = E.propagation_plan(steps=2)
    assert plan.steps == [2, 2]
    plan.close()
    plan.close()   # twice is fine
    with pytest.raises(_lib.GelatoAmdError):
        plan.info()
    with pytest.raises(_lib.GelatoAmdError):
        plan.apply(np.zeros(E.nvars))
    with pytest.raises(ValueError):
        propagate.shooting_check({}, {"num_sections": 2}, {}, steps=0, engine=E)
    # a plan keeps its engine's handle alive
    plan = E.propagation_plan(steps=1)
    del E
    assert plan.info()["S"] == 2


_ORDER = {}


def g24_rk4_errors(n, k):
    """group errors [4] of the RESTATEMENT on g24 noair against the DOP853 truth its x holds at the nodes (cached)"""
    if (n, k) not in _ORDER:
        g = load_golden("g24_mesh_truth.npz")
        prob, x = pt.g24_case(g, "noair", n)
        E = it.engine(prob)
        plan = E.propagation_plan(steps=k)
        r = pt.propagate_phase(E, plan, prob, x, 0, want_bound=False)
        _ORDER[(n, k)] = pt.group_err(r["X"], r["y"])[0]
    return _ORDER[(n, k)]


def test_restatement_truth_and_order_on_g24():
    """x of g24 noair holds the truth at the nodes, so err is RK4's own error: it falls by 15 .. 18 per halving of the step in
    position, velocity and quaternion; at n = 8, k = 16 every group is below 2e-11; the mass error (constant right-hand side)
    is rounding, (2 n k + 4) u"""
    for n in (3, 5, 8):
        for k in (1, 2, 4):
            a, b = g24_rk4_errors(n, k), g24_rk4_errors(n, 2 * k)
            for g in (1, 2, 3):
                assert 15.0 <= a[g] / b[g] <= 18.0, (n, k, g, float(a[g]), float(b[g]))
            assert a[0] <= (2 * n * k + 4) * U, (n, k, float(a[0]))
    e = g24_rk4_errors(8, 16)
    assert np.all(e <= 2e-11), e
    print("g24 noair n = 8, k = 16:", e)

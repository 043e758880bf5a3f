"""Collocation error estimate, host side (no GPU): the matrices of a host-only handle against a 50-digit ground truth and by
exactness on polynomials, the p-rule of suggest_num_nodes, and the records of collocation_error."""
import numpy as np
import pytest
from numpy.polynomial import chebyshev as cheb

from conftest import load_golden

U = 2.0 ** -53


def _prob(nn):
    from gelato_amd import con_dynamics, problem
    pdict, unitdict, _c, _x = problem.make_problem("example")
    prob = dict(con_dynamics.problem_arrays(pdict, unitdict))
    S = len(nn)
    for k in ("thrust", "massflow", "reference_area", "nozzle_area", "engine_on", "attitude_hold"):
        prob[k] = np.resize(prob[k], S)
    prob["num_nodes"] = np.array(nn, dtype=np.int32)
    return prob


def _host_engine(nn):
    from gelato_amd import Engine
    return Engine(_prob(nn), device=-1)


def test_matrices_match_50_digit_truth():
    g = load_golden("g23_mesh_matrices.npz")
    ns = [int(n) for n in g["ns"]]
    E = _host_engine(ns)
    assert E.mesh_npts() == sum(n + 1 for n in ns)
    for s, n in enumerate(ns):
        m = E.mesh_matrices(s)
        assert np.array_equal(E.tau(s), g["tau_%d" % n])
        assert np.array_equal(m["sigma"], g["sigma_%d" % n])
        assert m["sigma"][-1] == 1.0
        for k in ("Lx", "Lu", "I"):
            ref = g["%s_%d" % (k, n)]
            assert m[k].shape == ref.shape
            row = np.abs(ref).max(axis=1, keepdims=True)
            assert np.all(np.abs(m[k] - ref) <= 1e-13 * row), (n, k, float((np.abs(m[k] - ref) / row).max()))


def test_matrices_exact_on_polynomials_n128():
    """n = 128: Lx reproduces Chebyshev polynomials of degree <= n on [-1, tau], Lu those of degree <= n - 1 on tau, and I
    integrates the derivative of those of degree <= n + 1 (degree <= n), each to rounding: the error of a row is a few ulps of
    sum |row| |p| (the row's entries are rounded once, the products and the sum in fp64)."""
    n = 128
    E = _host_engine([n])
    m = E.mesh_matrices(0)
    tau = E.tau(0)
    tx = np.concatenate([[-1.0], tau])
    sg = m["sigma"]
    tol = 64 * U
    for k in range(n + 1):
        c = np.zeros(k + 1)
        c[k] = 1.0
        got, ref = m["Lx"] @ cheb.chebval(tx, c), cheb.chebval(sg, c)
        assert np.all(np.abs(got - ref) <= tol * (k + 1) * (np.abs(m["Lx"]).sum(axis=1) + 1)), ("Lx", k)
        if k <= n - 1:
            got, ref = m["Lu"] @ cheb.chebval(tau, c), cheb.chebval(sg, c)
            assert np.all(np.abs(got - ref) <= tol * (k + 1) * (np.abs(m["Lu"]).sum(axis=1) + 1)), ("Lu", k)
    for k in range(1, n + 2):
        c = np.zeros(k + 1)
        c[k] = 1.0
        dp = cheb.chebval(sg, cheb.chebder(c))
        got, ref = m["I"] @ dp, cheb.chebval(sg, c) - cheb.chebval(-1.0, c)
        scale = np.abs(m["I"]) @ np.abs(dp) + 1.0
        assert np.all(np.abs(got - ref) <= tol * (k + 1) * scale), ("I", k, float(np.max(np.abs(got - ref) / scale)))


def test_handle_with_caller_tau_builds_on_it():
    """the matrices are built on the handle's own tau: a caller-supplied tau moves Lx and Lu, not sigma or I"""
    from gelato_amd import Engine
    prob = _prob([6])
    E0 = Engine(prob, device=-1)
    tau = E0.tau(0).copy()
    tau[:-1] += 1e-3 * np.sin(np.arange(5))
    D = [E0.D(0)]
    E1 = Engine(prob, D=D, tau=[tau], device=-1)
    a, b = E0.mesh_matrices(0), E1.mesh_matrices(0)
    assert np.array_equal(a["sigma"], b["sigma"]) and np.array_equal(a["I"], b["I"])
    assert not np.array_equal(a["Lx"], b["Lx"]) and not np.array_equal(a["Lu"], b["Lu"])
    tx = np.concatenate([[-1.0], tau])
    assert np.allclose(b["Lx"] @ tx ** 3, b["sigma"] ** 3, atol=1e-14)


def test_suggest_num_nodes_p_rule():
    from gelato_amd.mesh_error import suggest_num_nodes
    rep = [{"name": "A", "num_nodes": 8, "max": 1e-9},                 # kept
           {"name": "B", "num_nodes": 4, "max": 1e-6},                 # log(1e2)/log 4 = 3.32 -> +4
           {"name": "C", "num_nodes": 10, "max": 2e-8},                # log(2)/log 10 = 0.30 -> +1
           {"name": "D", "num_nodes": 16, "max": 1e-2},                # log(1e6)/log 16 = 4.98 -> +5 = 21 > 20: capped
           {"name": "E", "num_nodes": 15, "max": 1e-3}]                # log(1e5)/log 15 = 4.25 -> +5 = 20 = n_max: raised
    out = suggest_num_nodes(rep, 1e-8, 20)
    assert [(o["name"], o["suggested"], o["action"]) for o in out] == [
        ("A", 8, "kept"), ("B", 8, "raised"), ("C", 11, "raised"), ("D", 20, "capped"), ("E", 20, "raised")]
    assert suggest_num_nodes([{"name": "F", "num_nodes": 5, "max": 1e-8}], 1e-8, 20)[0]["action"] == "kept"
    with pytest.raises(FloatingPointError):
        suggest_num_nodes([{"name": "G", "num_nodes": 5, "max": float("nan")}], 1e-8, 20)


class _StubEngine:
    """stands in for the device: returns err[0, s, g] = 10 s + g"""
    def __init__(self, nn):
        self.num_nodes = np.array(nn)

    def mesh_error(self, x):
        S = len(self.num_nodes)
        return (np.arange(S)[:, None] * 10.0 + np.arange(4)[None, :])[None], None, 0


def test_collocation_error_records():
    from gelato_amd import problem
    from gelato_amd.mesh_error import GROUPS, collocation_error, report_array
    pdict, unitdict, _c, xdict = problem.make_problem("example")
    S = pdict["num_sections"]
    nn = [pdict["ps_params"].nodes(i) for i in range(S)]
    rep = collocation_error(xdict, pdict, unitdict, engine=_StubEngine(nn))
    assert GROUPS == ("mass", "position", "velocity", "quaternion")
    assert [r["name"] for r in rep] == [pdict["params"][i]["name"] for i in range(S)]
    assert [r["num_nodes"] for r in rep] == nn
    for s, r in enumerate(rep):
        assert [r[k] for k in GROUPS] == [10.0 * s + g for g in range(4)]
        assert r["max"] == 10.0 * s + 3
    assert np.array_equal(report_array(rep), np.arange(S)[:, None] * 10.0 + np.arange(4)[None, :])

"""Ground truth of the node-function rows' Jacobians for tests/test_exact_rows_jac.py (tests/golden/g22_exact_rows_jac.npz, written
by tests/golden/make_exact_rows_jac.py): the cases it is taken at, and engines on the shipped example problem configured with each
case's row table.

The fixture holds, per case: the long-form rows (fn, node, tcol, mode, p), the decision vectors x [B, nvars], and per (vector, row,
column) s (df / dx_c) / p[0] in 60-digit arithmetic with h = 1e-25 (`Tc` central, `Tf` / `Tb` one-sided), `kink` where the
one-sided quotients disagree, `conv` where a convention of include/gelato_amd.h fixes the entry (exact 0), and `trunc` [B, R] the
downrange rows' Vincenty stop-rule figure (make_exact_rows_jac.py)."""
import numpy as np

CASES = ["g11", "g13", "g13b", "synthetic", "corners"]


def table(G, name):
    """the case's rows in Engine.rows_configure's long form"""
    return [(int(f), int(n), int(t), int(m), [float(q) for q in p])
            for f, n, t, m, p in zip(G[name + "_fn"], G[name + "_node"], G[name + "_tcol"], G[name + "_mode"], G[name + "_p"])]


def example_engine(flags, device=0):
    """an Engine of the shipped example problem (what con_dynamics builds for it), with the given flags"""
    from gelato_amd import Engine, con_dynamics, problem
    pdict, unitdict, _, _ = problem.make_problem("example")
    ps, S = pdict["ps_params"], pdict["num_sections"]
    return Engine(con_dynamics.problem_arrays(pdict, unitdict), D=[ps.D(i) for i in range(S)], tau=[ps.tau(i) for i in range(S)],
                  device=device, flags=flags)


def engine(G, name, flags):
    E = example_engine(flags)
    E.rows_configure([], table(G, name))
    return E


def within(J, G, name, rel=1e-9, row_rel=1e-12, trunc=0.0):
    """-> bool [B, R, 7]: |J - T| <= rel |T| + (row_rel + trunc_row) max_row |T| against the central quotient, or at a kink against
    either one-sided quotient (the side the value took); trunc_row = `trunc` times the row's Vincenty stop-rule figure"""
    Tc, Tf, Tb, kink = G[name + "_Tc"], G[name + "_Tf"], G[name + "_Tb"], G[name + "_kink"]
    scale = np.abs(Tc).max(axis=2, keepdims=True) * (row_rel + trunc * G[name + "_trunc"][:, :, None])

    def ok(T):
        with np.errstate(invalid="ignore"):
            return np.abs(J - T) <= rel * np.abs(T) + scale
    return np.where(kink, ok(Tf) | ok(Tb), ok(Tc))

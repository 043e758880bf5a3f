"""GEL_FLAG_EXACT_ROWS_JAC on the GPU: the node-function rows' Jacobians (terminal orbit rows, device-form user constraints, waypoint /
impact-point / antenna / downrange rows) exact to rounding, against the 60-digit ground truth of tests/golden/g22_exact_rows_jac.npz
(tests/exact_rows_truth.py), with row values bit-identical to a handle without the flag and the same jfn bits through every entry
point.

Bound (test_exact_against_the_ground_truth): every entry is within 1e-9 |true| + 1e-12 max_row |true| of the truth (at a kink, of
the one-sided quotient on either side); entries a convention fixes, and the columns a function does not read, are exactly 0.
Downrange rows near the launch point: the value code stops Vincenty's loop at |d lambda| < 1e-12 rad, an absolute step, so where
lambda itself is 1e-8 rad or less the loop ends after one or two trips and the derivative of the distance the product computes
is off the converged one by ~f^trips of itself.  The fixture carries that figure per row (`trunc`: the relative change of the
row's derivative between the stopped and the converged loop, in 60 digits); rows with trunc > 1e-10 are held to the bound plus
2 trunc max_row |true| (measured: the error is trunc to two digits), and their number is frozen."""
import numpy as np
import pytest

import exact_rows_truth as T
from conftest import load_golden

pytestmark = pytest.mark.gpu

# the forward-difference handle fails the same bound on this many entries at least over all cases on an MI355X (the count is printed)
FD_FAILS_AT_LEAST = 2200   # 2,249 measured
# downrange rows (vector, row) whose Vincenty stop rule leaves the derivative more than 1e-10 off the converged one: synthetic rows 15,
# 31 and 47 of the first vector (0.9 um, 0.17 m and 35 m from the launch point)
TRUNC_ROWS = {"synthetic": 3}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def rows_flag():
    from gelato_amd import _lib
    return _lib.GEL_FLAG_EXACT_ROWS_JAC


def structural_zero(G, name):
    """[R, 7]: the columns the row's function does not read (the kernel writes exact zeros there)"""
    fn, tcol = G[name + "_fn"][:, None], G[name + "_tcol"][:, None]
    c = np.arange(7)[None, :]
    t_free = (c == 6) & ((fn <= 8) | (tcol < 0))
    v_free = (c >= 3) & (c < 6) & (fn >= 9) & (fn != 12) & (fn != 13)
    return t_free | v_free


def test_exact_against_the_ground_truth():
    G = load_golden("g22_exact_rows_jac.npz")
    fd_fails = 0
    for name in T.CASES:
        X = G[name + "_x"]
        Ex, Ed = T.engine(G, name, rows_flag()), T.engine(G, name, 0)
        con, jfn, rc = Ex.rows_eval(X)
        assert rc == 0, name
        assert np.all(np.isfinite(jfn)), name
        conv = G[name + "_conv"]
        zero = np.broadcast_to(structural_zero(G, name)[None], jfn.shape)
        assert np.all(jfn[zero] == 0.0), name
        assert np.all(jfn[conv] == 0.0), name
        assert int((G[name + "_trunc"] > 1e-10).sum()) == TRUNC_ROWS.get(name, 0), name
        ok = T.within(jfn, G, name, trunc=2.0) | conv
        bad = np.argwhere(~ok)
        assert bad.size == 0, (name, [(tuple(i), jfn[tuple(i)], G[name + "_Tc"][tuple(i)]) for i in bad[:8]])
        # the forward-difference handle on the same bound (teeth): the entries a convention does not fix
        _, jd, rcd = Ed.rows_eval(X)
        fd_fails += int((~T.within(jd, G, name) & ~conv & ~zero).sum())
    print("forward-difference entries outside the bound:", fd_fails)
    assert fd_fails >= FD_FAILS_AT_LEAST


def _vectors(G, name, B, seed=7):
    X0 = G[name + "_x"]
    rng = np.random.default_rng(seed)
    X = X0[np.arange(B) % len(X0)].copy()
    X[len(X0):] *= 1.0 + 1e-4 * rng.standard_normal(X[len(X0):].shape)
    return X


@pytest.mark.parametrize("name", ["synthetic", "g13b"])
def test_values_bit_identical_and_the_same_jfn_bits_through_every_entry_point(name):
    import torch
    from gelato_amd import _lib
    G = load_golden("g22_exact_rows_jac.npz")
    Ex, Ed = T.engine(G, name, rows_flag()), T.engine(G, name, 0)
    R = len(G[name + "_fn"])
    X7 = _vectors(G, name, 7)
    c1, j1, rc = Ex.rows_eval(X7[:1])
    assert rc == 0
    c7, j7, rc = Ex.rows_eval(X7)
    assert rc == 0
    d7, _, _ = Ed.rows_eval(X7)
    assert np.array_equal(bits(c7), bits(d7)) and np.array_equal(bits(c1), bits(d7[:1]))
    assert np.array_equal(bits(j1[0]), bits(j7[0]))
    # the host path through device buffers (no zero copy) and the device form at B = 1000, d_x at an offset
    X = _vectors(G, name, 1000, seed=8)
    cB, jB, rc = Ex.rows_eval(X)
    assert rc == 0
    dB, _, _ = Ed.rows_eval(X)
    assert np.array_equal(bits(cB), bits(dB))
    for B in (1, 1000):
        buf = torch.from_numpy(np.concatenate([np.zeros(3), X[:B].ravel()])).cuda()
        d_x = buf.data_ptr() + 3 * 8
        for E, want in ((Ex, True), (Ed, False)):
            d_con = torch.empty((B, R), dtype=torch.float64, device="cuda")
            d_jfn = torch.empty((B, R, 7), dtype=torch.float64, device="cuda")
            E.rows_eval_device(B, d_x, d_con.data_ptr(), d_jfn.data_ptr())
            assert E.sync() == 0
            assert np.array_equal(bits(d_con.cpu().numpy()), bits(dB[:B]))
            if want:
                assert np.array_equal(bits(d_jfn.cpu().numpy()), bits(jB[:B]))
    # the callback, with the flag alone and with the exact defect and aero Jacobians
    d0 = T.engine(G, name, 0).eval_callback(X[0], True)
    for flags in (rows_flag(), rows_flag() | _lib.GEL_FLAG_EXACT_DEFECT_JAC | _lib.GEL_FLAG_EXACT_AERO_JAC):
        E = T.engine(G, name, flags)
        fr = E.eval_callback(X[0], True)
        assert np.array_equal(bits(fr["rows_con"]), bits(d0["rows_con"])) and np.array_equal(bits(fr["rows_con"]), bits(dB[0]))
        assert np.array_equal(bits(fr["rows_jfn"]), bits(jB[0]))
        assert np.array_equal(bits(fr["res"]), bits(d0["res"]))
        if not flags & _lib.GEL_FLAG_EXACT_DEFECT_JAC:
            assert np.array_equal(bits(fr["vals"]), bits(d0["vals"]))
        fr = E.eval_callback(X[1], False)                      # values only: the one-launch form, same row values
        assert np.array_equal(bits(fr["rows_con"]), bits(dB[1]))


def _example(extra, exact=True):
    from gelato_amd import problem
    pdict, unitdict, condition, xdict = problem.make_problem("example")
    if exact:
        pdict["rows_jacobian"] = "exact"
    return pdict, unitdict, dict(condition, **(extra or {})), xdict


def _xdict(pdict, x):
    M, N, S = pdict["M"], pdict["N"], pdict["num_sections"]
    o = np.cumsum([0, M, 3 * M, 3 * M, 4 * M, 2 * N, S + 1])
    return {k: x[o[i]:o[i + 1]].copy() for i, k in enumerate(["mass", "position", "velocity", "quaternion", "u", "t"])}


def test_exact_agrees_with_the_reference_forward_differences():
    """The reference-named functions on a handle with pdict["rows_jacobian"] = "exact" against the goldens of the imported
    reference's forward differences, with the tolerances of the existing forward-difference tests (test_rows_engine.py,
    test_waypoint.py): the exact values are what the reference approximates.  Also shows the shared handle carries the flag."""
    import json
    from gelato_amd import con_dynamics, con_user
    from gelato_amd import con_init_terminal_knot as ck
    from gelato_amd import con_waypoint as cw
    from gelato_amd.examples import user_constraints as uc
    g = load_golden("g11_knot_terminal.npz")
    conds = {"Payload": {}, "Other_incl": {"OptimizationMode": "Other", "inclination": 42.3},
             "radius": {"altitude_perigee": None, "altitude_apogee": None}}
    for cname, cd in conds.items():
        pdict, unitdict, condition, _ = _example(cd)
        assert con_dynamics.engine_of(pdict, unitdict).flags & rows_flag()
        for xname in ("init", "moved"):
            J = ck.equality_jac_6DoF_LGR_terminal(_xdict(pdict, g["x_" + xname]), pdict, unitdict, condition)
            for var, blk in J.items():
                ref = g["%s_%s_terminal_jac_%s_vals" % (xname, cname, var)]
                assert np.all(np.abs(blk["coo"][2] - ref) <= 1e-5 + 1e-6 * np.abs(ref)), (cname, xname, var)
    pdict, unitdict, condition, _ = _example({})
    con_user.set_user_module(uc)
    try:
        for xname in ("init", "moved"):
            xd = _xdict(pdict, g["x_" + xname])
            J = con_user.equality_jac_user(xd, pdict, unitdict, condition)
            for key in xd:
                nz = g["%s_user_jac_%s_nzcols" % (xname, key)]
                ref = g["%s_user_jac_%s_nzvals" % (xname, key)]
                # the reference's own forward difference of this row at x_init is 7.4e-5 from the 60-digit truth (g22, case g11, last
                # row): its truncation dx/2 |f''|, which the default handle shares with it and the exact handle does not
                tol = 1e-4 if xname == "init" else 1e-5
                assert np.all(np.abs(J[key][0, nz] - ref) <= tol + 1e-6 * np.abs(ref)), (xname, key)
    finally:
        con_user.set_user_module(None)
    g = load_golden("g13_waypoint.npz")
    fns = {"eqpos": cw.equality_jac_posLLH, "ineqpos": cw.inequality_jac_posLLH, "eqiip": cw.equality_jac_IIP,
           "ineqiip": cw.inequality_jac_IIP, "antenna": cw.inequality_jac_antenna}
    for cname, cd in json.loads(str(g["conds_json"])).items():
        pdict, unitdict, condition, _ = _example(cd)
        for xname in ("init", "moved"):
            xd = _xdict(pdict, g["x_" + xname])
            for grp, jf in fns.items():
                base = "%s_%s_%s" % (xname, cname, grp)
                if bool(g[base + "_none"]):
                    continue
                for var, blk in jf(xd, pdict, unitdict, condition).items():
                    rv = g[base + "_jac_" + var + "_vals"]
                    assert np.all(np.abs(blk["coo"][2] - rv) <= 2e-5 + 1e-6 * np.abs(rv)), (base, var)
    g = load_golden("g13b_downrange.npz")
    for cname, cd in json.loads(str(g["conds_json"])).items():
        pdict, unitdict, condition, _ = _example(dict(cd, antenna={}))
        from oracle import knot_terminal as kt
        from oracle import waypoint as wp
        sp = kt.make_spec(pdict, unitdict, condition)
        rows = wp.make_rows(sp, pdict, condition)
        names = [pdict["params"][i]["name"] for i in range(pdict["num_sections"])]
        dx = sp["dx"]
        for xname in ("init", "moved"):
            xd = _xdict(pdict, g["x_" + xname])
            for grp, jf in (("eqpos", cw.equality_jac_posLLH), ("ineqpos", cw.inequality_jac_posLLH)):
                base = "%s_%s_%s" % (xname, cname, grp)
                if bool(g[base + "_none"]):
                    continue
                jac = jf(xd, pdict, unitdict, condition)
                mine = [r for r in rows if r[0] == grp]
                rp, rt = list(g[base + "_jac_position_vals"]), list(g[base + "_jac_t_vals"])
                for ir, r in enumerate(mine):          # the unscrambling of test_waypoint.py's downrange test
                    pos3 = [rp.pop(0) for _ in range(3)]
                    if r[3] == "dr":
                        tval = rp.pop(0)
                        if r[5] == "max":
                            b = cd["waypoint"][names[r[1]]]["downrange"]
                            tval = tval * b["max"] / b["min"]
                        tol = (4e-10 + 6.4e-6) / dx / r[6]
                    else:
                        tval = rt.pop(0)
                        tol = 2e-5
                    got = list(jac["position"]["coo"][2][3 * ir:3 * ir + 3]) + [jac["t"]["coo"][2][ir]]
                    for a_, b_ in zip(got, pos3 + [tval]):
                        assert abs(a_ - b_) <= tol + 1e-6 * abs(b_), (base, ir, a_, b_, tol)
        assert con_dynamics.last_status(pdict) == 0


# rows of the synthetic case whose Taylor remainder does not fall by ~4 per halving, frozen: the step crosses a branch or passes
# within eps of a point where the function is not smooth -- the impact point at the launch pad and at the end of the first
# section (|r| crosses the polar radius: the below-the-surface branch; rows 12, 13, 28, 29), the downrange at and near the launch
# point (distance 0 is a cone; rows 15, 31, 47), and e, a(1 - e), a(1 + e) of the near-circular orbits of sections 9 and 10
# (|Laplace vector| near 0; rows 148-150, 164-166)
TAYLOR_SKIP = {12, 13, 15, 28, 29, 31, 47, 148, 149, 150, 164, 165, 166}


def test_taylor_remainder_falls_by_four_per_halving():
    G = load_golden("g22_exact_rows_jac.npz")
    name = "synthetic"
    E = T.engine(G, name, rows_flag())
    x = G[name + "_x"][0]
    M, N = E.M, E.N
    node, tcol = G[name + "_node"], G[name + "_tcol"]
    rng = np.random.default_rng(3)
    d = np.zeros_like(x)
    d[M:4 * M] = rng.standard_normal(3 * M)
    d[4 * M:7 * M] = rng.standard_normal(3 * M)
    d[11 * M + 2 * N:] = rng.standard_normal(x.size - 11 * M - 2 * N) * 1e-2
    con0, jfn, rc = E.rows_eval(x)
    assert rc == 0
    cols = np.stack([M + 3 * node, M + 3 * node + 1, M + 3 * node + 2, 4 * M + 3 * node, 4 * M + 3 * node + 1,
                     4 * M + 3 * node + 2, np.where(tcol >= 0, 11 * M + 2 * N + np.maximum(tcol, 0), 0)], axis=1)
    Jd = (jfn[0] * d[cols]).sum(axis=1)
    eps = 1e-4 * 0.5 ** np.arange(4)
    rem = np.array([np.abs(E.rows_eval(x + e * d)[0][0] - con0[0] - e * Jd) for e in eps])
    live = rem[-1] > 1e-13                                    # remainders above the rounding of the values
    ratio = rem[:-1] / np.maximum(rem[1:], 1e-300)
    bad = {int(r) for r in np.nonzero(live & ~np.all((ratio > 3.0) & (ratio < 5.0), axis=0))[0]}
    print("Taylor: %d rows live, not clean: %s" % (int(live.sum()), sorted(bad)))
    assert live.sum() >= 100
    assert bad <= TAYLOR_SKIP, sorted(bad - TAYLOR_SKIP)


def test_corners_and_nonfinite_status():
    import torch
    G = load_golden("g22_exact_rows_jac.npz")
    name = "corners"
    E = T.engine(G, name, rows_flag())
    x = G[name + "_x"][0]
    con, jfn, rc = E.rows_eval(x)
    assert rc == 0 and np.all(np.isfinite(jfn)) and np.all(np.isfinite(con))
    assert np.all(jfn[0][G[name + "_conv"][0]] == 0.0)
    assert np.all(jfn[0][:3] == 0.0) and np.all(jfn[0][-1] == 0.0)   # no impact point, equatorial inclination, downrange at lon 0
    fr = E.eval_callback(x, True)
    assert np.array_equal(bits(fr["rows_jfn"]), bits(jfn[0]))
    x_nan = x.copy()
    x_nan[E.M + 3 * int(G[name + "_node"][3])] = np.nan     # a position component of the equatorial node
    _, jn, rc = E.rows_eval(x_nan)
    assert rc == 1
    assert E.rows_eval(x)[2] == 0                            # the flag was consumed
    R = len(G[name + "_fn"])
    d_x = torch.from_numpy(np.vstack([x, x_nan])).cuda()
    d_con = torch.empty((2, R), dtype=torch.float64, device="cuda")
    d_jfn = torch.empty((2, R, 7), dtype=torch.float64, device="cuda")
    E.rows_eval_device(2, d_x.data_ptr(), d_con.data_ptr(), d_jfn.data_ptr())
    assert E.sync() == 1
    assert np.array_equal(bits(d_jfn[0].cpu().numpy()), bits(jfn[0]))


def test_gauss_newton_consumer_converges_with_every_jacobian_exact():
    import gn_consumer
    from gelato_amd import con_dynamics, con_user, driver, problem
    from gelato_amd.examples import user_constraints as uc
    g = load_golden("g17_gn_trace.npz")
    pdict, unitdict, condition, xdict = problem.make_problem("example")
    pdict["defect_jacobian"] = pdict["aero_jacobian"] = pdict["rows_jacobian"] = "exact"
    con_user.set_user_module(uc)
    try:
        objfunc, sens = driver.make_callbacks(pdict, unitdict, condition)
        tr = gn_consumer.gauss_newton(objfunc, sens, xdict)
    finally:
        con_user.set_user_module(None)
    assert con_dynamics.engine_of(pdict, unitdict).flags & rows_flag()
    norms = np.array([t["norm"] for t in tr])
    assert norms[-1] < 1e-4 * norms[0] and norms[1] < 0.1 * norms[0]
    assert norms[-1] <= 1.1 * g["norms"][len(tr) - 1] + 1e-9, (norms, g["norms"])
    assert con_dynamics.last_status(pdict) == 0

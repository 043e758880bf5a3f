"""GEL_FLAG_EXACT_AERO_JAC on the GPU: the aero path constraints' gradients (angle of attack, dynamic pressure, q-alpha) exact to
rounding, against the 60-digit ground truth of tests/golden/g20_exact_aero_jac.npz (tests/exact_aero_truth.py), with constraint
values bit-identical to a handle without the flag and the same bits through every entry point.

Bound (test_exact_against_the_ground_truth).  Every entry of a row with alpha >= 1e-3 rad, of every q row, is within
1e-12 + 1e-9 |true| of the truth (the one-sided quotient on the side the value took where a knot lies within h).  Rows with a
smaller alpha: the perpendicular vectors e - c u, u - c e of the kernel have length sin(alpha) but are formed from unit vectors
whose direction carries eps kappa, kappa = (|v| + omega |r_xy| + |w|) / |v_air| the row's own cancellation in the air-relative
velocity (the fp64 inputs v = x unit_v, r = x unit_p are eps |v| off the exact ones; kappa is in the fixture, up to 7e4 at the
lift-off nodes of mixed-6x64), so every alpha entry is off by O(eps kappa / alpha) of the row's size, and so is the alpha value
(acos of c near 1) that q-alpha's alpha dq term carries.  Those rows are held to 1e-12 + 1e-9 |true| + 8 eps kappa / alpha
max_row |true| (measured: at most 0.014 of the allowance, row 1 of mixed-6x64), and their number is frozen.  The q part of every
q-alpha row (alpha dq, with the kernel's own alpha value and dalpha entries taken out) is held to 1e-12 + 1e-9 |true| whatever
alpha is.  Rows whose fp64 value clamps alpha to 0
(cos > 1 or |v_air|^2 < 1e-12) are not compared with the truth (exact arithmetic has c <= 1): their alpha entries must be exactly
0 and their number is frozen too.  The t columns are exactly 0."""
import numpy as np
import pytest

import exact_aero_truth as T
from conftest import load_golden

pytestmark = pytest.mark.gpu

EPS = 2.220446049250313e-16
# the small-alpha rows' allowance in units of eps kappa / alpha of the row's largest entry (kappa: the fixture's per-row conditioning
# of the air-relative velocity)
C_SMALL = 8.0
SMALL_ALPHA = 1e-3
# rows with 0 < alpha < SMALL_ALPHA (the vertical ascent of mixed-6x64) and rows whose fp64 value clamps alpha, per (case, kind)
SMALL_ROWS = {("g9_synthetic", "qalpha"): 4, ("mixed-6x64", "alpha"): 50, ("mixed-6x64", "qalpha"): 50}
CLAMPED_ROWS = {("g9_synthetic", "qalpha"): 1, ("mixed-6x64", "alpha"): 1, ("mixed-6x64", "qalpha"): 1, ("corners", "alpha"): 2,
                ("corners", "qalpha"): 2}
# the forward-difference handle fails the same bound on 16,478 entries over all cases on an MI355X (the count is printed)
FD_FAILS_AT_LEAST = 16000
# rows whose Taylor step crosses a table knot or atmosphere layer (remainder not falling by ~4), per workload: the union over kinds
TAYLOR_CROSSING = {"mixed-6x64": {98, 180, 281, 301}, "stress-12x128": {276, 277, 279, 342, 578, 579}}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def engine(name, flags):
    from gelato_amd import Engine
    prob, D, x, specs = T.case(name)
    E = Engine(prob, D=D, tau=prob["tau"], flags=flags)
    for kind in T.KINDS:
        E.aero_configure(kind, specs[kind])
    return E, prob, x, specs


def aero():
    from gelato_amd import _lib
    return _lib.GEL_FLAG_EXACT_AERO_JAC


def check_against_truth(name, flags, report, fixture="g20_exact_aero_jac.npz"):
    """-> number of entries outside the bound (asserted 0 by the caller for the exact handle)"""
    G = load_golden(fixture)
    E, prob, x, specs = engine(name, flags)
    from gelato_amd import Engine
    A = Engine(prob, D=T.case(name)[1], tau=prob["tau"], flags=aero())   # the same rows with limit 1: alpha, dalpha, dq as they are
    kappa = G[name + "_kappa"]
    fails = 0
    for kind in T.KINDS:
        if len(specs[kind]) == 0:
            continue
        tr = T.Truth(G, name, prob, x, kind, specs[kind])
        con, jv, rc = E.eval_aero(kind, x[None, :])
        assert rc == 0
        jv = jv[0]
        rows = tr.rows_all()
        true_c = tr.coo_all(tr.grad("c"))
        true_f, true_b = tr.coo_all(tr.grad("f")), tr.coo_all(tr.grad("b"))
        kink = np.concatenate([tr.coo(tr.kinked().astype(float), v) for v in T.VARS]) > 0
        # rows whose fp64 value has alpha clamped to 0: the angle of attack of the same rows with limit 1 is exactly 0
        clamped = np.zeros(len(tr.lim), bool)
        if kind != "q":
            spec_a = np.array(specs[kind], dtype=np.float64).reshape(-1, 3).copy()
            spec_a[:, 2] = 1.0
            A.aero_configure("alpha", spec_a)
            ca, ja, rca = A.eval_aero("alpha", x[None, :])
            assert rca == 0
            alpha_e = 1.0 - ca[0]                          # the kernel's alpha value (exact to 1 ulp of 1)
            clamped = alpha_e == 0.0
        small = (tr.alpha < SMALL_ALPHA) & ~clamped if kind != "q" else np.zeros(len(tr.lim), bool)
        rowmax = np.zeros(len(tr.lim))
        np.maximum.at(rowmax, rows, np.abs(true_c))
        kap = tr.per_row(kappa)
        with np.errstate(divide="ignore", invalid="ignore"):
            extra = np.where(small, C_SMALL * EPS * kap / np.maximum(tr.alpha, 1e-300) * rowmax, 0.0)[rows]
        err = np.abs(jv - true_c)
        err = np.where(kink, np.minimum(np.abs(jv - true_f), np.abs(jv - true_b)), err)
        # on the polar axis the value jumps along x / y (altitude -N on the axis): no derivative exists; the kernel's convention (the
        # partials of p and of the longitude are 0) is checked for finiteness only (test_corners_finite_and_nonfinite_status)
        jump = np.zeros((len(tr.lim), 10), bool)
        for sd in "aq":
            jump |= np.abs(tr.d[(sd, "f")] - tr.d[(sd, "b")]) > 1e3 * (np.abs(tr.d[(sd, "c")]) + 1.0)
        jump = np.concatenate([tr.coo(jump.astype(float), v) for v in T.VARS]) > 0
        assert not jump.any() or name == "corners"
        tight = 1e-12 + 1e-9 * np.abs(true_c)
        ok = (err <= tight + extra) | clamped[rows] | jump
        fails += int(np.count_nonzero(~ok))
        with np.errstate(divide="ignore", invalid="ignore"):
            used = np.where(small[rows] & ~jump, (err - tight) / extra, 0.0)
        report.append((name, kind, int(small.sum()), int(clamped.sum()), int(np.count_nonzero(~ok)), float(np.max(used, initial=0.0))))
        if flags & aero():
            bad = np.flatnonzero(~ok)
            assert ok.all(), (name, kind, [(int(i), int(rows[i]), float(tr.alpha[rows[i]]), float(err[i]), float(true_c[i])) for i in bad[:20]])
            if kind == "qalpha":
                # the q part: entry limit = -(q dalpha + alpha dq); with the kernel's alpha value and dalpha entries (the alpha kind of the
                # limit-1 handle: -dalpha) and the true q, what is left is alpha dq against the truth's dq, to the tight bound
                dal_e = -ja[0]
                dq_t = tr.coo_all(tr.d[("q", "c")])
                q_t = tr.q[rows]
                recon = -(q_t * dal_e + alpha_e[rows] * dq_t) / tr.lim[rows]
                nok = np.concatenate([tr.coo(tr.kink["q"].astype(float), v) for v in T.VARS]) > 0
                part = (np.abs(jv - recon) <= tight) | nok | jump
                assert part.all(), (name, "q part of q-alpha", np.flatnonzero(~part)[:8], np.abs(jv - recon)[~part][:8])
            assert int(small.sum()) == SMALL_ROWS.get((name, kind), 0), (name, kind, int(small.sum()))
            assert int(clamped.sum()) == CLAMPED_ROWS.get((name, kind), 0), (name, kind, int(clamped.sum()))
            if kind != "q":   # the alpha part of a clamped row is exactly 0; for q-alpha so is alpha dq (alpha = 0)
                assert not jv[clamped[rows]].any()
            nrow, nnz = E.aero_dims(kind)
            assert not jv[sum(nnz[:3]):].any(), "t columns: exact zeros"
            assert np.all(np.isfinite(jv))
    return fails


def test_exact_against_the_ground_truth_and_the_fd_handle_fails_it():
    report, fd_report = [], []
    for name in T.CASES:
        assert check_against_truth(name, aero(), report) == 0
    fd = sum(check_against_truth(name, 0, fd_report) for name in T.CASES)
    print("exact: (case, kind, small-alpha rows, clamped rows, fails)", report)
    print("forward differences: entries outside the bound", fd, fd_report)
    assert fd >= FD_FAILS_AT_LEAST, fd


@pytest.mark.parametrize("name", T.LONG_CASES)
def test_exact_against_the_ground_truth_over_long_tables(name):
    """the same bound and rules, nothing excluded, over 160 wind rows and 48 CA rows (tests/table_cases.py LONG; g28,
    tests/golden/make_long_tables.py) on the (40, 65, 2) mesh, all three kinds on both aerodynamic phases: exact_aero_kernel's
    wind slopes come from slope[idx] of the bisection branch; the forward-difference handle fails the bound"""
    report, fd_report = [], []
    assert check_against_truth(name, aero(), report, "g28_long_tables.npz") == 0
    fd = check_against_truth(name, 0, fd_report, "g28_long_tables.npz")
    print("exact:", report, "forward differences: entries outside the bound", fd)
    assert fd >= 300, fd        # the q rows' position entries alone (105 rows x 3): truncation dx unit_p / (2 H) = 6e-6 of the entry


@pytest.mark.parametrize("name", ["mixed-6x64", "g9_synthetic"])
def test_values_bit_identical_through_every_entry_point(name):
    import torch
    E0, prob, x, specs = engine(name, 0)
    E1, _, _, _ = engine(name, aero())
    rng = np.random.default_rng(11)
    for B in (1, 300):      # zero-copy and copied forms of gel_eval_aero_all
        X = np.tile(x, (B, 1))
        X[1:] += rng.standard_normal((B - 1, E0.nvars)) * 1e-4
        c0, _, rc0 = E0.eval_aero_all(X)
        c1, _, rc1 = E1.eval_aero_all(X)
        assert rc0 == rc1 == 0
        for kind in c0:
            assert np.array_equal(bits(c0[kind]), bits(c1[kind])), (B, kind)
            a0, _, _ = E0.eval_aero(kind, X)
            a1, _, _ = E1.eval_aero(kind, X)
            assert np.array_equal(bits(a0), bits(a1)) and np.array_equal(bits(a1), bits(c1[kind])), (B, kind)
    # device form, callback and records
    B = 300
    d_x = torch.from_numpy(X).cuda()
    outs = []
    for E in (E0, E1):
        dc = {k: torch.empty((B, E.aero_dims(k)[0]), dtype=torch.float64, device="cuda") for k in T.KINDS}
        dj = {k: torch.empty((B, sum(E.aero_dims(k)[1])), dtype=torch.float64, device="cuda") for k in T.KINDS}
        E.eval_aero_all_device(B, d_x.data_ptr(), [dc[k].data_ptr() if E.aero_dims(k)[0] else 0 for k in T.KINDS],
                               [dj[k].data_ptr() if E.aero_dims(k)[0] else 0 for k in T.KINDS])
        assert E.sync() == 0
        outs.append({k: dc[k].cpu().numpy() for k in T.KINDS if E.aero_dims(k)[0]})
    for k in outs[0]:
        assert np.array_equal(bits(outs[0][k]), bits(outs[1][k])), k
    cb0, cb1 = E0.eval_callback(x, True), E1.eval_callback(x, True)
    assert cb0["rc"] == cb1["rc"] == 0
    for k in cb0["aero_con"]:
        assert np.array_equal(bits(cb0["aero_con"][k]), bits(cb1["aero_con"][k])), k
    recs = []
    for E in (E0, E1):
        w, ci, ji = E.aero_record_layout()
        d_res = torch.empty((B, E.nres), dtype=torch.float64, device="cuda")
        d_jv = torch.empty((B, E.V), dtype=torch.float64, device="cuda")
        d_a = torch.full((B, w), np.nan, dtype=torch.float64, device="cuda")
        E.eval_batch_aero_device(B, d_x.data_ptr(), d_res.data_ptr(), d_jv.data_ptr(), d_a.data_ptr())
        assert E.sync() == 0
        recs.append((d_a.cpu().numpy(), ci, ji, d_res.cpu().numpy(), d_jv.cpu().numpy()))
    for k in T.KINDS:
        if E0.aero_dims(k)[0]:
            g0, g1 = E0.aero_gather(recs[0][0], recs[0][1][k]), E1.aero_gather(recs[1][0], recs[1][1][k])
            assert np.array_equal(bits(g0), bits(g1)), k
            assert np.array_equal(bits(g1), bits(outs[1][k])), k
    assert np.array_equal(bits(recs[0][3]), bits(recs[1][3])), "defect residuals"
    assert np.array_equal(bits(recs[0][4]), bits(recs[1][4])), "defect Jacobian (forward differences on both handles)"


def test_exact_gradient_bits_through_every_entry_point():
    import torch
    from gelato_amd import _lib
    name = "mixed-6x64"
    E, prob, x, specs = engine(name, aero())
    E32, _, _, _ = engine(name, _lib.GEL_FLAG_EXACT_DEFECT_JAC)
    E96, _, _, _ = engine(name, aero() | _lib.GEL_FLAG_EXACT_DEFECT_JAC)
    ref = {k: E.eval_aero(k, x[None, :])[1][0] for k in T.KINDS}
    cb = E.eval_callback(x, True)
    assert cb["rc"] == 0
    for k in T.KINDS:
        assert np.array_equal(bits(cb["aero_jac"][k]), bits(ref[k])), ("callback", k)
    cb96 = E96.eval_callback(x, True)
    assert cb96["rc"] == 0
    assert np.array_equal(bits(cb96["vals"]), bits(E32.eval_callback(x, True)["vals"]))
    for k in T.KINDS:
        assert np.array_equal(bits(cb96["aero_jac"][k]), bits(ref[k])), ("callback 32|64", k)
    rng = np.random.default_rng(5)
    for B, pos in ((1, 0), (5, 3), (300, 257), (4100, 4099), (4100, 0), (4100, 2050)):
        X = np.tile(x, (B, 1)) + rng.standard_normal((B, E.nvars)) * 1e-4
        X[pos] = x
        if B <= 300:
            _, jac, rc = E.eval_aero_all(X)
            assert rc == 0
            for k in T.KINDS:
                assert np.array_equal(bits(jac[k][pos]), bits(ref[k])), ("eval_aero_all", B, pos, k)
        d_x = torch.from_numpy(X).cuda()
        dc = {k: torch.empty((B, E.aero_dims(k)[0]), dtype=torch.float64, device="cuda") for k in T.KINDS}
        dj = {k: torch.empty((B, sum(E.aero_dims(k)[1])), dtype=torch.float64, device="cuda") for k in T.KINDS}
        E.eval_aero_all_device(B, d_x.data_ptr(), [dc[k].data_ptr() for k in T.KINDS], [dj[k].data_ptr() for k in T.KINDS])
        assert E.sync() == 0
        for k in T.KINDS:
            assert np.array_equal(bits(dj[k][pos].cpu().numpy()), bits(ref[k])), ("device", B, pos, k)
        for Eh in (E, E96):
            w, ci, ji = Eh.aero_record_layout()
            d_res = torch.empty((B, Eh.nres), dtype=torch.float64, device="cuda")
            d_jv = torch.empty((B, Eh.V), dtype=torch.float64, device="cuda")
            d_a = torch.full((B, w), np.nan, dtype=torch.float64, device="cuda")
            Eh.eval_batch_aero_device(B, d_x.data_ptr(), d_res.data_ptr(), d_jv.data_ptr(), d_a.data_ptr())
            assert Eh.sync() == 0
            rec = d_a[pos].cpu().numpy()
            for k in T.KINDS:
                assert np.array_equal(bits(Eh.aero_gather(rec, ji[k])), bits(ref[k])), ("records", Eh.flags, B, pos, k)
            # the defect part: the handle's own gel_eval_batch_device (32|64: the 32-only handle's exact Jacobian)
            Ed = E32 if Eh is E96 else E
            r2 = torch.empty((B, Ed.nres), dtype=torch.float64, device="cuda")
            j2 = torch.empty((B, Ed.V), dtype=torch.float64, device="cuda")
            Ed.eval_batch_device(B, d_x.data_ptr(), r2.data_ptr(), j2.data_ptr())
            assert Ed.sync() == 0
            assert np.array_equal(bits(d_jv[pos].cpu().numpy()), bits(j2[pos].cpu().numpy())), ("defects", Eh.flags, B, pos)
            assert np.array_equal(bits(d_res[pos].cpu().numpy()), bits(r2[pos].cpu().numpy())), ("residuals", Eh.flags, B, pos)
        del d_x, dc, dj


@pytest.mark.parametrize("name", ["mixed-6x64", "stress-12x128"])
def test_taylor_remainder_falls_by_four_per_halving(name):
    """|con(x + eps v) - con(x) - eps J v| falls by ~4 per halving of eps (3 .. 5.3 over three halvings) on every row whose remainder
    is above rounding; alpha and q-alpha rows with alpha < 1e-2 rad are left out (alpha = acos(c) is not smooth at 0 on the scale of
    the step) and counted; the rows whose step crosses a table knot or atmosphere layer are listed (TAYLOR_CROSSING) and at most 3 %."""
    from gelato_amd import Engine, con_dynamics, pack_x, problem
    import oracle
    pdict, unitdict, _, xdict = problem.make_problem(name)
    prob, x = dict(con_dynamics.problem_arrays(pdict, unitdict)), pack_x(xdict)
    P = oracle.Problem(prob)
    E = Engine(prob, D=[P.D(i) for i in range(P.S)], tau=[P.tau(i) for i in range(P.S)], flags=aero())
    spec = np.array([(i, 1, 1.0) for i in range(P.S - 1) if prob["reference_area"][i] != 0.0])
    for kind in T.KINDS:
        E.aero_configure(kind, spec)
    M, N = E.M, E.N
    rng = np.random.default_rng(2)
    v = np.zeros(E.nvars)
    v[M:11 * M] = rng.standard_normal(10 * M)
    v[M:11 * M] *= 1e-3                                   # 1e-3 of the position / velocity units (and of the quaternion) per unit step
    c0, J, rc = E.eval_aero_all(x[None, :])
    assert rc == 0
    alpha = 1.0 - c0["alpha"][0]                          # limit 1
    report = {}
    for kind in T.KINDS:
        nrow, nnz = E.aero_dims(kind)
        Jv = np.zeros(nrow)
        off = 0
        for base, (r, c) in zip((M, 4 * M, 7 * M, 11 * M + 2 * N), E.aero_pattern(kind)):
            Jv += np.bincount(r, weights=J[kind][0, off:off + len(r)] * v[base + c], minlength=nrow)
            off += len(r)
        rem = []
        for s in range(4):
            eps = 1e-2 * 0.5 ** s
            cs, _, rc = E.eval_aero_all((x + eps * v)[None, :], want_jac=False)
            assert rc == 0
            rem.append(np.abs(cs[kind][0] - c0[kind][0] - eps * Jv))
        rem = np.array(rem)
        smooth = (alpha >= 1e-2) if kind != "q" else np.ones(nrow, bool)
        live = (rem[0] > 1e-11) & smooth
        ratios = rem[:-1, live] / np.maximum(rem[1:, live], 1e-300)
        ok = np.all((ratios > 3.0) & (ratios < 5.3), axis=0)
        bad_rows = np.flatnonzero(live)[~ok]
        report[kind] = {"rows": nrow, "live": int(live.sum()), "left out (alpha < 1e-2)": int((~smooth).sum()), "crossing": bad_rows.tolist()}
        assert live.sum() >= nrow // 2, (kind, report)
        assert len(bad_rows) <= max(3, 0.03 * live.sum()), (kind, report)
        assert set(bad_rows.tolist()) <= TAYLOR_CROSSING[name], (kind, report)
    print("taylor", name, report)


def test_corners_finite_and_nonfinite_status():
    """the corner nodes (air at rest, exactly on the polar axis, below the polar radius): finite gradients and GEL_OK.  A NaN in a
    position gives GEL_NONFINITE from eval_aero, the callback and gel_sync after a device call.  This covers the status path end to
    end: the NaN also makes the constraint values non-finite, so the values-only launch raises the flag as well -- the aero entry
    points have no gradient-only call that would isolate the exact kernel's own store of the flag."""
    import torch
    E, prob, x, specs = engine("corners", aero())
    con, jac, rc = E.eval_aero_all(x[None, :])
    assert rc == 0
    for k in T.KINDS:
        assert np.all(np.isfinite(jac[k])) and np.all(np.isfinite(con[k]))
    x_nan = x.copy()
    x_nan[E.M + 3 * 2] = np.nan                            # x component of phase 0's node 2's position
    assert E.eval_aero("q", x_nan[None, :])[2] == 1
    assert E.eval_aero("q", x[None, :])[2] == 0            # the flag was consumed
    cb = E.eval_callback(x_nan, True)
    assert cb["rc"] == 1
    d_x = torch.from_numpy(np.vstack([x, x_nan])).cuda()
    dc = {k: torch.empty((2, E.aero_dims(k)[0]), dtype=torch.float64, device="cuda") for k in T.KINDS}
    dj = {k: torch.empty((2, sum(E.aero_dims(k)[1])), dtype=torch.float64, device="cuda") for k in T.KINDS}
    E.eval_aero_all_device(2, d_x.data_ptr(), [dc[k].data_ptr() for k in T.KINDS], [dj[k].data_ptr() for k in T.KINDS])
    assert E.sync() == 1
    for k in T.KINDS:
        assert np.all(np.isfinite(dj[k][0].cpu().numpy()))


def test_con_aero_mirror_returns_the_exact_values():
    from gelato_amd import con_aero, con_dynamics, pack_x, problem
    pdict, unitdict, condition, xdict = problem.make_problem("example")
    pdict["aero_jacobian"] = "exact"
    cond = {"AOA_max": {"MECO": {"value": 10.0, "range": "initial"}}, "dynamic_pressure_max": {"ZEROLIFT_START": {"value": 40000.0, "range": "all"}},
            "Q_alpha_max": {"ZEROLIFT_START": {"value": 30000.0, "range": "all"}}}
    for kind, jfn in (("alpha", con_aero.inequality_jac_max_alpha), ("q", con_aero.inequality_jac_max_q),
                      ("qalpha", con_aero.inequality_jac_max_qalpha)):
        jac = jfn(xdict, pdict, unitdict, cond)
        st, n = con_aero._configured(pdict, unitdict, cond, kind)
        assert n > 0 and st.engine.flags & aero()
        E = st.engine
        _, jv, rc = E.eval_aero(kind, pack_x(xdict)[None, :])
        assert rc == 0
        pat = E.aero_pattern(kind)
        vals = np.concatenate([jac[var]["coo"][2] for var in T.VARS])
        for var, (r, c) in zip(T.VARS, pat):
            assert np.array_equal(jac[var]["coo"][0], r) and np.array_equal(jac[var]["coo"][1], c)
        assert np.array_equal(bits(vals), bits(jv[0])), kind
    assert con_dynamics.last_status(pdict) == 0

"""GPU: the exact defect Jacobian (GEL_FLAG_EXACT_DEFECT_JAC, gelato_amd/csrc/gel_kernels_exact.hip).

  * against the ground truth (tests/golden/g19_exact_jac.npz: 60-digit derivatives of the reference's formulas, see
    tests/golden/make_exact_jac.py): every x-dependent entry within 1e-12 + 1e-9 |true| on the shipped example, the synthetic
    extremes of tests/states.py and the corner nodes; the forward-difference handle fails that bound on most velocity-group
    entries of aerodynamic phases;
  * against the reference's forward differences: every G6 fixture within the flat Jacobian tolerance 1e-5 + 1e-6 |ref| of the
    golden values and of the oracle (vel/position: 1e-5 + 1e-5 |ref|, the difference's own truncation error, see below); same pattern, same constants (bit for bit), residuals bit-identical to the default handle;
  * Taylor test at full size: |r(x + e v) - r(x) - e J v| falls by 4 per halving of e (2 for a wrong or misplaced entry);
  * the same exact rows through gel_eval, gel_eval_callback and gel_eval_batch_device at several batch sizes and positions;
  * corners (underground, polar axis, at rest in the air): finite, GEL_OK; a NaN input: GEL_NONFINITE;
  * the Gauss-Newton consumer converges with pdict["defect_jacobian"] = "exact"."""
import numpy as np
import pytest

from conftest import D_tau_from_golden, load_golden, problem_from_golden

pytestmark = pytest.mark.gpu

EXACT = 32   # GEL_FLAG_EXACT_DEFECT_JAC


def engines(prob, D=None, tau=None):
    from gelato_amd import Engine
    return Engine(prob, D=D, tau=tau, device=0), Engine(prob, D=D, tau=tau, device=0, flags=EXACT)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


TRUTH_STATES = ["example", "ragged", "layers", "breaks", "polar", "corners"]


def check_state_against_truth(G, name, prob, x):
    """one state of a fixture written by make_exact_jac.state_truth against the exact handle (asserted) and the default handle
    -> (velocity-group entries of aerodynamic phases the forward differences have outside the bound, their number)"""
    import exact_jac_truth
    from gelato_amd import Engine
    from gelato_amd.engine import BLOCKS
    fd_bad = fd_all = 0
    assert np.array_equal(x, G[name + "_x"]), "the state builder no longer reproduces the fixture's decision vector"
    E0, E1 = Engine(prob, device=0), Engine(prob, device=0, flags=EXACT)
    _, v1, rc = E1.eval(x)
    assert rc == 0
    want = [exact_jac_truth.expected_full(E1, prob, x, G, name, w) for w in ("c", "f", "b")]
    var = E1.var_mask()
    assert np.all(np.isfinite(want[0][var])) and np.all(np.isnan(want[0][~var]))
    # where the value jumps (the polar-axis nodes, x / y position columns) no derivative exists: the engine follows the stated
    # convention (the partials of p and of the longitude are 0: the air of the axis point held), to the same bound
    jump = exact_jac_truth.jump_entries(E1, prob, G, name)
    assert name == "corners" or not jump.any()
    assert jump.sum() <= 18
    conv = exact_jac_truth.expected_full(E1, prob, x, G, name, "conv")
    cex = np.abs(v1 - conv) - (1e-12 + 1e-9 * np.abs(conv))
    assert cex[jump].max(initial=-1.0) <= 0.0, "convention at the polar axis: excess %g" % cex[jump].max()
    ex = np.min([np.abs(v1 - w) - (1e-12 + 1e-9 * np.abs(w)) for w in want], axis=0)[var & ~jump]
    assert ex.max() <= 0.0, "%s: %d entries outside 1e-12 + 1e-9 |true|, worst excess %g" % (
        name, int((ex > 0).sum()), ex.max())
    if name == "corners":
        return fd_bad, fd_all
    _, v0, _ = E0.eval(x)
    ex0 = np.min([np.abs(v0 - w) - (1e-12 + 1e-9 * np.abs(w)) for w in want], axis=0)
    nn = [int(v) for v in prob["num_nodes"]]
    aero_node = np.repeat(np.asarray(prob["reference_area"]) > 0, nn)
    pat = E1.pattern()
    for b, (grp, vn) in enumerate(BLOCKS):
        if grp != "vel" or vn == "t":
            continue
        sl = slice(E1.block_off[b], E1.block_off[b + 1])
        m = var[sl] & aero_node[pat[b][0] // 3]
        fd_all += int(m.sum())
        fd_bad += int((ex0[sl][m] > 0).sum())
    return fd_bad, fd_all


def test_exact_against_the_ground_truth():
    """every x-dependent entry of the exact handle within 1e-12 + 1e-9 |true| of the 60-digit derivative (at a node with a knot
    within the truth's step -- the polar-axis nodes, whose longitude jumps, and the nodes at rest in the air -- of the central
    or of either one-sided quotient); teeth: the default handle's forward differences (truncation dx / 2 |f''| ~ 1e-8 of an
    entry, plus rounding amplified by 1 / dx) fail the bound on most velocity-group entries of the aerodynamic phases"""
    import exact_jac_truth
    G = load_golden("g19_exact_jac.npz")
    builders = exact_jac_truth.states()
    fd_bad = fd_all = 0
    for name in TRUTH_STATES:
        prob, x = builders[name]()
        bad, n = check_state_against_truth(G, name, prob, x)
        fd_bad, fd_all = fd_bad + bad, fd_all + n
    assert fd_bad > 0.5 * fd_all, "the forward-difference handle meets the exact bound on %d of %d entries" % (fd_all - fd_bad, fd_all)
    print("forward differences outside the exact bound: %d of %d velocity-group entries" % (fd_bad, fd_all))


@pytest.mark.parametrize("vector", ["climb", "knots"])
def test_exact_against_the_ground_truth_over_long_tables(vector):
    """the same bound, nothing excluded, over 160 wind rows and 48 CA rows (tests/table_cases.py LONG: the bisection branch of the
    lookups and of interp_tab_slope's slope[idx]; g28, tests/golden/make_long_tables.py) on the (40, 65, 2) mesh: `climb` visits
    102 wind and 45 CA intervals, `knots` has nodes 4 mm and 4 cm either side of six wind knots (none ON a knot: the fixture has no `kink` entry) -- a slope taken from the
    neighbouring interval is off by the table's noise, far outside 1e-9 of the entry"""
    import states
    import table_cases as TC
    G = load_golden("g28_long_tables.npz")
    prob, x = states.table_state("LONG", TC.MESHES["coop"], vector)
    fd_bad, fd_all = check_state_against_truth(G, vector, prob, x)
    assert fd_bad > 0.5 * fd_all, (fd_bad, fd_all)


@pytest.mark.parametrize("name", ["example", "3x32", "mixed6x64", "dense6x64", "negarea"])
def test_exact_against_the_references_finite_differences(name):
    import oracle
    from gelato_amd.engine import BLOCKS
    g = load_golden("g6_%s.npz" % name)
    prob = problem_from_golden(g)
    D, tau = D_tau_from_golden(g, prob)
    x = g["x"]
    E0, E1 = engines(prob, D, tau)
    r0, v0, rc0 = E0.eval(x)
    r1, v1, rc1 = E1.eval(x)
    assert rc0 == 0 and rc1 == 0
    assert np.array_equal(bits(r0), bits(r1)), "residuals of the exact handle differ from the default handle's"
    var = E1.var_mask()
    assert np.array_equal(bits(v0[~var]), bits(v1[~var])), "constant entries"
    assert np.all(np.isfinite(v1))
    P = oracle.Problem(prob, D=D, tau=tau)
    worst = 0.0
    for b, (grp, vname) in enumerate(BLOCKS):
        sl = slice(E1.block_off[b], E1.block_off[b + 1])
        got, m = v1[sl], var[sl]
        Jo = P.jacobian(grp, x)[vname]["coo"][2]
        # vel/position: the forward difference's own truncation error, dx unit_p / 2 |d2f/dr2| <= dx unit_p / (2 H) |df/dr| with H >= 5 km
        # the density scale height (the fastest-varying factor of the chain: rho ~ exp(-h / H)), is 6.4e-6 of the entry at dx = 1e-8
        # -- above the flat 1e-6 (measured: 3.4e-6 against the exact value at 11 km) -- so that block takes 1e-5 relative
        rt = 1e-5 if (grp, vname) == ("vel", "position") else 1e-6
        for ref in [Jo] + ([g["jac_%s_%s_vals" % (grp, vname)]] if "jac_%s_%s_vals" % (grp, vname) in g else []):
            ex = np.abs(got[m] - ref[m]) - (1e-5 + rt * np.abs(ref[m]))
            if ex.size:
                worst = max(worst, float(ex.max()))
    assert worst <= 0.0, "exact Jacobian outside the flat FD tolerance by %g" % worst


def _state(name):
    from gelato_amd import con_dynamics, pack_x, problem
    pdict, unitdict, condition, xdict = problem.make_problem(name)
    ps = pdict["ps_params"]
    S = pdict["num_sections"]
    return dict(con_dynamics.problem_arrays(pdict, unitdict)), [ps.D(i) for i in range(S)], [ps.tau(i) for i in range(S)], \
        pack_x(xdict)


def _jv(E, vals, v):
    """J v per group from the full COO values"""
    from gelato_amd.engine import BLOCKS
    pat = E.pattern()
    V = E.split_x(v)
    out = {g: np.zeros(n) for g, n in zip(["mass", "pos", "vel", "quat"], E.nrows)}
    for b, (grp, var) in enumerate(BLOCKS):
        r, c = pat[b]
        np.add.at(out[grp], r, vals[E.block_off[b]:E.block_off[b + 1]] * V[var][c])
    return out


@pytest.mark.parametrize("name", ["mixed-6x64", "stress-12x128"])
def test_taylor_remainder_is_second_order_at_full_size(name):
    """r(x + e v) - r(x) - e J v = O(e^2): per node and group the remainder falls by 4 per halving of e.  Steps per variable
    group: at e = 1 a node moves by up to 40 m and 4 m/s, the mass by 1e-4, quaternion / u by 1e-3 of their scale and the knot
    times by 1e-6 -- large enough that the remainder at the smallest e stays far above the fp64 rounding of r, small enough
    that few nodes leave their table interval or atmosphere layer.  Nodes where that happens (the remainder is not quadratic
    over the range) are counted and must stay rare; a wrong or misplaced entry breaks the ratio at every node it touches."""
    prob, D, tau, x = _state(name)
    _, E1 = engines(prob, D, tau)
    up, uv = float(prob["units"][1]), float(prob["units"][2])
    rng = np.random.default_rng(19)
    X = E1.split_x(x)
    scale = {"mass": 1e-4, "position": 40.0 / up, "velocity": 4.0 / uv, "quaternion": 1e-3, "u": 1e-3, "t": 1e-6}
    v = np.concatenate([rng.uniform(-1.0, 1.0, X[k].size) * scale[k] * max(1.0, float(np.max(np.abs(X[k]))) if k in ("u", "t") else 1.0)
                        for k in ("mass", "position", "velocity", "quaternion", "u", "t")])
    eps = np.array([1.0, 0.5, 0.25, 0.125])
    Xb = np.vstack([x] + [x + e * v for e in eps])
    res, _, rc = E1.eval_batch(Xb, want_res=True, want_jac=False)
    assert rc == 0
    _, vals, rc = E1.eval(x)
    assert rc == 0
    Jv = _jv(E1, vals, v)
    rs = E1.split_res(res)
    N = E1.N
    report = {}
    for grp, k in (("pos", 3), ("vel", 3), ("quat", 4)):
        rem = np.stack([rs[grp][i + 1] - rs[grp][0] - e * Jv[grp] for i, e in enumerate(eps)])    # [4, k N]
        node = np.sqrt((rem.reshape(4, N, k) ** 2).sum(axis=2))                                       # [4, N]
        scale_r = np.abs(rs[grp][0]).reshape(N, k).max(axis=1) + np.abs(eps[0] * Jv[grp]).reshape(N, k).max(axis=1) + 1.0
        live = node[-1] > 1e-12 * scale_r                     # remainder above the rounding of r at the smallest step
        ratio = node[1:-1][:, live] / node[2:][:, live]       # the last two halvings
        ok = np.all((ratio > 3.3) & (ratio < 4.7), axis=0)
        bad = int(np.count_nonzero(~ok))
        report[grp] = (int(np.count_nonzero(live)), bad)
        if grp == "vel":
            assert np.count_nonzero(live) >= N // 2, "the velocity remainder must be measurable at most nodes"
        assert bad <= max(3, 0.02 * np.count_nonzero(live)), (grp, report)
    print("taylor", name, report)


def test_exact_rows_are_the_same_through_every_entry_point():
    import torch
    prob, D, tau, x = _state("mixed-6x64")
    E0, E = engines(prob, D, tau)
    _, vals, rc = E.eval(x)
    assert rc == 0
    out = E.eval_callback(x, True)
    assert out["rc"] == 0
    assert np.array_equal(bits(out["vals"]), bits(vals))
    # the callback's defect part is split out on an exact handle: its residuals are still the default handle's
    res_cb = out["res"].copy()
    assert np.array_equal(bits(res_cb), bits(E0.eval_callback(x, True)["res"]))
    rng = np.random.default_rng(5)
    for B, pos in ((1, 0), (5, 3), (300, 257), (4100, 4099)):
        X = np.tile(x, (B, 1)) + (rng.standard_normal((B, E.nvars)) * 1e-3)
        X[pos] = x
        d_x = torch.from_numpy(X).cuda()
        d_res = torch.empty((B, E.nres), dtype=torch.float64, device="cuda")
        d_jv = torch.empty((B, E.V), dtype=torch.float64, device="cuda")
        E.eval_batch_device(B, d_x.data_ptr(), d_res.data_ptr(), d_jv.data_ptr())
        assert E.sync() == 0
        full = E.expand(d_jv[pos].cpu().numpy())
        assert np.array_equal(bits(full), bits(vals)), (B, pos)
        res1, _, _ = E.eval(x)
        assert np.array_equal(bits(d_res[pos].cpu().numpy()), bits(res1)), (B, pos)


def test_corners_underground_polar_and_at_rest_and_nonfinite_jacobian():
    """the corner nodes (exact_jac_truth.corner_state: below the polar radius, exactly on the polar axis, at rest in the air):
    finite, GEL_OK (their values against the truth: test_exact_against_the_ground_truth).  A NaN in a node's position makes the
    exact kernel's OWN outputs non-finite: GEL_NONFINITE from a Jacobian-only call (no residual launch to flag it) and from
    gel_sync after a device call without residuals."""
    import torch
    import exact_jac_truth
    from gelato_amd import Engine
    prob, x = exact_jac_truth.corner_state()
    E = Engine(prob, device=0, flags=EXACT)
    res, vals, rc = E.eval(x)
    assert rc == 0 and np.all(np.isfinite(vals)) and np.all(np.isfinite(res))
    x_nan = x.copy()
    x_nan[E.M + 3 * 2] = np.nan                            # x component of node 1's position
    _, rc = E.eval_jacobian(x_nan)
    assert rc == 1
    assert E.eval_jacobian(x)[1] == 0                      # the flag was consumed
    d_x = torch.from_numpy(np.vstack([x, x_nan])).cuda()
    d_jv = torch.empty((2, E.V), dtype=torch.float64, device="cuda")
    E.eval_batch_device(2, d_x.data_ptr(), 0, d_jv.data_ptr())
    assert E.sync() == 1
    assert np.all(np.isfinite(d_jv[0].cpu().numpy()))


def test_gauss_newton_consumer_converges_with_the_exact_jacobian():
    import gn_consumer
    from gelato_amd import con_dynamics, con_user, driver, problem
    from gelato_amd.examples import user_constraints as uc
    g = load_golden("g17_gn_trace.npz")
    pdict, unitdict, condition, xdict = problem.make_problem("example")
    pdict["defect_jacobian"] = "exact"
    con_user.set_user_module(uc)
    try:
        objfunc, sens = driver.make_callbacks(pdict, unitdict, condition)
        tr = gn_consumer.gauss_newton(objfunc, sens, xdict)
    finally:
        con_user.set_user_module(None)
    norms = np.array([t["norm"] for t in tr])
    assert norms[-1] < 1e-4 * norms[0] and norms[1] < 0.1 * norms[0]
    # no worse than the forward-difference trace after the same number of steps, beyond a margin of 10 %
    assert norms[-1] <= 1.1 * g["norms"][len(tr) - 1] + 1e-9, (norms, g["norms"])
    assert con_dynamics.last_status(pdict) == 0

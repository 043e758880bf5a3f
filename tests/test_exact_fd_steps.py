"""The velocity-defect Jacobian and the aero rows against EXACT finite-difference quotients over the range of position steps the
difference form accepts (tests/golden/g29_exact_fd_steps.npz, tests/golden/make_exact_fd_steps.py; the cases: tests/fd_steps.py).

tests/test_exact_fd.py holds the engine to its bound at the reference's own step alone, dx * unit_position = 6.4 cm.  The series of
pos_delta / atmosphere_delta are cut for steps up to 1 m, a truncation error grows with the square or the cube of the step, and
fd_noise.engine_bound shrinks as 1 / dx: a term that is missing shows at the large steps, not at 6.4 cm.  Here: steps of 1e-5 m,
1e-3 m, 0.25 m and the largest the host accepts (dx_one: the largest double with fl(dx * unit_position) <= 1.0) by dx alone, and
1 m / 1e-5 m by unit_position with dx = 1e-8; the all-layers state, the polar state, and a break state and its mirror (breaks,
breaks_m) whose nodes together sit +-0.06, +-0.6, +-1.2 and +-2.5 STEPS from every break of the atmosphere layers, the 86 km
branch, 91 / 110 / 120 km and the wind table's rows.

A node counts as handed over to the recomputing sweep (its entries are held to the reference's bound, not the engine's) if
fd_noise's `near_break` says so (within 1.5 steps of a break), if pos_delta's |u| reaches 1e-4 at this step (states.pos_delta_u),
or if its altitude is within 1.5 steps of 86 km -- fd_noise lists that break by its geopotential image rounded to 84852 m, 5 cm
below the real one, which steps of millimetres do not reach.  Handed over, of the nodes of each state (the tests print it):
layers 1 of 64 at every step (the node at 11 km, a wind row and a layer break; asserted: at most half); polar none of 48 below
1 m, 1 at the three 1 m steps; breaks 35 (breaks_m 36) of 60 at the two 1e-5 m steps, 44 of 60 at the others (0.06, 0.6 and 1.2 steps from a
break count, 2.5 steps do not).

The position entries of the nodes that are not handed over are held to fd_noise.engine_bound ALONE (compare() of
tests/test_exact_fd.py allows 1e-9 of the entry besides: up to 8.9 times the bound at 1 m); measured on the MI355X they use at most
0.049 of it at any step, 0.046 at 1 m (DESIGN.md 3.1 has the figure of every case).

CPU part: the oracle within the reference's bound at every (state, step) -- the bounds hold for the reference's algorithm there
before the device is asked.  GPU part (-m gpu): the engine through the C-ABI."""
import numpy as np
import pytest

import fd_noise
import fd_steps
import states
from conftest import load_golden
from test_exact_fd import VARS, block_entries, compare

CASES = [(s, l) for s in fd_steps.STATES for l in fd_steps.STEPS]
GOLDEN = "g29_exact_fd_steps.npz"
_G = {}


def golden():
    if not _G:
        _G.update(load_golden(GOLDEN))
    return _G


def handed_over(prob, x, terms):
    """[n] bool: the nodes of phase 0 whose position sweeps the engine recomputes (see the module's docstring)"""
    n = int(prob["num_nodes"][0])
    M = sum(int(v) for v in prob["num_nodes"]) + len(prob["num_nodes"])
    xr = x[M:4 * M].reshape(-1, 3)[1:n + 1]
    u, _p = states.pos_delta_u(prob, xr)
    step = abs(float(prob["dx"]) * float(prob["units"][1]))
    return terms["near_break"] | (np.abs(u) >= states.POS_DELTA_U).any(axis=1) | (np.abs(terms["alt"] - 86000.0) <= 1.5 * step)


def setup(state, label, step=None):
    """step: (dx, unit_position) of a case without a fixture (dx_over)"""
    import oracle
    prob, x = fd_steps.build(state, label if step is None else step)
    name = "%s@%s" % (state, label)
    G = golden()
    if step is None:
        assert np.array_equal(fd_steps.digest(x), G[name + "_xsha"]), "the state builder no longer reproduces the fixture's decision vector"
    P = oracle.Problem(prob)
    prob["tau"] = [P.tau(i) for i in range(P.S)]
    terms = fd_noise.velocity_noise_terms(oracle, prob, x)
    terms[0]["near_break"] = handed_over(prob, x, terms[0])      # what fd_noise.engine_bound switches on
    return oracle, G, name, prob, x, P, terms


def test_fixture_is_smaller_than_the_largest_one_and_the_default_break_state_is_unchanged():
    import os
    from conftest import GOLDEN as DIR
    sizes = {f: os.path.getsize(os.path.join(DIR, f)) for f in os.listdir(DIR) if f.endswith(".npz")}
    assert sizes[GOLDEN] < max(v for f, v in sizes.items() if f != GOLDEN) and sizes[GOLDEN] < 410 * 1024
    assert np.array_equal(states.layer_break_state()[1], load_golden("g15_exact_fd.npz")["breaks_x"])
    up = fd_steps.example_unit_position()
    one, over = fd_steps.dx_at_the_switch(up)
    assert np.float64(one) * np.float64(up) <= 1.0 < np.float64(over) * np.float64(up) and np.nextafter(one, np.inf) == over


@pytest.mark.parametrize("state,label", CASES)
def test_oracle_within_the_reference_noise_bound_at_every_step(state, label):
    oracle, G, name, prob, x, P, terms = setup(state, label)
    J = P.jacobian("vel", x)
    worst = compare(J, G, name, prob, P, terms, fd_noise.reference_bound, fd_noise.reference_bound_other, "oracle")
    ho = terms[0]["near_break"]
    print("%s: step %.3g m, %d of %d nodes handed over; oracle's worst |entry - exact| / reference bound %.3f (%s)" % (
        name, float(prob["dx"]) * float(prob["units"][1]), ho.sum(), len(ho), max(worst.values()),
        ", ".join("%s %.3f" % (k[1], v) for k, v in worst.items())))
    if state == "layers":      # the engine's own bound is asked of at least half of this state's nodes at every step
        assert 2 * int(ho.sum()) <= len(ho), (name, int(ho.sum()))
    if state.startswith("breaks"):      # ... and some nodes of the break state are handed over, some are not, at every step
        assert 4 <= int(ho.sum()) < len(ho), (name, int(ho.sum()))


def closed_form_columns(J, G, name, prob, x):
    """the mass, quaternion and t columns as tests/test_exact_fd.py holds them: closed forms of the exact quotient"""
    for var in ("quaternion", "mass"):
        got = block_entries(J, prob, 0, var)
        exact = G["%s_p0_%s" % (name, var)].reshape(got.shape)
        scale = np.abs(exact).reshape(len(exact), -1).max(axis=1)[:, None, None]
        assert np.all(np.abs(got - exact) <= 1e-12 * scale + 1e-300), (name, var, (np.abs(got - exact) / (scale + 1e-300)).max())
    r, c, v = J["t"]["coo"]
    n = int(prob["num_nodes"][0])
    ut = prob["units"][4]
    fc = G["%s_p0_fc" % name].ravel()
    for col, sign in ((0, 1.0), (1, -1.0)):
        sel = (r >= 0) & (r < 3 * n) & (c == col)
        assert np.all(np.abs(v[sel] - sign * fc * ut / 2) <= 1e-12 + 1e-10 * np.abs(fc * ut / 2)), (name, col)


@pytest.mark.gpu
@pytest.mark.parametrize("state,label", CASES)
def test_engine_difference_form_within_its_bound_at_every_step(state, label):
    oracle, G, name, prob, x, P, terms = setup(state, label)
    from gelato_amd import Engine
    E = Engine(prob, D=[P.D(0)], tau=prob["tau"], barC20=oracle.BARC20_CPP)
    vals, rc = E.eval_jacobian(x)
    assert rc == 0
    J = E.jac_dicts(vals)["vel"]
    # the position block at the nodes the difference form covers: fd_noise.engine_bound ALONE -- compare() below allows 1e-9 of the
    # entry besides, which at 1 m is several times the bound and would hide exactly the series error these steps are here for.
    # Nothing is added: one ulp of an entry (entries are up to 1e3 x chain) is 1e-6 of the bound at 1 m.  Measured, then asserted.
    keep = ~terms[0]["near_break"]
    bound = fd_noise.engine_bound(terms[0])[:, None, None]
    got = block_entries(J, prob, 0, "position")
    exact = G["%s_p0_position" % name].reshape(got.shape)
    share = np.abs(got - exact) / (bound + 1e-300)
    slack = (1e-9 * np.abs(exact) / (bound + 1e-300))[keep].max()
    print("%s: position entries at the %d of %d nodes not handed over: worst |entry - exact| / engine_bound %.3f (the 1e-9 |exact| that "
          "compare() would add is up to %.2f of the bound here); at the handed-over nodes, over the reference bound: %.3f" % (
              name, keep.sum(), len(keep), share[keep].max(), slack, share[~keep].max() if (~keep).any() else 0.0))
    assert share[keep].max() <= 1.0, "%s: a position entry of a covered node is %.2f x fd_noise.engine_bound off the exact quotient" % (
        name, share[keep].max())
    compare(J, G, name, prob, P, terms, fd_noise.engine_bound, fd_noise.engine_bound, "engine (exact-difference form)")
    closed_form_columns(J, G, name, prob, x)
    # the same vector in a batch (throughput form of the kernel): same bits
    B = 9
    res, jv, rc = E.eval_batch(np.tile(x, (B, 1)))
    assert rc == 0 and np.array_equal(E.expand(jv[B - 1]), vals)


@pytest.mark.gpu
@pytest.mark.parametrize("state,label", CASES)
def test_engine_recomputing_form_within_the_reference_bound_at_every_step(state, label):
    oracle, G, name, prob, x, P, terms = setup(state, label)
    from gelato_amd import Engine
    E = Engine(prob, D=[P.D(0)], tau=prob["tau"], barC20=oracle.BARC20_CPP, flags=8)
    vals, rc = E.eval_jacobian(x)
    assert rc == 0
    worst = compare(E.jac_dicts(vals)["vel"], G, name, prob, P, terms, fd_noise.reference_bound, fd_noise.reference_bound_other,
                    "engine (recomputing form)")
    print("%s: recomputing form, worst |entry - exact| / reference bound %.3f" % (name, max(worst.values())))


@pytest.mark.gpu
@pytest.mark.parametrize("state", ["layers", "breaks"])
def test_hand_over_to_the_recomputing_sweeps_at_exactly_one_metre(state):
    """dx_one (fl(dx * unit_position) <= 1.0): the difference form -- not the recomputing form's bits, both inside their bounds,
    and the exact-Jacobian flags accepted.  dx_over, one ulp on: the default handle IS the recomputing form, residual and Jacobian
    bit for bit, and the exact-Jacobian flags are refused (their position parts lean on the same series)."""
    from gelato_amd import Engine
    from gelato_amd._lib import GelatoAmdError
    up = fd_steps.example_unit_position()
    one, over = fd_steps.dx_at_the_switch(up)
    oracle, G, name, prob, x, P, terms = setup(state, "one")
    assert float(prob["dx"]) == one
    kw = dict(D=[P.D(0)], tau=prob["tau"], barC20=oracle.BARC20_CPP)
    out = {}
    for flags in (0, 8):
        E = Engine(prob, flags=flags, **kw)
        res, vals, rc = E.eval(x)
        assert rc == 0
        out[flags] = (res, vals)
        J = E.jac_dicts(vals)["vel"]
        if flags == 0:
            compare(J, G, name, prob, P, terms, fd_noise.engine_bound, fd_noise.engine_bound, "engine (exact-difference form)")
        else:
            compare(J, G, name, prob, P, terms, fd_noise.reference_bound, fd_noise.reference_bound_other, "engine (recomputing form)")
    assert np.array_equal(out[0][0], out[8][0]), "the residual does not depend on the form of the sweeps"
    assert not np.array_equal(out[0][1], out[8][1]), "at dx_one the default handle takes the difference form"
    for flag in (32, 64):
        assert Engine(prob, flags=flag, **kw) is not None
    oracle, G, name, prob, x, P, terms = setup(state, "over", step=(over, up))
    assert np.float64(prob["dx"]) * np.float64(prob["units"][1]) > 1.0
    out = {}
    for flags in (0, 8):
        E = Engine(prob, flags=flags, **kw)
        res, vals, rc = E.eval(x)
        assert rc == 0
        out[flags] = (res, vals)
    assert np.array_equal(out[0][0], out[8][0]) and np.array_equal(out[0][1], out[8][1]), "beyond 1 m the default handle recomputes"
    for flag in (32, 64):
        with pytest.raises(GelatoAmdError, match="unit_position"):
            Engine(prob, flags=flag, **kw)


AERO_STEPS = {"6.4cm": ("polar", "g18_aero_exact_fd.npz"), "one": (fd_steps.AERO_CASE, GOLDEN)}


AERO_VARS = ("position", "velocity", "quaternion", "t")


def aero_case(label):
    """-> prob (with tau), x, P, {kind: spec}, the fixture's case name and file"""
    import oracle
    from test_aero_exact_fd import LIMITS
    from test_aero_oracle_golden import KINDS
    name, gold = AERO_STEPS[label]
    if label == "one":
        prob, x = fd_steps.build("polar", "one", coast_tail=True)
    else:
        prob, x = states.with_coast_tail(states.polar_dense_state)
        prob = dict(prob)
    P = oracle.Problem(prob)
    prob["tau"] = [P.tau(i) for i in range(P.S)]
    return prob, x, P, {k: np.array([(0, 1, LIMITS[k])]) for k in KINDS}, name, gold


def aero_truth_bounds_and_truncation(prob, x, kind, spec, name, gold):
    """per var, in the reference's emission order: the exact quotients, fd_noise.aero_coo_bounds (nothing added), and what
    fd_noise.aero_first_order_truncation would move an entry by at THIS problem's dx -- the engine's alpha difference (aero_dalpha:
    t = t0 (1 - x + 2 x^2 - x^3), x = cot(alpha) t0 / 2) cut after its first term; t0 is proportional to the step, the entry's shift
    to the step and the bound to its inverse: the teeth of the bound grow with the square of the step"""
    import oracle
    from test_aero_exact_fd import COLS, Truth
    T = Truth(name, prob, x, kind, spec, golden=gold)
    bounds = fd_noise.aero_coo_bounds(oracle, prob, x, kind, spec)
    rows = fd_noise.aero_coo_rows(prob, kind, spec)
    lim = fd_noise.aero_row_limits(prob, spec)
    dx = float(prob["dx"])
    Ta = Truth(name, prob, x, "alpha", np.array([(sp[0], sp[1], 1.0) for sp in spec]), golden=gold)    # alpha_p - alpha_c of every entry
    out = {}
    for var in AERO_VARS:
        exact = T.coo_order(T.jac[:, COLS[var]])
        if bounds[var].size == 0:      # the dynamic pressure has no quaternion entries
            continue
        t_true = -Ta.coo_order(Ta.jac[:, COLS[var]]) * dx
        out[var] = (exact, bounds[var], fd_noise.aero_first_order_truncation(T.terms, rows[var], lim[rows[var]], kind, t_true, dx))
    return out


@pytest.mark.parametrize("label", list(AERO_STEPS))
def test_aero_bound_would_reject_a_truncated_alpha_difference_at_one_metre(label):
    """Teeth of fd_noise.aero_coo_bounds at the step at hand: the exact entries moved by aero_first_order_truncation.  At 1 m the
    alpha and the q-alpha kind must leave the bound (position and velocity sweeps alike); at 6.4 cm the figure is printed -- there the
    shift is 244 times smaller against a bound 15.6 times larger (measured: see DESIGN.md 3.1).  The q kind has no alpha: no shift."""
    from test_aero_oracle_golden import KINDS
    prob, x, P, specs, name, gold = aero_case(label)
    for kind in KINDS:
        for var, (exact, bound, shift) in aero_truth_bounds_and_truncation(prob, x, kind, specs[kind], name, gold).items():
            assert np.isfinite(bound).all()
            ratio = np.abs(shift) / (bound + 1e-300)
            print("aero %s %s/%s: truncated alpha difference moves an entry by up to %.3g x aero_coo_bounds (%d of %d entries beyond it)" % (
                label, kind, var, ratio.max(), (ratio > 1.0).sum(), ratio.size))
            if kind == "q":
                assert not shift.any()
            elif var == "t":       # the t quotients are zero to the fixture's 40 digits
                assert ratio.max() < 1e-12
            elif label == "one" and var in ("position", "velocity"):
                assert ratio.max() > 1.0, (kind, var, ratio.max())


@pytest.mark.gpu
@pytest.mark.parametrize("label", list(AERO_STEPS))
def test_aero_rows_fused_and_two_kernel_forms_at_the_reference_step_and_at_one_metre(label, monkeypatch):
    """states.with_coast_tail(states.polar_dense_state), every node of its aerodynamic phase constrained by the three kinds: the
    gradients against exact_fd.aero_fd_truth within fd_noise.aero_coo_bounds (which takes the problem's dx; nothing added) from
    gel_eval_batch_aero_device's records, with the rows in the fused kernel (GEL_AERO_FUSED=1) and from aero_kernel (=0): same bits.
    Teeth: the device's entries moved by aero_first_order_truncation at this step -- at 1 m the alpha and q-alpha kinds then leave
    the bound, which the device's full series does not."""
    import oracle
    from gelato_amd import Engine
    from test_aero_oracle_golden import KINDS
    from test_aero_engine import check_fused_equals_two, fused_outputs
    prob, x, P, specs, name, gold = aero_case(label)
    B = 132          # 132 vectors x 2 work items x 4 > 1024 wavefronts: not the split latency form (tests/test_degenerate_fd.py)
    X = np.tile(x, (B, 1))
    records = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("GEL_AERO_FUSED", fused)      # read when the handle is created
        E = Engine(prob, D=[P.D(i) for i in range(P.S)], tau=prob["tau"])
        for kind in KINDS:
            E.aero_configure(kind, specs[kind])
        info = E.launch_info(B)
        assert info[2] == 0 and info[4] == 0, info
        one, two, layout = fused_outputs(E, X)
        check_fused_equals_two(E, one, two, layout)
        width, ocon, ojac = layout
        records[fused] = [E.aero_gather(one["aero"], idx[kind]) for idx in (ocon, ojac) for kind in KINDS]
        for kind in KINDS:
            tb = aero_truth_bounds_and_truncation(prob, x, kind, specs[kind], name, gold)
            jv = E.aero_gather(one["aero"], ojac[kind])[B - 1]
            nrow, nnz = E.aero_dims(kind)
            off = 0
            for v, var in enumerate(AERO_VARS):
                vals = jv[off:off + nnz[v]]
                off += nnz[v]
                if vals.size == 0:
                    continue
                exact, bound, shift = tb[var]
                ratio = np.abs(vals - exact) / (bound + 1e-300)
                mutant = np.abs(vals + shift - exact) / (bound + 1e-300)
                print("aero %s GEL_AERO_FUSED=%s %s/%s: worst |entry - exact| / aero_coo_bounds %.3f; with the alpha difference cut after "
                      "its first term %.3g" % (label, fused, kind, var, ratio.max(), mutant.max()))
                assert np.isfinite(bound).all() and ratio.max() <= 1.0, (label, fused, kind, var, ratio.max())
                if label == "one" and kind != "q" and var in ("position", "velocity"):
                    assert mutant.max() > 1.0, (kind, var, mutant.max())
                if var == "t":
                    assert not vals.any()
    assert all(np.array_equal(a, b) for a, b in zip(records["1"], records["0"])), "the fused and the two-kernel form: the same bits"

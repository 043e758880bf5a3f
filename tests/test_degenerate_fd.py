"""The default Jacobian where its forms change hands or its formulas degenerate: next to the polar axis and at rest in the air,
against EXACT finite-difference quotients (tests/golden/g27_degenerate_fd.npz, tests/golden/make_degenerate_fd.py: the reference's
formulas in 40-digit arithmetic on the fp64 inputs its sweeps form).

The position columns of the velocity defect and of the aero rows are formed in two ways (gel_rhs_parts.h pos_delta): the
exact-difference form, and -- for a lane whose node is too close to the polar axis for its series, |u| >= 1e-4 with
u = dlt (2 x + dlt) / p^2 -- the reference's recomputation of the chain on the perturbed point.  Three classes of nodes:

  covered      every sweep takes the difference form (axis_state phase 0: p from within 2 % above the switch, 1276 m for x = p, to
               11 km; rest_state; the underground and at-rest nodes of corner_state):
                   default handle  |entry - exact| <= fd_noise.engine_bound     (chain term only, half the constant)
  fallback     1 m <= p <= the switch (axis_state phase 1): the reference's algorithm, the reference's noise class
                   default handle, GEL_FLAG_FD_RECOMPUTE everywhere, the oracle  <= fd_noise.reference_bound(_other)
  undecidable  p < 1 m (axis_state phase 2) and the on-axis nodes of corner_state: fp64 cannot decide the answer.  The reference's
               alt = p / cos(lat) - N is off by 3 cm .. 29 km there (cos(lat) = p / 6.4e6 from an angle whose ulp is 1e-16), so every
               entry is a quotient at ANOTHER altitude; and with the centre or a perturbed point exactly on the axis its convention
               (cos(pi / 2) = 6.1e-17: alt = -N) makes the x / y quotients a jump.  No accuracy assertion; they get the status
               property and the bit identity across the output paths, their exact COUNT is asserted, and the engine's distance from
               the truth is printed.

Status property, every node of every state: every output path returns GEL_OK and every residual, Jacobian value, aero value and
aero gradient entry is finite -- no finite residual beside a non-finite entry (1 / |v_air|, the guarded cot(alpha)).

The aero rows are held to fd_noise.aero_bound (the oracle: + aero_drift).  Centre values: the suite's value tolerance plus
|d f / d alt| d_alt of the same module -- near the axis the reference's altitude rounding shows in the VALUE too.  No tolerance
here is new.  The truth of this fixture takes the Earth rate as the double the reference's C++ holds (make_degenerate_fd.py): next to
rest v - omega x r cancels to 1e-13 m/s, and the decimal's 9e-17 is 3e-14 m/s there.  Measured fractions of every bound: DESIGN.md 5.
CPU part: the oracle, the classes, the teeth.  GPU part (-m gpu): the engine through the C-ABI."""
import functools
import types

import numpy as np
import pytest

import exact_jac_truth
import fd_noise
import states
from conftest import load_golden
from test_aero_exact_fd import COLS, LIMITS, VALUE_BOUND_CAP, Truth
from test_aero_oracle_golden import KINDS, VARS as AERO_VARS
from test_exact_fd import VARS, block_entries, compare

GOLDEN = "g27_degenerate_fd.npz"
BUILD = {"axis": states.axis_state, "rest": states.rest_state,
         "corners": lambda: states.with_coast_tail(exact_jac_truth.corner_state)}
NAMES = list(BUILD)
COVERED, FALLBACK, UNDECIDABLE = 0, 1, 2          # the aerodynamic phases of axis_state
# the nodes that are held to no truth, per state: (collocation nodes of the velocity defect, aero rows = state nodes).  axis: phase 2
# (36 nodes, 37 with its node 0).  corners: its three on-axis nodes; the one at 143 km is still held to the defect's truth (what
# air there is changes no entry by more than the bound), its aero rows are not (q jumps from 0 to its true value over dx).
UNCHECKED = {"axis": (36, 37), "rest": (0, 0), "corners": (2, 3)}
# aero rows whose REFERENCE value is not finite, per (state, kind): the only rows that may report GEL_NONFINITE.  None.
NONFINITE_ROWS = {}
# rows that are held to the truth but whose alpha is clamped to 0 (|v_air| < 1e-6 m/s): no finite bound, per (state, kind).  rest: its 3
# nodes exactly at rest and its 15 below the clamp (q alpha: q = 0 exactly at rest, the bound is 0 there); corners: its two at-rest nodes
UNBOUNDED_ROWS = {("rest", "alpha"): 18, ("rest", "qalpha"): 15, ("corners", "alpha"): 2, ("corners", "qalpha"): 1}
# rows whose derived value bound is finite but above the 1e-8 cap of the value tolerance (value_capped): rest's nodes at 3e-6 and 1e-4 m/s
VALUE_CAPPED = {("rest", "alpha"): 2}          # (their q is 1e-12 Pa: q alpha is far inside the tolerance)
OMEGA_E = 7.2921151467e-5
R_POLAR = 6356752.314245


@functools.lru_cache(maxsize=None)
def setup(name):
    import oracle
    G = load_golden(GOLDEN)
    prob, x = BUILD[name]()
    assert np.array_equal(x, G[name + "_x"]), "the state builder no longer reproduces the fixture's decision vector"
    P0 = oracle.Problem(prob)
    prob = dict(prob)
    prob["tau"] = [P0.tau(i) for i in range(P0.S)]
    D = [P0.D(i) for i in range(P0.S)]
    P = oracle.Problem(prob, D=D, tau=prob["tau"])
    nn = [int(v) for v in prob["num_nodes"]]
    M = sum(nn) + len(nn)
    xr, xv = x[M:4 * M].reshape(-1, 3), x[4 * M:7 * M].reshape(-1, 3)
    r, _ = states.pos_step(prob, xr)
    u, p = states.pos_delta_u(prob, xr)
    phases = [int(v) for v in G[name + "_phases"]]
    # the classes, from the state itself
    if name == "axis":
        undecidable = p < 1.0 - 1e-9          # the nodes "at 1 m" are there to rounding
    elif name == "corners":
        undecidable = p == 0.0
    else:
        undecidable = np.zeros(M, dtype=bool)
    with np.errstate(invalid="ignore"):
        fallback = ~undecidable & (np.abs(u).max(axis=1) >= states.POS_DELTA_U)
    # ... of which the velocity defect still decides: on the axis, above the air that could move an entry (100 km)
    no_air = undecidable & (np.abs(r[:, 2]) - R_POLAR >= 100.0e3) if name == "corners" else np.zeros(M, dtype=bool)
    with np.errstate(all="ignore"):
        terms = fd_noise.velocity_noise_terms(oracle, prob, x)
    rows, skip_nodes = [], {}
    for ph in phases:
        xa = sum(nn[:ph]) + ph
        rows += list(range(xa, xa + nn[ph] + 1))
        skip_nodes[ph] = (undecidable & ~no_air)[xa + 1:xa + 1 + nn[ph]]
        terms[ph]["unchecked"] = skip_nodes[ph]
        terms[ph]["fallback"] = fallback[xa + 1:xa + 1 + nn[ph]]
    rows = np.array(rows)
    vs, rs = xv * float(prob["units"][2]), r
    rel = np.column_stack([vs[:, 0] + OMEGA_E * rs[:, 1], vs[:, 1] - OMEGA_E * rs[:, 0], vs[:, 2]])
    specs = {k: np.array([(ph, 1, LIMITS[k]) for ph in phases]) for k in KINDS}
    return types.SimpleNamespace(name=name, oracle=oracle, G=G, prob=prob, x=x, P=P, D=D, nn=nn, M=M, phases=phases, terms=terms, p=p,
                                 u=u, r=r, undecidable=undecidable, fallback=fallback, skip_nodes=skip_nodes,
                                 skip_rows=undecidable[rows], rows=rows, vair=np.linalg.norm(rel, axis=1)[rows], specs=specs)


def masked(bound):
    """a per-node bound of tests/fd_noise.py, infinite at the nodes that are held to no truth"""
    return lambda t: np.where(t["unchecked"], np.inf, bound(t))


def by_class(t):
    """the default handle's bound: the difference form's where it applies, the reference's at the lanes that recompute"""
    return np.where(t["fallback"], fd_noise.reference_bound(t), fd_noise.engine_bound(t))


def by_class_other(t):
    return np.where(t["fallback"], fd_noise.reference_bound_other(t), fd_noise.engine_bound(t))


def truth(S, kind):
    """the fixture's rows of one kind; the sanity check of Truth (the oracle's alpha and q, which the noise terms are made of, against
    the fixture's) is made here instead, at every row that is held to the truth, with what one fp64 evaluation is off by: the
    altitude term and the module's e_alpha / e_q (tests/fd_noise.py) beside Truth's 1e-9"""
    T = Truth(S.name, S.prob, S.x, kind, S.specs[kind], golden=GOLDEN, checked=np.zeros(len(S.rows), dtype=bool))
    T.unchecked = S.skip_rows
    t, keep = T.terms, ~S.skip_rows
    a, q = S.G[S.name + "_alpha"], S.G[S.name + "_q"]          # the spec lists the fixture's phases in its order
    with np.errstate(all="ignore"):
        e_a = fd_noise.aero_bound(t, "alpha", 1.0, T.dx, position=True) * T.dx / 2.0
        e_q = fd_noise.aero_bound(t, "q", 1.0, T.dx, position=True) * T.dx / 2.0
    e_a = np.where(t["alpha"] > 0.0, e_a, 0.0)                 # clamped to 0 in both
    assert np.all((np.abs(t["alpha"] - a) <= 1e-9 + e_a)[keep]) and np.all((np.abs(t["q"] - q) <= 1e-9 * q + 1e-12 + e_q)[keep]), S.name
    return T


def value_capped(T):
    """rows whose DERIVED value bound is finite but above the cap of the suite's value tolerance (VALUE_BOUND_CAP = 1e-8 on f): one
    fp64 evaluation of alpha / limit is off by eps (C_ACOS / sin + C_DIR (|v| + omega |r|) / |v_air|) / limit, which passes 1e-8 below
    |v_air| = 7e-4 m/s -- no implementation can be held to the cap there, the reference included -- and above the rest of the
    tolerance too (a huge q underground is covered by its relative part).  Counted (VALUE_CAPPED)."""
    with np.errstate(all="ignore"):
        b = fd_noise.aero_bound(T.terms, T.kind, T.lim, T.dx, position=False) * T.dx / 2.0
    return np.isfinite(b) & (b > VALUE_BOUND_CAP) & (b > aero_value_tolerance(T)) & ~T.unchecked


def aero_value_tolerance(T):
    """the suite's value tolerance of f = alpha / limit, q / limit, q alpha / limit (test_aero_exact_fd) + |d f / d alt| d_alt"""
    t = T.terms
    dfdalt = {"alpha": t["dalpha_dalt"], "q": t["dq_dalt"], "qalpha": t["q"] * t["dalpha_dalt"] + t["alpha"] * t["dq_dalt"]}[T.kind]
    return 1e-11 + 1e-10 * np.abs(T.f) + T.value_bound() + dfdalt * t["dalt"] / T.lim


def aero_ratio(T, var, vals):
    """|entry - exact| / (aero_bound + 1e-9 |exact|) per entry, as Truth.check forms it (no drift: the engine does not perturb in
    place); 0 where no finite bound exists or the row is held to no truth.  The t columns are compared with their exact value, 0
    (the air-relative velocity does not depend on the Earth angle; the fixture holds what 40 digits leave of it, 1e-40 |f| / dx)."""
    exact = T.jac[:, COLS[var]]
    if not vals.size:
        return np.zeros(0)
    if var == "t":
        exact = np.zeros_like(exact)
    b = np.where(T.unchecked, np.inf, fd_noise.aero_bound(T.terms, T.kind, T.lim, T.dx, position=(var == "position")))
    bound = T.coo_order(np.repeat(b[:, None], exact.shape[1], axis=1)) + 1e-9 * np.abs(T.coo_order(exact))
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(bound), np.abs(vals - T.coo_order(exact)) / (bound + 1e-300), 0.0)


def unbounded_rows(T):
    """rows that are held to the truth but have no finite bound (alpha clamped to 0: not differentiable) -- their alpha and q alpha
    gradients and values are held to nothing but finiteness; asserted per state and kind (UNBOUNDED_ROWS)"""
    with np.errstate(all="ignore"):
        b = fd_noise.aero_bound(T.terms, T.kind, T.lim, T.dx, position=False)
    return int(np.count_nonzero(~np.isfinite(np.where(np.isnan(b), 0.0, b)) & ~T.unchecked))


def check_aero_values(S, T, con, what):
    keep = ~S.skip_rows & ~value_capped(T)
    err, tol = np.abs(con - (1.0 - T.f)), aero_value_tolerance(T)
    assert np.all(err[keep] <= tol[keep]), (what, S.name, T.kind, (err / tol)[keep].max())
    assert unbounded_rows(T) == UNBOUNDED_ROWS.get((S.name, T.kind), 0), (S.name, T.kind, unbounded_rows(T))
    assert int(value_capped(T).sum()) == VALUE_CAPPED.get((S.name, T.kind), 0), (S.name, T.kind, int(value_capped(T).sum()))


def check_centre_defect(S, res_vel, what):
    """D v - f_c dt against the exact f_c: 1e-12 + 1e-10 |.| like every residual + the dot product's rounding + |d f / d alt| d_alt dt"""
    xs = S.P.split_x(S.x)
    for ph in S.phases:
        ua = sum(S.nn[:ph]); xa = ua + ph; n = S.nn[ph]
        v = xs["velocity"].reshape(-1, 3)[xa:xa + n + 1]
        dt = (xs["t"][ph + 1] - xs["t"][ph]) * S.prob["units"][4] / 2
        Dm = S.P.D(ph)
        want = Dm @ v - S.G["%s_p%d_fc" % (S.name, ph)] * dt
        got = res_vel.reshape(-1, 3)[ua:ua + n]
        t = S.terms[ph]
        tol = 1e-12 + 1e-10 * np.abs(want) + (n + 1) * fd_noise.EPS * (np.abs(Dm) @ np.abs(v)) + (t["dfdalt"] * t["dalt"] * abs(dt))[:, None]
        keep = ~S.skip_nodes[ph]
        assert np.all(np.abs(got - want)[keep] <= tol[keep]), (what, S.name, ph, (np.abs(got - want) / tol)[keep].max())


def undecided_distance(S, J, label):
    """printed, not asserted: how far the entries at the undecidable nodes are from the 40-digit truth, in units of the reference's bound"""
    out = {}
    for ph in S.phases:
        sk = S.skip_nodes[ph]
        if not sk.any():
            continue
        with np.errstate(all="ignore"):
            b = fd_noise.reference_bound(S.terms[ph])
        for var in VARS:
            got = block_entries(J, S.prob, ph, var)
            if var == "velocity":
                for j in range(got.shape[0]):
                    got[j] -= np.eye(3) * S.P.D(ph)[j, j + 1]
            exact = S.G["%s_p%d_%s" % (S.name, ph, var)].reshape(got.shape)
            err = np.abs(got - exact)[sk]
            out[var] = (float(err.max()), float((err / (np.abs(exact)[sk] + 1e-300)).max()))
    print("%s %s, undecidable nodes: max |entry - truth| (and relative to |truth|) %s" % (label, S.name, out))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the classes, the oracle, the teeth
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_states_sort_into_their_classes():
    S = setup("axis")
    n0, n1, n2 = states.AXIS_NODES
    a, b, c = slice(0, n0 + 1), slice(n0 + 1, n0 + n1 + 2), slice(n0 + n1 + 2, n0 + n1 + n2 + 3)
    T = 2.0 * float(S.prob["dx"] * S.prob["units"][1]) / states.POS_DELTA_U
    # covered: every sweep inside the predicate (u, and v = u / 2 to first order), some within 2 % of it for x, for y, for both
    ua = np.abs(S.u[a])
    assert ua.max() < states.POS_DELTA_U and not S.fallback[a].any() and S.p[a].max() >= 11000.0 and n0 >= 10
    near = ua > 0.98 * states.POS_DELTA_U
    assert near[:, 0].sum() >= 3 and near[:, 1].sum() >= 3 and (near[:, 0] & near[:, 1]).sum() >= 2
    assert (S.r[a][near[:, 0], 0] < 0).any() and (S.r[a][near[:, 1], 1] < 0).any()          # either sign
    # fallback, decidable: 1 m <= p <= the switch, every node recomputes a sweep; within 2 % below both conditions; p = 1, 30, 300 m
    assert S.fallback[b].all() and S.p[b].min() >= 1.0 - 1e-12 and S.p[b].max() <= T and not S.undecidable[b].any()
    ub = np.abs(S.u[b]).max(axis=1)
    assert np.count_nonzero((ub >= states.POS_DELTA_U) & (ub < states.POS_DELTA_U / 0.98)) >= 4
    assert np.count_nonzero((ub >= 2 * states.POS_DELTA_U) & (ub < 2 * states.POS_DELTA_U / 0.98)) >= 3      # |v| = |u| / 2
    for want in (1.0, 30.0, 300.0):
        assert np.isclose(S.p[b], want, rtol=1e-9).any()
    # undecidable: ON the axis at both poles, p <= 0.1 m, a perturbed point that crosses the axis, one that lands on it
    r, dlt = states.pos_step(S.prob, S.x[S.M:4 * S.M].reshape(-1, 3)[c])
    assert S.undecidable[c].all() and S.p[c].max() <= 0.1 + 1e-12
    on = S.p[c] == 0.0
    assert (r[on, 2] > 0).any() and (r[on, 2] < 0).any()
    assert ((r[:, :2] < 0) & (r[:, :2] + dlt[:, :2] > 0)).any() and ((r[:, :2] < 0) & (r[:, :2] + dlt[:, :2] == 0)).any()
    # the unchecked nodes, counted: a change cannot move nodes out of the checked classes unnoticed
    for name in NAMES:
        S = setup(name)
        assert (sum(int(v.sum()) for v in S.skip_nodes.values()), int(S.skip_rows.sum())) == UNCHECKED[name], name
        # no node within a step of a break of the atmosphere / wind tables: there engine_bound would quietly become reference_bound
        assert not any(S.terms[ph]["near_break"].any() for ph in S.phases), name
    constrained = len(setup("axis").rows)
    assert UNCHECKED["axis"][1] <= constrained // 3 and constrained == n0 + n1 + n2 + 3
    # rest: three nodes exactly at rest in the air (the builder asserts that the products are exact), the others 1e-13 .. 30 m/s
    S = setup("rest")
    assert np.count_nonzero(S.vair == 0.0) == 3 and S.vair[S.vair > 0].min() < 1e-12 and 25.0 < S.vair.max() <= 30.0 + 1e-9
    # ... 15 below the reference's clamp, 9 between it and 1 m/s (1 / |v_air| times a live angle of attack), 10 above
    assert [int(np.count_nonzero((S.vair > lo) & (S.vair < hi))) for lo, hi in ((0.0, 1e-6), (1e-6, 0.99), (0.99, 31.0))] == [15, 9, 10]
    assert np.abs(np.degrees(np.arctan2(S.r[:, 2], np.hypot(S.r[:, 0], S.r[:, 1])))).max() <= 70.0


@pytest.mark.parametrize("name", NAMES)
def test_oracle_within_the_reference_bounds_at_the_decidable_nodes(name):
    S = setup(name)
    J = S.P.jacobian("vel", S.x)
    assert all(np.isfinite(J[var]["coo"][2]).all() for var in J)
    worst = compare(J, S.G, name, S.prob, S.P, S.terms, masked(fd_noise.reference_bound), masked(fd_noise.reference_bound_other), "oracle")
    assert max(worst.values()) > 0.02, worst          # the bound is not vacuous
    res = S.P.residual("vel", S.x)
    assert np.isfinite(res).all()
    check_centre_defect(S, res, "oracle")
    undecided_distance(S, J, "oracle")
    used = []
    for kind in KINDS:
        S.P.aero_configure(kind, S.specs[kind])
        T = truth(S, kind)
        con = S.P.aero_residual(kind, S.x)
        assert np.isfinite(con).all(), "a reference value that is not finite belongs into NONFINITE_ROWS"
        check_aero_values(S, T, con, "oracle")
        Ja = S.P.aero_jacobian(kind, S.x)
        for var in AERO_VARS:
            assert np.isfinite(Ja[var]["coo"][2]).all()
            used.append(T.check(var, Ja[var]["coo"][2], "oracle", with_drift=True))
    assert max(used) > 0.02, "the bound is vacuous here: nothing uses 2 % of it"


def wrong_position_block(S, ph, mutant):
    """vel/position of phase ph as a WRONG implementation's exact arithmetic would give it: `altitude` takes the perturbed point's
    altitude p' / cos(lat) - N(lat) at the CENTRE's latitude; `longitude` rotates the perturbed point's wind with the centre's
    longitude.  Everything else as oracle/exact_fd.py."""
    from mpmath import cos, mpf, sin, sqrt
    from oracle import exact_fd as X
    prob, x = S.prob, S.x
    nn, xm, xr, xv, xq, xu, xt = X._split(prob, x)
    um, up, uv = (X.f64(prob["units"][k]) for k in range(3))
    ut, dx = X.f64(prob["units"][4]), float(prob["dx"])
    xa, n = sum(nn[:ph]) + ph, nn[ph]
    to, tf = float(xt[ph]), float(xt[ph + 1])
    tn = np.asarray(prob["tau"][ph]) * (tf - to) / 2 + (tf + to) / 2
    wt, ct = np.asarray(prob["wind_table"]), np.asarray(prob["ca_table"])
    wind = [[X.f64(v) for v in wt[:, c]] for c in range(3)]
    ca = [[X.f64(v) for v in ct[:, c]] for c in range(2)]
    args = (X.f64(prob["thrust"][ph]), X.f64(prob["reference_area"][ph]), X.f64(prob["nozzle_area"][ph]), wind, ca, (um, up, uv),
            mpf(S.oracle.BARC20_CPP))
    scale = (X.f64(tf) - X.f64(to)) * ut / 2
    real, state = X.geodetic, {}

    def geodetic(px, py, pz):
        lat, lon, alt = real(px, py, pz)
        k = state["call"]
        state["call"] += 1
        if state["centre"]:
            state[k] = (lat, lon)
            return lat, lon, alt
        clat, clon = state[k]
        if mutant == "altitude" and k == 0:
            alt = sqrt(px * px + py * py) / cos(clat) - X.RA / sqrt(1 - X.E2 * sin(clat) ** 2)
        if mutant == "longitude" and k == 1:
            lon = clon
        return lat, lon, alt

    out = np.zeros((n, 3, 3))
    X.geodetic = geodetic
    try:
        for j in range(n):
            k = xa + 1 + j

            def f(r, centre):
                state["call"], state["centre"] = 0, centre
                return X.rhs_air(X.f64(xm[k]), [X.f64(v) for v in r], [X.f64(v) for v in xv[k]], [X.f64(v) for v in xq[k]], X.f64(tn[j]), *args)

            fc = f(xr[k], True)
            for c in range(3):
                rp = [float(v) for v in xr[k]]
                rp[c] = rp[c] + dx
                fp = f(rp, False)
                out[j, :, c] = [float(-(fp[i] - fc[i]) / X.f64(dx) * scale) for i in range(3)]
    finally:
        X.geodetic = real
    return out


@pytest.mark.parametrize("mutant", ["altitude", "longitude"])
def test_teeth_a_wrong_position_sweep_breaks_the_bound_next_to_the_axis(mutant):
    """what the checks of phases 0 and 1 would say of an implementation that is wrong only in how the perturbed point's geodetic
    angles enter -- the two things that change fastest next to the axis"""
    from oracle import exact_fd
    S = setup("axis")
    worst = {}
    for ph in (COVERED, FALLBACK):
        exact = S.G["axis_p%d_position" % ph]
        with exact_fd.earth_rate(exact_fd.OMEGA_F64):          # the Earth rate the fixture was made with
            got = wrong_position_block(S, ph, mutant)
        b = fd_noise.reference_bound(S.terms[ph])[:, None, None] + 1e-9 * np.abs(exact)
        worst[ph] = (np.abs(got - exact) / b).max()
    print("wrong oracle (%s): %s x the reference's bound" % (mutant, worst))
    assert max(worst.values()) > 10.0, worst


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the engine
# ---------------------------------------------------------------------------------------------------------------------------
def engine(S, flags=0):
    from gelato_amd import Engine
    E = Engine(S.prob, D=S.D, tau=S.prob["tau"], barC20=S.oracle.BARC20_CPP, flags=flags)
    for kind in KINDS:
        E.aero_configure(kind, S.specs[kind])
    return E


def finite_ok(rc, *arrays):
    return rc == 0 and all(np.isfinite(a).all() for a in arrays)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, 8])
@pytest.mark.parametrize("name", NAMES)
def test_engine_defect_jacobian_at_the_degenerate_states(name, flags):
    S = setup(name)
    E = engine(S, flags)
    vals, rc = E.eval_jacobian(S.x)
    assert finite_ok(rc, vals), ("status / finiteness", name, flags, rc)
    J = E.jac_dicts(vals)["vel"]
    what = "engine (flags %d)" % flags
    if flags == 0:
        worst = compare(J, S.G, name, S.prob, S.P, S.terms, masked(by_class), masked(by_class_other), what)
    else:
        worst = compare(J, S.G, name, S.prob, S.P, S.terms, masked(fd_noise.reference_bound), masked(fd_noise.reference_bound_other), what)
    print("%s %s: largest used fraction of the bound per (phase, block): %s" % (what, name, {k: round(float(v), 4) for k, v in worst.items()}))
    undecided_distance(S, J, what)
    if flags == 0:
        # closed forms of the exact quotient (mass: e / (1 + e); quaternion: a quadratic form): no finite-difference noise
        for ph in S.phases:
            keep = ~S.skip_nodes[ph]
            for var in ("quaternion", "mass"):
                got = block_entries(J, S.prob, ph, var)
                exact = S.G["%s_p%d_%s" % (name, ph, var)].reshape(got.shape)
                scale = np.abs(exact).reshape(len(exact), -1).max(axis=1)[:, None, None]
                rel = (np.abs(got - exact) / (scale + 1e-300))[keep]
                print("%s %s phase %d vel/%s closed form: %.3e of the node's largest entry" % (what, name, ph, var, rel.max() if rel.size else 0.0))
                assert np.all((np.abs(got - exact) <= 1e-12 * scale + 1e-300)[keep]), (name, ph, var, rel.max())
    # the same vector through every output path: same bits, GEL_OK, finite
    res1, rc1 = E.eval_residual(S.x)
    res2, vals2, rc2 = E.eval(S.x)
    cb = E.eval_callback(S.x, True)
    B = 9
    resb, jvb, rcb = E.eval_batch(np.tile(S.x, (B, 1)))
    assert finite_ok(rc1, res1) and finite_ok(rc2, res2, vals2) and finite_ok(cb["rc"], cb["res"], cb["vals"]) and finite_ok(rcb, resb, jvb)
    assert np.array_equal(vals2, vals) and np.array_equal(cb["vals"], vals) and np.array_equal(E.expand(jvb[B - 1]), vals)
    assert np.array_equal(res2, res1) and np.array_equal(cb["res"], res1) and np.array_equal(resb[B - 1], res1)
    check_centre_defect(S, E.split_res(res1)["vel"], what)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, 8])
@pytest.mark.parametrize("name", NAMES)
def test_engine_aero_rows_at_the_degenerate_states(name, flags):
    S = setup(name)
    E = engine(S, flags)
    what = "engine (flags %d)" % flags
    cb = E.eval_callback(S.x, True)
    assert cb["rc"] == 0
    conb, jacb, rcb = E.eval_aero_all(np.tile(S.x, (9, 1)))
    assert rcb == 0
    used, over = {}, []
    for kind in KINDS:
        T = truth(S, kind)
        con, jv, rc = E.eval_aero(kind, S.x[None, :])
        assert finite_ok(rc, con, jv), ("status / finiteness", name, kind, flags, rc)
        assert (name, kind) not in NONFINITE_ROWS
        check_aero_values(S, T, con[0], what)
        keep, err = ~S.skip_rows, np.abs(con[0] - (1.0 - T.f))
        if (~keep).any():
            print("%s %s/%s, undecidable rows: max |f - truth| %.3e" % (what, name, kind, err[~keep].max()))
        nrow, nnz = E.aero_dims(kind)
        off = 0
        for v, var in enumerate(AERO_VARS):
            vals = jv[0, off:off + nnz[v]]
            off += nnz[v]
            ratio = aero_ratio(T, var, vals)
            if ratio.size:      # per phase (axis: per class)
                rows_ = T.coo_order(np.repeat(np.arange(len(T.lim))[:, None], T.jac[:, COLS[var]].shape[1], axis=1)).astype(int)
                used[(kind, var)] = [round(float(ratio[(rows_ >= r0) & (rows_ < r0 + nk)].max()), 4) for r0, nk in T.blocks]
            if ratio.size and ratio.max() > 1.0:
                rows = T.coo_order(np.repeat(np.arange(len(T.lim))[:, None], T.jac[:, COLS[var]].shape[1], axis=1)).astype(int)
                bad = np.unique(rows[ratio > 1.0])
                over.append("%s/%s: %.2f x aero_bound; rows %s, |v_air| there %s" % (kind, var, ratio.max(), bad.tolist(), S.vair[bad].tolist()))
            if var == "t" and flags == 0:
                assert not vals.any(), "the default form writes the exact t0 / tf columns: zeros"
            if (~keep).any() and vals.size:
                exact = T.coo_order(T.jac[:, COLS[var]])
                sk = T.coo_order(np.repeat(S.skip_rows[:, None], T.jac[:, COLS[var]].shape[1], axis=1)).astype(bool)
                print("%s %s/%s/%s, undecidable rows: max |entry - truth| %.3e (|truth| up to %.3e)" % (
                    what, name, kind, var, np.abs(vals - exact)[sk].max(), np.abs(exact)[sk].max()))
        # the callback's rows and the last slot of a batch: same bits
        assert np.array_equal(cb["aero_con"][kind], con[0]) and np.array_equal(cb["aero_jac"][kind], jv[0]), kind
        assert np.array_equal(conb[kind][8], con[0]) and np.array_equal(jacb[kind][8], jv[0]), kind
    print("%s %s: largest used fraction of aero_bound per (kind, block): %s" % (what, name, used))
    assert not over, "%s %s: |entry - exact| beyond aero_bound: %s" % (what, name, "; ".join(over))


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_fused_aero_rows_same_bits_and_status_ok_at_the_degenerate_states(name, monkeypatch):
    """eval_batch_aero_device with GEL_AERO_FUSED=1 (the AERO instantiation of the fused kernel where the launch form has one: not
    the split latency form, not two vectors per wavefront): bit-identical to eval_aero_all and eval_batch_device; every path GEL_OK
    and finite (gel_sync reports the status of the device-pointer calls)."""
    import oracle
    import torch
    from gelato_amd import Engine
    S = setup(name)
    prob, x, D = S.prob, S.x, S.D
    monkeypatch.setenv("GEL_AERO_FUSED", "1")   # read when the handle is created
    E = Engine(prob, D=D, tau=prob["tau"], barC20=oracle.BARC20_CPP)
    S_ = len(prob["num_nodes"])
    for kind in KINDS:
        E.aero_configure(kind, [(i, 1, LIMITS[kind]) for i in range(S_ - 1)])
    B = 132          # 132 vectors x 2 work items x 4 > 1024 wavefronts: not the split latency form
    info = E.launch_info(B)
    assert info[2] == 0, info
    X = np.tile(x, (B, 1))
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    dX = torch.from_numpy(X).to(dev)
    width, ocon, ojac = E.aero_record_layout()
    r1 = torch.empty((B, E.nres), dtype=torch.float64, device=dev)
    j1 = torch.empty((B, E.V), dtype=torch.float64, device=dev)
    a1 = torch.full((B, width), float("nan"), dtype=torch.float64, device=dev)
    E.eval_batch_aero_device(B, dX.data_ptr(), r1.data_ptr(), j1.data_ptr(), a1.data_ptr(), s)
    assert E.sync(s) == 0
    r0, j0 = torch.empty_like(r1), torch.empty_like(j1)
    E.eval_batch_device(B, dX.data_ptr(), r0.data_ptr(), j0.data_ptr(), s)
    assert E.sync(s) == 0
    assert torch.equal(r0.view(torch.int64), r1.view(torch.int64)) and torch.equal(j0.view(torch.int64), j1.view(torch.int64))
    assert bool(torch.isfinite(r0).all()) and bool(torch.isfinite(j0).all())
    con, jac, rc = E.eval_aero_all(X)
    assert rc == 0
    res, vals, rc1 = E.eval(x)
    assert finite_ok(rc1, res, vals)
    assert np.array_equal(res, r0[B - 1].cpu().numpy()) and np.array_equal(vals, E.expand(j0[B - 1].cpu().numpy()))
    a = a1.cpu().numpy()
    stored = np.unique(np.concatenate([idx[idx >= 0] for idx in list(ocon.values()) + list(ojac.values())]))
    assert np.isfinite(a[:, stored]).all(), "every cell of the aero record that the layout stores"
    for kind in KINDS:
        one_c, one_j, rck = E.eval_aero(kind, x[None, :])
        assert finite_ok(rck, one_c, one_j), (name, kind, rck)
        assert np.array_equal(E.aero_gather(a, ocon[kind]), con[kind]) and np.array_equal(E.aero_gather(a, ojac[kind]), jac[kind]), kind
        assert np.array_equal(con[kind][B - 1], one_c[0]) and np.array_equal(jac[kind][B - 1], one_j[0]), kind

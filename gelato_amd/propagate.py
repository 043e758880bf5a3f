"""The shooting check: an explicit integration of every section, independent of the collocation matrices.

The collocation error estimate (mesh_error.py) judges the collocation polynomial with the collocation method's own matrices.
The shooting check takes the controls the optimiser found, integrates the equations of motion with classical RK4 from each
section's first state (include/gelato_amd.h gel_propagate) and compares the trajectory with the collocated
states at the nodes.  It exposes a control polynomial that oscillates between its nodes, which the node values hide.  The
integration runs on the device (Engine.propagation_plan); this module turns it into one record per section.

fly() is the flight itself: ONE integration per decision vector from lift-off to the last node (the plan's chain mode), the state
carried across the knots with the collocated jump (a stage drop) added, optionally under per-vector dispersions of thrust, mass
flow, reference area and wind (sample_dispersion) -- the terminal miss of a solution and its Monte-Carlo spread.
"""
import numpy as np

from . import con_dynamics
from .engine import Engine, pack_x

GROUPS = ("mass", "position", "velocity", "quaternion")
GROUP_COLS = ((0, 1), (1, 4), (4, 7), (7, 11))


def _node_states(V, M):
    """[M, 11] (mass, position, velocity, quaternion per state node) of the state part of a packed vector"""
    return np.concatenate([V[0:M, None], V[M:4 * M].reshape(-1, 3), V[4 * M:7 * M].reshape(-1, 3), V[7 * M:11 * M].reshape(-1, 4)],
                          axis=1)


def shooting_check(xdict, pdict, unitdict, steps=4, engine=None):
    """One record per section of a solution xdict: {"name", "num_nodes", "steps": RK4 steps per node interval of the run the
    errors come from (2 * steps), "mass", "position", "velocity", "quaternion": the group errors of that run (max over the
    nodes and the group's components of |y - x| / (1 + max |x|)), "max": the largest of the four, "integrator_groups": per
    group the step-doubling estimate of RK4's own error in that run, max |y_steps - y_2steps| / 15 under the same
    normalisation, "integrator": the largest of them}.  A group error far above its integrator estimate is the collocation's;
    one at its level is RK4's: raise steps.  engine: an Engine of the same problem (one is created on device 0 otherwise).
    Raises if an output is NaN / Inf."""
    steps = int(steps)
    if steps < 1:
        raise ValueError("steps: at least 1")
    S = pdict["num_sections"]
    if engine is None:
        ps = pdict["ps_params"]
        engine = Engine(con_dynamics.problem_arrays(pdict, unitdict), D=[ps.D(i) for i in range(S)],
                        tau=[ps.tau(i) for i in range(S)])
    x = pack_x(xdict)
    runs = []
    for k in (steps, 2 * steps):
        plan = engine.propagation_plan(steps=k)
        try:
            Y, err, rc = plan.apply(x)
        finally:
            plan.close()
        if rc != 0:
            raise FloatingPointError("shooting check: non-finite output (status %d)" % rc)
        runs.append((Y[0], err[0]))
    (y1, _e1), (y2, err) = runs
    M = engine.M
    X, Y1, Y2 = _node_states(x, M), _node_states(y1, M), _node_states(y2, M)
    nn = [int(v) for v in engine.num_nodes]
    report = []
    for i in range(S):
        xa = sum(nn[:i]) + i
        rows = slice(xa, xa + nn[i] + 1)
        den = 1.0 + np.abs(X[rows]).max(axis=0)
        est = np.abs(Y1[rows] - Y2[rows]).max(axis=0) / den / 15.0
        rec = {"name": pdict["params"][i]["name"], "num_nodes": nn[i], "steps": 2 * steps}
        for g, k in enumerate(GROUPS):
            rec[k] = float(err[i, g])
        rec["max"] = max(rec[k] for k in GROUPS)
        rec["integrator_groups"] = {k: float(est[a:b].max()) for k, (a, b) in zip(GROUPS, GROUP_COLS)}
        rec["integrator"] = max(rec["integrator_groups"].values())
        report.append(rec)
    return report


def sample_dispersion(B, S, sigma, seed, per="vector"):
    """Factors [B, S, 4] (thrust, mass flow, reference area, wind) for PropagationPlan.apply / fly: 1 + sigma N(0, 1) per factor.
    sigma: one number or one per factor [4]; per="vector": one draw per vector and factor, the same in all its phases;
    per="phase": one per (vector, phase, factor).  numpy only, deterministic in seed; sigma = 0 gives exact ones."""
    if per not in ("vector", "phase"):
        raise ValueError("per: 'vector' or 'phase'")
    B, S = int(B), int(S)
    if B < 0 or S < 1:
        raise ValueError("B >= 0 and S >= 1")
    sg = np.asarray(sigma, dtype=np.float64)
    if sg.shape not in ((), (4,)) or not np.all(sg >= 0):
        raise ValueError("sigma: one non-negative number, or one per factor (4)")
    z = np.random.default_rng(seed).standard_normal((B, S if per == "phase" else 1, 4))
    return np.array(np.broadcast_to(1.0 + sg * z, (B, S, 4)), order="C")   # (an array of its own: writable, contiguous)


def assign_members(B, E, order="blocked", seed=0, own=0):
    """An assignment int32 [B] for WindEnsemble.assign: the first `own` flights get -1 (the engine's own wind table), the other
    B - own are spread over the E members so that the counts per member differ by at most one.
    order="blocked": flight j of those gets member j // ceil((B - own) / E) -- consecutive flights share a table, so a workgroup's
    lanes read few of them; "cyclic": j % E; "random": the cyclic assignment permuted, deterministic in seed.  numpy only."""
    if order not in ("blocked", "cyclic", "random"):
        raise ValueError("order: 'blocked', 'cyclic' or 'random'")
    B, E, own = int(B), int(E), int(own)
    if B < 0 or E < 1 or not 0 <= own <= B:
        raise ValueError("B >= 0, E >= 1 and 0 <= own <= B")
    n = B - own
    j = np.arange(n)
    if order == "blocked":
        # the first n % E members take ceil(n / E) flights, the others floor(n / E): with n a multiple of E this is j // (n / E)
        q, r = divmod(n, E)
        m = np.where(j < r * (q + 1), j // (q + 1), r + (j - r * (q + 1)) // max(q, 1))
    else:
        m = j % E
        if order == "random":
            m = np.random.default_rng(seed).permutation(m)
    return np.concatenate([np.full(own, -1), m]).astype(np.int32)


def fly(xdict_or_X, pdict, unitdict, steps=4, dispersion=None, engine=None, ensemble=None):
    """The flight of every decision vector: the controls integrated from lift-off to the last node in ONE chain
    (Engine.propagation_plan(restart="chain")), RK4 with 2 * steps steps per node interval.  xdict_or_X: a solution xdict, or
    packed vectors [B, nvars] / [nvars]; dispersion: None or [B, S, 4] (sample_dispersion); engine: an Engine of the same
    problem (one is created on device 0 from pdict / unitdict otherwise, which may be None when it is given); ensemble: None, or
    a WindEnsemble of that engine assigned B vectors (Engine.wind_ensemble, assign_members): every flight under its own wind table.
    -> {"steps": 2 * steps, "status": 0 or GEL_NONFINITE (a non-finite vector does not stop the others),
        "y" [B, 11 M]: the flown state at every state node, laid out like the state part of x,
        "err" [B, S, 4]: the accumulated flight error per section (mass, position, velocity, quaternion), |y - x| / (1 + max |x|);
                         its last row is the terminal miss in that normalisation,
        "integrator" [B, S, 4]: the step-doubling estimate of RK4's own share of err, max |y_steps - y_2steps| / 15 / (1 + max |x|),
        "x_flown" [B, nvars] = [y | u | t]: a decision vector that holds the flown states -- what Engine.rows_eval,
                         Engine.output_table and the aero constraints take,
        "terminal": {group: [B, 1 | 3 | 3 | 4]}: y - x at the last state node in physical units (kg, m, m/s, 1),
        "rows" [B, rows]: the engine's row table (orbit insertion errors, ...) at x_flown -- only where one is configured}"""
    steps = int(steps)
    if steps < 1:
        raise ValueError("steps: at least 1")
    if engine is None:
        S = pdict["num_sections"]
        ps = pdict["ps_params"]
        engine = Engine(con_dynamics.problem_arrays(pdict, unitdict), D=[ps.D(i) for i in range(S)],
                        tau=[ps.tau(i) for i in range(S)])
    X = pack_x(xdict_or_X) if isinstance(xdict_or_X, dict) else np.asarray(xdict_or_X, dtype=np.float64)
    X = np.ascontiguousarray(X).reshape(-1, engine.nvars)
    B, M, S = X.shape[0], engine.M, engine.S
    runs, status = [], 0
    for k in (steps, 2 * steps):
        plan = engine.propagation_plan(steps=k, restart="chain")
        try:
            Y, err, rc = plan.apply(X, dispersion=dispersion, ensemble=ensemble)
        finally:
            plan.close()
        status = max(status, rc)
        runs.append((Y, err))
    (Y1, _e1), (Y, err) = runs
    nn = [int(v) for v in engine.num_nodes]
    with np.errstate(invalid="ignore"):
        Xn = np.stack([_node_states(X[b], M) for b in range(B)]) if B else np.zeros((0, M, 11))
        d12 = np.abs(np.stack([_node_states(Y1[b], M) - _node_states(Y[b], M) for b in range(B)])) if B else np.zeros((0, M, 11))
        integ = np.zeros((B, S, 4))
        xa = 0
        for i in range(S):
            rows = slice(xa, xa + nn[i] + 1)
            den = 1.0 + np.abs(Xn[:, rows]).max(axis=1)
            est = d12[:, rows].max(axis=1) / den / 15.0
            for g, (a, b) in enumerate(GROUP_COLS):
                integ[:, i, g] = est[:, a:b].max(axis=1)
            xa += nn[i] + 1
    x_flown = X.copy()
    x_flown[:, :11 * M] = Y
    u = engine.units
    scale = (u[0], u[1], u[2], 1.0)
    last = M - 1
    idx = ([last], [M + 3 * last + c for c in range(3)], [4 * M + 3 * last + c for c in range(3)], [7 * M + 4 * last + c for c in range(4)])
    out = {"steps": 2 * steps, "status": int(status), "y": Y, "err": err, "integrator": integ, "x_flown": x_flown,
           "terminal": {k: (Y[:, ix] - X[:, ix]) * sc for k, ix, sc in zip(GROUPS, idx, scale)}}
    if engine._nlin + engine._nfn:
        con, _jfn, rc = engine.rows_eval(x_flown, want_jac=False)
        out["rows"] = con
        out["status"] = max(out["status"], int(rc))
    return out


JACOBIAN_GROUPS = ("initial", "dispersion", "times", "controls_bias")
_STATE_NAMES = ("mass", "x", "y", "z", "vx", "vy", "vz", "q0", "q1", "q2", "q3")
_FACTOR_NAMES = ("thrust", "massflow", "area", "wind")


def jacobian_seeds(num_nodes, attitude_hold, wrt=("initial", "dispersion", "times")):
    """The shared unit seeds of flight_jacobian for phases of num_nodes nodes -> (columns [P] names, dX [P, nvars], dD [P, S, 4]).
    "initial": the 11 lift-off components (state row 0); "dispersion": the 4 S factors, phase-major; "times": the S + 1 knot
    times; "controls_bias": per free-attitude phase and control one constant direction (all its nodes 1).  numpy only."""
    nn = [int(v) for v in num_nodes]
    S, N = len(nn), sum(nn)
    M = N + S
    nvars = 11 * M + 2 * N + S + 1
    wrt = tuple(wrt)
    if not wrt or any(g not in JACOBIAN_GROUPS for g in wrt) or len(set(wrt)) != len(wrt):
        raise ValueError("wrt: distinct groups of %r" % (JACOBIAN_GROUPS,))
    cols, rows = [], []          # rows: (index array into dx or None, (phase, factor) or None)
    for g in wrt:
        if g == "initial":
            off = (0, M, M + 1, M + 2, 4 * M, 4 * M + 1, 4 * M + 2, 7 * M, 7 * M + 1, 7 * M + 2, 7 * M + 3)
            for c in range(11):
                cols.append("initial:%s" % _STATE_NAMES[c]); rows.append((np.array([off[c]]), None))
        elif g == "dispersion":
            for s in range(S):
                for f in range(4):
                    cols.append("dispersion:%s[%d]" % (_FACTOR_NAMES[f], s)); rows.append((None, (s, f)))
        elif g == "times":
            for i in range(S + 1):
                cols.append("time[%d]" % i); rows.append((np.array([11 * M + 2 * N + i]), None))
        else:
            for s in range(S):
                if attitude_hold[s]:
                    continue
                ua = sum(nn[:s])
                for c in range(2):
                    cols.append("u%d_bias[%d]" % (c, s)); rows.append((11 * M + 2 * (ua + np.arange(nn[s])) + c, None))
    P = len(cols)
    dX, dD = np.zeros((P, nvars)), np.zeros((P, S, 4))
    for p, (ix, sf) in enumerate(rows):
        if ix is not None:
            dX[p, ix] = 1.0
        else:
            dD[p, sf[0], sf[1]] = 1.0
    return cols, dX, dD


def flight_jacobian(xdict_or_X, pdict, unitdict, steps=4, wrt=("initial", "dispersion", "times"), dispersion=None, engine=None,
                    ensemble=None):
    """The exact Jacobian of the flight fly() reports (one chain, RK4 with 2 * steps steps per node interval) with respect to the
    lift-off state, the 4 S dispersion factors, the S + 1 knot times and optionally a constant bias of every free phase's controls
    (wrt; jacobian_seeds): the tangent-linear propagation (PropagationPlan.tangent) along shared unit seeds --
    derivatives of the discrete map, without sampling noise, where montecarlo.dispersion_sensitivity regresses over a batch.
    ensemble: None, or a WindEnsemble of the engine assigned B vectors, as fly() takes it: every vector's flight and its derivative
    under the wind table its entry selects.  B vectors under B members give one Jacobian per sounding, each of
    which feeds the linear covariance of that day's insertion state:
        ens = engine.wind_ensemble(soundings); ens.assign(np.arange(B))
        J = flight_jacobian(np.tile(x, (B, 1)), None, None, wrt=("dispersion",), engine=engine, ensemble=ens)
        cov = [montecarlo.linear_covariance(J["terminal"]["velocity"][b], sigma) for b in range(B)]
    -> {"columns": names [P], "status", "y" [B, 11 M], "dy" [B, P, 11 M], "x_flown" [B, nvars],
        "terminal": {group: [B, 1 | 3 | 3 | 4, P]}: the last state node's derivative in physical units (kg, m, m/s, 1),
        "rows" [B, R, P]: the engine's row table's derivative, Engine.con_matvec applied to [dy | du | dt] at x_flown -- only
                          where a row table is configured}"""
    steps = int(steps)
    if steps < 1:
        raise ValueError("steps: at least 1")
    if engine is None:
        S = pdict["num_sections"]
        ps = pdict["ps_params"]
        engine = Engine(con_dynamics.problem_arrays(pdict, unitdict), D=[ps.D(i) for i in range(S)],
                        tau=[ps.tau(i) for i in range(S)])
    X = pack_x(xdict_or_X) if isinstance(xdict_or_X, dict) else np.asarray(xdict_or_X, dtype=np.float64)
    X = np.ascontiguousarray(X).reshape(-1, engine.nvars)
    B, M = X.shape[0], engine.M
    cols, dX, dD = jacobian_seeds(engine.num_nodes, engine.prob["attitude_hold"], wrt)
    P = len(cols)
    plan = engine.propagation_plan(steps=2 * steps, restart="chain")
    try:
        Y, dY, rc = plan.tangent(X, dX=dX if dX.any() else None, dispersion=dispersion, ddispersion=dD if dD.any() else None, shared=True,
                                 ensemble=ensemble)
    finally:
        plan.close()
    x_flown = X.copy()
    x_flown[:, :11 * M] = Y
    u = engine.units
    scale = (u[0], u[1], u[2], 1.0)
    last = M - 1
    idx = ([last], [M + 3 * last + c for c in range(3)], [4 * M + 3 * last + c for c in range(3)], [7 * M + 4 * last + c for c in range(4)])
    out = {"columns": cols, "status": int(rc), "y": Y, "dy": dY, "x_flown": x_flown,
           "terminal": {k: np.swapaxes(dY[:, :, ix], 1, 2) * sc for k, ix, sc in zip(GROUPS, idx, scale)}}
    if engine._nlin + engine._nfn:
        _con, jfn, rc2 = engine.rows_eval(x_flown, want_jac=True)
        V = np.broadcast_to(dX[None], (B, P, engine.nvars)).copy()    # [dy | du | dt]: the seeds' own control and time parts
        V[:, :, :11 * M] = dY
        jf = np.ascontiguousarray(np.broadcast_to(jfn[:, None], (B, P) + jfn.shape[1:]))
        r, rc3 = engine.con_matvec(V, jfn=jf)
        out["rows"] = np.swapaxes(r, 1, 2)
        out["status"] = max(out["status"], int(rc2), int(rc3))
    return out


GRADIENT_OF = ("terminal", "rows")


def flight_gradient(xdict_or_X, pdict, unitdict, steps=4, of=("terminal",), dispersion=None, engine=None, ensemble=None, wind=False):
    """The gradients of functionals of the flight fly() reports (one chain, RK4 with 2 * steps steps per node interval) with respect to
    EVERY input in one backward pass: the adjoint flight (PropagationPlan.adjoint), where flight_jacobian pays one
    lane per column.  of = ("terminal",): the 11 components of the last state node in physical units (kg, m, m/s, 1);
    of = ("rows", mu): mu [R] or [Q, R] multipliers on the engine's row table at x_flown -- Engine.con_rmatvec carries them to
    [dy | du | dt]: the state part becomes the functional's weights on y, the u and t parts are added to the result (the mirror of
    what flight_jacobian does with con_matvec).
    ensemble: None, or a WindEnsemble of the engine assigned B vectors, as fly() takes it: the flight that yields x_flown and the
    adjoint both run under every vector's own wind table.  The row table and con_rmatvec are evaluated AT x_flown
    and read no wind table, so of=("rows", mu) passes through them unchanged: the ensemble enters through x_flown alone.
    -> {"functionals": names [Q], "status", "y" [B, 11 M], "x_flown" [B, nvars],
        "gx" [B, Q, nvars]: the gradient with respect to the decision vector (its own units): the lift-off state, both state rows of
                            every knot, ALL controls and the knot times; +0.0 where the flight does not read x,
        "gdisp" [B, Q, S, 4]: with respect to the factors,
        "columns" names [P] and "jacobian" [B, Q, P]: the entries flight_jacobian's columns name (jacobian_seeds with all four groups:
                            "initial:*", "dispersion:*[s]", "time[i]", and "u*_bias[s]" = the sum over the phase's nodes)}
    wind=True adds the gradient with respect to the VALUES of the wind table every flight reads:
        "gwind" [B, Q, Kg, 2]: north and east per row, in the functional's units per m/s (scaled like gx for of=("terminal",)); rows
                            beyond a vector's own table and rows no stage touched are zero,
        "wind_altitudes":   the rows' altitudes: [Kg] the engine's table's, or under an ensemble [B, Kg] those of every vector's
                            member (NaN beyond its rows).  montecarlo.wind_linear_prediction reads both."""
    steps = int(steps)
    if steps < 1:
        raise ValueError("steps: at least 1")
    of = tuple(of) if isinstance(of, (tuple, list)) else (of,)
    if not of or of[0] not in GRADIENT_OF or len(of) != (1 if of[0] == "terminal" else 2):
        raise ValueError('of: ("terminal",) or ("rows", mu)')
    if engine is None:
        S = pdict["num_sections"]
        ps = pdict["ps_params"]
        engine = Engine(con_dynamics.problem_arrays(pdict, unitdict), D=[ps.D(i) for i in range(S)],
                        tau=[ps.tau(i) for i in range(S)])
    X = pack_x(xdict_or_X) if isinstance(xdict_or_X, dict) else np.asarray(xdict_or_X, dtype=np.float64)
    X = np.ascontiguousarray(X).reshape(-1, engine.nvars)
    B, M, nv = X.shape[0], engine.M, engine.nvars
    plan = engine.propagation_plan(steps=2 * steps, restart="chain")
    try:
        status, extra = 0, None
        if of[0] == "terminal":
            u = engine.units
            last = M - 1
            idx = [last] + [M + 3 * last + c for c in range(3)] + [4 * M + 3 * last + c for c in range(3)] + [7 * M + 4 * last + c for c in range(4)]
            scale = np.array([u[0]] + [u[1]] * 3 + [u[2]] * 3 + [1.0] * 4)
            names = ["terminal:%s" % n for n in _STATE_NAMES]
            lam = np.zeros((11, 11 * M))
            lam[np.arange(11), idx] = 1.0
            shared = True
        else:
            if not engine._nlin + engine._nfn:
                raise ValueError('of=("rows", mu): the engine has no row table')
            mu = np.asarray(of[1], dtype=np.float64)
            R = engine._nlin + engine._nfn
            if mu.ndim not in (1, 2) or mu.shape[-1] != R:
                raise ValueError("mu: [R] or [Q, R] with R = %d rows" % R)
            mu = mu.reshape(-1, R)
            Q = mu.shape[0]
            names = ["rows:mu[%d]" % q for q in range(Q)]
            Y0, _err, rc0 = plan.apply(X, want_err=False, dispersion=dispersion, ensemble=ensemble)
            x_fl = X.copy()
            x_fl[:, :11 * M] = Y0
            _con, jfn, rc1 = engine.rows_eval(x_fl, want_jac=True)
            jf = np.ascontiguousarray(np.broadcast_to(jfn[:, None], (B, Q) + jfn.shape[1:]))
            g, rc2 = engine.con_rmatvec(np.ascontiguousarray(np.broadcast_to(mu[None], (B, Q, R))), jfn=jf)
            status = max(int(rc0), int(rc1), int(rc2))
            lam = np.ascontiguousarray(g[:, :, :11 * M])
            extra = g[:, :, 11 * M:]          # the rows' own dependence on u and t
            scale = np.ones(Q)
            shared = False
        GW = None
        if wind:
            Y, GX, GD, rc, GW = plan.adjoint(X, lam, dispersion=dispersion, shared=shared, ensemble=ensemble, want_wind=True)
        else:
            Y, GX, GD, rc = plan.adjoint(X, lam, dispersion=dispersion, shared=shared, ensemble=ensemble)
    finally:
        plan.close()
    GX = GX * scale[None, :, None]
    GD = GD * scale[None, :, None, None]
    if extra is not None:
        GX[:, :, 11 * M:] += extra
    x_flown = X.copy()
    x_flown[:, :11 * M] = Y
    cols, dX, dD = jacobian_seeds(engine.num_nodes, engine.prob["attitude_hold"], JACOBIAN_GROUPS)
    jac = np.einsum("bqv,pv->bqp", GX, dX) + np.einsum("bqsf,psf->bqp", GD, dD)
    out = {"functionals": names, "status": max(status, int(rc)), "y": Y, "x_flown": x_flown, "gx": GX, "gdisp": GD, "columns": cols,
           "jacobian": jac}
    if wind:
        out["gwind"] = GW * scale[None, :, None, None]
        own = engine.wind_altitudes
        Kg = GW.shape[2]
        if ensemble is None:
            out["wind_altitudes"] = own.copy()
        else:
            alt = np.full((B, Kg), np.nan)
            rows = {-1: own}
            for b, e in enumerate(ensemble.members):
                e = int(e)
                if e not in rows:
                    rows[e] = ensemble.member(e)["rows"][:, 0].copy()
                alt[b, :rows[e].size] = rows[e]
            out["wind_altitudes"] = alt
    return out

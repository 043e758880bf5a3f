"""The Monte-Carlo look at a solution: fly a dispersed batch and read its post-processing table as an envelope.

propagate.fly integrates every decision vector from lift-off to the last node under per-vector dispersions of thrust, mass flow,
reference area and wind.  flight_envelope() takes the flown states and asks the batched output table (Engine.output_table_batch,
include/gelato_amd.h gel_output_table_batch) for what a launch-vehicle user wants of such a batch: per node the
spread of max-Q, q-alpha, Mach, altitude, the impact point and the orbit over the flights, and the peak of every flight -- formed
with the SAME factors the flight was flown with (the dispersed wind is the wind of the dynamic pressure).  flight_quantiles() reads
the same batch by exact percentiles over the flights (Engine.batch_quantiles_device, gel_batch_quantiles), with the
table kept on the device.  flight_covariance() reads it by co-moments (Engine.batch_comoments_device, gel_batch_comoments, DESIGN.md
3.18): the covariance of the terminal row, and through dispersion_sensitivity() the regression of the outputs on the factors flown.
"""
import numpy as np

from . import con_dynamics
from .engine import Engine, pack_x


def flight_envelope(xdict_or_X, pdict, unitdict, dispersion=None, steps=4, columns=None, engine=None, ensemble=None):
    """xdict_or_X: a solution xdict or packed vectors [B, nvars] / [nvars]; dispersion: None or [B, S, 4]
    (propagate.sample_dispersion); steps: as propagate.fly; ONE chain run with 2 * steps RK4 steps per node interval, the run fly's y and err
    come from; columns: None (all of Engine.OUTPUT_COLUMNS) or a list of names; engine: an Engine of the same problem (one is
    created on device 0 otherwise); ensemble: None, or a WindEnsemble of that engine assigned B vectors: the flight AND the table of
    every vector take the wind table its entry selects (flight_quantiles and flight_covariance take it alike).
    -> {"steps": 2 * steps, "status": 0 or GEL_NONFINITE (of the flight and the row table; the output table reports its own
        non-finite entries through count / first_nonfinite), "columns": names,
        "envelope", "peaks": as Engine.output_table_batch returns them, at x_flown,
        "terminal_miss" [B, 4]: the last row of fly's err (mass, position, velocity, quaternion),
        "x_flown" [B, nvars], "rows" [B, rows]: the engine's row table at x_flown -- only where one is configured}"""
    if engine is None:
        S = pdict["num_sections"]
        ps = pdict["ps_params"]
        engine = Engine(con_dynamics.problem_arrays(pdict, unitdict), D=[ps.D(i) for i in range(S)],
                        tau=[ps.tau(i) for i in range(S)])
    steps = int(steps)
    if steps < 1:
        raise ValueError("steps: at least 1")
    X = pack_x(xdict_or_X) if isinstance(xdict_or_X, dict) else np.asarray(xdict_or_X, dtype=np.float64)
    X = np.ascontiguousarray(X).reshape(-1, engine.nvars)
    # fly's chain plan, the run that counts alone (fly's second run only estimates the integrator's share of err)
    plan = engine.propagation_plan(steps=2 * steps, restart="chain")
    try:
        Y, err, status = plan.apply(X, dispersion=dispersion, ensemble=ensemble)
    finally:
        plan.close()
    x_flown = X.copy()
    x_flown[:, :11 * engine.M] = Y
    lc = pdict["LaunchCondition"]
    T = engine.output_table_batch(x_flown, lc["lat"], lc["lon"], dispersion=dispersion, columns=columns, table=False, ensemble=ensemble)
    out = {"steps": 2 * steps, "status": int(status), "columns": T["columns"], "envelope": T["envelope"], "peaks": T["peaks"],
           "terminal_miss": err[:, -1], "x_flown": x_flown}
    if engine._nlin + engine._nfn:
        con, _jfn, rc = engine.rows_eval(x_flown, want_jac=False)
        out["rows"] = con
        out["status"] = max(out["status"], int(rc))
    return out


def flight_quantiles(xdict_or_X, pdict, unitdict, probs, dispersion=None, steps=4, columns=None, engine=None, ensemble=None):
    """The same flight as flight_envelope, read by exact quantiles over the flights (Engine.batch_quantiles_device, include/gelato_amd.h
    gel_batch_quantiles).  The flown states, the table [B, M, ncols] and the peaks stay on the device; only results of
    the size [M][ncols][nq] come back.  probs: 1 .. 16 probabilities in [0, 1]; the other arguments as flight_envelope takes them.
    -> {"steps": 2 * steps, "status": 0 or GEL_NONFINITE (of the flight), "columns": names, "probs" [nq],
        "node": {name: {"lower", "upper", "value" [M, nq], "count" [M] int}}   -- per node over the flights,
        "peak": {name: {"min": {...}, "max": {...}}}, each {"lower", "upper", "value" [nq], "count" int, "who_lower", "who_upper" [nq]
                 int}   -- over the flights, of every flight's minimum / maximum over its nodes; who: the flight that is that case,
        "terminal_miss": {"lower", "upper", "value" [4, nq], "count" [4] int}   -- of the last row of fly's err}"""
    import torch
    if engine is None:
        S = pdict["num_sections"]
        ps = pdict["ps_params"]
        engine = Engine(con_dynamics.problem_arrays(pdict, unitdict), D=[ps.D(i) for i in range(S)],
                        tau=[ps.tau(i) for i in range(S)])
    steps = int(steps)
    if steps < 1:
        raise ValueError("steps: at least 1")
    p = engine._quantile_probs(probs)
    names, _ids = engine._output_columns(columns)
    X = pack_x(xdict_or_X) if isinstance(xdict_or_X, dict) else np.asarray(xdict_or_X, dtype=np.float64)
    X = np.ascontiguousarray(X).reshape(-1, engine.nvars)
    B, M, S, nc, nq = X.shape[0], engine.M, engine.S, len(names), p.size
    d_disp = None
    if dispersion is not None:
        disp = np.asarray(dispersion)
        if disp.dtype != np.float64:
            raise TypeError("dispersion: float64")
        if disp.shape == (S, 4) and B == 1:
            disp = disp[None]
        if disp.shape != (B, S, 4):
            raise ValueError("dispersion: [B, S, 4] = %s, not %s" % ((B, S, 4), disp.shape))
        d_disp = torch.from_numpy(np.ascontiguousarray(disp)).cuda()

    def buf(*shape):
        return torch.empty(shape, dtype=torch.float64, device="cuda")
    d_x = torch.from_numpy(X).cuda()
    d_y, d_err = buf(B, 11 * M), buf(B, S, 4)
    d_table, d_peaks = buf(B, M, nc), buf(B, nc, 4)
    q_node, c_node = buf(M * nc, nq, 2), buf(M * nc)
    q_peak, c_peak, w_peak = buf(nc * 4, nq, 2), buf(nc * 4), buf(nc * 4, nq, 2)
    q_miss, c_miss = buf(4, nq, 2), buf(4)
    dptr = d_disp.data_ptr() if d_disp is not None else 0
    plan = engine.propagation_plan(steps=2 * steps, restart="chain")
    try:
        plan.apply_device(B, d_x.data_ptr(), d_y.data_ptr(), d_err.data_ptr(), dptr, ensemble=ensemble)
        d_x[:, :11 * M] = d_y          # x_flown; the null stream orders itself against the engine's blocking stream
        lc = pdict["LaunchCondition"]
        engine.output_table_batch_device(B, d_x.data_ptr(), lc["lat"], lc["lon"], d_dispersion=dptr, columns=columns,
                                         d_out=d_table.data_ptr(), d_peaks=d_peaks.data_ptr(), ensemble=ensemble)
        engine.batch_quantiles_device(B, M * nc, M * nc, d_table.data_ptr(), p, q_node.data_ptr(), c_node.data_ptr())
        engine.batch_quantiles_device(B, nc * 4, nc * 4, d_peaks.data_ptr(), p, q_peak.data_ptr(), c_peak.data_ptr(), w_peak.data_ptr())
        engine.batch_quantiles_device(B, 4, S * 4, d_err.data_ptr() + 8 * (S - 1) * 4, p, q_miss.data_ptr(), c_miss.data_ptr())
        status = engine.sync()
    finally:
        plan.close()

    def read(q, c, shape):
        q, c = q.cpu().numpy().reshape(shape + (nq, 2)), c.cpu().numpy().reshape(shape).astype(np.int64)
        lower, upper = np.ascontiguousarray(q[..., 0]), np.ascontiguousarray(q[..., 1])
        return {"lower": lower, "upper": upper, "value": engine.quantile_value(p, c, lower, upper), "count": c}
    node, peak, miss = read(q_node, c_node, (M, nc)), read(q_peak, c_peak, (nc, 4)), read(q_miss, c_miss, (4,))
    who = w_peak.cpu().numpy().reshape(nc, 4, nq, 2).astype(np.int64)
    out = {"steps": 2 * steps, "status": int(status), "columns": names, "probs": p, "node": {}, "peak": {}, "terminal_miss": miss}
    for k, name in enumerate(names):
        out["node"][name] = {f: v[:, k] for f, v in node.items()}
        out["peak"][name] = {}
        for j, side in ((0, "min"), (2, "max")):       # Engine.PEAK_FIELDS: min, argmin, max, argmax
            d = {f: v[k, j] for f, v in peak.items()}
            d["count"] = int(d["count"])
            d["who_lower"], d["who_upper"] = who[k, j, :, 0], who[k, j, :, 1]
            out["peak"][name][side] = d
    return out


def dispersion_sensitivity(count, C_dd, C_dy, m2_y):
    """The regression of outputs y on the dispersion factors d from their co-moments (host numpy; Engine.batch_comoments).
    count: the flights counted; C_dd [K, K]: the factors' self co-moments; C_dy [K, J]: factors x outputs; m2_y [J].
    Active factors are the k with C_dd[k][k] > 0.  beta [K, J]: the minimum-norm least-squares solution of
    C_dd[act, act] beta = C_dy[act] (np.linalg.lstsq, default rcond); the rows of inactive factors are 0.
    -> {"count", "active" [K] bool, "beta" [K, J] (dy / dd), "explained" [J] = (beta_j . C_dy[act, j]) / m2_y[j]: the part of y_j's
        spread the linear model carries, "share" [K, J] = beta_kj^2 C_dd[k][k] / m2_y[j]: factor k's part alone (the shares add up
        to explained where the factors are uncorrelated)}; explained and share are NaN where m2_y[j] = 0."""
    C_dd, C_dy, m2_y = (np.asarray(v, dtype=np.float64) for v in (C_dd, C_dy, m2_y))
    K, J = C_dy.shape
    if C_dd.shape != (K, K) or m2_y.shape != (J,):
        raise ValueError("C_dd [K, K], C_dy [K, J], m2_y [J]: %s, %s, %s" % (C_dd.shape, C_dy.shape, m2_y.shape))
    var = np.diagonal(C_dd)
    act = var > 0.0
    beta = np.zeros((K, J))
    if act.any() and J:
        beta[act] = np.linalg.lstsq(C_dd[np.ix_(act, act)], C_dy[act], rcond=None)[0]
    ok = m2_y != 0.0
    den = np.where(ok, m2_y, 1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        explained = np.where(ok, np.einsum("kj,kj->j", beta[act], C_dy[act]) / den, np.nan)
        share = np.where(ok[None, :], beta * beta * var[:, None] / den[None, :], np.nan)
    return {"count": int(count), "active": act, "beta": beta, "explained": explained, "share": share}


def flight_covariance(xdict_or_X, pdict, unitdict, dispersion, steps=4, columns=None, engine=None, ensemble=None):
    """The same flight as flight_quantiles, read by co-moments over the flights (Engine.batch_comoments_device, include/gelato_amd.h
    gel_batch_comoments).  The flown states, the table and the peaks stay on the device; the calls read them as
    views.  dispersion: [B, S, 4], required; the other arguments as flight_envelope takes them.
    Every call counts LISTWISE: a flight counts only if every entry the call reads of it is finite.  The default columns=None
    selects all 34 columns, and so excludes every flight at a node where any column is NaN (e.g. no impact point once the stage is
    in orbit): the listwise exclusion is the caller's to steer, by choosing columns that are finite.
    -> {"steps": 2 * steps, "status": 0 or GEL_NONFINITE (of the flight), "columns": names,
        "terminal": the self form over the last node's row of the selected columns [nc, nc],
        "dispersion": the self form over the 4 S factors,
        "sensitivity": {"terminal" (disp x the last node's row), "peak_max" (disp x every flight's maximum of every column),
                        "terminal_miss" (disp x the last row of fly's err)},
        every one of the five a dict {"count", "first_excluded", "C", "mean_a", "m2_a", "mean_b", "m2_b", "cov", "corr"} as
        Engine.batch_comoments returns it; the three of "sensitivity" also hold "beta", "explained", "share", "active" of
        dispersion_sensitivity(count, C_dd of "dispersion", C, m2_b).  (C_dd is that of every flight with finite factors: where a
        group's own count is lower, choose columns that are finite in every flight.)}"""
    import torch
    if engine is None:
        S = pdict["num_sections"]
        ps = pdict["ps_params"]
        engine = Engine(con_dynamics.problem_arrays(pdict, unitdict), D=[ps.D(i) for i in range(S)],
                        tau=[ps.tau(i) for i in range(S)])
    steps = int(steps)
    if steps < 1:
        raise ValueError("steps: at least 1")
    names, _ids = engine._output_columns(columns)
    X = pack_x(xdict_or_X) if isinstance(xdict_or_X, dict) else np.asarray(xdict_or_X, dtype=np.float64)
    X = np.ascontiguousarray(X).reshape(-1, engine.nvars)
    B, M, S, nc = X.shape[0], engine.M, engine.S, len(names)
    if dispersion is None:
        raise ValueError("dispersion: [B, S, 4] is required")
    disp = np.asarray(dispersion)
    if disp.dtype != np.float64:
        raise TypeError("dispersion: float64")
    if disp.shape == (S, 4) and B == 1:
        disp = disp[None]
    if disp.shape != (B, S, 4):
        raise ValueError("dispersion: [B, S, 4] = %s, not %s" % ((B, S, 4), disp.shape))
    d_disp = torch.from_numpy(np.ascontiguousarray(disp)).cuda()

    def buf(*shape):
        return torch.empty(shape, dtype=torch.float64, device="cuda")
    d_x = torch.from_numpy(X).cuda()
    d_y, d_err = buf(B, 11 * M), buf(B, S, 4)
    d_table, d_peaks = buf(B, M, nc), buf(B, nc, 4)
    K = 4 * S
    # (a view, its width, inc, ld) of every b side; None: the self form
    term = (d_table.data_ptr() + 8 * (M - 1) * nc, nc, 1, M * nc)
    views = {"terminal": (term, None), "dispersion": ((d_disp.data_ptr(), K, 1, K), None),
             "s_terminal": ((d_disp.data_ptr(), K, 1, K), term),
             "s_peak_max": ((d_disp.data_ptr(), K, 1, K), (d_peaks.data_ptr() + 8 * 2, nc, 4, 4 * nc)),
             "s_terminal_miss": ((d_disp.data_ptr(), K, 1, K), (d_err.data_ptr() + 8 * (S - 1) * 4, 4, 1, 4 * S))}
    outs = {}
    plan = engine.propagation_plan(steps=2 * steps, restart="chain")
    try:
        plan.apply_device(B, d_x.data_ptr(), d_y.data_ptr(), d_err.data_ptr(), d_disp.data_ptr(), ensemble=ensemble)
        d_x[:, :11 * M] = d_y          # x_flown; the null stream orders itself against the engine's blocking stream
        lc = pdict["LaunchCondition"]
        engine.output_table_batch_device(B, d_x.data_ptr(), lc["lat"], lc["lon"], d_dispersion=d_disp.data_ptr(), columns=columns,
                                         d_out=d_table.data_ptr(), d_peaks=d_peaks.data_ptr(), ensemble=ensemble)
        for key, (va, vb) in views.items():
            Wa, Wb = va[1], (va[1] if vb is None else vb[1])
            o = (buf(Wa, Wb), buf(Wa, 2), None if vb is None else buf(Wb, 2), buf(2))
            pb, wb, ib, lb = (0, 0, 1, 1) if vb is None else vb
            engine.batch_comoments_device(B, Wa, va[2], va[3], va[0], wb, ib, lb, pb, o[0].data_ptr(), o[1].data_ptr(),
                                          0 if o[2] is None else o[2].data_ptr(), o[3].data_ptr())
            outs[key] = o
        status = engine.sync()
    finally:
        plan.close()

    def read(o):
        Cm, sa, info = o[0].cpu().numpy(), o[1].cpu().numpy(), o[3].cpu().numpy()
        sb = sa if o[2] is None else o[2].cpu().numpy()
        count = int(info[0])
        cov, corr = engine.comoment_ratios(count, Cm, sa[:, 1], sb[:, 1])
        return {"count": count, "first_excluded": int(info[1]), "C": Cm, "mean_a": sa[:, 0].copy(), "m2_a": sa[:, 1].copy(),
                "mean_b": sb[:, 0].copy(), "m2_b": sb[:, 1].copy(), "cov": cov, "corr": corr}
    res = {k: read(o) for k, o in outs.items()}
    out = {"steps": 2 * steps, "status": int(status), "columns": names, "terminal": res["terminal"], "dispersion": res["dispersion"],
           "sensitivity": {}}
    for g in ("terminal", "peak_max", "terminal_miss"):
        r = res["s_" + g]
        sens = dispersion_sensitivity(r["count"], res["dispersion"]["C"], r["C"], r["m2_b"])
        r.update({k: sens[k] for k in ("active", "beta", "explained", "share")})
        out["sensitivity"][g] = r
    return out


def availability_from_peaks(peaks, members, limits, E=None):
    """The launch-availability record of a batch flown against a wind ensemble, from every flight's peaks (host numpy; no GPU).
    peaks: {column: {"min", "argmin", "max", "argmax" [B]}} as Engine.output_table_batch returns them; members: int [B], the member
    0 .. E - 1 every flight flew under (several flights per member: its replicas); limits: {column: upper} or {column: (lower,
    upper)}, either bound None for none; E: the number of members (default: max(members) + 1).  Every member needs a flight.
    Per limited column and member, over the member's flights in ascending order: the worst (largest) maximum and the worst
    (smallest) minimum, NaN peaks left out, with the FIRST flight that holds each and its node.  A member is ok when every one of
    its flights has finite peaks in every limited column, worst_max <= upper and worst_min >= lower.
    -> {"columns": the limited columns, "limits": {column: (lower | None, upper | None)},
        "worst_max", "worst_min": {column: [E]}, "flight_max", "node_max", "flight_min", "node_min": {column: [E] int (-1: none)},
        "ok" [E] bool, "ok_by_column": {column: [E] bool}, "availability": ok.sum() / E, "failing": the members that are not ok}"""
    members = np.asarray(members)
    if members.ndim != 1 or (members.size and not np.issubdtype(members.dtype, np.integer)):
        raise ValueError("members: integers [B]")
    B = members.size
    if B == 0 or members.min() < 0:
        raise ValueError("members: at least one flight, every flight under a member 0 .. E - 1")
    E = int(members.max()) + 1 if E is None else int(E)
    if members.max() >= E:
        raise ValueError("members: an entry >= E = %d" % E)
    if np.bincount(members, minlength=E).min() == 0:
        raise ValueError("members: every member needs at least one flight")
    if not limits:
        raise ValueError("limits: at least one limited column")
    lim = {}
    for name, v in limits.items():
        if name not in peaks:
            raise ValueError("limits: no peaks of column %r" % (name,))
        lo, up = v if isinstance(v, (tuple, list)) else (None, v)
        lo, up = (None if lo is None else float(lo)), (None if up is None else float(up))
        if (lo is not None and lo != lo) or (up is not None and up != up) or (lo is None and up is None):
            raise ValueError("limits[%r]: upper, or (lower, upper), numbers, at least one of them" % (name,))
        lim[name] = (lo, up)
    out = {"columns": list(lim), "limits": lim, "ok_by_column": {}}
    for k in ("worst_max", "worst_min", "flight_max", "node_max", "flight_min", "node_min"):
        out[k] = {}
    ok = np.ones(E, dtype=bool)
    flights = np.arange(B)
    for name, (lo, up) in lim.items():
        pk = peaks[name]
        vmax, vmin = np.asarray(pk["max"], dtype=np.float64), np.asarray(pk["min"], dtype=np.float64)
        if vmax.shape != (B,) or vmin.shape != (B,):
            raise ValueError("peaks[%r]: [B] = [%d]" % (name, B))
        wmax, wmin = np.full(E, np.nan), np.full(E, np.nan)
        fmax, fmin = np.full(E, -1, dtype=np.int64), np.full(E, -1, dtype=np.int64)
        nmax, nmin = fmax.copy(), fmin.copy()
        okc = np.ones(E, dtype=bool)
        for e in range(E):
            fl = flights[members == e]
            fin = np.isfinite(vmax[fl]) & np.isfinite(vmin[fl])
            okc[e] = bool(fin.all())
            if fin.any():
                g = fl[fin]
                i, j = g[np.argmax(vmax[g])], g[np.argmin(vmin[g])]      # (argmax / argmin: the first that attains it)
                wmax[e], fmax[e], nmax[e] = vmax[i], i, int(np.asarray(pk["argmax"])[i])
                wmin[e], fmin[e], nmin[e] = vmin[j], j, int(np.asarray(pk["argmin"])[j])
                if up is not None and not wmax[e] <= up:
                    okc[e] = False
                if lo is not None and not wmin[e] >= lo:
                    okc[e] = False
        out["worst_max"][name], out["worst_min"][name] = wmax, wmin
        out["flight_max"][name], out["node_max"][name], out["flight_min"][name], out["node_min"][name] = fmax, nmax, fmin, nmin
        out["ok_by_column"][name] = okc
        ok &= okc
    out["ok"] = ok
    out["availability"] = float(ok.sum()) / E
    out["failing"] = np.flatnonzero(~ok)
    return out


def wind_availability(xdict_or_x, pdict, unitdict, wind_tables, limits, replicas=1, sigma=0.0, seed=0, steps=4, engine=None):
    """Launch availability of ONE trajectory over an ensemble of wind profiles: the share of profiles under which the flight keeps
    its limits.  xdict_or_x: a solution xdict or one packed vector [nvars]; wind_tables: float64 [E, Kw, 3] (Engine.wind_ensemble);
    limits: {column of Engine.OUTPUT_COLUMNS: upper} or {column: (lower, upper)}; replicas: flights per member, B = E replicas
    flights blocked by member (propagate.assign_members); sigma, seed: the factors of propagate.sample_dispersion(B, S, sigma,
    seed) -- none at all with sigma == 0 and replicas == 1; steps: as flight_envelope (ONE chain run, 2 * steps RK4 steps per node
    interval); engine: an Engine of the same problem (one is created on device 0 otherwise).  The flown states stay on the device and
    only the peaks of the limited columns come back.
    -> the record of availability_from_peaks(peaks, members, limits, E), and "steps": 2 * steps, "status": 0 or GEL_NONFINITE (of
       the flight), "members" [B], "peaks": {column: {"min", "argmin", "max", "argmax" [B]}}, "dispersion": [B, S, 4] | None"""
    import torch
    from .propagate import assign_members, sample_dispersion
    if engine is None:
        S = pdict["num_sections"]
        ps = pdict["ps_params"]
        engine = Engine(con_dynamics.problem_arrays(pdict, unitdict), D=[ps.D(i) for i in range(S)],
                        tau=[ps.tau(i) for i in range(S)])
    steps, replicas = int(steps), int(replicas)
    if steps < 1 or replicas < 1:
        raise ValueError("steps and replicas: at least 1")
    if not limits:
        raise ValueError("limits: at least one limited column")
    names, _ids = engine._output_columns(list(limits))
    x = pack_x(xdict_or_x) if isinstance(xdict_or_x, dict) else np.asarray(xdict_or_x, dtype=np.float64)
    if x.size != engine.nvars:
        raise ValueError("wind_availability takes ONE decision vector [nvars = %d]" % engine.nvars)
    ens = engine.wind_ensemble(wind_tables)
    try:
        E = ens.E
        B, M, S, nc = E * replicas, engine.M, engine.S, len(names)
        members = assign_members(B, E, order="blocked")
        ens.assign(members)
        disp = None if (replicas == 1 and np.all(np.asarray(sigma) == 0)) else sample_dispersion(B, S, sigma, seed)
        d_disp = torch.from_numpy(disp).cuda() if disp is not None else None
        dptr = d_disp.data_ptr() if d_disp is not None else 0
        d_x = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(x.reshape(1, -1), (B, engine.nvars)))).cuda()
        d_y = torch.empty((B, 11 * M), dtype=torch.float64, device="cuda")
        d_peaks = torch.empty((B, nc, 4), dtype=torch.float64, device="cuda")
        plan = engine.propagation_plan(steps=2 * steps, restart="chain")
        try:
            plan.apply_device(B, d_x.data_ptr(), d_y.data_ptr(), 0, dptr, ensemble=ens)
            d_x[:, :11 * M] = d_y          # x_flown; the null stream orders itself against the engine's blocking stream
            lc = pdict["LaunchCondition"]
            engine.output_table_batch_device(B, d_x.data_ptr(), lc["lat"], lc["lon"], d_dispersion=dptr, columns=names,
                                             d_peaks=d_peaks.data_ptr(), ensemble=ens)
            status = engine.sync()
        finally:
            plan.close()
    finally:
        ens.close()
    pk = d_peaks.cpu().numpy()
    peaks = {}
    for k, name in enumerate(names):
        q = {f: pk[:, k, j].copy() for j, f in enumerate(engine.PEAK_FIELDS)}
        for f in ("argmin", "argmax"):
            q[f] = q[f].astype(np.int64)
        peaks[name] = q
    out = availability_from_peaks(peaks, members, limits, E)
    out.update({"steps": 2 * steps, "status": int(status), "members": members, "peaks": peaks, "dispersion": disp})
    return out


def linear_covariance(J, sigma):
    """J diag(sigma^2) J^T: the covariance of outputs whose Jacobian with respect to independent inputs of standard deviations sigma
    is J -- the linear-covariance counterpart of flight_covariance, fed by propagate.flight_jacobian where that one needs a dispersed
    batch.  J [..., R, P], sigma [P] (or one number) -> [..., R, R], symmetric bit for bit.  Host numpy."""
    J = np.asarray(J, dtype=np.float64)
    if J.ndim < 2:
        raise ValueError("J: [..., R, P]")
    sg = np.asarray(sigma, dtype=np.float64)
    if sg.shape not in ((), (J.shape[-1],)) or not np.all(sg >= 0):
        raise ValueError("sigma: one non-negative number, or one per column of J (%d)" % J.shape[-1])
    A = J * sg                      # (J sigma)(J sigma)^T: every entry and its mirror are the same sum of the same products
    C = np.einsum("...ip,...jp->...ij", A, A)
    lo = np.tril(np.ones(C.shape[-2:], dtype=bool))
    return np.where(lo, C, np.swapaxes(C, -1, -2))


def wind_linear_prediction(gwind, base_table, tables):
    """The first-order change of every functional under other wind tables, without flying them:
    sum over rows and components of gwind * (W_e - W_0).  gwind [..., Kg, 2]: propagate.flight_gradient(wind=True)["gwind"] (or
    PropagationPlan.adjoint(want_wind=True)'s GW) taken under base_table; base_table [Kw, 3] (altitude, north, east), Kw <= Kg;
    tables [E, Kw, 3] (one table: [Kw, 3]).  Every table must have the base's altitudes, bit for bit: the gradient holds the
    altitudes fixed, and another grid is another map (ValueError).  -> [E, ...]: the leading axes of gwind behind the table's.
    Host numpy."""
    g = np.asarray(gwind, dtype=np.float64)
    base = np.asarray(base_table, dtype=np.float64)
    T = np.asarray(tables, dtype=np.float64)
    if base.ndim != 2 or base.shape[1] != 3:
        raise ValueError("base_table: [Kw, 3]")
    if T.ndim == 2:
        T = T[None]
    if T.ndim != 3 or T.shape[1:] != base.shape:
        raise ValueError("tables: [E, Kw, 3] with the base's Kw = %d rows" % base.shape[0])
    Kw = base.shape[0]
    if g.ndim < 2 or g.shape[-1] != 2 or g.shape[-2] < Kw:
        raise ValueError("gwind: [..., Kg, 2] with Kg >= the base's %d rows" % Kw)
    if not np.array_equal(T[:, :, 0], np.broadcast_to(base[:, 0], T.shape[:2])):
        raise ValueError("tables: a member's altitudes differ from the base table's (the gradient holds the altitudes fixed)")
    dW = T[:, :, 1:] - base[None, :, 1:]                      # [E, Kw, 2]
    return np.einsum("...kc,ekc->e...", g[..., :Kw, :], dW)

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


def flight_envelope(xdict_or_X, pdict, unitdict, dispersion=None, steps=4, columns=None, engine=None):
    """xdict_or_X: a solution xdict or packed vectors [B, nvars] / [nvars]; dispersion: None or [B, S, 4]
    (propagate.sample_dispersion); steps: as propagate.fly; ONE chain run with 2 * steps RK4 steps per node interval, the run fly's y and err
    come from; columns: None (all of Engine.OUTPUT_COLUMNS) or a list of names; engine: an Engine of the same problem (one is
    created on device 0 otherwise).
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
        Y, err, status = plan.apply(X, dispersion=dispersion)
    finally:
        plan.close()
    x_flown = X.copy()
    x_flown[:, :11 * engine.M] = Y
    lc = pdict["LaunchCondition"]
    T = engine.output_table_batch(x_flown, lc["lat"], lc["lon"], dispersion=dispersion, columns=columns, table=False)
    out = {"steps": 2 * steps, "status": int(status), "columns": T["columns"], "envelope": T["envelope"], "peaks": T["peaks"],
           "terminal_miss": err[:, -1], "x_flown": x_flown}
    if engine._nlin + engine._nfn:
        con, _jfn, rc = engine.rows_eval(x_flown, want_jac=False)
        out["rows"] = con
        out["status"] = max(out["status"], int(rc))
    return out


def flight_quantiles(xdict_or_X, pdict, unitdict, probs, dispersion=None, steps=4, columns=None, engine=None):
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
        plan.apply_device(B, d_x.data_ptr(), d_y.data_ptr(), d_err.data_ptr(), dptr)
        d_x[:, :11 * M] = d_y          # x_flown; the null stream orders itself against the engine's blocking stream
        lc = pdict["LaunchCondition"]
        engine.output_table_batch_device(B, d_x.data_ptr(), lc["lat"], lc["lon"], d_dispersion=dptr, columns=columns,
                                         d_out=d_table.data_ptr(), d_peaks=d_peaks.data_ptr())
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


def flight_covariance(xdict_or_X, pdict, unitdict, dispersion, steps=4, columns=None, engine=None):
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
        plan.apply_device(B, d_x.data_ptr(), d_y.data_ptr(), d_err.data_ptr(), d_disp.data_ptr())
        d_x[:, :11 * M] = d_y          # x_flown; the null stream orders itself against the engine's blocking stream
        lc = pdict["LaunchCondition"]
        engine.output_table_batch_device(B, d_x.data_ptr(), lc["lat"], lc["lon"], d_dispersion=d_disp.data_ptr(), columns=columns,
                                         d_out=d_table.data_ptr(), d_peaks=d_peaks.data_ptr())
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

"""The Monte-Carlo look at a solution: fly a dispersed batch and read its post-processing table as an envelope.

propagate.fly integrates every decision vector from lift-off to the last node under per-vector dispersions of thrust, mass flow,
reference area and wind.  flight_envelope() takes the flown states and asks the batched output table (Engine.output_table_batch,
include/gelato_amd.h gel_output_table_batch) for what a launch-vehicle user wants of such a batch: per node the
spread of max-Q, q-alpha, Mach, altitude, the impact point and the orbit over the flights, and the peak of every flight -- formed
with the SAME factors the flight was flown with (the dispersed wind is the wind of the dynamic pressure).  flight_quantiles() reads
the same batch by exact percentiles over the flights (Engine.batch_quantiles_device, gel_batch_quantiles), with the
table kept on the device.
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

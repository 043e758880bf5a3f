"""The Monte-Carlo look at a solution: fly a dispersed batch and read its post-processing table as an envelope.

propagate.fly integrates every decision vector from lift-off to the last node under per-vector dispersions of thrust, mass flow,
reference area and wind.  flight_envelope() takes the flown states and asks the batched output table (Engine.output_table_batch,
include/gelato_amd.h gel_output_table_batch) for what a launch-vehicle user wants of such a batch: per node the
spread of max-Q, q-alpha, Mach, altitude, the impact point and the orbit over the flights, and the peak of every flight -- formed
with the SAME factors the flight was flown with (the dispersed wind is the wind of the dynamic pressure).
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

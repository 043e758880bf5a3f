"""The shooting check: an explicit integration of every section, independent of the collocation matrices.

The collocation error estimate (mesh_error.py) judges the collocation polynomial with the collocation method's own matrices.
The shooting check takes the controls the optimiser found, integrates the equations of motion with classical RK4 from each
section's first state (include/gelato_amd.h gel_propagate) and compares the trajectory with the collocated
states at the nodes.  It exposes a control polynomial that oscillates between its nodes, which the node values hide.  The
integration runs on the device (Engine.propagation_plan); this module turns it into one record per section.
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

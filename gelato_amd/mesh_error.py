"""Collocation error estimate per section, and the node counts it suggests.

Once the optimiser stops, the defect at the collocation points is zero by construction and says nothing about the trajectory
between the nodes.  The LGR estimate (Garg et al. 2009; Patterson, Hager & Rao's ph method, as in GPOPS-II) interpolates the
solution onto the LGR grid of one node more, integrates the dynamics there with that grid's Radau integration matrix and takes
the relative mismatch (include/gelato_amd.h gel_mesh_error).  The estimate runs on the device (Engine.mesh_error);
this module turns it into one record per section of the events CSV.
"""
import math

import numpy as np

from . import con_dynamics
from .engine import Engine, pack_x

GROUPS = ("mass", "position", "velocity", "quaternion")


def collocation_error(xdict, pdict, unitdict, engine=None):
    """One record per section of a solution xdict: {"name": the section's event name, "num_nodes", "mass", "position",
    "velocity", "quaternion": the group errors (max over the test points and the group's components of
    |X^ - X~| / (1 + max |X~|)), "max": the largest of the four}.  engine: an Engine of the same problem (one is created
    on device 0 otherwise).  Raises if an error is NaN / Inf."""
    S = pdict["num_sections"]
    if engine is None:
        ps = pdict["ps_params"]
        engine = Engine(con_dynamics.problem_arrays(pdict, unitdict), D=[ps.D(i) for i in range(S)],
                        tau=[ps.tau(i) for i in range(S)])
    err, _diff, rc = engine.mesh_error(pack_x(xdict))
    if rc != 0:
        raise FloatingPointError("collocation error estimate: non-finite output (status %d)" % rc)
    report = []
    for i in range(S):
        rec = {"name": pdict["params"][i]["name"], "num_nodes": int(engine.num_nodes[i])}
        for g, k in enumerate(GROUPS):
            rec[k] = float(err[0, i, g])
        rec["max"] = max(rec[k] for k in GROUPS)
        report.append(rec)
    return report


def suggest_num_nodes(report, tol, n_max):
    """The ph method's p-rule on a collocation_error report.  A section with n nodes and error e_max = rec["max"] keeps n when
    e_max <= tol; otherwise it gets

        n' = min(n_max, n + max(1, ceil(log(e_max / tol) / log(n))))

    (the estimate falls like n^-p for a smooth solution: log_n(e_max / tol) more nodes reach tol).  A section whose n' hits
    n_max is marked "capped": GELATO cannot split a section without a new event, so more accuracy there needs another event.
    Returns one record per section: {"name", "num_nodes", "max", "suggested", "action": "kept" | "raised" | "capped"}."""
    out = []
    for rec in report:
        n, e = int(rec["num_nodes"]), float(rec["max"])
        if not math.isfinite(e):
            raise FloatingPointError("section %r: non-finite error estimate" % (rec.get("name"),))
        if e <= tol:
            new, action = n, "kept"
        else:
            p = max(1, int(math.ceil(math.log(e / tol) / math.log(n))))
            new = n + p
            action = "raised"
            if new > n_max:
                new, action = max(n, n_max), "capped"
        out.append({"name": rec.get("name"), "num_nodes": n, "max": e, "suggested": new, "action": action})
    return out


def report_array(report):
    """the four group errors of a report as an [S, 4] array (GROUPS order)"""
    return np.array([[rec[k] for k in GROUPS] for rec in report])

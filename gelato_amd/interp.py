"""Spectral interpolation of a solution: dense output, and transfer to a mesh of other node counts.

Per section the collocation solution is a polynomial (degree n in the states on [-1, tau], degree n - 1 in the controls on tau).
The engine evaluates it at any points inside the sections (include/gelato_amd.h gel_interp_*); this module is
the xdict / pdict face of it: ``sample`` gives SI arrays of one solution on a grid of the caller's choice, ``refine`` carries a
solution to the node counts that ``mesh_error.suggest_num_nodes`` proposes and returns the pdict of the refined problem, ready
for the next solve.  Host-only handles are enough for both (one solution; batches go through Engine.interp_plan /
Engine.transfer_plan on a device).
"""
import numpy as np

from . import con_dynamics
from .SectionParameters import PSparams
from .engine import Engine, pack_x


def _host_engine(pdict, unitdict):
    ps = pdict["ps_params"]
    S = pdict["num_sections"]
    return Engine(con_dynamics.problem_arrays(pdict, unitdict), D=[ps.D(i) for i in range(S)], tau=[ps.tau(i) for i in range(S)],
                  device=-1)


def sample(xdict, pdict, unitdict, points=None, per_section=None, engine=None):
    """One solution xdict on a grid inside its sections, in SI units: {"t" [s], "mass", "position" [npts, 3], "velocity"
    [npts, 3], "quaternion" [npts, 4], "u" [npts, 2], "section" [npts] (index of the section of every row)}, rows in section order.
    points: a list of S arrays of points in [-1, 1] (-1 / +1 = the section's knots); or per_section = k: k uniform points in
    each section, end points included.  A control sampled below the section's first collocation node is the control polynomial
    extrapolated.  engine: an Engine of the same problem (a host-only one is created otherwise)."""
    S = pdict["num_sections"]
    if (points is None) == (per_section is None):
        raise ValueError("give either points or per_section")
    if points is None:
        if int(per_section) < 2:
            raise ValueError("per_section: at least the two end points")
        points = [np.linspace(-1.0, 1.0, int(per_section))] * S
    own = engine is None
    if own:
        engine = _host_engine(pdict, unitdict)
    plan = engine.interp_plan(points)
    try:
        out, rc = plan.apply_host(pack_x(xdict))
    finally:
        plan.close()
        if own:
            engine.close()
    if rc != 0:
        raise FloatingPointError("interpolation: non-finite output (status %d)" % rc)
    tab = out[0]
    return {"t": tab[:, 0] * unitdict["t"], "mass": tab[:, 1] * unitdict["mass"], "position": tab[:, 2:5] * unitdict["position"],
            "velocity": tab[:, 5:8] * unitdict["velocity"], "quaternion": tab[:, 8:12].copy(), "u": tab[:, 12:14] * unitdict["u"],
            "section": np.repeat(np.arange(S), [np.asarray(p).size for p in points])}


def refine(xdict, pdict, unitdict, num_nodes, unit_quat=False):
    """Carry a solution to a mesh of other node counts -> (xdict_new, pdict_new).  num_nodes: one count per section, or the
    records of mesh_error.suggest_num_nodes (their "suggested").  Every section's polynomial is evaluated at the new mesh's
    nodes; nodes the two meshes share (each section's first and last state node, always) keep their bits, and so does t.
    pdict_new is a shallow copy of pdict with a new PSparams, N and M, and without the constraint mirrors' device cache; neither
    pdict nor xdict is modified.  unit_quat: renormalise the interpolated quaternions (rows that are not copies)."""
    S = pdict["num_sections"]
    nn = [int(r["suggested"]) if isinstance(r, dict) else int(r) for r in num_nodes]
    if len(nn) != S:
        raise ValueError("num_nodes: one count per section (%d)" % S)
    pnew = {k: v for k, v in pdict.items() if k != con_dynamics._KEY}
    pnew["ps_params"] = PSparams(nn)
    pnew["N"] = sum(nn)
    pnew["M"] = pnew["N"] + S
    src, dst = _host_engine(pdict, unitdict), _host_engine(pnew, unitdict)
    plan = src.transfer_plan(dst, unit_quat=unit_quat)
    try:
        out, rc = plan.apply_host(pack_x(xdict))
        xnew = {k: np.array(v) for k, v in dst.split_x(out[0]).items()}
    finally:
        plan.close()
        src.close()
        dst.close()
    if rc != 0:
        raise FloatingPointError("mesh transfer: non-finite output (status %d)" % rc)
    return xnew, pnew

"""Engine: Python handle on a device-resident LGR defect/Jacobian problem.

Thin wrapper over the C-ABI (include/gelato_amd.h).  Holds no numerics of its own.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import GelCallbackIO, GelDims, GelLinearRow, GelNodefnRow, GelProblemDesc, check, lib

GROUPS = ["mass", "pos", "vel", "quat"]
# funcs / funcsSens keys of the reference callbacks (Trajectory_Optimization.py:199-210,250-261)
CON_NAMES = {"mass": "eqcon_dyn_mass", "pos": "eqcon_dyn_pos", "vel": "eqcon_dyn_vel", "quat": "eqcon_dyn_quat"}
# Jacobian blocks in C-ABI order: (group, var); var order per group = the reference's dict order
BLOCKS = [("mass", "mass"), ("mass", "t"),
          ("pos", "position"), ("pos", "velocity"), ("pos", "t"),
          ("vel", "mass"), ("vel", "position"), ("vel", "velocity"), ("vel", "quaternion"), ("vel", "t"),
          ("quat", "quaternion"), ("quat", "u"), ("quat", "t")]
XKEYS = ["mass", "position", "velocity", "quaternion", "u", "t"]

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_lp = C.POINTER(C.c_int64)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _d(a):
    return a.ctypes.data_as(_dp)


def pack_x(xdict, out=None):
    """xdict (reference layout, Trajectory_Optimization.py:318-352) -> packed decision vector (into `out` if given)."""
    return np.concatenate([np.asarray(xdict[k], dtype=np.float64).ravel() for k in XKEYS], out=out)


class _Handle:
    """The one owner of a C problem handle: close() destroys it (once), and so does the collector when the last holder goes --
    the Engine, or a pinned view of the handle's memory that outlives it.  It refers to nothing else, so reference counting
    frees it."""

    def __init__(self, ptr):
        self.ptr = ptr

    def close(self):
        if self.ptr:
            ptr, self.ptr = self.ptr, None
            lib().gel_problem_destroy(ptr)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _PinnedView(np.ndarray):
    """numpy view of the handle's pinned host memory that keeps the handle alive (attribute _owner on the base view)"""


class InterpPlan:
    """An interpolation plan of one engine (include/gelato_amd.h gel_interp_*): the matrices that evaluate every
    section's polynomial at the plan's points -- a table of points (Engine.interp_plan) or another engine's mesh
    (Engine.transfer_plan).  It holds the engine's handle owner, so the handle outlives it; close() destroys the plan."""

    INFO = ("S", "mode", "state_rows", "out_doubles", "src_nvars", "vb")

    def __init__(self, owner, ptr, src_nodes, P, Pu):
        self._owner = owner       # the source engine's _Handle: not destroyed while a plan refers to it
        self._p = ptr
        self._n = [int(v) for v in src_nodes]
        self._P, self._Pu = [int(v) for v in P], [int(v) for v in Pu]
        i = self.info()
        self.S, self.mode, self.nvars, self.out_doubles = i["S"], i["mode"], i["src_nvars"], i["out_doubles"]
        self.out_shape = (i["state_rows"], 14) if self.mode == 0 else (self.out_doubles,)

    def close(self):
        if self._p:
            ptr, self._p = self._p, None
            if self._owner.ptr:     # (a handle closed first has taken the device down with it: the plan's host memory leaks)
                lib().gel_interp_plan_destroy(ptr)
        self._owner = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        """{"S", "mode" (0 table, 1 transfer), "state_rows", "out_doubles" per vector, "src_nvars", "vb": vectors per workgroup a
        launch will use NOW (GEL_INTERP_VB is read per call)}"""
        info = (C.c_int64 * 6)()
        check(lib().gel_interp_plan_info(self._p, info))
        return dict(zip(self.INFO, (int(v) for v in info)))

    def matrices(self, phase):
        """{"Wx" [P, n+1], "Wu" [Pu, n], "copy_x" [P], "copy_u" [Pu]} of one phase"""
        n, P, Pu = self._n[phase], self._P[phase], self._Pu[phase]
        out = {"Wx": np.zeros((P, n + 1)), "Wu": np.zeros((Pu, n)), "copy_x": np.zeros(P, dtype=np.int32),
               "copy_u": np.zeros(Pu, dtype=np.int32)}
        check(lib().gel_interp_matrices(self._p, int(phase), _d(out["Wx"]), _d(out["Wu"]), out["copy_x"].ctypes.data_as(_ip),
                                        out["copy_u"].ctypes.data_as(_ip)))
        return out

    def _apply(self, fn, X):
        if not (self._p and self._owner.ptr):
            raise _lib.GelatoAmdError("interpolation plan: closed, or its engine was closed first")
        X = _f64(X).reshape(-1, self.nvars)
        B = X.shape[0]
        out = np.empty((B,) + self.out_shape)
        rc = check(fn(self._p, B, _d(X), _d(out)))
        return out, rc

    def apply(self, X):
        """X [B, nvars] (or [nvars]) -> (out [B, npts, 14] (table) or [B, dst nvars] (transfer), status): one device launch"""
        return self._apply(lib().gel_interp, X)

    def apply_host(self, X):
        """the same in plain C++ on the host (works on host-only handles), the same bits -> (out, status)"""
        return self._apply(lib().gel_interp_host, X)

    def apply_resident(self, B, d_x, d_out):
        """device buffers, asynchronous on the source engine's own stream; status through Engine.sync()"""
        if not (self._p and self._owner.ptr):
            raise _lib.GelatoAmdError("interpolation plan: closed, or its engine was closed first")
        check(lib().gel_interp_resident(self._p, int(B), d_x, d_out))


class PropagationPlan:
    """An RK4 propagation plan of one engine (include/gelato_amd.h gel_prop_*): per section the stage points and
    the matrix that samples the control polynomial there.  apply() integrates the equations of motion explicitly through every
    section -- the shooting check.  It holds the engine's handle owner, so the handle outlives it; close() destroys the plan."""

    INFO = ("S", "flags", "stage_points", "lane_steps", "workspace_bytes_per_vector", "slab")

    def __init__(self, owner, ptr, nodes, steps, dims):
        self._owner = owner       # the engine's _Handle: not destroyed while a plan refers to it
        self._p = ptr
        self._n = [int(v) for v in nodes]
        self.steps = [int(v) for v in steps]
        self.S, self.M, self.nvars = dims

    def close(self):
        if self._p:
            ptr, self._p = self._p, None
            if self._owner.ptr:     # (a handle closed first has taken the device down with it: the plan's host memory leaks)
                lib().gel_prop_plan_destroy(ptr)
        self._owner = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _live(self):
        if not (self._p and self._owner.ptr):
            raise _lib.GelatoAmdError("propagation plan: closed, or its engine was closed first")

    def info(self):
        """{"S", "flags", "stage_points" in total, "lane_steps": RK4 steps of the longest lane, "workspace_bytes_per_vector",
        "slab": vectors per slab a call will use NOW (GEL_PROP_SLAB is read per call)}"""
        self._live()
        info = (C.c_int64 * 6)()
        check(lib().gel_prop_plan_info(self._p, info))
        return dict(zip(self.INFO, (int(v) for v in info)))

    def matrices(self, phase):
        """{"pts" [Pp], "Wu" [Pp, n], "copy_u" [Pp]} of one phase, Pp = 2 steps n + 1 (works on host-only handles)"""
        self._live()
        n = self._n[phase]
        Pp = 2 * self.steps[phase] * n + 1
        out = {"pts": np.zeros(Pp), "Wu": np.zeros((Pp, n)), "copy_u": np.zeros(Pp, dtype=np.int32)}
        check(lib().gel_prop_matrices(self._p, int(phase), _d(out["pts"]), _d(out["Wu"]), out["copy_u"].ctypes.data_as(_ip)))
        return out

    def apply(self, X, want_err=True, dispersion=None, ensemble=None):
        """X [B, nvars] (or [nvars]) -> (Y [B, 11 M]: the propagated state at every state node, laid out like the state part of
        x; err [B, S, 4] (mass, position, velocity, quaternion) | None; status).  dispersion: None, or float64 [B, S, 4] ([S, 4]
        for one vector): per vector and phase the factors of thrust, mass flow, reference area and wind (gel_propagate_dispersed).
        ensemble: None, or a WindEnsemble of this engine assigned B vectors: every vector flies under the wind table its entry
        selects (gel_propagate_ensemble)"""
        self._live()
        X = _f64(X).reshape(-1, self.nvars)
        B = X.shape[0]
        ens = _ensemble_ptr(ensemble, self._owner)
        disp = None
        if dispersion is not None:
            disp = np.asarray(dispersion)
            if disp.dtype != np.float64:
                raise TypeError("dispersion: float64")
            if disp.shape == (self.S, _lib.GEL_PROP_NDISP) and B == 1:
                disp = disp[None]
            if disp.shape != (B, self.S, _lib.GEL_PROP_NDISP):
                raise ValueError("dispersion: [B, S, %d] = %s, not %s" % (_lib.GEL_PROP_NDISP, (B, self.S, _lib.GEL_PROP_NDISP), disp.shape))
            disp = np.ascontiguousarray(disp)
        Y = np.empty((B, 11 * self.M))
        err = np.empty((B, self.S, 4)) if want_err else None
        rc = check(lib().gel_propagate_ensemble(self._p, B, _d(X), _d(disp) if disp is not None else None, ens, _d(Y),
                                                _d(err) if want_err else None))
        return Y, err, rc

    def apply_device(self, B, d_x, d_y, d_err=0, d_dispersion=0, ensemble=None):
        """device buffers: d_y [B][11 M], d_err [B][S][4] or 0, d_dispersion [B][S][4] or 0; ensemble: None or a WindEnsemble of
        this engine assigned B vectors; asynchronous on the engine's own stream; status through Engine.sync()"""
        self._live()
        check(lib().gel_propagate_ensemble_device(self._p, int(B), d_x, d_dispersion or None, _ensemble_ptr(ensemble, self._owner), d_y,
                                                  d_err or None))


    def _seed(self, a, name, B, P, shared, tail):
        """a seed array as the library takes it: [P, *tail] when shared, else [B, P, *tail]; None stays None"""
        if a is None:
            return None
        a = np.asarray(a)
        if a.dtype != np.float64:
            raise TypeError("%s: float64" % name)
        want = ((P,) if shared else (B, P)) + tail
        if a.shape != want:
            raise ValueError("%s: %s, not %s" % (name, want, a.shape))
        return np.ascontiguousarray(a)

    def wind_rows(self, ensemble=None):
        """Kg: the rows of a wind seed / of GW (gel_prop_wind_rows): the handle's Kw, under an ensemble the larger
        of that and the ensemble's (works on host-only handles)"""
        self._live()
        kg = C.c_int32(0)
        check(lib().gel_prop_wind_rows(self._p, _ensemble_ptr(ensemble, self._owner), C.byref(kg)))
        return int(kg.value)

    def tangent(self, X, dX=None, dispersion=None, ddispersion=None, shared=False, ensemble=None, dwind=None):
        """The flight of apply() and its exact derivative along seed directions (gel_propagate_tangent).
        X [B, nvars] (or [nvars]); dX: None, or the directions in x, [B, P, nvars] ([P, nvars] with shared=True: one set for every
        vector); dispersion: None or [B, S, 4]; ddispersion: None, or the directions in the factors, [B, P, S, 4] ([P, S, 4] shared).
        At least one of dX / ddispersion / dwind.  ensemble: None, or a WindEnsemble of this engine assigned B vectors: every vector's
        flight AND derivative under the wind table its entry selects (gel_propagate_tangent_ensemble).
        dwind: None, or the directions in the VALUES of the wind table the flight reads, [B, P, Kg, 2] ([P, Kg, 2] shared), north and
        east per row, Kg = wind_rows(ensemble) (gel_propagate_tangent_wind); None is the call without it.
        -> (Y [B, 11 M]: apply()'s Y bit for bit, dY [B, P, 11 M], status)"""
        self._live()
        X = _f64(X).reshape(-1, self.nvars)
        B = X.shape[0]
        ens = _ensemble_ptr(ensemble, self._owner)
        if dX is None and ddispersion is None and dwind is None:
            raise ValueError("tangent: at least one of dX, ddispersion and dwind")
        shared = bool(shared)
        lead = np.asarray(dX if dX is not None else ddispersion if ddispersion is not None else dwind)
        if lead.ndim < (2 if shared else 3):
            raise ValueError("tangent: seeds are [P, ...] with shared=True, else [B, P, ...]")
        P = int(lead.shape[0] if shared else lead.shape[1])
        if P < 1:
            raise ValueError("tangent: at least one direction")
        nd = _lib.GEL_PROP_NDISP
        dx = self._seed(dX, "dX", B, P, shared, (self.nvars,))
        dd = self._seed(ddispersion, "ddispersion", B, P, shared, (self.S, nd))
        disp = None
        if dispersion is not None:
            disp = np.asarray(dispersion)
            if disp.dtype != np.float64:
                raise TypeError("dispersion: float64")
            if disp.shape == (self.S, nd) and B == 1:
                disp = disp[None]
            if disp.shape != (B, self.S, nd):
                raise ValueError("dispersion: [B, S, %d] = %s, not %s" % (nd, (B, self.S, nd), disp.shape))
            disp = np.ascontiguousarray(disp)
        Y = np.empty((B, 11 * self.M))
        dY = np.empty((B, P, 11 * self.M))
        opt = lambda a: _d(a) if a is not None else None   # noqa: E731
        if dwind is None:
            rc = check(lib().gel_propagate_tangent_ensemble(self._p, B, P, int(shared), _d(X), opt(disp), opt(dx), opt(dd), ens, _d(Y), _d(dY)))
            return Y, dY, rc
        dw = self._seed(dwind, "dwind", B, P, shared, (self.wind_rows(ensemble), 2))
        rc = check(lib().gel_propagate_tangent_wind(self._p, B, P, int(shared), _d(X), opt(disp), opt(dx), opt(dd), _d(dw), ens, _d(Y), _d(dY)))
        return Y, dY, rc

    def tangent_device(self, B, P, d_x, d_y, d_dy, d_dx=0, d_dispersion=0, d_ddispersion=0, shared=False, ensemble=None, d_dwind=0):
        """device buffers: d_y [B][11 M], d_dy [B][P][11 M], d_dx / d_ddispersion / d_dwind as tangent() lays them out or 0 (not
        all), d_dispersion [B][S][4] or 0; ensemble: None or a WindEnsemble of this engine assigned B vectors; asynchronous on the
        engine's own stream; status through Engine.sync()"""
        self._live()
        if d_dwind:
            check(lib().gel_propagate_tangent_wind_device(self._p, int(B), int(P), int(bool(shared)), d_x, d_dispersion or None,
                                                          d_dx or None, d_ddispersion or None, d_dwind,
                                                          _ensemble_ptr(ensemble, self._owner), d_y, d_dy))
            return
        check(lib().gel_propagate_tangent_ensemble_device(self._p, int(B), int(P), int(bool(shared)), d_x, d_dispersion or None,
                                                          d_dx or None, d_ddispersion or None, _ensemble_ptr(ensemble, self._owner),
                                                          d_y, d_dy))

    def tangent_info(self, B, P, shared=False):
        """{"sample_set_bytes", "lanes_per_slab", "slabs"} of a tangent call NOW (works on host-only handles)"""
        self._live()
        info = (C.c_int64 * 3)()
        check(lib().gel_prop_tangent_info(self._p, int(B), int(P), int(bool(shared)), info))
        return dict(zip(("sample_set_bytes", "lanes_per_slab", "slabs"), (int(v) for v in info)))

    def adjoint(self, X, Lam, dispersion=None, shared=False, ensemble=None, want_wind=False):
        """The flight of apply() and the gradients of Q functionals of it in one backward pass (gel_propagate_adjoint):
        the transpose of the linear map tangent() applies.  X [B, nvars] (or [nvars]); Lam: the functionals as weights on Y,
        [B, Q, 11 M] ([Q, 11 M] with shared=True: one set for every vector); dispersion: None or [B, S, 4].  Chain and section plans.
        ensemble: None, or a WindEnsemble of this engine assigned B vectors: every vector's flight AND gradients under the wind
        table its entry selects (gel_propagate_adjoint_ensemble).
        want_wind: also the gradients with respect to the VALUES of the wind table every flight reads (gel_propagate_adjoint_wind;
        DESIGN.md 3.23), GW [B, Q, Kg, 2], Kg = wind_rows(ensemble): rows at or beyond a vector's own table, and rows no stage of its
        flight touched, are +0.0.
        -> (Y [B, 11 M]: apply()'s Y bit for bit, GX [B, Q, nvars], GD [B, Q, S, 4], status), with want_wind
        (Y, GX, GD, status, GW)"""
        self._live()
        X = _f64(X).reshape(-1, self.nvars)
        B = X.shape[0]
        ens = _ensemble_ptr(ensemble, self._owner)
        shared = bool(shared)
        lam = np.asarray(Lam)
        if lam.dtype != np.float64:
            raise TypeError("Lam: float64")
        if lam.ndim != (2 if shared else 3):
            raise ValueError("adjoint: Lam is [Q, 11 M] with shared=True, else [B, Q, 11 M]")
        Q = int(lam.shape[0] if shared else lam.shape[1])
        if Q < 1:
            raise ValueError("adjoint: at least one functional")
        lam = self._seed(lam, "Lam", B, Q, shared, (11 * self.M,))
        nd = _lib.GEL_PROP_NDISP
        disp = None
        if dispersion is not None:
            disp = np.asarray(dispersion)
            if disp.dtype != np.float64:
                raise TypeError("dispersion: float64")
            if disp.shape == (self.S, nd) and B == 1:
                disp = disp[None]
            if disp.shape != (B, self.S, nd):
                raise ValueError("dispersion: [B, S, %d] = %s, not %s" % (nd, (B, self.S, nd), disp.shape))
            disp = np.ascontiguousarray(disp)
        Y = np.empty((B, 11 * self.M))
        GX = np.empty((B, Q, self.nvars))
        GD = np.empty((B, Q, self.S, nd))
        if want_wind:
            GW = np.empty((B, Q, self.wind_rows(ensemble), 2))
            rc = check(lib().gel_propagate_adjoint_wind(self._p, B, Q, int(shared), _d(X), _d(disp) if disp is not None else None, _d(lam),
                                                        ens, _d(Y), _d(GX), _d(GD), _d(GW)))
            return Y, GX, GD, rc, GW
        rc = check(lib().gel_propagate_adjoint_ensemble(self._p, B, Q, int(shared), _d(X), _d(disp) if disp is not None else None, _d(lam),
                                                        ens, _d(Y), _d(GX), _d(GD)))
        return Y, GX, GD, rc

    def adjoint_device(self, B, Q, d_x, d_lam, d_y, d_gx, d_gdisp=0, d_dispersion=0, shared=False, ensemble=None, d_gwind=0):
        """device buffers: d_lam as adjoint() lays Lam out, d_y [B][11 M], d_gx [B][Q][nvars], d_gdisp [B][Q][S][4] or 0,
        d_gwind [B][Q][Kg][2] or 0, d_dispersion [B][S][4] or 0; ensemble: None or a WindEnsemble of this engine assigned B vectors;
        asynchronous on the engine's own stream; status through Engine.sync()"""
        self._live()
        if d_gwind:
            check(lib().gel_propagate_adjoint_wind_device(self._p, int(B), int(Q), int(bool(shared)), d_x, d_dispersion or None,
                                                          d_lam or None, _ensemble_ptr(ensemble, self._owner), d_y, d_gx, d_gdisp or None,
                                                          d_gwind))
            return
        check(lib().gel_propagate_adjoint_ensemble_device(self._p, int(B), int(Q), int(bool(shared)), d_x, d_dispersion or None,
                                                          d_lam or None, _ensemble_ptr(ensemble, self._owner), d_y, d_gx, d_gdisp or None))

    def adjoint_info(self, B, Q, shared=False, want_wind=False, ensemble=None):
        """{"lane_bytes", "lanes_per_slab", "slabs"} of an adjoint call NOW (works on host-only handles); with want_wind those of a
        call that also returns GW (16 Kg bytes per lane more), and "wind_rows": Kg"""
        self._live()
        if want_wind:
            info = (C.c_int64 * 4)()
            check(lib().gel_prop_adjoint_wind_info(self._p, _ensemble_ptr(ensemble, self._owner), int(B), int(Q), int(bool(shared)), 1, info))
            return dict(zip(("lane_bytes", "lanes_per_slab", "slabs", "wind_rows"), (int(v) for v in info)))
        info = (C.c_int64 * 3)()
        check(lib().gel_prop_adjoint_info(self._p, int(B), int(Q), int(bool(shared)), info))
        return dict(zip(("lane_bytes", "lanes_per_slab", "slabs"), (int(v) for v in info)))


def _ensemble_ptr(ensemble, owner):
    """the raw pointer of a live WindEnsemble (None for None); an ensemble of another engine is refused here, by name"""
    if ensemble is None:
        return None
    if not isinstance(ensemble, WindEnsemble):
        raise TypeError("ensemble: a WindEnsemble (Engine.wind_ensemble) or None")
    ensemble._live()
    if ensemble._owner is not owner:
        raise ValueError("ensemble: created by another engine")
    return ensemble._p


class WindEnsemble:
    """A wind ensemble of one engine (include/gelato_amd.h gel_wind_ensemble_*): E member tables [Kw, 3] resident on
    the device and one assignment member [B] (-1: the engine's own table) that the flight and the table of a batch read alike.  It
    holds the engine's handle owner, so the handle outlives it; close() destroys the ensemble."""

    INFO = ("E", "Kw", "member_doubles", "device_bytes", "assigned")

    def __init__(self, owner, ptr, E, Kw):
        self._owner = owner
        self._p = ptr
        self.E, self.Kw = int(E), int(Kw)

    def close(self):
        if self._p:
            ptr, self._p = self._p, None
            if self._owner.ptr:     # (a handle closed first has taken the device down with it: the ensemble's host memory leaks)
                lib().gel_wind_ensemble_destroy(ptr)
        self._owner = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _live(self):
        if not (self._p and self._owner.ptr):
            raise _lib.GelatoAmdError("wind ensemble: closed, or its engine was closed first")

    def info(self):
        """{"E", "Kw", "member_doubles": 5 Kw - 2, "device_bytes", "assigned": vectors of the current assignment or -1}"""
        self._live()
        info = (C.c_int64 * 5)()
        check(lib().gel_wind_ensemble_info(self._p, info))
        return dict(zip(self.INFO, (int(v) for v in info)))

    def member(self, e):
        """member e as staged -> {"rows" [Kw, 3], "slopes" [Kw - 1, 2]} (works on host-only handles)"""
        self._live()
        st = np.empty(5 * self.Kw - 2)
        check(lib().gel_wind_ensemble_member(self._p, int(e), _d(st)))
        return {"rows": st[:3 * self.Kw].reshape(self.Kw, 3), "slopes": st[3 * self.Kw:].reshape(self.Kw - 1, 2)}

    def assign(self, members):
        """members: integers [B], each -1 (the engine's own wind table) or 0 .. E - 1; validated by the library"""
        self._live()
        m = np.asarray(members)
        if m.ndim != 1:
            raise ValueError("members: one entry per vector, [B]")
        if m.size and not np.issubdtype(m.dtype, np.integer):
            raise TypeError("members: integers")
        if m.size and (int(m.min()) < -1 or int(m.max()) >= self.E):
            raise ValueError("members: -1 or 0 .. %d, not %d .. %d" % (self.E - 1, int(m.min()), int(m.max())))
        m = np.ascontiguousarray(m, dtype=np.int32)
        check(lib().gel_wind_ensemble_assign(self._p, int(m.size), m.ctypes.data_as(_ip)))
        self.members = m.copy()   # the assignment in force (what flight_gradient(wind=True) names the altitudes by)
        return self


class Engine:
    """prob: dict with num_nodes, thrust, massflow, reference_area, nozzle_area, engine_on,
    attitude_hold, units (mass, position, velocity, u, t), dx, wind_table [K,3], ca_table [K,2];
    optional D / tau (lists per phase, e.g. pdict["ps_params"].D(i)); barC20 (0 -> C++ constant)."""

    def __init__(self, prob, D=None, tau=None, barC20=0.0, device=0, flags=0):
        L = lib()
        self._keep = []
        nn = np.ascontiguousarray(prob["num_nodes"], dtype=np.int32)
        S = len(nn)

        def darr(key):
            a = _f64(prob[key])
            assert a.size == S, key
            self._keep.append(a)
            return _d(a)

        def iarr(key):
            a = np.ascontiguousarray(prob[key], dtype=np.int32)
            assert a.size == S, key
            self._keep.append(a)
            return a.ctypes.data_as(_ip)

        wind, ca = _f64(prob["wind_table"]), _f64(prob["ca_table"])
        units = _f64(prob["units"])
        self.units = units.copy()   # (mass, position, velocity, u, t)
        self.wind_altitudes = wind.reshape(-1, 3)[:, 0].copy()   # of the handle's own wind table (flight_gradient(wind=True))
        self.prob = {k: np.array(prob[k]) for k in ("num_nodes", "thrust", "massflow", "reference_area", "nozzle_area",
                                                    "engine_on", "attitude_hold")}
        d = GelProblemDesc()
        d.num_sections = S
        d.num_nodes = nn.ctypes.data_as(_ip)
        d.thrust, d.massflow = darr("thrust"), darr("massflow")
        d.reference_area, d.nozzle_area = darr("reference_area"), darr("nozzle_area")
        d.engine_on, d.attitude_hold = iarr("engine_on"), iarr("attitude_hold")
        d.unit_mass, d.unit_position, d.unit_velocity, d.unit_u, d.unit_t = [float(u) for u in units]
        d.dx = float(prob["dx"])
        d.barC20 = float(barC20)
        d.wind_rows, d.wind_table = wind.shape[0], _d(wind)
        d.ca_rows, d.ca_table = ca.shape[0], _d(ca)
        if D is not None:
            Dall = _f64(np.concatenate([np.asarray(x, dtype=np.float64).ravel() for x in D]))
            tall = _f64(np.concatenate([np.asarray(x, dtype=np.float64).ravel() for x in tau]))
            d.D, d.tau = _d(Dall), _d(tall)
        else:
            d.D, d.tau = None, None
        d.device = device
        self.flags = int(flags)
        d.flags = int(flags)  # 0, or GEL_FLAG_DX_MFMA (1) / GEL_FLAG_DX_VALU (2) to force the D.X path, GEL_FLAG_NO_PACK (4), GEL_FLAG_FD_RECOMPUTE (8),
        # GEL_FLAG_EXACT_DEFECT_JAC (32, _lib): the defect groups' Jacobians exact to rounding instead of forward differences
        # GEL_FLAG_EXACT_AERO_JAC (64, _lib): the aero path constraints' gradients exact to rounding instead of forward differences
        # GEL_FLAG_EXACT_ROWS_JAC (128, _lib): the node-function rows' jfn exact to rounding instead of forward differences
        h = C.c_void_p()
        check(L.gel_problem_create(C.byref(d), C.byref(h)))
        self._owner = _Handle(h)
        self._h = h   # the raw pointer every call passes (self._owner holds the handle)
        dims = GelDims()
        check(L.gel_problem_dims(h, C.byref(dims)))
        self.S, self.N, self.M, self.nvars = dims.S, dims.N, dims.M, dims.num_vars
        self.num_nodes = nn.copy()
        self.nrows = list(dims.num_rows)
        self.nres = 11 * self.N
        self.block_nnz = [int(v) for v in dims.block_nnz]
        self.block_shape = [(int(s[0]), int(s[1])) for s in dims.block_shape]
        self.total_nnz = int(dims.total_nnz)
        self.V = int(dims.num_var_entries)
        self.algorithmic_bytes = int(dims.algorithmic_bytes)   # SURVEY 8(d) A_min per eval
        self.stored_bytes = int(dims.stored_bytes)             # residual + compact values actually written
        self.block_off = np.concatenate([[0], np.cumsum(self.block_nnz)]).astype(np.int64)
        self.row_off = {"mass": 0, "pos": self.N, "vel": 4 * self.N, "quat": 7 * self.N}
        self._pattern = None
        self._vals = None      # persistent full COO values (constants pre-filled)
        self._var_idx = None
        self._src = None
        self._nlin = self._nfn = 0
        self._cfg_gen = 0       # bumped by every (re)configuration of the row table or of an aero kind
        self.shard_plan_key = None   # (ranks, width, unit ranges) of the plan the handle holds (shard_plan)

    # ------------------------------------------------------------------
    def close(self):
        """Destroys the handle now.  Without close(), it goes when neither the engine nor a pinned view of it is left."""
        owner = self.__dict__.get("_owner")
        if owner is not None:
            owner.close()
            self._h = None
            # the pinned buffers died with the handle: drop the views this object handed out of them (arrays a caller still holds
            # point at freed memory, like any view of a closed resource)
            self.__dict__.pop("_pinned", None)
            self.__dict__.pop("_cb_out", None)
            self._vals = None

    # ------------------------------------------------------------------
    def D(self, i):
        n = int(self.num_nodes[i])
        out = np.zeros((n, n + 1))
        check(lib().gel_problem_D(self._h, i, _d(out)))
        return out

    def tau(self, i):
        out = np.zeros(int(self.num_nodes[i]))
        check(lib().gel_problem_tau(self._h, i, _d(out)))
        return out

    def pattern(self):
        """[(rows int32, cols int32)] for the 13 blocks (fixed; depends only on the static problem)."""
        if self._pattern is None:
            rows = np.zeros(self.total_nnz, dtype=np.int32)
            cols = np.zeros(self.total_nnz, dtype=np.int32)
            check(lib().gel_pattern_all(self._h, rows.ctypes.data_as(_ip), cols.ctypes.data_as(_ip)))   # one pass
            self._pattern = [(rows[self.block_off[b]:self.block_off[b + 1]].copy(),
                              cols[self.block_off[b]:self.block_off[b + 1]].copy()) for b in range(13)]
        return self._pattern

    def const_values(self):
        v = np.zeros(self.total_nnz)
        check(lib().gel_const_values(self._h, _d(v)))
        return v

    def var_index(self):
        if self._var_idx is None:
            idx = np.zeros(self.V, dtype=np.int64)
            check(lib().gel_var_index(self._h, idx.ctypes.data_as(_lp)))
            self._var_idx = idx
        return self._var_idx

    def full_source(self):
        """gather map full <- compact: -1 constant, s >= 0: compact[s], s <= -2: -compact[-2 - s]"""
        if self._src is None:
            src = np.zeros(self.total_nnz, dtype=np.int32)
            check(lib().gel_full_source(self._h, src.ctypes.data_as(_ip)))
            self._src = src
        return self._src

    def var_mask(self):
        """boolean [total_nnz]: entries that depend on x (everything the gather map takes from the compact vector)"""
        return self.full_source() != -1

    # ------------------------------------------------------------------
    def eval_residual(self, x):
        """-> (res [11N], status)"""
        x = _f64(x)
        assert x.size == self.nvars
        res = np.empty(self.nres)
        self._direct_call()
        rc = check(lib().gel_eval_residual(self._h, _d(x), _d(res)))
        return res, rc

    def _direct_call(self):
        """A one-vector call outside eval_callback rewrites the handle's pinned value array (the COO-direct path writes through
        it even when the caller names its own output) and residual vector -- the memory eval_callback hands out as its frame's
        `vals` / `res`.  A frame cached by the reference-named functions (con_dynamics._State.frame) is only valid for the
        generation it was evaluated in: bump it, so that the next mirror call evaluates again."""
        self._cfg_gen = getattr(self, "_cfg_gen", 0) + 1

    def eval_jacobian(self, x, out=None):
        """-> (vals_full [total_nnz], status).  `out` (from a previous call) is updated in place:
        only the x-dependent entries are rewritten."""
        x = _f64(x)
        assert x.size == self.nvars
        fill = 0
        if out is None:
            out = np.empty(self.total_nnz)
            fill = 1
        self._direct_call()
        rc = check(lib().gel_eval_jacobian(self._h, _d(x), _d(out), fill))
        return out, rc

    def pinned_buffers(self):
        """(res [11N], vals_full [total_nnz]): numpy views of the handle's own pinned host buffers (gel_pinned_buffers).  Passing
        them as `res_out` / `out` of eval / eval_jacobian (eval_callback uses them by itself) makes the one-vector calls
        zero-copy: the kernel writes the residual rows and every all-x-dependent block of the value vector straight into them.
        They belong to the engine and are rewritten by its next one-vector call."""
        pb = self.__dict__.get("_pinned")
        if pb is None:
            r, v, x0, x1 = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
            check(lib().gel_pinned_buffers(self._h, C.byref(r), C.byref(v), C.byref(x0), C.byref(x1)))
            dp = C.POINTER(C.c_double)
            # the views hold a reference to the handle's owner, not to this engine (every slice of them reaches it through .base):
            # the pinned memory is freed by close(), or once the engine and every one of these arrays are gone
            owner = self._owner

            def view(ptr, n):
                a = np.ctypeslib.as_array(C.cast(ptr, dp), shape=(n,)).view(_PinnedView)
                a._owner = owner
                return a
            res = view(r, self.nres)
            vals = view(v, max(self.total_nnz, 1))[:self.total_nnz]
            xb = [view(q, self.nvars) for q in (x0, x1)]
            pb = self._pinned = (res, vals, _d(res), _d(vals), xb, [_d(b) for b in xb])
        return pb[0], pb[1]

    def pinned_x(self):
        """-> ([x0, x1], [their ctypes pointers]): two pinned decision-vector buffers of the handle; a one-vector call whose x is
        one of them (eval_callback(x, .., xptr=pointer)) reads it in place instead of copying it into the staging buffer"""
        self.pinned_buffers()
        return self._pinned[4], self._pinned[5]

    def eval(self, x, out=None, res_out=None):
        """-> (res, vals_full, status).  out / res_out: arrays to write into (the engine's pinned_buffers() make it zero-copy)."""
        x = _f64(x)
        pb = self.__dict__.get("_pinned")
        if res_out is None:
            res, rp = np.empty(self.nres), None
        else:
            res = res_out
            rp = pb[2] if (pb is not None and res_out is pb[0]) else _d(res_out)
        fill = 0
        if out is None:
            out = np.empty(self.total_nnz)
            fill = 1
        vp = pb[3] if (pb is not None and out is pb[1]) else _d(out)
        self._direct_call()
        rc = check(lib().gel_eval(self._h, _d(x), rp if rp is not None else _d(res), vp, fill))
        return res, out, rc

    def eval_batch(self, X, want_res=True, want_jac=True, out=None):
        """X [B, nvars] -> (res [B, 11N] | None, jvar [B, V] | None, status).  `out` = (res, jvar) arrays of a
        previous call to write into (saves the page faults of fresh 100-MB arrays on large batches)."""
        X = _f64(X).reshape(-1, self.nvars)
        B = X.shape[0]
        if out is not None:
            res, jv = out
            for a, shp, want in ((res, (B, self.nres), want_res), (jv, (B, self.V), want_jac)):
                if want and (a is None or a.shape != shp or a.dtype != np.float64 or not a.flags.c_contiguous):
                    raise ValueError("out arrays must be C-contiguous float64 of shape %r" % (shp,))
        else:
            res = np.empty((B, self.nres)) if want_res else None
            jv = np.empty((B, self.V)) if want_jac else None
        rc = check(lib().gel_eval_batch(self._h, B, _d(X), _d(res) if want_res else None,
                                        _d(jv) if want_jac else None))
        return res, jv, rc

    def expand(self, jvar):
        """compact [.., V] -> full [.., total_nnz] on the host (numpy), using the constant template."""
        jvar = np.asarray(jvar)
        src = self.full_source()
        full = np.broadcast_to(self.const_values(), jvar.shape[:-1] + (self.total_nnz,)).copy()
        pos, neg = np.nonzero(src >= 0)[0], np.nonzero(src <= -2)[0]
        full[..., pos] = jvar[..., src[pos]]
        full[..., neg] = -jvar[..., -2 - src[neg]]
        return full

    # device-pointer API (pointers are integers, e.g. torch.Tensor.data_ptr())
    def eval_batch_device(self, B, d_x, d_res, d_jvar, stream=0):
        check(lib().gel_eval_batch_device(self._h, B, d_x, d_res or None, d_jvar or None, stream or None))

    def expand_full_device(self, B, d_jvar, d_jfull, stream=0):
        check(lib().gel_expand_full_device(self._h, B, d_jvar, d_jfull, stream or None))

    def fill_full_device(self, B, d_jfull, stream=0):
        """the constant template into d_jfull [B][total_nnz], once (then update_full_device after every evaluation)"""
        check(lib().gel_fill_full_device(self._h, B, d_jfull, stream or None))

    def update_full_device(self, B, d_jvar, d_jfull, stream=0):
        """only the x-dependent entries of d_jfull [B][total_nnz] from d_jvar [B][V] (the buffer holds the constants already)"""
        check(lib().gel_update_full_device(self._h, B, d_jvar, d_jfull, stream or None))

    def eval_full_device(self, B, d_x, d_res, d_jvar, d_jfull, stream=0):
        """one evaluation with every COO value valid in d_jfull [B][total_nnz] afterwards (fill_full_device once before): the fused
        launch + the update in place; a launch that fits the Infinity Cache keeps its compact values there for the update"""
        check(lib().gel_eval_full_device(self._h, B, d_x, d_res or None, d_jvar, d_jfull, stream or None))

    def launch_info(self, B, want_res=True, want_jac=True):
        """-> [jacobian, mfma, split, wavefronts, pack] of the kernel form a launch of B vectors takes"""
        info = (C.c_int32 * 5)()
        check(lib().gel_launch_info(self._h, int(B), int(bool(want_res)), int(bool(want_jac)), info))
        return [int(v) for v in info]

    def sync(self, stream=0):
        return check(lib().gel_sync(self._h, stream or None))

    # work items (one 64-node chunk of one phase each) for phase-sharded multi-GPU evaluation
    def num_chunks(self):
        n = C.c_int32()
        check(lib().gel_num_chunks(self._h, C.byref(n)))
        return n.value

    def chunk_phase(self):
        out = np.zeros(self.num_chunks(), dtype=np.int32)
        check(lib().gel_chunk_phase(self._h, out.ctypes.data_as(_ip)))
        return out

    def unit_owner(self):
        """(res_owner [11N], jvar_owner [V]): the unit (4 * work item + part) that writes each output entry"""
        ro = np.zeros(self.nres, dtype=np.int32)
        jo = np.zeros(self.V, dtype=np.int32)
        check(lib().gel_unit_owner(self._h, ro.ctypes.data_as(_ip), jo.ctypes.data_as(_ip)))
        return ro, jo

    def eval_shard_units_device(self, B, d_x, d_res, d_jvar, unit_begin, unit_count, stream=0):
        """unit = 4 * work_item + part (part 0: all but the three position sweeps; 1..3: one position sweep)."""
        check(lib().gel_eval_shard_units_device(self._h, B, d_x, d_res or None, d_jvar, int(unit_begin),
                                                int(unit_count), stream or None))

    def shard_plan(self, unit_begin):
        """Packed unit-shard exchange layout (gel_shard_plan) for ranks holding the contiguous unit ranges
        [unit_begin[r], unit_begin[r + 1]) -> (width, res_pos [11N], jvar_pos [V]); pos = rank * width + offset."""
        ub = np.ascontiguousarray(unit_begin, dtype=np.int32)
        width = C.c_int64(0)
        rp = np.zeros(self.nres, dtype=np.int64)
        jp = np.zeros(self.V, dtype=np.int64)
        _lp = C.POINTER(C.c_int64)
        check(lib().gel_shard_plan(self._h, len(ub) - 1, ub.ctypes.data_as(_ip), C.byref(width), rp.ctypes.data_as(_lp),
                                   jp.ctypes.data_as(_lp)))
        self.shard_plan_key = (len(ub) - 1, int(width.value), ub.tobytes())   # the plan the handle holds NOW (the next call replaces it)
        return int(width.value), rp, jp

    def eval_shard_packed_device(self, B, d_x, d_out, rank, stream=0, plan=None):
        """rank `rank`'s units of all B vectors straight into its slice of the exchange buffer d_out [nranks][B][width].
        plan = (nranks, width) the buffer was sized for (default: the handle's current plan); the call fails if the handle
        holds another plan by now."""
        if plan is None and self.shard_plan_key is None:
            raise _lib.GelatoAmdError("no shard plan on this handle: call shard_plan(unit_begin) first (or pass plan=(ranks, width))")
        nr, w = plan if plan is not None else self.shard_plan_key[:2]
        check(lib().gel_eval_shard_packed_device(self._h, B, d_x, d_out, int(rank), int(nr), int(w), stream or None))

    def shard_unpack_device(self, B, d_out, d_res, d_jvar, stream=0, plan=None):
        """exchange buffer -> the ordinary res [B][11N] / jvar [B][V] layouts (one gather launch; either may be 0)"""
        if plan is None and self.shard_plan_key is None:
            raise _lib.GelatoAmdError("no shard plan on this handle: call shard_plan(unit_begin) first (or pass plan=(ranks, width))")
        nr, w = plan if plan is not None else self.shard_plan_key[:2]
        check(lib().gel_shard_unpack_device(self._h, B, d_out, d_res or None, d_jvar or None, int(nr), int(w), stream or None))

    def jac_fd(self, group, x):
        gi = GROUPS.index(group)
        x = _f64(x)
        J = np.empty((self.nrows[gi], self.nvars))
        rc = check(lib().gel_jac_fd(self._h, gi, _d(x), _d(J)))
        return J, rc

    def jac_fd_block_dims(self, group):
        """-> (rows [S], cols [S], row0 [S], offset [S + 1]) of the group's per-phase blocks, (cols of phase i: global column of each
        local column) -- the phase's rows see only these columns (every other column of lib/jac_fd.py's dense result is zero)."""
        key = ("jfd_dims", group)
        if key not in self.__dict__:
            S = self.S
            r, c, r0, off = (np.zeros(S + (1 if k == 3 else 0), dtype=np.int64) for k in range(4))
            check(lib().gel_jac_fd_block_dims(self._h, GROUPS.index(group), *(a.ctypes.data_as(C.POINTER(C.c_int64)) for a in (r, c, r0, off))))
            cols = []
            for i in range(S):
                ci = np.zeros(int(c[i]), dtype=np.int32)
                check(lib().gel_jac_fd_block_cols(self._h, i, ci.ctypes.data_as(_ip)))
                cols.append(ci)
            self.__dict__[key] = (r, c, r0, off, cols)
        return self.__dict__[key]

    def jac_fd_blocks(self, group, x):
        """the group's forward-difference Jacobian as per-phase blocks: [(row0, global cols, block [rows, cols])], rc"""
        r, c, r0, off, cols = self.jac_fd_block_dims(group)
        x = _f64(x)
        buf = np.empty(int(off[-1]))
        rc = check(lib().gel_jac_fd_blocks(self._h, GROUPS.index(group), _d(x), _d(buf)))
        return [(int(r0[i]), cols[i], buf[int(off[i]):int(off[i + 1])].reshape(int(r[i]), int(c[i]))) for i in range(self.S)], rc

    def jac_fd_device(self, group, d_x, d_J, blocks=False, stream=0):
        """device pointers (ints): x [nvars] -> dense J [nrows[group]][nvars] or the blocks (jac_fd_block_dims), all in HBM"""
        check(lib().gel_jac_fd_device(self._h, GROUPS.index(group), d_x, d_J, 1 if blocks else 0, stream or None))

    # ---- aero path constraints (lib/con_aero.py): kind in AERO_KINDS ----
    AERO_KINDS = ["alpha", "q", "qalpha"]
    AERO_VARS = ["position", "velocity", "quaternion", "t"]

    def aero_configure(self, kind, spec):
        """spec: rows of (phase, range_all, limit); limit = units[3] of con_aero.py."""
        spec = np.asarray(spec, dtype=np.float64).reshape(-1, 3)
        ph = np.ascontiguousarray(spec[:, 0], dtype=np.int32)
        ra = np.ascontiguousarray(spec[:, 1], dtype=np.int32)
        lim = _f64(spec[:, 2])
        check(lib().gel_aero_configure(self._h, self.AERO_KINDS.index(kind), len(ph), ph.ctypes.data_as(_ip),
                                       ra.ctypes.data_as(_ip), _d(lim)))
        self._aero_dims = {}
        self._aero_out = {}
        self._cb_out = {}
        self._cfg_gen = getattr(self, "_cfg_gen", 0) + 1

    def aero_dims(self, kind):
        d = self.__dict__.setdefault("_aero_dims", {})
        if kind not in d:
            n = C.c_int32()
            nnz = (C.c_int64 * 4)()
            check(lib().gel_aero_dims(self._h, self.AERO_KINDS.index(kind), C.byref(n), nnz))
            d[kind] = (n.value, [int(v) for v in nnz])
        return d[kind]

    def aero_pattern(self, kind):
        nrow, nnz = self.aero_dims(kind)
        out = []
        for v in range(4):
            r = np.zeros(nnz[v], dtype=np.int32)
            c = np.zeros(nnz[v], dtype=np.int32)
            check(lib().gel_aero_pattern(self._h, self.AERO_KINDS.index(kind), v, r.ctypes.data_as(_ip),
                                         c.ctypes.data_as(_ip)))
            out.append((r, c))
        return out

    def eval_aero(self, kind, X, want_jac=True):
        """X [B, nvars] (or [nvars]) -> (con [B, nrows], jac_vals [B, sum nnz] | None, status)"""
        X = _f64(X).reshape(-1, self.nvars)
        B = X.shape[0]
        nrow, nnz = self.aero_dims(kind)
        con = np.empty((B, nrow))
        jv = np.empty((B, sum(nnz))) if want_jac else None
        rc = check(lib().gel_eval_aero(self._h, self.AERO_KINDS.index(kind), B, _d(X), _d(con),
                                       _d(jv) if want_jac else None))
        return con, jv, rc

    def eval_aero_all(self, X, want_jac=True, kinds=None, reuse=False):
        """all configured kinds in one launch: X [B, nvars] (or [nvars]) -> ({kind: con [B, nrows]}, {kind: jac_vals} | None,
        status); kinds without rows are left out.  reuse=True hands out the engine's own output arrays (overwritten by
        the next call of the same shape) instead of fresh ones."""
        X = _f64(X).reshape(-1, self.nvars)
        B = X.shape[0]
        key = (B, bool(want_jac), None if kinds is None else tuple(kinds))
        slot = self.__dict__.setdefault("_aero_out", {}).get(key) if reuse else None
        if slot is None:
            con, jac = {}, {}
            cp, jp = (_dp * 3)(), (_dp * 3)()
            for i, kind in enumerate(self.AERO_KINDS):
                nrow, nnz = self.aero_dims(kind)
                if nrow and (kinds is None or kind in kinds):
                    con[kind] = np.empty((B, nrow))
                    cp[i] = _d(con[kind])
                    if want_jac:
                        jac[kind] = np.empty((B, sum(nnz)))
                        jp[i] = _d(jac[kind])
            slot = (con, jac, cp, jp)
            if reuse:
                self._aero_out[key] = slot
        con, jac, cp, jp = slot
        rc = check(lib().gel_eval_aero_all(self._h, B, _d(X), cp, jp if want_jac else None))
        return con, (jac if want_jac else None), rc

    def eval_aero_all_device(self, B, d_x, d_con, d_jac=None, stream=0):
        """device pointers (ints): d_con / d_jac = 3 entries per kind (0 = not wanted)"""
        cp = (C.c_void_p * 3)(*[p or None for p in d_con])
        jp = (C.c_void_p * 3)(*[p or None for p in d_jac]) if d_jac is not None else None
        check(lib().gel_eval_aero_all_device(self._h, B, d_x, cp, jp, stream or None))

    def aero_record_layout(self):
        """-> (width, {kind: con index [nrows]}, {kind: jac index [sum nnz]}): the per-vector record of eval_batch_aero_device and
        the gather that restores eval_aero_all's arrays from it -- con[kind] = aero_gather(record, con_idx[kind]), jac likewise (the four
        blocks position | velocity | quaternion | t concatenated, as eval_aero_all returns them; index -1: an exact zero, not stored)"""
        w = C.c_int64()
        oc, oj = (C.c_int64 * 6)(), (C.c_int64 * 6)()
        check(lib().gel_aero_record_layout(self._h, C.byref(w), oc, oj))
        con, jac = {}, {}
        for i, kind in enumerate(self.AERO_KINDS):
            nrow, nnz = self.aero_dims(kind)
            ci = np.zeros(nrow, dtype=np.int64)
            if nrow:
                check(lib().gel_aero_record_map(self._h, i, -1, ci.ctypes.data_as(_lp)))
            parts = []
            for v in range(4):
                ji = np.zeros(nnz[v], dtype=np.int64)
                if nnz[v]:
                    check(lib().gel_aero_record_map(self._h, i, v, ji.ctypes.data_as(_lp)))
                parts.append(ji)
            con[kind], jac[kind] = ci, np.concatenate(parts)
        return int(w.value), con, jac

    @staticmethod
    def aero_gather(records, idx):
        """records [..., width], idx from aero_record_layout -> the reference's array; index -1 = an exact zero that is not stored"""
        records = np.asarray(records)
        out = records[..., np.maximum(idx, 0)]
        if (idx < 0).any():
            out[..., idx < 0] = 0.0
        return out

    def eval_batch_aero_device(self, B, d_x, d_res, d_jvar, d_aero, stream=0):
        """defect groups + aero path constraints of a resident batch (device pointers as ints): res [B, nres], jvar [B, V] as
        eval_batch_device, aero [B, width] one record per vector (aero_record_layout)"""
        check(lib().gel_eval_batch_aero_device(self._h, B, d_x, d_res, d_jvar, d_aero, stream or None))

    def aero_launch_info(self, B, records=False):
        """-> {"flat", "runs", "run_len", "max_bytes"}: the form aero_kernel's launcher takes for B vectors (gel_aero_launch_info) --
        records=False: the dense arrays of eval_aero_all_device; True: part A of eval_batch_aero_device's records where aero_kernel
        writes it.  A last, shorter run decides its own form: ask with its length."""
        info = (C.c_int64 * 4)()
        check(lib().gel_aero_launch_info(self._h, int(B), int(bool(records)), info))
        return dict(zip(("flat", "runs", "run_len", "max_bytes"), (int(v) for v in info)))

    def eval_callback(self, x, want_jac, xptr=None):
        """ONE device round trip for one decision vector: the four defect groups, the row table (if configured) and the aero
        kinds (if configured), values only or values + derivatives.  -> dict of the engine's own output arrays (overwritten
        by the next call): res, vals (full COO values) | None, rows_con, rows_jfn | None, aero_con {kind}, aero_jac {kind} |
        None, rc."""
        if xptr is None:      # xptr: the caller's cached pointer to x (a persistent, contiguous float64 buffer of nvars doubles)
            x = _f64(x)
            assert x.size == self.nvars
            xptr = _d(x)
        key = bool(want_jac)
        slot = self.__dict__.setdefault("_cb_out", {}).get(key)
        if slot is None:
            io = GelCallbackIO()
            # the handle's own pinned buffers: the kernel writes the residual rows and the all-x-dependent blocks of the value
            # vector straight into them (gel_pinned_buffers: no host copy of either)
            pres, pvals = self.pinned_buffers()
            out = {"res": pres, "vals": None, "rows_con": None, "rows_jfn": None, "aero_con": {}, "aero_jac": {}}
            io.res = self._pinned[2]
            if want_jac:
                if self._vals is None:
                    self._vals = pvals          # constants in place; x-dependent entries rewritten per call
                out["vals"] = self._vals
                io.vals_full, io.fill_constants = (self._pinned[3] if self._vals is pvals else _d(self._vals)), 0
            if self._nlin + self._nfn:
                out["rows_con"] = np.empty(self._nlin + self._nfn)
                io.rows_con = _d(out["rows_con"])
                if want_jac:
                    out["rows_jfn"] = np.empty((max(self._nfn, 1), 7))
                    io.rows_jfn = _d(out["rows_jfn"])
            for i, kind in enumerate(self.AERO_KINDS):
                nrow, nnz = self.aero_dims(kind)
                if nrow:
                    out["aero_con"][kind] = np.empty(nrow)
                    io.aero_con[i] = _d(out["aero_con"][kind])
                    if want_jac:
                        out["aero_jac"][kind] = np.empty(sum(nnz))
                        io.aero_jac[i] = _d(out["aero_jac"][kind])
            slot = (io, out)
            self._cb_out[key] = slot
        io, out = slot
        out["rc"] = check(lib().gel_eval_callback(self._h, xptr, C.byref(io)))
        if out["rows_jfn"] is not None:
            out["rows_jfn"] = out["rows_jfn"][:self._nfn]
        return out

    OUTPUT_COLUMNS = ["thrust", "lat", "lon", "lat_IIP", "lon_IIP", "downrange", "altitude", "altitude_apogee", "altitude_perigee",
                      "inclination", "argument_perigee", "lon_ascending_node", "true_anomaly", "vel_ground_NED_X",
                      "vel_ground_NED_Y", "vel_ground_NED_Z", "accel_BODY_X", "aero_BODY_X", "heading_NED2BODY", "pitch_NED2BODY",
                      "roll_NED2BODY", "flightpath_vel_inertial_geocentric", "azimuth_vel_inertial_geocentric",
                      "thrust_direction_ECI_X", "thrust_direction_ECI_Y", "thrust_direction_ECI_Z", "vel_ground", "vel_air",
                      "AOA_total", "AOA_pitch", "AOA_yaw", "dynamic_pressure", "Q_alpha", "M"]   # gel_output_column

    def output_table(self, x, tx_res, launch_lat, launch_lon):
        """x [nvars], tx_res [M] (seconds) -> [M, 34] derived quantities of the reference's post-processing table
        (output_result.py:121-262), columns OUTPUT_COLUMNS; one device thread per state node"""
        x, tx = _f64(x), _f64(tx_res)
        if x.shape != (self.nvars,) or tx.shape != (self.M,):
            raise ValueError("x must have nvars entries and tx_res one time per state node")
        out = np.empty((self.M, len(self.OUTPUT_COLUMNS)))
        check(lib().gel_output_table(self._h, _d(x), _d(tx), float(launch_lat), float(launch_lon), _d(out)))
        return out

    ENVELOPE_FIELDS = ("count", "mean", "m2", "min", "max", "argmin", "argmax", "first_nonfinite")   # GEL_ENV_NSTAT
    PEAK_FIELDS = ("min", "argmin", "max", "argmax")                                                     # GEL_PEAK_NSTAT

    def _output_columns(self, columns):
        """column names or gel_output_column values -> (names, int32 ids | None for all 34 in order)"""
        if columns is None:
            return list(self.OUTPUT_COLUMNS), None
        ids = []
        for c in columns:
            if isinstance(c, str):
                if c not in self.OUTPUT_COLUMNS:
                    raise ValueError("unknown output column %r" % (c,))
                ids.append(self.OUTPUT_COLUMNS.index(c))
            else:
                ids.append(int(c))
        if not ids or len(set(ids)) != len(ids) or min(ids) < 0 or max(ids) >= len(self.OUTPUT_COLUMNS):
            raise ValueError("columns: 1 .. %d distinct columns of OUTPUT_COLUMNS" % len(self.OUTPUT_COLUMNS))
        return [self.OUTPUT_COLUMNS[i] for i in ids], np.asarray(ids, dtype=np.int32)

    def output_table_batch(self, X, launch_lat, launch_lon, tx=None, dispersion=None, columns=None, table=True, envelope=True,
                           peaks=True, ensemble=None):
        """The post-processing table of a batch with its envelope and peaks (gel_output_table_batch).
        X [B, nvars] (or [nvars]); tx None (every vector's node times from its own knots) or [B, M] seconds; dispersion None or
        float64 [B, S, 4] as PropagationPlan.apply takes it (the mass-flow factor has no reader here); columns None (all of
        OUTPUT_COLUMNS) or a list of distinct names; ensemble None or a WindEnsemble of this engine assigned B vectors: every
        vector's rows take the wind of the table its entry selects (gel_output_table_batch_ensemble).
        -> {"columns": names, "table": [B, M, ncols] | None,
            "envelope": {name: {count [M] int, mean, std (sqrt(m2 / (count - 1)), NaN where count < 2), m2, min, max [M],
                                argmin, argmax, first_nonfinite [M] int (-1: none)}} | None   -- per node over the vectors,
            "peaks": {name: {min, max [B], argmin, argmax [B] int (node; -1: no finite entry)}} | None   -- per vector over the nodes}"""
        if not (table or envelope or peaks):
            raise ValueError("output_table_batch: no output selected (table, envelope and peaks are all off)")
        names, ids = self._output_columns(columns)
        X = _f64(X)
        if X.ndim == 1:
            X = X[None]
        if X.ndim != 2 or X.shape[1] != self.nvars:
            raise ValueError("X: [B, nvars] = [B, %d], not %s" % (self.nvars, X.shape))
        B, M, nc = X.shape[0], self.M, len(names)
        if tx is not None:
            tx = _f64(tx)
            if tx.shape == (M,) and B == 1:
                tx = tx[None]
            if tx.shape != (B, M):
                raise ValueError("tx: [B, M] = %s, not %s" % ((B, M), tx.shape))
        disp = None
        if dispersion is not None:
            disp = np.asarray(dispersion)
            if disp.dtype != np.float64:
                raise TypeError("dispersion: float64")
            if disp.shape == (self.S, _lib.GEL_PROP_NDISP) and B == 1:
                disp = disp[None]
            if disp.shape != (B, self.S, _lib.GEL_PROP_NDISP):
                raise ValueError("dispersion: [B, S, %d] = %s, not %s" % (_lib.GEL_PROP_NDISP, (B, self.S, _lib.GEL_PROP_NDISP), disp.shape))
            disp = np.ascontiguousarray(disp)
        out = np.empty((B, M, nc)) if table else None
        env = np.empty((M, nc, _lib.GEL_ENV_NSTAT)) if envelope else None
        pk = np.empty((B, nc, _lib.GEL_PEAK_NSTAT)) if peaks else None
        check(lib().gel_output_table_batch_ensemble(self._h, B, _d(X), _d(tx) if tx is not None else None,
                                                    _d(disp) if disp is not None else None, _ensemble_ptr(ensemble, self._owner),
                                                    float(launch_lat), float(launch_lon), nc,
                                                    ids.ctypes.data_as(_ip) if ids is not None else None, _d(out) if table else None,
                                                    _d(env) if envelope else None, _d(pk) if peaks else None))
        res = {"columns": names, "table": out, "envelope": None, "peaks": None}
        if envelope:
            res["envelope"] = {}
            for k, name in enumerate(names):
                e = {f: env[:, k, j] for j, f in enumerate(self.ENVELOPE_FIELDS)}
                for f in ("count", "argmin", "argmax", "first_nonfinite"):
                    e[f] = e[f].astype(np.int64)
                with np.errstate(invalid="ignore", divide="ignore"):
                    e["std"] = np.where(e["count"] >= 2, np.sqrt(e["m2"] / np.maximum(e["count"] - 1, 1)), np.nan)
                res["envelope"][name] = e
        if peaks:
            res["peaks"] = {}
            for k, name in enumerate(names):
                q = {f: pk[:, k, j] for j, f in enumerate(self.PEAK_FIELDS)}
                for f in ("argmin", "argmax"):
                    q[f] = q[f].astype(np.int64)
                res["peaks"][name] = q
        return res

    def output_table_batch_device(self, B, d_x, launch_lat, launch_lon, d_tx=0, d_dispersion=0, columns=None, d_out=0, d_env=0,
                                  d_peaks=0, ensemble=None):
        """device buffers (raw pointers; 0 = not given): d_out [B][M][ncols], d_env [M][ncols][8], d_peaks [B][ncols][4];
        ensemble: None or a WindEnsemble of this engine assigned B vectors; asynchronous on the engine's own stream; status
        through Engine.sync()"""
        names, ids = self._output_columns(columns)
        check(lib().gel_output_table_batch_ensemble_device(self._h, int(B), d_x or None, d_tx or None, d_dispersion or None,
                                                           _ensemble_ptr(ensemble, self._owner), float(launch_lat), float(launch_lon),
                                                           len(names), ids.ctypes.data_as(_ip) if ids is not None else None,
                                                           d_out or None, d_env or None, d_peaks or None))

    @staticmethod
    def _quantile_probs(probs):
        p = np.atleast_1d(np.asarray(probs, dtype=np.float64)).copy()
        if p.ndim != 1 or not 1 <= p.size <= _lib.GEL_QUANT_MAXQ:
            raise ValueError("probs: 1 .. %d probabilities, not shape %s" % (_lib.GEL_QUANT_MAXQ, p.shape))
        if not np.all((p >= 0.0) & (p <= 1.0)):
            raise ValueError("probs: numbers in [0, 1], not %s" % (p,))
        return p

    @staticmethod
    def quantile_value(probs, count, lower, upper):
        """the interpolated quantile lower + (upper - lower) (h - lo), h = p (count - 1), lo = floor(h); NaN where count = 0.
        probs [nq]; count [...]; lower, upper [..., nq].  (Where upper - lower overflows, between two ranks 1.8e308 apart, so does
        the value: lower and upper are the exact answer there.)"""
        p = np.asarray(probs, dtype=np.float64)
        n1 = np.maximum(np.asarray(count, dtype=np.int64) - 1, 0).astype(np.float64)[..., None]
        h = p * n1
        with np.errstate(invalid="ignore", over="ignore"):
            v = lower + (upper - lower) * (h - np.floor(h))
        return np.where(np.asarray(count)[..., None] > 0, v, np.nan)

    def batch_quantiles(self, A, probs, who=False):
        """Exact quantiles over the first axis of A (gel_batch_quantiles).  A: float64 [B, W], or any C-contiguous
        [B, ...], flattened behind the first axis; probs: 1 .. 16 probabilities in [0, 1].
        -> {"probs" [nq], "count" [W] int64 (the finite entries of a column), "lower", "upper" [W, nq]: the floor(h)-th and ceil(h)-th
            finite entry in key order, h = p (count - 1), bit copies of entries of A (NaN where count = 0),
            "value" [W, nq]: lower + (upper - lower) (h - floor(h)), formed here,
            "who_lower", "who_upper" [W, nq] int64 (who=True): the lowest b whose entry is that one; -1 where count = 0}"""
        p = self._quantile_probs(probs)
        A = np.asarray(A)
        if A.dtype != np.float64:
            raise TypeError("A: float64, not %s" % A.dtype)
        if A.ndim < 1:
            raise ValueError("A: [B, ...]")
        if not A.flags.c_contiguous:
            raise ValueError("A: C-contiguous")
        B = A.shape[0]
        W = int(np.prod(A.shape[1:], dtype=np.int64)) if A.ndim > 1 else 1
        nq = p.size
        q = np.empty((W, nq, 2))
        cnt = np.empty(W)
        wh = np.empty((W, nq, 2)) if who else None
        check(lib().gel_batch_quantiles(self._h, B, W, W, _d(A) if A.size else None, nq, _d(p), _d(q), _d(cnt), _d(wh) if who else None))
        count = cnt.astype(np.int64)
        lower, upper = np.ascontiguousarray(q[:, :, 0]), np.ascontiguousarray(q[:, :, 1])
        res = {"probs": p, "count": count, "lower": lower, "upper": upper, "value": self.quantile_value(p, count, lower, upper)}
        if who:
            res["who_lower"], res["who_upper"] = wh[:, :, 0].astype(np.int64), wh[:, :, 1].astype(np.int64)
        return res

    def batch_quantiles_device(self, B, W, ld, d_src, probs, d_q, d_count=0, d_who=0):
        """device buffers (raw pointers; 0 = not given): d_src [B][ld] of which columns 0 .. W - 1 are read, d_q [W][nq][2], d_count
        [W], d_who [W][nq][2]; probs stays on the host; asynchronous on the engine's own stream; status through Engine.sync()"""
        p = self._quantile_probs(probs)
        check(lib().gel_batch_quantiles_device(self._h, int(B), int(W), int(ld), d_src or None, p.size, _d(p), d_q or None, d_count or None,
                                               d_who or None))

    def batch_quantiles_info(self, B, W, nq):
        """-> {"bins", "cap", "chunk", "slab_cols", "workspace_bytes", "workspace_cap_bytes", "passes", "slabs"}: what a call
        would select (gel_batch_quantiles_info; needs no GPU)"""
        info = _lib.GelQuantilesInfo()
        check(lib().gel_batch_quantiles_info(self._h, int(B), int(W), int(nq), C.byref(info)))
        return {k: int(getattr(info, k)) for k, _t in info._fields_}

    def batch_quantiles_last(self):
        """-> {"targets", "by_range", "by_candidates", "by_fallback"}: how the (column, rank) pairs of the last batch_quantiles*
        call were settled (gel_batch_quantiles_last; waits for the engine's stream)"""
        st = (C.c_int64 * 4)()
        check(lib().gel_batch_quantiles_last(self._h, st))
        return dict(zip(("targets", "by_range", "by_candidates", "by_fallback"), (int(v) for v in st)))

    @staticmethod
    def comoment_ratios(count, C_, m2_a, m2_b):
        """-> (cov, corr): cov = C / (count - 1), NaN below a count of 2; corr = C / sqrt(m2_a m2_b), NaN where an m2 is 0.  numpy."""
        C_, m2_a, m2_b = np.asarray(C_, dtype=np.float64), np.asarray(m2_a, dtype=np.float64), np.asarray(m2_b, dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            cov = C_ / (count - 1) if count >= 2 else np.full(C_.shape, np.nan)
            den = np.sqrt(m2_a[:, None] * m2_b[None, :])
            corr = np.where(den > 0.0, C_ / np.where(den > 0.0, den, 1.0), np.nan)
        return cov, corr

    def batch_comoments(self, A, Bv=None):
        """Co-moments over the first axis (gel_batch_comoments).  A: C-contiguous float64 [B, Wa]; Bv: [B, Wb], or
        None = the self form (Bv is A; only the pairs i <= j are formed, C is symmetric in bits).  A flight counts iff every entry
        of its rows of A and Bv is finite (listwise).
        -> {"count" int, "first_excluded" int (-1: none), "C" [Wa, Wb] = sum (a_i - mean a_i)(b_j - mean b_j) over the counted
            flights, "mean_a", "m2_a" [Wa], "mean_b", "m2_b" [Wb] (the self form: those of a), "cov" = C / (count - 1) (NaN below
            2), "corr" = C / sqrt(m2_a m2_b) (NaN where an m2 is 0) -- cov and corr formed here in numpy}"""
        def arr(X, name):
            X = np.asarray(X)
            if X.dtype != np.float64:
                raise TypeError("%s: float64, not %s" % (name, X.dtype))
            if X.ndim != 2:
                raise ValueError("%s: [B, W]" % name)
            if not X.flags.c_contiguous:
                raise ValueError("%s: C-contiguous" % name)
            return X
        A = arr(A, "A")
        B, Wa = A.shape
        self_form = Bv is None
        if self_form:
            Wb = Wa
        else:
            Bv = arr(Bv, "Bv")
            if Bv.shape[0] != B:
                raise ValueError("Bv: %d rows, A has %d" % (Bv.shape[0], B))
            Wb = Bv.shape[1]
        Cm = np.full((Wa, Wb), np.nan)
        sa, sb, info = np.full((Wa, 2), np.nan), np.full((Wb, 2), np.nan), np.empty(2)
        check(lib().gel_batch_comoments(self._h, B, Wa, 1, max(Wa, 1), _d(A) if A.size else None, Wb, 1, max(Wb, 1),
                                        None if self_form else _d(Bv), _d(Cm) if Cm.size else None, _d(sa) if Wa else None,
                                        None if self_form or not Wb else _d(sb), _d(info)))
        if self_form:
            sb = sa
        count = int(info[0])
        cov, corr = self.comoment_ratios(count, Cm, sa[:, 1], sb[:, 1])
        return {"count": count, "first_excluded": int(info[1]), "C": Cm, "mean_a": sa[:, 0].copy(), "m2_a": sa[:, 1].copy(),
                "mean_b": sb[:, 0].copy(), "m2_b": sb[:, 1].copy(), "cov": cov, "corr": corr}

    def batch_comoments_device(self, B, Wa, inca, lda, d_a, Wb, incb, ldb, d_b, d_C, d_stat_a=0, d_stat_b=0, d_info=0):
        """device buffers (raw pointers; 0 = not given): column i of flight r of a is d_a[r lda + i inca] (b likewise; d_b = 0: the
        self form), d_C [Wa][Wb], d_stat_a [Wa][2], d_stat_b [Wb][2], d_info [2] (required); asynchronous on the engine's own
        stream; status through Engine.sync()"""
        check(lib().gel_batch_comoments_device(self._h, int(B), int(Wa), int(inca), int(lda), d_a or None, int(Wb), int(incb), int(ldb),
                                               d_b or None, d_C or None, d_stat_a or None, d_stat_b or None, d_info or None))

    def batch_comoments_info(self, B, Wa, Wb=None):
        """-> {"block", "tile_a", "tile_b", "slab_rows", "slab_cols", "slabs", "workspace_bytes", "workspace_cap_bytes", "passes_a",
        "passes_b"}: what a call would select (gel_batch_comoments_info; needs no GPU).  Wb = None: the self form"""
        info = _lib.GelComomentsInfo()
        check(lib().gel_batch_comoments_info(self._h, int(B), int(Wa), int(Wa if Wb is None else Wb), 1 if Wb is None else 0, C.byref(info)))
        return {k: int(getattr(info, k)) for k, _t in info._fields_}

    def initial_guess(self, t_ref, table, knot_times):
        """initialize.py:322-409 behind the C-ABI: reference trajectory (t_ref [n], table [n, 13] = mass | pos 3 | vel 3 |
        quat 4 | body rates y, z) interpolated at the mesh's node times -> packed decision vector"""
        t_ref, table, knot_times = _f64(t_ref), _f64(table), _f64(knot_times)
        assert table.shape == (t_ref.size, 13) and knot_times.size == self.S + 1
        x = np.empty(self.nvars)
        rc = check(lib().gel_initial_guess(self._h, t_ref.size, _d(t_ref), _d(table), _d(knot_times), _d(x)))
        if rc == _lib.GEL_NONFINITE:
            # np.interp semantics of the reference (initialize.py:346-409): a node time on a zero-width interval of the table
            # (a repeated time at either end) extrapolates to NaN / Inf there; the guess is returned as the reference would
            # return it, with a warning
            import warnings
            warnings.warn("initial_guess: non-finite node values (the reference table repeats a time where a node time "
                          "falls): %d of %d" % (int(np.count_nonzero(~np.isfinite(x))), x.size), RuntimeWarning, stacklevel=2)
        return x

    # ---- knot / terminal / user rows (lib/con_init_terminal_knot.py, example/user_constraints.py) ----
    NODE_FUNCTIONS = {"orbit_energy": 0, "angular_momentum": 1, "inclination_rad": 2, "semi_major_axis": 3,
                      "eccentricity": 4, "periapsis_radius": 5, "apoapsis_radius": 6, "radius": 7, "speed": 8,
                      "latitude_deg": 9, "longitude_deg": 10, "altitude": 11, "lat_IIP_deg": 12, "lon_IIP_deg": 13,
                      "sin_elevation": 14, "downrange": 15}
    # row modes (include/gelato_amd.h): value f / p0 - p1 | (f - p1) / p0; difference of the value | scaled raw difference
    MODE_SHIFTED, MODE_RAW_DIFFERENCE, MODE_NEGATED = 1, 4, 8

    def var_offset(self, key):
        """first index of xdict[key] inside the packed decision vector"""
        M, N = self.M, self.N
        return {"mass": 0, "position": M, "velocity": 4 * M, "quaternion": 7 * M, "u": 11 * M, "t": 11 * M + 2 * N}[key]

    def rows_configure(self, linear, nodefn):
        """linear: rows (idx0, coef0, idx1 | -1, coef1, c0) -> (coef0 x[idx0] + coef1 x[idx1]) + c0;
        nodefn: rows (fn, node, p0, p1) -> f(r, v at state node) / p0 - p1 with its forward difference, or the long form
        (fn, node, tcol, mode, [p0 .. p7]) of include/gelato_amd.h (functions of the knot time, other value / difference forms)."""
        lin = (GelLinearRow * max(1, len(linear)))()
        for k, (i0, c0_, i1, c1_, cc) in enumerate(linear):
            lin[k] = GelLinearRow(int(i0), int(i1), float(c0_), float(c1_), float(cc))
        fn = (GelNodefnRow * max(1, len(nodefn)))()
        for k, row in enumerate(nodefn):
            if len(row) == 4:
                f, node, p0, p1 = row
                tcol, mode, pp = -1, 0, [p0, p1]
            else:
                f, node, tcol, mode, pp = row
            pp = [float(v) for v in pp] + [0.0] * (8 - len(pp))
            fn[k] = GelNodefnRow(int(self.NODE_FUNCTIONS.get(f, f)), int(node), int(tcol), int(mode), (C.c_double * 8)(*pp))
        check(lib().gel_rows_configure(self._h, len(linear), lin, len(nodefn), fn))
        self._nlin, self._nfn = len(linear), len(nodefn)
        self._cb_out = {}
        self._cfg_gen = getattr(self, "_cfg_gen", 0) + 1

    def rows_eval(self, X, want_jac=True):
        """X [B, nvars] (or [nvars]) -> (con [B, nlin + nfn], jfn [B, nfn, 7] | None, status); the seven difference columns
        are position xyz, velocity xyz of the row's node, then its knot time"""
        X = _f64(X).reshape(-1, self.nvars)
        B = X.shape[0]
        con = np.empty((B, self._nlin + self._nfn))
        jfn = np.empty((B, self._nfn, 7)) if want_jac else None
        rc = check(lib().gel_rows_eval(self._h, B, _d(X), _d(con), _d(jfn) if want_jac else None))
        return con, jfn, rc

    def rows_eval_device(self, B, d_x, d_con, d_jfn, stream=0):
        check(lib().gel_rows_eval_device(self._h, B, d_x, d_con, d_jfn or None, stream or None))

    # ------------------------------------------------------------------
    # collocation error estimate per section (include/gelato_amd.h gel_mesh_*)
    MESH_GROUPS = ("mass", "position", "velocity", "quaternion")

    def mesh_npts(self):
        """test points of the estimate: sum over phases of n + 1 (the rows of mesh_error's diff)"""
        n = C.c_int32()
        check(lib().gel_mesh_dims(self._h, C.byref(n)))
        return int(n.value)

    def mesh_matrices(self, phase):
        """{"sigma" [n+1], "Lx" [n+1, n+1], "Lu" [n+1, n], "I" [n+1, n+1]} of one phase (works on host-only handles)"""
        n = int(self.num_nodes[phase])
        P = n + 1
        out = {"sigma": np.zeros(P), "Lx": np.zeros((P, P)), "Lu": np.zeros((P, n)), "I": np.zeros((P, P))}
        check(lib().gel_mesh_matrices(self._h, int(phase), _d(out["sigma"]), _d(out["Lx"]), _d(out["Lu"]), _d(out["I"])))
        return out

    def mesh_error(self, X, want_diff=False):
        """X [B, nvars] (or [nvars]) -> (err [B, S, 4] (mass, position, velocity, quaternion), diff [B, npts, 11] | None, status)"""
        X = _f64(X).reshape(-1, self.nvars)
        B = X.shape[0]
        err = np.empty((B, self.S, 4))
        diff = np.empty((B, self.mesh_npts(), 11)) if want_diff else None
        rc = check(lib().gel_mesh_error(self._h, B, _d(X), _d(err), _d(diff) if want_diff else None))
        return err, diff, rc

    def mesh_error_device(self, B, d_x, d_err, d_diff=0, stream=0):
        """device buffers: d_err [B][S][4], d_diff [B][npts][11] or 0; status through sync()"""
        check(lib().gel_mesh_error_device(self._h, int(B), d_x, d_err, d_diff or None, stream or None))

    # ------------------------------------------------------------------
    # spectral interpolation: dense output and mesh transfer (include/gelato_amd.h gel_interp_*)
    def interp_plan(self, points, unit_quat=False):
        """points: a list of S arrays of points inside [-1, 1] (an empty one: no output for that phase) -> InterpPlan whose
        apply(X) gives [B, npts, 14] = time | mass, position, velocity, quaternion | u at the points, in x's normalised units"""
        if len(points) != self.S:
            raise ValueError("points: one array per phase (%d)" % self.S)
        pts = [_f64(np.asarray(p, dtype=np.float64).ravel()) for p in points]
        npts = np.array([p.size for p in pts], dtype=np.int32)
        allp = _f64(np.concatenate(pts)) if pts else np.zeros(0)
        h = C.c_void_p()
        check(lib().gel_interp_plan_create(self._h, npts.ctypes.data_as(_ip), _d(allp), int(bool(unit_quat)), C.byref(h)))
        return InterpPlan(self._owner, h, self.num_nodes, npts, npts)

    def transfer_plan(self, dst_engine, unit_quat=False):
        """-> InterpPlan whose apply(X) gives [B, dst nvars]: the decision vectors carried to dst_engine's mesh (the same number
        of phases; dst_engine may be host-only and may be closed afterwards)"""
        h = C.c_void_p()
        check(lib().gel_interp_plan_create_transfer(self._h, dst_engine._h, int(bool(unit_quat)), C.byref(h)))
        nd = [int(v) for v in dst_engine.num_nodes]
        return InterpPlan(self._owner, h, self.num_nodes, [n + 1 for n in nd], nd)

    # ------------------------------------------------------------------
    # explicit RK4 propagation of the sections: the shooting check (include/gelato_amd.h gel_prop_*)
    def propagation_plan(self, steps=4, restart="section"):
        """steps: RK4 steps per node interval, one number or one per phase; restart: "section" (integrate from the section's
        first state to its last node), "node" (every node interval starts from the collocated state) or "chain" (one flight per
        vector: the state is carried across the knots, with the collocated jump added) -> PropagationPlan"""
        if restart not in ("section", "node", "chain"):
            raise ValueError("restart: 'section', 'node' or 'chain'")
        st = np.asarray(steps)
        if st.ndim > 1 or (st.ndim == 1 and st.size != self.S):
            raise ValueError("steps: one number, or one per phase (%d)" % self.S)
        if not np.issubdtype(st.dtype, np.integer):
            raise TypeError("steps: integers")
        st = np.ascontiguousarray(np.broadcast_to(st, (self.S,)), dtype=np.int32)
        h = C.c_void_p()
        check(lib().gel_prop_plan_create(self._h, st.ctypes.data_as(_ip), {"section": 0, "node": _lib.GEL_PROP_RESTART_NODE, "chain": _lib.GEL_PROP_CHAIN}[restart], C.byref(h)))
        return PropagationPlan(self._owner, h, self.num_nodes, st, (self.S, self.M, self.nvars))

    # ------------------------------------------------------------------
    # a Monte-Carlo batch against an ensemble of wind profiles (include/gelato_amd.h gel_wind_ensemble_*)
    def wind_ensemble(self, tables):
        """tables: float64 [E, Kw, 3] (one member: [Kw, 3]), the columns of prob["wind_table"]; every member's altitudes increase
        strictly -> WindEnsemble (assign() it before a call takes it)"""
        t = np.asarray(tables)
        if t.dtype != np.float64:
            raise TypeError("tables: float64")
        if t.ndim == 2:
            t = t[None]
        if t.ndim != 3 or t.shape[2] != 3:
            raise ValueError("tables: [E, Kw, 3], not %s" % (t.shape,))
        t = np.ascontiguousarray(t)
        h = C.c_void_p()
        check(lib().gel_wind_ensemble_create(self._h, int(t.shape[0]), int(t.shape[1]), _d(t), C.byref(h)))
        return WindEnsemble(self._owner, h, t.shape[0], t.shape[1])

    # ------------------------------------------------------------------
    # Jacobian products from the compact values (include/gelato_amd.h gel_jac_*)
    def _jac_product(self, fn, jvar, inp, nin, nout):
        jvar, inp = _f64(jvar), _f64(inp)
        lead = inp.shape[:-1]
        if jvar.shape[-1] != self.V or inp.shape[-1] != nin or jvar.shape[:-1] != lead:
            raise ValueError("jvar [..., %d] and the input [..., %d] must share their leading shape" % (self.V, nin))
        B = int(np.prod(lead, dtype=np.int64)) if lead else 1
        out = np.empty(lead + (nout,))
        rc = check(fn(self._h, B, _d(jvar), _d(inp), _d(out)))
        return out, rc

    def jac_matvec(self, jvar, V):
        """jvar [..., V], V [..., nvars] -> (y [..., 11N] = J v per vector, status)"""
        return self._jac_product(lib().gel_jac_matvec, jvar, V, self.nvars, self.nres)

    def jac_rmatvec(self, jvar, Lam):
        """jvar [..., V], Lam [..., 11N] -> (g [..., nvars] = J^T lambda per vector, status)"""
        return self._jac_product(lib().gel_jac_rmatvec, jvar, Lam, self.nres, self.nvars)

    def jac_matvec_device(self, B, d_jvar, d_v, d_y, stream=0):
        """device buffers: d_jvar [B][V], d_v [B][nvars] -> d_y [B][11N]; status through sync()"""
        check(lib().gel_jac_matvec_device(self._h, int(B), d_jvar, d_v, d_y, stream or None))

    def jac_rmatvec_device(self, B, d_jvar, d_lam, d_g, stream=0):
        """device buffers: d_jvar [B][V], d_lam [B][11N] -> d_g [B][nvars]; status through sync()"""
        check(lib().gel_jac_rmatvec_device(self._h, int(B), d_jvar, d_lam, d_g, stream or None))

    def jac_products_host(self, jvar, inp, transpose=False):
        """the same products in plain C++ on the host, from the same tables (works on host-only handles) -> (out, status)"""
        t = int(bool(transpose))
        return self._jac_product(lambda h, B, a, b, c: lib().gel_jac_products_host(h, B, a, b, c, t), jvar, inp,
                                 self.nres if t else self.nvars, self.nvars if t else self.nres)

    def jac_products_info(self):
        """{"const_nnz", "var_entries", "max_row_nnz", "max_col_nnz"} of the operator tables, and what a product launch will use
        NOW (GEL_JPROD_VB is read per call): "vb" / "threads" of J v, "vb_t" / "threads_t" of J^T lambda"""
        info = (C.c_int64 * 4)()
        check(lib().gel_jac_products_info(self._h, info))
        out = dict(zip(("const_nnz", "var_entries", "max_row_nnz", "max_col_nnz"), (int(v) for v in info)))
        li = (C.c_int32 * 4)()
        check(lib().gel_jac_products_launch_info(self._h, li))
        out.update(zip(("vb", "threads", "vb_t", "threads_t"), (int(v) for v in li)))
        return out

    def jac_operator(self, jvar_row):
        """scipy.sparse.linalg.LinearOperator of shape (11N, nvars) for ONE vector's compact values; matvec / rmatvec run on the
        device (scipy is imported here, not with the package)"""
        from scipy.sparse.linalg import LinearOperator
        jv = _f64(jvar_row).reshape(self.V).copy()

        def mv(v):
            return self.jac_matvec(jv, np.asarray(v, dtype=np.float64).reshape(self.nvars))[0]

        def rmv(lam):
            return self.jac_rmatvec(jv, np.asarray(lam, dtype=np.float64).reshape(self.nres))[0]

        return LinearOperator((self.nres, self.nvars), matvec=mv, rmatvec=rmv, dtype=np.float64)

    # ------------------------------------------------------------------
    # products with K, the Jacobian of every row that is not a defect row (include/gelato_amd.h gel_con_*)
    CON_DIMS = ("R", "nlin", "nfn", "alpha", "q", "qalpha", "entries", "max_row_entries", "max_col_entries")

    def con_products_dims(self):
        """{"R", "nlin", "nfn", "alpha", "q", "qalpha" (rows), "entries", "max_row_entries", "max_col_entries"} of the operator
        the handle holds NOW (rebuilt by every rows_configure / aero_configure; works on host-only handles)"""
        info = (C.c_int64 * 9)()
        check(lib().gel_con_products_dims(self._h, info))
        return dict(zip(self.CON_DIMS, (int(v) for v in info)))

    def _con_product(self, fn, jfn, aero_jac, aero_record, inp, transpose, out=None):
        """host arrays with a leading batch shape: jfn [..., nfn, 7] | None, aero_jac {kind: [..., sum nnz]} | None,
        aero_record [..., width] | None, inp [..., num_vars] (or [..., R] transposed) -> (out, status)"""
        d = self.con_products_dims()
        nin, nout = (d["R"], self.nvars) if transpose else (self.nvars, d["R"])
        inp = _f64(inp)
        if inp.ndim < 1 or inp.shape[-1] != nin:
            raise ValueError("the input must be [..., %d]" % nin)
        lead = inp.shape[:-1]
        B = int(np.prod(lead, dtype=np.int64)) if lead else 1
        keep = []

        def arr(a, tail, what):
            a = _f64(a)
            if a.shape != lead + tail:
                raise ValueError("%s must be %r" % (what, lead + tail))
            keep.append(a)
            return _d(a)
        jp = arr(jfn, (d["nfn"], 7), "jfn") if jfn is not None else None
        ap = None
        if aero_jac is not None:
            ap = (_dp * 3)()
            for i, kind in enumerate(self.AERO_KINDS):
                if aero_jac.get(kind) is not None:
                    ap[i] = arr(aero_jac[kind], (sum(self.aero_dims(kind)[1]),), "aero_jac[%r]" % kind)
        rp = None
        if aero_record is not None:
            rec = _f64(aero_record)
            if rec.shape[:-1] != lead:
                raise ValueError("aero_record must share the leading shape %r" % (lead,))
            keep.append(rec)
            rp = _d(rec)
        if out is None:
            out = np.empty(lead + (nout,))
        elif out.shape != lead + (nout,) or out.dtype != np.float64 or not out.flags.c_contiguous:
            raise ValueError("out must be C-contiguous float64 of shape %r" % (lead + (nout,),))
        rc = check(fn(B, jp, ap, rp, _d(inp), _d(out)))
        return out, rc

    def con_matvec(self, V, jfn=None, aero_jac=None, aero_record=None):
        """V [..., nvars] -> (y [..., R] = K v per vector, status); the values as rows_eval / eval_aero_all return them (aero_jac
        {kind: array}) or as the records of eval_batch_aero_device (aero_record)"""
        L, h = lib(), self._h
        return self._con_product(lambda B, j, a, r, i, o: L.gel_con_matvec(h, B, j, a, r, i, o), jfn, aero_jac, aero_record, V, False)

    def con_rmatvec(self, Lam, jfn=None, aero_jac=None, aero_record=None, out=None):
        """Lam [..., R] -> (g [..., nvars] = K^T lambda per vector, status); out: an array to ACCUMULATE into, g = out + K^T lambda"""
        L, h, acc = lib(), self._h, int(out is not None)
        return self._con_product(lambda B, j, a, r, i, o: L.gel_con_rmatvec(h, B, j, a, r, i, o, acc), jfn, aero_jac, aero_record, Lam,
                                 True, out)

    def con_products_host(self, inp, jfn=None, aero_jac=None, aero_record=None, transpose=False, out=None):
        """the same products in plain C++ on the host, from the same tables in the same order (works on host-only handles) ->
        (out, status); out: an array to accumulate into"""
        L, h, t, acc = lib(), self._h, int(bool(transpose)), int(out is not None)
        return self._con_product(lambda B, j, a, r, i, o: L.gel_con_products_host(h, B, j, a, r, i, o, t, acc), jfn, aero_jac,
                                 aero_record, inp, bool(transpose), out)

    def con_matvec_device(self, B, d_jfn, d_aero_jac, d_aero_record, d_v, d_y):
        """device pointers (ints; 0 = NULL): d_jfn [B][nfn][7], d_aero_jac = 3 entries per kind or None, d_aero_record [B][width] or
        0, d_v [B][nvars] -> d_y [B][R]; asynchronous on the engine's own stream; status through sync()"""
        jp = (C.c_void_p * 3)(*[q or None for q in d_aero_jac]) if d_aero_jac is not None else None
        check(lib().gel_con_matvec_device(self._h, int(B), d_jfn or None, jp, d_aero_record or None, d_v or None, d_y or None))

    def con_rmatvec_device(self, B, d_jfn, d_aero_jac, d_aero_record, d_lam, d_g, accumulate=False):
        """d_lam [B][R] -> d_g [B][nvars] (accumulate: g = g + K^T lambda); asynchronous on the engine's own stream"""
        jp = (C.c_void_p * 3)(*[q or None for q in d_aero_jac]) if d_aero_jac is not None else None
        check(lib().gel_con_rmatvec_device(self._h, int(B), d_jfn or None, jp, d_aero_record or None, d_lam or None, d_g or None,
                                           int(bool(accumulate))))

    def merit_gradient(self, X):
        """X [B, nvars] (or [nvars]) -> (phi [B] = 1/2 ||res||^2, g [B, nvars] = J^T res, status): one eval_batch, one product"""
        X = _f64(X).reshape(-1, self.nvars)
        res, jv, rc = self.eval_batch(X)
        g, rc2 = self.jac_rmatvec(jv, res)
        return 0.5 * np.einsum("bi,bi->b", res, res), g, max(rc, rc2)

    # ------------------------------------------------------------------
    def split_x(self, x):
        M, N, S = self.M, self.N, self.S
        o = np.cumsum([0, M, 3 * M, 3 * M, 4 * M, 2 * N, S + 1])
        return {k: x[o[i]:o[i + 1]] for i, k in enumerate(XKEYS)}

    def split_res(self, res):
        N = self.N
        return {"mass": res[..., :N], "pos": res[..., N:4 * N], "vel": res[..., 4 * N:7 * N], "quat": res[..., 7 * N:]}

    def jac_dicts(self, vals_full):
        """full values -> {group: {var: {"coo": [rows, cols, vals], "shape": ...}}} (reference layout,
        lib/con_dynamics.py:75-76,108-113)."""
        pat = self.pattern()
        out = {g: {} for g in GROUPS}
        for b, (g, var) in enumerate(BLOCKS):
            r, c = pat[b]
            v = vals_full[self.block_off[b]:self.block_off[b + 1]]
            out[g][var] = {"coo": [r, c, v], "shape": self.block_shape[b]}
        return out

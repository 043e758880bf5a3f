#!/usr/bin/env python3
"""Cost of a Monte-Carlo batch against a wind ensemble (gel_propagate_ensemble_device, gel_output_table_batch_ensemble_device;
DESIGN.md 3.19), in ONE process on the SAME device buffers (as tools/propagate_bench.py and tools/output_batch_bench.py): for
mixed-6x64 and stress-12x128 at B = 65536, from device events after a warm-up, the median of three turns, turns alternating:
    flight   k = 1 and 4, section and chain mode, under per-(vector, phase) factors:
             disp          gel_propagate_dispersed_device: the handle's own table in LDS (what there was before)
             ens-own       every vector assigned -1: the same table through global memory and the kept interval
             ens-blocked   E members of Kw rows, propagate.assign_members(order="blocked"): a workgroup's lanes on one or two tables
             ens-cyclic    the same members, order="cyclic": every wavefront on all E tables
    table    34 and 5 columns, table + envelope + peaks, under the same factors: disp, ens-blocked, ens-cyclic
    tangent  mixed-6x64, chain, k = 1, P = 16 shared seeds (the first columns of propagate.jacobian_seeds), under the same factors
             (gel_propagate_tangent_ensemble_device): disp = the call without an ensemble, ens-own, ens-blocked,
             ens-cyclic
    adjoint  the same with Q = 11 shared terminal functionals (gel_propagate_adjoint_ensemble_device)
ENS_BENCH_LEGS (flight,table,tangent,adjoint) and ENS_BENCH_WORKLOADS (mixed-6x64,stress-12x128) select.
ENS_BENCH_PARENT=path/to/libgelato_amd.so adds "disp@parent": the dispersed call of ANOTHER build of the library (the parent
commit's), loaded beside this one into the same process through the symbols both have, on the same buffers in the same turns.
Prints one JSON line.
GPU box:  python3 tools/ensemble_bench.py [B (65536)] [turns (3)] [E (30)] [Kw (33)]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIVE = ["altitude", "dynamic_pressure", "Q_alpha", "M", "vel_air"]


def timed(fn, reps=1):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3 / reps


def wind_members(E, Kw, seed=100):
    """[E, Kw, 3]: altitudes from 300 m to 95 km with spacings from metres to kilometres, a smooth profile plus seeded noise"""
    import numpy as np
    out = []
    for e in range(E):
        rng = np.random.default_rng(seed + e)
        gaps = 10.0 ** rng.uniform(0.5, 3.7, Kw - 1)
        h = 300.0 + np.concatenate([[0.0], np.cumsum(gaps)]) * (94700.0 / gaps.sum())
        out.append(np.column_stack([h, 30.0 * np.sin(h / 9000.0) + 8.0 * rng.standard_normal(Kw),
                                    -20.0 * np.cos(h / 14000.0) + 6.0 * rng.standard_normal(Kw)]))
    return np.ascontiguousarray(np.stack(out))


class Parent:
    """another build of the library beside the loaded one: a handle, chain / section plans and the two dispersed device calls"""

    def __init__(self, path, eng_desc):
        from gelato_amd import _lib
        self.L = C.CDLL(path)
        for name in ("gel_problem_create", "gel_problem_destroy", "gel_prop_plan_create", "gel_prop_plan_destroy",
                     "gel_propagate_dispersed_device", "gel_output_table_batch_device", "gel_sync"):
            fn = getattr(self.L, name)
            fn.restype, fn.argtypes = _lib.SIGNATURES[name]
        self.h = C.c_void_p()
        assert self.L.gel_problem_create(C.byref(eng_desc), C.byref(self.h)) == 0

    def plan(self, steps, flags):
        import numpy as np
        p = C.c_void_p()
        st = np.ascontiguousarray(steps, dtype=np.int32)
        assert self.L.gel_prop_plan_create(self.h, st.ctypes.data_as(C.POINTER(C.c_int32)), flags, C.byref(p)) == 0
        return p


def main():
    import numpy as np
    import torch
    from gelato_amd import Engine, _lib, con_dynamics, pack_x, problem, propagate
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    turns = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    nE = int(sys.argv[3]) if len(sys.argv) > 3 else 30
    Kw = int(sys.argv[4]) if len(sys.argv) > 4 else 33
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_bench: no GPU visible")
    parent_path = os.environ.get("ENS_BENCH_PARENT")
    legs = os.environ.get("ENS_BENCH_LEGS", "flight,table,tangent,adjoint").split(",")
    workloads = os.environ.get("ENS_BENCH_WORKLOADS", "mixed-6x64,stress-12x128").split(",")
    out = {"B": B, "turns": turns, "E": nE, "Kw": Kw, "cases": [], "build": _lib.build_info(), "parent": parent_path}
    T = wind_members(nE, Kw)
    for wl in workloads:
        pd, ud, _, xd = problem.make_problem(wl)
        prob = con_dynamics.problem_arrays(pd, ud)
        ps, S, lc = pd["ps_params"], pd["num_sections"], pd["LaunchCondition"]
        E = Engine(prob, D=[ps.D(i) for i in range(S)], tau=[ps.tau(i) for i in range(S)])
        x = pack_x(xd)
        M = E.M
        X = np.tile(problem.synthetic_batch(x, M, 64), (B // 64 + 1, 1))[:B]
        dX = torch.from_numpy(X).cuda()
        dD = torch.from_numpy(propagate.sample_dispersion(B, S, 0.02, seed=1, per="phase")).cuda()
        dY = torch.empty((B, 11 * M), dtype=torch.float64, device="cuda")
        de = torch.empty((B, S, 4), dtype=torch.float64, device="cuda")
        ens = {"ens-own": E.wind_ensemble(T).assign(np.full(B, -1)),
               "ens-blocked": E.wind_ensemble(T).assign(propagate.assign_members(B, nE, "blocked")),
               "ens-cyclic": E.wind_ensemble(T).assign(propagate.assign_members(B, nE, "cyclic"))}
        par = _parent_of(parent_path, prob, ps, S) if parent_path else None

        def run(calls, rec):
            per = {name: [] for name in calls}
            for fn in calls.values():
                fn()
            torch.cuda.synchronize()
            assert E.sync() == 0
            for t in range(turns):
                for name in (list(calls) if t % 2 == 0 else list(calls)[::-1]):
                    per[name].append(timed(calls[name]))
            assert E.sync() == 0
            med = {name: float(np.median(v)) for name, v in per.items()}
            rec.update({"call_s": med, "call_s_all": per, "over_disp": {name: med[name] / med["disp"] for name in med}})
            out["cases"].append(rec)
            print({k: v for k, v in rec.items() if k != "call_s_all"}, file=sys.stderr, flush=True)   # progress

        for k in (1, 4) if "flight" in legs else ():
            for mode in ("section", "chain"):
                plan = E.propagation_plan(steps=k, restart=mode)
                calls = {"disp": lambda: plan.apply_device(B, dX.data_ptr(), dY.data_ptr(), de.data_ptr(), dD.data_ptr())}
                for name, en in ens.items():
                    calls[name] = (lambda en: lambda: plan.apply_device(B, dX.data_ptr(), dY.data_ptr(), de.data_ptr(), dD.data_ptr(), ensemble=en))(en)
                pplan = None
                if par:
                    pplan = par.plan(np.full(S, k), _lib.GEL_PROP_CHAIN if mode == "chain" else 0)
                    calls["disp@parent"] = lambda: par.L.gel_propagate_dispersed_device(pplan, B, dX.data_ptr(), dD.data_ptr(), dY.data_ptr(), de.data_ptr())
                run(calls, {"workload": wl, "what": "flight", "k": k, "mode": mode, "steps_per_vector": k * E.N})
                if par:
                    assert par.L.gel_sync(par.h, None) == 0
                    par.L.gel_prop_plan_destroy(pplan)
                plan.close()
        tab = "table" in legs
        dO = torch.empty((B if tab else 0, M, 34), dtype=torch.float64, device="cuda")
        dV = torch.empty((M, 34, 8), dtype=torch.float64, device="cuda")
        dP = torch.empty((B if tab else 0, 34, 4), dtype=torch.float64, device="cuda")
        for cols in (None, FIVE) if "table" in legs else ():
            def table(en):
                return lambda: E.output_table_batch_device(B, dX.data_ptr(), lc["lat"], lc["lon"], d_dispersion=dD.data_ptr(), columns=cols,
                                                           d_out=dO.data_ptr(), d_env=dV.data_ptr(), d_peaks=dP.data_ptr(), ensemble=en)
            calls = {"disp": table(None), "ens-blocked": table(ens["ens-blocked"]), "ens-cyclic": table(ens["ens-cyclic"])}
            if par:
                ids = None if cols is None else np.asarray([Engine.OUTPUT_COLUMNS.index(c) for c in cols], dtype=np.int32)
                calls["disp@parent"] = (lambda ids: lambda: par.L.gel_output_table_batch_device(
                    par.h, B, dX.data_ptr(), None, dD.data_ptr(), float(lc["lat"]), float(lc["lon"]), 34 if ids is None else len(ids),
                    None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int32)), dO.data_ptr(), dV.data_ptr(), dP.data_ptr()))(ids)
            run(calls, {"workload": wl, "what": "table", "ncols": 34 if cols is None else len(cols), "M": M})
            if par:
                assert par.L.gel_sync(par.h, None) == 0
        del dO, dV, dP
        torch.cuda.empty_cache()
        # the derivative calls under the ensemble against the same calls without one: shared seeds / functionals
        if wl == "mixed-6x64" and ("tangent" in legs or "adjoint" in legs):
            P, Q, nv = 16, 11, E.nvars
            _cols, sX, sD = propagate.jacobian_seeds(E.num_nodes, prob["attitude_hold"])
            last = M - 1
            idx = [last] + [M + 3 * last + c for c in range(3)] + [4 * M + 3 * last + c for c in range(3)] + [7 * M + 4 * last + c for c in range(4)]
            lam = np.zeros((Q, 11 * M))
            lam[np.arange(Q), idx] = 1.0
            tX, tD, tL = torch.from_numpy(sX[:P].copy()).cuda(), torch.from_numpy(sD[:P].copy()).cuda(), torch.from_numpy(lam).cuda()
            plan = E.propagation_plan(steps=1, restart="chain")
            if "tangent" in legs:
                ddY = torch.empty((B, P, 11 * M), dtype=torch.float64, device="cuda")

                def tangent(en):
                    return lambda: plan.tangent_device(B, P, dX.data_ptr(), dY.data_ptr(), ddY.data_ptr(), d_dx=tX.data_ptr(),
                                                       d_dispersion=dD.data_ptr(), d_ddispersion=tD.data_ptr(), shared=True, ensemble=en)
                calls = {"disp": tangent(None)}
                calls.update({name: tangent(en) for name, en in ens.items()})
                run(calls, {"workload": wl, "what": "tangent", "k": 1, "mode": "chain", "P": P, "info": plan.tangent_info(B, P, True)})
                del ddY
                torch.cuda.empty_cache()
            if "adjoint" in legs:
                gX = torch.empty((B, Q, nv), dtype=torch.float64, device="cuda")
                gD = torch.empty((B, Q, S, 4), dtype=torch.float64, device="cuda")

                def adjoint(en):
                    return lambda: plan.adjoint_device(B, Q, dX.data_ptr(), tL.data_ptr(), dY.data_ptr(), gX.data_ptr(), d_gdisp=gD.data_ptr(),
                                                       d_dispersion=dD.data_ptr(), shared=True, ensemble=en)
                calls = {"disp": adjoint(None)}
                calls.update({name: adjoint(en) for name, en in ens.items()})
                run(calls, {"workload": wl, "what": "adjoint", "k": 1, "mode": "chain", "Q": Q, "info": plan.adjoint_info(B, Q, True)})
                del gX, gD
            plan.close()
            del tX, tD, tL
        for en in ens.values():
            en.close()
        if par:
            par.L.gel_problem_destroy(par.h)
        del dX, dD, dY, de
        torch.cuda.empty_cache()
        E.close()
    print(json.dumps(out))


def _parent_of(path, prob, ps, S):
    """the problem once more, on the other build: the descriptor Engine.__init__ fills, restated"""
    import numpy as np
    from gelato_amd._lib import GelProblemDesc
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    keep = []

    def arr(a, dt):
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a.ctypes.data_as(dp if dt == np.float64 else ip)
    d = GelProblemDesc()
    d.num_sections = S
    d.num_nodes = arr(prob["num_nodes"], np.int32)
    d.thrust, d.massflow = arr(prob["thrust"], np.float64), arr(prob["massflow"], np.float64)
    d.reference_area, d.nozzle_area = arr(prob["reference_area"], np.float64), arr(prob["nozzle_area"], np.float64)
    d.engine_on, d.attitude_hold = arr(prob["engine_on"], np.int32), arr(prob["attitude_hold"], np.int32)
    d.unit_mass, d.unit_position, d.unit_velocity, d.unit_u, d.unit_t = [float(u) for u in prob["units"]]
    d.dx, d.barC20 = float(prob["dx"]), 0.0
    wind, ca = np.asarray(prob["wind_table"], dtype=np.float64), np.asarray(prob["ca_table"], dtype=np.float64)
    d.wind_rows, d.wind_table = wind.shape[0], arr(wind, np.float64)
    d.ca_rows, d.ca_table = ca.shape[0], arr(ca, np.float64)
    d.D = arr(np.concatenate([np.asarray(ps.D(i), dtype=np.float64).ravel() for i in range(S)]), np.float64)
    d.tau = arr(np.concatenate([np.asarray(ps.tau(i), dtype=np.float64).ravel() for i in range(S)]), np.float64)
    d.device, d.flags = 0, 0
    p = Parent(path, d)
    p.keep = keep
    return p


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of the wind-profile sensitivities (gel_propagate_tangent_wind_device, gel_propagate_adjoint_wind_device), in
ONE process on the SAME device buffers (as tools/ensemble_bench.py, whose helpers this uses): for mixed-6x64 and stress-12x128 at
B = 65536, chain mode, k = 1 and 4, from device events after a warm-up, the median of three turns, turns alternating:
    adjoint  Q = 11 shared terminal functionals, under per-(vector, phase) factors:
             own           gel_propagate_adjoint_device's kernels: the handle's table, no gwind
             own+gwind     the same with the wind rows' gradient [B][Q][Kw][2]
             ens           E members of Kw rows, blocked assignment, no gwind
             ens+gwind     the same with gwind [B][Q][max(Kw, handle's)][2]
    tangent  P = 16 shared seeds (the first columns of propagate.jacobian_seeds): own, own+dwind (a dense seed on the table's rows beside
             them), ens, ens+dwind
WIND_BENCH_LEGS (adjoint,tangent), WIND_BENCH_WORKLOADS (mixed-6x64,stress-12x128) and WIND_BENCH_K (1,4) select.
WIND_BENCH_PARENT=path/to/libgelato_amd.so adds "own@parent": gel_propagate_adjoint_device / gel_propagate_tangent_device of ANOTHER
build of the library (the parent commit's), loaded beside this one, on the same buffers in the same turns: the existing calls are
unmoved if it equals "own".
Prints one JSON line.
GPU box:  python3 tools/wind_gradient_bench.py [B (65536)] [turns (3)] [E (30)] [Kw (33)]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    import numpy as np
    import torch
    import ensemble_bench as eb
    from gelato_amd import Engine, _lib, con_dynamics, pack_x, problem, propagate
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    turns = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    nE = int(sys.argv[3]) if len(sys.argv) > 3 else 30
    Kw = int(sys.argv[4]) if len(sys.argv) > 4 else 33
    if not torch.cuda.is_available():
        raise SystemExit("wind_gradient_bench: no GPU visible")
    parent_path = os.environ.get("WIND_BENCH_PARENT")
    legs = os.environ.get("WIND_BENCH_LEGS", "adjoint,tangent").split(",")
    workloads = os.environ.get("WIND_BENCH_WORKLOADS", "mixed-6x64,stress-12x128").split(",")
    ks = [int(v) for v in os.environ.get("WIND_BENCH_K", "1,4").split(",")]
    out = {"B": B, "turns": turns, "E": nE, "Kw": Kw, "cases": [], "build": _lib.build_info(), "parent": parent_path}
    T = eb.wind_members(nE, Kw)
    for wl in workloads:
        pd, ud, _, xd = problem.make_problem(wl)
        prob = con_dynamics.problem_arrays(pd, ud)
        ps, S = pd["ps_params"], pd["num_sections"]
        E = Engine(prob, D=[ps.D(i) for i in range(S)], tau=[ps.tau(i) for i in range(S)])
        M, nv = E.M, E.nvars
        X = np.tile(problem.synthetic_batch(pack_x(xd), M, 64), (B // 64 + 1, 1))[:B]
        dX = torch.from_numpy(X).cuda()
        dD = torch.from_numpy(propagate.sample_dispersion(B, S, 0.02, seed=1, per="phase")).cuda()
        dY = torch.empty((B, 11 * M), dtype=torch.float64, device="cuda")
        ens = E.wind_ensemble(T).assign(propagate.assign_members(B, nE, "blocked"))
        par = eb._parent_of(parent_path, prob, ps, S) if parent_path else None
        if par:
            for name in ("gel_propagate_tangent_device", "gel_propagate_adjoint_device"):
                fn = getattr(par.L, name)
                fn.restype, fn.argtypes = _lib.SIGNATURES[name]
        P, Q = 16, 11
        _cols, sX, sD = propagate.jacobian_seeds(E.num_nodes, prob["attitude_hold"])
        last = M - 1
        idx = [last] + [M + 3 * last + c for c in range(3)] + [4 * M + 3 * last + c for c in range(3)] + [7 * M + 4 * last + c for c in range(4)]
        lam = np.zeros((Q, 11 * M))
        lam[np.arange(Q), idx] = 1.0
        tX, tD, tL = torch.from_numpy(sX[:P].copy()).cuda(), torch.from_numpy(sD[:P].copy()).cuda(), torch.from_numpy(lam).cuda()

        def run(calls, rec):
            per = {name: [] for name in calls}
            for fn in calls.values():
                fn()
            torch.cuda.synchronize()
            assert E.sync() == 0
            for t in range(turns):
                for name in (list(calls) if t % 2 == 0 else list(calls)[::-1]):
                    per[name].append(eb.timed(calls[name]))
            assert E.sync() == 0
            if par:
                assert par.L.gel_sync(par.h, None) == 0
            med = {name: float(np.median(v)) for name, v in per.items()}
            rec.update({"call_s": med, "call_s_all": per, "over_own": {name: med[name] / med["own"] for name in med}})
            out["cases"].append(rec)
            print({k: v for k, v in rec.items() if k != "call_s_all"}, file=sys.stderr, flush=True)   # progress

        for k in ks:
            plan = E.propagation_plan(steps=k, restart="chain")
            pplan = par.plan(np.full(S, k), _lib.GEL_PROP_CHAIN) if par else None
            Kown, Kens = plan.wind_rows(), plan.wind_rows(ens)
            if "adjoint" in legs:
                gX = torch.empty((B, Q, nv), dtype=torch.float64, device="cuda")
                gD = torch.empty((B, Q, S, 4), dtype=torch.float64, device="cuda")
                gW = torch.empty((B, Q, Kens, 2), dtype=torch.float64, device="cuda")

                def adjoint(en, wind):
                    return lambda: plan.adjoint_device(B, Q, dX.data_ptr(), tL.data_ptr(), dY.data_ptr(), gX.data_ptr(), d_gdisp=gD.data_ptr(),
                                                       d_dispersion=dD.data_ptr(), shared=True, ensemble=en, d_gwind=gW.data_ptr() if wind else 0)
                calls = {"own": adjoint(None, False), "own+gwind": adjoint(None, True), "ens": adjoint(ens, False), "ens+gwind": adjoint(ens, True)}
                if par:
                    calls["own@parent"] = lambda: par.L.gel_propagate_adjoint_device(pplan, B, Q, 1, dX.data_ptr(), dD.data_ptr(), tL.data_ptr(),
                                                                                     dY.data_ptr(), gX.data_ptr(), gD.data_ptr())
                run(calls, {"workload": wl, "what": "adjoint", "k": k, "Q": Q, "wind_rows": [Kown, Kens],
                            "info": plan.adjoint_info(B, Q, True), "info_gwind": plan.adjoint_info(B, Q, True, want_wind=True, ensemble=ens)})
                del gX, gD, gW
                torch.cuda.empty_cache()
            if "tangent" in legs:
                ddY = torch.empty((B, P, 11 * M), dtype=torch.float64, device="cuda")
                tW = torch.from_numpy(np.random.default_rng(3).standard_normal((P, Kens, 2))).cuda()
                tWo = tW[:, :Kown].contiguous()

                def tangent(en, wind):
                    w = (tW if en is not None else tWo).data_ptr() if wind else 0
                    return lambda: plan.tangent_device(B, P, dX.data_ptr(), dY.data_ptr(), ddY.data_ptr(), d_dx=tX.data_ptr(),
                                                       d_dispersion=dD.data_ptr(), d_ddispersion=tD.data_ptr(), shared=True, ensemble=en, d_dwind=w)
                calls = {"own": tangent(None, False), "own+dwind": tangent(None, True), "ens": tangent(ens, False), "ens+dwind": tangent(ens, True)}
                if par:
                    calls["own@parent"] = lambda: par.L.gel_propagate_tangent_device(pplan, B, P, 1, dX.data_ptr(), dD.data_ptr(), tX.data_ptr(),
                                                                                     tD.data_ptr(), dY.data_ptr(), ddY.data_ptr())
                run(calls, {"workload": wl, "what": "tangent", "k": k, "P": P, "wind_rows": [Kown, Kens], "info": plan.tangent_info(B, P, True)})
                del ddY, tW, tWo
                torch.cuda.empty_cache()
            if par:
                par.L.gel_prop_plan_destroy(pplan)
            plan.close()
        ens.close()
        if par:
            par.L.gel_problem_destroy(par.h)
        del dX, dD, dY, tX, tD, tL
        torch.cuda.empty_cache()
        E.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of the tangent-linear propagation (gel_propagate_tangent_device), in ONE process on the SAME device buffers
(as tools/propagate_bench.py): for mixed-6x64 and stress-12x128, chain and section mode, k = 1 and 4 steps per node interval,
  B = 65536 (argv) with SHARED seeds and P = 1, 4, 16;   B = 1 with P = 1 and the full flight_jacobian (11 + 4 S + S + 1 columns),
next to gel_propagate_dispersed_device on the same x and factors, turns alternating -- ns per (vector . direction), the ratio to
the value-only call of the same mode, and the slab count -- from device events after a warm-up, median of `turns`.
Prints one JSON line.   GPU box:  python3 tools/flight_tangent_bench.py [B (65536)] [turns (3)]
TANGENT_BENCH_ONLY=workload,mode,k,B,P runs that one tangent call alone, a few times (for a kernel trace or a counter run);
TANGENT_BENCH_WORKLOADS / TANGENT_BENCH_MODES select; a configuration whose dy exceeds TANGENT_BENCH_MAX_GB (64) is skipped and listed."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3 / reps


def main():
    import numpy as np
    import torch
    from gelato_amd import Engine, _lib, con_dynamics, pack_x, problem, propagate
    Bbig = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    turns = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    if not torch.cuda.is_available():
        raise SystemExit("flight_tangent_bench: no GPU visible")
    only = os.environ.get("TANGENT_BENCH_ONLY")
    workloads = os.environ.get("TANGENT_BENCH_WORKLOADS", "mixed-6x64,stress-12x128").split(",")
    modes = os.environ.get("TANGENT_BENCH_MODES", "chain,section").split(",")
    out = {"B": Bbig, "turns": turns, "cases": [], "build": _lib.build_info()}
    for wl in workloads:
        if only and only.split(",")[0] != wl:
            continue
        pd, ud, _, xd = problem.make_problem(wl)
        prob = con_dynamics.problem_arrays(pd, ud)
        ps = pd["ps_params"]
        S = pd["num_sections"]
        E = Engine(prob, D=[ps.D(i) for i in range(S)], tau=[ps.tau(i) for i in range(S)])
        x = pack_x(xd)
        cols, sX, sD = propagate.jacobian_seeds(E.num_nodes, prob["attitude_hold"])
        full = len(cols)
        for B, Ps in ((1, (1, full)), (Bbig, (1, 4, 16))):
            X = np.tile(problem.synthetic_batch(x, E.M, 64), (B // 64 + 1, 1))[:B]
            dX = torch.from_numpy(X).cuda()
            dY = torch.empty((B, 11 * E.M), dtype=torch.float64, device="cuda")
            dD = torch.from_numpy(propagate.sample_dispersion(B, E.S, 0.02, seed=1, per="phase")).cuda()
            reps = 20 if B == 1 else 1
            for P in Ps:
                gb = B * P * 11 * E.M * 8 / 2.0 ** 30
                if gb > float(os.environ.get("TANGENT_BENCH_MAX_GB", "64")):
                    out["cases"].append({"workload": wl, "B": B, "P": P, "skipped": "dy alone is %.0f GB (TANGENT_BENCH_MAX_GB)" % gb})
                    continue
                # shared seeds: the first P columns of the full Jacobian's (P = 1: the lift-off mass)
                tX, tD = torch.from_numpy(sX[:P].copy()).cuda(), torch.from_numpy(sD[:P].copy()).cuda()
                ddY = torch.empty((B, P, 11 * E.M), dtype=torch.float64, device="cuda")
                for mode in modes:
                    for k in (1, 4):
                        if only and only.split(",")[1:] != [mode, str(k), str(B), str(P)]:
                            continue
                        plan = E.propagation_plan(steps=k, restart=mode)
                        calls = {"value": lambda: plan.apply_device(B, dX.data_ptr(), dY.data_ptr(), 0, dD.data_ptr()),
                                 "tangent": lambda: plan.tangent_device(B, P, dX.data_ptr(), dY.data_ptr(), ddY.data_ptr(), d_dx=tX.data_ptr(),
                                                                        d_dispersion=dD.data_ptr(), d_ddispersion=tD.data_ptr(), shared=True)}
                        if only:
                            calls = {"tangent": calls["tangent"]}
                        per = {name: [] for name in calls}
                        for fn in calls.values():
                            fn()
                        torch.cuda.synchronize()
                        assert E.sync() == 0
                        for t in range(turns):
                            for name in (list(calls) if t % 2 == 0 else list(calls)[::-1]):
                                per[name].append(timed(calls[name], reps))
                        assert E.sync() == 0
                        med = {name: float(np.median(v)) for name, v in per.items()}
                        rec = {"workload": wl, "B": B, "P": P, "k": k, "mode": mode, "info": plan.tangent_info(B, P, True),
                               "call_s": med, "ns_per_vector_direction": med["tangent"] / B / P * 1e9, "call_s_all": per}
                        if not only:
                            rec["ns_per_vector_value"] = med["value"] / B * 1e9
                            rec["tangent_over_value"] = med["tangent"] / med["value"]
                        out["cases"].append(rec)
                        plan.close()
                del tX, tD, ddY
            del dX, dY, dD
            torch.cuda.empty_cache()
        E.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

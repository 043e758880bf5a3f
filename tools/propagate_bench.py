#!/usr/bin/env python3
"""Cost of the explicit RK4 propagation (gel_propagate_device, gel_propagate_dispersed_device), in ONE process on the SAME device
buffers (as tools/mesh_error_bench.py): for mixed-6x64 and stress-12x128, k = 1 and 4 steps per node interval, section and node
restart, the chained flight ("chain") and the chain and the section mode under per-vector dispersions ("chain+disp",
"section+disp": factors 1 + 0.02 N(0, 1) per vector and phase; PROP_BENCH_MODES=section,node,... selects), at
B = 1 and B = 65536 -- ns per vector and ns per (vector . RK4 step) from device events after a warm-up, next to the
residual-only gel_eval_batch_device launch (the same right-hand side once per node: the expected ratio is about 4 k per
right-hand-side evaluation) and gel_mesh_error_device on the same x, turns alternating.  Prints one JSON line.
GPU box:  python3 tools/propagate_bench.py [B (65536)] [turns (3)]        (PROP_BENCH_ONLY=workload,k,restart,B runs that
one propagation launch alone, a few times: the command to put under a kernel trace or a counter run)"""
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
        raise SystemExit("propagate_bench: no GPU visible")
    only = os.environ.get("PROP_BENCH_ONLY")
    modes = os.environ.get("PROP_BENCH_MODES", "section,node,chain,chain+disp,section+disp").split(",")
    out = {"B": Bbig, "turns": turns, "cases": [], "build": _lib.build_info()}
    for wl in ("mixed-6x64", "stress-12x128"):
        if only and only.split(",")[0] != wl:
            continue
        pd, ud, _, xd = problem.make_problem(wl)
        prob = con_dynamics.problem_arrays(pd, ud)
        ps = pd["ps_params"]
        S = pd["num_sections"]
        E = Engine(prob, D=[ps.D(i) for i in range(S)], tau=[ps.tau(i) for i in range(S)])
        x = pack_x(xd)
        s = torch.cuda.current_stream().cuda_stream
        for B in (1, Bbig):
            X = np.tile(problem.synthetic_batch(x, E.M, 64), (B // 64 + 1, 1))[:B]
            dX = torch.from_numpy(X).cuda()
            r = torch.empty((B, E.nres), dtype=torch.float64, device="cuda")
            de = torch.empty((B, E.S, 4), dtype=torch.float64, device="cuda")
            dY = torch.empty((B, 11 * E.M), dtype=torch.float64, device="cuda")
            dD = torch.from_numpy(propagate.sample_dispersion(B, E.S, 0.02, seed=1, per="phase")).cuda()
            reps = 20 if B == 1 else 1
            base = {"residual_only": lambda: E.eval_batch_device(B, dX.data_ptr(), r.data_ptr(), 0, s),
                    "mesh_error": lambda: E.mesh_error_device(B, dX.data_ptr(), de.data_ptr(), 0, s)}
            for k in (1, 4):
                for restart in modes:
                    if only and only.split(",")[1:] != [str(k), restart, str(B)]:
                        continue
                    plan = E.propagation_plan(steps=k, restart=restart.split("+")[0])
                    disp = dD.data_ptr() if restart.endswith("+disp") else 0
                    calls = dict(base, propagate=lambda: plan.apply_device(B, dX.data_ptr(), dY.data_ptr(), de.data_ptr(), disp))
                    if only:
                        calls = {"propagate": calls["propagate"]}
                    per = {name: [] for name in calls}
                    for fn in calls.values():
                        fn()
                    torch.cuda.synchronize()
                    assert E.sync(s) == 0
                    for t in range(turns):
                        for name in (list(calls) if t % 2 == 0 else list(calls)[::-1]):
                            per[name].append(timed(calls[name], reps))
                    assert E.sync(s) == 0
                    med = {name: float(np.median(v)) for name, v in per.items()}
                    steps = k * E.N                       # RK4 steps per vector (either restart mode)
                    rec = {"workload": wl, "B": B, "k": k, "restart": restart, "info": plan.info(),
                           "ns_per_vector": {name: med[name] / B * 1e9 for name in med},
                           "ns_per_vector_step": med["propagate"] / B / steps * 1e9, "call_s_all": per}
                    if not only:
                        rec["propagate_over_residual_only"] = med["propagate"] / med["residual_only"]
                        rec["per_rhs_over_residual_only"] = med["propagate"] / med["residual_only"] / (4 * k)
                        rec["propagate_over_mesh_error"] = med["propagate"] / med["mesh_error"]
                    out["cases"].append(rec)
                    plan.close()
            del dX, r, de, dY, dD
            torch.cuda.empty_cache()
        E.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

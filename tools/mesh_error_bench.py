#!/usr/bin/env python3
"""Cost of the collocation error estimate (gel_mesh_error*), in ONE process on the SAME device buffers (as tools/exact_jac_bench.py):
us per Engine.mesh_error call at B = 1 (example, mixed-6x64); ns per vector of gel_mesh_error_device at B = 65536 (mixed-6x64,
stress-12x128) next to the residual-only gel_eval_batch_device on the same x, turns alternating; the fp64 operations the estimate
issues per vector, counted from the shapes.  Prints one JSON line.
GPU box:  python3 tools/mesh_error_bench.py [B (65536)] [turns (6)]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fp64_ops(E):
    """fp64 FMAs per vector of the matrix products (interpolation 11 (n+1) + control 2 n + integration 11 (n+1) per test point)
    -- the right-hand side's chain comes on top (about 1.3 k fp64 operations per aerodynamic point, 0.1 k NoAir)"""
    fma = 0
    for n in E.num_nodes:
        P = int(n) + 1
        fma += P * (11 * P + 2 * int(n) + 11 * P)
    return fma


def main():
    import numpy as np
    import torch
    from gelato_amd import Engine, _lib, con_dynamics, pack_x, problem
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    turns = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    if not torch.cuda.is_available():
        raise SystemExit("mesh_error_bench: no GPU visible")
    reps = max(1, int(os.environ.get("MESH_BENCH_REPS", "10")))
    out = {"B": B, "turns": turns, "reps": reps, "B1_us": {}, "device": {}, "build": _lib.build_info()}
    for wl in ("example", "mixed-6x64", "stress-12x128"):
        pd, ud, _, xd = problem.make_problem(wl)
        prob = con_dynamics.problem_arrays(pd, ud)
        ps = pd["ps_params"]
        S = pd["num_sections"]
        E = Engine(prob, D=[ps.D(i) for i in range(S)], tau=[ps.tau(i) for i in range(S)])
        x = pack_x(xd)
        if wl != "stress-12x128":
            for _ in range(20):
                E.mesh_error(x)
            t0 = time.perf_counter()
            for _ in range(300):
                E.mesh_error(x)
            out["B1_us"][wl] = (time.perf_counter() - t0) / 300 * 1e6
        if wl == "example":
            continue
        X = np.tile(problem.synthetic_batch(x, E.M, 64), (B // 64 + 1, 1))[:B]
        dX = torch.from_numpy(X).cuda()
        r = torch.empty((B, E.nres), dtype=torch.float64, device="cuda")
        de = torch.empty((B, E.S, 4), dtype=torch.float64, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        calls = {"mesh_error": lambda: E.mesh_error_device(B, dX.data_ptr(), de.data_ptr(), 0, s),
                 "residual_only": lambda: E.eval_batch_device(B, dX.data_ptr(), r.data_ptr(), 0, s)}
        per = {k: [] for k in calls}
        for k in calls:
            calls[k]()
            torch.cuda.synchronize()
        for t in range(turns):
            for k in (("mesh_error", "residual_only") if t % 2 == 0 else ("residual_only", "mesh_error")):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(reps):
                    calls[k]()
                b.record()
                torch.cuda.synchronize()
                per[k].append(a.elapsed_time(b) / 1e3 / reps)
                assert E.sync(s) == 0
        med = {k: float(np.median(v)) for k, v in per.items()}
        fma = fp64_ops(E)
        out["device"][wl] = {"ns_per_vector": {k: med[k] / B * 1e9 for k in med}, "call_s_all": per,
                             "mesh_over_residual_only": med["mesh_error"] / med["residual_only"],
                             "product_fma_per_vector": fma,
                             # MI355X vector fp64: 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz FMAs/s (78.6 TFLOP/s)
                             "product_fma_time_at_vector_peak_ns": fma / (256 * 64 * 2.4e9) * 1e9}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

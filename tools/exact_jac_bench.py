#!/usr/bin/env python3
"""Cost of the exact defect Jacobian (GEL_FLAG_EXACT_DEFECT_JAC) against the default forward-difference form, in ONE process on the
SAME device buffers (placement common to both, as tools/ab_inproc.py): steady-state evaluations/s with derivatives through
gel_eval_batch_device, turns of the two handles alternating; and Engine.eval / Engine.eval_callback latency at B = 1 (the
callback of an exact handle runs its defect part as the residual-only launch + the exact kernel).  Prints one JSON line.
GPU box:  python3 tools/exact_jac_bench.py [workload (mixed-6x64)] [B (65536)] [turns (6)]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import torch
    from gelato_amd import Engine, _lib, con_dynamics, pack_x, problem
    wl = sys.argv[1] if len(sys.argv) > 1 else "mixed-6x64"
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
    turns = int(sys.argv[3]) if len(sys.argv) > 3 else 6
    if not torch.cuda.is_available():
        raise SystemExit("exact_jac_bench: no GPU visible")
    pd, ud, _, xd = problem.make_problem(wl)
    prob = con_dynamics.problem_arrays(pd, ud)
    ps = pd["ps_params"]
    S = pd["num_sections"]
    D, tau = [ps.D(i) for i in range(S)], [ps.tau(i) for i in range(S)]
    E = {"fd": Engine(prob, D=D, tau=tau), "exact": Engine(prob, D=D, tau=tau, flags=_lib.GEL_FLAG_EXACT_DEFECT_JAC)}
    x = pack_x(xd)
    X = np.tile(problem.synthetic_batch(x, E["fd"].M, 64), (B // 64 + 1, 1))[:B]
    dX = torch.from_numpy(X).cuda()
    r = torch.empty((B, E["fd"].nres), dtype=torch.float64, device="cuda")
    j = torch.empty((B, E["fd"].V), dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    reps = max(1, int(os.environ.get("EXACT_BENCH_REPS", "10")))
    per = {k: [] for k in E}
    for k in E:   # warm-up: code objects loaded, first-touch of the buffers
        E[k].eval_batch_device(B, dX.data_ptr(), r.data_ptr(), j.data_ptr(), s)
        torch.cuda.synchronize()
    for t in range(turns):
        for k in (("fd", "exact") if t % 2 == 0 else ("exact", "fd")):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                E[k].eval_batch_device(B, dX.data_ptr(), r.data_ptr(), j.data_ptr(), s)
            b.record()
            torch.cuda.synchronize()
            per[k].append(a.elapsed_time(b) / 1e3 / reps)
            assert E[k].sync(s) == 0
    lat, cb = {}, {}
    for k in E:
        for name, call, dst in (("eval", lambda: E[k].eval(x), lat), ("callback", lambda: E[k].eval_callback(x, True), cb)):
            for _ in range(20):
                call()
            t0 = time.perf_counter()
            n1 = 200
            for _ in range(n1):
                call()
            dst[k] = (time.perf_counter() - t0) / n1 * 1e6
    med = {k: float(np.median(v)) for k, v in per.items()}
    out = {"workload": wl, "B": B, "turns": turns, "reps": reps,
           "evals_per_s": {k: B / med[k] for k in E}, "call_s_median": med, "call_s_all": per,
           "exact_over_fd_time": med["exact"] / med["fd"], "eval_B1_us": lat, "callback_B1_us": cb,
           "build": _lib.build_info()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

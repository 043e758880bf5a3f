#!/usr/bin/env python3
"""Cost of the exact aero gradients (GEL_FLAG_EXACT_AERO_JAC) against the default forward differences, in ONE process on the SAME
device buffers (tools/ab_inproc.py's method), turns of the handles alternating:
  gel_eval_aero_all_device with gradients, FD against exact (mixed-6x64, every aerodynamic phase but the last constrained by all
  three kinds);
  gel_eval_batch_aero_device, ns per vector: FD (the fused AERO launch) against flag 64 and flags 32 | 64;
  Engine.eval_callback at B = 1 with the aero kinds (the exact handle runs its aero part as the values-only launch + the exact kernel).
Prints one JSON line.
GPU box:  python3 tools/exact_aero_bench.py [workload (mixed-6x64)] [B (16384)] [turns (6)]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = ("alpha", "q", "qalpha")
LIMITS = {"alpha": 0.2, "q": 4.0e4, "qalpha": 5.0e3}


def main():
    import numpy as np
    import torch
    from gelato_amd import Engine, _lib, con_dynamics, pack_x, problem
    wl = sys.argv[1] if len(sys.argv) > 1 else "mixed-6x64"
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 16384
    turns = int(sys.argv[3]) if len(sys.argv) > 3 else 6
    if not torch.cuda.is_available():
        raise SystemExit("exact_aero_bench: no GPU visible")
    pd, ud, _, xd = problem.make_problem(wl)
    prob = con_dynamics.problem_arrays(pd, ud)
    ps = pd["ps_params"]
    S = pd["num_sections"]
    D, tau = [ps.D(i) for i in range(S)], [ps.tau(i) for i in range(S)]
    A, X32 = _lib.GEL_FLAG_EXACT_AERO_JAC, _lib.GEL_FLAG_EXACT_DEFECT_JAC
    E = {"fd": Engine(prob, D=D, tau=tau), "exact": Engine(prob, D=D, tau=tau, flags=A),
         "exact32+64": Engine(prob, D=D, tau=tau, flags=A | X32)}
    for e in E.values():
        for k in KINDS:
            e.aero_configure(k, np.array([(i, 1, LIMITS[k]) for i in range(S - 1) if prob["reference_area"][i] != 0.0]))
    x = pack_x(xd)
    e0 = E["fd"]
    X = np.tile(problem.synthetic_batch(x, e0.M, 64), (B // 64 + 1, 1))[:B]
    dX = torch.from_numpy(X).cuda()
    dc = {k: torch.empty((B, e0.aero_dims(k)[0]), dtype=torch.float64, device="cuda") for k in KINDS}
    dj = {k: torch.empty((B, sum(e0.aero_dims(k)[1])), dtype=torch.float64, device="cuda") for k in KINDS}
    w = e0.aero_record_layout()[0]
    r = torch.empty((B, e0.nres), dtype=torch.float64, device="cuda")
    j = torch.empty((B, e0.V), dtype=torch.float64, device="cuda")
    rec = torch.empty((B, w), dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    reps = max(1, int(os.environ.get("EXACT_BENCH_REPS", "10")))
    cp, jp = [dc[k].data_ptr() for k in KINDS], [dj[k].data_ptr() for k in KINDS]
    calls = {
        "aero_all_device": (("fd", "exact"), lambda e: e.eval_aero_all_device(B, dX.data_ptr(), cp, jp, s)),
        "batch_aero_device": (("fd", "exact", "exact32+64"),
                              lambda e: e.eval_batch_aero_device(B, dX.data_ptr(), r.data_ptr(), j.data_ptr(), rec.data_ptr(), s)),
    }
    out = {"workload": wl, "B": B, "turns": turns, "reps": reps}
    for what, (keys, call) in calls.items():
        per = {k: [] for k in keys}
        for k in keys:   # warm-up: code objects loaded, first-touch of the buffers
            call(E[k])
            torch.cuda.synchronize()
        for t in range(turns):
            order = keys if t % 2 == 0 else tuple(reversed(keys))
            for k in order:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(reps):
                    call(E[k])
                b.record()
                torch.cuda.synchronize()
                per[k].append(a.elapsed_time(b) / 1e3 / reps)
                assert E[k].sync(s) == 0
        med = {k: float(np.median(v)) for k, v in per.items()}
        out[what] = {"ns_per_vector_median": {k: med[k] / B * 1e9 for k in keys},
                     "ns_per_vector_all": {k: [v / B * 1e9 for v in per[k]] for k in keys},
                     "over_fd_time": {k: med[k] / med["fd"] for k in keys}}
    cb = {}
    for k in ("fd", "exact"):
        for _ in range(20):
            E[k].eval_callback(x, True)
        t0 = time.perf_counter()
        n1 = 200
        for _ in range(n1):
            E[k].eval_callback(x, True)
        cb[k] = (time.perf_counter() - t0) / n1 * 1e6
    out["callback_B1_us"] = cb
    out["build"] = _lib.build_info()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of the adjoint flight (gel_propagate_adjoint_device), in ONE process on the SAME device buffers (as
tools/flight_tangent_bench.py): for mixed-6x64 and stress-12x128, chain mode, k = 1 and 4 steps per node interval, B = 1 and
B = 65536 (argv), three calls on the same x and factors, turns alternating:
  gel_propagate_dispersed_device;   gel_propagate_tangent_device with SHARED seeds at P = 1 and P = 16;
  gel_propagate_adjoint_device with SHARED terminal functionals at Q = 1 and Q = 11
-- ms per call, ns per (vector . functional), the ratio to the value flight, and the break-even P: the number of tangent directions
one adjoint functional costs, (adjoint s / Q) / (tangent s / P) at P = 16, Q = 11 -- from device events after a warm-up, median
of `turns`.  Where the largest output of a workload would exceed ADJOINT_BENCH_MAX_GB (64), B is halved until it fits (recorded).
Prints one JSON line.   GPU box:  python3 tools/flight_adjoint_bench.py [B (65536)] [turns (3)]
ADJOINT_BENCH_WORKLOADS / ADJOINT_BENCH_KS select."""
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
        raise SystemExit("flight_adjoint_bench: no GPU visible")
    workloads = os.environ.get("ADJOINT_BENCH_WORKLOADS", "mixed-6x64,stress-12x128").split(",")
    ks = [int(v) for v in os.environ.get("ADJOINT_BENCH_KS", "1,4").split(",")]
    max_gb = float(os.environ.get("ADJOINT_BENCH_MAX_GB", "64"))
    out = {"B": Bbig, "turns": turns, "cases": [], "build": _lib.build_info()}
    for wl in workloads:
        pd, ud, _, xd = problem.make_problem(wl)
        prob = con_dynamics.problem_arrays(pd, ud)
        ps = pd["ps_params"]
        S = pd["num_sections"]
        E = Engine(prob, D=[ps.D(i) for i in range(S)], tau=[ps.tau(i) for i in range(S)])
        x = pack_x(xd)
        M, nv = E.M, E.nvars
        _cols, sX, sD = propagate.jacobian_seeds(E.num_nodes, prob["attitude_hold"])
        last = M - 1
        idx = [last] + [M + 3 * last + c for c in range(3)] + [4 * M + 3 * last + c for c in range(3)] + [7 * M + 4 * last + c for c in range(4)]
        lam = np.zeros((11, 11 * M))
        lam[np.arange(11), idx] = 1.0
        for B in (1, Bbig):
            while max(B * 16 * 11 * M, B * 11 * nv) * 8 / 2.0 ** 30 > max_gb:
                B //= 2
            X = np.tile(problem.synthetic_batch(x, M, 64), (B // 64 + 1, 1))[:B]
            dX = torch.from_numpy(X).cuda()
            dY = torch.empty((B, 11 * M), dtype=torch.float64, device="cuda")
            dD = torch.from_numpy(propagate.sample_dispersion(B, E.S, 0.02, seed=1, per="phase")).cuda()
            reps = 20 if B == 1 else 1
            Ps, Qs = (1, 16), (1, 11)
            tX = {P: torch.from_numpy(sX[:P].copy()).cuda() for P in Ps}
            tD = {P: torch.from_numpy(sD[:P].copy()).cuda() for P in Ps}
            tL = {Q: torch.from_numpy(lam[:Q].copy()).cuda() for Q in Qs}
            ddY = torch.empty((B, max(Ps), 11 * M), dtype=torch.float64, device="cuda")
            gX = torch.empty((B, max(Qs), nv), dtype=torch.float64, device="cuda")
            gD = torch.empty((B, max(Qs), E.S, 4), dtype=torch.float64, device="cuda")
            for k in ks:
                plan = E.propagation_plan(steps=k, restart="chain")
                calls = {"value": lambda: plan.apply_device(B, dX.data_ptr(), dY.data_ptr(), 0, dD.data_ptr())}
                for P in Ps:
                    calls["tangent_P%d" % P] = (lambda P=P: plan.tangent_device(B, P, dX.data_ptr(), dY.data_ptr(), ddY.data_ptr(), d_dx=tX[P].data_ptr(),
                                                                                 d_dispersion=dD.data_ptr(), d_ddispersion=tD[P].data_ptr(), shared=True))
                for Q in Qs:
                    calls["adjoint_Q%d" % Q] = (lambda Q=Q: plan.adjoint_device(B, Q, dX.data_ptr(), tL[Q].data_ptr(), dY.data_ptr(), gX.data_ptr(),
                                                                                 d_gdisp=gD.data_ptr(), d_dispersion=dD.data_ptr(), shared=True))
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
                rec = {"workload": wl, "B": B, "k": k, "mode": "chain", "call_ms": {n: v * 1e3 for n, v in med.items()},
                       "ns_per_vector_value": med["value"] / B * 1e9,
                       "ns_per_vector_direction": {P: med["tangent_P%d" % P] / B / P * 1e9 for P in Ps},
                       "ns_per_vector_functional": {Q: med["adjoint_Q%d" % Q] / B / Q * 1e9 for Q in Qs},
                       "over_value": {n: v / med["value"] for n, v in med.items() if n != "value"},
                       "break_even_P": (med["adjoint_Q11"] / 11) / (med["tangent_P16"] / 16),
                       "info": {Q: plan.adjoint_info(B, Q, True) for Q in Qs}, "call_s_all": per}
                out["cases"].append(rec)
                print("%s B=%d k=%d: %s" % (wl, B, k, {n: round(v, 3) for n, v in rec["call_ms"].items()}), file=sys.stderr, flush=True)
                plan.close()
            del dX, dY, dD, ddY, gX, gD, tX, tD, tL
            torch.cuda.empty_cache()
        E.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

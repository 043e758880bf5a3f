#!/usr/bin/env python3
"""Cost of the batched post-processing table (gel_output_table_batch_device), in ONE process on the SAME device
buffers (as tools/propagate_bench.py): for mixed-6x64 and stress-12x128 at B = 1 and B = 65536, from device events after a
warm-up, the median of three turns, in ns per (vector . node):
    table34    the table of all 34 columns                table5   altitude, dynamic_pressure, Q_alpha, M, vel_air
    envelope   the envelope alone (34 columns)            peaks    the peaks alone (34 columns)
    all        table + envelope + peaks                   all+disp the same under per-(vector, phase) factors
next to the bytes each form moves (its inputs once per pass over the rows, its outputs once, the table once more where the envelope
is read from it, the envelope's partials written and read) against 8 TB/s, and
next to a loop of gel_output_table calls over 64 vectors on the same build (host buffers, one synchronous call per vector, wall
clock): the only thing there was before.  Node times are formed on the device (tx = NULL).  Prints one JSON line.
GPU box:  python3 tools/output_batch_bench.py [B (65536)] [turns (3)]      (OUT_BENCH_ONLY=workload,form,B runs that one launch
alone, a few times: the command to put under a kernel trace or a counter run)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIVE = ["altitude", "dynamic_pressure", "Q_alpha", "M", "vel_air"]
HBM_BYTES_PER_S = 8.0e12


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
    from gelato_amd import Engine, _lib, con_dynamics, output_result, pack_x, problem, propagate
    Bbig = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    turns = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    if not torch.cuda.is_available():
        raise SystemExit("output_batch_bench: no GPU visible")
    only = os.environ.get("OUT_BENCH_ONLY")
    out = {"B": Bbig, "turns": turns, "cases": [], "build": _lib.build_info()}
    for wl in ("mixed-6x64", "stress-12x128"):
        if only and only.split(",")[0] != wl:
            continue
        pd, ud, _, xd = problem.make_problem(wl)
        prob = con_dynamics.problem_arrays(pd, ud)
        ps, S, lc = pd["ps_params"], pd["num_sections"], pd["LaunchCondition"]
        E = Engine(prob, D=[ps.D(i) for i in range(S)], tau=[ps.tau(i) for i in range(S)])
        x = pack_x(xd)
        M = E.M
        # the loop the parent commit offers: one synchronous host-buffer call per vector, 64 vectors
        X64 = problem.synthetic_batch(x, M, 64)
        TX64 = [output_result.node_times(E.split_x(v), ud, pd)[0] for v in X64]
        E.output_table(X64[0], TX64[0], lc["lat"], lc["lon"])
        loop = []
        for _ in range(turns):
            t0 = time.perf_counter()
            for v, tx in zip(X64, TX64):
                E.output_table(v, tx, lc["lat"], lc["lon"])
            loop.append((time.perf_counter() - t0) / 64)
        loop_ns_per_node = float(np.median(loop)) / M * 1e9
        for B in (1, Bbig):
            X = np.tile(X64, (B // 64 + 1, 1))[:B]
            dX = torch.from_numpy(X).cuda()
            dD = torch.from_numpy(propagate.sample_dispersion(B, S, 0.02, seed=1, per="phase")).cuda()
            dO = torch.empty((B, M, 34), dtype=torch.float64, device="cuda")
            dE = torch.empty((M, 34, 8), dtype=torch.float64, device="cuda")
            dP = torch.empty((B, 34, 4), dtype=torch.float64, device="cuda")
            reps = 20 if B == 1 else 1

            def call(columns=None, o=False, e=False, p=False, disp=False):
                return lambda: E.output_table_batch_device(B, dX.data_ptr(), lc["lat"], lc["lon"], d_dispersion=dD.data_ptr() if disp else 0,
                                                           columns=columns, d_out=dO.data_ptr() if o else 0, d_env=dE.data_ptr() if e else 0,
                                                           d_peaks=dP.data_ptr() if p else 0)
            forms = {"table34": (call(o=True), 34, 1, 0, 0), "table5": (call(FIVE, o=True), 5, 1, 0, 0),
                     "envelope": (call(e=True), 34, 0, 1, 0), "peaks": (call(p=True), 34, 0, 0, 1),
                     "all": (call(o=True, e=True, p=True), 34, 1, 1, 1), "all+disp": (call(o=True, e=True, p=True, disp=True), 34, 1, 1, 1)}
            if only:
                forms = {k: v for k, v in forms.items() if only.split(",")[1:] == [k, str(B)]}
            per = {name: [] for name in forms}
            for fn, *_ in forms.values():
                fn()
            torch.cuda.synchronize()
            assert E.sync() == 0
            for t in range(turns):
                for name in (list(forms) if t % 2 == 0 else list(forms)[::-1]):
                    per[name].append(timed(forms[name][0], reps))
            assert E.sync() == 0
            nblk = (B + 255) // 256
            for name, (_fn, nc, o, e, p) in forms.items():
                med = float(np.median(per[name]))
                # inputs once per kernel that forms rows (the table / peaks kernel; the envelope kernel of a call without a table),
                # outputs once, the table once more where the envelope is read from it, partials twice
                row_passes = max(o, p) + (e if not o else 0)
                nbytes = 8.0 * (row_passes * B * E.nvars + o * (1 + e) * B * M * nc + p * B * nc * 4 + e * (M * nc * 8 + 2 * nblk * M * nc * 8))
                out["cases"].append({"workload": wl, "B": B, "form": name, "M": M, "ncols": nc, "call_s": med, "call_s_all": per[name],
                                     "ns_per_vector_node": med / B / M * 1e9, "bytes": nbytes,
                                     "s_at_8TBps": nbytes / HBM_BYTES_PER_S, "share_of_8TBps": nbytes / HBM_BYTES_PER_S / med,
                                     "loop_of_gel_output_table_ns_per_vector_node": loop_ns_per_node})
            del dX, dD, dO, dE, dP
            torch.cuda.empty_cache()
        E.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

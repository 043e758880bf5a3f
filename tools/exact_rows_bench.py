#!/usr/bin/env python3
"""Cost of the exact row Jacobian (GEL_FLAG_EXACT_ROWS_JAC) against the default forward differences, in ONE process on the SAME
device buffers (tools/ab_inproc.py's method), turns of the handles alternating:
  gel_rows_eval_device with jfn, us per call, FD against exact, at B = 1, 1024, 65536, for two tables on the example problem:
    "terminal_user"  its terminal rows and the user example row (fn 5);
    "waypoint"       latitude / longitude / altitude, IIP latitude / longitude and downrange rows at every section's first node;
  Engine.eval_callback at B = 1 (rows, defect groups, Jacobian) with flags 0, 32 | 64 and 32 | 64 | 128.
Prints one JSON line.
GPU box:  python3 tools/exact_rows_bench.py [turns (6)]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def tables(pdict, unitdict, condition):
    from gelato_amd import con_init_terminal_knot as ck
    from gelato_amd.engine import Engine
    pd = dict(pdict, device=-1)
    pd.pop("_gelato_amd", None)
    ev, ps, S = pdict["event_index"], pdict["ps_params"], pdict["num_sections"]
    xa = [ps.index_start_x(i) for i in range(S)]
    term = [r for r in ck._Rows(pd, unitdict, condition).fn]
    term.append(("periapsis_radius", xa[ev["IIP_END"]], 6378137.0, 1.0))
    lc = pdict["LaunchCondition"]
    SH, RAW = Engine.MODE_SHIFTED, Engine.MODE_RAW_DIFFERENCE
    way = []
    for sec in range(S):
        way += [("latitude_deg", xa[sec], sec, SH | RAW, [90.0, 30.0]), ("longitude_deg", xa[sec], sec, SH | RAW, [180.0, 140.0]),
                ("altitude", xa[sec], sec, RAW, [1.0e5, 1.0]), ("lat_IIP_deg", xa[sec], sec, SH | RAW, [90.0, 30.0]),
                ("lon_IIP_deg", xa[sec], sec, SH | RAW, [180.0, 150.0]),
                ("downrange", xa[sec], sec, RAW, [1.0e6, 1.0, float(lc["lat"]), float(lc["lon"])])]
    return {"terminal_user": term, "waypoint": way}


def main():
    import numpy as np
    import torch
    from gelato_amd import Engine, _lib, con_dynamics, pack_x, problem
    turns = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    if not torch.cuda.is_available():
        raise SystemExit("exact_rows_bench: no GPU visible")
    pdict, unitdict, condition, xdict = problem.make_problem("example")
    prob = con_dynamics.problem_arrays(pdict, unitdict)
    ps, S = pdict["ps_params"], pdict["num_sections"]
    D, tau = [ps.D(i) for i in range(S)], [ps.tau(i) for i in range(S)]
    R128, X32, A64 = _lib.GEL_FLAG_EXACT_ROWS_JAC, _lib.GEL_FLAG_EXACT_DEFECT_JAC, _lib.GEL_FLAG_EXACT_AERO_JAC
    x = pack_x(xdict)
    reps = max(1, int(os.environ.get("EXACT_BENCH_REPS", "20")))
    s = torch.cuda.current_stream().cuda_stream
    out = {"turns": turns, "reps": reps, "rows_eval_device_us": {}}
    Bmax = 65536
    e0 = Engine(prob, D=D, tau=tau)
    X = np.tile(problem.synthetic_batch(x, e0.M, 64), (Bmax // 64 + 1, 1))[:Bmax]
    dX = torch.from_numpy(X).cuda()
    for tname, rows in tables(pdict, unitdict, condition).items():
        E = {"fd": Engine(prob, D=D, tau=tau), "exact": Engine(prob, D=D, tau=tau, flags=R128)}
        for e in E.values():
            e.rows_configure([], rows)
        R = len(rows)
        dc = torch.empty((Bmax, R), dtype=torch.float64, device="cuda")
        dj = torch.empty((Bmax, R, 7), dtype=torch.float64, device="cuda")
        res = {"rows": R}
        for B in (1, 1024, Bmax):
            per = {k: [] for k in E}
            for k in E:   # warm-up
                E[k].rows_eval_device(B, dX.data_ptr(), dc.data_ptr(), dj.data_ptr(), s)
                torch.cuda.synchronize()
            for t in range(turns):
                for k in (("fd", "exact") if t % 2 == 0 else ("exact", "fd")):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(reps):
                        E[k].rows_eval_device(B, dX.data_ptr(), dc.data_ptr(), dj.data_ptr(), s)
                    b.record()
                    torch.cuda.synchronize()
                    per[k].append(a.elapsed_time(b) * 1e3 / reps)
                    assert E[k].sync(s) == 0
            res["B%d" % B] = {k: float(np.median(v)) for k, v in per.items()}
        out["rows_eval_device_us"][tname] = res
    # the optimiser's callback at B = 1: every row of both tables, defect groups with their Jacobian
    allrows = [r for rows in tables(pdict, unitdict, condition).values() for r in rows]
    cb = {}
    handles = {"0": Engine(prob, D=D, tau=tau), "32|64": Engine(prob, D=D, tau=tau, flags=X32 | A64),
               "32|64|128": Engine(prob, D=D, tau=tau, flags=X32 | A64 | R128)}
    for e in handles.values():
        e.rows_configure([], allrows)
    per = {k: [] for k in handles}
    for k, e in handles.items():
        for _ in range(20):
            e.eval_callback(x, True)
    for t in range(turns):
        for k in (list(handles) if t % 2 == 0 else list(reversed(list(handles)))):
            t0 = time.perf_counter()
            n1 = 100
            for _ in range(n1):
                handles[k].eval_callback(x, True)
            per[k].append((time.perf_counter() - t0) / n1 * 1e6)
    out["callback_B1_us"] = {k: float(np.median(v)) for k, v in per.items()}
    out["build"] = _lib.build_info()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of the batched Jacobian products (gel_jac_matvec_device, gel_jac_rmatvec_device), in ONE process on the
SAME device buffers, device events, a warm-up launch and >= 20 timed launches each:
  ns per vector of each product at mixed-6x64 and stress-12x128 for B = 1024, 16384, 65536 (jvar of a real evaluation), next to
  (a) gel_eval_batch_device with derivatives (the launch that produced jvar) and, at B = 1024,
  (b) the only other route: gel_eval_full_device (evaluation + update of the full values in place) plus reading jfull once, taken
      as its bytes over the device copy rate measured on the same buffers;
  each product's share of the 8 TB/s roofline by the bytes it must move, 8 (V + num_vars + 11 N) per vector;
  the vectors-per-workgroup A/B (GEL_JPROD_VB = 8 / 4 / 2 / 1, how many vectors' FMAs one table element feeds) at B = 16384, and
  the lanes-per-workgroup A/B (a second handle created under GEL_JPROD_THREADS = 256; the default is 512) at B = 65536.
Prints one JSON line.
GPU box:  python3 tools/jac_products_bench.py [launches (20)] [workloads, comma separated]
          python3 tools/jac_products_bench.py --loop WORKLOAD B N     N launches of each product and nothing else (the program to
                                                                      put behind rocprofv3 --kernel-trace --stats, or --pmc alone)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8.0e12


def timed(torch, fn, n):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3 / n


def loop(wl, B, n):
    import numpy as np
    import torch
    from gelato_amd import Engine, con_dynamics, pack_x, problem
    pd, ud, _, xd = problem.make_problem(wl)
    E = Engine(con_dynamics.problem_arrays(pd, ud))
    dX = torch.from_numpy(np.tile(problem.synthetic_batch(pack_x(xd), E.M, 64), (B // 64, 1))).cuda()
    res = torch.empty((B, E.nres), dtype=torch.float64, device="cuda")
    jv = torch.empty((B, E.V), dtype=torch.float64, device="cuda")
    v = torch.randn((B, E.nvars), dtype=torch.float64, device="cuda")
    y, g = torch.empty_like(res), torch.empty_like(v)
    s = torch.cuda.current_stream().cuda_stream
    E.eval_batch_device(B, dX.data_ptr(), res.data_ptr(), jv.data_ptr(), s)
    for _ in range(n):
        E.jac_matvec_device(B, jv.data_ptr(), v.data_ptr(), y.data_ptr(), s)
        E.jac_rmatvec_device(B, jv.data_ptr(), res.data_ptr(), g.data_ptr(), s)
    assert E.sync(s) == 0


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--loop":
        return loop(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    import numpy as np
    import torch
    from gelato_amd import Engine, _lib, con_dynamics, pack_x, problem
    n = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 20
    wls = sys.argv[2].split(",") if len(sys.argv) > 2 else ["mixed-6x64", "stress-12x128"]
    if not torch.cuda.is_available():
        raise SystemExit("jac_products_bench: no GPU visible")
    out = {"launches": n, "build": _lib.build_info(), "workloads": {}}
    for wl in wls:
        pd, ud, _, xd = problem.make_problem(wl)
        prob = con_dynamics.problem_arrays(pd, ud)
        ps = pd["ps_params"]
        S = pd["num_sections"]
        E = Engine(prob, D=[ps.D(i) for i in range(S)], tau=[ps.tau(i) for i in range(S)])
        x = pack_x(xd)
        X64 = problem.synthetic_batch(x, E.M, 64)
        floor_bytes = 8 * (E.V + E.nvars + E.nres)
        rec = {"V": E.V, "num_vars": E.nvars, "rows": E.nres, "info": E.jac_products_info(), "floor_bytes_per_vector": floor_bytes,
               "floor_ns_per_vector": floor_bytes / HBM_BYTES_PER_S * 1e9, "B": {}}
        s = torch.cuda.current_stream().cuda_stream
        for B in (1024, 16384, 65536):
            dX = torch.from_numpy(np.tile(X64, (B // 64, 1))).cuda()
            res = torch.empty((B, E.nres), dtype=torch.float64, device="cuda")
            jv = torch.empty((B, E.V), dtype=torch.float64, device="cuda")
            v = torch.randn((B, E.nvars), dtype=torch.float64, device="cuda")
            y = torch.empty((B, E.nres), dtype=torch.float64, device="cuda")
            g = torch.empty((B, E.nvars), dtype=torch.float64, device="cuda")
            calls = {"eval_batch": lambda: E.eval_batch_device(B, dX.data_ptr(), res.data_ptr(), jv.data_ptr(), s),
                     "matvec": lambda: E.jac_matvec_device(B, jv.data_ptr(), v.data_ptr(), y.data_ptr(), s),
                     "rmatvec": lambda: E.jac_rmatvec_device(B, jv.data_ptr(), res.data_ptr(), g.data_ptr(), s)}
            r = {}
            for k, fn in calls.items():
                t = timed(torch, fn, n)
                assert E.sync(s) == 0
                r[k + "_ns_per_vector"] = t / B * 1e9
            for k in ("matvec", "rmatvec"):
                r[k + "_share_of_eval"] = r[k + "_ns_per_vector"] / r["eval_batch_ns_per_vector"]
                r[k + "_roofline_share"] = rec["floor_ns_per_vector"] / r[k + "_ns_per_vector"]
            if B == 16384:
                ab = {}
                for vb in (8, 4, 2, 1):
                    os.environ["GEL_JPROD_VB"] = str(vb)
                    ab[str(vb)] = {k: timed(torch, calls[k], n) / B * 1e9 for k in ("matvec", "rmatvec")}
                os.environ.pop("GEL_JPROD_VB")
                r["vectors_per_workgroup_ab_ns_per_vector"] = ab
            if B == 65536:
                os.environ["GEL_JPROD_THREADS"] = "256"
                E256 = Engine(prob, D=[ps.D(i) for i in range(S)], tau=[ps.tau(i) for i in range(S)])
                os.environ.pop("GEL_JPROD_THREADS")
                r["lanes_256_ns_per_vector"] = {
                    "matvec": timed(torch, lambda: E256.jac_matvec_device(B, jv.data_ptr(), v.data_ptr(), y.data_ptr(), s), n) / B * 1e9,
                    "rmatvec": timed(torch, lambda: E256.jac_rmatvec_device(B, jv.data_ptr(), res.data_ptr(), g.data_ptr(), s), n) / B * 1e9}
                assert E256.sync(s) == 0
                E256.close()
            if B == 1024:
                jf = torch.empty((B, E.total_nnz), dtype=torch.float64, device="cuda")
                jf2 = torch.empty_like(jf)
                E.fill_full_device(B, jf.data_ptr(), s)
                t_full = timed(torch, lambda: E.eval_full_device(B, dX.data_ptr(), res.data_ptr(), jv.data_ptr(), jf.data_ptr(), s), n)
                assert E.sync(s) == 0
                t_copy = timed(torch, lambda: jf2.copy_(jf), n)
                rate = 2 * jf.numel() * 8 / t_copy          # a copy reads and writes every byte
                r["eval_full_ns_per_vector"] = t_full / B * 1e9
                r["copy_rate_bytes_per_s"] = rate
                r["jfull_read_ns_per_vector"] = E.total_nnz * 8 / rate * 1e9
                r["full_route_ns_per_vector"] = r["eval_full_ns_per_vector"] + r["jfull_read_ns_per_vector"]
                del jf, jf2
            rec["B"][str(B)] = r
            del dX, res, jv, v, y, g
            torch.cuda.empty_cache()
        out["workloads"][wl] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()

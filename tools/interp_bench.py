#!/usr/bin/env python3
"""Cost of the spectral interpolation (gel_interp_resident), in ONE process on the SAME device buffers (as tools/mesh_error_bench.py):
ns per vector of a mesh transfer (mixed-6x64 -> +8 nodes per phase, stress-12x128 -> 12 x 136) and of table mode at 256 points per
phase (mixed-6x64), at B = 1, 1024 and 65536, next to a device-to-device copy that moves the same number of bytes, next to
gel_mesh_error_device on the same x, and as a share of the byte floor 8 (src num_vars + output doubles) per vector at 8 TB/s.
Device events around 20 launches after a warm-up.  Prints one JSON line.
GPU box:  python3 tools/interp_bench.py [B ...  (1 1024 65536)]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = 20
HBM_BYTES_PER_S = 8.0e12


def timed(torch, fn):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3 / REPS


def main():
    import numpy as np
    import torch
    from gelato_amd import Engine, _lib, con_dynamics, pack_x, problem
    Bs = [int(v) for v in sys.argv[1:]] or [1, 1024, 65536]
    if not torch.cuda.is_available():
        raise SystemExit("interp_bench: no GPU visible")
    out = {"reps": REPS, "cases": {}, "build": _lib.build_info()}
    for case, wl in (("transfer mixed-6x64 +8", "mixed-6x64"), ("transfer stress-12x128 -> 136", "stress-12x128"),
                     ("table mixed-6x64 256 points", "mixed-6x64")):
        pd, ud, _, xd = problem.make_problem(wl)
        prob = con_dynamics.problem_arrays(pd, ud)
        E = Engine(prob)
        if case.startswith("transfer"):
            dst = dict(prob)
            dst["num_nodes"] = np.array([int(n) + 8 for n in E.num_nodes], dtype=np.int32)
            Ed = Engine(dst, device=-1)
            plan = E.transfer_plan(Ed)
            Ed.close()
        else:
            plan = E.interp_plan([np.linspace(-1.0, 1.0, 256)] * E.S)
        info = plan.info()
        w = info["out_doubles"]
        X64 = torch.from_numpy(problem.synthetic_batch(pack_x(xd), E.M, 64)).cuda()
        rec = {"info": info, "floor_ns_per_vector": 8.0 * (E.nvars + w) / HBM_BYTES_PER_S * 1e9, "B": {}}
        for B in Bs:
            dX = X64.repeat(B // 64 + 1, 1)[:B].contiguous()
            dO = torch.empty((B, w), dtype=torch.float64, device="cuda")
            de = torch.empty((B, E.S, 4), dtype=torch.float64, device="cuda")
            half = (B * (E.nvars + w)) // 2           # a copy of `half` doubles reads and writes as many bytes as the interpolation
            src = torch.empty(half, dtype=torch.float64, device="cuda").zero_()
            dstv = dO.view(-1)[:half] if half <= dO.numel() else torch.empty(half, dtype=torch.float64, device="cuda")
            s = torch.cuda.current_stream().cuda_stream
            t_copy = timed(torch, lambda: dstv.copy_(src))
            t_mesh = timed(torch, lambda: E.mesh_error_device(B, dX.data_ptr(), de.data_ptr(), 0, s))
            assert E.sync(s) == 0
            t_int = timed(torch, lambda: plan.apply_resident(B, dX.data_ptr(), dO.data_ptr()))
            assert E.sync() == 0
            ns = {"interp": t_int / B * 1e9, "copy_same_bytes": t_copy / B * 1e9, "mesh_error": t_mesh / B * 1e9}
            rec["B"][str(B)] = {"ns_per_vector": ns, "interp_over_copy": t_int / t_copy, "interp_over_mesh_error": t_int / t_mesh,
                                "share_of_byte_floor": rec["floor_ns_per_vector"] / ns["interp"]}
            del dX, dO, de, src, dstv
            torch.cuda.empty_cache()
        out["cases"][case] = rec
        plan.close()
        E.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

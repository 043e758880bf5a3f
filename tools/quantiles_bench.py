#!/usr/bin/env python3
"""Cost of the exact batched quantiles (gel_batch_quantiles_device), in ONE process on the SAME device buffers (as
tools/output_batch_bench.py): for mixed-6x64 and stress-12x128 at B = 65536 and five probabilities, from device events after a
warm-up, the median of three turns, in ns per (vector . node):
    table34   the quantiles of the table of all 34 columns      table5   of altitude, dynamic_pressure, Q_alpha, M, vel_air
    peaks     of every flight's peaks (34 columns x 4, with who)
next to the time ONE read of the source would take at 8 TB/s, the passes over the source the call makes, how its (column, rank)
pairs were settled (range pass / candidate buffers / bisection over the column), and beside them on the same buffers
    copy      a device copy of the same bytes (one read and one write: above the floor of one pass)
    form      gel_output_table_batch_device forming that table (or those peaks)
    sort      torch.sort(dim=0) of the first rows of the same tensor, as many as keep it below 2 GiB (informational: a sort needs the
              whole tensor again for its values and once more, as int64, for its indices)
The batch is 64 synthetic vectors tiled to B and then scaled per entry by 1 + 1e-6 z on the device, so that no two flights are equal.
Prints one JSON line.   GPU box:  python3 tools/quantiles_bench.py [B (65536)] [turns (3)]      (QUANT_BENCH_ONLY=workload,case runs that
one case alone: the command to put under a kernel trace or a counter run)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIVE = ["altitude", "dynamic_pressure", "Q_alpha", "M", "vel_air"]
PROBS = [0.00135, 0.025, 0.5, 0.975, 0.99865]
HBM_BYTES_PER_S = 8.0e12
SORT_BYTES = 2 << 30


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3


def main():
    import numpy as np
    import torch
    from gelato_amd import Engine, _lib, con_dynamics, pack_x, problem, propagate
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    turns = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    if not torch.cuda.is_available():
        raise SystemExit("quantiles_bench: no GPU visible")
    out = {"B": B, "turns": turns, "probs": PROBS, "cases": [], "build": _lib.build_info()}
    nq = len(PROBS)
    only = os.environ.get("QUANT_BENCH_ONLY")
    for wl in ("mixed-6x64", "stress-12x128"):
        if only and only.split(",")[0] != wl:
            continue
        pd, ud, _, xd = problem.make_problem(wl)
        ps, S, lc = pd["ps_params"], pd["num_sections"], pd["LaunchCondition"]
        E = Engine(con_dynamics.problem_arrays(pd, ud), D=[ps.D(i) for i in range(S)], tau=[ps.tau(i) for i in range(S)])
        M = E.M
        X64 = problem.synthetic_batch(pack_x(xd), M, 64)
        dX = torch.from_numpy(np.tile(X64, (B // 64 + 1, 1))[:B]).cuda()
        z = torch.randn(dX.shape, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))
        z[:, M:4 * M].abs_()                                        # positions outward only, as synthetic_batch
        z[:, 11 * M:] = 0.0                                         # controls and knot times as they are
        dX *= 1.0 + 1e-6 * z
        del z
        dD = torch.from_numpy(propagate.sample_dispersion(B, S, 0.02, seed=1, per="phase")).cuda()
        for name, cols, nc in (("table34", None, 34), ("table5", FIVE, 5), ("peaks", None, 34)):
            if only and only.split(",")[1:] != [name]:
                continue
            peaks = name == "peaks"
            W = 4 * nc if peaks else M * nc
            src = torch.empty((B, W), dtype=torch.float64, device="cuda")
            dst = torch.empty_like(src)
            dq = torch.empty((W, nq, 2), dtype=torch.float64, device="cuda")
            dc = torch.empty((W,), dtype=torch.float64, device="cuda")
            dw = torch.empty((W, nq, 2), dtype=torch.float64, device="cuda")

            def form():
                E.output_table_batch_device(B, dX.data_ptr(), lc["lat"], lc["lon"], d_dispersion=dD.data_ptr(), columns=cols,
                                            d_out=0 if peaks else src.data_ptr(), d_peaks=src.data_ptr() if peaks else 0)

            def quant():
                E.batch_quantiles_device(B, W, W, src.data_ptr(), PROBS, dq.data_ptr(), dc.data_ptr(), dw.data_ptr() if peaks else 0)

            def copy():
                dst.copy_(src)
            nsort = max(1, min(B, SORT_BYTES // (8 * W)))

            def sort():
                torch.sort(src[:nsort], dim=0)
            fns = {"form": form, "quantiles": quant, "copy": copy, "sort": sort}
            for fn in fns.values():
                fn()
            assert E.sync() == 0
            torch.cuda.synchronize()
            per = {k: [] for k in fns}
            for t in range(turns):
                for k in (list(fns) if t % 2 == 0 else list(fns)[::-1]):
                    per[k].append(timed(fns[k]))
            quant()
            how = E.batch_quantiles_last()
            info = E.batch_quantiles_info(B, W, nq)
            med = {k: float(np.median(v)) for k, v in per.items()}
            nodes = 1 if peaks else M
            out["cases"].append({
                "workload": wl, "case": name, "B": B, "M": M, "W": W, "source_bytes": 8.0 * B * W, "info": info, "settled": how,
                "share_fallback": how["by_fallback"] / max(1, how["targets"]), "passes": info["passes"] + (1 if peaks else 0),
                "quantiles_s": med["quantiles"], "quantiles_s_all": per["quantiles"], "ns_per_vector_node": med["quantiles"] / B / nodes * 1e9,
                "one_read_s_at_8TBps": 8.0 * B * W / HBM_BYTES_PER_S, "one_read_share": 8.0 * B * W / HBM_BYTES_PER_S / med["quantiles"],
                "copy_s": med["copy"], "form_s": med["form"], "form_ns_per_vector_node": med["form"] / B / nodes * 1e9,
                "sort_rows": nsort, "sort_s": med["sort"], "sort_s_scaled_to_B": med["sort"] * B / nsort})
            del src, dst, dq, dc, dw
            torch.cuda.empty_cache()
        del dX, dD
        E.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

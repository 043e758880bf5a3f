#!/usr/bin/env python3
"""Cost of the batched co-moments (gel_batch_comoments_device), in ONE process on the SAME device buffers (as
tools/quantiles_bench.py): for mixed-6x64 and stress-12x128 at B = 65536, from device events after a warm-up, the median of three
turns, the order of the cases alternating from turn to turn:
    a   disp (4 S columns) x the terminal row of the 34-column table (a view: ld = M 34)
    b   the self form of that terminal row
    c   disp x the whole table of altitude, dynamic_pressure, Q_alpha, M, vel_air (W = 5 M)
    d   disp x the whole table of all 34 columns (W = 34 M)
next to two yardsticks, neither of them the code under test:
    torch     the centred fp64 product (A - mean)^T (B - mean) on the same device tensors, in chunks of b columns where the centred
              copy would pass 2 GiB (no stated order, no rule for a NaN flight, a second centred copy of the source)
    one_read  ONE read of both sources at the 4.5 TB/s the quantiles' range pass measured
and to gel_output_table_batch_device forming that table.  The table's NaN entries (no impact point) are set to 0 before the timing,
so that every flight counts (listwise, a NaN anywhere in a flight's row would leave the call with nothing to do); the count is
reported.  The batch is built as tools/quantiles_bench.py builds it.
Prints one JSON line.   GPU box:  python3 tools/comoments_bench.py [B (65536)] [turns (3)]      (COMOM_BENCH_ONLY=workload,case runs
that one case alone: the command to put under a kernel trace)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIVE = ["altitude", "dynamic_pressure", "Q_alpha", "M", "vel_air"]
READ_BYTES_PER_S = 4.5e12
CHUNK_BYTES = 2 << 30


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
        raise SystemExit("comoments_bench: no GPU visible")
    out = {"B": B, "turns": turns, "cases": [], "build": _lib.build_info()}
    only = os.environ.get("COMOM_BENCH_ONLY")
    for wl in ("mixed-6x64", "stress-12x128"):
        if only and only.split(",")[0] != wl:
            continue
        pd, ud, _, xd = problem.make_problem(wl)
        ps, S, lc = pd["ps_params"], pd["num_sections"], pd["LaunchCondition"]
        E = Engine(con_dynamics.problem_arrays(pd, ud), D=[ps.D(i) for i in range(S)], tau=[ps.tau(i) for i in range(S)])
        M, K = E.M, 4 * S
        X64 = problem.synthetic_batch(pack_x(xd), M, 64)
        dX = torch.from_numpy(np.tile(X64, (B // 64 + 1, 1))[:B]).cuda()
        z = torch.randn(dX.shape, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))
        z[:, M:4 * M].abs_()                                        # positions outward only, as synthetic_batch
        z[:, 11 * M:] = 0.0                                         # controls and knot times as they are
        dX *= 1.0 + 1e-6 * z
        del z
        dD = torch.from_numpy(propagate.sample_dispersion(B, S, 0.02, seed=1, per="phase")).cuda().reshape(B, K)
        for name, cols, nc, whole, self_form in (("a", None, 34, False, False), ("b", None, 34, False, True), ("c", FIVE, 5, True, False),
                                                 ("d", None, 34, True, False)):
            if only and only.split(",")[1:] != [name]:
                continue
            table = torch.empty((B, M, nc), dtype=torch.float64, device="cuda")

            def form():
                E.output_table_batch_device(B, dX.data_ptr(), lc["lat"], lc["lon"], d_dispersion=dD.data_ptr(), columns=cols, d_out=table.data_ptr())
            form()
            assert E.sync() == 0
            table.nan_to_num_(nan=0.0, posinf=0.0, neginf=0.0)
            # the b side as a view of the table, and the same view as a tensor for the yardstick
            if whole:
                vb, Wb, ldb, tb = table.data_ptr(), M * nc, M * nc, table.reshape(B, M * nc)
            else:
                vb, Wb, ldb, tb = table.data_ptr() + 8 * (M - 1) * nc, nc, M * nc, table[:, M - 1, :]
            if self_form:
                va, Wa, lda, ta = vb, Wb, ldb, tb
            else:
                va, Wa, lda, ta = dD.data_ptr(), K, K, dD
            wb = Wa if self_form else Wb
            dC = torch.empty((Wa, wb), dtype=torch.float64, device="cuda")
            dsa, dsb, di = (torch.empty(s, dtype=torch.float64, device="cuda") for s in ((Wa, 2), (wb, 2), (2,)))
            ref = torch.empty((Wa, wb), dtype=torch.float64, device="cuda")

            def comom():
                E.batch_comoments_device(B, Wa, 1, lda, va, 0 if self_form else Wb, 1, ldb, 0 if self_form else vb, dC.data_ptr(), dsa.data_ptr(),
                                         0 if self_form else dsb.data_ptr(), di.data_ptr())
            step = max(1, min(wb, CHUNK_BYTES // (8 * B)))

            def centred():
                ac = ta - ta.mean(dim=0)
                for j0 in range(0, wb, step):
                    bc = tb[:, j0:j0 + step]
                    ref[:, j0:j0 + step] = ac.T @ (bc - bc.mean(dim=0))
            fns = {"comoments": comom, "torch": centred}
            for fn in fns.values():
                fn()
            assert E.sync() == 0
            torch.cuda.synchronize()
            per = {k: [] for k in fns}
            per["form"] = []
            for t in range(turns):
                for k in (list(fns) if t % 2 == 0 else list(fns)[::-1]):
                    per[k].append(timed(fns[k]))
            got, want = dC.cpu().numpy(), ref.cpu().numpy()
            scale = np.sqrt(np.outer(dsa.cpu().numpy()[:, 1], (dsa if self_form else dsb).cpu().numpy()[:, 1]))
            with np.errstate(invalid="ignore", divide="ignore"):
                dev = float(np.nanmax(np.where(scale > 0.0, np.abs(got - want) / scale, 0.0)))
            count = float(di.cpu().numpy()[0])
            for t in range(turns):                                   # (forming overwrites the table: timed last)
                per["form"].append(timed(form))
            med = {k: float(np.median(v)) for k, v in per.items()}
            info = E.batch_comoments_info(B, Wa, None if self_form else Wb)
            read = 8.0 * B * (Wa + (0 if self_form else Wb))
            out["cases"].append({
                "workload": wl, "case": name, "B": B, "M": M, "Wa": Wa, "Wb": wb, "self": self_form, "count": count, "info": info,
                "source_bytes": read, "comoments_s": med["comoments"], "comoments_s_all": per["comoments"],
                "torch_s": med["torch"], "torch_s_all": per["torch"], "torch_chunk_cols": step, "ratio_to_torch": med["comoments"] / med["torch"],
                "one_read_s_at_4p5TBps": read / READ_BYTES_PER_S, "ratio_to_one_read": med["comoments"] / (read / READ_BYTES_PER_S),
                "form_s": med["form"], "ratio_to_form": med["comoments"] / med["form"],
                "largest_difference_to_torch_over_sqrt_m2a_m2b": dev})
            del table, dC, dsa, dsb, di, ref
            torch.cuda.empty_cache()
        del dX, dD
        E.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

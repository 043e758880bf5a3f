#!/usr/bin/env python3
"""Cost of the batched products with K, the Jacobian of every row that is not a defect row (gel_con_matvec_device,
gel_con_rmatvec_device), in ONE process on the SAME device buffers, device events, a warm-up launch and >= 20
timed launches each:
  ns per vector of K v, K^T lambda and K^T lambda with accumulate at mixed-6x64 and stress-12x128 (all three aero kinds on every
  phase but the last, a short row table) for B = 1024, 16384, 65536, in both source forms, next to
  (1) the launch that produced the inputs: gel_eval_aero_all_device with gradients (dense form), gel_eval_batch_aero_device minus
      gel_eval_batch_device (record form);
  (2) the byte floor at 8 TB/s of what the call must move: the stored gradient values K names, jfn, the input and the output (the
      output twice with accumulate); the byte count is stated;
  (3) the defect products gel_jac_matvec_device / gel_jac_rmatvec_device at the same B.
Prints one JSON line.
GPU box:  python3 tools/con_products_bench.py [launches (20)] [workloads, comma separated] [batch sizes, comma separated]
          python3 tools/con_products_bench.py --loop WORKLOAD B N FORM   N launches of each product and nothing else (the program
                                                                         to put behind rocprofv3 --kernel-trace --stats, or --pmc alone)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8.0e12
KINDS = ["alpha", "q", "qalpha"]


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


def setup(wl):
    """(engine, x) with all three aero kinds on every phase but the last and a short row table (linear knot / time rows and
    node-function rows with and without a time column)"""
    from gelato_amd import Engine, con_dynamics, pack_x, problem
    pd, ud, _, xd = problem.make_problem(wl)
    E = Engine(con_dynamics.problem_arrays(pd, ud))
    for kind, lim in zip(KINDS, (0.2, 4.0e4, 5.0e3)):
        E.aero_configure(kind, [(i, 1, lim) for i in range(E.S - 1)])
    t0 = E.var_offset("t")
    lin = [(t0 + i + 1, 1.0, t0 + i, -1.0, 0.0) for i in range(E.S)]
    fn = [("orbit_energy", E.M - 1, 1.0e7, 1.0), ("altitude", E.M - 1, E.S, 4, [1.0e5, 1.0])]
    E.rows_configure(lin, fn)
    return E, pack_x(xd)


class Buffers:
    def __init__(self, torch, E, x, B):
        import numpy as np
        from gelato_amd import problem
        d = self.d = E.con_products_dims()
        self.width = E.aero_record_layout()[0]

        def buf(*shape):
            return torch.empty(shape, dtype=torch.float64, device="cuda")
        self.x = torch.from_numpy(np.tile(problem.synthetic_batch(x, E.M, 64), (B // 64, 1))).cuda()
        self.res, self.jv = buf(B, E.nres), buf(B, E.V)
        self.rows, self.jfn = buf(B, d["nlin"] + d["nfn"]), buf(B, d["nfn"], 7)
        self.con = [buf(B, d[k]) for k in KINDS]
        self.jac = [buf(B, sum(E.aero_dims(k)[1])) for k in KINDS]
        self.rec = buf(B, self.width)
        self.v, self.lam = torch.randn((B, E.nvars), dtype=torch.float64, device="cuda"), torch.randn((B, d["R"]), dtype=torch.float64, device="cuda")
        self.y, self.g = buf(B, d["R"]), torch.zeros((B, E.nvars), dtype=torch.float64, device="cuda")
        self.yd, self.gd = buf(B, E.nres), buf(B, E.nvars)

    def producers(self, E, B):
        p = lambda t: t.data_ptr()   # noqa: E731
        return {"aero_all": lambda: E.eval_aero_all_device(B, p(self.x), [p(c) for c in self.con], [p(j) for j in self.jac]),
                "batch_aero": lambda: E.eval_batch_aero_device(B, p(self.x), p(self.res), p(self.jv), p(self.rec)),
                "batch": lambda: E.eval_batch_device(B, p(self.x), p(self.res), p(self.jv)),
                "rows": lambda: E.rows_eval_device(B, p(self.x), p(self.rows), p(self.jfn))}

    def products(self, E, B, form):
        p = lambda t: t.data_ptr()   # noqa: E731
        jac = [p(j) for j in self.jac] if form == "dense" else None
        rec = p(self.rec) if form == "record" else 0
        return {"matvec": lambda: E.con_matvec_device(B, p(self.jfn), jac, rec, p(self.v), p(self.y)),
                "rmatvec": lambda: E.con_rmatvec_device(B, p(self.jfn), jac, rec, p(self.lam), p(self.g)),
                "rmatvec_accumulate": lambda: E.con_rmatvec_device(B, p(self.jfn), jac, rec, p(self.lam), p(self.g), accumulate=True)}


def loop(wl, B, n, form):
    import torch
    E, x = setup(wl)
    bf = Buffers(torch, E, x, B)
    for fn in bf.producers(E, B).values():
        fn()
    prods = bf.products(E, B, form)
    for _ in range(n):
        prods["matvec"]()
        prods["rmatvec"]()
    assert E.sync() == 0


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--loop":
        return loop(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5] if len(sys.argv) > 5 else "record")
    import torch
    from gelato_amd import _lib
    n = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 20
    wls = sys.argv[2].split(",") if len(sys.argv) > 2 else ["mixed-6x64", "stress-12x128"]
    Bs = [int(b) for b in sys.argv[3].split(",")] if len(sys.argv) > 3 else [1024, 16384, 65536]
    if not torch.cuda.is_available():
        raise SystemExit("con_products_bench: no GPU visible")
    out = {"launches": n, "build": _lib.build_info(), "workloads": {}}
    for wl in wls:
        E, x = setup(wl)
        d = E.con_products_dims()
        width, _con, rec_idx = E.aero_record_layout()
        stored = sum(int((rec_idx[k] >= 0).sum()) for k in KINDS)          # the gradient values K names (structural zeros left out)
        rec = {"dims": d, "num_vars": E.nvars, "record_width": width, "stored_gradient_values": stored, "B": {}}
        for B in Bs:
            bf = Buffers(torch, E, x, B)
            r = {}
            for k, fn in bf.producers(E, B).items():
                r[k + "_ns_per_vector"] = timed(torch, fn, n) / B * 1e9
                assert E.sync() == 0
            r["defect_matvec_ns_per_vector"] = timed(torch, lambda: E.jac_matvec_device(B, bf.jv.data_ptr(), bf.v.data_ptr(), bf.yd.data_ptr()), n) / B * 1e9
            r["defect_rmatvec_ns_per_vector"] = timed(torch, lambda: E.jac_rmatvec_device(B, bf.jv.data_ptr(), bf.res.data_ptr(), bf.gd.data_ptr()), n) / B * 1e9
            assert E.sync() == 0
            for form in ("dense", "record"):
                producer = r["aero_all_ns_per_vector"] if form == "dense" else r["batch_aero_ns_per_vector"] - r["batch_ns_per_vector"]
                f = {"producer_ns_per_vector": producer}
                for k, fn in bf.products(E, B, form).items():
                    bf.g.zero_()
                    t = timed(torch, fn, n) / B * 1e9
                    assert E.sync() == 0
                    nin, nout = (d["R"], E.nvars) if k != "matvec" else (E.nvars, d["R"])
                    floor_bytes = 8 * (stored + 7 * d["nfn"] + nin + nout * (2 if k == "rmatvec_accumulate" else 1))
                    f[k] = {"ns_per_vector": t, "times_producer": t / producer, "floor_bytes_per_vector": floor_bytes,
                            "floor_ns_per_vector": floor_bytes / HBM_BYTES_PER_S * 1e9,
                            "share_of_floor": floor_bytes / HBM_BYTES_PER_S * 1e9 / t,
                            "times_defect_product": t / r["defect_matvec_ns_per_vector" if k == "matvec" else "defect_rmatvec_ns_per_vector"]}
                r[form] = f
            rec["B"][str(B)] = r
            del bf
            torch.cuda.empty_cache()
        out["workloads"][wl] = rec
        E.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

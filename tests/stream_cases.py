"""The caller-stream case table (tests/test_caller_stream.py runs it on the GPU, tests/test_caller_stream_cpu.py holds its keys
against include/gelato_amd.h): CASES = {C function name: [(case id, make)]}, make() -> stream_harness.Case.  Every prototype of
the header with a `void* stream` parameter has a key; an entry point added later without a case fails the CPU guard.

Importing this module needs neither a GPU nor torch: everything heavy happens inside make()."""
import numpy as np

KINDS = ["alpha", "q", "qalpha"]
GROUPS = ["mass", "pos", "vel", "quat"]
STALE_SEED = 777
_last = {}


def engine(name, flags=0, cfg=None):
    """(engine, x0) of a named problem; only the last one is kept, so that few handles (and streams) are alive at a time"""
    from gelato_amd import Engine
    import jac_products_truth as jt
    key = (name, flags, cfg)
    if _last.get("key") != key:
        _last.clear()
        prob, x0 = jt.named(name)
        E = Engine(prob, flags=flags)
        if cfg:
            CONFIGS[cfg](E)
        _last.update(key=key, E=E, x0=x0)
    return _last["E"], _last["x0"]


def inputs(E, x0, B, distinct=64):
    """(good, stale) [min(B, distinct)][nvars]: two different valid batches (element 0 of synthetic_batch is x0 for every seed,
    so the stale batch leaves it out)"""
    from gelato_amd import problem
    P = min(B, distinct)
    return problem.synthetic_batch(x0, E.M, P), problem.synthetic_batch(x0, E.M, P + 1, seed=STALE_SEED)[1:]


# ---- configurations of a handle -------------------------------------------------------------------------------------------
def _cfg_aero_all(E):
    for kind, lim in zip(KINDS, (0.2, 4.0e4, 5.0e3)):
        E.aero_configure(kind, [(i, 1, lim) for i in range(E.S - 1)])


def _cfg_aero_initial(E):
    """"initial" specs only: no row for the fused kernel's lanes, part A of the record is empty"""
    E.aero_configure("alpha", [(i, 0, 0.2) for i in range(0, E.S - 1, 2)])
    E.aero_configure("q", [])
    E.aero_configure("qalpha", [(1, 0, 5.0e3)])


def _row_tables():
    from gelato_amd import problem
    from tools.exact_rows_bench import tables
    pdict, unitdict, condition, _x = problem.make_problem("example")
    return tables(pdict, unitdict, condition)


def _cfg_rows_terminal(E):
    lin = [(0, 1.0, 1, -1.0, 0.5), (E.var_offset("t"), 2.0, -1, 0.0, -1.0)]
    E.rows_configure(lin, _row_tables()["terminal_user"])


def _cfg_rows_waypoint(E):
    way = _row_tables()["waypoint"]
    assert len(way) == 72
    E.rows_configure([], way)


def _cfg_example_everything(E):
    _cfg_aero_all(E)
    _cfg_rows_terminal(E)


CONFIGS = {"aero_all": _cfg_aero_all, "aero_initial": _cfg_aero_initial, "rows_terminal": _cfg_rows_terminal,
           "rows_waypoint": _cfg_rows_waypoint, "example_everything": _cfg_example_everything}


# ---- case builders ----------------------------------------------------------------------------------------------------------
def _case(*a, **k):
    from stream_harness import Case
    return Case(*a, **k)


def eval_batch(name, flags, B, want):
    def make():
        E, x0 = engine(name, flags)
        outs = {}
        if "r" in want:
            outs["res"] = (B, E.nres)
        if "j" in want:
            outs["jvar"] = (B, E.V)
        return _case(E, B, {"x": inputs(E, x0, B)}, outs,
                     lambda E, p, s: E.eval_batch_device(B, p["x"], p.get("res", 0), p.get("jvar", 0), s))
    return "eval_batch %s flags %d B %d %s" % (name, flags, B, want), make


def full_chain(name, flags, B):
    def make():
        E, x0 = engine(name, flags)

        def call(E, p, s):
            E.fill_full_device(B, p["jfull"], s)
            E.eval_full_device(B, p["x"], p["res"], p["jvar"], p["jfull"], s)
            E.expand_full_device(B, p["jvar"], p["jfull_expanded"], s)
            E.fill_full_device(B, p["jfull_updated"], s)
            E.update_full_device(B, p["jvar"], p["jfull_updated"], s)
        outs = {"res": (B, E.nres), "jvar": (B, E.V)}
        outs.update({k: (B, E.total_nnz) for k in ("jfull", "jfull_expanded", "jfull_updated")})
        return _case(E, B, {"x": inputs(E, x0, B)}, outs, call)
    return "full chain %s flags %d B %d" % (name, flags, B), make


def _thirds(E):
    nu = 4 * E.num_chunks()
    return [0, nu // 3, (2 * nu) // 3, nu]


def shard_units(name, flags, B):
    def make():
        E, x0 = engine(name, flags)
        ub = _thirds(E)

        def call(E, p, s):
            for r in range(3):
                E.eval_shard_units_device(B, p["x"], p["res"], p["jvar"], ub[r], ub[r + 1] - ub[r], s)
        return _case(E, B, {"x": inputs(E, x0, B)}, {"res": (B, E.nres), "jvar": (B, E.V)}, call)
    return "shard units %s flags %d B %d" % (name, flags, B), make


def shard_packed(name, flags, B):
    def make():
        E, x0 = engine(name, flags)
        width, _rp, _jp = E.shard_plan(_thirds(E))

        def call(E, p, s):
            for r in range(3):                      # every rank of a world of 3, on ONE stream
                E.eval_shard_packed_device(B, p["x"], p["exchange"], r, s)
            E.shard_unpack_device(B, p["exchange"], p["res"], p["jvar"], s)
        return _case(E, B, {"x": inputs(E, x0, B)}, {"exchange": (3, B, width), "res": (B, E.nres), "jvar": (B, E.V)}, call)
    return "shard packed + unpack %s flags %d B %d" % (name, flags, B), make


def aero_all(flags, B, grads):
    def make():
        E, x0 = engine("mixed-6x64", flags, "aero_all")
        dims = [E.aero_dims(k) for k in KINDS]
        outs = {"con%d" % i: (B, d[0]) for i, d in enumerate(dims)}
        if grads:
            outs.update({"jac%d" % i: (B, sum(d[1])) for i, d in enumerate(dims)})

        def call(E, p, s):
            E.eval_aero_all_device(B, p["x"], [p["con%d" % i] for i in range(3)], [p["jac%d" % i] for i in range(3)] if grads else None, s)
        return _case(E, B, {"x": inputs(E, x0, B)}, outs, call)
    return "aero all flags %d B %d %s" % (flags, B, "values+gradients" if grads else "values"), make


def batch_aero(flags, B, cfg="aero_all"):
    def make():
        E, x0 = engine("mixed-6x64", flags, cfg)
        width, ocon, ojac = E.aero_record_layout()
        named = np.concatenate([ocon[k] for k in KINDS] + [ojac[k] for k in KINDS])
        named = np.unique(named[named >= 0]).astype(np.int64)       # the rest of a record is padding / the fused lanes' dump area
        return _case(E, B, {"x": inputs(E, x0, B)}, {"res": (B, E.nres), "jvar": (B, E.V), "aero": (B, width)},
                     lambda E, p, s: E.eval_batch_aero_device(B, p["x"], p["res"], p["jvar"], p["aero"], s), select={"aero": named})
    return "batch aero flags %d B %d %s" % (flags, B, cfg), make


def rows(flags, B, jfn, cfg):
    def make():
        E, x0 = engine("example", flags, cfg)
        outs = {"con": (B, E._nlin + E._nfn)}
        if jfn:
            outs["jfn"] = (B, E._nfn, 7)
        return _case(E, B, {"x": inputs(E, x0, B)}, outs, lambda E, p, s: E.rows_eval_device(B, p["x"], p["con"], p.get("jfn", 0), s))
    return "rows %s flags %d B %d %s" % (cfg, flags, B, "con+jfn" if jfn else "con"), make


def jac_fd(name, blocks):
    def make():
        E, x0 = engine(name, 0)
        if blocks:
            outs = {g: (int(E.jac_fd_block_dims(g)[3][-1]),) for g in GROUPS}
        else:
            outs = {g: (E.nrows[i], E.nvars) for i, g in enumerate(GROUPS)}

        def call(E, p, s):
            for g in GROUPS:                        # all four groups back to back
                E.jac_fd_device(g, p["x"], p[g], blocks, s)
        good, stale = inputs(E, x0, 1)
        return _case(E, 1, {"x": (good, stale)}, outs, call)
    return "jac_fd %s %s" % (name, "blocks" if blocks else "dense"), make


def mesh(name, B, diff):
    def make():
        E, x0 = engine(name, 0)
        outs = {"err": (B, E.S, 4)}
        if diff:
            outs["diff"] = (B, E.mesh_npts(), 11)
        return _case(E, B, {"x": inputs(E, x0, B)}, outs, lambda E, p, s: E.mesh_error_device(B, p["x"], p["err"], p.get("diff", 0), s))
    return "mesh error %s B %d %s" % (name, B, "err+diff" if diff else "err"), make


def jprod(name, flags, B, transpose):
    def make():
        E, x0 = engine(name, flags)
        good, stale = inputs(E, x0, B)
        jv = []
        for X in (good, stale):
            _r, j, rc = E.eval_batch(X, want_res=False)
            assert rc == 0
            jv.append(j)
        rng = np.random.default_rng(20261017 + flags)
        nin, nout = (E.nres, E.nvars) if transpose else (E.nvars, E.nres)
        vin = (rng.standard_normal((len(good), nin)), rng.standard_normal((len(good), nin)))
        fn = (lambda E, p, s: E.jac_rmatvec_device(B, p["jvar"], p["in"], p["out"], s)) if transpose else \
             (lambda E, p, s: E.jac_matvec_device(B, p["jvar"], p["in"], p["out"], s))
        return _case(E, B, {"jvar": tuple(jv), "in": vin}, {"out": (B, nout)}, fn)
    return "%s %s flags %d B %d" % ("J^T lambda" if transpose else "J v", name, flags, B), make


# ---- the table --------------------------------------------------------------------------------------------------------------
_EVAL_SHAPES = [("example", (1, 5, 300)), ("mixed-6x64", (5, 16384)), ("stress-12x128", (3, 300)), ("3x32", (5, 300))]
_eval = [eval_batch(n, f, B, w) for f in (0, 8, 32) for n, Bs in _EVAL_SHAPES for B in Bs for w in ("rj", "r", "j")]
_full = [full_chain(n, f, B) for f in (0, 32) for n, B in (("example", 3), ("mixed-6x64", 37))]
_units = [shard_units(n, f, B) for f in (0, 8) for n, B in (("mixed-6x64", 5), ("stress-12x128", 2))]
_packed = [shard_packed(n, f, B) for f in (0, 8) for n, B in (("mixed-6x64", 5), ("stress-12x128", 2))]
_aero_all = [aero_all(f, B, g) for f in (0, 64) for B in (1, 300, 16384) for g in (False, True)]
_batch_aero = [batch_aero(f, B) for f in (0, 64, 32 | 64) for B in (1, 300, 16384)] + [batch_aero(f, 300, "aero_initial") for f in (0, 64)]
_rows = [rows(f, B, j, "rows_terminal") for f in (0, 128, 8 | 128) for B in (1, 300) for j in (False, True)] + \
        [rows(f, B, True, "rows_waypoint") for f in (0, 128, 8 | 128) for B in (1, 300)]
_jfd = [jac_fd(n, b) for n in ("example", "ragged") for b in (False, True)]
_mesh = [mesh(n, B, d) for n, B in (("example", 1), ("mixed-6x64", 300)) for d in (False, True)]
_JP_SHAPES = [("example", 1), ("mixed-6x64", 37), ("mixed-6x64", 1024), ("stress-12x128", 3)]
_matvec = [jprod(n, f, B, False) for f in (0, 8, 32) for n, B in _JP_SHAPES]
_rmatvec = [jprod(n, f, B, True) for f in (0, 8, 32) for n, B in _JP_SHAPES]

CASES = {
    "gel_eval_batch_device": _eval,
    # one chain: fill_full -> eval_full -> expand_full / fill_full + update_full
    "gel_fill_full_device": _full, "gel_eval_full_device": _full, "gel_expand_full_device": _full, "gel_update_full_device": _full,
    "gel_eval_shard_units_device": _units,
    "gel_eval_shard_packed_device": _packed, "gel_shard_unpack_device": _packed,
    "gel_eval_aero_all_device": _aero_all,
    "gel_eval_batch_aero_device": _batch_aero,
    "gel_rows_eval_device": _rows,
    "gel_jac_fd_device": _jfd,
    "gel_mesh_error_device": _mesh,
    "gel_jac_matvec_device": _matvec,
    "gel_jac_rmatvec_device": _rmatvec,
    # every case ends with gel_sync(stream) (stream_harness.Pending.finish); the status tests of test_caller_stream.py read it too
    "gel_sync": _eval[:1],
}


def all_cases():
    """every case once, in table order -> [(id, make)]"""
    seen, out = set(), []
    for lst in CASES.values():
        for cid, make in lst:
            if cid not in seen:
                seen.add(cid)
                out.append((cid, make))
    return out

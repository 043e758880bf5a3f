"""Reference and bound of the products with K, the Jacobian of every row that is not a defect row (test infrastructure, shared
by test_con_products_cpu.py and test_con_products.py; include/gelato_amd.h gel_con_*).

The reference is independent of the operator tables.  The triplets (R, C, vals) of ONE vector come from the row lists the test
itself configured, Engine.aero_pattern and the values in either source form: the dense arrays of eval_aero_all, or
Engine.aero_gather(record, map) of a record.  An entry whose record-map index is -1 is a structural zero and is dropped in both
forms.  Products are accumulated with jac_products_truth._accumulate (numpy.longdouble, or math.fsum where longdouble is no wider).

Bound (derived, not measured): with m the number of entries of a row (column), u = 2^-53, gamma_k = k u / (1 - k u),

    |y_i - y^_i| <= 2 gamma_{m_i + 2} (|K| |v|)_i          |g_j - g^_j| <= 2 gamma_{m_j + 2} (|K|^T |lambda|)_j

|K| |in| is taken over the triplets.  gamma_m bounds an m-term fp64 sum of products in any fixed order, with or without FMA.  Where
the bound is 0 the output must be exactly 0."""
import numpy as np

import jac_products_truth as jt

LD = jt.LD
KINDS = ["alpha", "q", "qalpha"]
AERO_VARS = ["position", "velocity", "quaternion", "t"]


def rows_of_lists(E, linear, nodefn):
    """-> (R, C, source) of the row table's entries: source = ("c", coefficient) or ("j", index into one vector's jfn.ravel())"""
    M = E.M
    R, C, src = [], [], []
    for r, (i0, c0, i1, c1, _cc) in enumerate(linear):
        R.append(r), C.append(int(i0)), src.append(("c", float(c0)))
        if int(i1) >= 0:
            R.append(r), C.append(int(i1)), src.append(("c", float(c1)))
    nlin = len(linear)
    for r, row in enumerate(nodefn):
        node, tcol = (row[1], -1) if len(row) == 4 else (row[1], row[2])
        for c in range(3):
            R.append(nlin + r), C.append(E.var_offset("position") + 3 * int(node) + c), src.append(("j", 7 * r + c))
        for c in range(3):
            R.append(nlin + r), C.append(E.var_offset("velocity") + 3 * int(node) + c), src.append(("j", 7 * r + 3 + c))
        if int(tcol) >= 0:
            R.append(nlin + r), C.append(E.var_offset("t") + int(tcol)), src.append(("j", 7 * r + 6))
    assert M == E.M
    return np.array(R, dtype=np.int64), np.array(C, dtype=np.int64), src


class Truth:
    """the triplet structure of one configuration: built once per engine, values filled per vector"""

    def __init__(self, E, linear, nodefn):
        self.E = E
        self.nlin, self.nfn = len(linear), len(nodefn)
        self.Rr, self.Cr, src = rows_of_lists(E, linear, nodefn)
        self.const = np.array([s[1] if s[0] == "c" else 0.0 for s in src])
        self.jsel = np.array([k for k, s in enumerate(src) if s[0] == "j"], dtype=np.int64)
        self.jidx = np.array([s[1] for s in src if s[0] == "j"], dtype=np.int64)
        self.width, _con, self.rec_idx = E.aero_record_layout()
        row0 = self.nlin + self.nfn
        self.aero = {}
        self.nrows = {}
        for kind in KINDS:
            nrow, nnz = E.aero_dims(kind)
            self.nrows[kind] = nrow
            if not nrow:
                continue
            pat = E.aero_pattern(kind)
            R = np.concatenate([pat[v][0].astype(np.int64) + row0 for v in range(4)])
            C = np.concatenate([pat[v][1].astype(np.int64) + E.var_offset(AERO_VARS[v]) for v in range(4)])
            keep = self.rec_idx[kind] >= 0                      # structural zeros are not entries of K
            assert R.size == sum(nnz) == keep.size
            self.aero[kind] = (R[keep], C[keep], keep)
            row0 += nrow
        self.R = row0

    def triplets(self, jfn=None, aero_jac=None, aero_record=None):
        """one vector's (R, C, vals): jfn [nfn, 7], aero_jac {kind: [sum nnz]} or aero_record [width]"""
        vals = self.const.copy()
        if self.jsel.size:
            vals[self.jsel] = np.asarray(jfn, dtype=np.float64).ravel()[self.jidx]
        R, C, V = [self.Rr], [self.Cr], [vals]
        for kind, (r, c, keep) in self.aero.items():
            if aero_record is not None:
                dense = self.E.aero_gather(np.asarray(aero_record), self.rec_idx[kind])
            else:
                dense = np.asarray(aero_jac[kind], dtype=np.float64)
            R.append(r), C.append(c), V.append(dense[keep])
        return np.concatenate(R), np.concatenate(C), np.concatenate(V)

    def dense(self, R, C, vals):
        """K [R, nvars]; cells that several entries share hold their sum"""
        K = np.zeros((self.R, self.E.nvars))
        np.add.at(K, (R, C), vals)
        return K


def products(T, R, C, vals, inp, transpose):
    """-> (reference out [n] longdouble, |K| |in| [n] longdouble, entry counts m [n]) for one vector"""
    if transpose:
        out_idx, in_idx, n = C, R, T.E.nvars
    else:
        out_idx, in_idx, n = R, C, T.R
    w = np.asarray(inp, dtype=np.float64)[in_idx]
    ref = jt._accumulate(out_idx, jt._terms(vals, w), n)
    mag = jt._accumulate(out_idx, jt._terms(np.abs(vals), np.abs(w)), n)
    return ref, mag, np.bincount(out_idx, minlength=n)


def check(T, R, C, vals, inp, got, transpose):
    """-> (ok, largest share of the bound used, index of the worst element); an element whose bound is 0 must be exactly 0"""
    ref, mag, m = products(T, R, C, vals, inp, transpose)
    bd = jt.bound(mag, m)
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got.astype(LD) - ref)
    zero = bd == 0
    ok = bool(np.all(err[~zero] <= bd[~zero])) and bool(np.all(got[zero] == 0.0))
    share = np.zeros(err.shape, dtype=np.float64)
    share[~zero] = (err[~zero] / bd[~zero]).astype(np.float64)
    share[zero] = np.where(got[zero] == 0.0, 0.0, np.inf)
    worst = int(np.argmax(share))
    return ok, float(share[worst]), worst


# ---- the configurations the tests share ---------------------------------------------------------------------------------------
def example_full_tables():
    """(linear, nodefn) of the example's full row table: the linear rows as con_init_terminal_knot._Rows builds them, the
    terminal / user rows and the 72 waypoint rows of tools.exact_rows_bench.tables"""
    from gelato_amd import con_init_terminal_knot as ck
    from gelato_amd import problem
    from tools.exact_rows_bench import tables
    pdict, unitdict, condition, _x = problem.make_problem("example")
    pd = dict(pdict, device=-1)
    pd.pop("_gelato_amd", None)
    lin = list(ck._Rows(pd, unitdict, condition).lin)
    tb = tables(pdict, unitdict, condition)
    assert len(tb["waypoint"]) == 72
    return lin, list(tb["terminal_user"]) + list(tb["waypoint"])


def aero_all_specs(E):
    """all three kinds on every phase but the last, every node (stream_cases' aero_all limits)"""
    return {kind: [(i, 1, lim) for i in range(E.S - 1)] for kind, lim in zip(KINDS, (0.2, 4.0e4, 5.0e3))}


def configure(E, linear, nodefn, aero):
    E.rows_configure(linear, nodefn)
    for kind in KINDS:
        E.aero_configure(kind, aero.get(kind, []))
    return Truth(E, linear, nodefn)


def small_tables(E):
    """a short table for problems without a shipped one: two knot-style linear rows, a one-term time row, a row whose two terms
    share ONE cell, and node-function rows with and without a time column at the first and last state nodes"""
    t0 = E.var_offset("t")
    lin = [(0, 1.0, 1, -1.0, 0.5), (t0, 2.0, -1, 0.0, -1.0), (t0 + E.S, 1.0, t0, -1.0, 0.0),
           (E.var_offset("position") + 4, 0.75, E.var_offset("position") + 4, 0.5, 0.0)]
    fn = [("orbit_energy", E.M - 1, 1.0e7, 1.0), ("radius", 0, 6.4e6, 1.0),
          ("altitude", E.M - 1, E.S, 4, [1.0e5, 1.0]), ("latitude_deg", 0, 0, 5, [90.0, 30.0]),
          ("longitude_deg", E.M // 2, 1, 5, [180.0, 140.0])]
    return lin, fn


def random_values(T, B, seed, record=False):
    """random finite values of B vectors (the operator is linear in them): jfn [B, nfn, 7], aero_jac {kind: [B, sum nnz]} and the
    record [B, width] that holds the same values (structural zeros: the dense arrays hold random numbers there, which K must not
    read; the record has no cell for them)"""
    rng = np.random.default_rng(seed)
    E = T.E
    jfn = rng.standard_normal((B, T.nfn, 7)) if T.nfn else None
    jac = {kind: rng.standard_normal((B, sum(E.aero_dims(kind)[1]))) for kind in T.aero}
    rec = None
    if T.aero:
        rec = rng.standard_normal((B, T.width))       # the cells no entry names hold random numbers too
        for kind in T.aero:
            idx = T.rec_idx[kind]
            rec[:, idx[idx >= 0]] = jac[kind][:, idx >= 0]
    return jfn, (jac if T.aero else None), rec

"""Reference and bound of the Jacobian products (test infrastructure, shared by test_jac_products_cpu.py and test_jac_products.py).

The reference is independent of the operator tables: the COO triplets (R, C, vals) of ONE vector come from Engine.pattern(), the
group and variable offsets and Engine.expand(jvar); the products are accumulated in numpy.longdouble (64-bit mantissa), or, where
longdouble is no wider than double, row by row with math.fsum.

Bound (derived, not measured).  With m_i the number of non-zero entries of row (column) i, u = 2^-53, gamma_k = k u / (1 - k u):

    |y_i - y^_i| <= 2 gamma_{m_i + 2} (|J| |v|)_i          |g_j - g^_j| <= 2 gamma_{m_j + 2} (|J|^T |lambda|)_j

gamma_m is the standard bound of an m-term fp64 sum of products in any order, with or without FMA; the two extra terms and the
factor 2 pay for a regrouping of a diagonal coefficient.  Where the bound is 0 the output must be exactly 0."""
import math

import numpy as np

U = 2.0 ** -53
LD = np.longdouble
WIDE = np.finfo(np.longdouble).nmant >= 63
BLOCK_GROUP = [0, 0, 1, 1, 1, 2, 2, 2, 2, 2, 3, 3, 3]
BLOCK_VAR = ["mass", "t", "position", "velocity", "t", "mass", "position", "velocity", "quaternion", "t", "quaternion", "u", "t"]


def named(name):
    """-> (prob, x0) of example / mixed-6x64 / stress-12x128 / ragged"""
    from gelato_amd import con_dynamics, pack_x, problem
    if name == "ragged":
        import states
        return states.ragged_state()
    pdict, unitdict, _c, xdict = problem.make_problem(name)
    return dict(con_dynamics.problem_arrays(pdict, unitdict)), pack_x(xdict)


def triplet_index(E):
    """-> (R, C) int64 [total_nnz]: global row (residual order) and global column (packed decision vector) of every COO entry"""
    row_off = [0, E.N, 4 * E.N, 7 * E.N]
    R = np.empty(E.total_nnz, dtype=np.int64)
    C = np.empty(E.total_nnz, dtype=np.int64)
    for b, (r, c) in enumerate(E.pattern()):
        sl = slice(int(E.block_off[b]), int(E.block_off[b + 1]))
        R[sl] = r.astype(np.int64) + row_off[BLOCK_GROUP[b]]
        C[sl] = c.astype(np.int64) + E.var_offset(BLOCK_VAR[b])
    return R, C


def structural_nonzero(E):
    """boolean [total_nnz]: variable entries and non-zero constants (what the tables keep)"""
    return (E.full_source() != -1) | (E.const_values() != 0.0)


def _accumulate(idx, terms, n):
    """sum of terms (fp64 products, exact in longdouble or summed exactly by fsum) per index"""
    if WIDE:
        out = np.zeros(n, dtype=LD)
        np.add.at(out, idx, terms)
        return out
    order = np.argsort(idx, kind="stable")
    idx_s, t_s = idx[order], terms[order]
    cuts = np.searchsorted(idx_s, np.arange(n + 1))
    return np.array([math.fsum(t_s[cuts[i]:cuts[i + 1]]) for i in range(n)], dtype=LD)


def _terms(vals, w):
    if WIDE:
        return vals.astype(LD) * w.astype(LD)
    return vals * w   # no wider format on this platform: fp64 products, each row summed exactly by math.fsum


def products(E, R, C, vals, inp, transpose):
    """-> (reference out [n] longdouble, |J| |in| [n] longdouble, counts m [n]) for one vector"""
    nz = structural_nonzero(E)
    if transpose:
        out_idx, in_idx, n = C, R, E.nvars
    else:
        out_idx, in_idx, n = R, C, E.nres
    w = np.asarray(inp, dtype=np.float64)[in_idx]
    ref = _accumulate(out_idx, _terms(vals, w), n)
    mag = _accumulate(out_idx, _terms(np.abs(vals), np.abs(w)), n)
    m = np.bincount(out_idx[nz], minlength=n)
    return ref, mag, m


def bound(mag, m):
    k = (m + 2).astype(LD) * LD(U)
    return LD(2) * k / (LD(1) - k) * mag


def check(E, R, C, vals, inp, got, transpose):
    """-> (ok, largest share of the bound used, index of the worst element); an element whose bound is 0 must be exactly 0"""
    ref, mag, m = products(E, R, C, vals, inp, transpose)
    bd = bound(mag, m)
    err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - ref)
    zero = bd == 0
    ok = bool(np.all(err[~zero] <= bd[~zero])) and bool(np.all(np.asarray(got)[zero] == 0.0))
    share = np.zeros(err.shape, dtype=np.float64)
    share[~zero] = (err[~zero] / bd[~zero]).astype(np.float64)
    share[zero] = np.where(np.asarray(got)[zero] == 0.0, 0.0, np.inf)
    worst = int(np.argmax(share))
    return ok, float(share[worst]), worst


def oracle_full_values(prob, x, E):
    """the CPU oracle's COO values of the four groups in the engine's full order"""
    import oracle
    P = oracle.Problem(prob, D=[E.D(i) for i in range(E.S)], tau=[E.tau(i) for i in range(E.S)])
    parts = []
    for g in oracle.GROUPS:
        J = P.jacobian(g, x)
        parts.extend(J[var]["coo"][2] for var in oracle.BLOCK_VARS[g])
    full = np.concatenate(parts)
    assert full.size == E.total_nnz
    return full

"""Jacobian products from the compact values, host side (no GPU): gel_jac_products_host on host-only handles against a
reference built from the pattern, the constant template and the gather map (tests/jac_products_truth.py) under the derived
bound; the bound's teeth; the table counts; argument errors."""
import numpy as np
import pytest

import jac_products_truth as jt

NAMES = ["example", "ragged", "mixed-6x64", "stress-12x128"]
FLAGS = [0, 8, 32]   # default, GEL_FLAG_FD_RECOMPUTE, GEL_FLAG_EXACT_DEFECT_JAC
_CACHE = {}


def _case(name, flags):
    """host-only engine, triplet indices, one vector's compact values: the oracle's Jacobian read through var_index (example,
    ragged, mixed-6x64) or seeded random values (stress-12x128: the matrix is linear in jvar, any values test the tables)"""
    key = (name, flags)
    if key not in _CACHE:
        from gelato_amd import Engine
        prob, x0 = jt.named(name)
        E = Engine(prob, device=-1, flags=flags)
        R, C = jt.triplet_index(E)
        if name == "stress-12x128":
            jvar = np.random.default_rng(128 + flags).standard_normal(E.V)
        else:
            if ("full", name) not in _CACHE:
                _CACHE[("full", name)] = jt.oracle_full_values(prob, x0, E)
            jvar = _CACHE[("full", name)][E.var_index()]
        _CACHE[key] = (E, R, C, jvar)
    return _CACHE[key]


def _inputs(E, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(E.nvars), rng.standard_normal(E.nres)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("name", NAMES)
def test_host_products_within_bound(name, flags):
    E, R, C, jvar = _case(name, flags)
    vals = E.expand(jvar)
    v, lam = _inputs(E, 20261016)
    y, rc = E.jac_products_host(jvar, v)
    assert rc == 0 and y.shape == (E.nres,)
    g, rc = E.jac_products_host(jvar, lam, transpose=True)
    assert rc == 0 and g.shape == (E.nvars,)
    ok_y, use_y, wy = jt.check(E, R, C, vals, v, y, False)
    ok_g, use_g, wg = jt.check(E, R, C, vals, lam, g, True)
    print("bound usage %s flags %d: J v %.3f (row %d)  J^T lambda %.3f (column %d)" % (name, flags, use_y, wy, use_g, wg))
    assert ok_y, (name, flags, use_y, wy)
    assert ok_g, (name, flags, use_g, wg)


@pytest.mark.parametrize("name", NAMES)
def test_batched_host_products_equal_single(name):
    E, R, C, jvar = _case(name, 0)
    rng = np.random.default_rng(5)
    JV = np.stack([jvar, jvar * 0.5, rng.standard_normal(E.V)])
    Vs, Ls = rng.standard_normal((3, E.nvars)), rng.standard_normal((3, E.nres))
    Y, rc = E.jac_products_host(JV, Vs)
    G, rc2 = E.jac_products_host(JV, Ls, transpose=True)
    assert rc == 0 and rc2 == 0
    for b in range(3):
        assert np.array_equal(Y[b], E.jac_products_host(JV[b], Vs[b])[0])
        assert np.array_equal(G[b], E.jac_products_host(JV[b], Ls[b], transpose=True)[0])


def test_columns_without_entries_are_exact_zeros():
    """the u columns of hold-type phases have no entry: 28 / 256 / 1280 / 42 of them"""
    for name, want in zip(["example", "mixed-6x64", "stress-12x128", "ragged"], [28, 256, 1280, 42]):
        E, R, C, jvar = _case(name, 0)
        nz = jt.structural_nonzero(E)
        empty = np.bincount(C[nz], minlength=E.nvars) == 0
        assert int(empty.sum()) == want, (name, int(empty.sum()))
        g = E.jac_products_host(jvar, np.full(E.nres, np.pi), transpose=True)[0]
        assert np.all(g[empty] == 0.0) and not np.any(np.signbit(g[empty]))


@pytest.mark.parametrize("name", ["example", "ragged", "mixed-6x64"])
def test_bound_has_teeth(name):
    """a reference with (a) the negated uses taken with a plus sign, (b) the t columns dropped, (c) the per-phase diagonal scalar
    used once instead of 3n times is NOT met by the products: each mutation violates the bound"""
    E, R, C, jvar = _case(name, 0)
    vals = E.expand(jvar)
    src = E.full_source()
    v, lam = _inputs(E, 7)
    y = E.jac_products_host(jvar, v)[0]
    g = E.jac_products_host(jvar, lam, transpose=True)[0]
    tcol0 = E.var_offset("t")
    mutants = {}
    a = vals.copy()
    a[src <= -2] = -a[src <= -2]
    assert (src <= -2).sum() == {"example": 916, "mixed-6x64": 4864, "ragged": 2878}[name]
    mutants["plus sign"] = a
    b = vals.copy()
    b[C >= tcol0] = 0.0
    mutants["t columns dropped"] = b
    c = vals.copy()
    b3 = slice(int(E.block_off[3]), int(E.block_off[4]))      # pos / velocity: the diagonal scalar of every phase, 3n uses each
    s3 = src[b3]
    assert np.all(s3 >= 0)
    first = np.zeros(s3.size, dtype=bool)
    first[np.unique(s3, return_index=True)[1]] = True
    assert first.sum() == E.S and s3.size == 3 * E.N
    c[b3] = np.where(first, c[b3], 0.0)
    mutants["scalar used once"] = c
    for what, mv in mutants.items():
        ok_y, use_y, _ = jt.check(E, R, C, mv, v, y, False)
        ok_g, use_g, _ = jt.check(E, R, C, mv, lam, g, True)
        print("teeth %s / %s: bound missed by %.2e (J v) %.2e (J^T lambda)" % (name, what, use_y, use_g))
        assert not ok_y and use_y > 1e6, (name, what, use_y)
        assert not ok_g and use_g > 1e6, (name, what, use_g)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("name", NAMES)
def test_info_equals_pattern_counts(name, flags):
    E, R, C, _ = _case(name, flags)
    src, cv = E.full_source(), E.const_values()
    nz = jt.structural_nonzero(E)
    info = E.jac_products_info()
    assert info["const_nnz"] == int(((src == -1) & (cv != 0.0)).sum())
    assert info["var_entries"] == int((src != -1).sum())
    assert info["max_row_nnz"] == int(np.bincount(R[nz], minlength=E.nres).max())
    assert info["max_col_nnz"] == int(np.bincount(C[nz], minlength=E.nvars).max())
    if flags == 0 and name == "mixed-6x64":
        assert (info["const_nnz"], info["max_col_nnz"]) == (237952, 1408)
    if flags == 0 and name == "stress-12x128":
        assert info["max_col_nnz"] == 2816


def test_host_product_reports_nonfinite():
    E, R, C, jvar = _case("example", 0)
    v, lam = _inputs(E, 3)
    bad = jvar.copy()
    bad[E.V // 2] = np.nan
    JV = np.stack([jvar, bad])
    Y, rc = E.jac_products_host(JV, np.stack([v, v]))
    assert rc == 1 and np.isnan(Y[1]).any() and np.array_equal(Y[0], E.jac_products_host(jvar, v)[0])


def test_argument_errors():
    import ctypes as C_
    from gelato_amd import _lib
    E, R, C, jvar = _case("example", 0)
    L = _lib.lib()
    dp = C_.POINTER(C_.c_double)
    v, lam = _inputs(E, 1)
    y, g = np.zeros(E.nres), np.zeros(E.nvars)
    p = lambda a: a.ctypes.data_as(dp)   # noqa: E731
    null = dp()
    assert L.gel_jac_products_host(E._h, 0, p(jvar), p(v), p(y), 0) == -1
    assert L.gel_jac_products_host(E._h, -3, p(jvar), p(v), p(y), 1) == -1
    assert L.gel_jac_products_host(E._h, 1, null, p(v), p(y), 0) == -1
    assert L.gel_jac_products_host(E._h, 1, p(jvar), null, p(y), 0) == -1
    assert L.gel_jac_products_host(E._h, 1, p(jvar), p(v), null, 0) == -1
    assert L.gel_jac_products_host(None, 1, p(jvar), p(v), p(y), 0) == -1
    assert L.gel_jac_products_info(E._h, None) == -1 and L.gel_jac_products_info(None, (C_.c_int64 * 4)()) == -1
    assert L.gel_last_error()
    # the evaluating entry points refuse a host-only handle (and say why), before they touch a buffer
    for fn, a, b in ((L.gel_jac_matvec, v, y), (L.gel_jac_rmatvec, lam, g)):
        assert fn(E._h, 1, p(jvar), p(a), p(b)) == -1
        assert b"host-only" in L.gel_last_error()
        assert fn(E._h, 0, p(jvar), p(a), p(b)) == -1 and fn(E._h, 1, null, p(a), p(b)) == -1
    one = C_.c_void_p(8)   # never dereferenced: the handle is refused first
    for fn in (L.gel_jac_matvec_device, L.gel_jac_rmatvec_device):
        assert fn(E._h, 1, one, one, one, None) == -1
        assert b"host-only" in L.gel_last_error()
        assert fn(E._h, 0, one, one, one, None) == -1 and fn(E._h, 1, None, one, one, None) == -1
    with pytest.raises(_lib.GelatoAmdError):
        E.jac_matvec(jvar, v)
    with pytest.raises(ValueError):
        E.jac_products_host(jvar, lam)   # lambda where v is expected

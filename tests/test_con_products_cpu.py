"""Products with K, the Jacobian of every row that is not a defect row, host side (no GPU): gel_con_products_host on host-only
handles against a reference built from the row lists, Engine.aero_pattern and the record map (tests/con_products_truth.py) under
the derived bound; the whole matrix recovered from unit vectors; dense = record form; the accumulate rule; the unread jfn column;
the counts; every refusal; a reconfiguration."""
import ctypes as C_

import numpy as np
import pytest

import con_products_truth as ct
import jac_products_truth as jt

CASES = ["example-full", "example-aero-initial", "ragged"]
_CACHE = {}


def _case(name, flags=0):
    """(engine, truth) of a configuration on a host-only handle"""
    key = (name, flags)
    if key not in _CACHE:
        from gelato_amd import Engine
        import stream_cases as SC
        prob, _x0 = jt.named("ragged" if name == "ragged" else "example")
        E = Engine(prob, device=-1, flags=flags)
        if name == "example-full":
            lin, fn = ct.example_full_tables()
            T = ct.configure(E, lin, fn, ct.aero_all_specs(E))
        elif name == "example-aero-initial":
            lin, fn = ct.small_tables(E)
            E.rows_configure(lin, fn)
            SC.CONFIGS["aero_initial"](E)          # part A empty, kind q absent
            T = ct.Truth(E, lin, fn)
            assert T.nrows["q"] == 0 and T.nrows["alpha"] > 0
        else:
            lin, fn = ct.small_tables(E)
            T = ct.configure(E, lin, fn, ct.aero_all_specs(E))
        _CACHE[key] = (E, T)
    return _CACHE[key]


@pytest.mark.parametrize("flags", [0, 8])
@pytest.mark.parametrize("name", CASES)
def test_host_products_within_bound(name, flags):
    """both products, both source forms, B = 3, random finite values (the operator is linear in them)"""
    E, T = _case(name, flags)
    B = 3
    jfn, jac, rec = ct.random_values(T, B, 20261018 + flags)
    rng = np.random.default_rng(7 + flags)
    V, Lam = rng.standard_normal((B, E.nvars)), rng.standard_normal((B, T.R))
    use = [0.0, 0.0]
    for form in ("dense", "record"):
        kw = dict(jfn=jfn, aero_jac=jac) if form == "dense" else dict(jfn=jfn, aero_record=rec)
        Y, rc = E.con_products_host(V, **kw)
        G, rc2 = E.con_products_host(Lam, transpose=True, **kw)
        assert rc == 0 and rc2 == 0 and Y.shape == (B, T.R) and G.shape == (B, E.nvars)
        for b in range(B):
            tk = dict(jfn=None if jfn is None else jfn[b])
            if form == "dense":
                tk["aero_jac"] = {k: v[b] for k, v in jac.items()} if jac else None
            else:
                tk["aero_record"] = rec[b]
            R, C, vals = T.triplets(**tk)
            for t, (inp, got) in enumerate(((V[b], Y[b]), (Lam[b], G[b]))):
                ok, share, worst = ct.check(T, R, C, vals, inp, got, bool(t))
                use[t] = max(use[t], share)
                assert ok, (name, flags, form, b, "K^T lambda" if t else "K v", share, worst)
    print("bound usage %s flags %d: K v %.3f  K^T lambda %.3f" % (name, flags, use[0], use[1]))


@pytest.mark.parametrize("flags", [0, 8])
@pytest.mark.parametrize("name", CASES)
def test_whole_matrix_recovery(name, flags):
    """B = num_vars unit vectors through K v and B = R unit vectors through K^T lambda, one vector's values tiled: the outputs are
    the truth's dense K, element for element -- every entry's place and sign"""
    E, T = _case(name, flags)
    jfn, jac, rec = ct.random_values(T, 1, 99 + flags)
    R, C, vals = T.triplets(jfn=None if jfn is None else jfn[0], aero_jac={k: v[0] for k, v in jac.items()} if jac else None)
    K = T.dense(R, C, vals)
    for form in ("dense", "record"):
        for transpose, n in ((False, E.nvars), (True, T.R)):
            kw = {"jfn": None if jfn is None else np.tile(jfn, (n, 1, 1))}
            if form == "dense":
                kw["aero_jac"] = {k: np.tile(v, (n, 1)) for k, v in jac.items()} if jac else None
            else:
                kw["aero_record"] = None if rec is None else np.tile(rec, (n, 1))
            out, rc = E.con_products_host(np.eye(n), transpose=transpose, **kw)
            assert rc == 0
            want = K if transpose else K.T          # row i of the output: K^T e_i = row i of K; K e_j = column j of K
            assert np.array_equal(out, want), (name, flags, form, transpose, np.argwhere(out != want)[:5])
    assert int(np.count_nonzero(K)) > 0


@pytest.mark.parametrize("name", CASES)
def test_dense_and_record_forms_give_equal_bits_and_batches_equal_singles(name):
    E, T = _case(name)
    B = 3
    jfn, jac, rec = ct.random_values(T, B, 5)
    rng = np.random.default_rng(6)
    for transpose, inp in ((False, rng.standard_normal((B, E.nvars))), (True, rng.standard_normal((B, T.R)))):
        a, rc = E.con_products_host(inp, jfn=jfn, aero_jac=jac, transpose=transpose)
        b, rc2 = E.con_products_host(inp, jfn=jfn, aero_record=rec, transpose=transpose)
        assert rc == 0 and rc2 == 0 and np.array_equal(a.view(np.int64), b.view(np.int64))
        for k in range(B):
            one, _ = E.con_products_host(inp[k], jfn=None if jfn is None else jfn[k],
                                         aero_jac={q: v[k] for q, v in jac.items()} if jac else None, transpose=transpose)
            assert np.array_equal(one.view(np.int64), a[k].view(np.int64))


@pytest.mark.parametrize("name", CASES)
def test_accumulate_is_g_in_plus_s_bit_for_bit(name):
    E, T = _case(name)
    B = 3
    jfn, jac, rec = ct.random_values(T, B, 11)
    rng = np.random.default_rng(12)
    Lam, g_in = rng.standard_normal((B, T.R)), rng.standard_normal((B, E.nvars))
    s, rc = E.con_products_host(Lam, jfn=jfn, aero_record=rec, transpose=True)
    g = g_in.copy()
    out, rc2 = E.con_products_host(Lam, jfn=jfn, aero_record=rec, transpose=True, out=g)
    assert rc == 0 and rc2 == 0 and out is g
    assert np.array_equal(g.view(np.int64), (g_in + s).view(np.int64))
    # a column without an entry gets +0.0
    _R, C, _v = T.triplets(jfn=None if jfn is None else jfn[0], aero_record=rec[0])
    empty = np.bincount(C, minlength=E.nvars) == 0
    assert empty.any() and np.all(s[:, empty] == 0.0) and not np.any(np.signbit(s[:, empty]))


def test_nan_in_unread_jfn_column_reaches_no_output():
    """jfn[r][6] of a row with tcol < 0 is not an entry of K"""
    E, T = _case("example-full")
    lin, fn = ct.example_full_tables()
    no_t = [r for r, row in enumerate(fn) if len(row) == 4 or row[2] < 0]
    assert no_t and len(no_t) < len(fn)
    jfn, jac, rec = ct.random_values(T, 2, 21)
    bad = jfn.copy()
    bad[:, no_t, 6] = np.nan
    rng = np.random.default_rng(22)
    for transpose, inp in ((False, rng.standard_normal((2, E.nvars))), (True, rng.standard_normal((2, T.R)))):
        a, rc = E.con_products_host(inp, jfn=jfn, aero_jac=jac, transpose=transpose)
        b, rc2 = E.con_products_host(inp, jfn=bad, aero_jac=jac, transpose=transpose)
        assert rc == 0 and rc2 == 0 and np.array_equal(a.view(np.int64), b.view(np.int64))
    # a NaN in a column that IS read stays in its vector and is reported
    bad = jfn.copy()
    bad[1, no_t[0], 0] = np.nan
    y, rc = E.con_products_host(rng.standard_normal((2, E.nvars)), jfn=bad, aero_jac=jac)
    assert rc == 1 and np.isnan(y[1]).any() and not np.isnan(y[0]).any()


@pytest.mark.parametrize("flags", [0, 8])
@pytest.mark.parametrize("name", CASES)
def test_dims(name, flags):
    E, T = _case(name, flags)
    jfn, jac, rec = ct.random_values(T, 1, 1)
    R, C, _v = T.triplets(jfn=None if jfn is None else jfn[0], aero_jac={k: v[0] for k, v in jac.items()} if jac else None)
    d = E.con_products_dims()
    assert (d["R"], d["nlin"], d["nfn"]) == (T.R, T.nlin, T.nfn)
    assert [d[k] for k in ct.KINDS] == [T.nrows[k] for k in ct.KINDS]
    assert d["entries"] == R.size
    assert d["max_row_entries"] == int(np.bincount(R, minlength=T.R).max())
    assert d["max_col_entries"] == int(np.bincount(C, minlength=E.nvars).max())
    if name == "example-full":
        # the t0 / tf columns of part A are stored (and entries) only with GEL_FLAG_FD_RECOMPUTE
        dropped = sum(int((T.rec_idx[k] < 0).sum()) for k in ct.KINDS)
        assert (dropped > 0) == (flags == 0)


def test_refusals():
    from gelato_amd import Engine, _lib
    E, T = _case("example-full")
    L = _lib.lib()
    dp = C_.POINTER(C_.c_double)
    p = lambda a: a.ctypes.data_as(dp)   # noqa: E731
    jfn, jac, rec = ct.random_values(T, 1, 3)
    v, lam, y, g = np.zeros(E.nvars), np.zeros(T.R), np.zeros(T.R), np.zeros(E.nvars)
    ja = (dp * 3)(*[p(jac[k]) for k in ct.KINDS])
    host = L.gel_con_products_host
    assert host(E._h, 1, p(jfn), ja, None, p(v), p(y), 0, 0) == 0
    assert host(E._h, 1, p(jfn), None, p(rec), p(lam), p(g), 1, 0) == 0
    assert host(E._h, 0, p(jfn), ja, None, p(v), p(y), 0, 0) == -1                  # B < 1
    assert host(None, 1, p(jfn), ja, None, p(v), p(y), 0, 0) == -1
    assert host(E._h, 1, p(jfn), ja, None, None, p(y), 0, 0) == -1 and host(E._h, 1, p(jfn), ja, None, p(v), None, 0, 0) == -1
    assert host(E._h, 1, None, ja, None, p(v), p(y), 0, 0) == -1                    # jfn NULL with nfn > 0
    assert host(E._h, 1, p(jfn), ja, p(rec), p(v), p(y), 0, 0) == -1                # both sources
    assert host(E._h, 1, p(jfn), None, None, p(v), p(y), 0, 0) == -1                # neither
    hole = (dp * 3)(p(jac["alpha"]), None, p(jac["qalpha"]))
    assert host(E._h, 1, p(jfn), hole, None, p(v), p(y), 0, 0) == -1                # a kind with rows is NULL
    assert L.gel_last_error()
    assert L.gel_con_products_dims(E._h, None) == -1 and L.gel_con_products_dims(None, (C_.c_int64 * 9)()) == -1
    # the evaluating entry points refuse a host-only handle (and say why)
    assert L.gel_con_matvec(E._h, 1, p(jfn), ja, None, p(v), p(y)) == -1 and b"host-only" in L.gel_last_error()
    assert L.gel_con_rmatvec(E._h, 1, p(jfn), ja, None, p(lam), p(g), 0) == -1 and b"host-only" in L.gel_last_error()
    one = C_.c_void_p(8)   # never dereferenced: the handle is refused first
    jd = (C_.c_void_p * 3)(8, 8, 8)
    assert L.gel_con_matvec_device(E._h, 1, one, jd, None, one, one) == -1 and b"host-only" in L.gel_last_error()
    assert L.gel_con_rmatvec_device(E._h, 1, one, jd, None, one, one, 1) == -1 and b"host-only" in L.gel_last_error()
    assert L.gel_con_matvec_device(E._h, 1, one, jd, one, one, one) == -1 and L.gel_con_matvec_device(E._h, 0, one, jd, None, one, one) == -1
    # nothing configured: R = 0
    prob, _x0 = jt.named("example")
    E0 = Engine(prob, device=-1)
    assert E0.con_products_dims()["R"] == 0
    assert host(E0._h, 1, None, None, None, p(v), p(y), 0, 0) == -1
    # no aero kind has rows: both sources must be NULL; a kind without rows may be NULL inside aero_jac
    lin, fn = ct.small_tables(E0)
    E0.rows_configure(lin, [])
    y0 = np.zeros(len(lin))
    assert host(E0._h, 1, None, None, None, p(v), p(y0), 0, 0) == 0                 # jfn may be NULL when nfn = 0
    assert host(E0._h, 1, None, ja, None, p(v), p(y0), 0, 0) == -1 and host(E0._h, 1, None, None, p(rec), p(v), p(y0), 0, 0) == -1
    E0.aero_configure("q", [(0, 1, 4.0e4)])
    jq = np.zeros(sum(E0.aero_dims("q")[1]))
    yq = np.zeros(E0.con_products_dims()["R"])
    assert host(E0._h, 1, None, (dp * 3)(None, p(jq), None), None, p(v), p(yq), 0, 0) == 0
    with pytest.raises(ValueError):
        E.con_products_host(lam, jfn=jfn[0], aero_jac={k: a[0] for k, a in jac.items()})    # lambda where v is expected
    with pytest.raises(_lib.GelatoAmdError):
        E.con_matvec(v, jfn=jfn[0], aero_jac={k: a[0] for k, a in jac.items()})


def test_reconfiguration_and_failed_configure():
    """after a reconfiguration with fewer rows the products follow the new table; a configure call that fails leaves the old
    operator in place"""
    from gelato_amd import Engine, _lib
    prob, _x0 = jt.named("example")
    E = Engine(prob, device=-1)
    lin, fn = ct.example_full_tables()
    T1 = ct.configure(E, lin, fn, ct.aero_all_specs(E))
    lin2, fn2 = lin[:5], fn[:3]
    aero2 = {"alpha": [(0, 1, 0.2)], "qalpha": [(1, 0, 5.0e3)]}
    T2 = ct.configure(E, lin2, fn2, aero2)
    assert T2.R < T1.R and E.con_products_dims()["R"] == T2.R
    jfn, jac, rec = ct.random_values(T2, 1, 31)
    R, C, vals = T2.triplets(jfn=jfn[0], aero_record=rec[0])
    K = T2.dense(R, C, vals)
    out, rc = E.con_products_host(np.eye(T2.R), jfn=np.tile(jfn, (T2.R, 1, 1)), aero_record=np.tile(rec, (T2.R, 1)), transpose=True)
    assert rc == 0 and np.array_equal(out, K)
    before = E.con_products_dims()
    with pytest.raises(_lib.GelatoAmdError):
        E.aero_configure("q", [(E.S - 1, 1, 4.0e4)])      # the last phase is never constrained
    with pytest.raises(_lib.GelatoAmdError):
        E.rows_configure([(E.nvars, 1.0, -1, 0.0, 0.0)], [])
    assert E.con_products_dims() == before
    out2, rc = E.con_products_host(np.eye(T2.R), jfn=np.tile(jfn, (T2.R, 1, 1)), aero_record=np.tile(rec, (T2.R, 1)), transpose=True)
    assert rc == 0 and np.array_equal(out2, K)

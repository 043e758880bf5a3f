"""Products with K, the Jacobian of every row that is not a defect row, on the device (gel_con_matvec*, gel_con_rmatvec*;
DESIGN.md 3.15): values from real evaluations (gel_rows_eval, gel_eval_aero_all, gel_eval_batch_aero_device), both products and
both source forms against the reference of tests/con_products_truth.py under the derived bound; the adjoint identity; the whole
matrix from unit vectors; bit identities; status; and the record form at B = 65,536, where the record buffer passes 2^32 bytes.

Largest share of the bound used, measured on an MI355X (printed by test_products_within_bound): see DESIGN.md 3.15."""
import gc

import numpy as np
import pytest

import con_products_truth as ct
import jac_products_truth as jt
import size_forms as SF

pytestmark = pytest.mark.gpu
LD = jt.LD
NAMES = ["example-everything", "ragged", "mixed-6x64"]
FLAGS = [0, 8, 64 | 128]   # default, GEL_FLAG_FD_RECOMPUTE (time columns stored), exact aero gradients and exact jfn
_CACHE = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _buf(shape, fill=SF.POISON):
    import torch
    return torch.full(tuple(shape), fill, dtype=torch.float64, device="cuda")


def _engine(name, flags=0):
    """(engine, truth, x0) of a configured device handle; only the last one is kept alive"""
    key = (name, flags)
    if _CACHE.get("key") != key:
        _CACHE.clear()
        gc.collect()
        from gelato_amd import Engine
        prob, x0 = jt.named("example" if name == "example-everything" else name)
        E = Engine(prob, flags=flags)
        lin, fn = ct.example_full_tables() if name == "example-everything" else ct.small_tables(E)
        T = ct.configure(E, lin, fn, ct.aero_all_specs(E))
        _CACHE.update(key=key, E=E, T=T, x0=x0)
    return _CACHE["E"], _CACHE["T"], _CACHE["x0"]


def _values(E, T, X):
    """one real evaluation of X [B, nvars] -> (jfn [B, nfn, 7], aero_jac {kind: [B, sum nnz]}, record [B, width]): the row table
    and the dense arrays through the host-buffer calls, the records from gel_eval_batch_aero_device"""
    B = X.shape[0]
    _con, jfn, rc = E.rows_eval(X)
    assert rc == 0
    _c, jac, rc = E.eval_aero_all(X)
    assert rc == 0
    dX, dres, djv, drec = _up(X), _buf((B, E.nres)), _buf((B, max(E.V, 1))), _buf((B, T.width))
    E.eval_batch_aero_device(B, dX.data_ptr(), dres.data_ptr(), djv.data_ptr(), drec.data_ptr())
    assert E.sync() == 0
    return jfn, jac, drec.cpu().numpy()


def _device(E, T, V, Lam, jfn, jac=None, rec=None, g_in=None):
    """both device forms on torch buffers -> (y, g, status); g_in: accumulate into it"""
    B = V.shape[0]
    dj = _up(jfn) if jfn is not None else None
    da = [_up(jac[k]) if k in jac else None for k in ct.KINDS] if jac is not None else None
    dr = _up(rec) if rec is not None else None
    dv, dl = _up(V), _up(Lam)
    dy = _buf((B, T.R))                                             # every element must be overwritten
    dg = _up(g_in) if g_in is not None else _buf((B, E.nvars))
    ap = [a.data_ptr() if a is not None else 0 for a in da] if da is not None else None
    E.con_matvec_device(B, dj.data_ptr() if dj is not None else 0, ap, dr.data_ptr() if dr is not None else 0, dv.data_ptr(), dy.data_ptr())
    E.con_rmatvec_device(B, dj.data_ptr() if dj is not None else 0, ap, dr.data_ptr() if dr is not None else 0, dl.data_ptr(), dg.data_ptr(),
                         accumulate=g_in is not None)
    rc = E.sync()
    return dy.cpu().numpy(), dg.cpu().numpy(), rc


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("name", NAMES)
def test_products_within_bound(name, flags):
    """every row and every column of both products, both source forms, B = 3, and the adjoint identity
    |lambda^T (K v) - (K^T lambda)^T v| <= sum |lambda_i| bound_y,i + sum |v_j| bound_g,j"""
    from gelato_amd import problem
    E, T, x0 = _engine(name, flags)
    B = 3
    X = problem.synthetic_batch(x0, E.M, B)
    jfn, jac, rec = _values(E, T, X)
    if name == "mixed-6x64":
        d = E.con_products_dims()
        assert (d["alpha"], d["q"], d["qalpha"]) == (325, 325, 325)      # 5 phases x 65 state nodes: 320 of them in part A
    rng = np.random.default_rng(20261018 + flags)
    V, Lam = rng.standard_normal((B, E.nvars)), rng.standard_normal((B, T.R))
    use = [0.0, 0.0, 0.0]
    for form in ("dense", "record"):
        y, g, rc = _device(E, T, V, Lam, jfn, jac=jac if form == "dense" else None, rec=rec if form == "record" else None)
        assert rc == 0
        for b in range(B):
            if form == "dense":
                R, C, vals = T.triplets(jfn=jfn[b], aero_jac={k: v[b] for k, v in jac.items()})
            else:
                R, C, vals = T.triplets(jfn=jfn[b], aero_record=rec[b])
            for t, (inp, got) in enumerate(((V[b], y[b]), (Lam[b], g[b]))):
                ok, share, worst = ct.check(T, R, C, vals, inp, got, bool(t))
                use[t] = max(use[t], share)
                assert ok, (name, flags, form, b, "K^T lambda" if t else "K v", share, worst)
            _ry, mag_y, m_y = ct.products(T, R, C, vals, V[b], False)
            _rg, mag_g, m_g = ct.products(T, R, C, vals, Lam[b], True)
            lhs = np.sum(Lam[b].astype(LD) * y[b].astype(LD)) - np.sum(g[b].astype(LD) * V[b].astype(LD))
            rhs = np.sum(np.abs(Lam[b]).astype(LD) * jt.bound(mag_y, m_y)) + np.sum(np.abs(V[b]).astype(LD) * jt.bound(mag_g, m_g))
            assert abs(lhs) <= rhs, (name, flags, form, b, float(lhs), float(rhs))
            use[2] = max(use[2], float(abs(lhs) / rhs))
    print("bound usage %s flags %d: K v %.3f  K^T lambda %.3f  adjoint identity %.3f" % (name, flags, use[0], use[1], use[2]))


def test_whole_matrix_recovery_on_the_device():
    """the example: num_vars unit vectors through K v and R unit vectors through K^T lambda, one vector's values tiled -> the
    truth's dense K, element for element, in both source forms"""
    from gelato_amd import problem
    E, T, x0 = _engine("example-everything", 0)
    jfn, jac, rec = _values(E, T, problem.synthetic_batch(x0, E.M, 2)[1:])
    R, C, vals = T.triplets(jfn=jfn[0], aero_jac={k: v[0] for k, v in jac.items()})
    K = T.dense(R, C, vals)
    for form in ("dense", "record"):
        for transpose, n in ((False, E.nvars), (True, T.R)):
            kw = {"jfn": np.tile(jfn, (n, 1, 1))}
            if form == "dense":
                kw["aero_jac"] = {k: np.tile(v, (n, 1)) for k, v in jac.items()}
            else:
                kw["aero_record"] = np.tile(rec, (n, 1))
            out, rc = (E.con_rmatvec if transpose else E.con_matvec)(np.eye(n), **kw)
            assert rc == 0
            want = K if transpose else K.T
            assert np.array_equal(out, want), (form, transpose, np.argwhere(out != want)[:5])


@pytest.mark.parametrize("name", NAMES)
def test_bit_identity(name):
    """device = host form; dense = record; B = 1 = the same vector at positions 0, 4 and 36 of B = 37; a repeat into poisoned
    buffers; the accumulate rule; the host-buffer wrappers"""
    from gelato_amd import problem
    E, T, x0 = _engine(name, 0)
    B = 37
    X = problem.synthetic_batch(x0, E.M, B)
    X[4], X[36] = X[0], X[0]
    jfn, jac, rec = _values(E, T, X)
    rng = np.random.default_rng(37)
    V, Lam = rng.standard_normal((B, E.nvars)), rng.standard_normal((B, T.R))
    for k in (4, 36):
        V[k], Lam[k] = V[0], Lam[0]
    y, g, rc = _device(E, T, V, Lam, jfn, jac=jac)
    assert rc == 0
    yr, gr, rc = _device(E, T, V, Lam, jfn, rec=rec)
    assert rc == 0 and np.array_equal(_bits(y), _bits(yr)) and np.array_equal(_bits(g), _bits(gr))       # dense = record
    y2, g2, rc = _device(E, T, V, Lam, jfn, rec=rec)
    assert rc == 0 and np.array_equal(_bits(y2), _bits(y)) and np.array_equal(_bits(g2), _bits(g))       # repeat, poisoned buffers
    yh, rc1 = E.con_products_host(V, jfn=jfn, aero_jac=jac)
    gh, rc2 = E.con_products_host(Lam, jfn=jfn, aero_record=rec, transpose=True)
    assert rc1 == 0 and rc2 == 0 and np.array_equal(_bits(y), _bits(yh)) and np.array_equal(_bits(g), _bits(gh))   # device = host form
    y1, g1, rc = _device(E, T, V[:1], Lam[:1], jfn[:1], jac={k: v[:1] for k, v in jac.items()})
    assert rc == 0
    for k in (0, 4, 36):
        assert np.array_equal(_bits(y[k]), _bits(y1[0])) and np.array_equal(_bits(g[k]), _bits(g1[0])), (name, k)
    g_in = rng.standard_normal((B, E.nvars))
    _y, ga, rc = _device(E, T, V, Lam, jfn, rec=rec, g_in=g_in)
    assert rc == 0 and np.array_equal(_bits(ga), _bits(g_in + g))                                        # accumulate
    yw, rc1 = E.con_matvec(V, jfn=jfn, aero_record=rec)
    gw, rc2 = E.con_rmatvec(Lam, jfn=jfn, aero_jac=jac, out=g_in.copy())
    assert rc1 == 0 and rc2 == 0 and np.array_equal(_bits(yw), _bits(y)) and np.array_equal(_bits(gw), _bits(g_in + g))


def test_constraint_operator_is_the_two_call_sum():
    """ConstraintOperator over all rows [defect 11N | K's R]: rmatvec = J^T lambda_defect + K^T lambda_other bit for bit, matvec
    = the two products side by side; for_vector gives the same rows"""
    from gelato_amd import problem
    from gelato_amd.products import ConstraintOperator
    E, T, x0 = _engine("example-everything", 0)
    B = 3
    X = problem.synthetic_batch(x0, E.M, B)
    A = ConstraintOperator(E, X)
    assert A.status == 0 and A.shape == (E.nres + T.R, E.nvars)
    sl = A.row_slices
    assert sl["mass"] == slice(0, E.N) and sl["quat"].stop == E.nres and sl["linear"] == slice(E.nres, E.nres + T.nlin)
    assert sl["qalpha"].stop == E.nres + T.R and sl["nodefn"].stop - sl["nodefn"].start == T.nfn
    res, jv, rc = E.eval_batch(X)
    jfn, jac, _rec = _values(E, T, X)
    con, _j, _rc = E.rows_eval(X)
    assert np.array_equal(A.res, res) and np.array_equal(A.con[:, :T.nlin + T.nfn], con)
    rng = np.random.default_rng(3)
    V, Lam = rng.standard_normal((B, E.nvars)), rng.standard_normal((B, E.nres + T.R))
    g0, _ = E.jac_rmatvec(jv, Lam[:, :E.nres])
    g1, _ = E.con_rmatvec(Lam[:, E.nres:], jfn=jfn, aero_jac=jac)
    g = A.rmatvec(Lam)
    assert A.last_status == 0 and np.array_equal(_bits(g), _bits(g0 + g1))
    y = A.matvec(V)
    assert np.array_equal(_bits(y[:, :E.nres]), _bits(E.jac_matvec(jv, V)[0]))
    assert np.array_equal(_bits(y[:, E.nres:]), _bits(E.con_matvec(V, jfn=jfn, aero_jac=jac)[0]))
    op = A.for_vector(1)
    assert op.shape == A.shape and np.array_equal(op.matvec(V[1]), y[1]) and np.array_equal(op.rmatvec(Lam[1]), g[1])


def test_nonfinite_status_and_isolation():
    """a NaN planted in vector 1 of 3 (one jfn value, one record value): GEL_NONFINITE from sync, vectors 0 and 2 keep their bits;
    the next call is clean again"""
    from gelato_amd import problem
    E, T, x0 = _engine("mixed-6x64", 0)
    X = problem.synthetic_batch(x0, E.M, 3)
    jfn, jac, rec = _values(E, T, X)
    rng = np.random.default_rng(4)
    V, Lam = rng.standard_normal((3, E.nvars)), rng.standard_normal((3, T.R))
    y0, g0, rc = _device(E, T, V, Lam, jfn, rec=rec)
    assert rc == 0
    badj, badr = jfn.copy(), rec.copy()
    badj[1, 0, 0] = np.nan
    idx = T.rec_idx["q"]
    badr[1, idx[idx >= 0][7]] = np.nan
    for kw in (dict(jfn=badj, rec=rec), dict(jfn=jfn, rec=badr)):
        y, g, rc = _device(E, T, V, Lam, kw["jfn"], rec=kw["rec"])
        assert rc == 1 and np.isnan(y[1]).any() and np.isnan(g[1]).any()
        for b in (0, 2):
            assert np.array_equal(_bits(y[b]), _bits(y0[b])) and np.array_equal(_bits(g[b]), _bits(g0[b]))
    y, g, rc = _device(E, T, V, Lam, jfn, rec=rec)
    assert rc == 0 and np.array_equal(_bits(y), _bits(y0)) and np.array_equal(_bits(g), _bits(g0))


def test_device_argument_errors():
    from gelato_amd import _lib
    E, T, x0 = _engine("example-everything", 0)
    L = _lib.lib()
    import ctypes as C_
    jd = (C_.c_void_p * 3)(8, 8, 8)
    for fn, tail in ((L.gel_con_matvec_device, ()), (L.gel_con_rmatvec_device, (0,))):
        assert fn(E._h, 0, 8, jd, None, 8, 8, *tail) == -1                     # B < 1
        assert fn(E._h, 1, None, jd, None, 8, 8, *tail) == -1                  # jfn NULL, nfn > 0
        assert fn(E._h, 1, 8, jd, 8, 8, 8, *tail) == -1                        # both sources
        assert fn(E._h, 1, 8, None, None, 8, 8, *tail) == -1                   # neither
        assert fn(E._h, 1, 8, jd, None, None, 8, *tail) == -1 and fn(E._h, 1, 8, jd, None, 8, None, *tail) == -1
        assert L.gel_last_error()


def test_record_form_at_full_size():
    """mixed-6x64, record form, B = 65,536: the record buffer passes 2^32 bytes.  256 distinct vectors tiled; every block of 256
    output rows equals the B = 256 call bit for bit; a call of B - 5 vectors leaves the rows behind it untouched; one planted bit
    is reported at exactly its cell (size_forms.check_blocks).  Peak memory: records 6.1 GB, v and g 2.7 GB each, lambda and y
    0.5 GB each, jfn: 12.5 GB."""
    import torch
    from gelato_amd import problem
    E, T, x0 = _engine("mixed-6x64", 0)
    B, P = 65536, SF.P
    need = 8 * B * (T.width + 2 * E.nvars + 2 * T.R + 7 * T.nfn) + (2 << 30)
    assert need <= SF.LIMIT_BYTES and 8 * (B - 5) * T.width > 2 ** 32
    gc.collect()
    torch.cuda.empty_cache()
    if torch.cuda.mem_get_info()[0] < need:
        pytest.skip("needs %.1f GB of device memory" % (need / 1e9))
    X = problem.synthetic_batch(x0, E.M, P, seed=3)
    jfn, _jac, rec = _values(E, T, X)
    rng = np.random.default_rng(7)
    V, Lam = rng.standard_normal((P, E.nvars)), rng.standard_normal((P, T.R))
    rj, rr, rv, rl = _up(jfn.reshape(P, -1)), _up(rec), _up(V), _up(Lam)
    ry, rg = _buf((P, T.R)), _buf((P, E.nvars))

    def call(Bt, dj, dr, dv, dl, dy, dg):
        E.con_matvec_device(Bt, dj.data_ptr(), None, dr.data_ptr(), dv.data_ptr(), dy.data_ptr())
        E.con_rmatvec_device(Bt, dj.data_ptr(), None, dr.data_ptr(), dl.data_ptr(), dg.data_ptr())
        return E.sync()
    assert call(P, rj, rr, rv, rl, ry, rg) == 0
    assert bool(torch.isfinite(ry).all()) and bool(torch.isfinite(rg).all())
    tiled = lambda r: r.repeat(B // P, 1).contiguous()   # noqa: E731
    dj, dr, dv, dl = tiled(rj), tiled(rr), tiled(rv), tiled(rl)
    dy, dg = _buf((B, T.R)), _buf((B, E.nvars))
    for turn, Bt in enumerate((B, B - 5)):
        dy.fill_(SF.POISON)
        dg.fill_(SF.POISON)
        assert call(Bt, dj, dr, dv, dl, dy, dg) == 0
        assert Bt == B or (bool((dy[Bt:] == SF.POISON).all()) and bool((dg[Bt:] == SF.POISON).all()))   # rows behind B - 5 untouched
        SF.check_blocks(dy[:Bt], ry, "K v B %d" % Bt, teeth=(turn == 0))
        SF.check_blocks(dg[:Bt], rg, "K^T lambda B %d" % Bt, teeth=(turn == 0))

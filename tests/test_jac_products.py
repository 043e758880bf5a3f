"""Jacobian products from the compact values on the device (gel_jac_matvec*, gel_jac_rmatvec*): both device forms
and both host-buffer forms against a reference built from the pattern, the constant template and the gather map
(tests/jac_products_truth.py) under the derived bound; unit inputs; the adjoint identity; bit-identity; status; merit_gradient.

Largest share of the bound used, measured on an MI355X (printed by test_products_within_bound; four problems x flags 0 / 8 / 32,
B = 3): see DESIGN.md 3.10."""
import numpy as np
import pytest

import jac_products_truth as jt

pytestmark = pytest.mark.gpu
NAMES = ["example", "mixed-6x64", "stress-12x128", "ragged"]
FLAGS = [0, 8, 32]   # default, GEL_FLAG_FD_RECOMPUTE, GEL_FLAG_EXACT_DEFECT_JAC
LD = jt.LD


def _setup(name, flags=0, B=3):
    from gelato_amd import Engine, problem
    prob, x0 = jt.named(name)
    E = Engine(prob, flags=flags)
    X = problem.synthetic_batch(x0, E.M, B)
    res, jv, rc = E.eval_batch(X)
    assert rc == 0
    return E, X, res, jv


def _device_products(E, jv, V, Lam):
    """both device forms on torch buffers -> (y, g, status)"""
    import torch
    B = jv.shape[0]
    dj, dv, dl = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (jv, V, Lam))
    dy = torch.full((B, E.nres), 7.0, dtype=torch.float64, device="cuda")       # every element must be overwritten
    dg = torch.full((B, E.nvars), 7.0, dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    E.jac_matvec_device(B, dj.data_ptr(), dv.data_ptr(), dy.data_ptr(), s)
    E.jac_rmatvec_device(B, dj.data_ptr(), dl.data_ptr(), dg.data_ptr(), s)
    rc = E.sync(s)
    return dy.cpu().numpy(), dg.cpu().numpy(), rc


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("name", NAMES)
def test_products_within_bound(name, flags):
    """every row and every column of both products, device and host-buffer forms, B = 3; and the adjoint identity
    |lambda^T (J v) - (J^T lambda)^T v| <= sum |lambda_i| bound_y,i + sum |v_j| bound_g,j on the device results"""
    E, X, _res, jv = _setup(name, flags)
    B = X.shape[0]
    rng = np.random.default_rng(20261016 + flags)
    V, Lam = rng.standard_normal((B, E.nvars)), rng.standard_normal((B, E.nres))
    yd, gd, rc = _device_products(E, jv, V, Lam)
    assert rc == 0
    yh, rc1 = E.jac_matvec(jv, V)
    gh, rc2 = E.jac_rmatvec(jv, Lam)
    assert rc1 == 0 and rc2 == 0
    assert np.array_equal(yd, yh) and np.array_equal(gd, gh)          # host-buffer form = device form, bit for bit
    R, C = jt.triplet_index(E)
    full = E.expand(jv)
    use = [0.0, 0.0, 0.0]
    for b in range(B):
        for t, (inp, got) in enumerate(((V[b], yd[b]), (Lam[b], gd[b]))):
            ok, share, worst = jt.check(E, R, C, full[b], inp, got, bool(t))
            use[t] = max(use[t], share)
            assert ok, (name, flags, b, "J^T lambda" if t else "J v", share, worst)
        _ry, mag_y, m_y = jt.products(E, R, C, full[b], V[b], False)
        _rg, mag_g, m_g = jt.products(E, R, C, full[b], Lam[b], True)
        lhs = np.sum(Lam[b].astype(LD) * yd[b].astype(LD)) - np.sum(gd[b].astype(LD) * V[b].astype(LD))
        rhs = np.sum(np.abs(Lam[b]).astype(LD) * jt.bound(mag_y, m_y)) + np.sum(np.abs(V[b]).astype(LD) * jt.bound(mag_g, m_g))
        assert abs(lhs) <= rhs, (name, flags, b, float(lhs), float(rhs))
        use[2] = max(use[2], float(abs(lhs) / rhs))
    print("bound usage %s flags %d: J v %.3f  J^T lambda %.3f  adjoint identity %.3f" % (name, flags, use[0], use[1], use[2]))


@pytest.mark.parametrize("name", NAMES)
def test_unit_inputs(name):
    """v = e_j for every t column and for one u column of a hold-type phase: y is that column of J (exact zeros for the u column);
    lambda = e_i for the first and last row of every group: g is that row of J"""
    E, X, _res, jv = _setup(name, 0, B=1)
    R, C = jt.triplet_index(E)
    full = E.expand(jv)[0]
    nz = jt.structural_nonzero(E)
    tcol0 = E.var_offset("t")
    empty = np.nonzero(np.bincount(C[nz], minlength=E.nvars) == 0)[0]
    assert empty.size and np.all((empty >= E.var_offset("u")) & (empty < tcol0))
    cols = list(range(tcol0, tcol0 + E.S + 1)) + [int(empty[0])]
    V = np.zeros((len(cols), E.nvars))
    V[np.arange(len(cols)), cols] = 1.0
    Y, rc = E.jac_matvec(np.repeat(jv, len(cols), axis=0), V)
    assert rc == 0
    for k, j in enumerate(cols):
        ok, share, worst = jt.check(E, R, C, full, V[k], Y[k], False)
        assert ok, (name, "column", j, share, worst)
        sel = C == j
        col = np.zeros(E.nres)
        np.add.at(col, R[sel], full[sel])          # one entry per (row, column): no rounding
        assert np.array_equal(Y[k], col), (name, "column", j)
    assert np.all(Y[-1] == 0.0) and not np.any(np.signbit(Y[-1]))
    N = E.N
    rows = [0, N - 1, N, 4 * N - 1, 4 * N, 7 * N - 1, 7 * N, 11 * N - 1]
    Lam = np.zeros((len(rows), E.nres))
    Lam[np.arange(len(rows)), rows] = 1.0
    G, rc = E.jac_rmatvec(np.repeat(jv, len(rows), axis=0), Lam)
    assert rc == 0
    for k, i in enumerate(rows):
        ok, share, worst = jt.check(E, R, C, full, Lam[k], G[k], True)
        assert ok, (name, "row", i, share, worst)
        sel = R == i
        row = np.zeros(E.nvars)
        np.add.at(row, C[sel], full[sel])
        assert np.array_equal(G[k], row), (name, "row", i)


@pytest.mark.parametrize("name", ["example", "mixed-6x64", "ragged"])
def test_bit_identity(name):
    """the call repeated; vector 0 alone against vector 0 inside B = 37 and B = 1024; the operator against jac_matvec"""
    from gelato_amd import problem
    E, X, _res, jv3 = _setup(name, 0, B=3)
    prob, x0 = jt.named(name)
    rng = np.random.default_rng(99)
    v0, l0 = rng.standard_normal(E.nvars), rng.standard_normal(E.nres)
    y1, rc = E.jac_matvec(jv3[0], v0)
    g1, rc2 = E.jac_rmatvec(jv3[0], l0)
    assert rc == 0 and rc2 == 0
    for B in (37, 1024):
        XB = problem.synthetic_batch(x0, E.M, B)
        _r, jv, rc = E.eval_batch(XB, want_res=False)
        assert rc == 0 and np.array_equal(jv[0], jv3[0])
        V, Lam = rng.standard_normal((B, E.nvars)), rng.standard_normal((B, E.nres))
        V[0], Lam[0] = v0, l0
        y, g, rc = _device_products(E, jv, V, Lam)
        assert rc == 0
        y2, g2, rc = _device_products(E, jv, V, Lam)
        assert rc == 0 and np.array_equal(y, y2) and np.array_equal(g, g2)          # run to run
        assert np.array_equal(y[0], y1) and np.array_equal(g[0], g1), (name, B)      # alone = inside the batch
        # a vector in the middle of the batch, alone
        k = B // 2
        assert np.array_equal(E.jac_matvec(jv[k], V[k])[0], y[k]) and np.array_equal(E.jac_rmatvec(jv[k], Lam[k])[0], g[k])
    A = E.jac_operator(jv3[0])
    assert A.shape == (E.nres, E.nvars)
    assert np.array_equal(A.matvec(v0), y1) and np.array_equal(A.rmatvec(l0), g1)
    assert np.array_equal(A @ v0, y1) and np.array_equal(A.T @ l0, g1)


def test_nonfinite_status_and_isolation():
    """a NaN planted in one vector's jvar (an input value): GEL_NONFINITE from sync, NaN in that vector's outputs, the others'
    outputs bit-identical; the next call on the handle is clean again"""
    E, X, _res, jv = _setup("mixed-6x64", 0, B=11)
    B = X.shape[0]
    rng = np.random.default_rng(4)
    V, Lam = rng.standard_normal((B, E.nvars)), rng.standard_normal((B, E.nres))
    y0, g0, rc = _device_products(E, jv, V, Lam)
    assert rc == 0
    bad = jv.copy()
    bad[5, E.V // 3] = np.nan
    y, g, rc = _device_products(E, bad, V, Lam)
    assert rc == 1
    assert np.isnan(y[5]).any() and np.isnan(g[5]).any()
    keep = np.arange(B) != 5
    assert np.array_equal(y[keep], y0[keep]) and np.array_equal(g[keep], g0[keep])
    yh, rch = E.jac_matvec(bad, V)
    assert rch == 1 and np.array_equal(yh[keep], y0[keep])
    y2, g2, rc = _device_products(E, jv, V, Lam)
    assert rc == 0 and np.array_equal(y2, y0) and np.array_equal(g2, g0)


def test_device_argument_errors():
    from gelato_amd import _lib
    E, X, _res, jv = _setup("example", 0, B=1)
    L = _lib.lib()
    for fn in (L.gel_jac_matvec_device, L.gel_jac_rmatvec_device):
        assert fn(E._h, 0, 8, 8, 8, None) == -1
        assert fn(E._h, 1, None, 8, 8, None) == -1 and fn(E._h, 1, 8, None, 8, None) == -1 and fn(E._h, 1, 8, 8, None, None) == -1
        assert L.gel_last_error()
    with pytest.raises(ValueError):
        E.jac_matvec(jv, np.zeros(E.nres))


@pytest.mark.parametrize("name", ["example", "mixed-6x64"])
def test_merit_gradient(name):
    """g = J^T res bit for bit, phi = 1/2 ||res||^2, and g is a descent direction of phi: Armijo's condition
    phi(x - a g) <= phi(x) - 1e-4 a ||g||^2 holds for some a = 2^-k, k <= 40, for every vector"""
    E, X, res, jv = _setup(name, 0, B=8)
    phi, g, rc = E.merit_gradient(X)
    assert rc == 0
    gr, rc = E.jac_rmatvec(jv, res)
    assert rc == 0 and np.array_equal(g, gr)
    assert np.array_equal(phi, 0.5 * np.einsum("bi,bi->b", res, res))
    gg = np.einsum("bi,bi->b", g, g)
    assert np.all(gg > 0)
    met = np.full(X.shape[0], -1)
    for k in range(41):
        a = 2.0 ** -k
        todo = np.nonzero(met < 0)[0]
        if not todo.size:
            break
        r2, _j, rc = E.eval_batch(X[todo] - a * g[todo], want_jac=False)
        p2 = 0.5 * np.einsum("bi,bi->b", r2, r2)
        ok = np.isfinite(p2) & (p2 <= phi[todo] - 1e-4 * a * gg[todo])
        met[todo[ok]] = k
    print("Armijo %s: met at k = %s" % (name, met.tolist()))
    assert np.all(met >= 0), met

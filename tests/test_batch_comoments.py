"""gel_batch_comoments* on the GPU (include/gelato_amd.h) against the stated order restated exactly
(tests/comoment_truth.py comoments_exact): every comparison of C, mean and m2 is bit for bit.  Batch sizes on both sides of the
block, widths on both sides of the tiles gel_batch_comoments_info reports, both forms; strided views; the listwise exclusion;
independence of the form of the call, of the neighbouring columns, of the slab walk and of the call before; the example problem's
dispersed flight through montecarlo.flight_covariance."""
import ctypes as C
import os

import numpy as np
import pytest

import comoment_truth as ct
from gelato_amd import Engine, _lib

pytestmark = pytest.mark.gpu

_dp = C.POINTER(C.c_double)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def E():
    import interp_truth as it
    e = Engine(it.prob_of([3, 4]))
    yield e
    e.close()


@pytest.fixture(scope="module")
def tiles(E):
    i = E.batch_comoments_info(300, 5, 5)
    assert i["tile_a"] >= 2 and i["tile_b"] >= 2 and i["block"] == 256
    return i["tile_a"], i["tile_b"]


def data(B, W, seed):
    """[B, W] finite: levels and scales that differ from column to column, a slow drift so that the blocks' means differ"""
    rng = np.random.default_rng(100 * seed + 7 * B + W)
    lev = rng.choice(np.array([0.0, 1.0, -30.0, 1e3, -1e-3]), W)
    sc = rng.choice(np.array([1.0, 1e-2, 40.0]), W)
    return np.ascontiguousarray(rng.standard_normal((B, W)) * sc + lev + 0.003 * np.arange(B)[:, None] * sc)


def raw(E, B, va, vb=None, want_stats=True):
    """the host form on views: va = (flat array, offset, W, inc, ld), vb likewise or None (the self form)
    -> {"count", "first_excluded", "C", "stat_a", "stat_b"} (untouched outputs keep -3)"""
    fa, oa_, Wa, inca, lda = va
    self_form = vb is None
    fb, ob, Wb, incb, ldb = (None, 0, 0, 0, 0) if self_form else vb
    wb = Wa if self_form else Wb
    Cm, sa, sb, info = np.full((Wa, wb), -3.0), np.full((Wa, 2), -3.0), np.full((wb, 2), -3.0), np.full(2, -3.0)
    pa = C.cast(fa.ctypes.data + 8 * oa_, _dp) if fa is not None else None
    pb = C.cast(fb.ctypes.data + 8 * ob, _dp) if fb is not None else None
    rc = _lib.check(_lib.lib().gel_batch_comoments(E._h, B, Wa, inca, lda, pa, Wb, incb, ldb, pb, Cm.ctypes.data_as(_dp) if Cm.size else None,
                                                   sa.ctypes.data_as(_dp) if want_stats and Wa else None,
                                                   sb.ctypes.data_as(_dp) if want_stats and not self_form and wb else None, info.ctypes.data_as(_dp)))
    assert rc == 0
    return {"count": int(info[0]), "first_excluded": int(info[1]), "C": Cm, "stat_a": sa, "stat_b": sa if self_form else sb}


def packed(E, A, Bv=None, **k):
    A = np.ascontiguousarray(A)
    va = (A.reshape(-1), 0, A.shape[1], 1, max(A.shape[1], 1))
    vb = None if Bv is None else (np.ascontiguousarray(Bv).reshape(-1), 0, Bv.shape[1], 1, max(Bv.shape[1], 1))
    return raw(E, A.shape[0], va, vb, **k)


def check_exact(R, A, Bv=None):
    T = ct.comoments_exact(A, Bv)
    assert R["count"] == T["count"] and R["first_excluded"] == T["first_excluded"]
    for f in ("C", "stat_a", "stat_b"):
        assert same(R[f], T[f]), (f, np.argwhere(_bits(R[f]) != _bits(T[f]))[:5], R[f].ravel()[:4], T[f].ravel()[:4])
    if Bv is None:
        assert same(R["C"], R["C"].T) and same(np.diagonal(R["C"]), R["stat_a"][:, 1])
    return T


# ------------------------------------------------------------------ 1. bit for bit at every batch size and width
def _shapes(B, ta, tb):
    wa, wb = [1, ta - 1, ta, ta + 1, 2 * ta + 3], [1, tb - 1, tb, tb + 1, 2 * tb + 3]
    two = {1: [(0, 0), (1, 4), (4, 3), (2, 2)], 2: [(0, 4), (4, 1), (3, 3), (1, 2)], 255: [(1, 3)], 256: [(2, 2), (0, 4)], 257: [(3, 1), (4, 0)],
           513: [(3, 3)]}[B]
    one = {1: [0, 1, 2, 3, 4], 2: [0, 1, 2, 3, 4], 255: [2], 256: [3], 257: [4], 513: [1]}[B]
    return [(wa[i], wb[j]) for i, j in two], [wa[i] for i in one]


@pytest.mark.parametrize("B", [1, 2, 255, 256, 257, 513])
def test_two_views_bit_for_bit(E, tiles, B):
    for Wa, Wb in _shapes(B, *tiles)[0]:
        assert B * Wa * Wb <= 1500 * 513
        A, Bv = data(B, Wa, 1), data(B, Wb, 2)
        check_exact(packed(E, A, Bv), A, Bv)


@pytest.mark.parametrize("B", [1, 2, 255, 256, 257, 513])
def test_self_form_bit_for_bit(E, tiles, B):
    for W in _shapes(B, *tiles)[1]:
        A = data(B, W, 3)
        R = packed(E, A)
        check_exact(R, A)
        if B == 1:
            assert np.all(R["C"] == 0.0) and same(R["stat_a"][:, 0], A[0])


def test_python_layer(E):
    A, Bv = data(300, 5, 4), data(300, 3, 5)
    R, T = E.batch_comoments(A, Bv), ct.comoments_exact(A, Bv)
    assert R["count"] == 300 and R["first_excluded"] == -1 and same(R["C"], T["C"])
    assert same(R["mean_a"], T["stat_a"][:, 0]) and same(R["m2_a"], T["stat_a"][:, 1]) and same(R["m2_b"], T["stat_b"][:, 1])
    assert same(R["cov"], T["C"] / 299.0) and same(R["corr"], T["C"] / np.sqrt(T["stat_a"][:, 1][:, None] * T["stat_b"][:, 1][None, :]))
    S = E.batch_comoments(A)
    assert same(S["C"], ct.comoments_exact(A)["C"]) and same(S["mean_b"], S["mean_a"]) and np.all(np.abs(np.diagonal(S["corr"]) - 1.0) <= 2.0 ** -52)
    assert ct.check_C(A, Bv, R["C"]) <= 1.0


# ------------------------------------------------------------------ 2. views
def test_strided_views_with_offsets(E):
    """inc = 4, ld > W, a non-zero base offset, in both views; everything the call does not read is NaN"""
    B, Wa, Wb = 300, 7, 5
    A, Bv = data(B, Wa, 6), data(B, Wb, 7)
    P = packed(E, A, Bv)
    check_exact(P, A, Bv)
    lda, oa_, ldb, ob = 4 * Wa + 5, 3, Wb + 9, 2
    fa = np.full(B * lda + 16, np.nan)
    fb = np.full(B * ldb + 16, np.nan)
    for r in range(B):
        fa[oa_ + r * lda:oa_ + r * lda + 4 * Wa:4] = A[r]
        fb[ob + r * ldb:ob + r * ldb + Wb] = Bv[r]
    V = raw(E, B, (fa, oa_, Wa, 4, lda), (fb, ob, Wb, 1, ldb))
    S = raw(E, B, (fa, oa_, Wa, 4, lda))
    for f in ("C", "stat_a", "stat_b"):
        assert same(V[f], P[f]), f
    assert V["count"] == B and V["first_excluded"] == -1
    Ps = packed(E, A)
    assert same(S["C"], Ps["C"]) and same(S["stat_a"], Ps["stat_a"]) and S["count"] == B
    # the least ld: (W - 1) inc + 1
    tight = np.ascontiguousarray(fa[oa_:oa_ + B * lda].reshape(B, lda)[:, :4 * (Wa - 1) + 1]).reshape(-1)
    assert same(raw(E, B, (tight, 0, Wa, 4, 4 * (Wa - 1) + 1))["C"], Ps["C"])


# ------------------------------------------------------------------ 3. the listwise exclusion
def test_nan_and_infinities_exclude_the_flight(E):
    B = 300
    A, Bv = data(B, 3, 8), data(B, 2, 9)
    A[5, 1], Bv[100, 0], A[299, 2] = np.nan, np.inf, -np.inf
    R = packed(E, A, Bv)
    check_exact(R, A, Bv)
    assert R["count"] == 297 and R["first_excluded"] == 5
    assert ct.check_C(A, Bv, R["C"]) <= 1.0
    S = packed(E, A)                                          # the self form reads a alone: flight 100 counts
    check_exact(S, A)
    assert S["count"] == 298
    # pairwise exclusion would give other bits for the pairs of clean columns
    assert not same(R["C"], ct.comoments_exact(A, Bv, wrong="pairwise")["C"])


@pytest.mark.parametrize("block", [0, 2])
def test_a_whole_block_excluded(E, block):
    """B = 1,000: block 0 wholly excluded (the first counted block is block 1), or block 2 (the merge steps over it)"""
    B = 1000
    A, Bv = data(B, 2, 10 + block), data(B, 2, 20 + block)
    Bv[256 * block:256 * block + 256, 1] = np.nan
    R = packed(E, A, Bv)
    check_exact(R, A, Bv)
    assert R["count"] == B - 256 and R["first_excluded"] == 256 * block


def test_every_flight_excluded_and_one_flight_left(E):
    B = 300
    A, Bv = data(B, 3, 12), data(B, 2, 13)
    Bv[:, 0] = np.nan
    R = packed(E, A, Bv)
    assert R["count"] == 0 and R["first_excluded"] == 0
    assert np.isnan(R["C"]).all() and np.isnan(R["stat_a"]).all() and np.isnan(R["stat_b"]).all()
    Bv[277, 0] = 1.5
    R = packed(E, A, Bv)
    check_exact(R, A, Bv)
    assert R["count"] == 1 and R["first_excluded"] == 0 and same(R["C"], np.zeros((3, 2)))
    assert same(R["stat_a"], np.stack([A[277], np.zeros(3)], axis=1)) and same(R["stat_b"], np.stack([Bv[277], np.zeros(2)], axis=1))


# ------------------------------------------------------------------ 4. independence
def test_host_form_device_form_second_call(E):
    import torch
    B, Wa, Wb = 513, 9, 6
    A, Bv = data(B, Wa, 14), data(B, Wb, 15)
    A[7, 0] = np.nan
    H = packed(E, A, Bv)
    check_exact(H, A, Bv)
    H2 = packed(E, A, Bv)
    dA, dB = torch.from_numpy(A).cuda(), torch.from_numpy(Bv).cuda()
    for turn in range(2):
        dC = torch.full((Wa, Wb), -3.0, dtype=torch.float64, device="cuda")
        dsa, dsb, di = (torch.full(s, -3.0, dtype=torch.float64, device="cuda") for s in ((Wa, 2), (Wb, 2), (2,)))
        torch.cuda.synchronize()
        E.batch_comoments_device(B, Wa, 1, Wa, dA.data_ptr(), Wb, 1, Wb, dB.data_ptr(), dC.data_ptr(), dsa.data_ptr() if turn == 0 else 0,
                                 dsb.data_ptr() if turn == 0 else 0, di.data_ptr())
        assert E.sync() == 0                                  # NaN in the source never raises the status
        assert same(dC.cpu().numpy(), H["C"]) and di.cpu().numpy().tolist() == [B - 1.0, 7.0]
        if turn == 0:
            assert same(dsa.cpu().numpy(), H["stat_a"]) and same(dsb.cpu().numpy(), H["stat_b"])
        else:
            assert (dsa.cpu().numpy() == -3.0).all() and (dsb.cpu().numpy() == -3.0).all()      # not asked for: not written
    dC = torch.full((Wa, Wa), -3.0, dtype=torch.float64, device="cuda")
    dsa, di = torch.full((Wa, 2), -3.0, dtype=torch.float64, device="cuda"), torch.full((2,), -3.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    E.batch_comoments_device(B, Wa, 1, Wa, dA.data_ptr(), 0, 0, 0, 0, dC.data_ptr(), dsa.data_ptr(), 0, di.data_ptr())
    assert E.sync() == 0
    S = packed(E, A)
    assert same(dC.cpu().numpy(), S["C"]) and same(dsa.cpu().numpy(), S["stat_a"])
    for f in ("C", "stat_a", "stat_b"):
        assert same(H[f], H2[f]), f


def test_a_pair_alone_and_inside_a_wide_call(E, tiles):
    ta, tb = tiles
    B, Wa, Wb = 300, ta + 8, tb + 5
    A, Bv = data(B, Wa, 16), data(B, Wb, 17)
    R = packed(E, A, Bv)
    S = packed(E, A)
    fa, fb = A.reshape(-1), Bv.reshape(-1)
    for i, j in ((0, 0), (3, tb + 4), (ta - 1, tb), (ta, tb - 1), (ta + 7, 2)):
        one = raw(E, B, (fa, i, 1, 1, Wa), (fb, j, 1, 1, Wb))
        assert same(one["C"][0, 0], R["C"][i, j]) and same(one["stat_a"][0], R["stat_a"][i]) and same(one["stat_b"][0], R["stat_b"][j]), (i, j)
    for i, j in ((0, 1), (2, ta + 3), (ta - 1, ta), (ta, ta + 7)):
        one = raw(E, B, (fa, i, 1, 1, Wa), (fa, j, 1, 1, Wa))            # the same pair of a's columns, as a two-view call
        assert same(one["C"][0, 0], S["C"][i, j]) and same(one["C"][0, 0], S["C"][j, i]), (i, j)


def test_one_slab_and_many(E, tiles):
    """the measurement switches cut the product into slabs of b columns and of a columns: the same bits"""
    ta, tb = tiles
    B, Wa, Wb = 300, 2 * ta + 3, tb + 9
    A, Bv = data(B, Wa, 18), data(B, Wb, 19)
    R, S = packed(E, A, Bv), packed(E, A)
    assert E.batch_comoments_info(B, Wa, Wb)["slabs"] == 1
    for env in ({"GEL_COMOM_SLAB": "5"}, {"GEL_COMOM_SLAB": str(tb)}, {"GEL_COMOM_SLAB_ROWS": str(ta)}, {"GEL_COMOM_SLAB": "7", "GEL_COMOM_SLAB_ROWS": "3"}):
        os.environ.update(env)
        try:
            assert E.batch_comoments_info(B, Wa, Wb)["slabs"] > 1
            R2, S2 = packed(E, A, Bv), packed(E, A)
        finally:
            for k in env:
                del os.environ[k]
        for f in ("C", "stat_a", "stat_b"):
            assert same(R2[f], R[f]) and same(S2[f], S[f]), (env, f)
    T = ct.comoments_exact(A[:, ta - 2:ta + 3], Bv[:, tb - 2:tb + 3])            # a window across the tile edges against the truth
    assert same(R["C"][ta - 2:ta + 3, tb - 2:tb + 3], T["C"])


def test_empty_batch_empty_width_and_the_call_after(E):
    A, Bv = data(40, 3, 30), data(40, 2, 31)
    good = packed(E, A, Bv)
    check_exact(good, A, Bv)
    R = packed(E, np.zeros((0, 3)), np.zeros((0, 2)))
    assert R["count"] == 0 and R["first_excluded"] == -1 and np.isnan(R["C"]).all() and np.isnan(R["stat_a"]).all() and np.isnan(R["stat_b"]).all()
    assert same(packed(E, A, Bv)["C"], good["C"])
    S = packed(E, np.zeros((0, 3)))
    assert S["count"] == 0 and np.isnan(S["C"]).all() and S["C"].shape == (3, 3)
    R = packed(E, np.zeros((40, 0)), Bv)                      # Wa = 0: info only
    assert R["count"] == 40 and R["first_excluded"] == -1 and (R["stat_b"] == -3.0).all()
    Bn = Bv.copy()
    Bn[11, 1] = np.nan
    R = packed(E, A, np.ascontiguousarray(Bn[:, :0]))         # Wb = 0
    assert R["count"] == 40 and (R["stat_a"] == -3.0).all()
    R = packed(E, np.zeros((40, 0)), Bn)                      # the entries of b are read all the same: the count says so
    assert R["count"] == 39 and R["first_excluded"] == 11
    after = packed(E, A, Bv)
    for f in ("C", "stat_a", "stat_b"):
        assert same(after[f], good[f]), f
    P = E.batch_comoments(np.zeros((0, 2)))
    assert P["count"] == 0 and np.isnan(P["cov"]).all() and np.isnan(P["corr"]).all()


# ------------------------------------------------------------------ 5. the example problem's dispersed flight
def test_flight_covariance():
    from gelato_amd import con_dynamics, montecarlo, pack_x, problem, propagate
    pdict, unitdict, _cond, xdict = problem.make_problem("example")
    S, ps = pdict["num_sections"], pdict["ps_params"]
    Ee = Engine(con_dynamics.problem_arrays(pdict, unitdict), D=[ps.D(i) for i in range(S)], tau=[ps.tau(i) for i in range(S)])
    lc = pdict["LaunchCondition"]
    B = 300
    X = np.tile(pack_x(xdict), (B, 1))
    D = propagate.sample_dispersion(B, S, [0.02, 0.01, 0.03, 0.2], seed=4)
    cols = ["altitude", "altitude_apogee", "altitude_perigee", "inclination", "dynamic_pressure", "Q_alpha", "M", "lat_IIP"]
    F = montecarlo.flight_covariance(X, pdict, unitdict, D, steps=1, columns=cols, engine=Ee)
    env = montecarlo.flight_envelope(X, pdict, unitdict, dispersion=D, steps=1, columns=cols, engine=Ee)
    assert F["columns"] == cols and F["steps"] == env["steps"] == 2 and F["status"] == env["status"]
    T = Ee.output_table_batch(env["x_flown"], lc["lat"], lc["lon"], dispersion=D, columns=cols)
    M, nc = Ee.M, len(cols)
    table = T["table"]
    term = np.ascontiguousarray(table[:, M - 1, :])
    finite = np.isfinite(term).all(axis=0)
    assert finite[:4].all()                                   # the insertion state is there in every flight
    # the self form over the columns that are finite in every flight: the envelope's mean and m2 at the last node, bit for bit
    fin_cols = [k for k in range(nc) if finite[k]]
    R = Ee.batch_comoments(np.ascontiguousarray(term[:, fin_cols]))
    assert R["count"] == B
    for k2, k in enumerate(fin_cols):
        e = T["envelope"][cols[k]]
        assert e["count"][M - 1] == B and same(R["mean_a"][k2], e["mean"][M - 1]) and same(R["m2_a"][k2], e["m2"][M - 1]), cols[k]
    # flight_covariance is these calls composed by hand
    disp = np.ascontiguousarray(D.reshape(B, 4 * S))
    pkmax = np.ascontiguousarray(np.stack([np.asarray(T["peaks"][c]["max"], dtype=np.float64) for c in cols], axis=1))
    miss = np.ascontiguousarray(env["terminal_miss"])
    hand = {"terminal": Ee.batch_comoments(term), "dispersion": Ee.batch_comoments(disp)}
    sens = {"terminal": Ee.batch_comoments(disp, term), "peak_max": Ee.batch_comoments(disp, pkmax), "terminal_miss": Ee.batch_comoments(disp, miss)}
    for got, want in [(F[k], hand[k]) for k in hand] + [(F["sensitivity"][k], sens[k]) for k in sens]:
        assert got["count"] == want["count"] and got["first_excluded"] == want["first_excluded"]
        for f in ("C", "mean_a", "m2_a", "mean_b", "m2_b", "cov", "corr"):
            assert same(got[f], want[f]), f
    listwise = int(np.isfinite(term).all(axis=1).sum())
    assert F["terminal"]["count"] == listwise == F["sensitivity"]["terminal"]["count"] and F["dispersion"]["count"] == B
    assert same(F["terminal"]["C"], F["terminal"]["C"].T)
    for g, want in sens.items():
        s = montecarlo.dispersion_sensitivity(want["count"], hand["dispersion"]["C"], want["C"], want["m2_b"])
        got = F["sensitivity"][g]
        assert same(got["beta"], s["beta"]) and same(got["explained"], s["explained"]) and same(got["share"], s["share"])
        ex = got["explained"]
        print("explained by the linear model,", g, dict(zip(cols if g != "terminal_miss" else ("mass", "position", "velocity", "quaternion"),
                                                               np.round(ex, 4).tolist())))
        if want["count"] == B:                                # the factors' co-moments are those of the same flights
            assert np.all((ex[np.isfinite(ex)] >= 0.0) & (ex[np.isfinite(ex)] <= 1.0 + 1e-9)), (g, ex)
    assert np.isfinite(F["sensitivity"]["peak_max"]["explained"]).any()
    Ee.close()

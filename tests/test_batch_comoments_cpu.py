"""gel_batch_comoments* without a GPU: the symbols, every refusal (decided before the device is looked at) on a
host-only handle, gel_batch_comoments_info, the truth module (tests/comoment_truth.py) on its own -- the restated order against
output_batch_truth's m2 bit for bit and inside the derived bound of the exact co-moment, told apart from four wrong restatements
and from the textbook formula -- montecarlo.dispersion_sensitivity on a designed batch, and the refusals under AddressSanitizer +
UBSan in a stand-alone program."""
import ctypes as C
import os

import numpy as np
import pytest

import comoment_truth as ct
import interp_truth as it
import output_batch_truth as obt
import sanitized_lib
from gelato_amd import Engine, _lib, montecarlo

GEL_ERR_ARG, GEL_ERR_HIP = -1, -2          # include/gelato_amd.h
_dp = C.POINTER(C.c_double)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def host():
    E = it.engine(it.prob_of([3, 4]))
    yield E
    E.close()


def test_symbols_and_signatures():
    L = _lib.lib()
    for name, nargs in (("gel_batch_comoments", 14), ("gel_batch_comoments_device", 14), ("gel_batch_comoments_info", 6)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert getattr(L, name).restype is C.c_int
    for name in ("batch_comoments", "batch_comoments_device", "batch_comoments_info"):
        assert callable(getattr(Engine, name))
    assert callable(montecarlo.flight_covariance) and callable(montecarlo.dispersion_sensitivity)
    assert "listwise" in montecarlo.flight_covariance.__doc__.lower() and "NaN" in montecarlo.flight_covariance.__doc__


def _call(E, B, Wa, inca, lda, a, Wb, incb, ldb, b, Cm, sa, sb, info, device_form=False, handle=True):
    h = E._h if handle else None
    if device_form:
        vp = lambda v: None if v is None else v.ctypes.data
        rc = _lib.lib().gel_batch_comoments_device(h, B, Wa, inca, lda, vp(a), Wb, incb, ldb, vp(b), vp(Cm), vp(sa), vp(sb), vp(info))
    else:
        dp = lambda v: None if v is None else v.ctypes.data_as(_dp)
        rc = _lib.lib().gel_batch_comoments(h, B, Wa, inca, lda, dp(a), Wb, incb, ldb, dp(b), dp(Cm), dp(sa), dp(sb), dp(info))
    return rc, _lib.lib().gel_last_error().decode()


@pytest.mark.parametrize("device_form", [False, True])
def test_refusals_on_a_host_only_handle(host, device_form):
    a, b = np.zeros((7, 12)), np.zeros((7, 4))
    Cm, sa, sb, info = np.zeros((3, 4)), np.zeros((3, 2)), np.zeros((4, 2)), np.zeros(2)
    call = lambda *v, **k: _call(host, *v, device_form=device_form, **k)
    cases = [
        (call(7, 3, 1, 3, a, 4, 1, 4, b, Cm, sa, sb, info, handle=False), "null handle"),
        (call(-1, 3, 1, 3, a, 4, 1, 4, b, Cm, sa, sb, info), "B < 0"),
        (call(7, -1, 1, 3, a, 4, 1, 4, b, Cm, sa, sb, info), "W < 0"),
        (call(7, 3, 1, 3, a, -1, 1, 4, b, Cm, sa, sb, info), "W < 0"),
        (call(7, 3, 0, 3, a, 4, 1, 4, b, Cm, sa, sb, info), "inc < 1"),
        (call(7, 3, 1, 3, a, 4, 0, 4, b, Cm, sa, sb, info), "inc < 1"),
        (call(7, 3, 1, 2, a, 4, 1, 4, b, Cm, sa, sb, info), "lda = 2"),
        (call(7, 3, 4, 8, a, 4, 1, 4, b, Cm, sa, sb, info), "lda = 8"),          # (3 - 1) 4 + 1 = 9 is the least
        (call(7, 3, 1, 3, a, 4, 1, 3, b, Cm, sa, sb, info), "ldb = 3"),
        (call(7, 3, 1, 3, None, 4, 1, 4, b, Cm, sa, sb, info), "a is NULL"),
        (call(7, 3, 1, 3, a, 4, 1, 4, b, None, sa, sb, info), "C is NULL"),
        (call(7, 3, 1, 3, a, 4, 1, 4, b, Cm, sa, sb, None), "info is NULL"),
        (call(7, 3, 1, 3, a, 0, 0, 0, None, Cm, sa, sb, info), "stat_b given in the self form"),
    ]
    for (rc, msg), text in cases:
        assert rc == GEL_ERR_ARG and text in msg, (rc, msg, text)
    # valid calls: what gel_output_table_batch returns on such a handle
    x, env = np.zeros((2, host.nvars)), np.zeros((host.M, 34, 8))
    rc1 = _lib.lib().gel_output_table_batch(host._h, 2, x.ctypes.data_as(_dp), None, None, 28.5, 0.0, 0, None, None, env.ctypes.data_as(_dp), None)
    msg1 = _lib.lib().gel_last_error().decode()
    assert rc1 == GEL_ERR_HIP and "host-only" in msg1
    for got in (call(7, 3, 1, 3, a, 4, 1, 4, b, Cm, sa, sb, info), call(7, 3, 4, 9, a, 4, 1, 4, b, Cm, None, None, info),
                call(7, 3, 1, 3, a, 0, 0, 0, None, Cm, sa, None, info), call(0, 3, 1, 3, None, 4, 1, 4, None, Cm, None, None, info),
                call(7, 0, 1, 0, None, 4, 1, 4, b, None, None, None, info), call(7, 3, 1, 3, a, 0, 1, 0, b, None, None, None, info)):
        assert got == (rc1, msg1)


def test_python_argument_checks(host):
    A = np.zeros((4, 3))
    with pytest.raises(TypeError, match="float64"):
        host.batch_comoments(A.astype(np.float32))
    with pytest.raises(ValueError, match="C-contiguous"):
        host.batch_comoments(np.zeros((3, 4)).T)
    with pytest.raises(ValueError, match=r"\[B, W\]"):
        host.batch_comoments(np.zeros(4))
    with pytest.raises(ValueError, match="rows"):
        host.batch_comoments(A, np.zeros((5, 2)))
    with pytest.raises(_lib.GelatoAmdError, match="host-only"):   # well-formed calls reach the library
        host.batch_comoments(A)
    with pytest.raises(_lib.GelatoAmdError, match="host-only"):
        host.batch_comoments(A, np.zeros((4, 2)))
    with pytest.raises(_lib.GelatoAmdError, match="info is NULL"):
        host.batch_comoments_device(4, 3, 1, 3, A.ctypes.data, 0, 1, 1, 0, A.ctypes.data)


def test_info_on_a_host_only_handle(host):
    keys = {"block", "tile_a", "tile_b", "slab_rows", "slab_cols", "slabs", "workspace_bytes", "workspace_cap_bytes", "passes_a", "passes_b"}
    for B, Wa, Wb in ((65536, 24, 34), (65536, 24, 13260), (65536, 48, 128 * 13 * 34), (300, 34, None), (65536, 13260, None), (1, 1, 1)):
        i = host.batch_comoments_info(B, Wa, Wb)
        wb = Wa if Wb is None else Wb
        assert set(i) == keys and i["block"] == 256 and i["tile_a"] >= 1 and i["tile_b"] >= 1
        assert 1 <= i["slab_cols"] <= wb and 1 <= i["slab_rows"] <= Wa
        assert -(-Wa // i["slab_rows"]) * -(-wb // i["slab_cols"]) == i["slabs"] and i["slabs"] * i["slab_cols"] >= wb
        assert i["workspace_bytes"] <= i["workspace_cap_bytes"] == 256 << 20
        assert i["passes_a"] == 1 + -(-wb // i["tile_b"]) and i["passes_b"] == (0 if Wb is None else 1 + -(-Wa // i["tile_a"]))
    assert host.batch_comoments_info(65536, 24, 34)["slabs"] == 1
    wide = host.batch_comoments_info(65536, 24, 13260)
    assert wide["slabs"] > 1 and wide["slab_rows"] == 24 and wide["slab_cols"] % wide["tile_b"] == 0
    tall = host.batch_comoments_info(65536, 13260, None)          # all a columns beside one tile of b do not fit: a is walked too
    assert tall["slab_rows"] < 13260 and tall["slab_rows"] % tall["tile_a"] == 0
    assert host.batch_comoments_info(0, 9, 9)["passes_a"] == 0 and host.batch_comoments_info(5, 0, 3)["slabs"] == 0
    # the measurement switch caps the b columns of a slab
    os.environ["GEL_COMOM_SLAB"] = "5"
    try:
        j = host.batch_comoments_info(300, 7, 23)
    finally:
        del os.environ["GEL_COMOM_SLAB"]
    assert j["slab_cols"] == 5 and j["slabs"] == 5 and host.batch_comoments_info(300, 7, 23)["slabs"] == 1
    info = _lib.GelComomentsInfo()
    L = _lib.lib()
    for args in ((None, 1, 1, 1, 0, C.byref(info)), (host._h, 1, 1, 1, 0, None), (host._h, -1, 1, 1, 0, C.byref(info)),
                 (host._h, 1, -1, 1, 0, C.byref(info)), (host._h, 1, 1, -1, 0, C.byref(info))):
        assert L.gel_batch_comoments_info(*args) == GEL_ERR_ARG
    # a batch whose per-vector and per-column part alone fills the cap is refused, with the reason
    assert L.gel_batch_comoments_info(host._h, 2 ** 31 - 1, 4, 4, 0, C.byref(info)) == GEL_ERR_ARG
    assert "no room" in L.gel_last_error().decode()


# ---------------------------------------------------------------- the truth module alone
def test_integer_fma_is_the_fraction_fma():
    rng = np.random.default_rng(5)
    v = rng.standard_normal((4000, 3)) * np.exp(rng.uniform(-40.0, 40.0, (4000, 3)))
    v[:50, 2] = 0.0
    v[50:100, 0] = 0.0
    v[100:200, 2] = -(v[100:200, 0] * v[100:200, 1])         # heavy cancellation: the one rounding matters
    v[200:260] *= 1e-160                                     # products in the subnormal range
    v[260:300, 2] = 1e300
    for a, b, c in v.tolist():
        assert _bits(ct.fma(a, b, c)) == _bits(obt.fma(a, b, c)), (a, b, c)
    assert ct.fma(1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30, -1.0) == -2.0 ** -60 != (1.0 + 2.0 ** -30) * (1.0 - 2.0 ** -30) - 1.0


def _batches():
    """name -> (A, Bv or None): random data over several blocks, with and without excluded flights, and the 1 + 1e-9 b batches whose
    means dwarf their spread (|v|_2 / sqrt(m2) >= 1e6)"""
    rng = np.random.default_rng(21)
    out = {}
    A, Bv = rng.standard_normal((600, 3)) * [1.0, 30.0, 1e-3] + [0.0, 100.0, -2.0], rng.standard_normal((600, 2)) + [5.0, -1e4]
    Bv[:, 0] += 0.7 * A[:, 0]
    out["random"] = (A.copy(), Bv.copy())
    A[[3, 300], 1] = np.nan
    Bv[[17, 256, 599], 0] = [np.inf, -np.inf, np.nan]
    out["random_excluded"] = (A, Bv)
    out["self"] = (rng.standard_normal((300, 4)) + [0.0, 1.0, -50.0, 1e3], None)
    r = np.arange(700.0)
    out["offset_1e6"] = (np.stack([3.7 * (1.0 + 1e-9 * r), -0.9 * (1.0 + 1e-9 * ((r * 37.0) % 700.0))], axis=1),
                         np.stack([-2.2 * (1.0 + 1e-9 * r), 41.0 * (1.0 + 1e-9 * ((r * 11.0) % 700.0))], axis=1))
    out["offset_1e6_self"] = (out["offset_1e6"][0], None)
    return out


BATCHES = _batches()


def test_offset_batches_are_as_hard_as_stated():
    A, Bv = BATCHES["offset_1e6"]
    for col in list(A.T) + list(Bv.T):
        st = obt.exact_stats(col)
        assert st["l2"] / np.sqrt(st["m2"]) >= 1e6


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_restated_order_diagonal_is_the_envelopes_m2_and_inside_the_bound(name):
    A, Bv = BATCHES[name]
    R = ct.comoments_exact(A, Bv)
    ok = ct.counted_rows(A, Bv)
    assert R["count"] == int(ok.sum()) and R["first_excluded"] == (int(np.nonzero(~ok)[0][0]) if not ok.all() else -1)
    # a column's mean and m2 are the envelope's bits where the counted flights are the column's finite ones: NaN the others first
    for M_, stat in ((A, R["stat_a"]),) + (() if Bv is None else ((Bv, R["stat_b"]),)):
        for c in range(M_.shape[1]):
            env = obt.welford_merge_exact(np.where(ok, M_[:, c], np.nan))
            assert env[0] == R["count"] and np.array_equal(_bits(env[1:3]), _bits(stat[c])), (name, c)
    if Bv is None:
        assert np.array_equal(_bits(R["C"]), _bits(R["C"].T)) and np.array_equal(_bits(np.diagonal(R["C"])), _bits(R["stat_a"][:, 1]))
    share = ct.check_C(A, Bv, R["C"])
    print("comoments_exact %s: largest share of the bound of C used %.4f" % (name, share))
    assert 0.0 < share <= 1.0


def test_teeth_each_wrong_variant_differs_in_bits():
    A, Bv = BATCHES["random_excluded"]
    good = ct.comoments_exact(A, Bv)
    for wrong in ("eb_old_mean", "pairwise", "merge_mean_first"):
        bad = ct.comoments_exact(A, Bv, wrong=wrong)
        assert not np.array_equal(_bits(good["C"]), _bits(bad["C"])), wrong
    # the contracted merge shows where the spread between the blocks is comparable with the spread inside them (as m2's does): the
    # same batch with every block's level stepped
    step = (np.arange(600) // 256)[:, None]
    As, Bs = BATCHES["random"][0][:, :2] + step * [1.0, -2.0], BATCHES["random"][1] + step * [3.0, 0.5]
    assert not np.array_equal(_bits(ct.comoments_exact(As, Bs)["C"]), _bits(ct.comoments_exact(As, Bs, wrong="merge_fma")["C"]))
    # inside ONE block there is no merge: the two merge variants cannot show there, the other two do
    A1, B1 = A[:200], Bv[:200]
    g1 = ct.comoments_exact(A1, B1)
    for wrong, shows in (("eb_old_mean", True), ("pairwise", True), ("merge_fma", False), ("merge_mean_first", False)):
        assert np.array_equal(_bits(g1["C"]), _bits(ct.comoments_exact(A1, B1, wrong=wrong)["C"])) != shows, wrong
    # pairwise exclusion counts more flights for the pairs of clean columns; listwise is one set for every pair
    pw = ct.comoments_exact(A, Bv, wrong="pairwise")
    assert np.array_equal(_bits(pw["C"][1, 0]), _bits(ct.comoments_exact(A[:, 1:2], Bv[:, 0:1])["C"][0, 0]))
    # eb with the old mean is sum d_a d_b: larger than the co-moment by the factor of Welford's update, far outside the bound
    with pytest.raises(AssertionError):
        ct.check_C(A1, B1, ct.comoments_exact(A1, B1, wrong="eb_old_mean")["C"])


def test_teeth_textbook_formula_breaks_the_bound():
    A, Bv = BATCHES["offset_1e6"]
    worst = 0.0
    for i in range(2):
        for j in range(2):
            st = ct.exact_comoment(A[:, i], Bv[:, j])
            lim = ct.comoment_bound(st, A.shape[0]) + ct.U * abs(st["C"])
            worst = max(worst, abs(ct.textbook(A[:, i], Bv[:, j]) - st["C"]) / lim)
    print("textbook sum a b - n mean_a mean_b on the 1e6 batch: %.3g times the bound" % worst)
    assert worst > 1.0
    A0, B0 = BATCHES["random"]                              # ... and passes where the means do not dwarf the spread
    st = ct.exact_comoment(A0[:, 0], B0[:, 0])
    assert abs(ct.textbook(A0[:, 0], B0[:, 0]) - st["C"]) <= ct.comoment_bound(st, 600) + ct.U * abs(st["C"])


def test_exact_comoment_by_hand():
    st = ct.exact_comoment([1.0, 2.0, 3.0, 6.0], [2.0, 0.0, -2.0, 4.0])
    # deviations (-2, -1, 0, 3) . (1, -1, -3, 3)
    assert st["C"] == 8.0 and st["Sa"] == 14.0 and st["Sb"] == 20.0 and st["la"] == np.sqrt(50.0) and st["n"] == 4
    one = ct.comoments_exact(np.array([[2.5, -1.0]]), np.array([[4.0]]))
    assert one["count"] == 1 and np.all(one["C"] == 0.0) and np.all(one["stat_a"][:, 1] == 0.0) and one["stat_a"][0, 0] == 2.5
    none = ct.comoments_exact(np.array([[np.nan, 1.0], [2.0, np.inf]]))
    assert none["count"] == 0 and none["first_excluded"] == 0 and np.isnan(none["C"]).all() and np.isnan(none["stat_a"]).all()


# ---------------------------------------------------------------- dispersion_sensitivity
def test_dispersion_sensitivity_on_a_designed_batch():
    """a two-level full factorial in four factors (16 runs, repeated over three blocks of 256 = 48 x 16 flights), a fifth factor that
    never moves, and outputs that are integer combinations of the factors: every co-moment is an exact integer, so the regression
    must return the combinations' coefficients"""
    design = np.array([[1.0 if (r >> k) & 1 else -1.0 for k in range(4)] for r in range(16)])
    D = np.concatenate([np.tile(design, (48, 1)), np.ones((768, 1))], axis=1)
    coef = np.array([[3.0, 0.0, 1.0, 0.0], [-2.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 4.0, 5.0, 0.0], [9.0, 9.0, 9.0, 9.0]])
    Y = D @ coef + [7.0, -1.0, 0.0, 5.0]                     # the last output is a constant: m2 = 0
    def exact(P, Q):
        return np.array([[ct.exact_comoment(P[:, i], Q[:, j])["C"] for j in range(Q.shape[1])] for i in range(P.shape[1])])
    dd = {"count": 768, "C": exact(D, D), "stat_a": np.stack([D.mean(axis=0), np.diagonal(exact(D, D))], axis=1)}
    dy = {"count": 768, "C": exact(D, Y), "stat_b": np.stack([Y.mean(axis=0), np.diagonal(exact(Y, Y))], axis=1)}
    assert np.array_equal(dd["C"], np.diag([768.0] * 4 + [0.0])) and np.array_equal(dy["C"][:4], 768.0 * coef[:4]) and np.all(dy["C"][4] == 0.0)
    # the restated order comes within its bound of these integers, and to them exactly where the running means are dyadic
    assert ct.check_C(D, Y, ct.comoments_exact(D, Y)["C"]) <= 1.0
    s = montecarlo.dispersion_sensitivity(dd["count"], dd["C"], dy["C"], dy["stat_b"][:, 1])
    tol = 64.0 * 2.0 ** -53
    assert s["count"] == 768 and s["active"].tolist() == [True] * 4 + [False]
    assert np.all(np.abs(s["beta"][:4] - coef[:4]) <= tol * np.abs(coef[:4])) and np.all(s["beta"][4] == 0.0)      # the zero-variance factor: a zero row
    assert np.all(np.abs(s["explained"][:3] - 1.0) <= tol) and np.isnan(s["explained"][3]) and np.isnan(s["share"][:, 3]).all()
    share = coef[:4, :3] ** 2 * 768.0 / dy["stat_b"][:3, 1]
    assert np.all(np.abs(s["share"][:4, :3] - share) <= 4.0 * tol) and np.all(s["share"][4, :3] == 0.0)
    assert np.all(np.abs(s["share"][:, :3].sum(axis=0) - 1.0) <= 8.0 * tol)                                        # orthogonal factors: the shares add up
    with pytest.raises(ValueError):
        montecarlo.dispersion_sensitivity(3, np.eye(2), np.zeros((3, 1)), np.zeros(1))
    cov, corr = Engine.comoment_ratios(768, dy["C"], dd["stat_a"][:, 1], dy["stat_b"][:, 1])
    assert np.array_equal(cov, dy["C"] / 767.0) and np.isnan(corr[4]).all() and np.isnan(corr[:, 3]).all()
    assert abs(corr[1, 0] + 2.0 / np.sqrt(13.0)) <= tol and np.isnan(Engine.comoment_ratios(1, dy["C"], dd["stat_a"][:, 1], dy["stat_b"][:, 1])[0]).all()


# ---------------------------------------------------------------- the refusals under sanitizers, stand-alone
@sanitized_lib.needs_toolchain
def test_refusals_and_info_under_asan_ubsan(tmp_path):
    """every refusal of both forms and gel_batch_comoments_info on a host-only handle, in a stand-alone program
    (tests/comoments_sanitize.c) under AddressSanitizer + UBSan + LeakSanitizer; nothing is launched"""
    sanitized_lib.run_program(tmp_path, sanitized_lib.build(tmp_path), "comoments_sanitize")

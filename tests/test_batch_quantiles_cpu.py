"""gel_batch_quantiles* without a GPU: the symbols, every refusal (decided before the device is looked at) on a host-only handle,
the Python layer's argument checks, gel_batch_quantiles_info, and the truth module (tests/quantile_truth.py) on its own: against
np.quantile's "lower" / "higher" methods, and told apart from three wrong restatements."""
import ctypes as C

import numpy as np
import pytest

import output_atlas as oa
import quantile_truth as qt
from conftest import load_golden
from gelato_amd import Engine, _lib, montecarlo

GEL_ERR_ARG, GEL_ERR_HIP = -1, -2          # include/gelato_amd.h
_dp = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def g():
    return load_golden(oa.FIXTURE)


@pytest.fixture(scope="module")
def host(g):
    E = Engine(oa.prob_arrays(oa.NODES, g["wind"], g["ca"]), device=-1)
    yield E
    E.close()


def test_symbols_and_signatures():
    L = _lib.lib()
    for name, nargs in (("gel_batch_quantiles", 10), ("gel_batch_quantiles_device", 10), ("gel_batch_quantiles_info", 5),
                        ("gel_batch_quantiles_last", 2)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert getattr(L, name).restype is C.c_int
    assert _lib.GEL_QUANT_MAXQ == 16
    for name in ("batch_quantiles", "batch_quantiles_device", "batch_quantiles_info"):
        assert callable(getattr(Engine, name))
    assert callable(montecarlo.flight_quantiles) and callable(montecarlo.flight_envelope)


def _call(E, B, W, ld, src, nq, probs, q, count=None, who=None, device_form=False, handle=True):
    h = E._h if handle else None
    pp = None if probs is None else np.asarray(probs, dtype=np.float64)
    pptr = None if pp is None else pp.ctypes.data_as(_dp)
    if device_form:
        vp = lambda a: None if a is None else a.ctypes.data
        rc = _lib.lib().gel_batch_quantiles_device(h, B, W, ld, vp(src), nq, pptr, vp(q), vp(count), vp(who))
    else:
        dp = lambda a: None if a is None else a.ctypes.data_as(_dp)
        rc = _lib.lib().gel_batch_quantiles(h, B, W, ld, dp(src), nq, pptr, dp(q), dp(count), dp(who))
    return rc, _lib.lib().gel_last_error().decode()


@pytest.mark.parametrize("device_form", [False, True])
def test_refusals_on_a_host_only_handle(host, g, device_form):
    src, q, cnt, who = np.zeros((3, 5)), np.zeros((5, 2, 2)), np.zeros(5), np.zeros((5, 2, 2))
    p2 = [0.25, 0.5]
    call = lambda *a, **k: _call(host, *a, device_form=device_form, **k)
    cases = [
        (call(3, 5, 5, src, 2, p2, q, handle=False), "null handle"),
        (call(-1, 5, 5, src, 2, p2, q), "B < 0 or W < 0"),
        (call(3, -1, 5, src, 2, p2, q), "B < 0 or W < 0"),
        (call(3, 5, 4, src, 2, p2, q), "ld = 4 < W = 5"),
        (call(3, 5, 5, None, 2, p2, q), "src is NULL"),
        (call(3, 5, 5, src, 2, p2, None), "q is NULL"),
        (call(3, 5, 5, src, 0, p2, q), "nq = 0 outside 1 .. 16"),
        (call(3, 5, 5, src, 17, [0.5] * 17, np.zeros((5, 17, 2))), "nq = 17 outside 1 .. 16"),
        (call(3, 5, 5, src, 2, None, q), "probs is NULL"),
        (call(3, 5, 5, src, 2, [0.5, np.nan], q), "probs[1]"),
        (call(3, 5, 5, src, 2, [np.inf, 0.5], q), "probs[0]"),
        (call(3, 5, 5, src, 2, [0.5, -1e-300], q), "probs[1]"),
        (call(3, 5, 5, src, 2, [0.5, 1.0 + 2.0 ** -52], q), "probs[1]"),
    ]
    for (rc, msg), text in cases:
        assert rc == GEL_ERR_ARG and text in msg, (rc, msg, text)
    # valid calls: what gel_output_table_batch returns on such a handle
    x, env = np.ascontiguousarray(np.tile(g["x_big"], (2, 1))), np.zeros((host.M, 34, 8))
    rc1 = _lib.lib().gel_output_table_batch(host._h, 2, x.ctypes.data_as(_dp), None, None, 28.5, 0.0, 0, None, None, env.ctypes.data_as(_dp), None)
    msg1 = _lib.lib().gel_last_error().decode()
    assert rc1 == GEL_ERR_HIP and "host-only" in msg1
    for got in (call(3, 5, 5, src, 2, p2, q, cnt, who), call(3, 2, 5, src, 2, [0.0, 1.0], q), call(0, 5, 5, None, 2, p2, q), call(3, 0, 0, None, 2, p2, q),
                call(3, 5, 5, src, 16, np.linspace(0.0, 1.0, 16), np.zeros((5, 16, 2)))):
        assert got == (rc1, msg1)
    st = (C.c_int64 * 4)()
    assert _lib.lib().gel_batch_quantiles_last(host._h, st) == GEL_ERR_HIP
    assert _lib.lib().gel_batch_quantiles_last(None, st) == GEL_ERR_ARG and _lib.lib().gel_batch_quantiles_last(host._h, None) == GEL_ERR_ARG


def test_python_argument_checks(host):
    A = np.zeros((4, 3))
    with pytest.raises(ValueError, match="probs:"):
        host.batch_quantiles(A, [])
    with pytest.raises(ValueError, match="probs:"):
        host.batch_quantiles(A, [0.5] * 17)
    with pytest.raises(ValueError, match="probs:"):
        host.batch_quantiles(A, [[0.5, 0.6]])
    with pytest.raises(ValueError, match="probs:"):
        host.batch_quantiles(A, [0.5, 1.5])
    with pytest.raises(ValueError, match="probs:"):
        host.batch_quantiles(A, [np.nan])
    with pytest.raises(TypeError, match="float64"):
        host.batch_quantiles(A.astype(np.float32), [0.5])
    with pytest.raises(ValueError, match="C-contiguous"):
        host.batch_quantiles(np.zeros((3, 4)).T, [0.5])
    with pytest.raises(ValueError, match="probs:"):
        host.batch_quantiles_device(4, 3, 3, 0, [2.0], 0)
    with pytest.raises(_lib.GelatoAmdError, match="host-only"):   # well-formed calls reach the library
        host.batch_quantiles(A, [0.5], who=True)
    with pytest.raises(_lib.GelatoAmdError, match="host-only"):
        host.batch_quantiles(np.zeros((4, 2, 3)), 0.5)
    with pytest.raises(_lib.GelatoAmdError, match="q is NULL"):
        host.batch_quantiles_device(4, 3, 3, A.ctypes.data, [0.5], 0)
    with pytest.raises(_lib.GelatoAmdError, match="host-only"):
        host.batch_quantiles_last()


def test_info_on_a_host_only_handle(host):
    i = host.batch_quantiles_info(65536, 13260, 5)
    assert set(i) == {"bins", "cap", "chunk", "slab_cols", "workspace_bytes", "workspace_cap_bytes", "passes", "slabs"}
    assert i["bins"] >= 64 and i["cap"] >= 256 and 4 <= i["chunk"] < 65536 and i["passes"] == 3
    assert i["slab_cols"] % 64 == 0 and i["slab_cols"] >= 64 and i["workspace_bytes"] <= i["workspace_cap_bytes"] == 256 << 20
    assert i["slabs"] == -(-13260 // i["slab_cols"])
    # the slab is the most the cap holds: what the header states per column and per (column, rank)
    per_col = 1048 + 2 * 5 * (32 + 8 * i["cap"])
    assert (i["slab_cols"] + 64) * per_col > i["workspace_cap_bytes"] - 1024 >= i["slab_cols"] * per_col - 1024
    # more probabilities, fewer columns per slab; a narrow source takes what it needs and the narrow chunk
    j = host.batch_quantiles_info(600, 9, 16)
    assert j["slab_cols"] < i["slab_cols"] and j["slabs"] == 1 and j["workspace_bytes"] < i["workspace_bytes"] and j["chunk"] <= i["chunk"]
    assert host.batch_quantiles_info(0, 9, 1)["passes"] == 0 and host.batch_quantiles_info(5, 0, 1)["slabs"] == 0
    # every threshold sits where a test batch can straddle it
    assert j["chunk"] + 1 <= 4096 and 2 * j["cap"] + 3 <= 8192
    info = _lib.GelQuantilesInfo()
    L = _lib.lib()
    for args in ((None, 1, 1, 1, C.byref(info)), (host._h, 1, 1, 1, None), (host._h, -1, 1, 1, C.byref(info)), (host._h, 1, -1, 1, C.byref(info)),
                 (host._h, 1, 1, 0, C.byref(info)), (host._h, 1, 1, 17, C.byref(info))):
        assert L.gel_batch_quantiles_info(*args) == GEL_ERR_ARG


# ---------------------------------------------------------------- the truth module alone
def test_keys_are_the_total_order():
    d = 5e-324
    v = np.array([-np.inf, -1e308, -1.0, -2.0 * d, -d, -0.0, 0.0, d, 2.0 * d, 1.0, np.nextafter(1.0, 2.0), 1e308, np.inf])
    k = qt.keys(v)
    assert np.all(k[1:] > k[:-1]) and qt.same(qt.unkeys(k), v)
    assert int(k[6]) - int(k[5]) == 1 and int(k[10]) - int(k[9]) == 1          # -0.0 | +0.0 and 1 | its successor: adjacent keys


def test_truth_against_numpy_lower_and_higher():
    rng = np.random.default_rng(11)
    for n in (2, 3, 65, 257, 1025):
        A = np.stack([rng.standard_normal(n), rng.uniform(-1.0, 1.0, n), np.sort(rng.standard_normal(n))[::-1]], axis=1)
        exact = [k / (n - 1) for k in (0, 1, (n - 1) // 2, n - 2, n - 1)] if (n - 1) & (n - 2) == 0 else [0.0, 1.0]
        for p in exact:                           # p (n - 1) is an integer without rounding: n - 1 is a power of two
            assert np.float64(p) * np.float64(n - 1) == round(p * (n - 1))
        away = [p for p in (0.00135, 0.025, 1.0 / 3.0, 0.3141, 0.975, 0.99865)
                if abs(p * (n - 1) - round(p * (n - 1))) >= 1e-3]
        probs = exact + away
        T = qt.order_stats(A, probs)
        assert T["count"].tolist() == [n] * 3
        lo = np.quantile(A, probs, axis=0, method="lower").T
        hi = np.quantile(A, probs, axis=0, method="higher").T
        assert qt.same(T["lower"], lo) and qt.same(T["upper"], hi), n
        for j, p in enumerate(exact):
            assert qt.same(T["lower"][:, j], T["upper"][:, j])
        assert np.array_equal(A[T["who_lower"], np.arange(3)[:, None]], T["lower"]) and np.array_equal(A[T["who_upper"], np.arange(3)[:, None]], T["upper"])


def test_truth_rejects_a_sort_that_counts_nan():
    rng = np.random.default_rng(12)
    A = rng.standard_normal((41, 1))
    A[[3, 9, 30], 0] = np.nan
    A[5, 0] = np.inf
    T = qt.order_stats(A, [0.5, 0.9, 1.0])
    assert T["count"][0] == 37
    s = np.sort(A[:, 0])                           # numpy puts NaN last and counts it; Inf too
    naive = np.array([[s[int(np.floor(p * 40))] for p in (0.5, 0.9, 1.0)]])
    assert not qt.same(T["lower"], naive)
    assert T["upper"][0, 2] == np.max(A[np.isfinite(A)]) and not np.isfinite(naive[0, 2])


def test_truth_rejects_round_for_floor():
    A = np.arange(11.0)[:, None] * 1.5
    T = qt.order_stats(A, [0.26, 0.74])            # h = 2.6, 7.4
    assert T["lower"][0].tolist() == [3.0, 10.5] and T["upper"][0].tolist() == [4.5, 12.0]
    rounded = [A[qt.ranks(p, 11, lower_of=np.round)[0], 0] for p in (0.26, 0.74)]
    assert rounded == [4.5, 10.5] and rounded != T["lower"][0].tolist()


def test_truth_rejects_equal_and_unordered_zeros():
    A = np.array([0.0, -0.0, 0.0, -0.0, 0.0, 1.0, -1.0, 2.0, -2.0])[:, None]
    T = qt.order_stats(A, [0.25, 0.375, 0.5])      # h = 2, 3, 4 without rounding
    # key order: -2, -1, -0, -0, +0, +0, +0, 1, 2
    assert qt.same(T["lower"][0], [-0.0, -0.0, 0.0]) and qt.same(T["upper"], T["lower"]) and T["who_lower"][0].tolist() == [1, 1, 0]
    by_value = np.sort(A[:, 0], kind="stable")     # a comparison sort of the doubles: -0.0 == 0.0, the zeros keep their order of arrival
    assert not qt.same(by_value[[2, 3, 4]], T["lower"][0]) and np.array_equal(by_value[[2, 3, 4]], T["lower"][0])


def test_lerp_exact_by_hand():
    from fractions import Fraction
    assert qt.lerp_exact(0.5, 4, 1.0, 2.0) == Fraction(3, 2)                   # h = 1.5
    assert qt.lerp_exact(0.25, 5, -3.0, 7.0) == -3                              # h = 1 exactly
    h = np.float64(0.1) * np.float64(7.0)
    assert qt.lerp_exact(0.1, 8, 0.0, 1.0) == Fraction(float(h))                # the fraction is that of the ROUNDED product
    v = Engine.quantile_value([0.5, 0.25], np.array([4, 0]), np.array([[1.0, 1.0], [np.nan, np.nan]]), np.array([[2.0, 1.0], [np.nan, np.nan]]))
    assert v[0].tolist() == [1.5, 1.0] and np.isnan(v[1]).all()

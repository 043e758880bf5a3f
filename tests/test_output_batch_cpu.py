"""gel_output_table_batch* without a GPU: the symbols, every refusal (decided before the device is looked at) on a host-only handle
with its gel_last_error text, the Python layer's argument checks, and the truth module (tests/output_batch_truth.py) on its own: the
exact statistics against numpy, the bound against the stated order restated in Python and against four wrong reductions."""
import ctypes as C
import math

import numpy as np
import pytest

import output_atlas as oa
import output_batch_truth as obt
from conftest import load_golden
from gelato_amd import Engine, _lib

GEL_ERR_ARG, GEL_ERR_HIP = -1, -2          # include/gelato_amd.h


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
    for name in ("gel_output_table_batch", "gel_output_table_batch_device"):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 12
        assert getattr(L, name).restype is C.c_int
    assert (_lib.GEL_ENV_NSTAT, _lib.GEL_PEAK_NSTAT) == (8, 4) == (len(Engine.ENVELOPE_FIELDS), len(Engine.PEAK_FIELDS))
    assert Engine.ENVELOPE_FIELDS == obt.ENV_FIELDS


def _call(E, B, x, cols, out, env, peaks, device_form=False, handle=True, ncols=None):
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    ids = None if cols is None else np.asarray(cols, dtype=np.int32)
    ip = None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int32))
    n = (0 if ids is None else ids.size) if ncols is None else ncols
    h = E._h if handle else None
    if device_form:
        vp = lambda a: None if a is None else a.ctypes.data
        rc = _lib.lib().gel_output_table_batch_device(h, B, vp(x), None, None, 28.5, 0.0, n, ip, vp(out), vp(env), vp(peaks))
    else:
        rc = _lib.lib().gel_output_table_batch(h, B, dp(x), None, None, 28.5, 0.0, n, ip, dp(out), dp(env), dp(peaks))
    return rc, _lib.lib().gel_last_error().decode()


@pytest.mark.parametrize("device_form", [False, True])
def test_refusals_on_a_host_only_handle(host, g, device_form):
    M, nv = host.M, host.nvars
    x = np.ascontiguousarray(np.tile(g["x_big"], (2, 1)))
    out, env, pk = np.zeros((2, M, 34)), np.zeros((M, 34, 8)), np.zeros((2, 34, 4))
    call = lambda *a, **k: _call(host, *a, device_form=device_form, **k)
    cases = [
        (call(2, x, None, out, env, pk, handle=False), "null handle"),
        (call(2, None, None, out, env, pk), "x is NULL with B > 0"),
        (call(-1, x, None, out, env, pk), "B < 0"),
        (call(2, x, [5], out, env, pk, ncols=0), "ncols = 0 outside 1 .. 34"),
        (call(2, x, list(range(34)), out, env, pk, ncols=35), "ncols = 35 outside 1 .. 34"),
        (call(2, x, [5, 34], out, env, pk), "column id 34 out of range (cols[1])"),
        (call(2, x, [-1], out, env, pk), "column id -1 out of range (cols[0])"),
        (call(2, x, [5, 7, 5], out, env, pk), "column id 5 repeated (cols[2])"),
        (call(2, x, None, None, None, None), "no output selected"),
    ]
    for (rc, msg), text in cases:
        assert rc == GEL_ERR_ARG and text in msg, (rc, msg, text)
    # a valid call: what gel_output_table returns on such a handle
    tx, one = np.zeros(M), np.zeros((M, 34))
    rc1 = _lib.lib().gel_output_table(host._h, x.ctypes.data_as(C.POINTER(C.c_double)), tx.ctypes.data_as(C.POINTER(C.c_double)), 28.5, 0.0,
                                      one.ctypes.data_as(C.POINTER(C.c_double)))
    msg1 = _lib.lib().gel_last_error().decode()
    for cols in (None, [32, 3, 0]):
        rc, msg = call(2, x, cols, out[:, :, :3] if cols else out, None, None)
        assert (rc, msg) == (rc1, msg1) and rc == GEL_ERR_HIP and "host-only" in msg
    rc, msg = call(0, None, None, None, env, None)        # B = 0 is valid too: refused for the missing device alone
    assert (rc, msg) == (rc1, msg1)


def test_python_argument_checks(host, g):
    x, M, S = g["x_big"], host.M, host.S
    X = np.tile(x, (3, 1))
    with pytest.raises(ValueError, match="X:"):
        host.output_table_batch(X[:, :-1], 28.5, 0.0)
    with pytest.raises(ValueError, match="X:"):
        host.output_table_batch(X[None], 28.5, 0.0)
    with pytest.raises(ValueError, match="tx:"):
        host.output_table_batch(X, 28.5, 0.0, tx=np.zeros((2, M)))
    with pytest.raises(ValueError, match="tx:"):
        host.output_table_batch(X, 28.5, 0.0, tx=np.zeros(M))
    with pytest.raises(ValueError, match="dispersion:"):
        host.output_table_batch(X, 28.5, 0.0, dispersion=np.ones((3, S, 3)))
    with pytest.raises(ValueError, match="dispersion:"):
        host.output_table_batch(X, 28.5, 0.0, dispersion=np.ones((S, 4)))
    with pytest.raises(TypeError, match="float64"):
        host.output_table_batch(X, 28.5, 0.0, dispersion=np.ones((3, S, 4), dtype=np.float32))
    with pytest.raises(ValueError, match="unknown output column 'mach'"):
        host.output_table_batch(X, 28.5, 0.0, columns=["M", "mach"])
    with pytest.raises(ValueError, match="distinct"):
        host.output_table_batch(X, 28.5, 0.0, columns=["M", "M"])
    with pytest.raises(ValueError, match="distinct"):
        host.output_table_batch(X, 28.5, 0.0, columns=[])
    with pytest.raises(ValueError, match="no output selected"):
        host.output_table_batch(X, 28.5, 0.0, table=False, envelope=False, peaks=False)
    with pytest.raises(_lib.GelatoAmdError, match="host-only"):   # a well-formed call reaches the library
        host.output_table_batch(X, 28.5, 0.0, columns=["Q_alpha", "M"])
    assert host._output_columns(["Q_alpha", "lat_IIP"]) [1].tolist() == [32, 3]


# ---------------------------------------------------------------- the truth module alone
def _altitude_copies(g, B):
    """the altitude column of the 1 + 1e-9 b copies of the atlas vector, from the oracle's geodetic conversion, at eight nodes that
    lie above 100 km: |v|_2 / sqrt(m2) >= 1e6"""
    M, x, tx = 129, g["x_big"], g["tx_big"]
    X = obt.batch_of(x, M, B)
    alt0 = np.array([oa.wp.eci2geodetic(x[M + 3 * i:M + 3 * i + 3] * oa.UNITS["position"], tx[i])[2] for i in range(M)])
    nodes = np.nonzero(alt0 > 1.0e5)[0][:8]
    T = np.array([[[oa.wp.eci2geodetic(X[b, M + 3 * i:M + 3 * i + 3] * oa.UNITS["position"], tx[i])[2]] for i in nodes] for b in range(B)])
    return T                                                   # [B, 8, 1]


def test_exact_statistics_agree_with_numpy():
    rng = np.random.default_rng(7)
    v = rng.standard_normal(300) * 3.0 + 1.0
    st = obt.exact_stats(v)
    assert st["count"] == 300 and st["first_nonfinite"] == -1
    assert abs(st["mean"] - v.mean()) <= 1e-14 and abs(st["m2"] - ((v - v.mean()) ** 2).sum()) <= 1e-10
    assert (st["min"], st["max"], st["argmin"], st["argmax"]) == (v.min(), v.max(), int(v.argmin()), int(v.argmax()))
    assert abs(st["l2"] - np.linalg.norm(v)) <= 1e-12
    assert st["mean"] == math.fsum(v.tolist()) / 300 or abs(st["mean"] - math.fsum(v.tolist()) / 300) <= 2 * obt.U * abs(st["mean"])
    w = v.copy()
    w[[4, 17]] = np.nan, np.inf
    st = obt.exact_stats(w)
    assert st["count"] == 298 and st["first_nonfinite"] == 4
    ok = np.isfinite(w)
    assert abs(st["mean"] - w[ok].mean()) <= 1e-14
    e = obt.exact_stats(np.full(3, np.nan))
    assert e["count"] == 0 and math.isnan(e["mean"]) and e["argmin"] == -1 and e["first_nonfinite"] == 0
    # exactness where fp64 summation is not: 1e16 + 1 - 1e16
    assert obt.exact_stats(np.array([1e16, 1.0, -1e16]))["mean"] == 1.0 / 3.0


@pytest.mark.parametrize("B", [1, 2, 65, 256, 257, 600])
def test_bound_accepts_the_stated_order(B):
    T = _stated_order_table(B)
    env = obt.envelope_of(T)
    share = obt.check_envelope(T, env, std=obt.std_of(env[:, :, 0], env[:, :, 2]))
    assert all(s <= 1.0 for s in share.values())
    if B > 2:
        assert env[0, 1, 6] == 0.0
    assert env[1, 1, 0] == 0.0 and env[1, 1, 7] == 0.0 and np.isnan(env[1, 1, 1:5]).all() and (env[1, 1, 5:7] == -1.0).all()
    if B == 1:
        assert np.all(env[[0, 2], :3, 2] == 0.0)


def _stated_order_table(B):
    """the table of test_bound_accepts_the_stated_order and of the exact restatement's checks: [B, 3 nodes, 4 columns]"""
    rng = np.random.default_rng(B)
    T = np.empty((B, 3, 4))
    T[:, :, 0] = 6.4e6 * (1.0 + 1e-9 * np.arange(B))[:, None]              # nearly constant: |v|_2 / sqrt(m2) large
    T[:, :, 1] = rng.standard_normal((B, 3))
    T[:, :, 2] = rng.standard_normal((B, 3)) * 1e-3 + 180.0
    T[:, :, 3] = np.where(rng.random((B, 3)) < 0.3, np.nan, rng.standard_normal((B, 3)) * 50.0)
    T[:, 1, 1] = np.nan                                                     # a count == 0 pair
    if B > 2:
        T[2, 0, 1] = T[0, 0, 1] = T[:, 0, 1].max() + 1.0                    # a tie for the maximum: the lower index
    return T


def test_fma_is_one_rounding():
    """obt.fma against cases worked by hand: the product's low bits survive into the sum, ties go to even"""
    e = 2.0 ** -30
    assert obt.fma(1.0 + e, 1.0 - e, -1.0) == -(2.0 ** -60) and (1.0 + e) * (1.0 - e) - 1.0 == 0.0
    assert obt.fma(2.0 ** -53, 1.0, 1.0) == 1.0 and obt.fma(2.0 ** -53, 3.0, 1.0) == 1.0 + 2.0 ** -51      # ties to even, both ways
    assert obt.fma(0.1, 10.0, -1.0) == 2.0 ** -54 and obt.fma(3.0, 4.0, 5.0) == 17.0


@pytest.mark.parametrize("B", [1, 2, 65, 256, 257, 600])
def test_exact_restatement_inside_the_bound_and_apart_from_its_neighbours(B):
    """welford_merge_exact (the header's order with a correctly rounded fma) stays inside bounds() on the tables of
    test_bound_accepts_the_stated_order, gives the exact fields of welford_merge, and is told apart by its bits: from the no-fma
    welford_merge in m2 (B >= 65), and from the variant whose Chan mean update is contracted into one fma (B >= 257: there is a
    merge) -- so a bit-for-bit comparison with it holds the device to each written rounding."""
    T = _stated_order_table(B)
    exact = obt.envelope_of(T, obt.welford_merge_exact)
    share = obt.check_envelope(T, exact, std=obt.std_of(exact[:, :, 0], exact[:, :, 2]))
    assert all(s <= 1.0 for s in share.values())
    plain = obt.envelope_of(T)
    for j, f in enumerate(obt.ENV_FIELDS):
        if f in obt.EXACT_FIELDS:
            assert np.array_equal(exact[:, :, j], plain[:, :, j], equal_nan=True), f
    m2_bits = int((exact[:, :, 2] != plain[:, :, 2]).sum())          # (NaN != NaN does not count: the count == 0 pair is excluded below)
    m2_bits -= int(np.isnan(exact[:, :, 2]).sum())
    contracted = obt.envelope_of(T, lambda v: obt.welford_merge_exact(v, contract_merge=True))
    fin = exact[:, :, 0] > 0
    mean_bits = int((contracted[:, :, 1][fin] != exact[:, :, 1][fin]).sum())
    contracted_m2 = obt.envelope_of(T, lambda v: obt.welford_merge_exact(v, contract_merge="m2"))
    assert np.array_equal(contracted_m2[:, :, [0, 1, 3, 4, 5, 6, 7]], exact[:, :, [0, 1, 3, 4, 5, 6, 7]], equal_nan=True)
    cm2_bits = int((contracted_m2[:, :, 2][fin] != exact[:, :, 2][fin]).sum())
    print("B = %d: m2 differs from the no-fma order in %d of %d pairs, mean from the contracted merge in %d, m2 from the merge with a "
          "contracted m2 in %d" % (B, m2_bits, int(fin.sum()), mean_bits, cm2_bits))
    if B <= 256:      # (with merges it shows where the blocks' means lie apart, as on the trending columns of tests/test_output_batch.py's
        assert cm2_bits == 0      # batch: counted there, restatement against restatement; these columns' blocks have nearly one mean)
    if B >= 65:
        assert m2_bits >= 1
    if B <= 256:
        assert mean_bits == 0 and np.array_equal(contracted, exact, equal_nan=True)          # one block: no merge to contract
    elif B == 600:               # (B = 257 merges ONE entry into 256: d / 257 seldom lands on a tie among eleven pairs)
        assert mean_bits >= 1
    if B <= 2:
        assert np.all(exact[:, :, 2][fin] >= 0.0)


def test_bound_rejects_the_sum_of_squares_formula(g):
    T = _altitude_copies(g, 64)
    st = obt.exact_stats(T[:, 0, 0])
    assert st["l2"] / math.sqrt(st["m2"]) >= 1e6
    good = obt.envelope_of(T)
    obt.check_envelope(T, good)

    def textbook(v):
        r = obt.welford_merge(v)
        v = np.asarray(v, dtype=np.float64)
        r[2] = float(np.sum(v * v) - v.size * np.mean(v) ** 2)
        return r
    bad = obt.envelope_of(T, textbook)
    assert not np.array_equal(bad[:, :, 2], good[:, :, 2])
    with pytest.raises(AssertionError):
        obt.check_envelope(T, bad)


def test_bound_rejects_nan_as_zero_last_tie_and_count_in_std():
    rng = np.random.default_rng(3)
    T = rng.standard_normal((40, 2, 2)) + 5.0
    T[7, 0, 0] = np.nan
    T[9, 1, 1] = T[3, 1, 1] = T[:, 1, 1].min() - 1.0               # a tie for the minimum
    good = obt.envelope_of(T)
    obt.check_envelope(T, good, std=obt.std_of(good[:, :, 0], good[:, :, 2]))
    assert good[1, 1, 5] == 3.0 and good[0, 0, 7] == 7.0 and good[0, 0, 0] == 39.0
    # NaN entries counted as zeros
    bad = obt.envelope_of(np.nan_to_num(T, nan=0.0))
    with pytest.raises(AssertionError):
        obt.check_envelope(T, bad)
    # the same with the count put right: the mean still carries the zero
    bad[0, 0, 0], bad[0, 0, 7] = 39.0, 7.0
    with pytest.raises(AssertionError, match="mean|min"):
        obt.check_envelope(T, bad)
    # ties resolved to the last index
    bad = good.copy()
    bad[1, 1, 5] = 9.0
    with pytest.raises(AssertionError, match="argmin"):
        obt.check_envelope(T, bad)
    # count in place of count - 1
    with pytest.raises(AssertionError, match="std"):
        obt.check_envelope(T, good, std=np.sqrt(good[:, :, 2] / good[:, :, 0]))


def test_peaks_restatement_by_hand():
    nan = math.nan
    T = np.array([[[1.0, nan], [nan, nan], [1.0, nan], [3.0, nan]],          # ties: node 0; a column NaN at every node
                  [[nan, 2.0], [5.0, 2.0], [5.0, -1.0], [nan, math.inf]],    # first finite at node 1; Inf is not finite
                  [[7.0, 0.0], [6.0, -0.0], [8.0, 0.0], [6.0, 0.0]]])        # -0.0 == 0.0: the first node
    P = obt.peaks_reference(T)
    want = np.array([[[1.0, 0, 3.0, 3], [nan, -1, nan, -1]],
                     [[5.0, 1, 5.0, 1], [-1.0, 2, 2.0, 0]],
                     [[6.0, 1, 8.0, 2], [0.0, 0, 0.0, 0]]])
    assert np.array_equal(P, want, equal_nan=True)

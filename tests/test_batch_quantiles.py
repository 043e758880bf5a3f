"""gel_batch_quantiles* on the GPU (include/gelato_amd.h) against a plain sort of the keys (tests/quantile_truth.py):
every comparison is bit for bit -- order statistics have no tolerance.  One synthetic source whose columns are built to drive every
path (the range pass alone, the candidate buffers, the bisection over the column), at batch sizes and widths on both sides of every
threshold gel_batch_quantiles_info reports; the device's own batch table through its views; independence of a column from its
neighbours and of the order of the vectors; host form, device form and repeated calls; the Python layer."""
import ctypes as C

import numpy as np
import pytest

import output_atlas as oa
import output_batch_truth as obt
import quantile_truth as qt
from conftest import load_golden
from gelato_amd import Engine, _lib
from quantile_truth import same

pytestmark = pytest.mark.gpu

LAT, LON = oa.LAUNCH_LAT, oa.LAUNCH_LON
PROBS = [0.0, 0.00135, 0.025, 1.0 / 3.0, 0.5, 0.975, 0.99865, 1.0]
MS = {"big": 129, "m64": 64, "m3": 3}
_dp = C.POINTER(C.c_double)
COLUMNS = ("normal", "uniform", "constant", "all_nan", "one_finite", "two_finite", "zeros_denormals", "with_inf", "adjacent", "half_zero",
           "outlier", "overflow", "ascending", "descending", "permuted")
NINE = ("normal", "uniform", "constant", "all_nan", "zeros_denormals", "adjacent", "half_zero", "outlier", "overflow")


def source(B, seed=0, names=COLUMNS):
    """[B, len(names)]: the synthetic columns, in the order of `names`"""
    rng = np.random.default_rng(1000 * seed + B)
    d = 5e-324
    normal = rng.standard_normal(B)
    c = {"normal": normal, "uniform": rng.uniform(-1.0, 1.0, B), "constant": np.full(B, 3.25 + seed), "all_nan": np.full(B, np.nan)}
    one = np.full(B, np.nan)
    one[B // 2] = -7.5
    two = one.copy()
    two[(B // 2 + 1) % B] = 2.5                                                    # (B = 1: the same entry again)
    c["one_finite"], c["two_finite"] = one, two
    c["zeros_denormals"] = rng.choice(np.array([-0.0, 0.0, d, -d, 2 * d, -2 * d, 3 * d]), B)
    w = rng.standard_normal(B)
    w[rng.random(B) < 0.2] = np.inf
    w[rng.random(B) < 0.2] = -np.inf
    w[rng.random(B) < 0.1] = np.nan
    c["with_inf"] = w
    c["adjacent"] = (np.float64(1.0).view(np.uint64) + rng.integers(0, 4, B).astype(np.uint64)).view(np.float64)   # 1 + k ulp
    h = rng.standard_normal(B) * 5.0
    h[rng.permutation(B)[:(B + 1) // 2]] = 0.0
    c["half_zero"] = h
    o = rng.standard_normal(B) * 1e-300
    if B > 1:
        o[B // 3] = 1e300
    c["outlier"] = o
    v = rng.standard_normal(B)
    if B > 1:
        v[0], v[B - 1] = -1e308, 1e308
    c["overflow"] = v
    c["ascending"] = np.sort(rng.standard_normal(B))
    c["descending"] = c["ascending"][::-1] * 2.0
    c["permuted"] = normal[rng.permutation(B)]
    return np.ascontiguousarray(np.stack([c[n] for n in names], axis=1))


def wide_source(B, W):
    """[B, W]: the synthetic columns again and again, from other seeds"""
    blocks = [source(B, seed=s) for s in range(-(-W // len(COLUMNS)))]
    return np.ascontiguousarray(np.concatenate(blocks, axis=1)[:, :W])


def check_against_truth(R, A, probs, who=True):
    T = qt.order_stats(A, probs)
    assert np.array_equal(R["count"], T["count"])
    bad = [w for w in range(T["count"].size) if not (same(R["lower"][w], T["lower"][w]) and same(R["upper"][w], T["upper"][w]))]
    assert not bad, ("columns", bad[:10], R["lower"][bad[0]], T["lower"][bad[0]], R["upper"][bad[0]], T["upper"][bad[0]])
    if who:
        assert np.array_equal(R["who_lower"], T["who_lower"]) and np.array_equal(R["who_upper"], T["who_upper"])
    return T


@pytest.fixture(scope="module")
def g():
    return load_golden(oa.FIXTURE)


@pytest.fixture(scope="module")
def engines(g):
    E = {h: Engine(oa.prob_arrays(nodes, g["wind"], g["ca"])) for h, nodes in oa.HANDLES.items()}
    yield E
    for e in E.values():
        e.close()


@pytest.fixture(scope="module")
def E(engines):
    return engines["m3"]


def raw(E, A, W, ld, offset, probs, who=True):
    """the host form on a view of A: columns offset .. offset + W - 1 of rows of ld doubles"""
    flat = A.reshape(-1)
    B = (flat.size - offset - W) // ld + 1 if flat.size else 0
    p = np.asarray(probs, dtype=np.float64)
    q, cnt, wh = np.full((W, p.size, 2), -3.0), np.full(W, -3.0), np.full((W, p.size, 2), -3.0)
    src = C.cast(flat.ctypes.data + 8 * offset, _dp)
    rc = _lib.check(_lib.lib().gel_batch_quantiles(E._h, B, W, ld, src, p.size, p.ctypes.data_as(_dp), q.ctypes.data_as(_dp), cnt.ctypes.data_as(_dp),
                                                   wh.ctypes.data_as(_dp) if who else None))
    assert rc == 0
    return {"count": cnt.astype(np.int64), "lower": q[:, :, 0], "upper": q[:, :, 1], "who_lower": wh[:, :, 0].astype(np.int64),
            "who_upper": wh[:, :, 1].astype(np.int64)}


# ------------------------------------------------------------------ 1. the synthetic columns at every batch size
@pytest.mark.parametrize("B", [1, 2, 3, 63, 64, 65, 255, 256, 257, 600])
def test_synthetic_columns(E, B):
    A = source(B)
    R = E.batch_quantiles(A, PROBS, who=True)
    T = check_against_truth(R, A, PROBS)
    k = {n: i for i, n in enumerate(COLUMNS)}
    assert T["count"][k["all_nan"]] == 0 and T["count"][k["one_finite"]] == 1 and T["count"][k["two_finite"]] == min(B, 2)
    assert np.isnan(R["lower"][k["all_nan"]]).all() and (R["who_upper"][k["all_nan"]] == -1).all() and np.isnan(R["value"][k["all_nan"]]).all()
    # a permutation of a column: the same answers, from other vectors
    assert same(R["lower"][k["permuted"]], R["lower"][k["normal"]]) and same(R["upper"][k["permuted"]], R["upper"][k["normal"]])
    if B >= 63:
        assert not np.array_equal(R["who_lower"][k["permuted"]], R["who_lower"][k["normal"]])
        assert R["who_lower"][k["ascending"]].tolist() == sorted(R["who_lower"][k["ascending"]].tolist())
        assert R["who_lower"][k["descending"]].tolist() == sorted(R["who_lower"][k["descending"]].tolist(), reverse=True)
    st = E.batch_quantiles_last()
    assert st["targets"] == 2 * len(PROBS) * len(COLUMNS) == st["by_range"] + st["by_candidates"] + st["by_fallback"]


def test_batch_sizes_at_the_thresholds(E):
    """chunk - 1, chunk, chunk + 1 vectors (one workgroup of a pass, then two), cap and cap + 1 (a column that fits one candidate
    buffer whole, then does not), for the narrow source and for one wide enough to take the long chunk"""
    narrow = E.batch_quantiles_info(600, len(COLUMNS), len(PROBS))
    probs = [0.0, 0.3, 1.0]
    wide_w = 64 * 16
    wide = E.batch_quantiles_info(600, wide_w, len(probs))
    assert wide["slabs"] == 1 and wide["chunk"] > narrow["chunk"] and E.batch_quantiles_info(600, wide_w - 64, len(probs))["chunk"] == narrow["chunk"]
    for B in sorted({narrow["chunk"] - 1, narrow["chunk"], narrow["chunk"] + 1, narrow["cap"], narrow["cap"] + 1}):
        A = source(B)
        check_against_truth(E.batch_quantiles(A, PROBS, who=True), A, PROBS)
    for B in (wide["chunk"] - 1, wide["chunk"], wide["chunk"] + 1):
        A = wide_source(B, wide_w)
        check_against_truth(E.batch_quantiles(A, probs, who=True), A, probs)


# ------------------------------------------------------------------ 2. the paths
def test_every_path_is_taken_where_it_must_be(E):
    """B = 2 cap + 3 with nine columns: the whole call against the truth, then column by column (a W = 1 view) how its targets were settled"""
    info = E.batch_quantiles_info(1, len(NINE), len(PROBS))
    cap, B, T = info["cap"], 2 * info["cap"] + 3, 2 * len(PROBS)
    A = source(B, names=NINE)
    check_against_truth(E.batch_quantiles(A, PROBS, who=True), A, PROBS)
    took = {}
    for i, name in enumerate(NINE):
        R = raw(E, A, 1, len(NINE), i, PROBS)
        check_against_truth(R, A[:, i], PROBS)
        took[name] = E.batch_quantiles_last()
        assert took[name]["targets"] == T
    print(took)
    for name in ("normal", "uniform"):                       # smooth: every bin far below the cap
        assert took[name]["by_candidates"] == T and took[name]["by_fallback"] == 0, (name, took[name])
    for name in ("constant", "all_nan"):
        assert took[name]["by_range"] == T, (name, took[name])
    # vmax - vmin overflows: one bin holds all B > cap entries
    assert took["overflow"]["by_fallback"] == T, took["overflow"]
    # 1e300 beside 1e-300-scale noise: B - 1 > cap entries in the lowest bin; only p = 1 (both ranks) finds the outlier's own bin
    assert took["outlier"]["by_fallback"] == T - 2 and took["outlier"]["by_candidates"] == 2, took["outlier"]
    # cap + 2 exact zeros: the ranks inside them (1/3 and 1/2, both sides) cannot be gathered; the extremes can
    nz = int((A[:, NINE.index("half_zero")] == 0.0).sum())
    assert nz > cap and took["half_zero"]["by_fallback"] >= 4 and took["half_zero"]["by_candidates"] >= 4, (nz, took["half_zero"])
    # seven values around zero, five denormal steps apart: bins / range is no finite number, so one bin holds all B entries
    assert took["zeros_denormals"]["by_fallback"] == T, took["zeros_denormals"]
    # four adjacent keys, three ulps apart: four bins of about B / 4 < cap ties each
    assert took["adjacent"]["by_candidates"] == T, took["adjacent"]


@pytest.mark.parametrize("probs", [[0.5], [0.99865], list(np.linspace(0.0, 1.0, 16))])
def test_one_and_sixteen_probabilities(E, probs):
    for B in (3, 257):
        A = source(B)
        check_against_truth(E.batch_quantiles(A, probs, who=True), A, probs)


def test_empty_batch_and_empty_width(E):
    R = E.batch_quantiles(np.zeros((0, 5)), PROBS, who=True)
    assert (R["count"] == 0).all() and np.isnan(R["lower"]).all() and np.isnan(R["upper"]).all() and np.isnan(R["value"]).all()
    assert (R["who_lower"] == -1).all() and (R["who_upper"] == -1).all() and R["lower"].shape == (5, len(PROBS))
    R = E.batch_quantiles(np.zeros((4, 0)), PROBS, who=True)
    assert R["count"].shape == (0,) and R["lower"].shape == (0, len(PROBS))
    assert E.batch_quantiles_last()["targets"] == 0


# ------------------------------------------------------------------ 3. widths
@pytest.mark.parametrize("W", [1, 4, 63, 64, 65, 136])
def test_widths(E, W):
    for B in (65, 257):
        A = wide_source(B, W)
        check_against_truth(E.batch_quantiles(A, PROBS, who=True), A, PROBS)


def test_slab_boundary(E):
    """sixteen probabilities: the narrowest slab; one column less, exactly one slab, one column into the second"""
    probs = list(np.linspace(0.0, 1.0, 16))
    slab = E.batch_quantiles_info(65, 1 << 20, 16)["slab_cols"]
    assert slab <= 1024
    A = wide_source(65, slab + 1)
    for W in (slab - 1, slab, slab + 1):
        assert E.batch_quantiles_info(65, W, 16)["slabs"] == (2 if W > slab else 1)
        a = np.ascontiguousarray(A[:, :W])
        check_against_truth(E.batch_quantiles(a, probs, who=True), a, probs)


# ------------------------------------------------------------------ 4. the device's own batch table, through its views
def _batch(g, handle, B):
    """as tests/test_output_batch.py builds it: vector 0 plus the 1 + 1e-9 b copies; node 70 of vector 1 NaN (big handle)"""
    M = MS[handle]
    X = obt.batch_of(g["x_" + handle], M, B)
    if handle == "big" and B > 1:
        obt.nan_node(X, 1, 70, M)
    TX = np.tile(g["tx_" + handle], (B, 1)) + 0.25 * np.arange(B)[:, None]
    return X, TX


@pytest.mark.parametrize("handle,B", [("big", 600), ("big", 257), ("m64", 600), ("m64", 257), ("m3", 600), ("m3", 257)])
def test_the_batch_table(g, engines, handle, B):
    Eh, M, nc = engines[handle], MS[handle], 34
    X, TX = _batch(g, handle, B)
    out = Eh.output_table_batch(X, LAT, LON, tx=TX)
    table = out["table"]
    assert table.shape == (B, M, nc)
    R = Eh.batch_quantiles(table, PROBS, who=True)                                  # W = ld = M ncols (129 * 34 on the big handle)
    check_against_truth(R, table.reshape(B, -1), PROBS)
    i0, i1 = PROBS.index(0.0), PROBS.index(1.0)
    for k, name in enumerate(out["columns"]):
        e = out["envelope"][name]
        sl = slice(k, M * nc, nc)
        assert np.array_equal(R["count"][sl], e["count"]), name
        assert same(R["lower"][sl, i0], e["min"]) and same(R["upper"][sl, i1], e["max"]), name
        assert np.array_equal(R["who_lower"][sl, i0], e["argmin"]) and np.array_equal(R["who_upper"][sl, i1], e["argmax"]), name
    last = raw(Eh, table, nc, M * nc, (M - 1) * nc, PROBS)                          # the last node's row through the ld view
    check_against_truth(last, table[:, M - 1, :], PROBS)
    for f in ("count", "lower", "upper", "who_lower", "who_upper"):
        assert same(last[f], R[f][(M - 1) * nc:]), f
    pk = np.stack([np.stack([np.asarray(out["peaks"][c][f], dtype=np.float64) for f in Engine.PEAK_FIELDS], axis=-1) for c in out["columns"]], axis=1)
    Rp = Eh.batch_quantiles(pk, PROBS, who=True)                                    # W = ld = 4 ncols
    check_against_truth(Rp, pk.reshape(B, -1), PROBS)


# ------------------------------------------------------------------ 5. independence
def test_column_alone_and_rows_permuted(E):
    B, W = 257, 70
    A = wide_source(B, W)
    R = E.batch_quantiles(A, PROBS, who=True)
    for w in (0, 3, 9, 11, 63, 64, 69):
        one = raw(E, A, 1, W, w, PROBS)                                             # a view of that column alone
        for f in ("count", "lower", "upper", "who_lower", "who_upper"):
            assert same(one[f][0], R[f][w]), (w, f)
    perm = np.random.default_rng(3).permutation(B)
    A2 = np.ascontiguousarray(A[perm])
    R2 = E.batch_quantiles(A2, PROBS, who=True)
    for f in ("count", "lower", "upper"):
        assert same(R2[f], R[f]), f
    check_against_truth(R2, A2, PROBS)
    inv = np.argsort(perm)                                                          # where a vector of A went
    distinct = [w for w in range(W) if COLUMNS[w % len(COLUMNS)] in ("normal", "uniform", "ascending", "descending", "permuted")]
    assert np.array_equal(R2["who_lower"][distinct], inv[R["who_lower"][distinct]])
    assert np.array_equal(R2["who_upper"][distinct], inv[R["who_upper"][distinct]])


# ------------------------------------------------------------------ 6. forms and memory
def test_host_form_device_form_second_call(E):
    import torch
    B, W, ld = 300, 40, 47
    A = wide_source(B, ld)
    p = np.asarray(PROBS)
    H = raw(E, A, W, ld, 3, PROBS)
    check_against_truth(H, A[:, 3:3 + W], PROBS)
    H2 = raw(E, A, W, ld, 3, PROBS)
    dA = torch.from_numpy(A).cuda()
    for turn in range(2):
        dq = torch.full((W, p.size, 2), -3.0, dtype=torch.float64, device="cuda")
        dc = torch.full((W,), -3.0, dtype=torch.float64, device="cuda")
        dw = torch.full((W, p.size, 2), -3.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        E.batch_quantiles_device(B, W, ld, dA.data_ptr() + 8 * 3, p, dq.data_ptr(), dc.data_ptr(), dw.data_ptr() if turn == 0 else 0)
        assert E.sync() == 0                                                        # NaN and Inf in the source never raise the status
        q, c, w = dq.cpu().numpy(), dc.cpu().numpy(), dw.cpu().numpy()
        assert same(q[:, :, 0], H["lower"]) and same(q[:, :, 1], H["upper"]) and np.array_equal(c.astype(np.int64), H["count"])
        if turn == 0:
            assert np.array_equal(w[:, :, 0].astype(np.int64), H["who_lower"]) and np.array_equal(w[:, :, 1].astype(np.int64), H["who_upper"])
        else:
            assert (w == -3.0).all()                                                # who not asked for: not written
    for f in H:
        assert same(H[f], H2[f]), f


def test_arena_shared_with_rows_eval(g):
    x = g["x_big"]
    B = 96
    X = obt.batch_of(x, 129, B)
    A = wide_source(B, 200)
    Eb = Engine(oa.prob_arrays(oa.NODES, g["wind"], g["ca"]))
    Eb.rows_configure([], [("orbit_energy", 5, 1.0e6, 0.0), ("radius", 70, 6.4e6, 1.0), ("speed", 128, 1.0e3, 0.0)])
    q0 = Eb.batch_quantiles(A, PROBS, who=True)
    r0 = Eb.rows_eval(X)
    q1 = Eb.batch_quantiles(A, PROBS, who=True)
    r1 = Eb.rows_eval(X)
    Eb.close()
    Ec = Engine(oa.prob_arrays(oa.NODES, g["wind"], g["ca"]))
    Ec.rows_configure([], [("orbit_energy", 5, 1.0e6, 0.0), ("radius", 70, 6.4e6, 1.0), ("speed", 128, 1.0e3, 0.0)])
    r2 = Ec.rows_eval(X)
    Ec.close()
    check_against_truth(q0, A, PROBS)
    for f in q0:
        assert same(q0[f], q1[f]), f
    for a, b in ((r0, r1), (r0, r2)):
        assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True) and a[2] == b[2]


# ------------------------------------------------------------------ 7. the Python layer
def test_interpolated_value(E):
    """"value" lies inside [lower, upper] and within 6 u max(|lower|, |upper|) of the exact interpolation: three roundings (the
    difference, the product, the sum), each of a quantity of at most 2 max(|lower|, |upper|)"""
    B = 257
    names = ("normal", "uniform", "constant", "one_finite", "two_finite", "zeros_denormals", "with_inf", "adjacent", "half_zero", "ascending")
    A = source(B, names=names)
    probs = [0.0, 0.00135, 0.025, 1.0 / 3.0, 0.5, 0.7, 0.975, 0.99865, 1.0]
    R = E.batch_quantiles(A, probs)
    assert "who_lower" not in R and same(R["probs"], probs)
    lo, up, v = R["lower"], R["upper"], R["value"]
    assert np.all((v >= lo) & (v <= up))
    interior = 0
    for w in range(len(names)):
        for j, p in enumerate(probs):
            exact = qt.lerp_exact(p, int(R["count"][w]), lo[w, j], up[w, j])
            bound = 6.0 * qt.U * max(abs(lo[w, j]), abs(up[w, j]))
            assert abs(float(exact - qt.Fraction(float(v[w, j])))) <= bound, (names[w], p, v[w, j], float(exact))
            interior += int(lo[w, j] < v[w, j] < up[w, j])
    assert interior >= 10


def test_flight_quantiles():
    from gelato_amd import con_dynamics, montecarlo, pack_x, problem, propagate
    pdict, unitdict, _cond, xdict = problem.make_problem("example")
    S, ps = pdict["num_sections"], pdict["ps_params"]
    Ee = Engine(con_dynamics.problem_arrays(pdict, unitdict), D=[ps.D(i) for i in range(S)], tau=[ps.tau(i) for i in range(S)])
    lc = pdict["LaunchCondition"]
    B = 64
    X = np.tile(pack_x(xdict), (B, 1))
    D = propagate.sample_dispersion(B, S, [0.02, 0.01, 0.03, 0.2], seed=4)
    cols = ["altitude", "dynamic_pressure", "Q_alpha", "M", "lat_IIP", "inclination"]
    probs = [0.00135, 0.5, 0.99865]
    Q = montecarlo.flight_quantiles(X, pdict, unitdict, probs, dispersion=D, steps=1, columns=cols, engine=Ee)
    env = montecarlo.flight_envelope(X, pdict, unitdict, dispersion=D, steps=1, columns=cols, engine=Ee)
    assert Q["columns"] == cols and Q["steps"] == env["steps"] == 2 and Q["status"] == env["status"] and same(Q["probs"], probs)
    T = Ee.output_table_batch(env["x_flown"], lc["lat"], lc["lon"], dispersion=D, columns=cols, envelope=False)
    M, nc = Ee.M, len(cols)
    Rn = Ee.batch_quantiles(T["table"], probs)
    pk = np.stack([np.stack([np.asarray(T["peaks"][c][f], dtype=np.float64) for f in Engine.PEAK_FIELDS], axis=-1) for c in cols], axis=1)
    Rp = Ee.batch_quantiles(pk, probs, who=True)
    for k, c in enumerate(cols):
        for f in ("lower", "upper", "value"):
            assert same(Q["node"][c][f], Rn[f].reshape(M, nc, -1)[:, k]), (c, f)
        assert np.array_equal(Q["node"][c]["count"], Rn["count"].reshape(M, nc)[:, k])
        for j, side in ((0, "min"), (2, "max")):
            for f in ("lower", "upper", "value", "who_lower", "who_upper"):
                assert same(Q["peak"][c][side][f], Rp[f].reshape(nc, 4, -1)[k, j]), (c, side, f)
            assert Q["peak"][c][side]["count"] == Rp["count"].reshape(nc, 4)[k, j]
    q99, b99 = Q["peak"]["dynamic_pressure"]["max"]["upper"][2], Q["peak"]["dynamic_pressure"]["max"]["who_upper"][2]
    assert T["peaks"]["dynamic_pressure"]["max"][b99] == q99 and q99 > Q["peak"]["dynamic_pressure"]["max"]["lower"][0]
    Tm = qt.order_stats(env["terminal_miss"], probs)
    assert same(Q["terminal_miss"]["lower"], Tm["lower"]) and same(Q["terminal_miss"]["upper"], Tm["upper"])
    assert np.array_equal(Q["terminal_miss"]["count"], Tm["count"]) and Q["terminal_miss"]["value"].shape == (4, 3)
    Ee.close()

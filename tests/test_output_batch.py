"""gel_output_table_batch* on the device: the table bit for bit the single-vector call's on the atlas handles
(M = 129 / 64 / 3), with all columns, a scrambled subset and one column; the node times formed on the device; the dispersion factors
against handles built with the scaled parameters (bits) and against the oracle (values); peaks and the exact envelope fields against
numpy on the device's own table; mean and m2 against the exactly rounded values under the bound derived in
tests/output_batch_truth.py; host form = device form = second call, with or without the table; the handle's arena between two
gel_rows_eval calls; gelato_amd.montecarlo.flight_envelope.

Batch sizes: 1, 2, 3, 64, 65, 67 (one envelope block), 256 and 257 (the block size and one more), 600 (three blocks: the merge runs
twice).  Largest share of the bound the device used (MI355X, recorded in DESIGN.md 3.16): mean 0.50, m2 0.26, std 0.18.

The envelope's node groups of 8 also on M = 64 and M = 3, with and without a table; and at B = 600 mean and m2 bit for bit the stated
order restated with a correctly rounded fma (output_batch_truth.welford_merge_exact): the header's order is the contract, not only a
bound around the exact statistics.  The long wind and CA tables: tests/test_table_sizes_outbatch.py."""
import numpy as np
import pytest

import output_atlas as oa
import output_batch_truth as obt
from conftest import load_golden
from gelato_amd import Engine
from test_output_table import TOL

pytestmark = pytest.mark.gpu

LAT, LON = oa.LAUNCH_LAT, oa.LAUNCH_LON
SUBSET = ["Q_alpha", "lat_IIP", "thrust", "downrange", "M"]
MS = {"big": 129, "m64": 64, "m3": 3}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """bit for bit (a -0.0 is not a 0.0), NaN where the other has NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(_bits(a)[~na], _bits(b)[~nb]))


@pytest.fixture(scope="module")
def g():
    return load_golden(oa.FIXTURE)


@pytest.fixture(scope="module")
def engines(g):
    E = {h: Engine(oa.prob_arrays(nodes, g["wind"], g["ca"])) for h, nodes in oa.HANDLES.items()}
    yield E
    for e in E.values():
        e.close()


def _batch(g, handle, B):
    """vector 0 plus the 1 + 1e-9 b copies; node 70 of vector 1 NaN (big handle, B > 1), and the node times per vector"""
    M = MS[handle]
    X = obt.batch_of(g["x_" + handle], M, B)
    if handle == "big" and B > 1:
        obt.nan_node(X, 1, 70, M)
    TX = np.tile(g["tx_" + handle], (B, 1)) + 0.25 * np.arange(B)[:, None]
    return X, TX


_SINGLE = {}


def single_tables(g, engines, handle, B):
    """Engine.output_table of every vector of _batch(handle, B): computed once per (handle, vector)"""
    X, TX = _batch(g, handle, B)
    have = _SINGLE.setdefault(handle, [])
    for b in range(len(have), B):
        have.append(engines[handle].output_table(X[b], TX[b], LAT, LON))
    return np.stack(have[:B])


@pytest.fixture(scope="module")
def full(g, engines):
    """the call with everything on the big handle, per batch size: computed once, shared, left unchanged"""
    cache = {}

    def get(B):
        if B not in cache:
            X, TX = _batch(g, "big", B)
            cache[B] = engines["big"].output_table_batch(X, LAT, LON, tx=TX)
        return cache[B]
    return get


# ------------------------------------------------------------------ 1. table bits
@pytest.mark.parametrize("handle,B", [("big", 1), ("big", 2), ("big", 3), ("big", 64), ("big", 65), ("big", 257), ("m64", 3), ("m64", 65), ("m3", 1), ("m3", 65)])
def test_table_bits(g, engines, handle, B):
    E = engines[handle]
    X, TX = _batch(g, handle, B)
    ref = single_tables(g, engines, handle, B)
    assert int(np.isnan(ref).sum()) > 0 or handle != "big"
    T = E.output_table_batch(X, LAT, LON, tx=TX, envelope=False, peaks=False)
    assert T["columns"] == Engine.OUTPUT_COLUMNS and T["envelope"] is None and T["peaks"] is None
    assert same(T["table"], ref)
    for cols in (SUBSET, ["vel_air"], ["lat_IIP"], ["altitude_perigee", "lon"]):
        S = E.output_table_batch(X, LAT, LON, tx=TX, columns=cols, envelope=False, peaks=False)
        assert S["columns"] == cols
        assert same(S["table"], ref[:, :, [Engine.OUTPUT_COLUMNS.index(c) for c in cols]]), cols


# ------------------------------------------------------------------ 2. times
def test_node_times_formed_on_the_device(g):
    """tx = None: the expression of output_result.node_times with the handle's own tau, vectors with different knot times"""
    from gelato_amd import output_result as orr
    from gelato_amd.SectionParameters import PSparams
    ps, S, B = PSparams(oa.NODES), len(oa.NODES), 5
    E = Engine(oa.prob_arrays(oa.NODES, g["wind"], g["ca"]), D=[ps.D(i) for i in range(S)], tau=[ps.tau(i) for i in range(S)])
    X, _ = _batch(g, "big", B)
    rng = np.random.default_rng(11)
    for b in range(B):
        X[b, -(S + 1):] = np.sort(rng.random(S + 1) * (3.0 + b)) - 0.4
    pdict = oa.pdict_of(oa.NODES, g["wind"], g["ca"], ps)
    TX = np.stack([orr.node_times(oa.xdict_of(X[b], 129, 125, S), dict(oa.UNITS), pdict)[0] for b in range(B)])
    assert len({tuple(t) for t in TX}) == B
    a = E.output_table_batch(X, LAT, LON)
    b_ = E.output_table_batch(X, LAT, LON, tx=TX)
    assert same(a["table"], b_["table"]) and int(np.isfinite(a["table"]).sum()) > 0
    assert all(same(np.asarray(a["peaks"][c][f], dtype=np.float64), np.asarray(b_["peaks"][c][f], dtype=np.float64)) for c in a["columns"] for f in Engine.PEAK_FIELDS)
    assert same(a["table"][4], E.output_table(X[4], TX[4], LAT, LON))
    E.close()


# ------------------------------------------------------------------ 3. dispersion bits
def test_dispersion_ones_null_and_mass_flow(g, engines):
    E, B = engines["big"], 5
    X, TX = _batch(g, "big", B)
    ref = E.output_table_batch(X, LAT, LON, tx=TX)
    D = np.ones((B, E.S, 4))
    one = E.output_table_batch(X, LAT, LON, tx=TX, dispersion=D)
    D[:, :, 1] = 0.9 + 0.05 * np.arange(B)[:, None]      # a mass-flow factor changes nothing
    mf = E.output_table_batch(X, LAT, LON, tx=TX, dispersion=D)
    for r in (one, mf):
        assert same(r["table"], ref["table"])
        for c in Engine.OUTPUT_COLUMNS:
            assert all(same(np.asarray(r["envelope"][c][f], dtype=np.float64), np.asarray(ref["envelope"][c][f], dtype=np.float64)) for f in ref["envelope"][c])
            assert all(same(np.asarray(r["peaks"][c][f], dtype=np.float64), np.asarray(ref["peaks"][c][f], dtype=np.float64)) for f in ref["peaks"][c])


@pytest.mark.parametrize("handle", ["big", "m64"])
def test_dispersion_bits_against_scaled_handles(g, engines, handle):
    """thrust and area factors arbitrary per (vector, phase), wind factors powers of two (and 0), one per vector: the single-vector
    call on a handle built with fl(thrust f0), fl(area f2) and the wind columns times f3"""
    E, nodes, B = engines[handle], oa.HANDLES[handle], 5
    X, TX = _batch(g, handle, B)
    S = len(nodes)
    D = 0.9 + 0.2 * np.random.default_rng(23).random((B, S, 4))
    D[:, :, 3] = np.array([0.0, 0.5, 1.0, 2.0, 4.0])[:, None]
    got = E.output_table_batch(X, LAT, LON, tx=TX, dispersion=D, envelope=False, peaks=False)["table"]
    sub = E.output_table_batch(X, LAT, LON, tx=TX, dispersion=D, columns=SUBSET, envelope=False, peaks=False)["table"]
    plain = E.output_table_batch(X, LAT, LON, tx=TX, envelope=False, peaks=False)["table"]
    for b in range(B):
        params = [(p[0] * D[b, s, 0], p[1] * D[b, s, 2], p[2]) for s, p in enumerate(oa.PARAMS[:S])]
        wind = np.array(g["wind"], dtype=np.float64)
        wind[:, 1:] = wind[:, 1:] * D[b, 0, 3]
        Eb = Engine(oa.prob_arrays(nodes, wind, g["ca"], params))
        ref = Eb.output_table(X[b], TX[b], LAT, LON)
        Eb.close()
        assert same(got[b], ref), b
        assert same(sub[b], ref[:, [Engine.OUTPUT_COLUMNS.index(c) for c in SUBSET]]), b
        assert not same(got[b], plain[b])


# ------------------------------------------------------------------ 4. dispersion values
def test_dispersed_wind_against_the_oracle():
    import test_output_table as tot
    from gelato_amd import con_dynamics
    gg = load_golden("g14_output_table.npz")
    pdict, unitdict, _, _ = tot.example(device=None)
    E = con_dynamics.engine_of(pdict, unitdict)
    x, tx, lc = gg["x_moved"], gg["tx_moved"], pdict["LaunchCondition"]
    O1 = tot.oracle_table(gg, "moved", pdict, unitdict)
    windy = dict(pdict)
    windy["wind_table"] = np.array(pdict["wind_table"], dtype=np.float64)
    windy["wind_table"][:, 1:] *= 1.3
    O13 = tot.oracle_table(gg, "moved", windy, unitdict)
    a, r = TOL["dynamic_pressure"]
    teeth = np.abs(O13["dynamic_pressure"] - O1["dynamic_pressure"]) > 10.0 * (a + r * np.abs(O13["dynamic_pressure"]))
    assert teeth.any()                                                     # oracle against oracle: the factor is visible
    D = np.ones((2, E.S, 4))
    D[1, :, 3] = 1.3
    T = E.output_table_batch(np.stack([x, x]), lc["lat"], lc["lon"], tx=np.stack([tx, tx]), dispersion=D, envelope=False, peaks=False)["table"]
    for k, c in enumerate(Engine.OUTPUT_COLUMNS):
        tot.check_device_column(c, T[1, :, k], ((O13[c], "oracle, wind x 1.3"),))
        tot.check_device_column(c, T[0, :, k], ((O1[c], "oracle"),))
    k = Engine.OUTPUT_COLUMNS.index("dynamic_pressure")
    i = int(np.argmax(teeth))
    assert abs(T[0, i, k] - O13["dynamic_pressure"][i]) > a + r * abs(O13["dynamic_pressure"][i])   # the undispersed table misses it


# ------------------------------------------------------------------ 5. peaks
@pytest.mark.parametrize("B", [1, 3, 65])
def test_peaks(g, engines, full, B):
    R = full(B)
    P = np.stack([np.stack([np.asarray(R["peaks"][c][f], dtype=np.float64) for f in Engine.PEAK_FIELDS], axis=-1) for c in R["columns"]], axis=1)
    want = obt.peaks_reference(R["table"])
    assert same(P, want)
    assert R["peaks"]["M"]["argmax"].dtype == np.int64
    if B > 1:                                              # vector 1 has a NaN node: it is never a peak; the others' peaks are whole
        assert not (P[1, :, 1] == 70).any() and not (P[1, :, 3] == 70).any()
    # a vector whose every node is NaN: no finite entry in any column
    X, TX = _batch(g, "big", 3)
    X[2, :11 * 129] = np.nan
    R2 = engines["big"].output_table_batch(X, LAT, LON, tx=TX, columns=SUBSET, envelope=False)
    P2 = np.stack([np.stack([np.asarray(R2["peaks"][c][f], dtype=np.float64) for f in Engine.PEAK_FIELDS], axis=-1) for c in SUBSET], axis=1)
    assert same(P2, obt.peaks_reference(R2["table"]))
    assert np.isnan(P2[2, :, 0]).all() and (P2[2, :, 1] == -1).all() and (P2[2, :, 3] == -1).all()


# ------------------------------------------------------------------ 6. / 7. envelope
def _env_array(R):
    return np.stack([np.stack([np.asarray(R["envelope"][c][f], dtype=np.float64) for f in obt.ENV_FIELDS], axis=-1) for c in R["columns"]], axis=1)


@pytest.mark.parametrize("B", [1, 2, 3, 64, 65, 256, 257, 600])
def test_envelope_mean_and_m2(g, engines, full, B):
    """exact fields exactly, mean / m2 / std under the derived bound of the exactly rounded values.  Largest shares of the bound
    the device used on the MI355X (printed; DESIGN.md 3.16 records them)."""
    R = full(B)
    env = _env_array(R)
    std = np.stack([R["envelope"][c]["std"] for c in R["columns"]], axis=1)
    share = obt.check_envelope(R["table"], env, std=std)
    print("\nB = %d: largest share of the bound used: mean %.3g, m2 %.3g, std %.3g" % (B, share["mean"], share["m2"], share["std"]))
    assert R["envelope"]["M"]["count"].dtype == np.int64
    if B == 1:
        fin = np.isfinite(R["table"][0])
        assert np.all(env[:, :, 2][fin] == 0.0) and np.all(env[:, :, 0][fin] == 1.0)
    if B > 1:
        k = Engine.OUTPUT_COLUMNS.index("altitude")
        assert env[70, k, 7] == 1.0 and env[70, k, 0] == B - 1


@pytest.mark.parametrize("B", [1, 9, 257])
@pytest.mark.parametrize("handle", ["m64", "m3"])
def test_envelope_mean_and_m2_node_groups(g, engines, handle, B):
    """the same on M = 64 (every node group of outbatch_env_kernel full) and M = 3 (one group, five idle node lanes), B = 1, 9
    (a second step of one vector) and 257 (a second block of one vector), in both forms: with a table (outbatch_env_table_kernel)
    and without one (outbatch_env_kernel) -- each against the exact statistics of the table, and bit for bit each other's"""
    E = engines[handle]
    X, TX = _batch(g, handle, B)
    R = E.output_table_batch(X, LAT, LON, tx=TX)
    assert R["table"].shape == (B, MS[handle], 34) and same(R["table"][:1], single_tables(g, engines, handle, 1))
    alone = E.output_table_batch(X, LAT, LON, tx=TX, table=False, peaks=False)
    for form, r in (("with a table", R), ("without a table", alone)):
        env = _env_array(r)
        std = np.stack([r["envelope"][c]["std"] for c in r["columns"]], axis=1)
        share = obt.check_envelope(R["table"], env, std=std)
        print("\n%s B = %d %s: largest share of the bound used: mean %.3g, m2 %.3g, std %.3g" % (handle, B, form, share["mean"], share["m2"], share["std"]))
        fin = np.isfinite(R["table"]).all(axis=0)
        assert fin.any() and np.all(env[:, :, 0][fin] == float(B))
        if B == 1:
            assert np.all(env[:, :, 2][fin] == 0.0)
    assert same(_env_array(alone), _env_array(R))


EXACT_NODES = (0, 1, 5, 63, 64, 70, 127, 128)      # both ends of a node group and of a tile of 64; node 70 holds vector 1's NaN


def test_envelope_is_the_stated_order_bit_for_bit(g, engines, full):
    """B = 600 on the big handle (three blocks, two merges): count, mean, m2 and the other five fields of eight nodes x all 34
    columns equal output_batch_truth.welford_merge_exact -- the header's order, each written operation one rounding, the fma
    correctly rounded -- on the device's own table, bit for bit.  tests/test_output_batch_cpu.py shows that this restatement differs
    in its bits from the order without the fma and from a contracted merge."""
    B = 600
    R = full(B)
    env = _env_array(R)
    T = R["table"]
    differ, told_apart, contracted = [], 0, 0
    for i in EXACT_NODES:
        for k, c in enumerate(R["columns"]):
            want = obt.welford_merge_exact(T[:, i, k])
            # restatement against restatement on this table: the order without the fma, and a merge whose m2 is contracted
            told_apart += int(not same(obt.welford_merge(T[:, i, k])[2], want[2]))
            contracted += int(not same(obt.welford_merge_exact(T[:, i, k], contract_merge="m2")[2], want[2]))
            if not same(env[i, k], want):
                differ.append((i, c, [f for j, f in enumerate(obt.ENV_FIELDS) if not same(env[i, k, j], want[j])], env[i, k, 1:3].tolist(), want[1:3].tolist()))
    assert not differ, (len(differ), differ[:5])
    k = Engine.OUTPUT_COLUMNS.index("altitude")
    assert env[70, k, 0] == B - 1 and env[70, k, 7] == 1.0
    print("\nB = %d: %d of %d pairs equal the stated order bit for bit; in m2 the order without the fma differs at %d of them, a "
          "contracted merge at %d" % (B, len(EXACT_NODES) * 34 - len(differ), len(EXACT_NODES) * 34, told_apart, contracted))
    # (a contracted MEAN update cannot show on this batch: its block means differ by 1e-7 of their size, so the product's lost bits
    # lie 23 places below the sum's last one; tests/test_output_batch_cpu.py tells that variant apart on spread-out columns)
    assert told_apart >= 1 and contracted >= 1, (told_apart, contracted)


def test_envelope_count_zero_and_ties(g, engines):
    """node 5 NaN in EVERY vector: the count == 0 pattern; two identical vectors: the lower index"""
    E, B, M = engines["big"], 4, 129
    X, TX = _batch(g, "big", B)
    X[3], TX[3] = X[0], TX[0]
    X[2], TX[2] = X[0], TX[0]
    obt.nan_node(X, None, 5, M)
    R = E.output_table_batch(X, LAT, LON, tx=TX)
    env = _env_array(R)
    obt.check_envelope(R["table"], env, std=np.stack([R["envelope"][c]["std"] for c in R["columns"]], axis=1))
    assert np.all(env[5, :, 0] == 0.0) and np.isnan(env[5, :, 1:5]).all() and np.all(env[5, :, 5:7] == -1.0) and np.all(env[5, :, 7] == 0.0)
    ident = E.output_table_batch(np.stack([X[0], X[0]]), LAT, LON, tx=np.stack([TX[0], TX[0]]), table=False, peaks=False)
    e2 = _env_array(ident)
    fin = e2[:, :, 0] == 2.0
    assert fin.any() and np.all(e2[:, :, 5][fin] == 0.0) and np.all(e2[:, :, 6][fin] == 0.0) and np.all(e2[:, :, 2][fin] == 0.0)
    # B = 0: the count == 0 envelope
    Z = E.output_table_batch(np.zeros((0, E.nvars)), LAT, LON)
    assert Z["table"].shape == (0, M, 34) and np.all(Z["envelope"]["M"]["count"] == 0) and np.all(Z["envelope"]["M"]["argmin"] == -1)
    assert np.isnan(Z["envelope"]["M"]["mean"]).all() and np.all(Z["envelope"]["M"]["first_nonfinite"] == -1)


# ------------------------------------------------------------------ 8. reproducibility
def _raw(E, X, TX, cols, out=True, env=True, pk=True, D=None):
    R = E.output_table_batch(X, LAT, LON, tx=TX, dispersion=D, columns=cols, table=out, envelope=env, peaks=pk)
    return (R["table"], _env_array(R) if env else None,
            np.stack([np.stack([np.asarray(R["peaks"][c][f], dtype=np.float64) for f in Engine.PEAK_FIELDS], axis=-1) for c in R["columns"]], axis=1) if pk else None)


@pytest.mark.parametrize("B,cols", [(67, None), (300, SUBSET)])
def test_reproducible_host_device_and_partial_calls(g, engines, B, cols):
    import torch
    E, M = engines["big"], 129
    X, TX = _batch(g, "big", B)
    D = 0.9 + 0.2 * np.random.default_rng(5).random((B, E.S, 4))
    nc = 34 if cols is None else len(cols)
    t0, e0, p0 = _raw(E, X, TX, cols, D=D)
    t1, e1, p1 = _raw(E, X, TX, cols, D=D)                                   # a second call
    assert same(t0, t1) and same(e0, e1) and same(p0, p1)
    _t, e2, p2 = _raw(E, X, TX, cols, out=False, D=D)                        # without the table
    assert _t is None and same(e0, e2) and same(p0, p2)
    _t, e3, _p = _raw(E, X, TX, cols, out=False, pk=False, D=D)              # the envelope alone
    _t, _e, p3 = _raw(E, X, TX, cols, out=False, env=False, D=D)             # the peaks alone
    assert same(e0, e3) and same(p0, p3)
    # the device form
    dX, dT, dD = torch.from_numpy(X).cuda(), torch.from_numpy(TX).cuda(), torch.from_numpy(D).cuda()
    dO = torch.full((B, M, nc), -3.0, dtype=torch.float64, device="cuda")
    dE = torch.full((M, nc, 8), -3.0, dtype=torch.float64, device="cuda")
    dP = torch.full((B, nc, 4), -3.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    E.output_table_batch_device(B, dX.data_ptr(), LAT, LON, d_tx=dT.data_ptr(), d_dispersion=dD.data_ptr(), columns=cols,
                                d_out=dO.data_ptr(), d_env=dE.data_ptr(), d_peaks=dP.data_ptr())
    assert E.sync() == 0                                                     # the table's NaNs never raise the status
    assert same(dO.cpu().numpy(), t0) and same(dE.cpu().numpy(), e0) and same(dP.cpu().numpy(), p0)
    dE.fill_(-3.0)
    torch.cuda.synchronize()
    E.output_table_batch_device(B, dX.data_ptr(), LAT, LON, d_tx=dT.data_ptr(), d_dispersion=dD.data_ptr(), columns=cols, d_env=dE.data_ptr())
    assert E.sync() == 0 and same(dE.cpu().numpy(), e0)


def test_vector_independent_of_batch_and_position(g, engines):
    E, M = engines["big"], 129
    X, TX = _batch(g, "big", 67)
    D = 0.9 + 0.2 * np.random.default_rng(6).random((67, E.S, 4))
    t, _e, p = _raw(E, X, TX, None, env=False, D=D)
    for b in (0, 63, 64, 66):
        t1, _e, p1 = _raw(E, X[b:b + 1], TX[b:b + 1], None, env=False, D=D[b:b + 1])
        assert same(t1[0], t[b]) and same(p1[0], p[b]), b


# ------------------------------------------------------------------ 9. shared memory
def test_arena_shared_with_rows_eval(g):
    x, tx = g["x_big"], g["tx_big"]
    B = 96
    X = np.tile(x, (B, 1)) * (1.0 + 1e-9 * np.arange(B))[:, None]
    X[:, 7 * 129:11 * 129] = x[7 * 129:11 * 129]
    assert X.nbytes > (1 << 20)
    rows = [("orbit_energy", 5, 1.0e6, 0.0), ("radius", 70, 6.4e6, 1.0), ("speed", 128, 1.0e3, 0.0), ("altitude", 30, 1, 0, [1.0e5, 0.0]),
            ("downrange", 90, 2, 0, [1.0e6, 0.0, LAT, LON])]
    got = []
    for with_table in (True, False):
        E = Engine(oa.prob_arrays(oa.NODES, g["wind"], g["ca"]))
        E.rows_configure([], rows)
        a = E.rows_eval(X)
        if with_table:
            T = E.output_table_batch(X, LAT, LON, tx=np.tile(tx, (B, 1)))
            assert same(T["table"][0], E.output_table(X[0], tx, LAT, LON))
        b = E.rows_eval(X)
        res, vals, rc = E.eval(x)
        got.append((a, b, res.copy(), vals.copy(), rc))
        E.close()
    (a1, b1, r1, v1, rc1), (a0, b0, r0, v0, rc0) = got
    for p, q in ((a1, a0), (b1, b0), (a1, b1)):
        assert np.array_equal(p[0], q[0], equal_nan=True) and np.array_equal(p[1], q[1], equal_nan=True) and p[2] == q[2]
    assert np.array_equal(r1, r0, equal_nan=True) and np.array_equal(v1, v0, equal_nan=True) and rc1 == rc0


# ------------------------------------------------------------------ 10. the Python layer
def test_flight_envelope():
    from gelato_amd import con_dynamics, montecarlo, output_result as orr, pack_x, problem, propagate
    pdict, unitdict, _cond, xdict = problem.make_problem("example")
    S, ps = pdict["num_sections"], pdict["ps_params"]
    E = Engine(con_dynamics.problem_arrays(pdict, unitdict), D=[ps.D(i) for i in range(S)], tau=[ps.tau(i) for i in range(S)])
    lc = pdict["LaunchCondition"]
    x = pack_x(xdict)
    X = np.tile(x, (5, 1))
    D = propagate.sample_dispersion(5, S, [0.02, 0.01, 0.03, 0.2], seed=4)
    cols = ["altitude", "dynamic_pressure", "Q_alpha", "M", "vel_air", "lat_IIP"]
    out = montecarlo.flight_envelope(X, pdict, unitdict, dispersion=D, steps=1, columns=cols, engine=E)
    f = propagate.fly(X, pdict, unitdict, steps=1, dispersion=D, engine=E)
    assert out["steps"] == f["steps"] == 2 and out["status"] == f["status"] and "rows" not in out
    assert np.array_equal(_bits(out["x_flown"]), _bits(f["x_flown"])) and np.array_equal(_bits(out["terminal_miss"]), _bits(f["err"][:, -1]))
    R = E.output_table_batch(f["x_flown"], lc["lat"], lc["lon"], dispersion=D, columns=cols)
    assert out["columns"] == cols
    for c in cols:
        for k in ("envelope", "peaks"):
            for fld, v in R[k][c].items():
                assert same(np.asarray(out[k][c][fld], dtype=np.float64), np.asarray(v, dtype=np.float64)), (c, k, fld)
    assert R["envelope"]["dynamic_pressure"]["std"].max() > 0.0
    # all factors one, one vector: the single-vector table at the flown state and its own node times
    one = montecarlo.flight_envelope(xdict, pdict, unitdict, dispersion=np.ones((1, S, 4)), steps=1, engine=E)
    xf = one["x_flown"][0]
    tx = orr.node_times(E.split_x(xf), unitdict, pdict)[0]
    T1 = E.output_table_batch(xf, lc["lat"], lc["lon"], dispersion=np.ones((1, S, 4)), envelope=False, peaks=False)["table"]
    assert same(T1[0], E.output_table(xf, tx, lc["lat"], lc["lon"]))
    for k, c in enumerate(Engine.OUTPUT_COLUMNS):
        assert same(one["envelope"][c]["mean"], T1[0, :, k]) and np.all((one["envelope"][c]["m2"] == 0.0) | np.isnan(T1[0, :, k]))
    E.rows_configure([(E.M - 1, 1.0, -1, 0.0, -0.25)], [("radius", E.M - 1, 6378137.0, 1.0)])
    withrows = montecarlo.flight_envelope(X, pdict, unitdict, dispersion=D, steps=1, columns=cols, engine=E)
    assert np.array_equal(_bits(withrows["rows"]), _bits(E.rows_eval(f["x_flown"], want_jac=False)[0]))
    E.close()

"""gel_output_table on the atlas (tests/output_atlas.py, tests/golden/g26_output_atlas.npz): every branch of output_kernel against
a 50-digit truth under a bound derived from the reference's own fp64 cost, against the reference's recorded table and the oracle
under the example test's tolerances, through the Python layer, on handles of M = 129 / 64 / 3, twice, next to a NaN node, and
between two uses of the scratch buffer it shares with gel_rows_eval.  Every launch is one node per lane."""
import numpy as np
import pytest

import output_atlas as oa
from conftest import load_golden
from gelato_amd import Engine
from gelato_amd.SectionParameters import PSparams
from oracle import output_table as ot
from test_output_table import TOL

pytestmark = pytest.mark.gpu


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
def device_tables(g, engines):
    return {h: engines[h].output_table(g["x_" + h], g["tx_" + h], oa.LAUNCH_LAT, oa.LAUNCH_LON) for h in oa.HANDLES}


@pytest.fixture(scope="module")
def oracle_tables(g):
    return {h: oa.oracle_table(g["x_" + h], g["tx_" + h], nodes, g["wind"], g["ca"]) for h, nodes in oa.HANDLES.items()}


def test_device_vs_truth(g, engines, device_tables):
    """|device - T| <= 4 max(K_col, 1) u s (+ the downrange term) on every entry, equal NaN pattern, nothing masked"""
    assert engines["big"].M == 129 and Engine.OUTPUT_COLUMNS == ot.DEVICE_COLUMNS == [str(c) for c in g["columns"]]
    r = oa.usage(device_tables["big"], g, "big")
    print("\n" + oa.usage_report(r, "device, M = 129"))
    assert int(np.isnan(g["T_big"]).sum()) > 0
    bad = [(i, str(g["tags"][i]), ot.DEVICE_COLUMNS[k], device_tables["big"][i, k], g["T_big"][i, k], r[i, k]) for i, k in zip(*np.nonzero(r > 1.0))]
    assert not bad, bad


@pytest.mark.parametrize("handle", ["m64", "m3"])
def test_small_handles_vs_truth_and_oracle(g, engines, device_tables, oracle_tables, handle):
    """one full workgroup exactly (M = 64) and three lanes (M = 3): the truth of these nodes is in the fixture; the oracle's values
    +- the same bound as well"""
    D, O, b = device_tables[handle], oracle_tables[handle], oa.bound(g, handle)
    assert engines[handle].M == oa.HANDLES[handle][0] + 1 == D.shape[0]
    r = oa.usage(D, g, handle)
    assert r.max() <= 1.0, [(i, ot.DEVICE_COLUMNS[k], r[i, k]) for i, k in zip(*np.nonzero(r > 1.0))]
    assert np.array_equal(np.isnan(D), np.isnan(O))
    ok = (np.abs(D - O) <= b) | np.isnan(O)
    assert ok.all(), [(i, ot.DEVICE_COLUMNS[k], D[i, k], O[i, k]) for i, k in zip(*np.nonzero(~ok))]


@pytest.mark.parametrize("handle", list(oa.HANDLES))
def test_device_vs_reference_recorded_table_and_oracle(g, device_tables, oracle_tables, handle):
    """the example test's per-column tolerances, unchanged, on the atlas"""
    D, O = device_tables[handle], oracle_tables[handle]
    for k, c in enumerate(ot.DEVICE_COLUMNS):
        ref = g["ref_%s_%s" % (handle, c)]
        assert np.array_equal(np.isnan(D[:, k]), np.isnan(ref)), c
        a, rel = TOL[c]
        for other, name in ((ref, "reference"), (O[:, k], "oracle")):
            d = np.abs(D[:, k] - other)
            ok = (d <= a + rel * np.abs(other)) | np.isnan(other)
            assert ok.all(), (c, name, int(np.nanargmax(np.where(ok, 0.0, d))), np.nanmax(np.where(ok, 0.0, d)))


def test_gimbal_lock_state_outside_the_atlas(g, engines):
    """identity quaternion over latitude 0, longitude 0 (output_atlas.edge): every operation up to the predicate is exact but one
    division, so the kernel sees the reference's 2 (w y - z x) = 1 - 2^-52 and, like it, returns pitch asin(.) and heading = roll = 0"""
    D = engines["m3"].output_table(g["x_edge"], g["tx_edge"], oa.LAUNCH_LAT, oa.LAUNCH_LON)
    O = oa.oracle_table(g["x_edge"], g["tx_edge"], oa.SMALL["m3"], g["wind"], g["ca"])
    for c in ("heading_NED2BODY", "roll_NED2BODY"):
        assert np.all(D[:, ot.DEVICE_COLUMNS.index(c)] == 0.0), c
    for k, c in enumerate(ot.DEVICE_COLUMNS):
        ref = g["ref_edge_" + c]
        assert np.array_equal(np.isnan(D[:, k]), np.isnan(ref)), c
        a, rel = TOL[c]
        for other, name in ((ref, "reference"), (O[:, k], "oracle")):
            assert np.all((np.abs(D[:, k] - other) <= a + rel * np.abs(other)) | np.isnan(other)), (c, name, D[:, k], other)


def test_python_layer(g, device_tables):
    """gelato_amd.output_result.output_result on the atlas: text and host-formed columns bit for bit the reference's, the device
    columns the handle's own, the input dict untouched"""
    from gelato_amd import output_result as orr
    pdict = oa.pdict_of(oa.NODES, g["wind"], g["ca"], PSparams(oa.NODES))
    xd = oa.xdict_of(g["x_big"], 129, 125, 4)
    keep = {k: v.copy() for k, v in xd.items()}
    df = orr.output_result(xd, dict(oa.UNITS), g["tx_big"].copy(), g["tu_big"].copy(), pdict)
    assert list(df.columns) == [str(c) for c in g["ref_columns"]] and len(df) == 129
    for c in df.columns:
        ref, got = g["ref_big_" + c], df[c].to_numpy()
        if ref.dtype.kind == "U":
            assert [str(v) for v in got] == [str(v) for v in ref], c
        elif c in Engine.OUTPUT_COLUMNS:
            assert np.array_equal(got, device_tables["big"][:, Engine.OUTPUT_COLUMNS.index(c)], equal_nan=True), c
        else:
            assert np.array_equal(got, ref), c
    assert all(np.array_equal(xd[k], keep[k]) for k in xd)


def test_repeat_and_isolation(g, engines, device_tables):
    E, x, tx = engines["big"], g["x_big"], g["tx_big"]
    again = E.output_table(x, tx, oa.LAUNCH_LAT, oa.LAUNCH_LON)
    assert np.array_equal(again, device_tables["big"], equal_nan=True)
    # one node's state NaN: its row is non-finite, every other row keeps its bits
    i, M = 70, 129
    xn = x.copy()
    xn[i] = xn[M + 3 * i:M + 3 * i + 3] = xn[4 * M + 3 * i:4 * M + 3 * i + 3] = xn[7 * M + 4 * i:7 * M + 4 * i + 4] = np.nan
    D = E.output_table(xn, tx, oa.LAUNCH_LAT, oa.LAUNCH_LON)
    assert not np.isfinite(D[i]).any()
    others = np.arange(M) != i
    assert np.array_equal(D[others], device_tables["big"][others], equal_nan=True)


def test_shared_scratch_with_rows_eval(g, device_tables):
    """gel_output_table stages through the device buffer large gel_rows_eval calls use: rows_eval, output_table, rows_eval, eval on
    one handle give the bits of a handle that never called output_table"""
    x, tx = g["x_big"], g["tx_big"]
    B = 96                                                  # 96 vectors of 1674 doubles: above the pinned-memory path's 1 MiB
    X = np.tile(x, (B, 1)) * (1.0 + 1e-9 * np.arange(B))[:, None]
    X[:, 7 * 129:11 * 129] = x[7 * 129:11 * 129]
    assert X.nbytes > (1 << 20)
    rows = [("orbit_energy", 5, 1.0e6, 0.0), ("radius", 70, 6.4e6, 1.0), ("speed", 128, 1.0e3, 0.0), ("altitude", 30, 1, 0, [1.0e5, 0.0]),
            ("downrange", 90, 2, 0, [1.0e6, 0.0, oa.LAUNCH_LAT, oa.LAUNCH_LON])]
    got = []
    for with_table in (True, False):
        E = Engine(oa.prob_arrays(oa.NODES, g["wind"], g["ca"]))
        E.rows_configure([], rows)
        a = E.rows_eval(X)
        if with_table:
            T = E.output_table(x, tx, oa.LAUNCH_LAT, oa.LAUNCH_LON)
            assert np.array_equal(T, device_tables["big"], equal_nan=True)
        b = E.rows_eval(X)
        res, vals, rc = E.eval(x)
        got.append((a, b, res.copy(), vals.copy(), rc))
        E.close()
    (a1, b1, r1, v1, rc1), (a0, b0, r0, v0, rc0) = got
    for p, q in ((a1, a0), (b1, b0), (a1, b1)):
        assert np.array_equal(p[0], q[0], equal_nan=True) and np.array_equal(p[1], q[1], equal_nan=True) and p[2] == q[2]
    assert np.array_equal(r1, r0, equal_nan=True) and np.array_equal(v1, v0, equal_nan=True) and rc1 == rc0

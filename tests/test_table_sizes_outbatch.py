"""gel_output_table_batch over the wind and CA tables of tests/table_cases.py: outbatch_rows_kernel and
outbatch_env_kernel put their 64 x 34 row tile and the column map at (table_doubles + 1) & ~1 doubles, behind the staged tables --
the parity LONG (1029 staged doubles) and LONGEVEN (1032) exist for -- and stage the tables through one wavefront (seventeen
passes).  tests/test_output_batch.py runs them on the atlas handles' one table size only.

Over test_table_sizes.PARAMS: M = 56 / 110 / 80 state nodes (7 / 13.75 / 10 node groups of outbatch_env_kernel; two tiles of
outbatch_rows_kernel on the coop and slab meshes).  The batch interleaves output_batch_truth.batch_of of `climb` and of `knots`: the
1 + 1e-9 b scaling raises a node by 6.4 mm per b, so the `knots` nodes 4 mm and 4 cm below a knot cross it inside one batch and
the lanes of one wavefront of outbatch_env_kernel (8 vectors x 8 nodes) look up different intervals -- asserted from the exact
lookup's piece at the oracle's altitudes.

The table is held to Engine.output_table bit for bit (which test_table_sizes.test_output_table holds to the oracle on the same
states); the envelope and peaks to output_batch_truth on the device's own table; no tolerance of its own."""
import numpy as np
import pytest

import output_batch_truth as obt
import states
import table_cases as TC
from gelato_amd import Engine
from test_output_batch import SUBSET, _env_array, same
from test_table_sizes import PARAMS, _state, behind_the_wind_extra

LAT, LON = 28.5, 0.0
_ENGINE, _SINGLE = {}, {}


def _engine(case, mesh):
    if (case, mesh) not in _ENGINE:
        _ENGINE[(case, mesh)] = Engine(_state(case, mesh, "climb")[0])
    return _ENGINE[(case, mesh)]


def batch(case, mesh, B):
    """(X [B, nvars], TX [B, M]): vector b is the 1 + 1e-9 b copy of `climb` (b even) or of `knots` (b odd); the node times of
    every vector from its own knot times"""
    prob, xc = _state(case, mesh, "climb")
    _p, xk = _state(case, mesh, "knots")
    M = sum(TC.MESHES[mesh]) + len(TC.MESHES[mesh])
    Xc, Xk = obt.batch_of(xc, M, B), obt.batch_of(xk, M, B)
    X = np.ascontiguousarray(np.where((np.arange(B) % 2 == 0)[:, None], Xc, Xk))
    times = {}                                                  # (batch_of leaves the knot times: two distinct sets per batch)
    S = len(TC.MESHES[mesh])
    TX = np.empty((B, M))
    for b in range(B):
        key = X[b, -(S + 1):].tobytes()
        if key not in times:
            times[key] = states.table_node_times(prob, X[b])
        TX[b] = times[key]
    assert len(times) <= 2
    return X, TX


def single_tables(case, mesh, B):
    """Engine.output_table of every vector of batch(case, mesh, B): once per (case, mesh, vector)"""
    X, TX = batch(case, mesh, B)
    have = _SINGLE.setdefault((case, mesh), [])
    for b in range(len(have), B):
        have.append(_engine(case, mesh).output_table(X[b], TX[b], LAT, LON))
    return np.stack(have[:B])


@pytest.mark.parametrize("case,mesh", PARAMS)
def test_knots_nodes_cross_their_knots_inside_one_batch(case, mesh):
    """(no device: the batch alone) every knot of table_knots has a `knots` node whose wind lookup changes its piece among the odd
    vectors 1 .. 15 of the batch: lanes of one wavefront on either side of a knot"""
    import oracle
    prob = _state(case, mesh, "climb")[0]
    wind = TC.CASES[case][0]
    X, _TX = batch(case, mesh, 16)
    pieces = []
    for b in range(1, 16, 2):
        alt = states.table_oracle_rows(prob, X[b])["altitude"]
        pieces.append([TC.lookup_truth(oracle.geopotential_altitude(z), wind[:, 0], wind[:, 1])[1] for z in alt])
    pieces = np.array(pieces)
    changing = np.nonzero((pieces != pieces[0]).any(axis=0))[0]
    crossed = {tuple(sorted(set(pieces[:, i]))) for i in changing}
    assert len(crossed) >= len(states.table_knots(case)), (case, mesh, crossed)
    assert all(len(c) == 2 for c in crossed)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("case,mesh", PARAMS)
def test_table_bits_against_the_single_vector_call(case, mesh, B):
    """outbatch_rows_kernel: all columns, a scrambled subset and one column behind the wind lookup"""
    E = _engine(case, mesh)
    X, TX = batch(case, mesh, B)
    ref = single_tables(case, mesh, B)
    assert np.isfinite(ref).any() and ref.shape == (B, E.M, 34)
    T = E.output_table_batch(X, LAT, LON, tx=TX, envelope=False, peaks=False)
    assert T["columns"] == Engine.OUTPUT_COLUMNS and same(T["table"], ref)
    for cols in (SUBSET, ["vel_air"]):
        S = E.output_table_batch(X, LAT, LON, tx=TX, columns=cols, envelope=False, peaks=False)
        assert S["columns"] == cols
        assert same(S["table"], ref[:, :, [Engine.OUTPUT_COLUMNS.index(c) for c in cols]]), (case, mesh, B, cols)


@pytest.mark.gpu
@pytest.mark.parametrize("case,mesh", PARAMS)
def test_envelope_and_peaks_two_blocks(case, mesh):
    """B = 259: two envelope blocks, the last step of the last holds 3 of 8 vectors.  The envelope of a call without a table
    (outbatch_env_kernel: the rows formed in its tile behind the tables) equals the one of a call with a table
    (outbatch_env_table_kernel) bit for bit; check_envelope and peaks_reference on the device's own table."""
    E, B = _engine(case, mesh), 259
    X, TX = batch(case, mesh, B)
    R = E.output_table_batch(X, LAT, LON, tx=TX)
    env = _env_array(R)
    alone = E.output_table_batch(X, LAT, LON, tx=TX, table=False, peaks=False)
    assert alone["table"] is None and same(_env_array(alone), env), (case, mesh)
    few = E.output_table_batch(X, LAT, LON, tx=TX, columns=SUBSET, table=False, peaks=False)
    assert same(_env_array(few), env[:, [Engine.OUTPUT_COLUMNS.index(c) for c in SUBSET]]), (case, mesh)
    assert same(R["table"][:65], single_tables(case, mesh, 65))
    std = np.stack([R["envelope"][c]["std"] for c in R["columns"]], axis=1)
    share = obt.check_envelope(R["table"], env, std=std)
    print("\n%s/%s B = %d: largest share of the bound used: mean %.3g, m2 %.3g, std %.3g" % (case, mesh, B, share["mean"], share["m2"], share["std"]))
    P = np.stack([np.stack([np.asarray(R["peaks"][c][f], dtype=np.float64) for f in Engine.PEAK_FIELDS], axis=-1) for c in R["columns"]], axis=1)
    assert same(P, obt.peaks_reference(R["table"]))
    pk = E.output_table_batch(X, LAT, LON, tx=TX, table=False, envelope=False)
    P2 = np.stack([np.stack([np.asarray(pk["peaks"][c][f], dtype=np.float64) for f in Engine.PEAK_FIELDS], axis=-1) for c in pk["columns"]], axis=1)
    assert same(P2, P)


def _scaled(prob, f, wind_only=False):
    """prob with thrust f[s, 0], reference area f[s, 2] per phase and the wind columns f[0, 3]: the products the device forms"""
    p = dict(prob)
    if not wind_only:
        p["thrust"] = np.asarray(prob["thrust"], dtype=np.float64) * f[:, 0]
        p["reference_area"] = np.asarray(prob["reference_area"], dtype=np.float64) * f[:, 2]
    w = np.array(prob["wind_table"], dtype=np.float64)
    w[:, 1:3] = w[:, 1:3] * f[0, 3]
    p["wind_table"] = w
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["LONG", "LONGEVEN"])
def test_dispersed_wind_bits_and_values(case):
    """outbatch_rows_kernel<true> on the coop mesh.  Bits: B = 5, wind factors 0, 0.5, 1, 2, 4 (one per vector) under arbitrary
    thrust and area factors per (vector, phase), against handles built with the scaled parameters and the scaled wind table, as
    test_output_batch.test_dispersion_bits_against_scaled_handles does.  Values: a wind factor of 1.3 against the oracle's table of
    the wind-scaled problem under TOL and test_table_sizes.test_output_table's extra term."""
    from test_output_table import check_device_column
    mesh = "coop"
    E, B = _engine(case, mesh), 5
    prob = _state(case, mesh, "climb")[0]
    X, TX = batch(case, mesh, B)
    D = 0.9 + 0.2 * np.random.default_rng(23).random((B, E.S, 4))
    D[:, :, 3] = np.array([0.0, 0.5, 1.0, 2.0, 4.0])[:, None]
    got = E.output_table_batch(X, LAT, LON, tx=TX, dispersion=D, envelope=False, peaks=False)["table"]
    sub = E.output_table_batch(X, LAT, LON, tx=TX, dispersion=D, columns=SUBSET, envelope=False, peaks=False)["table"]
    plain = E.output_table_batch(X, LAT, LON, tx=TX, envelope=False, peaks=False)["table"]
    for b in range(B):
        Eb = Engine(_scaled(prob, D[b]))
        ref = Eb.output_table(X[b], TX[b], LAT, LON)
        Eb.close()
        assert same(got[b], ref), (case, b)
        assert same(sub[b], ref[:, [Engine.OUTPUT_COLUMNS.index(c) for c in SUBSET]]), (case, b)
        assert not same(got[b], plain[b])
    # values: `climb` and `knots` themselves, the two states test_table_sizes.test_output_table holds to the oracle at a factor of
    # one, so that the wind factor is all that differs.  (Their 1 + 1e-9 b copies are no inputs for a comparison with the oracle:
    # these states are no orbits, and the oracle's OWN altitude_apogee moves by up to 3.7 times its allowance when positions and
    # velocities of the copies b = 1 .. 4 move by one ulp -- measured on the CPU, oracle against oracle.  The copies are held to
    # the single-vector call by bits above.)
    X13 = np.stack([_state(case, mesh, "climb")[1], _state(case, mesh, "knots")[1]])
    TX13 = np.stack([states.table_node_times(prob, x) for x in X13])
    D13 = np.ones((2, E.S, 4))
    D13[:, :, 3] = 1.3
    T = E.output_table_batch(X13, LAT, LON, tx=TX13, dispersion=D13, envelope=False, peaks=False)["table"]
    windy = _scaled(prob, D13[0], wind_only=True)
    for b in range(2):
        Tt = states.table_oracle_rows(windy, X13[b])
        extra = behind_the_wind_extra(windy, X13[b], Tt)
        for j, c in enumerate(Engine.OUTPUT_COLUMNS):
            check_device_column(c, T[b, :, j], ((Tt[c], "oracle, wind x 1.3"),), extra=extra[c])
        # the factor is visible, oracle against oracle: the unscaled wind is metres per second away in vel_air
        T1 = states.table_oracle_rows(prob, X13[b])
        assert np.nanmax(np.abs(T1["vel_air"] - Tt["vel_air"])) > 1.0

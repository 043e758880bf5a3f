"""The output table's atlas on the CPU (tests/output_atlas.py, tests/golden/g26_output_atlas.npz): every tag and every branch of
the 50-digit truth's control flow is present and decided, the numpy oracle agrees with the reference's recorded table on every new
branch and costs K_col against the truth, and the bound the GPU test asserts rejects five wrong oracles."""
import math

import numpy as np
import pytest

import output_atlas as oa
from conftest import load_golden
from oracle import output_table as ot


@pytest.fixture(scope="module")
def g():
    return load_golden(oa.FIXTURE)


@pytest.fixture(scope="module")
def oracle_tables(g):
    return {h: oa.oracle_table(g["x_" + h], g["tx_" + h], nodes, g["wind"], g["ca"]) for h, nodes in oa.HANDLES.items()}


def test_atlas_is_the_fixture(g):
    """the module still builds the vector the fixture was written from, bit for bit, and every tag's property holds"""
    A = oa.build()
    oa.validate(A)                        # (also tags the nodes above the wind table's last knot)
    assert np.array_equal(A["x"], g["x_big"]) and np.array_equal(A["tx"], g["tx_big"]) and np.array_equal(A["tu"], g["tu_big"])
    assert np.array_equal(A["wind"], g["wind"]) and np.array_equal(A["ca"], g["ca"])
    assert ["|".join(t) for t, _, _ in A["nodes"]] == [str(t) for t in g["tags"]]
    for h in oa.SMALL:
        x, tx, tu, _ = oa.small(h)
        assert np.array_equal(x, g["x_" + h]) and np.array_equal(tx, g["tx_" + h]) and np.array_equal(tu, g["tu_" + h])
    assert len(g["x_big"]) == 11 * 129 + 2 * 125 + 5 and len(g["tx_m64"]) == 64 and len(g["tx_m3"]) == 3
    assert g["wind"].shape == (40, 3) and g["ca"].shape == (30, 2)
    assert len({tuple(p) for p in oa.PARAMS}) == 4 and any(p[1] == 0.0 for p in oa.PARAMS) and any(p[2] == 0.0 for p in oa.PARAMS)


def test_every_tag_and_every_branch(g):
    have = {t for tags in g["tags"] for t in str(tags).split("|")}
    missing = [t for t in oa.REQUIRED_TAGS if t not in have]
    assert not missing, missing
    assert g["tx_big"].min() < 0.0 and 0.0 in g["tx_big"] and g["tx_big"].max() > 86164.1
    # every outcome of every predicate of the truth's control flow, counted while the truth was formed
    taken = {str(n): int(c) for n, c in zip(g["coverage_names"], g["coverage_counts"])}
    both = ["z86", "samelon", "inc", "fz", "rv", "asc_neg", "argp_neg", "vn", "vbx", "az", "iip_r0", "iip_ecos", "iip_hp",
            "iip_int", "lapse"]
    need = ["%s=%s" % (p, o) for p in both for o in (True, False)]
    need += ["ta_neg=False", "calpha=False", "gimbal=False", "iip_e1=True", "iip_conv=False"]
    need += ["layer=%d" % k for k in range(11)] + ["Tbranch=%d" % k for k in range(4)]
    need += ["wind_n=-1", "wind_n=40", "wind_e=-1", "wind_e=40", "ca=-1", "ca=30"]
    missing = [n for n in need if taken.get(n, 0) < 1]
    assert not missing, missing
    assert any(n.startswith("wind_n=") and 0 <= int(n[7:]) < 39 for n in taken) and any(n.startswith("ca=") and 0 <= int(n[3:]) < 29 for n in taken)
    # the outcomes nobody takes are exactly the ones the generator declares unreachable, each with its reason
    unreachable = {str(u).split(":")[0] for u in g["unreachable"]}
    assert unreachable == {"ta_neg=True", "gimbal=True", "iip_conv=True", "iip_e1=False", "calpha=True"}
    assert not [u for u in unreachable if taken.get(u, 0)]


def test_every_predicate_is_decided(g):
    """exact by construction (argument on the threshold, the node lists the predicate) or a margin of 1e6 roundings"""
    names = [str(n) for n in g["pred_names"]]
    m = g["margin_big"]
    assert m.shape == (129, len(names))
    for i in range(129):
        exact = set(str(g["exact"][i]).split("|"))
        for k, n in enumerate(names):
            if np.isnan(m[i, k]) or n == "calpha":          # not evaluated; continuous across its threshold
                continue
            assert m[i, k] >= 1e6 or (m[i, k] == 0.0 and n in exact), (i, str(g["tags"][i]), n, m[i, k])


@pytest.mark.parametrize("handle", list(oa.HANDLES))
def test_oracle_vs_reference_recorded_table(g, oracle_tables, handle):
    """the rule of test_oracle_table_vs_reference_golden, on every new branch"""
    O = oracle_tables[handle]
    n_nan = 0
    for k, c in enumerate(ot.DEVICE_COLUMNS):
        ref = g["ref_%s_%s" % (handle, c)]
        assert np.array_equal(np.isnan(ref), np.isnan(O[:, k])), c
        n_nan += int(np.isnan(ref).sum())
        ok = np.abs(O[:, k] - ref) <= 1e-13 * np.maximum(1.0, np.abs(ref))
        assert np.all(ok | np.isnan(ref)), (c, int(np.nanargmax(np.abs(O[:, k] - ref))), np.nanmax(np.abs(O[:, k] - ref)))
    assert n_nan > 0


def k_col(O, g, handle):
    T, S = g["T_" + handle], g["s_" + handle]
    d = np.abs(O - T)
    dr = ot.DEVICE_COLUMNS.index("downrange")
    d[:, dr] = np.maximum(d[:, dr] - float(g["downrange_term"]), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0.0, 0.0, d / (oa.U64 * S))
    return np.max(np.where(np.isnan(T), 0.0, r), axis=0)


def test_oracle_vs_truth_costs_k_col(g, oracle_tables):
    """K_col = max over nodes |oracle - T| / (u s): what the reference's own fp64 algorithm costs on this libm.  Asserted against
    the value stored when the fixture was written: the same libm gives the same bits; another one may move every libm call of a
    column's path by an ulp, i.e. the column by a few u s (at most 8 calls) or, for downrange whose K is the stopping rule's
    truncation (the reference forms the distance from the lambda BEFORE its last update, an error up to Rb 1e-12 = 6.4e-6 m that
    the issue's term Rb 1e-12 2f / (1 - 2f) does not carry), not at all."""
    K = np.zeros(34)
    for h in oa.HANDLES:
        assert np.array_equal(np.isnan(oracle_tables[h]), np.isnan(g["T_" + h])), h
        K = np.maximum(K, k_col(oracle_tables[h], g, h))
    print("\nK_col (now / stored)")
    for c, a, b in zip(ot.DEVICE_COLUMNS, K, g["K_col"]):
        print("  %-38s %9.3g %9.3g" % (c, a, b))
    assert np.all(np.isfinite(K))
    assert np.all(K <= g["K_col"] + 8.0), [(c, a, b) for c, a, b in zip(ot.DEVICE_COLUMNS, K, g["K_col"]) if a > b + 8.0]
    # and the oracle itself is inside the bound the device is held to (a quarter of it on the libm the fixture was written with)
    for h in oa.HANDLES:
        assert oa.usage(oracle_tables[h], g, h).max() <= 1.0


# ---- the bound has teeth: five wrong oracles, each rejected on at least one entry
def _mutant_elements(kind):
    orig = ot.orbital_elements

    def f(r, v):
        el = orig(r, v)
        c = np.cross(r, v)
        fv = np.cross(v, c) - ot.MU * r / np.linalg.norm(r)
        inclined = math.acos(c[2] / np.linalg.norm(c)) > 1e-10
        if kind == "no_ta_flip" and float(np.dot(r, v)) < 0.0:
            el[5] = 360.0 - el[5]                                   # ta stays acos(.)
        if kind == "no_argp_sign" and inclined and fv[2] < 0:
            el[4] = 360.0 - el[4]                                   # argp stays +acos(.)
        if kind == "equatorial_always" and inclined:
            el[3] = 0.0
            el[4] = math.degrees(math.atan2(fv[1], fv[0]) % (2.0 * math.pi))
        return el
    return f


class _NumpyExtrapolating:
    """numpy, but interp extrapolates past the last knot"""

    def __getattr__(self, k):
        return getattr(np, k)

    @staticmethod
    def interp(x, xp, fp):
        if x > xp[-1]:
            return fp[-1] + (fp[-1] - fp[-2]) / (xp[-1] - xp[-2]) * (x - xp[-1])
        return np.interp(x, xp, fp)


@pytest.mark.parametrize("kind", ["no_ta_flip", "no_argp_sign", "equatorial_always", "knot_section_before", "ca_extrapolates"])
def test_bound_rejects_mutant(g, oracle_tables, monkeypatch, kind):
    assert oa.usage(oracle_tables["big"], g, "big").max() <= 1.0       # the unmutated oracle passes what the mutants fail
    if kind == "knot_section_before":
        orig = ot.node_sections

        def sections(nodes):
            s = orig(nodes)
            first = np.cumsum([n + 1 for n in nodes])[:-1]
            s[first] -= 1
            return s
        monkeypatch.setattr(ot, "node_sections", sections)
    elif kind == "ca_extrapolates":
        monkeypatch.setattr(ot, "np", _NumpyExtrapolating())
    else:
        monkeypatch.setattr(ot, "orbital_elements", _mutant_elements(kind))
    O = oa.oracle_table(g["x_big"], g["tx_big"], oa.NODES, g["wind"], g["ca"])
    r = oa.usage(O, g, "big")
    assert r.max() > 1.0, kind
    rows, cols = np.nonzero(r > 1.0)
    expect = {"no_ta_flip": {"true_anomaly"}, "no_argp_sign": {"argument_perigee"},
              "equatorial_always": {"argument_perigee", "lon_ascending_node"}, "knot_section_before": {"thrust", "accel_BODY_X", "aero_BODY_X"},
              "ca_extrapolates": {"aero_BODY_X", "accel_BODY_X"}}[kind]
    assert {ot.DEVICE_COLUMNS[k] for k in cols} <= expect and len(rows) > 0, (kind, {ot.DEVICE_COLUMNS[k] for k in cols})


def test_gimbal_lock_state_outside_the_atlas(g):
    """identity quaternion over latitude 0, longitude 0: 90 degrees of pitch in exact arithmetic, 2 (w y - z x) = 1 - 2^-52 in fp64
    (tests/output_atlas.py): the reference does not take the gimbal branch there, and the oracle follows it on every column"""
    x, tx, tu = oa.edge()
    assert np.array_equal(x, g["x_edge"]) and np.array_equal(tx, g["tx_edge"]) and np.array_equal(tu, g["tu_edge"])
    pitch = g["ref_edge_pitch_NED2BODY"]
    assert np.all(pitch == np.degrees(np.arcsin(1.0 - 2.0 ** -52))) and np.all(pitch < 90.0)
    assert np.all(g["ref_edge_heading_NED2BODY"] == 0.0) and np.all(g["ref_edge_roll_NED2BODY"] == 0.0)
    O = oa.oracle_table(x, tx, oa.SMALL["m3"], g["wind"], g["ca"])
    for k, c in enumerate(ot.DEVICE_COLUMNS):
        ref = g["ref_edge_" + c]
        assert np.array_equal(np.isnan(ref), np.isnan(O[:, k])), c
        assert np.all((np.abs(O[:, k] - ref) <= 1e-13 * np.maximum(1.0, np.abs(ref))) | np.isnan(ref)), c

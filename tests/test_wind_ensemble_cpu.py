"""The wind ensemble, host side (no GPU; host-only handles): the staged members against a numpy restatement of
append_rows_and_slopes, every refusal with its message, the Python argument checks, propagate.assign_members, the availability
reduction on hand-made peaks, and the ensemble's host code under AddressSanitizer + UBSan in a stand-alone program.

(The library exposes no handle's staged tables, so "the wind part of a handle created with that member" is held here through the
restatement of the one staging function both go through; the GPU suite holds the flights to such handles bit for bit.)"""
import ctypes as C

import numpy as np
import pytest

import interp_truth as it
import sanitized_lib
import table_cases as TC


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def members(K, seeds, calm_of=None):
    """[E, K, 3]: table_cases._wind_table(K, seed) per seed (K = 2: MIN's table and shifted copies of it); calm_of: append a member
    with the altitudes of that member and both wind columns exactly zero"""
    if K == 2:
        base = TC.CASES["MIN"][0]
        t = [base * np.array([1.0, 1.0 + 0.25 * s, 1.0 - 0.5 * s]) + np.array([100.0 * s, 0.0, 0.0]) for s in range(len(seeds))]
    else:
        t = [TC._wind_table(K, s) for s in seeds]
    if calm_of is not None:
        c = t[calm_of].copy()
        c[:, 1:] = 0.0
        t.append(c)
    return np.ascontiguousarray(np.stack(t))


_E = {}


def engine():
    if "e" not in _E:
        _E["e"] = it.engine(it.prob_of([2, 3, 16, 4]))
    return _E["e"]


@pytest.mark.parametrize("K", [2, 32, 33, 160, 400])
def test_member_is_rows_and_slopes_bit_for_bit(K):
    """gel_wind_ensemble_member: the member's rows, then (y1 - y0) / (x1 - x0) per interval and component, 5 Kw - 2 doubles; K = 400
    is longer than any handle accepts (its limit is on LDS, which an ensemble does not use)"""
    E = engine()
    T = members(K, (11, 12, 13, 14), calm_of=1)
    ens = E.wind_ensemble(T)
    info = ens.info()
    assert info == {"E": 5, "Kw": K, "member_doubles": 5 * K - 2, "device_bytes": 0, "assigned": -1}
    for e in range(5):
        m = ens.member(e)
        assert np.array_equal(_bits(m["rows"]), _bits(T[e]))
        slopes = (T[e, 1:, 1:] - T[e, :-1, 1:]) / (T[e, 1:, :1] - T[e, :-1, :1])
        assert m["slopes"].shape == (K - 1, 2) and np.array_equal(_bits(m["slopes"]), _bits(slopes)), (K, e)
    assert np.all(ens.member(4)["slopes"] == 0.0) and np.all(ens.member(4)["rows"][:, 1:] == 0.0)   # the calm member
    ens.close()
    if K == 400:
        from gelato_amd import _lib
        with pytest.raises(_lib.GelatoAmdError, match="doubles of LDS"):
            it.engine(dict(it.prob_of([2, 3]), wind_table=T[0]))


def _create(E, nE, Kw, tables):
    from gelato_amd import _lib
    h = C.c_void_p()
    p = None if tables is None else np.ascontiguousarray(tables).ctypes.data_as(C.POINTER(C.c_double))
    rc = _lib.lib().gel_wind_ensemble_create(E._h, nE, Kw, p, C.byref(h))
    return rc, (_lib.lib().gel_last_error() or b"").decode(), h


def test_create_refusals():
    E = engine()
    T = members(33, (1, 2, 3, 4, 5))
    for nE, Kw, tab, text in ((0, 33, T, "E = 0 < 1"), (-1, 33, T, "E = -1 < 1"), (5, 1, T, "Kw = 1 < 2"), (5, 33, None, "tables is NULL"),
                              # the size bounds, sizes only: at the limit the null table is what is refused, one past it the size
                              (1 << 20, 26, None, "tables is NULL"), ((1 << 20) + 1, 26, None, "exceed 2^27"),
                              (1, 1 << 20, None, "tables is NULL"), (1, (1 << 20) + 1, None, "exceeds 2^20 rows"),
                              (26, 1 << 20, None, "exceed 2^27")):
        rc, msg, h = _create(E, nE, Kw, tab)
        assert rc == -1 and text in msg and not h.value, (nE, Kw, msg)
    bad = T.copy()
    bad[3, 17, 0] = bad[3, 16, 0]                                     # member 3 of 5: an altitude that does not increase
    rc, msg, h = _create(E, 5, 33, bad)
    assert rc == -1 and "member 3" in msg and "increase strictly" in msg and not h.value
    bad[3, 17, 0] = np.nan                                            # a NaN altitude
    rc, msg, h = _create(E, 5, 33, bad)
    assert rc == -1 and "member 3" in msg and "increase strictly" in msg
    bad = T.copy()
    bad[0, 0, 0], bad[4, 32, 0] = T[0, 1, 0] + 1.0, np.nan            # members 0 and 4: the FIRST offender is named
    rc, msg, h = _create(E, 5, 33, bad)
    assert rc == -1 and "member 0" in msg
    ok = T.copy()
    ok[2, 5, 1] = np.nan                                              # a NaN wind entry is data
    rc, msg, h = _create(E, 5, 33, ok)
    assert rc == 0 and h.value
    from gelato_amd import _lib
    assert _lib.lib().gel_wind_ensemble_destroy(h) == 0


def test_assign_and_evaluation_refusals():
    from gelato_amd import _lib
    E, other = engine(), it.engine(it.prob_of([2, 3, 16, 4]))
    L = _lib.lib()
    ens = E.wind_ensemble(members(32, (1, 2, 3)))
    ip = C.POINTER(C.c_int32)

    def assign(m):
        m = np.asarray(m, dtype=np.int32)
        return L.gel_wind_ensemble_assign(ens._p, m.size, m.ctypes.data_as(ip)), L.gel_last_error().decode()
    assert assign([0, -1, 2, 1])[0] == 0 and ens.info()["assigned"] == 4
    rc, msg = assign([0, 1, 3, 1])
    assert rc == -1 and "member[2] = 3 outside -1 .. 2" in msg
    rc, msg = assign([0, -2, 3, 1])
    assert rc == -1 and "member[1] = -2 outside -1 .. 2" in msg
    assert ens.info()["assigned"] == 4                                # a refused assignment leaves the old one
    assert L.gel_wind_ensemble_assign(ens._p, 2, None) == -1 and L.gel_wind_ensemble_assign(ens._p, -1, None) == -1
    assert L.gel_wind_ensemble_assign(ens._p, 0, None) == 0 and ens.info()["assigned"] == 0
    ens.assign([1, 1, -1])
    # an assigned B that does not match, an ensemble of another handle, a host-only handle -- in that order of precedence
    plan, plan_o = E.propagation_plan(steps=1, restart="chain"), other.propagation_plan(steps=1, restart="node")
    X = np.zeros((3, E.nvars))
    with pytest.raises(_lib.GelatoAmdError, match="assigned 3 vectors, the call has B = 2"):
        plan.apply(X[:2], ensemble=ens)
    with pytest.raises(_lib.GelatoAmdError, match="host-only handle"):
        plan.apply(X, ensemble=ens)
    with pytest.raises(_lib.GelatoAmdError, match="host-only handle"):
        plan.apply_device(3, 1, 1, ensemble=ens)
    with pytest.raises(_lib.GelatoAmdError, match="B = 4"):
        E.output_table_batch(np.zeros((4, E.nvars)), 0.0, 0.0, ensemble=ens)
    with pytest.raises(_lib.GelatoAmdError, match="host-only handle"):
        E.output_table_batch(X, 0.0, 0.0, ensemble=ens)
    with pytest.raises(_lib.GelatoAmdError, match="host-only handle"):
        E.output_table_batch_device(3, 1, 0.0, 0.0, d_out=1, ensemble=ens)
    # another handle: the Python layer refuses by name, the library on its own too
    with pytest.raises(ValueError, match="another engine"):
        plan_o.apply(X, ensemble=ens)
    with pytest.raises(ValueError, match="another engine"):
        other.output_table_batch(X, 0.0, 0.0, ensemble=ens)
    dp = C.POINTER(C.c_double)
    y = np.zeros(3 * 11 * E.M)
    assert L.gel_propagate_ensemble(plan_o._p, 3, X.ctypes.data_as(dp), None, ens._p, y.ctypes.data_as(dp), None) == -1
    assert "another handle" in L.gel_last_error().decode()
    assert L.gel_output_table_batch_ensemble_device(other._h, 3, 1, None, None, ens._p, 0.0, 0.0, 0, None, 1, None, None) == -1
    assert "another handle" in L.gel_last_error().decode()
    unassigned = E.wind_ensemble(members(32, (4,)))
    with pytest.raises(_lib.GelatoAmdError, match="no vectors yet"):
        plan.apply(X, ensemble=unassigned)
    # ens = NULL is the existing call: the same refusal as gel_propagate_dispersed on a host-only handle
    with pytest.raises(_lib.GelatoAmdError, match="host-only handle"):
        plan.apply(X)
    for o in (unassigned, ens, plan, plan_o):
        o.close()
    other.close()


def test_python_argument_checks():
    from gelato_amd import WindEnsemble, _lib
    E = engine()
    T = members(32, (1, 2))
    with pytest.raises(TypeError, match="float64"):
        E.wind_ensemble(T.astype(np.float32))
    with pytest.raises(ValueError, match=r"\[E, Kw, 3\]"):
        E.wind_ensemble(T[:, :, :2])
    with pytest.raises(ValueError, match=r"\[E, Kw, 3\]"):
        E.wind_ensemble(T[None])
    one = E.wind_ensemble(T[0])                                       # one member, [Kw, 3]
    assert one.info()["E"] == 1 and isinstance(one, WindEnsemble)
    one.close()
    ens = E.wind_ensemble(T)
    with pytest.raises(TypeError, match="integers"):
        ens.assign([0.0, 1.0])
    with pytest.raises(ValueError, match=r"\[B\]"):
        ens.assign([[0, 1]])
    with pytest.raises(ValueError, match="-1 or 0 .. 1"):
        ens.assign([0, 2])
    with pytest.raises(ValueError, match="-1 or 0 .. 1"):
        ens.assign(np.array([0, -2 ** 40]))
    assert ens.assign(np.array([1, -1, 0], dtype=np.int64)) is ens and ens.info()["assigned"] == 3
    assert ens.assign([]).info()["assigned"] == 0
    plan = E.propagation_plan(steps=1)
    with pytest.raises(TypeError, match="WindEnsemble"):
        plan.apply(np.zeros(E.nvars), ensemble=T)
    with pytest.raises(_lib.GelatoAmdError, match="member 2 outside 0 .. 1"):
        ens.member(2)
    ens.close()
    ens.close()                                                       # twice is fine
    with pytest.raises(_lib.GelatoAmdError, match="closed"):
        ens.info()
    with pytest.raises(_lib.GelatoAmdError, match="closed"):
        plan.apply(np.zeros(E.nvars), ensemble=ens)
    plan.close()
    # the ensemble keeps its engine's handle alive, like the plans
    E2 = it.engine(it.prob_of([2, 3]))
    e2 = E2.wind_ensemble(T)
    del E2
    assert e2.info()["Kw"] == 32
    e2.close()


@pytest.mark.parametrize("order", ["blocked", "cyclic", "random"])
def test_assign_members(order):
    from gelato_amd.propagate import assign_members
    for B, E, own in ((10, 5, 0), (67, 5, 0), (67, 5, 3), (7, 3, 0), (3, 5, 1), (1, 1, 0), (0, 2, 0), (4, 2, 4), (65536, 12, 0)):
        m = assign_members(B, E, order=order, seed=7, own=own)
        assert m.dtype == np.int32 and m.shape == (B,)
        assert np.all(m[:own] == -1) and np.all(m[own:] >= 0) and np.all(m[own:] < E)
        c = np.bincount(m[own:], minlength=E)
        assert c.max() - c.min() <= 1, (order, B, E, own, c)
        assert np.array_equal(m, assign_members(B, E, order=order, seed=7, own=own))
    B, E = 60, 5
    m = assign_members(B, E, order=order, seed=1)
    if order == "blocked":
        assert np.array_equal(m, np.arange(B) // -(-B // E))          # b // ceil(B / E) where E divides B
        assert np.all(np.diff(assign_members(67, 5, order=order)) >= 0)
    elif order == "cyclic":
        assert np.array_equal(m, np.arange(B) % E)
    else:
        assert not np.array_equal(m, assign_members(B, E, order=order, seed=2))
        assert np.array_equal(np.sort(m), np.sort(np.arange(B) % E))
    for bad in (dict(B=-1, E=2), dict(B=3, E=0), dict(B=3, E=2, own=4), dict(B=3, E=2, own=-1), dict(B=3, E=2, order="sorted")):
        with pytest.raises(ValueError):
            assign_members(**bad)


def test_availability_reduction_on_hand_made_peaks():
    from gelato_amd.montecarlo import availability_from_peaks
    # 3 members x 2 replicas, blocked.  Q_alpha: member 1 fails only through its second replica; alt has a (lower, upper) limit that
    # member 2 misses from below; member 0 passes both
    nan = np.nan
    peaks = {"Q_alpha": {"max": np.array([10.0, 12.0, 11.0, 30.0, 5.0, 6.0]), "argmax": np.array([3, 4, 5, 6, 7, 8]),
                         "min": np.array([0.0, -1.0, 0.5, 0.25, 0.0, 0.0]), "argmin": np.array([0, 1, 0, 2, 0, 0])},
             "altitude": {"max": np.array([90.0, 91.0, 92.0, 93.0, 94.0, 95.0]), "argmax": np.array([9] * 6),
                          "min": np.array([1.0, 2.0, 1.5, 1.25, -3.0, 2.0]), "argmin": np.array([0, 0, 0, 0, 4, 0])}}
    members_ = np.array([0, 0, 1, 1, 2, 2])
    R = availability_from_peaks(peaks, members_, {"Q_alpha": 20.0, "altitude": (0.0, 100.0)})
    assert R["columns"] == ["Q_alpha", "altitude"] and R["limits"] == {"Q_alpha": (None, 20.0), "altitude": (0.0, 100.0)}
    assert np.array_equal(R["ok"], [True, False, False]) and R["availability"] == 1.0 / 3.0 and np.array_equal(R["failing"], [1, 2])
    assert np.array_equal(R["worst_max"]["Q_alpha"], [12.0, 30.0, 6.0]) and np.array_equal(R["flight_max"]["Q_alpha"], [1, 3, 5])
    assert np.array_equal(R["node_max"]["Q_alpha"], [4, 6, 8])
    assert np.array_equal(R["worst_min"]["Q_alpha"], [-1.0, 0.25, 0.0]) and np.array_equal(R["flight_min"]["Q_alpha"], [1, 3, 4])   # a tie: the first
    assert np.array_equal(R["node_min"]["Q_alpha"], [1, 2, 0])
    assert np.array_equal(R["ok_by_column"]["Q_alpha"], [True, False, True]) and np.array_equal(R["ok_by_column"]["altitude"], [True, True, False])
    assert np.array_equal(R["worst_min"]["altitude"], [1.0, 1.25, -3.0]) and np.array_equal(R["flight_min"]["altitude"], [0, 3, 4])
    # at the limit is within it
    assert availability_from_peaks(peaks, members_, {"Q_alpha": 30.0})["ok"].all()
    assert np.array_equal(availability_from_peaks(peaks, members_, {"Q_alpha": np.nextafter(30.0, 0.0)})["ok"], [True, False, True])
    # a NaN peak: the member fails although its other replica is within the limit; the worst values leave the NaN out
    pk = {"Q_alpha": {k: v.copy() for k, v in peaks["Q_alpha"].items()}}
    pk["Q_alpha"]["max"] = np.array([10.0, nan, 11.0, 12.0, nan, nan])
    pk["Q_alpha"]["argmax"] = np.array([3, -1, 5, 6, -1, -1])
    R = availability_from_peaks(pk, members_, {"Q_alpha": 20.0})
    assert np.array_equal(R["ok"], [False, True, False]) and R["availability"] == 1.0 / 3.0
    assert R["worst_max"]["Q_alpha"][0] == 10.0 and R["flight_max"]["Q_alpha"][0] == 0
    assert np.isnan(R["worst_max"]["Q_alpha"][2]) and R["flight_max"]["Q_alpha"][2] == -1 and R["node_max"]["Q_alpha"][2] == -1
    # cyclic members, E given
    R = availability_from_peaks(peaks, np.array([0, 1, 2, 0, 1, 2]), {"Q_alpha": (None, 20.0)}, E=3)
    assert np.array_equal(R["ok"], [False, True, True]) and np.array_equal(R["flight_max"]["Q_alpha"], [3, 1, 2])
    for bad in (dict(members=[0, 0, 1, 1, 3, 3]),                      # member 2 has no flight
                dict(members=[0, 0, 1, 1, -1, 2]), dict(members=[0, 0, 1, 1, 2, 2], E=2), dict(members=[]),
                dict(members=[0, 0, 1, 1, 2, 2], limits={}), dict(members=[0, 0, 1, 1, 2, 2], limits={"M": 1.0}),
                dict(members=[0, 0, 1, 1, 2, 2], limits={"Q_alpha": (None, None)}), dict(members=[0, 1, 2], limits={"Q_alpha": 1.0})):
        kw = dict(limits={"Q_alpha": 20.0})
        kw.update(bad)
        with pytest.raises(ValueError):
            availability_from_peaks(peaks, np.asarray(kw.pop("members"), dtype=np.int64), **kw)


@sanitized_lib.needs_toolchain
def test_ensemble_host_code_under_asan_ubsan(tmp_path):
    """create, member, info, assign, every refusal and destroy on host-only handles, in a stand-alone program
    (tests/ensemble_sanitize.c) under AddressSanitizer + UBSan + LeakSanitizer, linked against the sanitized library directly;
    nothing is preloaded and nothing is launched"""
    sanitized_lib.run_program(tmp_path, sanitized_lib.build(tmp_path), "ensemble_sanitize")

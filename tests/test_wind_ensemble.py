"""A Monte-Carlo batch against an ensemble of wind profiles on the device (gel_wind_ensemble*, gel_propagate_ensemble*,
gel_output_table_batch_ensemble*).

The truth is the existing single-table path, which the existing suites pin to the oracle: a vector assigned member e must have,
BIT FOR BIT, what the call without an ensemble returns for the same x and factors on an engine created with wind_table =
tables[e], and a vector assigned -1 what that call returns on the engine itself.  Tests 1 - 3 and 5 carry no tolerance; test 4 (a
member longer than any handle accepts) uses flight_truth's derived 2 E and nothing fitted.

Members: table_cases._wind_table(K, seed) with seed 1976 (the table the table-size suite flies) and three others, and one calm member
with the altitudes of member 1 and both wind columns exactly zero.  The assignment cycles -1, 0, 1, 2, 3, 4 with the vector index, so
every wavefront mixes all six tables, the calm one among them.  Every flight and table call of tests 1 - 6 is a device-form call
with one sentinel row behind each output."""
import numpy as np
import pytest

import flight_truth as ft
import interp_truth as it
import output_batch_truth as obt
import propagate_truth as pt
import states
import table_cases as TC
from test_flight import _bits, check_parity, dispersion
from test_output_batch import same
from test_table_sizes import _batch
from test_table_sizes_flight import VISITS, intervals_visited
from test_wind_ensemble_cpu import members

pytestmark = pytest.mark.gpu
SENTINEL = -7.0
SEEDS = (1976, 12, 13, 14)            # + the calm member of index 4, on member 1's altitudes
B67 = 67
CYCLE = (np.arange(B67) % 6) - 1      # -1, 0, 1, 2, 3, 4, -1, ...
_CACHE = {}


def example():
    """(prob, engine, X [67, nvars], pdict, unitdict): the example and flight_truth.flight_batch cycled to 67 vectors"""
    if "example" not in _CACHE:
        from gelato_amd import Engine, problem
        prob, x0 = it.named("example")
        E = Engine(prob)
        pdict, unitdict, _c, _x = problem.make_problem("example")
        _CACHE["example"] = (prob, E, _batch(list(ft.flight_batch(x0, E)), B67), pdict, unitdict)
    return _CACHE["example"]


def member_engines(key, prob, T):
    """one engine per member: prob with wind_table = T[e] (shared by the tests of a key)"""
    if key not in _CACHE:
        from gelato_amd import Engine
        _CACHE[key] = [Engine(dict(prob, wind_table=T[e].copy())) for e in range(len(T))]
    return _CACHE[key]


def fly_checked(E, plan, X, D=None, ens=None, status=0):
    """the plan on device buffers -> (Y [B, 11 M], err [B, S, 4]); the row behind each output is untouched"""
    import torch
    X = np.ascontiguousarray(np.atleast_2d(X))
    B = X.shape[0]
    dX = torch.from_numpy(X).cuda()
    dD = None if D is None else torch.from_numpy(np.ascontiguousarray(np.asarray(D, dtype=np.float64).reshape(B, E.S, 4))).cuda()
    dY = torch.full((B + 1, 11 * E.M), SENTINEL, dtype=torch.float64, device="cuda")
    dE = torch.full((B + 1, E.S, 4), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    plan.apply_device(B, dX.data_ptr(), dY.data_ptr(), dE.data_ptr(), dD.data_ptr() if dD is not None else 0, ensemble=ens)
    assert E.sync() == status
    Y, err = dY.cpu().numpy(), dE.cpu().numpy()
    assert np.all(Y[B] == SENTINEL) and np.all(err[B] == SENTINEL), "wrote behind the batch"
    return Y[:B], err[:B]


def table_checked(E, X, D=None, ens=None, cols=None, out=True, env=True, pk=True, lat=28.5, lon=-80.5):
    """gel_output_table_batch_ensemble_device -> (table [B, M, nc] | None, env [M, nc, 8] | None, peaks [B, nc, 4] | None)"""
    import torch
    X = np.ascontiguousarray(np.atleast_2d(X))
    B, M, nc = X.shape[0], E.M, 34 if cols is None else len(cols)
    dX = torch.from_numpy(X).cuda()
    dD = None if D is None else torch.from_numpy(np.ascontiguousarray(D)).cuda()
    dO = torch.full((B + 1, M, nc), SENTINEL, dtype=torch.float64, device="cuda")
    dE = torch.full((M + 1, nc, 8), SENTINEL, dtype=torch.float64, device="cuda")
    dP = torch.full((B + 1, nc, 4), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    E.output_table_batch_device(B, dX.data_ptr(), lat, lon, d_dispersion=dD.data_ptr() if dD is not None else 0, columns=cols,
                                d_out=dO.data_ptr() if out else 0, d_env=dE.data_ptr() if env else 0, d_peaks=dP.data_ptr() if pk else 0,
                                ensemble=ens)
    assert E.sync() == 0                                                     # the table calls never raise the status
    O, V, P = dO.cpu().numpy(), dE.cpu().numpy(), dP.cpu().numpy()
    assert np.all(O[B] == SENTINEL) and np.all(V[M] == SENTINEL) and np.all(P[B] == SENTINEL), "wrote behind the batch"
    assert out or np.all(O == SENTINEL)
    assert env or np.all(V == SENTINEL)
    assert pk or np.all(P == SENTINEL)
    return (O[:B] if out else None), (V[:M] if env else None), (P[:B] if pk else None)


def assigned_rows(per_engine, own, assignment):
    """row b of the engine vector b is assigned to: per_engine [E][B, ...], own [B, ...] (-1)"""
    return np.stack([own[b] if m < 0 else per_engine[m][b] for b, m in enumerate(assignment)])


def flown(X, Y, M):
    x = np.array(X, copy=True)
    x[..., :11 * M] = Y
    return x


# ------------------------------------------------------------------ 1. member bits, chain
@pytest.mark.parametrize("dispersed", [False, True])
@pytest.mark.parametrize("K", [2, 32, 33, 160])
def test_member_bits_chain(K, dispersed):
    """prop_kernel<true, true, 1>: one interval, the count and the bisection on either side of lower_count's switch, the 9-row handle
    beside them; the kept interval is left and found again (the intervals the flights visit are counted)"""
    prob, E, X, _pd, _ud = example()
    T = members(K, SEEDS, calm_of=1)
    eng = member_engines(("example", K), prob, T)
    D = dispersion(B67, E.S) if dispersed else None
    ens = E.wind_ensemble(T).assign(CYCLE)
    plan = E.propagation_plan(steps=1, restart="chain")
    Y, err = fly_checked(E, plan, X, D, ens)
    own = fly_checked(E, plan, X, D)
    refs = []
    for e in eng:
        p = e.propagation_plan(steps=1, restart="chain")
        refs.append(fly_checked(e, p, X, D))
        p.close()
    wantY, wantE = assigned_rows([r[0] for r in refs], own[0], CYCLE), assigned_rows([r[1] for r in refs], own[1], CYCLE)
    bad = [b for b in range(B67) if not (np.array_equal(_bits(Y[b]), _bits(wantY[b])) and np.array_equal(_bits(err[b]), _bits(wantE[b])))]
    assert not bad, (K, dispersed, bad[:10], CYCLE[bad[:10]])
    assert np.all(np.isfinite(Y)) and np.all(np.isfinite(err))
    # the wind is felt: the same vector under two different tables differs in its bits (wind factor 0 excepted)
    for b in range(B67):
        felt = D is None or np.any(D[b, :, 3] != 0.0)
        others = [own[0][b]] + [r[0][b] for r in refs]
        mine = int(CYCLE[b]) + 1
        differ = [j for j, o in enumerate(others) if j != mine and not np.array_equal(_bits(o), _bits(Y[b]))]
        if felt:
            assert len(differ) >= 4, (K, b, differ)                          # (the calm member and a table the flight never enters may coincide)
    if K in (33, 160):
        case = {33: "EDGE33", 160: "LONG"}[K]
        for b in (1, 2, 3, 4):                                               # vectors under members 0 .. 3; member 0 is the suite's own table
            e = int(CYCLE[b])
            hit_w, _c = intervals_visited(dict(prob, wind_table=T[e]), flown(X[b], Y[b], E.M))
            print("K = %d member %d (vector %d): the flight visits %d of %d wind intervals" % (K, e, b, hit_w, K - 1))
            if e == 0 and not dispersed:
                assert hit_w >= VISITS[case][0] - 2, (K, hit_w)
            assert hit_w >= 3
    plan.close()
    ens.close()


# ------------------------------------------------------------------ 2. member bits, section and node mode
_COOP = {}


def coop():
    """(prob, engine, X [67, nvars]): the coop mesh over LONG's tables, `climb` and `knots` alternating"""
    if not _COOP:
        from gelato_amd import Engine
        prob, xc = states.table_state("LONG", TC.MESHES["coop"], "climb")
        _p, xk = states.table_state("LONG", TC.MESHES["coop"], "knots")
        _COOP["v"] = (prob, Engine(prob), _batch([xc, xk], B67))
    return _COOP["v"]


@pytest.mark.parametrize("mode", ["section", "node"])
@pytest.mark.parametrize("K", [2, 33, 160])
def test_member_bits_section_and_node(K, mode):
    """prop_kernel<true, false, 1>, k = 2: the node restart puts consecutive lookups of a lane in unrelated intervals (a stale kept
    interval shows here), `knots` puts lookups on breakpoints; and vectors 0, 63, 64 and 66 equal their one-vector calls"""
    prob, E, X = coop()
    T = members(K, SEEDS, calm_of=1)
    eng = member_engines(("coop", K), prob, T)
    turn = np.array([2.0, 0.0, 0.5, 1.0, 0.0])[np.arange(B67) % 5]
    D = 0.9 + 0.2 * np.random.default_rng(67).random((B67, E.S, 4))
    D[:, :, 3] = turn[:, None]
    ens = E.wind_ensemble(T).assign(CYCLE)
    plan = E.propagation_plan(steps=2, restart=mode)
    for disp in (None, D):
        Y, err = fly_checked(E, plan, X, disp, ens)
        own = fly_checked(E, plan, X, disp)
        refs = []
        for e in eng:
            p = e.propagation_plan(steps=2, restart=mode)
            refs.append(fly_checked(e, p, X, disp))
            p.close()
        wantY, wantE = assigned_rows([r[0] for r in refs], own[0], CYCLE), assigned_rows([r[1] for r in refs], own[1], CYCLE)
        bad = [b for b in range(B67) if not (np.array_equal(_bits(Y[b]), _bits(wantY[b])) and np.array_equal(_bits(err[b]), _bits(wantE[b])))]
        assert not bad, (K, mode, disp is not None, bad[:10])
        assert np.all(np.isfinite(Y[:, :E.M]))                               # (the masses: every lane ran)
        assert not np.array_equal(_bits(refs[0][0]), _bits(refs[2][0]))      # two members differ
        one = E.wind_ensemble(T)
        for pos in (0, 63, 64, 66):
            one.assign([CYCLE[pos]])
            y1, e1 = fly_checked(E, plan, X[pos], None if disp is None else disp[pos], one)
            assert np.array_equal(_bits(Y[pos]), _bits(y1[0])) and np.array_equal(_bits(err[pos]), _bits(e1[0])), (K, mode, pos)
        one.close()
    plan.close()
    ens.close()


# ------------------------------------------------------------------ 3. slabs and forms
def test_slabs_forms_and_the_own_table(monkeypatch):
    prob, E, X, _pd, _ud = example()
    T = members(33, SEEDS, calm_of=1)
    D = dispersion(B67, E.S)
    ens = E.wind_ensemble(T).assign(CYCLE)
    plan = E.propagation_plan(steps=1, restart="chain")
    Y, err = fly_checked(E, plan, X, D, ens)
    # slabs of 64 + 3: the second slab reads ITS part of the assignment
    monkeypatch.setenv("GEL_PROP_SLAB", "64")
    assert plan.info()["slab"] == 64
    Ys, errs = fly_checked(E, plan, X, D, ens)
    monkeypatch.delenv("GEL_PROP_SLAB")
    assert plan.info()["slab"] > 64
    assert np.array_equal(_bits(Ys), _bits(Y)) and np.array_equal(_bits(errs), _bits(err))    # (vectors 64 .. 66 are assigned 3, 4, -1, not -1, 0, 1)
    # host form = device form
    Yh, errh, rc = plan.apply(X, dispersion=D, ensemble=ens)
    assert rc == 0 and np.array_equal(_bits(Yh), _bits(Y)) and np.array_equal(_bits(errh), _bits(err))
    Yp, errp, rc = plan.apply(X, ensemble=ens)                               # without factors: the dispersed instantiation, factors of one
    Yq, errq = fly_checked(E, plan, X, np.ones((B67, E.S, 4)), ens)
    assert rc == 0 and np.array_equal(_bits(Yp), _bits(Yq)) and np.array_equal(_bits(errp), _bits(errq))
    # an all -1 assignment = the existing dispersed call = ens NULL
    ens.assign(np.full(B67, -1))
    Ya, erra = fly_checked(E, plan, X, D, ens)
    Y0, err0 = fly_checked(E, plan, X, D)
    assert np.array_equal(_bits(Ya), _bits(Y0)) and np.array_equal(_bits(erra), _bits(err0))
    Yb, errb = fly_checked(E, plan, X, None, ens)
    Y1, err1 = fly_checked(E, plan, X)                                       # the undispersed instantiation
    assert np.array_equal(_bits(Yb), _bits(Y1)) and np.array_equal(_bits(errb), _bits(err1))
    ens.close()
    # a member that is a copy of the handle's own table = -1 (the same flights through the other address)
    own = np.ascontiguousarray(np.asarray(prob["wind_table"], dtype=np.float64))
    ens9 = E.wind_ensemble(np.stack([own, own * np.array([1.0, -1.0, 2.0])])).assign(np.arange(B67) % 2)
    Yc, errc = fly_checked(E, plan, X, D, ens9)
    assert np.array_equal(_bits(Yc[0::2]), _bits(Y0[0::2])) and np.array_equal(_bits(errc[0::2]), _bits(err0[0::2]))
    assert not np.array_equal(_bits(Yc[1]), _bits(Y0[1]))
    t9, e9, p9 = table_checked(E, flown(X, Y0, E.M), D, ens9)
    t0, e0, p0 = table_checked(E, flown(X, Y0, E.M), D)
    assert same(t9[0::2], t0[0::2]) and same(p9[0::2], p0[0::2]) and not same(t9[1], t0[1])
    ens9.assign(np.zeros(B67, dtype=np.int32))
    t9, e9, p9 = table_checked(E, flown(X, Y0, E.M), D, ens9)
    assert same(t9, t0) and same(e9, e0) and same(p9, p0)
    # B = 0 is valid
    ens9.assign([])
    Yz, errz, rc = plan.apply(np.zeros((0, E.nvars)), ensemble=ens9)
    assert rc == 0 and Yz.shape == (0, 11 * E.M)
    ens9.close()
    plan.close()


# ------------------------------------------------------------------ 4. beyond the handle's limit
def test_a_member_longer_than_any_handle_accepts():
    """Kw = 400 (a handle refuses it: tests/test_wind_ensemble_cpu.py), B = 3, chain, k = 1, within 2 E of flight_truth.fly_all on
    a copy of prob with that member as wind_table; the bound around the device's y rejects the neighbouring member"""
    prob, E, X67, _pd, _ud = example()
    X = X67[:3]
    T = members(400, (15, 16, 17))
    ens = E.wind_ensemble(T).assign([0, 1, 2])
    assert ens.info()["device_bytes"] >= 3 * (5 * 400 - 2) * 8
    plan = E.propagation_plan(steps=1, restart="chain")
    Y, err = fly_checked(E, plan, X, None, ens)
    ref = [ft.fly_all(E, plan, dict(prob, wind_table=T[b]), X[b]) for b in range(3)]
    use, _last, worst = check_parity(E, Y, err, ref)
    print("largest share of 2 E used under the Kw = 400 members: y %s err %s" % (np.array2string(use[0], precision=3),
                                                                                 np.array2string(use[1], precision=3)))
    assert all(wy <= 1.0 and we <= 1.0 for wy, we in worst), worst
    Ydev, by = pt.unpack_y(Y[1], E.M), ref[1][1]
    wrong = ft.fly_all(E, plan, dict(prob, wind_table=T[2]), X[1], want_bound=False)[0]
    d = np.abs(wrong - Ydev)
    ok = np.isfinite(d) & (by > 0)
    miss = float((d[ok] / by[ok]).max())
    print("the neighbouring member misses the bound around the device's y by a factor %.3g" % miss)
    assert miss > 1.0e3, miss
    plan.close()
    ens.close()


# ------------------------------------------------------------------ 5. table, peaks, envelope
B300 = 300
CYCLE300 = (np.arange(B300) % 6) - 1
FIVE = ["dynamic_pressure", "Q_alpha", "AOA_total", "M", "altitude"]
EXACT_NODES = (0, 1, 7, 8, 40, 63, 64, 77)


def flights300(K):
    """(x_flown [300, nvars], D [300, S, 4]): test 1's dispersed flights under the K-row ensemble, cycled"""
    key = ("flights", K)
    if key not in _CACHE:
        prob, E, X, _pd, _ud = example()
        D = dispersion(B67, E.S)
        ens = E.wind_ensemble(members(K, SEEDS, calm_of=1)).assign(CYCLE)
        plan = E.propagation_plan(steps=1, restart="chain")
        Y, _err = fly_checked(E, plan, X, D, ens)
        plan.close()
        ens.close()
        xf = flown(X, Y, E.M)
        idx = np.arange(B300) % B67
        _CACHE[key] = (np.ascontiguousarray(xf[idx]), np.ascontiguousarray(D[idx]))
    return _CACHE[key]


@pytest.mark.parametrize("dispersed", [False, True])
@pytest.mark.parametrize("K", [33, 160])
def test_table_peaks_envelope(K, dispersed):
    """B = 300: two envelope blocks (256 + 44).  out and peaks row by row against the per-member engines, env against the stated
    order restated on the assembled table, with the table requested and without it, all 34 columns and five of them"""
    from gelato_amd import Engine
    prob, E, _X, _pd, _ud = example()
    T = members(K, SEEDS, calm_of=1)
    eng = member_engines(("example", K), prob, T)
    xf, D = flights300(K)
    D = D if dispersed else None
    ens = E.wind_ensemble(T).assign(CYCLE300)
    for cols in (None, FIVE):
        tab, env, pk = table_checked(E, xf, D, ens, cols)
        own = table_checked(E, xf, D, None, cols, env=False)
        refs = [table_checked(e, xf, D, None, cols, env=False) for e in eng]
        want_t = assigned_rows([r[0] for r in refs], own[0], CYCLE300)
        want_p = assigned_rows([r[2] for r in refs], own[2], CYCLE300)
        bad = [b for b in range(B300) if not (same(tab[b], want_t[b]) and same(pk[b], want_p[b]))]
        assert not bad, (K, dispersed, cols, bad[:10])
        assert same(pk, obt.peaks_reference(tab))
        names = Engine.OUTPUT_COLUMNS if cols is None else cols
        q = names.index("Q_alpha")
        assert not same(refs[0][0][:, :, q], refs[2][0][:, :, q])            # the wind is felt in the table
        nodes = EXACT_NODES if cols is None else range(E.M)
        differ = [(i, c) for i in nodes for c in range(len(names)) if not same(env[i, c], obt.welford_merge_exact(tab[:, i, c]))]
        assert not differ, (K, dispersed, cols, len(differ), differ[:5])
        _t, env2, pk2 = table_checked(E, xf, D, ens, cols, out=False)       # without the table: outbatch_env_kernel forms the rows
        assert same(env2, env) and same(pk2, pk)
        _t, env3, _p = table_checked(E, xf, D, ens, cols, out=False, pk=False)
        assert same(env3, env)
    # host form = device form
    R = E.output_table_batch(xf, 28.5, -80.5, dispersion=D, columns=FIVE, ensemble=ens)
    assert same(R["table"], tab) and same(np.stack([R["peaks"][c]["max"] for c in FIVE], axis=1), pk[:, :, 2])
    ens.close()


# ------------------------------------------------------------------ 6. status
def test_status_nan_member_and_refusals():
    """member 2 holds a NaN wind entry inside the altitudes flown: exactly its flights are non-finite, from the phase that reaches
    it on; the others keep their bits; gel_sync reports GEL_NONFINITE and the next call is clean; the table call returns GEL_OK
    and reports through count / first_nonfinite.  B = 3 against an assignment of 67: GEL_ERR_ARG with nothing written"""
    import torch
    from gelato_amd import _lib
    prob, E, X, _pd, _ud = example()
    T = members(33, SEEDS, calm_of=1)
    Tn = T.copy()
    rows = (T[2, :, 0] > 4000.0) & (T[2, :, 0] < 12000.0)                    # the rows between 4 and 12 km: every ascent has nodes there
    assert rows.sum() >= 2 and not rows[0] and not rows[-1]
    Tn[2, rows, 1] = np.nan
    D = dispersion(B67, E.S)
    D[:, :, 3] = np.where(D[:, :, 3] == 0.0, 0.5, D[:, :, 3])                # (a wind factor of 0 would still give 0 * NaN = NaN; keep it plain)
    clean = E.wind_ensemble(T).assign(CYCLE)
    ens = E.wind_ensemble(Tn).assign(CYCLE)
    plan = E.propagation_plan(steps=1, restart="chain")
    Y0, err0 = fly_checked(E, plan, X, D, clean)
    Y, err = fly_checked(E, plan, X, D, ens, status=_lib.GEL_NONFINITE)
    hit = CYCLE == 2
    assert hit.sum() == 11
    for b in range(B67):
        if hit[b]:
            fin = np.isfinite(err[b]).all(axis=1)
            s0 = int(np.argmin(fin))
            assert not fin.all() and not fin[s0:].any() and fin[:s0].all(), (b, fin)
            assert np.array_equal(_bits(err[b, :s0]), _bits(err0[b, :s0]))
            assert np.all(np.isfinite(Y[b, E.M:E.M + 3])) and not np.isfinite(Y[b, E.M + 3 * (E.M - 1)])   # position: the first node, the last
        else:
            assert np.array_equal(_bits(Y[b]), _bits(Y0[b])) and np.array_equal(_bits(err[b]), _bits(err0[b])), b
    Y1, err1 = fly_checked(E, plan, X, D, clean)                             # the next call is clean (status 0 inside)
    assert np.array_equal(_bits(Y1), _bits(Y0))
    # the table of the clean flights under the NaN ensemble: GEL_OK, the NaN flights counted out of the columns behind the wind
    xf = flown(X, Y0, E.M)
    tab, env, pk = table_checked(E, xf, D, ens, ["dynamic_pressure", "altitude"])
    tab0, env0, _pk0 = table_checked(E, xf, D, clean, ["dynamic_pressure", "altitude"])
    gone = ~np.isfinite(tab[:, :, 0])
    assert gone.any() and not gone[~hit].any() and gone[hit].any(axis=1).all()
    assert same(tab[~hit], tab0[~hit]) and same(tab[:, :, 1], tab0[:, :, 1])
    i = int(np.nonzero(gone.any(axis=0))[0][0])
    assert env[i, 0, 0] == B67 - gone[:, i].sum() and env[i, 0, 7] == np.nonzero(gone[:, i])[0][0] and env0[i, 0, 7] == -1.0
    # refusals on the device path: nothing is written
    dX = torch.from_numpy(X[:3]).cuda()
    dY = torch.full((4, 11 * E.M), SENTINEL, dtype=torch.float64, device="cuda")
    dO = torch.full((4, E.M, 34), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(_lib.GelatoAmdError, match="assigned 67 vectors, the call has B = 3"):
        plan.apply_device(3, dX.data_ptr(), dY.data_ptr(), ensemble=ens)
    with pytest.raises(_lib.GelatoAmdError, match="assigned 67 vectors, the call has B = 3"):
        E.output_table_batch_device(3, dX.data_ptr(), 0.0, 0.0, d_out=dO.data_ptr(), ensemble=ens)
    assert E.sync() == 0
    assert torch.all(dY == SENTINEL).item() and torch.all(dO == SENTINEL).item()
    clean.assign(CYCLE[:3])                                                  # re-assign and succeed
    Y3, err3 = fly_checked(E, plan, X[:3], D[:3], clean)
    assert np.array_equal(_bits(Y3), _bits(Y0[:3])) and np.array_equal(_bits(err3), _bits(err0[:3]))
    for o in (plan, ens, clean):
        o.close()


# ------------------------------------------------------------------ 7. Python
def test_fly_and_the_montecarlo_readers_take_the_ensemble():
    from gelato_amd import montecarlo as mc, propagate
    prob, E, X67, pdict, unitdict = example()
    B = 12
    X = X67[:B]
    T = members(33, SEEDS, calm_of=1)
    D = propagate.sample_dispersion(B, E.S, 0.03, seed=4)
    m = propagate.assign_members(B, 5, order="cyclic", own=2)
    ens = E.wind_ensemble(T).assign(m)
    lc = pdict["LaunchCondition"]
    plan = E.propagation_plan(steps=2, restart="chain")
    Y, err, rc = plan.apply(X, dispersion=D, ensemble=ens)
    plan.close()
    xf = flown(X, Y, E.M)
    F = propagate.fly(X, pdict, unitdict, steps=1, dispersion=D, engine=E, ensemble=ens)
    assert F["status"] == rc == 0 and np.array_equal(_bits(F["y"]), _bits(Y)) and np.array_equal(_bits(F["err"]), _bits(err))
    F0 = propagate.fly(X, pdict, unitdict, steps=1, dispersion=D, engine=E)
    assert np.array_equal(_bits(F0["y"][:2]), _bits(Y[:2])) and not np.array_equal(_bits(F0["y"][2:]), _bits(Y[2:]))   # own = 2
    R = E.output_table_batch(xf, lc["lat"], lc["lon"], dispersion=D, columns=FIVE, ensemble=ens)
    V = mc.flight_envelope(X, pdict, unitdict, dispersion=D, steps=1, columns=FIVE, engine=E, ensemble=ens)
    assert np.array_equal(_bits(V["x_flown"]), _bits(xf)) and np.array_equal(_bits(V["terminal_miss"]), _bits(err[:, -1]))
    for c in FIVE:
        for f in ("mean", "m2", "min", "max"):
            assert same(V["envelope"][c][f], R["envelope"][c][f]), (c, f)
        assert same(V["peaks"][c]["max"], R["peaks"][c]["max"]) and np.array_equal(V["peaks"][c]["argmax"], R["peaks"][c]["argmax"])
    Q = mc.flight_quantiles(X, pdict, unitdict, [0.0, 1.0], dispersion=D, steps=1, columns=FIVE, engine=E, ensemble=ens)
    assert Q["status"] == 0
    for c in FIVE:                                                           # the extreme quantiles are entries of the same device table
        assert same(Q["node"][c]["lower"][:, 0], R["envelope"][c]["min"]) and same(Q["node"][c]["upper"][:, 1], R["envelope"][c]["max"]), c
        assert Q["peak"][c]["max"]["upper"][1] == R["peaks"][c]["max"].max() and Q["peak"][c]["max"]["who_upper"][1] == np.argmax(R["peaks"][c]["max"])
    Cv = mc.flight_covariance(X, pdict, unitdict, D, steps=1, columns=FIVE, engine=E, ensemble=ens)
    direct = E.batch_comoments(np.ascontiguousarray(R["table"][:, E.M - 1, :]))
    assert Cv["status"] == 0 and Cv["terminal"]["count"] == direct["count"] and direct["count"] >= 2
    assert same(Cv["terminal"]["C"], direct["C"]) and same(Cv["terminal"]["mean_a"], direct["mean_a"])
    ens.close()
    # wind_availability: one vector over the five members; the limit lies between the sorted per-member peaks of Q_alpha
    x = X67[1]
    ens = E.wind_ensemble(T).assign(np.arange(5))
    plan = E.propagation_plan(steps=2, restart="chain")
    Y5, _e5, rc = plan.apply(np.tile(x, (5, 1)), ensemble=ens)
    R5 = E.output_table_batch(flown(np.tile(x, (5, 1)), Y5, E.M), lc["lat"], lc["lon"], columns=["Q_alpha"], table=False, envelope=False, ensemble=ens)
    qa = R5["peaks"]["Q_alpha"]["max"]
    srt = np.sort(qa)
    assert rc == 0 and np.all(np.diff(srt) > 0), qa
    limit = 0.5 * (srt[1] + srt[2])
    A = mc.wind_availability(x, pdict, unitdict, T, {"Q_alpha": limit}, steps=1, engine=E)
    assert A["status"] == 0 and A["dispersion"] is None and np.array_equal(A["members"], np.arange(5))
    assert np.array_equal(A["ok"], qa <= limit) and A["ok"].sum() == 2 and A["availability"] == 0.4
    assert np.array_equal(A["failing"], np.nonzero(qa > limit)[0])
    assert same(A["worst_max"]["Q_alpha"], qa) and np.array_equal(A["flight_max"]["Q_alpha"], np.arange(5))
    assert np.array_equal(A["node_max"]["Q_alpha"], R5["peaks"]["Q_alpha"]["argmax"])
    # replicas with factors: the record is the direct reduction of the Engine-level peaks of the same flights
    m15 = propagate.assign_members(15, 5)
    D15 = propagate.sample_dispersion(15, E.S, 0.02, 9)
    ens.assign(m15)
    Y15, _e, rc = plan.apply(np.tile(x, (15, 1)), dispersion=D15, ensemble=ens)
    R15 = E.output_table_batch(flown(np.tile(x, (15, 1)), Y15, E.M), lc["lat"], lc["lon"], dispersion=D15, columns=["Q_alpha", "dynamic_pressure"],
                               table=False, envelope=False, ensemble=ens)
    worst = np.sort(R15["peaks"]["Q_alpha"]["max"].reshape(5, 3).max(axis=1))
    assert rc == 0 and np.all(np.diff(worst) > 0), worst
    limits = {"Q_alpha": (0.0, 0.5 * (worst[2] + worst[3])), "dynamic_pressure": 1.0e9}
    A2 = mc.wind_availability(x, pdict, unitdict, T, limits, replicas=3, sigma=0.02, seed=9, steps=1, engine=E)
    assert np.array_equal(A2["members"], m15) and np.array_equal(_bits(A2["dispersion"]), _bits(D15))
    want = mc.availability_from_peaks(R15["peaks"], m15, limits, 5)
    for key in ("worst_max", "worst_min"):
        for c in want["columns"]:
            assert same(A2[key][c], want[key][c]), (key, c)
    assert np.array_equal(A2["ok"], want["ok"]) and np.array_equal(A2["flight_max"]["Q_alpha"], want["flight_max"]["Q_alpha"])
    assert A2["availability"] == want["availability"] == 0.6 and A2["ok"].sum() == 3
    plan.close()
    ens.close()

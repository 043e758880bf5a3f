"""The wind-profile sensitivities (gel_propagate_tangent_wind*, gel_propagate_adjoint_wind*) on the plans and
batches tests/test_flight_wind.py does not fly, through the C ABI: node plans, plans whose step count differs by phase (inner
checkpoints in air phases), per-lane seeds and functionals across slab boundaries with and without a wind ensemble, a non-finite
seed in a row the flight reads, and the two-row table.

Truth: tests/golden/g36_flight_wind_plans.npz (80 digits; tests/golden/make_flight_wind_plans.py), vector 1 of the flights
flight_wind_truth.PLAN_FLIGHTS within the carried bounds 2 E / 2 Eg; everything else is bit for bit against another call of the
library that the existing suites pin.  Batches of 130 repeat their vectors with period 64, so that the lanes 64 vectors apart -- the
same place in the next slab of 64 -- fly the same x and factors and differ through their own seed / functional alone."""
import numpy as np
import pytest

import flight_adjoint_truth as at
import flight_tangent_truth as tt
import flight_wind_truth as wt
import mixed_steps as ms
from test_flight_wind import _bits, _case, adjoint_raw, same, tangent_raw

pytestmark = pytest.mark.gpu
B130 = 130
PERIOD = np.arange(B130) % 64


def _plan(E, mode, steps):
    return E.propagation_plan(steps=tt.steps_of(steps, E.S), restart=mode)


_DEV = {}


def _device(name):
    """the device's results of one of wt.PLAN_NAMES, computed once: the batch of three, the seven seeds (shared) and the twelve
    functionals (shared) -> (engine, dY [3, 7, 11 M], GW [3, 12, Kw, 2] | None)"""
    if name not in _DEV:
        case, mode, steps = wt.PLAN_FLIGHTS[name]
        prob, E, X, disp = _case(case)
        g = wt.load_plan(name)
        _w, dX, dD = wt.seeds(prob, X[wt.TRUTH_VEC])
        plan = _plan(E, mode, steps)
        Y, dY = tangent_raw(E, plan, X, disp, dX, dD, g["dW"], True)
        GW = None
        if name in wt.PLAN_ADJOINT:
            Ya, _gx, _gd, GW = adjoint_raw(E, plan, X, disp, at.pack_lam(wt.functionals(prob)), True)
            assert same(Ya, Y)
        plan.close()
        _DEV[name] = (E, dY, GW)
    return _DEV[name]


def _batch130(X, disp):
    """130 vectors that repeat with period 64 (the three of the case, cycled)"""
    idx = PERIOD % X.shape[0]
    return np.ascontiguousarray(X[idx]), np.ascontiguousarray(disp[idx])


# ------------------------------------------------------------------ 1. the truth
@pytest.mark.parametrize("name", wt.PLAN_NAMES)
def test_truth(name):
    """dy within 2 E of g36 for every seed and entry, gwind within 2 Eg for every functional and row; nothing masked, an entry with a
    zero bound exact"""
    g = wt.load_plan(name)
    E, dY, GW = _device(name)
    b = wt.TRUTH_VEC
    got = tt.unpack_dy(dY[b], E.M)
    use_t = np.array([wt.miss(got[d], g["dy"][d], g["bound"][d]) for d in range(len(wt.SEEDS))])
    print("%s: largest |error| / E per seed %s" % (name, np.array2string(use_t, precision=3)))
    if GW is not None:
        use_a = np.array([wt.miss(GW[b, q], g["gW"][q], g["Eg"][q]) for q in range(wt.NQ)])
        print("%s: largest |error| / Eg per functional %s" % (name, np.array2string(use_a, precision=3)))
    assert np.all(use_t <= 2.0), (name, use_t)
    if GW is not None:
        assert np.all(use_a <= 2.0), (name, use_a)
        assert GW.shape == (3, wt.NQ) + g["gW"].shape[1:]
    else:
        assert name == "W-node"


# ------------------------------------------------------------------ 2. duality on the device
@pytest.mark.parametrize("name", wt.PLAN_ADJOINT)
def test_device_duality(name):
    """|<lam, dy(dW)> - <gwind, dW>| <= sum |lam| 2 E + sum 2 Eg |dW| for the pure wind seeds"""
    prob = _case(wt.PLAN_FLIGHTS[name][0])[0]
    g = wt.load_plan(name)
    E, dY, GW = _device(name)
    b = wt.TRUTH_VEC
    lam = wt.functionals(prob)
    dy = tt.unpack_dy(dY[b], E.M)
    for q in range(wt.NQ):
        for d in range(6):
            lhs, rhs = (lam[q] * dy[d]).sum(), (GW[b, q] * g["dW"][d]).sum()
            tol = (np.abs(lam[q]) * 2 * g["bound"][d]).sum() + (2 * g["Eg"][q] * np.abs(g["dW"][d])).sum()
            assert abs(lhs - rhs) <= tol, (name, q, wt.SEEDS[d], lhs, rhs, tol)


# ------------------------------------------------------------------ 3. the rolled plan
@pytest.mark.parametrize("name", wt.PLAN_E)
def test_rolled_plan_rejected(name):
    """the device flying the rolled step assignment misses 2 E / 2 Eg of the right plan's truth by more than 1e3 in dy(dW) and in
    gwind, as the stored 80-digit flight of the rolled plan does"""
    case, mode, steps = wt.PLAN_FLIGHTS[name]
    prob, E, X, disp = _case(case)
    g = wt.load_plan(name)
    _w, dX, dD = wt.seeds(prob, X[wt.TRUTH_VEC])
    plan = _plan(E, mode, ms.wrong_steps(steps, "rolled"))
    _Y, dY = tangent_raw(E, plan, X, disp, dX, dD, g["dW"], True)
    _Y, _gx, _gd, GW = adjoint_raw(E, plan, X, disp, at.pack_lam(wt.functionals(prob)), True)
    plan.close()
    b = wt.TRUTH_VEC
    dy = tt.unpack_dy(dY[b], E.M)
    for what, dev_dy, dev_gw in (("device", dy, GW[b]), ("stored", g["dy_rolled"], g["gW_rolled"])):
        t_dy = max(wt.miss_bounded(dev_dy[d], g["dy"][d], 2 * g["bound"][d]) for d in range(6))
        t_gw = max(wt.miss_bounded(dev_gw[q], g["gW"][q], 2 * g["Eg"][q]) for q in range(wt.NQ))
        print("%s, rolled steps, %s: misses 2 E by %.3g in dy(dW), 2 Eg by %.3g in gwind" % (name, what, t_dy, t_gw))
        assert t_dy > 1.0e3 and t_gw > 1.0e3, (name, what, t_dy, t_gw)


# ------------------------------------------------------------------ 4. the node plan, bits
def test_node_plan_bits():
    """proptan_kernel<false, 2> with Pd.restart (one node interval per lane, j0 = seg - seg0): (a) the rows xa, xa + 1 of every phase
    are the section plan's bits; (b) a zero wind seed gives gel_propagate_tangent's; (c) P = 1, per-vector copies, the device form;
    (d) 2^k; (e) the rows past a phase's first interval are NOT the section plan's, by more than 1e3 of 2 E"""
    case, mode, steps = wt.PLAN_FLIGHTS["W-node"]
    prob, E, X, disp = _case(case)
    g = wt.load_plan("W-node")
    _w, dX7, dD7 = wt.seeds(prob, X[wt.TRUTH_VEC])
    sel = [6, 5, 0]                     # dx, ddisp and dwind together; dwind alone: dense, the bump
    dW, dX, dD = g["dW"][sel], dX7[sel], dD7[sel]
    M = E.M
    first, later = wt.node_rows(tt.layout(prob)[0])
    node, section = _plan(E, "node", 1), _plan(E, "section", 1)
    Y, dY = tangent_raw(E, node, X, disp, dX, dD, dW, True)
    Ys, dYs = tangent_raw(E, section, X, disp, dX, dD, dW, True)
    dy, dys = tt.unpack_dy(dY, M), tt.unpack_dy(dYs, M)
    # (a) the rows xa and xa + 1 of every phase are the section plan's
    assert same(dy[:, :, first], dys[:, :, first])
    _y, dYw = tangent_raw(E, node, X, disp, None, None, dW[1:], True)
    _y, dYsw = tangent_raw(E, section, X, disp, None, None, dW[1:], True)
    assert same(dYw, dY[:, 1:]) and same(tt.unpack_dy(dYw, M)[:, :, first], tt.unpack_dy(dYsw, M)[:, :, first]) and np.any(dYw != 0)
    # (e) and the rows past them are not: under the mixed seed every one, under a pure wind seed those of the phases with air
    assert np.all((dy[:, 0, later] != dys[:, 0, later]).any(axis=-1))
    air_later = np.array([r for s, sl in enumerate(ms.phase_rows(tt.layout(prob)[0])) if prob["reference_area"][s] > 0
                          for r in range(sl.start + 2, sl.stop)])
    assert len(air_later) > 0 and np.all((dy[:, 1, air_later] != dys[:, 1, air_later]).any(axis=-1))
    b = wt.TRUTH_VEC
    for d in (6, 5, 0):                 # (the stored section restatement's teeth, around the device's node flight)
        t = wt.miss_bounded(g["dy_section"][d][later], dy[b, sel.index(d)][later], 2 * g["bound"][d][later])
        assert t > 1.0e3, (wt.SEEDS[d], t)
    # (b) a zero wind seed: the bits of gel_propagate_tangent on the node plan
    Y0, dY0, rc = node.tangent(X, dX=dX, dispersion=disp, ddispersion=dD, shared=True)
    assert rc == 0
    for form in ("host", "device"):
        Yz, dYz = tangent_raw(E, node, X, disp, dX, dD, np.zeros_like(dW), True, form=form)
        assert same(Yz, Y0) and same(dYz, dY0) and same(Y, Y0), form
    assert not same(dY, dY0)
    # (c) a direction alone, per-vector copies of the shared seeds, the device form
    for i in range(3):
        _y, d1 = tangent_raw(E, node, X, disp, dX[[i]], dD[[i]], dW[[i]], True)
        assert same(d1[:, 0], dY[:, i]), i
    bc = lambda a: np.broadcast_to(a, (3,) + a.shape)   # noqa: E731
    Yc, dYc = tangent_raw(E, node, X, disp, bc(dX), bc(dD), bc(dW), False, form="device")
    assert same(Yc, Y) and same(dYc, dY)
    # (d) 2^k
    for sc in (2.0 ** -3, 2.0 ** 7):
        _y, dYk = tangent_raw(E, node, X, disp, dX * sc, dD * sc, dW * sc, True)
        assert same(dYk, dY * sc), sc
    node.close()
    section.close()


# ------------------------------------------------------------------ 5. phase locality under mixed steps
@pytest.mark.parametrize("slab", [None, "64"])
def test_phase_locality_under_mixed_steps(slab, monkeypatch):
    """B = 130.  Section plans: the rows of phase s of dy, from a pure wind seed and from the mixed seed, are bit for bit those of
    the uniform plan steps = E_STEPS[s]; with one functional per phase supported on that phase's rows, gwind[:, s] is the uniform
    plan's.  Chain plans: a plan that agrees with E_STEPS on the phases 0 .. s and differs later gives the same dy on their rows."""
    prob, E, X3, disp3 = _case("example")
    X, disp = _batch130(X3, disp3)
    g = wt.load_plan("W-E-section")
    _w, dX7, dD7 = wt.seeds(prob, X3[wt.TRUTH_VEC])
    dW, dX, dD = g["dW"][[5, 6]], dX7[[5, 6]], dD7[[5, 6]]
    nn, S, N, M = tt.layout(prob)
    rows = ms.phase_rows(nn)
    lamM = np.zeros((S, M, 11))
    rng = np.random.default_rng(5)
    for s in range(S):
        lamM[s, rows[s]] = rng.standard_normal((nn[s] + 1, 11))
    lam = at.pack_lam(lamM)
    if slab:
        monkeypatch.setenv("GEL_PROP_SLAB", slab)
    want = 3 if slab else 1

    def fly(mode, steps, adjoint):
        plan = _plan(E, mode, steps)
        assert plan.tangent_info(B130, 2, shared=True)["slabs"] == want
        _Y, dY = tangent_raw(E, plan, X, disp, dX, dD, dW, True, form="device" if slab else "host")
        GW = None
        if adjoint:
            assert plan.adjoint_info(B130, S, shared=True, want_wind=True)["slabs"] == want
            GW = adjoint_raw(E, plan, X, disp, lam, True, form="device" if slab else "host")[3]
        plan.close()
        return tt.unpack_dy(dY, M), GW

    dy, GW = fly("section", ms.E_STEPS, True)
    assert np.any(GW[:, :5] != 0) and np.all(GW[:, 5:] == 0.0)                 # (the phases 5 .. 11 fly without air)
    uniform = {k: fly("section", k, True) for k in sorted(set(ms.E_STEPS))}
    for s, k in enumerate(ms.E_STEPS):
        udy, uGW = uniform[k]
        assert same(dy[:, :, rows[s]], udy[:, :, rows[s]]), (s, k)
        assert same(GW[:, s], uGW[:, s]), (s, k)
        others = [v for kk, v in uniform.items() if kk != k]
        if prob["reference_area"][s] > 0:                                      # (and the test can tell the step counts apart)
            assert all(not same(dy[:, 0, rows[s]], o[0][:, 0, rows[s]]) and not same(GW[:, s], o[1][:, s]) for o in others), (s, k)
    cdy, _g = fly("chain", ms.E_STEPS, False)
    for s in (0, 1, 2, 4):
        later = tuple(k % 3 + 1 for k in ms.E_STEPS[s + 1:])
        ady, _g = fly("chain", ms.E_STEPS[:s + 1] + later, False)
        upto = slice(0, rows[s].stop)
        assert same(ady[:, :, upto], cdy[:, :, upto]), s
        assert not same(ady[:, :, rows[s + 1]], cdy[:, :, rows[s + 1]]), s


# ------------------------------------------------------------------ 6. per-lane seeds and functionals across slabs
def _runs(E, plan, monkeypatch, tangent_args, adjoint_args, P, Q, ens=None):
    """the two calls in one slab and in three (GEL_PROP_SLAB=64), host and device form -> [(dY, GX, GD, GW)] of the four runs; the
    device form checks the sentinel row behind every output"""
    out = []
    for slab, want in ((None, 1), ("64", 3)):
        if slab:
            monkeypatch.setenv("GEL_PROP_SLAB", slab)
        assert plan.tangent_info(B130, P, shared=False)["slabs"] == want
        assert plan.adjoint_info(B130, Q, shared=False, want_wind=True, ensemble=ens)["slabs"] == want
        for form in ("host", "device"):
            Y, dY = tangent_raw(E, plan, *tangent_args, False, ens, form=form)
            Ya, GX, GD, GW = adjoint_raw(E, plan, *adjoint_args, False, ens, form=form)
            assert same(Ya, Y)
            out.append((dY, GX, GD, GW))
        if slab:
            monkeypatch.delenv("GEL_PROP_SLAB")
    return out


@pytest.mark.parametrize("mode", ["chain", "section"])
def test_per_lane_seeds_and_functionals_across_slabs(mode, monkeypatch):
    """B = 130, P = Q = 2, shared = 0: every lane has its own random dwind and lam.  The d_dwind / d_gwind offsets of a slab's first
    lane, the re-zeroing of the lanes' wind columns per slab: the bits do not depend on the slab size, and the vectors 0, 64, 65, 129
    are the B = 1 calls with their own seeds / functionals"""
    prob, E, X3, disp3 = _case("example")
    X, disp = _batch130(X3, disp3)
    P = Q = 2
    Kw = E.wind_altitudes.size
    rng = np.random.default_rng(6)
    dW = rng.standard_normal((B130, P, Kw, 2))
    lam = rng.standard_normal((B130, Q, 11 * E.M))
    plan = _plan(E, mode, ms.E_STEPS)
    runs = _runs(E, plan, monkeypatch, (X, disp, None, None, dW), (X, disp, lam), P, Q)
    dY, GX, GD, GW = runs[0]
    assert GW.shape == (B130, Q, Kw, 2) and np.all(np.isfinite(dY)) and np.all(np.isfinite(GW))
    # lanes 64 vectors apart fly the same x and factors: their results differ through their own seed / functional alone
    for b in range(B130 - 64):
        assert same(X[b], X[b + 64]) and same(disp[b], disp[b + 64])
        for p in range(P):
            assert not same(dY[b, p], dY[b + 64, p]) and not same(GW[b, p], GW[b + 64, p]) and not same(GX[b, p], GX[b + 64, p]), (b, p)
    for r in runs[1:]:
        assert all(same(a, c) for a, c in zip(r, runs[0]))
    for b in (0, 64, 65, 129):
        _y, d1 = tangent_raw(E, plan, X[b:b + 1], disp[b:b + 1], None, None, dW[b:b + 1], False)
        _y, gx1, gd1, gw1 = adjoint_raw(E, plan, X[b:b + 1], disp[b:b + 1], lam[b:b + 1], False)
        assert same(d1[0], dY[b]) and same(gw1[0], GW[b]) and same(gx1[0], GX[b]) and same(gd1[0], GD[b]), b
    plan.close()


# ------------------------------------------------------------------ 7. the same under an ensemble
@pytest.mark.parametrize("mode", ["chain", "section"])
def test_per_lane_seeds_across_slabs_under_an_ensemble(mode, monkeypatch):
    """K = 33 members over the 9-row handle (Kg = 33 > Kw), the assignment cycling -1, 0, 1, ...: the slab's part of the assignment
    together with the lane offsets of seeds of 33 rows.  gwind rows at or beyond a lane's own Kw are +0.0; the vectors 0, 64, 129 are
    the calls on their member's handle"""
    from test_flight import dispersion
    from test_wind_ensemble import SEEDS, example, member_engines
    from test_wind_ensemble_cpu import members
    prob, E, X67, _pd, _ud = example()
    K, Kown = 33, E.wind_altitudes.size
    X = np.ascontiguousarray(X67[PERIOD])
    D = np.ascontiguousarray(dispersion(67, E.S)[PERIOD])
    T = members(K, SEEDS, calm_of=1)
    eng = member_engines(("example", K), prob, T)
    cyc = (np.arange(B130) % 6) - 1
    P = Q = 2
    rng = np.random.default_rng(7)
    dW = rng.standard_normal((B130, P, K, 2))
    lam = rng.standard_normal((B130, Q, 11 * E.M))
    ens = E.wind_ensemble(T).assign(cyc)
    plan = _plan(E, mode, ms.E_STEPS)
    assert plan.wind_rows(ens) == K
    runs = _runs(E, plan, monkeypatch, (X, D, None, None, dW), (X, D, lam), P, Q, ens)
    dY, GX, GD, GW = runs[0]
    assert GW.shape == (B130, Q, K, 2)
    for r in runs:
        assert all(same(a, c) for a, c in zip(r, runs[0]))
        own = cyc < 0
        assert np.all(_bits(r[3][own][:, :, Kown:]) == 0) and np.any(r[3][~own][:, :, Kown:] != 0)
    for b in (0, 64, 129):
        m = int(cyc[b])
        Em, Kl = (E, Kown) if m < 0 else (eng[m], K)
        p = _plan(Em, mode, ms.E_STEPS)
        _y, d1 = tangent_raw(Em, p, X[b:b + 1], D[b:b + 1], None, None, dW[b:b + 1, :, :Kl], False)
        _y, gx1, gd1, gw1 = adjoint_raw(Em, p, X[b:b + 1], D[b:b + 1], lam[b:b + 1], False)
        p.close()
        assert same(d1[0], dY[b]) and same(gx1[0], GX[b]) and same(gd1[0], GD[b]) and same(gw1[0], GW[b, :, :Kl]), (b, m)
    assert sorted(int(cyc[b]) for b in (0, 64, 129)) == [-1, 2, 3]
    plan.close()
    ens.close()


# ------------------------------------------------------------------ 8. the status
def test_status_nonfinite_seed_in_a_row_the_flight_reads():
    """shared = 0, NaN in ONE lane's seed at the bump row (g36: stages on both adjacent pieces): gel_sync returns GEL_NONFINITE, that
    lane's dy is not finite, every other (vector, direction) keeps the clean run's bits, the next clean call is clean"""
    from gelato_amd import _lib
    prob, E, X, disp = _case("example")
    g = wt.load_plan("W-E-chain")
    bump = int(g["counts"][wt.COUNTS.index("bump")])
    assert int(g["counts"][wt.COUNTS.index("lo")]) > 0 and int(g["counts"][wt.COUNTS.index("hi")]) > 0
    P = 2
    dW = np.random.default_rng(8).standard_normal((3, P, g["dW"].shape[1], 2))
    bad = dW.copy()
    bad[1, 1, bump, 0] = np.nan
    plan = _plan(E, "chain", ms.E_STEPS)
    Y, dY = tangent_raw(E, plan, X, disp, None, None, dW, False, form="device")
    Yb, dYb = tangent_raw(E, plan, X, disp, None, None, bad, False, form="device", status=_lib.GEL_NONFINITE)
    assert same(Yb, Y) and not np.all(np.isfinite(dYb[1, 1]))
    keep = np.ones((3, P), dtype=bool)
    keep[1, 1] = False
    assert same(dYb[keep], dY[keep]) and np.all(np.isfinite(dY))
    Yc, dYc = tangent_raw(E, plan, X, disp, None, None, dW, False, form="device")       # status 0 inside
    assert same(Yc, Y) and same(dYc, dY)
    plan.close()


# ------------------------------------------------------------------ 9. the shortest table
def test_two_row_table():
    """example@MIN: Kg = 2, gwind [B][Q][2][2]; the row_last seed moves dy (stages over the table clamp onto row 1, which the one piece
    uses too) and so does row_first (row 0 belongs to the only piece); the truth of test_truth holds for it"""
    case, mode, steps = wt.PLAN_FLIGHTS["W-MIN"]
    prob, E, X, disp = _case(case)
    g = wt.load_plan("W-MIN")
    plan = _plan(E, mode, steps)
    assert plan.wind_rows() == 2 and E.wind_altitudes.size == 2
    plan.close()
    Em, dY, GW = _device("W-MIN")
    assert Em is E and GW.shape == (3, wt.NQ, 2, 2) and dY.shape == (3, len(wt.SEEDS), 11 * E.M)
    b = wt.TRUTH_VEC
    dy = tt.unpack_dy(dY[b], E.M)
    for d in (wt.SEEDS.index("row_first"), wt.SEEDS.index("row_last")):
        assert wt.miss(dy[d], g["dy"][d], g["bound"][d]) <= 2.0
        assert np.any(np.abs(dy[d]) > 1.0e3 * 2 * g["bound"][d]), wt.SEEDS[d]
    for q in range(wt.NQ):
        assert wt.miss(GW[b, q], g["gW"][q], g["Eg"][q]) <= 2.0, q
    assert np.all(np.abs(GW[:, 1:7]).reshape(3, 6, 2, 2).max(axis=3) > 0)          # both rows, for every functional that feels the wind

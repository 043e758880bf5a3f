"""prop_kernel's dispersed and chained instantiations over the wind and CA tables of tests/table_cases.py: the kernel
stages the tables like every other (table_doubles of them through 256 threads), and its dispersed form scales the interpolated wind
per lane between the lookup and the wavefront's calm-air vote -- the one place where the lanes of a wavefront share the tables but
not the winds.  tests/test_flight.py flies the example's 9 wind and 7 CA rows only.

Inputs.  The table states (states.table_state) are no trajectories: flown as a chain they leave the tables in the first phase (CPU
restatement: LONG / coop visits 1 wind interval of 159, LONG / pack ends at positions of 1e24 units), and the section mode visits
18 of 159.  Node restart starts every interval from the collocated node, so the lookups stay where check_table_state puts them:
`climb` and `knots` in dispersed node mode (prop_kernel<true, false>) over test_table_sizes.PARAMS.  The chain (prop_kernel<false,
true>, <true, true>) flies the example's own ascent over each of the five table cases (table_cases.with_tables), which stays finite
and, from the restatement's own y, visits the numbers of intervals asserted below.

Every comparison is test_flight.check_parity under flight_truth's 2 E, or bits; no tolerance of its own.  Every call goes through
the device form with one row more than the batch behind each output: status 0, the row untouched."""
import numpy as np
import pytest

import flight_truth as ft
import propagate_truth as pt
import states
import table_cases as TC
from test_flight import _bits, check_parity, dispersion
from test_table_sizes import PARAMS, _batch, _state

pytestmark = pytest.mark.gpu
SENTINEL = -7.0
# the wind / CA intervals the example's ascent (vector 1 of flight_truth.flight_batch, k = 1) visits over each case, from the CPU
# restatement under teeth_dispersion: 1 of 1 | 9 of 31 | 11 of 32 | 20 of 159 | 20 of 159 wind, 1 of 1 | 19 of 31 | 20 of 32 |
# 22 of 47 | 21 of 48 CA; the tests ask for two fewer (the plain chain's y is the one looked at)
VISITS = {"MIN": (1, 1), "EDGE32": (9, 19), "EDGE33": (11, 20), "LONG": (20, 22), "LONGEVEN": (20, 21)}


def apply_checked(E, plan, X, D=None):
    """the plan on device buffers -> (Y [B, 11 M], err [B, S, 4]); the status is 0 and the row behind each output is untouched"""
    import torch
    X = np.ascontiguousarray(np.atleast_2d(X))
    B = X.shape[0]
    dX = torch.from_numpy(X).cuda()
    dD = None if D is None else torch.from_numpy(np.ascontiguousarray(np.asarray(D, dtype=np.float64).reshape(B, E.S, 4))).cuda()
    dY = torch.full((B + 1, 11 * E.M), SENTINEL, dtype=torch.float64, device="cuda")
    dE = torch.full((B + 1, E.S, 4), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    plan.apply_device(B, dX.data_ptr(), dY.data_ptr(), dE.data_ptr(), dD.data_ptr() if dD is not None else 0)
    assert E.sync() == 0
    Y, err = dY.cpu().numpy(), dE.cpu().numpy()
    assert np.all(Y[B] == SENTINEL) and np.all(err[B] == SENTINEL), "wrote behind the batch"
    return Y[:B], err[:B]


def factors(B, S, wind, seed):
    """[B, S, 4]: thrust, mass flow and area distinct per (vector, phase) in [0.9, 1.1]; the wind factor wind[b] in every phase"""
    d = 0.9 + 0.2 * np.random.default_rng(seed).random((B, S, 4))
    assert len(np.unique(d[:, :, :3])) == 3 * B * S
    d[:, :, 3] = np.asarray(wind, dtype=np.float64)[:, None]
    return d


def intervals_visited(prob, x, rows=slice(None)):
    """(wind intervals, CA intervals) that hold a lookup at the state nodes `rows` of x: altitude and Mach number from the oracle's
    table, counted as states.check_table_state counts them"""
    import oracle
    wind, ca = np.asarray(prob["wind_table"]), np.asarray(prob["ca_table"])
    T = states.table_oracle_rows(prob, x)
    alt, mach = T["altitude"][rows], T["M"][rows]
    ok = np.isfinite(alt) & np.isfinite(mach)
    h = np.array([oracle.geopotential_altitude(z) for z in alt[ok]])
    inw = h[(h > wind[0, 0]) & (h <= wind[-1, 0])]
    inc = mach[ok][(mach[ok] > ca[0, 0]) & (mach[ok] <= ca[-1, 0])]
    return (len(set(np.searchsorted(wind[:, 0], inw, side="left") - 1)), len(set(np.searchsorted(ca[:, 0], inc, side="left") - 1)))


def _usage(what, use):
    print("bound usage %s: y %s err %s" % (what, np.array2string(use[0], precision=3), np.array2string(use[1], precision=3)))


@pytest.mark.parametrize("case,mesh", PARAMS)
def test_dispersed_node_restart_on_the_table_states(case, mesh):
    """prop_kernel<true, false>, node restart: `climb` under a wind factor of 2 and `knots` under 0.5 in one batch (the two lanes
    share the staged tables, not the winds), thrust, mass flow and area factors distinct per (vector, phase), k = 1 and 2, against
    flight_truth.fly_all(restart="node") within 2 E.  The start nodes are the collocated ones, so the lookups cover what
    test_states_are_where_they_claim_to_be asserts of the states -- asserted here from the states, under the scaled wind."""
    from gelato_amd import Engine
    prob, xc = _state(case, mesh, "climb")
    _p, xk = _state(case, mesh, "knots")
    nn = TC.MESHES[mesh]
    wind, ca = TC.CASES[case]
    E = Engine(prob)
    X = np.stack([xc, xk])
    D = factors(2, E.S, [2.0, 0.5], seed=sum(nn))
    Ma = sum(nn) + len(nn) - (nn[-1] + 1)
    for b, vector in enumerate(("climb", "knots")):
        states.check_table_state(case, nn, vector)                       # the promises, knots on both sides included
        hit_w, hit_c = intervals_visited(ft.dispersed_prob(prob, 0, D[b, 0]), X[b], slice(0, Ma))
        inside = Ma - 5
        if vector == "climb":
            assert hit_w >= min((len(wind) - 1 + 1) // 2, inside, len(wind) - 3), (case, mesh, hit_w)
            assert hit_c >= (len(ca) - 1 + 1) // 2, (case, mesh, hit_c)
        if (case, mesh, vector) == ("LONG", "coop", "climb"):
            assert hit_w >= 80 and hit_c >= 24
    for k in (1, 2):
        plan = E.propagation_plan(steps=k, restart="node")
        ref = [ft.fly_all(E, plan, prob, X[b], disp=D[b], restart="node") for b in range(2)]
        Y, err = apply_checked(E, plan, X, D)
        use, _last, worst = check_parity(E, Y, err, ref)
        _usage("%s/%s k=%d node restart dispersed" % (case, mesh, k), use)
        assert all(wy <= 1.0 and we <= 1.0 for wy, we in worst), (case, mesh, k, worst)
        Y0, _e0 = apply_checked(E, plan, X)
        assert not np.array_equal(_bits(Y0), _bits(Y))                    # the factors matter
        plan.close()
    E.close()


_EXAMPLE = {}


def _example_over(case):
    """(prob, engine, X [3, nvars]) of the example over the case's tables"""
    if case not in _EXAMPLE:
        import interp_truth as it
        from gelato_amd import Engine
        prob0, x0 = it.named("example")
        prob = TC.with_tables(prob0, case)
        E = Engine(prob)
        _EXAMPLE[case] = (prob, E, ft.flight_batch(x0, E))
    return _EXAMPLE[case]


@pytest.mark.parametrize("case", list(TC.CASES))
def test_chain_of_the_example_over_the_tables(case):
    """prop_kernel<false, true> and <true, true>: the example's batch of three as one chain per vector, k = 1, over each table
    case -- plain against fly_all, dispersed with test_flight.dispersion (wind factors 0, 1, 2 mixed inside the wavefront) -- within
    2 E.  The flight stays in the tables: the intervals its restated y visits are counted.  On LONG the bound around the device's y
    rejects the restatement that ignores the wind factor."""
    prob, E, X = _example_over(case)
    B = X.shape[0]
    plan = E.propagation_plan(steps=1, restart="chain")
    ref = [ft.fly_all(E, plan, prob, X[b]) for b in range(B)]
    Y, err = apply_checked(E, plan, X)
    use, _last, worst = check_parity(E, Y, err, ref)
    _usage("example over %s k=1 chain" % case, use)
    assert all(wy <= 1.0 and we <= 1.0 for wy, we in worst), (case, worst)
    ry = ref[1][0]
    flown = np.concatenate([ry[:, 0], ry[:, 1:4].ravel(), ry[:, 4:7].ravel(), ry[:, 7:11].ravel(), X[1, 11 * E.M:]])
    hit_w, hit_c = intervals_visited(prob, flown)
    print("example over %s: the restated chain visits %d of %d wind and %d of %d CA intervals" % (
        case, hit_w, len(TC.CASES[case][0]) - 1, hit_c, len(TC.CASES[case][1]) - 1))
    assert hit_w >= max(VISITS[case][0] - 2, 1) and hit_c >= max(VISITS[case][1] - 2, 1), (case, hit_w, hit_c)
    D = dispersion(B, E.S)
    refd = [ft.fly_all(E, plan, prob, X[b], disp=D[b]) for b in range(B)]
    Yd, errd = apply_checked(E, plan, X, D)
    use, _last, worst = check_parity(E, Yd, errd, refd)
    _usage("example over %s k=1 chain dispersed" % case, use)
    assert all(wy <= 1.0 and we <= 1.0 for wy, we in worst), (case, worst)
    assert not np.array_equal(_bits(Yd), _bits(Y))
    if case == "LONG":
        teeth = ft.teeth_dispersion(E.S)
        Yt, _et = apply_checked(E, plan, X[1], teeth)
        Ydev = pt.unpack_y(Yt[0], E.M)
        ty, tby, _re, _be = ft.fly_all(E, plan, prob, X[1], disp=teeth)
        assert np.all(np.abs(Ydev - ty) <= tby)
        miss = ft.mutant_miss(E, plan, prob, X[1], teeth, "no_wind_factor", Ydev, tby)
        print("example over LONG: ignoring the wind factor misses the bound around the device's y by a factor %.3g" % miss)
        assert miss > 1.0e3, miss
    plan.close()


@pytest.mark.parametrize("mode", ["node", "section"])
@pytest.mark.parametrize("case", ["LONG", "LONGEVEN"])
def test_bits_of_a_vector_in_a_mixed_batch(case, mode):
    """prop_kernel<true, false> on the coop mesh: 67 vectors, `climb` and `knots` alternating, every vector its own thrust, mass
    flow and area factors and a wind factor of 2, 0, 0.5, 1, 0 by turns (calm and windy lanes side by side in the wavefront).  The
    vectors at 0, 63, 64 and 66 have the bits of their one-vector calls; and in a batch whose EVERY wind factor is 0 -- the whole
    wavefront takes the calm branch on a windy handle -- the vectors that were calm in the mixed batch keep their bits."""
    from gelato_amd import Engine
    prob, xc = _state(case, "coop", "climb")
    _p, xk = _state(case, "coop", "knots")
    assert np.abs(np.asarray(prob["wind_table"])[:, 1:]).min() > 0.0          # a windy handle: no row is calm
    E = Engine(prob)
    B = 67
    X = _batch([xc, xk], B)
    turn = np.array([2.0, 0.0, 0.5, 1.0, 0.0])[np.arange(B) % 5]
    D = factors(B, E.S, turn, seed=67)
    plan = E.propagation_plan(steps=2, restart=mode)
    Y, err = apply_checked(E, plan, X, D)
    assert np.all(np.isfinite(Y[:, :E.M]))                                    # (the masses: every lane ran)
    for pos in (0, 63, 64, 66):
        y1, e1 = apply_checked(E, plan, X[pos], D[pos])
        assert np.array_equal(_bits(Y[pos]), _bits(y1[0])) and np.array_equal(_bits(err[pos]), _bits(e1[0])), (case, mode, pos)
    Dz = D.copy()
    Dz[:, :, 3] = 0.0
    Yz, errz = apply_checked(E, plan, X, Dz)
    calm = turn == 0.0
    assert calm.sum() >= 26 and calm[64] and calm[66] and not calm[0] and not calm[63]
    assert np.array_equal(_bits(Yz[calm]), _bits(Y[calm])) and np.array_equal(_bits(errz[calm]), _bits(err[calm])), (case, mode)
    windy = ~calm & (turn != 1.0)
    assert all(not np.array_equal(_bits(Yz[b]), _bits(Y[b])) for b in np.nonzero(windy)[0]), (case, mode)   # the wind is felt
    plan.close()
    E.close()

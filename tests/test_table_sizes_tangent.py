"""proptan_kernel over the wind and CA tables of tests/table_cases.py: the kernel reads the tables where the
handle keeps them (global memory; it stages nothing into LDS) AND reads their slope regions behind them (the tangents of the
interpolants), whose places depend on the row counts.  The
example's batch of three is flown as one chain per vector, k = 1, over each of the five table cases (the flight that
tests/test_table_sizes_flight.py shows to stay inside the tables):
  y    bit for bit gel_propagate_dispersed's -- prop_kernel<true, true>, held to its truth over these tables there;
  dy   over EDGE32 (the last size the rows are counted over) and LONG (bisection; an odd number of staged doubles) within 2 E of the
       60-digit truth of tests/golden/g30_flight_tangent.npz for all eleven seeds; over every case the wind factor's and the
       position's directions are finite and move the flight, and a seed scaled by 2^4 scales dy bit for bit.
Every call goes through the device form with one row more than the batch behind each output: status 0, the row untouched."""
import numpy as np
import pytest

import flight_tangent_truth as tt
import propagate_truth as pt
import table_cases as TC

pytestmark = pytest.mark.gpu
SENTINEL = -7.0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def tangent_checked(E, plan, X, D, dX, dD):
    """the plan's tangent on device buffers -> (Y [B, 11 M], dY [B, P, 11 M]); status 0, the row behind each output untouched"""
    import torch
    B, P = dX.shape[:2]
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (X, D, dX, dD)]
    dY = torch.full((B + 1, 11 * E.M), SENTINEL, dtype=torch.float64, device="cuda")
    ddY = torch.full((B + 1, P, 11 * E.M), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    plan.tangent_device(B, P, t[0].data_ptr(), dY.data_ptr(), ddY.data_ptr(), d_dx=t[2].data_ptr(), d_dispersion=t[1].data_ptr(),
                        d_ddispersion=t[3].data_ptr())
    assert E.sync() == 0
    Y, dYh = dY.cpu().numpy(), ddY.cpu().numpy()
    assert np.all(Y[B] == SENTINEL) and np.all(dYh[B] == SENTINEL), "wrote behind the batch"
    return Y[:B], dYh[:B]


@pytest.mark.parametrize("case", list(TC.CASES))
def test_tangent_of_the_example_over_the_tables(case):
    from gelato_amd import Engine
    prob, X, disp = tt.case("example@" + case)
    assert np.asarray(prob["wind_table"]).shape[0] == TC.CASES[case][0].shape[0]
    E = Engine(prob)
    seeds = [tt.directions(prob, X[b]) for b in range(3)]
    dX, dD = np.stack([s[0] for s in seeds]), np.stack([s[1] for s in seeds])
    plan = E.propagation_plan(steps=1, restart="chain")
    Y, dY = tangent_checked(E, plan, X, disp, dX, dD)
    Y0, _e, rc = plan.apply(X, want_err=False, dispersion=disp)
    assert rc == 0 and np.array_equal(_bits(Y), _bits(Y0)), case
    un = tt.unpack_dy(dY, E.M)                                                  # [B, P, M, 11]
    assert np.all(np.isfinite(dY))
    wind, posy = tt.DIRECTIONS.index("wind_all"), tt.DIRECTIONS.index("position0_y")
    assert np.all(np.abs(un[:, wind, -1, 1:7]).max(axis=1) > 0) and np.all(np.abs(un[:, posy, -1, 1:7]).max(axis=1) > 0), case
    _Y, dY16 = tangent_checked(E, plan, X, disp, dX * 16.0, dD * 16.0)
    assert np.array_equal(_bits(dY16), _bits(dY * 16.0)), case
    flight = ("example@" + case, "chain", 1)
    if flight in tt.TABLE_FLIGHTS:
        g = tt.load(flight)
        b = tt.TRUTH_VEC
        assert np.array_equal(_bits(g["x"]), _bits(X[b])) and np.array_equal(_bits(g["disp"]), _bits(disp[b]))
        d = np.abs(un[b] - g["dy"])
        bound = 2 * g["bound"]
        with np.errstate(divide="ignore", invalid="ignore"):
            share = np.where(bound > 0, d / bound, np.where(d == 0, 0.0, np.inf))
        use = [float(share[..., a:c].max()) for a, c in pt.GROUP_COLS]
        print("share of 2 E used, example over %s, per group (mass, position, velocity, quaternion): %s" % (case, np.array2string(np.array(use), precision=3)))
        assert max(use) <= 1.0, (case, use)
    plan.close()
    E.close()

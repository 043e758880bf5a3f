"""Tangent-linear propagation, host side (no GPU; host-only handles): the conditions g30's truth must meet, the
refusals of the new entry points and gel_prop_tangent_info, the Python argument checks, flight_jacobian's seeds,
linear_covariance, and the entry points' validation under AddressSanitizer + UBSan in a stand-alone program."""
import ctypes as C
import os

import numpy as np
import pytest

import flight_tangent_truth as tt
import interp_truth as it
import sanitized_lib


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("flight", tt.FLIGHTS, ids=lambda f: "%s-%s-k%d" % f)
def test_truth_conditions(flight):
    """(a) the whole map's central quotient and (b) the tangent recursion agree to 1e-30 of the direction's largest entry (this
    pins the generator); the forward and the backward quotient agree for every stored entry, so no kink lies within h of any
    stage -- the example's lift-off stage included: the vehicle stands on the pad, but the wind there is not zero, so |v_air| > 0
    (the aerodynamic force has a velocity derivative at that stage) and no table end is hit exactly: no side needs to be held; the
    stored inputs are the case's"""
    g = tt.load(flight)
    prob, X, disp = tt.case(flight[0])
    assert np.array_equal(_bits(g["x"]), _bits(X[tt.TRUTH_VEC])) and np.array_equal(_bits(g["disp"]), _bits(disp[tt.TRUTH_VEC]))
    assert g["dy"].shape == (11, X.shape[1] and tt.layout(prob)[3], 11)
    assert np.all(g["ab"] <= 1e-30), g["ab"]
    for d, name in enumerate(tt.DIRECTIONS):
        big = np.abs(g["dy"][d]).max()
        assert np.abs(g["dy"][d] - g["dy_a"][d]).max() <= 4 * tt.U * big, name     # (both stored rounded to fp64)
        assert np.abs(g["dy_f"][d] - g["dy_b"][d]).max() <= 1e-18 * big + 1e-300, name
        assert np.all(np.isfinite(g["bound"][d])) and np.all(g["bound"][d] >= 0), name
        moves = name not in ("area_all", "wind_all") or flight[0] == "example"
        assert (big > 0) == moves, name
    # the lift-off stage of the example: in the air, off the axis, moving through it
    if flight[0] == "example":
        J0 = g["J"][0]
        assert np.any(J0[4:7, 4:7] != 0.0)          # |v_air| > 0: the force has a velocity derivative there


@pytest.mark.parametrize("flight", tt.TABLE_FLIGHTS, ids=lambda f: "%s-%s-k%d" % f)
def test_truth_conditions_over_the_long_tables(flight):
    """the same two conditions for the flights over tests/table_cases.py's tables, of which g30 keeps dy and the bound alone"""
    g = tt.load(flight)
    prob, X, disp = tt.case(flight[0])
    assert np.array_equal(_bits(g["x"]), _bits(X[tt.TRUTH_VEC])) and np.array_equal(_bits(g["disp"]), _bits(disp[tt.TRUTH_VEC]))
    assert g["dy"].shape == (11, tt.layout(prob)[3], 11) and np.all(g["ab"] <= 1e-30) and np.all(g["fb"] <= 1e-18)
    assert np.all(np.isfinite(g["bound"])) and np.all(np.abs(g["dy"]).max(axis=(1, 2)) > 0)


def test_truth_rejects_wrong_restatements():
    """each wrong restatement, evaluated in fp64 from the stored partials, misses the truth by far more than 2 E in some direction,
    and the correct recursion in fp64 stays inside: the device test cannot pass vacuously"""
    for flight in tt.FLIGHTS:
        g = tt.load(flight)
        prob, X, _d = tt.case(flight[0])
        mats, hs = tt.plan_tables(it.engine(prob), flight[2], flight[1])
        dX, dD = tt.directions(prob, g["x"])
        muts = [m for m in tt.MUTATIONS if not (m == "no_wind_slope" and flight[0] != "example") and not (m == "no_djump" and flight[1] != "chain")]
        for mut in [None] + muts:
            worst = 0.0
            for d in range(11):
                r = tt.recursion(prob, flight[1], flight[2], g["x"], mats, hs, g, dX[d], dD[d], mutate=mut)
                worst = max(worst, miss(r, g["dy"][d], 2 * g["bound"][d]))
            print("%s %s k=%d, %s: at most %.3g of 2 E" % (flight + (mut, worst)))
            assert (worst <= 1.0) if mut is None else (worst > 1.0e3), (flight, mut, worst)


def miss(a, ref, bound):
    d = np.abs(a - ref)
    if np.any((bound == 0) & (d > 0)) or not np.all(np.isfinite(d)):
        return np.inf
    ok = bound > 0
    return float((d[ok] / bound[ok]).max()) if ok.any() else 0.0


NODES, STEPS = [2, 3, 16, 64], [1, 3, 4, 2]


def test_info_and_refusals():
    """gel_prop_tangent_info against the plan's workspace arithmetic; every refusal, a host-only handle's among them"""
    from gelato_amd import _lib
    prob = it.prob_of(NODES)
    E = it.engine(prob)
    L = _lib.lib()
    for mode in ("section", "node", "chain"):
        plan = E.propagation_plan(steps=STEPS, restart=mode)
        pi = plan.info()
        sset = pi["workspace_bytes_per_vector"]
        assert sset == 16 * sum(2 * k * n + 1 for n, k, h in zip(NODES, STEPS, prob["attitude_hold"]) if not h)
        for P in (1, 5, 75):
            for shared in (False, True):
                ti = plan.tangent_info(100000, P, shared)
                per_vec = sset if shared else sset * (1 + P)
                fixed = sset * ((P + 63) // 64 * 64) if shared else 0
                vs = max(64, min(2 ** 20, ((2 ** 30 - fixed) // per_vec) // 64 * 64, (2 ** 31 - 1) // P // 64 * 64))
                assert ti == {"sample_set_bytes": sset, "lanes_per_slab": vs * P, "slabs": -(-100000 // vs)}, (mode, P, shared)
        os.environ["GEL_PROP_SLAB"] = "100"
        try:
            assert plan.tangent_info(1000, 3)["lanes_per_slab"] == 128 * 3 and plan.tangent_info(1000, 3)["slabs"] == 8
        finally:
            del os.environ["GEL_PROP_SLAB"]
        info = (C.c_int64 * 3)()
        for B, P, sh in ((1, 0, 0), (-1, 1, 0), (1, 1, 2), (1, 1, -1), (65536, 65536, 0)):
            assert L.gel_prop_tangent_info(plan._p, B, P, sh, info) == -1, (B, P, sh)
        x = np.zeros(E.nvars); y = np.zeros(11 * E.M); dy = np.zeros(11 * E.M); dd = np.zeros((E.S, 4)); dx = np.zeros(E.nvars)
        p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None   # noqa: E731
        for fn in (L.gel_propagate_tangent, L.gel_propagate_tangent_device):
            dev = fn is L.gel_propagate_tangent_device
            q = (lambda a: a.ctypes.data if a is not None else None) if dev else p
            for B, P, sh, sx, sd, why in ((1, 0, 0, dx, dd, "P < 1"), (65536, 65536, 1, dx, dd, "2^31"), (1, 1, 0, None, None, "both seeds"),
                                          (1, 1, 2, dx, dd, "shared"), (1, 1, 0, dx, dd, "host-only"), (1, 1, 1, None, dd, "host-only")):
                assert fn(plan._p, B, P, sh, q(x), None, q(sx), q(sd), q(y), q(dy)) == -1, why
                assert why in L.gel_last_error().decode(), (why, L.gel_last_error())
        plan.close()


def test_python_argument_checks():
    from gelato_amd import _lib, montecarlo, propagate
    E = it.engine(it.prob_of([3, 4]))
    plan = E.propagation_plan(steps=1, restart="chain")
    X = np.stack([it.random_x(E, 0), it.random_x(E, 1)])
    nv, S = E.nvars, E.S
    with pytest.raises(ValueError):
        plan.tangent(X)                                              # no seed at all
    for dX, kw in ((np.ones((2, 3, nv + 1)), {}), (np.ones((3, nv)), {}), (np.ones((2, 3, nv)), {"shared": True}), (np.ones((1, 3, nv)), {}),
                   (np.ones((2, 0, nv)), {}), (np.ones(nv), {"shared": True})):
        with pytest.raises(ValueError):
            plan.tangent(X, dX=dX, **kw)
    with pytest.raises(ValueError):
        plan.tangent(X, dX=np.ones((2, 3, nv)), ddispersion=np.ones((2, 2, S, 4)))     # P differs between the seeds
    with pytest.raises(ValueError):
        plan.tangent(X, ddispersion=np.ones((3, S, 4)))                                 # [B, P, S, 4] without shared
    with pytest.raises(ValueError):
        plan.tangent(X, dX=np.ones((3, nv)), dispersion=np.ones((3, S, 4)), shared=True)
    for dtype in (np.float32, np.int64):
        with pytest.raises(TypeError):
            plan.tangent(X, dX=np.ones((2, 3, nv), dtype=dtype))
        with pytest.raises(TypeError):
            plan.tangent(X, ddispersion=np.ones((3, S, 4), dtype=dtype), shared=True)
    # a host-only handle does not evaluate: no CPU fallback
    with pytest.raises(_lib.GelatoAmdError, match="host-only"):
        plan.tangent(X, dX=np.ones((3, nv)), shared=True)
    with pytest.raises(_lib.GelatoAmdError, match="host-only"):
        plan.tangent_device(2, 3, 8, 8, 8, d_dx=8, shared=True)   # (refused before a pointer is looked at)
    with pytest.raises(ValueError):
        propagate.flight_jacobian(X, None, None, steps=0, engine=E)
    for bad in ((), ("initial", "initial"), ("states",)):
        with pytest.raises(ValueError):
            propagate.jacobian_seeds([3, 4], [1, 0], wrt=bad)
    for J, sg in ((np.ones(3), 1.0), (np.ones((2, 3)), [1.0, 2.0]), (np.ones((2, 3)), -1.0)):
        with pytest.raises(ValueError):
            montecarlo.linear_covariance(J, sg)
    plan.close()


def test_jacobian_seeds():
    from gelato_amd import propagate
    nn, hold = [3, 4, 2], [1, 0, 0]
    S, N = 3, 9
    M = N + S
    nv = 11 * M + 2 * N + S + 1
    cols, dX, dD = propagate.jacobian_seeds(nn, hold, wrt=("initial", "dispersion", "times", "controls_bias"))
    assert len(cols) == 11 + 4 * S + S + 1 + 2 * 2 and dX.shape == (len(cols), nv) and dD.shape == (len(cols), S, 4)
    assert cols[0] == "initial:mass" and cols[3] == "initial:z" and cols[10] == "initial:q3"
    assert cols[11] == "dispersion:thrust[0]" and cols[11 + 4 * 2 + 3] == "dispersion:wind[2]"
    assert cols[23] == "time[0]" and cols[26] == "time[3]" and cols[27:] == ["u0_bias[1]", "u1_bias[1]", "u0_bias[2]", "u1_bias[2]"]
    assert len(set(cols)) == len(cols)
    for c in range(11):                                  # the lift-off state: row 0 of every state block
        assert np.flatnonzero(dX[c]).tolist() == [tt.sidx(M, 0, c)] and dX[c].sum() == 1.0 and not dD[c].any()
    for s in range(S):
        for f in range(4):
            p = 11 + 4 * s + f
            assert not dX[p].any() and dD[p].sum() == 1.0 and dD[p, s, f] == 1.0
    for i in range(S + 1):
        assert np.flatnonzero(dX[23 + i]).tolist() == [11 * M + 2 * N + i]
    assert np.flatnonzero(dX[27]).tolist() == [11 * M + 2 * (3 + j) for j in range(4)]          # u0 of phase 1's four nodes
    assert np.flatnonzero(dX[30]).tolist() == [11 * M + 2 * (7 + j) + 1 for j in range(2)]      # u1 of phase 2's two nodes
    cols2, dX2, dD2 = propagate.jacobian_seeds(nn, hold)
    assert cols2 == cols[:27] and np.array_equal(dX2, dX[:27]) and np.array_equal(dD2, dD[:27])
    assert propagate.jacobian_seeds(nn, hold, wrt=("times",))[0] == ["time[%d]" % i for i in range(4)]


def test_linear_covariance_hand_case():
    from gelato_amd import montecarlo
    J = np.array([[1.0, 2.0, 0.0], [0.0, -1.0, 3.0]])
    sg = np.array([0.5, 2.0, 1.0])
    C_ = montecarlo.linear_covariance(J, sg)
    assert np.array_equal(C_, np.array([[0.25 + 16.0, -8.0], [-8.0, 4.0 + 9.0]]))
    assert np.array_equal(montecarlo.linear_covariance(J, 2.0), 4.0 * (J @ J.T))
    rng = np.random.default_rng(0)
    Jb, s = rng.standard_normal((4, 7, 30)), rng.random(30)
    Cb = montecarlo.linear_covariance(Jb, s)
    assert Cb.shape == (4, 7, 7) and np.array_equal(_bits(Cb), _bits(np.swapaxes(Cb, 1, 2)))
    ref = np.einsum("bip,p,bjp->bij", Jb, s * s, Jb)
    assert np.abs(Cb - ref).max() <= 64 * tt.U * np.abs(ref).max()
    assert np.all(np.linalg.eigvalsh(Cb) >= -1e-12)
    assert np.array_equal(montecarlo.linear_covariance(J, np.zeros(3)), np.zeros((2, 2)))


@sanitized_lib.needs_toolchain
def test_entry_points_under_asan_ubsan(tmp_path):
    """the new entry points' validation and gel_prop_tangent_info on a host-only handle, in a stand-alone program
    (tests/flight_tangent_sanitize.c) under AddressSanitizer + UBSan + LeakSanitizer; nothing is launched, nothing preloaded"""
    sanitized_lib.run_program(tmp_path, sanitized_lib.build(tmp_path), "flight_tangent_sanitize")

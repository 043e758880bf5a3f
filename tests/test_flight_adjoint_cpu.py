"""Adjoint flight, host side (no GPU; host-only handles): the conditions g31's truth must meet -- duality against the
tangent recursion in 60-digit arithmetic, the fp64 restatement inside half the bound, every wrong restatement far outside --
gel_prop_adjoint_info against the workspace arithmetic, the refusals of the new entry points and the Python argument checks."""
import ctypes as C
import os

import numpy as np
import pytest

import flight_adjoint_truth as at
import flight_tangent_truth as tt
import interp_truth as it
import sanitized_lib

IDS = lambda f: "%s-%s-k%d" % f   # noqa: E731


def _tables(flight):
    prob, _X, _d = tt.case(flight[0])
    return prob, tt.plan_tables(it.engine(prob), flight[2], flight[1])


@pytest.mark.parametrize("flight", tt.FLIGHTS, ids=IDS)
def test_duality_pins_the_restatement(flight):
    """(a) in 60-digit arithmetic, for the 11 seed directions and the 7 functionals: <gx, dX> + <gdisp, dD> = <lam, recursion(dX, dD)>
    to 1e-30 relative; the stored gx and gdisp are that run's, rounded"""
    import mpmath
    mpmath.mp.dps = 60
    mpf = mpmath.mpf
    num = lambda v: mpf(float(v))   # noqa: E731

    def marr(a):
        a = np.asarray(a, dtype=float)
        out = np.empty(a.shape, dtype=object)
        for i in np.ndindex(a.shape):
            out[i] = mpf(float(a[i]))
        return out

    g30, g31 = tt.load(flight), at.load(flight)
    prob, (mats, hs) = _tables(flight)
    st = {k: marr(g30[k]) for k in ("F", "J", "Pu", "Pf", "Jw")}
    xm = marr(g30["x"])
    dX, dD = tt.directions(prob, g30["x"])
    lam = at.functionals(prob, g30["x"])
    dys = [tt.recursion(prob, flight[1], flight[2], xm, mats, hs, st, marr(dX[d]), marr(dD[d]), num=num) for d in range(11)]
    worst = mpf(0)
    for q in range(7):
        lm = marr(lam[q])
        gx, gd = at.adjoint(prob, flight[1], flight[2], xm, mats, hs, st, lm, num=num)
        assert np.array_equal(gx.astype(float), g31["gx"][q]) and np.array_equal(gd.astype(float), g31["gdisp"][q])
        for d in range(11):
            left = (gx * marr(dX[d])).sum() + (gd * marr(dD[d])).sum()
            right = (lm * dys[d]).sum()
            scale = (abs(gx) * abs(marr(dX[d]))).sum() + (abs(gd) * abs(marr(dD[d]))).sum() + (abs(lm) * abs(dys[d])).sum()
            if scale != 0:
                worst = max(worst, abs(left - right) / scale)
            else:
                assert left == right
    print("%s %s k=%d: duality to %.2e" % (flight + (float(worst),)))
    assert worst <= mpf("1e-30")


@pytest.mark.parametrize("flight", tt.FLIGHTS, ids=IDS)
def test_fp64_restatement_inside_half_the_bound(flight):
    """(b) the recursion in fp64 over the stored partials stays within 0.5 x 2 Eg of g31 in every entry, zero pattern included; the
    largest share of 2 Eg per group is printed"""
    g30, g31 = tt.load(flight), at.load(flight)
    prob, (mats, hs) = _tables(flight)
    lam = at.functionals(prob, g30["x"])
    grp = at.groups(prob)
    for q, name in enumerate(at.FUNCTIONALS):
        gx, gd = at.adjoint(prob, flight[1], flight[2], g30["x"], mats, hs, g30, lam[q])
        assert np.all(np.isfinite(g31["Egx"][q])) and np.all(np.isfinite(g31["Egd"][q]))
        assert np.array_equal(gx != 0, g31["gx"][q] != 0) and np.array_equal(gd != 0, g31["gdisp"][q] != 0), name
        shares = {k: at.miss(gx[i], g31["gx"][q][i], 2 * g31["Egx"][q][i]) for k, i in grp.items()}
        shares["factors"] = at.miss(gd, g31["gdisp"][q], 2 * g31["Egd"][q])
        print("%s %s k=%d, %s: " % (flight + (name,)) + ", ".join("%s %.3g" % kv for kv in shares.items()))
        assert max(shares.values()) <= 0.5, (name, shares)


def _mutations(flight):
    return [m for m in at.MUTATIONS if not (m == "no_knot_minus" and flight[1] != "chain")]


@pytest.mark.parametrize("flight", tt.FLIGHTS, ids=IDS)
def test_truth_rejects_wrong_restatements(flight):
    """(c) each wrong restatement, evaluated in fp64 from the stored partials, misses 2 Eg by more than 1e3 in some entry of some
    functional"""
    g30, g31 = tt.load(flight), at.load(flight)
    prob, (mats, hs) = _tables(flight)
    lam = at.functionals(prob, g30["x"])
    for mut in _mutations(flight):
        worst = 0.0
        for q in range(7):
            gx, gd = at.adjoint(prob, flight[1], flight[2], g30["x"], mats, hs, g30, lam[q], mutate=mut)
            worst = max(worst, at.miss(gx, g31["gx"][q], 2 * g31["Egx"][q]), at.miss(gd, g31["gdisp"][q], 2 * g31["Egd"][q]))
        print("%s %s k=%d, %s: %.3g of 2 Eg" % (flight + (mut, worst)))
        assert worst > 1.0e3, (flight, mut, worst)


NODES, STEPS = [2, 3, 16, 64], [1, 3, 4, 2]


def test_info_and_refusals():
    """(d) gel_prop_adjoint_info against the plan's workspace arithmetic; every refusal with its reason in gel_last_error, a
    host-only handle's and a node-restart plan's among them"""
    from gelato_amd import _lib
    prob = it.prob_of(NODES)
    E = it.engine(prob)
    L = _lib.lib()
    S, N = len(NODES), sum(NODES)
    for mode in ("section", "chain"):
        plan = E.propagation_plan(steps=STEPS, restart=mode)
        sset = plan.info()["workspace_bytes_per_vector"]
        lane = sset + 8 * S + 88 * (max(STEPS) - 1)
        for Q in (1, 7, 75):
            for shared in (False, True):
                ai = plan.adjoint_info(100000, Q, shared)
                vs = min(2 ** 20, (2 ** 30 // (sset + Q * lane)) // 64 * 64, min((2 ** 31 - 1) // (N + 1) * 256, 2 ** 31 - 1) // Q // 64 * 64)
                assert vs >= 64
                assert ai == {"lane_bytes": lane, "lanes_per_slab": vs * Q, "slabs": -(-100000 // vs)}, (mode, Q, shared)
        os.environ["GEL_PROP_SLAB"] = "100"
        try:
            assert plan.adjoint_info(1000, 3) == {"lane_bytes": lane, "lanes_per_slab": 128 * 3, "slabs": 8}
        finally:
            del os.environ["GEL_PROP_SLAB"]
        info = (C.c_int64 * 3)()
        for B, Q, sh, why in ((1, 0, 0, "Q < 1"), (-1, 1, 0, "B < 0"), (1, 1, 2, "shared"), (1, 1, -1, "shared"), (65536, 65536, 0, "2^31"),
                              (1, 2 ** 24, 0, "1 GB")):
            assert L.gel_prop_adjoint_info(plan._p, B, Q, sh, info) == -1, (B, Q, sh)
            assert why in L.gel_last_error().decode(), (why, L.gel_last_error())
        assert L.gel_prop_adjoint_info(plan._p, 1, 1, 0, None) == -1
        x = np.zeros(E.nvars); y = np.zeros(11 * E.M); lam = np.zeros(11 * E.M); gx = np.zeros(E.nvars); gd = np.zeros((E.S, 4))
        p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None   # noqa: E731
        for fn in (L.gel_propagate_adjoint, L.gel_propagate_adjoint_device):
            dev = fn is L.gel_propagate_adjoint_device
            q = (lambda a: a.ctypes.data if a is not None else None) if dev else p
            for B, Q, sh, sl, why in ((1, 0, 0, lam, "Q < 1"), (65536, 65536, 1, lam, "2^31"), (1, 1, 0, None, "lam is NULL"),
                                      (1, 1, 2, lam, "shared"), (1, 2 ** 24, 1, lam, "1 GB"), (1, 1, 0, lam, "host-only"),
                                      (0, 1, 1, lam, "host-only")):
                assert fn(plan._p, B, Q, sh, q(x), None, q(sl), q(y), q(gx), q(gd)) == -1, why
                assert why in L.gel_last_error().decode(), (why, L.gel_last_error())
            assert fn(None, 1, 1, 0, q(x), None, q(lam), q(y), q(gx), q(gd)) == -1 and "null plan" in L.gel_last_error().decode()
        plan.close()
    plan = E.propagation_plan(steps=STEPS, restart="node")
    with pytest.raises(_lib.GelatoAmdError, match="GEL_PROP_RESTART_NODE"):
        plan.adjoint_info(1, 1)
    with pytest.raises(_lib.GelatoAmdError, match="GEL_PROP_RESTART_NODE"):
        plan.adjoint(np.zeros((1, E.nvars)), np.zeros((1, 1, 11 * E.M)))
    with pytest.raises(_lib.GelatoAmdError, match="GEL_PROP_RESTART_NODE"):
        plan.adjoint_device(1, 1, 8, 8, 8, 8)
    plan.close()


def test_python_argument_checks():
    from gelato_amd import _lib, propagate
    E = it.engine(it.prob_of([3, 4]))
    plan = E.propagation_plan(steps=1, restart="chain")
    X = np.stack([it.random_x(E, 0), it.random_x(E, 1)])
    ny, S = 11 * E.M, E.S
    for Lam, kw in ((np.ones((2, 3, ny + 1)), {}), (np.ones((3, ny)), {}), (np.ones((2, 3, ny)), {"shared": True}), (np.ones((1, 3, ny)), {}),
                    (np.ones((2, 0, ny)), {}), (np.ones(ny), {"shared": True}), (np.ones(ny), {})):
        with pytest.raises(ValueError):
            plan.adjoint(X, Lam, **kw)
    with pytest.raises(ValueError):
        plan.adjoint(X, np.ones((3, ny)), dispersion=np.ones((3, S, 4)), shared=True)
    for dtype in (np.float32, np.int64):
        with pytest.raises(TypeError):
            plan.adjoint(X, np.ones((2, 3, ny), dtype=dtype))
        with pytest.raises(TypeError):
            plan.adjoint(X, np.ones((3, ny)), dispersion=np.ones((2, S, 4), dtype=dtype), shared=True)
    # a host-only handle does not evaluate: no CPU fallback
    with pytest.raises(_lib.GelatoAmdError, match="host-only"):
        plan.adjoint(X, np.ones((3, ny)), shared=True)
    with pytest.raises(_lib.GelatoAmdError, match="host-only"):
        plan.adjoint_device(2, 3, 8, 8, 8, 8, shared=True)   # (refused before a pointer is looked at)
    with pytest.raises(_lib.GelatoAmdError, match="lam is NULL"):
        plan.adjoint_device(2, 3, 8, 0, 8, 8)
    with pytest.raises(ValueError):
        propagate.flight_gradient(X, None, None, steps=0, engine=E)
    for bad in (("nonsense",), ("rows",), ("terminal", 1), ()):
        with pytest.raises(ValueError):
            propagate.flight_gradient(X[0], None, None, of=bad, engine=E)
    plan.close()


@sanitized_lib.needs_toolchain
def test_entry_points_under_asan_ubsan(tmp_path):
    """the new entry points' validation and gel_prop_adjoint_info on a host-only handle, in a stand-alone program
    (tests/flight_adjoint_sanitize.c) under AddressSanitizer + UBSan + LeakSanitizer; nothing is launched, nothing preloaded"""
    sanitized_lib.run_program(tmp_path, sanitized_lib.build(tmp_path), "flight_adjoint_sanitize")

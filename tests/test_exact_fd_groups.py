"""The rest of the default forward-difference Jacobian, and the residuals, against EXACT quotients (tests/golden/
g21_exact_fd_groups.npz: the reference's formulas in 40-digit arithmetic on the fp64 inputs its sweeps form,
tests/golden/make_exact_fd_groups.py).  test_exact_fd.py does this for the velocity group of the aerodynamic phases; here:

  * the velocity group of every phase without aerodynamics (mass, position and quaternion sweeps, t columns);
  * the quaternion group of the free-attitude phases (quat/quaternion, quat/u, quat/t);
  * the residuals of all four defect groups.

Each form is held to its own derived bound (tests/fd_noise.py; ~1e-8 of an entry where test_gpu_parity allows 1e-5 + 1e-6 |ref|):
the engine's closed forms (flags 0) to a few roundings of the entry (quaternion group: plus the |rho - 1| of the step the reference
really takes), the recomputing form (flag 8) and the oracle to the chain bound of two runs differenced.

CPU part: the oracle, the bounds' non-vacuity and their added power over the flat tolerance.  GPU part (-m gpu): the engine
through eval_jacobian (gather map), eval (COO-direct one-vector form) and eval_batch (truth rows inside batches of distinct
vectors, partly filled workgroups), flags 0 and 8; residuals also under the D.X path flags 1, 2 and 4."""
import numpy as np
import pytest

import exact_fd_groups_truth as T

NAMES = list(T.STATES)
# batch sizes that leave workgroups partly filled
BATCH = {"3x32": (9, 33), "mixed-6x64": (47,), "stress-12x128": (37,)}


def _oracle_items(name):
    import oracle
    G, prob, x, P, D = T.setup(name)
    J = {g: P.jacobian(g, x) for g in ("vel", "quat")}
    R = {g: P.residual(g, x) for g in oracle.GROUPS}
    return T.checks(J, G, name, prob, x, D, "recompute"), T.residual_checks(R, G, name, prob, x, D), (G, prob, x, P, D, J)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_within_the_recomputing_bound_of_the_exact_quotients(name):
    """the oracle runs the reference's sweeps: every NoAir velocity-group and quaternion-group entry within the chain bound, every
    residual row within the residual bound -- validates the exact evaluation, the oracle and the bounds at once"""
    jac, res, _ = _oracle_items(name)
    w = T.ratios(jac + res)
    bad = {k: v for k, v in w.items() if v > 1.0}
    assert not bad, (name, bad)


def test_the_rounding_driven_bounds_are_not_vacuous():
    """somewhere the oracle uses more than 5 % of each rounding-driven bound: the NoAir chain bound (its position, mass and
    quaternion sweeps), the quaternion group's chain bound (quaternion and u sweeps), its t columns' bound, the residual bound of
    every group"""
    use = {}
    for name in NAMES:
        jac, res, _ = _oracle_items(name)
        for k, v in T.ratios(jac + res).items():
            fam = {"NoAir vel/position": "noair chain", "NoAir vel/mass": "noair chain", "NoAir vel/quaternion": "noair chain",
                   "quat/quaternion": "quat chain", "quat/u": "quat chain", "quat/t": "quat t",
                   "res/vel aero": None, "NoAir vel/t": None}.get(k, k)
            if fam is not None:
                use[fam] = max(use.get(fam, 0.0), v)
    assert set(use) == {"noair chain", "quat chain", "quat t", "res/mass", "res/pos", "res/vel NoAir", "res/quat"}, use
    assert all(v > 0.05 for v in use.values()), use


def test_the_new_bounds_are_tighter_than_the_flat_tolerance():
    """added power: per block, the engine's default-form bound is at most 1e-2 of the flat 1e-5 + 1e-6 |exact| that
    test_gpu_parity holds these entries to, on at least 99 % of them.  Not NoAir vel/position: every form recomputes gravity
    there, and the chain bound of two runs differenced (C_CHAIN eps |g| S / dx) is 0.3 of the flat tolerance at the median entry
    and exceeds it on long phases -- the rounding noise of any fp64 forward difference of gravity, which no tolerance can undercut;
    test_gpu_parity's flat check still holds those entries"""
    frac = {}
    for name in NAMES:
        G, prob, x, P, D = T.setup(name)
        J = {g: P.jacobian(g, x) for g in ("vel", "quat")}
        for label, got, exact, b in T.checks(J, G, name, prob, x, D, "closed"):
            ok = np.asarray(b) <= 1e-2 * (1e-5 + 1e-6 * np.abs(exact))
            n0, n1 = frac.get(label, (0, 0))
            frac[label] = (n0 + int(ok.sum()), n1 + ok.size)
    assert len(frac) == 7, frac
    del frac["NoAir vel/position"]
    low = {k: a / b for k, (a, b) in frac.items() if a < 0.99 * b}
    assert not low, low


# ------------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------------
def _engine(prob, D, flags):
    import oracle
    from gelato_amd import Engine
    return Engine(prob, D=D, tau=prob["tau"], barC20=oracle.BARC20_CPP, flags=flags)


def _check(items, what):
    w = T.ratios(items)
    bad = {k: v for k, v in w.items() if v > 1.0}
    assert not bad, (what, bad)
    return w


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, 8])
@pytest.mark.parametrize("name", NAMES)
def test_engine_within_its_bound_through_every_output_path(name, flags):
    """flags 0: the closed forms; flags 8: the reference's sweeps.  eval_jacobian (compact kernel output through the gather map),
    eval (COO-direct), eval_batch with the truth state at the first, a middle and the last position of a batch of distinct
    vectors: every checked entry and residual row within its bound, and the batch rows bit-identical to the one-vector call"""
    from gelato_amd import problem
    G, prob, x, P, D = T.setup(name)
    form = "closed" if flags == 0 else "recompute"
    E = _engine(prob, D, flags)
    try:
        vals, rc = E.eval_jacobian(x)
        assert rc == 0
        J = E.jac_dicts(vals)
        lay = T.Layout(J, prob)
        _check(T.checks(J, G, name, prob, x, D, form, lay), "%s flags %d eval_jacobian" % (name, flags))
        res, vals1, rc = E.eval(x)
        assert rc == 0
        _check(T.checks(E.jac_dicts(vals1), G, name, prob, x, D, form, lay), "%s flags %d eval (COO-direct)" % (name, flags))
        _check(T.residual_checks(E.split_res(res), G, name, prob, x, D), "%s flags %d eval residuals" % (name, flags))
        for B in BATCH.get(name, (9,)):
            X = problem.synthetic_batch(x, E.M, B)
            pos = (0, B // 2, B - 1)
            for b in pos:
                X[b] = x
            assert len({X[b].tobytes() for b in range(B)}) == B - 2      # the others distinct
            rb, jb, rc = E.eval_batch(X)
            assert rc == 0
            for b in pos:
                full = E.expand(jb[b])
                _check(T.checks(E.jac_dicts(full), G, name, prob, x, D, form, lay), "%s flags %d batch %d row %d" % (name, flags, B, b))
                _check(T.residual_checks(E.split_res(rb[b]), G, name, prob, x, D), "%s flags %d batch %d row %d residuals" % (name, flags, B, b))
                assert np.array_equal(full, vals), (name, flags, B, b, "batch row differs from eval_jacobian")
                assert np.array_equal(rb[b], res), (name, flags, B, b, "batch residual row differs from eval")
    finally:
        E.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,flags", [(n, f) for n in NAMES for f in (1, 2)] + [("3x32", 4)])
def test_engine_residuals_within_the_bound_on_every_dx_path(name, flags):
    """GEL_FLAG_DX_MFMA (1), GEL_FLAG_DX_VALU (2) force the D.X path; GEL_FLAG_NO_PACK (4) the one-vector-per-wavefront form
    (only 3x32 packs two vectors per wavefront)"""
    G, prob, x, P, D = T.setup(name)
    E = _engine(prob, D, flags)
    try:
        res, rc = E.eval_residual(x)
        assert rc == 0
        _check(T.residual_checks(E.split_res(res), G, name, prob, x, D), "%s flags %d residuals" % (name, flags))
        B = BATCH.get(name, (9,))[0]
        from gelato_amd import problem
        X = problem.synthetic_batch(x, E.M, B)
        X[B - 1] = x
        rb, _, rc = E.eval_batch(X, want_jac=False)
        assert rc == 0
        _check(T.residual_checks(E.split_res(rb[B - 1]), G, name, prob, x, D), "%s flags %d batch residuals" % (name, flags))
    finally:
        E.close()

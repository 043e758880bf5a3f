"""CPU: GEL_FLAG_EXACT_AERO_JAC on host-only handles (device = GEL_DEVICE_NONE), the pdict key that selects it, and a cross-check of
the 60-digit ground truth (tests/golden/g20_exact_aero_jac.npz) against the 40-digit forward-difference quotients of G18.

The exact aero gradients fill the default layout, so the flag leaves the aero dims, pattern, record layout and record map exactly
as they are without it; it cannot be combined with GEL_FLAG_FD_RECOMPUTE (whose t columns are laid out differently)."""
import numpy as np
import pytest

import exact_aero_truth as T
from conftest import load_golden

from gelato_amd import Engine, _lib

AERO = _lib.GEL_FLAG_EXACT_AERO_JAC


def _configured(prob, D, tau, specs, flags):
    E = Engine(prob, D=D, tau=tau, device=-1, flags=flags)
    for kind in T.KINDS:
        E.aero_configure(kind, specs[kind])
    return E


def test_flag_value():
    assert AERO == 64 and AERO & _lib.GEL_FLAG_EXACT_DEFECT_JAC == 0


@pytest.mark.parametrize("name", ["g9_synthetic", "ragged", "mixed-6x64"])
@pytest.mark.parametrize("flags", [AERO, AERO | _lib.GEL_FLAG_EXACT_DEFECT_JAC])
def test_exact_aero_flag_keeps_the_default_layout(name, flags):
    prob, D, x, specs = T.case(name)
    E0 = _configured(prob, D, prob["tau"], specs, 0)
    E1 = _configured(prob, D, prob["tau"], specs, flags)
    for kind in T.KINDS:
        assert E0.aero_dims(kind) == E1.aero_dims(kind)
        for (r0, c0), (r1, c1) in zip(E0.aero_pattern(kind), E1.aero_pattern(kind)):
            assert np.array_equal(r0, r1) and np.array_equal(c0, c1)
    w0, con0, jac0 = E0.aero_record_layout()
    w1, con1, jac1 = E1.aero_record_layout()
    assert w0 == w1
    for kind in T.KINDS:
        assert np.array_equal(con0[kind], con1[kind]) and np.array_equal(jac0[kind], jac1[kind])


def test_exact_aero_flag_with_fd_recompute_is_rejected():
    prob, D, x, specs = T.case("ragged")
    with pytest.raises(_lib.GelatoAmdError, match="EXACT_AERO_JAC"):
        Engine(prob, device=-1, flags=AERO | _lib.GEL_FLAG_FD_RECOMPUTE)
    with pytest.raises(_lib.GelatoAmdError, match="FD_RECOMPUTE"):
        Engine(prob, device=-1, flags=AERO | _lib.GEL_FLAG_EXACT_DEFECT_JAC | _lib.GEL_FLAG_FD_RECOMPUTE)
    Engine(prob, device=-1, flags=AERO)                                  # alone, and with the exact defect Jacobian
    Engine(prob, device=-1, flags=AERO | _lib.GEL_FLAG_EXACT_DEFECT_JAC)


def test_pdict_aero_jacobian_selects_the_flag():
    from gelato_amd import con_dynamics
    assert con_dynamics._aero_jacobian_flags({}) == 0
    assert con_dynamics._aero_jacobian_flags({"aero_jacobian": "fd"}) == 0
    assert con_dynamics._aero_jacobian_flags({"aero_jacobian": "exact"}) == AERO
    assert con_dynamics._aero_jacobian_flags({"defect_jacobian": "exact"}) == 0      # the two keys are independent
    with pytest.raises(ValueError):
        con_dynamics._aero_jacobian_flags({"aero_jacobian": "analytic"})


# G18 rows whose forward-difference quotient is not within O(dx) of the derivative, per case: the synthetic G9 set's rows where the
# air-relative speed vanishes within the step (clamped), and layer-break nodes whose position step crosses a layer or table break
FD_FAR = {("g9_synthetic", "a"): 5, ("g9_synthetic", "q"): 1, ("breaks", "a"): 21, ("breaks", "q"): 36}


@pytest.mark.parametrize("name", ["g9_example", "g9_synthetic", "ragged", "polar", "layers", "breaks"])
def test_truth_agrees_with_the_exact_forward_difference_quotients(name):
    """(f(x + dx e_k) - f(x)) / dx = f' + O(dx f''): with dx = 1e-8 (normalised) every entry is within 1e-4 of its row's largest
    derivative, except the rows counted in FD_FAR (only position columns where a break is crossed)."""
    G, F = load_golden("g20_exact_aero_jac.npz"), load_golden("g18_aero_exact_fd.npz")
    prob, D, x, specs = T.case(name)
    assert np.array_equal(F[name + "_x"], G[name + "_x"])
    nn = [int(v) for v in prob["num_nodes"]]
    where = {(int(p), int(k)): i for i, (p, k) in enumerate(G[name + "_nodes"])}
    idx = [where[(int(ph), k)] for ph, al in F[name + "_nodes"] for k in range(nn[ph] + 1 if al else 1)]
    for s, key in (("a", "d_alpha"), ("q", "d_q")):
        tr, fd = G["%s_d%s_c" % (name, s)][idx], F["%s_%s" % (name, key)][:, :10]
        assert np.all(np.isfinite(tr))
        with np.errstate(invalid="ignore", over="ignore"):
            far = ~(np.abs(fd - tr) <= 1e-4 * np.abs(tr).max(axis=1, keepdims=True) + 1e-12)
        assert int(far.any(axis=1).sum()) == FD_FAR.get((name, s), 0), (name, s, int(far.any(axis=1).sum()))
        if name == "breaks":
            assert not far[:, 3:].any()
        assert not G["%s_kink_%s" % (name, s)][idx].any() or name == "g9_synthetic"

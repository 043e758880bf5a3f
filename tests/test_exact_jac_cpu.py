"""CPU: GEL_FLAG_EXACT_DEFECT_JAC on a host-only handle (device = GEL_DEVICE_NONE).  The exact Jacobian fills the default compact
layout, so the flag leaves dims, pattern, constants, compact index and gather map exactly as they are without it; it cannot be
combined with GEL_FLAG_FD_RECOMPUTE (whose layout differs), and the handle says so at creation."""
import numpy as np
import pytest

from conftest import D_tau_from_golden, load_golden, problem_from_golden

from gelato_amd import Engine, _lib


@pytest.mark.parametrize("name", ["example", "mixed6x64", "negarea"])
def test_exact_flag_keeps_the_default_layout(name):
    g = load_golden("g6_%s.npz" % name)
    prob = problem_from_golden(g)
    D, tau = D_tau_from_golden(g, prob)
    E0 = Engine(prob, D=D, tau=tau, device=-1)
    E1 = Engine(prob, D=D, tau=tau, device=-1, flags=_lib.GEL_FLAG_EXACT_DEFECT_JAC)
    assert (E1.N, E1.M, E1.nvars, E1.V, E1.total_nnz) == (E0.N, E0.M, E0.nvars, E0.V, E0.total_nnz)
    assert E1.block_nnz == E0.block_nnz and E1.block_shape == E0.block_shape
    for (r0, c0), (r1, c1) in zip(E0.pattern(), E1.pattern()):
        assert np.array_equal(r0, r1) and np.array_equal(c0, c1)
    assert np.array_equal(E0.const_values().view(np.int64), E1.const_values().view(np.int64))
    assert np.array_equal(E0.var_index(), E1.var_index())
    assert np.array_equal(E0.full_source(), E1.full_source())


def test_exact_flag_with_fd_recompute_is_rejected():
    g = load_golden("g6_3x32.npz")
    prob = problem_from_golden(g)
    with pytest.raises(_lib.GelatoAmdError, match="EXACT_DEFECT_JAC"):
        Engine(prob, device=-1, flags=_lib.GEL_FLAG_EXACT_DEFECT_JAC | _lib.GEL_FLAG_FD_RECOMPUTE)
    Engine(prob, device=-1, flags=_lib.GEL_FLAG_FD_RECOMPUTE)          # either flag alone is fine
    Engine(prob, device=-1, flags=_lib.GEL_FLAG_EXACT_DEFECT_JAC)


def test_pdict_defect_jacobian_selects_the_flag():
    from gelato_amd import con_dynamics
    assert con_dynamics._defect_jacobian_flags({}) == 0
    assert con_dynamics._defect_jacobian_flags({"defect_jacobian": "fd"}) == 0
    assert con_dynamics._defect_jacobian_flags({"defect_jacobian": "exact"}) == _lib.GEL_FLAG_EXACT_DEFECT_JAC
    with pytest.raises(ValueError):
        con_dynamics._defect_jacobian_flags({"defect_jacobian": "analytic"})

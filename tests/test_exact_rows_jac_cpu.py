"""CPU: GEL_FLAG_EXACT_ROWS_JAC on host-only handles (device = GEL_DEVICE_NONE), the pdict key that selects it, and the shape of the
60-digit ground truth (tests/golden/g22_exact_rows_jac.npz).

The jfn layout [B][nfn][7] does not depend on any flag, so the flag combines with every other one, GEL_FLAG_FD_RECOMPUTE included;
the exact defect and aero Jacobians keep rejecting that combination."""
import numpy as np
import pytest

import exact_rows_truth as T
from conftest import load_golden

from gelato_amd import _lib

ROWS = _lib.GEL_FLAG_EXACT_ROWS_JAC


def test_flag_value():
    assert ROWS == 128
    for other in (_lib.GEL_FLAG_FD_RECOMPUTE, _lib.GEL_FLAG_EXACT_DEFECT_JAC, _lib.GEL_FLAG_EXACT_AERO_JAC, 1, 2, 4, 16):
        assert ROWS & other == 0


def test_pdict_rows_jacobian_selects_the_flag():
    from gelato_amd import con_dynamics
    assert con_dynamics._rows_jacobian_flags({}) == 0
    assert con_dynamics._rows_jacobian_flags({"rows_jacobian": "fd"}) == 0
    assert con_dynamics._rows_jacobian_flags({"rows_jacobian": "exact"}) == ROWS
    # the three keys are independent
    assert con_dynamics._rows_jacobian_flags({"defect_jacobian": "exact", "aero_jacobian": "exact"}) == 0
    assert con_dynamics._defect_jacobian_flags({"rows_jacobian": "exact"}) == 0
    assert con_dynamics._aero_jacobian_flags({"rows_jacobian": "exact"}) == 0
    with pytest.raises(ValueError):
        con_dynamics._rows_jacobian_flags({"rows_jacobian": "analytic"})


def test_pdict_key_reaches_the_shared_handle():
    from gelato_amd import con_dynamics, problem
    pdict, unitdict, _, _ = problem.make_problem("example")
    pdict["device"] = -1
    pdict["rows_jacobian"] = "exact"
    pdict["aero_jacobian"] = "exact"
    assert con_dynamics.engine_of(pdict, unitdict).flags == ROWS | _lib.GEL_FLAG_EXACT_AERO_JAC


def test_host_only_handles_accept_the_flag_with_every_other():
    FD8, DEF, AERO = _lib.GEL_FLAG_FD_RECOMPUTE, _lib.GEL_FLAG_EXACT_DEFECT_JAC, _lib.GEL_FLAG_EXACT_AERO_JAC
    G = load_golden("g22_exact_rows_jac.npz")
    for flags in (ROWS, ROWS | FD8, ROWS | DEF | AERO, ROWS | DEF, ROWS | AERO):
        E = T.example_engine(flags, device=-1)
        E.rows_configure([], T.table(G, "synthetic"))
        assert E.flags == flags
    for flags in (DEF | FD8, AERO | FD8, ROWS | DEF | FD8, ROWS | AERO | FD8):   # as without the flag: still rejected
        with pytest.raises(_lib.GelatoAmdError, match="FD_RECOMPUTE"):
            T.example_engine(flags, device=-1)


def test_ground_truth_fixture_covers_every_function_mode_and_corner():
    G = load_golden("g22_exact_rows_jac.npz")
    for name in T.CASES:
        R = len(G[name + "_fn"])
        B = G[name + "_x"].shape[0]
        for k in ("Tc", "Tf", "Tb", "kink", "conv"):
            assert G[name + "_" + k].shape == (B, R, 7), (name, k)
        assert np.all(np.isfinite(G[name + "_Tc"][~G[name + "_conv"]]))
    fn, mode, tcol = G["synthetic_fn"], G["synthetic_mode"], G["synthetic_tcol"]
    assert set(fn.tolist()) == set(range(16))
    for bit in (1, 4, 8):
        assert (mode & bit).any() and (~mode & bit).any()
    assert np.all(tcol[fn >= 9] >= 0)                         # functions of the knot time always name one
    for f in range(9):
        assert (tcol[fn == f] >= 0).any() and (tcol[fn == f] < 0).any()
    assert G["corners_conv"].any()
    # the default and exact tables are the same rows: the IIP rows without an impact point are all zero in the truth
    iip = (G["synthetic_fn"] >= 12) & (G["synthetic_fn"] <= 13)
    assert (np.abs(G["synthetic_Tc"][:, iip]).sum(axis=2) == 0).any()

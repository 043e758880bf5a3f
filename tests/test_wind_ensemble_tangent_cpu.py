"""The tangent and the adjoint flight under a wind ensemble, host side (no GPU; host-only handles): the four entry
points gel_propagate_tangent_ensemble*, gel_propagate_adjoint_ensemble* are in the header and bound, every refusal is decided before
a buffer or the device is looked at -- every buffer passed here is a poisoned non-NULL address -- and carries its reason, and the two
*_info calls are what they were: the ensemble adds no per-lane workspace."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import interp_truth as it
import sanitized_lib
from test_wind_ensemble_cpu import members

NAMES = ("gel_propagate_tangent_ensemble", "gel_propagate_tangent_ensemble_device", "gel_propagate_adjoint_ensemble",
         "gel_propagate_adjoint_ensemble_device")
GEL_ERR_ARG = -1         # include/gelato_amd.h
POISON = 0xDEAD0000          # never dereferenced: a refusal that looked at a buffer would fault here
NUM_NODES = [2, 3, 16, 4]


def _dp(addr):
    return C.cast(C.c_void_p(addr), C.POINTER(C.c_double))


def _tangent(L, form, plan, B, P, shared, ens, dx=POISON, ddisp=POISON):
    """a raw call with poisoned buffers -> (return code, message)"""
    if form == "host":
        rc = L.gel_propagate_tangent_ensemble(plan, B, P, shared, _dp(POISON), _dp(POISON), _dp(dx) if dx else None,
                                              _dp(ddisp) if ddisp else None, ens, _dp(POISON), _dp(POISON))
    else:
        rc = L.gel_propagate_tangent_ensemble_device(plan, B, P, shared, POISON, POISON, dx or None, ddisp or None, ens, POISON, POISON)
    return rc, (L.gel_last_error() or b"").decode()


def _adjoint(L, form, plan, B, Q, shared, ens, lam=POISON):
    if form == "host":
        rc = L.gel_propagate_adjoint_ensemble(plan, B, Q, shared, _dp(POISON), _dp(POISON), _dp(lam) if lam else None, ens, _dp(POISON),
                                              _dp(POISON), _dp(POISON))
    else:
        rc = L.gel_propagate_adjoint_ensemble_device(plan, B, Q, shared, POISON, POISON, lam or None, ens, POISON, POISON, POISON)
    return rc, (L.gel_last_error() or b"").decode()


def test_prototypes_in_the_header_and_bound():
    from gelato_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "gelato_amd.h")).read()
    L = _lib.lib()
    for n in NAMES:
        m = re.search(r"^int %s\(([^;]*)\);" % n, text, re.M)
        assert m, n
        args = m.group(1)
        assert "gel_wind_ensemble* ens" in args and "stream" not in args, n        # no caller-stream argument
        fn = getattr(L, n)
        assert fn.restype is C.c_int and len(fn.argtypes) == 11, n
    assert "out of scope" not in text[text.index("tangent-linear propagation"):text.index("one optimiser callback")]
    # the ensemble's place in the argument list: behind the seeds / lam, before the outputs
    assert re.search(r"gel_propagate_tangent_ensemble\([^;]*ddisp[^;]*ens[^;]*\by,", text)
    assert re.search(r"gel_propagate_adjoint_ensemble\([^;]*lam[^;]*ens[^;]*\by,", text)


def test_refusals_on_a_host_only_handle_touch_no_buffer():
    from gelato_amd import _lib
    L = _lib.lib()
    E, other = it.engine(it.prob_of(NUM_NODES)), it.engine(it.prob_of(NUM_NODES))
    B = 5
    ens = E.wind_ensemble(members(33, (1, 2, 3))).assign([0, -1, 2, 1, 0])
    short = E.wind_ensemble(members(33, (1, 2, 3))).assign([0, -1, 2, 1])          # B - 1 vectors
    foreign = other.wind_ensemble(members(33, (1, 2, 3))).assign([0, -1, 2, 1, 0])
    unassigned = E.wind_ensemble(members(2, (1,)))
    chain, section, node = (E.propagation_plan(steps=1, restart=r) for r in ("chain", "section", "node"))
    for form in ("host", "device"):
        suffix = "_ensemble" + ("_device" if form == "device" else "")
        for plan in (chain, section, node):
            # an ensemble created and assigned, everything else in order: the host-only handle is what is refused, as in the parent
            rc, msg = _tangent(L, form, plan._p, B, 3, 1, ens._p)
            assert rc == GEL_ERR_ARG and "gel_propagate_tangent" + suffix in msg and "host-only" in msg, msg
            rc, msg = _tangent(L, form, plan._p, B, 3, 1, None)                    # ens == NULL: the parent's refusal
            assert rc == GEL_ERR_ARG and "host-only" in msg, msg
            # the ensemble's rules come before the handle is looked at
            rc, msg = _tangent(L, form, plan._p, B, 3, 0, short._p)
            assert rc == GEL_ERR_ARG and "assigned 4 vectors, the call has B = 5" in msg, msg
            rc, msg = _tangent(L, form, plan._p, B, 3, 0, foreign._p)
            assert rc == GEL_ERR_ARG and "another handle" in msg, msg
            rc, msg = _tangent(L, form, plan._p, B, 3, 0, unassigned._p)
            assert rc == GEL_ERR_ARG and "no vectors yet" in msg, msg
            # the parent's own rules come before the ensemble's
            rc, msg = _tangent(L, form, plan._p, B, 0, 1, short._p)
            assert rc == GEL_ERR_ARG and "P < 1" in msg, msg
            rc, msg = _tangent(L, form, plan._p, B, 3, 1, short._p, dx=0, ddisp=0)
            assert rc == GEL_ERR_ARG and "both seeds" in msg, msg
            rc, msg = _tangent(L, form, plan._p, B, 3, 2, short._p)
            assert rc == GEL_ERR_ARG and "shared is neither 0 nor 1" in msg, msg
            # B = 0 with an ensemble of no vectors: nothing to refuse but the handle
            empty = E.wind_ensemble(members(2, (1,))).assign([])
            rc, msg = _tangent(L, form, plan._p, 0, 3, 1, empty._p)
            assert rc == GEL_ERR_ARG and "host-only" in msg, msg
            empty.close()
        for plan in (chain, section):
            rc, msg = _adjoint(L, form, plan._p, B, 2, 1, ens._p)
            assert rc == GEL_ERR_ARG and "gel_propagate_adjoint" + suffix in msg and "host-only" in msg, msg
            rc, msg = _adjoint(L, form, plan._p, B, 2, 1, None)
            assert rc == GEL_ERR_ARG and "host-only" in msg, msg
            rc, msg = _adjoint(L, form, plan._p, B, 2, 0, short._p)
            assert rc == GEL_ERR_ARG and "assigned 4 vectors, the call has B = 5" in msg, msg
            rc, msg = _adjoint(L, form, plan._p, B, 2, 0, foreign._p)
            assert rc == GEL_ERR_ARG and "another handle" in msg, msg
            rc, msg = _adjoint(L, form, plan._p, B, 0, 1, short._p)
            assert rc == GEL_ERR_ARG and "Q < 1" in msg, msg
            rc, msg = _adjoint(L, form, plan._p, B, 2, 1, short._p, lam=0)
            assert rc == GEL_ERR_ARG and "lam is NULL" in msg, msg
        # a node-restart plan has no adjoint flight, with or without an ensemble, whatever the ensemble is assigned
        for e in (ens, short, None):
            rc, msg = _adjoint(L, form, node._p, B, 2, 1, e._p if e else None)
            assert rc == GEL_ERR_ARG and "GEL_PROP_RESTART_NODE" in msg, msg
    # the Python layer: another engine's ensemble is refused by name, anything else by type
    X = np.zeros((B, E.nvars))
    dX, lam = np.ones((3, E.nvars)), np.ones((2, 11 * E.M))
    oplan = other.propagation_plan(steps=1, restart="chain")
    with pytest.raises(ValueError, match="another engine"):
        oplan.tangent(X, dX=dX, shared=True, ensemble=ens)
    with pytest.raises(ValueError, match="another engine"):
        oplan.adjoint(X, lam, shared=True, ensemble=ens)
    with pytest.raises(ValueError, match="another engine"):
        oplan.tangent_device(B, 3, POISON, POISON, POISON, d_dx=POISON, ensemble=ens)
    with pytest.raises(ValueError, match="another engine"):
        oplan.adjoint_device(B, 2, POISON, POISON, POISON, POISON, ensemble=ens)
    with pytest.raises(TypeError, match="WindEnsemble"):
        chain.tangent(X, dX=dX, shared=True, ensemble=members(33, (1,)))
    with pytest.raises(_lib.GelatoAmdError, match="assigned 4 vectors, the call has B = 5"):
        chain.tangent(X, dX=dX, shared=True, ensemble=short)
    with pytest.raises(_lib.GelatoAmdError, match="assigned 4 vectors, the call has B = 5"):
        chain.adjoint(X, lam, shared=True, ensemble=short)
    with pytest.raises(_lib.GelatoAmdError, match="host-only"):
        chain.tangent(X, dX=dX, shared=True, ensemble=ens)
    with pytest.raises(_lib.GelatoAmdError, match="host-only"):
        chain.adjoint(X, lam, shared=True, ensemble=ens)
    for o in (oplan, chain, section, node, ens, short, foreign, unassigned):
        o.close()
    other.close()


def test_info_calls_are_what_they_were():
    """the figures restated from the plan's own numbers, before and after an ensemble exists"""
    E = it.engine(it.prob_of(NUM_NODES))
    hold = [bool(h) for h in E.prob["attitude_hold"]]
    for k in (1, 3):
        plan = E.propagation_plan(steps=k, restart="chain")
        pts = sum(2 * k * n + 1 for n, h in zip(NUM_NODES, hold) if not h)
        before = [plan.tangent_info(67, 3), plan.tangent_info(67, 3, shared=True), plan.adjoint_info(67, 2), plan.adjoint_info(67, 2, shared=True)]
        assert before[0]["sample_set_bytes"] == before[1]["sample_set_bytes"] == 16 * pts
        assert before[2]["lane_bytes"] == before[3]["lane_bytes"] == 16 * pts + 8 * E.S + 88 * (k - 1)
        for info, lanes in zip(before, (3, 3, 2, 2)):
            per = info["lanes_per_slab"] // lanes
            assert info["lanes_per_slab"] % (64 * lanes) == 0 and info["slabs"] == -(-67 // per), info
        ens = E.wind_ensemble(members(160, (1, 2, 3, 4))).assign(np.arange(67) % 4)
        after = [plan.tangent_info(67, 3), plan.tangent_info(67, 3, shared=True), plan.adjoint_info(67, 2), plan.adjoint_info(67, 2, shared=True)]
        assert after == before
        ens.close()
        plan.close()


@sanitized_lib.needs_toolchain
def test_entry_points_under_asan_ubsan(tmp_path):
    """every refusal of the four calls on host-only handles, with buffers of ONE double, in a stand-alone program
    (tests/ensemble_tangent_sanitize.c) under AddressSanitizer + UBSan + LeakSanitizer, linked against the sanitized library directly;
    nothing is preloaded and nothing is launched"""
    sanitized_lib.run_program(tmp_path, sanitized_lib.build(tmp_path), "ensemble_tangent_sanitize")

"""Chained flight and dispersions, host side (no GPU; host-only handles): the chain plan's flag, its refusals and
gel_prop_plan_info, the Python argument checks, sample_dispersion, the restatement of tests/flight_truth.py against
propagate_truth's bits (the chain's phase 0; the node restart as a whole), the teeth of its three wrong restatements, and the plan builder under AddressSanitizer + UBSan in a
stand-alone program."""
import numpy as np
import pytest

import flight_truth as ft
import interp_truth as it
import mesh_truth as mt
import propagate_truth as pt
import sanitized_lib


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


NODES = [2, 3, 16, 64]
STEPS = [1, 3, 4, 2]


def test_chain_plan_flag_and_info():
    from gelato_amd import _lib
    assert _lib.GEL_PROP_CHAIN == 2 and _lib.GEL_PROP_NDISP == 4
    E = it.engine(it.prob_of(NODES))
    plan = E.propagation_plan(steps=STEPS, restart="chain")
    info = plan.info()
    assert info["S"] == 4 and info["flags"] == 2
    assert info["lane_steps"] == sum(k * n for n, k in zip(NODES, STEPS))
    sec = E.propagation_plan(steps=STEPS)
    si = sec.info()
    assert si["flags"] == 0 and si["lane_steps"] == max(k * n for n, k in zip(NODES, STEPS))
    for key in ("stage_points", "workspace_bytes_per_vector", "slab"):
        assert info[key] == si[key], key
    for s in range(4):   # the same tables in every mode
        a, b = plan.matrices(s), sec.matrices(s)
        assert all(np.array_equal(_bits(a[key]), _bits(b[key])) for key in ("pts", "Wu")) and np.array_equal(a["copy_u"], b["copy_u"])
    # both mode flags at once, and an unknown flag, are refused
    import ctypes as C
    st = np.ones(4, dtype=np.int32)
    for flags in (2 | 1, 4, 2 | 4):
        h = C.c_void_p()
        rc = _lib.lib().gel_prop_plan_create(E._h, st.ctypes.data_as(C.POINTER(C.c_int32)), flags, C.byref(h))
        assert rc < 0 and not h.value, flags
    plan.close()
    sec.close()


def test_chain_refusal_at_two_to_the_twenty():
    """sum_s steps[s] n_s is one lane's run length: 2^20 is the last plan created, one more is refused; each phase alone is
    below the per-section cap, which the other modes keep"""
    from gelato_amd import _lib
    E = it.engine(it.prob_of([4, 4]))
    half = 2 ** 17                                   # 4 * 2^17 = 2^19 steps per phase
    ok = E.propagation_plan(steps=[half, half], restart="chain")
    assert ok.info()["lane_steps"] == 2 ** 20
    ok.close()
    with pytest.raises(_lib.GelatoAmdError, match="sum"):
        E.propagation_plan(steps=[half, half + 1], restart="chain")     # 2^20 + 4
    E3 = it.engine(it.prob_of([4, 3, 2]))
    third = (2 ** 18 - 1) // 3                       # 4 * 2^17 + 3 * third + 2 * 2^17 = 2^19 + (2^18 - 1) + 2^18 = 2^20 - 1
    one_below = E3.propagation_plan(steps=[half, third, half], restart="chain")
    assert one_below.info()["lane_steps"] == 2 ** 20 - 1
    one_below.close()
    with pytest.raises(_lib.GelatoAmdError, match="sum"):
        E3.propagation_plan(steps=[half, third, half + 1], restart="chain")         # 2^20 + 1
    sec = E.propagation_plan(steps=[half, half + 1])                                # section mode: each phase on its own
    assert sec.info()["lane_steps"] == 4 * (half + 1)
    sec.close()
    # a chain plan on a host-only handle does not evaluate: no CPU fallback
    plan = E.propagation_plan(steps=1, restart="chain")
    with pytest.raises(_lib.GelatoAmdError):
        plan.apply(it.random_x(E))
    with pytest.raises(_lib.GelatoAmdError):
        plan.apply_device(1, 0, 0, 0, 0)


def test_python_argument_checks():
    from gelato_amd import propagate
    E = it.engine(it.prob_of([3, 4]))
    for name in ("section", "node", "chain"):
        E.propagation_plan(steps=1, restart=name).close()
    for bad in ("phase", "flight", None, 2):
        with pytest.raises(ValueError):
            E.propagation_plan(restart=bad)
    plan = E.propagation_plan(steps=1, restart="chain")
    X = np.stack([it.random_x(E, 0), it.random_x(E, 1)])
    for shape in ((2, 2, 3), (1, 2, 4), (2, 4), (2, 3, 4), (16,)):
        with pytest.raises(ValueError):
            plan.apply(X, dispersion=np.ones(shape))
    with pytest.raises(ValueError):
        plan.apply(X[0], dispersion=np.ones((2, 2, 4)))
    for dtype in (np.float32, np.int64):
        with pytest.raises(TypeError):
            plan.apply(X, dispersion=np.ones((2, 2, 4), dtype=dtype))
    with pytest.raises(ValueError):
        propagate.fly(X, None, None, steps=0, engine=E)
    with pytest.raises(ValueError):
        propagate.sample_dispersion(3, 2, 0.1, 0, per="node")
    with pytest.raises(ValueError):
        propagate.sample_dispersion(3, 2, [0.1, 0.2], 0)
    with pytest.raises(ValueError):
        propagate.sample_dispersion(3, 2, -0.1, 0)


def test_sample_dispersion():
    from gelato_amd import propagate
    a = propagate.sample_dispersion(5, 3, 0.02, seed=7)
    assert a.shape == (5, 3, 4) and a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    assert np.array_equal(_bits(a), _bits(propagate.sample_dispersion(5, 3, 0.02, seed=7)))
    assert not np.array_equal(a, propagate.sample_dispersion(5, 3, 0.02, seed=8))
    assert np.all(a == a[:, :1, :])                                    # per vector: the same factors in all its phases
    assert len(np.unique(a[:, 0, :])) == 20                            # one draw per (vector, factor)
    p = propagate.sample_dispersion(5, 3, 0.02, seed=7, per="phase")
    assert p.shape == (5, 3, 4) and len(np.unique(p)) == 60
    assert np.array_equal(_bits(propagate.sample_dispersion(4, 2, 0.0, seed=1)), _bits(np.ones((4, 2, 4))))
    sg = np.array([0.1, 0.0, 0.01, 0.5])
    m = propagate.sample_dispersion(2000, 1, sg, seed=3)
    assert np.all(m[:, :, 1] == 1.0)
    assert np.all(np.abs(m.std(axis=0)[0] - sg) <= 0.1 * sg) and np.all(np.abs(m.mean(axis=0)[0] - 1.0) <= 0.1 * sg + 1e-15)
    assert propagate.sample_dispersion(0, 3, 0.1, seed=0).shape == (0, 3, 4)


_EX = {}


def example():
    """(prob, host-only engine, X [3, nvars]) of the shipped example: x0 itself (every knot continuous), x0 with the mass
    jettisoned at the stage knots (SEP1, FAIRING, SEP2: the collocated mass drops there and stays lower), and a perturbed vector
    whose every component jumps a little at every knot"""
    if not _EX:
        from gelato_amd import problem
        prob, x0 = it.named("example")
        E = it.engine(prob)
        _EX["v"] = (prob, E, ft.flight_batch(x0, E))
    return _EX["v"]


def test_truth_phase0_and_continuous_knots():
    """the chain restatement: phase 0 is propagate_phase's, bit for bit (y and bound); across a continuous knot the start of
    s + 1 is the end of s, bit for bit; across a mass drop it is fl(y + jump) in the mass and the bits elsewhere"""
    prob, E, X = example()
    k = 2
    plan = E.propagation_plan(steps=k, restart="chain")
    nn = [int(v) for v in E.num_nodes]
    for b in (0, 1):
        y, by, err, be = ft.fly_all(E, plan, prob, X[b])
        r0 = pt.propagate_phase(E, plan, prob, X[b], 0)
        assert np.array_equal(_bits(y[:nn[0] + 1]), _bits(r0["y"])) and np.array_equal(_bits(by[:nn[0] + 1]), _bits(r0["bound"]))
        drops = 0
        for s in range(1, E.S):
            xa = sum(nn[:s]) + s
            jump = mt.phase_state(E, X[b], s)[0][0] - mt.phase_state(E, X[b], s - 1)[0][-1]
            assert np.all(jump[1:] == 0.0)
            if jump[0] == 0.0:
                assert np.array_equal(_bits(y[xa]), _bits(y[xa - 1])), (b, s)
                assert np.array_equal(by[xa], by[xa - 1])
            else:
                drops += 1
                assert np.array_equal(_bits(y[xa, 1:]), _bits(y[xa - 1, 1:])) and y[xa, 0] == y[xa - 1, 0] + jump[0], (b, s)
                assert by[xa, 0] == 2 * (by[xa - 1, 0] / 2 + pt.U * (abs(jump[0]) + abs(y[xa, 0])))
        assert drops == (0, 3)[b]
        assert np.all(np.isfinite(err)) and np.all(be > 0)
    # no dispersion and factors of one: the same bits (x * 1.0 is x)
    y1, _b, _e, _be = ft.fly_all(E, plan, prob, X[1], disp=np.ones((E.S, 4)), want_bound=False)
    assert np.array_equal(_bits(y1), _bits(ft.fly_all(E, plan, prob, X[1], want_bound=False)[0]))
    plan.close()


def test_truth_node_restart():
    """fly_all(restart="node"): without factors it is propagate_truth.propagate_all(restart=True), bit for bit (y, bound, err);
    the first node interval of every phase is the section mode's (both start from X_0 with E = 0), with factors too; the later
    intervals are not (the section mode carries its state on); and the factors reach every interval"""
    prob, E, X = example()
    k = 2
    plan = E.propagation_plan(steps=k, restart="node")
    nn = [int(v) for v in E.num_nodes]
    for b in (1, 2):
        got = ft.fly_all(E, plan, prob, X[b], restart="node")
        ref = pt.propagate_all(E, plan, prob, X[b], restart=True)
        for a, r, name in zip(got, ref, ("y", "bound_y", "err", "bound_err")):
            assert np.array_equal(_bits(a), _bits(r)), (b, name)
    disp = ft.teeth_dispersion(E.S)
    for d in (None, disp):
        yn, bn, _e, _be = ft.fly_all(E, plan, prob, X[1], disp=d, restart="node")
        ys, bs, _e, _be = ft.fly_all(E, plan, prob, X[1], disp=d, chain=False)
        later = 0
        for s in range(E.S):
            xa = sum(nn[:s]) + s
            assert np.array_equal(_bits(yn[xa:xa + 2]), _bits(ys[xa:xa + 2])) and np.array_equal(_bits(bn[xa:xa + 2]), _bits(bs[xa:xa + 2])), s
            later += int(not np.array_equal(_bits(yn[xa + 2:xa + nn[s] + 1]), _bits(ys[xa + 2:xa + nn[s] + 1])))
        assert later == E.S
    y0 = ft.fly_all(E, plan, prob, X[1], restart="node", want_bound=False)[0]
    moved = np.any(_bits(yn) != _bits(y0), axis=1)
    powered = [s for s in range(E.S) if prob["engine_on"][s]]
    assert len(powered) >= 6
    for s in range(E.S):
        xa = sum(nn[:s]) + s
        assert not moved[xa], s                                              # node xa is X_0
        if s in powered:                                                     # (a coast above the air has nothing to scale)
            assert moved[xa + 1:xa + nn[s] + 1].all(), s                     # every interval feels the phase's factors
    plan.close()


@pytest.mark.parametrize("mutate", ["no_jump", "shift_factors", "no_wind_factor"])
def test_truth_rejects_wrong_restatements(mutate):
    """the correct restatement and each wrong one differ by far more than 2 E, so the device test cannot pass vacuously"""
    prob, E, X = example()
    plan = E.propagation_plan(steps=1, restart="chain")
    disp = None if mutate == "no_jump" else ft.teeth_dispersion(E.S)
    y, by, _e, _be = ft.fly_all(E, plan, prob, X[1], disp=disp)
    miss = ft.mutant_miss(E, plan, prob, X[1], disp, mutate, y, by)
    print("mutation %s: differs from the restatement by %.3g of 2 E" % (mutate, miss))
    assert miss > 1.0e4, (mutate, miss)
    plan.close()


@sanitized_lib.needs_toolchain
def test_chain_plan_builder_under_asan_ubsan(tmp_path):
    """the plan builder in all three modes, its refusals and gel_prop_matrices on a host-only handle, in a stand-alone program
    (tests/flight_sanitize.c) under AddressSanitizer + UBSan + LeakSanitizer; nothing is launched"""
    sanitized_lib.run_program(tmp_path, sanitized_lib.build(tmp_path), "flight_sanitize")

"""Who owns a problem handle and what it frees: the Engine and the pinned views it hands out each hold the handle's
owner object, never the Engine itself, so reference counting frees both without the cyclic collector; and destroying a handle
returns every working set it grew on the device."""
import gc
import weakref

import numpy as np
import pytest

from gelato_amd import Engine, con_dynamics, pack_x, problem


def _engine(name, device=0):
    pdict, unitdict, _c, xdict = problem.make_problem(name)
    return Engine(con_dynamics.problem_arrays(pdict, unitdict), device=device), pdict, pack_x(xdict)


def test_a_host_only_engine_is_freed_by_reference_counting():
    """`del` frees the engine and its handle's owner at once, without the cyclic collector (which GPU memory pressure never
    triggers), after every call that caches something on the engine."""
    gc.collect()
    gc.disable()
    try:
        E, _p, _x = _engine("mixed-6x64", device=-1)
        E.pattern(); E.var_index(); E.full_source(); E.jac_fd_block_dims("vel")
        E.shard_plan([0, 4 * E.num_chunks()])
        E.aero_configure("q", [(0, 1, 3.5e4)]); E.aero_record_layout()
        E.rows_configure([(0, 1.0, -1, 0.0, 0.0)], [])
        we, wo = weakref.ref(E), weakref.ref(E._owner)
        del E
        assert we() is None and wo() is None
    finally:
        gc.enable()


@pytest.mark.gpu
def test_pinned_views_keep_the_handle_alive_not_the_engine():
    """A pinned view that outlives its engine keeps the handle's owner -- and so the pinned memory it reads -- alive; the engine
    itself goes at once, and the handle with the last view."""
    E, _p, x0 = _engine("example")
    pres, pvals = E.pinned_buffers()
    xb, xp = E.pinned_x()
    xb[0][:] = x0
    _r, _v, rc = E.eval(xb[0], out=pvals, res_out=pres)
    assert rc == 0
    want = pres.copy()
    gc.collect()
    gc.disable()
    try:
        we, wo = weakref.ref(E), weakref.ref(E._owner)
        del E, pvals, xb, xp, _r, _v
        assert we() is None
        assert wo() is not None and wo().ptr
        assert np.array_equal(pres, want)
        del pres
        assert wo() is None
    finally:
        gc.enable()


@pytest.mark.gpu
def test_handle_teardown_returns_its_device_memory():
    """One warm-up cycle, then ten: each creates a handle, grows every lazily allocated working set (pipelined slots, the zero-copy
    one-vector set, jac_fd, aero and row tables with calls above the zero-copy limit, a shard plan, the output table's scratch)
    and destroys it.  Free device memory after the ten cycles is within one cycle's largest working set of its value after the
    warm-up."""
    import torch
    torch.cuda.init()

    def cycle():
        free0 = torch.cuda.mem_get_info()[0]
        E, pdict, x0 = _engine("mixed-6x64")
        S = pdict["num_sections"]
        X = problem.synthetic_batch(x0, E.M, 8)
        B = (16 << 20) // (8 * E.V) + 3                      # above one staging slot: the pipelined path
        assert E.eval_batch(np.tile(X, (B // 8 + 1, 1))[:B])[2] == 0
        pres, pvals = E.pinned_buffers()
        assert E.eval(x0, out=pvals, res_out=pres)[2] == 0
        assert E.jac_fd("vel", x0)[1] == 0
        for kind, lim in (("alpha", 0.2), ("q", 4.0e4), ("qalpha", 5.0e3)):
            E.aero_configure(kind, [(i, 1, lim) for i in range(S - 1)])
        Bz = (1 << 20) // (8 * E.nvars) + 2                  # above the zero-copy limit: the device working set
        Xz = np.tile(X, (Bz // 8 + 1, 1))[:Bz]
        assert E.eval_aero_all(Xz)[2] == 0
        E.rows_configure([(0, 1.0, -1, 0.0, 0.0)], [("radius", 0, 6.4e6, 1.0)])
        assert E.rows_eval(Xz)[2] == 0
        E.shard_plan([0, 2 * E.num_chunks(), 4 * E.num_chunks()])
        assert E.output_table(x0, np.linspace(0.0, 100.0, E.M), 30.0, 130.0).shape == (E.M, len(E.OUTPUT_COLUMNS))
        used = free0 - torch.cuda.mem_get_info()[0]
        E.close()
        del E, pres, pvals
        return used

    cycle()
    after_warmup = torch.cuda.mem_get_info()[0]
    largest = max(cycle() for _ in range(10))
    after = torch.cuda.mem_get_info()[0]
    print("handle teardown: largest working set %.1f MiB, free after warm-up %.1f MiB, after ten cycles %.1f MiB"
          % (largest / 2**20, after_warmup / 2**20, after / 2**20))
    assert largest > 0
    assert after_warmup - after <= largest

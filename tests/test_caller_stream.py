"""Every device entry point of include/gelato_amd.h on a caller-owned, non-blocking stream (tests/stream_harness.py has the
protocol, tests/stream_cases.py the case table).  Until this module, every GPU test passed torch.cuda.current_stream().cuda_stream,
which is 0 for torch's default stream and selects the handle's own (blocking) stream: the `stream != NULL` branch of no entry
point had ever run, and a launch, memset or workspace tied to the wrong stream could not be seen.

Reference: bit-identity with the same call on the handle's stream (stream = 0), which carries every oracle and 60-digit
comparison of that path over; one independent anchor, the chained consumer's g against tests/jac_products_truth.py (long double)
under its derived bound.

Measured on an MI355X (printed by every case; DESIGN.md 3.11 has the figures): the calibration of torch.cuda._sleep in cycles per
ms and the largest delay used."""
import numpy as np
import pytest

import stream_cases as SC
import stream_harness as H

pytestmark = pytest.mark.gpu

ALL = SC.all_cases()


@pytest.mark.parametrize("make", [m for _i, m in ALL], ids=[i for i, _m in ALL])
def test_entry_point_on_a_caller_stream(make, request):
    """late input behind a delay, the call(s) on the side stream, snapshots, poison; bit-identical to the stream = 0 call, nothing
    written late, status 0 from gel_sync(stream)"""
    H.check(make(), request.node.callspec.id)


def _chain_case(E, X, Xs):
    B = len(X)

    def call(E, p, s):
        E.eval_batch_device(B, p["x"], p["res"], p["jvar"], s)
        E.jac_rmatvec_device(B, p["jvar"], p["res"], p["g"], s)      # lambda = the residual the launch before has just written
    return H.Case(E, B, {"x": (X, Xs)}, {"res": (B, E.nres), "jvar": (B, E.V), "g": (B, E.nvars)}, call)


@pytest.mark.parametrize("flags", [0, 32])
@pytest.mark.parametrize("B", [8, 1024])
def test_chained_consumer(B, flags):
    """an optimiser that keeps its state on the GPU: late x -> eval_batch_device (res, jvar) -> jac_rmatvec_device(lambda = d_res)
    -> g, all on its own stream with no host synchronisation.  g is Engine.merit_gradient(X)[1] bit for bit, and lies within the
    derived bound of the long-double products (the anchor that does not rest on the engine)"""
    import jac_products_truth as jt
    E, x0 = SC.engine("mixed-6x64", flags)
    X, Xs = SC.inputs(E, x0, B, distinct=B)
    snaps = H.check(_chain_case(E, X, Xs), "chained consumer B %d flags %d" % (B, flags))
    g, res, jv = (snaps[k].cpu().numpy() for k in ("g", "res", "jvar"))
    _phi, gm, rc = E.merit_gradient(X)
    assert rc == 0 and np.array_equal(g, gm)
    R, C = jt.triplet_index(E)
    worst = 0.0
    for b in (range(B) if B <= 8 else (0, 1, B // 2, B - 1)):
        ok, share, at = jt.check(E, R, C, E.expand(jv[b]), res[b], g[b], True)
        assert ok, (b, share, at)
        worst = max(worst, share)
    print("chained consumer B %d flags %d: largest share of the J^T lambda bound used %.3f" % (B, flags, worst))


def test_two_handles_on_two_side_streams():
    """one handle = one stream at a time, two handles on two streams at once: both enqueued behind their own delays before either
    runs, both bit-identical to the serial results"""
    from gelato_amd import Engine
    import jac_products_truth as jt
    cases = []
    for name in ("mixed-6x64", "example"):
        prob, x0 = jt.named(name)
        E = Engine(prob)
        B = 37
        cases.append(H.Case(E, B, {"x": SC.inputs(E, x0, B)}, {"res": (B, E.nres), "jvar": (B, E.V)},
                            lambda E, p, s, B=B: E.eval_batch_device(B, p["x"], p["res"], p["jvar"], s)))
    refs = [H.reference(c) for c in cases]
    assert all(rc == 0 for _o, rc, _ms in refs)
    d = H.delay_ms_for(sum(ms for _o, _rc, ms in refs))
    import torch
    pend = [H.prepare(c, k) for k, c in enumerate(cases)]
    torch.cuda.synchronize()
    for p in pend:
        p.start(d)
    for p in pend:
        p.assert_pending()
    for c, p, (ref, _rc, _ms) in zip(cases, pend, refs):
        snaps, outs, rc = p.finish()
        assert rc == 0 and H.compare(c, snaps, ref) == [] and H.poisoned(outs) == []


def _nonfinite_cases():
    def bad_x(case, E):
        good, stale = case.late["x"]
        bad = good.copy()
        bad[2, E.M:4 * E.M] = np.nan                 # vector 2: every position
        return case.with_late(x=(bad, stale))

    def bad_jvar(case, E):
        good, stale = case.late["jvar"]
        bad = good.copy()
        bad[2, E.V // 3] = np.nan
        return case.with_late(jvar=(bad, stale))
    return [("gel_eval_batch_device", SC.eval_batch("mixed-6x64", 0, 5, "rj")[1], bad_x),
            ("gel_eval_aero_all_device", SC.aero_all(64, 5, True)[1], bad_x),
            ("gel_rows_eval_device", SC.rows(128, 5, True, "rows_terminal")[1], bad_x),
            ("gel_mesh_error_device", SC.mesh("mixed-6x64", 5, True)[1], bad_x),
            ("gel_jac_matvec_device", SC.jprod("mixed-6x64", 0, 5, False)[1], bad_jvar)]


@pytest.mark.parametrize("entry,make,plant", _nonfinite_cases(), ids=[c[0] for c in _nonfinite_cases()])
def test_nonfinite_status_on_a_caller_stream(entry, make, plant):
    """a NaN in one vector: gel_sync(stream) answers 1, the other vectors' rows are the bits of a clean run, and the same call
    made clean answers 0 again"""
    case = make()
    clean = H.check(case, entry + " clean")
    keep = [0, 1, 3, 4]
    snaps = H.check(plant(case, case.E), entry + " with a NaN", expect_rc=1, rows=keep)
    for name in case.outputs:
        assert H.same_bits(snaps[name][keep], clean[name][keep]), (entry, name)
    assert any(bool(snaps[name][2].isnan().any()) for name in case.outputs), entry
    again = H.check(case, entry + " clean again")
    assert all(H.same_bits(again[name], clean[name]) for name in case.outputs)


HOST_FORMS = ["gel_eval_batch", "gel_rows_eval", "gel_mesh_error", "gel_jac_matvec", "gel_eval_aero_all", "gel_jac_fd"]


@pytest.mark.parametrize("form", HOST_FORMS)
def test_host_form_nonfinite_then_device_form(form):
    """A host-form call that returns GEL_NONFINITE clears the device's flag.  A NaN batch on the caller's stream right after that
    return, with no synchronise, must still be reported by gel_sync(stream): the clear is waited for before the host form returns
    (it cannot be forced to lose the race from here; the ordering is fixed in gel_host.hip clear_flag).  Then a clean batch
    answers 0.  B = 300 takes the copy path of every host form (the small zero-copy path keeps its flag in host memory)."""
    import torch
    from gelato_amd import Engine, problem
    import jac_products_truth as jt
    prob, x0 = jt.named("example")
    E = Engine(prob)
    SC.CONFIGS["example_everything"](E)
    X = problem.synthetic_batch(x0, E.M, 300)
    bad = X.copy()
    bad[7, E.M:4 * E.M] = np.nan
    _r, jv5, rc = E.eval_batch(X[:5], want_res=False)
    assert rc == 0
    jv_bad = jv5.copy()
    jv_bad[3, E.V // 2] = np.nan
    V5 = np.random.default_rng(3).standard_normal((5, E.nvars))
    host = {"gel_eval_batch": lambda: E.eval_batch(bad)[2], "gel_rows_eval": lambda: E.rows_eval(bad)[2],
            "gel_mesh_error": lambda: E.mesh_error(bad)[2], "gel_jac_matvec": lambda: E.jac_matvec(jv_bad, V5)[1],
            "gel_eval_aero_all": lambda: E.eval_aero_all(bad)[2], "gel_jac_fd": lambda: E.jac_fd("vel", bad[7])[1]}[form]
    side = H.side_stream()
    B = 5
    d_bad, d_good = torch.from_numpy(bad[5:10].copy()).cuda(), torch.from_numpy(X[5:10].copy()).cuda()
    res = torch.full((B, E.nres), H.SENTINEL, dtype=torch.float64, device="cuda")
    jv = torch.full((B, E.V), H.SENTINEL, dtype=torch.float64, device="cuda")
    ref_r, ref_j = torch.empty_like(res), torch.empty_like(jv)
    E.eval_batch_device(B, d_good.data_ptr(), ref_r.data_ptr(), ref_j.data_ptr(), 0)
    assert E.sync(0) == 0
    torch.cuda.synchronize()
    assert host() == 1
    E.eval_batch_device(B, d_bad.data_ptr(), res.data_ptr(), jv.data_ptr(), side.cuda_stream)     # at once: no synchronise
    assert E.sync(side.cuda_stream) == 1
    assert bool(res[2].isnan().any())
    E.eval_batch_device(B, d_good.data_ptr(), res.data_ptr(), jv.data_ptr(), side.cuda_stream)
    assert E.sync(side.cuda_stream) == 0
    assert H.same_bits(res, ref_r) and H.same_bits(jv, ref_j)
    if form == "gel_eval_batch":
        # the copy path must not leave its host-side copy of the flag set either: the next one-vector call (zero-copy path, flag in
        # host memory) is clean
        assert host() == 1
        _res1, rc1 = E.eval_residual(X[0])
        assert rc1 == 0


def test_workspace_growth_behind_a_pending_product():
    """gel_jac_rmatvec_device sums the time columns through a workspace of the handle that grows with B: behind one delay, the
    product at B = 8 and then at B = 4096 on a handle that has not made a product yet.  The growing call waits for the caller's
    stream before the old block is released; both results are the bits of the serial calls (made on another handle, whose
    workspace never grows behind anything)."""
    from gelato_amd import Engine, problem
    import jac_products_truth as jt
    prob, x0 = jt.named("mixed-6x64")
    E_serial, E = Engine(prob), Engine(prob)
    P, B = 64, 4096
    X, Xs = SC.inputs(E, x0, P)
    jv = [E_serial.eval_batch(a, want_res=False)[1] for a in (X, Xs)]
    rng = np.random.default_rng(8)
    lam = (rng.standard_normal((P, E.nres)), rng.standard_normal((P, E.nres)))

    def call(E, p, s):
        E.jac_rmatvec_device(8, p["jvar"], p["lam"], p["g8"], s)
        if s:
            assert H.side_stream().query() is False, "delay too short"
        E.jac_rmatvec_device(B, p["jvar"], p["lam"], p["g"], s)
    case = H.Case(E_serial, B, {"jvar": tuple(jv), "lam": lam}, {"g8": (8, E.nvars), "g": (B, E.nvars)}, call)
    ref, rc, ms = H.reference(case)
    assert rc == 0
    case.E = E
    snaps, outs, rc = H.enqueue(case, H.delay_ms_for(ms)).finish()
    assert rc == 0 and H.compare(case, snaps, ref) == [] and H.poisoned(outs) == []


def test_host_calls_of_growing_batch_between_device_calls():
    """two gel_eval_batch host calls of growing B (the handle's staging buffers grow twice) placed between device calls that are
    pending behind a delay on the caller's stream: every result is the bits of the serial calls"""
    from gelato_amd import Engine
    import jac_products_truth as jt
    prob, x0 = jt.named("mixed-6x64")
    E_serial, E = Engine(prob), Engine(prob)
    B = 37
    X, Xs = SC.inputs(E, x0, B)
    host = {}

    def call(E, p, s):
        E.eval_batch_device(B, p["x"], p["res0"], p["jvar0"], s)
        host[2] = E.eval_batch(X[:2])
        E.eval_batch_device(B, p["x"], p["res1"], 0, s)
        host[64] = E.eval_batch(np.tile(X, (2, 1))[:64])
        E.eval_batch_device(B, p["x"], 0, p["jvar2"], s)
    case = H.Case(E_serial, B, {"x": (X, Xs)}, {"res0": (B, E.nres), "jvar0": (B, E.V), "res1": (B, E.nres), "jvar2": (B, E.V)}, call)
    ref, rc, ms = H.reference(case, timed=False)
    assert rc == 0
    serial = dict(host)
    case.E = E
    snaps, outs, rc = H.enqueue(case, H.MIN_DELAY_MS).finish()
    assert rc == 0 and H.compare(case, snaps, ref) == [] and H.poisoned(outs) == []
    for n in (2, 64):
        assert host[n][2] == 0 and np.array_equal(host[n][0], serial[n][0]) and np.array_equal(host[n][1], serial[n][1])


def _aero_shapes(E, B):
    dims = [E.aero_dims(k) for k in SC.KINDS]
    out = {"con%d" % i: (B, d[0]) for i, d in enumerate(dims)}
    out.update({"jac%d" % i: (B, sum(d[1])) for i, d in enumerate(dims)})
    return out


def _aero_launch(E, B, p, s, t):
    E.eval_aero_all_device(B, p["x"], [p["con%d%s" % (i, t)] for i in range(3)], [p["jac%d%s" % (i, t)] for i in range(3)], s)


def _rows_launch(E, B, p, s, t):
    E.rows_eval_device(B, p["x"], p["con" + t], p["jfn" + t], s)


def _shard_launch(E, B, p, s, t):
    for r in range(E.shard_plan_key[0]):
        E.eval_shard_packed_device(B, p["x"], p["exchange" + t], r, s)
    E.shard_unpack_device(B, p["exchange" + t], p["res" + t], p["jvar" + t], s)


# what: (problem, the two configurations, shapes of one launch's outputs under the current configuration, the launch)
RECONFIGURATIONS = {
    "gel_aero_configure": ("mixed-6x64", [SC.CONFIGS["aero_all"], SC.CONFIGS["aero_initial"]], _aero_shapes, _aero_launch),
    "gel_rows_configure": ("example", [SC.CONFIGS["rows_terminal"], SC.CONFIGS["rows_waypoint"]],
                           lambda E, B: {"con": (B, E._nlin + E._nfn), "jfn": (B, E._nfn, 7)}, _rows_launch),
    "gel_shard_plan": ("mixed-6x64", [lambda E: E.shard_plan([0, (4 * E.num_chunks()) // 3, (8 * E.num_chunks()) // 3, 4 * E.num_chunks()]),
                                      lambda E: E.shard_plan([0, 2 * E.num_chunks(), 4 * E.num_chunks()])],
                       lambda E, B: {"exchange": (E.shard_plan_key[0], B, E.shard_plan_key[1]), "res": (B, E.nres), "jvar": (B, E.V)},
                       _shard_launch),
}


@pytest.mark.parametrize("what", list(RECONFIGURATIONS))
def test_reconfiguration_waits_for_the_callers_stream(what):
    """gel_aero_configure, gel_rows_configure and gel_shard_plan replace device tables that launches read.  Behind a delay on the
    caller's stream: a launch under configuration A (pending: side.query() is False), then the reconfiguration to B from the host
    -- it must come back only when the caller's stream has drained (side.query() is True: the old tables are released after
    that) -- then a launch under B.  Both launches' outputs are the bits of the serial calls on another handle."""
    from gelato_amd import Engine
    import jac_products_truth as jt
    name, cfgs, shapes, launch = RECONFIGURATIONS[what]
    prob, x0 = jt.named(name)
    E_serial, E = Engine(prob), Engine(prob)
    B = 37
    outs = {}
    for t, cfg in zip("BA", reversed(cfgs)):            # leaves configuration A on the serial handle
        cfg(E_serial)
        outs.update({k + t: shp for k, shp in shapes(E_serial, B).items()})
    cfgs[0](E)
    side, seen = H.side_stream(), {}

    def call(E, p, s):
        launch(E, B, p, s, "A")
        if s:
            assert side.query() is False, "delay too short"
        cfgs[1](E)
        if s:
            seen["drained"] = side.query()
        launch(E, B, p, s, "B")
    case = H.Case(E_serial, B, {"x": SC.inputs(E, x0, B)}, outs, call)
    ref, rc, _ms = H.reference(case, timed=False)
    assert rc == 0
    case.E = E
    snaps, after, rc = H.enqueue(case, H.MIN_DELAY_MS).finish()
    assert seen["drained"] is True, "the reconfiguration returned while the caller's stream still had work in flight"
    assert rc == 0 and H.compare(case, snaps, ref) == [] and H.poisoned(after) == []


def _teeth_cases():
    return [("gel_eval_batch_device", SC.eval_batch("mixed-6x64", 0, 37, "rj")[1]),
            ("gel_jac_matvec_device", SC.jprod("mixed-6x64", 0, 37, False)[1])]


@pytest.mark.parametrize("entry,make", _teeth_cases(), ids=[c[0] for c in _teeth_cases()])
def test_teeth_a_call_on_the_wrong_stream_is_seen(entry, make):
    """the harness unchanged, except that the engine call gets stream = 0 while the producer stays on the side stream: the
    handle's blocking stream does not wait for a non-blocking side stream, so the snapshot is the result for the STALE input, bit
    for bit, and differs from the result for the good input.  Valid memory and finite values only."""
    case = make()
    ref_good, rc0, ms = H.reference(case, 0)
    ref_stale, rc1, _ms = H.reference(case, 1, timed=False)
    assert rc0 == 0 and rc1 == 0
    p = H.enqueue(case, H.delay_ms_for(ms), engine_on_handle=True)
    p.assert_pending()
    snaps, outs, rc = p.finish()
    assert rc == 0 and H.poisoned(outs) == []
    assert H.compare(case, snaps, ref_stale) == [], "the call on the handle's stream did not read the stale input"
    assert set(H.compare(case, snaps, ref_good)) == set(case.outputs), "the harness cannot tell a call on the wrong stream"

"""GPU: the launch forms that only a large batch or an environment switch selects.

Method (tests/size_forms.py): a batch tiles 256 distinct decision vectors; the reference is the same entry point called once at
B = 256; every block of 256 rows of every output must equal it bit for bit (compared on the device, chunk by chunk); the call is
repeated into the poisoned buffers and checked again (run-to-run bits); three sampled vectors are held against the one-vector host
call (bits) and against an independent anchor at a tolerance the project already states; and the checker shows its teeth on every
output: one bit planted in the last cell, in the first cell past 2^31 bytes / 2^31 elements and in the first vector of a second run
is found exactly there.  Which form a batch size selects is asserted through gel_aero_launch_info / gel_jac_products_launch_info or
plain arithmetic on the dims.  Since every block equals the B = 256 reference, its finiteness is the whole batch's.

No input is invalid and no launch gets a wrong size: the only non-finite values are NaNs planted in ONE decision vector, whose
handling (status through gel_sync, the other vectors untouched) is part of the contract.

Each test states the device memory it needs (asserted <= 64 GB from the dims) and skips only when the card has less free."""
import gc

import numpy as np
import pytest

import jac_products_truth as jt
import size_forms as SF

pytestmark = pytest.mark.gpu
P = SF.P
KINDS = ["alpha", "q", "qalpha"]
VARS = ["position", "velocity", "quaternion", "t"]
CTOL = {"alpha": 1e-11, "q": 1e-12, "qalpha": 1e-11}     # tests/test_aero_oracle_golden.py: constraint values against the oracle


@pytest.fixture(autouse=True)
def _release_device_memory():
    yield
    import torch
    gc.collect()
    torch.cuda.empty_cache()


def _need(nbytes, what):
    """the test's peak device memory, from its dims: at most 64 GB by arithmetic; a skip only where the card has less free"""
    import torch
    nbytes = int(nbytes) + (2 << 30)                   # the checker's temporaries and the B = 256 references
    assert nbytes <= SF.LIMIT_BYTES, (what, nbytes)
    gc.collect()
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < nbytes:
        pytest.skip("%s needs %.1f GB of device memory, %.1f GB are free" % (what, nbytes / 1e9, free / 1e9))


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _buf(shape, fill=SF.POISON):
    import torch
    return torch.full(tuple(shape), fill, dtype=torch.float64, device="cuda")


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tiled(ref, B):
    """[B, w] on the device: row b = row b % 256 of ref"""
    return ref.repeat(-(-B // ref.shape[0]), 1)[:B].contiguous()


def _finite(*tensors):
    import torch
    return all(bool(torch.isfinite(t).all()) for t in tensors)


def _untouched(t, B):
    """rows B.. of a buffer that a call of B vectors must leave alone"""
    return t.shape[0] == B or bool((t[B:] == SF.POISON).all())


def _oracle(E, prob):
    import oracle
    return oracle.Problem(prob, D=[E.D(i) for i in range(E.S)], tau=[E.tau(i) for i in range(E.S)])


def _anchor_defects(E, Por, x, flags, what):
    """one vector against the oracle: check_against_oracle's bounds for the forward-difference forms (residuals 1e-12 + 1e-10 |ref|
    + the D.X summation bound, x-dependent entries 1e-5 + 1e-6 |ref|); for the exact defect Jacobian (flag 32) the residuals likewise
    and the entries within 1e-5 + 1e-6 |ref|, vel/position 1e-5 + 1e-5 |ref| (tests/test_exact_jac.py) -> (res, vals) of gel_eval"""
    from test_gpu_parity import check_against_oracle, close, dx_roundoff_bound
    import oracle
    from gelato_amd.engine import BLOCKS
    if not flags & 32:
        return check_against_oracle(E, Por, x, what)
    res, vals, rc = E.eval(x)
    assert rc == 0
    R, bound = E.split_res(res), dx_roundoff_bound(E, x)
    for grp in oracle.GROUPS:
        close(R[grp], Por.residual(grp, x), atol=1e-12 + bound[grp], what="%s residual %s" % (what, grp))
    var, worst = E.var_mask(), -1.0
    for b, (grp, vname) in enumerate(BLOCKS):
        sl = slice(E.block_off[b], E.block_off[b + 1])
        ref, m = Por.jacobian(grp, x)[vname]["coo"][2], var[sl]
        assert np.array_equal(vals[sl][~m], ref[~m]), (what, grp, vname, "constants")
        rt = 1e-5 if (grp, vname) == ("vel", "position") else 1e-6
        ex = np.abs(vals[sl][m] - ref[m]) - (1e-5 + rt * np.abs(ref[m]))
        worst = max(worst, float(ex.max()) if ex.size else -1.0)
    print("%s: exact entries against the oracle, worst excess %.3e" % (what, worst))
    assert worst <= 0.0, (what, worst)
    return res, vals


# ==================================================================================================================================
# 1. gel_eval_aero_all_device with gradients: the flat mapping's negative 32-bit offsets, and the tile fallback
# ==================================================================================================================================
def _aero_all_call(E, B, dX, dcon, djac):
    E.eval_aero_all_device(B, dX.data_ptr(), [t.data_ptr() for t in dcon], [t.data_ptr() for t in djac], _stream())
    return E.sync(_stream())


@pytest.mark.parametrize("flags", [0, 8, 64])
@pytest.mark.parametrize("name,region", [("mixed-6x64", "negative"), ("mixed-6x64", "tiles"),
                                         ("stress-12x128", "negative"), ("stress-12x128", "tiles")])
def test_aero_all_dense_arrays_past_the_32_bit_offsets(name, region, flags):
    """three kinds on phases 0 .. S-2.  "negative": the largest kind's gradient array exceeds 2^31 bytes while the launcher still
    takes the flat mapping (its byte offsets parked as int are negative for the last vectors); "tiles": the first multiple of 256
    for which the launcher falls back to one tile per vector.  Flags 0, 8 (recomputing sweeps: t columns stored) and 64 (values-only
    launch of the same form + exact_aero_kernel).
    Peak memory: x + three constraint arrays + three gradient arrays of B vectors (mixed-6x64 tiles: 18.0 GB; stress-12x128
    tiles: 17.6 GB)."""
    E, prob, x0 = SF.engine(name, flags, "aero_all")
    B = SF.aero_dense_B(E, region)
    info = E.aero_launch_info(B)
    if region == "negative":
        assert info["flat"] == 1 and info["runs"] == 1 and 2 ** 31 < info["max_bytes"] < 2 ** 32, info
    else:
        assert info["flat"] == 0 and info["runs"] == 1 and E.aero_launch_info(B - P)["flat"] == 1, info
    dims = [E.aero_dims(k) for k in KINDS]
    widths = [d[0] for d in dims] + [sum(d[1]) for d in dims]
    assert max(widths) * 8 * B == info["max_bytes"]
    _need(8 * B * (E.nvars + sum(widths)), "aero arrays %s B = %d" % (name, B))
    X = SF.distinct_vectors(E, x0)
    dXr = _up(X)
    ref = [_buf((P, w)) for w in widths]
    assert _aero_all_call(E, P, dXr, ref[:3], ref[3:]) == 0 and E.aero_launch_info(P)["flat"] == 1
    assert _finite(*ref)
    dX = _tiled(dXr, B)
    out = [_buf((B, w)) for w in widths]
    for turn in range(2):                                   # the second turn: the same bits again, into poisoned buffers
        assert _aero_all_call(E, B, dX, out[:3], out[3:]) == 0
        for i, (o, r) in enumerate(zip(out, ref)):
            what = "%s %s %s flags %d B %d" % (name, KINDS[i % 3], "values" if i < 3 else "gradients", flags, B)
            shown = SF.check_blocks(o, r, what, teeth=(turn == 0))
            if turn == 0 and i >= 3 and widths[i] == max(widths):
                assert any(8 * (row * widths[i] + c) >= 2 ** 31 for row, c in shown), "no tooth past 2^31 bytes"
            o.fill_(SF.POISON)
    del out, dX
    # three vectors: the one-vector host call (one tile per wavefront, the callback's form), bit for bit, and the oracle
    Por = _oracle(E, prob)
    specs = {k: [(i, 1, lim) for i in range(E.S - 1)] for k, lim in zip(KINDS, (0.2, 4.0e4, 5.0e3))}
    for k in KINDS:
        Por.aero_configure(k, specs[k])
    for b in SF.SAMPLES:
        c1, j1, rc = E.eval_aero_all(X[b])
        assert rc == 0
        for i, k in enumerate(KINDS):
            assert np.array_equal(ref[i][b].cpu().numpy(), c1[k][0]) and np.array_equal(ref[3 + i][b].cpu().numpy(), j1[k][0]), (k, b)
            oc = Por.aero_residual(k, X[b])
            d = np.abs(c1[k][0] - oc) - (CTOL[k] + 1e-10 * np.abs(oc))
            print("%s vector %d %s values against the oracle: worst excess %.3e" % (name, b, k, d.max()))
            assert d.max() <= 0.0, (k, b, d.max())
        if not flags & 64:
            # dynamic-pressure gradients meet the flat tolerance everywhere (tests/test_aero_engine.py); the angle kinds' stated
            # tolerance needs tests/fd_noise.py's per-entry bounds and stays with that module
            Jo = Por.aero_jacobian("q", X[b])
            rv = np.concatenate([Jo[v]["coo"][2] for v in VARS if dims[1][1][VARS.index(v)]])
            d = np.abs(j1["q"][0] - rv) - (1e-5 + 1e-6 * np.abs(rv))
            print("%s vector %d q gradients against the oracle: worst excess %.3e" % (name, b, d.max()))
            assert d.max() <= 0.0, (b, d.max())


# ==================================================================================================================================
# 2. gel_eval_batch_aero_device where aero_kernel writes part A of the records
# ==================================================================================================================================
def _records_case(E, prob, x0, flags, Bs, name, fused_ref=None):
    """res / jvar / records of every B in Bs (largest first: the buffers are shared, rows past a smaller B must stay untouched)
    block-wise against the B = 256 call; -> the references"""
    import torch
    width, ci, ji = E.aero_record_layout()
    named = np.concatenate([ci[k] for k in KINDS] + [ji[k] for k in KINDS])
    named = torch.from_numpy(np.unique(named[named >= 0]).astype(np.int64)).cuda()
    shapes = (E.nres, E.V, width)
    Bmax = max(Bs)
    _need(8 * Bmax * (E.nvars + sum(shapes)), "records %s B = %d" % (name, Bmax))
    X = SF.distinct_vectors(E, x0)
    dXr = _up(X)

    def call(B, dX, o):
        E.eval_batch_aero_device(B, dX.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), _stream())
        return E.sync(_stream())
    ref = [_buf((P, w)) for w in shapes]
    assert call(P, dXr, ref) == 0
    assert _finite(ref[0], ref[1], ref[2][:, named])
    if fused_ref is not None:                                   # the default handle's fused launch: the same named cells
        assert SF.first_mismatch(fused_ref[0], ref[0]) is None and SF.first_mismatch(fused_ref[1], ref[1]) is None
        assert SF.first_mismatch(fused_ref[2], ref[2], named) is None
    dX = _tiled(dXr, Bmax)
    out = [_buf((Bmax, w)) for w in shapes]
    for B in Bs:
        info = E.aero_launch_info(B, records=True)
        second_run = (info["run_len"],) if info["runs"] > 1 else ()
        for turn in range(2):
            assert call(B, dX, out) == 0
            for o, r, w in zip(out, ref, ("residual rows", "compact values", "records")):
                assert _untouched(o, B), (w, B)
                SF.check_blocks(o[:B], r, "%s %s flags %d B %d" % (name, w, flags, B), rows=second_run if w == "records" else (),
                                teeth=(turn == 0))
                o.fill_(SF.POISON)
    del out, dX
    Por = _oracle(E, prob)
    for b in SF.SAMPLES:
        rec = ref[2][b].cpu().numpy()
        c1, j1, rc = E.eval_aero_all(X[b])
        assert rc == 0
        for k in KINDS:
            assert np.array_equal(E.aero_gather(rec, ci[k]), c1[k][0]) and np.array_equal(E.aero_gather(rec, ji[k]), j1[k][0]), (k, b)
        r1, v1 = _anchor_defects(E, Por, X[b], flags, "%s flags %d vector %d" % (name, flags, b))
        assert np.array_equal(ref[0][b].cpu().numpy(), r1) and np.array_equal(ref[1][b].cpu().numpy(), v1[E.var_index()]), b
    return ref


@pytest.mark.parametrize("flags", [0, 8, 64, 32 | 64])
def test_batch_aero_records_by_aero_kernel_at_bench_size(flags, monkeypatch):
    """mixed-6x64, B = 65536, with GEL_AERO_FUSED=0 (flags 0), flag 8, flag 64 and flags 32|64: aero_kernel (flag 64: its values-only
    launch + exact_aero_kernel) writes part A of 6.07 GB of records.  Part A has 5 x 64 = 320 nodes here -- whole tiles -- so the
    launcher takes one tile per vector with 64-bit record addresses and does NOT split the batch (asserted through the info call;
    the runs are reached by the next test).  Flags 0: the named record cells, residual rows and compact values equal the default
    handle's fused launch.  Peak memory: x 2.7 + res 2.2 + jvar 8.9 + records 6.1 = 19.9 GB."""
    B = 65536
    fused_ref = None
    if flags == 0:
        monkeypatch.setenv("GEL_AERO_FUSED", "1")
        Ef, _prob, x0 = SF.engine("mixed-6x64", 0, "aero_all")
        li = Ef.launch_info(P)
        assert li[1] == 1 and li[2] == 0 and li[4] == 0          # cooperative form, one vector per wavefront: the fused AERO launch
        dXr = _up(SF.distinct_vectors(Ef, x0))
        fused_ref = [_buf((P, w)) for w in (Ef.nres, Ef.V, Ef.aero_record_layout()[0])]
        Ef.eval_batch_aero_device(P, dXr.data_ptr(), *[t.data_ptr() for t in fused_ref], _stream())
        assert Ef.sync(_stream()) == 0
    monkeypatch.setenv("GEL_AERO_FUSED", "0")
    E, prob, x0 = SF.engine("mixed-6x64", flags, "aero_all")
    info = E.aero_launch_info(B, records=True)
    assert info == {"flat": 0, "runs": 1, "run_len": B, "max_bytes": B * 8 * E.aero_record_layout()[0]} and info["max_bytes"] > 2 ** 32
    _records_case(E, prob, x0, flags, [B], "mixed-6x64", fused_ref)


@pytest.mark.parametrize("flags", [0, 8, 64, 32 | 64])
def test_batch_aero_records_in_runs(flags, monkeypatch):
    """stress-12x100: part A has 5 x 100 = 500 nodes (not whole tiles), so aero_kernel takes the flat mapping over the records and a
    batch whose records span more than its 32-bit byte offsets is launched in runs.  B = the next multiple of 256 past one run (two
    runs, the second flat too) and B = run length + 1 (the last run is ONE vector: a tile, same bits) -- runs = 2 asserted through
    the info call, a planted bit found in the first vector of the second run.  A full run reaches byte offsets past 2^31.
    Peak memory (B = 13,568; a run is 13,563 vectors): x 1.7 + res 1.4 + jvar 5.2 + records 4.3 = 12.6 GB."""
    monkeypatch.setenv("GEL_AERO_FUSED", "0")
    name = "stress-12x100"
    E, prob, x0 = SF.engine(name, flags, "aero_all")
    one = E.aero_launch_info(2, records=True)
    assert one["flat"] == 1 and one["runs"] == 1
    hi = SF.round_up(2 ** 32 // (8 * E.aero_record_layout()[0]) + 1)
    Bm = SF.first_multiple_where(lambda B: E.aero_launch_info(B, records=True)["runs"] > 1, P, hi)
    info = E.aero_launch_info(Bm, records=True)
    run = info["run_len"]
    assert info["runs"] == 2 and info["flat"] == 1 and 2 ** 31 < info["max_bytes"] < 2 ** 32 and run < Bm <= run + P
    last = E.aero_launch_info(run + 1, records=True)
    assert last["runs"] == 2 and last["run_len"] == run
    assert E.aero_launch_info(1, records=True)["flat"] == 0 and E.aero_launch_info(Bm - run, records=True)["flat"] == int(Bm - run > 1)
    _records_case(E, prob, x0, flags, [Bm, run + 1], name)


# ==================================================================================================================================
# 3. Jacobian products
# ==================================================================================================================================
def _products(E, B, dj, dv, dl, dy, dg):
    E.jac_matvec_device(B, dj.data_ptr(), dv.data_ptr(), dy.data_ptr(), _stream())
    E.jac_rmatvec_device(B, dj.data_ptr(), dl.data_ptr(), dg.data_ptr(), _stream())
    return E.sync(_stream())


def _bound_check(E, jv_row, v, lam, y, g, what):
    R, C = jt.triplet_index(E)
    full = E.expand(jv_row)
    for t, (inp, got) in enumerate(((v, y), (lam, g))):
        ok, share, worst = jt.check(E, R, C, full, inp, got, bool(t))
        print("%s %s: share of the bound used %.3f" % (what, "J^T lambda" if t else "J v", share))
        assert ok, (what, "J^T lambda" if t else "J v", share, worst)


@pytest.mark.parametrize("name", ["example", "mixed-6x64", "stress-12x128", "ragged"])
def test_products_do_not_depend_on_vb_b_or_the_lane_count(name, monkeypatch):
    """every VB of 1, 2, 4, 8 that fits x 256 / 512 lanes per workgroup, B = 3 and 37: the VB in effect asserted through the info
    call; all outputs bit-identical across VB and across B at a fixed lane count; across the lane counts everything but the time
    columns of J^T lambda bit-identical (lane t sums terms t, t + lanes, ...: their order follows the lane count), those within
    jac_products_truth's bound like everything else.  (Small buffers.)"""
    monkeypatch.delenv("GEL_JPROD_VB", raising=False)
    monkeypatch.delenv("GEL_JPROD_THREADS", raising=False)
    results = {}
    for threads in (512, 256):
        monkeypatch.setenv("GEL_JPROD_THREADS", str(threads))
        E, prob, x0 = SF.engine(name)
        monkeypatch.delenv("GEL_JPROD_THREADS")
        info = E.jac_products_info()
        assert info["threads"] == info["threads_t"] == threads
        default = (info["vb"], info["vb_t"])
        from gelato_amd import problem
        X = problem.synthetic_batch(x0, E.M, 37)
        _res, jv, rc = E.eval_batch(X, want_res=False)
        assert rc == 0
        rng = np.random.default_rng(20261017)
        V, Lam = rng.standard_normal((37, E.nvars)), rng.standard_normal((37, E.nres))
        dj, dv, dl = _up(jv), _up(V), _up(Lam)
        seen = [set(), set()]
        for vb in (1, 2, 4, 8):
            monkeypatch.setenv("GEL_JPROD_VB", str(vb))
            info = E.jac_products_info()
            for t, key in enumerate(("vb", "vb_t")):
                assert info[key] in (vb, default[t]) and info[key] <= max(vb, default[t])     # in effect, or ignored: it does not fit
                seen[t].add(info[key])
            for B in (3, 37):
                dy, dg = _buf((37, E.nres)), _buf((37, E.nvars))
                assert _products(E, B, dj, dv, dl, dy, dg) == 0
                assert _untouched(dy, B) and _untouched(dg, B)
                results[(threads, vb, B)] = (dy[:B].cpu().numpy(), dg[:B].cpu().numpy(), info["vb"], info["vb_t"])
            monkeypatch.delenv("GEL_JPROD_VB")
        assert 1 in seen[0] and 1 in seen[1] and max(seen[0]) == default[0] and max(seen[1]) == default[1]
        assert seen[0] == {v for v in (1, 2, 4, 8) if v <= default[0]} and seen[1] == {v for v in (1, 2, 4, 8) if v <= default[1]}
        y0, g0, _a, _b = results[(threads, 1, 37)]
        for vb in (1, 2, 4, 8):
            for B in (3, 37):
                y, g, _a, _b = results[(threads, vb, B)]
                assert np.array_equal(y.view(np.int64), y0[:B].view(np.int64)), (name, threads, vb, B, "J v")
                assert np.array_equal(g.view(np.int64), g0[:B].view(np.int64)), (name, threads, vb, B, "J^T lambda")
        for b in (0, 2, 36):
            _bound_check(E, jv[b], V[b], Lam[b], y0[b], g0[b], "%s %d lanes vector %d" % (name, threads, b))
        tcol0, S = E.var_offset("t"), E.S
    ya, ga = results[(512, 1, 37)][:2]
    yb, gb = results[(256, 1, 37)][:2]
    assert np.array_equal(ya.view(np.int64), yb.view(np.int64))
    other = np.ones(ga.shape[1], dtype=bool)
    other[tcol0:tcol0 + S + 1] = False
    assert np.array_equal(ga[:, other].view(np.int64), gb[:, other].view(np.int64))
    print("%s: time columns of J^T lambda, 256 against 512 lanes: %d of %d differ in bits" % (
        name, int((ga[:, ~other] != gb[:, ~other]).sum()), ga[:, ~other].size))


@pytest.mark.parametrize("name", ["mixed-6x64", "stress-12x128"])
def test_products_at_full_size(name):
    """mixed-6x64 at B = 65536 (the README's figure) and stress-12x128 with jvar past 2^31 elements; then B - 7 and B - 5 on the same
    buffers, so that B mod VB != 0 for every VB and the clamped tail group runs (the rows behind B stay untouched); and the
    consumer's chain gel_eval_batch_device -> gel_jac_rmatvec_device(lambda = d_res) against Engine.merit_gradient on the 256
    distinct vectors.  Peak memory: x, v, g (nvars each) + res, lambda, y (11 N each) + jvar: mixed-6x64 23.5 GB, stress-12x128
    48.6 GB."""
    E, prob, x0 = SF.engine(name)
    B = 65536 if name == "mixed-6x64" else SF.first_multiple_past(2 ** 31, E.V)
    if name == "stress-12x128":
        assert B * E.V > 2 ** 31 >= (B - P) * E.V
    info = E.jac_products_info()
    for Bt in (B - 7, B - 5):
        assert Bt % 2 == 1                                       # not a multiple of any VB > 1
    _need(8 * B * (3 * E.nvars + 3 * E.nres + E.V), "products %s B = %d" % (name, B))
    X = SF.distinct_vectors(E, x0)
    rng = np.random.default_rng(7)
    V, Lam = rng.standard_normal((P, E.nvars)), rng.standard_normal((P, E.nres))
    dXr, dVr, dLr = _up(X), _up(V), _up(Lam)
    rres, rjv, ry, rg = _buf((P, E.nres)), _buf((P, E.V)), _buf((P, E.nres)), _buf((P, E.nvars))
    E.eval_batch_device(P, dXr.data_ptr(), rres.data_ptr(), rjv.data_ptr(), _stream())
    assert _products(E, P, rjv, dVr, dLr, ry, rg) == 0 and _finite(ry, rg)
    dX, dv, dl = _tiled(dXr, B), _tiled(dVr, B), _tiled(dLr, B)
    dres, djv, dy, dg = _buf((B, E.nres)), _buf((B, E.V)), _buf((B, E.nres)), _buf((B, E.nvars))
    E.eval_batch_device(B, dX.data_ptr(), dres.data_ptr(), djv.data_ptr(), _stream())
    assert E.sync(_stream()) == 0
    SF.check_blocks(djv, rjv, "%s compact values B %d" % (name, B))
    SF.check_blocks(dres, rres, "%s residual rows B %d" % (name, B), teeth=False)
    for turn, Bt in enumerate((B, B, B - 7, B - 5)):
        dy.fill_(SF.POISON)
        dg.fill_(SF.POISON)
        assert _products(E, Bt, djv, dv, dl, dy, dg) == 0
        assert _untouched(dy, Bt) and _untouched(dg, Bt)
        SF.check_blocks(dy[:Bt], ry, "%s J v B %d (VB %d)" % (name, Bt, info["vb"]), teeth=(turn in (0, 2)))
        SF.check_blocks(dg[:Bt], rg, "%s J^T lambda B %d (VB %d)" % (name, Bt, info["vb_t"]), teeth=(turn in (0, 2)))
    # the chain: lambda = the residual rows where the launch left them
    dg.fill_(SF.POISON)
    E.jac_rmatvec_device(B, djv.data_ptr(), dres.data_ptr(), dg.data_ptr(), _stream())
    assert E.sync(_stream()) == 0
    phi, g, rc = E.merit_gradient(X)
    assert rc == 0
    SF.check_blocks(dg, _up(g), "%s merit gradient B %d" % (name, B))
    jv_host = rjv.cpu().numpy()
    for b in SF.SAMPLES:
        y1, rc1 = E.jac_matvec(jv_host[b], V[b])
        g1, rc2 = E.jac_rmatvec(jv_host[b], Lam[b])
        assert rc1 == 0 and rc2 == 0 and np.array_equal(ry[b].cpu().numpy(), y1) and np.array_equal(rg[b].cpu().numpy(), g1), b
        _bound_check(E, jv_host[b], V[b], Lam[b], y1, g1, "%s vector %d" % (name, b))


# ==================================================================================================================================
# 4. Full COO values
# ==================================================================================================================================
def _full_coo_sizes():
    return [("mixed-6x64", "streamed"), ("mixed-6x64", "elements"), ("example", "entrywise"), ("ragged", "odd")]


@pytest.mark.parametrize("name,which", _full_coo_sizes())
def test_full_coo_forms(name, which):
    """gel_expand_full_device, gel_fill_full_device + gel_update_full_device, and gel_eval_full_device with and without residual
    rows, one jfull at a time, block-wise against Engine.expand of the 256 reference rows (uploaded once).
      streamed   mixed-6x64 past the switch of launch_eval's cooperative form from ordinary (cached) to non-temporal Jacobian stores
                 under gel_eval_full_device, B 8 (V + 11 N) > 192e6.  The reference comes from gel_eval_batch_device, which always
                 streams; gel_eval_full_device at B = 256, on the cached side of the switch, must give its bits too; 7.0 GB
      elements   mixed-6x64 with jfull past 2^31 elements; 18.1 GB
      entrywise  example, B = 4099: total_nnz % 8 != 0 selects the entry-wise update kernel; 0.7 GB
      odd        ragged, B = 4099: total_nnz is odd, so every second vector of expand_kernel takes the unaligned store path; 14.5 GB
    fill / update stride a capped gridDim.y over B in all four (the cap binds from B = 16)."""
    E, prob, x0 = SF.engine(name)
    nnz = E.total_nnz
    if which == "streamed":
        B = SF.first_multiple_past(192e6, 8 * (E.V + 11 * E.N))
        assert B * 8 * (E.V + 11 * E.N) > 192e6 >= P * 8 * (E.V + 11 * E.N)
        for Bs in (B, P):                                        # the switch exists in the cooperative, non-split form only
            li = E.launch_info(Bs)
            assert li[0] == 1 and li[1] == 1 and li[2] == 0, (Bs, li)
    elif which == "elements":
        B = SF.first_multiple_past(2 ** 31, nnz)
        assert B * nnz > 2 ** 31 and nnz % 8 == 0
    elif which == "entrywise":
        B = 4099
        assert nnz % 8 != 0 and nnz % 2 == 0
    else:
        B = 4099
        assert nnz % 2 == 1
    assert B >= 16
    _need(8 * (B * (nnz + E.nvars + 2 * E.nres + 2 * E.V) + 2 * P * nnz), "full COO %s B = %d" % (name, B))
    X = SF.distinct_vectors(E, x0)
    dXr = _up(X)
    rres, rjv = _buf((P, E.nres)), _buf((P, E.V))
    E.eval_batch_device(P, dXr.data_ptr(), rres.data_ptr(), rjv.data_ptr(), _stream())
    assert E.sync(_stream()) == 0
    jv_host = rjv.cpu().numpy()
    rfull = _up(E.expand(jv_host))
    assert _finite(rfull)
    s = _stream()
    if which == "streamed":                                      # the cached-store side: the same call at B = 256
        cres, cjv, cfull = _buf((P, E.nres)), _buf((P, E.V)), _buf((P, nnz))
        E.fill_full_device(P, cfull.data_ptr(), s)
        E.eval_full_device(P, dXr.data_ptr(), cres.data_ptr(), cjv.data_ptr(), cfull.data_ptr(), s)
        assert E.sync(s) == 0
        for o, r, w in ((cres, rres, "res"), (cjv, rjv, "jvar"), (cfull, rfull, "jfull")):
            assert SF.first_mismatch(o, r) is None, "eval_full at B = 256 (cached stores): " + w
        del cres, cjv, cfull
    dX = _tiled(dXr, B)
    dres, djv = _buf((B, E.nres)), _buf((B, E.V))
    E.eval_batch_device(B, dX.data_ptr(), dres.data_ptr(), djv.data_ptr(), s)
    assert E.sync(s) == 0
    SF.check_blocks(djv, rjv, "%s compact values B %d" % (name, B), teeth=False)
    dfull = _buf((B, nnz))
    E.expand_full_device(B, djv.data_ptr(), dfull.data_ptr(), s)
    assert E.sync(s) == 0
    shown = SF.check_blocks(dfull, rfull, "%s expand B %d" % (name, B))
    if which == "elements":
        assert any(row * nnz + c >= 2 ** 31 for row, c in shown)
    dfull.fill_(SF.POISON)
    E.fill_full_device(B, dfull.data_ptr(), s)
    E.update_full_device(B, djv.data_ptr(), dfull.data_ptr(), s)
    assert E.sync(s) == 0
    SF.check_blocks(dfull, rfull, "%s fill + update B %d" % (name, B))
    for with_res in (True, False):
        dfull.fill_(SF.POISON)
        dres2, djv2 = _buf((B, E.nres)), _buf((B, E.V))
        E.fill_full_device(B, dfull.data_ptr(), s)
        E.eval_full_device(B, dX.data_ptr(), dres2.data_ptr() if with_res else 0, djv2.data_ptr(), dfull.data_ptr(), s)
        assert E.sync(s) == 0
        what = "%s eval_full %s residual rows B %d" % (name, "with" if with_res else "without", B)
        SF.check_blocks(dfull, rfull, what + " jfull", teeth=with_res)
        SF.check_blocks(djv2, rjv, what + " jvar", teeth=False)
        if with_res:
            SF.check_blocks(dres2, rres, what + " res", teeth=False)
        else:
            assert bool((dres2 == SF.POISON).all())
        del dres2, djv2
    del dfull
    if which == "elements":
        return                                                   # the same problem and vectors: anchored once
    Por = _oracle(E, prob)
    for b in SF.SAMPLES:
        if name == "ragged":                                     # far-from-flight states: the one-vector bits; the oracle anchor on the others
            r1, v1, rc = E.eval(X[b])
            assert rc == 0
        else:
            r1, v1 = _anchor_defects(E, Por, X[b], 0, "%s vector %d" % (name, b))
        assert np.array_equal(rfull[b].cpu().numpy(), v1) and np.array_equal(rres[b].cpu().numpy(), r1), b


# ==================================================================================================================================
# 5. Exact kernels and the row kernels
# ==================================================================================================================================
def _nan_isolation(call, sync, dX, outs, refs, B, col, what):
    """a NaN planted in vector B - 2 (the far end of the grid): gel_sync returns 1, then 0; only that vector's outputs may be
    non-finite, every other vector keeps its bits; the clean call afterwards is clean"""
    import torch
    bad = B - 2
    keep = dX[bad, col].clone()
    dX[bad, col] = float("nan")
    for o in outs:
        o.fill_(SF.POISON)
    rc = call()
    dX[bad, col] = keep
    assert rc == 1 and sync() == 0, (what, rc)                # the status is consumed by the gel_sync that reports it
    for o, r in zip(outs, refs):
        row = o[bad].clone()
        o[bad] = r[bad % P]
        SF.check_blocks(o, r, what + " (the other vectors)", teeth=False)
        o[bad] = row
    assert any(not bool(torch.isfinite(o[bad]).all()) for o in outs), what
    for o in outs:
        o.fill_(SF.POISON)
    assert call() == 0, what
    for o, r in zip(outs, refs):
        SF.check_blocks(o, r, what + " (clean again)", teeth=False)


@pytest.mark.parametrize("name", ["mixed-6x64", "stress-12x128"])
def test_exact_defect_jacobian_at_full_size(name):
    """gel_eval_batch_device on a flag-32 handle (residual-only fused launch + exact_jac_kernel): mixed-6x64 at B = 65536,
    stress-12x128 with jvar past 2^31 elements.  Residual rows bit-equal to a flags-0 handle's at the same B.  Peak memory: x + two
    res + jvar: mixed-6x64 16.0 GB, stress-12x128 32.4 GB."""
    E, prob, x0 = SF.engine(name, 32)
    E0, _p, _x = SF.engine(name, 0)
    B = 65536 if name == "mixed-6x64" else SF.first_multiple_past(2 ** 31, E.V)
    if name == "stress-12x128":
        assert B * E.V > 2 ** 31 >= (B - P) * E.V
    _need(8 * B * (E.nvars + 2 * E.nres + E.V), "exact defects %s B = %d" % (name, B))
    X = SF.distinct_vectors(E, x0)
    dXr = _up(X)
    s = _stream()
    rres, rjv = _buf((P, E.nres)), _buf((P, E.V))
    E.eval_batch_device(P, dXr.data_ptr(), rres.data_ptr(), rjv.data_ptr(), s)
    assert E.sync(s) == 0 and _finite(rres, rjv)
    dX = _tiled(dXr, B)
    dres, djv = _buf((B, E.nres)), _buf((B, E.V))

    def call():
        E.eval_batch_device(B, dX.data_ptr(), dres.data_ptr(), djv.data_ptr(), s)
        return E.sync(s)
    for turn in range(2):
        assert call() == 0
        cells = SF.check_blocks(djv, rjv, "%s exact compact values B %d" % (name, B), teeth=(turn == 0))
        SF.check_blocks(dres, rres, "%s residual rows B %d" % (name, B), teeth=(turn == 0))
        if turn == 0:
            shown = cells
            dres.fill_(SF.POISON)
            djv.fill_(SF.POISON)
    if name == "stress-12x128":
        assert any(row * E.V + c >= 2 ** 31 for row, c in shown)
    dres0 = _buf((B, E.nres))
    E0.eval_batch_device(B, dX.data_ptr(), dres0.data_ptr(), 0, s)
    assert E0.sync(s) == 0
    assert SF.first_mismatch(dres0, dres) is None, "residual rows of the exact handle differ from the flags-0 handle's"
    del dres0
    _nan_isolation(call, lambda: E.sync(s), dX, [dres, djv], [rres, rjv], B, E.M + 3 * 2, "%s exact defects B %d" % (name, B))
    del dres, djv, dX
    Por = _oracle(E, prob)
    for b in SF.SAMPLES:
        r1, v1 = _anchor_defects(E, Por, X[b], 32, "%s flag 32 vector %d" % (name, b))
        assert np.array_equal(rres[b].cpu().numpy(), r1) and np.array_equal(rjv[b].cpu().numpy(), v1[E.var_index()]), b


@pytest.mark.parametrize("flags", [0, 128])
def test_row_kernels_at_full_size(flags):
    """gel_rows_eval_device on the 72-row waypoint table of tools/exact_rows_bench.py (example problem), B = 65536: rows_kernel's
    forward differences (flags 0) and rows_kernel without jfn + exact_rows_kernel (flag 128).  Peak memory: x 0.5 + con 0.04 + jfn
    0.26 GB."""
    E, prob, x0 = SF.engine("example", flags, "rows_waypoint")
    B = 65536
    R = E._nfn
    assert R == 72 and E._nlin == 0
    _need(8 * B * (E.nvars + R + 7 * R), "rows B = %d" % B)
    X = SF.distinct_vectors(E, x0)
    dXr = _up(X)
    s = _stream()
    rcon, rjfn = _buf((P, R)), _buf((P, R * 7))
    E.rows_eval_device(P, dXr.data_ptr(), rcon.data_ptr(), rjfn.data_ptr(), s)
    assert E.sync(s) == 0 and _finite(rcon, rjfn)
    dX = _tiled(dXr, B)
    dcon, djfn = _buf((B, R)), _buf((B, R * 7))

    def call():
        E.rows_eval_device(B, dX.data_ptr(), dcon.data_ptr(), djfn.data_ptr(), s)
        return E.sync(s)
    for turn in range(2):
        assert call() == 0
        SF.check_blocks(dcon, rcon, "rows values flags %d B %d" % (flags, B), teeth=(turn == 0))
        SF.check_blocks(djfn, rjfn, "rows jfn flags %d B %d" % (flags, B), teeth=(turn == 0))
        if turn == 0:
            dcon.fill_(SF.POISON)
            djfn.fill_(SF.POISON)
    _nan_isolation(call, lambda: E.sync(s), dX, [dcon, djfn], [rcon, rjfn], B, E.M, "rows flags %d B %d" % (flags, B))     # x of state node 0: section 0's rows
    for b in SF.SAMPLES:
        c1, j1, rc = E.rows_eval(X[b])
        assert rc == 0 and np.array_equal(rcon[b].cpu().numpy(), c1[0]) and np.array_equal(rjfn[b].cpu().numpy(), j1[0].ravel()), b
    if flags == 128:                                            # the values are rows_kernel's own: bit-equal to the flags-0 handle's
        E0, _p, _x = SF.engine("example", 0, "rows_waypoint")
        c0, _j0, rc = E0.rows_eval(X[0])
        assert rc == 0 and np.array_equal(rcon[0].cpu().numpy(), c0[0])


# ==================================================================================================================================
# 6. The collocation error estimate
# ==================================================================================================================================
@pytest.mark.parametrize("name,B", [("mixed-6x64", 65536), ("stress-12x128", 16384)])
def test_mesh_error_at_full_size(name, B):
    """gel_mesh_error_device with diff.  mesh_kernel packs 512 // (n + 1) vectors into a workgroup (7 at n = 64, 3 at n = 128) and
    neither B is a multiple of that: the last workgroup of every phase is a partial one.  Peak memory: x + err + diff: mixed-6x64
    4.9 GB, stress-12x128 4.9 GB."""
    import mesh_truth as mt
    E, prob, x0 = SF.engine(name)
    vpb = sorted({512 // (int(n) + 1) for n in E.num_nodes})
    assert vpb == ([7] if name == "mixed-6x64" else [3]) and all(B % v != 0 for v in vpb)
    npts = E.mesh_npts()
    _need(8 * B * (E.nvars + 4 * E.S + 11 * npts), "mesh error %s B = %d" % (name, B))
    X = SF.distinct_vectors(E, x0)
    dXr = _up(X)
    s = _stream()
    rerr, rdiff = _buf((P, E.S * 4)), _buf((P, npts * 11))
    E.mesh_error_device(P, dXr.data_ptr(), rerr.data_ptr(), rdiff.data_ptr(), s)
    assert E.sync(s) == 0 and _finite(rerr, rdiff)
    dX = _tiled(dXr, B)
    derr, ddiff = _buf((B, E.S * 4)), _buf((B, npts * 11))

    def call():
        E.mesh_error_device(B, dX.data_ptr(), derr.data_ptr(), ddiff.data_ptr(), s)
        return E.sync(s)
    for turn in range(2):
        assert call() == 0
        SF.check_blocks(derr, rerr, "%s mesh err B %d" % (name, B), teeth=(turn == 0))
        SF.check_blocks(ddiff, rdiff, "%s mesh diff B %d" % (name, B), teeth=(turn == 0))
        if turn == 0:
            derr.fill_(SF.POISON)
            ddiff.fill_(SF.POISON)
    _nan_isolation(call, lambda: E.sync(s), dX, [derr, ddiff], [rerr, rdiff], B, E.M + 3 * 2, "%s mesh B %d" % (name, B))
    for b in SF.SAMPLES:
        e1, d1, rc = E.mesh_error(X[b], want_diff=True)
        assert rc == 0 and np.array_equal(rerr[b].cpu().numpy(), e1[0].ravel()) and np.array_equal(rdiff[b].cpu().numpy(), d1[0].ravel()), b
        re, rd, be, bd = mt.estimate_all(E, prob, X[b])
        ge, gd = np.abs(e1[0] - re), np.abs(d1[0] - rd)
        print("%s vector %d: share of mesh_truth's bound used, err %.3f diff %.3f" % (name, b, float((ge / be).max()), float((gd / bd).max())))
        assert np.all(ge <= be) and np.all(gd <= bd), (name, b)

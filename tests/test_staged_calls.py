"""The host-buffer entry points share one staged-call helper and one pair of arenas per handle (gel_host_handle.h staged_call, DESIGN.md
3.5): what seven private working sets could not get wrong and a shared one can -- a pointer kept across a growth, two carve-outs
that overlap, one form's output landing in another's input -- and the parts of the helper the older tests do not reach: both sides
of the zero-copy limit, optional outputs that are absent, the status rule on the zero-copy branch.

Reference: bit-identity, with the same call made as the only call of a fresh handle, or with the device-pointer entry point of the
same form (which the tests of that form hold against their oracles).  The example problem with rows and every aero kind configured
(stream_cases.CONFIGS["example_everything"]); at most a few hundred vectors."""
import ctypes as C

import numpy as np
import pytest

import stream_cases as SC
import stream_harness as H

pytestmark = pytest.mark.gpu

ZERO_COPY_BYTES = 1 << 20       # gel_host_handle.h kZeroCopyBytes: a call moving at most this much takes the zero-copy branch
FORMS = ["rows", "mesh", "aero"]


def _engine():
    from gelato_amd import Engine
    import jac_products_truth as jt
    prob, x0 = jt.named("example")
    E = Engine(prob)
    SC.CONFIGS["example_everything"](E)
    return E, x0


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(got, ref):
    """tuples of arrays / dicts of arrays / None / status: equal bit for bit"""
    if isinstance(ref, (tuple, list)):
        return len(got) == len(ref) and all(_same(g, r) for g, r in zip(got, ref))
    if isinstance(ref, dict):
        return sorted(got) == sorted(ref) and all(_same(got[k], ref[k]) for k in ref)
    if isinstance(ref, np.ndarray):
        return got.shape == ref.shape and np.array_equal(_bits(got), _bits(ref))
    return got == ref


def _doubles_per_vector(E, form):
    """what one vector moves through the host-buffer form with every output asked for: inputs plus outputs, in doubles"""
    if form == "rows":
        return E.nvars + (E._nlin + E._nfn) + 7 * E._nfn
    if form == "mesh":
        return E.nvars + 4 * E.S + 11 * E.mesh_npts()
    return E.nvars + sum(E.aero_dims(k)[0] + sum(E.aero_dims(k)[1]) for k in SC.KINDS)


def _limit(E, form):
    """the largest B whose call still moves at most ZERO_COPY_BYTES"""
    return ZERO_COPY_BYTES // (8 * _doubles_per_vector(E, form))


@pytest.fixture(scope="module")
def data():
    """inputs shared by the tests, made once on a handle of their own and left unchanged"""
    from gelato_amd import problem
    E, x0 = _engine()
    big = {f: _limit(E, f) + 1 for f in FORMS}
    X = problem.synthetic_batch(x0, E.M, max(max(big.values()), 300))
    rng = np.random.default_rng(20261019)
    _r, jv, rc = E.eval_batch(X[:300], want_res=False)
    assert rc == 0
    _c, jfn4, rc1 = E.rows_eval(X[:4])
    _c, ajac4, rc2 = E.eval_aero_all(X[:4])
    assert rc1 == 0 and rc2 == 0
    R = E.con_products_dims()["R"]
    d = {"x0": x0, "X": X, "big": big, "jv": jv, "V5": rng.standard_normal((5, E.nvars)), "Lam300": rng.standard_normal((300, E.nres)),
         "jfn4": jfn4, "ajac4": ajac4, "Lam4": rng.standard_normal((4, R)), "g4": rng.standard_normal((4, E.nvars)),
         "tx": np.linspace(0.0, 480.0, E.M), "pts": [np.array([-0.5, 0.0, 0.7])] * E.S}
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    E.close()
    return d


def _steps(d):
    """the interleaving of the issue, in order: (name, call(E) -> results)"""
    X, big = d["X"], d["big"]

    def interp(E):
        plan = E.interp_plan(d["pts"])
        out = plan.apply(X[:3])
        plan.close()
        return out

    def propagate(E):
        plan = E.propagation_plan(steps=2)
        out = plan.apply(X[:2], want_err=True)
        plan.close()
        return out
    return [
        ("rows_eval B 1", lambda E: E.rows_eval(X[:1])),
        ("mesh_error diff B %d" % big["mesh"], lambda E: E.mesh_error(X[:big["mesh"]], want_diff=True)),
        ("eval_aero_all B 1", lambda E: E.eval_aero_all(X[:1])),
        ("jac_matvec B 5", lambda E: E.jac_matvec(d["jv"][:5], d["V5"])),
        ("rows_eval B %d" % big["rows"], lambda E: E.rows_eval(X[:big["rows"]])),
        ("interp apply B 3", interp),
        ("propagate apply err B 2", propagate),
        ("con_rmatvec accumulate B 4", lambda E: E.con_rmatvec(d["Lam4"], jfn=d["jfn4"], aero_jac=d["ajac4"], out=d["g4"].copy())),
        ("output_table", lambda E: E.output_table(X[1], d["tx"], 31.25, 131.08)),
        ("jac_rmatvec B 300", lambda E: E.jac_rmatvec(d["jv"], d["Lam300"])),
        ("rows_eval B 1 again", lambda E: E.rows_eval(X[:1])),
    ]


def test_interleaved_forms_on_one_handle(data):
    """every host-buffer form in turn on ONE handle, small and large calls mixed so that both arenas grow between calls that hold
    addresses in them: each result is the bits of the same call made as the only call of a fresh handle"""
    steps = _steps(data)
    E, _x0 = _engine()
    got = [call(E) for _n, call in steps]
    E.close()
    for (name, call), g in zip(steps, got):
        F, _x0 = _engine()
        ref = call(F)
        F.close()
        assert _same(g, ref), name


def _host_and_device(E, form, X):
    """(host-buffer results, device-pointer results) of one form with every output, as lists of numpy arrays"""
    import torch
    B = len(X)
    dX = torch.from_numpy(np.array(X)).cuda()

    def dev(*shape):
        return torch.full((B,) + shape, H.SENTINEL, dtype=torch.float64, device="cuda")
    if form == "rows":
        con, jfn, rc = E.rows_eval(X)
        host, out = [con, jfn], [dev(E._nlin + E._nfn), dev(E._nfn, 7)]
        E.rows_eval_device(B, dX.data_ptr(), out[0].data_ptr(), out[1].data_ptr())
    elif form == "mesh":
        err, diff, rc = E.mesh_error(X, want_diff=True)
        host, out = [err, diff], [dev(E.S, 4), dev(E.mesh_npts(), 11)]
        E.mesh_error_device(B, dX.data_ptr(), out[0].data_ptr(), out[1].data_ptr())
    else:
        con, jac, rc = E.eval_aero_all(X)
        host = [con[k] for k in SC.KINDS] + [jac[k] for k in SC.KINDS]
        out = [dev(E.aero_dims(k)[0]) for k in SC.KINDS] + [dev(sum(E.aero_dims(k)[1])) for k in SC.KINDS]
        E.eval_aero_all_device(B, dX.data_ptr(), [t.data_ptr() for t in out[:3]], [t.data_ptr() for t in out[3:]])
    assert rc == 0 and E.sync() == 0
    return host, [t.cpu().numpy() for t in out]


@pytest.mark.parametrize("form", FORMS)
def test_both_sides_of_the_zero_copy_limit(form, data):
    """the largest B that moves at most 1 MiB (zero-copy branch) and B + 1 (copied branch), from the engine's dims: the host-buffer
    results at both sizes are the device-pointer entry point's bits"""
    E, _x0 = _engine()
    B = _limit(E, form)
    assert 1 <= B and B * _doubles_per_vector(E, form) * 8 <= ZERO_COPY_BYTES < (B + 1) * _doubles_per_vector(E, form) * 8
    for n in (B, B + 1):
        host, device = _host_and_device(E, form, data["X"][:n])
        assert _same(host, device), (form, n)
    E.close()


def _filled(*shape):
    return np.full(shape, H.SENTINEL)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


@pytest.mark.parametrize("B", [1, 300])
def test_optional_outputs_absent(B, data):
    """rows_eval without jfn, mesh_error without diff, eval_aero_all with one kind and no gradients (through the C entry points, so
    that the caller owns every array): what was asked for is the full call's bits, and the arrays the caller filled with the
    sentinel and did not pass stay sentinel"""
    from gelato_amd._lib import lib
    L = lib()
    E, _x0 = _engine()
    X = np.ascontiguousarray(data["X"][:B])
    con_f, jfn_f, rc = E.rows_eval(X)
    err_f, diff_f, rc1 = E.mesh_error(X, want_diff=True)
    acon_f, ajac_f, rc2 = E.eval_aero_all(X)
    assert rc == 0 and rc1 == 0 and rc2 == 0

    con, jfn = _filled(*con_f.shape), _filled(*jfn_f.shape)
    assert L.gel_rows_eval(E._h, B, _dp(X), _dp(con), None) == 0
    assert _same(con, con_f) and np.all(jfn == H.SENTINEL)

    err, diff = _filled(*err_f.shape), _filled(*diff_f.shape)
    assert L.gel_mesh_error(E._h, B, _dp(X), _dp(err), None) == 0
    assert _same(err, err_f) and np.all(diff == H.SENTINEL)

    for i, kind in enumerate(SC.KINDS):
        acon = {k: _filled(*acon_f[k].shape) for k in SC.KINDS}
        ajac = {k: _filled(*ajac_f[k].shape) for k in SC.KINDS}
        cp = (C.POINTER(C.c_double) * 3)()
        cp[i] = _dp(acon[kind])
        assert L.gel_eval_aero_all(E._h, B, _dp(X), cp, None) == 0
        assert _same(acon[kind], acon_f[kind])
        assert all(np.all(acon[k] == H.SENTINEL) for k in SC.KINDS if k != kind) and all(np.all(ajac[k] == H.SENTINEL) for k in SC.KINDS)
    E.close()


@pytest.mark.parametrize("form", FORMS)
def test_status_on_the_zero_copy_branch(form, data):
    """B = 1 keeps its flag in host memory: a NaN vector answers 1, the same call with a clean vector 0, and a device-form batch on
    a side stream right after answers 0 from gel_sync -- the host word did not leak into the device flag, nor the other way"""
    import torch
    E, _x0 = _engine()
    X = data["X"]
    bad = X[:1].copy()
    bad[0, E.M:4 * E.M] = np.nan
    call = {"rows": lambda x: E.rows_eval(x)[2], "mesh": lambda x: E.mesh_error(x, want_diff=True)[2],
            "aero": lambda x: E.eval_aero_all(x)[2]}[form]
    assert call(bad) == 1
    assert call(X[:1]) == 0
    side = H.side_stream()
    d_x = torch.from_numpy(X[:5].copy()).cuda()
    res = torch.empty((5, E.nres), dtype=torch.float64, device="cuda")
    jv = torch.empty((5, E.V), dtype=torch.float64, device="cuda")
    E.eval_batch_device(5, d_x.data_ptr(), res.data_ptr(), jv.data_ptr(), side.cuda_stream)
    assert E.sync(side.cuda_stream) == 0
    assert call(bad) == 1           # and after a device-form call the host word still answers for its own call only
    assert call(X[:1]) == 0
    E.close()

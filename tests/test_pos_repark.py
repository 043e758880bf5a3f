"""GPU: the position part carries (sin lat, cos lat) instead of the half-latitude pair, and the fused kernel keeps the centre's 1/T and
sweep margin in the two park slots the pair used to take (gel_eval_kernel.h, the park slots LV0 / LV1; AERO: 1/hypot(z Ra, p Rb)).

  1  parked equals re-derived: point hook 16 chains one centre and the three sweeps as the fused kernel does -- 1/T and the margin taken
     once (pos_centre_tail), each sweep re-deriving only the wind slopes and the centre's wind (pos_centre_tail_kept) -- and must give
     hook 15's 18 outputs (one pos_centre_tail per sweep) bit for bit, for every point of tests/delta_model.py's input set and every kk;
  2  the slots across launch forms on a windy problem (test_wind_axes.small_problem `3x8` with the never-calm table, and one phase of
     n = 5 nodes): latency form (COO-direct and callback), a handful of vectors, two vectors per wavefront, one vector per wavefront,
     unit-sharded launches -- the same bits; GEL_FLAG_FD_RECOMPUTE (t0 / tf sweeps through wind_eci_chain(), which now forms the
     half-latitude pair itself) the same bits in every form; the fused AERO launch bit for bit as aero_kernel;
  3  a dropped lane: a wavefront with nodes the difference form does not cover (tests/states.py layer_break_state at the position step,
     60 nodes) writes, in its covered lanes, the bits it writes when those nodes are moved off their breaks -- the recomputing pass
     reads the kept 1/T and margin once more, after the first pass's stores.
No shape here is the workload's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LIMS = {"alpha": 0.2, "q": 4.0e4, "qalpha": 5.0e3}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. parked equals re-derived
# ---------------------------------------------------------------------------------------------------------------------------
def test_hook_16_one_centre_three_sweeps_equals_hook_15_bit_for_bit():
    """What this holds: pos_centre_tail_kept(), given pos_centre_tail()'s 1/T and margin, leads pos_delta() to the bits of a
    pos_centre_tail() per sweep, over every layer, wind piece and branch.  Hook 16 is a restatement of the fused kernel's chaining, not
    its GEL_LOAD_POS_CENTRE: it does NOT guard the kernel's park slots or their order against the store tiles -- the launch-form and
    dropped-lane tests below do."""
    import delta_model as M
    import states
    from gelato_amd.dynamics import point_eval
    wind = np.array(states._example_prob()["wind_table"], dtype=np.float64)
    I = M.inputs(wind)
    r, dlt = I["r"], I["dlt"]
    n = len(dlt)
    assert n >= 3000
    cen = M._centre(r, wind)
    assert set(cen["k"]) == set(range(11)), "every atmosphere layer"
    out16 = point_eval(16, np.column_stack([r, np.zeros(n), dlt]), aux=wind).reshape(n, 3, 18)
    seen_ok = seen_not = 0
    for kk in range(3):
        out15 = point_eval(15, np.column_stack([r, np.full(n, float(kk)), dlt]), aux=wind)
        d = bits(out15) != bits(out16[:, kk])
        assert not d.any(), (kk, int(d.sum()), np.argwhere(d)[:6])
        seen_ok += int((out15[:, 16] == 1.0).sum())
        seen_not += int((out15[:, 16] == 0.0).sum())
    # what the input set holds besides every layer: both flat ends of the wind table and a sloping row inside it, the 86 km branch from
    # both sides (layer 6's margin ends at 84852 m geopotential), a point next to the axis, lanes on either side of the predicate
    assert seen_ok > 1000 and seen_not > 100
    assert (cen["h"] < wind[1, 0]).any() and (cen["h"] > wind[-2, 0]).any() and (cen["s0"] != 0.0).any() and (cen["s1"] != 0.0).any()
    assert ((cen["k"] == 6) & (cen["alt"] < 86000.0)).any() and ((cen["k"] == 7) & (cen["alt"] < 86100.0)).any()
    assert (cen["p"] < 1e3).any()
    assert (out16[:, :, 3:5] != 0.0).any() and (out16[:, :, 3:5] == 0.0).any()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the slots across launch forms, in wind
# ---------------------------------------------------------------------------------------------------------------------------
def _windy(case):
    from test_wind_axes import node_winds, small_problem
    from gelato_amd import Engine, problem
    prob, x0 = small_problem(case, "windy")
    E = Engine(prob, flags=1)
    X5 = problem.synthetic_batch(x0, E.M, 5, seed=13)
    assert all((node_winds(prob, x, E.M) != 0.0).all() for x in X5)
    return prob, X5


def _singles(E, X5):
    """the latency form, one vector at a time: COO-direct into the pinned arrays, and the callback -> [(res, compact values)]"""
    vidx = E.var_index()
    pres, pvals = E.pinned_buffers()
    assert E.launch_info(1)[2] == 1
    out = []
    for x in X5:
        r, v, rc = E.eval(x, out=pvals, res_out=pres)
        assert rc == 0
        out.append((r.copy(), v[vidx].copy()))
        cb = E.eval_callback(x, True)
        assert cb["rc"] == 0 and np.array_equal(bits(cb["res"]), bits(out[-1][0])) and np.array_equal(bits(cb["vals"][vidx]), bits(out[-1][1]))
    return out


def _batch_equals(E, X5, single, B):
    import torch
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    X = np.tile(X5, (B // 5 + 1, 1))[:B]
    dX = torch.from_numpy(X.copy()).to(dev)
    dres = torch.empty((B, E.nres), dtype=torch.float64, device=dev)
    djv = torch.empty((B, E.V), dtype=torch.float64, device=dev)
    E.eval_batch_device(B, dX.data_ptr(), dres.data_ptr(), djv.data_ptr(), s)
    assert E.sync(s) == 0
    res, jv = dres.cpu().numpy(), djv.cpu().numpy()
    for b in range(B):
        assert np.array_equal(bits(res[b]), bits(single[b % 5][0])) and np.array_equal(bits(jv[b]), bits(single[b % 5][1])), (B, b)
    return dX, dres, djv


@pytest.mark.parametrize("flags", [0, 8])
@pytest.mark.parametrize("case", ["3x8", "n5"])
def test_every_form_reads_the_same_slots_in_wind(case, flags):
    """flags 0: the difference form (kept 1/T and margin); flags 8: GEL_FLAG_FD_RECOMPUTE, whose t0 / tf columns come from
    wind_eci_chain()."""
    import torch
    from gelato_amd import Engine, parallel
    prob, X5 = _windy(case)
    Ep = Engine(prob, flags=1 | flags)          # matrix pipe; two vectors per wavefront in the throughput form
    E1 = Engine(prob, flags=1 | 4 | flags)      # GEL_FLAG_NO_PACK
    Bt = 1005
    assert Ep.launch_info(Bt)[2] == 0 and Ep.launch_info(Bt)[4] == 1 and E1.launch_info(Bt)[2] == 0 and E1.launch_info(Bt)[4] == 0
    single = _singles(Ep, X5)
    assert np.isfinite(single[0][0]).all() and np.isfinite(single[0][1]).all()
    for E in (Ep, E1):
        for B in (5, Bt):
            dX, dres, djv = _batch_equals(E, X5, single, B)
    # unit-sharded launches (unit = 4 * work item + part: one position sweep per wavefront), any disjoint cover: the same bits
    s = torch.cuda.current_stream().cuda_stream
    costs = parallel.unit_costs(E1)
    for world in (3, len(costs)):
        nan = float("nan")
        tot_r, tot_j = torch.full_like(dres, nan), torch.full_like(djv, nan)
        for b0, c in parallel.shard_chunks(costs, world):
            r, jv = torch.full_like(dres, nan), torch.full_like(djv, nan)
            E1.eval_shard_units_device(Bt, dX.data_ptr(), r.data_ptr(), jv.data_ptr(), b0, c, s)
            assert E1.sync(s) == 0
            assert not bool((~torch.isnan(tot_r) & ~torch.isnan(r)).any()) and not bool((~torch.isnan(tot_j) & ~torch.isnan(jv)).any())   # disjoint owners
            tot_r = torch.where(torch.isnan(r), tot_r, r)              # (not a sum: an entry may be -0)
            tot_j = torch.where(torch.isnan(jv), tot_j, jv)
        assert torch.equal(tot_r.view(torch.int64), dres.view(torch.int64)) and torch.equal(tot_j.view(torch.int64), djv.view(torch.int64)), world


@pytest.mark.parametrize("case", ["3x8", "n5"])
def test_flag_8_t_columns_keep_the_bits_they_had_with_the_parked_pair(case):
    """The t0 / tf sweeps of GEL_FLAG_FD_RECOMPUTE go through wind_eci_chain(), which forms the half-latitude pair itself since the
    position part stopped carrying it.  tests/golden/g37_flag8_t_columns_in_wind.npz holds the vel / t block as the last library that
    parked the pair wrote it (tests/golden/make_flag8_t_columns.py): the same bits now, in the latency form and in a batch -- a pair
    rounded otherwise (another operation order, a contraction) would move every form together and pass the cross-form test above."""
    import hashlib
    from conftest import load_golden
    from test_wind_axes import small_problem
    from gelato_amd import Engine
    g = load_golden("g37_flag8_t_columns_in_wind.npz")
    prob, x0 = small_problem(case, "windy")
    sha = np.frombuffer(hashlib.sha256(np.ascontiguousarray(x0, dtype=np.float64).tobytes()).digest(), dtype=np.uint8)
    assert np.array_equal(sha, g[case + "_x_sha256"]), "the fixture was recorded for another decision vector"
    E = Engine(prob, flags=1 | 8)
    _, vals, rc = E.eval(x0)
    assert rc == 0
    want = g[case + "_vel_t"]
    assert np.isfinite(want).all() and np.count_nonzero(want) > len(want) // 2
    got = E.jac_dicts(vals)["vel"]["t"]["coo"][2]
    d = bits(got) != bits(want)
    assert not d.any(), (int(d.sum()), np.argwhere(d)[:6].ravel(), got[d][:3], want[d][:3])
    _, jv, rcb = E.eval_batch(np.tile(x0, (300, 1)))
    assert rcb == 0 and np.array_equal(bits(E.jac_dicts(E.expand(jv[299]))["vel"]["t"]["coo"][2]), bits(want))


def test_fused_aero_launch_equals_aero_kernel_in_wind(monkeypatch):
    """B = 261 with GEL_FLAG_NO_PACK: the cooperative form with one vector per wavefront, where the aero rows ride in the fused kernel's
    lanes (their sweeps read 1/hypot from slot LV1) -- bit for bit gel_eval_batch_device + gel_eval_aero_all_device.  `3x8` only: aero
    specs name phases in [0, num_sections - 1), so the one-phase problem has no aero rows."""
    from gelato_amd import Engine
    from test_aero_engine import KINDS, check_fused_equals_two, fused_outputs
    prob, X5 = _windy("3x8")
    S = len(prob["num_nodes"])
    monkeypatch.setenv("GEL_AERO_FUSED", "1")                          # read when the handle is created
    E = Engine(prob, flags=4)
    for kind in KINDS:
        E.aero_configure(kind, [(i, 1, LIMS[kind]) for i in range(S - 1)])
    B = 261
    X = np.tile(X5, (B // 5 + 1, 1))[:B]
    one, two, layout = fused_outputs(E, X)
    check_fused_equals_two(E, one, two, layout)
    assert all(two["con"][k].size and np.isfinite(two["con"][k]).all() and np.isfinite(two["jac"][k]).all() for k in KINDS)
    assert any(np.abs(two["jac"][k]).max() > 0.0 for k in KINDS)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. a dropped lane
# ---------------------------------------------------------------------------------------------------------------------------
def test_covered_lanes_keep_their_bits_beside_a_dropped_lane():
    import states
    from gelato_amd import Engine
    from gelato_amd.dynamics import point_eval
    prob0, _ = states.layer_break_state()
    up = float(prob0["units"][1])
    step = float(np.float64(prob0["dx"]) * np.float64(up))
    prob, xb = states.layer_break_state(step=step)
    n = int(prob["num_nodes"][0])
    assert n == 60
    M = n + 1
    wind = np.ascontiguousarray(prob["wind_table"], dtype=np.float64)
    dx = float(prob["dx"])

    def covered(x):
        """[M, 3]: does the difference form cover sweep kk of state node i?  (point hook 15 on the kernel's own operands)"""
        re = x[M:4 * M].reshape(-1, 3)
        r = re * up
        ok = np.zeros((M, 3), dtype=bool)
        for kk in range(3):
            dlt = (re[:, kk] + dx) * up - r[:, kk]
            ok[:, kk] = point_eval(15, np.column_stack([r, np.full(M, float(kk)), dlt]), aux=wind)[:, 16] == 1.0
        return ok

    okb = covered(xb)
    dropped = ~okb.all(axis=1)
    dropped[0] = True                                   # state node 0 has no row of the velocity defect
    assert 4 <= np.count_nonzero(dropped[1:]) <= n - 8, "lanes on either side of the predicate"
    xm = xb.copy()
    pos = xm[M:4 * M].reshape(-1, 3)
    pos[dropped] *= (1.0 + 50.0 / (np.linalg.norm(pos[dropped], axis=1, keepdims=True) * up))
    assert covered(xm)[1:].all(), "moved off the breaks, no lane is dropped"
    rows = np.array([3 * (i - 1) + c for i in np.flatnonzero(~dropped) for c in range(3)])
    E = Engine(prob, flags=1 | 4)
    pres, pvals = E.pinned_buffers()

    def forms(x):
        """{form: full values}: latency (COO-direct), callback, a handful of vectors, the cooperative form"""
        out = {}
        _, v, rc = E.eval(x, out=pvals, res_out=pres)
        assert rc == 0
        out["latency"] = v.copy()
        cb = E.eval_callback(x, True)
        assert cb["rc"] == 0
        out["callback"] = cb["vals"].copy()
        for name, B in (("few", 3), ("coop", 300)):
            assert E.launch_info(B)[2] == (1 if name == "few" else 0)
            _, jv, rc = E.eval_batch(np.tile(x, (B, 1)))
            assert rc == 0
            out[name] = E.expand(jv[B - 1])
        return out

    fb, fm = forms(xb), forms(xm)
    for name in fb:
        assert np.array_equal(bits(fb[name]), bits(fb["latency"])) and np.array_equal(bits(fm[name]), bits(fm["latency"])), name
        Jb, Jm = E.jac_dicts(fb[name])["vel"], E.jac_dicts(fm[name])["vel"]
        compared = 0
        for var in Jb:
            rr, _, vb = Jb[var]["coo"]
            _, _, vm = Jm[var]["coo"]
            m = np.isin(rr, rows)
            assert np.array_equal(bits(vb[m]), bits(vm[m])), (name, var)
            compared += int(m.sum())
        assert compared > 100
    # the comparison is not blind: the moved nodes' own entries differ
    rr, _, vb = E.jac_dicts(fb["latency"])["vel"]["position"]["coo"]
    vm = E.jac_dicts(fm["latency"])["vel"]["position"]["coo"][2]
    assert not np.array_equal(vb[~np.isin(rr, rows)], vm[~np.isin(rr, rows)])

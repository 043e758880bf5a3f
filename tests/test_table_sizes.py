"""The kernels that read the wind and CA tables -- the fused kernel, the aero kernels, rhs_vel_air_kernel, mesh_kernel, output_kernel
and prop_kernel<false, false> here; prop_kernel's dispersed and chained instantiations in tests/test_table_sizes_flight.py; the
batched output table's outbatch_rows_kernel and outbatch_env_kernel in tests/test_table_sizes_outbatch.py (table_cases.TABLE_KERNELS
lists kernel by kernel which test runs it; tests/test_table_sizes_cpu.py holds the list to the sources) -- on small problems over
the tables of tests/table_cases.py (two rows; 32 | 33 rows:
the two branches of lower_count; 160 wind rows: several passes of every staging loop, both parities of the padded table size that
the regions behind the tables start at), under the comparisons the suite already makes for the same entry points on the example's
tables -- imported, not restated; no tolerance of its own.

Meshes (table_cases.MESHES; the last phase coasts without aerodynamics): "pack" (20, 31, 2) every phase within 32 nodes, two vectors
per wavefront; "coop" (40, 65, 2) the one-slab cooperative form, 107 constrained nodes (the flat aero mapping); "slab" (70, 5, 2) the
long-phase slab form.  Batch sizes are asked of the library (gel_launch_info, gel_aero_launch_info): B = 1 and 3 (the values-only
split / one tile per vector), and the first B past the split form plus one (cooperative forms, an incomplete last workgroup; the
flat aero mapping; where the mesh allows it the fused-AERO instantiation).  No B is above 512.

Nothing here launches with more than 64 KB of LDS: every case fits every launch (table_cases.check_case, on the CPU)."""
import numpy as np
import pytest

import exact_aero_truth as T
import states
import table_cases as TC

# The derived gradient bound carries the altitude's rounding (eps R = 1.4e-9 m) times the row's altitude sensitivity, which
# tests/fd_noise.py measures on the oracle over a radial step of 10 m: right for the example's tables (intervals of kilometres), an
# average over three intervals here (3 m apart, winds 10 m/s apart: a slope of 4 per second against 5e-3).  With 10 m alone one entry
# (LONG, (70, 5, 2), `knots`, alpha / position) lay 3.5e-3 outside an allowance of 2.0e-3 on an MI355X.  The same quotient of the
# same oracle is therefore also taken over 10 cm, 1 cm and 1 mm either way -- inside an interval, and across the knot that the
# 6.4 cm step of a `knots` node crosses; the largest counts.  Constants and formula are fd_noise's own.
SECANTS = (10.0, 0.1, -0.1, 0.01, -0.01, 0.001, -0.001)
PARAMS = [("LONG", "pack"), ("LONG", "coop"), ("LONG", "slab"), ("MIN", "coop"), ("EDGE32", "coop"), ("EDGE33", "coop"),
          ("LONGEVEN", "coop")]
_STATE = {}


def _state(case, mesh, vector):
    key = (case, mesh, vector)
    if key not in _STATE:
        _STATE[key] = states.table_state(case, TC.MESHES[mesh], vector)
    return _STATE[key]


@pytest.mark.parametrize("case,mesh", PARAMS)
def test_states_are_where_they_claim_to_be(case, mesh):
    """table_state's promises from the oracle's altitude and Mach number per node: below / inside / above both tables, a metre
    (1e-6 in Mach) off every knot but for the `knots` nodes, which sit 4 mm and 4 cm either side of theirs; on the (40, 65, 2) mesh
    the climb visits more than half of the wind and of the CA intervals, on the smaller ones a different wind interval per node"""
    wind, ca = TC.CASES[case]
    for vector in ("climb", "knots"):
        hit_w, hit_c = states.check_table_state(case, TC.MESHES[mesh], vector)
        nn = TC.MESHES[mesh]
        inside = sum(nn[:-1]) + len(nn) - 1 - 5 - (0 if vector == "climb" else 4 * len(states.table_knots(case)))
        if vector == "climb":
            assert hit_w >= min((len(wind) - 1 + 1) // 2, inside, len(wind) - 3), (case, mesh, hit_w)
            assert hit_c >= (len(ca) - 1 + 1) // 2, (case, mesh, hit_c)
        if (case, mesh, vector) == ("LONG", "coop", "climb"):
            assert hit_w >= 80 and hit_c >= 24


def _pair(prob, flags=0):
    from test_gpu_parity import make_pair
    return make_pair(prob, flags=flags)


def _batch_sizes(E):
    """1, 3 and the first batch past the split form plus one (not a multiple of the four / eight vectors of a workgroup)"""
    Bc = next(B for B in range(2, 512) if E.launch_info(B)[2] == 0) + 1
    assert E.launch_info(1)[2] == 1 and E.launch_info(3)[2] == 1 and E.launch_info(Bc)[2] == 0 and Bc % 4 and Bc <= 512
    return (1, 3, Bc)


def _batch(xs, B):
    """the vectors xs alternating, B of them"""
    return np.ascontiguousarray(np.stack([xs[b % len(xs)] for b in range(B)]))


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, 8])
@pytest.mark.parametrize("case,mesh", PARAMS)
def test_defect_groups_against_the_oracle_in_every_form(case, mesh, flags):
    """Residuals and the finite-difference Jacobian of `climb` by check_against_oracle as it stands, through gel_eval_residual /
    gel_eval_jacobian, Engine.eval (the COO-direct one-vector path), the callback (values only, then with derivatives) and
    gel_eval_batch_device in every form the launcher selects; residuals of `knots` against the oracle; and (flags 0, where
    test_cooperative_dx_form_equals_single_vector_calls and test_batch_matches_single_and_oracle assert it) every vector of
    every batch the bits of its one-vector call."""
    import torch
    from test_gpu_parity import check_against_oracle, close, dx_roundoff_bound
    import oracle
    prob, xc = _state(case, mesh, "climb")
    _p, xk = _state(case, mesh, "knots")
    E, P = _pair(prob, flags)
    what = "%s/%s/flags %d" % (case, mesh, flags)
    form = E.launch_info(300)
    assert form[4] == (1 if mesh == "pack" else 0), form
    res1, vals1 = check_against_oracle(E, P, xc, what + " one vector", prob=prob)
    r2, v2, rc = E.eval(xc)
    assert rc == 0
    check_against_oracle(E, P, xc, what + " gel_eval", prob=prob, res=r2, vals=v2)
    fr = E.eval_callback(xc, False)
    assert fr["rc"] == 0
    rcb = fr["res"].copy()
    fr = E.eval_callback(xc, True)
    assert fr["rc"] == 0 and np.array_equal(fr["res"], rcb)
    check_against_oracle(E, P, xc, what + " callback", prob=prob, res=rcb, vals=fr["vals"].copy())
    single = {}
    for name, x in (("climb", xc), ("knots", xk)):
        r, rc = E.eval_residual(x)
        v, rc2 = E.eval_jacobian(x)
        assert rc == 0 and rc2 == 0
        single[name] = (r, v[E.var_index()])
        R, bound = E.split_res(r), dx_roundoff_bound(E, x)
        for grp in oracle.GROUPS:
            close(R[grp], P.residual(grp, x), atol=1e-12 + bound[grp], what="%s %s residual %s" % (what, name, grp))
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    for B in _batch_sizes(E):
        X = _batch([xc, xk], B)
        dX = torch.from_numpy(X).to(dev)
        dres = torch.full((B + 1, E.nres), -7.0, dtype=torch.float64, device=dev)
        djv = torch.full((B + 1, E.V), -7.0, dtype=torch.float64, device=dev)
        dres2 = torch.full((B + 1, E.nres), -7.0, dtype=torch.float64, device=dev)
        E.eval_batch_device(B, dX.data_ptr(), dres.data_ptr(), djv.data_ptr(), s)
        E.eval_batch_device(B, dX.data_ptr(), dres2.data_ptr(), 0, s)
        assert E.sync(s) == 0
        res, jv, res2 = dres.cpu().numpy(), djv.cpu().numpy(), dres2.cpu().numpy()
        assert np.all(res[B] == -7.0) and np.all(jv[B] == -7.0) and np.all(res2[B] == -7.0), (what, B, "wrote behind the batch")
        assert np.array_equal(res, res2), (what, B, "residual-only launch")
        last_climb = (B - 1) - ((B - 1) % 2)
        check_against_oracle(E, P, xc, "%s B %d" % (what, B), prob=prob, res=res[last_climb], vals=E.expand(jv[last_climb]))
        if flags == 0:
            for b in range(B):
                r, v = single["knots" if b % 2 else "climb"]
                assert np.array_equal(res[b], r) and np.array_equal(jv[b], v), (what, B, b, E.launch_info(B))


def _aero_engine(prob, flags=0):
    import oracle
    from gelato_amd import Engine
    pt, D, _x = T._with_tau(prob, None)
    E = Engine(prob, D=D, tau=pt["tau"], flags=flags)
    P = oracle.Problem(prob, D=D, tau=pt["tau"])
    specs = T._all_aero(prob)
    for kind in T.KINDS:
        E.aero_configure(kind, specs[kind])
        P.aero_configure(kind, specs[kind])
    return E, P, pt, specs


@pytest.mark.gpu
@pytest.mark.parametrize("case,mesh", PARAMS)
def test_aero_kinds_dense_records_and_callback(case, mesh, monkeypatch):
    """The three aero kinds on every aerodynamic phase.  Against the oracle (test_aero_engine.check_kind_against_oracle: the
    assertions of test_aero_values_and_gradients_gpu), `climb` and `knots`, from the one-vector dense call.  Then bits: the callback
    form, the dense batch (one tile per vector at B = 1 and on the meshes without 64 constrained nodes, the flat mapping otherwise),
    and gel_eval_batch_aero_device's records with GEL_AERO_FUSED = 1 (the rows ride in the fused kernel where the batch takes the
    cooperative one-vector form; aero_kernel's spec-major part A otherwise) and = 0 -- each equal to the separate launches, as
    test_aero_engine's identity tests hold them for the named problems."""
    from test_aero_engine import check_fused_equals_two, check_kind_against_oracle, fused_outputs
    prob, xc = _state(case, mesh, "climb")
    _p, xk = _state(case, mesh, "knots")
    E, P, pt, specs = _aero_engine(prob)
    nnodes = E.aero_dims("alpha")[0]
    assert nnodes == sum(TC.MESHES[mesh][:-1]) + 2
    what = "%s/%s" % (case, mesh)
    one = {}
    for name, x in (("climb", xc), ("knots", xk)):
        con, jac, rc = E.eval_aero_all(x[None, :])
        assert rc == 0
        one[name] = (con, jac)
        unbounded = sum(check_kind_against_oracle(P, pt, x, kind, specs[kind], con[kind][0], jac[kind][0], what + " " + name, SECANTS)
                        for kind in T.KINDS)
        # entries without a finite bound are counted, not hidden (as test_aero_values_and_gradients_gpu does): they are the 12 + 8 + 12
        # entries of the nodes slower over the ground than the table's largest wind, whose air-relative speed may vanish (fd_noise)
        slow = int((states.table_oracle_rows(prob, x)["vel_ground"][:nnodes] <= np.abs(TC.CASES[case][0][:, 1:]).max()).sum())
        assert unbounded == 32 * slow and 5 * slow <= nnodes, (what, name, unbounded, slow)
        fr = E.eval_callback(x, True)
        assert fr["rc"] == 0
        for kind in T.KINDS:
            assert np.array_equal(fr["aero_con"][kind], con[kind][0]) and np.array_equal(fr["aero_jac"][kind], jac[kind][0]), (what, name, kind)
    Bs = _batch_sizes(E)
    # the form of the fused kernel at the largest batch: cooperative (matrix pipe, not split), two vectors per wavefront only on the
    # pack mesh -- on the others gel_eval_batch_aero_device's rows ride in the AERO instantiation (eval_aero_fusable) and the rows it
    # leaves (state node 0 of a phase) go to aero_wide_kernel; on the pack mesh and at B = 3 aero_sm_kernel writes the records
    form = E.launch_info(Bs[-1])
    assert form[:3] == [1, 1, 0] and form[4] == (1 if mesh == "pack" else 0) and E.launch_info(3)[2] == 1, (what, form)
    flat = [E.aero_launch_info(B)["flat"] for B in Bs]
    assert flat == ([0, 1, 1] if (nnodes >= 64 and nnodes % 64) else [0, 0, 0]), (what, nnodes, flat)
    for B in Bs[1:]:
        X = _batch([xc, xk], B)
        con, jac, rc = E.eval_aero_all(X)
        assert rc == 0
        for b in range(B):
            c1, j1 = one["knots" if b % 2 else "climb"]
            for kind in T.KINDS:
                assert np.array_equal(con[kind][b], c1[kind][0]) and np.array_equal(jac[kind][b], j1[kind][0]), (what, B, b, kind)
    from gelato_amd import Engine
    for fused in ("1", "0"):
        monkeypatch.setenv("GEL_AERO_FUSED", fused)               # read when the handle is created
        Ef = Engine(prob, D=[E.D(i) for i in range(E.S)], tau=pt["tau"])
        for kind in T.KINDS:
            Ef.aero_configure(kind, specs[kind])
        for B in Bs[1:]:
            o1, o2, layout = fused_outputs(Ef, _batch([xc, xk], B))
            check_fused_equals_two(Ef, o1, o2, layout)
            for kind in T.KINDS:                                  # and the separate launches are the dense calls above
                assert np.array_equal(o2["con"][kind][0], one["climb"][0][kind][0]) and np.array_equal(o2["jac"][kind][1], one["knots"][1][kind][0])


@pytest.mark.gpu
@pytest.mark.parametrize("case,mesh", PARAMS)
def test_velocity_rhs_of_every_phase(case, mesh):
    """dynamics.dynamics_velocity (rhs_vel_air_kernel: 64 threads stage the tables) on each phase's state nodes against the
    oracle's, as test_rhs_functions_vs_golden_and_oracle holds it"""
    import oracle
    from gelato_amd import dynamics
    from test_gpu_parity import close
    prob, xc = _state(case, mesh, "climb")
    _p, xk = _state(case, mesh, "knots")
    P = oracle.Problem(prob)
    units = prob["units"][:3]
    for name, x in (("climb", xc), ("knots", xk)):
        X = P.split_x(x)
        xa = 0
        for i, n in enumerate(int(v) for v in prob["num_nodes"]):
            xb = xa + n + 1
            pa = np.array([prob["thrust"][i], prob["massflow"][i], prob["reference_area"][i] or 2.21, 0, prob["nozzle_area"][i]])
            m_, p_, v_, q_ = (X["mass"][xa:xb], X["position"].reshape(-1, 3)[xa:xb], X["velocity"].reshape(-1, 3)[xa:xb],
                              X["quaternion"].reshape(-1, 4)[xa:xb])
            tn = np.concatenate([[X["t"][i]], P.tau(i) * (X["t"][i + 1] - X["t"][i]) / 2 + (X["t"][i + 1] + X["t"][i]) / 2])
            got = dynamics.dynamics_velocity(m_, p_, v_, q_, tn, pa, prob["wind_table"], prob["ca_table"], units, oracle.BARC20_CPP)
            ref = oracle.dynamics_velocity(m_, p_, v_, q_, tn, pa, prob["wind_table"], prob["ca_table"], units, oracle.BARC20_CPP)
            close(got, ref, what="%s/%s %s phase %d dynamics_velocity vs oracle" % (case, mesh, name, i))
            xa = xb


@pytest.mark.gpu
@pytest.mark.parametrize("case,mesh", PARAMS)
def test_mesh_error_and_propagation(case, mesh):
    """gel_mesh_error[_device] (mesh_kernel: 512 threads; its vectors' region starts behind the padded tables, and the vectors per
    workgroup of the two-node tail are what fits beside the tables) against mesh_truth under its bound; gel_propagate with k = 1 and 2
    RK4 steps per interval, both restart modes (prop_kernel), against propagate_truth under its bound -- both restatements take
    the tables from prob"""
    import torch
    import propagate_truth as pt
    from gelato_amd import Engine
    from test_mesh_error import check_parity as mesh_parity
    from test_propagate import check_parity as prop_parity
    prob, xc = _state(case, mesh, "climb")
    _p, xk = _state(case, mesh, "knots")
    E = Engine(prob)
    X = np.stack([xc, xk])
    use = mesh_parity(E, prob, X, "%s/%s" % (case, mesh))
    print("mesh bound usage %s/%s: err %s diff %s" % (case, mesh, np.array2string(use[0], precision=3), np.array2string(use[1], precision=3)))
    eh, dh, rc = E.mesh_error(X, want_diff=True)
    assert rc == 0
    B = 173                                                        # past the 170 vectors a workgroup of the tail could hold
    XX = _batch([xc, xk], B)
    dX = torch.from_numpy(XX).cuda()
    de = torch.empty((B, E.S, 4), dtype=torch.float64, device="cuda")
    dd = torch.empty((B, E.mesh_npts(), 11), dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    E.mesh_error_device(B, dX.data_ptr(), de.data_ptr(), dd.data_ptr(), s)
    assert E.sync(s) == 0
    de, dd = de.cpu().numpy(), dd.cpu().numpy()
    for b in range(B):
        assert np.array_equal(de[b], eh[b % 2]) and np.array_equal(dd[b], dh[b % 2]), (case, mesh, b)
    for k in (1, 2):
        for restart in (False, True):
            plan = E.propagation_plan(steps=k, restart="node" if restart else "section")
            ref = [pt.propagate_all(E, plan, prob, X[b], restart=restart) for b in range(2)]
            use, worst = prop_parity(E, plan, X, ref)
            plan.close()
            assert all(wy <= 1.0 and we <= 1.0 for wy, we in worst), (case, mesh, k, restart, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("case,mesh", PARAMS)
def test_output_table(case, mesh):
    """gel_output_table (output_kernel: 64 threads stage the tables) against the oracle's table on the same tables, under
    test_output_table.py's device tolerances.  The columns behind the wind lookup carry one more term, from the oracle alone: these
    tables have intervals of 3 m with winds 10 m/s apart (the example's: 2 km), so the wind moves by up to 8e-8 m/s within the
    2e-8 m the altitude column itself is allowed (it cancels 6.4e6 m: eps R = 1.4e-9 m of rounding in either implementation) --
    measured 8.6e-9 m/s on vel_air against a flat 1e-9.  The term is what the oracle's own column moves by when every node is
    raised or lowered by TOL["altitude"]; the other columns keep TOL as it is."""
    from gelato_amd import Engine
    from test_output_table import check_device_column
    prob, _xc = _state(case, mesh, "climb")
    E = Engine(prob)
    for vector in ("climb", "knots"):
        x = _state(case, mesh, vector)[1]
        tx = states.table_node_times(prob, x)
        Tt = states.table_oracle_rows(prob, x)
        extra = behind_the_wind_extra(prob, x, Tt)
        got = E.output_table(x, tx, 28.5, 0.0)
        for j, c in enumerate(E.OUTPUT_COLUMNS):
            check_device_column(c, got[:, j], ((Tt[c], "oracle"),), extra=extra[c])


BEHIND_THE_WIND = ("vel_air", "AOA_total", "AOA_pitch", "AOA_yaw", "dynamic_pressure", "Q_alpha", "M", "aero_BODY_X", "accel_BODY_X")


def behind_the_wind_extra(prob, x, Tt):
    """{column: the extra term of test_output_table's docstring}: what the oracle's own column (Tt = table_oracle_rows(prob, x))
    moves by when every node is raised or lowered by TOL["altitude"], for the columns behind the wind lookup; 0.0 for the others"""
    from test_output_table import TOL
    M = len(Tt["altitude"])
    moved = []
    for sign in (1.0, -1.0):
        xm = x.copy()
        r = xm[M:4 * M].reshape(-1, 3)
        r *= 1.0 + sign * TOL["altitude"][0] / (np.linalg.norm(r, axis=1, keepdims=True) * float(prob["units"][1]))
        moved.append(states.table_oracle_rows(prob, xm))
    return {c: (np.maximum(np.abs(moved[0][c] - Tt[c]), np.abs(moved[1][c] - Tt[c])) if c in BEHIND_THE_WIND else 0.0) for c in Tt}

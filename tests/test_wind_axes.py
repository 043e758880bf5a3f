"""GPU: the wind in ECI by the local north and east axes (gel_rhs_parts.h wind_eci()), the Earth angle on the polar axis only.

Off the axis the reference's chain quat_nedg2eci = conj(q_eci2ecef(t) * q_ecef2ned(Rz(-omega t) pos)) composes to
w = wn N + we E at the ECI longitude: the two rotations by omega t cancel and no time enters.  Exactly ON the axis the reference's
atan2(0, 0) = 0 makes the ECEF longitude 0, so the ECI longitude is omega t there -- the one place where the Earth angle is in the
result.  What is checked:

  1  the point hook against a 40-digit evaluation of the reference's chain, both poles at t != 0 included (drop the angle on the axis and
     this fails by metres per second);
  2  windy fused launches at the smallest shapes against the oracle, tolerances of tests/test_gpu_parity.py;
  3  windy nodes on and next to the axis against the oracle within the per-class bounds of tests/test_degenerate_fd.py, GEL_OK and finite
     on every output path, the fused AERO launch bit for bit as the two kernels;
  4  every launch form gives the same bits on a fully windy problem;
  5  a calm lane beside windy lanes gives the bits it gives in all-calm air.
No shape here is the workload's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LIMS = {"alpha": 0.2, "q": 4.0e4, "qalpha": 5.0e3}


def windy_table(top=700.0e3, rows=60):
    """never calm: both components are bounded away from zero at every altitude, clamped ends included (the pattern of
    test_single_phase_long_tables_other_units, carried above the top of every trajectory here so that the late nodes, where omega t is
    largest, are windy too; more than 32 rows: the binary-search branch of the look-up)"""
    alt = np.concatenate([[-1e8], np.linspace(0.0, top, rows), [1e10]])
    return np.column_stack([alt, 25.0 + 20.0 * np.sin(alt / 7e3), -(20.0 + 15.0 * np.cos(alt / 9e3))])


def small_problem(case, table):
    """-> (prob, x0): `3x8` / `3x16` of the package, or one phase of n = 5 nodes (not a multiple of four); the shipped wind table or
    windy_table()"""
    from test_gpu_parity import named_problem
    if case in ("3x8", "3x16"):
        prob, x0, _ = named_problem(case)
        prob = dict(prob)
    else:
        prob, _, _ = named_problem("example")
        prob = dict(prob)
        n = 5
        rng = np.random.default_rng(5)
        prob["num_nodes"] = np.array([n], dtype=np.int32)
        for k, v in [("thrust", 420000.0), ("massflow", 140.9), ("reference_area", 2.21), ("nozzle_area", 0.68)]:
            prob[k] = np.array([v])
        prob["engine_on"] = np.array([1], dtype=np.int32)
        prob["attitude_hold"] = np.array([0], dtype=np.int32)
        up, uv, ut = (float(prob["units"][k]) for k in (1, 2, 4))
        th = -0.6 + np.linspace(0, 0.02, n + 1)                           # southern hemisphere, cos lon < 0, y < 0
        R = (6378137.0 + np.linspace(800.0, 21e3, n + 1)) / up            # inside the measured part of the shipped table
        pos = np.column_stack([R * np.cos(th) * -0.8, R * np.cos(th) * -0.6, R * np.sin(th)])
        vel = np.column_stack([np.linspace(300.0, 1400.0, n + 1), np.linspace(600.0, 200.0, n + 1), np.linspace(100.0, 900.0, n + 1)]) / uv
        quat = rng.standard_normal((n + 1, 4))
        quat /= np.linalg.norm(quat, axis=1, keepdims=True)
        x0 = np.concatenate([np.linspace(1.0, 0.8, n + 1), pos.ravel(), vel.ravel(), quat.ravel(), 0.5 * rng.standard_normal(2 * n),
                             np.array([400.0, 520.0]) / ut])
    if table == "windy":
        prob["wind_table"] = windy_table()
    return prob, x0


def node_winds(prob, x, M):
    """wind (north, east) at every state node of x, by the engine's own point hooks: [M, 2]"""
    from gelato_amd.dynamics import point_eval
    r = x[M:4 * M].reshape(-1, 3) * float(prob["units"][1])
    alt = point_eval(1, r)[:, 2]
    return point_eval(5, alt, aux=np.ascontiguousarray(prob["wind_table"]))[:, :2]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the hook against the truth
# ---------------------------------------------------------------------------------------------------------------------------
def chain_truth(pos, t, wn, we):
    """quatrot(quat_ned2eci(pos, t), (wn, we, 0)) as the reference composes it (src/Coordinate.cpp:75-110,
    src/wrapper_coordinate.hpp:70-78), in 40-digit arithmetic on the fp64 inputs, with the Earth rate as the double the reference's
    C++ holds"""
    from mpmath import cos, mpf, sin, sqrt
    from oracle import exact_fd as X
    r, t = [X.f64(v) for v in pos], X.f64(t)
    om = X.OMEGA_F64
    c, s = cos(om * t), sin(om * t)
    pe = [r[0] * c + r[1] * s, -r[0] * s + r[1] * c, r[2]]          # eci2ecef
    lat, lon, _ = X.geodetic(*pe)                                     # atan2(0, 0) = 0 on the axis, as in C++
    cl, sl, cp, sp = cos(lon / 2), sin(lon / 2), cos(lat / 2), sin(lat / 2)
    rt2 = sqrt(mpf(2))
    q_e2n = [cl * (cp - sp) / rt2, sl * (cp + sp) / rt2, -cl * (cp + sp) / rt2, sl * (cp - sp) / rt2]
    q_i2e = [cos(om * t / 2), mpf(0), mpf(0), sin(om * t / 2)]
    q_n2i = X.conj(X.quatmult(q_i2e, q_e2n))
    return [float(v) for v in X.quatrot(q_n2i, [X.f64(wn), X.f64(we), mpf(0)])]


def hook_points():
    """[n, 6] rows pos (m), t (s), wn, we (m/s)"""
    RA, RB = 6378137.0, 6356752.314245
    rng = np.random.default_rng(7)
    times = (0.0, 597.0, 1.0e5)
    rows = []

    def at(p, lon, south, alt):
        z = RB * np.sqrt(max(1.0 - (p / RA) ** 2, 0.0)) + alt
        return [p * np.cos(lon), p * np.sin(lon), -z if south else z]
    k = 0
    for south in (False, True):                                       # both hemispheres x four quadrants x p = 1 mm .. 6400 km
        for lon in (0.3, 2.0, -2.5, -1.0):
            for p in np.geomspace(1e-3, 6.4e6, 8):
                mag, ang = rng.uniform(1.0, 100.0), rng.uniform(-np.pi, np.pi)
                rows.append(at(p, lon, south, 10e3 * (k % 4)) + [times[k % 3], mag * np.cos(ang), mag * np.sin(ang)])
                k += 1
    for south in (False, True):                                       # x = y = 0 at both poles, every time, each component alone and both
        for t in times:
            for wn, we in ((60.0, 0.0), (0.0, -45.0), (-70.0, 70.0)):
                rows.append([0.0, 0.0, (-1.0 if south else 1.0) * (RB + 5e3), t, wn, we])
    for i, lon in enumerate((0.0, np.pi / 2, np.pi, -np.pi / 2, 3.0, -3.0, 1.2, -0.2)):   # the cardinal longitudes; one component zero
        for south in (False, True):
            wn, we = ((0.0, 100.0), (-100.0, 0.0))[(i + south) % 2]
            rows.append(at(3.0e6 + 4.0e5 * i, lon, south, 20e3) + [times[(i + 1) % 3], wn, we])
    for t in times:                                                   # equator and a point one millimetre from the axis, no z offset
        rows.append([6378137.0 + 30e3, 0.0, 0.0, t, 33.0, -21.0])
        rows.append([0.0, -1e-3, RB + 100.0, t, 80.0, 60.0])
    return np.array(rows)


def test_wind_hook_against_the_reference_chain_in_40_digits():
    """point hook 3 (wind_eci() as every kernel calls it) on 104 points -- both hemispheres, the four quadrants, p from 1 mm to 6400 km,
    x = y = 0 at both poles with t = 0, 597 and 1e5 s, either component alone, |w| <= 100 m/s -- against chain_truth(), at the
    tolerance of test_point_functions_vs_oracle_and_golden (atol 1e-13).
    Measured on an MI355X: max |d| 5.7e-14 m/s off the axis, 2.8e-14 m/s on it (the quaternion chain this form replaced: 5.7e-14 /
    2.2e-14); with the Earth angle dropped on the axis the test fails by up to 100 m/s."""
    from gelato_amd.dynamics import point_eval
    from test_gpu_parity import close
    pts = hook_points()
    p = np.hypot(pts[:, 0], pts[:, 1])
    assert len(pts) >= 100 and np.count_nonzero(p == 0.0) == 18 and p[p > 0].min() <= 1e-3 and p.max() >= 6.39e6
    assert np.hypot(pts[:, 4], pts[:, 5]).max() <= 100.0 + 1e-9
    on = pts[p == 0.0]
    assert {(np.sign(z), t) for z, t in zip(on[:, 2], on[:, 3])} == {(s, t) for s in (-1.0, 1.0) for t in (0.0, 597.0, 1.0e5)}
    off = pts[p > 0]
    assert all(((np.sign(off[:, 0]) == a) & (np.sign(off[:, 1]) == b) & (np.sign(off[:, 2]) == c)).any()
               for a in (-1, 1) for b in (-1, 1) for c in (-1, 1))
    assert ((pts[:, 4] == 0) & (pts[:, 5] != 0)).any() and ((pts[:, 4] != 0) & (pts[:, 5] == 0)).any()
    ref = np.array([chain_truth(r[:3], r[3], r[4], r[5]) for r in pts])
    out = point_eval(3, pts)
    d = np.abs(out - ref).max(axis=1)
    print("wind hook against the 40-digit chain: max |d| %.3e m/s off the axis, %.3e m/s on it" % (d[p > 0].max(), d[p == 0].max()))
    # the truth itself has teeth on the axis: without the Earth angle there (longitude 0 instead of omega t) it is metres per second off
    blind = np.array([chain_truth(r[:3], 0.0, r[4], r[5]) for r in on])
    assert np.abs(blind - ref[p == 0.0]).max() > 1.0
    close(out, ref, atol=1e-13, what="wind NED->ECI against the 40-digit chain")


# ---------------------------------------------------------------------------------------------------------------------------
# 2. windy fused launches at the smallest shapes against the oracle
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 8])
@pytest.mark.parametrize("table", ["shipped", "windy"])
@pytest.mark.parametrize("case", ["3x8", "3x16", "n5"])
def test_windy_small_launches_against_the_oracle(case, table, flags):
    """B = 3 (a ragged group of the four-vector workgroup; matrix tiles that are mostly padding): residual rows, x-dependent values
    (1e-5 + 1e-6 |ref|) and constants (bit-exact) of every vector against the oracle -- check_against_oracle's tolerances -- with the
    default handle and GEL_FLAG_FD_RECOMPUTE, status GEL_OK.  `windy`: no node of any vector is in calm air."""
    from gelato_amd import problem
    from test_gpu_parity import check_against_oracle, make_pair
    prob, x0 = small_problem(case, table)
    E, P = make_pair(prob, flags=flags)
    X = problem.synthetic_batch(x0, E.M, 3, seed=31)
    if table == "windy":
        assert all((node_winds(prob, x, E.M) != 0.0).all() for x in X)
    else:
        assert (node_winds(prob, X[0], E.M) != 0.0).any()             # the shipped table is not calm everywhere either
    res, jv, rc = E.eval_batch(X)
    assert rc == 0
    r_only, _, rc2 = E.eval_batch(X, want_jac=False)                  # residual-only launches: always the cooperative form
    assert rc2 == 0 and np.array_equal(bits(r_only), bits(res))
    full = E.expand(jv)
    for b in range(3):
        check_against_oracle(E, P, X[b], "%s/%s flags %d vector %d" % (case, table, flags, b), res=res[b], vals=full[b])


# ---------------------------------------------------------------------------------------------------------------------------
# 3. windy nodes on and next to the polar axis
# ---------------------------------------------------------------------------------------------------------------------------
def axis_windy():
    """tests/states.py axis_state (nodes from 11 km off the axis down to exactly on it, both poles, 50 m .. 30 km, t = 10 .. 160 s) in a
    wind that is nowhere calm and has no break between its ends: one linear piece from the ground to 40 km"""
    import types
    import fd_noise
    import oracle
    import states
    from test_degenerate_fd import KINDS
    prob, x = states.axis_state()
    prob = dict(prob)
    prob["wind_table"] = np.array([[-1e8, 30.0, -25.0], [0.0, 30.0, -25.0], [40e3, -45.0, 55.0], [1e10, -45.0, 55.0]])
    P0 = oracle.Problem(prob)
    prob["tau"] = [P0.tau(i) for i in range(P0.S)]
    D = [P0.D(i) for i in range(P0.S)]
    P = oracle.Problem(prob, D=D, tau=prob["tau"])
    nn = [int(v) for v in prob["num_nodes"]]
    M = sum(nn) + len(nn)
    u, p = states.pos_delta_u(prob, x[M:4 * M].reshape(-1, 3))
    undecidable = p < 1.0 - 1e-9
    with np.errstate(invalid="ignore"):
        fallback = ~undecidable & (np.abs(u).max(axis=1) >= states.POS_DELTA_U)
    with np.errstate(all="ignore"):
        terms = fd_noise.velocity_noise_terms(oracle, prob, x)
    phases = [ph for ph in range(len(nn)) if terms[ph] is not None]
    for ph in phases:
        xa = sum(nn[:ph]) + ph
        terms[ph]["unchecked"] = undecidable[xa + 1:xa + 1 + nn[ph]]
        terms[ph]["fallback"] = fallback[xa + 1:xa + 1 + nn[ph]]
    specs = {k: [(ph, 1, LIMS[k]) for ph in phases] for k in KINDS}
    return types.SimpleNamespace(prob=prob, x=x, P=P, D=D, nn=nn, M=M, p=p, terms=terms, phases=phases, specs=specs, oracle=oracle)


@pytest.mark.parametrize("flags", [0, 8])
def test_windy_nodes_on_and_next_to_the_axis(flags, monkeypatch):
    """The velocity defect's Jacobian against the ORACLE's, per class as tests/test_degenerate_fd.py sorts the nodes: both are within
    their own bound of the exact quotient there (by_class / reference_bound for the engine, reference_bound for the oracle), hence
    within the SUM of the two of each other; the nodes fp64 cannot decide (p < 1 m, the axis itself) are held to status and
    finiteness like there.  Then every output path: GEL_OK (through gel_sync for the device-pointer calls), finite, the same bits;
    the fused AERO launch (B = 132: the cooperative form) bit for bit as aero_kernel and the plain fused kernel."""
    import torch
    import fd_noise
    from gelato_amd import Engine
    from test_degenerate_fd import KINDS, by_class, by_class_other, finite_ok, masked
    from test_exact_fd import VARS, block_entries, compare
    S = axis_windy()
    w = node_winds(S.prob, S.x, S.M)
    aero_nodes = np.concatenate([np.arange(sum(S.nn[:ph]) + ph, sum(S.nn[:ph]) + ph + S.nn[ph] + 1) for ph in S.phases])
    assert (w[aero_nodes] != 0.0).all() and np.count_nonzero(S.p[aero_nodes] == 0.0) >= 4 and S.x[-len(S.nn) - 1] > 0.0
    monkeypatch.setenv("GEL_AERO_FUSED", "1")
    E = Engine(S.prob, D=S.D, tau=S.prob["tau"], barC20=S.oracle.BARC20_CPP, flags=flags)
    for kind in KINDS:
        E.aero_configure(kind, S.specs[kind])
    vals, rc = E.eval_jacobian(S.x)
    assert finite_ok(rc, vals)
    J = E.jac_dicts(vals)["vel"]
    Jo = S.P.jacobian("vel", S.x)
    G = {"axisw_phases": np.array(S.phases)}
    for ph in S.phases:
        for var in VARS:
            ref = block_entries(Jo, S.prob, ph, var)
            if var == "velocity":
                for j in range(ref.shape[0]):
                    ref[j] -= np.eye(3) * S.P.D(ph)[j, j + 1]
            G["axisw_p%d_%s" % (ph, var)] = ref
    mine = (by_class, by_class_other) if flags == 0 else (fd_noise.reference_bound, fd_noise.reference_bound_other)
    worst = compare(J, G, "axisw", S.prob, S.P, S.terms, masked(lambda t: mine[0](t) + fd_noise.reference_bound(t)),
                    masked(lambda t: mine[1](t) + fd_noise.reference_bound_other(t)), "engine (flags %d) against the oracle" % flags)
    print("windy axis, flags %d: largest used fraction of the two bounds' sum per (phase, block): %s" % (
        flags, {k: round(float(v), 4) for k, v in worst.items()}))
    # every output path: GEL_OK, finite, the same bits
    res1, rc1 = E.eval_residual(S.x)
    res2, vals2, rc2 = E.eval(S.x)
    cb = E.eval_callback(S.x, True)
    resb, jvb, rcb = E.eval_batch(np.tile(S.x, (9, 1)))
    assert finite_ok(rc1, res1) and finite_ok(rc2, res2, vals2) and finite_ok(cb["rc"], cb["res"], cb["vals"]) and finite_ok(rcb, resb, jvb)
    assert np.array_equal(bits(vals2), bits(vals)) and np.array_equal(bits(cb["vals"]), bits(vals)) and np.array_equal(bits(E.expand(jvb[8])), bits(vals))
    assert np.array_equal(bits(res2), bits(res1)) and np.array_equal(bits(cb["res"]), bits(res1)) and np.array_equal(bits(resb[8]), bits(res1))
    B = 132          # 132 vectors x 2 work items x 4 > 1024 wavefronts: not the split latency form
    assert E.launch_info(B)[2] == 0
    X = np.tile(S.x, (B, 1))
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    dX = torch.from_numpy(X).to(dev)
    width, ocon, ojac = E.aero_record_layout()
    r1 = torch.empty((B, E.nres), dtype=torch.float64, device=dev)
    j1 = torch.empty((B, E.V), dtype=torch.float64, device=dev)
    a1 = torch.full((B, width), float("nan"), dtype=torch.float64, device=dev)
    E.eval_batch_aero_device(B, dX.data_ptr(), r1.data_ptr(), j1.data_ptr(), a1.data_ptr(), s)
    assert E.sync(s) == 0
    r0, j0 = torch.empty_like(r1), torch.empty_like(j1)
    E.eval_batch_device(B, dX.data_ptr(), r0.data_ptr(), j0.data_ptr(), s)
    assert E.sync(s) == 0
    assert torch.equal(r0.view(torch.int64), r1.view(torch.int64)) and torch.equal(j0.view(torch.int64), j1.view(torch.int64))
    assert bool(torch.isfinite(r0).all()) and bool(torch.isfinite(j0).all())
    assert np.array_equal(bits(r0[B - 1].cpu().numpy()), bits(res1)) and np.array_equal(bits(E.expand(j0[B - 1].cpu().numpy())), bits(vals))
    con, jac, rca = E.eval_aero_all(X)
    assert rca == 0
    a = a1.cpu().numpy()
    stored = np.unique(np.concatenate([idx[idx >= 0] for idx in list(ocon.values()) + list(ojac.values())]))
    assert np.isfinite(a[:, stored]).all()
    for kind in KINDS:
        one_c, one_j, rck = E.eval_aero(kind, S.x[None, :])
        assert finite_ok(rck, one_c, one_j), (kind, rck)
        assert np.array_equal(bits(E.aero_gather(a, ocon[kind])), bits(con[kind])) and np.array_equal(bits(E.aero_gather(a, ojac[kind])), bits(jac[kind])), kind
        assert np.array_equal(bits(con[kind][B - 1]), bits(one_c[0])) and np.array_equal(bits(jac[kind][B - 1]), bits(one_j[0])), kind
        assert np.array_equal(bits(cb["aero_con"][kind]), bits(one_c[0])) and np.array_equal(bits(cb["aero_jac"][kind]), bits(one_j[0])), kind


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the forms agree bit for bit on a fully windy problem
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["3x8", "3x16"])
def test_every_form_gives_the_same_bits_in_wind(case):
    """Five distinct decision vectors, no node in calm air: the latency form with COO-direct output (one-vector calls into the handle's
    pinned arrays) and the callback; the batch of five; and the five tiled to 1005 rows in the throughput form with two vectors per
    wavefront and (GEL_FLAG_NO_PACK) with one -- residual rows and compact values, the same bits everywhere (the comparisons of
    test_two_vectors_per_wavefront_equal_one_vector_per_wavefront and test_coo_direct_one_vector_output_equals_the_compact_path)."""
    import torch
    from gelato_amd import Engine, problem
    prob, x0 = small_problem(case, "windy")
    Ep = Engine(prob, flags=1)          # matrix pipe; two vectors per wavefront in the throughput form
    E1 = Engine(prob, flags=1 | 4)      # GEL_FLAG_NO_PACK
    X5 = problem.synthetic_batch(x0, Ep.M, 5, seed=13)
    assert all((node_winds(prob, x, Ep.M) != 0.0).all() for x in X5)
    Bt = 1005
    assert Ep.launch_info(Bt)[2] == 0 and Ep.launch_info(Bt)[4] == 1 and E1.launch_info(Bt)[2] == 0 and E1.launch_info(Bt)[4] == 0
    assert Ep.launch_info(1)[2] == 1
    vidx = Ep.var_index()
    pres, pvals = Ep.pinned_buffers()
    single = []
    for b in range(5):
        r, v, rc = Ep.eval(X5[b], out=pvals, res_out=pres)              # split latency form, COO-direct
        assert rc == 0
        single.append((r.copy(), v[vidx].copy()))
        cb = Ep.eval_callback(X5[b], True)
        assert cb["rc"] == 0 and np.array_equal(bits(cb["res"]), bits(single[b][0])) and np.array_equal(bits(cb["vals"][vidx]), bits(single[b][1]))
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    for E in (Ep, E1):
        for B in (5, Bt):
            X = np.tile(X5, (B // 5 + 1, 1))[:B]
            dX = torch.from_numpy(X.copy()).to(dev)
            dres = torch.full((B + 1, E.nres), -7.0, dtype=torch.float64, device=dev)
            djv = torch.full((B + 1, E.V), -7.0, dtype=torch.float64, device=dev)
            E.eval_batch_device(B, dX.data_ptr(), dres.data_ptr(), djv.data_ptr(), s)
            assert E.sync(s) == 0
            res, jv = dres.cpu().numpy(), djv.cpu().numpy()
            assert np.all(res[B] == -7.0) and np.all(jv[B] == -7.0)
            for b in range(B):
                assert np.array_equal(bits(res[b]), bits(single[b % 5][0])) and np.array_equal(bits(jv[b]), bits(single[b % 5][1])), (B, b)


@pytest.mark.parametrize("flags,B", [(0, 5), (4, 5), (4, 261)])
@pytest.mark.parametrize("case", ["3x8", "3x16"])
def test_fused_aero_call_equals_the_two_kernels_in_wind(case, flags, B, monkeypatch):
    """gel_eval_batch_aero_device with GEL_AERO_FUSED=1 and =0 on the fully windy problem: each the bits of gel_eval_batch_device +
    gel_eval_aero_all_device (check_fused_equals_two of tests/test_aero_engine.py), and the same record cells from both handles.
    B = 5: a handful of vectors; GEL_FLAG_NO_PACK at B = 261: the cooperative form with one vector per wavefront, where the aero rows
    ride in the fused kernel's lanes."""
    from gelato_amd import Engine, problem
    from test_aero_engine import KINDS, check_fused_equals_two, fused_outputs
    prob, x0 = small_problem(case, "windy")
    S = len(prob["num_nodes"])
    got = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("GEL_AERO_FUSED", fused)                    # read when the handle is created
        E = Engine(prob, flags=flags)
        for kind in KINDS:
            E.aero_configure(kind, [(i, 1, LIMS[kind]) for i in range(S - 1)])
        X5 = problem.synthetic_batch(x0, E.M, 5, seed=13)
        X = np.tile(X5, (B // 5 + 1, 1))[:B]
        one, two, layout = fused_outputs(E, X)
        check_fused_equals_two(E, one, two, layout)
        assert all(np.isfinite(two["con"][k]).all() and np.isfinite(two["jac"][k]).all() for k in KINDS)
        got[fused] = (E, one, layout)
    (Ea, a, la), (Eb, b, lb) = got["1"], got["0"]
    assert np.array_equal(bits(a["res"]), bits(b["res"])) and np.array_equal(bits(a["jvar"]), bits(b["jvar"]))
    for kind in KINDS:
        assert np.array_equal(bits(Ea.aero_gather(a["aero"], la[1][kind])), bits(Eb.aero_gather(b["aero"], lb[1][kind]))), kind
        assert np.array_equal(bits(Ea.aero_gather(a["aero"], la[2][kind])), bits(Eb.aero_gather(b["aero"], lb[2][kind]))), kind


# ---------------------------------------------------------------------------------------------------------------------------
# 5. a lane does not see its neighbours
# ---------------------------------------------------------------------------------------------------------------------------
def test_a_calm_lane_beside_windy_lanes_gives_the_bits_of_all_calm_air():
    """`3x16`, one decision vector, a wind table that is windy below 8 km, falls to EXACTLY zero at 12 km and stays there: phase 1
    (one wavefront) holds windy and calm nodes.  With the calm-air shortcut the all-calm wavefront gets w = +0; beside a windy lane the
    calm lane runs the formula, whose products with wn = we = 0 may be -0.  The outputs cannot tell: v - omega x r - (+-0) is the same
    number either way, so the calm nodes' rows of the velocity group -- residual rows and every Jacobian value -- are the bits of the
    launch with the same table's knots and all-zero winds (the same knots: the same pieces and margins for the difference form)."""
    from gelato_amd import Engine
    from test_gpu_parity import named_problem
    prob, x0, _ = named_problem("3x16")
    knots = np.array([-1e8, 0.0, 4e3, 8e3, 12e3, 300e3, 1e10])
    mixed = np.column_stack([knots, [18.0, 18.0, -30.0, 22.0, 0.0, 0.0, 0.0], [-12.0, -12.0, 26.0, -35.0, 0.0, 0.0, 0.0]])
    calm = np.column_stack([knots, np.zeros((len(knots), 2))])
    out = {}
    for name, W in (("mixed", mixed), ("calm", calm)):
        pr = dict(prob)
        pr["wind_table"] = W
        E = Engine(pr)
        res, vals, rc = E.eval(x0)
        assert rc == 0
        out[name] = (E.split_res(res)["vel"], E.jac_dicts(vals)["vel"])
    pr = dict(prob)
    pr["wind_table"] = mixed
    M = E.M
    w = node_winds(pr, x0, M)
    r = x0[M:4 * M].reshape(-1, 3) * float(prob["units"][1])
    from gelato_amd.dynamics import point_eval
    alt = point_eval(1, r)[:, 2]
    nn = [int(v) for v in prob["num_nodes"]]
    calm_rows, found = [], False
    for ph, n in enumerate(nn):
        xa, ua = sum(nn[:ph]) + ph, sum(nn[:ph])
        nodes = np.arange(xa + 1, xa + 1 + n)                          # the collocation nodes of the velocity defect
        is_calm = (w[nodes] == 0.0).all(axis=1) & (alt[nodes] > 12e3 + 1.0)   # and every perturbed point of theirs (steps of 6.4 cm)
        is_windy = (w[nodes] != 0.0).any(axis=1)
        found |= bool(is_calm.any() and is_windy.any())
        calm_rows += [3 * (ua + j) + c for j in np.flatnonzero(is_calm) for c in range(3)]
    assert found, "no phase holds calm and windy nodes at once"
    calm_rows = np.array(calm_rows)
    assert np.array_equal(bits(out["mixed"][0][calm_rows]), bits(out["calm"][0][calm_rows]))
    compared = 0
    for var in out["mixed"][1]:
        rr, cc, va = out["mixed"][1][var]["coo"]
        _, _, vb = out["calm"][1][var]["coo"]
        m = np.isin(rr, calm_rows)
        assert np.array_equal(bits(va[m]), bits(vb[m])), var
        compared += int(m.sum())
    assert compared > 100
    # ... and the windy nodes do differ: the comparison is not blind
    assert not np.array_equal(out["mixed"][0], out["calm"][0])

"""Spectral interpolation, host side (no GPU; host-only handles): the plans' matrices against a 50-digit ground truth and by
exactness on polynomials, the copy rule, the host product against its own matrices in longdouble, anchors on the manufactured
solution of g24, round trips, unit quaternions, interp.refine / interp.sample, and the argument checks."""
import ctypes as C

import numpy as np
import pytest
from numpy.polynomial import chebyshev as cheb

import interp_truth as it
from conftest import load_golden
from interp_truth import LD, U, gamma

PAIRS = [(3, 5), (5, 3), (8, 12), (64, 80), (128, 64), (64, 64)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_matrices_match_50_digit_truth():
    g = load_golden("g25_interp_matrices.npz")
    assert [tuple(int(v) for v in p) for p in g["pairs"]] == PAIRS
    for a, b in PAIRS:
        Ea, Eb = it.engine(it.prob_of([a])), it.engine(it.prob_of([b]))
        assert np.array_equal(Ea.tau(0), g["tau_%d" % a]) and np.array_equal(Eb.tau(0), g["tau_%d" % b])
        plan = Ea.transfer_plan(Eb)
        info = plan.info()
        assert (info["S"], info["mode"], info["state_rows"], info["out_doubles"], info["src_nvars"]) == (1, 1, b + 1, Eb.nvars, Ea.nvars)
        m = plan.matrices(0)
        tx_a, tx_b = np.concatenate([[-1.0], Ea.tau(0)]), np.concatenate([[-1.0], Eb.tau(0)])
        for k, sup, pts in (("Wx", tx_a, tx_b), ("Wu", Ea.tau(0), Eb.tau(0))):
            ref = g["%s_%d_%d" % (k, a, b)]
            assert m[k].shape == ref.shape
            row = np.abs(ref).max(axis=1, keepdims=True)
            assert np.all(np.abs(m[k] - ref) <= 1e-13 * row), (a, b, k, float((np.abs(m[k] - ref) / row).max()))
            # copies mark exactly the coincident points, with the support index
            want = np.array([int(np.flatnonzero(sup == z)[0]) if np.any(sup == z) else -1 for z in pts])
            assert np.array_equal(m["copy_" + k[1]], want), (a, b, k)
            hit = want >= 0
            assert np.array_equal(m[k][hit], np.eye(len(sup))[want[hit]])
        assert m["copy_x"][0] == 0 and m["copy_x"][-1] == a and m["copy_u"][-1] == a - 1
    # table mode
    n = int(g["table_n"])
    E = it.engine(it.prob_of([n]))
    pts = g["table_pts"]
    plan = E.interp_plan([pts])
    assert plan.info()["mode"] == 0 and plan.info()["state_rows"] == len(pts) and plan.info()["out_doubles"] == 14 * len(pts)
    m = plan.matrices(0)
    for k in ("Wx", "Wu"):
        ref = g["table_" + k]
        row = np.abs(ref).max(axis=1, keepdims=True)
        assert np.all(np.abs(m[k] - ref) <= 1e-13 * row), (k, float((np.abs(m[k] - ref) / row).max()))
    tau = E.tau(0)
    assert list(m["copy_x"]) == [0, n, 4, -1, -1, -1, -1, 1, -1, -1]
    assert list(m["copy_u"]) == [-1, n - 1, 3, -1, -1, -1, -1, 0, -1, -1]
    assert pts[2] == tau[3] and pts[7] == tau[0]


@pytest.mark.parametrize("a,b", PAIRS)
def test_copies_keep_their_bits(a, b):
    """first and last state node of every section and all of t keep their bits; 64 -> 64 is the identity, signed zero included;
    a NaN at an interior node of one vector reaches neither its copied entries nor the other vectors"""
    Ea, Eb = it.engine(it.prob_of([a, a])), it.engine(it.prob_of([b, b]))
    plan = Ea.transfer_plan(Eb)
    X = np.stack([it.random_x(Ea, s) for s in range(3)])
    X[0, 0] = -0.0                       # mass of the first knot
    X[1, Ea.M + 3 * (a + 1)] = -0.0      # position x of the second section's first node
    out, rc = plan.apply_host(X)
    assert rc == 0 and out.shape == (3, Eb.nvars)

    def knots(E, Y):
        n = int(E.num_nodes[0])
        rows = [0, n, n + 1, 2 * n + 1]
        M = E.M
        cols = ([r for r in rows] + [M + 3 * r + c for r in rows for c in range(3)] + [4 * M + 3 * r + c for r in rows for c in range(3)]
                + [7 * M + 4 * r + c for r in rows for c in range(4)] + list(range(11 * M + 2 * E.N, E.nvars)))
        return _bits(Y[:, cols])

    assert np.array_equal(knots(Ea, X), knots(Eb, out))
    assert np.signbit(out[0, 0]) and np.signbit(out[1, Eb.M + 3 * (b + 1)])
    if a == b:
        assert np.array_equal(_bits(out), _bits(X))
    Xn = X.copy()
    Xn[1, Ea.M + 3 * 2 + 1] = np.nan     # position y of interior node 2 of section 0
    outn, rc = plan.apply_host(Xn)
    assert rc == 1
    assert np.array_equal(_bits(outn[[0, 2]]), _bits(out[[0, 2]]))
    assert np.array_equal(knots(Eb, outn), knots(Eb, out))
    if a == b:
        assert np.array_equal(_bits(outn), _bits(Xn))


@pytest.mark.parametrize("a,b", [(128, 96), (64, 80)])
def test_matrices_exact_on_polynomials(a, b):
    """T_k of degree <= n_s on the state support and <= n_s - 1 on the control support arrive as T_k at the destination points;
    the bound of the mesh matrices' test: 64 u (k + 1) (sum_i |W_li| + 1)"""
    Ea, Eb = it.engine(it.prob_of([a])), it.engine(it.prob_of([b]))
    m = Ea.transfer_plan(Eb).matrices(0)
    tx_a, tx_b = np.concatenate([[-1.0], Ea.tau(0)]), np.concatenate([[-1.0], Eb.tau(0)])
    tol = 64 * U
    worst = [0.0, 0.0]
    for k in range(a + 1):
        c = np.zeros(k + 1)
        c[k] = 1.0
        got, ref = m["Wx"] @ cheb.chebval(tx_a, c), cheb.chebval(tx_b, c)
        bd = tol * (k + 1) * (np.abs(m["Wx"]).sum(axis=1) + 1)
        worst[0] = max(worst[0], float((np.abs(got - ref) / bd).max()))
        assert np.all(np.abs(got - ref) <= bd), ("Wx", k)
        if k <= a - 1:
            got, ref = m["Wu"] @ cheb.chebval(Ea.tau(0), c), cheb.chebval(Eb.tau(0), c)
            bd = tol * (k + 1) * (np.abs(m["Wu"]).sum(axis=1) + 1)
            worst[1] = max(worst[1], float((np.abs(got - ref) / bd).max()))
            assert np.all(np.abs(got - ref) <= bd), ("Wu", k)
    print("polynomial exactness %d -> %d: share of the bound used Wx %.3f Wu %.3f; Lebesgue constants %.2f / %.2f"
          % (a, b, worst[0], worst[1], np.abs(m["Wx"]).sum(axis=1).max(), np.abs(m["Wu"]).sum(axis=1).max()))


@pytest.mark.parametrize("name", ["example", "mixed-6x64", "stress-12x128", "ragged"])
def test_host_product_parity(name):
    """gel_interp_host against W @ X in longdouble from the plan's own matrices: |out - ref| <= gamma_{n_s + 2} (|W| |X|), in
    transfer mode (packed destination: every row at its place) and in table mode"""
    from gelato_amd import problem
    prob, x0 = it.named(name)
    E = it.engine(prob)
    nn = [int(v) for v in E.num_nodes]
    Ed = it.engine(it.with_nodes(prob, it.targets(name, nn)))
    X = problem.synthetic_batch(x0, E.M, 3)
    plan = E.transfer_plan(Ed)
    out, rc = plan.apply_host(X)
    assert rc == 0
    use = 0.0
    for b in range(3):
        ref, sc, cp = it.reference(plan, E, X[b])
        err = np.abs(out[b].astype(LD) - ref).astype(float)
        assert np.array_equal(_bits(out[b][cp]), _bits(ref[cp].astype(float)))
        # per phase gamma: lay gamma_{n_s + 2} out like the destination
        gs = it.pack([np.full((nd + 1, 11), gamma(n + 2)) for n, nd in zip(nn, Ed.num_nodes)],
                     [np.full((nd, 2), gamma(n + 2)) for n, nd in zip(nn, Ed.num_nodes)], np.zeros(E.S + 1))
        assert np.all(err <= gs * sc), (name, b, float((err[~cp] / (gs * sc)[~cp]).max()))
        if np.any(~cp & (sc > 0)):
            k = ~cp & (sc > 0)
            use = max(use, float((err[k] / (gs * sc)[k]).max()))
    rng = np.random.default_rng(5)
    pts = [np.concatenate([[-1.0, 1.0], rng.uniform(-1, 1, 7)]) for _ in nn]
    tplan = E.interp_plan(pts)
    tout, rc = tplan.apply_host(X)
    assert rc == 0 and tout.shape == (3, 9 * E.S, 14)
    for b in range(3):
        ref, sc, cp = it.reference(tplan, E, X[b])
        err = np.abs(tout[b].astype(LD) - ref).astype(float)
        gs = np.repeat([gamma(n + 2) for n in nn], 9)[:, None]
        assert np.all(err[:, 1:] <= (gs * sc)[:, 1:]), (name, b)
        assert np.array_equal(_bits(tout[b][:, 0]), _bits(it.table_times(pts, E, X[b])))
        k = ~cp & (sc > 0)
        use = max(use, float((err[k] / (gs * sc)[k]).max()))
    print("host product parity %s: largest share of the bound used %.3f" % (name, use))


def _g24_case(g, n):
    prob = {k[len("prob_noair_"):]: g[k] for k in g if k.startswith("prob_noair_")}
    prob["num_nodes"] = np.array([n], dtype=np.int32)
    return prob, g["x_noair_%d" % n], g["true_noair_%d" % n]


def test_anchors_on_manufactured_solution():
    """NoAir n -> n + 1: the transferred states are Lx @ X of the mesh estimate (independent matrices, pinned by g23) plus row 0;
    their deviation from the DOP853 truth falls strictly with n and is below 1e-11 at n = 12 and 16, where linear resampling of
    the same vectors misses 1e-4 at every n"""
    from mesh_truth import phase_state
    g = load_golden("g24_mesh_truth.npz")
    ns = [int(v) for v in g["ns"]]
    assert ns == [3, 5, 8, 12, 16]
    dev, lin = [], []
    for n in ns:
        prob, x, true = _g24_case(g, n)
        E, Ed = it.engine(prob), it.engine(it.with_nodes(prob, [n + 1]))
        out, rc = E.transfer_plan(Ed).apply_host(x)
        assert rc == 0
        Xd, _u, _to, _tf = phase_state(Ed, out[0], 0)
        X, _u, _to, _tf = phase_state(E, x, 0)
        Lx = E.mesh_matrices(0)["Lx"]
        assert np.array_equal(_bits(Xd[0]), _bits(X[0]))
        assert np.all(np.abs(Xd[1:] - Lx @ X) <= 2 * gamma(n + 2) * (np.abs(Lx) @ np.abs(X))), n
        den = 1.0 + np.abs(Xd).max(axis=0)
        dev.append(float((np.abs(Xd - true) / den).max()))
        tx, txd = np.concatenate([[-1.0], E.tau(0)]), np.concatenate([[-1.0], Ed.tau(0)])
        Xl = np.stack([np.interp(txd, tx, X[:, c]) for c in range(11)], axis=1)
        lin.append(float((np.abs(Xl - true) / den).max()))
    print("deviation from the truth by n:", ["%.1e" % v for v in dev], " linear resampling:", ["%.1e" % v for v in lin])
    assert all(b < a for a, b in zip(dev, dev[1:])), dev
    assert dev[3] <= 1e-11 and dev[4] <= 1e-11
    assert all(v > 1e-4 for v in lin), lin


@pytest.mark.parametrize("a,b", [(5, 8), (16, 24), (64, 80)])
def test_round_trip(a, b):
    """down(up(x)) = x within (gamma_{n_s + 2} + gamma_{n_d + 2} + 2e-13) (|W_dn| |W_up| |X|): two rounded products and two
    matrices, each within 1e-13 of the exact one (test 1's bound)"""
    from mesh_truth import phase_state
    Ea, Eb = it.engine(it.prob_of([a, a])), it.engine(it.prob_of([b, b]))
    up, dn = Ea.transfer_plan(Eb), Eb.transfer_plan(Ea)
    x = it.random_x(Ea, 7)
    y, rc = up.apply_host(x)
    z, rc2 = dn.apply_host(y[0])
    assert rc == 0 and rc2 == 0
    f = gamma(a + 2) + gamma(b + 2) + 2e-13
    tn = x.size - 3
    assert np.array_equal(_bits(z[0, tn:]), _bits(x[tn:]))
    for s in range(2):
        mu, md = up.matrices(s), dn.matrices(s)
        X, Uc, _to, _tf = phase_state(Ea, x, s)
        Z, Zu, _to, _tf = phase_state(Ea, z[0], s)
        assert np.all(np.abs(Z - X) <= f * (np.abs(md["Wx"]) @ np.abs(mu["Wx"]) @ np.abs(X)))
        assert np.all(np.abs(Zu - Uc) <= f * (np.abs(md["Wu"]) @ np.abs(mu["Wu"]) @ np.abs(Uc)))
        print("round trip %d <-> %d section %d: |W_dn W_up - I| %.1e / %.1e" % (
            a, b, s, np.abs(md["Wx"] @ mu["Wx"] - np.eye(a + 1)).max(), np.abs(md["Wu"] @ mu["Wu"] - np.eye(a)).max()))


def test_unit_quaternions():
    """GEL_INTERP_UNIT_QUAT: rows that are not copies carry q_lin / |q_lin| within 6 u |q| (the fma chain's 4 roundings on a sum
    of positive terms, the square root's and the division's; reference in longdouble), copy rows and everything but the
    quaternion are the unflagged run's bits"""
    prob, x0 = it.named("example")
    E = it.engine(prob)
    nn = [int(v) for v in E.num_nodes]
    Ed = it.engine(it.with_nodes(prob, [n + 2 for n in nn]))
    from gelato_amd import problem
    X = problem.synthetic_batch(x0, E.M, 2)
    lin, rc = E.transfer_plan(Ed).apply_host(X)
    plan = E.transfer_plan(Ed, unit_quat=True)
    unit, rc2 = plan.apply_host(X)
    assert rc == 0 and rc2 == 0
    qs = it.quat_slice(Ed)
    other = np.ones(Ed.nvars, dtype=bool)
    other[qs] = False
    assert np.array_equal(_bits(unit[:, other]), _bits(lin[:, other]))
    cpx = np.concatenate([plan.matrices(s)["copy_x"] >= 0 for s in range(E.S)])
    assert cpx.sum() == 2 * E.S
    ql, qu = lin[:, qs].reshape(2, -1, 4), unit[:, qs].reshape(2, -1, 4)
    assert np.array_equal(_bits(qu[:, cpx]), _bits(ql[:, cpx]))
    qL = ql.astype(LD)
    ref = qL / np.sqrt((qL * qL).sum(axis=2, keepdims=True))
    err = np.abs(qu.astype(LD) - ref).astype(float)
    assert np.all(err[:, ~cpx] <= 6 * U * np.abs(ref[:, ~cpx]).astype(float))
    assert np.all(np.abs(np.linalg.norm(qu[:, ~cpx], axis=2) - 1.0) <= 12 * U)   # 6 u from the components, the rest numpy's own norm
    assert not np.array_equal(qu[:, ~cpx], ql[:, ~cpx])
    # table mode takes the flag as well
    pts = [np.array([-1.0, 0.1, 1.0])] * E.S
    tl, _rc = E.interp_plan(pts).apply_host(X)
    tu, _rc = E.interp_plan(pts, unit_quat=True).apply_host(X)
    assert np.array_equal(_bits(tu[:, :, :8]), _bits(tl[:, :, :8])) and np.array_equal(_bits(tu[:, :, 12:]), _bits(tl[:, :, 12:]))
    assert np.array_equal(_bits(tu[:, 0::3, 8:12]), _bits(tl[:, 0::3, 8:12])) and np.array_equal(_bits(tu[:, 2::3, 8:12]), _bits(tl[:, 2::3, 8:12]))
    q = tl[:, 1::3, 8:12].astype(LD)
    ref = q / np.sqrt((q * q).sum(axis=2, keepdims=True))
    assert np.all(np.abs(tu[:, 1::3, 8:12].astype(LD) - ref).astype(float) <= 6 * U * np.abs(ref).astype(float))


def test_refine_and_sample():
    from gelato_amd import Engine, con_dynamics, interp, pack_x, problem
    from gelato_amd.SectionParameters import PSparams
    pdict, unitdict, _c, xdict = problem.make_problem("example")
    pdict["_gelato_amd"] = object()          # what the constraint mirrors cache in pdict
    S = pdict["num_sections"]
    nn = [pdict["ps_params"].nodes(i) for i in range(S)]
    keys0, ps0 = sorted(pdict), pdict["ps_params"]
    x_before = {k: np.array(v) for k, v in xdict.items()}
    new = [n + (3 if i % 2 == 0 else 0) for i, n in enumerate(nn)]
    recs = [{"name": pdict["params"][i]["name"], "num_nodes": n, "max": 0.0, "suggested": m, "action": "raised" if m > n else "kept"}
            for i, (n, m) in enumerate(zip(nn, new))]
    xn, pn = interp.refine(xdict, pdict, unitdict, recs)
    N = sum(new)
    assert pn["N"] == N and pn["M"] == N + S and pn["num_sections"] == S
    assert isinstance(pn["ps_params"], PSparams) and [pn["ps_params"].nodes(i) for i in range(S)] == new
    assert "_gelato_amd" not in pn and pn["params"] is pdict["params"]
    assert {k: v.shape for k, v in xn.items()} == {"mass": (N + S,), "position": (3 * (N + S),), "velocity": (3 * (N + S),),
                                                     "quaternion": (4 * (N + S),), "u": (2 * N,), "t": (S + 1,)}
    # the inputs are untouched
    assert sorted(pdict) == keys0 and pdict["ps_params"] is ps0 and pdict["N"] == sum(nn) and "_gelato_amd" in pdict
    assert all(np.array_equal(_bits(xdict[k]), _bits(x_before[k])) for k in x_before)
    # the same bits as the plan
    src = Engine(con_dynamics.problem_arrays(pdict, unitdict), device=-1)
    dst = Engine(con_dynamics.problem_arrays(pn, unitdict), device=-1)
    ref, rc = src.transfer_plan(dst).apply_host(pack_x(xdict))
    assert rc == 0 and np.array_equal(_bits(pack_x(xn)), _bits(ref[0]))
    # a plain list of counts; all kept = the input bits
    xk, pk = interp.refine(xdict, pdict, unitdict, [dict(r, suggested=r["num_nodes"], action="kept") for r in recs])
    assert np.array_equal(_bits(pack_x(xk)), _bits(pack_x(xdict))) and pk["N"] == pdict["N"]
    xl, _pl = interp.refine(xdict, pdict, unitdict, new)
    assert np.array_equal(_bits(pack_x(xl)), _bits(pack_x(xn)))
    with pytest.raises(ValueError):
        interp.refine(xdict, pdict, unitdict, new[:-1])
    # dense output
    k = 7
    out = interp.sample(xdict, pdict, unitdict, per_section=k)
    assert out["t"].shape == (k * S,) and out["position"].shape == (k * S, 3) and out["quaternion"].shape == (k * S, 4)
    assert out["u"].shape == (k * S, 2) and np.array_equal(out["section"], np.repeat(np.arange(S), k))
    assert np.all(np.diff(out["t"]) >= 0) and np.all(np.diff(out["t"].reshape(S, k), axis=1) > 0)
    ps = pdict["ps_params"]
    for s in range(S):
        xa, xb = ps.index_start_x(s), ps.index_end_x(s) - 1
        for row, node in ((s * k, xa), (s * k + k - 1, xb)):
            assert out["mass"][row] == xdict["mass"][node] * unitdict["mass"]
            assert np.array_equal(out["position"][row], xdict["position"].reshape(-1, 3)[node] * unitdict["position"])
            assert np.array_equal(out["velocity"][row], xdict["velocity"].reshape(-1, 3)[node] * unitdict["velocity"])
            assert np.array_equal(out["quaternion"][row], xdict["quaternion"].reshape(-1, 4)[node])
        # the time column is sigma (tf - to) / 2 + (tf + to) / 2 also at sigma = -1 / +1: the knot time within its three roundings
        to, tf = xdict["t"][s], xdict["t"][s + 1]
        tb = 4 * U * (abs(to) + abs(tf)) * unitdict["t"]
        assert abs(out["t"][s * k] - to * unitdict["t"]) <= tb and abs(out["t"][s * k + k - 1] - tf * unitdict["t"]) <= tb
        assert np.array_equal(out["u"][s * k + k - 1], xdict["u"].reshape(-1, 2)[ps.index_end_u(s) - 1] * unitdict["u"])
    pts = [np.array([0.25])] * S
    one = interp.sample(xdict, pdict, unitdict, points=pts)
    assert one["t"].shape == (S,)
    with pytest.raises(ValueError):
        interp.sample(xdict, pdict, unitdict)


def test_argument_checks():
    from gelato_amd import _lib
    L = _lib.lib()
    E2, E3 = it.engine(it.prob_of([4, 5])), it.engine(it.prob_of([4, 5, 6]))
    sentinel = 0x5A5A5A5A
    h = C.c_void_p(sentinel)

    def create(npts, pts):
        npts = np.array(npts, dtype=np.int32)
        pts = np.array(pts, dtype=np.float64)
        return L.gel_interp_plan_create(E2._h, npts.ctypes.data_as(_lib._ip), pts.ctypes.data_as(_lib._dp), 0, C.byref(h))

    assert L.gel_interp_plan_create_transfer(E2._h, E3._h, 0, C.byref(h)) == -1 and h.value == sentinel   # S mismatch
    for bad in (1.0000000000000002, -1.5, np.nan, np.inf):
        assert create([2, 1], [0.0, bad, 0.5]) == -1 and h.value == sentinel
    assert create([2, -1], [0.0, 0.1]) == -1 and h.value == sentinel
    assert L.gel_interp_plan_create_transfer(E2._h, E2._h, 2, C.byref(h)) == -1 and h.value == sentinel   # unknown flag
    # npts[s] = 0 and B = 0 are valid; B < 0 is not, and leaves out alone
    plan = E2.interp_plan([np.array([0.5, -1.0]), np.zeros(0)])
    assert plan.info()["state_rows"] == 2 and plan.matrices(1)["Wx"].shape == (0, 6)
    x = it.random_x(E2)
    out = np.full((1, 2, 14), 7.0)
    assert L.gel_interp_host(plan._p, -1, x.ctypes.data_as(_lib._dp), out.ctypes.data_as(_lib._dp)) == -1 and np.all(out == 7.0)
    assert L.gel_interp_host(plan._p, 0, x.ctypes.data_as(_lib._dp), out.ctypes.data_as(_lib._dp)) == 0 and np.all(out == 7.0)
    got, rc = plan.apply_host(x)
    assert rc == 0 and got.shape == (1, 2, 14) and np.all(np.isfinite(got))
    none = E2.interp_plan([np.zeros(0), np.zeros(0)])
    got, rc = none.apply_host(x)
    assert rc == 0 and got.shape == (1, 0, 14)
    # a host-only handle has no device form
    with pytest.raises(_lib.GelatoAmdError):
        plan.apply(x)
    with pytest.raises(ValueError):
        E2.interp_plan([np.zeros(1)])
    plan.close()
    plan.close()

"""Ground truth of the defect Jacobian for tests/test_exact_jac.py (tests/golden/g19_exact_jac.npz, written by
tests/golden/make_exact_jac.py): the states it is taken at, and the expected value of every x-dependent COO entry built from it.

The fixture holds, per collocation node g of each state: the velocity RHS f = acc / unit_v [N, 3] and its derivatives with
respect to the NORMALISED variables (mass, position 3, velocity 3, quaternion 4) [N, 3, 11] -- central differences of the
reference's formulas composed in 60-digit arithmetic on exact inputs (h = 1e-25), and both one-sided quotients where they
disagree (a table knot, layer break or clamp within h: `kink`), and the central quotient [N, 3, 11]; the quaternion kinematics fq [N, 4] and d fq / d(q, u) [N, 4, 6]."""
import numpy as np


def corner_state():
    """The nodes of test_parity_corners_underground_polar_and_air_at_rest as one aerodynamic phase in calm air: 8 below the polar
    radius (the r < b clamp of gravity), 3 exactly on the polar axis, 2 at rest in the air (v = omega x r)."""
    from gelato_amd import con_dynamics, problem
    pdict, unitdict, _, _ = problem.make_problem("example")
    base = con_dynamics.problem_arrays(pdict, unitdict)
    Rb = 6378137.0 * (1.0 - 1.0 / 298.257223563)
    omega = 7.2921151467e-5
    rng = np.random.default_rng(3)
    d = rng.standard_normal((8, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    r_under = d * (np.linspace(0.3, 0.999, 8) * Rb)[:, None]
    r_polar = np.array([[0.0, 0.0, 6.45e6], [0.0, 0.0, -6.5e6], [0.0, 0.0, 6.36e6]])
    r_rest = np.array([[4.2e6, 3.9e6, 2.9e6], [-5.0e6, 1.0e6, 4.0e6]]) * 1.02
    v_rest = np.column_stack([-(omega * r_rest[:, 1]), omega * r_rest[:, 0], np.zeros(2)])
    r = np.vstack([r_under, r_polar, r_rest])
    v = np.vstack([rng.standard_normal((11, 3)) * 300.0, v_rest])
    n = len(r)
    calm = np.array(base["wind_table"], dtype=np.float64).copy()
    calm[:, 1:] = 0.0
    prob = {"num_nodes": np.array([n], dtype=np.int32), "thrust": np.array([4.2e5]), "massflow": np.array([140.0]),
            "reference_area": np.array([2.21]), "nozzle_area": np.array([0.68]), "engine_on": np.array([1], dtype=np.int32),
            "attitude_hold": np.array([0], dtype=np.int32), "units": np.array(base["units"], dtype=np.float64),
            "dx": float(base["dx"]), "wind_table": calm, "ca_table": np.array(base["ca_table"], dtype=np.float64)}
    up, uv = float(prob["units"][1]), float(prob["units"][2])
    M = n + 1
    q = rng.standard_normal((M, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    x = np.concatenate([np.full(M, 0.7), np.vstack([r[:1], r]).ravel() / up, np.vstack([v[:1], v]).ravel() / uv, q.ravel(),
                        rng.standard_normal(2 * n) * 0.1, [0.0, 0.05]])
    return prob, x


def example_state():
    from gelato_amd import con_dynamics, pack_x, problem
    pdict, unitdict, _, xdict = problem.make_problem("example")
    return dict(con_dynamics.problem_arrays(pdict, unitdict)), pack_x(xdict)


def states():
    import states as st
    return {"example": example_state, "ragged": st.ragged_state, "layers": st.all_layers_state, "breaks": st.layer_break_state,
            "polar": st.polar_dense_state, "corners": corner_state}


def jump_entries(E, prob, G, name):
    """boolean [total_nnz]: vel/position entries whose two one-sided quotients differ by orders of magnitude -- the value jumps
    at the node (on the polar axis the altitude is the reference's -N, off it the true altitude): no derivative exists there"""
    from gelato_amd.engine import BLOCKS
    f, b = G[name + "_Jv_f"], G[name + "_Jv_b"]
    jump = np.abs(f - b) > 1e3 * (np.abs(G[name + "_Jv_c"]) + 1.0)          # [N, 3, 11]
    nn = [int(v) for v in prob["num_nodes"]]
    S, N = len(nn), sum(nn)
    ua = np.concatenate([[0], np.cumsum(nn)[:-1]]).astype(int)
    phase = np.repeat(np.arange(S), nn)
    out = np.zeros(E.total_nnz, dtype=bool)
    pat = E.pattern()
    b = BLOCKS.index(("vel", "position"))
    r, c = pat[b]
    g, comp = r // 3, r % 3
    xj = ua[phase[g]] + phase[g] + 1 + (g - ua[phase[g]])
    out[E.block_off[b]:E.block_off[b + 1]] = jump[g, comp, 1 + (c - 3 * xj)]
    return out


def expected_full(E, prob, x, G, name, which="c"):
    """expected value of every x-dependent entry of E's full COO value array (NaN elsewhere) from the fixture's state `name`.
    which: "c" central quotients, "f" / "b" the one-sided ones (they differ only at kinks)."""
    from gelato_amd.engine import BLOCKS
    nn = [int(v) for v in prob["num_nodes"]]
    S, N = len(nn), sum(nn)
    M = N + S
    um, up, uv, uu, ut = [float(u) for u in prob["units"]]
    Jv = G[name + "_Jv_" + which]
    fv, fq, Jq = G[name + "_fv"], G[name + "_fq"], G[name + "_Jq"]
    ua = np.concatenate([[0], np.cumsum(nn)[:-1]]).astype(int)
    phase = np.repeat(np.arange(S), nn)
    xt = x[11 * M + 2 * N:]
    Sg = (xt[phase + 1] - xt[phase]) * ut / 2.0           # d(residual) / d(rhs) = -S per node
    vel = x[4 * M:7 * M].reshape(-1, 3)
    Dj = np.array([E.D(int(phase[g]))[g - ua[phase[g]], g - ua[phase[g]] + 1] for g in range(N)])
    var = E.var_mask()
    pat = E.pattern()
    out = np.full(E.total_nnz, np.nan)
    for b, (grp, vn) in enumerate(BLOCKS):
        r, c = pat[b]
        m = var[E.block_off[b]:E.block_off[b + 1]]
        if not m.any():
            continue
        r, c = r[m], c[m]
        k = 4 if grp == "quat" else 3
        g, comp = r // k, r % k
        i = phase[g]
        xa = ua[i] + i
        xj = xa + 1 + (g - ua[i])                          # the node's state row
        if grp == "pos":
            if vn == "velocity":
                val = -(uv * ut / 2.0 / up) * (xt[i + 1] - xt[i]) * np.ones(len(g))
            else:                                          # t0 / tf columns
                val = np.where(c == i, 1.0, -1.0) * (uv * ut / 2.0 / up) * vel[xj, comp]
        elif grp == "vel":
            if vn == "mass":
                val = -Sg[g] * Jv[g, comp, 0]
            elif vn in ("position", "velocity", "quaternion"):
                o, w = {"position": (1, 3), "velocity": (4, 3), "quaternion": (7, 4)}[vn]
                kk = c - w * xj
                val = -Sg[g] * Jv[g, comp, o + kk]
                if vn == "velocity":
                    val = val + np.where(kk == comp, Dj[g], 0.0)
            else:
                val = np.where(c == i, 1.0, -1.0) * (ut / 2.0) * fv[g, comp]
        else:
            if vn == "quaternion":
                kk = c - 4 * xj
                val = -Sg[g] * Jq[g, comp, kk] + np.where(kk == comp, Dj[g], 0.0)
            elif vn == "u":
                val = -Sg[g] * Jq[g, comp, 4 + (c - 2 * g)]
            else:
                val = np.where(c == i, 1.0, -1.0) * (ut / 2.0) * fq[g, comp]
        blk = out[E.block_off[b]:E.block_off[b + 1]]
        idx = np.nonzero(m)[0]
        blk[idx] = val
    return out

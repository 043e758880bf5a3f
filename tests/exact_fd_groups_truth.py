"""The known answers of tests/golden/g21_exact_fd_groups.npz and how a Jacobian / residual is held to them (shared by
tests/test_exact_fd_groups.py, tests/parity_margin.py and the fixture's generator; no mpmath here).

Blocks checked, per fixture phase (bounds: tests/fd_noise.py):
  vel/mass, vel/position, vel/quaternion, vel/t    of every NoAir phase listed in <name>_noair
  quat/quaternion, quat/u, quat/t                  of every free-attitude phase listed in <name>_quat
  residual rows of the mass, pos, vel, quat groups of every phase listed in <name>_res"""
import hashlib

import numpy as np

import fd_noise
import states
from conftest import load_golden


def workload_state(name):
    from gelato_amd import con_dynamics, pack_x, problem
    pdict, unitdict, condition, xdict = problem.make_problem(name)
    return dict(con_dynamics.problem_arrays(pdict, unitdict)), pack_x(xdict)


# name: (builder, NoAir phases, quaternion-group phases, residual phases); None = every phase of the kind (residuals: the union)
STATES = {
    # every phase without aerodynamics; the quaternion group of every free-attitude phase
    "example": (lambda: workload_state("example"), None, None, None),
    # NoAir 3 (2 nodes, hold), 4 (engine off, hold), 6; quaternion group of 1 (engine off, free) and 2 (100 nodes: two chunks)
    "ragged": (states.ragged_state, [3, 4, 6], [1, 2], [1, 2, 3, 4, 6]),
    # 129 nodes: chunked, slab-staged D.X
    "long": (lambda: states.long_state((87, 129, 64)), [1], [0, 1], [1]),
    # the BASELINE.json workloads
    "mixed-6x64": (lambda: workload_state("mixed-6x64"), None, [1, 5], [1, 5]),
    "stress-12x128": (lambda: workload_state("stress-12x128"), [6, 8], [2, 7], [2, 6]),
    # two vectors per wavefront
    "3x32": (lambda: workload_state("3x32"), None, [0, 2], [0, 2]),
    # on and next to the polar axis, -20 km .. 20,000 km, thrust off and on
    "noair-polar": (states.noair_polar_state, None, None, None),
    # the aero path constraints' coast tail: a 2-node engine-off phase behind a 64-node climb through every layer
    "coast-tail": (lambda: states.with_coast_tail(states.all_layers_state), [1], [1], [1]),
}
BASELINE = ("mixed-6x64", "stress-12x128")     # their decision vectors live in g15b; g21 holds a digest
FIXTURE = "g21_exact_fd_groups.npz"


def x_digest(x):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(x, dtype="<f8").tobytes()).digest(), dtype=np.uint8)


def setup(name, G=None):
    """-> (G, prob, x, P, D): the fixture, the state (prob with the oracle's tau), the oracle problem and its fp64 D per phase"""
    import oracle
    G = load_golden(FIXTURE) if G is None else G
    prob, x = STATES[name][0]()
    if name + "_x" in G:
        assert np.array_equal(x, G[name + "_x"]), "the state builder no longer reproduces the fixture's decision vector"
    else:
        assert np.array_equal(x_digest(x), G[name + "_x_sha256"]), "the workload no longer reproduces the fixture's decision vector"
    P = oracle.Problem(prob)
    prob = dict(prob)
    prob["tau"] = [P.tau(i) for i in range(P.S)]
    return G, prob, x, P, [P.D(i) for i in range(P.S)]


def split(prob, x):
    nn = [int(v) for v in prob["num_nodes"]]
    S, N = len(nn), sum(nn)
    M = N + S
    o = np.cumsum([0, M, 3 * M, 3 * M, 4 * M, 2 * N, S + 1])
    xs = {k: x[o[i]:o[i + 1]] for i, k in enumerate(["mass", "position", "velocity", "quaternion", "u", "t"])}
    for k, w in (("position", 3), ("velocity", 3), ("quaternion", 4), ("u", 2)):
        xs[k] = xs[k].reshape(-1, w)
    return xs


class Layout:
    """the position of every checked entry in a group's COO arrays (the reference's pattern: the same for the oracle and every
    engine form and output path), sorted once per state"""

    def __init__(self, J, prob):
        self.nn = [int(v) for v in prob["num_nodes"]]
        self._keys = {}
        for g, blocks in J.items():
            for var, blk in blocks.items():
                r, c = np.asarray(blk["coo"][0], dtype=np.int64), np.asarray(blk["coo"][1], dtype=np.int64)
                w = int(c.max()) + 2 if c.size else 1
                key = r * w + c
                order = np.argsort(key, kind="stable")
                self._keys[(g, var)] = (key[order], order, w)

    def index(self, g, var, rows, cols):
        skey, order, w = self._keys[(g, var)]
        key = (np.asarray(rows, dtype=np.int64) * w + np.asarray(cols, dtype=np.int64)).ravel()
        pos = np.minimum(np.searchsorted(skey, key), skey.size - 1)
        assert np.array_equal(skey[pos], key), (g, var, "entry not in the pattern")
        return order[pos].reshape(np.shape(rows))

    def phase(self, ph):
        ua = sum(self.nn[:ph])
        return ua, ua + ph, self.nn[ph]


def _grid(*axes):
    return np.meshgrid(*axes, indexing="ij")


def checks(J, G, name, prob, x, D, form, lay=None):
    """-> list of (label, got, exact, bound) for every checked Jacobian entry of J ({group: {var: {"coo": ...}}}, the reference's
    layout).  form: "closed" (the engine's default form) or "recompute" (GEL_FLAG_FD_RECOMPUTE, and the oracle)."""
    lay = Layout(J, prob) if lay is None else lay
    xs = split(prob, x)
    dx, uu, ut = float(prob["dx"]), float(prob["units"][3]), float(prob["units"][4])
    out = []

    def val(g, var, rows, cols):
        return np.asarray(J[g][var]["coo"][2])[lay.index(g, var, rows, cols)]

    for ph in G[name + "_noair"]:
        ph = int(ph)
        ua, xa, n = lay.phase(ph)
        j = np.arange(n)
        to, tf = xs["t"][ph], xs["t"][ph + 1]
        chain = fd_noise.noair_chain_bound(G["%s_p%d_ntmag" % (name, ph)], G["%s_p%d_ngmag" % (name, ph)],
                                           (tf - to) * ut / 2 / dx)[:, None, None]
        for var, w, key in (("mass", 1, "nmass"), ("position", 3, "npos"), ("quaternion", 4, "nquat")):
            jj, cc, kk = _grid(j, np.arange(3), np.arange(w))
            got = val("vel", var, 3 * (ua + jj) + cc, w * (xa + 1 + jj) + kk)
            exact = G["%s_p%d_%s" % (name, ph, key)].reshape(n, 3, w)
            if var == "position" or form == "recompute":
                b = np.broadcast_to(chain, exact.shape)
            else:
                b = fd_noise.closed_bound(exact)
            out.append(("NoAir vel/" + var, got, exact, b))
        fc = G["%s_p%d_nfc" % (name, ph)]
        jj, cc = _grid(j, np.arange(3))
        for col, sign in ((ph, 1.0), (ph + 1, -1.0)):
            got = val("vel", "t", 3 * (ua + jj) + cc, np.full_like(jj, col))
            exact = sign * fc * ut / 2
            out.append(("NoAir vel/t", got, exact, fd_noise.t_column_bound(exact)))
    for ph in G[name + "_quat"]:
        ph = int(ph)
        ua, xa, n = lay.phase(ph)
        j = np.arange(n)
        to, tf = xs["t"][ph], xs["t"][ph + 1]
        q, u = xs["quaternion"][xa + 1:xa + 1 + n], xs["u"][ua:ua + n]
        W = fd_noise.quat_magnitude(q, u, uu)
        rq, ru = fd_noise.quat_step_ratio(q, u, dx, uu)
        Djj = D[ph][j, j + 1]
        # quat/quaternion: D on the diagonal + the quotient (lib/con_dynamics.py:575-589)
        jj, cc, kk = _grid(j, np.arange(4), np.arange(4))
        diag = np.where(cc == kk, Djj[:, None, None], 0.0)
        got = val("quat", "quaternion", 4 * (ua + jj) + cc, 4 * (xa + 1 + jj) + kk) - diag
        exact = G["%s_p%d_qquat" % (name, ph)]
        sc = (tf - to) * ut / 2 / dx
        b = fd_noise.quat_chain_bound(W, sc, exact) if form == "recompute" else fd_noise.quat_closed_bound(exact, rq)
        out.append(("quat/quaternion", got, exact, b + 4 * fd_noise.EPS * np.abs(diag)))
        jj, cc, kk = _grid(j, np.arange(4), np.arange(2))
        got = val("quat", "u", 4 * (ua + jj) + cc, 2 * (ua + jj) + kk)
        exact = G["%s_p%d_qu" % (name, ph)]
        b = fd_noise.quat_chain_bound(W, sc, exact) if form == "recompute" else fd_noise.quat_closed_bound(exact, ru)
        out.append(("quat/u", got, exact, b))
        fc = G["%s_p%d_qfc" % (name, ph)]
        jj, cc = _grid(j, np.arange(4))
        bt = np.broadcast_to((fd_noise.C_QUAT * fd_noise.EPS * W * ut / 2)[:, None], fc.shape)
        for col, sign in ((ph, 1.0), (ph + 1, -1.0)):
            got = val("quat", "t", 4 * (ua + jj) + cc, np.full_like(jj, col))
            out.append(("quat/t", got, sign * fc * ut / 2, bt))
    return out


def residual_checks(R, G, name, prob, x, D):
    """R: {group: residual vector} (the reference's layout) -> list of (label, got, exact, bound).  Aerodynamic velocity rows keep
    test_exact_fd's tolerance (1e-12 + 1e-10 |ref| + (n + 1) eps |D| |X|): their f carries the atmosphere's chain."""
    nn = [int(v) for v in prob["num_nodes"]]
    xs = split(prob, x)
    um, up, uv, uu, ut = (float(v) for v in prob["units"])
    out = []
    for ph in G[name + "_res"]:
        ph = int(ph)
        ua, n = sum(nn[:ph]), nn[ph]
        xa = ua + ph
        sl = slice(xa, xa + n + 1)
        Dm = D[ph]
        h = (xs["t"][ph + 1] - xs["t"][ph]) * ut / 2
        m = xs["mass"][sl]
        if prob["engine_on"][ph]:
            b = fd_noise.residual_bound(Dm, m[:, None], h * prob["massflow"][ph] / um)[:, 0]
        else:
            b = fd_noise.residual_bound(None, None, diff=m)
        out.append(("res/mass", np.asarray(R["mass"])[ua:ua + n], G["%s_p%d_rmass" % (name, ph)], b))
        b = fd_noise.residual_bound(Dm, xs["position"][sl], h * np.abs(xs["velocity"][xa + 1:xa + n + 1]) * uv / up)
        out.append(("res/pos", np.asarray(R["pos"]).reshape(-1, 3)[ua:ua + n], G["%s_p%d_rpos" % (name, ph)], b))
        exact = G["%s_p%d_rvel" % (name, ph)]
        got = np.asarray(R["vel"]).reshape(-1, 3)[ua:ua + n]
        if prob["reference_area"][ph] == 0.0:
            tg = G["%s_p%d_ntmag" % (name, ph)] + G["%s_p%d_ngmag" % (name, ph)]
            b = fd_noise.residual_bound(Dm, xs["velocity"][sl], h * tg[:, None] * np.ones((1, 3)))
            out.append(("res/vel NoAir", got, exact, b))
        else:
            b = 1e-12 + 1e-10 * np.abs(exact) + (n + 1) * fd_noise.EPS * (np.abs(Dm) @ np.abs(xs["velocity"][sl]))
            out.append(("res/vel aero", got, exact, b))
        got = np.asarray(R["quat"]).reshape(-1, 4)[ua:ua + n]
        if prob["attitude_hold"][ph]:
            b = fd_noise.residual_bound(None, None, diff=xs["quaternion"][sl])
        else:
            W = fd_noise.quat_magnitude(xs["quaternion"][xa + 1:xa + n + 1], xs["u"][ua:ua + n], uu)
            b = fd_noise.residual_bound(Dm, xs["quaternion"][sl], h * W[:, None] * np.ones((1, 4)))
        out.append(("res/quat", got, G["%s_p%d_rquat" % (name, ph)], b))
    return out


def ratios(items):
    """{label: max |got - exact| / bound} (an exact match counts 0, whatever the bound)"""
    w = {}
    for label, got, exact, b in items:
        err = np.abs(np.asarray(got) - exact)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0.0, 0.0, err / b)
        w[label] = max(w.get(label, 0.0), float(r.max()) if r.size else 0.0)
    return w

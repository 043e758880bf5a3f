"""Ground truth of the aero path constraints' gradients for tests/test_exact_aero_jac.py (tests/golden/g20_exact_aero_jac.npz,
written by tests/golden/make_exact_aero_jac.py): the cases it is taken at and the expected gradient values built from it.

The fixture holds, per constrained node of each case: alpha [rad] and q [Pa] of the reference's formulas on exact inputs, and their
derivatives with respect to the NORMALISED position (3), velocity (3) and quaternion (4) [R, 10]: central differences in 60-digit
arithmetic with h = 1e-25 (`c`) and both one-sided quotients (`f`, `b`), which differ only where a table knot, layer break or
clamp lies within h of the node (`kink`)."""
import numpy as np

KINDS = ["alpha", "q", "qalpha"]
VARS = ["position", "velocity", "quaternion", "t"]
LIMITS = {"alpha": 0.2, "q": 4.0e4, "qalpha": 5.0e3}     # units[3] of con_aero.py for the synthetic cases
CASES = ["g9_example", "g9_synthetic", "ragged", "polar", "layers", "breaks", "mixed-6x64", "corners"]
LONG_CASES = ["climb", "knots"]     # g28_long_tables.npz: tests/states.py table_state("LONG", (40, 65, 2), .)
COLS = {"position": slice(0, 3), "velocity": slice(3, 6), "quaternion": slice(6, 10)}


def _with_tau(prob, x):
    import oracle
    P = oracle.Problem(prob)
    prob = dict(prob)
    prob["tau"] = [P.tau(i) for i in range(P.S)]
    return prob, [P.D(i) for i in range(P.S)], x


def _all_aero(prob):
    """every aerodynamic phase but the last (lib/con_aero.py:108), all nodes, for every kind"""
    S = len(prob["num_nodes"])
    return {k: np.array([(i, 1, LIMITS[k]) for i in range(S - 1) if prob["reference_area"][i] != 0.0]).reshape(-1, 3) for k in KINDS}


def case(name):
    """-> prob (with tau), D, x, {kind: spec rows (phase, range_all, limit)}"""
    import states
    if name.startswith("g9_"):
        from conftest import D_tau_from_golden, load_golden, problem_from_golden
        from test_aero_oracle_golden import spec_from_golden
        g = load_golden("g9_aero_example.npz")
        prob = dict(problem_from_golden(g))
        D, tau = D_tau_from_golden(g, prob)
        prob["tau"] = tau
        return prob, D, g["x"], {k: spec_from_golden(g, name[3:], k) for k in KINDS}
    if name == "mixed-6x64":
        from gelato_amd import con_dynamics, pack_x, problem
        pdict, unitdict, _, xdict = problem.make_problem(name)
        prob, D, x = _with_tau(dict(con_dynamics.problem_arrays(pdict, unitdict)), pack_x(xdict))
        return prob, D, x, _all_aero(prob)
    if name in LONG_CASES:
        import table_cases as TC
        prob, D, x = _with_tau(*states.table_state("LONG", TC.MESHES["coop"], name))
        return prob, D, x, _all_aero(prob)
    if name == "corners":
        import exact_jac_truth
        prob, D, x = _with_tau(*states.with_coast_tail(exact_jac_truth.corner_state))
        return prob, D, x, _all_aero(prob)
    build = {"ragged": states.ragged_state, "polar": lambda: states.with_coast_tail(states.polar_dense_state),
             "layers": lambda: states.with_coast_tail(states.all_layers_state),
             "breaks": lambda: states.with_coast_tail(states.layer_break_state)}[name]
    prob, D, x = _with_tau(*build())
    return prob, D, x, _all_aero(prob)


def case_nodes(prob, specs):
    """the union of the constrained state nodes (phase, node) over the kinds, in (phase, node) order"""
    nn = [int(v) for v in prob["num_nodes"]]
    out = set()
    for spec in specs.values():
        for ph, al, _ in spec:
            out.update((int(ph), k) for k in range(nn[int(ph)] + 1 if int(al) else 1))
    return sorted(out)


class Truth:
    """the fixture's rows for one kind's spec, in the constraint's row order"""

    def __init__(self, G, name, prob, x, kind, spec):
        assert np.array_equal(x, G[name + "_x"]), "the case builder no longer reproduces the fixture's decision vector"
        nn = [int(v) for v in prob["num_nodes"]]
        where = {(int(p), int(k)): i for i, (p, k) in enumerate(G[name + "_nodes"])}
        idx, lim, self.blocks = [], [], []
        for ph, al, limit in spec:
            nk = nn[int(ph)] + 1 if int(al) else 1
            self.blocks.append((len(idx), nk))
            idx += [where[(int(ph), k)] for k in range(nk)]
            lim += [limit] * nk
        idx = np.array(idx, dtype=int)
        self.idx = idx
        self.kind, self.lim = kind, np.array(lim)
        self.alpha, self.q = G[name + "_alpha"][idx], G[name + "_q"][idx]
        self.d = {(s, w): G["%s_d%s_%s" % (name, s, w)][idx] for s in "aq" for w in "cfb"}
        self.kink = {s: G["%s_kink_%s" % (name, s)][idx] for s in "aq"}

    def per_row(self, per_node):
        """a per-node array of the fixture [nodes] -> per row of this spec"""
        return np.asarray(per_node)[self.idx]

    def grad(self, which):
        """[R, 10] d con / d x (con = 1 - f / limit) from the quotients `which` ("c", "f", "b"): per row and variable"""
        da, dq = self.d[("a", which)], self.d[("q", which)]
        d = {"alpha": da, "q": dq, "qalpha": self.q[:, None] * da + self.alpha[:, None] * dq}[self.kind]
        return -d / self.lim[:, None]

    def kinked(self):
        """[R, 10] entries with a knot, layer break or clamp within h"""
        return {"alpha": self.kink["a"], "q": self.kink["q"], "qalpha": self.kink["a"] | self.kink["q"]}[self.kind]

    def coo(self, per_row, var):
        """[R, 10] -> the block of `var` in the reference's emission order (per spec, column-major; con_aero.py:437-463)"""
        if var == "t":
            return np.zeros(2 * sum(nk for _, nk in self.blocks))
        if var == "quaternion" and self.kind == "q":
            return np.zeros(0)
        v = per_row[:, COLS[var]]
        return np.concatenate([v[r0:r0 + nk].T.ravel() for r0, nk in self.blocks]) if self.blocks else np.zeros(0)

    def coo_all(self, per_row):
        return np.concatenate([self.coo(per_row, var) for var in VARS])

    def row_of_entries(self, var):
        """row index of every entry of `var`'s block (same order as coo())"""
        rows = np.arange(len(self.lim))
        w = {"position": 3, "velocity": 3, "quaternion": 0 if self.kind == "q" else 4, "t": 2}[var]
        return np.concatenate([np.tile(rows[r0:r0 + nk], w) for r0, nk in self.blocks]) if self.blocks else np.zeros(0, int)

    def rows_all(self):
        return np.concatenate([self.row_of_entries(var) for var in VARS])

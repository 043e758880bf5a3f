"""Independent restatement of the chained flight and of the dispersions (include/gelato_amd.h gel_propagate, GEL_PROP_CHAIN and
gel_propagate_dispersed) for the tests: propagate_truth's RK4 step, right-hand side and first-order bound, with
the start state and the start bound E passed in, so that a flight is the phases in order.

  knot into phase s + 1   jump = x(first node of s + 1) - x(last node of s), the same subtraction of the same bits on both sides;
                          y <- y where jump == 0 (the bits are carried; E grows by nothing), else y + jump, and E grows by
                          u (|jump| + |y + jump|): the roundings of the difference and of the sum
  dispersed phase         a copy of prob with thrust[s] f_0, reference_area[s] f_2 and the wind table's two wind columns f_3 --
                          the fp64 products the device forms -- and the mass row restated as (-massflow / unit_mass) f_1: the same
                          quotient and the same product, so its dF stays 0.  Only the wind differs in form (the scaled table here,
                          the scaled interpolant on the device: one rounding each side, 2u of the wind), which enters F through
                          dF_wind = 2u |F(f_3 (1 + 2^-20)) - F(f_3)| 2^20 from the oracle's own right-hand side.
  node restart            fly_all(restart="node"): every node interval from the collocated X_j with E = 0 under the phase's factors
                          (gel_propagate_dispersed on a GEL_PROP_RESTART_NODE plan); the step is rk4_step, the one of the chain
The tests allow 2 E, as propagate_truth's do.

Three WRONG restatements (`mutate`) give the bound its teeth: "no_jump" carries y across every knot without the collocated jump,
"shift_factors" flies phase s + 1 with the factors of phase s (phase 0 undispersed), "no_wind_factor" ignores the wind factor."""
import numpy as np

import mesh_truth as mt
from mesh_truth import GROUP_COLS, U
from propagate_truth import _dF, _jac_abs, _rhs, group_err, samples

EPS_W = 2.0 ** -20


def dispersed_prob(prob, s, f, wind_scale=1.0):
    """prob with phase s's thrust and reference area and the wind table's wind columns scaled by the factors f [4]"""
    p = dict(prob)
    p["thrust"] = np.array(prob["thrust"], dtype=float)
    p["thrust"][s] = p["thrust"][s] * f[0]
    p["reference_area"] = np.array(prob["reference_area"], dtype=float)
    p["reference_area"][s] = p["reference_area"][s] * f[2]
    w = np.array(prob["wind_table"], dtype=float)
    w[:, 1:3] = w[:, 1:3] * (f[3] * wind_scale)
    p["wind_table"] = w
    return p


class _Phase:
    """the right-hand side of phase s under the factors f (None: undispersed) and what the two sides may differ by"""

    def __init__(self, prob, s, f):
        self.prob, self.s, self.f = prob, s, f
        self.pd = prob if f is None else dispersed_prob(prob, s, f)
        self.air = float(prob["reference_area"][s]) != 0.0
        self.windy = f is not None and self.air and float(f[3]) != 0.0 and np.isfinite(f[3])
        self.pw = dispersed_prob(prob, s, f, 1.0 + EPS_W) if self.windy else None
        self.mass = None
        if f is not None and prob["engine_on"][s]:
            self.mass = (-float(prob["massflow"][s]) / float(prob["units"][0])) * f[1]

    def F(self, X, Uv, sig, to, tf, pd=None):
        F = _rhs(pd if pd is not None else self.pd, self.s, X, Uv, sig, to, tf)
        if self.mass is not None:
            F[:, 0] = self.mass
        return F

    def dF(self, y, yt, Uv, dUv, sig, to, tf, F):
        """y: the step's start (what propagate_truth's dF takes); yt: the stage's state, where F was formed"""
        d = _dF(self.pd, self.s, y, Uv, dUv, F)
        if self.windy:
            d = d + 2 * U * np.abs(self.F(yt, Uv, sig, to, tf, pd=self.pw)[0] - F) / EPS_W
        return d


def rk4_step(ph, s, y, Eb, Sh, p, Us, dUs, pts, to, tf, want_bound=True):
    """one RK4 step of phase ph from (y, Eb) over S h = Sh, whose stage points are p, p + 1, p + 2 -> (y, Eb) at its end.
    propagate_truth.propagate_phase's loop body, operation for operation (Eb is returned as it came where want_bound is off)."""
    k1 = ph.F(y, Us[p], pts[p], to, tf)[0]
    y2 = y + Sh * 0.5 * k1
    k2 = ph.F(y2, Us[p + 1], pts[p + 1], to, tf)[0]
    y3 = y + Sh * 0.5 * k2
    k3 = ph.F(y3, Us[p + 1], pts[p + 1], to, tf)[0]
    y4 = y + Sh * k3
    k4 = ph.F(y4, Us[p + 2], pts[p + 2], to, tf)[0]
    if want_bound:
        A = _jac_abs(ph.pd, s, y, Us[p], pts[p], to, tf, k1)
        if ph.mass is not None:
            A[0, :] = 0.0    # (k1's mass row is the restated constant, not the oracle's: its derivative is zero)
        aS = abs(Sh)
        e1 = A @ Eb + ph.dF(y, y, Us[p], dUs[p], pts[p], to, tf, k1)
        e2 = A @ (Eb + aS / 2 * e1) + ph.dF(y, y2, Us[p + 1], dUs[p + 1], pts[p + 1], to, tf, k2)
        e3 = A @ (Eb + aS / 2 * e2) + ph.dF(y, y3, Us[p + 1], dUs[p + 1], pts[p + 1], to, tf, k3)
        e4 = A @ (Eb + aS * e3) + ph.dF(y, y4, Us[p + 2], dUs[p + 2], pts[p + 2], to, tf, k4)
    y = y + Sh / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)
    if want_bound:
        Eb = Eb + aS / 6 * (e1 + 2 * e2 + 2 * e3 + e4) + 8 * U * np.abs(y)
    return y, Eb


def fly_phase(E, plan, prob, x, s, y0, E0, f=None, want_bound=True, restart=False):
    """phase s of one vector from the start state y0 [11] with the start bound E0 [11] -> (Y [n+1, 11], bound [n+1, 11] = 2 E at
    every node, E at the last node).  restart: every node interval j starts from the collocated X_j with E = 0
    (GEL_PROP_RESTART_NODE; y0 and E0 serve node 0 alone, where they are X_0 and 0)."""
    m = plan.matrices(s)
    k = plan.steps[s]
    X, Uc, to, tf = mt.phase_state(E, x, s)
    n = X.shape[0] - 1
    ph = _Phase(prob, s, f)
    ut = float(prob["units"][4])
    S = (tf - to) * ut / 2.0
    tx = np.concatenate([[-1.0], E.tau(s)])
    pts = m["pts"]
    if bool(prob["attitude_hold"][s]):
        Us, dUs = np.zeros((len(pts), 2)), np.zeros((len(pts), 2))
    else:
        Us, dUs = samples(m, Uc)
    hs = (tx[1:] - tx[:-1]) / k
    Y = np.full((n + 1, 11), np.nan)
    Bd = np.zeros((n + 1, 11))
    Y[0] = y0
    Bd[0] = 2 * E0
    y = np.array(y0, dtype=float)
    Eb = np.array(E0, dtype=float)
    for j in range(n):
        if restart:
            y, Eb = X[j].copy(), np.zeros(11)
        Sh = S * hs[j]
        for i in range(k):
            y, Eb = rk4_step(ph, s, y, Eb, Sh, 2 * (k * j + i), Us, dUs, pts, to, tf, want_bound)
        Y[j + 1] = y
        Bd[j + 1] = 2 * Eb
    return Y, Bd, Eb


def carry(y, Eb, x_last, x_first):
    """across a knot: (start state, start bound) of the next phase from the end state y, its bound Eb and the collocated states
    on the two sides of the knot"""
    jump = x_first - x_last
    with np.errstate(invalid="ignore"):
        moved = y + jump
    y0 = np.where(jump == 0.0, y, moved)
    E0 = Eb + np.where(jump == 0.0, 0.0, U * (np.abs(jump) + np.abs(moved)))
    return y0, E0


def fly_all(E, plan, prob, x, disp=None, want_bound=True, mutate=None, chain=True, restart=None):
    """one vector through every phase -> (y [M, 11], bound_y [M, 11], err [S, 4], bound_err [S, 4]).  disp: None or [S, 4];
    chain=False: every phase from its own X_0 (the section mode, for the dispersed parity there); restart="node": every node
    interval of every phase from the collocated X_j with E = 0, under the phase's factors (the node mode; nothing is carried, so
    chain is moot); mutate: see the module"""
    assert restart in (None, "node")
    node = restart == "node"
    ys, bs, es, bes = [], [], [], []
    y_end, E_end, X_prev = None, None, None
    for s in range(E.S):
        X = mt.phase_state(E, x, s)[0]
        if s == 0 or not chain or node:
            y0, E0 = X[0].copy(), np.zeros(11)
        elif mutate == "no_jump":
            y0, E0 = y_end, E_end
        else:
            y0, E0 = carry(y_end, E_end, X_prev[-1], X[0])
        f = None if disp is None else np.array(disp[s], dtype=float)
        if f is not None and mutate == "shift_factors":
            f = np.array(disp[s - 1], dtype=float) if s else None
        if f is not None and mutate == "no_wind_factor":
            f[3] = 1.0
        Y, Bd, E_end = fly_phase(E, plan, prob, x, s, y0, E0, f=f, want_bound=want_bound, restart=node)
        y_end, X_prev = Y[-1], X
        e, ec, den = group_err(X, Y)
        bc = Bd[1:].max(axis=0) / den + 4 * U * ec
        ys.append(Y); bs.append(Bd); es.append(e)
        bes.append(np.array([bc[a:b].max() for a, b in GROUP_COLS]))
    return np.concatenate(ys), np.concatenate(bs), np.array(es), np.array(bes)


def flight_batch(x0, E):
    """the example as a batch of three: x0 itself (every knot continuous), x0 with the mass jettisoned at the stage knots (the
    collocated mass drops there and stays lower), and a perturbed vector whose every component jumps a little at every knot"""
    from gelato_amd import problem
    pdict, unitdict, _c, _x = problem.make_problem("example")
    X = problem.synthetic_batch(x0, E.M, 3)
    X[1] = x0
    nn = [int(v) for v in E.num_nodes]
    for s, p in enumerate(pdict["params"][:E.S]):
        if p["mass_jettison"]:
            xa = sum(nn[:s]) + s
            X[1, xa:E.M] -= p["mass_jettison"] / unitdict["mass"]
    return X


def teeth_dispersion(S):
    """[S, 4]: thrust, mass flow and area away from one and different in every phase, the wind doubled"""
    d = np.ones((S, 4))
    s = np.arange(S)
    d[:, 0] = 0.9 + 0.2 * ((7 * s + 3) % 11) / 10.0
    d[:, 1] = 0.9 + 0.2 * ((5 * s + 1) % 11) / 10.0
    d[:, 2] = 0.9 + 0.2 * ((3 * s + 8) % 11) / 10.0
    d[:, 3] = 2.0
    return d


def mutant_miss(E, plan, prob, x, disp, mutate, y, by, **mode):
    """the largest |mutant - y| / bound over the nodes and components where the bound is positive (mode: fly_all's chain / restart)"""
    wrong = fly_all(E, plan, prob, x, disp=disp, want_bound=False, mutate=mutate, **mode)[0]
    d = np.abs(wrong - y)
    ok = np.isfinite(d) & (by > 0)
    return float((d[ok] / by[ok]).max())

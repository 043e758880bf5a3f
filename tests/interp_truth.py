"""Shared pieces of the interpolation tests (include/gelato_amd.h gel_interp_*): problems of chosen node counts,
random decision vectors, and the reference every product is held to -- W @ X in np.longdouble from the plan's OWN matrices,
packed like the output, with the bound of an fp64 dot product of k terms whose factors are given:
  |fl(sum_i w_i x_i) - sum_i w_i x_i| <= gamma_k sum_i |w_i| |x_i|,   gamma_k = k u / (1 - k u),  u = 2^-53
(an fma chain of n_s + 1 terms from +0.0 rounds n_s + 1 times; the tests allow gamma_{n_s + 2}: one more for the longdouble
reference's own rounding)."""
import numpy as np

from mesh_truth import phase_state

U = 2.0 ** -53
LD = np.longdouble


def gamma(k):
    return k * U / (1.0 - k * U)


def named(name):
    """(prob, x0) of a named configuration, or of states.ragged_state()"""
    from gelato_amd import con_dynamics, pack_x, problem
    if name == "ragged":
        import states
        return states.ragged_state()
    pdict, unitdict, _c, xdict = problem.make_problem(name)
    return dict(con_dynamics.problem_arrays(pdict, unitdict)), pack_x(xdict)


_BASE = []


def prob_of(nn):
    """the example problem's static data resized to len(nn) phases of nn nodes"""
    from gelato_amd import con_dynamics, problem
    if not _BASE:
        pdict, unitdict, _c, _x = problem.make_problem("example")
        _BASE.append(dict(con_dynamics.problem_arrays(pdict, unitdict)))
    prob = dict(_BASE[0])
    for k in ("thrust", "massflow", "reference_area", "nozzle_area", "engine_on", "attitude_hold"):
        prob[k] = np.resize(prob[k], len(nn))
    prob["num_nodes"] = np.array(nn, dtype=np.int32)
    return prob


def with_nodes(prob, nn):
    out = dict(prob)
    out["num_nodes"] = np.array(nn, dtype=np.int32)
    return out


def targets(name, nn):
    """destination node counts of the named transfers: per-phase changes that include +3, 0 (all copies), -2 and +8 on the example"""
    if name == "example":
        d = [3, 0, -2, 8]
        return [max(2, n + d[i % 4]) for i, n in enumerate(nn)]
    if name == "mixed-6x64":
        return [80, 64, 72, 64, 96, 60]
    if name == "stress-12x128":
        return [136] * 12
    return [n + 3 for n in nn]


def engine(prob, device=-1, **kw):
    from gelato_amd import Engine
    return Engine(prob, device=device, **kw)


def random_x(E, seed=0):
    """a decision vector of E's layout with O(1) entries of both signs, unit quaternions, increasing t"""
    rng = np.random.default_rng(1000 + seed)
    M, N, S = E.M, E.N, E.S
    q = rng.standard_normal((M, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.concatenate([0.2 + rng.random(M), rng.standard_normal(3 * M), 3.0 * rng.standard_normal(3 * M), q.ravel(),
                           rng.standard_normal(2 * N), np.sort(rng.random(S + 1))])


def pack(Xs, Us, t):
    """per-phase X [n+1, 11] and U [n, 2] and t [S+1] -> packed decision vector (any dtype)"""
    X, Uc = np.concatenate(Xs), np.concatenate(Us)
    return np.concatenate([X[:, 0], X[:, 1:4].ravel(), X[:, 4:7].ravel(), X[:, 7:11].ravel(), Uc.ravel(), np.asarray(t, dtype=X.dtype)])


def reference(plan, E, x):
    """-> (ref, scale, is_copy): W @ X in longdouble from the plan's matrices, sum |W| |X|, and the copy mask, each laid out like
    the plan's output for ONE vector ([npts, 14] or the packed destination).  Copies and t (and the time column, from its
    expression) are exact in ref and have scale 0."""
    S = E.S
    tk = x[11 * E.M + 2 * E.N:]
    Xs, Us, Ss, Su, Cx, Cu = [], [], [], [], [], []
    for s in range(S):
        m = plan.matrices(s)
        X, Uc, _to, _tf = phase_state(E, x, s)
        rx = m["Wx"].astype(LD) @ X.astype(LD)
        ru = m["Wu"].astype(LD) @ Uc.astype(LD)
        sx = np.abs(m["Wx"]) @ np.abs(X)
        su = np.abs(m["Wu"]) @ np.abs(Uc)
        cx, cu = m["copy_x"] >= 0, m["copy_u"] >= 0
        rx[cx], sx[cx] = X[m["copy_x"][cx]], 0.0
        ru[cu], su[cu] = Uc[m["copy_u"][cu]], 0.0
        Xs.append(rx); Us.append(ru); Ss.append(sx); Su.append(su)
        Cx.append(np.repeat(cx[:, None], 11, axis=1)); Cu.append(np.repeat(cu[:, None], 2, axis=1))
    if plan.mode == 1:
        return (pack(Xs, Us, tk.astype(LD)), pack(Ss, Su, np.zeros(S + 1)),
                pack([c.astype(float) for c in Cx], [c.astype(float) for c in Cu], np.ones(S + 1)) > 0)
    rows = sum(X.shape[0] for X in Xs)
    ref, sc, cp = np.zeros((rows, 14), dtype=LD), np.zeros((rows, 14)), np.zeros((rows, 14), dtype=bool)
    r = 0
    for s in range(S):
        P = Xs[s].shape[0]
        ref[r:r + P, 1:12], ref[r:r + P, 12:] = Xs[s], Us[s]
        sc[r:r + P, 1:12], sc[r:r + P, 12:] = Ss[s], Su[s]
        cp[r:r + P, 1:12], cp[r:r + P, 12:] = Cx[s], Cu[s]
        r += P
    return ref, sc, cp


def table_times(points, E, x):
    """column 0 of table mode: sigma (tf - to) / 2 + (tf + to) / 2 in fp64, the engine's expression"""
    tk = x[11 * E.M + 2 * E.N:]
    return np.concatenate([np.asarray(p, dtype=float) * (tk[s + 1] - tk[s]) / 2 + (tk[s + 1] + tk[s]) / 2 for s, p in enumerate(points)])


def quat_slice(E_dst):
    M = E_dst.M
    return slice(7 * M, 11 * M)

#!/usr/bin/env python3
"""Ground truth of the node-function rows' Jacobians (tests/golden/g22_exact_rows_jac.npz) for tests/test_exact_rows_jac.py.

Needs mpmath (build container only; the tests read the .npz).  Every node function of the row table (include/gelato_amd.h,
gel_rows_configure: fn 0 .. 15) is restated here in 60-digit arithmetic -- the orbit energy / angular momentum / inclination of
the terminal rows, the orbital elements, |r|, |v|, the geodetic latitude / longitude / altitude (Bowring's one step), the
instantaneous impact point (FAA algorithm, exactly five steps), the antenna elevation and the Vincenty downrange (iterated until
|d lambda| < 1e-50, so the truth is the derivative of the converged distance).  Inputs are the fp64 products the kernel forms
(r = fl(x unit_position), v = fl(x unit_velocity), t = fl(x_t unit_t)) taken as exact numbers, so input rounding drops out of the
comparison.  Each row is differentiated with respect to the normalised columns (position xyz, velocity xyz of the row's node, its
knot time) by differences with h = 1e-25: the central quotient and both one-sided ones are kept; where the one-sided ones disagree
(a jump or kink within h) the entry is marked `kink`.  The stored truth is s (df / dx_c) / p[0] (s = -1 with mode & 8), what a
handle with GEL_FLAG_EXACT_ROWS_JAC writes into jfn.

Cases (all on the shipped example problem, tests/exact_rows_truth.py):
  g11        the terminal rows of G11's three terminal conditions and the user example row (fn 5) on G11's two vectors;
  g13, g13b  the waypoint / impact-point / antenna rows of G13 and the downrange rows of G13b on their decision vectors;
  synthetic  every fn 0 .. 15 at the first state node of every section, modes cycling over every bit, tcol >= 0 and (fn 0 .. 8)
             < 0;
  corners    an impact point without a solution (orbital state), an exactly equatorial orbit (inclination), a position on the
             polar axis (latitude / longitude / altitude / downrange) and a downrange row at the launch longitude; `conv` marks
             the entries fixed by a convention (compared for exact zeros, not with the quotients).

Per case: fn, node, tcol, mode [R], p [R, 8], x [B, nvars], f [B, R] (the function values), Tc, Tf, Tb [B, R, 7], kink [B, R, 7],
conv [B, R, 7], and trunc [B, R]: for the downrange rows, the relative change of the row's derivative between Vincenty's loop
stopped as the value code stops it (|d lambda| < 1e-12) and converged -- the conditioning figure of the rows near the launch point.

Usage:  python tests/golden/make_exact_rows_jac.py"""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from mpmath import mp, mpf  # noqa: E402

DPS, H = 60, "1e-25"
MU, OMEGA = mpf("3.986004418e14"), mpf("7.2921151467e-5")
RA = mpf(6378137)
FL = 1 / mpf("298.257223563")
RB = RA * (1 - FL)
E2 = (RA * RA - RB * RB) / RA / RA
EP2 = (RA * RA - RB * RB) / RB / RB


def geodetic(x, y, z):
    """Bowring's one step (src/Earth.cpp:49-61): latitude [rad], longitude [rad], altitude [m]"""
    p = mp.sqrt(x * x + y * y)
    th = mp.atan2(z * RA, p * RB)
    lat = mp.atan2(z + EP2 * RB * mp.sin(th) ** 3, p - E2 * RA * mp.cos(th) ** 3)
    lon = mp.atan2(y, x)
    N = RA / mp.sqrt(1 - E2 * mp.sin(lat) ** 2)
    return lat, lon, p / mp.cos(lat) - N


def iip(pe, ve):
    """FAA impact point, five steps (lib/IIP.py posLLH_IIP_FAA, fill_na): (lat, lon) [deg], (0, 0) without a solution"""
    a, b = RA, RB
    e2 = 2 * FL - FL * FL
    r_k1 = b
    r0 = mp.sqrt(sum(c * c for c in pe))
    if r0 < r_k1:
        return mpf(0), mpf(0)
    vi = [ve[0] - OMEGA * pe[1], ve[1] + OMEGA * pe[0], ve[2]]
    v0 = mp.sqrt(sum(c * c for c in vi))
    eps_cos = r0 * v0 * v0 / MU - 1
    if eps_cos >= 1:
        return mpf(0), mpf(0)
    a_t = r0 / (1 - eps_cos)
    eps_sin = sum(p_ * v_ for p_, v_ in zip(pe, vi)) / mp.sqrt(MU * a_t)
    eps2 = eps_cos ** 2 + eps_sin ** 2
    if mp.sqrt(eps2) <= 1 and a_t * (1 - mp.sqrt(eps2)) - a >= 0:
        return mpf(0), mpf(0)
    root = mp.sqrt(a_t ** 3 / MU)
    for _ in range(5):
        eps_k_cos = (a_t - r_k1) / a_t
        if eps2 - eps_k_cos ** 2 < 0:
            return mpf(0), mpf(0)
        eps_k_sin = -mp.sqrt(eps2 - eps_k_cos ** 2)
        dcos = (eps_k_cos * eps_cos + eps_k_sin * eps_sin) / eps2
        dsin = (eps_k_sin * eps_cos - eps_k_cos * eps_sin) / eps2
        fs = (dcos - eps_cos) / (1 - eps_cos)
        gs = (dsin + eps_sin - eps_k_sin) * root
        Ek, Fk, Gk = (fs * pe[i] + gs * vi[i] for i in range(3))
        r_k2 = a / mp.sqrt(e2 / (1 - e2) * (Gk / r_k1) ** 2 + 1)
        r_prev, r_k1 = r_k1, r_k2
    if abs(r_prev - r_k2) > 1:
        return mpf(0), mpf(0)
    time_sec = (mp.atan2(dsin, dcos) + eps_sin - eps_k_sin) * root
    phi = mp.atan2(mp.tan(mp.asin(Gk / r_k2)), 1 - e2)
    lam = mp.atan2(Fk, Ek) - OMEGA * time_sec
    return phi * 180 / mp.pi, lam * 180 / mp.pi


def vincenty(lat_o, lon_o, lat_t, lon_t, stop="1e-50"):
    """Vincenty's inverse formula (lib/downrange.py:32-111) iterated to |d lambda| < stop [m]"""
    lat1, lon1, lat2, lon2 = (v * mp.pi / 180 for v in (lat_o, lon_o, lat_t, lon_t))
    if lon2 - lon1 == 0:
        return mpf(0)
    U1, U2 = mp.atan((1 - FL) * mp.tan(lat1)), mp.atan((1 - FL) * mp.tan(lat2))
    sU1, cU1, sU2, cU2 = mp.sin(U1), mp.cos(U1), mp.sin(U2), mp.cos(U2)
    dl = lon2 - lon1
    lam = dl
    for _ in range(1000):
        sl, cl = mp.sin(lam), mp.cos(lam)
        sin_sigma = mp.sqrt((cU2 * sl) ** 2 + (cU1 * sU2 - sU1 * cU2 * cl) ** 2)
        cos_sigma = sU1 * sU2 + cU1 * cU2 * cl
        sigma = mp.atan2(sin_sigma, cos_sigma)
        sin_alpha = cU1 * cU2 * sl / sin_sigma
        ca2 = 1 - sin_alpha ** 2
        cos_2sm = cos_sigma - 2 * sU1 * sU2 / ca2
        C = FL / 16 * ca2 * (4 + FL * (4 - 3 * ca2))
        prev = lam
        # the reference's update has (-1 + 2 cos_2sm) here, not Vincenty's cos_2sm^2: restated as the product computes it
        lam = dl + (1 - C) * FL * sin_alpha * (sigma + C * sin_sigma * (cos_2sm + C * cos_sigma * (-1 + 2 * cos_2sm)))
        if abs(lam - prev) < mpf(stop):
            break
    else:
        raise RuntimeError("Vincenty did not converge")
    u2 = ca2 * (RA * RA - RB * RB) / (RB * RB)
    A = 1 + u2 / 16384 * (4096 + u2 * (-768 + u2 * (320 - 175 * u2)))
    Bc = u2 / 1024 * (256 + u2 * (-128 + u2 * (74 - 47 * u2)))
    ds = Bc * sin_sigma * (cos_2sm + Bc / 4 * (cos_sigma * (-1 + 2 * cos_2sm ** 2) -
                                                Bc / 6 * cos_2sm * (-3 + 4 * sin_sigma ** 2) * (-3 + 4 * cos_2sm ** 2)))
    return RB * A * (sigma - ds)


def node_fn(fn, r, v, t, p, stop="1e-50"):
    """gel_rows_body.h node_fn in exact arithmetic (r, v [SI], t [s], row parameters p as mpf)"""
    if fn >= 9:
        sn, cs = mp.sin(OMEGA * t), mp.cos(OMEGA * t)
        pe = [r[0] * cs + r[1] * sn, -r[0] * sn + r[1] * cs, r[2]]
        if fn <= 11 or fn == 15:
            lat, lon, alt = geodetic(*pe)
            if fn == 15:
                return vincenty(p[2], p[3], lat * 180 / mp.pi, lon * 180 / mp.pi, stop)
            return (lat * 180 / mp.pi, lon * 180 / mp.pi, alt)[fn - 9]
        if fn <= 13:
            d0, d1 = v[0] + OMEGA * r[1], v[1] - OMEGA * r[0]
            ve = [d0 * cs + d1 * sn, -d0 * sn + d1 * cs, v[2]]
            return iip(pe, ve)[fn - 12]
        d = [pe[i] - p[2 + i] for i in range(3)]
        dn = mp.sqrt(sum(c * c for c in d))
        return sum(d[i] / dn * p[5 + i] for i in range(3))
    rn, vn = mp.sqrt(sum(c * c for c in r)), mp.sqrt(sum(c * c for c in v))
    if fn == 0:
        return vn * vn / 2 - MU / rn
    if fn == 7:
        return rn
    if fn == 8:
        return vn
    c = [r[1] * v[2] - r[2] * v[1], r[2] * v[0] - r[0] * v[2], r[0] * v[1] - r[1] * v[0]]
    cn = mp.sqrt(sum(q * q for q in c))
    if fn == 1:
        return cn
    if fn == 2:
        return mp.acos(c[2] / cn)
    f = [v[1] * c[2] - v[2] * c[1] - MU * r[0] / rn, v[2] * c[0] - v[0] * c[2] - MU * r[1] / rn,
         v[0] * c[1] - v[1] * c[0] - MU * r[2] / rn]
    e = mp.sqrt(sum(q * q for q in f)) / MU
    if fn == 4:
        return e
    a = cn * cn / MU / (1 - e * e)
    return {3: a, 5: a * (1 - e), 6: a * (1 + e)}[fn]


def _reads(fn, tcol, c):
    """does column c enter the row's function (the kernel's exact zeros are the columns it does not read)"""
    if c == 6:
        return fn >= 9 and tcol >= 0
    if c >= 3:
        return fn <= 8 or fn in (12, 13)
    return True


def truth_row(args):
    fn, node, tcol, mode, p, xb, M, N, units = args
    up, uv, ut = (mpf(float(u)) for u in units)
    # the fp64 products the kernel forms, as exact numbers
    r0 = [mpf(float(np.float64(xb[M + 3 * node + k]) * np.float64(units[0]))) for k in range(3)]
    v0 = [mpf(float(np.float64(xb[4 * M + 3 * node + k]) * np.float64(units[1]))) for k in range(3)]
    t0 = mpf(float(np.float64(xb[11 * M + 2 * N + tcol]) * np.float64(units[2]))) if tcol >= 0 else mpf(0)
    pm = [mpf(float(q)) for q in p]
    h = mpf(H)

    def f_at(c, s, stop="1e-50"):
        r, v, t = list(r0), list(v0), t0
        if c < 3:
            r[c] += s * h * up
        elif c < 6:
            v[c - 3] += s * h * uv
        else:
            t += s * h * ut
        return node_fn(fn, r, v, t, pm, stop)

    fc = node_fn(fn, r0, v0, t0, pm)
    sgn = -1 if mode & 8 else 1
    out = np.zeros((3, 7))
    for c in range(7):
        if not _reads(fn, tcol, c):
            continue
        fp, fm = f_at(c, 1), f_at(c, -1)
        out[0, c] = float(sgn * (fp - fm) / (2 * h) / pm[0])
        out[1, c] = float(sgn * (fp - fc) / h / pm[0])
        out[2, c] = float(sgn * (fc - fm) / h / pm[0])
    # downrange: the value code stops Vincenty's loop at |d lambda| < 1e-12 rad, an ABSOLUTE step; near the launch point (lambda
    # itself ~1e-8 rad or less) that is after one or two trips, and the distance's derivative then differs from the converged one by
    # ~f^trips of itself.  trunc = max_c |T(stopped as the value code stops) - T(converged)| / max_c |T(converged)| of the row
    trunc = 0.0
    if fn == 15 and np.abs(out[0]).max() > 0:
        tk = [float(sgn * (f_at(c, 1, "1e-12") - f_at(c, -1, "1e-12")) / (2 * h) / pm[0]) if _reads(fn, tcol, c) else 0.0
              for c in range(7)]
        trunc = float(np.abs(np.array(tk) - out[0]).max() / np.abs(out[0]).max())
    return float(fc), out, trunc


def example():
    from gelato_amd import problem
    pdict, unitdict, condition, xdict = problem.make_problem("example")
    pdict["device"] = -1
    return pdict, unitdict, condition, xdict


def table_of(condition, user_rows=()):
    """the long-form node-function rows the product builds for this condition (con_init_terminal_knot._Rows)"""
    from gelato_amd import con_init_terminal_knot as ck
    from gelato_amd.engine import Engine
    pdict, unitdict, _, _ = example()
    R = ck._Rows(pdict, unitdict, condition, user_rows)
    rows = []
    for row in R.fn:
        if len(row) == 4:
            f, node, p0, p1 = row
            tcol, mode, pp = -1, 0, [p0, p1]
        else:
            f, node, tcol, mode, pp = row
        rows.append((int(Engine.NODE_FUNCTIONS.get(f, f)), int(node), int(tcol), int(mode),
                     [float(q) for q in pp] + [0.0] * (8 - len(pp))))
    return rows


def load(name):
    return np.load(os.path.join(HERE, name), allow_pickle=False)


def cases():
    from gelato_amd import pack_x
    from gelato_amd import con_waypoint as cw
    pdict, unitdict, condition, xdict = example()
    S, M = pdict["num_sections"], pdict["M"]
    ps, ev = pdict["ps_params"], pdict["event_index"]
    xa = [ps.index_start_x(i) for i in range(S)]
    out = {}
    # G11: terminal rows of the three terminal conditions, and the user example row (fn 5 at the knot opening IIP_END)
    g = load("g11_knot_terminal.npz")
    conds = [{}, {"OptimizationMode": "Other", "inclination": 42.3}, {"altitude_perigee": None, "altitude_apogee": None}]
    rows = []
    for cd in conds:
        rows += table_of(dict(condition, **cd))
    rows.append((5, xa[ev["IIP_END"]], -1, 0, [6378137.0, 1.0] + [0.0] * 6))
    out["g11"] = (rows, np.vstack([g["x_init"], g["x_moved"]]))
    # G13: waypoint, impact-point and antenna rows; G13b: downrange rows
    for name, fx in (("g13", "g13_waypoint.npz"), ("g13b", "g13b_downrange.npz")):
        g = load(fx)
        rows = []
        for cd in json.loads(str(g["conds_json"])).values():
            cond = dict(condition, **cd)
            if name == "g13b":
                cond["antenna"] = {}
            rows += [(int(r[0]), int(r[1]), int(r[2]), int(r[3]), list(r[4]))
                     for r in (table_of(cond)[k] for k in range(len(table_of(cond))))
                     if r[0] >= 9]
        out[name] = (rows, np.vstack([g["x_init"], g["x_moved"]]))
    # synthetic: every fn at every section's first node, modes cycling over the bits, tcol >= 0 and < 0
    ant = cw._geodetic2ecef(36.0, 140.0, 300.0)
    up = cw._vertical(ant)
    lc = pdict["LaunchCondition"]
    modes = [0, 1, 4, 5, 8, 9, 12, 13]
    P = {0: [-3.0e7, 1.0], 1: [5.0e10, 1.0], 2: [1.0, 0.5], 3: [7.0e6, 1.0], 4: [1.0, 0.1], 5: [6378137.0, 1.0], 6: [6378137.0, 1.0],
         7: [6378137.0, 1.0], 8: [7800.0, 1.0], 9: [90.0, 30.0], 10: [180.0, 140.0], 11: [1.0e5, 1.0], 12: [90.0, 30.0],
         13: [180.0, 150.0], 14: [1.0, 0.1, *ant, *up], 15: [1.0e6, 1.0, float(lc["lat"]), float(lc["lon"])]}
    rows = []
    k = 0
    for sec in range(S):
        for fn in range(16):
            tcol = sec if (fn >= 9 or k % 3 == 0) else -1        # functions of the knot time need one (gel_rows_configure)
            rows.append((fn, xa[sec], tcol, modes[k % len(modes)], [float(q) for q in P[fn]] + [0.0] * (8 - len(P[fn]))))
            k += 1
    x0 = pack_x(xdict)
    rng = np.random.default_rng(22)
    X = np.vstack([x0, x0 * (1.0 + 1e-3 * rng.standard_normal(x0.size))])
    X[1, -(S + 1):] = np.sort(X[1, -(S + 1):])
    out["synthetic"] = (rows, X)
    # corners, one per node of a copy of the example vector
    xc = x0.copy()
    upos, uvel = float(unitdict["position"]), float(unitdict["velocity"])

    def put(node, r, v):
        xc[M + 3 * node:M + 3 * node + 3] = np.array(r) / upos
        xc[4 * M + 3 * node:4 * M + 3 * node + 3] = np.array(v) / uvel
    n_orbit, n_equ, n_pole, n_lon0 = xa[1], xa[2], xa[3], xa[4]
    put(n_orbit, [7.0e6, 0.0, 1.0e5], [0.0, 7600.0, 500.0])          # circular-ish orbit: positive perigee, no impact point
    put(n_equ, [6.9e6, 1.0e5, 0.0], [-100.0, 7700.0, 0.0])           # exactly in the equatorial plane: c = (0, 0, c_z)
    put(n_pole, [0.0, 0.0, 6.4e6], [10.0, 20.0, 30.0])               # on the polar axis (t = 0: ECEF = ECI)
    put(n_lon0, [6.4e6, 0.0, 1.0e6], [100.0, 200.0, 300.0])          # longitude exactly 0 (t = 0)
    xc[11 * M + 2 * pdict["N"]] = 0.0                                  # knot time 0 (tcol 0): ECEF = ECI
    z8 = [0.0] * 8
    rows = [(12, n_orbit, 1, 1, [90.0, 30.0] + z8[:6]), (13, n_orbit, 1, 4, [180.0, 150.0] + z8[:6]),
            (2, n_equ, -1, 0, [1.0, 0.5] + z8[:6]), (1, n_equ, -1, 0, [5.0e10, 1.0] + z8[:6]),
            (9, n_pole, 0, 4, [90.0, 30.0] + z8[:6]), (10, n_pole, 0, 4, [180.0, 0.0] + z8[:6]),
            (11, n_pole, 0, 4, [1.0e5, 1.0] + z8[:6]), (15, n_pole, 0, 4, [1.0e6, 1.0, 35.0, 139.0] + z8[:4]),
            (15, n_lon0, 0, 4, [1.0e6, 1.0, 30.0, 0.0] + z8[:4])]
    out["corners"] = (rows, xc[None, :])
    return out


# entries fixed by a convention in the corners case: (row, columns)
CORNER_CONV = {0: range(7), 1: range(7), 2: range(7), 4: range(7), 5: range(7), 6: range(7), 7: range(7), 8: range(7)}


def main():
    mp.dps = DPS
    pdict, unitdict, _, _ = example()
    M, N = pdict["M"], pdict["N"]
    units = [float(unitdict["position"]), float(unitdict["velocity"]), float(unitdict["t"])]
    res = {}
    t0 = time.time()
    for name, (rows, X) in cases().items():
        B, R = X.shape[0], len(rows)
        f = np.zeros((B, R))
        T = np.zeros((3, B, R, 7))
        trunc = np.zeros((B, R))
        for b in range(B):
            for i, (fn, node, tcol, mode, p) in enumerate(rows):
                f[b, i], T[:, b, i], trunc[b, i] = truth_row((fn, node, tcol, mode, p, X[b], M, N, units))
        kink = np.abs(T[1] - T[2]) > 1e-15 * (np.abs(T[0]).max(axis=2, keepdims=True) + 1e-300)
        conv = np.zeros((B, R, 7), bool)
        if name == "corners":
            for i, cols in CORNER_CONV.items():
                conv[:, i, list(cols)] = True
        res[name + "_fn"] = np.array([r[0] for r in rows], np.int32)
        res[name + "_node"] = np.array([r[1] for r in rows], np.int32)
        res[name + "_tcol"] = np.array([r[2] for r in rows], np.int32)
        res[name + "_mode"] = np.array([r[3] for r in rows], np.int32)
        res[name + "_p"] = np.array([r[4] for r in rows], np.float64)
        res[name + "_x"] = X
        res[name + "_f"] = f
        res[name + "_Tc"], res[name + "_Tf"], res[name + "_Tb"] = T
        res[name + "_kink"] = kink
        res[name + "_conv"] = conv
        res[name + "_trunc"] = trunc
        print("%-10s rows %3d  vectors %d  kinks %d  (%.0f s)" % (name, R, B, int(kink.sum()), time.time() - t0))
    res["units"] = np.array(units)
    path = os.path.join(HERE, "g22_exact_rows_jac.npz")
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

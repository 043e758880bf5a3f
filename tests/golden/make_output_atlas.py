#!/usr/bin/env python3
"""Ground truth of the output table's atlas (tests/golden/g26_output_atlas.npz) for tests/test_output_atlas_cpu.py and
tests/test_output_atlas.py.  Needs mpmath and the reference checkout (build container only; the tests read the .npz).

Written for the three handles of tests/output_atlas.py (M = 129, 64, 3):
  (a) the inputs: x, tx, tu, the two tables, units, launch point, phase parameters, the tags of every node;
  (b) the reference's own table: its output_result run on a hand-made pdict through the aliases make_golden.py uses for G14 (the
      pure-Python twins, lib/downrange.py) -- every column it returns, as data;
  (c) T [node, column]: the reference's algorithm restated in 50-digit arithmetic, branch for branch; the impact point takes five
      steps as the reference does, Vincenty is iterated to convergence, the atmosphere / wind / CA lookups are restated from the
      same constants (the fp64 numbers the reference's literals denote, taken as exact).  Inputs are the fp64 products the kernel
      forms, fl(x unit), taken as exact numbers;
  (d) s [node, column] = |T| + sum_j |dT/dz_j| |z_j| over the node's scalar inputs z (mass, position, velocity, quaternion, time,
      the launch point, the two rows of each table the lookup interpolates between), by differences with a 1e-20 relative step
      and the centre's branch decisions held; plus, for the columns that come out of acos / asin of a rounded scalar product
      (inclination, argument of perigee, true anomaly, pitch, flight-path angle, total angle of attack, Q alpha, the impact
      latitude), the conditioning the input scale does not see: sum_i |a_i b_i| / sqrt(max(1 - c^2, 2u)) -- one rounding of the
      argument c moves the angle by u / sqrt(1 - c^2), and by sqrt(2u) at the ends, whatever the inputs' own sensitivity is.
      Two more of the same kind: a = p / (1 - e^2) -- one rounding of e^2 moves a, hence apogee and perigee, by a u e^2 / |1 - e^2|,
      large on a near-radial trajectory whose apogee itself is well conditioned; and the components of a rotated vector (ground
      velocity in NED, thrust direction, axial force and acceleration) -- a quaternion rotation is backward stable in the norm of
      the vector, not in each component, so |v| is added (an exactly equatorial orbit has north velocity 0 with zero input scale);
      and, outside the atlas, the reference's table at the state that is gimbal lock in exact arithmetic only (output_atlas.edge);
  (e) the margin of every branch predicate at every node: |argument - threshold| / (u s_argument), NaN where the predicate is not
      evaluated.

Conditions asserted here: every predicate with a jump across its threshold is decided exactly by construction (the node says
which) or has a margin >= 1e6; the reference raises on no state; every tag's defining property holds (output_atlas.validate).
K_col = max over nodes |oracle - T| / (u s), the cost of the reference's fp64 algorithm on this libm, is stored next to them.

Usage:  python tests/golden/make_output_atlas.py"""
import importlib
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

from mpmath import mp, mpf  # noqa: E402

import output_atlas as oa  # noqa: E402
from oracle import output_table as ot  # noqa: E402

mp.dps = 50
U = mpf(2) ** -53
REL = mpf("1e-20")
F = mpf  # fp64 literal -> the exact number it denotes
MU, OMEGA, RA = F(3.986004418e14), F(7.2921151467e-5), F(6378137.0)
FL = 1 / F(298.257223563)
RB = RA * (1 - FL)
E2 = (RA * RA - RB * RB) / RA / RA
EP2 = (RA * RA - RB * RB) / RB / RB
DEG = 180 / mp.pi
# the reference's stopping rule |d lambda| < 1e-12 with a contraction factor below 2f away from the antipode
DOWNRANGE_TERM = float(RB * mpf("1e-12") * 2 * FL / (1 - 2 * FL))
ATM = [[F(v) for v in row] for row in (
    [0.0, -0.0065, 288.15, 101325.0, 28.9644], [11000.0, 0.0, 216.65, 22632.0, 28.9644], [20000.0, 0.001, 216.65, 5474.9, 28.9644],
    [32000.0, 0.0028, 228.65, 868.02, 28.9644], [47000.0, 0.0, 270.65, 110.91, 28.9644], [51000.0, -0.0028, 270.65, 66.939, 28.9644],
    [71000.0, -0.002, 214.65, 3.9564, 28.9644], [86000.0, 0.0, 186.8673, 0.37338, 28.9522], [91000.0, 0.0025, 186.8673, 0.15381, 28.89],
    [110000.0, 0.012, 240.0, 7.1042e-3, 27.27], [120000.0, 0.012, 360.0, 2.5382e-3, 26.20])]
RSTAR, G0, R0 = F(8314.32), F(9.80665), F(6356766.0)
# predicates whose value is continuous across the threshold (no margin needed): the cosine test of the total angle of attack
CONTINUOUS = {"calpha"}
# outcomes no state of the atlas can have, with the reason
UNREACHABLE = {
    ("ta_neg", True): "ta comes out of acos or 2 pi - acos: never negative (dead code of the reference)",
    ("gimbal", True): "the argument is a sine: see tests/output_atlas.py, states left out",
    ("iip_conv", True): "five steps always converge below 1 m on this ellipsoid",
    ("iip_e1", False): "eps2 is the squared eccentricity and eps_cos >= 1 has already left for e >= 1",
    ("calpha", True): "exactly parallel vectors only; in fp64 the aoa_aligned node takes it by rounding, continuously",
}


class Ctx:
    """records (or replays) the branch decisions of one node evaluation and the predicates' arguments"""

    def __init__(self, replay=None):
        self.dec, self.args, self.replay, self.k = [], {}, replay, 0

    def freeze(self, name, value):
        if self.replay is not None:
            n, value = self.replay[self.k]
            assert n == name, (n, name)
            self.k += 1
        self.dec.append((name, value))
        return value

    def test(self, name, arg, op):
        """arg op 0"""
        self.args[name] = arg
        out = {"<": arg < 0, "<=": arg <= 0, ">": arg > 0, ">=": arg >= 0, "==": arg == 0}[op]
        return self.freeze(name, bool(out))


def hyp(*v):
    """Euclidean norm, exact where at most one component is non-zero"""
    nz = [c for c in v if c != 0]
    if len(nz) <= 1:
        return abs(nz[0]) if nz else mpf(0)
    return mp.sqrt(sum(c * c for c in nz))


def qmul(q, p):
    return [q[0] * p[0] - q[1] * p[1] - q[2] * p[2] - q[3] * p[3], q[1] * p[0] + q[0] * p[1] - q[3] * p[2] + q[2] * p[3],
            q[2] * p[0] + q[3] * p[1] + q[0] * p[2] - q[1] * p[3], q[3] * p[0] - q[2] * p[1] + q[1] * p[2] + q[0] * p[3]]


def qconj(q):
    return [q[0], -q[1], -q[2], -q[3]]


def qrot(q, v):
    return qmul(qconj(q), qmul([mpf(0), v[0], v[1], v[2]], q))[1:4]


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def angle_cond(terms, c):
    """what one rounding of each product of the scalar product c = sum terms does to acos(c) / asin(c), in units of u [deg]"""
    return DEG * sum(abs(x) for x in terms) / mp.sqrt(max(1 - c * c, 2 * U))


def geodetic(x, y, z):
    """lib/coordinate.py:103-128 (Bowring's one step): latitude, longitude [rad], altitude [m]"""
    p = hyp(x, y)
    th = mp.atan2(z * RA, p * RB)
    lat = mp.atan2(z + EP2 * RB * mp.sin(th) ** 3, p - E2 * RA * mp.cos(th) ** 3)
    lon = mp.atan2(y, x)
    N = RA / mp.sqrt(1 - E2 * mp.sin(lat) ** 2)
    return lat, lon, p / mp.cos(lat) - N


def interp(xq, tab, col, ctx, name):
    """np.interp: clamped ends, linear inside; the interval is part of the frozen decisions"""
    K = len(tab)
    if xq <= tab[0][0]:
        j = -1
    elif xq >= tab[K - 1][0]:
        j = K
    else:
        j = max(i for i in range(K - 1) if tab[i][0] <= xq)
    j = ctx.freeze(name, j)
    if j < 0:
        return tab[0][col]
    if j >= K:
        return tab[K - 1][col]
    return (tab[j + 1][col] - tab[j][col]) / (tab[j + 1][0] - tab[j][0]) * (xq - tab[j][0]) + tab[j][col]


def atmosphere(h, ctx):
    """lib/USStandardAtmosphere.py: temperature, pressure, density, speed of sound at geopotential (< 86 km) / geometric altitude"""
    k = 0
    for i in range(len(ATM)):
        if h >= ATM[i][0]:
            k = i
    near = min((row[0] for row in ATM[1:]), key=lambda b: abs(h - b))
    ctx.args["layer"] = h - near
    k = ctx.freeze("layer", k)
    HAL, LR, T0, P0, Mw = ATM[k]
    R = RSTAR / Mw
    tb = ctx.freeze("Tbranch", 0 if h <= 91000 else 1 if h <= 110000 else 2 if h <= 120000 else 3)
    if tb == 0 or tb == 2:
        T = T0 + LR * (h - HAL)
    elif tb == 1:
        T = F(263.1905) + F(-76.3232) * mp.sqrt(1 - (h - 91000) ** 2 / F(-19942.9) ** 2)
    else:
        xi = (h - HAL) * (R0 + HAL) / (R0 + h)
        T = 1000 - (1000 - T0) * mp.exp(F(-0.01875) * F(1e-3) * xi)
    if ctx.freeze("lapse", bool(abs(LR) > F(1.0e-10))):
        P = P0 * ((T0 + LR * (h - HAL)) / T0) ** (G0 / -LR / R)
    else:
        P = P0 * mp.exp(G0 / R * (HAL - h) / T0)
    return T, P, P / R / T, mp.sqrt(F(1.4) * R * T)


def vincenty(lat_o, lon_o, lat_t, lon_t, ctx):
    """lib/downrange.py:32-111, iterated to convergence"""
    lat1, lon1, lat2, lon2 = (v * mp.pi / 180 for v in (lat_o, lon_o, lat_t, lon_t))
    if ctx.test("samelon", lon2 - lon1, "=="):
        return mpf(0)
    U1, U2 = mp.atan((1 - FL) * mp.tan(lat1)), mp.atan((1 - FL) * mp.tan(lat2))
    sU1, cU1, sU2, cU2 = mp.sin(U1), mp.cos(U1), mp.sin(U2), mp.cos(U2)
    dl = lon2 - lon1
    lam = dl
    for _ in range(400):
        sl, cl = mp.sin(lam), mp.cos(lam)
        sin_sigma = mp.sqrt((cU2 * sl) ** 2 + (cU1 * sU2 - sU1 * cU2 * cl) ** 2)
        cos_sigma = sU1 * sU2 + cU1 * cU2 * cl
        sigma = mp.atan2(sin_sigma, cos_sigma)
        sin_alpha = cU1 * cU2 * sl / sin_sigma
        ca2 = 1 - sin_alpha ** 2
        cos_2sm = cos_sigma - 2 * sU1 * sU2 / ca2
        C = FL / 16 * ca2 * (4 + FL * (4 - 3 * ca2))
        prev = lam
        # the reference's update has (-1 + 2 cos_2sm) here, not Vincenty's cos_2sm^2: restated as the reference computes it
        lam = dl + (1 - C) * FL * sin_alpha * (sigma + C * sin_sigma * (cos_2sm + C * cos_sigma * (-1 + 2 * cos_2sm)))
        if abs(lam - prev) < mpf("1e-46"):
            break
    else:
        raise RuntimeError("Vincenty did not converge")
    u2 = ca2 * (RA * RA - RB * RB) / (RB * RB)
    A = 1 + u2 / 16384 * (4096 + u2 * (-768 + u2 * (320 - 175 * u2)))
    Bc = u2 / 1024 * (256 + u2 * (-128 + u2 * (74 - 47 * u2)))
    ds = Bc * sin_sigma * (cos_2sm + Bc / 4 * (cos_sigma * (-1 + 2 * cos_2sm ** 2) -
                                                Bc / 6 * cos_2sm * (-3 + 4 * sin_sigma ** 2) * (-3 + 4 * cos_2sm ** 2)))
    return RB * A * (sigma - ds)


def iip(pe, ve, ctx, extra):
    """lib/IIP.py:30-136 with fill_na = False, five steps: (lat, lon) [deg] or None"""
    a, b = RA, RA * (1 - FL)
    e2 = 2 * FL - FL * FL
    r_k1 = b
    r0 = hyp(*pe)
    if ctx.test("iip_r0", r0 - r_k1, "<"):
        return None
    vi = [ve[0] - OMEGA * pe[1], ve[1] + OMEGA * pe[0], ve[2]]
    v0 = hyp(*vi)
    eps_cos = r0 * v0 ** 2 / MU - 1
    if ctx.test("iip_ecos", eps_cos - 1, ">="):
        return None
    a_t = r0 / (1 - eps_cos)
    eps_sin = dot(pe, vi) / mp.sqrt(MU * a_t)
    eps2 = eps_cos ** 2 + eps_sin ** 2
    if ctx.test("iip_e1", mp.sqrt(eps2) - 1, "<=") and ctx.test("iip_hp", a_t * (1 - mp.sqrt(eps2)) - a, ">="):
        return None
    root = mp.sqrt(a_t ** 3 / MU)
    for it in range(5):
        eps_k_cos = (a_t - r_k1) / a_t
        if ctx.test("iip_int%d" % it, eps2 - eps_k_cos ** 2, "<"):
            return None
        eps_k_sin = -mp.sqrt(eps2 - eps_k_cos ** 2)
        dcos = (eps_k_cos * eps_cos + eps_k_sin * eps_sin) / eps2
        dsin = (eps_k_sin * eps_cos - eps_k_cos * eps_sin) / eps2
        fs = (dcos - eps_cos) / (1 - eps_cos)
        gs = (dsin + eps_sin - eps_k_sin) * root
        Ek, Fk, Gk = (fs * pe[i] + gs * vi[i] for i in range(3))
        r_k2 = a / mp.sqrt(e2 / (1 - e2) * (Gk / r_k1) ** 2 + 1)
        r_prev, r_k1 = r_k1, r_k2
    if ctx.test("iip_conv", abs(r_prev - r_k2) - 1, ">"):
        return None
    time_sec = (mp.atan2(dsin, dcos) + eps_sin - eps_k_sin) * root
    phi = mp.atan2(mp.tan(mp.asin(Gk / r_k2)), 1 - e2)
    extra["lat_IIP"] = angle_cond([Gk / r_k2], Gk / r_k2)
    lam = mp.atan2(Fk, Ek) - OMEGA * time_sec
    return phi * DEG, lam * DEG


def truth_node(z, par, wind, ca, ctx):
    """output_result.py:126-262 for one node -> ({column: value | None}, {column: extra scale})"""
    mass, pos, vel, qr, t, lat0, lon0 = z["mass"], z["pos"], z["vel"], z["quat"], z["t"], z["lat0"], z["lon0"]
    thrust_vac, area, nozzle = par
    o, extra = {}, {}
    qn = hyp(*qr)
    q = [c / qn for c in qr]
    cs, sn = mp.cos(OMEGA * t), mp.sin(OMEGA * t)
    pe = [pos[0] * cs + pos[1] * sn, -pos[0] * sn + pos[1] * cs, pos[2]]
    g0, g1 = vel[0] + OMEGA * pos[1], vel[1] - OMEGA * pos[0]
    ve = [g0 * cs + g1 * sn, -g0 * sn + g1 * cs, vel[2]]
    lat, lon, alt = geodetic(*pe)
    o["lat"], o["lon"], o["altitude"] = lat * DEG, lon * DEG, alt
    h = R0 * alt / (R0 + alt) if ctx.test("z86", alt - 86000, "<") else alt
    o["downrange"] = vincenty(lat0, lon0, lat * DEG, lon * DEG, ctx)
    # orbital elements (lib/coordinate.py:591-649)
    rn = hyp(*pos)
    nr = [c / rn for c in pos]
    c = cross(pos, vel)
    f = [a - MU * b for a, b in zip(cross(vel, c), nr)]
    cn, fn = hyp(*c), hyp(*f)
    c1, f1 = [x / cn for x in c], [x / fn for x in f]
    inc = mp.acos(c1[2])
    if 1 - c1[2] ** 2 > 0:
        extra["inclination"] = angle_cond([c1[2]], c1[2])
    if ctx.test("inc", inc - F(1e-10), ">"):
        asc = mp.atan2(c1[0], -c1[1])
        terms = [mp.cos(asc) * f1[0], mp.sin(asc) * f1[1]]
        argp = mp.acos(sum(terms))
        extra["argument_perigee"] = angle_cond(terms, sum(terms))
        if ctx.test("fz", f[2], "<"):
            argp = -argp
    else:
        asc = mpf(0)
        argp = mp.atan2(f[1], f[0])
    p = cn ** 2 / MU
    e = fn / MU
    a = p / (1 - e ** 2)
    terms = [f1[i] * nr[i] for i in range(3)]
    ta = mp.acos(sum(terms))
    extra["true_anomaly"] = angle_cond(terms, sum(terms))
    if ctx.test("rv", dot(vel, pos), "<"):
        ta = 2 * mp.pi - ta
    if ctx.test("asc_neg", asc, "<"):
        asc += 2 * mp.pi
    if ctx.test("argp_neg", argp, "<"):
        argp += 2 * mp.pi
    if ctx.test("ta_neg", ta, "<"):
        ta += 2 * mp.pi
    o["altitude_apogee"], o["altitude_perigee"] = a * (1 + e) - 6378137, a * (1 - e) - 6378137
    extra["altitude_apogee"], extra["altitude_perigee"] = (abs(a * (1 + s_)) * e ** 2 / abs(1 - e ** 2) for s_ in (e, -e))
    o["inclination"], o["lon_ascending_node"], o["argument_perigee"], o["true_anomaly"] = inc * DEG, asc * DEG, argp * DEG, ta * DEG
    # ground / inertial velocity in NED (output_result.py:169-185)
    s_hl, c_hl, s_hp, c_hp = mp.sin(lon / 2), mp.cos(lon / 2), mp.sin(lat / 2), mp.cos(lat / 2)
    r2 = mp.sqrt(2)
    q_e2n = [c_hl * (c_hp - s_hp) / r2, s_hl * (c_hp + s_hp) / r2, -c_hl * (c_hp + s_hp) / r2, s_hl * (c_hp - s_hp) / r2]
    q_i2n = qmul([mp.cos(OMEGA * t / 2), mpf(0), mpf(0), mp.sin(OMEGA * t / 2)], q_e2n)
    vg_ned = qrot(q_e2n, ve)
    v_ned = qrot(q_i2n, vel)
    o["vel_ground_NED_X"], o["vel_ground_NED_Y"], o["vel_ground_NED_Z"] = vg_ned
    extra["vel_ground_NED_X"] = extra["vel_ground_NED_Y"] = extra["vel_ground_NED_Z"] = hyp(*ve)
    o["vel_ground"] = hyp(*ve)
    o["azimuth_vel_inertial_geocentric"] = mp.atan2(v_ned[1], v_ned[0]) * DEG
    sfp = -v_ned[2] / hyp(*v_ned)
    o["flightpath_vel_inertial_geocentric"] = mp.asin(sfp) * DEG
    extra["flightpath_vel_inertial_geocentric"] = angle_cond([sfp], sfp)
    T, P, rho, a_snd = atmosphere(h, ctx)
    wn, we = interp(h, wind, 1, ctx, "wind_n"), interp(h, wind, 2, ctx, "wind_e")
    va_ned = [vg_ned[0] - wn, vg_ned[1] - we, vg_ned[2]]
    qdyn = hyp(*va_ned) ** 2 * rho / 2
    o["dynamic_pressure"] = qdyn
    w_eci = qrot(qconj(q_i2n), [wn, we, mpf(0)])
    va = [(ve[0] * cs - ve[1] * sn) - w_eci[0], (ve[0] * sn + ve[1] * cs) - w_eci[1], ve[2] - w_eci[2]]
    vn = hyp(*va)
    tdir = qrot(qconj(q), [mpf(1), mpf(0), mpf(0)])
    o["thrust_direction_ECI_X"], o["thrust_direction_ECI_Y"], o["thrust_direction_ECI_Z"] = tdir
    extra["thrust_direction_ECI_X"] = extra["thrust_direction_ECI_Y"] = extra["thrust_direction_ECI_Z"] = mpf(1)
    # angles of attack (lib/utils.py:92-161); the reference tests c >= 1 first, the outcome of the pair is the same
    if ctx.test("vn", vn - F(0.001), "<"):
        a_all = mpf(0)
    else:
        tn = hyp(*tdir)
        terms = [(va[i] / vn) * (tdir[i] / tn) for i in range(3)]
        if ctx.test("calpha", sum(terms) - 1, ">="):
            a_all = mpf(0)
        else:
            a_all = mp.acos(sum(terms))
        extra["AOA_total"] = angle_cond(terms, min(sum(terms), mpf(1)))
        extra["Q_alpha"] = extra["AOA_total"] * qdyn
    o["AOA_total"], o["Q_alpha"] = a_all * 180 / mp.pi, a_all * 180 / mp.pi * qdyn
    vb = qrot(q, va)
    if ctx.test("vbx", vb[0] - F(0.001), "<"):
        o["AOA_pitch"], o["AOA_yaw"] = mpf(0), mpf(0)
    else:
        o["AOA_pitch"], o["AOA_yaw"] = mp.atan2(vb[2], vb[0]) * DEG, mp.atan2(vb[1], vb[0]) * DEG
    # euler_from_quat(quat_nedg2body) (lib/coordinate.py:488-528)
    qb = qmul(qconj(q_i2n), q)
    terms = [2 * qb[0] * qb[2], -2 * qb[3] * qb[1]]
    if ctx.test("gimbal", sum(terms) - 1, ">="):
        az, el, ro = mpf(0), mp.pi / 2, mpf(0)
    else:
        az = mp.atan2(2 * (qb[0] * qb[3] + qb[1] * qb[2]), 1 - 2 * (qb[2] ** 2 + qb[3] ** 2))
        el = mp.asin(sum(terms))
        ro = mp.atan2(2 * (qb[0] * qb[1] + qb[2] * qb[3]), 1 - 2 * (qb[1] ** 2 + qb[2] ** 2))
        extra["pitch_NED2BODY"] = angle_cond(terms, sum(terms))
    if ctx.test("az", az, "<"):
        az += 2 * mp.pi
    o["heading_NED2BODY"], o["pitch_NED2BODY"], o["roll_NED2BODY"] = az * DEG, el * DEG, ro * DEG
    # Mach number, axial force, thrust, acceleration (output_result.py:217-253)
    mach = vn / a_snd
    o["M"], o["vel_air"] = mach, vn
    cax = interp(mach, ca, 1, ctx, "ca")
    aero = [rho / 2 * vn * -va[i] * area * cax for i in range(3)]
    aero_b = qrot(q, aero)
    thrust = thrust_vac - nozzle * P
    o["thrust"], o["aero_BODY_X"], o["accel_BODY_X"] = thrust, aero_b[0], (thrust + aero_b[0]) / mass
    extra["aero_BODY_X"], extra["accel_BODY_X"] = hyp(*aero), hyp(*aero) / mass
    ll = iip(pe, ve, ctx, extra)
    o["lat_IIP"], o["lon_IIP"] = ll if ll is not None else (None, None)
    return o, extra


def node_truth(si, par, wind_np, ca_np):
    """T, s [34], {predicate: (argument, margin)}, decisions of one node; si = (mass, pos, vel, quat, t) as fp64"""
    mass, pos, vel, quat, t = si
    wind = [[F(float(v)) for v in row] for row in wind_np]
    ca = [[F(float(v)) for v in row] for row in ca_np]
    z0 = {"mass": F(float(mass)), "pos": [F(float(v)) for v in pos], "vel": [F(float(v)) for v in vel],
          "quat": [F(float(v)) for v in quat], "t": F(float(t)), "lat0": F(oa.LAUNCH_LAT), "lon0": F(oa.LAUNCH_LON)}
    parm = [F(float(v)) for v in par]
    ctx = Ctx()
    o0, extra = truth_node(z0, parm, wind, ca, ctx)
    dec = list(ctx.dec)
    jw = max(0, min(len(wind) - 2, dict(dec)["wind_n"]))
    jc = max(0, min(len(ca) - 2, dict(dec)["ca"]))
    inputs = [("mass", None), ("t", None), ("lat0", None), ("lon0", None)] + [(k, i) for k in ("pos", "vel") for i in range(3)] + \
        [("quat", i) for i in range(4)] + [("wind", (jw + r, cc)) for r in (0, 1) for cc in (1, 2)] + [("ca", (jc + r, 1)) for r in (0, 1)]
    cols = ot.DEVICE_COLUMNS
    s = {c: (abs(o0[c]) if o0[c] is not None else None) for c in cols}
    sa = {k: abs(v) for k, v in ctx.args.items()}
    for key, idx in inputs:
        z, w, cc = dict(z0), wind, ca
        if key == "wind" or key == "ca":
            tab = [list(r) for r in (wind if key == "wind" else ca)]
            if tab[idx[0]][idx[1]] == 0:
                continue
            tab[idx[0]][idx[1]] *= 1 + REL
            w, cc = (tab, ca) if key == "wind" else (wind, tab)
        elif idx is None:
            if z0[key] == 0:
                continue
            z[key] = z0[key] * (1 + REL)
        else:
            if z0[key][idx] == 0:
                continue
            z[key] = list(z0[key])
            z[key][idx] *= 1 + REL
        c1 = Ctx(replay=dec)
        o1, _ = truth_node(z, parm, w, cc, c1)
        for c in cols:
            if o0[c] is not None:
                s[c] += abs(o1[c] - o0[c]) / REL
        for k in sa:
            sa[k] += abs(c1.args[k] - ctx.args[k]) / REL
    for c, v in extra.items():
        if s[c] is not None:
            s[c] += v
    T = np.array([float(o0[c]) if o0[c] is not None else np.nan for c in cols])
    S = np.array([float(s[c]) if s[c] is not None else np.nan for c in cols])
    marg = {k: (float(ctx.args[k]), float(abs(ctx.args[k]) / (U * sa[k])) if sa[k] != 0 else (np.inf if ctx.args[k] != 0 else 0.0))
            for k in ctx.args}
    return T, S, marg, dec


def reference_tables(handles):
    """the reference's output_result on every handle -> {handle: DataFrame}"""
    from make_golden import import_reference
    ref = import_reference()
    ref.coordinate.distance_vincenty = importlib.import_module("lib.downrange").distance_vincenty
    sys.modules["lib.IIP_c"] = importlib.import_module("lib.IIP")
    importlib.import_module("lib.utils").distance_vincenty = ref.coordinate.distance_vincenty
    orr = importlib.import_module("output_result")
    out = {}
    for name, (x, tx, tu, nodes, wind, ca) in handles.items():
        M, N, S = sum(nodes) + len(nodes), sum(nodes), len(nodes)
        pd_ = oa.pdict_of(nodes, wind, ca, ref.sp.PSparams(nodes))
        out[name] = orr.output_result(oa.xdict_of(x, M, N, S), dict(oa.UNITS), tx.copy(), tu.copy(), pd_)
    return out


def main():
    t0 = time.time()
    A = oa.build()
    oa.validate(A)
    wind, ca = A["wind"], A["ca"]
    handles = {"big": (A["x"], A["tx"], A["tu"], oa.NODES, wind, ca)}
    for nm in oa.SMALL:
        x, tx, tu, src = oa.small(nm)
        handles[nm] = (x, tx, tu, oa.SMALL[nm], wind, ca)
    out = {"wind": wind, "ca": ca, "units": np.array([oa.UNITS[k] for k in ("mass", "position", "velocity", "u", "t")]),
           "launch": np.array([oa.LAUNCH_LAT, oa.LAUNCH_LON]), "params": np.array(oa.PARAMS), "nodes_big": np.array(oa.NODES),
           "tags": np.array(["|".join(t) for t, _, _ in A["nodes"]]), "exact": np.array(["|".join(e) for _, _, e in A["nodes"]]),
           "columns": np.array(ot.DEVICE_COLUMNS), "downrange_term": DOWNRANGE_TERM}
    xe, txe, tue = oa.edge()
    ref = reference_tables({**handles, "edge": (xe, txe, tue, oa.SMALL["m3"], wind, ca)})
    out["x_edge"], out["tx_edge"], out["tu_edge"] = xe, txe, tue
    for col in ref["edge"].columns:                      # outside the atlas: the reference's record only (output_atlas.edge)
        v = ref["edge"][col].to_numpy()
        out["ref_edge_" + col] = v.astype(str) if v.dtype == object else v
    pred_names, coverage, bad = [], {}, []
    K = np.zeros(len(ot.DEVICE_COLUMNS))
    for name, (x, tx, tu, nodes, _, _) in handles.items():
        M = sum(nodes) + len(nodes)
        sec = ot.node_sections(nodes)
        T, S, margins = np.empty((M, 34)), np.empty((M, 34)), []
        for i in range(M):
            si = oa.node_si(x, M, i) + (tx[i],)
            T[i], S[i], marg, dec = node_truth(si, oa.PARAMS[sec[i]], wind, ca)
            margins.append(marg)
            for n, v in dec:
                key = (n.rstrip("0123456789") if n.startswith("iip_int") else n, v)
                coverage[key] = coverage.get(key, 0) + 1
            exact = set(A["nodes"][i][2]) if name == "big" else None
            for k, (arg, m) in marg.items():
                if k in CONTINUOUS or exact is None:
                    continue
                if not (m >= 1e6 or (k in exact and arg == 0.0)):
                    bad.append(("margin", name, i, A["nodes"][i][0], k, arg, m))
        for k in sorted({k for m in margins for k in m}):
            if k not in pred_names:
                pred_names.append(k)
        out["x_" + name], out["tx_" + name], out["tu_" + name] = x, tx, tu
        out["T_" + name], out["s_" + name] = T, S
        out["margin_" + name] = np.array([[m.get(k, (np.nan, np.nan))[1] for k in pred_names] for m in margins])
        df = ref[name]
        out["ref_columns"] = np.array(list(df.columns))
        for col in df.columns:
            v = df[col].to_numpy()
            out["ref_%s_%s" % (name, col)] = v.astype(str) if v.dtype == object else v
        # the oracle against the truth: the cost of the reference's fp64 algorithm
        O = oa.oracle_table(x, tx, nodes, wind, ca)
        assert np.array_equal(np.isnan(O), np.isnan(T)), name
        K = np.maximum(K, k_col(O, T, S))
        print("%s: M = %d, %.0f s" % (name, M, time.time() - t0), flush=True)
    assert not bad, "\n".join(str(b) for b in bad)
    out["pred_names"] = np.array(pred_names)
    out["K_col"] = K
    cov = sorted(coverage.items(), key=lambda kv: str(kv[0]))
    out["coverage_names"] = np.array(["%s=%s" % k for k, _ in cov])
    out["coverage_counts"] = np.array([n for _, n in cov])
    out["unreachable"] = np.array(["%s=%s: %s" % (k[0], k[1], v) for k, v in UNREACHABLE.items()])
    for c, k in zip(ot.DEVICE_COLUMNS, K):
        print("  K %-40s %.3g" % (c, k))
    path = os.path.join(HERE, "g26_output_atlas.npz")
    np.savez_compressed(path, **out)
    print("wrote g26", os.path.getsize(path), "bytes")


def k_col(O, T, S, term=DOWNRANGE_TERM):
    """per column max over nodes of |O - T| / (u s), the downrange column less its stopping-rule term; 0 / 0 = 0"""
    u = 2.0 ** -53
    d = np.abs(O - T)
    d[:, ot.DEVICE_COLUMNS.index("downrange")] = np.maximum(d[:, ot.DEVICE_COLUMNS.index("downrange")] - term, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0.0, 0.0, d / (u * S))
    return np.nanmax(np.where(np.isnan(T), 0.0, r), axis=0)


if __name__ == "__main__":
    main()

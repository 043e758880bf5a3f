"""The model of the exact-difference position sweep (gelato_amd/csrc/gel_rhs_parts.h pos_delta, gel_physics.h atmosphere_delta
and wind_piece, the margin of pos_centre_tail) for tests/test_delta_model.py -- TEST INFRASTRUCTURE, two things:

  restate()  the device's formulas, series by series, in plain numpy fp64: what the ALGORITHM gives, free of the device's own
             arithmetic (its reciprocals, fused operations, libm).  Bit parity with the device is not wanted;
  truth()    the same chain recomputed at r and at r' (component kk moved by dlt, the sum exact) with oracle/exact_fd.py's geodetic,
             atmosphere and interp at 40 digits, and differenced: what the change IS.

Quantities, in the order of gel_point_eval kind 15: rho, P, 1/a, wn, we, sin(lat/2), cos(lat/2), 1/p.

The tolerance of a quantity X (tolerance()):   |dX - dX_true| <= REL[X] |dX_true| + 4 eps |X_centre|
first term: the accuracy gel_rhs_parts.h documents for the change; second: the rounding of the output (X_c + dX, one fma) and
of the centre value the change is taken from."""
import numpy as np

EPS = np.finfo(np.float64).eps
NAMES = ("rho", "P", "inv_a", "wn", "we", "shp", "chp", "inv_p")
RA = 6378137.0
RB = RA * (1.0 - 1.0 / 298.257223563)
E2 = (RA * RA - RB * RB) / RA / RA
EP2 = (RA * RA - RB * RB) / RB / RB
R0 = 6356766.0
RSTAR, G0 = 8314.32, 9.80665
HB = np.array([0.0, 11000.0, 20000.0, 32000.0, 47000.0, 51000.0, 71000.0, 86000.0, 91000.0, 110000.0, 120000.0])
LMB = np.array([-0.0065, 0.0, 0.001, 0.0028, 0.0, -0.0028, -0.002, 0.0, 0.0025, 0.012, 0.012])
TMB = np.array([288.15, 216.65, 216.65, 228.65, 270.65, 270.65, 214.65, 186.8673, 186.8673, 240.0, 360.0])
PB = np.array([101325.0, 22632.0, 5474.9, 868.02, 110.91, 66.939, 3.9564, 0.37338, 0.15381, 7.1042e-3, 2.5382e-3])
MB = np.array([28.9644, 28.9644, 28.9644, 28.9644, 28.9644, 28.9644, 28.9644, 28.9522, 28.89, 27.27, 26.20])
GEOPOT86 = 84852.0          # kGeopot86: the end of the geopotential branch, rounded down
U_LIMIT = 1.0e-4            # pos_delta's predicate on u and v
# REL: 1e-12 of the change is what gel_rhs_parts.h claimed for every quantity.  The restatement itself -- the algorithm in clean
# fp64 -- misses it in two places, both within kilometres of the polar axis (tests/test_delta_model.py measures the figures over
# inputs()); there the comment was wrong, and it and the tolerance now say twice the restatement's worst figure, as a term that
# vanishes away from the axis (rel_at()):
#   wn, we  + min(WIND_CAP, WIND_POLAR eps / cos^2 lat): the change of altitude d(p / cos lat) - dN cancels
#           (dp cos lat - p dcos) / cos^2 lat, so what its terms are off -- roundings, and at 1 m the v^3 the series of 1 / (1 + v)
#           drops -- weighs 1 / cos^2 lat.  Measured: 54 eps / cos^2 lat (89.8 deg, 1 m) and never more than 7.7e-9 (1.4 km from
#           the axis, 6.4 cm); below 80 degrees the term is under 8e-13.  Every quantity that follows the altitude shares this; only
#           a wind of 1e-22 m/s, a rounding residue of the example's table, has no output rounding above it to show it;
#   1/p     + INVP_U2 u^2: (1 + u)^-1/2 - 1 is cut after u^2 and the next term is 5/8 u^2 of the change (measured 0.623 u^2):
#           6.2e-9 at the limit |u| = 1e-4, below 1e-12 where |u| < 9e-7.
REL = 1e-12
WIND_POLAR, WIND_CAP, INVP_U2 = 108.0, 1.54e-8, 1.25
MUTANTS = ("dp_u2", "uP_e3", "hl2")


def _centre(r, wind):
    """the centre evaluation as pos_part<CENTRE> and pos_centre_tail leave it (fp64, formula by formula)"""
    x, y, z = r[:, 0], r[:, 1], r[:, 2]
    c = {}
    p = np.sqrt(x * x + y * y)
    c["p"], c["inv_p"] = p, 1.0 / p
    a, b = z * RA, p * RB
    c["ih"] = 1.0 / np.sqrt(a * a + b * b)
    st, ct = a * c["ih"], b * c["ih"]
    zz, pp = z + EP2 * RB * st ** 3, p - E2 * RA * ct ** 3
    c["ihy"] = 1.0 / np.sqrt(zz * zz + pp * pp)
    sl, cl = zz * c["ihy"], pp * c["ihy"]
    c["sl"], c["cl"] = sl, cl
    c["chp"] = np.sqrt(0.5 * (1.0 + cl))
    c["shp"] = 0.5 * sl / c["chp"]
    c["N"] = RA / np.sqrt(1.0 - E2 * sl * sl)
    q = p / cl
    alt = q - c["N"]
    c["icl"] = q * c["inv_p"]
    low = alt < 86000.0
    c["G"] = np.where(low, R0 / (R0 + alt), 1.0)
    h = np.where(low, R0 * alt / (R0 + alt), alt)
    c["alt"], c["h"] = alt, h
    k = np.searchsorted(HB[1:], h, side="right")
    c["k"] = k
    Hb, Lmb, Tmb, Pb, R = HB[k], LMB[k], TMB[k], PB[k], RSTAR / MB[k]
    Tl = Tmb + Lmb * (h - Hb)
    with np.errstate(all="ignore"):
        T = np.where(h <= 91000.0, Tl, np.where(h <= 110000.0, 263.1905 - 76.3232 * np.sqrt(np.maximum(1.0 - ((h - 91000.0) / -19942.9) ** 2, 0.0)),
                     np.where(h <= 120000.0, Tl, 1000.0 - (1000.0 - Tmb) * np.exp(-0.01875e-3 * (h - Hb) * (R0 + Hb) / (R0 + h)))))
        lapse = np.abs(Lmb) > 1.0e-6
        P = np.where(lapse, Pb * np.power(Tl / Tmb, -G0 / np.where(lapse, Lmb, 1.0) / R), Pb * np.exp(G0 / R * (Hb - h) / Tmb))
    c["T"], c["P"], c["rho"], c["inv_a"] = T, P, P / R / T, 1.0 / np.sqrt(1.4 * R * T)
    c["Tl"], c["R"] = Tl, R
    # wind: the piece xp[i] < h <= xp[i + 1], clamped below (h <= xp[0]) and above; wind_piece's slopes and margin
    xp = wind[:, 0]
    n = len(xp)
    below, above = h <= xp[0], h > xp[-1]
    i = np.clip(np.searchsorted(xp, h, side="left") - 1, 0, n - 2)
    inside = ~below & ~above
    s = (wind[1:, 1:] - wind[:-1, 1:]) / (xp[1:] - xp[:-1])[:, None]
    for col, key, sk in ((1, "wn", "s0"), (2, "we", "s1")):
        c[key] = np.where(below, wind[0, col], np.where(above, wind[-1, col], wind[i, col] + (h - xp[i]) * s[i, col - 1]))
        c[sk] = np.where(inside, s[i, col - 1], 0.0)
    wm = np.where(below, xp[0] - h, np.where(above, h - xp[-1], np.minimum(h - xp[i], xp[i + 1] - h)))
    lo = np.where(k == 0, -1.0e300, HB[k])
    hi = np.where(k == 6, GEOPOT86, np.where(k < 10, HB[np.minimum(k + 1, 10)], 1.0e300))
    c["margin"] = np.minimum(wm, np.minimum(h - lo, hi - h))
    return c


def restate(r, kk, dlt, wind, mutant=None):
    """-> (centre [n, 8], perturbed [n, 8], ok [n] bool, margin [n]): pos_delta after pos_part<CENTRE> and pos_centre_tail, the
    series as the device cuts them.  mutant: one of MUTANTS -- a series with one term dropped (the teeth of the test)"""
    r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
    kk = np.asarray(kk).astype(int)
    dlt = np.asarray(dlt, dtype=np.float64)
    wind = np.asarray(wind, dtype=np.float64)
    c = _centre(r, wind)
    along_z = kk == 2
    a, b = r[:, 2] * RA, c["p"] * RB
    ih = c["ih"]
    xs = np.where(kk == 0, r[:, 0], r[:, 1])
    dp2 = np.where(along_z, 0.0, dlt * (2.0 * xs + dlt))
    u = dp2 * c["inv_p"] * c["inv_p"]
    dp = (0.5 * dp2 * c["inv_p"]) * (1.0 + u * (-0.25 + (0.0 if mutant == "dp_u2" else 0.125) * u))
    inv_p1 = c["inv_p"] * (1.0 + u * (-0.5 + 0.375 * u))
    db = dp * RB
    da = np.where(along_z, dlt * RA, 0.0)
    dh2 = da * (2.0 * a + da) + db * (2.0 * b + db)
    uh = dh2 * ih * ih
    dih = ih * (uh * (-0.5 + 0.375 * uh))
    ih1 = ih + dih
    dst = da * ih1 + a * dih
    dct = db * ih1 + b * dih
    st, ct = a * ih, b * ih
    dst3 = dst * (3.0 * st * (st + dst) + dst * dst)
    dct3 = dct * (3.0 * ct * (ct + dct) + dct * dct)
    dzz = np.where(along_z, dlt, 0.0) + (EP2 * RB) * dst3
    dpp = dp - (E2 * RA) * dct3
    sl, cl = c["sl"], c["cl"]
    e = (cl * dpp + sl * dzz) * c["ihy"]
    dlat = ((dzz * cl - dpp * sl) * c["ihy"]) * (1.0 + e * (e - 1.0))
    hl2 = 0.0 if mutant == "hl2" else 0.5 * dlat * dlat
    dsl, dcl = cl * dlat - sl * hl2, -(sl * dlat + cl * hl2)
    hd = 0.5 * dlat
    hd2 = 0.5 * hd * hd
    shp1 = c["shp"] + (c["chp"] * hd - c["shp"] * hd2)
    chp1 = c["chp"] - (c["shp"] * hd + c["chp"] * hd2)
    v = dcl * c["icl"]
    dq = ((dp - (c["p"] * c["icl"]) * dcl) * c["icl"]) * (1.0 + v * (v - 1.0))
    nr = c["N"] / RA
    uw = (-E2 * dsl * (2.0 * sl + dsl)) * (nr * nr)
    dN = c["N"] * (uw * (-0.5 + 0.375 * uw))
    dalt = dq - dN
    g1 = np.where(c["k"] <= 6, c["G"] / R0, 0.0)
    dh = (c["G"] * c["G"]) * dalt * (1.0 - dalt * g1)
    # atmosphere_delta
    k, h, T = c["k"], c["h"], c["T"]
    iT = 1.0 / T
    Lmb = LMB[k]
    dTl = Lmb * dh
    ia = 1.0 / -19942.9
    yv, dyv = (h - 91000.0) * ia, dh * ia
    dy2 = dyv * (2.0 * yv + dyv)
    with np.errstate(all="ignore"):
        s = (T - 263.1905) / -76.3232
        us = -dy2 / (s * s)
        dT8 = (-76.3232 * s) * (us * (0.5 + us * (-0.125 + 0.0625 * us)))
        irh = 1.0 / (R0 + h)
        dxi = ((R0 + HB[10]) * (R0 + HB[10])) * dh * irh * irh * (1.0 - dh * irh)
        zc = -0.01875e-3 * dxi
        dT10 = (T - 1000.0) * (zc * (1.0 + zc * (0.5 + zc / 6.0)))
    dT = np.where(k == 8, dT8, np.where(k == 10, dT10, dTl))
    iTl = np.where((k == 8) | (k == 10), 1.0 / c["Tl"], iT)
    uT = dT * iT
    ul = dTl * iTl
    R = c["R"]
    lapse = np.abs(Lmb) > 1.0e-6
    with np.errstate(all="ignore"):
        e_lapse = (-G0 / np.where(lapse, Lmb, 1.0) / R) * (ul * (1.0 + ul * (-0.5 + ul / 3.0)))
    e_iso = -((G0 / R) / TMB[k]) * dh
    ee = np.where(lapse, e_lapse, e_iso)
    uP = ee * (1.0 + ee * (0.5 + (0.0 if mutant == "uP_e3" else ee / 6.0)))
    P1 = c["P"] + c["P"] * uP
    rho1 = c["rho"] + c["rho"] * ((uP - uT) * (1.0 + uT * (uT - 1.0)))
    inv_a1 = c["inv_a"] + c["inv_a"] * (uT * (-0.5 + uT * (0.375 - 0.3125 * uT)))
    wn1, we1 = c["wn"] + c["s0"] * dh, c["we"] + c["s1"] * dh
    ok = (c["inv_p"] > 0.0) & (np.abs(u) < U_LIMIT) & (np.abs(v) < U_LIMIT) & (np.maximum(np.abs(dalt), np.abs(dh)) < c["margin"])
    cen = np.column_stack([c[key] for key in NAMES])
    per = np.column_stack([rho1, P1, inv_a1, wn1, we1, shp1, chp1, inv_p1])
    return cen, per, ok, c["margin"]


# ---------------------------------------------------------------------------------------------------------------------------
# the truth
# ---------------------------------------------------------------------------------------------------------------------------
def _point(X, mpf, x, y, z, wind_mp):
    """-> (the eight quantities, (layer, wind piece, below 86 km), geopotential altitude, altitude, cos(lat)) as mpf"""
    from mpmath import cos, sin, sqrt
    lat, _, alt = X.geodetic(x, y, z)
    low = alt < 86000
    h = X.R0 * alt / (X.R0 + alt) if low else alt
    T, P, rho, a = X.atmosphere(h)
    xp = wind_mp[0]
    wn, we = X.interp(h, xp, wind_mp[1]), X.interp(h, xp, wind_mp[2])
    k = max(i for i in range(11) if i == 0 or h >= X.HB[i])
    piece = -1 if h <= xp[0] else (-2 if h > xp[-1] else max(i for i in range(len(xp) - 1) if xp[i] < h))
    vals = [rho, P, 1 / a, wn, we, sin(lat / 2), cos(lat / 2), 1 / sqrt(x * x + y * y)]
    return vals, (k, piece, bool(low)), h, alt, cos(lat)


def truth(r, kk, dlt, wind):
    """-> dict: `centre` [n, 8], `delta` [n, 8] (X(r') - X(r), rounded once), `same` [n] (r' in the centre's layer, wind piece and
    geopotential branch), `u`, `v` [n] (pos_delta's u = dlt (2 x_k + dlt) / p^2 -- 0 along z -- and v = cos(lat') / cos(lat) - 1),
    `clear` [n]: the distance of the centre from the nearest break (layers and wind rows in geopotential altitude, 86 km in
    altitude) in units of |dlt|, `lat` [n] (rad)"""
    from mpmath import acos, mpf
    from oracle import exact_fd as X
    r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
    wind = np.asarray(wind, dtype=np.float64)
    wind_mp = [[X.f64(v) for v in wind[:, col]] for col in range(3)]
    breaks = [X.HB[i] for i in range(1, 11) if i != 7] + wind_mp[0]
    n = len(r)
    out = {"centre": np.zeros((n, 8)), "delta": np.zeros((n, 8)), "same": np.zeros(n, dtype=bool), "u": np.zeros(n), "v": np.zeros(n),
           "clear": np.zeros(n), "lat": np.zeros(n)}
    for i in range(n):
        c = [X.f64(v) for v in r[i]]
        q = list(c)
        k, d = int(kk[i]), X.f64(dlt[i])
        q[k] = c[k] + d
        vc, gc, hc, ac, clc = _point(X, mpf, *c, wind_mp)
        vp, gp, hp, ap, clp = _point(X, mpf, *q, wind_mp)
        out["centre"][i] = [float(v) for v in vc]
        out["delta"][i] = [float(b - a) for a, b in zip(vc, vp)]
        out["same"][i] = gc == gp
        out["u"][i] = 0.0 if k == 2 else float(d * (2 * c[k] + d) / (c[0] * c[0] + c[1] * c[1]))
        out["v"][i] = float(clp / clc - 1)
        dist = min([abs(hc - b) for b in breaks] + [abs(ac - 86000)] + ([abs(hc - mpf(GEOPOT86))] if gc[0] == 6 else []))
        out["clear"][i] = float(dist / abs(d))
        out["lat"][i] = float(acos(clc)) * (1.0 if r[i, 2] >= 0 else -1.0)
    return out


def rel_at(T):
    """[n, 8]: the relative accuracy of every change at every point (see REL above)"""
    rel = np.full(T["delta"].shape, REL)
    rel[:, 3:5] += np.minimum(WIND_CAP, WIND_POLAR * EPS / np.cos(T["lat"]) ** 2)[:, None]
    rel[:, 7] += INVP_U2 * T["u"] ** 2
    return rel


def tolerance(T, rel=None):
    """[n, 8]: rel |dX_true| + 4 eps |X_centre|; rel: rel_at(T), or one number for all (what a claim without exceptions would be)"""
    return (rel_at(T) if rel is None else rel) * np.abs(T["delta"]) + 4.0 * EPS * np.abs(T["centre"])


def ratios(cen, per, T, rel=None):
    """[n, 8]: |(per - cen) - dX_true| over the tolerance"""
    return np.abs((per - cen) - T["delta"]) / (tolerance(T, rel) + 1e-300)


# ---------------------------------------------------------------------------------------------------------------------------
# the inputs
# ---------------------------------------------------------------------------------------------------------------------------
STEPS = (1e-6, 1e-3, 0.064, 0.25, 1.0)


def _ecef(lat, lon, alt):
    N = RA / np.sqrt(1.0 - E2 * np.sin(lat) ** 2)
    return np.column_stack([(N + alt) * np.cos(lat) * np.cos(lon), (N + alt) * np.cos(lat) * np.sin(lon), (N * (1.0 - E2) + alt) * np.sin(lat)])


def _geometric(h):
    h = np.asarray(h, dtype=np.float64)
    return np.where(h < 84851.0, R0 * h / (R0 - h), h)


def inputs(wind):
    """-> dict: r [n, 3] (m), kk [n], dlt [n], group [n] (0 the grid, 1 around the breaks, 2 around pos_delta's |u| limit)
      grid    11 latitudes -89.9 .. 89.9 deg x 14 altitudes -300 m .. 700 km through every layer x the three components x
              dlt = +-STEPS (the sign alternates), longitudes spread;
      breaks  0.5 and 2 steps below and above every layer break, 86 km and every wind row, at 40 deg N, 30 deg E (a positive step
              of any component climbs, a negative one descends), |dlt| = 1e-3, 0.064, 1 m, both signs, the three components;
      limit   x or y sweeps near the polar axis with u = dlt (2 x + dlt) / p^2 at 0.4 .. 2 times 1e-4, |dlt| = 0.064 and 1 m."""
    wind = np.asarray(wind, dtype=np.float64)
    rng = np.random.default_rng(15)
    R, K, D, Gp = [], [], [], []
    lats = np.deg2rad([-89.9, -85.0, -72.0, -45.0, -10.0, 0.5, 30.0, 60.0, 78.0, 88.0, 89.9])
    alts = [-300.0, 0.0, 5.0e3, 12.0e3, 25.0e3, 40.0e3, 49.0e3, 60.0e3, 80.0e3, 88.0e3, 100.0e3, 115.0e3, 150.0e3, 700.0e3]
    for la in lats:
        for al in alts:
            for kk in range(3):
                for d in STEPS:
                    sg = 1.0 if len(R) % 2 == 0 else -1.0
                    R.append(_ecef(np.array([la]), rng.uniform(-np.pi, np.pi, 1), np.array([al]))[0])
                    K.append(kk); D.append(sg * d); Gp.append(0)
    hb = [float(v) for v in HB[1:] if v != 86000.0] + [float(v) for v in wind[:, 0] if -1.0e3 <= v <= 1.0e6]   # not the table's far end rows
    la, lo = np.array([np.deg2rad(40.0)]), np.array([np.deg2rad(30.0)])
    for d in (1e-3, 0.064, 1.0):
        alt_list = [float(_geometric(hk + off * d)) for hk in hb for off in (-2.0, -0.5, 0.5, 2.0)]
        alt_list += [86000.0 + off * d for off in (-2.0, -0.5, 0.5, 2.0)]
        for al in alt_list:
            for kk in range(3):
                for sg in (1.0, -1.0):
                    R.append(_ecef(la, lo, np.array([al]))[0]); K.append(kk); D.append(sg * d); Gp.append(1)
    b_e = RB
    for d in (0.064, 1.0):
        for f in (0.4, 0.9, 0.99, 1.01, 1.1, 2.0):
            p = 2.0 * d / (U_LIMIT * f)
            for kk in (0, 1):
                for sg in (1.0, -1.0):
                    for al, south in ((1000.0, False), (20000.0, True)):
                        xy = (p, 0.0) if kk == 0 else (0.0, p)
                        R.append(np.array([xy[0], xy[1], (-1.0 if south else 1.0) * (b_e + al)])); K.append(kk); D.append(sg * d); Gp.append(2)
    return {"r": np.array(R), "kk": np.array(K, dtype=np.int64), "dlt": np.array(D), "group": np.array(Gp)}

"""One flight whose every phase STARTS on another branch of the flight's right-hand side: what
tests/golden/make_flight_kinks.py, tests/test_flight_kinks_cpu.py and tests/test_flight_kinks.py share.

section_rhs_tangent and section_rhs_adjoint (gel_section_rhs_tan.h, gel_section_rhs_adj.h) select by `s2 > 0`, `inv_p > 0`,
`tail.piece >= 0`, ph.air / engine_on / hold, and through gel_exact.h's helpers by the atmosphere layer, the 86 km switch, gravity's
r < b clamp and the CA table's clamps.  The flights of g30 - g33 are smooth: none of them takes the other side of any of these.
Here the first state row of every phase -- stage 1 of the phase's first step in section mode, and of every first interval in node
mode -- sits in one class (PHASES), exactly where the class is an equality (x = y = 0; v = omega x r in fp64 arithmetic).

  kink_problem(variant)      (prob, X [3, nvars], disp [3, S, 4]); vector TRUTH_VEC is the kink vector, vector 0 the same with
                             every position scaled by 1 + 2^-10 and the at-rest velocity doubled (off every exact kink), vector 2 with
                             the axis phases moved 5 km off the axis
  kink_census(prob, phases, Z, fw)   the class flags of every stage, in fp64 from the stage states (the rounded 60-digit ones)
  directions / functionals   the 16 seeds and 9 functionals

The example's tables are kept as they ship.  Two things follow that the case cannot change: the wind table spans -1e8 .. 1e10 m of
geopotential altitude with calm, flat end intervals, and the CA table's end intervals are flat -- leaving either table changes no
slope that was not zero already; and the polar axis (altitude -N, geopotential altitude +9.5e8 m) lies in the wind table's calm last
interval, so the longitude the axis convention picks multiplies a zero wind.  The branches are taken all the same (a lookup that
mis-indexed there would not return zero), but a derivative that ignored them would not differ.  Those three restatements are
therefore held on the ENDS variant of the case (kink_problem("ends"); see ENDS below), whose tables are windy and sloped at
their ends and whose southern axis stage flies in air that carries a force."""
import os

import numpy as np

import flight_adjoint_truth as at
import flight_tangent_truth as tt

HERE = os.path.dirname(os.path.abspath(__file__))
G34 = os.path.join(HERE, "golden", "g34_flight_kinks.npz")
TRUTH_VEC = tt.TRUTH_VEC
N_NODES = 3
FLIGHTS = (("kinks", "section", 1), ("kinks", "node", 1), ("kinks", "section", 2))
FULL = FLIGHTS[0]            # the flight whose per-stage data the fixture keeps
# The example's tables end in flat, calm intervals, and the axis altitude -N (geopotential +9.5e8 m) lies in air of 2e-20 kg/m^3:
# on them a slope continued outside a table, or another longitude on the axis, changes nothing.  The ENDS variant is the same
# flight over tables that are windy and sloped at their ends (ends_tables), with the southern axis phase moved to z = -1e9 m and
# given 5e16 m^2 of area -- the air is as thin off the axis there as on it, so the flight stays finite and the axis stage's force
# is that of thin air, not nothing -- and with every knot time shifted by 1e4 units, so that the Earth angle on the axis is 0.73
# rad away from the one of t = 0.
ENDS = ("kinks@ENDS", "section", 1)
ENDS_TIME_SHIFT = 1.0e4
ENDS_AXIS_AREA = 5.0e16
ENDS_TEETH = ("wind_slope_outside", "ca_slope_outside", "axis_angle_t0")

RA, RB = 6378137.0, 6378137.0 * (1.0 - 1.0 / 298.257223563)
E2 = (RA * RA - RB * RB) / RA / RA
EP2 = (RA * RA - RB * RB) / RB / RB
OMEGA = 7.2921151467e-5
R0 = 6356766.0
HB = np.array([0.0, 11000.0, 20000.0, 32000.0, 47000.0, 51000.0, 71000.0, 86000.0, 91000.0, 110000.0, 120000.0])
LMB = np.array([-0.0065, 0.0, 0.001, 0.0028, 0.0, -0.0028, -0.002, 0.0, 0.0025, 0.012, 0.012])
TMB = np.array([288.15, 216.65, 216.65, 228.65, 270.65, 270.65, 214.65, 186.8673, 186.8673, 240.0, 360.0])
MB = np.array([28.9644] * 7 + [28.9522, 28.89, 27.27, 26.20])

# (the class of the first row, thrust, massflow, reference_area, nozzle_area, engine_on, attitude_hold); _first_rows places the rows
PHASES = (
    ("axis_north", 420000.0, 140.9, 2.21, 0.68, 1, 0),
    ("axis_south", 0.0, 0.0, 2.21, 0.0, 0, 1),
    ("at_rest", 420000.0, 140.9, 2.21, 0.68, 1, 1),
    ("under_air", 30700.0, 9.8, 1.3, 0.1, 1, 0),
    ("under_noair", 30700.0, 9.8, 0.0, 0.0, 1, 1),
    ("lapse", 0.0, 0.0, -2.21, 0.0, 0, 0),
    ("isothermal", 420000.0, 140.9, 2.21, 0.68, 1, 0),
    ("ellipse", 0.0, 0.0, 2.21, 0.0, 0, 1),
    ("exponential", 30700.0, 9.8, 0.7, 0.1, 1, 0),
    # 330 km from the Earth's centre: geopotential altitude -1e8 m and below, where the lapse law gives 1e15 kg/m^3 -- the area is
    # what keeps the force that of thin air, and a nozzle would be pushed by 1e23 Pa
    ("wind_below", 30700.0, 9.8, 2.0e-16, 0.0, 1, 0),
    ("wind_above", 0.0, 0.0, 2.21, 0.0, 0, 0),
    ("ca_above", 420000.0, 140.9, 2.21, 0.68, 1, 0),
)
NAMES = tuple(p[0] for p in PHASES)
AXIS_PHASES = (NAMES.index("axis_north"), NAMES.index("axis_south"))
REST_PHASE = NAMES.index("at_rest")
DIRECTIONS = tt.DIRECTIONS + ("position_all", "velocity_all", "quaternion_all", "axis_x", "knot_time_axis")
FUNCTIONALS = at.FUNCTIONALS + ("dense_all", "axis_rest_ends")
# the classes of the table: each met by stage 1 of at least one phase
CLASSES = ("axis_north", "axis_south", "at_rest", "under_air", "under_noair", "lapse", "isothermal", "ellipse", "exponential",
           "below_86km", "above_86km", "wind_below", "wind_above", "ca_below", "ca_above", "coast_hold_air", "engine_free_air",
           "area_negative", "area_zero")
# the WRONG restatements of single branches whose dy the fixture stores beside the truth (make_flight_kinks.py), section k = 1:
#   wind_slope_outside      outside the wind table the end interval's slope continued (value and slope)
#   ca_slope_outside        the same for the CA table
#   axis_longitude_partial  on the axis the plain central quotient along x / y: the partials of p and of the longitude not zeroed
#   axis_angle_t0           on the axis the held wind's longitude from the Earth angle of t = 0
#   no_gravity_clamp        below the polar radius the magnitude terms of gravity not clamped
#   neighbour_lapse         stage 1 of the lapse and of the isothermal phase with the next layer's lapse rate
#   rest_from_1e-100        the at-rest stage's partials taken 1e-100 m/s off rest
#   hold_rows_free          the quaternion rows of the hold phases as a free phase has them, under the sampled control
TEETH = ("wind_slope_outside", "ca_slope_outside", "axis_longitude_partial", "axis_angle_t0", "no_gravity_clamp", "neighbour_lapse",
         "rest_from_1e-100", "hold_rows_free")
# what no stage of the smooth flights (g30, g32, g33) meets
GAP = ("on_axis", "at_rest", "underground", "above_110km_air", "above_wind_table")


def _geodetic_to_eci(lat, lon, alt):
    Np = RA / np.sqrt(1.0 - E2 * np.sin(lat) ** 2)
    return np.array([(Np + alt) * np.cos(lat) * np.cos(lon), (Np + alt) * np.cos(lat) * np.sin(lon), (Np * (1.0 - E2) + alt) * np.sin(lat)])


def ends_tables(prob):
    """(wind [9, 3], ca [7, 2]) of the ENDS variant: the example's row counts; the wind table from -1e8 m to 120 km, windy and
    sloped in its first and last interval (the phases at 150 km, at 2e10 m and both axis stages lie above it, the phase 330 km
    from the centre below it); the CA table sloped in its first and last interval"""
    w = np.array(prob["wind_table"], dtype=np.float64).copy()
    c = np.array(prob["ca_table"], dtype=np.float64).copy()
    assert w.shape == (9, 3) and c.shape == (7, 2)
    w[0, 1:], w[1, 1:] = (5.0, -3.0), (8.0, 2.0)
    w[7, 1:] = (4.0, 6.0)
    w[8] = (120000.0, 40.0, -25.0)
    c[0, 1], c[6, 1] = 0.25, 0.5
    return w, c


def _first_rows(prob, variant=None):
    """(r [S, 3] m, v [S, 3] m/s) of the first row of every phase"""
    import states
    up, uv = float(prob["units"][1]), float(prob["units"][2])
    rng = np.random.default_rng(34)
    S = len(PHASES)
    r, rel = np.zeros((S, 3)), np.zeros((S, 3))
    d = rng.standard_normal((S, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    place = {"lapse": (0.6, 1.0, 5000.0, 600.0), "isothermal": (-0.4, -2.0, 17000.0, 250.0), "ellipse": (0.9, 2.5, 100e3, 2000.0),
             "exponential": (-0.2, 0.3, 150e3, 1500.0), "wind_above": (0.3, -1.0, 2.0e10, 0.0), "ca_above": (0.5, 1.7, 60e3, 40e3)}
    for s, name in enumerate(NAMES):
        if name in place:
            lat, lon, alt, speed = place[name]
            r[s] = _geodetic_to_eci(lat, lon, alt)
            rel[s] = d[s] * speed
    # the polar axis: z as exact_jac_truth.corner_state's polar nodes; 20 km/s across it, so that stages 2 - 4 of a step of a
    # half node interval (k = 2: 0.09 s to stage 2) lie beyond the 1276 m switch of pos_delta
    r[AXIS_PHASES[0]] = (0.0, 0.0, 6.36e6)
    r[AXIS_PHASES[1]] = (0.0, 0.0, -6.45e6 if variant is None else -1.0e9)
    rel[AXIS_PHASES[0]] = (20e3 * np.cos(0.7), 20e3 * np.sin(0.7), 200.0)
    rel[AXIS_PHASES[1]] = (-20e3 * np.sin(0.4), 20e3 * np.cos(0.4), -150.0)
    # below the polar radius, as corner_state's underground nodes
    r[NAMES.index("under_air")] = d[3] * 0.999 * RB
    rel[NAMES.index("under_air")] = d[4] * 300.0
    r[NAMES.index("under_noair")] = d[5] * 0.6 * RB
    rel[NAMES.index("under_noair")] = d[6] * 300.0
    r[NAMES.index("wind_below")] = (2.6e5, -1.7e5, 1.0e5)
    rel[NAMES.index("wind_below")] = d[7] * 50.0
    v = rel + np.column_stack([-OMEGA * r[:, 1], OMEGA * r[:, 0], np.zeros(S)])
    v[AXIS_PHASES[0]], v[AXIS_PHASES[1]] = rel[AXIS_PHASES[0]], rel[AXIS_PHASES[1]]
    v[NAMES.index("wind_above")] = d[8] * 1000.0
    xr, xv = r / up, v / uv
    xr[list(AXIS_PHASES), :2] = 0.0
    # at rest in the air: states.rest_state's construction (x, y powers of two metres, v = omega x r exact), its node 5
    _p, xs = states.rest_state()
    Mr = 40
    xr[REST_PHASE] = xs[Mr:4 * Mr].reshape(-1, 3)[5]
    xv[REST_PHASE] = xs[4 * Mr:7 * Mr].reshape(-1, 3)[5]
    return xr, xv


def kink_problem(variant=None):
    """-> (prob, X [3, nvars], disp [3, S, 4]); variant: None, or "ends" (see ENDS)"""
    assert variant in (None, "ends")
    import interp_truth as it
    S, n = len(PHASES), N_NODES
    prob = it.prob_of([n] * S)
    for i, key in enumerate(("thrust", "massflow", "reference_area", "nozzle_area")):
        prob[key] = np.array([p[1 + i] for p in PHASES], dtype=np.float64)
    prob["engine_on"] = np.array([p[5] for p in PHASES], dtype=np.int32)
    prob["attitude_hold"] = np.array([p[6] for p in PHASES], dtype=np.int32)
    up, uv, ut = float(prob["units"][1]), float(prob["units"][2]), float(prob["units"][4])
    N, M = S * n, S * (n + 1)
    rng = np.random.default_rng(340)
    xr0, xv0 = _first_rows(prob, variant)
    pos, vel = np.zeros((M, 3)), np.zeros((M, 3))
    for s in range(S):
        for j in range(n + 1):
            # the later rows (the starts of the later intervals in node mode): a few kilometres and some 100 m/s on, off every kink
            pos[s * (n + 1) + j] = xr0[s] + j * np.array([3100.0, 2300.0, 1700.0]) / up
            vel[s * (n + 1) + j] = xv0[s] + j * np.array([110.0, -70.0, 40.0]) / uv
    quat = rng.standard_normal((M, 4))
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    mass = np.linspace(0.9, 0.4, M) + 0.01 * rng.random(M)
    x = np.concatenate([mass, pos.ravel(), vel.ravel(), quat.ravel(), 0.1 * rng.standard_normal(2 * N), (10.0 + 2.0 * np.arange(S + 1)) / ut])
    if variant == "ends":
        prob["wind_table"], prob["ca_table"] = ends_tables(prob)
        prob["reference_area"][AXIS_PHASES[1]] = ENDS_AXIS_AREA
        x[11 * M + 2 * N:] += ENDS_TIME_SHIFT
    first = np.arange(S) * (n + 1)
    # vector 0: off every exact kink
    x0 = x.copy()
    x0[M:4 * M] = x[M:4 * M] * (1.0 + 2.0 ** -10)
    x0[4 * M + 3 * first[REST_PHASE]:4 * M + 3 * first[REST_PHASE] + 3] *= 2.0
    # vector 2: the axis phases 5 km off the axis
    x2 = x.copy()
    for s in AXIS_PHASES:
        x2[M + 3 * first[s]:M + 3 * first[s] + 2] = np.array([4000.0, -3000.0]) / up
    import flight_truth as ft
    disp = np.stack([ft.teeth_dispersion(S) * (1.0 + 0.01 * b) for b in range(3)])
    disp[:, :, 3] = 2.0 - 0.5 * np.arange(3)[:, None]
    disp[:, REST_PHASE, 3] = 0.0          # calm air for the phase at rest in it (and the calm vote of its wavefront)
    return prob, np.stack([x0, x, x2]), np.ascontiguousarray(disp)


def directions(prob, x):
    """the 16 seeds at the vector x -> (dX [16, nvars], dD [16, S, 4])"""
    nn, S, N, M = tt.layout(prob)
    dX11, dD11 = tt.directions(prob, x)
    P = len(DIRECTIONS)
    dX, dD = np.zeros((P, dX11.shape[1])), np.zeros((P, S, 4))
    dX[:11], dD[:11] = dX11, dD11
    first = [sum(nn[:s]) + s for s in range(S)]
    vecs = {11: (1, (0.6, -0.48, 0.64)), 12: (4, (-0.36, 0.8, 0.48)), 13: (7, (0.1, 0.7, -0.5, 0.5))}
    for d, (c0, vec) in vecs.items():
        for f in first:
            for c, v in enumerate(vec):
                dX[d, tt.sidx(M, f, c0 + c)] = v
    for s in AXIS_PHASES:
        dX[14, tt.sidx(M, first[s], 1)] = 1.0
    dX[15, 11 * M + 2 * N + AXIS_PHASES[0] + 1] = 1.0
    return dX, dD


def functionals(prob, x):
    """the 9 functionals -> lam [9, M, 11]"""
    nn, S, N, M = tt.layout(prob)
    lam = np.zeros((len(FUNCTIONALS), M, 11))
    lam[:7] = at.functionals(prob, x)
    lam[7] = np.random.default_rng(341).standard_normal((M, 11))
    w = np.random.default_rng(342).standard_normal((3, 11))
    for i, s in enumerate(AXIS_PHASES + (REST_PHASE,)):
        lam[8, sum(nn[:s]) + s + nn[s]] = w[i]
    return lam


# ------------------------------------------------------------------ the census
def _geodetic(r):
    """src/Earth.cpp:49-61 in fp64 -> (sin lat, cos lat, alt); on the polar axis the altitude is the reference's -N"""
    p = np.hypot(r[0], r[1])
    th = np.arctan2(r[2] * RA, p * RB)
    lat = np.arctan2(r[2] + EP2 * RB * np.sin(th) ** 3, p - E2 * RA * np.cos(th) ** 3)
    Np = RA / np.sqrt(1.0 - E2 * np.sin(lat) ** 2)
    return np.sin(lat), np.cos(lat), (p / np.cos(lat) if p > 0.0 else 0.0) - Np


def _temperature(h, k):
    if h <= 91000.0 or 110000.0 < h <= 120000.0:
        return TMB[k] + LMB[k] * (h - HB[k])
    if h <= 110000.0:
        return 263.1905 - 76.3232 * np.sqrt(1.0 - ((h - 91000.0) / 19942.9) ** 2)
    xi = (h - HB[k]) * (R0 + HB[k]) / (R0 + h)
    return 1000.0 - (1000.0 - TMB[k]) * np.exp(-0.01875e-3 * xi)


def kink_census(prob, phases, Z, fw):
    """the class flags of every stage: phases [T] (the stage's phase), Z [T, 11] the stage states (normalised, fp64 -- the rounded
    60-digit states, or a fixture's), fw [S] the wind factor of every phase -> dict of arrays [T]: air, on_axis, north, rest
    (|v_air|^2 == 0), under (r < b), alt, h, layer, above86, wind (-1 below the first row, K - 1 above the last, else the interval),
    mach, ca (likewise), margin (the smallest relative distance to a branch boundary that the stage is not exactly on)"""
    um, up, uv = (float(v) for v in prob["units"][:3])
    W, Ct = np.asarray(prob["wind_table"], dtype=float), np.asarray(prob["ca_table"], dtype=float)
    T = len(phases)
    out = {k: np.zeros(T, dtype=bool) for k in ("air", "on_axis", "north", "rest", "under", "above86")}
    out.update({k: np.zeros(T) for k in ("alt", "h", "mach")})
    out.update({k: np.full(T, -2, dtype=int) for k in ("layer", "wind", "ca")})
    out["margin"] = np.full(T, np.inf)

    def rel(a, b):
        return abs(a - b) / max(abs(b), 1.0)

    for i in range(T):
        s = int(phases[i])
        r, v = Z[i, 1:4] * up, Z[i, 4:7] * uv
        rn = float(np.sqrt((r * r).sum()))
        out["under"][i] = rn < RB
        m = rel(rn, RB)
        out["north"][i] = r[2] > 0
        out["air"][i] = air = float(prob["reference_area"][s]) != 0.0
        if not air:
            out["margin"][i] = m
            continue
        p = float(np.hypot(r[0], r[1]))
        out["on_axis"][i] = axis = r[0] == 0.0 and r[1] == 0.0
        if not axis:
            m = min(m, p / rn)
        sl, cl, alt = _geodetic(r)
        h = R0 * alt / (R0 + alt) if alt < 86000.0 else alt
        k = int(np.nonzero(h >= HB)[0].max()) if h >= 0 else 0
        out["alt"][i], out["h"][i], out["layer"][i], out["above86"][i] = alt, h, k, alt >= 86000.0
        m = min(m, rel(alt, 86000.0), min(rel(h, b) for b in HB))
        K = len(W)
        out["wind"][i] = wi = -1 if h <= W[0, 0] else (K - 1 if h > W[-1, 0] else int(np.searchsorted(W[:, 0], h, side="left")) - 1)
        m = min(m, min(rel(h, b) for b in W[:, 0]))
        wn, we = (np.interp(h, W[:, 0], W[:, c]) * fw[s] for c in (1, 2))
        if axis:
            clon, slon = 1.0, 0.0       # (the Earth angle is not the census's business: |wind| of 20 km/s moves no Mach class)
        else:
            clon, slon = r[0] / p, r[1] / p
        w = np.array([-wn * sl * clon - we * slon, -wn * sl * slon + we * clon, wn * cl])
        a = np.array([(v[0] + OMEGA * r[1]) - w[0], (v[1] - OMEGA * r[0]) - w[1], v[2] - w[2]])
        s2 = float((a * a).sum())
        out["rest"][i] = s2 == 0.0
        if s2 > 0.0:
            m = min(m, np.sqrt(s2) / (np.sqrt((v * v).sum()) + OMEGA * rn))
        Tk = _temperature(h, k)
        out["mach"][i] = mach = np.sqrt(s2) / np.sqrt(1.4 * (8314.32 / MB[k]) * Tk)
        Kc = len(Ct)
        out["ca"][i] = -1 if mach <= Ct[0, 0] else (Kc - 1 if mach > Ct[-1, 0] else int(np.searchsorted(Ct[:, 0], mach, side="left")) - 1)
        if s2 > 0.0:
            m = min(m, min(rel(mach, b) for b in Ct[:, 0]))
        out["margin"][i] = m
    return out


def class_flags(prob, phases, c):
    """[T, len(CLASSES)] booleans from a census"""
    eng = np.asarray(prob["engine_on"])[phases].astype(bool)
    hold = np.asarray(prob["attitude_hold"])[phases].astype(bool)
    area = np.asarray(prob["reference_area"], dtype=float)[phases]
    air, off = c["air"], c["air"] & ~c["on_axis"]
    Kw, Kc = len(prob["wind_table"]), len(prob["ca_table"])
    f = {"axis_north": c["on_axis"] & c["north"], "axis_south": c["on_axis"] & ~c["north"], "at_rest": air & c["rest"],
         "under_air": air & c["under"], "under_noair": ~air & c["under"],
         "lapse": off & (c["h"] <= 91000.0) & (LMB[c["layer"]] != 0.0), "isothermal": off & (c["h"] <= 91000.0) & (LMB[c["layer"]] == 0.0),
         "ellipse": off & (c["h"] > 91000.0) & (c["h"] <= 110000.0), "exponential": off & (c["h"] > 120000.0),
         "below_86km": off & ~c["above86"], "above_86km": off & c["above86"],
         "wind_below": air & (c["wind"] == -1), "wind_above": air & (c["wind"] == Kw - 1),
         "ca_below": air & (c["ca"] == -1), "ca_above": air & (c["ca"] == Kc - 1),
         "coast_hold_air": air & ~eng & hold, "engine_free_air": air & eng & ~hold, "area_negative": area < 0.0, "area_zero": area == 0.0}
    return np.column_stack([f[k] for k in CLASSES])


def gap_flags(prob, c):
    """{name: [T]} of GAP -- what the smooth flights never meet -- and, beside them, "below_wind_table", which the flights over
    EDGE32 / LONG do meet (tests/test_flight_kinks_cpu.py asserts both)"""
    air = c["air"]
    return {"on_axis": c["on_axis"], "at_rest": air & c["rest"], "underground": c["under"], "above_110km_air": air & ~c["on_axis"] & (c["h"] > 110000.0), "below_wind_table": air & (c["wind"] == -1),
            "above_wind_table": air & (c["wind"] == len(prob["wind_table"]) - 1)}


def stage_phases(prob, mode, k):
    """[T]: the phase of every stage in the order the flight stores them"""
    nn, S, N, M = tt.layout(prob)
    ks = tt.steps_of(k, S)
    return np.concatenate([np.full(4 * ks[s] * nn[s], s, dtype=int) for s in range(S)])


def first_stage(prob, mode, k):
    """[S]: the index of stage 1 of every phase's first step"""
    nn, S, N, M = tt.layout(prob)
    ks = tt.steps_of(k, S)
    return np.cumsum([0] + [4 * ks[s] * nn[s] for s in range(S)])[:-1]


def axis_rows(prob):
    """[M] booleans: the state rows of the two axis phases"""
    nn, S, N, M = tt.layout(prob)
    return np.concatenate([np.full(nn[s] + 1, s in AXIS_PHASES) for s in range(S)])


def load(flight):
    g = np.load(G34)
    key = "%s_%s_k%d_" % flight
    return {name[len(key):]: g[name] for name in g.files if name.startswith(key)}


def fly_stages(E, plan, prob, x, disp, mode):
    """the fp64 value flight of flight_truth (its right-hand side, its carry) with every stage state kept -> (phases [T], Z [T, 11]);
    mode: "chain", "section" or "node\""""
    import flight_truth as ft
    import mesh_truth as mt
    from propagate_truth import samples
    ut = float(prob["units"][4])
    phases, Z = [], []
    y_end, X_prev = None, None
    for s in range(E.S):
        X, Uc, to, tf = mt.phase_state(E, x, s)
        n = X.shape[0] - 1
        m, k = plan.matrices(s), plan.steps[s]
        ph = ft._Phase(prob, s, None if disp is None else np.array(disp[s], dtype=float))
        pts = m["pts"]
        Us = np.zeros((len(pts), 2)) if bool(prob["attitude_hold"][s]) else samples(m, Uc)[0]
        tx = np.concatenate([[-1.0], E.tau(s)])
        hs = (tx[1:] - tx[:-1]) / k
        y = X[0].copy() if (s == 0 or mode != "chain") else ft.carry(y_end, np.zeros(11), X_prev[-1], X[0])[0]
        for j in range(n):
            if mode == "node":
                y = X[j].copy()
            Sh = (tf - to) * ut / 2.0 * hs[j]
            for i in range(k):
                p = 2 * (k * j + i)
                k1 = ph.F(y, Us[p], pts[p], to, tf)[0]
                y2 = y + Sh * 0.5 * k1
                k2 = ph.F(y2, Us[p + 1], pts[p + 1], to, tf)[0]
                y3 = y + Sh * 0.5 * k2
                k3 = ph.F(y3, Us[p + 1], pts[p + 1], to, tf)[0]
                y4 = y + Sh * k3
                k4 = ph.F(y4, Us[p + 2], pts[p + 2], to, tf)[0]
                Z += [y, y2, y3, y4]
                phases += [s] * 4
                y = y + Sh / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)
        y_end, X_prev = y, X
    return np.array(phases), np.array(Z)


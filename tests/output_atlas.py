"""The output table's atlas: one synthetic problem and one decision vector whose state nodes are placed by hand, one node or
more for every branch of the post-processing table (output_result.py:37-263; output_kernel in gel_kernels_rows.hip), each carrying tags.
Plain numpy, no GPU.  tests/golden/make_output_atlas.py turns it into tests/golden/g26_output_atlas.npz (the inputs, the reference's
own table, a 50-digit truth with its sensitivity scale and the margin of every branch predicate); the tests read that fixture and
rebuild nothing but the handles.

Problem: four phases of 5 / 20 / 40 / 60 collocation nodes (M = 129 state nodes: three workgroups of 64 lanes, one lane in the
last), pairwise different (thrust, reference_area, nozzle_area) including reference_area = 0 and nozzle_area = 0, units unlike
the example's, a wind table of 40 rows and a CA table of 30 rows on non-uniform knots.  Two further handles: M = 64 (one phase,
n = 63) and M = 3 (n = 2), their nodes taken from the big one.

States left out on purpose:
  * the exact pole: the reference's altitude p / cos(lat) - N divides 0 by 0 there;
  * e < 1e-3: the perigee direction is 0 / 0, argp and ta are noise in any arithmetic;
  * points within 10 degrees of the launch site's antipode: Vincenty's iteration need not contract there;
  * gimbal lock itself: the predicate's argument 2 (w y - z x) is a sine, so no state has a margin above the threshold 1, and
    the state that has it equal to 1 in exact arithmetic (identity quaternion over latitude 0, longitude 0) evaluates to
    0.9999999999999998 in fp64 (quat_ecef2nedg divides by fl(sqrt 2) > sqrt 2): the reference does NOT take the branch there,
    the exact arithmetic does, and heading / roll are atan2(0, 0) on one side only.  The atlas carries the approach instead
    (pitch 89.99 degrees, both signs of the heading), where the predicate is decided;
  * a geopotential altitude exactly on a layer boundary below 86 km: the altitude is a rounded function of the position, so
    the comparison is undecidable; the atlas has nodes 1 cm either side of each (margin > 1e6), and nodes exactly on the four
    boundaries above 86 km, where the geometric altitude itself is compared and x - Ra is exact on the equator at t = 0;
  * the impact point's "not converged" exit: five steps on an ellipsoid of flattening 1 / 298 always converge below 1 m.
"""
import math

import numpy as np

from oracle import output_table as ot
from oracle import waypoint as wp

OMEGA, MU, RA = wp.OMEGA, wp.MU, wp.A_E
UNITS = {"mass": 23456.789, "position": 4194304.0, "velocity": 7654.321, "u": 0.5, "t": 431.0}
LAUNCH_LAT, LAUNCH_LON = 28.5, 0.0
NODES = [5, 20, 40, 60]
PARAMS = [(1.2e6, 3.1, 0.9), (4.5e5, 0.0, 0.35), (7.7e4, 1.7, 0.0), (0.0, 0.4, 0.05)]     # thrust, reference_area, nozzle_area
NAMES = ["LIFTOFF", "MECO", "SEP", "COAST", "END"]
STAGES = ["1", "1", "2", "2", "2"]
M_BIG = sum(NODES) + len(NODES)
SMALL = {"m64": [63], "m3": [2]}
# geopotential / geometric base altitudes of the atmosphere's layers (lib/USStandardAtmosphere.py:71-83)
LAYER_BASE = [0.0, 11000.0, 20000.0, 32000.0, 47000.0, 51000.0, 71000.0, 86000.0, 91000.0, 110000.0, 120000.0]

REQUIRED_TAGS = """equatorial inclined_ascending inclined_descending fz_negative asc_negative argp_atan2_negative hyperbolic
near_circular iip_below_surface iip_not_elliptical iip_positive_perigee iip_no_intersection iip_converging_ascending
iip_converging_descending iip_southern iip_lon_west_of_minus_180 lat_plus_89_9 lat_minus_89_9 lon_plus_180 lon_minus_180
alt_minus_100 alt_above_table downrange_same_longitude downrange_1e-9deg downrange_1m downrange_90deg downrange_170deg
near_gimbal heading_negative quat_norm_3 quat_norm_1e-3 aoa_aligned air_at_rest backwards windy_layer ca_below_first
ca_on_knot ca_above_last wind_below_first wind_on_knot wind_above_last knot_last knot_first time_negative time_zero
time_beyond_sidereal_day""".split() + ["layer_%d" % k for k in range(11)] + ["boundary_%d" % int(b) for b in LAYER_BASE[7:]] + \
    ["below_boundary_%d" % int(b) for b in LAYER_BASE[1:7]] + ["above_boundary_%d" % int(b) for b in LAYER_BASE[1:7]]


# ---------------------------------------------------------------- building blocks (fp64)
def ned_axes(lat, lon):
    """north, east, down unit vectors [ECEF] at a geodetic latitude / longitude [deg]"""
    p, l = math.radians(lat), math.radians(lon)
    return (np.array([-math.sin(p) * math.cos(l), -math.sin(p) * math.sin(l), math.cos(p)]),
            np.array([-math.sin(l), math.cos(l), 0.0]),
            np.array([-math.cos(p) * math.cos(l), -math.cos(p) * math.sin(l), -math.sin(p)]))


def quat_euler(az, el, ro):
    """NED -> body quaternion of heading / pitch / roll [deg] (Z-Y-X), the inverse of euler_from_quat"""
    cz, sz = math.cos(math.radians(az) / 2), math.sin(math.radians(az) / 2)
    cy, sy = math.cos(math.radians(el) / 2), math.sin(math.radians(el) / 2)
    cx, sx = math.cos(math.radians(ro) / 2), math.sin(math.radians(ro) / 2)
    return np.array([cz * cy * cx + sz * sy * sx, cz * cy * sx - sz * sy * cx, cz * sy * cx + sz * cy * sx,
                     sz * cy * cx - cz * sy * sx])


def quat_x_to(d, roll=0.0):
    """ECI -> body quaternion whose thrust direction quatrot(conj(q), e_x) is d, rolled about it"""
    d = np.asarray(d, dtype=np.float64) / np.linalg.norm(d)
    ax = np.cross([1.0, 0.0, 0.0], d)
    q = np.array([1.0 + d[0], ax[0], ax[1], ax[2]])
    q /= np.linalg.norm(q)
    r = np.array([math.cos(roll / 2), math.sin(roll / 2), 0.0, 0.0])
    return ot.quatmult(q, r)


def state(lat, lon, alt, t, v_ned=(0.0, 0.0, 0.0), att=(90.0, 45.0, 0.0), mass=1.0e4, qscale=1.0):
    """a node from its geodetic position [deg, deg, m] at time t [s], ground velocity in NED [m/s] and heading / pitch / roll"""
    pe = wp.geodetic2ecef(lat, lon, alt)
    pos = ot.ecef2eci(pe, t)
    n, e, d = ned_axes(lat, lon)
    ve = v_ned[0] * n + v_ned[1] * e + v_ned[2] * d
    vel = ot.ecef2eci(ve, t) + np.cross([0.0, 0.0, OMEGA], pos)
    quat = ot.quatmult(ot.quat_eci2nedg(pos, t), quat_euler(*att)) * qscale
    return [float(mass), pos, vel, quat, float(t)]


def orbit_state(r, v, t=100.0, att_dir=None, mass=5.0e3):
    r, v = np.asarray(r, dtype=np.float64), np.asarray(v, dtype=np.float64)
    return [float(mass), r, v, quat_x_to(v if att_dir is None else att_dir, 0.3), float(t)]


def kepler_state(a, e, inc, asc, argp, ta):
    """r, v [ECI] of classical elements (angles in degrees)"""
    inc, asc, argp, ta = (math.radians(x) for x in (inc, asc, argp, ta))
    p = a * (1.0 - e * e)
    r = p / (1.0 + e * math.cos(ta))
    rp = np.array([r * math.cos(ta), r * math.sin(ta), 0.0])
    vp = math.sqrt(MU / p) * np.array([-math.sin(ta), e + math.cos(ta), 0.0])

    def rot(v):
        c, s = math.cos(argp), math.sin(argp)
        v = np.array([c * v[0] - s * v[1], s * v[0] + c * v[1], v[2]])
        c, s = math.cos(inc), math.sin(inc)
        v = np.array([v[0], c * v[1] - s * v[2], s * v[1] + c * v[2]])
        c, s = math.cos(asc), math.sin(asc)
        return np.array([c * v[0] - s * v[1], s * v[0] + c * v[1], v[2]])
    return rot(rp), rot(vp)


# ---------------------------------------------------------------- the atlas
def _special_nodes():
    """[(tags, node, exact predicates)]: node = [mass, pos, vel, quat, t] in SI; tags are checked by validate()"""
    out = []

    def add(tags, node, exact=()):
        out.append((tags.split(), node, list(exact)))

    # ---- orbital elements
    r, v = kepler_state(7.0e6, 0.05, 0.0, 0.0, 200.0, 60.0)
    r[2], v[2] = 0.0, 0.0
    add("equatorial argp_atan2_negative inclined_no", orbit_state(r, v), ["inc", "asc_neg"])
    add("equatorial", orbit_state(*[w * np.array([1.0, 1.0, 0.0]) for w in kepler_state(7.1e6, 0.02, 0.0, 0.0, 40.0, 250.0)]), ["inc", "asc_neg"])
    add("inclined_ascending asc_negative", orbit_state(*kepler_state(7.0e6, 0.03, 51.6, 250.0, 30.0, 70.0), t=-20.0))
    add("inclined_descending fz_negative", orbit_state(*kepler_state(7.2e6, 0.04, 97.5, 40.0, 300.0, 200.0)))
    add("inclined_descending", orbit_state(*kepler_state(6.9e6, 0.01, 28.5, 120.0, 80.0, 300.0)))
    add("fz_negative inclined_ascending asc_negative", orbit_state(*kepler_state(7.5e6, 0.1, 63.4, 300.0, 270.0, 20.0)))
    add("hyperbolic", orbit_state(*kepler_state(-2.0e7, 1.4, 30.0, 10.0, 50.0, 40.0)))
    add("hyperbolic inclined_descending", orbit_state(*kepler_state(-3.0e7, 1.25, 140.0, 200.0, 250.0, 320.0)))
    add("near_circular", orbit_state(*kepler_state(6.8e6, 1.0e-3, 45.0, 80.0, 120.0, 100.0)))
    add("near_circular inclined_descending", orbit_state(*kepler_state(6.78e6, 1.0e-3, 98.0, 200.0, 300.0, 260.0)))
    # ---- impact point
    add("iip_below_surface lat_plus_89_9 alt_minus_100", state(89.9, 40.0, -100.0, 50.0, (30.0, 10.0, -5.0)))
    add("iip_below_surface lat_minus_89_9", state(-89.9, -130.0, -100.0, 70.0, (-20.0, 40.0, 3.0)))
    add("iip_not_elliptical", orbit_state(*kepler_state(-1.0e7, 1.8, 20.0, 15.0, 40.0, 10.0)))
    add("iip_positive_perigee", orbit_state(*kepler_state(6.8e6, 0.005, 35.0, 20.0, 10.0, 45.0)))
    add("iip_no_intersection", orbit_state(*kepler_state((6.62e6 + 6.37e6) / 2, (6.62e6 - 6.37e6) / (6.62e6 + 6.37e6), 5.0, 30.0, 50.0, 150.0)))
    add("iip_converging_ascending", state(31.0, 132.0, 80000.0, 200.0, (1500.0, 2500.0, -900.0), (60.0, 20.0, 5.0)))
    add("iip_converging_descending", state(33.0, 140.0, 120500.0, 420.0, (1400.0, 2600.0, 700.0), (62.0, -15.0, -5.0)))
    add("iip_southern", state(-10.0, -60.0, 90500.0, 300.0, (-3000.0, 1000.0, -1500.0), (160.0, 25.0, 0.0)))
    add("iip_lon_west_of_minus_180", state(5.0, -174.0, 150000.0, 30.0, (100.0, -1200.0, -3000.0), (270.0, 60.0, 0.0)))
    # ---- position
    add("lat_plus_89_9", state(89.9, -75.0, 30000.0, 90.0, (100.0, 200.0, -50.0)))
    add("lat_minus_89_9", state(-89.9, 15.0, 12000.0, 95.0, (300.0, -100.0, -20.0)))
    add("lon_plus_180", state(12.0, 180.0 - 5e-7, 25000.0, 0.0, (10.0, 600.0, -100.0)))
    add("lon_minus_180", state(-12.0, -180.0 + 5e-7, 40000.0, 0.0, (10.0, -600.0, -100.0)))
    add("alt_minus_100", state(20.0, 30.0, -100.0, 5.0, (5.0, 3.0, 0.5), (45.0, 10.0, 0.0)))
    mid = [5000.0, 15000.0, 25000.0, 40000.0, 49000.0, 60000.0, 81500.0, 88000.0, 100000.0, 115000.0, 150000.0]
    for k, z in enumerate(mid):
        add("layer_%d" % k + (" alt_above_table" if k == 10 else ""),
            state(10.0 + 3 * k, 20.0 + 11 * k, z, 60.0 + 10 * k, (200.0 + 90 * k, 300.0 + 150 * k, -100.0 - 20 * k), (50.0 + k, 30.0 - k, 2.0 * k)))
    for b in LAYER_BASE[7:]:             # the geometric altitude itself is compared: x - Ra is exact on the equator at t = 0
        n = state(0.0, 0.0, b, 0.0, (50.0, 900.0, -300.0), (80.0, 40.0, 0.0))
        n[1] = np.array([RA + b, 0.0, 0.0])
        add("boundary_%d downrange_same_longitude time_zero" % int(b), n, ["layer", "z86", "samelon", "asc_neg"])   # asc_neg: c_x = 0 exactly, asc = atan2(0, .)
    for b in LAYER_BASE[1:7]:            # geopotential h = r0 z / (r0 + z): 1 cm either side
        for side, dz in (("below", -0.01), ("above", 0.01)):
            z = 6356766.0 * (b + dz) / (6356766.0 - (b + dz))
            add("%s_boundary_%d" % (side, int(b)), state(-25.0, 70.0, z, 130.0, (250.0, 400.0, -150.0), (100.0, 35.0, 1.0)))
    # ---- downrange (launch point 28.5 N, 0 E)
    n = state(-40.0, 0.0, 20500.0, 0.0, (100.0, 50.0, -10.0))
    n[1][1] = 0.0
    add("downrange_same_longitude time_zero", n, ["samelon"])
    add("downrange_1e-9deg", state(38.5, 1e-9, 18000.0, 0.0, (100.0, 50.0, -10.0)))
    add("downrange_1m", state(28.5, 1.02e-5, 300.0, 0.0, (1.0, 2.0, -3.0), (90.0, 85.0, 0.0)))
    add("downrange_90deg", state(10.0, 90.0, 70000.0, 700.0, (100.0, 2000.0, -100.0)))
    add("downrange_170deg", state(-20.0, 170.0, 65000.0, 2000.0, (-100.0, 2000.0, 100.0)))
    # ---- attitude
    add("near_gimbal", state(15.0, 25.0, 35000.0, 110.0, (300.0, 500.0, -400.0), (30.0, 89.99, 0.0)))
    add("near_gimbal heading_negative", state(0.0, 3.0, 1000.0, 0.0, (1.0, 2.0, -30.0), (-60.0, 89.99, 10.0)))
    add("heading_negative", state(-35.0, 100.0, 45000.0, 150.0, (-700.0, -900.0, -200.0), (-130.0, 20.0, -15.0)))
    add("quat_norm_3", state(42.0, -20.0, 55000.0, 170.0, (900.0, 1200.0, -500.0), (55.0, 33.0, 4.0), qscale=3.0))
    add("quat_norm_1e-3", state(-42.0, 20.0, 58000.0, 175.0, (900.0, -1200.0, -500.0), (125.0, 31.0, -4.0), qscale=1e-3))
    # ---- angle of attack
    out.append(None)                     # aoa_aligned: needs the wind table, see build()
    # vel = omega x r plus 0.1 mm/s upwards: still below the 1 mm/s of the test, and r . v (the true anomaly's branch) is decided
    add("air_at_rest ca_below_first", state(35.0, 50.0, 3000.0, 20.0, (0.0, 0.0, -1.0e-4), (10.0, 80.0, 0.0)))
    add("backwards", state(25.0, -100.0, 30500.0, 250.0, (400.0, 300.0, 100.0), (216.87 + 0.0, -10.0, 0.0)))
    add("windy_layer", state(30.0, 131.0, 9000.0, 45.0, (150.0, 250.0, -200.0), (59.0, 50.0, 0.0)))
    # ---- tables
    add("wind_below_first", state(31.0, 131.0, 120.0, 3.0, (0.5, 1.0, -20.0), (90.0, 88.0, 0.0)))
    add("wind_on_knot", state(31.5, 131.5, 7300.0, 40.0, (100.0, 200.0, -250.0), (70.0, 60.0, 0.0)))
    add("ca_on_knot", state(32.0, 132.0, 21000.0, 75.0, (300.0, 600.0, -400.0), (65.0, 40.0, 0.0)))
    add("ca_above_last", state(32.5, 133.0, 50500.0, 140.0, (1200.0, 2600.0, -600.0), (66.0, 15.0, 0.0)))
    # ---- time
    add("time_negative", state(5.0, 5.0, 16000.0, -37.5, (120.0, 80.0, -60.0)))
    add("time_beyond_sidereal_day", state(-5.0, 95.0, 420000.0, 90000.0, (1000.0, 7000.0, 10.0), (80.0, 0.0, 0.0)))
    return out


def wind_table():
    """40 rows [altitude m, north m/s, east m/s] on non-uniform knots; calm below 4 km; one knot is moved onto the geopotential
    altitude of the wind_on_knot node by build()"""
    k = np.arange(40)
    alt = 400.0 + 180.0 * k + 22.0 * k ** 2 + 37.0 * np.sin(1.7 * k)
    north = np.where(alt < 4000.0, 0.0, 18.0 * np.sin(alt / 5100.0) + 0.4 * k)
    east = np.where(alt < 4000.0, 0.0, 31.0 * np.cos(alt / 7300.0) - 0.7 * k)
    return np.column_stack([alt, north, east])


def ca_table():
    """30 rows [Mach, CA] on non-uniform knots from Mach 0.2 to 8, the last interval with a slope (a lookup that extrapolates
    past it instead of clamping differs); one knot is moved onto the Mach number of the ca_on_knot node by build()"""
    k = np.arange(30)
    mach = 0.2 + 0.11 * k + 0.0055 * k ** 2 + 0.03 * np.sin(2.3 * k)
    mach[-1] = 8.0
    ca = 0.25 + 0.35 * np.exp(-((mach - 1.1) / 0.4) ** 2) + 0.02 * mach
    return np.column_stack([mach, ca])


_CACHE = {}


def build():
    """-> dict: nodes [(tags, [mass, pos, vel, quat, t], exact)] of the M = 129 handle in node order, wind, ca, x, tx, tu"""
    if _CACHE:
        return _CACHE
    import oracle as _c
    wind, ca = wind_table(), ca_table()
    spec = _special_nodes()
    # a wind knot on the geopotential altitude of the wind_on_knot node (the lookup is continuous there)
    for e in spec:
        if e is not None and "wind_on_knot" in e[0]:
            h = _c.geopotential_altitude(wp.eci2geodetic(e[1][1], e[1][4])[2])
            j = int(np.argmin(np.abs(wind[:, 0] - h)))
            assert 0 < j < len(wind) - 1
            wind[j, 0] = h
    assert np.all(np.diff(wind[:, 0]) > 0)
    # thrust direction along the air velocity: the quaternion that turns e_x onto the air velocity the oracle forms
    n = state(27.0, 128.0, 14000.0, 65.0, (350.0, 500.0, -450.0))
    va = ot._air_velocity_eci(n[1], n[2], n[4], wind)
    n[3] = quat_x_to(va, 0.0)
    spec[spec.index(None)] = ("aoa_aligned".split(), n, [])
    for e in spec:
        if "ca_on_knot" in e[0]:
            mach = ot.node_row(*_si(e[1]), PARAMS[0], wind, ca, LAUNCH_LAT, LAUNCH_LON)["M"]
            j = int(np.argmin(np.abs(ca[:, 0] - mach)))
            assert 0 < j < len(ca) - 1
            ca[j, 0] = mach
    assert np.all(np.diff(ca[:, 0]) > 0)
    # generic states fill the rest: seeded, suborbital, every latitude band
    rng = np.random.default_rng(26)
    fill = M_BIG - len(spec) - (len(NODES) - 1)
    assert fill >= 0, fill
    for _ in range(fill):
        lat, lon = rng.uniform(-80.0, 80.0), rng.uniform(-179.0, 179.0)
        while abs(lon - 180.0) < 12.0 + 0 * lat or abs(lon + 180.0) < 12.0:       # away from the antipode (-28.5, 180)
            lon = rng.uniform(-179.0, 179.0)
        alt = float(rng.choice([rng.uniform(200.0, 85000.0), rng.uniform(87000.0, 400000.0)], p=[0.7, 0.3]))
        sp = rng.uniform(100.0, 5000.0)
        az, fpa = rng.uniform(0.0, 360.0), rng.uniform(-40.0, 70.0)
        vn = (sp * math.cos(math.radians(fpa)) * math.cos(math.radians(az)), sp * math.cos(math.radians(fpa)) * math.sin(math.radians(az)),
              -sp * math.sin(math.radians(fpa)))
        att = (az + rng.uniform(-8.0, 8.0), fpa + rng.uniform(-8.0, 8.0), rng.uniform(-30.0, 30.0))
        spec.append((["generic"], state(lat, lon, alt, rng.uniform(0.0, 900.0), vn, att, mass=rng.uniform(500.0, 3.0e5),
                                        qscale=rng.uniform(0.9, 1.1)), []))
    # order: the three knots carry one state on both sides (only the section parameters tell the two rows apart)
    first = np.cumsum([0] + [n + 1 for n in NODES])[1:-1]              # first node of phases 1 .. S - 1
    order = list(rng.permutation(len(spec)))
    nodes = []
    for i in range(M_BIG):
        if i in first:
            tags, nd, ex = nodes[-1]
            nodes[-1] = (tags + ["knot_last"], nd, ex)
            nodes.append(([t for t in tags if t != "knot_last"] + ["knot_first"], [nd[0], nd[1].copy(), nd[2].copy(), nd[3].copy(), nd[4]], ex))
        else:
            tags, nd, ex = spec[order.pop()]
            nodes.append((list(tags), nd, list(ex)))
    assert not order and len(nodes) == M_BIG
    # snap every state to what the kernel forms from x: fl(x unit)
    x = pack([nd for _, nd, _ in nodes], NODES, rng)
    tx = np.array([nd[4] for _, nd, _ in nodes])
    for i, (tags, nd, ex) in enumerate(nodes):
        nd[0], nd[1], nd[2], nd[3] = node_si(x, M_BIG, i)
        if nd[4] < 0.0:
            tags.append("time_negative")
        if nd[4] == 0.0 and "time_zero" not in tags:
            tags.append("time_zero")
    N = sum(NODES)
    tu = np.sort(rng.uniform(tx.min(), tx.max(), N))                   # times of the controls (the host's body-rate columns)
    _CACHE.update(nodes=nodes, wind=wind, ca=ca, x=x, tx=tx, tu=tu)
    return _CACHE


def _si(nd):
    return nd[0], nd[1], nd[2], nd[3], nd[4]


def pack(states, nodes, rng):
    """packed decision vector [mass M | position 3M | velocity 3M | quaternion 4M | u 2N | t S+1] of SI states"""
    M, N, S = len(states), sum(nodes), len(nodes)
    x = np.empty(11 * M + 2 * N + S + 1)
    x[:M] = [s[0] / UNITS["mass"] for s in states]
    x[M:4 * M] = np.concatenate([s[1] / UNITS["position"] for s in states])
    x[4 * M:7 * M] = np.concatenate([s[2] / UNITS["velocity"] for s in states])
    x[7 * M:11 * M] = np.concatenate([s[3] for s in states])
    x[11 * M:11 * M + 2 * N] = rng.uniform(-1.0, 1.0, 2 * N)
    x[11 * M + 2 * N:] = np.sort(rng.uniform(0.0, 2.0, S + 1))
    return x


def node_si(x, M, i):
    """what the kernel forms from x for node i: fl(x unit)"""
    return (float(x[i] * UNITS["mass"]), x[M + 3 * i:M + 3 * i + 3] * UNITS["position"],
            x[4 * M + 3 * i:4 * M + 3 * i + 3] * UNITS["velocity"], x[7 * M + 4 * i:7 * M + 4 * i + 4].copy())


def small(name):
    """(x, tx, tu, source node of every node) of the M = 64 / M = 3 handle: nodes of the big handle, every third / the first three
    special ones; one phase, so PARAMS[0] applies to all"""
    A = build()
    n = SMALL[name][0]
    src = np.arange(0, 3 * (n + 1), 3) % M_BIG if name == "m64" else np.array([7, 40, 90])
    rng = np.random.default_rng(2600 + n)
    states = [[A["nodes"][j][1][0], A["nodes"][j][1][1], A["nodes"][j][1][2], A["nodes"][j][1][3], A["nodes"][j][1][4]] for j in src]
    x = pack(states, [n], rng)
    # the same bits as the big handle's x (x = SI / unit was formed from these very quotients)
    M = n + 1
    for k, j in enumerate(src):
        x[k] = A["x"][j]
        x[M + 3 * k:M + 3 * k + 3] = A["x"][M_BIG + 3 * j:M_BIG + 3 * j + 3]
        x[4 * M + 3 * k:4 * M + 3 * k + 3] = A["x"][4 * M_BIG + 3 * j:4 * M_BIG + 3 * j + 3]
        x[7 * M + 4 * k:7 * M + 4 * k + 4] = A["x"][7 * M_BIG + 4 * j:7 * M_BIG + 4 * j + 4]
    return x, A["tx"][src].copy(), np.sort(rng.uniform(0.0, 900.0, n)), src


def edge():
    """(x, tx, tu) of a third M = 3 handle OUTSIDE the atlas: the identity quaternion over latitude 0, longitude 0 at t = 0, the state
    whose pitch is 90 degrees in exact arithmetic (module docstring: gimbal lock).  Every operation up to the predicate is exact but
    the division by fl(sqrt 2), so the reference, the oracle and the kernel all see 2 (w y - z x) = 0.9999999999999998, take the
    ordinary branch and return pitch asin(.) = 89.9999988 with heading = roll = atan2(0, +) = 0.  No truth for it (exact arithmetic
    takes the other branch): compared with the reference's record and the oracle under the example test's tolerances."""
    rng = np.random.default_rng(2603)
    states = []
    for vel in ((1.0, 2.0, -30.0), (0.0, 465.0, 0.0), (-200.0, 900.0, 50.0)):
        n = state(0.0, 0.0, 1000.0, 0.0, vel)
        n[1] = np.array([RA + 1000.0, 0.0, 0.0])
        n[3] = np.array([1.0, 0.0, 0.0, 0.0])
        states.append(n)
    return pack(states, SMALL["m3"], rng), np.zeros(3), np.array([0.0, 1.0])


def prob_arrays(nodes, wind, ca, params=PARAMS):
    """what gelato_amd.Engine takes"""
    S = len(nodes)
    return {"num_nodes": np.array(nodes, dtype=np.int32), "thrust": np.array([p[0] for p in params[:S]]),
            "massflow": np.array([p[0] / 3000.0 for p in params[:S]]), "reference_area": np.array([p[1] for p in params[:S]]),
            "nozzle_area": np.array([p[2] for p in params[:S]]), "engine_on": np.array([1 if p[0] > 0 else 0 for p in params[:S]], dtype=np.int32),
            "attitude_hold": np.zeros(S, dtype=np.int32),
            "units": np.array([UNITS[k] for k in ("mass", "position", "velocity", "u", "t")]), "dx": 1.0e-8,
            "wind_table": np.asarray(wind, dtype=np.float64), "ca_table": np.asarray(ca, dtype=np.float64)}


def pdict_of(nodes, wind, ca, ps_params, device=None):
    """the pdict the reference's output_result and gelato_amd.output_result read"""
    S = len(nodes)
    params = [{"name": NAMES[s], "rocketStage": STAGES[s], "thrust": PARAMS[min(s, S - 1)][0], "massflow": PARAMS[min(s, S - 1)][0] / 3000.0,
               "reference_area": PARAMS[min(s, S - 1)][1], "nozzle_area": PARAMS[min(s, S - 1)][2],
               "engineOn": PARAMS[min(s, S - 1)][0] > 0, "attitude": "free"} for s in range(S + 1)]
    pd = {"params": params, "ps_params": ps_params, "wind_table": np.array(wind), "ca_table": np.array(ca), "N": sum(nodes),
          "M": sum(nodes) + S, "num_sections": S, "dx": 1.0e-8, "LaunchCondition": {"lat": LAUNCH_LAT, "lon": LAUNCH_LON}}
    if device is not None:
        pd["device"] = device
    return pd


def xdict_of(x, M, N, S):
    o = np.cumsum([0, M, 3 * M, 3 * M, 4 * M, 2 * N, S + 1])
    return {k: x[o[i]:o[i + 1]].copy() for i, k in enumerate(["mass", "position", "velocity", "quaternion", "u", "t"])}


def oracle_table(x, tx, nodes, wind, ca, table=None):
    """oracle.output_table.table on an atlas handle -> [M, 34] in the order of DEVICE_COLUMNS"""
    M, N = sum(nodes) + len(nodes), sum(nodes)
    T = (table or ot.table)(x, M, N, nodes, (UNITS["mass"], UNITS["position"], UNITS["velocity"]), tx, PARAMS[:len(nodes)], wind, ca,
                            LAUNCH_LAT, LAUNCH_LON)
    return np.column_stack([T[c] for c in ot.DEVICE_COLUMNS])


def validate(A=None):
    """every tag's defining property, checked on the fp64 oracle (the generator calls this before it writes)"""
    A = A or build()
    wind, ca = A["wind"], A["ca"]
    have = set()
    sec = ot.node_sections(NODES)
    b = RA * (1.0 - wp.F_E)
    for i, (tags, nd, ex) in enumerate(A["nodes"]):
        mass, pos, vel, quat, t = nd
        row = ot.node_row(mass, pos, vel, quat, t, PARAMS[sec[i]], wind, ca, LAUNCH_LAT, LAUNCH_LON)
        c = np.cross(pos, vel)
        f = np.cross(vel, c) - MU * pos / np.linalg.norm(pos)
        e = np.linalg.norm(f) / MU
        inc = math.acos(c[2] / np.linalg.norm(c))
        rv = float(np.dot(pos, vel))
        llh = wp.eci2geodetic(pos, t)
        import oracle as _c
        h = _c.geopotential_altitude(llh[2])
        pe, ve = wp.eci2ecef(pos, t), wp.vel_eci2ecef(vel, pos, t)
        iip_none = np.isnan(row["lat_IIP"])
        r0, vi = np.linalg.norm(pe), ve + np.cross([0.0, 0.0, OMEGA], pe)
        eps_cos = r0 * np.dot(vi, vi) / MU - 1.0
        qn = quat / np.linalg.norm(quat)
        qb = ot.quatmult(ot.conj(ot.quat_eci2nedg(pos, t)), qn)
        az_raw = math.atan2(2.0 * (qb[0] * qb[3] + qb[1] * qb[2]), 1.0 - 2.0 * (qb[2] ** 2 + qb[3] ** 2))
        va = ot._air_velocity_eci(pos, vel, t, wind)
        vb = ot.quatrot(qn, va)
        w = _c.wind_ned(h, wind)
        asc_raw = math.atan2(c[0], -c[1])
        check = {
            "equatorial": lambda: pos[2] == 0.0 and vel[2] == 0.0 and inc == 0.0,
            "inclined_ascending": lambda: inc > 1e-3 and rv > 0.0,
            "inclined_descending": lambda: inc > 1e-3 and rv < 0.0,
            "fz_negative": lambda: inc > 1e-3 and f[2] < 0.0,
            "asc_negative": lambda: inc > 1e-3 and asc_raw < 0.0,
            "argp_atan2_negative": lambda: inc == 0.0 and math.atan2(f[1], f[0]) < 0.0,
            "hyperbolic": lambda: e > 1.0 and row["altitude_apogee"] < -RA,
            "near_circular": lambda: 0.9e-3 < e < 1.2e-3,
            "iip_below_surface": lambda: r0 < b and iip_none,
            "iip_not_elliptical": lambda: r0 >= b and eps_cos >= 1.0 and iip_none,
            "iip_positive_perigee": lambda: r0 >= b and eps_cos < 1.0 and row["altitude_perigee"] > 0.0 and iip_none,
            "iip_no_intersection": lambda: r0 >= b and eps_cos < 1.0 and -(RA - b) < row["altitude_perigee"] < 0.0 and iip_none,
            "iip_converging_ascending": lambda: not iip_none and rv > 0.0,
            "iip_converging_descending": lambda: not iip_none and rv < 0.0,
            "iip_southern": lambda: not iip_none and row["lat_IIP"] < 0.0,
            "iip_lon_west_of_minus_180": lambda: not iip_none and row["lon_IIP"] < -180.0,
            "lat_plus_89_9": lambda: abs(llh[0] - 89.9) < 1e-6,
            "lat_minus_89_9": lambda: abs(llh[0] + 89.9) < 1e-6,
            "lon_plus_180": lambda: 0.0 < 180.0 - llh[1] < 1e-6,
            "lon_minus_180": lambda: 0.0 < 180.0 + llh[1] < 1e-6,
            "alt_minus_100": lambda: abs(llh[2] + 100.0) < 1e-3,
            "alt_above_table": lambda: llh[2] > 120000.0,
            "downrange_same_longitude": lambda: llh[1] == LAUNCH_LON and row["downrange"] == 0.0,
            "downrange_1e-9deg": lambda: 0.5e-9 < abs(llh[1] - LAUNCH_LON) < 2e-9 and row["downrange"] > 1e5,
            "downrange_1m": lambda: 0.5 < row["downrange"] < 2.0,
            "downrange_90deg": lambda: abs(llh[1] - 90.0) < 1e-6,
            "downrange_170deg": lambda: abs(llh[1] - 170.0) < 1e-6,
            "near_gimbal": lambda: 89.98 < row["pitch_NED2BODY"] < 89.999,
            "heading_negative": lambda: az_raw < -1e-3,
            "quat_norm_3": lambda: abs(np.linalg.norm(quat) - 3.0) < 1e-9,
            "quat_norm_1e-3": lambda: abs(np.linalg.norm(quat) - 1e-3) < 1e-12,
            "aoa_aligned": lambda: row["AOA_total"] < 1e-5 and np.linalg.norm(va) > 100.0,
            "air_at_rest": lambda: np.linalg.norm(va) < 2e-4 and row["AOA_total"] == 0.0 and row["M"] < 1e-6 and w[0] == 0.0 and w[1] == 0.0,
            "backwards": lambda: vb[0] < -1.0 and row["AOA_pitch"] == 0.0 and row["AOA_yaw"] == 0.0,
            "windy_layer": lambda: math.hypot(w[0], w[1]) > 5.0,
            "ca_below_first": lambda: row["M"] < ca[0, 0],
            "ca_on_knot": lambda: row["M"] in ca[1:-1, 0],
            "ca_above_last": lambda: row["M"] > ca[-1, 0] and row["aero_BODY_X"] != 0.0 and llh[2] < 86000.0,
            "wind_below_first": lambda: h < wind[0, 0],
            "wind_on_knot": lambda: h in wind[1:-1, 0],
            "wind_above_last": lambda: h > wind[-1, 0],
            "knot_last": lambda: i + 1 < M_BIG and sec[i + 1] == sec[i] + 1 and all(np.array_equal(u, v) for u, v in zip(nd[1:4], A["nodes"][i + 1][1][1:4])) and nd[0] == A["nodes"][i + 1][1][0] and t == A["nodes"][i + 1][1][4],
            "knot_first": lambda: i > 0 and sec[i - 1] == sec[i] - 1,
            "time_negative": lambda: t < 0.0,
            "time_zero": lambda: t == 0.0,
            "time_beyond_sidereal_day": lambda: t > 86164.1,
        }
        for k in range(11):
            check["layer_%d" % k] = (lambda k=k: LAYER_BASE[k] < h and (k == 10 or h < LAYER_BASE[k + 1]))
        for bb in LAYER_BASE[7:]:
            check["boundary_%d" % int(bb)] = (lambda bb=bb: llh[2] == bb and h == bb)
        for bb in LAYER_BASE[1:7]:
            check["below_boundary_%d" % int(bb)] = (lambda bb=bb: 0.005 < bb - h < 0.015)
            check["above_boundary_%d" % int(bb)] = (lambda bb=bb: 0.005 < h - bb < 0.015)
        if h > wind[-1, 0] and "wind_above_last" not in tags:
            tags.append("wind_above_last")
        for tg in tags:
            if tg in ("generic", "inclined_no"):
                continue
            assert check[tg](), (i, tg, {k: row[k] for k in ("lat", "lon", "altitude", "M", "pitch_NED2BODY", "downrange", "lat_IIP", "lon_IIP", "altitude_perigee")}, e, h)
            have.add(tg)
        # excluded on purpose: within 10 degrees of the launch point's antipode, e < 1e-3, the pole
        assert abs(llh[0]) < 89.95 and e > 0.9e-3, (i, tags)
        assert not (abs(llh[0] + LAUNCH_LAT) < 10.0 and abs(abs(llh[1] - LAUNCH_LON) - 180.0) < 10.0), (i, tags)
    missing = [t for t in REQUIRED_TAGS if t not in have]
    assert not missing, missing
    return have


# ---------------------------------------------------------------- the fixture and the bound (what the tests share)
FIXTURE = "g26_output_atlas.npz"
U64 = 2.0 ** -53
HANDLES = {"big": NODES, "m64": SMALL["m64"], "m3": SMALL["m3"]}


def bound(g, handle):
    """[M, 34]: 4 max(K_col, 1) u s, the downrange column plus the stopping-rule term of the reference's Vincenty loop.  K_col is
    the oracle's (the reference's algorithm in fp64 against the 50-digit truth), never the device's; the 4 covers the device math
    library's 1-2 ulp functions against glibc's, the kernel's operation order and its guard-free division / square root."""
    b = 4.0 * np.maximum(g["K_col"], 1.0)[None, :] * U64 * g["s_" + handle]
    b[:, ot.DEVICE_COLUMNS.index("downrange")] += float(g["downrange_term"])
    return b


def usage(table, g, handle):
    """share of the bound used: per column the largest |table - T| / bound over the nodes (0 / 0 = 0); NaN patterns must agree"""
    T, b = g["T_" + handle], bound(g, handle)
    assert np.array_equal(np.isnan(table), np.isnan(T)), handle
    d = np.abs(table - T)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0.0, 0.0, d / b)
    return np.where(np.isnan(T), 0.0, r)


def usage_report(r, title):
    worst = r.argmax(axis=0)
    lines = ["%s: share of the bound used per column (node of the largest)" % title]
    lines += ["  %-38s %9.3g  (node %d)" % (c, r[worst[k], k], worst[k]) for k, c in enumerate(ot.DEVICE_COLUMNS)]
    return "\n".join(lines)

"""Synthetic extreme states shared by the parity tests and by tests/golden/make_exact_fd.py (which pins them with
exact-arithmetic finite-difference values).  Every builder returns (prob, x): the static problem as the engine / oracle take
it and a packed decision vector.  Deterministic (seeded)."""
from fractions import Fraction

import numpy as np


def _example_prob():
    from gelato_amd import con_dynamics, problem
    pdict, unitdict, condition, xdict = problem.make_problem("example")
    return dict(con_dynamics.problem_arrays(pdict, unitdict))


def ragged_state():
    """n = 2 phases, engine-off + free attitude, NoAir + hold, zero thrust with aero, a multi-chunk phase (n = 100 > 64) with a
    ragged tail; positions anywhere on the sphere (all latitudes, the poles' neighbourhood included) at 0 .. 127 km, speeds of
    several km/s in whatever air there is: dynamic pressures far beyond any flight."""
    prob = _example_prob()
    rng = np.random.default_rng(7)
    S = 7
    prob["num_nodes"] = np.array([2, 3, 100, 2, 17, 64, 5], dtype=np.int32)
    prob["thrust"] = np.array([420000.0, 0.0, 420000.0, 30700.0, 0.0, 30700.0, 1000.0])
    prob["massflow"] = np.array([140.0, 0.0, 140.0, 9.8, 0.0, 9.8, 0.3])
    prob["reference_area"] = np.array([2.21, 2.21, 2.21, 0.0, 0.0, 2.21, 0.0])
    prob["nozzle_area"] = np.array([0.68, 0.0, 0.68, 0.0, 0.0, 0.1, 0.0])
    prob["engine_on"] = np.array([1, 0, 1, 1, 0, 1, 1], dtype=np.int32)
    prob["attitude_hold"] = np.array([1, 0, 0, 1, 1, 0, 0], dtype=np.int32)
    N = int(prob["num_nodes"].sum())
    M = N + S
    # physically sensible random state: radius 1.0..1.02 Earth radii, speeds up to 7 km/s
    pos = rng.standard_normal((M, 3))
    pos = pos / np.linalg.norm(pos, axis=1, keepdims=True) * (1.0 + 0.02 * rng.random((M, 1)))
    vel = rng.standard_normal((M, 3)) * 3.0
    quat = rng.standard_normal((M, 4))
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    x = np.concatenate([0.2 + rng.random(M), pos.ravel(), vel.ravel(), quat.ravel(), rng.standard_normal(2 * N),
                        np.sort(rng.random(S + 1))])
    return prob, x


def long_state(nn):
    """phases of 68 nodes and more (slab-staged D.X), every second one aerodynamic, |lat| <= 57 deg, 0 .. 150 km, up to ~12 km/s"""
    prob = _example_prob()
    rng = np.random.default_rng(sum(nn))
    S = len(nn)
    prob["num_nodes"] = np.array(nn, dtype=np.int32)
    prob["engine_on"] = np.ones(S, dtype=np.int32)
    prob["thrust"] = rng.uniform(1e4, 5e5, S)
    prob["massflow"] = rng.uniform(1.0, 150.0, S)
    prob["reference_area"] = np.where(np.arange(S) % 2 == 0, 2.0, 0.0)
    prob["nozzle_area"] = rng.uniform(0.0, 1.0, S)
    prob["attitude_hold"] = np.zeros(S, dtype=np.int32)
    N = int(sum(nn))
    M = N + S
    up = prob["units"][1]
    lat = rng.uniform(-1.0, 1.0, M)
    lon = rng.uniform(-np.pi, np.pi, M)
    R = (6378137.0 - 21385.0 * np.sin(lat) ** 2 + rng.uniform(0.0, 150e3, M)) / up
    pos = np.column_stack([R * np.cos(lat) * np.cos(lon), R * np.cos(lat) * np.sin(lon), R * np.sin(lat)])
    vel = rng.standard_normal((M, 3)) * rng.uniform(0.05, 4.0, (M, 1))
    quat = rng.standard_normal((M, 4))
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    x = np.concatenate([0.2 + rng.random(M), pos.ravel(), vel.ravel(), quat.ravel(), rng.standard_normal(2 * N),
                        np.sort(rng.random(S + 1))])
    return prob, x


def all_layers_state(lat_lo=-0.95, lat_hi=1.45):
    """One aerodynamic phase whose 64 nodes climb from 300 m below the ellipsoid to 700 km: every US-1976 layer (lapse,
    isothermal, the 91-110 km ellipse, the exponential above 120 km), the geopotential switch at 86 km, wind / CA clamps on both
    sides, southern and northern latitudes (geocentric lat_lo .. lat_hi rad along the climb), Mach 0.03 ... 30, long flight times."""
    prob = _example_prob()
    rng = np.random.default_rng(23)
    n = 64
    prob["num_nodes"] = np.array([n], dtype=np.int32)
    for k, v in [("thrust", 420000.0), ("massflow", 140.9), ("reference_area", 2.21), ("nozzle_area", 0.68)]:
        prob[k] = np.array([v])
    prob["engine_on"] = np.array([1], dtype=np.int32)
    prob["attitude_hold"] = np.array([0], dtype=np.int32)
    up, uv, ut = prob["units"][1], prob["units"][2], prob["units"][4]
    alt = np.concatenate([[-300.0, -50.0, 0.0, 10.0], np.linspace(2e3, 130e3, 53), [150e3, 200e3, 300e3, 400e3, 500e3, 600e3, 700e3, 700e3]])
    assert len(alt) == n + 1
    lat = np.linspace(lat_lo, lat_hi, n + 1)
    lon = np.linspace(-3.0, 3.0, n + 1)
    a_e, b_e = 6378137.0, 6356752.314245
    R = (a_e * b_e / np.sqrt((b_e * np.cos(lat)) ** 2 + (a_e * np.sin(lat)) ** 2) + alt) / up   # ellipsoid radius + altitude
    pos = np.column_stack([R * np.cos(lat) * np.cos(lon), R * np.cos(lat) * np.sin(lon), R * np.sin(lat)])
    speed = np.geomspace(10.0, 9000.0, n + 1) / uv
    d = rng.standard_normal((n + 1, 3))
    vel = d / np.linalg.norm(d, axis=1, keepdims=True) * speed[:, None]
    quat = rng.standard_normal((n + 1, 4))
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    x = np.concatenate([np.linspace(1.0, 0.3, n + 1), pos.ravel(), vel.ravel(), quat.ravel(),
                        2.0 * rng.standard_normal(2 * n), [100.0 / ut, 9000.0 / ut]])
    return prob, x


def polar_dense_state():
    """What rounds 1-2 kept out of the parity claim: dense air at high latitude.  One aerodynamic phase of 48 nodes at
    geodetic-ish latitudes 55 .. 89.9 deg, both hemispheres, sea level .. 30 km, 300 .. 2500 m/s (max-q conditions and
    beyond), nozzle area 0.68 (the sea-level pressure-thrust term)."""
    prob = _example_prob()
    rng = np.random.default_rng(91)
    n = 48
    prob["num_nodes"] = np.array([n], dtype=np.int32)
    for k, v in [("thrust", 420000.0), ("massflow", 140.9), ("reference_area", 2.21), ("nozzle_area", 0.68)]:
        prob[k] = np.array([v])
    prob["engine_on"] = np.array([1], dtype=np.int32)
    prob["attitude_hold"] = np.array([0], dtype=np.int32)
    up, uv, ut = prob["units"][1], prob["units"][2], prob["units"][4]
    lat = np.deg2rad(np.concatenate([np.linspace(55.0, 89.9, 25), -np.linspace(56.0, 89.5, 24)]))
    alt = np.concatenate([np.linspace(0.0, 30e3, 25), np.linspace(29e3, 100.0, 24)])
    lon = rng.uniform(-np.pi, np.pi, n + 1)
    a_e, b_e = 6378137.0, 6356752.314245
    R = (a_e * b_e / np.sqrt((b_e * np.cos(lat)) ** 2 + (a_e * np.sin(lat)) ** 2) + alt) / up
    pos = np.column_stack([R * np.cos(lat) * np.cos(lon), R * np.cos(lat) * np.sin(lon), R * np.sin(lat)])
    speed = rng.uniform(300.0, 2500.0, n + 1) / uv
    d = rng.standard_normal((n + 1, 3))
    vel = d / np.linalg.norm(d, axis=1, keepdims=True) * speed[:, None]
    quat = rng.standard_normal((n + 1, 4))
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    x = np.concatenate([np.linspace(1.0, 0.5, n + 1), pos.ravel(), vel.ravel(), quat.ravel(),
                        2.0 * rng.standard_normal(2 * n), [10.0 / ut, 160.0 / ut]])
    return prob, x


def with_coast_tail(build, n_tail=2):
    """(prob, x) of `build` with one short engine-off phase without aerodynamics appended: the aero path constraints never apply to
    the LAST phase (lib/con_aero.py:108 walks range(num_sections - 1)), so a one-phase state needs a successor to be constrained."""
    prob, x = build()
    prob = dict(prob)
    nn = [int(v) for v in prob["num_nodes"]]
    S, N = len(nn), sum(nn)
    M = N + S
    for key, v in [("num_nodes", n_tail), ("thrust", 0.0), ("massflow", 0.0), ("reference_area", 0.0), ("nozzle_area", 0.0),
                   ("engine_on", 0), ("attitude_hold", 0)]:
        prob[key] = np.concatenate([prob[key], np.array([v], dtype=np.asarray(prob[key]).dtype)])
    o = np.cumsum([0, M, 3 * M, 3 * M, 4 * M, 2 * N, S + 1])
    mass, pos, vel, quat, u, t = (x[o[i]:o[i + 1]] for i in range(6))
    rep = n_tail + 1
    return prob, np.concatenate([mass, np.repeat(mass[-1:], rep), pos, np.tile(pos[-3:], rep), vel, np.tile(vel[-3:], rep),
                                 quat, np.tile(quat[-4:], rep), u, np.zeros(2 * n_tail), t, [t[-1] + 0.01]])


BREAK_STEP_OFFSETS = ((-0.06, 0.6, -1.2, 2.5), (0.06, -0.6, 1.2, -2.5))


def layer_break_state(n_max=None, step=None):
    """One aerodynamic phase whose nodes sit within a few centimetres of the breaks of the atmosphere layers (geopotential 11, 20, 32, 47,
    51, 71 km), of the geopotential branch (86 km geometric) and of the wind table's pieces (1, 3, 11, 15, 16, 23 km): the position
    step of a sweep (dx * unit = 6.4 cm) carries some of them across -- what the exact-difference forms hand back to the recomputing
    sweeps.  Mid latitudes, 400 .. 3000 m/s.

    step (m; None: the vector above, bit for bit): the nodes scale with the position step of the problem the vector is made for.
    The breaks gain 91, 110 and 120 km (where the ellipse and the exponential of the temperature begin and end); every break has
    two nodes below and two above it, at 0.06, 0.6, 1.2 and 2.5 steps in geopotential altitude (geometric at the 86 km branch and
    above) -- the signs alternate from break to break (BREAK_STEP_OFFSETS), which keeps the 15 breaks within one 64-node phase.
    A negative step gives the mirrored vector (every offset on the other side of its break): the two together put a node at each
    of the eight offsets +-0.06 .. +-2.5 steps of every break."""
    prob = _example_prob()
    rng = np.random.default_rng(5)
    r0 = 6356766.0
    breaks_h = [11000.0, 20000.0, 32000.0, 47000.0, 51000.0, 71000.0, 1000.0, 3000.0, 15000.0, 16000.0, 23000.0]
    if step is None:
        alt = [r0 * h / (r0 - h) + off for h in breaks_h for off in (-0.04, -0.004, 0.004, 0.04)] + [86000.0 + off for off in (-0.04, -0.004, 0.004, 0.04)]
    else:
        alt = [r0 * (h + off * step) / (r0 - (h + off * step)) for i, h in enumerate(breaks_h) for off in BREAK_STEP_OFFSETS[i % 2]]
        alt += [z + off * step for i, z in enumerate([86000.0, 91000.0, 110000.0, 120000.0]) for off in BREAK_STEP_OFFSETS[(i + 1) % 2]]
    alt = np.array(alt + [5000.0])
    if n_max is not None:            # a phase that fits two-vectors-per-wavefront launches: the first n_max + 1 of them
        alt = alt[:n_max + 1]
    n = len(alt) - 1
    prob["num_nodes"] = np.array([n], dtype=np.int32)
    for k, v in [("thrust", 420000.0), ("massflow", 140.9), ("reference_area", 2.21), ("nozzle_area", 0.68)]:
        prob[k] = np.array([v])
    prob["engine_on"] = np.array([1], dtype=np.int32)
    prob["attitude_hold"] = np.array([0], dtype=np.int32)
    up, uv, ut = prob["units"][1], prob["units"][2], prob["units"][4]
    lat = rng.uniform(-1.0, 1.0, n + 1)
    lon = rng.uniform(-np.pi, np.pi, n + 1)
    a_e, b_e = 6378137.0, 6356752.314245
    # geodetic latitude `lat`, altitude `alt` exactly (to rounding): x = (N + alt) cos lat cos lon, z = (N (1 - e^2) + alt) sin lat
    e2 = 1.0 - (b_e / a_e) ** 2
    Np = a_e / np.sqrt(1.0 - e2 * np.sin(lat) ** 2)
    pos = np.column_stack([(Np + alt) * np.cos(lat) * np.cos(lon), (Np + alt) * np.cos(lat) * np.sin(lon), (Np * (1.0 - e2) + alt) * np.sin(lat)]) / up
    speed = rng.uniform(400.0, 3000.0, n + 1) / uv
    d = rng.standard_normal((n + 1, 3))
    vel = d / np.linalg.norm(d, axis=1, keepdims=True) * speed[:, None]
    quat = rng.standard_normal((n + 1, 4))
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    x = np.concatenate([np.linspace(1.0, 0.5, n + 1), pos.ravel(), vel.ravel(), quat.ravel(),
                        2.0 * rng.standard_normal(2 * n), [10.0 / ut, 160.0 / ut]])
    return prob, x


def noair_polar_state():
    """Two phases without aerodynamics (reference_area 0), engine off (thrust 0, free attitude) then on (hold), 16 nodes each: nodes
    ON the polar axis (x = y = 0 exactly, both poles), within millimetres .. metres of it, and elsewhere, at altitudes from 20 km
    below the ellipsoid (below the polar radius: gravity's radius clamp) to 20,000 km.  The NoAir RHS (src/pybind_dynamics.cpp:73-92)
    is thrust + J2 gravity: no geodetic conversion, no polar convention, so its quotients must hold there like anywhere."""
    prob = _example_prob()
    rng = np.random.default_rng(4242)
    n = 16
    S = 2
    prob["num_nodes"] = np.array([n, n], dtype=np.int32)
    prob["thrust"] = np.array([0.0, 30700.0])
    prob["massflow"] = np.array([0.0, 9.8])
    prob["reference_area"] = np.zeros(S)
    prob["nozzle_area"] = np.zeros(S)
    prob["engine_on"] = np.array([0, 1], dtype=np.int32)
    prob["attitude_hold"] = np.array([0, 1], dtype=np.int32)
    up, ut = prob["units"][1], prob["units"][4]
    M = 2 * n + S
    alt = np.tile([1e5, -20e3, -300.0, 0.0, 50.0, 100e3, 400e3, 1e6, 2e6, 5e6, 1e7, 2e7, -5e3, 30e3, 3e5, 3e6, 8e6], 2)
    # colatitude from the +z axis, after node 0 of the phase (no sweep perturbs it): exactly 0 / pi (on the axis), 1e-12 .. 1e-6 rad
    # (micrometres .. metres off it), then anywhere
    colat = np.tile(np.concatenate([[0.7, 0.0, np.pi, 1e-12, 1e-9, np.pi - 1e-7, 1e-6], rng.uniform(0.0, np.pi, 10)]), 2)
    lon = rng.uniform(-np.pi, np.pi, M)
    a_e, b_e = 6378137.0, 6356752.314245
    lat = np.pi / 2 - colat
    R = (a_e * b_e / np.sqrt((b_e * np.cos(lat)) ** 2 + (a_e * np.sin(lat)) ** 2) + alt) / up
    s = np.where((colat == 0.0) | (colat == np.pi), 0.0, np.sin(colat))
    pos = np.column_stack([R * s * np.cos(lon), R * s * np.sin(lon), R * np.cos(colat)])
    vel = rng.standard_normal((M, 3)) * 3.0
    quat = rng.standard_normal((M, 4))
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    x = np.concatenate([0.2 + rng.random(M), pos.ravel(), vel.ravel(), quat.ravel(), 2.0 * rng.standard_normal(2 * 2 * n),
                        [10.0 / ut, 200.0 / ut, 900.0 / ut]])
    return prob, x


# ---------------------------------------------------------------------------------------------------------------------------
# Degenerate states of the aerodynamic forms (tests/golden/make_degenerate_fd.py, tests/test_degenerate_fd.py): the polar axis,
# where the exact-difference position sweeps (gel_rhs_parts.h pos_delta) hand over to the recomputing ones, and rest in the air.
# ---------------------------------------------------------------------------------------------------------------------------
POS_DELTA_U = 1.0e-4     # pos_delta's predicate: |u| < 1e-4 and |v| < 1e-4, u = dlt (2 x_k + dlt) / p^2, v ~ u / 2
AXIS_NODES = (40, 40, 36)


def pos_step(prob, xr):
    """xr [.., 3] normalised -> (r [.., 3] in metres, dlt [.., 3]): the fp64 position the chain starts from and the exact step
    fl((x + dx) unit) - fl(x unit) of each component's sweep"""
    up, dx = float(prob["units"][1]), float(prob["dx"])
    r = xr * up
    return r, (xr + dx) * up - r


def pos_delta_u(prob, xr):
    """-> u [.., 2] of the x and the y sweep as pos_delta forms it (the z sweep leaves p alone: u = 0), p [..]"""
    r, dlt = pos_step(prob, xr)
    p2 = r[..., 0] ** 2 + r[..., 1] ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        u = dlt[..., :2] * (2.0 * r[..., :2] + dlt[..., :2]) / p2[..., None]
    return u, np.sqrt(p2)


def _polar_phase(prob, p, lon, alt, south):
    """normalised positions [len(p), 3] at distance p (m) from the polar axis, longitude lon, altitude alt above the pole (the
    ellipsoid falls 10 m below its polar radius at p = 11 km), south: which pole"""
    b_e = 6356752.314245
    up = prob["units"][1]
    z = np.where(south, -1.0, 1.0) * (b_e + alt)
    return np.column_stack([p * np.cos(lon), p * np.sin(lon), z]) / up


def axis_state():
    """Three aerodynamic phases in dense air (50 m .. 30 km, 300 .. 2500 m/s, the example's wind table) around BOTH poles, by
    how pos_delta's predicate |u| < 1e-4 sorts their position sweeps (u = dlt (2 x + dlt) / p^2, dlt = dx unit_position =
    6.4 cm: with x = p the switch lies at p = 2e4 dlt = 1276 m, its second condition |v| < 1e-4, v = u / 2, at 638 m):
      phase 0  "covered"      p from just above the switch to 11 km; nodes within 2 % above it for the x sweep (y = 0), the y sweep
                              (x = 0), both (x = y), with either sign;
      phase 1  "fallback"     1 m <= p <= the switch; within 2 % below the switch and below 638 m, p = 1, 30, 300 m;
      phase 2  "undecidable"  p = 0 exactly (both poles), 1e-6 .. 0.1 m; x or y negative and smaller than the step (the perturbed
                              point crosses the axis), x = -dx exactly (it lands on it)
    and no aerodynamics in the last one (the aero path constraints skip the last phase)."""
    prob = _example_prob()
    rng = np.random.default_rng(27)
    nn = list(AXIS_NODES)
    S = len(nn)
    prob["num_nodes"] = np.array(nn, dtype=np.int32)
    prob["thrust"] = np.full(S, 420000.0)
    prob["massflow"] = np.full(S, 140.9)
    prob["reference_area"] = np.full(S, 2.21)
    prob["nozzle_area"] = np.full(S, 0.68)
    prob["engine_on"] = np.ones(S, dtype=np.int32)
    prob["attitude_hold"] = np.zeros(S, dtype=np.int32)
    up, uv, ut, dx = prob["units"][1], prob["units"][2], prob["units"][4], float(prob["dx"])
    step = dx * up
    T = 2.0 * step / POS_DELTA_U          # x = p: |u| = 1e-4
    T2 = T / np.sqrt(2.0)                 # x = y = p / sqrt 2: both sweeps at once
    q = np.pi / 2
    # (p, lon) per state node; node 0 of a phase has an aero row only
    A = [(1.002 * T, 0.0), (1.010 * T, 0.0), (1.019 * T, 2 * q), (1.001 * T, q), (1.012 * T, -q), (1.018 * T, q),
         (1.004 * T2, q / 2), (1.015 * T2, -3 * q / 2), (1.019 * T2, 3 * q / 2), (1.0005 * T, 1e-3), (1.003 * T, q - 1e-3)]
    A += [(pp, ll) for pp, ll in zip(np.geomspace(1.03 * T, 11000.0, nn[0] + 1 - len(A)), np.arange(nn[0] + 1) * 0.61 - 3.0)]
    B = [(1.0, 0.3), (1.0, q), (30.0, 0.0), (30.0, -2.0), (300.0, q), (300.0, 2.5), (0.999 * T, 0.0), (0.990 * T, 2 * q),
         (0.981 * T, 0.0), (0.998 * T, q), (0.985 * T, -q), (0.996 * T2, q / 2), (0.982 * T2, -3 * q / 2), (0.999 * T / 2, 0.0),
         (0.990 * T / 2, q), (0.981 * T / 2, 2 * q), (0.995 * T / 2, -q)]
    B += [(pp, ll) for pp, ll in zip(np.geomspace(1.5, 0.97 * T, nn[1] + 1 - len(B)), np.arange(nn[1] + 1) * 0.47 - 3.0)]
    Cp = np.array([0.0, 0.0, 1e-6, 1e-3, 0.03, 0.05, step, 0.1] * 5)[:nn[2] + 1]
    Cl = np.array([0.0, q, 2 * q, -q, 2 * q, -q, 2 * q, 0.7] * 5)[:nn[2] + 1] + 0.0 * Cp
    Cl[24:] = np.array([0.3, 2.0, -2.5, 1.0, -1.0, 2.9, 2 * q, -0.4] * 2)[:nn[2] + 1 - 24]
    pos, k = [], 0
    levels = np.array([50.0, 700.0, 1500.0, 2500.0, 4000.0, 6000.0, 8000.0, 9500.0, 12500.0, 14000.0, 17500.0, 21000.0, 25000.0,
                       28000.0, 30000.0])
    for nodes in (A, B, list(zip(Cp, Cl))):
        p_, l_ = np.array([v[0] for v in nodes]), np.array([v[1] for v in nodes])
        i = np.arange(len(nodes))
        pos.append(_polar_phase(prob, p_, l_, levels[(3 * i + k) % len(levels)], (i + k) % 2 == 1))
        k += 1
    pos = np.vstack(pos)
    # exact members of the undecidable class: ON the axis (the cos / sin of the builder leave 1e-17 there), and one step short of it
    c0 = nn[0] + nn[1] + 2
    for j in range(nn[2] + 1):
        if Cp[j] == 0.0:
            pos[c0 + j, :2] = 0.0
        elif Cp[j] == step:
            pos[c0 + j, :2] = (-dx, 0.0) if (j // 8) % 2 == 0 else (0.0, -dx)
    M = sum(nn) + S
    speed = rng.uniform(300.0, 2500.0, M) / uv
    d = rng.standard_normal((M, 3))
    vel = d / np.linalg.norm(d, axis=1, keepdims=True) * speed[:, None]
    quat = rng.standard_normal((M, 4))
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    x = np.concatenate([np.linspace(1.0, 0.5, M), pos.ravel(), vel.ravel(), quat.ravel(), 2.0 * rng.standard_normal(2 * sum(nn)),
                        np.array([10.0, 60.0, 110.0, 160.0]) / ut])
    return with_coast_tail(lambda: (prob, x))


def rest_state():
    """One aerodynamic phase of 36 nodes in calm, dense air (0.5 .. 30 km, |lat| <= 70 deg) at rest or nearly at rest in it: at
    three nodes the air-relative velocity v unit - omega x r is EXACTLY zero in fp64, fused or not (x and y are powers of two
    metres, so omega x and omega y are exact products; asserted), at the others |v_air| = 1e-13 .. 30 m/s in a random direction:
    15 below the reference's clamp (|v_air| < 1e-6: alpha = 0), 9 from 3e-6 to 0.6 m/s -- where 1 / |v_air| multiplies a live angle
    of attack and v_air is what is left of terms of |v| + omega |r| = 300 .. 930 m/s --, 10 from 1 to 30 m/s.  Mach <= 0.1: on the
    CA table's first piece (its first knot is Mach 0), below every interior knot."""
    prob = _example_prob()
    rng = np.random.default_rng(72)
    n = 36
    omega = 7.2921151467e-5
    prob["num_nodes"] = np.array([n], dtype=np.int32)
    for k, v in [("thrust", 420000.0), ("massflow", 140.9), ("reference_area", 2.21), ("nozzle_area", 0.68)]:
        prob[k] = np.array([v])
    prob["engine_on"] = np.array([1], dtype=np.int32)
    prob["attitude_hold"] = np.array([0], dtype=np.int32)
    calm = np.array(prob["wind_table"], dtype=np.float64).copy()
    calm[:, 1:] = 0.0
    prob["wind_table"] = calm
    up, uv, ut = prob["units"][1], prob["units"][2], prob["units"][4]
    a_e, b_e = 6378137.0, 6356752.314245
    lat = np.deg2rad(np.linspace(-70.0, 70.0, n + 1))
    lon = rng.uniform(-np.pi, np.pi, n + 1)
    alt = np.geomspace(500.0, 30000.0, n + 1)[rng.permutation(n + 1)]
    R = a_e * b_e / np.sqrt((b_e * np.cos(lat)) ** 2 + (a_e * np.sin(lat)) ** 2) + alt
    r = np.column_stack([R * np.cos(lat) * np.cos(lon), R * np.cos(lat) * np.sin(lon), R * np.sin(lat)])
    exact = {5: (2.0 ** 22, 2.0 ** 21, 1.0), 17: (-2.0 ** 22, 2.0 ** 22, -1.0), 30: (2.0 ** 21, -2.0 ** 20, 1.0)}
    for j, (x0, y0, sg) in exact.items():          # x, y powers of two; z puts the node at its altitude above the ellipsoid
        pp = np.hypot(x0, y0)
        z = b_e * np.sqrt(1.0 - (pp / a_e) ** 2)
        r[j] = (x0, y0, sg * z * (1.0 + alt[j] / np.hypot(pp, z)))
    xr = r / up

    def reaching(target, unit, start):     # a double xs with fl(xs unit) == target, among the neighbours of start
        xs = start
        for _ in range(64):
            got = xs * unit
            if got == target:
                return xs
            xs = np.nextafter(xs, np.inf if (got < target) == (unit > 0) else -np.inf)
        raise AssertionError("no fp64 number scales to %r" % target)

    for j, (x0, y0, _) in exact.items():
        xr[j, 0], xr[j, 1] = reaching(x0, up, x0 / up), reaching(y0, up, y0 / up)
    rs = xr * up
    slow = np.concatenate([np.geomspace(1e-13, 5e-7, 15), [3e-6, 1e-4, 1e-3, 3e-3, 1e-2, 3e-2, 0.1, 0.3, 0.6], np.geomspace(1.0, 30.0, 10)])
    speed = np.zeros(n + 1)          # the three exact nodes get their velocity below
    speed[[j for j in range(n + 1) if j not in exact]] = slow[rng.permutation(len(slow))]
    d = rng.standard_normal((n + 1, 3))
    v = np.column_stack([-omega * rs[:, 1], omega * rs[:, 0], np.zeros(n + 1)]) + d / np.linalg.norm(d, axis=1, keepdims=True) * speed[:, None]
    xv = v / uv
    for j in exact:
        xv[j] = (reaching(-(omega * rs[j, 1]), uv, -(omega * rs[j, 1]) / uv), reaching(omega * rs[j, 0], uv, omega * rs[j, 0] / uv), 0.0)
    vs = xv * uv
    rel = np.column_stack([vs[:, 0] + omega * rs[:, 1], vs[:, 1] - omega * rs[:, 0], vs[:, 2]])
    at_rest = ~rel.any(axis=1)
    assert sorted(np.nonzero(at_rest)[0]) == sorted(exact), "three nodes exactly at rest in the air, in fp64"
    for j in exact:      # ... and the products omega x, omega y are exact, so a fused multiply-add finds the same zero
        assert all(Fraction(omega) * Fraction(rs[j, c]) == Fraction(omega * rs[j, c]) for c in (0, 1))
    # the slowest sound of the standard atmosphere is 295 m/s (11 .. 20 km)
    assert np.linalg.norm(rel, axis=1).max() / 295.0 < np.asarray(prob["ca_table"])[1, 0]
    quat = rng.standard_normal((n + 1, 4))
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    x = np.concatenate([np.linspace(1.0, 0.5, n + 1), xr.ravel(), xv.ravel(), quat.ravel(), 2.0 * rng.standard_normal(2 * n),
                        [10.0 / ut, 160.0 / ut]])
    return with_coast_tail(lambda: (prob, x))


# ---------------------------------------------------------------------------------------------------------------------------
# Small problems over the long wind / CA tables of tests/table_cases.py (tests/test_table_sizes.py, tests/golden/make_long_tables.py)
# ---------------------------------------------------------------------------------------------------------------------------
GEOPOT_R0 = 6356766.0
TABLE_KNOT_OFFSETS = (-0.04, -0.004, 0.004, 0.04)


def _geometric(h):
    """geometric altitude whose geopotential altitude (src/Air.cpp:47-54) is h: the inverse of r0 z / (r0 + z) below 86 km
    geometric, h itself from there on.  Geopotential 84 852 .. 86 000 m is the image of no altitude."""
    h = np.asarray(h, dtype=np.float64)
    assert not np.any((h > 84850.0) & (h < 86000.0))
    return np.where(h < 84851.0, GEOPOT_R0 * h / (GEOPOT_R0 - h), h)


def table_knots(case):
    """the (up to) six wind knots the `knots` vector sits around: the first and the last row among them"""
    import table_cases as TC
    alt = TC.CASES[case][0][:, 0]
    K = len(alt)
    idx = sorted({0, 1, K // 3, K // 2, K - 2, K - 1})
    return [float(alt[k]) for k in idx if not 84850.0 < alt[k] < 86000.0]


def table_state(case, nn, vector="climb"):
    """Aerodynamic phases of nn[:-1] nodes and a coasting tail of nn[-1] without aerodynamics, over the wind and CA tables of
    tests/table_cases.py CASES[case].
      "climb"  the state nodes climb from 50 m to 130 km: two below the wind table's first row, three above its last, the others
               inside as many different intervals of it as there are nodes (none within 1 m of a knot); air-relative speeds aim
               at Mach 0.05 .. 20 -- inside as many different CA intervals as possible, some above the last Mach row;
      "knots"  the same, but for nodes 4 mm and 4 cm below and above table_knots(case) (the geodetic construction of
               layer_break_state): a position sweep (dx * unit = 6.4 cm) carries some of them across the knot."""
    import oracle
    import table_cases as TC
    assert vector in ("climb", "knots") and len(nn) >= 2
    prob = TC.with_tables(_example_prob(), case)
    wind, ca = TC.CASES[case]
    rng = np.random.default_rng(1000 + sum(nn) + len(wind))
    S = len(nn)
    prob["num_nodes"] = np.array(nn, dtype=np.int32)
    prob["thrust"] = np.array([420000.0, 30700.0, 9000.0][:S - 1] + [0.0])
    prob["massflow"] = np.array([140.9, 9.8, 2.5][:S - 1] + [0.0])
    prob["reference_area"] = np.array([2.21, 1.3, 0.7][:S - 1] + [0.0])
    prob["nozzle_area"] = np.array([0.68, 0.1, 0.0][:S - 1] + [0.0])
    prob["engine_on"] = np.array([1] * (S - 1) + [0], dtype=np.int32)
    prob["attitude_hold"] = np.zeros(S, dtype=np.int32)
    up, uv, ut = prob["units"][1], prob["units"][2], prob["units"][4]
    N, M = sum(nn), sum(nn) + S
    Ma = M - (nn[-1] + 1)                                            # state nodes of the aerodynamic phases
    # geopotential altitudes: below, inside (one interval each while there are enough), above
    gaps = np.diff(wind[:, 0])
    usable = [k for k in range(len(gaps)) if gaps[k] >= 2.5 and not (wind[k, 0] < 86000.0 and wind[k + 1, 0] > 84850.0)]
    n_in = Ma - 5
    pick = [usable[i] for i in np.unique(np.round(np.linspace(0, len(usable) - 1, min(n_in, len(usable)))).astype(int))]
    pick = (pick * (n_in // len(pick) + 1))[:n_in]
    f = rng.uniform(0.3, 0.7, n_in)
    inside = np.array([wind[k, 0] + min(max(1.05, fi * gaps[k]), gaps[k] - 1.05) for k, fi in zip(pick, f)])
    h = np.sort(np.concatenate([[50.0, min(150.0, 0.5 * (50.0 + wind[0, 0]))] if wind[0, 0] > 60.0 else [50.0, 1500.0], inside,
                                [100e3, 115e3, 130e3]]))
    alt = _geometric(h)
    if vector == "knots":
        at = np.round(np.linspace(1, Ma - 2, 4 * len(table_knots(case)))).astype(int)
        assert len(set(at)) == len(at)
        alt[at] = [float(_geometric(hk)) + off for hk in table_knots(case) for off in TABLE_KNOT_OFFSETS]
    alt = np.concatenate([alt, np.full(M - Ma, alt[-1])])
    lat = np.concatenate([rng.uniform(-1.0, 1.0, Ma), np.zeros(M - Ma)])
    lon = np.concatenate([rng.uniform(-np.pi, np.pi, Ma), np.zeros(M - Ma)])
    lat[Ma:], lon[Ma:] = lat[Ma - 1], lon[Ma - 1]
    a_e, b_e = 6378137.0, 6356752.314245
    e2 = 1.0 - (b_e / a_e) ** 2
    Np = a_e / np.sqrt(1.0 - e2 * np.sin(lat) ** 2)
    r = np.column_stack([(Np + alt) * np.cos(lat) * np.cos(lon), (Np + alt) * np.cos(lat) * np.sin(lon), (Np * (1.0 - e2) + alt) * np.sin(lat)])
    # Mach targets: the middle of a CA interval each, in shuffled order; the ends and beyond the last row
    mids = 0.5 * (ca[:-1, 0] + ca[1:, 0])
    mach = np.concatenate([[0.05, 0.5 * (ca[-1, 0] + 20.0), 12.0, 20.0], np.tile(mids, Ma // len(mids) + 1)])[:Ma]
    mach = np.concatenate([mach[rng.permutation(Ma)], np.full(M - Ma, 5.0)])
    hh = np.array([oracle.geopotential_altitude(z) for z in alt])
    sound = np.array([oracle.speed_of_sound(z) for z in hh])
    d = rng.standard_normal((M, 3))
    omega = 7.2921151467e-5
    v = np.column_stack([-omega * r[:, 1], omega * r[:, 0], np.zeros(M)]) + d / np.linalg.norm(d, axis=1, keepdims=True) * (mach * sound)[:, None]
    quat = rng.standard_normal((M, 4))
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    t = np.array([10.0, 160.0, 400.0, 640.0][:S - 1] + [0.0]) / ut
    t[-1] = t[-2] + 10.0 / ut
    x = np.concatenate([np.linspace(1.0, 0.4, M), (r / up).ravel(), (v / uv).ravel(), quat.ravel(), 2.0 * rng.standard_normal(2 * N),
                        [5.0 / ut], t])
    return prob, x


def table_node_times(prob, x):
    """tx [M]: the time of every state node in seconds (output_result.py:121-143 with the oracle's LGR nodes)"""
    import oracle
    nn = [int(v) for v in prob["num_nodes"]]
    S, N = len(nn), sum(nn)
    M = N + S
    tn = x[11 * M + 2 * N:] * float(prob["units"][4])
    return np.concatenate([np.concatenate([[-1.0], oracle.lgr_nodes(n)]) * (tn[s + 1] - tn[s]) / 2.0 + (tn[s + 1] + tn[s]) / 2.0
                           for s, n in enumerate(nn)])


def table_oracle_rows(prob, x, launch=(28.5, 0.0)):
    """{column: [M]} of the oracle's post-processing table (oracle/output_table.py) of (prob, x) on prob's own tables: "altitude"
    (geodetic, m) and "M" (Mach number) per state node among them"""
    from oracle import output_table as ot
    nn = [int(v) for v in prob["num_nodes"]]
    S, N = len(nn), sum(nn)
    params = [(prob["thrust"][s], prob["reference_area"][s], prob["nozzle_area"][s]) for s in range(S)]
    return ot.table(x, N + S, N, nn, tuple(prob["units"][:3]), table_node_times(prob, x), params, np.asarray(prob["wind_table"]),
                    np.asarray(prob["ca_table"]), launch[0], launch[1])


def check_table_state(case, nn, vector):
    """what table_state promises, from the oracle's altitude and Mach number per node -> (wind intervals hit, CA intervals hit)"""
    import oracle
    import table_cases as TC
    prob, x = table_state(case, nn, vector)
    wind, ca = TC.CASES[case]
    T = table_oracle_rows(prob, x)
    Ma = sum(nn) + len(nn) - (nn[-1] + 1)
    alt, mach = T["altitude"][:Ma], T["M"][:Ma]
    h = np.array([oracle.geopotential_altitude(z) for z in alt])
    assert alt.min() < 60.0 and alt.max() > 129e3 and mach.min() < 0.2 and mach.max() > 15.0
    assert (h < wind[0, 0]).sum() >= (2 if wind[0, 0] > 60.0 else 0) and (h > wind[-1, 0]).sum() >= 3 and (mach > ca[-1, 0]).sum() >= 3
    dk = np.abs(h[:, None] - wind[None, :, 0]).min(axis=1)
    assert np.abs(mach[:, None] - ca[None, :, 0]).min() > 1e-6
    if vector == "climb":
        assert dk.min() > 1.0
    else:
        near = np.sort(dk)[:4 * len(table_knots(case))]
        assert np.all(near < 0.05) and (near < 0.01).sum() == 2 * len(table_knots(case)) and np.sort(dk)[4 * len(table_knots(case))] > 1.0
        for hk in table_knots(case):                               # two nodes on either side of every knot
            side = h[np.abs(h - hk) < 0.05] - hk
            assert (side < 0).sum() == 2 and (side > 0).sum() == 2, (hk, side)
    inw = h[(h > wind[0, 0]) & (h <= wind[-1, 0])]
    inc = mach[(mach > ca[0, 0]) & (mach <= ca[-1, 0])]
    hit_w = len(set(np.searchsorted(wind[:, 0], inw, side="left") - 1))
    hit_c = len(set(np.searchsorted(ca[:, 0], inc, side="left") - 1))
    return hit_w, hit_c

"""The (state, position step) cases of tests/test_exact_fd_steps.py and tests/golden/make_exact_fd_steps.py: the states of
tests/states.py on problems whose position step dx * unit_position runs from 1e-5 m to the 1 m at which the engine's host hands
the position sweeps over to the recomputing form (gel_host.hip: !(fabs(dx * unit_position) <= 1.0)).

A step is reached by dx alone (every sweep of the Jacobian then takes that dx) or by unit_position alone (dx = 1e-8: the mass,
velocity and quaternion sweeps keep the reference's step).  A state built for another unit_position keeps its positions in
metres: the normalised components are rescaled, r / unit_position."""
import hashlib

import numpy as np

import states


def example_unit_position():
    return float(states._example_prob()["units"][1])


def dx_at_the_switch(up):
    """-> (dx_one, dx_over): the largest double with fl(dx * up) <= 1.0 and the next one above it, the product formed as the host
    forms it"""
    up = np.float64(up)
    dx = np.float64(1.0) / up
    while np.float64(dx) * up <= 1.0:
        dx = np.nextafter(dx, np.inf)
    while not (np.float64(dx) * up <= 1.0):
        dx = np.nextafter(dx, -np.inf)
    over = np.nextafter(dx, np.inf)
    assert dx * up <= 1.0 and over * up > 1.0
    return float(dx), float(over)


def step_cases():
    """{label: (dx, unit_position)} of the steps the difference form accepts"""
    up = example_unit_position()
    return {"1e-5m": (1e-5 / up, up), "1e-3m": (1e-3 / up, up), "0.25m": (0.25 / up, up), "one": (dx_at_the_switch(up)[0], up),
            "unit1e8": (1e-8, 1e8), "unit1e3": (1e-8, 1e3)}


STATES = ("layers", "polar", "breaks", "breaks_m")      # breaks_m: the break state mirrored, layer_break_state(step=-step)
STEPS = ("1e-5m", "1e-3m", "0.25m", "one", "unit1e8", "unit1e3")
AERO_CASE = "aero_polar@one"      # states.with_coast_tail(states.polar_dense_state) at the switch: the aero rows' fixture


def with_step(prob, x, dx, up):
    """(prob, x) with the position step dx * up: the same positions in metres (to rounding)"""
    prob = dict(prob)
    x = x.copy()
    up0 = float(prob["units"][1])
    units = np.array(prob["units"], dtype=np.float64).copy()
    units[1] = up
    prob["units"] = units
    prob["dx"] = float(dx)
    nn = [int(v) for v in prob["num_nodes"]]
    M = sum(nn) + len(nn)
    if up != up0:
        x[M:4 * M] = x[M:4 * M] * up0 / up
    return prob, x


def build(state, label, coast_tail=False):
    """-> (prob, x) of `state` at the step `label` (or (dx, unit_position) itself)"""
    dx, up = step_cases()[label] if isinstance(label, str) else label
    step = float(np.float64(dx) * np.float64(up))
    make = {"layers": states.all_layers_state, "polar": states.polar_dense_state,
            "breaks": lambda: states.layer_break_state(step=step), "breaks_m": lambda: states.layer_break_state(step=-step)}[state]
    prob, x = states.with_coast_tail(make) if coast_tail else make()
    return with_step(prob, x, dx, up)


def digest(x):
    """what the fixture keeps of a decision vector: the SHA-256 of its bytes, as 32 uint8"""
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(x, dtype=np.float64).tobytes()).digest(), dtype=np.uint8).copy()

"""What the tests of plans whose RK4 step count differs by phase share (tests/test_mixed_steps*.py): the
four flights, their wrong step assignments, the rows of a phase, and the fixtures' reader.

gel_prop_plan_create takes one step count per phase, and every flight kernel forms its phase's offsets -- the stage points, the
control samples, the step fractions, the adjoint's inner checkpoints -- from those counts.  With one count for all phases an offset
formed with a neighbour's count, or a sample block advanced over a held phase, changes no result.  These flights make every phase's
count differ from its predecessor's:

  N-chain    noair   chain    (3, 1, 4)   inner checkpoints on the held phase 0, k = 1 behind k = 3, k_max on a sampled phase
  N-section  noair   section  (2, 4, 1)
  E-chain    example chain    (1, 3, 2, 1, 2, 3, 1, 3, 2, 1, 2, 3)   k = 3 on the free aerodynamic phase 1, k = 2 on the 16-node phase 2,
  E-section  example section  the same                              k = 2 and 3 on the held phases 4 and 5; 125 steps in all

All are flight_tangent_truth.case's batches of three; the truth (tests/golden/g32_mixed_steps_noair.npz, g33_mixed_steps_example.npz,
written by tests/golden/make_flight_mixed_steps.py) holds vector 1.  The N flights store what g30 and g31 store per flight, the
per-stage F, J, Pu, Pf and verr included; the E flights dy, its bound, gx, gdisp and their bounds alone."""
import os

import numpy as np

import flight_tangent_truth as tt

HERE = os.path.dirname(os.path.abspath(__file__))
G32 = os.path.join(HERE, "golden", "g32_mixed_steps_noair.npz")
G33 = os.path.join(HERE, "golden", "g33_mixed_steps_example.npz")
E_STEPS = (1, 3, 2, 1, 2, 3, 1, 3, 2, 1, 2, 3)
CASES = {"N-chain": ("noair", "chain", (3, 1, 4)), "N-section": ("noair", "section", (2, 4, 1)),
         "E-chain": ("example", "chain", E_STEPS), "E-section": ("example", "section", E_STEPS)}
NAMES = tuple(CASES)
N_NAMES = ("N-chain", "N-section")       # the flights whose per-stage data is stored
WRONG = ("rolled", "reversed", "uniform_max", "uniform_1")


def wrong_steps(steps, how):
    """a wrong assignment of the same counts: rolled by one phase (phase s gets phase s - 1's), reversed, max(steps) or 1 everywhere"""
    k = [int(v) for v in steps]
    return {"rolled": tuple(k[-1:] + k[:-1]), "reversed": tuple(k[::-1]), "uniform_max": (max(k),) * len(k), "uniform_1": (1,) * len(k)}[how]


def fixture_of(name):
    return G32 if name in N_NAMES else G33


def load(name):
    """the stored truth of one of NAMES -> dict (see the module)"""
    g = np.load(fixture_of(name))
    key = name + "_"
    return {k[len(key):]: g[k] for k in g.files if k.startswith(key)}


def phase_rows(nn):
    """[slice of the state rows of phase s]"""
    return [slice(sum(nn[:s]) + s, sum(nn[:s]) + s + nn[s] + 1) for s in range(len(nn))]


def _differs_from_predecessor(steps):
    for s, k in enumerate(steps):
        assert s == 0 or k != steps[s - 1], steps


for _c in CASES.values():
    _differs_from_predecessor(_c[2])
assert all(wrong_steps(c[2], h) != c[2] for c in CASES.values() for h in WRONG)
assert tt.TRUTH_VEC == 1

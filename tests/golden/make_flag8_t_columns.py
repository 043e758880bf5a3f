#!/usr/bin/env python3
"""The t0 / tf columns of the velocity defect under GEL_FLAG_FD_RECOMPUTE on the windy small problems, as the engine gives them
(tests/golden/g37_flag8_t_columns_in_wind.npz; tests/test_pos_repark.py reads it).

A RECORD of the engine's own bits, not an independent truth: the committed file was written with the library of commit 9459ea5, the
last one whose position part carried the half-latitude pair, on an MI355X.  The two sweeps evaluate their perturbed point with the
reference's quaternion chain (wind_eci_chain()), which since then forms the half-latitude pair itself from (sin lat, cos lat): the
fixture pins that its statements round as pos_part()'s did.  Run it again only with a library that is meant to become the new record.
Per case (test_wind_axes.small_problem `3x8` and `n5`, the never-calm table, Engine flags 1 | 8, one evaluation of x0): the SHA-256
of the decision vector and the vel / t block's values.

Usage (needs the GPU):  python tests/golden/make_flag8_t_columns.py"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def columns(case):
    """-> (sha256 of x0 as 32 uint8, vel / t values of one evaluation with GEL_FLAG_FD_RECOMPUTE)"""
    from gelato_amd import Engine
    from test_wind_axes import small_problem
    prob, x0 = small_problem(case, "windy")
    E = Engine(prob, flags=1 | 8)
    _, vals, rc = E.eval(x0)
    assert rc == 0
    sha = np.frombuffer(hashlib.sha256(np.ascontiguousarray(x0, dtype=np.float64).tobytes()).digest(), dtype=np.uint8).copy()
    return sha, E.jac_dicts(vals)["vel"]["t"]["coo"][2].copy()


if __name__ == "__main__":
    out = {}
    for case in ("3x8", "n5"):
        out[case + "_x_sha256"], out[case + "_vel_t"] = columns(case)
    np.savez_compressed(os.path.join(HERE, "g37_flag8_t_columns_in_wind.npz"), **out)

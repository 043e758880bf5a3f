#!/usr/bin/env python3
"""g25_interp_matrices.npz: the interpolation plans' matrices (include/gelato_amd.h gel_interp_matrices) in 50-digit arithmetic.

For every transfer a -> b in PAIRS, with tau_a / tau_b the fp64 nodes a host-only handle reports (gel_problem_tau), taken as exact:
  Wx_a_b [b+1, a+1]  Lagrange basis on [-1, tau_a] at [-1, tau_b]
  Wu_a_b [b, a]      Lagrange basis on tau_a at tau_b
and one table-mode list on n = TABLE_N: table_pts (-1, +1, a node value, irrational points), table_Wx [P, n+1], table_Wu [P, n].
A point that equals a support node gives the unit row.  Rounded once to fp64.  mpmath at 50 digits, barycentric form.
Deterministic: rerunning reproduces the file byte for byte.     python3 tests/golden/make_interp_matrices.py"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
PAIRS = ((3, 5), (5, 3), (8, 12), (64, 80), (128, 64), (64, 64))
TABLE_N = 8
mp.mp.dps = 50


def handle_tau(n):
    from gelato_amd import _lib
    tau = np.zeros(n)
    _lib.check(_lib.lib().gel_lgr_nodes(n, tau.ctypes.data_as(_lib._dp)))
    return tau


def weights(t):
    w = []
    for i in range(len(t)):
        p = mp.mpf(1)
        for m in range(len(t)):
            if m != i:
                p *= t[i] - t[m]
        w.append(1 / p)
    return w


def basis_rows(t, pts):
    w = weights(t)
    rows = []
    for z in pts:
        hit = [i for i, ti in enumerate(t) if z == ti]
        if hit:
            rows.append([1.0 if k == hit[0] else 0.0 for k in range(len(t))])
            continue
        terms = [w[i] / (z - t[i]) for i in range(len(t))]
        s = mp.fsum(terms)
        rows.append([float(v / s) for v in terms])
    return np.array(rows)


def main():
    out = {"pairs": np.array(PAIRS, dtype=np.int32)}
    taus = {}
    for a, b in PAIRS:
        for n in (a, b):
            if n not in taus:
                taus[n] = handle_tau(n)
                out["tau_%d" % n] = taus[n]
        ta = [mp.mpf(float(v)) for v in taus[a]]
        tb = [mp.mpf(float(v)) for v in taus[b]]
        out["Wx_%d_%d" % (a, b)] = basis_rows([mp.mpf(-1)] + ta, [mp.mpf(-1)] + tb)
        out["Wu_%d_%d" % (a, b)] = basis_rows(ta, tb)
    n = TABLE_N
    if n not in taus:
        taus[n] = handle_tau(n)
        out["tau_%d" % n] = taus[n]
    pts = np.array([-1.0, 1.0, taus[n][3], float(mp.sqrt(2) - 1), float(-1 / mp.pi), float(mp.e - 3), float(-mp.sqrt(3) / 2),
                    taus[n][0], 0.0, float(mp.pi - 3)])
    t = [mp.mpf(float(v)) for v in taus[n]]
    z = [mp.mpf(float(v)) for v in pts]
    out["table_n"] = np.array(n, dtype=np.int32)
    out["table_pts"] = pts
    out["table_Wx"] = basis_rows([mp.mpf(-1)] + t, z)
    out["table_Wu"] = basis_rows(t, z)
    path = os.path.join(HERE, "g25_interp_matrices.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()

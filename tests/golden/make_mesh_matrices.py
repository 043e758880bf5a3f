#!/usr/bin/env python3
"""g23_mesh_matrices.npz: the collocation error estimate's matrices (include/gelato_amd.h gel_mesh_matrices) in 50-digit arithmetic.

For n in NS: tau_n = the flipped LGR points of n (the negated roots of P_{n-1} + P_n, ending at +1), sigma_n = those of n + 1,
  Lx_n [n+1, n+1]  Lagrange basis on [-1, tau_n] at sigma_n
  Lu_n [n+1, n]    Lagrange basis on tau_n at sigma_n
  I_n  [n+1, n+1]  (D^[:, 1:])^-1, D^[k][i] = l_i'(s_{k+1}) on s = [-1, sigma_n]
rounded once to fp64.  mpmath at 50 digits: roots by Newton from numpy's fp64 roots, the bases and D^ in closed form, the inverse by
mpmath's LU.  Deterministic: rerunning reproduces the file byte for byte.     python3 tests/golden/make_mesh_matrices.py"""
import os

import mpmath as mp
import numpy as np
from numpy.polynomial import legendre as npleg

HERE = os.path.dirname(os.path.abspath(__file__))
NS = (2, 3, 4, 5, 8, 16, 32, 64)
mp.mp.dps = 50


def lgr_flipped(n):
    c = np.zeros(n + 1)
    c[n - 1] = c[n] = 1.0
    guesses = np.sort(npleg.legroots(c).real)
    f = lambda x: mp.legendre(n - 1, x) + mp.legendre(n, x)
    roots = [mp.mpf(-1)] + [mp.findroot(f, mp.mpf(float(g))) for g in guesses if g > -1 + 1e-12]
    assert len(roots) == n
    tau = sorted(-r for r in roots)
    tau[-1] = mp.mpf(1)
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


def basis(t, z):
    w = weights(t)
    for i, ti in enumerate(t):
        if z == ti:
            return [mp.mpf(1) if k == i else mp.mpf(0) for k in range(len(t))]
    terms = [w[i] / (z - t[i]) for i in range(len(t))]
    s = mp.fsum(terms)
    return [v / s for v in terms]


def matrices(n):
    tau = lgr_flipped(n)
    sig = lgr_flipped(n + 1)
    tx = [mp.mpf(-1)] + tau
    Lx = [basis(tx, z) for z in sig]
    Lu = [basis(tau, z) for z in sig]
    sup = [mp.mpf(-1)] + sig
    ws = weights(sup)
    P = n + 1
    A = mp.matrix(P, P)
    for k in range(P):
        diag = mp.mpf(0)
        for i in range(P + 1):
            if i == k + 1:
                continue
            v = (ws[i] / ws[k + 1]) / (sup[k + 1] - sup[i])
            if i > 0:
                A[k, i - 1] = v
            diag -= v
        A[k, k] = diag
    Ainv = A ** -1
    f = lambda rows: np.array([[float(v) for v in r] for r in rows])
    return (np.array([float(v) for v in tau]), np.array([float(v) for v in sig]), f(Lx), f(Lu),
            np.array([[float(Ainv[i, j]) for j in range(P)] for i in range(P)]))


def main():
    out = {}
    for n in NS:
        tau, sig, Lx, Lu, I = matrices(n)
        out["tau_%d" % n], out["sigma_%d" % n], out["Lx_%d" % n], out["Lu_%d" % n], out["I_%d" % n] = tau, sig, Lx, Lu, I
    out["ns"] = np.array(NS, dtype=np.int32)
    path = os.path.join(HERE, "g23_mesh_matrices.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()

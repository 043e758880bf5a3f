"""The truth of gel_batch_quantiles* (include/gelato_amd.h), numpy only: a plain sort of the 64-bit keys of the
finite entries of every column, and the rank rule.  Order statistics depend on no order of operations, so the device is held to
these bits with no tolerance.  lerp_exact forms the interpolated quantile in rational arithmetic (for the Python layer's "value")."""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
SIGN = np.uint64(1) << np.uint64(63)
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def keys(a):
    """u ^ (u >> 63 ? ~0 : 1 << 63): ascending keys are ascending doubles, -0.0 before +0.0"""
    u = bits(a)
    return u ^ np.where((u >> np.uint64(63)).astype(bool), ALL, SIGN)


def unkeys(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return (k ^ np.where((k >> np.uint64(63)).astype(bool), SIGN, ALL)).view(np.float64)


def same(a, b):
    """bit for bit (a -0.0 is not a 0.0), NaN where the other has NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb]))


def ranks(p, n, lower_of=np.floor):
    """the rank rule: h = p * (n - 1) in fp64, one rounding; (floor(h), ceil(h))"""
    h = np.float64(p) * np.float64(n - 1)
    return int(lower_of(h)), int(np.ceil(h))


def order_stats(A, probs):
    """A [B, W] (or [B]) -> {"lower", "upper" [W, nq] float64 (NaN where count = 0), "count" [W] int64,
    "who_lower", "who_upper" [W, nq] int64 (-1 where count = 0)}"""
    A = np.asarray(A, dtype=np.float64)
    A = A.reshape(A.shape[0], -1)
    probs = np.atleast_1d(np.asarray(probs, dtype=np.float64))
    B, W = A.shape
    nq = probs.size
    lower, upper = np.full((W, nq), np.nan), np.full((W, nq), np.nan)
    count = np.zeros(W, dtype=np.int64)
    who = np.full((2, W, nq), -1, dtype=np.int64)
    for w in range(W):
        col = np.ascontiguousarray(A[:, w])
        fin = np.isfinite(col)
        n = count[w] = int(fin.sum())
        if n == 0:
            continue
        k = keys(col)
        ks = np.sort(k[fin])
        for j, p in enumerate(probs):
            for side, r in enumerate(ranks(p, n)):
                kk = ks[r]
                (lower, upper)[side][w, j] = unkeys(np.array([kk]))[0]
                who[side, w, j] = int(np.nonzero(fin & (k == kk))[0][0])
    return {"lower": lower, "upper": upper, "count": count, "who_lower": who[0], "who_upper": who[1]}


def lerp_exact(p, n, lower, upper):
    """lower + (upper - lower) (h - floor(h)) with h = fl(p (n - 1)), as a Fraction (finite lower, upper; n >= 1)"""
    h = np.float64(p) * np.float64(n - 1)
    f = Fraction(float(h)) - int(np.floor(h))
    return Fraction(float(lower)) + (Fraction(float(upper)) - Fraction(float(lower))) * f

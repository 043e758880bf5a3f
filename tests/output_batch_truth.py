"""What gel_output_table_batch's reductions are checked against (tests/test_output_batch_cpu.py, tests/test_output_batch.py): the
exactly rounded statistics of a table, the bound the device's mean and m2 must keep to them, and plain restatements of the peaks
and of the stated reduction order -- in Python floats without the fma (welford_merge: inside the bound) and exactly as written, the
fma in one rounding (welford_merge_exact: what the device gives bit for bit).  numpy, Python integers and fractions only, no GPU.

The order the header states (include/gelato_amd.h): blocks of BLOCK = 256 consecutive vectors; inside a block Welford's update over
the finite entries in ascending b,
    n += 1;  d = v - mean;  mean = mean + d / n;  m2 = fma(d, v - mean, m2)
and the blocks that hold a finite entry merged in ascending order into a running total (the first is copied), Chan's form,
    nt = n + nb;  d = mean_b - mean;  mean = mean + d (nb / nt);  m2 = (m2 + m2_b) + (d d) ((n nb) / nt).

The bound, derived for that order.  Notation: n = count of finite entries, K = number of blocks of the batch (ceil(B / 256)),
nb = min(n, 256) (no block holds more), u = 2^-53, |v|_2 the 2-norm of the finite entries, m2 their exact sum of squared
deviations; m_k / S_k the exact running mean / m2 of the first k entries of a block, hats the computed ones.  First order in u
throughout; the factor 1 / (1 - 4 (n + K + 8) u) at the end absorbs the products of roundings (the usual gamma_k argument).

  Mean.  A Welford step commits three roundings: mean_k^ = m_{k-1}^ (1 - 1/k) + v_k / k + eta_k with
  |eta_k| <= 2 u |d_k| / k + u |m_k|, so k e_k = (k - 1) e_{k-1} + k eta_k and  k |e_k| <= sum_{j<=k} (2 u |d_j| + j u |m_j|).
  Cauchy-Schwarz gives j |m_j| = |sum_{i<=j} v_i| <= sqrt(j) |v|_2, hence sum_j j |m_j| <= k sqrt(k) |v|_2; and since
  d2_j = v_j - m_j = d_j (j - 1) / j and sum_j d_j d2_j = S_k, sum_{j>=2} d_j^2 <= 2 S_k, hence sum_j |d_j| <= sqrt(2 k S_k).
  Together  |e_k| <= u (sqrt(k) |v|_2 + 2 sqrt(2 m2 / k)) <= u (sqrt(n) |v|_2 + 3 sqrt(m2)).
  A merge commits four roundings, u (3 |d| nb / nt + |mean|) <= 7 u max|v| <= 7 u |v|_2, and passes the errors it receives on as
  a convex combination.  Every intermediate mean, block or running total, therefore errs by at most
      E = u (sqrt(n) |v|_2 + 3 sqrt(m2) + 7 (K - 1) |v|_2)                                                    -- mean_bound
  m2 inside a block.  m2_k^ = fma(d_k^, d2_k^, m2_{k-1}^): the product of two rounded differences of v_k and two erring means, one
  rounding of the fma.  Its error is at most |d2_k| |e_{k-1}| + |d_k| |e_k| + 2 u |d_k d2_k| + u S_k.  Summed over a block of nb
  entries: the last two give (nb + 2) u m2; the first two give 2 E sum |d_k| <= 2 E sqrt(2 nb m2_block), with E the block's own
  u (sqrt(nb) |v_b|_2 + 3 sqrt(m2_b)).  Over the blocks (Cauchy-Schwarz once more: sum_b |v_b|_2 sqrt(m2_b) <= |v|_2 sqrt(m2), and
  sum_b m2_b <= m2):
      u ((nb + 2 + 6 sqrt(2 nb)) m2 + 2 sqrt(2) nb |v|_2 sqrt(m2))
  m2 across the merges.  A merge adds d^2 w, w = n nb / nt <= nb, with d from two erring means (|error of d| <= 2 E) and commits six
  roundings: at most 4 E |d| w + 4 u d^2 w + 2 u m2.  The exact d^2 w of the K - 1 merges sum to at most m2 and sum_w <= n, so
  sum |d| w <= sqrt(n m2):
      (K > 1)  4 E sqrt(n m2) + (4 + 2 (K - 1)) u m2
  m2_bound is the sum of the two displays: of the known form c count u (m2 + |v|_2 sqrt(m2)) of the updating algorithms (Chan, Golub
  and LeVeque 1983), with c = 2 sqrt 2 inside one block and 2 sqrt 2 + 4 with merges, and lower-order terms written out.  A sum of
  squares minus count mean^2 errs by count u |v|_2^2 = (|v|_2 / sqrt(m2)) times that: where |v|_2 / sqrt(m2) >= 1e6 it cannot pass.
"""
import math
from fractions import Fraction

import numpy as np

BLOCK = 256
U = 2.0 ** -53
ENV_FIELDS = ("count", "mean", "m2", "min", "max", "argmin", "argmax", "first_nonfinite")
EXACT_FIELDS = ("count", "min", "max", "argmin", "argmax", "first_nonfinite")


def exact_stats(v):
    """one (node, column) over the vectors: v [B] -> dict of the exactly rounded statistics and the norms the bound needs"""
    v = np.asarray(v, dtype=np.float64)
    fin = np.isfinite(v)
    w = v[fin]
    n = int(w.size)
    bad = np.nonzero(~fin)[0]
    out = {"count": n, "first_nonfinite": int(bad[0]) if bad.size else -1}
    if n == 0:
        out.update(mean=math.nan, m2=math.nan, min=math.nan, max=math.nan, argmin=-1, argmax=-1, l2=0.0, m2_exact=Fraction(0))
        return out
    m, e = np.frexp(w)
    mi = np.ldexp(m, 53).astype(np.int64).tolist()          # exact: |m| < 1 has 53 bits
    e = (e.astype(np.int64) - 53)
    emin = int(e.min())
    ints = [a << s for a, s in zip(mi, (e - emin).tolist())]
    S, Q = sum(ints), sum(a * a for a in ints)
    scale = Fraction(2) ** emin
    m2x = Fraction(n * Q - S * S, n) * scale * scale        # sum (v - mean)^2 = sum v^2 - (sum v)^2 / n, exactly
    idx = np.nonzero(fin)[0]
    out.update(mean=float(Fraction(S, n) * scale), m2=float(m2x), min=float(w.min()), max=float(w.max()),
               argmin=int(idx[np.argmin(w)]), argmax=int(idx[np.argmax(w)]),          # numpy: the first occurrence
               l2=math.sqrt(float(Fraction(Q) * scale * scale)), m2_exact=m2x)
    return out


def bounds(st, B):
    """(mean_bound, m2_bound) of the module docstring for one pair's exact statistics and the batch size"""
    n = st["count"]
    if n == 0:
        return 0.0, 0.0
    K = (B + BLOCK - 1) // BLOCK
    nb = min(n, BLOCK)
    l2, m2 = st["l2"], st["m2"]
    r = math.sqrt(m2)
    E = U * (math.sqrt(n) * l2 + 3.0 * r + 7.0 * (K - 1) * l2)
    bm2 = U * ((nb + 2 + 6.0 * math.sqrt(2.0 * nb)) * m2 + 2.0 * math.sqrt(2.0) * nb * l2 * r)
    if K > 1:
        bm2 += 4.0 * E * math.sqrt(n * m2) + (4 + 2 * (K - 1)) * U * m2
    g = 1.0 / (1.0 - 4.0 * (n + K + 8) * U)
    return E * g, bm2 * g


def std_of(count, m2):
    """sqrt(m2 / (count - 1)) where count >= 2, else NaN: what Engine.output_table_batch reports as std"""
    count, m2 = np.asarray(count), np.asarray(m2, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(count >= 2, np.sqrt(m2 / np.maximum(count - 1, 1)), np.nan)


def check_envelope(table, env, std=None):
    """table [B, M, nc] (the device's own), env [M, nc, 8] (, std [M, nc]) -> {"mean": s, "m2": s, "std": s}: the largest share of
    the bound used per field.  count, min, max, argmin, argmax, first_nonfinite must be exactly numpy's (first index under < / >,
    finite entries only), the count == 0 pattern NaN / -1, m2 exactly 0 where count == 1; mean and m2 within the derived bound of
    the exactly rounded values (plus half an ulp of the reference itself); std within what m2's bound leaves of it."""
    table, env = np.asarray(table), np.asarray(env)
    B, M, nc = table.shape
    assert env.shape == (M, nc, len(ENV_FIELDS)), env.shape
    share = {"mean": 0.0, "m2": 0.0, "std": 0.0}
    for i in range(M):
        for c in range(nc):
            st, got = exact_stats(table[:, i, c]), dict(zip(ENV_FIELDS, env[i, c].tolist()))
            where = (i, c)
            for f in EXACT_FIELDS:
                a, b = got[f], st[f]
                assert (a == b) or (a != a and b != b), (where, f, a, b)
            if st["count"] == 0:
                assert math.isnan(got["mean"]) and math.isnan(got["m2"]), (where, got)
                assert std is None or math.isnan(std[i, c]), where
                continue
            if st["count"] == 1:
                assert got["m2"] == 0.0 and got["mean"] == st["mean"], (where, got)
            bmean, bm2 = bounds(st, B)
            for f, b in (("mean", bmean), ("m2", bm2)):
                d = abs(got[f] - st[f])
                lim = b + U * abs(st[f])
                assert d <= lim, (where, f, got[f], st[f], d, lim, st["count"])
                if d > 0.0:
                    share[f] = max(share[f], d / lim)
            assert got["m2"] >= 0.0, (where, got["m2"])
            if std is not None:
                if st["count"] < 2:
                    assert math.isnan(std[i, c]), where
                    continue
                sx = math.sqrt(float(st["m2_exact"] / (st["count"] - 1)))
                # |sqrt(a) - sqrt(b)| <= |a - b| / sqrt(max(a, b)) and two more roundings; m2 = 0: sqrt of the bound itself
                lim = (math.sqrt(bm2 / (st["count"] - 1)) if sx == 0.0 else bm2 / (st["count"] - 1) / sx) + 4.0 * U * sx
                d = abs(std[i, c] - sx)
                assert d <= lim, (where, "std", std[i, c], sx, d, lim)
                if d > 0.0:
                    share["std"] = max(share["std"], d / lim)
    return share


def peaks_reference(table):
    """table [B, M, nc] -> [B, nc, 4]: min, its node, max, its node over the finite entries of every (vector, column), the first node
    that attains it; NaN and -1 where no node is finite"""
    table = np.asarray(table)
    B, M, nc = table.shape
    out = np.empty((B, nc, 4))
    for b in range(B):
        for c in range(nc):
            v = table[b, :, c]
            idx = np.nonzero(np.isfinite(v))[0]
            if idx.size == 0:
                out[b, c] = (math.nan, -1.0, math.nan, -1.0)
                continue
            w = v[idx]
            out[b, c] = (w.min(), idx[np.argmin(w)], w.max(), idx[np.argmax(w)])
    return out


def welford_merge(v, block=BLOCK):
    """the stated order restated in Python floats (no fma: one rounding more per step, inside the bound) -> the eight fields"""
    n, mean, m2, lo, hi, alo, ahi, fnf = 0, 0.0, 0.0, 0.0, 0.0, -1, -1, -1
    for b0 in range(0, len(v), block):
        nb, mb, sb, lob, hib, alob, ahib = 0, 0.0, 0.0, 0.0, 0.0, -1, -1
        for b in range(b0, min(b0 + block, len(v))):
            x = float(v[b])
            if not math.isfinite(x):
                if fnf < 0:
                    fnf = b
                continue
            nb += 1
            d = x - mb
            mb = mb + d / nb
            sb = sb + d * (x - mb)
            if alob < 0 or x < lob:
                lob, alob = x, b
            if ahib < 0 or x > hib:
                hib, ahib = x, b
        if nb == 0:
            continue
        if n == 0:
            n, mean, m2, lo, hi, alo, ahi = nb, mb, sb, lob, hib, alob, ahib
            continue
        nt, d = n + nb, mb - mean
        mean = mean + d * (nb / nt)
        m2 = (m2 + sb) + (d * d) * ((n * nb) / nt)
        n = nt
        if lob < lo:
            lo, alo = lob, alob
        if hib > hi:
            hi, ahi = hib, ahib
    if n == 0:
        return np.array([0.0, math.nan, math.nan, math.nan, math.nan, -1.0, -1.0, float(fnf)])
    return np.array([float(n), mean, m2, lo, hi, float(alo), float(ahi), float(fnf)])


def fma(a, b, c):
    """a b + c with ONE rounding (finite arguments): the exact value in fractions.Fraction, rounded to nearest even by float()"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def welford_merge_exact(v, block=BLOCK, contract_merge=False):
    """the stated order EXACTLY as the header writes it -- welford_merge with m2 = fma(d, v - mean, m2) in one rounding, every
    other written operation one rounding as Python floats give it -> the eight fields, which the device must give bit for bit.
    contract_merge: a WRONG variant for the teeth, a merge that a compiler has contracted: "mean" Chan's mean + d (nb / nt) as one
    fma(d, nb / nt, mean) (True means this one); "m2" the merged m2 as fma(d d, (n nb) / nt, m2 + m2_b).  The first shows only where
    the block means differ by about as much as they are (the product's lost bits lie log2 |mean / d| places below the sum's last
    bit); the second wherever the spread between the blocks is comparable with the spread inside them."""
    assert contract_merge in (False, True, "mean", "m2")
    n, mean, m2, lo, hi, alo, ahi, fnf = 0, 0.0, 0.0, 0.0, 0.0, -1, -1, -1
    for b0 in range(0, len(v), block):
        nb, mb, sb, lob, hib, alob, ahib = 0, 0.0, 0.0, 0.0, 0.0, -1, -1
        for b in range(b0, min(b0 + block, len(v))):
            x = float(v[b])
            if not math.isfinite(x):
                if fnf < 0:
                    fnf = b
                continue
            nb += 1
            d = x - mb
            mb = mb + d / nb
            sb = fma(d, x - mb, sb)
            if alob < 0 or x < lob:
                lob, alob = x, b
            if ahib < 0 or x > hib:
                hib, ahib = x, b
        if nb == 0:
            continue
        if n == 0:
            n, mean, m2, lo, hi, alo, ahi = nb, mb, sb, lob, hib, alob, ahib
            continue
        nt, d = n + nb, mb - mean
        mean = fma(d, nb / nt, mean) if contract_merge in (True, "mean") else mean + d * (nb / nt)
        m2 = fma(d * d, (n * nb) / nt, m2 + sb) if contract_merge == "m2" else (m2 + sb) + (d * d) * ((n * nb) / nt)
        n = nt
        if lob < lo:
            lo, alo = lob, alob
        if hib > hi:
            hi, ahi = hib, ahib
    if n == 0:
        return np.array([0.0, math.nan, math.nan, math.nan, math.nan, -1.0, -1.0, float(fnf)])
    return np.array([float(n), mean, m2, lo, hi, float(alo), float(ahi), float(fnf)])


def envelope_of(table, fn=welford_merge):
    """[B, M, nc] -> [M, nc, 8] by fn on every (node, column)"""
    B, M, nc = table.shape
    return np.array([[fn(table[:, i, c]) for c in range(nc)] for i in range(M)])


# ---- the batches of the tests: vector 0 plus copies whose positions and velocities are scaled by 1 + 1e-9 b (quaternions untouched)
def batch_of(x, M, B):
    X = np.tile(x, (B, 1)) * (1.0 + 1e-9 * np.arange(B))[:, None]
    X[:, 7 * M:11 * M] = x[7 * M:11 * M]
    X[:, 11 * M:] = x[11 * M:]                # the controls and knot times too
    X[:, :M] = x[:M]                          # and the masses
    return X


def nan_node(X, b, i, M):
    """node i of vector b (None: of every vector) set to NaN, as tests/test_output_atlas.py does"""
    rows = slice(None) if b is None else b
    for lo, w in ((0, 1), (M, 3), (4 * M, 3), (7 * M, 4)):
        X[rows, lo + w * i:lo + w * i + w] = np.nan
    return X

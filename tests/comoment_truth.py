"""What gel_batch_comoments is checked against (tests/test_batch_comoments_cpu.py, tests/test_batch_comoments.py): the exactly
rounded co-moment of two columns, the bound the device's C must keep to it, and the stated order restated exactly as the header
writes it (comoments_exact: what the device gives bit for bit), with wrong variants for the teeth.  numpy, Python integers and
fractions only, no GPU.

The order (include/gelato_amd.h).  A flight counts iff every entry read of it, in both views, is finite (listwise).  Blocks of
BLOCK = 256 consecutive vectors; inside a block, over the counted flights in ascending r, n, m, s, C starting at 0:
    n += 1
    da_i = a_i - ma_i;  ma_i = ma_i + da_i / n;  ea_i = a_i - ma_i;  sa_i = fma(da_i, ea_i, sa_i)        (b likewise)
    C_ij = fma(da_i, eb_j, C_ij)
and the blocks that hold a counted flight merged in ascending order into a running total (the first is copied), every d from the
means before the merge's own mean update:
    nt = n + nb;  da_i = ma_b,i - ma_i;  db_j = mb_b,j - mb_j;  w = (n nb) / nt
    C_ij = (C_ij + Cb_ij) + (da_i db_j) w;   sa_i = (sa_i + sab_i) + (da_i da_i) w;   ma_i = ma_i + da_i (nb / nt);   n = nt

The bound of C, derived for that order the way tests/output_batch_truth.py derives m2's.  Notation: n = counted flights, K = blocks
of the batch, nb = min(n, 256), u = 2^-53, |a|_2 the 2-norm of a column's counted entries, Sa / Sb the exact m2 of the two columns,
hats the computed values, first order in u; the factor 1 / (1 - 4 (n + K + 8) u) at the end absorbs the products of roundings.
  Means.  Every intermediate mean of column x, block or running total, errs by at most (output_batch_truth, mean_bound)
      Ex = u (sqrt(n) |x|_2 + 3 sqrt(Sx) + 7 (K - 1) |x|_2),   inside one block  u (sqrt(nb) |x_b|_2 + 3 sqrt(Sx_b)).
  C inside a block.  C_k^ = fma(da_k^, eb_k^, C_{k-1}^): da_k^ is a rounded difference of a_k and an erring mean (error at most
  |e^a_{k-1}| + u |da_k|), eb_k^ likewise (|e^b_k| + u |eb_k|), and the fma rounds once, by at most u |C_k|.  A partial co-moment is a
  co-moment of a subset, so Cauchy-Schwarz gives |C_k| <= sqrt(Sa_b Sb_b).  The step's error is therefore at most
      |eb_k| Ea_b + |da_k| Eb_b + 2 u |da_k eb_k| + u sqrt(Sa_b Sb_b).
  Summed over the nb steps: sum_k da_k^2 <= 2 Sa_b (m2's derivation: d2_k = d_k (k - 1) / k and sum d_k d2_k = S), and
  |eb_k| <= |db_k|, so sum |da_k| <= sqrt(2 nb Sa_b), sum |eb_k| <= sqrt(2 nb Sb_b), sum |da_k eb_k| <= 2 sqrt(Sa_b Sb_b):
      u ((nb + 4) sqrt(Sa_b Sb_b)) + Ea_b sqrt(2 nb Sb_b) + Eb_b sqrt(2 nb Sa_b)
    = u ((nb + 4 + 6 sqrt(2 nb)) sqrt(Sa_b Sb_b) + sqrt(2) nb (|a_b|_2 sqrt(Sb_b) + |b_b|_2 sqrt(Sa_b))).
  Over the blocks, Cauchy-Schwarz once more (sum_b sqrt(Sa_b Sb_b) <= sqrt(Sa Sb), sum_b |a_b|_2 sqrt(Sb_b) <= |a|_2 sqrt(Sb)):
      u ((nb + 4 + 6 sqrt(2 nb)) sqrt(Sa Sb) + sqrt(2) nb (|a|_2 sqrt(Sb) + |b|_2 sqrt(Sa)))
  C across the merges.  A merge adds (da db) w, w = n nb / nt <= nb, with da, db from two erring means each (errors <= 2 Ea, 2 Eb),
  five roundings on the product's way (da, db, da db, the quotient of w, the product with w; n nb is an integer below 2^53) and two
  on the sums, whose operands are co-moments of subsets, at most sqrt(Sa Sb):
      (2 Ea |db| + 2 Eb |da|) w + 5 u |da db| w + 2 u sqrt(Sa Sb).
  The exact da^2 w of the K - 1 merges sum to at most Sa and sum w <= n, so sum |da| w <= sqrt(n Sa), sum |da db| w <= sqrt(Sa Sb):
      (K > 1)  2 Ea sqrt(n Sb) + 2 Eb sqrt(n Sa) + (5 + 2 (K - 1)) u sqrt(Sa Sb)
  comoment_bound is the sum of the two displays times the factor: m2's bound with sqrt(Sa Sb) where that has m2 and
  |a|_2 sqrt(Sb) + |b|_2 sqrt(Sa) where that has 2 |v|_2 sqrt(m2).  The textbook sum a b - n mean_a mean_b errs by about
  n u |a|_2 |b|_2 = (|a|_2 |b|_2 / sqrt(Sa Sb)) times the first term: where |v|_2 / sqrt(m2) >= 1e6 in both columns it cannot pass.
"""
import math
from fractions import Fraction

import numpy as np

BLOCK = 256
U = 2.0 ** -53


def fma(a, b, c):
    """a b + c with ONE rounding (finite arguments): the exact value in Python integers, rounded to nearest even by int -> float;
    through fractions.Fraction where the integer would leave the range of a double or the result the normal range"""
    if a == 0.0 or b == 0.0:
        return a * b + c
    ma, ea = math.frexp(a)
    mb, eb = math.frexp(b)
    p, ep = int(math.ldexp(ma, 53)) * int(math.ldexp(mb, 53)), ea + eb - 106
    if c == 0.0:
        N, e = p, ep
    else:
        mc, ec = math.frexp(c)
        ic, ec = int(math.ldexp(mc, 53)), ec - 53
        e = min(ep, ec)
        if max(ep, ec) - e > 900:
            return float(Fraction(a) * Fraction(b) + Fraction(c))
        N = (p << (ep - e)) + (ic << (ec - e))
    if N == 0:
        return 0.0
    if N.bit_length() + e > 1020 or N.bit_length() + e < -960:
        return float(Fraction(a) * Fraction(b) + Fraction(c))
    return math.ldexp(float(N), e) if N.bit_length() <= 1000 else float(Fraction(N) * Fraction(2) ** e)


def _ints(w):
    """finite float64 [n] -> (Python integers, exponent): w[k] = ints[k] 2^exponent exactly"""
    m, e = np.frexp(w)
    mi = np.ldexp(m, 53).astype(np.int64).tolist()
    e = e.astype(np.int64) - 53
    emin = int(e.min())
    return [a << s for a, s in zip(mi, (e - emin).tolist())], emin


def counted_rows(A, Bv=None):
    """the listwise rule: bool [B], True where every entry of the flight's rows of A (and Bv) is finite"""
    ok = np.isfinite(np.asarray(A)).all(axis=1)
    if Bv is not None:
        ok &= np.isfinite(np.asarray(Bv)).all(axis=1)
    return ok


def exact_comoment(a, b):
    """two columns over the SAME counted flights (finite entries only) -> dict: C = sum a b - sum a sum b / n exactly in integers,
    rounded once ("C"), as a Fraction ("C_exact"), and what the bound needs: the exact m2 of either column rounded (Sa, Sb) and
    the 2-norms (la, lb)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n = int(a.size)
    assert b.size == n and np.isfinite(a).all() and np.isfinite(b).all()
    if n == 0:
        return {"n": 0, "C": math.nan, "C_exact": Fraction(0), "Sa": 0.0, "Sb": 0.0, "la": 0.0, "lb": 0.0}
    ia, ea = _ints(a)
    ib, eb = _ints(b)
    sa, sb = Fraction(2) ** ea, Fraction(2) ** eb
    Sa_, Sb_ = sum(ia), sum(ib)
    P, Qa, Qb = sum(x * y for x, y in zip(ia, ib)), sum(x * x for x in ia), sum(y * y for y in ib)
    Cx = Fraction(n * P - Sa_ * Sb_, n) * sa * sb
    m2a, m2b = Fraction(n * Qa - Sa_ * Sa_, n) * sa * sa, Fraction(n * Qb - Sb_ * Sb_, n) * sb * sb
    return {"n": n, "C": float(Cx), "C_exact": Cx, "Sa": float(m2a), "Sb": float(m2b),
            "la": math.sqrt(float(Fraction(Qa) * sa * sa)), "lb": math.sqrt(float(Fraction(Qb) * sb * sb))}


def comoment_bound(st, B):
    """the bound of the module docstring for one pair's exact statistics (exact_comoment) and the batch size"""
    n = st["n"]
    if n == 0:
        return 0.0
    K = (B + BLOCK - 1) // BLOCK
    nb = min(n, BLOCK)
    ra, rb, la, lb = math.sqrt(st["Sa"]), math.sqrt(st["Sb"]), st["la"], st["lb"]
    bound = U * ((nb + 4 + 6.0 * math.sqrt(2.0 * nb)) * ra * rb + math.sqrt(2.0) * nb * (la * rb + lb * ra))
    if K > 1:
        Ea = U * (math.sqrt(n) * la + 3.0 * ra + 7.0 * (K - 1) * la)
        Eb = U * (math.sqrt(n) * lb + 3.0 * rb + 7.0 * (K - 1) * lb)
        bound += 2.0 * Ea * math.sqrt(n) * rb + 2.0 * Eb * math.sqrt(n) * ra + (5 + 2 * (K - 1)) * U * ra * rb
    return bound / (1.0 - 4.0 * (n + K + 8) * U)


WRONG = (None, "eb_old_mean", "merge_fma", "pairwise", "merge_mean_first")


def comoments_exact(A, Bv=None, self_form=None, block=BLOCK, wrong=None):
    """the stated order EXACTLY as the header writes it, the fma in one rounding, every other written operation one rounding as
    Python floats give it.  A [B, Wa], Bv [B, Wb] or None (the self form: only i <= j formed, the lower triangle a copy).
    -> {"count", "first_excluded", "C" [Wa, Wb], "stat_a" [Wa, 2], "stat_b" [Wb, 2] (self form: stat_a)}
    wrong: a WRONG variant for the teeth --
      "eb_old_mean"       eb_j taken with the mean before the step's update (db_j in its place)
      "merge_fma"         the merge's (da db) w contracted with the sum: fma(da db, w, C + Cb)
      "pairwise"          a pair counts the flights whose entries in ITS two columns are finite, not the listwise set
      "merge_mean_first"  the merge's means updated before da, db are formed"""
    assert wrong in WRONG
    A = np.asarray(A, dtype=np.float64)
    if self_form is None:
        self_form = Bv is None
    Bm = A if self_form else np.asarray(Bv, dtype=np.float64)
    nB, Wa = A.shape
    Wb = Bm.shape[1]
    ok = counted_rows(A, None if self_form else Bm)
    if wrong == "pairwise":
        C = np.empty((Wa, Wb))
        for i in range(Wa):
            for j in range(Wb):
                r = comoments_exact(A[:, i:i + 1], Bm[:, j:j + 1], self_form=False, block=block)
                C[i, j] = r["C"][0, 0]
        base = comoments_exact(A, Bv, self_form, block)
        base["C"] = C
        return base
    bad = np.nonzero(~ok)[0]
    first_excluded = int(bad[0]) if bad.size else -1
    n = 0
    ma, sa, mb, sb = [0.0] * Wa, [0.0] * Wa, [0.0] * Wb, [0.0] * Wb
    C = [[0.0] * Wb for _ in range(Wa)]
    rowsA, rowsB = A.tolist(), Bm.tolist()
    for r0 in range(0, nB, block):
        nb = 0
        mab, sab, mbb, sbb = [0.0] * Wa, [0.0] * Wa, [0.0] * Wb, [0.0] * Wb
        Cb = [[0.0] * Wb for _ in range(Wa)]
        for r in range(r0, min(r0 + block, nB)):
            if not ok[r]:
                continue
            nb += 1
            ra, rb = rowsA[r], rowsB[r]
            da, eb = [0.0] * Wa, [0.0] * Wb
            for i in range(Wa):
                d = ra[i] - mab[i]
                mab[i] = mab[i] + d / nb
                sab[i] = fma(d, ra[i] - mab[i], sab[i])
                da[i] = d
            for j in range(Wb):
                d = rb[j] - mbb[j]
                mbb[j] = mbb[j] + d / nb
                e = rb[j] - mbb[j]
                sbb[j] = fma(d, e, sbb[j])
                eb[j] = d if wrong == "eb_old_mean" else e
            for i in range(Wa):
                Ci, d = Cb[i], da[i]
                for j in range(i if self_form else 0, Wb):
                    Ci[j] = fma(d, eb[j], Ci[j])
        if nb == 0:
            continue
        if n == 0:
            n, ma, sa, mb, sb, C = nb, mab, sab, mbb, sbb, Cb
            continue
        nt = n + nb
        w, fb = (n * nb) / nt, nb / nt
        if wrong == "merge_mean_first":
            ma_new = [ma[i] + (mab[i] - ma[i]) * fb for i in range(Wa)]
            mb_new = [mb[j] + (mbb[j] - mb[j]) * fb for j in range(Wb)]
            da = [mab[i] - ma_new[i] for i in range(Wa)]
            db = [mbb[j] - mb_new[j] for j in range(Wb)]
        else:
            da = [mab[i] - ma[i] for i in range(Wa)]
            db = [mbb[j] - mb[j] for j in range(Wb)]
        for i in range(Wa):
            for j in range(i if self_form else 0, Wb):
                if wrong == "merge_fma":
                    C[i][j] = fma(da[i] * db[j], w, C[i][j] + Cb[i][j])
                else:
                    C[i][j] = (C[i][j] + Cb[i][j]) + (da[i] * db[j]) * w
        for i in range(Wa):
            sa[i] = (sa[i] + sab[i]) + (da[i] * da[i]) * w
        for j in range(Wb):
            sb[j] = (sb[j] + sbb[j]) + (db[j] * db[j]) * w
        if wrong == "merge_mean_first":
            ma, mb = ma_new, mb_new
        else:
            ma = [ma[i] + da[i] * fb for i in range(Wa)]
            mb = [mb[j] + db[j] * fb for j in range(Wb)]
        n = nt
    if n == 0:
        return {"count": 0, "first_excluded": first_excluded, "C": np.full((Wa, Wb), np.nan), "stat_a": np.full((Wa, 2), np.nan),
                "stat_b": np.full((Wb, 2), np.nan)}
    Cn = np.array(C, dtype=np.float64).reshape(Wa, Wb)
    if self_form:
        iu = np.triu_indices(Wa, 1)
        Cn[(iu[1], iu[0])] = Cn[iu]
    stat_a = np.array([ma, sa]).T.reshape(Wa, 2)
    stat_b = stat_a if self_form else np.array([mb, sb]).T.reshape(Wb, 2)
    return {"count": n, "first_excluded": first_excluded, "C": Cn, "stat_a": stat_a, "stat_b": stat_b}


def textbook(a, b):
    """sum a b - n mean_a mean_b in plain fp64: what the bound must refuse where the columns' means dwarf their spread"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n = a.size
    return float(np.dot(a, b) - n * (a.sum() / n) * (b.sum() / n))


def check_C(A, Bv, C, B=None):
    """C [Wa, Wb] of the listwise-counted rows of A and Bv (None: A) against exact_comoment within comoment_bound (plus half an ulp
    of the reference itself) -> the largest share of the bound used"""
    A = np.asarray(A)
    Bm = A if Bv is None else np.asarray(Bv)
    ok = counted_rows(A, Bv)
    nB = A.shape[0] if B is None else B
    share = 0.0
    for i in range(A.shape[1]):
        for j in range(Bm.shape[1]):
            st = exact_comoment(A[ok, i], Bm[ok, j])
            lim = comoment_bound(st, nB) + U * abs(st["C"])
            d = abs(C[i, j] - st["C"])
            assert d <= lim, (i, j, C[i, j], st["C"], d, lim)
            if d > 0.0:
                share = max(share, d / lim)
    return share

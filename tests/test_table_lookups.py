"""The table lookups themselves (gel_physics.h lower_count / interp_tab / wind_ned2 and their kept-interval forms, through
gel_point_eval kinds 5, 6, 9, 10) against exact arithmetic, over the tables of tests/table_cases.py: two rows, the last size of the
counting branch and the first of the bisection, and 160 wind rows (point_kernel stages the rows and their slopes, 798 doubles, in
thirteen passes of its 64 threads; the 48 CA rows, 143 doubles, in three).

The truth and the bound are table_cases.lookup_truth / lookup_bound (derived there, not fitted).

Which interval serves x == xp[k]: both neighbours give yp[k] to rounding, so the bound cannot tell, but the BITS can.  The interval
that starts at the knot returns yp[k] itself (yp[k] + 0 slope); the one that ends there returns yl + (xp[k] - xl) slope, which at
some knots rounds to a neighbour of yp[k] (table_cases.knot_values: with and without contraction).  The device's value at every
interior knot must be one of the latter, and at the knots where yp[k] is not among them that rules out `<=` for `<` in
lower_count: 6 wind knots of EDGE32 (the counting branch), 4 of EDGE33 and 19 of LONG (the bisection), counted on the CPU as well.
At the other knots, and at every knot of the CA tables (their increments are small beside the values: the expression lands on
yp[k] exactly), the two intervals give the same bits and nothing tells them apart.
NOT tested on the device: the same choice in the exact kernels' slope[idx] (gel_exact.h interp_tab_slope, the wind slopes of
gel_rhs_parts.h).  It shows only at a node whose altitude or Mach number IS a knot in the device's arithmetic; both are rounded
functions of the position and no state of the suite has one: g28's `knots` nodes are 4 mm and 4 cm off their knots, which pins the
interval on either side of a knot, not at it, and the fixture has no `kink` entry (tests/golden/make_long_tables.py asserts
that)."""
import numpy as np
import pytest

import table_cases as TC

CASES = list(TC.CASES)
# interior knots (both wind columns; the CA tables have none) at which the lookup's bits tell the interval that ends at the knot from
# the one that starts there (table_cases.knot_values)
DECIDING_KNOTS = {"MIN": 0, "EDGE32": 6, "EDGE33": 4, "LONG": 19, "LONGEVEN": 19}
WRONG = {"count <= for <": dict(count="<="), "no clamp to K - 2": dict(clamp_top=False), "next interval's slope": dict(slope_of=1),
         "previous interval's slope": dict(slope_of=-1)}


def _tables(case):
    wind, ca = TC.CASES[case]
    return (("ca", ca, 1), ("wind", wind, 2))


@pytest.mark.parametrize("case", CASES)
def test_truth_is_np_interp_and_the_oracles_interp(case):
    """the Fraction restatement against np.interp (which computes yl + slope (x - xl): a few ulp of the increment) and the oracle's
    interp (the reference's own expression), on every abscissa the device test uses; the fp64 model of the device's expression
    stays inside the derived bound; the budgets and check_tables hold for the case"""
    import oracle
    decided = 0
    for name, t, ncol in _tables(case):
        xp = t[:, 0]
        xs = TC.abscissae(xp, seed=len(xp), nrand=600)
        for c in range(1, ncol + 1):
            yp = t[:, c]
            scale = np.abs(yp).max()
            for x in xs:
                v, piece = TC.lookup_truth(x, xp, yp)
                assert abs(float(v) - np.interp(x, xp, yp)) <= 8 * TC.U * 2 * scale, (case, name, x)
                if np.isfinite(x) and x != xp[0]:                  # x == xp[0]: the reference reads before its table (appendix C-3)
                    assert abs(float(v) - oracle.interp(x, xp, yp)) <= 8 * TC.U * 2 * scale, (case, name, x)
                if piece >= 0 and x == xp[piece + 1]:
                    assert v == TC.Fraction(float(yp[piece + 1]))  # a knot, from the interval that ends there: the entry itself
            if len(xp) > 2:                                        # the knots' bits: which of them decide the side, and catch `<=` for `<`
                inner = xp[1:-1]
                n = TC.check_knot_sides([TC.device_model(x, xp, yp)[0] for x in inner], xp, yp)
                decided += n
                if n:
                    with pytest.raises(AssertionError):
                        TC.check_knot_sides([TC.device_model(x, xp, yp, count="<=")[0] for x in inner], xp, yp)
            model = [TC.device_model(x, xp, yp)[0] for x in xs]
            worst, exact = TC.check_lookups(model, xs, xp, yp, "%s %s model" % (case, name))
            assert worst <= 1.0 and exact >= 4
    assert decided == DECIDING_KNOTS[case]
    lim = TC.check_case(case)
    assert lim["table"] == TC.staged_doubles(case)
    if case == "LONG":
        assert lim["table"] == 1029 and lim["table"] % 2 == 1 and TC.staged_doubles("LONGEVEN") % 2 == 0
        assert -(-lim["table"] // 512) >= 3 and -(-lim["table"] // 256) >= 5 and -(-lim["table"] // 64) >= 17


@pytest.mark.parametrize("case", CASES)
def test_truth_rejects_wrong_lookups(case):
    """the truth's teeth, shown on the device's own formulation with checked table reads (table_cases.device_model): each wrong
    lookup is told from the right one on at least one abscissa of the case.  A table of two rows has one interval and no interior
    knot: `<=` for `<` in the count selects no other interval anywhere (that is what the clamp to K - 2 = 0 is for), so that one
    has nothing to be seen by there -- asserted as such."""
    for name, t, ncol in _tables(case):
        xp, yp = t[:, 0], t[:, 1]
        xs = [x for x in TC.abscissae(xp, seed=len(xp), nrand=300)]
        assert not any(TC.rejects(x, xp, yp) for x in xs), "the right lookup is rejected"
        for what, wrong in WRONG.items():
            caught = sum(TC.rejects(x, xp, yp, **wrong) for x in xs)
            if len(xp) == 2 and what == "count <= for <":
                assert caught == 0
            else:
                assert caught >= 1, (case, name, what)


def _fresh(kind, xs, t):
    from gelato_amd.dynamics import point_eval
    return point_eval(kind, xs, aux=t)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_device_lookups_against_exact_arithmetic(case):
    """kinds 6 (interp_tab) and 5 (wind_ned2) on every knot, its neighbours, every midpoint, both ends, +-inf and 3000 seeded
    points, shuffled over the lanes: the table entry bit for bit where the value is a select, within 8 u (|yl| + |yu|) elsewhere;
    kinds 9 and 10 (the kept interval) give the bits of 6 and 5 on the shared sequences"""
    wind, ca = TC.CASES[case]
    xs = TC.abscissae(ca[:, 0], seed=len(ca))
    got = _fresh(6, xs, ca).ravel()
    worst, exact = TC.check_lookups(got, xs, ca[:, 0], ca[:, 1], case + " CA")
    print("%s CA: worst use of the bound %.3f, %d bit-exact points of %d" % (case, worst, exact, len(xs)))
    assert exact >= 6
    xs = TC.abscissae(wind[:, 0], seed=len(wind))
    got = _fresh(5, xs, wind)
    assert np.all(got[:, 2] == 0.0)
    for c in (1, 2):
        worst, exact = TC.check_lookups(got[:, c - 1], xs, wind[:, 0], wind[:, c], "%s wind column %d" % (case, c))
        print("%s wind %d: worst use of the bound %.3f, %d bit-exact points of %d" % (case, c, worst, exact, len(xs)))
        assert exact >= 6
    # x == xp[k]: served by the interval that ends there, seen in the bits
    decided = 0
    for t, kind, cols in ((ca, 6, 1), (wind, 5, 2)):
        if len(t) > 2:
            got = _fresh(kind, t[1:-1, 0], t)
            for c in range(1, cols + 1):
                decided += TC.check_knot_sides(got[:, c - 1], t[:, 0], t[:, c], "%s kind %d column %d" % (case, kind, c))
    assert decided == DECIDING_KNOTS[case]
    rng = np.random.default_rng(99)
    n = 64 * 12 + 17
    for kind_c, kind_f, t in ((9, 6, ca), (10, 5, wind)):
        seq = TC.kept_interval_sequences(rng, t, n)
        kept, _fresh_bits = TC.check_kept_equal_fresh(t, kind_c, kind_f, seq)
        # and the kept-interval values themselves against the truth (first component)
        flat = seq.ravel()
        vals = kept.ravel() if kind_c == 9 else kept.reshape(n, 8, 2)[:, :, 0].ravel()
        TC.check_lookups(vals, flat, t[:, 0], t[:, 1], "%s kind %d" % (case, kind_c))

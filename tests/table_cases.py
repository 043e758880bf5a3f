"""Wind and CA tables beyond the example's handful of rows, and the exact truth of a lookup in them (tests/test_table_lookups.py,
tests/test_table_sizes.py, tests/golden/make_long_tables.py).  Importing this module needs neither a GPU nor torch.

The cases (CASES[name] -> (wind [Kw][3], ca [Kc][2]), deterministic):
  MIN        Kw = 2, Kc = 2       one interval per table: every lookup is clamped to interval 0 (n - 2 = 0)
  EDGE32     Kw = Kc = 32         the last size lower_count() counts over the rows
  EDGE33     Kw = Kc = 33         the first size it searches by bisection -- same generating functions as EDGE32
  LONG       Kw = 160, Kc = 48    T = 1029 staged doubles (odd: the regions behind the tables start one double further on):
                                  three staging passes of a 512-thread workgroup, five of 256 threads, seventeen of 64
  LONGEVEN   Kw = 160, Kc = 49    T = 1032, the other parity
Wind rows from 300 m to 95 km with spacings from metres to kilometres (nodes lie below, inside and above the table), values a
smooth function plus seeded noise, of both signs; Mach rows from 0 to 8, denser around Mach 1.

The truth (lookup_truth) is the reference's rule -- src/wrapper_utils.hpp:51-80 with np.interp's value at x == xp[0] (SURVEY.md
appendix C-3) -- in fractions.Fraction on the fp64 table entries and the fp64 abscissa: exact, no tolerance of its own.

The bound a device lookup is held to, |got - truth| <= 8 u (|yl| + |yu|), u = 2^-53, follows from the expression
(gel_physics.h interp_tab / wind_ned2: yl + (x - xl) * slope[idx], slope tabulated by the host as (yu - yl) / (xu - xl)):
  host    slope = fl(fl(yu - yl) / fl(xu - xl)): three roundings, slope = (D / H)(1 + e)^3 with D = yu - yl, H = xu - xl;
  device  h = fl(x - xl), p = fl(h slope), v = fl(yl + p): three roundings, two when the product and the sum contract to
          one fused multiply-add.
With 0 < x - xl <= H the increment p is (x - xl) D / H (1 + e)^5, at most 5 u / (1 - 5 u) |D| <= 5.01 u (|yl| + |yu|) away from
the exact increment; the last rounding adds u |v| with |v| <= max(|yl|, |yu|) (1 + 6 u): below 6.1 u (|yl| + |yu|) in all, and
8 u covers it with or without contraction.  Where the value is a select of a table entry (x <= xp[0], x > xp[K-1]) it is that
entry, bit for bit; NaN gives NaN (every comparison false, the arithmetic value is NaN)."""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
BOUND_U = 8


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def _wind_table(K, seed):
    rng = np.random.default_rng(seed)
    gaps = 10.0 ** rng.uniform(0.5, 3.7, K - 1)                  # 3 m .. 5 km, log-uniform
    big = gaps >= 500.0                                          # the short gaps stay as drawn, the long ones fill the span
    gaps[big] *= (95000.0 - 300.0 - gaps[~big].sum()) / gaps[big].sum()
    h = 300.0 + np.concatenate([[0.0], np.cumsum(gaps)])
    h[0], h[-1] = 300.0, 95000.0
    assert np.all(np.diff(h) > 0.5)
    wn = 30.0 * np.sin(h / 9000.0) + 8.0 * rng.standard_normal(K)
    we = -20.0 * np.cos(h / 14000.0) + 6.0 * rng.standard_normal(K)
    return np.column_stack([h, wn, we])


def _ca_table(K, seed):
    rng = np.random.default_rng(seed)
    m = 8.0 * (np.arange(K) / (K - 1.0)) ** 1.7
    m[1:-1] *= 1.0 + 0.2 / K * rng.uniform(-1.0, 1.0, K - 2)     # off the grid, still increasing
    m[0], m[-1] = 0.0, 8.0
    assert np.all(np.diff(m) > 1e-4)
    ca = 0.3 + 0.25 * np.exp(-((m - 1.1) / 0.35) ** 2) + 0.02 * rng.standard_normal(K)
    return np.column_stack([m, ca])


def _generated(Kw, Kc):
    return _wind_table(Kw, 1976), _ca_table(Kc, 51)


CASES = {
    "MIN": (np.array([[0.0, 12.5, -7.25], [60000.0, -31.0, 22.5]]), np.array([[0.0, 0.35], [6.0, 0.22]])),
    "EDGE32": _generated(32, 32),
    "EDGE33": _generated(33, 33),
    "LONG": _generated(160, 48),
    "LONGEVEN": _generated(160, 49),
}
MESHES = {"pack": (20, 31, 2), "coop": (40, 65, 2), "slab": (70, 5, 2)}      # tests/states.py table_state(); the tail has no aerodynamics


# Every kernel that stages the tables into LDS -> the tests that run it over CASES ("file::test", parametrisation left off).
# tests/test_table_sizes_cpu.py finds the kernels in gelato_amd/csrc and fails where one has no entry here or a named test is gone.
# PER_INSTANTIATION: kernels keyed per value of their bool template parameters (each instantiation has a table-staging path of its own)
PER_INSTANTIATION = {"prop_kernel": ("kDisp", "kChain")}
_SIZES, _FLIGHT, _OUTBATCH = "test_table_sizes.py::", "test_table_sizes_flight.py::", "test_table_sizes_outbatch.py::"
TABLE_KERNELS = {
    "eval_kernel": [_SIZES + "test_defect_groups_against_the_oracle_in_every_form"],
    "callback_kernel": [_SIZES + "test_defect_groups_against_the_oracle_in_every_form", _SIZES + "test_aero_kinds_dense_records_and_callback"],
    "aero_kernel": [_SIZES + "test_aero_kinds_dense_records_and_callback"],
    "aero_sm_kernel": [_SIZES + "test_aero_kinds_dense_records_and_callback"],
    "aero_wide_kernel": [_SIZES + "test_aero_kinds_dense_records_and_callback"],
    "rhs_vel_air_kernel": [_SIZES + "test_velocity_rhs_of_every_phase"],
    "mesh_kernel": [_SIZES + "test_mesh_error_and_propagation"],
    "output_kernel": [_SIZES + "test_output_table"],
    "prop_kernel<false,false>": [_SIZES + "test_mesh_error_and_propagation"],
    "prop_kernel<true,false>": [_FLIGHT + "test_dispersed_node_restart_on_the_table_states", _FLIGHT + "test_bits_of_a_vector_in_a_mixed_batch"],
    "prop_kernel<false,true>": [_FLIGHT + "test_chain_of_the_example_over_the_tables"],
    "prop_kernel<true,true>": [_FLIGHT + "test_chain_of_the_example_over_the_tables"],
    "outbatch_rows_kernel": [_OUTBATCH + "test_table_bits_against_the_single_vector_call", _OUTBATCH + "test_envelope_and_peaks_two_blocks",
                             _OUTBATCH + "test_dispersed_wind_bits_and_values"],
    "outbatch_env_kernel": [_OUTBATCH + "test_envelope_and_peaks_two_blocks"],
    # the exact kernels: LONG alone, in their own suites (exact arithmetic as the truth)
    "exact_jac_kernel": ["test_exact_jac.py::test_exact_against_the_ground_truth_over_long_tables"],
    "exact_aero_kernel": ["test_exact_aero_jac.py::test_exact_against_the_ground_truth_over_long_tables"],
}


def with_tables(prob, case):
    """a copy of prob over the case's tables"""
    prob = dict(prob)
    wind, ca = CASES[case]
    prob["wind_table"], prob["ca_table"] = wind.copy(), ca.copy()
    return prob


def staged_doubles(case):
    wind, ca = CASES[case]
    return 85 + 5 * len(wind) + 3 * len(ca)


def check_case(case, meshes=tuple(MESHES.values())):
    """the case's shape, its place against every launch's LDS budget (asked of the library: gel_table_limits reports what the
    launchers' own expressions leave) and check_tables (a host-only handle takes the tables) -> the limits of the first mesh's
    first phase"""
    from gelato_amd import Engine, _lib
    import states
    wind, ca = CASES[case]
    Kw, Kc = len(wind), len(ca)
    for t in (wind, ca):
        assert t.dtype == np.float64 and np.all(np.diff(t[:, 0]) > 0) and np.all(np.isfinite(t))
    if case != "MIN":
        assert wind[0, 0] == 300.0 and wind[-1, 0] == 95000.0 and ca[0, 0] == 0.0 and ca[-1, 0] == 8.0
        assert np.diff(wind[:, 0]).min() < 20.0 and np.diff(wind[:, 0]).max() > 1000.0          # metres to kilometres
        assert (wind[:, 1:] > 0).any(axis=0).all() and (wind[:, 1:] < 0).any(axis=0).all()    # both signs, both components
    first = None
    for nn in meshes:
        for n in nn:
            lim = _lib.table_limits(Kw, Kc, n)
            assert lim["table"] == staged_doubles(case) and lim["cap_bytes"] == 65536
            for launch in ("fused", "aero", "mesh", "plain"):
                assert lim["table"] <= lim[launch], (case, n, launch, lim)
            first = first or lim
        prob, _x = states.table_state(case, nn, "climb")
        Engine(prob, device=-1)                                   # gel_problem_create: check_tables and the launch budgets
    return first


# ---- the truth of one lookup --------------------------------------------------------------------------------------------------
def lookup_truth(x, xp, yp):
    """-> (value as a Fraction, piece): piece -1 where x <= xp[0] (the value is yp[0]), -2 where x > xp[K-1] (yp[K-1]), else the
    interval k with xp[k] < x <= xp[k+1] the value is interpolated in: a knot belongs to the interval that ENDS there.
    x may be +-inf; NaN has no truth."""
    K = len(xp)
    assert x == x
    if x <= xp[0]:
        return Fraction(float(yp[0])), -1
    if x > xp[K - 1]:
        return Fraction(float(yp[K - 1])), -2
    k = int(np.searchsorted(xp, x, side="left")) - 1               # std::lower_bound: the number of entries < x, less one
    assert 0 <= k <= K - 2 and xp[k] < x <= xp[k + 1]
    xl, xu, yl, yu = (Fraction(float(v)) for v in (xp[k], xp[k + 1], yp[k], yp[k + 1]))
    return yl + (Fraction(float(x)) - xl) / (xu - xl) * (yu - yl), k


def lookup_bound(piece, yp):
    """what a device lookup may differ from the truth by (module docstring); 0 where the value is a select of a table entry"""
    if piece < 0:
        return Fraction(0)
    return BOUND_U * Fraction(U) * (abs(Fraction(float(yp[piece]))) + abs(Fraction(float(yp[piece + 1]))))


def check_lookups(got, xs, xp, yp, what=""):
    """got[i] against the truth at xs[i]: bit-equal where the value is a table entry, within lookup_bound elsewhere, NaN for NaN
    -> (worst use of the bound, number of bit-exact points)"""
    worst, exact = 0.0, 0
    for g, x in zip(np.asarray(got, dtype=np.float64), xs):
        if x != x:
            assert g != g, (what, "NaN in, %r out" % g)
            continue
        v, piece = lookup_truth(x, xp, yp)
        if piece < 0:
            assert g == float(v) and np.signbit(g) == np.signbit(float(v)), (what, float(x), g, float(v))
            exact += 1
            continue
        assert g == g, (what, float(x))
        err, bound = abs(Fraction(float(g)) - v), lookup_bound(piece, yp)
        assert err <= bound, (what, float(x), piece, float(g), float(v), float(err / bound) if bound else np.inf)
        if bound:
            worst = max(worst, float(err / bound))
    return worst, exact


# ---- the device's formulation, restated with checked indices: what the truth's teeth are shown on ------------------------------
def device_model(x, xp, yp, count="<", clamp_top=True, slope_of=0):
    """gel_physics.h interp_tab in numpy fp64 (no contraction): the count over the rows, the clamps of the index, the value from
    the tabulated slope, then the selects -> (value, index used).  The wrong lookups of the teeth: count = "<=", clamp_top = False
    (no clamp to K - 2), slope_of = +-1 (the neighbouring interval's slope).  Every table read is checked: IndexError where the
    device would read past its table."""
    K = len(xp)
    slope = (yp[1:] - yp[:-1]) / (xp[1:] - xp[:-1])
    lo = int(np.sum(xp <= x)) if count == "<=" else int(np.sum(xp < x))
    idx = max(lo - 1, 0)
    if clamp_top:
        idx = min(idx, K - 2)

    def at(a, i):
        if not 0 <= i < len(a):
            raise IndexError(i)
        return a[i]
    v = at(yp, idx) + (x - at(xp, idx)) * at(slope, idx + slope_of)
    at(xp, idx + 1)                                                # the interval's upper end exists
    return (yp[0] if x <= xp[0] else (yp[K - 1] if x > xp[K - 1] else v)), idx


def rejects(x, xp, yp, **wrong):
    """does the truth tell the wrong lookup from the right one at x: a read past the table, a value outside the bound, or the
    interval on the other side of a knot"""
    v, piece = lookup_truth(x, xp, yp)
    try:
        g, idx = device_model(x, xp, yp, **wrong)
    except IndexError:
        return True
    if piece >= 0 and idx != piece:
        return True
    return abs(Fraction(float(g)) - v) > lookup_bound(piece, yp)


def knot_values(xp, yp, k):
    """x == xp[k], 1 <= k <= K - 2, in fp64 as the device forms it: -> (the values the interval that ENDS at the knot can give --
    yl + fl(fl(x - xl) slope) with the host's slope, and the same with product and sum contracted to one fused multiply-add --,
    the value the interval that STARTS there gives: yp[k] + 0 slope = yp[k]).  Where yp[k] is not among the former, the bits of a
    lookup tell which interval served the knot."""
    xl, yl = xp[k - 1], yp[k - 1]
    s = (yp[k] - yl) / (xp[k] - xl)
    h = xp[k] - xl
    fused = float(Fraction(float(yl)) + Fraction(float(h)) * Fraction(float(s)))      # float(Fraction) rounds to nearest
    return {float(yl + h * s), fused}, float(yp[k])


def check_knot_sides(got, xp, yp, what=""):
    """got[k - 1] = the lookup at x == xp[k], k = 1 .. K - 2: one of the values of the interval that ends there, bit for bit
    -> the number of knots at which that rules out the interval that starts there"""
    decided = 0
    for k in range(1, len(xp) - 1):
        ends, starts = knot_values(xp, yp, k)
        assert float(got[k - 1]) in ends, (what, k, float(got[k - 1]), sorted(ends), starts)
        decided += starts not in ends
    return decided


# ---- abscissae -------------------------------------------------------------------------------------------------------------------
def abscissae(xp, seed, nrand=3000):
    """every knot, its neighbours one ulp below and above, every interval's midpoint, the table's ends less / plus a little,
    +-inf and nrand seeded points from below the first to above the last knot -- shuffled, so that the lanes of a wavefront mix
    interior points, knots and both clamps (and the bisection of its lanes takes different ways)"""
    rng = np.random.default_rng(seed)
    span = xp[-1] - xp[0]
    little = [xp[0] - 1e-9 * max(abs(xp[0]), 1.0), xp[0] - 0.01 * span, xp[-1] + 1e-9 * max(abs(xp[-1]), 1.0), xp[-1] + 0.01 * span]
    pts = np.concatenate([xp, np.nextafter(xp, -np.inf), np.nextafter(xp, np.inf), 0.5 * (xp[:-1] + xp[1:]), little,
                          [xp[0], xp[-1], -np.inf, np.inf], rng.uniform(xp[0] - 0.05 * span, xp[-1] + 0.05 * span, nrand),
                          xp[rng.integers(0, len(xp), nrand // 4)] + rng.uniform(-1.0, 1.0, nrand // 4) * 1e-7 * span])
    return pts[rng.permutation(len(pts))]


def kept_interval_sequences(rng, t, n):
    """[n][8] abscissae per lane for the kept-interval lookups (gel_point_eval kinds 9 / 10) over table t: just below a breakpoint,
    on it, an ulp above, a forward-difference step above and another, anywhere (also beyond both ends) and 1e-8 beside that; half of
    the lanes stay within 1e-8 of one point (wavefronts with hits AND misses); NaN and +-inf sprinkled in"""
    bp = t[:, 0]
    base = bp[rng.integers(0, len(bp), n)]
    seq = np.empty((n, 8))
    seq[:, 0] = base * (1.0 - 1e-9) - 1e-12                       # just below a breakpoint
    seq[:, 1] = base                                              # on it
    seq[:, 2] = np.nextafter(base, np.inf)                        # an ulp above
    seq[:, 3] = base * (1.0 + 1e-8) + 1e-8                        # a forward-difference step above
    seq[:, 4] = seq[:, 3] + 1e-8 * np.abs(seq[:, 3])              # and another (same interval: the short way)
    seq[:, 5] = rng.uniform(bp[0] - 1.0, min(bp[-1], 3e4) * 1.1, n)   # anywhere, also beyond both ends
    seq[:, 6] = seq[:, 5] * (1.0 + 1e-8)
    seq[:, 7] = seq[:, 6]
    calm = rng.random(n) < 0.5                                    # half of the lanes stay put: wavefronts with hits AND misses
    seq[calm, :] = seq[calm, 5:6] * (1.0 + 1e-9 * np.arange(8)[None, :])
    seq[rng.integers(0, n, 25), rng.integers(0, 8, 25)] = np.nan
    seq[rng.integers(0, n, 25), rng.integers(0, 8, 25)] = np.inf
    seq[rng.integers(0, n, 25), rng.integers(0, 8, 25)] = -np.inf
    return seq


def check_kept_equal_fresh(t, kind_c, kind_f, seq):
    """kinds 9 / 10 through the kept interval give the bits of kinds 6 / 5 called afresh on the same abscissae -> (kept, fresh)"""
    from gelato_amd.dynamics import point_eval
    n = len(seq)
    got = point_eval(kind_c, seq, aux=t)
    fresh = point_eval(kind_f, seq.ravel(), aux=t)
    if kind_f == 5:
        fresh = fresh[:, :2].reshape(n, 16)
    else:
        fresh = fresh.reshape(n, 8)
    assert np.array_equal(got, fresh, equal_nan=True), (kind_c, np.argwhere(~((got == fresh) | (np.isnan(got) & np.isnan(fresh))))[:5])
    assert np.isnan(got).any() and np.isfinite(got).any()
    return got, fresh

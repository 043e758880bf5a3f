"""Helpers of the size-selected-form tests (tests/test_size_forms.py on the GPU, tests/test_size_forms_cpu.py anywhere; DESIGN.md
3.12): the block-wise bit checker with its teeth, and the choice of a batch size past a threshold.

Method (test_full_size_batches_size_independent_properties): a batch tiles P = 256 distinct decision vectors, the reference is the
SAME entry point called once at B = 256, and every block of 256 rows of every output must equal that reference bit for bit --
compared where the output lies, chunk by chunk, so that no second full-size buffer exists.  Which form a batch size selects is asked
of the library (gel_aero_launch_info, gel_jac_products_launch_info: the functions the launchers decide by) or follows from plain
arithmetic on the dims (a buffer past 2^31 elements); no launcher threshold is restated here.

Importing this module needs neither a GPU nor torch."""
import numpy as np

P = 256                      # distinct vectors of a batch
SAMPLES = (0, 77, P - 1)     # the vectors that are also held against the one-vector host call and an independent anchor
LIMIT_BYTES = 64e9           # no test may need more device memory than this
POISON = 7.0                 # what every output holds before a call (a cell the call does not write keeps it, in both sizes)
CHUNK_ELEMS = 1 << 27        # elements compared at a time (the comparison's temporary is one byte per element)


# ---- batch sizes ----------------------------------------------------------------------------------------------------------------
def round_up(n, m=P):
    return -(-int(n) // m) * m


def first_multiple_past(threshold, per_vector, m=P):
    """smallest multiple of m whose batch holds MORE than `threshold` units at `per_vector` units per vector"""
    B = round_up(int(threshold) // int(per_vector) + 1, m)
    assert B * per_vector > threshold and (B - m) * per_vector <= threshold
    return B


def first_multiple_where(pred, lo, hi, m=P):
    """smallest multiple of m in (lo, hi] with pred(B), for a pred that is false at lo, true at hi and changes once (bisection over
    the library's own answer)"""
    a, b = int(lo) // m, int(hi) // m
    assert a * m == lo and b * m == hi and not pred(lo) and pred(hi)
    while b - a > 1:
        c = (a + b) // 2
        if pred(c * m):
            b = c
        else:
            a = c
    return b * m


def engine(name, flags=0, cfg=None, device=0):
    """(engine, prob, x0) of a named problem, configured like the caller-stream cases (stream_cases.CONFIGS)"""
    from gelato_amd import Engine
    import jac_products_truth as jt
    import stream_cases as SC
    prob, x0 = jt.named(name)
    E = Engine(prob, flags=flags, device=device)
    if cfg:
        SC.CONFIGS[cfg](E)
    return E, prob, x0


def distinct_vectors(E, x0, seed=3):
    from gelato_amd import problem
    return problem.synthetic_batch(x0, E.M, P, seed=seed)


def aero_dense_bytes(E):
    """bytes of one vector's gradient values of the largest kind in gel_eval_aero_all_device's dense arrays"""
    return 8 * max(sum(E.aero_dims(k)[1]) for k in E.AERO_KINDS)


def aero_dense_B(E, region):
    """"negative": the smallest multiple of 256 whose largest gradient array exceeds 2^31 bytes (the flat mapping's 32-bit byte
    offsets of its last vectors are negative as `int`); "tiles": the smallest multiple of 256 for which the launcher gives up the
    flat mapping -- found by asking gel_aero_launch_info, not by restating its threshold"""
    Bn = first_multiple_past(2 ** 31, aero_dense_bytes(E))
    if region == "negative":
        return Bn
    assert region == "tiles"
    hi = round_up(2 ** 32 // aero_dense_bytes(E) + 1)          # the array itself is past 2^32 bytes here: no 32-bit offset reaches its end
    return first_multiple_where(lambda B: E.aero_launch_info(B)["flat"] == 0, Bn, hi)


# ---- the checker ------------------------------------------------------------------------------------------------------------------
def _bits(a):
    """[rows, width] view of a tensor / array with float64 seen as int64 (bit comparison: NaN payloads and the sign of zero count)"""
    import torch
    t = torch.from_numpy(a) if isinstance(a, np.ndarray) else a
    assert t.is_contiguous()
    t = t.reshape(t.shape[0], -1)
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def first_mismatch(out, ref, cols=None, chunk_elems=CHUNK_ELEMS):
    """out [B, ...], ref [p, ...] (torch tensors on one device, or numpy arrays): None where row b of out equals row b % p of ref bit
    for bit for every b, else (row, cell) of the first difference in row-major order.  cols (1-D int64 tensor): compare these cells of
    a row only; the cell reported is the original index.  Works through out in chunks of whole blocks of p rows."""
    o, r = _bits(out), _bits(ref)
    B, w = o.shape
    p = r.shape[0]
    assert r.shape[1] == w and o.dtype == r.dtype and B >= 1
    if cols is not None:
        r = r[:, cols]
    wc = r.shape[1]
    per = max(1, chunk_elems // (p * wc))                      # blocks per chunk
    for k0 in range(0, B // p, per):
        k1 = min(B // p, k0 + per)
        blk = o[k0 * p:k1 * p]
        if cols is not None:
            blk = blk[:, cols]
        ne = blk.reshape(k1 - k0, p, wc) != r
        if bool(ne.any()):
            i = int(ne.reshape(-1).nonzero()[0, 0])
            row, c = k0 * p + i // wc, i % wc
            return row, (int(cols[c]) if cols is not None else c)
    tail = B % p
    if tail:
        blk = o[B - tail:]
        if cols is not None:
            blk = blk[:, cols]
        ne = blk != r[:tail]
        if bool(ne.any()):
            i = int(ne.reshape(-1).nonzero()[0, 0])
            row, c = B - tail + i // wc, i % wc
            return row, (int(cols[c]) if cols is not None else c)
    return None


def flip_bit(out, row, cell, bit=0):
    """one bit of one cell, in place (twice = restored)"""
    o = _bits(out)
    m = 1 << bit
    o[row, cell] ^= (m - (1 << 64)) if m >= (1 << 63) else m     # bit 63 of an int64 as a negative value


def teeth_cells(B, w, itemsize=8, rows=()):
    """(row, cell) of the cells a planted bit must be found in: the last cell of the last vector, the first cell past 2^31 bytes and
    past 2^31 elements of the buffer where it is that long, and cell 0 of every row in `rows` (the first vector of a second run)"""
    cells = [(B - 1, w - 1)]
    for flat in (2 ** 31 // itemsize, 2 ** 31):
        if flat < B * w and divmod(flat, w) not in cells:
            cells.append(divmod(flat, w))
    cells += [(int(r), 0) for r in rows if (int(r), 0) not in cells]
    return cells


def check_blocks(out, ref, what="", rows=(), cols=None, teeth=True):
    """every block of out equals ref; then the checker's teeth: one bit planted in each of teeth_cells() is found exactly there, and
    taken out again.  -> the cells the teeth were shown at"""
    bad = first_mismatch(out, ref, cols)
    assert bad is None, "%s: row %d (vector %d of the %d distinct ones), cell %d differs from the B = %d reference" % (
        what, bad[0], bad[0] % ref.shape[0], ref.shape[0], bad[1], ref.shape[0])
    if not teeth:
        return []
    o = _bits(out)
    cells = teeth_cells(o.shape[0], o.shape[1], o.element_size(), rows)
    if cols is not None:                                      # a planted bit outside the compared cells would not be looked at
        cells = [(r, int(cols[min(int((cols < c).sum()), len(cols) - 1)])) for r, c in cells]
    for row, cell in cells:
        flip_bit(out, row, cell)
        found = first_mismatch(out, ref, cols)
        flip_bit(out, row, cell)
        assert found == (row, cell), "%s: a bit planted at row %d, cell %d was reported as %r" % (what, row, cell, found)
    return cells

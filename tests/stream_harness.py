"""Caller-owned streams (test infrastructure of tests/test_caller_stream.py; a helper, not a conftest).

Every device entry point of include/gelato_amd.h takes a `void* stream`.  A case is run here on a NON-BLOCKING side stream
(torch.cuda.Stream()) whose input arrives late:

    device input buffer = x_stale (another valid, finite input of the same shape), every output buffer = 7.0
    side stream, no host synchronisation in between:
        delay  ->  d_in.copy_(x_good)  ->  the engine call(s) with side.cuda_stream  ->  snap.copy_(out)  ->  out.fill_(-3.0)
    assert side.query() is False          (everything was enqueued behind a producer that had not run yet)
    rc = E.sync(side.cuda_stream)
    snap == the same call with stream = 0 on fresh buffers holding x_good, BIT FOR BIT;  out == -3.0 everywhere;  rc == 0

A launch, memset or workspace tied to another stream than the caller's runs early (stale input: plausible wrong numbers, no NaN)
or late (writes over the -3.0).  The handle's own stream is a blocking stream and torch's default stream is the null stream: the
two synchronise implicitly, which is why a test on torch.cuda.current_stream() (value 0 = the handle's stream) cannot see any of it.

The delay is torch.cuda._sleep(cycles) (one lane spinning on the clock: the CUs stay free), calibrated once per process with two
events.  It lasts FACTOR x the case's own duration -- measured with events around the stream = 0 reference run, i.e. on the
reference path -- and at least MIN_DELAY_MS (the host's enqueue time; side.query() checks it), at most MAX_DELAY_MS.  Nothing here
can block a stream for longer than that: no host-memory spin, no wait on a value.

Lifetime rule: every tensor the side stream touches is held by the Pending object until the stream has been synchronised (the
caching allocator does not know about the side stream)."""
import numpy as np

SENTINEL, POISON = 7.0, -3.0
FACTOR = 10.0
MIN_DELAY_MS, MAX_DELAY_MS = 20.0, 200.0

_sides = []
report = {"cycles_per_ms": None, "largest_delay_ms": 0.0, "cases": 0}


def side_stream(k=0):
    """one of the (at most two) non-blocking side streams of this process, on the current device"""
    import torch
    assert k in (0, 1), "at most two side streams per process"
    while len(_sides) <= k:
        _sides.append(torch.cuda.Stream())
    return _sides[k]


def cycles_per_ms():
    """clock cycles of torch.cuda._sleep per millisecond, measured once: the cycle count grows by tens until the sleep lasts 5 ms"""
    import torch
    if report["cycles_per_ms"] is None:
        s = side_stream(0)
        cycles, ms = 100_000, 0.0
        with torch.cuda.stream(s):
            torch.cuda._sleep(cycles)          # the kernel's code is loaded by its first launch
            s.synchronize()
            for _ in range(6):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                torch.cuda._sleep(cycles)
                b.record()
                s.synchronize()
                ms = a.elapsed_time(b)
                if ms >= 5.0:
                    break
                cycles *= 10
        assert 5.0 <= ms <= 10 * MAX_DELAY_MS, "torch.cuda._sleep cannot be calibrated: %d cycles took %.3f ms" % (cycles, ms)
        report["cycles_per_ms"] = cycles / ms
        print("caller-stream harness: torch.cuda._sleep runs %.0f cycles per ms (%d cycles took %.3f ms)" % (cycles / ms, cycles, ms))
    return report["cycles_per_ms"]


def delay_ms_for(case_ms):
    """the delay of a case that takes case_ms on the handle's stream"""
    ms = max(MIN_DELAY_MS, FACTOR * case_ms)
    assert ms <= MAX_DELAY_MS, "the case takes %.2f ms: %.0f x that is above the %.0f ms cap of a delay" % (case_ms, FACTOR, MAX_DELAY_MS)
    return ms


def enqueue_delay(ms):
    """a delay of ms on torch's current stream"""
    import torch
    assert 0 < ms <= MAX_DELAY_MS
    torch.cuda._sleep(int(ms * cycles_per_ms()))
    report["largest_delay_ms"] = max(report["largest_delay_ms"], ms)


class Case:
    """One case: E the engine; B vectors; late = {name: (good, stale)} host arrays [P][w] (row b of the device buffer is row b % P)
    that arrive behind the delay; fixed = {name: array} resident inputs; outputs = {name: shape}; call(E, ptr, stream) makes the
    engine call(s), ptr = {name: device pointer}; select = {output name: int64 column index} where only some columns of a
    [B][w] output are defined (the padding of the aero record)."""

    def __init__(self, E, B, late, outputs, call, fixed=None, select=None):
        self.E, self.B, self.late, self.outputs, self.call = E, int(B), dict(late), dict(outputs), call
        self.fixed, self.select = dict(fixed or {}), dict(select or {})

    def with_late(self, **late):
        c = Case(self.E, self.B, self.late, self.outputs, self.call, self.fixed, self.select)
        c.late.update(late)
        return c


def _dev(a, B):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if t.shape[0] != B:
        t = t.repeat((B + t.shape[0] - 1) // t.shape[0], *([1] * (t.dim() - 1)))[:B].contiguous()
    return t


def _outputs(case, value):
    import torch
    return {k: torch.full(tuple(shp), value, dtype=torch.float64, device="cuda") for k, shp in case.outputs.items()}


def _ptrs(*dicts):
    return {k: t.data_ptr() for d in dicts for k, t in d.items()}


def reference(case, which=0, timed=True):
    """the case with stream = 0 (the handle's own stream) on fresh buffers holding the good (which = 0) or the stale (1) input
    -> ({output: tensor}, status of E.sync(0), duration in ms of the second of two runs, events on torch's default stream)"""
    import torch
    E = case.E
    ins = {k: _dev(v[which], case.B) for k, v in case.late.items()}
    ins.update({k: _dev(v, v.shape[0]) for k, v in case.fixed.items()})
    outs = _outputs(case, SENTINEL)
    ptr = _ptrs(ins, outs)
    torch.cuda.synchronize()
    ms = 0.0
    if timed:
        case.call(E, ptr, 0)            # a kernel's first launch loads its code: not timed
        E.sync(0)
        for t in outs.values():
            t.fill_(SENTINEL)
        torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    case.call(E, ptr, 0)
    b.record()
    rc = E.sync(0)
    torch.cuda.synchronize()
    if timed:
        ms = a.elapsed_time(b)
    return outs, rc, ms


class Pending:
    """one case's buffers on the device (prepare) and what start() has put on its side stream; holds every tensor until finish()"""

    def __init__(self, case, side, stale, good, fixed, outs, snaps, on_handle):
        self.case, self.side, self.stale, self.good, self.fixed = case, side, stale, good, fixed
        self.outs, self.snaps, self.on_handle = outs, snaps, on_handle

    def start(self, delay_ms, call=None):
        """delay, late input, engine call(s), snapshots, poison -- no host synchronisation in between"""
        import torch
        case, call = self.case, call or self.case.call
        ptr = _ptrs(self.stale, self.fixed, self.outs)

        def engine_and_snapshots(stream):
            call(case.E, ptr, stream)
            for k_ in self.outs:
                self.snaps[k_].copy_(self.outs[k_])
                self.outs[k_].fill_(POISON)
        with torch.cuda.stream(self.side):
            enqueue_delay(delay_ms)
            for k_ in self.stale:
                self.stale[k_].copy_(self.good[k_], non_blocking=True)
            if not self.on_handle:
                engine_and_snapshots(self.side.cuda_stream)
        if self.on_handle:
            engine_and_snapshots(0)          # snapshots and poison on torch's default stream, behind the handle's blocking stream
        return self

    def assert_pending(self):
        assert self.side.query() is False, "delay too short: the side stream had drained before everything was enqueued"

    def finish(self):
        """synchronises (E.sync on the side stream) -> (snapshots, outputs as they are afterwards, status)"""
        import torch
        rc = self.case.E.sync(self.side.cuda_stream)
        if self.on_handle:
            rc = max(rc, self.case.E.sync(0))
        torch.cuda.synchronize()
        self.stale = self.good = self.fixed = None
        return self.snaps, self.outs, rc


def prepare(case, k=0, engine_on_handle=False):
    """the buffers of one run on side stream k: inputs holding the STALE values, outputs holding 7.0.  The caller synchronises the
    device (torch.cuda.synchronize()) once everything is prepared and before the first start(): a non-blocking stream does not wait
    for the default stream the buffers were filled on."""
    side = side_stream(k)
    stale = {k_: _dev(v[1], case.B) for k_, v in case.late.items()}
    good = {k_: _dev(v[0], case.B) for k_, v in case.late.items()}
    fixed = {k_: _dev(v, v.shape[0]) for k_, v in case.fixed.items()}
    cycles_per_ms()
    return Pending(case, side, stale, good, fixed, _outputs(case, SENTINEL), _outputs(case, 0.0), engine_on_handle)


def enqueue(case, delay_ms, k=0, engine_on_handle=False, call=None):
    """prepare + synchronise + start for one case.
    engine_on_handle (the teeth of the harness): the producer stays on the side stream, the engine call gets stream = 0 and the
    snapshots follow it on torch's default stream; the handle's blocking stream does not wait for a non-blocking side stream."""
    import torch
    p = prepare(case, k, engine_on_handle)
    torch.cuda.synchronize()
    return p.start(delay_ms, call)


def same_bits(a, b):
    import torch
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)))


def compare(case, snaps, ref, rows=None):
    """-> names of the outputs whose snapshot is not the reference bit for bit (rows: only these vectors of the batch)"""
    import torch
    bad = []
    for name in case.outputs:
        a, b = snaps[name], ref[name]
        if name in case.select:
            idx = torch.as_tensor(case.select[name], device=a.device)
            a, b = a[:, idx], b[:, idx]
        if rows is not None:
            r = torch.as_tensor(rows, device=a.device)
            a, b = a[r], b[r]
        if not same_bits(a, b):
            bad.append(name)
    return bad


def poisoned(outs):
    """-> names of the outputs that are NOT -3.0 everywhere (something wrote after the snapshot)"""
    return [k for k, t in outs.items() if not bool((t == POISON).all())]


def check(case, label="", expect_rc=0, rows=None, k=0):
    """the whole protocol of the module docstring for one case -> {output: snapshot tensor}"""
    ref, rc_ref, ms = reference(case)
    assert rc_ref == expect_rc, (label, "stream = 0 status", rc_ref)
    d = delay_ms_for(ms)
    p = enqueue(case, d, k)
    p.assert_pending()
    snaps, outs, rc = p.finish()
    report["cases"] += 1
    print("caller-stream %s: case %.3f ms on the handle's stream, delay %.1f ms (%.0f cycles per ms; largest delay so far %.1f ms)"
          % (label, ms, d, report["cycles_per_ms"], report["largest_delay_ms"]))
    assert rc == expect_rc, (label, "status on the caller's stream", rc)
    assert compare(case, snaps, ref, rows) == [], (label, "not the bits of the stream = 0 call")
    assert poisoned(outs) == [], (label, "written after the snapshot")
    return snaps

"""A stalled stream with a built-in control: the helpers of tests/test_gpu_stream_order.py ("Stream contract").

include/ron_hip.h promises that every entry point enqueues its work on the stream it is given and does not synchronise with the
host.  On an idle default stream with inputs that were complete long ago neither promise can be seen to fail.  Here the caller's
stream is busy with one long, finite kernel (the stall) and the real inputs are copied into the input buffers BEHIND it; until
then the buffers hold poison: another valid case of the same shapes.  Whatever part of an entry runs on some other stream without
waiting runs during the stall, reads the poison (or is overwritten later), and the result differs from the one computed on the
default stream.

Every use asserts that the stall was still pending when the last piece of host work had been enqueued (`marker.query() is False`):
a stall that had already ended proves nothing, and the test fails as inconclusive instead of passing."""
import contextlib
import gc
import time

import torch

STALL_MS = 250.0          # default stall: see DESIGN.md for the measured enqueue times it has to outlast
MAX_STALL_MS = 1000.0     # no single stall is longer than this: a test stays within a few seconds
PROBE_MS = 40.0           # stall of one independent_stream() probe
MAX_TRIES = 8             # fresh streams independent_stream() looks at before it gives up

INCONCLUSIVE = ('inconclusive: the stall had ended before all host work was enqueued (a host synchronisation inside the call, or a '
                'stall shorter than the enqueue)')

_CYCLES_PER_MS = {}
_INDEPENDENT = {}         # device index -> streams found so far (kept for the session: at most 16 streams per process)
ENQUEUE_MS = {}           # label -> host milliseconds from the stall to the last enqueue of a run_late()


def cycles_per_ms(device):
    """torch.cuda._sleep counts device clock ticks: how many make a millisecond, measured once per session with events on the idle
    default stream (the second of two runs: the first loads the kernel)."""
    key = torch.device(device).index or 0
    if key not in _CYCLES_PER_MS:
        cycles = 4 * 1000 * 1000
        with torch.cuda.device(key):
            torch.cuda.synchronize()
            ms = 0.0
            for _ in range(2):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                torch.cuda._sleep(cycles)
                b.record()
                b.synchronize()
                ms = a.elapsed_time(b)
        assert ms > 0.05, 'torch.cuda._sleep(%d) took %g ms: cannot calibrate a stall' % (cycles, ms)
        _CYCLES_PER_MS[key] = cycles / ms
    return _CYCLES_PER_MS[key]


def stall(stream, ms=None):
    """One long, finite piece of device work on `stream`; returns the stall marker, an event recorded right behind it."""
    ms = STALL_MS if ms is None else float(ms)
    assert 0 < ms <= MAX_STALL_MS, 'a stall of %g ms is outside (0, %g]' % (ms, MAX_STALL_MS)
    cycles = int(ms * cycles_per_ms(stream.device))
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
        marker = torch.cuda.Event()
        marker.record(stream)
    return marker


def _runs_beside(stalled, other):
    """True when a tiny op on `other` completes while `stalled` is still busy: the two do not share a hardware queue."""
    torch.cuda.synchronize()
    marker = stall(stalled, PROBE_MS)
    with torch.cuda.stream(other):
        probe = torch.zeros((8,), dtype=torch.float32, device=stalled.device).add_(1.0)
        done = torch.cuda.Event()
        done.record(other)
    done.synchronize()                       # returns at once, or behind the stall when the queue is shared: finite either way
    beside = marker.query() is False
    stalled.synchronize()
    del probe
    return beside


def independent_stream(dev, index=0):
    """The index-th stream of this session that runs beside the default stream and beside the earlier ones of this list.

    A process has a handful of hardware queues and several streams can share one; a side stream that shares the default stream's
    queue would serialise behind a stall and hide exactly what these tests look for.  Fresh streams are probed (stall the candidate,
    run a tiny op on each of the others, see it complete while the stall is pending); at most MAX_TRIES per stream."""
    dev = torch.device(dev)
    found = _INDEPENDENT.setdefault(dev.index or 0, [])
    with torch.cuda.device(dev):
        while len(found) <= index:
            others = [torch.cuda.default_stream(dev)] + found
            for _ in range(MAX_TRIES):
                s = torch.cuda.Stream(device=dev)
                if all(_runs_beside(s, o) for o in others):
                    found.append(s)
                    break
            else:
                raise AssertionError('no stream independent of the default stream%s among %d fresh ones: every one of them shares a '
                                     'hardware queue with it, so a stalled side stream would serialise the work under test'
                                     % (' and %d earlier side stream(s)' % len(found) if found else '', MAX_TRIES))
    return found[index]


@contextlib.contextmanager
def quiet_host():
    """The window between a stall and the last marker query holds nothing but the enqueue under test: no cyclic garbage collection
    (a full collection of a long pytest session's objects can take longer than a stall)."""
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


def run_late(stream, fill, call, collect, blocks_host=False, stall_ms=None, label=None):
    """The pattern every test uses.  The caller has computed `expected` on the default stream, left poison in the input buffers and
    a sentinel in the output buffers.  Here: synchronise; on `stream`: stall, fill() (device-to-device copies of the real inputs into
    the input buffers), call() (the entry under test, which picks up torch's current stream), collect(out) (copies of the outputs,
    on the same stream); synchronise the stream; return what collect returned.

    blocks_host False: the stall marker must still be pending when call() returns (the entry did not synchronise with the host) and
    when collect() has returned (the test is conclusive).  True (entries documented to block the host): it must be pending
    immediately before call()."""
    with torch.cuda.stream(stream):          # once on this stream, on the poison, outside the timed window: the allocator's pool of
        del_me = collect(call())             # the stream and the entry's scratch exist, so the window below allocates nothing new;
    del del_me                               # the blocks the outputs will reuse now hold the poison's results
    torch.cuda.synchronize()
    with quiet_host():
        t0 = time.perf_counter()
        with torch.cuda.stream(stream):
            marker = stall(stream, stall_ms)
            fill()
            pending_before = marker.query() is False
            out = call()
            pending_at_return = marker.query() is False
            kept = collect(out)
            pending_at_end = marker.query() is False
        ms = (time.perf_counter() - t0) * 1e3
    if label is not None:
        ENQUEUE_MS[label] = ms
    stream.synchronize()                     # before any assertion: nothing stays queued on buffers a failing test lets go of
    assert pending_before, INCONCLUSIVE + ' [before the call, %.2f ms after the stall was issued]' % ms
    if not blocks_host:
        assert pending_at_return, ('the stall marker was complete when the call returned, %.2f ms after the stall was issued: the '
                                   'entry synchronised with the host (or: ' % ms) + INCONCLUSIVE + ')'
        assert pending_at_end, INCONCLUSIVE + ' [after collect, %.2f ms]' % ms
    return kept


def run_misdirected(stream, fill, call, collect, stall_ms=None):
    """The positive control: the mistake of passing the wrong stream.  The real inputs arrive late on the stalled `stream`, but
    call() and collect() run OUTSIDE the stream context, i.e. on the default stream, during the stall: they read the poison.  The
    stream is stalled, the poison is valid data and nothing writes the buffers concurrently (the fill waits behind the stall), so the
    outcome is deterministic and nothing can fault.  Returns what collect returned, after a device synchronise."""
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        marker = stall(stream, stall_ms)
        fill()
    kept = collect(call())
    done = torch.cuda.Event()
    done.record(torch.cuda.current_stream())
    done.synchronize()                       # the misdirected work has finished ...
    pending = marker.query() is False        # ... while the real inputs were still held back
    torch.cuda.synchronize()
    assert pending, INCONCLUSIVE + ' [control]'
    return kept


def same_bytes(a, b):
    """Two lists of tensors, equal in shape, dtype and bytes (NaN payloads included).  Call after the synchronise only."""
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if x.shape != y.shape or x.dtype != y.dtype:
            return False
        if x.contiguous().cpu().numpy().tobytes() != y.contiguous().cpu().numpy().tobytes():
            return False
    return True

"""Delay injection for the streams of a step (tests/test_stream_delay_host.py, tests/test_gpu_stream_delays.py).

A step is deterministic from run to run, so its results may not depend on WHEN a stream gets to its work: with every
ordering between the streams in place — ``OP_WAIT`` records, ``wait_stream`` / ``wait_event`` / ``avid_stream_wait`` calls,
``record_stream`` towards the allocator — a stream that is late by much more than the whole step takes changes no bit.  A
missing ordering passes every undisturbed test as long as the producer happens to finish first, which at test shapes it
nearly always does; a delay on the producer's stream makes it lose that race reliably.

The delay is ``avid_probe_spin`` (csrc/program.hip): one wave that spins, bounded by the entry point (< 100 ms).  Nothing here
removes or weakens an ordering of a real program: a delay only ADDS work to a stream."""
import contextlib
import ctypes as C

SPIN_CHUNK_MS = 50            # one launch spins this long at the most (avid_probe_spin refuses 100 ms and more)
FACTOR, FLOOR_MS, CEILING_MS = 3.0, 5.0, 150.0
EXTRA_CUTS = 8


def spin(stream, ms):
    """``ms`` milliseconds of spinning on the raw stream handle ``stream``: a chain of launches of at most SPIN_CHUNK_MS each.
    Returns the number of launches."""
    from avid_hip import lib
    us, launches = int(round(ms * 1000.0)), 0
    handle = stream if isinstance(stream, C.c_void_p) else C.c_void_p(stream)
    while us > 0:
        part = min(us, SPIN_CHUNK_MS * 1000)
        lib.call("avid_probe_spin", part, handle)
        us -= part
        launches += 1
    return launches


def delay_ms(t0_ms):
    """D of a step that takes ``t0_ms`` undisturbed: three times the step — the late stream has to outlast everything the others
    can still do without it, and avid_probe_spin converts microseconds at an assumed 2.1 GHz shader clock — and 5 ms at least.
    A step too long for a 150 ms delay is too large for these tests: the answer is a smaller shape, not a smaller factor."""
    d = max(FACTOR * float(t0_ms), FLOOR_MS)
    if d > CEILING_MS:
        raise ValueError(f"a step of {t0_ms:.2f} ms needs a delay of {d:.1f} ms (> {CEILING_MS:.0f} ms): use a smaller shape")
    return d


def program_cuts(prog, n):
    """The record indices at which a program of ``n`` records may be split for a delay: 0, the index behind every ``OP_WAIT``
    record, and EXTRA_CUTS evenly spaced further ones — never an ``OP_WGRAD_ITEM`` (a group and its items stay in one call:
    an index that lands on an item moves back to its group record).  Sorted, each once, all inside [0, n].

    The cuts behind waits are the ones that matter: a consumer that waited on stream s for an earlier producer is released when
    that producer ends; a later producer on s that it does NOT wait for then runs right behind the earlier one, and only a
    delay placed on s after that wait makes it reliably late."""
    from avid_hip import plan
    cuts = {0}
    for k in range(n):
        if prog[k].op == plan.OP_WAIT:
            cuts.add(k + 1)
    for j in range(1, EXTRA_CUTS + 1):
        cuts.add(n * j // (EXTRA_CUTS + 1))
    out = set()
    for k in cuts:
        while 0 < k < n and prog[k].op == plan.OP_WGRAD_ITEM:
            k -= 1
        out.add(k)
    return sorted(out)


class _Fired:
    """What a context of this module did: ``spins`` delays issued, ``count`` launching calls seen (``delayed_calls``)."""

    def __init__(self):
        self.spins, self.count, self.names = 0, 0, []


@contextlib.contextmanager
def delayed_programs(stream_index, cut, ms, which, visit=None):
    """Inside: a run of the launch program ``which`` ("fwd" / "bwd": told by the identity of the record array, ``self.fwd_prog`` /
    ``self.bwd_prog``) whose range [begin, end) holds ``cut`` is issued as [begin, cut), then ``spin`` on the run's stream
    ``stream_index`` (``self.streams``), then [cut, end).  A cut equal to the program's length is held by the range that ends
    there (the delay goes behind the last record).  Every other program and every range that does not hold the cut — the
    segmented ``backward(begin, end)`` — passes through untouched.  ``visit``: only the visit-th such run (0: the first; a
    virtual-rank step runs one program once per shard), default every one.  Yields the record of what was done."""
    from avid_hip import plan
    fired = _Fired()
    original = plan.Programs._run
    seen = [0]

    def _run(self, prog, begin, end):
        chosen = getattr(self, "fwd_prog" if which == "fwd" else "bwd_prog", None)
        holds = begin <= cut < end or (cut == end == len(prog))
        if prog is not chosen or not holds:
            return original(self, prog, begin, end)
        k, seen[0] = seen[0], seen[0] + 1
        if visit is not None and k != visit:
            return original(self, prog, begin, end)
        if cut > begin:
            original(self, prog, begin, cut)
        spin(self.streams[stream_index], ms)
        fired.spins += 1
        if end > cut:
            original(self, prog, cut, end)

    plan.Programs._run = _run
    try:
        yield fired
    finally:
        plan.Programs._run = original


_QUERIES = {"avid_last_error", "avid_version", "avid_device_info", "avid_timing_enable", "avid_timing_report",
            "avid_conv_kernel_name", "avid_conv_wgrad_groupable", "avid_set_cu_budget", "avid_cu_budget",
            "avid_logspec_basis_floats", "avid_program_instr_bytes"}


def launches(name):
    """``lib.call(name, ...)`` puts work on a stream: everything but the pure queries — sizes (``*_bytes``, ``*_rows``), dispatch
    questions (``avid_conv_uses_*``, ``avid_conv_takes_*``, ``avid_conv_kernel_name``), switches (``*_configure``), counters
    (``avid_debug_*``) and their like."""
    if name in _QUERIES or name.endswith(("_bytes", "_rows", "_configure")):
        return False
    return not name.startswith(("avid_conv_uses_", "avid_conv_takes_", "avid_debug_"))


@contextlib.contextmanager
def delayed_calls(stream_index, nth, ms, device=None):
    """Inside: ``lib.call`` is wrapped; in front of the ``nth`` launching call (0: the first; ``launches`` says what counts)
    ``spin`` goes on stream ``stream_index`` of ``streams.current_set(device)`` — the set the calling thread's current stream
    belongs to, so a call issued by autograd's thread or under a helper stream finds the step's four streams.  Every call returns
    what ``lib.call`` returns.  ``nth=None``: a dry run.  Yields the record: ``count`` launching calls seen, their ``names``."""
    import torch
    from avid_hip import lib, streams
    fired = _Fired()
    original = lib.call

    def call(name, *args):
        if launches(name):
            k, fired.count = fired.count, fired.count + 1
            fired.names.append(name)
            if nth is not None and k == nth:
                dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
                ss = streams.current_set(dev)
                handle = (ss.main, ss.side, ss.trail, ss.comm)[stream_index].cuda_stream
                lib.call = original                  # (the delay's own launches are not counted and not wrapped)
                try:
                    spin(handle, ms)
                finally:
                    lib.call = call
                fired.spins += 1
        return original(name, *args)

    lib.call = call
    try:
        yield fired
    finally:
        lib.call = original


def time_ms(run, warmup=1, repeats=3):
    """T0: the median of ``repeats`` runs of ``run()`` after ``warmup`` ones, each timed with events on the current (compute)
    stream and ended with a device synchronisation."""
    import torch
    for _ in range(warmup):
        run()
        torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]

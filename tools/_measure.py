"""The timing, memory and launch-count helpers of tools/*.py: the only timing code under tools/*.py (DESIGN §3.38 lists the few
loops that stay in their tools, and why).  A number means what the docstring of the function that produced it says; every caller
passes its warm-up and iteration counts explicitly.  All of them need the GPU: a CPU run measures nothing.

Three kinds of step time, which are not comparable with each other:
  event_ms / alternate    device events around ONE call, the host waiting for each call's end: the call alone on an idle stream
                          (launch latency of the first kernel included, no overlap between calls);
  event_total_ms          device events around a window of back-to-back calls: the calls queued behind each other, so the device
                          never waits for the host unless the host is the slower of the two;
  host_ms                 host clock around a window that starts and ends with the queue drained: what a user waits.
enqueue_ms is no step time: it is the host's share alone."""
import time

import numpy as np
import torch


def _warm(fn, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()


def event_ms(fn, iters, warmup):
    """-> (median, min, max) ms of one call of fn().  `warmup` untimed calls, the queue drained, then `iters` calls, each between
    its own pair of device events on the current stream, the host waiting on the end event before the next call starts.
    Covers: device time of the call on an otherwise idle stream, from its first kernel's dispatch to its last kernel's end, gaps
    between its kernels included.  Excludes: the warm-up, host work before the first enqueue of a call, overlap between calls."""
    _warm(fn, warmup)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(iters):
        start.record()
        fn()
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def event_queued_ms(fn, iters, warmup):
    """-> (list of `iters` ms, the last call's return value).  As event_ms, but with one event pair per call and one wait after
    the last call: the host runs ahead, so a call's span starts when the device reaches its start event (behind the previous call)
    and host enqueue time shows only where the device runs dry.  Excludes: the warm-up."""
    out = None
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in evs:
        a.record()
        out = fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in evs], out


def event_total_ms(fn, iters, warmup):
    """-> ms per call: one pair of device events around `iters` back-to-back calls of fn(), divided by iters (a mean).  `warmup`
    untimed calls and a drained queue before the window; one wait after it.
    Covers: device time of the window, the calls queued behind each other; where the host enqueues slower than the device runs, the
    host's time.  Excludes: the warm-up; says nothing about the spread between calls."""
    _warm(fn, warmup)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def event_and_enqueue_ms(fn, steps):
    """-> (device ms per call, host enqueue ms per call) of one window of `steps` calls of fn(): event_total_ms and enqueue_ms
    taken on the same window.  No warm-up of its own; the queue is drained before the window, and the host clock stops when the
    last call returns, before the final wait."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return start.elapsed_time(end) / steps, host * 1e3 / steps


def host_ms(fn, steps, warmup=0):
    """-> ms per call (a mean) by the host clock around `steps` calls of fn(), the queue drained before the clock starts and
    again before it stops.  `warmup` untimed calls first (0: the caller warms up itself).
    Covers: everything between the first call and the end of the last kernel: host work, enqueue, device time, synchronisations
    inside fn.  Excludes: the warm-up."""
    _warm(fn, warmup)
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def enqueue_ms(fn, iters):
    """-> host ms per call to enqueue `iters` calls of fn(): the queue drained first, the clock stopped when the last call returns,
    the final wait untimed.  Covers: host time only (Python, launches, any synchronisation inside fn).  Excludes: device time
    that the host does not wait for; for a sync-free fn this is no step time."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (t1 - t0) / iters * 1e3


def alternate(fns, iters, warmup):
    """{name: (median ms, min ms)}, the callables timed in turn within every iteration; each call as in event_ms (own event pair,
    the host waiting for its end), so a drift of the machine hits every column alike"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for k in fns}
    times = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            ev[k][0].record()
            fn()
            ev[k][1].record()
            ev[k][1].synchronize()
            times[k].append(ev[k][0].elapsed_time(ev[k][1]))
    return {k: (float(np.median(v)), float(np.min(v))) for k, v in times.items()}


def peak_mb(fn):
    """-> MiB (one decimal) that one call of fn() allocates at its peak above what was allocated before the call, from torch's
    caching allocator (max_memory_allocated).  Excludes: memory that does not come from that allocator, and cached free blocks."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def kernel_count(fn):
    """-> {"kernels", "copies", "d2h_copies", "item_calls", "names"} of one call of fn() under torch.profiler, after one untimed
    call: device kernels (memcpy and memset events excluded), all device copies, the device-to-host ones among them, aten::item
    calls (scalar reads: each waits for the device), and the sorted distinct kernel names cut at the first '<' or '('.
    A count, not a time: the profiler slows the host."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    dev_events = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA")]
    names = [n for n in dev_events if "memcpy" not in n.lower() and "memset" not in n.lower()]
    copies = [n for n in dev_events if "memcpy" in n.lower()]
    d2h = [n for n in copies if "dtoh" in n.lower().replace(" ", "")]
    items = sum(1 for e in prof.events() if e.name == "aten::item")
    short = lambda n: n.split("<")[0].split("(")[0].strip()   # noqa: E731  templated torch kernels carry names of several KB
    return {"kernels": len(names), "copies": len(copies), "d2h_copies": len(d2h), "item_calls": items,
            "names": sorted({short(n) for n in names})}

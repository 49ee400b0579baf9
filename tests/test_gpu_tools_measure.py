"""tools/_measure.py, the timing helpers every tool under tools/ reports through: call counts, ordering of the returned figures,
what enqueue time leaves out, the allocator peak and the interleaving of `alternate`.  No absolute time is asserted anywhere."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import _measure  # noqa: E402

pytestmark = pytest.mark.gpu
MIB = 2 ** 20


def _counted(dev):
    """x.add_(1) on a 1-element tensor, counting its calls"""
    x = torch.zeros(1, device=dev)
    calls = []

    def fn():
        calls.append(1)
        x.add_(1)
    return fn, calls, x


def test_event_ms_calls_and_order(dev):
    fn, calls, x = _counted(dev)
    med, lo, hi = _measure.event_ms(fn, 7, 3)
    assert len(calls) == 3 + 7 and float(x) == 10.0
    assert all(math.isfinite(v) and v > 0 for v in (med, lo, hi))
    assert lo <= med <= hi


def test_event_total_and_queued_calls(dev):
    fn, calls, _ = _counted(dev)
    per_call = _measure.event_total_ms(fn, 5, 2)
    assert len(calls) == 7 and math.isfinite(per_call) and per_call > 0
    times, out = _measure.event_queued_ms(lambda: fn() or len(calls), 4, 1)
    assert len(calls) == 12 and out == 12 and len(times) == 4 and all(t > 0 for t in times)


def test_host_and_enqueue_calls(dev):
    fn, calls, _ = _counted(dev)
    assert _measure.host_ms(fn, 6) > 0 and len(calls) == 6
    assert _measure.enqueue_ms(fn, 5) > 0 and len(calls) == 11
    gpu, enq = _measure.event_and_enqueue_ms(fn, 4)
    assert len(calls) == 15 and gpu > 0 and enq > 0
    _measure.host_ms(fn, 2, warmup=3)
    assert len(calls) == 20


def test_enqueue_excludes_the_drain(dev):
    buf = torch.empty(64 * MIB, dtype=torch.uint8, device=dev)
    fill = lambda: buf.fill_(1)   # noqa: E731
    fill()
    # one window for both: host_ms times a single call that is enqueue_ms over the 200 fills, so the host window holds the
    # enqueue window and the drain after it
    enq = []
    host = _measure.host_ms(lambda: enq.append(_measure.enqueue_ms(fill, 200)), 1) / 200
    print(f"64 MiB fill x 200: enqueue {enq[0]:.4f} ms per call, host {host:.4f} ms per call")
    assert len(enq) == 1 and 0 < enq[0] <= host


def test_peak_mb(dev):
    def alloc():
        t = torch.empty(32 * MIB, dtype=torch.uint8, device=dev)
        del t
    alloc()
    assert 32 <= _measure.peak_mb(alloc) <= 33


def test_alternate_interleaves(dev):
    order = []
    x = torch.zeros(1, device=dev)

    def make(name):
        def fn():
            order.append(name)
            x.add_(1)
        return fn
    res = _measure.alternate({"A": make("A"), "B": make("B")}, 3, 2)
    assert order == ["A", "B"] * 5
    assert set(res) == {"A", "B"} and all(0 < mn <= med for med, mn in res.values())

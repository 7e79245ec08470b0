"""Late ids: the one operation the ordering tests of tests/test_gpu_late_ids.py are built on.

Every ahead-of-time planner of this project reads id tensors on a side stream and promises something about who orders that
read behind the work that PRODUCES the ids.  A test that hands over ids staged and synchronised long before cannot see a
planner that reads too early.  LateIds.write makes the ids late:

  1. the id buffer is filled with a DECOY and the device synchronised;
  2. a gate (ha_stream_gate: one wave that holds a stream until the host writes a pinned word, bounded at ~2 s by its own
     loop) is enqueued on the caller's stream;
  3. `buf.copy_(real ids, staged elsewhere)` is enqueued behind the gate, and an event behind the copy.

The test then makes the call under test and calls LateIds.release: the event must not have completed (the gate is still
closed: the call did not wait on the host for the caller's stream), the host dwells DWELL seconds -- 30 x the 300-322 us of
the largest bookkeeping launch (README.md), so a reader that is not ordered behind the caller's stream has certainly run --,
the event must still not have completed, and the gate is opened.  A reader that ran early has read the decoy.

The decoy is a batch of VALID ids -- same count and dtype, every id in range, another unique set (asserted here, on the CPU):
a mis-ordered read gives wrong numbers, never an access out of range, a fault or a hang; and the gate never waits for anything
the test has not already enqueued."""
import threading
import time

import numpy as np
import torch

from herald_amd import _lib

DWELL = 0.010


def decoy_of(real, rows, sort=False):
    """Valid ids of another unique set: (real + rows // 2) % rows (sort=True: ascending, for push keys)."""
    real = np.asarray(real)
    ints = real.astype(np.int64)
    assert real.size > 0 and ints.min() >= 0 and ints.max() < rows, "late ids must be a non-empty batch of ids in range"
    d = (ints + rows // 2) % rows
    if sort:
        d = np.sort(d)
    assert d.min() >= 0 and d.max() < rows
    assert not np.array_equal(np.unique(d), np.unique(ints)), "the decoy names the unique set of the real ids"
    return d.astype(real.dtype).reshape(real.shape)


class LateIds:
    """One gate at a time on the caller's stream (default: torch's current stream of `dev` at each write)."""

    def __init__(self, dev, rows, gates=256):
        self.dev, self.rows = torch.device(dev), int(rows)
        self._L = _lib.load()
        self._flags = torch.zeros(gates, dtype=torch.int32).pin_memory()
        self._np = self._flags.numpy()
        self._next = 0
        self._ev = None
        self._keep = []
        self._timer = None
        self.batches = 0          # late batches written
        self.released = 0         # ... whose gate was found closed behind the call under test

    def pending(self):
        return self._ev is not None

    def write(self, items, stream=None, then=None):
        """items: (buf, real[, sort[, decoy]]) -- buf a preallocated device tensor, real a numpy array of its size (any
        integer or float dtype: converted to buf's); all of them are written late behind ONE gate.  decoy (optional): the
        item's own decoy, a numpy array of the same size (anything that is not an id: offsets, weights, rows of floats -- the
        caller answers for its validity); without it the decoy is decoy_of(real).
        then (optional): called with the stream once behind the decoy writes (before the device is synchronised) and once
        behind the real writes (behind the gate): what a test derives from the late buffers on that stream, a plan for one."""
        assert self._ev is None, "LateIds: the gate of the last write is still closed (release it first)"
        assert self._next < self._np.size
        s = stream if stream is not None else torch.cuda.current_stream(self.dev)
        staged = []
        for it in items:
            buf, real = it[0], np.asarray(it[1])
            sort = len(it) > 2 and bool(it[2])
            assert buf.is_cuda and buf.is_contiguous() and buf.numel() == real.size
            npdt = {torch.float32: np.float32, torch.int64: np.int64, torch.int32: np.int32, torch.uint8: np.uint8}[buf.dtype]
            real = np.ascontiguousarray(real.astype(npdt).reshape(tuple(buf.shape)))
            if len(it) > 3 and it[3] is not None:
                decoy = np.asarray(it[3])
                assert decoy.size == real.size, "an item's own decoy has the size of its real values"
                decoy = np.ascontiguousarray(decoy.astype(npdt).reshape(tuple(buf.shape)))
            else:
                decoy = decoy_of(real, self.rows, sort)
            staged.append((buf, torch.from_numpy(real).to(self.dev), torch.from_numpy(decoy).to(self.dev)))
        with torch.cuda.stream(s):
            for buf, _, decoy in staged:
                buf.copy_(decoy)
            if then is not None:
                then(s)
        torch.cuda.synchronize(self.dev)
        word = self._next
        self._next += 1
        with torch.cuda.device(self.dev):
            _lib.check(self._L.ha_stream_gate(self._flags.data_ptr() + 4 * word, s.cuda_stream), "ha_stream_gate")
        with torch.cuda.stream(s):
            for buf, real, _ in staged:
                buf.copy_(real)
            if then is not None:
                then(s)
            ev = torch.cuda.Event()
            ev.record(s)
        self._ev, self._word, self._keep = ev, word, staged
        self._timer = None
        self.batches += len(staged)

    def open_later(self, delay=DWELL):
        """For a call that is SYNCHRONOUS by contract (it returns a count to the host, so it waits for the caller's stream):
        a timer thread opens the gate `delay` seconds from now, so the call waits out the dwell and not the gate's own
        bound.  Start it just before the call; release_timed() afterwards."""
        assert self._ev is not None and self._timer is None
        state = {"closed_at_fire": None}
        ev, word = self._ev, self._word

        def fire():
            state["closed_at_fire"] = not ev.query()
            self._np[word] = 1

        self._timer = (threading.Timer(delay, fire), state, time.perf_counter(), delay)
        self._timer[0].start()

    def release_timed(self, returned_at=None):
        """After a synchronous call made under open_later(): the gate was still closed when the timer fired (it did not
        run to its bound), and the call did not return before the timer fired (it did wait for the caller's stream).
        returned_at: time.perf_counter() taken right after the call returned (default: now)."""
        assert self._ev is not None and self._timer is not None, "LateIds.release_timed without open_later"
        timer, state, t0, delay = self._timer
        returned_after = (time.perf_counter() if returned_at is None else returned_at) - t0
        timer.join()
        n = len(self._keep)
        self._ev = self._timer = None
        assert state["closed_at_fire"], "the gate had opened before the timer fired (it ran to its bound)"
        assert returned_after >= delay, "a synchronous call returned before the gate was opened: it did not wait for its count"
        self.released += n

    def release(self):
        """After the call under test has returned: the gate is still closed, dwell, still closed, open."""
        assert self._ev is not None, "LateIds.release without a late write"
        ev, n = self._ev, len(self._keep)
        before = ev.query()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < DWELL:
            pass
        after = ev.query()
        self._np[self._word] = 1
        self._ev = None
        assert not before, "the gate had opened before the call under test returned (the call waited on the host for " \
                           "the caller's stream, or the gate ran to its bound)"
        assert not after, "the gate opened during the dwell"
        self.released += n

    def drain(self):
        """Open the gate whatever its state (a test that failed half way leaves no stream held)."""
        if self._ev is not None:
            self._np[self._word] = 1
            self._ev = None
        if self._timer is not None:
            self._timer[0].join()
            self._timer = None

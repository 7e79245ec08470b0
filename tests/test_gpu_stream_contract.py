"""The stream contract (herald_amd/ops.py module docstring) of every row of tests/stream_contract.py, on a side stream S.

Late inputs: every device input of the call is still its DECOY when the call returns -- a gate (tests/late_ids.py) holds S in
front of the copies that write the real values, and is opened 10 ms after the call.  The call must not have waited for S
(LateIds.release), and its result must be the CPU model's on the real inputs: a call that reads an input, or computes an
intermediate, anywhere but on S reads the decoy, and the model of the decoy differs (tests/test_stream_contract_cpu.py).  Once
with stream=S while torch's current stream is the default one, once with stream=None under torch.cuda.stream(S).  The
synchronous rows wait for S by contract: a timer thread opens their gate after the dwell (LateIds.open_later).

Temporaries: while the gate is closed, no block of ANOTHER stream's pool may have become reusable -- read from the caching
allocator's own trace (free_completed events and their stream).  The counter memory_stats()["active_bytes.all.freed"] is read
and reported too, but it cannot carry the assertion: it also counts a temporary allocated while S was current, which the
allocator hands on in S's order only (the controls below show both: the counter moves for a temporary dropped on the wrong
stream and stays for a record_stream'ed one, and so does the trace, which alone tells the pools apart).

History: all rows on one side stream in two fixed orders, so that every one-call form builds its plan in scratch that a larger
and a smaller call of another op wrote last.

Nothing here uses an out-of-range value or an unbounded wait, and nothing needs a fault to fail."""
import contextlib
import time

import numpy as np
import pytest
import torch

import stream_contract as sc
from herald_amd import ops
from late_ids import DWELL, LateIds

pytestmark = pytest.mark.gpu

TORCH_OF = {np.dtype(np.float32): torch.float32, np.dtype(np.int64): torch.int64, np.dtype(np.int32): torch.int32,
            np.dtype(np.uint8): torch.uint8}
CASES = sc.cases()
IDS = ["%s-%s" % (e.name, v.id) for e, v in CASES]
_SIDE = {}


@pytest.fixture
def side(dev):
    """One side stream for the module (the scratch is per stream: the rows then share it, as the calls of a training loop do)."""
    if "s" not in _SIDE:
        _SIDE["s"] = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    yield _SIDE["s"]
    torch.cuda.synchronize()


def _alloc(arrays, dev):
    return {k: torch.empty(a.shape, dtype=TORCH_OF[a.dtype], device=dev) for k, a in arrays.items()}


def _stage(t, arrays, dev):
    for k, a in arrays.items():
        t[k].copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
    torch.cuda.synchronize()


def _compare(entry, v, got, want):
    assert set(got) == set(want), "%s: outputs %s, the model's %s" % (entry.name, sorted(got), sorted(want))
    for k, w in want.items():
        g = got[k].detach().cpu().numpy()
        if entry.name.startswith("dedup_reduce"):      # the reduce writes the first n_unique rows of an n-row output
            g = g[:w.shape[0]]
        assert g.shape == w.shape, "%s %s: shape %s, the model's %s" % (entry.name, k, g.shape, w.shape)
        if entry.atol is not None:
            np.testing.assert_allclose(g, w, rtol=entry.atol, atol=entry.atol, err_msg="%s %s %s" % (entry.name, v.id, k))
        else:
            same = np.ascontiguousarray(g).view(np.uint8).reshape(-1) == np.ascontiguousarray(w.astype(g.dtype)).view(np.uint8).reshape(-1)
            assert same.all(), "%s %s %s: %d of %d bytes differ from the model (first at byte %d)" \
                % (entry.name, v.id, k, int((~same).sum()), same.size, int(np.flatnonzero(~same)[0]))


class _Frees:
    """What the caching allocator did between start() and read(): the two counters, and from its trace the blocks that became
    reusable (free_completed) with the stream of their pool."""

    def __init__(self, dev):
        self.dev = torch.device(dev)

    def start(self):
        st = torch.cuda.memory_stats(self.dev)
        self._c0 = (st["active_bytes.all.freed"], st["allocated_bytes.all.freed"])
        kw = dict(enabled="all", context=None, stacks="python", max_entries=100000)
        try:
            torch.cuda.memory._record_memory_history(clear_history=True, **kw)
        except TypeError:           # (a torch without clear_history: the events before start() are skipped by their count)
            torch.cuda.memory._record_memory_history(**kw)
        self._n0 = len(torch.cuda.memory._snapshot()["device_traces"][self.dev.index or 0])

    def read(self):
        traces = torch.cuda.memory._snapshot()["device_traces"]
        torch.cuda.memory._record_memory_history(enabled=None)
        st = torch.cuda.memory_stats(self.dev)
        self.active_freed = st["active_bytes.all.freed"] - self._c0[0]
        self.allocated_freed = st["allocated_bytes.all.freed"] - self._c0[1]
        trace = traces[self.dev.index or 0][self._n0:]
        self.completed = [(e["stream"], e["size"]) for e in trace if e["action"] == "free_completed"]
        self.requested = [(e["stream"], e["size"]) for e in trace if e["action"] == "free_requested"]
        return self

    def foreign(self, stream):
        """Blocks of a pool other than `stream`'s that became reusable."""
        return [x for x in self.completed if x[0] != stream.cuda_stream]


def _late_case(dev, side, entry, v, current):
    real, decoy = entry.inputs(v), entry.inputs(v, decoy=True)
    want = sc.expected(entry, v)
    t, st = _alloc(real, dev), {}
    arg = None if current else side
    ctx = (lambda: torch.cuda.stream(side)) if current else contextlib.nullcontext
    prep = (lambda s: entry.prep(t, side, st)) if entry.prep is not None else None
    # warm: the same call on inputs of the same sizes (scratch growth synchronises and allocates; not part of the late run)
    _stage(t, real, dev)
    with ctx():
        if prep is not None:
            with torch.cuda.stream(side):
                prep(side)
        entry.call(t, arg, st)
    side.synchronize()
    torch.cuda.synchronize()
    late = LateIds(dev, v.rows, gates=2)
    frees = _Frees(dev)
    try:
        late.write([(t[k], real[k], False, decoy[k]) for k in t], stream=side, then=prep)
        frees.start()
        with ctx():
            if entry.synchronous:
                late.open_later()
                got = entry.call(t, arg, st)
                returned_at = time.perf_counter()
                frees.read()
                late.release_timed(returned_at)
            else:
                got = entry.call(t, arg, st)
                frees.read()                # (the gate is still closed: release() asserts it)
                late.release()
        side.synchronize()
    finally:
        late.drain()
        torch.cuda.memory._record_memory_history(enabled=None)
        side.synchronize()
    print("%s %s: active_bytes.all.freed +%d, allocated_bytes.all.freed +%d, free_completed %s"
          % (entry.name, v.id, frees.active_freed, frees.allocated_freed, frees.completed))
    if not entry.synchronous:       # (a synchronous call's gate has opened by the time it returns)
        assert not frees.foreign(side), \
            "%s: memory of another stream's pool became reusable before S had run the launches of the call: (stream, bytes) %s; " \
            "active_bytes.all.freed moved by %d" % (entry.name, frees.foreign(side), frees.active_freed)
    _compare(entry, v, got, want)
    assert late.released == late.batches == len(t)


@pytest.mark.parametrize("entry,v", CASES, ids=IDS)
def test_late_inputs_explicit_stream(dev, side, entry, v):
    """stream=S while torch's current stream is the default one."""
    assert torch.cuda.current_stream(dev) != side
    _late_case(dev, side, entry, v, current=False)


@pytest.mark.parametrize("entry,v", CASES, ids=IDS)
def test_late_inputs_stream_current(dev, side, entry, v):
    """stream=None under torch.cuda.stream(S)."""
    _late_case(dev, side, entry, v, current=True)


# ---- controls: the harness sees both hazards ----------------------------------------------------------------------------------
def _control_inputs(dev):
    e = sc.BY_NAME["embedding_lookup"]
    v = [x for x in e.variants() if x.ragged][0]
    f32 = lambda a: a.astype(np.float32)
    real, decoy = e.inputs(v), e.inputs(v, decoy=True)
    real, decoy = dict(real, ids=f32(real["ids"])), dict(decoy, ids=f32(decoy["ids"]))
    return v, real, decoy, _alloc(real, dev)


def test_control_an_intermediate_on_the_current_stream_reads_the_decoy(dev, side):
    """A wrapper that computes an intermediate with a torch op on torch's current stream and gathers from it on gated S
    returns the rows of the DECOY ids; the same wrapper under torch.cuda.stream(S) returns the rows of the real ones.
    Whether work on another stream runs while S is held depends on the hardware queues the two streams share (docs/EXPERIMENTS.md,
    round 6, section 12): a current stream that is parked behind the gate itself reads nothing early.  So the unordered leg tries
    the default stream and up to four fresh ones as the current stream, and asserts the decoy for the first one whose
    intermediate is seen to have run while the gate was closed -- there must be one."""
    v, real, decoy, t = _control_inputs(dev)

    def wrapper(stream, fixed):
        with (torch.cuda.stream(stream) if fixed else contextlib.nullcontext()):
            keys = t["ids"].to(torch.int64)                     # the intermediate
            ran = torch.cuda.Event()
            ran.record()
            return ops.embedding_lookup(t["table"], keys, stream=stream), ran

    def leg(current, fixed):
        _stage(t, real, dev)
        late.write([(t[k], real[k], False, decoy[k]) for k in t], stream=side)
        with (torch.cuda.stream(current) if current is not None else contextlib.nullcontext()):
            got, ran = wrapper(side, fixed)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < DWELL:
            pass
        early = ran.query()                 # did the intermediate run while the gate was closed?
        late.release()
        side.synchronize()
        torch.cuda.synchronize()
        return got.cpu().numpy(), early

    rows = lambda a: real["table"][a["ids"].astype(np.int64)]           # (the table is read on S either way)
    assert not np.array_equal(rows(real), rows(decoy))
    high = min(torch.cuda.Stream.priority_range())
    candidates = [None, torch.cuda.Stream(device=dev, priority=high)] + [torch.cuda.Stream(device=dev) for _ in range(3)]
    late = LateIds(dev, v.rows, gates=len(candidates) + 1)
    legs = 0
    try:
        seen = False
        for current in candidates:
            got, early = leg(current, fixed=False)
            legs += 1
            if early:
                np.testing.assert_array_equal(got, rows(decoy))
                seen = True
                break
            # (parked behind the gate: whether it then ran before or after S's copy is not ordered, so nothing is asserted)
        assert seen, "no stream of five ran its work while S was held: the harness cannot see an unordered intermediate here"
        got, early = leg(None, fixed=True)
        legs += 1
        assert not early
        np.testing.assert_array_equal(got, rows(real))
    finally:
        late.drain()
        side.synchronize()
    assert late.released == late.batches == legs * len(t)


def test_control_a_dropped_temporary_moves_the_counter_and_the_trace(dev, side):
    """A wrapper that drops a temporary of torch's current stream while the launch that writes it waits on gated S: the block
    is reusable at once -- active_bytes.all.freed moves and the trace shows a free_completed of the default stream's pool.  With
    the temporary record_stream'ed to S neither moves while the gate is closed.  Allocated while S is current (what ops.on_stream does),
    the counter moves but the block stays in S's pool: the trace names S."""
    v, real, decoy, t = _control_inputs(dev)
    shape = tuple(t["ids"].shape) + (v.width,)
    nbytes = int(np.prod(shape)) * 4

    def wrapper(how):
        with (torch.cuda.stream(side) if how == "on_stream" else contextlib.nullcontext()):
            tmp = torch.empty(shape, dtype=torch.float32, device=dev)
            ops.embedding_lookup(t["table"], t["ids"], out=tmp, stream=side)
            if how == "record_stream":
                tmp.record_stream(side)
            del tmp

    late = LateIds(dev, v.rows, gates=3)
    seen = {}
    try:
        for how in ("dropped", "record_stream", "on_stream"):
            _stage(t, real, dev)
            late.write([(t[k], real[k], False, decoy[k]) for k in t], stream=side)
            frees = _Frees(dev)
            frees.start()
            wrapper(how)
            seen[how] = frees.read()
            late.release()
            side.synchronize()
            torch.cuda.synchronize()
    finally:
        late.drain()
        torch.cuda.memory._record_memory_history(enabled=None)
        side.synchronize()
    print({k: (f.active_freed, f.allocated_freed, f.completed, f.requested) for k, f in seen.items()})
    assert seen["dropped"].active_freed >= nbytes and seen["dropped"].foreign(side)
    assert all(s == 0 for s, _ in seen["dropped"].foreign(side)), "the default stream's pool"
    assert seen["record_stream"].active_freed == 0 and not seen["record_stream"].completed
    assert seen["record_stream"].allocated_freed >= nbytes and seen["record_stream"].requested
    assert seen["on_stream"].active_freed >= nbytes and not seen["on_stream"].foreign(side)
    assert [s for s, _ in seen["on_stream"].completed] == [side.cuda_stream]


# ---- history: every row on scratch that other rows wrote -------------------------------------------------------------------------
def _size(case):
    e, v = case
    return sum(a.nbytes for a in e.inputs(v).values())


def _orders():
    by_size = sorted(range(len(CASES)), key=lambda i: (_size(CASES[i]), i))
    alternating = []
    lo, hi = 0, len(by_size) - 1
    while lo <= hi:                 # the biggest, the smallest, the second biggest, ...: neighbours are different ops
        alternating.append(by_size[hi])
        if lo < hi:
            alternating.append(by_size[lo])
        lo, hi = lo + 1, hi - 1
    return {"ascending": by_size, "alternating": alternating}


@pytest.mark.parametrize("order", ["ascending", "alternating"])
def test_history_on_one_stream(dev, order):
    """All rows on ONE fresh side stream, stream=S, in a fixed order; every result equals the model's.  Ascending: every call
    grows into scratch a smaller call of another op left; alternating: a big and a small call take turns."""
    s = torch.cuda.Stream(device=dev)
    seq = _orders()[order]
    assert sorted(seq) == list(range(len(CASES)))
    assert any(CASES[a][0].name != CASES[b][0].name and CASES[a][1].big != CASES[b][1].big for a, b in zip(seq, seq[1:]))
    pending = []
    for i in seq:
        entry, v = CASES[i]
        real = entry.inputs(v)
        t, st = _alloc(real, dev), {}
        _stage(t, real, dev)
        if entry.prep is not None:
            with torch.cuda.stream(s):
                entry.prep(t, s, st)
        pending.append((entry, v, entry.call(t, s, st), t, st))
        if len(pending) == 8:        # (compared in groups of eight)
            s.synchronize()
            for e2, v2, got, _, _ in pending:
                _compare(e2, v2, got, sc.expected(e2, v2))
            pending = []
    s.synchronize()
    for e2, v2, got, _, _ in pending:
        _compare(e2, v2, got, sc.expected(e2, v2))
    torch.cuda.synchronize()

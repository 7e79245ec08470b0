"""Weighted bags in the PLANNED pairs of the HET cache (csrc/cache_block.hip: ha_cache_lookup_wsum_planned /
ha_cache_update_planned_wbags / ha_cache_run_planned_pairs_wbags) against oracle/cache_model.py + tests/wbag_model.py.

Every step: want_rows = model.lookup(keys); the pooled output equals wbag_model.wbag_sum(want_rows, positions, weights) BIT FOR
BIT; model.update(keys, fl(scale * wbag_grad_rows(...))) with both roundings explicit in float32; the perf counts, the server's
versions and table every step; the whole line state BY BIT VIEW at block ends.  A second cache over a copy of the store runs the
composed calls (embedding_lookup_planned + ops.embedding_lookup_wsum; ops.wbag_grad_rows + scale + embedding_update_planned) and
is compared bit for bit as well.

The weight streams follow the FAE pattern: a share of the slots is dead with the id replaced by the padding id 0, some dead
slots keep their id with weight -0.0f, the live weights come from {1, 0.5, -2}, and id 0 is sometimes live.  What a trace claims
to cover is COUNTED from the CPU model and the ids alone and asserted > 0."""
import numpy as np
import pytest
import torch

import bag_model
import wbag_model
from herald_amd import cache as hcache
from herald_amd import ops
from oracle import cache_model
from test_gpu_cache import _compare_state
from test_gpu_cache_planned import _check_perf, _draw, _setup

pytestmark = pytest.mark.gpu

K_SHORT, K_LONG, K_SCAN = 3, 48, 1024      # scatter_dev.h: kShortRun, kLongRun, kCoopScan


@pytest.fixture(autouse=True)
def _table_registry_as_found():
    before = dict(hcache._TABLES)
    yield
    hcache._TABLES.clear()
    hcache._TABLES.update(before)


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _new_stats():
    return {"dead_head_pulled": 0, "dead_head_pulled_grad": 0, "all_dead_pushed": 0, "mixed_short": 0, "mixed_medium": 0,
            "mixed_long": 0, "mixed_huge": 0, "own_line_evicted": 0, "own_line_evicted_dirty": 0}


def _fae(rng, keys, dead=0.4, neg0=0.1, live0=0.05):
    """The FAE pattern over a drawn key stream -> (keys, weights)."""
    keys = keys.copy()
    n = keys.size
    w = rng.choice(np.array([1.0, 0.5, -2.0], dtype=np.float32), size=n)
    d = rng.random(n) < dead
    keys[d] = 0
    w[d] = 0.0
    z = ~d & (rng.random(n) < neg0)
    w[z] = -0.0                                   # dead, but the id stays
    l0 = rng.random(n) < live0
    keys[l0] = 0                                  # the padding id, live
    w[l0] = rng.choice(np.array([1.0, 0.5, -2.0], dtype=np.float32), size=int(l0.sum()))
    return keys, w.astype(np.float32)


def _positions(n, bag, offsets):
    pos = np.arange(n, dtype=np.int64)
    return (pos.reshape(n // bag, bag), None) if offsets is None else (pos, offsets)


def _which(n, bag, offsets):
    return np.arange(n) // bag if offsets is None else bag_model.bag_of(offsets, n).astype(np.int64)


def _terms(bag_grads, w, which, scale):
    with np.errstate(all="ignore"):
        return (np.float32(scale) * wbag_model.wbag_grad_rows(bag_grads, w, which)).astype(np.float32)


def _count_before_lookup(stats, model, server, keys, w):
    res = model.resident()
    uk, first, cnt = np.unique(keys, return_index=True, return_counts=True)
    for k, f, c in zip(uk.tolist(), first.tolist(), cnt.tolist()):
        ln = res.get(int(k))
        pulled = ln is None or ln.version == -1 or server.ver[int(k)] - ln.version > model.pull_bound
        if pulled and w[f] == 0:
            stats["dead_head_pulled"] += 1
            if ln is not None and ln.grad is not None and np.any(ln.grad != 0):
                stats["dead_head_pulled_grad"] += 1
        live = w[keys == k] != 0
        if live.any() and not live.all():
            stats["mixed_short" if c <= K_SHORT else "mixed_medium" if c < K_LONG else "mixed_long"] += 1
            if c > K_SCAN:
                stats["mixed_huge"] += 1
    return res


class _Trace:
    """A cache held to the model, and (twin) a second cache over a copy of the store that runs the composed calls."""

    def __init__(self, dev, limit, rows, width, nmax, pull_bound, push_bound, seed, policy="lru", twin=True):
        self.dev, self.width, self.rows = dev, width, rows
        self.rng, self.server, self.model, self.table, self.versions, self.gpu = _setup(dev, limit, rows, width, nmax, pull_bound,
                                                                                         push_bound, seed, policy)
        self.stats = _new_stats()
        self.all_dead = set()
        self.twin = None
        if twin:
            cls = {"lru": hcache.LRUCache, "lfu": hcache.LFUCache, "lfuopt": hcache.LFUOptCache}[policy]
            t = self.table.clone()
            v = torch.zeros(rows, dtype=torch.int64, device=dev)
            c = cls(limit, rows, width, node_id=0, max_batch=max(nmax, 64), device=dev)
            c.bind_store(t, v)
            c.pull_bound, c.push_bound = pull_bound, push_bound
            self.twin = (c, t, v)

    def plan(self, kts, **kw):
        self.gpu.plan_block(kts, **kw)
        if self.twin:
            self.twin[0].plan_block(kts, **kw)

    def step(self, keys, w, bag_grads, scale, step, bag=None, offsets=None, pk=False, lookup="w", update="w"):
        """One planned pair.  lookup / update: "w" the weighted call, "u" the unpooled call composed with the ops."""
        dev, width, gpu, model = self.dev, self.width, self.gpu, self.model
        n = keys.size
        off_t = None if offsets is None else torch.from_numpy(np.asarray(offsets, dtype=np.int64)).to(dev)
        res = _count_before_lookup(self.stats, model, self.server, keys, w)
        held = {int(k): res[int(k)].updates for k in np.unique(keys) if int(k) in res}
        want_rows = model.lookup(keys.astype(np.uint64)).reshape(n, width)
        gone = [k for k in held if not model.policy.count(k)]
        self.stats["own_line_evicted"] += len(gone)
        self.stats["own_line_evicted_dirty"] += sum(1 for k in gone if held[k] != 0)
        pos, off = _positions(n, bag, offsets)
        want = wbag_model.wbag_sum(want_rows, pos, w, off) if n else np.zeros((0 if offsets is None else len(offsets) - 1, width),
                                                                              dtype=np.float32)
        nbags = want.shape[0]
        wt = torch.from_numpy(w).to(dev)
        pos_t = torch.arange(n, dtype=torch.int64, device=dev)
        pos_t = pos_t.reshape(nbags, bag) if offsets is None else pos_t

        def composed_lookup(c):
            rows_t = torch.empty((n, width), dtype=torch.float32, device=dev)
            c.embedding_lookup_planned(rows_t).wait()
            if n == 0:
                return rows_t, torch.zeros((nbags, width), dtype=torch.float32, device=dev)
            return rows_t, ops.embedding_lookup_wsum(rows_t, pos_t, wt.reshape(pos_t.shape), offsets=off_t)

        if lookup == "w":
            out = torch.full((nbags, width), float("nan"), dtype=torch.float32, device=dev)
            gpu.embedding_lookup_wsum_planned(out, wt, bag=bag, offsets=off_t).wait()
        else:
            rows_t, out = composed_lookup(gpu)
            np.testing.assert_array_equal(_bits(rows_t), _bits(want_rows), err_msg="unpooled lookup rows at step %d" % step)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_bits(out), _bits(want), err_msg="weighted pooled rows at step %d" % step)
        which = _which(n, bag, offsets)
        terms = _terms(bag_grads, w, which, scale)
        uk = np.unique(keys)
        self.all_dead |= {int(k) for k in uk if not (w[keys == k] != 0).any()}
        ver_before = self.server.ver.copy()
        if pk is False:
            model.update(keys.astype(np.uint64), terms)
        else:
            model.update_with_push_keys(keys.astype(np.uint64), pk.astype(np.uint64), terms)
        pushed = {k for k in self.all_dead if self.server.ver[k] > ver_before[k]}
        self.stats["all_dead_pushed"] += len(pushed)
        self.all_dead -= pushed
        g = torch.from_numpy(np.ascontiguousarray(bag_grads)).to(dev)
        bof = None if offsets is None else ops.bag_of(off_t, n)

        def composed_update(c):
            if n == 0:
                c.embedding_update_planned(torch.empty((0, width), dtype=torch.float32, device=dev)).wait()
                return
            gr = ops.wbag_grad_rows(g, wt.reshape(pos_t.shape), bag=bag, bag_of=bof) if offsets is None else \
                ops.wbag_grad_rows(g, wt, bag_of=bof)
            gr = gr.reshape(n, width)
            gr.mul_(float(scale))
            c.embedding_update_planned(gr).wait()

        if update == "w":
            gpu.embedding_update_planned_wbags(g, wt, bag=bag, bag_of=bof, scale=scale).wait()
        else:
            composed_update(gpu)
        _check_perf(gpu, model, step)
        np.testing.assert_array_equal(self.versions.cpu().numpy(), self.server.ver, err_msg="server versions step %d" % step)
        np.testing.assert_array_equal(_bits(self.table), _bits(self.server.table), err_msg="server table step %d" % step)
        if self.twin:
            c = self.twin[0]
            _, out2 = composed_lookup(c)
            composed_update(c)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(_bits(out2), _bits(out), err_msg="composed / fused output at step %d" % step)
        return out

    def block_end(self, step):
        assert self.gpu.plan_pending() == 0
        _compare_state(self.gpu, self.model, step)
        _state_bits(self.gpu, self.model, step)
        if self.twin:
            c, t, v = self.twin
            np.testing.assert_array_equal(_bits(t), _bits(self.table), err_msg="composed / fused store at step %d" % step)
            assert torch.equal(v, self.versions)
            _lines_equal(c, self.gpu, "composed / fused lines at step %d" % step)


def _state_bits(gpu, model, step):
    res, lines = model.resident(), gpu.lines()
    for k, ln in res.items():
        np.testing.assert_array_equal(_bits(lines[k].data), _bits(ln.data), err_msg="data bits of key %d at step %d" % (k, step))
        if ln.grad is not None:
            np.testing.assert_array_equal(_bits(lines[k].grad), _bits(ln.grad), err_msg="grad bits of key %d at step %d" % (k, step))


def _lines_equal(a, b, what):
    la, lb = a.lines(), b.lines()
    assert sorted(la) == sorted(lb), what
    for k in la:
        assert la[k].version == lb[k].version and la[k].updates == lb[k].updates, (what, k)
        np.testing.assert_array_equal(_bits(la[k].data), _bits(lb[k].data), err_msg="%s: data of key %d" % (what, k))
        np.testing.assert_array_equal(_bits(la[k].grad), _bits(lb[k].grad), err_msg="%s: grad of key %d" % (what, k))


def _run(dev, limit, rows, width, B, F, steps, pull_bound, push_bound, block, seed, scale, zipf=True, ahead=True, policy="lru",
         twin=True, shape=None):
    n = B * F
    tr = _Trace(dev, limit, rows, width, n, pull_bound, push_bound, seed, policy, twin=twin)
    rng = tr.rng
    streams = [(shape or _fae)(rng, _draw(rng, n, rows, zipf)) for _ in range(steps)]     # the whole stream before any gradient
    kts = [torch.from_numpy(k.astype(np.float32)).to(dev) for k, _ in streams]
    blocks = [list(range(b0, min(b0 + block, steps))) for b0 in range(0, steps, block)]
    if ahead:
        tr.plan([kts[s] for s in blocks[0]])
    for j, blk in enumerate(blocks):
        if ahead and j + 1 < len(blocks):
            tr.plan([kts[s] for s in blocks[j + 1]])
        elif not ahead:
            tr.plan([kts[s] for s in blk])
        for step in blk:
            bag_grads = rng.standard_normal((B, width), dtype=np.float32)
            tr.step(streams[step][0], streams[step][1], bag_grads, scale, step, bag=F)
        if not ahead or j + 1 == len(blocks):
            tr.block_end(blk[-1])
    assert tr.gpu.size() == tr.model.policy.size()
    return tr


# ---- 1. small traces --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pull_bound,push_bound", [(0, 0), (1, 3), (100, 100)])
@pytest.mark.parametrize("block,ahead,scale", [(1, False, 1.0), (4, False, -0.01), (16, True, 0.01), (5, True, -0.01)])
def test_weighted_lru_trace_small(dev, pull_bound, push_bound, block, ahead, scale):
    tr = _run(dev, limit=100, rows=1500, width=8, B=16, F=4, steps=32, pull_bound=pull_bound, push_bound=push_bound, block=block,
              seed=11, scale=scale, ahead=ahead)
    st = tr.stats
    assert st["dead_head_pulled"] > 0 and st["mixed_short"] > 0 and st["mixed_medium"] > 0, st
    if push_bound < 100:
        assert st["all_dead_pushed"] > 0, st


@pytest.mark.parametrize("policy", ["lfu", "lfuopt"])
@pytest.mark.parametrize("limit", [7, 64])
@pytest.mark.parametrize("scale", [1.0, -0.01])
def test_weighted_lfu_cache_smaller_than_the_batch(dev, policy, limit, scale):
    tr = _run(dev, limit=limit, rows=300, width=8, B=16, F=4, steps=40, pull_bound=1, push_bound=3, block=4, seed=5 + limit,
              scale=scale, ahead=False, policy=policy)
    st = dict(tr.stats)
    tr = _run(dev, limit=limit, rows=300, width=8, B=16, F=4, steps=40, pull_bound=1, push_bound=0, block=16, seed=6 + limit,
              scale=scale, zipf=False, ahead=True, policy=policy)
    for k in st:
        st[k] += tr.stats[k]
    assert st["dead_head_pulled"] > 0 and st["all_dead_pushed"] > 0 and st["mixed_short"] > 0 and st["mixed_medium"] > 0, st
    if limit == 7:      # (the FAE pattern moves 45 % of the slots to id 0: at limit 64 no batch evicts a line of its own)
        assert st["own_line_evicted"] > 0 and st["own_line_evicted_dirty"] > 0, st


@pytest.mark.parametrize("policy", ["lfu", "lfuopt"])
@pytest.mark.parametrize("block,ahead,scale", [(1, False, 0.01), (16, True, -0.01), (5, True, 1.0)])
def test_weighted_lfu_trace_small(dev, policy, block, ahead, scale):
    tr = _run(dev, limit=100, rows=1500, width=8, B=16, F=4, steps=32, pull_bound=1, push_bound=3, block=block, seed=12,
              scale=scale, ahead=ahead, policy=policy)
    assert tr.stats["dead_head_pulled"] > 0, tr.stats


# ---- 1b. a stale line with a gradient buffer whose head occurrence is dead ------------------------------------------------------
@pytest.mark.parametrize("policy", ["lru", "lfu"])
def test_dead_head_of_a_stale_line_with_a_gradient_buffer(dev, policy):
    """Between steps another worker pushes to store rows the cache holds (push_bound 10,000: the lines keep their gradient
    buffers).  The next batch names such keys with a DEAD first occurrence (weight +0 / -0.0f) and live later ones: the line is
    refreshed with the unweighted store row + gradient row and its version staged all the same."""
    limit, rows, width, B, F = 200, 600, 8, 24, 4
    n = B * F
    tr = _Trace(dev, limit, rows, width, n, 2, 10000, 51, policy)
    rng, server, model = tr.rng, tr.server, tr.model
    streams = [_fae(rng, _draw(rng, n, rows, True), dead=0.2) for _ in range(8)]
    for step in (3, 6):
        keys, w = streams[step]
        prev_k, prev_w = streams[step - 1]
        stale = np.unique(prev_k[(prev_w != 0) & (prev_k != 0)])[:3]      # resident after the step before, gradient not zero
        for t, k in enumerate(stale):
            for at, wv in (((2 + t) * F + 1, [0.0, -0.0, 0.0][t]), ((5 + t) * F + 3, 0.5), ((15 + t) * F + 2, 1.0)):
                keys[at], w[at] = k, wv
        first = [int(np.nonzero(keys == k)[0][0]) for k in stale]
        assert all(w[f] == 0 for f in first)
    kts = [torch.from_numpy(k.astype(np.float32)).to(dev) for k, _ in streams]
    tr.plan(kts)
    torch.cuda.synchronize()
    for step in range(8):
        if step in (3, 6):
            prev_k, prev_w = streams[step - 1]
            stale = np.unique(prev_k[(prev_w != 0) & (prev_k != 0)])[:3]
            delta = rng.standard_normal((stale.size, width), dtype=np.float32)
            server.ver[stale] += 4
            server.table[stale] = (server.table[stale] + delta).astype(np.float32)
            for c_t, c_v in [(tr.table, tr.versions), (tr.twin[1], tr.twin[2])]:
                c_v[torch.from_numpy(stale).to(dev)] += 4
                c_t[torch.from_numpy(stale).to(dev)] += torch.from_numpy(delta).to(dev)
        bag_grads = rng.standard_normal((B, width), dtype=np.float32)
        tr.step(streams[step][0], streams[step][1], bag_grads, 0.01, step, bag=F)
    tr.block_end(7)
    assert tr.stats["dead_head_pulled_grad"] >= 6, tr.stats


# ---- 2. run lengths: short, medium, long and beyond 1,024 sorted positions ---------------------------------------------------
def _run_length_shape(rng, keys):
    """75 % of the slots dead on id 0 (a run beyond 1,024 positions) with a few LIVE occurrences of id 0 among them; a second
    heavy key with ~60 occurrences and keys with 2 .. 16 occurrences, live and dead (-0.0f, id kept) mixed."""
    keys = keys.copy()
    n = keys.size
    w = rng.choice(np.array([1.0, 0.5, -2.0], dtype=np.float32), size=n)
    d = rng.random(n) < 0.75
    keys[d] = 0
    w[d] = 0.0
    free = np.nonzero(~d)[0]
    rng.shuffle(free)
    at = 0
    for key, cnt in [(4321, 60)] + [(100 + c, c) for c in (2, 3, 5, 9, 16)]:
        idx = free[at:at + cnt]
        at += cnt
        keys[idx] = key
        w[idx[::3]] = -0.0
    l0 = np.nonzero(d)[0][::97]
    w[l0] = 0.5                                   # id 0, live
    return keys, w.astype(np.float32)


@pytest.mark.parametrize("width", [8, 6, 200])
@pytest.mark.parametrize("policy,scale", [("lru", -0.01), ("lfu", 1.0)])
def test_weighted_run_lengths(dev, width, policy, scale):
    tr = _run(dev, limit=2048, rows=5000, width=width, B=64, F=26, steps=6, pull_bound=1, push_bound=2, block=3, seed=31,
              scale=scale, zipf=False, policy=policy, shape=_run_length_shape)
    st = tr.stats
    assert st["mixed_short"] > 0 and st["mixed_medium"] > 0 and st["mixed_long"] > 0 and st["mixed_huge"] > 0, st


@pytest.mark.parametrize("width,policy,scale", [(520, "lru", -0.01), (1040, "lfu", 1.0), (70, "lfu", -0.01), (130, "lru", 1.0)])
def test_weighted_run_lengths_over_several_column_slices(dev, width, policy, scale):
    """The weighted accumulate's slice is 64 * VEC columns: widths 520 and 1,040 are 3 and 5 slices of the 16-byte path, 70 and
    130 are 2 and 3 slices of the scalar path, each with a partial last slice.  A run's first min(run, slices) waves are its
    workers -- waves at an offset > 0, reading the record of a position that is not the run's head, striding over the slices --
    for short, medium and long runs and the run beyond 1,024 positions alike (a run of 2 has fewer workers than slices)."""
    tr = _run(dev, limit=2048, rows=5000, width=width, B=64, F=26, steps=4, pull_bound=1, push_bound=2, block=2, seed=33,
              scale=scale, zipf=False, policy=policy, shape=_run_length_shape)
    st = tr.stats
    assert st["mixed_short"] > 0 and st["mixed_medium"] > 0 and st["mixed_long"] > 0 and st["mixed_huge"] > 0, st
    assert st["dead_head_pulled"] > 0, st


@pytest.mark.parametrize("width,F", [(256, 2), (128, 2), (256, 9), (128, 9)])
def test_weighted_lookup_in_its_wide_instantiations(dev, width, F):
    """2,048 bags: the pooled lookup's launch takes 16-byte (width 256) and 8-byte (width 128) column slices, with 8 (bags of
    2) and 32 (bags of 9) rows in flight -- the four weighted instantiations the smaller traces never launch."""
    tr = _run(dev, limit=30000, rows=20000, width=width, B=2048, F=F, steps=2, pull_bound=0, push_bound=1, block=2, seed=34,
              scale=-0.01, zipf=True)
    assert tr.stats["dead_head_pulled"] > 0 and tr.stats["mixed_short"] > 0, tr.stats


def test_weighted_run_lengths_all_dead_padding_run(dev):
    """The padding id's run holds no live occurrence at all: one scan, one add of z (the dead-run shortcut)."""
    def shape(rng, keys):
        k, w = _run_length_shape(rng, keys)
        w[k == 0] = 0.0
        return k, w
    tr = _run(dev, limit=2048, rows=5000, width=200, B=64, F=26, steps=4, pull_bound=0, push_bound=1, block=2, seed=32,
              scale=-0.01, zipf=False, shape=shape)
    assert tr.stats["all_dead_pushed"] > 0 and tr.stats["mixed_long"] > 0, tr.stats


# ---- 3. ragged bags, empty batches ---------------------------------------------------------------------------------------------
def _ragged_offsets(rng, n):
    cuts = np.sort(rng.integers(0, n + 1, size=5)).tolist()
    return np.array([0, 0] + cuts[:3] + [cuts[2]] + cuts[3:] + [n, n], dtype=np.int64)


@pytest.mark.parametrize("policy", ["lru", "lfu"])
def test_weighted_ragged_bags_and_empty_batches(dev, policy):
    sizes = [64, 1, 0, 33, 64, 0, 0, 17, 64, 2]
    width, rows = 8, 700
    tr = _Trace(dev, 100, rows, width, 64, 1, 1, 9, policy)
    rng = tr.rng
    streams = [_fae(rng, _draw(rng, m, rows, True)) for m in sizes]
    kts = [torch.from_numpy(k.astype(np.int64)).to(dev) for k, _ in streams]
    offs = [_ragged_offsets(rng, m) for m in sizes]
    offs[4] = np.array([0, 64], dtype=np.int64)
    for b0 in range(0, len(sizes), 4):
        blk = list(range(b0, min(b0 + 4, len(sizes))))
        tr.plan([kts[s] for s in blk])
        for step in blk:
            bag_grads = rng.standard_normal((offs[step].size - 1, width), dtype=np.float32)
            tr.step(streams[step][0], streams[step][1], bag_grads, -0.01, step, offsets=offs[step])
        tr.block_end(blk[-1])


# ---- 4. push keys ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["lru", "lfu"])
def test_weighted_pairs_of_batches_planned_with_push_keys(dev, policy):
    limit, rows, width, B, F, steps, block = 100, 1500, 8, 16, 4, 24, 4
    n = B * F
    tr = _Trace(dev, limit, rows, width, n, 2, 2, 71, policy)
    rng = tr.rng
    streams = [_fae(rng, _draw(rng, n, rows, True)) for _ in range(steps)]
    pks = []
    for s, (k, _) in enumerate(streams):
        u = np.unique(k.astype(np.int64))
        pks.append(None if s == 5 else np.sort(rng.choice(u, size=max(1, u.size // 3), replace=False)))
    kts = [torch.from_numpy(k.astype(np.float32)).to(dev) for k, _ in streams]
    pts = [None if p is None else torch.from_numpy(p.astype(np.float32)).to(dev) for p in pks]
    for b0 in range(0, steps, block):
        tr.plan(kts[b0:b0 + block], push_keys_list=pts[b0:b0 + block])
        for step in range(b0, b0 + block):
            bag_grads = rng.standard_normal((B, width), dtype=np.float32)
            tr.step(streams[step][0], streams[step][1], bag_grads, -0.01, step, bag=F, pk=False if pks[step] is None else pks[step])
        tr.block_end(b0 + block - 1)
    assert tr.stats["dead_head_pulled"] > 0, tr.stats


# ---- 5. all-ones weights: the sum-pooled calls, bit for bit ---------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["lru", "lfu"])
def test_all_ones_weights_equal_the_sum_pooled_calls(dev, policy):
    limit, rows, width, B, F, steps, block = 100, 1500, 8, 16, 4, 16, 4
    n = B * F
    rng = np.random.default_rng(13)
    table0 = rng.standard_normal((rows, width), dtype=np.float32)
    cls = {"lru": hcache.LRUCache, "lfu": hcache.LFUCache}[policy]
    caches = []
    for _ in range(2):
        t = torch.from_numpy(table0.copy()).to(dev)
        v = torch.zeros(rows, dtype=torch.int64, device=dev)
        c = cls(limit, rows, width, node_id=0, max_batch=n, device=dev)
        c.bind_store(t, v)
        c.pull_bound, c.push_bound = 1, 3
        caches.append((c, t, v))
    kts = [torch.from_numpy(_draw(rng, n, rows, True).astype(np.float32)).to(dev) for _ in range(steps)]
    ones = torch.ones((B, F), dtype=torch.float32, device=dev)
    for b0 in range(0, steps, block):
        for c, _, _ in caches:
            c.plan_block(kts[b0:b0 + block])
        for step in range(b0, b0 + block):
            g = torch.from_numpy(rng.standard_normal((B, width), dtype=np.float32) * np.float32(-0.01)).to(dev)
            o0 = torch.empty((B, width), dtype=torch.float32, device=dev)
            o1 = torch.empty((B, width), dtype=torch.float32, device=dev)
            caches[0][0].embedding_lookup_sum_planned(o0, bag=F).wait()
            caches[0][0].embedding_update_planned_bags(g, bag=F).wait()
            caches[1][0].embedding_lookup_wsum_planned(o1, ones, bag=F).wait()
            caches[1][0].embedding_update_planned_wbags(g, ones, bag=F, scale=1.0).wait()
            torch.cuda.synchronize()
            np.testing.assert_array_equal(_bits(o0), _bits(o1), err_msg="step %d" % step)
        np.testing.assert_array_equal(_bits(caches[0][1]), _bits(caches[1][1]))
        assert torch.equal(caches[0][2], caches[1][2])
        _lines_equal(caches[0][0], caches[1][0], "after the block at %d" % b0)


# ---- 6. mixed forms within a block ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["lru", "lfu"])
def test_mixed_forms_within_a_block(dev, policy):
    """Weighted / sum-pooled / unpooled lookup and update in every combination: the model is told what each call means."""
    limit, rows, width, B, F, block = 100, 1500, 8, 16, 4, 9
    n = B * F
    tr = _Trace(dev, limit, rows, width, n, 1, 3, 17, policy, twin=False)
    rng, gpu, model = tr.rng, tr.gpu, tr.model
    forms = [(a, b) for a in "wsu" for b in "wsu"]
    for rnd in range(2):
        streams = [_fae(rng, _draw(rng, n, rows, True)) for _ in range(block)]
        gpu.plan_block([torch.from_numpy(k.astype(np.float32)).to(dev) for k, _ in streams])
        for j, (fl, fu) in enumerate(forms):
            keys, w = streams[j]
            step = rnd * block + j
            bag_grads = rng.standard_normal((B, width), dtype=np.float32)
            if fl == "s" or fu == "s":
                # a sum-pooled call is the weighted one with all-ones weights: held to the model on its own terms
                ones = np.ones(n, dtype=np.float32)
                want_rows = model.lookup(keys.astype(np.uint64)).reshape(n, width)
                wl = ones if fl == "s" else w
                want = wbag_model.wbag_sum(want_rows, np.arange(n).reshape(B, F), wl)
                out = torch.empty((B, width), dtype=torch.float32, device=dev)
                wt = torch.from_numpy(w).to(dev)
                if fl == "s":
                    gpu.embedding_lookup_sum_planned(out, bag=F).wait()
                elif fl == "w":
                    gpu.embedding_lookup_wsum_planned(out, wt, bag=F).wait()
                else:
                    rows_t = torch.empty((n, width), dtype=torch.float32, device=dev)
                    gpu.embedding_lookup_planned(rows_t).wait()
                    out = ops.embedding_lookup_wsum(rows_t, torch.arange(n, device=dev).reshape(B, F), wt.reshape(B, F))
                torch.cuda.synchronize()
                np.testing.assert_array_equal(_bits(out), _bits(want), err_msg="step %d" % step)
                wu = ones if fu == "s" else w
                terms = _terms(bag_grads, wu, np.arange(n) // F, -0.01 if fu != "s" else 1.0)
                model.update(keys.astype(np.uint64), terms)
                g = torch.from_numpy(bag_grads).to(dev)
                if fu == "s":
                    gpu.embedding_update_planned_bags(g, bag=F).wait()
                elif fu == "w":
                    gpu.embedding_update_planned_wbags(g, wt, bag=F, scale=-0.01).wait()
                else:
                    gpu.embedding_update_planned(torch.from_numpy(terms).to(dev)).wait()
                _check_perf(gpu, model, step)
                np.testing.assert_array_equal(_bits(tr.table), _bits(tr.server.table), err_msg="server table step %d" % step)
            else:
                tr.step(keys, w, bag_grads, -0.01, step, bag=F, lookup=fl, update=fu)
        tr.block_end(rnd * block + block - 1)


# ---- 7. the -0.0f pin -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, -1.0])
@pytest.mark.parametrize("push_bound", [100, 0])
def test_minus_zero_rows_under_dead_and_minus_zero_terms(dev, scale, push_bound):
    """Store rows that hold -0.0f elements, (i) under a key all of whose occurrences are dead and (ii) under a key whose only
    live terms are -0.0f (gradient elements +-0): data rows, gradient rows and pushed store rows by bit view.  With z = +0 a
    -0 data element turns +0; with z = -0 it stays."""
    rows, width, B, F = 64, 8, 4, 4
    n = B * F
    tr = _Trace(dev, 32, rows, width, n, 0, push_bound, 3, "lru")
    mz = np.float32(-0.0)
    for k in (5, 6, 7):
        tr.server.table[k, ::2] = mz
    tr.table.copy_(torch.from_numpy(tr.server.table))
    tr.twin[1].copy_(tr.table)
    assert np.signbit(tr.server.table[5, 0]) and tr.server.table[5, 0] == 0
    keys = np.array([5, 5, 6, 9, 6, 7, 9, 10, 5, 7, 11, 12, 13, 6, 14, 15], dtype=np.int64)
    w = np.ones(n, dtype=np.float32)
    w[keys == 5] = 0.0                      # (i) all dead
    w[1] = mz
    w[keys == 7] = 0.0                      # all dead, one occurrence -0.0f
    w[9] = mz
    bag_grads = tr.rng.standard_normal((B, width), dtype=np.float32)
    for j in np.nonzero(keys == 6)[0]:      # (ii) key 6: live, but every term it meets is -0 * scale'
        bag_grads[j // F, :] = mz if scale > 0 else np.float32(0.0)
    # (bags that hold key 6 hold other keys too: their terms are zero as well, which is fine)
    kt = torch.from_numpy(keys.astype(np.float32)).to(dev)
    for step in range(3):
        tr.plan([kt])
        tr.step(keys, w, bag_grads, scale, step, bag=F)
        tr.block_end(step)
    res = tr.model.resident()
    # the model itself shows the effect the kernel must reproduce
    assert np.signbit(res[5].data[0]) == (scale < 0)
    if push_bound == 0:
        assert tr.stats["all_dead_pushed"] > 0


# ---- 8. non-finite gradients under dead occurrences only ------------------------------------------------------------------------
def test_inf_and_nan_gradient_rows_under_dead_occurrences_only(dev):
    rows, width, B, F = 400, 8, 8, 4
    n = B * F
    tr = _Trace(dev, 64, rows, width, n, 0, 1, 4, "lfu")
    rng = tr.rng
    for step in range(4):
        keys = _draw(rng, n, rows, True)
        w = rng.choice(np.array([1.0, 0.5, -2.0], dtype=np.float32), size=n).astype(np.float32)
        w.reshape(B, F)[1::2] = 0.0          # every other bag is dead throughout ...
        w.reshape(B, F)[3, 0] = -0.0
        bag_grads = rng.standard_normal((B, width), dtype=np.float32)
        bag_grads[1::4] = np.inf             # ... and its gradient row is not finite
        bag_grads[3::4] = np.nan
        tr.plan([torch.from_numpy(keys.astype(np.float32)).to(dev)])
        tr.step(keys, w, bag_grads, -0.01, step, bag=F)
        tr.block_end(step)
    assert np.isfinite(tr.table.cpu().numpy()).all()
    for ln in tr.gpu.lines().values():
        assert np.isfinite(ln.data).all() and np.isfinite(ln.grad).all()


# ---- 9. run_planned_pairs_wbags ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["lru", "lfuopt"])
def test_run_planned_pairs_wbags_equals_the_per_call_methods(dev, policy):
    limit, rows, width, B, F, block = 100, 1500, 8, 16, 4, 4
    n = B * F
    rng = np.random.default_rng(21)
    table0 = rng.standard_normal((rows, width), dtype=np.float32)
    cls = {"lru": hcache.LRUCache, "lfuopt": hcache.LFUOptCache}[policy]
    pair = []
    for _ in range(2):
        t = torch.from_numpy(table0.copy()).to(dev)
        v = torch.zeros(rows, dtype=torch.int64, device=dev)
        c = cls(limit, rows, width, node_id=0, max_batch=n, device=dev)
        c.bind_store(t, v)
        c.pull_bound, c.push_bound = 2, 2
        pair.append((c, t, v))
    for blk in range(2):
        streams = [_fae(rng, _draw(rng, n, rows, True)) for _ in range(block)]
        kts = [torch.from_numpy(k.astype(np.float32)).to(dev) for k, _ in streams]
        ws = [torch.from_numpy(w).to(dev).reshape(B, F) for _, w in streams]
        gs = [torch.from_numpy(rng.standard_normal((B, width), dtype=np.float32)).to(dev) for _ in range(block)]
        outs = [[torch.empty((B, width), dtype=torch.float32, device=dev) for _ in range(block)] for _ in range(2)]
        for c, _, _ in pair:
            c.plan_block(kts)
        for k in range(block):
            pair[0][0].embedding_lookup_wsum_planned(outs[0][k], ws[k], bag=F)
            pair[0][0].embedding_update_planned_wbags(gs[k], ws[k], bag=F, scale=-0.01)
        pair[1][0].run_planned_pairs_wbags(outs[1], gs, ws, F, scale=-0.01)
        torch.cuda.synchronize()
        assert pair[0][0].plan_pending() == 0 and pair[1][0].plan_pending() == 0
        for k in range(block):
            np.testing.assert_array_equal(_bits(outs[0][k]), _bits(outs[1][k]), err_msg="block %d pair %d" % (blk, k))
        np.testing.assert_array_equal(_bits(pair[0][1]), _bits(pair[1][1]))
        assert torch.equal(pair[0][2], pair[1][2])
        _lines_equal(pair[0][0], pair[1][0], "block %d" % blk)


# ---- 10. refusals -------------------------------------------------------------------------------------------------------------------
def test_weighted_calls_refuse_misuse_and_leave_the_cache_untouched(dev):
    limit, rows, width, B, F = 200, 1500, 8, 16, 4
    n = B * F
    tr = _Trace(dev, limit, rows, width, n, 2, 2, 61, twin=False)
    rng, gpu, model = tr.rng, tr.gpu, tr.model
    streams = [_fae(rng, _draw(rng, n, rows, True)) for _ in range(3)]
    kts = [torch.from_numpy(k.astype(np.float32)).to(dev) for k, _ in streams]
    out = torch.empty((B, width), dtype=torch.float32, device=dev)
    g = torch.zeros((B, width), dtype=torch.float32, device=dev)
    wt = torch.from_numpy(streams[0][1]).to(dev)
    off = torch.arange(0, n + 1, F, dtype=torch.int64, device=dev)
    bof = ops.bag_of(off, n)
    gpu.plan_block(kts[:2])
    pending = gpu.plan_pending()
    table_before = tr.table.clone()
    torch.cuda.synchronize()            # (the block's bookkeeping has run: the line state below is what the row launches see)

    def state():
        snap = gpu._snapshot()
        order = np.argsort(snap["keys"])
        return [np.asarray(snap[f])[order].tolist() for f in ("keys", "version", "updates", "slots")] + \
               [tr.versions.cpu().numpy().tolist()]

    state_before = [state()]

    def refused(exc, fn, *a, **kw):
        with pytest.raises(exc):
            fn(*a, **kw)
        assert gpu.plan_pending() == pending
        assert state() == state_before[0]
        assert torch.equal(tr.table, table_before)

    both = (ValueError, RuntimeError)
    refused(TypeError, gpu.embedding_lookup_wsum_planned, out, wt.double(), bag=F)
    refused(ValueError, gpu.embedding_lookup_wsum_planned, out, wt[:-1], bag=F)
    refused(both, gpu.embedding_lookup_wsum_planned, out, wt, bag=F, offsets=off)
    refused(both, gpu.embedding_lookup_wsum_planned, out, wt)
    refused(both, gpu.embedding_lookup_wsum_planned, out, wt, bag=F + 1)
    refused(both, gpu.embedding_update_planned_wbags, g, wt, bag=F)                    # an update before its lookup
    L, h, s = gpu._L, gpu._h, gpu._stream().cuda_stream
    assert L.ha_cache_lookup_wsum_planned(h, n, B, F + 1, None, wt.data_ptr(), out.data_ptr(), s) == -1
    assert L.ha_cache_lookup_wsum_planned(h, n, B, F, off.data_ptr(), wt.data_ptr(), out.data_ptr(), s) == -1
    assert L.ha_cache_lookup_wsum_planned(h, n, B, F, None, None, out.data_ptr(), s) == -1
    assert L.ha_cache_update_planned_wbags(h, n, g.data_ptr(), wt.data_ptr(), 1.0, B, F, None, s) == -1
    assert gpu.plan_pending() == pending
    tr.step(streams[0][0], streams[0][1], rng.standard_normal((B, width), dtype=np.float32), -0.01, 0, bag=F)
    table_before = tr.table.clone()
    state_before[0] = state()
    want_rows = model.lookup(streams[1][0].astype(np.uint64)).reshape(n, width)
    w1 = torch.from_numpy(streams[1][1]).to(dev)
    gpu.embedding_lookup_wsum_planned(out, w1, bag=F).wait()
    np.testing.assert_array_equal(_bits(out), _bits(wbag_model.wbag_sum(want_rows, np.arange(n).reshape(B, F), streams[1][1])))
    pending = gpu.plan_pending()
    state_before[0] = state()
    refused(TypeError, gpu.embedding_update_planned_wbags, g, w1.double(), bag=F)
    refused(ValueError, gpu.embedding_update_planned_wbags, g, w1[:-1], bag=F)
    refused(both, gpu.embedding_update_planned_wbags, g, w1, bag=F, bag_of=bof)
    refused(both, gpu.embedding_update_planned_wbags, g, w1)
    refused(both, gpu.embedding_update_planned_wbags, g, w1, bag=F, scale=float("inf"))
    refused(both, gpu.embedding_lookup_wsum_planned, out, w1, bag=F)                   # the update is due
    assert L.ha_cache_update_planned_wbags(h, n, g.data_ptr(), w1.data_ptr(), float("nan"), B, F, None, s) == -1
    assert L.ha_cache_update_planned_wbags(h, n, g.data_ptr(), w1.data_ptr(), 1.0, B, F, bof.data_ptr(), s) == -1
    assert gpu.plan_pending() == pending
    bag_grads = rng.standard_normal((B, width), dtype=np.float32)
    model.update(streams[1][0].astype(np.uint64), _terms(bag_grads, streams[1][1], np.arange(n) // F, 0.01))
    gpu.embedding_update_planned_wbags(torch.from_numpy(bag_grads).to(dev), w1, bag_of=bof, scale=0.01).wait()
    _check_perf(gpu, model, 1)
    tr.block_end(1)
    # ---- a push-pull chain block, and an open chain
    table_before = tr.table.clone()
    gpu.plan_block([kts[2], kts[0]], push_pull=True)
    pending = gpu.plan_pending()
    torch.cuda.synchronize()
    state_before[0] = state()
    w2 = torch.from_numpy(streams[2][1]).to(dev)
    refused(both, gpu.embedding_lookup_wsum_planned, out, w2, bag=F)
    assert L.ha_cache_lookup_wsum_planned(h, n, B, F, None, w2.data_ptr(), out.data_ptr(), s) == -1
    assert b"chain" in L.ha_last_error()
    rows_t = torch.empty((n, width), dtype=torch.float32, device=dev)
    want = model.lookup(streams[2][0].astype(np.uint64)).reshape(n, width)
    gpu.embedding_lookup_planned(rows_t).wait()
    np.testing.assert_array_equal(_bits(rows_t), _bits(want))
    pending = gpu.plan_pending()
    state_before[0] = state()
    refused(both, gpu.embedding_update_planned_wbags, g, w2, bag=F)
    refused(both, gpu.embedding_lookup_wsum_planned, out, w2, bag=F)
    assert L.ha_cache_update_planned_wbags(h, n, g.data_ptr(), w2.data_ptr(), 1.0, B, F, None, s) == -1
    assert b"chain" in L.ha_last_error()
    assert gpu.plan_pending() == pending
    # the chain goes on and closes as planned: the model's state
    grads = rng.standard_normal((n, width), dtype=np.float32) * np.float32(0.01)
    want = model.push_pull(streams[0][0].astype(np.uint64), streams[2][0].astype(np.uint64), grads).reshape(n, width)
    gpu.embedding_push_pull_planned(rows_t, torch.from_numpy(grads).to(dev)).wait()
    np.testing.assert_array_equal(_bits(rows_t), _bits(want))
    gpu.plan_block([None], push_pull=True)
    model.update(streams[0][0].astype(np.uint64), grads)
    gpu.embedding_update_planned(torch.from_numpy(grads).to(dev)).wait()
    assert gpu.plan_pending() == 0
    np.testing.assert_array_equal(tr.versions.cpu().numpy(), tr.server.ver)
    np.testing.assert_array_equal(_bits(tr.table), _bits(tr.server.table))
    _compare_state(gpu, model, 3)

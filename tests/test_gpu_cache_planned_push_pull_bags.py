"""The planned PUSH-PULL CHAIN of the HET cache with SUM-POOLED entries (csrc/cache_block.hip: ha_cache_push_pull_planned_bags /
ha_cache_run_planned_push_pulls_bags) against oracle/cache_model.py + tests/bag_model.py.

The chain's head is CacheModel.lookup, every middle step CacheModel.push_pull(pull = batch k, push = batch k - 1 with the pooled
gradient's row of every id's bag), its closing entry CacheModel.update.  After EVERY entry: the pooled output equals
bag_model.bag_sum over the model's rows (ids 0 .. n-1) bit for bit -- one float32 add per term, position order --, the server's
versions and its table; resident set / versions / update counters / data and gradient rows of every line wherever
test_gpu_cache_planned_push_pull._run_chain compares them (the end of a block that was planned alone; after the closing entry
otherwise).  And against the unpooled chain calls on caches over copies of the store.  No tolerance anywhere.

The shapes are the smallest that reach each instantiation of the pooled pull half, by the launch rule of lookup_sum_rows: VEC
from the width and nbags * slices >= 2048, ROWS 8 for a mean bag of at most 8 ids and 32 above."""
import numpy as np
import pytest
import torch

import bag_model
from herald_amd import _lib
from herald_amd import cache as hcache
from herald_amd import ops
from oracle import cache_model
from test_gpu_cache import _compare_state
from test_gpu_cache_planned import _draw, _setup
from test_gpu_cache_planned_bags import _bits, _lines_equal, _ragged_offsets, _want_pooled, _which_bag
from test_gpu_cache_planned_push_pull import _check_perf_last, _count_cases, _new_stats, _second_writer

pytestmark = pytest.mark.gpu

REFUSED = (ValueError, RuntimeError, _lib.HeraldAmdError)


class _Stream:
    """The inputs of a chain: keys, bags and pooled gradients of every batch, drawn before anything runs."""

    def __init__(self, rng, rows, width, steps, B=None, F=None, sizes=None, zipf=True, hot=None, plant=None):
        self.width, self.steps, self.F = width, steps, F
        self.sizes = list(sizes) if sizes is not None else [B * F] * steps
        self.keys = [_draw(rng, m, rows, zipf) for m in self.sizes]
        if hot is not None:                      # (key, times): that key that often at the front of every batch
            for k in self.keys:
                k[:hot[1]] = hot[0]
        for step, key in (plant or {}).items():
            # `key` three times in the batch before: the step at `step` pushes its line (push_bound < 3); and in the step's own
            # batch as occurrences 0 and 1 (bag 0: the head occurrence and a second one) and in bag 2
            self.keys[step - 1][[5, 9, 13]] = key
            self.keys[step][[0, 1, 2 * F + 1]] = key
        self.offs = None if F is not None else [_ragged_offsets(rng, m) for m in self.sizes]
        self.nbags = [m // F if F is not None else self.offs[e].size - 1 for e, m in enumerate(self.sizes)]
        self.bag_grads = [rng.standard_normal((nb, width), dtype=np.float32) * np.float32(-0.01) for nb in self.nbags]

    def off(self, e):
        return None if self.offs is None else self.offs[e]

    def expanded(self, e):
        which = _which_bag(self.sizes[e], self.F, self.off(e))
        return np.ascontiguousarray(self.bag_grads[e][which].reshape(self.sizes[e], self.width))

    def want(self, e, want_rows):
        return _want_pooled(want_rows.reshape(self.sizes[e], self.width), self.sizes[e], self.F, self.off(e))


def _entry(dev, gpu, model, S, e, pooled=True):
    """Entry e of the chain (None: the closing one) on the model and -- gpu is not None -- on the cache, pooled or through the
    unpooled call of the same place; the pooled output is compared."""
    last = S.steps - 1
    if e is None:
        model.update(S.keys[last].astype(np.uint64), S.expanded(last))
        if gpu is None:
            return
        if pooled:
            bof = None if S.F is not None else ops.bag_of(torch.from_numpy(S.off(last)).to(dev), S.sizes[last])
            gpu.embedding_push_pull_planned_bags(None, torch.from_numpy(S.bag_grads[last]).to(dev), bag=S.F, push_bag_of=bof).wait()
        else:
            gpu.embedding_update_planned(torch.from_numpy(S.expanded(last)).to(dev)).wait()
        _check_perf_last(gpu, model, S.steps)
        return
    n, keys = S.sizes[e], S.keys[e].astype(np.uint64)
    if e == 0:
        want_rows = model.lookup(keys)
    else:
        want_rows = model.push_pull(keys, S.keys[e - 1].astype(np.uint64), S.expanded(e - 1))
    if gpu is None:
        return
    want = S.want(e, want_rows)
    off_t = None if S.F is not None else torch.from_numpy(S.off(e)).to(dev)
    if pooled:
        out = torch.full((S.nbags[e], S.width), float("nan"), dtype=torch.float32, device=dev)
        g = bof = None
        if e > 0:
            g = torch.from_numpy(S.bag_grads[e - 1]).to(dev)
            bof = None if S.F is not None else ops.bag_of(torch.from_numpy(S.off(e - 1)).to(dev), S.sizes[e - 1])
        gpu.embedding_push_pull_planned_bags(out, g, bag=S.F, pull_offsets=off_t, push_bag_of=bof).wait()
    else:
        rows = torch.empty((n, S.width), dtype=torch.float32, device=dev)
        if e == 0:
            gpu.embedding_lookup_planned(rows).wait()
        else:
            gpu.embedding_push_pull_planned(rows, torch.from_numpy(S.expanded(e - 1)).to(dev)).wait()
        pos = torch.arange(n, dtype=torch.int64, device=dev)
        out = ops.embedding_lookup_sum(rows, pos.reshape(S.nbags[e], S.F) if S.F is not None else pos, offsets=off_t)
        torch.cuda.synchronize()
    if e == 0:
        _check_perf_last(gpu, model, e)
    np.testing.assert_array_equal(_bits(out), _bits(want), err_msg="pooled rows at step %d" % e)


def _model_only(limit, rows, width, n, pull_bound, push_bound, seed):
    """_setup without a device: the same draws from the same generator, the store as host tensors (for _second_writer)."""
    rng = np.random.default_rng(seed)
    table0 = rng.standard_normal((rows, width), dtype=np.float32)
    server = cache_model.Server(table0)
    model = cache_model.CacheModel("lru", limit, width, server, pull_bound, push_bound)
    return rng, server, model, torch.from_numpy(table0.copy()), torch.zeros(rows, dtype=torch.int64), None


def _run_chain_bags(dev, limit, rows, width, steps, pull_bound, push_bound, block, B=None, F=None, sizes=None, seed=0, zipf=True,
                    ahead=True, dtype=np.float32, light=False, second_writer=0, hot=None, plant=None, pooled=lambda e: True):
    """`steps` batches of B bags of F ids (or of `sizes` ids in ragged bags): a head, steps - 1 push-pull steps, the closing
    entry -- steps + 1 entries in blocks of `block`; ahead / light / second_writer / hot as _run_chain of
    test_gpu_cache_planned_push_pull.py.  pooled(e): whether entry e (None: the closing one) is made by the pooled call.
    dev = None: the model alone (the counters of a seed are a condition on the inputs, checked without a GPU).
    -> (cache, model, counters, counters after every entry)."""
    nmax = max(sizes) if sizes is not None else B * F
    if dev is None:
        rng, server, model, table, versions, gpu = _model_only(limit, rows, width, nmax, pull_bound, push_bound, seed)
    else:
        rng, server, model, table, versions, gpu = _setup(dev, limit, rows, width, nmax, pull_bound, push_bound, seed)
    S = _Stream(rng, rows, width, steps, B=B, F=F, sizes=sizes, zipf=zipf, hot=hot, plant=plant)
    kts = [torch.from_numpy(k.astype(dtype)).to(dev) for k in S.keys] if gpu is not None else None
    entries = list(range(steps)) + [None]
    blocks = [entries[b0:b0 + block] for b0 in range(0, len(entries), block)]
    stats, per_entry = _new_stats(), []

    def plan(blk):
        if gpu is not None:
            gpu.plan_block([kts[e] if e is not None else None for e in blk], push_pull=True)

    if ahead:
        plan(blocks[0])
    for j, blk in enumerate(blocks):
        if ahead and j + 1 < len(blocks):
            plan(blocks[j + 1])
        elif not ahead:
            plan(blk)
        for e in blk:
            if e is not None and e > 0:
                _count_cases(model, S.keys[e], S.keys[e - 1], stats)
            per_entry.append(dict(stats))
            nperf = len(gpu.perf) if gpu is not None else 0
            _entry(dev, gpu, model, S, e, pooled(e))
            step = steps if e is None else e
            if gpu is not None:
                assert len(gpu.perf) == nperf + (1 if e is None or e == 0 else 0)       # a push-pull step appends no record
                np.testing.assert_array_equal(versions.cpu().numpy(), server.ver, err_msg="server versions step %d" % step)
                if not light:
                    np.testing.assert_array_equal(table.cpu().numpy(), server.table, err_msg="server table step %d" % step)
            if second_writer and e is not None:
                _second_writer(rng, model, server, table, versions, second_writer)
        if gpu is not None and (not ahead or j + 1 == len(blocks)):
            assert gpu.plan_pending() == 0
            if not light:
                _compare_state(gpu, model, blk[-1] if blk[-1] is not None else steps)
    if gpu is not None:
        np.testing.assert_array_equal(table.cpu().numpy(), server.table, err_msg="server table at the end")
        st = gpu.state()
        assert st["size"] == model.policy.size() and st["pending_evictions"] == 0 and len(model.evict) == 0
        np.testing.assert_array_equal(gpu.keys(), np.array(model.policy.keys(), dtype=np.uint64))
    return gpu, model, stats, per_entry


# ---- 1. LRU trace ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pull_bound,push_bound", [(0, 0), (2, 2), (1, 5), (100, 100)])
@pytest.mark.parametrize("block,ahead", [(1, False), (16, True), (5, True)])
def test_pooled_chain_lru_trace(dev, pull_bound, push_bound, block, ahead):
    _run_chain_bags(dev, limit=128, rows=1500, width=8, B=16, F=4, steps=64, pull_bound=pull_bound, push_bound=push_bound,
                    block=block, seed=11, ahead=ahead)


# ---- 2. the version adjust --------------------------------------------------------------------------------------------------
ADJUST = dict(limit=128, rows=1500, width=8, B=16, F=4, steps=64, pull_bound=2, push_bound=2, block=6, seed=5)
PLANTED = dict(limit=128, rows=1500, width=8, B=16, F=4, steps=12, pull_bound=2, push_bound=2, block=6, seed=7, plant={5: 1234})


def test_pooled_chain_line_pulled_back_because_of_its_own_push(dev):
    # seed 5: the model alone (dev = None, no GPU) counts pulled_and_pushed = 669, pulled_back_by_own_push = 42
    _, _, stats, _ = _run_chain_bags(dev, **ADJUST)
    assert stats["pulled_and_pushed"] > 0 and stats["pulled_back_by_own_push"] > 0, stats


def test_pooled_chain_pulled_back_line_twice_in_bag_0_and_once_in_another(dev):
    """A hand-built step (seed 7, step 5; checked on the model alone: pulled_back_by_own_push goes from 11 to 15 there): key 1234 three times in batch 4, so step 5 pushes its
    line with 3 > push_bound updates, and in batch 5 as occurrences 0 and 1 -- bag 0 holds the key's head occurrence and a second
    one -- and 9 (bag 2).  Its version before the push half's commit is within pull_bound of the store's, after it it is not:
    every occurrence reads the store row + the kept gradient row, the slice waves of bag 0 refresh the line, and the version
    staged is the store's + the adjust."""
    key, step, F = 1234, 5, PLANTED["F"]
    _, model, _, per_entry = _run_chain_bags(None, **PLANTED)              # the inputs' own condition, on the model alone
    S = _Stream(_model_only(128, 1500, 8, 64, 2, 2, 7)[0], 1500, 8, 12, B=16, F=F, plant={5: key})
    assert (S.keys[step - 1] == key).sum() == 3
    assert np.flatnonzero(S.keys[step] == key).tolist() == [0, 1, 2 * F + 1]
    assert per_entry[step]["pulled_back_by_own_push"] > per_entry[step - 1]["pulled_back_by_own_push"]
    _, model, _, got = _run_chain_bags(dev, **PLANTED)
    assert got == per_entry


# ---- 3. every insert evicts -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ahead", [False, True])
def test_pooled_chain_evicted_key_is_pulled_again_in_the_step_that_pushes_it(dev, ahead):
    # limit == n_pull + n_push, uniform keys (seed 3: the model alone counts evicted_key_pulled_again = 200)
    _, _, stats, _ = _run_chain_bags(dev, limit=128, rows=1000, width=4, B=16, F=4, steps=64, pull_bound=2, push_bound=2, block=8,
                                     seed=3, zipf=False, ahead=ahead)
    assert stats["evicted_key_pulled_again"] > 0, stats


# ---- 4. a second writer -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ahead", [False, True])
def test_pooled_chain_second_writer_makes_lines_with_gradients_stale(dev, ahead):
    # (seed 17: the model alone counts addup_with_gradient = 234)
    _, _, stats, _ = _run_chain_bags(dev, limit=160, rows=1500, width=8, B=16, F=4, steps=40, pull_bound=1, push_bound=6, block=4,
                                     seed=17, ahead=ahead, second_writer=3)
    assert stats["addup_with_gradient"] > 0, stats


# ---- 5. the instantiations of the pooled pull half ----------------------------------------------------------------------------
@pytest.mark.parametrize("width,B,F,limit,rows,steps,light", [
    (128, 16, 26, 1000, 5000, 8, False),           # VEC 1 (16 bags of one slice), ROWS 32
    (512, 1024, 2, 4608, 12000, 4, True),          # VEC 4 (1,024 bags x 2 slices = 2,048), ROWS 8
    (128, 2048, 2, 9216, 24000, 4, True),          # VEC 2 (2,048 bags x 1 slice), ROWS 8
    (512, 1024, 9, 20000, 50000, 3, True),         # VEC 4, ROWS 32
    (10, 24, 4, 200, 900, 20, False),              # the scalar path: a width that is no multiple of 4
    (66, 24, 4, 200, 900, 12, False),              # ... and one wider than a slice of 64 columns
])
def test_pooled_chain_instantiations(dev, width, B, F, limit, rows, steps, light):
    _run_chain_bags(dev, limit=limit, rows=rows, width=width, B=B, F=F, steps=steps, pull_bound=1, push_bound=2, block=3,
                    seed=24 + width, light=light)


def test_pooled_chain_width_512_one_key_hundreds_of_times(dev):
    # the hot key is pulled AND pushed by every step, 600 occurrences over bags 0 .. 23: the cooperative long-run path of the
    # accumulate reads pooled gradient rows and keeps the line's gradient row for the pull half's addup
    # (seed 25: the model alone counts pulled_back_by_own_push = 105)
    _, _, stats, _ = _run_chain_bags(dev, limit=5000, rows=6000, width=512, B=80, F=25, steps=4, pull_bound=1, push_bound=2,
                                     block=3, seed=25, hot=(77, 600))
    assert stats["pulled_back_by_own_push"] > 0, stats


# ---- 6. ragged bags -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ahead,block", [(True, 4), (False, 3)])
def test_pooled_chain_ragged_bags_empty_batches_and_int64_keys(dev, ahead, block):
    sizes = [64, 1, 0, 33, 64, 0, 0, 17, 64, 2]
    _run_chain_bags(dev, limit=128, rows=700, width=8, steps=len(sizes), pull_bound=1, push_bound=1, block=block, seed=9,
                    dtype=np.int64, sizes=sizes, ahead=ahead)


# ---- 7. pooled equals unpooled, bit for bit -----------------------------------------------------------------------------------
def _lines_equal_in_an_open_chain(a, b, what):
    """_lines_equal between two steps of a chain: the lines the last step inserted have no gradient buffer yet (their rows
    are whatever the allocation held; the next accumulate starts from zero), so gradient rows are compared where a line holds
    unpushed updates."""
    la, lb = a.lines(), b.lines()
    assert sorted(la) == sorted(lb), what
    for k in la:
        assert la[k].version == lb[k].version and la[k].updates == lb[k].updates, (what, k)
        np.testing.assert_array_equal(_bits(la[k].data), _bits(lb[k].data), err_msg="%s: data of key %d" % (what, k))
        if la[k].updates:
            np.testing.assert_array_equal(_bits(la[k].grad), _bits(lb[k].grad), err_msg="%s: grad of key %d" % (what, k))


def test_pooled_chain_equals_the_unpooled_chain_bit_for_bit(dev):
    limit, rows, width, B, F, steps, block = 128, 1500, 8, 16, 4, 32, 4
    n = B * F
    rng = np.random.default_rng(11)
    table0 = rng.standard_normal((rows, width), dtype=np.float32)
    caches = []
    for _ in range(3):            # unpooled, pooled, alternating entry by entry
        t = torch.from_numpy(table0.copy()).to(dev)
        v = torch.zeros(rows, dtype=torch.int64, device=dev)
        c = hcache.LRUCache(limit, rows, width, node_id=0, max_batch=n, device=dev)
        c.bind_store(t, v)
        c.pull_bound, c.push_bound = 2, 2
        caches.append((c, t, v))
    kts = [torch.from_numpy(_draw(rng, n, rows, True).astype(np.float32)).to(dev) for _ in range(steps)]
    gs = [torch.from_numpy(rng.standard_normal((B, width), dtype=np.float32) * np.float32(-0.01)).to(dev) for _ in range(steps)]
    pos = torch.arange(n, dtype=torch.int64, device=dev).reshape(B, F)
    entries = list(range(steps)) + [None]
    count = 0
    for b0 in range(0, len(entries), block):
        blk = entries[b0:b0 + block]
        for c, _, _ in caches:
            c.plan_block([kts[e] if e is not None else None for e in blk], push_pull=True)
        for e in blk:
            prev = steps - 1 if e is None else e - 1
            expanded = None if e == 0 else ops.IndexedSlices(indices=kts[prev].reshape(B, F), values=gs[prev],
                                                             dense_shape=(rows, width), bag=F).expanded_values()
            outs = []
            for which, (c, _, _) in enumerate(caches):
                if which == 1 or (which == 2 and count % 2 == 0):
                    out = None if e is None else torch.empty((B, width), dtype=torch.float32, device=dev)
                    c.embedding_push_pull_planned_bags(out, None if e == 0 else gs[prev], bag=F).wait()
                else:
                    rws = torch.empty((n, width), dtype=torch.float32, device=dev)
                    if e is None:
                        c.embedding_update_planned(expanded).wait()
                    elif e == 0:
                        c.embedding_lookup_planned(rws).wait()
                    else:
                        c.embedding_push_pull_planned(rws, expanded).wait()
                    out = None if e is None else ops.embedding_lookup_sum(rws, pos)
                torch.cuda.synchronize()
                outs.append(None if out is None else _bits(out))
            count += 1
            if e is not None:
                np.testing.assert_array_equal(outs[0], outs[1], err_msg="pooled / unpooled output at step %d" % e)
                np.testing.assert_array_equal(outs[0], outs[2], err_msg="alternating / unpooled output at step %d" % e)
            for j in (1, 2):
                what = "cache %d after entry %s" % (j, e)
                np.testing.assert_array_equal(_bits(caches[0][1]), _bits(caches[j][1]), err_msg=what + ": store table")
                assert torch.equal(caches[0][2], caches[j][2]), what + ": server versions"
        for j in (1, 2):          # (a block planned alone has ended: lines() shows what the rows have reached)
            _lines_equal_in_an_open_chain(caches[0][0], caches[j][0], "cache %d after the block at %d" % (j, b0))
    assert all(c.plan_pending() == 0 for c, _, _ in caches)
    for j in (1, 2):              # the chain is closed: every line has its gradient buffer
        _lines_equal(caches[0][0], caches[j][0], "cache %d after the closing entry" % j)


# ---- 8. run_planned_push_pulls_bags -------------------------------------------------------------------------------------------
def test_run_planned_push_pulls_bags_equals_the_per_call_method(dev):
    limit, rows, width, B, F, block = 128, 1500, 8, 16, 4, 4
    n = B * F
    rng = np.random.default_rng(21)
    table0 = rng.standard_normal((rows, width), dtype=np.float32)
    pair = []
    for _ in range(2):
        t = torch.from_numpy(table0.copy()).to(dev)
        v = torch.zeros(rows, dtype=torch.int64, device=dev)
        c = hcache.LRUCache(limit, rows, width, node_id=0, max_batch=n, device=dev)
        c.bind_store(t, v)
        c.pull_bound, c.push_bound = 2, 2
        pair.append((c, t, v))
    head = torch.from_numpy(_draw(rng, n, rows, True).astype(np.float32)).to(dev)
    gprev = torch.from_numpy(rng.standard_normal((B, width), dtype=np.float32) * np.float32(0.01)).to(dev)
    first = [torch.empty((B, width), dtype=torch.float32, device=dev) for _ in range(2)]
    for j, (c, _, _) in enumerate(pair):
        c.plan_block([head], push_pull=True)
        c.embedding_push_pull_planned_bags(first[j], None, bag=F)
    for blk in range(2):
        kts = [torch.from_numpy(_draw(rng, n, rows, True).astype(np.float32)).to(dev) for _ in range(block)]
        gs = [gprev] + [torch.from_numpy(rng.standard_normal((B, width), dtype=np.float32) * np.float32(0.01)).to(dev)
                        for _ in range(block)]
        outs = [[torch.empty((B, width), dtype=torch.float32, device=dev) for _ in range(block)] for _ in range(2)]
        for c, _, _ in pair:
            c.plan_block(kts, push_pull=True)
        for k in range(block):
            pair[0][0].embedding_push_pull_planned_bags(outs[0][k], gs[k], bag=F)
        pair[1][0].run_planned_push_pulls_bags(outs[1], gs[:block], F)
        torch.cuda.synchronize()
        assert pair[0][0].plan_pending() == 0 and pair[1][0].plan_pending() == 0
        for k in range(block):
            np.testing.assert_array_equal(_bits(outs[0][k]), _bits(outs[1][k]), err_msg="block %d step %d" % (blk, k))
        np.testing.assert_array_equal(_bits(pair[0][1]), _bits(pair[1][1]))
        assert torch.equal(pair[0][2], pair[1][2])
        _lines_equal_in_an_open_chain(pair[0][0], pair[1][0], "block %d" % blk)
        gprev = gs[block]
    np.testing.assert_array_equal(_bits(first[0]), _bits(first[1]))
    for c, _, _ in pair:
        c.plan_block([None], push_pull=True)
        c.embedding_push_pull_planned_bags(None, gprev, bag=F).wait()
    np.testing.assert_array_equal(_bits(pair[0][1]), _bits(pair[1][1]))
    _lines_equal(pair[0][0], pair[1][0], "after the closing entry")


# ---- 9. life cycle ------------------------------------------------------------------------------------------------------------
def test_pooled_chain_life_cycle(dev):
    """lines() and a snapshot taken right after a pooled pull half see its staged versions committed (and the gradient rows its
    push half kept zeroed), as after an unpooled one; the chain goes on from there; afterwards a pooled pair block and a new
    chain work."""
    limit, rows, width, B, F, steps = 128, 900, 8, 12, 4, 6
    rng, server, model, table, versions, gpu = _setup(dev, limit, rows, width, B * F, 1, 2, seed=51)
    S = _Stream(rng, rows, width, steps, B=B, F=F)
    kts = [torch.from_numpy(k.astype(np.float32)).to(dev) for k in S.keys]
    nperf = len(gpu.perf)
    gpu.plan_block(kts[:3], push_pull=True)
    for e in range(3):
        _entry(dev, gpu, model, S, e)
        assert gpu.plan_pending() == 2 - e
    _compare_state(gpu, model, 2)                    # lines(): right after a pooled pull half
    snap = gpu._snapshot()
    assert sorted(snap["keys"].tolist()) == sorted(int(k) for k in model.resident())
    _compare_state(gpu, model, 2)                    # ... and settled once only
    gpu.plan_block(kts[3:] + [None], push_pull=True)
    for e in [3, 4, 5, None]:
        _entry(dev, gpu, model, S, e)
    assert [p["type"] for p in gpu.perf[nperf:]] == ["Pull", "Push"]
    _compare_state(gpu, model, steps)
    np.testing.assert_array_equal(table.cpu().numpy(), server.table)
    np.testing.assert_array_equal(versions.cpu().numpy(), server.ver)
    # a pooled PAIR block after the chain, then a new chain closed by a block of its own
    k = _draw(rng, B * F, rows, True)
    g = rng.standard_normal((B, width), dtype=np.float32) * np.float32(0.01)
    gpu.plan_block([torch.from_numpy(k.astype(np.float32)).to(dev)])
    want = model.lookup(k.astype(np.uint64)).reshape(B * F, width)
    out = torch.empty((B, width), dtype=torch.float32, device=dev)
    gpu.embedding_lookup_sum_planned(out, bag=F).wait()
    np.testing.assert_array_equal(_bits(out), _bits(bag_model.bag_sum(want, np.arange(B * F).reshape(B, F))))
    model.update(k.astype(np.uint64), np.ascontiguousarray(g[np.arange(B * F) // F]))
    gpu.embedding_update_planned_bags(torch.from_numpy(g).to(dev), bag=F).wait()
    _compare_state(gpu, model, 100)
    S2 = _Stream(rng, rows, width, 3, B=B, F=F)
    gpu.plan_block([torch.from_numpy(k.astype(np.float32)).to(dev) for k in S2.keys], push_pull=True)
    for e in range(3):
        _entry(dev, gpu, model, S2, e)
    gpu.plan_block([None], push_pull=True)
    assert gpu.plan_pending() == 1
    _entry(dev, gpu, model, S2, None)
    _compare_state(gpu, model, 101)
    np.testing.assert_array_equal(table.cpu().numpy(), server.table)


def test_cache_destroyed_with_pooled_chain_steps_outstanding(dev):
    rows, width, B, F = 500, 8, 12, 4
    rng, server, model, table, versions, gpu = _setup(dev, 128, rows, width, B * F, 2, 2, seed=81)
    ks = [torch.from_numpy(_draw(rng, B * F, rows, True).astype(np.float32)).to(dev) for _ in range(3)]
    gpu.plan_block(ks, push_pull=True)
    out = torch.empty((B, width), dtype=torch.float32, device=dev)
    gpu.embedding_push_pull_planned_bags(out, None, bag=F).wait()
    gpu.embedding_push_pull_planned_bags(out, torch.zeros((B, width), device=dev), bag=F).wait()
    assert gpu.plan_pending() == 1
    del gpu
    torch.cuda.synchronize()


# ---- 10. refusals -------------------------------------------------------------------------------------------------------------
def test_pooled_chain_calls_refuse_misuse_and_leave_the_plan_untouched(dev):
    limit, rows, width, B, F = 200, 1500, 8, 16, 4
    n = B * F
    rng, server, model, table, versions, gpu = _setup(dev, limit, rows, width, n, 2, 2, 61)
    S = _Stream(rng, rows, width, 3, B=B, F=F)
    kts = [torch.from_numpy(k.astype(np.float32)).to(dev) for k in S.keys]
    out = torch.empty((B, width), dtype=torch.float32, device=dev)
    g = torch.zeros((B, width), dtype=torch.float32, device=dev)
    off = torch.arange(0, n + 1, F, dtype=torch.int64, device=dev)
    bof = ops.bag_of(off, n)
    L, h, s = gpu._L, gpu._h, gpu._stream().cuda_stream
    pending = [0]

    def refused(*a, **kw):
        with pytest.raises(REFUSED):
            gpu.embedding_push_pull_planned_bags(*a, **kw)
        assert gpu.plan_pending() == pending[0]

    def native_refused(*a):
        assert L.ha_cache_push_pull_planned_bags(h, *a, s) == -1
        assert b"cache_push_pull_planned_bags" in L.ha_last_error()
        assert gpu.plan_pending() == pending[0]

    # ---- no entry is due; a pair block is not a chain
    refused(out, None, bag=F)
    native_refused(n, B, F, None, out.data_ptr(), 0, 0, 0, None, None)
    gpu.plan_block([kts[0]])
    pending[0] = gpu.plan_pending()
    assert pending[0] == 2
    refused(out, None, bag=F)
    native_refused(n, B, F, None, out.data_ptr(), 0, 0, 0, None, None)
    rows_t = torch.empty((n, width), dtype=torch.float32, device=dev)
    want = model.lookup(S.keys[0].astype(np.uint64))
    gpu.embedding_lookup_planned(rows_t).wait()
    np.testing.assert_array_equal(rows_t.cpu().numpy(), want)
    pending[0] = gpu.plan_pending()
    refused(None, g, bag=F)
    native_refused(-1, 0, 0, None, None, n, B, F, None, g.data_ptr())
    grads0 = np.zeros((n, width), dtype=np.float32)
    model.update(S.keys[0].astype(np.uint64), grads0)
    gpu.embedding_update_planned(torch.from_numpy(grads0).to(dev)).wait()
    # ---- the head
    gpu.plan_block(kts, push_pull=True)
    pending[0] = gpu.plan_pending()
    assert pending[0] == 3
    refused(out, g, bag=F)                                         # the head pushes nothing
    refused(None, g, bag=F)                                        # ... and is no closing entry
    refused(out[:B - 1], None, bag=F)                              # wrong sizes
    refused(out, None, bag=F + 1)
    refused(out, None, bag=F, pull_offsets=off)                    # both descriptions
    refused(out, None)                                             # neither
    native_refused(n, B, F, None, out.data_ptr(), n, B, F, None, g.data_ptr())
    native_refused(-1, 0, 0, None, None, n, B, F, None, g.data_ptr())
    native_refused(n, B, F + 1, None, out.data_ptr(), 0, 0, 0, None, None)
    native_refused(n - F, B - 1, F, None, out.data_ptr(), 0, 0, 0, None, None)
    native_refused(n, B, F, off.data_ptr(), out.data_ptr(), 0, 0, 0, None, None)
    native_refused(n, B, 0, None, out.data_ptr(), 0, 0, 0, None, None)
    native_refused(n, B, F, None, None, 0, 0, 0, None, None)
    _entry(dev, gpu, model, S, 0)
    # ---- a middle step
    pending[0] = gpu.plan_pending()
    assert pending[0] == 2
    refused(out, None, bag=F)                                      # a missing side
    refused(None, g, bag=F)
    refused(out[:B - 1], g, bag=F)                                 # wrong sizes, either side
    refused(out, g[:B - 1], bag=F)
    refused(out, g, bag=F + 1)
    refused(out, g, bag=F, pull_offsets=off, push_bag_of=bof)      # both descriptions
    refused(out, g)                                                # neither
    refused(out, g, pull_offsets=off)                              # ... on the push side
    refused(out, g, push_bag_of=bof)                               # ... on the pull side
    native_refused(n, B, F, None, out.data_ptr(), 0, 0, 0, None, None)
    native_refused(-1, 0, 0, None, None, n, B, F, None, g.data_ptr())
    native_refused(n, B, F, off.data_ptr(), out.data_ptr(), n, B, F, None, g.data_ptr())
    native_refused(n, B, F, None, out.data_ptr(), n, B, F, bof.data_ptr(), g.data_ptr())
    native_refused(n, B, 0, None, out.data_ptr(), n, B, F, None, g.data_ptr())
    native_refused(n, B, F, None, out.data_ptr(), n, B, 0, None, g.data_ptr())
    native_refused(n, B, F, None, out.data_ptr(), n, B, F, None, None)
    native_refused(n, B, F, None, out.data_ptr(), n - F, B - 1, F, None, g.data_ptr())
    with pytest.raises(REFUSED):
        gpu.run_planned_push_pulls_bags([out] * 3, [g] * 3, F)     # two steps are planned, the third entry is not one
    assert gpu.plan_pending() == pending[0]
    _entry(dev, gpu, model, S, 1)
    _entry(dev, gpu, model, S, 2)
    # ---- the chain is open and nothing is outstanding
    pending[0] = gpu.plan_pending()
    assert pending[0] == 0
    refused(out, g, bag=F)
    native_refused(n, B, F, None, out.data_ptr(), n, B, F, None, g.data_ptr())
    # ---- the closing entry
    gpu.plan_block([None], push_pull=True)
    pending[0] = gpu.plan_pending()
    assert pending[0] == 1
    refused(out, g, bag=F)                                         # it pulls nothing
    refused(out, None, bag=F)
    refused(None, g[:B - 1], bag=F)
    refused(None, g, bag=F, push_bag_of=bof)
    refused(None, g)
    native_refused(n, B, F, None, out.data_ptr(), n, B, F, None, g.data_ptr())
    native_refused(-1, 0, 0, None, None, n, B, F, bof.data_ptr(), g.data_ptr())
    native_refused(-1, 0, 0, None, None, n, B, 0, None, g.data_ptr())
    native_refused(-1, 0, 0, None, None, n, B, F, None, None)
    _entry(dev, gpu, model, S, None)
    # ---- the chain has completed as the model's
    assert gpu.plan_pending() == 0
    np.testing.assert_array_equal(versions.cpu().numpy(), server.ver)
    np.testing.assert_array_equal(table.cpu().numpy(), server.table)
    _compare_state(gpu, model, 3)

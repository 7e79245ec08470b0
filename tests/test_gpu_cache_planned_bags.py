"""Sum-pooled lookup and update in the PLANNED flow of the HET cache (csrc/cache_block.hip: ha_cache_lookup_sum_planned /
ha_cache_update_planned_bags / ha_cache_run_planned_pairs_bags) against oracle/cache_model.py + tests/bag_model.py.

Every step: want_rows = model.lookup(keys); the pooled output equals bag_model.bag_sum(want_rows, ids 0 .. n-1) BIT FOR BIT
(one float32 add per term, position order); model.update(keys, bag_grads[bag of every id]); the perf dict's counts, the
server's versions and table; the whole line state (_compare_state) at the end of every block that was planned alone and at the
end of the stream.  And against the unfused calls on a second cache over a copy of the store, bit for bit."""
import numpy as np
import pytest
import torch

import bag_model
from herald_amd import cache as hcache
from herald_amd import ops
from oracle import cache_model
from test_gpu_cache import _compare_state
from test_gpu_cache_planned import _check_perf, _draw, _setup

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _table_registry_as_found():
    """Leave the process-wide table registry (cache.register_table) as it was found."""
    before = dict(hcache._TABLES)
    yield
    hcache._TABLES.clear()
    hcache._TABLES.update(before)


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _want_pooled(want_rows, n, bag, offsets):
    pos = np.arange(n, dtype=np.int64)
    if offsets is None:
        return bag_model.bag_sum(want_rows, pos.reshape(n // bag, bag))
    return bag_model.bag_sum(want_rows, pos, offsets)


def _which_bag(n, bag, offsets):
    if offsets is None:
        return np.arange(n) // bag
    return bag_model.bag_of(offsets, n).astype(np.int64)


def _bag_step(dev, gpu, model, keys, bag_grads, width, step, versions, server, bag=None, offsets=None, pk=False,
              pooled_lookup=True, pooled_update=True, stats=None):
    """One planned pair held to the model.  bag: fixed bags; offsets (numpy int64 [nbags + 1]): ragged bags.  pk: False = a
    bound-mode batch, else the batch's push keys (numpy).  pooled_* False: the unpooled call takes that place."""
    n = keys.size
    off_t = None if offsets is None else torch.from_numpy(np.asarray(offsets, dtype=np.int64)).to(dev)
    res = model.resident()
    held = {int(k): res[int(k)].updates for k in np.unique(keys) if int(k) in res}
    want_rows = model.lookup(keys.astype(np.uint64)).reshape(n, width)
    if stats is not None:
        gone = [k for k in held if not model.policy.count(k)]
        stats["own_line_evicted"] += len(gone)
        stats["own_line_evicted_dirty"] += sum(1 for k in gone if held[k] != 0)
    want = _want_pooled(want_rows, n, bag, offsets)
    nbags = want.shape[0]
    if pooled_lookup:
        out = torch.full((nbags, width), float("nan"), dtype=torch.float32, device=dev)
        gpu.embedding_lookup_sum_planned(out, bag=bag, offsets=off_t).wait()
    else:
        rows = torch.empty((n, width), dtype=torch.float32, device=dev)
        gpu.embedding_lookup_planned(rows).wait()
        np.testing.assert_array_equal(_bits(rows), _bits(want_rows), err_msg="unpooled lookup rows at step %d" % step)
        pos = torch.arange(n, dtype=torch.int64, device=dev)
        out = ops.embedding_lookup_sum(rows, pos.reshape(nbags, bag) if offsets is None else pos, offsets=off_t)
        torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(out), _bits(want), err_msg="pooled rows at step %d" % step)
    which = _which_bag(n, bag, offsets)
    expanded = np.ascontiguousarray(bag_grads[which].reshape(n, width))
    if pk is False:
        model.update(keys.astype(np.uint64), expanded)
    else:
        model.update_with_push_keys(keys.astype(np.uint64), pk.astype(np.uint64), expanded)
    g = torch.from_numpy(np.ascontiguousarray(bag_grads)).to(dev)
    if pooled_update:
        gpu.embedding_update_planned_bags(g, bag=bag, bag_of=None if offsets is None else ops.bag_of(off_t, n)).wait()
    else:
        gpu.embedding_update_planned(torch.from_numpy(expanded).to(dev)).wait()
    _check_perf(gpu, model, step)
    np.testing.assert_array_equal(versions.cpu().numpy(), server.ver, err_msg="server versions step %d" % step)
    return out


def _run_bags(dev, limit, rows, width, B, F, steps, pull_bound, push_bound, block, seed=0, zipf=True, ahead=True, policy="lru",
              dtype=np.float32, stats=None):
    """Fixed bags of F ids, B bags per batch.  ahead as in test_gpu_cache_planned._run_planned."""
    n = B * F
    rng, server, model, table, versions, gpu = _setup(dev, limit, rows, width, n, pull_bound, push_bound, seed, policy)
    keys_all = [_draw(rng, n, rows, zipf) for _ in range(steps)]      # (the whole key stream before any gradient)
    kts = [torch.from_numpy(k.astype(dtype)).to(dev) for k in keys_all]
    blocks = [list(range(b0, min(b0 + block, steps))) for b0 in range(0, steps, block)]
    if ahead:
        gpu.plan_block([kts[s] for s in blocks[0]])
    for j, blk in enumerate(blocks):
        if ahead and j + 1 < len(blocks):
            gpu.plan_block([kts[s] for s in blocks[j + 1]])
        elif not ahead:
            gpu.plan_block([kts[s] for s in blk])
        for step in blk:
            bag_grads = rng.standard_normal((B, width), dtype=np.float32) * np.float32(-0.01)
            _bag_step(dev, gpu, model, keys_all[step], bag_grads, width, step, versions, server, bag=F, stats=stats)
            np.testing.assert_array_equal(table.cpu().numpy(), server.table, err_msg="server table step %d" % step)
        if not ahead or j + 1 == len(blocks):
            assert gpu.plan_pending() == 0
            _compare_state(gpu, model, blk[-1])
    assert gpu.size() == model.policy.size()
    np.testing.assert_array_equal(gpu.keys(), np.array(model.policy.keys(), dtype=np.uint64))
    return gpu, model


# ---- 1. LRU small trace ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pull_bound,push_bound", [(0, 0), (3, 3), (100, 100)])
@pytest.mark.parametrize("block,ahead", [(1, False), (4, False), (16, True), (5, True)])
def test_pooled_lru_trace_small(dev, pull_bound, push_bound, block, ahead):
    _run_bags(dev, limit=100, rows=1500, width=8, B=16, F=4, steps=32, pull_bound=pull_bound, push_bound=push_bound,
              block=block, seed=11, ahead=ahead)


# ---- 2. LRU heavy eviction ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ahead", [False, True])
def test_pooled_lru_uniform_heavy_eviction_at_limit_equal_batch(dev, ahead):
    _run_bags(dev, limit=64, rows=1000, width=4, B=8, F=8, steps=48, pull_bound=2, push_bound=2, block=8, seed=3, zipf=False,
              ahead=ahead)


# ---- 3. LFU and LFUOpt, small cache ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["lfu", "lfuopt"])
@pytest.mark.parametrize("limit", [7, 64])
def test_pooled_lfu_cache_smaller_than_the_batch(dev, policy, limit):
    """The traces of test_planned_lfu_cache_smaller_than_the_batch (same seeds, the key stream is drawn before any gradient):
    they hold "own line evicted" and, at limit 7, "own line evicted dirty" -- counted from the CPU model alone."""
    stats = {"own_line_evicted": 0, "own_line_evicted_dirty": 0}
    _run_bags(dev, limit=limit, rows=300, width=8, B=16, F=4, steps=40, pull_bound=1, push_bound=3, block=4, seed=5 + limit,
              ahead=False, policy=policy, stats=stats)
    _run_bags(dev, limit=limit, rows=300, width=8, B=16, F=4, steps=40, pull_bound=1, push_bound=0, block=16, seed=6 + limit,
              zipf=False, ahead=True, policy=policy, stats=stats)
    assert stats["own_line_evicted"] > 0, stats
    if limit == 7:
        assert stats["own_line_evicted_dirty"] > 0, stats


@pytest.mark.parametrize("policy", ["lfu", "lfuopt"])
@pytest.mark.parametrize("block,ahead", [(1, False), (16, True), (5, True)])
def test_pooled_lfu_trace_small(dev, policy, block, ahead):
    _run_bags(dev, limit=100, rows=1500, width=8, B=16, F=4, steps=32, pull_bound=3, push_bound=3, block=block, seed=12,
              ahead=ahead, policy=policy)


# ---- 4. widths and long runs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["lru", "lfu"])
def test_pooled_width_128_bags_of_26(dev, policy):
    _run_bags(dev, limit=500, rows=5000, width=128, B=16, F=26, steps=12, pull_bound=2, push_bound=2, block=4, seed=24,
              policy=policy)


@pytest.mark.parametrize("policy,limit", [("lru", 2500), ("lfu", 900)])
def test_pooled_width_512_one_key_hundreds_of_times(dev, policy, limit):
    """zipf ids: one key holds hundreds of a batch's 2,002 positions -- the cooperative long-run path of the accumulate reads
    pooled gradient rows (BAGS) and takes the push epilogue."""
    rng = np.random.default_rng(25)
    rng.standard_normal((6000, 512), dtype=np.float32)
    top = max(np.bincount(_draw(rng, 77 * 26, 6000, True)).max() for _ in range(6))      # (_setup's own stream, seed 25)
    assert top >= 200, top
    _run_bags(dev, limit=limit, rows=6000, width=512, B=77, F=26, steps=6, pull_bound=1, push_bound=2, block=3, seed=25,
              policy=policy)


@pytest.mark.parametrize("policy", ["lru", "lfu"])
def test_pooled_odd_widths(dev, policy):
    # width 10: the scalar kernels; width 516: a row wider than two 16-byte vectors per lane
    _run_bags(dev, limit=120, rows=900, width=10, B=24, F=4, steps=20, pull_bound=1, push_bound=1, block=5, seed=8, policy=policy)
    _run_bags(dev, limit=100, rows=700, width=516, B=8, F=3, steps=10, pull_bound=1, push_bound=1, block=5, seed=9, policy=policy)


# ---- 5. ragged bags ---------------------------------------------------------------------------------------------------------
def _ragged_offsets(rng, n):
    """nbags = 10: empty bags at the front, in the middle and at the end."""
    cuts = np.sort(rng.integers(0, n + 1, size=5)).tolist()
    return np.array([0, 0] + cuts[:3] + [cuts[2]] + cuts[3:] + [n, n], dtype=np.int64)


@pytest.mark.parametrize("policy", ["lru", "lfu"])
def test_pooled_ragged_bags_empty_batches_and_int64_keys(dev, policy):
    sizes = [64, 1, 0, 33, 64, 0, 0, 17, 64, 2]
    width, rows = 8, 700
    rng, server, model, table, versions, gpu = _setup(dev, 100, rows, width, 64, 1, 1, 9, policy)
    keys_all = [_draw(rng, m, rows, True) for m in sizes]
    kts = [torch.from_numpy(k.astype(np.int64)).to(dev) for k in keys_all]
    offs = [_ragged_offsets(rng, m) for m in sizes]
    offs[4] = np.array([0, 64], dtype=np.int64)                               # one bag that holds everything
    offs[8] = np.array([-7, -1, 0, 5, 5, 40, 64, 64 + 3, 64 + 900], dtype=np.int64)      # entries below 0 and above n
    blocks = [list(range(b0, min(b0 + 4, len(sizes)))) for b0 in range(0, len(sizes), 4)]
    for blk in blocks:
        gpu.plan_block([kts[s] for s in blk])
        for step in blk:
            n, off = sizes[step], offs[step]
            nbags = off.size - 1
            bag_grads = rng.standard_normal((nbags, width), dtype=np.float32) * np.float32(-0.01)
            if step == 8:
                # nothing outside `out` is written: a guard row on each side
                want_rows = model.lookup(keys_all[step].astype(np.uint64)).reshape(n, width)
                want = bag_model.bag_sum(want_rows, np.arange(n), off)
                lo, hi = bag_model.clamp_offsets(off, n)
                assert lo[0] == 0 and hi[-1] == n and np.array_equal(lo[1:], hi[:-1])      # (every position in one bag)
                buf = torch.full((nbags + 2, width), 12345.0, dtype=torch.float32, device=dev)
                off_t = torch.from_numpy(off).to(dev)
                gpu.embedding_lookup_sum_planned(buf[1:-1], offsets=off_t).wait()
                got = buf.cpu().numpy()
                np.testing.assert_array_equal(_bits(got[1:-1]), _bits(want))
                assert (got[0] == 12345.0).all() and (got[-1] == 12345.0).all()
                which = bag_model.bag_of(off, n).astype(np.int64)
                model.update(keys_all[step].astype(np.uint64), np.ascontiguousarray(bag_grads[which]))
                gpu.embedding_update_planned_bags(torch.from_numpy(bag_grads).to(dev), bag_of=ops.bag_of(off_t, n)).wait()
                _check_perf(gpu, model, step)
                np.testing.assert_array_equal(versions.cpu().numpy(), server.ver)
            else:
                _bag_step(dev, gpu, model, keys_all[step], bag_grads, width, step, versions, server, offsets=off)
            np.testing.assert_array_equal(table.cpu().numpy(), server.table, err_msg="server table step %d" % step)
        assert gpu.plan_pending() == 0
        _compare_state(gpu, model, blk[-1])


# ---- 6. pulls inside bags ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["lru", "lfu"])
def test_pooled_pull_of_a_stale_key_twice_in_one_bag_and_once_in_another(dev, policy):
    """Between steps of a planned block another worker pushes to store rows the cache holds.  The next batch names such a stale
    key twice in one bag and once in another; its line has a gradient buffer (push_bound 10,000: nothing is pushed).  Every
    occurrence reads store row + gradient row, the wave of the first occurrence refreshes the line's data row."""
    limit, rows, width, B, F = 200, 600, 8, 24, 4
    n = B * F
    rng, server, model, table, versions, gpu = _setup(dev, limit, rows, width, n, 2, 10000, seed=51, policy=policy)
    keys_all = [_draw(rng, n, rows, True) for _ in range(8)]
    for step in (3, 6):
        stale = np.unique(keys_all[step - 1])[:3]        # keys of the batch before: resident, with a gradient buffer
        for t, k in enumerate(stale):
            keys_all[step][(5 + t) * F + 1] = k            # twice in bag 5 + t ...
            keys_all[step][(5 + t) * F + 3] = k
            keys_all[step][(15 + t) * F + 2] = k           # ... and once in bag 15 + t
    kts = [torch.from_numpy(k.astype(np.float32)).to(dev) for k in keys_all]
    gpu.plan_block(kts)
    torch.cuda.synchronize()            # the whole block is booked before a single row moves
    for step in range(8):
        stale = None
        if step in (3, 6):               # another worker's push: +4 updates on rows the cache holds
            stale = np.unique(keys_all[step - 1])[:3]
            hot = np.union1d(np.unique(keys_all[step])[::2], stale)
            delta = rng.standard_normal((hot.size, width), dtype=np.float32)
            server.ver[hot] += 4
            server.table[hot] = (server.table[hot] + delta).astype(np.float32)
            versions[torch.from_numpy(hot).to(dev)] += 4
            table[torch.from_numpy(hot).to(dev)] += torch.from_numpy(delta).to(dev)
            res = model.resident()
            assert all(int(k) in res and res[int(k)].grad is not None and np.any(res[int(k)].grad != 0) for k in stale)
        bag_grads = rng.standard_normal((B, width), dtype=np.float32) * np.float32(0.01)
        n_pull_before = len(model.perf)
        keys = keys_all[step]
        want_rows = model.lookup(keys.astype(np.uint64)).reshape(n, width)
        want = bag_model.bag_sum(want_rows, np.arange(n).reshape(B, F))
        out = torch.empty((B, width), dtype=torch.float32, device=dev)
        gpu.embedding_lookup_sum_planned(out, bag=F).wait()
        np.testing.assert_array_equal(_bits(out), _bits(want), err_msg="pooled rows at step %d" % step)
        if stale is not None:
            assert model.perf[n_pull_before]["num_transfered"] > model.perf[n_pull_before]["num_miss"]
            res = model.resident()
            slots = dict(zip(gpu._snapshot()["keys"].tolist(), gpu._snapshot()["slots"].tolist()))
            for k in stale:              # the refreshed data rows (the bookkeeping of the whole block ran ahead: rows only)
                np.testing.assert_array_equal(_bits(gpu._rows("data", [slots[int(k)]])[0]), _bits(res[int(k)].data),
                                              err_msg="refreshed line of key %d at step %d" % (k, step))
        model.update(keys.astype(np.uint64), np.ascontiguousarray(bag_grads[np.arange(n) // F]))
        gpu.embedding_update_planned_bags(torch.from_numpy(bag_grads).to(dev), bag=F).wait()
        _check_perf(gpu, model, step)
        np.testing.assert_array_equal(versions.cpu().numpy(), server.ver, err_msg="server versions step %d" % step)
    _compare_state(gpu, model, 8)
    np.testing.assert_array_equal(table.cpu().numpy(), server.table)


# ---- 7. fused equals unfused, bit for bit -----------------------------------------------------------------------------------
def _lines_equal(a, b, what):
    la, lb = a.lines(), b.lines()
    assert sorted(la) == sorted(lb), what
    for k in la:
        assert la[k].version == lb[k].version and la[k].updates == lb[k].updates, (what, k)
        np.testing.assert_array_equal(_bits(la[k].data), _bits(lb[k].data), err_msg="%s: data of key %d" % (what, k))
        np.testing.assert_array_equal(_bits(la[k].grad), _bits(lb[k].grad), err_msg="%s: grad of key %d" % (what, k))


@pytest.mark.parametrize("policy", ["lru", "lfu"])
def test_pooled_calls_equal_the_unpooled_pair_bit_for_bit(dev, policy):
    limit, rows, width, B, F, steps, block = 100, 1500, 8, 16, 4, 32, 4
    n = B * F
    rng = np.random.default_rng(11)
    table0 = rng.standard_normal((rows, width), dtype=np.float32)
    cls = {"lru": hcache.LRUCache, "lfu": hcache.LFUCache}[policy]
    caches = []
    for _ in range(3):            # unfused, fused, alternating
        t = torch.from_numpy(table0.copy()).to(dev)
        v = torch.zeros(rows, dtype=torch.int64, device=dev)
        c = cls(limit, rows, width, node_id=0, max_batch=n, device=dev)
        c.bind_store(t, v)
        c.pull_bound, c.push_bound = 3, 3
        caches.append((c, t, v))
    keys_all = [_draw(rng, n, rows, True) for _ in range(steps)]
    kts = [torch.from_numpy(k.astype(np.float32)).to(dev) for k in keys_all]
    pos = torch.arange(n, dtype=torch.int64, device=dev).reshape(B, F)
    for b0 in range(0, steps, block):
        for c, _, _ in caches:
            c.plan_block(kts[b0:b0 + block])
        for step in range(b0, b0 + block):
            g = torch.from_numpy(rng.standard_normal((B, width), dtype=np.float32) * np.float32(-0.01)).to(dev)
            expanded = ops.IndexedSlices(indices=kts[step].reshape(B, F), values=g, dense_shape=(rows, width),
                                         bag=F).expanded_values()
            outs = []
            for which, (c, _, _) in enumerate(caches):
                pooled_lookup = which == 1 or (which == 2 and step % 2 == 0)
                pooled_update = which == 1 or (which == 2 and step % 2 == 1)
                if pooled_lookup:
                    out = torch.empty((B, width), dtype=torch.float32, device=dev)
                    c.embedding_lookup_sum_planned(out, bag=F).wait()
                else:
                    rws = torch.empty((n, width), dtype=torch.float32, device=dev)
                    c.embedding_lookup_planned(rws).wait()
                    out = ops.embedding_lookup_sum(rws, pos)
                if pooled_update:
                    c.embedding_update_planned_bags(g, bag=F).wait()
                else:
                    c.embedding_update_planned(expanded).wait()
                torch.cuda.synchronize()
                outs.append(_bits(out))
            np.testing.assert_array_equal(outs[0], outs[1], err_msg="fused / unfused output at step %d" % step)
            np.testing.assert_array_equal(outs[0], outs[2], err_msg="alternating / unfused output at step %d" % step)
        for j in (1, 2):
            what = "cache %d after the block at %d" % (j, b0)
            np.testing.assert_array_equal(_bits(caches[0][1]), _bits(caches[j][1]), err_msg=what + ": store table")
            assert torch.equal(caches[0][2], caches[j][2]), what + ": server versions"
            _lines_equal(caches[0][0], caches[j][0], what)


# ---- 8. push keys -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["lru", "lfu"])
def test_pooled_pairs_of_batches_planned_with_push_keys(dev, policy):
    limit, rows, width, B, F, steps, block = 100, 1500, 8, 16, 4, 24, 4
    n = B * F
    rng, server, model, table, versions, gpu = _setup(dev, limit, rows, width, n, 2, 2, 71, policy)
    keys_all = [_draw(rng, n, rows, True) for _ in range(steps)]
    pks = []
    for s, k in enumerate(keys_all):
        u = np.unique(k.astype(np.int64))
        pks.append(None if s == 5 else np.sort(rng.choice(u, size=u.size // 3, replace=False)))     # one bound-mode batch
    kts = [torch.from_numpy(k.astype(np.float32)).to(dev) for k in keys_all]
    pts = [None if p is None else torch.from_numpy(p.astype(np.float32)).to(dev) for p in pks]
    for b0 in range(0, steps, block):
        gpu.plan_block(kts[b0:b0 + block], push_keys_list=pts[b0:b0 + block])
        for step in range(b0, b0 + block):
            bag_grads = rng.standard_normal((B, width), dtype=np.float32) * np.float32(-0.01)
            _bag_step(dev, gpu, model, keys_all[step], bag_grads, width, step, versions, server, bag=F,
                      pk=False if pks[step] is None else pks[step])
            np.testing.assert_array_equal(table.cpu().numpy(), server.table, err_msg="server table step %d" % step)
        assert gpu.plan_pending() == 0
        _compare_state(gpu, model, b0 + block - 1)


# ---- 9. run_planned_pairs_bags ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["lru", "lfuopt"])
def test_run_planned_pairs_bags_equals_the_per_call_methods(dev, policy):
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
        kts = [torch.from_numpy(_draw(rng, n, rows, True).astype(np.float32)).to(dev) for _ in range(block)]
        gs = [torch.from_numpy(rng.standard_normal((B, width), dtype=np.float32) * np.float32(0.01)).to(dev) for _ in range(block)]
        outs = [[torch.empty((B, width), dtype=torch.float32, device=dev) for _ in range(block)] for _ in range(2)]
        for c, _, _ in pair:
            c.plan_block(kts)
        for k in range(block):
            pair[0][0].embedding_lookup_sum_planned(outs[0][k], bag=F)
            pair[0][0].embedding_update_planned_bags(gs[k], bag=F)
        pair[1][0].run_planned_pairs_bags(outs[1], gs, F)
        torch.cuda.synchronize()
        assert pair[0][0].plan_pending() == 0 and pair[1][0].plan_pending() == 0
        for k in range(block):
            np.testing.assert_array_equal(_bits(outs[0][k]), _bits(outs[1][k]), err_msg="block %d pair %d" % (blk, k))
        np.testing.assert_array_equal(_bits(pair[0][1]), _bits(pair[1][1]))
        assert torch.equal(pair[0][2], pair[1][2])
        _lines_equal(pair[0][0], pair[1][0], "block %d" % blk)


# ---- 10. refusals -----------------------------------------------------------------------------------------------------------
def test_pooled_calls_refuse_misuse_and_leave_the_plan_untouched(dev):
    limit, rows, width, B, F = 200, 1500, 8, 16, 4
    n = B * F
    rng, server, model, table, versions, gpu = _setup(dev, limit, rows, width, n, 2, 2, 61)
    keys_all = [_draw(rng, n, rows, True) for _ in range(3)]
    kts = [torch.from_numpy(k.astype(np.float32)).to(dev) for k in keys_all]
    out = torch.empty((B, width), dtype=torch.float32, device=dev)
    g = torch.zeros((B, width), dtype=torch.float32, device=dev)
    off = torch.arange(0, n + 1, F, dtype=torch.int64, device=dev)
    bof = ops.bag_of(off, n)
    gpu.plan_block(kts[:2])
    pending = gpu.plan_pending()
    assert pending == 4

    def refused(fn, *a, **kw):
        with pytest.raises((ValueError, RuntimeError)):
            fn(*a, **kw)
        assert gpu.plan_pending() == pending

    refused(gpu.embedding_lookup_sum_planned, out, bag=F + 1)                      # nbags * bag != n
    refused(gpu.embedding_lookup_sum_planned, out[:B - 1], bag=F)
    refused(gpu.embedding_lookup_sum_planned, out, bag=F, offsets=off)             # both
    refused(gpu.embedding_lookup_sum_planned, out)                                 # neither
    refused(gpu.embedding_update_planned_bags, g, bag=F)                           # a pooled update before its lookup
    # the native entry points make the same checks before anything is enqueued
    L, h, s = gpu._L, gpu._h, gpu._stream().cuda_stream
    assert L.ha_cache_lookup_sum_planned(h, n, B, F + 1, None, out.data_ptr(), s) == -1
    assert L.ha_cache_lookup_sum_planned(h, n, B, F, off.data_ptr(), out.data_ptr(), s) == -1
    assert L.ha_cache_lookup_sum_planned(h, n, B, 0, None, out.data_ptr(), s) == -1
    assert L.ha_cache_update_planned_bags(h, n, g.data_ptr(), B, F, None, s) == -1
    assert gpu.plan_pending() == pending
    bag_grads = rng.standard_normal((B, width), dtype=np.float32) * np.float32(0.01)
    _bag_step(dev, gpu, model, keys_all[0], bag_grads, width, 0, versions, server, bag=F)      # the correct calls succeed
    pending = gpu.plan_pending()
    assert pending == 2
    want_rows = model.lookup(keys_all[1].astype(np.uint64)).reshape(n, width)
    gpu.embedding_lookup_sum_planned(out, bag=F).wait()
    np.testing.assert_array_equal(_bits(out), _bits(bag_model.bag_sum(want_rows, np.arange(n).reshape(B, F))))
    pending = gpu.plan_pending()
    refused(gpu.embedding_update_planned_bags, g, bag=F + 1)
    refused(gpu.embedding_update_planned_bags, g, bag=F, bag_of=bof)
    refused(gpu.embedding_update_planned_bags, g)
    refused(gpu.embedding_lookup_sum_planned, out, bag=F)                          # the update is due, not a lookup
    assert L.ha_cache_update_planned_bags(h, n, g.data_ptr(), B, F, bof.data_ptr(), s) == -1
    assert L.ha_cache_update_planned_bags(h, n, g.data_ptr(), B, 0, None, s) == -1
    assert L.ha_cache_lookup_sum_planned(h, n, B, F, None, out.data_ptr(), s) == -1
    assert gpu.plan_pending() == pending
    model.update(keys_all[1].astype(np.uint64), np.ascontiguousarray(bag_grads[np.arange(n) // F]))
    gpu.embedding_update_planned_bags(torch.from_numpy(bag_grads).to(dev), bag_of=bof).wait()       # ragged form of the same bags
    _check_perf(gpu, model, 1)
    assert gpu.plan_pending() == 0
    _compare_state(gpu, model, 1)
    # ---- a pooled call while a push-pull chain is open
    gpu.plan_block([kts[2], kts[0]], push_pull=True)
    pending = gpu.plan_pending()
    refused(gpu.embedding_lookup_sum_planned, out, bag=F)                          # the chain's head is a plain lookup
    assert L.ha_cache_lookup_sum_planned(h, n, B, F, None, out.data_ptr(), s) == -1
    assert b"chain" in L.ha_last_error()
    rows_t = torch.empty((n, width), dtype=torch.float32, device=dev)
    want = model.lookup(keys_all[2].astype(np.uint64)).reshape(n, width)
    gpu.embedding_lookup_planned(rows_t).wait()
    np.testing.assert_array_equal(_bits(rows_t), _bits(want))
    pending = gpu.plan_pending()
    refused(gpu.embedding_update_planned_bags, g, bag=F)
    refused(gpu.embedding_lookup_sum_planned, out, bag=F)
    assert L.ha_cache_update_planned_bags(h, n, g.data_ptr(), B, F, None, s) == -1
    assert b"chain" in L.ha_last_error()
    assert gpu.plan_pending() == pending
    # the chain goes on and closes as planned: step, closing update -- the model's state
    grads = rng.standard_normal((n, width), dtype=np.float32) * np.float32(0.01)
    want = model.push_pull(keys_all[0].astype(np.uint64), keys_all[2].astype(np.uint64), grads).reshape(n, width)
    gpu.embedding_push_pull_planned(rows_t, torch.from_numpy(grads).to(dev)).wait()
    np.testing.assert_array_equal(_bits(rows_t), _bits(want))
    gpu.plan_block([None], push_pull=True)
    pending = gpu.plan_pending()
    refused(gpu.embedding_update_planned_bags, g, bag=F)                           # the closing step is a plain update
    assert L.ha_cache_update_planned_bags(h, n, g.data_ptr(), B, F, None, s) == -1
    assert gpu.plan_pending() == pending
    model.update(keys_all[0].astype(np.uint64), grads)
    gpu.embedding_update_planned(torch.from_numpy(grads).to(dev)).wait()
    assert gpu.plan_pending() == 0
    np.testing.assert_array_equal(versions.cpu().numpy(), server.ver)
    np.testing.assert_array_equal(table.cpu().numpy(), server.table)
    _compare_state(gpu, model, 3)

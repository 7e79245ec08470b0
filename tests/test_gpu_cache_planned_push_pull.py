"""The planned PUSH-PULL CHAIN of the HET cache (csrc/cache_block.hip: ha_cache_plan_block_push_pull / ha_cache_push_pull_planned)
against oracle/cache_model.py: the chain's head is CacheModel.lookup, every middle step CacheModel.push_pull(pull = batch k,
push = batch k - 1), its closing step CacheModel.update.  Rows, server table and server versions are compared bit for bit EVERY
step; resident set / versions / update counters / data and gradient rows of every line whenever no bookkeeping has run ahead of
the rows (the end of a block that was planned alone; after the closing step otherwise).

Reference: CacheBase::_embeddingPushPull (src/hetu_cache/src/cache.cc:356-422), the server's push-then-sync handler
(ps-lite/src/PSFhandle_embedding.cc:66-79), LRUCache (src/hetu_cache/src/lru_cache.cc:5-39)."""
import numpy as np
import pytest
import torch

from herald_amd import _lib
from herald_amd import cache as hcache
from oracle import cache_model
from test_gpu_cache import _compare_state
from test_gpu_cache_planned import _draw, _setup

pytestmark = pytest.mark.gpu

REFUSED = (ValueError, _lib.HeraldAmdError)


def _count_cases(model, pull, push, stats):
    """What the step that is about to run will meet, counted on the model BEFORE the step."""
    res = model.resident()
    up, uq = set(int(k) for k in np.unique(pull)), {}
    for k in push:
        uq[int(k)] = uq.get(int(k), 0) + 1
    srv = model.server
    # (b) a line evicted by the step before is pushed by this step, and its key is pulled again (a miss) in the same step
    stats["evicted_key_pulled_again"] += len({ln.key for ln in model.evict} & up)
    for k in up:
        ln = res.get(k)
        if ln is None:
            continue
        if k in uq:
            stats["pulled_and_pushed"] += 1
            upd = ln.updates + uq[k]
            if upd > model.push_bound and srv.ver[k] - ln.version <= model.pull_bound < srv.ver[k] + upd - ln.version:
                stats["pulled_back_by_own_push"] += 1
        elif ln.grad is not None and np.any(ln.grad) and srv.ver[k] - ln.version > model.pull_bound:
            stats["addup_with_gradient"] += 1


def _new_stats():
    return {"evicted_key_pulled_again": 0, "pulled_and_pushed": 0, "pulled_back_by_own_push": 0, "addup_with_gradient": 0}


def _check_perf_last(gpu, model, step):
    got, exp = gpu.perf[-1], model.perf[-1]
    for f in ("type", "num_all", "num_unique", "num_miss", "num_transfered", "is_full"):
        assert got[f] == exp[f], (step, f, got, exp)
    if exp["type"] == "Push":
        assert got["num_evict"] == exp["num_evict"], (step, got, exp)


def _second_writer(rng, model, server, table, versions, bump):
    """Another worker pushes to rows whose lines hold unpushed gradients here (on the row stream, between two steps)."""
    cand = sorted(k for k, ln in model.resident().items() if ln.updates > 0)
    if not cand:
        return
    idx = np.array(cand[::2], dtype=np.int64)
    delta = rng.standard_normal((idx.size, table.shape[1]), dtype=np.float32) * np.float32(0.05)
    server.table[idx] = (server.table[idx] + delta).astype(np.float32)
    server.ver[idx] += bump
    dev = table.device
    ti = torch.from_numpy(idx).to(dev)
    table[ti] = table[ti] + torch.from_numpy(delta).to(dev)
    versions[ti] = versions[ti] + bump


def _chain_step(dev, gpu, model, e, steps, keys_all, grads_all, width, versions, server):
    """Entry e of the chain (None: the closing one) on the model and on the cache; the rows are compared."""
    if e is None:
        model.update(keys_all[steps - 1].astype(np.uint64), grads_all[steps - 1])
        gpu.embedding_update_planned(torch.from_numpy(grads_all[steps - 1]).to(dev)).wait()
        _check_perf_last(gpu, model, steps)
        return
    keys = keys_all[e]
    dest = torch.empty((keys.size, width), dtype=torch.float32, device=dev)
    if e == 0:
        want = model.lookup(keys.astype(np.uint64))
        gpu.embedding_lookup_planned(dest).wait()
        _check_perf_last(gpu, model, e)
    else:
        want = model.push_pull(keys.astype(np.uint64), keys_all[e - 1].astype(np.uint64), grads_all[e - 1])
        gpu.embedding_push_pull_planned(dest, torch.from_numpy(grads_all[e - 1]).to(dev)).wait()
    np.testing.assert_array_equal(dest.cpu().numpy(), want, err_msg="pulled rows at step %d" % e)


def _run_chain(dev, limit, rows, width, n, steps, pull_bound, push_bound, block, seed=0, zipf=True, ahead=True,
               dtype=np.float32, sizes=None, light=False, second_writer=0, hot=None):
    """`steps` batches: a head, steps - 1 push-pull steps, the closing step -- steps + 1 entries in blocks of `block`.
    ahead / light: as _run_planned of test_gpu_cache_planned.py.  second_writer = k > 0: see _second_writer (versions + k).
    hot = (key, times): that key that often in every batch (a long run of the accumulate)."""
    rng, server, model, table, versions, gpu = _setup(dev, limit, rows, width, n, pull_bound, push_bound, seed)
    sizes = sizes or [n] * steps
    keys_all = [_draw(rng, m, rows, zipf) for m in sizes]
    if hot is not None:
        for k in keys_all:
            k[:hot[1]] = hot[0]
    grads_all = [rng.standard_normal((m, width), dtype=np.float32) * np.float32(-0.01) for m in sizes]
    kts = [torch.from_numpy(k.astype(dtype)).to(dev) for k in keys_all]
    entries = list(range(steps)) + [None]
    blocks = [entries[b0:b0 + block] for b0 in range(0, len(entries), block)]
    stats = _new_stats()

    def plan(blk):
        gpu.plan_block([kts[e] if e is not None else None for e in blk], push_pull=True)

    if ahead:
        plan(blocks[0])
    for j, blk in enumerate(blocks):
        if ahead and j + 1 < len(blocks):
            plan(blocks[j + 1])
        elif not ahead:
            plan(blk)
        for e in blk:
            nperf = len(gpu.perf)
            if e is not None and e > 0:
                _count_cases(model, keys_all[e], keys_all[e - 1], stats)
            _chain_step(dev, gpu, model, e, steps, keys_all, grads_all, width, versions, server)
            assert len(gpu.perf) == nperf + (1 if e is None or e == 0 else 0)       # a push-pull step appends no record
            step = steps if e is None else e
            np.testing.assert_array_equal(versions.cpu().numpy(), server.ver, err_msg="server versions step %d" % step)
            if not light:
                np.testing.assert_array_equal(table.cpu().numpy(), server.table, err_msg="server table step %d" % step)
            if second_writer and e is not None:
                _second_writer(rng, model, server, table, versions, second_writer)
        if not ahead or j + 1 == len(blocks):
            assert gpu.plan_pending() == 0
            if not light:
                _compare_state(gpu, model, blk[-1] if blk[-1] is not None else steps)
    np.testing.assert_array_equal(table.cpu().numpy(), server.table, err_msg="server table at the end")
    st = gpu.state()
    assert st["size"] == model.policy.size() and st["pending_evictions"] == 0 and len(model.evict) == 0
    np.testing.assert_array_equal(gpu.keys(), np.array(model.policy.keys(), dtype=np.uint64))
    return gpu, model, stats


@pytest.mark.parametrize("pull_bound,push_bound", [(0, 0), (3, 3), (1, 5), (100, 100)])
@pytest.mark.parametrize("block,ahead", [(1, False), (4, False), (16, True), (5, True)])
def test_push_pull_chain_lru_trace(dev, pull_bound, push_bound, block, ahead):
    _run_chain(dev, limit=128, rows=1500, width=8, n=64, steps=64, pull_bound=pull_bound, push_bound=push_bound, block=block,
               seed=11, ahead=ahead)


@pytest.mark.parametrize("ahead", [False, True])
def test_push_pull_chain_evicted_key_is_pulled_again_in_the_step_that_pushes_it(dev, ahead):
    # limit == n_pull + n_push: every insert evicts; the evicted dirty lines wait one step, and some keys come back at once
    _, _, stats = _run_chain(dev, limit=128, rows=1000, width=4, n=64, steps=64, pull_bound=2, push_bound=2, block=8, seed=3,
                             zipf=False, ahead=ahead)
    assert stats["evicted_key_pulled_again"] > 0, stats


def test_push_pull_chain_line_pulled_back_because_of_its_own_push(dev):
    _, _, stats = _run_chain(dev, limit=128, rows=1500, width=8, n=64, steps=64, pull_bound=2, push_bound=2, block=6, seed=5)
    assert stats["pulled_and_pushed"] > 0 and stats["pulled_back_by_own_push"] > 0, stats


@pytest.mark.parametrize("ahead", [False, True])
def test_push_pull_chain_second_writer_makes_lines_with_gradients_stale(dev, ahead):
    _, _, stats = _run_chain(dev, limit=160, rows=1500, width=8, n=64, steps=40, pull_bound=1, push_bound=6, block=4, seed=17,
                             ahead=ahead, second_writer=3)
    assert stats["addup_with_gradient"] > 0, stats


def test_push_pull_chain_criteo_width_and_long_runs(dev):
    # width 128 with medium runs; width 512 with one key several hundred times per batch: the cooperative long-run path of the
    # accumulate with the push epilogue (the hot key is pulled AND pushed by every step: its gradient row is kept for addup)
    _run_chain(dev, limit=1000, rows=5000, width=128, n=416, steps=12, pull_bound=2, push_bound=2, block=4, seed=24)
    _, _, stats = _run_chain(dev, limit=5000, rows=6000, width=512, n=2000, steps=6, pull_bound=1, push_bound=2, block=3,
                             seed=25, hot=(77, 600))
    assert stats["pulled_back_by_own_push"] > 0, stats


def test_push_pull_chain_odd_width_takes_the_scalar_kernels(dev):
    _run_chain(dev, limit=200, rows=900, width=10, n=96, steps=20, pull_bound=1, push_bound=1, block=5, seed=8)


def test_push_pull_chain_ragged_empty_batches_and_int64_keys(dev):
    sizes = [64, 1, 0, 33, 64, 0, 0, 17, 64, 2]
    _run_chain(dev, limit=128, rows=700, width=8, n=64, steps=len(sizes), pull_bound=1, push_bound=1, block=4, seed=9,
               dtype=np.int64, sizes=sizes)
    _run_chain(dev, limit=128, rows=700, width=8, n=64, steps=len(sizes), pull_bound=1, push_bound=1, block=3, seed=10,
               dtype=np.int64, sizes=sizes, ahead=False)


def test_push_pull_chain_many_keys_per_bookkeeping_thread(dev):
    _run_chain(dev, limit=45000, rows=120000, width=4, n=20000, steps=6, pull_bound=1, push_bound=2, block=3, seed=31,
               zipf=False, ahead=True, light=True)


def test_push_pull_chain_equals_call_by_call(dev):
    limit, rows, width, n, steps, block = 128, 1200, 8, 64, 40, 6
    rng, server, model, table, versions, gpu = _setup(dev, limit, rows, width, n, 2, 3, seed=41)
    table2, versions2 = table.clone(), versions.clone()
    ref = hcache.LRUCache(limit, rows, width, node_id=1, max_batch=n, device=dev)
    ref.bind_store(table2, versions2)
    ref.pull_bound, ref.push_bound = 2, 3
    keys_all = [_draw(rng, n, rows, True) for _ in range(steps)]
    grads = [torch.from_numpy(rng.standard_normal((n, width), dtype=np.float32) * np.float32(0.01)).to(dev) for _ in range(steps)]
    kts = [torch.from_numpy(k.astype(np.float32)).to(dev) for k in keys_all]
    entries = kts + [None]
    blocks = [entries[b0:b0 + block] for b0 in range(0, len(entries), block)]
    gpu.plan_block(blocks[0], push_pull=True)
    e = 0
    for j, blk in enumerate(blocks):
        if j + 1 < len(blocks):
            gpu.plan_block(blocks[j + 1], push_pull=True)
        for k in blk:
            d1 = torch.empty((n, width), device=dev)
            d2 = torch.empty((n, width), device=dev)
            if k is None:
                gpu.embedding_update_planned(grads[e - 1]).wait()
                ref.embedding_update(kts[e - 1], grads[e - 1]).wait()
            elif e == 0:
                gpu.embedding_lookup_planned(d1).wait()
                ref.embedding_lookup(k, d2).wait()
            else:
                gpu.embedding_push_pull_planned(d1, grads[e - 1]).wait()
                ref.embedding_push_pull(k, d2, kts[e - 1], grads[e - 1]).wait()
            if k is not None:
                np.testing.assert_array_equal(d1.cpu().numpy(), d2.cpu().numpy(), err_msg="rows at step %d" % e)
            e += 1
    np.testing.assert_array_equal(table.cpu().numpy(), table2.cpu().numpy())
    np.testing.assert_array_equal(versions.cpu().numpy(), versions2.cpu().numpy())
    a, b = gpu.lines(), ref.lines()
    assert sorted(a) == sorted(b)
    for key in a:
        assert (a[key].version, a[key].updates) == (b[key].version, b[key].updates), key
        np.testing.assert_array_equal(a[key].data, b[key].data)
        np.testing.assert_array_equal(a[key].grad, b[key].grad)


def test_push_pull_chain_life_cycle(dev):
    """Head by embedding_lookup_planned, close by a None entry + embedding_update_planned; afterwards call-by-call calls and a
    planned PAIR block work and match the model, and a new chain can start."""
    limit, rows, width, n = 128, 900, 8, 48
    rng, server, model, table, versions, gpu = _setup(dev, limit, rows, width, n, 1, 2, seed=51)

    def batch():
        k = _draw(rng, n, rows, True)
        return k, torch.from_numpy(k.astype(np.float32)).to(dev), rng.standard_normal((n, width), dtype=np.float32) * np.float32(0.01)

    def chain(nb, split):
        bs = [batch() for _ in range(nb)]
        keys_all, kts, grads_all = [b[0] for b in bs], [b[1] for b in bs], [b[2] for b in bs]
        gpu.plan_block(kts[:split], push_pull=True)
        assert gpu.plan_pending() == split
        for e in range(split):
            _chain_step(dev, gpu, model, e, nb, keys_all, grads_all, width, versions, server)
        assert gpu.plan_pending() == 0
        gpu.plan_block(kts[split:] + [None], push_pull=True)
        for e in list(range(split, nb)) + [None]:
            _chain_step(dev, gpu, model, e, nb, keys_all, grads_all, width, versions, server)
        _compare_state(gpu, model, nb)
        np.testing.assert_array_equal(table.cpu().numpy(), server.table)

    nperf = len(gpu.perf)
    chain(5, 2)
    assert [p["type"] for p in gpu.perf[nperf:]] == ["Pull", "Push"]
    # call by call
    k, kt, g = batch()
    dest = torch.empty((n, width), device=dev)
    want = model.lookup(k.astype(np.uint64))
    gpu.embedding_lookup(kt, dest).wait()
    np.testing.assert_array_equal(dest.cpu().numpy(), want)
    model.update(k.astype(np.uint64), g)
    gpu.embedding_update(kt, torch.from_numpy(g).to(dev)).wait()
    _compare_state(gpu, model, 100)
    # a planned pair block
    k, kt, g = batch()
    gpu.plan_block([kt])
    want = model.lookup(k.astype(np.uint64))
    gpu.embedding_lookup_planned(dest).wait()
    np.testing.assert_array_equal(dest.cpu().numpy(), want)
    model.update(k.astype(np.uint64), g)
    gpu.embedding_update_planned(torch.from_numpy(g).to(dev)).wait()
    _compare_state(gpu, model, 101)
    # and a new chain, closed by a block whose only entry is the closing one
    bs = [batch() for _ in range(3)]
    keys_all, kts, grads_all = [b[0] for b in bs], [b[1] for b in bs], [b[2] for b in bs]
    gpu.plan_block(kts, push_pull=True)
    for e in range(3):
        _chain_step(dev, gpu, model, e, 3, keys_all, grads_all, width, versions, server)
    gpu.plan_block([None], push_pull=True)
    assert gpu.plan_pending() == 1
    _chain_step(dev, gpu, model, None, 3, keys_all, grads_all, width, versions, server)
    _compare_state(gpu, model, 102)
    np.testing.assert_array_equal(table.cpu().numpy(), server.table)
    np.testing.assert_array_equal(versions.cpu().numpy(), server.ver)


def test_push_pull_chain_reads_ids_written_on_the_row_stream_just_before(dev):
    """Ids written by kernels on the row stream right before each plan_block, behind a long launch, for 8 blocks."""
    limit, rows, width, n, block, nblk = 200, 3000, 8, 96, 3, 8
    rng, server, model, table, versions, gpu = _setup(dev, limit, rows, width, n, 2, 2, seed=111)
    steps = block * nblk
    keys_all = [_draw(rng, n, rows, True) for _ in range(steps)]
    grads_all = [rng.standard_normal((n, width), dtype=np.float32) * np.float32(0.01) for _ in range(steps)]
    src = [torch.from_numpy((k + 7 * rows).astype(np.float32)).to(dev) for k in keys_all]
    dst = [torch.zeros(n, dtype=torch.float32, device=dev) for _ in range(steps)]      # zeros until the row stream writes
    big = torch.randn((2048, 2048), device=dev)
    torch.cuda.synchronize()

    def plan(b):
        with torch.cuda.stream(gpu._stream()):
            for _ in range(4):
                big.copy_(big @ big * 1e-3)      # a long launch in front of the writes
            for st in range(b * block, (b + 1) * block):
                torch.remainder(src[st], float(rows), out=dst[st])       # ids % rows
        gpu.plan_block(dst[b * block:(b + 1) * block] + ([None] if b + 1 == nblk else []), push_pull=True)

    plan(0)
    for b in range(nblk):
        if b + 1 < nblk:
            plan(b + 1)
        for st in range(b * block, (b + 1) * block):
            _chain_step(dev, gpu, model, st, steps, keys_all, grads_all, width, versions, server)
            np.testing.assert_array_equal(versions.cpu().numpy(), server.ver)
    _chain_step(dev, gpu, model, None, steps, keys_all, grads_all, width, versions, server)
    assert gpu.plan_pending() == 0
    _compare_state(gpu, model, steps)
    np.testing.assert_array_equal(table.cpu().numpy(), server.table)


def _state_of(gpu, table, versions):
    lines = gpu.lines()
    return ({k: (ln.version, ln.updates, ln.data.copy(), ln.grad.copy()) for k, ln in lines.items()}, gpu.state(),
            table.cpu().numpy().copy(), versions.cpu().numpy().copy(), gpu.plan_pending())


def _assert_same_state(a, b):
    assert sorted(a[0]) == sorted(b[0]) and a[1] == b[1] and a[4] == b[4]
    for k in a[0]:
        assert a[0][k][:2] == b[0][k][:2]
        np.testing.assert_array_equal(a[0][k][2], b[0][k][2])
        np.testing.assert_array_equal(a[0][k][3], b[0][k][3])
    np.testing.assert_array_equal(a[2], b[2])
    np.testing.assert_array_equal(a[3], b[3])


@pytest.mark.parametrize("policy", ["lfu", "lfuopt"])
def test_push_pull_chain_refuses_the_lfu_policies(dev, policy):
    rows, width, n = 500, 8, 32
    rng, server, model, table, versions, gpu = _setup(dev, 128, rows, width, n, 2, 2, seed=61, policy=policy)
    kt = torch.from_numpy(_draw(rng, n, rows, True).astype(np.float32)).to(dev)
    dest = torch.empty((n, width), device=dev)
    gpu.embedding_lookup(kt, dest).wait()
    gpu.embedding_update(kt, torch.full((n, width), 0.01, device=dev)).wait()
    before = _state_of(gpu, table, versions)
    with pytest.raises(REFUSED, match="LRU"):
        gpu.plan_block([kt], push_pull=True)
    _assert_same_state(before, _state_of(gpu, table, versions))
    # and the call-by-call push-pull still works
    gpu.embedding_push_pull(kt, dest, kt, torch.full((n, width), 0.01, device=dev)).wait()


def test_push_pull_chain_refuses_misuse_and_leaves_the_cache_unchanged(dev):
    rows, width, n, limit = 500, 8, 48, 100
    rng, server, model, table, versions, gpu = _setup(dev, limit, rows, width, n, 2, 2, seed=71)
    ks = [torch.from_numpy(_draw(rng, n, rows, True).astype(np.float32)).to(dev) for _ in range(4)]
    dest = torch.empty((n, width), device=dev)
    g = torch.full((n, width), 0.01, device=dev)
    # a first pair, so that the state is not empty
    gpu.embedding_lookup(ks[0], dest).wait()
    gpu.embedding_update(ks[0], g).wait()
    before = _state_of(gpu, table, versions)
    big = torch.arange(limit - n + 1, dtype=torch.float32, device=dev)
    with pytest.raises(REFUSED, match="limit"):              # n_pull + n_push > limit (second step)
        gpu.plan_block([ks[1], torch.cat([ks[2], ks[3]])[:limit - n + 1]], push_pull=True)
    with pytest.raises(REFUSED, match="limit"):
        gpu.plan_block([big, ks[1]], push_pull=True)
    with pytest.raises(REFUSED):                              # None not last
        gpu.plan_block([ks[1], None, ks[2]], push_pull=True)
    with pytest.raises(REFUSED):                              # nothing to close
        gpu.plan_block([None], push_pull=True)
    with pytest.raises(REFUSED):                              # push keys in a chain
        gpu.plan_block([ks[1]], push_keys_list=[ks[1]], push_pull=True)
    gpu.bypass()
    with pytest.raises(REFUSED, match="bypass"):
        gpu.plan_block([ks[1]], push_pull=True)
    gpu.undo_bypass()
    _assert_same_state(before, _state_of(gpu, table, versions))
    # a remote cache
    rem = hcache.LRUCache(limit, rows, width, node_id=3, max_batch=n, device=dev)
    with pytest.raises(REFUSED):
        rem.plan_block([ks[1]], push_pull=True)
    # an open chain: the head is due
    gpu.plan_block(ks[1:3], push_pull=True)
    with pytest.raises(REFUSED):
        gpu.embedding_push_pull_planned(dest, g)
    with pytest.raises(REFUSED):
        gpu.embedding_update_planned(g)
    assert gpu.plan_pending() == 2
    gpu.embedding_lookup_planned(dest).wait()
    with pytest.raises(REFUSED):                              # wrong sizes
        gpu.embedding_push_pull_planned(dest[:-1], g)
    with pytest.raises(REFUSED):
        gpu.embedding_push_pull_planned(dest, g[:-1])
    with pytest.raises(REFUSED):
        gpu.embedding_lookup_planned(dest)
    assert gpu.plan_pending() == 1
    gpu.embedding_push_pull_planned(dest, g).wait()
    # the chain is open, nothing is outstanding: call-by-call methods and pair blocks are refused, and say how to close it
    assert gpu.plan_pending() == 0
    torch.cuda.synchronize()
    mid = _state_of(gpu, table, versions)
    with pytest.raises(REFUSED, match="clos"):
        gpu.embedding_lookup(ks[3], dest)
    with pytest.raises(REFUSED, match="clos"):
        gpu.embedding_update(ks[2], g)
    with pytest.raises(REFUSED, match="clos"):
        gpu.embedding_push_pull(ks[3], dest, ks[2], g)
    with pytest.raises(REFUSED, match="clos"):
        gpu.prefetch_keys(ks[3])
    with pytest.raises(REFUSED, match="clos"):
        gpu.plan_block([ks[3]])
    with pytest.raises(REFUSED, match="clos"):
        gpu.plan_block([ks[3]], push_keys_list=[ks[3]])
    _assert_same_state(mid, _state_of(gpu, table, versions))
    gpu.plan_block([None], push_pull=True)
    gpu.embedding_update_planned(g).wait()
    gpu.embedding_lookup(ks[3], dest).wait()
    gpu.embedding_update(ks[3], g).wait()


def test_cache_destroyed_with_planned_chain_steps_outstanding(dev):
    rows, width, n = 500, 8, 48
    rng, server, model, table, versions, gpu = _setup(dev, 128, rows, width, n, 2, 2, seed=81)
    ks = [torch.from_numpy(_draw(rng, n, rows, True).astype(np.float32)).to(dev) for _ in range(3)]
    gpu.plan_block(ks, push_pull=True)
    dest = torch.empty((n, width), device=dev)
    gpu.embedding_lookup_planned(dest).wait()
    assert gpu.plan_pending() == 2
    del gpu
    torch.cuda.synchronize()

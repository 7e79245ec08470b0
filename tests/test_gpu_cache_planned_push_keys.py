"""The PLANNED flow with push keys (ha_cache_plan_block_push_keys, csrc/cache_block.hip) against oracle/cache_model.py's
update_with_push_keys -- the comparisons of tests/test_gpu_cache_planned.py: lookup rows bit for bit and the perf dict's counts
every step, server table and versions every step, the whole line state at block ends with nothing planned ahead.  And against
the call-by-call embedding_update_with_push_keys on a second cache, bit for bit (a yardstick that does not need the model).

Reference: CacheBase::_embeddingUpdateWithPushKeys (src/hetu_cache/src/cache.cc:248-335): a line is pushed iff its key is a
push key and it holds data; every line's version += its counter; only pushed lines start again at 0."""
import numpy as np
import pytest
import torch

from herald_amd import cache as hcache
from test_gpu_cache import _compare_state
from test_gpu_cache_planned import STATS, _check_perf, _draw, _setup

pytestmark = pytest.mark.gpu

MODES = ("third", "empty", "all", "absent", "beyond", "dups")


def _push_set(rng, keys, mode, rows):
    u = np.unique(keys.astype(np.int64))
    third = np.sort(rng.choice(u, size=u.size // 3, replace=False)) if u.size else u
    if mode == "mixed":
        mode = MODES[int(rng.integers(0, len(MODES)))]
    if mode == "third":
        return third
    if mode == "empty":
        return u[:0]
    if mode == "all":
        return u
    if mode == "absent":
        return np.setdiff1d(rng.integers(0, rows, size=24), u)
    if mode == "beyond":
        return np.concatenate([third, rows + np.arange(4)])
    if mode == "dups":
        return np.sort(np.concatenate([third, third[::2]]))
    raise ValueError(mode)


def _pk_step(dev, gpu, model, keys, pk, grads, width, step, versions, server):
    res = model.resident()
    held = {int(k): res[int(k)].updates for k in np.unique(keys) if int(k) in res}
    want = model.lookup(keys.astype(np.uint64))
    gone = [k for k in held if not model.policy.count(k)]
    STATS["own_line_evicted"] += len(gone)
    STATS["own_line_evicted_dirty"] += sum(1 for k in gone if held[k] != 0)
    dest = torch.empty((keys.size, width), dtype=torch.float32, device=dev)
    gpu.embedding_lookup_planned(dest).wait()
    np.testing.assert_array_equal(dest.cpu().numpy(), want, err_msg="lookup rows at step %d" % step)
    if pk is None:
        model.update(keys.astype(np.uint64), grads)
    else:
        model.update_with_push_keys(keys.astype(np.uint64), pk.astype(np.uint64), grads)
    gpu.embedding_update_planned(torch.from_numpy(grads).to(dev)).wait()
    STATS["update_misses"] += model.perf[-1]["num_miss"]
    _check_perf(gpu, model, step)
    np.testing.assert_array_equal(versions.cpu().numpy(), server.ver, err_msg="server versions step %d" % step)


def _run_pk(dev, limit, rows, width, n, steps, pull_bound, push_bound, block, seed=0, zipf=True, ahead=True,
            dtype=np.float32, pdtype=np.float32, sizes=None, policy="lru", mode="third", bound_every=0, light=False):
    """As test_gpu_cache_planned._run_planned, every batch with push keys (`mode`, see _push_set); bound_every = m > 0: every
    m-th batch is planned in bound mode instead (mixed blocks)."""
    rng, server, model, table, versions, gpu = _setup(dev, limit, rows, width, n, pull_bound, push_bound, seed, policy)
    sizes = sizes or [n] * steps
    keys_all = [_draw(rng, m, rows, zipf) for m in sizes]
    pks = [None if bound_every and s % bound_every == 0 else _push_set(rng, keys_all[s], mode, rows) for s in range(steps)]
    kts = [torch.from_numpy(k.astype(dtype)).to(dev) for k in keys_all]
    pts = [None if p is None else torch.from_numpy(p.astype(pdtype)).to(dev) for p in pks]
    blocks = [list(range(b0, min(b0 + block, steps))) for b0 in range(0, steps, block)]

    def plan(blk):
        gpu.plan_block([kts[s] for s in blk], push_keys_list=[pts[s] for s in blk])

    if ahead:
        plan(blocks[0])
    for j, blk in enumerate(blocks):
        if ahead and j + 1 < len(blocks):
            plan(blocks[j + 1])
        elif not ahead:
            plan(blk)
        for step in blk:
            grads = rng.standard_normal((sizes[step], width), dtype=np.float32) * np.float32(-0.01)
            _pk_step(dev, gpu, model, keys_all[step], pks[step], grads, width, step, versions, server)
            if not light:
                np.testing.assert_array_equal(table.cpu().numpy(), server.table, err_msg="server table step %d" % step)
        if not ahead or j + 1 == len(blocks):
            assert gpu.plan_pending() == 0
            if not light:
                _compare_state(gpu, model, blk[-1])
    np.testing.assert_array_equal(table.cpu().numpy(), server.table, err_msg="server table at the end")
    assert gpu.size() == model.policy.size()
    np.testing.assert_array_equal(gpu.keys(), np.array(model.policy.keys(), dtype=np.uint64))
    return gpu, model


@pytest.mark.parametrize("pull_bound,push_bound", [(0, 0), (3, 3), (5, 100)])
@pytest.mark.parametrize("block,ahead", [(1, False), (4, False), (16, True)])
def test_planned_push_keys_lru_trace(dev, pull_bound, push_bound, block, ahead):
    # push_bound plays no part: the same push sets give the model's results whatever it is
    _run_pk(dev, limit=100, rows=1500, width=8, n=64, steps=48, pull_bound=pull_bound, push_bound=push_bound, block=block,
            seed=71, ahead=ahead)


@pytest.mark.parametrize("mode", MODES)
def test_planned_push_keys_lru_push_sets(dev, mode):
    _run_pk(dev, limit=100, rows=1500, width=8, n=64, steps=24, pull_bound=1, push_bound=1, block=5, seed=72, mode=mode)


@pytest.mark.parametrize("dtype,pdtype", [(np.float32, np.int64), (np.int64, np.float32), (np.int64, np.int64)])
def test_planned_push_keys_dtypes_ragged_and_empty_batches(dev, dtype, pdtype):
    sizes = [64, 1, 0, 33, 64, 0, 0, 17, 64, 2]
    _run_pk(dev, limit=100, rows=700, width=8, n=64, steps=len(sizes), pull_bound=1, push_bound=1, block=4, seed=73,
            dtype=dtype, pdtype=pdtype, sizes=sizes, mode="mixed")


@pytest.mark.parametrize("policy", ["lru", "lfu", "lfuopt"])
def test_planned_push_keys_mixed_blocks(dev, policy):
    """Bound-mode and push-key batches in one block: the first follow model.update, the others update_with_push_keys."""
    _run_pk(dev, limit=100, rows=1500, width=8, n=64, steps=40, pull_bound=2, push_bound=2, block=8, seed=74, policy=policy,
            mode="mixed", bound_every=3)
    _run_pk(dev, limit=100, rows=1500, width=8, n=64, steps=24, pull_bound=2, push_bound=0, block=16, seed=75, policy=policy,
            mode="third", bound_every=2, ahead=False)


@pytest.mark.parametrize("policy", ["lfu", "lfuopt"])
@pytest.mark.parametrize("limit", [1, 7, 40])
def test_planned_push_keys_lfu_cache_smaller_than_the_batch(dev, policy, limit):
    """limit < batch: push sets that name the keys whose inserts do not stay and the key of the line the batch's own first insert
    evicts -- lines without data, NOT pushed (their gradients dropped; the evicted line itself pushed as an eviction)."""
    before = dict(STATS)
    _run_pk(dev, limit=limit, rows=300, width=8, n=64, steps=40, pull_bound=1, push_bound=3, block=4, seed=80 + limit,
            ahead=False, policy=policy, mode="all")
    _run_pk(dev, limit=limit, rows=300, width=8, n=64, steps=40, pull_bound=1, push_bound=0, block=16, seed=90 + limit,
            zipf=False, ahead=True, policy=policy, mode="mixed")
    assert STATS["update_misses"] > before["update_misses"] + 100
    assert STATS["own_line_evicted"] > before["own_line_evicted"], STATS
    if limit in (1, 7):
        assert STATS["own_line_evicted_dirty"] > before["own_line_evicted_dirty"], STATS


@pytest.mark.parametrize("policy", ["lru", "lfu", "lfuopt"])
def test_planned_push_keys_width_512_long_runs_and_odd_width(dev, policy):
    _run_pk(dev, limit=2500 if policy == "lru" else 900, rows=6000, width=512, n=2000, steps=6, pull_bound=1, push_bound=2,
            block=3, seed=76, policy=policy)
    _run_pk(dev, limit=120, rows=900, width=10, n=96, steps=20, pull_bound=1, push_bound=1, block=5, seed=77, policy=policy,
            mode="mixed")


def _pair(dev, policy, limit, rows, width, n, seed):
    rng = np.random.default_rng(seed)
    table0 = rng.standard_normal((rows, width), dtype=np.float32)
    out = []
    cls = {"lru": hcache.LRUCache, "lfu": hcache.LFUCache, "lfuopt": hcache.LFUOptCache}[policy]
    for _ in range(2):
        t = torch.from_numpy(table0.copy()).to(dev)
        v = torch.zeros(rows, dtype=torch.int64, device=dev)
        c = cls(limit, rows, width, node_id=0, max_batch=n, device=dev)
        c.bind_store(t, v)
        c.pull_bound, c.push_bound = 2, 2
        out.append((c, t, v))
    return rng, out


def _same_state(a, b):
    sa, sb = a.state(), b.state()
    assert a.keys().tolist() == b.keys().tolist()
    la, lb = a.lines(), b.lines()
    assert sorted(la) == sorted(lb)
    for k in la:
        ea, eb = la[k], lb[k]
        assert (ea.version, ea.updates) == (eb.version, eb.updates), k
        np.testing.assert_array_equal(ea.data, eb.data)
        if ea.grad is None or eb.grad is None:
            assert ea.grad is None and eb.grad is None
        else:
            np.testing.assert_array_equal(ea.grad, eb.grad)
    assert sa["size"] == sb["size"]


@pytest.mark.parametrize("policy", ["lru", "lfu", "lfuopt"])
def test_planned_push_keys_equal_call_by_call(dev, policy):
    """Two caches, the same inputs: planned push-key blocks on one, embedding_lookup + embedding_update_with_push_keys on the
    other; rows, store table and versions, every line: bit-identical.  Then planned blocks alternate with call-by-call pairs."""
    limit, rows, width, n = (100 if policy == "lru" else 40), 1500, 16, 64
    rng, ((pc, pt, pv), (cc, ct, cv)) = _pair(dev, policy, limit, rows, width, n, seed=101)

    def classic_both(count):
        for _ in range(count):
            keys = torch.from_numpy(_draw(rng, n, rows, True).astype(np.float32)).to(dev)
            pk = torch.from_numpy(_push_set(rng, keys.cpu().numpy(), "mixed", rows).astype(np.float32)).to(dev)
            g = torch.from_numpy(rng.standard_normal((n, width), dtype=np.float32) * np.float32(0.01)).to(dev)
            d0, d1 = torch.empty((n, width), device=dev), torch.empty((n, width), device=dev)
            pc.embedding_lookup(keys, d0).wait()
            cc.embedding_lookup(keys, d1).wait()
            assert torch.equal(d0, d1)
            pc.embedding_update_with_push_keys(keys, pk, g).wait()
            cc.embedding_update_with_push_keys(keys, pk, g).wait()

    def planned(count, blocks):
        ks = [[torch.from_numpy(_draw(rng, n, rows, True).astype(np.float32)).to(dev) for _ in range(count)]
              for _ in range(blocks)]
        ps = [[torch.from_numpy(_push_set(rng, k.cpu().numpy(), "mixed", rows).astype(np.int64)).to(dev) for k in blk]
              for blk in ks]
        pc.plan_block(ks[0], push_keys_list=ps[0])
        for b in range(blocks):
            if b + 1 < blocks:
                pc.plan_block(ks[b + 1], push_keys_list=ps[b + 1])
            for k, p in zip(ks[b], ps[b]):
                g = torch.from_numpy(rng.standard_normal((n, width), dtype=np.float32) * np.float32(0.01)).to(dev)
                d0, d1 = torch.empty((n, width), device=dev), torch.empty((n, width), device=dev)
                pc.embedding_lookup_planned(d0)
                cc.embedding_lookup(k, d1)
                pc.embedding_update_planned(g)
                cc.embedding_update_with_push_keys(k, p, g)
                torch.cuda.synchronize()
                assert torch.equal(d0, d1)
                assert torch.equal(pv, cv)
        assert torch.equal(pt, ct)
        _same_state(pc, cc)

    planned(6, 3)
    classic_both(5)
    planned(4, 2)
    classic_both(3)
    planned(16, 2)
    assert torch.equal(pt, ct) and torch.equal(pv, cv)
    _same_state(pc, cc)


@pytest.mark.parametrize("policy", ["lru", "lfu"])
def test_planned_push_keys_read_ids_written_on_the_row_stream_just_before(dev, policy):
    """Ids and push keys written by kernels on the row stream right before each plan_block, behind a long launch, for 8 blocks
    (past the first blocks, which ha_cache_plan_block orders behind the row stream anyway): the bookkeeping reads them as
    written -- every result equals the model's."""
    limit, rows, width, n, block, nblk = 200, 3000, 8, 96, 3, 8
    rng, server, model, table, versions, gpu = _setup(dev, limit, rows, width, n, 2, 2, seed=111, policy=policy)
    steps = block * nblk
    keys_all = [_draw(rng, n, rows, True) for _ in range(steps)]
    pks = [_push_set(rng, k, "third", rows) for k in keys_all]
    src_k = [torch.from_numpy(k.astype(np.float32)).to(dev) for k in keys_all]
    src_p = [torch.from_numpy(p.astype(np.float32)).to(dev) for p in pks]
    dst_k = [torch.zeros(n, dtype=torch.float32, device=dev) for _ in range(steps)]       # zeros until the row stream writes
    dst_p = [torch.zeros(p.size, dtype=torch.float32, device=dev) for p in pks]
    big = torch.randn((2048, 2048), device=dev)
    torch.cuda.synchronize()

    def plan(b):
        s = gpu._stream()
        with torch.cuda.stream(s):
            for _ in range(4):
                big.copy_(big @ big * 1e-3)      # a long launch in front of the writes
            for st in range(b * block, (b + 1) * block):
                dst_k[st].copy_(src_k[st])
                dst_p[st].copy_(src_p[st])
        gpu.plan_block(dst_k[b * block:(b + 1) * block], push_keys_list=dst_p[b * block:(b + 1) * block])

    plan(0)
    for b in range(nblk):
        if b + 1 < nblk:
            plan(b + 1)
        for st in range(b * block, (b + 1) * block):
            grads = rng.standard_normal((n, width), dtype=np.float32) * np.float32(0.01)
            _pk_step(dev, gpu, model, keys_all[st], pks[st], grads, width, st, versions, server)
    assert gpu.plan_pending() == 0
    _compare_state(gpu, model, steps)
    np.testing.assert_array_equal(table.cpu().numpy(), server.table)


def test_planned_push_keys_refuse_misuse_and_leave_the_cache_unchanged(dev):
    rows, width, n = 500, 8, 64
    rng, server, model, table, versions, gpu = _setup(dev, 200, rows, width, n, 2, 2, seed=121)
    ks = [torch.from_numpy(_draw(rng, n, rows, True).astype(np.float32)).to(dev) for _ in range(2)]
    pk = torch.from_numpy(np.unique(ks[0].cpu().numpy())[::3].copy()).to(dev)
    # a first pair, so that the state is not empty
    gpu.plan_block(ks[:1], push_keys_list=[pk])
    dest = torch.empty((n, width), device=dev)
    gpu.embedding_lookup_planned(dest)
    gpu.embedding_update_planned(torch.ones((n, width), device=dev)).wait()
    before = (gpu.state(), gpu.keys().tolist(), table.clone(), versions.clone())
    big = torch.zeros(gpu._max_batch + 1, dtype=torch.float32, device=dev)
    with pytest.raises(ValueError):
        gpu.plan_block(ks, push_keys_list=[pk])                                      # one entry for two batches
    with pytest.raises(ValueError):
        gpu.plan_block(ks[:1], push_keys_list=[big])                                 # more than max_batch push keys
    with pytest.raises(ValueError):
        gpu.plan_block(ks[:1], push_keys_list=[pk.to(torch.int32)])                  # not float32 / int64
    with pytest.raises(ValueError):
        gpu.plan_block(ks[:1], push_keys_list=[pk.cpu()])                            # not on the device
    assert gpu.plan_pending() == 0
    torch.cuda.synchronize()
    after = (gpu.state(), gpu.keys().tolist())
    assert after[0] == before[0] and after[1] == before[1]
    assert torch.equal(table, before[2]) and torch.equal(versions, before[3])
    # and the cache still plans and runs
    gpu.plan_block(ks[1:], push_keys_list=[None])
    gpu.embedding_lookup_planned(dest)
    gpu.embedding_update_planned(torch.ones((n, width), device=dev)).wait()
    assert gpu.plan_pending() == 0

"""The pooled call-by-call cache calls over a store the cache cannot address (bind_remote): ha_cache_lookup_begin + the exchange
+ ha_cache_lookup_sum_finish, the pooled updates into the outbox, ha_cache_push_pull_begin_bags / ha_cache_push_pull_finish_sum.
  * LocalStore (host_counts = False: the request and the outbox are handed over padded) -- the traces of
    test_gpu_cache_bag_calls.py again, against oracle/cache_model.py + bag_model.bag_sum and an unfused cache;
  * the same store with host_counts = True (n_unique and the outbox count are read back);
  * ShardedStore, two processes on one GPU (host-staged all-to-all under gloo): each rank runs a pooled cache and an unfused one
    over two copies of the sharded table and is held to the unfused run and to the per-rank cache models, every step."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from herald_amd import cache as hcache
from herald_amd import remote_store
from oracle import cache_model

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_cache_bag_calls import Bags, bits, run_trace, test_push_pull as _push_pull_trace  # noqa: E402
from test_gpu_cache_remote import _bind_local, _free_port, host_staged_a2a  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _CountedStore(remote_store.LocalStore):
    host_counts = True


def _bind_counted(gpu, table, versions):
    gpu.bind_remote(_CountedStore(table, versions))


@pytest.mark.parametrize("policy", ["lru", "lfu", "lfuopt"])
@pytest.mark.parametrize("pull_bound,push_bound", [(0, 0), (3, 3)])
def test_remote_traces(dev, policy, pull_bound, push_bound):
    run_trace(dev, policy, pull_bound=pull_bound, push_bound=push_bound, seed=11, bind=_bind_local)


@pytest.mark.parametrize("policy", ["lru", "lfu"])
@pytest.mark.parametrize("variant", ["same", "pushkeys", "alternate"])
def test_remote_call_variants(dev, policy, variant):
    steps = 20
    _, fused = run_trace(dev, policy, limit=100, rows=1500, steps=steps, pull_bound=2, push_bound=2, seed=17, variant=variant,
                         bind=_bind_local)
    if variant in ("same", "alternate"):       # the two-launch update, its pushes in the outbox
        assert fused == (steps if policy == "lru" else 0)


def test_remote_limit_below_the_batch_ragged_and_wide_rows(dev):
    run_trace(dev, "lru", limit=5, rows=200, zipf=False, pull_bound=1, push_bound=1, seed=4, steps=16, bind=_bind_local)
    run_trace(dev, "lru", width=7, ragged=dict(empty=3), pull_bound=1, push_bound=2, seed=5, steps=10, bind=_bind_local)
    run_trace(dev, "lru", width=260, B=5, F=70, limit=200, rows=3000, steps=5, pull_bound=1, push_bound=2, seed=6, bind=_bind_local)


@pytest.mark.parametrize("variant", ["plain", "same", "pushkeys"])
def test_remote_store_that_counts_on_the_host(dev, variant):
    run_trace(dev, "lru", limit=100, rows=1500, steps=12, pull_bound=2, push_bound=2, seed=19, variant=variant, bind=_bind_counted)


@pytest.mark.parametrize("sides", ["both", "pull", "push", "ragged"])
@pytest.mark.parametrize("policy", ["lru", "lfu", "lfuopt"])
def test_remote_push_pull(dev, policy, sides):
    _push_pull_trace(dev, policy, sides, bind=_bind_local)


def test_remote_push_pull_counted(dev):
    _push_pull_trace(dev, "lru", "both", bind=_bind_counted)


# ---- two caches per rank over a sharded store -------------------------------------------------------------------------------
def _worker(rank, world, port, rows, width, B, F, limit, steps):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    from herald_amd.sharded import partition
    n = B * F
    rng = np.random.default_rng(99)                       # identical on every rank
    table0 = rng.standard_normal((rows, width), dtype=np.float32)
    starts = partition(rows, world)
    sides = []                                            # [pooled, unfused]: (cache, local store, shard)
    for _ in range(2):
        shard = torch.from_numpy(table0[starts[rank]:starts[rank + 1]].copy()).to(dev)
        local = remote_store.LocalStore(shard)
        store = remote_store.ShardedStore(rows, width, dev, local, a2a=host_staged_a2a)
        c = hcache.LRUCache(limit, rows, width, node_id=0, max_batch=n, device=dev)
        c.bind_remote(store)
        c.pull_bound = c.push_bound = 2
        c.perf_enabled = True
        sides.append((c, local, shard))
    (gpu, local, shard), (ref, local_ref, shard_ref) = sides
    server = cache_model.Server(table0)
    models = [cache_model.CacheModel("lru", limit, width, server, 2, 2) for _ in range(world)]
    bags = Bags(dev, n, F)

    def keys_of(step, r):
        g = np.random.default_rng(1000 * step + r)
        k = (np.minimum(g.zipf(1.25, size=n) - 1, rows - 1) * 7919) % rows
        k[: n // 5] = (np.random.default_rng(step).integers(0, rows, size=n // 5))     # shared between ranks
        return k.astype(np.float32)

    out = torch.empty((B, width), dtype=torch.float32, device=dev)
    dest = torch.empty((n, width), dtype=torch.float32, device=dev)
    for step in range(steps):
        bag_grads = [np.random.default_rng(5000 * step + r).standard_normal((B, width), dtype=np.float32) * np.float32(-0.01)
                     for r in range(world)]
        wants = [m.lookup(keys_of(step, r).astype(np.uint64)) for r, m in enumerate(models)]
        kt = torch.from_numpy(keys_of(step, rank)).to(dev)
        gpu.embedding_lookup_sum(kt, out, bag=F).wait()
        ref.embedding_lookup(kt, dest).wait()
        np.testing.assert_array_equal(bits(dest), bits(wants[rank]), err_msg="unfused rows, step %d rank %d" % (step, rank))
        np.testing.assert_array_equal(bits(out), bits(bags.sum(wants[rank])), err_msg="pooled rows, step %d rank %d" % (step, rank))
        for r, m in enumerate(models):                                      # pushes land in rank order
            m.update(keys_of(step, r).astype(np.uint64), np.ascontiguousarray(bag_grads[r][bags.of]))
        same = step % 2 == 1               # every other step reuses the lookup's plan
        uk = kt if same else torch.from_numpy(keys_of(step, rank)).to(dev)
        gpu.embedding_update_bags(uk, torch.from_numpy(bag_grads[rank]).to(dev), bag=F, same_as_lookup=same).wait()
        ref.embedding_update(uk, torch.from_numpy(np.ascontiguousarray(bag_grads[rank][bags.of])).to(dev),
                             same_as_lookup=same).wait()
        torch.cuda.synchronize()
        dist.barrier()
        for lo, sh in ((local, shard), (local_ref, shard_ref)):
            np.testing.assert_array_equal(lo.versions.cpu().numpy(), server.ver[starts[rank]:starts[rank + 1]],
                                          err_msg="versions, step %d rank %d" % (step, rank))
            np.testing.assert_array_equal(bits(sh), bits(server.table[starts[rank]:starts[rank + 1]]),
                                          err_msg="shard, step %d rank %d" % (step, rank))
        for i in (-2, -1):
            for f in ("type", "num_all", "num_unique", "num_miss", "num_transfered"):
                assert gpu.perf[i][f] == ref.perf[i][f] == models[rank].perf[i][f], (step, rank, f)
    res, lines, lines_ref = models[rank].resident(), gpu.lines(), ref.lines()
    assert sorted(lines.keys()) == sorted(res.keys()) == sorted(lines_ref.keys())
    for k, ln in res.items():
        assert lines[k].version == ln.version == lines_ref[k].version and lines[k].updates == ln.updates, k
        np.testing.assert_array_equal(bits(lines[k].data), bits(ln.data))
        np.testing.assert_array_equal(bits(lines[k].data), bits(lines_ref[k].data))
    assert int(gpu._L.ha_cache_fused_updates(gpu._h)) == int(ref._L.ha_cache_fused_updates(ref._h))
    dist.barrier()
    dist.destroy_process_group()


def test_pooled_caches_over_a_sharded_store(dev):
    mp.spawn(_worker, args=(2, _free_port(), 6000, 32, 125, 4, 600, 6), nprocs=2, join=True)

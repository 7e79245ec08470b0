"""Sum-pooled access through the cache's CALL-BY-CALL interface (embedding_lookup_sum, embedding_update_bags,
embedding_update_with_push_keys_bags, embedding_push_pull_bags), bit patterns, every step held to oracle/cache_model.py +
bag_model.bag_sum AND to a second cache that runs the unfused calls on a copy of the store: pooled rows, perf counts, server
table and versions every step, line state through test_gpu_cache._compare_state.

Kernel instances and the case that reaches each (the dispatcher: 16-byte path when width % 4 == 0, 8 rows per round when the
mean bag holds at most 8 ids; the accumulate: 16-byte path the same way, fixed bags by division, ragged ones through bag_of):
  cache_lookup_rows_sum_kernel<4, 8>    test_shapes[w8-F4], [w4-F1], every trace of test_traces (B=16, F=4, width 8)
  cache_lookup_rows_sum_kernel<4, 32>   test_shapes[w128-F26], [w260-F70] (two column slices, the second partial; a bag longer
                                        than one block of 64 positions), [w512-F26-long-runs], [w8-ragged-long]
  cache_lookup_rows_sum_kernel<1, 8>    test_shapes[w6-F4], [w7-F1], [w7-ragged]
  cache_lookup_rows_sum_kernel<1, 32>   test_shapes[w7-F26]
  apply_mapped2_bags_kernel<4, fixed>   every fixed-bag case of a width that is a multiple of 4; its long-run path (a run of
                                        >= 48 occurrences of one key, the cooperative accumulate): [w512-F26-long-runs]
  apply_mapped2_bags_kernel<4, ragged>  test_shapes[w8-ragged], [w8-ragged-long], [w8-ragged-clamped]
  apply_mapped2_bags_kernel<1, fixed>   test_shapes[w6-F4], [w7-F1], [w7-F26]
  apply_mapped2_bags_kernel<1, ragged>  test_shapes[w7-ragged]; test_apply_mapped2_bags_alone reaches all four directly
  cache_slot_map_kernel + bag_sum_kernel (the pooled pull side of a push-pull)   test_push_pull
  the two-launch update (ha_cache_update_same_keys_bags, fused path)             test_traces[...same...], asserted through
                                                                                 ha_cache_fused_updates
Remote mode, the sharded store and the operator layer: test_gpu_cache_bag_calls_remote.py, test_gpu_hetu_ops_bag_calls.py."""
import ctypes

import numpy as np
import pytest
import torch

import bag_model
from herald_amd import _lib
from herald_amd import cache as hcache
from herald_amd import ops
from oracle import cache_model
from test_gpu_cache import _compare_state

pytestmark = pytest.mark.gpu

CLS = {"lru": hcache.LRUCache, "lfu": hcache.LFUCache, "lfuopt": hcache.LFUOptCache}
PERF = ("type", "num_all", "num_unique", "num_miss", "num_transfered", "is_full")


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Bags:
    """The bags of one batch: fixed [B, F] or ragged by offsets (numpy) -- and what the calls and the models take."""

    def __init__(self, dev, n, F=None, offsets=None):
        self.n, self.F = n, F
        self.offsets = None if offsets is None else np.asarray(offsets, dtype=np.int64)
        self.nbags = n // F if F else self.offsets.size - 1
        self.of = np.arange(n) // F if F else bag_model.bag_of(self.offsets, n)
        self.d_off = None if F else torch.from_numpy(self.offsets).to(dev)
        self.d_of = None if F else torch.from_numpy(self.of.astype(np.int32)).to(dev)

    def sum(self, rows):
        pos = np.arange(self.n)
        return bag_model.bag_sum(rows, pos.reshape(self.nbags, self.F) if self.F else pos, self.offsets)

    def pull_kw(self):
        return dict(bag=self.F) if self.F else dict(offsets=self.d_off)

    def push_kw(self):
        return dict(bag=self.F) if self.F else dict(bag_of=self.d_of)


def ragged_offsets(rng, n, nbags, empty=2, long=0, clamp=False):
    """offsets of nbags bags over n ids: `empty` empty bags, bag 0 of `long` ids (0: any); clamp: the ends lie out of range."""
    cuts = [int(x) for x in rng.integers(long, n + 1, size=nbags - 1 - empty - (1 if long else 0))]
    if long:
        cuts.append(long)                                   # bag 0 = [0, long): every other cut lies at or behind it
    cuts += [int(x) for x in rng.choice(cuts, size=empty)]  # a cut twice: an empty bag
    off = np.array([0] + sorted(cuts) + [n], dtype=np.int64)
    assert off.size == nbags + 1 and np.sum(np.diff(off) == 0) >= empty and np.diff(off).max() >= long
    if clamp:
        off[0], off[-1] = -5, n + 9
    return off


def _pair(dev, policy, limit, rows, width, nmax, pull_bound, push_bound, table0, bind=None):
    """(pooled cache, its store, unfused cache, its store): two caches of one kind over two copies of one table."""
    out = []
    for _ in range(2):
        table = torch.from_numpy(table0.copy()).to(dev)
        versions = torch.zeros(rows, dtype=torch.int64, device=dev)
        c = CLS[policy](limit, rows, width, node_id=0, max_batch=max(nmax, 64), device=dev)
        (bind or (lambda g, t, v: g.bind_store(t, v)))(c, table, versions)
        c.pull_bound, c.push_bound = pull_bound, push_bound
        c.perf_enabled = True
        out += [c, (table, versions)]
    return out


def _same_perf(got, exp, step, what):
    for f in PERF:
        assert got[f] == exp[f], (what, step, f, got, exp)
    if exp["type"] == "Push":
        assert got["num_evict"] == exp["num_evict"], (what, step, got, exp)


def _stores_equal(step, server, *stores):
    for table, versions in stores:
        np.testing.assert_array_equal(versions.cpu().numpy(), server.ver, err_msg="server versions step %d" % step)
        np.testing.assert_array_equal(bits(table), bits(server.table), err_msg="server table step %d" % step)


def run_trace(dev, policy="lru", limit=40, rows=400, width=8, B=16, F=4, steps=24, pull_bound=3, push_bound=3, seed=0, zipf=True,
              variant="plain", int_keys=False, bind=None, ragged=None):
    """ragged: dict for ragged_offsets (F is then the mean bag size: n = B * F ids in B bags).  variant: plain | same (the
    update names the lookup's key tensor) | pushkeys | ahead (prefetch_keys) | ahead_batch (prefetch_keys_batch, blocks of 4)
    | alternate (pooled and unpooled calls take turns on the SAME cache, plans reused across the two forms)."""
    n = B * F
    rng = np.random.default_rng(seed)
    table0 = rng.standard_normal((rows, width), dtype=np.float32)
    server = cache_model.Server(table0)
    model = cache_model.CacheModel(policy, limit, width, server, pull_bound, push_bound)
    gpu, st, ref, st_ref = _pair(dev, policy, limit, rows, width, n, pull_bound, push_bound, table0, bind)
    rk = np.random.default_rng(seed + 1000)

    def draw():
        if zipf:
            return (np.minimum(rk.zipf(1.3, size=n) - 1, rows - 1).astype(np.int64) * 7919) % rows
        return rk.integers(0, rows, size=n)

    keys_all = [draw() for _ in range(steps)]
    dkey = (lambda k: torch.from_numpy(k.astype(np.int64)).to(dev)) if int_keys else \
        (lambda k: torch.from_numpy(k.astype(np.float32)).to(dev))
    kts = [dkey(k) for k in keys_all]
    same = variant in ("same", "alternate")
    for step in range(steps):
        keys, kt = keys_all[step], kts[step]
        bags = Bags(dev, n, offsets=ragged_offsets(rng, n, B, **ragged)) if ragged is not None else Bags(dev, n, F)
        if variant == "ahead_batch" and step % 4 == 0:
            gpu.prefetch_keys_batch(kts[step:step + 4])
            ref.prefetch_keys_batch(kts[step:step + 4])
        want_rows = model.lookup(keys.astype(np.uint64))
        want = bags.sum(want_rows)
        out = torch.full((bags.nbags, width), 7.0, dtype=torch.float32, device=dev)
        dest = torch.empty((n, width), dtype=torch.float32, device=dev)
        pooled_lookup = variant != "alternate" or step % 2 == 0
        if pooled_lookup:
            gpu.embedding_lookup_sum(kt, out, **bags.pull_kw()).wait()
        else:
            gpu.embedding_lookup(kt, dest).wait()
            out = ops.embedding_lookup_sum(dest, torch.arange(n, device=dev).view(-1, F))
        ref.embedding_lookup(kt, dest).wait()
        np.testing.assert_array_equal(bits(dest), bits(want_rows), err_msg="unfused rows step %d" % step)
        np.testing.assert_array_equal(bits(out), bits(want), err_msg="pooled rows step %d" % step)
        _same_perf(gpu.perf[-1], model.perf[-1], step, "lookup")
        _same_perf(gpu.perf[-1], ref.perf[-1], step, "lookup vs unfused")
        if variant == "ahead" and step + 1 < steps:
            gpu.prefetch_keys(kts[step + 1])
            ref.prefetch_keys(kts[step + 1])
        bag_grads = rng.standard_normal((bags.nbags, width), dtype=np.float32) * np.float32(-0.01)
        grads = np.ascontiguousarray(bag_grads[bags.of])
        d_bg, d_g = torch.from_numpy(bag_grads).to(dev), torch.from_numpy(grads).to(dev)
        pooled_update = variant != "alternate" or step % 4 in (1, 2)      # all four pairings of the two forms
        if variant == "pushkeys":
            pk = np.unique(rng.choice(keys, size=max(1, n // 3)))
            d_pk = torch.from_numpy(pk.astype(np.int64)).to(dev)
            model.update_with_push_keys(keys.astype(np.uint64), pk.astype(np.uint64), grads)
            gpu.embedding_update_with_push_keys_bags(dkey(keys), d_pk, d_bg, **bags.push_kw()).wait()
            ref.embedding_update_with_push_keys(dkey(keys), d_pk, d_g).wait()
        else:
            model.update(keys.astype(np.uint64), grads)
            uk = kt if same else dkey(keys)
            if pooled_update:
                gpu.embedding_update_bags(uk, d_bg, same_as_lookup=same, **bags.push_kw()).wait()
            else:
                gpu.embedding_update(uk, d_g, same_as_lookup=same).wait()
            ref.embedding_update(uk, d_g, same_as_lookup=same).wait()
        _same_perf(gpu.perf[-1], model.perf[-1], step, "update")
        _same_perf(gpu.perf[-1], ref.perf[-1], step, "update vs unfused")
        _stores_equal(step, server, st, st_ref)
        _compare_state(gpu, model, step)
    assert gpu.size() == model.policy.size()
    np.testing.assert_array_equal(gpu.keys(), np.array(model.policy.keys(), dtype=np.uint64))
    fused = lambda c: int(c._L.ha_cache_fused_updates(c._h))
    assert fused(gpu) == fused(ref)
    return gpu, fused(gpu)


@pytest.mark.parametrize("pull_bound,push_bound", [(0, 0), (3, 3), (100, 100)])
@pytest.mark.parametrize("policy", ["lru", "lfu", "lfuopt"])
def test_traces(dev, policy, pull_bound, push_bound):
    run_trace(dev, policy, pull_bound=pull_bound, push_bound=push_bound, seed=11)


@pytest.mark.parametrize("policy,limit", [("lru", 64), ("lfu", 64), ("lfuopt", 64), ("lru", 5), ("lfu", 7)])
def test_heavy_eviction_and_limit_below_the_batch(dev, policy, limit):
    run_trace(dev, policy, limit=limit, rows=1000, zipf=False, pull_bound=2, push_bound=2, seed=3, steps=20)


@pytest.mark.parametrize("variant", ["same", "pushkeys", "ahead", "ahead_batch", "alternate"])
@pytest.mark.parametrize("policy", ["lru", "lfu"])
def test_call_variants(dev, policy, variant):
    steps = 24
    _, fused = run_trace(dev, policy, limit=100, rows=1500, steps=steps, pull_bound=2, push_bound=2, seed=21, variant=variant)
    if variant in ("same", "alternate"):       # limit >= batch, LRU, the lookup's plan reused: the two-launch update, every step
        assert fused == (steps if policy == "lru" else 0)


@pytest.mark.parametrize("variant", ["plain", "same", "ahead"])
def test_int64_keys(dev, variant):
    run_trace(dev, "lru", limit=100, rows=1500, steps=12, pull_bound=1, push_bound=1, seed=22, variant=variant, int_keys=True)


SHAPES = {
    "w4-F1": dict(width=4, B=48, F=1),
    "w8-F4": dict(width=8, B=16, F=4),
    "w6-F4": dict(width=6, B=16, F=4),
    "w7-F1": dict(width=7, B=40, F=1),
    "w7-F26": dict(width=7, B=6, F=26),
    "w128-F26": dict(width=128, B=16, F=26, limit=300, rows=5000, steps=6),
    "w260-F70": dict(width=260, B=5, F=70, limit=200, rows=3000, steps=6),
    "w512-F26-long-runs": dict(width=512, B=77, F=26, limit=2500, rows=6000, steps=3, variant="same"),
    "w8-ragged": dict(width=8, B=16, F=4, ragged=dict(empty=3)),
    "w7-ragged": dict(width=7, B=16, F=4, ragged=dict(empty=3)),
    "w8-ragged-long": dict(width=8, B=6, F=20, ragged=dict(empty=1, long=70)),
    "w8-ragged-clamped": dict(width=8, B=16, F=4, ragged=dict(empty=2, clamp=True)),
    # key placement: 12 rows only -- every key sits in many bags and most bags hold a key twice
    "w8-F4-few-keys": dict(width=8, B=16, F=4, rows=12, limit=8, zipf=False),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(dev, name):
    kw = dict(steps=10, pull_bound=1, push_bound=2, seed=31)
    kw.update(SHAPES[name])
    if name == "w512-F26-long-runs":
        # (the zipf draw repeats one key several hundred times per batch: the accumulate's cooperative long-run path)
        rk = np.random.default_rng(kw["seed"] + 1000)
        k = (np.minimum(rk.zipf(1.3, size=77 * 26) - 1, 5999).astype(np.int64) * 7919) % 6000
        assert np.bincount(k).max() >= 48
    if name == "w8-F4-few-keys":
        rk = np.random.default_rng(kw["seed"] + 1000).integers(0, 12, size=64).reshape(16, 4)
        assert any(len(set(r)) < 4 for r in rk)
    _, fused = run_trace(dev, "lru", **kw)
    if name == "w512-F26-long-runs":
        assert fused == 3


def test_a_resident_line_with_a_pending_gradient_that_is_pulled_again(dev):
    """Two caches alternate over ONE store, pull_bound 0, push_bound large: a line that holds un-pushed updates goes stale when the
    other cache pushes its key, and its next lookup pulls the row and re-adds the line's gradient inside the sum (Line::addup).
    The count of such pulls comes from the CPU model alone."""
    rows, width, B, F, limit, steps = 60, 8, 8, 4, 200, 16
    n = B * F
    rng = np.random.default_rng(5)
    table0 = rng.standard_normal((rows, width), dtype=np.float32)
    server = cache_model.Server(table0)
    table = torch.from_numpy(table0.copy()).to(dev)
    versions = torch.zeros(rows, dtype=torch.int64, device=dev)
    models, gpus = [], []
    for i in range(2):
        # cache 0 keeps its updates (they stay pending), cache 1 pushes every update (its pushes make cache 0's lines stale)
        pb = 1000 if i == 0 else 0
        models.append(cache_model.CacheModel("lru", limit, width, server, 0, pb))
        g = hcache.LRUCache(limit, rows, width, node_id=0, max_batch=64, device=dev)
        g.bind_store(table, versions)
        g.pull_bound, g.push_bound = 0, pb
        gpus.append(g)
    bags = Bags(dev, n, F)
    readded = 0
    for step in range(steps):
        i = step % 2
        keys = rng.integers(0, rows, size=n)
        res = models[i].resident()
        readded += sum(1 for k in np.unique(keys) if k in res and res[k].grad is not None and np.any(res[k].grad != 0) and
                       res[k].version != -1 and server.ver[k] - res[k].version > 0)
        want = bags.sum(models[i].lookup(keys.astype(np.uint64)))
        kt = torch.from_numpy(keys.astype(np.float32)).to(dev)
        out = torch.empty((B, width), dtype=torch.float32, device=dev)
        gpus[i].embedding_lookup_sum(kt, out, bag=F).wait()
        np.testing.assert_array_equal(bits(out), bits(want), err_msg="pooled rows step %d" % step)
        bag_grads = rng.standard_normal((B, width), dtype=np.float32) * np.float32(-0.01)
        models[i].update(keys.astype(np.uint64), np.ascontiguousarray(bag_grads[bags.of]))
        gpus[i].embedding_update_bags(kt, torch.from_numpy(bag_grads).to(dev), bag=F, same_as_lookup=True).wait()
        _stores_equal(step, server, (table, versions))
        _compare_state(gpus[i], models[i], step)
    assert readded > 0, "the trace never pulls a line with a pending gradient: choose another seed"


@pytest.mark.parametrize("sides", ["both", "pull", "push", "ragged", "ragged-pull"])
@pytest.mark.parametrize("policy", ["lru", "lfu", "lfuopt"])
def test_push_pull(dev, policy, sides, bind=None):
    """run_push_pull_trace's shape (rows 300, width 8, n 48, limit 30, 40 steps), pooled on both sides, on one side only, with
    fixed (F = 4) and ragged bags."""
    rng = np.random.default_rng(21)
    rows, width, n, limit, F = 300, 8, 48, 30, 4
    B = n // F
    table0 = rng.standard_normal((rows, width), dtype=np.float32)
    server = cache_model.Server(table0)
    model = cache_model.CacheModel(policy, limit, width, server, 2, 2)
    gpu, st, ref, st_ref = _pair(dev, policy, limit, rows, width, 64, 2, 2, table0, bind)
    batches = [((np.minimum(rng.zipf(1.3, size=n) - 1, rows - 1) * 31) % rows).astype(np.float32) for _ in range(40)]

    def bags_of_step():
        if sides.startswith("ragged"):
            return Bags(dev, n, offsets=ragged_offsets(rng, n, B, empty=2))
        return Bags(dev, n, F)

    pull_bags = bags_of_step()
    want = pull_bags.sum(model.lookup(batches[0].astype(np.uint64)))
    out = torch.empty((B, width), dtype=torch.float32, device=dev)
    dest = torch.empty((n, width), dtype=torch.float32, device=dev)
    gpu.embedding_lookup_sum(torch.from_numpy(batches[0]).to(dev), out, **pull_bags.pull_kw()).wait()
    ref.embedding_lookup(torch.from_numpy(batches[0]).to(dev), dest).wait()
    np.testing.assert_array_equal(bits(out), bits(want))
    for k in range(len(batches) - 1):
        push_bags, pull_bags = pull_bags, bags_of_step()
        bag_grads = rng.standard_normal((B, width), dtype=np.float32) * np.float32(0.01)
        grads = np.ascontiguousarray(bag_grads[push_bags.of])
        want_rows = model.push_pull(batches[k + 1].astype(np.uint64), batches[k].astype(np.uint64), grads)
        pullk, pushk = torch.from_numpy(batches[k + 1]).to(dev), torch.from_numpy(batches[k]).to(dev)
        d_bg, d_g = torch.from_numpy(bag_grads).to(dev), torch.from_numpy(grads).to(dev)
        if sides in ("both", "ragged"):
            kw = dict(bag=F) if sides == "both" else dict(pull_offsets=pull_bags.d_off, push_bag_of=push_bags.d_of)
            gpu.embedding_push_pull_bags(pullk, out, pushk, d_bg, **kw).wait()
            got = out
        elif sides in ("pull", "ragged-pull"):
            kw = dict(pull_bag=F) if sides == "pull" else dict(pull_offsets=pull_bags.d_off)
            gpu.embedding_push_pull_bags_side(pullk, out, pushk, d_g, **kw).wait()
            got = out
        else:
            rows_got = torch.empty((n, width), dtype=torch.float32, device=dev)
            gpu.embedding_push_pull_bags_side(pullk, rows_got, pushk, d_bg, push_bag=F).wait()
            np.testing.assert_array_equal(bits(rows_got), bits(want_rows), err_msg="push_pull rows at step %d" % k)
            got = None
        ref.embedding_push_pull(pullk, dest, pushk, d_g).wait()
        np.testing.assert_array_equal(bits(dest), bits(want_rows), err_msg="unfused push_pull rows at step %d" % k)
        if got is not None:
            np.testing.assert_array_equal(bits(got), bits(pull_bags.sum(want_rows)), err_msg="pooled push_pull at step %d" % k)
        _stores_equal(k, server, st, st_ref)
        _compare_state(gpu, model, k)


@pytest.mark.parametrize("width,misalign", [(8, 0), (7, 0), (8, 1), (260, 0)])
@pytest.mark.parametrize("ragged", [False, True])
def test_apply_mapped2_bags_alone(dev, width, misalign, ragged):
    """ha_apply_mapped2_bags against ha_apply_mapped2 on the expanded gradient, both destinations, bit for bit: rowmap2 with
    negative entries, dst_init mixed, the 16-byte path and the other one (an odd width, or a gradient that starts off 16 bytes)."""
    L = _lib.load()
    rng = np.random.default_rng(7 + width)
    B, F, rows, S = 40, 6, 50, 64
    n = B * F
    ids = rng.integers(0, rows, size=n)
    ids[:90] = 3                                            # a run of 90 occurrences: the cooperative path
    d_ids = torch.from_numpy(ids.astype(np.float32)).to(dev)
    plan = ops.IndexPlan(n, device=dev).build(d_ids)
    U = plan.n_unique()
    rowmap = rng.permutation(S)[:U].astype(np.int32)
    rowmap2 = rowmap.copy()
    rowmap2[rng.random(U) < 0.3] = -1
    init = (rng.random(S) < 0.5).astype(np.uint8)
    bags = Bags(dev, n, offsets=ragged_offsets(rng, n, B, empty=3)) if ragged else Bags(dev, n, F)
    bag_grads = rng.standard_normal((B, width), dtype=np.float32)
    buf = torch.zeros(B * width + 4, dtype=torch.float32, device=dev)
    d_bg = buf[misalign:misalign + B * width].view(B, width)
    d_bg.copy_(torch.from_numpy(bag_grads))
    d_g = torch.from_numpy(np.ascontiguousarray(bag_grads[bags.of])).to(dev)
    d_rm, d_rm2, d_init = (torch.from_numpy(x).to(dev) for x in (rowmap, rowmap2, init))
    a0 = rng.standard_normal((S, width), dtype=np.float32)
    b0 = rng.standard_normal((S, width), dtype=np.float32)
    res = []
    vp = ctypes.c_void_p
    for pooled in (False, True):
        a, b = torch.from_numpy(a0.copy()).to(dev), torch.from_numpy(b0.copy()).to(dev)
        head = (vp(a.data_ptr()), S, vp(b.data_ptr()), width, vp(plan.ws.data_ptr()), n)
        if pooled:
            _lib.check(L.ha_apply_mapped2_bags(*head, vp(d_bg.data_ptr()), ctypes.c_float(-1.0), vp(d_rm.data_ptr()),
                                               vp(d_rm2.data_ptr()), 0 if ragged else F,
                                               vp(bags.d_of.data_ptr()) if ragged else None, vp(d_init.data_ptr()), None),
                       "ha_apply_mapped2_bags")
        else:
            _lib.check(L.ha_apply_mapped2(*head, vp(d_g.data_ptr()), ctypes.c_float(-1.0), vp(d_rm.data_ptr()),
                                          vp(d_rm2.data_ptr()), vp(d_init.data_ptr()), None), "ha_apply_mapped2")
        torch.cuda.synchronize()
        res.append((bits(a), bits(b)))
    np.testing.assert_array_equal(res[0][0], res[1][0], err_msg="first destination")
    np.testing.assert_array_equal(res[0][1], res[1][1], err_msg="second destination")
    assert not np.array_equal(res[1][0], bits(a0)) and not np.array_equal(res[1][1], bits(b0))

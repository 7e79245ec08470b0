"""Stream ordering of the ahead-of-time planners with LATE ids (tests/late_ids.py): every entry point that reads id tensors on
a side stream is handed ids that are still a decoy when the call returns -- a gate holds the caller's stream in front of the
copy that writes the real ones, and is opened 10 ms after the call --, and its results are compared, assert_array_equal, with
the CPU models every other test of the engines uses (oracle/cache_model.py; the oracle's serial lookup / sparse SGD / sparse
push).  An entry point that reads its ids before the caller's stream has produced them computes the decoy's rows, hits and
slots and fails the comparison; it cannot fault (the decoy is a batch of valid ids).  DESIGN.md ("Who orders the ids")
lists the entry points, what each is ordered behind, and the test here that holds it.

Late writes begin with the second block (first-call allocations, stream calibration and the LFU take-over's synchronisation
stay out of the way) and reach block index >= 4 (the steady-state paths).  Every late batch's "the gate is still closed"
condition is asserted (LateIds.release), and every test asserts at its end that it released as many late batches as it meant
to write."""
import numpy as np
import pytest
import torch

from herald_amd import cache as hcache
from herald_amd import hetu_ops, ops, synth
from herald_amd.sharded import FramedStep, ShardedEmbedding
from late_ids import LateIds, decoy_of
from oracle import cache_model, cpu
from test_gpu_cache import _compare_state
from test_gpu_cache_planned import _draw, _planned_step, _setup
from test_gpu_cache_planned_push_keys import _pk_step, _push_set
from test_gpu_cache_planned_push_pull import _chain_step
import bag_model

pytestmark = pytest.mark.gpu

LIMIT, ROWS, WIDTH, N = 100, 1500, 8, 64          # the shapes of the small-trace tests: only the ordering is under test
TORCH_OF = {np.float32: torch.float32, np.int64: torch.int64}


_CALLER = {}


@pytest.fixture(autouse=True)
def caller_stream(dev):
    """The caller's stream of every test here: a stream of its own, not the null stream.  The library's first-call
    allocations zero their memory through the null stream and wait for it; behind a gate on the null stream itself those
    waits would run to the gate's bound, and a non-blocking stream is what a training loop hands the engines anyway.  (One
    stream for the module: the planning streams are chosen, once, per caller's stream.)"""
    if "s" not in _CALLER:
        _CALLER["s"] = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(_CALLER["s"]):
        yield _CALLER["s"]
    torch.cuda.synchronize()


def _on_device(arrs, dev, shape=None):
    """The real ids of the batches that are written early, staged up front: nothing is uploaded while a gate is closed."""
    return [torch.from_numpy(np.ascontiguousarray(a.astype(np.float32).reshape(shape or a.shape))).to(dev) for a in arrs]


@pytest.fixture
def late(dev):
    lt = LateIds(dev, ROWS)
    yield lt
    lt.drain()
    torch.cuda.synchronize()


def _stage(buf, arr):
    """An ordinary (early) write of a ring buffer: staged, copied, synchronised."""
    buf.copy_(torch.from_numpy(np.ascontiguousarray(arr.astype({torch.float32: np.float32, torch.int64: np.int64}[buf.dtype])
                                                    .reshape(tuple(buf.shape)))).to(buf.device))
    torch.cuda.synchronize()


# ---- control: the harness sees the hazard -----------------------------------------------------------------------------------
def test_control_an_unordered_side_stream_copy_reads_the_decoy(dev, late):
    """A copy on a side stream that nothing orders behind the caller's stream returns the decoy; the same copy behind
    side.wait_stream(caller's stream) returns the real ids."""
    rng = np.random.default_rng(1)
    real = rng.integers(0, ROWS, size=N).astype(np.float32)
    buf = torch.empty(N, dtype=torch.float32, device=dev)
    got = [torch.zeros(N, dtype=torch.float32, device=dev) for _ in range(2)]
    side = torch.cuda.Stream(device=dev, priority=min(torch.cuda.Stream.priority_range()))
    torch.cuda.synchronize()
    late.write([(buf, real)])
    with torch.cuda.stream(side):
        got[0].copy_(buf)
    late.release()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got[0].cpu().numpy(), decoy_of(real, ROWS))
    np.testing.assert_array_equal(buf.cpu().numpy(), real)
    late.write([(buf, real)])
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        got[1].copy_(buf)
    late.release()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got[1].cpu().numpy(), real)
    assert late.released == late.batches == 2


# ---- the cache's planned flow ----------------------------------------------------------------------------------------------
def _blocks_of(entries, block):
    return [entries[b0:b0 + block] for b0 in range(0, len(entries), block)]


@pytest.mark.parametrize("block", [1, 4])
@pytest.mark.parametrize("dtype", [np.float32, np.int64], ids=["f32keys", "i64keys"])
@pytest.mark.parametrize("policy", ["lru", "lfuopt"])
def test_cache_planned_pairs_with_late_ids(dev, late, policy, dtype, block):
    """CacheSparseTable.plan_block(after_current=True), 8 blocks planned one block ahead, every block from the second on
    written late: rows, perf counters, server table and versions every step, the whole line state at the end."""
    nblk = 8
    steps = nblk * block
    rng, server, model, table, versions, gpu = _setup(dev, LIMIT, ROWS, WIDTH, N, 2, 2, 91 + block, policy)
    tbl = hcache.CacheSparseTable.wrap(gpu)
    keys_all = [_draw(rng, N, ROWS, True) for _ in range(steps)]
    ring = [torch.empty(N, dtype=TORCH_OF[dtype], device=dev) for _ in range(3 * block)]
    blocks = _blocks_of(list(range(steps)), block)

    def plan(j):
        bufs = [ring[s % len(ring)] for s in blocks[j]]
        if j == 0:
            for b, s in zip(bufs, blocks[j]):
                _stage(b, keys_all[s])
            tbl.plan_block(bufs, after_current=True)
            return
        late.write([(b, keys_all[s]) for b, s in zip(bufs, blocks[j])])
        tbl.plan_block(bufs, after_current=True)
        late.release()

    plan(0)
    for j, blk in enumerate(blocks):
        if j + 1 < nblk:
            plan(j + 1)
        for step in blk:
            grads = rng.standard_normal((N, WIDTH), dtype=np.float32) * np.float32(-0.01)
            _planned_step(dev, gpu, model, keys_all[step], grads, WIDTH, step, versions, server)
            np.testing.assert_array_equal(table.cpu().numpy(), server.table, err_msg="server table step %d" % step)
    assert gpu.plan_pending() == 0
    _compare_state(gpu, model, steps)
    np.testing.assert_array_equal(gpu.keys(), np.array(model.policy.keys(), dtype=np.uint64))
    assert late.released == late.batches == (nblk - 1) * block


@pytest.mark.parametrize("policy", ["lru", "lfuopt"])
def test_cache_planned_push_key_blocks_with_late_ids_and_late_push_keys(dev, late, policy):
    """ha_cache_plan_block_push_keys promises the ordering itself: ids AND push keys written late, no switch."""
    nblk, block = 8, 4
    steps = nblk * block
    rng, server, model, table, versions, gpu = _setup(dev, LIMIT, ROWS, WIDTH, N, 2, 2, 95, policy)
    keys_all = [_draw(rng, N, ROWS, True) for _ in range(steps)]
    pks = [_push_set(rng, keys_all[s], "third", ROWS) for s in range(steps)]
    assert all(p.size for p in pks)
    ring = [torch.empty(N, dtype=torch.float32, device=dev) for _ in range(3 * block)]
    pbuf = [torch.empty(p.size, dtype=torch.int64, device=dev) for p in pks]       # (sizes differ: one buffer per batch)
    blocks = _blocks_of(list(range(steps)), block)

    def plan(j):
        bufs = [ring[s % len(ring)] for s in blocks[j]]
        if j == 0:
            for b, s in zip(bufs, blocks[j]):
                _stage(b, keys_all[s])
                _stage(pbuf[s], pks[s])
        else:
            late.write([(b, keys_all[s]) for b, s in zip(bufs, blocks[j])] + [(pbuf[s], pks[s], True) for s in blocks[j]])
        gpu.plan_block(bufs, push_keys_list=[pbuf[s] for s in blocks[j]])
        if j:
            late.release()

    plan(0)
    for j, blk in enumerate(blocks):
        if j + 1 < nblk:
            plan(j + 1)
        for step in blk:
            grads = rng.standard_normal((N, WIDTH), dtype=np.float32) * np.float32(-0.01)
            _pk_step(dev, gpu, model, keys_all[step], pks[step], grads, WIDTH, step, versions, server)
            np.testing.assert_array_equal(table.cpu().numpy(), server.table, err_msg="server table step %d" % step)
    assert gpu.plan_pending() == 0
    _compare_state(gpu, model, steps)
    assert late.released == late.batches == 2 * (nblk - 1) * block


def test_cache_planned_push_pull_chain_with_late_ids(dev, late):
    """The push-pull chain (head, middle steps, closing entry) promises the ordering itself: late ids, no switch."""
    nblk, block, limit = 8, 4, 128
    steps = nblk * block - 1                   # + the closing entry: 8 whole blocks
    rng, server, model, table, versions, gpu = _setup(dev, limit, ROWS, WIDTH, N, 2, 2, 97)
    keys_all = [_draw(rng, N, ROWS, True) for _ in range(steps)]
    grads_all = [rng.standard_normal((N, WIDTH), dtype=np.float32) * np.float32(-0.01) for _ in range(steps)]
    ring = [torch.empty(N, dtype=torch.float32, device=dev) for _ in range(4 * block)]   # (a batch is used by two steps)
    blocks = _blocks_of(list(range(steps)) + [None], block)

    def plan(j):
        real = [e for e in blocks[j] if e is not None]
        if j == 0:
            for e in real:
                _stage(ring[e % len(ring)], keys_all[e])
        else:
            late.write([(ring[e % len(ring)], keys_all[e]) for e in real])
        gpu.plan_block([ring[e % len(ring)] if e is not None else None for e in blocks[j]], push_pull=True)
        if j:
            late.release()

    plan(0)
    for j, blk in enumerate(blocks):
        if j + 1 < nblk:
            plan(j + 1)
        for e in blk:
            _chain_step(dev, gpu, model, e, steps, keys_all, grads_all, WIDTH, versions, server)
            step = steps if e is None else e
            np.testing.assert_array_equal(versions.cpu().numpy(), server.ver, err_msg="server versions step %d" % step)
            np.testing.assert_array_equal(table.cpu().numpy(), server.table, err_msg="server table step %d" % step)
    assert gpu.plan_pending() == 0
    _compare_state(gpu, model, steps)
    assert late.released == late.batches == steps - block


# ---- the communicate op with cache_plan_ahead: a loader that produces its ids on the current stream ---------------------------
@pytest.mark.parametrize("schedule,policy", [("bsp_pairs", "lru"), ("bsp_pairs", "lfuopt"), ("asp_chain", "lru")])
def test_communicate_op_plans_ahead_from_a_loader_whose_ids_are_late(dev, schedule, policy):
    """ParameterServerCommunicateOp with Config.cache_plan_ahead, 9 steps: next_ids / peek_ids return ring buffers that are
    written late at the moment they are first handed out.  bsp_pairs is the regression for the steady-state branch of
    ha_cache_plan_block (from the fourth block on it waits only for an event three blocks old): the op plans with
    after_current=True."""
    rows, width, bs, lr, bound, nb = 3000, 16, 8, 0.1, 1, 10
    limit = 300 if schedule == "bsp_pairs" else 2 * bs * 26 + 40
    late = LateIds(dev, rows)
    rng = np.random.default_rng(2)
    table0 = rng.standard_normal((rows, width), dtype=np.float32)
    store = ShardedEmbedding(rows, width, dev, table=torch.from_numpy(table0.copy()).to(dev))
    emb = hetu_ops.EmbeddingParameter(store=store)
    batches = [(synth.criteo_batch(bs, b, seed=9).reshape(bs, 26) % rows).astype(np.float32) for b in range(nb)]
    ring = [torch.empty((bs, 26), dtype=torch.float32, device=dev) for _ in range(nb)]
    _stage(ring[0], batches[0])
    state = {"k": 0, "handed": {0}}

    def hand(i):
        if i not in state["handed"]:           # the loader's upload of batch i, on the current stream, when it is first asked for
            state["handed"].add(i)
            late.write([(ring[i], batches[i])])
        return ring[i]

    def next_ids():
        return hand(state["k"] + 1)

    def peek_ids(j):
        i = state["k"] + 1 + j
        return hand(i) if i < nb else None

    cfg = hetu_ops.Config(comm_mode="Hybrid", bsp=0 if schedule == "bsp_pairs" else -1, prefetch=True,
                          cstable_policy=policy.upper(), cache_bound=bound, cache_limit=limit, cache_plan_ahead=True)
    comm = hetu_ops.ParameterServerCommunicateOp(emb, lr, next_ids, peek_ids=peek_ids)
    try:
        comm.forward_hook(cfg, first_ids=ring[0])
        late.release()                             # batch 1: the second block
        assert comm._planned is not None and comm._chain == (schedule == "asp_chain")
        look = hetu_ops.EmbeddingLookUp(emb)
        look.forward_hook(cfg)
        gradop = hetu_ops.EmbeddingLookUp_Gradient(emb.shape)
        server = cache_model.Server(table0)
        model = cache_model.CacheModel(policy, limit, width, server, bound, bound)
        pending = model.lookup(batches[0].reshape(-1).astype(np.uint64))
        for k in range(nb - 1):
            state["k"] = k
            ids, d_ids = batches[k], ring[k]
            out = torch.empty((bs, 26, width), dtype=torch.float32, device=dev)
            look.compute(d_ids, out)
            np.testing.assert_array_equal(out.cpu().numpy().reshape(-1, width), pending, err_msg="lookup step %d" % k)
            gout = (out * 0.25 - 0.5).contiguous()
            g_np = cpu.scale_values(gout.cpu().numpy().reshape(-1, width), lr)
            comm.compute(gradop.compute(gout, d_ids))
            if k + 2 < nb:
                late.release()                     # batch k + 2 was handed out, planned, and is still a decoy
            nxt = batches[k + 1].reshape(-1).astype(np.uint64)
            if schedule == "asp_chain":
                pending = model.push_pull(nxt, ids.reshape(-1).astype(np.uint64), g_np)
            else:
                model.update(ids.reshape(-1).astype(np.uint64), g_np)
                pending = model.lookup(nxt)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(store.table.cpu().numpy(), server.table, err_msg="server table step %d" % k)
        assert late.released == late.batches == nb - 1
    finally:
        late.drain()
        torch.cuda.synchronize()
        hcache._TABLES.pop(emb.id, None)       # (register_table is for the life of a model: not beyond this test)


# ---- the call-by-call cache's prefetch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [0, 4], ids=["prefetch_keys", "prefetch_keys_batch4"])
def test_cache_prefetch_keys_with_late_keys(dev, late, batch):
    """prefetch_keys (the sort on the cache's own stream, forked from the caller's) and prefetch_keys_batch (one launch on
    the caller's stream): late keys, then their lookups and updates against the model."""
    steps = 24
    rng, server, model, table, versions, gpu = _setup(dev, LIMIT, ROWS, WIDTH, N, 2, 2, 93)
    keys_all = [_draw(rng, N, ROWS, True) for _ in range(steps)]
    ring = [torch.empty(N, dtype=torch.float32, device=dev) for _ in range(8)]
    _stage(ring[0], keys_all[0])
    want_late = 0
    for step in range(steps):
        if batch and step % batch == 0:
            blk = list(range(step, step + batch))
            if step == 0:
                for s in blk:
                    _stage(ring[s % 8], keys_all[s])
            else:
                late.write([(ring[s % 8], keys_all[s]) for s in blk])
                want_late += batch
            gpu.prefetch_keys_batch([ring[s % 8] for s in blk])
            if step:
                late.release()
        kt = ring[step % 8]
        dest = torch.empty((N, WIDTH), dtype=torch.float32, device=dev)
        want = model.lookup(keys_all[step].astype(np.uint64))
        gpu.embedding_lookup(kt, dest).wait()
        np.testing.assert_array_equal(dest.cpu().numpy(), want, err_msg="lookup rows at step %d" % step)
        if not batch and step + 1 < steps:
            late.write([(ring[(step + 1) % 8], keys_all[step + 1])])
            want_late += 1
            gpu.prefetch_keys(ring[(step + 1) % 8])
            late.release()
        grads = rng.standard_normal((N, WIDTH), dtype=np.float32) * np.float32(-0.01)
        model.update(keys_all[step].astype(np.uint64), grads)
        gpu.embedding_update(kt, torch.from_numpy(grads).to(dev)).wait()
        np.testing.assert_array_equal(versions.cpu().numpy(), server.ver, err_msg="server versions step %d" % step)
        np.testing.assert_array_equal(table.cpu().numpy(), server.table, err_msg="server table step %d" % step)
    _compare_state(gpu, model, steps)
    assert late.released == late.batches == want_late


# ---- the step engines of ops.py: nothing is read back until the stream of batches has been enqueued ------------------------------
def _uniform_stream(rng, rows, n, nb):
    ids = [rng.integers(0, rows, size=n) for _ in range(nb)]
    for b in ids:       # below 16 occurrences of a key the work-queue step IS the reference's serial chain, bit for bit
        assert np.unique(b, return_counts=True)[1].max() < 16
    return ids


def _check_steps(table0, table, ids, grads, outs, lr):
    """Rows of every batch and the table at the end against the oracle's serial lookup / sparse SGD."""
    torch.cuda.synchronize()
    want = table0.copy()
    for k, b in enumerate(ids):
        f = b.astype(np.float32)
        np.testing.assert_array_equal(outs[k].cpu().numpy().reshape(b.size, -1), cpu.embedding_lookup(want, f),
                                      err_msg="lookup rows of batch %d" % k)
        cpu.sgd_sparse_update(want, f, grads[k], lr)
    np.testing.assert_array_equal(table.cpu().numpy(), want, err_msg="table after the stream")


def _ahead(late, k, block, first, LA, nb, bufs, ids, d_real, written):
    """The ahead ids (batch k + LA) that step k of a block-wise engine hands over.  From step `first` on ONE gate per block,
    put in front of the block's second step, holds every ahead batch of the block's steps 2 .. B and of the next block's first
    step: ALL ahead ids are late from there on (the copies that write them are enqueued behind the gate at once; the steps
    hand the buffers over while it is closed).  The caller opens the gate when the next block's first step has returned: that
    step enqueues the side-stream work that reads the block's batches.  Batches before `first` are written early."""
    if block > 1 and k >= first and k % block == 1 and not late.pending():
        items = [(bufs[j + LA], ids[j + LA]) for j in range(k, k + block) if j + LA < nb]
        if items:
            late.write(items)
            written.update(j + LA for j in range(k, k + block) if j + LA < nb)
    a = k + LA
    if a >= nb:
        return None
    if a not in written:
        bufs[a].copy_(d_real[a])
    return bufs[a]


@pytest.mark.parametrize("rows,n,block,nblk", [(ROWS, N, 2, 8), (ROWS, N, 8, 8), (50000, 7169, 2, 8)],
                         ids=["block2", "block8", "wide_7169_ids"])
def test_queue_step_pipeline_events_with_late_ahead_ids(dev, rows, n, block, nblk):
    """QueueStepPipeline(sync="events"): from the second block on every ahead batch handed to step() is written late (_ahead:
    one gate per block); the plans of a block's batches are enqueued by the next block's first step, after which the gate is
    opened.  (sync="flags" forbids such ids.)"""
    late = LateIds(dev, rows)
    rng = np.random.default_rng(n + block)
    lr, nb = 0.05, nblk * block
    table0 = rng.standard_normal((rows, WIDTH), dtype=np.float32)
    table = torch.from_numpy(table0.copy()).to(dev)
    ids = _uniform_stream(rng, rows, n, nb)
    grads = [rng.standard_normal((n, WIDTH), dtype=np.float32) for _ in range(nb)]
    d_grads = [torch.from_numpy(g).to(dev) for g in grads]
    bufs = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(nb)]
    d_real = _on_device(ids, dev)
    pipe = ops.QueueStepPipeline(table, n, lr, block=block, sync="events")
    assert pipe.wide == (n > ops.qstep_max_ids())
    LA = pipe.LOOKAHEAD
    for k in range(min(LA, nb)):
        _stage(bufs[k], ids[k])
    try:
        outs = [pipe.start(bufs[:LA])]
        written = set()
        for k in range(nb):
            outs.append(pipe.step(d_grads[k], _ahead(late, k, block, block, LA, nb, bufs, ids, d_real, written)))
            if late.pending() and k % block == 0:
                late.release()                 # this step started a block: the late batches' plans are enqueued
        assert not late.pending() and late.released == late.batches == len(written)
        assert written == set(range(LA + block + 1, nb))          # every ahead batch from the second block's second step on
        assert outs[nb] is None and pipe.fallbacks == 0
        _check_steps(table0, table, ids, grads, outs, lr)
    finally:
        late.drain()
        torch.cuda.synchronize()


@pytest.mark.parametrize("engine", ["step_pipeline", "sort_ahead", "sort_ahead_pipeline"])
def test_step_engines_with_late_next_ids(dev, late, engine):
    """StepPipeline.step (the ahead ids are sorted inside the step's launch), SortAhead.lookup(next_ids=) and
    SortAheadPipeline.prepare_block (a side stream that follows the caller's stream): late ids from the second batch / block on."""
    rng = np.random.default_rng(77)
    lr, nb = 0.05, 12
    table0 = rng.standard_normal((ROWS, WIDTH), dtype=np.float32)
    table = torch.from_numpy(table0.copy()).to(dev)
    ids = _uniform_stream(rng, ROWS, N, nb)
    grads = [rng.standard_normal((N, WIDTH), dtype=np.float32) for _ in range(nb)]
    d_grads = [torch.from_numpy(g).to(dev) for g in grads]
    bufs = [torch.empty(N, dtype=torch.float32, device=dev) for _ in range(nb)]
    outs = []
    if engine == "step_pipeline":
        for k in range(3):
            _stage(bufs[k], ids[k])
        pipe = ops.StepPipeline(table, N, lr)
        outs.append(pipe.start(bufs[0], bufs[1], bufs[2]))
        for k in range(nb):
            a = k + 3
            if a < nb:
                late.write([(bufs[a], ids[a])])
            outs.append(pipe.step(d_grads[k], bufs[a] if a < nb else None))
            if a < nb:
                late.release()
        want_late = nb - 3
    elif engine == "sort_ahead":
        _stage(bufs[0], ids[0])
        sa = ops.SortAhead(table, N, lr)
        sa.begin(bufs[0])
        for k in range(nb):
            if k + 1 < nb:
                late.write([(bufs[k + 1], ids[k + 1])])
            outs.append(sa.lookup(bufs[k], next_ids=bufs[k + 1] if k + 1 < nb else None))
            if k + 1 < nb:
                late.release()
            sa.apply(d_grads[k])
        want_late = nb - 1
    else:
        block = 2
        for k in range(block):
            _stage(bufs[k], ids[k])
        pipe = ops.SortAheadPipeline(table, N, lr, block=block)
        pipe.prepare_block(bufs[:block])
        for k in range(nb):
            if k % block == 0 and k + block < nb:
                nxt = list(range(k + block, k + 2 * block))
                late.write([(bufs[j], ids[j]) for j in nxt])
                pipe.prepare_block([bufs[j] for j in nxt])
                late.release()
            outs.append(pipe.lookup(k, bufs[k]))
            pipe.apply(k, d_grads[k])
        want_late = nb - block
    assert late.released == late.batches == want_late
    _check_steps(table0, table, ids, grads, outs, lr)


# ---- the sharded store ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side_stream", [True, False], ids=["side_stream", "callers_stream"])
def test_sharded_prefetch_after_current_with_late_ids(dev, late, side_stream):
    """ShardedEmbedding(side_stream=True).prefetch(after_current=True) routes on the engine's side stream behind the caller's
    stream; in the default mode (side_stream=False) the routing runs on the caller's stream itself and program order does the
    ordering.  Late ids, then pull(route=) and push(route=) against the oracle's serial PS semantics."""
    rng = np.random.default_rng(5)
    lr, nb = 0.05, 8
    table0 = rng.standard_normal((ROWS, WIDTH), dtype=np.float32)
    emb = ShardedEmbedding(ROWS, WIDTH, dev, table=torch.from_numpy(table0.copy()).to(dev), side_stream=side_stream)
    assert emb.side_stream == side_stream
    ids = _uniform_stream(rng, ROWS, N, nb)
    bufs = [torch.empty(N, dtype=torch.float32, device=dev) for _ in range(3)]
    want = table0.copy()
    first_late = emb.engine.NSLOT      # (a routing workspace is allocated, and waited for, at its first use)
    for k in range(nb):
        buf = bufs[k % 3]
        if k < first_late:
            _stage(buf, ids[k])
            r = emb.prefetch(buf, after_current=True)
        else:
            late.write([(buf, ids[k])])
            r = emb.prefetch(buf, after_current=True)
            late.release()
            assert (r.ready is not None) == side_stream     # (the routing ran on the side stream: pull / push wait for it)
        f = ids[k].astype(np.float32)
        got = emb.pull(route=r)
        np.testing.assert_array_equal(got.cpu().numpy().reshape(N, WIDTH), want[ids[k]], err_msg="pull of batch %d" % k)
        g = rng.standard_normal((N, WIDTH), dtype=np.float32)
        emb.push(None, torch.from_numpy(g).to(dev), lr, route=r)
        cpu.sparse_push(want, f, g, lr)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(emb.table.cpu().numpy(), want, err_msg="table after batch %d" % k)
    assert late.released == late.batches == nb - first_late == 5


def _framed_case(dev, nb, bag=None, seed=15):
    rng = np.random.default_rng(seed)
    table0 = rng.standard_normal((ROWS, WIDTH), dtype=np.float32)
    emb = ShardedEmbedding(ROWS, WIDTH, dev, table=torch.from_numpy(table0.copy()).to(dev))
    ids = _uniform_stream(rng, ROWS, N, nb)
    nrow = N if bag is None else N // bag
    grads = [rng.standard_normal((nrow, WIDTH), dtype=np.float32) for _ in range(nb)]
    d_grads = [torch.from_numpy(g).to(dev) for g in grads]
    shape = (N,) if bag is None else (N // bag, bag)
    bufs = [torch.empty(shape, dtype=torch.float32, device=dev) for _ in range(nb)]
    return table0, emb, ids, grads, d_grads, bufs, _on_device(ids, dev, shape)


def _check_framed(table0, emb, ids, grads, res, lr, bag=None):
    torch.cuda.synchronize()
    want = table0.copy()
    for k, b in enumerate(ids):
        f = b.astype(np.float32)
        if bag is None:
            ref, g = want[b], grads[k]
        else:
            ref, g = bag_model.bag_sum(want, f.reshape(-1, bag)), grads[k][np.arange(b.size) // bag]
        np.testing.assert_array_equal(res[k].cpu().numpy().reshape(ref.shape), ref, err_msg="rows of batch %d" % k)
        cpu.sparse_push(want, f, g, lr)
    np.testing.assert_array_equal(emb.table.cpu().numpy(), want, err_msg="table after the stream")


@pytest.mark.parametrize("form", ["sized_eager", "fixed_frames_graphs"])
def test_framed_step_pull_push_with_late_ahead_ids(dev, late, form):
    """FramedStep at world size 1, pull / push step by step: every ahead batch the pulls stage is written late (_ahead: one
    gate per block); the next block's first pull routes the block (behind the caller's stream), after which the gate is opened.  The graph
    form's late writes begin once every graph of the ring has been captured: a (slot, buffers) key runs eagerly at its
    first use and is captured, which synchronises, at its second."""
    block, nblk, lr = 2, 12, 0.05
    nb = nblk * block
    graphs = form == "fixed_frames_graphs"
    table0, emb, ids, grads, d_grads, bufs, d_real = _framed_case(dev, nb)
    fs = FramedStep(emb, N, graphs=graphs, block=block)
    assert fs.sized == (not graphs)
    LA = fs.LOOKAHEAD
    for k in range(LA):
        _stage(bufs[k], ids[k])
    outs = [torch.empty((N, WIDTH), device=dev) for _ in range(3 * block)]      # (the graphs' buffers: one per ring slot)
    first_late = 2 * len(outs) if graphs else block
    fs.start(bufs[:LA])
    res, written = [], set()
    for k in range(nb):
        got = fs.pull(_ahead(late, k, block, first_late, LA, nb, bufs, ids, d_real, written), out=outs[k % len(outs)])
        if late.pending() and k % block == 0:
            late.release()
        res.append(got.clone())
        fs.push(d_grads[k % len(outs)], lr)        # (a ring of gradient buffers too: a graph is keyed by its buffers)
    assert fs.fallbacks == 0 and not late.pending()
    assert late.released == late.batches == len(written)
    assert written == set(range(LA + first_late + 1, nb)) and len(written) >= 7
    _check_framed(table0, emb, ids, [grads[k % len(outs)] for k in range(nb)], res, lr)


@pytest.mark.parametrize("bag", [None, 8], ids=["steps", "steps_bags"])
def test_framed_step_native_steps_with_late_ahead_ids(dev, late, bag):
    """FramedStep.steps / steps_bags, one native call per block: all ahead ids of every other call are written late; the next
    call enqueues the routing of their block behind the end of the block that staged them."""
    block, nblk, lr = 2, 8, 0.05
    nb = nblk * block
    table0, emb, ids, grads, d_grads, bufs, d_real = _framed_case(dev, nb, bag)
    fs = FramedStep(emb, N, graphs=False, block=block)
    assert fs.sized and fs.native_ok()
    LA = fs.LOOKAHEAD
    for k in range(LA):
        _stage(bufs[k], ids[k])
    fs.start(bufs[:LA])
    res, want_late = [], 0
    call = fs.steps if bag is None else fs.steps_bags
    for b in range(nblk):
        k0 = b * block
        ahead, items = [], []
        for i in range(block):
            a = k0 + i + LA
            if a >= nb:
                ahead.append(None)
            elif b % 2 == 1:                       # (every other block: one gate at a time, held over two calls)
                items.append((bufs[a], ids[a]))
                ahead.append(bufs[a])
            else:
                bufs[a].copy_(d_real[a])
                ahead.append(bufs[a])
        if items:
            late.write(items)                      # ALL ahead ids of this call, behind one gate
            want_late += len(items)
        res.extend(call(ahead, d_grads[k0:k0 + block], lr))
        if late.pending() and b % 2 == 0:
            late.release()                         # this call enqueued the routing that reads the late batch
    assert fs.fallbacks == 0 and not late.pending()
    assert late.released == late.batches == want_late == 6
    _check_framed(table0, emb, ids, grads, res, lr, bag)


def test_framed_steps_after_a_block_of_pull_push_routes_behind_its_late_ids(dev, late):
    """Regression: two native blocks, one block through pull() / push() whose last ahead ids are written late, native blocks
    again.  The native block after the step-by-step one must route its successor behind everything queued on the step
    stream (the block-end event of the last NATIVE block is stale: the late batch was staged after it); the gate is still
    closed when that steps() call returns."""
    block, nblk, lr = 2, 7, 0.05
    nb = nblk * block
    table0, emb, ids, grads, d_grads, bufs, d_real = _framed_case(dev, nb, seed=16)
    fs = FramedStep(emb, N, graphs=False, block=block)
    assert fs.sized and fs.native_ok()
    LA = fs.LOOKAHEAD
    for k in range(LA):
        _stage(bufs[k], ids[k])
    fs.start(bufs[:LA])
    res = []

    def ahead_of(k, is_late=False):
        a = k + LA
        if a >= nb:
            return None
        if is_late:
            late.write([(bufs[a], ids[a])])
        else:
            bufs[a].copy_(d_real[a])
        return bufs[a]

    for b in range(nblk):
        k0 = b * block
        if b == 2:                                 # step by step; the block's LAST ahead ids (a batch of block 4) are late
            for k in (k0, k0 + 1):
                res.append(fs.pull(ahead_of(k, is_late=(k == k0 + 1))))
                fs.push(d_grads[k], lr)
            assert late.pending()
            continue
        res.extend(fs.steps([ahead_of(k0 + i) for i in range(block)], d_grads[k0:k0 + block], lr))
        if b == 3:
            late.release()                         # block 3's call has enqueued the routing of block 4
    assert fs.fallbacks == 0 and late.released == late.batches == 1
    _check_framed(table0, emb, ids, grads, res, lr)

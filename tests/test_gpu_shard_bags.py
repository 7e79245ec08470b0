"""Sum-pooled pull and push over the row-sharded table on the GPU: ha_gather_sum_u32keys against the numpy restatement
(tests/bag_model.py) and against the float-id kernel, ha_dedup_reduce_bags against ha_dedup_reduce(_scaled) on the expanded
gradient (whole output buffers) and against a float32 chain written out here, and ShardedEmbedding.pull_sum / push_bags /
push_pull_bags at world size 1 against pull / push on a twin store and the oracle's serial PS semantics (oracle/cpu.py).
Every comparison is on float32 bit patterns."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bag_model  # noqa: E402

from herald_amd import _lib, ops  # noqa: E402
from herald_amd.sharded import ShardedEmbedding  # noqa: E402
from oracle import cpu  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = -123.456


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---- ha_gather_sum_u32keys ------------------------------------------------------------------------------------------------------
BUF_ROWS = 300
_bufs = {}


def _rows_buf(width):
    """One 300-row buffer per width, shared and never written: magnitudes over many binades so that the order of a sum shows."""
    if width not in _bufs:
        rng = np.random.default_rng(1000 + width)
        _bufs[width] = (rng.standard_normal((BUF_ROWS, width)) * np.exp(rng.uniform(-8, 8, (BUF_ROWS, 1)))).astype(np.float32)
    return _bufs[width]


def _keys(n, seed):
    rng = np.random.default_rng(seed)
    k = rng.integers(0, BUF_ROWS, n).astype(np.int32)
    k[: n // 3] = k[0]                                  # repeats
    if n > 4:
        k[n - 2] = BUF_ROWS + 7                         # a key beyond the buffer: a zero row
    return rng.permutation(k)


def _check_gather_sum(dev, buf, keys, offsets=None, d_buf=None):
    """gather_sum_u32keys on (buf, keys) equals the restatement and the float-id kernel; inputs stay as they were."""
    d_buf = torch.from_numpy(buf).to(dev) if d_buf is None else d_buf
    d_keys = torch.from_numpy(keys).to(dev)
    d_off = torch.from_numpy(np.asarray(offsets, dtype=np.int64)).to(dev) if offsets is not None else None
    nbags = keys.shape[0] if offsets is None else len(offsets) - 1
    out = torch.full((nbags, buf.shape[1]), CANARY, dtype=torch.float32, device=dev)
    got = ops.gather_sum_u32keys(d_buf, d_keys, offsets=d_off, out=out)
    assert got is out and got.shape == (nbags, buf.shape[1])
    want = bag_model.bag_sum(buf, keys.astype(np.int64), offsets)
    assert np.array_equal(_bits(got), _bits(want))
    twin = ops.embedding_lookup_sum(d_buf, d_keys.to(torch.float32), offsets=d_off)
    assert np.array_equal(_bits(got), _bits(twin))
    if nbags:
        assert not np.array_equal(_bits(got), _bits(np.full(want.shape, CANARY, np.float32)))
    assert np.array_equal(_bits(d_buf), _bits(buf)) and np.array_equal(d_keys.cpu().numpy(), keys)
    return got


@pytest.mark.parametrize("F", [1, 8, 9, 26, 64, 65, 130])       # 8 / 9: the ROWS switch; 64 / 65 / 130: the 64-id block
def test_gather_sum_u32keys_fixed_bags(dev, F):
    for width in (4, 37, 64, 192, 516):
        for B in (3, 41):
            _check_gather_sum(dev, _rows_buf(width), _keys(B * F, 10 * F + B).reshape(B, F))


def test_gather_sum_u32keys_every_slice_width(dev):
    buf, keys = _rows_buf(516), _keys(33 * 26, 5).reshape(33, 26)
    L = _lib.load()
    try:
        for floats in (64, 128, 256):                   # 516 floats: a partial last slice in each
            assert L.ha_debug_bag_slice(floats) == 0
            _check_gather_sum(dev, buf, keys)
    finally:
        L.ha_debug_bag_slice(0)


def test_gather_sum_u32keys_ragged_bags_and_the_clamp(dev):
    n = 300
    keys = _keys(n, 77)
    # empty bags at the front, in the middle and at the end, one bag of 200 ids, one of 1
    offsets = [0, 0, 0, 200, 200, 201, 230, 230, 300, 300, 300]
    for width in (4, 37, 64, 516):
        _check_gather_sum(dev, _rows_buf(width), keys, offsets)
    # offsets beyond n (and a decreasing one): clamped to [0, n], a bag's end to its start
    for width in (37, 64):
        _check_gather_sum(dev, _rows_buf(width), keys, [0, 50, 40, 290, 350, 1000])


def test_gather_sum_u32keys_misaligned_buffer_takes_the_scalar_path(dev):
    width = 64
    buf = _rows_buf(width)
    base = torch.zeros(BUF_ROWS * width + 4, dtype=torch.float32, device=dev)
    d_buf = base[1:1 + BUF_ROWS * width].view(BUF_ROWS, width)      # 4 bytes into its allocation
    d_buf.copy_(torch.from_numpy(buf))
    assert d_buf.data_ptr() % 16 == 4
    keys = _keys(20 * 26, 3).reshape(20, 26)
    got = _check_gather_sum(dev, buf, keys, d_buf=d_buf)
    aligned = ops.gather_sum_u32keys(torch.from_numpy(buf).to(dev), torch.from_numpy(keys).to(dev))
    assert np.array_equal(_bits(got), _bits(aligned))


def test_gather_sum_u32keys_no_bags_and_no_keys(dev):
    buf = _rows_buf(64)
    d_buf = torch.from_numpy(buf).to(dev)
    out = ops.gather_sum_u32keys(d_buf, torch.zeros((0, 26), dtype=torch.int32, device=dev))
    assert out.shape == (0, 64)
    off = torch.zeros(5, dtype=torch.int64, device=dev)             # n = 0, four empty bags
    out = torch.full((4, 64), CANARY, dtype=torch.float32, device=dev)
    ops.gather_sum_u32keys(d_buf, torch.zeros(0, dtype=torch.int32, device=dev), offsets=off, out=out)
    assert np.array_equal(_bits(out), np.zeros((4, 64), np.int32))


# ---- ha_dedup_reduce_bags -------------------------------------------------------------------------------------------------------
def _chain_reduce(keys, which, g, scale):
    """reduced[u,:] = (0 + scale * g[which[i0],:]) + scale * g[which[i1],:] + ... over the occurrences i0 < i1 < ... of the
    u-th smallest key, float32 throughout (one rounding per product, one per sum): the worker-side reduce of a PS sparse push
    (PSAgent::vecPushSparse) on the gradient of a sum-pooled lookup.  Vectorised over the keys, sequential over a key's
    occurrences."""
    uniq, inv = np.unique(keys, return_inverse=True)
    order = np.argsort(inv, kind="stable")                          # occurrences grouped by key, in occurrence order
    cnt = np.bincount(inv)
    seg = np.concatenate([[0], np.cumsum(cnt)])
    by_len = np.argsort(-cnt, kind="stable")
    neg = -cnt[by_len]
    s = np.float32(1.0 if scale is None else scale)
    red = np.zeros((uniq.size, g.shape[1]), dtype=np.float32)
    for r in range(int(cnt.max())):
        live = by_len[:np.searchsorted(neg, -r, side="left")]       # the keys with more than r occurrences
        term = (s * g[which[order[seg[live] + r]]]).astype(np.float32)
        red[live] = (red[live] + term).astype(np.float32)
    return red


def _ids_with_runs(n, runs, rows, seed):
    """n float32 ids < rows: one key per entry of `runs` repeated that often, the rest drawn at random; shuffled."""
    rng = np.random.default_rng(seed)
    assert sum(runs) <= n
    parts = [np.full(c, 7 + 11 * j, dtype=np.int64) for j, c in enumerate(runs)]
    parts.append(rng.integers(1000, rows, n - sum(runs)))
    return rng.permutation(np.concatenate(parts)).astype(np.float32)


def _ragged_offsets(n, nbags, seed, whole=None):
    """int64 offsets[nbags + 1] over n ids with empty bags at the front, in the middle and at the end; whole = (lo, hi): one
    bag is exactly ids[lo:hi]."""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.integers(0, n + 1, nbags - 4))
    if whole is not None:
        cuts = np.sort(np.concatenate([cuts[(cuts <= whole[0]) | (cuts >= whole[1])], [whole[0], whole[1]]]))
    off = np.concatenate([[0, 0], cuts[: cuts.size // 2], [cuts[cuts.size // 2]], cuts[cuts.size // 2:], [n, n]])
    off = np.concatenate([[0], off[1:]]).astype(np.int64)
    assert off[0] == 0 and off[-1] == n and np.all(np.diff(off) >= 0) and (whole is not None or off.size == nbags + 1)
    return off


def _check_reduce_bags(dev, ids, g, width, bag=None, offsets=None, scale=None, chain=True, plan_ids=None):
    """dedup_reduce_bags equals dedup_reduce on the expanded gradient over the WHOLE output buffer (both pre-filled with the
    same canary) and the float32 chain; the result differs from the canary and the inputs stay as they were."""
    n = ids.size
    d_ids = torch.from_numpy(ids if plan_ids is None else plan_ids).to(dev)
    plan = ops.IndexPlan(n, dev).build(d_ids.reshape(-1))
    if offsets is None:
        which = np.arange(n) // bag
        d_bag_of = None
    else:
        d_off = torch.from_numpy(offsets).to(dev)
        d_bag_of = ops.bag_of(d_off, n)
        which = bag_model.bag_of(offsets, n) if n <= 4096 else d_bag_of.cpu().numpy()
        assert np.array_equal(d_bag_of.cpu().numpy(), which)
    d_g = torch.from_numpy(g).to(dev)
    expanded = torch.from_numpy(g[which]).to(dev)
    want = torch.full((n, width), CANARY, dtype=torch.float32, device=dev)
    ops.dedup_reduce(plan, expanded, out=want, scale=scale)
    got = torch.full((n, width), CANARY, dtype=torch.float32, device=dev)
    assert ops.dedup_reduce_bags(plan, d_g, bag=bag, bag_of=d_bag_of, scale=scale, out=got) is got
    torch.cuda.synchronize()
    assert np.array_equal(_bits(got), _bits(want))
    u = plan.n_unique()
    assert not np.array_equal(_bits(got[:u]), _bits(np.full((u, width), CANARY, np.float32)))
    if chain:
        keys = cpu.ids_to_keys(ids)
        red = _chain_reduce(keys, which, g, scale)
        assert red.shape[0] == u
        assert np.array_equal(_bits(got[:u]), _bits(red))
    assert np.array_equal(_bits(d_g), _bits(g))
    if plan_ids is None:
        assert np.array_equal(_bits(d_ids), _bits(ids))
    return got


POS_RUNS = (1, 3, 15, 16, 63, 64, 300, 1100)


def _pos_ids(F, seed=1):
    n = -(-(sum(POS_RUNS) + 60) // F) * F
    return _ids_with_runs(n, POS_RUNS, 30000, seed)


@pytest.mark.parametrize("F", [2, 26, 27])
def test_dedup_reduce_bags_by_position(dev, F):
    ids = _pos_ids(F)
    for width in (64, 66, 516):
        g = np.random.default_rng(width + F).standard_normal((ids.size // F, width)).astype(np.float32)
        for scale in (None, -0.05):
            _check_reduce_bags(dev, ids, g, width, bag=F, scale=scale)


def test_dedup_reduce_bags_ragged_by_position(dev):
    ids = np.sort(_pos_ids(26))                 # sorted: the 300-run is contiguous, one bag is that whole run
    lo = int(np.flatnonzero(ids == 7 + 11 * 6)[0])
    assert np.all(ids[lo:lo + 300] == ids[lo])
    offsets = _ragged_offsets(ids.size, 40, 3, whole=(lo, lo + 300))
    assert np.any((offsets[:-1] == lo) & (offsets[1:] == lo + 300))
    for width in (64, 66):
        g = np.random.default_rng(width).standard_normal((offsets.size - 1, width)).astype(np.float32)
        for scale in (None, -0.05):
            _check_reduce_bags(dev, ids, g, width, offsets=offsets, scale=scale)
    shuffled = _pos_ids(26, seed=5)
    offsets = _ragged_offsets(shuffled.size, 40, 4)
    g = np.random.default_rng(9).standard_normal((offsets.size - 1, 64)).astype(np.float32)
    _check_reduce_bags(dev, shuffled, g, 64, offsets=offsets, scale=-0.05)


LISTED_N = 40014            # = 26 x 1,539: beyond the by-position range, the finish lists the long keys
LISTED_RUNS = (5000, 2500, 300, 48, 5)


@pytest.fixture(scope="module")
def listed_ids():
    return _ids_with_runs(LISTED_N, LISTED_RUNS, 200000, 21)


@pytest.mark.parametrize("width", [64, 66])
def test_dedup_reduce_bags_by_unique_key_listed(dev, listed_ids, width):
    g = np.random.default_rng(width).standard_normal((LISTED_N // 26, width)).astype(np.float32)
    _check_reduce_bags(dev, listed_ids, g, width, bag=26, scale=-0.05)
    _check_reduce_bags(dev, listed_ids, g, width, bag=26, scale=None, chain=False)


def test_dedup_reduce_bags_by_unique_key_listed_ragged(dev, listed_ids):
    offsets = _ragged_offsets(LISTED_N, 1500, 8)
    g = np.random.default_rng(2).standard_normal((offsets.size - 1, 64)).astype(np.float32)
    _check_reduce_bags(dev, listed_ids, g, 64, offsets=offsets, scale=-0.05)


def test_dedup_reduce_bags_by_unique_key_unlisted(dev):
    n = 1048606             # = 26 x 40,331: beyond 2^20 ids, apply_unique_kernel + apply_long_kernel
    ids = _ids_with_runs(n, (5000, 300, 48), 3000000, 31)
    g = np.random.default_rng(4).standard_normal((n // 26, 4)).astype(np.float32)
    _check_reduce_bags(dev, ids, g, 4, bag=26, scale=-0.05)


def test_dedup_reduce_bags_int64_ids_equal_their_float32_twins(dev, listed_ids):
    for ids in (_pos_ids(26), listed_ids):
        g = np.random.default_rng(6).standard_normal((ids.size // 26, 64)).astype(np.float32)
        a = _check_reduce_bags(dev, ids, g, 64, bag=26, scale=-0.05, chain=False)
        b = _check_reduce_bags(dev, ids, g, 64, bag=26, scale=-0.05, chain=False, plan_ids=ids.astype(np.int64))
        assert np.array_equal(_bits(a), _bits(b))


def test_dedup_reduce_bags_misaligned_bag_grads(dev):
    ids = _pos_ids(26)
    B, width = ids.size // 26, 64
    g = np.random.default_rng(12).standard_normal((B, width)).astype(np.float32)
    aligned = _check_reduce_bags(dev, ids, g, width, bag=26, scale=-0.05)
    base = torch.zeros(B * width + 4, dtype=torch.float32, device=dev)
    d_g = base[1:1 + B * width].view(B, width)                      # 4 bytes into its allocation: the scalar path
    d_g.copy_(torch.from_numpy(g))
    assert d_g.data_ptr() % 16 == 4
    plan = ops.IndexPlan(ids.size, dev).build(torch.from_numpy(ids).to(dev))
    got = torch.full((ids.size, width), CANARY, dtype=torch.float32, device=dev)
    ops.dedup_reduce_bags(plan, d_g, bag=26, scale=-0.05, out=got)
    assert np.array_equal(_bits(got), _bits(aligned))
    assert np.array_equal(_bits(d_g), _bits(g))


@pytest.mark.parametrize("mode", [1, 2])
def test_dedup_reduce_bags_in_tolerance_mode_equals_the_expanded_call(dev, listed_ids, mode):
    """Mode 1: the same runs take the same tree, by position and by unique key.  Mode 2 (listed ids): the expanded call cuts
    its long runs into chunks; the bag call expands into scratch and runs that launch -- the same bits.  At width 66 (the scalar
    path) the expanded call does not chunk in mode 2 and neither call leaves the by-unique kernels."""
    prev = ops.set_tolerance_mode(mode)
    try:
        cases = [listed_ids] if mode == 2 else [_pos_ids(26), listed_ids]
        for ids in cases:
            g = np.random.default_rng(mode).standard_normal((ids.size // 26, 64)).astype(np.float32)
            _check_reduce_bags(dev, ids, g, 64, bag=26, scale=-0.05, chain=False)
        if mode == 2:
            g = np.random.default_rng(66).standard_normal((LISTED_N // 26, 66)).astype(np.float32)
            _check_reduce_bags(dev, listed_ids, g, 66, bag=26, scale=-0.05, chain=False)
            offsets = _ragged_offsets(LISTED_N, 1500, 8)
            g = np.random.default_rng(3).standard_normal((offsets.size - 1, 64)).astype(np.float32)
            _check_reduce_bags(dev, listed_ids, g, 64, offsets=offsets, scale=-0.05, chain=False)
    finally:
        ops.set_tolerance_mode(prev)


def test_reduce_bags_argument_errors_come_before_any_device_access(dev):
    plan = ops.IndexPlan(52, dev).build(torch.arange(52, dtype=torch.float32, device=dev))
    g = torch.zeros((2, 8), dtype=torch.float32, device=dev)
    with pytest.raises(ValueError):
        ops.dedup_reduce_bags(plan, g)                              # neither bag nor bag_of
    with pytest.raises(ValueError):
        ops.dedup_reduce_bags(plan, g, bag=26, bag_of=torch.zeros(52, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        ops.dedup_reduce_bags(plan, g, bag=13)                      # 4 bags of 13 need 4 gradient rows
    L = _lib.load()
    assert L.ha_dedup_reduce_bags(None, 52, None, 8, 0, None, 1.0, None, None) != 0      # neither, with null pointers
    assert b"exactly one" in L.ha_last_error()
    assert L.ha_dedup_reduce_bags(None, 52, None, 8, 5, None, 1.0, None, None) != 0
    assert b"multiple" in L.ha_last_error()


# ---- ShardedEmbedding at world size 1 ----------------------------------------------------------------------------------------
ROWS, B, F = 5000, 50, 26


def _store_case(kind):
    """(width, ids as numpy in the shape the store takes, offsets or None)."""
    rng = np.random.default_rng(40)
    ids = rng.integers(0, ROWS, (B, F))
    ids[:, 0] = 17                              # a key in every bag
    ids[3, :] = 99                              # a bag of one key
    width = 33 if kind == "d33" else 64
    if kind == "ragged":
        return width, ids.reshape(-1).astype(np.float32), _ragged_offsets(B * F, B, 41)
    return width, ids.astype(np.int64 if kind == "int64" else np.float32), None


def _expanded(g, ids, offsets):
    n = ids.size
    return g[np.arange(n) // F] if offsets is None else g[bag_model.bag_of(offsets, n)]


@pytest.mark.parametrize("kind", ["fixed", "ragged", "int64", "d33"])
def test_sharded_pull_sum_and_push_bags_at_world_size_1(dev, kind):
    width, ids, offsets = _store_case(kind)
    rng = np.random.default_rng(42)
    table0 = rng.standard_normal((ROWS, width)).astype(np.float32)
    g = rng.standard_normal((B, width)).astype(np.float32)
    g2 = rng.standard_normal((B, width)).astype(np.float32)
    lr = 0.05
    f_ids = ids.astype(np.float32)
    d_ids = torch.from_numpy(ids).to(dev)
    d_off = torch.from_numpy(offsets).to(dev) if offsets is not None else None
    d_g, d_g2 = torch.from_numpy(g).to(dev), torch.from_numpy(g2).to(dev)
    emb = ShardedEmbedding(ROWS, width, dev, table=torch.from_numpy(table0).to(dev))
    twin = ShardedEmbedding(ROWS, width, dev, table=torch.from_numpy(table0).to(dev))

    # pull_sum: the restatement on the global table, and the float-id kernel over the rows the twin's pull returns
    got = emb.pull_sum(d_ids, offsets=d_off)
    assert got.shape == (B, width)
    want = bag_model.bag_sum(table0, f_ids, offsets)
    assert np.array_equal(_bits(got), _bits(want))
    assert not np.array_equal(_bits(got), np.zeros((B, width), np.int32))
    rows = twin.pull(d_ids).reshape(-1, width)
    pos = torch.arange(B * F, dtype=torch.int64, device=dev).view(d_ids.shape)
    assert np.array_equal(_bits(got), _bits(ops.embedding_lookup_sum(rows, pos, offsets=d_off)))

    # push_bags: the table push(ids, expanded values) leaves on the twin, and the oracle's
    emb.push_bags(d_ids, d_g, lr, offsets=d_off)
    exp = _expanded(g, ids, offsets)
    twin.push(d_ids, torch.from_numpy(exp).to(dev), lr)
    table1 = table0.copy()
    cpu.sparse_push(table1, f_ids.reshape(-1), exp, lr)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(emb.table), _bits(twin.table))
    assert np.array_equal(_bits(emb.table), _bits(table1))
    assert not np.array_equal(_bits(emb.table), _bits(table0))

    # one prefetched route serves pull (fixed bags: [B, F, d]), pull_sum ([B, d]) and push_bags
    route = emb.prefetch(d_ids)
    if offsets is None:
        per_occ = emb.pull(route=route)
        assert per_occ.shape == (B, F, width)
        assert np.array_equal(_bits(per_occ), _bits(cpu.sparse_pull(table1, f_ids.reshape(-1)).reshape(B, F, width)))
    out = torch.full((B, width), CANARY, dtype=torch.float32, device=dev)
    got, r = emb.pull_sum(offsets=d_off, route=route, return_route=True, out=out)
    assert got is out and r is route
    assert np.array_equal(_bits(got), _bits(bag_model.bag_sum(table1, f_ids, offsets)))
    emb.push_bags(None, d_g2, lr, offsets=d_off, route=route)
    exp2 = _expanded(g2, ids, offsets)
    troute = twin.prefetch(d_ids)
    twin.pull(route=troute)
    twin.push(None, torch.from_numpy(exp2).to(dev), lr, route=troute)
    table2 = table1.copy()
    cpu.sparse_push(table2, f_ids.reshape(-1), exp2, lr)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(emb.table), _bits(table2))
    assert np.array_equal(_bits(emb.table), _bits(twin.table))

    # push_pull_bags: the pull sees the push
    got = emb.push_pull_bags(d_ids, d_g, lr, d_ids, push_offsets=d_off, pull_offsets=d_off)
    twin.push_pull(d_ids, torch.from_numpy(exp).to(dev), lr, d_ids)
    table3 = table2.copy()
    cpu.sparse_push(table3, f_ids.reshape(-1), exp, lr)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(got), _bits(bag_model.bag_sum(table3, f_ids, offsets)))
    assert np.array_equal(_bits(emb.table), _bits(table3)) and np.array_equal(_bits(emb.table), _bits(twin.table))
    assert emb.stats == twin.stats
    # inputs as they were
    assert np.array_equal(d_ids.cpu().numpy(), ids) and np.array_equal(_bits(d_g), _bits(g))
    assert np.array_equal(_bits(d_g2), _bits(g2))


def test_sharded_bag_calls_refuse_bad_shapes(dev):
    width = 16
    emb = ShardedEmbedding(ROWS, width, dev)
    flat = torch.zeros(B * F, dtype=torch.float32, device=dev)
    ids = flat.view(B, F)
    good = torch.zeros((B, width), dtype=torch.float32, device=dev)
    with pytest.raises(ValueError, match="offsets"):
        emb.pull_sum(flat)                                          # 1-D ids without offsets
    with pytest.raises(ValueError, match="offsets"):
        emb.push_bags(flat, good, 0.1)
    with pytest.raises(ValueError, match="bag_values"):
        emb.push_bags(ids, torch.zeros((B * F, width), dtype=torch.float32, device=dev), 0.1)
    with pytest.raises(ValueError, match="bag_values"):
        emb.push_bags(ids, torch.zeros((B, width + 1), dtype=torch.float32, device=dev), 0.1)
    off = torch.arange(0, B * F + 1, F)
    with pytest.raises(ValueError, match="int64"):
        emb.pull_sum(flat, offsets=off.to(dev).to(torch.int32))     # wrong dtype
    with pytest.raises(ValueError, match="int64"):
        emb.pull_sum(flat, offsets=off)                             # wrong device
    with pytest.raises(ValueError, match="int64"):
        emb.push_bags(flat, good, 0.1, offsets=off)
    with pytest.raises(ValueError, match="offsets"):
        emb.push_pull_bags(ids, good, 0.1, flat)                    # the pull's shape is checked before the push runs
    assert emb._live == {} and not torch.any(emb.table)             # nothing was routed, nothing written

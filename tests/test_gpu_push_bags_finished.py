"""The pooled end launches of the sharded step's push half against their expanded twins, whole destinations, float32 bit
patterns: ha_push_apply_scaled_bags_finished against ha_push_apply_scaled_finished on the expanded gradient (and, with the
tolerance mode off, against the oracle's serial PS push, oracle/cpu.py sparse_push), ha_apply_mapped_bags against
ha_apply_mapped on the expanded gradient -- by sorted position, by unique key with the long keys listed (36,865 .. 2^20 ids)
and beyond 2^20 ids."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bag_model  # noqa: E402
from test_gpu_shard_bags import _bits, _ids_with_runs, _ragged_offsets  # noqa: E402

from herald_amd import _lib, ops  # noqa: E402
from oracle import cpu  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = -123.456
F = 26
POS_RUNS = (1, 3, 16, 47, 48, 64, 300)          # short / medium / cooperative runs around kLongRun = 48
POS_N = F * 50
LISTED_N = 40014                                # = 26 x 1,539: by unique key, the finish lists the long keys
LISTED_RUNS = (4000, 300, 64, 48, 5)
_tables = {}


def _table(rows, width):
    """One table per shape, shared and never written: magnitudes over many binades so that the order of a sum shows."""
    if (rows, width) not in _tables:
        rng = np.random.default_rng(rows + width)
        _tables[(rows, width)] = (rng.standard_normal((rows, width), dtype=np.float32) *
                                  np.exp(rng.uniform(-6, 6, (rows, 1))).astype(np.float32))
    return _tables[(rows, width)]


def _pos_ids(seed=1):
    return _ids_with_runs(POS_N, POS_RUNS, 3000, seed)


@pytest.fixture(scope="module")
def listed_ids():
    return _ids_with_runs(LISTED_N, LISTED_RUNS, 60000, 21)


def _check(dev, ids, rows, width, seed, bag=None, offsets=None, scale=-0.05, chain=True, plan_ids=None, misaligned=False):
    """Both pooled calls equal their expanded twins over the whole destination; inputs stay as they were."""
    n = ids.size
    L = _lib.load()
    vp = ctypes.c_void_p
    d_ids = torch.from_numpy(ids if plan_ids is None else plan_ids).to(dev)
    plan = ops.IndexPlan(n, dev).build(d_ids.reshape(-1))
    if offsets is None:
        which, d_bag_of, nbags = np.arange(n) // bag, None, n // bag
    else:
        d_bag_of = ops.bag_of(torch.from_numpy(offsets).to(dev), n)
        which, nbags = d_bag_of.cpu().numpy(), offsets.size - 1
        if n <= 4096:
            assert np.array_equal(which, bag_model.bag_of(offsets, n))
    g = np.random.default_rng(seed).standard_normal((nbags, width), dtype=np.float32)
    if misaligned:
        base = torch.zeros(nbags * width + 4, dtype=torch.float32, device=dev)
        d_g = base[1:1 + nbags * width].view(nbags, width)            # 4 bytes into its allocation: the scalar path
        d_g.copy_(torch.from_numpy(g))
        assert d_g.data_ptr() % 16 == 4
    else:
        d_g = torch.from_numpy(g).to(dev)
    expanded = torch.from_numpy(g[which]).to(dev)
    table = _table(rows, width)
    # the world-1 push: reduce of scale * values by unique key + server add, one launch
    want = torch.from_numpy(table).to(dev)
    assert L.ha_push_apply_scaled_finished(vp(want.data_ptr()), rows, width, vp(plan.ws.data_ptr()), n, vp(expanded.data_ptr()),
                                           ctypes.c_float(scale), None) == 0
    got = torch.from_numpy(table).to(dev)
    assert ops.push_apply_scaled_bags_finished(got, plan, d_g, scale, bag=bag, bag_of=d_bag_of) is got
    torch.cuda.synchronize()
    assert np.array_equal(_bits(got), _bits(want))
    assert not np.array_equal(_bits(got), _bits(table))
    if chain:          # (tolerance mode off: every run is the serial chain)
        ref = table.copy()
        cpu.sparse_push(ref, ids, g[which], -scale)
        assert np.array_equal(_bits(got), _bits(ref))
    # the pooled mapped reduce: destination rows through a map (some keys without a destination), fresh and initialised rows
    u = plan.n_unique()
    rng = np.random.default_rng(seed + 1)
    rowmap = rng.permutation(u + 3)[:u].astype(np.int32)
    rowmap[rng.random(u) < 0.1] = -1
    init = (rng.random(u + 3) < 0.5).astype(np.uint8)
    d_rowmap, d_init = torch.from_numpy(rowmap).to(dev), torch.from_numpy(init).to(dev)
    dst0 = rng.standard_normal((u + 3, width), dtype=np.float32)
    want_m, got_m = torch.from_numpy(dst0).to(dev), torch.from_numpy(dst0).to(dev)
    assert L.ha_apply_mapped(vp(want_m.data_ptr()), u + 3, width, vp(plan.ws.data_ptr()), n, vp(expanded.data_ptr()),
                             ctypes.c_float(-scale), vp(d_rowmap.data_ptr()), None, vp(d_init.data_ptr()), None) == 0
    assert ops.apply_mapped_bags(got_m, plan, d_g, -scale, rowmap=d_rowmap, bag=bag, bag_of=d_bag_of, dst_init=d_init) is got_m
    torch.cuda.synchronize()
    assert np.array_equal(_bits(got_m), _bits(want_m))
    assert not np.array_equal(_bits(got_m), _bits(dst0))
    assert np.array_equal(_bits(d_g), _bits(g))
    if plan_ids is None:
        assert np.array_equal(_bits(d_ids), _bits(ids))
    return got, got_m


def test_push_bags_by_position(dev):
    ids = _pos_ids()
    for width in (64, 66, 516):
        for scale in (1.0, -0.05):
            _check(dev, ids, 3000, width, width, bag=F, scale=scale)


def test_push_bags_ragged_by_position(dev):
    ids = np.sort(_pos_ids())                   # sorted: the 300-run is contiguous, one bag is that whole run
    lo = int(np.flatnonzero(ids == 7 + 11 * 6)[0])
    assert np.all(ids[lo:lo + 300] == ids[lo])
    offsets = _ragged_offsets(ids.size, 40, 3, whole=(lo, lo + 300))
    for width in (64, 66):
        _check(dev, ids, 3000, width, width, offsets=offsets)
    _check(dev, _pos_ids(seed=5), 3000, 64, 9, offsets=_ragged_offsets(POS_N, 40, 4))


def test_push_bags_int64_ids_and_misaligned_bag_grads(dev):
    ids = _pos_ids()
    a = _check(dev, ids, 3000, 64, 6, bag=F)
    b = _check(dev, ids, 3000, 64, 6, bag=F, plan_ids=ids.astype(np.int64))
    c = _check(dev, ids, 3000, 64, 6, bag=F, misaligned=True)
    for x, y, z in zip(a, b, c):
        assert np.array_equal(_bits(x), _bits(y)) and np.array_equal(_bits(x), _bits(z))


@pytest.mark.parametrize("width", [64, 66])
def test_push_bags_by_unique_key_listed(dev, listed_ids, width):
    _check(dev, listed_ids, 60000, width, width, bag=F)
    _check(dev, listed_ids, 60000, width, width + 1, offsets=_ragged_offsets(LISTED_N, 1500, 8), chain=False)


def test_push_bags_by_unique_key_unlisted(dev):
    n = 1048606             # = 26 x 40,331: beyond 2^20 ids, apply_unique_kernel + apply_long_kernel
    ids = _ids_with_runs(n, (5000, 300, 48), 3000000, 31)
    _check(dev, ids, 3000000, 4, 4, bag=F)


@pytest.mark.parametrize("mode", [1, 2])
def test_push_bags_in_tolerance_mode_equals_the_expanded_call(dev, listed_ids, mode):
    """Mode 1: the same runs take the same tree, by position and by unique key.  Mode 2 (listed ids, 16-byte path, at most four
    slices): the expanded call cuts its long runs into chunks; the pooled push expands into scratch and runs that launch."""
    prev = ops.set_tolerance_mode(mode)
    try:
        _check(dev, _pos_ids(), 3000, 64, mode, bag=F, chain=False)
        _check(dev, listed_ids, 60000, 64, mode, bag=F, chain=False)
        _check(dev, listed_ids, 60000, 66, mode, bag=F, chain=False)
        _check(dev, listed_ids, 60000, 64, mode + 2, offsets=_ragged_offsets(LISTED_N, 1500, 8), chain=False)
    finally:
        ops.set_tolerance_mode(prev)


def test_push_bags_argument_errors_come_before_any_device_access(dev):
    L = _lib.load()
    vp = ctypes.c_void_p
    bad = vp(0x10)           # never dereferenced: every call below must fail in its checks
    f = ctypes.c_float(1.0)
    assert L.ha_push_apply_scaled_bags_finished(bad, 5, 8, bad, 52, bad, 0, None, f, None) != 0        # neither bag nor bag_of
    assert L.ha_push_apply_scaled_bags_finished(bad, 5, 8, bad, 52, bad, 26, bad, f, None) != 0        # both
    assert L.ha_push_apply_scaled_bags_finished(bad, 5, 8, bad, 52, bad, 25, None, f, None) != 0       # 52 is no multiple of 25
    assert L.ha_push_apply_scaled_bags_finished(bad, 5, 0, bad, 52, bad, 26, None, f, None) != 0       # width
    assert L.ha_push_apply_scaled_bags_finished(None, 5, 8, bad, 52, bad, 26, None, f, None) != 0      # no table
    assert L.ha_push_apply_scaled_bags_finished(bad, 5, 8, bad, 52, None, 26, None, f, None) != 0      # no gradient
    assert b"ha_push_apply_scaled_bags_finished" in L.ha_last_error()
    assert L.ha_apply_mapped_bags(bad, 5, 8, bad, 52, bad, f, bad, 0, None, None, None) != 0
    assert L.ha_apply_mapped_bags(bad, 5, 8, bad, 52, bad, f, bad, 26, bad, None, None) != 0
    assert L.ha_apply_mapped_bags(bad, 5, 8, bad, 52, bad, f, bad, 25, None, None, None) != 0
    assert L.ha_apply_mapped_bags(None, 5, 8, bad, 52, bad, f, bad, 26, None, None, None) != 0
    assert b"ha_apply_mapped_bags" in L.ha_last_error()
    # n == 0 is a call that does nothing
    assert L.ha_push_apply_scaled_bags_finished(None, 5, 8, None, 0, None, 26, None, f, None) == 0
    assert L.ha_apply_mapped_bags(None, 5, 8, None, 0, None, f, None, 26, None, None, None) == 0
    torch.cuda.synchronize()

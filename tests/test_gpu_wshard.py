"""Weighted bags on the row-sharded table on the GPU: ha_gather_wsum_u32keys against the numpy restatement (tests/wshard_model.py)
and the float-id kernel, ha_dedup_reduce_wbags against ha_wbag_grad_rows + ha_dedup_reduce_scaled on the same plan (whole
output buffers) and against the restatement, and ShardedEmbedding.pull_wsum / push_wbags / push_pull_wbags at world size 1
against pull / push on a twin store.  Every comparison is on float32 bit patterns."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bag_model     # noqa: E402
import wbag_model    # noqa: E402
import wshard_model  # noqa: E402

from herald_amd import _lib, ops  # noqa: E402
from herald_amd.sharded import ShardedEmbedding  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = -123.456


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same_as_model(got, want):
    """Bit patterns equal; where the restatement holds a NaN the kernel holds one too (a NaN's payload is the host's or the
    device's own; kernel against kernel the comparisons below are on every bit)."""
    g, w = got.detach().cpu().numpy(), np.asarray(want, dtype=np.float32)
    return g.shape == w.shape and bool(np.all((_bits(g) == _bits(w)) | (np.isnan(g) & np.isnan(w))))


# ---- ha_gather_wsum_u32keys -----------------------------------------------------------------------------------------------------
BUF_ROWS = 300
_bufs = {}


def _rows_buf(width):
    """One 300-row buffer per width, shared and never written: magnitudes over many binades so that the order of a sum shows."""
    if width not in _bufs:
        rng = np.random.default_rng(2000 + width)
        _bufs[width] = (rng.standard_normal((BUF_ROWS, width)) * np.exp(rng.uniform(-8, 8, (BUF_ROWS, 1)))).astype(np.float32)
    return _bufs[width]


def _keys(n, seed):
    rng = np.random.default_rng(seed)
    k = rng.integers(0, BUF_ROWS, n).astype(np.int32)
    k[: n // 3] = k[0]                                  # repeats
    if n > 4:
        k[n - 2] = BUF_ROWS + 7                         # a key beyond the buffer: dead whatever its weight
    return rng.permutation(k)


def _weights(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "ones":
        return np.ones(n, dtype=np.float32)
    if kind == "mask":
        return (rng.random(n) < 0.5).astype(np.float32)
    w = rng.standard_normal(n).astype(np.float32)
    w[rng.random(n) < 0.3] = 0
    return w


def _check_wsum(dev, buf, keys, w, offsets=None, d_buf=None, misaligned_out=False):
    """gather_wsum_u32keys on (buf, keys, w) equals the restatement and the float-id kernel; inputs stay as they were."""
    d_buf = torch.from_numpy(buf).to(dev) if d_buf is None else d_buf
    d_keys, d_w = torch.from_numpy(keys).to(dev), torch.from_numpy(w.reshape(keys.shape)).to(dev)
    d_off = torch.from_numpy(np.asarray(offsets, dtype=np.int64)).to(dev) if offsets is not None else None
    nbags, width = (keys.shape[0] if offsets is None else len(offsets) - 1), buf.shape[1]
    if misaligned_out:
        base = torch.full((nbags * width + 4,), CANARY, dtype=torch.float32, device=dev)
        out = base[1:1 + nbags * width].view(nbags, width)
        assert out.data_ptr() % 16 == 4
    else:
        out = torch.full((nbags, width), CANARY, dtype=torch.float32, device=dev)
    got = ops.gather_wsum_u32keys(d_buf, d_keys, d_w, offsets=d_off, out=out)
    assert got is out
    want = wshard_model.gather_wsum_u32keys(buf, keys, w, bag=keys.shape[-1] if offsets is None else None,
                                            offsets=None if offsets is None else np.asarray(offsets, dtype=np.int64))
    assert _same_as_model(got, want)
    twin = ops.embedding_lookup_wsum(d_buf, d_keys.to(torch.float32), d_w, offsets=d_off)
    assert np.array_equal(_bits(got), _bits(twin))
    assert not np.any(_bits(got) == _bits(np.float32(CANARY)))
    assert np.array_equal(_bits(d_buf), _bits(buf)) and np.array_equal(d_keys.cpu().numpy(), keys)
    assert np.array_equal(_bits(d_w), _bits(w.reshape(keys.shape)))
    return got


@pytest.mark.parametrize("F", [1, 8, 9, 26, 64, 65, 130])       # 8 / 9: the ROWS switch; 64 / 65 / 130: the 64-id block
def test_gather_wsum_u32keys_fixed_bags(dev, F):
    for width in (4, 37, 64):
        for B, kind in ((3, "general"), (41, "mask")):
            keys = _keys(B * F, 10 * F + B).reshape(B, F)
            _check_wsum(dev, _rows_buf(width), keys, _weights(kind, B * F, F + width))


@pytest.mark.parametrize("width", [1, 33, 64, 66, 128, 260])
def test_gather_wsum_u32keys_every_slice_width(dev, width):
    for B, bag in ((33, 26), (2100, 3)):                # 2,100 bags: the launch rule takes its wider slices
        keys = _keys(B * bag, 5 + B).reshape(B, bag)
        _check_wsum(dev, _rows_buf(width), keys, _weights("general", B * bag, width))


def test_gather_wsum_u32keys_ragged_bags_and_the_clamp(dev):
    n = 300
    keys, w = _keys(n, 77), _weights("general", n, 78)
    offsets = [0, 0, 0, 200, 200, 201, 230, 230, 300, 300, 300]      # empty bags, one bag of 200 ids, one of 1
    for width in (4, 37, 64):
        _check_wsum(dev, _rows_buf(width), keys, w, offsets)
    for width in (37, 64):                              # offsets beyond n (and a decreasing one): clamped
        _check_wsum(dev, _rows_buf(width), keys, w, [0, 50, 40, 290, 350, 1000])


def test_gather_wsum_u32keys_misaligned_buffers_take_the_scalar_path(dev):
    width = 64
    buf = _rows_buf(width)
    base = torch.zeros(BUF_ROWS * width + 4, dtype=torch.float32, device=dev)
    d_buf = base[1:1 + BUF_ROWS * width].view(BUF_ROWS, width)      # 4 bytes into its allocation
    d_buf.copy_(torch.from_numpy(buf))
    assert d_buf.data_ptr() % 16 == 4
    keys, w = _keys(20 * 26, 3).reshape(20, 26), _weights("general", 20 * 26, 4)
    a = _check_wsum(dev, buf, keys, w, d_buf=d_buf)
    b = _check_wsum(dev, buf, keys, w, misaligned_out=True)
    c = _check_wsum(dev, buf, keys, w)
    assert np.array_equal(_bits(a), _bits(c)) and np.array_equal(_bits(b), _bits(c))


def test_gather_wsum_u32keys_all_ones_is_gather_sum_u32keys(dev):
    for width, F in ((64, 26), (37, 65)):
        buf, keys = _rows_buf(width), _keys(41 * F, F).reshape(41, F)
        got = _check_wsum(dev, buf, keys, _weights("ones", keys.size, 0))
        plain = ops.gather_sum_u32keys(torch.from_numpy(buf).to(dev), torch.from_numpy(keys).to(dev))
        assert np.array_equal(_bits(got), _bits(plain))


def test_gather_wsum_u32keys_zero_signs_nan_weights_and_poisoned_dead_rows(dev):
    width, B, F = 64, 12, 26
    buf = _rows_buf(width).copy()
    rng = np.random.default_rng(9)
    keys = rng.integers(3, BUF_ROWS, (B, F)).astype(np.int32)
    w = rng.standard_normal((B, F)).astype(np.float32)
    dead = rng.random((B, F)) < 0.4
    keys[dead] = rng.integers(0, 3, int(dead.sum()))    # rows 0 .. 2 are named by dead occurrences only
    w[dead] = np.where(rng.random(int(dead.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
    buf[0], buf[1], buf[2] = np.inf, np.nan, -np.inf
    got = _check_wsum(dev, buf, keys, w.reshape(-1))
    assert np.all(np.isfinite(got.cpu().numpy()))
    w[1, 5] = np.nan                                    # a NaN weight is not zero: live
    keys[1, 5] = 7
    got = _check_wsum(dev, buf, keys, w.reshape(-1))
    assert np.all(np.isnan(got.cpu().numpy()[1])) and np.all(np.isfinite(got.cpu().numpy()[2]))


# ---- ha_dedup_reduce_wbags ------------------------------------------------------------------------------------------------------
RUNS = (1, 47, 48, 49, 120, 121, 241)      # kPlanLongRun = 48: the short / long switch; kWbagCoopRound = 120: one, two, three rounds
PATTERNS = ("live", "dead", "last", "first", "alternating")
F = 26
N_RUNS = -(-(sum(RUNS) + 150) // F) * F


def _run_key(j):
    return 7 + 11 * j


def _run_case(pattern, seed, rows=30000):
    """ids with one key per entry of RUNS repeated that often (shuffled among random ids) and weights: general with a third
    dead outside the runs, `pattern` inside every run."""
    rng = np.random.default_rng(seed)
    parts = [np.full(c, _run_key(j), dtype=np.int64) for j, c in enumerate(RUNS)]
    parts.append(rng.integers(1000, rows, N_RUNS - sum(RUNS)))
    ids = rng.permutation(np.concatenate(parts)).astype(np.float32)
    w = rng.standard_normal(ids.size).astype(np.float32)
    w[rng.random(ids.size) < 0.33] = 0
    for j, c in enumerate(RUNS):
        at = np.flatnonzero(ids == _run_key(j))
        assert at.size == c
        live = {"live": np.ones(c, bool), "dead": np.zeros(c, bool), "last": np.arange(c) == c - 1,
                "first": np.arange(c) == 0, "alternating": np.arange(c) % 2 == 1}[pattern]
        w[at] = np.where(live, np.where(w[at] == 0, np.float32(0.75), w[at]), np.float32(0))
    return ids, w


def _ragged_offsets(n, nbags, seed):
    cuts = np.sort(np.random.default_rng(seed).integers(0, n + 1, nbags - 4))
    h = cuts.size // 2
    return np.concatenate([[0, 0], cuts[:h], [cuts[h]], cuts[h:], [n, n]]).astype(np.int64)


def _check_reduce(dev, ids, w, g, bag=None, offsets=None, scale=1.0, plan_ids=None, d_g=None, model=True):
    """dedup_reduce_wbags equals wbag_grad_rows + dedup_reduce(scale) on the SAME plan over the whole output buffer (both
    pre-filled with the same canary) and the restatement; inputs stay as they were."""
    n, width = ids.size, g.shape[1]
    d_ids = torch.from_numpy(ids if plan_ids is None else plan_ids).to(dev)
    plan = ops.IndexPlan(n, dev).build(d_ids.reshape(-1))
    d_w = torch.from_numpy(w).to(dev)
    d_g = torch.from_numpy(g).to(dev) if d_g is None else d_g
    d_bag_of = ops.bag_of(torch.from_numpy(offsets).to(dev), n) if offsets is not None else None
    which = wshard_model.which_of(n, bag=bag, offsets=offsets)
    rows = ops.wbag_grad_rows(d_g, d_w, bag=bag, bag_of=d_bag_of)
    want = torch.full((n, width), CANARY, dtype=torch.float32, device=dev)
    ops.dedup_reduce(plan, rows, out=want, scale=scale)
    got = torch.full((n, width), CANARY, dtype=torch.float32, device=dev)
    assert ops.dedup_reduce_wbags(plan, d_g, d_w, bag=bag, bag_of=d_bag_of, scale=scale, out=got) is got
    torch.cuda.synchronize()
    assert np.array_equal(_bits(got), _bits(want))
    u = plan.n_unique()
    assert not np.any(_bits(got[:u]) == _bits(np.float32(CANARY)))
    if model:
        inv = plan.inverse().cpu().numpy()
        red = wshard_model.dedup_reduce_wbags(inv, u, g, w, which, scale)
        assert np.array_equal(_bits(got[:u]), _bits(red))
    assert np.array_equal(_bits(d_g), _bits(g)) and np.array_equal(_bits(d_w), _bits(w))
    return got, plan


@pytest.mark.parametrize("pattern", PATTERNS)
def test_dedup_reduce_wbags_runs_across_every_switch(dev, pattern):
    ids, w = _run_case(pattern, 11)
    g = np.random.default_rng(3).standard_normal((ids.size // F, 64)).astype(np.float32)
    got, plan = _check_reduce(dev, ids, w, g, bag=F, scale=-0.05)
    if pattern == "dead":                               # the rows of the all-dead runs are +0.0f
        inv = plan.inverse().cpu().numpy()
        for j in range(len(RUNS)):
            at = int(inv[np.flatnonzero(ids == _run_key(j))[0]])
            assert not np.any(_bits(got[at]))


def test_dedup_reduce_wbags_whole_batch_all_dead(dev):
    """Every id the padding id, every weight zero: one run of the whole batch, no live occurrence."""
    n = F * 40
    ids, w = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    w[::3] = -0.0
    g = np.random.default_rng(4).standard_normal((n // F, 64)).astype(np.float32)
    g[5] = np.nan
    got, plan = _check_reduce(dev, ids, w, g, bag=F, scale=-0.05)
    assert plan.n_unique() == 1
    assert not np.any(_bits(got[:1]))
    assert np.all(_bits(got[1:]) == _bits(np.float32(CANARY)))


@pytest.mark.parametrize("width", [64, 66, 4, 260])
def test_dedup_reduce_wbags_widths_scales_and_zero_gradients(dev, width):
    ids, w = _run_case("alternating", 12)
    rng = np.random.default_rng(width)
    g = rng.standard_normal((ids.size // F, width)).astype(np.float32)
    g[rng.random(g.shape) < 0.3] = 0                     # zero elements: with scale < 0 the composed sequence adds -0 terms
    for scale in (1.0, -0.05):
        _check_reduce(dev, ids, w, g, bag=F, scale=scale)


def test_dedup_reduce_wbags_ragged_bags(dev):
    for pattern in ("live", "alternating"):
        ids, w = _run_case(pattern, 13)
        offsets = _ragged_offsets(ids.size, 40, 3)
        for width in (64, 66):
            g = np.random.default_rng(width).standard_normal((offsets.size - 1, width)).astype(np.float32)
            _check_reduce(dev, ids, w, g, offsets=offsets, scale=-0.05)


def test_dedup_reduce_wbags_misaligned_bag_grads(dev):
    ids, w = _run_case("alternating", 14)
    B, width = ids.size // F, 64
    g = np.random.default_rng(12).standard_normal((B, width)).astype(np.float32)
    aligned, _ = _check_reduce(dev, ids, w, g, bag=F, scale=-0.05)
    base = torch.zeros(B * width + 4, dtype=torch.float32, device=dev)
    d_g = base[1:1 + B * width].view(B, width)                      # 4 bytes into its allocation: the scalar path
    d_g.copy_(torch.from_numpy(g))
    assert d_g.data_ptr() % 16 == 4
    plan = ops.IndexPlan(ids.size, dev).build(torch.from_numpy(ids).to(dev))
    got = torch.full((ids.size, width), CANARY, dtype=torch.float32, device=dev)
    ops.dedup_reduce_wbags(plan, d_g, torch.from_numpy(w).to(dev), bag=F, scale=-0.05, out=got)
    assert np.array_equal(_bits(got), _bits(aligned))
    assert np.array_equal(_bits(d_g), _bits(g))


def test_dedup_reduce_wbags_int64_ids_equal_their_float32_twins(dev):
    ids, w = _run_case("alternating", 15)
    g = np.random.default_rng(6).standard_normal((ids.size // F, 64)).astype(np.float32)
    a, _ = _check_reduce(dev, ids, w, g, bag=F, scale=-0.05)
    b, _ = _check_reduce(dev, ids, w, g, bag=F, scale=-0.05, plan_ids=ids.astype(np.int64))
    assert np.array_equal(_bits(a), _bits(b))


def test_dedup_reduce_wbags_poisoned_gradients_of_dead_bags_reach_nothing(dev):
    ids, w = _run_case("first", 16)
    B = ids.size // F
    g = np.random.default_rng(7).standard_normal((B, 64)).astype(np.float32)
    w = w.reshape(B, F)
    for b, poison in ((0, np.inf), (3, np.nan), (B - 1, -np.inf)):      # bags whose occurrences are all dead
        w[b] = 0
        g[b] = poison
    got, plan = _check_reduce(dev, ids, w.reshape(-1), g, bag=F, scale=-0.05)
    assert np.all(np.isfinite(got[:plan.n_unique()].cpu().numpy()))


def test_dedup_reduce_wbags_clamps_bag_of(dev):
    """bag_of entries beyond nbags - 1 read the last gradient row, as wbag_grad_rows reads it."""
    ids, w = _run_case("live", 17)
    n, nbags = ids.size, 20
    g = np.random.default_rng(8).standard_normal((nbags, 64)).astype(np.float32)
    bag_of = np.random.default_rng(9).integers(0, nbags, n).astype(np.int32)
    bag_of[::7] = nbags + 5
    bag_of[3] = -1
    d_bag_of, d_g, d_w = torch.from_numpy(bag_of).to(dev), torch.from_numpy(g).to(dev), torch.from_numpy(w).to(dev)
    plan = ops.IndexPlan(n, dev).build(torch.from_numpy(ids).to(dev))
    want = ops.dedup_reduce(plan, ops.wbag_grad_rows(d_g, d_w, bag_of=d_bag_of), scale=-0.05)
    got = ops.dedup_reduce_wbags(plan, d_g, d_w, bag_of=d_bag_of, scale=-0.05)
    u = plan.n_unique()
    assert np.array_equal(_bits(got[:u]), _bits(want[:u]))


@pytest.mark.parametrize("mode", [1, 2])
def test_dedup_reduce_wbags_in_tolerance_mode_is_the_composed_call(dev, mode):
    prev = ops.set_tolerance_mode(mode)
    try:
        ids, w = _run_case("alternating", 18)
        g = np.random.default_rng(mode).standard_normal((ids.size // F, 64)).astype(np.float32)
        _check_reduce(dev, ids, w, g, bag=F, scale=-0.05, model=False)
        offsets = _ragged_offsets(ids.size, 40, 5)
        g = np.random.default_rng(mode + 2).standard_normal((offsets.size - 1, 66)).astype(np.float32)
        _check_reduce(dev, ids, w, g, offsets=offsets, scale=-0.05, model=False)
    finally:
        ops.set_tolerance_mode(prev)


def test_argument_errors_leave_a_poisoned_output_untouched(dev):
    n, width = 52, 8
    plan = ops.IndexPlan(n, dev).build(torch.arange(n, dtype=torch.float32, device=dev))
    g = torch.ones((2, width), dtype=torch.float32, device=dev)
    w = torch.ones(n, dtype=torch.float32, device=dev)
    out = torch.full((n, width), CANARY, dtype=torch.float32, device=dev)
    with pytest.raises(ValueError):
        ops.dedup_reduce_wbags(plan, g, w, out=out)                              # neither bag nor bag_of
    with pytest.raises(ValueError):
        ops.dedup_reduce_wbags(plan, g, w, bag=26, bag_of=torch.zeros(n, dtype=torch.int32, device=dev), out=out)
    with pytest.raises(ValueError):
        ops.dedup_reduce_wbags(plan, g, w, bag=13, out=out)                      # 4 bags of 13 need 4 gradient rows
    with pytest.raises(ValueError):
        ops.dedup_reduce_wbags(plan, g, w[:10], bag=26, out=out)
    L = _lib.load()
    vp = lambda t: t.data_ptr()      # noqa: E731
    assert L.ha_dedup_reduce_wbags(vp(plan.ws), n, vp(g), vp(w), width, 0, None, 2, 1.0, vp(out), None) != 0
    assert b"exactly one" in L.ha_last_error()
    assert L.ha_dedup_reduce_wbags(vp(plan.ws), n, vp(g), vp(w), width, 5, None, 2, 1.0, vp(out), None) != 0
    assert L.ha_dedup_reduce_wbags(vp(plan.ws), n, vp(g), vp(w), 0, 26, None, 2, 1.0, vp(out), None) != 0
    assert L.ha_dedup_reduce_wbags(vp(plan.ws), n, vp(g), None, width, 26, None, 2, 1.0, vp(out), None) != 0
    assert b"null" in L.ha_last_error()
    assert L.ha_dedup_reduce_wbags(vp(plan.ws), n, vp(g), vp(w), width, 26, None, 2, 1.0, vp(g), None) != 0      # aliased
    # the forward: no rows to read, bad bags, null weights
    keys = torch.zeros(n, dtype=torch.int32, device=dev)
    buf = torch.ones((4, width), dtype=torch.float32, device=dev)
    o2 = torch.full((2, width), CANARY, dtype=torch.float32, device=dev)
    assert L.ha_gather_wsum_u32keys(vp(buf), 0, width, vp(keys), vp(w), n, 26, None, 2, vp(o2), None) != 0
    assert b"rows" in L.ha_last_error()
    assert L.ha_gather_wsum_u32keys(vp(buf), 4, width, vp(keys), vp(w), n, 25, None, 2, vp(o2), None) != 0
    assert L.ha_gather_wsum_u32keys(vp(buf), 4, width, vp(keys), None, n, 26, None, 2, vp(o2), None) != 0
    assert L.ha_gather_wsum_u32keys(vp(buf), 4, width, vp(keys), vp(w), n, 26, vp(keys), 2, vp(o2), None) != 0   # bag and offsets
    with pytest.raises(ValueError):
        ops.gather_wsum_u32keys(buf, keys.view(2, 26), w[:5], out=o2)
    torch.cuda.synchronize()
    assert np.all(_bits(out) == _bits(np.float32(CANARY))) and np.all(_bits(o2) == _bits(np.float32(CANARY)))
    assert np.all(_bits(g) == _bits(np.float32(1.0)))
    assert L.ha_dedup_reduce_wbags(None, 0, None, None, width, 26, None, 0, 1.0, None, None) == 0              # n == 0


# ---- ShardedEmbedding at world size 1 ----------------------------------------------------------------------------------------
ROWS, B = 5000, 50


def _store_case(kind):
    """(width, ids as numpy in the shape the store takes, weights in that shape, offsets or None): FAE data -- half of the
    slots dead, naming the padding id 0 -- with general weights on the live ones."""
    rng = np.random.default_rng(40)
    ids = rng.integers(1, ROWS, (B, F))
    ids[:, :3] = ids[0, :3]                 # keys shared by every bag
    w = rng.standard_normal((B, F)).astype(np.float32)
    dead = rng.random((B, F)) < 0.5
    ids[dead], w[dead] = 0, 0
    width = 33 if kind == "d33" else 64
    if kind == "ragged":
        return width, ids.reshape(-1).astype(np.float32), w.reshape(-1), _ragged_offsets(B * F, B, 41)
    return width, ids.astype(np.int64 if kind == "int64" else np.float32), w, None


@pytest.mark.parametrize("kind", ["fixed", "ragged", "int64", "d33"])
def test_sharded_pull_wsum_and_push_wbags_at_world_size_1(dev, kind):
    width, ids, w, offsets = _store_case(kind)
    rng = np.random.default_rng(42)
    table0 = rng.standard_normal((ROWS, width)).astype(np.float32)
    g = rng.standard_normal((B, width)).astype(np.float32)
    g2 = rng.standard_normal((B, width)).astype(np.float32)
    lr = 0.05
    d_ids, d_w = torch.from_numpy(ids).to(dev), torch.from_numpy(w).to(dev)
    d_off = torch.from_numpy(offsets).to(dev) if offsets is not None else None
    d_bag_of = ops.bag_of(d_off, ids.size) if offsets is not None else None
    bag = None if offsets is not None else F
    d_g, d_g2 = torch.from_numpy(g).to(dev), torch.from_numpy(g2).to(dev)
    emb = ShardedEmbedding(ROWS, width, dev, table=torch.from_numpy(table0).to(dev))
    twin = ShardedEmbedding(ROWS, width, dev, table=torch.from_numpy(table0).to(dev))
    pos = torch.arange(B * F, dtype=torch.int64, device=dev).view(d_ids.shape)

    def twin_rows():
        return ops.embedding_lookup_wsum(twin.pull(d_ids).reshape(-1, width), pos, d_w, offsets=d_off)

    def twin_push(grads, route=None):
        twin.push(d_ids if route is None else None, ops.wbag_grad_rows(grads, d_w, bag=bag, bag_of=d_bag_of), lr, route=route)

    # pull_wsum: pull + embedding_lookup_wsum over the row buffer, and the restatement on the table
    got = emb.pull_wsum(d_ids, d_w, offsets=d_off)
    assert got.shape == (B, width)
    assert np.array_equal(_bits(got), _bits(twin_rows()))
    assert np.array_equal(_bits(got), _bits(wbag_model.wbag_sum(table0, ids, w, offsets)))
    assert np.any(_bits(got))

    # push_wbags: push of wbag_grad_rows on the twin
    emb.push_wbags(d_ids, d_g, d_w, lr, offsets=d_off)
    twin_push(d_g)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(emb.table), _bits(twin.table))
    assert not np.array_equal(_bits(emb.table), _bits(table0))

    # one prefetched route serves pull (fixed bags: [B, F, d]), pull_wsum ([B, d]) and push_wbags
    route = emb.prefetch(d_ids)
    if offsets is None:
        assert emb.pull(route=route).shape == (B, F, width)
    out = torch.full((B, width), CANARY, dtype=torch.float32, device=dev)
    got, r = emb.pull_wsum(weights=d_w, offsets=d_off, route=route, return_route=True, out=out)
    assert got is out and r is route
    troute = twin.prefetch(d_ids)
    if offsets is None:
        twin.pull(route=troute)
    rows = twin.pull(route=troute).reshape(-1, width)
    assert np.array_equal(_bits(got), _bits(ops.embedding_lookup_wsum(rows, pos, d_w, offsets=d_off)))
    emb.push_wbags(None, d_g2, d_w, lr, offsets=d_off, route=route)
    twin_push(d_g2, route=troute)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(emb.table), _bits(twin.table))

    # push_pull_wbags: the pull sees the push
    got = emb.push_pull_wbags(d_ids, d_g, d_w, lr, d_ids, d_w, push_offsets=d_off, pull_offsets=d_off)
    twin_push(d_g)
    want = twin_rows()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(emb.table), _bits(twin.table))
    assert emb.stats == twin.stats
    # inputs as they were
    assert np.array_equal(d_ids.cpu().numpy(), ids) and np.array_equal(_bits(d_g), _bits(g))
    assert np.array_equal(_bits(d_g2), _bits(g2)) and np.array_equal(_bits(d_w), _bits(w))


def test_sharded_wbag_calls_refuse_bad_arguments_before_any_collective(dev):
    width = 16
    emb = ShardedEmbedding(ROWS, width, dev)
    flat = torch.zeros(B * F, dtype=torch.float32, device=dev)
    ids, wt = flat.view(B, F), torch.ones((B, F), dtype=torch.float32, device=dev)
    good = torch.zeros((B, width), dtype=torch.float32, device=dev)
    stats = dict(emb.stats)
    with pytest.raises(ValueError, match="offsets"):
        emb.pull_wsum(flat, wt.view(-1))                                         # flat ids without offsets
    with pytest.raises(ValueError, match="weights"):
        emb.pull_wsum(ids, wt.view(-1))                                          # not the ids' shape
    with pytest.raises(ValueError, match="weights"):
        emb.pull_wsum(ids, wt.double())                                          # wrong dtype
    with pytest.raises(ValueError, match="weights"):
        emb.pull_wsum(ids, wt.cpu())                                             # another device
    with pytest.raises(ValueError, match="weights"):
        emb.pull_wsum(ids)                                                       # no weights at all
    with pytest.raises(ValueError, match="out"):
        emb.pull_wsum(ids, wt, out=torch.zeros((B, width + 1), dtype=torch.float32, device=dev))
    with pytest.raises(ValueError, match="bag_values"):
        emb.push_wbags(ids, torch.zeros((B * F, width), dtype=torch.float32, device=dev), wt, 0.1)
    with pytest.raises(ValueError, match="weights"):
        emb.push_wbags(ids, good, wt[:, :5].contiguous(), 0.1)
    with pytest.raises(ValueError, match="int64"):
        emb.pull_wsum(flat, wt.view(-1), offsets=torch.zeros(B + 1, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="weights"):
        emb.push_pull_wbags(ids, good, wt, 0.1, ids, wt.view(-1))
    assert emb.stats == stats and emb._slot == 0      # nothing was routed

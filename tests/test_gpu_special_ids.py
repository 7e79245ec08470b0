"""Special ids -- negative, NaN, infinite, at or beyond 2^32, and the live edges -0.0, -0.99, rows - 0.5 -- through every consumer
of ids, against the one id rule (include/herald_amd.h, "Which ids name a row"; tests/special_ids.py is its numpy statement).

ONE batch shape for every consumer (make_batch): ordinary ids, every special of the list twice, two genuine occurrences of
id 0.  The float32 and the int64 form of a batch name the same logical ids position by position (PAIRS), so they have the same
keys and every consumer must give the same bits for both.  Row 0 of every table and the gradients of the genuine id-0
occurrences hold values nothing else holds: an id that leaks into row 0 (what a saturating conversion makes of -1.0 or NaN)
changes bits.

Expected result: the model of the same batch with every dead id replaced by rows + 1 (special_ids.replace_dead), compared on
the bits.  The optimizers whose arithmetic holds a square root and a division are held to their numpy model within the
reference tests' 1e-5 (tests/test_gpu_optim.py), so there the bit-for-bit yardstick is the library's own result on the
replaced batch -- ids the suite already covers -- and the numpy model is compared at that tolerance besides.  Also: rows no
live id names keep their bits, and the lookup rows of dead occurrences are +0.0.  Plans are compared with numpy on
special_ids.keys_of (all dead occurrences: one run of key 0xFFFFFFFE, exported as 4294967296.0).

Where every float-id conversion of csrc/ is exercised (grep f32_to_key|to_key<|id_to_row<|static_cast<uint32_t>( ):

    site                                                           case
    common.h f32_to_key                                            all of the below
    gather.hip:40 gather_scalar (width 5)                          test_lookup[5]
    gather_dev.h:53 gather_vec4_body (width 4)                     test_lookup[4], test_apply_finish_and_prefetch (lookup_sort)
    gather.hip:105 scatter_rows (DLGpuEmbeddingLookUp_Gradient)    test_lookup_gradient_symbol
    bagsum.hip:80 bag_sum / :235 fm                                test_pooled_lookups
    wbag.hip:99 wbag_sum / :176 masked keys                        test_pooled_lookups, test_bag_applies (wbags one call)
    plan_dev.h:272,356 rank_tile_body_f32 (rank by counting)       test_plan_rank_by_counting[f32], every 60-id plan below
    plan_dev.h:175 rank_tile_body_int                              test_plan_rank_by_counting[i64]
    plan_dev.h:118 radix_first_tile_body                           test_plan_radix, test_plan_bucket_sort
    plan.hip:953 key range scan of the bucket sort                 test_plan_bucket_sort
    plan.hip plan_sort_wg_batch / plan_rank_small_batch            test_plan_batched_one_workgroup_sort
    fused.hip:65 prefetch of the next batch's rows                 test_apply_finish_and_prefetch
    fused.hip fwd_fused / fwd_large (lookup_sort)                  test_apply_finish_and_prefetch, test_plan_radix
    optim.hip:57 sparse_row_kernel (row_launch)                    test_dl_named_optimizers
    step.hip:98,175 gather of the step launches                    test_push_pull, test_step_pipeline
    qstep.hip:298 qplan / :2037,2099 wide path buckets             test_queue_step_pipeline, test_queue_step_pipeline_wide
    herald_amd/hetu_ops.py sgd_update_sparse, ragged weighted      test_hetu_ops_sgd_update_sparse_on_weighted_slices (the one conversion
      slices: masked keys built with torch                         outside csrc/)
    cache.hip:1834 cache_f32_to_u32_kernel, cache_block.hip:943    not run here: these tiers index per-row arrays by key and REQUIRE
                                                                   in-range ids (header; cache.py, sharded.py); the conversion
                                                                   they share is f32_to_key, held by every case above
"""
import ctypes

import numpy as np
import pytest
import torch

import bag_model
import fm_model
import fm_pooled_model
import special_ids
import wbag_model
from herald_amd import _lib, ops
from oracle import cpu

pytestmark = pytest.mark.gpu

ROWS, N, BAG = 37, 60, 3
DEAD = special_ids.DEAD_KEY
LR = 0.05
RAGGED = np.cumsum([0, 3, 0, 3, 1, 5, 3, 3, 2, 4] + [3] * 12).astype(np.int64)       # 21 bags over 60 ids, one empty
assert RAGGED[-1] == N
OPT_TOL = dict(rtol=1e-5, atol=1e-5)      # tests/test_gpu_optim.py: the tolerance the reference's optimizer tests state


def pairs(rows):
    """[(float32 form, int64 form)] of the same logical id: both special lists, every entry of either at least once."""
    f = np.float32
    neg_nan = np.array([0xFFC00000], dtype=np.uint32).view(np.float32)[0]
    return [
        (f(-1.0), -1), (f(-1.5), -1), (f(-3e9), special_ids.INT64_MIN), (f(-np.inf), special_ids.INT64_MIN),
        (f(np.inf), 2 ** 63 - 1), (f(3.4e38), 2 ** 63 - 1), (f(np.nan), 0xFFFFFFFF), (neg_nan, 0xFFFFFFFE),
        (special_ids.nan_with_payload(), 2 ** 32 + 5), (f(4294967296.0), 2 ** 32), (f(4294967040.0), 0xFFFFFF00),
        (f(rows), rows),
        (f(-0.0), 0), (f(-0.99), 0), (f(rows - 1), rows - 1), (f(rows - 0.5), rows - 1),
    ]


def make_batch(rows=ROWS, n=N, seed=0, extra_dead=0, ordinary=None):
    """-> (float32 ids [n], int64 ids [n], positions of the genuine id-0 occurrences).  Every pair twice, `extra_dead` more
    occurrences of the ids whose key is the dead key, two genuine zeros, the rest ordinary ids of [1, rows)."""
    rng = np.random.default_rng(seed)
    base = rng.integers(1, rows, n) if ordinary is None else np.asarray(ordinary)
    fl, it = base.astype(np.float32), base.astype(np.int64)
    pr = pairs(rows)
    dead_pr = [p for p in pr if special_ids.keys_of(np.array([p[0]]))[0] == DEAD]
    entries = pr * 2 + [dead_pr[k % len(dead_pr)] for k in range(extra_dead)] + [(np.float32(0.0), 0)] * 2
    assert len(entries) <= n
    slots = rng.permutation(n)[:len(entries)]
    for s, (a, b) in zip(slots, entries):
        fl[s], it[s] = a, b
    np.testing.assert_array_equal(special_ids.keys_of(fl), special_ids.keys_of(it))
    return fl, it, np.sort(slots[-2:])


def make_table(rows, width, seed=1):
    t = np.random.default_rng(seed).standard_normal((rows, width)).astype(np.float32)
    t[0] = 1000.0 + np.arange(width, dtype=np.float32)          # values no other row holds
    return t


def make_grads(n, width, zeros_at=(), seed=2):
    g = np.random.default_rng(seed).standard_normal((n, width)).astype(np.float32)
    for j, p in enumerate(zeros_at):
        g[p] = -500.0 - 10.0 * j - np.arange(width, dtype=np.float32)      # values no other gradient holds
    mine = np.concatenate([g[p] for p in zeros_at]) if len(zeros_at) else g[:0].reshape(-1)
    assert np.unique(mine).size == mine.size and np.count_nonzero(np.isin(g, mine)) == mine.size
    return g


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same(got, want, what=""):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32, what
    np.testing.assert_array_equal(got.reshape(want.shape).view(np.uint32), want.view(np.uint32), err_msg=what)


def _rep(ids, rows=ROWS):
    return special_ids.replace_dead(ids, rows)


def _repf(ids, rows=ROWS):
    """The replaced batch as float32 ids (exact: every id left is at most rows + 1): what the float-only models take."""
    return _rep(ids, rows).astype(np.float32)


def _dead(ids, rows=ROWS):
    return special_ids.keys_of(ids) >= np.uint64(rows)


def _untouched(ids, rows=ROWS):
    """Rows no live id of the batch names."""
    keys = special_ids.keys_of(ids)
    named = np.zeros(rows, dtype=bool)
    named[keys[keys < np.uint64(rows)].astype(np.int64)] = True
    return ~named


def _forms(fl, it):
    return (("f32", fl), ("i64", it))


# ---- lookups ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [4, 5])
def test_lookup(dev, width):
    fl, it, _ = make_batch()
    table = make_table(ROWS, width)
    want = cpu.embedding_lookup(table, _repf(fl))
    assert not want[_dead(fl)].view(np.uint32).any() and want[~_dead(fl)].any(axis=1).all()
    t = _dev(table, dev)
    for name, ids in _forms(fl, it):
        got = ops.embedding_lookup(t, _dev(ids, dev))
        _same(got, want, "embedding_lookup " + name)
        assert not got.cpu().numpy()[_dead(ids)].view(np.uint32).any(), "dead occurrences are rows of +0.0"
        got2 = ops.embedding_lookup(t, _dev(ids.reshape(20, 3), dev))
        _same(got2, want, "embedding_lookup [20, 3] " + name)
    out = torch.full((N, width), 7.0, dtype=torch.float32, device=dev)
    ops.dl_call("DLGpuEmbeddingLookUp", [t, _dev(fl, dev), out])
    torch.cuda.synchronize()
    _same(out, want, "DLGpuEmbeddingLookUp")
    _same(t, table, "the table is read only")


@pytest.mark.parametrize("width", [4, 5])
def test_lookup_gradient_symbol(dev, width):
    """DLGpuEmbeddingLookUp_Gradient: the dense gradient = zeros + scatter-add of the rows; dead ids add nothing anywhere."""
    fl, _, zeros_at = make_batch()
    vals = make_grads(N, width, zeros_at)
    uniq, _, red = cpu.dedup_reduce(_repf(fl), vals)
    want = cpu.push_apply(np.zeros((ROWS, width), dtype=np.float32), uniq, red)
    g = torch.full((ROWS, width), 7.0, dtype=torch.float32, device=dev)
    ops.dl_call("DLGpuEmbeddingLookUp_Gradient", [_dev(vals, dev), _dev(fl, dev), g])
    torch.cuda.synchronize()
    _same(g, want)
    assert not g.cpu().numpy()[_untouched(fl)].view(np.uint32).any()
    t = _dev(make_table(ROWS, width), dev)
    ops.dl_call("IndexedSlicesOneSideAdd", [_dev(fl, dev), _dev(vals, dev), t])
    torch.cuda.synchronize()
    _same(t, cpu.push_apply(make_table(ROWS, width), uniq, red), "IndexedSlicesOneSideAdd")


@pytest.mark.parametrize("ragged", [False, True], ids=["fixed", "ragged"])
@pytest.mark.parametrize("width", [4, 5])
def test_pooled_lookups(dev, width, ragged):
    fl, it, _ = make_batch()
    table = make_table(ROWS, width)
    t = _dev(table, dev)
    off = RAGGED if ragged else None
    d_off = _dev(RAGGED, dev) if ragged else None
    rep = _rep(fl) if ragged else _rep(fl).reshape(-1, BAG)
    want_sum = bag_model.bag_sum(table, rep, off)
    want_rows, covered, want_S, want_fm = fm_model.fm_lookup(table, rep, off)
    assert covered.all()
    ones = np.ones(N, dtype=np.float32)
    mask = (np.arange(N) % 3 != 1).astype(np.float32)
    want_w1 = wbag_model.wbag_sum(table, rep, ones, off)
    want_wm = wbag_model.wbag_sum(table, rep, mask, off)
    _same(want_w1, want_sum)
    for name, ids in _forms(fl, it):
        d_ids = _dev(ids if ragged else ids.reshape(-1, BAG), dev)
        _same(ops.embedding_lookup_sum(t, d_ids, d_off), want_sum, "embedding_lookup_sum " + name)
        rows, S, fm = ops.embedding_lookup_fm(t, d_ids, d_off)
        _same(rows, want_rows.reshape(tuple(d_ids.shape) + (width,)), "fm rows " + name)
        assert not rows.cpu().numpy().reshape(N, width)[_dead(ids)].view(np.uint32).any()
        _same(S, want_S, "fm sum " + name)
        _same(fm, want_fm, "fm " + name)
        none, S2, fm2 = ops.embedding_lookup_fm(t, d_ids, d_off, want_rows=False)
        assert none is None
        _same(S2, want_S, "fm sum without rows " + name)
        _same(fm2, want_fm, "fm without rows " + name)
        _same(ops.embedding_lookup_wsum(t, d_ids, _dev(ones, dev), d_off), want_w1, "wsum, weights 1 " + name)
        _same(ops.embedding_lookup_wsum(t, d_ids, _dev(mask, dev), d_off), want_wm, "wsum, 0/1 mask " + name)
    _same(t, table, "the table is read only")


# ---- plans ------------------------------------------------------------------------------------------------------------
def _u32(t):
    return (t.cpu().numpy().astype(np.int64) & 0xFFFFFFFF).astype(np.uint64)


def _check_plan(plan, ids, what, export=True):
    """As _check_plan of test_gpu_parity.py, against special_ids.keys_of."""
    torch.cuda.synchronize()
    keys = special_ids.keys_of(ids)
    uniq, inv, cnt = np.unique(keys, return_inverse=True, return_counts=True)
    u = plan.n_unique()
    assert u == uniq.size, what
    np.testing.assert_array_equal(_u32(plan.keys()), keys, err_msg=what + ": keys")
    np.testing.assert_array_equal(_u32(plan.uniq(u)), uniq, err_msg=what + ": uniq")
    np.testing.assert_array_equal(plan.inverse().cpu().numpy().astype(np.int64), inv, err_msg=what + ": inverse")
    np.testing.assert_array_equal(plan.counts(u).cpu().numpy().astype(np.int64), cnt, err_msg=what + ": counts")
    perm = plan.perm().cpu().numpy()
    np.testing.assert_array_equal(perm, np.argsort(keys, kind="stable"), err_msg=what + ": stable perm")
    np.testing.assert_array_equal(_u32(plan.sorted_keys()), keys[perm], err_msg=what + ": sorted keys")
    np.testing.assert_array_equal(plan.seg(u).cpu().numpy(), np.concatenate([[0], np.cumsum(cnt)]), err_msg=what + ": seg")
    assert uniq[-1] == DEAD and cnt[-1] == np.count_nonzero(keys == DEAD), "the dead occurrences: one run of one key"
    if export:
        uf, invf = plan.export_f32()
        want_uf = uniq.astype(np.float32)
        assert want_uf[-1] == np.float32(4294967296.0)
        np.testing.assert_array_equal(uf.cpu().numpy(), want_uf, err_msg=what + ": export_f32 uniq")
        np.testing.assert_array_equal(invf.cpu().numpy(), inv.astype(np.float32), err_msg=what + ": export_f32 inverse")


def _tiled(n, seed):
    """n ids: the 60-id batch first, then ordinary ids and more copies of it."""
    fl, it, _ = make_batch(seed=seed)
    rng = np.random.default_rng(seed)
    rest = rng.integers(0, ROWS, n - 3 * N)
    f = np.concatenate([fl, rest[:rest.size // 2].astype(np.float32), fl, rest[rest.size // 2:].astype(np.float32), fl])
    i = np.concatenate([it, rest[:rest.size // 2], it, rest[rest.size // 2:], it]).astype(np.int64)
    return f, i


@pytest.mark.parametrize("form", ["f32", "i64"])
def test_plan_rank_by_counting(dev, form):
    fl, it, _ = make_batch()
    ids = fl if form == "f32" else it
    _check_plan(ops.IndexPlan(N, dev).build(_dev(ids, dev)), ids, "build")
    p = ops.IndexPlan(N, dev).sort(_dev(ids, dev))
    p.finish()
    _check_plan(p, ids, "sort + finish")
    f2, i2 = _tiled(1000, 3)                       # several rank tiles
    ids = f2 if form == "f32" else i2
    _check_plan(ops.IndexPlan(1000, dev).build(_dev(ids, dev)), ids, "build of 1000")


@pytest.mark.parametrize("form", ["f32", "i64"])
def test_plan_bucket_sort(dev, form):
    n = 18433
    f, i = _tiled(n, 4)
    ids = f if form == "f32" else i
    _check_plan(ops.IndexPlan(n, dev).build(_dev(ids, dev), key_limit=ROWS), ids, "bucket sort")
    table = make_table(ROWS, 4)
    g = make_grads(n, 4)
    t = _dev(table, dev)
    plan = ops.IndexPlan(n, dev).sort(_dev(ids, dev), key_limit=ROWS)
    ops.sgd_apply(t, plan, _dev(g, dev), LR)
    torch.cuda.synchronize()
    _same(t, cpu.sgd_sparse_update(table.copy(), _repf(ids), g, LR), "sgd_apply on the bucket-sorted plan")


@pytest.mark.parametrize("form", ["f32", "i64"])
def test_plan_radix(dev, form):
    n = 36865
    f, i = _tiled(n, 5)
    ids = f if form == "f32" else i
    _check_plan(ops.IndexPlan(n, dev).build(_dev(ids, dev)), ids, "radix sort")
    table = make_table(ROWS, 4)
    t = _dev(table, dev)
    p2 = ops.IndexPlan(n, dev)
    out = ops.lookup_sort(t, _dev(ids, dev), p2)              # fwd_large: gather blocks beside the first radix pass
    p2.finish()
    _same(out, cpu.embedding_lookup(table, _repf(ids)), "lookup_sort rows")
    _check_plan(p2, ids, "lookup_sort plan", export=False)


@pytest.mark.parametrize("form", ["f32", "i64"])
def test_plan_batched_one_workgroup_sort(dev, form):
    """Two batches of 64 through ha_plan_build_batch_*_lim."""
    L = _lib.load()
    batches = [make_batch(n=64, seed=s)[0 if form == "f32" else 1] for s in (6, 7)]
    tens = [_dev(b, dev) for b in batches]
    plans = [ops.IndexPlan(64, dev) for _ in batches]
    fn = L.ha_plan_build_batch_f32ids_lim if form == "f32" else L.ha_plan_build_batch_u64ids_lim
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    _lib.check(fn((vp * 2)(*[t.data_ptr() for t in tens]), (i64 * 2)(64, 64), (vp * 2)(*[p.ws.data_ptr() for p in plans]), 2,
                  ctypes.c_uint64(ROWS), None), "plan_build_batch")
    for b, p in zip(batches, plans):
        p.n, p._view = 64, None
        _check_plan(p, b, "batched plan")


# ---- unpooled applies -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [4, 5])
def test_sgd_push_and_dedup(dev, width):
    fl, it, zeros_at = make_batch()
    table = make_table(ROWS, width)
    g = make_grads(N, width, zeros_at)
    want_sgd = cpu.sgd_sparse_update(table.copy(), _repf(fl), g, LR)
    _same(want_sgd[_untouched(fl)], table[_untouched(fl)])
    assert (want_sgd[0] != table[0]).all()
    u_rep, _, red_rep = cpu.dedup_reduce(_repf(fl), g)
    want_push = cpu.push_apply(table.copy(), u_rep, red_rep)
    uniq, _, want_red = cpu.dedup_reduce(fl, g)              # per key of the batch itself: its three dead keys are three runs
    assert uniq.size == np.unique(special_ids.keys_of(fl)).size
    d_g = _dev(g, dev)
    for name, ids in _forms(fl, it):
        d_ids = _dev(ids, dev)
        for finished in (False, True):
            t = _dev(table, dev)
            plan = ops.IndexPlan(N, dev).build(d_ids) if finished else ops.IndexPlan(N, dev).sort(d_ids)
            ops.sgd_apply(t, plan, d_g, LR, finished=finished)
            _same(t, want_sgd, "sgd_apply %s finished=%s" % (name, finished))
        t = _dev(table, dev)
        plan = ops.IndexPlan(N, dev).build(d_ids)
        ops.push_apply(t, plan, d_g)
        _same(t, want_push, "push_apply " + name)
        red = ops.dedup_reduce(plan, d_g)
        _same(red[:uniq.size], want_red, "dedup_reduce " + name)
        red2 = ops.dedup_reduce(plan, d_g, scale=-LR)
        _same(red2[:uniq.size], cpu.dedup_reduce(fl, cpu.scale_values(g, LR))[2], "dedup_reduce scaled " + name)
    t = _dev(table, dev)
    ops.sgd_sparse_update(t, _dev(fl, dev), d_g, LR)
    _same(t, want_sgd, "sgd_sparse_update")
    t = _dev(table, dev)
    ops.dl_call("SGDOptimizerSparseUpdate", [t, _dev(fl, dev), d_g], scalars=[ctypes.c_float(LR)])
    torch.cuda.synchronize()
    _same(t, want_sgd, "SGDOptimizerSparseUpdate")


@pytest.mark.parametrize("width", [4, 5])
def test_apply_finish_and_prefetch(dev, width):
    """lookup_sort + sgd_apply_finish, with the next batch's ids (specials among them) prefetched on the way out."""
    fl, it, zeros_at = make_batch()
    nxt = make_batch(seed=9)[0]
    table = make_table(ROWS, width)
    g = make_grads(N, width, zeros_at)
    want_out = cpu.embedding_lookup(table, _repf(fl))
    want_t = cpu.sgd_sparse_update(table.copy(), _repf(fl), g, LR)
    for name, ids in _forms(fl, it):
        for pf in (None, nxt):
            t = _dev(table, dev)
            plan = ops.IndexPlan(N, dev)
            out = ops.lookup_sort(t, _dev(ids, dev), plan)
            ops.sgd_apply_finish(t, plan, _dev(g, dev), LR, next_ids=None if pf is None else _dev(pf, dev))
            _same(out, want_out, "lookup_sort " + name)
            _same(t, want_t, "sgd_apply_finish " + name)
            _check_plan(plan, ids, "plan of lookup_sort + sgd_apply_finish " + name, export=False)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("width", [4, 5])
def test_tolerance_modes_leave_a_dead_run_of_70_alone(dev, width, mode):
    """Tolerance modes apply runs of 64 or more occurrences as a tree.  The dead run here has 70; every live key has fewer than
    64, so the expected table is the serial chain bit for bit: a dead run takes no tree and changes nothing."""
    n = 120
    fl, it, zeros_at = make_batch(n=n, extra_dead=50, seed=11)
    keys = special_ids.keys_of(fl)
    assert np.count_nonzero(keys == DEAD) == 70 and np.bincount(keys[keys < ROWS].astype(np.int64)).max() < 16
    table = make_table(ROWS, width)
    g = make_grads(n, width, zeros_at)
    bg = make_grads(n // BAG, width, seed=12)
    want = cpu.sgd_sparse_update(table.copy(), _repf(fl), g, LR)
    want_bags = bag_model.sgd_bags(table, _rep(fl).reshape(-1, BAG), bg, LR)
    prev = ops.set_tolerance_mode(mode)
    try:
        for name, ids in _forms(fl, it):
            for finished in (False, True):
                t = _dev(table, dev)
                plan = ops.IndexPlan(n, dev).build(_dev(ids, dev))
                ops.sgd_apply(t, plan, _dev(g, dev), LR, finished=finished)
                _same(t, want, "sgd_apply %s finished=%s" % (name, finished))
            t = _dev(table, dev)
            plan = ops.IndexPlan(n, dev).build(_dev(ids, dev))
            ops.sgd_apply_bags(t, plan, _dev(bg, dev), LR, bag=BAG)
            _same(t, want_bags, "sgd_apply_bags " + name)
            _same(t.cpu().numpy()[_untouched(fl)], table[_untouched(fl)])
    finally:
        ops.set_tolerance_mode(prev)


# ---- pooled applies ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ragged", [False, True], ids=["fixed", "ragged"])
@pytest.mark.parametrize("width", [4, 5])
def test_bag_applies(dev, width, ragged):
    fl, it, _ = make_batch()
    table = make_table(ROWS, width)
    off = RAGGED if ragged else None
    d_off = _dev(RAGGED, dev) if ragged else None
    nb = RAGGED.size - 1 if ragged else N // BAG
    bg, g_fm = make_grads(nb, width, seed=3), make_grads(nb, width, seed=4)
    w = (np.arange(N) % 3 != 1).astype(np.float32)
    w[np.arange(N) % 7 == 0] = 1.5
    rep = _rep(fl) if ragged else _rep(fl).reshape(-1, BAG)
    S = fm_model.fm_lookup(table, rep, off)[2]
    want_bags = bag_model.sgd_bags(table, rep, bg, LR, off)
    want_fm = fm_pooled_model.fm_pooled_sgd(table, rep, bg, g_fm, S, LR, off)
    want_fm0 = fm_pooled_model.fm_pooled_sgd(table, rep, None, g_fm, S, LR, off)
    want_w = wbag_model.wbag_sgd(table, rep, w, bg, LR, off)
    same = _untouched(fl)
    for want in (want_bags, want_fm, want_fm0, want_w):
        _same(want[same], table[same])
    d_bg, d_gfm, d_S, d_w = _dev(bg, dev), _dev(g_fm, dev), _dev(S, dev), _dev(w, dev)
    for name, ids in _forms(fl, it):
        d_ids = _dev(ids if ragged else ids.reshape(-1, BAG), dev)
        how = dict(bag_of=ops.bag_of(d_off, N)) if ragged else dict(bag=BAG)

        def plan():
            return ops.IndexPlan(N, dev).build(d_ids.reshape(-1))
        t = _dev(table, dev)
        ops.sgd_apply_bags(t, plan(), d_bg, LR, **how)
        _same(t, want_bags, "sgd_apply_bags " + name)
        t = _dev(table, dev)
        ops.sgd_sparse_update_bags(t, d_ids, d_bg, LR, offsets=d_off)
        _same(t, want_bags, "sgd_sparse_update_bags " + name)
        for g_sum, want in ((d_bg, want_fm), (None, want_fm0)):
            t = _dev(table, dev)
            ops.sgd_apply_fm_bags(t, plan(), g_sum, d_gfm, d_S, LR, **how)
            _same(t, want, "sgd_apply_fm_bags " + name)
            t = _dev(table, dev)
            ops.sgd_sparse_update_fm_bags(t, d_ids, g_sum, d_gfm, d_S, LR, offsets=d_off)
            _same(t, want, "sgd_sparse_update_fm_bags " + name)
        t = _dev(table, dev)
        ops.sgd_apply_wbags(t, plan(), d_bg, d_w, LR, **how)
        _same(t, want_w, "sgd_apply_wbags " + name)
        t = _dev(table, dev)
        ops.sgd_sparse_update_wbags(t, d_ids, d_bg, d_w, LR, offsets=d_off)
        _same(t, want_w, "sgd_sparse_update_wbags " + name)


@pytest.mark.parametrize("ragged", [False, True], ids=["fixed", "ragged"])
@pytest.mark.parametrize("width", [4, 5])
def test_hetu_ops_sgd_update_sparse_on_weighted_slices(dev, width, ragged):
    """hetu_ops.sgd_update_sparse on weighted pooled slices.  For ragged bags it builds the masked keys itself, on the host side
    of the library (torch), by the same rule: every special id carries a NON-ZERO weight here, so only the id rule can keep it
    out of row 0; float32 and int64 forms, with the offsets and with bag_of alone."""
    from herald_amd import hetu_ops
    fl, it, _ = make_batch()
    table = make_table(ROWS, width)
    off = RAGGED if ragged else None
    nb = RAGGED.size - 1 if ragged else N // BAG
    bg = make_grads(nb, width, seed=3)
    w = np.where(np.arange(N) % 5 == 2, 0.0, 1.0 + (np.arange(N) % 4) * 0.25).astype(np.float32)
    w[_dead(fl) | (special_ids.keys_of(fl) == 0)] = 1.5        # every dead id, and -0.0, -0.99 and the genuine zeros
    assert (w[_dead(fl)] != 0).all() and np.count_nonzero(w == 0) >= 5
    rep = _rep(fl) if ragged else _rep(fl).reshape(-1, BAG)
    want = wbag_model.wbag_sgd(table, rep, w, bg, LR, off)
    _same(want[_untouched(fl)], table[_untouched(fl)])
    assert (want[0] != table[0]).all()
    for name, ids in _forms(fl, it):
        for with_offsets in ((False, True) if ragged else (False,)):
            param = hetu_ops.EmbeddingParameter(table=_dev(table, dev))
            d_ids = _dev(ids if ragged else ids.reshape(-1, BAG), dev)
            if ragged:
                d_off = _dev(RAGGED, dev)
                grad = ops.IndexedSlices(indices=d_ids, values=_dev(bg, dev), dense_shape=(ROWS, width), bag_of=ops.bag_of(d_off, N),
                                         offsets=d_off if with_offsets else None, weights=_dev(w, dev))
            else:
                grad = ops.IndexedSlices(indices=d_ids, values=_dev(bg, dev), dense_shape=(ROWS, width), bag=BAG,
                                         weights=_dev(w.reshape(-1, BAG), dev))
            hetu_ops.sgd_update_sparse(param, grad, LR)
            torch.cuda.synchronize()
            _same(param.table, want, "sgd_update_sparse %s offsets=%s" % (name, with_offsets))


# ---- optimizers -------------------------------------------------------------------------------------------------------
HYPER =dict(lr=0.05, eps=1e-2, beta1=0.9, beta2=0.999, beta1t=0.9 ** 2, beta2t=0.999 ** 2, weight_decay=0.1)


def _states(width, seed=21):
    rng = np.random.default_rng(seed)
    param = make_table(ROWS, width)
    s1 = (rng.standard_normal((ROWS, width)).astype(np.float32)) ** 2
    s2 = (rng.standard_normal((ROWS, width)).astype(np.float32)) ** 2
    return param, s1, s2


def _numpy_opt(kind, param, s1, s2, ids_f32, grads):
    """grad.deduplicate() + the optimizer, oracle/cpu.py, on the ids that name a row."""
    uniq, _, red = cpu.dedup_reduce(ids_f32, grads)
    live = uniq < ROWS
    p, a, b = param.copy(), s1.copy(), s2.copy()
    if kind == "adagrad":
        cpu.adagrad_sparse(p, a, uniq[live], red[live], HYPER["lr"], HYPER["eps"])
    else:
        cpu.adam_sparse(p, a, b, uniq[live], red[live], HYPER["lr"], HYPER["beta1"], HYPER["beta2"], np.float32(HYPER["beta1t"]),
                        np.float32(HYPER["beta2t"]), HYPER["eps"], HYPER["weight_decay"] if kind == "adamw" else None)
    return p, a, b


def _check_twin(got, twin, start, same, what):
    """got: the arrays after the call on the batch; twin: after the call on the replaced batch; start: before."""
    for x, y, z in zip(got, twin, start):
        _same(x, y.cpu().numpy(), what + ": the batch and the batch with rows + 1 for every dead id")
        if same is not None:
            _same(x.cpu().numpy()[same], z[same], what + ": rows no live id names")


@pytest.mark.parametrize("kind", ["adagrad", "adam", "adamw"])
@pytest.mark.parametrize("width", [4, 5])
def test_fused_optimizers(dev, width, kind):
    fl, it, zeros_at = make_batch()
    param, s1, s2 = _states(width)
    g = make_grads(N, width, zeros_at)
    bg = make_grads(N // BAG, width, seed=5)
    bg_ragged = make_grads(RAGGED.size - 1, width, seed=6)
    same = _untouched(fl)

    def run(ids, pooled, offsets=None):
        p, a, b = _dev(param, dev), _dev(s1, dev), _dev(s2, dev)
        if pooled:
            ops.sparse_opt_fused_bags(kind, p, _dev(ids if offsets is not None else ids.reshape(-1, BAG), dev),
                                      _dev(bg if offsets is None else bg_ragged, dev), a,
                                      None if kind == "adagrad" else b, offsets=offsets, **HYPER)
        else:
            ops.sparse_opt_fused(kind, p, _dev(ids, dev), _dev(g, dev), a, None if kind == "adagrad" else b, **HYPER)
        torch.cuda.synchronize()
        return p, a, b
    twin = run(_repf(fl), False)
    for x, y in zip(twin, _numpy_opt(kind, param, s1, s2, _repf(fl), g)):
        np.testing.assert_allclose(x.cpu().numpy(), y, **OPT_TOL)
    assert (twin[0].cpu().numpy()[0] != param[0]).all()
    for name, ids in _forms(fl, it):
        _check_twin(run(ids, False), twin, (param, s1, s2), same, "sparse_opt_fused " + name)
    twin = run(_repf(fl), True)
    for x, y in zip(twin, _numpy_opt(kind, param, s1, s2, _repf(fl), np.repeat(bg, BAG, axis=0))):
        np.testing.assert_allclose(x.cpu().numpy(), y, **OPT_TOL)
    for name, ids in _forms(fl, it):
        _check_twin(run(ids, True), twin, (param, s1, s2), same, "sparse_opt_fused_bags " + name)
    d_off = _dev(RAGGED, dev)
    twin = run(_repf(fl), True, d_off)
    for name, ids in _forms(fl, it):
        _check_twin(run(ids, True, d_off), twin, (param, s1, s2), same, "sparse_opt_fused_bags ragged " + name)


@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("width", [4, 5])
def test_momentum(dev, width, nesterov):
    """The first phase is the serial chain per occurrence, the second one dense: bit for bit oracle/cpu.py's restatement but for
    the dense phase's product, so the yardstick is the replaced batch (and numpy within 1e-5)."""
    fl, it, zeros_at = make_batch()
    param, vel, _ = _states(width)
    vel = (vel * np.float32(0.1)).astype(np.float32)
    g = make_grads(N, width, zeros_at)
    bg = make_grads(N // BAG, width, seed=5)

    def run(ids, pooled):
        p, v = _dev(param, dev), _dev(vel, dev)
        if pooled:
            ops.momentum_sparse_update_bags(p, _dev(ids.reshape(-1, BAG), dev), _dev(bg, dev), v, 0.01, 0.9, nesterov)
        else:
            ops.dl_call("MomentumOptimizerSparseUpdate", [p, _dev(ids, dev), _dev(g, dev), v],
                        scalars=[ctypes.c_float(0.01), ctypes.c_float(0.9), ctypes.c_bool(nesterov)])
        torch.cuda.synchronize()
        return p, v
    for pooled in (False, True):
        twin = run(_repf(fl), pooled)
        mp, mv = param.copy(), vel.copy()
        live = ~_dead(fl)
        grads = np.repeat(bg, BAG, axis=0) if pooled else g
        cpu.momentum_sparse(mp, mv, special_ids.rows_of(fl)[live], grads[live], 0.01, 0.9, nesterov)
        np.testing.assert_allclose(twin[0].cpu().numpy(), mp, **OPT_TOL)
        np.testing.assert_allclose(twin[1].cpu().numpy(), mv, **OPT_TOL)
        _check_twin(run(fl, pooled), twin, (param, vel), None, "momentum f32 pooled=%s" % pooled)
        if pooled:
            _check_twin(run(it, pooled), twin, (param, vel), None, "momentum i64 pooled")


@pytest.mark.parametrize("op", ["adagrad", "adam", "adamw", "lamb", "l2"])
@pytest.mark.parametrize("width", [4, 5])
def test_dl_named_optimizers(dev, width, op):
    """The reference-named sparse updates on deduplicated slices (csrc/optim.hip, sparse_row_kernel): every live id once (0 as
    -0.0, rows - 1 as rows - 0.5), every dead id of the list twice."""
    rng = np.random.default_rng(31)
    f = np.float32
    dead_ids = np.array([p[0] for p in pairs(ROWS) if special_ids.keys_of(np.array([p[0]]))[0] >= ROWS], dtype=f)
    ids = np.concatenate([rng.permutation(np.arange(1, ROWS - 1))[:20].astype(f), f([-0.0, ROWS - 0.5]), dead_ids, dead_ids])
    ids = ids[rng.permutation(ids.size)]
    n = ids.size
    g = make_grads(n, width, np.flatnonzero(special_ids.keys_of(ids) == 0))
    param, s1, s2 = _states(width)
    same = _untouched(ids)
    sc = [ctypes.c_float(x) for x in (HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["beta1t"], HYPER["beta2t"], HYPER["eps"])]
    wd = [ctypes.c_float(HYPER["weight_decay"])]

    def run(batch):
        p, a, b, d_g = _dev(param, dev), _dev(s1, dev), _dev(s2, dev), _dev(g, dev)
        d_ids = _dev(batch, dev)
        if op == "adagrad":
            ops.dl_call("AdaGradOptimizerSparseUpdate", [p, d_ids, d_g, a], scalars=[ctypes.c_float(HYPER["lr"]), ctypes.c_float(HYPER["eps"])])
        elif op == "adam":
            ops.dl_call("AdamOptimizerSparseUpdate", [p, d_ids, d_g, a, b], scalars=sc)
        elif op == "adamw":
            ops.dl_call("AdamWOptimizerSparseUpdate", [p, d_ids, d_g, a, b], scalars=sc + wd)
        elif op == "lamb":
            ops.dl_call("LambOptimizerSparseUpdate", [p, d_ids, d_g, a, b], scalars=sc + wd)
        else:
            ops.dl_call("AddL2RegularizationSparse", [p, d_ids, d_g], scalars=[ctypes.c_float(0.3)])
        torch.cuda.synchronize()
        return p, a, b, d_g
    twin = run(_repf(ids))
    got = run(ids)
    for x, y in zip(got, twin):
        _same(x, y.cpu().numpy(), op + ": the batch and the batch with rows + 1 for every dead id")
    for x, z in zip(got[:3], (param, s1, s2)):
        _same(x.cpu().numpy()[same], z[same], op + ": rows no live id names")
    dead = _dead(ids)
    _same(got[3].cpu().numpy()[dead], g[dead], op + ": gradient rows of dead ids")
    live = ~dead
    key = special_ids.rows_of(ids)[live]
    p, a, b = param.copy(), s1.copy(), s2.copy()
    b1t, b2t = np.float32(HYPER["beta1t"]), np.float32(HYPER["beta2t"])
    if op == "adagrad":
        cpu.adagrad_sparse(p, a, key, g[live], HYPER["lr"], HYPER["eps"])
    elif op == "lamb":
        cpu.lamb_sparse(p, a, b, key, g[live], HYPER["lr"], HYPER["beta1"], HYPER["beta2"], b1t, b2t, HYPER["eps"], HYPER["weight_decay"])
    elif op == "l2":
        np.testing.assert_allclose(got[3].cpu().numpy()[live], cpu.l2_sparse(param, key, g[live], 0.3), rtol=1e-6, atol=1e-6)
    else:
        cpu.adam_sparse(p, a, b, key, g[live], HYPER["lr"], HYPER["beta1"], HYPER["beta2"], b1t, b2t, HYPER["eps"],
                        HYPER["weight_decay"] if op == "adamw" else None)
    for x, y in zip(got[:3], (p, a, b)):
        np.testing.assert_allclose(x.cpu().numpy(), y, **OPT_TOL)
    if op != "l2":
        assert (got[0].cpu().numpy()[0] != param[0]).all()


# ---- libps names at one rank ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [4, 5])
def test_libps_names(dev, width):
    from herald_amd import ps
    P = ps.lib()
    node = 9100 + width
    lrs = (ctypes.c_float * 1)(0.1)
    P.InitTensor(node, 2, ROWS, width, 0, 0.5, 0.0, 7, 0, lrs, 1)
    P.Wait(node)
    shard, info = ps.tensor(node, dev)
    assert (info.len, info.width) == (ROWS, width)
    table = make_table(ROWS, width)
    shard.copy_(_dev(table, dev))
    torch.cuda.synchronize()
    fl, _, zeros_at = make_batch()
    nxt = make_batch(seed=9)[0]
    vals = make_grads(N, width, zeros_at)
    try:
        d_ids = _dev(fl, dev)
        out = torch.full((N, width), 7.0, dtype=torch.float32, device=dev)
        hi, ho = ops.DLHolder(d_ids), ops.DLHolder(out)
        P.SparsePull(node, hi.handle, ho.handle)
        P.Wait(node)
        _same(out, cpu.sparse_pull(table, _repf(fl)), "SparsePull")
        assert not out.cpu().numpy()[_dead(fl)].view(np.uint32).any()
        hv = ops.DLHolder(_dev(vals, dev))
        P.SparsePush(node, hi.handle, hv.handle, None)
        P.Wait(node)
        want = cpu.sparse_push(table.copy(), _repf(fl), vals)
        _same(shard, want, "SparsePush")
        _same(want[_untouched(fl)], table[_untouched(fl)])
        out2 = np.empty((N, width), dtype=np.float32)
        hs = [ops.DLHolder(torch.from_numpy(x)) for x in (fl, vals, nxt, out2)]
        P.SSPushPull(node, hs[0].handle, hs[1].handle, hs[2].handle, hs[3].handle, None)
        P.Wait(node)
        cpu.sparse_push(want, _repf(fl), vals)
        _same(shard, want, "SSPushPull: the push")
        _same(out2, cpu.sparse_pull(want, _repf(nxt)), "SSPushPull: the pull")
    finally:
        P.Clear(node)


# ---- step engines -----------------------------------------------------------------------------------------------------
def _stream(rows, width, n, steps=3, wide=False):
    """`steps` batches for a step engine: no live key has 16 or more occurrences (the work-queue step is then the serial chain
    bit for bit), the dead run of every batch is longer than 16."""
    batches = []
    for k in range(steps):
        ordinary = None
        if wide:        # every key of [1, rows) about seven times
            ordinary = 1 + np.random.default_rng(40 + k).permutation(n) % (rows - 1)
        fl, it, zeros_at = make_batch(rows=rows, n=n, seed=50 + k, extra_dead=4, ordinary=ordinary)
        keys = special_ids.keys_of(fl)
        assert np.bincount(keys[keys < rows].astype(np.int64)).max() < 16 and np.count_nonzero(keys == DEAD) > 16
        batches.append((fl, it, make_grads(n, width, zeros_at, seed=60 + k)))
    return batches


def _lookup_model(t, ids):
    return cpu.embedding_lookup(t, _repf(ids, t.shape[0]))


def _drive(dev, rows, width, n, start, step, form, wide=False):
    """start(d_ids list) -> rows of batch 0; step(k, grads, d_ids list) -> rows of batch k + 1 or None; -> the table tensor."""
    batches = _stream(rows, width, n, wide=wide)
    table = make_table(rows, width)
    model = table.copy()
    t = _dev(table, dev)
    d_ids = [_dev(b[0] if form == "f32" else b[1], dev) for b in batches]
    out = start(t, d_ids)
    never = np.ones(rows, dtype=bool)
    for k, (fl, it, g) in enumerate(batches):
        torch.cuda.synchronize()
        _same(out, _lookup_model(model, fl), "rows of batch %d" % k)
        assert not out.cpu().numpy().reshape(n, width)[_dead(fl, rows)].view(np.uint32).any()
        cpu.sgd_sparse_update(model, _repf(fl, rows), g, LR)
        never &= _untouched(fl, rows)
        out = step(k, _dev(g, dev), d_ids)
        torch.cuda.synchronize()
        _same(t, model, "table after step %d" % k)
    assert out is None
    _same(t.cpu().numpy()[never], table[never], "rows no live id names")
    assert (model[0] != table[0]).all()
    return t


@pytest.mark.parametrize("form", ["f32", "i64"])
@pytest.mark.parametrize("width", [4, 5])
def test_push_pull(dev, width, form):
    """ops.sgd_push_pull: the one-launch step (width 4), the separate launches it falls back to (width 5)."""
    plans = [ops.IndexPlan(64, dev), ops.IndexPlan(64, dev)]
    pends = [ops.PendingTable(dev), ops.PendingTable(dev)]
    state = {}

    def start(t, d_ids):
        state["t"] = t
        return ops.lookup_sort_pend(t, d_ids[0], plans[0], pends[0])

    def step(k, g, d_ids):
        if k + 1 < len(d_ids):
            out = ops.sgd_push_pull(state["t"], plans[k % 2], g, LR, pends[k % 2], d_ids[k + 1], plans[(k + 1) % 2], pends[(k + 1) % 2])
            torch.cuda.synchronize()
            assert not plans[(k + 1) % 2].handoff_timed_out()
            return out
        return ops.sgd_push_pull(state["t"], plans[k % 2], g, LR, pends[k % 2])
    _drive(dev, ROWS, width, 64, start, step, form)
    assert pends[0].is_idle() and pends[1].is_idle()


@pytest.mark.parametrize("form", ["f32", "i64"])
def test_step_pipeline(dev, form):
    state = {}

    def start(t, d_ids):
        state["p"] = ops.StepPipeline(t, 64, LR)
        return state["p"].start(d_ids[0], d_ids[1], d_ids[2])

    def step(k, g, d_ids):
        return state["p"].step(g, None)
    _drive(dev, ROWS, 4, 64, start, step, form)


@pytest.mark.parametrize("form", ["f32", "i64"])
def test_queue_step_pipeline(dev, form):
    state = {}

    def start(t, d_ids):
        state["p"] = ops.QueueStepPipeline(t, 64, LR, block=1, overlap=False)
        assert not state["p"].wide and state["p"].LOOKAHEAD == 3
        return state["p"].start(d_ids[:3])

    def step(k, g, d_ids):
        return state["p"].step(g, None)
    _drive(dev, ROWS, 4, 64, start, step, form)
    assert not state["p"].overflowed()


def test_queue_step_pipeline_wide(dev):
    """The wide path (hash buckets of the batch planned side by side) at its smallest size."""
    n = ops.qstep_max_ids() + 1
    state = {}

    def start(t, d_ids):
        state["p"] = ops.QueueStepPipeline(t, n, LR, block=1, overlap=False)
        assert state["p"].wide
        return state["p"].start(d_ids[:3])

    def step(k, g, d_ids):
        return state["p"].step(g, None)
    _drive(dev, 1021, 4, n, start, step, "f32", wide=True)
    assert not state["p"].overflowed() and state["p"].fallbacks == 0


def test_sort_ahead_pipeline(dev):
    state = {}

    def start(t, d_ids):
        state["p"] = ops.SortAheadPipeline(t, 64, LR, block=2)
        state["p"].prepare_block(d_ids[0:2])
        return state["p"].lookup(0, d_ids[0])

    def step(k, g, d_ids):
        if k == 0:
            state["p"].prepare_block(d_ids[2:3])
        state["p"].apply(k, g)
        return state["p"].lookup(k + 1, d_ids[k + 1]) if k + 1 < len(d_ids) else None
    _drive(dev, ROWS, 4, 64, start, step, "f32")

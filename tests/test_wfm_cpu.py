"""CPU-side checks of the weighted FM-pooled lookup (the second-order term of the FAE DeepFM): the six new calls are declared,
exported and bound; their arguments are validated before any device access; the numpy restatement the GPU tests are held to
(tests/wfm_model.py) agrees with the restatements it builds on -- S is wbag_model.wbag_sum, all-ones weights give
fm_model.fm_lookup's S and FM output, a 0/1 mask equals all ones on the compacted ragged bags, the fused apply is gather +
wfm_grad_rows + the unpooled serial apply -- and with float64 autograd of the reference's own graph; and IndexedSlices' rules for
sq_grad."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fm_model  # noqa: E402
import wbag_model  # noqa: E402
import wfm_model  # noqa: E402

from herald_amd import _lib  # noqa: E402

FORWARD = ["ha_gather_wfm_f32ids", "ha_gather_wfm_u64ids"]
ONE_CALL = ["ha_sgd_sparse_update_wfm_bags_f32ids", "ha_sgd_sparse_update_wfm_bags_u64ids"]
SYMBOLS = FORWARD + ["ha_wfm_grad_rows", "ha_sgd_apply_wfm_bags"] + ONE_CALL


def test_wfm_symbols_are_declared_exported_and_bound(lib):
    declared = _lib.declared_symbols()
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.ha_gather_wfm_f32ids.argtypes) == len(lib.ha_gather_wfm_u64ids.argtypes) == 12
    assert len(lib.ha_wfm_grad_rows.argtypes) == 11
    assert len(lib.ha_sgd_apply_wfm_bags.argtypes) == 13
    assert len(lib.ha_sgd_sparse_update_wfm_bags_f32ids.argtypes) == len(lib.ha_sgd_sparse_update_wfm_bags_u64ids.argtypes) == 13


def test_nothing_in_the_package_imports_the_restatement():
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "herald_amd")
    for name in os.listdir(pkg):
        if name.endswith(".py"):
            with open(os.path.join(pkg, name)) as fh:
                assert "wfm_model" not in fh.read(), name


# non-null addresses that are never dereferenced: validation comes before any device access (there is no GPU here)
P = ctypes.c_void_p(0x1000)
Q = [ctypes.c_void_p(0x2000 + 0x1000 * i) for i in range(5)]
BIG = 1 << 31

COMMON = [
    ("neither bag nor offsets", dict(bag=0, ragged=None)),
    ("both bag and offsets", dict(bag=2, ragged=P)),
    ("n not a multiple of bag", dict(n=7, bag=2, nbags=3)),
    ("n / bag is not nbags", dict(n=8, bag=2, nbags=3)),
    ("n of 2^31", dict(n=BIG, bag=2, nbags=BIG // 2)),
    ("width 0", dict(width=0)),
    ("negative width", dict(width=-4)),
    ("width of 2^30", dict(width=1 << 30)),
    ("negative n", dict(n=-1)),
    ("ragged occurrences in no bag", dict(bag=0, ragged=P, nbags=0)),
    ("null weights", dict(weights=None)),
]


@pytest.mark.parametrize("fn", FORWARD)
@pytest.mark.parametrize("case,args", COMMON + [("null table", dict(table=None)), ("null ids", dict(ids=None)),
                                                ("null out_sum", dict(out_sum=None)), ("null out_sq", dict(out_sq=None)),
                                                ("out_sq is out_sum", dict(out_sq=Q[2]))])
def test_forward_rejects_bad_arguments_before_any_device_access(lib, fn, case, args):
    a = dict(table=Q[0], rows=10, width=4, ids=P, weights=Q[1], n=8, bag=2, ragged=None, nbags=4, out_sum=Q[2], out_sq=Q[3])
    a.update(args)
    rc = getattr(lib, fn)(a["table"], a["rows"], a["width"], a["ids"], a["weights"], a["n"], a["bag"], a["ragged"], a["nbags"],
                          a["out_sum"], a["out_sq"], None)
    assert rc == -1, case
    assert fn.encode() in lib.ha_last_error(), (case, lib.ha_last_error())


@pytest.mark.parametrize("case,args", COMMON + [("null g_sum", dict(gs=None)), ("null g_sq", dict(gq=None)),
                                                ("null emb_rows", dict(e=None)), ("null out", dict(out=None)),
                                                ("out is g_sum", dict(out=Q[0])), ("out is g_sq", dict(out=Q[1])),
                                                ("out is weights", dict(out=Q[2])),
                                                ("out overlaps emb_rows", dict(out=ctypes.c_void_p(0x5000 + 16)))])
def test_grad_rows_rejects_bad_arguments_before_any_device_access(lib, case, args):
    a = dict(gs=Q[0], gq=Q[1], weights=Q[2], e=Q[3], n=8, width=4, bag=2, ragged=None, nbags=4, out=Q[4])
    a.update(args)
    rc = lib.ha_wfm_grad_rows(a["gs"], a["gq"], a["weights"], a["e"], a["n"], a["width"], a["bag"], a["ragged"], a["nbags"],
                              a["out"], None)
    assert rc == -1, case
    assert b"ha_wfm_grad_rows" in lib.ha_last_error(), (case, lib.ha_last_error())


APPLY = [("null table", dict(table=None)), ("null g_sum", dict(gs=None)), ("null g_sq", dict(gq=None)),
         ("g_sum aliases the table", dict(gs=Q[0])), ("g_sq aliases the table", dict(gq=Q[0])),
         ("weights alias the table", dict(weights=Q[0])),
         ("g_sq lies inside the table", dict(gq=ctypes.c_void_p(0x2000 + 64)))]


@pytest.mark.parametrize("case,args", COMMON + APPLY + [("null plan_ws", dict(plan_ws=None))])
def test_apply_rejects_bad_arguments_before_any_device_access(lib, case, args):
    a = dict(table=Q[0], rows=10, width=4, plan_ws=P, n=8, gs=Q[1], gq=Q[2], weights=Q[3], bag=2, ragged=None, nbags=4)
    a.update(args)
    rc = lib.ha_sgd_apply_wfm_bags(a["table"], a["rows"], a["width"], a["plan_ws"], a["n"], a["gs"], a["gq"], a["weights"],
                                   a["bag"], a["ragged"], a["nbags"], 0.1, None)
    assert rc == -1, case
    assert b"ha_sgd_apply_wfm_bags" in lib.ha_last_error(), (case, lib.ha_last_error())


@pytest.mark.parametrize("fn", ONE_CALL)
@pytest.mark.parametrize("case,args", COMMON + APPLY + [("null ids", dict(ids=None)), ("rows beyond 32-bit keys", dict(rows=1 << 32))])
def test_one_call_forms_reject_bad_arguments_before_any_device_access(lib, fn, case, args):
    a = dict(table=Q[0], rows=10, width=4, ids=P, weights=Q[3], n=8, gs=Q[1], gq=Q[2], bag=2, ragged=None, nbags=4)
    a.update(args)
    rc = getattr(lib, fn)(a["table"], a["rows"], a["width"], a["ids"], a["weights"], a["n"], a["gs"], a["gq"], a["bag"],
                          a["ragged"], a["nbags"], 0.1, None)
    assert rc == -1, case
    assert fn.encode() in lib.ha_last_error(), (case, lib.ha_last_error())


def test_no_ids_is_not_an_error(lib):
    for fn in FORWARD:
        assert getattr(lib, fn)(None, 10, 4, None, None, 0, 2, None, 0, None, None, None) == 0
        assert getattr(lib, fn)(None, 10, 4, None, None, 0, 0, P, 3, None, None, None) == 0       # ragged, every bag empty
    assert lib.ha_wfm_grad_rows(None, None, None, None, 0, 4, 2, None, 0, None, None) == 0
    assert lib.ha_wfm_grad_rows(None, None, None, None, 0, 4, 0, P, 3, None, None) == 0
    assert lib.ha_sgd_apply_wfm_bags(None, 10, 4, None, 0, None, None, None, 2, None, 0, 0.1, None) == 0
    assert lib.ha_sgd_apply_wfm_bags(None, 10, 4, None, 0, None, None, None, 0, P, 3, 0.1, None) == 0
    for fn in ONE_CALL:
        assert getattr(lib, fn)(None, 10, 4, None, None, 0, None, None, 2, None, 0, 0.1, None) == 0
        assert getattr(lib, fn)(None, 10, 4, None, None, 0, None, None, 0, P, 3, 0.1, None) == 0


# ---- the restatement against the restatements it builds on --------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _inputs(rows, width, B, seed):
    rng = np.random.default_rng(seed)
    table = (rng.standard_normal((rows, width)) * np.exp(rng.uniform(-4, 4, (rows, 1)))).astype(np.float32)
    gs = (rng.standard_normal((B, width)) * np.exp(rng.uniform(-3, 3, (B, 1)))).astype(np.float32)
    gq = (rng.standard_normal((B, width)) * np.exp(rng.uniform(-3, 3, (B, 1)))).astype(np.float32)
    return rng, table, gs, gq


def _fixed(rng, rows, B, F):
    ids = rng.integers(0, rows, (B, F)).astype(np.float32)
    ids[:, 0] = 3                                     # one key in every bag
    ids[2, 1] = ids[2, 2] = 9                         # a duplicate inside a bag
    ids[5, 3], ids[B - 1, F - 1] = rows, rows + 7     # ids >= rows
    return ids


RAGGED = np.array([0, 0, 10, 37, 37, 37, 102, 120, 120], dtype=np.int64)


def _case(ragged, seed):
    rows, width = 40, 7
    if ragged:
        rng, table, gs, gq = _inputs(rows, width, RAGGED.size - 1, seed)
        return rng, table, gs, gq, rng.integers(0, rows + 2, 120).astype(np.float32), RAGGED
    rng, table, gs, gq = _inputs(rows, width, 33, seed)
    return rng, table, gs, gq, _fixed(rng, rows, 33, 6), None


def _general_weights(rng, ids):
    w = rng.standard_normal(ids.shape).astype(np.float32)
    flat = w.reshape(-1)
    flat[::7] = np.float32(0.0)
    flat[3::11] = np.float32(-0.0)
    return w


@pytest.mark.parametrize("ragged", [False, True])
def test_the_sum_is_the_weighted_bag_sum_for_any_weights(ragged):
    rng, table, _, _, ids, off = _case(ragged, 31)
    w = _general_weights(rng, ids)
    S, Q = wfm_model.wfm_lookup(table, ids, w, off)
    assert np.array_equal(_bits(S), _bits(wbag_model.wbag_sum(table, ids, w, off)))
    assert (Q >= 0).all() and (Q > 0).any()


@pytest.mark.parametrize("ragged", [False, True])
def test_all_ones_weights_are_the_fm_lookup_bit_for_bit(ragged):
    rng, table, _, _, ids, off = _case(ragged, 32)
    S, Q = wfm_model.wfm_lookup(table, ids, np.ones(ids.size, np.float32), off)
    _, _, want_S, want_fm = fm_model.fm_lookup(table, ids, off)
    fm = (np.float32(0.5) * ((S * S).astype(np.float32) - Q).astype(np.float32)).astype(np.float32)
    assert np.array_equal(_bits(S), _bits(want_S)) and np.array_equal(_bits(fm), _bits(want_fm))
    assert np.count_nonzero(fm) >= fm.size // 2      # (half of the ragged bags are empty)


@pytest.mark.parametrize("ragged", [False, True])
def test_a_mask_is_all_ones_on_the_compacted_ragged_bags(ragged):
    rng, table, gs, gq, ids, off = _case(ragged, 33)
    w = (rng.random(ids.size) < 0.6).astype(np.float32)
    if not ragged:
        w.reshape(ids.shape)[:, 0] = 0                # the padding column
        w.reshape(ids.shape)[7, :] = 0                # a bag with no live occurrence
    w[np.flatnonzero(w == 0)[::2]] = np.float32(-0.0)
    cids, coff = wbag_model.compact(ids, w, off)
    assert 0 < cids.size < ids.size
    ones = np.ones(cids.size, np.float32)
    S, Q = wfm_model.wfm_lookup(table, ids, w, off)
    cS, cQ = wfm_model.wfm_lookup(table, cids, ones, coff)
    assert np.array_equal(_bits(S), _bits(cS)) and np.array_equal(_bits(Q), _bits(cQ))
    got = wfm_model.wfm_sgd(table, ids, w, gs, gq, 0.05, off)
    assert np.array_equal(_bits(got), _bits(wfm_model.wfm_sgd(table, cids, ones, gs, gq, 0.05, coff)))
    assert not np.array_equal(_bits(got), _bits(table))


@pytest.mark.parametrize("ragged", [False, True])
def test_the_fused_apply_is_gather_gradient_and_the_unpooled_apply(ragged):
    rng, table, gs, gq, ids, off = _case(ragged, 34)
    w = _general_weights(rng, ids)
    assert not np.signbit(table[table == 0]).any()
    which = wbag_model.which_bag(ids, off)
    G = wfm_model.wfm_grad_rows(gs, gq, w, wfm_model.gather(table, ids), which)
    assert np.array_equal(_bits(G[w.reshape(-1) == 0]), np.zeros_like(_bits(G[w.reshape(-1) == 0])))
    got = wfm_model.wfm_sgd(table, ids, w, gs, gq, 0.05, off)
    assert np.array_equal(_bits(got), _bits(wbag_model.sgd_rows(table, ids, G, 0.05)))
    assert not np.array_equal(_bits(got), _bits(table))


def test_every_gradient_of_a_key_is_formed_from_the_row_before_the_call():
    """One key twice, g_S = 0, g_Q = 1, w = 1: g = 2 e for both occurrences from e = 1, so 1 - 0.5 - 0.5 = 0; a chain that formed
    the second gradient from the updated row would give 1 - 0.5 - 0.25."""
    one = np.ones((1, 1), np.float32)
    got = wfm_model.wfm_sgd(one, np.zeros((1, 2), np.float32), np.ones((1, 2), np.float32), 0 * one, one, 0.25)
    assert got[0, 0] == 0.0


def test_a_dead_occurrence_under_inf_rows_or_inf_gradients_leaves_no_trace():
    rows, width, lr = 12, 5, 0.1
    rng, table, gs, gq = _inputs(rows, width, 4, 35)
    ids = rng.integers(1, rows, (4, 3)).astype(np.float32)
    w = rng.standard_normal((4, 3)).astype(np.float32)
    ids[:, 0], w[:, 0] = 0, 0                          # the padding id, dead, in every bag
    w[2, :] = [0.0, -0.0, 0.0]                         # bag 2: no live occurrence at all
    table[0] = np.inf
    gs[2] = [np.inf, -np.inf, np.nan, np.inf, np.nan]
    gq[2] = [np.nan, np.inf, np.inf, -np.inf, np.nan]
    S, Q = wfm_model.wfm_lookup(table, ids, w)
    assert np.isfinite(S).all() and np.isfinite(Q).all()
    assert np.array_equal(_bits(S[2]), np.zeros(width, np.int32)) and np.array_equal(_bits(Q[2]), np.zeros(width, np.int32))
    G = wfm_model.wfm_grad_rows(gs, gq, w, wfm_model.gather(table, ids), wbag_model.which_bag(ids))
    assert np.isfinite(G).all() and np.array_equal(_bits(G[6:9]), np.zeros((3, width), np.int32))
    got = wfm_model.wfm_sgd(table, ids, w, gs, gq, lr)
    assert np.isfinite(got[1:]).all() and np.array_equal(_bits(got[0]), _bits(table[0]))
    only_dead = np.setdiff1d(ids[2].astype(np.int64), ids[[0, 1, 3], 1:].astype(np.int64))
    for k in only_dead:
        assert np.array_equal(_bits(got[k]), _bits(table[k]))


def test_the_sign_of_a_zero_is_the_one_corner_where_fused_and_composed_differ():
    table = np.array([[-0.0], [1.0]], dtype=np.float32)
    ids, w = np.array([[0.0, 1.0]], np.float32), np.array([[0.0, 1.0]], np.float32)
    gs, gq = np.array([[2.0]], np.float32), np.array([[0.5]], np.float32)
    G = wfm_model.wfm_grad_rows(gs, gq, w, wfm_model.gather(table, ids), wbag_model.which_bag(ids))
    assert G[1, 0] == 3.0                              # 1 * (2 + 2 * 0.5 * (1 * 1))
    fused = wfm_model.wfm_sgd(table, ids, w, gs, gq, -0.5)
    comp = wbag_model.sgd_rows(table, ids, G, -0.5)
    assert np.signbit(fused[0, 0]) and not np.signbit(comp[0, 0]) and fused[1, 0] == comp[1, 0] == 2.5
    assert np.array_equal(_bits(wfm_model.wfm_sgd(table, ids, w, gs, gq, 0.5)), _bits(wbag_model.sgd_rows(table, ids, G, 0.5)))


def test_the_gradient_is_float64_autograd_of_the_reference_graph_within_the_derived_bound():
    """x = w * e, S = sum over the bag of x, Q = sum of x * x, loss linear in S and Q, in float64 autograd.  Magnitudes in
    [2^-4, 2^4] (nothing underflows or overflows) plus exact zero weights.  Bound per element: four roundings at 2^-24 relative,
    two on each term's path -- fl(w * e) and fl(g_Q * x) on the second-order term (the doubling is exact), the sum and the final
    product on both -- with one more unit for the second-order terms: 5 * 2^-24 * |w| * (|g_S| + 2 * |g_Q * w * e|)."""
    import torch
    rng = np.random.default_rng(36)
    B, F, width = 9, 5, 6

    def mags(shape):
        return (np.exp2(rng.uniform(-4, 4, shape)) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)

    w, e, gs, gq = mags((B, F)), mags((B * F, width)), mags((B, width)), mags((B, width))
    w.reshape(-1)[::4] = 0
    got = wfm_model.wfm_grad_rows(gs, gq, w, e, np.arange(B * F) // F)
    te = torch.from_numpy(e.astype(np.float64)).requires_grad_(True)
    tw = torch.from_numpy(w.astype(np.float64)).reshape(B, F, 1)
    x = tw * te.reshape(B, F, width)
    S, Qs = x.sum(1), (x * x).sum(1)
    ((torch.from_numpy(gs.astype(np.float64)) * S).sum() + (torch.from_numpy(gq.astype(np.float64)) * Qs).sum()).backward()
    want = te.grad.numpy()
    w64 = np.abs(w.astype(np.float64)).reshape(-1, 1)
    second = np.abs(np.repeat(gq.astype(np.float64), F, axis=0) * w64 * e.astype(np.float64))
    bound = 5 * 2.0 ** -24 * w64 * (np.abs(np.repeat(gs.astype(np.float64), F, axis=0)) + 2 * second)
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    assert (got[w.reshape(-1) == 0] == 0).all() and (want[w.reshape(-1) == 0] == 0).all()
    assert np.count_nonzero(err) > err.size // 4      # (the comparison is not vacuous: float32 rounding shows)


# ---- IndexedSlices -----------------------------------------------------------------------------------------------------------
def test_indexed_slices_sq_grad_rules():
    import torch
    from herald_amd import hetu_ops, ops
    idx, g, q, w = torch.zeros((2, 3)), torch.ones((2, 4)), torch.ones((2, 4)), torch.ones((2, 3))
    sl = ops.IndexedSlices(indices=idx, values=g, dense_shape=(10, 4), bag=3, weights=w, sq_grad=q)
    assert sl.weighted_fm and sl.weighted and sl.pooled and not sl.fm_pooled and sl.sq_grad is q
    assert ops.IndexedSlices(indices=idx, values=g, dense_shape=(10, 4), bag_of=torch.zeros(6, dtype=torch.int32), weights=w,
                             sq_grad=q).weighted_fm
    assert not ops.IndexedSlices(indices=idx, values=g, dense_shape=(10, 4), bag=3, weights=w).weighted_fm
    assert not ops.IndexedSlices(indices=idx, values=g, dense_shape=(10, 4)).weighted_fm
    with pytest.raises(ValueError):
        ops.IndexedSlices(indices=idx, values=g, bag=3, sq_grad=q)                            # without weights
    with pytest.raises(ValueError):
        ops.IndexedSlices(indices=idx, values=g, weights=w, sq_grad=q)                        # without bag / bag_of
    with pytest.raises(ValueError):
        ops.IndexedSlices(indices=idx, values=g, bag=3, fm_grad=g, fm_sum=g, sq_grad=q)       # not with fm_grad
    with pytest.raises(ValueError):
        ops.IndexedSlices(indices=idx, values=None, bag=3, fm_grad=g, fm_sum=g, weights=w)    # weights + fm_grad: as before
    with pytest.raises(TypeError):
        ops.IndexedSlices(indices=idx, values=g, bag=3, weights=w, sq_grad=q.double())
    for call in (sl.expanded_values, sl.deduplicate, sl.to_dense, lambda: hetu_ops.unweighted_slices(sl)):
        with pytest.raises(ValueError, match="table row"):
            call()
    assert sl.weighted_fm and sl.values is g                                                  # the refusals changed nothing
    # update() carries the new field, and drops it
    plain = ops.IndexedSlices()
    plain.update(idx, g, (10, 4), bag=3, weights=w, sq_grad=q)
    assert plain.weighted_fm and plain.weighted and plain.bag == 3
    plain.update(idx, g, (10, 4), bag=3, weights=w)
    assert not plain.weighted_fm and plain.weighted
    with pytest.raises(ValueError):
        plain.update(idx, g, (10, 4), bag=3, sq_grad=q)


def test_the_operator_pair_and_the_ops_functions_exist():
    from herald_amd import hetu_ops, ops
    for name in ("EmbeddingLookUpWeightedFMSum", "EmbeddingLookUpWeightedFMSum_Gradient"):
        assert hasattr(hetu_ops, name), name
    for name in ("embedding_lookup_wfm", "wfm_grad_rows", "sgd_apply_wfm_bags", "sgd_sparse_update_wfm_bags"):
        assert hasattr(ops, name), name


def test_every_consumer_but_sgd_on_a_device_table_refuses_the_slices():
    import torch
    from herald_amd import hetu_ops, ops
    idx, g, w = torch.zeros((2, 3)), torch.ones((2, 4)), torch.ones((2, 3))
    sl = ops.IndexedSlices(indices=idx, values=g, dense_shape=(10, 4), bag=3, weights=w, sq_grad=g.clone())
    param = hetu_ops.EmbeddingParameter(table=torch.zeros((10, 4)))
    st = torch.zeros((10, 4))
    calls = [lambda: hetu_ops.momentum_update_sparse(param, sl, st, 0.1, 0.9, False),
             lambda: hetu_ops.adagrad_update_sparse(param, sl, st, 0.1, 1e-7),
             lambda: hetu_ops.adam_update_sparse(param, sl, st, st, 0.1, 0.9, 0.999, 0.9, 0.999, 1e-7),
             lambda: hetu_ops.adamw_update_sparse(param, sl, st, st, 0.1, 0.9, 0.999, 0.9, 0.999, 1e-7, 0.01)]
    for fuse in (True, False):
        with pytest.raises(ValueError, match="table row"):
            hetu_ops.adagrad_update_sparse(param, sl, st, 0.1, 1e-7, fuse_bags=fuse)
    for call in calls:
        with pytest.raises(ValueError, match="table row"):
            call()
    assert not param.table.any() and not st.any()

"""CPU-side checks of the fused FM-pooled sparse SGD apply (the pooled DeepFM step): the three new calls are declared, exported
and bound; their arguments are validated before any device access; the numpy restatement the GPU tests are held to
(tests/fm_pooled_model.py) equals the composed restatements -- fm_model.fm_grad_rows on the expanded g_sum, then
fm_model.sgd_serial -- bit for bit (those two are held to float64 bounds by tests/test_fm_cpu.py); and IndexedSlices' rules for
FM-pooled slices."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bag_model  # noqa: E402
import fm_model  # noqa: E402
import fm_pooled_model  # noqa: E402

from herald_amd import _lib  # noqa: E402

SYMBOLS = ["ha_sgd_apply_fm_bags", "ha_sgd_sparse_update_fm_bags_f32ids", "ha_sgd_sparse_update_fm_bags_u64ids"]


def test_fm_pooled_symbols_are_declared_exported_and_bound(lib):
    declared = _lib.declared_symbols()
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.ha_sgd_apply_fm_bags.argtypes) == 13
    assert len(lib.ha_sgd_sparse_update_fm_bags_f32ids.argtypes) == len(lib.ha_sgd_sparse_update_fm_bags_u64ids.argtypes) == 13


# non-null addresses that are never dereferenced: validation comes before any device access (there is no GPU here)
P = ctypes.c_void_p(0x1000)
Q = [ctypes.c_void_p(0x2000 + 0x1000 * i) for i in range(4)]


@pytest.mark.parametrize("case,args", [
    ("neither bag nor bag_of", dict(bag=0, bag_of=None)),
    ("both bag and bag_of", dict(bag=2, bag_of=P)),
    ("n not a multiple of bag", dict(n=7, bag=2, nbags=3)),
    ("n / bag is not nbags", dict(n=8, bag=2, nbags=3)),
    ("null g_fm", dict(g_fm=None)),
    ("null sum", dict(sum=None)),
    ("null table", dict(table=None)),
    ("null plan_ws", dict(plan_ws=None)),
    ("width 0", dict(width=0)),
    ("negative width", dict(width=-4)),
    ("negative n", dict(n=-1)),
    ("g_fm aliases the table", dict(g_fm=Q[0])),
    ("ragged occurrences in no bag", dict(bag=0, bag_of=P, nbags=0)),
])
def test_apply_fm_bags_rejects_bad_arguments_before_any_device_access(lib, case, args):
    a = dict(table=Q[0], rows=10, width=4, plan_ws=P, n=8, g_sum=Q[1], g_fm=Q[2], sum=Q[3], bag=2, bag_of=None, nbags=4)
    a.update(args)
    rc = lib.ha_sgd_apply_fm_bags(a["table"], a["rows"], a["width"], a["plan_ws"], a["n"], a["g_sum"], a["g_fm"], a["sum"],
                                  a["bag"], a["bag_of"], a["nbags"], 0.1, None)
    assert rc == -1, case
    assert b"ha_sgd_apply_fm_bags" in lib.ha_last_error(), (case, lib.ha_last_error())


@pytest.mark.parametrize("fn", SYMBOLS[1:])
@pytest.mark.parametrize("case,args", [
    ("neither bag nor offsets", dict(bag=0, offsets=None)),
    ("both bag and offsets", dict(bag=2, offsets=P)),
    ("n not a multiple of bag", dict(n=7, bag=2, nbags=3)),
    ("n / bag is not nbags", dict(n=8, bag=2, nbags=3)),
    ("null g_fm", dict(g_fm=None)),
    ("null sum", dict(sum=None)),
    ("null table", dict(table=None)),
    ("null ids", dict(ids=None)),
    ("width 0", dict(width=0)),
    ("negative n", dict(n=-1)),
    ("sum aliases the table", dict(sum=Q[0])),
])
def test_one_call_forms_reject_bad_arguments_before_any_device_access(lib, fn, case, args):
    a = dict(table=Q[0], rows=10, width=4, ids=P, n=8, bag=2, offsets=None, nbags=4, g_sum=Q[1], g_fm=Q[2], sum=Q[3])
    a.update(args)
    rc = getattr(lib, fn)(a["table"], a["rows"], a["width"], a["ids"], a["n"], a["bag"], a["offsets"], a["nbags"], a["g_sum"],
                          a["g_fm"], a["sum"], 0.1, None)
    assert rc == -1, case
    assert fn.encode() in lib.ha_last_error(), (case, lib.ha_last_error())


def test_no_ids_is_not_an_error(lib):
    assert lib.ha_sgd_apply_fm_bags(None, 10, 4, None, 0, None, None, None, 2, None, 0, 0.1, None) == 0
    assert lib.ha_sgd_apply_fm_bags(None, 10, 4, None, 0, None, None, None, 0, P, 3, 0.1, None) == 0      # ragged, every bag empty
    for fn in SYMBOLS[1:]:
        assert getattr(lib, fn)(None, 10, 4, None, 0, 2, None, 0, None, None, None, 0.1, None) == 0
        assert getattr(lib, fn)(None, 10, 4, None, 0, 0, P, 3, None, None, None, 0.1, None) == 0


# ---- the restatement against the composed restatements -----------------------------------------------------------------------
def _inputs(rows, width, B, seed):
    rng = np.random.default_rng(seed)
    table = (rng.standard_normal((rows, width)) * np.exp(rng.uniform(-4, 4, (rows, 1)))).astype(np.float32)
    g_sum = (rng.standard_normal((B, width)) * np.exp(rng.uniform(-3, 3, (B, 1)))).astype(np.float32)
    g_fm = (rng.standard_normal((B, width)) * np.exp(rng.uniform(-3, 3, (B, 1)))).astype(np.float32)
    return rng, table, g_sum, g_fm


def _composed(table, ids, g_sum, g_fm, S, lr, offsets=None):
    flat = np.asarray(ids).reshape(-1)
    bag = None if offsets is not None else np.asarray(ids).shape[1]
    rows, _, _, _ = fm_model.fm_lookup(table, ids, offsets)       # the rows of every occurrence (zeros for an id >= rows)
    G = fm_model.fm_grad_rows(fm_pooled_model.expand(g_sum, flat.size, S.shape[0], bag, offsets), rows, S, g_fm, bag=bag,
                              offsets=offsets)
    return fm_model.sgd_serial(table, flat, G, lr)


@pytest.mark.parametrize("with_sum", [True, False])
def test_restatement_equals_the_composed_restatements_fixed_bags(with_sum):
    rows, width, B, F, lr = 40, 7, 33, 6, 0.05
    rng, table, g_sum, g_fm = _inputs(rows, width, B, 11)
    ids = rng.integers(0, rows, (B, F)).astype(np.float32)
    ids[:, 0] = 3                                     # one key in every bag: a run of B occurrences
    ids[2, 1] = ids[2, 2] = 9                         # a duplicate inside a bag
    ids[5, 3], ids[B - 1, F - 1] = rows, rows + 7     # ids >= rows
    _, _, S, _ = fm_model.fm_lookup(table, ids)
    gs = g_sum if with_sum else None
    got = fm_pooled_model.fm_pooled_sgd(table, ids, gs, g_fm, S, lr)
    want = _composed(table, ids, gs, g_fm, S, lr)
    assert got.dtype == np.float32
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    touched = np.unique(ids[ids < rows].astype(np.int64))
    untouched = np.setdiff1d(np.arange(rows), touched)
    assert untouched.size and np.array_equal(got[untouched].view(np.int32), table[untouched].view(np.int32))
    assert not np.array_equal(got[3].view(np.int32), table[3].view(np.int32))


@pytest.mark.parametrize("with_sum", [True, False])
def test_restatement_equals_the_composed_restatements_ragged_bags_with_empty_bags(with_sum):
    rows, width, n, lr = 25, 5, 120, 0.1
    offsets = np.array([0, 0, 10, 37, 37, 37, 102, 120, 120], dtype=np.int64)
    B = offsets.size - 1
    rng, table, g_sum, g_fm = _inputs(rows, width, B, 12)
    ids = rng.integers(0, rows, n).astype(np.float32)
    ids[4], ids[50] = rows + 1, rows
    _, covered, S, _ = fm_model.fm_lookup(table, ids, offsets)
    assert covered.all()
    gs = g_sum if with_sum else None
    got = fm_pooled_model.fm_pooled_sgd(table, ids, gs, g_fm, S, lr, offsets)
    want = _composed(table, ids, gs, g_fm, S, lr, offsets)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert not np.array_equal(got.view(np.int32), table.view(np.int32))
    # the same bags given as fixed ones give the same bits
    ids2 = ids[:120].reshape(20, 6)
    rng2, _, g_sum2, g_fm2 = _inputs(rows, width, 20, 13)
    _, _, S2, _ = fm_model.fm_lookup(table, ids2)
    off2 = np.arange(21, dtype=np.int64) * 6
    a = fm_pooled_model.fm_pooled_sgd(table, ids2, g_sum2, g_fm2, S2, lr)
    b = fm_pooled_model.fm_pooled_sgd(table, ids2.reshape(-1), g_sum2, g_fm2, S2, lr, off2)
    assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_restatement_uses_the_row_before_the_call_for_every_occurrence():
    """Two occurrences of one key: the second one's e is still the original row, not the row after the first update."""
    table = np.array([[2.0]], dtype=np.float32)
    ids = np.array([[0.0, 0.0]], dtype=np.float32)
    S, g_fm, lr = np.array([[4.0]], np.float32), np.array([[1.0]], np.float32), 0.5
    # g = 1*4 - 1*2 = 2 for both occurrences: 2 - 1 - 1 = 0 (with e re-read after the first update it would be 2 - 1 - 1.5)
    assert fm_pooled_model.fm_pooled_sgd(table, ids, None, g_fm, S, lr)[0, 0] == 0.0


# ---- IndexedSlices ---------------------------------------------------------------------------------------------------------
def test_indexed_slices_fm_pooled_rules():
    from herald_amd import ops
    idx, g, s = np.zeros((2, 3), np.float32), np.ones((2, 4), np.float32), np.ones((2, 4), np.float32)
    sl = ops.IndexedSlices(indices=idx, values=None, dense_shape=(10, 4), bag=3, fm_grad=g, fm_sum=s)
    assert sl.fm_pooled and sl.pooled and sl.values is None and sl.fm_grad is g and sl.fm_sum is s
    assert ops.IndexedSlices(indices=idx, values=g, dense_shape=(10, 4), bag_of=np.zeros(6, np.int32), fm_grad=g, fm_sum=s).fm_pooled
    assert not ops.IndexedSlices(indices=idx, values=g, dense_shape=(10, 4), bag=3).fm_pooled
    assert not ops.IndexedSlices(indices=idx, values=g, dense_shape=(10, 4)).fm_pooled
    with pytest.raises(ValueError):
        ops.IndexedSlices(indices=idx, values=None, bag=3, fm_grad=g)                    # not together
    with pytest.raises(ValueError):
        ops.IndexedSlices(indices=idx, values=None, bag=3, fm_sum=s)
    with pytest.raises(ValueError):
        ops.IndexedSlices(indices=idx, values=None, fm_grad=g, fm_sum=s)                 # without bag / bag_of
    for method in ("deduplicate", "to_dense", "expanded_values"):
        with pytest.raises(ValueError, match="FM-pooled"):
            getattr(sl, method)()
    # update() carries the new fields, and drops them
    plain = ops.IndexedSlices()
    plain.update(idx, None, (10, 4), bag=3, fm_grad=g, fm_sum=s)
    assert plain.fm_pooled and plain.bag == 3
    plain.update(idx, g, (10, 4), bag=3)
    assert not plain.fm_pooled and plain.pooled
    with pytest.raises(ValueError):
        plain.update(idx, None, (10, 4), fm_grad=g, fm_sum=s)

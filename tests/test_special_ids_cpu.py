"""The id rule (include/herald_amd.h, "Which ids name a row") on the CPU side: the oracle's conversion and the numpy helper
against keys written out here, and every model that consumes ids against the same batch with its dead ids replaced by rows + 1.
Nothing here needs a GPU."""
import warnings

import numpy as np
import pytest

import bag_model
import fm_model
import fm_pooled_model
import special_ids
import test_optim_oracle as too
import wbag_model
from oracle import cpu
from oracle import optim_ref64 as ref64

ROWS, WIDTH = 37, 5
DEAD = 0xFFFFFFFE


def _bits(u32):
    return np.array([u32], dtype=np.uint32).view(np.float32)[0]


# float32 id -> key, literally (rows = 37)
FLOAT_TABLE = [
    (np.float32(-1.0), DEAD), (np.float32(-1.5), DEAD), (np.float32(-3e9), DEAD), (np.float32(-np.inf), DEAD),
    (np.float32(np.inf), DEAD), (np.float32(3.4e38), DEAD), (_bits(0x7FC00000), DEAD), (_bits(0xFFC00000), DEAD),
    (_bits(0x7FC12345), DEAD), (_bits(0xFF800001), DEAD), (np.float32(4294967296.0), DEAD),
    (np.float32(4294967040.0), 0xFFFFFF00), (np.float32(37.0), 37),
    (np.float32(-0.0), 0), (np.float32(-0.99), 0), (_bits(0xBF7FFFFF), 0),      # the float just above -1
    (np.float32(36.0), 36), (np.float32(36.5), 36), (np.float32(0.0), 0), (np.float32(5.75), 5),
    (np.float32(16777216.0), 16777216), (np.float32(2147483648.0), 0x80000000), (np.float32(4.0e9), 4000000000),
]
# int64 id -> key, literally
INT_TABLE = [
    (-1, DEAD), (-2 ** 63, DEAD), (2 ** 63 - 1, DEAD), (2 ** 32, DEAD), (2 ** 32 + 5, DEAD), (0xFFFFFFFF, DEAD),
    (0xFFFFFFFE, DEAD), (0xFFFFFFFD, 0xFFFFFFFD), (37, 37), (36, 36), (0, 0), (-2, DEAD),
]


def test_float_keys_match_the_table_written_out():
    ids = np.array([f for f, _ in FLOAT_TABLE], dtype=np.float32)
    want = np.array([k for _, k in FLOAT_TABLE], dtype=np.uint64)
    with warnings.catch_warnings():
        warnings.simplefilter("error")          # no cast of an out-of-range value: numpy warns about those
        got = special_ids.keys_of(ids)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(cpu.ids_to_keys(ids), want)
    assert got.dtype == np.uint64 and cpu.ids_to_keys(ids).dtype == np.uint64
    np.testing.assert_array_equal(special_ids.keys_of(ids.reshape(-1, 1)), want)      # flattened


def test_int_keys_match_the_table_written_out():
    ids = np.array([v for v, _ in INT_TABLE], dtype=np.int64)
    want = np.array([k for _, k in INT_TABLE], dtype=np.uint64)
    np.testing.assert_array_equal(special_ids.keys_of(ids), want)
    np.testing.assert_array_equal(special_ids.keys_of(ids.view(np.uint64)), want)
    np.testing.assert_array_equal(cpu.ids_to_keys(ids), want)
    np.testing.assert_array_equal(cpu.ids_to_keys(ids.view(np.uint64)), want)


def test_the_special_lists_carry_the_same_keys():
    """special_ids.float_specials / int_specials (what the GPU module feeds) agree with keys_of and the oracle."""
    fl = special_ids.float_specials(ROWS)
    ids = np.array([f for f, _ in fl], dtype=np.float32)
    want = np.array([k for _, k in fl], dtype=np.uint64)
    np.testing.assert_array_equal(special_ids.keys_of(ids), want)
    np.testing.assert_array_equal(cpu.ids_to_keys(ids), want)
    assert np.isnan(ids[6]) and np.isnan(ids[7]) and np.isnan(ids[8]) and np.signbit(ids[7]) and not np.signbit(ids[6])
    assert ids[8].view(np.uint32) & 0x3FFFFF
    il = special_ids.int_specials(ROWS)
    ids = np.array([v for v, _ in il], dtype=np.int64)
    want = np.array([k for _, k in il], dtype=np.uint64)
    np.testing.assert_array_equal(special_ids.keys_of(ids), want)
    np.testing.assert_array_equal(cpu.ids_to_keys(ids), want)


def test_in_range_ids_keep_the_keys_the_plain_cast_gave():
    rng = np.random.default_rng(5)
    f = np.concatenate([rng.uniform(0, 2.0 ** 32 - 512, 4000), rng.integers(0, 1 << 24, 4000)]).astype(np.float32)
    np.testing.assert_array_equal(special_ids.keys_of(f), f.astype(np.uint64))
    np.testing.assert_array_equal(cpu.ids_to_keys(f), f.astype(np.uint64))
    i = rng.integers(0, 0xFFFFFFFE, 4000)
    np.testing.assert_array_equal(special_ids.keys_of(i), i.astype(np.uint64))


def test_named_rows_of_the_float64_reference_follows_the_rule():
    ids = np.array([f for f, _ in FLOAT_TABLE], dtype=np.float32)
    keys = np.array([k for _, k in FLOAT_TABLE], dtype=np.int64)
    sel, idx = ref64.named_rows(ids, ROWS)
    np.testing.assert_array_equal(sel, np.flatnonzero(keys < ROWS))
    np.testing.assert_array_equal(idx, keys[keys < ROWS])


# ---- every model: a batch with specials == the batch with each dead id replaced by rows + 1 ---------------------------
def _batch(kind, n=60, seed=0):
    """n ids of [0, ROWS) with every special of the list twice (dead and live ones), shuffled."""
    rng = np.random.default_rng(seed)
    if kind == "f32":
        sp = np.array([f for f, _ in special_ids.float_specials(ROWS)] * 2, dtype=np.float32)
        ids = rng.integers(0, ROWS, n).astype(np.float32)
    else:
        sp = np.array([v for v, _ in special_ids.int_specials(ROWS)] * 2, dtype=np.int64)
        ids = rng.integers(0, ROWS, n).astype(np.int64)
    where = rng.permutation(n)[:sp.size]
    ids[where] = sp
    return ids


def _table(seed=1):
    return np.random.default_rng(seed).standard_normal((ROWS, WIDTH)).astype(np.float32)


RAGGED = np.array([0, 3, 3, 10, 11, 30, 60], dtype=np.int64)


def _same(a, b):
    for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        x, y = np.asarray(x), np.asarray(y)
        assert x.dtype == y.dtype and x.shape == y.shape
        np.testing.assert_array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                                      y.view(np.uint32) if y.dtype == np.float32 else y)


def test_replace_dead_keeps_live_specials_and_replaces_the_rest():
    for kind in ("f32", "i64"):
        ids = _batch(kind)
        rep = special_ids.replace_dead(ids, ROWS)
        dead = special_ids.keys_of(ids) >= ROWS
        assert rep.dtype == ids.dtype and dead.sum() >= (24 if kind == "f32" else 16)
        assert np.all(rep[dead] == ROWS + 1)
        _same(rep[~dead], ids[~dead])
        assert np.all(special_ids.keys_of(rep)[~dead] == special_ids.keys_of(ids)[~dead])


@pytest.mark.parametrize("kind", ["f32", "i64"])
@pytest.mark.parametrize("ragged", [False, True])
def test_bag_fm_and_wbag_models_treat_dead_ids_as_rows_plus_one(kind, ragged):
    table = _table()
    ids = _batch(kind)
    rep = special_ids.replace_dead(ids, ROWS)
    off = RAGGED if ragged else None
    if not ragged:
        ids, rep = ids.reshape(20, 3), rep.reshape(20, 3)
    nb = RAGGED.size - 1 if ragged else 20
    rng = np.random.default_rng(2)
    bg = rng.standard_normal((nb, WIDTH)).astype(np.float32)
    g = rng.standard_normal((60, WIDTH)).astype(np.float32)
    w = rng.integers(0, 2, 60).astype(np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _same(bag_model.bag_sum(table, ids, off), bag_model.bag_sum(table, rep, off))
        _same(bag_model.sgd_bags(table, ids, bg, 0.1, off), bag_model.sgd_bags(table, rep, bg, 0.1, off))
        a, b = fm_model.fm_lookup(table, ids, off), fm_model.fm_lookup(table, rep, off)
        _same(a, b)
        dead = special_ids.keys_of(ids) >= ROWS
        assert not a[0][dead].view(np.uint32).any()                       # dead occurrences: rows of +0.0
        _same(fm_model.sgd_serial(table, ids, g, 0.1), fm_model.sgd_serial(table, rep, g, 0.1))
        _same(fm_model.ps_push(table, ids, g, 0.1), fm_model.ps_push(table, rep, g, 0.1))
        S = a[2]
        _same(fm_pooled_model.fm_pooled_sgd(table, ids, bg, bg[::-1].copy(), S, 0.1, off),
              fm_pooled_model.fm_pooled_sgd(table, rep, bg, bg[::-1].copy(), S, 0.1, off))
        _same(wbag_model.live_mask(ROWS, ids, w), wbag_model.live_mask(ROWS, rep, w))
        _same(wbag_model.wbag_sum(table, ids, w, off), wbag_model.wbag_sum(table, rep, w, off))
        _same(wbag_model.wbag_sgd(table, ids, w, bg, 0.1, off), wbag_model.wbag_sgd(table, rep, w, bg, 0.1, off))
        _same(wbag_model.sgd_rows(table, ids, g, 0.1), wbag_model.sgd_rows(table, rep, g, 0.1))
        # and nothing leaked: a row that no live id names keeps its bits
        named = np.zeros(ROWS, dtype=bool)
        named[special_ids.rows_of(ids)[~dead]] = True
        _same(bag_model.sgd_bags(table, ids, bg, 0.1, off)[~named], table[~named])


def test_oracle_pull_update_and_push_treat_dead_ids_as_rows_plus_one():
    table = _table()
    ids = _batch("f32")
    rep = special_ids.replace_dead(ids, ROWS)
    dead = special_ids.keys_of(ids) >= ROWS
    g = np.random.default_rng(3).standard_normal((60, WIDTH)).astype(np.float32)
    out = cpu.sparse_pull(table, ids)
    _same(out, cpu.sparse_pull(table, rep))
    assert not out[dead].view(np.uint32).any()
    _same(out[~dead], table[special_ids.rows_of(ids)[~dead]])
    _same(cpu.embedding_lookup(table, ids.reshape(20, 3)), out.reshape(20, 3, WIDTH))
    _same(cpu.sgd_sparse_update(table.copy(), ids, g, 0.1), cpu.sgd_sparse_update(table.copy(), rep, g, 0.1))
    _same(cpu.sgd_sparse_update(table.copy(), ids, g, 0.1), fm_model.sgd_serial(table, ids, g, 0.1))
    _same(cpu.sparse_push(table.copy(), ids, g, 0.1), cpu.sparse_push(table.copy(), rep, g, 0.1))
    _same(cpu.sparse_push(table.copy(), ids, g, 0.1), fm_model.ps_push(table, ids, g, 0.1))
    # all dead occurrences of a batch are one run of one key
    uniq, inverse, counts = cpu.unique(cpu.ids_to_keys(ids))
    assert uniq[-1] == DEAD and counts[-1] == np.count_nonzero(special_ids.keys_of(ids) == DEAD)
    assert np.count_nonzero(uniq >= ROWS) == 3          # rows, 0xFFFFFF00 and the dead key


def test_oracle_entry_points_from_before_the_row_count_keep_their_signatures():
    """oracle_embedding_lookup / oracle_sgd_sparse_update / oracle_push_apply are bound by name and argument list by front-ends
    older than the *_rows forms: called the old way, on ids that all name rows, they give what the *_rows forms give."""
    import ctypes
    c = ctypes
    L = c.CDLL(cpu.lib()._name)       # a handle of its own: no argtypes of oracle/cpu.py on it
    L.oracle_embedding_lookup.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t, c.c_void_p]
    L.oracle_sgd_sparse_update.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t, c.c_void_p, c.c_float]
    L.oracle_push_apply.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t, c.c_void_p]
    p = lambda a: a.ctypes.data_as(c.c_void_p)                                                  # noqa: E731
    rng = np.random.default_rng(8)
    table = _table()
    ids = np.concatenate([rng.integers(0, ROWS, 40).astype(np.float32), np.float32([-0.0, -0.99, ROWS - 0.5])])
    g = rng.standard_normal((ids.size, WIDTH)).astype(np.float32)
    out = np.empty((ids.size, WIDTH), dtype=np.float32)
    assert L.oracle_embedding_lookup(p(table), WIDTH, p(ids), ids.size, p(out)) == 0
    _same(out, cpu.embedding_lookup(table, ids))
    t = table.copy()
    assert L.oracle_sgd_sparse_update(p(t), WIDTH, p(ids), ids.size, p(g), c.c_float(0.1)) == 0
    _same(t, cpu.sgd_sparse_update(table.copy(), ids, g, 0.1))
    uniq, _, red = cpu.dedup_reduce(ids, g)
    t = table.copy()
    assert L.oracle_push_apply(p(t), WIDTH, p(uniq), uniq.size, p(red)) == 0
    _same(t, cpu.push_apply(table.copy(), uniq, red))


@pytest.mark.parametrize("op", too.OPS + ("momentum", "nesterov"))
def test_optimizer_restatement_and_float64_reference_treat_dead_ids_as_rows_plus_one(op):
    rng = np.random.default_rng(4)
    f = np.float32
    a = dict(param=rng.standard_normal((ROWS, WIDTH), dtype=f), m=rng.standard_normal((ROWS, WIDTH), dtype=f),
             v=rng.standard_normal((ROWS, WIDTH), dtype=f) ** 2, acc=rng.standard_normal((ROWS, WIDTH), dtype=f) ** 2,
             velocity=rng.standard_normal((ROWS, WIDTH), dtype=f))
    fl = special_ids.float_specials(ROWS)
    dead_ids = np.array([x for x, k in fl if k >= ROWS], dtype=f)
    if op in ("momentum", "nesterov"):          # repeats allowed
        ids = _batch("f32")
    else:                                        # unique live ids: 0 (as -0.0), rows - 1 (as rows - 0.5) and 20 more, all dead ones
        ids = np.concatenate([rng.permutation(np.arange(1, ROWS - 1))[:20].astype(f), f([-0.0, ROWS - 0.5]), dead_ids, dead_ids])
        ids = ids[rng.permutation(ids.size)]
    rep = special_ids.replace_dead(ids, ROWS)
    grads = rng.standard_normal((ids.size, WIDTH), dtype=f)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        new, want = too.step32(op, a, ids, grads, 2), too.step32(op, a, rep, grads, 2)
        for name in new:
            _same(new[name], want[name])
        sel, idx, out = too.step64(op, a, ids, grads, 2)
        sel2, idx2, out2 = too.step64(op, a, rep, grads, 2)
    np.testing.assert_array_equal(sel, sel2)
    np.testing.assert_array_equal(idx, idx2)
    np.testing.assert_array_equal(sel, np.flatnonzero(special_ids.keys_of(ids) < ROWS))
    for name in out:
        np.testing.assert_array_equal(out[name][0], out2[name][0])

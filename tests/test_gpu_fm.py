"""FM-pooled embedding lookup and its per-occurrence gradient on the GPU (the DeepFM models): ha_gather_fm_* and ha_fm_grad_rows
against the numpy restatement (tests/fm_model.py) bit for bit, at the smallest shapes that reach each branch of the kernels --
the three vector widths, a partly live last column slice, more than one slice, the 64-id block edge, a partial round of row
loads, two blocks of ids, ragged bags -- and the width-1 sum-pooled lookup and apply of the models' first-order table against
tests/bag_model.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bag_model  # noqa: E402
import fm_model  # noqa: E402

from herald_amd import _lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS = 300                       # a small table: ids repeat within a bag
WIDTHS = [1, 5, 6, 64, 100, 128, 260, 512]
# (ids per bag, bags): one id (the 8-rows-per-round kernels), 26 (a partial round of 32), 64 (the block edge), 65 and 130 (two
# and three blocks), with 1, 3 and 256 bags
SHAPES = [(1, 3), (26, 1), (26, 256), (64, 1), (65, 3), (130, 3)]


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


_tables = {}


def _table(width):
    """One table per width, shared and never written: magnitudes over many binades so that the order of a sum shows, row 5
    all -0.0."""
    if width not in _tables:
        rng = np.random.default_rng(1000 + width)
        t = (rng.standard_normal((ROWS, width)) * np.exp(rng.uniform(-8, 8, (ROWS, 1)))).astype(np.float32)
        t[5] = -0.0
        _tables[width] = t
    return _tables[width]


def _fixed_ids(B, F, seed):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, ROWS, (B, F)).astype(np.float32)
    if F >= 2:
        ids[0, 1] = ids[0, 0]              # a duplicate id inside a bag
    ids[B - 1, F - 1] = ROWS + 3           # an id >= rows: a zero row in all three outputs
    ids[min(1, B - 1), 0] = ROWS           # the first id beyond the table
    ids[0, 0] = 5                          # the -0.0 row
    return ids


def _slices(width):
    """ha_debug_bag_slice settings that reach VEC 1 (automatic at these batch sizes), 2 and 4."""
    return (0, 128, 256) if width % 4 == 0 else (0,)


def _check_forward(d_table, table, d_ids, ids, d_off=None, off=None, what=None):
    rows_m, covered, S_m, fm_m = fm_model.fm_lookup(table, ids, off)
    width = table.shape[1]
    sentinel = 12345.0
    rows_buf = torch.full(tuple(d_ids.shape) + (width,), sentinel, dtype=torch.float32, device=d_table.device)
    rows, S, fm = ops.embedding_lookup_fm(d_table, d_ids, offsets=d_off, rows_out=rows_buf)
    assert rows.data_ptr() == rows_buf.data_ptr()
    assert S.shape == fm.shape == (S_m.shape[0], width)
    assert np.array_equal(_bits(S), _bits(S_m)), what
    assert np.array_equal(_bits(fm), _bits(fm_m)), what
    got_rows = rows.reshape(-1, width).cpu().numpy()
    assert np.array_equal(_bits(got_rows[covered]), _bits(rows_m[covered])), what
    assert np.all(got_rows[~covered] == sentinel), what         # an occurrence in no bag: its row is not written
    # the sum is the sum-pooled lookup's and the rows are the gather's
    assert np.array_equal(_bits(S), _bits(ops.embedding_lookup_sum(d_table, d_ids, offsets=d_off))), what
    assert np.array_equal(_bits(got_rows[covered]),
                          _bits(ops.embedding_lookup(d_table, d_ids).reshape(-1, width).cpu().numpy()[covered])), what
    return rows, S, fm


@pytest.mark.parametrize("d", WIDTHS)
def test_forward_fixed_bags_equal_the_restatement_bit_for_bit(dev, d):
    table = _table(d)
    d_table = torch.from_numpy(table).to(dev)
    L = _lib.load()
    try:
        for floats in _slices(d):
            assert L.ha_debug_bag_slice(floats) == 0
            for F, B in SHAPES:
                ids = _fixed_ids(B, F, 100 * F + B)
                _check_forward(d_table, table, torch.from_numpy(ids).to(dev), ids, what=(d, floats, F, B))
    finally:
        L.ha_debug_bag_slice(0)


def test_forward_table_view_that_is_not_16_byte_aligned(dev):
    d, F, B = 128, 26, 3
    table = _table(d)
    buf = torch.zeros(ROWS * d + 4, dtype=torch.float32, device=dev)
    d_table = buf[1:1 + ROWS * d].view(ROWS, d)
    d_table.copy_(torch.from_numpy(table))
    assert d_table.data_ptr() % 16 == 4 and d_table.is_contiguous()
    ids = _fixed_ids(B, F, 31)
    _check_forward(d_table, table, torch.from_numpy(ids).to(dev), ids)
    # ... and unaligned outputs
    out = torch.zeros(B * F * d + 2 * B * d + 12, dtype=torch.float32, device=dev)
    aligned = torch.from_numpy(table).to(dev)
    rows = out[1:1 + B * F * d].view(B, F, d)
    S = out[B * F * d + 5:B * F * d + 5 + B * d].view(B, d)
    fm = out[B * F * d + B * d + 9:B * F * d + 2 * B * d + 9].view(B, d)
    ops.embedding_lookup_fm(aligned, torch.from_numpy(ids).to(dev), rows_out=rows, sum_out=S, fm_out=fm)
    rows_m, _, S_m, fm_m = fm_model.fm_lookup(table, ids)
    assert np.array_equal(_bits(rows.reshape(-1, d)), _bits(rows_m))
    assert np.array_equal(_bits(S), _bits(S_m)) and np.array_equal(_bits(fm), _bits(fm_m))


def test_forward_int64_ids_and_no_rows(dev):
    d, F, B = 260, 26, 3
    table = _table(d)
    d_table = torch.from_numpy(table).to(dev)
    ids = _fixed_ids(B, F, 7)
    rows_m, _, S_m, fm_m = fm_model.fm_lookup(table, ids)
    d_ids64 = torch.from_numpy(ids.astype(np.int64)).to(dev)
    rows, S, fm = ops.embedding_lookup_fm(d_table, d_ids64)
    assert rows.shape == (B, F, d)
    assert np.array_equal(_bits(rows.reshape(-1, d)), _bits(rows_m))
    assert np.array_equal(_bits(S), _bits(S_m)) and np.array_equal(_bits(fm), _bits(fm_m))
    for d_ids in (d_ids64, torch.from_numpy(ids).to(dev)):
        none, S, fm = ops.embedding_lookup_fm(d_table, d_ids, want_rows=False)
        assert none is None
        assert np.array_equal(_bits(S), _bits(S_m)) and np.array_equal(_bits(fm), _bits(fm_m))
    # the row-buffer route of the operators: the rows as a table, ids 0 .. n-1, no row store
    pos = torch.arange(B * F, dtype=torch.int64, device=dev).view(B, F)
    _, S, fm = ops.embedding_lookup_fm(rows.view(B * F, d), pos, want_rows=False)
    assert np.array_equal(_bits(S), _bits(S_m)) and np.array_equal(_bits(fm), _bits(fm_m))
    with pytest.raises(ValueError):
        ops.embedding_lookup_fm(d_table, d_ids64, rows_out=rows, want_rows=False)


def test_forward_float32_ids_beyond_2_to_24_at_width_1(dev):
    rows, d = (1 << 24) + 64, 1
    d_table = torch.zeros((rows, d), dtype=torch.float32, device=dev)
    top = np.array([(1 << 24) + 2, (1 << 24) + 62, (1 << 24) - 1, (1 << 24) + 4, 7, (1 << 24) + 62], dtype=np.int64)
    rng = np.random.default_rng(24)
    vals = (rng.standard_normal((rows - ((1 << 24) - 8), d)) * 100).astype(np.float32)
    d_table[(1 << 24) - 8:] = torch.from_numpy(vals).to(dev)
    d_table[7] = 3.25
    ids = top.astype(np.float32).reshape(3, 2)
    assert np.array_equal(ids.astype(np.int64).reshape(-1), top)       # (all exactly representable)
    got_rows, S, fm = ops.embedding_lookup_fm(d_table, torch.from_numpy(ids).to(dev))
    picked = d_table[torch.from_numpy(top).to(dev)].cpu().numpy()       # [6, 1]
    rows_m, _, S_m, fm_m = fm_model.fm_lookup(picked, np.arange(6, dtype=np.float32).reshape(3, 2))
    assert np.array_equal(_bits(got_rows.reshape(-1, d)), _bits(rows_m))
    assert np.array_equal(_bits(S), _bits(S_m)) and np.array_equal(_bits(fm), _bits(fm_m))
    assert np.abs(S_m).min() > 0 and np.abs(fm_m).max() > 0


RAGGED = {
    # n = 300 ids
    "empty first, middle and last bag": [0, 0, 10, 37, 37, 37, 102, 300, 300],
    "a first offset above 0 and a last one beyond n": [7, 7, 71, 72, 137, 1 << 40],
    "a last offset below n, one bag of 130 ids": [0, 130, 131, 290],
}


@pytest.mark.parametrize("d", [5, 64, 260])
def test_forward_ragged_bags(dev, d):
    table = _table(d)
    d_table = torch.from_numpy(table).to(dev)
    rng = np.random.default_rng(d)
    n = 300
    ids = rng.integers(0, ROWS, n).astype(np.float32)
    ids[9], ids[200], ids[40] = ROWS + 1, 5, ROWS
    d_ids = torch.from_numpy(ids).to(dev)
    L = _lib.load()
    try:
        for floats in _slices(d):
            assert L.ha_debug_bag_slice(floats) == 0
            for name, off in RAGGED.items():
                off = np.array(off, dtype=np.int64)
                _check_forward(d_table, table, d_ids, ids, torch.from_numpy(off).to(dev), off, what=(name, floats))
    finally:
        L.ha_debug_bag_slice(0)
    # n = 0: every bag is empty
    off = torch.zeros(4, dtype=torch.int64, device=dev)
    _, S, fm = ops.embedding_lookup_fm(d_table, torch.empty(0, dtype=torch.float32, device=dev), offsets=off)
    assert np.array_equal(_bits(S), np.zeros((3, d), np.int32)) and np.array_equal(_bits(fm), np.zeros((3, d), np.int32))


def test_forward_writes_nothing_behind_its_outputs(dev):
    d, F, B = 100, 26, 3
    table = _table(d)
    ids = _fixed_ids(B, F, 3)
    rows = torch.full((B * F + 1, d), 7.0, dtype=torch.float32, device=dev)
    S = torch.full((B + 1, d), 7.0, dtype=torch.float32, device=dev)
    fm = torch.full((B + 1, d), 7.0, dtype=torch.float32, device=dev)
    ops.embedding_lookup_fm(torch.from_numpy(table).to(dev), torch.from_numpy(ids).to(dev), rows_out=rows[:B * F].view(B, F, d),
                            sum_out=S[:B], fm_out=fm[:B])
    rows_m, _, S_m, fm_m = fm_model.fm_lookup(table, ids)
    assert np.array_equal(_bits(rows[:B * F]), _bits(rows_m)) and np.array_equal(_bits(fm[:B]), _bits(fm_m))
    assert torch.all(rows[B * F] == 7.0) and torch.all(S[B] == 7.0) and torch.all(fm[B] == 7.0)


# ---- the gradient kernel --------------------------------------------------------------------------------------------------
def _grad_inputs(d, B, F, seed):
    rng = np.random.default_rng(seed)
    table = _table(d)
    ids = _fixed_ids(B, F, seed)
    e, _, S, _ = fm_model.fm_lookup(table, ids)
    g = (rng.standard_normal((B * F, d)) * np.exp(rng.uniform(-4, 4, (B * F, 1)))).astype(np.float32)
    gf = (rng.standard_normal((B, d)) * np.exp(rng.uniform(-4, 4, (B, 1)))).astype(np.float32)
    return e, S, g, gf


@pytest.mark.parametrize("d", WIDTHS)
def test_gradient_fixed_bags_with_and_without_row_gradients_and_in_place(dev, d):
    B, F = 5, 26
    e, S, g, gf = _grad_inputs(d, B, F, 40 + d)
    d_e, d_S, d_gf = (torch.from_numpy(a).to(dev) for a in (e, S, gf))
    d_g = torch.from_numpy(g).to(dev)
    want = fm_model.fm_grad_rows(g, e, S, gf, bag=F)
    out = ops.fm_grad_rows(d_g, d_e.view(B, F, d), d_S, d_gf, bag=F)
    assert out.shape == (B, F, d) and out.data_ptr() != d_g.data_ptr()
    assert np.array_equal(_bits(out.reshape(-1, d)), _bits(want))
    assert np.array_equal(_bits(d_g), _bits(g))                              # the inputs as they were
    # no consumer of the rows
    out = ops.fm_grad_rows(None, d_e, d_S, d_gf, bag=F)
    assert np.array_equal(_bits(out), _bits(fm_model.fm_grad_rows(None, e, S, gf, bag=F)))
    # in place over the rows' gradient
    same = ops.fm_grad_rows(d_g, d_e, d_S, d_gf, bag=F, out=d_g)
    assert same.data_ptr() == d_g.data_ptr()
    assert np.array_equal(_bits(d_g), _bits(want))
    assert np.array_equal(_bits(d_e), _bits(e)) and np.array_equal(_bits(d_S), _bits(S)) and np.array_equal(_bits(d_gf), _bits(gf))


@pytest.mark.parametrize("d", [5, 128])
def test_gradient_ragged_bags_and_unaligned_pointers(dev, d):
    n = 130
    off = np.array([0, 0, 10, 75, 75, 130, 130], dtype=np.int64)
    B = off.size - 1
    rng = np.random.default_rng(d)
    table = _table(d)
    ids = rng.integers(0, ROWS, n).astype(np.float32)
    e, covered, S, _ = fm_model.fm_lookup(table, ids, off)
    assert covered.all()
    g = rng.standard_normal((n, d)).astype(np.float32)
    gf = rng.standard_normal((B, d)).astype(np.float32)
    d_e, d_S, d_gf, d_g = (torch.from_numpy(a).to(dev) for a in (e, S, gf, g))
    which = ops.bag_of(torch.from_numpy(off).to(dev), n)
    want = fm_model.fm_grad_rows(g, e, S, gf, offsets=off)
    assert np.array_equal(_bits(ops.fm_grad_rows(d_g, d_e, d_S, d_gf, bag_of=which)), _bits(want))
    assert np.array_equal(_bits(ops.fm_grad_rows(None, d_e, d_S, d_gf, bag_of=which)),
                          _bits(fm_model.fm_grad_rows(None, e, S, gf, offsets=off)))
    # an output that is not 16-byte aligned takes the scalar path
    buf = torch.zeros(n * d + 4, dtype=torch.float32, device=dev)
    out = buf[1:1 + n * d].view(n, d)
    ops.fm_grad_rows(d_g, d_e, d_S, d_gf, bag_of=which, out=out)
    assert np.array_equal(_bits(out), _bits(want)) and float(buf[0]) == 0.0 and torch.all(buf[1 + n * d:] == 0)
    with pytest.raises(ValueError):
        ops.fm_grad_rows(d_g, d_e, d_S, d_gf)
    with pytest.raises(ValueError):
        ops.fm_grad_rows(d_g, d_e, d_S, d_gf, bag=5, bag_of=which)


# ---- a full step ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [6, 128])
def test_full_step_equals_the_restatement_and_the_serial_apply(dev, d):
    B, F, lr = 9, 26, 0.05
    rng = np.random.default_rng(60 + d)
    table = rng.standard_normal((ROWS, d)).astype(np.float32)
    ids = _fixed_ids(B, F, 61)
    d_table, d_ids = torch.from_numpy(table).to(dev), torch.from_numpy(ids).to(dev)
    rows, S, fm = ops.embedding_lookup_fm(d_table, d_ids)
    g = rng.standard_normal((B, F, d)).astype(np.float32)
    gf = rng.standard_normal((B, d)).astype(np.float32)
    grad = ops.fm_grad_rows(torch.from_numpy(g).to(dev), rows, S, torch.from_numpy(gf).to(dev), bag=F)
    ops.sgd_sparse_update(d_table, d_ids.reshape(-1), grad.reshape(-1, d), lr)
    rows_m, _, S_m, _ = fm_model.fm_lookup(table, ids)
    want = fm_model.sgd_serial(table, ids, fm_model.fm_grad_rows(g, rows_m, S_m, gf, bag=F), lr)
    assert np.array_equal(_bits(d_table), _bits(want))
    assert not np.array_equal(_bits(want), _bits(table))


# ---- the first-order table: width 1 through the sum-pooled lookup and the bag apply ------------------------------------------
def test_width_1_sum_pooled_lookup_and_bag_apply(dev):
    B, F, lr = 37, 26, 0.05
    rng = np.random.default_rng(71)
    table = (rng.standard_normal((ROWS, 1)) * np.exp(rng.uniform(-8, 8, (ROWS, 1)))).astype(np.float32)
    ids = _fixed_ids(B, F, 72)
    d_table, d_ids = torch.from_numpy(table).to(dev), torch.from_numpy(ids).to(dev)
    out = ops.embedding_lookup_sum(d_table, d_ids)
    assert out.shape == (B, 1)
    assert np.array_equal(_bits(out), _bits(bag_model.bag_sum(table, ids)))
    g = rng.standard_normal((B, 1)).astype(np.float32)
    ops.sgd_sparse_update_bags(d_table, d_ids, torch.from_numpy(g).to(dev), lr)
    want = bag_model.sgd_bags(table, ids, g, lr)
    assert np.array_equal(_bits(d_table), _bits(want)) and not np.array_equal(_bits(want), _bits(table))
    # ragged bags, int64 ids
    off = np.array([0, 0, 100, 101, B * F], dtype=np.int64)
    flat = ids.reshape(-1)
    d_off, d_flat = torch.from_numpy(off).to(dev), torch.from_numpy(flat.astype(np.int64)).to(dev)
    d_table = torch.from_numpy(table).to(dev)
    assert np.array_equal(_bits(ops.embedding_lookup_sum(d_table, d_flat, offsets=d_off)), _bits(bag_model.bag_sum(table, flat, off)))
    g4 = rng.standard_normal((4, 1)).astype(np.float32)
    ops.sgd_sparse_update_bags(d_table, d_flat, torch.from_numpy(g4).to(dev), lr, offsets=d_off)
    assert np.array_equal(_bits(d_table), _bits(bag_model.sgd_bags(table, flat, g4, lr, off)))

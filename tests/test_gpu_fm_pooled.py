"""The fused FM-pooled sparse SGD apply on the GPU (ha_sgd_apply_fm_bags and its one-call forms): every case is compared bit
for bit, over the whole table, with the numpy restatement (tests/fm_pooled_model.py) AND with the composed GPU sequence --
embedding_lookup, fm_grad_rows on the expanded g_sum, sgd_apply -- and the one-call form with plan + apply.  Shapes are the
smallest that reach each path of the kernel: runs of 1 .. 47 occurrences (one wave, batches of 4 or 16 loads), 48 and more (the
workgroup's cooperative path; 120 occurrences per round, so 384 is three full rounds and a part, 49 seven waves' worth),
the scalar and the 16-byte path, one, two and more 64-column slices, a partly live last slice, more items than one round of
the grid.  The table always sits between guard rows."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fm_model  # noqa: E402
import fm_pooled_model  # noqa: E402

from herald_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu

LR = 0.05
GUARD = 2          # rows in front of and behind the table


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _values(rng, shape, spread):
    return (rng.standard_normal(shape) * np.exp(rng.uniform(-spread, spread, (shape[0], 1)))).astype(np.float32)


class Case:
    """The inputs of one case on the host and the device, and the restatement's result (computed once)."""

    def __init__(self, dev, rows, d, ids, offsets, with_sum, seed, int64_ids=False, off16=0):
        rng = np.random.default_rng(seed)
        self.dev, self.rows, self.d, self.ids, self.offsets = dev, rows, d, ids, offsets
        self.table = _values(rng, (rows, d), 3)
        self.nbags = ids.shape[0] if offsets is None else offsets.size - 1
        self.bag = ids.shape[1] if offsets is None else None
        self.g_sum = _values(rng, (self.nbags, d), 2) if with_sum else None
        self.g_fm = _values(rng, (self.nbags, d), 2)
        self.d_ids = torch.from_numpy(ids.astype(np.int64) if int64_ids else ids).to(dev)
        self.d_off = torch.from_numpy(offsets).to(dev) if offsets is not None else None
        self.d_g_sum = torch.from_numpy(self.g_sum).to(dev) if with_sum else None
        self.d_g_fm = torch.from_numpy(self.g_fm).to(dev)
        self.off16 = off16
        # the forward, as the model runs it: no rows
        none, self.d_S, _ = ops.embedding_lookup_fm(self.fresh_table()[1], self.d_ids, offsets=self.d_off, want_rows=False)
        assert none is None
        _, _, self.S, _ = fm_model.fm_lookup(self.table, ids, offsets)
        assert _same(self.d_S, torch.from_numpy(self.S).to(dev))
        self.want = fm_pooled_model.fm_pooled_sgd(self.table, ids, self.g_sum, self.g_fm, self.S, LR, offsets)
        assert not np.array_equal(self.want, self.table)

    def fresh_table(self):
        """(buffer, table view): the table between GUARD rows of a sentinel; off16 floats off 16-byte alignment."""
        n = (self.rows + 2 * GUARD) * self.d
        buf = torch.full((n + 4,), 777.0, dtype=torch.float32, device=self.dev)
        view = buf[self.off16 + GUARD * self.d:self.off16 + (GUARD + self.rows) * self.d].view(self.rows, self.d)
        view.copy_(torch.from_numpy(self.table))
        return buf, view

    def guards_intact(self, buf):
        lo, hi = self.off16 + GUARD * self.d, self.off16 + (GUARD + self.rows) * self.d
        return bool(torch.all(buf[:lo] == 777.0)) and bool(torch.all(buf[hi:] == 777.0))

    def bag_args(self):
        if self.offsets is None:
            return dict(bag=self.bag)
        return dict(bag_of=ops.bag_of(self.d_off, self.d_ids.numel()))

    def plan(self):
        flat = self.d_ids.reshape(-1)
        return ops.IndexPlan(max(flat.numel(), 1), device=self.dev).sort(flat).finish()

    def fused(self):
        buf, table = self.fresh_table()
        ops.sgd_apply_fm_bags(table, self.plan(), self.d_g_sum, self.d_g_fm, self.d_S, LR, **self.bag_args())
        return buf, table

    def one_call(self):
        buf, table = self.fresh_table()
        ops.sgd_sparse_update_fm_bags(table, self.d_ids, self.d_g_sum, self.d_g_fm, self.d_S, LR, offsets=self.d_off)
        return buf, table

    def composed(self):
        """E = gather, G = fm_grad_rows(expand(g_sum), E, S, g_fm), sgd_apply(table, plan, G)."""
        buf, table = self.fresh_table()
        ba = self.bag_args()
        flat = self.d_ids.reshape(-1)
        E = ops.embedding_lookup(table, flat)
        g_rows = None
        if self.d_g_sum is not None:
            which = torch.arange(flat.numel(), device=self.dev) // self.bag if self.offsets is None else ba["bag_of"].long()
            g_rows = self.d_g_sum[which].contiguous()
        G = ops.fm_grad_rows(g_rows, E, self.d_S, self.d_g_fm, **ba)
        ops.sgd_apply(table, self.plan(), G, LR, finished=True)
        return buf, table

    def check(self, what=None):
        want = torch.from_numpy(self.want).to(self.dev)
        buf, got = self.fused()
        assert _same(got, want), ("fused vs restatement", what)
        assert self.guards_intact(buf), what
        buf_c, comp = self.composed()
        assert _same(got, comp), ("fused vs composed", what)
        buf_1, one = self.one_call()
        assert _same(got, one), ("one call vs plan + apply", what)
        assert self.guards_intact(buf_1), what
        return got


# ---- fixed bags ------------------------------------------------------------------------------------------------------------
ROWS = 997
RUNS = [1, 2, 3, 4, 15, 16, 17, 47, 48, 49]


def _fixed_ids():
    """B = 64 bags of F = 26: column 0 all id 0 (a run of 64), column 1 from 3 ids (medium runs), key 10 + j exactly RUNS[j]
    times, the rest from [100, ROWS) with three ids >= ROWS mixed in."""
    B, F = 64, 26
    rng = np.random.default_rng(2024)
    ids = np.empty((B, F), dtype=np.float32)
    ids[:, 0] = 0
    ids[:, 1] = rng.integers(1, 4, B)
    rest = rng.integers(100, ROWS, B * (F - 2)).astype(np.float32)
    forced = np.concatenate([np.full(L, 10 + j, dtype=np.float32) for j, L in enumerate(RUNS)])
    where = rng.permutation(rest.size)[:forced.size + 3]
    rest[where[:forced.size]] = forced
    rest[where[forced.size:]] = [ROWS, ROWS + 5, 1 << 20]
    ids[:, 2:] = rest.reshape(B, F - 2)
    return ids


def test_the_forced_run_lengths_are_there():
    keys, counts = np.unique(_fixed_ids(), return_counts=True)
    got = dict(zip(keys.astype(np.int64).tolist(), counts.tolist()))
    assert got[0] == 64 and all(got[10 + j] == L for j, L in enumerate(RUNS))
    assert 4 <= min(got[1], got[2], got[3]) and max(got[1], got[2], got[3]) < 48
    assert sum(c for k, c in got.items() if k >= ROWS) == 3


@pytest.mark.parametrize("with_sum", [True, False], ids=["g_sum", "no_g_sum"])
@pytest.mark.parametrize("d", [1, 5, 16, 64, 128, 132, 512])
def test_fixed_bags_every_run_class(dev, d, with_sum):
    case = Case(dev, ROWS, d, _fixed_ids(), None, with_sum, seed=d)
    got = case.check((d, with_sum))
    # rows that no id names keep their bits
    named = np.unique(case.ids[case.ids < ROWS].astype(np.int64))
    rest = torch.from_numpy(np.setdiff1d(np.arange(ROWS), named)).to(dev)
    assert rest.numel() and _same(got[rest], torch.from_numpy(case.table).to(dev)[rest])


@pytest.mark.parametrize("d", [128, 260])
def test_a_run_of_384_occurrences(dev, d):
    B, F, rows = 384, 3, 500
    rng = np.random.default_rng(d)
    ids = rng.integers(1, rows + 20, (B, F)).astype(np.float32)       # ids >= rows among them
    ids[:, 1] = 0                                                     # the hot column
    Case(dev, rows, d, ids, None, True, seed=384 + d).check(d)


def test_int64_ids(dev):
    Case(dev, ROWS, 64, _fixed_ids(), None, True, seed=64, int64_ids=True).check()
    off = np.array([0, 40, 40, 100], dtype=np.int64)
    ids = np.random.default_rng(5).integers(0, 30, 100).astype(np.float32)
    Case(dev, 25, 12, ids, off, False, seed=65, int64_ids=True).check()


def test_a_table_view_4_bytes_off_16_byte_alignment(dev):
    case = Case(dev, ROWS, 8, _fixed_ids(), None, True, seed=8, off16=1)
    _, view = case.fresh_table()
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    case.check()


# ---- ragged bags -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [5, 64, 260])
def test_ragged_bags_with_empty_bags(dev, d):
    n, rows = 600, 120
    off = np.array([0, 0, 10, 37, 37, 37, 230, 231, 600, 600], dtype=np.int64)
    rng = np.random.default_rng(d)
    ids = rng.integers(0, rows + 6, n).astype(np.float32)
    ids[rng.permutation(n)[:60]] = 7                                  # a run of 60 across the bags
    for with_sum in (True, False):
        Case(dev, rows, d, ids, off, with_sum, seed=d + 1).check((d, with_sum))


# ---- more than 36,864 ids: the plan's large-batch sort ---------------------------------------------------------------------------
def test_more_than_36864_ids_fixed_and_ragged(dev):
    B, F, rows, d = 1536, 26, 5000, 8
    rng = np.random.default_rng(39936)
    ids = rng.integers(0, rows + 50, (B, F)).astype(np.float32)
    ids[:, 3] = 17                                                    # the hot column: a run of 1,536
    ids[:, 4] = rng.integers(20, 24, B)                               # and four runs of some 384
    fixed = Case(dev, rows, d, ids, None, True, seed=1)
    assert fixed.d_ids.numel() == 39936 > 36864
    got = fixed.check("fixed")
    # the same bags given as ragged ones: the same inputs (same seed), the same result
    off = np.arange(B + 1, dtype=np.int64) * F
    ragged = Case(dev, rows, d, ids.reshape(-1), off, True, seed=1)
    assert np.array_equal(ragged.want.view(np.int32), fixed.want.view(np.int32))
    assert _same(ragged.check("ragged"), got)


# ---- tolerance mode ----------------------------------------------------------------------------------------------------------
def test_tolerance_mode_1_is_the_composed_sequence_in_that_mode(dev):
    B, F, rows, d = 384, 3, 500, 128
    rng = np.random.default_rng(1)
    ids = rng.integers(1, rows + 20, (B, F)).astype(np.float32)
    ids[:, 1] = 0
    case = Case(dev, rows, d, ids, None, True, seed=77)
    exact = case.fused()[1]
    prev = ops.set_tolerance_mode(1)
    try:
        _, comp = case.composed()
        buf, got = case.fused()
        buf_1, one = case.one_call()
    finally:
        ops.set_tolerance_mode(0)
    assert prev is False
    assert _same(got, comp) and _same(one, comp)
    assert case.guards_intact(buf) and case.guards_intact(buf_1)
    assert not _same(comp, exact)                 # the mode took effect: the 384-run is summed by the tree
    assert _same(case.fused()[1], exact)          # back in mode 0


# ---- the Python entry points' checks -------------------------------------------------------------------------------------------
def test_argument_validation(dev):
    case = Case(dev, 50, 4, np.zeros((3, 2), dtype=np.float32), None, True, seed=3)
    _, table = case.fresh_table()
    plan = case.plan()
    with pytest.raises(ValueError):
        ops.sgd_apply_fm_bags(table, plan, case.d_g_sum, case.d_g_fm, case.d_S, LR)                       # neither
    with pytest.raises(ValueError):
        ops.sgd_apply_fm_bags(table, plan, case.d_g_sum, case.d_g_fm, case.d_S, LR, bag=2,
                              bag_of=torch.zeros(6, dtype=torch.int32, device=dev))                       # both
    with pytest.raises(ValueError):
        ops.sgd_apply_fm_bags(table, plan, case.d_g_sum, case.d_g_fm, case.d_S, LR, bag=3)                # 6 ids, 3 bags of 3
    with pytest.raises(ValueError):
        ops.sgd_apply_fm_bags(table, plan, case.d_g_sum, case.d_g_fm[:2], case.d_S, LR, bag=2)            # shapes differ
    with pytest.raises(ValueError):
        ops.sgd_apply_fm_bags(table, plan, case.d_g_sum, table[:3], case.d_S, LR, bag=2)                  # aliases the table
    with pytest.raises(TypeError):
        ops.sgd_apply_fm_bags(table, plan, case.d_g_sum, case.d_g_fm.double(), case.d_S, LR, bag=2)
    with pytest.raises(ValueError):
        ops.sgd_sparse_update_fm_bags(table, case.d_ids[:2], case.d_g_sum, case.d_g_fm, case.d_S, LR)     # 2 bags, 3 rows
    assert _same(table, torch.from_numpy(case.table).to(dev))
    # no ids: nothing happens
    empty = torch.empty((0, 2), dtype=torch.float32, device=dev)
    z = torch.empty((0, 4), dtype=torch.float32, device=dev)
    ops.sgd_sparse_update_fm_bags(table, empty, None, z, z, LR)
    assert _same(table, torch.from_numpy(case.table).to(dev))

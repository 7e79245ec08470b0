"""The weighted bags on the GPU (ha_gather_wsum_*, ha_wbag_grad_rows, ha_sgd_apply_wbags and its one-call forms): every case is
compared bit for bit, over the whole table and between guard rows of a sentinel, with the numpy restatement
(tests/wbag_model.py), with the composed GPU sequence (wbag_grad_rows + sgd_apply on a finished plan), the one-call form with
mask + plan + apply, a plan of the ids with a plan of masked keys, and with the unweighted kernels through the two identities:
all-ones weights are embedding_lookup_sum / sgd_sparse_update_bags, a 0/1 mask is both on the compacted ragged bags.

Shapes and the path each one reaches (kernels as built, csrc/wbag.hip):
  B = 64, F = 26, rows = 997 (1,664 occurrences; the plan's rank-by-counting sort)
      d = 1, 5          forward VEC 1 / 32 rows per round; apply scalar, one 64-column slice, partly live
      d = 16, 64        apply 16-byte path, one chunk (partly live at 16)
      d = 128, 132      forward two and three slices; apply one and two chunks of 256 columns, the second partly live
      d = 512           forward eight slices; apply two chunks; the long path eight slices per listed key
      runs of 1, 2, 3, 4, 15, 16, 17, 47 occurrences: the one-wave path (batches of 8 or 16 loads: one batch, a part, two, more)
      runs of 48, 49, 64 (all ones: the padding column), 384: the workgroup path (120 per round: a part, three rounds and a part)
  B = 2048, F = 3 / 12, d = 128 / 256   forward VEC 2 and VEC 4 (at least 2,048 waves), 8 and 32 rows per round
  ragged bags: empty bags and one bag of 130 ids (three blocks of 64 in the forward)
  1,500 x 26 = 39,000 occurrences at d = 16, fixed and ragged: the masked keys go through the radix planner (> 36,864)."""
import gc
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wbag_model  # noqa: E402

from herald_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu

LR = 0.05
GUARD = 2          # rows in front of and behind the table
SENTINEL = 777.0


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    """What this module created and only the cyclic collector frees (operators that hold their configs, stores, plans) is
    collected here, with the device idle -- not at some later allocation inside another module's gated or timed call, where a
    finalizer that frees device memory would wait for that module's stream."""
    yield
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _values(rng, shape, spread):
    return (rng.standard_normal(shape) * np.exp(rng.uniform(-spread, spread, (shape[0], 1)))).astype(np.float32)


def weights_of(kind, ids, rng):
    """all ones; a 0/1 mask (fixed bags: column 0 dead, the padding column; 40 % of the rest dead); general weights with
    negatives, +0.0, -0.0 and a subnormal among them."""
    if kind == "ones":
        return np.ones(ids.shape, dtype=np.float32)
    if kind == "mask":
        w = (rng.random(ids.shape) >= 0.4).astype(np.float32)
        if ids.ndim == 2:
            w[:, 0] = 0
        return w
    w = rng.standard_normal(ids.shape).astype(np.float32)
    flat = w.reshape(-1)
    pick = rng.permutation(flat.size)
    k = max(flat.size // 10, 3)
    flat[pick[:k]] = np.float32(0.0)
    flat[pick[k:2 * k]] = np.float32(-0.0)
    flat[pick[2 * k:2 * k + 3]] = np.float32(1e-40)
    assert (flat < 0).any() and np.signbit(flat[flat == 0]).any() and not np.signbit(flat[flat == 0]).all()
    return w


class Case:
    """The inputs of one case on the host and the device, and the restatement's results (computed once)."""

    def __init__(self, dev, rows, d, ids, weights, offsets, seed, int64_ids=False, off16=0, table=None, bag_grads=None):
        rng = np.random.default_rng(seed)
        self.dev, self.rows, self.d, self.ids, self.w, self.offsets = dev, rows, d, ids, weights.astype(np.float32), offsets
        self.table = _values(rng, (rows, d), 3) if table is None else table
        self.nbags = ids.shape[0] if offsets is None else offsets.size - 1
        self.bag = ids.shape[1] if offsets is None else None
        self.g = _values(rng, (self.nbags, d), 2) if bag_grads is None else bag_grads
        self.d_ids = torch.from_numpy(ids.astype(np.int64) if int64_ids else ids).to(dev)
        self.d_w = torch.from_numpy(self.w).to(dev)
        self.d_off = torch.from_numpy(offsets).to(dev) if offsets is not None else None
        self.d_g = torch.from_numpy(self.g).to(dev)
        self.off16 = off16
        self._want_sum = self._want = None

    @property
    def want_sum(self):
        if self._want_sum is None:
            self._want_sum = wbag_model.wbag_sum(self.table, self.ids, self.w, self.offsets)
        return self._want_sum

    @property
    def want(self):
        if self._want is None:
            self._want = wbag_model.wbag_sgd(self.table, self.ids, self.w, self.g, LR, self.offsets)
        return self._want

    def fresh_table(self):
        """(buffer, table view): the table between GUARD rows of a sentinel; off16 floats off 16-byte alignment."""
        n = (self.rows + 2 * GUARD) * self.d
        buf = torch.full((n + 4,), SENTINEL, dtype=torch.float32, device=self.dev)
        view = buf[self.off16 + GUARD * self.d:self.off16 + (GUARD + self.rows) * self.d].view(self.rows, self.d)
        view.copy_(torch.from_numpy(self.table))
        return buf, view

    def guards_intact(self, buf):
        lo, hi = self.off16 + GUARD * self.d, self.off16 + (GUARD + self.rows) * self.d
        return bool(torch.all(buf[:lo] == SENTINEL)) and bool(torch.all(buf[hi:] == SENTINEL))

    def bag_args(self):
        if self.offsets is None:
            return dict(bag=self.bag)
        return dict(bag_of=ops.bag_of(self.d_off, self.d_ids.numel()))

    def plan(self, masked=False):
        flat = self.d_ids.reshape(-1)
        if masked:      # the row number of a live occurrence, the key `rows` for a dead one
            keys = flat.to(torch.int64)
            live = (self.d_w.reshape(-1) != 0) & (keys >= 0) & (keys < self.rows)
            flat = torch.where(live, keys, torch.full_like(keys, self.rows))
        return ops.IndexPlan(max(flat.numel(), 1), device=self.dev).sort(flat).finish()

    def forward(self, guarded=False):
        _, table = self.fresh_table()
        if not guarded:
            return ops.embedding_lookup_wsum(table, self.d_ids, self.d_w, offsets=self.d_off)
        buf = torch.full(((self.nbags + 2) * self.d,), SENTINEL, dtype=torch.float32, device=self.dev)
        out = buf[self.d:(self.nbags + 1) * self.d].view(self.nbags, self.d)
        got = ops.embedding_lookup_wsum(table, self.d_ids, self.d_w, offsets=self.d_off, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert bool(torch.all(buf[:self.d] == SENTINEL)) and bool(torch.all(buf[(self.nbags + 1) * self.d:] == SENTINEL))
        return out

    def fused(self, masked=False):
        buf, table = self.fresh_table()
        ops.sgd_apply_wbags(table, self.plan(masked), self.d_g, self.d_w, LR, **self.bag_args())
        return buf, table

    def one_call(self):
        buf, table = self.fresh_table()
        ops.sgd_sparse_update_wbags(table, self.d_ids, self.d_g, self.d_w, LR, offsets=self.d_off)
        return buf, table

    def composed(self):
        """G = wbag_grad_rows(g, w), sgd_apply(table, finished plan of the ids, G)."""
        buf, table = self.fresh_table()
        G = ops.wbag_grad_rows(self.d_g, self.d_w.reshape(-1), **self.bag_args())
        ops.sgd_apply(table, self.plan(), G, LR, finished=True)
        return buf, table, G

    def check(self, what=None, composed=True):
        out = self.forward(guarded=True)
        assert _same(out, torch.from_numpy(self.want_sum).to(self.dev)), ("forward vs restatement", what)
        assert _same(self.forward(), out), ("out= given vs allocated", what)
        want = torch.from_numpy(self.want).to(self.dev)
        buf, got = self.fused()
        assert _same(got, want), ("fused vs restatement", what)
        assert self.guards_intact(buf), what
        buf_m, got_m = self.fused(masked=True)
        assert _same(got_m, got), ("plan of masked keys vs plan of the ids", what)
        assert self.guards_intact(buf_m), what
        buf_1, one = self.one_call()
        assert _same(one, got), ("one call vs mask + plan + apply", what)
        assert self.guards_intact(buf_1), what
        if composed:      # (tables without -0.0 elements: the one corner where the two differ)
            _, comp, G = self.composed()
            assert _same(comp, got), ("fused vs composed", what)
            which = wbag_model.which_bag(self.ids, self.offsets)
            assert _same(G, torch.from_numpy(wbag_model.wbag_grad_rows(self.g, self.w, which)).to(self.dev)), what
        return out, got

    def check_unweighted_identity(self, what=None):
        """All weights 0 or 1: the unweighted kernels on the ragged bags left when the dead occurrences are deleted (all ones:
        on the bags as they are)."""
        assert set(np.unique(self.w).tolist()) <= {0.0, 1.0}
        if (self.w == 1).all():
            d_ids, d_off = self.d_ids, self.d_off
        else:
            cids, coff = wbag_model.compact(self.ids, self.w, self.offsets)
            d_ids = torch.from_numpy(cids.astype(np.int64) if self.d_ids.dtype == torch.int64 else cids).to(self.dev)
            d_off = torch.from_numpy(coff).to(self.dev)
        _, table = self.fresh_table()
        assert _same(self.forward(), ops.embedding_lookup_sum(table, d_ids, offsets=d_off)), ("forward identity", what)
        ops.sgd_sparse_update_bags(table, d_ids, self.d_g, LR, offsets=d_off)
        assert _same(self.fused()[1], table), ("apply identity", what)


# ---- fixed bags ------------------------------------------------------------------------------------------------------------
ROWS = 997
RUNS = [1, 2, 3, 4, 15, 16, 17, 47, 48, 49, 384]
KINDS = ["ones", "mask", "general"]


def _fixed_ids():
    """B = 64 bags of F = 26: column 0 all id 0 (the padding id), key 10 + j exactly RUNS[j] times, the rest from [100, ROWS)
    with three ids >= ROWS mixed in (their weights are not zero in any class but by chance)."""
    B, F = 64, 26
    rng = np.random.default_rng(2025)
    ids = np.empty((B, F), dtype=np.float32)
    ids[:, 0] = 0
    rest = rng.integers(100, ROWS, B * (F - 1)).astype(np.float32)
    forced = np.concatenate([np.full(L, 10 + j, dtype=np.float32) for j, L in enumerate(RUNS)])
    where = rng.permutation(rest.size)[:forced.size + 3]
    rest[where[:forced.size]] = forced
    rest[where[forced.size:]] = [ROWS, ROWS + 5, 1 << 20]
    ids[:, 1:] = rest.reshape(B, F - 1)
    return ids


def _fixed_case(dev, d, kind, **kw):
    ids = _fixed_ids()
    w = weights_of(kind, ids, np.random.default_rng(7 + len(kind)))
    w.reshape(-1)[np.flatnonzero(ids.reshape(-1) >= ROWS)] = 1.5 if kind == "general" else 1.0      # live weights beyond the table
    return Case(dev, ROWS, d, ids, w, None, seed=d, **kw)


def test_the_forced_run_lengths_are_there_with_dead_occurrences_inside():
    ids = _fixed_ids()
    keys, counts = np.unique(ids, return_counts=True)
    got = dict(zip(keys.astype(np.int64).tolist(), counts.tolist()))
    assert got[0] == 64 and all(got[10 + j] == L for j, L in enumerate(RUNS))
    assert sum(c for k, c in got.items() if k >= ROWS) == 3
    for kind in ("mask", "general"):
        w = weights_of(kind, ids, np.random.default_rng(7 + len(kind)))
        for j, L in enumerate(RUNS):
            if L >= 15:      # dead and live occurrences inside every longer run
                sel = w[ids == 10 + j]
                assert (sel == 0).any() and (sel != 0).any(), (kind, L)
    assert (weights_of("mask", ids, np.random.default_rng(11))[:, 0] == 0).all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [1, 5, 16, 64, 128, 132, 512])
def test_fixed_bags_every_run_class(dev, d, kind):
    case = _fixed_case(dev, d, kind)
    _, got = case.check((d, kind))
    if kind != "general":
        case.check_unweighted_identity((d, kind))
    # rows that no live occurrence names keep their bits: unnamed keys, and keys with dead occurrences only
    live = wbag_model.live_mask(ROWS, case.ids, case.w)
    named = np.unique(case.ids.reshape(-1)[live].astype(np.int64))
    rest = torch.from_numpy(np.setdiff1d(np.arange(ROWS), named)).to(dev)
    assert rest.numel() and _same(got[rest], torch.from_numpy(case.table).to(dev)[rest])
    if kind == "mask":      # the padding id: 64 occurrences, all dead
        assert 0 not in named and _same(got[0], torch.from_numpy(case.table[0]).to(dev))


@pytest.mark.parametrize("B,F,d", [(2048, 3, 128), (2048, 12, 128), (2048, 3, 256), (2048, 12, 256)])
def test_forward_16_and_8_byte_slices(dev, B, F, d):
    rows = 300
    rng = np.random.default_rng(B + F + d)
    ids = rng.integers(0, rows + 3, (B, F)).astype(np.float32)
    ids[:, 0] = 0
    for kind in ("mask", "general"):
        case = Case(dev, rows, d, ids, weights_of(kind, ids, rng), None, seed=d + F)
        assert _same(case.forward(guarded=True), torch.from_numpy(case.want_sum).to(dev)), kind
    ones = Case(dev, rows, d, ids, weights_of("ones", ids, rng), None, seed=d + F)
    _, table = ones.fresh_table()
    assert _same(ones.forward(), ops.embedding_lookup_sum(table, ones.d_ids))


def test_a_bag_without_live_occurrence_under_inf_and_nan(dev):
    """Bag 5 has no live occurrence and its gradient row is inf / NaN; the padding row 0 of the table is inf and every bag names
    it with weight 0: outputs and table are finite (but the padding row, which keeps its bits) and equal the restatement."""
    d = 64
    base = _fixed_case(dev, d, "mask")
    w = base.w.copy()
    w[5, :] = [0.0, -0.0] * 13
    table = base.table.copy()
    table[0] = np.inf
    g = base.g.copy()
    g[5, ::3], g[5, 1::3], g[5, 2::3] = np.inf, np.nan, -np.inf
    case = Case(dev, ROWS, d, base.ids, w, None, seed=d, table=table, bag_grads=g)
    out, got = case.check("inf")
    assert bool(torch.isfinite(out).all()) and bool((_bits(out[5]) == 0).all())
    assert bool(torch.isfinite(got[1:]).all()) and _same(got[0], torch.from_numpy(table[0]).to(dev))
    # a key that occurs in bag 5 only keeps its bits
    only = np.setdiff1d(base.ids[5].astype(np.int64), np.delete(base.ids, 5, axis=0).astype(np.int64))
    only = only[only < ROWS]
    assert only.size
    assert _same(got[torch.from_numpy(only).to(dev)], torch.from_numpy(table[only]).to(dev))


def test_int64_ids(dev):
    case = _fixed_case(dev, 64, "general", int64_ids=True)
    case.check("int64")
    off = np.array([0, 40, 40, 100], dtype=np.int64)
    rng = np.random.default_rng(5)
    ids = rng.integers(0, 30, 100).astype(np.float32)
    Case(dev, 25, 12, ids, weights_of("mask", ids, rng), off, seed=65, int64_ids=True).check("int64 ragged")


def test_a_table_view_4_bytes_off_16_byte_alignment(dev):
    case = _fixed_case(dev, 8, "general", off16=1)
    _, view = case.fresh_table()
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    case.check("off16")


# ---- ragged bags -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [5, 64, 260])
def test_ragged_bags_with_empty_bags_and_a_bag_of_130(dev, d, kind):
    n, rows = 600, 120
    off = np.array([0, 0, 10, 37, 37, 37, 167, 231, 600, 600], dtype=np.int64)
    assert 130 in np.diff(off)
    rng = np.random.default_rng(d)
    ids = rng.integers(0, rows + 6, n).astype(np.float32)
    ids[rng.permutation(n)[:60]] = 7                                  # a run of 60 across the bags
    case = Case(dev, rows, d, ids, weights_of(kind, ids, rng), off, seed=d + 1)
    case.check((d, kind))
    if kind != "general":
        case.check_unweighted_identity((d, kind))


# ---- more than 36,864 ids: the masked keys go through the radix planner -----------------------------------------------------
def test_more_than_36864_ids_fixed_and_ragged(dev):
    B, F, rows, d = 1500, 26, 5000, 16
    rng = np.random.default_rng(39000)
    ids = rng.integers(0, rows + 50, (B, F)).astype(np.float32)
    ids[:, 0] = 0                                                     # the padding column, dead
    ids[:, 3] = 17                                                    # the hot column: a run of 1,500
    ids[:, 4] = rng.integers(20, 24, B)                               # and four runs of some 375
    w = weights_of("mask", ids, rng)
    fixed = Case(dev, rows, d, ids, w, None, seed=1)
    assert fixed.d_ids.numel() == 39000 > 36864
    _, got = fixed.check("fixed")
    fixed.check_unweighted_identity("fixed")
    # the same bags given as ragged ones: the same inputs (same seed), the same result, the restatement shared
    off = np.arange(B + 1, dtype=np.int64) * F
    ragged = Case(dev, rows, d, ids.reshape(-1), w.reshape(-1), off, seed=1)
    ragged._want, ragged._want_sum = fixed.want, fixed.want_sum
    assert _same(ragged.check("ragged")[1], got)


# ---- tolerance mode ----------------------------------------------------------------------------------------------------------
def test_tolerance_mode_1_is_the_composed_sequence_in_that_mode(dev):
    case = _fixed_case(dev, 128, "general")
    exact = case.fused()[1]
    prev = ops.set_tolerance_mode(1)
    try:
        _, comp, _ = case.composed()
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
    ids = np.zeros((3, 2), dtype=np.float32)
    case = Case(dev, 50, 4, ids, np.ones((3, 2), np.float32), None, seed=3)
    _, table = case.fresh_table()
    plan = case.plan()
    with pytest.raises(ValueError):
        ops.sgd_apply_wbags(table, plan, case.d_g, case.d_w, LR)                                        # neither
    with pytest.raises(ValueError):
        ops.sgd_apply_wbags(table, plan, case.d_g, case.d_w, LR, bag=2,
                            bag_of=torch.zeros(6, dtype=torch.int32, device=dev))                       # both
    with pytest.raises(ValueError):
        ops.sgd_apply_wbags(table, plan, case.d_g, case.d_w, LR, bag=3)                                 # 6 ids, 3 bags of 3
    with pytest.raises(ValueError):
        ops.sgd_apply_wbags(table, plan, case.d_g, case.d_w.reshape(-1)[:5], LR, bag=2)                 # five weights
    with pytest.raises(ValueError):
        ops.sgd_apply_wbags(table, plan, table[:3], case.d_w, LR, bag=2)                                # aliases the table
    with pytest.raises(TypeError):
        ops.sgd_apply_wbags(table, plan, case.d_g, case.d_w.double(), LR, bag=2)
    with pytest.raises(ValueError):
        ops.sgd_sparse_update_wbags(table, case.d_ids[:2], case.d_g, case.d_w[:2], LR)                  # 2 bags, 3 rows
    with pytest.raises(ValueError):
        ops.embedding_lookup_wsum(table, case.d_ids, case.d_w[:2])
    with pytest.raises(ValueError):
        ops.wbag_grad_rows(case.d_g, case.d_w.reshape(-1), bag=3)
    assert _same(table, torch.from_numpy(case.table).to(dev))
    # no ids: nothing happens
    empty = torch.empty((0, 2), dtype=torch.float32, device=dev)
    ops.sgd_sparse_update_wbags(table, empty, torch.empty((0, 4), dtype=torch.float32, device=dev), empty, LR)
    assert _same(table, torch.from_numpy(case.table).to(dev))
    assert ops.embedding_lookup_wsum(table, empty, empty).shape == (0, 4)

"""The weighted FM-pooled lookup on the GPU (ha_gather_wfm_*, ha_wfm_grad_rows, ha_sgd_apply_wfm_bags and its one-call forms):
every case is compared bit for bit, over the whole table and between guard rows of a sentinel, with the numpy restatement
(tests/wfm_model.py), with the composed GPU sequence (embedding_lookup + wfm_grad_rows + sgd_apply on a finished plan), the
one-call form with mask + plan + apply, a plan of the ids with a plan of masked keys, and with the sibling kernels through the two
identities: S is embedding_lookup_wsum for any weights, and with all-ones weights S and fl(0.5 * fl(fl(S*S) - Q)) are
embedding_lookup_fm's sum and fm.

Shapes and the path each one reaches (kernels as built, csrc/wfm.hip):
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
import special_ids  # noqa: E402
import wbag_model  # noqa: E402
import wfm_model  # noqa: E402

from herald_amd import _lib, ops  # noqa: E402

LR = 0.05
GUARD = 2          # rows in front of and behind the table
SENTINEL = 777.0


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    """What this module created and only the cyclic collector frees is collected here, with the device idle."""
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

    def __init__(self, dev, rows, d, ids, weights, offsets, seed, int64_ids=False, off16=0, table=None, g_sum=None, g_sq=None,
                 d_ids=None):
        rng = np.random.default_rng(seed)
        self.dev, self.rows, self.d, self.ids, self.w, self.offsets = dev, rows, d, ids, weights.astype(np.float32), offsets
        self.table = _values(rng, (rows, d), 3) if table is None else table
        self.nbags = ids.shape[0] if offsets is None else offsets.size - 1
        self.bag = ids.shape[1] if offsets is None else None
        self.gs = _values(rng, (self.nbags, d), 2) if g_sum is None else g_sum
        self.gq = _values(rng, (self.nbags, d), 2) if g_sq is None else g_sq
        self.d_ids = torch.from_numpy(ids.astype(np.int64) if int64_ids else ids).to(dev) if d_ids is None else d_ids
        self.d_w = torch.from_numpy(self.w).to(dev)
        self.d_off = torch.from_numpy(offsets).to(dev) if offsets is not None else None
        self.d_gs, self.d_gq = torch.from_numpy(self.gs).to(dev), torch.from_numpy(self.gq).to(dev)
        self.off16 = off16
        self._want_sq = self._want = None

    @property
    def want_sq(self):
        if self._want_sq is None:
            self._want_sq = wfm_model.wfm_lookup(self.table, self.ids, self.w, self.offsets)
        return self._want_sq

    @property
    def want(self):
        if self._want is None:
            self._want = wfm_model.wfm_sgd(self.table, self.ids, self.w, self.gs, self.gq, LR, self.offsets)
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
            keys = torch.from_numpy(special_ids.rows_of(self.ids)).to(self.dev)
            live = (self.d_w.reshape(-1) != 0) & (keys < self.rows)
            flat = torch.where(live, keys, torch.full_like(keys, self.rows))
        return ops.IndexPlan(max(flat.numel(), 1), device=self.dev).sort(flat).finish()

    def forward(self, guarded=False):
        _, table = self.fresh_table()
        if not guarded:
            return ops.embedding_lookup_wfm(table, self.d_ids, self.d_w, offsets=self.d_off)
        m = self.nbags * self.d
        buf = torch.full((3 * self.d + 2 * m,), SENTINEL, dtype=torch.float32, device=self.dev)
        out_s = buf[self.d:self.d + m].view(self.nbags, self.d)
        out_q = buf[2 * self.d + m:2 * self.d + 2 * m].view(self.nbags, self.d)
        S, Q = ops.embedding_lookup_wfm(table, self.d_ids, self.d_w, offsets=self.d_off, sum_out=out_s, sq_out=out_q)
        assert S.data_ptr() == out_s.data_ptr() and Q.data_ptr() == out_q.data_ptr()
        for lo, hi in ((0, self.d), (self.d + m, 2 * self.d + m), (2 * self.d + 2 * m, 3 * self.d + 2 * m)):
            assert bool(torch.all(buf[lo:hi] == SENTINEL)), (lo, hi)
        return out_s, out_q

    def fused(self, masked=False):
        buf, table = self.fresh_table()
        ops.sgd_apply_wfm_bags(table, self.plan(masked), self.d_gs, self.d_gq, self.d_w, LR, **self.bag_args())
        return buf, table

    def one_call(self):
        buf, table = self.fresh_table()
        ops.sgd_sparse_update_wfm_bags(table, self.d_ids, self.d_gs, self.d_gq, self.d_w, LR, offsets=self.d_off)
        return buf, table

    def composed(self):
        """E = embedding_lookup(table, ids), G = wfm_grad_rows(g_S, g_Q, w, E), sgd_apply(table, finished plan of the ids, G)."""
        buf, table = self.fresh_table()
        E = ops.embedding_lookup(table, self.d_ids.reshape(-1))
        G = ops.wfm_grad_rows(self.d_gs, self.d_gq, self.d_w.reshape(-1), E, **self.bag_args())
        in_place = ops.wfm_grad_rows(self.d_gs, self.d_gq, self.d_w.reshape(-1), E, out=E, **self.bag_args())
        assert in_place.data_ptr() == E.data_ptr()
        ops.sgd_apply(table, self.plan(), G, LR, finished=True)
        return buf, table, G, in_place

    def check(self, what=None, composed=True):
        S, Q = self.forward(guarded=True)
        assert _same(S, torch.from_numpy(self.want_sq[0]).to(self.dev)), ("S vs restatement", what)
        assert _same(Q, torch.from_numpy(self.want_sq[1]).to(self.dev)), ("Q vs restatement", what)
        S2, Q2 = self.forward()
        assert _same(S2, S) and _same(Q2, Q), ("out= given vs allocated", what)
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
            _, comp, G, in_place = self.composed()
            assert _same(comp, got), ("fused vs composed", what)
            assert _same(in_place, G), ("wfm_grad_rows in place vs out of place", what)
            which = wbag_model.which_bag(self.ids, self.offsets)
            E = wfm_model.gather(self.table, self.ids)
            assert _same(G, torch.from_numpy(wfm_model.wfm_grad_rows(self.gs, self.gq, self.w, E, which)).to(self.dev)), what
        return S, Q, got

    def check_identities(self, what=None):
        """S is embedding_lookup_wsum for any weights; all ones: S and fl(0.5 * fl(fl(S*S) - Q)), formed by separate torch ops,
        are embedding_lookup_fm(want_rows=False)'s sum and fm."""
        _, table = self.fresh_table()
        S, Q = self.forward()
        assert _same(S, ops.embedding_lookup_wsum(table, self.d_ids, self.d_w, offsets=self.d_off)), ("S is wsum", what)
        if (self.w == 1).all():
            _, fm_S, fm = ops.embedding_lookup_fm(table, self.d_ids, offsets=self.d_off, want_rows=False)
            sq = torch.mul(S, S)
            diff = torch.sub(sq, Q)
            assert _same(S, fm_S) and _same(torch.mul(diff, 0.5), fm), ("all ones: the FM lookup", what)


# ---- fixed bags ------------------------------------------------------------------------------------------------------------
ROWS = 997
RUNS = [1, 2, 3, 4, 15, 16, 17, 47, 48, 49, 384]
KINDS = ["ones", "mask", "general"]


def _fixed_ids():
    """B = 64 bags of F = 26: column 0 all id 0 (the padding id), key 10 + j exactly RUNS[j] times, the rest from [100, ROWS)
    with three ids >= ROWS mixed in (their weights are not zero in any class)."""
    B, F = 64, 26
    rng = np.random.default_rng(2026)
    ids = np.empty((B, F), dtype=np.float32)
    ids[:, 0] = 0
    rest = rng.integers(100, ROWS, B * (F - 1)).astype(np.float32)
    forced = np.concatenate([np.full(L, 10 + j, dtype=np.float32) for j, L in enumerate(RUNS)])
    where = rng.permutation(rest.size)[:forced.size + 3]
    rest[where[:forced.size]] = forced
    rest[where[forced.size:]] = [ROWS, ROWS + 5, 1 << 20]
    ids[:, 1:] = rest.reshape(B, F - 1)
    return ids


def _fixed_weights(kind, ids):
    w = weights_of(kind, ids, np.random.default_rng(7 + len(kind)))
    w.reshape(-1)[np.flatnonzero(ids.reshape(-1) >= ROWS)] = 1.5 if kind == "general" else 1.0      # live weights beyond the table
    return w


def _fixed_case(dev, d, kind, **kw):
    ids = _fixed_ids()
    return Case(dev, ROWS, d, ids, _fixed_weights(kind, ids), None, seed=d, **kw)


def test_the_forced_run_lengths_are_there_with_dead_occurrences_inside():
    """CPU only: what the fixed-bag cases below rely on is true of their inputs."""
    ids = _fixed_ids()
    keys, counts = np.unique(ids, return_counts=True)
    got = dict(zip(keys.astype(np.int64).tolist(), counts.tolist()))
    assert got[0] == 64 and all(got[10 + j] == L for j, L in enumerate(RUNS))
    assert sum(c for k, c in got.items() if k >= ROWS) == 3
    for kind in KINDS:
        w = _fixed_weights(kind, ids)
        assert (w[ids >= ROWS] != 0).all() and np.count_nonzero(ids >= ROWS) == 3, kind
        if kind == "ones":
            continue
        for j, L in enumerate(RUNS):
            if L >= 15:      # dead and live occurrences inside every longer run
                sel = w[ids == 10 + j]
                assert (sel == 0).any() and (sel != 0).any(), (kind, L)
    assert (_fixed_weights("mask", ids)[:, 0] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [1, 5, 16, 64, 128, 132, 512])
def test_fixed_bags_every_run_class(dev, d, kind):
    case = _fixed_case(dev, d, kind)
    _, _, got = case.check((d, kind))
    case.check_identities((d, kind))
    # rows that no live occurrence names keep their bits: unnamed keys, and keys with dead occurrences only
    live = wbag_model.live_mask(ROWS, case.ids, case.w)
    named = np.unique(case.ids.reshape(-1)[live].astype(np.int64))
    rest = torch.from_numpy(np.setdiff1d(np.arange(ROWS), named)).to(dev)
    assert rest.numel() and _same(got[rest], torch.from_numpy(case.table).to(dev)[rest])
    changed = torch.from_numpy(named).to(dev)
    assert not _same(got[changed], torch.from_numpy(case.table).to(dev)[changed])
    if kind == "mask":      # the padding id: 64 occurrences, all dead
        assert 0 not in named and _same(got[0], torch.from_numpy(case.table[0]).to(dev))


@pytest.mark.gpu
@pytest.mark.parametrize("B,F,d", [(2048, 3, 128), (2048, 12, 128), (2048, 3, 256), (2048, 12, 256)])
def test_forward_16_and_8_byte_slices(dev, B, F, d):
    rows = 300
    rng = np.random.default_rng(B + F + d)
    ids = rng.integers(0, rows + 3, (B, F)).astype(np.float32)
    ids[:, 0] = 0
    for kind in ("mask", "general"):
        case = Case(dev, rows, d, ids, weights_of(kind, ids, rng), None, seed=d + F)
        S, Q = case.forward(guarded=True)
        assert _same(S, torch.from_numpy(case.want_sq[0]).to(dev)) and _same(Q, torch.from_numpy(case.want_sq[1]).to(dev)), kind
        case.check_identities(kind)
    Case(dev, rows, d, ids, weights_of("ones", ids, rng), None, seed=d + F).check_identities("ones")


@pytest.mark.gpu
def test_a_bag_without_live_occurrence_under_inf_and_nan(dev):
    """Bag 5 has no live occurrence and both its gradient rows are inf / NaN; the padding row 0 of the table is inf and every bag
    names it with weight 0: S = Q = +0 for bag 5, outputs and table are finite (but the padding row, which keeps its bits)."""
    d = 64
    base = _fixed_case(dev, d, "mask")
    w = base.w.copy()
    w[5, :] = [0.0, -0.0] * 13
    table = base.table.copy()
    table[0] = np.inf
    gs, gq = base.gs.copy(), base.gq.copy()
    gs[5, ::3], gs[5, 1::3], gs[5, 2::3] = np.inf, np.nan, -np.inf
    gq[5, ::3], gq[5, 1::3], gq[5, 2::3] = np.nan, -np.inf, np.inf
    case = Case(dev, ROWS, d, base.ids, w, None, seed=d, table=table, g_sum=gs, g_sq=gq)
    S, Q, got = case.check("inf")
    assert bool(torch.isfinite(S).all()) and bool(torch.isfinite(Q).all())
    assert bool((_bits(S[5]) == 0).all()) and bool((_bits(Q[5]) == 0).all())
    assert bool(torch.isfinite(got[1:]).all()) and _same(got[0], torch.from_numpy(table[0]).to(dev))
    only = np.setdiff1d(base.ids[5].astype(np.int64), np.delete(base.ids, 5, axis=0).astype(np.int64))
    only = only[only < ROWS]
    assert only.size
    assert _same(got[torch.from_numpy(only).to(dev)], torch.from_numpy(table[only]).to(dev))


@pytest.mark.gpu
def test_int64_ids(dev):
    _fixed_case(dev, 64, "general", int64_ids=True).check("int64")
    off = np.array([0, 40, 40, 100], dtype=np.int64)
    rng = np.random.default_rng(5)
    ids = rng.integers(0, 30, 100).astype(np.float32)
    Case(dev, 25, 12, ids, weights_of("mask", ids, rng), off, seed=65, int64_ids=True).check("int64 ragged")


@pytest.mark.gpu
def test_a_table_view_4_bytes_off_16_byte_alignment(dev):
    case = _fixed_case(dev, 8, "general", off16=1)
    _, view = case.fresh_table()
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    case.check("off16")


@pytest.mark.gpu
@pytest.mark.parametrize("int64_ids", [False, True], ids=["f32", "i64"])
def test_the_special_ids_are_dead_with_live_weights(dev, int64_ids):
    """Negative, NaN, infinite and >= 2^32 ids with weight 1.5 take no part in forward or apply; the live ones of the list do."""
    rows, d = 37, 8
    spec = special_ids.int_specials(rows) if int64_ids else special_ids.float_specials(rows)
    vals = [s[0] for s in spec]
    n = 3 * ((len(vals) + 5 + 2) // 3)
    if int64_ids:
        ids = np.array(vals + [5, 6, 7, 8, 9] + [1] * (n - len(vals) - 5), dtype=np.int64).reshape(-1, 3)
        d_ids = torch.from_numpy(ids).to(dev)
    else:
        ids = np.array(vals + [5, 6, 7, 8, 9] + [1] * (n - len(vals) - 5), dtype=np.float32).reshape(-1, 3)
        d_ids = torch.from_numpy(ids).to(dev)
    w = np.full(ids.shape, 1.5, dtype=np.float32)
    case = Case(dev, rows, d, ids, w, None, seed=77, d_ids=d_ids)
    keys = special_ids.keys_of(ids)
    assert (keys >= rows).sum() >= len(vals) - 5 and (keys < rows).sum() >= 6
    _, _, got = case.check("specials")
    untouched = np.setdiff1d(np.arange(rows), keys[keys < rows].astype(np.int64))
    assert _same(got[torch.from_numpy(untouched).to(dev)], torch.from_numpy(case.table[untouched]).to(dev))
    assert not _same(got[rows - 1], torch.from_numpy(case.table[rows - 1]).to(dev))


# ---- ragged bags -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
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
    case.check_identities((d, kind))


# ---- more than 36,864 ids: the masked keys go through the radix planner -----------------------------------------------------
@pytest.mark.gpu
def test_more_than_36864_ids_fixed_and_ragged(dev):
    B, F, rows, d = 1500, 26, 5000, 16
    rng = np.random.default_rng(39001)
    ids = rng.integers(0, rows + 50, (B, F)).astype(np.float32)
    ids[:, 0] = 0                                                     # the padding column, dead
    ids[:, 3] = 17                                                    # the hot column: a run of 1,500
    ids[:, 4] = rng.integers(20, 24, B)                               # and four runs of some 375
    w = weights_of("mask", ids, rng)
    fixed = Case(dev, rows, d, ids, w, None, seed=1)
    assert fixed.d_ids.numel() == 39000 > 36864
    _, _, got = fixed.check("fixed")
    # the same bags given as ragged ones: the same inputs (same seed), the same result, the restatement shared
    off = np.arange(B + 1, dtype=np.int64) * F
    ragged = Case(dev, rows, d, ids.reshape(-1), w.reshape(-1), off, seed=1)
    ragged._want, ragged._want_sq = fixed.want, fixed.want_sq
    assert _same(ragged.check("ragged")[2], got)


# ---- tolerance mode ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_tolerance_mode_1_is_the_composed_sequence_in_that_mode(dev):
    case = _fixed_case(dev, 128, "general")
    exact = case.fused()[1]
    prev = ops.set_tolerance_mode(1)
    try:
        _, comp, _, _ = case.composed()
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
@pytest.mark.gpu
def test_argument_validation(dev):
    ids = np.zeros((3, 2), dtype=np.float32)
    case = Case(dev, 50, 4, ids, np.ones((3, 2), np.float32), None, seed=3)
    _, table = case.fresh_table()
    plan = case.plan()
    gs, gq, w = case.d_gs, case.d_gq, case.d_w
    with pytest.raises(ValueError):
        ops.sgd_apply_wfm_bags(table, plan, gs, gq, w, LR)                                              # neither
    with pytest.raises(ValueError):
        ops.sgd_apply_wfm_bags(table, plan, gs, gq, w, LR, bag=2, bag_of=torch.zeros(6, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        ops.sgd_apply_wfm_bags(table, plan, gs, gq, w, LR, bag=3)                                       # 6 ids, 3 bags of 3
    with pytest.raises(ValueError):
        ops.sgd_apply_wfm_bags(table, plan, gs, gq, w.reshape(-1)[:5], LR, bag=2)                       # five weights
    with pytest.raises(ValueError):
        ops.sgd_apply_wfm_bags(table, plan, table[:3], gq, w, LR, bag=2)                                # aliases the table
    with pytest.raises(ValueError):
        ops.sgd_apply_wfm_bags(table, plan, gs, table[:3], w, LR, bag=2)
    with pytest.raises(ValueError):
        ops.sgd_apply_wfm_bags(table, plan, gs, gq[:2], w, LR, bag=2)                                   # g_sq shaped otherwise
    with pytest.raises(TypeError):
        ops.sgd_apply_wfm_bags(table, plan, gs, gq, w.double(), LR, bag=2)
    with pytest.raises(TypeError):
        ops.sgd_apply_wfm_bags(table, plan, gs, gq.double(), w, LR, bag=2)
    with pytest.raises(ValueError):
        ops.sgd_sparse_update_wfm_bags(table, case.d_ids[:2], gs, gq, w[:2], LR)                        # 2 bags, 3 rows
    with pytest.raises(ValueError):
        ops.embedding_lookup_wfm(table, case.d_ids, w[:2])
    with pytest.raises(ValueError):
        ops.embedding_lookup_wfm(table, case.d_ids, w, sq_out=torch.empty((2, 4), dtype=torch.float32, device=dev))
    E = ops.embedding_lookup(table, case.d_ids.reshape(-1))
    with pytest.raises(ValueError):
        ops.wfm_grad_rows(gs, gq, w.reshape(-1), E, bag=3)
    with pytest.raises(ValueError):
        ops.wfm_grad_rows(gs, gq, w.reshape(-1), E[:, :3].contiguous(), bag=2)
    gs6 = gs.repeat(2, 1)
    with pytest.raises(_lib.HeraldAmdError, match="ha_wfm_grad_rows"):
        ops.wfm_grad_rows(gs6, gq.repeat(2, 1), w.reshape(-1), E, out=gs6, bag=1)                       # out is g_sum
    assert _same(table, torch.from_numpy(case.table).to(dev))
    # no ids: nothing happens
    empty = torch.empty((0, 2), dtype=torch.float32, device=dev)
    none = torch.empty((0, 4), dtype=torch.float32, device=dev)
    ops.sgd_sparse_update_wfm_bags(table, empty, none, none.clone(), empty, LR)
    assert _same(table, torch.from_numpy(case.table).to(dev))
    S, Q = ops.embedding_lookup_wfm(table, empty, empty)
    assert S.shape == (0, 4) and Q.shape == (0, 4)

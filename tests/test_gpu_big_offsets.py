"""Every row-addressing kernel that the full-scale file does not reach, on tables whose row offsets pass 32 bits: T128
(33,762,577 x 128: byte offsets pass 2^32 from key 2^23, float offsets 2^31 from 2^24 and 2^32 from 2^25), T130 (the same rows
x 130: the scalar path) and T1 ((2^30 + 2^16) x 1: the first-order table of the DeepFM models), three views of ONE allocation
that is never filled.

Method (tests/test_gpu_fullscale.py's: the oracle never sees the big table).  Per call: the rows the batch touches get random
values, the ALIAS ranges of those rows -- where a 32-bit float or byte offset would land, tests/big_offsets.py -- and a handful
of sentinel rows (row 0 among them: dead ids are clamped to it) get a poison pattern; the project's numpy model of the call runs
on the compact table of the touched rows with the ids remapped by searchsorted; outputs and touched rows are compared under the
rule of the call's small-table test (bit for bit everywhere; the optimizers' row kernel also against float64 as
tests/test_gpu_optim_paths.py judges it), and alias ranges and sentinels must hold, bit for bit, what was written.  A kernel
that wraps an offset reads poison (the output differs) or writes into poison (the poison changes and the true row stays stale).
tests/test_big_offsets_cpu.py holds the batches to what this relies on."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bag_model  # noqa: E402
import big_offsets as bo  # noqa: E402
import fm_model  # noqa: E402
import fm_pooled_model  # noqa: E402
import wbag_model  # noqa: E402
import wfm_model  # noqa: E402
import wshard_model  # noqa: E402

from herald_amd import ops  # noqa: E402
from oracle import cpu  # noqa: E402
from oracle import optim_ref64 as ref64  # noqa: E402
from test_optim_oracle import HYPER, bound_units, named_part, step32, step64  # noqa: E402

pytestmark = pytest.mark.gpu

GIB = 1 << 30
MARGIN = 8 * GIB
LR = 0.05
HYPER3 = dict(lr=HYPER["lr"], eps=HYPER["eps"], beta1=HYPER["beta1"], beta2=HYPER["beta2"], beta1t=HYPER["beta1"] ** 3,
              beta2t=HYPER["beta2"] ** 3, weight_decay=HYPER["weight_decay"])


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what):
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=what)


def _need(dev, nbytes):
    free, _ = torch.cuda.mem_get_info(dev)
    if free < nbytes + MARGIN:
        pytest.skip("needs %.1f GiB of free HBM, %.1f are free" % ((nbytes + MARGIN) / GIB, free / GIB))


@functools.lru_cache(maxsize=None)
def case_of(table, dtype="f32", layout="fixed", weighted=False, big=False):
    c = bo.make_case(table, dtype, layout, weighted, big)
    bo.check_case(c)
    return c


# ---- the tables ---------------------------------------------------------------------------------------------------------------
class Arena:
    """One uninitialised buffer of T130's size; T128, T130 and T1 are views of its head."""

    def __init__(self, dev, zero=False):
        self.buf = (torch.zeros if zero else torch.empty)(bo.T130.numel, dtype=torch.float32, device=dev)

    def view(self, t):
        return self.buf[:t.numel].view(t.rows, t.width)


@pytest.fixture(scope="module")
def arena(dev):
    _need(dev, bo.T130.numel * 4)
    a = Arena(dev)
    assert a.view(bo.T128).data_ptr() % 16 == 0
    yield a
    del a
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def states(dev, arena):
    """The optimizer state tables: two uninitialised ones and the momentum velocity, zeroed whole by one memset (the dense
    phase reads all of it)."""
    _need(dev, 3 * bo.T130.numel * 4)
    s = {"s1": Arena(dev), "s2": Arena(dev), "velocity": Arena(dev, zero=True)}
    yield s
    s.clear()
    torch.cuda.empty_cache()


class Guard:
    """One view of a table under one case: write() gives the touched rows their values and poisons the alias ranges and the
    sentinel rows; check() compares the touched rows with the model's and finds the poison as it was written."""

    def __init__(self, view, case, dev, poison=True):
        t = case.table
        self.view, self.case, self.flat = view, case, view.view(-1)
        self.keys = torch.from_numpy(case.keys).to(dev)
        self.sent = torch.from_numpy(case.sentinels).to(dev)
        al = case.aliases
        idx = al[:, None] + np.arange(t.width, dtype=np.int64)[None, :]
        self.alias_idx = torch.from_numpy(idx).to(dev)
        if poison:      # exact float32 values; an alias element's is a function of its offset (T130's ranges may overlap)
            self.sent_vals = (3e6 + 1000.0 * np.arange(case.sentinels.size)[:, None] + np.arange(t.width)[None, :]).astype(np.float32)
            self.alias_vals = -(4e6 + idx % 4000000).astype(np.float32)
        else:           # (the momentum velocity: zero everywhere but the touched rows)
            self.sent_vals = np.zeros((case.sentinels.size, t.width), np.float32)
            self.alias_vals = np.zeros((al.size, t.width), np.float32)

    def write(self, values):
        """values [keys.size, width] -> the touched rows; poison -> alias ranges and sentinels.  Returns the compact table: the
        row of key 0 (the dead slot of a weighted case) is the sentinel's."""
        case, t = self.case, self.case.table
        compact = np.ascontiguousarray(values, dtype=np.float32).copy()
        assert compact.shape == (case.keys.size, t.width)
        if case.keys[0] == 0:
            compact[0] = self.sent_vals[0]
        dev = self.keys.device
        self.view[self.keys] = torch.from_numpy(compact).to(dev)
        self.flat[self.alias_idx] = torch.from_numpy(self.alias_vals).to(dev)
        self.view[self.sent] = torch.from_numpy(self.sent_vals).to(dev)
        # the harness itself: read back through indexing, and the last row through a plain slice of the buffer
        _same(self.view[self.keys], compact, "rows as written")
        last = t.last_row(case.dtype)
        _same(self.flat[last * t.width:(last + 1) * t.width], compact[np.searchsorted(case.keys, last)], "the last row, by slice")
        self.check(None, "as written")
        return compact

    def check(self, want, what):
        if want is not None:
            got = self.view[self.keys].cpu().numpy()
            _same(got, want, "%s: touched rows" % what)
        _same(self.flat[self.alias_idx], self.alias_vals, "%s: alias ranges (where a 32-bit offset lands)" % what)
        _same(self.view[self.sent], self.sent_vals, "%s: sentinel rows, row 0 first" % what)


def _rows(case, seed, scale=1.0):
    rng = np.random.default_rng([seed, case.keys.size])
    return rng.standard_normal((case.keys.size, case.table.width), dtype=np.float32) * np.float32(scale)


def _dev_inputs(case, dev):
    d_ids = torch.from_numpy(case.ids).to(dev)
    d_off = torch.from_numpy(case.offsets).to(dev) if case.offsets is not None else None
    d_w = torch.from_numpy(case.weights.reshape(case.ids.shape)).to(dev) if case.weights is not None else None
    return d_ids, d_off, d_w


def _bag_grads(case, seed, count=1):
    rng = np.random.default_rng([seed, 77])
    g = [rng.standard_normal((case.nbags, case.table.width), dtype=np.float32) for _ in range(count)]
    return g[0] if count == 1 else g


def _weights(case):
    return case.weights.reshape(case.ids.shape)


TABLES_ALL = ["T128", "T130", "T1"]
TABLES_WIDE = ["T128", "T130"]
DTYPES = ["f32", "i64"]
LAYOUTS = ["fixed", "ragged"]


def test_the_cases_hold_what_this_file_relies_on():
    """tests/test_big_offsets_cpu.py asserts it for every case; here once more for the ones below, on the GPU machine."""
    for t in TABLES_ALL:
        for dt in DTYPES:
            for lay in LAYOUTS:
                for w in (False, True):
                    case_of(t, dt, lay, w)
    for t in TABLES_WIDE:
        for w in (False, True):
            assert case_of(t, "f32", "fixed", w, True).n > 36864


# ---- ops, forward -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("table", TABLES_ALL)
def test_embedding_lookup(dev, arena, table, dtype):
    """csrc/gather.hip: gather_vec4 (T128), gather_scalar (T130, T1)."""
    case = case_of(table, dtype)
    g = Guard(arena.view(case.table), case, dev)
    compact = g.write(_rows(case, 1))
    d_ids, _, _ = _dev_inputs(case, dev)
    out = ops.embedding_lookup(g.view, d_ids)
    torch.cuda.synchronize()
    assert out.shape == case.ids.shape + (case.table.width,)
    _same(out.reshape(case.n, -1), wfm_model.gather(compact, case.compact_ids()), "rows")
    g.check(compact, "embedding_lookup")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("table", TABLES_ALL)
def test_embedding_lookup_sum(dev, arena, table, dtype, layout):
    """csrc/bagsum.hip bag_sum_kernel: (ok ? r : 0) * width in 64 bits, split into two 32-bit halves for readlane."""
    case = case_of(table, dtype, layout)
    g = Guard(arena.view(case.table), case, dev)
    compact = g.write(_rows(case, 2))
    d_ids, d_off, _ = _dev_inputs(case, dev)
    out = ops.embedding_lookup_sum(g.view, d_ids, offsets=d_off)
    torch.cuda.synchronize()
    _same(out, bag_model.bag_sum(compact, case.compact_ids(), case.offsets), "pooled rows")
    assert np.any(_bits(out))
    g.check(compact, "embedding_lookup_sum")


@pytest.mark.parametrize("want_rows", [True, False], ids=["rows", "norows"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("table", TABLES_WIDE)
def test_embedding_lookup_fm(dev, arena, table, dtype, layout, want_rows):
    """csrc/bagsum.hip bag_fm_kernel."""
    case = case_of(table, dtype, layout)
    g = Guard(arena.view(case.table), case, dev)
    compact = g.write(_rows(case, 3))
    d_ids, d_off, _ = _dev_inputs(case, dev)
    rows, s, fm = ops.embedding_lookup_fm(g.view, d_ids, offsets=d_off, want_rows=want_rows)
    torch.cuda.synchronize()
    w_rows, covered, w_s, w_fm = fm_model.fm_lookup(compact, case.compact_ids(), case.offsets)
    _same(s, w_s, "sum")
    _same(fm, w_fm, "fm")
    if want_rows:
        _same(rows.reshape(case.n, -1)[torch.from_numpy(covered).to(dev)], w_rows[covered], "rows")
    else:
        assert rows is None
    g.check(compact, "embedding_lookup_fm")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("table", TABLES_ALL)
def test_embedding_lookup_wsum(dev, arena, table, dtype, layout):
    """csrc/wbag_dev.h wbag_sum_kernel; the dead slots of the mask sit on id 0."""
    case = case_of(table, dtype, layout, True)
    g = Guard(arena.view(case.table), case, dev)
    compact = g.write(_rows(case, 4))
    d_ids, d_off, d_w = _dev_inputs(case, dev)
    out = ops.embedding_lookup_wsum(g.view, d_ids, d_w, offsets=d_off)
    torch.cuda.synchronize()
    _same(out, wbag_model.wbag_sum(compact, case.compact_ids(), _weights(case), case.offsets), "pooled rows")
    g.check(compact, "embedding_lookup_wsum")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("table", TABLES_WIDE)
def test_embedding_lookup_wfm(dev, arena, table, dtype, layout):
    """csrc/wfm.hip wfm_sum_kernel."""
    case = case_of(table, dtype, layout, True)
    g = Guard(arena.view(case.table), case, dev)
    compact = g.write(_rows(case, 5))
    d_ids, d_off, d_w = _dev_inputs(case, dev)
    s, q = ops.embedding_lookup_wfm(g.view, d_ids, d_w, offsets=d_off)
    torch.cuda.synchronize()
    w_s, w_q = wfm_model.wfm_lookup(compact, case.compact_ids(), _weights(case), case.offsets)
    _same(s, w_s, "S")
    _same(q, w_q, "Q")
    g.check(compact, "embedding_lookup_wfm")


# ---- ops, SGD -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("big", [False, True], ids=["1664ids", "36894ids"])
@pytest.mark.parametrize("table", TABLES_WIDE)
def test_sgd_sparse_update(dev, arena, table, big):
    """csrc/scatter.hip / scatter_dev.h, kModeSgd: by sorted position, and by unique key beyond 36,864 ids."""
    case = case_of(table, "f32", "fixed", False, big)
    g = Guard(arena.view(case.table), case, dev)
    compact = g.write(_rows(case, 6))
    grads = np.random.default_rng(60).standard_normal((case.n, case.table.width), dtype=np.float32)
    d_ids, _, _ = _dev_inputs(case, dev)
    ops.sgd_sparse_update(g.view, d_ids.reshape(-1), torch.from_numpy(grads).to(dev), LR)
    torch.cuda.synchronize()
    want = wbag_model.sgd_rows(compact, case.compact_ids().reshape(-1), grads, LR)
    assert not np.array_equal(want, compact)
    g.check(want, "sgd_sparse_update")


def _bag_kw(case, d_off, dev):
    return dict(bag=case.bag) if case.offsets is None else dict(bag_of=ops.bag_of(d_off, case.n))


WBAG_CASES = [(t, dt, lay, False) for t in TABLES_WIDE for dt in DTYPES for lay in LAYOUTS] + \
             [(t, "f32", "fixed", True) for t in TABLES_WIDE]
WBAG_IDS = ["%s-%s-%s%s" % (t, dt, lay, "-36894ids" if big else "") for t, dt, lay, big in WBAG_CASES]


BAG_CASES = [(t, dt, lay, False) for t in TABLES_ALL for dt in DTYPES for lay in LAYOUTS] + \
            [(t, "f32", "fixed", True) for t in TABLES_WIDE]
BAG_IDS = ["%s-%s-%s%s" % (t, dt, lay, "-36894ids" if big else "") for t, dt, lay, big in BAG_CASES]


@pytest.mark.parametrize("table,dtype,layout,big", BAG_CASES, ids=BAG_IDS)
def test_sgd_sparse_update_bags_and_apply_bags(dev, arena, table, dtype, layout, big):
    """The BAGS instantiations of the apply (scatter.hip / scatter_dev.h): the one-call form, then sgd_apply_bags on a finished
    plan, from the same rows."""
    case = case_of(table, dtype, layout, False, big)
    g = Guard(arena.view(case.table), case, dev)
    bg = _bag_grads(case, 7)
    d_ids, d_off, _ = _dev_inputs(case, dev)
    d_bg = torch.from_numpy(bg).to(dev)
    want = None
    for form in ("one call", "finished plan"):
        compact = g.write(_rows(case, 7))
        if form == "one call":
            ops.sgd_sparse_update_bags(g.view, d_ids, d_bg, LR, offsets=d_off)
        else:
            plan = ops.IndexPlan(case.n, dev).build(d_ids.reshape(-1))
            ops.sgd_apply_bags(g.view, plan, d_bg, LR, **_bag_kw(case, d_off, dev))
        torch.cuda.synchronize()
        if want is None:
            want = bag_model.sgd_bags(compact, case.compact_ids(), bg, LR, case.offsets)
            assert not np.array_equal(want, compact)
        g.check(want, "sgd bags, " + form)


@pytest.mark.parametrize("table,dtype,layout,big", WBAG_CASES, ids=WBAG_IDS)
def test_sgd_sparse_update_fm_bags(dev, arena, table, dtype, layout, big):
    """csrc/fmapply.hip: table + uint64(key) * width row bases; float32 cases hand over g_sum, int64 ones none."""
    case = case_of(table, dtype, layout, False, big)
    g = Guard(arena.view(case.table), case, dev)
    compact = g.write(_rows(case, 8))
    cid = case.compact_ids()
    _, _, s, _ = fm_model.fm_lookup(compact, cid, case.offsets)
    g_sum, g_fm = _bag_grads(case, 8, 2)
    if dtype == "i64":
        g_sum = None
    d_ids, d_off, _ = _dev_inputs(case, dev)
    ops.sgd_sparse_update_fm_bags(g.view, d_ids, torch.from_numpy(g_sum).to(dev) if g_sum is not None else None,
                                  torch.from_numpy(g_fm).to(dev), torch.from_numpy(s).to(dev), LR, offsets=d_off)
    torch.cuda.synchronize()
    want = fm_pooled_model.fm_pooled_sgd(compact, cid, g_sum, g_fm, s, LR, case.offsets)
    assert not np.array_equal(want, compact)
    g.check(want, "sgd_sparse_update_fm_bags")


@pytest.mark.parametrize("table,dtype,layout,big", WBAG_CASES, ids=WBAG_IDS)
def test_sgd_sparse_update_wbags(dev, arena, table, dtype, layout, big):
    """csrc/wbag.hip: the readlane-broadcast bag offsets and table + uint64(key) * width."""
    case = case_of(table, dtype, layout, True, big)
    g = Guard(arena.view(case.table), case, dev)
    compact = g.write(_rows(case, 9))
    bg = _bag_grads(case, 9)
    d_ids, d_off, d_w = _dev_inputs(case, dev)
    ops.sgd_sparse_update_wbags(g.view, d_ids, torch.from_numpy(bg).to(dev), d_w, LR, offsets=d_off)
    torch.cuda.synchronize()
    want = wbag_model.wbag_sgd(compact, case.compact_ids(), _weights(case), bg, LR, case.offsets)
    assert not np.array_equal(want, compact)
    g.check(want, "sgd_sparse_update_wbags")


@pytest.mark.parametrize("table,dtype,layout,big", WBAG_CASES, ids=WBAG_IDS)
def test_sgd_sparse_update_wfm_bags(dev, arena, table, dtype, layout, big):
    """csrc/wfm.hip, the apply half."""
    case = case_of(table, dtype, layout, True, big)
    g = Guard(arena.view(case.table), case, dev)
    compact = g.write(_rows(case, 10))
    g_sum, g_sq = _bag_grads(case, 10, 2)
    d_ids, d_off, d_w = _dev_inputs(case, dev)
    ops.sgd_sparse_update_wfm_bags(g.view, d_ids, torch.from_numpy(g_sum).to(dev), torch.from_numpy(g_sq).to(dev), d_w, LR,
                                   offsets=d_off)
    torch.cuda.synchronize()
    want = wfm_model.wfm_sgd(compact, case.compact_ids(), _weights(case), g_sum, g_sq, LR, case.offsets)
    assert not np.array_equal(want, compact)
    g.check(want, "sgd_sparse_update_wfm_bags")


@pytest.mark.parametrize("table,dtype,layout,big", BAG_CASES[:8] + BAG_CASES[12:], ids=BAG_IDS[:8] + BAG_IDS[12:])
def test_push_apply_scaled_bags_finished(dev, arena, table, dtype, layout, big):
    """The world-1 push of the sharded step (scatter.hip, kModePush with BAGS): the oracle's serial PS push (cpu.sparse_push)."""
    case = case_of(table, dtype, layout, False, big)
    g = Guard(arena.view(case.table), case, dev)
    compact = g.write(_rows(case, 11))
    bg = _bag_grads(case, 11)
    d_ids, d_off, _ = _dev_inputs(case, dev)
    plan = ops.IndexPlan(case.n, dev).build(d_ids.reshape(-1))
    ops.push_apply_scaled_bags_finished(g.view, plan, torch.from_numpy(bg).to(dev), -LR, **_bag_kw(case, d_off, dev))
    torch.cuda.synchronize()
    want = compact.copy()
    cpu.sparse_push(want, case.compact_ids().reshape(-1), bg[case.which_bag()], LR)
    assert not np.array_equal(want, compact)
    g.check(want, "push_apply_scaled_bags_finished")


# ---- ops, optimizers ----------------------------------------------------------------------------------------------------------
def _opt_arrays(case, seed, kind):
    """Compact param and states of build_inputs' kind: every row a scale drawn log-uniformly over 1e-4 .. 3, m of either sign,
    v and acc as squares."""
    rng = np.random.default_rng([seed, 5])
    k, w = case.keys.size, case.table.width
    f = np.float32
    scale = (10.0 ** rng.uniform(-4.0, np.log10(3.0), size=k)).astype(f)[:, None]
    a = dict(param=rng.standard_normal((k, w), dtype=f))
    if kind == "adagrad":
        a["acc"] = (rng.standard_normal((k, w), dtype=f) * scale) ** 2
    elif kind != "l2":
        a["m"] = rng.standard_normal((k, w), dtype=f) * scale
        a["v"] = (rng.standard_normal((k, w), dtype=f) * scale) ** 2
    return a, scale


def _opt_guards(case, arena, states, dev, a):
    """Guards of the param view and of the state views an optimizer uses, written; a's arrays are replaced by what lies there."""
    names = [n for n in ("param", "acc", "m", "v") if n in a]
    where = {"param": arena, "acc": states["s1"], "m": states["s1"], "v": states["s2"]}
    guards = {}
    for n in names:
        guards[n] = Guard(where[n].view(case.table), case, dev)
        a[n] = guards[n].write(a[n])
    return guards


def _check_opt(guards, want, a, what):
    for n, g in guards.items():
        g.check(want[n], "%s %s" % (what, n))
    assert not np.array_equal(want["param"], a["param"])


FUSED_CASES = [(t, dt, False) for t in TABLES_WIDE for dt in DTYPES] + [("T128", "f32", True)]


@pytest.mark.parametrize("table,dtype,big", FUSED_CASES, ids=["%s-%s%s" % (t, dt, "-36894ids" if b else "") for t, dt, b in FUSED_CASES])
@pytest.mark.parametrize("kind", ["adagrad", "adam", "adamw"])
def test_sparse_opt_fused(dev, arena, states, kind, table, dtype, big):
    """kModeOpt of scatter_dev.h: opt_s1 + row * width, opt_s2 + row * width beside the parameter row, states at table size;
    by sorted position, and by unique key beyond 36,864 ids (apply_by_unique).  Rule of tests/test_gpu_bag_optim.py: bit for
    bit cpu.dedup_reduce + step32 in param and both states."""
    case = case_of(table, dtype, "fixed", False, big)
    a, _ = _opt_arrays(case, 12, kind)
    guards = _opt_guards(case, arena, states, dev, a)
    grads = np.random.default_rng(120).standard_normal((case.n, case.table.width), dtype=np.float32)
    d_ids, _, _ = _dev_inputs(case, dev)
    s1 = guards["acc" if kind == "adagrad" else "m"].view
    ops.sparse_opt_fused(kind, guards["param"].view, d_ids.reshape(-1), torch.from_numpy(grads).to(dev), s1,
                         None if kind == "adagrad" else guards["v"].view, **HYPER3)
    torch.cuda.synchronize()
    uniq, _, red = cpu.dedup_reduce(case.compact_ids().reshape(-1), grads)
    want = step32(kind, a, uniq.astype(np.float32), red, 3)
    _check_opt(guards, want, a, "sparse_opt_fused " + kind)


OPT_BAG_CASES = [("T128", "f32", "fixed", False), ("T128", "i64", "ragged", False), ("T130", "f32", "ragged", False),
                 ("T130", "i64", "fixed", False), ("T128", "f32", "fixed", True), ("T130", "f32", "fixed", True)]
OPT_BAG_IDS = ["%s-%s-%s%s" % (t, dt, lay, "-36894ids" if big else "") for t, dt, lay, big in OPT_BAG_CASES]


@pytest.mark.parametrize("table,dtype,layout,big", OPT_BAG_CASES, ids=OPT_BAG_IDS)
@pytest.mark.parametrize("kind", ["adagrad", "adam", "adamw"])
def test_sparse_opt_fused_bags(dev, arena, states, kind, table, dtype, layout, big):
    """The BAGS instantiation of kModeOpt; beyond 36,864 ids it works by unique key."""
    case = case_of(table, dtype, layout, False, big)
    a, _ = _opt_arrays(case, 13, kind)
    guards = _opt_guards(case, arena, states, dev, a)
    bg = _bag_grads(case, 13)
    d_ids, d_off, _ = _dev_inputs(case, dev)
    s1 = guards["acc" if kind == "adagrad" else "m"].view
    ops.sparse_opt_fused_bags(kind, guards["param"].view, d_ids, torch.from_numpy(bg).to(dev), s1,
                              None if kind == "adagrad" else guards["v"].view, offsets=d_off, **HYPER3)
    torch.cuda.synchronize()
    uniq, _, red = cpu.dedup_reduce(case.compact_ids().reshape(-1), bg[case.which_bag()])
    want = step32(kind, a, uniq.astype(np.float32), red, 3)
    _check_opt(guards, want, a, "sparse_opt_fused_bags " + kind)


@pytest.mark.parametrize("table,dtype,layout,big", OPT_BAG_CASES[:5], ids=OPT_BAG_IDS[:5])
@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
def test_momentum_sparse_update_bags(dev, arena, states, nesterov, table, dtype, layout, big):
    """The occurrence-ordered first phase on the velocity (and, Nesterov, the parameter) rows, then momentum_dense_kernel over
    the whole 16 GiB pair.  The velocity is zero but for the touched rows, so the dense phase leaves every other parameter
    element -- the poison among them -- as it was; bit for bit cpu.momentum_sparse on the compact pair.  Beyond 36,864 ids the
    first phase sorts by radix."""
    case = case_of(table, dtype, layout, False, big)
    gp = Guard(arena.view(case.table), case, dev)
    gv = Guard(states["velocity"].view(case.table), case, dev, poison=False)
    try:
        param = gp.write(_rows(case, 14))
        vel = gv.write(_rows(case, 15, 0.1))
        bg = _bag_grads(case, 14)
        d_ids, d_off, _ = _dev_inputs(case, dev)
        ops.momentum_sparse_update_bags(gp.view, d_ids, torch.from_numpy(bg).to(dev), gv.view, LR, HYPER["momentum"],
                                        nesterov=nesterov, offsets=d_off)
        torch.cuda.synchronize()
        cid = case.compact_ids().reshape(-1)
        sel = np.flatnonzero((cid >= 0) & (cid < case.keys.size))
        w_p, w_v = param.copy(), vel.copy()
        cpu.momentum_sparse(w_p, w_v, cid[sel], bg[case.which_bag()][sel], LR, HYPER["momentum"], nesterov)
        assert not np.array_equal(w_p, param)
        gp.check(w_p, "momentum param")
        gv.check(w_v, "momentum velocity")
    finally:
        gv.view[gv.keys] = 0.0
        torch.cuda.synchronize()


SYMBOL = {"l2": "AddL2RegularizationSparse", "adagrad": "AdaGradOptimizerSparseUpdate", "adam": "AdamOptimizerSparseUpdate",
          "adamw": "AdamWOptimizerSparseUpdate", "lamb": "LambOptimizerSparseUpdate"}


@pytest.mark.parametrize("op", ["l2", "adagrad", "adam", "adamw", "lamb"])
def test_sparse_row_kernel(dev, arena, states, op):
    """sparse_row_kernel of csrc/optim.hip (prow = r * uint64(width)) through the reference-named symbol of every optimizer
    kind, Lamb's norms over the indexed rows included: the unique keys of the float32 batch, shuffled, the dead ids among them.
    Judged as tests/test_gpu_optim_paths.py judges a call: named rows bit for bit the float32 restatement (step32) and within
    (2 c32 + 2) units of 2^-24 S of the float64 reference (step64)."""
    from test_gpu_optim_paths import _raw_call
    case = case_of("T128", "f32")
    t = case.table
    rng = np.random.default_rng(16)
    a, scale = _opt_arrays(case, 16, op)
    guards = _opt_guards(case, arena, states, dev, a)
    live = np.flatnonzero(case.keys != 0)
    order = rng.permutation(live)
    ids = np.concatenate([case.keys[order], np.array(t.dead_ids("f32")[:2])]).astype(np.float32)
    cids = np.concatenate([order, [case.keys.size + 5, case.keys.size + 9]]).astype(np.float32)
    perm = rng.permutation(ids.size)
    ids, cids = ids[perm], cids[perm]
    assert np.array_equal(ids.astype(np.int64)[cids < case.keys.size], case.keys[cids[cids < case.keys.size].astype(np.int64)])
    grads = rng.standard_normal((ids.size, t.width), dtype=np.float32)
    inside = cids < case.keys.size
    grads[inside] *= scale[cids[inside].astype(np.int64)]
    sel, idx, out = step64(op, a, cids, grads, 3)
    want = step32(op, a, cids, grads, 3)
    d = {n: g.view for n, g in guards.items()}
    d_grads = torch.from_numpy(grads.copy()).to(dev)
    assert _raw_call(op, d, torch.from_numpy(ids).to(dev), d_grads, 3) == 0
    torch.cuda.synchronize()
    after = {n: g.view[g.keys].cpu().numpy() for n, g in guards.items()}
    after["grad"] = d_grads.cpu().numpy()
    for name, (x64, s) in out.items():
        got, w32 = named_part(op, name, after[name], sel, idx), named_part(op, name, want[name], sel, idx)
        _same(got, w32, "%s %s, named rows against the float32 restatement" % (op, name))
        off = ref64.units(got, x64, s)
        assert off <= bound_units(op, name), "%s %s: %.2f units of 2^-24 S from float64" % (op, name, off)
    if op == "l2":
        _same(after["grad"], want["grad"], "l2 gradients")
        guards["param"].check(a["param"], "l2 param")
    else:
        for n, g in guards.items():
            g.check(want[n], "%s %s" % (op, n))
        assert not np.array_equal(want["param"], a["param"])


# ---- the row-sharded table at world size 1, on the caller's table -------------------------------------------------------------
def _store(case, view, dev):
    from herald_amd.sharded import ShardedEmbedding
    return ShardedEmbedding(case.table.rows, case.table.width, dev, table=view)


@pytest.mark.parametrize("dtype", DTYPES)
def test_sharded_pull_and_push(dev, arena, dtype):
    """csrc/shard.hip: the owner gather (table + uint64(ok ? key : 0) * width) and the owner apply."""
    case = case_of("T128", dtype)
    g = Guard(arena.view(case.table), case, dev)
    compact = g.write(_rows(case, 20))
    emb = _store(case, g.view, dev)
    d_ids, _, _ = _dev_inputs(case, dev)
    cid = case.compact_ids()
    out = emb.pull(d_ids)
    torch.cuda.synchronize()
    _same(out.reshape(case.n, -1), wfm_model.gather(compact, cid), "pull")
    vals = np.random.default_rng(200).standard_normal((case.n, case.table.width), dtype=np.float32)
    emb.push(d_ids, torch.from_numpy(vals).to(dev), LR)
    torch.cuda.synchronize()
    want = compact.copy()
    cpu.sparse_push(want, cid.reshape(-1), vals, LR)
    assert not np.array_equal(want, compact)
    g.check(want, "push")


SHARD_CASES = [(dt, lay, False) for dt in DTYPES for lay in LAYOUTS] + [("f32", "fixed", True)]
SHARD_IDS = ["%s-%s%s" % (dt, lay, "-36894ids" if b else "") for dt, lay, b in SHARD_CASES]


@pytest.mark.parametrize("dtype,layout,big", SHARD_CASES, ids=SHARD_IDS)
def test_sharded_pull_sum_and_push_bags(dev, arena, dtype, layout, big):
    """The bag ends of csrc/shard.hip / bagsum.hip (ha_gather_sum_u32keys over the received rows, ha_dedup_reduce_bags; beyond
    36,864 ids the reduce works by unique key)."""
    case = case_of("T128", dtype, layout, False, big)
    g = Guard(arena.view(case.table), case, dev)
    compact = g.write(_rows(case, 21))
    emb = _store(case, g.view, dev)
    d_ids, d_off, _ = _dev_inputs(case, dev)
    cid = case.compact_ids()
    out = emb.pull_sum(d_ids, offsets=d_off)
    torch.cuda.synchronize()
    _same(out, bag_model.bag_sum(compact, cid, case.offsets), "pull_sum")
    bg = _bag_grads(case, 21)
    emb.push_bags(d_ids, torch.from_numpy(bg).to(dev), LR, offsets=d_off)
    torch.cuda.synchronize()
    want = compact.copy()
    cpu.sparse_push(want, cid.reshape(-1), bg[case.which_bag()], LR)
    assert not np.array_equal(want, compact)
    g.check(want, "push_bags")


@pytest.mark.parametrize("dtype,layout,big", SHARD_CASES, ids=SHARD_IDS)
def test_sharded_pull_wsum_and_push_wbags(dev, arena, dtype, layout, big):
    """csrc/wshard.hip: ha_gather_wsum_u32keys and ha_dedup_reduce_wbags around the owner gather / apply."""
    case = case_of("T128", dtype, layout, True, big)
    g = Guard(arena.view(case.table), case, dev)
    compact = g.write(_rows(case, 22))
    emb = _store(case, g.view, dev)
    d_ids, d_off, d_w = _dev_inputs(case, dev)
    cid = case.compact_ids()
    out = emb.pull_wsum(d_ids, d_w, offsets=d_off)
    torch.cuda.synchronize()
    _same(out, wbag_model.wbag_sum(compact, cid, _weights(case), case.offsets), "pull_wsum")
    bg = _bag_grads(case, 22)
    emb.push_wbags(d_ids, torch.from_numpy(bg).to(dev), d_w, LR, offsets=d_off)
    torch.cuda.synchronize()
    flat = cid.reshape(-1)
    ok = np.flatnonzero((flat >= 0) & (flat < case.keys.size))
    uniq, inv = np.unique(flat[ok], return_inverse=True)
    red = wshard_model.dedup_reduce_wbags(inv, uniq.size, bg, case.weights[ok], case.which_bag()[ok], -LR)
    want = compact.copy()
    want[uniq] = (want[uniq] + red).astype(np.float32)          # the owner's `+=`, one rounding
    assert not np.array_equal(want, compact)
    g.check(want, "push_wbags")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("graphs", [True, False], ids=["frames", "sized"])
def test_framed_step_pull_sum_and_push_bags(dev, arena, graphs, dtype, layout):
    """FramedStep at world size 1: fixed frames replayed from graphs, and the sized launches, whose own-shard source is the
    big table (ha_gather2_sum_u32map: two-source addresses).  The same batch every step, other gradients."""
    from herald_amd.sharded import FramedStep
    case = case_of("T128", dtype, layout)
    g = Guard(arena.view(case.table), case, dev)
    want = g.write(_rows(case, 23))
    emb = _store(case, g.view, dev)
    d_ids, d_off, _ = _dev_inputs(case, dev)
    cid = case.compact_ids()
    fs = FramedStep(emb, case.n, graphs=graphs, block=2)
    la = fs.LOOKAHEAD
    steps = la + 3
    grads = _bag_grads(case, 23, steps)
    fs.start([d_ids] * la)
    out = torch.empty((case.nbags, case.table.width), device=dev)
    for k in range(steps):
        got = fs.pull_sum(d_ids if k + la < steps else None, offsets=d_off, out=out)
        torch.cuda.synchronize()
        _same(got, bag_model.bag_sum(want, cid, case.offsets), "pull_sum of step %d" % k)
        fs.push_bags(torch.from_numpy(grads[k]).to(dev), LR, offsets=d_off)
        cpu.sparse_push(want, cid.reshape(-1), grads[k][case.which_bag()], LR)
    torch.cuda.synchronize()
    assert fs.fallbacks == 0
    g.check(want, "framed step")


# ---- the HET cache bound to the big store -------------------------------------------------------------------------------------
CACHE_LIMIT = 3400          # >= the 2 x 1,664 keys a push-pull step touches, below the ~6,000 unique keys of a stream of four
CACHE_CASES = [("f32", "fixed"), ("i64", "ragged")]


@functools.lru_cache(maxsize=None)
def stream_of(dtype, layout, weighted=False):
    union, cases = bo.make_stream("T128", dtype, layout, weighted)
    bo.check_stream(union, cases)
    return union, cases


def _perf_same(got, exp, what):
    for f in ("type", "num_all", "num_unique", "num_miss", "num_transfered", "is_full"):
        assert got[f] == exp[f], (what, f, got, exp)
    if exp["type"] == "Push":
        assert got["num_evict"] == exp["num_evict"], (what, got, exp)


class Batch:
    """One batch of a cache stream: the ids as the cache takes them (flat; the cache serves valid keys, so the batch's dead ids
    name the last row here), the model's keys (indices into the union's compact table) and the bags."""

    def __init__(self, dev, union, case):
        t = case.table
        self.case, self.dev = case, dev
        flat = case.flat_keys.copy()
        flat[flat >= t.rows] = t.last_row(case.dtype)
        self.ckeys = np.searchsorted(union.keys, flat).astype(np.uint64)
        assert np.array_equal(union.keys[self.ckeys.astype(np.int64)], flat)
        self.ids = flat.astype(np.float32) if case.dtype == "f32" else flat
        assert np.array_equal(self.ids.astype(np.int64), flat)
        self.off_t = torch.from_numpy(case.offsets).to(dev) if case.offsets is not None else None
        self.bag_of = ops.bag_of(self.off_t, case.n) if case.offsets is not None else None
        self.which = case.which_bag()
        self.bag = case.bag
        pos = np.arange(case.n, dtype=np.int64)
        self.pos = pos.reshape(case.nbags, case.bag) if case.offsets is None else pos
        self.pull_kw = dict(bag=case.bag) if case.offsets is None else dict(offsets=self.off_t)
        self.push_kw = dict(bag=case.bag) if case.offsets is None else dict(bag_of=self.bag_of)

    def kt(self):
        return torch.from_numpy(self.ids).to(self.dev)

    def pooled(self, rows):
        return bag_model.bag_sum(rows, self.pos, self.case.offsets)

    def expanded(self, bag_grads):
        return np.ascontiguousarray(bag_grads[self.which])


class BigCache:
    """An LRU cache over T128 (bind_store(T128, zeros(rows))) beside oracle/cache_model.py over the compact table of the
    stream's keys: the model's keys are the real ones remapped by searchsorted (LRU order and the key-ordered push lists
    survive a monotone map).  Four batches of other keys: from the third on the cache evicts lines that hold un-pushed
    updates, and the next update pushes them back to their rows, the far band's among them."""

    def __init__(self, dev, arena, dtype, layout, seed, weighted=False, pull_bound=1, push_bound=1):
        from herald_amd import cache as hcache
        from oracle import cache_model
        union, cases = stream_of(dtype, layout, weighted)
        t = union.table
        self.union, self.dev, self.width = union, dev, t.width
        self.g = Guard(arena.view(t), union, dev)
        compact = self.g.write(_rows(union, seed))
        self.server = cache_model.Server(compact)
        self.model = cache_model.CacheModel("lru", CACHE_LIMIT, t.width, self.server, pull_bound, push_bound)
        self.versions = torch.zeros(t.rows, dtype=torch.int64, device=dev)
        self.gpu = hcache.LRUCache(CACHE_LIMIT, t.rows, t.width, node_id=0, max_batch=cases[0].n, device=dev)
        self.gpu.bind_store(self.g.view, self.versions)
        self.gpu.pull_bound, self.gpu.push_bound = pull_bound, push_bound
        self.gpu.perf_enabled = True
        self.batches = [Batch(dev, union, c) for c in cases]
        self.rng = np.random.default_rng([seed, 9])
        assert union.keys.size > CACHE_LIMIT >= 2 * cases[0].n

    def bag_grads(self, b):
        return self.rng.standard_normal((b.case.nbags, self.width), dtype=np.float32) * np.float32(-0.01)

    def new_out(self, b):
        return torch.full((b.case.nbags, self.width), float("nan"), dtype=torch.float32, device=self.dev)

    def check_store(self, what):
        """Versions and rows of the store against the model's server; no version anywhere else; poison and sentinels."""
        v = self.versions[self.g.keys].cpu().numpy()
        np.testing.assert_array_equal(v, self.server.ver, err_msg="%s: server versions" % what)
        assert int(torch.count_nonzero(self.versions)) == int(np.count_nonzero(self.server.ver)), "%s: a version elsewhere" % what
        self.g.check(self.server.table, what)

    def check_lines(self, what):
        keys = self.union.keys
        res, lines = self.model.resident(), self.gpu.lines()
        assert sorted(lines) == [int(keys[k]) for k in sorted(res)], "%s: resident set" % what
        for ck, ln in res.items():
            gl = lines[int(keys[ck])]
            assert gl.version == ln.version and gl.updates == ln.updates, (what, ck)
            _same(gl.data, ln.data, "%s: data of key %d" % (what, keys[ck]))
            if ln.grad is not None:
                _same(gl.grad, ln.grad, "%s: grad of key %d" % (what, keys[ck]))
        assert self.gpu.size() == self.model.policy.size()
        np.testing.assert_array_equal(self.gpu.keys(), keys[np.array(self.model.policy.keys(), dtype=np.int64)].astype(np.uint64))

    def check_pushed_far(self):
        """The trace did what it is here for: lines were evicted, and rows of the top band were pushed back to the store."""
        t, keys = self.union.table, self.union.keys
        assert any(p["type"] == "Push" and p["num_evict"] > 0 for p in self.model.perf)
        top = t.band_of(keys) == t.top_band
        assert (self.server.ver[top] > 0).any() and (self.server.ver[~top] > 0).any()


@pytest.mark.parametrize("dtype,layout", CACHE_CASES)
def test_cache_planned_pairs_sum_pooled(dev, arena, dtype, layout):
    """csrc/cache_block.hip, the pooled role: lookup_sum_planned / update_planned_bags, four pairs planned as one block."""
    c = BigCache(dev, arena, dtype, layout, 30)
    c.gpu.plan_block([b.kt() for b in c.batches])
    for step, b in enumerate(c.batches):
        want_rows = c.model.lookup(b.ckeys)
        out = c.new_out(b)
        c.gpu.embedding_lookup_sum_planned(out, **b.pull_kw).wait()
        _same(out, b.pooled(want_rows), "pooled rows of step %d" % step)
        bg = c.bag_grads(b)
        c.model.update(b.ckeys, b.expanded(bg))
        c.gpu.embedding_update_planned_bags(torch.from_numpy(bg).to(dev), **b.push_kw).wait()
        for got, exp in zip(c.gpu.perf[-2:], c.model.perf[-2:]):
            _perf_same(got, exp, "step %d" % step)
        c.check_store("planned pair %d" % step)
    assert c.gpu.plan_pending() == 0
    c.check_lines("planned pairs")
    c.check_pushed_far()


@pytest.mark.parametrize("dtype,layout", CACHE_CASES)
def test_cache_planned_pairs_weighted(dev, arena, dtype, layout):
    """csrc/cache_block.hip, the weighted role: lookup_wsum_planned / update_planned_wbags; the mask's dead slots sit on key 0,
    whose line is cached and pushed like any other and whose row must keep its bits."""
    c = BigCache(dev, arena, dtype, layout, 31, weighted=True)
    scale = -0.5
    c.gpu.plan_block([b.kt() for b in c.batches])
    for step, b in enumerate(c.batches):
        w = b.case.weights
        wt = torch.from_numpy(w).to(dev)
        want_rows = c.model.lookup(b.ckeys)
        want = wbag_model.wbag_sum(want_rows, b.pos, w.reshape(b.pos.shape), b.case.offsets)
        out = c.new_out(b)
        c.gpu.embedding_lookup_wsum_planned(out, wt, **b.pull_kw).wait()
        _same(out, want, "weighted pooled rows of step %d" % step)
        bg = c.rng.standard_normal((b.case.nbags, c.width), dtype=np.float32)
        terms = (np.float32(scale) * wbag_model.wbag_grad_rows(bg, w, b.which)).astype(np.float32)
        c.model.update(b.ckeys, terms)
        c.gpu.embedding_update_planned_wbags(torch.from_numpy(bg).to(dev), wt, scale=scale, **b.push_kw).wait()
        for got, exp in zip(c.gpu.perf[-2:], c.model.perf[-2:]):
            _perf_same(got, exp, "step %d" % step)
        c.check_store("weighted planned pair %d" % step)
    assert c.gpu.plan_pending() == 0
    c.check_lines("weighted planned pairs")
    c.check_pushed_far()


@pytest.mark.parametrize("dtype,layout", CACHE_CASES)
def test_cache_planned_push_pull_bag_chain(dev, arena, dtype, layout):
    """The planned push-pull chain with pooled entries (ha_cache_push_pull_planned_bags): a head, three push-pull steps, the
    closing entry."""
    c = BigCache(dev, arena, dtype, layout, 32)
    bs = c.batches
    c.gpu.plan_block([b.kt() for b in bs] + [None], push_pull=True)
    grads = [c.bag_grads(b) for b in bs]
    for e, b in enumerate(bs):
        if e == 0:
            want_rows = c.model.lookup(b.ckeys)
        else:
            want_rows = c.model.push_pull(b.ckeys, bs[e - 1].ckeys, bs[e - 1].expanded(grads[e - 1]))
        out = c.new_out(b)
        g = torch.from_numpy(grads[e - 1]).to(dev) if e else None
        c.gpu.embedding_push_pull_planned_bags(out, g, bag=b.bag, pull_offsets=b.off_t,
                                               push_bag_of=bs[e - 1].bag_of if e else None).wait()
        _same(out, b.pooled(want_rows), "pooled rows of entry %d" % e)
        if e == 0:
            _perf_same(c.gpu.perf[-1], c.model.perf[-1], "head")
        c.check_store("chain entry %d" % e)
    c.model.update(bs[-1].ckeys, bs[-1].expanded(grads[-1]))
    c.gpu.embedding_push_pull_planned_bags(None, torch.from_numpy(grads[-1]).to(dev), bag=bs[-1].bag,
                                           push_bag_of=bs[-1].bag_of).wait()
    _perf_same(c.gpu.perf[-1], c.model.perf[-1], "closing entry")
    c.check_store("closing entry")
    assert c.gpu.plan_pending() == 0
    c.check_lines("push-pull chain")
    c.check_pushed_far()


@pytest.mark.parametrize("dtype,layout", CACHE_CASES)
def test_cache_bag_calls_one_by_one(dev, arena, dtype, layout):
    """csrc/cache.hip, the bag calls: embedding_lookup_sum, embedding_update_bags and embedding_push_pull_bags."""
    c = BigCache(dev, arena, dtype, layout, 33)
    bs = c.batches

    def lookup(b, what):
        want_rows = c.model.lookup(b.ckeys)
        out = c.new_out(b)
        c.gpu.embedding_lookup_sum(b.kt(), out, **b.pull_kw).wait()
        _same(out, b.pooled(want_rows), what)
        _perf_same(c.gpu.perf[-1], c.model.perf[-1], what)

    def update(b, what):
        bg = c.bag_grads(b)
        c.model.update(b.ckeys, b.expanded(bg))
        c.gpu.embedding_update_bags(b.kt(), torch.from_numpy(bg).to(dev), **b.push_kw).wait()
        _perf_same(c.gpu.perf[-1], c.model.perf[-1], what)
        c.check_store(what)

    lookup(bs[0], "lookup of batch 0")
    update(bs[0], "update of batch 0")
    lookup(bs[1], "lookup of batch 1")
    bg = c.bag_grads(bs[1])
    want_rows = c.model.push_pull(bs[2].ckeys, bs[1].ckeys, bs[1].expanded(bg))
    out = c.new_out(bs[2])
    c.gpu.embedding_push_pull_bags(bs[2].kt(), out, bs[1].kt(), torch.from_numpy(bg).to(dev), bag=bs[1].bag,
                                   pull_offsets=bs[2].off_t, push_bag_of=bs[1].bag_of).wait()
    _same(out, bs[2].pooled(want_rows), "push-pull rows")
    c.check_store("push-pull of batches 2 and 1")
    update(bs[2], "update of batch 2")
    lookup(bs[3], "lookup of batch 3")
    update(bs[3], "update of batch 3")
    c.check_lines("bag calls")
    c.check_pushed_far()

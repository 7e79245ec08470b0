"""Which FLOAT VALUES go through the row kernels: +-0, subnormals, sums that overflow, infinities, NaNs with payloads and exact
cancellations (tests/special_values.py plants them; tests/test_special_values_cpu.py proves the cases worth running), through
every family of entry points.  The assertion is always special_values.same_bits against the family's reference over the WHOLE
output or table -- np.testing.assert_array_equal sees no zero's sign --, so a special value that leaks into any other row or
column is seen, and the message says whether the first differing element lies inside the case's poisoned set.

    copies               raw bits (a NaN's payload and sign survive)                       table[ids]
    plan-driven applies  NaN where the reference has NaN, everything else bit for bit      oracle/cpu.py serial chain
    tolerance modes      the same                                                         oracle/qstep_model.py trees
    one-launch steps, work-queue step, optimizers, pooled forms, sharded table, planned cache pair: see each test.

The elements compared per family are counted (STATS, printed when the module ends; HERALD_SPECIAL_STATS=<file> writes them as
JSON): docs/EXPERIMENTS.md, "Special float values"."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import bag_model
import fm_model
import fm_pooled_model
import special_values as sv
from herald_amd import cache as hcache
from herald_amd import _lib, ops
from oracle import cache_model, cpu, qstep_model
from test_optim_oracle import build_momentum, step32

pytestmark = pytest.mark.gpu
F = np.float32
STATS = {}


def _same(family, got, want, what, **kw):
    STATS[family] = STATS.get(family, 0) + sv.same_bits(np.ascontiguousarray(got), np.ascontiguousarray(want), what, **kw)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for family, count in STATS.items():
        print("\n%-22s %12d elements compared bit for bit by the comparisons that passed" % (family, count))
    if os.environ.get("HERALD_SPECIAL_STATS"):
        with open(os.environ["HERALD_SPECIAL_STATS"], "w") as f:
            json.dump(STATS, f)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _small(width, n=8000):
    return sv.make_case(width, sv.SMALL_RUNS, n, 6000, seed=width)


@functools.lru_cache(maxsize=None)
def _big(width):
    return sv.big_case(width, seed=width)


@functools.lru_cache(maxsize=None)
def _stream(width, n=8000):
    return tuple(sv.make_stream(width, 3, n=n, seed=width + 1))


@functools.lru_cache(maxsize=None)
def _ref(case, form, tree=None):
    """The reference result of `form` on a case, computed once and never written to.  form: "chain" (table after the sparse SGD),
    "push" (table after row += reduced), "push_scaled" (a parameter-server push: row += reduce of -lr * g), "reduce" /
    "reduce_scaled" (the reduced rows of the unique keys, the latter of -lr * g).  tree None: the reference's serial chain
    (oracle/cpu.py); "tree": the tolerance mode, one tree per run of 64 and more; "chunked": runs beyond 256 in chunks of 256
    (oracle/qstep_model.py -- which keeps the chain on rows that are no multiple of 4 floats)."""
    t = case.table.copy()
    with np.errstate(all="ignore"):
        if tree is None:
            if form == "chain":
                out = cpu.sgd_sparse_update(t, case.ids_f32, case.grads, case.lr)
            elif form == "push":
                uniq, _, red = cpu.dedup_reduce(case.ids_f32, case.grads)
                out = cpu.push_apply(t, uniq, red)
            elif form == "push_scaled":
                out = cpu.sparse_push(t, case.ids_f32, case.grads, case.lr)
            elif form == "reduce":
                out = cpu.dedup_reduce(case.ids_f32, case.grads)[2]
            elif form == "reduce_scaled":
                out = cpu.dedup_reduce(case.ids_f32, cpu.scale_values(case.grads, case.lr))[2]
            else:
                raise ValueError(form)
        else:
            chunked = tree == "chunked"
            assert not chunked or qstep_model.listed_chunking(case.ids, case.width)
            grads = cpu.scale_values(case.grads, case.lr) if form.endswith("_scaled") else case.grads
            if form == "chain":
                out = qstep_model.sgd_sparse_update(t, case.ids, grads, case.lr, long_min=None, coop_min=64, chunked=chunked)
            elif form in ("push", "push_scaled"):
                out = qstep_model.sgd_sparse_update(t, case.ids, grads, 1.0, long_min=None, coop_min=64, mode="push", chunked=chunked)
            else:
                full = qstep_model.sgd_sparse_update(np.zeros_like(t), case.ids, grads, 1.0, long_min=None, coop_min=64, mode="push",
                                                     chunked=chunked)
                out = full[np.unique(case.ids)]
    out.setflags(write=False)
    return out


def _special_table(rows, width, seed):
    rng = np.random.default_rng([seed, rows, width])
    return sv.sprinkle(rng.standard_normal((rows, width), dtype=np.float32), seed, 0.05)[0]


# ---- copies ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ptr_mod_16_is_4"])
@pytest.mark.parametrize("ids_kind", ["f32", "i64"])
@pytest.mark.parametrize("width", [1, 4, 200])
def test_copies_embedding_lookup(dev, width, ids_kind, aligned):
    """A gather moves rows: every bit pattern arrives as it is -- both zeros, subnormals, infinities, a NaN's payload and sign."""
    rows, n = 4000, 5000
    table = _special_table(rows, width, 3 * width + aligned)
    rng = np.random.default_rng(width)
    ids = rng.integers(1, rows, size=n)
    if aligned:
        t = _dev(table, dev)
    else:
        flat = torch.empty(rows * width + 1, dtype=torch.float32, device=dev)
        t = flat[1:].view(rows, width)
        t.copy_(torch.from_numpy(table))
        assert t.data_ptr() % 16 == 4
    out = ops.embedding_lookup(t, _dev(ids.astype(np.float32) if ids_kind == "f32" else ids, dev))
    torch.cuda.synchronize()
    _same("copies", _np(out), table[ids], "embedding_lookup", copy=True, rows=ids)
    _same("copies", _np(t), table, "the table after the lookup", copy=True)


@pytest.mark.parametrize("width", [1, 4, 200])
def test_copies_lookup_sort_and_first_pipeline_lookups(dev, width):
    """The lookup half of lookup_sort and the first lookup of both step pipelines (before any update): copies."""
    case = _small(width, 7000)
    table = sv.sprinkle(case.table, width, 0.05)[0]
    ids = case.ids
    d_ids = _dev(ids.astype(np.float32), dev)
    t = _dev(table, dev)
    out = ops.lookup_sort(t, d_ids, ops.IndexPlan(case.n, dev))
    torch.cuda.synchronize()
    _same("copies", _np(out), table[ids], "lookup_sort", copy=True, rows=ids)
    if width % 4 == 0:
        pipe = ops.StepPipeline(t, case.n, case.lr)
        out = pipe.start(d_ids)
        torch.cuda.synchronize()
        _same("copies", _np(out), table[ids], "StepPipeline.start", copy=True, rows=ids)
        qp = ops.QueueStepPipeline(t, case.n, case.lr, overlap=False, block=1)       # (both pipelines: rows of 4 k floats)
        out = qp.start([d_ids])
        torch.cuda.synchronize()
        _same("copies", _np(out), table[ids], "QueueStepPipeline.start", copy=True, rows=ids)
    _same("copies", _np(t), table, "the table after the lookups", copy=True)


# ---- plan-driven applies: the serial chain -----------------------------------------------------------------------------------------
APPLIES = ("sgd_apply", "sgd_sparse_update", "sgd_apply_finish", "push_apply", "push_apply_finish", "dedup_reduce",
           "dedup_reduce_scaled")
# ... and, on the batch of 36,894 ids, the two entries that exist for a FINISHED plan: ha_sgd_apply_finished (ops.sgd_apply(finished=
# True)) and ha_push_apply_scaled_finished (the launch DESIGN.md 3c times; herald_amd.ops has no wrapper of it -- the framed step
# engine of the sharded table calls it -- so the test calls the symbol)
BIG_APPLIES = APPLIES + ("sgd_apply_finished", "push_apply_scaled_finished")
# what a batch beyond 36,864 ids maps to unique keys (csrc/scatter.hip apply_by_unique, csrc/fused.hip apply_finish), and so what
# tolerance mode 2 cuts into chunks; the others stay one wave per sorted position, one tree per run in every tolerance mode
BY_UNIQUE_KEY = ("sgd_apply_finished", "push_apply_scaled_finished", "sgd_apply_finish", "push_apply_finish", "dedup_reduce", "dedup_reduce_scaled")


def _run_apply(dev, case, entry, table=None):
    """-> (result, reference form, keys of the result's rows or None for the whole table)."""
    d_ids, d_g = _dev(case.ids_f32, dev), _dev(case.grads, dev)
    t = _dev(case.table, dev) if table is None else table
    if entry == "sgd_sparse_update":
        ops.sgd_sparse_update(t, d_ids, d_g, case.lr)
        return t, "chain", None
    plan = ops.IndexPlan(case.n, dev)
    if entry.endswith("_finish"):
        plan.sort(d_ids)
    else:
        plan.build(d_ids)
    if entry in ("sgd_apply", "sgd_apply_finished"):
        ops.sgd_apply(t, plan, d_g, case.lr, finished=entry == "sgd_apply_finished")
        return t, "chain", None
    if entry == "sgd_apply_finish":
        ops.sgd_apply_finish(t, plan, d_g, case.lr)
        return t, "chain", None
    if entry == "push_apply_scaled_finished":
        rc = _lib.load().ha_push_apply_scaled_finished(t.data_ptr(), case.rows, case.width, plan.ws.data_ptr(), case.n,
                                                       d_g.data_ptr(), -case.lr, ops._stream_ptr())
        assert rc == 0, _lib.load().ha_last_error()
        return t, "push_scaled", None
    if entry == "push_apply":
        ops.push_apply(t, plan, d_g)
        return t, "push", None
    if entry == "push_apply_finish":
        ops.push_apply_finish(t, plan, d_g)
        return t, "push", None
    uniq = np.unique(case.ids)
    assert plan.n_unique() == uniq.size
    red = ops.dedup_reduce(plan, d_g, scale=-case.lr if entry == "dedup_reduce_scaled" else None)
    return red[:uniq.size], "reduce" if entry == "dedup_reduce" else "reduce_scaled", uniq


def _check_apply(dev, family, case, entry, tree=None):
    got, form, keys = _run_apply(dev, case, entry)
    torch.cuda.synchronize()
    poisoned = case.poisoned if keys is None else case.mask_of(keys)
    _same(family, _np(got), _ref(case, form, tree), "%s on %s against %s (%s)" % (entry, case, form, tree or "serial chain"),
          poisoned=poisoned, rows=keys)
    return form


@pytest.mark.parametrize("entry", APPLIES)
@pytest.mark.parametrize("width", [1, 4, 64, 200])
def test_plan_driven_applies_serial_chain(dev, width, entry):
    """Tolerance mode off: every run length class (short, medium, long, cooperative LDS slices, runs beyond 1,024) holds the
    reference's serial chain with the specials at the first, middle and last slot and around every multiple of 16 and 256."""
    assert ops.set_tolerance_mode(False) is False
    _check_apply(dev, "plan-driven applies", _small(width), entry)


@pytest.mark.parametrize("entry", BIG_APPLIES)
@pytest.mark.parametrize("width", [4, 64, 200])
def test_big_batch_serial_chain(dev, width, entry):
    """36,894 ids, tolerance mode off.  BY_UNIQUE_KEY entries map their waves to unique keys there (the applies of a finished
    plan, the fused finishes, the reduces); sgd_apply, push_apply and sgd_sparse_update stay one wave per sorted position."""
    assert ops.set_tolerance_mode(False) is False
    _check_apply(dev, "plan-driven applies", _big(width), entry)


# ---- tolerance modes: the trees ----------------------------------------------------------------------------------------------------
@pytest.fixture()
def tolerance():
    prev = ops.set_tolerance_mode(True)
    yield
    ops.set_tolerance_mode(prev)


@pytest.fixture()
def tolerance_chunked():
    prev = ops.set_tolerance_mode(2)
    yield
    ops.set_tolerance_mode(prev)


@pytest.mark.parametrize("entry", APPLIES)
@pytest.mark.parametrize("width", [1, 4, 64, 200])
def test_tolerance_mode_tree_from_64(dev, tolerance, width, entry):
    """All seven entry points with the mode on.  Runs of 64 and more are row - tree_sum(lr * g) in the fixed order of oracle/
    qstep_model.py tree_coop: unused slots of the tree hold +0 whatever lies beyond the run, a partial sum starts from +0
    (0 + (-0) = +0), and an exact cancellation over a -0 row ends in -0 where the chain ends in +0.  No "within 1e-5 of the
    chain" here: it has no meaning on a poisoned element.  Width 1: rows that are no multiple of 4 floats have no tree -- the
    mode is the serial chain there (include/herald_amd.h; the model says so itself)."""
    case = _small(width)
    form = _check_apply(dev, "tolerance modes", case, entry, tree="tree")
    # the mode really took the tree where it has one, and the chain where it has none (width 1: 4-byte rows)
    assert (sv.canon(_ref(case, form, "tree")) != sv.canon(_ref(case, form))).any() == qstep_model.tolerance_has_tree(width)


def test_tolerance_mode_misaligned_table_is_the_chain(dev, tolerance):
    """A table that does not start on 16 bytes has no tree either, at any width (qstep_model.tolerance_has_tree(aligned=False))."""
    case = _small(4)
    flat = torch.empty(case.rows * 4 + 1, dtype=torch.float32, device=dev)
    t = flat[1:].view(case.rows, 4)
    t.copy_(torch.from_numpy(case.table))
    assert t.data_ptr() % 16 == 4 and not qstep_model.tolerance_has_tree(4, aligned=False)
    got, form, _ = _run_apply(dev, case, "sgd_apply", table=t)
    torch.cuda.synchronize()
    with np.errstate(all="ignore"):
        want = qstep_model.sgd_sparse_update(case.table.copy(), case.ids, case.grads, case.lr, long_min=None, coop_min=64, aligned=False)
    sv.same_bits(want, _ref(case, "chain"), "the model of a misaligned call is the chain")
    _same("tolerance modes", _np(got), want, "sgd_apply, tolerance mode, misaligned table", poisoned=case.poisoned)


@pytest.mark.parametrize("mode", ["tree", "chunked"])
@pytest.mark.parametrize("entry", BIG_APPLIES)
@pytest.mark.parametrize("width", [64, 200])
def test_tolerance_modes_big_batch(dev, width, entry, mode):
    """36,894 ids with runs of 300 and 2,100, every entry point, modes 1 and 2.  Mode 1: one tree per run everywhere.  Mode 2: the
    BY_UNIQUE_KEY entries cut a run beyond 256 occurrences into chunks of 256 whose sums are added in chunk order
    (qstep_model.tree_coop_chunked, in the sgd, push and reduce forms); the entries by sorted position keep one tree per run."""
    case = _big(width)
    assert qstep_model.listed_chunking(case.ids, width)
    prev = ops.set_tolerance_mode(2 if mode == "chunked" else 1)
    try:
        tree = "chunked" if mode == "chunked" and entry in BY_UNIQUE_KEY else "tree"
        form = _check_apply(dev, "tolerance modes", case, entry, tree=tree)
    finally:
        ops.set_tolerance_mode(prev)
    if mode == "chunked" and entry in BY_UNIQUE_KEY:      # the chunks are another order than the one tree
        assert (sv.canon(_ref(case, form, "chunked")) != sv.canon(_ref(case, form, "tree"))).any()


# ---- one-launch steps ----------------------------------------------------------------------------------------------------------------
def _chain_stream(cases):
    """[(lookup rows of batch k before its update)], table after the stream, by the serial chain."""
    key = ("chain_stream",) + tuple(c.name for c in cases)
    if key not in _STREAMS:
        t = cases[0].table.copy()
        outs = []
        with np.errstate(all="ignore"):
            for c in cases:
                outs.append(t[c.ids].copy())
                cpu.sgd_sparse_update(t, c.ids_f32, c.grads, c.lr)
        _STREAMS[key] = (outs, t)
    return _STREAMS[key]


_STREAMS = {}


@pytest.mark.parametrize("width", [4, 64, 200])
def test_one_launch_steps_sgd_push_pull(dev, width):
    """Three batches that share their poisoned keys: the rows handed from the applying wave to the gathering wave carry the
    updated bits (NaN where the chain has NaN, both zeros, subnormals), and nothing else changes."""
    cases = _stream(width)
    outs, want_t = _chain_stream(cases)
    first = cases[0]
    table = _dev(first.table, dev)
    plans = [ops.IndexPlan(first.n, dev), ops.IndexPlan(first.n, dev)]
    pends = [ops.PendingTable(dev), ops.PendingTable(dev)]
    d_ids = [_dev(c.ids_f32, dev) for c in cases]
    out = ops.lookup_sort_pend(table, d_ids[0], plans[0], pends[0])
    for k, c in enumerate(cases):
        torch.cuda.synchronize()
        _same("one-launch steps", _np(out), outs[k], "sgd_push_pull: rows of batch %d" % k, copy=k == 0,
              poisoned=first.mask_of(c.ids), rows=c.ids)
        g = _dev(c.grads, dev)
        if k + 1 < len(cases):
            out = ops.sgd_push_pull(table, plans[k % 2], g, c.lr, pends[k % 2], d_ids[k + 1], plans[(k + 1) % 2], pends[(k + 1) % 2])
            torch.cuda.synchronize()
            assert not plans[(k + 1) % 2].handoff_timed_out()
        else:
            ops.sgd_push_pull(table, plans[k % 2], g, c.lr, pends[k % 2])
    torch.cuda.synchronize()
    _same("one-launch steps", _np(table), want_t, "sgd_push_pull: table after the stream", poisoned=first.poisoned)
    assert pends[0].is_idle() and pends[1].is_idle()


@pytest.mark.parametrize("width", [4, 64, 200])
def test_one_launch_steps_step_pipeline(dev, width):
    cases = _stream(width)
    outs, want_t = _chain_stream(cases)
    first = cases[0]
    table = _dev(first.table, dev)
    pipe = ops.StepPipeline(table, first.n, first.lr)
    d_ids = [_dev(c.ids_f32, dev) for c in cases]
    out = pipe.start(*d_ids)
    for k, c in enumerate(cases):
        torch.cuda.synchronize()
        _same("one-launch steps", _np(out), outs[k], "StepPipeline: rows of batch %d" % k, copy=k == 0,
              poisoned=first.mask_of(c.ids), rows=c.ids)
        out = pipe.step(_dev(c.grads, dev), None)
    torch.cuda.synchronize()
    assert out is None
    _same("one-launch steps", _np(table), want_t, "StepPipeline: table after the stream", poisoned=first.poisoned)


# ---- work-queue step -----------------------------------------------------------------------------------------------------------------
def _qstep_stream(cases):
    key = ("qstep_stream",) + tuple(c.name for c in cases)
    if key not in _STREAMS:
        t = cases[0].table.copy()
        outs = []
        with np.errstate(all="ignore"):
            for c in cases:
                outs.append(t[c.ids].copy())
                qstep_model.sgd_sparse_update(t, c.ids, c.grads, c.lr)
        _STREAMS[key] = (outs, t)
    return _STREAMS[key]


@pytest.mark.parametrize("mode", [(False, 1), (True, 2)], ids=["one_stream", "side_stream_block2"])
@pytest.mark.parametrize("width,n", [(4, 7000), (64, 7000), (200, 7000), (64, 8000), (200, 8000)],
                         ids=["w4_narrow", "w64_narrow", "w200_narrow", "w64_wide", "w200_wide"])
def test_work_queue_step(dev, width, n, mode):
    """The chain below 16 occurrences, tree_long below 64, the sixteen-wave tree from 64 and chunks of 256 beyond (oracle/
    qstep_model.py): narrow path (up to 7,168 ids) and wide path; lookups of every batch and the table after three batches."""
    if n > ops.qstep_max_ids() and mode == (False, 1):
        mode = (True, 4)
    cases = _stream(width, n)
    outs, want_t = _qstep_stream(cases)
    first = cases[0]
    table = _dev(first.table, dev)
    pipe = ops.QueueStepPipeline(table, n, first.lr, overlap=mode[0], block=mode[1])
    assert pipe.wide == (n > ops.qstep_max_ids())
    L = pipe.LOOKAHEAD
    d_ids = [_dev(c.ids_f32, dev) for c in cases]
    out = pipe.start(d_ids[:L])
    for k, c in enumerate(cases):
        torch.cuda.synchronize()
        _same("work-queue step", _np(out), outs[k], "QueueStepPipeline: rows of batch %d" % k, copy=k == 0,
              poisoned=first.mask_of(c.ids), rows=c.ids)
        out = pipe.step(_dev(c.grads, dev), d_ids[k + L] if k + L < len(cases) else None)
    torch.cuda.synchronize()
    assert out is None
    _same("work-queue step", _np(table), want_t, "QueueStepPipeline: table after the stream", poisoned=first.poisoned)


# ---- optimizers ----------------------------------------------------------------------------------------------------------------------
SYMBOL = {"l2": "AddL2RegularizationSparse", "adagrad": "AdaGradOptimizerSparseUpdate", "adam": "AdamOptimizerSparseUpdate",
          "adamw": "AdamWOptimizerSparseUpdate", "lamb": "LambOptimizerSparseUpdate", "momentum": "MomentumOptimizerSparseUpdate",
          "nesterov": "MomentumOptimizerSparseUpdate"}
STATE_NAMES = {"l2": (), "adagrad": ("acc",), "adam": ("m", "v"), "adamw": ("m", "v"), "lamb": ("m", "v"),
               "momentum": ("velocity",), "nesterov": ("velocity",)}


def _hyper(op, eps, t=2):
    if op == "l2":
        return (0.3,)
    if op == "adagrad":
        return (0.05, eps)
    if op in ("momentum", "nesterov"):
        return (0.05, 0.9, op == "nesterov")
    sc = (0.05, 0.9, 0.999, 0.9 ** t, 0.999 ** t, eps)
    return sc if op == "adam" else sc + (0.1,)


def _optim_inputs(op, width, n=300, rows=700, finite_only=False):
    o = sv.optim_specials(n, width, seed=width)
    rng = np.random.default_rng([11, width, n])
    idx = rng.permutation(rows)[:n]
    a = dict(param=rng.standard_normal((rows, width), dtype=np.float32),
             acc=(rng.standard_normal((rows, width), dtype=np.float32) ** 2).astype(F),
             m=rng.standard_normal((rows, width), dtype=np.float32),
             v=(rng.standard_normal((rows, width), dtype=np.float32) ** 2).astype(F))
    g = o["g"].copy()
    for name in ("acc", "m", "v"):
        a[name][idx] = o[name]
    a["param"][idx[:o["special_rows"]], ::3] = sv.NEG_ZERO
    if finite_only:                                # (Lamb: the norms stay finite, the other specials stay)
        bad = ~(np.isfinite(g).all(axis=1) & np.isfinite(o["acc"]).all(axis=1) & (np.abs(g) < 1e19).all(axis=1))
        g[bad] = rng.standard_normal((int(bad.sum()), width), dtype=np.float32)
        for name in ("acc", "v"):
            a[name][idx[bad]] = F(0.5)
    a["ids"], a["grads"] = idx.astype(np.float32), g
    return a


def _call_symbol(dev, op, a, hyper):
    """One call of the reference-named symbol on device copies of `a`; -> the arrays read back (l2: its gradient output)."""
    names = ("param",) + STATE_NAMES[op]
    d = {k: _dev(a[k], dev) for k in names}
    ids, grads = _dev(a["ids"], dev), _dev(a["grads"], dev)
    scalars = [ctypes.c_bool(x) if isinstance(x, bool) else ctypes.c_float(x) for x in hyper]
    ops.dl_call(SYMBOL[op], [d["param"], ids, grads] + [d[k] for k in STATE_NAMES[op]], scalars=scalars)
    torch.cuda.synchronize()
    got = {k: _np(v) for k, v in d.items()}
    got["grad"] = _np(grads)
    return got


@pytest.mark.parametrize("width", [1, 4, 260])
@pytest.mark.parametrize("op,eps", [("adagrad", 0.0), ("adagrad", 1e-7), ("adagrad", 1e-39), ("adam", 0.0), ("adam", 1e-7), ("adamw", 1e-7),
                                    ("l2", 0.0), ("lamb", 1e-7), ("lamb_finite_norms", 1e-7)])
def test_optimizer_row_kernels(dev, op, eps, width):
    """Specials in gradients and in state, every pairing of special_values.optim_specials in every column: acc = 0 with eps = 0
    (0 / 0 as the reference divides), a subnormal eps (a subnormal denominator: g / d is finite where g * (1 / d) overflows),
    subnormal v, v = inf, a gradient whose square is subnormal / underflows / overflows,
    infinities and NaNs; Lamb with non-finite norms (every named row takes them) and with finite ones.  Reference: the float32
    restatement of oracle/cpu.py, call by call, whole arrays."""
    finite = op == "lamb_finite_norms"
    op = "lamb" if finite else op
    a = _optim_inputs(op, width, finite_only=finite)
    hyper = _hyper(op, eps)
    with np.errstate(all="ignore"):
        want = step32(op, a, a["ids"], a["grads"], 2, hyper)
    got = _call_symbol(dev, op, a, hyper)
    if finite:
        assert np.isfinite(want["param"]).all()
    elif op == "lamb":
        assert np.isnan(want["param"][a["ids"].astype(np.int64)]).all()
    for name, w in want.items():
        _same("optimizers", got[name], w, "%s eps=%g width=%d: %s" % (op, eps, width, name))
    if op != "l2":
        _same("optimizers", got["grad"], a["grads"], "%s: the gradients are inputs" % op, copy=True)


@pytest.mark.parametrize("width", [1, 4, 260])
@pytest.mark.parametrize("op", ["momentum", "nesterov"])
def test_optimizer_momentum(dev, op, width):
    a = build_momentum(5 + width, 300, width, 300)
    a["grads"] = sv.sprinkle(a["grads"], 1, 0.05)[0]
    a["velocity"] = sv.sprinkle(a["velocity"], 2, 0.05)[0]
    a["param"] = sv.sprinkle(a["param"], 3, 0.05)[0]
    hyper = _hyper(op, 0.0)
    with np.errstate(all="ignore"):
        want = step32(op, a, a["ids"], a["grads"], 1, hyper)
    got = _call_symbol(dev, op, a, hyper)
    for name in ("param", "velocity"):
        _same("optimizers", got[name], want[name], "%s width=%d: %s" % (op, width, name))


def _fused_reference(kind, case, ids, grads, state, hp):
    p = case.table.copy()
    s = {k: v.copy() for k, v in state.items()}
    with np.errstate(all="ignore"):
        uniq, _, red = cpu.dedup_reduce(ids, grads)
        idx = uniq.astype(np.int64)
        if kind == "adagrad":
            cpu.adagrad_sparse(p, s["acc"], idx, red, hp["lr"], hp["eps"])
        else:
            cpu.adam_sparse(p, s["m"], s["v"], idx, red, hp["lr"], hp["beta1"], hp["beta2"], F(hp["beta1t"]), F(hp["beta2t"]),
                            hp["eps"], hp["weight_decay"] if kind == "adamw" else None)
    return p, s


def _fused_state(case, seed):
    rng = np.random.default_rng([seed, case.width])
    shape = case.table.shape
    return {"acc": sv.sprinkle((rng.standard_normal(shape, dtype=np.float32) ** 2).astype(F), seed, 0.03)[0],
            "m": sv.sprinkle(rng.standard_normal(shape, dtype=np.float32), seed + 1, 0.03)[0],
            "v": sv.sprinkle((rng.standard_normal(shape, dtype=np.float32) ** 2).astype(F), seed + 2, 0.03)[0]}


HP = dict(lr=0.05, eps=1e-7, beta1=0.9, beta2=0.999, beta1t=0.81, beta2t=0.998001, weight_decay=0.1)


@pytest.mark.parametrize("kind", ["adagrad", "adam", "adamw"])
@pytest.mark.parametrize("width", [4, 64, 200])
def test_optimizers_sparse_opt_fused(dev, width, kind):
    """dedup (the serial chain from +0) + the row update in one call, on the raw ids of the run-length batch: the reduced
    gradient of a poisoned (key, column) is a NaN, an infinity, a subnormal or a signed zero before the optimizer sees it."""
    case = _small(width)
    state = _fused_state(case, 20)
    want_p, want_s = _fused_reference(kind, case, case.ids_f32, case.grads, state, HP)
    p = _dev(case.table, dev)
    names = ("acc",) if kind == "adagrad" else ("m", "v")
    d = [_dev(state[k], dev) for k in names]
    ops.sparse_opt_fused(kind, p, _dev(case.ids_f32, dev), _dev(case.grads, dev), d[0], d[1] if len(d) > 1 else None, **HP)
    torch.cuda.synchronize()
    _same("optimizers", _np(p), want_p, "sparse_opt_fused %s: param" % kind, poisoned=case.poisoned)
    for k, t in zip(names, d):
        _same("optimizers", _np(t), want_s[k], "sparse_opt_fused %s: %s" % (kind, k), poisoned=case.poisoned)


# ---- pooled forms --------------------------------------------------------------------------------------------------------------------
BAG = 25


@functools.lru_cache(maxsize=None)
def _pooled(width, layout):
    """The run-length batch of _small(width) as bags: fixed [320, 25], or ragged with an empty first bag, a ONE-ROW bag of a -0 row
    and an empty bag inside.  Table and pooled gradients carry sprinkled specials; two bags meet rows of 1.2e19 (S * S overflows
    while Q is finite) and of 2e19 (both infinite: fm is NaN there)."""
    case = _small(width)
    ids = case.ids.copy()
    table = sv.sprinkle(case.table, 40 + width, 0.03)[0]
    n = ids.size
    rng = np.random.default_rng([width, layout == "fixed"])
    if layout == "fixed":
        offsets = None
        shaped = ids.reshape(-1, BAG)
        nbags = shaped.shape[0]
        lo = np.arange(nbags) * BAG
    else:
        cuts = np.sort(rng.choice(np.arange(4, n), size=316, replace=False))
        offsets = np.concatenate([[0, 0, 1], cuts[:100], [cuts[99]], cuts[100:], [n]]).astype(np.int64)
        nbags = offsets.size - 1
        shaped = ids
        lo = offsets[:-1]
    hi = np.r_[lo[1:], n]
    ukeys, ucnt = np.unique(ids, return_counts=True)
    once = np.isin(ids, ukeys[ucnt == 1])             # occurrences of keys the batch names once
    big = [b for b in range(2, nbags) if once[lo[b]:hi[b]].sum() >= 2][:2]
    for b in big:
        table[ids[lo[b]:hi[b]], 0] = F(1.0)           # (no other special in this column of the two bags)
    for b, x in zip(big, (1.2e19, 2e19)):
        k0, k1 = ids[lo[b]:hi[b]][once[lo[b]:hi[b]]][:2]
        table[k0, 0] = table[k1, 0] = F(x)
    if layout == "ragged":
        table[ids[0]] = sv.NEG_ZERO                   # bag 1 is ids[0] alone
    bag_grads = sv.sprinkle(rng.standard_normal((nbags, width), dtype=np.float32), 50 + width, 0.03)[0]
    g_fm = sv.sprinkle(rng.standard_normal((nbags, width), dtype=np.float32), 60 + width, 0.03)[0]
    return dict(ids=shaped, flat=ids, offsets=offsets, table=table, bag_grads=bag_grads, g_fm=g_fm, nbags=nbags, big=big, lr=case.lr)


@functools.lru_cache(maxsize=None)
def _pooled_ref(width, layout, what):
    p = _pooled(width, layout)
    ids_f = p["ids"].astype(np.float32)
    with np.errstate(all="ignore"):
        if what == "sum":
            return bag_model.bag_sum(p["table"], ids_f, p["offsets"])
        if what == "fm":
            return fm_model.fm_lookup(p["table"], ids_f, p["offsets"])
        if what == "sgd_bags":
            return bag_model.sgd_bags(p["table"], ids_f, p["bag_grads"], p["lr"], p["offsets"])
        rows, covered, S, fm = _pooled_ref(width, layout, "fm")
        if what == "fm_grad_rows":
            g_rows = fm_pooled_model.expand(p["bag_grads"], p["flat"].size, p["nbags"], BAG if p["offsets"] is None else None, p["offsets"])
            return fm_model.fm_grad_rows(g_rows, rows, S, p["g_fm"], BAG if p["offsets"] is None else None, p["offsets"])
        if what == "fm_pooled_sgd":
            return fm_pooled_model.fm_pooled_sgd(p["table"], ids_f, p["bag_grads"], p["g_fm"], S, p["lr"], p["offsets"])
    raise ValueError(what)


@pytest.mark.parametrize("layout", ["fixed", "ragged"])
@pytest.mark.parametrize("width", [4, 64, 200])
def test_pooled_lookups(dev, width, layout):
    """embedding_lookup_sum: the documented chain 0 + r_0 + ...: a one-row bag of a -0 row gives +0.  embedding_lookup_fm: rows
    are copies; S the same chain; fm = 0.5 * (S*S - Q) is +inf where S*S overflows and Q is finite, NaN where both are infinite.
    fm_grad_rows on those outputs."""
    p = _pooled(width, layout)
    t = _dev(p["table"], dev)
    d_ids = _dev(p["ids"].astype(np.float32), dev)
    d_off = _dev(p["offsets"], dev) if p["offsets"] is not None else None
    want_sum = _pooled_ref(width, layout, "sum")
    rows, covered, S, fm = _pooled_ref(width, layout, "fm")
    if layout == "ragged":
        assert (sv.bits(want_sum[1]) == 0).all() and (sv.bits(p["table"][p["flat"][0]]) == 0x80000000).all()
    b0, b1 = p["big"]
    assert np.isposinf(fm[b0, 0]) and np.isnan(fm[b1, 0]) and np.isfinite(S[[b0, b1], 0]).all()
    got = ops.embedding_lookup_sum(t, d_ids, d_off)
    torch.cuda.synchronize()
    _same("pooled forms", _np(got), want_sum, "embedding_lookup_sum")
    g_rows, g_sum, g_fmo = ops.embedding_lookup_fm(t, d_ids, d_off)
    torch.cuda.synchronize()
    assert covered.all()
    _same("pooled forms", _np(g_rows).reshape(-1, width), rows, "embedding_lookup_fm: rows", copy=True, rows=p["flat"])
    _same("pooled forms", _np(g_sum), S, "embedding_lookup_fm: sum")
    _same("pooled forms", _np(g_fmo), fm, "embedding_lookup_fm: fm")
    n = p["flat"].size
    bag_of = ops.bag_of(d_off, n) if d_off is not None else None
    expanded = fm_pooled_model.expand(p["bag_grads"], n, p["nbags"], BAG if bag_of is None else None, p["offsets"])
    out = ops.fm_grad_rows(_dev(expanded, dev), _dev(rows, dev), _dev(S, dev), _dev(p["g_fm"], dev),
                           bag=BAG if bag_of is None else None, bag_of=bag_of)
    torch.cuda.synchronize()
    _same("pooled forms", _np(out).reshape(-1, width), _pooled_ref(width, layout, "fm_grad_rows"), "fm_grad_rows", rows=p["flat"])
    _same("pooled forms", _np(t), p["table"], "the table after the lookups", copy=True)


@pytest.mark.parametrize("layout", ["fixed", "ragged"])
@pytest.mark.parametrize("width", [4, 64, 200])
def test_pooled_applies(dev, width, layout):
    """sgd_apply_bags, sgd_apply_fm_bags and sparse_opt_fused_bags over every run length class, specials in the table and in the
    pooled gradients."""
    p = _pooled(width, layout)
    n = p["flat"].size
    d_ids = _dev(p["ids"].astype(np.float32), dev)
    d_off = _dev(p["offsets"], dev) if p["offsets"] is not None else None
    bag_of = ops.bag_of(d_off, n) if d_off is not None else None
    bag = BAG if bag_of is None else None
    plan = ops.IndexPlan(n, dev).build(d_ids)
    t = _dev(p["table"], dev)
    ops.sgd_apply_bags(t, plan, _dev(p["bag_grads"], dev), p["lr"], bag=bag, bag_of=bag_of)
    torch.cuda.synchronize()
    _same("pooled forms", _np(t), _pooled_ref(width, layout, "sgd_bags"), "sgd_apply_bags")
    S = _pooled_ref(width, layout, "fm")[2]
    t = _dev(p["table"], dev)
    ops.sgd_apply_fm_bags(t, plan, _dev(p["bag_grads"], dev), _dev(p["g_fm"], dev), _dev(S, dev), p["lr"], bag=bag, bag_of=bag_of)
    torch.cuda.synchronize()
    _same("pooled forms", _np(t), _pooled_ref(width, layout, "fm_pooled_sgd"), "sgd_apply_fm_bags")
    # the optimizers from pooled gradients: bit for bit the fused call on the expanded gradient (its reference above)
    case = _small(width)
    expanded = fm_pooled_model.expand(p["bag_grads"], n, p["nbags"], bag, p["offsets"])
    state = _fused_state(case, 30)
    for kind in ("adagrad", "adamw"):
        pooled_case = sv.Case(case.name + "-pooled", case.ids, expanded, p["table"], expanded, p["table"], case.poisoned, (), case.runs,
                              case.lr)
        want_p, want_s = _fused_reference(kind, pooled_case, case.ids_f32, expanded, state, HP)
        prm = _dev(p["table"], dev)
        names = ("acc",) if kind == "adagrad" else ("m", "v")
        d = [_dev(state[k], dev) for k in names]
        ops.sparse_opt_fused_bags(kind, prm, d_ids, _dev(p["bag_grads"], dev), d[0], d[1] if len(d) > 1 else None, offsets=d_off, **HP)
        torch.cuda.synchronize()
        _same("pooled forms", _np(prm), want_p, "sparse_opt_fused_bags %s: param" % kind)
        for k, x in zip(names, d):
            _same("pooled forms", _np(x), want_s[k], "sparse_opt_fused_bags %s: %s" % (kind, k))


# ---- sharded table, world size 1 -----------------------------------------------------------------------------------------------------
def test_sharded_table_world_size_1(dev):
    from herald_amd.sharded import ShardedEmbedding
    width = 64
    case = _small(width)
    table = sv.sprinkle(case.table, 70, 0.03)[0]
    emb = ShardedEmbedding(case.rows, width, dev, table=_dev(table, dev))
    d_ids = _dev(case.ids_f32, dev)
    out, route = emb.pull(d_ids, return_route=True)
    torch.cuda.synchronize()
    _same("sharded table", _np(out), table[case.ids], "ShardedEmbedding.pull", copy=True, rows=case.ids)
    emb.push(d_ids, _dev(case.grads, dev), case.lr, route=route)
    torch.cuda.synchronize()
    with np.errstate(all="ignore"):
        want = cpu.sparse_push(table.copy(), case.ids_f32, case.grads, case.lr)
    _same("sharded table", _np(emb.table), want, "ShardedEmbedding.push", poisoned=case.poisoned)
    # the pooled forms on the table the push left
    p = _pooled(width, "fixed")
    bags = _dev(p["ids"].astype(np.float32), dev)
    got = emb.pull_sum(bags)
    torch.cuda.synchronize()
    with np.errstate(all="ignore"):
        _same("sharded table", _np(got), bag_model.bag_sum(want, p["ids"].astype(np.float32)), "ShardedEmbedding.pull_sum")
        expanded = fm_pooled_model.expand(p["bag_grads"], case.n, p["nbags"], BAG)
        want2 = cpu.sparse_push(want.copy(), case.ids_f32, expanded, case.lr)
    emb.push_bags(bags, _dev(p["bag_grads"], dev), case.lr)
    torch.cuda.synchronize()
    _same("sharded table", _np(emb.table), want2, "ShardedEmbedding.push_bags")


# ---- planned cache pair --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["lru", "lfu"])
def test_planned_cache_pair(dev, policy):
    """One block of plan_block + embedding_lookup_planned + embedding_update_planned: specials in the store's rows and in the
    gradients of keys that are hit, missed, evicted and pushed.  Returned rows (the first lookup moves rows only: raw bits), the
    backing table after the pushes, and every line's data and gradient arrays, against oracle/cache_model.py."""
    limit, rows, width, n, steps = 100, 1500, 8, 64, 8
    rng = np.random.default_rng(81)
    table0 = sv.sprinkle(rng.standard_normal((rows, width), dtype=np.float32), 82, 0.05)[0]
    server = cache_model.Server(table0)
    model = cache_model.CacheModel(policy, limit, width, server, 1, 1)
    table = _dev(table0, dev)
    versions = torch.zeros(rows, dtype=torch.int64, device=dev)
    gpu = {"lru": hcache.LRUCache, "lfu": hcache.LFUCache}[policy](limit, rows, width, node_id=0, max_batch=n, device=dev)
    gpu.bind_store(table, versions)
    gpu.pull_bound, gpu.push_bound = 1, 1
    gpu.perf_enabled = True
    keys_all = [(np.minimum(rng.zipf(1.3, size=n) - 1, rows - 1).astype(np.int64) * 7919) % rows for _ in range(steps)]
    gpu.plan_block([_dev(k.astype(np.float32), dev) for k in keys_all])
    hits = evicted = 0
    for step, keys in enumerate(keys_all):
        grads = sv.sprinkle(rng.standard_normal((n, width), dtype=np.float32) * F(-0.01), 90 + step, 0.1)[0]
        with np.errstate(all="ignore"):
            want = model.lookup(keys.astype(np.uint64))
        hits += model.perf[-1]["num_unique"] - model.perf[-1]["num_miss"]
        dest = torch.empty((n, width), dtype=torch.float32, device=dev)
        gpu.embedding_lookup_planned(dest).wait()
        _same("planned cache pair", _np(dest), want, "%s: lookup rows of step %d" % (policy, step), copy=step == 0, rows=keys)
        with np.errstate(all="ignore"):
            model.update(keys.astype(np.uint64), grads)
        evicted += sum(p.get("num_evict", 0) for p in model.perf[-2:] if p["type"] == "Push")
        gpu.embedding_update_planned(_dev(grads, dev)).wait()
        for got, exp in zip(gpu.perf[-2:], model.perf[-2:]):
            for f in ("type", "num_all", "num_unique", "num_miss", "num_transfered"):
                assert got[f] == exp[f], (step, f, got, exp)
        _same("planned cache pair", _np(table), server.table, "%s: backing table after step %d" % (policy, step))
        np.testing.assert_array_equal(_np(versions), server.ver)
    assert gpu.plan_pending() == 0 and hits > 0 and evicted > 0
    assert (sv.bits(table0) != sv.bits(server.table)).any()            # pushes reached the store
    res, lines = model.resident(), gpu.lines()
    assert sorted(lines.keys()) == sorted(res.keys())
    for k, ln in res.items():
        assert lines[k].version == ln.version and lines[k].updates == ln.updates, k
        _same("planned cache pair", lines[k].data, ln.data, "%s: data of line %d" % (policy, k))
        if ln.grad is not None:
            _same("planned cache pair", lines[k].grad, ln.grad, "%s: gradient of line %d" % (policy, k))

"""The stream contract of every op that takes `stream=` (herald_amd/ops.py module docstring, include/herald_amd.h next to
ha_stream_t): one registry row per call, for tests/test_stream_contract_cpu.py and tests/test_gpu_stream_contract.py.  Test
infrastructure only: nothing under herald_amd/ imports it, and this module needs numpy and the CPU models alone.

A row (Entry) gives
  uses         the names of the device inputs of the call, out of the WORLD of a variant (below);
  call         call(t, stream, st) -> {name: device tensor}: the call under test on the device tensors t[name];
  prep         (optional) prep(t, stream, st): what the call takes that is DERIVED from the inputs on the same stream -- a plan
               built or sorted from the ids.  It runs once behind the decoy writes and once behind the real ones, so a plan is as
               late as the ids it is built from;
  model        model(a, v) -> {name: numpy array}: the expected result from the CPU models the suite already has, applied to
               the numpy inputs a[name].  Compared bit for bit, except the optimizer rows (atol), which the existing tests of
               those ops compare within 1e-5 of the numpy oracle (tests/test_gpu_optim.py);
  synchronous  the call returns a count to the host, so it waits for the stream; `why` says which count.

The WORLD of a variant is every array any row may use, drawn from one seed: ids (fixed bags [B, F] or ragged [n] + offsets),
a table, gradients, weights with dead occurrences, states, and what is derived from them on the CPU (bag_of, the inverse as
uint32 keys, a position map).  The DECOY of every input is the same array of the world of another seed, with the ids replaced by
late_ids.decoy_of (of the real ids rolled by one position): valid ids of another unique set, monotone offsets with the same n
and B, weights with another live/dead pattern, finite floats.  A misordered read gives wrong numbers, never an access out of
range.  A dl_call row names the reference-named symbol it calls (`symbol`): every symbol bound with a DLStream has one."""
import functools

import numpy as np

import bag_model
import fm_model
import fm_pooled_model
import wbag_model
import wfm_model
import wshard_model
from oracle import cpu

F32 = np.float32
LR = 0.37                       # not a power of two: lr * g rounds
SCALE = -0.37
B, F = 8, 26
BIG_B = 1500                    # 1,500 x 26 = 39,000 ids > 36,864: the plan built inside a call is a radix sort in the scratch
HYPER = dict(lr=0.01, eps=1e-7, beta1=0.9, beta2=0.999, beta1t=0.9, beta2t=0.999, weight_decay=0.01)
MOMENTUM = 0.9
OPT_ATOL = 1e-5                 # the tolerance of tests/test_gpu_optim.py (the reference test's atol)


def decoy_of(real, rows):
    """late_ids.decoy_of, restated here so that this module needs no GPU library: (real + rows // 2) % rows."""
    real = np.asarray(real)
    ints = real.astype(np.int64)
    assert real.size > 0 and ints.min() >= 0 and ints.max() < rows
    d = (ints + rows // 2) % rows
    assert not np.array_equal(np.unique(d), np.unique(ints)), "the decoy names the unique set of the real ids"
    return d.astype(real.dtype).reshape(real.shape)


class Variant:
    def __init__(self, width, idt, ragged, big=False):
        self.width, self.idt, self.ragged, self.big = width, idt, ragged, big
        self.nbags = BIG_B if big else B
        self.n = self.nbags * F
        self.rows = 100000 if big else 2000
        self.id = "%s-d%d-%s-%s" % ("big" if big else "small", width, "f32" if idt == np.float32 else "i64",
                                   "ragged" if ragged else "fixed")

    def __repr__(self):
        return self.id


def _offsets(rng, n, nbags):
    """Monotone, offsets[0] = 0, offsets[B] = n, with an empty bag and a long one."""
    cuts = np.sort(rng.integers(0, n + 1, size=nbags - 1))
    if nbags > 3:
        cuts[1] = cuts[0]
    return np.concatenate([[0], cuts, [n]]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _world(width, idt, ragged, big, seed, decoy_for=None):
    v = Variant(width, idt, ragged, big)
    rng = np.random.default_rng(seed)
    n, nb, rows = v.n, v.nbags, v.rows
    w = {}
    hot = rng.integers(0, 40, size=n)
    cold = rng.integers(0, rows // 2 - 1, size=n)          # (the real ids leave half of the rows to the decoy)
    flat = np.where(rng.random(n) < 0.3, hot, cold)
    if decoy_for is not None:
        # (of the real ids rolled by one: the shift alone keeps their order, and with it a plan's perm and inverse)
        flat = decoy_of(np.roll(_world(width, idt, ragged, big, decoy_for)["ids"].reshape(-1), 1), rows).astype(np.int64)
    w["ids"] = flat.astype(idt) if ragged else flat.astype(idt).reshape(nb, F)
    w["offsets"] = _offsets(rng, n, nb) if ragged else None
    w["which"] = bag_model.bag_of(w["offsets"], n).astype(np.int64) if ragged else np.arange(n) // F
    w["bag_of"] = w["which"].astype(np.int32)
    w["table"] = rng.standard_normal((rows, width), dtype=F32)
    w["grads"] = rng.standard_normal((n, width), dtype=F32)
    w["emb_rows"] = rng.standard_normal((n, width), dtype=F32)
    w["rows_buf"] = rng.standard_normal((n, width), dtype=F32)
    w["dst"] = rng.standard_normal((n, width), dtype=F32)
    # a buffer the caller pre-zeroes (DeduplicateIndexedSlices' compressed rows): the decoy is not zero
    w["zeros"] = np.zeros((n, width), dtype=F32) if decoy_for is None else rng.standard_normal((n, width), dtype=F32)
    for name in ("bg", "bg2", "S"):
        w[name] = rng.standard_normal((nb, width), dtype=F32)
    w["bg_wide"] = rng.standard_normal((nb, 2 * width), dtype=F32)      # its even columns are a strided [B, width] view
    wts = rng.standard_normal(n, dtype=F32)
    wts[rng.random(n) < 0.3] = 0
    wts[0] = 0 if decoy_for is None else 1.5                # (the live/dead pattern differs for certain)
    w["weights"] = wts
    w["state1"] = np.abs(rng.standard_normal((rows, width), dtype=F32))
    w["state2"] = np.abs(rng.standard_normal((rows, width), dtype=F32))
    w["veloc"] = rng.standard_normal((rows, width), dtype=F32)
    uniq, inverse = np.unique(flat, return_inverse=True)
    w["invf"] = inverse.astype(F32)                                   # the inverse as the reference hands it on: float32
    w["keys"] = inverse.astype(np.int32).reshape(w["ids"].shape)      # uint32 keys into rows_buf / dst (all below n)
    pos = np.where(np.arange(n) % 2 == 0, flat.astype(np.uint32) | np.uint32(0x80000000), inverse.astype(np.uint32))
    w["posmap"] = pos.astype(np.uint32).view(np.int32)
    # distinct ids (what the symbols on deduplicated slices and IndexedSlices2Dense take), and a push set
    lo = 0 if decoy_for is None else rows // 2
    w["uids"] = (lo + rng.permutation(rows // 2)[:n]).astype(F32) if rows // 2 >= n else None
    w["pids"] = w["ids"].reshape(-1)[::3].astype(F32).copy()
    w["rowmap"] = np.arange(n, dtype=np.int32) if decoy_for is None else np.arange(n, dtype=np.int32)[::-1].copy()
    w["dst_init"] = np.full(n, 1 if decoy_for is None else 0, dtype=np.uint8)
    for a in w.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return w


def world(v, seed=0):
    return _world(v.width, v.idt, v.ragged, v.big, seed)


def decoy_world(v, seed=0):
    return _world(v.width, v.idt, v.ragged, v.big, seed + 7919, decoy_for=seed)


# ---- the registry ------------------------------------------------------------------------------------------------------------
class Entry:
    def __init__(self, name, target, uses, call, model, prep=None, layouts="both", f32only=False, big=False, atol=None,
                 synchronous=False, why="", symbol=None):
        self.name, self.target, self.uses, self.call, self.model, self.prep = name, target, tuple(uses), call, model, prep
        self.layouts, self.f32only, self.big, self.atol = layouts, f32only, big, atol
        self.synchronous, self.why = synchronous, why
        self.symbol = symbol         # dl_call rows: the reference-named symbol the row calls directly
        assert not synchronous or why, "a synchronous row says which count the call returns"

    def variants(self):
        lays = {"both": (False, True), "fixed": (False,), "ragged": (True,)}[self.layouts]
        narrow = np.float32 if self.f32only else np.int64
        out = [Variant(64, np.float32, r) for r in lays] + [Variant(5, narrow, r) for r in lays]
        if self.big:
            out.append(Variant(16, np.float32, self.layouts == "ragged", big=True))
        return out

    def inputs(self, v, decoy=False):
        """{name: numpy array} of the device inputs of this row (None entries, the offsets of fixed bags, left out)."""
        w = decoy_world(v) if decoy else world(v)
        return {k: w[k] for k in self.uses if w[k] is not None and (v.ragged or k != "bag_of")}      # (fixed bags: bag=F)


REGISTRY = []


def row(*a, **kw):
    REGISTRY.append(Entry(*a, **kw))


def _ops():
    from herald_amd import ops
    return ops


def _hetu():
    from herald_amd import hetu_ops
    return hetu_ops


def _bagkw(t, st=None):
    """bag= for fixed bags, bag_of= for ragged ones (the rows that take a plan and either)."""
    return dict(bag_of=t["bag_of"]) if "offsets" in t else dict(bag=F)


def _off(a):
    return a.get("offsets")


def _plan(build):
    """prep: a plan of the ids, sorted ('sort'), finished ('build'), or only allocated ('none'), on the call's stream."""
    def prep(t, stream, st):
        ops = _ops()
        if "plan" not in st:
            st["plan"] = ops.IndexPlan(t["ids"].numel(), t["ids"].device)
        ids = t["ids"].reshape(-1)
        if build == "sort":
            st["plan"].sort(ids, stream)
        elif build == "build":
            st["plan"].build(ids, stream)
    return prep


def _uniq(a):
    return np.unique(bag_model.ids_to_rows(a["ids"]), return_inverse=True)


def _gather(a, v):
    return {"out": wfm_model.gather(a["table"], a["ids"]).reshape(a["ids"].shape + (v.width,))}


def _which(a):
    n = np.asarray(a["ids"]).size if "ids" in a else a["weights"].size
    off = _off(a)
    return np.arange(n) // F if off is None else bag_model.bag_of(off, n).astype(np.int64)


def _flat_ids(a):
    return np.asarray(a["ids"]).reshape(-1)


def _ps_push(a, grads, lr):
    return {"table": fm_model.ps_push(a["table"], _flat_ids(a), grads, lr)}


BAGS = ("ids", "offsets")

# -- herald_amd/ops.py, in the order of the file ---------------------------------------------------------------------------------
row("embedding_lookup", "ops.embedding_lookup", ("table", "ids"),
    lambda t, s, st: {"out": _ops().embedding_lookup(t["table"], t["ids"], stream=s)}, _gather)
row("dedup_reduce", "ops.dedup_reduce", ("ids", "grads"),
    lambda t, s, st: {"out": _ops().dedup_reduce(st["plan"], t["grads"], stream=s)},
    lambda a, v: {"out": cpu.dedup_reduce(_flat_ids(a), a["grads"])[2]}, prep=_plan("build"))
row("dedup_reduce[scale]", "ops.dedup_reduce", ("ids", "grads"),
    lambda t, s, st: {"out": _ops().dedup_reduce(st["plan"], t["grads"], stream=s, scale=SCALE)},
    lambda a, v: {"out": wshard_model.reduce_rows_scaled(_uniq(a)[1], _uniq(a)[0].size, a["grads"], SCALE)}, prep=_plan("build"))
row("sgd_apply", "ops.sgd_apply", ("table", "ids", "grads"),
    lambda t, s, st: {"table": _ops().sgd_apply(t["table"], st["plan"], t["grads"], LR, stream=s)},
    lambda a, v: {"table": fm_model.sgd_serial(a["table"], _flat_ids(a), a["grads"], LR)}, prep=_plan("sort"))
row("sgd_apply[finished]", "ops.sgd_apply", ("table", "ids", "grads"),
    lambda t, s, st: {"table": _ops().sgd_apply(t["table"], st["plan"], t["grads"], LR, stream=s, finished=True)},
    lambda a, v: {"table": fm_model.sgd_serial(a["table"], _flat_ids(a), a["grads"], LR)}, prep=_plan("build"))
row("push_apply", "ops.push_apply", ("table", "ids", "grads"),
    lambda t, s, st: {"table": _ops().push_apply(t["table"], st["plan"], t["grads"], stream=s)},
    lambda a, v: _ps_push(a, a["grads"], -1.0), prep=_plan("sort"))
row("sgd_sparse_update", "ops.sgd_sparse_update", ("table", "ids", "grads"),
    lambda t, s, st: {"table": _ops().sgd_sparse_update(t["table"], t["ids"], t["grads"], LR, stream=s)},
    lambda a, v: {"table": fm_model.sgd_serial(a["table"], _flat_ids(a), a["grads"], LR)}, f32only=True, big=True)
row("embedding_lookup_sum", "ops.embedding_lookup_sum", ("table",) + BAGS,
    lambda t, s, st: {"out": _ops().embedding_lookup_sum(t["table"], t["ids"], t.get("offsets"), stream=s)},
    lambda a, v: {"out": bag_model.bag_sum(a["table"], a["ids"], _off(a))})


def _fm_lookup(a, v):
    rows, covered, S, fm = fm_model.fm_lookup(a["table"], a["ids"], _off(a))
    assert covered.all()
    return {"rows": rows.reshape(a["ids"].shape + (v.width,)), "sum": S, "fm": fm}


row("embedding_lookup_fm", "ops.embedding_lookup_fm", ("table",) + BAGS,
    lambda t, s, st: dict(zip(("rows", "sum", "fm"), _ops().embedding_lookup_fm(t["table"], t["ids"], t.get("offsets"), stream=s))),
    _fm_lookup)
row("fm_grad_rows", "ops.fm_grad_rows", ("grads", "emb_rows", "S", "bg2", "bag_of", "offsets"),
    lambda t, s, st: {"out": _ops().fm_grad_rows(t["grads"], t["emb_rows"], t["S"], t["bg2"], stream=s, **_bagkw(t))},
    lambda a, v: {"out": fm_model.fm_grad_rows(a["grads"], a["emb_rows"], a["S"], a["bg2"], bag=F, offsets=_off(a))})
row("gather_sum_u32keys", "ops.gather_sum_u32keys", ("rows_buf", "keys", "offsets"),
    lambda t, s, st: {"out": _ops().gather_sum_u32keys(t["rows_buf"], t["keys"], offsets=t.get("offsets"), stream=s)},
    lambda a, v: {"out": bag_model.bag_sum(a["rows_buf"], a["keys"].astype(np.int64), _off(a))})


def _gather2_model(a, v):
    m = a["posmap"].view(np.uint32)
    idx = (m & np.uint32(0x7FFFFFFF)).astype(np.int64)
    rows = np.where(((m >> 31) != 0)[:, None], a["table"][np.minimum(idx, a["table"].shape[0] - 1)],
                    a["rows_buf"][np.minimum(idx, a["rows_buf"].shape[0] - 1)]).astype(F32)
    pos = np.arange(m.size, dtype=np.int64)
    return {"out": bag_model.bag_sum(rows, pos if _off(a) is not None else pos.reshape(-1, F), _off(a))}


def _mapped_model(a):
    """ha_apply_mapped: dst[rowmap[u]] = (dst_init[rowmap[u]] ? dst[rowmap[u]] : 0) - lr * g_i0 - lr * g_i1 ... per unique key u."""
    uniq, inv = _uniq(a)
    dst, touched = a["dst"].copy(), a["rowmap"][:uniq.size]
    dst[touched[a["dst_init"][touched] == 0]] = 0
    return {"dst": fm_model.sgd_serial(dst, a["rowmap"][inv], a["bg"][_which(a)], LR)}


row("gather2_sum_u32map", "ops.gather2_sum_u32map", ("table", "rows_buf", "posmap", "offsets"),
    lambda t, s, st: {"out": _ops().gather2_sum_u32map(t["table"], t["rows_buf"], t["posmap"],
                                                       bag=None if "offsets" in t else F, offsets=t.get("offsets"), stream=s)},
    _gather2_model)
row("apply_mapped_bags", "ops.apply_mapped_bags", ("dst", "ids", "bg", "rowmap", "dst_init", "bag_of", "offsets"),
    lambda t, s, st: {"dst": _ops().apply_mapped_bags(t["dst"], st["plan"], t["bg"], LR, rowmap=t["rowmap"],
                                                      dst_init=t["dst_init"], stream=s, **_bagkw(t))},
    lambda a, v: _mapped_model(a), prep=_plan("build"))
row("push_apply_scaled_bags_finished", "ops.push_apply_scaled_bags_finished", ("table", "ids", "bg", "bag_of", "offsets"),
    lambda t, s, st: {"table": _ops().push_apply_scaled_bags_finished(t["table"], st["plan"], t["bg"], SCALE, stream=s, **_bagkw(t))},
    lambda a, v: _ps_push(a, a["bg"][_which(a)], -SCALE), prep=_plan("build"))
row("dedup_reduce_bags", "ops.dedup_reduce_bags", ("ids", "bg", "bag_of", "offsets"),
    lambda t, s, st: {"out": _ops().dedup_reduce_bags(st["plan"], t["bg"], stream=s, **_bagkw(t))},
    lambda a, v: {"out": cpu.dedup_reduce(_flat_ids(a), a["bg"][_which(a)])[2]}, prep=_plan("build"))
row("bag_of", "ops.bag_of", ("offsets",),
    lambda t, s, st: {"out": _ops().bag_of(t["offsets"], (t["offsets"].numel() - 1) * F, stream=s)},
    lambda a, v: {"out": bag_model.bag_of(a["offsets"], v.n)}, layouts="ragged")
row("sgd_apply_bags", "ops.sgd_apply_bags", ("table", "ids", "bg", "bag_of", "offsets"),
    lambda t, s, st: {"table": _ops().sgd_apply_bags(t["table"], st["plan"], t["bg"], LR, stream=s, **_bagkw(t))},
    lambda a, v: {"table": bag_model.sgd_bags(a["table"], a["ids"], a["bg"], LR, _off(a))}, prep=_plan("sort"))
row("sgd_sparse_update_bags", "ops.sgd_sparse_update_bags", ("table", "bg") + BAGS,
    lambda t, s, st: {"table": _ops().sgd_sparse_update_bags(t["table"], t["ids"], t["bg"], LR, t.get("offsets"), stream=s)},
    lambda a, v: {"table": bag_model.sgd_bags(a["table"], a["ids"], a["bg"], LR, _off(a))}, big=True)


def _fm_sgd(a, v, g_sum="bg"):
    return {"table": fm_pooled_model.fm_pooled_sgd(a["table"], a["ids"], a[g_sum] if g_sum else None, a["bg2"], a["S"], LR, _off(a))}


row("sgd_apply_fm_bags", "ops.sgd_apply_fm_bags", ("table", "ids", "bg", "bg2", "S", "bag_of", "offsets"),
    lambda t, s, st: {"table": _ops().sgd_apply_fm_bags(t["table"], st["plan"], t["bg"], t["bg2"], t["S"], LR, stream=s, **_bagkw(t))},
    _fm_sgd, prep=_plan("build"))
row("sgd_sparse_update_fm_bags", "ops.sgd_sparse_update_fm_bags", ("table", "bg", "bg2", "S") + BAGS,
    lambda t, s, st: {"table": _ops().sgd_sparse_update_fm_bags(t["table"], t["ids"], t["bg"], t["bg2"], t["S"], LR,
                                                                t.get("offsets"), stream=s)}, _fm_sgd, big=True)
row("embedding_lookup_wsum", "ops.embedding_lookup_wsum", ("table", "weights") + BAGS,
    lambda t, s, st: {"out": _ops().embedding_lookup_wsum(t["table"], t["ids"], t["weights"], t.get("offsets"), stream=s)},
    lambda a, v: {"out": wbag_model.wbag_sum(a["table"], a["ids"], a["weights"], _off(a))})
row("wbag_grad_rows", "ops.wbag_grad_rows", ("bg", "weights", "bag_of", "offsets"),
    lambda t, s, st: {"out": _ops().wbag_grad_rows(t["bg"], t["weights"], stream=s, **_bagkw(t))},
    lambda a, v: {"out": wbag_model.wbag_grad_rows(a["bg"], a["weights"], _which(a))})
row("sgd_apply_wbags", "ops.sgd_apply_wbags", ("table", "ids", "bg", "weights", "bag_of", "offsets"),
    lambda t, s, st: {"table": _ops().sgd_apply_wbags(t["table"], st["plan"], t["bg"], t["weights"], LR, stream=s, **_bagkw(t))},
    lambda a, v: {"table": wbag_model.wbag_sgd(a["table"], a["ids"], a["weights"], a["bg"], LR, _off(a))}, prep=_plan("build"))
row("sgd_sparse_update_wbags", "ops.sgd_sparse_update_wbags", ("table", "bg", "weights") + BAGS,
    lambda t, s, st: {"table": _ops().sgd_sparse_update_wbags(t["table"], t["ids"], t["bg"], t["weights"], LR, t.get("offsets"),
                                                              stream=s)},
    lambda a, v: {"table": wbag_model.wbag_sgd(a["table"], a["ids"], a["weights"], a["bg"], LR, _off(a))}, big=True)
row("gather_wsum_u32keys", "ops.gather_wsum_u32keys", ("rows_buf", "keys", "weights", "offsets"),
    lambda t, s, st: {"out": _ops().gather_wsum_u32keys(t["rows_buf"], t["keys"], t["weights"], offsets=t.get("offsets"), stream=s)},
    lambda a, v: {"out": wshard_model.gather_wsum_u32keys(a["rows_buf"], a["keys"], a["weights"], bag=F, offsets=_off(a))})
row("dedup_reduce_wbags", "ops.dedup_reduce_wbags", ("ids", "bg", "weights", "bag_of", "offsets"),
    lambda t, s, st: {"out": _ops().dedup_reduce_wbags(st["plan"], t["bg"], t["weights"], scale=SCALE, stream=s, **_bagkw(t))},
    lambda a, v: {"out": wshard_model.dedup_reduce_wbags(_uniq(a)[1], _uniq(a)[0].size, a["bg"], a["weights"], _which(a), SCALE)},
    prep=_plan("build"))
row("embedding_lookup_wfm", "ops.embedding_lookup_wfm", ("table", "weights") + BAGS,
    lambda t, s, st: dict(zip(("sum", "sq"), _ops().embedding_lookup_wfm(t["table"], t["ids"], t["weights"], t.get("offsets"),
                                                                         stream=s))),
    lambda a, v: dict(zip(("sum", "sq"), wfm_model.wfm_lookup(a["table"], a["ids"], a["weights"], _off(a)))))
row("wfm_grad_rows", "ops.wfm_grad_rows", ("bg", "bg2", "weights", "emb_rows", "bag_of", "offsets"),
    lambda t, s, st: {"out": _ops().wfm_grad_rows(t["bg"], t["bg2"], t["weights"], t["emb_rows"], stream=s, **_bagkw(t))},
    lambda a, v: {"out": wfm_model.wfm_grad_rows(a["bg"], a["bg2"], a["weights"], a["emb_rows"], _which(a))})


def _wfm_sgd(a, v):
    return {"table": wfm_model.wfm_sgd(a["table"], a["ids"], a["weights"], a["bg"], a["bg2"], LR, _off(a))}


row("sgd_apply_wfm_bags", "ops.sgd_apply_wfm_bags", ("table", "ids", "bg", "bg2", "weights", "bag_of", "offsets"),
    lambda t, s, st: {"table": _ops().sgd_apply_wfm_bags(t["table"], st["plan"], t["bg"], t["bg2"], t["weights"], LR, stream=s,
                                                         **_bagkw(t))}, _wfm_sgd, prep=_plan("build"))
row("sgd_sparse_update_wfm_bags", "ops.sgd_sparse_update_wfm_bags", ("table", "bg", "bg2", "weights") + BAGS,
    lambda t, s, st: {"table": _ops().sgd_sparse_update_wfm_bags(t["table"], t["ids"], t["bg"], t["bg2"], t["weights"], LR,
                                                                 t.get("offsets"), stream=s)}, _wfm_sgd, big=True)
row("lookup_sort", "ops.lookup_sort", ("table", "ids"),
    lambda t, s, st: {"out": _ops().lookup_sort(t["table"], t["ids"], st["plan"], stream=s)}, _gather, prep=_plan("none"))
row("sgd_apply_finish", "ops.sgd_apply_finish", ("table", "ids", "grads"),
    lambda t, s, st: {"table": _ops().sgd_apply_finish(t["table"], st["plan"], t["grads"], LR, stream=s)},
    lambda a, v: {"table": fm_model.sgd_serial(a["table"], _flat_ids(a), a["grads"], LR)}, prep=_plan("sort"))
row("push_apply_finish", "ops.push_apply_finish", ("table", "ids", "grads"),
    lambda t, s, st: {"table": _ops().push_apply_finish(t["table"], st["plan"], t["grads"], stream=s)},
    lambda a, v: _ps_push(a, a["grads"], -1.0), prep=_plan("sort"))


def _pend(sorted_too):
    """prep of the two building blocks of a push-pull sequence: a plan and an idle PendingTable; for the apply, the batch sorted
    and registered by lookup_sort_pend on the same stream."""
    def prep(t, stream, st):
        ops = _ops()
        if "plan" not in st:
            st["plan"] = ops.IndexPlan(t["ids"].numel(), t["ids"].device)
            st["pend"] = ops.PendingTable(t["ids"].device)
            st["rows"] = t["table"].new_empty(tuple(t["ids"].shape) + (t["table"].shape[1],))
        st["pend"].reset(stream)
        if sorted_too:
            ops.lookup_sort_pend(t["table"], t["ids"], st["plan"], st["pend"], out=st["rows"], stream=stream)
    return prep


row("lookup_sort_pend", "ops.lookup_sort_pend", ("table", "ids"),
    lambda t, s, st: {"out": _ops().lookup_sort_pend(t["table"], t["ids"], st["plan"], st["pend"], stream=s)}, _gather,
    prep=_pend(False))
row("sgd_push_pull[last batch]", "ops.sgd_push_pull", ("table", "ids", "grads"),
    lambda t, s, st: (_ops().sgd_push_pull(t["table"], st["plan"], t["grads"], LR, st["pend"], stream=s), {"table": t["table"]})[1],
    lambda a, v: {"table": fm_model.sgd_serial(a["table"], _flat_ids(a), a["grads"], LR)}, prep=_pend(True))


# -- the optimizers: the numpy oracle on the deduplicated slices, within OPT_ATOL (tests/test_gpu_optim.py) ------------------
def _opt_model(kind, grads_of):
    def model(a, v):
        p, s1, s2 = a["table"].copy(), a["state1"].copy(), a["state2"].copy()
        uniq, _, red = cpu.dedup_reduce(_flat_ids(a), grads_of(a))
        h = HYPER
        if kind == "adagrad":
            cpu.adagrad_sparse(p, s1, uniq, red, h["lr"], h["eps"])
            return {"table": p, "state1": s1}
        cpu.adam_sparse(p, s1, s2, uniq, red, h["lr"], h["beta1"], h["beta2"], F32(h["beta1t"]), F32(h["beta2t"]), h["eps"],
                        h["weight_decay"] if kind == "adamw" else None)
        return {"table": p, "state1": s1, "state2": s2}
    return model


def _opt_out(t, kind):
    return {k: t[k] for k in (("table", "state1") if kind == "adagrad" else ("table", "state1", "state2"))}


def _hyper(kind):
    h = dict(HYPER)
    if kind != "adamw":
        h.pop("weight_decay")
    if kind == "adagrad":
        h = dict(lr=h["lr"], eps=h["eps"])
    return h


def _expanded(a):
    return a["bg"][_which(a)]


for _kind in ("adagrad", "adam", "adamw"):
    row("sparse_opt_fused[%s]" % _kind, "ops.sparse_opt_fused", ("table", "ids", "grads", "state1", "state2"),
        lambda t, s, st, k=_kind: (_ops().sparse_opt_fused(k, t["table"], t["ids"].reshape(-1), t["grads"], t["state1"], t["state2"],
                                                           stream=s, **_hyper(k)), _opt_out(t, k))[1],
        _opt_model(_kind, lambda a: a["grads"]), big=True, atol=OPT_ATOL)
    row("sparse_opt_fused_bags[%s]" % _kind, "ops.sparse_opt_fused_bags", ("table", "bg", "state1", "state2") + BAGS,
        lambda t, s, st, k=_kind: (_ops().sparse_opt_fused_bags(k, t["table"], t["ids"], t["bg"], t["state1"], t["state2"],
                                                                offsets=t.get("offsets"), stream=s, **_hyper(k)), _opt_out(t, k))[1],
        _opt_model(_kind, _expanded), big=True, atol=OPT_ATOL)


def _momentum_model(grads_of, nesterov):
    def model(a, v):
        p, vel = a["table"].copy(), a["veloc"].copy()
        cpu.momentum_sparse(p, vel, bag_model.ids_to_rows(a["ids"]), grads_of(a), HYPER["lr"], MOMENTUM, nesterov)
        return {"table": p, "veloc": vel}
    return model


for _nest in (False, True):
    row("momentum_sparse_update_bags[nesterov=%s]" % _nest, "ops.momentum_sparse_update_bags", ("table", "bg", "veloc") + BAGS,
        lambda t, s, st, nv=_nest: (_ops().momentum_sparse_update_bags(t["table"], t["ids"], t["bg"], t["veloc"], HYPER["lr"], MOMENTUM,
                                                                       nv, offsets=t.get("offsets"), stream=s),
                                    {"table": t["table"], "veloc": t["veloc"]})[1],
        _momentum_model(_expanded, _nest), big=True, atol=OPT_ATOL)


# -- dl_call on the reference-named symbols ------------------------------------------------------------------------------------
def _c(x):
    import ctypes
    return ctypes.c_float(x)


row("dl_call[DLGpuEmbeddingLookUp]", "ops.dl_call", ("table", "ids"),
    lambda t, s, st: (_ops().dl_call("DLGpuEmbeddingLookUp", [t["table"], t["ids"], st["out"]], stream=s), {"out": st["out"]})[1],
    _gather, f32only=True, symbol="DLGpuEmbeddingLookUp",       # (the output is the caller's: allocated with the inputs, before anything is late)
    prep=lambda t, s, st: st.setdefault("out", t["table"].new_empty(tuple(t["ids"].shape) + (t["table"].shape[1],))))
row("dl_call[SGDOptimizerSparseUpdate]", "ops.dl_call", ("table", "ids", "grads"),
    lambda t, s, st: (_ops().dl_call("SGDOptimizerSparseUpdate", [t["table"], t["ids"], t["grads"]], scalars=[_c(LR)], stream=s),
                      {"table": t["table"]})[1],
    lambda a, v: {"table": fm_model.sgd_serial(a["table"], _flat_ids(a), a["grads"], LR)}, f32only=True, big=True,
    symbol="SGDOptimizerSparseUpdate")
row("dl_call[MomentumOptimizerSparseUpdate]", "ops.dl_call", ("table", "ids", "grads", "veloc"),
    lambda t, s, st: (_ops().dl_call("MomentumOptimizerSparseUpdate", [t["table"], t["ids"].reshape(-1), t["grads"], t["veloc"]],
                                     scalars=[_c(HYPER["lr"]), _c(MOMENTUM), __import__("ctypes").c_bool(False)], stream=s),
                      {"table": t["table"], "veloc": t["veloc"]})[1],
    _momentum_model(lambda a: a["grads"], False), f32only=True, big=True, atol=OPT_ATOL, symbol="MomentumOptimizerSparseUpdate")


def _uids_adagrad(a, v):
    p, acc = a["table"].copy(), a["state1"].copy()
    cpu.adagrad_sparse(p, acc, a["uids"], a["grads"], HYPER["lr"], HYPER["eps"])
    return {"table": p, "state1": acc}


row("dl_call[AdaGradOptimizerSparseUpdate]", "ops.dl_call", ("table", "uids", "grads", "state1"),
    lambda t, s, st: (_ops().dl_call("AdaGradOptimizerSparseUpdate", [t["table"], t["uids"], t["grads"], t["state1"]],
                                     scalars=[_c(HYPER["lr"]), _c(HYPER["eps"])], stream=s),
                      {"table": t["table"], "state1": t["state1"]})[1],
    _uids_adagrad, f32only=True, big=True, atol=OPT_ATOL, symbol="AdaGradOptimizerSparseUpdate")
row("dl_call[AddL2RegularizationSparse]", "ops.dl_call", ("table", "uids", "grads"),
    lambda t, s, st: (_ops().dl_call("AddL2RegularizationSparse", [t["table"], t["uids"], t["grads"]], scalars=[_c(0.3)], stream=s),
                      {"grads": t["grads"]})[1],
    lambda a, v: {"grads": cpu.l2_sparse(a["table"], a["uids"], a["grads"], 0.3)}, f32only=True, atol=1e-6,
    symbol="AddL2RegularizationSparse")


def _uids_moments(which):
    """Adam / AdamW / Lamb symbols on distinct ids: the numpy oracle of tests/test_gpu_optim.py."""
    def model(a, v):
        p, m, vv = a["table"].copy(), a["state1"].copy(), a["state2"].copy()
        h = HYPER
        args = (p, m, vv, a["uids"], a["grads"], h["lr"], h["beta1"], h["beta2"], F32(h["beta1t"]), F32(h["beta2t"]), h["eps"])
        if which == "lamb":
            cpu.lamb_sparse(*args, h["weight_decay"])
        else:
            cpu.adam_sparse(*args, h["weight_decay"] if which == "adamw" else None)
        return {"table": p, "state1": m, "state2": vv}
    return model


def _moment_scalars(which):
    h = HYPER
    sc = [h["lr"], h["beta1"], h["beta2"], h["beta1t"], h["beta2t"], h["eps"]] + ([] if which == "adam" else [h["weight_decay"]])
    return [_c(x) for x in sc]


for _which_opt, _sym in (("adam", "AdamOptimizerSparseUpdate"), ("adamw", "AdamWOptimizerSparseUpdate"),
                         ("lamb", "LambOptimizerSparseUpdate")):
    row("dl_call[%s]" % _sym, "ops.dl_call", ("table", "uids", "grads", "state1", "state2"),
        lambda t, s, st, w=_which_opt, y=_sym: (_ops().dl_call(y, [t["table"], t["uids"], t["grads"], t["state1"], t["state2"]],
                                                               scalars=_moment_scalars(w), stream=s), _opt_out(t, "adam"))[1],
        _uids_moments(_which_opt), f32only=True, big=True, atol=OPT_ATOL, symbol=_sym)

# the scatter symbols: occurrence-order sums per key, as tests/test_gpu_parity.py compares them (the oracle's serial push)
row("dl_call[IndexedSlicesOneSideAdd]", "ops.dl_call", ("ids", "grads", "table"),
    lambda t, s, st: (_ops().dl_call("IndexedSlicesOneSideAdd", [t["ids"], t["grads"], t["table"]], stream=s), {"table": t["table"]})[1],
    lambda a, v: _ps_push(a, a["grads"], -1.0), f32only=True, big=True, symbol="IndexedSlicesOneSideAdd")


def _dense_out(t, s, st):
    """A dense [rows, width] output of the caller's, allocated before anything is late (7.0 everywhere: the symbol zeroes it)."""
    if "dense" not in st:
        st["dense"] = t["table"].new_full(tuple(t["table"].shape), 7.0)


row("dl_call[DLGpuEmbeddingLookUp_Gradient]", "ops.dl_call", ("grads", "ids", "table"),      # (the table: the shape of the output)
    lambda t, s, st: (_ops().dl_call("DLGpuEmbeddingLookUp_Gradient", [t["grads"], t["ids"], st["dense"]], stream=s),
                      {"dense": st["dense"]})[1],
    lambda a, v: {"dense": fm_model.ps_push(np.zeros_like(a["table"]), _flat_ids(a), a["grads"], -1.0)}, prep=_dense_out,
    f32only=True, big=True, symbol="DLGpuEmbeddingLookUp_Gradient")
row("dl_call[DeduplicateIndexedSlices]", "ops.dl_call", ("grads", "invf", "zeros"),
    lambda t, s, st: (_ops().dl_call("DeduplicateIndexedSlices", [t["grads"], t["invf"], t["zeros"]], stream=s),
                      {"zeros": t["zeros"]})[1],
    lambda a, v: {"zeros": fm_model.ps_push(a["zeros"], a["invf"], a["grads"], -1.0)}, f32only=True, big=True,
    symbol="DeduplicateIndexedSlices")


def _zero_dense(t, s, st):
    """IndexedSlices2Dense's output is pre-zeroed by the caller: on the stream, behind the late writes."""
    if "dense" not in st:
        st["dense"] = t["grads"].new_empty((2000, t["grads"].shape[1]))
    st["dense"].zero_()


row("dl_call[IndexedSlices2Dense]", "ops.dl_call", ("grads", "uids"),
    lambda t, s, st: (_ops().dl_call("IndexedSlices2Dense", [t["grads"], t["uids"], st["dense"]], stream=s), {"out": st["dense"]})[1],
    lambda a, v: _dense_model(a, v), prep=_zero_dense, f32only=True, symbol="IndexedSlices2Dense")


# -- IndexedSlices ---------------------------------------------------------------------------------------------------------------
def _shape(t):
    return tuple(t["table"].shape) if "table" in t else None


def _slices(t, kind, values="bg", with_offsets=True):
    """IndexedSlices of the device tensors t: kind 'flat' (unpooled), 'pooled', 'weighted', 'fm', 'fm0' (no g_sum), 'wfm'."""
    ops = _ops()
    kw = {}
    if kind != "flat":
        if "offsets" in t:
            kw.update(bag_of=t["bag_of"], offsets=t["offsets"] if with_offsets else None)
        else:
            kw.update(bag=F)
    if kind in ("weighted", "wfm"):
        kw["weights"] = t["weights"]
    if kind == "wfm":
        kw["sq_grad"] = t["bg2"]
    if kind in ("fm", "fm0"):
        kw.update(fm_grad=t["bg2"], fm_sum=t["S"])
    vals = None if kind == "fm0" else t["grads" if kind == "flat" else values]
    return ops.IndexedSlices(indices=t["ids"], values=vals, dense_shape=_shape(t), **kw)


row("IndexedSlices.expanded_values[pooled]", "ops.IndexedSlices.expanded_values", ("ids", "bg", "bag_of", "offsets"),
    lambda t, s, st: {"out": _slices(t, "pooled").expanded_values(stream=s)}, lambda a, v: {"out": _expanded(a)})
row("IndexedSlices.expanded_values[weighted]", "ops.IndexedSlices.expanded_values", ("ids", "bg", "weights", "bag_of", "offsets"),
    lambda t, s, st: {"out": _slices(t, "weighted").expanded_values(stream=s)},
    lambda a, v: {"out": wbag_model.wbag_grad_rows(a["bg"], a["weights"], _which(a))})


def _dedup_call(t, s, st):
    sl = _ops().IndexedSlices(indices=t["ids"], values=t["grads"], push_indices=t["pids"])
    sl.deduplicate(stream=s)
    return {"indices": sl.indices, "values": sl.values, "push_indices": sl.push_indices}


def _dedup_model(a, v):
    uniq, _, red = cpu.dedup_reduce(_flat_ids(a), a["grads"])
    return {"indices": uniq.astype(F32), "values": red, "push_indices": np.unique(a["pids"]).astype(F32)}


row("IndexedSlices.deduplicate", "ops.IndexedSlices.deduplicate", ("ids", "grads", "pids"), _dedup_call, _dedup_model, f32only=True,
    big=True, synchronous=True,
    why="the number of unique indices shapes the returned slices: IndexPlan.export_f32 reads n_unique back (ndarray.py:534-545 "
        "does the same with np.unique on the host)")


row("IndexPlan.export_f32", "ops.IndexPlan.export_f32", ("ids",),
    lambda t, s, st: dict(zip(("uniq", "inverse"), st["plan"].export_f32(stream=s))),
    lambda a, v: {"uniq": _uniq(a)[0].astype(F32), "inverse": _uniq(a)[1].astype(F32)}, prep=_plan("build"), synchronous=True,
    why="it returns uniq[:n_unique]: the count is read back from the plan (IndexPlan.n_unique waits for the plan's producer)")


def _dense_model(a, v):
    dense = np.zeros((v.rows, v.width), dtype=F32)
    dense[a["uids"].astype(np.int64)] = a["grads"]
    return {"out": dense}


row("IndexedSlices.to_dense", "ops.IndexedSlices.to_dense", ("uids", "grads"),
    lambda t, s, st: {"out": _ops().IndexedSlices(indices=t["uids"], values=t["grads"],
                                                  dense_shape=st["shape"]).to_dense(stream=s)},
    _dense_model, f32only=True, prep=lambda t, s, st: st.__setitem__("shape", (2000, t["grads"].shape[1])))

# -- herald_amd/hetu_ops.py ------------------------------------------------------------------------------------------------------
row("hetu.scale_", "hetu_ops.scale_", ("grads",),
    lambda t, s, st: {"grads": _hetu().scale_(t["grads"], SCALE, stream=s)},
    lambda a, v: {"grads": (a["grads"] * F32(SCALE)).astype(F32)})
row("hetu.unweighted_slices", "hetu_ops.unweighted_slices", ("ids", "bg", "weights", "bag_of", "offsets"),
    lambda t, s, st: {"values": _hetu().unweighted_slices(_slices(t, "weighted"), stream=s).values},
    lambda a, v: {"values": wbag_model.wbag_grad_rows(a["bg"], a["weights"], _which(a))})


def _param(t):
    return _hetu().EmbeddingParameter(table=t["table"])


def _sgd_row(name, kind, layouts, uses, model, big=False):
    row("hetu.sgd_update_sparse[%s]" % name, "hetu_ops.sgd_update_sparse", ("table", "ids") + uses,
        lambda t, s, st: (_hetu().sgd_update_sparse(_param(t), _slices(t, kind), LR, stream=s), {"table": t["table"]})[1],
        model, layouts=layouts, f32only=True, big=big)


_POOLED = ("bg", "bag_of", "offsets")
_sgd_row("fm-fixed", "fm", "fixed", _POOLED + ("bg2", "S"), _fm_sgd)
_sgd_row("fm-ragged", "fm", "ragged", _POOLED + ("bg2", "S"), _fm_sgd, big=True)
_sgd_row("fm-no-g_sum", "fm0", "ragged", ("bag_of", "offsets", "bg2", "S"), lambda a, v: _fm_sgd(a, v, None), big=True)
_sgd_row("wfm-fixed", "wfm", "fixed", _POOLED + ("bg2", "weights"), _wfm_sgd)
_sgd_row("wfm-ragged", "wfm", "ragged", _POOLED + ("bg2", "weights"), _wfm_sgd, big=True)
_sgd_row("weighted-fixed", "weighted", "fixed", _POOLED + ("weights",),
         lambda a, v: {"table": wbag_model.wbag_sgd(a["table"], a["ids"], a["weights"], a["bg"], LR, _off(a))})
_sgd_row("weighted-ragged", "weighted", "ragged", _POOLED + ("weights",),
         lambda a, v: {"table": wbag_model.wbag_sgd(a["table"], a["ids"], a["weights"], a["bg"], LR, _off(a))}, big=True)
_sgd_row("pooled-fixed", "pooled", "fixed", _POOLED, lambda a, v: {"table": bag_model.sgd_bags(a["table"], a["ids"], a["bg"], LR, _off(a))})
_sgd_row("pooled-ragged", "pooled", "ragged", _POOLED,
         lambda a, v: {"table": bag_model.sgd_bags(a["table"], a["ids"], a["bg"], LR, _off(a))}, big=True)
row("hetu.sgd_update_sparse(strided values)[pooled-fixed]", "hetu_ops.sgd_update_sparse", ("table", "ids", "bg_wide"),
    # values is a strided view of a late buffer: the .contiguous() inside the call makes a real copy
    lambda t, s, st: (_hetu().sgd_update_sparse(_param(t), _ops().IndexedSlices(indices=t["ids"], values=t["bg_wide"][:, ::2],
                                                                               dense_shape=_shape(t), bag=F), LR, stream=s),
                      {"table": t["table"]})[1],
    lambda a, v: {"table": bag_model.sgd_bags(a["table"], a["ids"], np.ascontiguousarray(a["bg_wide"][:, ::2]), LR)},
    layouts="fixed", f32only=True)
_sgd_row("unpooled", "flat", "both", ("grads",), lambda a, v: {"table": fm_model.sgd_serial(a["table"], _flat_ids(a), a["grads"], LR)},
         big=True)

# fuse_bags=False is the reference's own sequence: expanded_values, IndexedSlices.deduplicate, the symbol -- synchronous as
# deduplicate is (the momentum update does not deduplicate)
_REFERENCE_SEQUENCE = {True: {}, False: dict(synchronous=True, why="fuse_bags=False runs IndexedSlices.deduplicate, which reads the "
                                                                    "number of unique indices back (the fused forms do not)")}
for _fuse in (True, False):
    row("hetu.momentum_update_sparse[fuse_bags=%s]" % _fuse, "hetu_ops.momentum_update_sparse", ("table", "ids", "veloc") + _POOLED,
        lambda t, s, st, fb=_fuse: (_hetu().momentum_update_sparse(_param(t), _slices(t, "pooled"), t["veloc"], HYPER["lr"], MOMENTUM,
                                                                   False, stream=s, fuse_bags=fb),
                                    {"table": t["table"], "veloc": t["veloc"]})[1],
        _momentum_model(_expanded, False), f32only=True, big=True, atol=OPT_ATOL)
    row("hetu.adagrad_update_sparse[fuse_bags=%s]" % _fuse, "hetu_ops.adagrad_update_sparse", ("table", "ids", "state1", "state2") + _POOLED,
        lambda t, s, st, fb=_fuse: (_hetu().adagrad_update_sparse(_param(t), _slices(t, "pooled"), t["state1"], HYPER["lr"], HYPER["eps"],
                                                                  stream=s, fuse_bags=fb), _opt_out(t, "adagrad"))[1],
        _opt_model("adagrad", _expanded), f32only=True, big=True, atol=OPT_ATOL, **_REFERENCE_SEQUENCE[_fuse])
    row("hetu.adam_update_sparse[fuse_bags=%s]" % _fuse, "hetu_ops.adam_update_sparse", ("table", "ids", "state1", "state2") + _POOLED,
        lambda t, s, st, fb=_fuse: (_hetu().adam_update_sparse(_param(t), _slices(t, "pooled"), t["state1"], t["state2"], HYPER["lr"], HYPER["beta1"],
                                                               HYPER["beta2"], HYPER["beta1t"], HYPER["beta2t"], HYPER["eps"], stream=s, fuse_bags=fb),
                                    _opt_out(t, "adam"))[1],
        _opt_model("adam", _expanded), f32only=True, big=True, atol=OPT_ATOL, **_REFERENCE_SEQUENCE[_fuse])
    row("hetu.adamw_update_sparse[fuse_bags=%s]" % _fuse, "hetu_ops.adamw_update_sparse", ("table", "ids", "state1", "state2") + _POOLED,
        lambda t, s, st, fb=_fuse: (_hetu().adamw_update_sparse(_param(t), _slices(t, "pooled"), t["state1"], t["state2"], HYPER["lr"],
                                                                HYPER["beta1"], HYPER["beta2"], HYPER["beta1t"], HYPER["beta2t"], HYPER["eps"],
                                                                HYPER["weight_decay"], stream=s, fuse_bags=fb), _opt_out(t, "adamw"))[1],
        _opt_model("adamw", _expanded), f32only=True, big=True, atol=OPT_ATOL, **_REFERENCE_SEQUENCE[_fuse])
row("hetu.adam_update_sparse[unpooled]", "hetu_ops.adam_update_sparse", ("table", "ids", "grads", "state1", "state2"),
    lambda t, s, st: (_hetu().adam_update_sparse(_param(t), _slices(t, "flat"), t["state1"], t["state2"], HYPER["lr"], HYPER["beta1"], HYPER["beta2"],
                                                 HYPER["beta1t"], HYPER["beta2t"], HYPER["eps"], stream=s), _opt_out(t, "adam"))[1],
    _opt_model("adam", lambda a: a["grads"]), f32only=True, big=True, atol=OPT_ATOL)
row("hetu.adagrad_update_sparse[weighted]", "hetu_ops.adagrad_update_sparse", ("table", "ids", "state1", "state2", "weights") + _POOLED,
    lambda t, s, st: (_hetu().adagrad_update_sparse(_param(t), _slices(t, "weighted"), t["state1"], HYPER["lr"], HYPER["eps"], stream=s),
                      _opt_out(t, "adagrad"))[1],
    _opt_model("adagrad", lambda a: wbag_model.wbag_grad_rows(a["bg"], a["weights"], _which(a))), f32only=True, big=True,
    atol=OPT_ATOL)

BY_NAME = {e.name: e for e in REGISTRY}
assert len(BY_NAME) == len(REGISTRY), "registry names are unique"

# Every public callable of ops.py / hetu_ops.py with a `stream` parameter that is NOT in the registry, and why.
EXCLUDED = {
    "ops.IndexPlan.sort": "planner: ordering pinned by test_gpu_late_ids; every registry row with a plan runs it on the late ids",
    "ops.IndexPlan.finish": "planner: ordering pinned by test_gpu_late_ids; run by the rows that take a finished plan",
    "ops.IndexPlan.build": "planner: ordering pinned by test_gpu_late_ids; run by the rows that take a finished plan",
    "ops.IndexPlan.produced_on": "host bookkeeping: records a stream, enqueues nothing",
    "ops.on_stream": "the context the fixes are built on, not an op",
    "ops.DLStreamHolder.__init__": "plumbing of dl_call (covered by the dl_call rows)",
    "ops.PendingTable.reset": "pipeline: ordering pinned by test_gpu_late_ids",
    "ops.StepPipeline": "pipeline: ordering pinned by test_gpu_late_ids",
    "ops.SortAheadPipeline": "planner: ordering pinned by test_gpu_late_ids",
    "ops.QueueStepPipeline": "pipeline (work-queue engine): out of scope, ordering pinned by test_gpu_late_ids",
    "hetu_ops.EmbeddingLookUpFM_Gradient": "builds slices; its launches are ops.bag_of and ops.fm_grad_rows, both registry rows",
    "hetu_ops.EmbeddingLookUpFMSum_Gradient": "builds slices; its one launch is ops.bag_of (a registry row)",
    "hetu_ops.EmbeddingLookUpWeightedFMSum_Gradient": "builds slices; its one launch is ops.bag_of (a registry row)",
}


@functools.lru_cache(maxsize=None)
def _expected(name, vid, decoy):
    e = BY_NAME[name]
    v = [x for x in e.variants() if x.id == vid][0]
    return e.model(e.inputs(v, decoy), v)


def expected(entry, v, decoy=False):
    """The model's result on the real (or the decoy) inputs: computed once, shared, never written to."""
    return _expected(entry.name, v.id, decoy)


def cases():
    return [(e, v) for e in REGISTRY for v in e.variants()]

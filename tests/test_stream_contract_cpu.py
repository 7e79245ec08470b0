"""The registry of tests/stream_contract.py, checked without a GPU: it names every public callable of ops.py and hetu_ops.py that
takes `stream=` (or an exclusion says why not), and every row's decoy is valid and visible: the model applied to the decoy
inputs differs from the model applied to the real ones, so a stale read cannot pass tests/test_gpu_stream_contract.py."""
import inspect

import numpy as np
import pytest

import stream_contract as sc
from herald_amd import hetu_ops, ops


def _takes_stream(fn):
    try:
        return "stream" in inspect.signature(fn).parameters
    except (TypeError, ValueError):
        return False


def _stream_callables(registry=None, excluded=None):
    """(every 'module.name' / 'module.Class.method' with a stream parameter, those of them neither registered nor excluded)."""
    registry = sc.REGISTRY if registry is None else registry
    excluded = sc.EXCLUDED if excluded is None else excluded
    found = []
    for modname, mod in (("ops", ops), ("hetu_ops", hetu_ops)):
        for name, obj in vars(mod).items():
            if name.startswith("_") or getattr(obj, "__module__", None) != mod.__name__:
                continue
            if inspect.isfunction(obj):
                if _takes_stream(obj):
                    found.append("%s.%s" % (modname, name))
            elif inspect.isclass(obj):
                for mname, m in vars(obj).items():
                    if (mname == "__init__" or not mname.startswith("_")) and inspect.isfunction(m) and _takes_stream(m):
                        found.append("%s.%s.%s" % (modname, name, mname))
    targets = {e.target for e in registry}
    undecided = [k for k in found if k not in targets and k not in excluded and k.rsplit(".", 1)[0] not in excluded]
    return found, undecided


def test_every_callable_with_a_stream_parameter_has_a_row_or_a_reason():
    found, undecided = _stream_callables()
    assert len(found) > 60
    assert not undecided, "ops with a stream= parameter and no row in tests/stream_contract.py (REGISTRY or EXCLUDED): %s" % undecided
    known = set(found) | {k.rsplit(".", 1)[0] for k in found}
    assert not [k for k in sc.EXCLUDED if k not in known], "stale exclusions"
    assert not [e.target for e in sc.REGISTRY if e.target not in found], "rows for callables that are not there"
    assert all(reason.strip() for reason in sc.EXCLUDED.values())


@pytest.mark.parametrize("target", ["ops.sgd_sparse_update_wfm_bags", "hetu_ops.adamw_update_sparse", "ops.IndexedSlices.to_dense"])
def test_the_completeness_check_fails_when_a_row_is_removed(target):
    fewer = [e for e in sc.REGISTRY if e.target != target]
    assert len(fewer) < len(sc.REGISTRY)
    assert _stream_callables(registry=fewer)[1] == [target]


def test_every_reference_named_symbol_with_a_stream_has_a_dl_call_row():
    """The symbol table of herald_amd/_lib.py (the DLArray ABI: the entries whose last argument is a DLStream) against the
    dl_call rows: a new symbol needs a row of its own, one that calls it directly."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(ops.__file__), "_lib.py")).read()
    table = src[src.index("    dl = {"):src.index("for name, args in dl.items()")]
    bound = dict(re.findall(r'"(\w+)": \[([^\]]*)\]', table))
    assert len(bound) >= 14
    with_stream = sorted(n for n, args in bound.items() if args.split(",")[-1].strip() == "S")
    assert len(with_stream) == 12 and "LambOptimizerSparseUpdate" in with_stream and "cpu_EmbeddingLookup" not in with_stream
    rows = sorted(e.symbol for e in sc.REGISTRY if e.target == "ops.dl_call")
    assert rows == with_stream, "dl_call rows %s, symbols bound with a DLStream %s" % (rows, with_stream)
    assert all(e.symbol in e.name for e in sc.REGISTRY if e.symbol) and not [e for e in sc.REGISTRY if e.symbol and e.target != "ops.dl_call"]


def test_the_rows_the_issue_counts():
    names = [e.name for e in sc.REGISTRY]
    assert len([n for n in names if n.startswith("hetu.sgd_update_sparse[")]) == 10
    for opt in ("momentum", "adagrad", "adam", "adamw"):
        for fuse in (True, False):
            assert "hetu.%s_update_sparse[fuse_bags=%s]" % (opt, fuse) in names
    sync = sorted(e.name for e in sc.REGISTRY if e.synchronous)
    assert sync == sorted(["IndexPlan.export_f32", "IndexedSlices.deduplicate"] +        # ... and the forms that run deduplicate
                          ["hetu.%s_update_sparse[fuse_bags=False]" % o for o in ("adagrad", "adam", "adamw")])
    assert all(sc.BY_NAME[n].why for n in sync)
    shapes = {v.id for e, v in sc.cases()}
    assert {"small-d64-f32-fixed", "small-d5-i64-ragged", "big-d16-f32-fixed", "big-d16-f32-ragged"} <= shapes
    assert sc.BIG_B * sc.F == 39000


def _check_decoy(name, real, decoy, v):
    assert decoy.shape == real.shape and decoy.dtype == real.dtype, name
    assert not np.array_equal(decoy, real), "%s: the decoy is the real input" % name
    n, limit = v.n, {"ids": v.rows, "uids": v.rows, "pids": v.rows, "keys": v.n, "invf": v.n, "rowmap": v.n, "bag_of": v.nbags}
    if name in limit:
        ints = decoy.astype(np.int64)
        assert np.array_equal(ints.astype(decoy.dtype), decoy) and ints.min() >= 0 and ints.max() < limit[name], name
        if name == "uids":
            assert np.unique(ints).size == ints.size
        if name == "bag_of":
            assert (np.diff(ints) >= 0).all()
    elif name == "offsets":
        assert decoy[0] == 0 and decoy[-1] == n and (np.diff(decoy) >= 0).all() and decoy.size == v.nbags + 1
    elif name == "posmap":
        m = decoy.view(np.uint32)
        idx = (m & np.uint32(0x7FFFFFFF)).astype(np.int64)
        assert (idx[(m >> 31) != 0] < v.rows).all() and (idx[(m >> 31) == 0] < v.n).all()
    elif name == "dst_init":
        assert set(np.unique(decoy)) <= {0, 1}
    else:
        assert decoy.dtype == np.float32 and np.isfinite(decoy).all(), name
        if name == "weights":
            assert not np.array_equal(decoy == 0, real == 0), "weights: the same live/dead pattern"
            assert (decoy == 0).any() and (decoy != 0).any()


@pytest.mark.parametrize("entry,v", sc.cases(), ids=["%s-%s" % (e.name, v.id) for e, v in sc.cases()])
def test_decoys_are_valid_and_the_model_sees_them(entry, v):
    real, decoy = entry.inputs(v), entry.inputs(v, decoy=True)
    assert set(real) == set(decoy) and real
    for name in real:
        _check_decoy(name, real[name], decoy[name], v)
    if "ids" in real:
        ids = real["ids"].astype(np.int64)
        assert ids.min() >= 0 and ids.max() < v.rows and np.unique(ids).size < ids.size, "real ids: in range, with duplicates"
    want, stale = sc.expected(entry, v), sc.expected(entry, v, decoy=True)
    assert set(want) == set(stale) and want
    for k in want:
        assert want[k].shape != stale[k].shape or not np.array_equal(want[k], stale[k]), \
            "%s: the model gives the same %s for the decoy inputs: a stale read would pass" % (entry.name, k)
        if entry.atol is not None and want[k].shape == stale[k].shape:       # ... and not within the row's tolerance either
            assert np.abs(want[k].astype(np.float64) - stale[k]).max() > 100 * entry.atol

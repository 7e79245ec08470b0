"""CPU-side checks of the optimizers on pooled gradients: the new entry points are declared in include/herald_amd.h with the
argument lists herald_amd/_lib.py binds and the library exports them; every refusal comes before any device access and names
the function; the Python wrappers and the four hetu_ops functions reject bad shapes without a native call."""
import ctypes
import re

import pytest
import torch

from herald_amd import _lib, hetu_ops, ops

_FUSED = ["int", "float *", "int64_t", "int64_t", None, "int64_t", "const float *", "float *", "float *", "const float *",
          "void *", "ha_stream_t"]
_FUSED_BAGS = ["int", "float *", "int64_t", "int64_t", None, "int64_t", "const float *", "int64_t", "const int64_t *",
               "int64_t", "float *", "float *", "const float *", "void *", "ha_stream_t"]
_MOMENTUM_BAGS = ["float *", "int64_t", "int64_t", None, "int64_t", "const float *", "int64_t", "const int64_t *", "int64_t",
                  "float *", "float", "float", "int", "ha_stream_t"]


def _with_ids(args, ids):
    return [ids if a is None else a for a in args]


NEW = {
    "ha_sparse_opt_fused_u64ids": _with_ids(_FUSED, "const uint64_t *"),
    "ha_sparse_opt_fused_bags_f32ids": _with_ids(_FUSED_BAGS, "const float *"),
    "ha_sparse_opt_fused_bags_u64ids": _with_ids(_FUSED_BAGS, "const uint64_t *"),
    "ha_momentum_sparse_update_bags_f32ids": _with_ids(_MOMENTUM_BAGS, "const float *"),
    "ha_momentum_sparse_update_bags_u64ids": _with_ids(_MOMENTUM_BAGS, "const uint64_t *"),
}


def _header_args(name):
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;{}]*)\)\s*;" % name, text)
    assert m, "%s is not declared in the header" % name
    out = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        out.append(re.sub(r"\s*\b\w+$", "", a).strip())       # drop the parameter's name
    return out


def test_header_declares_the_new_entry_points():
    declared = _lib.declared_symbols()
    for name, want in NEW.items():
        assert _header_args(name) == want, name
        assert name in declared
    # the unpooled int64 call takes what the float32 one takes, but for the ids
    f32 = _header_args("ha_sparse_opt_fused_f32ids")
    assert [a.replace("const float *", "X") if i == 4 else a for i, a in enumerate(f32)] == \
           [a.replace("const uint64_t *", "X") if i == 4 else a for i, a in enumerate(NEW["ha_sparse_opt_fused_u64ids"])]


def test_library_exports_and_binds_the_new_entry_points(lib):
    ctype_of = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
    for name, want in NEW.items():
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int
        assert len(fn.argtypes) == len(want), name
        for got, decl in zip(fn.argtypes, want):
            assert got is ctype_of.get(decl, ctypes.c_void_p), (name, decl, got)


# a non-null address that is never dereferenced: validation comes before any device access (there is no GPU here)
P = ctypes.c_void_p(0x1000)

_FUSED_REFUSALS = [
    ("kind -1", dict(kind=-1)),
    ("kind 3", dict(kind=3)),
    ("null param", dict(param=None)),
    ("null ids", dict(ids=None)),
    ("null gradient", dict(grads=None)),
    ("null state1", dict(state1=None)),
    ("null hyper-parameters", dict(hyper=None)),
    ("null plan workspace", dict(plan=None)),
    ("Adam without state2", dict(kind=1, state2=None)),
    ("AdamW without state2", dict(kind=2, state2=None)),
    ("width 0", dict(width=0)),
    ("negative width", dict(width=-4)),
    ("negative n", dict(n=-1)),
    ("negative rows", dict(rows=-1)),
    ("n = 2^31", dict(n=1 << 31, nbags=1 << 30)),
]
_BAG_REFUSALS = [
    ("negative nbags", dict(nbags=-1)),
    ("negative bag", dict(bag=-2)),
    ("neither bag nor offsets", dict(bag=0, offsets=None)),
    ("both bag and offsets", dict(bag=2, offsets=P)),
    ("n not a multiple of bag", dict(n=7, bag=2, nbags=3)),
    ("n is not nbags * bag", dict(n=8, bag=2, nbags=3)),
]


@pytest.mark.parametrize("fn", ["ha_sparse_opt_fused_bags_f32ids", "ha_sparse_opt_fused_bags_u64ids"])
@pytest.mark.parametrize("case,args", _FUSED_REFUSALS + _BAG_REFUSALS)
def test_fused_bag_calls_refuse_before_any_device_access(lib, fn, case, args):
    a = dict(kind=1, param=P, rows=10, width=4, ids=P, n=8, grads=P, bag=2, offsets=None, nbags=4, state1=P, state2=P, hyper=P,
             plan=P)
    a.update(args)
    rc = getattr(lib, fn)(a["kind"], a["param"], a["rows"], a["width"], a["ids"], a["n"], a["grads"], a["bag"], a["offsets"],
                          a["nbags"], a["state1"], a["state2"], a["hyper"], a["plan"], None)
    assert rc == -1, case
    assert fn.encode() in lib.ha_last_error(), (case, lib.ha_last_error())


@pytest.mark.parametrize("case,args", _FUSED_REFUSALS)
def test_unpooled_int64_call_refuses_before_any_device_access(lib, case, args):
    a = dict(kind=1, param=P, rows=10, width=4, ids=P, n=8, grads=P, state1=P, state2=P, hyper=P, plan=P)
    a.update({k: v for k, v in args.items() if k != "nbags"})
    rc = lib.ha_sparse_opt_fused_u64ids(a["kind"], a["param"], a["rows"], a["width"], a["ids"], a["n"], a["grads"], a["state1"],
                                        a["state2"], a["hyper"], a["plan"], None)
    assert rc == -1, case
    assert b"ha_sparse_opt_fused_u64ids" in lib.ha_last_error(), (case, lib.ha_last_error())


def test_nothing_to_do_returns_0(lib):
    for fn in ("ha_sparse_opt_fused_bags_f32ids", "ha_sparse_opt_fused_bags_u64ids"):
        assert getattr(lib, fn)(0, None, 10, 4, None, 0, None, 2, None, 0, None, None, None, None, None) == 0
        assert getattr(lib, fn)(1, None, 10, 4, None, 0, None, 0, P, 3, None, None, None, None, None) == 0     # ragged, all empty
    assert lib.ha_sparse_opt_fused_u64ids(2, None, 10, 4, None, 0, None, None, None, None, None, None) == 0
    assert lib.ha_sparse_opt_fused_f32ids(2, None, 10, 4, None, 0, None, None, None, None, None, None) == 0


@pytest.mark.parametrize("fn", ["ha_momentum_sparse_update_bags_f32ids", "ha_momentum_sparse_update_bags_u64ids"])
@pytest.mark.parametrize("case,args", _BAG_REFUSALS + [
    ("null param", dict(param=None)),
    ("null ids", dict(ids=None)),
    ("null gradient", dict(grads=None)),
    ("null velocity", dict(velocity=None)),
    ("null param, nothing to apply", dict(param=None, n=0, nbags=0)),
    ("width 0", dict(width=0)),
    ("negative n", dict(n=-1)),
    ("negative rows", dict(rows=-1)),
    ("n = 2^31", dict(n=1 << 31, nbags=1 << 30)),
])
def test_momentum_bag_calls_refuse_before_any_device_access(lib, fn, case, args):
    a = dict(param=P, rows=10, width=4, ids=P, n=8, grads=P, bag=2, offsets=None, nbags=4, velocity=P)
    a.update(args)
    rc = getattr(lib, fn)(a["param"], a["rows"], a["width"], a["ids"], a["n"], a["grads"], a["bag"], a["offsets"], a["nbags"],
                          a["velocity"], ctypes.c_float(0.1), ctypes.c_float(0.9), 1, None)
    assert rc == -1, case
    assert fn.encode() in lib.ha_last_error(), (case, lib.ha_last_error())


# ---- Python wrappers: shape checks without a native call --------------------------------------------------------------
class _OnDevice(torch.Tensor):
    """A host tensor that claims to live on a device: reaches the wrappers' shape checks.  Nothing may dereference it."""
    is_cuda = property(lambda self: True)


def _t(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype).as_subclass(_OnDevice)


class _NoNativeCall:
    """Stands where the library would be: any use is a failure of the test."""

    def load(self, *a, **kw):
        return self

    def __getattr__(self, name):
        raise AssertionError("the argument checks reached for %s" % name)


@pytest.fixture
def no_native(monkeypatch):
    monkeypatch.setattr(ops, "_lib", _NoNativeCall())
    monkeypatch.setattr(hetu_ops, "_lib", _NoNativeCall())


ROWS, WIDTH, B, F = 10, 4, 3, 2


def test_sparse_opt_fused_bags_checks_its_arguments(no_native):
    param, s1, s2 = _t(ROWS, WIDTH), _t(ROWS, WIDTH), _t(ROWS, WIDTH)
    ids, g = _t(B, F), _t(B, WIDTH)
    off = _t(B + 1, dtype=torch.int64)
    for kw, exc, msg in [
        (dict(kind="sgd"), ValueError, "kind must be"),
        (dict(param=_t(ROWS * WIDTH)), ValueError, "param must be 2-D"),
        (dict(param=torch.zeros(ROWS, WIDTH)), TypeError, "param must be a CUDA/HIP"),
        (dict(state1=_t(ROWS - 1, WIDTH)), ValueError, "state1 must have the size"),
        (dict(state2=None), ValueError, "needs state2"),
        (dict(state2=_t(ROWS, WIDTH + 1)), ValueError, "state2 must have the size"),
        (dict(state1=_t(ROWS, WIDTH, dtype=torch.float64)), TypeError, "state1 must be"),
        (dict(bag_grads=_t(B + 1, WIDTH)), ValueError, r"bag_grads must be \[B, width\]"),
        (dict(bag_grads=_t(B, WIDTH + 1)), ValueError, r"bag_grads must be \[B, width\]"),
        (dict(bag_grads=_t(WIDTH, B).t()), ValueError, "bag_grads must be contiguous"),
        (dict(ids=_t(B * F)), ValueError, "fixed bags need ids of shape"),
        (dict(ids=_t(B, F), offsets=off), ValueError, "ragged bags need ids of shape"),
        (dict(ids=_t(B * F), offsets=_t(B + 1, dtype=torch.int32)), TypeError, "offsets must be"),
        (dict(ids=_t(B * F), offsets=_t(B + 2, dtype=torch.int64)), ValueError, r"bag_grads must be \[B, width\]"),
        (dict(ids=_t(B, F, dtype=torch.int32)), TypeError, "ids must be float32 or"),
    ]:
        a = dict(kind="adam", param=param, ids=ids, bag_grads=g, state1=s1, state2=s2)
        a.update(kw)
        with pytest.raises(exc, match=msg):
            ops.sparse_opt_fused_bags(**a)
    with pytest.raises(ValueError, match="needs state2"):
        ops.sparse_opt_fused_bags("adamw", param, ids, g, s1)


def test_momentum_sparse_update_bags_checks_its_arguments(no_native):
    param, v = _t(ROWS, WIDTH), _t(ROWS, WIDTH)
    ids, g = _t(B, F), _t(B, WIDTH)
    for kw, exc, msg in [
        (dict(param=_t(ROWS * WIDTH)), ValueError, "param must be 2-D"),
        (dict(velocity=_t(ROWS + 1, WIDTH)), ValueError, "velocity must have the size"),
        (dict(velocity=torch.zeros(ROWS, WIDTH)), TypeError, "velocity must be a CUDA/HIP"),
        (dict(bag_grads=_t(B + 1, WIDTH)), ValueError, r"bag_grads must be \[B, width\]"),
        (dict(ids=_t(B * F)), ValueError, "fixed bags need ids of shape"),
        (dict(ids=_t(B * F), offsets=_t(B, dtype=torch.int64)), ValueError, r"bag_grads must be \[B, width\]"),
        (dict(ids=_t(B, F, dtype=torch.int32)), TypeError, "ids must be float32 or"),
    ]:
        a = dict(param=param, ids=ids, bag_grads=g, velocity=v, lr=0.1, momentum=0.9)
        a.update(kw)
        with pytest.raises(exc, match=msg):
            ops.momentum_sparse_update_bags(**a)


def _call(name, param, grad, s1, s2, **kw):
    if name == "momentum_update_sparse":
        return hetu_ops.momentum_update_sparse(param, grad, s1, 0.1, 0.9, False, **kw)
    if name == "adagrad_update_sparse":
        return hetu_ops.adagrad_update_sparse(param, grad, s1, 0.1, 1e-7, **kw)
    if name == "adam_update_sparse":
        return hetu_ops.adam_update_sparse(param, grad, s1, s2, 0.1, 0.9, 0.999, 0.9, 0.999, 1e-7, **kw)
    return hetu_ops.adamw_update_sparse(param, grad, s1, s2, 0.1, 0.9, 0.999, 0.9, 0.999, 1e-7, 0.01, **kw)


@pytest.mark.parametrize("fuse_bags", [True, False])
@pytest.mark.parametrize("name", ["momentum_update_sparse", "adagrad_update_sparse", "adam_update_sparse",
                                  "adamw_update_sparse"])
def test_hetu_ops_reject_bad_shapes_without_a_native_call(no_native, name, fuse_bags):
    param = hetu_ops.EmbeddingParameter(table=_t(ROWS, WIDTH))
    s1, s2 = _t(ROWS, WIDTH), _t(ROWS, WIDTH)
    shape = (ROWS, WIDTH)
    pooled = ops.IndexedSlices(_t(B, F), _t(B, WIDTH), shape, bag=F)
    two_states = name in ("adam_update_sparse", "adamw_update_sparse")
    cases = [
        (param, ops.IndexedSlices(_t(B, F), _t(B, WIDTH + 1), shape, bag=F), s1, s2, "gradient rows must be 4 wide"),
        (param, ops.IndexedSlices(_t(B, F), _t(B + 1, WIDTH), shape, bag=F), s1, s2, "indices are not"),
        (param, ops.IndexedSlices(_t(B, F), _t(B, WIDTH), shape, bag=F + 1), s1, s2, "indices are not"),
        (param, ops.IndexedSlices(_t(B * F), _t(B, WIDTH), shape), s1, s2, "gradient rows for"),
        (param, ops.IndexedSlices(_t(B * F), _t(B, WIDTH), shape, bag_of=_t(B * F + 1, dtype=torch.int32)), s1, s2,
         "bag_of must have one entry"),
        (param, ops.IndexedSlices(_t(B * F), _t(B, WIDTH), shape, bag_of=_t(B * F, dtype=torch.int32),
                                  offsets=_t(B, dtype=torch.int64)), s1, s2, "offsets must have"),
        (param, ops.IndexedSlices(None, None, shape), s1, s2, "no indices"),
        (param, pooled, _t(ROWS + 1, WIDTH), s2, "must be a float32 tensor of the table's shape"),
        (param, pooled, _t(ROWS, WIDTH, dtype=torch.float64), s2, "must be a float32 tensor of the table's shape"),
        (hetu_ops.EmbeddingParameter(table=_t(ROWS * WIDTH)), pooled, s1, s2, "2-D device table"),
    ]
    if two_states:
        cases.append((param, pooled, s1, _t(ROWS, WIDTH - 1), "the second state must be"))
        cases.append((param, pooled, s1, None, "the second state must be"))
    for p, grad, a, b, msg in cases:
        with pytest.raises(ValueError, match=msg):
            _call(name, p, grad, a, b, fuse_bags=fuse_bags)
    if fuse_bags:      # ragged slices made by hand, without the offsets the one-call form takes
        with pytest.raises(ValueError, match="need their offsets"):
            _call(name, param, ops.IndexedSlices(_t(B * F), _t(B, WIDTH), shape, bag_of=_t(B * F, dtype=torch.int32)), s1, s2)


def test_indexed_slices_offsets_come_with_bag_of():
    with pytest.raises(ValueError, match="offsets come with bag_of"):
        ops.IndexedSlices(_t(B, F), _t(B, WIDTH), (ROWS, WIDTH), bag=F, offsets=_t(B + 1, dtype=torch.int64))
    sl = ops.IndexedSlices(_t(B * F), _t(B, WIDTH), (ROWS, WIDTH), bag_of=_t(B * F, dtype=torch.int32),
                           offsets=_t(B + 1, dtype=torch.int64))
    assert sl.pooled and sl.offsets is not None
    assert ops.IndexedSlices(_t(B * F), _t(B * F, WIDTH), (ROWS, WIDTH)).offsets is None


def test_example_takes_an_optimizer():
    import importlib.util
    import inspect
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "ctr", "run_wdl.py")
    spec = importlib.util.spec_from_file_location("run_wdl_for_bag_optim", path)
    run_wdl = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(run_wdl)
    sig = inspect.signature(run_wdl.train).parameters
    assert sig["optimizer"].default == "sgd" and sig["opt_fuse_bags"].default is True
    assert run_wdl.OPTIMIZERS == ("sgd", "momentum", "nesterov", "adagrad", "adam", "adamw")
    for engine in ("step", "step3", "queue", "ps", "cache"):
        with pytest.raises(ValueError, match="--embedding hbm only"):
            run_wdl.train(embedding=engine, optimizer="adam", device="cpu")
    with pytest.raises(ValueError, match="optimizer must be one of"):
        run_wdl.train(optimizer="lamb", device="cpu")

"""CPU-side checks of the pooled planned flow's interface: the three entry points are declared in include/herald_amd.h with the
argument lists herald_amd/_lib.py binds, the library exports them, and the Python methods check their arguments before any
native call (no device is touched)."""
import ctypes
import re

import pytest
import torch

from herald_amd import _lib
from herald_amd import cache as hcache

NEW = {
    "ha_cache_lookup_sum_planned": ["ha_cache *", "int64_t", "int64_t", "int64_t", "const int64_t *", "float *", "ha_stream_t"],
    "ha_cache_update_planned_bags": ["ha_cache *", "int64_t", "const float *", "int64_t", "int64_t", "const int32_t *",
                                     "ha_stream_t"],
    "ha_cache_run_planned_pairs_bags": ["ha_cache *", "int", "int64_t", "int64_t", "int64_t", "float *const *",
                                        "const float *const *", "ha_stream_t"],
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


def test_header_declares_the_pooled_entry_points():
    for name, want in NEW.items():
        assert _header_args(name) == want, name
        assert name in _lib.declared_symbols()


def test_library_exports_and_binds_the_pooled_entry_points(lib):
    ctype_of = {"int": ctypes.c_int, "int64_t": ctypes.c_int64}
    for name, want in NEW.items():
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int
        assert len(fn.argtypes) == len(want), name
        for got, decl in zip(fn.argtypes, want):
            assert got is ctype_of.get(decl, ctypes.c_void_p), (name, decl, got)


def test_native_argument_checks_come_before_any_device_access(lib):
    assert lib.ha_cache_lookup_sum_planned(None, 8, 2, 4, None, None, None) == -1
    assert b"cache_lookup_sum_planned" in lib.ha_last_error()
    assert lib.ha_cache_update_planned_bags(None, 8, None, 2, 4, None, None) == -1
    assert b"cache_update_planned_bags" in lib.ha_last_error()
    assert lib.ha_cache_run_planned_pairs_bags(None, 1, 8, 2, 4, None, None, None) == -1
    assert b"cache_run_planned_pairs_bags" in lib.ha_last_error()


class _NoDevice:
    """Stands where the library and the stream would be: any use is a failure of the test."""

    def __getattr__(self, name):
        raise AssertionError("the argument checks reached for %s" % name)


def _cache_with_a_planned_batch(n, width, looked_up):
    c = hcache.LRUCache.__new__(hcache.LRUCache)
    c._h = None
    c._L = _NoDevice()
    c._stream = _NoDevice()
    c._width = width
    c._planned = [[torch.zeros(n, dtype=torch.float32), looked_up, None]]
    return c


def test_python_argument_checks_raise_without_touching_a_device():
    n, width, bag = 8, 4, 2
    good = torch.zeros((n // bag, width), dtype=torch.float32)          # right shape, but a CPU tensor
    c = _cache_with_a_planned_batch(n, width, looked_up=False)
    for bad in (good, good.numpy(), None):
        with pytest.raises(ValueError, match="device tensor"):
            c.embedding_lookup_sum_planned(bad, bag=bag)
    with pytest.raises(ValueError, match="comes first"):
        c.embedding_update_planned_bags(good, bag=bag)
    c = _cache_with_a_planned_batch(n, width, looked_up=True)
    with pytest.raises(ValueError, match="device tensor"):
        c.embedding_update_planned_bags(good, bag=bag)
    with pytest.raises(ValueError, match="no planned batch is due"):
        c.embedding_lookup_sum_planned(good, bag=bag)
    assert len(c._planned) == 1 and c._planned[0][1] is True             # nothing was consumed


class _Shaped:
    """A tensor stand-in that claims to live on a device: reaches the shape checks of _pooled_args."""

    def __init__(self, t):
        self._t = t

    def __getattr__(self, name):
        return True if name == "is_cuda" else getattr(self._t, name)


def test_python_shape_checks(monkeypatch):
    n, width, bag = 8, 4, 2
    c = _cache_with_a_planned_batch(n, width, looked_up=False)
    monkeypatch.setattr(torch, "is_tensor", lambda x: isinstance(x, (torch.Tensor, _Shaped)))
    ok = _Shaped(torch.zeros((n // bag, width)))
    off = _Shaped(torch.zeros(n // bag + 1, dtype=torch.int64))
    assert c._pooled_args("t", "out", ok, n, bag, None, "offsets") == n // bag
    assert c._pooled_args("t", "out", ok, n, None, off, "offsets") == n // bag
    for x, kw, msg in [
        (_Shaped(torch.zeros((n // bag, width + 1))), dict(bag=bag), "device tensor"),          # wrong width
        (_Shaped(torch.zeros(n // bag * width)), dict(bag=bag), "device tensor"),               # not 2-D
        (_Shaped(torch.zeros((n // bag, width), dtype=torch.float64)), dict(bag=bag), "device tensor"),
        (_Shaped(torch.zeros((width, n // bag)).t()), dict(bag=bag), "device tensor"),          # not contiguous
        (ok, dict(bag=bag + 1), "are not the planned batch"),                                   # nbags * bag != n
        (_Shaped(torch.zeros((n // bag + 1, width))), dict(bag=bag), "are not the planned batch"),
        (ok, dict(bag=0), "are not the planned batch"),
        (ok, dict(bag=bag, offsets=off), "exactly one"),
        (ok, dict(), "exactly one"),
        (ok, dict(offsets=_Shaped(torch.zeros(n // bag, dtype=torch.int64))), "offsets must be"),      # not nbags + 1 entries
        (ok, dict(offsets=_Shaped(torch.zeros(n // bag + 1, dtype=torch.int32))), "offsets must be"),
    ]:
        with pytest.raises(ValueError, match=msg):
            c.embedding_lookup_sum_planned(x, **kw)
    c = _cache_with_a_planned_batch(n, width, looked_up=True)
    for kw, msg in [
        (dict(bag=bag + 1), "are not the planned batch"),
        (dict(bag=bag, bag_of=_Shaped(torch.zeros(n, dtype=torch.int32))), "exactly one"),
        (dict(), "exactly one"),
        (dict(bag_of=_Shaped(torch.zeros(n + 1, dtype=torch.int32))), "bag_of must be"),
        (dict(bag_of=_Shaped(torch.zeros(n, dtype=torch.int64))), "bag_of must be"),
    ]:
        with pytest.raises(ValueError, match=msg):
            c.embedding_update_planned_bags(ok, **kw)
    assert len(c._planned) == 1


def test_python_methods_of_the_pooled_flow():
    for cls in (hcache.LRUCache, hcache.LFUCache, hcache.LFUOptCache, hcache.CacheSparseTable):
        assert callable(cls.embedding_lookup_sum_planned) and callable(cls.embedding_update_planned_bags)
        assert callable(cls.run_planned_pairs_bags)
    import inspect
    for name in ("embedding_lookup_sum_planned", "embedding_update_planned_bags"):
        assert inspect.signature(getattr(hcache.CacheSparseTable, name)).parameters["sync"].default is False
    from herald_amd import hetu_ops
    assert hetu_ops.Config().cache_fuse_bags is True
    assert inspect.signature(hetu_ops.ParameterServerCommunicateOp.__init__).parameters["bag"].default is None

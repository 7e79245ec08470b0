"""CPU-side checks of the planned push-pull chain's interface: the three entry points are declared in include/herald_amd.h
with the argument lists herald_amd/_lib.py binds, the library exports them, and the Python methods exist."""
import ctypes
import inspect
import re

from herald_amd import _lib
from herald_amd import cache as hcache

NEW = {
    "ha_cache_plan_block_push_pull": ["ha_cache *", "const void *const *", "int", "const int64_t *", "int", "ha_stream_t", "ha_stream_t"],
    "ha_cache_push_pull_planned": ["ha_cache *", "int64_t", "float *", "int64_t", "const float *", "ha_stream_t"],
    "ha_cache_run_planned_push_pulls": ["ha_cache *", "int", "const int64_t *", "float *const *", "const int64_t *",
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


def test_header_declares_the_chain_entry_points():
    for name, want in NEW.items():
        assert _header_args(name) == want, name
        assert name in _lib.declared_symbols()


def test_library_exports_and_binds_the_chain_entry_points(lib):
    ctype_of = {"int": ctypes.c_int, "int64_t": ctypes.c_int64}
    for name, want in NEW.items():
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int
        assert len(fn.argtypes) == len(want), name
        for got, decl in zip(fn.argtypes, want):
            assert got is ctype_of.get(decl, ctypes.c_void_p), (name, decl, got)


def test_python_methods_of_the_chain():
    for cls in (hcache.LRUCache, hcache.CacheSparseTable):
        sig = inspect.signature(cls.plan_block)
        assert sig.parameters["push_pull"].default is False
        assert callable(cls.embedding_push_pull_planned) and callable(cls.run_planned_push_pulls)

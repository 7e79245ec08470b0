"""CPU-side checks of the pooled push-pull chain's interface: the two entry points are declared in include/herald_amd.h with the
argument lists herald_amd/_lib.py binds, the library exports them, and the Python methods check their arguments -- shapes, and
which of `bag` / the ragged descriptions describes which side of which entry -- before any native call (no device is touched)."""
import ctypes
import inspect

import pytest
import torch

from herald_amd import _lib
from herald_amd import cache as hcache
from test_cache_bags_api import _NoDevice, _Shaped, _header_args

NEW = {
    "ha_cache_push_pull_planned_bags": ["ha_cache *", "int64_t", "int64_t", "int64_t", "const int64_t *", "float *", "int64_t",
                                        "int64_t", "int64_t", "const int32_t *", "const float *", "ha_stream_t"],
    "ha_cache_run_planned_push_pulls_bags": ["ha_cache *", "int", "int64_t", "int64_t", "int64_t", "float *const *",
                                             "const float *const *", "ha_stream_t"],
}


def test_header_declares_the_pooled_chain_entry_points():
    for name, want in NEW.items():
        assert _header_args(name) == want, name
        assert name in _lib.declared_symbols()


def test_library_exports_and_binds_the_pooled_chain_entry_points(lib):
    ctype_of = {"int": ctypes.c_int, "int64_t": ctypes.c_int64}
    for name, want in NEW.items():
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int
        assert len(fn.argtypes) == len(want), name
        for got, decl in zip(fn.argtypes, want):
            assert got is ctype_of.get(decl, ctypes.c_void_p), (name, decl, got)


def test_native_null_handle_is_refused_with_the_entry_name(lib):
    assert lib.ha_cache_push_pull_planned_bags(None, 8, 2, 4, None, None, 8, 2, 4, None, None, None) == -1
    assert b"cache_push_pull_planned_bags" in lib.ha_last_error()
    assert lib.ha_cache_run_planned_push_pulls_bags(None, 1, 8, 2, 4, None, None, None) == -1
    assert b"cache_run_planned_push_pulls_bags" in lib.ha_last_error()


def _cache_with_a_chain(entries, width):
    """entries: (kind, n_pull or None, n_push or None), the chain list plan_block(..., push_pull=True) leaves."""
    c = hcache.LRUCache.__new__(hcache.LRUCache)
    c._h = None
    c._L = _NoDevice()
    c._stream = _NoDevice()
    c._width = width
    keys = lambda m: None if m is None else torch.zeros(m, dtype=torch.float32)
    c._chain = [[kind, keys(a), keys(b)] for kind, a, b in entries]
    return c


def test_python_argument_checks_raise_without_touching_a_device(monkeypatch):
    n, width, bag = 8, 4, 2
    B = n // bag
    cpu = torch.zeros((B, width), dtype=torch.float32)                  # right shape, but a CPU tensor
    c = _cache_with_a_chain([("step", n, n)], width)
    for bad in (cpu, cpu.numpy()):
        with pytest.raises(ValueError, match="device tensor"):
            c.embedding_push_pull_planned_bags(bad, bad, bag=bag)
    monkeypatch.setattr(torch, "is_tensor", lambda x: isinstance(x, (torch.Tensor, _Shaped)))
    ok = _Shaped(torch.zeros((B, width)))
    off = _Shaped(torch.zeros(B + 1, dtype=torch.int64))
    bof = _Shaped(torch.zeros(n, dtype=torch.int32))
    # ---- a middle step
    assert c._chain_bags_args("t", 0, ok, ok, bag, None, None)[3:] == (B, B, bag, bag)
    assert c._chain_bags_args("t", 0, ok, ok, bag, off, None)[3:] == (B, B, None, bag)
    assert c._chain_bags_args("t", 0, ok, ok, bag, None, bof)[3:] == (B, B, bag, None)
    assert c._chain_bags_args("t", 0, ok, ok, None, off, bof)[3:] == (B, B, None, None)
    for args, kw, msg in [
        ((None, ok), dict(bag=bag), "out is missing"),                                          # a missing side
        ((ok, None), dict(bag=bag), "bag_grads is missing"),
        ((ok, ok), dict(), "exactly one"),                                                      # neither, on both sides
        ((ok, ok), dict(pull_offsets=off), "exactly one"),                                      # neither, on the push side
        ((ok, ok), dict(push_bag_of=bof), "exactly one"),                                       # neither, on the pull side
        ((ok, ok), dict(bag=bag, pull_offsets=off, push_bag_of=bof), "exactly one"),            # bag and both descriptions
        ((ok, ok), dict(bag=bag + 1), "are not the planned batch"),
        ((ok, ok), dict(bag=0), "are not the planned batch"),
        ((_Shaped(torch.zeros((B + 1, width))), ok), dict(bag=bag), "are not the planned batch"),
        ((ok, _Shaped(torch.zeros((B - 1, width)))), dict(bag=bag), "are not the planned batch"),
        ((_Shaped(torch.zeros((B, width + 1))), ok), dict(bag=bag), "device tensor"),           # wrong width
        ((ok, _Shaped(torch.zeros(B * width))), dict(bag=bag), "device tensor"),                # not 2-D
        ((ok, _Shaped(torch.zeros((B, width), dtype=torch.float64))), dict(bag=bag), "device tensor"),
        ((_Shaped(torch.zeros((width, B)).t()), ok), dict(bag=bag), "device tensor"),           # not contiguous
        ((ok, ok), dict(bag=bag, pull_offsets=_Shaped(torch.zeros(B, dtype=torch.int64))), "pull_offsets must be"),
        ((ok, ok), dict(bag=bag, pull_offsets=_Shaped(torch.zeros(B + 1, dtype=torch.int32))), "pull_offsets must be"),
        ((ok, ok), dict(bag=bag, push_bag_of=_Shaped(torch.zeros(n + 1, dtype=torch.int32))), "push_bag_of must be"),
        ((ok, ok), dict(bag=bag, push_bag_of=_Shaped(torch.zeros(n, dtype=torch.int64))), "push_bag_of must be"),
    ]:
        with pytest.raises(ValueError, match=msg):
            c.embedding_push_pull_planned_bags(*args, **kw)
    with pytest.raises(ValueError, match="2 outs, 1 bag_grads"):
        c.run_planned_push_pulls_bags([ok, ok], [ok], bag)
    with pytest.raises(ValueError, match="no entry"):                   # two steps asked for, one planned
        c.run_planned_push_pulls_bags([ok, ok], [ok, ok], bag)
    with pytest.raises(ValueError, match="are not the planned batch"):
        c.run_planned_push_pulls_bags([ok], [ok], bag + 1)
    with pytest.raises(ValueError, match="fixed bags only"):
        c.run_planned_push_pulls_bags([ok], [ok], None)
    assert len(c._chain) == 1                                           # nothing was consumed
    # ---- the head pushes nothing, the closing entry pulls nothing
    c = _cache_with_a_chain([("head", n, None)], width)
    assert c._chain_bags_args("t", 0, ok, None, bag, None, None)[3:] == (B, 0, bag, None)
    assert c._chain_bags_args("t", 0, ok, None, None, off, None)[3:] == (B, 0, None, None)
    for args, kw, msg in [
        ((ok, ok), dict(bag=bag), "head"),
        ((ok, None), dict(bag=bag, push_bag_of=bof), "head"),
        ((None, None), dict(bag=bag), "out is missing"),
        ((ok, None), dict(), "exactly one"),
        ((ok, None), dict(bag=bag, pull_offsets=off), "exactly one"),
    ]:
        with pytest.raises(ValueError, match=msg):
            c.embedding_push_pull_planned_bags(*args, **kw)
    with pytest.raises(ValueError, match="no push-pull step is due"):
        c.run_planned_push_pulls_bags([ok], [ok], bag)
    c = _cache_with_a_chain([("close", None, n)], width)
    assert c._chain_bags_args("t", 0, None, ok, bag, None, None)[3:] == (0, B, None, bag)
    assert c._chain_bags_args("t", 0, None, ok, None, None, bof)[3:] == (0, B, None, None)
    for args, kw, msg in [
        ((ok, ok), dict(bag=bag), "closes the chain"),
        ((None, ok), dict(bag=bag, pull_offsets=off), "closes the chain"),
        ((None, None), dict(bag=bag), "bag_grads is missing"),
        ((None, ok), dict(), "exactly one"),
        ((None, ok), dict(bag=bag, push_bag_of=bof), "exactly one"),
    ]:
        with pytest.raises(ValueError, match=msg):
            c.embedding_push_pull_planned_bags(*args, **kw)
    assert len(c._chain) == 1
    # ---- no chain, or a chain with nothing planned
    c = _cache_with_a_chain([], width)
    with pytest.raises(ValueError, match="no entry"):
        c.embedding_push_pull_planned_bags(ok, ok, bag=bag)
    del c._chain
    c._planned = [[torch.zeros(n), False, None]]                        # a pair block is not a chain
    with pytest.raises(ValueError, match="no entry"):
        c.embedding_push_pull_planned_bags(ok, None, bag=bag)
    assert c._planned[0][1] is False


def test_python_methods_of_the_pooled_chain():
    for cls in (hcache.LRUCache, hcache.LFUCache, hcache.LFUOptCache, hcache.CacheSparseTable):
        assert callable(cls.embedding_push_pull_planned_bags) and callable(cls.run_planned_push_pulls_bags)
        p = inspect.signature(cls.embedding_push_pull_planned_bags).parameters
        assert [k for k in p][1:6] == ["out", "bag_grads", "bag", "pull_offsets", "push_bag_of"]
        assert p["bag"].default is None and p["pull_offsets"].default is None and p["push_bag_of"].default is None
        assert [k for k in inspect.signature(cls.run_planned_push_pulls_bags).parameters][1:] == ["outs", "bag_grads", "bag"]
    assert inspect.signature(hcache.CacheSparseTable.embedding_push_pull_planned_bags).parameters["sync"].default is False

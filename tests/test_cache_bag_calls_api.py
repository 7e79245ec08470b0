"""CPU-side checks of the interface of sum-pooled access through the cache's CALL-BY-CALL entry points: every new entry point is
declared in include/herald_amd.h with the argument list herald_amd/_lib.py binds, the library exports them, their native argument
checks refuse a null handle and bad sizes with the function's name in ha_last_error(), and the Python methods refuse bad bag /
offsets / bag_of / shapes before any native call (no device is touched)."""
import ctypes
import inspect

import pytest
import torch

from herald_amd import _lib, hetu_ops
from herald_amd import cache as hcache
from test_cache_bags_api import _NoDevice, _Shaped, _header_args

C, K, I, N = "ha_cache *", "const void *", "int", "int64_t"
NEW = {
    "ha_cache_lookup_sum": [C, K, I, N, N, N, "const int64_t *", "float *", "ha_stream_t"],
    "ha_cache_lookup_sum_presorted": [C, K, I, N, N, N, "const int64_t *", "float *", "ha_stream_t"],
    "ha_cache_lookup_sum_finish": [C, N, N, N, "const int64_t *", "float *", "ha_stream_t"],
    "ha_cache_update_bags": [C, K, I, N, "const float *", N, N, "const int32_t *", "ha_stream_t"],
    "ha_cache_update_same_keys_bags": [C, N, "const float *", N, N, "const int32_t *", "ha_stream_t"],
    "ha_cache_update_with_push_keys_bags": [C, K, I, N, K, I, N, "const float *", N, N, "const int32_t *", "ha_stream_t"],
    "ha_cache_push_pull_bags": [C, K, I, N, N, N, "const int64_t *", "float *", K, I, N, "const float *", N, N,
                                "const int32_t *", "ha_stream_t"],
    "ha_cache_push_pull_begin_bags": [C, K, I, N, K, I, N, "const float *", N, N, "const int32_t *", "int64_t *", "ha_stream_t"],
    "ha_cache_push_pull_finish_sum": [C, N, N, "const int64_t *", "float *", "ha_stream_t"],
    "ha_apply_mapped2_bags": ["float *", N, "float *", N, K, N, "const float *", "float", "const int32_t *", "const int32_t *", N,
                              "const int32_t *", "const uint8_t *", "ha_stream_t"],
}


def test_header_declares_the_pooled_call_by_call_entry_points():
    for name, want in NEW.items():
        assert _header_args(name) == want, name
        assert name in _lib.declared_symbols()


def test_library_exports_and_binds_them(lib):
    ctype_of = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
    for name, want in NEW.items():
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int
        assert len(fn.argtypes) == len(want), name
        for got, decl in zip(fn.argtypes, want):
            assert got is ctype_of.get(decl, ctypes.c_void_p), (name, decl, got)


def test_native_checks_refuse_a_null_handle_with_the_entry_name(lib):
    calls = {
        "ha_cache_lookup_sum": (None, None, 0, 8, 2, 4, None, None, None),
        "ha_cache_lookup_sum_presorted": (None, None, 0, 8, 2, 4, None, None, None),
        "ha_cache_lookup_sum_finish": (None, 8, 2, 4, None, None, None),
        "ha_cache_update_bags": (None, None, 0, 8, None, 2, 4, None, None),
        "ha_cache_update_same_keys_bags": (None, 8, None, 2, 4, None, None),
        "ha_cache_update_with_push_keys_bags": (None, None, 0, 8, None, 0, 0, None, 2, 4, None, None),
        "ha_cache_push_pull_bags": (None, None, 0, 8, 2, 4, None, None, None, 0, 8, None, 2, 4, None, None),
        "ha_cache_push_pull_begin_bags": (None, None, 0, 8, None, 0, 8, None, 2, 4, None, None, None),
        "ha_cache_push_pull_finish_sum": (None, 2, 4, None, None, None),
    }
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == -1, name
        assert name.encode() in lib.ha_last_error(), (name, lib.ha_last_error())


def test_native_checks_refuse_bad_sizes_before_any_device_access(lib):
    """A handle that is no cache: were it dereferenced before the size checks the process would fault; the checks come first."""
    h = ctypes.c_void_p(8)
    one = ctypes.c_void_p(16)      # a non-null pointer that is never read
    bad = [
        ("ha_cache_lookup_sum", (h, one, 0, 8, 3, 4, None, one, None)),              # 3 bags of 4 are not 8 ids
        ("ha_cache_lookup_sum", (h, one, 0, 8, 2, 4, one, one, None)),               # bag and offsets
        ("ha_cache_lookup_sum", (h, one, 0, 8, 2, 0, None, one, None)),              # neither
        ("ha_cache_lookup_sum", (h, one, 0, 8, 2, 4, None, None, None)),             # null output
        ("ha_cache_lookup_sum", (h, one, 0, -1, 0, 1, None, None, None)),            # negative n
        ("ha_cache_lookup_sum_presorted", (h, one, 0, 8, 0, 0, one, one, None)),     # ids in no bag
        ("ha_cache_lookup_sum_finish", (h, 8, 2, 3, None, one, None)),
        ("ha_cache_update_bags", (h, one, 0, 8, one, 2, 3, None, None)),             # 8 is no multiple of 3
        ("ha_cache_update_bags", (h, one, 0, 8, one, 2, 4, one, None)),              # bag and bag_of
        ("ha_cache_update_bags", (h, one, 0, 8, None, 2, 4, None, None)),            # null bag_grads
        ("ha_cache_update_same_keys_bags", (h, 8, one, 4, 4, None, None)),           # 4 bags of 4 are not 8 ids
        ("ha_cache_update_with_push_keys_bags", (h, one, 0, 8, one, 0, 2, one, 2, 0, None, None)),
        ("ha_cache_push_pull_begin_bags", (h, one, 0, 8, one, 0, 8, one, 2, 3, None, None, None)),
        ("ha_apply_mapped2_bags", (one, 4, one, 4, one, 8, one, 1.0, one, one, 3, None, None, None)),
        ("ha_apply_mapped2_bags", (one, 4, one, 4, one, 8, one, 1.0, one, one, 0, None, None, None)),
        ("ha_apply_mapped2_bags", (one, 4, one, 0, one, 8, one, 1.0, one, one, 4, None, None, None)),     # width 0
        ("ha_apply_mapped2_bags", (None, 4, one, 4, one, 8, one, 1.0, one, one, 4, None, None, None)),    # null dst
    ]
    for name, args in bad:
        assert getattr(lib, name)(*args) == -1, (name, args)
        assert name.encode() in lib.ha_last_error(), (name, lib.ha_last_error())
    assert lib.ha_apply_mapped2_bags(None, 0, None, 4, None, 0, None, 1.0, None, None, 4, None, None, None) == 0     # n == 0


def _cache(width, remote=False):
    c = hcache.LRUCache.__new__(hcache.LRUCache)
    c._h = None
    c._L = _NoDevice()
    c._stream = _NoDevice()
    c._width = width
    c._remote = _NoDevice() if remote else None
    return c


@pytest.mark.parametrize("remote", [False, True])
def test_python_argument_checks_raise_without_touching_a_device(monkeypatch, remote):
    n, width, bag = 8, 4, 2
    B = n // bag
    keys = torch.zeros(n, dtype=torch.float32)
    c = _cache(width, remote)
    cpu = torch.zeros((B, width), dtype=torch.float32)                  # right shape, but a CPU tensor
    for bad in (cpu, cpu.numpy(), None):
        with pytest.raises(ValueError, match="device tensor"):
            c.embedding_lookup_sum(keys, bad, bag=bag)
        with pytest.raises(ValueError, match="device tensor"):
            c.embedding_update_bags(keys, bad, bag=bag)
        with pytest.raises(ValueError, match="device tensor"):
            c.embedding_update_with_push_keys_bags(keys, keys[:2], bad, bag=bag)
        with pytest.raises(ValueError, match="device tensor"):
            c.embedding_push_pull_bags(keys, bad, keys, bad, bag=bag)
    monkeypatch.setattr(torch, "is_tensor", lambda x: isinstance(x, (torch.Tensor, _Shaped)))
    ok = _Shaped(torch.zeros((B, width)))
    off = _Shaped(torch.zeros(B + 1, dtype=torch.int64))
    bof = _Shaped(torch.zeros(n, dtype=torch.int32))
    shapes = [
        (_Shaped(torch.zeros((B, width + 1))), dict(bag=bag), "device tensor"),                 # wrong width
        (_Shaped(torch.zeros(B * width)), dict(bag=bag), "device tensor"),                      # not 2-D
        (_Shaped(torch.zeros((B, width), dtype=torch.float64)), dict(bag=bag), "device tensor"),
        (_Shaped(torch.zeros((width, B)).t()), dict(bag=bag), "device tensor"),                 # not contiguous
        (ok, dict(bag=bag + 1), "bags of"),                                                     # nbags * bag != n
        (_Shaped(torch.zeros((B + 1, width))), dict(bag=bag), "bags of"),
        (ok, dict(bag=0), "bags of"),
        (ok, dict(), "exactly one"),
    ]
    for x, kw, msg in shapes + [
        (ok, dict(bag=bag, offsets=off), "exactly one"),
        (ok, dict(offsets=_Shaped(torch.zeros(B, dtype=torch.int64))), "offsets must be"),      # not nbags + 1 entries
        (ok, dict(offsets=_Shaped(torch.zeros(B + 1, dtype=torch.int32))), "offsets must be"),
    ]:
        with pytest.raises(ValueError, match=msg):
            c.embedding_lookup_sum(keys, x, **kw)
    for x, kw, msg in shapes + [
        (ok, dict(bag=bag, bag_of=bof), "exactly one"),
        (ok, dict(bag_of=_Shaped(torch.zeros(n + 1, dtype=torch.int32))), "bag_of must be"),
        (ok, dict(bag_of=_Shaped(torch.zeros(n, dtype=torch.int64))), "bag_of must be"),
    ]:
        with pytest.raises(ValueError, match=msg):
            c.embedding_update_bags(keys, x, **kw)
        with pytest.raises(ValueError, match=msg):
            c.embedding_update_with_push_keys_bags(keys, keys[:3], x, **kw)
    for args, kw, msg in [
        ((ok, ok), dict(), "exactly one"),
        ((ok, ok), dict(pull_offsets=off), "exactly one"),                                      # neither, on the push side
        ((ok, ok), dict(push_bag_of=bof), "exactly one"),                                       # neither, on the pull side
        ((ok, ok), dict(bag=bag, pull_offsets=off, push_bag_of=bof), "exactly one"),            # bag and both descriptions
        ((ok, ok), dict(bag=bag + 1), "bags of"),
        ((_Shaped(torch.zeros((B + 1, width))), ok), dict(bag=bag), "bags of"),
        ((ok, _Shaped(torch.zeros((B - 1, width)))), dict(bag=bag), "bags of"),
        ((_Shaped(torch.zeros((B, width + 1))), ok), dict(bag=bag), "device tensor"),
        ((ok, ok), dict(bag=bag, pull_offsets=_Shaped(torch.zeros(B, dtype=torch.int64))), "pull_offsets must be"),
        ((ok, ok), dict(bag=bag, push_bag_of=_Shaped(torch.zeros(n, dtype=torch.int64))), "push_bag_of must be"),
    ]:
        with pytest.raises(ValueError, match=msg):
            c.embedding_push_pull_bags(keys, args[0], keys, args[1], **kw)
    with pytest.raises(TypeError, match="keys must be"):
        c.embedding_lookup_sum([1, 2], ok, bag=bag)


def test_python_methods_and_the_switch():
    for cls in (hcache.LRUCache, hcache.LFUCache, hcache.LFUOptCache, hcache.CacheSparseTable):
        p = inspect.signature(cls.embedding_lookup_sum).parameters
        assert [k for k in p][1:5] == ["keys", "out", "bag", "offsets"] and p["bag"].default is None and p["offsets"].default is None
        p = inspect.signature(cls.embedding_update_bags).parameters
        assert [k for k in p][1:5] == ["keys", "bag_grads", "bag", "bag_of"] and p["same_as_lookup"].default is False
        p = inspect.signature(cls.embedding_update_with_push_keys_bags).parameters
        assert [k for k in p][1:6] == ["keys", "push_keys", "bag_grads", "bag", "bag_of"]
        p = inspect.signature(cls.embedding_push_pull_bags).parameters
        assert [k for k in p][1:8] == ["pullkeys", "out", "pushkeys", "bag_grads", "bag", "pull_offsets", "push_bag_of"]
    assert inspect.signature(hcache.CacheSparseTable.embedding_lookup_sum).parameters["sync"].default is False
    assert hetu_ops.Config().cache_fuse_bag_calls is False
    assert hetu_ops.Config(cache_fuse_bag_calls=True).cache_fuse_bag_calls is True

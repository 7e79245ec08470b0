"""CPU-side checks of the pooled framed step's interface: the new entry points are declared in include/herald_amd.h with the
argument lists herald_amd/_lib.py binds, the library exports them, and every one of them refuses bad arguments before any
device access (no device is touched: there is none here)."""
import ctypes
import re

from herald_amd import _lib

P, I, F32 = "ptr", "int64_t", "float"
NEW = {
    "ha_gather2_sum_u32map": [P, I, P, I, I, P, I, I, P, I, P, P],
    "ha_apply_mapped_bags": [P, I, I, P, I, P, F32, P, I, P, P, P],
    "ha_push_apply_scaled_bags_finished": [P, I, I, P, I, P, I, P, F32, P],
    "ha_shard_step_pull_sum": [P, I, I, P, P, P, P, I, I, I, P, P, P],
    "ha_shard_step_push_bags": [P, I, I, P, P, P, I, P, P, I, I, P, F32, P],
    "ha_shard_step_bags": [P, I, I, P, P, P, P, I, P, I, P, I, I, P, P, P, P, F32, P],
    "ha_shard_steps_bags": [P, I, I, I, P, P, P, P, I, P, I, P, P, P, P, P, P, P, F32, P],
}


def _header_kinds(name):
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;{}]*)\)\s*;" % name, text)
    assert m, "%s is not declared in the header" % name
    out = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        a = re.sub(r"\s*\b\w+$", "", a).strip()       # drop the parameter's name
        out.append(P if ("*" in a or a == "ha_stream_t") else a)
    return out


def test_header_declares_the_pooled_step_entry_points():
    for name, want in NEW.items():
        assert _header_kinds(name) == want, name
        assert name in _lib.declared_symbols()


def test_library_exports_and_binds_the_pooled_step_entry_points(lib):
    ctype_of = {I: ctypes.c_int64, F32: ctypes.c_float, P: ctypes.c_void_p}
    for name, want in NEW.items():
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int
        assert [t for t in fn.argtypes] == [ctype_of[k] for k in want], name


def _slot(world=1, rank=0, n=52):
    d = _lib.ShardSlot()
    d.world, d.rank, d.rcap, d.n = world, rank, 64, n
    return d


def test_native_argument_checks_come_before_any_device_access(lib):
    vp = ctypes.c_void_p
    bad = vp(0x10)                      # never dereferenced: every call below fails in its checks
    f = ctypes.c_float(1.0)
    assert lib.ha_gather2_sum_u32map(bad, 5, bad, 5, 8, bad, 52, 26, bad, 2, bad, None) == -1          # bag and offsets
    assert b"ha_gather2_sum_u32map" in lib.ha_last_error()
    assert lib.ha_apply_mapped_bags(bad, 5, 8, bad, 52, bad, f, bad, 25, None, None, None) == -1
    assert b"ha_apply_mapped_bags" in lib.ha_last_error()
    assert lib.ha_push_apply_scaled_bags_finished(bad, 5, 8, bad, 52, bad, 0, None, f, None) == -1
    assert b"ha_push_apply_scaled_bags_finished" in lib.ha_last_error()
    s = _slot()
    sp = ctypes.byref(s)
    # pull: no slot, both bag and offsets, n that is not nbags bags, no output
    assert lib.ha_shard_step_pull_sum(bad, 5, 8, None, None, None, None, 0, 2, 26, None, bad, None) == -1
    assert lib.ha_shard_step_pull_sum(bad, 5, 8, sp, None, None, None, 0, 2, 26, bad, bad, None) == -1
    assert lib.ha_shard_step_pull_sum(bad, 5, 8, sp, None, None, None, 0, 3, 26, None, bad, None) == -1
    assert lib.ha_shard_step_pull_sum(bad, 5, 8, sp, None, None, None, 0, 2, 26, None, None, None) == -1
    assert b"ha_shard_step_pull_sum" in lib.ha_last_error()
    # push: neither bag nor bag_of, no gradient
    assert lib.ha_shard_step_push_bags(bad, 5, 8, sp, None, None, 0, None, bad, 2, 0, None, f, None) == -1
    assert lib.ha_shard_step_push_bags(bad, 5, 8, sp, None, None, 0, None, None, 2, 26, None, f, None) == -1
    assert b"ha_shard_step_push_bags" in lib.ha_last_error()
    # world > 1 without the exchange
    s2 = _slot(world=2)
    assert lib.ha_shard_step_pull_sum(bad, 5, 8, ctypes.byref(s2), None, bad, bad, 128, 2, 26, None, bad, None) == -1
    assert lib.ha_shard_step_bags(bad, 5, 8, sp, None, None, None, 0, None, 0, None, 3, 26, None, None, bad, bad, f, None) == -1
    # a run of steps: the SECOND step's arguments are bad -- nothing of the first is enqueued (there is no device to enqueue on)
    slots = (ctypes.POINTER(_lib.ShardSlot) * 2)(ctypes.pointer(s), ctypes.pointer(s))
    i64s, vps = ctypes.c_int64 * 2, vp * 2
    assert lib.ha_shard_steps_bags(bad, 5, 8, 2, slots, None, None, None, 0, None, 0, None, i64s(2, 3), i64s(26, 26),
                                   vps(None, None), vps(None, None), vps(0x10, 0x10), vps(0x10, 0x10), f, None) == -1
    assert b"ha_shard_steps_bags" in lib.ha_last_error()
    assert lib.ha_shard_steps_bags(bad, 5, 8, 0, None, None, None, None, 0, None, 0, None, None, None, None, None, None, None,
                                   f, None) == 0                       # no steps: nothing to do

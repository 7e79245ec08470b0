"""ha_gather2_sum_u32map, the sized expand of the sharded step fused with the sum over each bag: against ha_gather2_u32map
followed by embedding_lookup_sum over the delivered rows (ids 0 .. n-1), and against the numpy position-ordered float32 chain
(tests/bag_model.py) over the rows the map names.  Hand-made maps mix own-shard words (bit 31), received-row indices, indices
beyond either array and 0xFFFFFFFF.  Every comparison is on float32 bit patterns."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bag_model  # noqa: E402

from herald_amd import _lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = -123.456
T_ROWS, R_ROWS = 211, 157
_src = {}


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _sources(width):
    """(table, recv) per width, shared and never written: magnitudes over many binades so that the order of a sum shows."""
    if width not in _src:
        rng = np.random.default_rng(2000 + width)
        mk = lambda rows: (rng.standard_normal((rows, width)) * np.exp(rng.uniform(-8, 8, (rows, 1)))).astype(np.float32)
        _src[width] = (mk(T_ROWS), mk(R_ROWS))
    return _src[width]


def _map(n, seed, t_rows=T_ROWS, r_rows=R_ROWS):
    """uint32 map words: own-shard rows, received rows, repeats, and -- where there is room -- an index beyond each array and
    the zero-row word."""
    rng = np.random.default_rng(seed)
    own = rng.random(n) < 0.5
    m = np.where(own, 0x80000000 | rng.integers(0, max(t_rows, 1), n), rng.integers(0, max(r_rows, 1), n)).astype(np.uint32)
    m[: n // 3] = m[0]
    if n > 6:
        m[n - 2] = 0x80000000 | (t_rows + 5)        # beyond the shard
        m[n - 3] = r_rows + 3                       # beyond the received rows
        m[n - 4] = 0xFFFFFFFF
        m[n - 5] = 0x7FFFFFFF
    return rng.permutation(m)


def _rows_of(m, table, recv, width):
    """The row ha_gather2_u32map writes for every position."""
    own = (m >> 31) != 0
    r = (m & 0x7FFFFFFF).astype(np.int64)
    rows = np.zeros((m.size, width), dtype=np.float32)
    t_rows = 0 if table is None else table.shape[0]
    r_rows = 0 if recv is None else recv.shape[0]
    a = own & (r < t_rows)
    b = ~own & (r < r_rows)
    if a.any():
        rows[a] = table[r[a]]
    if b.any():
        rows[b] = recv[r[b]]
    return rows


def _check(dev, width, m, B=None, offsets=None, table="shared", recv="shared", d_recv=None):
    t_np, r_np = _sources(width)
    table = t_np if isinstance(table, str) else table
    recv = r_np if isinstance(recv, str) else recv
    n = m.size
    d_table = torch.from_numpy(table).to(dev) if table is not None else None
    if d_recv is None:
        d_recv = torch.from_numpy(recv).to(dev) if recv is not None else None
    d_map = torch.from_numpy(m.view(np.int32)).to(dev)
    d_off = torch.from_numpy(np.asarray(offsets, dtype=np.int64)).to(dev) if offsets is not None else None
    nbags = B if offsets is None else len(offsets) - 1
    bag = (n // B if B else 26) if offsets is None else None
    out = torch.full((nbags, width), CANARY, dtype=torch.float32, device=dev)
    got = ops.gather2_sum_u32map(d_table, d_recv, d_map, bag=bag, offsets=d_off, nbags=nbags, out=out)
    assert got is out
    rows = _rows_of(m, table, recv, width)
    pos = np.arange(n, dtype=np.int64)
    want = bag_model.bag_sum(rows, pos.reshape(B, -1) if offsets is None else pos, offsets) if n or offsets is not None \
        else np.zeros((nbags, width), np.float32)
    assert np.array_equal(_bits(got), _bits(want))
    # the unfused pair on the device: the expand, then the sum over the delivered rows
    if n and ((table is not None and table.shape[0]) or (recv is not None and recv.shape[0])):
        delivered = torch.full((n, width), CANARY, dtype=torch.float32, device=dev)
        L = _lib.load()
        vp = ctypes.c_void_p
        assert L.ha_gather2_u32map(vp(d_table.data_ptr()) if d_table is not None else None, table.shape[0] if table is not None else 0,
                                   vp(d_recv.data_ptr()) if d_recv is not None else None, recv.shape[0] if recv is not None else 0,
                                   width, vp(d_map.data_ptr()), n, vp(delivered.data_ptr()), None) == 0
        assert np.array_equal(_bits(delivered), _bits(rows))
        d_pos = torch.arange(n, dtype=torch.float32, device=dev)
        twin = ops.embedding_lookup_sum(delivered, d_pos.view(B, -1) if offsets is None else d_pos, offsets=d_off)
        assert np.array_equal(_bits(got), _bits(twin))
    if nbags and n:
        assert not np.array_equal(_bits(got), _bits(np.full(want.shape, CANARY, np.float32)))
    if d_table is not None:
        assert np.array_equal(_bits(d_table), _bits(table))
    assert np.array_equal(d_map.cpu().numpy().view(np.uint32), m)
    return got


@pytest.mark.parametrize("F", [1, 8, 9, 26, 64, 65, 130])       # 8 / 9: the ROWS switch; 64 / 65 / 130: the 64-position block
def test_gather2_sum_fixed_bags(dev, F):
    for width in (33, 64, 128, 512, 1024):                      # B = 4: 64-float slices (width 33: the scalar path)
        _check(dev, width, _map(4 * F, 10 * F + width), B=4)


@pytest.mark.parametrize("B,F,width", [(2048, 26, 128), (2048, 8, 128), (1024, 9, 512), (2048, 8, 64)])
def test_gather2_sum_wide_slices(dev, B, F, width):
    """Enough (bag, slice) waves for the 128- and 256-float slices: 2,048 bags of 128 floats take VEC 2, 1,024 bags of 512
    floats VEC 4 in two slices, 2,048 bags of 64 floats VEC 1."""
    _check(dev, width, _map(B * F, B + F), B=B)


def test_gather2_sum_every_slice_width(dev):
    m = _map(33 * 26, 5)
    L = _lib.load()
    try:
        for floats in (64, 128, 256):                   # 516 floats: a partial last slice in each
            assert L.ha_debug_bag_slice(floats) == 0
            _check(dev, 516, m, B=33)
    finally:
        L.ha_debug_bag_slice(0)


def test_gather2_sum_ragged_bags_and_the_clamp(dev):
    n = 300
    m = _map(n, 77)
    offsets = [0, 0, 0, 200, 200, 201, 230, 230, 300, 300, 300]      # empty bags at the front, in the middle, at the end
    for width in (33, 64, 516):
        _check(dev, width, m, offsets=offsets)
    for width in (33, 64):                                           # offsets outside [0, n] and a decreasing one: clamped
        _check(dev, width, m, offsets=[0, 50, 40, 290, 350, 1000])
        _check(dev, width, m, offsets=[-5, 3, 9, 300])
    _check(dev, 64, _map(40, 3), offsets=[0, 3, 5, 9, 12, 40])       # bags of at most 8 positions on average: ROWS 8


def test_gather2_sum_misaligned_recv_takes_the_scalar_path(dev):
    width = 64
    _, recv = _sources(width)
    base = torch.zeros(R_ROWS * width + 4, dtype=torch.float32, device=dev)
    d_recv = base[1:1 + R_ROWS * width].view(R_ROWS, width)          # 4 bytes into its allocation
    d_recv.copy_(torch.from_numpy(recv))
    assert d_recv.data_ptr() % 16 == 4
    m = _map(20 * 26, 3)
    got = _check(dev, width, m, B=20, d_recv=d_recv)
    aligned = _check(dev, width, m, B=20)
    assert np.array_equal(_bits(got), _bits(aligned))


def test_gather2_sum_a_side_without_rows_is_never_read(dev):
    width = 64
    table, recv = _sources(width)
    n = 12 * 26
    remote = _map(n, 8, t_rows=0) & np.uint32(0x7FFFFFFF)            # every position names a received row (or none)
    remote[5] = 0x80000000 | 3                                       # ... but one own-shard word: the shard has no rows -> zeros
    _check(dev, width, remote, B=12, table=None)
    local = _map(n, 9, r_rows=0) | np.uint32(0x80000000)
    local[7] = 4                                                     # a received-row index with nothing received -> zeros
    _check(dev, width, local, B=12, recv=None)
    out = _check(dev, width, _map(n, 10), B=12, table=table[:0], recv=recv[:0])     # neither side has rows: all zeros
    assert not out.any()


def test_gather2_sum_no_bags_and_no_positions(dev):
    width = 64
    got = _check(dev, width, np.zeros(0, np.uint32), B=0)
    assert got.shape == (0, width)
    got = _check(dev, width, np.zeros(0, np.uint32), offsets=[0, 0, 0, 0, 0])       # n = 0, four empty bags
    assert np.array_equal(_bits(got), np.zeros((4, width), np.int32))


def test_gather2_sum_argument_errors_come_before_any_device_access(dev):
    L = _lib.load()
    vp = ctypes.c_void_p
    bad = vp(0x10)           # never dereferenced: every call below must fail in its checks
    call = lambda *a: L.ha_gather2_sum_u32map(*a, None)
    assert call(bad, 5, bad, 5, 8, bad, 52, 26, bad, 2, bad) != 0           # both bag and offsets
    assert call(bad, 5, bad, 5, 8, bad, 52, 0, None, 2, bad) != 0           # neither
    assert call(bad, 5, bad, 5, 8, bad, 52, 26, None, 3, bad) != 0          # 52 positions are not 3 bags of 26
    assert call(bad, 5, bad, 5, 0, bad, 52, 26, None, 2, bad) != 0          # width
    assert call(bad, -1, bad, 5, 8, bad, 52, 26, None, 2, bad) != 0         # rows
    assert call(bad, 5, bad, -1, 8, bad, 52, 26, None, 2, bad) != 0         # recv_rows
    assert call(bad, 5, bad, 5, 8, bad, 52, 26, None, 2, None) != 0         # no output
    assert call(None, 5, bad, 5, 8, bad, 52, 26, None, 2, bad) != 0         # rows without a table
    assert call(bad, 5, None, 5, 8, bad, 52, 26, None, 2, bad) != 0         # received rows without a buffer
    assert call(bad, 5, bad, 5, 8, None, 52, 26, None, 2, bad) != 0         # no map
    assert b"ha_gather2_sum_u32map" in L.ha_last_error()
    torch.cuda.synchronize()

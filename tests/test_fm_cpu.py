"""CPU-side checks of the FM-pooled lookup (the DeepFM models): the three new calls are declared and exported, their arguments
are validated before any device access, and the numpy restatement the GPU tests are held to (tests/fm_model.py) is itself held
to the float64 formulas within bounds that follow from its float32 operations."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bag_model  # noqa: E402
import fm_model  # noqa: E402

from herald_amd import _lib  # noqa: E402

SYMBOLS = ["ha_gather_fm_f32ids", "ha_gather_fm_u64ids", "ha_fm_grad_rows"]
EPS32 = 2.0 ** -24      # unit roundoff of float32


def test_fm_symbols_are_declared_and_exported(lib):
    declared = _lib.declared_symbols()
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name


# a non-null address that is never dereferenced: validation comes before any device access (there is no GPU here)
P = ctypes.c_void_p(0x1000)


@pytest.mark.parametrize("fn", ["ha_gather_fm_f32ids", "ha_gather_fm_u64ids"])
@pytest.mark.parametrize("case,args", [
    ("neither bag nor offsets", dict(bag=0, offsets=None)),
    ("both bag and offsets", dict(bag=2, offsets=P)),
    ("n not a multiple of bag", dict(n=7, bag=2, nbags=3)),
    ("n is not nbags * bag", dict(n=8, bag=2, nbags=3)),
    ("width 0", dict(width=0)),
    ("negative width", dict(width=-4)),
    ("negative n", dict(n=-1)),
    ("negative rows", dict(rows=-1)),
    ("null out_sum", dict(out_sum=None)),
    ("null out_fm", dict(out_fm=None)),
    ("null table", dict(table=None)),
])
def test_gather_fm_rejects_bad_arguments_before_any_device_access(lib, fn, case, args):
    a = dict(table=P, rows=10, width=4, ids=P, n=8, bag=2, offsets=None, nbags=4, out_rows=P, out_sum=P, out_fm=P)
    a.update(args)
    rc = getattr(lib, fn)(a["table"], a["rows"], a["width"], a["ids"], a["n"], a["bag"], a["offsets"], a["nbags"],
                          a["out_rows"], a["out_sum"], a["out_fm"], None)
    assert rc == -1, case
    assert fn.encode() in lib.ha_last_error(), (case, lib.ha_last_error())


@pytest.mark.parametrize("case,args", [
    ("neither bag nor bag_of", dict(bag=0, bag_of=None)),
    ("both bag and bag_of", dict(bag=2, bag_of=P)),
    ("n not a multiple of bag", dict(n=7, bag=2, nbags=3)),
    ("n is not nbags * bag", dict(n=8, bag=2, nbags=3)),
    ("width 0", dict(width=0)),
    ("negative n", dict(n=-1)),
    ("null emb_rows", dict(emb_rows=None)),
    ("null sum", dict(sum=None)),
    ("null g_fm", dict(g_fm=None)),
    ("null out", dict(out=None)),
    ("out aliases emb_rows", dict(out=ctypes.c_void_p(0x2000), emb_rows=ctypes.c_void_p(0x2000))),
    ("ragged occurrences in no bag", dict(bag=0, bag_of=P, nbags=0)),
])
def test_fm_grad_rows_rejects_bad_arguments_before_any_device_access(lib, case, args):
    a = dict(g_rows=P, emb_rows=ctypes.c_void_p(0x3000), sum=ctypes.c_void_p(0x4000), g_fm=ctypes.c_void_p(0x5000), n=8,
             width=4, bag=2, bag_of=None, nbags=4, out=P)
    a.update(args)
    rc = lib.ha_fm_grad_rows(a["g_rows"], a["emb_rows"], a["sum"], a["g_fm"], a["n"], a["width"], a["bag"], a["bag_of"],
                             a["nbags"], a["out"], None)
    assert rc == -1, case
    assert b"ha_fm_grad_rows" in lib.ha_last_error(), (case, lib.ha_last_error())


def test_nothing_to_do_is_not_an_error(lib):
    assert lib.ha_gather_fm_f32ids(P, 10, 4, None, 0, 2, None, 0, None, None, None, None) == 0       # no bags
    assert lib.ha_fm_grad_rows(None, None, None, None, 0, 4, 2, None, 0, None, None) == 0             # no occurrences


def _table(rows, width, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((rows, width)) * np.exp(rng.uniform(-6, 6, (rows, 1)))).astype(np.float32)


@pytest.mark.parametrize("F", [1, 2, 26, 65])
def test_restatement_sum_is_the_bag_sum_and_fm_is_within_the_bound_of_the_float64_formula(F):
    """S is bag_model.bag_sum bit for bit.  fm against 0.5 * (S^2 - Q) in float64, within 4 * F * eps32 * (S*S + Q) per element
    (S, Q the float64 sum and sum of squares): Q is a sequential float32 sum of F rounded products, (F + 1) eps Q at most; S is
    a sequential sum of F terms and the three closing operations add an eps each."""
    rows, width, B = 500, 37, 33
    table = _table(rows, width, F)
    rng = np.random.default_rng(100 + F)
    ids = rng.integers(0, rows, (B, F)).astype(np.float32)
    erows, covered, S, fm = fm_model.fm_lookup(table, ids)
    assert S.dtype == fm.dtype == erows.dtype == np.float32 and covered.all()
    assert np.array_equal(S.view(np.int32), bag_model.bag_sum(table, ids).view(np.int32))
    assert np.array_equal(erows, table[ids.astype(np.int64).reshape(-1)])
    picked = table[ids.astype(np.int64)].astype(np.float64)              # [B, F, width]
    S64, Q64 = picked.sum(axis=1), (picked * picked).sum(axis=1)
    want = 0.5 * (S64 * S64 - Q64)
    bound = 4 * F * EPS32 * (S64 * S64 + Q64)
    assert np.all(np.abs(fm.astype(np.float64) - want) <= bound)
    # ragged bags with the same contents give the same bits
    offsets = np.arange(B + 1, dtype=np.int64) * F
    r2, c2, S2, fm2 = fm_model.fm_lookup(table, ids.reshape(-1), offsets)
    assert c2.all() and np.array_equal(S2.view(np.int32), S.view(np.int32)) and np.array_equal(fm2.view(np.int32), fm.view(np.int32))
    assert np.array_equal(r2, erows)


@pytest.mark.parametrize("with_rows", [True, False])
def test_restatement_gradient_is_within_the_bound_of_the_float64_formula(with_rows):
    """g + gf * (S - e) in float64 against the three rounded products / sums: each of the at most four float32 operations adds
    a relative eps on a quantity bounded by |g| + |gf*S| + |gf*e|."""
    rows, width, B, F = 300, 29, 17, 26
    table = _table(rows, width, 5)
    rng = np.random.default_rng(6)
    ids = rng.integers(0, rows, (B, F)).astype(np.float32)
    e, _, S, _ = fm_model.fm_lookup(table, ids)
    g = rng.standard_normal((B * F, width)).astype(np.float32) if with_rows else None
    gf = rng.standard_normal((B, width)).astype(np.float32)
    got = fm_model.fm_grad_rows(g, e, S, gf, bag=F)
    assert got.dtype == np.float32 and got.shape == (B * F, width)
    b = np.arange(B * F) // F
    g64 = g.astype(np.float64) if with_rows else np.zeros((B * F, width))
    gfS, gfe = gf[b].astype(np.float64) * S[b].astype(np.float64), gf[b].astype(np.float64) * e.astype(np.float64)
    want = g64 + gfS - gfe
    assert np.all(np.abs(got.astype(np.float64) - want) <= 4 * EPS32 * (np.abs(g64) + np.abs(gfS) + np.abs(gfe)))
    # ragged bags with the same contents give the same bits
    offsets = np.arange(B + 1, dtype=np.int64) * F
    assert np.array_equal(fm_model.fm_grad_rows(g, e, S, gf, offsets=offsets).view(np.int32), got.view(np.int32))


def test_restatement_edge_cases():
    table = np.array([[-0.0, -0.0], [1.5, -2.5], [0.25, 4.0]], dtype=np.float32)
    # a bag of one row: S = r, Q = r*r, fm = 0.5 * (r*r - r*r) = +0
    _, _, S, fm = fm_model.fm_lookup(table, np.array([[1.0]], dtype=np.float32))
    assert np.array_equal(S, table[1:2]) and np.array_equal(fm.view(np.int32), np.zeros((1, 2), np.int32))
    # an id >= rows is a zero row everywhere; an empty bag gives zeros; offsets are clamped; a first offset above 0 and a last
    # one below n leave occurrences in no bag
    ids = np.array([2, 1, 7, 2, 1], dtype=np.float32)
    offsets = np.array([1, 1, 4, 4], dtype=np.int64)
    rows, covered, S, fm = fm_model.fm_lookup(table, ids, offsets)
    assert list(covered) == [False, True, True, True, False]
    assert np.array_equal(rows[2], np.zeros(2, np.float32))
    assert np.array_equal(S, np.array([[0, 0], [1.75, 1.5], [0, 0]], dtype=np.float32))
    # bag 1: rows (1.5, -2.5), 0, (0.25, 4): Q = (2.3125, 22.25); fm = 0.5 * (S*S - Q)
    assert np.array_equal(fm[1], np.array([0.5 * (1.75 * 1.75 - 2.3125), 0.5 * (1.5 * 1.5 - 22.25)], dtype=np.float32))
    assert np.array_equal(fm[0], np.zeros(2, np.float32)) and np.array_equal(fm[2], np.zeros(2, np.float32))
    # the gradient: (g + gf*S) - gf*e
    g = np.full((2, 2), 1.0, dtype=np.float32)
    e = np.array([[1.0, 2.0], [3.0, 4.0]], dtype=np.float32)
    S1 = np.array([[4.0, 6.0]], dtype=np.float32)
    gf = np.array([[0.5, -1.0]], dtype=np.float32)
    assert np.array_equal(fm_model.fm_grad_rows(g, e, S1, gf, bag=2), np.array([[2.5, -3.0], [1.5, -1.0]], dtype=np.float32))
    assert np.array_equal(fm_model.fm_grad_rows(None, e, S1, gf, bag=2), np.array([[1.5, -4.0], [0.5, -2.0]], dtype=np.float32))

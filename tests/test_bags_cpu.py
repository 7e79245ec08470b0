"""CPU-side checks of the sum-pooled lookup ("bags"): the new symbols are declared and exported, arguments are validated
before any device access, and the numpy restatement the GPU tests are held to (tests/bag_model.py) is itself held to a
float64 sum within the bound of a sequential float32 summation."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bag_model  # noqa: E402

from herald_amd import _lib  # noqa: E402

SYMBOLS = ["ha_gather_sum_f32ids", "ha_gather_sum_u64ids", "ha_bag_of", "ha_sgd_apply_bags",
           "ha_sgd_sparse_update_bags_f32ids", "ha_sgd_sparse_update_bags_u64ids"]


def test_bag_symbols_are_declared_and_exported(lib):
    declared = _lib.declared_symbols()
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name


# a non-null address that is never dereferenced: validation comes before any device access (there is no GPU here)
P = ctypes.c_void_p(0x1000)


@pytest.mark.parametrize("fn", ["ha_gather_sum_f32ids", "ha_gather_sum_u64ids"])
@pytest.mark.parametrize("case,args", [
    ("bag = 0 without offsets", dict(bag=0, offsets=None)),
    ("both bag and offsets", dict(bag=2, offsets=P)),
    ("n not a multiple of bag", dict(n=7, bag=2, nbags=3)),
    ("n is not nbags * bag", dict(n=8, bag=2, nbags=3)),
    ("negative n", dict(n=-1)),
    ("negative rows", dict(rows=-1)),
    ("width 0", dict(width=0)),
    ("negative nbags", dict(nbags=-1)),
    ("negative bag", dict(bag=-2)),
    ("null table", dict(table=None)),
])
def test_gather_sum_rejects_bad_arguments_before_any_device_access(lib, fn, case, args):
    a = dict(table=P, rows=10, width=4, ids=P, n=8, bag=2, offsets=None, nbags=4, out=P)
    a.update(args)
    rc = getattr(lib, fn)(a["table"], a["rows"], a["width"], a["ids"], a["n"], a["bag"], a["offsets"], a["nbags"], a["out"],
                          None)
    assert rc == -1, case
    assert fn.encode() in lib.ha_last_error(), (case, lib.ha_last_error())


@pytest.mark.parametrize("case,args", [
    ("bag = 0 without bag_of", dict(bag=0, bag_of=None)),
    ("both bag and bag_of", dict(bag=2, bag_of=P)),
    ("n not a multiple of bag", dict(n=7, bag=2)),
    ("negative n", dict(n=-1)),
    ("negative rows", dict(rows=-1)),
    ("width 0", dict(width=0)),
    ("null table", dict(table=None)),
])
def test_sgd_apply_bags_rejects_bad_arguments_before_any_device_access(lib, case, args):
    a = dict(table=P, rows=10, width=4, plan=P, n=8, grads=P, bag=2, bag_of=None)
    a.update(args)
    rc = lib.ha_sgd_apply_bags(a["table"], a["rows"], a["width"], a["plan"], a["n"], a["grads"], a["bag"], a["bag_of"],
                               ctypes.c_float(0.1), None)
    assert rc == -1, case
    assert b"ha_sgd_apply_bags" in lib.ha_last_error(), (case, lib.ha_last_error())


@pytest.mark.parametrize("fn", ["ha_sgd_sparse_update_bags_f32ids", "ha_sgd_sparse_update_bags_u64ids"])
@pytest.mark.parametrize("case,args", [
    ("bag = 0 without offsets", dict(bag=0, offsets=None)),
    ("both bag and offsets", dict(bag=2, offsets=P)),
    ("n not a multiple of bag", dict(n=7, bag=2, nbags=3)),
    ("negative n", dict(n=-1)),
    ("negative rows", dict(rows=-1)),
    ("null table", dict(table=None)),
])
def test_one_call_form_rejects_bad_arguments_before_any_device_access(lib, fn, case, args):
    a = dict(table=P, rows=10, width=4, ids=P, n=8, grads=P, bag=2, offsets=None, nbags=4)
    a.update(args)
    rc = getattr(lib, fn)(a["table"], a["rows"], a["width"], a["ids"], a["n"], a["grads"], a["bag"], a["offsets"],
                          a["nbags"], ctypes.c_float(0.1), None)
    assert rc == -1, case
    assert fn.encode() in lib.ha_last_error(), (case, lib.ha_last_error())


def test_bag_of_rejects_bad_arguments_before_any_device_access(lib):
    assert lib.ha_bag_of(P, -1, 4, P, None) == -1 and b"ha_bag_of" in lib.ha_last_error()
    assert lib.ha_bag_of(P, 0, 4, P, None) == -1 and b"ha_bag_of" in lib.ha_last_error()      # ids in no bag
    assert lib.ha_bag_of(None, 2, 4, P, None) == -1 and b"ha_bag_of" in lib.ha_last_error()
    assert lib.ha_bag_of(None, 2, 0, None, None) == 0                                          # nothing to do


@pytest.mark.parametrize("F", [1, 2, 26, 65])
def test_restatement_is_within_the_sequential_sum_bound_of_a_float64_sum(F):
    """|bag_sum - sum64| <= F * 2^-24 * sum|r_j| elementwise: gamma_{F-1} * sum|x| of a sequential sum, rounded up."""
    rng = np.random.default_rng(F)
    rows, width, B = 500, 37, 33
    table = (rng.standard_normal((rows, width)) * np.exp(rng.uniform(-6, 6, (rows, 1)))).astype(np.float32)
    ids = rng.integers(0, rows, (B, F)).astype(np.float32)
    got = bag_model.bag_sum(table, ids)
    assert got.dtype == np.float32 and got.shape == (B, width)
    picked = table[ids.astype(np.int64)].astype(np.float64)              # [B, F, width]
    want, mag = picked.sum(axis=1), np.abs(picked).sum(axis=1)
    assert np.all(np.abs(got.astype(np.float64) - want) <= F * 2.0 ** -24 * mag)
    # ragged bags with the same contents give the same bits
    offsets = np.arange(B + 1, dtype=np.int64) * F
    assert np.array_equal(bag_model.bag_sum(table, ids.reshape(-1), offsets).view(np.int32), got.view(np.int32))


def test_restatement_edge_cases():
    table = np.array([[-0.0, -0.0], [1.5, -2.5], [0.25, 4.0]], dtype=np.float32)
    # a row of -0.0 in a bag of one sums to +0.0: the chain starts from +0.0f
    out = bag_model.bag_sum(table, np.array([[0.0]], dtype=np.float32))
    assert np.array_equal(out.view(np.int32), np.zeros((1, 2), np.int32))
    # an id >= rows contributes a zero row; an empty bag gives zeros; offsets beyond n are clamped
    ids = np.array([1, 7, 2, 1], dtype=np.float32)
    offsets = np.array([0, 0, 3, 3, 9], dtype=np.int64)
    out = bag_model.bag_sum(table, ids, offsets)
    assert np.array_equal(out, np.array([[0, 0], [1.75, 1.5], [0, 0], [1.5, -2.5]], dtype=np.float32))
    assert list(bag_model.bag_of(np.array([0, 0, 3, 3, 4], dtype=np.int64), 4)) == [1, 1, 1, 3]
    # the pooled SGD restatement is the per-occurrence update on the expanded gradient
    g = np.array([[1, 2], [3, 4]], dtype=np.float32)
    ids2 = np.array([[1, 1], [2, 9]], dtype=np.float32)
    want = table.copy()
    for i, r in enumerate([1, 1, 2]):
        want[r] = want[r] - np.float32(0.1) * g[i // 2]
    assert np.array_equal(bag_model.sgd_bags(table, ids2, g, 0.1), want)
    assert np.array_equal(bag_model.sgd_bags(table, ids2.reshape(-1), g, 0.1, np.array([0, 2, 4], dtype=np.int64)), want)

"""Identities of tests/wshard_model.py, the numpy restatement of ha_gather_wsum_u32keys / ha_dedup_reduce_wbags: what the GPU
tests compare the kernels against must itself agree with the weighted bags on a table (wbag_model) and with the plain
occurrence-order chain over the expanded gradient."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bag_model      # noqa: E402
import wbag_model     # noqa: E402
import wshard_model   # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _case(seed, rows=37, width=5, B=11, F=7, dead=0.5):
    rng = np.random.default_rng(seed)
    table = rng.standard_normal((rows, width), dtype=np.float32)
    ids = rng.integers(0, rows, size=(B, F)).astype(np.float32)
    w = rng.standard_normal((B, F), dtype=np.float32)
    deadm = rng.random((B, F)) < dead
    w[deadm] = np.where(rng.random(int(deadm.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
    ids[deadm] = 0      # the padding id: one long run, all dead (unless id 0 is drawn live too)
    return table, ids, w


def _offsets(n, nbags, seed):
    cuts = np.sort(np.random.default_rng(seed).integers(0, n + 1, nbags - 3))
    return np.concatenate([[0, 0], cuts, [n, n]]).astype(np.int64)


@pytest.mark.parametrize("ragged", [False, True])
def test_pull_model_over_the_unique_rows_is_the_weighted_bag_on_the_table(ragged):
    table, ids, w = _case(1)
    uniq, inv = np.unique(ids.reshape(-1).astype(np.int64), return_inverse=True)
    rows_buf = table[uniq]
    if ragged:
        off = _offsets(ids.size, 9, 4)
        got = wshard_model.gather_wsum_u32keys(rows_buf, inv, w, offsets=off)
        want = wbag_model.wbag_sum(table, ids.reshape(-1), w.reshape(-1), off)
    else:
        got = wshard_model.gather_wsum_u32keys(rows_buf, inv, w, bag=ids.shape[1])
        want = wbag_model.wbag_sum(table, ids, w)
    np.testing.assert_array_equal(_bits(got), _bits(want))
    assert np.any(got)


@pytest.mark.parametrize("scale", [1.0, -0.05])
@pytest.mark.parametrize("ragged", [False, True])
def test_reduce_model_is_the_plain_chain_over_the_expanded_gradient(scale, ragged):
    _, ids, w = _case(2)
    n = ids.size
    rng = np.random.default_rng(5)
    g = rng.standard_normal((9 if ragged else ids.shape[0], 6), dtype=np.float32)
    g[rng.random(g.shape) < 0.3] = 0      # zero gradient elements: with scale < 0 the composed sequence adds -0 terms
    off = _offsets(n, 9, 6) if ragged else None
    which = wshard_model.which_of(n, bag=ids.shape[1], offsets=off)
    uniq, inv = np.unique(ids.reshape(-1).astype(np.int64), return_inverse=True)
    got = wshard_model.dedup_reduce_wbags(inv, uniq.size, g, w, which, scale)
    rows = wbag_model.wbag_grad_rows(g, w, which)                   # +0 rows for the dead occurrences
    want = wshard_model.reduce_rows_scaled(inv, uniq.size, rows, scale)      # every occurrence takes part, as -0 or +0
    np.testing.assert_array_equal(_bits(got), _bits(want))
    assert not np.any(_bits(got) == np.int32(-2 ** 31)), "a chain from +0 never holds -0"
    assert np.any(got)


def test_negative_scale_with_all_zero_gradients_changes_no_bit():
    _, ids, w = _case(3, dead=0.3)
    n = ids.size
    g = np.zeros((ids.shape[0], 4), dtype=np.float32)
    which = wshard_model.which_of(n, bag=ids.shape[1])
    uniq, inv = np.unique(ids.reshape(-1).astype(np.int64), return_inverse=True)
    got = wshard_model.dedup_reduce_wbags(inv, uniq.size, g, w, which, -0.05)
    want = wshard_model.reduce_rows_scaled(inv, uniq.size, wbag_model.wbag_grad_rows(g, w, which), -0.05)
    np.testing.assert_array_equal(_bits(got), _bits(want))
    assert not np.any(_bits(got)), "every row is +0.0f"


def test_all_ones_weights_are_the_unweighted_chains():
    table, ids, _ = _case(4, dead=0.0)
    w = np.ones(ids.shape, dtype=np.float32)
    uniq, inv = np.unique(ids.reshape(-1).astype(np.int64), return_inverse=True)
    got = wshard_model.gather_wsum_u32keys(table[uniq], inv, w, bag=ids.shape[1])
    np.testing.assert_array_equal(_bits(got), _bits(bag_model.bag_sum(table, ids)))
    g = np.random.default_rng(8).standard_normal((ids.shape[0], 6), dtype=np.float32)
    which = wshard_model.which_of(ids.size, bag=ids.shape[1])
    red = wshard_model.dedup_reduce_wbags(inv, uniq.size, g, w, which, -0.05)
    np.testing.assert_array_equal(_bits(red), _bits(wshard_model.reduce_rows_scaled(inv, uniq.size, g[which], -0.05)))


def test_dead_occurrences_keep_inf_and_nan_out():
    table, ids, w = _case(6)
    n = ids.size
    g = np.random.default_rng(9).standard_normal((ids.shape[0], 3), dtype=np.float32)
    dead_bags = np.all(w == 0, axis=1)
    w[0] = 0      # at least one bag whose occurrences are all dead
    g[0] = [np.inf, np.nan, -np.inf]
    which = wshard_model.which_of(n, bag=ids.shape[1])
    uniq, inv = np.unique(ids.reshape(-1).astype(np.int64), return_inverse=True)
    red = wshard_model.dedup_reduce_wbags(inv, uniq.size, g, w, which, 1.0)
    assert np.all(np.isfinite(red)) and dead_bags.shape == (ids.shape[0],)


def test_the_new_symbols_are_declared_and_exported(lib):
    from herald_amd import _lib
    names = _lib.declared_symbols()
    for n in ("ha_gather_wsum_u32keys", "ha_dedup_reduce_wbags"):
        assert n in names and hasattr(lib, n)
    # every argument check precedes any device access (there is no GPU here)
    assert lib.ha_gather_wsum_u32keys(None, 0, 4, None, None, 3, 3, None, 1, None, None) == -1
    assert b"rows" in lib.ha_last_error()
    assert lib.ha_dedup_reduce_wbags(None, 6, None, None, 4, 0, None, 2, 1.0, None, None) == -1
    assert b"exactly one" in lib.ha_last_error()
    assert lib.ha_dedup_reduce_wbags(None, 6, None, None, 4, 3, None, 2, 1.0, None, None) == -1
    assert b"null" in lib.ha_last_error()
    assert lib.ha_dedup_reduce_wbags(None, 0, None, None, 4, 3, None, 0, 1.0, None, None) == 0

"""Numpy restatement of the sum-pooled lookup ("bags") and its sparse SGD apply (include/herald_amd.h, ha_gather_sum_* /
ha_bag_of / ha_sgd_apply_bags).  Test infrastructure only: nothing under herald_amd/ imports it.

Every sum is a sequential chain of float32 additions in position order, every update a float32 multiply followed by a
float32 subtract -- the order and the roundings the kernels are held to bit for bit."""
import numpy as np

import special_ids


def clamp_offsets(offsets, n):
    """The bag bounds the kernels use: every offset clamped to [0, n], a bag's end to its start."""
    offsets = np.asarray(offsets, dtype=np.int64)
    lo = np.clip(offsets[:-1], 0, n)
    hi = np.maximum(np.clip(offsets[1:], 0, n), lo)
    return lo, hi


def bag_bounds(n_or_ids_shape, offsets=None):
    """(lo, hi) per bag: fixed bags from an ids shape [B, F], ragged ones from offsets[B + 1]."""
    if offsets is None:
        b, f = n_or_ids_shape
        lo = np.arange(b, dtype=np.int64) * f
        return lo, lo + f
    return clamp_offsets(offsets, int(n_or_ids_shape))


def ids_to_rows(ids):
    """(size_t)ids[i] of the reference: float32 ids truncate toward zero, integer ids are keys as they are; an id that
    names no row of any table (negative, NaN, infinite, beyond 32 bits) is special_ids.DEAD_KEY, never a negative index."""
    return special_ids.rows_of(ids)


def bag_sum(table, ids, offsets=None):
    """out[b, :] = ((0.0f + r_0) + r_1) + ... + r_{m-1}; an id >= rows is a zero row, an empty bag gives zeros."""
    table = np.asarray(table, dtype=np.float32)
    rows, width = table.shape
    flat = ids_to_rows(ids)
    lo, hi = bag_bounds(np.asarray(ids).shape if offsets is None else flat.size, offsets)
    if offsets is None:      # fixed bags: the same chain per element, all bags at once
        fixed = flat.reshape(np.asarray(ids).shape)
        acc = np.full((fixed.shape[0], width), np.float32(0), dtype=np.float32)
        for j in range(fixed.shape[1]):
            r = fixed[:, j]
            ok = (r >= 0) & (r < rows)
            term = np.where(ok[:, None], table[np.where(ok, r, 0)], np.float32(0)).astype(np.float32)
            acc = (acc + term).astype(np.float32)
        return acc
    out = np.empty((lo.size, width), dtype=np.float32)
    zero = np.zeros(width, dtype=np.float32)
    for b in range(lo.size):
        acc = np.full(width, np.float32(0), dtype=np.float32)
        for j in range(int(lo[b]), int(hi[b])):
            r = flat[j]
            acc = (acc + (table[r] if 0 <= r < rows else zero)).astype(np.float32)
        out[b] = acc
    return out


def bag_of(offsets, n):
    """bag_of[i] = the largest b in [0, B) with offsets[b] <= i (empty bags are skipped), by the kernel's own bisection."""
    offsets = np.asarray(offsets, dtype=np.int64)
    nbags = offsets.size - 1
    out = np.empty(n, dtype=np.int32)
    for i in range(n):
        lo, hi = 0, nbags
        while hi - lo > 1:
            mid = (lo + hi) >> 1
            if offsets[mid] <= i:
                lo = mid
            else:
                hi = mid
        out[i] = lo
    return out


def sgd_bags(table, ids, bag_grads, lr, offsets=None):
    """table[key_i, :] -= lr * bag_grads[bag of i, :] for i ascending; an id >= rows is ignored."""
    table = np.array(table, dtype=np.float32, copy=True)
    rows = table.shape[0]
    flat = ids_to_rows(ids)
    bag_grads = np.asarray(bag_grads, dtype=np.float32)
    if offsets is None:
        which = np.arange(flat.size) // np.asarray(ids).shape[1]
    else:
        which = bag_of(offsets, flat.size)
    lr = np.float32(lr)
    for i in range(flat.size):
        r = flat[i]
        if 0 <= r < rows:
            table[r] = (table[r] - (lr * bag_grads[which[i]]).astype(np.float32)).astype(np.float32)
    return table

"""Numpy restatement of the weighted bags (include/herald_amd.h, ha_gather_wsum_* / ha_wbag_grad_rows / ha_sgd_apply_wbags): the
masked sum-pooled lookup of the FAE models and its sparse SGD apply.  Test infrastructure only: nothing under herald_amd/
imports it.

Every chain is sequential float32 arithmetic with each rounding explicit.  An occurrence is LIVE when its weight is not zero
(+0 and -0 are zero, NaN is not) and its id is below rows; a dead occurrence takes no part in anything."""
import numpy as np

import bag_model


def _f32(x):
    return np.asarray(x, dtype=np.float32)


def live_mask(rows, ids, weights):
    flat = bag_model.ids_to_rows(ids)
    w = _f32(weights).reshape(-1)
    return (w != 0) & (flat >= 0) & (flat < rows)      # (NaN != 0 is True)


def wbag_sum(table, ids, weights, offsets=None):
    """out[b, c]: acc = +0; acc = fl(acc + fl(w_j * r_j[c])) over the live occurrences of bag b in position order."""
    table = _f32(table)
    rows, width = table.shape
    flat = bag_model.ids_to_rows(ids)
    w = _f32(weights).reshape(-1)
    live = live_mask(rows, ids, weights)
    lo, hi = bag_model.bag_bounds(np.asarray(ids).shape if offsets is None else flat.size, offsets)
    out = np.empty((lo.size, width), dtype=np.float32)
    with np.errstate(all="ignore"):
        for b in range(lo.size):
            acc = np.zeros(width, dtype=np.float32)
            for j in range(int(lo[b]), int(hi[b])):
                if live[j]:
                    term = (w[j] * table[flat[j]]).astype(np.float32)
                    acc = (acc + term).astype(np.float32)
            out[b] = acc
    return out


def which_bag(ids, offsets=None):
    flat_n = np.asarray(ids).size
    if offsets is None:
        return np.arange(flat_n) // np.asarray(ids).shape[1]
    return bag_model.bag_of(offsets, flat_n)


def wbag_grad_rows(bag_grads, weights, which):
    """out[i, c] = fl(w_i * g[which[i], c]); exactly +0 where w_i is zero, whatever g holds."""
    g = _f32(bag_grads)
    w = _f32(weights).reshape(-1)
    out = np.zeros((w.size, g.shape[1]), dtype=np.float32)
    with np.errstate(all="ignore"):
        for i in range(w.size):
            if w[i] != 0:
                out[i] = (w[i] * g[which[i]]).astype(np.float32)
    return out


def wbag_sgd(table, ids, weights, bag_grads, lr, offsets=None):
    """row = fl(row - fl(lr * fl(w_i * g[bag(i), :]))) over the live occurrences i ascending; everything else keeps its bits."""
    table = np.array(table, dtype=np.float32, copy=True)
    rows = table.shape[0]
    flat = bag_model.ids_to_rows(ids)
    w = _f32(weights).reshape(-1)
    g = _f32(bag_grads)
    live = live_mask(rows, ids, weights)
    which = which_bag(ids, offsets)
    lr = np.float32(lr)
    with np.errstate(all="ignore"):
        for i in range(flat.size):
            if live[i]:
                wg = (w[i] * g[which[i]]).astype(np.float32)
                table[flat[i]] = (table[flat[i]] - (lr * wg).astype(np.float32)).astype(np.float32)
    return table


def sgd_rows(table, ids, grads, lr):
    """The unpooled serial apply (ha_sgd_apply): row = fl(row - fl(lr * grads[i])) for i ascending, ids >= rows ignored."""
    table = np.array(table, dtype=np.float32, copy=True)
    rows = table.shape[0]
    flat = bag_model.ids_to_rows(ids)
    lr = np.float32(lr)
    with np.errstate(all="ignore"):
        for i in range(flat.size):
            if 0 <= flat[i] < rows:
                table[flat[i]] = (table[flat[i]] - (lr * grads[i]).astype(np.float32)).astype(np.float32)
    return table


def compact(ids, weights, offsets=None):
    """The ragged bags left when the occurrences of zero weight are deleted: (ids [m], offsets [B + 1])."""
    flat = np.asarray(ids).reshape(-1)
    w = _f32(weights).reshape(-1)
    lo, hi = bag_model.bag_bounds(np.asarray(ids).shape if offsets is None else flat.size, offsets)
    keep = w != 0
    out_ids, out_off = [], [0]
    for b in range(lo.size):
        sel = np.arange(int(lo[b]), int(hi[b]))
        sel = sel[keep[sel]]
        out_ids.append(flat[sel])
        out_off.append(out_off[-1] + sel.size)
    return np.concatenate(out_ids) if out_ids else flat[:0], np.array(out_off, dtype=np.int64)

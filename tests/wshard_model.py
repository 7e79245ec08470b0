"""Numpy restatement of the weighted bags of the row-sharded table (include/herald_amd.h, ha_gather_wsum_u32keys /
ha_dedup_reduce_wbags): the two end steps of ShardedEmbedding.pull_wsum / push_wbags.  Test infrastructure only: nothing under
herald_amd/ imports it.

Every chain is sequential float32 arithmetic with each rounding explicit (wbag_model.py's rules: an occurrence is live when its
weight is not zero; +0 and -0 are zero, NaN is not)."""
import numpy as np

import bag_model
import wbag_model


def _f32(x):
    return np.asarray(x, dtype=np.float32)


def gather_wsum_u32keys(rows_buf, keys, weights, bag=None, offsets=None):
    """out[b, c]: acc = +0; acc = fl(acc + fl(w_j * rows_buf[keys[j], c])) over the live occurrences of bag b in position order
    (live: weight not zero and key < rows).  keys: integers [n]; fixed bags of `bag` keys, or ragged ones by offsets[B + 1]."""
    ids = np.asarray(keys).reshape(-1).astype(np.int64)      # (integer ids are keys as they are)
    if offsets is None:
        return wbag_model.wbag_sum(rows_buf, ids.reshape(-1, int(bag)), _f32(weights).reshape(-1, int(bag)))
    return wbag_model.wbag_sum(rows_buf, ids, _f32(weights).reshape(-1), offsets)


def dedup_reduce_wbags(inverse, n_unique, bag_grads, weights, which, scale):
    """reduced[u, c]: acc = +0; acc = fl(acc + fl(scale * fl(w_i * g[which[i], c]))) over the occurrences i of unique key u
    (inverse[i] == u) in ascending order whose weight is not zero; a key without one gets +0.  Returns [n_unique, width]."""
    g = _f32(bag_grads)
    w = _f32(weights).reshape(-1)
    scale = np.float32(scale)
    red = np.zeros((n_unique, g.shape[1]), dtype=np.float32)
    with np.errstate(all="ignore"):
        for i, u in enumerate(np.asarray(inverse).reshape(-1)):
            if w[i] != 0:      # (NaN != 0 is True)
                wg = (w[i] * g[which[i]]).astype(np.float32)
                red[u] = (red[u] + (scale * wg).astype(np.float32)).astype(np.float32)
    return red


def reduce_rows_scaled(inverse, n_unique, grads, scale):
    """The unpooled chain (ha_dedup_reduce_scaled): acc = +0; acc = fl(acc + fl(scale * grads[i])) over every occurrence."""
    grads = _f32(grads)
    scale = np.float32(scale)
    red = np.zeros((n_unique, grads.shape[1]), dtype=np.float32)
    with np.errstate(all="ignore"):
        for i, u in enumerate(np.asarray(inverse).reshape(-1)):
            red[u] = (red[u] + (scale * grads[i]).astype(np.float32)).astype(np.float32)
    return red


def which_of(n, bag=None, offsets=None):
    return np.arange(n) // int(bag) if offsets is None else bag_model.bag_of(offsets, n)

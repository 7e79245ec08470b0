"""Numpy restatement of the fused FM-pooled sparse SGD apply (include/herald_amd.h, ha_sgd_apply_fm_bags): the backward of an
FM-pooled lookup whose rows nothing consumed, applied per unique key.  Test infrastructure only: nothing under herald_amd/
imports it.

Per key k < rows with occurrences i0 < i1 < ..., e = table[k] BEFORE the call (the same for every occurrence) and acc = e:
    a   = fl(g_fm[b] * S[b]);   with g_sum: a = fl(g_sum[b] + a)
    g   = fl(a - fl(g_fm[b] * e))
    acc = fl(acc - fl(lr * g))
with b the bag of the occurrence; then table[k] = acc.  Everything float32, every operation rounded on its own."""
import numpy as np

import bag_model
import fm_model

F32 = np.float32


def expand(g_sum, n, nbags, bag=None, offsets=None):
    """g_sum [B, width] -> [n, width]: every occurrence a copy of its bag's row (None stays None)."""
    if g_sum is None:
        return None
    return np.asarray(g_sum, dtype=F32)[fm_model.which_bag(n, nbags, bag, offsets)]


def fm_pooled_sgd(table, ids, g_sum, g_fm, S, lr, offsets=None):
    """-> the table after ha_sgd_apply_fm_bags.  ids [B, F] (fixed bags) or [n] with offsets [B + 1] (ragged bags)."""
    before = np.asarray(table, dtype=F32)
    out = np.array(before, dtype=F32, copy=True)
    g_fm, S = np.asarray(g_fm, dtype=F32), np.asarray(S, dtype=F32)
    g_sum = None if g_sum is None else np.asarray(g_sum, dtype=F32)
    flat = bag_model.ids_to_rows(ids)
    bag = None if offsets is not None else np.asarray(ids).shape[1]
    which = fm_model.which_bag(flat.size, S.shape[0], bag, offsets)
    lr = F32(lr)
    for i in range(flat.size):
        k = flat[i]
        if not 0 <= k < before.shape[0]:
            continue
        b = which[i]
        e = before[k]                       # the row as it was before the call, whatever was applied to it since
        a = (g_fm[b] * S[b]).astype(F32)
        if g_sum is not None:
            a = (g_sum[b] + a).astype(F32)
        g = (a - (g_fm[b] * e).astype(F32)).astype(F32)
        out[k] = (out[k] - (lr * g).astype(F32)).astype(F32)
    return out

"""Numpy restatement of the FM-pooled lookup and its per-occurrence gradient (include/herald_amd.h, ha_gather_fm_* /
ha_fm_grad_rows).  Test infrastructure only: nothing under herald_amd/ imports it.

Everything is float32 and every operation is rounded on its own, in the kernels' order:
    S  = ((0 + r_0) + r_1) + ...                  the chain of bag_model.bag_sum
    Q  = ((0 + fl(r_0*r_0)) + fl(r_1*r_1)) + ...
    fm = fl(0.5 * fl(fl(S*S) - Q))
    grad[i] = fl(fl(g_rows[i] + fl(g_fm[b] * S[b])) - fl(g_fm[b] * e[i]))        (g_rows None: fl(fl(g_fm*S) - fl(g_fm*e)))
numpy's float32 arithmetic rounds every elementwise operation once and never contracts, which is what is asked."""
import numpy as np

import bag_model

F32 = np.float32


def fm_lookup(table, ids, offsets=None):
    """-> (rows [n, width], covered [n] bool, S [B, width], fm [B, width]).  rows[i] is the row of occurrence i (zeros for an
    id >= rows); covered[i] says whether occurrence i lies in a bag (always, for fixed bags): the kernel writes only those."""
    table = np.asarray(table, dtype=F32)
    nrows, width = table.shape
    flat = bag_model.ids_to_rows(ids)
    n = flat.size
    lo, hi = bag_model.bag_bounds(np.asarray(ids).shape if offsets is None else n, offsets)
    ok = (flat >= 0) & (flat < nrows)
    rows = np.where(ok[:, None], table[np.where(ok, flat, 0)], F32(0)).astype(F32) if nrows else np.zeros((n, width), F32)
    covered = np.zeros(n, dtype=bool)
    nb = lo.size
    S = np.zeros((nb, width), dtype=F32)
    Q = np.zeros((nb, width), dtype=F32)
    if offsets is None and nb:      # fixed bags: the same chains per element, all bags at once
        covered[:] = True
        r3 = rows.reshape(nb, -1, width)
        for j in range(r3.shape[1]):
            S = (S + r3[:, j]).astype(F32)
            Q = (Q + (r3[:, j] * r3[:, j]).astype(F32)).astype(F32)
    else:
        for b in range(nb):
            for j in range(int(lo[b]), int(hi[b])):
                covered[j] = True
                S[b] = (S[b] + rows[j]).astype(F32)
                Q[b] = (Q[b] + (rows[j] * rows[j]).astype(F32)).astype(F32)
    fm = (F32(0.5) * ((S * S).astype(F32) - Q).astype(F32)).astype(F32)
    return rows, covered, S, fm


def which_bag(n, nbags, bag=None, offsets=None):
    """The bag of every occurrence: i // bag, or ha_bag_of's bisection over the offsets."""
    if offsets is None:
        return np.arange(n) // int(bag)
    return bag_model.bag_of(offsets, n).astype(np.int64)


def fm_grad_rows(g_rows, emb_rows, S, g_fm, bag=None, offsets=None):
    """The per-occurrence gradient [n, width], in the kernel's fixed order of the three adjoints."""
    S, g_fm = np.asarray(S, dtype=F32), np.asarray(g_fm, dtype=F32)
    width = S.shape[1]
    e = np.asarray(emb_rows, dtype=F32).reshape(-1, width)
    b = which_bag(e.shape[0], S.shape[0], bag, offsets)
    a = (g_fm[b] * S[b]).astype(F32)
    if g_rows is not None:
        a = (np.asarray(g_rows, dtype=F32).reshape(-1, width) + a).astype(F32)
    return (a - (g_fm[b] * e).astype(F32)).astype(F32)


def sgd_serial(table, ids, grads, lr):
    """cpu_SGDOptimizerSparseUpdate: table[key_i] -= fl(lr * grads[i]) for i ascending; an id >= rows is ignored."""
    table = np.array(table, dtype=F32, copy=True)
    flat = bag_model.ids_to_rows(ids)
    grads = np.asarray(grads, dtype=F32).reshape(flat.size, -1)
    lr = F32(lr)
    for i in range(flat.size):
        r = flat[i]
        if 0 <= r < table.shape[0]:
            table[r] = (table[r] - (lr * grads[i]).astype(F32)).astype(F32)
    return table


def ps_push(table, ids, grads, lr):
    """What ParameterServerCommunicateOp does with unpooled slices: values scaled by -lr (one rounding), reduced per unique key
    in occurrence order from +0 -- (0 + v_i0) + v_i1 + ... -- and the sum added to the row."""
    table = np.array(table, dtype=F32, copy=True)
    flat = bag_model.ids_to_rows(ids)
    vals = (F32(-lr) * np.asarray(grads, dtype=F32).reshape(flat.size, -1)).astype(F32)
    acc = {}
    for i in range(flat.size):
        r = int(flat[i])
        if 0 <= r < table.shape[0]:
            acc[r] = (acc.get(r, np.zeros(vals.shape[1], F32)) + vals[i]).astype(F32)
    for r, v in acc.items():
        table[r] = (table[r] + v).astype(F32)
    return table

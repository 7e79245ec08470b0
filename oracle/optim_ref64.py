"""float64 yardstick of the sparse optimizers (AddL2RegularizationSparse, AdaGrad / Adam / AdamW / Lamb /
Momentum OptimizerSparseUpdate): one plain evaluation of the mathematics per operator.

TEST INFRASTRUCTURE ONLY, like oracle/cpu.py; no GPU, no torch.  The formulas are those of the reference's
src/ops/OptimizersSparse.cu (:3-18 sparse L2, :101-155 Momentum and Nesterov, :331-349 AdaGrad, :391-416 Adam,
:457-484 AdamW, :539-579 Lamb), written from the mathematics and not from the float32 expression order.

Every function takes float32 arrays, changes none of them, and returns (sel, idx, out):

  sel   positions of `ids` whose id names a row of the table (an id beyond the table is skipped);
  idx   the rows they name (int64), idx[k] = row of position sel[k];
  out   {array name: (X, S)}: X the new float64 values and S the per-element SCALE, the sum of the absolute
        values of the terms that are added to give that element, carried through the moments:
            S_m = |beta1 m| + |(1 - beta1) g|         S_v = |beta2 v| + |(1 - beta2) g^2|
        and for the parameter the update term evaluated with S_m in place of the new m.  Where beta1 m and
        (1 - beta1) g cancel, the new m is small but carries the rounding of its two large terms into the
        parameter; a scale built from the new m alone would not cover that.  A float32 evaluation differs from
        X by a few units of 2^-24 S per element (tests/test_optim_oracle.py measures how many).
        The deduplicated operators return the named rows only, shape (len(sel), width); Momentum, whose second
        phase is dense, returns whole tables.

Scalars enter as the float32 value the C ABI receives, so 1 - beta is the same number on both sides.

`mutant` selects a deliberately WRONG variant, for the test that shows the yardstick has teeth
(tests/test_optim_oracle.py, MUTANTS); None is the operator.
"""
import numpy as np

UNIT = 2.0 ** -24     # half an ulp of a float32 in [1, 2): the unit every difference is stated in


def scalar(x):
    """The number a `float` argument of the C ABI holds."""
    return np.float64(np.float32(x))


def named_rows(ids, rows):
    """(sel, idx) of the ids that name a row, by the id rule of include/herald_amd.h ("Which ids name a row"): the key
    of a float32 id f is trunc(f) for -1 < f < 4294967295 and 0xFFFFFFFE for every other f (NaN, f <= -1, beyond 32
    bits, the infinities); a key >= rows is skipped.  The integer cast runs on in-range values only."""
    f = np.asarray(ids, dtype=np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        live = (f > np.float32(-1.0)) & (f < np.float32(4294967296.0))
    key = np.full(f.size, 0xFFFFFFFE, dtype=np.int64)
    key[live] = np.trunc(f[live]).astype(np.int64)
    sel = np.flatnonzero(key < rows)
    return sel, key[sel]


def _gather(ids, grads, *tables):
    rows = tables[0].shape[0]
    sel, idx = named_rows(ids, rows)
    g = np.asarray(grads, dtype=np.float32).reshape(np.asarray(ids).size, tables[0].shape[1])[sel].astype(np.float64)
    return (sel, idx, g) + tuple(t[idx].astype(np.float64) for t in tables)


def units(x, x64, s):
    """Largest |x - x64| in units of 2^-24 S.  An element whose scale is 0 must be exact."""
    d = np.abs(np.asarray(x, dtype=np.float64) - x64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(d == 0, 0.0, d / (UNIT * s))
    return float(q.max()) if q.size else 0.0


def l2(param, ids, grads, l2reg, mutant=None):
    """grad[i, :] += l2reg * param[ids[i], :]"""
    sel, idx, g, p = _gather(ids, grads, param)
    term = scalar(l2reg) * p
    out = g - term if mutant == "sign_flipped" else g + term
    return sel, idx, {"grad": (out, np.abs(g) + np.abs(term))}


def adagrad(param, acc, ids, grads, lr, eps, mutant=None):
    """acc += g^2;  param -= lr g / (sqrt(acc) + eps), with the NEW acc"""
    sel, idx, g, p, a = _gather(ids, grads, param, acc)
    lr, eps = scalar(lr), scalar(eps)
    new = a + g * g
    root = a if mutant == "old_accumulator" else new
    if mutant == "eps_inside_sqrt":
        den = np.sqrt(root + eps)
    elif mutant == "eps_dropped":
        den = np.sqrt(root)
    else:
        den = np.sqrt(root) + eps
    step = lr * g / den
    return sel, idx, {"param": (p - step, np.abs(p) + np.abs(step)),
                      "acc": (new, np.abs(a) + g * g)}


def _moments(g, m, v, beta1, beta2, beta1t, beta2t, eps, mutant):
    """New moments, their scales, and the direction m^ / (sqrt(v^) + eps) with the scale of its numerator."""
    b1, b2, b1t, b2t, eps = scalar(beta1), scalar(beta2), scalar(beta1t), scalar(beta2t), scalar(eps)
    nm = b1 * m + (1.0 - b1) * g
    sm = np.abs(b1 * m) + np.abs((1.0 - b1) * g)
    nv = b2 * v + (1.0 - b2) * g * g
    sv = np.abs(b2 * v) + np.abs((1.0 - b2) * g * g)
    c1 = {"beta1_for_beta1t": 1.0 - b1, "bias1_dropped": 1.0}.get(mutant, 1.0 - b1t)
    c2 = {"beta2_for_beta2t": 1.0 - b2, "bias2_dropped": 1.0}.get(mutant, 1.0 - b2t)
    vh = nv / c2
    if mutant == "eps_inside_sqrt":
        den = np.sqrt(vh + eps)
    elif mutant == "eps_dropped":
        den = np.sqrt(vh)
    else:
        den = np.sqrt(vh) + eps
    return nm, sm, nv, sv, (nm / c1) / den, (sm / c1) / den


def adam(param, m, v, ids, grads, lr, beta1, beta2, beta1t, beta2t, eps, mutant=None):
    """m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  param -= lr m^ / (sqrt(v^) + eps)"""
    sel, idx, g, p, m0, v0 = _gather(ids, grads, param, m, v)
    nm, sm, nv, sv, upd, supd = _moments(g, m0, v0, beta1, beta2, beta1t, beta2t, eps, mutant)
    lr = scalar(lr)
    return sel, idx, {"param": (p - lr * upd, np.abs(p) + lr * supd), "m": (nm, sm), "v": (nv, sv)}


def adamw(param, m, v, ids, grads, lr, beta1, beta2, beta1t, beta2t, eps, weight_decay, mutant=None):
    """Adam's moments;  param -= lr (m^ / (sqrt(v^) + eps) + weight_decay param), the OLD param decayed"""
    sel, idx, g, p, m0, v0 = _gather(ids, grads, param, m, v)
    nm, sm, nv, sv, upd, supd = _moments(g, m0, v0, beta1, beta2, beta1t, beta2t, eps, mutant)
    lr, wd = scalar(lr), scalar(weight_decay)
    if mutant == "weight_decay_dropped":
        new = p - lr * upd
    elif mutant == "decays_updated_param":
        new = (p - lr * upd) * (1.0 - lr * wd)
    else:
        new = p - lr * (upd + wd * p)
    return sel, idx, {"param": (new, np.abs(p) + lr * supd + np.abs(lr * wd * p)), "m": (nm, sm), "v": (nv, sv)}


def lamb(param, m, v, ids, grads, lr, beta1, beta2, beta1t, beta2t, eps, weight_decay, mutant=None):
    """Adam's moments and direction u;  ratio = |param[idx]|_2 / |u|_2, both over the indexed, in-range rows;
    param -= lr ratio (u + weight_decay param).  A zero |u|_2 divides by zero, as the reference does (:578)."""
    sel, idx, g, p, m0, v0 = _gather(ids, grads, param, m, v)
    nm, sm, nv, sv, upd, supd = _moments(g, m0, v0, beta1, beta2, beta1t, beta2t, eps, mutant)
    lr, wd = scalar(lr), scalar(weight_decay)
    if mutant == "weight_decay_dropped":
        wd = 0.0
    norm_p = np.sqrt(np.sum(param.astype(np.float64) ** 2 if mutant == "norms_over_whole_table" else p * p))
    norm_u = np.sqrt(np.sum(upd * upd))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = norm_p / norm_u
        if mutant == "ratio_inverted":     # = the two norms taken over each other's array
            ratio = norm_u / norm_p
        new = p - lr * ratio * (upd + wd * p)
        s = np.abs(p) + lr * ratio * supd + np.abs(lr * ratio * wd * p)
    return sel, idx, {"param": (new, s), "m": (nm, sm), "v": (nv, sv)}


def momentum(param, veloc, ids, grads, lr, momentum, nesterov, mutant=None):
    """ids may repeat.  First phase, per occurrence: velocity[id] += -lr g (Nesterov: param[id] too).  Second
    phase over the WHOLE table: plain  param += velocity; velocity *= mu;  Nesterov  velocity *= mu; param +=
    velocity.  Returns whole tables."""
    rows = param.shape[0]
    sel, idx = named_rows(ids, rows)
    g = np.asarray(grads, dtype=np.float32).reshape(np.asarray(ids).size, param.shape[1])[sel].astype(np.float64)
    lr, mu = scalar(lr), scalar(momentum)
    p, v = param.astype(np.float64), veloc.astype(np.float64)
    sp, sv = np.abs(p), np.abs(v)
    np.add.at(v, idx, -lr * g)
    np.add.at(sv, idx, np.abs(lr * g))
    if nesterov:
        np.add.at(p, idx, -lr * g)
        np.add.at(sp, idx, np.abs(lr * g))
    dense = np.ones(rows, dtype=bool)
    if mutant == "dense_phase_on_touched_rows_only":
        dense[:] = False
        dense[idx] = True
    d = dense[:, None]
    if nesterov != (mutant == "second_phases_swapped"):
        nv = np.where(d, mu * v, v)
        np_ = np.where(d, p + nv, p)
        return sel, idx, {"param": (np_, sp + mu * sv), "velocity": (nv, mu * sv)}
    np_ = np.where(d, p + v, p)
    return sel, idx, {"param": (np_, sp + sv), "velocity": (np.where(d, mu * v, v), mu * sv)}

"""The float64 yardstick of the sparse optimizers (oracle/optim_ref64.py) against the float32 restatement
(oracle/cpu.py:156-227), on the CPU.

Two statements, both about the inputs the GPU tests use (build_inputs / build_momentum below are the one input
builder of this module and of tests/test_gpu_optim_paths.py):

  * yardstick: per operator and output array, c32 = max |X32 - X64| / (2^-24 S), X32 the float32 restatement,
    X64 and the scale S from the float64 reference.  c32 is COMPUTED here, on three consecutive steps, and only
    capped at 8: a value of 10 or more would mean a cancellation that S does not carry.  The GPU tests take their
    bound (2 c32 + 2 units) from c32() of this module;
  * mutants: every deliberately wrong float64 variant of MUTANTS moves some output by more than that bound on
    these inputs -- so a kernel with that defect cannot pass, and the inputs are not too tame to tell.
"""
import functools

import numpy as np
import pytest

import special_ids
from oracle import cpu
from oracle import optim_ref64 as ref64

# eps = 1e-2 is within the range of sqrt(v^) (gradient rows are scaled over 1e-4 .. 3), so where eps sits in the
# formula matters; weight decay and l2 are large enough to show against a parameter of about 1.
HYPER = dict(lr=0.05, eps=1e-2, beta1=0.9, beta2=0.999, weight_decay=0.1, l2reg=0.3, momentum=0.9)
OPS = ("l2", "adagrad", "adam", "adamw", "lamb")
STATES = {"l2": (), "adagrad": ("acc",), "adam": ("m", "v"), "adamw": ("m", "v"), "lamb": ("m", "v")}
OUTPUTS = {"l2": ("grad",), "adagrad": ("param", "acc"), "adam": ("param", "m", "v"),
           "adamw": ("param", "m", "v"), "lamb": ("param", "m", "v"), "momentum": ("param", "velocity"),
           "nesterov": ("param", "velocity")}
BEYOND = (None, None, 2.0 ** 31, 4.0e9)       # ids beyond a table of `rows` rows: rows, rows + 1, 2^31, 4.0e9
C32_CAP = 8.0


def build_inputs(seed, rows, width, n, beyond=False, other_scale=1.0):
    """One sparse update on a (rows, width) table: dict of float32 arrays param, m, v, acc, ids, grads.
    Every table row has a scale drawn log-uniformly over 1e-4 .. 3; the gradient row of an id, and the states of
    that table row (m of either sign, v and acc as squares), are N(0,1) times that scale, so beta m and
    (1 - beta) g are of a kind and do cancel.  ids are unique and SHUFFLED (not ascending).  beyond: a tenth of
    the positions name no row (BEYOND).  other_scale multiplies the parameter rows that no id names."""
    assert rows < (1 << 24) and n <= rows
    rng = np.random.default_rng(seed)
    f = np.float32
    scale = (10.0 ** rng.uniform(-4.0, np.log10(3.0), size=rows)).astype(f)[:, None]
    param = rng.standard_normal((rows, width), dtype=f)
    m = rng.standard_normal((rows, width), dtype=f) * scale
    v = (rng.standard_normal((rows, width), dtype=f) * scale) ** 2
    acc = (rng.standard_normal((rows, width), dtype=f) * scale) ** 2
    idx = rng.permutation(rows)[:n]
    ids = idx.astype(f)
    grads = rng.standard_normal((n, width), dtype=f) * scale[idx]
    if beyond:
        far = np.array([rows, rows + 1, BEYOND[2], BEYOND[3]], dtype=f)
        where = rng.permutation(n)[:max(1, n // 10)]
        ids[where] = far[np.arange(where.size) % 4]
        grads[where] = rng.standard_normal((where.size, width), dtype=f)
    if other_scale != 1.0:
        named = np.zeros(rows, dtype=bool)
        named[ref64.named_rows(ids, rows)[1]] = True
        param[~named] *= f(other_scale)
    return dict(param=param, m=m, v=v, acc=acc, ids=ids, grads=grads)


def build_momentum(seed, rows, width, n, beyond=0):
    """Momentum is called WITHOUT deduplication: Zipf-repeated ids (a few rows take most occurrences), non-zero
    velocity.  beyond: that many positions name no row."""
    rng = np.random.default_rng(seed)
    f = np.float32
    ids = np.minimum(rng.zipf(1.5, size=n) - 1, rows - 1).astype(f)
    if beyond:
        ids[rng.permutation(n)[:beyond]] = np.array([rows, rows + 1, BEYOND[2], BEYOND[3]], dtype=f)[
            np.arange(beyond) % 4]
    return dict(param=rng.standard_normal((rows, width), dtype=f),
                velocity=rng.standard_normal((rows, width), dtype=f) * f(0.1), ids=ids,
                grads=rng.standard_normal((n, width), dtype=f))


def hyper_of(op, t):
    """Scalar arguments of `op` at step t, in the order of its C prototype after the arrays."""
    h = HYPER
    if op == "l2":
        return (h["l2reg"],)
    if op == "adagrad":
        return (h["lr"], h["eps"])
    if op in ("momentum", "nesterov"):
        return (h["lr"], h["momentum"], op == "nesterov")
    sc = (h["lr"], h["beta1"], h["beta2"], h["beta1"] ** t, h["beta2"] ** t, h["eps"])
    return sc if op == "adam" else sc + (h["weight_decay"],)


def step64(op, a, ids, grads, t, mutant=None, hyper=None):
    """One float64 step of `op` from the float32 arrays in `a`: (sel, idx, {name: (X64, S)})."""
    sc = hyper_of(op, t) if hyper is None else hyper
    if op == "l2":
        return ref64.l2(a["param"], ids, grads, *sc, mutant=mutant)
    if op == "adagrad":
        return ref64.adagrad(a["param"], a["acc"], ids, grads, *sc, mutant=mutant)
    if op in ("momentum", "nesterov"):
        return ref64.momentum(a["param"], a["velocity"], ids, grads, *sc, mutant=mutant)
    fn = {"adam": ref64.adam, "adamw": ref64.adamw, "lamb": ref64.lamb}[op]
    return fn(a["param"], a["m"], a["v"], ids, grads, *sc, mutant=mutant)


def step32(op, a, ids, grads, t, hyper=None):
    """The same step by the float32 restatement of oracle/cpu.py, ids beyond the table skipped: {name: whole
    new float32 array} (for l2 the whole gradient array; a skipped position keeps its row)."""
    sc = hyper_of(op, t) if hyper is None else hyper
    f = np.float32
    ids = np.asarray(ids, dtype=f).reshape(-1)
    grads = np.asarray(grads, dtype=f).reshape(ids.size, a["param"].shape[1])
    key = special_ids.rows_of(ids)
    sel = np.flatnonzero(key < a["param"].shape[0])
    idx = key[sel]
    new = {k: a[k].copy() for k in ("param",) + STATES.get(op, ("velocity",))}
    with np.errstate(divide="ignore", invalid="ignore"):       # Lamb divides by norm(update), which may be 0
        if op == "l2":
            out = grads.copy()
            out[sel] = cpu.l2_sparse(a["param"], idx, grads[sel], sc[0])
            return {"grad": out}
        if op == "adagrad":
            cpu.adagrad_sparse(new["param"], new["acc"], idx, grads[sel], *sc)
        elif op in ("momentum", "nesterov"):
            cpu.momentum_sparse(new["param"], new["velocity"], idx, grads[sel], *sc)
        elif op == "lamb":
            cpu.lamb_sparse(new["param"], new["m"], new["v"], idx, grads[sel], sc[0], sc[1], sc[2], f(sc[3]),
                            f(sc[4]), sc[5], sc[6])
        else:
            cpu.adam_sparse(new["param"], new["m"], new["v"], idx, grads[sel], sc[0], sc[1], sc[2], f(sc[3]),
                            f(sc[4]), sc[5], sc[6] if op == "adamw" else None)
    return new


def named_part(op, name, x, sel, idx):
    """The part of a whole float32 output array that the float64 reference returns."""
    if op in ("momentum", "nesterov"):
        return x
    return x[sel] if name == "grad" else x[idx]


def canonical(op):
    """The draw c32 and the mutants are judged on.  Lamb: the rows no id names are 100 times larger, so norms
    taken over the wrong rows are far off."""
    if op in ("momentum", "nesterov"):
        return build_momentum(11, 300, 64, 200, beyond=3)
    return build_inputs(7, 3000, 64, 2000, beyond=True, other_scale=100.0 if op == "lamb" else 1.0)


@functools.lru_cache(maxsize=None)
def c32(op):
    """{output name: c32} of `op`: the float32 restatement against float64 over steps t = 1, 2, 3 on canonical(op),
    each step judged from the float32 state the step before left (nothing compounds)."""
    a = canonical(op)
    ids, grads = a["ids"], a["grads"]
    worst = dict.fromkeys(OUTPUTS[op], 0.0)
    for t in (1, 2, 3):
        sel, idx, out = step64(op, a, ids, grads, t)
        new = step32(op, a, ids, grads, t)
        for name, (x64, s) in out.items():
            worst[name] = max(worst[name], ref64.units(named_part(op, name, new[name], sel, idx), x64, s))
        if op != "l2":
            a = dict(a, **new)
    return worst


def bound_units(op, name):
    """What a kernel may differ from float64 by, in units of 2^-24 S: numpy's square root and division are
    correctly rounded, the device's may each be one unit off and there are two of them in the chain."""
    return 2.0 * c32(op)[name] + 2.0


@pytest.mark.parametrize("op", OPS + ("momentum", "nesterov"))
def test_float32_restatement_is_within_a_few_units_of_float64(op):
    got = c32(op)
    print("c32 %-9s %s" % (op, "  ".join("%s %.2f" % kv for kv in got.items())))
    for name, value in got.items():
        assert 0.0 < value <= C32_CAP, (op, name, value)


MUTANTS = [
    ("l2", "sign_flipped"),
    ("adagrad", "old_accumulator"), ("adagrad", "eps_inside_sqrt"), ("adagrad", "eps_dropped"),
    ("adam", "beta1_for_beta1t"), ("adam", "beta2_for_beta2t"), ("adam", "bias1_dropped"),
    ("adam", "bias2_dropped"), ("adam", "eps_inside_sqrt"), ("adam", "eps_dropped"),
    ("adamw", "beta1_for_beta1t"), ("adamw", "beta2_for_beta2t"), ("adamw", "bias1_dropped"),
    ("adamw", "bias2_dropped"), ("adamw", "eps_inside_sqrt"), ("adamw", "eps_dropped"),
    ("adamw", "decays_updated_param"), ("adamw", "weight_decay_dropped"),
    ("lamb", "beta1_for_beta1t"), ("lamb", "beta2_for_beta2t"), ("lamb", "eps_inside_sqrt"),
    ("lamb", "eps_dropped"), ("lamb", "weight_decay_dropped"), ("lamb", "ratio_inverted"),
    ("lamb", "norms_over_whole_table"),
    ("momentum", "dense_phase_on_touched_rows_only"), ("momentum", "second_phases_swapped"),
    ("nesterov", "dense_phase_on_touched_rows_only"), ("nesterov", "second_phases_swapped"),
]


def mutant_excess(op, mutant, hyper=None):
    """{output name: (units the mutant is off by, the GPU bound)} at t = 3 on canonical(op)."""
    a = canonical(op)
    _, _, good = step64(op, a, a["ids"], a["grads"], 3, hyper=hyper)
    _, _, bad = step64(op, a, a["ids"], a["grads"], 3, mutant=mutant, hyper=hyper)
    return {name: (ref64.units(bad[name][0], x64, s), bound_units(op, name)) for name, (x64, s) in good.items()}


@pytest.mark.parametrize("op,mutant", MUTANTS)
def test_every_mutant_exceeds_the_gpu_bound(op, mutant):
    """t = 3, where beta^t != beta.  The output that shows a mutant is the parameter (the gradient for l2); a
    mutant of the moments' use leaves m and v themselves right."""
    got = mutant_excess(op, mutant)
    print("mutant %-9s %-34s %s" % (op, mutant, "  ".join("%s %.3g (bound %.1f)" % ((k,) + v) for k, v in got.items())))
    shown = "grad" if op == "l2" else "param"
    off, bound = got[shown]
    assert off > 100.0 * bound, (op, mutant, got)     # not by a hair: two orders above the bound


def test_out_of_range_ids_are_skipped_by_both_oracles():
    a = build_inputs(3, 50, 5, 20, beyond=True)
    sel, idx = ref64.named_rows(a["ids"], 50)
    assert sel.size == 18 and np.all(idx < 50) and np.unique(idx).size == idx.size
    assert set(a["ids"][np.setdiff1d(np.arange(20), sel)]) <= {50.0, 51.0, 2.0 ** 31, np.float32(4.0e9)}
    new = step32("adam", a, a["ids"], a["grads"], 1)
    rest = np.setdiff1d(np.arange(50), idx)
    for name in ("param", "m", "v"):
        np.testing.assert_array_equal(new[name][rest], a[name][rest])
        assert np.all(new[name][idx] != a[name][idx])

"""AdaGrad, Adam, AdamW and Momentum / Nesterov steps straight from the POOLED gradient of a sum-pooled lookup
(ha_sparse_opt_fused_bags_*, ha_momentum_sparse_update_bags_*; the BAGS instantiations of scatter_dev.h / scatter.hip).

Every assertion is on bits.  A fused result is compared, in param, state1 and state2, with
  (a) ops.sparse_opt_fused on the gradient expanded on the host (existing code, held to float64 by
      tests/test_gpu_optim_paths.py), and
  (b) the float32 restatement: oracle.cpu.dedup_reduce on the expanded gradient, then step32 of tests/test_optim_oracle.py
-- whole arrays, so the rows no in-range id names are compared too (the restatement leaves them alone).  Inputs come from
build_inputs / HYPER of tests/test_optim_oracle.py; beta^t = beta^3, so that the step is not the first.  Momentum is compared,
whole tables, with MomentumOptimizerSparseUpdate on the expanded gradient.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from herald_amd import hetu_ops, ops
from oracle import cpu
from test_gpu_optim_paths import _LENGTHS
from test_gpu_parity import _runs_batch
from test_optim_oracle import HYPER, build_inputs, step32

pytestmark = pytest.mark.gpu

KINDS = ["adagrad", "adam", "adamw"]
HYPER3 = dict(lr=HYPER["lr"], eps=HYPER["eps"], beta1=HYPER["beta1"], beta2=HYPER["beta2"], beta1t=HYPER["beta1"] ** 3,
              beta2t=HYPER["beta2"] ** 3, weight_decay=HYPER["weight_decay"])


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _same_bits(got, want, what):
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=what)


def _bag_of(n, F=None, offsets=None):
    if offsets is None:
        return np.arange(n) // F
    return np.searchsorted(offsets, np.arange(n), side="right") - 1


# ---- id batches (built once per shape, never written) ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _position_ids(F):
    """One run of every length class -- 2, 3 (short), 4 .. 47 (medium), 48 .. 1000 (cooperative) and 1,100 (beyond the 1,024
    positions a workgroup scans and the 512 whose occurrence indices it keeps in LDS) -- between 3,000 singles, 9 occurrences
    of ids beyond the table, padded with unused single keys to a multiple of F and shuffled: float32 [n], n < 36,864."""
    rows = 4000
    rng = np.random.default_rng(100 + F)
    ids = np.concatenate([_runs_batch(rng, _LENGTHS + [1100], 3000, rows),
                          np.array([rows, rows, rows + 1, 2.0 ** 31, 4.0e9] + [rows + 7] * 4, dtype=np.float32)])
    pad = (-ids.size) % F
    unused = np.setdiff1d(np.arange(rows), ids[ids < rows].astype(np.int64))
    ids = np.concatenate([ids, rng.choice(unused, size=pad, replace=False).astype(np.float32)])
    rng.shuffle(ids)
    assert ids.size % F == 0 and ids.size < 36864
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def _ragged(seed, n_runs_key=300):
    """The ids of _position_ids(1) with every occurrence of the 300-run's key moved into ONE contiguous block, and offsets
    with empty bags at the front, in the middle and at the end, one bag that is exactly that block (the same gradient row
    summed 300 times) and one bag of a single id."""
    ids = _position_ids(1)
    rng = np.random.default_rng(seed)
    keys, counts = np.unique(ids, return_counts=True)
    key = keys[counts == n_runs_key][0]
    rest = ids[ids != key]
    p = int(rng.integers(100, rest.size - 100))
    ids = np.concatenate([rest[:p], np.full(n_runs_key, key, dtype=np.float32), rest[p:]])
    n = ids.size
    cuts = set(int(c) for c in rng.choice(np.arange(1, n), size=n // 20, replace=False))
    cuts = {c for c in cuts if not p < c < p + n_runs_key} | {p, p + n_runs_key, p + n_runs_key + 1}
    cuts = sorted(cuts)
    mid = cuts[len(cuts) // 2]
    offsets = np.array([0, 0] + cuts[:len(cuts) // 2] + [mid, mid] + cuts[len(cuts) // 2 + 1:] + [n, n], dtype=np.int64)
    assert np.all(np.diff(offsets) >= 0) and offsets[0] == 0 and offsets[-1] == n
    sizes = np.diff(offsets)
    assert sizes[0] == 0 and sizes[-1] == 0 and (sizes[1:-1] == 0).any() and (sizes == 1).any() and (sizes == n_runs_key).any()
    ids.setflags(write=False)
    offsets.setflags(write=False)
    return ids, offsets


@functools.lru_cache(maxsize=None)
def _listed_ids():
    """n = 40,014 = 26 x 1,539 > 36,864: runs of 5,000, 2,500, 300, 48 and 5 among singles over 50,000 rows, three ids
    beyond the table."""
    rows = 50000
    rng = np.random.default_rng(4001)
    lengths = [5000, 2500, 300, 48, 5]
    ids = np.concatenate([_runs_batch(rng, lengths, 40014 - sum(lengths) - 3, rows),
                          np.array([rows, rows + 1, rows], dtype=np.float32)])
    rng.shuffle(ids)
    assert ids.size == 40014 == 26 * 1539
    ids.setflags(write=False)
    return ids


# ---- one fused case ---------------------------------------------------------------------------------------------------
def _inputs(kind, seed, rows, width, nbags):
    a = build_inputs(seed, rows, width, 1)
    rng = np.random.default_rng(seed + 1)
    names = ("param", "acc", "v") if kind == "adagrad" else ("param", "m", "v")
    return {k: a[k] for k in names}, rng.standard_normal((nbags, width), dtype=np.float32)


def _upload(a, dev):
    return {k: torch.from_numpy(v.copy()).to(dev) for k, v in a.items()}


def _host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _bags_call(kind, d, d_ids, d_g, d_off=None):
    s1 = d["acc"] if kind == "adagrad" else d["m"]
    ops.sparse_opt_fused_bags(kind, d["param"], d_ids, d_g, s1, d["v"], offsets=d_off, **HYPER3)     # (AdaGrad: v is handed over too)


def _fused_case(dev, kind, width, ids, rows, seed, F=None, offsets=None, restate=True):
    """The bag call on ids (flat float32; fixed bags of F, or ragged by offsets) against (a) and (b).  Returns the arrays the
    bag call left, for the cases that compare twins with them."""
    n = ids.size
    nbags = n // F if offsets is None else offsets.size - 1
    a, g = _inputs(kind, seed, rows, width, nbags)
    expanded = g[_bag_of(n, F, offsets)]
    d_ids = torch.from_numpy(ids.copy()).to(dev)
    d_g = torch.from_numpy(g.copy()).to(dev)
    d_off = torch.from_numpy(offsets.copy()).to(dev) if offsets is not None else None
    d = _upload(a, dev)
    _bags_call(kind, d, d_ids.reshape(-1, F) if offsets is None else d_ids, d_g, d_off)
    torch.cuda.synchronize()
    got = _host(d)
    _same_bits(d_ids.cpu().numpy(), ids, "ids")
    _same_bits(d_g.cpu().numpy(), g, "bag_grads")
    # (a) the existing fused call on the expanded gradient
    e = _upload(a, dev)
    ops.sparse_opt_fused(kind, e["param"], d_ids, torch.from_numpy(expanded).to(dev), e["acc" if kind == "adagrad" else "m"],
                         None if kind == "adagrad" else e["v"], **HYPER3)
    torch.cuda.synchronize()
    exp = _host(e)
    for name in a:
        _same_bits(got[name], exp[name], "%s %s against sparse_opt_fused on the expanded gradient" % (kind, name))
    if kind == "adagrad":
        _same_bits(got["v"], a["v"], "a state2 handed to AdaGrad")
    # (b) the float32 restatement: whole arrays, rows that no in-range id names included
    if restate:
        uniq, _, red = cpu.dedup_reduce(ids, expanded)
        want = step32(kind, a, uniq.astype(np.float32), red, 3)
        for name in want:
            _same_bits(got[name], want[name], "%s %s against dedup_reduce + step32" % (kind, name))
        named = np.zeros(rows, dtype=bool)
        named[uniq[uniq < rows].astype(np.int64)] = True
        for name in a:
            _same_bits(got[name][~named], a[name][~named], "%s %s rows that no in-range id names" % (kind, name))
    return got


# ---- by position (n <= 36,864) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [64, 66, 516])
@pytest.mark.parametrize("F", [2, 26, 27])
@pytest.mark.parametrize("kind", KINDS)
def test_fixed_bags_every_run_class_by_position(dev, kind, F, width):
    """apply_opt_bags_kernel<VEC, true>: short, medium, cooperative runs and a run of 1,100; width 66 is the scalar path, 516
    the 16-byte path with a partial last slice; F = 2 / 26 / 27 put the bag boundaries at every alignment."""
    _fused_case(dev, kind, width, _position_ids(F), 4000, 31 * width + F + len(kind), F=F)


@pytest.mark.parametrize("kind", KINDS)
def test_bags_of_one_are_the_unpooled_call(dev, kind):
    """F = 1: pooled is unpooled -- the bag call equals sparse_opt_fused on the same [n, d] gradient (what (a) is here)."""
    _fused_case(dev, kind, 64, _position_ids(1), 4000, 77 + len(kind), F=1)


@pytest.mark.parametrize("width", [64, 66])
@pytest.mark.parametrize("kind", KINDS)
def test_ragged_bags_by_position(dev, kind, width):
    """apply_opt_bags_kernel<VEC, false> (bag_of through ha_bag_of in the per-stream scratch): empty bags at the front, in the
    middle and at the end, a bag that is a whole 300-run of one key, a bag of one id."""
    ids, offsets = _ragged(5)
    _fused_case(dev, kind, width, ids, 4000, 13 * width + len(kind), offsets=offsets)


def test_int64_ids_equal_their_float32_twins(dev):
    rows, width, F = 4000, 64, 26
    ids = _position_ids(F)
    ids64 = torch.from_numpy(ids.astype(np.int64)).to(dev)
    for kind in ("adam", "adagrad"):
        # fixed bags
        got = _fused_case(dev, kind, width, ids, rows, 900, F=F, restate=False)
        a, g = _inputs(kind, 900, rows, width, ids.size // F)
        d = _upload(a, dev)
        _bags_call(kind, d, ids64.reshape(-1, F), torch.from_numpy(g).to(dev))
        for name, x in _host(d).items():
            _same_bits(x, got[name], "fixed bags, int64 ids: %s %s" % (kind, name))
    # ragged bags
    rids, offsets = _ragged(5)
    got = _fused_case(dev, "adamw", width, rids, rows, 901, offsets=offsets, restate=False)
    a, g = _inputs("adamw", 901, rows, width, offsets.size - 1)
    d = _upload(a, dev)
    _bags_call("adamw", d, torch.from_numpy(rids.astype(np.int64)).to(dev), torch.from_numpy(g).to(dev),
               torch.from_numpy(offsets.copy()).to(dev))
    for name, x in _host(d).items():
        _same_bits(x, got[name], "ragged bags, int64 ids: adamw %s" % name)
    # the unpooled call
    a, g = _inputs("adam", 902, rows, width, ids.size)
    d32, d64 = _upload(a, dev), _upload(a, dev)
    d_g = torch.from_numpy(g).to(dev)
    ops.sparse_opt_fused("adam", d32["param"], torch.from_numpy(ids.copy()).to(dev), d_g, d32["m"], d32["v"], **HYPER3)
    ops.sparse_opt_fused("adam", d64["param"], ids64, d_g, d64["m"], d64["v"], **HYPER3)
    h32, h64 = _host(d32), _host(d64)
    assert not np.array_equal(_bits(h32["param"]), _bits(a["param"]))
    for name in a:
        _same_bits(h64[name], h32[name], "sparse_opt_fused, int64 ids: %s" % name)


@pytest.mark.parametrize("kind", KINDS)
def test_bag_grads_that_are_not_16_byte_aligned(dev, kind):
    """width % 4 == 0 but bag_grads starts 4 bytes into its buffer: the scalar path, the same bits."""
    rows, width, F = 4000, 64, 26
    ids = _position_ids(F)
    got = _fused_case(dev, kind, width, ids, rows, 55, F=F, restate=False)
    a, g = _inputs(kind, 55, rows, width, ids.size // F)
    buf = torch.full((g.size + 2,), -12345.625, dtype=torch.float32, device=dev)
    buf[1:1 + g.size] = torch.from_numpy(g.reshape(-1)).to(dev)
    view = buf[1:1 + g.size].view(*g.shape)
    assert view.data_ptr() % 16 == 4
    d = _upload(a, dev)
    _bags_call(kind, d, torch.from_numpy(ids.copy()).to(dev).reshape(-1, F), view)
    for name, x in _host(d).items():
        _same_bits(x, got[name], "%s %s from a misaligned bag_grads" % (kind, name))
    _same_bits(buf.cpu().numpy()[1:-1], g.reshape(-1), "bag_grads")
    assert buf[0].item() == -12345.625 and buf[-1].item() == -12345.625


# ---- by unique key (n > 36,864, finished plan) ----------------------------------------------------------------------
@pytest.mark.parametrize("width", [64, 66])
@pytest.mark.parametrize("kind", KINDS)
def test_fixed_bags_by_unique_key_listed(dev, kind, width):
    """apply_listed_kernel<kModeOpt, VEC, true>: the keys role maps the occurrence indices of short and medium runs, the
    listed role those coop_slices loads; a run of 5,000 and runs of 2,500, 300, 48 and 5."""
    _fused_case(dev, kind, width, _listed_ids(), 50000, 7 * width + len(kind), F=26)


def test_ragged_bags_by_unique_key_listed(dev):
    ids = _listed_ids()
    rng = np.random.default_rng(8)
    cuts = np.sort(rng.choice(np.arange(1, ids.size), size=1500, replace=False))
    offsets = np.concatenate([[0, 0], cuts[:700], cuts[699:], [ids.size, ids.size]]).astype(np.int64)
    _fused_case(dev, "adam", 64, ids, 50000, 123, offsets=offsets)


def test_fixed_bags_by_unique_key_unlisted(dev):
    """n = 1,048,606 = 26 x 40,331 > 1,048,576: apply_unique_kernel + apply_long_kernel (the long keys are listed by the first
    for the second).  Width 4, Adam; runs of 5,000, 300 and 48 among ids drawn from 200,000 rows."""
    rows, n = 200000, 1048606
    rng = np.random.default_rng(1048606)
    lengths = [5000, 300, 48]
    keys = rng.choice(rows, size=3, replace=False)
    ids = np.concatenate([np.full(L, k) for L, k in zip(lengths, keys)] + [rng.integers(0, rows, size=n - sum(lengths))])
    rng.shuffle(ids)
    assert ids.size == n == 26 * 40331
    _fused_case(dev, "adam", 4, ids.astype(np.float32), rows, 1, F=26)


# ---- Momentum / Nesterov -------------------------------------------------------------------------------------------
def _momentum_case(dev, nesterov, width, ids, rows, seed, F=None, offsets=None):
    n = ids.size
    nbags = n // F if offsets is None else offsets.size - 1
    rng = np.random.default_rng(seed)
    param = rng.standard_normal((rows, width), dtype=np.float32)
    veloc = rng.standard_normal((rows, width), dtype=np.float32) * np.float32(0.1)
    g = rng.standard_normal((nbags, width), dtype=np.float32)
    expanded = g[_bag_of(n, F, offsets)]
    lr, mom = HYPER["lr"], HYPER["momentum"]
    d_ids = torch.from_numpy(ids.copy()).to(dev)
    p1, v1 = torch.from_numpy(param.copy()).to(dev), torch.from_numpy(veloc.copy()).to(dev)
    d_g = torch.from_numpy(g.copy()).to(dev)
    ops.momentum_sparse_update_bags(p1, d_ids.reshape(-1, F) if offsets is None else d_ids, d_g, v1, lr, mom, nesterov,
                                    offsets=torch.from_numpy(offsets.copy()).to(dev) if offsets is not None else None)
    p2, v2 = torch.from_numpy(param.copy()).to(dev), torch.from_numpy(veloc.copy()).to(dev)
    ops.dl_call("MomentumOptimizerSparseUpdate", [p2, d_ids, torch.from_numpy(expanded).to(dev), v2],
                scalars=[ctypes.c_float(lr), ctypes.c_float(mom), ctypes.c_bool(nesterov)])
    torch.cuda.synchronize()
    _same_bits(p1.cpu().numpy(), p2.cpu().numpy(), "param")
    _same_bits(v1.cpu().numpy(), v2.cpu().numpy(), "velocity")
    assert not np.array_equal(_bits(p1.cpu().numpy()), _bits(param))
    _same_bits(d_ids.cpu().numpy(), ids, "ids")
    _same_bits(d_g.cpu().numpy(), g, "bag_grads")
    return p1.cpu().numpy(), v1.cpu().numpy()


@pytest.mark.parametrize("width", [64, 7])
@pytest.mark.parametrize("bags", [2, 26, "ragged"])
@pytest.mark.parametrize("nesterov", [False, True])
def test_momentum_from_the_pooled_gradient(dev, nesterov, bags, width):
    """ha_momentum_sparse_update_bags_f32ids against MomentumOptimizerSparseUpdate on the expanded gradient, whole tables;
    once more in tolerance mode (runs of 64 or more as fixed-order trees: the same tree over the same values)."""
    if bags == "ragged":
        ids, offsets = _ragged(5)
        kw = dict(offsets=offsets)
    else:
        ids, kw = _position_ids(bags), dict(F=bags)
    exact = _momentum_case(dev, nesterov, width, ids, 4000, width + 3, **kw)
    prev = ops.set_tolerance_mode(True)
    try:
        tol = _momentum_case(dev, nesterov, width, ids, 4000, width + 3, **kw)
    finally:
        ops.set_tolerance_mode(prev)
    if width % 4 == 0:      # (the trees need 16-byte rows: width 7 stays the serial chain)
        assert not np.array_equal(_bits(tol[1]), _bits(exact[1]))


def test_momentum_int64_ids(dev):
    ids = _position_ids(26)
    want = _momentum_case(dev, True, 64, ids, 4000, 9, F=26)
    rng = np.random.default_rng(9)
    param = rng.standard_normal((4000, 64), dtype=np.float32)
    veloc = rng.standard_normal((4000, 64), dtype=np.float32) * np.float32(0.1)
    g = rng.standard_normal((ids.size // 26, 64), dtype=np.float32)
    p, v = torch.from_numpy(param).to(dev), torch.from_numpy(veloc).to(dev)
    ops.momentum_sparse_update_bags(p, torch.from_numpy(ids.astype(np.int64)).to(dev).reshape(-1, 26), torch.from_numpy(g).to(dev),
                                    v, HYPER["lr"], HYPER["momentum"], True)
    _same_bits(p.cpu().numpy(), want[0], "param")
    _same_bits(v.cpu().numpy(), want[1], "velocity")


# ---- operator layer --------------------------------------------------------------------------------------------------
def _op_call(op, param, grad, st, t, fuse):
    h = HYPER
    if op in ("momentum", "nesterov"):
        hetu_ops.momentum_update_sparse(param, grad, st[0], h["lr"], h["momentum"], op == "nesterov", fuse_bags=fuse)
    elif op == "adagrad":
        hetu_ops.adagrad_update_sparse(param, grad, st[0], h["lr"], h["eps"], fuse_bags=fuse)
    elif op == "adam":
        hetu_ops.adam_update_sparse(param, grad, st[0], st[1], h["lr"], h["beta1"], h["beta2"], h["beta1"] ** t,
                                    h["beta2"] ** t, h["eps"], fuse_bags=fuse)
    else:
        hetu_ops.adamw_update_sparse(param, grad, st[0], st[1], h["lr"], h["beta1"], h["beta2"], h["beta1"] ** t,
                                     h["beta2"] ** t, h["eps"], h["weight_decay"], fuse_bags=fuse)


@pytest.mark.parametrize("slices", ["fixed", "ragged", "unpooled"])
@pytest.mark.parametrize("op", ["momentum", "nesterov", "adagrad", "adam", "adamw"])
def test_operator_layer_three_steps(dev, op, slices):
    """hetu_ops.*_update_sparse, fuse_bags=True against fuse_bags=False (the reference's sequence: expanded_values,
    deduplicate, the reference-named symbol), three consecutive steps with advancing beta^t: bit-equal table and states after
    every step.  Pooled slices come from EmbeddingLookUpSum_Gradient; unpooled ones from EmbeddingLookUp_Gradient (unpooled
    Momentum, where fuse_bags changes nothing: against a direct call of MomentumOptimizerSparseUpdate)."""
    rows, width, F = 4000, 64, 26
    a = build_inputs(17, rows, width, 1)
    rng = np.random.default_rng(18)
    sides = []
    for fuse in (True, False):
        param = hetu_ops.EmbeddingParameter(table=torch.from_numpy(a["param"].copy()).to(dev))
        st = [torch.from_numpy(a["acc" if op == "adagrad" else "m"].copy()).to(dev), torch.from_numpy(a["v"].copy()).to(dev)]
        sides.append((fuse, param, st))
    for t in (1, 2, 3):
        if slices == "ragged":
            ids, offsets = _ragged(5)
            nrow = offsets.size - 1
        else:
            ids, offsets = _position_ids(F), None
            nrow = ids.size // F if slices == "fixed" else ids.size
        ids = np.roll(ids, 7 * t) if slices != "ragged" else ids
        g = rng.standard_normal((nrow, width), dtype=np.float32)
        for fuse, param, st in sides:
            d_ids, d_g = torch.from_numpy(ids.copy()).to(dev), torch.from_numpy(g.copy()).to(dev)
            if slices == "fixed":
                grad = hetu_ops.EmbeddingLookUpSum_Gradient((rows, width)).compute(d_g, d_ids.reshape(-1, F))
            elif slices == "ragged":
                grad = hetu_ops.EmbeddingLookUpSum_Gradient((rows, width)).compute(d_g, d_ids,
                                                                                   offsets=torch.from_numpy(offsets.copy()).to(dev))
            else:
                grad = hetu_ops.EmbeddingLookUp_Gradient((rows, width)).compute(d_g, d_ids)
            assert grad.pooled == (slices != "unpooled")
            if slices == "unpooled" and op in ("momentum", "nesterov") and not fuse:
                # (fuse_bags has no effect on unpooled momentum: the yardstick is the symbol itself, called directly)
                ops.dl_call("MomentumOptimizerSparseUpdate", [param.table, d_ids, d_g, st[0]],
                            scalars=[ctypes.c_float(HYPER["lr"]), ctypes.c_float(HYPER["momentum"]),
                                     ctypes.c_bool(op == "nesterov")])
            else:
                _op_call(op, param, grad, st, t, fuse)
            _same_bits(grad.values.cpu().numpy(), g, "the gradient's values")
        torch.cuda.synchronize()
        (_, p1, s1), (_, p0, s0) = sides
        what = "%s, %s slices, step %d: " % (op, slices, t)
        _same_bits(p1.table.cpu().numpy(), p0.table.cpu().numpy(), what + "table")
        _same_bits(s1[0].cpu().numpy(), s0[0].cpu().numpy(), what + "state 1")
        _same_bits(s1[1].cpu().numpy(), s0[1].cpu().numpy(), what + "state 2")
    assert not np.array_equal(_bits(sides[0][1].table.cpu().numpy()), _bits(a["param"]))

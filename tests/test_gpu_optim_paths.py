"""Every branch of the sparse optimizers (csrc/optim.hip, optim_dev.h, the fused kModeOpt apply of scatter.hip /
scatter_dev.h) against the float64 reference of oracle/optim_ref64.py, through the reference-named symbols.

How a result is judged -- PER CALL (`_judged_call`): the device's float32 parameter and state are read back, one
float64 step is evaluated from exactly those, the call is made, whole arrays are read back.  So steps 2 and 3 (states
the kernel itself left, beta^t != beta) are judged as sharply as step 1 and nothing compounds.

  1. rows that no in-range id names are bit-unchanged in every array; so are the ids and (but for sparse L2, whose
     output they are) the gradients;
  2. named rows equal the float32 restatement of oracle/cpu.py BIT FOR BIT.  The first run of this module on the
     MI355X found not one differing bit in 275 million elements over 1,271 calls, for any of the five operators
     (docs/EXPERIMENTS.md, "Sparse optimizers against float64"): the kernels keep the reference's expression order
     and the library is built without contraction, so equality is what is asserted.  They are also held to float64,
     |X_gpu - X64| <= (2 c32 + 2) 2^-24 S element-wise with c32 and S from tests/test_optim_oracle.py -- which,
     the bits being the restatement's, says that the restatement is as close to float64 at these shapes as on
     the draw c32 was computed on;
  3. the elements that differ in bits from the restatement, and the largest such difference in units of 2^-24 S,
     are counted per operator before anything is asserted (STATS, printed when the module ends).

Momentum (plain and Nesterov) is bit for bit against cpu.momentum_sparse, whole tables: occurrence-ordered adds and
an element-wise dense phase leave no freedom.

Inputs come from the one builder of tests/test_optim_oracle.py (gradient rows scaled over 1e-4 .. 3, states over
matching ranges, eps = 1e-2, lr = 0.05, wd = 0.1; ids unique and SHUFFLED; Lamb: rows no id names are 100x larger).
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from herald_amd import _lib, ops
from oracle import cpu
from oracle import optim_ref64 as ref64
from test_gpu_parity import _runs_batch
from test_optim_oracle import (HYPER, OPS, STATES, bound_units, build_inputs, build_momentum, hyper_of,
                               named_part, step32, step64)

pytestmark = pytest.mark.gpu

SYMBOL = {"l2": "AddL2RegularizationSparse", "adagrad": "AdaGradOptimizerSparseUpdate",
          "adam": "AdamOptimizerSparseUpdate", "adamw": "AdamWOptimizerSparseUpdate",
          "lamb": "LambOptimizerSparseUpdate", "momentum": "MomentumOptimizerSparseUpdate",
          "nesterov": "MomentumOptimizerSparseUpdate"}
ALL_OPS = OPS + ("momentum", "nesterov")

STATS = {}     # op -> [calls, elements compared, elements differing in bits from the restatement, worst units]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _same_bits(got, want, what):
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=what)


def _state_names(op):
    return STATES[op] if op in STATES else ("velocity",)


def _scalars(op, t, hyper=None):
    sc = hyper_of(op, t) if hyper is None else hyper
    return [ctypes.c_bool(x) if isinstance(x, bool) else ctypes.c_float(x) for x in sc]


def _raw_call(op, d, ids, grads, t, hyper=None):
    """The symbol's own return value (ops.dl_call raises on -1).  d, ids, grads: tensors or ops.DLHolder."""
    arrays = [d["param"], ids, grads] + [d[k] for k in _state_names(op)]
    holders = [a if isinstance(a, ops.DLHolder) else ops.DLHolder(a) for a in arrays]
    stream = ops.DLStreamHolder()
    return getattr(_lib.load(), SYMBOL[op])(*([h.handle for h in holders] + _scalars(op, t, hyper) + [stream.handle]))


def _host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _judged_call(op, d, ids, grads, t, hyper=None, before=None):
    """One call of `op` on the device arrays d (param + states), judged as the module docstring says.  Returns the
    arrays read back after the call."""
    before = _host(d) if before is None else before
    ids0, g0 = ids.cpu().numpy(), grads.cpu().numpy()
    if op in ("momentum", "nesterov"):
        want = step32(op, before, ids0, g0, t, hyper)
        assert _raw_call(op, d, ids, grads, t, hyper) == 0, _lib.load().ha_last_error()
        after = _host(d)
        for name in ("param", "velocity"):
            _same_bits(after[name], want[name], "%s %s" % (op, name))
        _same_bits(ids.cpu().numpy(), ids0, "ids")
        _same_bits(grads.cpu().numpy(), g0, "gradients")
        return after
    sel, idx, out = step64(op, before, ids0, g0, t, hyper=hyper)
    want = step32(op, before, ids0, g0, t, hyper)
    assert _raw_call(op, d, ids, grads, t, hyper) == 0, _lib.load().ha_last_error()
    after = _host(d)
    after["grad"] = grads.cpu().numpy().reshape(ids0.size, -1)
    before = dict(before, grad=g0.reshape(ids0.size, -1))
    _same_bits(ids.cpu().numpy(), ids0, "ids")
    stats = STATS.setdefault(op, [0, 0, 0, 0.0])
    stats[0] += 1
    for name in before:
        what = "%s %s" % (op, name)
        if name not in out:                       # not an output of this operator: untouched altogether
            _same_bits(after[name], before[name], what)
            continue
        changed = np.flatnonzero((_bits(after[name]) != _bits(before[name])).any(axis=1))
        stray = np.setdiff1d(changed, sel if name == "grad" else idx)
        assert stray.size == 0, "%s: rows %s changed and no in-range id names them" % (what, stray[:10])
        x64, s = out[name]
        got, w32 = named_part(op, name, after[name], sel, idx), named_part(op, name, want[name], sel, idx)
        differs = _bits(got) != _bits(w32)
        stats[1] += got.size
        stats[2] += int(differs.sum())
        if differs.any():
            stats[3] = max(stats[3], ref64.units(got[differs], w32[differs].astype(np.float64), s[differs]))
        _same_bits(got, w32, what + ", named rows against the float32 restatement")
        off = ref64.units(got, x64, s)
        assert off <= bound_units(op, name), "%s: %.2f units of 2^-24 S from float64, bound %.2f" % (
            what, off, bound_units(op, name))
    return after


def _upload(a, dev, names):
    return {k: torch.from_numpy(a[k].copy()).to(dev) for k in names}


def _run_steps(op, a, dev, steps=(1, 2, 3), ids_shape=None):
    """Steps t = 1, 2, 3 of `op` on the inputs `a`, every call judged.  ids_shape: the ids handed over as an array of
    that shape with gradients of shape ids_shape + (width,): n = numel(ids)."""
    d = _upload(a, dev, ("param",) + _state_names(op))
    ids, grads = torch.from_numpy(a["ids"]).to(dev), torch.from_numpy(a["grads"].copy()).to(dev)
    if ids_shape is not None:
        ids, grads = ids.reshape(ids_shape), grads.reshape(tuple(ids_shape) + (grads.shape[-1],))
    for t in steps:
        if op == "l2":                            # its output is the gradient: start each step from the same one
            grads.copy_(torch.from_numpy(a["grads"]).to(dev).reshape(grads.shape))
        _judged_call(op, d, ids, grads, t)


def _inputs(op, seed, rows, width, n, beyond=False):
    return build_inputs(seed, rows, width, n, beyond=beyond, other_scale=100.0 if op == "lamb" else 1.0)


@pytest.fixture(scope="module", autouse=True)
def _report():
    """Assertion 3: print what was counted; HERALD_OPTIM_STATS=<file> also writes it as JSON."""
    yield
    for op, (calls, elems, differing, worst) in sorted(STATS.items()):
        print("\n%-8s %5d calls  %11d elements  %9d differ in bits from the float32 restatement  worst %.2f units"
              % (op, calls, elems, differing, worst))
    if os.environ.get("HERALD_OPTIM_STATS"):
        with open(os.environ["HERALD_OPTIM_STATS"], "w") as f:
            json.dump(STATS, f)


# ---- sparse_row_kernel: the column loop -------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 3, 4, 7, 252, 256, 260, 400, 508, 512, 516, 1024, 1030, 2048])
def test_every_column_trip_of_the_row_kernel(dev, width):
    """`for (c0 = 0; c0 < width; c0 += 2 * kWave * VEC)` of sparse_row_kernel, two vectors per lane per trip:
      VEC == 4 (width % 4 == 0, one trip covers 512 columns): 4 one lane of the first vector live; 252 / 256 the
        second vector dead (its clamped load at column 0 is discarded); 260 ONE lane of the second vector live; 400,
        508 part of it; 512 exactly one trip; 516 (> 512, % 4 == 0) a SECOND TRIP with one lane live; 1024 two full
        trips; 2048 four;
      VEC == 1 (one trip covers 128 columns): 1, 3, 7 inside the first vector; 1030 nine trips, the last with six
        lanes of its first vector.
    n = 1, 3, 4, 5 (one workgroup of four waves: fewer rows than waves, exactly as many, one wave with a second
    row) and 300; at n = 300 the ids are a (15, 20) array with (15, 20, width) gradients.  L2, AdaGrad, Adam, AdamW,
    Lamb; three steps each."""
    for n in (1, 3, 4, 5, 300):
        for op in OPS:
            a = _inputs(op, 1000 * width + n, 2 * n + 3, width, n)
            _run_steps(op, a, dev, ids_shape=(15, 20) if n == 300 else None)


# ---- sparse_row_kernel: the row loop ----------------------------------------------------------------------------
@pytest.mark.parametrize("width", [4, 7])
@pytest.mark.parametrize("n", [65536, 65537, 150001])
def test_second_trip_of_the_grid_stride_loop(dev, n, width):
    """`for (i = wave; i < n; i += nwaves)`: row_launch caps the grid at 16,384 workgroups of 4 waves, nwaves = 65,536.
    n = 65,536 is the last n with one trip; n = 65,537 > 16,384 x 4 gives wave 0 a second trip at its first index
    (i = 65,536); n = 150,001 = 2 x 65,536 + 18,929 three trips, the last ragged.  Width 4 is VEC == 4, width 7
    VEC == 1.  Lamb also sums 150,001 per-row partials in lamb_norms_kernel, 147 passes of its 1,024 threads."""
    for op in OPS:
        _run_steps(op, _inputs(op, n + width, 200000, width, n), dev)


# ---- n = 0 ------------------------------------------------------------------------------------------------------
def _empty(t):
    """DLArray of zero elements with a real data pointer (torch reports a null one for an empty tensor): the
    holder of `t` with its first extent set to 0."""
    h = ops.DLHolder(t)
    h.shape[0] = 0
    return h


@pytest.mark.parametrize("op", ALL_OPS)
def test_no_ids(dev, op):
    """n = 0 returns 0 for every symbol (row_launch's `if (n == 0) return 0`, Lamb's own) and changes nothing --
    but MomentumOptimizerSparseUpdate still runs its dense second phase over the table (`if (n > 0)` around the
    first phase only), as the reference does."""
    if op in ("momentum", "nesterov"):
        a = build_momentum(5, 30, 12, 8)
    else:
        a = build_inputs(5, 30, 12, 8)
    d = _upload(a, dev, ("param",) + _state_names(op))
    ids, grads = torch.from_numpy(a["ids"]).to(dev), torch.from_numpy(a["grads"]).to(dev)
    assert _raw_call(op, d, _empty(ids), _empty(grads), 2) == 0, _lib.load().ha_last_error()
    torch.cuda.synchronize()
    after = _host(d)
    want = step32(op, a, a["ids"][:0], a["grads"][:0], 2) if op in ("momentum", "nesterov") else a
    for name in d:
        _same_bits(after[name], want[name], name)
    if op in ("momentum", "nesterov"):
        assert np.all(_bits(after["param"]) != _bits(a["param"]))       # the dense phase did happen
    _same_bits(grads.cpu().numpy(), a["grads"], "gradients")


# ---- misaligned arrays ------------------------------------------------------------------------------------------
SENTINEL = -12345.625


def _offset_view(x, dev):
    """x on the device as a view that starts 4 bytes into its buffer, a sentinel before and after it."""
    buf = torch.full((x.size + 2,), SENTINEL, dtype=torch.float32, device=dev)
    buf[1:1 + x.size] = torch.from_numpy(x.reshape(-1)).to(dev)
    view = buf[1:1 + x.size].view(*x.shape)
    assert view.data_ptr() % 16 == 4
    return buf, view


_MISALIGNED = [(op, which) for op in ALL_OPS
               for which in ("param", "grads") + _state_names(op) + ("all",)]


@pytest.mark.parametrize("op,which", _MISALIGNED)
def test_arrays_that_are_not_16_byte_aligned(dev, op, which):
    """vec_ok() false because a POINTER is not 16-byte aligned while width % 4 == 0 (width 64): sparse_row_kernel
    runs as VEC == 1 at a width every other test runs as VEC == 4.  Each of param, gradients, state 1, state 2 in
    turn, and all together, is `buf[1:1 + rows * width].view(rows, width)`; the element before and the element after
    the view must survive.  Momentum: the first phase (ha_sgd_apply) and the dense phase (momentum_dense_kernel<.,
    1>, one element per thread) take their scalar paths; such views used to be refused."""
    rows, width, n = 50, 64, 20
    a = build_momentum(9, rows, width, 60, beyond=2) if op in ("momentum", "nesterov") else _inputs(op, 9, rows, width, n)
    bufs, d = {}, {}
    for name in ("param",) + _state_names(op):
        if which in (name, "all"):
            bufs[name], d[name] = _offset_view(a[name], dev)
        else:
            d[name] = torch.from_numpy(a[name].copy()).to(dev)
    ids = torch.from_numpy(a["ids"]).to(dev)
    if which in ("grads", "all"):
        bufs["grads"], grads = _offset_view(a["grads"], dev)
    else:
        grads = torch.from_numpy(a["grads"].copy()).to(dev)
    for t in (1, 2, 3):
        _judged_call(op, d, ids, grads, t)
    for name, buf in bufs.items():
        ends = buf[[0, -1]].cpu().numpy()
        _same_bits(ends, np.full(2, SENTINEL, dtype=np.float32), "sentinels around " + name)


# ---- ids beyond the table ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [7, 64])
@pytest.mark.parametrize("op", OPS)
def test_ids_beyond_the_table_are_skipped(dev, op, width):
    """`if (r < rows)` false: a tenth of the ids are rows, rows + 1, 2^31 and 4.0e9 (all below 2^32, the range of the
    float -> uint32 conversion), mixed in.  The result is the reference with those positions skipped: their
    gradient rows (L2's output) keep their bits, and Lamb -- whose skipped rows still write their two partial sums,
    as zeros -- takes both norms over the in-range rows only."""
    _run_steps(op, _inputs(op, 40 + width, 500, width, 200, beyond=True), dev)


def test_float32_ids_above_2_to_the_24(dev):
    """A table of 2^24 + 8 rows x width 4 and the ids {2^24, 2^24 + 2, 2^24 + 4, 3}: float32 ids where not every
    integer is a float any more, row offsets (r * width) beyond 2^26 elements.  One step (t = 3) of each operator
    from the same state; whole 268 MB arrays compared."""
    rows, width = (1 << 24) + 8, 4
    rng = np.random.default_rng(24)
    base = dict(param=rng.standard_normal((rows, width), dtype=np.float32))
    base["m"] = base["param"][::-1] * np.float32(0.3)
    base["v"] = base["param"] ** 2
    base["acc"] = base["v"][::-1] * np.float32(2.0)
    base = {k: np.ascontiguousarray(v) for k, v in base.items()}
    ids_np = np.array([1 << 24, (1 << 24) + 2, (1 << 24) + 4, 3], dtype=np.float32)
    g_np = rng.standard_normal((4, width), dtype=np.float32)
    ids = torch.from_numpy(ids_np).to(dev)
    dev_base = _upload(base, dev, ("param", "m", "v", "acc"))
    for op in OPS:
        d = {k: dev_base[k] for k in ("param",) + STATES[op]}
        for k in d:
            d[k].copy_(torch.from_numpy(base[k]))
        grads = torch.from_numpy(g_np.copy()).to(dev)
        _judged_call(op, d, ids, grads, 3, before={k: base[k] for k in d})


# ---- Lamb -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2500])
def test_lamb_norms_are_over_the_indexed_rows_in_a_fixed_order(dev, n):
    """LambOptimizerSparseUpdate's two norms are over the INDEXED rows: the other rows of the table are 100 times
    larger, so a norm over the whole table would change the step a hundredfold.  lamb_norms_kernel strides its
    1,024 threads over the n per-row partials: n = 1 one thread, 1,023 / 1,024 / 1,025 around one pass, 2,500 a
    ragged third pass.  The sums have a fixed order: the same call from the same state gives the same bits."""
    a = _inputs("lamb", n, 3000, 20, n, beyond=n > 1)
    _run_steps("lamb", a, dev)
    runs = []
    for _ in range(2):
        d = _upload(a, dev, ("param", "m", "v"))
        assert _raw_call("lamb", d, torch.from_numpy(a["ids"]).to(dev), torch.from_numpy(a["grads"]).to(dev), 2) == 0
        runs.append(_host(d))
    for name in ("param", "m", "v"):
        _same_bits(runs[0][name], runs[1][name], name)


@pytest.mark.parametrize("wd", [0.1, 0.0])
def test_lamb_divides_by_a_zero_norm_as_the_reference_does(dev, wd):
    """All-zero gradient on all-zero moments: the update direction is 0, norm(update) is 0 and the ratio is
    norm(param) / 0 (OptimizersSparse.cu:578).  With wd = 0.1 the step is inf * (0.1 p): every named element becomes
    an infinity of the sign opposite to p's; with wd = 0 it is inf * 0: NaN.  The pattern, element for element,
    is the float32 restatement's -- the one comparison here where values are set aside: NaN has no bits to compare."""
    a = build_inputs(6, 40, 12, 10)
    a["m"][...] = 0
    a["v"][...] = 0
    a["grads"][...] = 0
    hyper = hyper_of("lamb", 1)[:-1] + (wd,)
    want = step32("lamb", a, a["ids"], a["grads"], 1, hyper)
    idx = a["ids"].astype(np.int64)
    assert not np.isfinite(want["param"][idx]).any()
    assert np.isnan(want["param"][idx]).all() if wd == 0.0 else np.isinf(want["param"][idx]).all()
    d = _upload(a, dev, ("param", "m", "v"))
    assert _raw_call("lamb", d, torch.from_numpy(a["ids"]).to(dev), torch.from_numpy(a["grads"]).to(dev), 1, hyper) == 0
    after = _host(d)
    nan = np.isnan(want["param"])
    np.testing.assert_array_equal(np.isnan(after["param"]), nan)
    _same_bits(after["param"][~nan], want["param"][~nan], "param where it is not NaN")
    _same_bits(after["m"], want["m"], "m")
    _same_bits(after["v"], want["v"], "v")


# ---- Momentum ---------------------------------------------------------------------------------------------------
def _momentum_steps(op, a_of_step, dev, steps=3):
    a = a_of_step(0)
    d = _upload(a, dev, ("param", "velocity"))
    for t in range(steps):
        b = a_of_step(t)
        _judged_call(op, d, torch.from_numpy(b["ids"]).to(dev), torch.from_numpy(b["grads"]).to(dev), t + 1)


@pytest.mark.parametrize("op", ["momentum", "nesterov"])
@pytest.mark.parametrize("rows,width", [(5, 7), (3, 1), (1, 2), (9, 5), (40, 6)])
def test_momentum_dense_phase_tail(dev, op, rows, width):
    """momentum_dense_kernel's `if (blockIdx.x == 0 && threadIdx.x < (total & 3u))`: rows x width = 35, 3, 2, 45, 240
    -> total & 3 = 3, 3, 2, 1, 0.  (3, 1) and (1, 2) are tables of fewer than 4 elements: nvec == 0, `blocks = 1`,
    the tail is all there is.  Zipf-repeated ids, three of them beyond the table (the first phase ignores them);
    three steps, bit for bit."""
    _momentum_steps(op, lambda t: build_momentum(rows * 10 + width + t, rows, width, 50, beyond=3), dev)


@pytest.mark.parametrize("op", ["momentum", "nesterov"])
def test_momentum_first_phase_through_the_radix_plan(dev, op):
    """n = 40,000 > 36,864 on a 3,000 x 64 table: ha_plan_sort_f32ids takes the radix sort, and the occurrence-ordered
    apply meets runs of thousands (Zipf: row 0 takes about 15,000 occurrences)."""
    _momentum_steps(op, lambda t: build_momentum(77 + t, 3000, 64, 40000, beyond=4), dev, steps=2)


def test_momentum_dense_phase_grid_stride_loop(dev):
    """9,586,981 x 7 = 67,108,867 elements: nvec = 16,777,216 float4 + 3 tail elements, one more than the
    65,536 workgroups x 256 threads of the capped grid cover in one pass, so thread 0 makes a second trip of
    `for (e = ...; e < nvec; e += stride)`, and total & 3 == 3.  Plain and Nesterov, one step each from the same
    state; a handful of ids, two beyond the table."""
    rows, width = 9586981, 7
    assert rows * width == 65536 * 256 * 4 + 3
    rng = np.random.default_rng(67)
    a = dict(param=rng.standard_normal((rows, width), dtype=np.float32),
             ids=np.array([5, rows - 1, 5, 0, rows, 70000, 5, 4.0e9], dtype=np.float32),
             grads=rng.standard_normal((8, width), dtype=np.float32))
    a["velocity"] = np.ascontiguousarray(a["param"][::-1]) * np.float32(0.1)
    d = _upload(a, dev, ("param", "velocity"))
    ids, grads = torch.from_numpy(a["ids"]).to(dev), torch.from_numpy(a["grads"]).to(dev)
    for op in ("momentum", "nesterov"):
        for k in d:
            d[k].copy_(torch.from_numpy(a[k]))
        _judged_call(op, d, ids, grads, 1, before={k: a[k] for k in d})


# ---- fused dedup + optimizer ------------------------------------------------------------------------------------
_LENGTHS = [2, 3, 4, 5, 15, 16, 17, 30, 31, 32, 33, 46, 47, 48, 49, 50, 62, 63, 64, 65, 79, 80, 81, 95, 96,
            97, 127, 128, 129, 143, 144, 160, 200, 255, 256, 257, 300, 511, 512, 513, 1000]


def _fused_case(dev, kind, width, ids, rows, seed):
    rng = np.random.default_rng(seed)
    n = ids.size
    a = build_inputs(seed, rows, width, 1)
    a["grads"] = rng.standard_normal((n, width), dtype=np.float32)
    if kind == "adagrad":
        a["m"] = a["acc"]
    h = HYPER
    hyper = dict(lr=h["lr"], eps=h["eps"], beta1=h["beta1"], beta2=h["beta2"], beta1t=h["beta1"] ** 3,
                 beta2t=h["beta2"] ** 3, weight_decay=h["weight_decay"])
    d_ids, d_g = torch.from_numpy(ids).to(dev), torch.from_numpy(a["grads"]).to(dev)
    f = _upload(a, dev, ("param", "m", "v"))
    ops.sparse_opt_fused(kind, f["param"], d_ids, d_g, f["m"], None if kind == "adagrad" else f["v"], **hyper)
    torch.cuda.synchronize()
    fused = _host(f)
    # the two-step sequence, its optimizer call judged against float64 on the occurrence-ordered float32 sums
    uniq, _, red = cpu.dedup_reduce(ids, a["grads"])
    sl = ops.IndexedSlices(d_ids, d_g, (rows, width)).deduplicate()
    _same_bits(sl.indices.cpu().numpy(), uniq.astype(np.float32), "deduplicated ids")
    _same_bits(sl.values.cpu().numpy(), red, "deduplicated gradients")
    names = {"param": "param", "acc" if kind == "adagrad" else "m": "m"}
    if kind != "adagrad":
        names["v"] = "v"
    two = {k: torch.from_numpy(a[src].copy()).to(dev) for k, src in names.items()}
    after = _judged_call(kind, two, sl.indices.contiguous(), sl.values.contiguous(), 3)
    for k, src in names.items():
        _same_bits(fused[src], after[k], "fused %s against deduplicate() + %s" % (k, SYMBOL[kind]))
    if kind == "adagrad":
        _same_bits(fused["v"], a["v"], "state2 is not AdaGrad's")


@pytest.mark.parametrize("width", [64, 200, 516, 2048])
@pytest.mark.parametrize("kind", ["adagrad", "adam", "adamw"])
def test_fused_epilogue_of_every_run_length_class(dev, kind, width):
    """ha_sparse_opt_fused_f32ids, the kModeOpt epilogues of scatter_dev.h, one per run-length class: the raw ids
    hold one run of every length of test_apply_every_run_length_class -- 2, 3 (short: 1-3), 4 .. 47 (medium),
    48 .. 1000 (long, the cooperative workgroup path) -- between 3,000 singles, plus 9 occurrences of ids beyond
    the table; n = 8,854 <= 36,864 so apply_opt_kernel runs by position.  Bit-equal to deduplicate() + the symbol
    in ALL THREE arrays, and that symbol's call is judged against float64 like any other."""
    rng = np.random.default_rng(width + len(kind))
    rows = 4000
    ids = np.concatenate([_runs_batch(rng, _LENGTHS, 3000, rows),
                          np.array([rows, rows, rows + 1, 2.0 ** 31, 4.0e9] + [rows + 7] * 4, dtype=np.float32)])
    rng.shuffle(ids)
    _fused_case(dev, kind, width, ids, rows, width * 7 + len(kind))


@pytest.mark.parametrize("kind", ["adagrad", "adam", "adamw"])
def test_fused_epilogue_by_unique_key(dev, kind):
    """n = 40,000 > 36,864: ha_plan_finish + apply_by_unique<kModeOpt> (scatter.hip), waves mapped to unique keys;
    a run of 5,000 (giant: longer than the 1,024 positions a workgroup scans) and runs of 2,500, 300, 48, 5."""
    rng = np.random.default_rng(len(kind))
    rows, width = 50000, 64
    lengths = [5000, 2500, 300, 48, 5]
    ids = np.concatenate([_runs_batch(rng, lengths, 40000 - sum(lengths) - 3, rows),
                          np.array([rows, rows + 1, rows], dtype=np.float32)])
    rng.shuffle(ids)
    assert ids.size == 40000
    _fused_case(dev, kind, width, ids, rows, 400 + len(kind))


# ---- refused calls ----------------------------------------------------------------------------------------------
_REFUSALS = [(op, why) for op in ALL_OPS
             for why in ("gradient-size", "1-D-param", "host-gradients") +
             (("state-size", "host-state") if _state_names(op) else ())]     # sparse L2 has no state array


@pytest.mark.parametrize("op,why", _REFUSALS)
def test_refused_calls_change_nothing(dev, op, why):
    """check_args refuses before anything is enqueued: gradient size != n x width, state size != param size, a 1-D
    param, a host array (gradients; a state array) -> -1, ha_last_error() names the symbol, and after a
    torch.cuda.synchronize() every array has the bits it had.  (A MomentumOptimizerSparseUpdate on a param or
    velocity that is not 16-byte aligned used to be refused AFTER its first phase had run; it is served now:
    test_arrays_that_are_not_16_byte_aligned.)"""
    states = _state_names(op)
    rows, width, n = 30, 8, 12
    a = build_momentum(2, rows, width, n) if op in ("momentum", "nesterov") else build_inputs(2, rows, width, n)
    d = _upload(a, dev, ("param",) + states)
    ids, grads = torch.from_numpy(a["ids"]).to(dev), torch.from_numpy(a["grads"].copy()).to(dev)
    call = dict(d)
    c_ids, c_grads = ids, grads
    if why == "gradient-size":
        c_grads = grads[:n - 1]
    elif why == "state-size":
        call[states[-1]] = d[states[-1]][:rows - 1]
    elif why == "1-D-param":
        call["param"] = d["param"].view(-1)
    elif why == "host-gradients":
        c_grads = torch.from_numpy(a["grads"].copy())
    else:
        call[states[-1]] = torch.from_numpy(a[states[-1]].copy())
    L = _lib.load()
    assert _raw_call(op, call, c_ids, c_grads, 2) == -1
    assert SYMBOL[op] in L.ha_last_error().decode()
    torch.cuda.synchronize()
    after = _host(d)
    for name in d:
        _same_bits(after[name], a[name], name)
    _same_bits(grads.cpu().numpy(), a["grads"], "gradients")
    _same_bits(ids.cpu().numpy(), a["ids"], "ids")

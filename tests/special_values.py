"""Special FLOAT VALUES for every row kernel (tests/test_gpu_special_values.py, tests/test_special_values_cpu.py): +-0,
subnormals, values whose sums overflow, infinities, NaNs with payloads and exact cancellations, planted at chosen occurrence
slots and columns of an id batch that has one run of every length class.  Test infrastructure only: nothing under herald_amd/
imports it, and it needs numpy alone.

The contract: the kernels are plain IEEE float32, one rounding per operation, in the documented order.
Subnormals are kept, zeros keep their signs, and a NaN or an infinity spreads only along the chain of the key and the column it
sits in.  np.testing.assert_array_equal sees neither the sign of a zero nor (for computed values) should it see a NaN's
payload, so the comparisons here are same_bits().

Value classes, each planted into one (key, column) of a poisoned key (VARIANTS maps the planted variants to them):
    Z   the row holds -0 and every gradient of the column is +0 (the row stays -0), or every gradient is -0
    S   subnormal gradients (+-2^-149, +-1e-40, 0x007FFFFF, normal values whose product with lr is subnormal or rounds to a
        signed zero) over a zero or subnormal row; a subnormal row under zero gradients
    H   finite gradients of 3e38 at every chosen slot over a row of -3e38: sum and update overflow in every order
    I   one infinity at a chosen slot, or +inf and -inf at two of them (NaN in that element only)
    N   one quiet NaN (payload 0x7FC12345 or negative 0xFFC00001) at a chosen slot; a NaN row under normal gradients
    C   g and -g at two slots of an otherwise zero column over a -0 row: the chain ends in +0, a tree (row - sum) in -0

The chosen slots of a run of c occurrences are the first, the middle and the last one and the slots just before and just after
every multiple of 16 and of 256 the run reaches (m - 1 and m); the chosen columns are 0, 3, 63, 64 where the width has them, the
last one, one in the ragged last slice of 64 where width % 64 != 0, and further ones up to one per variant.

The clean twin of a poisoned key is the key just below it: a kernel that reads past the end of the twin's run in sorted order
reads the poisoned key's first occurrences."""
import numpy as np

F = np.float32
FLT_MIN = np.float32(1.17549435e-38)
CANON_NAN = np.uint32(0x7FC00000)
NAN_PAYLOAD = np.array([0x7FC12345], dtype=np.uint32).view(np.float32)[0]
NAN_NEGATIVE = np.array([0xFFC00001], dtype=np.uint32).view(np.float32)[0]
SUB_MAX = np.array([0x007FFFFF], dtype=np.uint32).view(np.float32)[0]
SUB_MIN = np.array([0x00000001], dtype=np.uint32).view(np.float32)[0]
NEG_ZERO = np.float32(-0.0)
HUGE = np.float32(3.0e38)
LR = 0.37                        # not a power of two: lr * g rounds

CLASSES = ("Z", "S", "H", "I", "N", "C")
# planted variants -> value class (T*: the special sits in the table row, under zero or normal gradients)
VARIANTS = (("Z", "Z"), ("S", "S"), ("H", "H"), ("I", "I"), ("N", "N"), ("C", "C"), ("TS", "S"), ("TN", "N"), ("ZN", "Z"))
SMALL_RUNS = (1, 2, 3, 4, 15, 16, 17, 47, 48, 49, 63, 64, 65, 70, 255, 256, 257, 1023, 1025)
BIG_RUNS = (3, 17, 70, 300, 2100)
BIG_N = 1419 * 26                # 36,894 ids > 36,864: the plans and applies switch to their by-unique-key paths
RUN_CLASSES = ((1, 3), (4, 15), (16, 47), (48, 63), (64, 256), (257, 1 << 30))     # short, medium (chain below 16 in the
# work-queue step), tree from 16 there, long, cooperative, chunked
RESULT_KINDS = {"Z": ("-0",), "S": ("sub",), "H": ("inf",), "I": ("inf", "nan"), "N": ("nan",), "C": ("+0", "-0")}


def run_class(c):
    return [i for i, (lo, hi) in enumerate(RUN_CLASSES) if lo <= c <= hi][0]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def canon(a):
    """uint32 bits with every NaN mapped to one pattern."""
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = CANON_NAN
    return b


def kind_of(x):
    """'nan', 'inf', 'sub', '-0', '+0' or 'normal' of one float32."""
    x = np.float32(x)
    if np.isnan(x):
        return "nan"
    if np.isinf(x):
        return "inf"
    if x == 0:
        return "-0" if np.signbit(x) else "+0"
    return "sub" if abs(x) < FLT_MIN else "normal"


def same_bits(got, want, what, copy=False, poisoned=None, rows=None):
    """Asserts that two float32 arrays are the same bit for bit.  copy=False (computed values): every NaN of either side counts
    as one NaN -- the CPU and the GPU make different default NaNs.  copy=True (kernels that only move rows): raw bits, a NaN's
    payload and sign included.  poisoned: bool array shaped as the arrays (or broadcastable rows: see Case.mask_of) saying which
    elements may depend on a planted value; rows: the key of every row of the arrays (default: the row index).  The message
    names the first differing element and whether it lies inside the poisoned set (a wrong value) or outside (a leak)."""
    got = np.asarray(got)
    want = np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32, "%s: float32 arrays expected" % what
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    g, w = (bits(got), bits(want)) if copy else (canon(got), canon(want))
    diff = g != w
    if not diff.any():
        return int(g.size)
    flat = np.flatnonzero(diff.reshape(-1))
    first = int(flat[0])
    width = got.shape[-1] if got.ndim >= 2 else 1
    r, col = divmod(first, width)
    key = int(np.asarray(rows).reshape(-1)[r]) if rows is not None else r
    if poisoned is None:
        where = "no poisoned set given"
    else:
        inside = bool(np.broadcast_to(np.asarray(poisoned), got.shape).reshape(-1)[first])
        where = "INSIDE the poisoned set: a wrong value" if inside else "OUTSIDE the poisoned set: a leak"
    raise AssertionError("%s: %d of %d elements differ; first at row %d (key %d) column %d: got 0x%08X (%r), expected 0x%08X (%r); %s"
                         % (what, flat.size, g.size, r, key, col, int(bits(got).reshape(-1)[first]), float(got.reshape(-1)[first]),
                            int(bits(want).reshape(-1)[first]), float(want.reshape(-1)[first]), where))


def chosen_slots(c):
    """Occurrence slots of a run of c: first, middle, last, and m - 1, m for every multiple m of 16 and of 256 below c."""
    s = {0, c // 2, c - 1}
    for m in range(16, c + 1, 16):
        s.update((m - 1, m))
    return sorted(x for x in s if 0 <= x < c)


def chosen_columns(width, want=len(VARIANTS)):
    cols = [x for x in (0, 3, 63, 64) if x < width] + [width - 1]
    if width % 64 and width > 64:
        cols.append(width // 64 * 64 + (width % 64) // 2)
    for extra in (1, 2, 5, 17, 31, 33, 65, 100, 130):
        if extra < width:
            cols.append(extra)
    out = []
    for x in cols:
        if x not in out:
            out.append(x)
    return out[:want]


class Case:
    """One batch.  ids int64 [n] (all in range, none 0); grads float32 [n, width]; table float32 [rows, width]; the clean twins
    grads_clean / table_clean hold a finite draw wherever a value was planted.  poisoned: bool [rows, width], the (key, column)
    pairs whose result may depend on a planted value.  planted: [(variant, class, key, run length, column)]."""

    def __init__(self, name, ids, grads, table, grads_clean, table_clean, poisoned, planted, runs, lr):
        self.name, self.ids, self.grads, self.table = name, ids, grads, table
        self.grads_clean, self.table_clean, self.poisoned, self.planted, self.runs, self.lr = \
            grads_clean, table_clean, poisoned, planted, runs, lr
        self.n, self.width = grads.shape
        self.rows = table.shape[0]

    @property
    def ids_f32(self):
        return self.ids.astype(np.float32)

    def mask_of(self, keys):
        """The poisoned set of an array whose row r belongs to key keys[r]."""
        return self.poisoned[np.asarray(keys, dtype=np.int64).reshape(-1)]

    def clean(self):
        """The same batch with every planted value replaced by a finite draw."""
        return Case(self.name + "-clean", self.ids, self.grads_clean, self.table_clean, self.grads_clean, self.table_clean,
                    self.poisoned, self.planted, self.runs, self.lr)

    def __repr__(self):
        return self.name


def _plant(variant, c, slots, which, g, p, rng, lr):
    """The gradient column g [c] (occurrence order) and the row element p of one planted (key, column); which: a counter that
    rotates the single-slot choices.  Returns (g, p)."""
    f = F
    if variant == "Z":
        return np.zeros(c, f), NEG_ZERO
    if variant == "ZN":
        return np.full(c, NEG_ZERO, f), NEG_ZERO
    if variant == "S":
        g = np.zeros(c, f)
        tiny = (SUB_MIN, -SUB_MIN, f(1e-40), f(-1e-40))
        for i, s in enumerate(slots):
            g[s] = tiny[(i + which) % 4]
        g[slots[0]] = SUB_MAX
        if c > 1:
            g[slots[-1]] = f(-2e-38)
        return g, (f(0) if which % 2 else SUB_MAX)
    if variant == "TS":
        g = np.zeros(c, f)
        g[slots[which % len(slots)]] = NEG_ZERO
        return g, f(1e-40) if which % 2 else -SUB_MIN
    if variant == "H":
        g = g.copy()
        g[slots] = HUGE
        return g, -HUGE
    if variant == "I":
        g = g.copy()
        a = slots[which % len(slots)]
        g[a] = f(np.inf) if which % 3 else f(-np.inf)
        if c > 1 and which % 2:
            b = slots[(which + 1) % len(slots)]
            if b != a:
                g[b] = -g[a]
        return g, p
    if variant == "N":
        g = g.copy()
        g[slots[which % len(slots)]] = NAN_PAYLOAD if which % 2 else NAN_NEGATIVE
        return g, p
    if variant == "TN":
        return g, (NAN_NEGATIVE if which % 2 else NAN_PAYLOAD)
    if variant == "C":
        g = np.zeros(c, f)
        x = f(rng.standard_normal())
        if c == 1:
            g[0] = x
            return g, f(f(lr) * x)                       # row - lr * g is an exact +0
        a, b = slots[which % len(slots)], slots[(which + 1) % len(slots)]
        if a == b:
            b = (a + 1) % c
        g[a], g[b] = x, -x
        return g, NEG_ZERO
    raise ValueError(variant)


def make_case(width, runs=SMALL_RUNS, n=8000, rows=4000, seed=0, key_seed=None, lr=LR, rotate=0, table=None):
    """One run of every length in `runs` for a poisoned key and one for its clean twin (the key just below), the rest of the
    `n` ids single occurrences of other keys (distinct while the table has enough rows, else drawn with repetition), in shuffled
    order.  key_seed fixes the keys and the planted columns so that the batches of a stream share their poisoned keys (seed then
    varies the order, the draws and -- through rotate -- which variant sits in which column); table: the table of an earlier
    batch of the stream, kept as it is."""
    key_seed = seed if key_seed is None else key_seed
    krng = np.random.default_rng([key_seed, width, len(runs)])
    rng = np.random.default_rng([seed, width, n, 7])
    assert n >= 2 * sum(runs) and rows >= 2 * len(runs) + 2
    # poisoned keys: even keys >= 2, twins the odd key below -> key - 1 >= 1
    pk = 2 * krng.choice(np.arange(1, rows // 2), size=len(runs), replace=False)
    used = set(pk.tolist()) | set((pk - 1).tolist()) | {0}
    free = np.array([k for k in range(1, rows) if k not in used], dtype=np.int64)
    n_fill = n - 2 * sum(runs)
    fill = krng.permutation(free)[:n_fill] if n_fill <= free.size else free[rng.integers(0, free.size, size=n_fill)]
    ids = np.concatenate([np.repeat(pk, runs), np.repeat(pk - 1, runs), fill]).astype(np.int64)
    ids = ids[rng.permutation(n)]
    grads = rng.standard_normal((n, width), dtype=np.float32)
    own_table = table is None
    table = rng.standard_normal((rows, width), dtype=np.float32) if own_table else table.copy()
    grads_clean, table_clean = grads.copy(), table.copy()
    cols = chosen_columns(width)
    poisoned = np.zeros((rows, width), bool)
    planted = []
    for r, (key, c) in enumerate(zip(pk.tolist(), runs)):
        occ = np.flatnonzero(ids == key)                 # occurrence order
        slots = chosen_slots(c)
        for ci, col in enumerate(cols):
            variant, cls = VARIANTS[(r + ci + rotate) % len(VARIANTS)]
            g, p = _plant(variant, c, slots, r + ci + rotate + seed, grads[occ, col], table[key, col], rng, lr)
            grads[occ, col] = g
            if own_table:
                table[key, col] = p
            poisoned[key, col] = True
            planted.append((variant, cls, key, c, col))
    name = "w%d-n%d-seed%d" % (width, n, seed)
    return Case(name, ids, grads, table, grads_clean, table_clean, poisoned, planted, tuple(runs), lr)


def small_case(width, seed=0, **kw):
    return make_case(width, SMALL_RUNS, 8000, 6000, seed, **kw)


def big_case(width, seed=0, **kw):
    return make_case(width, BIG_RUNS, BIG_N, 6000, seed, **kw)


def make_stream(width, batches=3, runs=SMALL_RUNS, n=8000, rows=6000, seed=0):
    """`batches` batches over ONE table that share their poisoned keys and columns; batch b rotates the variants by b, so a
    column that held a NaN row meets zero gradients and the other way round.  -> [Case]; cases[0].table is the table the stream
    starts from, and cases[0].poisoned the poisoned set of every batch and of the table after the stream."""
    first = make_case(width, runs, n, rows, seed=seed, key_seed=seed)
    out = [first]
    for b in range(1, batches):
        out.append(make_case(width, runs, n, rows, seed=seed + b, key_seed=seed, rotate=b, table=first.table))
        assert np.array_equal(out[-1].poisoned, first.poisoned)
    return out


# ---- numpy models with switchable defects ---------------------------------------------------------------------------------------
# Unmutated they restate oracle/cpu.py (tree=None) and oracle/qstep_model.py (tree="qstep": chain below 16, tree_long below 64,
# chunked sixteen-wave tree from 64; tree="tol": the tolerance mode, one sixteen-wave tree from 64) -- the CPU test holds them to
# those bit for bit.  mutant: one of MUTANTS.
MUTANTS = ("flush_inputs", "flush_results", "pad_times_zero", "seed_first_term", "fused_rounding", "abs_zero",
           "reciprocal_multiply", "sqrt_flushes_subnormals")


def _flush(a):
    a = np.asarray(a, dtype=F).copy()
    tiny = (np.abs(a) < FLT_MIN) & (a != 0)
    a[tiny] = np.copysign(F(0), a[tiny])
    return a


class _Arith:
    def __init__(self, mutant):
        self.m = mutant

    def out(self, x):
        x = np.asarray(x, dtype=F)
        return _flush(x) if self.m == "flush_results" else x

    def mul(self, a, b):
        return self.out(F(a) * b)

    def add(self, a, b):
        return self.out(a + b)

    def sub(self, a, b):
        return self.out(a - b)

    def axpy(self, p, s, g, sign):
        """p + sign * (s * g): two roundings; one under the fused-rounding mutant."""
        if self.m == "fused_rounding":
            return (p.astype(np.float64) + sign * (np.float64(F(s)) * g.astype(np.float64))).astype(F)
        t = self.mul(s, g)
        return self.add(p, t) if sign > 0 else self.sub(p, t)


def _tree(ar, G, s, waves, groups, pad_rows):
    """Sixteen-wave tree (waves=16, groups=4: tree_coop) or the eight-lane-group tree (waves=1, groups=8: tree_long) of
    oracle/qstep_model.py over the gradient rows G [c, width] scaled by s; pad_rows [*, width]: what a kernel that pads unused
    slots by value * 0 would read past the run (the pad mutant), else None."""
    c, width = G.shape
    span = groups * (8 if waves == 1 else 4)             # occurrences of one wave per block
    block = waves * span
    part = []
    for w in range(waves):
        p = [np.zeros(width, F) for _ in range(groups)]
        seeded = [False] * groups
        for base in range(0, c, block):
            mine = base + span * w
            if mine >= c:
                break
            for t in range(span // groups):
                for r in range(groups):
                    o = mine + groups * t + r
                    if o < c:
                        term = ar.mul(s, G[o])
                        if ar.m == "fused_rounding":
                            p[r] = (p[r].astype(np.float64) + np.float64(F(s)) * G[o].astype(np.float64)).astype(F)
                        elif ar.m == "seed_first_term" and not seeded[r]:
                            p[r] = term
                        else:
                            p[r] = ar.add(p[r], term)
                        seeded[r] = True
                    elif ar.m == "pad_times_zero" and pad_rows is not None and o - c < pad_rows.shape[0]:
                        with np.errstate(all="ignore"):
                            p[r] = ar.add(p[r], ar.mul(s, pad_rows[o - c] * F(0)))
        if groups == 8:
            s1 = [ar.add(p[0], p[1]), ar.add(p[2], p[3]), ar.add(p[4], p[5]), ar.add(p[6], p[7])]
            part.append(ar.add(ar.add(s1[0], s1[1]), ar.add(s1[2], s1[3])))
        else:
            part.append(ar.add(ar.add(p[0], p[1]), ar.add(p[2], p[3])))
    if waves == 1:
        return part[0]
    quad = [ar.add(ar.add(part[4 * q], part[4 * q + 1]), ar.add(part[4 * q + 2], part[4 * q + 3])) for q in range(4)]
    return ar.add(ar.add(quad[0], quad[1]), ar.add(quad[2], quad[3]))


def model_apply(table, ids, grads, lr, mode="sgd", tree=None, chunked=False, mutant=None):
    """In place: `table` after one apply of (ids, grads).  mode "sgd": row -= lr * g in occurrence order (tree: row - tree_sum);
    "push": row + (0 + g0 + g1 + ...) (tree: row + tree_sum(g)).  tree None / "tol" / "qstep" (above); chunked: the tolerance
    mode 2 of a finished plan (runs beyond 256 in chunks of 256, the chunk sums added in order)."""
    ar = _Arith(mutant)
    ids = np.asarray(ids).reshape(-1).astype(np.int64)
    G = np.asarray(grads, dtype=F).reshape(ids.size, -1)
    if tree == "tol" and G.shape[1] % 4:
        tree = None                                      # (the tolerance mode has its tree on rows of 4 k floats only)
    if mutant == "flush_inputs":
        G = _flush(G)
        table[...] = _flush(table)
    order = np.argsort(ids, kind="stable")
    sk = ids[order]
    starts = np.flatnonzero(np.r_[True, sk[1:] != sk[:-1]])
    ends = np.r_[starts[1:], ids.size]
    s = F(1.0) if mode == "push" else F(lr)
    with np.errstate(all="ignore"):
        for a, e in zip(starts, ends):
            key = int(sk[a])
            occ = order[a:e]
            c = e - a
            rows_g = G[occ]
            pad = G[order[e:e + 256]] if mutant == "pad_times_zero" else None
            t = None
            if tree is not None and c >= 64:
                if (tree == "qstep" or chunked) and c > 256:
                    for lo in range(0, c, 256):
                        part = _tree(ar, rows_g[lo:lo + 256], s, 16, 4, G[order[a + lo + 256:a + lo + 512]] if pad is not None else None)
                        t = part if t is None else ar.add(t, part)
                else:
                    t = _tree(ar, rows_g, s, 16, 4, pad)
            elif tree == "qstep" and c >= 16:
                t = _tree(ar, rows_g, s, 1, 8, pad)
            if t is not None:
                row = ar.sub(table[key], t) if mode == "sgd" else ar.add(table[key], t)
            elif mode == "sgd":
                row = table[key].copy()
                for i in occ:
                    row = ar.axpy(row, lr, G[i], -1)
            else:
                acc = None
                for i in occ:
                    if acc is None and mutant == "seed_first_term":
                        acc = G[i].copy()
                    else:
                        acc = ar.add(np.zeros(G.shape[1], F) if acc is None else acc, G[i])
                row = ar.add(table[key], acc)
            if mutant == "abs_zero":
                row = np.where(row == 0, F(0), row).astype(F)
            table[key] = row
    return table


def model_adagrad(param, acc, ids, grads, lr, eps, mutant=None):
    """oracle/cpu.py adagrad_sparse (ids unique), with the defects of MUTANTS.  In place."""
    ar = _Arith(mutant)
    idx = np.asarray(ids).astype(np.int64)
    g = np.asarray(grads, dtype=F)
    a0, p0 = acc[idx], param[idx]
    if mutant == "flush_inputs":
        g, a0, p0 = _flush(g), _flush(a0), _flush(p0)
    with np.errstate(all="ignore"):
        if mutant == "fused_rounding":
            a = (a0.astype(np.float64) + g.astype(np.float64) * g.astype(np.float64)).astype(F)
        else:
            a = ar.add(a0, ar.mul(g, g))
        root = np.sqrt(_flush(a) if mutant == "sqrt_flushes_subnormals" else a, dtype=F)
        den = ar.add(ar.out(root), F(eps))
        num = ar.mul(F(lr), g)
        if mutant == "reciprocal_multiply":
            q = ar.mul(num, ar.out(F(1) / den))
        else:
            q = ar.out(num / den)
        p = ar.sub(p0, q)
        if mutant == "abs_zero":
            p = np.where(p == 0, F(0), p).astype(F)
    acc[idx] = a
    param[idx] = p


def optim_specials(n, width, seed=0):
    """Gradients [n, width] and AdaGrad / Adam state rows for n unique keys: row r of the first rows carries one special pairing in
    every column, the rest is standard_normal.  -> dict(g, acc, m, v, special_rows, what)."""
    rng = np.random.default_rng([seed, n, width])
    g = rng.standard_normal((n, width), dtype=np.float32)
    acc = (rng.standard_normal((n, width), dtype=np.float32) ** 2).astype(F)
    m = rng.standard_normal((n, width), dtype=np.float32)
    v = (rng.standard_normal((n, width), dtype=np.float32) ** 2).astype(F)
    what = [
        ("acc = 0, g = +0: 0 / 0 where eps = 0", F(0), F(0)),
        ("acc = 0, g = -0", NEG_ZERO, F(0)),
        ("g^2 subnormal over acc = 0", F(1e-20), F(0)),
        ("g^2 subnormal, negative g", F(-3e-21), F(0)),
        ("g^2 underflows to 0 over acc = 0", F(1e-30), F(0)),
        ("g subnormal", SUB_MAX, F(0)),
        ("subnormal state", F(0.5), F(1e-40)),
        ("state = inf", F(0.5), F(np.inf)),
        ("g^2 overflows", F(1e30), F(1.0)),
        ("g = inf", F(np.inf), F(1.0)),
        ("g = -inf over state = inf", F(-np.inf), F(np.inf)),
        ("g = NaN with payload", NAN_PAYLOAD, F(1.0)),
        ("state = negative NaN", F(0.25), NAN_NEGATIVE),
        ("g near FLT_MAX", HUGE, F(0)),
    ]
    assert n > len(what)
    for r, (_, gv, sv) in enumerate(what):
        g[r, :] = gv
        acc[r, :] = sv
        v[r, :] = sv
        m[r, ::2] = F(0)
        if width > 1:
            m[r, 1::2] = NEG_ZERO if r % 2 else SUB_MIN
    return {"g": g, "acc": acc, "m": m, "v": v, "special_rows": len(what), "what": [w[0] for w in what]}


SPRINKLE = (F(0), NEG_ZERO, SUB_MIN, -SUB_MIN, F(1e-40), F(-1e-40), SUB_MAX, F(2e-38), HUGE, -HUGE, F(np.inf), F(-np.inf),
            NAN_PAYLOAD, NAN_NEGATIVE, F(1e-20), F(-1e20))


def sprinkle(a, seed, fraction=0.02, values=SPRINKLE):
    """A copy of the float32 array `a` with about `fraction` of its elements (at least one of every value) replaced by the special
    values, in order of appearance cyclically, and the bool mask of the replaced elements."""
    a = np.array(a, dtype=np.float32, copy=True)
    rng = np.random.default_rng([seed, a.size])
    k = min(a.size, max(len(values), int(a.size * fraction)))
    at = rng.choice(a.size, size=k, replace=False)
    a.reshape(-1)[at] = np.array(values, dtype=np.float32)[np.arange(k) % len(values)]
    mask = np.zeros(a.shape, bool)
    mask.reshape(-1)[at] = True
    return a, mask

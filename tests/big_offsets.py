"""Id batches for tables whose row offsets pass 32 bits (tests/test_gpu_big_offsets.py), and the element ranges a 32-bit
offset would land in.  Test infrastructure only: nothing under herald_amd/ imports it, and it needs numpy alone.

A table of `rows` x `width` float32 has, per key k, the float offset o = k * width and the byte offset 4 o.  The BANDS of a
table are the key ranges in which these pass a power of two that a narrow type cannot hold:
    band 0   o < 2^30                  every offset fits 32 bits
    band 1   2^30 <= o < 2^31          the byte offset passes 2^32
    band 2   2^31 <= o < 2^32          the float offset passes a signed 32-bit int
    band 3   2^32 <= o                 the float offset passes 32 bits
A table has the bands its last row reaches (T128 and T130 all four, T1 the first two); the last of them is its TOP band.

The ALIAS ranges of a touched key are the `width` elements starting at o mod 2^32, o mod 2^31 and o mod 2^30 (those that
differ from o): where a kernel that computed the float offset, its signed half or the byte offset in 32 bits would read or
write instead.  make_case() accepts a key only if no alias range of any touched key overlaps a touched row, a sentinel row or
row 0, so a test may poison every alias range and find the poison, bit for bit, after the call.

float32 ids: above 2^24 not every integer is a float, so a float32 case takes only multiples of `f32_step` there (4 for keys
below 2^26, 128 below 2^31).  The last row of T1 (2^30 + 2^16 - 1, odd) is no float32: its float32 cases take the last row a
float32 names, rows - 128, and its int64 cases the last row itself."""
import numpy as np

import special_ids


class Table:
    def __init__(self, name, rows, width, f32_step):
        self.name, self.rows, self.width, self.f32_step = name, int(rows), int(width), int(f32_step)

    @property
    def numel(self):
        return self.rows * self.width

    def band_of(self, key):
        o = np.asarray(key, dtype=np.int64) * self.width
        return (o >= 1 << 30).astype(np.int64) + (o >= 1 << 31) + (o >= 1 << 32)

    @property
    def top_band(self):
        return int(self.band_of(self.rows - 1))

    def band_start(self, band):
        """The first key of `band`."""
        return 0 if band == 0 else -(-(1 << (29 + band)) // self.width)

    def band_range(self, band):
        return self.band_start(band), (self.band_start(band + 1) if band < self.top_band else self.rows)

    def last_row(self, dtype):
        """The last row an id of `dtype` can name."""
        last = self.rows - 1
        if dtype == "f32" and last >= 1 << 24:
            last = last // self.f32_step * self.f32_step
        return last

    def dead_ids(self, dtype):
        """Ids that name no row: rows, rows + 4, -1 (float32: the first two floats at or beyond rows)."""
        if dtype == "f32":
            d0 = -(-self.rows // self.f32_step) * self.f32_step
            return [d0, d0 + self.f32_step, -1]
        return [self.rows, self.rows + 4, -1]

    def sentinels(self):
        """Rows no case touches: row 0 (where dead ids are clamped to), its neighbour, the rows around every band start and
        the row before the last one -- all odd or below 2^24 but the band starts, which make_case() refuses anyway."""
        s = {0, 1, self.rows - 2}
        for b in range(1, self.top_band + 1):
            s.update((self.band_start(b) - 1, self.band_start(b) + 1))
        return sorted(s)


T128 = Table("T128", 33762577, 128, 4)
T130 = Table("T130", 33762577, 130, 4)
T1 = Table("T1", (1 << 30) + (1 << 16), 1, 128)
TABLES = {t.name: t for t in (T128, T130, T1)}

NBAGS, BAG = 64, 26
BIG_NBAGS = 1419           # 1,419 x 26 = 36,894 ids > 36,864: the plans and applies switch to their by-unique-key paths
LONG_RUN = 70              # >= 64: the cooperative / LDS / tree class of every apply
SHORT_RUNS = (2, 3, 5, 15)


def alias_starts(table, keys):
    """Element offsets [m] (unique, sorted) of the alias ranges of `keys`: (k * width) mod 2^32, 2^31, 2^30 where that is not
    k * width itself.  Each range is `width` elements long and lies inside the table."""
    o = np.asarray(keys, dtype=np.int64).reshape(-1) * table.width
    out = [o[o >= m] % m for m in (1 << 32, 1 << 31, 1 << 30)]
    return np.unique(np.concatenate(out)) if out else np.empty(0, np.int64)


def rows_of_ranges(table, starts):
    """The rows that the `width`-element ranges at `starts` overlap (unique, sorted)."""
    starts = np.asarray(starts, dtype=np.int64)
    return np.unique(np.concatenate([starts // table.width, (starts + table.width - 1) // table.width]))


def wrapped_offset(table, key, bits, unit="float"):
    """Where a kernel lands that computes the row offset of `key` in `bits` bits: the float offset (unit="float":
    uint32_t(key * width)) or the byte offset (unit="byte": uint32_t(key * width * 4)), as a float offset into the table."""
    o = int(key) * table.width
    if unit == "byte":
        return ((o * 4) % (1 << bits)) // 4
    return o % (1 << bits)


class Case:
    """One id batch.  ids: float32 or int64, [B, F] (fixed bags) or [n] with offsets int64 [B + 1] (ragged); weights float32
    [n] or None.  keys: the sorted unique in-range keys of the batch -- the rows of the compact table (key 0 among them only as
    the dead slot of a weighted case); touched: keys without 0; aliases: alias_starts of touched; sentinels: rows to guard."""

    def __init__(self, table, dtype, layout, weighted, ids, offsets, weights, name):
        self.table, self.dtype, self.layout, self.weighted, self.name = table, dtype, layout, weighted, name
        self.ids, self.offsets, self.weights = ids, offsets, weights
        flat = special_ids.rows_of(ids)
        self.flat_keys = flat
        self.keys = np.unique(flat[flat < table.rows])
        self.touched = self.keys[self.keys != 0]
        self.aliases = alias_starts(table, self.touched)
        self.sentinels = np.array(table.sentinels(), dtype=np.int64)
        self.n = flat.size
        self.nbags = ids.shape[0] if offsets is None else offsets.size - 1
        self.bag = ids.shape[1] if offsets is None else None

    def compact_ids(self):
        """The batch over the compact table of self.keys, int64, shaped as ids: a live key's index in self.keys (searchsorted:
        key order kept), an id at or beyond rows -> keys.size + 5 (still beyond), a negative id -> -1."""
        flat = self.flat_keys
        out = np.searchsorted(self.keys, np.minimum(flat, self.table.rows)).astype(np.int64)
        out[flat >= self.table.rows] = self.keys.size + 5
        raw = np.asarray(self.ids).reshape(-1)
        out[raw < 0] = -1
        return out.reshape(np.asarray(self.ids).shape)

    def which_bag(self):
        if self.offsets is None:
            return np.arange(self.n) // self.bag
        return np.searchsorted(self.offsets, np.arange(self.n), side="right") - 1

    def __repr__(self):
        return self.name


def _snap(table, dtype, k):
    if dtype == "f32" and k >= 1 << 24:
        k = k // table.f32_step * table.f32_step
    return int(k)


class _Picker:
    """Draws keys and keeps the alias rule: a key is accepted when it is no sentinel, lies in no alias range of an accepted key,
    and none of its alias ranges overlaps an accepted key, a sentinel or row 0."""

    def __init__(self, table, dtype, rng):
        self.t, self.dtype, self.rng = table, dtype, rng
        self.taken = set()
        self.alias_rows = set()
        self.guard = set(table.sentinels())

    def accept(self, k):
        t = self.t
        if not 0 < k < t.rows or k in self.taken or k in self.guard or k in self.alias_rows:
            return False
        mine = set(int(r) for r in rows_of_ranges(t, alias_starts(t, [k])))
        if mine & self.taken or mine & self.guard or k in mine:
            return False
        self.taken.add(k)
        self.alias_rows |= mine
        return True

    def draw(self, band, odd=False):
        lo, hi = self.t.band_range(band)
        for _ in range(1000):
            k = int(self.rng.integers(lo, hi))
            k = (k | 1) if odd else _snap(self.t, self.dtype, k)
            if lo <= k < hi and self.accept(k):
                return k
        raise RuntimeError("no free key in band %d of %s" % (band, self.t.name))

    def take(self, k):
        if k in self.taken:          # (a later batch of a stream names the key again)
            return k
        if not self.accept(k):
            raise RuntimeError("key %d of %s breaks the alias rule" % (k, self.t.name))
        return k


def make_case(table, dtype, layout="fixed", weighted=False, big=False, seed=0, picker=None):
    """The batch of one test case (module docstring and Case).  dtype "f32" / "i64", layout "fixed" / "ragged"; big: 36,894 ids
    instead of 1,664, with a run of 400 and the filler drawn with repetition.  picker: the _Picker of a stream of batches
    (make_stream), which keeps the alias rule over all of them."""
    table = TABLES[table] if isinstance(table, str) else table
    name = "%s-%s-%s%s%s" % (table.name, dtype, layout, "-weighted" if weighted else "", "-big" if big else "")
    rng = np.random.default_rng([seed, table.width, dtype == "f32", layout == "fixed", weighted, big])
    nbags = BIG_NBAGS if big else NBAGS
    n = nbags * BAG
    pick = _Picker(table, dtype, rng) if picker is None else picker
    pick.rng = rng
    top = table.top_band
    plan = [(pick.take(table.last_row(dtype)), 1), (pick.draw(top), LONG_RUN)]
    plan += [(pick.draw(top), c) for c in SHORT_RUNS]
    plan += [(pick.draw(top), 1) for _ in range(24)]
    if dtype == "i64":                                   # the int64 twins also use odd keys, beyond any float32
        plan += [(pick.draw(top, odd=True), c) for c in (1, 1, 1, 4)]
    if big:
        plan.append((pick.draw(top), 400))
    for band in range(top):
        plan += [(pick.draw(band), 1) for _ in range(6)] + [(pick.draw(band), 4)]
    dead = table.dead_ids(dtype)
    n_masked = n // 10 if weighted else 0                # the dead slots of a weighted case: id 0, weight 0
    planned = sum(c for _, c in plan)
    fill = n - planned - len(dead) - n_masked
    assert fill > 0
    step = table.f32_step if dtype == "f32" else 1      # (a band with few keys an id can name gets no filler: T1's top band)
    wide = [b for b in range(top + 1) if (table.band_range(b)[1] - table.band_range(b)[0]) // step >= 10000]
    if big:
        pool = [pick.draw(wide[int(rng.integers(0, len(wide)))]) for _ in range(1500)]
        filler = [pool[i] for i in rng.integers(0, len(pool), fill)]
    else:
        filler = [pick.draw(wide[int(rng.integers(0, len(wide)))]) for _ in range(fill)]
    flat = np.array([k for k, c in plan for _ in range(c)] + filler + dead + [0] * n_masked, dtype=np.int64)
    assert flat.size == n
    perm = rng.permutation(n)
    flat = flat[perm]
    weights = None
    if weighted:
        weights = np.ones(n, dtype=np.float32)
        weights[flat == 0] = 0
        live = np.flatnonzero((flat > 0) & (flat < table.rows) & (flat != table.last_row(dtype)))
        odd = rng.choice(live, size=12, replace=False)
        weights[odd] = np.array([0.5, -1.25, 3.0, 0.0], dtype=np.float32)[np.arange(12) % 4]
    ids = flat.astype(np.float32) if dtype == "f32" else flat
    offsets = None
    if layout == "fixed":
        ids = ids.reshape(nbags, BAG)
    else:                                               # an empty first bag, an empty bag inside, the last bag ends on n
        cuts = np.sort(rng.choice(np.arange(1, n), size=nbags - 3, replace=False))
        offsets = np.concatenate([[0, 0], cuts[:nbags // 2], [cuts[nbags // 2 - 1]], cuts[nbags // 2:], [n]]).astype(np.int64)
        assert offsets.size == nbags + 1
    return Case(table, dtype, layout, weighted, ids, offsets, weights, name)


def make_stream(table, dtype, layout="fixed", weighted=False, batches=4, seed=100):
    """`batches` batches, each a case of its own with other keys, drawn by ONE picker: the alias rule holds over all of them.
    -> (union, cases): union is the fixed-bag case of all ids, whose keys / touched / aliases / sentinels describe the table
    while the stream runs (a cache keeps lines of earlier batches and pushes them back later)."""
    table = TABLES[table] if isinstance(table, str) else table
    pick = _Picker(table, dtype, None)
    cases = [make_case(table, dtype, layout, weighted, seed=seed + b, picker=pick) for b in range(batches)]
    ids = np.concatenate([c.ids.reshape(-1) for c in cases]).reshape(-1, BAG)
    weights = np.concatenate([c.weights for c in cases]) if weighted else None
    union = Case(table, dtype, "fixed", weighted, ids, None, weights, cases[0].name + "-stream%d" % batches)
    return union, cases


def check_stream(union, cases):
    """Every batch is a case of its own, shares at most a few keys with the others, and the alias rule holds over the union."""
    t = union.table
    for c in cases:
        check_case(c)
        assert np.isin(c.keys, union.keys).all()
    assert union.keys.size > 0.9 * sum(c.keys.size for c in cases)
    alias_rows = rows_of_ranges(t, union.aliases)
    assert np.intersect1d(alias_rows, union.touched).size == 0
    assert np.intersect1d(alias_rows, union.sentinels).size == 0
    assert np.intersect1d(union.sentinels, union.touched).size == 0


def check_case(case):
    """Every property the GPU tests rely on, asserted (tests/test_big_offsets_cpu.py runs it on every generated case; the GPU
    file runs it again on the cases it uses)."""
    t = case.table
    flat = case.flat_keys
    raw = np.asarray(case.ids).reshape(-1)
    live = flat < t.rows
    if case.weights is not None:
        live &= case.weights != 0
    live_keys = np.unique(flat[live])
    # the float32 ids are exact, the int64 ones use odd keys in the top band
    if case.dtype == "f32":
        assert raw.dtype == np.float32
        assert np.array_equal(raw.astype(np.float64), np.where(raw < 0, -1, flat).astype(np.float64))
        big = flat[(flat >= 1 << 24) & (flat < t.rows)]
        assert big.size and np.all(big % t.f32_step == 0)
    else:
        assert raw.dtype == np.int64
        assert np.any((live_keys % 2 == 1) & (t.band_of(live_keys) == t.top_band) & (live_keys >= 1 << 24))
    # every band of the table is present; the top band holds singletons, short runs, a long run and the last row
    bands = t.band_of(live_keys)
    assert set(bands.tolist()) == set(range(t.top_band + 1))
    if t is not T1:
        assert t.top_band == 3 and (live_keys * t.width >= 1 << 32).any()
    assert (live_keys * t.width * 4 >= 1 << 32).any()
    keys, counts = np.unique(flat[live], return_counts=True)
    topc = counts[t.band_of(keys) == t.top_band]
    assert (topc == 1).sum() >= 8 and ((topc >= 2) & (topc <= 15)).sum() >= 3 and (topc >= 64).any()
    assert t.last_row(case.dtype) in live_keys
    assert t.last_row("i64") == t.rows - 1 and (case.dtype == "f32" or t.rows - 1 in live_keys)
    # dead ids ride along and row 0 is never live
    assert (flat >= t.rows).sum() >= 3 and (raw < 0).any() and 0 not in live_keys
    if case.weights is not None:
        w = case.weights
        assert np.all(w[flat == 0] == 0) and (flat == 0).sum() >= 8 and np.any((w != 0) & (w != 1))
    else:
        assert 0 not in case.keys
    # alias ranges: inside the table, disjoint from touched rows, from sentinels and from row 0
    al = case.aliases
    assert al.size > 0
    assert al.min() >= 0 and al.max() + t.width <= t.numel
    alias_rows = rows_of_ranges(t, al)
    assert np.intersect1d(alias_rows, case.touched).size == 0
    assert np.intersect1d(alias_rows, case.sentinels).size == 0 and 0 in case.sentinels
    assert np.intersect1d(case.sentinels, case.keys[case.keys != 0]).size == 0
    for m in (1 << 32, 1 << 31, 1 << 30):               # (the definition, restated per key)
        o = case.touched * t.width
        assert np.isin(o[o >= m] % m, al).all()
    # the bags
    if case.offsets is not None:
        sizes = np.diff(case.offsets)
        assert case.offsets[0] == 0 and case.offsets[-1] == case.n and (sizes >= 0).all()
        assert (sizes == 0).any() and sizes[-1] > 0
    else:
        assert case.ids.shape == (case.nbags, BAG)
    assert case.n > 36864 if "-big" in case.name else case.n == NBAGS * BAG
    # the compact batch keeps key order and keeps dead ids dead
    cid = case.compact_ids().reshape(-1)
    ok = flat < t.rows
    assert np.array_equal(case.keys[cid[ok]], flat[ok])
    assert np.all((cid[~ok] < 0) | (cid[~ok] >= case.keys.size))


def all_cases():
    """Every case the GPU file uses, by name."""
    out = {}
    for t in ("T128", "T130", "T1"):
        for dtype in ("f32", "i64"):
            for layout in ("fixed", "ragged"):
                for weighted in (False, True):
                    c = make_case(t, dtype, layout, weighted)
                    out[c.name] = c
    for t in ("T128", "T130"):
        for weighted in (False, True):
            c = make_case(t, "f32", "fixed", weighted, big=True)
            out[c.name] = c
    return out

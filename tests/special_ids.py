"""The one id rule (include/herald_amd.h, "Which ids name a row") in numpy, and the special ids the tests feed every id consumer.
Test infrastructure only: nothing under herald_amd/ imports it.

    float32 id f     key = trunc(f) if -1 < f < 4294967295, else DEAD_KEY (NaN of either sign and any payload, f <= -1,
                     f >= 4294967295, both infinities)
    (u)int64 id v    read as uint64; key = v if v <= DEAD_KEY, else DEAD_KEY

DEAD_KEY = 0xFFFFFFFE is >= rows for every table, which is all that makes it dead.  No cast here runs on a value outside the
range of its target type (numpy's float -> integer astype is as undefined there as C's)."""
import numpy as np

DEAD_KEY = 0xFFFFFFFE
INT64_MIN = -2 ** 63


def keys_of(ids):
    """uint64 keys [ids.size] of a float32 or (u)int64 id array, flattened."""
    ids = np.asarray(ids)
    if ids.dtype.kind == "f":
        f = ids.reshape(-1).astype(np.float32)
        with np.errstate(invalid="ignore"):
            live = (f > np.float32(-1.0)) & (f < np.float32(4294967296.0))      # NaN: both False
        keys = np.full(f.size, DEAD_KEY, dtype=np.uint64)
        keys[live] = np.trunc(f[live]).astype(np.uint64)                       # |-0.99| -> -0.0 -> 0; all in [0, 2^32)
        return keys
    if ids.dtype.kind not in "iu":
        raise TypeError("ids must be float32 or (u)int64, not %s" % ids.dtype)
    v = ids.reshape(-1).astype(np.int64 if ids.dtype.kind == "i" else np.uint64).view(np.uint64)
    return np.minimum(v, np.uint64(DEAD_KEY))


def rows_of(ids):
    """keys_of as int64 (every key is below 2^32): what the models index tables with, after checking `< rows`."""
    return keys_of(ids).astype(np.int64)


def nan_with_payload():
    """A quiet NaN with payload bits set, sign bit clear (0x7FC12345)."""
    return np.array([0x7FC12345], dtype=np.uint32).view(np.float32)[0]


def float_specials(rows):
    """[(float32 id, expected key)] of the special list: DEAD ones first, then the live ones."""
    f = np.float32
    neg_nan = np.array([0xFFC00000], dtype=np.uint32).view(np.float32)[0]
    return [
        (f(-1.0), DEAD_KEY), (f(-1.5), DEAD_KEY), (f(-3e9), DEAD_KEY), (f(-np.inf), DEAD_KEY), (f(np.inf), DEAD_KEY),
        (f(3.4e38), DEAD_KEY), (f(np.nan), DEAD_KEY), (neg_nan, DEAD_KEY), (nan_with_payload(), DEAD_KEY),
        (f(4294967296.0), DEAD_KEY), (f(4294967040.0), 0xFFFFFF00), (f(rows), rows),
        (f(-0.0), 0), (f(-0.99), 0), (f(rows - 1), rows - 1), (f(rows - 0.5), rows - 1),
    ]


def int_specials(rows):
    """[(int64 id, expected key)] of the special list; the last one is live."""
    return [
        (-1, DEAD_KEY), (INT64_MIN, DEAD_KEY), (2 ** 63 - 1, DEAD_KEY), (2 ** 32, DEAD_KEY), (2 ** 32 + 5, DEAD_KEY),
        (0xFFFFFFFF, DEAD_KEY), (0xFFFFFFFE, DEAD_KEY), (rows, rows), (rows - 1, rows - 1),
    ]


def replace_dead(ids, rows):
    """The same batch with every id that names no row of a `rows`-row table replaced by rows + 1 (dtype and shape kept)."""
    ids = np.asarray(ids)
    out = ids.copy()
    out.reshape(-1)[keys_of(ids) >= np.uint64(rows)] = rows + 1
    return out

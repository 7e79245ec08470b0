"""The id batches of tests/test_gpu_big_offsets.py (tests/big_offsets.py) hold what the GPU tests rely on: every offset band of
the table, exact float32 ids, the last row, runs of 64 and more, dead ids, and alias ranges -- where a 32-bit offset would land
-- that no touched row, sentinel or row 0 overlaps.  A GPU test can then not pass because its inputs missed the far band."""
import functools

import numpy as np
import pytest

import big_offsets as bo


@functools.lru_cache(maxsize=None)
def _cases():
    return bo.all_cases()


NAMES = sorted(bo.all_cases())


def test_the_tables_are_the_ones_the_issue_names():
    assert (bo.T128.rows, bo.T128.width) == (33762577, 128) and (bo.T130.rows, bo.T130.width) == (33762577, 130)
    assert (bo.T1.rows, bo.T1.width) == ((1 << 30) + (1 << 16), 1)
    assert [bo.T128.band_start(b) for b in (1, 2, 3)] == [1 << 23, 1 << 24, 1 << 25]
    assert bo.T130.band_start(3) == 33038210 and bo.T1.band_start(1) == 1 << 30 and bo.T1.top_band == 1
    assert bo.T128.top_band == 3 and bo.T130.top_band == 3
    assert bo.T128.last_row("f32") == bo.T128.rows - 1                 # 33,762,576 is a multiple of 4
    assert np.float32(bo.T128.rows) == bo.T128.rows - 1                # ... and what float32(rows) rounds to: not a dead id
    for t in bo.TABLES.values():
        for d in t.dead_ids("f32")[:2]:
            assert int(np.float32(d)) == d >= t.rows
    assert len(NAMES) == 28


@pytest.mark.parametrize("name", NAMES)
def test_every_case_holds_what_the_gpu_tests_rely_on(name):
    bo.check_case(_cases()[name])


@pytest.mark.parametrize("name", NAMES)
def test_a_32_bit_offset_lands_in_a_checked_alias_range(name):
    """The teeth of the GPU file, restated: for every touched key, the offset a kernel would compute as uint32_t(key * width),
    int32-truncated (mod 2^31) or as a 32-bit byte offset is either the true offset or the start of a range in case.aliases --
    which the GPU tests poison before the call and compare after it, and which no touched row overlaps, so a read there
    returns poison (the output differs from the model's) and a write there changes poison (and leaves the true row stale)."""
    case = _cases()[name]
    t = case.table
    al = set(case.aliases.tolist())
    touched_elems = set()
    for k in case.touched.tolist():
        touched_elems.add(k * t.width)
    wrapped = 0
    for k in case.touched.tolist():
        o = k * t.width
        for bits, unit in ((32, "float"), (31, "float"), (32, "byte")):
            w = bo.wrapped_offset(t, k, bits, unit)
            if w != o:
                wrapped += 1
                assert w in al and w not in touched_elems
    far = case.touched[t.band_of(case.touched) == t.top_band]
    assert wrapped >= far.size >= 30
    # the run of 64+ and the last row wrap too
    keys, counts = np.unique(case.flat_keys, return_counts=True)
    long_key = int(keys[(counts >= 64) & (keys != 0) & (keys < t.rows)][0])
    for k in (long_key, t.last_row(case.dtype)):
        assert bo.wrapped_offset(t, k, 32, "byte") in al
        if t.top_band == 3:
            assert bo.wrapped_offset(t, k, 32, "float") in al


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dtype,layout", [("f32", "fixed"), ("i64", "ragged")])
def test_streams_of_batches_keep_the_alias_rule_over_all_of_them(dtype, layout, weighted):
    """The cache tests run four batches through one cache, which holds lines of earlier batches and pushes them back later."""
    union, cases = bo.make_stream("T128", dtype, layout, weighted)
    assert len(cases) == 4 and union.n == 4 * bo.NBAGS * bo.BAG
    bo.check_stream(union, cases)
    al = set(union.aliases.tolist())
    for k in union.touched.tolist():
        for bits, unit in ((32, "float"), (31, "float"), (32, "byte")):
            w = bo.wrapped_offset(union.table, k, bits, unit)
            assert w == k * union.table.width or w in al
    # n_pull + n_push of a push-pull step fits the limit the GPU tests use, and the stream overflows it
    assert 2 * cases[0].n <= 3400 < union.keys.size


def test_the_compact_batch_feeds_the_models():
    """compact_ids() keeps key order (searchsorted), keeps dead ids dead and gives the models the rows the kernel reads."""
    import bag_model
    case = _cases()["T128-i64-ragged"]
    rng = np.random.default_rng(0)
    compact = rng.standard_normal((case.keys.size, 4)).astype(np.float32)
    cid = case.compact_ids()
    assert cid.shape == case.ids.shape and cid.min() == -1 and cid.max() == case.keys.size + 5
    out = bag_model.bag_sum(compact, cid, case.offsets)
    assert out.shape == (case.nbags, 4) and np.all(out[0] == 0)          # the first bag is empty
    assert np.all(np.diff(case.keys) > 0)

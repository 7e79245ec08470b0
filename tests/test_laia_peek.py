"""LAIADataloader.peek_arr (herald_amd/laia.py): the (ids, plan) of a batch ahead, for the planned cache flow, without stepping
the scheduler's window -- on a fake native scheduler (tests/test_host_glue.py::_FakeNative), no GPU."""
import numpy as np

from herald_amd import laia as hlaia
from test_host_glue import _scheduler


def _loaders(monkeypatch, batches=20, dataset_num=2):
    s, fake = _scheduler(batches=batches, dataset_num=dataset_num, monkeypatch=monkeypatch)
    raw = np.arange(200 * 3, dtype=np.float32).reshape(200, 3)      # (the fake's dist(b) names samples b and b + 100)
    sparse = hlaia.LAIADataloader(s, 0, True, raw, 10)
    dense = hlaia.LAIADataloader(s, 1, False, raw, 10)
    for dl in (sparse, dense):
        dl.init_states(0, 1)
    return s, fake, sparse, dense


def test_peek_returns_the_objects_get_next_arr_and_get_arr_return_later(monkeypatch):
    s, fake, sparse, dense = _loaders(monkeypatch)
    ahead = [sparse.peek_arr(j) for j in range(3)]
    assert all(isinstance(a, tuple) for a in ahead)
    assert sparse.peek_arr(0) is sparse.get_next_arr() is ahead[0]
    for j in range(3):
        nxt = sparse.get_next_arr()
        assert nxt is ahead[j]
        got = sparse.get_arr()
        dense.get_arr()
        assert got is ahead[j] and got[0] is ahead[j][0] and got[1] is ahead[j][1]
        # (the window pairs dist(b) with plan(b + 1): the fake's dist(b) = [b, b + 100], plan(b + 1) = [1001 + b])
        np.testing.assert_array_equal(got[1], np.array([1001 + j], dtype=np.float32))
        np.testing.assert_array_equal(got[0], sparse.raw_data[[j, j + 100]])
    assert sparse.peek_arr(1) is sparse.peek_arr(1)
    p = sparse.peek_arr(1)
    sparse.get_arr()
    dense.get_arr()
    assert sparse.get_next_arr() is p


def test_peek_beyond_the_window_is_none(monkeypatch):
    s, fake, sparse, dense = _loaders(monkeypatch)
    w = s.WINDOW
    assert sparse.peek_arr(w - 1) is not None
    assert sparse.peek_arr(w) is None and sparse.peek_arr(w + 3) is None
    # the other loader has not moved: the window cannot move either, however far this one gets
    for _ in range(2):
        sparse.get_arr()
    assert sparse.peek_arr(w - 3) is not None and sparse.peek_arr(w - 2) is None


def test_peek_never_steps_the_window_nor_blocks(monkeypatch):
    s, fake, sparse, dense = _loaders(monkeypatch)
    pops, window, cursor = fake.pops, dict(s._window), list(s._cursor)
    fake.ready = 0                       # the scheduler has nothing computed: a blocking pop would assert
    for j in range(8):
        sparse.peek_arr(j)
        dense.peek_arr(j)
    assert fake.pops == pops and s._window == window and s._cursor == cursor
    assert sparse.batch_index == 0 and dense.batch_index == 0


def test_dense_loader_peeks_its_rows(monkeypatch):
    s, fake, sparse, dense = _loaders(monkeypatch)
    r = dense.peek_arr(1)
    assert isinstance(r, np.ndarray)
    np.testing.assert_array_equal(r, dense.raw_data[np.asarray(s.get_input_index_array(1))])
    dense.get_arr()
    assert dense.get_arr() is r

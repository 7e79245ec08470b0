"""bench.py's command line without a GPU: a plain run implies every --no-* option, --full restores them, and
dump_outputs writes what it is given as float32 / float64 arrays within 64 MB, sampled the same way every time."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402

SECONDARY = ("no_cpu_baseline", "no_kernel_pass", "no_cache_tier", "no_laia", "no_config_c", "no_wide", "no_sweeps",
             "no_cold_tier")


def _args(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return bench.parse_args()


def test_plain_run_implies_every_no_option_and_full_restores_them(monkeypatch):
    a = _args(monkeypatch, "--gpus", "1", "--steps", "20", "--warmup", "5")
    assert not a.full and a.steps == 20 and a.warmup == 5 and a.dump_outputs is None
    assert all(getattr(a, k) for k in SECONDARY)
    f = _args(monkeypatch, "--full", "--no-laia", "--dump-outputs", "out")
    assert f.full and f.no_laia and f.dump_outputs == "out"
    assert not any(getattr(f, k) for k in SECONDARY if k != "no_laia")


def _load(d, name):
    return np.load(os.path.join(str(d), name + ".npy"))


def test_dump_outputs_writes_the_rows_and_the_updated_table_rows(tmp_path):
    g = torch.Generator().manual_seed(0)
    table = torch.randn((5000, 16), generator=g)
    rows = torch.randn((300, 16), generator=g)
    applied = np.array([7, 7, 4999, 12, 0], dtype=np.float32)
    bench.dump_outputs(str(tmp_path), rows, table, applied)
    assert np.array_equal(_load(tmp_path, "lookup_rows"), rows.numpy())
    assert np.array_equal(_load(tmp_path, "lookup_positions"), np.arange(300, dtype=np.float64))
    ids = _load(tmp_path, "table_row_ids")
    assert ids.dtype == np.float64 and np.all(np.diff(ids) > 0) and set([0, 7, 12, 4999]) <= set(ids.tolist())
    assert np.array_equal(_load(tmp_path, "table_rows"), table.numpy()[ids.astype(np.int64)])
    # a shard: global ids, only the shard's own rows of the batch
    bench.dump_outputs(str(tmp_path / "s"), rows, table[1000:2000], np.array([5, 1500, 2500], dtype=np.float32),
                       id_offset=1000)
    sid = _load(tmp_path / "s", "table_row_ids")
    assert 1500 in sid and 5 not in sid and 2500 not in sid and sid.min() >= 1000 and sid.max() < 2000
    assert np.array_equal(_load(tmp_path / "s", "table_rows"), table.numpy()[sid.astype(np.int64)])


def test_dump_outputs_samples_large_outputs_the_same_way_every_time(tmp_path):
    width = 128
    rows = torch.arange(106496 * width, dtype=torch.float32).view(106496, width)      # 54.5 MB: sampled
    table = torch.zeros((200000, width))
    applied = np.arange(0, 200000, 2, dtype=np.float32)                               # 100,000 updated rows: sampled
    total = 0
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), rows, table, applied)
    for name in ("lookup_rows", "lookup_positions", "table_rows", "table_row_ids"):
        a, b = _load(tmp_path / "a", name), _load(tmp_path / "b", name)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), name
        total += a.nbytes
    assert total <= 64 << 20
    pos = _load(tmp_path / "a", "lookup_positions").astype(np.int64)
    assert 0 < pos.size < 106496 and np.all(np.diff(pos) > 0)
    assert np.array_equal(_load(tmp_path / "a", "lookup_rows"), rows.numpy()[pos])

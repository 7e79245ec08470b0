"""The apply launch's geometry: the wave items dealt over an odd number of worker workgroups (wave wv of worker b takes the
items (r * 16 + wv) * nworker + b) behind the workgroups reserved for the G items.  Every stream is
compared bit for bit with the one-launch-per-step model (tests/test_gpu_qstep.py's _run_stream); the item counts the cases
are built around are read back from the queues."""
import numpy as np
import pytest
import torch

from herald_amd import ops, synth
from test_gpu_qstep import _dev, _run_stream

pytestmark = pytest.mark.gpu
WPW = 16        # waves per workgroup of the apply launch


def _stream(dev, table0, batches, lr=0.03, seed=1, **kw):
    rng = np.random.default_rng(seed)
    grads = [rng.standard_normal((b.size, table0.shape[1]), dtype=np.float32) for b in batches]
    return _run_stream(dev, table0, batches, grads, lr, check_plans=False, **kw)


def _items(pipe, c):
    h = pipe.queue_header(c)
    return h["wave_items"] + h["copy_items"], h["workgroup_items"]


@pytest.mark.parametrize("hinted", [True, False], ids=["hinted", "unhinted"])
def test_fewer_items_than_workgroups(dev, monkeypatch, hinted):
    """40 ids at d = 512 on 1,000 rows (a handful of workgroups, most waves without an item), and 4,096 ids over 40 keys: the
    unhinted launch is sized by the ids, and all but 39 of its workgroups find nothing."""
    if not hinted:
        monkeypatch.setenv("HA_QHINT", "0")
    rng = np.random.default_rng(3)
    table0 = rng.standard_normal((1000, 512), dtype=np.float32)
    _stream(dev, table0, [rng.integers(0, 1000, size=40) for _ in range(4)], mode=(True, 2))
    keys = rng.choice(1000, size=40, replace=False)
    few = [rng.permutation(np.r_[keys, np.full(4096 - 40, keys[0])]) for _ in range(4)]      # 40 keys, one of them a G key
    pipe = _stream(dev, table0, few, mode=(True, 8, "flags"))
    n_items, _ = _items(pipe, 1)
    _, nworker = ops.qapply_geometry(512, 4096, 4096)
    assert n_items == 39 and (hinted or nworker > 8 * n_items), (n_items, nworker)


@pytest.mark.parametrize("hinted", [True, False], ids=["hinted", "unhinted"])
@pytest.mark.parametrize("k,off", [(1, -1), (1, 0), (1, 1), (2, -1), (2, 0), (2, 1)])
def test_item_counts_around_multiples_of_the_grid(dev, monkeypatch, k, off, hinted):
    """nworker * k - 1, nworker * k and nworker * k + 1 wave items for the grid of an unhinted launch: the last round of the
    deal is one item short, exact, and one item into the next.  (n ids = that many keys once each + one G key for the rest: a
    G key makes workgroup items only.)  Hinted, the same queues run on the few workgroups their items fill."""
    if not hinted:
        monkeypatch.setenv("HA_QHINT", "0")
    n, rows, width = 4096, 1200, 512
    _, nworker = ops.qapply_geometry(width, n, n)
    assert nworker > 1 and nworker % 2 == 1, "an odd number of workers keeps apply and copy items alternating"
    target = nworker * k + off
    assert target + 64 <= n and target < rows
    rng = np.random.default_rng(100 * k + off)
    table0 = rng.standard_normal((rows, width), dtype=np.float32)
    batches = [rng.permutation(np.r_[np.arange(target), np.full(n - target, rows - 1)]) for _ in range(3)]
    pipe = _stream(dev, table0, batches, mode=(True, 8, "flags"))
    for c in (0, 1):
        assert _items(pipe, c)[0] == target, (_items(pipe, c), target)


@pytest.mark.parametrize("width", [1024, 2048])
def test_more_items_than_resident_waves(dev, width):
    """7,168 ids at d = 1024 / 2048: more wave items than 16 x nworker, every wave loops."""
    n, rows = 7168, 9000
    rng = np.random.default_rng(width)
    table0 = rng.standard_normal((rows, width), dtype=np.float32)
    batches = [rng.integers(0, rows, size=n) for _ in range(3)]
    pipe = _stream(dev, table0, batches, mode=(True, 8, "flags"))
    _, nworker = ops.qapply_geometry(width, n, n, _items(pipe, 0)[0])
    assert _items(pipe, 0)[0] > WPW * nworker


@pytest.mark.parametrize("gkeys", [0, 1, 8, 9])
def test_g_region_beside_the_dealt_workers(dev, gkeys):
    """0, 1, 8 and 9 keys of 64 occurrences at d = 512 = 0, 8, 64 and 72 workgroup items on the 64 reserved G workgroups in
    front of the workers: none with an item, a few, all, and eight that take a second one."""
    n, rows, width = 1024, 3000, 512
    rng = np.random.default_rng(gkeys)
    table0 = rng.standard_normal((rows, width), dtype=np.float32)
    batches = []
    for _ in range(3):
        hot = np.repeat(rng.choice(100, size=gkeys, replace=False), 64)
        cold = rng.choice(np.arange(100, rows), size=n - hot.size, replace=False)
        batches.append(rng.permutation(np.r_[hot, cold]))
    pipe = _stream(dev, table0, batches, mode=(True, 8, "flags"))
    assert _items(pipe, 1)[1] == 8 * gkeys
    assert ops.qapply_geometry(width, n, n)[0] == 64


@pytest.mark.parametrize("hinted", [True, False], ids=["hinted", "unhinted"])
@pytest.mark.parametrize("width", [64, 128])
def test_narrow_rows_with_an_odd_number_of_items(dev, monkeypatch, width, hinted):
    """d <= 128: a wave takes a PAIR of items, dealt like the items of wider rows; 1,001 keys once each, 300 of them new from
    batch to batch = 1,001 wave items + 300 copies, the last pair has one item."""
    if not hinted:
        monkeypatch.setenv("HA_QHINT", "0")
    rows, u = 2000, 1001
    rng = np.random.default_rng(width)
    table0 = rng.standard_normal((rows, width), dtype=np.float32)
    batches = [rng.permutation((np.arange(u) + 300 * (k % 2)) % rows) for k in range(4)]
    pipe = _stream(dev, table0, batches, mode=(True, 8, "flags"))
    assert _items(pipe, 0)[0] == u + 300


def test_workgroups_are_equally_filled_and_mixed(dev):
    """The census of one launch (per wave: start, end, role, its first item) on a Criteo-shaped batch: worker workgroups
    differ by at most one busy wave, and every one with two items or more holds an apply item and a copy."""
    rows, width, bs, block = 100_000, 512, 256, 2
    rng = np.random.default_rng(41)
    table = _dev(rng.standard_normal((rows, width), dtype=np.float32) * np.float32(0.01), dev)
    n = synth.criteo_batch(bs, 0, rows=rows).size
    pipe = ops.QueueStepPipeline(table, n, 1e-3, block=block)
    LA, stamp = pipe.LOOKAHEAD, 1
    ids = [torch.from_numpy(np.minimum(synth.as_f32_ids(synth.criteo_batch(bs, b, rows=rows)).reshape(-1), rows - 1)).to(dev)
           for b in range(stamp + 2 + LA + 2 * block)]
    grads = _dev(rng.standard_normal((n, width), dtype=np.float32), dev)
    out = torch.empty((n, width), device=dev)
    ncoop, nworker = ops.qapply_geometry(width, n, n)
    dbg = torch.zeros((ncoop + nworker) * WPW * 4, dtype=torch.int64, device=dev)
    for c in range(-LA, stamp + 1):
        if c % block == 0:
            pipe.prepare_block(c // block, lambda j: ids[j] if 0 <= j < len(ids) else None)
        if c >= -1:
            pipe.apply(c, grads if c >= 0 else None, out, dbg=dbg if c == stamp else None)
    torch.cuda.synchronize()
    n_items, _ = _items(pipe, stamp)
    d = dbg.cpu().numpy().reshape(ncoop + nworker, WPW, 4)
    assert (d[:, :, 0] > 0).all(), "every wave of the grid left its stamps"
    assert ((d[:ncoop, :, 2] & 0xFF) == 0).all() and ((d[ncoop:, :, 2] & 0xFF) == 3).all()
    rec = d[ncoop:, :, 3]
    busy = (rec & 0xFF) < 15                       # the wave had an item (its kind)
    copy = busy & (((rec >> 8) & 0xFFFFF) == 0)    # no occurrences to apply: a copy item
    per_wg = busy.sum(axis=1)
    assert per_wg.sum() == min(n_items, WPW * nworker) and n_items > 2 * nworker
    assert per_wg.max() - per_wg.min() <= 1, (per_wg.min(), per_wg.max())
    mixed = (copy.sum(axis=1) > 0) & ((busy & ~copy).sum(axis=1) > 0)
    assert mixed[per_wg >= 2].all()

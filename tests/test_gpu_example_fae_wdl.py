"""examples/ctr/run_wdl.py --model fae_wdl (the reference's fae_wdl_criteo: the most frequent ids are served by a small dense
hot table, every other id by the main table through embedding_lookup_op, mul_op by the 0/1 mask of the cold ids and
reduce_sum_op(axes=1)) against the single-table emb_sum_wdl loop in plain PyTorch ops.  The hot table starts as a copy of the
main table's hot rows, so the FAE model IS that single-table model mathematically: the main table's cold rows are compared with
the reference table, the hot table with the reference table's rows at the hot ids.  The cold half runs on the weighted sum-pooled
lookup (ha_gather_wsum_*) and the fused weighted apply (ha_sgd_sparse_update_wbags_*); the hot half on torch's embedding_bag.

PyTorch sums a bag in its own order and sums the gradients of duplicate ids before the update, so the runs agree within
rounding: sizes and tolerances are those of tests/test_gpu_example_emb_sum.py, except the length of the run and the hot rate
(0.01 of 30,000 rows: 300 hot ids).  The PyTorch loop below run on the CPU in float32 and in float64 differs, after 2 / 3 / 4 /
5 / 6 / 8 / 12 steps, by 4.2e-8 / 6.6e-8 / 7.1e-8 / 8.5e-8 / 1.15e-7 / 1.67e-7 / 2.39e-7 absolute in the table (atol 5e-7: a fifth
is 1e-7), by 1.3e-7 relative in the losses at every length (rtol 1e-4) and by 3.3e-9 .. 1.2e-8 absolute in the tower's weights
(atol 1e-7): the table's gap passes a fifth of its tolerance at 6 steps, so the run is 3 steps, where the gaps are 1.3e-7, 6.6e-8
and 4.9e-9 (the tolerances are not widened).  test_the_tolerances_fit_this_model measures the gaps anew on the GPU, prints them
and holds each to a fifth of its tolerance; on the MI355X they were 1.0e-7, 7.5e-8 and 4.6e-9."""
import gc
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "ctr"))

pytestmark = pytest.mark.gpu

ROWS, WIDTH, BATCH, STEPS, LR, HOT_RATE = 30000, 16, 128, 3, 0.05, 0.01      # (3 steps: see the docstring)
RTOL = 1e-5     # north_star tolerance for accumulated fp32 gradients
ATOL = 5e-7     # table values are ~1e-2: entries that cancel to ~0 have no meaningful relative error


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    """What this module created and only the cyclic collector frees (operators that hold their configs, stores, plans) is
    collected here, with the device idle -- not at some later allocation inside another module's gated or timed call, where a
    finalizer that frees device memory would wait for that module's stream."""
    yield
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def torch_reference(dev, table_init, dtype=torch.float32):
    """The single-table emb_sum_wdl loop in plain PyTorch ops, in float32 or float64; returns (losses, table, tower)."""
    import run_wdl
    tower = run_wdl.make_tower("emb_sum_wdl", WIDTH, 0).to(dev).to(dtype)
    table = table_init.clone().to(dtype)
    opt = torch.optim.SGD(tower.parameters(), lr=LR)
    batches = run_wdl.make_batches(min(STEPS + 1, 64), BATCH, ROWS, 0)
    losses = []
    for k in range(STEPS):
        ids, dense, label = (torch.from_numpy(a).to(dev) for a in batches[k % len(batches)])
        idx = ids.long()
        emb = table[idx].clone().requires_grad_(True)
        pred = tower(dense.to(dtype), emb.sum(1))
        loss = torch.nn.functional.binary_cross_entropy(pred, label.to(dtype))
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        table.index_add_(0, idx.reshape(-1), emb.grad.reshape(-1, WIDTH), alpha=-LR)
        losses.append(float(loss.detach()))
    return losses, table, tower


@pytest.fixture(scope="module")
def reference(dev):
    g = torch.Generator(device=dev).manual_seed(1)
    table_init = torch.randn((ROWS, WIDTH), generator=g, device=dev) * 0.01
    return table_init, torch_reference(dev, table_init)


def test_fae_wdl_training_matches_the_single_table_model_in_pytorch(dev, reference):
    import run_wdl
    table_init, (ref_losses, ref_table, ref_tower) = reference
    losses, param, tower = run_wdl.train("hbm", ROWS, WIDTH, BATCH, STEPS, LR, table_init=table_init, device=str(dev),
                                         model="fae_wdl", fae_hot_rate=HOT_RATE)
    assert isinstance(tower, run_wdl.SumTower) and tower.W4.shape == (256 + WIDTH, 1)
    hot = param.hot_ids
    assert hot.numel() == int(HOT_RATE * ROWS) == 300 and param.hot_table.shape == (300, WIDTH)
    # the hot list: the most frequent ids of the run's batches, ties to the smaller id
    batches = run_wdl.make_batches(min(STEPS + 1, 64), BATCH, ROWS, 0)
    counts = np.bincount(np.concatenate([b[0].reshape(-1) for b in batches]).astype(np.int64), minlength=ROWS)
    order = sorted(range(ROWS), key=lambda i: (-counts[i], i))[:300]
    assert hot.cpu().tolist() == order
    np.testing.assert_allclose(losses, ref_losses, rtol=1e-4)
    cold = torch.ones(ROWS, dtype=torch.bool, device=dev)
    cold[hot] = False
    torch.testing.assert_close(param.table[cold], ref_table[cold], rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(param.hot_table.detach(), ref_table[hot], rtol=RTOL, atol=ATOL)
    for p, q in zip(tower.parameters(), ref_tower.parameters()):
        torch.testing.assert_close(p, q, rtol=1e-4, atol=1e-7)
    # hot ids occur in the main table's batches as dead occurrences only: their rows keep their initial bits
    assert torch.equal(param.table[hot].view(torch.int32), table_init[hot].view(torch.int32))
    # both tables must have changed elsewhere
    assert not torch.equal(param.table[cold], table_init[cold]) and not torch.equal(param.hot_table.detach(), table_init[hot])
    assert not torch.equal(ref_table[cold], table_init[cold]) and not torch.equal(ref_table[hot], table_init[hot])


def test_the_split_of_a_batch():
    import run_wdl
    ids = np.array([[5, 7, 0, 9], [7, 7, 3, 5]], dtype=np.float32)
    hot = np.array([7, 0], dtype=np.int64)                         # rank 1: id 7, rank 2: id 0
    rank, cold_ids, cold_mask = run_wdl.fae_split(ids, hot)
    assert rank.tolist() == [[0, 1, 2, 0], [1, 1, 0, 0]]
    assert cold_ids.dtype == np.float32 and cold_ids.tolist() == [[5, 0, 0, 9], [0, 0, 3, 5]]
    assert cold_mask.dtype == np.float32 and cold_mask.tolist() == [[1, 0, 0, 1], [0, 0, 1, 1]]
    # ties go to the smaller id
    batches = [(np.array([[4, 2, 2, 9, 4, 1]], dtype=np.float32),)]
    assert run_wdl.fae_hot_ids(batches, 10, 0.3).tolist() == [2, 4, 1]


def test_the_tolerances_fit_this_model(dev, reference):
    """The float32 PyTorch loop against the float64 one: each gap at least 5 times below the tolerance it stands for."""
    table_init, (l32, t32, w32) = reference
    l64, t64, w64 = torch_reference(dev, table_init, torch.float64)
    gap_loss = float(np.max(np.abs(np.array(l32) - np.array(l64)) / np.abs(np.array(l64))))
    gap_table = float((t32.double() - t64).abs().max())
    gap_tower = max(float((p.detach().double() - q.detach()).abs().max()) for p, q in zip(w32.parameters(), w64.parameters()))
    print("fae_wdl float32 vs float64: losses %.2e relative, table %.2e absolute, tower %.2e absolute"
          % (gap_loss, gap_table, gap_tower))
    assert 5 * gap_loss <= 1e-4
    assert 5 * gap_table <= ATOL
    assert 5 * gap_tower <= 1e-7


def test_the_aliases_name_the_model():
    import run_wdl
    assert run_wdl.MODEL_ALIASES["fae_wdl_criteo"] == "fae_wdl"
    assert "fae_wdl" in run_wdl.FAE_MODELS
    assert run_wdl.make_tower("fae_wdl", 8).W4.shape == (256 + 8, 1)


@pytest.mark.parametrize("embedding", ["queue", "cache", "ps", "step", "step3"])
def test_other_embeddings_refuse_fae_wdl(dev, embedding):
    import run_wdl
    with pytest.raises(ValueError, match="fae_wdl"):
        run_wdl.train(embedding, 2000, 16, 8, 2, 0.05, device=str(dev), model="fae_wdl")


@pytest.mark.parametrize("optimizer", ["momentum", "adam"])
def test_the_other_optimizers_run_through_the_expansion(dev, optimizer):
    """Not fused: the weighted slices are expanded (hetu_ops.unweighted_slices) and the optimizer runs as on any unpooled
    gradient; the main table changes and stays finite."""
    import run_wdl
    g = torch.Generator(device=dev).manual_seed(3)
    table_init = torch.randn((2000, 16), generator=g, device=dev) * 0.01
    losses, param, _ = run_wdl.train("hbm", 2000, 16, 16, 2, 0.05, table_init=table_init, device=str(dev), model="fae_wdl",
                                     optimizer=optimizer, fae_hot_rate=0.01)
    assert len(losses) == 2 and np.isfinite(losses).all()
    assert bool(torch.isfinite(param.table).all()) and not torch.equal(param.table, table_init)


def test_an_unknown_optimizer_is_refused_for_fae_wdl(dev):
    import run_wdl
    with pytest.raises(ValueError, match="optimizer"):
        run_wdl.train("hbm", 2000, 16, 8, 2, 0.05, device=str(dev), model="fae_wdl", optimizer="lamb")

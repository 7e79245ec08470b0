"""examples/ctr/run_wdl.py --model fae_deepfm (the reference's fae_deepfm_avazu: the most frequent ids are served by small dense
hot tables, every other id by the main tables through embedding_lookup_op and mul_op by the 0/1 mask of the cold ids; the
second-order rows are consumed as reduce_sum_op(x) and reduce_sum_op(x * x), and the square of the sum is taken after the hot
table's half has been added) against the single-table emb_sum_deepfm loop in plain PyTorch ops.  The hot tables start as copies of
the main tables' hot rows, so the FAE model IS that single-table model mathematically: the main tables' cold rows are compared with
the reference tables, the hot tables with the reference tables' rows at the hot ids.  The cold half of the second-order term runs
on the weighted FM-pooled lookup (ha_gather_wfm_*) and its fused apply (ha_sgd_sparse_update_wfm_bags_*), the cold half of the
first-order term on the weighted bags at width 1; the hot halves on torch's embedding_bag.

PyTorch sums a bag in its own order and sums the gradients of duplicate ids before the update, so the runs agree within
rounding: sizes and tolerances are those of tests/test_gpu_example_emb_sum_deepfm.py, except the length of the run and the hot
rate (0.01 of 30,000 rows: 300 hot ids).  The PyTorch loop below run on the CPU in float32 and in float64 differs, after
2 / 4 / 6 / 8 / 12 steps, by 6.0e-8 / 6.0e-8 / 6.0e-8 / 6.0e-8 / 7.5e-8 relative in the losses (rtol 1e-4), by 2.1e-8 / 3.2e-8 /
3.6e-8 / 3.9e-8 / 4.4e-8 absolute in the second-order table and 1.0e-8 / 1.5e-8 / 1.9e-8 / 3.7e-8 / 3.5e-8 in the first-order one
(atol 5e-7: a fifth is 1e-7) and by 3.5e-9 / 5.8e-9 / 7.2e-9 / 9.9e-9 / 1.5e-8 absolute in the tower's weights (atol 1e-7: a fifth
is 2e-8).  Every length up to 12 keeps each gap below a fifth of its tolerance on the CPU; the same loop on the GPU sums in
another order (tests/test_gpu_example_emb_sum_deepfm.py reports 8.2e-8 for the second-order table at 8 steps there), so the run is
6 steps, which leaves room on both (the tolerances are not widened).
test_the_tolerances_fit_this_model measures the gaps anew on the GPU, prints them and holds each to a fifth of its tolerance; on
the MI355X they were 4.9e-8, 6.2e-8 / 8.8e-9 and 6.4e-9 at 6 steps."""
import gc
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "ctr"))

pytestmark = pytest.mark.gpu

ROWS, WIDTH, BATCH, STEPS, LR, HOT_RATE = 30000, 16, 128, 6, 0.05, 0.01     # (the length of the run: see the docstring)
RTOL = 1e-5     # north_star tolerance for accumulated fp32 gradients
ATOL = 5e-7     # table values are ~1e-2: entries that cancel to ~0 have no meaningful relative error


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    """What this module created and only the cyclic collector frees is collected here, with the device idle."""
    yield
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def torch_reference(dev, table_init, first_init, dtype=torch.float32, steps=None):
    """The single-table emb_sum_deepfm loop in plain PyTorch ops, in float32 or float64; returns (losses, second-order table,
    first-order table, tower)."""
    import run_wdl
    steps = STEPS if steps is None else steps
    tower = run_wdl.make_tower("emb_sum_deepfm", WIDTH, 0).to(dev).to(dtype)
    table, first = table_init.clone().to(dtype), first_init.clone().to(dtype)
    opt = torch.optim.SGD(tower.parameters(), lr=LR)
    batches = run_wdl.make_batches(min(steps + 1, 64), BATCH, ROWS, 0)
    losses = []
    for k in range(steps):
        ids, dense, label = (torch.from_numpy(a).to(dev) for a in batches[k % len(batches)])
        idx = ids.long()
        emb = table[idx].clone().requires_grad_(True)              # [B, 26, d]
        one = first[idx].clone().requires_grad_(True)              # [B, 26, 1]
        total = emb.sum(1)
        fm = 0.5 * (total * total - (emb * emb).sum(1))
        pred = tower(dense.to(dtype), total, one.sum(1), fm)
        loss = torch.nn.functional.binary_cross_entropy(pred, label.to(dtype))
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        table.index_add_(0, idx.reshape(-1), emb.grad.reshape(-1, WIDTH), alpha=-LR)
        first.index_add_(0, idx.reshape(-1), one.grad.reshape(-1, 1), alpha=-LR)
        losses.append(float(loss.detach()))
    return losses, table, first, tower


def initial_tables(dev):
    g = torch.Generator(device=dev).manual_seed(1)
    table_init = torch.randn((ROWS, WIDTH), generator=g, device=dev) * 0.01
    first_init = torch.randn((ROWS, 1), generator=g, device=dev) * 0.01
    return table_init, first_init


def gaps(ref32, ref64):
    """(losses relative, second-order table, first-order table, tower absolute) between two runs of torch_reference."""
    (l32, t32, f32, w32), (l64, t64, f64, w64) = ref32, ref64
    gap_loss = float(np.max(np.abs(np.array(l32) - np.array(l64)) / np.abs(np.array(l64))))
    gap_table = float((t32.double() - t64.double()).abs().max())
    gap_first = float((f32.double() - f64.double()).abs().max())
    gap_tower = max(float((p.detach().double() - q.detach().double()).abs().max())
                    for p, q in zip(w32.parameters(), w64.parameters()))
    return gap_loss, gap_table, gap_first, gap_tower


@pytest.fixture(scope="module")
def reference(dev):
    table_init, first_init = initial_tables(dev)
    return table_init, first_init, torch_reference(dev, table_init, first_init)


def test_fae_deepfm_training_matches_the_single_table_model_in_pytorch(dev, reference):
    import run_wdl
    table_init, first_init, (ref_losses, ref_table, ref_first, ref_tower) = reference
    losses, param, tower = run_wdl.train("hbm", ROWS, WIDTH, BATCH, STEPS, LR, table_init=table_init, device=str(dev),
                                         model="fae_deepfm", first_order_init=first_init, fae_hot_rate=HOT_RATE)
    assert isinstance(tower, run_wdl.SumFMTower) and tower.FM_W.shape == (13, 1) and tower.W1.shape == (WIDTH, 256)
    first = param.first_order
    hot = param.hot_ids
    assert hot.numel() == int(HOT_RATE * ROWS) == 300 and torch.equal(first.hot_ids, hot)
    assert param.hot_table.shape == (300, WIDTH) and first.hot_table.shape == (300, 1)
    assert param.table.shape == (ROWS, WIDTH) and first.table.shape == (ROWS, 1)
    # the hot list and the split are fae_wdl's: fae_hot_ids over the run's batches
    batches = run_wdl.make_batches(min(STEPS + 1, 64), BATCH, ROWS, 0)
    assert hot.cpu().tolist() == run_wdl.fae_hot_ids(batches, ROWS, HOT_RATE).tolist()
    np.testing.assert_allclose(losses, ref_losses, rtol=1e-4)
    cold = torch.ones(ROWS, dtype=torch.bool, device=dev)
    cold[hot] = False
    torch.testing.assert_close(param.table[cold], ref_table[cold], rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(first.table[cold], ref_first[cold], rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(param.hot_table.detach(), ref_table[hot], rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(first.hot_table.detach(), ref_first[hot], rtol=RTOL, atol=ATOL)
    for p, q in zip(tower.parameters(), ref_tower.parameters()):
        torch.testing.assert_close(p, q, rtol=1e-4, atol=1e-7)
    # hot ids occur in the main tables' batches as dead occurrences only: their rows keep their initial bits
    assert torch.equal(param.table[hot].view(torch.int32), table_init[hot].view(torch.int32))
    assert torch.equal(first.table[hot].view(torch.int32), first_init[hot].view(torch.int32))
    # both tables must have changed elsewhere, and so must both hot tables
    assert not torch.equal(param.table[cold], table_init[cold]) and not torch.equal(first.table[cold], first_init[cold])
    assert not torch.equal(param.hot_table.detach(), table_init[hot]) and not torch.equal(first.hot_table.detach(), first_init[hot])
    assert not torch.equal(ref_table[cold], table_init[cold]) and not torch.equal(ref_table[hot], table_init[hot])
    assert not torch.equal(ref_first[cold], first_init[cold]) and not torch.equal(ref_first[hot], first_init[hot])


def test_the_tolerances_fit_this_model(dev, reference):
    """The float32 PyTorch loop against the float64 one: each gap at least 5 times below the tolerance it stands for."""
    table_init, first_init, ref32 = reference
    gap_loss, gap_table, gap_first, gap_tower = gaps(ref32, torch_reference(dev, table_init, first_init, torch.float64))
    print("fae_deepfm float32 vs float64: losses %.2e relative, tables %.2e / %.2e absolute, tower %.2e absolute"
          % (gap_loss, gap_table, gap_first, gap_tower))
    assert 5 * gap_loss <= 1e-4
    assert 5 * gap_table <= ATOL and 5 * gap_first <= ATOL
    assert 5 * gap_tower <= 1e-7


def test_the_aliases_name_the_model():
    import run_wdl
    assert run_wdl.MODEL_ALIASES["fae_deepfm_avazu"] == run_wdl.MODEL_ALIASES["fae_dfm_avazu"] == "fae_deepfm"
    assert "fae_deepfm" in run_wdl.FAE_FM_MODELS
    assert "fae_deepfm" not in run_wdl.FAE_MODELS + run_wdl.FM_MODELS      # it has its own loop and its own refusals
    assert isinstance(run_wdl.make_tower("fae_deepfm", 8), run_wdl.SumFMTower)


def test_the_split_is_the_one_fae_wdl_uses():
    import run_wdl
    ids = np.array([[5, 7, 0, 9], [7, 7, 3, 5]], dtype=np.float32)
    rank, cold_ids, cold_mask = run_wdl.fae_split(ids, np.array([7, 0], dtype=np.int64))
    assert rank.tolist() == [[0, 1, 2, 0], [1, 1, 0, 0]]
    assert cold_ids.tolist() == [[5, 0, 0, 9], [0, 0, 3, 5]] and cold_mask.tolist() == [[1, 0, 0, 1], [0, 0, 1, 1]]


def test_no_hot_ids_at_all_is_the_cold_path_alone(dev):
    """Hot rate 0: empty hot tables, every occurrence live on the main tables; the run is finite and changes both tables."""
    import run_wdl
    g = torch.Generator(device=dev).manual_seed(3)
    table_init = torch.randn((2000, 16), generator=g, device=dev) * 0.01
    losses, param, _ = run_wdl.train("hbm", 2000, 16, 16, 2, 0.05, table_init=table_init, device=str(dev), model="fae_deepfm",
                                     fae_hot_rate=0.0)
    assert len(losses) == 2 and np.isfinite(losses).all() and param.hot_table.shape == (0, 16)
    assert bool(torch.isfinite(param.table).all()) and not torch.equal(param.table, table_init)


@pytest.mark.parametrize("embedding", ["queue", "cache", "ps", "step", "step3"])
def test_other_embeddings_refuse_fae_deepfm(dev, embedding):
    import run_wdl
    with pytest.raises(ValueError, match="fae_deepfm"):
        run_wdl.train(embedding, 2000, 16, 8, 2, 0.05, device=str(dev), model="fae_deepfm")


@pytest.mark.parametrize("optimizer", ["momentum", "nesterov", "adagrad", "adam", "adamw"])
def test_other_optimizers_refuse_fae_deepfm(dev, optimizer):
    import run_wdl
    with pytest.raises(ValueError, match="fae_deepfm"):
        run_wdl.train("hbm", 2000, 16, 8, 2, 0.05, device=str(dev), model="fae_deepfm", optimizer=optimizer)

"""examples/ctr/run_wdl.py --model emb_sum_deepfm (the reference's emb_sum_deepfm_avazu: a first-order table of width 1 summed
over a sample's 26 ids, and a second-order table whose lookup is consumed only as the sum S -- the DNN's input and S*S -- and as
the sum of squares Q, combined into 0.5 * (S*S - Q)) against the same training loop in plain PyTorch ops, with both tables in
HBM: the FM-pooled lookup without rows and the ONE fused apply of its whole backward (ha_sgd_sparse_update_fm_bags_*) for the
second-order table, the width-1 sum-pooled lookup and the bag apply for the first-order one.

PyTorch sums a bag in its own order and sums the gradients of duplicate ids before the update, so the runs agree within
rounding: sizes and tolerances are those of tests/test_gpu_example_deepfm.py, except the length of the run.  The PyTorch loop
below run once in float32 and once in float64 (torch_reference's dtype) differs, after that file's 12 steps, by 8.2e-8 relative in
the losses (rtol here 1e-4), by 1.04e-7 / 1.6e-8 absolute in the two tables (atol 5e-7) and by 9.0e-9 absolute in the tower's
weights (atol 1e-7): the second-order table's gap is 4.8 times below its tolerance, not 5, so the run is 8 steps, where the gaps
are 4.9e-8, 8.2e-8 / 1.4e-8 and 7.9e-9 -- each more than 5 times below the tolerance it stands for (the tolerances are not
widened).  test_the_tolerances_fit_this_model measures the gaps anew, prints them and holds each to a fifth of its tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "ctr"))

pytestmark = pytest.mark.gpu

ROWS, WIDTH, BATCH, STEPS, LR = 30000, 16, 128, 8, 0.05      # (8 steps, not that file's 12: see the docstring)
RTOL = 1e-5     # north_star tolerance for accumulated fp32 gradients
ATOL = 5e-7     # table values are ~1e-2: entries that cancel to ~0 have no meaningful relative error


def torch_reference(dev, table_init, first_init, dtype=torch.float32):
    """The same loop in plain PyTorch ops, in float32 or float64; returns (losses, second-order table, first-order table,
    tower)."""
    import run_wdl
    tower = run_wdl.make_tower("emb_sum_deepfm", WIDTH, 0).to(dev).to(dtype)
    table, first = table_init.clone().to(dtype), first_init.clone().to(dtype)
    opt = torch.optim.SGD(tower.parameters(), lr=LR)
    batches = run_wdl.make_batches(min(STEPS + 1, 64), BATCH, ROWS, 0)
    losses = []
    for k in range(STEPS):
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


@pytest.fixture(scope="module")
def reference(dev):
    table_init, first_init = initial_tables(dev)
    return table_init, first_init, torch_reference(dev, table_init, first_init)


def test_emb_sum_deepfm_training_matches_pytorch(dev, reference):
    import run_wdl
    table_init, first_init, (ref_losses, ref_table, ref_first, ref_tower) = reference
    losses, param, tower = run_wdl.train("hbm", ROWS, WIDTH, BATCH, STEPS, LR, table_init=table_init, device=str(dev),
                                         model="emb_sum_deepfm", first_order_init=first_init)
    assert isinstance(tower, run_wdl.SumFMTower) and tower.FM_W.shape == (13, 1) and tower.W1.shape == (WIDTH, 256)
    assert tower.W2.shape == (256, 256) and tower.W3.shape == (256, 1)
    assert param.table.shape == (ROWS, WIDTH) and param.first_order.table.shape == (ROWS, 1)
    np.testing.assert_allclose(losses, ref_losses, rtol=1e-4)
    torch.testing.assert_close(param.table, ref_table, rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(param.first_order.table, ref_first, rtol=RTOL, atol=ATOL)
    for p, q in zip(tower.parameters(), ref_tower.parameters()):
        torch.testing.assert_close(p, q, rtol=1e-4, atol=1e-7)
    # both tables must have changed
    assert not torch.equal(param.table, table_init) and not torch.equal(param.first_order.table, first_init)
    assert not torch.equal(ref_table, table_init) and not torch.equal(ref_first, first_init)


def test_the_tolerances_fit_this_model(dev, reference):
    """The float32 PyTorch loop against the float64 one: each gap at least 5 times below the tolerance it stands for."""
    table_init, first_init, (l32, t32, f32, w32) = reference
    l64, t64, f64, w64 = torch_reference(dev, table_init, first_init, torch.float64)
    gap_loss = float(np.max(np.abs(np.array(l32) - np.array(l64)) / np.abs(np.array(l64))))
    gap_table = float((t32.double() - t64).abs().max())
    gap_first = float((f32.double() - f64).abs().max())
    gap_tower = max(float((p.detach().double() - q.detach()).abs().max()) for p, q in zip(w32.parameters(), w64.parameters()))
    print("emb_sum_deepfm float32 vs float64: losses %.2e relative, tables %.2e / %.2e absolute, tower %.2e absolute"
          % (gap_loss, gap_table, gap_first, gap_tower))
    assert 5 * gap_loss <= 1e-4
    assert 5 * gap_table <= ATOL and 5 * gap_first <= ATOL
    assert 5 * gap_tower <= 1e-7


def test_the_aliases_name_the_model():
    import run_wdl
    assert run_wdl.MODEL_ALIASES["emb_sum_deepfm_avazu"] == run_wdl.MODEL_ALIASES["emb_sum_dfm_avazu"] == "emb_sum_deepfm"
    assert "emb_sum_deepfm" in run_wdl.FM_MODELS


@pytest.mark.parametrize("embedding", ["queue", "cache", "ps", "step", "step3"])
def test_other_embeddings_refuse_emb_sum_deepfm(dev, embedding):
    import run_wdl
    with pytest.raises(ValueError, match="emb_sum_deepfm"):
        run_wdl.train(embedding, 2000, 16, 8, 2, 0.05, device=str(dev), model="emb_sum_deepfm")


def test_other_optimizers_refuse_emb_sum_deepfm(dev):
    import run_wdl
    with pytest.raises(ValueError, match="emb_sum_deepfm"):
        run_wdl.train("hbm", 2000, 16, 8, 2, 0.05, device=str(dev), model="emb_sum_deepfm", optimizer="adam")

"""examples/ctr/run_wdl.py --model emb_sum_wdl --optimizer O on --embedding hbm: the pooled model's embedding table trained
with AdaGrad, Adam and Nesterov momentum straight from the pooled gradient (opt_fuse_bags=True: ha_sparse_opt_fused_bags_*,
ha_momentum_sparse_update_bags_*) against the reference's own sequence for the same optimizer (opt_fuse_bags=False: the
expanded gradient, deduplicate, the reference-named symbol) -- identical losses, bit-equal tables."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "ctr"))

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("optimizer", ["adagrad", "adam", "nesterov"])
def test_pooled_model_trains_with_the_optimizer_from_the_pooled_gradient(dev, optimizer):
    import run_wdl
    g = torch.Generator(device=dev).manual_seed(1)
    table_init = torch.randn((2000, 16), generator=g, device=dev) * 0.01
    runs = []
    for fuse in (True, False):
        losses, param, _ = run_wdl.train(model="emb_sum_wdl", embedding="hbm", rows=2000, width=16, batch=32, steps=8,
                                         optimizer=optimizer, opt_fuse_bags=fuse, table_init=table_init, device=str(dev))
        runs.append((losses, param.table.cpu().numpy()))
    (l1, t1), (l0, t0) = runs
    assert len(l1) == 8 and np.all(np.isfinite(l1)) and np.all(np.isfinite(l0))
    assert l1 == l0
    np.testing.assert_array_equal(t1.view(np.uint32), t0.view(np.uint32))
    assert np.all(np.isfinite(t1))
    assert not np.array_equal(t1, table_init.cpu().numpy())          # the table must have changed


def test_other_engines_refuse_an_embedding_optimizer(dev):
    import run_wdl
    with pytest.raises(ValueError, match="--embedding hbm only"):
        run_wdl.train(model="emb_sum_wdl", embedding="queue", rows=2000, width=16, batch=32, steps=8, optimizer="adam",
                      device=str(dev))
    with pytest.raises(ValueError, match="--embedding hbm only"):
        run_wdl.train(model="wdl", embedding="queue", rows=2000, width=16, batch=32, steps=2, optimizer="adam",
                      device=str(dev))

"""examples/ctr/run_wdl.py --embedding ps --model emb_sum_wdl: the pooled pull and push of the sharded store
(ps_fuse_bags=True, the default) against the unfused path of the same loop (--no-ps-fuse-bags: per-occurrence rows, the
gradient expanded before the push) -- losses exactly equal, the store's table bit-equal."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "ctr"))

pytestmark = pytest.mark.gpu


def test_emb_sum_wdl_on_the_ps_fused_equals_unfused(dev):
    import run_wdl
    runs = {}
    for fuse in (True, False):
        losses, param, _ = run_wdl.train("ps", 2000, 16, 8, 5, 0.05, device=str(dev), model="emb_sum_wdl", ps_fuse_bags=fuse)
        torch.cuda.synchronize()
        runs[fuse] = (losses, param.store.table.cpu().numpy().copy())
    assert runs[True][0] == runs[False][0]
    assert np.array_equal(runs[True][1].view(np.int32), runs[False][1].view(np.int32))
    g = torch.Generator(device=dev).manual_seed(1)
    init = (torch.randn((2000, 16), generator=g, device=dev) * 0.01).cpu().numpy()
    assert not np.array_equal(runs[True][1].view(np.int32), init.view(np.int32))      # the table was trained
    assert len(runs[True][0]) == 5 and all(np.isfinite(runs[True][0]))

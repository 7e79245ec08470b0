"""examples/ctr/run_wdl.py --embedding cache --cache lru --cache-planned at the default --bsp -1: the asp-with-prefetch schedule
through the cache's planned push-pull chain gives the losses and the store table of the call-by-call run, bit for bit.  More
steps than the loader's ring holds batches (64), so that a key tensor comes round again inside one chain; the chain is still
open when training ends (one step's bookkeeping planned ahead and never run), which must be harmless."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "ctr"))

pytestmark = pytest.mark.gpu


def test_wdl_asp_planned_chain_equals_call_by_call(dev):
    import run_wdl
    rows, width, batch, steps = 20000, 16, 32, 70
    g = torch.Generator(device=dev).manual_seed(5)
    table_init = torch.randn((rows, width), generator=g, device=dev) * 0.01
    out = {}
    for planned in (False, True):
        losses, param, _ = run_wdl.train(embedding="cache", rows=rows, width=width, batch=batch, steps=steps, lr=0.05, cache="LRU",
                                         bound=2, cache_limit=4 * batch * run_wdl.NFIELD, seed=0, device=str(dev),
                                         table_init=table_init, bsp=-1, cache_planned=planned)
        torch.cuda.synchronize()
        out[planned] = (np.array(losses), param.store.table.cpu().numpy().copy())
        del param
    assert np.all(np.isfinite(out[True][0]))
    np.testing.assert_array_equal(out[True][0], out[False][0])
    np.testing.assert_array_equal(out[True][1], out[False][1])
    assert not np.array_equal(out[True][1], table_init.cpu().numpy())      # (something was pushed)

"""ParameterServerCommunicateOp(bag=26) + EmbeddingLookUpSum + EmbeddingLookUpSum_Gradient on the plain PS flavour (a world-1
sharded store): with Config.ps_fuse_bags the op pulls pooled rows (store.pull_sum) and pushes the pooled gradient
(store.push_bags) on every schedule -- ssp and asp with prefetch, and without prefetch, where the lookup pulls pooled rows
itself (ragged bags too).  The yardstick is the same three training steps with ps_fuse_bags=False (per-occurrence rows, a
summing pass, the expanded gradient): pooled outputs and tables are bit-equal after every step.  That the fusion is in effect
is shown by counters on store.pull, store.push and IndexedSlices.expanded_values, which stay at zero in the fused run."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bag_model  # noqa: E402

from herald_amd import hetu_ops, ops  # noqa: E402
from herald_amd.sharded import ShardedEmbedding  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS, WIDTH, B, F, LR, STEPS = 3000, 32, 24, 26, 0.05, 3
_EXPANDED_VALUES = ops.IndexedSlices.expanded_values      # the method itself: every run wraps it afresh


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


_shared = {}


def _inputs():
    """Table, id batches, gradients and ragged offsets: built once, shared by every run, never written."""
    if not _shared:
        rng = np.random.default_rng(77)
        _shared["table"] = rng.standard_normal((ROWS, WIDTH)).astype(np.float32)
        ids = rng.integers(0, ROWS, (STEPS + 2, B, F)).astype(np.float32)
        ids[:, :, 0] = 11                               # a key in every bag: a run of B occurrences
        ids[:, 2, :] = ids[:, 2, :1]                    # a bag of one key
        _shared["ids"] = ids
        _shared["grads"] = rng.standard_normal((STEPS, B, WIDTH)).astype(np.float32)
        cuts = np.sort(rng.integers(0, B * F + 1, B - 4))
        h = cuts.size // 2
        _shared["offsets"] = np.concatenate([[0, 0], cuts[:h], [cuts[h]], cuts[h:], [B * F, B * F]]).astype(np.int64)
    return _shared


def _train(dev, schedule, fuse, monkeypatch):
    """Three steps; returns (pooled outputs, tables after each step, counters, the communicate op)."""
    inp = _inputs()
    store = ShardedEmbedding(ROWS, WIDTH, dev, table=torch.from_numpy(inp["table"]).to(dev))
    calls = {"pull": 0, "push": 0, "expanded_values": 0}

    def counted(name, fn):
        def wrapper(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return wrapper

    store.pull = counted("pull", store.pull)
    store.push = counted("push", store.push)
    monkeypatch.setattr(ops.IndexedSlices, "expanded_values", counted("expanded_values", _EXPANDED_VALUES))
    param = hetu_ops.EmbeddingParameter(store=store)
    d_ids = [torch.from_numpy(a).to(dev) for a in inp["ids"]]
    d_off = torch.from_numpy(inp["offsets"]).to(dev)
    cfg = hetu_ops.Config(comm_mode="PS", bsp=0 if schedule == "ssp" else -1, prefetch=schedule != "none", ps_fuse_bags=fuse)
    state = {"k": 0}
    comm = hetu_ops.ParameterServerCommunicateOp(param, LR, next_ids=lambda: d_ids[state["k"] + 1], bag=F)
    comm.forward_hook(cfg, first_ids=d_ids[0])
    look = hetu_ops.EmbeddingLookUpSum(param)
    look.forward_hook(cfg)
    look_grad = hetu_ops.EmbeddingLookUpSum_Gradient(param.shape)
    outs, tables = [], []
    for k in range(STEPS):
        state["k"] = k
        ragged = schedule == "none" and k == 1          # without prefetch the lookup itself pulls: ragged bags too
        out = torch.full((B, WIDTH), -7.0, dtype=torch.float32, device=dev)
        g = torch.from_numpy(inp["grads"][k]).to(dev)   # (scaled in place by the op: a copy per run)
        if ragged:
            flat = d_ids[k].reshape(-1)
            look.compute(flat, out, offsets=d_off)
            grad = look_grad.compute(g, flat, offsets=d_off)
        else:
            look.compute(d_ids[k], out)
            grad = look_grad.compute(g, d_ids[k])
        assert grad.pooled
        comm.compute(grad)
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy().copy())
        tables.append(store.table.cpu().numpy().copy())
    for a, b in zip(d_ids, inp["ids"]):
        assert np.array_equal(_bits(a), _bits(b))       # inputs as they were
    return outs, tables, calls, comm


@pytest.mark.parametrize("schedule", ["ssp", "asp", "none"])
def test_ps_fuse_bags_equals_the_unfused_schedule_bit_for_bit(dev, monkeypatch, schedule):
    inp = _inputs()
    f_outs, f_tables, f_calls, f_comm = _train(dev, schedule, True, monkeypatch)
    u_outs, u_tables, u_calls, u_comm = _train(dev, schedule, False, monkeypatch)
    for k in range(STEPS):
        assert np.array_equal(_bits(f_outs[k]), _bits(u_outs[k])), (schedule, k)
        assert np.array_equal(_bits(f_tables[k]), _bits(u_tables[k])), (schedule, k)
        assert not np.array_equal(_bits(f_tables[k]), _bits(f_tables[k - 1] if k else inp["table"]))
    # the first pooled rows come from the initial table: the restatement
    assert np.array_equal(_bits(f_outs[0]), _bits(bag_model.bag_sum(inp["table"], inp["ids"][0])))
    # the fusion is in effect: no per-occurrence pull, no per-occurrence push, no expanded gradient
    assert f_calls == {"pull": 0, "push": 0, "expanded_values": 0}, f_calls
    assert u_calls["pull"] > 0 and u_calls["push"] == STEPS and u_calls["expanded_values"] == STEPS, u_calls
    if schedule != "none":
        assert f_comm.sparse_pull_val.shape == (B, WIDTH)
        assert u_comm.sparse_pull_val.shape == (B, F, WIDTH)
        assert f_comm.config.ps_pooled[f_comm.parameter] == F and not u_comm.config.ps_pooled


def test_ps_fuse_bags_needs_the_bag_size(dev):
    """Without bag= the op is today's on every path, whatever ps_fuse_bags says; with it, ids of another shape are refused."""
    inp = _inputs()
    d_ids = torch.from_numpy(inp["ids"][0]).to(dev)
    store = ShardedEmbedding(ROWS, WIDTH, dev, table=torch.from_numpy(inp["table"]).to(dev))
    param = hetu_ops.EmbeddingParameter(store=store)
    cfg = hetu_ops.Config(comm_mode="PS", bsp=0, prefetch=True, ps_fuse_bags=True)
    comm = hetu_ops.ParameterServerCommunicateOp(param, LR, next_ids=lambda: d_ids)
    comm.forward_hook(cfg, first_ids=d_ids)
    assert comm._bag is None and comm.sparse_pull_val.shape == (B, F, WIDTH) and not cfg.ps_pooled
    comm = hetu_ops.ParameterServerCommunicateOp(param, LR, next_ids=lambda: d_ids, bag=F)
    with pytest.raises(ValueError, match="ids must be"):
        comm.forward_hook(hetu_ops.Config(comm_mode="PS", bsp=0, prefetch=True), first_ids=d_ids.reshape(-1))

#!/usr/bin/env python3
"""Wide & Deep on Criteo-shaped data with the embedding path on herald_amd (MI355X).

The model is the reference's examples/ctr/models/wdl_criteo.py:8-46 (33,762,577 x d embedding table,
26 sparse fields, 13 dense features, a 13-256-256-256 tower, one 256+26d -> 1 output layer, sigmoid +
binary cross entropy, SGD on every parameter).  The dense tower runs on PyTorch-ROCm; everything that
touches the embedding table goes through the operator mirrors of herald_amd.hetu_ops, i.e. through
libherald_amd.so, in the three placements the reference's run_hetu.py offers:

  --embedding hbm    table in this GPU's HBM: EmbeddingLookUp -> DLGpuEmbeddingLookUp,
                     sparse SGD -> SGDOptimizerSparseUpdate           (comm_mode None)
  --embedding step   as hbm, but ONE launch per training step: ha_sgd_push_pull applies the sparse SGD of batch
                     k and looks batch k+1 up (rows both batches touch handed over inside the launch)
  --embedding queue  the work-queue step (ops.QueueStepPipeline / ha_qapply, what bench.py times): plans and queues a block
                     of steps ahead beside the model, long runs as fixed-order tree sums (1e-5 tolerance)
  --embedding step3  the same step through ops.StepPipeline (ha_step_*): ids three batches ahead, updated rows
                     forwarded to the next batch's output by the applying waves, nothing waits inside the launch
  --embedding ps     row-range sharded store (one shard per rank): SparsePull / SparsePush through
                     ParameterServerCommunicateOp                     (comm_mode PS; torchrun for N > 1)
  --embedding cache  HET cache (LRU / LFU / LFUOpt, bounded staleness) in front of the store
                     (comm_mode Hybrid + --cache POLICY --bound B, run_hetu.py:178-190).  With --cache-planned on one rank
                     the cache's bookkeeping runs a batch ahead: at --bsp 0 as planned lookup + update pairs, at the
                     default --bsp -1 (asp, --cache lru) as the planned push-pull chain, one cache call per step.

  --laia             the reference's run_laia.py loop (examples/ctr/run_laia.py:214-236): every rank runs the laia
                     scheduler over the whole sample set (herald_amd.laia.LAIAScheduler: LaiaScheduler, or with
                     --local-shared the TopkScheduler whose local rank 0 feeds the others through shared-memory rings),
                     three LAIADataloaders (sparse ids, labels, dense features) hand it ITS share of each global batch,
                     the sparse one as the tuple (ids, push plan); the rows come through the HET cache over the table
                     row-sharded across the ranks, EmbeddingLookUp_Gradient(enable_push_index=True) turns the plan into
                     IndexedSlices.push_indices and the communicate op pushes with embedding_update_with_push_keys;
                     the dense tower's gradients are all-reduced (Hybrid).  torchrun for N > 1.  With
                     --cache-planned on one rank the cache runs its planned flow: the batch after next and its plan are
                     booked ahead (LAIADataloader.peek_arr), every lookup and every push-plan update is one launch.
  --model emb_sum_wdl  the pooled Wide & Deep (examples/ctr/models/emb_sum_wdl_criteo.py): a sample's 26 rows are summed into one
                     before the tower (embedding_lookup_op + reduce_sum_op(axes=1)).  --embedding hbm: the fused sum-pooled
                     lookup (ha_gather_sum_*) and the bag apply (ha_sgd_apply_bags) -- neither [B, 26, d] nor the expanded
                     gradient is built; --embedding ps: pooled as well -- the sharded store sums a sample's rows out of the
                     unique rows it received (pull_sum, ha_gather_sum_u32keys) and reduces the [B, d] gradient by unique key
                     as it is (push_bags, ha_dedup_reduce_bags); what crosses the fabric is unchanged (--no-ps-fuse-bags:
                     per-occurrence rows, the gradient expanded before the push; the same bits); cache: per-occurrence
                     rows as before, summed in the same order, the pooled gradient expanded before the push -- except
                     --embedding cache --cache-planned, where the cache's planned flow is pooled as well: the pairs at
                     --bsp 0 (ha_cache_lookup_sum_planned / ha_cache_update_planned_bags) and, at the default --bsp -1 with
                     --cache lru, the push-pull chain (ha_cache_push_pull_planned_bags).  The step engines refuse the model.
  --optimizer        the embedding table's optimizer on --embedding hbm: sgd (default), momentum, nesterov, adagrad, adam or adamw
                     with the reference's default hyper-parameters (python/hetu/optimizer.py:232-483); the states live beside
                     the table.  A pooled model's gradient goes to the optimizer pooled as well (ha_sparse_opt_fused_bags_*,
                     ha_momentum_sparse_update_bags_*).  The dense tower keeps SGD.  Every other engine runs sparse SGD only.
  --model deepfm     DeepFM (examples/ctr/models/deepfm_criteo.py): a first-order table [rows, 1] read through the sum-pooled
                     lookup at width 1 and updated by the bag apply, and a second-order table [rows, d] whose one lookup feeds
                     the DNN (rows), the sum S and the sum of squares Q -- the fused FM-pooled lookup (ha_gather_fm_*) writes
                     rows, S and 0.5 * (S*S - Q) in one pass, ha_fm_grad_rows combines the gradients of the rows and of the FM
                     output into one per-occurrence gradient for the ordinary sparse SGD.  --embedding hbm, --optimizer sgd.
  --model emb_sum_deepfm  the pooled DeepFM (examples/ctr/models/emb_sum_deepfm_avazu.py; also emb_sum_deepfm_avazu,
                     emb_sum_dfm_avazu): the second-order lookup is consumed only as S (the DNN's input and S*S) and Q, so the
                     lookup writes no rows (ha_gather_fm_* with out_rows NULL) and its whole backward is ONE fused apply
                     (ha_sgd_sparse_update_fm_bags_*): no [batch * 26, d] tensor in the step.  --embedding hbm, --optimizer sgd.
  --model fae_wdl    the FAE Wide & Deep (examples/ctr/models/fae_wdl_criteo.py; also fae_wdl_criteo): the --fae-hot-rate most
                     frequent ids of the run are served by a small dense table that trains with the tower (its half of a sample's
                     sum: torch's embedding_bag with per-sample weights), every other id by the main table through the WEIGHTED
                     sum-pooled lookup (ha_gather_wsum_*: the slot of a hot id is the padding id 0 with weight 0) and, with
                     --optimizer sgd, the fused weighted apply (ha_sgd_sparse_update_wbags_*: the dead slots leave the plan as
                     one out-of-range key); the other optimizers take the weighted gradient expanded.  --embedding hbm; --embedding ps
                     with --ps-fuse-wbags; --embedding cache with --cache-planned --bsp 0 --cache-fuse-wbags (the reference's
                     hybrid_fae_wdl_criteo.sh: the cold table behind the HET cache, ha_cache_lookup_wsum_planned /
                     ha_cache_update_planned_wbags).
  --model fae_deepfm the FAE DeepFM (examples/ctr/models/fae_deepfm_avazu.py; also fae_deepfm_avazu, fae_dfm_avazu): fae_wdl's hot
                     list and split over the DeepFM's two tables.  The first-order table is the weighted bag at width 1; the
                     second-order table goes through the WEIGHTED FM-pooled lookup (ha_gather_wfm_*: S and Q of the cold rows,
                     separately, because the square of the sum is taken after the hot table's half has been added) and ONE fused
                     apply (ha_sgd_sparse_update_wfm_bags_*): no [batch * 26, d] tensor in the step.  Both tables have a hot
                     table that trains with the tower.  --embedding hbm, --optimizer sgd.
  --model dcn        Deep & Cross (examples/ctr/models/dcn_criteo.py:8-74; the reference hard-codes d = 128 there, the
                     embedding width is a parameter here) instead of Wide & Deep.

Data is synthetic (herald_amd.synth: per-field zipf over the public Criteo cardinalities); labels come
from a fixed random linear rule so that the loss has something to learn.

    python examples/ctr/run_wdl.py --embedding hbm --rows 2000000 --width 128 --steps 200
    torchrun --nproc-per-node 4 --master-addr 127.0.0.1 examples/ctr/run_wdl.py --laia --model dcn --width 128
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch

from herald_amd import hetu_ops, synth
from herald_amd.sharded import ShardedEmbedding

NFIELD, NDENSE = 26, 13


class Tower(torch.nn.Module):
    """The dense part of wdl_criteo (models/wdl_criteo.py:19-36); weights ~ N(0, 0.01) like init.random_normal."""

    def __init__(self, width, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)

        def w(*shape):
            return torch.nn.Parameter(torch.randn(*shape, generator=g) * 0.01)
        self.W1, self.W2, self.W3 = w(NDENSE, 256), w(256, 256), w(256, 256)
        self.W4 = w(256 + NFIELD * width, 1)

    def forward(self, dense, emb_flat):
        y3 = torch.relu(torch.relu(dense @ self.W1) @ self.W2) @ self.W3
        return torch.sigmoid(torch.cat([emb_flat, y3], dim=1) @ self.W4)


class CrossTower(torch.nn.Module):
    """The dense part of dcn_criteo (models/dcn_criteo.py:8-74): x0 = [embeddings | dense features], three cross
    layers x_{l+1} = x0 * (x_l w_l) + x_l + b_l, a 3-layer DNN on x0, one output layer over [cross | dnn]; every
    weight ~ N(0, 0.01)."""

    def __init__(self, width, seed=0, layers=3):
        super().__init__()
        g = torch.Generator().manual_seed(seed)

        def w(*shape):
            return torch.nn.Parameter(torch.randn(*shape, generator=g) * 0.01)
        n = NFIELD * width + NDENSE
        self.cw = torch.nn.ParameterList([w(n, 1) for _ in range(layers)])
        self.cb = torch.nn.ParameterList([w(n) for _ in range(layers)])
        self.W1, self.W2, self.W3 = w(n, 256), w(256, 256), w(256, 256)
        self.W4 = w(256 + n, 1)

    def forward(self, dense, emb_flat):
        x0 = torch.cat([emb_flat, dense], dim=1)
        x1 = x0
        for cw, cb in zip(self.cw, self.cb):
            x1 = x0 * (x1 @ cw) + x1 + cb
        y3 = torch.relu(torch.relu(x0 @ self.W1) @ self.W2) @ self.W3
        return torch.sigmoid(torch.cat([x1, y3], dim=1) @ self.W4)


class SumTower(Tower):
    """The dense part of emb_sum_wdl_criteo (models/emb_sum_wdl_criteo.py:18-35): the 26 embedding rows of a sample arrive
    summed into one, so W4 is [256 + width, 1] and y4 = cat(pooled, y3)."""

    def __init__(self, width, seed=0):
        super().__init__(width, seed)
        g = torch.Generator().manual_seed(seed + 4)
        self.W4 = torch.nn.Parameter(torch.randn(256 + width, 1, generator=g) * 0.01)


class FMTower(torch.nn.Module):
    """The dense part of deepfm_criteo (models/deepfm_criteo.py:13-52): FM_W [13, 1] for the first-order dense part and the DNN
    26d-256-256-1 over the flattened second-order rows; every weight ~ N(0, 0.01).  forward(dense, emb_flat [B, 26 d],
    first [B, 1] = the sum of a sample's first-order weights, fm [B, d] = 0.5 * (S*S - Q)):
    y = sigmoid(y1 + y2 + y3) with y1 = dense @ FM_W + first, y2 = fm.sum(1, keepdim) and y3 the DNN's output."""

    def __init__(self, width, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)

        def w(*shape):
            return torch.nn.Parameter(torch.randn(*shape, generator=g) * 0.01)
        self.FM_W = w(NDENSE, 1)
        self.W1, self.W2, self.W3 = w(NFIELD * width, 256), w(256, 256), w(256, 1)

    def forward(self, dense, emb_flat, first, fm):
        y1 = dense @ self.FM_W + first
        y2 = fm.sum(1, keepdim=True)
        y3 = torch.relu(torch.relu(emb_flat @ self.W1) @ self.W2) @ self.W3
        return torch.sigmoid((y1 + y2) + y3)


class FMLookup(torch.autograd.Function):
    """EmbeddingLookUpFM and EmbeddingLookUpFM_Gradient as one autograd node: forward returns the rows [B, 26, d] and the FM
    output [B, d] of one fused lookup; backward hands the gradients of both to the gradient operator, which combines them with
    the forward's rows and sum into the per-occurrence gradient (in place over the rows' gradient) and leaves the
    IndexedSlices in `sink`.  `anchor` is a scalar that requires grad: the table is no autograd leaf, the node needs one."""

    @staticmethod
    def forward(ctx, anchor, ids, lookup, lookup_grad, sink):
        batch, width = ids.shape[0], lookup.embedding.shape[1]
        rows = torch.empty((batch, NFIELD, width), dtype=torch.float32, device=ids.device)
        total = torch.empty((batch, width), dtype=torch.float32, device=ids.device)
        fm = torch.empty((batch, width), dtype=torch.float32, device=ids.device)
        lookup.compute(ids, rows, total, fm)
        ctx.save_for_backward(ids, rows, total)
        ctx.lookup_grad, ctx.sink = lookup_grad, sink
        return rows, fm

    @staticmethod
    def backward(ctx, g_rows, g_fm):
        ids, rows, total = ctx.saved_tensors
        ctx.sink["grad"] = ctx.lookup_grad.compute(g_rows.contiguous(), g_fm.contiguous(), rows, total, ids)
        return None, None, None, None, None


class SumFMTower(torch.nn.Module):
    """The dense part of emb_sum_deepfm_avazu (models/emb_sum_deepfm_avazu.py; the same shape in fae_deepfm_avazu.py): FM_W
    [13, 1] for the first-order dense part and the DNN d-256-256-1 over S, the SUM of a sample's second-order rows; every
    weight ~ N(0, 0.01).  forward(dense, total [B, d] = S, first [B, 1], fm [B, d] = 0.5 * (S*S - Q)):
    y = sigmoid((y1 + y2) + y3) as FMTower."""

    def __init__(self, width, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)

        def w(*shape):
            return torch.nn.Parameter(torch.randn(*shape, generator=g) * 0.01)
        self.FM_W = w(NDENSE, 1)
        self.W1, self.W2, self.W3 = w(width, 256), w(256, 256), w(256, 1)

    def forward(self, dense, total, first, fm):
        y1 = dense @ self.FM_W + first
        y2 = fm.sum(1, keepdim=True)
        y3 = torch.relu(torch.relu(total @ self.W1) @ self.W2) @ self.W3
        return torch.sigmoid((y1 + y2) + y3)


class FMSumLookup(torch.autograd.Function):
    """EmbeddingLookUpFMSum and EmbeddingLookUpFMSum_Gradient as one autograd node: forward returns S [B, d] and the FM output
    [B, d] of one fused lookup that writes no rows; backward wraps the gradients of both with S as FM-pooled IndexedSlices in
    `sink` -- nothing [B * 26, d] is saved or built.  `anchor` as in FMLookup."""

    @staticmethod
    def forward(ctx, anchor, ids, lookup, lookup_grad, sink):
        batch, width = ids.shape[0], lookup.embedding.shape[1]
        total = torch.empty((batch, width), dtype=torch.float32, device=ids.device)
        fm = torch.empty((batch, width), dtype=torch.float32, device=ids.device)
        lookup.compute(ids, total, fm)
        ctx.save_for_backward(ids, total)
        ctx.lookup_grad, ctx.sink = lookup_grad, sink
        return total, fm

    @staticmethod
    def backward(ctx, g_total, g_fm):
        ids, total = ctx.saved_tensors
        ctx.sink["grad"] = ctx.lookup_grad.compute(g_total.contiguous(), g_fm.contiguous(), total, ids)
        return None, None, None, None, None


class WeightedFMSumLookup(torch.autograd.Function):
    """EmbeddingLookUpWeightedFMSum and EmbeddingLookUpWeightedFMSum_Gradient as one autograd node: forward returns S [B, d] and
    Q [B, d] of one fused lookup over (ids, weights) that writes no rows; backward wraps the gradients of both as weighted
    FM-pooled IndexedSlices in `sink` -- nothing [B * 26, d] is saved or built.  `anchor` as in FMLookup."""

    @staticmethod
    def forward(ctx, anchor, ids, weights, lookup, lookup_grad, sink):
        batch, width = ids.shape[0], lookup.embedding.shape[1]
        total = torch.empty((batch, width), dtype=torch.float32, device=ids.device)
        sq = torch.empty((batch, width), dtype=torch.float32, device=ids.device)
        lookup.compute(ids, weights, total, sq)
        ctx.save_for_backward(ids, weights)
        ctx.lookup_grad, ctx.sink = lookup_grad, sink
        return total, sq

    @staticmethod
    def backward(ctx, g_total, g_sq):
        ids, weights = ctx.saved_tensors
        ctx.sink["grad"] = ctx.lookup_grad.compute(g_total.contiguous(), g_sq.contiguous(), ids, weights)
        return None, None, None, None, None, None


POOLED_MODELS = ("emb_sum_wdl",)
FM_MODELS = ("deepfm", "emb_sum_deepfm")
FAE_MODELS = ("fae_wdl",)
FAE_FM_MODELS = ("fae_deepfm",)
MODEL_ALIASES = {"emb_sum_deepfm_avazu": "emb_sum_deepfm", "emb_sum_dfm_avazu": "emb_sum_deepfm", "fae_wdl_criteo": "fae_wdl",
                 "fae_deepfm_avazu": "fae_deepfm", "fae_dfm_avazu": "fae_deepfm"}
OPTIMIZERS = ("sgd", "momentum", "nesterov", "adagrad", "adam", "adamw")


def make_tower(model, width, seed=0):
    return {"wdl": Tower, "dcn": CrossTower, "emb_sum_wdl": SumTower, "deepfm": FMTower,
            "emb_sum_deepfm": SumFMTower, "fae_wdl": SumTower, "fae_deepfm": SumFMTower}[model](width, seed)


def fae_hot_ids(batches, rows, rate):
    """The hot list of an FAE run, on the host: the int(rate * rows) most frequent ids of the run's batches, most frequent first,
    ties to the smaller id (int64 [num_hot])."""
    counts = np.bincount(np.concatenate([b[0].reshape(-1) for b in batches]).astype(np.int64), minlength=rows)
    order = np.lexsort((np.arange(rows), -counts))
    return order[:int(rate * rows)]


def fae_split(ids, hot):
    """A batch's ids [B, 26] split by the hot list: hot_rank int64 (the 1-based rank of a hot id, 0 if the id is cold), cold_ids
    float32 (the id if cold, else the padding id 0) and cold_mask float32 (1.0 where the id is cold)."""
    rank_of = np.zeros(max(int(ids.max()) + 1, int(hot.max(initial=0)) + 1), dtype=np.int64)
    rank_of[hot] = np.arange(1, hot.size + 1)
    hot_rank = rank_of[ids.astype(np.int64)]
    cold = hot_rank == 0
    return hot_rank, np.where(cold, ids, np.float32(0)).astype(np.float32), cold.astype(np.float32)


def make_samples(nsamples, rows, seed=0):
    """One sample set for every rank (the laia scheduler distributes it): ids float32 [S, 26], dense [S, 13],
    labels [S, 1]."""
    rng = np.random.default_rng(seed + 77)
    wd = rng.standard_normal(NDENSE).astype(np.float32)
    chunk = 256
    raw = np.concatenate([synth.criteo_batch(chunk, step=5000 + seed * 131 + c, rows=rows)
                          for c in range(-(-nsamples // chunk))], axis=0)[:nsamples]
    ids = np.minimum(synth.as_f32_ids(raw), np.float32(rows - 1))
    dense = rng.standard_normal((nsamples, NDENSE)).astype(np.float32)
    score = dense @ wd + ((raw[:, :4].sum(axis=1) % 7) - 3).astype(np.float32)
    return ids, dense, (score > 0).astype(np.float32).reshape(-1, 1)


def train_laia(model="wdl", rows=200000, width=32, batch=64, steps=20, lr=0.01, cache="LRU", bound=0, cache_limit=None,
               seed=0, device="cuda:0", table_init=None, a2a=None, allreduce=None, local_shared=False, nsamples=None,
               perf=False, log_every=0, cache_planned=False):
    """The laia-driven loop (run_laia.py:214-236).  `batch` = samples per worker and step; a2a / allreduce: optional
    replacements of the collectives (several ranks on one GPU under gloo in the tests).  cache_planned (--cache-planned): on
    one rank, the cache's planned flow -- the sparse loader hands the communicate op the (ids, push plan) of the batch after
    next (`peek_arr`), its bookkeeping runs beside the step; the update pushes the plan's keys (no effect at world > 1).
    Returns (losses, embedding parameter, tower, communicate op)."""
    import torch.distributed as dist
    from herald_amd import laia as hlaia
    dev = torch.device(device)
    rank = dist.get_rank() if dist.is_initialized() else 0
    world = dist.get_world_size() if dist.is_initialized() else 1
    if nsamples is None:
        nsamples = world * batch * max(steps + 2, hlaia.LAIAScheduler.WINDOW + 1)
    ids_all, dense_all, label_all = make_samples(nsamples, rows, seed)
    limit = cache_limit if cache_limit is not None else max(rows // 10, batch * NFIELD)
    # the scheduler walks the whole sample set (every rank the same: laia_dataloader.py:29-95) ...
    sched = hlaia.LAIAScheduler(ids_all, batch, dataset="criteo", local_shared=local_shared)
    epochs = -(-steps * batch * world // nsamples) + 1
    sched.start(nrank=world, rank=rank, cache_limit=limit, dataset_num=3, epoch_num=epochs, key_limit=rows,
                local_rank=rank, local_size=world)
    # ... and three loaders hand this worker its share of every global batch (run_laia.py:188-199)
    sparse_dl = hlaia.LAIADataloader(sched, 0, True, ids_all, batch, name="train", device=dev)
    label_dl = hlaia.LAIADataloader(sched, 1, False, label_all, batch, name="train", device=dev)
    dense_dl = hlaia.LAIADataloader(sched, 2, False, dense_all, batch, name="train", device=dev)
    for dl in (sparse_dl, label_dl, dense_dl):
        dl.init_states(rank, world)
    batch = sched.batch_size
    tower = make_tower(model, width, seed).to(dev)
    opt = torch.optim.SGD(tower.parameters(), lr=lr)
    if table_init is None:
        g = torch.Generator(device=dev).manual_seed(seed + 1)
        table_init = torch.randn((rows, width), generator=g, device=dev) * 0.01
    store = ShardedEmbedding(rows, width, dev, a2a=a2a)
    store.table.copy_(table_init[store.starts[store.rank]:store.starts[store.rank + 1]])
    param = hetu_ops.EmbeddingParameter(store=store)
    planned = bool(cache_planned) and world == 1
    config = hetu_ops.Config(comm_mode="Hybrid", bsp=0, prefetch=True, cstable_policy=cache, cache_bound=bound,
                             cache_limit=limit, cache_perf_enable=perf, cache_plan_ahead=planned)
    comm = hetu_ops.ParameterServerCommunicateOp(param, lr, next_ids=sparse_dl.get_next_arr,
                                                 peek_ids=sparse_dl.peek_arr if planned else None)
    barrier = dist.barrier if world > 1 else (lambda: None)
    if planned:
        # (the first batch is the one next_ids() returns now: peek_ids counts from it)
        comm.forward_hook(config, barrier=barrier)
    else:
        comm.forward_hook(config, first_ids=sparse_dl.get_next_arr(), barrier=barrier)
    lookup = hetu_ops.EmbeddingLookUp(param, enable_push_index=True)
    lookup.forward_hook(config)
    lookup_grad = hetu_ops.EmbeddingLookUp_Gradient(param.shape, enable_push_index=True)
    if allreduce is None:
        def allreduce(t):
            dist.all_reduce(t)

    losses = []
    t0 = time.perf_counter()
    for k in range(steps):
        ids_plan = sparse_dl.get_arr()                             # (ids [batch, 26], push plan): this worker's samples
        label = label_dl.get_arr()
        dense = dense_dl.get_arr()
        emb = torch.empty((batch, NFIELD, width), dtype=torch.float32, device=dev)
        lookup.compute(ids_plan, emb)                              # the rows the communicate op pulled for this batch
        emb.requires_grad_(True)
        pred = tower(dense, emb.reshape(batch, NFIELD * width))
        loss = torch.nn.functional.binary_cross_entropy(pred, label)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        if world > 1:                                              # Hybrid: dense parameters by all-reduce, averaged
            for p_ in tower.parameters():
                allreduce(p_.grad)
                p_.grad.div_(world)
        opt.step()
        grad = lookup_grad.compute(emb.grad, ids_plan)             # IndexedSlices(indices, values, push_indices = plan)
        comm.compute(grad)              # -lr scale, embedding_update_with_push_keys (planned: its planned form), barrier, next lookup
        losses.append(float(loss.detach()))
        if log_every and (k + 1) % log_every == 0 and rank == 0:
            print("step %d loss %.5f (%.1f ms/step)" % (k + 1, np.mean(losses[-log_every:]),
                                                        1e3 * (time.perf_counter() - t0) / (k + 1)))
    torch.cuda.synchronize()
    sched.sched.close()
    return losses, param, tower, comm


def make_batches(nbatch, batch, rows, seed=0, rank=0, world=1):
    """-> list of (ids float32 [batch, 26], dense float32 [batch, 13], label float32 [batch, 1])."""
    rng = np.random.default_rng(seed + 1000 * rank)
    wd = rng.standard_normal(NDENSE).astype(np.float32)
    out = []
    for b in range(nbatch):
        raw = synth.criteo_batch(batch, step=b * world + rank, rows=rows)
        ids = np.minimum(synth.as_f32_ids(raw), np.float32(rows - 1))
        dense = rng.standard_normal((batch, NDENSE)).astype(np.float32)
        score = dense @ wd + ((raw[:, :4].sum(axis=1) % 7) - 3).astype(np.float32)
        out.append((ids, dense, (score > 0).astype(np.float32).reshape(-1, 1)))
    return out


def train_deepfm(rows, width, batch, steps, lr, seed, device, table_init, first_order_init, log_every, model="deepfm"):
    """--model deepfm with both tables in HBM: the first-order table [rows, 1] through EmbeddingLookUpSum and the pooled SGD
    apply, the second-order table [rows, width] through the FM operator pair (FMLookup) and the unpooled sparse SGD.
    --model emb_sum_deepfm: the second-order table through the pooled pair (FMSumLookup: S and the FM output, no rows) and
    the fused FM apply of FM-pooled slices.  Returns (losses, second-order parameter, tower); the first-order parameter is
    `parameter.first_order`."""
    dev = torch.device(device)
    pooled = model == "emb_sum_deepfm"
    tower = make_tower(model, width, seed).to(dev)
    opt = torch.optim.SGD(tower.parameters(), lr=lr)
    dev_batches = [tuple(torch.from_numpy(a).to(dev) for a in b) for b in make_batches(min(steps + 1, 64), batch, rows, seed)]
    if table_init is None:
        g = torch.Generator(device=dev).manual_seed(seed + 1)
        table_init = torch.randn((rows, width), generator=g, device=dev) * 0.01    # init.random_normal(stddev=0.01)
    if first_order_init is None:
        g = torch.Generator(device=dev).manual_seed(seed + 2)
        first_order_init = torch.randn((rows, 1), generator=g, device=dev) * 0.01
    config = hetu_ops.Config(comm_mode=None)
    param = hetu_ops.EmbeddingParameter(table=table_init.clone())
    param.first_order = first = hetu_ops.EmbeddingParameter(table=first_order_init.clone())
    first_lookup = hetu_ops.EmbeddingLookUpSum(first)
    first_lookup.forward_hook(config)
    first_grad = hetu_ops.EmbeddingLookUpSum_Gradient(first.shape)
    lookup = (hetu_ops.EmbeddingLookUpFMSum if pooled else hetu_ops.EmbeddingLookUpFM)(param)
    lookup.forward_hook(config)
    lookup_grad = (hetu_ops.EmbeddingLookUpFMSum_Gradient if pooled else hetu_ops.EmbeddingLookUpFM_Gradient)(param.shape)
    anchor = torch.zeros((), device=dev, requires_grad=True)
    sink = {}
    losses = []
    t0 = time.perf_counter()
    for k in range(steps):
        ids, dense, label = dev_batches[k % len(dev_batches)]
        y_first = torch.empty((batch, 1), dtype=torch.float32, device=dev)
        first_lookup.compute(ids, y_first)                         # embedding_lookup_op + reduce_sum_op(axes=1), width 1
        y_first.requires_grad_(True)
        if pooled:
            total, fm = FMSumLookup.apply(anchor, ids, lookup, lookup_grad, sink)
            pred = tower(dense, total, y_first, fm)
        else:
            emb, fm = FMLookup.apply(anchor, ids, lookup, lookup_grad, sink)
            pred = tower(dense, emb.reshape(batch, NFIELD * width), y_first, fm)
        loss = torch.nn.functional.binary_cross_entropy(pred, label)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        hetu_ops.sgd_update_sparse(first, first_grad.compute(y_first.grad, ids), lr)      # pooled slices: the bag apply
        hetu_ops.sgd_update_sparse(param, sink.pop("grad"), lr)              # unpooled slices, or FM-pooled: the fused FM apply
        losses.append(float(loss.detach()))
        if log_every and (k + 1) % log_every == 0:
            print("step %d loss %.5f (%.1f ms/step)" % (k + 1, np.mean(losses[-log_every:]),
                                                        1e3 * (time.perf_counter() - t0) / (k + 1)))
    torch.cuda.synchronize()
    return losses, param, tower


def train_fae_deepfm(rows, width, batch, steps, lr, seed, device, table_init, first_order_init, log_every, fae_hot_rate):
    """--model fae_deepfm (examples/ctr/models/fae_deepfm_avazu.py) with both tables in HBM.  The hot list and the split of every
    batch are fae_wdl's (fae_hot_ids / fae_split).  First-order table [rows, 1]: EmbeddingLookUpWeightedSum over (cold_ids,
    cold_mask) plus a hot table [num_hot, 1].  Second-order table [rows, width]: the weighted FM operator pair (WeightedFMSumLookup:
    S and Q of the cold rows, no [B * 26, d] tensor) plus a hot table [num_hot, width] (the reference's W5), whose halves of S and Q
    are embedding_bag over W5 and over W5 * W5 with per-sample weights 1 - cold_mask; then S = S_cold + S_hot, Q = Q_cold + Q_hot
    and fm = 0.5 * (S*S - Q): the square of the sum is taken after the halves are added.  Both hot tables start as copies of the
    main tables' hot rows and are trained with the tower; the main tables take the fused weighted applies.  Returns (losses,
    second-order parameter, tower); the parameter carries `hot_table`, `hot_ids` and `first_order`, which carries its own
    `hot_table`."""
    dev = torch.device(device)
    tower = make_tower("fae_deepfm", width, seed).to(dev)
    opt = torch.optim.SGD(tower.parameters(), lr=lr)
    batches = make_batches(min(steps + 1, 64), batch, rows, seed)
    dev_batches = [tuple(torch.from_numpy(a).to(dev) for a in b) for b in batches]
    if table_init is None:
        g = torch.Generator(device=dev).manual_seed(seed + 1)
        table_init = torch.randn((rows, width), generator=g, device=dev) * 0.01    # init.random_normal(stddev=0.01)
    if first_order_init is None:
        g = torch.Generator(device=dev).manual_seed(seed + 2)
        first_order_init = torch.randn((rows, 1), generator=g, device=dev) * 0.01
    hot = fae_hot_ids(batches, rows, fae_hot_rate)
    splits = [tuple(torch.from_numpy(a).to(dev) for a in fae_split(b[0], hot)) for b in batches]
    config = hetu_ops.Config(comm_mode=None)
    param = hetu_ops.EmbeddingParameter(table=table_init.clone())
    param.first_order = first = hetu_ops.EmbeddingParameter(table=first_order_init.clone())
    param.hot_ids = first.hot_ids = torch.from_numpy(hot).to(dev)
    param.hot_table = hot_table = torch.nn.Parameter(param.table[param.hot_ids].clone())
    first.hot_table = first_hot = torch.nn.Parameter(first.table[param.hot_ids].clone())
    opt.add_param_group({"params": [hot_table, first_hot]})
    first_lookup = hetu_ops.EmbeddingLookUpWeightedSum(first)
    first_lookup.forward_hook(config)
    first_grad = hetu_ops.EmbeddingLookUpWeightedSum_Gradient(first.shape)
    lookup = hetu_ops.EmbeddingLookUpWeightedFMSum(param)
    lookup.forward_hook(config)
    lookup_grad = hetu_ops.EmbeddingLookUpWeightedFMSum_Gradient(param.shape)
    anchor = torch.zeros((), device=dev, requires_grad=True)
    sink = {}
    losses = []
    t0 = time.perf_counter()
    for k in range(steps):
        _, dense, label = dev_batches[k % len(dev_batches)]
        hot_rank, cold_ids, cold_mask = splits[k % len(splits)]
        y_cold = torch.empty((batch, 1), dtype=torch.float32, device=dev)
        first_lookup.compute(cold_ids, cold_mask, y_cold)          # the first-order term: the weighted bag at width 1
        y_cold.requires_grad_(True)
        total, sq = WeightedFMSumLookup.apply(anchor, cold_ids, cold_mask, lookup, lookup_grad, sink)
        y_first = y_cold
        if hot.size > 0:
            # the hot halves: a cold slot reads hot row 0 with weight 0
            idx, hw = (hot_rank - 1).clamp_(min=0), 1 - cold_mask
            bag = torch.nn.functional.embedding_bag
            y_first = y_cold + bag(idx, first_hot, per_sample_weights=hw, mode="sum")
            total = total + bag(idx, hot_table, per_sample_weights=hw, mode="sum")
            sq = sq + bag(idx, hot_table * hot_table, per_sample_weights=hw, mode="sum")
        fm = 0.5 * (total * total - sq)
        pred = tower(dense, total, y_first, fm)
        loss = torch.nn.functional.binary_cross_entropy(pred, label)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        hetu_ops.sgd_update_sparse(first, first_grad.compute(y_cold.grad, cold_ids, cold_mask), lr)    # weighted pooled slices
        hetu_ops.sgd_update_sparse(param, sink.pop("grad"), lr)          # weighted FM-pooled slices: the fused weighted FM apply
        losses.append(float(loss.detach()))
        if log_every and (k + 1) % log_every == 0:
            print("step %d loss %.5f (%.1f ms/step)" % (k + 1, np.mean(losses[-log_every:]),
                                                        1e3 * (time.perf_counter() - t0) / (k + 1)))
    torch.cuda.synchronize()
    return losses, param, tower


def train(embedding="hbm", rows=200000, width=32, batch=256, steps=50, lr=0.01, cache="LRU", bound=0,
          cache_limit=None, seed=0, device="cuda:0", table_init=None, log_every=0, model="wdl", a2a=None, allreduce=None,
          bsp=0, cache_perf=False, perf_csv_dir=None, cache_planned=False, cache_fuse_bags=True, optimizer="sgd",
          opt_fuse_bags=True, ps_fuse_bags=True, cache_fuse_bag_calls=False, first_order_init=None, fae_hot_rate=0.01,
          ps_fuse_wbags=False, cache_fuse_wbags=False):
    """Runs `steps` training steps; returns (losses, embedding parameter, tower).  cache_planned (--cache-planned, with
    --embedding cache on one rank): the cache's planned flow -- the loader's ring hands the communicate op the ids one
    batch further ahead (`peek_ids`), the bookkeeping of batch k + 1 runs beside the step on batch k.  At bsp 0 these are the
    planned lookup + update pairs; at bsp < 0 (asp, the command line's default) with the LRU policy the planned push-pull chain:
    one cache call per training step, which needs cache_limit >= 2 * batch * 26 (the default limit takes that into account).
    A pooled model (emb_sum_wdl) on the planned pairs (bsp 0) and on the planned push-pull chain (bsp < 0, LRU) pulls and pushes
    POOLED rows: the communicate op is told the bag size, the cache sums a sample's 26 rows as it reads them and takes the
    [batch, width] gradient as it is (cache_fuse_bags=False: the unfused path, the same bits).  On --embedding ps a pooled model does the same through the
    sharded store's pull_sum / push_bags on every schedule (ps_fuse_bags=False, --no-ps-fuse-bags: the unfused path, the same bits).
    cache_fuse_bag_calls (--cache-fuse-bag-calls): a pooled model whose cache flow is call by call (no cache_planned, LFU / LFUOpt
    at bsp < 0, world size > 1) pulls and pushes pooled rows through the cache's pooled calls as well (off: the unfused path, the
    same bits).
    The ring wraps round, so the chain is still open when training ends, with one step's bookkeeping planned ahead and never
    run -- harmless: the store's table is written by row launches only.  LFU / LFUOpt at bsp < 0 stay call by call.  a2a / allreduce: optional
    replacements of the collectives at world size > 1 (several ranks on one GPU under gloo in the tests).
    optimizer (--optimizer): the embedding table's optimizer, --embedding hbm only -- sgd, momentum, nesterov, adagrad, adam or
    adamw with the reference's defaults (momentum 0.9; beta 0.9 / 0.999, eps 1e-7, accumulator from 0, weight decay 0); the
    tower keeps SGD.  opt_fuse_bags=False: the reference's own sequence for it (expanded gradient, deduplicate, the symbol) --
    the same bits.
    model="deepfm" (--model deepfm): DeepFM, --embedding hbm with --optimizer sgd only (train_deepfm); first_order_init: its
    first-order table [rows, 1] (default: N(0, 0.01) from seed + 2), table_init the second-order one.
    model="fae_wdl" (--model fae_wdl), --embedding hbm -- or --embedding ps with ps_fuse_wbags (--ps-fuse-wbags), see below --: the int(fae_hot_rate * rows) most frequent ids of the run's batches
    are hot (fae_hot_ids).  The hot table [num_hot, width] is a torch parameter, initialised from the main table's rows at the
    hot ids and trained with the tower; its half of a sample's sum is embedding_bag with per-sample weights 1 - cold_mask.  The
    cold half is EmbeddingLookUpWeightedSum on the main table over (cold_ids, cold_mask), its gradient weighted pooled slices:
    --optimizer sgd applies them fused, the others expanded.  The returned parameter carries `hot_table` and `hot_ids`.
    With ps_fuse_wbags on --embedding ps the cold table lives behind the sharded store, as the reference keeps it on ctx=ht.cpu(0):
    the communicate op is given the COLD ids and the cold mask of batch k + 1 and bag=26, pulls weighted pooled rows
    (store.pull_wsum) and pushes the weighted pooled slices as they are (push_wbags): no [batch * 26, width] tensor either way.
    With cache_fuse_wbags (--cache-fuse-wbags) on --embedding cache with cache_planned at bsp 0 on one rank the cold table lives
    behind the HET cache -- the reference's hybrid_fae_wdl_criteo.sh, --cache lfu --bound 0 --bsp 0 --: the op pulls with
    embedding_lookup_wsum_planned and pushes with embedding_update_planned_wbags, the bookkeeping of batch k + 1 beside step k.
    Every other fae_wdl run on the cache is refused.
    model="fae_deepfm" (--model fae_deepfm), --embedding hbm with --optimizer sgd only (train_fae_deepfm): the FAE split over the
    DeepFM's two tables, the second-order one through the weighted FM-pooled lookup and its fused apply."""
    if model in FAE_FM_MODELS:
        if embedding != "hbm" or optimizer != "sgd":
            raise ValueError("%s runs with --embedding hbm and --optimizer sgd only: its weighted FM-pooled lookup is not part of "
                             "the step engines, the PS or the cache flows, nor of the other optimizers' pooled paths (got "
                             "--embedding %s --optimizer %s)" % (model, embedding, optimizer))
        return train_fae_deepfm(rows, width, batch, steps, lr, seed, device, table_init, first_order_init, log_every,
                                fae_hot_rate)
    if model in FM_MODELS:
        if embedding != "hbm" or optimizer != "sgd":
            raise ValueError("%s runs with --embedding hbm and --optimizer sgd only: its FM-pooled lookup is not part of the "
                             "step engines, the PS or the cache flows, nor of the other optimizers' pooled paths (got "
                             "--embedding %s --optimizer %s)" % (model, embedding, optimizer))
        return train_deepfm(rows, width, batch, steps, lr, seed, device, table_init, first_order_init, log_every, model)
    dev = torch.device(device)
    pooled = model in POOLED_MODELS
    fae = model in FAE_MODELS
    import torch.distributed as dist
    fae_on_cache = embedding == "cache" and cache_fuse_wbags and cache_planned and bsp == 0 and \
        not (dist.is_initialized() and dist.get_world_size() > 1)
    if fae and not (embedding == "hbm" or (embedding == "ps" and ps_fuse_wbags) or fae_on_cache):
        raise ValueError("%s runs with --embedding hbm, with --embedding ps and --ps-fuse-wbags (ps_fuse_wbags=True), or with "
                         "--embedding cache, --cache-planned, --bsp 0 and --cache-fuse-wbags (cache_fuse_wbags=True) on one rank: "
                         "the weighted sum-pooled lookup has no form on the step engines and no pooled form in the other cache "
                         "flows (got --embedding %s)" % (model, embedding))
    if optimizer not in OPTIMIZERS:
        raise ValueError("optimizer must be one of %s, got %r" % (", ".join(OPTIMIZERS), optimizer))
    if optimizer != "sgd" and embedding != "hbm":
        raise ValueError("--optimizer %s is applied to the embedding table on --embedding hbm only; --embedding %s runs sparse "
                         "SGD" % (optimizer, embedding))
    if pooled and embedding in ("step", "step3", "queue"):
        raise ValueError("--model %s pools its embeddings (sum over a sample's 26 rows): the step engines (--embedding step, "
                         "step3, queue) deliver and update per-occurrence rows only; use --embedding hbm (fused), ps or cache"
                         % model)
    import torch.distributed as dist
    rank = dist.get_rank() if dist.is_initialized() else 0
    world = dist.get_world_size() if dist.is_initialized() else 1
    tower = make_tower(model, width, seed).to(dev)
    if allreduce is None:
        def allreduce(t):
            dist.all_reduce(t)
    opt = torch.optim.SGD(tower.parameters(), lr=lr)
    batches = make_batches(min(steps + 1, 64), batch, rows, seed, rank, world)
    dev_batches = [tuple(torch.from_numpy(a).to(dev) for a in b) for b in batches]
    state = {"k": 0}

    def ids_of(k):
        return dev_batches[k % len(dev_batches)][0]

    if table_init is None:
        g = torch.Generator(device=dev).manual_seed(seed + 1)
        table_init = torch.randn((rows, width), generator=g, device=dev) * 0.01    # init.random_normal(stddev=0.01)
    splits = None
    if fae:      # the hot list from the run's batches, every batch split by it
        hot = fae_hot_ids(batches, rows, fae_hot_rate)
        splits = [tuple(torch.from_numpy(a).to(dev) for a in fae_split(b[0], hot)) for b in batches]
    if embedding in ("hbm", "step", "step3", "queue"):
        param = hetu_ops.EmbeddingParameter(table=table_init.clone())
        config = hetu_ops.Config(comm_mode=None)
        comm = None
    else:
        store = ShardedEmbedding(rows, width, dev, a2a=a2a)
        store.table.copy_(table_init[store.starts[store.rank]:store.starts[store.rank + 1]])
        param = hetu_ops.EmbeddingParameter(store=store)
        config = hetu_ops.Config(comm_mode="PS" if embedding == "ps" else "Hybrid", bsp=bsp, prefetch=True,
                                 cstable_policy=cache if embedding == "cache" else None, cache_bound=bound,
                                 cache_limit=cache_limit if cache_limit is not None else
                                 max(rows // 10, batch * NFIELD * (2 if cache_planned and bsp < 0 else 1)),
                                 cache_perf_enable=cache_perf, cache_plan_ahead=cache_planned, cache_fuse_bags=cache_fuse_bags,
                                 ps_fuse_bags=ps_fuse_bags, cache_fuse_bag_calls=cache_fuse_bag_calls,
                                 ps_fuse_wbags=ps_fuse_wbags, cache_fuse_wbags=cache_fuse_wbags)
        barrier = dist.barrier if world > 1 else (lambda: None)
        if fae:
            # the cold table behind the store (--embedding ps) or behind the cache over it (--embedding cache, the planned pairs):
            # the op pulls and pushes the COLD ids with their mask, weighted and pooled
            def cold_of(k, what):
                return splits[k % len(splits)][what]
            comm = hetu_ops.ParameterServerCommunicateOp(param, lr, next_ids=lambda: cold_of(state["k"] + 1, 1),
                                                         peek_ids=lambda j: cold_of(state["k"] + 1 + j, 1), bag=NFIELD,
                                                         next_weights=lambda: cold_of(state["k"] + 1, 2))
            comm.forward_hook(config, first_ids=cold_of(0, 1), barrier=barrier, first_weights=cold_of(0, 2))
        else:
            comm = hetu_ops.ParameterServerCommunicateOp(param, lr, next_ids=lambda: ids_of(state["k"] + 1),
                                                         peek_ids=lambda j: ids_of(state["k"] + 1 + j),
                                                         bag=NFIELD if pooled and embedding in ("cache", "ps") else None)
            comm.forward_hook(config, first_ids=ids_of(0), barrier=barrier)
    hot_table = None
    if fae:
        # the hot table starts as the main table's hot rows
        param.hot_ids = torch.from_numpy(hot).to(dev)
        param.hot_table = hot_table = torch.nn.Parameter(
            (param.table if param.table is not None else table_init)[param.hot_ids].clone())
        opt.add_param_group({"params": [hot_table]})
        lookup = hetu_ops.EmbeddingLookUpWeightedSum(param)
        lookup_grad = hetu_ops.EmbeddingLookUpWeightedSum_Gradient(param.shape)
    elif pooled:
        # embedding_lookup_op + reduce_sum_op(axes=1) as one operator: the fused kernel on a device table, the same ordered sum
        # over the delivered rows on the ps / cache paths; its gradient stays [batch, width] (pooled IndexedSlices)
        lookup = hetu_ops.EmbeddingLookUpSum(param)
        lookup_grad = hetu_ops.EmbeddingLookUpSum_Gradient(param.shape)
    else:
        lookup = hetu_ops.EmbeddingLookUp(param)
        lookup_grad = hetu_ops.EmbeddingLookUp_Gradient(param.shape)
    lookup.forward_hook(config)

    # the embedding optimizer's states, allocated beside the table (zeros: the reference's initial values)
    opt_state = None
    if optimizer != "sgd":
        opt_state = {"s1": torch.zeros_like(param.table), "beta1t": 1.0, "beta2t": 1.0}
        if optimizer in ("adam", "adamw"):
            opt_state["s2"] = torch.zeros_like(param.table)

    def embedding_update(grad):
        if optimizer == "sgd":
            hetu_ops.sgd_update_sparse(param, grad, lr)            # OptimizerOp, sparse SGD branch
        elif optimizer in ("momentum", "nesterov"):
            hetu_ops.momentum_update_sparse(param, grad, opt_state["s1"], lr, 0.9, optimizer == "nesterov",
                                            fuse_bags=opt_fuse_bags)
        elif optimizer == "adagrad":
            hetu_ops.adagrad_update_sparse(param, grad, opt_state["s1"], lr, 1e-7, fuse_bags=opt_fuse_bags)
        else:
            opt_state["beta1t"] *= 0.9                             # once per step, before the update (optimizer.py:384, 456)
            opt_state["beta2t"] *= 0.999
            args = (param, grad, opt_state["s1"], opt_state["s2"], lr, 0.9, 0.999, opt_state["beta1t"], opt_state["beta2t"],
                    1e-7)
            if optimizer == "adam":
                hetu_ops.adam_update_sparse(*args, fuse_bags=opt_fuse_bags)
            else:
                hetu_ops.adamw_update_sparse(*args, 0.0, fuse_bags=opt_fuse_bags)

    fused = None
    if embedding == "step":
        from herald_amd import ops
        n = batch * NFIELD
        fused = {"plans": [ops.IndexPlan(n, dev), ops.IndexPlan(n, dev)],
                 "pends": [ops.PendingTable(dev), ops.PendingTable(dev)],
                 "outs": [torch.empty((batch, NFIELD, width), dtype=torch.float32, device=dev) for _ in range(2)]}
        ops.lookup_sort_pend(param.table, ids_of(0).reshape(-1), fused["plans"][0], fused["pends"][0],
                             out=fused["outs"][0])                  # the lookup of the first batch

    pipe = None
    if embedding == "step3":
        from herald_amd import ops
        pipe = ops.StepPipeline(param.table, batch * NFIELD, lr)
        pipe_out = pipe.start(ids_of(0), ids_of(1), ids_of(2))     # rows of the first batch
    qpipe = None
    if embedding == "queue":
        # the work-queue step (ha_qapply; what bench.py times): plans and queues a block of steps ahead on a side stream,
        # one launch per step between the model's backward and the next forward
        from herald_amd import ops
        qpipe = pipe = ops.QueueStepPipeline(param.table, batch * NFIELD, lr, block=4)
        pipe_out = pipe.start([ids_of(j) for j in range(pipe.LOOKAHEAD)])

    losses = []
    t0 = time.perf_counter()
    for k in range(steps):
        state["k"] = k
        ids, dense, label = dev_batches[k % len(dev_batches)]
        if pipe is not None:
            emb = pipe_out.detach().clone()                        # written by the previous step's launch
        elif fused is not None:
            emb = fused["outs"][k % 2].detach().clone()            # looked up by the previous step's launch
        elif fae:
            hot_rank, cold_ids, cold_mask = splits[k % len(splits)]
            emb = torch.empty((batch, width), dtype=torch.float32, device=dev)
            lookup.compute(cold_ids, cold_mask, emb)               # embedding_lookup_op, mul_op by the mask, reduce_sum_op(axes=1)
        else:
            emb = torch.empty((batch, width) if pooled else (batch, NFIELD, width), dtype=torch.float32, device=dev)
            lookup.compute(ids, emb)                               # embedding_lookup_op (+ reduce_sum_op(axes=1))
        emb.requires_grad_(True)
        if fae and hot_table.shape[0] > 0:
            # the hot half of the sum: a cold slot reads hot row 0 with weight 0
            hot_sum = torch.nn.functional.embedding_bag((hot_rank - 1).clamp_(min=0), hot_table, per_sample_weights=1 - cold_mask,
                                                        mode="sum")
            pred = tower(dense, emb + hot_sum)
        else:
            pred = tower(dense, emb.reshape(batch, -1))
        loss = torch.nn.functional.binary_cross_entropy(pred, label)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        if world > 1:                                              # data parallel: dense parameters by all-reduce, averaged
            for p_ in tower.parameters():
                allreduce(p_.grad)
                p_.grad.div_(world)
        opt.step()
        if fae:
            grad = lookup_grad.compute(emb.grad, cold_ids, cold_mask)      # weighted pooled IndexedSlices
        else:
            grad = lookup_grad.compute(emb.grad, ids)              # IndexedSlices(indices, values)
        if pipe is not None:
            # sparse SGD of this batch, rows of the next one, plan finish of batch k+2, sort of batch k+3: one launch
            pipe_out = pipe.step(grad.values.reshape(-1, width).contiguous(),
                                 ids_of(k + (qpipe.LOOKAHEAD if qpipe is not None else 3)))
        elif fused is not None:
            # sparse SGD of this batch + lookup of the next one, one launch (plans / pending tables alternate)
            ops.sgd_push_pull(param.table, fused["plans"][k % 2], grad.values.reshape(-1, width).contiguous(), lr,
                              fused["pends"][k % 2], ids_of(k + 1).reshape(-1), fused["plans"][(k + 1) % 2],
                              fused["pends"][(k + 1) % 2], next_out=fused["outs"][(k + 1) % 2])
        elif comm is None:
            embedding_update(grad)                                 # OptimizerOp's sparse branch of --optimizer
        else:
            comm.compute(grad)                                     # -lr scale, push, (barrier), pull of batch k+1
        losses.append(float(loss.detach()))       # synchronises: a cheap place to poll the hand-off flag
        if fused is not None and log_every and (k + 1) % log_every == 0:
            ops.check_handoff(fused["plans"])
        if log_every and (k + 1) % log_every == 0 and rank == 0:
            print("step %d loss %.5f (%.1f ms/step)" % (k + 1, np.mean(losses[-log_every:]),
                                                        1e3 * (time.perf_counter() - t0) / (k + 1)))
    torch.cuda.synchronize()
    if fused is not None:
        ops.check_handoff(fused["plans"])
    if cache_perf and comm is not None and getattr(comm, "cache", None) is not None:
        dump_cache_perf([comm.cache], rank, perf_csv_dir)
    return losses, param, tower


def dump_cache_perf(caches, rank, csv_dir=None):
    """What /root/reference/examples/ctr/run_hetu.py:508-515 does after training with --cache-perf: one CSV per cache
    table, `csv/hetu_cache<idx>_<rank>.csv` beside the script, one row per cache call (the perf dicts: counts -- num_all,
    num_unique, num_miss, num_evict, num_transfered, ... -- and stage times)."""
    import csv
    csv_dir = csv_dir or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csv")
    os.makedirs(csv_dir, exist_ok=True)
    paths = []
    for idx, c in enumerate(caches):
        if c is None:
            print("Cache perf is None")
            continue
        rows = list(c.get_perf())
        path = os.path.join(csv_dir, "hetu_cache%d_%d.csv" % (idx, rank))
        cols = sorted({k for r in rows for k in r})
        with open(path, "w", newline="") as fh:
            w = csv.writer(fh)
            w.writerow([""] + cols)                      # pandas' to_csv layout: an index column first
            for i, r in enumerate(rows):
                w.writerow([i] + [r.get(k, "") for k in cols])
        paths.append(path)
    return paths


def main():
    # The reference's launch lines work as they are (/root/reference/examples/ctr/run_hetu.py:546-586, run_laia.py):
    #   python run_wdl.py --model wdl_criteo --comm Hybrid --cache lru --bound 3 --bsp 0 -b 256 -e 512 -r 0.1 --cache-perf
    # --comm / --cache choose the embedding engine unless --embedding names one (this build's own engines: the HBM-resident
    # table with one launch per step, "queue" = the work-queue step with lookahead, ...).
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="wdl", help="wdl_criteo | dcn_criteo | emb_sum_wdl_criteo | deepfm_criteo | "
                                                   "emb_sum_deepfm_avazu | emb_sum_dfm_avazu | fae_wdl_criteo | fae_deepfm_avazu | "
                                                   "fae_dfm_avazu (the reference's names) or wdl | dcn | emb_sum_wdl | deepfm | "
                                                   "emb_sum_deepfm | fae_wdl | fae_deepfm")
    ap.add_argument("--fae-hot-rate", type=float, default=0.01,
                    help="--model fae_wdl / fae_deepfm: the share of the table's rows, most frequent ids first, served by the hot table")
    ap.add_argument("-b", "--batch-size", "--batch", dest="batch", type=int, default=256)
    ap.add_argument("-e", "--embedding-size", "--width", dest="width", type=int, default=128)
    ap.add_argument("-r", "--cache-limit-ratio", type=float, default=0.1,
                    help="ratio of cache limit to total embedding sizes")
    ap.add_argument("--cache-perf", action="store_true",
                    help="record the cache's per-call counters and stage times; csv/hetu_cache<idx>_<rank>.csv after training")
    ap.add_argument("--val", action="store_true", help="accepted for the reference's launch lines (the data is synthetic)")
    ap.add_argument("--all", action="store_true", help="accepted for the reference's launch lines (the data is synthetic)")
    ap.add_argument("--comm", default=None, help="None, PS or Hybrid (sparse pull / push over the row-range sharded table)")
    ap.add_argument("--bsp", type=int, default=-1, help="bsp 0, asp -1, ssp > 0")
    ap.add_argument("--cache", default=None, help="cache policy: lru | lfu | lfuopt (with --comm PS / Hybrid)")
    ap.add_argument("--bound", type=int, default=100, help="cache bound")
    ap.add_argument("--cache-planned", action="store_true",
                    help="--embedding cache, or --laia: the cache's planned flow (bookkeeping of the next batch beside "
                         "this step; --bsp 0: planned lookup + update pairs; --bsp -1, the default, with --cache lru: the planned "
                         "push-pull chain, one cache call per step, cache limit >= 2 * batch * 26; "
                         "--model emb_sum_wdl: the pairs, and the chain at --bsp -1 with --cache lru, are pooled -- the cache "
                         "sums a sample's 26 rows as it reads them and takes the [batch, width] gradient as it is, no "
                         "[batch * 26, width] tensor; "
                         "--laia: the update pushes the batch's push plan).  With --laia at world size > 1 it is "
                         "accepted and has no effect (the cache there talks to a remote store, call by call)")
    ap.add_argument("--no-ps-fuse-bags", action="store_true",
                    help="--embedding ps with --model emb_sum_wdl: pull per-occurrence rows and push the expanded gradient "
                         "instead of the store's pooled pull_sum / push_bags (the same bits)")
    ap.add_argument("--cache-fuse-wbags", action="store_true",
                    help="--embedding cache --cache-planned --bsp 0 with --model fae_wdl: the cold table behind the HET cache -- the "
                         "communicate op pulls weighted pooled rows (embedding_lookup_wsum_planned) and pushes the weighted pooled "
                         "slices as they are (embedding_update_planned_wbags)")
    ap.add_argument("--ps-fuse-wbags", action="store_true",
                    help="--embedding ps with --model fae_wdl: the cold table behind the sharded store -- the communicate op "
                         "pulls weighted pooled rows (pull_wsum) and pushes the weighted pooled gradient as it is (push_wbags), "
                         "no [batch * 26, width] tensor; without it --model fae_wdl runs on --embedding hbm only")
    ap.add_argument("--cache-fuse-bag-calls", action="store_true",
                    help="--embedding cache with --model emb_sum_wdl where the cache is used call by call (no --cache-planned, "
                         "lfu / lfuopt at --bsp -1, world size > 1): pull pooled rows (embedding_lookup_sum) and push the "
                         "[batch, width] gradient as it is (embedding_update_bags / embedding_push_pull_bags) -- the same bits")
    ap.add_argument("--nepoch", type=int, default=-1, help="epochs of `--steps` steps each (default: one)")
    ap.add_argument("--embedding", choices=["hbm", "step", "step3", "queue", "ps", "cache"], default=None,
                    help="this build's engine names; default: from --comm / --cache")
    ap.add_argument("--optimizer", choices=list(OPTIMIZERS), default="sgd",
                    help="the embedding table's optimizer (--embedding hbm only; the tower keeps SGD)")
    ap.add_argument("--rows", type=int, default=33762577)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--lr", type=float, default=0.1)
    ap.add_argument("--laia", action="store_true", help="the laia-scheduled loop of run_laia.py (cache over the sharded table)")
    ap.add_argument("--local-shared", action="store_true", help="--laia with the TopkScheduler + shared-memory rings")
    args = ap.parse_args()
    model = args.model[:-len("_criteo")] if args.model.endswith("_criteo") else MODEL_ALIASES.get(args.model, args.model)
    if model not in ("wdl", "dcn") + POOLED_MODELS + FM_MODELS + FAE_MODELS + FAE_FM_MODELS:
        ap.error("--model must be wdl_criteo, dcn_criteo, emb_sum_wdl_criteo, deepfm_criteo, emb_sum_deepfm_avazu, "
                 "emb_sum_dfm_avazu, fae_wdl_criteo, fae_deepfm_avazu, fae_dfm_avazu, wdl, dcn, emb_sum_wdl, deepfm, "
                 "emb_sum_deepfm, fae_wdl or fae_deepfm")
    args.model = model
    if model in POOLED_MODELS and (args.laia or args.embedding in ("step", "step3", "queue")):
        ap.error("--model %s pools its embeddings: use --embedding hbm (the fused kernel), ps or cache; the step engines "
                 "(step, step3, queue) and --laia run per-occurrence models only" % model)
    comm = None if args.comm in (None, "None") else args.comm
    if comm not in (None, "PS", "Hybrid"):
        ap.error("--comm must be None, PS or Hybrid (dense AllReduce-only runs have no sparse path to replace)")
    policy = {"lru": "LRU", "lfu": "LFU", "lfuopt": "LFUOpt"}.get((args.cache or "lru").lower())
    if policy is None:
        ap.error("--cache must be lru, lfu or lfuopt")
    if args.embedding is None:
        args.embedding = "hbm" if comm is None else ("cache" if args.cache else "ps")
    args.cache = policy
    if args.optimizer != "sgd" and (args.laia or args.embedding != "hbm"):
        ap.error("--optimizer %s is applied to the embedding table on --embedding hbm only" % args.optimizer)
    if model in FM_MODELS + FAE_FM_MODELS and (args.laia or args.embedding != "hbm" or args.optimizer != "sgd"):
        ap.error("--model %s runs with --embedding hbm and --optimizer sgd only" % model)
    if args.cache_fuse_wbags and not (args.embedding == "cache" and args.cache_planned and args.bsp == 0):
        ap.error("--cache-fuse-wbags needs --embedding cache, --cache-planned and --bsp 0 (the planned lookup + update pairs)")
    if model in FAE_MODELS and (args.laia or not (args.embedding == "hbm" or (args.embedding == "ps" and args.ps_fuse_wbags) or
                                                  (args.embedding == "cache" and args.cache_fuse_wbags))):
        ap.error("--model %s runs with --embedding hbm, with --embedding ps and --ps-fuse-wbags, or with --embedding cache, "
                 "--cache-planned, --bsp 0 and --cache-fuse-wbags" % model)
    if args.nepoch > 0:
        args.steps *= args.nepoch
    cache_limit = max(int(args.cache_limit_ratio * args.rows), args.batch * NFIELD)
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    if args.laia:
        losses = train_laia(args.model, args.rows, args.width, args.batch, args.steps, args.lr, args.cache, args.bound,
                            device="cuda:%d" % local_rank, local_shared=args.local_shared,
                            log_every=max(1, args.steps // 10), cache_planned=args.cache_planned)[0]
    else:
        losses = train(args.embedding, args.rows, args.width, args.batch, args.steps, args.lr, args.cache,
                       args.bound, cache_limit=cache_limit, device="cuda:%d" % local_rank,
                       log_every=max(1, args.steps // 10), model=args.model, bsp=args.bsp if comm is not None else 0,
                       cache_perf=args.cache_perf, cache_planned=args.cache_planned, optimizer=args.optimizer,
                       ps_fuse_bags=not args.no_ps_fuse_bags, cache_fuse_bag_calls=args.cache_fuse_bag_calls,
                       fae_hot_rate=args.fae_hot_rate, ps_fuse_wbags=args.ps_fuse_wbags,
                       cache_fuse_wbags=args.cache_fuse_wbags)[0]
    if local_rank == 0:
        print("first 10 steps: loss %.5f   last 10 steps: loss %.5f" % (np.mean(losses[:10]), np.mean(losses[-10:])))


if __name__ == "__main__":
    main()

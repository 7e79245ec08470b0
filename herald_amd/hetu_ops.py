"""Operator-level mirror of the reference's embedding ops: which native call is made,
when, and on which buffers -- without the graph executor around them.

Mirrors (paths relative to /root/reference):
  EmbeddingLookUp / EmbeddingLookUp_Gradient      python/hetu/gpu_ops/EmbeddingLookUp.py:10-125
  EmbeddingLookUpSum / EmbeddingLookUpSum_Gradient  the same followed by reduce_sum_op(axes=1), python/hetu/gpu_ops/ReduceSum.py
                                                  (examples/ctr/models/emb_sum_*.py)
  EmbeddingLookUpFM / EmbeddingLookUpFM_Gradient  one lookup consumed as rows, as reduce_sum_op(axes=1) and as
                                                  reduce_sum_op(mul_op(e, e), axes=1): the second-order term of the DeepFM models
                                                  (examples/ctr/models/deepfm_criteo.py:24-39)
  EmbeddingLookUpFMSum / EmbeddingLookUpFMSum_Gradient  the same lookup when nothing consumes the rows: the pooled DeepFM
                                                  (examples/ctr/models/emb_sum_deepfm_avazu.py); its gradient is applied by
                                                  one fused launch (ops.sgd_apply_fm_bags)
  EmbeddingLookUpWeightedSum / EmbeddingLookUpWeightedSum_Gradient  the lookup followed by mul_op with a per-occurrence weight
                                                  and reduce_sum_op(axes=1): the FAE models (examples/ctr/models/
                                                  fae_wdl_criteo.py:19-31); its gradient is weighted pooled slices, applied by
                                                  one fused launch chain (ops.sgd_sparse_update_wbags) or expanded first
                                                  (unweighted_slices) for every consumer without a weighted form
  EmbeddingLookUpWeightedFMSum / EmbeddingLookUpWeightedFMSum_Gradient  the weighted lookup consumed as reduce_sum_op(x, axes=1)
                                                  and reduce_sum_op(mul_op(x, x), axes=1): the second-order term of the FAE
                                                  DeepFM (examples/ctr/models/fae_deepfm_avazu.py:43-80); its gradient is
                                                  weighted FM-pooled slices, applied by ops.sgd_sparse_update_wfm_bags on a
                                                  device table and refused everywhere else
  ParameterServerCommunicateOp                   python/hetu/gpu_ops/ParameterServerCommunicate.py:12-250
  ParameterServerSparsePullOp                     python/hetu/gpu_ops/ParameterServerCommunicate.py:254-306
  SGD sparse dispatch of OptimizerOp              python/hetu/gpu_links/OptimizerLink.py:23-33
  Momentum / AdaGrad / Adam / AdamW sparse dispatch  python/hetu/gpu_links/OptimizerLink.py:37-100 (*_update_sparse: fused, and
                                                  straight from the pooled gradient of EmbeddingLookUpSum_Gradient)

`Config` carries the HetuConfig fields those ops read (executor.py:162-182): comm_mode, bsp, prefetch,
cstable_policy, cache_bound, cache_limit, use_sparse_pull -- and six switches of this build: cache_plan_ahead (the cache's
planned flow), cache_fuse_bags (with it, at bsp 0 and on the LRU asp chain: a sum-pooled lookup is pulled and pushed pooled, see
Config), cache_fuse_bag_calls (the same through the cache's call-by-call interface, off by default),
ps_fuse_bags (the same on the plain PS flavour, every schedule), ps_fuse_wbags (the WEIGHTED sum-pooled lookup of the FAE
models pulled and pushed pooled on the plain PS flavour) and cache_fuse_wbags (the same in the cache's planned pairs, opt-in).  The data loader contract is the reference's
`get_arr` / `get_next_arr` (python/hetu/dataloader.py:63-98): `next_ids()` returns the ids of the batch
after the current one.  Everything computed goes through libherald_amd.so.
"""
import ctypes

import torch

from . import _lib, cache as hcache, ops
from ._lib import check
from .sharded import ShardedEmbedding


class Config:
    def __init__(self, comm_mode=None, bsp=0, prefetch=True, cstable_policy=None, cache_bound=100, cache_limit=0,
                 use_sparse_pull=True, cache_perf_enable=False, cache_plan_ahead=False, cache_fuse_bags=True,
                 ps_fuse_bags=True, cache_fuse_bag_calls=False, ps_fuse_wbags=True, cache_fuse_wbags=False):
        self.comm_mode, self.bsp, self.prefetch = comm_mode, bsp, prefetch
        # not a HetuConfig field: the cache's PLANNED flow (csrc/cache_block.hip) for the bsp-prefetch schedule -- the bookkeeping
        # of batch k + 1 runs on a side stream beside the model's step on batch k.  Needs ids one batch further ahead than
        # get_next_arr gives them: ParameterServerCommunicateOp(..., peek_ids=...); the reference's loader ring is three batches
        # deep (python/hetu/dataloader.py:63-98), so it has them.
        self.cache_plan_ahead = cache_plan_ahead
        # not a HetuConfig field either: with cache_plan_ahead at bsp 0 (the planned pairs), a communicate op that was told the
        # bag size of a sum-pooled lookup (ParameterServerCommunicateOp(..., bag=F)) pulls [B, width] pooled rows
        # (embedding_lookup_sum_planned) and pushes the pooled gradient as it is (embedding_update_planned_bags): no [n, width]
        # tensor on either side, the same bits.  The planned push-pull chain of the asp-prefetch schedule (bsp < 0, LRU) is
        # fused the same way: its head, every step and its last pull are embedding_push_pull_planned_bags.  False: the unfused
        # path (per-occurrence rows, a summing pass, the expanded gradient).  Every other schedule -- ssp, no prefetch,
        # world > 1, the call-by-call cache (LFU / LFUOpt at bsp < 0 included), laia push plans in a chain -- is unfused.
        self.cache_fuse_bags = cache_fuse_bags
        # the same for the prefetching schedules whose cache flow is CALL BY CALL -- no cache_plan_ahead, LFU / LFUOpt at bsp < 0,
        # the cache over a sharded store (world > 1), laia (ids, push plan) tuples: a communicate op that was told its bag size
        # pulls with embedding_lookup_sum, pushes with embedding_update_bags / embedding_update_with_push_keys_bags and, on the
        # asp schedule, makes embedding_push_pull_bags; sparse_pull_val is [B, width], the same bits.  Off by default: the
        # unfused shapes of those flows are what existing callers see.
        self.cache_fuse_bag_calls = cache_fuse_bag_calls
        # the same switch for the plain PS flavour (no cstable_policy; ssp, asp and no prefetch alike): a communicate op that
        # was told its bag size pulls pooled rows (ShardedEmbedding.pull_sum) and pushes the pooled gradient (push_bags), and
        # without prefetch EmbeddingLookUpSum pulls pooled rows itself (ragged bags too) -- that lookup reads this switch alone:
        # it is pooled whether or not the communicate op was given bag=, which decides the op's own pulls and pushes only.
        # What crosses the fabric does not change -- rows per unique key --, the same bits.  False: per-occurrence rows, a
        # summing pass, the expanded gradient.
        self.ps_fuse_bags = ps_fuse_bags
        # the weighted counterpart on the plain PS flavour (the cold table of the FAE models): a communicate op that was told its
        # bag size AND the weights of the batches it pulls (ParameterServerCommunicateOp(..., bag=F, next_weights=...)) pulls
        # weighted pooled rows (ShardedEmbedding.pull_wsum) and pushes weighted pooled slices as they are (push_wbags), and
        # without prefetch EmbeddingLookUpWeightedSum pulls them itself (ragged bags too).  The same rows per unique key cross
        # the fabric, the same bits.  False: per-occurrence rows, a weighted summing pass, the expanded gradient.
        self.ps_fuse_wbags = ps_fuse_wbags
        # the weighted counterpart on the cache's planned pairs (the FAE models' cold table behind the cache, the reference's
        # --cache lfu --bound 0 --bsp 0): OPT-IN.  With bsp == 0, prefetch, cache_plan_ahead, world size 1 and peek_ids, a
        # communicate op that was given bag=F and next_weights= pulls weighted pooled rows [B, width]
        # (embedding_lookup_wsum_planned) and pushes the weighted pooled slices as they are, -lr included
        # (embedding_update_planned_wbags): the same bits as per-occurrence rows, a weighted summing pass and the expanded
        # gradient.  In every other cache configuration next_weights is refused, with or without the switch.
        self.cache_fuse_wbags = cache_fuse_wbags
        self.cstable_policy, self.cache_bound, self.cache_limit = cstable_policy, cache_bound, cache_limit
        self.use_sparse_pull = use_sparse_pull
        self.cache_perf_enable = cache_perf_enable        # executor.py: cache_perf_enable (run_hetu.py:508-515 dumps the dicts)
        self.ps_map = {}
        self.ps_pooled = {}           # parameter -> bag size: its ps_map buffer holds POOLED rows [B, width]
        self.ps_wpooled = {}          # parameter -> bag size: its ps_map buffer holds WEIGHTED pooled rows [B, width]


class EmbeddingParameter:
    """The embedding Variable node: a device table (comm None/AllReduce) or a PS-resident table reached
    through a ShardedEmbedding and, optionally, a cache."""
    _next_id = 0

    def __init__(self, table=None, store=None):
        self.id = EmbeddingParameter._next_id
        EmbeddingParameter._next_id += 1
        self.table, self.store = table, store
        self.is_embed = True
        self.cache = None
        self.shape = tuple(table.shape) if table is not None else (store.rows, store.width)


def _same_tensor(a, b):
    return a is not None and a.data_ptr() == b.data_ptr() and a.numel() == b.numel() and a.dtype == b.dtype


def scale_(values, factor, stream=None):
    """values *= factor on the device (one rounding per element)."""
    check(_lib.load().ha_scale_f32(ctypes.c_void_p(values.data_ptr()), values.numel(), ctypes.c_float(factor),
                                   ops._stream_ptr(stream)), "ha_scale_f32")
    return values


class EmbeddingLookUp:
    """embedding_lookup_op(embedding, index, enable_push_index)."""

    def __init__(self, embedding, enable_push_index=False):
        self.embedding, self.enable_push_index = embedding, enable_push_index

    def forward_hook(self, config):                                   # EmbeddingLookUp.py:56-75
        self.config = config
        if config.use_sparse_pull and config.comm_mode in ("PS", "Hybrid") or config.cstable_policy:
            if config.prefetch:
                self.compute = self._compute_prefetched
            elif config.cstable_policy:
                self.compute = self._compute_sparsepull_from_cache
            else:
                self.compute = self._compute_sparsepull_from_ps
        else:
            self.compute = self._compute_gpu

    def _compute_gpu(self, ids, output_val, stream=None):              # :24-26
        return ops.embedding_lookup(self.embedding.table, ids, out=output_val, stream=stream)

    def _compute_sparsepull_from_ps(self, ids, output_val, stream=None):   # :28-35
        output_val.copy_(self.embedding.store.pull(ids))
        return output_val

    def _compute_sparsepull_from_cache(self, ids, output_val, stream=None):  # :37-42
        self.embedding.cache.embedding_lookup(ids, output_val).wait()
        return output_val

    def _compute_prefetched(self, ids, output_val, stream=None):
        """With prefetch the op is not computed: its output is the buffer the communicate op filled for
        this batch during the previous step (executor.py:625,883-885)."""
        ev, buf = self.config.ps_map[self.embedding]
        if ev is not None:
            ev.wait()
        output_val.copy_(buf)
        return output_val


class EmbeddingLookUp_Gradient:
    def __init__(self, embed_shape, enable_push_index=False):
        self.embed_shape, self.enable_push_index = embed_shape, enable_push_index

    def compute(self, vectors, index):                                 # EmbeddingLookUp.py:95-111
        if isinstance(index, tuple):
            push = index[1] if self.enable_push_index else None
            return ops.IndexedSlices(indices=index[0], values=vectors, dense_shape=self.embed_shape,
                                     push_indices=push)
        if self.enable_push_index:
            raise TypeError
        return ops.IndexedSlices(indices=index, values=vectors, dense_shape=self.embed_shape)


class EmbeddingLookUpSum(EmbeddingLookUp):
    """embedding_lookup_op(embedding, index) followed by reduce_sum_op(axes=1), the pair of the reference's pooled CTR models
    (examples/ctr/models/emb_sum_wdl_criteo.py:14-16): compute(ids[B, F], output_val[B, width]) -- or ids[n] with
    offsets[B + 1] for ragged bags.  With a device table it is the fused kernel (ops.embedding_lookup_sum).  On the PS, cache
    and prefetched paths the per-occurrence rows arrive as EmbeddingLookUp delivers them and the same kernel sums them, in the
    same position order, out of that row buffer (ids 0 .. n-1): every path agrees bit for bit on equal rows.  Two of those
    paths are fused as well: the cache's planned flow -- the pairs at bsp 0 and the LRU push-pull chain of the asp schedule
    (Config.cache_fuse_bags) -- and the plain PS flavour
    (Config.ps_fuse_bags) -- with prefetch the communicate op's buffer already holds the pooled rows (the cache, or the
    sharded store's pull_sum, summed them as it read them) and is copied as it is; without prefetch the rows come from
    store.pull_sum directly, ragged bags included, whether or not the communicate op was told a bag size (`stream` is not
    used there: the store works on the current stream, as its pull does).  The call-by-call cache with prefetch is fused under
    Config.cache_fuse_bag_calls (off by default); without it, and with ps_fuse_bags=False, [n, width] rows still move."""

    def forward_hook(self, config):
        super().forward_hook(config)
        self._rows_compute = self.compute
        self._fused = self._rows_compute == self._compute_gpu
        self._pos = None
        self.compute = self._compute_sum

    def _compute_sum(self, ids, output_val, stream=None, offsets=None):
        if self._fused:
            return ops.embedding_lookup_sum(self.embedding.table, ids, offsets=offsets, out=output_val, stream=stream)
        if self._rows_compute == self._compute_prefetched and \
                getattr(self.config, "ps_pooled", {}).get(self.embedding) is not None:
            if offsets is not None or ids.dim() != 2 or ids.shape[1] != self.config.ps_pooled[self.embedding]:
                raise ValueError("EmbeddingLookUpSum: the communicate op pulls pooled rows for fixed bags of %d ids"
                                 % self.config.ps_pooled[self.embedding])
            return self._compute_prefetched(ids, output_val, stream)      # a pooled buffer, as it is
        if self._rows_compute == self._compute_sparsepull_from_ps and getattr(self.config, "ps_fuse_bags", True):
            return self.embedding.store.pull_sum(ids, offsets=offsets, out=output_val)
        n, width = ids.numel(), self.embedding.shape[1]
        if self._pos is None or self._pos.numel() < n or self._pos.device != output_val.device:
            self._pos = torch.arange(max(n, 1), dtype=torch.int64, device=output_val.device)
        # (a buffer per call, as the per-occurrence operator's caller allocates its output: the cache fills it on its own stream)
        rows = torch.empty((n, width), dtype=torch.float32, device=output_val.device)
        self._rows_compute(ids, rows.view(tuple(ids.shape) + (width,)), stream)
        return ops.embedding_lookup_sum(rows, self._pos[:n].view(ids.shape), offsets=offsets, out=output_val, stream=stream)


class EmbeddingLookUpSum_Gradient:
    """The gradient of the pair: reduce_sum's gradient broadcasts the pooled gradient row to the bag's occurrences, and
    EmbeddingLookUp_Gradient wraps it as IndexedSlices.  Here the broadcast is not materialised: compute(vectors[B, width],
    index) returns POOLED IndexedSlices (values stay [B, width])."""

    def __init__(self, embed_shape, enable_push_index=False):
        self.embed_shape, self.enable_push_index = embed_shape, enable_push_index

    def compute(self, vectors, index, offsets=None):
        push = None
        if isinstance(index, tuple):
            index, push = index[0], (index[1] if self.enable_push_index else None)
        elif self.enable_push_index:
            raise TypeError
        if offsets is None:
            if index.dim() != 2:
                raise ValueError("fixed bags need an index of shape [B, F]; give offsets for ragged bags")
            return ops.IndexedSlices(indices=index, values=vectors, dense_shape=self.embed_shape, push_indices=push,
                                     bag=index.shape[1])
        return ops.IndexedSlices(indices=index, values=vectors, dense_shape=self.embed_shape, push_indices=push,
                                 bag_of=ops.bag_of(offsets, index.numel()), offsets=offsets)


class EmbeddingLookUpFM(EmbeddingLookUp):
    """embedding_lookup_op(embedding, index) consumed three ways, the second-order term of the reference's DeepFM models
    (examples/ctr/models/deepfm_criteo.py:24-39): as rows (the DNN), as reduce_sum_op(axes=1) and as
    reduce_sum_op(mul_op(e, e), axes=1), the last two combined into 0.5 * (S*S - Q).
    compute(ids[B, F], output_val[B, F, width], sum_val[B, width], fm_val[B, width]) -- or ids[n], output_val[n, width] with
    offsets[B + 1] for ragged bags.  With a device table it is the fused kernel (ops.embedding_lookup_fm): rows read once,
    written once.  On the PS, cache and prefetched paths the rows arrive in output_val exactly as EmbeddingLookUp delivers them
    and the same kernel runs over that buffer as a table (ids 0 .. n-1, no row store): every path agrees bit for bit on equal
    rows."""

    def forward_hook(self, config):
        super().forward_hook(config)
        self._rows_compute = self.compute
        self._fused = self._rows_compute == self._compute_gpu
        self._pos = None
        self.compute = self._compute_fm

    def _compute_fm(self, ids, output_val, sum_val, fm_val, stream=None, offsets=None):
        if self._fused:
            ops.embedding_lookup_fm(self.embedding.table, ids, offsets=offsets, rows_out=output_val, sum_out=sum_val,
                                    fm_out=fm_val, stream=stream)
            return output_val, sum_val, fm_val
        n, width = ids.numel(), self.embedding.shape[1]
        if self._pos is None or self._pos.numel() < n or self._pos.device != output_val.device:
            self._pos = torch.arange(max(n, 1), dtype=torch.int64, device=output_val.device)
        self._rows_compute(ids, output_val, stream)
        ops.embedding_lookup_fm(output_val.view(n, width), self._pos[:n].view(ids.shape), offsets=offsets, sum_out=sum_val,
                                fm_out=fm_val, want_rows=False, stream=stream)
        return output_val, sum_val, fm_val


class EmbeddingLookUpFM_Gradient:
    """The gradient of EmbeddingLookUpFM: the adjoints of the lookup's three consumers -- `vectors` (the gradient of the rows, or
    None when nothing consumed them) and `fm_grad` (the gradient of the FM output) with the forward's `rows` and `sum` -- are
    combined per occurrence by one launch (ops.fm_grad_rows, in place over `vectors` when given) and wrapped as ordinary
    UNPOOLED IndexedSlices: sgd_update_sparse, the fused optimizers and ParameterServerCommunicateOp take them as they take
    EmbeddingLookUp_Gradient's.  Push indices are handled as there."""

    def __init__(self, embed_shape, enable_push_index=False):
        self.embed_shape, self.enable_push_index = embed_shape, enable_push_index

    def compute(self, vectors, fm_grad, rows, sum, index, offsets=None, stream=None):
        push = None
        if isinstance(index, tuple):
            index, push = index[0], (index[1] if self.enable_push_index else None)
        elif self.enable_push_index:
            raise TypeError
        if offsets is None:
            if index.dim() != 2:
                raise ValueError("fixed bags need an index of shape [B, F]; give offsets for ragged bags")
            values = ops.fm_grad_rows(vectors, rows, sum, fm_grad, bag=index.shape[1], out=vectors, stream=stream)
        else:
            values = ops.fm_grad_rows(vectors, rows, sum, fm_grad, bag_of=ops.bag_of(offsets, index.numel(), stream=stream),
                                      out=vectors, stream=stream)
        return ops.IndexedSlices(indices=index, values=values, dense_shape=self.embed_shape, push_indices=push)


class EmbeddingLookUpFMSum(EmbeddingLookUp):
    """embedding_lookup_op(embedding, index) consumed as reduce_sum_op(axes=1) and reduce_sum_op(mul_op(e, e), axes=1) ONLY, the
    second-order term of the reference's pooled DeepFM (examples/ctr/models/emb_sum_deepfm_avazu.py, fae_deepfm_avazu.py):
    S feeds the DNN and S*S, nothing consumes the per-occurrence rows.  compute(ids[B, F], sum_val[B, width], fm_val[B, width])
    -- or ids[n] with offsets[B + 1] for ragged bags -- is ops.embedding_lookup_fm(want_rows=False): no [n, width] tensor.
    A device table only: on the PS and cache tiers the rows an update is applied to may have changed since the lookup, and what
    `e` means there is not decided."""

    def forward_hook(self, config):
        super().forward_hook(config)
        if self.compute != self._compute_gpu:
            raise ValueError("EmbeddingLookUpFMSum needs a device table (no PS, cache or prefetch tier): the pooled FM gradient "
                             "is a function of the table row at the time of the update")
        self.compute = self._compute_fm_sum

    def _compute_fm_sum(self, ids, sum_val, fm_val, stream=None, offsets=None):
        ops.embedding_lookup_fm(self.embedding.table, ids, offsets=offsets, sum_out=sum_val, fm_out=fm_val, want_rows=False,
                                stream=stream)
        return sum_val, fm_val


class EmbeddingLookUpFMSum_Gradient:
    """The gradient of EmbeddingLookUpFMSum: compute(sum_grad or None, fm_grad, sum, index) returns FM-POOLED IndexedSlices --
    values is the gradient of S ([B, width], None when nothing consumed S), fm_grad the gradient of the FM output and fm_sum the
    forward's S.  Nothing is computed here: the per-occurrence gradient (sum_grad[b] + fm_grad[b] * S[b]) - fm_grad[b] * e also
    depends on the row e, which sgd_update_sparse's fused apply holds in registers (ops.sgd_apply_fm_bags)."""

    def __init__(self, embed_shape):
        self.embed_shape = embed_shape

    def compute(self, sum_grad, fm_grad, sum, index, offsets=None, stream=None):
        if isinstance(index, tuple):
            raise TypeError("FM-pooled slices carry no push indices")
        if offsets is None:
            if index.dim() != 2:
                raise ValueError("fixed bags need an index of shape [B, F]; give offsets for ragged bags")
            return ops.IndexedSlices(indices=index, values=sum_grad, dense_shape=self.embed_shape, bag=index.shape[1],
                                     fm_grad=fm_grad, fm_sum=sum)
        return ops.IndexedSlices(indices=index, values=sum_grad, dense_shape=self.embed_shape,
                                 bag_of=ops.bag_of(offsets, index.numel(), stream=stream), offsets=offsets, fm_grad=fm_grad,
                                 fm_sum=sum)


class EmbeddingLookUpWeightedSum(EmbeddingLookUp):
    """embedding_lookup_op(embedding, index), mul_op by a per-occurrence weight and reduce_sum_op(axes=1): the embedding path of
    the reference's FAE models (examples/ctr/models/fae_wdl_criteo.py:19-31), where the weight is the 0/1 mask of the cold ids.
    compute(ids[B, F], weights[B, F], output_val[B, width]) -- or ids[n], weights[n] with offsets[B + 1] for ragged bags.  With a
    device table it is the fused kernel (ops.embedding_lookup_wsum): a dead occurrence (zero weight, or id >= rows) takes no
    part.  On the PS, cache and prefetched paths the per-occurrence rows arrive as EmbeddingLookUp delivers them and the same
    kernel sums them out of that row buffer (ids 0 .. n-1): every path agrees bit for bit on equal rows.  The plain PS
    flavour has a pooled weighted form (Config.ps_fuse_wbags): with prefetch the buffer of a communicate op that was given
    bag= and next_weights= already holds the weighted pooled rows (store.pull_wsum) and is copied as it is; without prefetch
    the rows come from store.pull_wsum directly, ragged bags included.  The cache's planned pairs have one too, opt-in
    (Config.cache_fuse_wbags: the op's buffer holds the rows of embedding_lookup_wsum_planned and is copied as it is); the other
    cache flows have none.  A communicate op that
    pulls rows pooled WITHOUT weights (bag= alone) cannot serve this operator and is refused."""

    def forward_hook(self, config):
        super().forward_hook(config)
        self._rows_compute = self.compute
        self._fused = self._rows_compute == self._compute_gpu
        self._pos = None
        self.compute = self._compute_wsum

    def _compute_wsum(self, ids, weights, output_val, stream=None, offsets=None):
        if self._fused:
            return ops.embedding_lookup_wsum(self.embedding.table, ids, weights, offsets=offsets, out=output_val, stream=stream)
        if getattr(self.config, "ps_pooled", {}).get(self.embedding) is not None:
            raise ValueError("EmbeddingLookUpWeightedSum: the communicate op pulls pooled rows (bag=%d), which carry no weights; "
                             "build it without bag=" % self.config.ps_pooled[self.embedding])
        wbag = getattr(self.config, "ps_wpooled", {}).get(self.embedding)
        if self._rows_compute == self._compute_prefetched and wbag is not None:
            if offsets is not None or ids.dim() != 2 or ids.shape[1] != wbag:
                raise ValueError("EmbeddingLookUpWeightedSum: the communicate op pulls weighted pooled rows for fixed bags of "
                                 "%d ids" % wbag)
            return self._compute_prefetched(ids, output_val, stream)      # a weighted pooled buffer, as it is
        if self._rows_compute == self._compute_sparsepull_from_ps and getattr(self.config, "ps_fuse_wbags", True):
            return self.embedding.store.pull_wsum(ids, weights.reshape(ids.shape), offsets=offsets, out=output_val)
        n, width = ids.numel(), self.embedding.shape[1]
        if self._pos is None or self._pos.numel() < n or self._pos.device != output_val.device:
            self._pos = torch.arange(max(n, 1), dtype=torch.int64, device=output_val.device)
        rows = torch.empty((n, width), dtype=torch.float32, device=output_val.device)
        self._rows_compute(ids, rows.view(tuple(ids.shape) + (width,)), stream)
        # (a row the store delivered as zeros for an id beyond the table is added as zeros times its weight: +0 or -0 into a
        # chain that starts at +0, which leaves every sum as it is)
        return ops.embedding_lookup_wsum(rows, self._pos[:n].view(ids.shape), weights, offsets=offsets, out=output_val,
                                         stream=stream)


class EmbeddingLookUpWeightedSum_Gradient:
    """The gradient of EmbeddingLookUpWeightedSum: compute(vectors[B, width], index, weights) returns WEIGHTED POOLED
    IndexedSlices -- values stay [B, width], the gradient of occurrence i is weights[i] * values[its bag].  sgd_update_sparse
    applies them fused (ops.sgd_apply_wbags); every other consumer expands them first (unweighted_slices)."""

    def __init__(self, embed_shape, enable_push_index=False):
        self.embed_shape, self.enable_push_index = embed_shape, enable_push_index

    def compute(self, vectors, index, weights, offsets=None):
        push = None
        if isinstance(index, tuple):
            index, push = index[0], (index[1] if self.enable_push_index else None)
        elif self.enable_push_index:
            raise TypeError
        if offsets is None:
            if index.dim() != 2:
                raise ValueError("fixed bags need an index of shape [B, F]; give offsets for ragged bags")
            return ops.IndexedSlices(indices=index, values=vectors, dense_shape=self.embed_shape, push_indices=push,
                                     bag=index.shape[1], weights=weights)
        return ops.IndexedSlices(indices=index, values=vectors, dense_shape=self.embed_shape, push_indices=push,
                                 bag_of=ops.bag_of(offsets, index.numel()), offsets=offsets, weights=weights)


class EmbeddingLookUpWeightedFMSum(EmbeddingLookUp):
    """embedding_lookup_op(embedding, index), mul_op by a per-occurrence weight, then reduce_sum_op(x, axes=1) and
    reduce_sum_op(mul_op(x, x), axes=1): the second-order term of the reference's FAE DeepFM
    (examples/ctr/models/fae_deepfm_avazu.py:43-80), which squares the sum only after the hot table's half has been added.
    compute(ids[B, F], weights[B, F], sum_val[B, width], sq_val[B, width]) -- or ids[n], weights[n] with offsets[B + 1] for
    ragged bags -- is ops.embedding_lookup_wfm: no [n, width] tensor.  A device table only: on the PS and cache tiers the rows
    an update is applied to may have changed since the lookup, and what `e` means there is not decided."""

    def forward_hook(self, config):
        super().forward_hook(config)
        if self.compute != self._compute_gpu:
            raise ValueError("EmbeddingLookUpWeightedFMSum needs a device table (no PS, cache or prefetch tier): the pooled FM "
                             "gradient is a function of the table row at the time of the update")
        self.compute = self._compute_wfm

    def _compute_wfm(self, ids, weights, sum_val, sq_val, stream=None, offsets=None):
        ops.embedding_lookup_wfm(self.embedding.table, ids, weights, offsets=offsets, sum_out=sum_val, sq_out=sq_val,
                                 stream=stream)
        return sum_val, sq_val


class EmbeddingLookUpWeightedFMSum_Gradient:
    """The gradient of EmbeddingLookUpWeightedFMSum: compute(sum_grad, sq_grad, index, weights) returns WEIGHTED FM-POOLED
    IndexedSlices -- values is the gradient of S, sq_grad the gradient of Q, both [B, width].  Nothing is computed here: the
    per-occurrence gradient w * (sum_grad[b] + 2 * sq_grad[b] * (w * e)) also depends on the row e, which sgd_update_sparse's
    fused apply holds in registers (ops.sgd_apply_wfm_bags)."""

    def __init__(self, embed_shape):
        self.embed_shape = embed_shape

    def compute(self, sum_grad, sq_grad, index, weights, offsets=None, stream=None):
        if isinstance(index, tuple):
            raise TypeError("weighted FM-pooled slices carry no push indices")
        if offsets is None:
            if index.dim() != 2:
                raise ValueError("fixed bags need an index of shape [B, F]; give offsets for ragged bags")
            return ops.IndexedSlices(indices=index, values=sum_grad, dense_shape=self.embed_shape, bag=index.shape[1],
                                     weights=weights, sq_grad=sq_grad)
        return ops.IndexedSlices(indices=index, values=sum_grad, dense_shape=self.embed_shape,
                                 bag_of=ops.bag_of(offsets, index.numel(), stream=stream), offsets=offsets, weights=weights,
                                 sq_grad=sq_grad)


def _masked_keys(ids, weights, rows):
    """Masked keys by the id rule of include/herald_amd.h ("Which ids name a row"), as wbag.hip builds them for fixed bags: the
    row of a live occurrence, `rows` for a dead one (zero weight, or an id that names no row)."""
    if ids.dtype == torch.float32:
        named = (ids > -1.0) & (ids < 4294967296.0)                  # NaN: False
        keys = torch.where(named, ids, torch.zeros_like(ids)).to(torch.int64)     # in-range values only; toward zero
    else:
        keys = ids.to(torch.int64)
        named = keys >= 0                                            # (a 64-bit id beyond 2^63 - 1 reads negative)
    return torch.where(named & (weights != 0) & (keys < rows), keys, torch.full_like(keys, rows))


def unweighted_slices(grad, stream=None):
    """Weighted pooled slices as ordinary UNPOOLED ones (values [n, width] = ops.wbag_grad_rows), anything else as it is.  The
    one door every consumer without a weighted form goes through -- the other optimizers, the communicate op's pushes, the
    fuse_bags branches -- so that a weight can never be silently dropped by a sum-pooled branch.  Weighted FM-pooled slices
    (sq_grad) have no expanded values and are refused here (IndexedSlices.expanded_values): their Q term is never dropped."""
    if not getattr(grad, "weighted", False):
        return grad
    return ops.IndexedSlices(indices=grad.indices, values=grad.expanded_values(stream), dense_shape=grad.dense_shape,
                             push_indices=grad.push_indices)


def _refuse_fm_pooled(name, grad):
    """FM-pooled slices must never fall into a sum-pooled branch: it would silently drop the row term of the gradient."""
    if getattr(grad, "fm_pooled", False):
        raise ValueError("%s: FM-pooled slices (EmbeddingLookUpFMSum_Gradient) are taken by sgd_update_sparse on a device "
                         "table only: the gradient of an occurrence depends on its table row" % name)
    if getattr(grad, "weighted_fm", False):
        raise ValueError("%s: weighted FM-pooled slices (EmbeddingLookUpWeightedFMSum_Gradient) are taken by sgd_update_sparse "
                         "on a device table only: the gradient of an occurrence depends on its table row" % name)


def sgd_update_sparse(param, grad, lr, stream=None):
    """OptimizerOp's sparse SGD branch on a device table (_sgd_update_sparse), with `stream` as torch's current stream while it
    runs: the .contiguous() copies, the masked keys and the temporary plans of the ragged branches are enqueued on, and
    allocated in the order of, the stream of the launches (the stream contract, ops.py)."""
    dev = param.table.device if param.table is not None else None
    with ops.on_stream(stream, dev):
        _sgd_update_sparse(param, grad, lr, stream)


def _sgd_update_sparse(param, grad, lr, stream):
    """OptimizerOp's sparse SGD branch on a device table (OptimizerLink.py:23-33): no dedup, duplicates in
    occurrence order.  Pooled slices (EmbeddingLookUpSum_Gradient) go to the bag apply: no expanded gradient is built.
    FM-pooled slices (EmbeddingLookUpFMSum_Gradient) go to the fused FM apply: the one-call form for fixed bags, sort + finish +
    ops.sgd_apply_fm_bags for ragged ones.  Weighted FM-pooled slices (EmbeddingLookUpWeightedFMSum_Gradient) go to the fused
    weighted FM apply over masked keys, ahead of the weighted branch."""
    if getattr(grad, "fm_pooled", False):
        if param.table is None:
            raise ValueError("sgd_update_sparse: FM-pooled slices need a device table")
        width = param.table.shape[1]
        g_sum = grad.values.reshape(-1, width).contiguous() if grad.values is not None else None
        g_fm, fm_sum = grad.fm_grad.reshape(-1, width).contiguous(), grad.fm_sum.reshape(-1, width).contiguous()
        if grad.bag is not None:
            ops.sgd_sparse_update_fm_bags(param.table, grad.indices.reshape(-1, int(grad.bag)).contiguous(), g_sum, g_fm, fm_sum,
                                          lr, stream=stream)
        else:
            ids = grad.indices.reshape(-1).contiguous()
            plan = ops.IndexPlan.temporary(max(ids.numel(), 1), ids.device, ops._torch_stream(stream, ids.device))
            plan.sort(ids, stream).finish(stream)
            ops.sgd_apply_fm_bags(param.table, plan, g_sum, g_fm, fm_sum, lr, bag_of=grad.bag_of, stream=stream)
        return
    if getattr(grad, "weighted_fm", False):
        # weighted FM-pooled slices (EmbeddingLookUpWeightedFMSum_Gradient), before the weighted branch, which would drop the Q
        # term: the one-call form for fixed bags; masked keys + sort + finish + ops.sgd_apply_wfm_bags for ragged ones
        if param.table is None:
            raise ValueError("sgd_update_sparse: weighted FM-pooled slices need a device table")
        table = param.table
        width = table.shape[1]
        g_sum, g_sq = grad.values.reshape(-1, width).contiguous(), grad.sq_grad.reshape(-1, width).contiguous()
        weights = grad.weights.reshape(-1).contiguous()
        if grad.bag is not None:
            ops.sgd_sparse_update_wfm_bags(table, grad.indices.reshape(-1, int(grad.bag)).contiguous(), g_sum, g_sq, weights, lr,
                                           stream=stream)
        else:
            keys = _masked_keys(grad.indices.reshape(-1).contiguous(), weights, table.shape[0])
            plan = ops.IndexPlan.temporary(max(keys.numel(), 1), keys.device, ops._torch_stream(stream, keys.device))
            plan.sort(keys, stream, key_limit=table.shape[0])
            ops.sgd_apply_wfm_bags(table, plan.finish(stream), g_sum, g_sq, weights, lr, bag_of=grad.bag_of, stream=stream)
        return
    if getattr(grad, "weighted", False):
        # weighted pooled slices (EmbeddingLookUpWeightedSum_Gradient): the fused weighted apply over masked keys -- the one-call
        # form for fixed bags; mask + sort + finish + ops.sgd_apply_wbags for ragged ones
        if param.table is None:
            raise ValueError("sgd_update_sparse: weighted pooled slices need a device table")
        table = param.table
        width = table.shape[1]
        values = grad.values.reshape(-1, width).contiguous()
        weights = grad.weights.reshape(-1).contiguous()
        if grad.bag is not None:
            ops.sgd_sparse_update_wbags(table, grad.indices.reshape(-1, int(grad.bag)).contiguous(), values, weights, lr,
                                        stream=stream)
        else:
            keys = _masked_keys(grad.indices.reshape(-1).contiguous(), weights, table.shape[0])
            plan = ops.IndexPlan.temporary(max(keys.numel(), 1), keys.device, ops._torch_stream(stream, keys.device))
            plan.sort(keys, stream, key_limit=table.shape[0])
            ops.sgd_apply_wbags(table, plan.finish(stream), values, weights, lr, bag_of=grad.bag_of, stream=stream)
        return
    if getattr(grad, "pooled", False):
        width = param.table.shape[1]
        values = grad.values.reshape(-1, width).contiguous()
        if grad.bag is not None:
            ops.sgd_sparse_update_bags(param.table, grad.indices.reshape(-1, int(grad.bag)).contiguous(), values, lr,
                                       stream=stream)
        else:
            ids = grad.indices.reshape(-1).contiguous()
            plan = ops.IndexPlan.temporary(max(ids.numel(), 1), ids.device, ops._torch_stream(stream, ids.device))
            plan.sort(ids, stream)
            ops.sgd_apply_bags(param.table, plan, values, lr, bag_of=grad.bag_of, stream=stream)
        return
    ops.dl_call("SGDOptimizerSparseUpdate",
                [param.table, grad.indices.contiguous(), grad.values.reshape(-1, param.table.shape[1]).contiguous()],
                scalars=[ctypes.c_float(lr)], stream=stream)


# ---- the sparse branches of the other optimizers (OptimizerLink.py:37-100), on a device table ----------------------------
def _sparse_args(name, param, grad, states):
    """Shape checks shared by the *_update_sparse functions below (no native call is made before they pass).  Returns
    (table, width)."""
    _refuse_fm_pooled(name, grad)
    table = param.table
    if table is None or table.dim() != 2:
        raise ValueError("%s: the parameter must hold a 2-D device table" % name)
    width = table.shape[1]
    for what, st in states:
        if st is None or tuple(st.shape) != tuple(table.shape) or st.dtype != table.dtype:
            raise ValueError("%s: %s must be a float32 tensor of the table's shape %s" % (name, what, tuple(table.shape)))
    if grad.indices is None or grad.values is None:
        raise ValueError("%s: the gradient has no indices / values" % name)
    if grad.values.dim() < 1 or grad.values.shape[-1] != width:
        raise ValueError("%s: gradient rows must be %d wide, got %s" % (name, width, tuple(grad.values.shape)))
    n = grad.indices.numel()
    nrows = grad.values.numel() // width
    if not getattr(grad, "pooled", False):
        if nrows != n:
            raise ValueError("%s: %d gradient rows for %d indices" % (name, nrows, n))
    elif grad.bag is not None:
        if int(grad.bag) < 1 or n != nrows * int(grad.bag):
            raise ValueError("%s: %d indices are not %d bags of %s ids" % (name, n, nrows, grad.bag))
    else:
        if grad.bag_of.numel() != n:
            raise ValueError("%s: bag_of must have one entry per index" % name)
        if grad.offsets is not None and grad.offsets.numel() != nrows + 1:
            raise ValueError("%s: offsets must have one entry per gradient row and one more" % name)
    return table, width


def _reference_slices(grad, width, dedup, stream):
    """The reference's own sequence on a copy of the slices: reduce_sum's broadcast gradient (expanded_values), then
    IndexedSlices.deduplicate for the optimizers that ask for it.  Returns (indices [m], values [m, width])."""
    ref = ops.IndexedSlices(indices=grad.indices.reshape(-1).contiguous(), values=grad.expanded_values(stream),
                            dense_shape=grad.dense_shape)
    if dedup:
        ref.deduplicate(stream)
    return ref.indices.reshape(-1).contiguous(), ref.values.reshape(-1, width).contiguous()


def _bag_call_args(name, grad, width):
    """(ids, offsets, values) as the one-call bag optimizers of ops take them."""
    values = grad.values.reshape(-1, width).contiguous()
    if grad.bag is not None:
        return grad.indices.reshape(-1, int(grad.bag)).contiguous(), None, values
    if grad.offsets is None:
        raise ValueError("%s: ragged pooled slices need their offsets (EmbeddingLookUpSum_Gradient attaches them); "
                         "fuse_bags=False takes bag_of alone" % name)
    return grad.indices.reshape(-1).contiguous(), grad.offsets, values


def momentum_update_sparse(param, grad, velocity, lr, momentum, nesterov, stream=None, fuse_bags=True):
    """momentum_update's sparse branch (OptimizerLink.py:37-49): MomentumOptimizerSparseUpdate WITHOUT deduplication.
    Pooled slices go to ops.momentum_sparse_update_bags -- no expanded gradient is built; fuse_bags=False runs the reference's
    sequence (expanded_values, then the symbol): the same bits.  Weighted pooled slices are expanded first (unweighted_slices)."""
    with ops.on_stream(stream, param.table.device if param.table is not None else None):
        _momentum_update_sparse(param, grad, velocity, lr, momentum, nesterov, stream, fuse_bags)


def _momentum_update_sparse(param, grad, velocity, lr, momentum, nesterov, stream, fuse_bags):
    grad = unweighted_slices(grad, stream)
    table, width = _sparse_args("momentum_update_sparse", param, grad, [("velocity", velocity)])
    if fuse_bags and getattr(grad, "pooled", False):
        ids, offsets, values = _bag_call_args("momentum_update_sparse", grad, width)
        ops.momentum_sparse_update_bags(table, ids, values, velocity, lr, momentum, nesterov, offsets=offsets, stream=stream)
        return
    ids, values = _reference_slices(grad, width, False, stream)
    ops.dl_call("MomentumOptimizerSparseUpdate", [table, ids, values, velocity],
                scalars=[ctypes.c_float(lr), ctypes.c_float(momentum), ctypes.c_bool(bool(nesterov))], stream=stream)


def _fused_update_sparse(name, kind, symbol, param, grad, state1, state2, hyper, scalars, stream, fuse_bags):
    with ops.on_stream(stream, param.table.device if param.table is not None else None):      # (as sgd_update_sparse)
        _fused_update_sparse_on(name, kind, symbol, param, grad, state1, state2, hyper, scalars, stream, fuse_bags)


def _fused_update_sparse_on(name, kind, symbol, param, grad, state1, state2, hyper, scalars, stream, fuse_bags):
    states = [("the first state", state1)] + ([("the second state", state2)] if kind != "adagrad" else [])
    grad = unweighted_slices(grad, stream)      # weighted pooled slices: expanded first, whatever fuse_bags says
    table, width = _sparse_args(name, param, grad, states)
    if not fuse_bags:        # the reference: deduplicate (on the expanded gradient), then the symbol on the reduced slices
        ids, values = _reference_slices(grad, width, True, stream)
        arrays = [table, ids, values, state1] + ([state2] if kind != "adagrad" else [])
        ops.dl_call(symbol, arrays, scalars=[ctypes.c_float(x) for x in scalars], stream=stream)
        return
    if getattr(grad, "pooled", False):
        ids, offsets, values = _bag_call_args(name, grad, width)
        ops.sparse_opt_fused_bags(kind, table, ids, values, state1, state2, offsets=offsets, stream=stream, **hyper)
        return
    ops.sparse_opt_fused(kind, table, grad.indices.reshape(-1).contiguous(), grad.values.reshape(-1, width).contiguous(),
                         state1, state2, stream=stream, **hyper)


def adagrad_update_sparse(param, grad, accumulation, lr, eps, stream=None, fuse_bags=True):
    """adagrad_update's sparse branch (OptimizerLink.py:52-66): grad.deduplicate + AdaGradOptimizerSparseUpdate, as ONE fused
    call on the raw ids (ops.sparse_opt_fused) -- for pooled slices on the pooled gradient (ops.sparse_opt_fused_bags).
    fuse_bags=False: the reference's own sequence (expanded_values, deduplicate, the symbol); the same bits."""
    _fused_update_sparse("adagrad_update_sparse", "adagrad", "AdaGradOptimizerSparseUpdate", param, grad, accumulation, None,
                         dict(lr=lr, eps=eps), [lr, eps], stream, fuse_bags)


def adam_update_sparse(param, grad, expavg, expavgsq, lr, beta1, beta2, beta1t, beta2t, eps, stream=None, fuse_bags=True):
    """adam_update's sparse branch (OptimizerLink.py:69-84), fused as adagrad_update_sparse is."""
    _fused_update_sparse("adam_update_sparse", "adam", "AdamOptimizerSparseUpdate", param, grad, expavg, expavgsq,
                         dict(lr=lr, eps=eps, beta1=beta1, beta2=beta2, beta1t=beta1t, beta2t=beta2t),
                         [lr, beta1, beta2, beta1t, beta2t, eps], stream, fuse_bags)


def adamw_update_sparse(param, grad, expavg, expavgsq, lr, beta1, beta2, beta1t, beta2t, eps, weight_decay, stream=None,
                        fuse_bags=True):
    """adamw_update's sparse branch (OptimizerLink.py:86-100), fused as adagrad_update_sparse is."""
    _fused_update_sparse("adamw_update_sparse", "adamw", "AdamWOptimizerSparseUpdate", param, grad, expavg, expavgsq,
                         dict(lr=lr, eps=eps, beta1=beta1, beta2=beta2, beta1t=beta1t, beta2t=beta2t,
                              weight_decay=weight_decay),
                         [lr, beta1, beta2, beta1t, beta2t, eps, weight_decay], stream, fuse_bags)


class ParameterServerCommunicateOp:
    def __init__(self, parameter, learning_rate, next_ids, peek_ids=None, bag=None, next_weights=None):
        """peek_ids(j) (optional, Config.cache_plan_ahead): the ids of the batch j batches after the one next_ids() returns
        (peek_ids(0) = that batch itself), without advancing the loader; None when there is none.
        bag (optional): the embedding is read through a sum-pooled lookup (EmbeddingLookUpSum) with fixed bags of `bag` ids --
        ids arrive as [B, bag].  With the cache's planned flow (the pairs at bsp 0, the LRU push-pull chain of the asp schedule)
        and Config.cache_fuse_bags, or on the plain PS flavour with Config.ps_fuse_bags, the op then keeps sparse_pull_val as
        [B, width] and moves pooled rows and pooled gradients only; so it does on the call-by-call cache flows (no plan-ahead,
        LFU / LFUOpt at bsp < 0, the cache over a sharded store, laia push plans) with Config.cache_fuse_bag_calls; on every
        other path it changes nothing.
        Without bag= the op's pulls and pushes are per occurrence as they always were; the lookup without prefetch
        (EmbeddingLookUpSum -> store.pull_sum) does not pass through this op and follows Config.ps_fuse_bags alone.
        next_weights (optional, with bag=): the embedding is read through a WEIGHTED sum-pooled lookup
        (EmbeddingLookUpWeightedSum); next_weights() returns the weights [B, bag] of the batch that the latest next_ids() call
        returned.  On the plain PS flavour with Config.ps_fuse_wbags the op then pulls weighted pooled rows
        (store.pull_wsum; sparse_pull_val is [B, width], recorded in config.ps_wpooled, not ps_pooled) and pushes weighted
        pooled slices as they are, -lr included (store.push_wbags); with ps_fuse_wbags=False it moves per-occurrence rows and
        the expanded gradient, as an op without bag= does (rows pooled without weights would be wrong for this lookup).  On the
        cache flavour the planned pairs have a pooled weighted form under Config.cache_fuse_wbags (bsp == 0, prefetch,
        cache_plan_ahead, world size 1, peek_ids): embedding_lookup_wsum_planned / embedding_update_planned_wbags; every other
        cache configuration refuses next_weights.  Without bag= it is ignored."""
        self.parameter = parameter
        self.learning_rate = -learning_rate                           # :24
        self.next_ids = next_ids
        self.next_weights = next_weights
        self.peek_ids = peek_ids
        self._peek_offset = 1
        self.bag = int(bag) if bag is not None else None
        self._bag = None              # the bag size while pooled rows are pulled and pushed (forward_hook decides)
        self._ps_bags = False         # ... by the plain PS flavour (store.pull_sum / push_bags)
        self._ps_wbags = False        # ... weighted, by the plain PS flavour (store.pull_wsum / push_wbags)
        self._first_weights = None    # the weights of an explicit first batch (forward_hook(first_ids=, first_weights=))
        self._planned = None          # the planned flow: (ids, push plan or None) of the planned batches, oldest first
        self._chain = False           # the planned flow of the asp schedule: _planned = ids of a push-pull chain's batches
        self._bag_calls = False       # pooled rows through the call-by-call cache (Config.cache_fuse_bag_calls)
        self._cache_wbags = False     # weighted pooled rows through the cache's planned pairs (Config.cache_fuse_wbags)

    def forward_hook(self, config, first_ids=None, barrier=lambda: None, first_weights=None):   # :130-242
        self.config, self.barrier = config, barrier
        p = self.parameter
        self.use_cache_table = config.cstable_policy is not None and p.is_embed
        cache_wbags = False
        if self.use_cache_table and self.next_weights is not None and self.bag is not None:
            cache_wbags = bool(getattr(config, "cache_fuse_wbags", False)) and config.bsp == 0 and bool(config.prefetch) and \
                bool(getattr(config, "cache_plan_ahead", False)) and p.store.world == 1 and self.peek_ids is not None
        if self.use_cache_table and self.next_weights is not None and not cache_wbags:
            raise ValueError("ParameterServerCommunicateOp(next_weights=): the cache tiers have a pooled weighted form in the "
                             "planned pairs only -- Config(cache_fuse_wbags=True) with bsp == 0, prefetch, cache_plan_ahead, "
                             "world size 1, peek_ids and bag= --; otherwise build the op without next_weights (weighted slices "
                             "are then expanded before every push)")
        if cache_wbags and first_ids is not None and first_weights is None:
            raise ValueError("ParameterServerCommunicateOp(next_weights=): first_ids come with first_weights")
        if self.use_cache_table:
            width = p.shape[1]
            store = p.store
            if store.world > 1:
                # the table is sharded over the ranks: the cache talks to the owners through the inbox /
                # outbox exchange (remote_store.ShardedStore) -- only misses, stale lines and pushed lines
                # cross the fabric (PSAgent.h:537-627 / PSFhandle_embedding.cc:5-79)
                from . import remote_store
                versions = torch.zeros(store.local_rows, dtype=torch.int64, device=store.table.device)
                torch.cuda.current_stream(versions.device).synchronize()
                rstore = remote_store.ShardedStore(p.shape[0], width, store.table.device,
                                                   remote_store.LocalStore(store.table, versions),
                                                   group=store.group, a2a=store._a2a_fn)
                cls = {"lru": hcache.LRUCache, "lfu": hcache.LFUCache, "lfuopt": hcache.LFUOptCache}[
                    config.cstable_policy.lower()]
                raw = cls(config.cache_limit, p.shape[0], width, node_id=-1 - p.id, device=store.table.device)
                raw.pull_bound = raw.push_bound = config.cache_bound
                raw.bind_remote(rstore)
                self.cache = hcache.CacheSparseTable.wrap(raw)
                self.remote_store = rstore
            else:
                hcache.register_table(p.id, store.table, row_start=store.starts[store.rank])
                self.cache = hcache.CacheSparseTable(config.cache_limit, p.shape[0], width, p.id,
                                                     config.cstable_policy, config.cache_bound,
                                                     device=store.table.device)
            p.cache = self.cache
            if getattr(config, "cache_perf_enable", False):
                self.cache.perf_enabled(True)
            self._push, self._pull, self._push_pull = self._push_cache, self._pull_cache, self._push_pull_cache
            if config.bsp == 0 and config.prefetch:
                self.compute = self._compute_bsp_prefetch
                if getattr(config, "cache_plan_ahead", False) and store.world == 1 and self.peek_ids is not None:
                    self._planned = []        # pull(k + 1) follows push(k) of the same ids batch after batch: the planned pairs
                    if cache_wbags:           # ... weighted pooled: embedding_lookup_wsum_planned / _update_planned_wbags
                        self._bag, self._cache_wbags = self.bag, True
                        self._first_weights = first_weights if first_ids is not None else None
                    elif self.bag is not None and getattr(config, "cache_fuse_bags", True):
                        self._bag = self.bag
            elif config.prefetch:
                self.compute = self._compute_asp_prefetch
                if getattr(config, "cache_plan_ahead", False) and store.world == 1 and self.peek_ids is not None and \
                        config.cstable_policy.lower() == "lru":
                    # every step is ONE cache call, push_pull(pull = batch k + 1, push = batch k): the planned push-pull chain
                    # (LRU; LFU / LFUOpt keep the call-by-call embedding_push_pull)
                    self._planned, self._chain = [], True
                    if self.bag is not None and getattr(config, "cache_fuse_bags", True):
                        self._bag = self.bag      # ... with pooled entries: embedding_push_pull_planned_bags
            else:
                self.compute = self._compute_no_prefetch
            if config.prefetch and self._planned is None and self.bag is not None and \
                    getattr(config, "cache_fuse_bag_calls", False):
                self._bag, self._bag_calls = self.bag, True       # the call-by-call flow, pooled
        else:
            self._push, self._pull, self._push_pull = self._push_sparse, self._pull_sparse, self._push_pull_sparse
            if self.bag is not None and self.next_weights is not None:
                if getattr(config, "ps_fuse_wbags", True):
                    self._bag, self._ps_wbags = self.bag, True
                    if config.prefetch and first_ids is not None:
                        if first_weights is None:
                            raise ValueError("ParameterServerCommunicateOp(next_weights=): first_ids come with first_weights")
                        self._first_weights = first_weights
            elif self.bag is not None and getattr(config, "ps_fuse_bags", True):
                self._bag, self._ps_bags = self.bag, True
            # :235-242: bsp >= 0 -> ssp (push, ssp_sync(version), pull), else asp (push_pull) when prefetching
            if config.prefetch and config.bsp >= 0:
                self.compute = self._compute_ssp_prefetch
                self.ssp_version = 0
            elif config.prefetch:
                self.compute = self._compute_asp_prefetch
            else:
                self.compute = self._compute_no_prefetch
        if config.prefetch:                                            # first prefetch (:168-176, 196-205)
            ids = first_ids if first_ids is not None else self.next_ids()
            # a laia data loader hands over (ids, push plan): cstable.py:49 (the planned flow plans the batch with its plan)
            first = ids[0] if isinstance(ids, tuple) else ids
            if self._bag is not None:
                if first.dim() != 2 or first.shape[1] != self._bag:
                    raise ValueError("ParameterServerCommunicateOp(bag=%d): ids must be [B, %d], got %s"
                                     % (self._bag, self._bag, tuple(first.shape)))
                self.sparse_pull_val = torch.empty((first.shape[0], p.shape[1]), dtype=torch.float32, device=first.device)
                if self._ps_wbags or self._cache_wbags:
                    config.ps_wpooled[p] = self._bag
                else:
                    config.ps_pooled[p] = self._bag
            else:
                self.sparse_pull_val = torch.empty(tuple(first.shape) + (p.shape[1],), dtype=torch.float32,
                                                   device=first.device)
            if self._planned is None:
                ids = first
            # (peek_ids counts from the batch next_ids() returns: an explicit first batch is the one before it)
            self._peek_offset = 0 if first_ids is not None else 1
            config.ps_map[p] = (self._pull(ids), self.sparse_pull_val)
            self._peek_offset = 1

    # -- compute variants (:37-56)
    def _per_occurrence(self, grad):
        """Pooled slices (the gradient of EmbeddingLookUpSum: one row per bag) are expanded to per-occurrence values before
        they are pushed -- what reduce_sum_op's broadcast gradient hands the reference's communicate op.  The step engines are
        NOT fused for pooled access, and the call-by-call cache is only with Config.cache_fuse_bag_calls (off by default):
        otherwise they move the expanded [n, width] values as they always did.  The cache's planned flow -- pairs and the asp
        chain -- (Config.cache_fuse_bags), the call-by-call cache under its switch and the plain PS flavour
        (Config.ps_fuse_bags) are: slices
        pooled by the op's own bag size stay [B, width] -- on the PS flavour ragged slices that carry their offsets too --;
        -lr is applied to those rows only, which is the same product for every occurrence of a bag.
        FM-pooled slices are refused: the rows a push is applied to may have changed since the lookup.  Weighted pooled slices
        (EmbeddingLookUpWeightedSum_Gradient) stay pooled on the plain PS flavour when the op pulls weighted pooled rows (bag=
        and next_weights=, Config.ps_fuse_wbags) and their bag is the op's, or they are ragged and carry offsets; everywhere else
        they are expanded first.  Such an op expands every OTHER pooled slice: its pushes have no unweighted pooled form."""
        _refuse_fm_pooled("ParameterServerCommunicateOp", grad)
        if self._ps_wbags and getattr(grad, "weighted", False) and \
                (grad.bag == self._bag if grad.bag is not None else grad.offsets is not None):
            return grad
        if self._cache_wbags:
            # the pull buffer holds weighted pooled rows of bags of self._bag ids: the gradients are the weighted slices of
            # that bag size and nothing else (as _pooled_by_bag for its flow); they stay pooled, -lr goes into the push
            if not (getattr(grad, "weighted", False) and grad.bag == self._bag):
                raise RuntimeError("ParameterServerCommunicateOp (cache_fuse_wbags, bag=%d): the pull buffer holds weighted "
                                   "pooled rows, so the gradients must be the weighted slices of "
                                   "EmbeddingLookUpWeightedSum_Gradient over bags of %d ids; use cache_fuse_wbags=False and no "
                                   "next_weights for other gradients" % (self._bag, self._bag))
            return grad
        grad = unweighted_slices(grad)
        if not getattr(grad, "pooled", False):
            return grad
        if self._bag is not None and grad.bag == self._bag and not self._ps_wbags:
            return grad
        if self._ps_bags and grad.bag is None and grad.offsets is not None:
            return grad
        return ops.IndexedSlices(indices=grad.indices, values=grad.expanded_values(), dense_shape=grad.dense_shape,
                                 push_indices=grad.push_indices)

    def _mult_lr(self, grad):
        if (self._ps_wbags or self._cache_wbags) and getattr(grad, "weighted", False):
            # (what _per_occurrence left weighted: -lr goes to push_wbags, which rounds fl(-lr * fl(w * g)) as wbag_grad_rows,
            # scale_ and a push with scale 1 do; the caller's values and weights are not written)
            return
        scale_(grad.values, self.learning_rate)

    def _compute_asp_prefetch(self, grad):
        grad = self._per_occurrence(grad)
        self._mult_lr(grad)
        self.config.ps_map[self.parameter] = (self._push_pull(grad), self.sparse_pull_val)

    def _compute_ssp_prefetch(self, grad):
        """:41-46.  ssp_sync(version) lets a worker run ahead of the slowest one by at most `bsp` versions
        (ps-lite/include/ps/server/ssp_handler.h:41-67).  The sparse push / pull of a sharded store are
        collectives over all ranks, so no rank can run ahead at all: every tolerance is served by the
        lock step of the exchange itself, which satisfies the bound; only the version counter is kept."""
        grad = self._per_occurrence(grad)
        self._mult_lr(grad)
        w = self._push(grad)
        if w is not None:
            w.wait()
        self.barrier()
        self.config.ps_map[self.parameter] = (self._pull(self.next_ids()), self.sparse_pull_val)
        self.ssp_version += 1

    def _compute_bsp_prefetch(self, grad):
        grad = self._per_occurrence(grad)
        self._mult_lr(grad)
        w = self._push(grad)
        if w is not None:
            w.wait()
        self.barrier()
        self.config.ps_map[self.parameter] = (self._pull(self.next_ids()), self.sparse_pull_val)

    def _compute_no_prefetch(self, grad):
        grad = self._per_occurrence(grad)
        self._mult_lr(grad)
        w = self._push(grad)
        if w is not None:
            w.wait()

    # -- cache flavour (:68-72, 88-92, 104-105)
    def _pooled_by_bag(self, grad):
        """Call-by-call pooled flow: the pull buffer holds pooled rows, so the gradients are the pooled slices of this bag size."""
        if not (getattr(grad, "pooled", False) and grad.bag == self._bag):
            raise RuntimeError("ParameterServerCommunicateOp (cache_fuse_bag_calls, bag=%d): the pull buffer holds pooled rows, "
                               "so the gradients must be the pooled slices of EmbeddingLookUpSum_Gradient over bags of %d ids; "
                               "use cache_fuse_bag_calls=False for per-occurrence gradients" % (self._bag, self._bag))

    def _push_cache(self, grad):
        vals = grad.values.reshape(-1, self.parameter.shape[1])
        if self._bag_calls:
            self._pooled_by_bag(grad)
            idx = grad.indices.reshape(-1)
            if grad.push_indices is None:
                return self.cache.embedding_update_bags(idx, vals.contiguous(), bag=self._bag,
                                                        same_as_lookup=self.cache.looked_up_last(idx))
            return self.cache.embedding_update_with_push_keys_bags(idx, grad.push_indices.reshape(-1), vals.contiguous(),
                                                                   bag=self._bag)
        if self._planned is not None:
            idx = grad.indices.reshape(-1)
            pk = grad.push_indices.reshape(-1) if grad.push_indices is not None else None
            if not self._planned or not _same_tensor(self._planned[0][0], idx) or (pk is None) != (self._planned[0][1] is None) \
                    or (pk is not None and not _same_tensor(self._planned[0][1], pk)):
                raise RuntimeError("ParameterServerCommunicateOp (cache_plan_ahead): the gradients pushed are not those of the "
                                   "batch pulled last, or not with the push plan it was planned with")
            self._planned.pop(0)
            if self._cache_wbags:      # (what _per_occurrence left weighted: vals is [B, width]; learning_rate is -lr)
                return self.cache.embedding_update_planned_wbags(vals.contiguous(), grad.weights.reshape(-1).contiguous(),
                                                                 bag=self._bag, scale=self.learning_rate)
            if self._bag is not None and getattr(grad, "pooled", False):      # vals is [B, width]: one row per bag
                return self.cache.embedding_update_planned_bags(vals.contiguous(), bag=self._bag)
            return self.cache.embedding_update_planned(vals)     # (a planned plan: cache.cc:248-335, _embeddingUpdateWithPushKeys)
        if grad.push_indices is None:
            # The executor pushes the gradients of the batch it looked up last (bsp / ssp: push(k) follows pull(k) as the
            # cache's next operation, ParameterServerCommunicate.py:41-56) and does not write the ids in between: when the
            # indices ARE that lookup's tensor the update reuses its index plan (and takes the two-launch path).
            idx = grad.indices.reshape(-1)
            return self.cache.embedding_update(idx, vals, same_as_lookup=self.cache.looked_up_last(idx))
        return self.cache.embedding_update_with_push_keys(grad.indices.reshape(-1), grad.push_indices.reshape(-1), vals)

    def _plan(self, batch):
        """Plan one batch: ids alone (the bounded push), or (ids, push plan) of a laia-scheduled batch (its update pushes the
        plan's keys, cache.cc:248-335).  The op cannot know where a loader's tensor came from (an upload or `ids % rows` on the
        current stream): a pair block is planned with after_current=True, so the planning stream reads the ids behind
        everything queued on the cache's stream (one event record and wait per planned batch; its cost is not measured)."""
        if isinstance(batch, tuple):
            ids, plan = batch[0].reshape(-1), batch[1].reshape(-1)
            self.cache.plan_block([ids], push_keys_list=[plan])
        else:
            ids, plan = batch.reshape(-1), None
            self.cache.plan_block([ids], after_current=True)
        self._planned.append((ids, plan))

    def _pull_cache(self, ids):
        dest = self.sparse_pull_val.reshape(-1, self.parameter.shape[1])
        if self._chain:
            # the chain's head (the first prefetch): this batch and the next one are planned, this one is looked up
            if isinstance(ids, tuple):
                raise RuntimeError("ParameterServerCommunicateOp (cache_plan_ahead, asp): push plans (laia) are not part of the "
                                   "planned push-pull chain")
            if self._planned:
                raise RuntimeError("ParameterServerCommunicateOp (cache_plan_ahead, asp): only the first pull is a plain lookup")
            self._plan_chain(ids)
            nxt = self.peek_ids(self._peek_offset)
            if nxt is not None:
                self._plan_chain(nxt)
            if self._bag is not None:                              # dest is [B, width]: the head, pooled
                return self.cache.embedding_push_pull_planned_bags(dest, None, bag=self._bag)
            return self.cache.embedding_lookup_planned(dest)
        if self._planned is not None:
            if not self._planned:                                  # the first pull: nothing planned yet
                self._plan(ids)
            flat = (ids[0] if isinstance(ids, tuple) else ids).reshape(-1)
            plan = ids[1].reshape(-1) if isinstance(ids, tuple) else None
            if len(self._planned) != 1 or not _same_tensor(self._planned[0][0], flat) or \
                    (plan is None) != (self._planned[0][1] is None) or (plan is not None and not _same_tensor(self._planned[0][1], plan)):
                raise RuntimeError("ParameterServerCommunicateOp (cache_plan_ahead): pulls and pushes must alternate, batch "
                                   "after batch, on the tensors the loader handed out")
            nxt = self.peek_ids(self._peek_offset)                 # the batch after this one: its bookkeeping runs from now on,
            if nxt is not None:                                    # beside this batch's rows and the model's step
                self._plan(nxt)
            if self._cache_wbags:
                shaped = ids[0] if isinstance(ids, tuple) else ids
                if shaped.dim() != 2 or shaped.shape[1] != self._bag:
                    raise ValueError("ParameterServerCommunicateOp(bag=%d): ids must be [B, %d], got %s"
                                     % (self._bag, self._bag, tuple(shaped.shape)))
                weights, self._first_weights = self._first_weights, None
                if weights is None:
                    weights = self.next_weights()      # of the batch the latest next_ids() call returned: these ids
                return self.cache.embedding_lookup_wsum_planned(dest, weights.reshape(-1).contiguous(), bag=self._bag)
            if self._bag is not None:
                return self.cache.embedding_lookup_sum_planned(dest, bag=self._bag)
            return self.cache.embedding_lookup_planned(dest)      # (no next batch: the next pull plans for itself)
        if isinstance(ids, tuple):              # (ids, push plan) of a laia-scheduled batch (cstable.py:49)
            ids = ids[0]
        if self._bag_calls:                     # dest is [B, width]
            return self.cache.embedding_lookup_sum(ids.reshape(-1), dest, bag=self._bag)
        return self.cache.embedding_lookup(ids.reshape(-1), dest)

    def _plan_chain(self, ids):
        if isinstance(ids, tuple):
            raise RuntimeError("ParameterServerCommunicateOp (cache_plan_ahead, asp): push plans (laia) are not part of the "
                               "planned push-pull chain")
        ids = ids.reshape(-1)
        self.cache.plan_block([ids], push_pull=True)
        self._planned.append(ids)

    def _push_pull_planned(self, grad):
        """One step of the planned push-pull chain: the gradients are those of the batch pulled last, the batch after next is
        planned from peek_ids (its bookkeeping runs beside this step's rows and the model), ONE cache call."""
        if grad.push_indices is not None:
            raise RuntimeError("ParameterServerCommunicateOp (cache_plan_ahead, asp): gradients with push_indices (laia push "
                               "plans) are not part of the planned push-pull chain; use bsp=0 or cache_plan_ahead=False")
        if not self._planned or not _same_tensor(self._planned[0], grad.indices.reshape(-1)):
            raise RuntimeError("ParameterServerCommunicateOp (cache_plan_ahead, asp): the gradients pushed are not those of the "
                               "batch pulled last")
        if self._bag is not None and not (getattr(grad, "pooled", False) and grad.bag == self._bag):
            raise RuntimeError("ParameterServerCommunicateOp (cache_plan_ahead, asp, bag=%d): the pull buffer holds pooled rows, "
                               "so the gradients must be the pooled slices of EmbeddingLookUpSum_Gradient over bags of %d ids; "
                               "use cache_fuse_bags=False for per-occurrence gradients" % (self._bag, self._bag))
        nxt = self.next_ids()
        if len(self._planned) < 2:                                 # peek_ids had run dry: the step is planned now
            self._plan_chain(nxt)
        elif isinstance(nxt, tuple) or not _same_tensor(self._planned[1], nxt.reshape(-1)):
            raise RuntimeError("ParameterServerCommunicateOp (cache_plan_ahead, asp): the batch to pull is not the one "
                               "peek_ids announced")
        after = self.peek_ids(1)
        if after is not None:
            self._plan_chain(after)
        self._planned.pop(0)
        width = self.parameter.shape[1]
        if self._bag is not None:      # (checked above, before anything was planned: the slices are pooled by this bag size)
            return self.cache.embedding_push_pull_planned_bags(self.sparse_pull_val.reshape(-1, width),
                                                               grad.values.reshape(-1, width).contiguous(), bag=self._bag)
        return self.cache.embedding_push_pull_planned(self.sparse_pull_val.reshape(-1, width),
                                                      grad.values.reshape(-1, width).contiguous())

    def _push_pull_cache(self, grad):
        if self._chain:
            return self._push_pull_planned(grad)
        if self._bag_calls:
            self._pooled_by_bag(grad)
            nxt = self.next_ids()
            width = self.parameter.shape[1]
            return self.cache.embedding_push_pull_bags((nxt[0] if isinstance(nxt, tuple) else nxt).reshape(-1),
                                                       self.sparse_pull_val.reshape(-1, width), grad.indices.reshape(-1),
                                                       grad.values.reshape(-1, width).contiguous(), bag=self._bag)
        nxt = self.next_ids()
        return self.cache.embedding_push_pull((nxt[0] if isinstance(nxt, tuple) else nxt).reshape(-1),
                                              self.sparse_pull_val.reshape(-1, self.parameter.shape[1]),
                                              grad.indices.reshape(-1),
                                              grad.values.reshape(-1, self.parameter.shape[1]))

    # -- plain PS flavour (SparsePush / SparsePull / SSPushPull, :74-111); values are already scaled
    def _push_sparse(self, grad):
        if self._ps_wbags and getattr(grad, "weighted", False):      # (what _per_occurrence left weighted: values is [B, width])
            width, store = self.parameter.shape[1], self.parameter.store
            if grad.bag is not None:
                ids = grad.indices.reshape(-1, int(grad.bag))
                store.push_wbags(ids, grad.values.reshape(-1, width), grad.weights.reshape(ids.shape).contiguous(),
                                 lr=-self.learning_rate)
            else:
                ids = grad.indices.reshape(-1)
                store.push_wbags(ids, grad.values.reshape(-1, width), grad.weights.reshape(-1).contiguous(),
                                 lr=-self.learning_rate, offsets=grad.offsets)
            return None
        if self._ps_bags and getattr(grad, "pooled", False):      # (what _per_occurrence left pooled: values is [B, width])
            width = self.parameter.shape[1]
            if grad.bag is not None:
                self.parameter.store.push_bags(grad.indices.reshape(-1, int(grad.bag)), grad.values.reshape(-1, width))
            else:
                self.parameter.store.push_bags(grad.indices.reshape(-1), grad.values.reshape(-1, width),
                                               offsets=grad.offsets)
            return None
        self.parameter.store.push(grad.indices, grad.values)
        return None

    def _pull_sparse(self, ids):
        if isinstance(ids, tuple):
            ids = ids[0]
        if self._ps_bags:
            if ids.dim() != 2 or ids.shape[1] != self._bag:
                raise ValueError("ParameterServerCommunicateOp(bag=%d): ids must be [B, %d], got %s"
                                 % (self._bag, self._bag, tuple(ids.shape)))
            self.parameter.store.pull_sum(ids, out=self.sparse_pull_val)
            return None
        if self._ps_wbags:
            if ids.dim() != 2 or ids.shape[1] != self._bag:
                raise ValueError("ParameterServerCommunicateOp(bag=%d): ids must be [B, %d], got %s"
                                 % (self._bag, self._bag, tuple(ids.shape)))
            weights, self._first_weights = self._first_weights, None
            if weights is None:
                weights = self.next_weights()      # of the batch the latest next_ids() call returned: these ids
            self.parameter.store.pull_wsum(ids, weights, out=self.sparse_pull_val)
            return None
        self.sparse_pull_val.copy_(self.parameter.store.pull(ids))
        return None

    def _push_pull_sparse(self, grad):
        self._push_sparse(grad)
        return self._pull_sparse(self.next_ids())


class ParameterServerSparsePullOp:
    """Inference-time pull of the next validation batch (:254-306)."""

    def __init__(self, parameter, next_ids):
        self.parameter, self.next_ids = parameter, next_ids

    def forward_hook(self, config):
        self.use_cache_table = config.cstable_policy is not None
        ids = self.next_ids()
        self.sparse_pull_val = torch.empty(tuple(ids.shape) + (self.parameter.shape[1],), dtype=torch.float32,
                                           device=ids.device)
        self.compute()

    def compute(self):
        ids = self.next_ids()
        if self.use_cache_table:
            w = self.parameter.cache.embedding_lookup(ids.reshape(-1),
                                                      self.sparse_pull_val.reshape(-1, self.parameter.shape[1]))
            w.wait()
        else:
            self.sparse_pull_val.copy_(self.parameter.store.pull(ids))
        return self.sparse_pull_val

/*
 * herald_amd.h -- C-ABI of the MI355X-native embedding-access engine.
 *
 * This is the drop-in boundary for Herald/Hetu's embedding hot path.  Two groups
 * of entry points are exported by libherald_amd.so:
 *
 *  (1) Reference-named operator symbols, with the reference's DLArray/DLStream
 *      calling convention, so the ctypes wrappers in python/hetu/gpu_links (ctypes) binds them
 *      unchanged.  Each declaration cites the reference prototype it replaces.
 *
 *  (2) `ha_*` plain-pointer entry points (device pointers, sizes, a hipStream_t
 *      passed as void*) that the reference-named symbols, the hetu_cache /
 *      laia_cache plugin mirrors and the sharded store are built from.
 *
 * Conventions (same as the reference, src/common/c_runtime_api.h + runtime_base.h):
 *   - return 0 on success, -1 on error (ha_last_error() holds the message);
 *   - caller owns every buffer; the callee borrows it for the call;
 *   - GPU work is asynchronous on the given stream; the caller synchronises;
 *   - indices at the operator boundary are float32 (python/hetu/dataloader.py:14),
 *     converted with (size_t)ids[i] semantics (src/dnnl_ops/EmbeddingLookup.cpp:31);
 *   - all embedding values are float32, row-major [rows, width].
 *
 * No torch types appear here; PyTorch is only used by the Python host side to
 * allocate device memory and provide streams.
 */
#ifndef HERALD_AMD_H_
#define HERALD_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- reference ABI structs (src/common/dlarray.h:18-60) ------------------ */
typedef enum { kCPU = 1, kGPU = 2 } DLDeviceType;
typedef struct {
    int device_id;
    DLDeviceType device_type;
} DLContext;
typedef struct {
    void *data;
    DLContext ctx;
    int ndim;
    int64_t *shape;
    int64_t *stride;
} DLArray;
typedef struct {
    int device_id;
    void *handle; /* points at a hipStream_t (reference: cudaStream_t*), may be NULL */
} DLStream;
typedef DLArray *DLArrayHandle;
typedef DLStream *DLStreamHandle;

/* The stream contract of every entry point that takes a stream (ha_stream_t, or a DLStreamHandle that points at one), and of
 * the Python functions built on them (herald_amd/ops.py, herald_amd/hetu_ops.py: `stream=S`, or `stream=None` while S is
 * torch's current stream).  tests/stream_contract.py holds one row per call; tests/test_gpu_stream_contract.py checks it.
 *   1. Everything the call enqueues runs on S.  Its device inputs need only be complete on S.
 *   2. Unless the call returns a count to the host (the n_unique of a plan: IndexPlan.n_unique / export_f32,
 *      IndexedSlices.deduplicate and the fuse_bags=False forms that run it), it never waits on the host for S.  (The first
 *      call of a size on a stream may: the per-stream scratch grows.)
 *   3. Device memory the call allocates for its own use does not become reusable before S has run the launches that use it.
 *      In this library that is the per-stream scratch (one request per call, never from a nested call); in the Python layer,
 *      temporaries allocated while S is torch's current stream.
 *   4. The result is a function of the arguments alone: it does not depend on what ran before on S -- the scratch a call finds
 *      holds whatever the last call on S left there -- nor on which stream S is. */
typedef void *ha_stream_t; /* hipStream_t */

/* ---- library / error handling ------------------------------------------- */
const char *ha_version(void);
const char *ha_last_error(void);
/* Free the internal per-stream scratch used by the one-call reference-named ops. */
int ha_scratch_release(void);
/* Number of visible HIP devices (does not initialise a context beyond hipGetDeviceCount). */
int ha_device_count(void);

/* ========================================================================= *
 * (1) Reference-named operator symbols
 * ========================================================================= */

/* src/common/c_runtime_api.h:308-310, src/ops/EmbeddingLookup.cu:16-52
 * output[..., :] = input[(size_t)ids[...], :]                                */
int DLGpuEmbeddingLookUp(const DLArrayHandle input, const DLArrayHandle ids,
                         DLArrayHandle output, DLStreamHandle stream_handle);

/* src/common/c_runtime_api.h:312-314, src/ops/EmbeddingLookup.cu:75-132
 * input_grad = 0; input_grad[ids[i], :] += output_grad[i, :]  (dense result) */
int DLGpuEmbeddingLookUp_Gradient(const DLArrayHandle output_grad,
                                  const DLArrayHandle ids,
                                  DLArrayHandle input_grad,
                                  DLStreamHandle stream_handle);

/* src/common/c_runtime_api.h:569-571, src/ops/IndexedSlices.cu:17-48
 * output[indices[i], :] += values[i, :]                                      */
int IndexedSlicesOneSideAdd(const DLArrayHandle indices,
                            const DLArrayHandle values, DLArrayHandle output,
                            DLStreamHandle stream_handle);

/* src/common/c_runtime_api.h:700-702, src/ops/OptimizersSparse.cu:282-329
 * compressed[(int)inverse[i], :] += origin[i, :]   (compressed pre-zeroed by caller) */
int DeduplicateIndexedSlices(const DLArrayHandle origin,
                             const DLArrayHandle inverse,
                             DLArrayHandle compressed,
                             DLStreamHandle stream_handle);

/* src/common/c_runtime_api.h:704-706, src/ops/OptimizersSparse.cu:233-280
 * new_values[(int)indices[i], :] = values[i, :]   (new_values pre-zeroed by caller) */
int IndexedSlices2Dense(const DLArrayHandle values, const DLArrayHandle indices,
                        DLArrayHandle new_values, DLStreamHandle stream_handle);

/* src/common/c_runtime_api.h:645-648, src/ops/OptimizersSparse.cu:53-99
 * param[indices[i], :] -= lr * values[i, :]; duplicates applied in occurrence
 * order per row (bit-identical to cpu_SGDOptimizerSparseUpdate,
 * src/dnnl_ops/Optimizers.cpp:51-74).                                         */
int SGDOptimizerSparseUpdate(DLArrayHandle param,
                             const DLArrayHandle grad_indices,
                             const DLArrayHandle grad_values, float lr,
                             DLStreamHandle stream_handle);

/* Sparse optimizers on DEDUPLICATED indices (callers run IndexedSlices.deduplicate first,
 * python/hetu/gpu_links/OptimizerLink.py:60,78,95).  For all of the optimizer symbols below: an index at or
 * beyond the number of rows is skipped, and so is every index that names no row -- negative, NaN, infinite, at or beyond
 * 2^32 -- by the one id rule ("Which ids name a row", below).  Arrays need not be 16-byte aligned.  A call whose arguments are
 * refused (-1) has enqueued nothing and changes nothing.
 * src/common/c_runtime_api.h:661-664 / src/ops/OptimizersSparse.cu:331-389 */
int AdaGradOptimizerSparseUpdate(DLArrayHandle param,
                                 const DLArrayHandle grad_indices,
                                 const DLArrayHandle grad_values,
                                 DLArrayHandle acc, float lr, float eps,
                                 DLStreamHandle stream_handle);
/* src/common/c_runtime_api.h:670-674 / src/ops/OptimizersSparse.cu:391-455 */
int AdamOptimizerSparseUpdate(DLArrayHandle param,
                              const DLArrayHandle grad_indices,
                              const DLArrayHandle grad_values,
                              DLArrayHandle expavg, DLArrayHandle expavgsq,
                              float lr, float beta1, float beta2, float beta1t,
                              float beta2t, float eps,
                              DLStreamHandle stream_handle);
/* src/common/c_runtime_api.h:681-686 / src/ops/OptimizersSparse.cu:457-522 */
int AdamWOptimizerSparseUpdate(DLArrayHandle param,
                               const DLArrayHandle grad_indices,
                               const DLArrayHandle grad_values,
                               DLArrayHandle expavg, DLArrayHandle expavgsq,
                               float lr, float beta1, float beta2,
                               float beta1t, float beta2t, float eps,
                               float weight_decay,
                               DLStreamHandle stream_handle);
/* src/common/c_runtime_api.h:639-643 / src/ops/OptimizersSparse.cu:3-51:
 * grad_values[i,:] += l2reg * param[grad_indices[i],:]  (deduplicated slices, OptimizerLink.py:15-20) */
int AddL2RegularizationSparse(const DLArrayHandle param,
                              const DLArrayHandle grad_indices,
                              DLArrayHandle grad_values, float l2reg,
                              DLStreamHandle stream_handle);
/* src/common/c_runtime_api.h:653-656 / src/ops/OptimizersSparse.cu:101-231: indices may repeat
 * (OptimizerLink.py:37-49 does not deduplicate).  velocity[id,:] += -lr*g per occurrence (Nesterov: the
 * parameter row too), in occurrence order instead of the reference's atomics; then the reference's DENSE
 * second phase over the whole array: param += velocity, velocity *= momentum (Nesterov: velocity *=
 * momentum first, then param += velocity).  With no indices (n = 0) the dense phase still runs. */
int MomentumOptimizerSparseUpdate(DLArrayHandle param,
                                  const DLArrayHandle grad_indices,
                                  const DLArrayHandle grad_values,
                                  DLArrayHandle velocity, float lr,
                                  float momentum, bool nesterov,
                                  DLStreamHandle stream_handle);
/* src/common/c_runtime_api.h:693-699 / src/ops/OptimizersSparse.cu:524-722 (deduplicated slices) */
int LambOptimizerSparseUpdate(DLArrayHandle param,
                              const DLArrayHandle grad_indices,
                              const DLArrayHandle grad_values,
                              DLArrayHandle expavg, DLArrayHandle expavgsq,
                              float lr, float beta1, float beta2, float beta1t,
                              float beta2t, float eps, float weight_decay,
                              DLStreamHandle stream_handle);
/* src/common/c_runtime_api.h:811-818, the reference's CPU operator names that python/hetu/_base.py:8-11,72
 * feature-probes.  Served by the HIP kernels (null stream, complete on return); there is no CPU arithmetic
 * behind them.  Arrays whose DLContext is the GPU are used where they lie.  HOST arrays (what the reference's
 * callers pass: EmbeddingLookUp.py:16-17, optimizer.py:203-207) are made visible to the device for the call:
 * below 64 MiB copied (H2D, kernel, D2H for the written one), from 64 MiB page-locked and mapped with
 * hipHostRegister -- the kernels then move only the rows the ids name across PCIe; the registration is kept
 * until ha_host_unmap(array) / ha_scratch_release() (callers pass the same parameter array every step).  An array
 * of that size must be unmapped BEFORE it is freed: an allocation that lands on the same address later would be
 * seen through the old mapping. */
int ha_host_unmap(void *host_array);
int cpu_EmbeddingLookup(const DLArrayHandle in_mat, const DLArrayHandle ids,
                        DLArrayHandle out_mat);
int cpu_SGDOptimizerSparseUpdate(DLArrayHandle param,
                                 const DLArrayHandle grad_indices,
                                 const DLArrayHandle grad_values, float lr);

/* ========================================================================= *
 * (2) Plain-pointer engine entry points.  All pointers are DEVICE pointers
 *     unless a parameter name ends in _host.
 * ========================================================================= */

/* Tolerance mode (process-wide, default off).  Off: every sparse update is the reference's serial chain, occurrence by
 * occurrence (cpu_SGDOptimizerSparseUpdate, src/dnnl_ops/Optimizers.cpp:65-72), bit for bit.  On: runs of 64 or more
 * occurrences of one key in a batch are applied as `row - tree_sum(lr * g)` in a fixed, deterministic order -- within
 * the 1e-5 relative BASELINE.json's north star allows for accumulated fp32 gradients; shorter runs stay bit-exact.
 * on = 1: one sixteen-wave tree over the whole run (oracle/qstep_model.py tree_coop).  on = 2: as 1, and the applies of a
 * FINISHED plan of 36,865 .. 2^20 ids on rows of up to 256 floats cut a run beyond 256 occurrences into chunks of 256 that
 * workgroups of their own sum, the chunk sums added in chunk order (tree_coop_chunked; the rule: listed_chunking) -- for
 * batches in which one key's run is the launch's critical path; at BASELINE configs[2]'s shape it is not (34.5 us without,
 * 35.8 with), so 1 is what bench.py's N>1 leg uses.  ha_get_tolerance_mode returns 0 / 1 / 2.
 * The trees read and write 16 bytes at a time: they serve rows of a multiple of 4 floats whose table and gradient pointers are
 * 16-byte aligned.  Any other call (width % 4 != 0, a misaligned view) is the serial chain in every mode, bit for bit
 * (oracle/qstep_model.py tolerance_has_tree).
 * Values: a tree slot beyond the run's end holds +0 whatever lies there in memory (a select, never value * 0), and every
 * partial sum starts from +0, so 0 + (-0) = +0 as in the reduce of ha_dedup_reduce; a NaN or an infinity stays in the key and
 * column it sits in.  `row - tree_sum` and the chain may differ in the SIGN OF A ZERO: g and -g over a -0 row end in +0 along
 * the chain and in -0 - (+0) = -0 through a tree (oracle/qstep_model.py states both).
 * Read at launch time by ha_sgd_apply*, ha_push_apply*, ha_dedup_reduce*, ha_apply_mapped, ha_shard_serve_push and the
 * entry points built on them (not by ha_sgd_push_pull_* / ha_step_*, which are bit-exact throughout, nor by
 * ha_qstep_* / ha_qapply, which have their own documented tolerance classes). */
int ha_set_tolerance_mode(int on);
int ha_get_tolerance_mode(void);

/* Which ids name a row.  Every entry point turns an id into a 32-bit KEY by one rule, and "an id >= rows" below (a zero row
 * on lookup, skipped by every update) means "an id whose key is >= rows":
 *   float32 id f     key = trunc(f) for -1 < f < 4294967295 -- so -0.0 and -0.99 are key 0, as the reference's (size_t)f --, and
 *                    0xFFFFFFFE for every other f: NaN of either sign and any payload, f <= -1, f >= 4294967295, both
 *                    infinities.  (The largest float32 below 2^32 is 4294967040 = key 0xFFFFFF00: dead by size, like rows.)
 *   int64 / uint64   the value read as uint64; anything above 0xFFFFFFFE becomes 0xFFFFFFFE.  So -1, INT64_MIN and 2^32 + 5
 *                    name no row, and 2^32 + 5 never aliases row 5.
 * Key 0xFFFFFFFE is >= rows for every table the library accepts, and nothing else about it is special: -1.0 and -1 are the
 * same id, all such occurrences of a batch are ONE run of one key in its plan (counted in n_unique, reduced by
 * ha_dedup_reduce like any key), and ha_plan_export_f32 exports it as 4294967296.0.  The conversion never evaluates a
 * float -> integer cast outside the cast's range (csrc/common.h f32_to_key; oracle/oracle.c and tests/special_ids.py
 * state the same rule for the checkers).
 * The tiers that index per-row arrays by key REQUIRE ids below rows (`length`) and do not check it on the device: the HET
 * cache, call by call and planned (ha_cache_*: slot_of[length]), the sharded store and its framed steps (ha_shard_*:
 * owners are found by key range) and laia (ha_laia_*).  An id that names no row is undefined behaviour there; callers
 * replace padding ids before they hand a batch to such a tier. */

/* ---- forward gather (replaces cpu_EmbeddingLookup / embedding_lookup_kernel) */
/* out[i,:] = table[(size_t)ids[i],:], ids float32.  width % 4 == 0 takes the
 * 16-byte vector path; any width >= 1 is supported.                          */
int ha_gather_f32ids(const float *table, int64_t rows, int64_t width,
                     const float *ids, int64_t n, float *out,
                     ha_stream_t stream);
/* Same with 64-bit keys (hetu_cache numpy-uint64 entry points, cache.cc:37-47). */
int ha_gather_u64ids(const float *table, int64_t rows, int64_t width,
                     const uint64_t *ids, int64_t n, float *out,
                     ha_stream_t stream);
int ha_gather_u32keys(const float *table, int64_t rows, int64_t width,
                      const uint32_t *keys, int64_t n, float *out,
                      ha_stream_t stream);

/* dst[(size_t)ids[i],:] = values[i,:] (ids deduplicated by the caller; the body of
 * IndexedSlices2Dense, src/ops/OptimizersSparse.cu:233-280). */
int ha_scatter_rows_f32ids(const float *values, const float *ids, int64_t n,
                           int64_t width, float *dst, int64_t rows,
                           ha_stream_t stream);

/* values[i] *= scale (one float32 rounding): the `values *= -lr` step of
 * ParameterServerCommunicateOp (python/hetu/gpu_ops/ParameterServerCommunicate.py:24,58-59). */
int ha_scale_f32(float *values, int64_t n, float scale, ha_stream_t stream);

/* ---- index plan: sorted-unique + inverse + counts + occurrence lists ------
 * Semantics of np.unique(ids, return_inverse=True, return_counts=True)
 * (python/hetu/ndarray.py:534,559) == hetu::Unique<T> (unqiue_tools.h:27-48)
 * == the std::map dedup of PSAgent::vecPushSparse (PSAgent.h:124-183):
 *   uniq   : ascending distinct keys
 *   inverse: inverse[i] = position of ids[i] in uniq
 *   counts : occurrences of each unique key
 *   perm   : stable argsort of ids (occurrence order inside a run of equal keys)
 *   seg    : seg[u] = first sorted position of unique key u; seg[U] = n
 * Keys are held as uint32 (tables up to 2^32-2 rows).
 *
 * A plan lives in a caller-provided device workspace of ha_plan_bytes(n) bytes
 * laid out as struct ha_plan_view describes; it is valid until the workspace is
 * reused.  n_unique is produced on the device (plan header) so that no host
 * sync is needed between plan and the kernels that consume it.
 * The first 256 bytes of a workspace (the header: n_unique and sticky flag
 * words) must be ZERO before its first use, and the zero fill must have
 * COMPLETED before the first call that names the workspace on another stream:
 * hipMemset / hipMemsetAsync on the null stream is not waited for by the host
 * and is not ordered with non-blocking streams -- synchronise the null stream
 * (or zero on the stream of the first call).  A late fill wipes n_unique.    */
typedef struct {
    int64_t n;           /* number of ids */
    int64_t *n_unique;   /* device scalar (first word of the workspace) */
    uint32_t *keys;      /* [n] ids converted to integer keys, original order */
    uint32_t *sorted;    /* [n] keys ascending */
    int32_t *perm;       /* [n] stable argsort: sorted[p] == keys[perm[p]] */
    int32_t *inverse;    /* [n] */
    uint32_t *uniq;      /* [n] first *n_unique valid */
    int32_t *counts;     /* [n] first *n_unique valid */
    int32_t *seg;        /* [n+1] first *n_unique+1 valid */
    int32_t *upos;       /* [n] upos[p] = unique index of sorted position p */
} ha_plan_view;

size_t ha_plan_bytes(int64_t n);
/* Fill `view` with the addresses of the sub-arrays of workspace `ws` (host-side
 * pointer arithmetic only; no device access). */
int ha_plan_view_of(void *ws, int64_t n, ha_plan_view *view);
/* Diagnostics: with HA_RADIX_STAMPS=1 in the environment the scatter launches of the radix sort (n > 36,864) stamp the GPU's
 * 100 MHz clock at their phase boundaries; out_host[24], eight slots per pass (tools/radix_phases.py). */
int ha_plan_radix_stamps(void *ws, int64_t n, uint64_t *out_host, ha_stream_t stream);
/* Build the plan from float32 ids / uint64 keys. */
int ha_plan_build_f32ids(const float *ids, int64_t n, void *ws,
                         ha_stream_t stream);
int ha_plan_build_u64ids(const uint64_t *ids, int64_t n, void *ws,
                         ha_stream_t stream);
/* Two-phase form.  ha_plan_sort_* produces only `keys`, `sorted` and `perm` -- all that
 * ha_sgd_apply / ha_push_apply need; ha_plan_finish adds n_unique, uniq, counts, seg, inverse and
 * upos (needed by ha_dedup_reduce, ha_plan_export_f32 and the cache).  build == sort + finish. */
int ha_plan_sort_u32keys(const uint32_t *keys, int64_t n, void *plan_ws, int key_bits, ha_stream_t stream);
int ha_plan_sort_f32ids(const float *ids, int64_t n, void *ws,
                        ha_stream_t stream);
int ha_plan_sort_u64ids(const uint64_t *ids, int64_t n, void *ws,
                        ha_stream_t stream);
/* The same with a known key range (key_limit = number of table rows, or any bound on the valid keys):
 * batches of 18,433 .. 36,864 ids then take the bucket sort -- one most-significant-digit scatter into
 * 2,048 ordered key ranges + stable rank-by-counting inside the ranges, three launches -- instead of the
 * O(n^2) single-launch sort or the three-pass LSD radix sort.  Keys at or above the limit are still sorted
 * correctly (they share the last range).  Identical results. */
/* The plans of `count` batches (ids[i], n[i] -> ws[i]; host arrays of device pointers): two launches for all of them
 * when every batch takes the rank-by-counting path (n <= 36,864 and no bucket sort), else one build per batch. */
int ha_plan_build_batch_f32ids_lim(const float *const *ids, const int64_t *n, void *const *ws, int count,
                                   uint64_t key_limit, ha_stream_t stream);
int ha_plan_build_batch_u64ids_lim(const uint64_t *const *ids, const int64_t *n, void *const *ws, int count,
                                   uint64_t key_limit, ha_stream_t stream);
/* the stable sorts alone of up to 16 small batches per launch (what ha_plan_sort_*_lim leaves in each workspace) */
int ha_plan_sort_batch_f32ids_lim(const float *const *ids, const int64_t *n, void *const *ws, int count,
                                  uint64_t key_limit, ha_stream_t stream);
int ha_plan_sort_batch_u64ids_lim(const uint64_t *const *ids, const int64_t *n, void *const *ws, int count,
                                  uint64_t key_limit, ha_stream_t stream);
int ha_plan_build_f32ids_lim(const float *ids, int64_t n, void *ws, uint64_t key_limit, ha_stream_t stream);
int ha_plan_sort_f32ids_lim(const float *ids, int64_t n, void *ws, uint64_t key_limit, ha_stream_t stream);
int ha_plan_build_u64ids_lim(const uint64_t *ids, int64_t n, void *ws, uint64_t key_limit, ha_stream_t stream);
int ha_plan_sort_u64ids_lim(const uint64_t *ids, int64_t n, void *ws, uint64_t key_limit, ha_stream_t stream);
int ha_plan_finish(void *ws, int64_t n, ha_stream_t stream);
/* keys already integer; key_bits = number of significant key bits (radix passes). */
int ha_plan_build_u32keys(const uint32_t *keys, int64_t n, void *ws,
                          int key_bits, ha_stream_t stream);
/* Export np.unique-style float32 results (what IndexedSlices.deduplicate hands to
 * DeduplicateIndexedSlices): uniq_f32[U], inverse_f32[n].  Either may be NULL. */
int ha_plan_export_f32(const void *ws, int64_t n, float *uniq_f32,
                       float *inverse_f32, ha_stream_t stream);

/* ---- backward: dedup-reduce and fused apply -------------------------------*/
/* reduced[u,:] = sum over occurrences i of key u, in occurrence order, starting
 * from 0.0f (IndexedSlices.cpu_deduplicate, python/hetu/ndarray.py:556-576;
 * PSAgent::vecPushSparse; Line::accumulate).  reduced must hold n rows; the
 * first *n_unique are written.  Deterministic, no atomics.                    */
int ha_dedup_reduce(const void *plan_ws, int64_t n, const float *grads,
                    int64_t width, float *reduced, ha_stream_t stream);

/* Same with every value multiplied by `scale` before it is summed: reduced[u,:] = sum(scale*g_i).
 * This is the worker side of a PS sparse push: `values *= -lr` (python/hetu/gpu_ops/
 * ParameterServerCommunicate.py:58-59) followed by the occurrence-order reduce of
 * PSAgent::vecPushSparse (PSAgent.h:146-160). */
int ha_dedup_reduce_scaled(const void *plan_ws, int64_t n, const float *grads,
                           int64_t width, float scale, float *reduced,
                           ha_stream_t stream);

/* table[key,:] -= lr * grads[i,:] for every occurrence i, applied per row in
 * occurrence order with separate multiply and subtract roundings: the result is
 * bit-identical to the serial loop of cpu_SGDOptimizerSparseUpdate
 * (src/dnnl_ops/Optimizers.cpp:65-72).  Each unique row is read and written once.
 * With lr = -1 this is the server side of sparse pushes applied one after the other in
 * occurrence order: table[key,:] = (table[key,:] + v_i0) + v_i1 ...  (PSFHandle.h:130-164). */
int ha_sgd_apply(float *table, int64_t rows, int64_t width,
                 const void *plan_ws, int64_t n, const float *grads, float lr,
                 ha_stream_t stream);
/* The same for a plan that is already FINISHED (ha_plan_build_*, or ha_plan_sort_* followed by ha_plan_finish): batches of
 * more than 36,864 ids map their waves to the unique keys the finish listed instead of to sorted positions (about a third
 * less time for 106,496 ids of 128-wide rows); smaller batches run as ha_sgd_apply.  Bit-identical results. */
int ha_sgd_apply_finished(float *table, int64_t rows, int64_t width, void *plan_ws, int64_t n, const float *grads,
                          float lr, ha_stream_t stream);

/* table[key,:] += scale * reduced_in_occurrence_order (PS push semantics:
 * worker pre-multiplies by -lr, server does +=;
 * ParameterServerCommunicate.py:58-59, PSFHandle.h:130-164).                  */
int ha_push_apply(float *table, int64_t rows, int64_t width,
                  const void *plan_ws, int64_t n, const float *grads,
                  ha_stream_t stream);

/* Mapped flavour used by the embedding cache: for every unique key u of a FINISHED plan
 *   dst[rowmap[u],:] = (dst_init[rowmap[u]] ? dst[rowmap[u],:] : 0) - lr*src[valmap[i0],:] - lr*src[valmap[i1],:] ...
 * over its occurrences i0 < i1 < ... (rowmap[u] < 0 skips u; NULL maps are identities).  With
 * lr = -1 this is Line::accumulate (src/hetu_cache/include/embedding.h:78-91) for a whole batch. */
int ha_apply_mapped(float *dst, int64_t dst_rows, int64_t width,
                    const void *plan_ws, int64_t n, const float *src, float lr,
                    const int32_t *rowmap, const int32_t *valmap,
                    const uint8_t *dst_init, ha_stream_t stream);
/* ha_apply_mapped into two destinations with one pass over src (the cache's Line::accumulate writes the
 * same ordered sum into a line's gradient buffer and into its data row, embedding.h:78-91):
 * dst as ha_apply_mapped with (rowmap, dst_init); dst2[rowmap2[u],:] always starts from its stored
 * value; rowmap2[u] < 0 = no second row.  Each result equals its own ha_apply_mapped call bit for bit. */
int ha_apply_mapped2(float *dst, int64_t dst_rows, float *dst2, int64_t width,
                     const void *plan_ws, int64_t n, const float *src, float lr,
                     const int32_t *rowmap, const int32_t *rowmap2,
                     const uint8_t *dst_init, ha_stream_t stream);
/* ha_apply_mapped2 with src = bag_grads[nbags, width] expanded to [n, width], without the expanded tensor: occurrence i reads
 * row i / bag (fixed bags: bag >= 1, bag_of NULL, n % bag == 0) or row bag_of[i] (ragged: bag == 0, device int32 bag_of[n]).
 * Both destinations equal the unpooled call's bit for bit. */
int ha_apply_mapped2_bags(float *dst, int64_t dst_rows, float *dst2, int64_t width, const void *plan_ws, int64_t n,
                          const float *bag_grads, float lr, const int32_t *rowmap, const int32_t *rowmap2, int64_t bag,
                          const int32_t *bag_of, const uint8_t *dst_init, ha_stream_t stream);

/* ---- fused deduplicate + optimizer step -----------------------------------------------------------
 * One call for what the reference does in two (python/hetu/gpu_links/OptimizerLink.py:52-100:
 * grad.deduplicate(stream), then {AdaGrad,Adam,AdamW}OptimizerSparseUpdate on the reduced slices): index plan
 * of the raw ids, then ONE launch in which every key's gradient rows are summed in occurrence order in
 * registers and consumed by that row's optimizer step -- the reduced slices never travel through HBM.
 * Bit-identical to ha_dedup_reduce + the optimizer symbol.  kind: 0 AdaGrad (state1 = accumulator, state2
 * unused), 1 Adam, 2 AdamW (state1 = exp_avg, state2 = exp_avg_sq).  hyper_host: 7 host floats
 * {lr, eps, beta1, beta2, beta1t, beta2t, weight_decay}.  plan_ws: ha_plan_bytes(n) of device scratch. */
int ha_sparse_opt_fused_f32ids(int kind, float *param, int64_t rows, int64_t width, const float *ids,
                               int64_t n, const float *grads, float *state1, float *state2,
                               const float *hyper_host, void *plan_ws, ha_stream_t stream);
/* The same for uint64 keys (the plan is ha_plan_sort_u64ids_lim's): equal ids give equal bits. */
int ha_sparse_opt_fused_u64ids(int kind, float *param, int64_t rows, int64_t width, const uint64_t *ids,
                               int64_t n, const float *grads, float *state1, float *state2,
                               const float *hyper_host, void *plan_ws, ha_stream_t stream);
/* The same on the POOLED gradient of a sum-pooled lookup (ha_gather_sum_*, below): bag_grads is [nbags, width] and
 * occurrence i takes the row of its bag -- i / bag for fixed bags (bag >= 1, offsets NULL, n == nbags * bag; computed in
 * registers, no map is read), the bag that offsets places it in for ragged ones (bag == 0, device offsets[nbags + 1];
 * ha_bag_of builds the map in the per-stream scratch).  No [n, width] gradient exists anywhere: the launch reads
 * nbags * width * 4 distinct gradient bytes.  kind, state1 / state2, hyper_host and plan_ws are ha_sparse_opt_fused_f32ids'.
 * Bit for bit, in param, state1 and state2, what ha_sparse_opt_fused_f32ids gives on bag_grads expanded to [n, width],
 * for every n (one wave per sorted position up to 36,864 ids, waves mapped to unique keys beyond) and in every tolerance
 * mode (the optimizer step is exact in all of them).  Rows no in-range id names are untouched, an id >= rows is skipped,
 * n == 0 returns 0 and touches nothing.  width % 4 == 0 with 16-byte aligned param, bag_grads and states takes the
 * 16-byte path, anything else the scalar one.  Returns -1 before any device access for a kind outside 0..2, a null
 * pointer, width < 1, a negative size, n >= 2^31, both or neither of bag / offsets, n != nbags * bag, or a missing
 * state2 for Adam / AdamW. */
int ha_sparse_opt_fused_bags_f32ids(int kind, float *param, int64_t rows, int64_t width, const float *ids,
                                    int64_t n, const float *bag_grads, int64_t bag, const int64_t *offsets,
                                    int64_t nbags, float *state1, float *state2, const float *hyper_host,
                                    void *plan_ws, ha_stream_t stream);
int ha_sparse_opt_fused_bags_u64ids(int kind, float *param, int64_t rows, int64_t width, const uint64_t *ids,
                                    int64_t n, const float *bag_grads, int64_t bag, const int64_t *offsets,
                                    int64_t nbags, float *state1, float *state2, const float *hyper_host,
                                    void *plan_ws, ha_stream_t stream);

/* ---- fused launches (two per training step) --------------------------------
 * ha_lookup_sort_*    == ha_gather_* + ha_plan_sort_*   in ONE launch (forward: the lookup of a
 *                        batch and the index plan its backward will need);
 * ha_sgd_apply_finish == ha_sgd_apply + ha_plan_finish  in ONE launch (backward);
 * ha_push_apply_finish likewise for the PS push semantics.  Bit-identical to the unfused calls;
 * batches larger than the single-launch sort limit fall back to the unfused sequence. */
int ha_lookup_sort_f32ids(const float *table, int64_t rows, int64_t width,
                          const float *ids, int64_t n, float *out,
                          void *plan_ws, ha_stream_t stream);
int ha_lookup_sort_u64ids(const float *table, int64_t rows, int64_t width,
                          const uint64_t *ids, int64_t n, float *out,
                          void *plan_ws, ha_stream_t stream);
int ha_sgd_apply_finish(float *table, int64_t rows, int64_t width,
                        void *plan_ws, int64_t n, const float *grads, float lr,
                        ha_stream_t stream);
int ha_push_apply_finish(float *table, int64_t rows, int64_t width,
                         void *plan_ws, int64_t n, const float *grads,
                         ha_stream_t stream);

/* ---- ONE launch per training step: backward of batch k beside the forward of batch k+1 -------------
 * ha_sgd_push_pull_* == ha_sgd_apply_finish(plan_cur, grads) followed by ha_lookup_sort_*(next_ids ->
 * next_out, plan_next), as ONE launch.  This is the reference's embedding_push_pull
 * (src/hetu_cache/src/cache.cc:356-422, python/hetu/cstable.py: push the gradients of one batch and
 * pull the rows of the next in one request) on the HBM-resident table; the rows returned for batch k+1
 * are the rows AFTER batch k's update, and every result is bit-identical to the two separate launches
 * (cpu_SGDOptimizerSparseUpdate, src/dnnl_ops/Optimizers.cpp:51-74, then cpu_EmbeddingLookup,
 * src/dnnl_ops/EmbeddingLookup.cpp:16-35).  The ids of the next batch are known one step ahead (the
 * reference prefetches too: ParameterServerCommunicate.py:96-139, dataloader.py:63-98).
 *
 * Rows that both batches touch are handed from the applying wave to the gathering wave inside the
 * launch through a per-batch PENDING TABLE (ha_pend_bytes() bytes of device memory, all-zero when
 * idle: ha_pend_reset).  The launch that SORTS a batch registers its keys in that batch's table
 * (ha_lookup_sort_pend_* for the first batch, ha_sgd_push_pull_* for every later one: pend_next); the
 * launch that APPLIES the batch drains it (pend_cur) and leaves it all-zero again.  So a plan sorted
 * with pending table P must be applied by ha_sgd_push_pull_* with pend_cur = P (n_next = 0 for the
 * last batch), and two tables alternate between consecutive batches.
 *   n_cur == 0: only the lookup + sort of the next batch (== ha_lookup_sort_pend_*);
 *   n_next == 0: only the apply + finish of the current batch.
 * grads / next_out must be 16-byte aligned.  The single launch needs rows that own their 128-byte lines
 * (width % 32 == 0, table 128-byte aligned) and batches of at most 18,432 ids (above that the bucket sort of the separate launches wins);
 * anything else runs as the separate launches with the same results (nothing is registered then).
 * Should a hand-off wait ever exceed its bound (~0.1 s; never observed), word 9 (int64) of
 * plan_next's 256-byte header is set to 1 (ha_plan_handoff_timeout) instead of hanging the device: the rows of
 * that lookup may then be stale, and the flag stays set.  The library never reads it back (that would put a
 * host synchronisation into every step); a caller that trains on the rows MUST poll it at a point where it
 * synchronises anyway (herald_amd.ops: IndexPlan.n_unique() raises, ops.check_handoff(plans) after a
 * synchronisation; examples/ctr/run_wdl.py checks it at every logging interval). */
size_t ha_pend_bytes(void);
int ha_pend_reset(void *pend, ha_stream_t stream);
int ha_lookup_sort_pend_f32ids(const float *table, int64_t rows, int64_t width,
                               const float *ids, int64_t n, float *out,
                               void *plan_ws, void *pend, ha_stream_t stream);
int ha_lookup_sort_pend_u64ids(const float *table, int64_t rows, int64_t width,
                               const uint64_t *ids, int64_t n, float *out,
                               void *plan_ws, void *pend, ha_stream_t stream);
int ha_sgd_push_pull_f32ids(float *table, int64_t rows, int64_t width,
                            void *plan_cur, int64_t n_cur, const float *grads, float lr,
                            void *pend_cur, const float *next_ids, int64_t n_next,
                            float *next_out, void *plan_next, void *pend_next,
                            ha_stream_t stream);
int ha_sgd_push_pull_u64ids(float *table, int64_t rows, int64_t width,
                            void *plan_cur, int64_t n_cur, const float *grads, float lr,
                            void *pend_cur, const uint64_t *next_ids, int64_t n_next,
                            float *next_out, void *plan_next, void *pend_next,
                            ha_stream_t stream);
/* development aid (tools/step_timeline.py): ha_sgd_push_pull_f32ids with per-wave time stamps,
 * dbg = device uint64[(number of workgroups) * 16 * 4] */
int ha_debug_step_timeline(float *table, int64_t rows, int64_t width,
                           void *plan_cur, int64_t n_cur, const float *grads, float lr,
                           void *pend_cur, const float *next_ids, int64_t n_next,
                           float *next_out, void *plan_next, void *pend_next,
                           unsigned long long *dbg, ha_stream_t stream);
/* device address of the sticky time-out flag (int64, 0 = fine) of a plan workspace: set by a launch whose wait for other
 * workgroups of the same launch exceeded its bound -- the hand-off above, or the histogram exchange of the one-launch radix
 * passes that sort more than 36,864 ids (all tiles of a pass are resident at once, so the wait is microseconds; the bound
 * keeps a scheduling surprise from hanging the device) */
int64_t *ha_plan_handoff_timeout(void *plan_ws);

/* The step with THREE batches of lookahead: ONE launch that
 *   - applies the gradients of batch k (plan_cur)
 *     == ha_sgd_apply(table, plan_cur, grads, lr)             [cpu_SGDOptimizerSparseUpdate, Optimizers.cpp:51-74]
 *   - writes the rows of batch k+1 AFTER that update to next_out (plan_next)
 *     == ha_gather_*(table, ids of batch k+1)                 [cpu_EmbeddingLookup, EmbeddingLookup.cpp:16-35]
 *   - finishes the plan of batch k+2 (plan_fin: unique keys, inverse, counts)   == ha_plan_finish
 *   - sorts batch k+3 (ahead_ids -> plan_ahead)               == ha_plan_sort_*(ahead_ids)
 * with results bit-identical to those calls.  Nothing waits inside the launch: batch k+1 was sorted and
 * finished by earlier calls, so the wave that holds the final values of a row of batch k writes them
 * straight to every output row of batch k+1 that names the key, and only the rows batch k does not touch
 * are copied from the table -- the rows both batches share (two thirds of the positions of consecutive
 * Criteo batches) are not read back from HBM.  The ids are known three batches ahead (the reference's
 * dataloader and laia scheduler run further ahead than that: dataloader.py:63-98, laia_scheduler.cc).
 *
 * Every batch owns a KEY TABLE (ha_step_tab_bytes() bytes of device memory, ha_step_tab_reset before first
 * use): filled by the call that finishes the batch's plan (tab_fin), read by the two calls after it
 * (tab_next, then tab_cur), and cleared by the call after those (tab_clear) -- four tables and four plans
 * rotate.  A stream of batches 0..B-1 is driven as calls c = -3 .. B-1 with cur = c, next = c+1, fin = c+2,
 * ahead = c+3 and n = 0 / null pointers for batches outside [0, B); call c uses tables T[c%4] (cur),
 * T[(c+1)%4] (next), T[(c+2)%4] (fin) and clears T[(c+3)%4].  Limits: at most ha_step_max_ids() ids per
 * batch, width % 4 == 0, table / grads / next_out 16-byte aligned; anything else is refused (-1): use
 * ha_sgd_push_pull_* or the separate calls. */
size_t ha_step_tab_bytes(void);
int64_t ha_step_max_ids(void);
int ha_step_tab_reset(void *tab, ha_stream_t stream);
int ha_step_f32ids(float *table, int64_t rows, int64_t width,
                   void *plan_cur, int64_t n_cur, const float *grads, float lr, const void *tab_cur,
                   void *plan_next, int64_t n_next, float *next_out, const void *tab_next,
                   void *plan_fin, int64_t n_fin, void *tab_fin,
                   const float *ahead_ids, int64_t n_ahead, void *plan_ahead,
                   void *tab_clear, ha_stream_t stream);
int ha_step_u64ids(float *table, int64_t rows, int64_t width,
                   void *plan_cur, int64_t n_cur, const float *grads, float lr, const void *tab_cur,
                   void *plan_next, int64_t n_next, float *next_out, const void *tab_next,
                   void *plan_fin, int64_t n_fin, void *tab_fin,
                   const uint64_t *ahead_ids, int64_t n_ahead, void *plan_ahead,
                   void *tab_clear, ha_stream_t stream);
/* development aid (tools/step_fwd_timeline.py): ha_step_f32ids with per-wave time stamps */
int ha_debug_step_fwd_timeline(float *table, int64_t rows, int64_t width,
                               void *plan_cur, int64_t n_cur, const float *grads, float lr, const void *tab_cur,
                               void *plan_next, int64_t n_next, float *next_out, const void *tab_next,
                               void *plan_fin, int64_t n_fin, void *tab_fin,
                               const float *ahead_ids, int64_t n_ahead, void *plan_ahead,
                               void *tab_clear, unsigned long long *dbg, ha_stream_t stream);

/* The same step driven by a WORK QUEUE that preparation launches have built (csrc/qstep.hip).
 *   ha_qapply        step c, ONE launch: applies the gradients of batch c and writes the rows of batch c+1 after that
 *                    update, item by item from QUEUE c: one wave per (unique key, column slice) applies the key's
 *                    occurrences to the row it holds in registers, writes the row back and writes it to every output
 *                    row of batch c+1 naming the key; keys only batch c+1 names are copies.  No probing, no waiting.
 *   ha_qplan_batch_* the plans of `count` batches, one workgroup each in one launch: unique keys, counts, segment
 *                    starts, inverse and occurrence lists (ascending inside every segment) of an index plan -- with
 *                    the unique keys in the order of a hash table's slots, NOT in key order (ha_plan_build_* gives
 *                    np.unique's order).
 *   ha_qqueue_batch  the queues of `count` steps, two workgroups each in one launch: queue k from the finished plans
 *                    of the batch step k applies (plans_a[k], n_a[k] ids; 0 = none) and of the batch it looks up
 *                    (plans_g[k]).
 * A plan takes one workgroup ~15 us and a queue ~13-20 us, longer than the items of a step (~11 us): callers prepare a
 * BLOCK of steps at a time on a stream of their own, beside the steps of the block before
 * (herald_amd.ops.QueueStepPipeline); ha_qprep_* (one plan and / or one queue) and ha_qstep_* (that, then the step: three
 * launches on one stream) are the serial forms.
 * Semantics and references as ha_step_* above (cpu_SGDOptimizerSparseUpdate, Optimizers.cpp:51-74;
 * cpu_EmbeddingLookup, EmbeddingLookup.cpp:16-35), with ONE difference: keys with fewer than 16 occurrences in a batch
 * take the reference's serial chain row = (row - lr*g0) - lr*g1 ... bit for bit; a key with 16 or more occurrences takes
 * row - T, T = a fixed (deterministic) tree sum of the lr*g_i -- within the 1e-5 relative that BASELINE.json's north star
 * allows for accumulated gradients, not bit-identical to the serial chain.  Integer results are exact.  Callers that need
 * the serial chain for every run length use ha_step_*.
 * A queue is ha_qstep_queue_bytes(n_cap, width) bytes (no initialisation); queue_n_cap = the n_cap it was sized with.
 * Limits: at most ha_qstep_max_ids() ids per batch, width % 4 == 0, table / grads / next_out 16-byte aligned.  ids / n /
 * plans / queues arguments of the batch calls are HOST arrays of `count` entries (device pointers inside).
 * CALLER REQUIREMENT (lookahead): step c reads queue c, which is built from the plans of batches c and c+1 -- the ids of
 * batch c+1 must be on the device before queue c is built, and the queue must be complete before ha_qapply(c) starts.
 * The serial forms need the ids 3 batches ahead; the block-pipelined schedule of ops.QueueStepPipeline (plans of block
 * b+2 and queues of block b+1 beside the steps of block b) needs them 3 * block batches ahead (48 at bench.py's block of
 * 16).  The reference's dataloader contract is one batch ahead in a 3-deep ring (python/hetu/dataloader.py:63-98) and
 * laia's queue is 5 deep: a caller that cannot name its ids that far ahead uses ha_step_* (3 batches) or
 * ha_sgd_push_pull_* (1 batch).
 * ha_qstep_init: per-device set-up (LDS attributes of the plan / queue kernels, the lane-order probe of the LDS atomics:
 * one small synchronous launch on the null stream), to be called once per device OUTSIDE any stream capture; the entry
 * points do the same lazily on their first call.  Returns 1 (atomic ranking), 0 (ballot ranking; HA_QSTEP_BALLOT=1) or -1. */
int ha_qstep_init(void);
int64_t ha_qstep_max_ids(void);
size_t ha_qstep_queue_bytes(int64_t n_cap, int64_t width);
int ha_qplan_batch_f32ids(const float *const *ids, const int64_t *n, void *const *plans, int64_t count,
                          ha_stream_t stream);
int ha_qplan_batch_u64ids(const uint64_t *const *ids, const int64_t *n, void *const *plans, int64_t count,
                          ha_stream_t stream);
int ha_qqueue_batch(int64_t rows, int64_t width, void *const *plans_a, const int64_t *n_a, void *const *plans_g,
                    const int64_t *n_g, void *const *queues, int64_t queue_n_cap, int64_t count, ha_stream_t stream);
int ha_qapply(float *table, int64_t rows, int64_t width, void *plan_cur, int64_t n_cur, const float *grads, float lr,
              void *plan_next, int64_t n_next, float *next_out, const void *queue_cur, int64_t queue_n_cap,
              ha_stream_t stream);
/* ha_qapply with the number of wave items of the queue (wave + copy items; -1 = unknown) when the caller knows it: the launch
 * then has no workgroups that find nothing.  A hint only: too small a number costs time (the waves loop over the items), never
 * correctness.  ha_qqueue_batch_counts = ha_qqueue_batch that also writes {wave items + 1, workgroup items + 1, copy items + 1}
 * of step k's queue to the first three of FOUR pinned host words counts_host[k] (0 = not built yet; the caller zeroes
 * them before the call): queues are built a block of steps ahead, so the host usually has the numbers when it enqueues
 * the step.  The fourth word is only ever written non-zero: bit 0 = the builder counted more items than the queue
 * holds (excluded by the layout's bounds), bit 1 = a plan's occurrence list was not in position order (the serial
 * chain's order; excluded on hardware whose LDS atomics the probe of ha_qstep_init accepted).  Either is a bug: the
 * caller must fail loudly (ops.QueueStepPipeline raises). */
int ha_qapply_sized(float *table, int64_t rows, int64_t width, void *plan_cur, int64_t n_cur, const float *grads,
                    float lr, void *plan_next, int64_t n_next, float *next_out, const void *queue_cur,
                    int64_t queue_n_cap, int64_t wave_items, ha_stream_t stream);
/* `count` consecutive steps enqueued by one call: per-step arrays of ha_qapply_sized's arguments (wave_items may be NULL). */
int ha_qapply_steps(float *table, int64_t rows, int64_t width, float lr, int64_t queue_n_cap, int64_t count,
                    void *const *plan_cur, const int64_t *n_cur, const float *const *grads, void *const *plan_next,
                    const int64_t *n_next, float *const *next_out, const void *const *queue_cur,
                    const int64_t *wave_items, ha_stream_t stream);
int ha_qqueue_batch_counts(int64_t rows, int64_t width, void *const *plans_a, const int64_t *n_a, void *const *plans_g,
                           const int64_t *n_g, void *const *queues, int64_t queue_n_cap, int64_t count,
                           uint32_t *const *counts_host, ha_stream_t stream);
/* Ordering the preparation stream and the apply's stream WITHOUT a packet on the apply's stream (an event record + an event
 * wait at every block boundary cost ~1 us per step at blocks of 16):
 *   (1) queue c must be complete before the apply of step c reads it: ha_qqueue_batch_epochs (= ha_qqueue_batch_counts +
 *       `epochs`, one non-zero tag per step) makes the builder finish every queue with a device-scope release and the tag;
 *       an apply launch that is handed the same tag (ha_qapply_steps_sync / ha_qapply_sync; epoch 0 = no check) looks at it
 *       before its first item -- it is there on the first look when the preparation runs a block ahead; otherwise the
 *       launch polls (~1 s at most), then raises *err = 8 (pinned host word) and does nothing.  The builder never waits
 *       for an apply launch.
 *   (2) the preparation must not rewrite plans / queues that steps still read: the last launch of a call completes
 *       `done_event` (an event of ha_event_create; it rides on that launch's own dispatch packet -- hipExtLaunchKernelGGL
 *       --, nothing is recorded between launches; with nothing to launch it is recorded on the stream), and the caller
 *       makes the preparation stream wait for it (ha_stream_wait_event).
 * The ids of the batches to plan must be complete on the device when the preparation is enqueued (nothing orders them
 * behind work of the apply's stream any more). */
void *ha_event_create(void);
int ha_event_destroy(void *event);
int ha_event_record(void *event, ha_stream_t stream);
int ha_stream_wait_event(ha_stream_t stream, void *event);
int ha_qqueue_batch_epochs(int64_t rows, int64_t width, void *const *plans_a, const int64_t *n_a, void *const *plans_g,
                           const int64_t *n_g, void *const *queues, int64_t queue_n_cap, int64_t count,
                           uint32_t *const *counts_host, const uint32_t *epochs, ha_stream_t stream);
int ha_qapply_steps_sync(float *table, int64_t rows, int64_t width, float lr, int64_t queue_n_cap, int64_t count,
                         void *const *plan_cur, const int64_t *n_cur, const float *const *grads, void *const *plan_next,
                         const int64_t *n_next, float *const *next_out, const void *const *queue_cur,
                         const int64_t *wave_items, const uint32_t *epochs, uint32_t *err, void *done_event,
                         ha_stream_t stream);
int ha_qapply_sync(float *table, int64_t rows, int64_t width, void *plan_cur, int64_t n_cur, const float *grads, float lr,
                   void *plan_next, int64_t n_next, float *next_out, const void *queue_cur, int64_t queue_n_cap,
                   int64_t wave_items, uint32_t epoch, uint32_t *err, void *done_event, ha_stream_t stream);
/* ha_qapply_steps_sync with, per step, the three pinned words the queue's builder wrote (ha_qqueue_batch_counts; NULL / zeros:
 * unknown): a launch that knows its queue's item counts is sized exactly, and its waves ask for their items without reading
 * the counts from the queue's header first (the epoch tag is then looked at beside the item). */
int ha_qapply_steps_counts(float *table, int64_t rows, int64_t width, float lr, int64_t queue_n_cap, int64_t count,
                           void *const *plan_cur, const int64_t *n_cur, const float *const *grads, void *const *plan_next,
                           const int64_t *n_next, float *const *next_out, const void *const *queue_cur,
                           const int64_t *wave_items, const uint32_t *const *counts_host, const uint32_t *epochs, uint32_t *err,
                           void *done_event, ha_stream_t stream);

/* The grid of the apply launch of a step (ha_qapply*) with these batch sizes and launch-size hints (< 0: none), for tests and
 * tools: workgroups [0, ncoop) take the G items, the nworker behind them the wave items -- DEALT: wave wv of worker b takes the
 * items (r * 16 + wv) * nworker + b, r = 0, 1, ...; nworker is odd so that apply and copy items, which alternate over the
 * list, alternate inside every workgroup too.  (ha_qbig_apply keeps worker b on the sixteen items from 16 * b.) */
int ha_qapply_geometry(int64_t width, int64_t n_cur, int64_t n_next, int64_t wave_items, int64_t coop_items, int32_t *ncoop,
                       int32_t *nworker);

/* The row / key exchange of the sharded sparse pull and push as RCCL point-to-point calls made by the LIBRARY on the caller's
 * stream (the reference's worker sends and receives inside C++ too: PSAgent::vecPullSparse / vecPushSparse,
 * ps-lite/include/ps/worker/PSAgent.h:124-237 -- U_s keys and U_s x d floats per server, ps/psf/sparse.h:9-32): one
 * ncclGroupStart / ncclSend + ncclRecv per peer with a non-zero count / ncclGroupEnd -- no Python in the step, no second
 * stream, capturable with the launches around it.  RCCL is resolved at run time (the copy the process has loaded, else
 * /opt/rocm's): ha_xchg_available() = 0 where there is none.  ha_xchg_unique_id: rank 0 makes the 128-byte id, the caller
 * carries it to the other ranks; ha_xchg_create: collective, one communicator per object, on the current device.  Counts are
 * per peer, buffers hold the peers' parts back to back in rank order; this rank's own counts are normally 0. */
int ha_xchg_available(void);
int ha_xchg_unique_id(void *id128);
void *ha_xchg_create(const void *id128, int world, int rank);
int ha_xchg_destroy(void *xchg);
int ha_xchg_bytes(void *xchg, const void *send, const int64_t *send_bytes, void *recv, const int64_t *recv_bytes,
                  ha_stream_t stream);
int ha_xchg_rows(void *xchg, const float *send, const int64_t *send_rows, float *recv, const int64_t *recv_rows, int64_t width,
                 ha_stream_t stream);

/* The WIDE path: batches of more than ha_qstep_max_ids() (7,168) and at most ha_qbig_max_ids() (131,072) ids -- BASELINE
 * configs[2] / configs[3]'s per-GPU shapes, 106,496 and 26,624 ids per step.  The batch is cut into hash buckets by one
 * stable multisplit (ha_qbig_buckets(n_cap) buckets of ~1,024 ids; a bucket may hold at most ha_qstep_max_ids() ids: hot
 * keys with more than ~6,000 occurrences together in one bucket overflow it -- the queues of the steps that touch such a
 * batch carry flag 4, header word and counts_host[k][3], and the caller runs those steps another way: ops.QueueStepPipeline
 * waits for counts_host[k][0] (written last, non-zero once queue k is complete) before it enqueues step k and falls back
 * to the sorted plan + ha_sgd_apply / ha_gather_*); every bucket is planned and joined like a narrow batch, side by side
 * (no sort anywhere), and
 * the apply is the narrow path's launch over all buckets' items.  ws: ha_qbig_plan_bytes(n_cap) bytes per batch (no
 * initialisation); queues: ha_qstep_queue_bytes(n_cap, width).  Semantics, tolerance classes and references as above
 * (Unique<T>'s contract -- every key once, occurrences in order -- unqiue_tools.h:27-48; cpu_deduplicate, ndarray.py:556-576).
 * ha_qbig_plan_batch_* = partition (two launches) + the bucket plans (one launch) of `count` batches; ha_qbig_queue_batch
 * = the queues of `count` steps (two launches); ha_qbig_apply = step c (one launch; coop_items = the queue's number of
 * workgroup items if known, counts_host[k][1] - 1, else -1; epoch / err / done_event as ha_qapply_sync, 0 / NULL / NULL
 * for none).  ha_qbig_plan_view: device pointers into a plan workspace for tests. */
int64_t ha_qbig_max_ids(void);
size_t ha_qbig_plan_bytes(int64_t n_cap);
int ha_qbig_buckets(int64_t n_cap);
int ha_qbig_plan_batch_f32ids(const float *const *ids, const int64_t *n, void *const *ws, int64_t n_cap, int64_t count,
                              ha_stream_t stream);
int ha_qbig_plan_batch_u64ids(const uint64_t *const *ids, const int64_t *n, void *const *ws, int64_t n_cap, int64_t count,
                              ha_stream_t stream);
int ha_qbig_queue_batch(int64_t rows, int64_t width, void *const *ws_a, const int64_t *n_a, void *const *ws_g,
                        const int64_t *n_g, void *const *queues, int64_t n_cap, int64_t count, uint32_t *const *counts_host,
                        const uint32_t *epochs, ha_stream_t stream);
int ha_qbig_apply(float *table, int64_t rows, int64_t width, void *ws_cur, int64_t n_cur, const float *grads, float lr,
                  void *ws_next, int64_t n_next, float *next_out, const void *queue_cur, int64_t n_cap, int64_t coop_items,
                  uint32_t epoch, uint32_t *err, void *done_event, ha_stream_t stream);
int ha_qbig_plan_view(void *ws, int64_t n_cap, void **boff, void **bhdr, void **uniq, void **counts, void **seg, void **gperm,
                      void **meta);

/* serial forms: ha_qprep_* = the plan of one batch (ahead_ids -> plan_ahead; n_ahead = 0: none) and / or the queue of one
 * step from (plan_a, plan_g) (n_a = n_g = 0: none); ha_qstep_*(call c) = ha_qprep_*(batch c+3; queue c+1 from plans
 * c+1 = plan_next, c+2 = plan_b1) followed by ha_qapply(step c).  A stream of batches 0..B-1 is driven as calls
 * c = -3 .. B-1 (n = 0 / null for batches outside [0, B)); four plans rotate and two queues alternate. */
int ha_qprep_f32ids(int64_t rows, int64_t width, const float *ahead_ids, int64_t n_ahead, void *plan_ahead,
                    void *plan_a, int64_t n_a, void *plan_g, int64_t n_g, void *queue_build, int64_t queue_n_cap,
                    ha_stream_t stream);
int ha_qprep_u64ids(int64_t rows, int64_t width, const uint64_t *ahead_ids, int64_t n_ahead, void *plan_ahead,
                    void *plan_a, int64_t n_a, void *plan_g, int64_t n_g, void *queue_build, int64_t queue_n_cap,
                    ha_stream_t stream);
int ha_qstep_f32ids(float *table, int64_t rows, int64_t width,
                    void *plan_cur, int64_t n_cur, const float *grads, float lr,
                    void *plan_next, int64_t n_next, float *next_out, const void *queue_cur,
                    void *plan_b1, int64_t n_b1, void *queue_build, int64_t queue_n_cap,
                    const float *ahead_ids, int64_t n_ahead, void *plan_ahead, ha_stream_t stream);
int ha_qstep_u64ids(float *table, int64_t rows, int64_t width,
                    void *plan_cur, int64_t n_cur, const float *grads, float lr,
                    void *plan_next, int64_t n_next, float *next_out, const void *queue_cur,
                    void *plan_b1, int64_t n_b1, void *queue_build, int64_t queue_n_cap,
                    const uint64_t *ahead_ids, int64_t n_ahead, void *plan_ahead, ha_stream_t stream);
/* a built queue's first words (device memory): {wave items, workgroup items, long, medium, small, copy items, copy
 * medium, copy small, overflow / order word of the apply part, overflow word of the copy part} */
const uint32_t *ha_qstep_queue_header(const void *queue);
/* development aids (tools/qstep_timeline.py): the items of a step with per-wave time stamps, dbg = device
 * uint64[(workgroups) * 4 * 4], zeroed; one plan + one queue with the phase stamps of their workgroups, ph = device
 * uint64[32], zeroed */
int ha_debug_qapply(float *table, int64_t rows, int64_t width, void *plan_cur, int64_t n_cur, const float *grads,
                    float lr, void *plan_next, int64_t n_next, float *next_out, const void *queue_cur,
                    int64_t queue_n_cap, unsigned long long *dbg, ha_stream_t stream);
int ha_debug_qprep_f32ids(int64_t rows, int64_t width, const float *ahead_ids, int64_t n_ahead, void *plan_ahead,
                          void *plan_a, int64_t n_a, void *plan_g, int64_t n_g, void *queue_build, int64_t queue_n_cap,
                          unsigned long long *ph, ha_stream_t stream);

/* A gate for a stream: the stream behind this call does not move on until the host has written a non-zero value to
 * *flag (pinned, device-visible host memory), or about 2 s have passed.  For callers that enqueue a whole sequence
 * behind the gate and release it once everything is queued (bench.py: the device must not wait for the host inside a
 * short timed region). */
int ha_stream_gate(const uint32_t *flag, ha_stream_t stream);
/* measurement aid (tools/occupy_ab.py): `wgs` workgroups of `threads` threads with `lds_bytes` of LDS that hold their wave
 * slots for `ticks` x 10 ns and touch no memory */
int ha_debug_occupy(int64_t wgs, int64_t threads, int64_t lds_bytes, int64_t ticks, ha_stream_t stream);

/* ha_sgd_apply_finish that also warms the memory-side cache for the NEXT batch: waves that have no
 * medium / long-run work (more than half of them) end by touching the table row that position p of
 * next_ids will gather, so the ha_lookup_sort_* / ha_gather_* that follows reads it from the
 * Infinity Cache instead of HBM.  The ids of the next batch are known one step ahead (the reference
 * prefetches too: ParameterServerCommunicate.py:96-139).  Results are those of ha_sgd_apply_finish. */
int ha_sgd_apply_finish_prefetch_f32ids(float *table, int64_t rows, int64_t width,
                                        void *plan_ws, int64_t n, const float *grads, float lr,
                                        const float *next_ids, int64_t next_n, ha_stream_t stream);

/* ---- row-range sharding (in-node replacement of the PS/worker split) -------
 * For the plan's sorted unique keys: offsets[g] = index of the first unique key owned by shard g
 * (offsets[nshard] = n_unique) and local_keys[u] = uniq[u] - starts[owner(u)], where shard g owns
 * rows [starts[g], starts[g+1]) -- AveragePartitioner ranges (ps-lite/include/ps/partitioner.h:46-57)
 * routed like PSAgent (PSAgent.h:537-560).  starts_host[nshard+1] is a HOST array; offsets
 * (int32[nshard+1]) and local_keys (uint32[n]) are device arrays. */
int ha_shard_bucket(const void *plan_ws, int64_t n, const int64_t *starts_host,
                    int nshard, int32_t *offsets, uint32_t *local_keys,
                    ha_stream_t stream);

/* One call for the routing of a batch: ha_plan_build_* of the ids, then the shard-local keys as
 * ha_shard_bucket writes them, and meta[0] = n_unique, meta[1+g] = number of unique keys owned by
 * shard g (device int64[1+nshard]: the send counts of the counts all-to-all and of the host read-back). */
int ha_shard_route_f32ids(const float *ids, int64_t n, void *plan_ws,
                          const int64_t *starts_host, int nshard, int64_t *meta,
                          uint32_t *local_keys, ha_stream_t stream);
int ha_shard_route_u64ids(const uint64_t *ids, int64_t n, void *plan_ws,
                          const int64_t *starts_host, int nshard, int64_t *meta,
                          uint32_t *local_keys, ha_stream_t stream);

/* The routing of a batch as ONE message per owner: ha_plan_build_* of the ids, then
 * send[g * (1 + cap) + 0] = number of this rank's unique keys that shard g owns, followed by those keys as
 * shard-local offsets (PSAgent.h:537-560), in a fixed frame of 1 + cap int32 per owner (cap >= n), and
 * meta[0] = n_unique, meta[1+g] = the same counts (device int64[1+nshard]) for the host read-back that sizes the
 * row exchanges.  The frames of all ranks travel in one equal-split all-to-all -- the reference sends key
 * lists and their lengths in one message too (PSAgent::vecPullSparse, PSAgent.h:185-237).
 * ha_shard_route_unpack turns the received frames recv[g] into the W key lists concatenated in rank order
 * (keys_out: what ha_gather_u32keys / ha_shard_serve_push take) and recv_cnt[g] (device int64[nshard]). */
int ha_shard_route_pack_f32ids(const float *ids, int64_t n, void *plan_ws,
                               const int64_t *starts_host, int nshard, int64_t cap,
                               int64_t *meta, int32_t *send, ha_stream_t stream);
int ha_shard_route_pack_u64ids(const uint64_t *ids, int64_t n, void *plan_ws,
                               const int64_t *starts_host, int nshard, int64_t cap,
                               int64_t *meta, int32_t *send, ha_stream_t stream);
int ha_shard_route_unpack(const int32_t *recv, int nshard, int64_t cap, int64_t *recv_cnt,
                          uint32_t *keys_out, ha_stream_t stream);

/* The same routing with FIXED frames, for a step whose launches and exchange sizes do not depend on device-side
 * counts (it replays from a hipGraph; PSAgent::vecPullSparse / vecPushSparse, PSAgent.h:124-237, with the next
 * batch routed ahead as ParameterServerCommunicate.py:147-185 prefetches it).  Per owner g:
 *   send[g * (2 + rcap)] = { count_g, overflow, rcap shard-local keys, 0xFFFFFFFF beyond count_g }
 * `overflow` = this batch names more than rcap unique keys of SOME owner (the same word in every frame of the sender:
 * after the equal-split key exchange every rank knows whether any rank overflowed and takes the sized exchange above
 * for that batch).  rowmap[u] = frame slot g * rcap + j of the plan's unique key u (-1 beyond rcap): the row map
 * ha_apply_mapped takes to reduce the gradients of a batch straight into the push frames; posmap[i] = frame slot
 * of position i (nshard * rcap, a zero row, beyond rcap): the key list ha_gather_u32keys takes to expand the
 * pulled row frames to the positions.  ha_shard_frames_unpack: received key frames -> keys_fixed[nshard * rcap]
 * (rank order, 0xFFFFFFFF in unused slots: a zero row for ha_gather_u32keys, skipped by ha_shard_serve_push) and
 * state = { any rank overflowed, keys received } (device int32[2]).  ha_shard_frames_pack is the second half of
 * ha_shard_frames_route_* for a plan that is already built. */
int ha_shard_frames_route_f32ids(const float *ids, int64_t n, void *plan_ws, const int64_t *starts_host,
                                 int nshard, int64_t rcap, int64_t frame_stride, int32_t *send, int32_t *rowmap,
                                 int32_t *posmap, ha_stream_t stream);
int ha_shard_frames_route_u64ids(const uint64_t *ids, int64_t n, void *plan_ws, const int64_t *starts_host,
                                 int nshard, int64_t rcap, int64_t frame_stride, int32_t *send, int32_t *rowmap,
                                 int32_t *posmap, ha_stream_t stream);
int ha_shard_frames_pack(const void *plan_ws, int64_t n, const int64_t *starts_host, int nshard, int64_t rcap,
                         int64_t frame_stride, int32_t *send, int32_t *rowmap, int32_t *posmap, ha_stream_t stream);
int ha_shard_frames_unpack(const int32_t *recv, int nshard, int64_t rcap, int64_t frame_stride, uint32_t *keys_fixed,
                           int32_t *state, ha_stream_t stream);
/* A block of batches in one launch each (the plans by ha_plan_build_batch_*): batch i's frames start
 * i * (2 + rcap) words into every owner's stride, rowmap / posmap / keys_fixed / state are per-batch arrays of `count`
 * device pointers given on the host. */
int ha_shard_frames_pack_batch(const void *const *plan_ws, const int64_t *n, int count, const int64_t *starts_host,
                               int nshard, int64_t rcap, int64_t frame_stride, int32_t *send, int32_t *const *rowmap,
                               int32_t *const *posmap, ha_stream_t stream);
int ha_shard_frames_unpack_batch(const int32_t *recv, int count, int nshard, int64_t rcap, int64_t frame_stride,
                                 uint32_t *const *keys_fixed, int32_t *const *state, ha_stream_t stream);
/* frame_stride: int32 words between the frames of consecutive owners, >= 2 + rcap.  With 2 + rcap the frames of one
 * batch are contiguous; a larger stride interleaves the frames of SEVERAL batches per owner, [owner][batch][2 + rcap],
 * so that the key frames of a block of batches travel in one equal-split all-to-all (herald_amd/sharded.py routes a
 * block of batches at a time, ahead of the steps that use them).
 * ha_shard_frames_serve_pull: ha_shard_frames_unpack and the owner-side gather of a pull in ONE launch
 * (PSHandler::serve(SparsePull), ps-lite/include/ps/server/PSFHandle.h:101-128): rows_out[g * rcap + j, :] =
 * table[key j of rank g, :] for the live slots (unused slots are not written), keys_fixed and state as
 * ha_shard_frames_unpack.  `state` may be pinned host memory: the host then reads the overflow word without a copy
 * in the stream. */
int ha_shard_frames_serve_pull(const float *table, int64_t rows, int64_t width, const int32_t *recv, int nshard,
                               int64_t rcap, int64_t frame_stride, float *rows_out, uint32_t *keys_fixed,
                               int32_t *state, ha_stream_t stream);

/* SIZED frames: the same key frames, routed a block of batches ahead, also leave the per-owner counts of every batch on
 * the device and in pinned host memory, so that the two row exchanges of a step carry exactly the rows the batch names
 * (the reference's messages hold U_s keys and U_s x d floats per server: PSAgent::vecPullSparse / vecPushSparse,
 * ps-lite/include/ps/worker/PSAgent.h:167-172,217-226; ps/psf/sparse.h:9-32) without a host read-back in the step, and
 * the keys a rank owns itself never enter an exchange.
 *   meta (int32[2 + 2 nshard]; meta_dev on the device, meta_host in pinned host memory, same contents):
 *     [0] some rank overflowed its key frames (the batch then takes the sized exchange with a read-back, as above)
 *     [1] keys received   [2 + g] unique keys this rank names of owner g   [2 + nshard + g] keys rank g names of this rank
 *   ha_shard_frames_pack_batch_sized   = ha_shard_frames_pack_batch + the send counts and the SIZED maps (self = this rank):
 *     posmap[i] = 0x80000000 | shard-local key  if position i names a key of this rank (the expand reads the table itself)
 *               = index of its unique key among the unique keys of the OTHER owners in key order (= the row of the
 *                 received rows: the all-to-all concatenates the owners' answers in rank order)
 *               = 0xFFFFFFFF (a zero row) for a batch that overflowed
 *     rowmap[u] = the same compact index for a key of another owner (region A of the push buffer), nshard * rcap + j for
 *                 the j-th key of this rank's own range (region S); -1 for a batch that overflowed
 *   ha_shard_frames_unpack_batch_sized = ha_shard_frames_unpack_batch + the receive counts; meta_host[0] is written last
 *   ha_shard_sized_serve_pull  rows_out[roff(g) + j,:] = table[key j of rank g,:] for the other ranks' requests, roff(g) =
 *     sum of the receive counts of the ranks before g without this rank (PSHandler::serve(SparsePull), PSFHandle.h:101-128)
 *   ha_gather2_u32map          the expand: out[i,:] = table[map & 0x7FFFFFFF,:] if map[i] has bit 31, else recv[map[i],:]
 *   ha_shard_sized_serve_push  push_buf = (2 nshard + 1) * rcap rows: A = rows for the other owners [0, nshard rcap), S =
 *     this rank's own keys [nshard rcap, +rcap), B = the rows received, compact in rank order [(nshard + 1) rcap, ...);
 *     the nshard key lists are merged in rank order and table[key,:] = ((table[key,:] + v_0) + v_1) ... (PSFHandle.h:130-164);
 *     total = keys received (host-known); plan_ws: ha_plan_bytes(nshard * rcap) of scratch
 *   ha_push_apply_scaled_finished  a rank alone (nshard = 1): reduce and server add of its own keys in ONE launch. */
int ha_shard_frames_pack_batch_sized(const void *const *plan_ws, const int64_t *n, int count, const int64_t *starts_host,
                                     int nshard, int self, int64_t rcap, int64_t frame_stride, int32_t *send,
                                     int32_t *const *rowmap, int32_t *const *posmap, int32_t *const *meta_dev,
                                     int32_t *const *meta_host, ha_stream_t stream);
int ha_shard_frames_unpack_batch_sized(const int32_t *recv, int count, int nshard, int64_t rcap, int64_t frame_stride,
                                       uint32_t *const *keys_fixed, int32_t *const *meta_dev, int32_t *const *meta_host,
                                       ha_stream_t stream);
int ha_shard_sized_serve_pull(const float *table, int64_t rows, int64_t width, const uint32_t *keys_fixed, int nshard,
                              int self, int64_t rcap, const int32_t *meta_dev, float *rows_out, ha_stream_t stream);
int ha_gather2_u32map(const float *table, int64_t rows, const float *recv, int64_t recv_rows, int64_t width,
                      const uint32_t *map, int64_t n, float *out, ha_stream_t stream);
int ha_shard_sized_serve_push(float *table, int64_t rows, int64_t width, const uint32_t *keys_fixed, int nshard, int self,
                              int64_t rcap, const int32_t *meta_dev, int64_t total, const float *push_buf, void *plan_ws,
                              ha_stream_t stream);
int ha_push_apply_scaled_finished(float *table, int64_t rows, int64_t width, void *plan_ws, int64_t n, const float *grads,
                                  float scale, ha_stream_t stream);

/* The sharded step as ONE native call: what PSAgent::vecPullSparse / vecPushSparse do inside one C++ call each
 * (ps-lite/include/ps/worker/PSAgent.h:124-237) -- the step's launches and its two row exchanges enqueued on the caller's
 * stream by the library, sized from the per-owner counts the routing left in pinned host memory a block ago.
 * ha_shard_slot describes one routed batch (herald_amd/sharded.py fills it once per routing slot):
 *   counts_host[2 + g] = unique keys this rank names at owner g, [2 + world + g] = unique keys rank g names here (pinned; the
 *   routing block's event has completed -- the caller looked at the overflow word [0] behind it);
 *   keys_fixed / meta_dev / posmap / rowmap: as ha_shard_frames_*_sized left them; plan_ws: the batch's index plan;
 *   owner_plan_ws: ha_plan_bytes(world * rcap + 16) of scratch for the owner-side merge (world > 1).
 * _pull: owner gather -> rows exchange (ha_xchg_rows on `xchg`) -> positions from the own shard / the received rows into out;
 * _push: reduce of scale * values by unique key -> rows exchange -> rank-ordered merge + apply; world 1: the lookup and one
 * reduce-and-add launch, xchg may be NULL.  ha_shard_step = both; ha_shard_steps = `count` steps (slots / outs / values per
 * step).  pull_send / pull_recv: [pull_rows = world * rcap, width]; push_buf: [push_rows = (2 world + 1) rcap, width] (rows
 * for the other owners | own keys | rows received); zero_flags: push_rows zero bytes. */
typedef struct ha_shard_slot {
    int32_t world, rank;
    int64_t rcap, n;
    void *plan_ws;
    const uint32_t *keys_fixed;
    const int32_t *meta_dev;
    const uint32_t *posmap;
    const int32_t *rowmap;
    const int32_t *counts_host;
    void *owner_plan_ws;
} ha_shard_slot;
int ha_shard_step_pull(const float *table, int64_t rows, int64_t width, const ha_shard_slot *slot, void *xchg, float *pull_send,
                       float *pull_recv, int64_t pull_rows, float *out, ha_stream_t stream);
int ha_shard_step_push(float *table, int64_t rows, int64_t width, const ha_shard_slot *slot, void *xchg, float *push_buf,
                       int64_t push_rows, const uint8_t *zero_flags, const float *values, float scale, ha_stream_t stream);
int ha_shard_step(float *table, int64_t rows, int64_t width, const ha_shard_slot *slot, void *xchg, float *pull_send,
                  float *pull_recv, int64_t pull_rows, float *push_buf, int64_t push_rows, const uint8_t *zero_flags, float *out,
                  const float *values, float scale, ha_stream_t stream);
int ha_shard_steps(float *table, int64_t rows, int64_t width, int64_t count, const ha_shard_slot *const *slots, void *xchg,
                   float *pull_send, float *pull_recv, int64_t pull_rows, float *push_buf, int64_t push_rows,
                   const uint8_t *zero_flags, float *const *outs, const float *const *values, float scale, ha_stream_t stream);

/* The same steps on SUM-POOLED access (bags, see ha_gather_sum_* below): the same owner gather, exchanges and owner merge --
 * the rows that cross the fabric are one per unique key either way --; only this rank's own end launches differ.
 *   ha_gather2_sum_u32map  ha_gather2_u32map fused with the sum over each bag: out[b,:] = ((0.0f + r_0) + r_1) + ... over bag
 *     b's positions in position order, one rounding per term, r_j exactly the row ha_gather2_u32map writes for the position
 *     (table[map & 0x7FFFFFFF] if bit 31 is set, else recv[map]; zeros for an index beyond its array, 0xFFFFFFFF included).
 *     Bags, offset clamping, slice rule and argument rules as ha_gather_sum_*; a side without rows is never dereferenced.
 *   ha_apply_mapped_bags   ha_apply_mapped (below) on bag_grads [nbags, width] expanded to [n, width], without the expanded
 *     tensor: fixed bags (bag >= 1, bag_of NULL, n % bag == 0; the source row i / bag is computed in registers) or ragged ones
 *     (bag == 0, bag_of = int32[n] from ha_bag_of).  By unique key where ha_apply_mapped goes by unique key.  Same bits.
 *   ha_push_apply_scaled_bags_finished  ha_push_apply_scaled_finished on the expanded gradient, without it (a FINISHED plan):
 *     the same bits in tolerance modes 0 and 1; in mode 2, where the expanded call would cut long runs into chunks, the
 *     gradient is expanded into the library's per-stream scratch and that call runs (see ha_dedup_reduce_bags).
 *   ha_shard_step_pull_sum / _push_bags / ha_shard_step_bags / ha_shard_steps_bags: the pooled twins of the native steps.  Per
 *     step: nbags bags of bag ids (fixed), or bag == 0 with offsets (device int64[nbags + 1], for the pull) and bag_of (device
 *     int32[n], for the push); out and bag_grads are [nbags, width].
 * Every argument (of every step) is checked before any device access and before anything is enqueued. */
int ha_gather2_sum_u32map(const float *table, int64_t rows, const float *recv, int64_t recv_rows, int64_t width,
                          const uint32_t *map, int64_t n, int64_t bag, const int64_t *offsets, int64_t nbags, float *out,
                          ha_stream_t stream);
int ha_apply_mapped_bags(float *dst, int64_t dst_rows, int64_t width, const void *plan_ws, int64_t n, const float *bag_grads,
                         float lr, const int32_t *rowmap, int64_t bag, const int32_t *bag_of, const uint8_t *dst_init,
                         ha_stream_t stream);
int ha_push_apply_scaled_bags_finished(float *table, int64_t rows, int64_t width, void *plan_ws, int64_t n,
                                       const float *bag_grads, int64_t bag, const int32_t *bag_of, float scale,
                                       ha_stream_t stream);
int ha_shard_step_pull_sum(const float *table, int64_t rows, int64_t width, const ha_shard_slot *slot, void *xchg,
                           float *pull_send, float *pull_recv, int64_t pull_rows, int64_t nbags, int64_t bag,
                           const int64_t *offsets, float *out, ha_stream_t stream);
int ha_shard_step_push_bags(float *table, int64_t rows, int64_t width, const ha_shard_slot *slot, void *xchg, float *push_buf,
                            int64_t push_rows, const uint8_t *zero_flags, const float *bag_grads, int64_t nbags, int64_t bag,
                            const int32_t *bag_of, float scale, ha_stream_t stream);
int ha_shard_step_bags(float *table, int64_t rows, int64_t width, const ha_shard_slot *slot, void *xchg, float *pull_send,
                       float *pull_recv, int64_t pull_rows, float *push_buf, int64_t push_rows, const uint8_t *zero_flags,
                       int64_t nbags, int64_t bag, const int64_t *offsets, const int32_t *bag_of, float *out,
                       const float *bag_grads, float scale, ha_stream_t stream);
int ha_shard_steps_bags(float *table, int64_t rows, int64_t width, int64_t count, const ha_shard_slot *const *slots, void *xchg,
                        float *pull_send, float *pull_recv, int64_t pull_rows, float *push_buf, int64_t push_rows,
                        const uint8_t *zero_flags, const int64_t *nbags, const int64_t *bag, const int64_t *const *offsets,
                        const int32_t *const *bag_of, float *const *outs, const float *const *bag_grads, float scale,
                        ha_stream_t stream);

/* Owner side of a sparse push (PSHandler::serve(SparsePush), ps-lite/include/ps/server/PSFHandle.h:130-164):
 * table[keys[j],:] = (table[keys[j],:] + values[a,:]) + values[b,:] ... over the positions a < b < ... that
 * list the key, i.e. in list order (the W received sorted lists concatenated in rank order).
 * plan_ws: ha_plan_bytes(n) of scratch. */
int ha_shard_serve_push(float *table, int64_t rows, int64_t width, const uint32_t *keys,
                        int64_t n, const float *values, void *plan_ws, ha_stream_t stream);

/* ha_shard_serve_push for the received frames of a framed push: keys_fixed = nshard lists of rcap slots in rank order,
 * each ascending with 0xFFFFFFFF in the unused slots (ha_shard_frames_unpack), values[nshard * rcap, width] the row
 * frames.  The lists are merged (stable: equal keys in rank order) instead of sorted; plan_ws: ha_plan_bytes(nshard *
 * rcap). */
int ha_shard_frames_serve_push(float *table, int64_t rows, int64_t width, const uint32_t *keys_fixed, int nshard,
                               int64_t rcap, const float *values, void *plan_ws, ha_stream_t stream);

/* ---- HET embedding cache (replaces the hetu_cache plugin, src/hetu_cache) ----
 * An opaque device-resident cache of `limit` lines in front of a store (the "server": a table shard
 * plus one int64 version per row, ps-lite/include/ps/server/param.h:119-138).  Semantics of
 * CacheBase::_embeddingLookup / _embeddingUpdate / _embeddingUpdateWithPushKeys
 * (src/hetu_cache/src/cache.cc:60-107, 132-197, 248-335) with LRUCache eviction
 * (lru_cache.cc), LFUCache (lfu_cache.cc) or LFUOptCache (lfuopt_cache.cc) eviction.
 * policy: 0 = LRU, 1 = LFU, 2 = LFUOpt.  max_batch bounds the keys of one call.
 * key_kind: 0 = float32 ids (the *_raw entry points, cache.cc:49-58), 1 = uint64 keys.
 * dest / grads / keys are DEVICE pointers; all calls are asynchronous on `stream`. */
typedef struct ha_cache ha_cache;
ha_cache *ha_cache_create(int policy, int64_t limit, int64_t length,
                          int64_t width, int64_t max_batch);
void ha_cache_destroy(ha_cache *cache);
int ha_cache_set_bounds(ha_cache *cache, int64_t pull_bound, int64_t push_bound);
int ha_cache_set_bypass(ha_cache *cache, int bypass);
/* store rows [row_start, row_start+store_rows) of the global table live at `table`;
 * versions[store_rows] are the server-side row versions (zero-initialised by the caller). */
int ha_cache_bind_store(ha_cache *cache, float *table, int64_t *versions,
                        int64_t store_rows, int64_t row_start);
int ha_cache_lookup(ha_cache *cache, const void *keys, int key_kind, int64_t n,
                    float *dest, ha_stream_t stream);
/* The stable sort of a lookup's keys ONE BATCH EARLY, beside the calls of the current batch (the reference's loader hands
 * the ids over a batch ahead: python/hetu/dataloader.py:63-98).  `stream` forks into a stream of the cache's own here and
 * joins it in ha_cache_lookup_presorted(same keys, kind, n) -- anything else there is an error; the keys must not change in
 * between.  Batches beyond 36,864 keys are accepted and ignored (their lookup sorts by itself).  Results are those of
 * ha_cache_lookup, bit for bit (cache.cc:60-107). */
int ha_cache_sort_ahead(ha_cache *cache, const void *keys, int key_kind, int64_t n, ha_stream_t stream);
int ha_cache_lookup_presorted(ha_cache *cache, const void *keys, int key_kind, int64_t n,
                              float *dest, ha_stream_t stream);
/* The sorts of the next `count` (<= 16) lookups in ONE launch on `stream` -- no second stream, no event edge --, into a ring of
 * plan workspaces: for a caller that has its ids a block of batches early (the work-queue step's lookahead).  The
 * ha_cache_lookup_presorted calls that follow must name these key buffers in this order; 1 .. min(max_batch, 36,864) keys per
 * batch; the first call allocates the ring (not inside a stream capture).  Results: those of ha_cache_lookup. */
int ha_cache_sort_ahead_batch(ha_cache *cache, const void *const *keys, int key_kind, const int64_t *n, int count,
                              ha_stream_t stream);
/* The PLANNED flow (csrc/cache_block.hip; LRU, LFU, LFUOpt over a local store -- device or pinned host memory --, LRU with
 * limit >= max_batch): CacheBase::_embeddingLookup and _embeddingUpdate (ha_cache_plan_block) or _embeddingUpdateWithPushKeys
 * (ha_cache_plan_block_push_keys) of the same keys, batch after batch (src/hetu_cache/src/cache.cc:60-107, 132-197; the training loop of
 * python/hetu/cstable.py:38-56), with the BOOKKEEPING of a block of up to 16 batches done ahead: which lines a batch hits and
 * misses, the slots of the misses, the lines the policy evicts for them (LRUCache::insert lru_cache.cc:9-25; LFUCache
 * lfu_cache.cc:9-42 and LFUOptCache lfuopt_cache.cc:9-60: the least (use, arrival) of all lines, kept as a two-level minimum
 * by the bookkeeping; they require that every resident line was updated since its lookup when the planned flow takes over --
 * true after any lookup + update pair), update counters and the bounded push (cache.cc:159) follow from the ids alone.  ha_cache_plan_block enqueues, on `side`, the index plans of the
 * block's batches and ONE bookkeeping launch that leaves per batch the items of its two row launches; `main` = the stream of
 * those row launches (what is enqueued on it so far is ordered in front of the bookkeeping for the first blocks and after
 * call-by-call calls ONLY: in steady state the key buffers must be complete on the device before the call -- see "Ordering"
 * under ha_cache_plan_block_push_keys).  Then, per batch and in order,
 * ha_cache_lookup_planned (ONE launch: the staleness-bounded pull decided as the rows are read, rows to dest) and
 * ha_cache_update_planned (ONE launch: ordered accumulate, the pushed lines' store rows in the same pass, evicted dirty lines,
 * versions).  Results: those of ha_cache_lookup + ha_cache_update_same_keys call by call.  At most two blocks are outstanding
 * (plan block b + 1 when block b starts: its bookkeeping then runs beside block b's rows); the key buffers stay unchanged
 * until the bookkeeping has run; the call-by-call entry points (and ha_cache_set_bounds / _bypass) are refused while planned
 * calls are outstanding (ha_cache_plan_pending); ha_cache_perf after a planned call reports that call; ha_cache_state /
 * ha_cache_snapshot see the bookkeeping of every planned batch, i.e. are meaningful at the end of a block. */
int ha_cache_plan_block(ha_cache *cache, const void *const *keys, int key_kind, const int64_t *n, int count,
                        ha_stream_t side, ha_stream_t main);
/* ha_cache_plan_block for batches whose update is CacheBase::_embeddingUpdateWithPushKeys (cache.cc:248-335; the laia
 * scheduler's push plans): a line is pushed iff its key is one of the batch's push keys and the line holds data; push_bound
 * plays no part; EVERY line of the batch gets version += its update counter, pushed or not, and only pushed lines start their
 * gradient and counter again at 0; pending evictions are pushed as usual.  LFU / LFUOpt: a key whose insert did not stay, or
 * whose line the batch's own first insert evicted, reaches the update as a line without data -- not pushed, its gradient
 * dropped (the evicted line itself is pushed as an eviction).  Per batch i: push_keys[i] = n_push[i] keys of `push_kind`
 * (0 float32, 1 64-bit integers, independent of key_kind), SORTED ascending (duplicates allowed), 0 <= n_push[i] <= max_batch
 * (0: only evictions are pushed); n_push[i] < 0 plans batch i in bound mode (as ha_cache_plan_block), so one block may mix both.
 * The push-key buffers follow the keys' rule: unchanged until the bookkeeping has run.  The lookups and updates are
 * ha_cache_lookup_planned / ha_cache_update_planned / ha_cache_run_planned_pairs, unchanged.  Results: those of
 * ha_cache_lookup + ha_cache_update_with_push_keys call by call.
 * Ordering: this entry point ALWAYS orders its work on `side` behind everything enqueued on `main` so far (ids and push keys
 * written there just before the call are read as written).  ha_cache_plan_block does so only for the first blocks and after
 * call-by-call calls; in steady state (from the fourth block on) it waits only for the rows of the block that last used its
 * buffers, so key buffers it is given must be complete by other means: staged and synchronised ahead, or the caller makes
 * `side` wait for an event it records on `main` in front of the call (herald_amd/cache.py: plan_block(after_current=True);
 * the cost of that wait per block is not measured). */
int ha_cache_plan_block_push_keys(ha_cache *cache, const void *const *keys, int key_kind, const int64_t *n,
                                  const void *const *push_keys, int push_kind, const int64_t *n_push, int count,
                                  ha_stream_t side, ha_stream_t main);
int ha_cache_lookup_planned(ha_cache *cache, int64_t n, float *dest, ha_stream_t stream);
int ha_cache_update_planned(ha_cache *cache, int64_t n, const float *grads, ha_stream_t stream);
int ha_cache_plan_pending(ha_cache *cache);
/* `count` planned pairs by one call: ha_cache_lookup_planned(n[k], dests[k]) then ha_cache_update_planned(n[k], grads[k]) */
int ha_cache_run_planned_pairs(ha_cache *cache, int count, const int64_t *n, float *const *dests, const float *const *grads,
                               ha_stream_t stream);
/* SUM-POOLED access in the planned flow (csrc/cache_block.hip): the embedding_lookup_op + reduce_sum_op(axes=1) pair of the
 * reference's emb_sum_* models over a cached table, without the per-occurrence [n, width] tensors on either side.  Bags as
 * ha_gather_sum_*: fixed -- bag >= 1, offsets == NULL, n == nbags * bag, occurrence i belongs to bag i / bag -- or ragged -- a
 * device int64 offsets[nbags + 1], every entry clamped to [0, n] and every bag's end to its start, so nothing outside the
 * batch is read and nothing outside out[nbags, width] written, whatever offsets holds.  Exactly one of the two.
 *
 * ha_cache_lookup_sum_planned: the lookup of the next planned batch, delivered pooled.  With r_j the row
 * ha_cache_lookup_planned would have written for occurrence j: out[b,:] = ((0.0f + r_lo) + r_lo+1) + ... in position order, one
 * __fadd_rn per term -- bit for bit ha_cache_lookup_planned followed by ha_gather_sum over the ids 0 .. n-1.  An empty bag is
 * zeros; a key the cache has no line for adds +0.0f.  It takes ha_cache_lookup_planned's place in the block's call sequence
 * (same order, same wait for the bookkeeping, same ha_cache_perf record), and every side effect on the cache is that lookup's:
 * the line of a pulled key (a miss, version -1, or a store version ahead by more than pull_bound) is refreshed with the store
 * row (+ the line's gradient row, Line::addup) and its version staged for the update.  The refresh is made by the waves whose
 * bag holds the key's first occurrence: every occurrence must lie in a bag (offsets[0] <= 0, offsets[nbags] >= n, entries
 * non-decreasing), or the lines whose first occurrence lies in none are not refreshed.
 *
 * ha_cache_update_planned_bags: the update of the planned batch from the POOLED gradient bag_grads[nbags, width]: occurrence i
 * takes row i / bag (bag >= 1, bag_of == NULL, n == nbags * bag) or row bag_of[i] (device int32 [n] with entries in [0, nbags),
 * from ha_bag_of; bag == 0) -- exactly one of the two, as ha_sgd_apply_bags (n == 0: bag_of may be NULL).  Bit for bit ha_cache_update_planned on the
 * gradient expanded to [n, width], in bound mode and in push-key mode; it takes that call's place in the sequence.
 *
 * The state either pooled call leaves is the state its unpooled counterpart leaves, so a pooled lookup may be followed by an
 * unpooled update and the other way round.  The steps of a push-pull chain (ha_cache_plan_block_push_pull) are not pooled by
 * these two calls: both refuse such a block, and an open chain, before anything is enqueued -- a chain's pooled entries are
 * ha_cache_push_pull_planned_bags. */
int ha_cache_lookup_sum_planned(ha_cache *cache, int64_t n, int64_t nbags, int64_t bag, const int64_t *offsets, float *out,
                                ha_stream_t stream);
int ha_cache_update_planned_bags(ha_cache *cache, int64_t n, const float *bag_grads, int64_t nbags, int64_t bag,
                                 const int32_t *bag_of, ha_stream_t stream);
/* `count` planned pairs of n ids in fixed bags by one call: ha_cache_lookup_sum_planned(n, nbags, bag, NULL, outs[k]) then
 * ha_cache_update_planned_bags(n, bag_grads[k], nbags, bag, NULL) */
int ha_cache_run_planned_pairs_bags(ha_cache *cache, int count, int64_t n, int64_t nbags, int64_t bag, float *const *outs,
                                    const float *const *bag_grads, ha_stream_t stream);
/* WEIGHTED bags in the planned pairs: the reference's FAE models over a cached cold table (embedding_lookup_op, mul_op by a 0/1
 * mask, reduce_sum_op(axes=1); examples/ctr/tests/hybrid_fae_wdl_criteo.sh runs them with --cache lfu --bound 0 --bsp 0).
 * weights: n device floats, one per occurrence (the batch's [nbags, bag] or [n]).  An occurrence is LIVE when its weight is not
 * zero: +0.0f and -0.0f are zero, a NaN weight is live.  The bookkeeping is a function of the ids alone: plans, hits, misses,
 * slots, victims, versions, update counters, pushes and evictions never look at a weight; the padding id is a key like any other.
 *
 * ha_cache_lookup_wsum_planned: per bag and column acc = +0.0f, then over the LIVE occurrences j of the bag in position order
 * acc = fl(acc + fl(w_j * r_j)) -- one __fmul_rn and one __fadd_rn, no FMA --, r_j the row ha_cache_lookup_planned would have
 * written for occurrence j (a pulled line with a gradient buffer: store row + gradient; a key without a line: zeros).  Bit for
 * bit ha_cache_lookup_planned followed by ha_gather_wsum over the ids 0 .. n-1; all-ones weights give
 * ha_cache_lookup_sum_planned.  The cache is left exactly as the unpooled lookup leaves it: a DEAD head occurrence of a pulled
 * key still refreshes its line with the unweighted row and stages its version.  Bags, offsets, the place in the call sequence
 * and the perf record: ha_cache_lookup_sum_planned's.
 *
 * ha_cache_update_planned_wbags: ha_cache_update_planned on the [n, width] tensor whose row i is
 * t_i = fl(scale * fl(w_i * bag_grads[bag(i), :])) when w_i is not zero and fl(scale * +0.0f) otherwise (+0 for scale >= 0, -0
 * for scale < 0, whatever bag_grads holds there) -- what ha_wbag_grad_rows followed by a multiplication by scale produces --,
 * bit for bit, in bound mode and in push-key mode: gradient buffers, data rows, the store rows of pushed and evicted lines,
 * versions and hasgrad are that call's.  scale must be finite.  No gradient row of a dead occurrence is read.  bag / bag_of:
 * as ha_cache_update_planned_bags; a bag_of entry beyond nbags - 1 reads row nbags - 1 (ha_wbag_grad_rows' clamp).
 * With all-ones weights and scale 1 the call is ha_cache_update_planned_bags.
 *
 * Weighted, sum-pooled and unpooled calls may be mixed freely within a block.  Both calls refuse a push-pull chain block and an
 * open chain, as the _bags calls do. */
int ha_cache_lookup_wsum_planned(ha_cache *cache, int64_t n, int64_t nbags, int64_t bag, const int64_t *offsets,
                                 const float *weights, float *out, ha_stream_t stream);
int ha_cache_update_planned_wbags(ha_cache *cache, int64_t n, const float *bag_grads, const float *weights, float scale,
                                  int64_t nbags, int64_t bag, const int32_t *bag_of, ha_stream_t stream);
/* `count` planned pairs of n ids in fixed bags by one call: ha_cache_lookup_wsum_planned(n, nbags, bag, NULL, weights[k], outs[k])
 * then ha_cache_update_planned_wbags(n, bag_grads[k], weights[k], scale, nbags, bag, NULL) */
int ha_cache_run_planned_pairs_wbags(ha_cache *cache, int count, int64_t n, int64_t nbags, int64_t bag, float *const *outs,
                                     const float *const *bag_grads, const float *const *weights, float scale,
                                     ha_stream_t stream);
/* The planned flow of a PUSH-PULL CHAIN: CacheBase::_embeddingPushPull (cache.cc:356-422), the one cache call per step of the
 * asp-with-prefetch schedule (python/hetu/gpu_ops/ParameterServerCommunicate.py:37-40, 68-72): step = push_pull(pull = the ids of
 * batch k + 1, push = the ids and gradients of batch k).  LRU over a local store only (the LFU policies' planned bookkeeping
 * rests on lookup + update pairs; they keep ha_cache_push_pull).  A block is 1..16 entries; entry i's step pulls batch i
 * (keys[i], n[i] >= 0 keys) and pushes the batch of the entry before it in the chain, across block boundaries.  The chain's
 * FIRST entry has nothing to push: its step is a plain _embeddingLookup (:60-107), made by ha_cache_lookup_planned.  An entry
 * with n[i] < 0, allowed as the LAST entry of a block only, CLOSES the chain: its step pulls nothing and is a plain
 * _embeddingUpdate (:132-197) of the batch pulled last, made by ha_cache_update_planned(n of that batch, grads).  Every other
 * step is ha_cache_push_pull_planned.  A call that is not the one due is refused and changes nothing; ha_cache_plan_pending
 * counts ONE call per entry.
 * Required, and checked before anything is enqueued: n_pull + n_push <= limit for every step (then no line that a step touches
 * is evicted by the step's own insert, and every push key is still resident); a chain starts from a cache with no planned call
 * outstanding and no pending evicted line; pair blocks (ha_cache_plan_block*) are refused while a chain is open.  Keys beyond
 * the cache's range give zeros on the pull side and are ignored on the push side, as in the pair flow.
 * The bookkeeping of the block (one launch, cache_book_chain_kernel: the reference's order of touches -- pull hits, push keys,
 * inserted misses --, slots, evictions, counters, the bounded push) runs on `side`, ALWAYS ordered behind everything enqueued
 * on `main` so far (as ha_cache_plan_block_push_keys).  The dirty lines a step's insert evicts wait for the NEXT step's push
 * (cache.cc:378), so between two steps ha_cache_state reports them as pending.  A step's row work is two launches on the row
 * stream and no bookkeeping: the push half (ordered accumulate, pushed and evicted lines' store rows, versions) and the pull
 * half, which judges staleness with the line's version as it was before the push half's commit (cache.cc:404 against :414-421:
 * a line pushed with more than pull_bound updates is pulled back at once, and Line::addup still adds its gradient).
 * While a chain is open and no planned call is outstanding, the call-by-call entry points are refused: close the chain first
 * (plan a block whose only entry is the closing one, then ha_cache_update_planned).  After the closing step the cache is in
 * the state call-by-call code expects.  Results: those of ha_cache_lookup, ha_cache_push_pull ..., ha_cache_update call by call
 * (tests/test_gpu_cache_planned_push_pull.py holds both to oracle/cache_model.py). */
int ha_cache_plan_block_push_pull(ha_cache *cache, const void *const *keys, int key_kind, const int64_t *n, int count,
                                  ha_stream_t side, ha_stream_t main);
int ha_cache_push_pull_planned(ha_cache *cache, int64_t n_pull, float *dest, int64_t n_push, const float *grads,
                               ha_stream_t stream);
/* `count` middle steps of a chain by one call: ha_cache_push_pull_planned(n_pull[k], dests[k], n_push[k], grads[k]) */
int ha_cache_run_planned_push_pulls(ha_cache *cache, int count, const int64_t *n_pull, float *const *dests,
                                    const int64_t *n_push, const float *const *grads, ha_stream_t stream);
/* The entries of a push-pull chain, SUM-POOLED on both sides (csrc/cache_block.hip): what the emb_sum_* models need of the
 * asp-with-prefetch schedule, without the [n, width] rows of the pull and without the expanded gradient of the push.
 * ha_cache_push_pull_planned_bags serves whichever entry of the chain block is due:
 *   the HEAD          n_push == 0, every push argument 0 / NULL: ha_cache_lookup_sum_planned's launch (one ha_cache_perf record,
 *                     as ha_cache_lookup_planned leaves for a head);
 *   a MIDDLE step     both sides: the push half reads bag_grads[nbags_push, width] -- the pooled gradient of the batch pulled by
 *                     the entry before -- as ha_cache_update_planned_bags does, then the pull half delivers the step's own batch
 *                     pooled into out[nbags_pull, width], judging staleness with the line's version as it was before the push
 *                     half's commit, as ha_cache_push_pull_planned does.  Two launches, no perf record;
 *   the CLOSING entry n_pull == -1, every pull argument 0 / NULL: the push half alone (one perf record, as
 *                     ha_cache_update_planned leaves for a closing entry).
 * Bags per side as in the pooled pair calls: exactly one of bag >= 1 (n == nbags * bag) and the ragged description -- device
 * int64 offsets_pull[nbags_pull + 1] (clamped as ha_cache_lookup_sum_planned clamps them), device int32 bag_of_push[n_push]
 * (ha_bag_of) -- with the argument checks of ha_cache_lookup_sum_planned / ha_cache_update_planned_bags.  Every check is made
 * before anything is enqueued and before the block's call counter moves; a block of pairs, or no chain entry due, is refused.
 * Bit for bit the unpooled entry followed by ha_gather_sum over the ids 0 .. n-1 / fed the expanded gradient, and the same
 * state of cache, store and host: pooled and unpooled entries may alternate freely within one chain.  The pooled pair calls
 * above keep refusing a chain. */
int ha_cache_push_pull_planned_bags(ha_cache *cache, int64_t n_pull, int64_t nbags_pull, int64_t bag_pull,
                                    const int64_t *offsets_pull, float *out, int64_t n_push, int64_t nbags_push, int64_t bag_push,
                                    const int32_t *bag_of_push, const float *bag_grads, ha_stream_t stream);
/* `count` middle steps of n ids in fixed bags by one call: ha_cache_push_pull_planned_bags(n, nbags, bag, NULL, outs[k], n, nbags,
 * bag, NULL, bag_grads[k]) */
int ha_cache_run_planned_push_pulls_bags(ha_cache *cache, int count, int64_t n, int64_t nbags, int64_t bag, float *const *outs,
                                         const float *const *bag_grads, ha_stream_t stream);
int ha_cache_update(ha_cache *cache, const void *keys, int key_kind, int64_t n,
                    const float *grads, ha_stream_t stream);
/* ha_cache_update for the key batch of the immediately preceding ha_cache_lookup on this cache (the
 * training step's lookup / update pair): its index plan is still in the workspace and is reused. */
int ha_cache_update_same_keys(ha_cache *cache, int64_t n, const float *grads, ha_stream_t stream);
int ha_cache_update_with_push_keys(ha_cache *cache, const void *keys,
                                   int key_kind, int64_t n,
                                   const void *push_keys, int push_kind,
                                   int64_t n_push, const float *grads,
                                   ha_stream_t stream);
/* CacheBase::_embeddingPushPull (cache.cc:356-422): push the gradients of `push_keys`, then pull the
 * rows of `pull_keys` (the server pushes before it syncs) -- the ASP-prefetch call of
 * ParameterServerCommunicateOp (python/hetu/gpu_ops/ParameterServerCommunicate.py:37-40,68-72). */
int ha_cache_push_pull(ha_cache *cache, const void *pull_keys, int pull_kind,
                       int64_t n_pull, float *dest, const void *push_keys,
                       int push_kind, int64_t n_push, const float *grads,
                       ha_stream_t stream);
/* ---- the cache over a REMOTE store (rows owned by other ranks, or kept in host memory) ---------------
 * The reference's cache never touches the table: it talks to the servers through syncEmbedding /
 * pushEmbedding (src/hetu_cache/src/hetu_client.cc:6-39 -> ps-lite PSAgent.h:537-627 ->
 * PSFhandle_embedding.cc:5-64).  In remote mode the cache kernels do the same through two device
 * buffers the host side moves (herald_amd/cache.py: exchange of sharded.py, or staging from pinned
 * host memory):
 *   lookup  = ha_cache_lookup_begin   : plan + probe; REQUEST = (req_keys[u], req_versions[u]) for the
 *                                       n_unique keys of the batch, ascending (version -1 = no data);
 *             [the owner decides per key  pull = version == -1 || server_version - version > pull_bound
 *              (kSyncEmbedding, PSFhandle_embedding.cc:30-64) and answers INBOX: inbox_pull[u], and for
 *              pulled keys inbox_versions[u] and the row inbox_rows[inbox_idx[u], :]]
 *             ha_cache_lookup_finish  : touch / insert / evict bookkeeping, rows to `dest`, lines refreshed.
 *   update  = ha_cache_update* as before, except that the lines to push land in the OUTBOX instead of the
 *             store: entries [0, U) = the batch's unique keys in ascending order (out_keys[u] = key, or
 *             0xFFFFFFFF when that line is not pushed), entries [U, U+E) = pending evicted lines in eviction
 *             order; out_updates = the line's update count, out_rows = its gradient row.  The owner applies
 *             row += gradient, version += updates per entry, entries of one sender in list order
 *             (kPushEmbedding, PSFhandle_embedding.cc:5-28).  ha_cache_outbox_count = U + E.
 * embedding_push_pull over a remote store = update, exchange, lookup (the server pushes before it syncs,
 * PSFhandle_embedding.cc:66-79). */
typedef struct {
    uint32_t *req_keys;
    int64_t *req_versions;
    int32_t *inbox_pull, *inbox_idx;
    int64_t *inbox_versions;
    float *inbox_rows;
    uint32_t *out_keys;
    int32_t *out_updates;
    float *out_rows;
    int64_t out_capacity, max_batch;
} ha_cache_remote;
int ha_cache_set_remote(ha_cache *cache);
int ha_cache_remote_buffers(ha_cache *cache, ha_cache_remote *out);
int ha_cache_lookup_begin(ha_cache *cache, const void *keys, int key_kind, int64_t n,
                          int64_t *n_unique_host, ha_stream_t stream);
int ha_cache_lookup_finish(ha_cache *cache, int64_t n, float *dest, ha_stream_t stream);
int ha_cache_outbox_count(ha_cache *cache, int64_t *count_host, ha_stream_t stream);
/* Owners that need no host-side counts (a store on this device or in host memory: no exchange to size): the
 * REQUEST is always padded to n entries with key 0xFFFFFFFF (never pulled) -- pass n_unique_host = NULL and serve
 * n entries --, and after ha_cache_outbox_pad(entries) the updates mark OUTBOX entries [U + E, entries) as not
 * pushed, so outbox[0, entries) can be handed over without ha_cache_outbox_count.  entries must bound U + E: the
 * batch's n plus the n of every lookup since the last update (each evicts at most as many lines as it has keys). */
int ha_cache_outbox_pad(ha_cache *cache, int64_t entries);
/* embedding_push_pull (cache.cc:356-422) over a remote store: begin = touch of the pull keys + the whole
 * push phase (OUTBOX filled, REQUEST = the pull keys' versions after the push phase); the host pushes the
 * outbox and then syncs the request; finish = pull, rows to dest, insert of the pull misses, the push
 * phase's deferred version bump / zeroGrad. */
int ha_cache_push_pull_begin(ha_cache *cache, const void *pull_keys, int pull_kind, int64_t n_pull,
                             const void *push_keys, int push_kind, int64_t n_push,
                             const float *grads, int64_t *n_unique_pull_host, ha_stream_t stream);
int ha_cache_push_pull_finish(ha_cache *cache, float *dest, ha_stream_t stream);
/* ---- sum-pooled access, call by call ("bags": embedding_lookup_op + reduce_sum_op(axes=1) of the emb_sum_* models) ----------
 * The pooled twins of the call-by-call entry points above, for the callers the planned flow does not reach (a cache over a
 * remote store, LFU / LFUOpt on the asp schedule, no ids a block ahead, push plans).  Bags as everywhere: fixed -- bag >= 1,
 * the ragged description NULL, nbags * bag == n --, or ragged -- bag == 0 and device int64 offsets[nbags + 1] (a pull side;
 * clamped to [0, n], an empty bag gives zeros) or device int32 bag_of[n] (a push side; ha_bag_of).  Every argument is checked
 * before any device access and before anything is enqueued; a refused call changes nothing.
 * Lookups: out[b,:] = ((0.0f + r_lo) + r_lo+1) + ... over the rows the unpooled call delivers for bag b's keys, in position
 * order, one rounding per add -- bit for bit that call followed by ha_gather_sum over its rows; the [n, width] rows are never
 * written.  Bookkeeping, line state, versions and ha_cache_perf counts are the unpooled call's; so is the handling of
 * ha_cache_sort_ahead / ha_cache_sort_ahead_batch, and an ha_cache_update_same_keys* may follow either form.
 * Updates: bag_grads[nbags, width] in place of grads[n, width]; occurrence i reads the row of its bag -- bit for bit the
 * unpooled call on the expanded gradient, on the two-launch path (ha_cache_fused_updates counts it) and the general one. */
int ha_cache_lookup_sum(ha_cache *cache, const void *keys, int key_kind, int64_t n, int64_t nbags, int64_t bag,
                        const int64_t *offsets, float *out, ha_stream_t stream);
int ha_cache_lookup_sum_presorted(ha_cache *cache, const void *keys, int key_kind, int64_t n, int64_t nbags, int64_t bag,
                                  const int64_t *offsets, float *out, ha_stream_t stream);
/* remote mode: the second half of a lookup, after the unchanged ha_cache_lookup_begin and the exchange */
int ha_cache_lookup_sum_finish(ha_cache *cache, int64_t n, int64_t nbags, int64_t bag, const int64_t *offsets, float *out,
                               ha_stream_t stream);
int ha_cache_update_bags(ha_cache *cache, const void *keys, int key_kind, int64_t n, const float *bag_grads, int64_t nbags,
                         int64_t bag, const int32_t *bag_of, ha_stream_t stream);
int ha_cache_update_same_keys_bags(ha_cache *cache, int64_t n, const float *bag_grads, int64_t nbags, int64_t bag,
                                   const int32_t *bag_of, ha_stream_t stream);
int ha_cache_update_with_push_keys_bags(ha_cache *cache, const void *keys, int key_kind, int64_t n, const void *push_keys,
                                        int push_kind, int64_t n_push, const float *bag_grads, int64_t nbags, int64_t bag,
                                        const int32_t *bag_of, ha_stream_t stream);
/* ha_cache_push_pull with its two sides pooled independently: the pull side delivers out[nbags_pull, width]; the push side takes
 * bag_grads[nbags_push, width].  A side with nbags < 0 is NOT pooled: `out` is then dest[n_pull, width], `bag_grads` is
 * grads[n_push, width], and the side's bag / ragged arguments are ignored.  Remote stores: ha_cache_push_pull_begin_bags (pooled
 * push side) or ha_cache_push_pull_begin, the exchange, then ha_cache_push_pull_finish_sum (pooled pull side) or
 * ha_cache_push_pull_finish. */
int ha_cache_push_pull_bags(ha_cache *cache, const void *pull_keys, int pull_kind, int64_t n_pull, int64_t nbags_pull,
                            int64_t bag_pull, const int64_t *pull_offsets, float *out, const void *push_keys, int push_kind,
                            int64_t n_push, const float *bag_grads, int64_t nbags_push, int64_t bag_push,
                            const int32_t *push_bag_of, ha_stream_t stream);
int ha_cache_push_pull_begin_bags(ha_cache *cache, const void *pull_keys, int pull_kind, int64_t n_pull, const void *push_keys,
                                  int push_kind, int64_t n_push, const float *bag_grads, int64_t nbags_push, int64_t bag_push,
                                  const int32_t *push_bag_of, int64_t *n_unique_pull_host, ha_stream_t stream);
int ha_cache_push_pull_finish_sum(ha_cache *cache, int64_t nbags, int64_t bag, const int64_t *offsets, float *out,
                                  ha_stream_t stream);
/* Owner side of a remote lookup (kSyncEmbedding, PSFhandle_embedding.cc:30-64) for m requested shard-local
 * keys: pull[j] = versions[j] == -1 || server_versions[key] - versions[j] > bound; pulled rows are packed
 * in request order into rows_out, idx[j] = its row there, ver_out[j] = the server version; *count_dev
 * (device int64) = number of pulled rows.  scan_ws: reserved, may be NULL. */
int ha_store_serve_sync(const float *table, const int64_t *server_versions, int64_t rows, int64_t width,
                        const uint32_t *keys, const int64_t *versions, int64_t m, int64_t bound,
                        int32_t *pull, int32_t *idx, int64_t *ver_out, float *rows_out,
                        int64_t *count_dev, void *scan_ws, ha_stream_t stream);
/* Owner side of the version half of a push: server_versions[keys[j]] += updates[j] (keys >= rows skipped). */
int ha_store_add_versions(int64_t *server_versions, int64_t rows, const uint32_t *keys,
                          const int32_t *updates, int64_t m, ha_stream_t stream);
/* The same server side for a push list whose live keys (< rows; 0xFFFFFFFF = not pushed) are pairwise DISTINCT -- what
 * ha_cache_update_same_keys' two-launch path leaves in the outbox (the batch's unique keys and the victims of one lookup):
 * one launch, table[key,:] += grad_rows[j,:] and server_versions[key] += updates[j], no sort.  The caller vouches for the
 * distinctness (herald_amd.cache asks ha_cache_fused_updates); lists with repeated keys need ha_shard_serve_push's order. */
int ha_store_push_distinct(float *table, int64_t *server_versions, int64_t rows, int64_t width, const uint32_t *keys,
                           const int32_t *updates, const float *grad_rows, int64_t m, ha_stream_t stream);
/* *acc += number of keys below `rows` (device-side traffic accounting of a store) */
int ha_store_count_valid(const uint32_t *keys, int64_t m, int64_t rows, int64_t *acc, ha_stream_t stream);
/* Synchronising inspectors.  perf out[8] = {type(0 pull / 1 push), num_all, num_unique, num_miss,
 * num_transfered, num_evict, is_full, size} of the last call (the perf dict of cache.cc:89-106).
 * state out[8] = {size, pending evictions, free slots, log head, log tail, clock, slots, log cap}. */
int ha_cache_perf(ha_cache *cache, int64_t *out_host, ha_stream_t stream);
int ha_cache_state(ha_cache *cache, int64_t *out_host, ha_stream_t stream);
/* Diagnostics: out_host[16] = the GPU's 100 MHz clock at the phase boundaries of the last lookup's bookkeeping
 * ([0..4] the bookkeeping workgroup, [8..12] the insert / eviction workgroup beside the row copies). */
int ha_cache_phase_times(ha_cache *cache, uint64_t *out_host, ha_stream_t stream);
/* Stage times of the last lookup / update in milliseconds, the fields of the reference's perf dict (`time, sort_time,
 * lookup_time, prepare_time, transfer_time, copy_time, insert_time / cleanup_time`, src/hetu_cache/src/cache.cc:99-105,
 * 189-194; dumped by examples/ctr/run_hetu.py:508-515), measured with HIP events between the call's launches once
 * ha_cache_set_timing(cache, 1) was called (off by default).  out_ms[6] = {whole call, sort, lookup (+ prepare), copy (+
 * insert), transfer, the rest}; -1 = a stage the call did not pass. */
int ha_cache_set_timing(ha_cache *cache, int on);
int ha_cache_stage_times(ha_cache *cache, double *out_ms);
/* Resident lines, unordered, into device arrays of capacity cap; *count_dev (zeroed by the
 * caller) receives the number of resident lines; slots[] index the rows of ha_cache_data/grad. */
int ha_cache_snapshot(ha_cache *cache, int64_t cap, uint32_t *keys,
                      int64_t *version, int32_t *updates, uint64_t *stamp,
                      int32_t *slots, uint64_t *count_dev, ha_stream_t stream);
/* Debug hook behind hetu_cache's insert(EmbeddingPT) (src/hetu_cache/src/python_api.cc:58, lru_cache.cc:9-25):
 * the RESIDENT line of `key` takes `version` and the `width` floats at data_dev; a key that is not resident
 * is left alone (the caller brings the line in with a one-key lookup first). */
int ha_cache_set_line(ha_cache *cache, int64_t key, int64_t version, const float *data_dev, ha_stream_t stream);
float *ha_cache_data(ha_cache *cache);
float *ha_cache_grad(ha_cache *cache);
int64_t ha_cache_limit(ha_cache *cache);
int64_t ha_cache_width(ha_cache *cache);
/* Updates that took the two-launch path of ha_cache_update_same_keys (LRU, local store, the keys of the preceding
 * lookup, limit >= batch: accumulate + one launch for touch / push / commit) since the cache was created.
 * HA_CACHE_FUSED=0 in the environment keeps every update on the general path. */
int64_t ha_cache_fused_updates(ha_cache *cache);

/* ---- laia embedding scheduler (replaces the laia_cache plugin, laia/) --------
 * LaiaScheduler::get_dist + the snapshot update of launch() (laia/src/laia_scheduler.cc:115-271) for
 * one global batch of nrank*mini_bs samples: probing / plan extraction on the GPU, the greedy
 * assignment and the MiniLRUCache bookkeeping (laia/include/mini_lru_cache.h) on the calling host
 * thread.  samples_host[num_sample*num_table] are the embedding keys (all < key_limit,
 * nrank*key_limit < 2^32).  ha_laia_next writes dist_out[nrank*mini_bs] (global sample indices per
 * worker) and the workers' sorted communication plans concatenated into plan_out with
 * plan_off[nrank+1].  All pointers are HOST pointers; the call synchronises its private stream. */
typedef struct ha_laia ha_laia;
ha_laia *ha_laia_create(const uint64_t *samples_host, int64_t num_sample,
                        int64_t num_table, int64_t nrank, int64_t cache_size,
                        int64_t key_limit, int64_t max_batch);
void ha_laia_destroy(ha_laia *sched);
int ha_laia_next(ha_laia *sched, int64_t batch_id, int64_t mini_bs,
                 int64_t *dist_out, uint64_t *plan_out, int64_t plan_cap_elems,
                 int64_t *plan_off);
/* One batch ahead: the caller announces the batch of its NEXT ha_laia_next* call (the reference's launch() walks them in
 * order, laia/src/laia_scheduler.cc:115-169); the call that follows the hint enqueues the announced batch before it returns
 * its own results.  The announced call must follow; scheduler state read in between is one batch ahead.  Device-resident
 * state only (ignored otherwise); next_batch_id < 0 withdraws an unused hint. */
int ha_laia_hint_next(ha_laia *laia, int64_t next_batch_id);
/* ha_laia_next for a caller that wants ONE worker's plan (what LaiaScheduler::launch queues for its own rank,
 * laia/src/laia_scheduler.cc:140-168): plan_out holds that plan, plan_off[w] = 0 for w <= rank and its length behind;
 * dist_out as ha_laia_next.  With the scheduler state on the device only that worker's plan rows cross PCIe. */
int ha_laia_next_for_rank(ha_laia *h, int64_t batch_id, int64_t mini_bs, int64_t rank, int64_t *dist_out,
                          uint64_t *plan_out, int64_t plan_cap_elems, int64_t *plan_off);
int64_t ha_laia_snapshot_keys(ha_laia *sched, int64_t worker, int32_t *out,
                              int64_t cap);

/* TopkScheduler::get_dist + the snapshot update of its launch() for one global batch
 * (laia/src/topk_scheduler.cc:362-502, 319-345): only the tables table_order[0..top_k) are scored, the
 * batch and every worker's quota are cut into num_threads slices assigned independently, a sample is
 * offered to the workers starting at the one that first reached its top score, and plan[w] = keys of w's
 * own samples that w's snapshot holds valid.  Outputs as ha_laia_next.  num_threads must divide the
 * work so that no slice holds more samples than nrank x its quota (the reference writes out of bounds
 * there). */
int ha_laia_next_topk(ha_laia *sched, int64_t batch_id, int64_t mini_bs,
                      const int32_t *table_order, int64_t top_k, int64_t num_threads,
                      int64_t *dist_out, uint64_t *plan_out, int64_t plan_cap_elems,
                      int64_t *plan_off);
/* out[4*nrank] = miss_pull, miss_push, update_pull, update_push per worker, accumulated over the
 * batches scheduled so far (TopkScheduler::report_cache_perf, topk_scheduler.cc:504-527). */
int ha_laia_counters(ha_laia *sched, int64_t *out);
/* Wall time of the scheduler per phase, summed since ha_laia_create (scheduler us per global
 * batch): out[4] = {calls of ha_laia_next*, whole calls us, host greedy assignment us, host snapshot
 * (MiniLRU) bookkeeping us}; the remainder of the total is GPU kernels, transfers and waits. */
int ha_laia_timing(ha_laia *h, double *out);
/* device-resident mode: out[4] = {calls, us enqueueing the next batch's launches, us waiting for a batch's results, us copying
 * dist and plan out of the pinned mirror}, summed since creation */
int ha_laia_timing_device(ha_laia *h, double *out);
/* 1 = the scheduler state (MiniLRU snapshots as stamp logs, assignment, sorted-unique plan / touched rows) lives on the
 * device -- LaiaScheduler and TopkScheduler alike, whenever cache_size >= global batch x tables (decided at the first
 * batch; HA_LAIA_HOST=1 keeps it on the host) --, 0 = host snapshots, -1 = no batch scheduled yet. */
int ha_laia_on_device(ha_laia *h);

/* Local-shared plan distribution (laia/include/share_mem.h:40-193, ring_buffer.h:13-125): a
 * single-producer / single-consumer ring of uint64 words in POSIX shared memory, message-framed.
 * The scheduler of local rank 0 creates "laia_cache_<i>" for every local worker i and sends it its
 * [plan, dist] stream; worker i opens its ring and receives.  send: 1 sent / 0 no room yet / -1 never
 * fits.  recv: message length / -1 empty / -2 `out` too small (*needed = length). */
typedef struct ha_shm_ring ha_shm_ring;
ha_shm_ring *ha_shm_ring_open(const char *name, int create, int64_t capacity_words);
void ha_shm_ring_close(ha_shm_ring *ring);
int ha_shm_ring_send(ha_shm_ring *ring, const uint64_t *words, int64_t n);
int64_t ha_shm_ring_recv(ha_shm_ring *ring, uint64_t *out, int64_t cap_words, int64_t *needed);
int64_t ha_shm_ring_pending_words(ha_shm_ring *ring);

/* Development aid: ha_sgd_apply with per-wave time stamps, dbg[4*n] u64 =
 * {s_memrealtime start, end (10 ns ticks), role/len, shader cycles} per sorted position. */
int ha_debug_apply_timeline(float *table, int64_t rows, int64_t width,
                            const void *plan_ws, int64_t n, const float *grads,
                            float lr, unsigned long long *dbg,
                            ha_stream_t stream);

/* One-call convenience used by the reference-named SGDOptimizerSparseUpdate:
 * plan + apply using an internal per-stream workspace. */
int ha_sgd_sparse_update_f32ids(float *table, int64_t rows, int64_t width,
                                const float *ids, int64_t n,
                                const float *grads, float lr,
                                ha_stream_t stream);

/* ---- sum-pooled embedding lookup ("bags") and its sparse SGD apply ------------------------------------
 * The fused form of embedding_lookup_op + reduce_sum_op(axes=1) of the reference's pooled CTR models
 * (examples/ctr/models/emb_sum_*.py).  A BAG is the list of ids of one sample.
 *   fixed bags : bag >= 1, offsets NULL -- ids is [nbags, bag] (n == nbags * bag), occurrence i is in bag i / bag;
 *   ragged bags: bag == 0, offsets = device int64[nbags + 1], offsets[0] = 0, offsets[nbags] = n, non-decreasing --
 *                bag b is ids[offsets[b] : offsets[b + 1]]; empty bags are allowed.
 * Exactly one of the two is given.  The kernels clamp every offset to [0, n]: no id at or beyond n is read and no
 * output row at or beyond nbags written, whatever offsets holds.
 *
 * Forward: out[b,:] = ((0.0f + r_0) + r_1) + ... + r_{m-1}, r_j = the table row of the bag's j-th id, added in position
 * order with one rounding per term (the reference's own order is unspecified; this one is the same on every path here).
 * An id >= rows contributes a zero row, as in ha_gather_*; an empty bag gives zeros.  Any width >= 1; width % 4 == 0
 * with 16-byte aligned table / out takes the 16-byte path. */
int ha_gather_sum_f32ids(const float *table, int64_t rows, int64_t width, const float *ids, int64_t n, int64_t bag,
                         const int64_t *offsets, int64_t nbags, float *out, ha_stream_t stream);
int ha_gather_sum_u64ids(const float *table, int64_t rows, int64_t width, const uint64_t *ids, int64_t n, int64_t bag,
                         const int64_t *offsets, int64_t nbags, float *out, ha_stream_t stream);
/* The same with the rows named by uint32 keys (device uint32[n]) into a buffer of rows: the contract of
 * ha_gather_sum_f32ids to the letter -- position-ordered chain, a key >= rows adds a zero row, clamped offsets, the same
 * slice rule and ha_debug_bag_slice.  The pull of the row-sharded store (herald_amd/sharded.py, pull_sum): rows_buf is
 * the [u, width] buffer of the unique rows a batch received and keys its plan's inverse[n], so the per-occurrence rows
 * [n, width] are neither written nor read back. */
int ha_gather_sum_u32keys(const float *rows_buf, int64_t rows, int64_t width, const uint32_t *keys, int64_t n, int64_t bag,
                          const int64_t *offsets, int64_t nbags, float *out, ha_stream_t stream);
/* bag_of[i] (int32[n]) = the bag of occurrence i of ragged bags; always in [0, nbags). */
int ha_bag_of(const int64_t *offsets, int64_t nbags, int64_t n, int32_t *bag_of, ha_stream_t stream);
/* Backward: bag_grads is the gradient of the pooled output, [nbags, width]; occurrence i takes the row of its bag:
 *   table[key_i,:] -= lr * bag_grads[bag_of(i),:]   for every occurrence, in occurrence order, two roundings each
 * -- bit for bit what ha_sgd_apply gives on bag_grads expanded to [n, width] (cpu_SGDOptimizerSparseUpdate on
 * reduce_sum's broadcast gradient) and what ha_apply_mapped gives with valmap = bag_of, in tolerance mode too.
 * plan_ws: a plan of the n ids, sorted (ha_plan_sort_*) or finished.  Fixed bags: bag >= 1, bag_of NULL -- the source
 * row i / bag is computed in registers; ragged bags: bag == 0 and bag_of from ha_bag_of (every entry must name a row of
 * bag_grads).  One wave per sorted position for every n. */
int ha_sgd_apply_bags(float *table, int64_t rows, int64_t width, const void *plan_ws, int64_t n, const float *bag_grads,
                      int64_t bag, const int32_t *bag_of, float lr, ha_stream_t stream);
/* ha_dedup_reduce_scaled on the pooled gradient: the worker side of a PS sparse push of a sum-pooled lookup,
 *   reduced[u,:] = (0 + scale * bag_grads[bag_of(i0),:]) + scale * bag_grads[bag_of(i1),:] + ...
 * over the occurrences i0 < i1 < ... of unique key u -- bit for bit ha_dedup_reduce_scaled on bag_grads expanded to
 * [n, width], on every path that call takes (by sorted position up to 36,864 ids; by unique key of a FINISHED plan
 * beyond, which is what plan_ws must then be) and in tolerance modes 0 and 1 (the same runs take the same chain or tree).
 * Exactly one of bag >= 1 (fixed bags, bag_of NULL, n % bag == 0) and bag_of (int32[n] from ha_bag_of, bag == 0), as
 * ha_sgd_apply_bags; every entry of bag_of must name a row of bag_grads.  reduced holds n rows, the first n_unique are
 * written.  width % 4 == 0 with 16-byte aligned bag_grads / reduced takes the 16-byte path, anything else the scalar one.
 * Tolerance mode 2 cuts long runs into chunks in plain launches only and there are no chunked bags: in that mode a batch
 * of 36,865 .. 2^20 ids that the expanded call would chunk (width % 4 == 0, width <= 256, 16-byte aligned reduced) is
 * expanded into the library's per-stream scratch (n * width floats) and goes through ha_dedup_reduce_scaled's own launch
 * -- the same bits as that call in mode 2 on a 16-byte aligned expanded gradient, without the saving.  That scratch is
 * the one the one-call entry points (ha_sgd_sparse_update_*, ...) use on the same stream, and it is freed and allocated
 * anew when it has to grow: plan_ws, bag_of, bag_grads and reduced must be the caller's own allocations, never pointers
 * into it.  Arguments are checked before any device access. */
int ha_dedup_reduce_bags(const void *plan_ws, int64_t n, const float *bag_grads, int64_t width, int64_t bag,
                         const int32_t *bag_of, float scale, float *reduced, ha_stream_t stream);
/* One call: plan + (ha_bag_of +) ha_sgd_apply_bags, on an internal per-stream workspace. */
int ha_sgd_sparse_update_bags_f32ids(float *table, int64_t rows, int64_t width, const float *ids, int64_t n,
                                     const float *bag_grads, int64_t bag, const int64_t *offsets, int64_t nbags, float lr,
                                     ha_stream_t stream);
int ha_sgd_sparse_update_bags_u64ids(float *table, int64_t rows, int64_t width, const uint64_t *ids, int64_t n,
                                     const float *bag_grads, int64_t bag, const int64_t *offsets, int64_t nbags, float lr,
                                     ha_stream_t stream);
/* Momentum / Nesterov from the pooled gradient, one call on an internal per-stream workspace: plan, (ha_bag_of,)
 * ha_sgd_apply_bags on velocity -- and on param too for Nesterov --, then the dense phase of MomentumOptimizerSparseUpdate
 * over the whole table (it runs for n == 0 as well, as there).  Bit for bit MomentumOptimizerSparseUpdate on bag_grads
 * expanded to [n, width]; the tolerance mode is honoured exactly as that symbol honours it.  nesterov: 0 / 1.  Argument
 * checks as ha_sgd_sparse_update_bags_*, before any device access. */
int ha_momentum_sparse_update_bags_f32ids(float *param, int64_t rows, int64_t width, const float *ids, int64_t n,
                                          const float *bag_grads, int64_t bag, const int64_t *offsets, int64_t nbags,
                                          float *velocity, float lr, float momentum, int nesterov, ha_stream_t stream);
int ha_momentum_sparse_update_bags_u64ids(float *param, int64_t rows, int64_t width, const uint64_t *ids, int64_t n,
                                          const float *bag_grads, int64_t bag, const int64_t *offsets, int64_t nbags,
                                          float *velocity, float lr, float momentum, int nesterov, ha_stream_t stream);
/* FM-pooled lookup: the second-order term of the reference's DeepFM models (examples/ctr/models/deepfm_criteo.py:24-39),
 * where one lookup is consumed as rows (the DNN), as reduce_sum_op(axes=1) and as reduce_sum_op(mul_op(e, e), axes=1).
 * Bags -- fixed or ragged, exactly one of bag >= 1 and offsets, offsets clamped -- are those of ha_gather_sum_*.  Per bag b
 * and column c, with r_j the table rows of the bag's ids in position order:
 *   out_sum[b,c] = S = ((0.0f + r_0) + r_1) + ...                   the chain of ha_gather_sum_*: the same bits
 *   Q                = ((0.0f + fl(r_0*r_0)) + fl(r_1*r_1)) + ...   one multiply and one add per term, each rounded
 *   out_fm[b,c]      = fl(0.5f * fl(fl(S*S) - Q))                   three roundings, nothing contracted
 *   out_rows[i,:]    = the row of occurrence i ([n, width]), as ha_gather_* writes it
 * An id >= rows is a zero row in all three outputs; an empty bag gives zeros in out_sum and out_fm.  out_rows may be NULL
 * (the caller holds the rows already: `table` is its [n, width] row buffer and ids are 0 .. n-1).  Ragged bags: the row of
 * an occurrence that lies in no bag (before offsets[0] or at / beyond offsets[nbags]) is not written.  Any width >= 1;
 * width % 4 == 0 with 16-byte aligned table / outputs takes the 16-byte path.  Rows read once, written once:
 * n * (8 * width + 4) bytes.  Arguments are checked before any device access (out_sum and out_fm must not be NULL). */
int ha_gather_fm_f32ids(const float *table, int64_t rows, int64_t width, const float *ids, int64_t n, int64_t bag,
                        const int64_t *offsets, int64_t nbags, float *out_rows, float *out_sum, float *out_fm,
                        ha_stream_t stream);
int ha_gather_fm_u64ids(const float *table, int64_t rows, int64_t width, const uint64_t *ids, int64_t n, int64_t bag,
                        const int64_t *offsets, int64_t nbags, float *out_rows, float *out_sum, float *out_fm,
                        ha_stream_t stream);
/* Its backward, one elementwise launch: the per-occurrence gradient [n, width] from the adjoints of the three consumers,
 *   out[i,c] = fl( fl(g_rows[i,c] + fl(g_fm[b,c] * sum[b,c])) - fl(g_fm[b,c] * emb_rows[i,c]) ),   b = the bag of i.
 * g_rows [n, width]: the gradient of out_rows, or NULL when nothing consumed the rows -- then
 *   out = fl(fl(g_fm*sum) - fl(g_fm*emb_rows)).
 * g_fm, sum [nbags, width]: the gradient of out_fm and the forward's out_sum; emb_rows [n, width]: the forward's out_rows.
 * The reference's executor adds the three adjoints in its topological order, which is specified nowhere: the order above is
 * this project's fixed choice (as the bag sum's order is), the same on every path here.  Fixed bags: bag >= 1, bag_of NULL,
 * n == nbags * bag, b = i / bag in registers; ragged bags: bag == 0 and bag_of = int32[n] from ha_bag_of -- exactly one of
 * the two, as ha_sgd_apply_bags.  out may alias g_rows (in place) and nothing else.  The result is an ordinary unpooled
 * gradient: ha_sgd_apply, the fused optimizers and the PS / cache pushes take it as they take any [n, width] gradient.
 * width % 4 == 0 with every pointer 16-byte aligned takes 16-byte accesses.  Checked before any device access. */
int ha_fm_grad_rows(const float *g_rows, const float *emb_rows, const float *sum, const float *g_fm, int64_t n,
                    int64_t width, int64_t bag, const int32_t *bag_of, int64_t nbags, float *out, ha_stream_t stream);
/* The backward of ha_gather_fm_* when nothing consumed the rows (out_rows == NULL: the pooled DeepFM,
 * examples/ctr/models/emb_sum_deepfm_avazu.py, where the lookup is consumed as S and as 0.5 * (S*S - Q) only), fused into the
 * sparse SGD apply: ONE launch that reads every unique row once and writes it once; no [n, width] tensor exists.
 * plan_ws: a FINISHED plan of the n ids (ha_plan_build_*, or ha_plan_sort_* + ha_plan_finish): what ha_sgd_apply_finished
 * takes.  g_fm, sum [nbags, width]: the gradient of out_fm and the forward's out_sum.  g_sum [nbags, width]: the gradient of
 * out_sum, or NULL when nothing consumed the sum.  Bags as ha_sgd_apply_bags: exactly one of bag >= 1 (fixed bags,
 * n == nbags * bag, b = i / bag in registers) and bag_of (int32[n] from ha_bag_of, bag == 0).
 * For every unique key k < rows with occurrences i0 < i1 < ..., let e = table[k,:] AS IT IS BEFORE THE CALL and acc = e; for
 * each occurrence in order, with b its bag and every operation rounded on its own:
 *   a   = fl(g_fm[b] * sum[b]);   with g_sum: a = fl(g_sum[b] + a)
 *   g   = fl(a - fl(g_fm[b] * e))
 *   acc = fl(acc - fl(lr * g))
 * then table[k,:] = acc.  Keys >= rows are ignored, rows that no id names are not touched.  Any width >= 1; width % 4 == 0
 * with every pointer 16-byte aligned takes 16-byte accesses.  None of g_sum, g_fm, sum may alias table.  n == 0 is not an
 * error.  Every argument check precedes any device access.
 * Equivalence: bit for bit E = ha_gather_*(table, ids), G = ha_fm_grad_rows(g_sum expanded to [n, width], E, sum, g_fm),
 * ha_sgd_apply(table, plan, G, lr) -- the project's fixed order of the three adjoints, unchanged.  That holds when the table
 * has not changed between the lookup that produced `sum` and this call (true of a table in HBM that only its own step
 * updates): e is the row now, not the row the lookup saw.
 * Tolerance mode 1 or 2 (ha_set_tolerance_mode): the entry points run exactly that composed sequence through the library's
 * per-stream scratch (rows and gradient, 2 * n * width floats) and are whatever ha_sgd_apply_finished is in that mode; the
 * fused kernel serves mode 0, the default, only.  plan_ws, bag_of and the three tensors must then be the caller's own
 * allocations, never pointers into that scratch (see ha_dedup_reduce_bags). */
int ha_sgd_apply_fm_bags(float *table, int64_t rows, int64_t width, void *plan_ws, int64_t n, const float *g_sum,
                         const float *g_fm, const float *sum, int64_t bag, const int32_t *bag_of, int64_t nbags, float lr,
                         ha_stream_t stream);
/* One call: plan (sort + finish) (+ ha_bag_of) + ha_sgd_apply_fm_bags, on an internal per-stream workspace.  bag / offsets
 * as ha_sgd_sparse_update_bags_* takes them: exactly one of bag >= 1 (n == nbags * bag) and offsets (int64[nbags + 1]). */
int ha_sgd_sparse_update_fm_bags_f32ids(float *table, int64_t rows, int64_t width, const float *ids, int64_t n, int64_t bag,
                                        const int64_t *offsets, int64_t nbags, const float *g_sum, const float *g_fm,
                                        const float *sum, float lr, ha_stream_t stream);
int ha_sgd_sparse_update_fm_bags_u64ids(float *table, int64_t rows, int64_t width, const uint64_t *ids, int64_t n, int64_t bag,
                                        const int64_t *offsets, int64_t nbags, const float *g_sum, const float *g_fm,
                                        const float *sum, float lr, ha_stream_t stream);
/* ---- weighted bags: the masked sum-pooled lookup of the FAE models (csrc/wbag.hip) ------------------------------------
 * examples/ctr/models/fae_wdl_criteo.py:19-31: embedding_lookup_op, mul_op by a per-occurrence 0/1 mask, reduce_sum_op(axes=1).
 * Bags -- fixed or ragged, exactly one of bag >= 1 and offsets / bag_of, offsets clamped -- are those of ha_gather_sum_* and
 * ha_sgd_apply_bags; weights is float32[n], one per occurrence, in the ids' order.
 * An occurrence is LIVE when its weight is not zero (+0.0f and -0.0f are zero, a NaN weight is not) and its id is below rows.
 * A dead occurrence takes no part in anything: its row is not added, its gradient is not applied, and whatever its row or its
 * bag's gradient holds (inf, NaN) does not reach a result.  This is the project's choice; the reference computes 0 * x, which
 * agrees for finite data except for the sign of a zero in one corner (see ha_sgd_apply_wbags).
 * Forward, per bag and column, in position order over the live occurrences:
 *   acc = +0;  acc = fl(acc + fl(w_j * r_j))      one multiply and one add per term, each rounded, nothing contracted
 * An empty bag or a bag with no live occurrence gives +0.  All weights 1.0f: ha_gather_sum_* bit for bit.  0/1 weights:
 * ha_gather_sum_* on the ragged bags left when the dead occurrences are deleted.  Any width >= 1; width % 4 == 0 with 16-byte
 * aligned table / out takes the 16-byte path.  Rules for every entry point of this section: exactly one of bag >= 1 and
 * offsets / bag_of, n % bag == 0 and n / bag == nbags, n < 2^31, 1 <= width < 2^30, nbags >= 1 when n > 0, null pointers refused
 * -- all checked before any device access; n == 0 returns 0 with null pointers allowed. */
int ha_gather_wsum_f32ids(const float *table, int64_t rows, int64_t width, const float *ids, const float *weights, int64_t n,
                          int64_t bag, const int64_t *offsets, int64_t nbags, float *out, ha_stream_t stream);
int ha_gather_wsum_u64ids(const float *table, int64_t rows, int64_t width, const uint64_t *ids, const float *weights, int64_t n,
                          int64_t bag, const int64_t *offsets, int64_t nbags, float *out, ha_stream_t stream);
/* The per-occurrence gradient, one elementwise launch: out[i,c] = fl(w_i * bag_grads[bag(i),c]), exactly +0.0f where w_i is
 * zero.  bag_grads [nbags, width], out [n, width]: an ordinary unpooled gradient, what every optimizer, push path and cache path
 * takes for weighted slices.  Fixed bags: bag >= 1, bag_of NULL; ragged: bag == 0 and bag_of = int32[n] from ha_bag_of. */
int ha_wbag_grad_rows(const float *bag_grads, const float *weights, int64_t n, int64_t width, int64_t bag,
                      const int32_t *bag_of, int64_t nbags, float *out, ha_stream_t stream);
/* The fused apply: for every key k < rows, over its LIVE occurrences i in ascending order,
 *   row = fl(row - fl(lr * fl(w_i * bag_grads[bag(i),:])))      three roundings per element
 * and the row of a key with no live occurrence keeps its bits; no [n, width] tensor exists.  plan_ws: a FINISHED plan
 * (ha_plan_build_*, or ha_plan_sort_* + ha_plan_finish) of the n ids, or of masked keys -- the row number of a live occurrence,
 * any key >= rows for a dead one; dead occurrences found inside a run are skipped, so every such plan gives the same table.
 * Bit for bit ha_wbag_grad_rows followed by ha_sgd_apply_finished whenever no table element is -0.0f: with lr < 0 that composed
 * sequence turns a -0.0f under a dead occurrence into +0.0f, this call keeps it.  Tolerance mode 1 or 2: the entry points run
 * exactly that composed sequence through the library's per-stream scratch (n * width floats), so long runs take the same tree
 * as everywhere else (plan_ws, bag_of, bag_grads and weights must then be the caller's own allocations, see
 * ha_dedup_reduce_bags).  bag_grads and weights must not alias the table. */
int ha_sgd_apply_wbags(float *table, int64_t rows, int64_t width, void *plan_ws, int64_t n, const float *bag_grads,
                       const float *weights, int64_t bag, const int32_t *bag_of, int64_t nbags, float lr, ha_stream_t stream);
/* One call on the internal per-stream workspace: one small launch writes masked uint64 keys (the row number of a live
 * occurrence, the key `rows` for a dead one), then ha_plan_sort_u64ids_lim + ha_plan_finish (+ ha_bag_of), then the apply.
 * The dead occurrences of FAE data -- thousands of padding ids per batch -- leave the plan as one out-of-range key that the
 * apply drops with one test instead of walking them as the batch's longest run.  Nothing is read back to the host.
 * rows <= 2^32 - 2.  Tolerance mode: the ids are planned as they are and the composed sequence runs (see above). */
int ha_sgd_sparse_update_wbags_f32ids(float *table, int64_t rows, int64_t width, const float *ids, const float *weights,
                                      int64_t n, const float *bag_grads, int64_t bag, const int64_t *offsets, int64_t nbags,
                                      float lr, ha_stream_t stream);
int ha_sgd_sparse_update_wbags_u64ids(float *table, int64_t rows, int64_t width, const uint64_t *ids, const float *weights,
                                      int64_t n, const float *bag_grads, int64_t bag, const int64_t *offsets, int64_t nbags,
                                      float lr, ha_stream_t stream);
/* ---- weighted bags on the row-sharded table: the end kernels of pull_wsum / push_wbags (csrc/wshard.hip) ----------------
 * The FAE models keep their cold table behind the parameter server (fae_wdl_criteo.py: ctx=ht.cpu(0)); herald_amd/sharded.py
 * serves it with the routing, exchanges and owner apply of pull / push and these two kernels at this rank's ends.
 * The weighted forward with the rows named by uint32 keys (device uint32[n]) into a buffer of rows: the contract of
 * ha_gather_wsum_f32ids to the letter -- weights float32[n] in position order, an occurrence is live when its weight is not zero
 * and its key is below rows, per bag and column over the live occurrences in position order acc = +0; acc = fl(acc + fl(w * r)),
 * nothing contracted, clamped offsets, the same slice rule.  All weights 1.0f: ha_gather_sum_u32keys bit for bit.  rows_buf is
 * the [u, width] buffer of the unique rows a batch received and keys its plan's inverse[n].  n > 0 requires rows >= 1 (the
 * kernel loads row 0 for a dead occurrence); checked, as everything else, before any device access. */
int ha_gather_wsum_u32keys(const float *rows_buf, int64_t rows, int64_t width, const uint32_t *keys, const float *weights,
                           int64_t n, int64_t bag, const int64_t *offsets, int64_t nbags, float *out, ha_stream_t stream);
/* The worker side of a PS sparse push of weighted pooled slices: for every unique key u of a FINISHED plan (ha_plan_build_*,
 * ha_plan_sort_* + ha_plan_finish; what ha_shard_route_pack_* builds), over its occurrences i0 < i1 < ... in ascending order,
 *   acc = +0;  acc = fl(acc + fl(scale * fl(w_i * bag_grads[bag(i),:])))      three roundings per element
 * An occurrence whose weight is zero takes no part and its bag's gradient row is not read; a key without live occurrence gets
 * a +0.0f row.  Keys are not tested against a row count.  reduced holds n rows, the first n_unique are written.  Exactly one of
 * bag >= 1 (fixed bags, bag_of NULL, n == nbags * bag) and bag_of (int32[n] from ha_bag_of, bag == 0), as ha_dedup_reduce_bags;
 * an entry of bag_of beyond nbags - 1 is clamped to it, as ha_wbag_grad_rows clamps it.  width % 4 == 0 with 16-byte aligned
 * bag_grads / reduced takes the 16-byte path, anything else the scalar one.  reduced must alias neither input.
 * Bit for bit, with no corner case, ha_wbag_grad_rows into an [n, width] tensor followed by ha_dedup_reduce_scaled: that
 * sequence gives a dead occurrence the term fl(scale * +0) = +-0, and a chain that starts at +0 never holds -0, so the term
 * changes no bit.  Tolerance mode 1 or 2: the entry point runs exactly that composed sequence through the library's per-stream
 * scratch (n * width floats); plan_ws, bag_of, bag_grads, weights and reduced must then be the caller's own allocations (see
 * ha_dedup_reduce_bags).  The plan's scratch words (header word 0, the radix scratch) are rewritten, as by ha_sgd_apply_wbags.
 * Every argument check precedes any device access; n == 0 returns 0. */
int ha_dedup_reduce_wbags(const void *plan_ws, int64_t n, const float *bag_grads, const float *weights, int64_t width,
                          int64_t bag, const int32_t *bag_of, int64_t nbags, float scale, float *reduced, ha_stream_t stream);
/* ---- weighted FM-pooled lookup: the second-order term of the FAE DeepFM (csrc/wfm.hip) ----------------------------------
 * examples/ctr/models/fae_deepfm_avazu.py:43-80: the cold rows are multiplied by the 0/1 mask and consumed as
 * reduce_sum_op(x, axes=1) and as reduce_sum_op(mul_op(x, x), axes=1); the square of the sum is taken only after the hot
 * table's half has been added, so S and Q leave as two [nbags, width] tensors.  Bags, weights, the LIVE occurrences and the
 * argument rules are those of the weighted bags above: live = weight not zero (a NaN weight is not zero) and an id that names
 * a row below `rows` ("Which ids name a row"); a dead occurrence takes no part in anything -- its row is not added, its
 * gradient is not applied, and whatever its row or its bag's gradients hold (inf, NaN) reaches no result.
 * Every fl() below is one float32 rounding (__fmul_rn, __fadd_rn, __fsub_rn); there is no FMA anywhere.
 * Forward, per bag b and column, over the live occurrences in position order, from S = +0 and Q = +0:
 *   x = fl(w_j * r_j);   S = fl(S + x);   Q = fl(Q + fl(x * x))
 * A bag without a live occurrence gives S = Q = +0.  out_sum is ha_gather_wsum_*'s output bit for bit for any weights; with all
 * weights 1.0f, out_sum and fl(0.5f * fl(fl(S*S) - Q)) are ha_gather_fm_*'s out_sum and out_fm bit for bit.  Both outputs are
 * required and must not overlap.  Any width >= 1; width % 4 == 0 with 16-byte aligned table / outputs takes the 16-byte path.
 * rows == 0 or n == 0: both outputs are zeroed. */
int ha_gather_wfm_f32ids(const float *table, int64_t rows, int64_t width, const float *ids, const float *weights, int64_t n,
                         int64_t bag, const int64_t *offsets, int64_t nbags, float *out_sum, float *out_sq, ha_stream_t stream);
int ha_gather_wfm_u64ids(const float *table, int64_t rows, int64_t width, const uint64_t *ids, const float *weights, int64_t n,
                         int64_t bag, const int64_t *offsets, int64_t nbags, float *out_sum, float *out_sq, ha_stream_t stream);
/* The per-occurrence gradient, one elementwise launch: an ordinary unpooled gradient [n, width].  With e = emb_rows[i,:] (row i
 * of a gathered row buffer), b the bag of i and w = weights[i]:
 *   x = fl(w * e);   t = fl(g_sq[b] * x);   a = fl(g_sum[b] + fl(t + t));   out[i] = fl(w * a)
 * and out[i] is exactly +0.0f where w is zero, whatever the operands hold.  The order is this project's fixed choice, as for
 * ha_fm_grad_rows: the reference's executor adds the two adjoints of mul_op(x, x) and the adjoint of the sum in an unspecified
 * topological order (fl(t) + fl(t) is fl(t + t) exactly, barring overflow).  g_sum, g_sq [nbags, width]: the gradients of
 * out_sum and out_sq.  Fixed bags: bag >= 1, bag_of NULL; ragged: bag == 0 and bag_of = int32[n] from ha_bag_of.  out may be
 * emb_rows itself (in place); it must not alias g_sum, g_sq or weights.  width % 4 == 0 with every pointer 16-byte aligned
 * takes 16-byte accesses. */
int ha_wfm_grad_rows(const float *g_sum, const float *g_sq, const float *weights, const float *emb_rows, int64_t n,
                     int64_t width, int64_t bag, const int32_t *bag_of, int64_t nbags, float *out, ha_stream_t stream);
/* The fused apply, two launches over a FINISHED plan (of the n ids, or of masked keys: any key >= rows for a dead occurrence).
 * For every key k < rows: e = table[k,:] AS IT IS BEFORE THE CALL and acc = e; over the key's LIVE occurrences in ascending
 * occurrence order g as above computed from this e, never from acc, then acc = fl(acc - fl(lr * g)); the row is written once.
 * A key without a live occurrence keeps its bits; dead occurrences inside a run are skipped, so every finished plan of the ids
 * gives the same table as a plan of masked keys.  No [n, width] tensor exists.  While the table has not changed since the
 * gather this is bit for bit ha_gather_*, ha_wfm_grad_rows, ha_sgd_apply_finished -- except the corner of ha_sgd_apply_wbags:
 * with lr < 0 a -0.0f element under a dead occurrence keeps its sign here and loses it in the composed sequence.
 * Tolerance mode 1 or 2: the entry points run exactly that composed sequence through the library's per-stream scratch (n *
 * width floats: the rows, then the gradient in place); plan_ws, bag_of, the gradients and weights must then be the caller's own
 * allocations (see ha_dedup_reduce_bags).  g_sum, g_sq and weights must not alias the table. */
int ha_sgd_apply_wfm_bags(float *table, int64_t rows, int64_t width, void *plan_ws, int64_t n, const float *g_sum,
                          const float *g_sq, const float *weights, int64_t bag, const int32_t *bag_of, int64_t nbags, float lr,
                          ha_stream_t stream);
/* One call on the internal per-stream workspace: masked keys (ha_sgd_sparse_update_wbags_*'s rule: the row number of a live
 * occurrence, the key `rows` for a dead one), ha_plan_sort_u64ids_lim with key_limit = rows, ha_plan_finish (+ ha_bag_of for
 * ragged bags), then the apply.  Nothing is read back to the host.  rows <= 2^32 - 2.  Tolerance mode: the ids are planned as
 * they are and the composed sequence runs (see above). */
int ha_sgd_sparse_update_wfm_bags_f32ids(float *table, int64_t rows, int64_t width, const float *ids, const float *weights,
                                         int64_t n, const float *g_sum, const float *g_sq, int64_t bag, const int64_t *offsets,
                                         int64_t nbags, float lr, ha_stream_t stream);
int ha_sgd_sparse_update_wfm_bags_u64ids(float *table, int64_t rows, int64_t width, const uint64_t *ids, const float *weights,
                                         int64_t n, const float *g_sum, const float *g_sq, int64_t bag, const int64_t *offsets,
                                         int64_t nbags, float lr, ha_stream_t stream);
/* Measurement aid (tools/bag_bench.py): column-slice width of ha_gather_sum_*'s 16-byte path, 64 / 128 / 256 floats per
 * wave; 0 = chosen from the batch (the default).  Process-wide; results do not depend on it. */
int ha_debug_bag_slice(int floats);

/* ---- in-node parameter-server engine behind the libps names (include/herald_ps.h) --------------------
 * ps-lite/src/python_binding.cc:6-151 -> Worker -> PSAgent (PSAgent.h:124-237) -> servers
 * (PSFHandle.h:101-164, 401-439).  Every process owns the AveragePartitioner row range of its rank
 * (partitioner.h:46-57) of every tensor, in its GPU's HBM.  Index / value DLArrays may be device or host
 * arrays.  Calls are asynchronous on the tensor's stream; ha_ps_wait joins it.  With nrank > 1 the sparse
 * exchange is provided by the host side as a backend (herald_amd/ps.py registers the RCCL all-to-all of
 * herald_amd/sharded.py); without one everything is served locally. */
typedef struct {
    /* ids_dev: float32 ids (global row numbers); out_dev / vals_dev: [n, width]; stream: the tensor's */
    int (*sparse_pull)(int node, const float *ids_dev, int64_t n, float *out_dev, void *stream);
    int (*sparse_push)(int node, const float *ids_dev, int64_t n, const float *vals_dev, void *stream);
    int (*barrier)(void);
} ha_ps_backend;
typedef struct {
    float *table;          /* this rank's rows [row_start, row_start + rows_local) */
    int64_t len, width, row_start, rows_local;
    void *stream;
} ha_ps_tensor_info;
int ha_ps_configure(int rank, int nrank);
int ha_ps_set_backend(const ha_ps_backend *backend);
int ha_ps_rank(void);
int ha_ps_nrank(void);
/* init_type: 0 Constant(a), 1 Uniform(a, b), 2 Normal(mean a, stddev b), 3 TruncatedNormal (psf/misc.h:7-12);
 * values are a function of (seed, element index) only: the same table whatever the number of ranks */
int ha_ps_init_tensor(int node, int ptype, int64_t len, int64_t width, int init_type,
                      double a, double b, uint64_t seed);
/* serve an existing device shard (rows of this rank's range) instead of allocating one */
int ha_ps_attach_tensor(int node, float *table_dev, int64_t len, int64_t width);
int ha_ps_tensor(int node, ha_ps_tensor_info *out);
int ha_ps_sparse_pull(int node, const DLArray *index, DLArray *value);
int ha_ps_sparse_push(int node, const DLArray *index, const DLArray *value);
int ha_ps_dense_pull(int node, DLArray *arr);
int ha_ps_wait(int node);
int ha_ps_barrier(void);
int ha_ps_clear(int node);
int ha_ps_save(int node, const char *address);   /* <address>/<node>_<rank>.dat, raw fp32 rows */
int ha_ps_load(int node, const char *address);

#ifdef __cplusplus
}
#endif
#endif /* HERALD_AMD_H_ */

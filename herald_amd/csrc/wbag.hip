// Weighted bags: the masked sum-pooled lookup of the reference's FAE models (examples/ctr/models/fae_wdl_criteo.py:19-31)
//     e = embedding_lookup_op(Embedding, cold_sparse_input);  e = mul_op(e, broadcast(cold_category_input));  reduce_sum_op(e, axes=1)
// and its backward, with a float32 weight per occurrence (in the reference's data a 0/1 mask: a hot id is served by a small
// dense table and its slot among the cold ids is the padding id 0 with weight 0).
//
// Live occurrences.  An occurrence is LIVE when its weight is not zero (+0.0f and -0.0f are both zero; a NaN weight is not)
// and its id is below `rows`.  A dead occurrence takes no part in anything: its row is not added, its gradient is not applied,
// and whatever its row or its bag's gradient holds (inf, NaN) does not reach a result.  This is the project's choice: the
// reference computes 0 * x.  For finite data the two agree, except for the sign of a zero in one corner: with lr < 0 the
// composed sequence below turns a -0.0f table element under a dead occurrence into +0.0f, the fused apply keeps it.
//
//   forward   per bag and column, in position order over the LIVE occurrences:  acc = +0;  acc = fl(acc + fl(w_j * r_j))
//             (one __fmul_rn and one __fadd_rn per term; no live occurrence: +0).  All weights 1.0f: ha_gather_sum_* bit for
//             bit; 0/1 weights: ha_gather_sum_* on the ragged bags left when the dead occurrences are deleted.
//   gradient  out[i,c] = fl(w_i * g[bag(i),c]), exactly +0.0f for a zero weight: an ordinary unpooled gradient [n, width].
//   apply     for every key k < rows, over its live occurrences i in ascending order:
//             row = fl(row - fl(lr * fl(w_i * g[bag(i),:])))   -- three roundings; a key without live occurrence keeps its bits.
//             Bit for bit the gradient above followed by ha_sgd_apply_finished whenever no table element is -0.0f.
//
// MI355X layout.  Forward: bag_sum_kernel's mapping (bagsum.hip) -- one wave per (bag, column slice), lane l holds id l and
// weight l of the current block of 64, v_readlane broadcasts both, ROWS branch-free loads in flight before the first add.  A
// dead occurrence loads row 0 (clamped address; in FAE data every dead slot names the same cached line) and the sum is
// discarded: the wave-uniform select costs nothing, compacting the live lanes was not built.  Apply: fmapply.hip's two
// launches over a FINISHED plan -- runs shorter than kPlanLongRun by one wave per (unique key, column chunk) with batched
// loads, longer ones by a workgroup per (listed key, 64-column slice) where waves 1 .. 15 leave fl(lr * fl(w * g)) and a
// live flag in LDS and wave 0 runs the chain, which is the final subtraction only.  Dead occurrences inside a run are
// skipped, so any finished plan of the ids gives the same table; the one-call form plans MASKED keys (a dead occurrence
// becomes the key `rows`), so the padding id's thousands of dead occurrences are one out-of-range key that the apply drops
// with one test instead of walking them as the batch's longest run.
#include "wbag_dev.h"

namespace ha {

int scratch_get(hipStream_t stream, size_t bytes, void **out);   // capi.hip
int tolerance_tree_from();                                       // scatter.hip

// ---- forward ---------------------------------------------------------------------------------------------------------------
// (wbag_sum_kernel, wbag_args_ok and wbag_sum_launch are in wbag_dev.h: wshard.hip instantiates them for uint32 keys)

// ---- per-occurrence gradient --------------------------------------------------------------------------------------------------
// out[i,c] = fl(w_i * g[bag(i),c]); +0.0f for a zero weight, whatever g holds.  A thread handles one vector of VEC floats.
template <int VEC>
__global__ __launch_bounds__(256) void wbag_grad_rows_kernel(const float *__restrict__ bag_grads,
                                                             const float *__restrict__ weights, uint64_t total_vec, uint32_t nv,
                                                             uint32_t bag, const int32_t *__restrict__ bag_of, uint32_t nbags,
                                                             float *__restrict__ out) {
    typedef typename WVec<VEC>::T V;
    const uint64_t e = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= total_vec)
        return;
    uint64_t i;
    if (total_vec <= 0xFFFFFFFFull)      // (uniform: the 32-bit division)
        i = static_cast<uint32_t>(e) / nv;
    else
        i = e / nv;
    const uint32_t cv = static_cast<uint32_t>(e - i * nv);
    uint32_t b;      // i < n < 2^31 (checked by the host)
    if (bag_of != nullptr)
        b = static_cast<uint32_t>(bag_of[i]);
    else
        b = static_cast<uint32_t>(i) / bag;
    b = b < nbags ? b : nbags - 1;       // (no row beyond bag_grads is read whatever bag_of holds)
    const float w = weights[i];
    const V g = *reinterpret_cast<const V *>(bag_grads + (static_cast<uint64_t>(b) * nv + cv) * VEC);
    V o;
#pragma unroll
    for (int k = 0; k < VEC; ++k)
        WVec<VEC>::set(o, k, w != 0.f ? __fmul_rn(w, WVec<VEC>::get(g, k)) : 0.f);
    *reinterpret_cast<V *>(out + e * VEC) = o;
}

// ---- apply ---------------------------------------------------------------------------------------------------------------------
// (the masked keys of the one-call form, wbag_mask_kernel, and wbag_bag are in wbag_dev.h: wfm.hip shares them)
// A run shorter than kPlanLongRun, by one wave: columns col .. col + VEC - 1 of every lane.  bg / wbits: lanes 0 .. len-1 hold
// the bags and the weights of the run's occurrences in occurrence order.
template <int VEC, int BATCH>
__device__ __forceinline__ void wbag_wave_run(float *__restrict__ row, int col, bool live, int bg, int wbits, int len,
                                              uint32_t width, const float *__restrict__ bag_grads, float lr) {
    typedef typename WVec<VEC>::T V;
    const int colc = live ? col : 0;      // lanes beyond the row load column 0 and store nothing
    V acc = *reinterpret_cast<const V *>(row + colc);
    for (int t0 = 0; t0 < len; t0 += BATCH) {
        const int cnt = min(BATCH, len - t0);
        V g[BATCH];
#pragma unroll
        for (int t = 0; t < BATCH; ++t) {
            if (t < cnt) {
                const uint64_t off = static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readlane(bg, t0 + t))) * width + colc;
                g[t] = *reinterpret_cast<const V *>(bag_grads + off);
            }
        }
#pragma unroll
        for (int t = 0; t < BATCH; ++t) {
            if (t < cnt) {
                const float w = __int_as_float(__builtin_amdgcn_readlane(wbits, t0 + t));      // wave-uniform
                if (w != 0.f) {
#pragma unroll
                    for (int k = 0; k < VEC; ++k)
                        WVec<VEC>::set(acc, k, __fsub_rn(WVec<VEC>::get(acc, k), __fmul_rn(lr, __fmul_rn(w, WVec<VEC>::get(g[t], k)))));
                }
            }
        }
    }
    if (live)      // (no live occurrence: the bits that were read)
        *reinterpret_cast<V *>(row + col) = acc;
}

// A long run, 64 columns, by the whole workgroup.  s_d: 2 * kWbagCoopRound * 64 floats, s_live: 2 * kWbagCoopRound flags.
template <bool FIXED>
__device__ __forceinline__ void wbag_coop_run(float *__restrict__ row, int col, bool live, const int32_t *__restrict__ perm, int s,
                                              int len, uint32_t width, const float *__restrict__ bag_grads,
                                              const float *__restrict__ weights, float lr, int bag,
                                              const int32_t *__restrict__ bag_of, float *s_d, int *s_live) {
    const int lane = lane_id(), w = static_cast<int>(threadIdx.x >> 6);
    const int colc = live ? col : 0;
    float acc = row[colc];
    int buf = 0;
    // waves 1 .. 15 form the values, kWbagCoopPerWave occurrences each per round; wave 0 only runs the chain.  The bags and
    // weights of a wave's occurrences are requested one round ahead, so a round waits for one memory round trip, not two.
    const int first = (w - 1) * kWbagCoopPerWave;
    int cnt_next = w == 0 ? 0 : max(0, min(kWbagCoopPerWave, len - first));      // (wave-uniform)
    int bg_next = 0;
    float wv_next = 0.f;
    if (cnt_next > 0) {
        const int i = perm[s + first + min(lane, cnt_next - 1)];
        bg_next = wbag_bag<FIXED>(i, bag, bag_of);
        wv_next = weights[i];
    }
    for (int r0 = 0; r0 < len; r0 += kWbagCoopRound) {
        const int cnt = cnt_next, bg = bg_next;
        const float wv = wv_next;
        const int t0n = r0 + kWbagCoopRound + first;
        cnt_next = w == 0 ? 0 : max(0, min(kWbagCoopPerWave, len - t0n));
        if (cnt_next > 0) {
            const int i = perm[s + t0n + min(lane, cnt_next - 1)];
            bg_next = wbag_bag<FIXED>(i, bag, bag_of);
            wv_next = weights[i];
        }
        if (cnt > 0) {      // (first >= 0 here: wave 0 has cnt == 0)
            float *dst = s_d + (buf * kWbagCoopRound + first) * kWave + lane;
            const int wbits = __float_as_int(wv);
            float g[kWbagCoopPerWave];
#pragma unroll
            for (int t = 0; t < kWbagCoopPerWave; ++t) {
                if (t < cnt) {
                    const uint64_t off = static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readlane(bg, t))) * width + colc;
                    g[t] = bag_grads[off];
                }
            }
#pragma unroll
            for (int t = 0; t < kWbagCoopPerWave; ++t)
                if (t < cnt)
                    dst[t * kWave] = __fmul_rn(lr, __fmul_rn(__int_as_float(__builtin_amdgcn_readlane(wbits, t)), g[t]));
            if (lane < cnt)
                s_live[buf * kWbagCoopRound + first + lane] = wv != 0.f ? 1 : 0;
        }
        __syncthreads();
        if (w == 0) {
            const int m = min(kWbagCoopRound, len - r0);
            const float *src = s_d + buf * kWbagCoopRound * kWave + lane;
            const int *lv = s_live + buf * kWbagCoopRound;
            int t = 0;
            for (; t + 8 <= m; t += 8) {
                float d[8];
                int f[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    d[q] = src[(t + q) * kWave];
                    f[q] = lv[t + q];
                }
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const float x = __fsub_rn(acc, d[q]);
                    acc = f[q] ? x : acc;
                }
            }
            for (; t < m; ++t) {
                const float x = __fsub_rn(acc, src[t * kWave]);
                acc = lv[t] ? x : acc;
            }
        }
        buf ^= 1;
    }
    if (w == 0 && live)
        row[col] = acc;
    __syncthreads();      // the buffers are free for the next listed item
}

// One wave per (unique key, chunk of 64 * VEC columns); the grid is sized by n, the waves beyond n_unique * nchunk leave at
// once.  Applies the runs shorter than kPlanLongRun and lists the keys of the longer ones (plan header word 0 / long_list, the
// scratch fmapply.hip and the by-unique applies of scatter.hip use for the same list) ...
template <int VEC, bool FIXED>
__global__ __launch_bounds__(kWbagWaves *kWave) void wbag_apply_short_kernel(
    float *__restrict__ table, uint64_t rows, uint32_t width, PlanHeader *__restrict__ hdr, const uint32_t *__restrict__ uniq,
    const int32_t *__restrict__ seg, const int32_t *__restrict__ counts, const int32_t *__restrict__ perm,
    const float *__restrict__ bag_grads, const float *__restrict__ weights, float lr, int bag,
    const int32_t *__restrict__ bag_of, uint32_t nchunk, uint32_t *__restrict__ long_list) {
    const int lane = lane_id();
    const uint64_t it = static_cast<uint64_t>(blockIdx.x) * kWbagWaves + (threadIdx.x >> 6);
    if (it >= static_cast<uint64_t>(hdr->n_unique) * nchunk)
        return;
    uint32_t u, c;
    if (nchunk == 1) {
        u = static_cast<uint32_t>(it);
        c = 0;
    } else {
        u = static_cast<uint32_t>(it / nchunk);
        c = static_cast<uint32_t>(it - static_cast<uint64_t>(u) * nchunk);
    }
    u = uniform(u);
    c = uniform(c);
    const int len = uniform(counts[u]);
    const uint32_t key = uniform(uniq[u]);
    if (key >= rows)
        return;      // out-of-range id, or the dead occurrences of a masked plan: ignored with this one test
    if (len >= kPlanLongRun) {
        if (c == 0 && lane == 0)
            long_list[atomicAdd(reinterpret_cast<unsigned long long *>(&hdr->reserved[0]), 1ull)] = u;
        return;
    }
    constexpr int kBatch = VEC == 4 ? 8 : 16;
    const int s = uniform(seg[u]);
    const int i = perm[s + min(lane, len - 1)];      // s + len <= n
    const int bg = wbag_bag<FIXED>(i, bag, bag_of);
    const int wbits = __float_as_int(weights[i]);
    const uint32_t col = (c * kWave + lane) * VEC;
    wbag_wave_run<VEC, kBatch>(table + static_cast<uint64_t>(key) * width, static_cast<int>(col), col < width, bg, wbits, len,
                               width, bag_grads, lr);
}

// ... and serves them here: work item = (listed key, 64-column slice), one per workgroup at a time (wbag_coop_run).
template <bool FIXED>
__global__ __launch_bounds__(kWbagLongWaves *kWave) void wbag_apply_long_kernel(
    float *__restrict__ table, uint32_t width, const PlanHeader *__restrict__ hdr, const uint32_t *__restrict__ uniq,
    const int32_t *__restrict__ seg, const int32_t *__restrict__ counts, const int32_t *__restrict__ perm,
    const float *__restrict__ bag_grads, const float *__restrict__ weights, float lr, int bag,
    const int32_t *__restrict__ bag_of, uint32_t nslice, const uint32_t *__restrict__ long_list) {
    __shared__ __attribute__((aligned(16))) float s_d[2 * kWbagCoopRound * kWave];
    __shared__ int s_live[2 * kWbagCoopRound];
    const int lane = lane_id();
    const uint64_t items = static_cast<uint64_t>(hdr->reserved[0]) * nslice;
    for (uint64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const uint32_t u = uniform(long_list[it / nslice]);
        const uint32_t col = static_cast<uint32_t>(it % nslice) * kWave + lane;
        wbag_coop_run<FIXED>(table + static_cast<uint64_t>(uniform(uniq[u])) * width, static_cast<int>(col), col < width, perm,
                             uniform(seg[u]), uniform(counts[u]), width, bag_grads, weights, lr, bag, bag_of, s_d, s_live);
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
static int wbag_grad_rows_launch(const char *what, const float *bag_grads, const float *weights, int64_t n, int64_t width,
                                 int64_t bag, const int32_t *bag_of, int64_t nbags, float *out, hipStream_t stream) {
    if (wbag_args_ok(what, 0, width, n, bag, bag_of != nullptr, nbags))
        return -1;
    if (n == 0)
        return 0;
    HA_REQUIRE(nbags >= 1, "%s: %ld occurrences in no bag", what, (long)n);
    HA_REQUIRE(bag_grads && weights && out, "%s: null pointer", what);
    HA_REQUIRE(out != bag_grads && out != weights, "%s: out must not alias bag_grads or weights", what);
    const bool vec_ok = (width % 4 == 0) &&
                        ((reinterpret_cast<uintptr_t>(bag_grads) | reinterpret_cast<uintptr_t>(out)) % 16 == 0);
    const int vec = vec_ok ? 4 : 1;
    const uint64_t total_vec = static_cast<uint64_t>(n) * static_cast<uint64_t>(width / vec);
    const uint64_t blocks64 = (total_vec + 255) / 256;
    HA_REQUIRE(blocks64 < (1ull << 31), "%s: batch too large", what);
    const dim3 grid(static_cast<unsigned>(blocks64)), block(256);
    if (vec == 4)
        hipLaunchKernelGGL((wbag_grad_rows_kernel<4>), grid, block, 0, stream, bag_grads, weights, total_vec,
                           (uint32_t)(width / 4), (uint32_t)bag, bag_of, (uint32_t)nbags, out);
    else
        hipLaunchKernelGGL((wbag_grad_rows_kernel<1>), grid, block, 0, stream, bag_grads, weights, total_vec, (uint32_t)width,
                           (uint32_t)bag, bag_of, (uint32_t)nbags, out);
    HA_LAUNCH_CHECK();
    return 0;
}

// the two launches of the fused apply over a finished plan (mode 0); arguments already checked
static int wbag_apply_launch(const char *what, float *table, int64_t rows, int64_t width, void *plan_ws, int64_t n,
                             const float *bag_grads, const float *weights, int64_t bag, const int32_t *bag_of, float lr,
                             hipStream_t stream) {
    PlanPtrs p = plan_layout(plan_ws, n);
    const bool fixed = bag_of == nullptr;
    const bool vec_ok = (width % 4 == 0) &&
                        ((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(bag_grads)) % 16 == 0);
    const uint32_t nslice = static_cast<uint32_t>((width + kWave - 1) / kWave);
    const uint32_t nchunk = vec_ok ? (nslice + 3) / 4 : nslice;
    const uint64_t blocks64 = (static_cast<uint64_t>(n) * nchunk + kWbagWaves - 1) / kWbagWaves;      // n_unique <= n
    HA_REQUIRE(blocks64 < (1ull << 31), "%s: batch too large (n=%ld ids of width %ld)", what, (long)n, (long)width);
    const dim3 grid(static_cast<unsigned>(blocks64)), block(kWbagWaves * kWave);
    // the list of the long keys: counter in plan header word 0, entries in the plan's keys_alt (free once the plan is sorted)
    HA_CHECK_HIP(hipMemsetAsync(&p.hdr->reserved[0], 0, sizeof(int64_t), stream));
#define HA_WBAG_SHORT_CASE(V, F)                                                                                             \
    hipLaunchKernelGGL((wbag_apply_short_kernel<V, F>), grid, block, 0, stream, table, (uint64_t)rows, (uint32_t)width, p.hdr, \
                       p.uniq, p.seg, p.counts, p.perm, bag_grads, weights, lr, (int)bag, bag_of, nchunk, p.keys_alt)
#define HA_WBAG_LONG_CASE(F)                                                                                                 \
    hipLaunchKernelGGL((wbag_apply_long_kernel<F>), dim3(kWbagLongBlocks), dim3(kWbagLongWaves * kWave), 0, stream, table,   \
                       (uint32_t)width, p.hdr, p.uniq, p.seg, p.counts, p.perm, bag_grads, weights, lr, (int)bag, bag_of,    \
                       nslice, p.keys_alt)
    if (fixed) {
        if (vec_ok) HA_WBAG_SHORT_CASE(4, true); else HA_WBAG_SHORT_CASE(1, true);
        HA_WBAG_LONG_CASE(true);
    } else {
        if (vec_ok) HA_WBAG_SHORT_CASE(4, false); else HA_WBAG_SHORT_CASE(1, false);
        HA_WBAG_LONG_CASE(false);
    }
#undef HA_WBAG_LONG_CASE
#undef HA_WBAG_SHORT_CASE
    HA_LAUNCH_CHECK();
    return 0;
}

static int wbag_apply(const char *what, float *table, int64_t rows, int64_t width, void *plan_ws, int64_t n,
                      const float *bag_grads, const float *weights, int64_t bag, const int32_t *bag_of, int64_t nbags, float lr,
                      hipStream_t stream) {
    if (wbag_args_ok(what, rows, width, n, bag, bag_of != nullptr, nbags))
        return -1;
    if (n == 0)
        return 0;
    HA_REQUIRE(nbags >= 1, "%s: %ld ids in no bag", what, (long)n);
    HA_REQUIRE(table && plan_ws && bag_grads && weights, "%s: null pointer", what);
    HA_REQUIRE(bag_grads != table && weights != table, "%s: bag_grads and weights must not alias the table", what);
    if (tolerance_tree_from() > 0) {
        // the composed sequence itself, through the per-stream scratch: whatever ha_sgd_apply_finished is in this mode
        void *ws = nullptr;
        if (scratch_get(stream, static_cast<size_t>(n) * static_cast<size_t>(width) * sizeof(float), &ws))
            return -1;
        float *G = static_cast<float *>(ws);
        if (wbag_grad_rows_launch(what, bag_grads, weights, n, width, bag, bag_of, nbags, G, stream))
            return -1;
        return ha_sgd_apply_finished(table, rows, width, plan_ws, n, G, lr, reinterpret_cast<ha_stream_t>(stream));
    }
    return wbag_apply_launch(what, table, rows, width, plan_ws, n, bag_grads, weights, bag, bag_of, lr, stream);
}

// One call: masked keys + plan (sort + finish) (+ ha_bag_of) + the apply, on the per-stream scratch; nothing is read back to
// the host.  In tolerance mode the composed sequence: the plan of the ids as they are, the per-occurrence gradient in the
// scratch behind it, ha_sgd_apply_finished.
template <typename IdT>
static int sgd_sparse_update_wbags(const char *what, float *table, int64_t rows, int64_t width, const IdT *ids,
                                   const float *weights, int64_t n, const float *bag_grads, int64_t bag, const int64_t *offsets,
                                   int64_t nbags, float lr, ha_stream_t stream) {
    if (wbag_args_ok(what, rows, width, n, bag, offsets != nullptr, nbags))
        return -1;
    if (n == 0)
        return 0;
    HA_REQUIRE(nbags >= 1, "%s: %ld ids in no bag", what, (long)n);
    HA_REQUIRE(table && ids && weights && bag_grads, "%s: null pointer", what);
    HA_REQUIRE(bag_grads != table && weights != table, "%s: bag_grads and weights must not alias the table", what);
    HA_REQUIRE(static_cast<uint64_t>(rows) <= 0xFFFFFFFEull, "%s: rows=%ld is beyond the plan's 32-bit keys", what, (long)rows);
    hipStream_t s = as_stream(stream);
    const size_t plan_bytes = align_up(ha_plan_bytes(n), 256);
    const size_t map_bytes = align_up(offsets ? static_cast<size_t>(n) * 4 : 0, 256);
    const bool composed = tolerance_tree_from() > 0;
    const size_t tail_bytes = composed ? static_cast<size_t>(n) * static_cast<size_t>(width) * sizeof(float)
                                       : static_cast<size_t>(n) * sizeof(uint64_t);
    void *ws = nullptr;
    if (scratch_get(s, plan_bytes + map_bytes + tail_bytes, &ws))
        return -1;
    char *tail = static_cast<char *>(ws) + plan_bytes + map_bytes;
    int32_t *bag_of = nullptr;
    if (offsets) {
        bag_of = reinterpret_cast<int32_t *>(static_cast<char *>(ws) + plan_bytes);
        if (ha_bag_of(offsets, nbags, n, bag_of, stream))
            return -1;
    }
    if (composed) {
        if (sizeof(IdT) == 4 ? ha_plan_sort_f32ids(reinterpret_cast<const float *>(ids), n, ws, stream)
                             : ha_plan_sort_u64ids(reinterpret_cast<const uint64_t *>(ids), n, ws, stream))
            return -1;
        if (ha_plan_finish(ws, n, stream))
            return -1;
        float *G = reinterpret_cast<float *>(tail);
        if (wbag_grad_rows_launch(what, bag_grads, weights, n, width, offsets ? 0 : bag, bag_of, nbags, G, s))
            return -1;
        return ha_sgd_apply_finished(table, rows, width, ws, n, G, lr, stream);
    }
    uint64_t *keys = reinterpret_cast<uint64_t *>(tail);
    hipLaunchKernelGGL((wbag_mask_kernel<IdT>), dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, s, ids, weights, n,
                       (uint64_t)rows, (uint64_t)rows, keys);
    HA_LAUNCH_CHECK();
    if (ha_plan_sort_u64ids_lim(keys, n, ws, static_cast<uint64_t>(rows), stream))
        return -1;
    if (ha_plan_finish(ws, n, stream))
        return -1;
    return wbag_apply_launch(what, table, rows, width, ws, n, bag_grads, weights, offsets ? 0 : bag, bag_of, lr, s);
}

}  // namespace ha

extern "C" int ha_gather_wsum_f32ids(const float *table, int64_t rows, int64_t width, const float *ids, const float *weights,
                                     int64_t n, int64_t bag, const int64_t *offsets, int64_t nbags, float *out,
                                     ha_stream_t stream) {
    return ha::wbag_sum_launch<float>("ha_gather_wsum_f32ids", table, rows, width, ids, weights, n, bag, offsets, nbags, out,
                                      ha::as_stream(stream));
}

extern "C" int ha_gather_wsum_u64ids(const float *table, int64_t rows, int64_t width, const uint64_t *ids, const float *weights,
                                     int64_t n, int64_t bag, const int64_t *offsets, int64_t nbags, float *out,
                                     ha_stream_t stream) {
    return ha::wbag_sum_launch<uint64_t>("ha_gather_wsum_u64ids", table, rows, width, ids, weights, n, bag, offsets, nbags, out,
                                         ha::as_stream(stream));
}

extern "C" int ha_wbag_grad_rows(const float *bag_grads, const float *weights, int64_t n, int64_t width, int64_t bag,
                                 const int32_t *bag_of, int64_t nbags, float *out, ha_stream_t stream) {
    return ha::wbag_grad_rows_launch("ha_wbag_grad_rows", bag_grads, weights, n, width, bag, bag_of, nbags, out,
                                     ha::as_stream(stream));
}

extern "C" int ha_sgd_apply_wbags(float *table, int64_t rows, int64_t width, void *plan_ws, int64_t n, const float *bag_grads,
                                  const float *weights, int64_t bag, const int32_t *bag_of, int64_t nbags, float lr,
                                  ha_stream_t stream) {
    return ha::wbag_apply("ha_sgd_apply_wbags", table, rows, width, plan_ws, n, bag_grads, weights, bag, bag_of, nbags, lr,
                          ha::as_stream(stream));
}

extern "C" int ha_sgd_sparse_update_wbags_f32ids(float *table, int64_t rows, int64_t width, const float *ids,
                                                 const float *weights, int64_t n, const float *bag_grads, int64_t bag,
                                                 const int64_t *offsets, int64_t nbags, float lr, ha_stream_t stream) {
    return ha::sgd_sparse_update_wbags<float>("ha_sgd_sparse_update_wbags_f32ids", table, rows, width, ids, weights, n,
                                              bag_grads, bag, offsets, nbags, lr, stream);
}

extern "C" int ha_sgd_sparse_update_wbags_u64ids(float *table, int64_t rows, int64_t width, const uint64_t *ids,
                                                 const float *weights, int64_t n, const float *bag_grads, int64_t bag,
                                                 const int64_t *offsets, int64_t nbags, float lr, ha_stream_t stream) {
    return ha::sgd_sparse_update_wbags<uint64_t>("ha_sgd_sparse_update_wbags_u64ids", table, rows, width, ids, weights, n,
                                                 bag_grads, bag, offsets, nbags, lr, stream);
}

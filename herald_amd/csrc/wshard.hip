// Weighted bags on the row-sharded table: the two end kernels of ShardedEmbedding.pull_wsum / push_wbags (herald_amd/sharded.py).
// The reference's FAE models keep the cold table behind the parameter server (examples/ctr/models/fae_wdl_criteo.py:19-31 with
// ctx=ht.cpu(0)): embedding_lookup_op, mul_op by a 0/1 mask, reduce_sum_op(axes=1).  What crosses the fabric is what pull / push
// send -- one row per unique key, both ways --, only this rank's two end kernels differ:
//
//   pull   ha_gather_wsum_u32keys: wbag.hip's forward (wbag_sum_kernel, wbag_dev.h) in its uint32 instantiation, over the buffer of
//          the unique rows a batch received, keys = the plan's inverse.  No [n, width] rows.
//   push   ha_dedup_reduce_wbags: for every unique key u of a FINISHED plan, over its occurrences i in ascending order,
//              acc = +0;  acc = fl(acc + fl(scale * fl(w_i * bag_grads[bag(i),:])))      an occurrence with w_i == 0 takes no part
//          Bit for bit ha_wbag_grad_rows into [n, width] followed by ha_dedup_reduce_scaled: there a dead occurrence adds
//          fl(scale * +0) = +-0 to a chain that started at +0 and therefore never holds -0, which changes no bit.
//
// MI355X layout of the reduce: wbag.hip's apply with the accumulator starting at +0 and reduced[u] as the destination.  Runs
// shorter than kPlanLongRun: one wave per (unique key, chunk of 64 * VEC columns); lanes 0 .. len-1 hold bag and weight of the
// run's occurrences, the live ones are walked by the bits of one ballot (scalar), so a dead occurrence costs neither a load nor
// a chain step.  Longer runs are listed and served by 16-wave workgroups per (listed key, 64-column slice).  In FAE data every
// dead slot names the padding id, so key 0 owns a run of thousands of occurrences, none of them live: before its rounds the
// workgroup scans the run's weights (every wave its share of 64-occurrence blocks, four blocks in flight) for the first and the
// last live occurrence.  No live occurrence: +0 is written and the item is done; otherwise wbag_coop_run's rounds cover first ..
// last only, the producer waves request no gradient row for a dead occurrence and wave 0 steps over a round without a live flag.
#include "wbag_dev.h"

namespace ha {

int scratch_get(hipStream_t stream, size_t bytes, void **out);   // capi.hip
int tolerance_tree_from();                                       // scatter.hip

// the bag of occurrence i, clamped as wbag_grad_rows_kernel clamps it: no row beyond bag_grads is read whatever bag_of holds
template <bool FIXED>
__device__ __forceinline__ int wshard_bag(int i, int bag, const int32_t *__restrict__ bag_of, uint32_t nbags) {
    const uint32_t b = static_cast<uint32_t>(wbag_bag<FIXED>(i, bag, bag_of));
    return static_cast<int>(b < nbags ? b : nbags - 1);
}

__device__ __forceinline__ bool wshard_live_bits(int wbits) { return (wbits & 0x7FFFFFFF) != 0; }      // w != 0.f (NaN: live)

// One wave per (unique key, chunk of 64 * VEC columns); the grid is sized by n, the waves beyond n_unique * nchunk leave at
// once.  Reduces the runs shorter than kPlanLongRun and lists the keys of the longer ones (plan header word 0 / long_list, as
// wbag_apply_short_kernel).
template <int VEC, bool FIXED>
__global__ __launch_bounds__(kWbagWaves *kWave) void wshard_reduce_short_kernel(
    float *__restrict__ reduced, uint32_t width, PlanHeader *__restrict__ hdr, const int32_t *__restrict__ seg,
    const int32_t *__restrict__ counts, const int32_t *__restrict__ perm, const float *__restrict__ bag_grads,
    const float *__restrict__ weights, float scale, int bag, const int32_t *__restrict__ bag_of, uint32_t nbags, uint32_t nchunk,
    uint32_t *__restrict__ long_list) {
    typedef typename WVec<VEC>::T V;
    constexpr int kBatch = VEC == 4 ? 8 : 16;
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
    if (len >= kPlanLongRun) {
        if (c == 0 && lane == 0)
            long_list[atomicAdd(reinterpret_cast<unsigned long long *>(&hdr->reserved[0]), 1ull)] = u;
        return;
    }
    const int s = uniform(seg[u]);
    const int i = perm[s + min(lane, len - 1)];      // s + len <= n
    const int bg = wshard_bag<FIXED>(i, bag, bag_of, nbags);
    const int wbits = __float_as_int(weights[i]);
    const uint32_t col = (c * kWave + lane) * VEC;
    const bool colok = col < width;      // (VEC > 1: width % VEC == 0)
    const uint32_t colc = colok ? col : 0;
    unsigned long long m = __ballot(lane < len && wshard_live_bits(wbits));      // the live occurrences, in occurrence order
    V acc;
#pragma unroll
    for (int k = 0; k < VEC; ++k)
        WVec<VEC>::set(acc, k, 0.f);
    while (m != 0ull) {
        int tt[kBatch];      // lanes of the next (up to) kBatch live occurrences: wave-uniform
        const int cnt = min(kBatch, static_cast<int>(__builtin_popcountll(m)));
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
            tt[k] = m != 0ull ? static_cast<int>(__builtin_ctzll(m)) : 0;
            m &= m - 1ull;      // (0 stays 0)
        }
        V g[kBatch];
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
            if (k < cnt) {
                const uint64_t off = static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readlane(bg, tt[k]))) * width + colc;
                g[k] = *reinterpret_cast<const V *>(bag_grads + off);
            }
        }
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
            if (k < cnt) {
                const float w = __int_as_float(__builtin_amdgcn_readlane(wbits, tt[k]));
#pragma unroll
                for (int q = 0; q < VEC; ++q)
                    WVec<VEC>::set(acc, q, __fadd_rn(WVec<VEC>::get(acc, q), __fmul_rn(scale, __fmul_rn(w, WVec<VEC>::get(g[k], q)))));
            }
        }
    }
    if (colok)      // (no live occurrence: +0)
        *reinterpret_cast<V *>(reduced + static_cast<uint64_t>(u) * width + col) = acc;
}

// First and last live occurrence of a run (positions 0 .. len-1 behind sorted position s), by the whole workgroup: wave w takes
// the 64-occurrence blocks w, w + 16, ..., four of them per trip with all their loads in flight.  s_range: {first, -(last)}
// kept as two minima; returns through first / last (first > last: no live occurrence).
__device__ __forceinline__ void wshard_live_range(const int32_t *__restrict__ perm, int s, int len,
                                                  const float *__restrict__ weights, int *s_range, int &first, int &last) {
    constexpr int kTrip = 4;
    const int lane = lane_id(), w = static_cast<int>(threadIdx.x >> 6);
    if (threadIdx.x == 0) {
        s_range[0] = 0x7FFFFFFF;
        s_range[1] = -1;
    }
    __syncthreads();
    int lo = 0x7FFFFFFF, hi = -1;
    for (int base = w * kWave; base < len; base += kTrip * kWbagLongWaves * kWave) {
        int idx[kTrip];
        float wv[kTrip];
#pragma unroll
        for (int q = 0; q < kTrip; ++q)
            idx[q] = perm[s + min(base + q * kWbagLongWaves * kWave + lane, len - 1)];
#pragma unroll
        for (int q = 0; q < kTrip; ++q)
            wv[q] = weights[idx[q]];
#pragma unroll
        for (int q = 0; q < kTrip; ++q) {
            const int t = base + q * kWbagLongWaves * kWave + lane;
            if (t < len && wv[q] != 0.f) {
                lo = min(lo, t);
                hi = max(hi, t);
            }
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o, 64));
        hi = max(hi, __shfl_xor(hi, o, 64));
    }
    if (lane == 0 && hi >= 0) {
        atomicMin(&s_range[0], lo);
        atomicMax(&s_range[1], hi);
    }
    __syncthreads();
    first = s_range[0];
    last = s_range[1];
}

// A long run, 64 columns, by the whole workgroup: wbag_coop_run with the accumulator starting at +0.  s_d: 2 * kWbagCoopRound
// * 64 floats, s_live: 2 * kWbagCoopRound flags.  Returns the sum in wave 0's lanes.
template <bool FIXED>
__device__ __forceinline__ float wshard_coop_run(int colc, const int32_t *__restrict__ perm, int s, int len, uint32_t width,
                                                 const float *__restrict__ bag_grads, const float *__restrict__ weights,
                                                 float scale, int bag, const int32_t *__restrict__ bag_of, uint32_t nbags,
                                                 float *s_d, int *s_live) {
    const int lane = lane_id(), w = static_cast<int>(threadIdx.x >> 6);
    float acc = 0.f;
    int buf = 0;
    // waves 1 .. 15 form the values, kWbagCoopPerWave occurrences each per round; wave 0 only runs the chain.  The bags and
    // weights of a wave's occurrences are requested one round ahead.
    const int first = (w - 1) * kWbagCoopPerWave;
    int cnt_next = w == 0 ? 0 : max(0, min(kWbagCoopPerWave, len - first));      // (wave-uniform)
    int bg_next = 0;
    float wv_next = 0.f;
    if (cnt_next > 0) {
        const int i = perm[s + first + min(lane, cnt_next - 1)];
        bg_next = wshard_bag<FIXED>(i, bag, bag_of, nbags);
        wv_next = weights[i];
    }
    for (int r0 = 0; r0 < len; r0 += kWbagCoopRound) {
        const int cnt = cnt_next, bg = bg_next;
        const float wv = wv_next;
        const int t0n = r0 + kWbagCoopRound + first;
        cnt_next = w == 0 ? 0 : max(0, min(kWbagCoopPerWave, len - t0n));
        if (cnt_next > 0) {
            const int i = perm[s + t0n + min(lane, cnt_next - 1)];
            bg_next = wshard_bag<FIXED>(i, bag, bag_of, nbags);
            wv_next = weights[i];
        }
        if (cnt > 0) {      // (first >= 0 here: wave 0 has cnt == 0)
            float *dst = s_d + (buf * kWbagCoopRound + first) * kWave + lane;
            const int wbits = __float_as_int(wv);
            float g[kWbagCoopPerWave];
#pragma unroll
            for (int t = 0; t < kWbagCoopPerWave; ++t) {
                g[t] = 0.f;
                // (wave-uniform) the gradient row of a dead occurrence is not read
                if (t < cnt && wshard_live_bits(__builtin_amdgcn_readlane(wbits, t))) {
                    const uint64_t off = static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readlane(bg, t))) * width + colc;
                    g[t] = bag_grads[off];
                }
            }
#pragma unroll
            for (int t = 0; t < kWbagCoopPerWave; ++t)
                if (t < cnt)
                    dst[t * kWave] = __fmul_rn(scale, __fmul_rn(__int_as_float(__builtin_amdgcn_readlane(wbits, t)), g[t]));
            if (lane < cnt)
                s_live[buf * kWbagCoopRound + first + lane] = wv != 0.f ? 1 : 0;
        }
        __syncthreads();
        if (w == 0) {
            const int m = min(kWbagCoopRound, len - r0);
            const float *src = s_d + buf * kWbagCoopRound * kWave + lane;
            const int *lv = s_live + buf * kWbagCoopRound;
            // a round without a live flag is stepped over (kWbagCoopRound <= 2 * kWave)
            const bool any = __ballot(lv[min(lane, m - 1)] != 0 || lv[min(lane + kWave, m - 1)] != 0) != 0ull;
            int t = 0;
            for (; any && t + 8 <= m; t += 8) {
                float d[8];
                int f[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    d[q] = src[(t + q) * kWave];
                    f[q] = lv[t + q];
                }
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const float x = __fadd_rn(acc, d[q]);
                    acc = f[q] ? x : acc;
                }
            }
            for (; any && t < m; ++t) {
                const float x = __fadd_rn(acc, src[t * kWave]);
                acc = lv[t] ? x : acc;
            }
        }
        buf ^= 1;
    }
    return acc;
}

// ... and serves the listed keys here: work item = (listed key, 64-column slice), one per workgroup at a time.
template <bool FIXED>
__global__ __launch_bounds__(kWbagLongWaves *kWave) void wshard_reduce_long_kernel(
    float *__restrict__ reduced, uint32_t width, const PlanHeader *__restrict__ hdr, const int32_t *__restrict__ seg,
    const int32_t *__restrict__ counts, const int32_t *__restrict__ perm, const float *__restrict__ bag_grads,
    const float *__restrict__ weights, float scale, int bag, const int32_t *__restrict__ bag_of, uint32_t nbags, uint32_t nslice,
    const uint32_t *__restrict__ long_list) {
    static_assert(kWbagCoopRound <= 2 * kWave, "wave 0 reads a round's live flags with two loads per lane");
    __shared__ __attribute__((aligned(16))) float s_d[2 * kWbagCoopRound * kWave];
    __shared__ int s_live[2 * kWbagCoopRound];
    __shared__ int s_range[2];
    const int lane = lane_id();
    const uint64_t items = static_cast<uint64_t>(hdr->reserved[0]) * nslice;
    for (uint64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const uint32_t u = uniform(long_list[it / nslice]);
        const uint32_t col = static_cast<uint32_t>(it % nslice) * kWave + lane;
        const bool colok = col < width;
        const int s = uniform(seg[u]), len = uniform(counts[u]);
        int first, last;
        wshard_live_range(perm, s, len, weights, s_range, first, last);      // (wave-uniform: read from LDS behind a barrier)
        first = uniform(first);
        last = uniform(last);
        float acc = 0.f;
        if (first <= last)
            acc = wshard_coop_run<FIXED>(static_cast<int>(colok ? col : 0), perm, s + first, last - first + 1, width, bag_grads,
                                         weights, scale, bag, bag_of, nbags, s_d, s_live);
        if (threadIdx.x < kWave && colok)
            reduced[static_cast<uint64_t>(u) * width + col] = acc;
        __syncthreads();      // the buffers and s_range are free for the next listed item
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
static int wshard_reduce_launch(const char *what, void *plan_ws, int64_t n, const float *bag_grads, const float *weights,
                                int64_t width, int64_t bag, const int32_t *bag_of, int64_t nbags, float scale, float *reduced,
                                hipStream_t stream) {
    PlanPtrs p = plan_layout(plan_ws, n);
    const bool fixed = bag_of == nullptr;
    const bool vec_ok = (width % 4 == 0) &&
                        ((reinterpret_cast<uintptr_t>(reduced) | reinterpret_cast<uintptr_t>(bag_grads)) % 16 == 0);
    const uint32_t nslice = static_cast<uint32_t>((width + kWave - 1) / kWave);
    const uint32_t nchunk = vec_ok ? (nslice + 3) / 4 : nslice;
    const uint64_t blocks64 = (static_cast<uint64_t>(n) * nchunk + kWbagWaves - 1) / kWbagWaves;      // n_unique <= n
    HA_REQUIRE(blocks64 < (1ull << 31), "%s: batch too large (n=%ld ids of width %ld)", what, (long)n, (long)width);
    const dim3 grid(static_cast<unsigned>(blocks64)), block(kWbagWaves * kWave);
    // the list of the long keys: counter in plan header word 0, entries in the plan's keys_alt (as wbag.hip's apply)
    HA_CHECK_HIP(hipMemsetAsync(&p.hdr->reserved[0], 0, sizeof(int64_t), stream));
#define HA_WSHARD_SHORT_CASE(V, F)                                                                                             \
    hipLaunchKernelGGL((wshard_reduce_short_kernel<V, F>), grid, block, 0, stream, reduced, (uint32_t)width, p.hdr, p.seg,      \
                       p.counts, p.perm, bag_grads, weights, scale, (int)bag, bag_of, (uint32_t)nbags, nchunk, p.keys_alt)
#define HA_WSHARD_LONG_CASE(F)                                                                                                 \
    hipLaunchKernelGGL((wshard_reduce_long_kernel<F>), dim3(kWbagLongBlocks), dim3(kWbagLongWaves * kWave), 0, stream, reduced, \
                       (uint32_t)width, p.hdr, p.seg, p.counts, p.perm, bag_grads, weights, scale, (int)bag, bag_of,           \
                       (uint32_t)nbags, nslice, p.keys_alt)
    if (fixed) {
        if (vec_ok) HA_WSHARD_SHORT_CASE(4, true); else HA_WSHARD_SHORT_CASE(1, true);
        HA_WSHARD_LONG_CASE(true);
    } else {
        if (vec_ok) HA_WSHARD_SHORT_CASE(4, false); else HA_WSHARD_SHORT_CASE(1, false);
        HA_WSHARD_LONG_CASE(false);
    }
#undef HA_WSHARD_LONG_CASE
#undef HA_WSHARD_SHORT_CASE
    HA_LAUNCH_CHECK();
    return 0;
}

}  // namespace ha

extern "C" int ha_gather_wsum_u32keys(const float *rows_buf, int64_t rows, int64_t width, const uint32_t *keys,
                                      const float *weights, int64_t n, int64_t bag, const int64_t *offsets, int64_t nbags,
                                      float *out, ha_stream_t stream) {
    // (the kernel loads row 0 for a dead occurrence)
    HA_REQUIRE(n <= 0 || rows >= 1, "ha_gather_wsum_u32keys: %ld keys into a buffer of rows=%ld rows", (long)n, (long)rows);
    return ha::wbag_sum_launch<uint32_t>("ha_gather_wsum_u32keys", rows_buf, rows, width, keys, weights, n, bag, offsets, nbags,
                                         out, ha::as_stream(stream));
}

extern "C" int ha_dedup_reduce_wbags(const void *plan_ws, int64_t n, const float *bag_grads, const float *weights, int64_t width,
                                     int64_t bag, const int32_t *bag_of, int64_t nbags, float scale, float *reduced,
                                     ha_stream_t stream) {
    using namespace ha;
    const char *what = "ha_dedup_reduce_wbags";
    if (wbag_args_ok(what, 0, width, n, bag, bag_of != nullptr, nbags))
        return -1;
    if (n == 0)
        return 0;
    HA_REQUIRE(nbags >= 1, "%s: %ld occurrences in no bag", what, (long)n);
    HA_REQUIRE(plan_ws && bag_grads && weights && reduced, "%s: null pointer", what);
    HA_REQUIRE(reduced != bag_grads && reduced != weights, "%s: reduced must not alias bag_grads or weights", what);
    hipStream_t s = as_stream(stream);
    if (tolerance_tree_from() > 0) {
        // the composed sequence itself, through the per-stream scratch: whatever ha_dedup_reduce_scaled is in this mode
        void *ws = nullptr;
        if (scratch_get(s, static_cast<size_t>(n) * static_cast<size_t>(width) * sizeof(float), &ws))
            return -1;
        float *G = static_cast<float *>(ws);
        if (ha_wbag_grad_rows(bag_grads, weights, n, width, bag, bag_of, nbags, G, stream))
            return -1;
        return ha_dedup_reduce_scaled(plan_ws, n, G, width, scale, reduced, stream);
    }
    return wshard_reduce_launch(what, const_cast<void *>(plan_ws), n, bag_grads, weights, width, bag, bag_of, nbags, scale,
                                reduced, s);
}

// Backward of the FM-pooled lookup when nothing consumes the rows (the pooled DeepFM: emb_sum_deepfm_avazu.py), fused into
// the sparse SGD apply: ha_sgd_apply_fm_bags and its one-call forms.
//
// The gradient of occurrence i of key k in bag b is  g_i = (g_S[b] + g_fm[b] * S[b]) - g_fm[b] * e_k  (ha_fm_grad_rows's
// fixed order of the adjoints), and e_k is the row the apply holds in registers anyway.  So one launch reads every unique
// row once, forms the g_i from three [nbags, width] tensors (L2 / Infinity-Cache resident) and writes the row once:
//     e = table[k,:] before the call;  acc = e
//     per occurrence, in occurrence order:   a = fl(g_fm*S);  a = fl(g_S + a) (with g_sum);  g = fl(a - fl(g_fm*e))
//                                            acc = fl(acc - fl(lr*g))
// bit for bit ha_gather_* + ha_fm_grad_rows + ha_sgd_apply with no [n, width] tensor anywhere.  Only the last line is an
// ordered chain; everything in front of it is independent per occurrence.
//
// Work mapping (a FINISHED plan: uniq / seg / counts / perm), two launches:
//   * fm_apply_short_kernel, one wave per (unique key, chunk of 64 or 256 columns): a run shorter than kFmLongRun is applied
//     by that wave alone, loads in batches (16 occurrences of 3 scalar loads, or 4 of 3 16-byte loads); an item has three
//     or four dependent memory round trips and nothing to overlap them with, so there are as many waves as items and the
//     hardware overlaps them (a first version looped 256 workgroups over the items and ran at the latency of its rounds).
//     The keys of longer runs go on a list.
//   * fm_apply_long_kernel, work item = (listed key, 64-column slice), a workgroup of 16 waves per item (a hot Criteo id
//     repeats hundreds of times per batch): 120 occurrences per round, waves 1 .. 15 each form fl(lr*g) of 8 occurrences for
//     the 64 columns and leave them in LDS, wave 0 runs the chain from LDS while the others already load the next round
//     (two buffers, one barrier per round).  The chain is one subtraction per occurrence and column, as narrow as
//     ha_sgd_apply's.
#include "plan_dev.h"

namespace ha {

int scratch_get(hipStream_t stream, size_t bytes, void **out);   // capi.hip
int tolerance_tree_from();                                       // scatter.hip

constexpr int kFmLongRun = 48;       // runs at least this long are served by the whole workgroup
constexpr int kFmWaves = 16;
constexpr int kFmCoopPerWave = 8;    // occurrences per wave and round of the cooperative path
constexpr int kFmCoopRound = (kFmWaves - 1) * kFmCoopPerWave;      // wave 0 runs the chain only
constexpr int kFmShortWaves = 4;     // waves per workgroup of the launch that applies the shorter runs
constexpr int kFmLongBlocks = 256;   // workgroups that loop over the (long key, slice) items: one per compute unit
static_assert(kFmLongRun == kPlanLongRun, "the list of long keys is the one the plan's finish and scatter.hip keep");

template <int VEC>
struct FmVec;
template <>
struct FmVec<1> {
    typedef float T;
    static __device__ __forceinline__ float get(const T &v, int) { return v; }
    static __device__ __forceinline__ void set(T &v, int, float x) { v = x; }
};
template <>
struct FmVec<4> {
    typedef float4v T;
    static __device__ __forceinline__ float get(const T &v, int k) { return v[k]; }
    static __device__ __forceinline__ void set(T &v, int k, float x) { v[k] = x; }
};

// the bag of occurrence i
template <bool FIXED>
__device__ __forceinline__ int fm_bag(int i, int bag, const int32_t *__restrict__ bag_of) {
    return FIXED ? i / bag : bag_of[i];
}

// g of one occurrence and column: the order of ha_fm_grad_rows
template <bool GS>
__device__ __forceinline__ float fm_g(float gs, float gf, float sm, float e) {
    float a = __fmul_rn(gf, sm);
    if (GS)
        a = __fadd_rn(gs, a);
    return __fsub_rn(a, __fmul_rn(gf, e));
}

// A run shorter than kFmLongRun, by one wave: columns col .. col + VEC - 1 of every lane.  bg: lanes 0 .. len-1 hold the
// bags of the run's occurrences in occurrence order.
template <int VEC, bool GS, int BATCH>
__device__ __forceinline__ void fm_wave_run(float *__restrict__ row, int col, bool live, int bg, int len, uint32_t width,
                                            const float *__restrict__ g_sum, const float *__restrict__ g_fm,
                                            const float *__restrict__ sum, float lr) {
    typedef typename FmVec<VEC>::T V;
    const int colc = live ? col : 0;      // lanes beyond the row load column 0 and store nothing
    const V e = *reinterpret_cast<const V *>(row + colc);
    V acc = e;
    for (int t0 = 0; t0 < len; t0 += BATCH) {
        const int cnt = min(BATCH, len - t0);
        V gf[BATCH], sm[BATCH], gs[BATCH];
#pragma unroll
        for (int t = 0; t < BATCH; ++t) {
            if (t < cnt) {
                const uint64_t off = static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readlane(bg, t0 + t))) * width + colc;
                gf[t] = *reinterpret_cast<const V *>(g_fm + off);
                sm[t] = *reinterpret_cast<const V *>(sum + off);
                if (GS)
                    gs[t] = *reinterpret_cast<const V *>(g_sum + off);
            }
        }
#pragma unroll
        for (int t = 0; t < BATCH; ++t) {
            if (t < cnt) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const float g = fm_g<GS>(GS ? FmVec<VEC>::get(gs[t], k) : 0.f, FmVec<VEC>::get(gf[t], k),
                                             FmVec<VEC>::get(sm[t], k), FmVec<VEC>::get(e, k));
                    FmVec<VEC>::set(acc, k, __fsub_rn(FmVec<VEC>::get(acc, k), __fmul_rn(lr, g)));
                }
            }
        }
    }
    if (live)
        *reinterpret_cast<V *>(row + col) = acc;
}

// A long run, 64 columns, by the whole workgroup (see the head of the file).  s_d: 2 * kFmCoopRound * 64 floats.
template <bool FIXED, bool GS>
__device__ __forceinline__ void fm_coop_run(float *__restrict__ row, int col, bool live, const int32_t *__restrict__ perm,
                                            int s, int len, uint32_t width, const float *__restrict__ g_sum,
                                            const float *__restrict__ g_fm, const float *__restrict__ sum, float lr, int bag,
                                            const int32_t *__restrict__ bag_of, float *s_d) {
    const int lane = lane_id(), w = static_cast<int>(threadIdx.x >> 6);
    const int colc = live ? col : 0;
    const float e = row[colc];
    float acc = e;
    int buf = 0;
    // waves 1 .. 15 form the values, kFmCoopPerWave occurrences each per round; wave 0 only runs the chain.  The bags of a
    // wave's occurrences are requested one round ahead, so a round waits for one memory round trip, not two or three.
    const int first = (w - 1) * kFmCoopPerWave;
    int cnt_next = w == 0 ? 0 : max(0, min(kFmCoopPerWave, len - first));      // (wave-uniform)
    int bg_next = 0;
    if (cnt_next > 0)
        bg_next = fm_bag<FIXED>(perm[s + first + min(lane, cnt_next - 1)], bag, bag_of);
    for (int r0 = 0; r0 < len; r0 += kFmCoopRound) {
        const int cnt = cnt_next, bg = bg_next;
        const int t0n = r0 + kFmCoopRound + first;
        cnt_next = w == 0 ? 0 : max(0, min(kFmCoopPerWave, len - t0n));
        if (cnt_next > 0)
            bg_next = fm_bag<FIXED>(perm[s + t0n + min(lane, cnt_next - 1)], bag, bag_of);
        float *dst = s_d + (buf * kFmCoopRound + first) * kWave + lane;
        if (cnt > 0) {
            float gf[kFmCoopPerWave], sm[kFmCoopPerWave], gs[kFmCoopPerWave];
#pragma unroll
            for (int t = 0; t < kFmCoopPerWave; ++t) {
                if (t < cnt) {
                    const uint64_t off = static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readlane(bg, t))) * width + colc;
                    gf[t] = g_fm[off];
                    sm[t] = sum[off];
                    if (GS)
                        gs[t] = g_sum[off];
                }
            }
#pragma unroll
            for (int t = 0; t < kFmCoopPerWave; ++t)
                if (t < cnt)
                    dst[t * kWave] = __fmul_rn(lr, fm_g<GS>(GS ? gs[t] : 0.f, gf[t], sm[t], e));
        }
        __syncthreads();
        if (w == 0) {
            const int m = min(kFmCoopRound, len - r0);
            const float *src = s_d + buf * kFmCoopRound * kWave + lane;
            int t = 0;
            for (; t + 8 <= m; t += 8) {
                float d[8];
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    d[q] = src[(t + q) * kWave];
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    acc = __fsub_rn(acc, d[q]);
            }
            for (; t < m; ++t)
                acc = __fsub_rn(acc, src[t * kWave]);
        }
        buf ^= 1;
    }
    if (w == 0 && live)
        row[col] = acc;
    __syncthreads();      // the buffers are free for the next listed item
}

// One wave per (unique key, chunk of 64 * VEC columns); the grid is sized by n, the waves beyond n_unique * nchunk leave at
// once.  Applies the runs shorter than kFmLongRun and lists the keys of the longer ones (plan header word 0 / long_list,
// the scratch the by-unique applies of scatter.hip use for the same list) ...
template <int VEC, bool FIXED, bool GS>
__global__ __launch_bounds__(kFmShortWaves * kWave) void fm_apply_short_kernel(
    float *__restrict__ table, uint64_t rows, uint32_t width, PlanHeader *__restrict__ hdr, const uint32_t *__restrict__ uniq,
    const int32_t *__restrict__ seg, const int32_t *__restrict__ counts, const int32_t *__restrict__ perm,
    const float *__restrict__ g_sum, const float *__restrict__ g_fm, const float *__restrict__ sum, float lr, int bag,
    const int32_t *__restrict__ bag_of, uint32_t nchunk, uint32_t *__restrict__ long_list) {
    const int lane = lane_id();
    const uint64_t it = static_cast<uint64_t>(blockIdx.x) * kFmShortWaves + (threadIdx.x >> 6);
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
        return;      // out-of-range id: ignored
    if (len >= kFmLongRun) {
        if (c == 0 && lane == 0)
            long_list[atomicAdd(reinterpret_cast<unsigned long long *>(&hdr->reserved[0]), 1ull)] = u;
        return;
    }
    constexpr int kBatch = VEC == 4 ? 4 : 16;
    const int s = uniform(seg[u]);
    const int bg = fm_bag<FIXED>(perm[s + min(lane, len - 1)], bag, bag_of);
    const uint32_t col = (c * kWave + lane) * VEC;
    fm_wave_run<VEC, GS, kBatch>(table + static_cast<uint64_t>(key) * width, static_cast<int>(col), col < width, bg, len, width,
                                 g_sum, g_fm, sum, lr);
}

// ... and serves them here: work item = (listed key, 64-column slice), one per workgroup at a time (fm_coop_run).
template <bool FIXED, bool GS>
__global__ __launch_bounds__(1024) void fm_apply_long_kernel(float *__restrict__ table, uint32_t width,
                                                             const PlanHeader *__restrict__ hdr, const uint32_t *__restrict__ uniq,
                                                             const int32_t *__restrict__ seg, const int32_t *__restrict__ counts,
                                                             const int32_t *__restrict__ perm, const float *__restrict__ g_sum,
                                                             const float *__restrict__ g_fm, const float *__restrict__ sum,
                                                             float lr, int bag, const int32_t *__restrict__ bag_of,
                                                             uint32_t nslice, const uint32_t *__restrict__ long_list) {
    __shared__ __attribute__((aligned(16))) float s_d[2 * kFmCoopRound * kWave];
    const int lane = lane_id();
    const uint64_t items = static_cast<uint64_t>(hdr->reserved[0]) * nslice;
    for (uint64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const uint32_t u = uniform(long_list[it / nslice]);
        const uint32_t col = static_cast<uint32_t>(it % nslice) * kWave + lane;
        fm_coop_run<FIXED, GS>(table + static_cast<uint64_t>(uniform(uniq[u])) * width, static_cast<int>(col), col < width, perm,
                               uniform(seg[u]), uniform(counts[u]), width, g_sum, g_fm, sum, lr, bag, bag_of, s_d);
    }
}

// Tolerance mode: the two [n, width] tensors of the composed sequence.  E[i,:] = table[key_i,:] (zeros for a key >= rows, as
// ha_gather_* writes them) and, with g_sum, G[i,:] = g_sum[bag of i,:] -- by sorted position: key_i = sorted[p], i = perm[p].
template <bool FIXED>
__global__ __launch_bounds__(256) void fm_expand_kernel(const float *__restrict__ table, uint64_t rows, uint32_t width,
                                                        const uint32_t *__restrict__ sorted, const int32_t *__restrict__ perm,
                                                        uint64_t total, const float *__restrict__ g_sum, int bag,
                                                        const int32_t *__restrict__ bag_of, float *__restrict__ E,
                                                        float *__restrict__ G) {
    for (uint64_t x = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x; x < total;
         x += static_cast<uint64_t>(gridDim.x) * 256) {
        const uint64_t p = x / width;
        const uint32_t c = static_cast<uint32_t>(x - p * width);
        const uint32_t key = sorted[p];
        const uint64_t i = static_cast<uint64_t>(perm[p]);
        E[i * width + c] = key < rows ? table[static_cast<uint64_t>(key) * width + c] : 0.f;
        if (G != nullptr)
            G[i * width + c] = g_sum[static_cast<uint64_t>(fm_bag<FIXED>(static_cast<int>(i), bag, bag_of)) * width + c];
    }
}

// the argument rules of the three entry points; everything here precedes any device access
static int fm_apply_args_ok(const char *what, int64_t rows, int64_t width, int64_t n, int64_t bag, bool ragged, int64_t nbags) {
    HA_REQUIRE(rows >= 0 && width >= 1 && width < (1ll << 30) && n >= 0 && n < (1ll << 31) && nbags >= 0 && nbags < (1ll << 31) &&
                   bag >= 0 && bag < (1ll << 31),
               "%s: bad sizes rows=%ld width=%ld n=%ld bag=%ld nbags=%ld", what, (long)rows, (long)width, (long)n, (long)bag,
               (long)nbags);
    HA_REQUIRE((bag >= 1) != ragged, "%s: give exactly one of bag >= 1 and %s (bag=%ld)", what,
               "bag_of / offsets", (long)bag);
    HA_REQUIRE(ragged || (n % bag == 0 && n / bag == nbags), "%s: n=%ld is not nbags=%ld bags of bag=%ld ids", what, (long)n,
               (long)nbags, (long)bag);
    return 0;
}

static int fm_apply(const char *what, float *table, int64_t rows, int64_t width, void *plan_ws, int64_t n, const float *g_sum,
                    const float *g_fm, const float *sum, int64_t bag, const int32_t *bag_of, int64_t nbags, float lr,
                    hipStream_t stream) {
    if (fm_apply_args_ok(what, rows, width, n, bag, bag_of != nullptr, nbags))
        return -1;
    if (n == 0)
        return 0;
    HA_REQUIRE(table && plan_ws && g_fm && sum, "%s: null pointer (table, plan_ws, g_fm and sum are required)", what);
    HA_REQUIRE(nbags >= 1, "%s: %ld ids in no bag", what, (long)n);
    HA_REQUIRE(g_fm != table && sum != table && g_sum != table, "%s: g_sum, g_fm and sum must not alias the table", what);
    PlanPtrs p = plan_layout(plan_ws, n);
    const bool fixed = bag_of == nullptr;
    if (tolerance_tree_from() > 0) {
        // the composed sequence itself, through the per-stream scratch: whatever ha_sgd_apply is in this mode
        const size_t nw = static_cast<size_t>(n) * static_cast<size_t>(width);
        void *ws = nullptr;
        if (scratch_get(stream, 2 * nw * sizeof(float), &ws))
            return -1;
        float *E = static_cast<float *>(ws), *G = E + nw;
        const unsigned blocks = static_cast<unsigned>(nw / 256 + 1 < 4096 ? nw / 256 + 1 : 4096);
        if (fixed)
            hipLaunchKernelGGL((fm_expand_kernel<true>), dim3(blocks), dim3(256), 0, stream, table, (uint64_t)rows, (uint32_t)width,
                               p.sorted, p.perm, (uint64_t)nw, g_sum, (int)bag, bag_of, E, g_sum ? G : nullptr);
        else
            hipLaunchKernelGGL((fm_expand_kernel<false>), dim3(blocks), dim3(256), 0, stream, table, (uint64_t)rows, (uint32_t)width,
                               p.sorted, p.perm, (uint64_t)nw, g_sum, (int)bag, bag_of, E, g_sum ? G : nullptr);
        HA_LAUNCH_CHECK();
        if (ha_fm_grad_rows(g_sum ? G : nullptr, E, sum, g_fm, n, width, bag, bag_of, nbags, G, stream))
            return -1;
        return ha_sgd_apply_finished(table, rows, width, plan_ws, n, G, lr, stream);
    }
    const bool vec_ok = (width % 4 == 0) &&
                        ((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(g_sum) |
                          reinterpret_cast<uintptr_t>(g_fm) | reinterpret_cast<uintptr_t>(sum)) % 16 == 0);
    const uint32_t nslice = static_cast<uint32_t>((width + kWave - 1) / kWave);
    const uint32_t nchunk = vec_ok ? (nslice + 3) / 4 : nslice;
    const uint64_t blocks64 = (static_cast<uint64_t>(n) * nchunk + kFmShortWaves - 1) / kFmShortWaves;      // n_unique <= n
    HA_REQUIRE(blocks64 < (1ull << 31), "%s: batch too large (n=%ld ids of width %ld)", what, (long)n, (long)width);
    const dim3 grid(static_cast<unsigned>(blocks64)), block(kFmShortWaves * kWave);
    // the list of the long keys: counter in plan header word 0, entries in the plan's keys_alt (free once the plan is sorted)
    HA_CHECK_HIP(hipMemsetAsync(&p.hdr->reserved[0], 0, sizeof(int64_t), stream));
#define HA_FM_SHORT_CASE(V, F, S)                                                                                          \
    hipLaunchKernelGGL((fm_apply_short_kernel<V, F, S>), grid, block, 0, stream, table, (uint64_t)rows, (uint32_t)width,   \
                       p.hdr, p.uniq, p.seg, p.counts, p.perm, g_sum, g_fm, sum, lr, (int)bag, bag_of, nchunk, p.keys_alt)
#define HA_FM_LONG_CASE(F, S)                                                                                              \
    hipLaunchKernelGGL((fm_apply_long_kernel<F, S>), dim3(kFmLongBlocks), dim3(kFmWaves * kWave), 0, stream, table,        \
                       (uint32_t)width, p.hdr, p.uniq, p.seg, p.counts, p.perm, g_sum, g_fm, sum, lr, (int)bag, bag_of,    \
                       nslice, p.keys_alt)
#define HA_FM_APPLY_CASE(F, S)                                                                                             \
    do {                                                                                                                   \
        if (vec_ok) HA_FM_SHORT_CASE(4, F, S);                                                                             \
        else HA_FM_SHORT_CASE(1, F, S);                                                                                    \
        HA_FM_LONG_CASE(F, S);                                                                                             \
    } while (0)
    if (fixed && g_sum) HA_FM_APPLY_CASE(true, true);
    else if (fixed) HA_FM_APPLY_CASE(true, false);
    else if (g_sum) HA_FM_APPLY_CASE(false, true);
    else HA_FM_APPLY_CASE(false, false);
#undef HA_FM_APPLY_CASE
#undef HA_FM_LONG_CASE
#undef HA_FM_SHORT_CASE
    HA_LAUNCH_CHECK();
    return 0;
}

// One call: plan (sort + finish) (+ ha_bag_of) + the apply, on the per-stream scratch.  In tolerance mode the scratch also
// holds the two [n, width] tensors of the composed sequence, behind the plan.
template <typename IdT>
static int sgd_sparse_update_fm_bags(const char *what, float *table, int64_t rows, int64_t width, const IdT *ids, int64_t n,
                                     int64_t bag, const int64_t *offsets, int64_t nbags, const float *g_sum, const float *g_fm,
                                     const float *sum, float lr, ha_stream_t stream) {
    if (fm_apply_args_ok(what, rows, width, n, bag, offsets != nullptr, nbags))
        return -1;
    if (n == 0)
        return 0;
    HA_REQUIRE(table && ids && g_fm && sum, "%s: null pointer (table, ids, g_fm and sum are required)", what);
    HA_REQUIRE(nbags >= 1, "%s: %ld ids in no bag", what, (long)n);
    HA_REQUIRE(g_fm != table && sum != table && g_sum != table, "%s: g_sum, g_fm and sum must not alias the table", what);
    hipStream_t s = as_stream(stream);
    const size_t plan_bytes = align_up(ha_plan_bytes(n), 256);
    const size_t map_bytes = align_up(offsets ? static_cast<size_t>(n) * 4 : 0, 256);
    const bool composed = tolerance_tree_from() > 0;
    const size_t nw = static_cast<size_t>(n) * static_cast<size_t>(width);
    void *ws = nullptr;
    if (scratch_get(s, plan_bytes + map_bytes + (composed ? 2 * nw * sizeof(float) : 0), &ws))
        return -1;
    int32_t *bag_of = nullptr;
    if (offsets) {
        bag_of = reinterpret_cast<int32_t *>(static_cast<char *>(ws) + plan_bytes);
        if (ha_bag_of(offsets, nbags, n, bag_of, stream))
            return -1;
    }
    if (sizeof(IdT) == 4 ? ha_plan_sort_f32ids(reinterpret_cast<const float *>(ids), n, ws, stream)
                         : ha_plan_sort_u64ids(reinterpret_cast<const uint64_t *>(ids), n, ws, stream))
        return -1;
    if (ha_plan_finish(ws, n, stream))
        return -1;
    if (!composed)
        return fm_apply(what, table, rows, width, ws, n, g_sum, g_fm, sum, offsets ? 0 : bag, bag_of, nbags, lr, s);
    // (the scratch is in use: the composed sequence here, not through fm_apply, which would ask for the scratch again)
    PlanPtrs p = plan_layout(ws, n);
    float *E = reinterpret_cast<float *>(static_cast<char *>(ws) + plan_bytes + map_bytes), *G = E + nw;
    const unsigned blocks = static_cast<unsigned>(nw / 256 + 1 < 4096 ? nw / 256 + 1 : 4096);
    if (!offsets)
        hipLaunchKernelGGL((fm_expand_kernel<true>), dim3(blocks), dim3(256), 0, s, table, (uint64_t)rows, (uint32_t)width, p.sorted,
                           p.perm, (uint64_t)nw, g_sum, (int)bag, bag_of, E, g_sum ? G : nullptr);
    else
        hipLaunchKernelGGL((fm_expand_kernel<false>), dim3(blocks), dim3(256), 0, s, table, (uint64_t)rows, (uint32_t)width, p.sorted,
                           p.perm, (uint64_t)nw, g_sum, 0, bag_of, E, g_sum ? G : nullptr);
    HA_LAUNCH_CHECK();
    if (ha_fm_grad_rows(g_sum ? G : nullptr, E, sum, g_fm, n, width, offsets ? 0 : bag, bag_of, nbags, G, stream))
        return -1;
    return ha_sgd_apply_finished(table, rows, width, ws, n, G, lr, stream);
}

}  // namespace ha

extern "C" int ha_sgd_apply_fm_bags(float *table, int64_t rows, int64_t width, void *plan_ws, int64_t n, const float *g_sum,
                                    const float *g_fm, const float *sum, int64_t bag, const int32_t *bag_of, int64_t nbags,
                                    float lr, ha_stream_t stream) {
    return ha::fm_apply("ha_sgd_apply_fm_bags", table, rows, width, plan_ws, n, g_sum, g_fm, sum, bag, bag_of, nbags, lr,
                        ha::as_stream(stream));
}

extern "C" int ha_sgd_sparse_update_fm_bags_f32ids(float *table, int64_t rows, int64_t width, const float *ids, int64_t n,
                                                   int64_t bag, const int64_t *offsets, int64_t nbags, const float *g_sum,
                                                   const float *g_fm, const float *sum, float lr, ha_stream_t stream) {
    return ha::sgd_sparse_update_fm_bags<float>("ha_sgd_sparse_update_fm_bags_f32ids", table, rows, width, ids, n, bag, offsets,
                                                nbags, g_sum, g_fm, sum, lr, stream);
}

extern "C" int ha_sgd_sparse_update_fm_bags_u64ids(float *table, int64_t rows, int64_t width, const uint64_t *ids, int64_t n,
                                                   int64_t bag, const int64_t *offsets, int64_t nbags, const float *g_sum,
                                                   const float *g_fm, const float *sum, float lr, ha_stream_t stream) {
    return ha::sgd_sparse_update_fm_bags<uint64_t>("ha_sgd_sparse_update_fm_bags_u64ids", table, rows, width, ids, n, bag,
                                                   offsets, nbags, g_sum, g_fm, sum, lr, stream);
}

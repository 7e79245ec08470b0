// Weighted FM-pooled lookup: the second-order term of the reference's FAE DeepFM (examples/ctr/models/fae_deepfm_avazu.py:43-80)
//     x = mul_op(embedding_lookup_op(Embedding, cold_sparse_input), broadcast(cold_category_input))
//     S = reduce_sum_op(x, axes=1);   Q = reduce_sum_op(mul_op(x, x), axes=1)
// where the square of the sum is taken only after the hot table's half has been added: S and Q leave as two [B, width]
// tensors.  Live occurrences are wbag.hip's: weight not zero (a NaN weight is not zero) and id below `rows`; a dead occurrence
// takes no part in anything, whatever its row or its bag's gradients hold.
//
//   forward   per bag and column, in position order over the LIVE occurrences, from S = Q = +0:
//             x = fl(w_j * r_j);  S = fl(S + x);  Q = fl(Q + fl(x * x))       (no FMA anywhere)
//             S is ha_gather_wsum_* bit for bit; all weights 1.0f: S and fl(0.5 * fl(fl(S*S) - Q)) are ha_gather_fm_*'s outputs.
//   gradient  x = fl(w * e);  t = fl(g_Q[b] * x);  a = fl(g_S[b] + fl(t + t));  out[i] = fl(w * a), +0.0f for a zero weight
//             (e: row i of a gathered row buffer) -- the project's fixed order, an ordinary unpooled gradient [n, width].
//   apply     for every key k < rows: e = table[k,:] as it is before the call, acc = e; over the key's live occurrences in
//             ascending order g as above FROM e (never from acc), acc = fl(acc - fl(lr * g)); the row is written once.  A key
//             without live occurrence keeps its bits.  Bit for bit gather + gradient + ha_sgd_apply_finished while the table
//             has not changed since the gather, except wbag.hip's corner: lr < 0 and a -0.0f element under a dead occurrence.
//
// MI355X layout.  wbag.hip's, kernel for kernel.  Forward: one wave per (bag, column slice), lane l holds id l and weight l
// of the current block of 64, v_readlane broadcasts both, ROWS branch-free loads in flight before the first add, two
// accumulators, two nontemporal stores; a dead occurrence loads row 0 and a wave-uniform select discards it.  Apply: two
// launches over a FINISHED plan -- runs shorter than kPlanLongRun by one wave per (unique key, column chunk) that loads e once
// and both gradients of a batch of occurrences before the first arithmetic; longer ones by a workgroup per (listed key,
// 64-column slice) where waves 1 .. 15 each load e themselves and leave fl(lr * g) with a live flag in LDS, and wave 0 runs the
// chain, which is the final subtraction only.  That split is valid because e is fixed: everything in front of the subtraction
// is independent per occurrence.
#include "wbag_dev.h"

namespace ha {

int scratch_get(hipStream_t stream, size_t bytes, void **out);   // capi.hip
int tolerance_tree_from();                                       // scatter.hip

// fl(lr * g) is formed by the callers that need it; this is g for a LIVE occurrence: four multiplies and two adds, each rounded
__device__ __forceinline__ float wfm_grad(float w, float e, float gs, float gq) {
    const float t = __fmul_rn(gq, __fmul_rn(w, e));
    return __fmul_rn(w, __fadd_rn(gs, __fadd_rn(t, t)));
}

// ---- forward ---------------------------------------------------------------------------------------------------------------
// ROWS: table rows requested per round (all in flight before the first add).
template <typename IdT, int VEC, int ROWS>
__global__ __launch_bounds__(kWbagWaves *kWave) void wfm_sum_kernel(
    const float *__restrict__ table, uint64_t rows, uint32_t width, const IdT *__restrict__ ids,
    const float *__restrict__ weights, int64_t n, int64_t bag, const int64_t *__restrict__ offsets, int64_t nbags,
    uint32_t nslice, float *__restrict__ out_sum, float *__restrict__ out_sq) {
    typedef typename WVec<VEC>::T V;
    const int lane = lane_id();
    const uint64_t item = static_cast<uint64_t>(blockIdx.x) * kWbagWaves + (threadIdx.x >> 6);   // wave-uniform
    if (item >= static_cast<uint64_t>(nbags) * nslice)
        return;
    const int64_t b = static_cast<int64_t>(item / nslice);
    const uint32_t sl = static_cast<uint32_t>(item - static_cast<uint64_t>(b) * nslice);
    int64_t lo, hi;
    if (offsets != nullptr) {      // clamped as bagsum.hip clamps them: no id at or beyond n is read
        lo = offsets[b];
        hi = offsets[b + 1];
        lo = lo < 0 ? 0 : (lo > n ? n : lo);
        hi = hi < lo ? lo : (hi > n ? n : hi);
    } else {
        lo = b * bag;
        hi = lo + bag;      // (n == nbags * bag: checked by the host)
    }
    const uint32_t col = (sl * kWave + lane) * VEC;
    const bool live = col < width;       // (VEC > 1: width % VEC == 0, so a live lane's VEC columns all exist)
    const uint32_t lcol = live ? col : 0;
    V acc_s, acc_q;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        WVec<VEC>::set(acc_s, k, 0.f);
        WVec<VEC>::set(acc_q, k, 0.f);
    }
    for (int64_t j0 = lo; j0 < hi; j0 += kWave) {
        const int cnt = static_cast<int>(hi - j0 < kWave ? hi - j0 : kWave);      // occurrences of this block (wave-uniform)
        const int64_t j = j0 + (lane < cnt ? lane : cnt - 1);                      // lo <= j < hi <= n
        const uint64_t r = id_to_row<IdT>(ids[j]);
        const float w = weights[j];
        const bool ok = r < rows && w != 0.f;       // the live occurrences (a NaN weight is not zero)
        const unsigned long long okm = __ballot(ok);
        const uint64_t off = (ok ? r : 0) * width;          // float offset of the row (row 0 for a dead occurrence)
        const int off_lo = static_cast<int>(static_cast<uint32_t>(off));
        const int off_hi = static_cast<int>(static_cast<uint32_t>(off >> 32));
        const int wbits = __float_as_int(w);
        for (int c = 0; c < cnt; c += ROWS) {
            V v[ROWS];
#pragma unroll
            for (int t = 0; t < ROWS; ++t) {
                const int tt = c + t < cnt ? c + t : cnt - 1;
                const uint64_t o = (static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readlane(off_hi, tt))) << 32) |
                                   static_cast<uint32_t>(__builtin_amdgcn_readlane(off_lo, tt));
                v[t] = *reinterpret_cast<const V *>(table + o + lcol);
            }
            __builtin_amdgcn_sched_barrier(0);      // (as wbag_sum_kernel: the whole round is requested before the first add)
#pragma unroll
            for (int t = 0; t < ROWS; ++t) {
                const int tt = c + t < cnt ? c + t : 0;                                    // wave-uniform
                const bool rok = c + t < cnt && ((okm >> tt) & 1ull) != 0;                 // a dead occurrence leaves both alone
                const float wt = __int_as_float(__builtin_amdgcn_readlane(wbits, tt));
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const float as = WVec<VEC>::get(acc_s, k), aq = WVec<VEC>::get(acc_q, k);
                    const float x = __fmul_rn(wt, WVec<VEC>::get(v[t], k));
                    const float s = __fadd_rn(as, x);
                    const float q = __fadd_rn(aq, __fmul_rn(x, x));
                    WVec<VEC>::set(acc_s, k, rok ? s : as);
                    WVec<VEC>::set(acc_q, k, rok ? q : aq);
                }
            }
        }
    }
    // both pooled tensors are consumed by another kernel (the dense tower): written around the L2, as the gather's
    if (live) {
        const uint64_t o = static_cast<uint64_t>(b) * width + col;
        __builtin_nontemporal_store(acc_s, reinterpret_cast<V *>(out_sum + o));
        __builtin_nontemporal_store(acc_q, reinterpret_cast<V *>(out_sq + o));
    }
}

// ---- per-occurrence gradient --------------------------------------------------------------------------------------------------
// out[i,c] = fl(w_i * fl(g_S[b,c] + 2 * fl(g_Q[b,c] * fl(w_i * e[i,c])))); +0.0f for a zero weight, whatever the operands hold.
// A thread handles one vector of VEC floats: it reads its element of emb_rows before it writes the same element of out, so
// out may be emb_rows itself (neither is __restrict__).
template <int VEC>
__global__ __launch_bounds__(256) void wfm_grad_rows_kernel(const float *__restrict__ g_sum, const float *__restrict__ g_sq,
                                                            const float *__restrict__ weights, const float *emb_rows,
                                                            uint64_t total_vec, uint32_t nv, uint32_t bag,
                                                            const int32_t *__restrict__ bag_of, uint32_t nbags, float *out) {
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
    b = b < nbags ? b : nbags - 1;       // (no row beyond the gradients is read whatever bag_of holds)
    const float w = weights[i];
    const uint64_t go = (static_cast<uint64_t>(b) * nv + cv) * VEC;
    const V gs = *reinterpret_cast<const V *>(g_sum + go);
    const V gq = *reinterpret_cast<const V *>(g_sq + go);
    const V r = *reinterpret_cast<const V *>(emb_rows + e * VEC);
    V o;
#pragma unroll
    for (int k = 0; k < VEC; ++k)
        WVec<VEC>::set(o, k, w != 0.f ? wfm_grad(w, WVec<VEC>::get(r, k), WVec<VEC>::get(gs, k), WVec<VEC>::get(gq, k)) : 0.f);
    *reinterpret_cast<V *>(out + e * VEC) = o;
}

// Tolerance mode: the row buffer of the composed sequence, E[i,:] = table[key_i,:] (zeros for a key >= rows, as ha_gather_*
// writes them), by sorted position: key_i = sorted[p], i = perm[p].
__global__ __launch_bounds__(256) void wfm_expand_kernel(const float *__restrict__ table, uint64_t rows, uint32_t width,
                                                         const uint32_t *__restrict__ sorted, const int32_t *__restrict__ perm,
                                                         uint64_t total, float *__restrict__ E) {
    for (uint64_t x = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x; x < total;
         x += static_cast<uint64_t>(gridDim.x) * 256) {
        const uint64_t p = x / width;
        const uint32_t c = static_cast<uint32_t>(x - p * width);
        const uint32_t key = sorted[p];
        const uint64_t i = static_cast<uint64_t>(perm[p]);
        E[i * width + c] = key < rows ? table[static_cast<uint64_t>(key) * width + c] : 0.f;
    }
}

// ---- apply ---------------------------------------------------------------------------------------------------------------------
// A run shorter than kPlanLongRun, by one wave: columns col .. col + VEC - 1 of every lane.  bg / wbits: lanes 0 .. len-1 hold
// the bags and the weights of the run's occurrences in occurrence order.
template <int VEC, int BATCH>
__device__ __forceinline__ void wfm_wave_run(float *__restrict__ row, int col, bool live, int bg, int wbits, int len,
                                             uint32_t width, const float *__restrict__ g_sum, const float *__restrict__ g_sq,
                                             float lr) {
    typedef typename WVec<VEC>::T V;
    const int colc = live ? col : 0;      // lanes beyond the row load column 0 and store nothing
    const V e = *reinterpret_cast<const V *>(row + colc);      // the row as it is before the call: every g is formed from it
    V acc = e;
    for (int t0 = 0; t0 < len; t0 += BATCH) {
        const int cnt = min(BATCH, len - t0);
        V gs[BATCH], gq[BATCH];
#pragma unroll
        for (int t = 0; t < BATCH; ++t) {
            if (t < cnt) {
                const uint64_t off = static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readlane(bg, t0 + t))) * width + colc;
                gs[t] = *reinterpret_cast<const V *>(g_sum + off);
                gq[t] = *reinterpret_cast<const V *>(g_sq + off);
            }
        }
#pragma unroll
        for (int t = 0; t < BATCH; ++t) {
            if (t < cnt) {
                const float w = __int_as_float(__builtin_amdgcn_readlane(wbits, t0 + t));      // wave-uniform
                if (w != 0.f) {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) {
                        const float g = wfm_grad(w, WVec<VEC>::get(e, k), WVec<VEC>::get(gs[t], k), WVec<VEC>::get(gq[t], k));
                        WVec<VEC>::set(acc, k, __fsub_rn(WVec<VEC>::get(acc, k), __fmul_rn(lr, g)));
                    }
                }
            }
        }
    }
    if (live)      // (no live occurrence: the bits that were read)
        *reinterpret_cast<V *>(row + col) = acc;
}

// A long run, 64 columns, by the whole workgroup.  s_d: 2 * kWbagCoopRound * 64 floats, s_live: 2 * kWbagCoopRound flags.
template <bool FIXED>
__device__ __forceinline__ void wfm_coop_run(float *__restrict__ row, int col, bool live, const int32_t *__restrict__ perm, int s,
                                             int len, uint32_t width, const float *__restrict__ g_sum,
                                             const float *__restrict__ g_sq, const float *__restrict__ weights, float lr, int bag,
                                             const int32_t *__restrict__ bag_of, float *s_d, int *s_live) {
    const int lane = lane_id(), w = static_cast<int>(threadIdx.x >> 6);
    const int colc = live ? col : 0;
    // every wave loads the slice itself, before the item's first barrier: e of waves 1 .. 15, the chain's start of wave 0.  The
    // row is stored only after the item's last barrier, so every wave has seen the row as it is before the call.
    const float e = row[colc];
    float acc = e;
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
            float gs[kWbagCoopPerWave], gq[kWbagCoopPerWave];
#pragma unroll
            for (int t = 0; t < kWbagCoopPerWave; ++t) {
                if (t < cnt) {
                    const uint64_t off = static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readlane(bg, t))) * width + colc;
                    gs[t] = g_sum[off];
                    gq[t] = g_sq[off];
                }
            }
#pragma unroll
            for (int t = 0; t < kWbagCoopPerWave; ++t)
                if (t < cnt)      // (a dead occurrence's value is never read: its flag is 0)
                    dst[t * kWave] = __fmul_rn(lr, wfm_grad(__int_as_float(__builtin_amdgcn_readlane(wbits, t)), e, gs[t], gq[t]));
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
// once.  Applies the runs shorter than kPlanLongRun and lists the keys of the longer ones (plan header word 0 / long_list, as
// wbag.hip and fmapply.hip do) ...
template <int VEC, bool FIXED>
__global__ __launch_bounds__(kWbagWaves *kWave) void wfm_apply_short_kernel(
    float *__restrict__ table, uint64_t rows, uint32_t width, PlanHeader *__restrict__ hdr, const uint32_t *__restrict__ uniq,
    const int32_t *__restrict__ seg, const int32_t *__restrict__ counts, const int32_t *__restrict__ perm,
    const float *__restrict__ g_sum, const float *__restrict__ g_sq, const float *__restrict__ weights, float lr, int bag,
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
    wfm_wave_run<VEC, kBatch>(table + static_cast<uint64_t>(key) * width, static_cast<int>(col), col < width, bg, wbits, len,
                              width, g_sum, g_sq, lr);
}

// ... and serves them here: work item = (listed key, 64-column slice), one per workgroup at a time (wfm_coop_run).
template <bool FIXED>
__global__ __launch_bounds__(kWbagLongWaves *kWave) void wfm_apply_long_kernel(
    float *__restrict__ table, uint32_t width, const PlanHeader *__restrict__ hdr, const uint32_t *__restrict__ uniq,
    const int32_t *__restrict__ seg, const int32_t *__restrict__ counts, const int32_t *__restrict__ perm,
    const float *__restrict__ g_sum, const float *__restrict__ g_sq, const float *__restrict__ weights, float lr, int bag,
    const int32_t *__restrict__ bag_of, uint32_t nslice, const uint32_t *__restrict__ long_list) {
    __shared__ __attribute__((aligned(16))) float s_d[2 * kWbagCoopRound * kWave];
    __shared__ int s_live[2 * kWbagCoopRound];
    const int lane = lane_id();
    const uint64_t items = static_cast<uint64_t>(hdr->reserved[0]) * nslice;
    for (uint64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const uint32_t u = uniform(long_list[it / nslice]);
        const uint32_t col = static_cast<uint32_t>(it % nslice) * kWave + lane;
        wfm_coop_run<FIXED>(table + static_cast<uint64_t>(uniform(uniq[u])) * width, static_cast<int>(col), col < width, perm,
                            uniform(seg[u]), uniform(counts[u]), width, g_sum, g_sq, weights, lr, bag, bag_of, s_d, s_live);
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
// the argument rules of every entry point (wbag.hip's); everything here precedes any device access
static int wfm_args_ok(const char *what, int64_t rows, int64_t width, int64_t n, int64_t bag, bool ragged, int64_t nbags) {
    HA_REQUIRE(rows >= 0 && width >= 1 && width < (1ll << 30) && n >= 0 && n < (1ll << 31) && nbags >= 0 && nbags < (1ll << 31) &&
                   bag >= 0 && bag < (1ll << 31),
               "%s: bad sizes rows=%ld width=%ld n=%ld bag=%ld nbags=%ld", what, (long)rows, (long)width, (long)n, (long)bag,
               (long)nbags);
    HA_REQUIRE((bag >= 1) != ragged, "%s: give exactly one of bag >= 1 and %s (bag=%ld)", what, "bag_of / offsets", (long)bag);
    HA_REQUIRE(ragged || (n % bag == 0 && n / bag == nbags), "%s: n=%ld is not nbags=%ld bags of bag=%ld ids", what, (long)n,
               (long)nbags, (long)bag);
    return 0;
}

// [p, p + bytes) and [q, q + qbytes) share a byte
static bool wfm_overlap(const void *p, size_t bytes, const void *q, size_t qbytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return p != nullptr && q != nullptr && a < b + qbytes && b < a + bytes;
}

template <typename IdT>
static int wfm_sum_launch(const char *what, const float *table, int64_t rows, int64_t width, const IdT *ids,
                          const float *weights, int64_t n, int64_t bag, const int64_t *offsets, int64_t nbags, float *out_sum,
                          float *out_sq, hipStream_t stream) {
    if (wfm_args_ok(what, rows, width, n, bag, offsets != nullptr, nbags))
        return -1;
    if (n == 0 && (nbags == 0 || (out_sum == nullptr && out_sq == nullptr)))
        return 0;
    HA_REQUIRE(nbags >= 1, "%s: %ld ids in no bag", what, (long)n);
    HA_REQUIRE(out_sum != nullptr && out_sq != nullptr, "%s: null out_sum or out_sq (both outputs are required)", what);
    HA_REQUIRE(table != nullptr || n == 0, "%s: null table", what);
    HA_REQUIRE((ids != nullptr && weights != nullptr) || n == 0, "%s: null ids or weights", what);
    const size_t out_bytes = static_cast<size_t>(nbags) * width * sizeof(float);
    HA_REQUIRE(!wfm_overlap(out_sum, out_bytes, out_sq, out_bytes), "%s: out_sum and out_sq must not overlap", what);
    if (rows == 0 || n == 0) {      // no live occurrence (and no row 0 for the clamped loads to read)
        HA_CHECK_HIP(hipMemsetAsync(out_sum, 0, out_bytes, stream));
        HA_CHECK_HIP(hipMemsetAsync(out_sq, 0, out_bytes, stream));
        return 0;
    }
    const bool vec_ok = (width % 4 == 0) && ((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(out_sum) |
                                              reinterpret_cast<uintptr_t>(out_sq)) % 16 == 0);
    // wbag.hip's launch rule: the widest slice that is no wider than a row and still gives the chip 8 waves per compute unit
    int vec = 1;
    if (vec_ok)
        for (vec = 4; vec > 1; vec >>= 1)
            if (kWave * vec <= width && nbags * ((width + kWave * vec - 1) / (kWave * vec)) >= 2048)
                break;
    const uint32_t nslice = static_cast<uint32_t>((width + kWave * vec - 1) / (kWave * vec));
    const uint64_t blocks64 = (static_cast<uint64_t>(nbags) * nslice + kWbagWaves - 1) / kWbagWaves;
    HA_REQUIRE(blocks64 < (1ull << 31), "%s: batch too large", what);
    const int64_t mean = offsets ? (n + nbags - 1) / nbags : bag;      // rows per round by the (mean) bag size
    const bool few = mean <= 8;
    const dim3 grid(static_cast<unsigned>(blocks64)), block(kWbagWaves * kWave);
#define HA_WFM_CASE(V, R)                                                                                                    \
    hipLaunchKernelGGL((wfm_sum_kernel<IdT, V, R>), grid, block, 0, stream, table, (uint64_t)rows, (uint32_t)width, ids,     \
                       weights, n, bag, offsets, nbags, nslice, out_sum, out_sq)
    if (vec == 4) {
        if (few) HA_WFM_CASE(4, 8); else HA_WFM_CASE(4, 32);
    } else if (vec == 2) {
        if (few) HA_WFM_CASE(2, 8); else HA_WFM_CASE(2, 32);
    } else {
        if (few) HA_WFM_CASE(1, 8); else HA_WFM_CASE(1, 32);
    }
#undef HA_WFM_CASE
    HA_LAUNCH_CHECK();
    return 0;
}

static int wfm_grad_rows_launch(const char *what, const float *g_sum, const float *g_sq, const float *weights,
                                const float *emb_rows, int64_t n, int64_t width, int64_t bag, const int32_t *bag_of,
                                int64_t nbags, float *out, hipStream_t stream) {
    if (wfm_args_ok(what, 0, width, n, bag, bag_of != nullptr, nbags))
        return -1;
    if (n == 0)
        return 0;
    HA_REQUIRE(nbags >= 1, "%s: %ld occurrences in no bag", what, (long)n);
    HA_REQUIRE(g_sum && g_sq && weights && emb_rows && out, "%s: null pointer", what);
    const size_t out_bytes = static_cast<size_t>(n) * width * sizeof(float), g_bytes = static_cast<size_t>(nbags) * width * sizeof(float);
    HA_REQUIRE(!wfm_overlap(out, out_bytes, g_sum, g_bytes) && !wfm_overlap(out, out_bytes, g_sq, g_bytes) &&
                   !wfm_overlap(out, out_bytes, weights, static_cast<size_t>(n) * sizeof(float)),
               "%s: out must not alias g_sum, g_sq or weights (it may be emb_rows itself)", what);
    HA_REQUIRE(out == emb_rows || !wfm_overlap(out, out_bytes, emb_rows, out_bytes),
               "%s: out overlaps emb_rows without being emb_rows", what);
    const bool vec_ok = (width % 4 == 0) &&
                        ((reinterpret_cast<uintptr_t>(g_sum) | reinterpret_cast<uintptr_t>(g_sq) |
                          reinterpret_cast<uintptr_t>(emb_rows) | reinterpret_cast<uintptr_t>(out)) % 16 == 0);
    const int vec = vec_ok ? 4 : 1;
    const uint64_t total_vec = static_cast<uint64_t>(n) * static_cast<uint64_t>(width / vec);
    const uint64_t blocks64 = (total_vec + 255) / 256;
    HA_REQUIRE(blocks64 < (1ull << 31), "%s: batch too large", what);
    const dim3 grid(static_cast<unsigned>(blocks64)), block(256);
    if (vec == 4)
        hipLaunchKernelGGL((wfm_grad_rows_kernel<4>), grid, block, 0, stream, g_sum, g_sq, weights, emb_rows, total_vec,
                           (uint32_t)(width / 4), (uint32_t)bag, bag_of, (uint32_t)nbags, out);
    else
        hipLaunchKernelGGL((wfm_grad_rows_kernel<1>), grid, block, 0, stream, g_sum, g_sq, weights, emb_rows, total_vec,
                           (uint32_t)width, (uint32_t)bag, bag_of, (uint32_t)nbags, out);
    HA_LAUNCH_CHECK();
    return 0;
}

// the composed sequence of the tolerance modes over a finished plan: E = the rows (into the scratch at `E`), the gradient in
// place, ha_sgd_apply_finished -- whatever that is in this mode
static int wfm_apply_composed(const char *what, float *table, int64_t rows, int64_t width, void *plan_ws, int64_t n,
                              const float *g_sum, const float *g_sq, const float *weights, int64_t bag, const int32_t *bag_of,
                              int64_t nbags, float lr, float *E, hipStream_t stream) {
    PlanPtrs p = plan_layout(plan_ws, n);
    const size_t nw = static_cast<size_t>(n) * static_cast<size_t>(width);
    const unsigned blocks = static_cast<unsigned>(nw / 256 + 1 < 4096 ? nw / 256 + 1 : 4096);
    hipLaunchKernelGGL(wfm_expand_kernel, dim3(blocks), dim3(256), 0, stream, table, (uint64_t)rows, (uint32_t)width, p.sorted,
                       p.perm, (uint64_t)nw, E);
    HA_LAUNCH_CHECK();
    if (wfm_grad_rows_launch(what, g_sum, g_sq, weights, E, n, width, bag, bag_of, nbags, E, stream))
        return -1;
    return ha_sgd_apply_finished(table, rows, width, plan_ws, n, E, lr, reinterpret_cast<ha_stream_t>(stream));
}

// the two launches of the fused apply over a finished plan (mode 0); arguments already checked
static int wfm_apply_launch(const char *what, float *table, int64_t rows, int64_t width, void *plan_ws, int64_t n,
                            const float *g_sum, const float *g_sq, const float *weights, int64_t bag, const int32_t *bag_of,
                            float lr, hipStream_t stream) {
    PlanPtrs p = plan_layout(plan_ws, n);
    const bool fixed = bag_of == nullptr;
    const bool vec_ok = (width % 4 == 0) && ((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(g_sum) |
                                              reinterpret_cast<uintptr_t>(g_sq)) % 16 == 0);
    const uint32_t nslice = static_cast<uint32_t>((width + kWave - 1) / kWave);
    const uint32_t nchunk = vec_ok ? (nslice + 3) / 4 : nslice;
    const uint64_t blocks64 = (static_cast<uint64_t>(n) * nchunk + kWbagWaves - 1) / kWbagWaves;      // n_unique <= n
    HA_REQUIRE(blocks64 < (1ull << 31), "%s: batch too large (n=%ld ids of width %ld)", what, (long)n, (long)width);
    const dim3 grid(static_cast<unsigned>(blocks64)), block(kWbagWaves * kWave);
    // the list of the long keys: counter in plan header word 0, entries in the plan's keys_alt (free once the plan is sorted)
    HA_CHECK_HIP(hipMemsetAsync(&p.hdr->reserved[0], 0, sizeof(int64_t), stream));
#define HA_WFM_SHORT_CASE(V, F)                                                                                              \
    hipLaunchKernelGGL((wfm_apply_short_kernel<V, F>), grid, block, 0, stream, table, (uint64_t)rows, (uint32_t)width, p.hdr, \
                       p.uniq, p.seg, p.counts, p.perm, g_sum, g_sq, weights, lr, (int)bag, bag_of, nchunk, p.keys_alt)
#define HA_WFM_LONG_CASE(F)                                                                                                  \
    hipLaunchKernelGGL((wfm_apply_long_kernel<F>), dim3(kWbagLongBlocks), dim3(kWbagLongWaves * kWave), 0, stream, table,    \
                       (uint32_t)width, p.hdr, p.uniq, p.seg, p.counts, p.perm, g_sum, g_sq, weights, lr, (int)bag, bag_of,  \
                       nslice, p.keys_alt)
    if (fixed) {
        if (vec_ok) HA_WFM_SHORT_CASE(4, true); else HA_WFM_SHORT_CASE(1, true);
        HA_WFM_LONG_CASE(true);
    } else {
        if (vec_ok) HA_WFM_SHORT_CASE(4, false); else HA_WFM_SHORT_CASE(1, false);
        HA_WFM_LONG_CASE(false);
    }
#undef HA_WFM_LONG_CASE
#undef HA_WFM_SHORT_CASE
    HA_LAUNCH_CHECK();
    return 0;
}

// null pointers and aliasing of the gradients / weights with the table: shared by both apply entry points
static int wfm_apply_ptrs_ok(const char *what, const float *table, int64_t rows, int64_t width, int64_t n, const float *g_sum,
                             const float *g_sq, const float *weights, int64_t nbags) {
    HA_REQUIRE(nbags >= 1, "%s: %ld ids in no bag", what, (long)n);
    HA_REQUIRE(table && g_sum && g_sq && weights, "%s: null pointer", what);
    const size_t t_bytes = static_cast<size_t>(rows) * width * sizeof(float), g_bytes = static_cast<size_t>(nbags) * width * sizeof(float);
    HA_REQUIRE(g_sum != table && g_sq != table && weights != table && !wfm_overlap(table, t_bytes, g_sum, g_bytes) &&
                   !wfm_overlap(table, t_bytes, g_sq, g_bytes) &&
                   !wfm_overlap(table, t_bytes, weights, static_cast<size_t>(n) * sizeof(float)),
               "%s: g_sum, g_sq and weights must not alias the table", what);
    return 0;
}

static int wfm_apply(const char *what, float *table, int64_t rows, int64_t width, void *plan_ws, int64_t n, const float *g_sum,
                     const float *g_sq, const float *weights, int64_t bag, const int32_t *bag_of, int64_t nbags, float lr,
                     hipStream_t stream) {
    if (wfm_args_ok(what, rows, width, n, bag, bag_of != nullptr, nbags))
        return -1;
    if (n == 0)
        return 0;
    if (wfm_apply_ptrs_ok(what, table, rows, width, n, g_sum, g_sq, weights, nbags))
        return -1;
    HA_REQUIRE(plan_ws != nullptr, "%s: null plan_ws", what);
    if (tolerance_tree_from() > 0) {
        void *ws = nullptr;
        if (scratch_get(stream, static_cast<size_t>(n) * static_cast<size_t>(width) * sizeof(float), &ws))
            return -1;
        return wfm_apply_composed(what, table, rows, width, plan_ws, n, g_sum, g_sq, weights, bag, bag_of, nbags, lr,
                                  static_cast<float *>(ws), stream);
    }
    return wfm_apply_launch(what, table, rows, width, plan_ws, n, g_sum, g_sq, weights, bag, bag_of, lr, stream);
}

// One call: masked keys + plan (sort + finish) (+ ha_bag_of) + the apply, on the per-stream scratch; nothing is read back to
// the host.  In tolerance mode the composed sequence: the plan of the ids as they are, the rows and then the per-occurrence
// gradient in the scratch behind it, ha_sgd_apply_finished.
template <typename IdT>
static int sgd_sparse_update_wfm_bags(const char *what, float *table, int64_t rows, int64_t width, const IdT *ids,
                                      const float *weights, int64_t n, const float *g_sum, const float *g_sq, int64_t bag,
                                      const int64_t *offsets, int64_t nbags, float lr, ha_stream_t stream) {
    if (wfm_args_ok(what, rows, width, n, bag, offsets != nullptr, nbags))
        return -1;
    if (n == 0)
        return 0;
    if (wfm_apply_ptrs_ok(what, table, rows, width, n, g_sum, g_sq, weights, nbags))
        return -1;
    HA_REQUIRE(ids != nullptr, "%s: null ids", what);
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
        return wfm_apply_composed(what, table, rows, width, ws, n, g_sum, g_sq, weights, offsets ? 0 : bag, bag_of, nbags, lr,
                                  reinterpret_cast<float *>(tail), s);
    }
    uint64_t *keys = reinterpret_cast<uint64_t *>(tail);
    hipLaunchKernelGGL((wbag_mask_kernel<IdT>), dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, s, ids, weights, n,
                       (uint64_t)rows, (uint64_t)rows, keys);
    HA_LAUNCH_CHECK();
    if (ha_plan_sort_u64ids_lim(keys, n, ws, static_cast<uint64_t>(rows), stream))
        return -1;
    if (ha_plan_finish(ws, n, stream))
        return -1;
    return wfm_apply_launch(what, table, rows, width, ws, n, g_sum, g_sq, weights, offsets ? 0 : bag, bag_of, lr, s);
}

}  // namespace ha

extern "C" int ha_gather_wfm_f32ids(const float *table, int64_t rows, int64_t width, const float *ids, const float *weights,
                                    int64_t n, int64_t bag, const int64_t *offsets, int64_t nbags, float *out_sum, float *out_sq,
                                    ha_stream_t stream) {
    return ha::wfm_sum_launch<float>("ha_gather_wfm_f32ids", table, rows, width, ids, weights, n, bag, offsets, nbags, out_sum,
                                     out_sq, ha::as_stream(stream));
}

extern "C" int ha_gather_wfm_u64ids(const float *table, int64_t rows, int64_t width, const uint64_t *ids, const float *weights,
                                    int64_t n, int64_t bag, const int64_t *offsets, int64_t nbags, float *out_sum, float *out_sq,
                                    ha_stream_t stream) {
    return ha::wfm_sum_launch<uint64_t>("ha_gather_wfm_u64ids", table, rows, width, ids, weights, n, bag, offsets, nbags, out_sum,
                                        out_sq, ha::as_stream(stream));
}

extern "C" int ha_wfm_grad_rows(const float *g_sum, const float *g_sq, const float *weights, const float *emb_rows, int64_t n,
                                int64_t width, int64_t bag, const int32_t *bag_of, int64_t nbags, float *out, ha_stream_t stream) {
    return ha::wfm_grad_rows_launch("ha_wfm_grad_rows", g_sum, g_sq, weights, emb_rows, n, width, bag, bag_of, nbags, out,
                                    ha::as_stream(stream));
}

extern "C" int ha_sgd_apply_wfm_bags(float *table, int64_t rows, int64_t width, void *plan_ws, int64_t n, const float *g_sum,
                                     const float *g_sq, const float *weights, int64_t bag, const int32_t *bag_of, int64_t nbags,
                                     float lr, ha_stream_t stream) {
    return ha::wfm_apply("ha_sgd_apply_wfm_bags", table, rows, width, plan_ws, n, g_sum, g_sq, weights, bag, bag_of, nbags, lr,
                         ha::as_stream(stream));
}

extern "C" int ha_sgd_sparse_update_wfm_bags_f32ids(float *table, int64_t rows, int64_t width, const float *ids,
                                                    const float *weights, int64_t n, const float *g_sum, const float *g_sq,
                                                    int64_t bag, const int64_t *offsets, int64_t nbags, float lr,
                                                    ha_stream_t stream) {
    return ha::sgd_sparse_update_wfm_bags<float>("ha_sgd_sparse_update_wfm_bags_f32ids", table, rows, width, ids, weights, n,
                                                 g_sum, g_sq, bag, offsets, nbags, lr, stream);
}

extern "C" int ha_sgd_sparse_update_wfm_bags_u64ids(float *table, int64_t rows, int64_t width, const uint64_t *ids,
                                                    const float *weights, int64_t n, const float *g_sum, const float *g_sq,
                                                    int64_t bag, const int64_t *offsets, int64_t nbags, float lr,
                                                    ha_stream_t stream) {
    return ha::sgd_sparse_update_wfm_bags<uint64_t>("ha_sgd_sparse_update_wfm_bags_u64ids", table, rows, width, ids, weights, n,
                                                    g_sum, g_sq, bag, offsets, nbags, lr, stream);
}

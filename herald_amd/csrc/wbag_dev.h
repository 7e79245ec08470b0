// Device helpers shared by the weighted bags (wbag.hip), the weighted FM-pooled lookup (wfm.hip) and the weighted bags of the
// row-sharded table (wshard.hip): the vector types of their kernels, the launch constants, the bag of an occurrence, the masked
// keys of the one-call applies, and the weighted forward (kernel and launch: wshard.hip instantiates it for uint32 keys).
#pragma once
#include "gather_dev.h"
#include "plan_dev.h"

namespace ha {

template <int VEC>
struct WVec;
template <>
struct WVec<1> {
    typedef float T;
    static __device__ __forceinline__ float get(const T &v, int) { return v; }
    static __device__ __forceinline__ void set(T &v, int, float x) { v = x; }
};
template <>
struct WVec<2> {
    typedef float T __attribute__((ext_vector_type(2)));
    static __device__ __forceinline__ float get(const T &v, int k) { return v[k]; }
    static __device__ __forceinline__ void set(T &v, int k, float x) { v[k] = x; }
};
template <>
struct WVec<4> {
    typedef float4v T;
    static __device__ __forceinline__ float get(const T &v, int k) { return v[k]; }
    static __device__ __forceinline__ void set(T &v, int k, float x) { v[k] = x; }
};

constexpr int kWbagWaves = 4;         // waves per workgroup of the forward and of the short-run apply
constexpr int kWbagLongWaves = 16;
constexpr int kWbagCoopPerWave = 8;   // occurrences per wave and round of the cooperative path
constexpr int kWbagCoopRound = (kWbagLongWaves - 1) * kWbagCoopPerWave;      // wave 0 runs the chain only
constexpr int kWbagLongBlocks = 256;  // workgroups that loop over the (long key, slice) items: one per compute unit

// ---- masked keys of the one-call apply --------------------------------------------------------------------------------------
// keys[i] = the row number of a live occurrence, `dead` (>= rows) for a dead one.
template <typename IdT>
__global__ __launch_bounds__(256) void wbag_mask_kernel(const IdT *__restrict__ ids, const float *__restrict__ weights, int64_t n,
                                                        uint64_t rows, uint64_t dead, uint64_t *__restrict__ keys) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n)
        return;
    const uint64_t r = id_to_row<IdT>(ids[i]);
    keys[i] = (r < rows && weights[i] != 0.f) ? r : dead;
}

template <bool FIXED>
__device__ __forceinline__ int wbag_bag(int i, int bag, const int32_t *__restrict__ bag_of) {
    return FIXED ? i / bag : bag_of[i];
}

// ---- forward ---------------------------------------------------------------------------------------------------------------
// ROWS: table rows requested per round (all in flight before the first add).
template <typename IdT, int VEC, int ROWS>
__global__ __launch_bounds__(kWbagWaves *kWave) void wbag_sum_kernel(
    const float *__restrict__ table, uint64_t rows, uint32_t width, const IdT *__restrict__ ids,
    const float *__restrict__ weights, int64_t n, int64_t bag, const int64_t *__restrict__ offsets, int64_t nbags,
    uint32_t nslice, float *__restrict__ out) {
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
    V acc;
#pragma unroll
    for (int k = 0; k < VEC; ++k)
        WVec<VEC>::set(acc, k, 0.f);
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
            __builtin_amdgcn_sched_barrier(0);      // (as bag_sum_kernel: the whole round is requested before the first add)
#pragma unroll
            for (int t = 0; t < ROWS; ++t) {
                const int tt = c + t < cnt ? c + t : 0;                                    // wave-uniform
                const bool rok = c + t < cnt && ((okm >> tt) & 1ull) != 0;                 // a dead occurrence leaves acc alone
                const float wt = __int_as_float(__builtin_amdgcn_readlane(wbits, tt));
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const float a = WVec<VEC>::get(acc, k);
                    const float s = __fadd_rn(a, __fmul_rn(wt, WVec<VEC>::get(v[t], k)));
                    WVec<VEC>::set(acc, k, rok ? s : a);
                }
            }
        }
    }
    // the pooled rows are consumed by another kernel (the dense tower): written around the L2, as the gather's
    if (live)
        __builtin_nontemporal_store(acc, reinterpret_cast<V *>(out + static_cast<uint64_t>(b) * width + col));
}

// ---- host --------------------------------------------------------------------------------------------------------------------
// the argument rules of the apply's entry points and of ha_wbag_grad_rows; everything here precedes any device access
static inline int wbag_args_ok(const char *what, int64_t rows, int64_t width, int64_t n, int64_t bag, bool ragged, int64_t nbags) {
    HA_REQUIRE(rows >= 0 && width >= 1 && width < (1ll << 30) && n >= 0 && n < (1ll << 31) && nbags >= 0 && nbags < (1ll << 31) &&
                   bag >= 0 && bag < (1ll << 31),
               "%s: bad sizes rows=%ld width=%ld n=%ld bag=%ld nbags=%ld", what, (long)rows, (long)width, (long)n, (long)bag,
               (long)nbags);
    HA_REQUIRE((bag >= 1) != ragged, "%s: give exactly one of bag >= 1 and %s (bag=%ld)", what, "bag_of / offsets", (long)bag);
    HA_REQUIRE(ragged || (n % bag == 0 && n / bag == nbags), "%s: n=%ld is not nbags=%ld bags of bag=%ld ids", what, (long)n,
               (long)nbags, (long)bag);
    return 0;
}

template <typename IdT>
static int wbag_sum_launch(const char *what, const float *table, int64_t rows, int64_t width, const IdT *ids,
                           const float *weights, int64_t n, int64_t bag, const int64_t *offsets, int64_t nbags, float *out,
                           hipStream_t stream) {
    if (wbag_args_ok(what, rows, width, n, bag, offsets != nullptr, nbags))
        return -1;
    if (n == 0 && (nbags == 0 || out == nullptr))
        return 0;
    HA_REQUIRE(nbags >= 1, "%s: %ld ids in no bag", what, (long)n);
    HA_REQUIRE((table != nullptr || n == 0) && out != nullptr, "%s: null table or out", what);
    HA_REQUIRE((ids != nullptr && weights != nullptr) || n == 0, "%s: null ids or weights", what);
    if (rows == 0 || n == 0) {      // no live occurrence (and no row 0 for the clamped loads to read)
        HA_CHECK_HIP(hipMemsetAsync(out, 0, static_cast<size_t>(nbags) * width * sizeof(float), stream));
        return 0;
    }
    const bool vec_ok = (width % 4 == 0) && (reinterpret_cast<uintptr_t>(table) % 16 == 0) &&
                        (reinterpret_cast<uintptr_t>(out) % 16 == 0);
    // bagsum.hip's launch rule: the widest slice that is no wider than a row and still gives the chip 8 waves per compute unit
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
#define HA_WBAG_CASE(V, R)                                                                                                   \
    hipLaunchKernelGGL((wbag_sum_kernel<IdT, V, R>), grid, block, 0, stream, table, (uint64_t)rows, (uint32_t)width, ids,    \
                       weights, n, bag, offsets, nbags, nslice, out)
    if (vec == 4) {
        if (few) HA_WBAG_CASE(4, 8); else HA_WBAG_CASE(4, 32);
    } else if (vec == 2) {
        if (few) HA_WBAG_CASE(2, 8); else HA_WBAG_CASE(2, 32);
    } else {
        if (few) HA_WBAG_CASE(1, 8); else HA_WBAG_CASE(1, 32);
    }
#undef HA_WBAG_CASE
    HA_LAUNCH_CHECK();
    return 0;
}

}  // namespace ha

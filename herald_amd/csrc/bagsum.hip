// Sum-pooled embedding lookup ("EmbeddingBag", sum mode): out[b,:] = ((0.0f + r_0) + r_1) + ... + r_{m-1} over the table rows
// r_j of bag b's ids, in position order, one __fadd_rn per term.
//
// Replaces the pair embedding_lookup_op + reduce_sum_op(axes=1) of the reference's pooled CTR models
// (examples/ctr/models/emb_sum_wdl_criteo.py:14-16): the per-occurrence tensor [B, F, d] is never written.  The reference's
// reduction order is cuDNN's / numpy's and specified nowhere; the fixed order here makes the result reproducible and equal on
// every path of this project.  An id >= rows contributes a zero row (as the gather, gather_dev.h); an empty bag gives zeros.
//
// Bags.  Fixed: ids is [nbags, bag], occurrence i belongs to bag i / bag.  Ragged: offsets[nbags + 1] (int64, offsets[0] = 0,
// offsets[nbags] = n, non-decreasing); every offset is clamped to [0, n] and every bag's end to its start, so no id at or beyond
// n is read and no output row at or beyond nbags written, whatever offsets holds.
//
// MI355X layout.  One wave per (bag, column slice): the sum of a bag is an ordered chain per column, so a bag is split over waves
// by COLUMNS only (a 256-bag batch of 512-float rows would otherwise leave the chip nearly empty).  A wave fetches its bag's ids
// once -- lane l holds id l of the current block of 64 -- and broadcasts the row numbers with v_readlane; the row loads are
// branch-free (clamped addresses, see gather_dev.h) and ROWS of them are in flight before the first add.  The slice is 64 * VEC
// floats: VEC = 1 (256 bytes of a row per request, also the path of any width / alignment), 2 or 4 (1 KiB per request).
// Slices of one bag are adjacent waves, so its ids are served by the L1 / L2 after the first of them.
//
// Algorithmic bytes: n * (4 * width + 4) read + nbags * 4 * width written.
#include "gather_dev.h"

namespace ha {

template <int VEC>
struct BagVec;
template <>
struct BagVec<1> {
    typedef float T;
    static __device__ __forceinline__ float get(const T &v, int) { return v; }
    static __device__ __forceinline__ void set(T &v, int, float x) { v = x; }
};
template <>
struct BagVec<2> {
    typedef float T __attribute__((ext_vector_type(2)));
    static __device__ __forceinline__ float get(const T &v, int k) { return v[k]; }
    static __device__ __forceinline__ void set(T &v, int k, float x) { v[k] = x; }
};
template <>
struct BagVec<4> {
    typedef float4v T;
    static __device__ __forceinline__ float get(const T &v, int k) { return v[k]; }
    static __device__ __forceinline__ void set(T &v, int k, float x) { v[k] = x; }
};

constexpr int kBagWaves = 4;   // waves per workgroup

// ROWS: table rows requested per round (all in flight before the first add).
template <typename IdT, int VEC, int ROWS>
__global__ __launch_bounds__(kBagWaves *kWave) void bag_sum_kernel(
    const float *__restrict__ table, uint64_t rows, uint32_t width, const IdT *__restrict__ ids, int64_t n, int64_t bag,
    const int64_t *__restrict__ offsets, int64_t nbags, uint32_t nslice, float *__restrict__ out) {
    typedef typename BagVec<VEC>::T V;
    const int lane = lane_id();
    const uint64_t item = static_cast<uint64_t>(blockIdx.x) * kBagWaves + (threadIdx.x >> 6);   // wave-uniform
    if (item >= static_cast<uint64_t>(nbags) * nslice)
        return;
    const int64_t b = static_cast<int64_t>(item / nslice);
    const uint32_t sl = static_cast<uint32_t>(item - static_cast<uint64_t>(b) * nslice);
    int64_t lo, hi;
    if (offsets != nullptr) {
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
        BagVec<VEC>::set(acc, k, 0.f);
    for (int64_t j0 = lo; j0 < hi; j0 += kWave) {
        const int cnt = static_cast<int>(hi - j0 < kWave ? hi - j0 : kWave);      // ids of this block (wave-uniform)
        const int64_t j = j0 + (lane < cnt ? lane : cnt - 1);                      // lo <= j < hi <= n
        const uint64_t r = id_to_row<IdT>(ids[j]);
        const bool ok = r < rows;
        const unsigned long long okm = __ballot(ok);
        const uint64_t off = (ok ? r : 0) * width;          // float offset of the row (row 0 for an id beyond the table)
        const int off_lo = static_cast<int>(static_cast<uint32_t>(off));
        const int off_hi = static_cast<int>(static_cast<uint32_t>(off >> 32));
        for (int c = 0; c < cnt; c += ROWS) {
            V v[ROWS];
#pragma unroll
            for (int t = 0; t < ROWS; ++t) {
                const int tt = c + t < cnt ? c + t : cnt - 1;
                const uint64_t o = (static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readlane(off_hi, tt))) << 32) |
                                   static_cast<uint32_t>(__builtin_amdgcn_readlane(off_lo, tt));
                v[t] = *reinterpret_cast<const V *>(table + o + lcol);
            }
            // every request of the round is issued before the first add: the scheduler would otherwise interleave them (about ten
            // rows in flight instead of ROWS, three round trips for a bag of 26 instead of one)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < ROWS; ++t) {
                const bool in = c + t < cnt;                                  // wave-uniform
                const bool rok = ((okm >> (in ? c + t : 0)) & 1ull) != 0;     // an id beyond the table adds a zero row
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const float a = BagVec<VEC>::get(acc, k);
                    const float s = __fadd_rn(a, rok ? BagVec<VEC>::get(v[t], k) : 0.f);
                    BagVec<VEC>::set(acc, k, in ? s : a);
                }
            }
        }
    }
    // the pooled rows are consumed by another kernel (the dense tower): written around the L2, as the gather's
    if (live)
        __builtin_nontemporal_store(acc, reinterpret_cast<V *>(out + static_cast<uint64_t>(b) * width + col));
}

// The same sum over TWO sources (the sized expand of the sharded step, ha_gather2_u32map, fused with the sum over each bag): lane
// l holds the map word of position l of the block and forms the ADDRESS of its row -- table[map & 0x7FFFFFFF] if bit 31 is set
// (a key of this rank's own shard), recv[map] otherwise (a row an owner sent); an index beyond its array is clamped to row 0 of
// its array and adds a zero row (0xFFFFFFFF is one) -- and the address is what v_readlane broadcasts.  Everything else is
// bag_sum_kernel's: one wave per (bag, column slice), ROWS branch-free loads in flight before the first add, the same chain.
// The host gives a side without rows the other side's pointer, so the clamped loads always read memory that exists.
template <int VEC, int ROWS>
__global__ __launch_bounds__(kBagWaves *kWave) void bag_sum2_kernel(
    const float *table, uint64_t rows, const float *recv, uint64_t recv_rows, uint32_t width, const uint32_t *__restrict__ map,
    int64_t n, int64_t bag, const int64_t *__restrict__ offsets, int64_t nbags, uint32_t nslice, float *__restrict__ out) {
    typedef typename BagVec<VEC>::T V;
    const int lane = lane_id();
    const uint64_t item = static_cast<uint64_t>(blockIdx.x) * kBagWaves + (threadIdx.x >> 6);   // wave-uniform
    if (item >= static_cast<uint64_t>(nbags) * nslice)
        return;
    const int64_t b = static_cast<int64_t>(item / nslice);
    const uint32_t sl = static_cast<uint32_t>(item - static_cast<uint64_t>(b) * nslice);
    int64_t lo, hi;
    if (offsets != nullptr) {
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
        BagVec<VEC>::set(acc, k, 0.f);
    for (int64_t j0 = lo; j0 < hi; j0 += kWave) {
        const int cnt = static_cast<int>(hi - j0 < kWave ? hi - j0 : kWave);      // positions of this block (wave-uniform)
        const int64_t j = j0 + (lane < cnt ? lane : cnt - 1);                      // lo <= j < hi <= n
        const uint32_t m = map[j];
        const bool own = (m & 0x80000000u) != 0;
        const uint64_t r = m & 0x7FFFFFFFu;
        const bool ok = r < (own ? rows : recv_rows);
        const unsigned long long okm = __ballot(ok);
        const uint64_t src = reinterpret_cast<uint64_t>((own ? table : recv) + (ok ? r : 0) * width);
        const int src_lo = static_cast<int>(static_cast<uint32_t>(src));
        const int src_hi = static_cast<int>(static_cast<uint32_t>(src >> 32));
        for (int c = 0; c < cnt; c += ROWS) {
            V v[ROWS];
#pragma unroll
            for (int t = 0; t < ROWS; ++t) {
                const int tt = c + t < cnt ? c + t : cnt - 1;
                const uint64_t a = (static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readlane(src_hi, tt))) << 32) |
                                   static_cast<uint32_t>(__builtin_amdgcn_readlane(src_lo, tt));
                v[t] = *reinterpret_cast<const V *>(reinterpret_cast<const float *>(a) + lcol);
            }
            __builtin_amdgcn_sched_barrier(0);      // (as bag_sum_kernel: the whole round is requested before the first add)
#pragma unroll
            for (int t = 0; t < ROWS; ++t) {
                const bool in = c + t < cnt;                                  // wave-uniform
                const bool rok = ((okm >> (in ? c + t : 0)) & 1ull) != 0;     // an index beyond its array adds a zero row
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const float a = BagVec<VEC>::get(acc, k);
                    const float s = __fadd_rn(a, rok ? BagVec<VEC>::get(v[t], k) : 0.f);
                    BagVec<VEC>::set(acc, k, in ? s : a);
                }
            }
        }
    }
    if (live)
        __builtin_nontemporal_store(acc, reinterpret_cast<V *>(out + static_cast<uint64_t>(b) * width + col));
}

// FM-pooled lookup (the DeepFM models, examples/ctr/models/deepfm_criteo.py:24-39): one lookup consumed three ways -- as rows
// (the DNN), as S = sum over the bag and as Q = sum of squares over the bag, combined into 0.5 * (S*S - Q).  bag_sum_kernel
// with a second accumulator and a row store: per (bag, column)
//   S  = ((0.0f + r_0) + r_1) + ...                    the chain of bag_sum_kernel, so out_sum is its output bit for bit
//   Q  = ((0.0f + fl(r_0*r_0)) + fl(r_1*r_1)) + ...    one __fmul_rn and one __fadd_rn per term
//   fm = fl(0.5f * fl(fl(S*S) - Q))                    three roundings, nothing contracted
// and out_rows[i,:] = the row of occurrence i (zeros for an id beyond the table), written around the L2 as the gather's; a
// null out_rows skips the store (the caller already holds the rows: the table IS its row buffer).  Every slice wave of a bag
// stores its own columns of the bag's rows, so the rows are read once and written once: n * (8 * width + 4) bytes.
// Registers (ROWS = 32, VEC = 4): 128 for the round's rows, 8 for the two accumulators -- see DESIGN.md for the compiler's
// counts; no instantiation spills.
template <typename IdT, int VEC, int ROWS>
__global__ __launch_bounds__(kBagWaves *kWave) void bag_fm_kernel(
    const float *__restrict__ table, uint64_t rows, uint32_t width, const IdT *__restrict__ ids, int64_t n, int64_t bag,
    const int64_t *__restrict__ offsets, int64_t nbags, uint32_t nslice, float *__restrict__ out_rows,
    float *__restrict__ out_sum, float *__restrict__ out_fm) {
    typedef typename BagVec<VEC>::T V;
    const int lane = lane_id();
    const uint64_t item = static_cast<uint64_t>(blockIdx.x) * kBagWaves + (threadIdx.x >> 6);   // wave-uniform
    if (item >= static_cast<uint64_t>(nbags) * nslice)
        return;
    const int64_t b = static_cast<int64_t>(item / nslice);
    const uint32_t sl = static_cast<uint32_t>(item - static_cast<uint64_t>(b) * nslice);
    int64_t lo, hi;
    if (offsets != nullptr) {
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
    const bool store_rows = out_rows != nullptr;      // wave-uniform
    V acc, sq;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        BagVec<VEC>::set(acc, k, 0.f);
        BagVec<VEC>::set(sq, k, 0.f);
    }
    for (int64_t j0 = lo; j0 < hi; j0 += kWave) {
        const int cnt = static_cast<int>(hi - j0 < kWave ? hi - j0 : kWave);      // ids of this block (wave-uniform)
        const int64_t j = j0 + (lane < cnt ? lane : cnt - 1);                      // lo <= j < hi <= n
        const uint64_t r = id_to_row<IdT>(ids[j]);
        const bool ok = r < rows;
        const unsigned long long okm = __ballot(ok);
        const uint64_t off = (ok ? r : 0) * width;          // float offset of the row (row 0 for an id beyond the table)
        const int off_lo = static_cast<int>(static_cast<uint32_t>(off));
        const int off_hi = static_cast<int>(static_cast<uint32_t>(off >> 32));
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
                const bool in = c + t < cnt;                                  // wave-uniform
                const bool rok = ((okm >> (in ? c + t : 0)) & 1ull) != 0;     // an id beyond the table is a zero row
                V row;
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const float x = rok ? BagVec<VEC>::get(v[t], k) : 0.f;
                    BagVec<VEC>::set(row, k, x);
                    const float a = BagVec<VEC>::get(acc, k);
                    const float q = BagVec<VEC>::get(sq, k);
                    const float s = __fadd_rn(a, x);
                    const float p = __fadd_rn(q, __fmul_rn(x, x));
                    BagVec<VEC>::set(acc, k, in ? s : a);
                    BagVec<VEC>::set(sq, k, in ? p : q);
                }
                if (store_rows && in && live)      // occurrence j0 + c + t < hi <= n
                    __builtin_nontemporal_store(
                        row, reinterpret_cast<V *>(out_rows + static_cast<uint64_t>(j0 + c + t) * width + col));
            }
        }
    }
    if (live) {
        V fm;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const float s = BagVec<VEC>::get(acc, k);
            BagVec<VEC>::set(fm, k, __fmul_rn(0.5f, __fsub_rn(__fmul_rn(s, s), BagVec<VEC>::get(sq, k))));
        }
        __builtin_nontemporal_store(acc, reinterpret_cast<V *>(out_sum + static_cast<uint64_t>(b) * width + col));
        __builtin_nontemporal_store(fm, reinterpret_cast<V *>(out_fm + static_cast<uint64_t>(b) * width + col));
    }
}

// The per-occurrence gradient of the FM-pooled lookup, one elementwise launch:
//   out[i,c] = fl( fl(g_rows[i,c] + fl(g_fm[b,c] * sum[b,c])) - fl(g_fm[b,c] * emb_rows[i,c]) ),   b = the bag of i
// (g_rows null: out = fl(fl(g_fm*sum) - fl(g_fm*emb_rows))).  The lookup's output has three consumers -- the rows, S and Q --
// and the reference's executor adds their adjoints g_rows, g_fm*S and -g_fm*e in its topological order, which is specified
// nowhere; the order above is this project's fixed one, as the bag sum's is.  out may alias g_rows: a thread reads its own
// elements before it writes them.  A thread handles one vector of VEC floats; nv = width / VEC.
template <int VEC>
__global__ __launch_bounds__(256) void fm_grad_rows_kernel(const float *g_rows, const float *__restrict__ emb_rows,
                                                           const float *__restrict__ sum, const float *__restrict__ g_fm,
                                                           uint64_t total_vec, uint32_t nv, uint32_t bag,
                                                           const int32_t *__restrict__ bag_of, uint32_t nbags, float *out) {
    typedef typename BagVec<VEC>::T V;
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
    b = b < nbags ? b : nbags - 1;       // (ha_bag_of's entries are in [0, nbags): no row beyond sum / g_fm is read whatever bag_of holds)
    const uint64_t bo = (static_cast<uint64_t>(b) * nv + cv) * VEC;
    const V ev = *reinterpret_cast<const V *>(emb_rows + e * VEC);
    const V sv = *reinterpret_cast<const V *>(sum + bo);
    const V gf = *reinterpret_cast<const V *>(g_fm + bo);
    V gr = sv;      // (not used without g_rows)
    if (g_rows != nullptr)
        gr = *reinterpret_cast<const V *>(g_rows + e * VEC);
    V o;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const float f = BagVec<VEC>::get(gf, k);
        float a = __fmul_rn(f, BagVec<VEC>::get(sv, k));
        if (g_rows != nullptr)
            a = __fadd_rn(BagVec<VEC>::get(gr, k), a);
        BagVec<VEC>::set(o, k, __fsub_rn(a, __fmul_rn(f, BagVec<VEC>::get(ev, k))));
    }
    *reinterpret_cast<V *>(out + e * VEC) = o;
}

// bag_of[i] = the bag of occurrence i: the largest b in [0, nbags) with offsets[b] <= i (empty bags are skipped).  Always in
// [0, nbags), whatever offsets holds; offsets[0] and offsets[nbags] are not read.
__global__ __launch_bounds__(256) void bag_of_kernel(const int64_t *__restrict__ offsets, int nbags, int64_t n,
                                                     int32_t *__restrict__ bag_of) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n)
        return;
    int lo = 0, hi = nbags;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= i)
            lo = mid;
        else
            hi = mid;
    }
    bag_of[i] = lo;
}

// Slice width of the 16-byte path in floats: 0 = by the rule in bag_sum_launch, else 64 / 128 / 256 (ha_debug_bag_slice).
static int g_bag_slice = 0;

// The launch rule of the bag sums (both kernels): column slice, grid and rows per round of a batch.
struct BagLaunchRule {
    int vec;
    uint32_t nslice;
    unsigned blocks;
    bool few;
};
static int bag_launch_rule(const char *what, bool vec_ok, int64_t width, int64_t n, int64_t bag, const int64_t *offsets,
                           int64_t nbags, BagLaunchRule *r) {
    // Slice of the 16-byte path: the widest one that is no wider than a row and still gives the chip 8 waves per compute unit
    // (2,048 waves); batches too small for that take 64-float slices.  (256 bags of 26 x 512 floats: 2,048 waves of 64 floats;
    // 4,096 bags of 128 floats: 4,096 waves of 128 floats.  Not measured yet: docs/EXPERIMENTS.md round 6 section 18.)
    int vec = 1;
    if (vec_ok) {
        if (g_bag_slice != 0) {
            vec = g_bag_slice / kWave;
        } else {
            for (vec = 4; vec > 1; vec >>= 1)
                if (kWave * vec <= width && nbags * ((width + kWave * vec - 1) / (kWave * vec)) >= 2048)
                    break;
        }
    }
    r->nslice = static_cast<uint32_t>((width + kWave * vec - 1) / (kWave * vec));
    const uint64_t blocks64 = (static_cast<uint64_t>(nbags) * r->nslice + kBagWaves - 1) / kBagWaves;
    HA_REQUIRE(blocks64 < (1ull << 31), "%s: batch too large", what);
    // rows per round by the (mean) bag size: a bag of 26 is one round of 32 requests
    const int64_t mean = offsets ? (n + nbags - 1) / nbags : bag;
    r->few = mean <= 8;
    r->blocks = static_cast<unsigned>(blocks64);
    r->vec = vec;
    return 0;
}

template <typename IdT>
static int bag_sum_launch(const char *what, const float *table, int64_t rows, int64_t width, const IdT *ids, int64_t n,
                          int64_t bag, const int64_t *offsets, int64_t nbags, float *out, hipStream_t stream) {
    HA_REQUIRE(rows >= 0 && width >= 1 && width < (1ll << 30) && n >= 0 && nbags >= 0 && bag >= 0,
               "%s: bad sizes rows=%ld width=%ld n=%ld bag=%ld nbags=%ld", what, (long)rows, (long)width, (long)n, (long)bag,
               (long)nbags);
    HA_REQUIRE((bag >= 1) != (offsets != nullptr), "%s: give exactly one of bag >= 1 and offsets (bag=%ld, offsets %s)", what,
               (long)bag, offsets ? "given" : "null");
    HA_REQUIRE(offsets != nullptr || (n % bag == 0 && n / bag == nbags), "%s: n=%ld is not nbags=%ld bags of bag=%ld ids", what,
               (long)n, (long)nbags, (long)bag);
    if (nbags == 0)
        return 0;
    HA_REQUIRE(table != nullptr, "%s: null table", what);
    HA_REQUIRE(out != nullptr && (ids != nullptr || n == 0), "%s: null pointer", what);
    if (rows == 0) {      // every id is beyond the table (and there is no row 0 for the clamped loads to read)
        HA_CHECK_HIP(hipMemsetAsync(out, 0, static_cast<size_t>(nbags) * width * sizeof(float), stream));
        return 0;
    }
    const bool vec_ok = (width % 4 == 0) && (reinterpret_cast<uintptr_t>(table) % 16 == 0) &&
                        (reinterpret_cast<uintptr_t>(out) % 16 == 0);
    BagLaunchRule lr;
    if (bag_launch_rule(what, vec_ok, width, n, bag, offsets, nbags, &lr))
        return -1;
    const int vec = lr.vec;
    const uint32_t nslice = lr.nslice;
    const bool few = lr.few;
    const dim3 grid(lr.blocks), block(kBagWaves * kWave);
#define HA_BAG_CASE(V, R)                                                                                               \
    hipLaunchKernelGGL((bag_sum_kernel<IdT, V, R>), grid, block, 0, stream, table, (uint64_t)rows, (uint32_t)width, ids, n, \
                       bag, offsets, nbags, nslice, out)
    if (vec == 4) {
        if (few) HA_BAG_CASE(4, 8); else HA_BAG_CASE(4, 32);
    } else if (vec == 2) {
        if (few) HA_BAG_CASE(2, 8); else HA_BAG_CASE(2, 32);
    } else {
        if (few) HA_BAG_CASE(1, 8); else HA_BAG_CASE(1, 32);
    }
#undef HA_BAG_CASE
    HA_LAUNCH_CHECK();
    return 0;
}

// ha_gather2_sum_u32map: every check of bag_sum_launch and of ha_gather2_u32map, before any device access.
static int bag_sum2_launch(const float *table, int64_t rows, const float *recv, int64_t recv_rows, int64_t width,
                           const uint32_t *map, int64_t n, int64_t bag, const int64_t *offsets, int64_t nbags, float *out,
                           hipStream_t stream) {
    const char *what = "ha_gather2_sum_u32map";
    HA_REQUIRE(rows >= 0 && recv_rows >= 0 && width >= 1 && width < (1ll << 30) && n >= 0 && nbags >= 0 && bag >= 0,
               "%s: bad sizes rows=%ld recv_rows=%ld width=%ld n=%ld bag=%ld nbags=%ld", what, (long)rows, (long)recv_rows,
               (long)width, (long)n, (long)bag, (long)nbags);
    HA_REQUIRE((bag >= 1) != (offsets != nullptr), "%s: give exactly one of bag >= 1 and offsets (bag=%ld, offsets %s)", what,
               (long)bag, offsets ? "given" : "null");
    HA_REQUIRE(offsets != nullptr || (n % bag == 0 && n / bag == nbags), "%s: n=%ld is not nbags=%ld bags of bag=%ld ids", what,
               (long)n, (long)nbags, (long)bag);
    if (nbags == 0)
        return 0;
    HA_REQUIRE(out != nullptr && (map != nullptr || n == 0) && (table != nullptr || rows == 0) &&
                   (recv != nullptr || recv_rows == 0), "%s: null pointer", what);
    // a side that has no rows is never dereferenced: its clamped loads read row 0 of the other side (and add zeros)
    if (rows == 0) table = recv;
    if (recv_rows == 0) recv = table;
    if (rows == 0 && recv_rows == 0) {      // every index is beyond its array
        HA_CHECK_HIP(hipMemsetAsync(out, 0, static_cast<size_t>(nbags) * width * sizeof(float), stream));
        return 0;
    }
    const bool vec_ok = (width % 4 == 0) && (reinterpret_cast<uintptr_t>(table) % 16 == 0) &&
                        (reinterpret_cast<uintptr_t>(recv) % 16 == 0) && (reinterpret_cast<uintptr_t>(out) % 16 == 0);
    BagLaunchRule lr;
    if (bag_launch_rule(what, vec_ok, width, n, bag, offsets, nbags, &lr))
        return -1;
    const dim3 grid(lr.blocks), block(kBagWaves * kWave);
#define HA_BAG2_CASE(V, R)                                                                                              \
    hipLaunchKernelGGL((bag_sum2_kernel<V, R>), grid, block, 0, stream, table, (uint64_t)rows, recv, (uint64_t)recv_rows, \
                       (uint32_t)width, map, n, bag, offsets, nbags, lr.nslice, out)
    if (lr.vec == 4) {
        if (lr.few) HA_BAG2_CASE(4, 8); else HA_BAG2_CASE(4, 32);
    } else if (lr.vec == 2) {
        if (lr.few) HA_BAG2_CASE(2, 8); else HA_BAG2_CASE(2, 32);
    } else {
        if (lr.few) HA_BAG2_CASE(1, 8); else HA_BAG2_CASE(1, 32);
    }
#undef HA_BAG2_CASE
    HA_LAUNCH_CHECK();
    return 0;
}

// ha_gather_fm_*: the checks of bag_sum_launch (before any device access), the same launch rule and rows per round.
template <typename IdT>
static int bag_fm_launch(const char *what, const float *table, int64_t rows, int64_t width, const IdT *ids, int64_t n,
                         int64_t bag, const int64_t *offsets, int64_t nbags, float *out_rows, float *out_sum, float *out_fm,
                         hipStream_t stream) {
    HA_REQUIRE(rows >= 0 && width >= 1 && width < (1ll << 30) && n >= 0 && nbags >= 0 && bag >= 0,
               "%s: bad sizes rows=%ld width=%ld n=%ld bag=%ld nbags=%ld", what, (long)rows, (long)width, (long)n, (long)bag,
               (long)nbags);
    HA_REQUIRE((bag >= 1) != (offsets != nullptr), "%s: give exactly one of bag >= 1 and offsets (bag=%ld, offsets %s)", what,
               (long)bag, offsets ? "given" : "null");
    HA_REQUIRE(offsets != nullptr || (n % bag == 0 && n / bag == nbags), "%s: n=%ld is not nbags=%ld bags of bag=%ld ids", what,
               (long)n, (long)nbags, (long)bag);
    HA_REQUIRE(nbags == 0 || (out_sum != nullptr && out_fm != nullptr), "%s: null out_sum or out_fm", what);
    if (nbags == 0)
        return 0;
    HA_REQUIRE(table != nullptr, "%s: null table", what);
    HA_REQUIRE(ids != nullptr || n == 0, "%s: null ids", what);
    const size_t pooled_bytes = static_cast<size_t>(nbags) * width * sizeof(float);
    if (rows == 0) {      // every id is beyond the table (and there is no row 0 for the clamped loads to read)
        HA_CHECK_HIP(hipMemsetAsync(out_sum, 0, pooled_bytes, stream));
        HA_CHECK_HIP(hipMemsetAsync(out_fm, 0, pooled_bytes, stream));
        if (out_rows != nullptr && n > 0)
            HA_CHECK_HIP(hipMemsetAsync(out_rows, 0, static_cast<size_t>(n) * width * sizeof(float), stream));
        return 0;
    }
    // (ragged bags: an occurrence outside every clamped bag belongs to no bag -- offsets[0] > 0, offsets[nbags] < n -- and
    // its row is not written)
    const bool vec_ok = (width % 4 == 0) && (reinterpret_cast<uintptr_t>(table) % 16 == 0) &&
                        (reinterpret_cast<uintptr_t>(out_sum) % 16 == 0) && (reinterpret_cast<uintptr_t>(out_fm) % 16 == 0) &&
                        (reinterpret_cast<uintptr_t>(out_rows) % 16 == 0);
    BagLaunchRule lr;
    if (bag_launch_rule(what, vec_ok, width, n, bag, offsets, nbags, &lr))
        return -1;
    const dim3 grid(lr.blocks), block(kBagWaves * kWave);
#define HA_FM_CASE(V, R)                                                                                               \
    hipLaunchKernelGGL((bag_fm_kernel<IdT, V, R>), grid, block, 0, stream, table, (uint64_t)rows, (uint32_t)width, ids, n, \
                       bag, offsets, nbags, lr.nslice, out_rows, out_sum, out_fm)
    if (lr.vec == 4) {
        if (lr.few) HA_FM_CASE(4, 8); else HA_FM_CASE(4, 32);
    } else if (lr.vec == 2) {
        if (lr.few) HA_FM_CASE(2, 8); else HA_FM_CASE(2, 32);
    } else {
        if (lr.few) HA_FM_CASE(1, 8); else HA_FM_CASE(1, 32);
    }
#undef HA_FM_CASE
    HA_LAUNCH_CHECK();
    return 0;
}

static int fm_grad_rows_launch(const float *g_rows, const float *emb_rows, const float *sum, const float *g_fm, int64_t n,
                               int64_t width, int64_t bag, const int32_t *bag_of, int64_t nbags, float *out,
                               hipStream_t stream) {
    const char *what = "ha_fm_grad_rows";
    HA_REQUIRE(n >= 0 && n < (1ll << 31) && width >= 1 && width < (1ll << 30) && bag >= 0 && nbags >= 0 && nbags < (1ll << 31),
               "%s: bad sizes n=%ld width=%ld bag=%ld nbags=%ld", what, (long)n, (long)width, (long)bag, (long)nbags);
    HA_REQUIRE((bag >= 1) != (bag_of != nullptr), "%s: give exactly one of bag >= 1 and bag_of (bag=%ld, bag_of %s)", what,
               (long)bag, bag_of ? "given" : "null");
    HA_REQUIRE(bag_of != nullptr || (n % bag == 0 && n / bag == nbags), "%s: n=%ld is not nbags=%ld bags of bag=%ld ids", what,
               (long)n, (long)nbags, (long)bag);
    if (n == 0)
        return 0;
    HA_REQUIRE(nbags >= 1, "%s: %ld occurrences in no bag", what, (long)n);
    HA_REQUIRE(emb_rows && sum && g_fm && out, "%s: null pointer", what);
    HA_REQUIRE(out != emb_rows && out != sum && out != g_fm, "%s: out may alias g_rows only", what);
    const bool vec_ok = (width % 4 == 0) &&
                        ((reinterpret_cast<uintptr_t>(g_rows) | reinterpret_cast<uintptr_t>(emb_rows) |
                          reinterpret_cast<uintptr_t>(sum) | reinterpret_cast<uintptr_t>(g_fm) |
                          reinterpret_cast<uintptr_t>(out)) % 16 == 0);
    const int vec = vec_ok ? 4 : 1;
    const uint64_t total_vec = static_cast<uint64_t>(n) * static_cast<uint64_t>(width / vec);
    const uint64_t blocks64 = (total_vec + 255) / 256;      // sized by the work: n * width elements
    HA_REQUIRE(blocks64 < (1ull << 31), "%s: batch too large", what);
    const dim3 grid(static_cast<unsigned>(blocks64)), block(256);
    if (vec == 4)
        hipLaunchKernelGGL((fm_grad_rows_kernel<4>), grid, block, 0, stream, g_rows, emb_rows, sum, g_fm, total_vec,
                           (uint32_t)(width / 4), (uint32_t)bag, bag_of, (uint32_t)nbags, out);
    else
        hipLaunchKernelGGL((fm_grad_rows_kernel<1>), grid, block, 0, stream, g_rows, emb_rows, sum, g_fm, total_vec,
                           (uint32_t)width, (uint32_t)bag, bag_of, (uint32_t)nbags, out);
    HA_LAUNCH_CHECK();
    return 0;
}

int scratch_get(hipStream_t stream, size_t bytes, void **out);   // capi.hip

template <typename IdT>
static int sgd_sparse_update_bags(const char *what, float *table, int64_t rows, int64_t width, const IdT *ids, int64_t n,
                                  const float *bag_grads, int64_t bag, const int64_t *offsets, int64_t nbags, float lr,
                                  ha_stream_t stream) {
    HA_REQUIRE(rows >= 0 && width >= 1 && width < (1ll << 30) && n >= 0 && n < (1ll << 31) && nbags >= 0 && bag >= 0 &&
                   nbags < (1ll << 31),
               "%s: bad sizes rows=%ld width=%ld n=%ld bag=%ld nbags=%ld", what, (long)rows, (long)width, (long)n, (long)bag,
               (long)nbags);
    HA_REQUIRE((bag >= 1) != (offsets != nullptr), "%s: give exactly one of bag >= 1 and offsets (bag=%ld)", what, (long)bag);
    HA_REQUIRE(offsets != nullptr || (n % bag == 0 && n / bag == nbags), "%s: n=%ld is not nbags=%ld bags of bag=%ld ids", what,
               (long)n, (long)nbags, (long)bag);
    if (n == 0)
        return 0;
    HA_REQUIRE(table && ids && bag_grads && nbags >= 1, "%s: null pointer or no bags", what);
    const size_t plan_bytes = align_up(ha_plan_bytes(n), 256);
    void *ws = nullptr;
    if (scratch_get(as_stream(stream), plan_bytes + (offsets ? static_cast<size_t>(n) * 4 : 0), &ws))
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
    return ha_sgd_apply_bags(table, rows, width, ws, n, bag_grads, offsets ? 0 : bag, bag_of, lr, stream);
}

}  // namespace ha

extern "C" int ha_gather_sum_f32ids(const float *table, int64_t rows, int64_t width, const float *ids, int64_t n, int64_t bag,
                                    const int64_t *offsets, int64_t nbags, float *out, ha_stream_t stream) {
    return ha::bag_sum_launch<float>("ha_gather_sum_f32ids", table, rows, width, ids, n, bag, offsets, nbags, out,
                                     ha::as_stream(stream));
}

extern "C" int ha_gather_sum_u64ids(const float *table, int64_t rows, int64_t width, const uint64_t *ids, int64_t n, int64_t bag,
                                    const int64_t *offsets, int64_t nbags, float *out, ha_stream_t stream) {
    return ha::bag_sum_launch<uint64_t>("ha_gather_sum_u64ids", table, rows, width, ids, n, bag, offsets, nbags, out,
                                        ha::as_stream(stream));
}

extern "C" int ha_gather_fm_f32ids(const float *table, int64_t rows, int64_t width, const float *ids, int64_t n, int64_t bag,
                                   const int64_t *offsets, int64_t nbags, float *out_rows, float *out_sum, float *out_fm,
                                   ha_stream_t stream) {
    return ha::bag_fm_launch<float>("ha_gather_fm_f32ids", table, rows, width, ids, n, bag, offsets, nbags, out_rows, out_sum,
                                    out_fm, ha::as_stream(stream));
}

extern "C" int ha_gather_fm_u64ids(const float *table, int64_t rows, int64_t width, const uint64_t *ids, int64_t n, int64_t bag,
                                   const int64_t *offsets, int64_t nbags, float *out_rows, float *out_sum, float *out_fm,
                                   ha_stream_t stream) {
    return ha::bag_fm_launch<uint64_t>("ha_gather_fm_u64ids", table, rows, width, ids, n, bag, offsets, nbags, out_rows, out_sum,
                                       out_fm, ha::as_stream(stream));
}

extern "C" int ha_fm_grad_rows(const float *g_rows, const float *emb_rows, const float *sum, const float *g_fm, int64_t n,
                               int64_t width, int64_t bag, const int32_t *bag_of, int64_t nbags, float *out,
                               ha_stream_t stream) {
    return ha::fm_grad_rows_launch(g_rows, emb_rows, sum, g_fm, n, width, bag, bag_of, nbags, out, ha::as_stream(stream));
}

// ha_gather_sum_* over a buffer of rows named by uint32 keys held in device memory (the sharded store's pull: rows_buf = the unique rows
// a batch received, keys = its plan's inverse[n]) -- the expand to [n, width] and the sum over it in one pass.
extern "C" int ha_gather_sum_u32keys(const float *rows_buf, int64_t rows, int64_t width, const uint32_t *keys, int64_t n,
                                     int64_t bag, const int64_t *offsets, int64_t nbags, float *out, ha_stream_t stream) {
    return ha::bag_sum_launch<uint32_t>("ha_gather_sum_u32keys", rows_buf, rows, width, keys, n, bag, offsets, nbags, out,
                                        ha::as_stream(stream));
}

// The sized expand of the sharded step and the sum over each bag in one pass: position i's row is the one ha_gather2_u32map
// writes for it (own shard / received rows / zeros), out[b,:] the position-ordered chain over bag b (csrc/shard.hip).
extern "C" int ha_gather2_sum_u32map(const float *table, int64_t rows, const float *recv, int64_t recv_rows, int64_t width,
                                     const uint32_t *map, int64_t n, int64_t bag, const int64_t *offsets, int64_t nbags,
                                     float *out, ha_stream_t stream) {
    return ha::bag_sum2_launch(table, rows, recv, recv_rows, width, map, n, bag, offsets, nbags, out, ha::as_stream(stream));
}

extern "C" int ha_bag_of(const int64_t *offsets, int64_t nbags, int64_t n, int32_t *bag_of, ha_stream_t stream) {
    HA_REQUIRE(nbags >= 0 && n >= 0 && nbags < (1ll << 31) && n < (1ll << 31), "ha_bag_of: bad sizes nbags=%ld n=%ld",
               (long)nbags, (long)n);
    if (n == 0)
        return 0;
    HA_REQUIRE(nbags >= 1, "ha_bag_of: %ld ids in no bag", (long)n);
    HA_REQUIRE(offsets && bag_of, "ha_bag_of: null pointer");
    hipLaunchKernelGGL(ha::bag_of_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, ha::as_stream(stream),
                       offsets, static_cast<int>(nbags), n, bag_of);
    HA_LAUNCH_CHECK();
    return 0;
}

extern "C" int ha_sgd_sparse_update_bags_f32ids(float *table, int64_t rows, int64_t width, const float *ids, int64_t n,
                                                const float *bag_grads, int64_t bag, const int64_t *offsets, int64_t nbags,
                                                float lr, ha_stream_t stream) {
    return ha::sgd_sparse_update_bags<float>("ha_sgd_sparse_update_bags_f32ids", table, rows, width, ids, n, bag_grads, bag,
                                             offsets, nbags, lr, stream);
}

extern "C" int ha_sgd_sparse_update_bags_u64ids(float *table, int64_t rows, int64_t width, const uint64_t *ids, int64_t n,
                                                const float *bag_grads, int64_t bag, const int64_t *offsets, int64_t nbags,
                                                float lr, ha_stream_t stream) {
    return ha::sgd_sparse_update_bags<uint64_t>("ha_sgd_sparse_update_bags_u64ids", table, rows, width, ids, n, bag_grads, bag,
                                                offsets, nbags, lr, stream);
}

extern "C" int ha_debug_bag_slice(int floats) {
    HA_REQUIRE(floats == 0 || floats == 64 || floats == 128 || floats == 256,
               "ha_debug_bag_slice: 0 (automatic), 64, 128 or 256 floats");
    ha::g_bag_slice = floats;
    return 0;
}

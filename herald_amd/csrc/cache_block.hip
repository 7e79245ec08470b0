// The PLANNED flow of the HET embedding cache: LRU / LFU / LFUOpt, local store, the ids of a block of batches known a block early.
//
// Reference flows (src/hetu_cache/src/cache.cc): _embeddingLookup :60-107 and _embeddingUpdate :132-197 of the SAME keys,
// batch after batch -- what a training loop does (python/hetu/cstable.py:38-56: embedding_lookup, the model, embedding_update).
// Policies: LRUCache (src/hetu_cache/src/lru_cache.cc:5-39), LFUCache (src/lfu_cache.cc:9-70), LFUOptCache
// (src/lfuopt_cache.cc:9-71; their bookkeeping: cache_book_lfu_kernel below).  Line::accumulate (include/embedding.h:78-91), Line::addup (:92-96),
// the server's handlers (ps-lite/src/PSFhandle_embedding.cc:5-64).  Results: those of ha_cache_lookup + ha_cache_update_same_keys
// call by call (rows, versions, update counters, resident set, server table and versions; tests/test_gpu_cache_planned.py holds
// both to oracle/cache_model.py).
//
// What is different is WHEN the bookkeeping happens.  Which lines a batch hits, which it misses, which slots the misses get,
// which lines are evicted for them, how many updates a line has collected and whether it is pushed -- all of it follows from the
// IDS alone (the stamps of an LRU list, update counters, a free-slot stack), none of it from a row.  So, as the work-queue step
// does for the headline (csrc/qstep.hip), the bookkeeping of a BLOCK of up to 16 batches runs ahead, on a side stream, beside the
// rows of the block before:
//
//   ha_cache_plan_block     side stream: the index plans of the block's batches (two launches: stable sort, finish) and ONE
//                           bookkeeping launch, cache_book_block_kernel: 32 workgroups walk the batches in order and exchange
//                           their counts inside the launch (two to three exchanges per batch); per batch they leave ITEMS:
//                           per unique key {slot, miss?, update count after the batch, push?}, per evicted dirty line
//                           {slot, key, update count}, and a record of counts (the perf dict's numbers).
//   ha_cache_lookup_planned ONE launch, a wave per sorted position (cache_lookup_planned_kernel): the staleness-bounded pull
//                           decision (cache.cc:84-93: version -1 or lagging by more than pull_bound -- taken HERE, from the
//                           versions as they are when the rows are read: other workers may have pushed meanwhile), row to dest,
//                           refreshed line + Line::addup for pulled lines.
//   ha_cache_update_planned ONE launch (cache_update_planned_kernel): the ordered accumulate into gradient buffer and data row
//                           (scatter_dev.h's bit-exact chains), the pushed lines' server side FUSED into the wave that holds the
//                           line's new gradient (store row += grad, grad = 0), a wave per evicted dirty line (store row += its
//                           gradient), a thread per line for versions.
//
//   ha_cache_plan_block_push_pull / ha_cache_push_pull_planned
//                           the same idea for _embeddingPushPull (cache.cc:356-422), the asp-with-prefetch schedule's one call
//                           per step (LRU): a CHAIN of steps, each pulling a batch and pushing the batch pulled by the step before
//                           -- cache_book_chain_kernel on the side stream, then per step the update launch (push half) and the
//                           lookup launch (pull half, which takes the push half's version commit back for its decision).
//
// Field ownership while a block is planned: the bookkeeping launch owns slot_of, a line's key / state / stamp / updates, the
// stamp log, the free stack and the control block (all accessed device-coherently inside the launch: `sc1` loads / stores,
// MI355X_MICROARCH.md "inter-workgroup visibility"); the row launches own data, grad, hasgrad, a line's version, the store's
// rows and versions, and read nothing the bookkeeping writes except the items.  The call-by-call entry points are refused
// until the planned batches are consumed.
#include <cmath>
#include "cache_dev.h"
#include "scatter_dev.h"

extern "C" int ha_plan_build_batch_f32ids_lim(const float *const *ids, const int64_t *n, void *const *ws, int count,
                                              uint64_t key_limit, ha_stream_t stream);
extern "C" int ha_plan_build_batch_u64ids_lim(const uint64_t *const *ids, const int64_t *n, void *const *ws, int count,
                                              uint64_t key_limit, ha_stream_t stream);

namespace ha {

constexpr int kBookWg = 32;          // workgroups of the bookkeeping launch (all resident: 32 x 256 threads)
constexpr int kBookThreads = 256;
constexpr int kBookKeysPerThread = (kSmallMax + kBookWg * kBookThreads - 1) / (kBookWg * kBookThreads);   // 5
constexpr long long kVerKeep = -2;   // pver: the lookup did not pull this line

// ---- device-coherent accessors (agent scope = `sc1`: the load bypasses the CU's L1, the store is written through the L2) ----
template <typename T>
__device__ __forceinline__ T ldc(const T *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T>
__device__ __forceinline__ void stc(T *p, T v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// a line record as four 8-byte words: {stamp, version, key | updates << 32, freq | state << 32}
__device__ __forceinline__ unsigned long long *line_word(LineMeta *line, long long s, int w) {
    return reinterpret_cast<unsigned long long *>(line + s) + w;
}
static_assert(offsetof(LineMeta, stamp) == 0 && offsetof(LineMeta, version) == 8 && offsetof(LineMeta, key) == 16 &&
              offsetof(LineMeta, updates) == 20 && offsetof(LineMeta, freq) == 24 && offsetof(LineMeta, state) == 28,
              "the bookkeeping launch addresses a line record by 8-byte words");

struct BookArgs {
    int count;
    int n[kPlanBlockMax];
    const PlanHeader *hdr[kPlanBlockMax];
    const uint32_t *uniq[kPlanBlockMax];
    const int32_t *counts[kPlanBlockMax];
    int32_t *it_slot;        // [count][nmax] slot of unique key u (-1: a key beyond the cache's key range)
    uint8_t *it_flag;        // [count][nmax] kPosMiss | kPosInit (the line has a gradient buffer) | kPosPush
    int32_t *it_upd;         // [count][nmax] update counter of the line after this batch (what a push carries)
    int32_t *ev_slot;        // [count][nmax] evicted dirty lines of the batch's lookup, pushed by its update
    uint32_t *ev_key;
    int32_t *ev_upd;
    PlanRec *rec;            // [count]
    unsigned long long *xw;  // [4][kBookWg] exchange words
    long long nmax;
    // per batch: nullptr = BOUND mode (a line is pushed when its counter exceeds push_bound, cache.cc:159); else PUSH-KEY mode
    // (cache.cc:295-299): pk_mark[i][u] = 1 when unique key u is one of the batch's push keys (cache_plan_push_mark_kernel),
    // and a line is pushed iff it is marked and holds data
    const uint8_t *pk_mark[kPlanBlockMax];
};
// a line record's word 3 = freq | state << 32 | hg << 40
__device__ __forceinline__ unsigned long long line_w3(uint8_t state, bool hg) {
    return (static_cast<unsigned long long>(state) << 32) | (hg ? 1ull << 40 : 0ull);
}

// One exchange between the workgroups of the bookkeeping launch: every workgroup publishes (a, b) -- both < 2^20 -- and
// learns everybody's.  Word = seq << 40 | b << 20 | a; four word arrays in turn (a workgroup is at most one exchange ahead
// of the slowest one, so a word is never overwritten before everybody has read it).  Every wave drains its stores first:
// what it stored (`sc1`) is in memory before its workgroup's word is.  Returns false after ~2 s without an answer (the
// sticky word of the control block is set; the caller leaves the launch).
__device__ __forceinline__ bool book_exchange(CacheCtl *ctl, unsigned long long *xw, unsigned long long seq, uint32_t a,
                                              uint32_t b, uint32_t *s_a, uint32_t *s_b, int *s_abort) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    unsigned long long *words = xw + (seq & 3ull) * kBookWg;
    const int tid = threadIdx.x;
    if (tid == 0)
        stc(words + blockIdx.x, ((seq & 0xFFFFFFull) << 40) | (static_cast<unsigned long long>(b) << 20) | a);
    if (tid < kBookWg) {
        unsigned long long w = ldc(words + tid);
        if ((w >> 40) != (seq & 0xFFFFFFull)) {
            const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();      // 100 MHz
            do {
                __builtin_amdgcn_s_sleep(1);
                w = ldc(words + tid);
                if (__builtin_amdgcn_s_memrealtime() - t0 > 200000000ull) {
                    *s_abort = 1;
                    ctl->fb_timeout = 1;
                    break;
                }
            } while ((w >> 40) != (seq & 0xFFFFFFull));
        }
        s_a[tid] = static_cast<uint32_t>(w & 0xFFFFFull);
        s_b[tid] = static_cast<uint32_t>((w >> 20) & 0xFFFFFull);
    }
    __syncthreads();
    return *s_abort == 0;
}

// rank of a set flag among the set flags of the workgroup's lower threads + total (256 threads = 4 waves)
__device__ __forceinline__ uint32_t book_rank(bool f, uint32_t *s_w4, uint32_t *total) {
    const unsigned long long m = __ballot(f);
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const uint32_t below = __builtin_popcountll(m & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0)
        s_w4[w] = __builtin_popcountll(m);
    __syncthreads();
    uint32_t off = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < kBookThreads / 64; ++k) {
        const uint32_t c = s_w4[k];
        off += k < w ? c : 0u;
        tot += c;
    }
    *total = tot;
    return off + below;
}

// The stamp log is nearly full: compact it (valid entries keep their order), a tile of kBookWg x 256 entries at a time.
// Returns false when an exchange gave up.
__device__ __forceinline__ bool book_compact_log(const Cache &c, CacheCtl *ctl, unsigned long long *xw, unsigned long long &seq,
                                                 long long head, long long &tail, uint32_t *s_a, uint32_t *s_b, uint32_t *s_w4,
                                                 int *s_abort) {
    const int tid = threadIdx.x, g = blockIdx.x;
    long long wr = head;
    for (long long t0 = head; t0 < tail; t0 += kBookWg * kBookThreads) {
        const long long e = t0 + g * kBookThreads + tid;
        int ls = -1;
        unsigned long long lst = 0;
        bool valid = false;
        if (e < tail) {
            ls = static_cast<int>(ldc(c.log_slot + e % c.Lcap));
            lst = ldc(c.log_stamp + e % c.Lcap);
            const unsigned long long st = ldc(line_word(c.line, ls, 0));
            const unsigned long long w3 = ldc(line_word(c.line, ls, 3));
            valid = static_cast<uint8_t>(w3 >> 32) == kResident && st == lst;
        }
        uint32_t tot;
        const uint32_t r = book_rank(valid, s_w4, &tot);
        if (!book_exchange(ctl, xw, ++seq, tot, 0, s_a, s_b, s_abort))
            return false;
        uint32_t before = 0, all = 0;
        for (int k = 0; k < kBookWg; ++k) {
            before += k < g ? s_a[k] : 0u;
            all += s_a[k];
        }
        if (valid) {      // (positions below this tile's first entry: read by everybody before the exchange)
            stc(c.log_slot + (wr + before + r) % c.Lcap, static_cast<uint32_t>(ls));
            stc(c.log_stamp + (wr + before + r) % c.Lcap, lst);
        }
        wr += all;
    }
    tail = wr;
    if (!book_exchange(ctl, xw, ++seq, 0, 0, s_a, s_b, s_abort))
        return false;
    return true;
}

// LRUCache::insert's evictions (lru_cache.cc:9-25): the first `need` VALID entries from the log's head (valid: the line is
// resident and still carries the entry's stamp; entries at `tail` and beyond are not looked at).  Their slots go back on the
// free stack above the M entries the batch's misses took; the dirty ones (updates != 0) are listed in ev_*.
struct BookEvicted {
    long long new_head, evicted;
    uint32_t dirty;
};
__device__ __forceinline__ bool book_evict(const Cache &c, CacheCtl *ctl, unsigned long long *xw, unsigned long long &seq,
                                           long long need, long long head, long long tail, long long ftop, uint32_t M,
                                           int32_t *ev_slot, uint32_t *ev_key, int32_t *ev_upd, BookEvicted *out, uint32_t *s_a,
                                           uint32_t *s_b, uint32_t *s_w4, int *s_abort,
                                           uint32_t step = 0) {
    const int tid = threadIdx.x, g = blockIdx.x;
    const long long need0 = need;
    uint32_t taken_before = 0, dirty_before = 0;      // victims / dirty victims of the rounds before this one
    long long new_head = head;
    while (need > 0 && new_head < tail) {
        const long long e = new_head + g * kBookThreads + tid;
        int ls = -1;
        unsigned long long lst = 0, w2 = 0;
        bool valid = false;
        if (e < tail) {
            ls = static_cast<int>(ldc(c.log_slot + e % c.Lcap));
            lst = ldc(c.log_stamp + e % c.Lcap);
            const unsigned long long st = ldc(line_word(c.line, ls, 0));
            w2 = ldc(line_word(c.line, ls, 2));
            const unsigned long long w3 = ldc(line_word(c.line, ls, 3));
            valid = static_cast<uint8_t>(w3 >> 32) == kResident && st == lst;
            // (a push-pull chain: never a line that step `step` or the one before pulled, see cache_book_chain_kernel's marks)
            if (step != 0u && (static_cast<uint32_t>(w3) == step || static_cast<uint32_t>(w3) == step - 1u))
                valid = false;
        }
        const bool dirty = valid && static_cast<uint32_t>(w2 >> 32) != 0u;
        uint32_t tv, td;
        const uint32_t rv = book_rank(valid, s_w4, &tv);
        const uint32_t rd = book_rank(dirty, s_w4, &td);
        if (!book_exchange(ctl, xw, ++seq, tv, td, s_a, s_b, s_abort))
            return false;
        uint32_t vb = 0, db = 0, vall = 0;
        for (int k = 0; k < kBookWg; ++k) {
            vb += k < g ? s_a[k] : 0u;
            db += k < g ? s_b[k] : 0u;
            vall += s_a[k];
        }
        const bool take = valid && static_cast<long long>(vb + rv) < need;
        if (take) {
            const uint32_t key = static_cast<uint32_t>(w2);
            stc(c.slot_of + key, -1);
            stc(line_word(c.line, ls, 3), line_w3(kFree, false));
            stc(c.free_list + (ftop - M + taken_before + vb + rv), ls);
            if (dirty) {      // every valid entry in front of a victim is a victim: its rank among the dirty victims
                const long long at_e = dirty_before + db + rd;
                ev_slot[at_e] = ls;
                ev_key[at_e] = key;
                ev_upd[at_e] = static_cast<int32_t>(w2 >> 32);
            }
        }
        // the round's last victim tells everybody where the log's head is now, and how many dirty lines were taken
        const bool last = take && static_cast<long long>(vb + rv) == need - 1;
        const bool all_taken = static_cast<long long>(vall) <= need;
        uint32_t adv = 0, dcut = 0;
        if (last) {
            adv = static_cast<uint32_t>(e + 1 - new_head);
            dcut = db + rd + (dirty ? 1u : 0u);
        }
        if (!all_taken || static_cast<long long>(vall) == need) {
            // the cut is inside this round: one thread holds it
            const unsigned long long mm = __ballot(last);
            __syncthreads();
            if (tid < 2)
                s_w4[tid] = 0;
            __syncthreads();
            if (mm != 0ull && lane_id() == __builtin_ctzll(mm)) {
                s_w4[0] = adv;
                s_w4[1] = dcut;
            }
            __syncthreads();
            if (!book_exchange(ctl, xw, ++seq, s_w4[0], s_w4[1], s_a, s_b, s_abort))
                return false;
            uint32_t A = 0, D = 0;
            for (int k = 0; k < kBookWg; ++k) {
                A += s_a[k];
                D += s_b[k];
            }
            new_head += A;
            dirty_before += D;
            taken_before += static_cast<uint32_t>(need);
            need = 0;
        } else {
            uint32_t dall = 0;
            for (int k = 0; k < kBookWg; ++k)
                dall += s_b[k];
            new_head = min(new_head + static_cast<long long>(kBookWg) * kBookThreads, tail);
            taken_before += vall;
            dirty_before += dall;
            need -= vall;
        }
    }
    out->new_head = new_head;
    out->evicted = need0 - need;
    out->dirty = dirty_before;
    return true;
}

// ---- the bookkeeping of a block of batches ---------------------------------------------------------------------------------
// Per batch i (its unique keys u = 0 .. U-1 in key order, as `Unique<T>` hands them to batchedLookup, cache.cc:15-26,66-68):
//   every line of the batch ends the pair lookup + update as the cache's newest, in key order: stamp = clock + u, log entry
//   tail + u (lookup and update both touch every line in key order, lru_cache.cc:27-39; what the lookup's touch leaves is
//   overwritten by the update's before anything reads it: the eviction in between takes lines OUTSIDE the batch, limit >= batch);
//   misses take slots from the free stack (by miss rank), become resident;
//   LRUCache::insert (lru_cache.cc:9-25) evicts while size > limit: the first size + M - limit VALID entries from the log head
//   (valid: the line is resident and still carries the entry's stamp); their slots go back on the stack, the dirty ones
//   (updates != 0) are listed for the batch's update to push (cache.cc:160-166: the pending evictions join every push);
//   updates += occurrences; a line whose counter exceeds push_bound is pushed and starts again at 0 (cache.cc:159,171-177);
//   a batch planned with push keys pushes the lines whose key is marked instead (cache.cc:295-299; BookArgs::pk_mark).
__global__ __launch_bounds__(kBookThreads) void cache_book_block_kernel(Cache c, BookArgs a) {
    __shared__ uint32_t s_a[kBookWg], s_b[kBookWg], s_w4[kBookThreads / 64];
    __shared__ int s_abort;
    CacheCtl *ctl = c.ctl;
    const int tid = threadIdx.x, g = blockIdx.x;
    if (tid == 0)
        s_abort = 0;
    // the control block as the last launch that owned it left it (every workgroup carries it forward by itself: what
    // changes it are the exchanged counts)
    long long clock = ctl->clock, tail = ctl->log_tail, head = ctl->log_head, ftop = ctl->free_top, size = ctl->size;
    unsigned long long seq = static_cast<unsigned long long>(ctl->book_seq);
    __syncthreads();
    for (int i = 0; i < a.count; ++i) {
        const int n = a.n[i];
        const long long at = static_cast<long long>(i) * a.nmax;
        if (n == 0) {
            if (g == 0 && tid == 0) {
                PlanRec r{};
                r.size = size;
                r.full = size == c.limit;
                r.vh_slot = -1;
                a.rec[i] = r;
            }
            continue;
        }
        const int U = static_cast<int>(a.hdr[i]->n_unique);
        const uint32_t *uniq = a.uniq[i];
        const int32_t *counts = a.counts[i];
        const uint8_t *pkm = a.pk_mark[i];      // (every line of the batch that the update finds holds data)
        // ---- log nearly full: compact it first (valid entries keep their order), a tile of kBookWg x 256 entries at a time
        if (tail - head > c.Lcap - 4 * c.nmax - 2048 - kBookWg * kBookThreads) {
            if (!book_compact_log(c, ctl, a.xw, seq, head, tail, s_a, s_b, s_w4, &s_abort))
                return;
        }
        // ---- phase 1: probe; hits are touched and counted at once -----------------------------------------------------------
        const int per = (U + kBookWg - 1) / kBookWg;         // this workgroup's keys: [u0, u1)
        const int u0 = min(g * per, U), u1 = min(u0 + per, U);
        int sl[kBookKeysPerThread];
        uint32_t kk[kBookKeysPerThread], rk[kBookKeysPerThread];
        bool miss[kBookKeysPerThread];
        uint32_t wg_miss = 0;
#pragma unroll
        for (int j = 0; j < kBookKeysPerThread; ++j) {
            const int u = u0 + j * kBookThreads + tid;
            const bool on = u < u1;
            kk[j] = on ? uniq[u] : 0u;
            const bool known = on && kk[j] < static_cast<unsigned long long>(c.length);
            sl[j] = known ? ldc(c.slot_of + kk[j]) : -1;
            miss[j] = known && sl[j] < 0;
            if (on && !known) {        // a key the cache has no line for: zeros on lookup, ignored by the update
                a.it_slot[at + u] = -1;
                a.it_flag[at + u] = 0;
                a.it_upd[at + u] = 0;
            }
        }
#pragma unroll
        for (int j = 0; j < kBookKeysPerThread; ++j) {
            const int u = u0 + j * kBookThreads + tid;
            if (u < u1 && sl[j] >= 0) {
                const int s = sl[j];
                const unsigned long long w2 = ldc(line_word(c.line, s, 2));
                const unsigned long long w3 = ldc(line_word(c.line, s, 3));
                const bool hg = ((w3 >> 40) & 1ull) != 0ull;
                const int upd = static_cast<int>(w2 >> 32) + counts[u];
                const bool push = pkm ? pkm[u] != 0 : upd > c.push_bound;
                const unsigned long long st = static_cast<unsigned long long>(clock + u);
                stc(line_word(c.line, s, 0), st);
                stc(line_word(c.line, s, 2), static_cast<unsigned long long>(kk[j]) |
                                                 (static_cast<unsigned long long>(static_cast<uint32_t>(push ? 0 : upd)) << 32));
                const long long pos = (tail + u) % c.Lcap;
                stc(c.log_slot + pos, static_cast<uint32_t>(s));
                stc(c.log_stamp + pos, st);
                if (!hg)           // the batch's update gives the line its gradient buffer (Line::_maybeInitGrad)
                    stc(line_word(c.line, s, 3), line_w3(kResident, true));
                a.it_slot[at + u] = s;
                a.it_flag[at + u] = static_cast<uint8_t>((hg ? kPosInit : 0) | (push ? kPosPush : 0));
                a.it_upd[at + u] = upd;
            }
            uint32_t tot;
            rk[j] = wg_miss + book_rank(miss[j], s_w4, &tot);
            wg_miss += tot;
        }
        if (!book_exchange(ctl, a.xw, ++seq, wg_miss, 0, s_a, s_b, &s_abort))
            return;
        uint32_t mb = 0, M = 0;
        for (int k = 0; k < kBookWg; ++k) {
            mb += k < g ? s_a[k] : 0u;
            M += s_a[k];
        }
        // ---- phase 2: the misses become lines -------------------------------------------------------------------------------
#pragma unroll
        for (int j = 0; j < kBookKeysPerThread; ++j) {
            const int u = u0 + j * kBookThreads + tid;
            if (u < u1 && miss[j]) {
                const long long fi = ftop - 1 - static_cast<long long>(mb + rk[j]);
                const int s = fi >= 0 ? ldc(c.free_list + fi) : 0;     // (running out of slots: sizing, checked on the host)
                const int upd = counts[u];
                const bool push = pkm ? pkm[u] != 0 : upd > c.push_bound;
                const unsigned long long st = static_cast<unsigned long long>(clock + u);
                stc(line_word(c.line, s, 0), st);
                stc(line_word(c.line, s, 2), static_cast<unsigned long long>(kk[j]) |
                                                 (static_cast<unsigned long long>(static_cast<uint32_t>(push ? 0 : upd)) << 32));
                stc(line_word(c.line, s, 3), line_w3(kResident, true));
                stc(c.slot_of + kk[j], s);
                const long long pos = (tail + u) % c.Lcap;
                stc(c.log_slot + pos, static_cast<uint32_t>(s));
                stc(c.log_stamp + pos, st);
                a.it_slot[at + u] = s;
                a.it_flag[at + u] = static_cast<uint8_t>(kPosMiss | (push ? kPosPush : 0));
                a.it_upd[at + u] = upd;
            }
        }
        // ---- phase 3: LRUCache::insert's evictions --------------------------------------------------------------------------
        BookEvicted ev;
        if (!book_evict(c, ctl, a.xw, seq, size + M > c.limit ? size + M - c.limit : 0, head, tail, ftop, M, a.ev_slot + at,
                        a.ev_key + at, a.ev_upd + at, &ev, s_a, s_b, s_w4, &s_abort))
            return;
        const long long new_head = ev.new_head, evicted = ev.evicted;
        const uint32_t dirty_before = ev.dirty;
        // ---- the batch is booked -------------------------------------------------------------------------------------------
        head = new_head;
        ftop = ftop - M + evicted;
        size = size + M - evicted;
        tail += U;
        clock += U;
        if (g == 0 && tid == 0) {
            PlanRec r{};
            r.n = n;
            r.U = U;
            r.M = M;
            r.E = dirty_before;
            r.evicted = evicted;
            r.size = size;
            r.full = size == c.limit;
            r.npush = -1;         // (counted when the perf dict asks: ha_cache_perf)
            r.erep = dirty_before;
            r.vh_slot = -1;
            a.rec[i] = r;
        }
        // the next batch probes what this one inserted and evicted
        if (!book_exchange(ctl, a.xw, ++seq, 0, 0, s_a, s_b, &s_abort))
            return;
    }
    if (g == 0 && tid == 0) {
        ctl->clock = clock;
        ctl->log_tail = tail;
        ctl->log_head = head;
        ctl->free_top = ftop;
        ctl->size = size;
        ctl->evict_n = 0;
        ctl->book_seq = static_cast<long long>(seq);
        ctl->U = 0;
        ctl->M = 0;
    }
}


// ---- LFU / LFUOpt: the bookkeeping of a block of batches ---------------------------------------------------------------------
// What the two policies do to a lookup + update pair of the SAME keys (lfu_cache.cc / lfuopt_cache.cc; every line found is
// touched twice, by the lookup and by the update: use + 2, or -- LFUOpt -- into the never-evicted store once use reaches 10),
// given that the lowest use bucket is EMPTY when the batch starts (it is after every pair: the update's touch lifts every line
// the lookup inserted; ha_cache_plan_block checks it when the planned flow takes over from call-by-call calls):
//   cache not full (free0 = limit - size > 0): the first free0 misses are inserted; every further insert evicts the back of
//       the lowest bucket = the batch's own oldest insert (lfu_cache.cc:31-42): of M misses the first M - free0 never stay;
//   cache full: the FIRST insert evicts the line with the least (use, arrival) of all lines outside LFUOpt's store -- lines
//       of this batch included, as the lookup's touch left them -- and every further insert evicts the insert before it: one
//       old line leaves, the batch's LAST miss stays (LFUOpt with nothing outside the store: every insert is dropped,
//       lfuopt_cache.cc:18-24);
//   the update does not find the keys whose inserts did not stay (nor the evicted line's, when the batch holds it): their
//       gradients go to a line without data that is pushed at once (cache.cc:147-152,159).
// "The least (use, arrival) of all lines" is the one global question; the call-by-call flow answers it by a scan over every
// line (cache_scan_victim_*), 3.4 M records per batch at configs[1]'s cache.  Here a two-level minimum is kept instead: lkey[s]
// = use << 48 | stamp of the line in slot s (all ones: none / stored), bmin[b] = the minimum of a block of 32 slots.  A batch's
// touches rewrite their lines' keys and re-reduce those blocks; the question is one pass over bmin (106 K words at that cache).
constexpr int kLfuBlk = 32;
constexpr unsigned long long kKeyNone = ~0ull;
struct LfuTree {
    unsigned long long *lkey;    // [nblk * kLfuBlk]
    unsigned long long *bmin;    // [nblk]
    long long nblk;
    unsigned long long *xk;      // [kBookWg] a query's candidate per workgroup: key, block
    long long *xb;
};
__device__ __forceinline__ unsigned long long lfu_key(uint32_t use, unsigned long long stamp) {
    // (a use count beyond 65,535 orders by arrival alone among its like: never the minimum in practice)
    return (static_cast<unsigned long long>(use < 0xFFFFu ? use : 0xFFFFu) << 48) | (stamp & 0xFFFFFFFFFFFFull);
}
__global__ __launch_bounds__(256) void cache_lfu_keys_kernel(Cache c, LfuTree t) {
    const long long s = blockIdx.x * 256ll + threadIdx.x;
    if (s >= t.nblk * kLfuBlk)
        return;
    unsigned long long k = kKeyNone;
    if (s < c.S) {
        const LineMeta m = c.line[s];
        if (m.state == kResident)
            k = lfu_key(static_cast<uint32_t>(m.freq), m.stamp);
    }
    t.lkey[s] = k;
}
__global__ __launch_bounds__(256) void cache_lfu_mins_kernel(LfuTree t) {
    const long long b = blockIdx.x * 256ll + threadIdx.x;
    if (b >= t.nblk)
        return;
    unsigned long long m = kKeyNone;
    for (int k = 0; k < kLfuBlk; ++k) {
        const unsigned long long v = t.lkey[b * kLfuBlk + k];
        m = v < m ? v : m;
    }
    t.bmin[b] = m;
}

// book_exchange with a 40-bit payload per workgroup
__device__ __forceinline__ bool book_exchange_p(CacheCtl *ctl, unsigned long long *xw, unsigned long long seq,
                                                unsigned long long payload, unsigned long long *s_p, int *s_abort) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    unsigned long long *words = xw + (seq & 3ull) * kBookWg;
    const int tid = threadIdx.x;
    if (tid == 0)
        stc(words + blockIdx.x, ((seq & 0xFFFFFFull) << 40) | (payload & 0xFFFFFFFFFFull));
    if (tid < kBookWg) {
        unsigned long long w = ldc(words + tid);
        if ((w >> 40) != (seq & 0xFFFFFFull)) {
            const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();      // 100 MHz
            do {
                __builtin_amdgcn_s_sleep(1);
                w = ldc(words + tid);
                if (__builtin_amdgcn_s_memrealtime() - t0 > 200000000ull) {
                    *s_abort = 1;
                    ctl->fb_timeout = 1;
                    break;
                }
            } while ((w >> 40) != (seq & 0xFFFFFFull));
        }
        s_p[tid] = w & 0xFFFFFFFFFFull;
    }
    __syncthreads();
    return *s_abort == 0;
}
// the block minimum of slot s's block from its 32 keys (an exchange separates this from the keys' stores)
__device__ __forceinline__ void lfu_block_refresh(const LfuTree &t, long long s) {
    const long long b = s / kLfuBlk;
    const unsigned long long *p = t.lkey + b * kLfuBlk;
    unsigned long long v[kLfuBlk];
#pragma unroll
    for (int k = 0; k < kLfuBlk; ++k)
        v[k] = ldc(p + k);
    unsigned long long m = kKeyNone;
#pragma unroll
    for (int k = 0; k < kLfuBlk; ++k)
        m = v[k] < m ? v[k] : m;
    stc(t.bmin + b, m);
}
// the slot with the least key of all (-1: there is none) and that key; one exchange.  Every workgroup settles the SLOT of
// its candidate before the exchange (nobody rewrites keys between the exchange in front of a query and the query's own);
// behind it the first workgroups through are already rewriting lines -- the answer must not be looked up again there.
__device__ __forceinline__ bool lfu_query(CacheCtl *ctl, unsigned long long *xw, unsigned long long seq, const LfuTree &t,
                                          unsigned long long *s_p, unsigned long long *s_k, long long *s_i, int *s_abort,
                                          long long *slot_out, unsigned long long *key_out) {
    const int tid = threadIdx.x, g = blockIdx.x, lane = lane_id(), w = tid >> 6;
    unsigned long long best = kKeyNone;
    long long bi = -1;
    for (long long b = g * kBookThreads + tid; b < t.nblk; b += static_cast<long long>(kBookWg) * kBookThreads) {
        const unsigned long long v = ldc(t.bmin + b);
        if (v < best) {
            best = v;
            bi = b;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long ob = __shfl_xor(best, o, 64);
        const long long oi = __shfl_xor(bi, o, 64);
        if (ob < best) {
            best = ob;
            bi = oi;
        }
    }
    __syncthreads();
    if (lane == 0) {
        s_k[w] = best;
        s_i[w] = bi;
    }
    __syncthreads();
    if (w == 0) {
        best = s_k[0];
        bi = s_i[0];
        for (int k = 1; k < kBookThreads / 64; ++k)
            if (s_k[k] < best) {
                best = s_k[k];
                bi = s_i[k];
            }
        // (keys are unique: a stamp is given once) the slot of the block that carries the key
        long long slot = -1;
        if (best != kKeyNone) {
            const unsigned long long v = lane < kLfuBlk ? ldc(t.lkey + bi * kLfuBlk + lane) : kKeyNone;
            const unsigned long long m = __ballot(v == best);
            slot = m ? bi * kLfuBlk + __builtin_ctzll(m) : -1;
        }
        if (lane == 0) {
            stc(t.xk + g, slot >= 0 ? best : kKeyNone);
            stc(t.xb + g, slot);
        }
    }
    if (!book_exchange_p(ctl, xw, seq, 0ull, s_p, s_abort))
        return false;
    if (w == 0) {
        best = lane < kBookWg ? ldc(t.xk + lane) : kKeyNone;
        bi = lane < kBookWg ? ldc(t.xb + lane) : -1;
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long ob = __shfl_xor(best, o, 64);
            const long long oi = __shfl_xor(bi, o, 64);
            if (ob < best) {
                best = ob;
                bi = oi;
            }
        }
        if (lane == 0) {
            s_i[0] = best != kKeyNone ? bi : -1;
            s_k[0] = best;
        }
    }
    __syncthreads();
    *slot_out = s_i[0];
    *key_out = s_k[0];
    __syncthreads();
    return true;
}
// is `key` one of the batch's sorted unique keys?  (every thread of the workgroup asks; two probes)
__device__ __forceinline__ bool lfu_in_batch(const uint32_t *uniq, int U, uint32_t key) {
    const int tid = threadIdx.x;
    const int stride = (U + kBookThreads - 1) / kBookThreads;
    const int i0 = tid * stride;
    const int cnt = __syncthreads_count(i0 < U && uniq[i0] <= key);
    const int seg0 = (cnt > 0 ? cnt - 1 : 0) * stride;
    return __syncthreads_or(cnt > 0 && tid < stride && seg0 + tid < U && uniq[seg0 + tid] == key) != 0;
}

__global__ __launch_bounds__(kBookThreads) void cache_book_lfu_kernel(Cache c, BookArgs a, LfuTree t) {
    __shared__ unsigned long long s_p[kBookWg], s_k[kBookThreads / 64];
    __shared__ long long s_i[kBookThreads / 64];
    __shared__ uint32_t s_w4[kBookThreads / 64];
    __shared__ int s_abort;
    CacheCtl *ctl = c.ctl;
    const int tid = threadIdx.x, g = blockIdx.x;
    if (tid == 0)
        s_abort = 0;
    long long clock = ctl->clock, ftop = ctl->free_top, size = ctl->size, n_hash = ctl->n_hash;
    unsigned long long seq = static_cast<unsigned long long>(ctl->book_seq);
    const bool opt = c.policy == kLFUOpt;
    const uint32_t new_use = opt ? 1u : 2u;       // a line the lookup inserted, after the update's touch
    __syncthreads();
    for (int i = 0; i < a.count; ++i) {
        const int n = a.n[i];
        const long long at = static_cast<long long>(i) * a.nmax;
        if (n == 0) {
            if (g == 0 && tid == 0) {
                PlanRec r{};
                r.size = size;
                r.full = size == c.limit;
                r.vh_slot = -1;
                a.rec[i] = r;
            }
            continue;
        }
        const int U = static_cast<int>(a.hdr[i]->n_unique);
        const uint32_t *uniq = a.uniq[i];
        const int32_t *counts = a.counts[i];
        const uint8_t *pkm = a.pk_mark[i];      // (every line of the batch that the update finds holds data)
        const int per = (U + kBookWg - 1) / kBookWg;
        const int u0 = min(g * per, U), u1 = min(u0 + per, U);
        // ---- phase 1: probe; what the two touches will make of every line found ---------------------------------------------
        int sl[kBookKeysPerThread];
        uint32_t kk[kBookKeysPerThread], rk[kBookKeysPerThread];
        unsigned long long w2[kBookKeysPerThread], w3[kBookKeysPerThread];
        bool miss[kBookKeysPerThread];
        uint32_t wg_miss = 0, wg_st1 = 0, wg_st2 = 0;
#pragma unroll
        for (int j = 0; j < kBookKeysPerThread; ++j) {
            const int u = u0 + j * kBookThreads + tid;
            const bool on = u < u1;
            kk[j] = on ? uniq[u] : 0u;
            const bool known = on && kk[j] < static_cast<unsigned long long>(c.length);
            sl[j] = known ? ldc(c.slot_of + kk[j]) : -1;
            miss[j] = known && sl[j] < 0;
            if (on && !known) {
                a.it_slot[at + u] = -1;
                a.it_flag[at + u] = 0;
                a.it_upd[at + u] = 0;
            }
        }
#pragma unroll
        for (int j = 0; j < kBookKeysPerThread; ++j) {
            bool st1 = false, st2 = false;
            w2[j] = w3[j] = 0ull;
            if (sl[j] >= 0) {
                w2[j] = ldc(line_word(c.line, sl[j], 2));
                w3[j] = ldc(line_word(c.line, sl[j], 3));
                const uint32_t f = static_cast<uint32_t>(w3[j]);
                const bool res = static_cast<uint8_t>(w3[j] >> 32) == kResident;
                st1 = opt && res && f + 1 >= static_cast<uint32_t>(kUseCntMax);     // lfuopt_cache.cc:33-39, by the lookup's touch
                st2 = opt && res && !st1 && f + 2 >= static_cast<uint32_t>(kUseCntMax);   // by the update's
            }
            uint32_t tot;
            rk[j] = wg_miss + book_rank(miss[j], s_w4, &tot);
            wg_miss += tot;
            wg_st1 += static_cast<uint32_t>(__syncthreads_count(st1));
            wg_st2 += static_cast<uint32_t>(__syncthreads_count(st2));
        }
        if (!book_exchange_p(ctl, a.xw, ++seq, static_cast<unsigned long long>(wg_miss) | (static_cast<unsigned long long>(wg_st1) << 13) |
                                                 (static_cast<unsigned long long>(wg_st2) << 26), s_p, &s_abort))
            return;
        long long mb = 0, M = 0, ST1 = 0, ST2 = 0;
        for (int k = 0; k < kBookWg; ++k) {
            const long long m_k = static_cast<long long>(s_p[k] & 0x1FFFull);
            mb += k < g ? m_k : 0;
            M += m_k;
            ST1 += static_cast<long long>((s_p[k] >> 13) & 0x1FFFull);
            ST2 += static_cast<long long>((s_p[k] >> 26) & 0x1FFFull);
        }
        const long long free0 = c.limit > size ? c.limit - size : 0;
        const long long ev = M > free0 ? M - free0 : 0;
        const bool drop_all = opt && ev > 0 && free0 == 0 && n_hash - ST1 == 0;
        const bool scan = ev > 0 && free0 == 0 && !drop_all;
        const long long v_new = drop_all ? M : (scan ? ev - 1 : ev);     // the batch's first v_new inserts do not stay
        // ---- the line that leaves for the batch's first insert ----------------------------------------------------------------
        long long vslot = -1;
        unsigned long long vw2 = 0, vkey_lfu = kKeyNone;
        bool vin = false;
        if (scan) {
            // as the tree stands (the lines as the batch found them): the lookup's touch only raises keys, so a minimum that
            // is NOT a line of this batch is the minimum after the touch as well
            // (of the line's record only the word {key, updates} is read: nobody writes it before the batch is booked; its
            // state word is the first thing the fastest workgroup rewrites)
            if (!lfu_query(ctl, a.xw, ++seq, t, s_p, s_k, s_i, &s_abort, &vslot, &vkey_lfu))
                return;
            if (vslot >= 0) {
                vw2 = ldc(line_word(c.line, vslot, 2));
                vin = lfu_in_batch(uniq, U, static_cast<uint32_t>(vw2));
            }
            if (vin) {
                // it is one of the batch's lines: the keys of the batch's lines as the lookup's touch leaves them (use + 1,
                // arrival in key order; LFUOpt: a line that reaches the store drops out), then the question again
#pragma unroll
                for (int j = 0; j < kBookKeysPerThread; ++j) {
                    const int u = u0 + j * kBookThreads + tid;
                    if (sl[j] >= 0 && static_cast<uint8_t>(w3[j] >> 32) == kResident) {
                        const uint32_t f = static_cast<uint32_t>(w3[j]);
                        const bool st1 = opt && f + 1 >= static_cast<uint32_t>(kUseCntMax);
                        stc(t.lkey + sl[j], st1 ? kKeyNone : lfu_key(f + 1, static_cast<unsigned long long>(clock + u)));
                    }
                }
                if (!book_exchange_p(ctl, a.xw, ++seq, 0ull, s_p, &s_abort))
                    return;
#pragma unroll
                for (int j = 0; j < kBookKeysPerThread; ++j)
                    if (sl[j] >= 0 && static_cast<uint8_t>(w3[j] >> 32) == kResident)
                        lfu_block_refresh(t, sl[j]);
                if (!book_exchange_p(ctl, a.xw, ++seq, 0ull, s_p, &s_abort))
                    return;
                if (!lfu_query(ctl, a.xw, ++seq, t, s_p, s_k, s_i, &s_abort, &vslot, &vkey_lfu))
                    return;
                if (vslot >= 0) {
                    vw2 = ldc(line_word(c.line, vslot, 2));
                    vin = lfu_in_batch(uniq, U, static_cast<uint32_t>(vw2));
                }
            }
            if (vslot < 0) {       // (the counters say a line exists: the tree does not hold what they count)
                if (tid == 0) {
                    ctl->fb_timeout = 2;
                    ctl->ph[8] = static_cast<unsigned long long>(i);
                    ctl->ph[9] = static_cast<unsigned long long>(size);
                    ctl->ph[10] = static_cast<unsigned long long>(M);
                    ctl->ph[11] = vkey_lfu;
                    ctl->ph[12] = static_cast<unsigned long long>(n_hash);
                }
                return;
            }
        }
        const uint32_t vkey = static_cast<uint32_t>(vw2);
        const int vupd = static_cast<int>(vw2 >> 32);
        const bool vdirty = scan && vupd != 0;
        // ---- phase 2: the state after the pair; the items --------------------------------------------------------------------
        const long long clock2 = clock + U;
        long long rf[kBookKeysPerThread];          // slots whose block minimum this thread re-reduces
#pragma unroll
        for (int j = 0; j < kBookKeysPerThread; ++j) {
            const int u = u0 + j * kBookThreads + tid;
            rf[j] = -1;
            if (u >= u1)
                continue;
            if (sl[j] >= 0) {
                const int s = sl[j];
                const uint32_t f = static_cast<uint32_t>(w3[j]);
                const uint8_t state = static_cast<uint8_t>(w3[j] >> 32);
                const bool hg = ((w3[j] >> 40) & 1ull) != 0ull;
                if (scan && s == vslot) {
                    // this line is the one the batch's first insert evicts: the lookup still reads it (slot vh_slot of the
                    // record), the update does not find it -- a line without data in a spare slot, pushed at once
                    a.it_slot[at + u] = ldc(c.free_list + (ftop - M - 1));
                    // (push-key mode: a line without data is not pushed -- its gradient is dropped, cache.cc:295-299; the
                    // evicted line itself is still pushed as an eviction, kPosVictimPush)
                    a.it_flag[at + u] = static_cast<uint8_t>(kPosTemp | (pkm ? 0 : kPosPush) | kPosVictim |
                                                             (hg ? kPosVictimHg : 0) | (vdirty ? kPosVictimPush : 0));
                    a.it_upd[at + u] = counts[u];
                    continue;
                }
                const int upd = static_cast<int>(w2[j] >> 32) + counts[u];
                const bool push = pkm ? pkm[u] != 0 : upd > c.push_bound;
                uint8_t ns = state;
                uint32_t f2 = f;
                if (state == kResident) {
                    if (opt && f + 2 >= static_cast<uint32_t>(kUseCntMax))
                        ns = kStored;
                    else
                        f2 = f + 2;
                }
                const unsigned long long st = static_cast<unsigned long long>(clock2 + u);
                stc(line_word(c.line, s, 0), st);
                stc(line_word(c.line, s, 2), static_cast<unsigned long long>(kk[j]) |
                                                 (static_cast<unsigned long long>(static_cast<uint32_t>(push ? 0 : upd)) << 32));
                stc(line_word(c.line, s, 3), static_cast<unsigned long long>(f2) | line_w3(ns, true));
                if (state == kResident) {
                    stc(t.lkey + s, ns == kStored ? kKeyNone : lfu_key(f2, st));
                    rf[j] = s;
                }
                a.it_slot[at + u] = s;
                a.it_flag[at + u] = static_cast<uint8_t>((hg ? kPosInit : 0) | (push ? kPosPush : 0));
                a.it_upd[at + u] = upd;
            } else if (miss[j]) {
                // the batch's misses take the top M stack entries in rank order from below: the ones that stay are on top
                const long long q = mb + rk[j];
                const int s = ldc(c.free_list + (ftop - M + q));
                const int upd = counts[u];
                if (q < v_new) {          // inserted and evicted again by a later insert (or dropped): see the header
                    a.it_slot[at + u] = s;
                    a.it_flag[at + u] = static_cast<uint8_t>(kPosMiss | kPosTemp | (pkm ? 0 : kPosPush));
                    a.it_upd[at + u] = upd;
                    continue;
                }
                const bool push = pkm ? pkm[u] != 0 : upd > c.push_bound;
                const unsigned long long st = static_cast<unsigned long long>(clock2 + u);
                stc(line_word(c.line, s, 0), st);
                stc(line_word(c.line, s, 2), static_cast<unsigned long long>(kk[j]) |
                                                 (static_cast<unsigned long long>(static_cast<uint32_t>(push ? 0 : upd)) << 32));
                stc(line_word(c.line, s, 3), static_cast<unsigned long long>(new_use) | line_w3(kResident, true));
                stc(c.slot_of + kk[j], s);
                stc(t.lkey + s, lfu_key(new_use, st));
                rf[j] = s;
                a.it_slot[at + u] = s;
                a.it_flag[at + u] = static_cast<uint8_t>(kPosMiss | (push ? kPosPush : 0));
                a.it_upd[at + u] = upd;
            }
        }
        const long long stay = M - v_new;
        // (the evicted line of the batch itself was counted among the lines the update's touch stores when its use was 8: the
        // key it left with is use + 1)
        const bool v_st2 = scan && vin && opt && static_cast<uint32_t>(vkey_lfu >> 48) + 1 >= static_cast<uint32_t>(kUseCntMax);
        if (g == 0 && tid == 0) {
            long long E = 0;
            if (scan) {
                stc(c.slot_of + vkey, -1);
                stc(line_word(c.line, vslot, 3), line_w3(kFree, false));
                stc(t.lkey + vslot, kKeyNone);
                if (vdirty && !vin) {
                    a.ev_slot[at] = static_cast<int32_t>(vslot);
                    a.ev_key[at] = vkey;
                    a.ev_upd[at] = vupd;
                    E = 1;
                }
            }
            PlanRec r{};
            r.n = n;
            r.U = U;
            r.M = M;
            r.E = E;
            r.evicted = scan ? 1 : 0;
            r.size = size + stay - (scan ? 1 : 0);
            r.full = r.size == c.limit;
            r.npush = -1;
            r.erep = vdirty ? 1 : 0;
            r.umiss = v_new + (scan && vin ? 1 : 0);
            r.vh_slot = scan && vin ? vslot : -1;
            r.vh_upd = scan && vin ? vupd : 0;
            r.vh_key = scan && vin ? vkey : 0;
            a.rec[i] = r;
        }
        // ---- the batch is booked: the next one probes what this one left; the blocks of the rewritten keys ---------------------
        if (!book_exchange_p(ctl, a.xw, ++seq, 0ull, s_p, &s_abort))
            return;
#pragma unroll
        for (int j = 0; j < kBookKeysPerThread; ++j)
            if (rf[j] >= 0)
                lfu_block_refresh(t, rf[j]);
        if (scan && g == 0 && tid == 0) {
            lfu_block_refresh(t, vslot);
            stc(c.free_list + (ftop - stay), static_cast<int32_t>(vslot));    // (everybody has read the stack's old top)
        }
        ftop = ftop - stay + (scan ? 1 : 0);
        size = size + stay - (scan ? 1 : 0);
        n_hash = n_hash - ST1 - ST2 + (v_st2 ? 1 : 0) + stay - (scan ? 1 : 0);
        clock += 2ll * U;
    }
    if (g == 0 && tid == 0) {
        ctl->clock = clock;
        ctl->free_top = ftop;
        ctl->size = size;
        ctl->n_hash = n_hash;
        ctl->n_base = 0;
        ctl->evict_n = 0;
        ctl->book_seq = static_cast<long long>(seq);
        ctl->U = 0;
        ctl->M = 0;
    }
}

// ---- the push keys of a push-key batch (side stream, behind the index plans, in front of the bookkeeping launch) -----------
// A thread per push key: the key as the call-by-call update reads it (cache_f32_to_u32_kernel / cache_u64_to_u32_kernel), its
// position among the batch's sorted unique keys by binary search, a mark there.  The bookkeeping launch then reads one byte
// per key instead of searching itself (its launch is serial per batch; the search is ~13 dependent loads per key).  Push keys
// that are not keys of the batch mark nothing (cache.cc:295-299 skips them); duplicates mark the same byte.
struct PushMarkArgs {
    const void *keys[kPlanBlockMax];     // nullptr: no push keys (a bound-mode batch, an empty push set or an empty batch)
    long long n[kPlanBlockMax];
    const PlanHeader *hdr[kPlanBlockMax];
    const uint32_t *uniq[kPlanBlockMax];
    int nb[kPlanBlockMax];               // keys of the batch (U <= nb)
    int kind;                            // 0: float32 push keys, 1: 64-bit integers
};
__global__ __launch_bounds__(256) void cache_plan_push_mark_kernel(PushMarkArgs m, uint8_t *mark, long long nmax) {
    const int i = blockIdx.y;
    const long long j = blockIdx.x * 256ll + threadIdx.x;
    if (m.keys[i] == nullptr || j >= m.n[i])
        return;
    uint32_t k;
    if (m.kind == 0) {
        k = f32_to_key(static_cast<const float *>(m.keys[i])[j]);
    } else {
        const uint64_t v = static_cast<const uint64_t *>(m.keys[i])[j];
        k = v > 0xFFFFFFFEull ? 0xFFFFFFFEu : static_cast<uint32_t>(v);
    }
    const int U = min(static_cast<int>(m.hdr[i]->n_unique), m.nb[i]);
    const uint32_t *uq = m.uniq[i];
    int lo = 0, hi = U;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (uq[mid] < k)
            lo = mid + 1;
        else
            hi = mid;
    }
    if (lo < U && uq[lo] == k)
        mark[static_cast<long long>(i) * nmax + lo] = 1;
}

// ---- the items per sorted position (side stream, behind the bookkeeping launch) --------------------------------------------
// pos_item[p] = {slot, key, kPos* flags (| kPosHead at the first position of a key), occurrence index perm[p]}: what a row
// wave of position p needs, in ONE 16-byte record instead of three dependent lookups (upos[p] -> item of the key -> rows).
struct PlanExpandPtrs {
    const int32_t *upos[kPlanBlockMax];
    const int32_t *perm[kPlanBlockMax];
};
__global__ __launch_bounds__(256) void cache_plan_expand_kernel(BookArgs a, PlanExpandPtrs e, int4 *pos_item, int32_t *it_upd_pos) {
    const int i = blockIdx.y;
    const int n = a.n[i];
    const long long at = static_cast<long long>(i) * a.nmax;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < n; p += gridDim.x * 256) {
        const int u = e.upos[i][p];
        const bool head = p == 0 || e.upos[i][p - 1] != u;
        pos_item[at + p] = int4{a.it_slot[at + u], static_cast<int>(a.uniq[i][u]),
                                static_cast<int>(a.it_flag[at + u]) | (head ? kPosHead : 0), e.perm[i][p]};
        it_upd_pos[at + p] = a.it_upd[at + u];
    }
}

// ---- the lookup of a planned batch: ONE launch, a wave per sorted position -------------------------------------------------
// dest[perm[p],:] = the line of the position's key after syncEmbedding (cache.cc:84-97).  The pull decision is taken by every
// wave of a key from words nothing in this launch writes (the line's version, the store's version); the wave of the key's
// first position refreshes the line and STAGES its new version (pver[p]; the update's launch commits it -- a store into the
// record here would race with the other waves' reads).  Two round trips: the position's record; then versions and row together.
// (Measured, docs/EXPERIMENTS.md round 6: the forward gather's shape -- the output as flat 16-byte vectors, four vectors of
// different rows per lane, 256-thread workgroups -- 11.3 us against 9.1 for a wave per position; without the two version reads
// 9.07 against 9.29 us; without the row stores 7.65: the launch is the part's "copy of 6,656 random 2 KB rows" (DESIGN.md
// section 6, yardstick: 8.0 us), the staleness check is almost free beside it.)
// PP (the pull half of a push-pull step, launched BEHIND the step's push half): vadj[p] = the update counter that the push half
// has just added to the line's version because it pushed the line (0: it did not).  cache.cc judges staleness with the version
// as it is BEFORE that commit (:404 against :414-421) and adds the counter AFTER the pull, so the commit is taken back for the
// decision and a pulled line's staged version is the store's version + the counter.
template <int VEC, bool PP = false>
__global__ __launch_bounds__(1024) void cache_lookup_planned_kernel(
    Cache c, const int4 *__restrict__ pos_item, long long n, float *__restrict__ dest, long long *__restrict__ pver,
    const PlanRec *__restrict__ rec, const int32_t *__restrict__ vadj = nullptr) {
    const int lane = lane_id();
    const long long p = static_cast<long long>(blockIdx.x) * 16ll + uniform(static_cast<int>(threadIdx.x >> 6));
    if (p >= n)
        return;
    const int4 it = pos_item[p];
    int s = uniform(it.x);
    const long long lk = static_cast<long long>(uniform(static_cast<uint32_t>(it.y)));
    int fl = uniform(it.z);
    if (fl & kPosVictim) {      // (LFU policies) the line this batch's own lookup evicts: still in its old slot when the rows are read
        s = uniform(static_cast<int>(rec->vh_slot));
        fl = (fl & ~kPosInit) | ((fl & kPosVictimHg) ? kPosInit : 0);
    }
    const bool head = (fl & kPosHead) != 0;
    float *out = dest + static_cast<long long>(uniform(it.w)) * c.width;
    if (s >= c.S || lk >= c.store_rows || it.w < 0 || it.w >= n) {
        // an item no bookkeeping launch wrote (it gave up, or the row launch ran in front of it): nothing is touched, the sticky
        // word says so (ha_cache_state / ha_cache_perf raise)
        if (lane == 0 && c.ctl->fb_timeout == 0) {
            c.ctl->fb_timeout = 3;
            c.ctl->ph[8] = static_cast<unsigned long long>(static_cast<uint32_t>(it.x));
            c.ctl->ph[9] = static_cast<unsigned long long>(static_cast<uint32_t>(it.y));
            c.ctl->ph[10] = static_cast<unsigned long long>(static_cast<uint32_t>(it.z));
            c.ctl->ph[11] = static_cast<unsigned long long>(static_cast<uint32_t>(it.w));
            c.ctl->ph[12] = static_cast<unsigned long long>(p) | (static_cast<unsigned long long>(rec->M) << 32);
            c.ctl->ph[13] = static_cast<unsigned long long>(rec->n) | (static_cast<unsigned long long>(rec->U) << 32);
            c.ctl->ph[14] = static_cast<unsigned long long>(rec->size);
            c.ctl->ph[15] = static_cast<unsigned long long>(n);
        }
        return;
    }
    if (s < 0) {
        for (long long j = lane; j < c.width; j += kWave)
            out[j] = 0.f;
        return;
    }
    float *line = c.data + static_cast<long long>(s) * c.width;
    const bool is_miss = (fl & kPosMiss) != 0;
    const long long sv = c.srv_ver[lk];
    long long v = is_miss ? -1 : c.line[s].version;
    long long adj = 0;
    if (PP) {
        adj = static_cast<long long>(uniform(vadj[p]));
        v = v == -1 ? -1 : v - adj;
    }
    // the cached row, requested beside the two versions (a hit that is not stale -- the usual case -- has it on the way)
    float4v x0{0.f, 0.f, 0.f, 0.f}, x1 = x0;
    const long long j0 = lane * 4, j1 = j0 + kWave * 4;
    if (VEC == 4 && !is_miss) {
        if (j0 < c.width)
            x0 = ld4(line + j0);
        if (j1 < c.width)
            x1 = ld4(line + j1);
    }
    const bool pull = is_miss || v == -1 || sv - v > c.pull_bound;
    if (!pull) {
        if (VEC == 4) {
            if (j0 < c.width)
                st4_nt(out + j0, x0);
            if (j1 < c.width)
                st4_nt(out + j1, x1);
            for (long long j = j1 + kWave * 4; j < c.width; j += kWave * 4)
                st4_nt(out + j, ld4(line + j));
        } else {
            for (long long j = lane; j < c.width; j += kWave)
                out[j] = line[j];
        }
        if (head && lane == 0)
            pver[p] = kVerKeep;
        return;
    }
    const bool hg = (fl & kPosInit) != 0;      // the line has a gradient buffer: Line::addup() re-adds it to the pulled row
    const float *src = c.table + lk * c.width;
    const float *gr = c.grad + static_cast<long long>(s) * c.width;
    if (VEC == 4) {
        for (long long j = lane * 4; j < c.width; j += kWave * 4) {
            float4v x = ld4(src + j);
            if (hg) {
                const float4v gv = ld4(gr + j);
                x = float4v{__fadd_rn(x[0], gv[0]), __fadd_rn(x[1], gv[1]), __fadd_rn(x[2], gv[2]), __fadd_rn(x[3], gv[3])};
            }
            st4_nt(out + j, x);
            if (head)
                st4(line + j, x);
        }
    } else {
        for (long long j = lane; j < c.width; j += kWave) {
            float x = src[j];
            if (hg)
                x = __fadd_rn(x, gr[j]);  // Line::addup(): data += grad
            out[j] = x;
            if (head)
                line[j] = x;
        }
    }
    if (head && lane == 0)
        pver[p] = sv + adj;
}

// ---- the lookup of a planned batch, delivered SUM-POOLED: ONE launch, a wave per (bag, column slice) ------------------------
// out[b,:] = ((0.0f + r_lo) + r_lo+1) + ... over the rows r_j that cache_lookup_planned_kernel would have written for the
// occurrences j of bag b, in position order, one __fadd_rn per term (bagsum.hip's chain: what ha_cache_lookup_planned followed
// by ha_gather_sum over the ids 0 .. n-1 gives, bit for bit); the [n, width] rows are never written.  The mapping is
// bag_sum_kernel's: a bag is split over waves by COLUMNS only, lane l of a block of 64 positions fetches what its occurrence
// needs, the row pointers are broadcast with v_readlane and ROWS clamped row loads are in flight before the first add.
//
// What an occurrence needs is reached through the batch's index plan instead of a record per sorted position: the item of
// occurrence i is {it_slot, uniq, it_flag}[inverse[i]], the key's head occurrence (the FIRST one, the sort is stable) is
// perm[seg[u]] and its staged version lies at pver[seg[u]] -- where the update's meta role, which walks the sorted positions,
// looks for it.  Three dependent round trips per block of 64 positions: inverse; the item and seg; the two versions and perm.
//
// One writer.  Every wave that meets key u takes the pull decision from srv_ver[key] and line[slot].version, words nothing in
// this launch writes (see cache_lookup_planned_kernel), so all of them agree.  A line that is not pulled is read from its data
// row, which nobody writes.  A pulled key is read by EVERY wave from the store (+ the line's gradient row, Line::addup), never
// from the data row being refreshed; the waves whose bag holds the key's head occurrence store the refreshed row there, each
// its own column slice, and the slice-0 wave of them stages the version.  (Bags of a batch are disjoint ranges of positions,
// so that is one wave per slice.)
// An item no bookkeeping launch wrote: sticky word 3 as in cache_lookup_planned_kernel, a zero row, nothing refreshed.
// PP (the pooled pull half of a push-pull step, behind the step's push half): as cache_lookup_planned_kernel<.., PP> -- vadj[u]
// is what the push half has just added to the version of a line it pushed; it is fetched beside the key's item, taken back for
// the decision and added to the version staged for a pulled line.  PP = false reads nothing more than it did.
template <int VEC>
struct SumVec;
template <>
struct SumVec<1> {
    typedef float T;
    static __device__ __forceinline__ float get(const T &v, int) { return v; }
    static __device__ __forceinline__ void set(T &v, int, float x) { v = x; }
};
template <>
struct SumVec<2> {
    typedef float T __attribute__((ext_vector_type(2)));
    static __device__ __forceinline__ float get(const T &v, int k) { return v[k]; }
    static __device__ __forceinline__ void set(T &v, int k, float x) { v[k] = x; }
};
template <>
struct SumVec<4> {
    typedef float4v T;
    static __device__ __forceinline__ float get(const T &v, int k) { return v[k]; }
    static __device__ __forceinline__ void set(T &v, int k, float x) { v[k] = x; }
};
struct SumPlan {
    const int32_t *it_slot;      // per unique key of the batch (BookArgs)
    const uint8_t *it_flag;
    const uint32_t *uniq;
    const int32_t *inverse;      // [n] unique index of occurrence i
    const int32_t *seg;          // [U] first sorted position of unique key u
    const int32_t *perm;         // [n] occurrence index of sorted position p
    long long *pver;             // [n] staged versions, per sorted position (the heads')
    const PlanRec *rec;
    const int32_t *vadj;         // PP only: per unique key, the version adjust (the chain slot's it_upd, see ChainArgs)
};
constexpr int kSumWaves = 4;     // waves per workgroup
// row-pointer flags of a lane's occurrence
constexpr int kSumOk = 1, kSumGrad = 2, kSumHead = 4, kSumLive = 8;

// WEIGHTED (ha_cache_lookup_wsum_planned, the FAE models' masked bags): occurrence j adds fl(w_j * r_j) when w_j != 0 (+-0 are
// zero, NaN is not) and nothing otherwise.  The weight of position l comes with inverse[j] in the first round trip and is
// broadcast as bits beside the row's flag word, where the live bit (kSumLive) lies.  Everything in front of the multiply --
// the pull decision, Line::addup, the head's refreshed data row and staged version -- works on the UNWEIGHTED row and does not
// look at the weight: a dead head occurrence refreshes its line as a live one does, so the cache is left as the unpooled
// lookup leaves it.  WEIGHTED = false reads no weight and compiles to what it was.
template <int VEC, int ROWS, bool PP = false, bool WEIGHTED = false>
__global__ __launch_bounds__(kSumWaves *kWave) void cache_lookup_sum_planned_kernel(
    Cache c, SumPlan sp, long long n, long long bag, const int64_t *__restrict__ offsets, long long nbags, uint32_t nslice,
    float *__restrict__ out, const float *__restrict__ weights) {
    typedef typename SumVec<VEC>::T V;
    typedef const V __attribute__((address_space(1))) *GlobalV;
    const int lane = lane_id();
    const uint64_t item = static_cast<uint64_t>(blockIdx.x) * kSumWaves + (threadIdx.x >> 6);   // wave-uniform
    if (item >= static_cast<uint64_t>(nbags) * nslice)
        return;
    const long long b = static_cast<long long>(item / nslice);
    const uint32_t sl = static_cast<uint32_t>(item - static_cast<uint64_t>(b) * nslice);
    long long lo, hi;
    if (offsets != nullptr) {
        lo = offsets[b];
        hi = offsets[b + 1];
        lo = lo < 0 ? 0 : (lo > n ? n : lo);
        hi = hi < lo ? lo : (hi > n ? n : hi);
    } else {
        lo = b * bag;
        hi = lo + bag;      // (n == nbags * bag: checked by the host)
    }
    const uint32_t width = static_cast<uint32_t>(c.width);
    const uint32_t col = (sl * kWave + lane) * VEC;
    const bool live = col < width;       // (VEC > 1: width % VEC == 0, so a live lane's VEC columns all exist)
    const uint32_t lcol = live ? col : 0;
    V acc;
#pragma unroll
    for (int k = 0; k < VEC; ++k)
        SumVec<VEC>::set(acc, k, 0.f);
    for (long long j0 = lo; j0 < hi; j0 += kWave) {
        const int cnt = static_cast<int>(hi - j0 < kWave ? hi - j0 : kWave);      // positions of this block (wave-uniform)
        const bool mine = lane < cnt;
        const long long j = j0 + (mine ? lane : cnt - 1);                          // lo <= j < hi <= n
        // ---- the occurrence's item (every index is checked before an address is formed from it)
        const int u = sp.inverse[j];
        int wbits = 0;
        if (WEIGHTED)
            wbits = __float_as_int(weights[j]);      // (weights: n floats)
        const bool u_ok = u >= 0 && u < n;
        const int uu = u_ok ? u : 0;
        int s = sp.it_slot[uu];
        const long long lk = static_cast<long long>(sp.uniq[uu]);
        int fl = sp.it_flag[uu];
        const int sg = sp.seg[uu];
        long long adj = 0;
        if (PP)
            adj = static_cast<long long>(sp.vadj[uu]);
        if (fl & kPosVictim) {      // (LFU policies) the line this batch's own lookup evicts: still in its old slot
            s = static_cast<int>(sp.rec->vh_slot);
            fl = (fl & ~kPosInit) | ((fl & kPosVictimHg) ? kPosInit : 0);
        }
        const bool bad = !u_ok || s >= c.S || lk >= c.store_rows || sg < 0 || sg >= n;
        const unsigned long long badm = __ballot(mine && bad);
        if (badm != 0ull && lane == __builtin_ctzll(badm) && c.ctl->fb_timeout == 0) {
            c.ctl->fb_timeout = 3;
            c.ctl->ph[8] = static_cast<unsigned long long>(static_cast<uint32_t>(s));
            c.ctl->ph[9] = static_cast<unsigned long long>(lk);
            c.ctl->ph[10] = static_cast<unsigned long long>(static_cast<uint32_t>(fl));
            c.ctl->ph[11] = static_cast<unsigned long long>(j);
            c.ctl->ph[12] = static_cast<unsigned long long>(static_cast<uint32_t>(u)) | (static_cast<unsigned long long>(sp.rec->M) << 32);
            c.ctl->ph[13] = static_cast<unsigned long long>(sp.rec->n) | (static_cast<unsigned long long>(sp.rec->U) << 32);
            c.ctl->ph[14] = static_cast<unsigned long long>(sp.rec->size);
            c.ctl->ph[15] = static_cast<unsigned long long>(n);
        }
        const bool ok = !bad && s >= 0;      // (s < 0: a key the cache has no line for -- a zero row)
        // ---- the pull decision, and which occurrence is the key's head
        const bool is_miss = (fl & kPosMiss) != 0;
        long long sv = 0, v = -1;
        int ho = -1;
        if (ok) {
            sv = c.srv_ver[lk];
            if (!is_miss)
                v = c.line[s].version;
            ho = sp.perm[sg];
        }
        if (PP)      // the push half's commit is taken back for the decision (cache.cc:404 against :414-421)
            v = v == -1 ? -1 : v - adj;
        const bool pull = is_miss || v == -1 || sv - v > c.pull_bound;
        const bool head = ok && mine && static_cast<long long>(ho) == j;
        if (head && sl == 0)
            sp.pver[sg] = pull ? sv + adj : kVerKeep;
        const uint64_t loff = static_cast<uint64_t>(ok ? s : 0) * width;      // float offset of the line's rows
        const float *src = ok ? (pull ? c.table + static_cast<uint64_t>(lk) * width : c.data + loff) : c.data;
        const uint64_t sa = reinterpret_cast<uint64_t>(src);
        const int src_lo = static_cast<int>(static_cast<uint32_t>(sa)), src_hi = static_cast<int>(static_cast<uint32_t>(sa >> 32));
        const int lof_lo = static_cast<int>(static_cast<uint32_t>(loff)), lof_hi = static_cast<int>(static_cast<uint32_t>(loff >> 32));
        // the line has a gradient buffer: Line::addup() re-adds it to the pulled row
        const int rf = (ok ? kSumOk : 0) | ((ok && pull && (fl & kPosInit)) ? kSumGrad : 0) | ((head && pull) ? kSumHead : 0) |
                       ((WEIGHTED && (wbits & 0x7FFFFFFF) != 0) ? kSumLive : 0);
        for (int r0 = 0; r0 < cnt; r0 += ROWS) {
            V x[ROWS];
#pragma unroll
            for (int t = 0; t < ROWS; ++t) {
                const int tt = r0 + t < cnt ? r0 + t : cnt - 1;
                const uint64_t a = (static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readlane(src_hi, tt))) << 32) |
                                   static_cast<uint32_t>(__builtin_amdgcn_readlane(src_lo, tt));
                // (a pointer rebuilt from two registers: told to be a GLOBAL one, or the loads would be flat_load)
                x[t] = *(GlobalV)(a + static_cast<uint64_t>(lcol) * sizeof(float));
            }
            // every request of the round is issued before the first add (see bag_sum_kernel)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < ROWS; ++t) {
                const bool in = r0 + t < cnt;                                     // wave-uniform
                const int f = __builtin_amdgcn_readlane(rf, in ? r0 + t : 0);     // wave-uniform
                V xv = x[t];
                if (in && (f & (kSumGrad | kSumHead))) {      // a pulled line with a gradient buffer, or the key's head: rare
                    const uint64_t o = (static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readlane(lof_hi, r0 + t))) << 32) |
                                       static_cast<uint32_t>(__builtin_amdgcn_readlane(lof_lo, r0 + t));
                    if (f & kSumGrad) {
                        const V g = *reinterpret_cast<const V *>(c.grad + o + lcol);
#pragma unroll
                        for (int k = 0; k < VEC; ++k)
                            SumVec<VEC>::set(xv, k, __fadd_rn(SumVec<VEC>::get(xv, k), SumVec<VEC>::get(g, k)));   // data += grad
                    }
                    if ((f & kSumHead) && live)
                        *reinterpret_cast<V *>(c.data + o + col) = xv;
                }
                const bool rok = (f & kSumOk) != 0;
                if (WEIGHTED) {
                    // (an item without a line is the zero row the unpooled lookup writes: w * 0)
                    const float w = __int_as_float(__builtin_amdgcn_readlane(wbits, in ? r0 + t : 0));      // wave-uniform
                    const bool take = in && (f & kSumLive) != 0;                                            // wave-uniform
#pragma unroll
                    for (int k = 0; k < VEC; ++k) {
                        const float a = SumVec<VEC>::get(acc, k);
                        const float sum = __fadd_rn(a, __fmul_rn(w, rok ? SumVec<VEC>::get(xv, k) : 0.f));
                        SumVec<VEC>::set(acc, k, take ? sum : a);
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) {
                        const float a = SumVec<VEC>::get(acc, k);
                        const float sum = __fadd_rn(a, rok ? SumVec<VEC>::get(xv, k) : 0.f);
                        SumVec<VEC>::set(acc, k, in ? sum : a);
                    }
                }
            }
        }
    }
    // the pooled rows are consumed by another kernel (the dense tower): written around the L2, as bag_sum_kernel's
    if (live)
        __builtin_nontemporal_store(acc, reinterpret_cast<V *>(out + static_cast<uint64_t>(b) * width + col));
}

// ---- the update of a planned batch from WEIGHTED bags (ha_cache_update_planned_wbags, the FAE models' masked bags) -----------
// The accumulate role of the launch below in its WEIGHTED form.  The term of occurrence i is
// t_i = fl(scale * fl(w_i * g[bag(i), :])) when w_i != 0 and z = fl(scale * +0) otherwise: ha_cache_update_planned on the
// [n, width] tensor of the t_i, bit for bit.  A key's chain is acc = acc - fl(-1 * t_i) over its occurrences in position
// order (step<kModeSgd> with lr = -1, what apply_body runs),
// into the line's gradient buffer (from +0 without kPosInit) and into its data row; the push epilogue and the stores are
// apply_body's.  The dead occurrences are NOT walked: adding z = -0 changes nothing, adding z = +0 changes only a -0
// accumulator, and after the first +0 term the accumulator is never -0 again (round-to-nearest gives -0 only from -0 + -0), so
// the chain over all occurrences is the chain over the live ones followed by ONE add of z whenever the run holds a dead
// occurrence (tests/test_wcache_cpu.py).  No gradient row of a dead occurrence is read: what it holds cannot reach the cache.
//
// MI355X layout: a wave per sorted position, as apply_body.  The wave at offset o < W = min(run length, slices, 16) of its run
// takes the column slices o, o + W, ... (64 * VEC columns each); every other wave leaves after its window.  It walks the run
// from its first position: the window of sorted positions p-16 .. p+47 holds a run shorter than 48 whole (the common case:
// perm and the weights are two round trips), a longer run goes on in blocks of kWcacheTrip * 64 positions, sorted and perm
// of the next block requested before this block's weights are used.  Lane l holds bag and weight of one position; the live
// ones are walked by the bits of one ballot (scalar), kBatch gradient rows in flight before the first multiply -- a dead
// occurrence costs neither a row load nor a chain step, and the padding id's all-dead run of thousands is one scan of its
// weights and one add of z.  No LDS, no barrier.
constexpr int kWcacheTrip = 4;
struct WbagArgs {
    const float *weights;      // [n]
    float scale;
    uint32_t nbags;
};
// the accumulate role of cache_update_planned_kernel<VEC, true, true>; vblock: the workgroup's index among the role's
template <int VEC>
__device__ __forceinline__ void cache_wbags_accumulate(const Cache &c, const uint32_t *__restrict__ sorted,
                                                       const int32_t *__restrict__ perm, int n,
                                                       const float *__restrict__ bag_grads, const ApplyMaps &maps,
                                                       const WbagArgs &wa, int vblock) {
    const float *__restrict__ weights = wa.weights;
    const float scale = wa.scale;
    const uint32_t nbags = wa.nbags;
    constexpr int kBatch = VEC == 4 ? 8 : 16;
    const int lane = lane_id();
    const int w = uniform(static_cast<int>(threadIdx.x >> 6));
    const int p = vblock * kPosPerBlock + w;
    if (p >= n)
        return;
    const int width = static_cast<int>(c.width);
    // ---- the window p-16 .. p+47: the wave's offset in its run, the run's end if it lies inside
    const int q = p - kLookBack + lane;
    const int cq = max(0, min(q, n - 1));
    const uint32_t ks = sorted[cq];
    const int pi0 = perm[cq];
    const int4 pit = maps.pos_item[p];
    const uint32_t key = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(ks), kLookBack));
    const unsigned long long eq = __ballot(q >= 0 && q < n && ks == key);
    const uint32_t inv_lo = static_cast<uint32_t>(~eq) & 0xFFFFu;
    const int o = inv_lo == 0 ? kLookBack : (__builtin_clz(inv_lo) - 16);      // offset in the run, capped
    const unsigned long long inv_hi = (~eq) >> kLookBack;                      // bit t <-> position p+t, 48 valid bits
    const int fwd = __builtin_ctzll(inv_hi | (1ull << 48));                    // 1..48 (48: the run reaches the window's end)
    const int nslice = (width + kWave * VEC - 1) / (kWave * VEC);
    const int workers = min(min(o + fwd, nslice), kLookBack);
    if (o >= workers)
        return;
    if (pit.x < 0 || pit.x >= c.S)
        return;      // a key without a line / a record out of range: ignored, as apply_body does
    const uint64_t row = static_cast<uint64_t>(pit.x);
    const bool init = (pit.z & kPosInit) != 0;
    float *dst_row = c.grad + row * static_cast<uint64_t>(width);
    const bool d2on = (pit.z & kPosTemp) == 0;
    float *d2row = maps.dst2 + row * static_cast<uint64_t>(width);
    float *push = ((pit.z & kPosPush) && static_cast<uint64_t>(static_cast<uint32_t>(pit.y)) < maps.push_rows)
                      ? maps.push_tab + static_cast<uint64_t>(static_cast<uint32_t>(pit.y)) * static_cast<uint64_t>(width)
                      : nullptr;
    const float *push2 = (pit.z & kPosVictimPush)
                             ? c.grad + static_cast<uint64_t>(*maps.victim_row) * static_cast<uint64_t>(width)
                             : nullptr;
    const bool keep = (pit.z & kPosKeep) != 0;
    const float z = __fmul_rn(scale, 0.f);
    // bag of occurrence i, clamped as wbag_grad_rows_kernel clamps it: no row beyond bag_grads is read whatever bag_of holds
    auto bag_at = [&](int i) {
        const uint32_t b = static_cast<uint32_t>(maps.valmap ? maps.valmap[i] : bag_row(i, maps.valdiv));
        return static_cast<int>(b < nbags ? b : nbags - 1);
    };
    // the window's share of the run: lanes kLookBack - o .. kLookBack + fwd - 1
    const int bg0 = bag_at(pi0);
    const int wb0 = __float_as_int(weights[pi0]);      // (pi0 < n whatever the lane's position: weights has n elements)
    const bool in0 = lane >= kLookBack - o && lane < kLookBack + fwd;
    const unsigned long long live0 = __ballot(in0 && (wb0 & 0x7FFFFFFF) != 0);
    const bool dead0 = __ballot(in0 && (wb0 & 0x7FFFFFFF) == 0) != 0ull;

    for (int sl = o; sl < nslice; sl += workers) {
        const int col = (sl * kWave + lane) * VEC;
        const bool colok = col < width;      // (VEC > 1: width % VEC == 0)
        const int colc = colok ? col : 0;
        Vec<VEC> acc, acc2;
        acc.zero();
        acc2.zero();
        if (init)
            acc.load(dst_row + colc);
        if (d2on)
            acc2.load(d2row + colc);
        // the live occurrences of one block of 64 positions, in position order
        auto chain = [&](unsigned long long m, int bg, int wb) {
            while (m != 0ull) {
                int tt[kBatch];      // lanes of the next (up to) kBatch live occurrences: wave-uniform
                const int cnt = min(kBatch, static_cast<int>(__builtin_popcountll(m)));
#pragma unroll
                for (int k = 0; k < kBatch; ++k) {
                    tt[k] = m != 0ull ? static_cast<int>(__builtin_ctzll(m)) : 0;
                    m &= m - 1ull;      // (0 stays 0)
                }
                Vec<VEC> g[kBatch];
#pragma unroll
                for (int k = 0; k < kBatch; ++k) {
                    if (k < cnt) {
                        const uint64_t off =
                            static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readlane(bg, tt[k]))) * width + colc;
                        g[k].load(bag_grads + off);
                    }
                }
#pragma unroll
                for (int k = 0; k < kBatch; ++k) {
                    if (k < cnt) {
                        const float wv = __int_as_float(__builtin_amdgcn_readlane(wb, tt[k]));
#pragma unroll
                        for (int e = 0; e < VEC; ++e) {
                            const float t = __fmul_rn(scale, __fmul_rn(wv, g[k].get(e)));
                            acc.set(e, step<kModeSgd>(acc.get(e), t, -1.0f));
                            acc2.set(e, step<kModeSgd>(acc2.get(e), t, -1.0f));
                        }
                    }
                }
            }
        };
        chain(live0, bg0, wb0);
        bool dead = dead0;
        // ---- the run goes on behind the window: blocks of kWcacheTrip * 64 positions from p + 48
        if (fwd >= 48 && p + 48 < n) {
            int base = p + 48;
            uint32_t kq[kWcacheTrip];
            int pq[kWcacheTrip];
#pragma unroll
            for (int k = 0; k < kWcacheTrip; ++k) {
                const int at = min(base + k * kWave + lane, n - 1);
                kq[k] = sorted[at];
                pq[k] = perm[at];
            }
            bool more = true;
            while (more) {
                int bg[kWcacheTrip], wb[kWcacheTrip], cnt[kWcacheTrip];
#pragma unroll
                for (int k = 0; k < kWcacheTrip; ++k) {
                    bg[k] = bag_at(pq[k]);
                    wb[k] = __float_as_int(weights[pq[k]]);
                    // the run is contiguous: its positions of this block are a prefix of the block
                    const unsigned long long mk = __ballot(base + k * kWave + lane < n && kq[k] == key);
                    cnt[k] = (~mk == 0ull) ? kWave : static_cast<int>(__builtin_ctzll(~mk));
                }
                more = cnt[kWcacheTrip - 1] == kWave && base + kWcacheTrip * kWave < n;
#pragma unroll
                for (int k = 0; k + 1 < kWcacheTrip; ++k)
                    more = more && cnt[k] == kWave;
                const int nbase = base + kWcacheTrip * kWave;
                if (more) {
#pragma unroll
                    for (int k = 0; k < kWcacheTrip; ++k) {
                        const int at = min(nbase + k * kWave + lane, n - 1);
                        kq[k] = sorted[at];
                        pq[k] = perm[at];
                    }
                }
                bool open = true;      // (a block behind the run's end holds none of its positions)
#pragma unroll
                for (int k = 0; k < kWcacheTrip; ++k) {
                    const bool ink = open && lane < cnt[k];
                    const bool lv = (wb[k] & 0x7FFFFFFF) != 0;
                    const unsigned long long m = __ballot(ink && lv);
                    dead = dead || __ballot(ink && !lv) != 0ull;
                    chain(m, bg[k], wb[k]);
                    open = open && cnt[k] == kWave;
                }
                base = nbase;
            }
        }
        if (dead) {      // (wave-uniform) every dead occurrence of the run at once
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                acc.set(e, step<kModeSgd>(acc.get(e), z, -1.0f));
                acc2.set(e, step<kModeSgd>(acc2.get(e), z, -1.0f));
            }
        }
        if (colok) {
            if (push)
                push_epilogue<VEC>(push, col, acc, push2, keep);
            acc.store(dst_row + col);
            if (d2on)
                acc2.store(d2row + col);
        }
    }
}

// ---- the update of a planned batch: ONE launch -----------------------------------------------------------------------------
// the first kPlanMetaBlocks workgroups: a thread per sorted position, the heads work: the line's version (staged by the
//     lookup, + updates for a pushed line: cache.cc:171-177; for EVERY line of a push-key batch: cache.cc:321-327), the store's
//     version of a pushed line, hasgrad;
// the next kPlanEvictBlocks workgroups: a wave per evicted dirty line: store row += its gradient, store version += its updates
//     (PSFhandle_embedding.cc:23-27); the slot is free already (the bookkeeping freed it, nothing reuses it before the next
//     batch's lookup);
// the rest: the ordered accumulate (apply_body, DUAL == 2: gradient buffer and data row; pushed lines take the push epilogue --
//     store row += the line's new gradient, gradient buffer = 0).
// (The independent short roles come first in the grid: they start with the launch, not behind 400 accumulate workgroups.)
// pkmode (a batch planned with push keys): a line without data (kPosTemp) carries no kPosPush, so its accumulate keeps the
// gradient in the spare slot instead of pushing it -- the gradient the reference drops.  Nothing reads it again: the slot stays
// on the free stack, and every line that takes a slot next is a miss (no kPosInit: its accumulate starts from 0, its lookup
// adds no gradient) or, call by call, an insert that clears hasgrad.
// BAGS (ha_cache_update_planned_bags): `grads` is the POOLED gradient [nbags, width]; the source row of occurrence i is its bag
// -- i / maps.valdiv (fixed bags) or maps.valmap[i] (ragged: bag_of) --, read in place of row i of an expanded [n, width]
// tensor: the same values in the same order, so the same bits.  The meta and evict roles do not read gradients.
// WEIGHTED (ha_cache_update_planned_wbags): the accumulate role is cache_wbags_accumulate above, which needs no workgroup
// memory and more registers than apply_body's budget leaves: launch bounds of its own.  The other instantiations ignore `wa`.
constexpr int kPlanEvictBlocks = 64, kPlanMetaBlocks = 8;
template <int VEC, bool BAGS = false, bool WEIGHTED = false>
__global__ __launch_bounds__(1024, WEIGHTED ? 4 : 8) void cache_update_planned_kernel(
    Cache c, const uint32_t *__restrict__ sorted, const int32_t *__restrict__ perm, int n, const float *__restrict__ grads,
    ApplyMaps maps, const int32_t *__restrict__ it_upd_pos, const long long *__restrict__ pver,
    const int32_t *__restrict__ ev_slot, const uint32_t *__restrict__ ev_key, const int32_t *__restrict__ ev_upd,
    const PlanRec *__restrict__ rec, int pkmode, WbagArgs wa) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_apply[];
    const int b = blockIdx.x;
    if (WEIGHTED && b >= kPlanMetaBlocks + kPlanEvictBlocks) {      // (launched without workgroup memory)
        cache_wbags_accumulate<VEC>(c, sorted, perm, n, grads, maps, wa, b - kPlanMetaBlocks - kPlanEvictBlocks);
        return;
    }
    if (b >= kPlanMetaBlocks + kPlanEvictBlocks) {
        apply_body<kModeSgd, VEC, 2, kHandNone, BAGS>(c.grad, static_cast<uint64_t>(c.S), static_cast<int>(c.width), sorted, perm,
                                                      nullptr, n, grads, -1.0f, b - kPlanMetaBlocks - kPlanEvictBlocks, s_apply,
                                                      nullptr, maps);
        return;
    }
    const int lane = lane_id();
    if (b >= kPlanMetaBlocks) {
        const int E = static_cast<int>(min(rec->E, static_cast<long long>(n)));
        // push-key mode, LFU policies: the dirty line the batch's own lookup evicted is pushed by a wave of its own (its key's
        // item is a line without data, not pushed, whose accumulate has no push epilogue to carry it); its version: meta role
        const int EV = E + ((pkmode && rec->vh_slot >= 0 && rec->vh_upd != 0) ? 1 : 0);
        for (int j = (b - kPlanMetaBlocks) * 16 + static_cast<int>(threadIdx.x >> 6); j < EV; j += kPlanEvictBlocks * 16) {
            const bool vic = j == E;
            const int s = uniform(vic ? static_cast<int>(rec->vh_slot) : ev_slot[j]);
            const long long lk = static_cast<long long>(uniform(vic ? static_cast<uint32_t>(rec->vh_key) : ev_key[j]));
            if (s < 0 || s >= c.S || lk >= c.store_rows)
                continue;
            float *row = c.table + lk * c.width;
            const float *g = c.grad + static_cast<long long>(s) * c.width;
            if (VEC == 4) {
                for (long long q0 = 0; q0 < c.width; q0 += kWave * 8) {
                    const long long q = q0 + lane * 4, q2 = q + kWave * 4;
                    const bool x = q < c.width, y = q2 < c.width;
                    float4v r0{0.f, 0.f, 0.f, 0.f}, r1 = r0, g0 = r0, g1 = r0;
                    if (x) {
                        r0 = ld4(row + q);
                        g0 = ld4(g + q);
                    }
                    if (y) {
                        r1 = ld4(row + q2);
                        g1 = ld4(g + q2);
                    }
                    if (x)
                        st4(row + q, float4v{__fadd_rn(r0[0], g0[0]), __fadd_rn(r0[1], g0[1]), __fadd_rn(r0[2], g0[2]),
                                             __fadd_rn(r0[3], g0[3])});
                    if (y)
                        st4(row + q2, float4v{__fadd_rn(r1[0], g1[0]), __fadd_rn(r1[1], g1[1]), __fadd_rn(r1[2], g1[2]),
                                              __fadd_rn(r1[3], g1[3])});
                }
            } else {
                for (long long q = lane; q < c.width; q += kWave)
                    row[q] = __fadd_rn(row[q], g[q]);
            }
            if (lane == 0 && !vic)
                c.srv_ver[lk] += ev_upd[j];
        }
        return;
    }
    for (int p = b * 1024 + static_cast<int>(threadIdx.x); p < n; p += kPlanMetaBlocks * 1024) {
        const int4 it = maps.pos_item[p];
        if (it.x < 0 || !(it.z & kPosHead) || it.x >= c.S || static_cast<long long>(static_cast<uint32_t>(it.y)) >= c.store_rows)
            continue;
        if (it.z & kPosTemp) {     // (LFU policies) a line that is not in the cache: pushed (push-key mode: dropped), nothing of it stays
            c.srv_ver[static_cast<uint32_t>(it.y)] += (pkmode ? 0 : it_upd_pos[p]) +
                                                      ((it.z & kPosVictimPush) ? static_cast<int>(rec->vh_upd) : 0);
            continue;
        }
        const int s = it.x;
        const long long pv = pver[p];
        long long v = pv != kVerKeep ? pv : c.line[s].version;
        const int upd = it_upd_pos[p];
        if (it.z & kPosPush) {
            v += upd;
            c.srv_ver[static_cast<uint32_t>(it.y)] += upd;
        } else if (pkmode) {       // cache.cc:321-327: every line's version goes up by its counter, pushed or not
            v += upd;
        }
        c.line[s].version = v;
        c.hasgrad[s] = 1;
    }
}

// ---- the bookkeeping of a block of a PUSH-PULL CHAIN (LRU) -------------------------------------------------------------------
// Step i of the block is CacheBase::_embeddingPushPull (cache.cc:356-422) with pull = batch i (unique keys u = 0 .. Up-1) and
// push = the batch of the step before (v = 0 .. Uq-1, every occurrence counted in counts_q); the chain's head has no push side
// (_embeddingLookup, :60-107), its closing step no pull side (_embeddingUpdate, :132-197).  In the reference's order:
//   the pull batch's hits are touched in key order, then EVERY push key (a key of both batches ends at its push touch), then the
//   pull misses are inserted in key order as the newest lines, each taking a slot from the free stack; LRUCache::insert evicts
//   from the old end.  The host has checked n_pull + n_push <= limit: no line the step touches is among its victims, and every
//   push key -- pulled by the step before -- is still resident (a push key that is not: sticky word 4).
//   Only the PUSH touch is stamped and logged (stamp clock + v): every line a step pulls is a push key of the NEXT step (the
//   closing step included) and is touched there again, in key order as well, before any eviction could look at it -- its place
//   among the lines that can be evicted is decided by push touches alone.  Until then the eviction walk passes over it by its
//   mark (ChainArgs), and a new line carries a stamp of its own that no log entry has (clock + Uq + miss rank).
//   A push line's counter grows by its occurrences; beyond push_bound it is pushed and starts again at 0 (:392,414-420).
//   The dirty victims are NOT pushed by this step: they wait (evict_, :378) for the next one, whose push half reads this step's
//   ev_* list.  ctl->evict_n carries their number from launch to launch; the closing step leaves 0.
// What the row launches get: per unique pull key {slot, kPosMiss, kPosInit: the line has a gradient buffer when the pull half
// runs (it had one, or the push half gives it one), the version adjust: its counter if this step pushes it, else 0 -- see
// cache_lookup_planned_kernel<.., PP>}; per unique push key {slot, kPosInit, kPosPush, kItemKeep, the counter after the step}.
// kItemKeep: a line pushed AND pulled by the step keeps its gradient row through the push (Line::addup of the pull still adds
// it, :404 is in front of zeroGrad :419); its bookkeeping copy of hasgrad is cleared instead, so the next step's accumulate --
// the line is a key of the batch pulled now, so it is pushed again by the next step -- starts from zero (no kPosInit).
constexpr uint8_t kItemKeep = 1;      // (q_flag only: the bit kPosMiss has in a pull item)
constexpr uint32_t kLogNoSlot = 0;
constexpr unsigned long long kLogNoStamp = ~0ull;      // a log entry that is never valid (no line carries this stamp)
struct ChainArgs {
    int count;
    int n_p[kPlanBlockMax];              // keys of the step's pull batch (-1: the closing step)
    int n_q[kPlanBlockMax];              // keys of its push batch (0: the chain's head, or an empty batch)
    const PlanHeader *hdr_p[kPlanBlockMax], *hdr_q[kPlanBlockMax];
    const uint32_t *uniq_p[kPlanBlockMax], *uniq_q[kPlanBlockMax];
    const int32_t *counts_q[kPlanBlockMax];
    int32_t *it_slot;        // [count][nmax] pull side, per unique key
    uint8_t *it_flag;
    int32_t *it_upd;         // the version adjust
    int32_t *q_slot;         // [count][nmax] push side, per unique key of the batch before
    uint8_t *q_flag;
    int32_t *q_upd;
    int32_t *ev_slot;        // [count][nmax] the dirty lines this step's insert evicted (pushed by the NEXT step)
    uint32_t *ev_key;
    int32_t *ev_upd;
    PlanRec *rec;
    unsigned long long *xw;
    long long nmax;
    // "is this line a key of the step's OTHER batch, and which": every line that step number t pulls (hit or miss, unique key
    // u) carries the MARK (t, u) in its record's word 3 (chain_w3: the LRU policy has no use for `freq`).  Step t's pull side
    // finds the marks of step t - 1 (whose pull batch is its push batch), its push side the marks the pull side has just
    // written, the eviction walk both -- in the record it reads anyway, instead of a binary search per key
    unsigned long long step0;            // number of the block's first step (32 bits are kept; numbers start at 2)
};
// a line record's word 3 with a mark: step | state << 32 | hg << 40 | u << 48
__device__ __forceinline__ unsigned long long chain_w3(unsigned long long step, uint8_t state, bool hg, uint32_t u) {
    return (step & 0xFFFFFFFFull) | line_w3(state, hg) | (static_cast<unsigned long long>(u) << 48);
}
static_assert(kSmallMax <= 65536, "a mark keeps the position among a batch's unique keys in 16 bits");
__global__ __launch_bounds__(kBookThreads) void cache_book_chain_kernel(Cache c, ChainArgs a) {
    __shared__ uint32_t s_a[kBookWg], s_b[kBookWg], s_w4[kBookThreads / 64];
    __shared__ int s_abort;
    CacheCtl *ctl = c.ctl;
    const int tid = threadIdx.x, g = blockIdx.x;
    if (tid == 0)
        s_abort = 0;
    long long clock = ctl->clock, tail = ctl->log_tail, head = ctl->log_head, ftop = ctl->free_top, size = ctl->size;
    long long pend = ctl->evict_n;      // dirty lines the step before evicted: this step's push half pushes them
    unsigned long long seq = static_cast<unsigned long long>(ctl->book_seq);
    __syncthreads();
    for (int i = 0; i < a.count; ++i) {
        const int np = a.n_p[i], nq = a.n_q[i];
        const long long at = static_cast<long long>(i) * a.nmax;
        const unsigned long long t = a.step0 + static_cast<unsigned long long>(i);
        const uint32_t t32 = static_cast<uint32_t>(t), tb32 = static_cast<uint32_t>(t - 1ull);
        const int Up = np > 0 ? static_cast<int>(a.hdr_p[i]->n_unique) : 0;
        const int Uq = nq > 0 ? static_cast<int>(a.hdr_q[i]->n_unique) : 0;
        const uint32_t *uniq_p = a.uniq_p[i], *uniq_q = a.uniq_q[i];
        const int32_t *counts_q = a.counts_q[i];
        if (tail - head > c.Lcap - 4 * c.nmax - 2048 - kBookWg * kBookThreads) {
            if (!book_compact_log(c, ctl, a.xw, seq, head, tail, s_a, s_b, s_w4, &s_abort))
                return;
        }
        // ---- everything the step READS of the lines, requested together: both batches' slots, then their line words -----------
        // (nothing is written before these loads are back except words nobody reads here; the push side's STORES wait behind
        // the exchange: the pull side of another workgroup reads the counter and the hasgrad copy of a line of both batches)
        const int per = (Up + kBookWg - 1) / kBookWg;
        const int u0 = min(g * per, Up), u1 = min(u0 + per, Up);
        const int perq = (Uq + kBookWg - 1) / kBookWg;
        const int v0 = min(g * perq, Uq), v1 = min(v0 + perq, Uq);
        uint32_t kk[kBookKeysPerThread], rk[kBookKeysPerThread], kq[kBookKeysPerThread];
        int sp[kBookKeysPerThread], sq[kBookKeysPerThread];
        bool miss[kBookKeysPerThread];
        unsigned long long pw2[kBookKeysPerThread], pw3[kBookKeysPerThread], qw2[kBookKeysPerThread];
        uint32_t wg_miss = 0;
#pragma unroll
        for (int j = 0; j < kBookKeysPerThread; ++j) {
            const int u = u0 + j * kBookThreads + tid, v = v0 + j * kBookThreads + tid;
            kk[j] = u < u1 ? uniq_p[u] : 0xFFFFFFFFu;
            kq[j] = v < v1 ? uniq_q[v] : 0xFFFFFFFFu;
            sp[j] = u < u1 && kk[j] < static_cast<unsigned long long>(c.length) ? ldc(c.slot_of + kk[j]) : -1;
            sq[j] = v < v1 && kq[j] < static_cast<unsigned long long>(c.length) ? ldc(c.slot_of + kq[j]) : -1;
            miss[j] = u < u1 && kk[j] < static_cast<unsigned long long>(c.length) && sp[j] < 0;
        }
#pragma unroll
        for (int j = 0; j < kBookKeysPerThread; ++j) {
            pw2[j] = pw3[j] = qw2[j] = 0ull;
            if (sp[j] >= 0) {
                pw2[j] = ldc(line_word(c.line, sp[j], 2));
                pw3[j] = ldc(line_word(c.line, sp[j], 3));
            }
            if (sq[j] >= 0)
                qw2[j] = ldc(line_word(c.line, sq[j], 2));
        }
        // ---- the pull side: marks, items, the misses' ranks (no stamp: see the header) ----------------------------------------
#pragma unroll
        for (int j = 0; j < kBookKeysPerThread; ++j) {
            const int u = u0 + j * kBookThreads + tid;
            if (u < u1) {
                const int s = sp[j];
                int vq = s >= 0 && Uq > 0 && static_cast<uint32_t>(pw3[j]) == tb32 ? static_cast<int>(pw3[j] >> 48) : -1;
                vq = vq < Uq ? vq : -1;      // (a mark of the step before names a key of its batch: always below Uq)
                if (s >= 0) {
                    stc(line_word(c.line, s, 3), chain_w3(t, kResident, ((pw3[j] >> 40) & 1ull) != 0ull, static_cast<uint32_t>(u)));
                    int adj = 0;
                    if (vq >= 0) {
                        const int upd = static_cast<int>(pw2[j] >> 32) + counts_q[vq];
                        adj = upd > c.push_bound ? upd : 0;
                    }
                    a.it_slot[at + u] = s;
                    a.it_flag[at + u] = static_cast<uint8_t>((((pw3[j] >> 40) & 1ull) != 0ull || vq >= 0) ? kPosInit : 0);
                    a.it_upd[at + u] = adj;
                } else if (!miss[j]) {
                    a.it_slot[at + u] = -1;
                    a.it_flag[at + u] = 0;
                    a.it_upd[at + u] = 0;
                }
            }
            uint32_t tot;
            rk[j] = wg_miss + book_rank(miss[j], s_w4, &tot);
            wg_miss += tot;
        }
        if (!book_exchange(ctl, a.xw, ++seq, wg_miss, 0, s_a, s_b, &s_abort))
            return;
        uint32_t mb = 0, M = 0;
        for (int k = 0; k < kBookWg; ++k) {
            mb += k < g ? s_a[k] : 0u;
            M += s_a[k];
        }
        // ---- the push side: every key is touched; counters, the bounded push -------------------------------------------------
#pragma unroll
        for (int j = 0; j < kBookKeysPerThread; ++j) {
            const int v = v0 + j * kBookThreads + tid;
            if (v >= v1)
                continue;
            const uint32_t key = kq[j];
            const int s = sq[j];
            const long long pos = (tail + v) % c.Lcap;
            if (s < 0) {      // beyond the cache's range: ignored; in range: cannot be (see the header)
                if (key < static_cast<unsigned long long>(c.length))
                    ctl->fb_timeout = 4;
                stc(c.log_slot + pos, kLogNoSlot);
                stc(c.log_stamp + pos, kLogNoStamp);
                a.q_slot[at + v] = -1;
                a.q_flag[at + v] = 0;
                a.q_upd[at + v] = 0;
                continue;
            }
            const unsigned long long w3 = ldc(line_word(c.line, s, 3));      // (with the mark of this step's pull side, if any)
            const bool hg = ((w3 >> 40) & 1ull) != 0ull;
            const int upd = static_cast<int>(qw2[j] >> 32) + counts_q[v];
            const bool push = upd > c.push_bound;
            const bool keep = push && static_cast<uint32_t>(w3) == t32;
            const unsigned long long st = static_cast<unsigned long long>(clock + v);
            stc(line_word(c.line, s, 0), st);
            stc(line_word(c.line, s, 2), static_cast<unsigned long long>(key) |
                                             (static_cast<unsigned long long>(static_cast<uint32_t>(push ? 0 : upd)) << 32));
            if (hg == keep)      // the accumulate gives the line its gradient buffer; a kept one counts as none afterwards
                stc(line_word(c.line, s, 3), (w3 & ~(0xFFull << 40)) | (keep ? 0ull : 1ull << 40));
            stc(c.log_slot + pos, static_cast<uint32_t>(s));
            stc(c.log_stamp + pos, st);
            a.q_slot[at + v] = s;
            a.q_flag[at + v] = static_cast<uint8_t>((hg ? kPosInit : 0) | (push ? kPosPush : 0) | (keep ? kItemKeep : 0));
            a.q_upd[at + v] = upd;
        }
        // ---- the pull misses become lines, the newest of all -----------------------------------------------------------------
#pragma unroll
        for (int j = 0; j < kBookKeysPerThread; ++j) {
            const int u = u0 + j * kBookThreads + tid;
            if (u < u1 && miss[j]) {
                const long long r = static_cast<long long>(mb + rk[j]);
                const long long fi = ftop - 1 - r;
                const int s = fi >= 0 ? ldc(c.free_list + fi) : 0;     // (running out of slots: sizing, checked on the host)
                // (a stamp no log entry carries: the slot's last line left its own behind)
                stc(line_word(c.line, s, 0), static_cast<unsigned long long>(clock + Uq + r));
                stc(line_word(c.line, s, 2), static_cast<unsigned long long>(kk[j]));
                stc(line_word(c.line, s, 3), chain_w3(t, kResident, false, static_cast<uint32_t>(u)));
                stc(c.slot_of + kk[j], s);
                a.it_slot[at + u] = s;
                a.it_flag[at + u] = static_cast<uint8_t>(kPosMiss);
                a.it_upd[at + u] = 0;
            }
        }
        // ---- LRUCache::insert's evictions: never a line this step or the step before pulled (by their marks: the first carry
        //      the stamps of their last push touch, the second are re-stamped by other workgroups just now) --------------------
        BookEvicted ev;
        if (!book_evict(c, ctl, a.xw, seq, size + M > c.limit ? size + M - c.limit : 0, head, tail, ftop, M, a.ev_slot + at,
                        a.ev_key + at, a.ev_upd + at, &ev, s_a, s_b, s_w4, &s_abort, t32))
            return;
        head = ev.new_head;
        ftop = ftop - M + ev.evicted;
        size = size + M - ev.evicted;
        tail += Uq;
        clock += static_cast<long long>(Uq) + M;
        if (g == 0 && tid == 0) {
            PlanRec r{};
            r.n = np >= 0 ? np : nq;      // (the closing step reports as the update it is: the perf dict's Push record)
            r.U = np >= 0 ? Up : Uq;
            r.M = M;
            r.E = ev.dirty;
            r.evicted = ev.evicted;
            r.size = size;
            r.full = size == c.limit;
            r.npush = -1;
            r.erep = np >= 0 ? static_cast<long long>(ev.dirty) : pend;
            r.vh_slot = -1;
            a.rec[i] = r;
        }
        pend = ev.dirty;
        if (!book_exchange(ctl, a.xw, ++seq, 0, 0, s_a, s_b, &s_abort))
            return;
    }
    if (g == 0 && tid == 0) {
        ctl->clock = clock;
        ctl->log_tail = tail;
        ctl->log_head = head;
        ctl->free_top = ftop;
        ctl->size = size;
        ctl->evict_n = pend;
        ctl->book_seq = static_cast<long long>(seq);
        ctl->U = 0;
        ctl->M = 0;
    }
}

// the items of a chain block per sorted position (as cache_plan_expand_kernel): blockIdx.z = 0 the pull side of entry
// blockIdx.y (positions of its own batch), 1 the push side (positions of the batch before)
struct ChainExpandPtrs {
    int n[2][kPlanBlockMax];
    const uint32_t *uniq[2][kPlanBlockMax];
    const int32_t *upos[2][kPlanBlockMax];
    const int32_t *perm[2][kPlanBlockMax];
};
__global__ __launch_bounds__(256) void cache_chain_expand_kernel(ChainArgs a, ChainExpandPtrs e, int4 *pos_item, int32_t *it_upd_pos,
                                                                 int4 *q_pos_item, int32_t *q_upd_pos) {
    const int i = blockIdx.y, side = blockIdx.z;
    const int n = e.n[side][i];
    const long long at = static_cast<long long>(i) * a.nmax;
    const int32_t *upos = e.upos[side][i], *perm = e.perm[side][i];
    const uint32_t *uniq = e.uniq[side][i];
    for (int p = blockIdx.x * 256 + threadIdx.x; p < n; p += gridDim.x * 256) {
        const int u = upos[p];
        const int head = (p == 0 || upos[p - 1] != u) ? kPosHead : 0;
        if (side == 0) {
            pos_item[at + p] = int4{a.it_slot[at + u], static_cast<int>(uniq[u]), static_cast<int>(a.it_flag[at + u]) | head, perm[p]};
            it_upd_pos[at + p] = a.it_upd[at + u];
        } else {
            const int f = a.q_flag[at + u];
            q_pos_item[at + p] = int4{a.q_slot[at + u], static_cast<int>(uniq[u]),
                                      (f & (kPosInit | kPosPush)) | ((f & kItemKeep) ? kPosKeep : 0) | head, perm[p]};
            q_upd_pos[at + p] = a.q_upd[at + u];
        }
    }
}

// An open chain, looked at from outside (ha_cache_snapshot) while the last row call made is a pull half: the versions it staged
// are committed (the next push half would do it: it finds kVerKeep then and keeps the line's version), and the gradient rows
// that the step's push half kept for it (kPosKeep) are zeroed -- what Line::zeroGrad leaves (nothing reads them again: the
// next accumulate of such a line carries no kPosInit).  A wave per sorted position.
__global__ __launch_bounds__(1024) void cache_chain_settle_kernel(Cache c, const int4 *__restrict__ pos_item, long long n,
                                                                  long long *__restrict__ pver, const int4 *__restrict__ q_pos_item,
                                                                  long long nq) {
    const int lane = lane_id();
    const long long p = static_cast<long long>(blockIdx.x) * 16ll + uniform(static_cast<int>(threadIdx.x >> 6));
    if (p < n) {
        const int4 it = pos_item[p];
        if (lane == 0 && it.x >= 0 && it.x < c.S && (it.z & kPosHead)) {
            const long long pv = pver[p];
            if (pv != kVerKeep) {
                c.line[it.x].version = pv;
                pver[p] = kVerKeep;
            }
        }
    }
    if (p < nq) {
        const int4 it = q_pos_item[p];
        if (it.x >= 0 && it.x < c.S && (it.z & kPosHead) && (it.z & kPosKeep)) {
            float *g = c.grad + static_cast<long long>(it.x) * c.width;
            for (long long j = lane; j < c.width; j += kWave)
                g[j] = 0.f;
        }
    }
}

// the perf dict's data-dependent counts of a planned batch, on demand: lines the lookup pulled, lines the update pushed
__global__ __launch_bounds__(1024) void cache_plan_count_kernel(PlanRec *rec, const long long *pver, const int4 *pos_item) {
    __shared__ unsigned long long s_p[16], s_q[16];
    const int n = static_cast<int>(rec->n);
    unsigned long long pulled = 0, pushed = 0;
    for (int p = threadIdx.x; p < n; p += 1024) {
        const int4 it = pos_item[p];
        if (it.x < 0 || !(it.z & kPosHead))
            continue;
        pulled += pver[p] != kVerKeep ? 1 : 0;
        pushed += (it.z & kPosPush) ? 1 : 0;
    }
    for (int o = 32; o >= 1; o >>= 1) {
        pulled += __shfl_xor(pulled, o, 64);
        pushed += __shfl_xor(pushed, o, 64);
    }
    if (lane_id() == 0) {
        s_p[threadIdx.x >> 6] = pulled;
        s_q[threadIdx.x >> 6] = pushed;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long a = 0, b = 0;
        for (int k = 0; k < 16; ++k) {
            a += s_p[k];
            b += s_q[k];
        }
        rec->pulled = static_cast<long long>(a);
        rec->npush = static_cast<long long>(b);
    }
}

}  // namespace ha

using namespace ha;

// ---- host side -------------------------------------------------------------------------------------------------------------
static int plan_slot_alloc(ha_cache *h, PlanSlot &sl) {
    if (sl.it_slot)
        return 0;
    const size_t per = static_cast<size_t>(h->c.nmax), all = per * kPlanBlockMax;
    bool ok = true;
#define PLAN_ALLOC(field, count)                                                \
    do {                                                                        \
        if (ok && dmalloc(&sl.field, static_cast<size_t>(count)) != 0)          \
            ok = false;                                                         \
        else if (ok)                                                            \
            h->allocs.push_back(sl.field);                                      \
    } while (0)
    PLAN_ALLOC(it_slot, all);
    PLAN_ALLOC(it_flag, all);
    PLAN_ALLOC(it_upd, all);
    PLAN_ALLOC(pos_item, all);
    PLAN_ALLOC(it_upd_pos, all);
    PLAN_ALLOC(pver, all);
    PLAN_ALLOC(ev_slot, all);
    PLAN_ALLOC(ev_key, all);
    PLAN_ALLOC(ev_upd, all);
    PLAN_ALLOC(rec, kPlanBlockMax);
    PLAN_ALLOC(pk_mark, all);
#undef PLAN_ALLOC
    for (int i = 0; ok && i < kPlanBlockMax; ++i) {
        char *p = nullptr;
        if (dmalloc(&p, h->plan_bytes) != 0) {
            ok = false;
            break;
        }
        ok = dzero(p, 256) == 0;      // the plan header (sticky flags)
        sl.ws[i] = p;
        h->allocs.push_back(p);
    }
    HA_REQUIRE(ok, "cache_plan_block: out of device memory");
    HA_CHECK_HIP(hipEventCreateWithFlags(&sl.booked, hipEventDisableTiming));
    HA_CHECK_HIP(hipEventCreateWithFlags(&sl.rows_done, hipEventDisableTiming));
    return 0;
}

extern "C" int ha_cache_plan_pending(ha_cache *h) {
    if (!h)
        return 0;
    int pending = 0;
    for (const PlanSlot &sl : h->plan)
        pending += sl.count > 0 ? sl.total() - sl.next_call : 0;
    return pending;
}

// The bookkeeping of the next `count` (1..16) batches: their lookups and updates follow as ha_cache_lookup_planned /
// ha_cache_update_planned, in this order, lookup and update alternating.  `side`: the stream the plans and the bookkeeping
// launch run on; `main`: the stream of the row launches (the row launches of the block that used this block's buffers before are
// ordered in front of the bookkeeping; EVERYTHING enqueued on it so far only with push keys, for the first blocks and after
// call-by-call entry points -- in steady state a bound-mode block's key buffers must be complete by other means).  At most TWO
// blocks are outstanding (the one being consumed and the next).  The key buffers must stay unchanged until the bookkeeping
// has run (event `booked`; the row launches wait for it).
// push_keys == nullptr: every batch in bound mode (ha_cache_plan_block); else ha_cache_plan_block_push_keys (see the header).
static int plan_block_impl(ha_cache *h, const void *const *keys, int key_kind, const int64_t *n, const void *const *push_keys,
                           int push_kind, const int64_t *n_push, int count, ha_stream_t side, ha_stream_t main) {
    HA_REQUIRE(h && keys && n && (key_kind == 0 || key_kind == 1) && count >= 1 && count <= kPlanBlockMax,
               "cache_plan_block: bad arguments (1..%d batches)", kPlanBlockMax);
    Cache &c = h->c;
    const bool with_pk = push_keys != nullptr;
    if (with_pk) {
        HA_REQUIRE(n_push && (push_kind == 0 || push_kind == 1), "cache_plan_block_push_keys: bad arguments (push_kind 0 or 1)");
        for (int i = 0; i < count; ++i)
            HA_REQUIRE(n_push[i] <= c.nmax && (n_push[i] <= 0 || push_keys[i]),
                       "cache_plan_block_push_keys: batch %d has %ld push keys (at most max_batch = %ld)", i, (long)n_push[i],
                       (long)c.nmax);
    }
    HA_REQUIRE(c.table && !c.remote && !c.bypass, "cache_plan_block: a cache over a local store, not bypassed");
    HA_REQUIRE(c.row_start == 0 && c.store_rows >= c.length, "cache_plan_block: the store must hold every key of the cache's range");

    HA_REQUIRE(c.limit >= 1, "cache_plan_block: an empty cache");
    HA_CACHE_CHAIN_CLOSED(h, "cache_plan_block");
    HA_REQUIRE(h->evict_empty || ha_cache_plan_pending(h) > 0, "cache_plan_block: evicted lines are pending (an update must follow "
               "the last lookup first)");
    HA_REQUIRE(h->ahead_n < 0, "cache_plan_block: a ha_cache_sort_ahead is pending");
    for (int i = 0; i < count; ++i) {
        HA_REQUIRE(n[i] >= 0 && n[i] <= c.nmax && n[i] <= kSmallMax && (n[i] == 0 || keys[i]),
                   "cache_plan_block: batch %d of %ld keys (at most min(max_batch, %d))", i, (long)n[i], kSmallMax);
        HA_REQUIRE(c.policy != kLRU || n[i] <= c.limit, "cache_plan_block: limit (%ld) must be at least the batch (%ld keys): the "
                   "lines of an LRU batch are never evicted by its own lookup", (long)c.limit, (long)n[i]);
    }
    PlanSlot &sl = h->plan[h->plan_next % ha_cache::kPlanSlots];
    int blocks_out = 0;
    for (const PlanSlot &q : h->plan)
        blocks_out += q.count > 0 && q.next_call < q.total() ? 1 : 0;
    HA_REQUIRE(blocks_out < 2 && (sl.count == 0 || sl.next_call >= sl.total()),
               "cache_plan_block: two planned blocks are outstanding already");
    if (plan_slot_alloc(h, sl))
        return -1;
    if (!h->plan_xw) {
        HA_REQUIRE(dmalloc(&h->plan_xw, static_cast<size_t>(4 * kBookWg)) == 0, "cache_plan_block: out of device memory");
        h->allocs.push_back(h->plan_xw);
        if (dzero(h->plan_xw, 4 * kBookWg * 8))
            return -1;
        HA_CHECK_HIP(hipEventCreateWithFlags(&h->plan_fork, hipEventDisableTiming));
    }
    hipStream_t ss = as_stream(side), ms = as_stream(main);
    LfuTree tree{};
    if (c.policy != kLRU) {
        if (!h->lfu_lkey) {
            h->lfu_nblk = (c.S + kLfuBlk - 1) / kLfuBlk;
            HA_REQUIRE(dmalloc(&h->lfu_lkey, static_cast<size_t>(h->lfu_nblk * kLfuBlk)) == 0 &&
                       dmalloc(&h->lfu_bmin, static_cast<size_t>(h->lfu_nblk)) == 0 &&
                       dmalloc(&h->lfu_xk, static_cast<size_t>(kBookWg)) == 0 && dmalloc(&h->lfu_xb, static_cast<size_t>(kBookWg)) == 0,
                       "cache_plan_block: out of device memory");
            h->allocs.push_back(h->lfu_lkey);
            h->allocs.push_back(h->lfu_bmin);
            h->allocs.push_back(h->lfu_xk);
            h->allocs.push_back(h->lfu_xb);
        }
        tree = LfuTree{h->lfu_lkey, h->lfu_bmin, h->lfu_nblk, h->lfu_xk, h->lfu_xb};
        if (!h->lfu_tree_ok) {
            // the planned flow takes over from call-by-call calls (or starts): the lowest use bucket must be empty -- it is
            // after every lookup + update pair, not after a lookup without its update (see cache_book_lfu_kernel)
            HA_CHECK_HIP(hipStreamSynchronize(ms));
            CacheCtl ctl_h;
            HA_CHECK_HIP(hipMemcpy(&ctl_h, c.ctl, sizeof(ctl_h), hipMemcpyDeviceToHost));
            HA_REQUIRE(ctl_h.n_base == 0, "cache_plan_block: %ld lines are in the lowest use bucket (a lookup without its update "
                       "put them there): the planned flow of the LFU policies starts from a cache whose lines were all updated",
                       (long)ctl_h.n_base);
        }
    }
    if (ss != ms) {
        if (with_pk) {
            // push keys (and ids) are often written on `main` just before this call (the laia loader's gather): ALWAYS order
            // behind everything enqueued there so far, not only behind the rows of the block that used this slot before
            if (sl.rows_recorded)
                HA_CHECK_HIP(hipStreamWaitEvent(ss, sl.rows_done, 0));
            HA_CHECK_HIP(hipEventRecord(h->plan_fork, ms));
            HA_CHECK_HIP(hipStreamWaitEvent(ss, h->plan_fork, 0));
        } else if (sl.rows_recorded && h->last_planned_type >= 0) {
            // the planned flow goes on: this slot's buffers were last read by the rows of the block two before the one being
            // consumed -- nothing else of the row stream concerns the bookkeeping (it owns the control fields, the rows the
            // data fields), and this event is long complete: no barrier parked on the planning stream's queue
            HA_CHECK_HIP(hipStreamWaitEvent(ss, sl.rows_done, 0));
        } else {
            // the first blocks, or call-by-call entry points ran in between: everything enqueued on `main` so far comes first
            HA_CHECK_HIP(hipEventRecord(h->plan_fork, ms));
            HA_CHECK_HIP(hipStreamWaitEvent(ss, h->plan_fork, 0));
        }
    }
    // the block before this one was booked on whatever side stream its call named: order behind it
    PlanSlot &other = h->plan[(h->plan_next + ha_cache::kPlanSlots - 1) % ha_cache::kPlanSlots];
    if (other.count > 0 && other.booked_on != ss)
        HA_CHECK_HIP(hipStreamWaitEvent(ss, other.booked, 0));
    const uint64_t lim = static_cast<uint64_t>(c.length);
    if (key_kind == 0 ? ha_plan_build_batch_f32ids_lim(reinterpret_cast<const float *const *>(keys), n, sl.ws, count, lim, side)
                      : ha_plan_build_batch_u64ids_lim(reinterpret_cast<const uint64_t *const *>(keys), n, sl.ws, count, lim, side))
        return -1;
    BookArgs a;
    memset(&a, 0, sizeof(a));
    a.count = count;
    PushMarkArgs pm;
    memset(&pm, 0, sizeof(pm));
    pm.kind = push_kind;
    long long np_max = 0, z0 = -1, z1 = 0;      // the marks to clear: [z0, z1) of pk_mark (one fill for the block)
    for (int i = 0; i < count; ++i) {
        PlanPtrs p = plan_layout(sl.ws[i], n[i]);
        a.n[i] = static_cast<int>(n[i]);
        a.hdr[i] = p.hdr;
        a.uniq[i] = p.uniq;
        a.counts[i] = p.counts;
        sl.n[i] = n[i];
        sl.pk[i] = with_pk && n_push[i] >= 0;
        if (sl.pk[i]) {
            uint8_t *mark = sl.pk_mark + static_cast<long long>(i) * c.nmax;
            a.pk_mark[i] = mark;
            if (n[i] > 0) {
                z0 = z0 < 0 ? static_cast<long long>(i) * c.nmax : z0;
                z1 = static_cast<long long>(i) * c.nmax + n[i];
                if (n_push[i] > 0) {
                    pm.keys[i] = push_keys[i];
                    pm.n[i] = n_push[i];
                    pm.hdr[i] = p.hdr;
                    pm.uniq[i] = p.uniq;
                    pm.nb[i] = static_cast<int>(n[i]);
                    np_max = n_push[i] > np_max ? n_push[i] : np_max;
                }
            }
        }
    }
    if (z0 >= 0)
        HA_CHECK_HIP(hipMemsetAsync(sl.pk_mark + z0, 0, static_cast<size_t>(z1 - z0), ss));
    if (np_max > 0)
        hipLaunchKernelGGL(cache_plan_push_mark_kernel, dim3(static_cast<unsigned>((np_max + 255) / 256), count), dim3(256), 0, ss,
                           pm, sl.pk_mark, (long long)c.nmax);
    a.it_slot = sl.it_slot; a.it_flag = sl.it_flag; a.it_upd = sl.it_upd;
    a.ev_slot = sl.ev_slot; a.ev_key = sl.ev_key; a.ev_upd = sl.ev_upd;
    a.rec = sl.rec;
    a.xw = h->plan_xw;
    a.nmax = c.nmax;
    if (c.policy == kLRU) {
        hipLaunchKernelGGL(cache_book_block_kernel, dim3(kBookWg), dim3(kBookThreads), 0, ss, c, a);
    } else {
        if (!h->lfu_tree_ok) {
            hipLaunchKernelGGL(cache_lfu_keys_kernel, dim3(static_cast<unsigned>((tree.nblk * kLfuBlk + 255) / 256)), dim3(256), 0, ss,
                               c, tree);
            hipLaunchKernelGGL(cache_lfu_mins_kernel, dim3(static_cast<unsigned>((tree.nblk + 255) / 256)), dim3(256), 0, ss, tree);
            h->lfu_tree_ok = true;
        }
        hipLaunchKernelGGL(cache_book_lfu_kernel, dim3(kBookWg), dim3(kBookThreads), 0, ss, c, a, tree);
    }
    {   // the items per sorted position
        PlanExpandPtrs ep;
        int nmx = 1;
        for (int i = 0; i < count; ++i) {
            PlanPtrs p = plan_layout(sl.ws[i], n[i]);
            ep.upos[i] = p.upos;
            ep.perm[i] = p.perm;
            nmx = n[i] > nmx ? static_cast<int>(n[i]) : nmx;
        }
        hipLaunchKernelGGL(cache_plan_expand_kernel, dim3((nmx + 255) / 256, count), dim3(256), 0, ss, a, ep, sl.pos_item,
                           sl.it_upd_pos);
    }
    HA_LAUNCH_CHECK();
    HA_CHECK_HIP(hipEventRecord(sl.booked, ss));
    sl.booked_on = ss;
    sl.count = count;
    sl.next_call = 0;
    sl.waited = false;
    sl.pp = false;
    h->plan_next += 1;
    h->plan_n = -1;
    h->same_fast = false;
    h->ring_count = h->ring_head = 0;
    return 0;
}

extern "C" int ha_cache_plan_block(ha_cache *h, const void *const *keys, int key_kind, const int64_t *n, int count,
                                   ha_stream_t side, ha_stream_t main) {
    return plan_block_impl(h, keys, key_kind, n, nullptr, 0, nullptr, count, side, main);
}

extern "C" int ha_cache_plan_block_push_keys(ha_cache *h, const void *const *keys, int key_kind, const int64_t *n,
                                             const void *const *push_keys, int push_kind, const int64_t *n_push, int count,
                                             ha_stream_t side, ha_stream_t main) {
    HA_REQUIRE(push_keys && n_push, "cache_plan_block_push_keys: push_keys and n_push are required");
    return plan_block_impl(h, keys, key_kind, n, push_keys, push_kind, n_push, count, side, main);
}

static int plan_slot_alloc_chain(ha_cache *h, PlanSlot &sl) {
    if (sl.q_slot)
        return 0;
    const size_t all = static_cast<size_t>(h->c.nmax) * kPlanBlockMax;
    HA_REQUIRE(dmalloc(&sl.q_slot, all) == 0 && dmalloc(&sl.q_flag, all) == 0 && dmalloc(&sl.q_upd, all) == 0 &&
               dmalloc(&sl.q_pos_item, all) == 0 && dmalloc(&sl.q_upd_pos, all) == 0, "cache_plan_block_push_pull: out of device memory");
    h->allocs.push_back(sl.q_slot);
    h->allocs.push_back(sl.q_flag);
    h->allocs.push_back(sl.q_upd);
    h->allocs.push_back(sl.q_pos_item);
    h->allocs.push_back(sl.q_upd_pos);
    return 0;
}

// The bookkeeping of the next `count` (1..16) steps of a push-pull chain, see the header (include/herald_amd.h) and
// cache_book_chain_kernel.  Everything is checked before anything is enqueued.
extern "C" int ha_cache_plan_block_push_pull(ha_cache *h, const void *const *keys, int key_kind, const int64_t *n, int count,
                                             ha_stream_t side, ha_stream_t main) {
    HA_REQUIRE(h && keys && n && (key_kind == 0 || key_kind == 1) && count >= 1 && count <= kPlanBlockMax,
               "cache_plan_block_push_pull: bad arguments (1..%d entries)", kPlanBlockMax);
    Cache &c = h->c;
    HA_REQUIRE(c.policy == kLRU, "cache_plan_block_push_pull: LRU only (the planned bookkeeping of LFU / LFUOpt rests on lookup + "
               "update pairs of the same keys; those policies keep the call-by-call ha_cache_push_pull)");
    HA_REQUIRE(c.table && !c.remote && !c.bypass, "cache_plan_block_push_pull: a cache over a local store, not bypassed");
    HA_REQUIRE(c.row_start == 0 && c.store_rows >= c.length, "cache_plan_block_push_pull: the store must hold every key of the cache's range");
    HA_REQUIRE(c.limit >= 1, "cache_plan_block_push_pull: an empty cache");
    HA_REQUIRE(h->ahead_n < 0, "cache_plan_block_push_pull: a ha_cache_sort_ahead is pending");
    HA_REQUIRE(h->chain_open || (ha_cache_plan_pending(h) == 0 && h->evict_empty),
               "cache_plan_block_push_pull: a chain starts from a cache without planned calls outstanding and without pending evicted "
               "lines (an update must follow the last lookup first)");
    const bool closes = n[count - 1] < 0;
    bool have_prev = h->chain_open;
    int64_t prev_n = h->chain_n;
    for (int i = 0; i < count; ++i) {
        const bool close_i = n[i] < 0;
        HA_REQUIRE(!close_i || i == count - 1, "cache_plan_block_push_pull: entry %d closes the chain, but only the last entry of a "
                   "block may", i);
        HA_REQUIRE(!close_i || have_prev, "cache_plan_block_push_pull: no chain is open (nothing to close)");
        HA_REQUIRE(close_i || (n[i] <= c.nmax && n[i] <= kSmallMax && (n[i] == 0 || keys[i])),
                   "cache_plan_block_push_pull: batch %d of %ld keys (at most min(max_batch, %d))", i, (long)n[i], kSmallMax);
        const int64_t np = close_i ? 0 : n[i], nq = have_prev ? prev_n : 0;
        HA_REQUIRE(np + nq <= c.limit, "cache_plan_block_push_pull: step %d pulls %ld and pushes %ld keys, limit is %ld: n_pull + "
                   "n_push must not exceed limit (no line a step touches is evicted by the step's own insert)", i, (long)np, (long)nq,
                   (long)c.limit);
        have_prev = !close_i;
        prev_n = np;
    }
    PlanSlot &sl = h->plan[h->plan_next % ha_cache::kPlanSlots];
    int blocks_out = 0;
    for (const PlanSlot &q : h->plan)
        blocks_out += q.count > 0 && q.next_call < q.total() ? 1 : 0;
    HA_REQUIRE(blocks_out < 2 && (sl.count == 0 || sl.next_call >= sl.total()),
               "cache_plan_block_push_pull: two planned blocks are outstanding already");
    if (plan_slot_alloc(h, sl) || plan_slot_alloc_chain(h, sl))
        return -1;
    if (!h->plan_xw) {
        HA_REQUIRE(dmalloc(&h->plan_xw, static_cast<size_t>(4 * kBookWg)) == 0, "cache_plan_block_push_pull: out of device memory");
        h->allocs.push_back(h->plan_xw);
        if (dzero(h->plan_xw, 4 * kBookWg * 8))
            return -1;
        HA_CHECK_HIP(hipEventCreateWithFlags(&h->plan_fork, hipEventDisableTiming));
    }
    hipStream_t ss = as_stream(side), ms = as_stream(main);
    if (ss != ms) {
        // ids are often written on `main` just before this call: ALWAYS behind everything enqueued there so far
        if (sl.rows_recorded)
            HA_CHECK_HIP(hipStreamWaitEvent(ss, sl.rows_done, 0));
        HA_CHECK_HIP(hipEventRecord(h->plan_fork, ms));
        HA_CHECK_HIP(hipStreamWaitEvent(ss, h->plan_fork, 0));
    }
    PlanSlot &other = h->plan[(h->plan_next + ha_cache::kPlanSlots - 1) % ha_cache::kPlanSlots];
    if (other.count > 0 && other.booked_on != ss)
        HA_CHECK_HIP(hipStreamWaitEvent(ss, other.booked, 0));
    const int built = count - (closes ? 1 : 0);
    const uint64_t lim = static_cast<uint64_t>(c.length);
    if (built > 0 &&
        (key_kind == 0 ? ha_plan_build_batch_f32ids_lim(reinterpret_cast<const float *const *>(keys), n, sl.ws, built, lim, side)
                       : ha_plan_build_batch_u64ids_lim(reinterpret_cast<const uint64_t *const *>(keys), n, sl.ws, built, lim, side)))
        return -1;
    ChainArgs a;
    memset(&a, 0, sizeof(a));
    ChainExpandPtrs ep;
    memset(&ep, 0, sizeof(ep));
    a.count = count;
    have_prev = h->chain_open;
    int nmx = 1;
    for (int i = 0; i < count; ++i) {
        const bool close_i = n[i] < 0;
        const long long at = static_cast<long long>(i) * c.nmax;
        sl.kind[i] = close_i ? kChainClose : have_prev ? kChainStep : kChainHead;
        sl.n[i] = close_i ? -1 : n[i];
        sl.pk[i] = false;
        a.n_p[i] = close_i ? -1 : static_cast<int>(n[i]);
        if (!close_i) {
            PlanPtrs p = plan_layout(sl.ws[i], n[i]);
            a.hdr_p[i] = p.hdr;
            a.uniq_p[i] = p.uniq;
            ep.n[0][i] = static_cast<int>(n[i]);
            ep.uniq[0][i] = p.uniq;
            ep.upos[0][i] = p.upos;
            ep.perm[0][i] = p.perm;
            nmx = n[i] > nmx ? static_cast<int>(n[i]) : nmx;
        }
        sl.q_n[i] = have_prev ? h->chain_n : 0;
        if (have_prev) {
            sl.q_ws[i] = h->chain_ws;
            sl.q_pver[i] = h->chain_pver;
            sl.q_ev_slot[i] = h->chain_ev_slot;
            sl.q_ev_key[i] = h->chain_ev_key;
            sl.q_ev_upd[i] = h->chain_ev_upd;
            sl.q_rec[i] = h->chain_rec;
            PlanPtrs q = plan_layout(h->chain_ws, h->chain_n);
            a.n_q[i] = static_cast<int>(h->chain_n);
            a.hdr_q[i] = q.hdr;
            a.uniq_q[i] = q.uniq;
            a.counts_q[i] = q.counts;
            ep.n[1][i] = static_cast<int>(h->chain_n);
            ep.uniq[1][i] = q.uniq;
            ep.upos[1][i] = q.upos;
            ep.perm[1][i] = q.perm;
            nmx = h->chain_n > nmx ? static_cast<int>(h->chain_n) : nmx;
        }
        have_prev = !close_i;
        if (have_prev) {
            h->chain_n = n[i];
            h->chain_ws = sl.ws[i];
            h->chain_pver = sl.pver + at;
            h->chain_ev_slot = sl.ev_slot + at;
            h->chain_ev_key = sl.ev_key + at;
            h->chain_ev_upd = sl.ev_upd + at;
            h->chain_rec = sl.rec + i;
        }
    }
    h->chain_open = have_prev;
    a.it_slot = sl.it_slot; a.it_flag = sl.it_flag; a.it_upd = sl.it_upd;
    a.q_slot = sl.q_slot; a.q_flag = sl.q_flag; a.q_upd = sl.q_upd;
    a.ev_slot = sl.ev_slot; a.ev_key = sl.ev_key; a.ev_upd = sl.ev_upd;
    a.rec = sl.rec;
    a.xw = h->plan_xw;
    a.nmax = c.nmax;
    a.step0 = h->chain_step;
    h->chain_step += static_cast<unsigned long long>(count);
    hipLaunchKernelGGL(cache_book_chain_kernel, dim3(kBookWg), dim3(kBookThreads), 0, ss, c, a);
    hipLaunchKernelGGL(cache_chain_expand_kernel, dim3((nmx + 255) / 256, count, 2), dim3(256), 0, ss, a, ep, sl.pos_item,
                       sl.it_upd_pos, sl.q_pos_item, sl.q_upd_pos);
    HA_LAUNCH_CHECK();
    HA_CHECK_HIP(hipEventRecord(sl.booked, ss));
    sl.booked_on = ss;
    sl.count = count;
    sl.next_call = 0;
    sl.waited = false;
    sl.pp = true;
    h->plan_next += 1;
    h->plan_n = -1;
    h->same_fast = false;
    h->ring_count = h->ring_head = 0;
    h->evict_empty = false;       // (the chain's evicted lines wait for the next step; its closing update leaves none)
    h->lfu_tree_ok = false;
    return 0;
}

// the slot and entry index of the next planned call of `type` (0 lookup, 1 update, 2 push-pull); nullptr: another call is due
static PlanSlot *plan_current(ha_cache *h, int type, int *idx) {
    for (int k = 0; k < ha_cache::kPlanSlots; ++k) {         // the older block first
        PlanSlot &sl = h->plan[(h->plan_next + k) % ha_cache::kPlanSlots];
        if (sl.count > 0 && sl.next_call < sl.total()) {
            if (sl.pp) {
                if (sl.kind[sl.next_call] != (type == 0 ? kChainHead : type == 1 ? kChainClose : kChainStep))
                    return nullptr;
                *idx = sl.next_call;
                return &sl;
            }
            if (type > 1 || (sl.next_call & 1) != type)
                return nullptr;
            *idx = sl.next_call >> 1;
            return &sl;
        }
    }
    return nullptr;
}

// the planned call (slot, entry, type) is enqueued
static int plan_called(ha_cache *h, PlanSlot *sl, int i, int type, hipStream_t s) {
    sl->next_call += 1;
    if (sl->next_call == sl->total()) {       // the block's last row launch is enqueued
        HA_CHECK_HIP(hipEventRecord(sl->rows_done, s));
        sl->rows_recorded = true;
    }
    h->last_planned = sl;
    h->last_planned_idx = i;
    h->last_planned_type = type;
    return 0;
}

// the row launch of a planned lookup / of a chain step's pull half (vadj != nullptr)
static int lookup_rows(ha_cache *h, hipStream_t s, const int4 *pos_item, int64_t n, float *dest, long long *pver,
                       const PlanRec *rec, const int32_t *vadj) {
    Cache &c = h->c;
    const unsigned blocks = static_cast<unsigned>((n + 15) / 16);
    const bool vec_ok = (c.width % 4 == 0) && (reinterpret_cast<uintptr_t>(dest) % 16 == 0) &&
                        (reinterpret_cast<uintptr_t>(c.table) % 16 == 0);
    if (vadj == nullptr) {
        if (vec_ok)
            hipLaunchKernelGGL((cache_lookup_planned_kernel<4, false>), dim3(blocks), dim3(1024), 0, s, c, pos_item, (long long)n,
                               dest, pver, rec, vadj);
        else
            hipLaunchKernelGGL((cache_lookup_planned_kernel<1, false>), dim3(blocks), dim3(1024), 0, s, c, pos_item, (long long)n,
                               dest, pver, rec, vadj);
    } else {
        if (vec_ok)
            hipLaunchKernelGGL((cache_lookup_planned_kernel<4, true>), dim3(blocks), dim3(1024), 0, s, c, pos_item, (long long)n,
                               dest, pver, rec, vadj);
        else
            hipLaunchKernelGGL((cache_lookup_planned_kernel<1, true>), dim3(blocks), dim3(1024), 0, s, c, pos_item, (long long)n,
                               dest, pver, rec, vadj);
    }
    HA_LAUNCH_CHECK();
    return 0;
}

// the row launch of a planned update / of a chain step's push half: the batch's index plan `ws`, its items per sorted position,
// the versions its lookup staged, the evicted dirty lines to push with it (rec->E of them)
// (bag >= 1 or bag_of: `grads` is the pooled gradient, see cache_update_planned_kernel's BAGS)
static int update_rows(ha_cache *h, hipStream_t s, void *ws, int64_t n, const float *grads, const int4 *pos_item,
                       const int32_t *it_upd_pos, const long long *pver, const int32_t *ev_slot, const uint32_t *ev_key,
                       const int32_t *ev_upd, const PlanRec *rec, int pkmode, int64_t bag = 0, const int32_t *bag_of = nullptr) {
    Cache &c = h->c;
    PlanPtrs p = plan_layout(ws, n);
    const int apply_blocks = static_cast<int>((n + kPosPerBlock - 1) / kPosPerBlock);
    ApplyMaps maps{};
    maps.dst2 = c.data;
    maps.push_tab = c.table;
    maps.push_rows = static_cast<uint64_t>(c.store_rows);
    maps.pos_item = pos_item;
    maps.victim_row = reinterpret_cast<const int *>(&rec->vh_slot);
    const bool vec_ok = (c.width % 4 == 0) && (reinterpret_cast<uintptr_t>(grads) % 16 == 0) &&
                        (reinterpret_cast<uintptr_t>(c.table) % 16 == 0);
    const dim3 grid(static_cast<unsigned>(apply_blocks + kPlanEvictBlocks + kPlanMetaBlocks));
    if (bag >= 1 || bag_of != nullptr) {
        maps.valmap = bag_of;
        maps.valdiv = bag_of ? 0 : static_cast<int>(bag);
        if (vec_ok)
            hipLaunchKernelGGL((cache_update_planned_kernel<4, true>), grid, dim3(1024), kApplyLdsBytes, s, c, p.sorted, p.perm,
                               (int)n, grads, maps, it_upd_pos, pver, ev_slot, ev_key, ev_upd, rec, pkmode, WbagArgs{});
        else
            hipLaunchKernelGGL((cache_update_planned_kernel<1, true>), grid, dim3(1024), kApplyLdsBytes, s, c, p.sorted, p.perm,
                               (int)n, grads, maps, it_upd_pos, pver, ev_slot, ev_key, ev_upd, rec, pkmode, WbagArgs{});
        HA_LAUNCH_CHECK();
        return 0;
    }
    if (vec_ok)
        hipLaunchKernelGGL(cache_update_planned_kernel<4>, grid, dim3(1024), kApplyLdsBytes, s, c, p.sorted, p.perm, (int)n,
                           grads, maps, it_upd_pos, pver, ev_slot, ev_key, ev_upd, rec, pkmode, WbagArgs{});
    else
        hipLaunchKernelGGL(cache_update_planned_kernel<1>, grid, dim3(1024), kApplyLdsBytes, s, c, p.sorted, p.perm, (int)n,
                           grads, maps, it_upd_pos, pver, ev_slot, ev_key, ev_upd, rec, pkmode, WbagArgs{});
    HA_LAUNCH_CHECK();
    return 0;
}
// the row launch of a planned update from weighted bags (cache_update_planned_kernel<.., WEIGHTED>): update_rows' arguments,
// the pooled gradient [nbags, width], the n weights and the scale
static int update_rows_wbags(ha_cache *h, hipStream_t s, void *ws, int64_t n, const float *bag_grads, const float *weights,
                             float scale, int64_t nbags, const int4 *pos_item, const int32_t *it_upd_pos, const long long *pver,
                             const int32_t *ev_slot, const uint32_t *ev_key, const int32_t *ev_upd, const PlanRec *rec, int pkmode,
                             int64_t bag, const int32_t *bag_of) {
    Cache &c = h->c;
    PlanPtrs p = plan_layout(ws, n);
    const int apply_blocks = static_cast<int>((n + kPosPerBlock - 1) / kPosPerBlock);
    ApplyMaps maps{};
    maps.dst2 = c.data;
    maps.push_tab = c.table;
    maps.push_rows = static_cast<uint64_t>(c.store_rows);
    maps.pos_item = pos_item;
    maps.victim_row = reinterpret_cast<const int *>(&rec->vh_slot);
    maps.valmap = bag_of;
    maps.valdiv = bag_of ? 0 : static_cast<int>(bag);
    const bool vec_ok = (c.width % 4 == 0) && (reinterpret_cast<uintptr_t>(bag_grads) % 16 == 0) &&
                        (reinterpret_cast<uintptr_t>(c.table) % 16 == 0);
    const dim3 grid(static_cast<unsigned>(apply_blocks + kPlanEvictBlocks + kPlanMetaBlocks));
    const WbagArgs wa{weights, scale, static_cast<uint32_t>(nbags)};
    if (vec_ok)
        hipLaunchKernelGGL((cache_update_planned_kernel<4, true, true>), grid, dim3(1024), 0, s, c, p.sorted, p.perm, (int)n,
                           bag_grads, maps, it_upd_pos, pver, ev_slot, ev_key, ev_upd, rec, pkmode, wa);
    else
        hipLaunchKernelGGL((cache_update_planned_kernel<1, true, true>), grid, dim3(1024), 0, s, c, p.sorted, p.perm, (int)n,
                           bag_grads, maps, it_upd_pos, pver, ev_slot, ev_key, ev_upd, rec, pkmode, wa);
    HA_LAUNCH_CHECK();
    return 0;
}
// ... of entry i of a chain block: the push half (the batch of the entry before)
// (bag >= 1 or bag_of: `grads` is the pooled gradient of that batch)
static int chain_push_rows(ha_cache *h, hipStream_t s, PlanSlot *sl, int i, const float *grads, int64_t bag = 0,
                           const int32_t *bag_of = nullptr) {
    const long long at = static_cast<long long>(i) * h->c.nmax;
    return update_rows(h, s, sl->q_ws[i], sl->q_n[i], grads, sl->q_pos_item + at, sl->q_upd_pos + at, sl->q_pver[i],
                       sl->q_ev_slot[i], sl->q_ev_key[i], sl->q_ev_upd[i], sl->q_rec[i], 0, bag, bag_of);
}

// the launch shape of the pooled lookup: the slice of the 16-byte path by bag_sum_launch's rule (bagsum.hip) -> workgroups
static uint64_t sum_blocks(const Cache &c, int64_t nbags, const float *out, int *vec_out, uint32_t *nslice_out) {
    const int64_t width = c.width;
    const bool vec_ok = (width % 4 == 0) && (reinterpret_cast<uintptr_t>(c.table) % 16 == 0) &&
                        (reinterpret_cast<uintptr_t>(out) % 16 == 0);
    int vec = 1;
    if (vec_ok)
        for (vec = 4; vec > 1; vec >>= 1)
            if (kWave * vec <= width && nbags * ((width + kWave * vec - 1) / (kWave * vec)) >= 2048)
                break;
    const uint32_t nslice = static_cast<uint32_t>((width + kWave * vec - 1) / (kWave * vec));
    *vec_out = vec;
    *nslice_out = nslice;
    return (static_cast<uint64_t>(nbags) * nslice + kSumWaves - 1) / kSumWaves;
}

// the row launch of a planned lookup delivered sum-pooled (entry i of the slot) / of a chain step's pooled pull half (pp)
// (weights != nullptr: the weighted form, cache_lookup_sum_planned_kernel<.., WEIGHTED>; never with pp)
static int lookup_sum_rows(ha_cache *h, hipStream_t s, PlanSlot *sl, int i, int64_t n, int64_t nbags, int64_t bag,
                           const int64_t *offsets, float *out, bool pp, const char *who, const float *weights = nullptr) {
    Cache &c = h->c;
    const long long at = static_cast<long long>(i) * c.nmax;
    PlanPtrs p = plan_layout(sl->ws[i], n);
    SumPlan sp{sl->it_slot + at, sl->it_flag + at, p.uniq, p.inverse, p.seg, p.perm, sl->pver + at, sl->rec + i,
               pp ? sl->it_upd + at : nullptr};
    int vec = 1;
    uint32_t nslice = 1;
    const uint64_t blocks64 = sum_blocks(c, nbags, out, &vec, &nslice);
    HA_REQUIRE(blocks64 < (1ull << 31), "%s: batch too large", who);
    const int64_t mean = offsets ? (n + nbags - 1) / nbags : bag;
    const bool few = mean <= 8;
    const dim3 grid(static_cast<unsigned>(blocks64)), block(kSumWaves * kWave);
#define HA_SUM_CASE(V, R)                                                                                                    \
    do {                                                                                                                     \
        if (weights)                                                                                                         \
            hipLaunchKernelGGL((cache_lookup_sum_planned_kernel<V, R, false, true>), grid, block, 0, s, c, sp, (long long)n, \
                               (long long)bag, offsets, (long long)nbags, nslice, out, weights);                             \
        else if (pp)                                                                                                         \
            hipLaunchKernelGGL((cache_lookup_sum_planned_kernel<V, R, true>), grid, block, 0, s, c, sp, (long long)n,        \
                               (long long)bag, offsets, (long long)nbags, nslice, out, (const float *)nullptr);              \
        else                                                                                                                 \
            hipLaunchKernelGGL((cache_lookup_sum_planned_kernel<V, R, false>), grid, block, 0, s, c, sp, (long long)n,       \
                               (long long)bag, offsets, (long long)nbags, nslice, out, (const float *)nullptr);              \
    } while (0)
    if (vec == 4) {
        if (few) HA_SUM_CASE(4, 8); else HA_SUM_CASE(4, 32);
    } else if (vec == 2) {
        if (few) HA_SUM_CASE(2, 8); else HA_SUM_CASE(2, 32);
    } else {
        if (few) HA_SUM_CASE(1, 8); else HA_SUM_CASE(1, 32);
    }
#undef HA_SUM_CASE
    HA_LAUNCH_CHECK();
    return 0;
}

extern "C" int ha_cache_lookup_planned(ha_cache *h, int64_t n, float *dest, ha_stream_t stream) {
    HA_REQUIRE(h, "cache_lookup_planned: null handle");
    int i = 0;
    PlanSlot *sl = plan_current(h, 0, &i);
    HA_REQUIRE(sl != nullptr, "cache_lookup_planned: no planned batch is due for its lookup (ha_cache_plan_block; lookup and "
               "update alternate; in a push-pull chain only the head is a lookup)");
    HA_REQUIRE(sl->n[i] == n && (n == 0 || dest), "cache_lookup_planned: the planned batch has %ld keys (got %ld)", (long)sl->n[i],
               (long)n);
    Cache &c = h->c;
    hipStream_t s = as_stream(stream);
    if (!sl->waited) {
        HA_CHECK_HIP(hipStreamWaitEvent(s, sl->booked, 0));
        sl->waited = true;
    }
    cache_mark(h, kTStart, s, true);
    if (n > 0) {
        const long long at = static_cast<long long>(i) * c.nmax;
        if (lookup_rows(h, s, sl->pos_item + at, n, dest, sl->pver + at, sl->rec + i, nullptr))
            return -1;
    }
    cache_mark(h, kTEnd, s);
    h->settle_slot = sl->pp ? sl : nullptr;
    h->settle_idx = i;
    return plan_called(h, sl, i, 0, s);
}

extern "C" int ha_cache_update_planned(ha_cache *h, int64_t n, const float *grads, ha_stream_t stream) {
    HA_REQUIRE(h, "cache_update_planned: null handle");
    int i = 0;
    PlanSlot *sl = plan_current(h, 1, &i);
    HA_REQUIRE(sl != nullptr, "cache_update_planned: no planned batch is due for its update (its lookup comes first; in a push-pull "
               "chain only the closing step is an update)");
    const int64_t planned_n = sl->pp ? sl->q_n[i] : sl->n[i];
    HA_REQUIRE(planned_n == n && (n == 0 || grads), "cache_update_planned: the planned batch has %ld keys (got %ld)", (long)planned_n,
               (long)n);
    Cache &c = h->c;
    hipStream_t s = as_stream(stream);
    if (!sl->waited) {       // (a chain block whose only entry closes the chain)
        HA_CHECK_HIP(hipStreamWaitEvent(s, sl->booked, 0));
        sl->waited = true;
    }
    cache_mark(h, kTStart, s, true);
    if (n > 0) {
        const long long at = static_cast<long long>(i) * c.nmax;
        if (sl->pp ? chain_push_rows(h, s, sl, i, grads)
                   : update_rows(h, s, sl->ws[i], n, grads, sl->pos_item + at, sl->it_upd_pos + at, sl->pver + at, sl->ev_slot + at,
                                 sl->ev_key + at, sl->ev_upd + at, sl->rec + i, sl->pk[i] ? 1 : 0))
            return -1;
    }
    cache_mark(h, kTEnd, s);
    h->settle_slot = nullptr;
    h->evict_empty = true;
    return plan_called(h, sl, i, 1, s);
}

// The lookup of the next planned batch, delivered sum-pooled (cache_lookup_sum_planned_kernel); takes ha_cache_lookup_planned's
// place in the slot's call sequence and leaves the cache in the same state.
extern "C" int ha_cache_lookup_sum_planned(ha_cache *h, int64_t n, int64_t nbags, int64_t bag, const int64_t *offsets, float *out,
                                           ha_stream_t stream) {
    HA_REQUIRE(h, "cache_lookup_sum_planned: null handle");
    HA_REQUIRE(n >= 0 && nbags >= 0 && nbags < (1ll << 31) && bag >= 0, "cache_lookup_sum_planned: bad sizes n=%ld nbags=%ld bag=%ld",
               (long)n, (long)nbags, (long)bag);
    HA_REQUIRE((bag >= 1) != (offsets != nullptr), "cache_lookup_sum_planned: give exactly one of bag >= 1 and offsets (bag=%ld, "
               "offsets %s)", (long)bag, offsets ? "given" : "null");
    HA_REQUIRE(offsets != nullptr || (n % bag == 0 && n / bag == nbags), "cache_lookup_sum_planned: n=%ld is not nbags=%ld bags of "
               "bag=%ld ids", (long)n, (long)nbags, (long)bag);
    HA_REQUIRE(n == 0 || nbags >= 1, "cache_lookup_sum_planned: %ld ids in no bag", (long)n);
    HA_REQUIRE(nbags == 0 || out, "cache_lookup_sum_planned: null output");
    int i = 0;
    PlanSlot *sl = plan_current(h, 0, &i);
    HA_REQUIRE(sl == nullptr || !sl->pp, "cache_lookup_sum_planned: the planned block is a push-pull chain (ha_cache_plan_block_push_pull): "
               "its steps are not pooled by this call -- ha_cache_push_pull_planned_bags serves the chain's entries pooled");
    HA_REQUIRE(!h->chain_open, "cache_lookup_sum_planned: a planned push-pull chain is open: its steps are not pooled by this call "
               "(ha_cache_push_pull_planned_bags)");
    HA_REQUIRE(sl != nullptr, "cache_lookup_sum_planned: no planned batch is due for its lookup (ha_cache_plan_block; lookup and "
               "update alternate)");
    HA_REQUIRE(sl->n[i] == n, "cache_lookup_sum_planned: the planned batch has %ld keys (got %ld)", (long)sl->n[i], (long)n);
    hipStream_t s = as_stream(stream);
    if (!sl->waited) {
        HA_CHECK_HIP(hipStreamWaitEvent(s, sl->booked, 0));
        sl->waited = true;
    }
    cache_mark(h, kTStart, s, true);
    if (nbags > 0 && lookup_sum_rows(h, s, sl, i, n, nbags, bag, offsets, out, false, "cache_lookup_sum_planned"))
        return -1;
    cache_mark(h, kTEnd, s);
    h->settle_slot = nullptr;
    h->settle_idx = i;
    return plan_called(h, sl, i, 0, s);
}

// The update of the planned batch from the POOLED gradient [nbags, width]: ha_cache_update_planned on the gradient expanded to
// [n, width], bit for bit, without the expansion (cache_update_planned_kernel<.., BAGS>).
extern "C" int ha_cache_update_planned_bags(ha_cache *h, int64_t n, const float *bag_grads, int64_t nbags, int64_t bag,
                                            const int32_t *bag_of, ha_stream_t stream) {
    HA_REQUIRE(h, "cache_update_planned_bags: null handle");
    HA_REQUIRE(n >= 0 && nbags >= 0 && nbags < (1ll << 31) && bag >= 0 && bag < (1ll << 31),
               "cache_update_planned_bags: bad sizes n=%ld nbags=%ld bag=%ld", (long)n, (long)nbags, (long)bag);
    // (an empty batch of ragged bags has no bag_of to give: neither is accepted then)
    HA_REQUIRE(n == 0 ? !(bag >= 1 && bag_of != nullptr) : (bag >= 1) != (bag_of != nullptr),
               "cache_update_planned_bags: give exactly one of bag >= 1 and bag_of (bag=%ld, bag_of %s)", (long)bag,
               bag_of ? "given" : "null");
    HA_REQUIRE(bag < 1 || (n % bag == 0 && n / bag == nbags), "cache_update_planned_bags: n=%ld is not nbags=%ld bags of "
               "bag=%ld ids", (long)n, (long)nbags, (long)bag);
    HA_REQUIRE(n == 0 || (nbags >= 1 && bag_grads), "cache_update_planned_bags: %ld ids, but no bags or no gradient", (long)n);
    int i = 0;
    PlanSlot *sl = plan_current(h, 1, &i);
    HA_REQUIRE(sl == nullptr || !sl->pp, "cache_update_planned_bags: the planned block is a push-pull chain "
               "(ha_cache_plan_block_push_pull): its steps are not pooled by this call -- ha_cache_push_pull_planned_bags serves the "
               "chain's entries pooled");
    HA_REQUIRE(!h->chain_open, "cache_update_planned_bags: a planned push-pull chain is open: its steps are not pooled by this call "
               "(ha_cache_push_pull_planned_bags)");
    HA_REQUIRE(sl != nullptr, "cache_update_planned_bags: no planned batch is due for its update (its lookup comes first)");
    HA_REQUIRE(sl->n[i] == n, "cache_update_planned_bags: the planned batch has %ld keys (got %ld)", (long)sl->n[i], (long)n);
    Cache &c = h->c;
    hipStream_t s = as_stream(stream);
    cache_mark(h, kTStart, s, true);
    if (n > 0) {
        const long long at = static_cast<long long>(i) * c.nmax;
        if (update_rows(h, s, sl->ws[i], n, bag_grads, sl->pos_item + at, sl->it_upd_pos + at, sl->pver + at, sl->ev_slot + at,
                        sl->ev_key + at, sl->ev_upd + at, sl->rec + i, sl->pk[i] ? 1 : 0, bag_of ? 0 : bag, bag_of))
            return -1;
    }
    cache_mark(h, kTEnd, s);
    h->settle_slot = nullptr;
    h->evict_empty = true;
    return plan_called(h, sl, i, 1, s);
}

// The lookup of the next planned batch, delivered as WEIGHTED sums of its bags (cache_lookup_sum_planned_kernel<.., WEIGHTED>):
// per bag and column acc = +0, then acc = fl(acc + fl(w_j * r_j)) over the occurrences with w_j != 0 in position order, r_j the row
// ha_cache_lookup_planned writes.  weights: n floats on the device.  Takes ha_cache_lookup_planned's place in the slot's call
// sequence and leaves the cache in the same state, whatever the weights are.
extern "C" int ha_cache_lookup_wsum_planned(ha_cache *h, int64_t n, int64_t nbags, int64_t bag, const int64_t *offsets,
                                            const float *weights, float *out, ha_stream_t stream) {
    HA_REQUIRE(h, "cache_lookup_wsum_planned: null handle");
    HA_REQUIRE(n >= 0 && nbags >= 0 && nbags < (1ll << 31) && bag >= 0, "cache_lookup_wsum_planned: bad sizes n=%ld nbags=%ld bag=%ld",
               (long)n, (long)nbags, (long)bag);
    HA_REQUIRE((bag >= 1) != (offsets != nullptr), "cache_lookup_wsum_planned: give exactly one of bag >= 1 and offsets (bag=%ld, "
               "offsets %s)", (long)bag, offsets ? "given" : "null");
    HA_REQUIRE(offsets != nullptr || (n % bag == 0 && n / bag == nbags), "cache_lookup_wsum_planned: n=%ld is not nbags=%ld bags of "
               "bag=%ld ids", (long)n, (long)nbags, (long)bag);
    HA_REQUIRE(n == 0 || nbags >= 1, "cache_lookup_wsum_planned: %ld ids in no bag", (long)n);
    HA_REQUIRE(nbags == 0 || out, "cache_lookup_wsum_planned: null output");
    HA_REQUIRE(n == 0 || weights, "cache_lookup_wsum_planned: %ld ids, but no weights", (long)n);
    int i = 0;
    PlanSlot *sl = plan_current(h, 0, &i);
    HA_REQUIRE(sl == nullptr || !sl->pp, "cache_lookup_wsum_planned: the planned block is a push-pull chain (ha_cache_plan_block_push_pull): "
               "its steps are not pooled by this call -- ha_cache_push_pull_planned_bags serves the chain's entries pooled");
    HA_REQUIRE(!h->chain_open, "cache_lookup_wsum_planned: a planned push-pull chain is open: its steps are not pooled by this call "
               "(ha_cache_push_pull_planned_bags)");
    HA_REQUIRE(sl != nullptr, "cache_lookup_wsum_planned: no planned batch is due for its lookup (ha_cache_plan_block; lookup and "
               "update alternate)");
    HA_REQUIRE(sl->n[i] == n, "cache_lookup_wsum_planned: the planned batch has %ld keys (got %ld)", (long)sl->n[i], (long)n);
    if (nbags > 0) {
        int vec = 1;
        uint32_t nslice = 1;
        HA_REQUIRE(sum_blocks(h->c, nbags, out, &vec, &nslice) < (1ull << 31), "cache_lookup_wsum_planned: batch too large");
    }
    hipStream_t s = as_stream(stream);
    if (!sl->waited) {
        HA_CHECK_HIP(hipStreamWaitEvent(s, sl->booked, 0));
        sl->waited = true;
    }
    cache_mark(h, kTStart, s, true);
    // (n == 0 with bags to fill: every bag is empty and its sum is zeros with or without weights -- the unweighted launch)
    if (nbags > 0 && lookup_sum_rows(h, s, sl, i, n, nbags, bag, offsets, out, false, "cache_lookup_wsum_planned",
                                     n > 0 ? weights : nullptr))
        return -1;
    cache_mark(h, kTEnd, s);
    h->settle_slot = nullptr;
    h->settle_idx = i;
    return plan_called(h, sl, i, 0, s);
}

// The update of the planned batch from the pooled gradient [nbags, width] of WEIGHTED bags: ha_cache_update_planned on the
// [n, width] tensor whose row i is fl(scale * fl(w_i * bag_grads[bag(i), :])) for w_i != 0 and fl(scale * +0) otherwise -- what
// ha_wbag_grad_rows followed by a multiplication by scale produces --, bit for bit, without that tensor
// (cache_update_planned_kernel<.., WEIGHTED>).  weights: n floats on the device; scale must be finite.  The bookkeeping, the versions
// and which lines are pushed do not depend on the weights.
extern "C" int ha_cache_update_planned_wbags(ha_cache *h, int64_t n, const float *bag_grads, const float *weights, float scale,
                                             int64_t nbags, int64_t bag, const int32_t *bag_of, ha_stream_t stream) {
    HA_REQUIRE(h, "cache_update_planned_wbags: null handle");
    HA_REQUIRE(n >= 0 && nbags >= 0 && nbags < (1ll << 31) && bag >= 0 && bag < (1ll << 31),
               "cache_update_planned_wbags: bad sizes n=%ld nbags=%ld bag=%ld", (long)n, (long)nbags, (long)bag);
    HA_REQUIRE(std::isfinite(scale), "cache_update_planned_wbags: scale must be finite (got %g)", (double)scale);
    // (an empty batch of ragged bags has no bag_of to give: neither is accepted then)
    HA_REQUIRE(n == 0 ? !(bag >= 1 && bag_of != nullptr) : (bag >= 1) != (bag_of != nullptr),
               "cache_update_planned_wbags: give exactly one of bag >= 1 and bag_of (bag=%ld, bag_of %s)", (long)bag,
               bag_of ? "given" : "null");
    HA_REQUIRE(bag < 1 || (n % bag == 0 && n / bag == nbags), "cache_update_planned_wbags: n=%ld is not nbags=%ld bags of "
               "bag=%ld ids", (long)n, (long)nbags, (long)bag);
    HA_REQUIRE(n == 0 || (nbags >= 1 && bag_grads && weights), "cache_update_planned_wbags: %ld ids, but no bags, no gradient or "
               "no weights", (long)n);
    int i = 0;
    PlanSlot *sl = plan_current(h, 1, &i);
    HA_REQUIRE(sl == nullptr || !sl->pp, "cache_update_planned_wbags: the planned block is a push-pull chain "
               "(ha_cache_plan_block_push_pull): its steps are not pooled by this call -- ha_cache_push_pull_planned_bags serves the "
               "chain's entries pooled");
    HA_REQUIRE(!h->chain_open, "cache_update_planned_wbags: a planned push-pull chain is open: its steps are not pooled by this call "
               "(ha_cache_push_pull_planned_bags)");
    HA_REQUIRE(sl != nullptr, "cache_update_planned_wbags: no planned batch is due for its update (its lookup comes first)");
    HA_REQUIRE(sl->n[i] == n, "cache_update_planned_wbags: the planned batch has %ld keys (got %ld)", (long)sl->n[i], (long)n);
    Cache &c = h->c;
    hipStream_t s = as_stream(stream);
    cache_mark(h, kTStart, s, true);
    if (n > 0) {
        const long long at = static_cast<long long>(i) * c.nmax;
        if (update_rows_wbags(h, s, sl->ws[i], n, bag_grads, weights, scale, nbags, sl->pos_item + at, sl->it_upd_pos + at,
                              sl->pver + at, sl->ev_slot + at, sl->ev_key + at, sl->ev_upd + at, sl->rec + i, sl->pk[i] ? 1 : 0,
                              bag_of ? 0 : bag, bag_of))
            return -1;
    }
    cache_mark(h, kTEnd, s);
    h->settle_slot = nullptr;
    h->evict_empty = true;
    return plan_called(h, sl, i, 1, s);
}

// A middle step of a push-pull chain (cache.cc:356-422): the push half of the batch pulled by the step before -- ordered
// accumulate, the pushed lines' and the pending evicted lines' store side, versions -- then the pull half of the step's own
// batch, whose staleness decision takes the push half's version commit back (cache_lookup_planned_kernel<.., PP>).  Two
// launches on `stream`, no bookkeeping.
extern "C" int ha_cache_push_pull_planned(ha_cache *h, int64_t n_pull, float *dest, int64_t n_push, const float *grads,
                                          ha_stream_t stream) {
    HA_REQUIRE(h, "cache_push_pull_planned: null handle");
    int i = 0;
    PlanSlot *sl = plan_current(h, 2, &i);
    HA_REQUIRE(sl != nullptr, "cache_push_pull_planned: no push-pull step is due (ha_cache_plan_block_push_pull; the chain's head "
               "is ha_cache_lookup_planned, its closing step ha_cache_update_planned)");
    HA_REQUIRE(sl->n[i] == n_pull && sl->q_n[i] == n_push && (n_pull == 0 || dest) && (n_push == 0 || grads),
               "cache_push_pull_planned: the planned step pulls %ld and pushes %ld keys (got %ld, %ld)", (long)sl->n[i],
               (long)sl->q_n[i], (long)n_pull, (long)n_push);
    Cache &c = h->c;
    hipStream_t s = as_stream(stream);
    if (!sl->waited) {
        HA_CHECK_HIP(hipStreamWaitEvent(s, sl->booked, 0));
        sl->waited = true;
    }
    const long long at = static_cast<long long>(i) * c.nmax;
    cache_mark(h, kTStart, s, true);
    if (n_push > 0 && chain_push_rows(h, s, sl, i, grads))
        return -1;
    cache_mark(h, kTCopy, s);
    if (n_pull > 0 && lookup_rows(h, s, sl->pos_item + at, n_pull, dest, sl->pver + at, sl->rec + i, sl->it_upd_pos + at))
        return -1;
    cache_mark(h, kTEnd, s);
    h->settle_slot = sl;
    h->settle_idx = i;
    return plan_called(h, sl, i, 2, s);
}

// `count` middle steps by ONE call (a caller that has the gradient buffers at hand: a benchmark loop)
extern "C" int ha_cache_run_planned_push_pulls(ha_cache *h, int count, const int64_t *n_pull, float *const *dests,
                                               const int64_t *n_push, const float *const *grads, ha_stream_t stream) {
    HA_REQUIRE(h && count >= 0 && (count == 0 || (n_pull && dests && n_push && grads)), "cache_run_planned_push_pulls: bad arguments");
    for (int k = 0; k < count; ++k)
        if (ha_cache_push_pull_planned(h, n_pull[k], dests[k], n_push[k], grads[k], stream))
            return -1;
    return 0;
}

// The entry of a push-pull chain that is due, POOLED on both sides: the head (a pooled plain lookup), a middle step (the push
// half from the pooled gradient of the batch pulled by the step before -- cache_update_planned_kernel<.., BAGS> --, then the
// pooled pull half, cache_lookup_sum_planned_kernel<.., PP>), or the closing entry (the push half alone).  It takes the place of
// ha_cache_lookup_planned / ha_cache_push_pull_planned / ha_cache_update_planned in the chain's call sequence and leaves the
// host state those leave; everything is checked before anything is enqueued.
extern "C" int ha_cache_push_pull_planned_bags(ha_cache *h, int64_t n_pull, int64_t nbags_pull, int64_t bag_pull,
                                               const int64_t *offsets_pull, float *out, int64_t n_push, int64_t nbags_push,
                                               int64_t bag_push, const int32_t *bag_of_push, const float *bag_grads,
                                               ha_stream_t stream) {
    HA_REQUIRE(h, "cache_push_pull_planned_bags: null handle");
    PlanSlot *sl = nullptr;
    int i = 0;
    for (int k = 0; k < ha_cache::kPlanSlots && sl == nullptr; ++k) {         // the older block first (as plan_current)
        PlanSlot &q = h->plan[(h->plan_next + k) % ha_cache::kPlanSlots];
        if (q.count > 0 && q.next_call < q.total())
            sl = &q;
    }
    HA_REQUIRE(sl != nullptr, "cache_push_pull_planned_bags: no entry of a push-pull chain is due (ha_cache_plan_block_push_pull)");
    HA_REQUIRE(sl->pp, "cache_push_pull_planned_bags: the planned block is a block of lookup + update pairs (ha_cache_plan_block): "
               "its pooled calls are ha_cache_lookup_sum_planned / ha_cache_update_planned_bags");
    i = sl->next_call;
    const int kind = sl->kind[i];
    const bool has_pull = kind != kChainClose, has_push = kind != kChainHead;
    if (has_pull) {
        HA_REQUIRE(n_pull >= 0 && nbags_pull >= 0 && nbags_pull < (1ll << 31) && bag_pull >= 0,
                   "cache_push_pull_planned_bags: the entry due pulls a batch; bad pull sizes n=%ld nbags=%ld bag=%ld", (long)n_pull,
                   (long)nbags_pull, (long)bag_pull);
        HA_REQUIRE((bag_pull >= 1) != (offsets_pull != nullptr), "cache_push_pull_planned_bags: pull side: give exactly one of "
                   "bag >= 1 and offsets (bag=%ld, offsets %s)", (long)bag_pull, offsets_pull ? "given" : "null");
        HA_REQUIRE(offsets_pull != nullptr || (n_pull % bag_pull == 0 && n_pull / bag_pull == nbags_pull),
                   "cache_push_pull_planned_bags: pull side: n=%ld is not nbags=%ld bags of bag=%ld ids", (long)n_pull,
                   (long)nbags_pull, (long)bag_pull);
        HA_REQUIRE(n_pull == 0 || nbags_pull >= 1, "cache_push_pull_planned_bags: pull side: %ld ids in no bag", (long)n_pull);
        HA_REQUIRE(nbags_pull == 0 || out, "cache_push_pull_planned_bags: null output");
        HA_REQUIRE(sl->n[i] == n_pull, "cache_push_pull_planned_bags: the planned entry pulls %ld keys (got %ld)", (long)sl->n[i],
                   (long)n_pull);
    } else {
        HA_REQUIRE(n_pull == -1 && nbags_pull == 0 && bag_pull == 0 && !offsets_pull && !out,
                   "cache_push_pull_planned_bags: the entry due closes the chain: it pulls nothing (n_pull == -1, pull arguments 0 / "
                   "null)");
    }
    if (has_push) {
        HA_REQUIRE(n_push >= 0 && nbags_push >= 0 && nbags_push < (1ll << 31) && bag_push >= 0 && bag_push < (1ll << 31),
                   "cache_push_pull_planned_bags: bad push sizes n=%ld nbags=%ld bag=%ld", (long)n_push, (long)nbags_push,
                   (long)bag_push);
        // (an empty batch of ragged bags has no bag_of to give: neither is accepted then)
        HA_REQUIRE(n_push == 0 ? !(bag_push >= 1 && bag_of_push != nullptr) : (bag_push >= 1) != (bag_of_push != nullptr),
                   "cache_push_pull_planned_bags: push side: give exactly one of bag >= 1 and bag_of (bag=%ld, bag_of %s)",
                   (long)bag_push, bag_of_push ? "given" : "null");
        HA_REQUIRE(bag_push < 1 || (n_push % bag_push == 0 && n_push / bag_push == nbags_push),
                   "cache_push_pull_planned_bags: push side: n=%ld is not nbags=%ld bags of bag=%ld ids", (long)n_push,
                   (long)nbags_push, (long)bag_push);
        HA_REQUIRE(n_push == 0 || (nbags_push >= 1 && bag_grads), "cache_push_pull_planned_bags: push side: %ld ids, but no bags or "
                   "no gradient", (long)n_push);
        HA_REQUIRE(sl->q_n[i] == n_push, "cache_push_pull_planned_bags: the planned entry pushes %ld keys (got %ld)", (long)sl->q_n[i],
                   (long)n_push);
    } else {
        HA_REQUIRE(n_push == 0 && nbags_push == 0 && bag_push == 0 && !bag_of_push && !bag_grads,
                   "cache_push_pull_planned_bags: the entry due is the chain's head: it pushes nothing (push arguments 0 / null)");
    }
    Cache &c = h->c;
    if (has_pull && nbags_pull > 0) {
        int vec = 1;
        uint32_t nslice = 1;
        HA_REQUIRE(sum_blocks(c, nbags_pull, out, &vec, &nslice) < (1ull << 31), "cache_push_pull_planned_bags: batch too large");
    }
    hipStream_t s = as_stream(stream);
    if (!sl->waited) {
        HA_CHECK_HIP(hipStreamWaitEvent(s, sl->booked, 0));
        sl->waited = true;
    }
    cache_mark(h, kTStart, s, true);
    if (has_push && n_push > 0 && chain_push_rows(h, s, sl, i, bag_grads, bag_of_push ? 0 : bag_push, bag_of_push))
        return -1;
    if (kind == kChainStep)
        cache_mark(h, kTCopy, s);
    if (has_pull && nbags_pull > 0 &&
        lookup_sum_rows(h, s, sl, i, n_pull, nbags_pull, bag_pull, offsets_pull, out, kind == kChainStep, "cache_push_pull_planned_bags"))
        return -1;
    cache_mark(h, kTEnd, s);
    h->settle_slot = has_pull ? sl : nullptr;
    h->settle_idx = i;
    if (!has_pull)
        h->evict_empty = true;
    return plan_called(h, sl, i, kind == kChainHead ? 0 : kind == kChainClose ? 1 : 2, s);
}

// `count` middle steps by ONE call, pooled both ways with fixed bags of `bag` ids: every step pulls and pushes n ids
extern "C" int ha_cache_run_planned_push_pulls_bags(ha_cache *h, int count, int64_t n, int64_t nbags, int64_t bag,
                                                    float *const *outs, const float *const *bag_grads, ha_stream_t stream) {
    HA_REQUIRE(h && count >= 0 && (count == 0 || (outs && bag_grads)), "cache_run_planned_push_pulls_bags: bad arguments");
    for (int k = 0; k < count; ++k)
        if (ha_cache_push_pull_planned_bags(h, n, nbags, bag, nullptr, outs[k], n, nbags, bag, nullptr, bag_grads[k], stream))
            return -1;
    return 0;
}

int ha::cache_chain_settle(ha_cache *h, hipStream_t s) {
    PlanSlot *sl = h->settle_slot;
    if (sl == nullptr)
        return 0;
    const int i = h->settle_idx;
    const long long at = static_cast<long long>(i) * h->c.nmax;
    const long long n = sl->n[i] > 0 ? sl->n[i] : 0, nq = sl->kind[i] == kChainStep ? sl->q_n[i] : 0;
    const long long m = n > nq ? n : nq;
    if (m > 0) {
        hipLaunchKernelGGL(cache_chain_settle_kernel, dim3(static_cast<unsigned>((m + 15) / 16)), dim3(1024), 0, s, h->c,
                           sl->pos_item + at, n, sl->pver + at, sl->q_pos_item + at, nq);
        HA_LAUNCH_CHECK();
    }
    h->settle_slot = nullptr;
    return 0;
}

// `count` planned pairs by ONE call: lookup of the next planned batch into dests[k], its update with grads[k], ... (a caller
// that has the gradient buffers of the pairs at hand: a benchmark loop, a pipeline whose model runs elsewhere)
extern "C" int ha_cache_run_planned_pairs(ha_cache *h, int count, const int64_t *n, float *const *dests,
                                          const float *const *grads, ha_stream_t stream) {
    HA_REQUIRE(h && count >= 0 && (count == 0 || (n && dests && grads)), "cache_run_planned_pairs: bad arguments");
    for (int k = 0; k < count; ++k) {
        if (ha_cache_lookup_planned(h, n[k], dests[k], stream))
            return -1;
        if (ha_cache_update_planned(h, n[k], grads[k], stream))
            return -1;
    }
    return 0;
}

// ... with fixed bags of `bag` ids, pooled both ways: ha_cache_lookup_sum_planned into outs[k] ([nbags, width]), then
// ha_cache_update_planned_bags with bag_grads[k] ([nbags, width]); every pair has n ids
extern "C" int ha_cache_run_planned_pairs_bags(ha_cache *h, int count, int64_t n, int64_t nbags, int64_t bag, float *const *outs,
                                               const float *const *bag_grads, ha_stream_t stream) {
    HA_REQUIRE(h && count >= 0 && (count == 0 || (outs && bag_grads)), "cache_run_planned_pairs_bags: bad arguments");
    for (int k = 0; k < count; ++k) {
        if (ha_cache_lookup_sum_planned(h, n, nbags, bag, nullptr, outs[k], stream))
            return -1;
        if (ha_cache_update_planned_bags(h, n, bag_grads[k], nbags, bag, nullptr, stream))
            return -1;
    }
    return 0;
}

// ... with fixed bags of `bag` ids and the weights weights[k] ([n]) of pair k: ha_cache_lookup_wsum_planned into outs[k], then
// ha_cache_update_planned_wbags with bag_grads[k] and `scale`
extern "C" int ha_cache_run_planned_pairs_wbags(ha_cache *h, int count, int64_t n, int64_t nbags, int64_t bag, float *const *outs,
                                                const float *const *bag_grads, const float *const *weights, float scale,
                                                ha_stream_t stream) {
    HA_REQUIRE(h && count >= 0 && (count == 0 || (outs && bag_grads && weights)), "cache_run_planned_pairs_wbags: bad arguments");
    for (int k = 0; k < count; ++k) {
        if (ha_cache_lookup_wsum_planned(h, n, nbags, bag, nullptr, weights[k], outs[k], stream))
            return -1;
        if (ha_cache_update_planned_wbags(h, n, bag_grads[k], weights[k], scale, nbags, bag, nullptr, stream))
            return -1;
    }
    return 0;
}

// out[8]: the report of the last planned call, as ha_cache_perf's (synchronises the stream)
int ha::cache_perf_planned(ha_cache *h, int64_t *out_host, hipStream_t s) {
    PlanSlot *sl = h->last_planned;
    const int i = h->last_planned_idx;
    const long long at = static_cast<long long>(i) * h->c.nmax;
    // (the closing step of a push-pull chain: the pushed lines are flagged in the push side's items)
    const int4 *items = (sl->pp && h->last_planned_type == 1 ? sl->q_pos_item : sl->pos_item) + at;
    hipLaunchKernelGGL(cache_plan_count_kernel, dim3(1), dim3(1024), 0, s, sl->rec + i, sl->pver + at, items);
    PlanRec r;
    long long sticky = 0;
    HA_CHECK_HIP(hipMemcpyAsync(&r, sl->rec + i, sizeof(r), hipMemcpyDeviceToHost, s));
    HA_CHECK_HIP(hipMemcpyAsync(&sticky, &h->c.ctl->fb_timeout, sizeof(sticky), hipMemcpyDeviceToHost, s));
    HA_CHECK_HIP(hipStreamSynchronize(s));
    HA_REQUIRE(sticky == 0, "cache: a bookkeeping launch gave up (code %ld, see ha_cache_state; the cache's state is not to be "
               "trusted)", (long)sticky);
    const int type = h->last_planned_type;
    out_host[0] = type;
    out_host[1] = r.n;
    out_host[2] = r.U;
    out_host[3] = type == 0 ? r.M : r.umiss;
    out_host[4] = type == 0 ? r.pulled : r.npush + r.erep;
    out_host[5] = type == 0 ? 0 : r.erep;
    out_host[6] = r.full;
    out_host[7] = r.size;
    return 0;
}

// k_order.hpp — order by a column: per query the first topk documents of its docID set by (column value, docID) (tri_batch_set_order / tri_batch_ordered)
// Part of libtrinity_hip.so (MI355X / gfx950); included by trinity_hip.hip.  New code, no reference source: the reference's consumer of a docID set is
// MatchedIndexDocumentsFilter::consider on the host (exec.h:12-23); this is that consumer for "list the first K by an attribute", run where the sets lie.
//
// One 64-bit key per match: (descending ? ~value : value) << 32 | docID.  Smaller is better; the keys of one source are distinct, so the order is strict and
// the selection is "the K smallest u64" — integers only, the same bits whatever the order of the workgroups, the waves and the lanes.
//
// k_order        a workgroup per task, as k_facet / k_deliver_docsets walk them: the task's segment of ascending docIDs (counts[task] of them), or — a
//                RESULT_BITMAP query — the words of the task's docID windows.  Every WAVE selects on its own: a buffer of ORDER_BUF keys in LDS that only the wave
//                touches, and a threshold in a register: the K-th best key as of the buffer's last prune.  A step offers ORDER_TILE documents, one per lane: a
//                coalesced read of the docID, one guarded gather from the column, one compare against the threshold, one ballot.  A step in which no lane beats the
//                threshold — nearly every step once K keys are held — ends there: no LDS access, no barrier of any kind.  Newcomers are appended, and only a buffer
//                past ORDER_PRUNE_AT keys is pruned to its best K, sorted, by rank counting (every lane counts, for the up to ORDER_BUF / 64 keys it holds in
//                registers, the keys below them: broadcast reads), which moves the threshold — a stale threshold lets more through, never less, and a prune is paid
//                once per ORDER_PRUNE_AT - K newcomers, not once per step that has one.  Wave-synchronous: the wave's own LDS accesses complete in order.  The workgroup meets ONCE, at the task's end: the waves'
//                sorted lists are merged by rank counting (a lower-bound search per other wave) into the task's partial list, ascending.
// k_order_merge  "L sorted lists of at most K keys -> the first K", by rank counting as k_rank_merge_sources does it: a lower-bound search per other list in a
//                fixed number of steps, no LDS, no atomics.  A workgroup per group of at most ORDER_FANIN lists; a query of more tasks takes further rounds
//                (the host lays the rounds out once per batch: they depend on the plan alone), so the work stays linear in the tasks times ORDER_FANIN.  The
//                last round of a query writes its row — every word of it, zeros past the count.  The same kernel (PARTS) merges a collection's parts' rows; there
//                equal keys of different sources both stay, the older source first.
// LDS: ORDER_WAVES * ORDER_BUF * 8 = 16 KB a workgroup, static — nine workgroups a CU fit, the registers allow eight: the register count decides the
// occupancy (profiles/order_kernel_resources.txt).  No scratch.
#pragma once
#include "docset_walk.hpp" // (docset_task, docset_for_each: the task preamble and the walk of its documents)

static_assert(ORDER_WG == ORDER_WAVES * 64 && ORDER_TILE == 64, "a wave offers one document per lane");
static_assert(ORDER_PRUNE_AT + ORDER_TILE == ORDER_BUF && ORDER_PRUNE_AT >= ORDER_MAX_TOPK && ORDER_BUF % 64 == 0,
              "a buffer at the prune mark has room for one step's newcomers, a pruned one is below the mark; a lane holds ORDER_BUF / 64 keys");
static_assert(ORDER_WG >= ORDER_MAX_TOPK, "the final merge gives every thread one entry per wave");

struct OrderShared {
        uint64_t buf[ORDER_WAVES][ORDER_BUF];
        uint32_t n[ORDER_WAVES];
};

// the wave's own LDS accesses complete in the order they were issued: all that is needed between one lane's write and another lane's read is that the compiler
// keeps that order
__device__ __forceinline__ void order_wave_sync() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the key of document d.  A docID at or past the column's end is never read: it takes the value 0xffffffff (tri_column_create makes that unreachable: the column
// covers every docID of its index)
__device__ __forceinline__ uint64_t order_key(const DevOrder &o, const uint32_t d, const bool live) {
        const uint32_t v = live && d < o.ndocs ? o.values[d] : 0xffffffffu;
        return (uint64_t)(v ^ o.flip) << 32 | d;
}

// The wave's buffer of n <= ORDER_BUF keys, in any order -> its min(n, k) smallest, sorted ascending at buf[0 ..).  Every lane takes the keys lane, lane + 64, ...
// into registers and counts for each the keys below it (the keys are distinct: the counts are the ranks); rank < k: the key goes to buf[rank].
__device__ __forceinline__ uint32_t order_prune(uint64_t *buf, const uint32_t n, const uint32_t k, const uint32_t lane) {
        constexpr uint32_t PER_LANE = ORDER_BUF / 64;
        uint64_t key[PER_LANE];
        uint32_t rank[PER_LANE];
#pragma unroll
        for (uint32_t u = 0; u < PER_LANE; ++u) {
                const uint32_t i = lane + 64u * u;
                key[u] = i < n ? buf[i] : ~0ull;
                rank[u] = 0;
        }
        for (uint32_t j = 0; j < n; ++j) {
                const uint64_t x = buf[j]; // (one address for the wave: a broadcast)
#pragma unroll
                for (uint32_t u = 0; u < PER_LANE; ++u)
                        rank[u] += x < key[u] ? 1u : 0u;
        }
        order_wave_sync(); // (every lane has read what it ranks before any lane overwrites it)
#pragma unroll
        for (uint32_t u = 0; u < PER_LANE; ++u)
                if (lane + 64u * u < n && rank[u] < k)
                        buf[rank[u]] = key[u];
        order_wave_sync();
        return n < k ? n : k;
}

// One step: every live lane offers its key.  n <= ORDER_PRUNE_AT on entry and on return; thr is the k-th smallest key as of the last prune, all ones before the
// first (a live key is below that: its docID is below the column's 32-bit entry count)
__device__ __forceinline__ void order_offer(uint64_t *buf, uint32_t &n, uint64_t &thr, const uint32_t k, const uint32_t lane, const bool live, const uint64_t key) {
        const bool pass = live && key < thr;
        const uint64_t m = __builtin_amdgcn_ballot_w64(pass);
        if (!m)
                return; // (wave-uniform: the steady state of a long segment)
        if (pass)
                buf[n + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = key;
        n += (uint32_t)__popcll(m);
        if (n > ORDER_PRUNE_AT) { // (more than k: the pruned buffer holds k keys)
                order_wave_sync();
                n = order_prune(buf, n, k, lane);
                thr = buf[k - 1];
        }
}

__global__ __launch_bounds__(ORDER_WG) void k_order(const DevQuery *__restrict__ plan, const DevTask *__restrict__ tasks, const uint32_t *__restrict__ counts,
                                                    const uint32_t *__restrict__ out, const DevOrder o, uint64_t *__restrict__ list_keys, uint32_t *__restrict__ list_counts) {
        __shared__ OrderShared sh;
        const uint32_t tix = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
        DevTask tk;
        DevQuery q;
        uint32_t c;
        const DocsetCase what = docset_task(plan, tasks, counts, tix, tk, q, c);
        if (what == DOCSET_HIDDEN)
                return; // (no caller query, no list any group names; uniform)
        if (what == DOCSET_EMPTY) { // (a one-pass scored task keeps no docID set; no matches: an empty list; uniform)
                if (tid == 0)
                        list_counts[tix] = 0;
                return;
        }
        const uint32_t k = o.topk;
        uint64_t *buf = sh.buf[wave];
        uint32_t n = 0;
        uint64_t thr = ~0ull;
        const uint32_t *p = out + tk.out_off;
        if (q.form != RESULT_BITMAP) {
                for (uint32_t i0 = wave * ORDER_TILE * ORDER_UNROLL; i0 < c; i0 += ORDER_WG * ORDER_UNROLL) { // (uniform per wave)
                        uint64_t key[ORDER_UNROLL];
                        bool live[ORDER_UNROLL];
#pragma unroll
                        for (uint32_t u = 0; u < ORDER_UNROLL; ++u) { // (the steps' gathers are all requested before the first is used)
                                const uint32_t i = i0 + ORDER_TILE * u + lane;
                                live[u] = i < c;
                                key[u] = order_key(o, live[u] ? p[i] : 0u, live[u]);
                        }
#pragma unroll
                        for (uint32_t u = 0; u < ORDER_UNROLL; ++u)
                                order_offer(buf, n, thr, k, lane, live[u], key[u]);
                }
        } else {
                const uint32_t nw = (tk.tile_end - tk.tile_begin) * SPAN_WORDS;
                for (uint32_t i0 = wave * 64u; i0 < nw; i0 += ORDER_WG) { // (uniform per wave) a word per lane, its documents ORDER_UNROLL at a time
                        const uint32_t i = i0 + lane;
                        uint32_t m = i < nw ? p[i] : 0u;
                        const uint32_t base = (tk.tile_begin * SPAN_WORDS + i) * 32u;
                        while (__builtin_amdgcn_ballot_w64(m != 0u)) {
                                uint64_t key[ORDER_UNROLL];
                                bool live[ORDER_UNROLL];
#pragma unroll
                                for (uint32_t u = 0; u < ORDER_UNROLL; ++u) {
                                        live[u] = m != 0u;
                                        key[u] = order_key(o, base + (live[u] ? (uint32_t)__builtin_ctz(m) : 0u), live[u]);
                                        m &= m - 1u;
                                }
#pragma unroll
                                for (uint32_t u = 0; u < ORDER_UNROLL; ++u)
                                        order_offer(buf, n, thr, k, lane, live[u], key[u]);
                        }
                }
        }
        // ---- the task's end: every wave's best k sorted, then the one meeting of the workgroup
        order_wave_sync();
        n = order_prune(buf, n, k, lane);
        if (lane == 0)
                sh.n[wave] = n;
        __syncthreads();
        uint32_t cnt[ORDER_WAVES], total = 0;
#pragma unroll
        for (uint32_t w = 0; w < ORDER_WAVES; ++w) {
                cnt[w] = sh.n[w];
                total += cnt[w];
        }
        uint64_t *list = list_keys + (uint64_t)tix * k;
        if (tid == 0)
                list_counts[tix] = total < k ? total : k;
        const uint32_t top_step = 1u << (31 - __builtin_clz(k)); // (2 * top_step - 1 >= k: the steps reach every count up to k)
#pragma unroll
        for (uint32_t w = 0; w < ORDER_WAVES; ++w) { // entry tid of wave w's list: its rank among all
                if (tid >= cnt[w])
                        continue;
                const uint64_t key = sh.buf[w][tid];
                uint32_t rank = tid;
#pragma unroll
                for (uint32_t j = 0; j < ORDER_WAVES; ++j) {
                        if (j == w)
                                continue;
                        uint32_t lo = 0; // keys of wave j known to be below
                        for (uint32_t step = top_step; step; step >>= 1) {
                                const uint32_t at = lo + step;
                                if (at <= cnt[j] && sh.buf[j][at - 1] < key)
                                        lo = at;
                        }
                        rank += lo;
                }
                if (rank < k)
                        list[rank] = key;
        }
}

// Lists [first, first + n) of the source folded into the destination's list g.dst: PARTS false — a batch: the lists lie in ONE block (`one`, by value: a run already queued keeps it), the destination is a
// list of `mid` or, g.reserved != 0, the query's row of `rows`; PARTS true — a collection: group = query blockIdx.x, list j = that query's row of part j (src[j]).
// An entry's rank is its index plus, per other list, the keys that precede it there: those below it, and — equal keys exist only between a collection's parts —
// the equal one of an older part.
template <bool PARTS>
__global__ __launch_bounds__(ORDER_WG) void k_order_merge(const DevOrderLists *__restrict__ src, const DevOrderLists one, const DevOrderGroup *__restrict__ groups, const uint32_t nparts, const uint32_t k,
                                                          uint64_t *__restrict__ mid_keys, uint32_t *__restrict__ mid_counts, uint64_t *__restrict__ row_keys,
                                                          uint32_t *__restrict__ row_counts) {
        const uint32_t tid = threadIdx.x;
        const DevOrderGroup g = PARTS ? DevOrderGroup{0u, nparts, blockIdx.x, 1u} : groups[blockIdx.x];
        const auto keys_of = [&](const uint32_t j) { return PARTS ? src[j].keys + (uint64_t)g.dst * k : one.keys + (uint64_t)(g.first + j) * k; };
        const auto count_of = [&](const uint32_t j) { return min(PARTS ? src[j].counts[g.dst] : one.counts[g.first + j], k); };
        uint32_t total = 0;
        for (uint32_t j = 0; j < g.n; ++j)
                total += count_of(j);
        const uint32_t n = total < k ? total : k;
        uint64_t *dst = (g.reserved ? row_keys : mid_keys) + (uint64_t)g.dst * k;
        for (uint32_t i = n + tid; i < k; i += ORDER_WG)
                dst[i] = 0; // (the ranks below are a permutation of 0 .. total - 1: with these every word of the list is written, once)
        if (tid == 0)
                (g.reserved ? row_counts : mid_counts)[g.dst] = n;
        const uint32_t top_step = 1u << (31 - __builtin_clz(k));
        for (uint32_t e = tid; e < g.n * k; e += ORDER_WG) {
                const uint32_t s = e / k, i = e - s * k;
                if (i >= count_of(s))
                        continue;
                const uint64_t key = keys_of(s)[i];
                uint32_t rank = i;
                for (uint32_t j = 0; j < g.n; ++j) {
                        if (j == s)
                                continue;
                        const uint32_t c = count_of(j);
                        const uint64_t *jk = keys_of(j);
                        uint32_t lo = 0;
                        for (uint32_t step = top_step; step; step >>= 1) {
                                const uint32_t at = lo + step;
                                if (at <= c) {
                                        const uint64_t x = jk[at - 1];
                                        if (x < key || (x == key && j < s))
                                                lo = at;
                                }
                        }
                        rank += lo;
                }
                if (rank < k)
                        dst[rank] = key;
        }
}

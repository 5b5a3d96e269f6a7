// k_stats.hpp — stats of a column per query and bucket: count, sum, min and max of a value column over a query's docID set, optionally grouped by a second column
// (tri_batch_set_stats / tri_batch_stats).  Part of libtrinity_hip.so (MI355X / gfx950); included by trinity_hip.hip.  New code, no reference source: the reference's
// consumer of a docID set is MatchedIndexDocumentsFilter::consider on the host (exec.h:12-23); this is that consumer for "the price range, the average rating, the
// revenue per brand of the matches", run where the sets lie.
//
// A workgroup per task, as k_facet walks them: the task's segment of ascending docIDs (counts[task] of them), or — a RESULT_BITMAP query — the words of the task's
// docID windows.  For every document d and stat k the record of bucket min(group_k[d], nb_k) takes value_k[d].  Three regimes, uniform per workgroup and stat:
//   registers  an ungrouped stat: every lane folds its documents into a record of its own, a wave folds its lanes with shuffles, the four waves meet in one LDS
//              record, and one lane issues the task's four global atomics — never an atomic per match on one address
//   on chip    the records of the query's grouped stats together fit STATS_LDS_BUCKETS and the segment has at least STATS_SHORT_SEGMENT matches: the workgroup keeps
//              four LDS planes (64-bit add for the sum; add, min, max for the rest) and flushes every record whose count is not zero once
//   direct     wider rows, shorter segments: four global atomics per match and stat
// Integer add, min and max commute: a record is the same bits whatever the order of the workgroups, the lanes and the regimes.
// The LDS planes are static — (STATS_LDS_BUCKETS + STATS_MAX) records of 20 bytes, 16 080 bytes —: every workgroup reserves them, also one that returns at once; see
// k_facet.hpp on why they stay under 16 KB (profiles/stats_kernel_resources.txt).
#pragma once
#include "docset_walk.hpp" // (docset_task, docset_for_each: the task preamble and the walk of its documents)

struct StatsLds { // record i < STATS_LDS_BUCKETS: a bucket of a grouped stat (DevStats::lds_off); record STATS_LDS_BUCKETS + k: ungrouped stat k, where the waves meet
        unsigned long long sums[STATS_LDS_BUCKETS + STATS_MAX];
        uint32_t counts[STATS_LDS_BUCKETS + STATS_MAX], mins[STATS_LDS_BUCKETS + STATS_MAX], maxs[STATS_LDS_BUCKETS + STATS_MAX];
};
static_assert(sizeof(StatsLds) <= 16384, "k_stats' static LDS stays at or under 16 KB");

struct StatsAcc { // a lane's record of the ungrouped stats
        unsigned long long sum[STATS_MAX];
        uint32_t cnt[STATS_MAX], mn[STATS_MAX], mx[STATS_MAX];
};

// a record into stat k's global planes: u64 add, u32 add, min, max
__device__ __forceinline__ void stats_global(const DevStats &s, const uint32_t k, uint32_t *__restrict__ blk, const uint32_t qid, const uint32_t bkt, const unsigned long long sum,
                                             const uint32_t cnt, const uint32_t mn, const uint32_t mx) {
        const uint64_t R = (uint64_t)s.nq * (s.nb[k] + 1u), rec = (uint64_t)qid * (s.nb[k] + 1u) + bkt;
        uint32_t *const base = blk + s.off[k];
        atomicAdd(reinterpret_cast<unsigned long long *>(base) + rec, sum);
        atomicAdd(base + 2 * R + rec, cnt);
        atomicMin(base + 3 * R + rec, mn);
        atomicMax(base + 4 * R + rec, mx);
}

template <bool LDS>
__device__ __forceinline__ void stats_take(const DevStats &s, const uint32_t qid, uint32_t *__restrict__ blk, StatsLds &l, StatsAcc &a, const uint32_t d) {
        // (the per-stat loops are unrolled: the specs stay in the kernel's argument registers, no indexed copy of them; a document's group and value gathers are
        //  requested together, ahead of the first use)
        const bool covered = d < s.ndocs; // (a docID the columns do not cover is never read: its group is overflow, its value 0xffffffff)
        uint32_t g[STATS_MAX], v[STATS_MAX];
#pragma unroll
        for (uint32_t k = 0; k < STATS_MAX; ++k) {
                if (k >= s.n)
                        break;
                v[k] = covered ? s.value[k][d] : 0xffffffffu;
                g[k] = covered && s.group[k] ? s.group[k][d] : 0xffffffffu;
        }
#pragma unroll
        for (uint32_t k = 0; k < STATS_MAX; ++k) {
                if (k >= s.n)
                        break;
                if (!s.group[k]) { // (uniform)
                        a.sum[k] += v[k];
                        a.cnt[k] += 1u;
                        a.mn[k] = min(a.mn[k], v[k]);
                        a.mx[k] = max(a.mx[k], v[k]);
                        continue;
                }
                const uint32_t bkt = g[k] < s.nb[k] ? g[k] : s.nb[k];
                if (LDS) {
                        const uint32_t i = s.lds_off[k] + bkt;
                        atomicAdd(&l.sums[i], (unsigned long long)v[k]);
                        atomicAdd(&l.counts[i], 1u);
                        atomicMin(&l.mins[i], v[k]);
                        atomicMax(&l.maxs[i], v[k]);
                } else
                        stats_global(s, k, blk, qid, bkt, v[k], 1u, v[k], v[k]);
        }
}

// the documents of the task (docset_walk.hpp), each handed to stats_take once
template <bool LDS>
__device__ __forceinline__ void stats_walk(const DevStats &s, const DevQuery &q, const DevTask &tk, const uint32_t c, const uint32_t *__restrict__ out, uint32_t *__restrict__ blk,
                                           StatsLds &l, StatsAcc &a) {
        docset_for_each<STATS_WG>(q, tk, c, out, [&](const uint32_t d) { stats_take<LDS>(s, q.qid, blk, l, a, d); });
}

__global__ __launch_bounds__(STATS_WG) void k_stats(const DevQuery *__restrict__ plan, const DevTask *__restrict__ tasks, const uint32_t *__restrict__ counts,
                                                    const uint32_t *__restrict__ out, const DevStats s, uint32_t *__restrict__ blk) {
        __shared__ StatsLds l;
        const uint32_t tix = blockIdx.x, tid = threadIdx.x;
        // (docset_task's cases in the kernel's own text: with the shared preamble the compiler spills two more SGPRs here — DESIGN.md §34)
        const DevTask tk = tasks[tix];
        if (task_onepass(tk.kind) && tk.kind != TASK_FUSED_GEN)
                return; // (a one-pass scored task keeps no docID set; uniform)
        const DevQuery q = plan[tk.slot];
        if (q.qid == 0xffffffffu)
                return; // (a hidden phrase query — a leaf of a TASK_TREE query: no caller query, no row; uniform)
        const uint32_t c = counts[tix];
        if (!c)
                return; // (uniform)
        const uint32_t records = s.lds_records;
        const bool on_chip = records && records <= STATS_LDS_BUCKETS && c >= STATS_SHORT_SEGMENT; // (uniform)
        for (uint32_t i = tid; i < (on_chip ? records : 0u); i += STATS_WG) {
                l.sums[i] = 0;
                l.counts[i] = 0;
                l.mins[i] = 0xffffffffu;
                l.maxs[i] = 0;
        }
        if (tid < STATS_MAX) {
                l.sums[STATS_LDS_BUCKETS + tid] = 0;
                l.counts[STATS_LDS_BUCKETS + tid] = 0;
                l.mins[STATS_LDS_BUCKETS + tid] = 0xffffffffu;
                l.maxs[STATS_LDS_BUCKETS + tid] = 0;
        }
        __syncthreads();
        StatsAcc a;
#pragma unroll
        for (uint32_t k = 0; k < STATS_MAX; ++k) {
                a.sum[k] = 0;
                a.cnt[k] = 0;
                a.mn[k] = 0xffffffffu;
                a.mx[k] = 0;
        }
        if (on_chip)
                stats_walk<true>(s, q, tk, c, out, blk, l, a);
        else
                stats_walk<false>(s, q, tk, c, out, blk, l, a);
        // the ungrouped stats: the lanes of a wave fold by shuffles, the waves meet in LDS record STATS_LDS_BUCKETS + k
#pragma unroll
        for (uint32_t k = 0; k < STATS_MAX; ++k) {
                if (k >= s.n)
                        break;
                if (s.group[k])
                        continue; // (uniform)
                unsigned long long sum = a.sum[k];
                uint32_t cnt = a.cnt[k], mn = a.mn[k], mx = a.mx[k];
#pragma unroll
                for (uint32_t w = 32; w; w >>= 1) {
                        sum += __shfl_xor(sum, w, 64);
                        cnt += __shfl_xor(cnt, w, 64);
                        mn = min(mn, __shfl_xor(mn, w, 64));
                        mx = max(mx, __shfl_xor(mx, w, 64));
                }
                if (!(tid & 63u) && cnt) {
                        atomicAdd(&l.sums[STATS_LDS_BUCKETS + k], sum);
                        atomicAdd(&l.counts[STATS_LDS_BUCKETS + k], cnt);
                        atomicMin(&l.mins[STATS_LDS_BUCKETS + k], mn);
                        atomicMax(&l.maxs[STATS_LDS_BUCKETS + k], mx);
                }
        }
        __syncthreads();
        if (tid < STATS_MAX && tid < s.n && l.counts[STATS_LDS_BUCKETS + tid]) { // one lane per ungrouped stat: the task's four global atomics
#pragma unroll
                for (uint32_t k = 0; k < STATS_MAX; ++k)
                        if (k == tid && !s.group[k])
                                stats_global(s, k, blk, q.qid, 0u, l.sums[STATS_LDS_BUCKETS + k], l.counts[STATS_LDS_BUCKETS + k], l.mins[STATS_LDS_BUCKETS + k],
                                             l.maxs[STATS_LDS_BUCKETS + k]);
        }
        if (!on_chip)
                return;
        for (uint32_t i = tid; i < records; i += STATS_WG) {
                const uint32_t cnt = l.counts[i];
                if (!cnt)
                        continue;
#pragma unroll
                for (uint32_t k = 0; k < STATS_MAX; ++k) // the stat record i belongs to
                        if (k < s.n && s.group[k] && i >= s.lds_off[k] && i < s.lds_off[k + 1])
                                stats_global(s, k, blk, q.qid, i - s.lds_off[k], l.sums[i], cnt, l.mins[i], l.maxs[i]);
        }
}

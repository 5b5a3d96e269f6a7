// k_facet.hpp — facet counts: per query a histogram of its docID set over per-document columns (tri_batch_set_facets / tri_batch_facets)
// Part of libtrinity_hip.so (MI355X / gfx950); included by trinity_hip.hip.  New code, no reference source: the reference's consumer of a docID set is
// MatchedIndexDocumentsFilter::consider on the host (exec.h:12-23); this is that consumer for "count the matches by an attribute", run where the sets lie.
//
// A workgroup per task, as k_deliver_docsets walks them: the task's segment of ascending docIDs (counts[task] of them), or — a RESULT_BITMAP query — the words
// of the task's docID windows.  For every document d and facet k: counter min(values_k[d], nb_k) of the query's row goes up by one.  Two regimes:
//   on chip   the counters of one query (all facets) fit FACET_LDS_COUNTERS and the segment has at least FACET_SHORT_SEGMENT matches: the workgroup counts into an
//             LDS row of its own and adds every non-zero counter to the global row once — a query's tasks meet in the global row only through those flushes
//   direct    wider rows, shorter segments: one global integer atomic per match and facet
// Integer adds commute: a row is the same bits whatever the order of the workgroups, the lanes and the regimes.
// The LDS row is static: EVERY workgroup reserves its FACET_LDS_COUNTERS * 4 bytes, also one that returns at once (a hidden query, a one-pass task, no matches) or goes
// direct.  At 16 KB that bounds nothing — ten workgroups a CU fit, the registers allow eight waves a SIMD —; past 20 KB a workgroup's LDS, not its registers, would set the
// occupancy of the direct path too: raise FACET_LDS_COUNTERS knowing that (profiles/facet_kernel_resources.txt).
#pragma once
#include "docset_walk.hpp" // (docset_task, docset_for_each: the task preamble and the walk of its documents)

// counter of facet k that document d falls into (a docID the column does not cover is never read: overflow)
__device__ __forceinline__ uint32_t facet_bucket(const DevFacets &f, const uint32_t k, const uint32_t d) {
        const uint32_t v = d < f.ndocs[k] ? f.values[k][d] : 0xffffffffu;
        return v < f.nb[k] ? v : f.nb[k];
}

template <bool LDS>
__device__ __forceinline__ void facet_count(const DevFacets &f, const uint32_t qid, uint32_t *__restrict__ rows, uint32_t *lds, const uint32_t d) {
#pragma unroll
        for (uint32_t k = 0; k < FACETS_MAX; ++k) { // (unrolled: the specs stay in the kernel's argument registers, no indexed copy of them)
                if (k >= f.n)
                        break;
                const uint32_t bkt = facet_bucket(f, k, d);
                if (LDS)
                        atomicAdd(&lds[f.lds_off[k] + bkt], 1u);
                else
                        atomicAdd(&rows[f.rows_off[k] + (uint64_t)qid * (f.nb[k] + 1u) + bkt], 1u);
        }
}

// the documents of the task (docset_walk.hpp), each handed to facet_count once
template <bool LDS>
__device__ __forceinline__ void facet_walk(const DevFacets &f, const DevQuery &q, const DevTask &tk, const uint32_t c, const uint32_t *__restrict__ out, uint32_t *__restrict__ rows,
                                           uint32_t *lds) {
        docset_for_each<FACET_WG>(q, tk, c, out, [&](const uint32_t d) { facet_count<LDS>(f, q.qid, rows, lds, d); });
}

__global__ __launch_bounds__(FACET_WG) void k_facet(const DevQuery *__restrict__ plan, const DevTask *__restrict__ tasks, const uint32_t *__restrict__ counts,
                                                    const uint32_t *__restrict__ out, const DevFacets f, uint32_t *__restrict__ rows) {
        __shared__ uint32_t lds[FACET_LDS_COUNTERS];
        const uint32_t tix = blockIdx.x, tid = threadIdx.x;
        DevTask tk;
        DevQuery q;
        uint32_t c;
        if (docset_task(plan, tasks, counts, tix, tk, q, c) != DOCSET_WALK)
                return; // (a hidden phrase query, a one-pass task, no matches: no row to count into; uniform)
        const uint32_t per_query = f.per_query;
        if (per_query > FACET_LDS_COUNTERS || c < FACET_SHORT_SEGMENT) { // (uniform)
                facet_walk<false>(f, q, tk, c, out, rows, nullptr);
                return;
        }
        for (uint32_t i = tid; i < per_query; i += FACET_WG)
                lds[i] = 0;
        __syncthreads();
        facet_walk<true>(f, q, tk, c, out, rows, lds);
        __syncthreads();
        for (uint32_t i = tid; i < per_query; i += FACET_WG) {
                const uint32_t v = lds[i];
                if (!v)
                        continue;
#pragma unroll
                for (uint32_t k = 0; k < FACETS_MAX; ++k) // the facet counter i belongs to
                        if (k < f.n && i >= f.lds_off[k] && i < f.lds_off[k + 1])
                                atomicAdd(&rows[f.rows_off[k] + (uint64_t)q.qid * (f.nb[k] + 1u) + (i - f.lds_off[k])], v);
        }
}

// docset_walk.hpp — how a kernel that consumes a batch's finished docID sets (k_facet, k_stats, k_order) opens a task and walks its documents.  Plain C++17 but for
// the one line that reads threadIdx: tests/cpp/docset_walk_cpu_test.cpp compiles the walk with g++.
//
// Contract.  A workgroup per task, behind every kernel that completes the sets (counts[] is final).
//   docset_task      loads the task, its query and its match count and says which case the workgroup is in.  All three cases are WORKGROUP-UNIFORM (they depend on
//                    blockIdx alone), so a kernel may return on them ahead of a barrier:
//                      DOCSET_HIDDEN  a hidden phrase query — a leaf of a TASK_TREE query: no caller query, no row.  Checked first: tk, q are loaded, c is not
//                      DOCSET_EMPTY   a one-pass scored task (it keeps no docID set), or no matches
//                      DOCSET_WALK    c > 0 documents to walk
//   docset_for_each  calls f(d) exactly once per document d of the task, over the WG threads of the workgroup together: thread tid takes the segment's out[out_off + i]
//                    for i = tid, tid + WG, .. < c, or — a RESULT_BITMAP query — the set bits of the window words i = tid, tid + WG, .. of the task's tiles, ascending
//                    inside a word: d = (tile_begin * SPAN_WORDS + i) * 32 + bit.  No order between threads, no barrier, nothing is written.
// k_order opens with docset_task but keeps a walk of its own (wave-tiled, ORDER_UNROLL gathers ahead); k_stats walks with docset_for_each but keeps a preamble of its
// own (with docset_task the compiler spills two more SGPRs there); k_deliver_docsets keeps its own text altogether.
#pragma once
#include "dev_search.hpp"

enum DocsetCase : uint32_t { DOCSET_HIDDEN, DOCSET_EMPTY, DOCSET_WALK };

// thread tid's share of the walk
template <uint32_t WG, typename F>
TRI_HDI void docset_for_each_of(const uint32_t tid, const DevQuery &q, const DevTask &tk, const uint32_t c, const uint32_t *__restrict__ out, F &&f) {
        const uint32_t *p = out + tk.out_off;
        if (q.form != RESULT_BITMAP) {
                for (uint32_t i = tid; i < c; i += WG)
                        f(p[i]);
                return;
        }
        const uint32_t nw = (tk.tile_end - tk.tile_begin) * SPAN_WORDS;
        for (uint32_t i = tid; i < nw; i += WG)
                for (uint32_t m = p[i]; m; m &= m - 1u)
                        f((tk.tile_begin * SPAN_WORDS + i) * 32u + (uint32_t)__builtin_ctz(m));
}

#if defined(__HIPCC__)
__device__ __forceinline__ DocsetCase docset_task(const DevQuery *__restrict__ plan, const DevTask *__restrict__ tasks, const uint32_t *__restrict__ counts, const uint32_t tix, DevTask &tk,
                                                  DevQuery &q, uint32_t &c) {
        tk = tasks[tix];
        q = plan[tk.slot];
        if (q.qid == 0xffffffffu)
                return DOCSET_HIDDEN;
        c = counts[tix];
        return (task_onepass(tk.kind) && tk.kind != TASK_FUSED_GEN) || !c ? DOCSET_EMPTY : DOCSET_WALK;
}

template <uint32_t WG, typename F>
__device__ __forceinline__ void docset_for_each(const DevQuery &q, const DevTask &tk, const uint32_t c, const uint32_t *__restrict__ out, F &&f) {
        docset_for_each_of<WG>(threadIdx.x, q, tk, c, out, f);
}
#endif

// k_filter.hpp — per-query document filters (IndexDocumentsFilter, matches.h:190-201: the application rules documents out BEFORE they are
// considered; exec.cpp:1133-1150 tests it next to the masked documents) on the device.
// Part of libtrinity_hip.so (MI355X / gfx950); included by trinity_hip.hip.  New code, no reference source.
//
// A filter (tri_filter) is a bitmap over docIDs in DROP polarity — bit d set: document d never matches —, of the extent of the index's masked
// bitmap: (max_doc / SPAN_BITS + 2) * SPAN_WORDS words (whole docID windows and a spare one; a multiple of 4096 words, so every row of the
// table below starts 16-byte aligned wherever a kernel reads it in 16- or 8-byte units).
//   k_filter_scatter      docID list (any order, duplicates) -> bits, one atomic OR each
//   k_filter_complement   TRI_FILTER_KEEP: the allow-list's bitmap turned into the drop bitmap, 16 bytes a lane
//   k_filter_from_docset  the same from a synced DocumentsOnly batch's result, in either form the engine holds it
//   k_filter_rows         per run: row r = filter r | the index's masked documents, for the filters the batch's queries name
// and FilterSel / filter_pick: how a matching kernel finds ITS task's bitmap — a row id per plan slot, 0 = the index's own mask.
// The persistent matching kernels (k_and_dense, k_and, k_psets, k_probe, k_fused, k_planes) are compiled TWICE: in trinity_hip.hip as they always were — the
// macros below expand to nothing there, so a batch without filters runs the very code it ran before filters existed — and in filtered_kernels.hip, inside
// namespace filtered and with TRI_FILTERED_KERNELS defined: one more argument (FilterSel) and, at the top of every task, `masked` shadowed by the task's own
// bitmap.  Both ways of doing it in ONE translation unit were tried and moved the unfiltered kernels' register allocation (profiles/filters_kernel_resources.txt):
// the selection behind a uniform null test cost k_and_dense and k_fused vector spills and all six kernels scalar ones; a second template instantiation beside
// the first changed the inliner's view of the helpers both call (k_fused<LUCENE, general trees>: 29 -> 62 spilled VGPRs in the instantiation WITHOUT filters).
// k_psets_prep and k_tree_eval — a workgroup per query, registers to spare, the table unchanged — keep the null test.
#pragma once

// what every kernel that drops masked documents is handed beside the index's mask (a batch without filters: rows == nullptr, nothing of it is read)
struct FilterSel {
        const uint32_t *rows;        // [nrows][stride]: filter | mask, rebuilt by every run (k_filter_rows)
        const uint32_t *row_of_slot; // per plan slot: 0 = the index's mask, r >= 1 = rows + (r - 1) * stride
        const DevTask *tasks;        // (for the kernels that know a task by its index only: k_psets, k_probe)
        uint32_t stride;             // words per row
};

// the drop bitmap of the task of plan slot `slot` (uniform: slot is the workgroup's or the wave's; nullptr: nothing is dropped), given the index's mask
__device__ __forceinline__ const uint32_t *filter_pick(const uint32_t *index_masked, const FilterSel &f, const uint32_t slot) {
        const uint32_t r = uni(f.row_of_slot[slot]);
        return r ? f.rows + (size_t)(r - 1u) * f.stride : index_masked;
}
// ... behind a uniform test, in the kernels that are compiled once
__device__ __forceinline__ const uint32_t *filter_pick_if(const uint32_t *index_masked, const FilterSel &f, const uint32_t slot) {
        return f.rows ? filter_pick(index_masked, f, slot) : index_masked;
}
#ifdef TRI_FILTERED_KERNELS
#define TRI_FILTER_ARG , const FilterSel fsel
// (inside the task loop's body: from here on `masked` is the task's bitmap — the index's masked documents and the query's filter)
#define TRI_FILTER_TASK(slot)                                                    \
        const uint32_t *const task_masked_ = filter_pick(masked, fsel, (slot)); \
        const uint32_t *const masked = task_masked_
#define TRI_FILTER_TASK_OF(tix) TRI_FILTER_TASK(uni(fsel.tasks[(tix)].slot))
#else
#define TRI_FILTER_ARG
#define TRI_FILTER_TASK(slot)
#define TRI_FILTER_TASK_OF(tix)
#endif

#ifndef TRI_FILTERED_KERNELS // (the filters' own kernels: trinity_hip.hip's alone)
constexpr int FILTER_WG = 256;

// bits[] zeroed beforehand.  IDs above max_doc are ignored (the segment holds no such document)
__global__ __launch_bounds__(FILTER_WG) void k_filter_scatter(const uint32_t *__restrict__ docids, const size_t n, const uint32_t max_doc, uint32_t *__restrict__ bits) {
        for (size_t i = (size_t)blockIdx.x * FILTER_WG + threadIdx.x; i < n; i += (size_t)gridDim.x * FILTER_WG) {
                const uint32_t d = docids[i];
                if (d <= max_doc)
                        atomicOr(&bits[d >> 5], 1u << (d & 31u));
        }
}

// every word of the bitmap, bit 0 and the bits past max_doc included (no document has those IDs: whatever they hold is never tested — they
// come out set, every time)
__global__ __launch_bounds__(FILTER_WG) void k_filter_complement(uint4 *__restrict__ bits, const size_t n4) {
        for (size_t i = (size_t)blockIdx.x * FILTER_WG + threadIdx.x; i < n4; i += (size_t)gridDim.x * FILTER_WG) {
                const uint4 v = bits[i];
                bits[i] = make_uint4(~v.x, ~v.y, ~v.z, ~v.w);
        }
}

// grid (x, the query's tasks).  RESULT_DOCIDS: task segment after task segment, counts[] documents each; RESULT_BITMAP: the region's words are
// the bitmap's, from the query's first docID window on (bits[] zeroed beforehand, `words` long)
__global__ __launch_bounds__(FILTER_WG) void k_filter_from_docset(const DevQuery *__restrict__ plan, const DevTask *__restrict__ tasks, const uint32_t slot,
                                                                  const uint32_t *__restrict__ out, const uint32_t *__restrict__ counts, const uint32_t max_doc,
                                                                  uint32_t *__restrict__ bits, const size_t words) {
        const DevQuery q = plan[slot];
        const uint32_t t = q.first_task + blockIdx.y;
        const DevTask task = tasks[t];
        if (q.form == RESULT_BITMAP) {
                const size_t w0 = (size_t)task.tile_begin * SPAN_WORDS, nw = (size_t)(task.tile_end - task.tile_begin) * SPAN_WORDS;
                const uint32_t *src = out + task.out_off;
                for (size_t i = (size_t)blockIdx.x * FILTER_WG + threadIdx.x; i < nw && w0 + i < words; i += (size_t)gridDim.x * FILTER_WG)
                        bits[w0 + i] = src[i];
                return;
        }
        const uint32_t n = counts[t];
        const uint32_t *src = out + task.out_off;
        for (uint32_t i = blockIdx.x * FILTER_WG + threadIdx.x; i < n; i += gridDim.x * FILTER_WG) {
                const uint32_t d = src[i];
                if (d <= max_doc)
                        atomicOr(&bits[d >> 5], 1u << (d & 31u));
        }
}

// grid (x, rows): row y = the filter src[y] | the index's masked documents (nullptr: none); n4 = 16-byte units per row
__global__ __launch_bounds__(FILTER_WG) void k_filter_rows(const uint4 *const *__restrict__ src, const uint4 *__restrict__ masked, uint4 *__restrict__ rows, const size_t n4) {
        const uint4 *f = src[blockIdx.y];
        uint4 *row = rows + (size_t)blockIdx.y * n4;
        for (size_t i = (size_t)blockIdx.x * FILTER_WG + threadIdx.x; i < n4; i += (size_t)gridDim.x * FILTER_WG) {
                uint4 v = f[i];
                if (masked) {
                        const uint4 m = masked[i];
                        v.x |= m.x, v.y |= m.y, v.z |= m.z, v.w |= m.w;
                }
                row[i] = v;
        }
}
#endif

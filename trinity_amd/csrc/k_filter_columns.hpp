// k_filter_columns.hpp — column predicates as document filters (tri_filters_from_columns): the drop bitmaps of up to COLFILTER_MAX_PREDS predicates over the
// index's resident columns, in ONE launch.  IndexDocumentsFilter (matches.h:190-201; exec.cpp:1133-1150) where the rule is "price between 10 and 50, in
// stock, category in {3, 17, 40}" and the attributes already lie in HBM (tri_column_create).
// Part of libtrinity_hip.so (MI355X / gfx950); included by trinity_hip.hip.  New code, no reference source.
//
// A workgroup owns COLFILTER_CHUNK consecutive docIDs — 64 words of every predicate's bitmap; the bitmap's extent (filter_words: whole docID windows and a spare
// one) is a multiple of it, so the grid writes every word of every bitmap: no memset, no atomics, no complement pass.
//   reads   each DISTINCT column's values of the chunk come on chip once, 16 bytes a lane, into LDS (COLFILTER_CHUNK x 4 bytes a column); every predicate is then
//           evaluated against the staged values: a call reads each column from HBM once, however many predicates and clauses name it.  Document 0 and documents
//           past max_doc never read a column (the 16-byte unit that holds such a document is loaded value by value, under the test): their staged value is 0 and
//           they hold for no predicate.
//   params  the predicate and clause records are read with wave-uniform indices (scalar loads, scalar registers); a SET clause is a bitset in device memory —
//           at most 8 KB: values below TRI_FACET_MAX_BUCKETS —, gathered per lane.
//   writes  a wave owns COLFILTER_WAVE_DOCS consecutive docIDs: eight ballots of 64 documents a predicate.  Lane l of the first sixteen picks word l of them —
//           half l & 1 of ballot l >> 1 —, ORs the `also` filter's word in, applies the polarity, and the wave stores the predicate's sixteen words with one
//           coalesced 4-byte-a-lane store.
#pragma once

struct DevColColumns { // passed BY VALUE: the distinct columns of the call, in the order the clauses number them
        const uint32_t *col[COLFILTER_MAX_COLUMNS];
};

// grid: the bitmap's extent in words / (COLFILTER_CHUNK / 32); dynamic LDS: ncols * COLFILTER_CHUNK * 4 bytes
__global__ __launch_bounds__(COLFILTER_WG) void k_filter_columns(const DevColPred *__restrict__ preds, const DevColClause *__restrict__ clauses, const uint32_t *__restrict__ sets,
                                                                 const DevColColumns cols, const uint32_t ncols, const uint32_t np, const uint32_t max_doc, const uint32_t keep) {
        extern __shared__ __align__(16) uint32_t cf_vals[]; // [ncols][COLFILTER_CHUNK]
        constexpr uint32_t GROUPS = COLFILTER_WAVE_DOCS / 64; // ballots a wave and predicate
        static_assert(COLFILTER_WAVE_WORDS == 2 * GROUPS && COLFILTER_WAVE_WORDS <= 64 && GROUPS <= 32, "a lane picks one half of one ballot");
        static_assert(COLFILTER_CHUNK % (4 * COLFILTER_WG) == 0, "whole 16-byte units a thread");
        const uint64_t d_base = (uint64_t)blockIdx.x * COLFILTER_CHUNK; // (64-bit: the spare window's docIDs may pass 2^32)

        // ---- stage: every distinct column's values of the chunk
        for (uint32_t c = 0; c < ncols; ++c) {
                const uint32_t *__restrict__ col = cols.col[c];
                uint4 *dst = reinterpret_cast<uint4 *>(cf_vals + c * COLFILTER_CHUNK);
#pragma unroll
                for (uint32_t i = threadIdx.x; i < COLFILTER_CHUNK / 4; i += COLFILTER_WG) {
                        const uint64_t d0 = d_base + 4u * i;
                        uint4 v = make_uint4(0, 0, 0, 0);
                        if (d0 >= 1 && d0 + 3 <= max_doc) { // (d0 is a multiple of 4 and the column's base 256-byte aligned: a 16-byte load)
                                v = *reinterpret_cast<const uint4 *>(col + d0);
                        } else if (d0 <= max_doc) { // the unit of document 0, or the one max_doc ends in: value by value
                                if (d0 >= 1)
                                        v.x = col[d0];
                                if (d0 + 1 <= max_doc)
                                        v.y = col[d0 + 1];
                                if (d0 + 2 <= max_doc)
                                        v.z = col[d0 + 2];
                                if (d0 + 3 <= max_doc)
                                        v.w = col[d0 + 3];
                        }
                        dst[i] = v;
                }
        }
        __syncthreads();

        const uint32_t wave = uni(threadIdx.x >> 6), lane = lane_id();
        const uint32_t local = wave * COLFILTER_WAVE_DOCS + lane; // group g's document of this lane: local + 64 g
        uint32_t valid = 0;                                        // bit g: that document exists (1 .. max_doc)
#pragma unroll
        for (uint32_t g = 0; g < GROUPS; ++g) {
                const uint64_t d = d_base + local + 64u * g;
                valid |= (uint32_t)(d >= 1 && d <= max_doc) << g;
        }
        const size_t word = (size_t)blockIdx.x * (COLFILTER_CHUNK / 32) + wave * COLFILTER_WAVE_WORDS + lane; // (lanes below COLFILTER_WAVE_WORDS)
        constexpr uint32_t ALL = (1u << GROUPS) - 1u;

        for (uint32_t p = 0; p < np; ++p) {
                const DevColPred P = preds[p];
                uint32_t acc = P.any ? 0u : ALL; // bit g: the predicate holds for group g's document
                for (uint32_t k = 0; k < P.nclauses; ++k) {
                        const DevColClause C = clauses[P.first_clause + k];
                        const uint32_t *vals = cf_vals + C.col * COLFILTER_CHUNK + local;
                        uint32_t t = 0;
                        if (C.kind == COLFILTER_RANGE) {
#pragma unroll
                                for (uint32_t g = 0; g < GROUPS; ++g) {
                                        const uint32_t v = vals[64u * g];
                                        t |= (uint32_t)(v >= C.lo && v <= C.hi) << g;
                                }
                        } else {
                                const uint32_t *__restrict__ set = sets + C.set_off;
#pragma unroll
                                for (uint32_t g = 0; g < GROUPS; ++g) {
                                        const uint32_t v = vals[64u * g];
                                        if (v < C.hi) // (the bitset ends at C.hi bits)
                                                t |= ((set[v >> 5] >> (v & 31u)) & 1u) << g;
                                }
                        }
                        if (C.negate)
                                t ^= ALL;
                        acc = P.any ? (acc | t) : (acc & t);
                }
                acc &= valid;
                uint32_t mine = 0;
#pragma unroll
                for (uint32_t g = 0; g < GROUPS; ++g) {
                        const uint64_t b = __ballot((acc >> g) & 1u);
                        if ((lane >> 1) == g)
                                mine = lane & 1u ? (uint32_t)(b >> 32) : (uint32_t)b;
                }
                if (lane < COLFILTER_WAVE_WORDS) {
                        uint32_t w = keep ? ~mine : mine;
                        if (P.also)
                                w |= P.also[word];
                        P.out[word] = w;
                }
        }
}

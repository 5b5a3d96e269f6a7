// result_rows.hpp — the host transforms of the read side (read_side.hpp) between the layout a result has on the device and the one the caller asked for:
// plain functions over pointers and counts, no HIP, so that they compile and are tested on a CPU alone (tests/cpp/result_rows_cpu_test.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace result_rows {
        struct Segment { // a task segment's share of a per-match column: its first cell, its matches
                size_t first;
                uint32_t count;
        };

        // tri_batch_matched_terms_wide's masks.  A segment's 32-bit low words were copied into the UPPER half of the segment's own u64 cells (words count .. 2 count
        // of them); each cell becomes low | high << 32, in place, front to back: cell i is written from word count + i, which no earlier cell's store reaches.
        // hi: the high words, indexed like present64 — NULL: zero (a query of at most 16 reportable terms)
        inline void widen(uint64_t *present64, const Segment *segs, const size_t nsegs, const uint32_t *hi) {
                for (size_t s = 0; s < nsegs; ++s) {
                        const uint32_t *lo = reinterpret_cast<const uint32_t *>(present64 + segs[s].first) + segs[s].count;
                        for (size_t i = 0; i < segs[s].count; ++i) {
                                uint32_t l;
                                memcpy(&l, lo + i, 4);
                                present64[segs[s].first + i] = (uint64_t)l | (hi ? (uint64_t)hi[segs[s].first + i] << 32 : 0ull);
                        }
                }
        }

        // frequency rows: `stride` cells apart as the device keeps them, nscore (<= stride) wide for the caller
        inline void narrow(uint16_t *out, const uint16_t *rows, const size_t c, const uint32_t stride, const uint32_t nscore) {
                for (size_t i = 0; i < c; ++i)
                        for (uint32_t k = 0; k < nscore; ++k)
                                out[i * nscore + k] = rows[i * stride + k];
        }

        // a result bitmap (bit j of words[i]: document (first_word + i) * 32 + j matches) as ascending docIDs.  The tasks counted n matches: a bitmap that holds
        // more is EXPAND_MORE (nothing is written at out[n] or beyond), one that holds fewer EXPAND_FEWER; *got = the docIDs written
        enum { EXPAND_OK = 0, EXPAND_MORE = 1, EXPAND_FEWER = 2 };
        inline int expand(const uint32_t *words, const size_t nwords, const size_t first_word, uint32_t *out, const size_t n, size_t *got) {
                size_t w = 0;
                for (size_t i = 0; i < nwords; ++i)
                        for (uint32_t m = words[i]; m; m &= m - 1u) {
                                if (w == n) {
                                        *got = w;
                                        return EXPAND_MORE;
                                }
                                out[w++] = (uint32_t)((first_word + i) * 32u + (uint32_t)__builtin_ctz(m));
                        }
                *got = w;
                return w == n ? EXPAND_OK : EXPAND_FEWER;
        }
} // namespace result_rows

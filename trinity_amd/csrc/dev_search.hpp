// dev_search.hpp — the scalar searches of the device headers: one lane bisecting or galloping over a sorted run of uint32_t, and
// term_block_range ("which blocks of this term reach a docID range") built on them.  Plain C++17, no HIP intrinsics: tests/cpp/dev_search_cpu_test.cpp compiles it with g++.
#pragma once
#include "dev_structs.hpp"

// (TRI_HD is dev_structs.hpp's bare __host__ __device__, which constexpr functions and members take too; the searches add the inlining)
#if defined(__HIPCC__)
#define TRI_HDI TRI_HD __forceinline__
#else
#define TRI_HDI inline
#endif

// Element i of `get`: a pointer or an array is indexed, anything else is called (i -> uint32_t), so that sh.cand[phys(i)] fits.
template <typename T> TRI_HDI uint32_t search_at(const T *a, const uint32_t i) { return a[i]; }
template <typename F> TRI_HDI auto search_at(const F get, const uint32_t i) -> decltype((uint32_t)get(i)) { return get(i); }

// The first index in [lo, hi) whose element is >= key (hi: none).
template <typename G> TRI_HDI uint32_t first_ge(const G get, uint32_t lo, uint32_t hi, const uint32_t key) {
        while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (search_at(get, mid) < key)
                        lo = mid + 1;
                else
                        hi = mid;
        }
        return lo;
}

// The first index in [lo, hi) whose element is > key (hi: none).
template <typename G> TRI_HDI uint32_t first_gt(const G get, uint32_t lo, uint32_t hi, const uint32_t key) {
        while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (search_at(get, mid) <= key)
                        lo = mid + 1;
                else
                        hi = mid;
        }
        return lo;
}

// The first index in [from, C) whose element is >= key (C: none), found by GALLOPING from `from`: a block of a rare term spans the docID range of
// thousands of candidates, and the lane that merges it must not walk them one by one (measured: a 21-document list against a tile of 8192
// candidates took 680 us of single-lane LDS reads — cfg3's k_and spent half its span in a handful of such tiles)
template <typename G> TRI_HDI uint32_t gallop_ge(const G get, const uint32_t from, const uint32_t C, const uint32_t key) {
        uint32_t step = 1, lo = from;
        while (lo + step <= C && search_at(get, lo + step - 1) < key) {
                lo += step;
                step <<= 1;
        }
        const uint32_t end = lo + step - 1;
        return first_ge(get, lo, end < C ? end : C, key);
}

// The blocks of term t that reach [d_lo, d_hi): the first block whose last docID is >= d_lo, and the first whose last docID is >= d_hi (it may still begin
// inside the range; t.nblocks: none).  With a cell index both are one load, which asks for CELL-ALIGNED bounds (window starts are).
struct BlockRange {
        uint32_t lo, hi;
};
TRI_HDI BlockRange term_block_range(const uint32_t *bl, const uint32_t *win, const DevTerm &t, const uint32_t d_lo, const uint32_t d_hi) {
        if (t.win_off != 0xffffffffu)
                return {win[t.win_off + (d_lo >> CELL_LOG2)], win[t.win_off + (d_hi >> CELL_LOG2)]};
        const uint32_t lo = first_ge(bl, 0u, t.nblocks, d_lo);
        return {lo, first_ge(bl, lo, t.nblocks, d_hi)};
}

// dev_search_cpu_test.cpp — the kernels' scalar searches (trinity_amd/csrc/dev_search.hpp) on the CPU, against std::lower_bound, std::upper_bound and a
// linear scan.  Stand-alone (tests/test_dev_search_cpu.py builds it with AddressSanitizer and UndefinedBehaviorSanitizer and runs it): every sorted array
// of 0 .. 9 elements over VALUES (duplicates included), every lo <= hi sub-range, keys below, between, equal to and above the elements, gallop_ge from
// every start, one run through a permuting accessor (the LDS layout's phys()), and term_block_range with and without a cell index.
#include "../../trinity_amd/csrc/dev_search.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

static const uint32_t VALUES[] = {1u, 2u, 5u, 9u, 0xffffffffu};
static const uint32_t KEYS[] = {0u, 1u, 2u, 3u, 5u, 6u, 9u, 10u, 0xfffffffeu, 0xffffffffu};

static void fail(const char *what, const std::vector<uint32_t> &a, const uint32_t lo, const uint32_t hi, const uint32_t key, const uint32_t got, const uint32_t want) {
        std::printf("%s: n=%zu [%u, %u) key=%u: got %u, want %u\n", what, a.size(), lo, hi, key, got, want);
        std::exit(1);
}

static unsigned long long n_arrays, n_ge, n_gt, n_gallop;

static void check_array(const std::vector<uint32_t> &a) {
        ++n_arrays;
        const uint32_t n = (uint32_t)a.size();
        const uint32_t *p = a.data(); // (n == 0: never dereferenced)
        for (const uint32_t key : KEYS) {
                for (uint32_t lo = 0; lo <= n; ++lo)
                        for (uint32_t hi = lo; hi <= n; ++hi) {
                                const uint32_t ge = (uint32_t)(std::lower_bound(a.begin() + lo, a.begin() + hi, key) - a.begin());
                                const uint32_t gt = (uint32_t)(std::upper_bound(a.begin() + lo, a.begin() + hi, key) - a.begin());
                                if (const uint32_t got = first_ge(p, lo, hi, key); got != ge)
                                        fail("first_ge", a, lo, hi, key, got, ge);
                                if (const uint32_t got = first_gt(p, lo, hi, key); got != gt)
                                        fail("first_gt", a, lo, hi, key, got, gt);
                                ++n_ge, ++n_gt;
                        }
                for (uint32_t from = 0; from <= n; ++from) { // (from == n: nothing to look at; a key beyond the last element: n)
                        uint32_t want = from;
                        while (want < n && a[want] < key)
                                ++want;
                        if (const uint32_t got = gallop_ge(p, from, n, key); got != want)
                                fail("gallop_ge", a, from, n, key, got, want);
                        ++n_gallop;
                }
        }
}

static void every_array(std::vector<uint32_t> &a, const size_t len, const size_t from_value) {
        if (a.size() == len) {
                check_array(a);
                return;
        }
        for (size_t v = from_value; v < sizeof(VALUES) / sizeof(VALUES[0]); ++v) {
                a.push_back(VALUES[v]);
                every_array(a, len, v);
                a.pop_back();
        }
}

// the candidate tiles' LDS layout (k_match.hpp: phys()): every row of 32 slots rotated by its row number
static uint32_t phys(const uint32_t j) { return (j & ~31u) | ((j + (j >> 5)) & 31u); }

static unsigned long long permuted_run() {
        const uint32_t C = 100;
        std::vector<uint32_t> a(C), store(128, 0xdeadbeefu);
        for (uint32_t j = 0; j < C; ++j) {
                a[j] = 3u * (j / 2u) + 1u; // 1 1 4 4 7 7 ...: duplicates, gaps
                store[phys(j)] = a[j];
        }
        const auto at = [&store](const uint32_t j) { return store[phys(j)]; };
        unsigned long long cases = 0;
        for (uint32_t key = 0; key <= a[C - 1] + 2u; ++key) {
                const uint32_t ge = (uint32_t)(std::lower_bound(a.begin(), a.end(), key) - a.begin());
                const uint32_t gt = (uint32_t)(std::upper_bound(a.begin(), a.end(), key) - a.begin());
                if (const uint32_t got = first_ge(at, 0u, C, key); got != ge)
                        fail("first_ge (permuted)", a, 0, C, key, got, ge);
                if (const uint32_t got = first_gt(at, 0u, C, key); got != gt)
                        fail("first_gt (permuted)", a, 0, C, key, got, gt);
                for (uint32_t from = 0; from <= C; ++from) {
                        const uint32_t want = std::max(from, ge);
                        if (const uint32_t got = gallop_ge(at, from, C, key); got != want)
                                fail("gallop_ge (permuted)", a, from, C, key, got, want);
                        ++cases;
                }
        }
        return cases;
}

// a term of 40 blocks whose last docIDs lie 700 apart (a cell of CELL_DOCS documents holds one or two block ends), with and without its cell index
static unsigned long long term_run() {
        const uint32_t nblocks = 40;
        std::vector<uint32_t> bl(nblocks);
        for (uint32_t b = 0; b < nblocks; ++b)
                bl[b] = 700u * (b + 1u);
        const uint32_t ncells = bl[nblocks - 1] / CELL_DOCS + 3u;
        std::vector<uint32_t> win(5u + ncells);
        for (uint32_t c = 0; c < ncells; ++c) // (win[c]: the first block whose last docID reaches the cell's first docID)
                win[5u + c] = (uint32_t)(std::lower_bound(bl.begin(), bl.end(), c * CELL_DOCS) - bl.begin());
        DevTerm plain{}, indexed{};
        plain.nblocks = indexed.nblocks = nblocks;
        plain.win_off = 0xffffffffu;
        indexed.win_off = 5u;
        unsigned long long cases = 0;
        for (uint32_t c_lo = 0; c_lo + 1 < ncells; ++c_lo)
                for (uint32_t c_hi = c_lo; c_hi + 1 < ncells; ++c_hi) {
                        const uint32_t d_lo = c_lo * CELL_DOCS, d_hi = c_hi * CELL_DOCS;
                        const uint32_t lo = (uint32_t)(std::lower_bound(bl.begin(), bl.end(), d_lo) - bl.begin());
                        const uint32_t hi = (uint32_t)(std::lower_bound(bl.begin(), bl.end(), d_hi) - bl.begin());
                        const BlockRange p = term_block_range(bl.data(), win.data(), plain, d_lo, d_hi), x = term_block_range(bl.data(), win.data(), indexed, d_lo, d_hi);
                        if (p.lo != lo || p.hi != hi || x.lo != lo || x.hi != hi)
                                fail("term_block_range", bl, d_lo, d_hi, 0, p.lo, lo);
                        ++cases;
                }
        return cases;
}

int main() {
        for (size_t len = 0; len <= 9; ++len) {
                std::vector<uint32_t> a;
                every_array(a, len, 0);
        }
        std::printf("arrays: %llu\nfirst_ge: %llu cases\nfirst_gt: %llu cases\ngallop_ge: %llu cases\n", n_arrays, n_ge, n_gt, n_gallop);
        std::printf("permuted: %llu cases\n", permuted_run());
        std::printf("terms: %llu cases\n", term_run());
        std::printf("ok\n");
        return 0;
}

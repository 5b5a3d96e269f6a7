// result_rows_cpu_test.cpp — the read side's host transforms (trinity_amd/csrc/host/result_rows.hpp) against naive out-of-place restatements, as a stand-alone
// program (tests/test_result_rows_cpu.py compiles it with AddressSanitizer and UndefinedBehaviorSanitizer and runs it directly).  Every array is allocated at its
// exact size, so that a store or a load beyond it is the sanitizer's to report.  Prints one line per group of cases and "ok"; exit status 1 on a mismatch.
#include "../../trinity_amd/csrc/host/result_rows.hpp"

#include <algorithm>
#include <cstdio>
#include <vector>

namespace R = result_rows;
static int failures = 0, n_more = 0, n_fewer = 0;
constexpr size_t SPAN_WORDS = 4096; // words per docID window (dev_structs.hpp)
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { // xorshift64*
        rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
        return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}
#define CHECK(cond, ...)                          \
        do {                                      \
                if (!(cond)) {                    \
                        ++failures;               \
                        printf("FAIL " __VA_ARGS__); \
                        printf("\n");             \
                }                                 \
        } while (0)

// ---- widen: `nsegs` segments of `count` matches each, back to back
static void widen_case(const size_t nsegs, const uint32_t count, const bool with_hi) {
        const size_t n = nsegs * count;
        std::vector<uint32_t> lo(n), hi(n);
        for (size_t i = 0; i < n; ++i)
                lo[i] = rnd(), hi[i] = rnd();
        std::vector<uint64_t> want(n); // the restatement: out of place
        for (size_t i = 0; i < n; ++i)
                want[i] = (uint64_t)lo[i] | (with_hi ? (uint64_t)hi[i] << 32 : 0ull);
        // the layout the read-backs leave: a segment's low words in the upper half of its own cells, the lower half garbage
        std::vector<uint64_t> cells(n, 0xa5a5a5a5a5a5a5a5ull);
        std::vector<R::Segment> segs;
        for (size_t s = 0; s < nsegs; ++s) {
                segs.push_back({s * count, count});
                if (count)
                        memcpy(reinterpret_cast<uint32_t *>(cells.data() + s * count) + count, lo.data() + s * count, (size_t)count * 4);
        }
        R::widen(cells.data(), segs.data(), segs.size(), with_hi ? hi.data() : nullptr);
        CHECK(cells == want, "widen: %zu segments of %u, hi %d", nsegs, count, (int)with_hi);
}

// ---- narrow
static void narrow_case(const uint32_t stride, const uint32_t nscore, const size_t c) {
        std::vector<uint16_t> rows(c * stride);
        for (auto &x : rows)
                x = (uint16_t)rnd();
        std::vector<uint16_t> want;
        for (size_t i = 0; i < c; ++i)
                for (uint32_t k = 0; k < nscore; ++k)
                        want.push_back(rows[i * stride + k]);
        std::vector<uint16_t> got(c * nscore, 0xbeef);
        R::narrow(got.data(), rows.data(), c, stride, nscore);
        CHECK(got == want, "narrow: stride %u nscore %u rows %zu", stride, nscore, c);
}

// ---- expand: `words` from window word `first_word` on; n = what the tasks counted
static void expand_case(const std::vector<uint32_t> &words, const size_t first_word, const long delta, const char *name) {
        std::vector<uint32_t> all; // the restatement: bit by bit
        for (size_t i = 0; i < words.size(); ++i)
                for (uint32_t j = 0; j < 32; ++j)
                        if (words[i] >> j & 1u)
                                all.push_back((uint32_t)((first_word + i) * 32 + j));
        if (delta < 0 && all.size() < (size_t)-delta)
                return;
        const size_t n = all.size() + delta;
        const uint32_t GUARD = 0xdeadbeefu;
        std::vector<uint32_t> out(n + 1, GUARD); // out[n]: the guard cell
        size_t got = ~(size_t)0;
        const int rc = R::expand(words.data(), words.size(), first_word, out.data(), n, &got);
        const size_t written = std::min(n, all.size());
        n_more += rc == R::EXPAND_MORE, n_fewer += rc == R::EXPAND_FEWER;
        CHECK(rc == (delta < 0 ? R::EXPAND_MORE : delta > 0 ? R::EXPAND_FEWER : R::EXPAND_OK), "expand %s delta %ld: rc %d", name, delta, rc);
        CHECK(got == written, "expand %s delta %ld: got %zu of %zu", name, delta, got, written);
        CHECK(std::vector<uint32_t>(out.begin(), out.begin() + written) == std::vector<uint32_t>(all.begin(), all.begin() + written), "expand %s delta %ld: docIDs", name, delta);
        for (size_t i = written; i <= n; ++i)
                CHECK(out[i] == GUARD, "expand %s delta %ld: a store at out[%zu] (n = %zu)", name, delta, i, n);
}

int main() {
        for (const size_t nsegs : {1, 2, 5})
                for (const uint32_t count : {0u, 1u, 2u, 3u, 64u, 65u})
                        for (const bool with_hi : {false, true})
                                widen_case(nsegs, count, with_hi);
        R::widen(nullptr, nullptr, 0, nullptr); // (a call that asked for no masks)
        printf("widen: 36 cases\n");
        const uint32_t shapes[4][2] = {{8, 1}, {24, 17}, {64, 64}, {16, 5}};
        for (const auto &sh : shapes)
                for (const size_t c : {0, 1, 2049})
                        narrow_case(sh[0], sh[1], c);
        printf("narrow: 12 cases\n");
        std::vector<uint32_t> mixed = {0u, 1u << 7, 0xffffffffu, 0u, 0x80000001u, rnd(), rnd(), 0xffffffffu};
        const struct {
                const char *name;
                std::vector<uint32_t> words;
        } bitmaps[] = {{"empty", {}}, {"zero words", {0u, 0u, 0u}}, {"one bit", {1u << 31}}, {"full word", {0xffffffffu}}, {"mixed", mixed}};
        for (const auto &bm : bitmaps)
                for (const size_t first_word : {(size_t)0, 3 * SPAN_WORDS, ((size_t)1 << 27) - 8}) // (window 3; the last: the eight-word bitmap ends at docID 2^32 - 1)
                        for (const long delta : {0l, -1l, 1l})
                                expand_case(bm.words, first_word, delta, bm.name);
        printf("expand: more %d fewer %d\n", n_more, n_fewer);
        if (failures)
                return printf("%d failures\n", failures), 1;
        printf("ok\n");
        return 0;
}

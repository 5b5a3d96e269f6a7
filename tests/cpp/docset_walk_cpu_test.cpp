// docset_walk_cpu_test.cpp — the consumers' walk of a task's documents (trinity_amd/csrc/docset_walk.hpp: docset_for_each_of, what docset_for_each runs per thread) on
// the CPU.  Stand-alone (tests/test_docset_walk_cpu.py builds it with AddressSanitizer and UndefinedBehaviorSanitizer and runs it): the WG threads' shares of a task,
// taken one after the other, must hand over every document exactly once with the right docID — segments of 0, 1, WG - 1, WG and WG + 1 documents, and a RESULT_BITMAP
// task of one window whose words are all zero, a single bit at position 0, a single bit at position 31 of the last word, and all ones.
#include "../../trinity_amd/csrc/docset_walk.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

static constexpr uint32_t WG = 256, OUT_OFF = 3, TILE = 2; // (the task's region starts inside out[]; its window is the third)

// every thread's share, in thread order; exits unless it is `want` as a multiset with no docID twice
static void check(const char *what, const DevQuery &q, const DevTask &tk, const uint32_t c, const std::vector<uint32_t> &out, std::vector<uint32_t> want) {
        std::vector<uint32_t> got;
        for (uint32_t tid = 0; tid < WG; ++tid)
                docset_for_each_of<WG>(tid, q, tk, c, out.data(), [&](const uint32_t d) { got.push_back(d); });
        std::sort(got.begin(), got.end());
        std::sort(want.begin(), want.end());
        if (got != want) {
                std::printf("%s: %zu documents handed over, %zu expected (first %u / %u)\n", what, got.size(), want.size(), got.empty() ? 0u : got[0], want.empty() ? 0u : want[0]);
                std::exit(1);
        }
        std::printf("%s: %zu documents\n", what, got.size());
}

int main() {
        DevQuery q{};
        DevTask tk{};
        tk.out_off = OUT_OFF;
        q.form = RESULT_DOCIDS;
        for (const uint32_t c : {0u, 1u, WG - 1, WG, WG + 1}) {
                std::vector<uint32_t> out(OUT_OFF, 0xdeadbeefu), want; // (the words ahead of the segment are not the task's)
                for (uint32_t i = 0; i < c; ++i)
                        want.push_back(7u * i + 1u);
                out.insert(out.end(), want.begin(), want.end());
                out.push_back(0xdeadbeefu); // ... nor is the one behind it
                char what[32];
                std::snprintf(what, sizeof what, "segment %u", c);
                check(what, q, tk, c, out, want);
        }
        q.form = RESULT_BITMAP;
        tk.tile_begin = TILE;
        tk.tile_end = TILE + 1;
        const uint32_t first = TILE * SPAN_WORDS * 32u; // the window's first docID
        const auto bitmap = [&](const char *what, const uint32_t fill, const uint32_t word, const uint32_t bits, const std::vector<uint32_t> &want) {
                std::vector<uint32_t> out(OUT_OFF + SPAN_WORDS + 1, 0xffffffffu); // (all ones around the window: a word read past it would show)
                std::fill(out.begin() + OUT_OFF, out.begin() + OUT_OFF + SPAN_WORDS, fill);
                if (bits)
                        out[OUT_OFF + word] = bits;
                check(what, q, tk, (uint32_t)want.size(), out, want);
        };
        bitmap("bitmap all zero", 0u, 0u, 0u, {});
        bitmap("bitmap bit 0", 0u, 0u, 1u, {first});
        bitmap("bitmap bit 31 of the last word", 0u, SPAN_WORDS - 1, 0x80000000u, {first + (SPAN_WORDS - 1) * 32u + 31u});
        std::vector<uint32_t> all;
        for (uint32_t d = 0; d < SPAN_WORDS * 32u; ++d)
                all.push_back(first + d);
        bitmap("bitmap all ones", 0xffffffffu, 0u, 0u, all);
        std::printf("ok\n");
        return 0;
}

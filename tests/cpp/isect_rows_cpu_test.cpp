// isect_rows_cpu_test.cpp — csrc/host/isect_rows.hpp's replay (the reference's intersect list from tables H and C) on the CPU: a stand-alone program, built with
// AddressSanitizer + UndefinedBehaviorSanitizer and run directly by tests/test_isect_cases.py, over the vectors tests/isect_cases.py dumped (dump_vectors):
// per case H, C and the list its line-by-line restatement of intersect.cpp:64-99 produced.
#include "../../trinity_amd/csrc/host/isect_rows.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char **argv) {
        if (argc != 2) {
                fprintf(stderr, "usage: %s <vectors>\n", argv[0]);
                return 2;
        }
        FILE *f = fopen(argv[1], "r");
        if (!f) {
                perror(argv[1]);
                return 2;
        }
        size_t ncases = 0, credited = 0, deleted = 0;
        unsigned long long nh, nc, nr;
        while (fscanf(f, " case %llu %llu %llu", &nh, &nc, &nr) == 3) {
                std::vector<isect_rows::HEntry> H;
                std::vector<isect_rows::CEntry> C;
                std::vector<std::pair<uint64_t, uint32_t>> want;
                unsigned long long a;
                unsigned b, c;
                for (size_t i = 0; i < nh; ++i) {
                        if (fscanf(f, " h %llu %u %u", &a, &b, &c) != 3)
                                return 3;
                        H.push_back({a, b, c});
                }
                for (size_t i = 0; i < nc; ++i) {
                        if (fscanf(f, " c %llu %u %u", &a, &b, &c) != 3)
                                return 3;
                        C.push_back({a, b, c});
                }
                for (size_t i = 0; i < nr; ++i) {
                        if (fscanf(f, " r %llu %u", &a, &b) != 2)
                                return 3;
                        want.emplace_back(a, b);
                }
                // the thresholds agree with where C's entries lie: an entry's mask has a strict superset
                std::vector<isect_rows::HEntry> sorted = H;
                isect_rows::sort_by_first(sorted);
                const std::vector<uint32_t> thr = isect_rows::thresholds(sorted);
                for (const auto &e : C) {
                        bool ok = false;
                        for (size_t i = 0; i < sorted.size(); ++i)
                                ok |= sorted[i].mask == e.mask && thr[i] != isect_rows::NEVER && e.epoch >= 1 && e.epoch <= sorted.size();
                        if (!ok) {
                                printf("case %zu: a C entry of mask %llu without a threshold\n", ncases, (unsigned long long)e.mask);
                                return 1;
                        }
                }
                // C handed over in reverse order too: the replay does not depend on it
                std::vector<isect_rows::CEntry> rev(C.rbegin(), C.rend());
                const auto got = isect_rows::replay(H, C), got2 = isect_rows::replay(H, rev);
                if (got != want || got2 != want) {
                        printf("case %zu: %zu entries, want %zu\n", ncases, got.size(), want.size());
                        for (size_t i = 0; i < got.size() || i < want.size(); ++i)
                                printf("  got %llx:%u want %llx:%u\n", i < got.size() ? (unsigned long long)got[i].first : 0ull, i < got.size() ? got[i].second : 0u,
                                       i < want.size() ? (unsigned long long)want[i].first : 0ull, i < want.size() ? want[i].second : 0u);
                        return 1;
                }
                credited += !C.empty();
                deleted += want.size() < H.size();
                ++ncases;
        }
        fclose(f);
        // an empty request
        if (!isect_rows::replay({}, {}).empty())
                return 1;
        printf("replay: %zu cases, %zu with credits, %zu with deleted or covered masks\nok\n", ncases, credited, deleted);
        return 0;
}

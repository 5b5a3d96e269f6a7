// crank_blend_test.cpp — ProximityRanker::blend (trinity_amd/csrc/host/trinity_gpu.hpp) on its own: no engine, no device.  A stand-alone program: it reads the
// per-source ranked lists of a case from a file, hands them to blend() and prints the blended list.  tests/test_crank_cases.py builds it with AddressSanitizer +
// UndefinedBehaviorSanitizer, runs it directly and compares the lines with tests/crank_cases.py.
//   usage: crank_blend_test <cases file>
//   cases file, text:  case <name> <K> <nparts>  then per part a line  <n> <doc>:<score bits, u64 decimal> ...
//   output per case:   <name> <count> then " <doc>:<score bits>", best first
#include "../../trinity_amd/csrc/host/trinity_gpu.hpp"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

using namespace trinity_amd;

int main(int argc, char **argv) {
        if (argc < 2)
                return 2;
        FILE *f = fopen(argv[1], "r");
        if (!f)
                return 2;
        char name[128], tag[16];
        while (fscanf(f, "%15s %127s", tag, name) == 2) {
                unsigned K, nparts;
                if (strcmp(tag, "case") || fscanf(f, "%u %u", &K, &nparts) != 2)
                        return 3;
                std::vector<std::unique_ptr<ProximityRanker>> parts;
                for (unsigned p = 0; p < nparts; ++p) {
                        size_t n;
                        if (fscanf(f, "%zu", &n) != 1)
                                return 3;
                        parts.push_back(std::make_unique<ProximityRanker>(K));
                        for (size_t i = 0; i < n; ++i) {
                                uint32_t doc;
                                uint64_t bits;
                                if (fscanf(f, "%" SCNu32 ":%" SCNu64, &doc, &bits) != 2)
                                        return 3;
                                double score;
                                memcpy(&score, &bits, 8);
                                parts.back()->list.emplace_back(doc, score);
                        }
                }
                const auto list = ProximityRanker::blend(parts, K);
                printf("%s %zu", name, list.size());
                for (const auto &e : list) {
                        uint64_t bits;
                        memcpy(&bits, &e.second, 8);
                        printf(" %u:%" PRIu64, e.first, bits);
                }
                printf("\n");
        }
        fclose(f);
        return 0;
}

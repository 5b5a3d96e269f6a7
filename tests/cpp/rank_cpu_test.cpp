// rank_cpu_test.cpp — ProximityRanker::consider (trinity_amd/csrc/host/trinity_gpu.hpp) on its own: no engine, no device.  A stand-alone program: it reads the CPU
// oracle's default-mode records from a file, builds the matched_document each record stands for, feeds them to a ProximityRanker and prints the list it keeps.
// tests/test_rank_cpu.py builds it with AddressSanitizer + UndefinedBehaviorSanitizer, runs it directly and compares the lines with tests/rank_cases.py.
//   usage: rank_cpu_test <cases file>
//   cases file, text, one case after another:
//     case <name> <topk> <freq_cap> <adjacency, hexfloat> <nslots> <weight per slot, hexfloat ...> <nslots slot terms ...> <nwords>
//     <nwords u32 words: per match  doc, nterms, then per matched term  term, freq, positions[freq]>
//   output per case:  <name> <count> then per kept match " <doc>:<score bits, u64 decimal>", best first
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
                unsigned topk, cap, nslots;
                double adj;
                if (strcmp(tag, "case") || fscanf(f, "%u %u %la %u", &topk, &cap, &adj, &nslots) != 4 || nslots > 64)
                        return 3;
                std::vector<double> w(nslots);
                std::vector<uint32_t> slotTerm(nslots);
                for (auto &x : w)
                        if (fscanf(f, "%la", &x) != 1)
                                return 3;
                for (auto &x : slotTerm)
                        if (fscanf(f, "%" SCNu32, &x) != 1)
                                return 3;
                size_t nwords;
                if (fscanf(f, "%zu", &nwords) != 1)
                        return 3;
                std::vector<uint32_t> flat(nwords);
                for (auto &x : flat)
                        if (fscanf(f, "%" SCNu32, &x) != 1)
                                return 3;
                std::vector<query_term_ctx> qctx(nslots);
                for (unsigned k = 0; k < nslots; ++k) {
                        qctx[k].term.id = exec_term_id_t(k + 1);
                        qctx[k].term.token = "t" + std::to_string(slotTerm[k]);
                }
                ProximityRanker r(topk, cap, adj, w);
                size_t at = 0;
                while (at < nwords) {
                        matched_document md;
                        md.id = flat[at];
                        const uint32_t nt = flat[at + 1];
                        at += 2;
                        std::vector<std::vector<term_hit>> store(nt);
                        std::vector<term_hits> th(nt);
                        std::vector<matched_query_term> mts(nt);
                        // (matchedTerms[] in the record's order — ascending TERM id, not slot order: consider() must not depend on it)
                        for (uint32_t i = 0; i < nt; ++i) {
                                const uint32_t term = flat[at], freq = flat[at + 1];
                                at += 2;
                                store[i].resize(freq);
                                for (uint32_t h = 0; h < freq; ++h)
                                        store[i][h].pos = tokenpos_t(flat[at + h]);
                                at += freq;
                                th[i].freq = tokenpos_t(freq);
                                th[i].all = store[i].data();
                                const size_t k = size_t(std::find(slotTerm.begin(), slotTerm.end(), term) - slotTerm.begin());
                                if (k == nslots)
                                        return 4;
                                mts[i] = {&qctx[k], &th[i]};
                        }
                        md.matchedTermsCnt = uint16_t(nt);
                        md.matchedTerms = mts.data();
                        r.consider(md);
                }
                const auto list = r.ranked();
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

// host_mirror_rank_test.cpp — exec_query's default mode with a ProximityRanker (trinity_amd/csrc/host/trinity_gpu.hpp): every query runs twice, once ranked on the
// device (device = true: tri_batch_set_ranker, K pairs come back, no match is replayed) and once through the per-match replay into ProximityRanker::consider
// (device = false).  Both lists are printed for tests/test_host_mirror_rank.py, which compares them with each other and with tests/rank_cases.py.
//   usage: host_mirror_rank_test <index file> <terms file (u32 triples)> <docsCnt>
//   output per query and path:  <name> <dev|host> <count> then " <doc>:<score bits, u64 decimal>", best first
#include "../../trinity_amd/csrc/host/trinity_gpu.hpp"
#include <cinttypes>
#include <cstdio>
#include <fstream>

using namespace trinity_amd;

int main(int argc, char **argv) {
        if (argc < 4)
                return 2;
        std::ifstream fi(argv[1], std::ios::binary);
        std::vector<uint8_t> index((std::istreambuf_iterator<char>(fi)), std::istreambuf_iterator<char>());
        std::ifstream ft(argv[2], std::ios::binary);
        std::vector<char> tb((std::istreambuf_iterator<char>(ft)), std::istreambuf_iterator<char>());
        const size_t nterms = tb.size() / 12;
        std::vector<term_index_ctx> tctx(nterms);
        memcpy(tctx.data(), tb.data(), nterms * 12);
        std::vector<std::string> names(nterms);
        field_statistics fs;
        for (size_t i = 0; i < nterms; ++i) {
                names[i] = "t" + std::to_string(i);
                fs.sumTermsDocs += tctx[i].documents;
                fs.totalTerms += tctx[i].documents != 0;
        }
        fs.docsCnt = uint32_t(strtoul(argv[3], nullptr, 10));
        try {
                IndexSource src(0, index.data(), index.size(), names, tctx, fs);
                auto t = [&](int i) { return src.term("t" + std::to_string(i)); };
                struct Q {
                        const char *name;
                        std::function<DocsSetIterators::Iterator *()> make;
                };
                const std::vector<Q> qs = {
                    {"and2", [&] { return src.conjunction({t(0), t(1)}); }},
                    {"or3", [&] { return src.disjunction({t(0), t(1), t(2)}); }},
                    {"phrases", [&] { return src.disjunction({src.phrase({"t0", "t1"}), src.phrase({"t1", "t2"}), src.phrase({"t2", "t3"})}); }},
                    {"opt", [&] { return src.optional(t(0), src.phrase({"t1", "t2"})); }},
                    {"and3", [&] { return src.conjunction({t(3), t(1), t(0)}); }},
                    {"none", [&] { return src.conjunction({t(0), t(int(nterms) - 1), t(int(nterms) - 2), t(int(nterms) - 3)}); }},
                };
                for (const Q &q : qs)
                        for (const bool device : {true, false}) {
                                ProximityRanker r(10, 3, 4.0, {1.0, 2.0, 3.0, 1.0, 2.0, 3.0}); // (1 + k % 3)
                                r.device = device;
                                exec_query(q.make(), &src, &r);
                                const auto list = r.ranked();
                                printf("%s %s %zu", q.name, device ? "dev" : "host", list.size());
                                for (const auto &e : list) {
                                        uint64_t bits;
                                        memcpy(&bits, &e.second, 8);
                                        printf(" %u:%" PRIu64, e.first, bits);
                                }
                                printf("\n");
                        }
        } catch (const std::exception &e) {
                printf("EXCEPTION %s\n", e.what());
                return 1;
        }
        return 0;
}

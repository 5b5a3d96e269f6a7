// host_mirror_collection_test.cpp — the collection surface of trinity_amd/csrc/host/trinity_gpu.hpp: IndexSourcesCollection, exec_query's collection form (one
// ProximityRanker per source, each source run under the registry of the sources newer than it) and ProximityRanker::blend.  Every query runs twice, ranked on the
// device (device = true) and through the per-match replay (device = false); the blended lists are printed for tests/test_host_mirror_collection.py, which
// compares them with each other and with tests/crank_cases.py.
//   usage: host_mirror_collection_test <topk> then per source, oldest first:  <index file> <terms file (u32 triples)> <docsCnt> <updates>
//          (<updates>: the source re-indexes documents 1 .. updates of the older sources)
//   output per query and path:  <name> <dev|host> <count> then " <doc>:<score bits, u64 decimal>", best first
#include "../../trinity_amd/csrc/host/trinity_gpu.hpp"
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <numeric>

using namespace trinity_amd;

static std::vector<char> slurp(const char *path) {
        std::ifstream f(path, std::ios::binary);
        return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char **argv) {
        if (argc < 6 || (argc - 2) % 4)
                return 2;
        const uint32_t topk = uint32_t(strtoul(argv[1], nullptr, 10));
        const size_t nsrc = size_t(argc - 2) / 4;
        try {
                std::vector<std::vector<char>> bytes(nsrc);
                std::vector<std::unique_ptr<IndexSource>> srcs;
                IndexSourcesCollection collection;
                size_t nterms = 0;
                for (size_t s = 0; s < nsrc; ++s) {
                        char **a = argv + 2 + 4 * s;
                        bytes[s] = slurp(a[0]);
                        const std::vector<char> tb = slurp(a[1]);
                        nterms = tb.size() / 12;
                        std::vector<term_index_ctx> tctx(nterms);
                        memcpy(tctx.data(), tb.data(), nterms * 12);
                        std::vector<std::string> names(nterms);
                        field_statistics fs;
                        for (size_t i = 0; i < nterms; ++i) {
                                names[i] = "t" + std::to_string(i);
                                fs.sumTermsDocs += tctx[i].documents;
                                fs.totalTerms += tctx[i].documents != 0;
                        }
                        fs.docsCnt = uint32_t(strtoul(a[2], nullptr, 10));
                        srcs.push_back(std::make_unique<IndexSource>(0, reinterpret_cast<const uint8_t *>(bytes[s].data()), bytes[s].size(), names, tctx, fs));
                        updated_documents ud;
                        ud.ids.resize(strtoul(a[3], nullptr, 10));
                        std::iota(ud.ids.begin(), ud.ids.end(), docid_t(1));
                        collection.insert(srcs.back().get(), std::move(ud));
                }
                struct Q {
                        const char *name;
                        std::function<DocsSetIterators::Iterator *(IndexSource &)> make;
                };
                auto t = [](IndexSource &src, int i) { return src.term("t" + std::to_string(i)); };
                const int V = int(nterms);
                const std::vector<Q> qs = {
                    {"and2", [&](IndexSource &s) { return s.conjunction({t(s, 0), t(s, 1)}); }},
                    {"or3", [&](IndexSource &s) { return s.disjunction({t(s, 0), t(s, 1), t(s, 2)}); }},
                    {"phrases", [&](IndexSource &s) { return s.disjunction({s.phrase({"t0", "t1"}), s.phrase({"t1", "t2"}), s.phrase({"t2", "t3"})}); }},
                    {"opt", [&](IndexSource &s) { return s.optional(t(s, 0), s.phrase({"t1", "t2"})); }},
                    {"and3", [&](IndexSource &s) { return s.conjunction({t(s, 3), t(s, 1), t(s, 0)}); }},
                    {"none", [&](IndexSource &s) { return s.conjunction({t(s, 0), t(s, V - 1), t(s, V - 2), t(s, V - 3)}); }},
                };
                const std::vector<double> weights = {1.0, 2.0, 3.0, 1.0, 2.0, 3.0}; // (1 + k % 3)
                for (const Q &q : qs)
                        for (const bool device : {true, false}) {
                                std::vector<DocsSetIterators::Iterator *> roots;
                                for (auto &s : srcs)
                                        roots.push_back(q.make(*s));
                                auto parts = exec_query<ProximityRanker>(roots, &collection, nullptr, 0, topk, 3u, 4.0, weights);
                                // (exec_query constructs the rankers: the path is chosen per ranker, so the replay runs the sources again)
                                if (!device) {
                                        for (size_t s = 0; s < nsrc; ++s) {
                                                parts[s] = std::make_unique<ProximityRanker>(topk, 3u, 4.0, weights);
                                                parts[s]->device = false;
                                                const auto scanner = collection.scanner_registry_for(s);
                                                exec_query(q.make(*srcs[s]), srcs[s].get(), scanner.get(), parts[s].get());
                                        }
                                }
                                const auto list = ProximityRanker::blend(parts, topk);
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

// host_mirror_filter_test.cpp — exec_query with an IndexDocumentsFilter the DEVICE applies (trinity_gpu.hpp: DeviceDocumentsFilter, installed through
// tri_batch_set_filters) next to the equivalent plain host filter (asked per replayed document), DocumentsOnly and AccumulatedScoreScheme + BM25; then both
// through exec_queries.  Prints each result list for the Python test (tests/test_host_mirror_filter.py) to compare.
//   usage: host_mirror_filter_test <index file> <terms file (u32 triples)> <docsCnt>
#include "../../trinity_amd/csrc/host/trinity_gpu.hpp"
#include <cinttypes>
#include <cstdio>
#include <fstream>

using namespace trinity_amd;

struct Collect final : public MatchedIndexDocumentsFilter {
        std::vector<docid_t> ids;
        std::vector<double> scores;
        void consider(const docid_t id) override { ids.push_back(id); }
        void consider(const docid_t id, const double s) override {
                ids.push_back(id);
                scores.push_back(s);
        }
        void consider(const docid_t *p, const std::size_t n) override { ids.insert(ids.end(), p, p + n); }
};

// the rule, as a plain host filter: disregard every third document and everything past 15000
static bool rule(const docid_t id) { return id % 3 == 0 || id > 15000; }
struct HostRule final : public IndexDocumentsFilter {
        size_t asked{0};
        bool filter(const docid_t id) override {
                ++asked;
                return rule(id);
        }
};

static void show(const char *name, const Collect &c) {
        printf("%s", name);
        for (size_t i = 0; i < c.ids.size(); ++i)
                if (c.scores.empty())
                        printf(" %u", c.ids[i]);
                else
                        printf(" %u:%.17g", c.ids[i], c.scores[i]);
        printf("\n");
}

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
                Similarity::IndexSourcesCollectionBM25Scorer bm25;
                std::unique_ptr<Similarity::IndexSourceTermsScorer> scorer(bm25.new_source_scorer(&src));
                {
                        DeviceDocumentsFilter onDevice(&src, rule); // the predicate, evaluated once over 1 .. docsCnt
                        std::vector<docid_t> kept;
                        for (docid_t d = 1; d <= fs.docsCnt; ++d)
                                if (!rule(d))
                                        kept.push_back(d);
                        DeviceDocumentsFilter allowList(&src, kept, true); // the same rule as the documents a query may match
                        HostRule onHost;
                        printf("device_filter handle=%d plain=%d\n", onDevice.device_filter() != nullptr, onHost.device_filter() != nullptr);
                        auto query = [&]() { return src.conjunction({src.term("t0"), src.disjunction({src.term("t1"), src.term("t2"), src.term("t3")})}); };
                        for (const uint32_t flags : {unsigned(ExecFlags::DocumentsOnly), unsigned(ExecFlags::AccumulatedScoreScheme)}) {
                                const char *mode = flags == unsigned(ExecFlags::DocumentsOnly) ? "docs" : "scored";
                                Collect d, k, h;
                                exec_query(query(), &src, &d, &onDevice, flags, scorer.get());
                                exec_query(query(), &src, &k, &allowList, flags, scorer.get());
                                const size_t before = onHost.asked;
                                exec_query(query(), &src, &h, &onHost, flags, scorer.get());
                                show((std::string(mode) + "_device").c_str(), d);
                                show((std::string(mode) + "_allow").c_str(), k);
                                show((std::string(mode) + "_host").c_str(), h);
                                printf("%s_asked host=%zu\n", mode, onHost.asked - before);
                        }
                        { // the default mode: the matches' ids
                                struct Ids final : public MatchedIndexDocumentsFilter {
                                        Collect c;
                                        void consider(const matched_document &m) override { c.ids.push_back(m.id); }
                                } d, h;
                                exec_query(query(), &src, &d, &onDevice);
                                exec_query(query(), &src, &h, &onHost);
                                show("rich_device", d.c);
                                show("rich_host", h.c);
                        }
                        { // one engine batch, a filter per query: the second query unfiltered
                                Collect a, b, c;
                                exec_queries({query(), query(), src.disjunction({src.term("t8"), src.term("t9")})}, &src, {&a, &b, &c}, unsigned(ExecFlags::DocumentsOnly), nullptr,
                                             {&onDevice, nullptr, &allowList});
                                show("batch_filtered", a);
                                show("batch_plain", b);
                                show("batch_other", c);
                        }
                        try {
                                Collect a;
                                exec_queries({query()}, &src, {&a}, unsigned(ExecFlags::DocumentsOnly), nullptr, {&onHost});
                                printf("host_filter_in_batch no-throw\n");
                        } catch (const invalid_argument &) {
                                printf("host_filter_in_batch invalid_argument\n");
                        }
                }
        } catch (const std::exception &e) {
                printf("EXCEPTION %s\n", e.what());
                return 1;
        }
        return 0;
}

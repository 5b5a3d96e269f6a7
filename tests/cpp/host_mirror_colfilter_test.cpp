// host_mirror_colfilter_test.cpp — exec_query with a ColumnPredicateFilter (trinity_gpu.hpp: an IndexDocumentsFilter over DeviceColumns, built on the device through
// tri_filters_from_columns) applied by the DEVICE and through the REPLAY (the same filter asked per replayed document, answered by column_pred.hpp from the
// columns' host copies), next to a plain host filter of the same rule; DocumentsOnly, AccumulatedScoreScheme + BM25 and the default mode; then through
// exec_queries, and with an `also` filter.  Prints each result list for the Python test (tests/test_host_mirror_colfilter.py) to compare.
//   usage: host_mirror_colfilter_test <index file> <terms file (u32 triples)> <docsCnt>
#include "../../trinity_amd/csrc/host/trinity_gpu.hpp"
#include <cinttypes>
#include <cstdio>
#include <fstream>

using namespace trinity_amd;
using PF = ColumnPredicateFilter;

struct Collect final : public MatchedIndexDocumentsFilter {
        std::vector<docid_t> ids;
        std::vector<double> scores;
        void consider(const docid_t id) override { ids.push_back(id); }
        void consider(const docid_t id, const double s) override {
                ids.push_back(id);
                scores.push_back(s);
        }
        void consider(const docid_t *p, const std::size_t n) override { ids.insert(ids.end(), p, p + n); }
        void consider(const matched_document &m) override { ids.push_back(m.id); }
};

// the rule, as a plain host filter: disregard a document whose price (id * 7 % 1000) lies outside 100 .. 600, or whose category (id % 11) is none of 3, 5, 8
static uint32_t price(const docid_t id) { return id * 7u % 1000u; }
static uint32_t category(const docid_t id) { return id % 11u; }
static bool rule(const docid_t id) { return price(id) < 100 || price(id) > 600 || !(category(id) == 3 || category(id) == 5 || category(id) == 8); }
struct HostRule final : public IndexDocumentsFilter {
        size_t asked{0};
        bool filter(const docid_t id) override {
                ++asked;
                return rule(id);
        }
};

static void show(const std::string &name, const Collect &c) {
        printf("%s", name.c_str());
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
                        DeviceColumn prices(&src, price), categories(&src, category);
                        // the allow-list form: price in 100 .. 600 AND category among {3, 5, 8} ...
                        const std::vector<PF::Clause> keepRule = {PF::Clause::range(&prices, 100, 600), PF::Clause::among(&categories, {8, 3, 5, 3})};
                        // ... and the drop form of the same rule: price outside 100 .. 600 OR category among the rest
                        const std::vector<PF::Clause> dropRule = {PF::Clause::range(&prices, 100, 600, true), PF::Clause::among(&categories, {0, 1, 2, 4, 6, 7, 9, 10})};
                        PF onDevice(&src, keepRule), dropForm(&src, dropRule, true, false), replayed(&src, keepRule, false, true, nullptr, false);
                        HostRule onHost;
                        printf("device_filter device=%d drop=%d replay=%d plain=%d\n", onDevice.device_filter() != nullptr, dropForm.device_filter() != nullptr, replayed.device_filter() != nullptr,
                               onHost.device_filter() != nullptr);
                        { // the device's bitmap, filter(id) and the rule agree on every document
                                const std::vector<uint32_t> words = onDevice.bitmap(), dwords = dropForm.bitmap();
                                size_t differ = 0, dropped = 0;
                                for (docid_t d = 1; d <= fs.docsCnt; ++d) {
                                        const bool bit = (words[d >> 5] >> (d & 31)) & 1, dbit = (dwords[d >> 5] >> (d & 31)) & 1;
                                        differ += bit != rule(d) || dbit != rule(d) || onDevice.filter(d) != rule(d) || dropForm.filter(d) != rule(d);
                                        dropped += bit;
                                }
                                printf("bitmap words=%zu differ=%zu dropped=%zu\n", words.size(), differ, dropped);
                        }
                        auto query = [&]() { return src.conjunction({src.term("t0"), src.disjunction({src.term("t1"), src.term("t2"), src.term("t3")})}); };
                        for (const uint32_t flags : {unsigned(ExecFlags::DocumentsOnly), unsigned(ExecFlags::AccumulatedScoreScheme)}) {
                                const std::string mode = flags == unsigned(ExecFlags::DocumentsOnly) ? "docs" : "scored";
                                Collect d, k, r, h;
                                exec_query(query(), &src, &d, &onDevice, flags, scorer.get());
                                exec_query(query(), &src, &k, &dropForm, flags, scorer.get());
                                exec_query(query(), &src, &r, &replayed, flags, scorer.get());
                                const size_t before = onHost.asked;
                                exec_query(query(), &src, &h, &onHost, flags, scorer.get());
                                show(mode + "_device", d);
                                show(mode + "_dropform", k);
                                show(mode + "_replay", r);
                                show(mode + "_host", h);
                                printf("%s_asked host=%zu\n", mode.c_str(), onHost.asked - before);
                        }
                        { // the default mode: the matches' ids
                                Collect d, r, h;
                                exec_query(query(), &src, &d, &onDevice);
                                exec_query(query(), &src, &r, &replayed);
                                exec_query(query(), &src, &h, &onHost);
                                show("rich_device", d);
                                show("rich_replay", r);
                                show("rich_host", h);
                        }
                        { // one engine batch, a filter per query: the second query unfiltered
                                Collect a, b, c;
                                exec_queries({query(), query(), src.disjunction({src.term("t8"), src.term("t9")})}, &src, {&a, &b, &c}, unsigned(ExecFlags::DocumentsOnly), nullptr,
                                             {&onDevice, nullptr, &dropForm});
                                show("batch_filtered", a);
                                show("batch_plain", b);
                                show("batch_other", c);
                        }
                        { // `also`: a docID-list filter that disregards the odd documents, folded into the column filter's bitmap; the column gone before filter() is asked again and before the query runs
                                DeviceDocumentsFilter odd(&src, [](const docid_t id) { return id % 2 == 1; });
                                std::unique_ptr<DeviceColumn> p2(new DeviceColumn(&src, price));
                                PF both(&src, {PF::Clause::range(p2.get(), 100, 600)}, false, true, &odd);
                                size_t differ = 0;
                                for (docid_t d = 1; d <= fs.docsCnt; ++d)
                                        differ += both.filter(d) != (d % 2 == 1 || price(d) < 100 || price(d) > 600);
                                p2.reset();
                                for (docid_t d = 1; d <= fs.docsCnt; ++d) // (the filter keeps its own copy of the column's host values)
                                        differ += both.filter(d) != (d % 2 == 1 || price(d) < 100 || price(d) > 600);
                                Collect a;
                                exec_query(query(), &src, &a, &both, unsigned(ExecFlags::DocumentsOnly), scorer.get());
                                printf("also_differ %zu\n", differ);
                                show("also_device", a);
                        }
                        try {
                                DeviceColumn huge(&src, [](const docid_t) { return 1u; });
                                PF bad(&src, {PF::Clause::among(&huge, {TRI_FACET_MAX_BUCKETS})});
                                printf("set_value_65536 no-throw\n");
                        } catch (const std::exception &) {
                                printf("set_value_65536 refused\n");
                        }
                }
        } catch (const std::exception &e) {
                printf("EXCEPTION %s\n", e.what());
                return 1;
        }
        return 0;
}

// host_mirror_wide_terms_test.cpp — exec_query's default mode (consider(const matched_document &)) on queries of more than 16 terms: the source's device is
// told rich_max_terms = 64 (trinity_gpu.hpp: IndexSource::set_option), and exec_query_default_mode reads the batch through the _wide result calls.  For each
// query the driver folds what consider() receives into the canonical stream the oracle's default mode writes — per match: doc, matched terms, then per matched
// term in ascending term order: term, freq, positions — and prints its FNV-1a hash for the Python test (tests/test_host_mirror_wide_terms.py) to compare.
//   usage: host_mirror_wide_terms_test <index file> <terms file (u32 triples)> <docsCnt>
#include "../../trinity_amd/csrc/host/trinity_gpu.hpp"
#include <cinttypes>
#include <cstdio>
#include <fstream>

using namespace trinity_amd;

struct Fold final : public MatchedIndexDocumentsFilter {
        uint64_t h{1469598103934665603ull};
        size_t matches{0}, terms{0}, hits{0};
        uint16_t widest{0};
        void u32(uint32_t v) {
                for (int b = 0; b < 4; ++b) {
                        h = (h ^ (v & 0xff)) * 1099511628211ull;
                        v >>= 8;
                }
        }
        void consider(const matched_document &m) override {
                std::vector<std::pair<uint32_t, const term_hits *>> byTerm;
                for (uint16_t k = 0; k < m.matchedTermsCnt; ++k) // tokens are "t<row>"
                        byTerm.emplace_back(uint32_t(strtoul(m.matchedTerms[k].queryCtx->term.token.c_str() + 1, nullptr, 10)), m.matchedTerms[k].hits);
                std::sort(byTerm.begin(), byTerm.end());
                u32(m.id);
                u32(uint32_t(byTerm.size()));
                for (const auto &t : byTerm) {
                        u32(t.first);
                        u32(t.second->freq);
                        for (uint32_t i = 0; i < t.second->freq; ++i)
                                u32(t.second->all[i].pos);
                        hits += t.second->freq;
                }
                ++matches;
                terms += byTerm.size();
                widest = std::max(widest, m.matchedTermsCnt);
        }
};

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
                auto terms = [&](int lo, int hi) {
                        std::vector<DocsSetIterators::Iterator *> its;
                        for (int i = lo; i < hi; ++i)
                                its.push_back(src.term("t" + std::to_string(i)));
                        return its;
                };
                auto or33 = [&]() { return src.disjunction(terms(0, 33)); };
                auto straddle = [&]() { // t40 OR ... OR t70 OR "t0 t1" OR "t1 t2" OR t80 OR ... OR t99
                        auto its = terms(40, 71);
                        its.push_back(src.phrase({"t0", "t1"}));
                        its.push_back(src.phrase({"t1", "t2"}));
                        for (auto it : terms(80, 100))
                                its.push_back(it);
                        return src.disjunction(its);
                };
                { // at the default the query is left out of the batch: the call reports it the way it always did
                        Fold f;
                        try {
                                exec_query(or33(), &src, &f);
                                printf("default matches=%zu\n", f.matches);
                        } catch (const std::exception &e) {
                                printf("default exception\n");
                        }
                }
                src.set_option("rich_max_terms", 64);
                {
                        Fold f;
                        exec_query(or33(), &src, &f);
                        printf("or33 %" PRIu64 " matches=%zu terms=%zu hits=%zu widest=%u\n", f.h, f.matches, f.terms, f.hits, unsigned(f.widest));
                }
                {
                        Fold f;
                        exec_query(straddle(), &src, &f);
                        printf("straddle %" PRIu64 " matches=%zu terms=%zu hits=%zu widest=%u\n", f.h, f.matches, f.terms, f.hits, unsigned(f.widest));
                }
                { // a query of at most 16 terms through the same calls
                        Fold f;
                        exec_query(src.disjunction(terms(0, 3)), &src, &f);
                        printf("or3 %" PRIu64 " matches=%zu terms=%zu hits=%zu widest=%u\n", f.h, f.matches, f.terms, f.hits, unsigned(f.widest));
                }
        } catch (const std::exception &e) {
                printf("EXCEPTION %s\n", e.what());
                return 1;
        }
        return 0;
}

// host_mirror_hits_test.cpp — Codecs::PostingsListIterator::materialize_hits, DocWordsSpace and IndexSource::term_hits_at of the C++ operator surface
// (trinity_gpu.hpp) driven the way an application's own CPU iterator drives the reference's: next() / advance() over postings lists, materialize_hits on
// every document it stops on.  Prints what it saw for the Python test (tests/test_host_mirror_hits.py) to compare with the oracle's walk.
//   usage: host_mirror_hits_test <index file> <terms file (u32 triples)> <docsCnt> <term a> <term b> [<hits.data file>: the segment is LUCENE]
#include "../../trinity_amd/csrc/host/trinity_gpu.hpp"
#include <cinttypes>
#include <cstdio>
#include <fstream>

using namespace trinity_amd;

static std::vector<uint8_t> slurp(const char *path) {
        std::ifstream f(path, std::ios::binary);
        return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
static void show_hits(const term_hit *h, const uint32_t n) {
        for (uint32_t k = 0; k < n; ++k)
                printf(" %u:%u:%" PRIu64, h[k].pos, h[k].payloadLen, h[k].payload);
}

int main(int argc, char **argv) {
        if (argc < 6)
                return 2;
        const std::vector<uint8_t> index = slurp(argv[1]), tb = slurp(argv[2]), hits = argc > 6 ? slurp(argv[6]) : std::vector<uint8_t>();
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
        const std::string ta = std::string("t") + argv[4], tbn = std::string("t") + argv[5];
        try {
                IndexSource src(0, index.data(), index.size(), names, tctx, fs, argc > 6 ? "LUCENE" : "GOOGLE", hits.data(), hits.size());
                DocWordsSpace dws;
                std::vector<term_hit> ha(65536), hb(65536);
                { // term a, next() to exhaustion: every document's hits, and whether the space holds the term at each of them
                        auto it = src.term(ta);
                        it->decoder()->execCtxTermID = 1;
                        for (auto d = it->next(); d != DocIDsEND; d = it->next()) {
                                dws.reset();
                                it->materialize_hits(&dws, ha.data());
                                printf("next %u %u", d, it->freq);
                                show_hits(ha.data(), it->freq);
                                printf(" |");
                                for (uint32_t k = 0; k < it->freq; ++k)
                                        printf(" %d%d", dws.test(1, ha[k].pos), dws.test(2, ha[k].pos));
                                printf("\n");
                        }
                }
                std::vector<std::pair<uint32_t, isrc_docid_t>> pairs;
                { // a AND b by hand, leap-frogging with advance(): on a common document both terms' hits go into ONE space (a first, then b: b owns a shared position)
                        auto a = src.term(ta), b = src.term(tbn);
                        a->decoder()->execCtxTermID = 1;
                        b->decoder()->execCtxTermID = 2;
                        auto d = a->next();
                        while (d != DocIDsEND) {
                                const auto e = b->advance(d);
                                if (e == DocIDsEND)
                                        break;
                                if (e != d) {
                                        d = a->advance(e);
                                        continue;
                                }
                                dws.reset();
                                a->materialize_hits(&dws, ha.data());
                                b->materialize_hits(&dws, hb.data());
                                printf("both %u a", d);
                                show_hits(ha.data(), a->freq);
                                printf(" b");
                                show_hits(hb.data(), b->freq);
                                printf(" |");
                                for (uint32_t k = 0; k < a->freq; ++k)
                                        printf(" %d", dws.test(1, ha[k].pos) ? 1 : dws.test(2, ha[k].pos) ? 2 : 0);
                                for (uint32_t k = 0; k < b->freq; ++k)
                                        printf(" %d", dws.test(1, hb[k].pos) ? 1 : dws.test(2, hb[k].pos) ? 2 : 0);
                                printf("\n");
                                pairs.emplace_back(src.term_id(ta), d);
                                pairs.emplace_back(src.term_id(tbn), d);
                                d = a->next();
                        }
                }
                // the same documents through term_hits_at, and two the lists do not hold
                pairs.emplace_back(src.term_id(ta), 0u);
                pairs.emplace_back(src.term_id(tbn), DocIDsEND);
                const auto r = src.term_hits_at(pairs);
                for (size_t i = 0; i < pairs.size(); ++i) {
                        printf("at %u %u %u", pairs[i].first, pairs[i].second, r.freqs[i]);
                        show_hits(r.hits.data() + r.offsets[i], uint32_t(r.offsets[i + 1] - r.offsets[i]));
                        printf("\n");
                }
        } catch (const std::exception &e) {
                printf("EXCEPTION %s\n", e.what());
                return 1;
        }
        return 0;
}

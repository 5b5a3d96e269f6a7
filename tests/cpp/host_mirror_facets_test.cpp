// host_mirror_facets_test.cpp — FacetCounter (trinity_gpu.hpp): the matches of a query counted by per-document columns, on the DEVICE (exec_query sets the facets on its
// batch and reads tri_batch_facets) and through the REPLAY (consider(ids, cnt) on the host), over single sources — also under a device filter and under a host filter — and
// over an IndexSourcesCollection (one counter per source, summed).  Prints every row for the Python test (tests/test_host_mirror_facets.py) to compare.
//   usage: host_mirror_facets_test { <index file> <terms file (u32 triples)> <docsCnt> <updates: this source re-indexes documents 1 .. updates of the older ones> }+
//   output: "single <source> <query> <device|replay> <facet> counters ...", "filtered <ondevice|onhost> <device|replay> <facet> counters ..." (source 0, query 0),
//           "collection <query> <device|replay> <facet> sums ..."
#include "../../trinity_amd/csrc/host/trinity_gpu.hpp"
#include <cinttypes>
#include <cstdio>
#include <fstream>

using namespace trinity_amd;

// the columns, as tests/facet_cases.py::columns writes them
static uint32_t mod7(const docid_t d) { return d % 7; }
static uint32_t huge(const docid_t d) { return d % 3 == 0 ? 0xffffffffu : d % 5; }
static uint32_t low16(const docid_t d) { return d & 0xffffu; }
static bool rule(const docid_t id) { return id % 4 == 1; } // the documents a filter disregards
struct HostRule final : public IndexDocumentsFilter {
        bool filter(const docid_t id) override { return rule(id); }
};

static std::vector<char> slurp(const char *path) {
        std::ifstream f(path, std::ios::binary);
        return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

template <class Row>
static void show(const std::string &head, const size_t k, const Row &row) {
        printf("%s %zu", head.c_str(), k);
        for (const auto v : row)
                printf(" %" PRIu64, uint64_t(v));
        printf("\n");
}

int main(int argc, char **argv) {
        if (argc < 5 || (argc - 1) % 4)
                return 2;
        const size_t nsrc = size_t(argc - 1) / 4;
        try {
                std::vector<std::vector<char>> bytes(nsrc);
                std::vector<std::unique_ptr<IndexSource>> srcs;
                IndexSourcesCollection collection;
                for (size_t s = 0; s < nsrc; ++s) {
                        char **a = argv + 1 + 4 * s;
                        bytes[s] = slurp(a[0]);
                        const std::vector<char> tb = slurp(a[1]);
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
                        fs.docsCnt = uint32_t(strtoul(a[2], nullptr, 10));
                        srcs.push_back(std::make_unique<IndexSource>(0, reinterpret_cast<const uint8_t *>(bytes[s].data()), bytes[s].size(), names, tctx, fs));
                        updated_documents ud;
                        for (docid_t d = 1; d <= strtoul(a[3], nullptr, 10); ++d)
                                ud.ids.push_back(d);
                        collection.insert(srcs.back().get(), std::move(ud));
                }
                // three columns per source; the facets name all of a column's copies, exec_query picks the source's
                std::vector<std::unique_ptr<DeviceColumn>> c7, ch, cl;
                std::vector<const DeviceColumn *> p7, ph, pl;
                for (auto &s : srcs) {
                        c7.push_back(std::make_unique<DeviceColumn>(s.get(), mod7));
                        ch.push_back(std::make_unique<DeviceColumn>(s.get(), huge));
                        cl.push_back(std::make_unique<DeviceColumn>(s.get(), low16));
                        p7.push_back(c7.back().get());
                        ph.push_back(ch.back().get());
                        pl.push_back(cl.back().get());
                }
                const std::vector<FacetCounter::Facet> facets = {{p7, 7}, {p7, 5}, {ph, 5}, {pl, 4096}};
                const auto query = [](IndexSource *s, const int q) -> DocsSetIterators::Iterator * {
                        switch (q) {
                        case 0:
                                return s->conjunction({s->term("t0"), s->term("t1")});
                        case 1:
                                return s->disjunction({s->term("t0"), s->term("t1"), s->term("t2")});
                        default:
                                return s->conjunction({s->term("t3"), s->disjunction({s->term("t4"), s->term("t5")})});
                        }
                };
                const uint32_t docs = unsigned(ExecFlags::DocumentsOnly);
                for (size_t s = 0; s < nsrc; ++s)
                        for (int q = 0; q < 3; ++q)
                                for (const bool device : {true, false}) {
                                        FacetCounter fc(facets, device);
                                        exec_query(query(srcs[s].get(), q), srcs[s].get(), &fc, nullptr, docs);
                                        for (size_t k = 0; k < facets.size(); ++k)
                                                show("single " + std::to_string(s) + " " + std::to_string(q) + (device ? " device" : " replay"), k, fc.rows[k]);
                                }
                { // a filter the device applies: counted on the device; a host filter: the counter is asked per replayed document whatever it prefers
                        DeviceDocumentsFilter onDevice(srcs[0].get(), rule);
                        HostRule onHost;
                        for (const bool device : {true, false}) {
                                FacetCounter a(facets, device), b(facets, device);
                                exec_query(query(srcs[0].get(), 0), srcs[0].get(), &a, &onDevice, docs);
                                exec_query(query(srcs[0].get(), 0), srcs[0].get(), &b, &onHost, docs);
                                for (size_t k = 0; k < facets.size(); ++k) {
                                        show(std::string("filtered ondevice") + (device ? " device" : " replay"), k, a.rows[k]);
                                        show(std::string("filtered onhost") + (device ? " device" : " replay"), k, b.rows[k]);
                                }
                        }
                }
                for (int q = 0; q < 3; ++q)
                        for (const bool device : {true, false}) {
                                std::vector<DocsSetIterators::Iterator *> roots;
                                for (auto &s : srcs)
                                        roots.push_back(query(s.get(), q));
                                const auto parts = exec_query<FacetCounter>(roots, &collection, nullptr, docs, facets, device);
                                for (size_t k = 0; k < facets.size(); ++k)
                                        show("collection " + std::to_string(q) + (device ? " device" : " replay"), k, FacetCounter::sum(parts, k));
                        }
                try {
                        FacetCounter unbound(facets);
                        const docid_t id = 1;
                        unbound.consider(&id, 1);
                        printf("unbound no-throw\n");
                } catch (const invalid_argument &) {
                        printf("unbound invalid_argument\n");
                }
        } catch (const std::exception &e) {
                printf("EXCEPTION %s\n", e.what());
                return 1;
        }
        return 0;
}

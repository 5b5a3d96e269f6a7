// host_mirror_stats_test.cpp — StatsCounter (trinity_gpu.hpp): the matches of a query aggregated per bucket — count, sum, min, max of a value column —, on the DEVICE
// (exec_query sets the stats on its batch and reads tri_batch_stats) and through the REPLAY (consider(ids, cnt) on the host), over single sources — also under a device
// filter and under a host filter — and over an IndexSourcesCollection (one counter per source, combined).  Prints every row for the Python test
// (tests/test_host_mirror_stats.py) to compare.
//   usage: host_mirror_stats_test { <index file> <terms file (u32 triples)> <docsCnt> <updates: this source re-indexes documents 1 .. updates of the older ones> }+
//   output: "single <source> <query> <device|replay> <stat> <plane> values ...", "filtered <ondevice|onhost> <device|replay> <stat> <plane> values ..." (source 0,
//           query 0), "collection <query> <device|replay> <stat> <plane> values ..." — plane: sums, counts, mins, maxs
#include "../../trinity_amd/csrc/host/trinity_gpu.hpp"
#include <cinttypes>
#include <cstdio>
#include <fstream>

using namespace trinity_amd;

// the columns, as tests/stats_cases.py::columns writes them
static uint32_t mod7(const docid_t d) { return d % 7; }
static uint32_t huge(const docid_t d) { return d % 3 == 0 ? 0xffffffffu : d % 5; }
static uint32_t low16(const docid_t d) { return d & 0xffffu; }
static uint32_t hash(const docid_t d) { return uint32_t(uint64_t(d) * 2654435761ull); }
static bool rule(const docid_t id) { return id % 4 == 1; } // the documents a filter disregards
struct HostRule final : public IndexDocumentsFilter {
        bool filter(const docid_t id) override { return rule(id); }
};

static std::vector<char> slurp(const char *path) {
        std::ifstream f(path, std::ios::binary);
        return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static void show(const std::string &head, const size_t k, const std::vector<stats_rows::Record> &row) {
        const char *planes[4] = {"sums", "counts", "mins", "maxs"};
        for (int p = 0; p < 4; ++p) {
                printf("%s %zu %s", head.c_str(), k, planes[p]);
                for (const auto &r : row)
                        printf(" %" PRIu64, p == 0 ? r.sum : p == 1 ? r.count : p == 2 ? uint64_t(r.min) : uint64_t(r.max));
                printf("\n");
        }
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
                // four columns per source; the stats name all of a column's copies, exec_query picks the source's
                std::vector<std::unique_ptr<DeviceColumn>> c7, ch, cl, cx;
                std::vector<const DeviceColumn *> p7, ph, pl, px;
                for (auto &s : srcs) {
                        c7.push_back(std::make_unique<DeviceColumn>(s.get(), mod7));
                        ch.push_back(std::make_unique<DeviceColumn>(s.get(), huge));
                        cl.push_back(std::make_unique<DeviceColumn>(s.get(), low16));
                        cx.push_back(std::make_unique<DeviceColumn>(s.get(), hash));
                        p7.push_back(c7.back().get());
                        ph.push_back(ch.back().get());
                        pl.push_back(cl.back().get());
                        px.push_back(cx.back().get());
                }
                const std::vector<StatsCounter::Stat> stats = {{{}, 0, px}, {p7, 5, px}, {ph, 5, pl}, {pl, 1000, ph}};
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
                                        StatsCounter sc(stats, device);
                                        exec_query(query(srcs[s].get(), q), srcs[s].get(), &sc, nullptr, docs);
                                        for (size_t k = 0; k < stats.size(); ++k)
                                                show("single " + std::to_string(s) + " " + std::to_string(q) + (device ? " device" : " replay"), k, sc.rows[k]);
                                }
                { // a filter the device applies: aggregated on the device; a host filter: the counter is asked per replayed document whatever it prefers
                        DeviceDocumentsFilter onDevice(srcs[0].get(), rule);
                        HostRule onHost;
                        for (const bool device : {true, false}) {
                                StatsCounter a(stats, device), b(stats, device);
                                exec_query(query(srcs[0].get(), 0), srcs[0].get(), &a, &onDevice, docs);
                                exec_query(query(srcs[0].get(), 0), srcs[0].get(), &b, &onHost, docs);
                                for (size_t k = 0; k < stats.size(); ++k) {
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
                                const auto parts = exec_query<StatsCounter>(roots, &collection, nullptr, docs, stats, device);
                                for (size_t k = 0; k < stats.size(); ++k)
                                        show("collection " + std::to_string(q) + (device ? " device" : " replay"), k, StatsCounter::combine(parts, k));
                        }
                try {
                        StatsCounter unbound(stats);
                        const docid_t id = 1;
                        unbound.consider(&id, 1);
                        printf("unbound no-throw\n");
                } catch (const invalid_argument &) {
                        printf("unbound invalid_argument\n");
                }
                try {
                        StatsCounter wrong({{{}, 3, px}});
                        printf("ungrouped-with-buckets no-throw\n");
                } catch (const invalid_argument &) {
                        printf("ungrouped-with-buckets invalid_argument\n");
                }
        } catch (const std::exception &e) {
                printf("EXCEPTION %s\n", e.what());
                return 1;
        }
        return 0;
}

// host_mirror_order_test.cpp — ColumnOrder (trinity_gpu.hpp): the first K matches of a query by a per-document column, on the DEVICE (exec_query sets the order on its
// batch and reads tri_batch_ordered) and through the REPLAY (consider(ids, cnt) on the host), over single sources — also under a device filter and under a host filter —
// and over an IndexSourcesCollection (one ColumnOrder per source, blended).  Prints every list for the Python test (tests/test_host_mirror_order.py) to compare.
//   usage: host_mirror_order_test { <index file> <terms file (u32 triples)> <docsCnt> <updates: this source re-indexes documents 1 .. updates of the older ones> }+
//   output: "single <source> <query> <column> <k> <up|down> <device|replay> docID value ...", "filtered <ondevice|onhost> <device|replay> docID value ..." (source 0,
//           query 0, hash, 10, up), "collection <query> <column> <k> <up|down> <device|replay> docID value ..."
#include "../../trinity_amd/csrc/host/trinity_gpu.hpp"
#include <cinttypes>
#include <cstdio>
#include <fstream>

using namespace trinity_amd;

// the columns, as tests/order_cases.py::columns writes them
static uint32_t mod7(const docid_t d) { return d % 7; }
static uint32_t hashed(const docid_t d) { return uint32_t(uint64_t(d) * 2654435761ull); }
static bool rule(const docid_t id) { return id % 4 == 1; } // the documents a filter disregards
struct HostRule final : public IndexDocumentsFilter {
        bool filter(const docid_t id) override { return rule(id); }
};

static std::vector<char> slurp(const char *path) {
        std::ifstream f(path, std::ios::binary);
        return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static void show(const std::string &head, const std::vector<std::pair<docid_t, uint32_t>> &list) {
        printf("%s", head.c_str());
        for (const auto &e : list)
                printf(" %" PRIu32 " %" PRIu32, uint32_t(e.first), e.second);
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
                // two columns per source; a ColumnOrder names all of a column's copies, exec_query picks the source's
                std::vector<std::unique_ptr<DeviceColumn>> c7, ch;
                std::vector<const DeviceColumn *> p7, ph;
                for (auto &s : srcs) {
                        c7.push_back(std::make_unique<DeviceColumn>(s.get(), mod7));
                        ch.push_back(std::make_unique<DeviceColumn>(s.get(), hashed));
                        p7.push_back(c7.back().get());
                        ph.push_back(ch.back().get());
                }
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
                const auto tag = [](const int col, const uint32_t k, const bool desc, const bool device) {
                        return std::string(col ? " hash " : " mod7 ") + std::to_string(k) + (desc ? " down" : " up") + (device ? " device" : " replay");
                };
                for (size_t s = 0; s < nsrc; ++s)
                        for (int q = 0; q < 3; ++q)
                                for (int col = 0; col < 2; ++col)
                                        for (const uint32_t k : {1u, 10u, 256u})
                                                for (const bool desc : {false, true})
                                                        for (const bool device : {true, false}) {
                                                                ColumnOrder co(col ? ph : p7, k, desc, device);
                                                                exec_query(query(srcs[s].get(), q), srcs[s].get(), &co, nullptr, docs);
                                                                show("single " + std::to_string(s) + " " + std::to_string(q) + tag(col, k, desc, device), co.list());
                                                        }
                { // a filter the device applies: selected on the device; a host filter: the order is asked per replayed document whatever it prefers
                        DeviceDocumentsFilter onDevice(srcs[0].get(), rule);
                        HostRule onHost;
                        for (const bool device : {true, false}) {
                                ColumnOrder a(ph, 10, false, device), b(ph, 10, false, device);
                                exec_query(query(srcs[0].get(), 0), srcs[0].get(), &a, &onDevice, docs);
                                exec_query(query(srcs[0].get(), 0), srcs[0].get(), &b, &onHost, docs);
                                show(std::string("filtered ondevice") + (device ? " device" : " replay"), a.list());
                                show(std::string("filtered onhost") + (device ? " device" : " replay"), b.list());
                        }
                }
                for (int q = 0; q < 3; ++q)
                        for (int col = 0; col < 2; ++col)
                                for (const uint32_t k : {10u, 256u})
                                        for (const bool desc : {false, true})
                                                for (const bool device : {true, false}) {
                                                        std::vector<DocsSetIterators::Iterator *> roots;
                                                        for (auto &s : srcs)
                                                                roots.push_back(query(s.get(), q));
                                                        const auto parts = exec_query<ColumnOrder>(roots, &collection, nullptr, docs, col ? ph : p7, k, desc, device);
                                                        show("collection " + std::to_string(q) + tag(col, k, desc, device), ColumnOrder::blend(parts));
                                                }
                try {
                        ColumnOrder unbound(ph, 10);
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

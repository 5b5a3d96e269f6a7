// host_mirror_isect_test.cpp — Trinity::intersect on the C++ operator surface (trinity_amd/csrc/host/trinity_gpu.hpp: intersect_impl / intersect over one source
// with a registry, intersect over an IndexSourcesCollection, intersection_indices, sort_intersections).  Prints every request's lists for
// tests/test_host_mirror_isect.py, which compares them with the restatement of tests/isect_cases.py.
//   usage: host_mirror_isect_test <requests file> then per source, oldest first: <index file> <terms file (u32 triples)> <names file> <docsCnt> <updates file (u32 docIDs)>
//   requests file, a request a line: <stopwordsMask> <groups> then per group <terms> <name> ...
//   output per request r: "single <r> <source> <n> mask:count ..." per source (run under the registry of the newer sources), "collection <r> <n> mask:count ...",
//   "indices <r> ..." (intersection_indices of the collection's first mask by sort_intersections)
#include "../../trinity_amd/csrc/host/trinity_gpu.hpp"
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <unordered_set>

using namespace trinity_amd;

static std::vector<char> slurp(const char *path) {
        std::ifstream f(path, std::ios::binary);
        return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static void print(const std::vector<std::pair<uint64_t, uint32_t>> &v) {
        printf(" %zu", v.size());
        for (const auto &e : v)
                printf(" %" PRIu64 ":%u", e.first, e.second);
        printf("\n");
}

int main(int argc, char **argv) {
        if (argc < 7 || (argc - 2) % 5)
                return 2;
        const size_t nsrc = size_t(argc - 2) / 5;
        try {
                std::vector<std::vector<char>> bytes(nsrc);
                std::vector<std::unique_ptr<IndexSource>> srcs;
                IndexSourcesCollection collection;
                for (size_t s = 0; s < nsrc; ++s) {
                        char **a = argv + 2 + 5 * s;
                        bytes[s] = slurp(a[0]);
                        const std::vector<char> tb = slurp(a[1]);
                        const size_t nterms = tb.size() / 12;
                        std::vector<term_index_ctx> tctx(nterms);
                        memcpy(tctx.data(), tb.data(), nterms * 12);
                        std::vector<std::string> names;
                        std::ifstream nf(a[2]);
                        for (std::string line; std::getline(nf, line);)
                                names.push_back(line);
                        field_statistics fs;
                        for (size_t i = 0; i < nterms; ++i) {
                                fs.sumTermsDocs += tctx[i].documents;
                                fs.totalTerms += tctx[i].documents != 0;
                        }
                        fs.docsCnt = uint32_t(strtoul(a[3], nullptr, 10));
                        srcs.push_back(std::make_unique<IndexSource>(0, reinterpret_cast<const uint8_t *>(bytes[s].data()), bytes[s].size(), names, tctx, fs));
                        const std::vector<char> ub = slurp(a[4]);
                        updated_documents ud;
                        ud.ids.resize(ub.size() / 4);
                        memcpy(ud.ids.data(), ub.data(), ud.ids.size() * 4);
                        collection.insert(srcs.back().get(), std::move(ud));
                }
                srcs[0]->set_masked_documents({1, 2, 3}); // (the call's registry replaces it and it is back afterwards)
                std::ifstream rf(argv[1]);
                size_t r = 0;
                for (std::string line; std::getline(rf, line); ++r) {
                        std::istringstream in(line);
                        uint64_t stop;
                        size_t ngroups;
                        in >> stop >> ngroups;
                        std::vector<std::unordered_set<std::string>> tokens(ngroups);
                        for (auto &set : tokens) {
                                size_t k;
                                in >> k;
                                for (size_t i = 0; i < k; ++i) {
                                        std::string name;
                                        in >> name;
                                        set.insert(name);
                                }
                        }
                        for (size_t s = 0; s < nsrc; ++s) {
                                const auto scanner = collection.scanner_registry_for(s);
                                const auto one = intersect(stop, tokens, srcs[s].get(), scanner.get());
                                std::vector<std::pair<uint64_t, uint32_t>> two;
                                intersect_impl(stop, tokens, srcs[s].get(), scanner.get(), &two);
                                if (one != two)
                                        return 3;
                                printf("single %zu %zu", r, s);
                                print(one);
                        }
                        auto all = intersect(stop, tokens, &collection);
                        printf("collection %zu", r);
                        print(all);
                        std::sort(all.begin(), all.end(), sort_intersections);
                        printf("indices %zu", r);
                        if (!all.empty()) {
                                uint8_t idx[64];
                                const uint8_t n = intersection_indices(all[0].first, idx);
                                for (uint8_t i = 0; i < n; ++i)
                                        printf(" %u", idx[i]);
                        }
                        printf("\n");
                }
                if (srcs[0]->masked_documents() != std::vector<docid_t>{1, 2, 3})
                        return 4;
                // refusals of the surface
                int refused = 0;
                try {
                        intersect(0, {}, srcs[0].get(), nullptr);
                } catch (const invalid_argument &) {
                        ++refused;
                }
                try {
                        intersect(0, std::vector<std::unordered_set<std::string>>(65), srcs[0].get(), nullptr);
                } catch (const invalid_argument &) {
                        ++refused;
                }
                printf("refused %d\n", refused);
        } catch (const std::exception &e) {
                fprintf(stderr, "exception: %s\n", e.what());
                return 1;
        }
        return 0;
}

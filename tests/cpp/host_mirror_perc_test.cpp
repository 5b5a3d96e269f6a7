// host_mirror_perc_test.cpp — an application written against the percolator of the operator surface (trinity_amd/csrc/host/trinity_gpu.hpp): the stored queries of a
// case file go into a PercolatorSet on the device, its documents are matched in one call, and every query's answer must be what percolator_query::match gives with a
// proxy over the same documents.  Prints the device's pairs in both orders ("q" / "d" lines) for tests/test_host_mirror_perc.py; exits 1 on a difference.
#include "perc_case_file.hpp"

#include <set>

int main(int argc, char **argv) {
        using namespace trinity_amd;
        if (argc != 2) {
                fprintf(stderr, "usage: host_mirror_perc_test CASES\n");
                return 2;
        }
        const perc_case::Case c = perc_case::read(argv[1]);
        tri_dev *dev = nullptr;
        check(tri_dev_open(0, &dev));
        int bad = 0;
        {
                PercolatorSet set(dev);
                for (const percolator_query &q : c.queries)
                        set.add(q);
                set.commit();
                const auto by_q = set.match(c.documents, TRI_PERC_BY_QUERY), by_d = set.match(c.documents, TRI_PERC_BY_DOCUMENT);
                std::set<std::pair<uint32_t, uint32_t>> device, host;
                for (const auto &p : by_q)
                        device.emplace(p.query, p.document);
                for (size_t q = 0; q < c.queries.size(); ++q)
                        for (size_t d = 0; d < c.documents.size(); ++d) {
                                percolator_positions_proxy proxy(c.queries[q], c.documents[d]);
                                if (c.queries[q].match(proxy))
                                        host.emplace(uint32_t(q), uint32_t(d));
                        }
                if (device != host || by_q.size() != host.size() || by_d.size() != host.size()) {
                        fprintf(stderr, "device %zu pairs (%zu distinct), host %zu\n", by_q.size(), device.size(), host.size());
                        bad = 1;
                }
                for (const auto &p : by_q)
                        printf("q %u %u\n", p.query, p.document);
                for (const auto &p : by_d)
                        printf("d %u %u\n", p.query, p.document);
                // unregister the first query: it vanishes; register it again: it is back
                if (!c.queries.empty()) {
                        set.set_enabled({0}, false);
                        size_t without = 0;
                        for (const auto &p : set.match(c.documents))
                                without += p.query == 0;
                        set.set_enabled({0}, true);
                        if (without || set.match(c.documents).size() != by_q.size()) {
                                fprintf(stderr, "set_enabled: %zu pairs of a disabled query\n", without);
                                bad = 1;
                        }
                }
                bool refused = false;
                try {
                        set.set_enabled({uint32_t(c.queries.size())}, false);
                } catch (const invalid_argument &) {
                        refused = true;
                }
                printf("refused %d\n", int(refused));
        }
        tri_dev_close(dev);
        return bad;
}

// perc_cpu_test.cpp — percolator_query::match (trinity_amd/csrc/host/trinity_gpu.hpp: the reference's recursion, percolator.cpp:5-137, over a postfix program) on
// the CPU, every stored query against every document of a case file; prints the matching pairs, query-major.  Stand-alone: tests/test_perc_cases.py compiles it with
// AddressSanitizer and UndefinedBehaviorSanitizer and compares the pairs with the restatement's.  Nothing of the engine is reached.
#include "perc_case_file.hpp"

int main(int argc, char **argv) {
        if (argc != 2) {
                fprintf(stderr, "usage: perc_cpu_test CASES\n");
                return 2;
        }
        const perc_case::Case c = perc_case::read(argv[1]);
        size_t pairs = 0;
        for (size_t q = 0; q < c.queries.size(); ++q) {
                const trinity_amd::percolator_query &pq = c.queries[q];
                if (bool(pq) != !pq.program().empty())
                        return 3;
                for (size_t d = 0; d < c.documents.size(); ++d) {
                        trinity_amd::percolator_positions_proxy proxy(pq, c.documents[d]);
                        if (pq.match(proxy)) {
                                printf("%zu %zu\n", q, d);
                                ++pairs;
                        }
                }
        }
        printf("pairs %zu\n", pairs);
        return 0;
}

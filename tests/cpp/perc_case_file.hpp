// perc_case_file.hpp — the case file tests/perc_cases.py writes for the two percolator drivers (perc_cpu_test.cpp, host_mirror_perc_test.cpp): whitespace-separated
// integers — nq, then per query { tokens, token... }; ndocs, then per document { terms, then per term { id, positions, position... } }.  Term id k is the string "t<k>".
#pragma once
#include "../../trinity_amd/csrc/host/trinity_gpu.hpp"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>

namespace perc_case {
        using namespace trinity_amd;
        struct Case {
                std::vector<percolator_query> queries;
                std::vector<percolator_document> documents;
        };
        inline uint64_t next(std::istream &in) {
                uint64_t v;
                if (!(in >> v)) {
                        fprintf(stderr, "perc_case: the file ends early\n");
                        exit(2);
                }
                return v;
        }
        inline Case read(const char *path) {
                std::ifstream in(path);
                Case c;
                const uint64_t nq = next(in);
                for (uint64_t q = 0; q < nq; ++q) {
                        const uint64_t n = next(in);
                        std::vector<uint32_t> prog;
                        std::vector<std::string> terms;
                        std::map<uint32_t, uint32_t> local; // the query's distinct terms, in order of first appearance (CCTX::resolve_query_term)
                        for (uint64_t i = 0; i < n; ++i) {
                                const uint32_t t = uint32_t(next(in));
                                if ((t >> 28) != TRI_OP_TERM) {
                                        prog.push_back(t);
                                        continue;
                                }
                                const auto it = local.emplace(t, uint32_t(local.size()));
                                if (it.second)
                                        terms.push_back("t" + std::to_string(t));
                                prog.push_back(TRI_TOK(TRI_OP_TERM, it.first->second));
                        }
                        c.queries.push_back(n ? percolator_query(std::move(prog), std::move(terms)) : percolator_query());
                }
                const uint64_t nd = next(in);
                for (uint64_t d = 0; d < nd; ++d) {
                        percolator_document doc;
                        const uint64_t nt = next(in);
                        for (uint64_t k = 0; k < nt; ++k) {
                                const uint64_t id = next(in), f = next(in);
                                std::vector<tokenpos_t> pos(f);
                                for (auto &p : pos)
                                        p = tokenpos_t(next(in));
                                doc.emplace_back("t" + std::to_string(id), std::move(pos));
                        }
                        c.documents.push_back(std::move(doc));
                }
                return c;
        }
} // namespace perc_case

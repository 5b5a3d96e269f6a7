// colpred_cpu_test.cpp — csrc/host/column_pred.hpp (the validation of tri_filters_from_columns and the host evaluation of a column predicate) against the numpy
// contract's cases (tests/colfilter_cases.py, written out by tests/test_colfilter_cases.py), and against every invalid shape the call refuses.  Stand-alone: no HIP, no
// engine; built with -fsanitize=address,undefined by the Python test.
//   usage: colpred_cpu_test <vectors file>
// The file is a stream of little-endian u32 words: [ncorpora] then per corpus [D][ncols] { [n][values ...] } [ncases] and per case
// [mode][any][nclauses] { [col][kind][negate][lo][hi][nset][set ...] } [has_also] { [nwords][also's drop words ...] } [nwords][expected drop words ...]
// (bit d & 31 of word d >> 5: document d).
#include "../../trinity_amd/csrc/host/column_pred.hpp"
#include <cinttypes>
#include <cstring>
#include <fstream>
#include <iterator>

// the handles, complete only here: a column knows its values and its index, a filter its index and what it drops
struct tri_column {
        const uint32_t *values;
        const void *ix;
};
struct tri_filter {
        const uint32_t *words;
        const void *ix;
};

static const void *ix_of_column(const tri_column *c) { return c->ix; }
static const void *ix_of_filter(const tri_filter *f) { return f->ix; }
static const uint32_t *values_of(const tri_column *c) { return c->values; }

static int refusals() {
        int bad = 0, n = 0;
        int here = 0, there = 0; // two indexes
        const uint32_t vals[4] = {0, 1, 2, 3};
        tri_column mine{vals, &here}, foreign{vals, &there}, more[TRI_PRED_MAX_COLUMNS + 1];
        for (auto &m : more)
                m = tri_column{vals, &here};
        tri_filter fmine{vals, &here}, fforeign{vals, &there};
        tri_filter *out[2] = {nullptr, nullptr};
        const uint32_t set_ok[2] = {1, TRI_FACET_MAX_BUCKETS - 1}, set_bad[2] = {1, TRI_FACET_MAX_BUCKETS};
        std::vector<const tri_column *> columns;
        std::string why;
        auto run = [&](const void *ix, const tri_predicate *p, size_t np, int mode, const void *o) { return colpred::validate(ix, p, np, mode, o, ix_of_column, ix_of_filter, columns, why); };
        auto refused = [&](const char *what, int rc, std::initializer_list<const char *> words) {
                ++n;
                bool ok = rc == TRI_ERR_INVALID && why.find("tri_filters_from_columns") != std::string::npos;
                for (const char *w : words)
                        ok = ok && why.find(w) != std::string::npos;
                if (!ok) {
                        ++bad;
                        printf("REFUSAL %s: rc %d, message '%s'\n", what, rc, why.c_str());
                }
                why.clear();
        };
        const tri_clause good{&mine, TRI_CLAUSE_RANGE, 0, 1, 2, nullptr, 0, 0};
        const tri_clause good_set{&mine, TRI_CLAUSE_SET, 1, 0, 0, set_ok, 2, 0};
        const tri_clause two[2] = {good, good_set};
        const tri_predicate ok{two, 2, 0, &fmine, 0};
        if (run(&here, &ok, 1, TRI_FILTER_KEEP, out) != TRI_OK || columns.size() != 1 || columns[0] != &mine) {
                ++bad;
                printf("a valid predicate is refused: %s\n", why.c_str());
        }
        refused("null index", run(nullptr, &ok, 1, 0, out), {"null argument"});
        refused("null predicates", run(&here, nullptr, 1, 0, out), {"null argument"});
        refused("null out", run(&here, &ok, 1, 0, nullptr), {"null argument"});
        refused("np 0", run(&here, &ok, 0, 0, out), {"0 predicates"});
        std::vector<tri_predicate> many(TRI_PREDS_MAX + 1, ok);
        refused("np above the limit", run(&here, many.data(), many.size(), 0, out), {"257 predicates"});
        if (run(&here, many.data(), TRI_PREDS_MAX, 0, out) != TRI_OK)
                ++bad, printf("TRI_PREDS_MAX predicates are refused: %s\n", why.c_str());
        refused("bad mode", run(&here, &ok, 1, 2, out), {"mode 2"});
        refused("bad mode", run(&here, &ok, 1, -1, out), {"mode -1"});
        tri_predicate p = ok;
        const tri_predicate pair_template[2] = {ok, ok};
        auto second = [&](const tri_predicate &q) { // the fault sits in predicate 1 of 2
                static tri_predicate pair[2];
                pair[0] = pair_template[0], pair[1] = q;
                return run(&here, pair, 2, TRI_FILTER_DROP, out);
        };
        p.nclauses = 0;
        refused("nclauses 0", second(p), {"predicate 1", "0 clauses"});
        p.nclauses = TRI_PRED_MAX_CLAUSES + 1;
        refused("nclauses 9", second(p), {"predicate 1", "9 clauses"});
        p = ok, p.clauses = nullptr;
        refused("null clauses", second(p), {"predicate 1", "null argument"});
        p = ok, p.reserved = 1;
        refused("predicate reserved", second(p), {"predicate 1", "reserved"});
        p = ok, p.also = &fforeign;
        refused("also of another index", second(p), {"predicate 1", "also", "another index"});
        tri_clause c2[2] = {good, good};
        p = ok, p.clauses = c2;
        c2[1].column = nullptr;
        refused("null column", second(p), {"predicate 1 clause 1", "null argument"});
        c2[1] = good, c2[1].column = &foreign;
        refused("column of another index", second(p), {"predicate 1 clause 1", "another index"});
        c2[1] = good, c2[1].kind = 2;
        refused("unknown kind", second(p), {"predicate 1 clause 1", "unknown kind 2"});
        c2[1] = good, c2[1].reserved = 7;
        refused("clause reserved", second(p), {"predicate 1 clause 1", "reserved"});
        c2[1] = good_set, c2[1].set = set_bad;
        refused("set value 65536", second(p), {"predicate 1 clause 1", "set value 65536"});
        c2[1] = good_set, c2[1].set = nullptr;
        refused("null set", second(p), {"predicate 1 clause 1", "null argument"});
        c2[1] = good_set, c2[1].set = nullptr, c2[1].nset = 0; // legal: the empty set
        if (second(p) != TRI_OK)
                ++bad, printf("an empty set is refused: %s\n", why.c_str());
        { // nine distinct columns across two predicates: eight in the first, the ninth in clause 0 of the second
                tri_clause a[TRI_PRED_MAX_COLUMNS], b[1];
                for (int i = 0; i < TRI_PRED_MAX_COLUMNS; ++i)
                        a[i] = good, a[i].column = &more[i];
                b[0] = good, b[0].column = &more[TRI_PRED_MAX_COLUMNS];
                tri_predicate pp[2] = {{a, TRI_PRED_MAX_COLUMNS, 0, nullptr, 0}, {b, 1, 1, nullptr, 0}};
                refused("nine distinct columns", run(&here, pp, 2, 0, out), {"predicate 1 clause 0", "distinct columns"});
                b[0].column = &more[3];
                if (run(&here, pp, 2, 0, out) != TRI_OK || columns.size() != TRI_PRED_MAX_COLUMNS)
                        ++bad, printf("eight distinct columns are refused: %s\n", why.c_str());
        }
        if (out[0] || out[1])
                ++bad, printf("out was written\n");
        printf("refusals %d bad %d\n", n, bad);
        return bad;
}

int main(int argc, char **argv) {
        if (argc < 2)
                return 2;
        std::ifstream f(argv[1], std::ios::binary);
        std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        std::vector<uint32_t> w(raw.size() / 4);
        memcpy(w.data(), raw.data(), w.size() * 4);
        size_t at = 0;
        auto next = [&]() {
                if (at >= w.size()) {
                        printf("vectors file ends early\n");
                        exit(2);
                }
                return w[at++];
        };
        size_t ncases = 0, bad = 0;
        int index = 0;
        const uint32_t ncorpora = next();
        for (uint32_t ci = 0; ci < ncorpora; ++ci) {
                const uint32_t D = next(), ncols = next();
                std::vector<std::vector<uint32_t>> vals(ncols);
                std::vector<tri_column> cols(ncols);
                for (uint32_t c = 0; c < ncols; ++c) {
                        const uint32_t n = next();
                        for (uint32_t i = 0; i < n; ++i)
                                vals[c].push_back(next());
                        cols[c] = tri_column{vals[c].data(), &index};
                }
                const uint32_t n = next();
                for (uint32_t k = 0; k < n; ++k, ++ncases) {
                        const int mode = int(next());
                        tri_predicate P{};
                        P.any = next();
                        P.nclauses = next();
                        std::vector<tri_clause> cl(P.nclauses);
                        std::vector<std::vector<uint32_t>> sets(P.nclauses);
                        for (auto &C : cl) {
                                C = tri_clause{};
                                C.column = &cols.at(next());
                                C.kind = next(), C.negate = next(), C.lo = next(), C.hi = next(), C.nset = next();
                                auto &s = sets[size_t(&C - cl.data())];
                                for (uint32_t i = 0; i < C.nset; ++i)
                                        s.push_back(next());
                                C.set = s.empty() ? nullptr : s.data();
                        }
                        P.clauses = cl.data();
                        std::vector<uint32_t> also, want;
                        tri_filter af{nullptr, &index};
                        if (next()) {
                                for (uint32_t i = next(); i; --i)
                                        also.push_back(next());
                                af.words = also.data();
                                P.also = &af;
                        }
                        for (uint32_t i = next(); i; --i)
                                want.push_back(next());
                        std::vector<const tri_column *> distinct;
                        std::string why;
                        tri_filter *out = nullptr;
                        if (colpred::validate(&index, &P, 1, mode, &out, ix_of_column, ix_of_filter, distinct, why) != TRI_OK) {
                                ++bad;
                                printf("corpus %u case %u refused: %s\n", ci, k, why.c_str());
                                continue;
                        }
                        size_t wrong = 0;
                        for (uint32_t d = 1; d <= D; ++d) {
                                const bool a = P.also && ((also[d >> 5] >> (d & 31)) & 1);
                                const bool got = colpred::drops(P, d, mode, a, values_of), exp = (want[d >> 5] >> (d & 31)) & 1;
                                if (got != exp && !wrong++)
                                        printf("corpus %u case %u document %u: drops %d, the contract %d\n", ci, k, d, got, exp);
                        }
                        bad += wrong != 0;
                }
        }
        printf("cases %zu bad %zu\n", ncases, bad);
        return (bad != 0) | (refusals() != 0);
}

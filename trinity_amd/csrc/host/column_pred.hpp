// column_pred.hpp — column predicates (include/trinity_hip.h: tri_clause / tri_predicate, tri_filters_from_columns) on the HOST: the validation the C-ABI entry
// runs before it touches the device, and the evaluation of a predicate for one document over host copies of the columns — what the operator surface's
// ColumnPredicateFilter answers filter(id) with (trinity_gpu.hpp), and what the device's bitmaps are checked against (tests/cpp/colpred_cpu_test.cpp).
// No HIP, no allocation beyond the caller's vectors.  New code, no reference source.
//
// The handles (tri_column, tri_filter, tri_index) are opaque here: the caller passes how to ask a column or a filter for its index (validation) and how to reach a
// column's values (evaluation) as callables.
#pragma once
#include "../../../include/trinity_hip.h"
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace colpred {
        inline std::string text(const char *fmt, ...) {
                char buf[320];
                va_list ap;
                va_start(ap, fmt);
                vsnprintf(buf, sizeof buf, fmt, ap);
                va_end(ap);
                return buf;
        }

        // TRI_OK, or TRI_ERR_INVALID with `why` naming the predicate and the clause.  index_of_column(c) / index_of_filter(f): the index a handle belongs to, compared
        // with `ix`.  columns: the call's DISTINCT columns in the order the clauses first name them (a clause's column number is its position there).
        // Nothing is read through clause.set beyond set[0 .. nset).
        template <class IndexOfColumn, class IndexOfFilter>
        int validate(const void *ix, const tri_predicate *preds, const size_t np, const int mode, const void *out, IndexOfColumn index_of_column, IndexOfFilter index_of_filter,
                     std::vector<const tri_column *> &columns, std::string &why) {
                const char *fn = "tri_filters_from_columns";
                columns.clear();
                if (!ix || !preds || !out)
                        return why = text("%s: null argument", fn), TRI_ERR_INVALID;
                if (mode != TRI_FILTER_DROP && mode != TRI_FILTER_KEEP)
                        return why = text("%s: mode %d is neither TRI_FILTER_DROP nor TRI_FILTER_KEEP", fn, mode), TRI_ERR_INVALID;
                if (!np || np > TRI_PREDS_MAX)
                        return why = text("%s: %zu predicates (1 .. %d)", fn, np, TRI_PREDS_MAX), TRI_ERR_INVALID;
                for (size_t p = 0; p < np; ++p) {
                        const tri_predicate &P = preds[p];
                        if (P.nclauses < 1 || P.nclauses > TRI_PRED_MAX_CLAUSES)
                                return why = text("%s: predicate %zu has %u clauses (1 .. %d)", fn, p, P.nclauses, TRI_PRED_MAX_CLAUSES), TRI_ERR_INVALID;
                        if (!P.clauses)
                                return why = text("%s: predicate %zu: null argument (clauses)", fn, p), TRI_ERR_INVALID;
                        if (P.reserved)
                                return why = text("%s: predicate %zu: reserved is not 0", fn, p), TRI_ERR_INVALID;
                        if (P.also && index_of_filter(P.also) != ix)
                                return why = text("%s: predicate %zu: the `also` filter belongs to another index", fn, p), TRI_ERR_INVALID;
                        for (uint32_t k = 0; k < P.nclauses; ++k) {
                                const tri_clause &C = P.clauses[k];
                                if (!C.column)
                                        return why = text("%s: predicate %zu clause %u: null argument (column)", fn, p, k), TRI_ERR_INVALID;
                                if (index_of_column(C.column) != ix)
                                        return why = text("%s: predicate %zu clause %u: the column belongs to another index", fn, p, k), TRI_ERR_INVALID;
                                if (C.kind != TRI_CLAUSE_RANGE && C.kind != TRI_CLAUSE_SET)
                                        return why = text("%s: predicate %zu clause %u: unknown kind %u", fn, p, k, C.kind), TRI_ERR_INVALID;
                                if (C.reserved)
                                        return why = text("%s: predicate %zu clause %u: reserved is not 0", fn, p, k), TRI_ERR_INVALID;
                                if (C.kind == TRI_CLAUSE_SET) {
                                        if (C.nset && !C.set)
                                                return why = text("%s: predicate %zu clause %u: null argument (set)", fn, p, k), TRI_ERR_INVALID;
                                        for (uint32_t i = 0; i < C.nset; ++i)
                                                if (C.set[i] >= TRI_FACET_MAX_BUCKETS)
                                                        return why = text("%s: predicate %zu clause %u: set value %u (entry %u) is not below %u", fn, p, k, C.set[i], i, TRI_FACET_MAX_BUCKETS), TRI_ERR_INVALID;
                                }
                                size_t c = 0;
                                while (c < columns.size() && columns[c] != C.column)
                                        ++c;
                                if (c == columns.size()) {
                                        if (c == TRI_PRED_MAX_COLUMNS)
                                                return why = text("%s: predicate %zu clause %u names the call's column %d (at most %d distinct columns)", fn, p, k, TRI_PRED_MAX_COLUMNS + 1, TRI_PRED_MAX_COLUMNS), TRI_ERR_INVALID;
                                        columns.push_back(C.column);
                                }
                        }
                }
                return TRI_OK;
        }

        // whether clause C holds for a document whose value in C's column is v
        inline bool clause_holds(const tri_clause &C, const uint32_t v) {
                bool t = false;
                if (C.kind == TRI_CLAUSE_RANGE)
                        t = v >= C.lo && v <= C.hi;
                else if (v < TRI_FACET_MAX_BUCKETS)
                        for (uint32_t i = 0; i < C.nset && !t; ++i)
                                t = C.set[i] == v;
                return t != (C.negate != 0);
        }

        // whether predicate P holds for document d; values_of(column) -> const uint32_t *: the column's values, values[d] document d's
        template <class ValuesOf>
        bool holds(const tri_predicate &P, const uint32_t d, ValuesOf values_of) {
                for (uint32_t k = 0; k < P.nclauses; ++k) {
                        const bool t = clause_holds(P.clauses[k], values_of(P.clauses[k].column)[d]);
                        if (t == (P.any != 0)) // any: the first clause that holds decides; all: the first that fails
                                return t;
                }
                return !P.any;
        }

        // whether the filter tri_filters_from_columns makes of P in `mode` DROPS document d (1 .. max_doc), given what P's `also` filter says of it
        template <class ValuesOf>
        bool drops(const tri_predicate &P, const uint32_t d, const int mode, const bool also_drops, ValuesOf values_of) {
                return also_drops || holds(P, d, values_of) == (mode == TRI_FILTER_DROP);
        }
} // namespace colpred

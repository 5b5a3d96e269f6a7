// colfilter_side.hpp — the host runtime of column predicates as document filters: tri_filters_from_columns (validated by host/column_pred.hpp, lowered to the
// records k_filter_columns.hpp reads, one launch for all predicates) and tri_filter_bitmap (any filter's drop bitmap, read back).
// Included by trinity_hip.hip behind the per-query document filters (filter_new, filter_words).  New code, no reference source.
#pragma once
#include "host/column_pred.hpp"

// IndexDocumentsFilter (matches.h:190-201; exec.cpp:1133-1150) from predicates over resident columns.  One pooled block carries the call's records — predicates,
// clauses, the SET clauses' bitsets — to the device; it and the staging go back to the pool before the call returns, the np bitmaps stay with their filters.
extern "C" int tri_filters_from_columns(tri_index *ix, const tri_predicate *preds, size_t np, int mode, tri_filter **out) {
        std::vector<const tri_column *> columns;
        std::string why;
        if (const int rc = colpred::validate(
                ix, preds, np, mode, out, [](const tri_column *c) -> const void * { return c->ix; }, [](const tri_filter *f) -> const void * { return f->ix; }, columns, why))
                return fail(rc, "%s", why.c_str());
        tri_dev *dev = ix->dev;
        HIP_TRY(hipSetDevice(dev->device));
        const size_t words = filter_words(ix);
        static_assert(SPAN_WORDS % (COLFILTER_CHUNK / 32) == 0, "a bitmap's extent is whole chunks of k_filter_columns");
        static_assert(COLFILTER_MAX_CLAUSES == TRI_PRED_MAX_CLAUSES && COLFILTER_MAX_COLUMNS == TRI_PRED_MAX_COLUMNS && COLFILTER_MAX_PREDS == TRI_PREDS_MAX &&
                              COLFILTER_RANGE == TRI_CLAUSE_RANGE && COLFILTER_SET == TRI_CLAUSE_SET,
                      "dev_structs.hpp mirrors the header");

        // ---- the records: [DevColPred np][DevColClause nc][bitset words], the SET clauses' bitsets sized by their largest value (at most 8 KB each)
        size_t nc = 0;
        for (size_t p = 0; p < np; ++p)
                nc += preds[p].nclauses;
        std::vector<DevColClause> clauses;
        clauses.reserve(nc);
        std::vector<uint32_t> sets;
        std::vector<DevColPred> recs(np);
        DevColColumns cols{};
        for (size_t c = 0; c < columns.size(); ++c)
                cols.col[c] = columns[c]->d_values;
        for (size_t p = 0; p < np; ++p) {
                const tri_predicate &P = preds[p];
                recs[p] = DevColPred{(uint32_t)clauses.size(), P.nclauses, P.any ? 1u : 0u, 0u, P.also ? (const uint32_t *)P.also->d_bits : nullptr, nullptr};
                for (uint32_t k = 0; k < P.nclauses; ++k) {
                        const tri_clause &C = P.clauses[k];
                        DevColClause d{};
                        d.col = (uint32_t)(std::find(columns.begin(), columns.end(), C.column) - columns.begin());
                        d.kind = C.kind;
                        d.negate = C.negate ? 1u : 0u;
                        d.lo = C.lo, d.hi = C.hi;
                        if (C.kind == TRI_CLAUSE_SET) {
                                uint32_t top = 0;
                                for (uint32_t i = 0; i < C.nset; ++i)
                                        top = std::max(top, C.set[i]);
                                const uint32_t nw = C.nset ? top / 32 + 1 : 0;
                                d.lo = 0, d.hi = nw * 32, d.set_off = (uint32_t)sets.size();
                                sets.resize(sets.size() + nw, 0);
                                for (uint32_t i = 0; i < C.nset; ++i)
                                        sets[d.set_off + C.set[i] / 32] |= 1u << (C.set[i] & 31u);
                        }
                        clauses.push_back(d);
                }
        }

        // ---- all np bitmaps, or none
        std::vector<std::unique_ptr<tri_filter>> made(np);
        for (size_t p = 0; p < np; ++p) {
                if (const int rc = filter_new(ix, made[p]))
                        return rc; // (TRI_ERR_NOMEM when the pool cannot supply it; the filters made so far hand their bitmaps back)
                recs[p].out = made[p]->d_bits;
        }
        const size_t preds_bytes = np * sizeof(DevColPred), clauses_bytes = nc * sizeof(DevColClause), sets_bytes = sets.size() * 4;
        std::vector<uint8_t> block(preds_bytes + clauses_bytes + sets_bytes);
        memcpy(block.data(), recs.data(), preds_bytes);
        memcpy(block.data() + preds_bytes, clauses.data(), clauses_bytes);
        if (sets_bytes)
                memcpy(block.data() + preds_bytes + clauses_bytes, sets.data(), sets_bytes);
        Pooled<uint8_t> d_block; // (+ POOL_MIN_BYTES: a pooled buffer whatever its size — no hipMalloc / hipFree pair a call)
        HIP_TRY(d_block.alloc(dev, block.size() + POOL_MIN_BYTES));

        std::unique_lock<std::recursive_mutex> lock(dev->mu);
        HIP_TRY(hipMemcpyAsync(d_block, block.data(), block.size(), hipMemcpyHostToDevice, dev->stream)); // (pageable source: staged before the call returns)
        const uint32_t ncols = (uint32_t)columns.size();
        hipLaunchKernelGGL(k_filter_columns, dim3((unsigned)(words / (COLFILTER_CHUNK / 32))), dim3(COLFILTER_WG), ncols * COLFILTER_CHUNK * 4, dev->stream,
                           (const DevColPred *)(d_block.get()), (const DevColClause *)(d_block.get() + preds_bytes), (const uint32_t *)(d_block.get() + preds_bytes + clauses_bytes), cols, ncols,
                           (uint32_t)np, ix->max_doc, mode == TRI_FILTER_KEEP ? 1u : 0u);
        HIP_TRY(hipGetLastError());
        if (const int rc = filter_finish(made[0].get(), TRI_FILTER_DROP, lock)) // (the polarity is the kernel's: nothing to complement; waits for the bitmaps, outside the lock)
                return rc;
        for (size_t p = 0; p < np; ++p)
                out[p] = made[p].release();
        return TRI_OK;
}

// what IndexDocumentsFilter::filter(id) answers (matches.h:190-201; exec.cpp:1133-1150), for every id at once: the filter's drop bitmap as the kernels read it
extern "C" int tri_filter_bitmap(const tri_filter *f, uint32_t *words, size_t cap, size_t *nwords) {
        if (!f || !words || !nwords)
                return fail(TRI_ERR_INVALID, "tri_filter_bitmap: null argument");
        *nwords = f->words;
        if (cap < f->words)
                return fail(TRI_ERR_INVALID, "tri_filter_bitmap: room for %zu words, the bitmap has %zu", cap, f->words);
        tri_dev *dev = f->dev;
        HIP_TRY(hipSetDevice(dev->device));
        PooledEvent done;
        std::unique_lock<std::recursive_mutex> lock(dev->mu);
        HIP_TRY(hipMemcpyAsync(words, f->d_bits, f->words * 4, hipMemcpyDeviceToHost, dev->stream));
        HIP_TRY(done.take(dev));
        const hipError_t e = hipEventRecord(done, dev->stream);
        lock.unlock(); // (the wait stands outside the lock, like tri_batch_sync's)
        HIP_TRY(e == hipSuccess ? hipEventSynchronize(done) : e);
        return TRI_OK;
}

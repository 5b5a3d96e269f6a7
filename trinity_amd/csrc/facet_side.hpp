// facet_side.hpp — facet counts on the device: the columns (tri_column_*) and a batch's specs and row block (tri_batch_set_facets).  Included once by trinity_hip.hip
// (the same translation unit, as isect_side.hpp is); the kernel is k_facet.hpp, enqueued by tri_batch_run (run_facets); the rows' read side — tri_batch_facets,
// tri_cbatch_facets — is read_side.hpp's; what each call delivers is documented in include/trinity_hip.h.
#pragma once

static_assert(FACETS_MAX == TRI_FACETS_MAX && FACET_MAX_BUCKETS == TRI_FACET_MAX_BUCKETS, "the header's limits are the kernel's");

extern "C" int tri_column_create(tri_index *ix, const uint32_t *values, size_t n, tri_column **out) {
        if (!ix || !values || !out)
                return fail(TRI_ERR_INVALID, "tri_column_create: null argument");
        if (n != (size_t)ix->info.docs_cnt + 1)
                return fail(TRI_ERR_INVALID, "tri_column_create: %zu values for an index of docs_cnt %u (docs_cnt + 1: values[d] is docID d's)", n, ix->info.docs_cnt);
        if (ix->max_doc >= n) // (k_facet never reads past the column, but such a document's attribute would be missing)
                return fail(TRI_ERR_INVALID, "tri_column_create: the index holds docID %u, above its docs_cnt %u: the column cannot cover it", ix->max_doc, ix->info.docs_cnt);
        tri_dev *dev = ix->dev;
        HIP_TRY(hipSetDevice(dev->device));
        auto c = std::make_unique<tri_column>();
        c->ix = ix;
        c->dev.retain(dev);
        c->n = (uint32_t)n;
        HIP_TRY(c->d_values.alloc(n * 4));
        HIP_TRY(hipMemcpy(c->d_values, values, n * 4, hipMemcpyHostToDevice)); // (returns once the column stands)
        *out = c.release();
        return TRI_OK;
}

extern "C" void tri_column_destroy(tri_column *c) {
        delete c; // its d_values hands the column back
}

extern "C" int tri_batch_set_facets(tri_batch *b, const tri_facet *facets, size_t n) {
        if (!b || (n && !facets))
                return fail(TRI_ERR_INVALID, "tri_batch_set_facets: null argument");
        if (b->flags & TRI_FLAG_ACCUMULATED_SCORE)
                return fail(TRI_ERR_INVALID, "tri_batch_set_facets: a TRI_FLAG_ACCUMULATED_SCORE batch's one-pass queries keep no docID sets to count");
        if (n > TRI_FACETS_MAX)
                return fail(TRI_ERR_INVALID, "tri_batch_set_facets: %zu facets (at most %d)", n, TRI_FACETS_MAX);
        DevFacets f{};
        uint64_t counters = 0;
        for (size_t k = 0; k < n; ++k) {
                const tri_facet &s = facets[k];
                if (!s.column || s.column->ix != b->ix)
                        return fail(TRI_ERR_INVALID, "tri_batch_set_facets: facet %zu's column %s", k, s.column ? "belongs to another index" : "is null");
                if (s.nbuckets < 1 || s.nbuckets > TRI_FACET_MAX_BUCKETS)
                        return fail(TRI_ERR_INVALID, "tri_batch_set_facets: facet %zu: nbuckets %u (1 .. %u)", k, s.nbuckets, TRI_FACET_MAX_BUCKETS);
                if (s.reserved)
                        return fail(TRI_ERR_INVALID, "tri_batch_set_facets: facet %zu: reserved must be 0", k);
                f.values[k] = s.column->d_values;
                f.ndocs[k] = s.column->n;
                f.nb[k] = s.nbuckets;
                f.lds_off[k] = f.per_query;
                f.rows_off[k] = counters;
                f.per_query += s.nbuckets + 1;
                counters += (uint64_t)b->nq * (s.nbuckets + 1);
        }
        f.lds_off[n] = f.per_query;
        f.n = (uint32_t)n;
        tri_dev *dev = b->dev;
        DevLock dev_lock(dev->mu);
        HIP_TRY(hipSetDevice(dev->device));
        Pooled<uint32_t> rows; // (the batch keeps the block it has until the new one stands)
        PooledEvent ev[2];
        if (n) {
                // (+ POOL_MIN_BYTES, as the plane cache's small blocks are taken: the block is then a POOLED buffer whatever its size — a facet set replaced run after run
                //  reuses an idle one instead of a hipMalloc / hipFree pair, and hipFree would synchronise the device)
                if (const hipError_t e = rows.alloc(dev, counters * 4 + POOL_MIN_BYTES))
                        return fail(e == hipErrorOutOfMemory ? TRI_ERR_NOMEM : TRI_ERR_DEVICE, "tri_batch_set_facets: the row block (%zu queries x %u counters x 4 B): %s", b->nq, f.per_query,
                                    hipGetErrorString(e));
                for (int i = 0; i < 2; ++i)
                        if (!b->facet_ev[i])
                                HIP_TRY(ev[i].take(dev));
        }
        if (b->ran && !b->synced) // (a run already queued counts into the block it was launched with: the block goes back to the pool behind it)
                HIP_TRY(hipStreamSynchronize(dev->stream));
        const uint32_t had = b->facets.n && !b->tasks.empty(), has = n && !b->tasks.empty();
        b->info.launches += has - had;
        b->d_facet_rows = std::move(rows);
        for (int i = 0; i < 2; ++i)
                if (ev[i])
                        b->facet_ev[i] = std::move(ev[i]);
        b->facets = f;
        b->facet_counters = (size_t)counters;
        b->facet_ran = b->facet_done = false;
        return TRI_OK;
}

// stats_side.hpp — stats of a column per query and bucket on the device: a batch's specs and row block (tri_batch_set_stats).  Included once by trinity_hip.hip (the
// same translation unit, as facet_side.hpp is); the columns are facet_side.hpp's (tri_column_*); the kernel is k_stats.hpp, enqueued by tri_batch_run (run_stats); the
// rows' read side — tri_batch_stats, tri_cbatch_stats — is read_side.hpp's; what each call delivers is documented in include/trinity_hip.h.
#pragma once

static_assert(STATS_MAX == TRI_STATS_MAX, "the header's limit is the kernel's");

extern "C" int tri_batch_set_stats(tri_batch *b, const tri_stat *stats, size_t n) {
        if (!b || (n && !stats))
                return fail(TRI_ERR_INVALID, "tri_batch_set_stats: null argument");
        if (b->flags & TRI_FLAG_ACCUMULATED_SCORE)
                return fail(TRI_ERR_INVALID, "tri_batch_set_stats: a TRI_FLAG_ACCUMULATED_SCORE batch's one-pass queries keep no docID sets to count");
        if (n > TRI_STATS_MAX)
                return fail(TRI_ERR_INVALID, "tri_batch_set_stats: %zu stats (at most %d)", n, TRI_STATS_MAX);
        DevStats s{};
        uint64_t words = 0;
        for (size_t k = 0; k < n; ++k) {
                const tri_stat &t = stats[k];
                if (!t.value || t.value->ix != b->ix)
                        return fail(TRI_ERR_INVALID, "tri_batch_set_stats: stat %zu's value column %s", k, t.value ? "belongs to another index" : "is null");
                if (t.group && t.group->ix != b->ix)
                        return fail(TRI_ERR_INVALID, "tri_batch_set_stats: stat %zu's group column belongs to another index", k);
                if (t.group && (t.nbuckets < 1 || t.nbuckets > TRI_FACET_MAX_BUCKETS))
                        return fail(TRI_ERR_INVALID, "tri_batch_set_stats: stat %zu: nbuckets %u (1 .. %u)", k, t.nbuckets, TRI_FACET_MAX_BUCKETS);
                if (!t.group && t.nbuckets)
                        return fail(TRI_ERR_INVALID, "tri_batch_set_stats: stat %zu: nbuckets %u without a group column (must be 0: one bucket)", k, t.nbuckets);
                if (t.reserved)
                        return fail(TRI_ERR_INVALID, "tri_batch_set_stats: stat %zu: reserved must be 0", k);
                s.group[k] = t.group ? (const uint32_t *)t.group->d_values : nullptr;
                s.value[k] = t.value->d_values;
                s.ndocs = t.value->n; // (every column of an index has docs_cnt + 1 entries: tri_column_create)
                s.nb[k] = t.nbuckets;
                s.lds_off[k] = s.lds_records;
                s.off[k] = words;
                if (t.group)
                        s.lds_records += t.nbuckets + 1;
                const uint64_t records = (uint64_t)b->nq * (t.nbuckets + 1);
                words += 5 * records + (records & 1); // (sums 2 R, counts, mins, maxs R each; padded: the next stat's sums are 8-byte aligned too)
        }
        for (size_t k = n; k <= STATS_MAX; ++k)
                s.lds_off[k] = s.lds_records;
        s.n = (uint32_t)n;
        s.nq = (uint32_t)b->nq;
        tri_dev *dev = b->dev;
        DevLock dev_lock(dev->mu);
        HIP_TRY(hipSetDevice(dev->device));
        Pooled<uint32_t> rows; // (the batch keeps the block it has until the new one stands)
        PooledEvent ev[2];
        if (n) {
                // (+ POOL_MIN_BYTES, as the facets' row block is taken: a POOLED buffer whatever its size — a set replaced run after run reuses an idle one)
                if (const hipError_t e = rows.alloc(dev, words * 4 + POOL_MIN_BYTES))
                        return fail(e == hipErrorOutOfMemory ? TRI_ERR_NOMEM : TRI_ERR_DEVICE, "tri_batch_set_stats: the row block (%zu queries, %llu bytes): %s", b->nq,
                                    (unsigned long long)words * 4, hipGetErrorString(e));
                for (int i = 0; i < 2; ++i)
                        if (!b->stats_ev[i])
                                HIP_TRY(ev[i].take(dev));
        }
        if (b->ran && !b->synced) // (a run already queued aggregates into the block it was launched with: the block goes back to the pool behind it)
                HIP_TRY(hipStreamSynchronize(dev->stream));
        const uint32_t had = b->stats.n && !b->tasks.empty(), has = n && !b->tasks.empty();
        b->info.launches += has - had;
        b->d_stats_rows = std::move(rows);
        for (int i = 0; i < 2; ++i)
                if (ev[i])
                        b->stats_ev[i] = std::move(ev[i]);
        b->stats = s;
        b->stats_words = (size_t)words;
        b->stats_ran = b->stats_done = false;
        return TRI_OK;
}

// consumers.hpp — the consumers of a batch's finished docID sets on the device: facet counts (tri_batch_set_facets, k_facet.hpp), order by a column (tri_batch_set_order,
// k_order.hpp) and stats of a column (tri_batch_set_stats, k_stats.hpp), and the columns they read (tri_column_*).  Included once by trinity_hip.hip (the same
// translation unit, as isect_side.hpp is), ahead of tri_batch_run.  One lifecycle for the three (tri_batch::ConsumerSlot):
//   set    the entry point validates its spec and sizes its block, then consumer_stage obtains the new block and the events the slot lacks into locals — a failure
//          leaves the batch as it was: it keeps what it has until the new one stands — and consumer_commit waits for a queued run, adjusts info.launches and moves them in
//   run    run_consumers, from tri_batch_run behind the kernels that complete the docID sets (the consumers' kernels read the device-side task counts) and ahead of the
//          run's end event: facets, order, stats, each between its slot's two events.  A consumer that is not set enqueues nothing
//   sync   sync_consumers, from tri_batch_sync: the events' span goes to the option *_last_us, and the slot is done
//   read   consumer_ready refuses a read of a consumer that is not set, or whose spec no synced run has seen.  The rows' read side — tri_batch_facets / _ordered /
//          _stats and the collection forms — is read_side.hpp's; what each call delivers is documented in include/trinity_hip.h.
#pragma once

static_assert(FACETS_MAX == TRI_FACETS_MAX && FACET_MAX_BUCKETS == TRI_FACET_MAX_BUCKETS && STATS_MAX == TRI_STATS_MAX && ORDER_MAX_TOPK == TRI_ORDER_MAX_TOPK,
              "the header's limits are the kernels'");

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

namespace {
        // ---- set
        int consumer_refuse_onepass(const tri_batch *b, const char *fn, const char *verb) {
                return b->flags & TRI_FLAG_ACCUMULATED_SCORE ? fail(TRI_ERR_INVALID, "%s: a TRI_FLAG_ACCUMULATED_SCORE batch's one-pass queries keep no docID sets to %s", fn, verb) : TRI_OK;
        }

        // what is wrong with a spec's column, in the words the setters' refusals end with; nullptr: it is a column of the batch's index
        const char *column_fault(const tri_batch *b, const tri_column *c) { return !c ? "is null" : c->ix != b->ix ? "belongs to another index" : nullptr; }

        // phase 1, under the device lock: the new block — `what` describes it, for the refusal — and the events the slot lacks, into `st`, a slot of the setter's own
        // (its block and events are all that is used).  Nothing of the batch is written.
        // (+ POOL_MIN_BYTES, as the plane cache's small blocks are taken: the block is then a POOLED buffer whatever its size — a spec replaced run after run reuses an
        //  idle one instead of a hipMalloc / hipFree pair, and hipFree would synchronise the device)
        int consumer_stage(const tri_batch *b, const Consumer which, const size_t bytes, const char *fn, const char *what, tri_batch::ConsumerSlot &st) {
                tri_dev *dev = b->dev;
                if (const hipError_t e = st.block.alloc(dev, bytes + POOL_MIN_BYTES))
                        return fail(e == hipErrorOutOfMemory ? TRI_ERR_NOMEM : TRI_ERR_DEVICE, "%s: %s: %s", fn, what, hipGetErrorString(e));
                for (int i = 0; i < 2; ++i)
                        if (!b->consumers[which].ev[i])
                                HIP_TRY(st.ev[i].take(dev));
                return TRI_OK;
        }

        // phase 2: the staged block (none: the consumer is cleared) becomes the slot's; the caller stores its spec behind a TRI_OK
        int consumer_commit(tri_batch *b, const Consumer which, tri_batch::ConsumerSlot &st, const bool on, const uint32_t launches) {
                tri_batch::ConsumerSlot &s = b->consumers[which];
                if (b->ran && !b->synced) // (a run already queued writes into the block it was launched with: the block goes back to the pool behind it)
                        HIP_TRY(hipStreamSynchronize(b->dev->stream));
                if (!b->tasks.empty())
                        b->info.launches += (on ? launches : 0u) - (s.on ? s.launches : 0u);
                s.block = std::move(st.block);
                for (int i = 0; i < 2; ++i)
                        if (st.ev[i])
                                s.ev[i] = std::move(st.ev[i]);
                s.on = on;
                s.launches = launches;
                s.ran = s.done = false;
                return TRI_OK;
        }

        // The rounds of k_order_merge for this batch: they depend on the plan alone (which tasks are whose), not on the spec — laid out by the first setter and kept.
        // Round 0 reads the tasks' partial lists; a query of at most ORDER_FANIN lists is folded into its row, a longer one into ceil(n / ORDER_FANIN) lists of the
        // next level, which the next round reads.  Every caller query has exactly one row group (a query without tasks: of no lists — its row is zeroed).
        int order_layout(tri_batch *b) {
                if (b->order_laid_out)
                        return TRI_OK;
                struct Cur {
                        uint32_t q, first, n;
                };
                std::vector<Cur> cur, next;
                for (size_t q = 0; q < b->nq; ++q) {
                        const uint32_t slot = b->slot_of_query[q];
                        if (slot == UINT32_MAX)
                                cur.push_back({(uint32_t)q, 0u, 0u}); // (the planner left it out)
                        else
                                cur.push_back({(uint32_t)q, b->plan[slot].first_task, b->plan[slot].ntasks});
                }
                std::vector<DevOrderGroup> groups;
                std::vector<tri_batch::OrderRound> rounds;
                size_t level[2] = {0, 0}; // lists of the two intermediate regions (the rounds alternate between them)
                while (!cur.empty()) {
                        tri_batch::OrderRound r{(uint32_t)groups.size(), 0u};
                        uint32_t made = 0;
                        next.clear();
                        for (const Cur &c : cur) {
                                if (c.n <= ORDER_FANIN) {
                                        groups.push_back({c.first, c.n, c.q, 1u});
                                        continue;
                                }
                                const uint32_t m = (c.n + ORDER_FANIN - 1) / ORDER_FANIN;
                                for (uint32_t i = 0; i < m; ++i)
                                        groups.push_back({c.first + i * ORDER_FANIN, std::min(ORDER_FANIN, c.n - i * ORDER_FANIN), made + i, 0u});
                                next.push_back({c.q, made, m});
                                made += m;
                        }
                        r.ngroups = (uint32_t)groups.size() - r.first_group;
                        level[rounds.size() & 1] = std::max<size_t>(level[rounds.size() & 1], made);
                        rounds.push_back(r);
                        cur.swap(next);
                }
                if (const int rc = dev_upload(b->d_order_groups, groups))
                        return rc;
                b->order_rounds = std::move(rounds);
                b->order_level[0] = level[0];
                b->order_level[1] = level[1];
                b->order_laid_out = true;
                return TRI_OK;
        }
} // namespace

extern "C" int tri_batch_set_facets(tri_batch *b, const tri_facet *facets, size_t n) {
        if (!b || (n && !facets))
                return fail(TRI_ERR_INVALID, "tri_batch_set_facets: null argument");
        if (const int rc = consumer_refuse_onepass(b, __func__, "count"))
                return rc;
        if (n > TRI_FACETS_MAX)
                return fail(TRI_ERR_INVALID, "tri_batch_set_facets: %zu facets (at most %d)", n, TRI_FACETS_MAX);
        DevFacets f{};
        uint64_t counters = 0;
        for (size_t k = 0; k < n; ++k) {
                const tri_facet &s = facets[k];
                if (const char *why = column_fault(b, s.column))
                        return fail(TRI_ERR_INVALID, "tri_batch_set_facets: facet %zu's column %s", k, why);
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
        DevLock dev_lock(b->dev->mu);
        HIP_TRY(hipSetDevice(b->dev->device));
        tri_batch::ConsumerSlot st;
        if (n) {
                char what[128];
                snprintf(what, sizeof what, "the row block (%zu queries x %u counters x 4 B)", b->nq, f.per_query);
                if (const int rc = consumer_stage(b, CONSUMER_FACETS, counters * 4, __func__, what, st))
                        return rc;
        }
        if (const int rc = consumer_commit(b, CONSUMER_FACETS, st, n != 0, 1u))
                return rc;
        b->facets = f;
        b->facet_counters = (size_t)counters;
        return TRI_OK;
}

extern "C" int tri_batch_set_order(tri_batch *b, const tri_order *spec) {
        if (!b)
                return fail(TRI_ERR_INVALID, "tri_batch_set_order: null argument");
        DevOrder o{};
        if (spec) {
                if (const int rc = consumer_refuse_onepass(b, __func__, "order"))
                        return rc;
                if (const char *why = column_fault(b, spec->column))
                        return fail(TRI_ERR_INVALID, "tri_batch_set_order: the column %s", why);
                if (spec->topk < 1 || spec->topk > TRI_ORDER_MAX_TOPK)
                        return fail(TRI_ERR_INVALID, "tri_batch_set_order: topk %u (1 .. %d)", spec->topk, TRI_ORDER_MAX_TOPK);
                if (spec->reserved)
                        return fail(TRI_ERR_INVALID, "tri_batch_set_order: reserved must be 0");
                o.values = spec->column->d_values;
                o.ndocs = spec->column->n;
                o.topk = spec->topk;
                o.flip = spec->descending ? 0xffffffffu : 0u;
        }
        DevLock dev_lock(b->dev->mu);
        HIP_TRY(hipSetDevice(b->dev->device));
        tri_batch::ConsumerSlot st;
        size_t lists = 0;
        if (spec) {
                if (const int rc = order_layout(b))
                        return rc;
                // the block: [task lists | level lists | level lists | rows] x topk keys, then a length per list and row
                lists = b->tasks.size() + b->order_level[0] + b->order_level[1];
                char what[128];
                snprintf(what, sizeof what, "the list block (%zu lists and %zu rows x %u keys x 8 B)", lists, b->nq, o.topk);
                if (const int rc = consumer_stage(b, CONSUMER_ORDER, (lists + b->nq) * ((size_t)o.topk * 8 + 4) + 8, __func__, what, st))
                        return rc;
        }
        if (const int rc = consumer_commit(b, CONSUMER_ORDER, st, spec != nullptr, 1u + (uint32_t)b->order_rounds.size())) // k_order and a k_order_merge per round
                return rc;
        b->order = o;
        b->order_lists = lists;
        return TRI_OK;
}

extern "C" int tri_batch_set_stats(tri_batch *b, const tri_stat *stats, size_t n) {
        if (!b || (n && !stats))
                return fail(TRI_ERR_INVALID, "tri_batch_set_stats: null argument");
        if (const int rc = consumer_refuse_onepass(b, __func__, "count"))
                return rc;
        if (n > TRI_STATS_MAX)
                return fail(TRI_ERR_INVALID, "tri_batch_set_stats: %zu stats (at most %d)", n, TRI_STATS_MAX);
        DevStats s{};
        uint64_t words = 0;
        for (size_t k = 0; k < n; ++k) {
                const tri_stat &t = stats[k];
                if (const char *why = column_fault(b, t.value))
                        return fail(TRI_ERR_INVALID, "tri_batch_set_stats: stat %zu's value column %s", k, why);
                if (const char *why = t.group ? column_fault(b, t.group) : nullptr)
                        return fail(TRI_ERR_INVALID, "tri_batch_set_stats: stat %zu's group column %s", k, why);
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
        DevLock dev_lock(b->dev->mu);
        HIP_TRY(hipSetDevice(b->dev->device));
        tri_batch::ConsumerSlot st;
        if (n) {
                char what[128];
                snprintf(what, sizeof what, "the row block (%zu queries, %llu bytes)", b->nq, (unsigned long long)words * 4);
                if (const int rc = consumer_stage(b, CONSUMER_STATS, words * 4, __func__, what, st))
                        return rc;
        }
        if (const int rc = consumer_commit(b, CONSUMER_STATS, st, n != 0, 1u))
                return rc;
        b->stats = s;
        b->stats_words = (size_t)words;
        return TRI_OK;
}

// ---- run: what each consumer enqueues between its two events
static int enqueue_facets(tri_batch *b) { // the rows zeroed and counted
        tri_dev *dev = b->dev;
        HIP_TRY(hipMemsetAsync(b->facet_rows(), 0, b->facet_counters * 4, dev->stream));
        if (!b->tasks.empty()) {
                hipLaunchKernelGGL(k_facet, dim3((uint32_t)b->tasks.size()), dim3(FACET_WG), 0, dev->stream, (const DevQuery *)b->dev_at(b->plan), (const DevTask *)b->dev_at(b->tasks),
                                   (const uint32_t *)b->d_counts, (const uint32_t *)b->d_out, b->facets, b->facet_rows());
                HIP_TRY(hipGetLastError());
        }
        return TRI_OK;
}

static int enqueue_order(tri_batch *b) { // every task's best keys selected into its partial list, then a query's lists folded into its row, round after round
        tri_dev *dev = b->dev;
        const uint32_t k = b->order.topk;
        const size_t ntasks = b->tasks.size(), rows = b->order_lists;
        if (b->tasks.empty()) { // (no query has a task: every row is empty)
                HIP_TRY(hipMemsetAsync(b->order_keys(rows), 0, b->nq * (size_t)k * 8, dev->stream));
                HIP_TRY(hipMemsetAsync(b->order_counts(rows), 0, b->nq * 4, dev->stream));
                return TRI_OK;
        }
        hipLaunchKernelGGL(k_order, dim3((uint32_t)ntasks), dim3(ORDER_WG), 0, dev->stream, (const DevQuery *)b->dev_at(b->plan), (const DevTask *)b->dev_at(b->tasks),
                           (const uint32_t *)b->d_counts, (const uint32_t *)b->d_out, b->order, b->order_keys(0), b->order_counts(0));
        HIP_TRY(hipGetLastError());
        const size_t level_at[2] = {ntasks, ntasks + b->order_level[0]};
        for (size_t r = 0; r < b->order_rounds.size(); ++r) {
                const tri_batch::OrderRound &round = b->order_rounds[r];
                const size_t from = r ? level_at[(r - 1) & 1] : 0, to = level_at[r & 1];
                hipLaunchKernelGGL(k_order_merge<false>, dim3(round.ngroups), dim3(ORDER_WG), 0, dev->stream, (const DevOrderLists *)nullptr,
                                   DevOrderLists{b->order_keys(from), b->order_counts(from)}, (const DevOrderGroup *)b->d_order_groups + round.first_group, 0u, k, b->order_keys(to),
                                   b->order_counts(to), b->order_keys(rows), b->order_counts(rows));
                HIP_TRY(hipGetLastError());
        }
        return TRI_OK;
}

static int enqueue_stats(tri_batch *b) { // the rows initialised (the mins planes to 0xffffffff, everything else to 0) and aggregated
        tri_dev *dev = b->dev;
        HIP_TRY(hipMemsetAsync(b->stats_rows(), 0, b->stats_words * 4, dev->stream));
        for (uint32_t k = 0; k < b->stats.n; ++k) {
                const size_t records = b->nq * ((size_t)b->stats.nb[k] + 1);
                HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(b->stats_rows() + b->stats.off[k] + 3 * records), (int)0xffffffffu, records, dev->stream));
        }
        if (!b->tasks.empty()) {
                hipLaunchKernelGGL(k_stats, dim3((uint32_t)b->tasks.size()), dim3(STATS_WG), 0, dev->stream, (const DevQuery *)b->dev_at(b->plan), (const DevTask *)b->dev_at(b->tasks),
                                   (const uint32_t *)b->d_counts, (const uint32_t *)b->d_out, b->stats, b->stats_rows());
                HIP_TRY(hipGetLastError());
        }
        return TRI_OK;
}

static int run_consumers(tri_batch *b) {
        static int (*const enqueue[CONSUMER_COUNT])(tri_batch *) = {enqueue_facets, enqueue_order, enqueue_stats};
        for (int i = 0; i < CONSUMER_COUNT; ++i) {
                tri_batch::ConsumerSlot &s = b->consumers[i];
                s.ran = s.done = false;
                if (!s.on)
                        continue;
                HIP_TRY(hipEventRecord(s.ev[0], b->dev->stream));
                if (const int rc = enqueue[i](b))
                        return rc;
                HIP_TRY(hipEventRecord(s.ev[1], b->dev->stream));
                s.ran = true;
        }
        return TRI_OK;
}

// ---- sync: behind the wait for the run's end event (both events of every slot precede it)
static void sync_consumers(tri_batch *b) {
        for (int i = 0; i < CONSUMER_COUNT; ++i) {
                tri_batch::ConsumerSlot &s = b->consumers[i];
                if (!s.ran)
                        continue;
                float ms = 0;
                if (hipEventElapsedTime(&ms, s.ev[0], s.ev[1]) == hipSuccess)
                        b->dev->consumer_last_us[i] = (uint64_t)(ms * 1000.0f);
                s.done = true;
        }
}

// ---- read: may `fn` deliver this consumer's rows?  set: "facets are", "order is", "stats are"
static int consumer_ready(const tri_batch *b, const Consumer which, const char *fn, const char *setter_name) {
        static const char *const set[CONSUMER_COUNT] = {"facets are", "order is", "stats are"};
        const tri_batch::ConsumerSlot &s = b->consumers[which];
        if (!s.on)
                return fail(TRI_ERR_INVALID, "%s: no %s set (%s)", fn, set[which], setter_name);
        if (!b->synced || !s.done)
                return fail(TRI_ERR_INVALID, "%s: tri_batch_sync first (a run that follows %s)", fn, setter_name);
        return TRI_OK;
}

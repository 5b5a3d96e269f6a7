// order_side.hpp — order by a column on the device: a batch's spec, its list / row block and the rounds of its merge (tri_batch_set_order).  Included once by
// trinity_hip.hip (the same translation unit, as facet_side.hpp is); the kernels are k_order.hpp, enqueued by tri_batch_run (run_order); the rows' read side —
// tri_batch_ordered, tri_cbatch_ordered — is read_side.hpp's; what each call delivers is documented in include/trinity_hip.h.
#pragma once

static_assert(ORDER_MAX_TOPK == TRI_ORDER_MAX_TOPK, "the header's limit is the kernel's");

namespace {
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

extern "C" int tri_batch_set_order(tri_batch *b, const tri_order *spec) {
        if (!b)
                return fail(TRI_ERR_INVALID, "tri_batch_set_order: null argument");
        DevOrder o{};
        if (spec) {
                if (b->flags & TRI_FLAG_ACCUMULATED_SCORE)
                        return fail(TRI_ERR_INVALID, "tri_batch_set_order: a TRI_FLAG_ACCUMULATED_SCORE batch's one-pass queries keep no docID sets to order");
                if (!spec->column || spec->column->ix != b->ix)
                        return fail(TRI_ERR_INVALID, "tri_batch_set_order: the column %s", spec->column ? "belongs to another index" : "is null");
                if (spec->topk < 1 || spec->topk > TRI_ORDER_MAX_TOPK)
                        return fail(TRI_ERR_INVALID, "tri_batch_set_order: topk %u (1 .. %d)", spec->topk, TRI_ORDER_MAX_TOPK);
                if (spec->reserved)
                        return fail(TRI_ERR_INVALID, "tri_batch_set_order: reserved must be 0");
                o.values = spec->column->d_values;
                o.ndocs = spec->column->n;
                o.topk = spec->topk;
                o.flip = spec->descending ? 0xffffffffu : 0u;
        }
        tri_dev *dev = b->dev;
        DevLock dev_lock(dev->mu);
        HIP_TRY(hipSetDevice(dev->device));
        Pooled<uint64_t> block; // (the batch keeps the block it has until the new one stands)
        PooledEvent ev[2];
        size_t lists = 0;
        if (spec) {
                if (const int rc = order_layout(b))
                        return rc;
                // the block: [task lists | level lists | level lists | rows] x topk keys, then a length per list and row.  (+ POOL_MIN_BYTES, as the facets' row block
                // is taken: a POOLED buffer whatever its size — an order replaced run after run reuses an idle one instead of a hipMalloc / hipFree pair)
                lists = b->tasks.size() + b->order_level[0] + b->order_level[1];
                const size_t bytes = (lists + b->nq) * ((size_t)o.topk * 8 + 4) + 8;
                if (const hipError_t e = block.alloc(dev, bytes + POOL_MIN_BYTES))
                        return fail(e == hipErrorOutOfMemory ? TRI_ERR_NOMEM : TRI_ERR_DEVICE, "tri_batch_set_order: the list block (%zu lists and %zu rows x %u keys x 8 B): %s", lists, b->nq,
                                    o.topk, hipGetErrorString(e));
                for (int i = 0; i < 2; ++i)
                        if (!b->order_ev[i])
                                HIP_TRY(ev[i].take(dev));
        }
        if (b->ran && !b->synced) // (a run already queued selects into the block it was launched with: the block goes back to the pool behind it)
                HIP_TRY(hipStreamSynchronize(dev->stream));
        const uint32_t per_run = 1u + (uint32_t)b->order_rounds.size(); // k_order and a k_order_merge per round
        const uint32_t had = b->order_on && !b->tasks.empty() ? per_run : 0u, has = spec && !b->tasks.empty() ? per_run : 0u;
        b->info.launches += has - had;
        b->d_order_block = std::move(block);
        for (int i = 0; i < 2; ++i)
                if (ev[i])
                        b->order_ev[i] = std::move(ev[i]);
        b->order = o;
        b->order_on = spec != nullptr;
        b->order_lists = lists;
        b->order_ran = b->order_done = false;
        return TRI_OK;
}

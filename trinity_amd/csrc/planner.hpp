// planner.hpp — the host planner behind tri_batch_create: postfix query programs -> the plan the kernels execute.
//
// Takes over, for a whole batch of queries at once, what the reference does per query before the first posting is touched:
// queryexec_ctx::build_iterator (exec.cpp:253-449: flattening of nested AND / OR :339-358, 382-393, operand ordering by cost
// :35-110, 133-240), build_span's choice of execution strategy (:452-505) and the scorer-weight set-up (similarity.h:179-226) —
// restated as data: CNF groups or a truth table per query, an execution class (candidate tiles / bitmap windows / one-pass scored
// windows / bit planes), tasks cut to even cost with private output regions, the head terms the batch shares (term planes), and one
// contiguous host block that is copied to the device in a single transfer.
//
// Host-only C++17, no HIP: trinity_hip.hip materialises the plan on the device; csrc/host/plan_host.cpp and tests/test_planner.py drive it
// without one.  The queries of a batch are independent, so every pass over them runs on a few host threads (HostPool) over contiguous
// fragments of the batch; what is global (the one-pass task size, the chosen planes, offsets into the shared arrays) is settled between
// the passes from per-fragment sums.  This file: plan_batch as its passes in call order, sharing one PlanState.  The types, the options
// and the list of the block's sections: planner_types.hpp; a query's lowering: planner_lower.hpp; its tasks: planner_tasks.hpp.
// New code, no reference source.
#pragma once
#include "planner_lower.hpp"
#include "planner_tasks.hpp"

namespace trip {
        // row -> queue(s) of k_and and the row's place in the queue (assign_cand_rows)
        struct RowQ {
                uint8_t n = 0, q[CAND_QUEUES] = {}, sub[CAND_QUEUES] = {};
        };
        // TRINITY_DEBUG_PLAN (stderr): the passes and the serial stretches between them
        struct LapTimer {
                const bool on;
                std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
                std::string line;
                void lap(const char *what) {
                        if (!on)
                                return;
                        char buf[64];
                        snprintf(buf, sizeof buf, " %s %.3f", what, ms_since(t0));
                        line += buf;
                }
        };

        // what the passes of one plan_batch share
        struct PlanState {
                const HostIndex &ix;
                const PlanEnv &env;
                const tri_options &opt;
                HostPool *pool;
                BatchPlan &P;
                std::string &err;
                Ctx C;
                LapTimer dbg;
                FragCache *cache = nullptr;
                std::vector<Frag> frags;
                SectionCounts n;
                uint64_t cand_queries_all = 0;      // candidate-tile and probe queries
                std::vector<uint64_t> benefit, cand_row; // per eligible term (by df rank): the fragments' sums
                std::vector<uint32_t> tree_terms;   // the distinct term leaves of the batch's TASK_TREE queries, ascending
                std::vector<uint32_t> chosen;       // the terms that get a plane, ascending
                std::vector<uint32_t> row_of_rank;  // df rank -> plane row, or PL_NONE
                bool cand_rows = false;             // k_and's tasks are queued by the plane row they probe
                std::vector<RowQ> rowq;
                uint32_t pset_ranges = 0;           // window ranges of the docID space (a TASK_PSET task's range: its first window / PSET_TASK_WINDOWS)
                uint32_t cand_first = 0, cand_qat[CAND_QUEUES] = {}; // (place_schedule) where the TASK_CAND section of sched, and each of its queues, begins
                std::vector<uint32_t> unit_of_task;
                ~PlanState() { // (every way out of plan_batch hands the fragments' buffers back to the caller's cache)
                        if (!cache)
                                return;
                        if (cache->frags.size() < frags.size())
                                cache->frags.resize(frags.size());
                        for (size_t k = 0; k < frags.size(); ++k)
                                cache->frags[k] = std::move(frags[k]);
                }
                template <class Fn>
                void run(Fn &&fn) { // fn(fragment index), on the pool
                        if (pool && frags.size() > 1)
                                pool->run((unsigned)frags.size(), fn);
                        else
                                for (unsigned k = 0; k < frags.size(); ++k)
                                        fn(k);
                }
                int first_error() {
                        for (Frag &f : frags)
                                if (f.rc != TRI_OK) {
                                        err = f.err;
                                        return f.rc;
                                }
                        return TRI_OK;
                }
                // one pass over the fragments: f.rc = fn(f) on the pool; `doing` completes "... while <doing>" of what an exception reports
                template <class Fn>
                int run_pass(const char *name, const char *doing, Fn &&fn) {
                        run([&](unsigned k) {
                                Frag &f = frags[k];
                                try {
                                        f.rc = fn(f);
                                } catch (const std::bad_alloc &) {
                                        f.rc = herr(f.err, TRI_ERR_NOMEM, "tri_batch_create: out of host memory while %s", doing);
                                } catch (...) {
                                        f.rc = herr(f.err, TRI_ERR_INVALID, "tri_batch_create: unexpected exception while %s", doing);
                                }
                        });
                        dbg.lap(name);
                        return first_error();
                }
        };

        // ---- which terms may get a plane: an indexed list of at least docs_cnt / plane_div documents, the longest lists first up to the
        //      scratch budget (a plane row is PL_PLANES bitmaps over the docID space)
        inline void eligible_planes(PlanState &S) {
                const HostIndex &ix = S.ix;
                const tri_options &opt = S.opt;
                S.P.plw = ((ix.max_doc >> 17) + 2u) * (SPAN_BITS / 32u); // whole bitmap windows (k_and_dense reads SPAN_WORDS at a time) + a spare one
                S.C.plw = S.P.plw;
                if (opt.planes && opt.plane_div && !ix.df_sorted.empty()) {
                        const uint64_t min_df = std::max<uint64_t>(1, ix.info.docs_cnt / opt.plane_div);
                        // df_sorted descends: the first rank whose list is too short
                        const size_t n = (size_t)(std::partition_point(ix.df_sorted.begin(), ix.df_sorted.end(), [&](uint32_t d) { return d && d >= min_df; }) - ix.df_sorted.begin());
                        const uint64_t row_bytes = (uint64_t)PL_PLANES * S.P.plw * 4;
                        S.C.n_ok = (uint32_t)std::min<uint64_t>(n, std::max<uint64_t>(1, opt.plane_max_bytes / std::max<uint64_t>(1, row_bytes)));
                }
        }

        // ---- fragments: contiguous ranges of the batch, a couple per thread (dealt out dynamically); their buffers come from the caller's
        //      cache of earlier plans' and go back to it (~PlanState)
        inline void take_fragments(PlanState &S, FragCache *cache) {
                const size_t nq = S.C.in.nq;
                const unsigned nthreads = S.pool ? std::min<unsigned>(S.pool->size(), (unsigned)std::max<size_t>(1, nq / 512)) : 1u;
                const size_t nfrag = nthreads <= 1 ? 1 : std::min<size_t>(2 * nthreads, std::max<size_t>(1, nq / 256));
                S.frags.resize(nfrag);
                S.cache = cache;
                for (size_t k = 0; k < nfrag; ++k) {
                        if (cache && k < cache->frags.size()) {
                                S.frags[k] = std::move(cache->frags[k]);
                                S.frags[k].recycle();
                        }
                        S.frags[k].q_lo = nq * k / nfrag;
                        S.frags[k].q_hi = nq * (k + 1) / nfrag;
                }
        }

        // ---- between the first two passes: what depends on the whole batch
        inline void settle_batch_knobs(PlanState &S) {
                const tri_options &opt = S.opt;
                const PlanEnv &env = S.env;
                Ctx &C = S.C;
                uint64_t onepass_queries = 0, fused_postings = 0, phrase_queries = 0;
                for (const Frag &f : S.frags) {
                        onepass_queries += f.onepass_queries;
                        fused_postings += f.fused_postings;
                        phrase_queries += f.phrase_queries;
                }
                // k_phrase's span is its longest task (a phrase candidate costs a walk into two or three lists' hits: a task of four windows of two head terms is 76 K
                // candidates, 1 - 2 ms) — a batch with few phrase queries per resident workgroup cuts their tasks finer; one with many has tasks enough to fill the tail and
                // keeps the cheaper large ones.  Measured (k_phrase ms at 1 / 2 / 4 / 8): cfg5's shard, 1 250 phrase queries: 2.05 / 1.13 / 0.64 / 0.64; cfg4, 16 384: 8.05 / 8.26 / 8.42 / 8.41
                C.phrase_task_div = opt.phrase_task_div ? opt.phrase_task_div : !phrase_queries ? 1 : phrase_queries <= 8ull * env.cus ? 4 : phrase_queries <= 16ull * env.cus ? 2 : 1;
                // k_planes: docID ranges per query.  A task has fixed costs (seed pass, end-of-task imbalance: about 140 us), the kernel's tail is its
                // longest tasks: two ranges when the batch brings ten or more tasks per resident workgroup anyway, three when it does not (measured,
                // cfg3's mix: 8192 queries 2 > 3 > 4; 3750 queries 6.5 / 5.9 / 6.2 ms for 2 / 3 / 4; 1024 queries 2.11 / 1.97 / 1.96)
                C.planes_split = opt.planes_split ? opt.planes_split : (2 * onepass_queries >= 4ull * (uint64_t)env.cus * env.plk_wgs_per_cu ? 2 : 3) /* (round 5: a task's tail is short now — two ranges from four tasks per resident workgroup on; cfg5's shard, ms: 2 -> 2.25, 3 -> 2.35, 4 -> 2.50) */;
                // one-pass tasks stage the query (slot map, score tables) once per task: the longer the task the better, as long as the batch still
                // cuts into a couple of tasks per workgroup the device holds (measured at cfg3: 512 K postings per task 55.4 ms, 1 M 51.1, 2 M 49.2,
                // 4 M 48.0, 8 M and more 47.1).  fused_task_cost = 0 (the default): sized from the batch; otherwise as given
                C.fused_task_cost = opt.fused_task_cost;
                if (!C.fused_task_cost) {
                        const uint64_t want_tasks = 2ull * (uint64_t)env.cus * env.fus_wgs_per_cu;
                        C.fused_task_cost = std::min<uint64_t>(8u << 20, std::max<uint64_t>(256u << 10, fused_postings / std::max<uint64_t>(1, want_tasks)));
                }
        }

        // ---- the fragments' places in the batch's arrays; sums; the batch's limits
        inline int place_fragments(PlanState &S) {
                BatchPlan &P = S.P;
                SectionCounts &n = S.n;
                const uint32_t n_ok = S.C.n_ok;
                uint64_t off = 0;
                S.benefit.assign(n_ok, 0), S.cand_row.assign(n_ok, 0);
                for (Frag &f : S.frags) {
                        f.b_plan = n.plan, f.b_qterms = n.qterms, f.b_sterms = n.sterms, f.b_phrases = n.phrases, f.b_pterms = n.pterms, f.b_tasks = n.tasks, f.b_fused = n.fused,
                        f.b_ptasks = n.ptasks, f.b_off = off, f.b_units = n.units, f.b_tree = n.tree, f.b_hidden = n.tree_hidden;
                        n.plan += f.tmp.size(), n.qterms += f.qterms.size(), n.sterms += f.sterms.size(), n.phrases += f.phrases.size(), n.pterms += f.pterms.size(),
                                n.tasks += f.tasks.size(), n.fused += f.fused.size(), n.ptasks += f.ptasks.size(), n.units += f.units.size(), n.tree += f.treepool.size(),
                                n.tree_hidden += f.n_hidden, off += f.off;
                        S.tree_terms.insert(S.tree_terms.end(), f.tree_terms.begin(), f.tree_terms.end());
                        P.merge(f);
                        for (uint32_t r = 0; r < n_ok; ++r)
                                S.benefit[r] += f.benefit[r], S.cand_row[r] += f.cand_row[r];
                        for (const size_t qi : f.left_out) { // a query shape the planner does not lower does not fail the batch: the query is left out (status
                                                             // TRI_ERR_UNSUPPORTED, no matches) and the caller keeps its CPU span for it
                                P.qstatus[qi] = TRI_ERR_UNSUPPORTED;
                                ++P.unsupported_queries;
                        }
                        if (!f.left_out.empty())
                                P.last_unsupported = f.err;
                }
                S.cand_queries_all = P.cand_queries + P.probe_queries;
                if (n.qterms > 0xfffffff0ull || n.sterms > 0xfffffff0ull || n.tasks > 0xfffffff0ull || n.pterms > 0xfffffff0ull)
                        return herr(S.err, TRI_ERR_UNSUPPORTED, "tri_batch_create: the batch exceeds 2^32 terms or tasks: split it");
                P.out_capacity = off;
                if (P.rich_wide_queries) // (default mode with wide-report queries: their side table and k_rich's own schedule — place_rich_wide)
                        n.rich_wide = n.plan, n.rich_sched = n.tasks;
                std::sort(S.tree_terms.begin(), S.tree_terms.end());
                S.tree_terms.erase(std::unique(S.tree_terms.begin(), S.tree_terms.end()), S.tree_terms.end());
                n.tree_terms = S.tree_terms.size();
                P.tree_scratch_bytes = ((uint64_t)n.tree_terms * PL_PLANES + n.tree_hidden + P.tree_queries) * P.plw * 4;
                if (P.tree_scratch_bytes > S.opt.tree_max_bytes)
                        return herr(S.err, TRI_ERR_NOMEM, "tri_batch_create: the batch's %llu tree queries need %llu bytes of bitmap scratch (%zu distinct term leaves, %zu phrase leaves; option tree_max_bytes = %llu): split the batch",
                                    (unsigned long long)P.tree_queries, (unsigned long long)P.tree_scratch_bytes, n.tree_terms, n.tree_hidden, (unsigned long long)S.opt.tree_max_bytes);
                return TRI_OK;
        }

        // ---- the planes that pay: rows in term order (deterministic), the uses pointed at them.  A term is chosen when the batch's uses repay
        //      one decode of its list (a one-pass slot counts a whole decode: always chosen).  Settles the three sections that exist only with planes
        //      or scores
        inline void choose_planes(PlanState &S) {
                const HostIndex &ix = S.ix;
                const uint32_t n_ok = S.C.n_ok;
                std::vector<uint32_t> rank_term(n_ok, UINT32_MAX); // df rank -> term, for the eligible ranks only (built lazily from the uses)
                std::vector<uint8_t> forced(n_ok, 0);
                for (const Frag &f : S.frags) {
                        for (const QUse &u : f.quses)
                                rank_term[ix.df_rank[u.term]] = u.term;
                        for (const QUse &u : f.suses)
                                rank_term[ix.df_rank[u.term]] = u.term;
                        for (const FUse &u : f.fuses)
                                rank_term[ix.df_rank[u.term]] = u.term, forced[ix.df_rank[u.term]] = 1;
                }
                for (uint32_t r = 0; r < n_ok; ++r)
                        if (rank_term[r] != UINT32_MAX && (forced[r] || S.benefit[r] * std::max<uint64_t>(1, S.opt.plane_amortize) >= ix.terms[rank_term[r]].documents))
                                S.chosen.push_back(rank_term[r]);
                std::sort(S.chosen.begin(), S.chosen.end());
                // a term's plane row is its DF RANK: the rows live with the INDEX (tri_index's plane cache: a head term is decoded into its planes the
                // first time any batch wants them and stays — the index does not change), so every batch addresses the same row for the same term
                S.row_of_rank.assign(n_ok, PL_NONE);
                for (const uint32_t term : S.chosen) {
                        S.row_of_rank[ix.df_rank[term]] = ix.df_rank[term];
                        S.P.plane_decoded_bytes += ix.docbytes[term];
                }
                S.P.plane_rows = n_ok;
                S.n.plane_terms = S.chosen.size();
                S.n.qplane = S.chosen.empty() ? 0 : S.n.qterms;
                S.n.splane = (S.chosen.empty() || !S.C.scored) ? 0 : S.n.sterms;
                S.n.sweights = S.C.scored ? S.n.sterms : 0;
        }

        // ---- k_and's tasks ordered by the plane row they probe ("k_and's queues", deal_cand_queues): where the probes are the kernel's traffic — conjunctions of two or
        //      three terms whose leads average a thousand documents or more (cfg2: 3.4 K).  Rare leads against four lists (cfg3 / cfg5: a few hundred
        //      candidates a task, several rows each) gain nothing from the order and lose the heaviest-first start: measured 0.49 -> 0.54 ms, 0.68 -> 0.72 ms
        inline void assign_cand_rows(PlanState &S) {
                const BatchPlan &P = S.P;
                const uint32_t n_ok = S.C.n_ok;
                const std::vector<uint64_t> &cand_row = S.cand_row;
                S.pset_ranges = ((S.ix.max_doc >> 17) + 1u + PSET_TASK_WINDOWS - 1) / PSET_TASK_WINDOWS;
                S.cand_rows = S.opt.cand_xcd && !S.chosen.empty() && S.cand_queries_all && P.cand_lead_docs >= CAND_ROWS_MIN_LEAD * S.cand_queries_all && P.cand_terms <= 3 * S.cand_queries_all;
                // row -> queue(s) and the row's place in the queue: heaviest row first to the least loaded queue (the rows are a few hundred); a row that outweighs
                // a 16th of the section is cut into pieces of that size, each placed on its own (a Zipf batch's first term is probed by a sixth of the tasks)
                S.rowq.assign(S.cand_rows ? n_ok : 0, RowQ{});
                if (S.cand_rows) {
                        uint64_t total = 0, load[CAND_QUEUES] = {};
                        uint32_t placed[CAND_QUEUES] = {};
                        std::vector<uint32_t> rows;
                        for (uint32_t r = 0; r < n_ok; ++r)
                                if (cand_row[r] && S.row_of_rank[r] != PL_NONE)
                                        rows.push_back(r), total += cand_row[r];
                        std::sort(rows.begin(), rows.end(), [&](uint32_t a, uint32_t b) { return cand_row[a] != cand_row[b] ? cand_row[a] > cand_row[b] : a < b; });
                        const uint64_t cap = std::max<uint64_t>(1, total / (2 * CAND_QUEUES));
                        for (const uint32_t r : rows) {
                                RowQ &z = S.rowq[r];
                                z.n = (uint8_t)std::min<uint64_t>(CAND_QUEUES, (cand_row[r] + cap - 1) / cap);
                                for (uint32_t k = 0; k < z.n; ++k) {
                                        const uint32_t x = (uint32_t)(std::min_element(load, load + CAND_QUEUES) - load);
                                        load[x] += cand_row[r] / z.n;
                                        z.q[k] = (uint8_t)x;
                                        z.sub[k] = (uint8_t)(CAND_COST_SUBS + placed[x]++ % (CAND_SUBS - CAND_COST_SUBS - 1));
                                }
                        }
                }
                if (S.dbg.on) {
                        char buf[96];
                        snprintf(buf, sizeof buf, " [cand queries %llu lead docs %llu terms %llu rows %d]", (unsigned long long)S.cand_queries_all, (unsigned long long)P.cand_lead_docs, (unsigned long long)P.cand_terms, (int)S.cand_rows);
                        S.dbg.line += buf;
                }
        }

        // ---- the host block: its sections laid out (for_each_section), allocated, the spans pointed into it, and what no fragment owns written
        inline int layout_block(PlanState &S, const std::function<uint8_t *(size_t)> &alloc_block) {
                BatchPlan &P = S.P;
                P.block_bytes = layout_sections(P, S.n);
                S.dbg.lap("sums+planes+layout");
                P.block = alloc_block(P.block_bytes);
                S.dbg.lap("alloc_block");
                if (!P.block)
                        return herr(S.err, TRI_ERR_NOMEM, "tri_batch_create: no host memory for the plan (%zu bytes)", P.block_bytes);
                point_sections(P, S.n);
                std::copy(S.tree_terms.begin(), S.tree_terms.end(), P.tree_terms.p);
                S.unit_of_task.assign(S.n.units ? S.n.tasks : 0, 0u);
                std::copy(S.chosen.begin(), S.chosen.end(), P.plane_terms.p);
                S.dbg.lap("spans");
                return TRI_OK;
        }

        // ---- a fragment writes its part of the batch's arrays, rebased; the plane rows of its uses; probe tasks whose planes were not chosen demoted
        inline int fill_fragment(PlanState &S, Frag &f) {
                const HostIndex &ix = S.ix;
                BatchPlan &P = S.P;
                const std::vector<uint32_t> &row_of_rank = S.row_of_rank;
                for (size_t i = 0; i < f.tmp.size(); ++i) {
                        DevQuery q = f.tmp[i].q;
                        q.term_base += (uint32_t)f.b_qterms;
                        q.score_base += (uint32_t)f.b_sterms;
                        q.phrase_base += (uint32_t)f.b_phrases;
                        q.first_task += (uint32_t)f.b_tasks;
                        q.out_off += f.b_off;
                        if (f.tmp[i].fuse)
                                q.fused_idx += (uint32_t)f.b_fused;
                        if (f.tmp[i].tree)
                                q.fused_idx += (uint32_t)f.b_tree;
                        if (f.tmp[i].hidden) { // (no caller query of its own: its matches are a leaf of a TASK_TREE query)
                                q.qid = 0xffffffffu;
                                P.tree_hidden[f.b_hidden + f.tmp[i].hidden_ord] = (uint32_t)(f.b_plan + i);
                        } else
                                P.slot_of_query[q.qid] = (uint32_t)(f.b_plan + i);
                        P.plan[f.b_plan + i] = q;
                }
                if (!f.treepool.empty()) {
                        memcpy(&P.tree[f.b_tree], f.treepool.data(), f.treepool.size() * 4);
                        for (size_t i = 0; i < f.tmp.size(); ++i) {
                                if (!f.tmp[i].tree)
                                        continue;
                                uint32_t *rec = &P.tree[f.b_tree + f.tmp[i].q.fused_idx];
                                DevTreeNode *tn = reinterpret_cast<DevTreeNode *>(rec + TREE_HDR_WORDS);
                                for (uint32_t k = 0; k < rec[0]; ++k)
                                        if (tn[k].op == TRI_OP_TERM)
                                                tn[k].row = (uint32_t)(std::lower_bound(P.tree_terms.begin(), P.tree_terms.end(), tn[k].arg) - P.tree_terms.begin());
                                        else if (tn[k].op == TRI_OP_PHRASE) {
                                                tn[k].arg += (uint32_t)f.b_plan;
                                                tn[k].row += (uint32_t)f.b_hidden;
                                        }
                        }
                }
                for (size_t i = 0; i < f.tasks.size(); ++i) {
                        DevTask t = f.tasks[i];
                        t.slot += (uint32_t)f.b_plan;
                        t.out_off += f.b_off;
                        P.tasks[f.b_tasks + i] = t;
                }
                if (!f.qterms.empty())
                        memcpy(&P.qterms[f.b_qterms], f.qterms.data(), f.qterms.size() * 4);
                if (!f.sterms.empty())
                        memcpy(&P.sterms[f.b_sterms], f.sterms.data(), f.sterms.size() * 4);
                if (S.C.scored && !f.sweights.empty())
                        memcpy(&P.sweights[f.b_sterms], f.sweights.data(), f.sweights.size() * 8);
                for (size_t i = 0; i < f.phrases.size(); ++i) {
                        DevPhrase ph = f.phrases[i];
                        ph.term_base += (uint32_t)f.b_pterms;
                        P.phrases[f.b_phrases + i] = ph;
                }
                if (!f.pterms.empty())
                        memcpy(&P.pterms[f.b_pterms], f.pterms.data(), f.pterms.size() * 4);
                for (size_t i = 0; i < f.ptasks.size(); ++i)
                        P.ptasks[f.b_ptasks + i] = f.ptasks[i] + (uint32_t)f.b_tasks;
                for (size_t i = 0; i < f.fused.size(); ++i)
                        P.fused[f.b_fused + i] = f.fused[i];
                for (const FUse &u : f.fuses)
                        P.fused[f.b_fused + u.fidx].plane[u.slot] = row_of_rank[ix.df_rank[u.term]];
                for (size_t i = 0; i < f.units.size(); ++i) {
                        DevPsetUnit u = f.units[i];
                        u.out_off += f.b_off;
                        u.tix += (uint32_t)f.b_tasks;
                        u.term_base += (uint32_t)f.b_qterms;
                        const bool is_probe = f.tasks[f.units[i].tix].kind == TASK_PROBE;
                        bool rows = true;
                        for (uint32_t k = is_probe ? 1u : 0u; k < u.nterms; ++k) { // (a TASK_PROBE unit's term 0 is the lead: decoded, never probed)
                                const uint32_t term = (k < PSET_INLINE_TERMS ? u.tt[k] : f.qterms[f.units[i].term_base + k]) & QT_TERM;
                                const uint32_t rank = ix.df_rank[term];
                                const uint32_t row = rank < row_of_rank.size() ? row_of_rank[rank] : PL_NONE; // (a PSET_UNIT_SCATTER union names terms without a plane)
                                rows &= row != PL_NONE;
                                if (k < PSET_INLINE_TERMS)
                                        u.row[k] = row;
                                if (row == PL_NONE && (u.first & PSET_UNIT_SCATTER) && u.w_begin == 0) // (a scatter union's first task: the documents k_psets_prep lists for the query)
                                        f.pscatter_docs += ix.terms[term].documents;
                        }
                        if (is_probe && !rows) { // a probed list did not get its plane (the batch's uses do not repay its decode): candidate tiles after all
                                P.tasks[u.tix].kind = TASK_CAND;
                                if (u.first & PSET_UNIT_FIRST) {
                                        ++f.probe_demoted;
                                        f.probe_demoted_bytes += distinct_docbytes(ix, &f.qterms[f.units[i].term_base], u.nterms, f.S.seen);
                                }
                        }
                        P.units[f.b_units + i] = u;
                        S.unit_of_task[u.tix] = (uint32_t)(f.b_units + i);
                }
                if (S.n.splane) {
                        std::fill(&P.splane.p[f.b_sterms], &P.splane.p[f.b_sterms] + f.sterms.size(), PL_NONE);
                        for (const QUse &u : f.suses)
                                P.splane[f.b_sterms + u.qpos] = row_of_rank[ix.df_rank[u.term]];
                }
                if (S.n.qplane) {
                        std::fill(&P.qplane.p[f.b_qterms], &P.qplane.p[f.b_qterms] + f.qterms.size(), PL_NONE);
                        for (const QUse &u : f.quses)
                                P.qplane[f.b_qterms + u.qpos] = row_of_rank[ix.df_rank[u.term]];
                }
                return TRI_OK;
        }

        // ---- schedule keys: one ordering per kind of task (task i of fragment f, as the fill pass left it in the plan)
        // (option planes_order: k_planes' tasks range by range, within a range by the heaviest plane row they sweep — the workgroups
        //  in flight then stream the same head rows from the same place: L2 instead of the fabric)
        inline uint32_t key_planes_order(const PlanState &S, const Frag &f, const size_t i, const DevTask &tk) {
                const DevQuery &q = S.P.plan[tk.slot];
                const DevFused &z = S.P.fused[q.fused_idx];
                uint32_t minrow = PL_NONE;
                for (uint32_t sidx = 0; sidx < z.nslots; ++sidx)
                        minrow = std::min(minrow, z.plane[sidx]);
                const uint32_t ord = (uint32_t)(f.b_tasks + i) - q.first_task, per = SCHED_NB / 4;
                return SCHED_RANK[tk.kind] * SCHED_NB + (S.opt.planes_order == 2 ? std::min(minrow, per - 1) * 4 + std::min(ord, 3u) : std::min(ord, 3u) * per + std::min(minrow, per - 1));
        }
        // (option pset_order: k_psets' tasks range by range, within a range by the query's heaviest term — the tasks in flight read ITS words of
        //  the range one after the other, the second reader on from L2)
        inline uint32_t key_pset_order(const PlanState &S, const Frag &f, const size_t i) {
                const uint32_t range = (uint32_t)(f.tcost[i] & 0xffffffffull) / PSET_TASK_WINDOWS;
                const uint32_t rb = S.pset_ranges <= PSET_RANGE_BKS ? std::min(range, PSET_RANGE_BKS - 1) : (uint32_t)std::min<uint64_t>((uint64_t)range * PSET_RANGE_BKS / S.pset_ranges, PSET_RANGE_BKS - 1);
                return PSET_KEY0 + rb * PSET_SUBS + pset_sub((uint32_t)(f.tcost[i] >> 32));
        }
        // k_and's queues (deal_cand_queues): the XCD's queue and the place in it by the plane row the task probes first
        inline uint32_t key_cand_rows(const PlanState &S, const Frag &f, const size_t i, const DevTask &tk) {
                const DevQuery &q = S.P.plan[tk.slot];
                uint32_t row = PL_NONE;
                for (uint32_t k = 1; k < q.nterms && row == PL_NONE; ++k)
                        row = S.P.qplane[q.term_base + k];
                uint32_t queue, sub;
                if (tk.tile_end - tk.tile_begin > CAND_HEAVY_TILES || row == PL_NONE)
                        // the long tasks, and the ones that gallop through every list (100 us and more where a probing task takes 20): first, dealt
                        // round the queues, heaviest first — left to the end they were the kernel's tail (a tenth of its span on a tenth of the workgroups)
                        queue = (uint32_t)(f.b_tasks + i) % CAND_QUEUES, sub = (sched_key(TASK_CAND, f.tcost[i]) % SCHED_NB) / (SCHED_NB / CAND_COST_SUBS);
                else if (row < S.rowq.size() && S.rowq[row].n) {
                        const RowQ &z = S.rowq[row];
                        const uint32_t piece = (uint32_t)(f.b_tasks + i) % z.n;
                        queue = z.q[piece], sub = z.sub[piece];
                } else // (a row the tally of assign_cand_rows did not see: a demoted probe task's)
                        queue = row % CAND_QUEUES, sub = CAND_SUBS - 1;
                return CAND_KEY0 + queue * CAND_SUBS + sub;
        }
        inline uint32_t schedule_key(const PlanState &S, const Frag &f, const size_t i) {
                const DevTask &tk = S.P.tasks[f.b_tasks + i]; // (the kinds are final: a probe task whose planes were not chosen is a candidate-tile task by now)
                switch (tk.kind) {
                        case TASK_PLANES:
                        case TASK_PLANES8:
                                if (S.opt.planes_order)
                                        return key_planes_order(S, f, i, tk);
                                break;
                        case TASK_PSET:
                                if (S.opt.pset_order)
                                        return key_pset_order(S, f, i);
                                break;
                        case TASK_CAND:
                                if (S.cand_rows)
                                        return key_cand_rows(S, f, i, tk);
                                break;
                }
                return sched_key(tk.kind, f.tcost[i]); // heaviest first
        }
        // ... per task of the fragment its bucket, and the fragment's tasks per bucket
        inline int key_fragment(const PlanState &S, Frag &f) {
                f.keys.resize(f.tasks.size());
                f.hist.assign(SCHED_KEYS, 0u);
                for (size_t i = 0; i < f.tasks.size(); ++i)
                        ++f.hist[f.keys[i] = schedule_key(S, f, i)];
                return TRI_OK;
        }

        // ---- the schedule: per kernel, heaviest tasks first.  A counting sort by (kernel, cost octave + 2 bits) — tasks within a fifth of each
        //      other keep their order in the batch: all a longest-first dispatch needs; TASK_PSET goes by docID window range instead.  The
        //      fragments counted their tasks per bucket (key_fragment); their places are settled here, the scatter runs on the pool again
        inline void place_schedule(PlanState &S) {
                BatchPlan &P = S.P;
                uint32_t at = 0;
                for (uint32_t r = 0; r < TASK_KINDS; ++r) {
                        const uint32_t before = at;
                        if (r == SCHED_RANK[TASK_CAND])
                                S.cand_first = at;
                        auto place = [&](const uint32_t bk) {
                                for (Frag &f : S.frags) {
                                        const uint32_t c = f.hist[bk];
                                        f.hist[bk] = at; // (count -> the fragment's first place in the bucket)
                                        at += c;
                                }
                        };
                        for (uint32_t bk = r * SCHED_NB; bk < (r + 1) * SCHED_NB; ++bk)
                                place(bk);
                        if (r == SCHED_RANK[TASK_PSET] && S.opt.pset_order) // (k_psets' tasks by range and heaviest term)
                                for (uint32_t bk = PSET_KEY0; bk < PSET_KEY0 + std::min(S.pset_ranges, PSET_RANGE_BKS) * PSET_SUBS; ++bk)
                                        place(bk);
                        if (r == SCHED_RANK[TASK_CAND]) // (a `cand_rows` batch: k_and's tasks are all in the row buckets)
                                for (uint32_t bk = CAND_KEY0; bk < PSET_KEY0; ++bk) {
                                        if ((bk - CAND_KEY0) % CAND_SUBS == 0)
                                                S.cand_qat[(bk - CAND_KEY0) / CAND_SUBS] = at;
                                        place(bk);
                                }
                        for (uint32_t k = 0; k < TASK_KINDS; ++k)
                                if (SCHED_RANK[k] == r)
                                        P.*SCHED_COUNT[k] = at - before;
                }
                const uint32_t units_first = sched_first(P, TASK_PSET), n_units_run = P.n_pset + P.n_probe;
                S.run([&](unsigned k) {
                        Frag &f = S.frags[k];
                        for (size_t i = 0; i < f.tasks.size(); ++i) {
                                const uint32_t pos = f.hist[f.keys[i]]++, ti = (uint32_t)(f.b_tasks + i);
                                P.sched[pos] = ti;
                                if (pos >= units_first && pos - units_first < n_units_run) // (a TASK_PSET / TASK_PROBE task: its unit record runs at the same place)
                                        P.pset_sched[pos - units_first] = S.unit_of_task[ti];
                        }
                });
        }

        // ---- the TASK_TREE section: the queries with narrow records first, the wide ones (k_tree_wide.hpp) last, each part in the order the schedule gave it — the
        //      narrow kernels are never handed a wide record (tree_load would clamp it to its first 64 nodes).  A batch without wide records: nothing moves
        inline void split_tree_section(BatchPlan &P) {
                if (!P.n_tree)
                        return;
                uint32_t *const ts = P.sched.p + sched_first(P, TASK_TREE);
                auto narrow = [&](const uint32_t ti) { return P.tree[P.plan[P.tasks[ti].slot].fused_idx + 1] != TREE_KIND_WIDE; };
                P.n_tree_wide = P.n_tree - (uint32_t)std::count_if(ts, ts + P.n_tree, narrow);
                if (P.n_tree_wide && P.n_tree_wide < P.n_tree)
                        std::stable_partition(ts, ts + P.n_tree, narrow);
        }

        // ---- default mode with wide-report queries (option rich_max_terms): the side table — per plan slot where the query's frequency rows (stride = nscore
        //      rounded up to 8 cells: 16-byte rows) and high mask words lie, query after query in plan order, nothing for the other queries — and k_rich's own
        //      schedule: sched's order, the wide-report queries' tasks moved behind everything else (the wide instantiation's launch)
        inline void place_rich_wide(BatchPlan &P) {
                if (P.rich_wide.empty())
                        return;
                uint64_t cells = 0, slots = 0;
                for (size_t i = 0; i < P.plan.size(); ++i) {
                        const DevQuery &q = P.plan[i];
                        DevRichWide w{};
                        if (q.nscore > RICH_NARROW_TERMS) {
                                w.cells = cells, w.slots = slots, w.stride = (q.nscore + 7u) & ~7u;
                                cells += (uint64_t)q.out_cap * w.stride, slots += q.out_cap;
                                P.n_rich_wide += q.ntasks;
                        }
                        P.rich_wide[i] = w;
                }
                P.rich_wide_cells = cells, P.rich_wide_slots = slots;
                std::copy(P.sched.begin(), P.sched.end(), P.rich_sched.begin());
                std::stable_partition(P.rich_sched.begin(), P.rich_sched.end(), [&](const uint32_t ti) { return P.rich_wide[P.tasks[ti].slot].stride == 0; });
        }

        // ---- k_and's queues.  A candidate tile probes the planes of the query's other terms: ONE bit per candidate, a 64-byte sector of a 1.25 MB row
        //      each — in cost order the tasks in flight probe a hundred rows at once and every sector comes from HBM (cfg2: 2.9 GB per step of them).
        //      The section is cut into one queue per XCD (workgroups draw from the queue of the XCD they run on, and from the next ones when theirs is
        //      empty).  A batch of few-term conjunctions with long leads (`cand_rows`) orders a queue BY THE ROW ITS TASKS PROBE, every row in ONE
        //      queue (key_cand_rows; the counting sort placed them): an XCD works through a couple of rows at a time, its 4 MB L2 keeps their sectors
        //      for the row's next tasks — k_and reads 0.76 GB (PMC, profiles/README.md).  Any other batch: the cost order, dealt round the queues
        inline void deal_cand_queues(PlanState &S) {
                BatchPlan &P = S.P;
                const uint32_t nc = P.n_cand;
                uint32_t *const sc = P.sched.p + S.cand_first;
                if (S.cand_rows) {
                        for (uint32_t x = 0; x <= CAND_QUEUES; ++x)
                                P.cand_q[x] = x < CAND_QUEUES ? S.cand_qat[x] - S.cand_first : nc;
                } else {
                        const std::vector<uint32_t> was(sc, sc + nc);
                        uint32_t pos = 0;
                        for (uint32_t x = 0; x < CAND_QUEUES; ++x) {
                                P.cand_q[x] = pos;
                                for (uint32_t i = x; i < nc; i += CAND_QUEUES)
                                        sc[pos++] = was[i];
                        }
                        P.cand_q[CAND_QUEUES] = pos;
                }
        }

        // ---- k_phrase's tasks, heaviest first: a task's candidates are bounded by its output region (the lead's documents in its range); in query
        //      order the 4 ms tasks of a head x head phrase started anywhere in the kernel's span and its last fifth ran on a tenth of the
        //      workgroups (cfg4: 70 % busy).  A counting sort by the region's size (octave + 2 bits), descending, stable
        inline void order_phrase_tasks(BatchPlan &P) {
                if (P.ptasks.size() <= 1)
                        return;
                const size_t np = P.ptasks.size();
                std::vector<uint32_t> key(np), sorted(np);
                uint32_t hist[SCHED_NB + 1] = {};
                for (size_t i = 0; i < np; ++i) {
                        const uint32_t ti = P.ptasks[i];
                        const DevTask &tk = P.tasks[ti];
                        const DevQuery &q = P.plan[tk.slot];
                        const uint64_t end = ti + 1 < q.first_task + q.ntasks ? P.tasks[ti + 1].out_off : q.out_off + q.out_cap;
                        key[i] = SCHED_NB - 1 - cost_bucket(end - tk.out_off);
                        ++hist[key[i] + 1];
                }
                for (uint32_t bk = 0; bk < SCHED_NB; ++bk)
                        hist[bk + 1] += hist[bk];
                for (size_t i = 0; i < np; ++i)
                        sorted[hist[key[i]]++] = P.ptasks[i];
                std::copy(sorted.begin(), sorted.end(), P.ptasks.p);
        }

        // ---- (option account_needed_bytes, a diagnostic) BatchPlan::distinct_bytes: one pass over the plan with a mark per term and class
        inline void account_distinct_bytes(const HostIndex &ix, const Ctx &C, BatchPlan &P) {
                std::vector<uint8_t> seen(ix.terms.size(), 0); // bit k: counted for kind k; bit 7: counted for the batch
                std::vector<uint8_t> seen_hits(ix.terms.size(), 0);
                for (size_t sidx = 0; sidx < P.plan.size(); ++sidx) {
                        const DevQuery &q = P.plan[sidx];
                        const uint32_t kind = P.tasks[q.first_task].kind;
                        auto touch = [&](uint32_t term) {
                                if (!(seen[term] & 0x80u))
                                        P.distinct_bytes += ix.docbytes[term];
                                if (!(seen[term] & (1u << kind)))
                                        P.distinct_bytes_kind[kind] += ix.docbytes[term];
                                seen[term] |= (uint8_t)(0x80u | (1u << kind));
                        };
                        if (kind == TASK_TREE) {
                                const uint32_t *rec = &P.tree[q.fused_idx];
                                const DevTreeNode *tn = reinterpret_cast<const DevTreeNode *>(rec + TREE_HDR_WORDS);
                                for (uint32_t k = 0; k < rec[0]; ++k)
                                        if (tn[k].op == TRI_OP_TERM)
                                                touch(tn[k].arg);
                        } else if (task_onepass(kind)) {
                                const DevFused &z = P.fused[q.fused_idx];
                                for (uint32_t k = 0; k < z.nslots; ++k)
                                        touch(z.term[k]);
                        } else {
                                for (uint32_t k = 0; k < q.nterms; ++k)
                                        touch(P.qterms[q.term_base + k] & QT_TERM);
                                if (C.mode != TRI_FLAG_DOCUMENTS_ONLY) // (k_score / k_rich read the scorer / reported terms' lists)
                                        for (uint32_t k = 0; k < q.nscore; ++k)
                                                touch(P.sterms[q.score_base + k]);
                        }
                        auto touch_hits = [&](uint32_t term, bool phrase) {
                                if (!(seen_hits[term] & 1u))
                                        P.distinct_bytes += ix.hitbytes[term];
                                if (phrase && !(seen_hits[term] & 2u))
                                        P.distinct_bytes_kind[TASK_KINDS] += ix.hitbytes[term];
                                seen_hits[term] |= (uint8_t)(1u | (phrase ? 2u : 0u));
                        };
                        for (uint32_t ph = 0; ph < q.nphrases; ++ph)
                                for (uint32_t k = 0; k < P.phrases[q.phrase_base + ph].nterms; ++k)
                                        touch_hits(P.pterms[P.phrases[q.phrase_base + ph].term_base + k], true);
                        if (C.rich)
                                for (uint32_t k = 0; k < q.nscore; ++k)
                                        touch_hits(P.sterms[q.score_base + k], false);
                }
        }
} // namespace trip

// Plan a batch.  `alloc_block(bytes)` provides the host block the plan's arrays are laid out in (pinned memory when a device will copy
// it; it must stay valid as long as the plan is used, and is 64-byte aligned); `pool` may be null (everything on the calling thread).
// Returns TRI_OK, or an error code with its text in `err` (a query shape the planner does not lower is NOT an error: BatchPlan::qstatus).
inline int plan_batch(const HostIndex &ix, const PlanEnv &env, const PlanInput &in, HostPool *pool, const std::function<uint8_t *(size_t)> &alloc_block,
                      BatchPlan &P, std::string &err, trip::FragCache *frag_cache = nullptr) {
        using namespace trip;
        auto t0 = std::chrono::steady_clock::now();
        static const bool dbg_plan = getenv("TRINITY_DEBUG_PLAN") != nullptr;
        const uint32_t mode = in.flags & (TRI_FLAG_DOCUMENTS_ONLY | TRI_FLAG_ACCUMULATED_SCORE | TRI_FLAG_MATCHED_TERMS);
        PlanState S{ix, env, env.opt, pool, P, err, Ctx{ix, env, in, mode == TRI_FLAG_ACCUMULATED_SCORE, mode == TRI_FLAG_MATCHED_TERMS, mode}, LapTimer{dbg_plan}};
        if (env.opt.tree_max_nodes < TREE_MAX_NODES || env.opt.tree_max_nodes > TREE_WIDE_MAX_NODES)
                return herr(err, TRI_ERR_INVALID, "tri_batch_create: option tree_max_nodes = %llu (%u .. %u)", (unsigned long long)env.opt.tree_max_nodes, TREE_MAX_NODES, TREE_WIDE_MAX_NODES);
        if (env.opt.rich_max_terms < RICH_NARROW_TERMS || env.opt.rich_max_terms > RICH_WIDE_TERMS)
                return herr(err, TRI_ERR_INVALID, "tri_batch_create: option rich_max_terms = %llu (%u .. %u)", (unsigned long long)env.opt.rich_max_terms, RICH_NARROW_TERMS, RICH_WIDE_TERMS);
        P.slot_of_query.assign(in.nq, UINT32_MAX);
        P.qstatus.assign(in.nq, TRI_OK);
        eligible_planes(S);
        take_fragments(S, frag_cache);
        S.dbg.lap("setup");
        if (const int rc = S.run_pass("LOWER", "lowering the batch", [&](Frag &f) { return lower_range(S.C, f); }))
                return rc;
        settle_batch_knobs(S);
        S.dbg.lap("glue0");
        P.plan_ms[0] = ms_since(t0);
        if (const int rc = S.run_pass("TASKS", "cutting the batch into tasks", [&](Frag &f) { return task_range(S.C, f); }))
                return rc;
        P.plan_ms[1] = ms_since(t0);
        if (const int rc = place_fragments(S))
                return rc;
        choose_planes(S);
        assign_cand_rows(S);
        if (const int rc = layout_block(S, alloc_block))
                return rc;
        if (const int rc = S.run_pass("FILL", "filling the plan", [&](Frag &f) {
                    fill_fragment(S, f);
                    return key_fragment(S, f);
            }))
                return rc;
        for (const Frag &f : S.frags) { // (what the fill pass sent back to the candidate tiles)
                P.pscatter_docs += f.pscatter_docs;
                P.probe_queries -= f.probe_demoted, P.cand_queries += f.probe_demoted;
                P.term_bytes_probe -= f.probe_demoted_bytes;
        }
        P.plan_ms[2] = ms_since(t0);
        place_schedule(S);
        deal_cand_queues(S);
        split_tree_section(P);
        place_rich_wide(P);
        order_phrase_tasks(P);
        P.sparse_cap = (P.sparse_cap + 63u) & ~63u;
        S.dbg.lap("sched+rest");
        if (dbg_plan)
                fprintf(stderr, "[tri plan] nq %zu frags %zu:%s\n", in.nq, S.frags.size(), S.dbg.line.c_str());
        P.plan_ms[3] = ms_since(t0);
        if (env.opt.account_needed_bytes && !ix.terms.empty())
                account_distinct_bytes(ix, S.C, P);
        return TRI_OK;
}

// planner_tasks.hpp — the planner's second pass (planner.hpp): a fragment's lowered queries cut into tasks of even cost with private output
// regions — one function per outcome (tree, one-pass windows, bitmap / plane-set windows, candidate / probe tiles) behind a short dispatcher —
// and the uses of term planes tallied for the choice of planes.  Host-only C++17, no HIP.  New code, no reference source.
#pragma once
#include "planner_types.hpp"

namespace trip {
        // TASK_TREE: one task — its chunks of the docID space are the kernels' grid, its region the bound of the tree's matches
        inline void tasks_tree(const Ctx &C, Frag &f, Tmp &t, const uint32_t slot, uint64_t &off) {
                t.q.out_off = off;
                t.q.out_cap = (uint32_t)t.tree_ub;
                t.q.first_task = (uint32_t)f.tasks.size();
                t.q.ntasks = 1;
                f.tcost.push_back(std::max<uint64_t>(1, t.tree_ub));
                f.tasks.push_back({slot, 0, (C.plw + TREE_CHUNK_WORDS - 1) / TREE_CHUNK_WORDS, TASK_TREE, off});
                off += t.q.out_cap;
                ++f.tree_queries;
        }

        // one pass over scored windows (k_fused), or — a CNF query whose top-K runs over bit planes (k_planes) — its head terms read from the
        // batch's term planes, the others (at most PLK_MAX_SPARSE) decoded per window into LDS planes
        inline int tasks_onepass(const Ctx &C, Frag &f, Tmp &t, const uint32_t slot, uint64_t &off) {
                const HostIndex &ix = C.ix;
                DevFused z = f.fz[t.fz];
                uint32_t nsparse = 0;
                for (uint32_t sidx = 0; sidx < z.nslots; ++sidx) {
                        z.plane[sidx] = PL_NONE;
                        nsparse += C.plane_ok(z.term[sidx]) ? 0u : 1u;
                }
                const bool pk = !t.truth && (C.env.opt.planes & 4u) && nsparse <= PLK_MAX_SPARSE && ix.max_doc < 0x7fff0000u; // (list entries are docID << 1 | flag)
                {
                        const uint32_t fm = (1u << z.fbits) - 1u;
                        z.negslots = 0;
                        for (uint32_t sidx = 0; sidx < z.nslots; ++sidx)
                                if ((z.nmask >> (sidx * z.fbits)) & fm)
                                        z.negslots |= 1u << sidx;
                }
                // every list of the slot map is read once (the optional terms too)
                uint64_t slotdf = 0;
                for (uint32_t sidx = 0; sidx < z.nslots; ++sidx) {
                        slotdf += ix.terms[z.term[sidx]].documents;
                        (pk ? f.term_bytes_planes : f.term_bytes_fused) += ix.docbytes[z.term[sidx]];
                        if (pk && C.plane_ok(z.term[sidx])) {
                                f.benefit[ix.df_rank[z.term[sidx]]] += ix.terms[z.term[sidx]].documents;
                                f.fuses.push_back({(uint32_t)f.fused.size(), sidx, z.term[sidx]});
                        }
                }
                ++(pk ? f.planes_queries : f.fused_queries);
                t.q.fused_idx = (uint32_t)f.fused.size();
                t.q.out_off = off;
                t.q.out_cap = 0; // the docID set is never materialised ...
                t.q.first_task = (uint32_t)f.tasks.size();
                const uint32_t fw = pk ? PL_W : FUS_W << z.hw; // documents per window: plane windows, or this query's word width
                const uint32_t nwin = t.last_doc / fw + 1;
                const uint64_t per_win = std::max<uint64_t>(1, slotdf / (ix.info.docs_cnt / fw + 1));
                // (k_planes' cost is the sweep of the range plus its candidates, not the postings: equal ranges, a few per query)
                const uint32_t win_per_task = pk && C.planes_split < 65536 ? (uint32_t)((nwin + C.planes_split - 1) / C.planes_split)
                                                                           : (uint32_t)std::max<uint64_t>(1, C.fused_task_cost / per_win);
                const bool emit = z.mode & FUS_MODE_EMIT; // ... except by a general tree in DocumentsOnly mode: a private region per task,
                                                          // bounded like TASK_DENSE's by the slots' blocks that reach the task's windows
                uint32_t ord = 0;
                for (uint32_t wb = 0; wb < nwin; wb += win_per_task, ++ord) {
                        const uint32_t we = std::min(nwin, wb + win_per_task);
                        uint64_t b1 = 0;
                        if (emit)
                                for (uint32_t sidx = 0; sidx < z.nslots; ++sidx)
                                        b1 += C.first_block_ge(ix.terms[z.term[sidx]], (uint64_t)wb * fw);
                        uint64_t entries = 0;
                        if (pk) { // the rows of the decoded slots that can reach the task's docID range: 32 list entries each (k_planes)
                                for (uint32_t sidx = 0; sidx < z.nslots; ++sidx) {
                                        if (C.plane_ok(z.term[sidx]))
                                                continue;
                                        const DevTerm &tk = ix.terms[z.term[sidx]];
                                        const uint32_t r0 = C.first_block_ge(tk, (uint64_t)wb * fw);
                                        const uint32_t r1 = C.first_block_ge(tk, (uint64_t)we * fw);
                                        if (r0 < tk.nblocks)
                                                entries += 32ull * (std::min(r1, tk.nblocks - 1) - r0 + 1);
                                }
                                if (entries > 0x7fffffffull)
                                        return herr(f.err, TRI_ERR_UNSUPPORTED, "query %u: a task's decoded lists exceed 2^31 entries", t.q.qid);
                                f.sparse_cap = std::max(f.sparse_cap, (uint32_t)entries);
                        }
                        // (largest first, by postings: for k_planes a poor estimate — its cost is the sweep plus the candidates — but ordering by the
                        //  decoded entries instead measured worse: cfg3's unions 10.6 ms against 9.2)
                        f.tcost.push_back(per_win * (we - wb));
                        f.tasks.push_back({slot, wb, we, pk ? (z.nslots <= PLK_NS_SMALL ? TASK_PLANES : TASK_PLANES8) : z.mode ? TASK_FUSED_GEN : z.hw ? TASK_FUSED16 : TASK_FUSED,
                                           off + (emit ? b1 * 32 + 32ull * ord * z.nslots : 0)});
                }
                if (emit) {
                        uint64_t blocks = 0;
                        for (uint32_t sidx = 0; sidx < z.nslots; ++sidx)
                                blocks += ix.terms[z.term[sidx]].nblocks;
                        t.q.out_cap = (uint32_t)std::min<uint64_t>(0xffffffffull, blocks * 32 + 32ull * (ord + 1) * z.nslots);
                        off += t.q.out_cap;
                }
                t.q.ntasks = (uint32_t)f.tasks.size() - t.q.first_task;
                f.fused.push_back(z);
                return TRI_OK;
        }

        // how a CNF query that is not run in one pass runs
        struct Route {
                bool pset = false;     // every term has a plane: its windows are word-wise algebra over the planes (k_psets)
                bool pscatter = false; // ... a union of head terms AND others whose result is a bitmap anyway (PSET_UNIT_SCATTER)
                bool probe = false;    // a short lead against lists that all have planes: k_probe (option probe_max_blocks)
        };
        // decides it (t.dense: bitmap / plane-set windows; else candidate / probe tiles) and tallies the query's bytes and its uses of term planes
        inline Route route_cnf(const Ctx &C, Frag &f, Tmp &t, const uint32_t *qt) {
                const HostIndex &ix = C.ix;
                const tri_options &opt = C.env.opt;
                const uint64_t planes_opt = opt.planes;
                const DevTerm &lead = ix.terms[qt[0] & QT_TERM];
                Route r;
                // every term of a bitmap-window query has a plane (a use as a window operand repays the decode by itself: such a term is
                // always chosen): the query's windows are word-wise algebra over the planes — its own kernel (k_psets.hpp)
                r.pset = t.dense && (planes_opt & 2u);
                for (uint32_t k = 0; r.pset && k < t.q.nterms; ++k)
                        r.pset = C.plane_ok(qt[k] & QT_TERM);
                // ... and a DocumentsOnly UNION (one group, nothing excluded) of head terms AND others whose result is a bitmap anyway (the head terms alone match
                // one document in 32 or more): the head terms' plane words are OR-ed and stored like any other k_psets window, the other terms' few
                // documents are then set in the stored words one by one (PSET_UNIT_SCATTER) — where k_and_dense decodes every list into an LDS window
                // bitmap behind half a dozen barriers per window (cfg5's 5-way unions: 2.5 of the shard's 8.9 ms)
                if (t.dense && !r.pset && (planes_opt & 2u) && C.mode == TRI_FLAG_DOCUMENTS_ONLY && opt.result_bitmaps && !t.q.nphrases && t.q.nterms >= 2) {
                        uint64_t plane_df = 0;
                        bool one_group = true;
                        for (uint32_t k = 0; k < t.q.nterms; ++k) {
                                one_group = one_group && !(qt[k] & QT_NOT) && (k == 0) == ((qt[k] & QT_GROUP) != 0);
                                if (C.plane_ok(qt[k] & QT_TERM))
                                        plane_df += ix.terms[qt[k] & QT_TERM].documents;
                        }
                        const uint32_t nwin = t.last_doc / SPAN_BITS + 1;
                        // (the result's form is decided below the same way on ALL the terms — min(N, sum of their documents) against the bitmap's words —: what
                        //  holds for the head terms alone holds for all of them, so a scatter union's result IS a bitmap)
                        const double N = std::max<double>(1.0, (double)ix.info.docs_cnt);
                        // (option scatter_bitmap_slack: such a union is run this way — and its result kept as a bitmap — from 1 / (32 x slack) of the documents on)
                        // (k_psets_prep counts such a query's documents per task in PSCAT_MAX_TASKS LDS counters: a union whose range needs more tasks — its last
                        //  document at or past 2^31 — is not run this way; it stays a bitmap-window query of k_and_dense)
                        const bool fits = (nwin + PSET_TASK_WINDOWS - 1) / PSET_TASK_WINDOWS <= PSCAT_MAX_TASKS && (uint64_t)nwin * SPAN_BITS < (1ull << 32); // (... and its nbits = out_cap * 32 is a 32-bit product)
                        r.pscatter = fits && one_group && plane_df && std::min<double>(N, (double)plane_df) * (double)std::max<uint64_t>(1, opt.scatter_bitmap_slack) >= (double)nwin * SPAN_WORDS;
                        r.pset = r.pscatter;
                }
                // a single lead list too short for a plane against lists that all have one: candidate tiles, every candidate tested with one
                // bit probe per list (k_and) — the bitmap kernel would decode the lead into an LDS window bitmap and expand the window
                // workgroup-wide for a handful of matches per window (cfg2: 253 such queries took 0.57 ms there, a third of the dense class's time)
                if (t.dense && !r.pset && t.nlead == 1 && (planes_opt & 1u) && !C.plane_ok(qt[0] & QT_TERM) && t.q.nterms >= 2) {
                        bool probes = true;
                        for (uint32_t k = 1; probes && k < t.q.nterms; ++k)
                                probes = C.plane_ok(qt[k] & QT_TERM);
                        if (probes)
                                t.dense = false;
                }
                if (t.dense) {
                        (r.pset ? f.term_bytes_pset : f.term_bytes_dense) += distinct_docbytes(ix, qt, t.q.nterms, f.S.seen);
                        for (uint32_t k = 0; k < t.q.nterms; ++k) {
                                const uint32_t term = qt[k] & QT_TERM;
                                if ((planes_opt & 2u) && C.plane_ok(term)) {
                                        f.benefit[ix.df_rank[term]] += ix.terms[term].documents;
                                        f.quses.push_back({t.q.term_base + k, term});
                                }
                        }
                        ++(r.pset ? f.pset_queries : f.dense_queries);
                } else {
                        // one lead list against lists that are all long enough for a plane: should the batch's uses repay every one of those
                        // planes (settled once the whole batch is known: the fill pass), the task runs in k_probe, else as candidate tiles
                        r.probe = t.nlead == 1 && t.q.nterms >= 2 && t.q.nphrases == 0 && (planes_opt & 1u) && lead.nblocks <= opt.probe_max_blocks;
                        for (uint32_t k = 1; r.probe && k < t.q.nterms; ++k)
                                r.probe = C.plane_ok(qt[k] & QT_TERM);
                        ++(r.probe ? f.probe_queries : f.cand_queries);
                        f.cand_lead_docs += lead.documents, f.cand_terms += t.q.nterms;
                        if (r.probe)
                                f.term_bytes_probe += distinct_docbytes(ix, qt, t.q.nterms, f.S.seen);
                        bool first_row = !r.probe;
                        for (uint32_t k = 1; k < t.q.nterms; ++k) { // (the lead list is decoded into the candidate tiles; the others are probed)
                                const uint32_t term = qt[k] & QT_TERM;
                                if ((planes_opt & 1u) && C.plane_ok(term)) {
                                        f.benefit[ix.df_rank[term]] += std::min<uint64_t>(ix.terms[term].documents, 32ull * lead.documents);
                                        f.quses.push_back({t.q.term_base + k, term});
                                        if (first_row) { // (k_and's queues: what the row's tasks will weigh)
                                                const uint32_t ntiles = (lead.nblocks + TILE_BLOCKS - 1) / TILE_BLOCKS;
                                                f.cand_row[ix.df_rank[term]] += ntiles + (ntiles + CAND_HEAVY_TILES - 1) / CAND_HEAVY_TILES;
                                                first_row = false;
                                        }
                                }
                        }
                }
                if (C.scored && (planes_opt & 1u)) // k_score: a scorer whose term has a plane reads the match's frequency off the planes
                        for (uint32_t k = 0; k < t.q.nscore; ++k) {
                                const uint32_t term = f.sterms[t.q.score_base + k];
                                if (C.plane_ok(term)) {
                                        f.benefit[ix.df_rank[term]] += std::min<uint64_t>(ix.terms[term].documents, 32ull * t.lead_docs);
                                        f.suses.push_back({t.q.score_base + k, term});
                                }
                        }
                return r;
        }

        // bitmap windows (TASK_DENSE) or plane-set windows (TASK_PSET, with their unit records); sets the query's region
        inline int tasks_windows(const Ctx &C, Frag &f, Tmp &t, const uint32_t slot, const uint32_t *qt, const Route r, const uint64_t off) {
                const HostIndex &ix = C.ix;
                const tri_options &opt = C.env.opt;
                const uint32_t nlead = t.nlead;
                const bool pset = r.pset, pscatter = r.pscatter;
                const uint32_t nwin = t.last_doc / SPAN_BITS + 1;
                // the result's form: a bitmap over the query's docID range when the matches to expect — the lead group's documents, thinned
                // by every further required group as if the lists were independent — outnumber the bitmap's words
                bool bitmap = false;
                double est = 1.0; // the share of the documents expected to match
                if (pset || (C.mode == TRI_FLAG_DOCUMENTS_ONLY && opt.result_bitmaps && !t.q.nphrases)) {
                        const double N = std::max<double>(1.0, (double)ix.info.docs_cnt);
                        double g = 0.0;
                        bool negg = false;
                        for (uint32_t k = 0; k <= t.q.nterms; ++k) {
                                if (k == t.q.nterms || (k && (qt[k] & QT_GROUP))) {
                                        if (!negg)
                                                est *= std::min(1.0, g / N);
                                        g = 0.0;
                                }
                                if (k == t.q.nterms)
                                        break;
                                if (qt[k] & QT_GROUP)
                                        negg = qt[k] & QT_NOT;
                                g += ix.terms[qt[k] & QT_TERM].documents;
                        }
                        bitmap = C.mode == TRI_FLAG_DOCUMENTS_ONLY && opt.result_bitmaps && !t.q.nphrases && (pscatter || est * N >= (double)nwin * SPAN_WORDS);
                }
                // (TASK_PSET) windows per ROUND of k_psets: a wave stages the survivors of its share of a round — a sub-window of PSET_ROUND_DOCS documents per
                // window — in PSET_STAGE_DOCS LDS slots before the round's counts cross; as many windows as are expected to fill three quarters of them
                uint32_t round_win = 1;
                while (round_win < PSET_TASK_WINDOWS && est * (double)PSET_ROUND_DOCS * (double)(round_win * 2u) <= 0.75 * (double)PSET_STAGE_DOCS)
                        round_win *= 2u;
                if (pscatter && !bitmap)
                        return herr(f.err, TRI_ERR_INTERNAL, "query %u: a scatter union whose result is not a bitmap", t.q.qid);
                t.q.form = bitmap ? RESULT_BITMAP : RESULT_DOCIDS;
                // bitmap-window tasks stage their terms once: two windows of a head pair per task
                const uint64_t per_win = std::max<uint64_t>(1, t.sumdf / (ix.info.docs_cnt / SPAN_BITS + 1)) + (pset ? 0 : opt.dense_window_cost);
                // (a query with phrases: its tasks are k_phrase's too, where a candidate costs a walk into two or three lists' hits — tens of times a bitmap
                //  word; a task of four windows of two head terms was 76 K candidates, 1 - 2 ms, and k_phrase's span is its longest task: option phrase_task_div)
                const uint32_t pdiv = t.q.nphrases ? (uint32_t)std::max<uint64_t>(1, C.phrase_task_div) : 1u;
                const uint32_t win_per_task = pset ? std::max(1u, PSET_TASK_WINDOWS / pdiv) : (uint32_t)std::max<uint64_t>(1, std::max<uint64_t>(1, opt.dense_task_cost) / pdiv / per_win);
                uint32_t ord = 0;
                uint64_t lead_blocks = 0;
                for (uint32_t k = 0; k < nlead; ++k)
                        lead_blocks += ix.terms[qt[k] & QT_TERM].nblocks;
                uint64_t heaviest = 0xffffffffull; // (TASK_PSET) the df rank of the query's heaviest term: the schedule's place within a window range
                for (uint32_t k = 0; pset && k < t.q.nterms; ++k)
                        heaviest = std::min<uint64_t>(heaviest, ix.df_rank[qt[k] & QT_TERM]);
                for (uint32_t wb = 0; wb < nwin; wb += win_per_task, ++ord) {
                        const uint32_t we = std::min(nwin, wb + win_per_task);
                        // matches of windows [wb, we) are lead-group documents of blocks b1 .. (next task's b1) of every
                        // lead list: a private region (+32 slots of slack per lead list and task for the straddling block)
                        uint64_t b1 = 0;
                        for (uint32_t k = 0; k < nlead; ++k)
                                b1 += C.first_block_ge(ix.terms[qt[k] & QT_TERM], (uint64_t)wb * SPAN_BITS);
                        f.tcost.push_back(pset ? wb | heaviest << 32 : per_win * (we - wb)); // (TASK_PSET: the schedule goes by window range, not by cost)
                        const uint64_t task_off = bitmap ? off + (uint64_t)wb * SPAN_WORDS : off + b1 * 32 + 32ull * ord * nlead;
                        if (pset)
                                f.units.push_back(make_unit(t.q, qt, (uint32_t)f.tasks.size(), wb, we, task_off,
                                                            (bitmap ? PSET_UNIT_BITMAP : 0u) | (pscatter ? PSET_UNIT_SCATTER : 0u) | round_win << PSET_UNIT_ROUND_SHIFT));
                        f.tasks.push_back({slot, wb, we, pset ? TASK_PSET : TASK_DENSE, task_off});
                }
                t.q.out_cap = bitmap ? nwin * SPAN_WORDS : (uint32_t)std::min<uint64_t>(0xffffffffull, lead_blocks * 32 + 32ull * (ord + 1) * nlead);
                f.bitmap_queries += bitmap;
                f.pscatter_queries += pscatter;
                return TRI_OK;
        }

        // (option account_needed_bytes) what a perfect gallop must read of a candidate-tile query: the lead list, and of every other list the
        // blocks that can hold a lead candidate — per lead block the other list's blocks its docID range meets, at most one per candidate
        // (directories only; a block counts docbytes / nblocks)
        inline uint64_t cand_needed_bytes(const HostIndex &ix, const uint32_t *qt, const uint32_t nterms) {
                const DevTerm &lead = ix.terms[qt[0] & QT_TERM];
                uint64_t need = ix.docbytes[qt[0] & QT_TERM];
                const uint32_t *ll = &ix.blk_last[lead.first_block];
                for (uint32_t k = 1; k < nterms; ++k) {
                        const DevTerm &tk = ix.terms[qt[k] & QT_TERM];
                        const uint32_t *ol = &ix.blk_last[tk.first_block];
                        uint64_t blocks = 0;
                        uint32_t at = 0; // (both directories ascend: the searches move forward)
                        for (uint32_t lb = 0; lb < lead.nblocks && at < tk.nblocks; ++lb) {
                                const uint32_t lo_doc = lb ? ll[lb - 1] + 1 : 1u, hi_doc = ll[lb];
                                at = (uint32_t)(std::lower_bound(ol + at, ol + tk.nblocks, lo_doc) - ol);
                                if (at >= tk.nblocks)
                                        break;
                                const uint32_t last = (uint32_t)(std::lower_bound(ol + at, ol + tk.nblocks, hi_doc) - ol);
                                const uint32_t span = std::min(last, tk.nblocks - 1) - at + 1;
                                const uint32_t ndocs = lb + 1 == lead.nblocks ? lead.last_n : 32u;
                                blocks += std::min(span, ndocs);
                        }
                        need += (uint64_t)((double)ix.docbytes[qt[k] & QT_TERM] * std::min(1.0, (double)blocks / std::max(1u, tk.nblocks)));
                }
                return need;
        }

        // candidate tiles of the lead list (TASK_CAND), or — Route::probe — the same tiles as k_probe's tasks (TASK_PROBE, with their unit records)
        inline void tasks_tiles(const Ctx &C, Frag &f, Tmp &t, const uint32_t slot, const uint32_t *qt, const Route r, const uint64_t off) {
                const tri_options &opt = C.env.opt;
                const DevTerm &lead = C.ix.terms[qt[0] & QT_TERM];
                const uint32_t ntiles = (lead.nblocks + TILE_BLOCKS - 1) / TILE_BLOCKS;
                const uint64_t per_tile = std::max<uint64_t>(1, t.cost / ntiles);
                const uint32_t tiles_per_task = (uint32_t)std::max<uint64_t>(1, std::max<uint64_t>(1, opt.cand_task_cost / (t.q.nphrases ? std::max<uint64_t>(1, C.phrase_task_div) : 1)) / per_tile);
                for (uint32_t tb = 0; tb < ntiles; tb += tiles_per_task) {
                        const uint32_t te = std::min(ntiles, tb + tiles_per_task);
                        f.tcost.push_back(per_tile * (te - tb));
                        if (r.probe)
                                f.units.push_back(make_unit(t.q, qt, (uint32_t)f.tasks.size(), tb, te, off + (uint64_t)tb * TILE_CANDS, tb == 0 ? PSET_UNIT_FIRST : 0u));
                        f.tasks.push_back({slot, tb, te, r.probe ? TASK_PROBE : TASK_CAND, off + (uint64_t)tb * TILE_CANDS});
                }
                t.q.out_cap = lead.documents; // |A ∩ …| <= df of the lead
                if (opt.account_needed_bytes)
                        f.cand_needed_term_bytes += cand_needed_bytes(C.ix, qt, t.q.nterms);
        }

        // ---- second pass: cut the fragment's queries into tasks (offsets relative to the fragment)
        inline int task_range(const Ctx &C, Frag &f) {
                const HostIndex &ix = C.ix;
                f.benefit.assign(C.n_ok, 0);
                f.cand_row.assign(C.n_ok, 0);
                uint64_t off = 0;
                for (size_t ti = 0; ti < f.tmp.size(); ++ti) {
                        if (ti + 6 < f.tmp.size()) { // (the per-term records of the query six queries on: see lower_range)
                                const Tmp &a = f.tmp[ti + 6];
                                for (uint32_t k = 0; k < a.q.nterms && k < 8 && !a.tree; ++k)
                                        prefetch_term(ix, f.qterms[a.q.term_base + k] & QT_TERM);
                        }
                        Tmp &t = f.tmp[ti];
                        const uint32_t slot = (uint32_t)ti;
                        if (t.tree) {
                                tasks_tree(C, f, t, slot, off);
                                continue;
                        }
                        if (t.fuse) {
                                if (const int rc = tasks_onepass(C, f, t, slot, off))
                                        return rc;
                                continue;
                        }
                        const uint32_t *qt = &f.qterms[t.q.term_base];
                        const Route r = route_cnf(C, f, t, qt);
                        t.q.out_off = off;
                        t.q.first_task = (uint32_t)f.tasks.size();
                        if (t.dense) {
                                if (const int rc = tasks_windows(C, f, t, slot, qt, r, off))
                                        return rc;
                        } else
                                tasks_tiles(C, f, t, slot, qt, r, off);
                        off += t.q.out_cap;
                        t.q.ntasks = (uint32_t)f.tasks.size() - t.q.first_task;
                        if (t.q.nphrases)
                                for (uint32_t k = t.q.first_task; k < t.q.first_task + t.q.ntasks; ++k)
                                        f.ptasks.push_back(k);
                }
                f.off = off;
                return TRI_OK;
        }
} // namespace trip

// planner_types.hpp — what the host planner's passes share (planner.hpp): the options, the plan a batch comes out as (BatchPlan: one host
// block of sections, declared ONCE in for_each_section), a fragment's working set (Frag, Scratch) and the small helpers the lowering
// (planner_lower.hpp) and the task cutter (planner_tasks.hpp) both use.  Host-only C++17, no HIP.  New code, no reference source.
#pragma once
#include "host_pool.hpp"
#include "index_host.hpp"

#include <array>
#include <chrono>
#include <cmath>
#include <memory>
#include <numeric>

// planner / launch options of a device handle (tri_dev_set_option); the defaults are what bench.py measures
struct tri_options {
        uint64_t dense_min_postings = 512 * 1024; // TASK_DENSE needs at least this many postings over the query's lists (0: every multi-term query)
        uint64_t dense_task_cost = 192 * 1024;    // postings per bitmap-window task
        uint64_t dense_window_cost = 16 * 1024;   // ... a docID window counts this many postings whatever it holds (k_and_dense: directory look-ups, barriers, the sweep:
                                                  // measured 28 us a window on unions of rare terms — a task of 77 near-empty windows ran 2.2 ms, cfg5's k_and_dense 58 % busy)
        uint64_t cand_task_cost = 32 * 1024;      // cost units (postings decoded + 32 per partner block that can hold a candidate) per candidate-tile task
                                                  // (cfg3's k_and, ms at 96 K / 32 K / 8 K: 0.61 / 0.60 / 0.60 — before the galloping merge 2.93 / 1.75 / 1.77)
        uint64_t fused = 1;                       // AccumulatedScore top-K of dense queries in one pass (k_fused); 0: k_and_dense + k_score
        uint64_t fused_task_cost = 0;             // postings per one-pass task; 0: sized from the batch (256 K .. 8 M, about two tasks per resident workgroup)
        uint64_t fused_freq_cap = 0;              // 0: the field width decides; else a smaller saturation point (exercises the rescoring path)
        uint64_t account_needed_bytes = 0;        // 1: tri_batch_create also works out tri_batch_info.cand_needed_bytes (a directory walk per candidate-tile query)
        uint64_t fused_halfwords = 1;             // 16-bit window words for queries of <= 5 distinct terms (windows twice as long); 0: always 32-bit
        uint64_t overlap_dense_wgs = 0, overlap_cand_wgs = 0; // both non-zero: the two matching kernels side by side on two streams
        uint64_t overlap = 0;                                 // 1: the candidate-tile kernel (k_and) on a second stream beside the window kernels (k_and_dense, k_psets, k_probe), full grids
        uint64_t planes = 7;     // term planes (k_planes.hpp), a bit set: 1 k_and probes them, 2 k_and_dense ORs them in, 4 top-K CNF queries run in k_planes; 0: off
        uint64_t planes_split = 0; // a k_planes query is cut into this many docID ranges (tasks) that share its threshold; 0: 2 or 3 by the batch's size; >= 65536: by postings like the other one-pass tasks.  cfg3's unions: 0 10.9 ms, 2 8.0, 3 8.5, 4 9.2 (a task has fixed costs)
        uint64_t plane_div = 1024; // a term gets a plane when it holds at least docs_cnt / plane_div documents (and the batch's uses repay one decode of its list).
                                 // Round 5 (k_planes' level words, k_and's row queues), step ms at 512 / 1024 / 2048: cfg3 5.95 / 5.63 / 5.57, cfg5 7.42 / 7.27 / 7.28, cfg2 1.30 / 1.31 / 1.31
                                 // — 698 rows at cfg3 (8.75 MB each at 10 M documents).  Earlier rounds:
                                 // While a batch built its own planes: step ms at 32 / 64 / 128 / 256: cfg3 16.9 / 15.9 / 15.3 / 15.4, cfg2 - / 2.90 / 2.71 / 2.76 (the
                                 // build grew with it).  The planes live with the index now (built once): 128 / 512 / 4096: cfg2 1.48 / 1.44 / 1.40, cfg3 12.64 / 12.40 / 12.4,
                                 // cfg4 17.4 / 16.9 / 16.9 — 355 rows (1.3 GB at 10 M documents) at 512
        uint64_t plane_amortize = 1;           // a term is given a plane when plane_amortize x (the postings the batch's uses of it save) repay one decode of its list: the rows live with the
                                               // index, so a stream of batches repays a row over several of them (1: every batch repays its own rows)
        uint64_t plane_max_bytes = 8ull << 30; // scratch budget of a batch's term planes: the eligible terms are the longest lists that fit (each costs PL_PLANES bitmaps over the docID space and one decode per index)
        uint64_t planes_rebuild = 0;           // 1: every tri_batch_run decodes the plane rows its batch names AGAIN (a cold plane cache: what a query stream pays whose head
                                               // terms have all just been evicted) — a measurement switch (bench.py's rotating leg), never a speed-up
        uint64_t phrase_task_div = 0;          // the tasks of a query with phrases are cut this many times finer (they are k_phrase's tasks too, and a phrase candidate costs far more than the
                                               // planner's unit: k_phrase's span is its longest task); 0: by the batch's phrase queries per compute unit (4 / 2 / 1: plan_batch)
        uint64_t planes_order = 1;             // k_planes' tasks: 1 docID range by range, within a range by the heaviest plane row they sweep (the workgroups in flight stream the same
                                               // head rows from about the same place: those words come from L2); 2: row by row, a query's ranges side by side; 0: heaviest task first.
                                               // Round 6, k_planes ms at 0 / 1 / 2: cfg3 4.40 / 4.12 / 4.33, cfg5's shard 2.17 / 2.10 / 2.20 (with four ranges a query: 5.44 / 4.73 / -)
        uint64_t scatter_bitmap_slack = 4;     // a DocumentsOnly union of head terms with terms that have no plane runs in k_psets (PSET_UNIT_SCATTER: plane words OR-ed, the other terms'
                                               // documents listed by k_psets_prep) — its result a bitmap — when its head terms hold one document in 32 x slack or more; 1: only where a
                                               // bitmap is no larger than the docID list (the rule of every other query).  The rest of those unions decode every list into LDS window
                                               // bitmaps (k_and_dense): 1.9 us a query against 0.5 (cfg5's 100 K batch).  A result at one document in 128 costs 4 x the bytes as a bitmap
        uint64_t pset_order = 1;               // k_psets' tasks: 1 docID range by range and, within a range, by the query's HEAVIEST term (PSET_SUBS places by its df rank): the workgroups in
                                               // flight read that term's words of the range one after the other — the second and later readers from L2, not over the fabric; 0: batch order
                                               // within a range
        uint64_t cand_xcd = 1;                 // k_and's tasks queued per XCD by the plane row they probe (planner.hpp "k_and's queues"); 0: the cost order dealt round the queues
        uint64_t plan_threads = 0;             // host threads a planner context plans with; 0: up to 16, one per 512 queries, within the process's CPU budget (affinity mask, cgroup quota) shared by the handle's contexts
        uint64_t plan_hot_us = 300;            // ... keep polling for a job this long after their last one before they sleep (a polling thread uses a CPU of the process's quota;
                                               // the gaps between the passes of one create are below 0.1 ms).  Read when a pool starts
        uint64_t plan_pin = 2;                 // the planner's workers: 1 each pinned to ONE CPU; 2 to its pool's STRETCH of CPUs (host_pool.hpp: spread); 0 not pinned at all.  Read when a pool starts
        uint64_t result_bitmaps = 1;           // DocumentsOnly: a bitmap-window query whose expected matches outnumber the words of a bitmap over its docID range
                                               // delivers its docID set AS that bitmap (RESULT_BITMAP, dev_structs.hpp); 0: always ascending docIDs
        uint64_t tree_max_bytes = 16ull << 30; // scratch budget of a batch's TASK_TREE queries (a PL_PLANES-plane row per distinct term leaf, a plane per phrase leaf and per query)
        uint64_t tree_max_nodes = 64;          // a tree of more than this many nodes is left out (TRI_ERR_UNSUPPORTED per query).  64 (TREE_MAX_NODES: all the narrow kernels of k_tree.hpp
                                               // hold) .. 1024 (TREE_WIDE_MAX_NODES); any other value fails tri_batch_create.  Trees above 64 nodes run in k_tree_wide.hpp's kernels
        uint64_t tree_wide_min_nodes = 65;     // a TASK_TREE query of at least this many nodes gets a wide record and k_tree_wide.hpp's kernels; 0: every tree query does — not a tuning
                                               // knob: it lets the tests run the trees they have reference answers for through the wide kernels
        uint64_t rich_max_terms = 16;          // default mode: a query of more reportable terms than this is left out (TRI_ERR_UNSUPPORTED per query).  16 (RICH_NARROW_TERMS) .. 64
                                               // (RICH_WIDE_TERMS: one 64-bit mask, and what the CPU oracle holds); any other value fails tri_batch_create.  Off by default because
                                               // of what a wide-report query reserves: 2 x stride bytes of frequency row + 8 bytes of masks per OUTPUT SLOT (its tree's upper bound)
        uint64_t isect_max_bytes = 2ull << 30; // tri_isect_run (isect_side.hpp): scratch budget of a call — plane-0 rows (one per distinct known term), the requests' tables, the per-span words;
                                               // beyond it the call is TRI_ERR_UNSUPPORTED
        uint64_t isect_max_masks = 262144;     // ... most slots of a request's table H (distinct considered masks; 16 + 4 bytes each): sized by the call's widest request (2 x 2^groups) up to this
        uint64_t isect_max_runs = 524288;      // ... of its table C ((mask, epoch) run credits; 12 bytes each): sized after pass 1 from H's exact bound, up to this.  A request that
                                               // overflows either table answers TRI_ERR_UNSUPPORTED
        uint64_t perc_max_bytes = 4ull << 30;  // tri_perc_match (perc_side.hpp): the pooled scratch of a call — the batch, a row per leaf it holds, a row of match words per candidate query, the pairs
                                               // in both orders; beyond it the call is TRI_ERR_UNSUPPORTED (split it)
        uint64_t perc_prune = 1;               // ... 0: every enabled stored query is evaluated, whether the batch holds one of its leaves or not (for measurement: the pairs are the same)
        uint64_t probe_max_blocks = 0;         // > 0: a lead list of at most this many blocks against lists that all have planes runs in k_probe (a wave per task) instead of
                                               // k_and's candidate tiles.  Off by default — measured at cfg2 (step ms / k_probe / k_and): 0: 2.14 / - / 0.78; 64: 2.25 / 0.15 / 0.75;
                                               // 256: 2.26 / 0.22 / 0.70; 1024: 2.35 / 0.41 / 0.59; all: 2.55 / 0.82 / 0.41 — k_and's time is its tail, not its task count
};

struct PlanEnv {
        tri_options opt;
        uint32_t cus = 256;          // compute units of the device (task sizes aim at a couple of tasks per resident workgroup)
        uint32_t fus_wgs_per_cu = 2; // k_fused workgroups a CU holds (LDS)
        uint32_t plk_wgs_per_cu = 2; // k_planes workgroups a CU holds
};

template <class T>
struct Span { // a typed window into the plan's host block: a SECTION of it (for_each_section), `off` bytes in
        T *p = nullptr;
        size_t n = 0;
        size_t off = 0;
        size_t size() const { return n; }
        bool empty() const { return !n; }
        T *data() { return p; }
        const T *data() const { return p; }
        T &operator[](size_t i) { return p[i]; }
        const T &operator[](size_t i) const { return p[i]; }
        T *begin() { return p; }
        T *end() { return p + n; }
        const T *begin() const { return p; }
        const T *end() const { return p + n; }
};

struct PlanInput {
        const uint32_t *prog = nullptr;
        size_t prog_len = 0;
        const tri_query *queries = nullptr;
        size_t nq = 0;
        const double *weights = nullptr; // optional: one ScorerWeight per program token
        uint32_t flags = 0, topk = 0;
        int similarity = TRI_SIM_BM25;
};

namespace trip {
        // What a fragment counts while it lowers and cuts its queries, and a plan reports for the batch: merge() folds a fragment's into the plan's
        struct PlanCounters {
                uint64_t term_bytes = 0, term_bytes_dense = 0, term_bytes_fused = 0, term_bytes_planes = 0, term_bytes_phrase_hits = 0, term_bytes_pset = 0, term_bytes_probe = 0,
                         cand_needed_term_bytes = 0; // (cand_needed_term_bytes: option account_needed_bytes)
                uint64_t dense_queries = 0, pset_queries = 0, probe_queries = 0, cand_queries = 0, fused_queries = 0, planes_queries = 0, tree_queries = 0;
                uint64_t bitmap_queries = 0; // queries whose docID set is delivered as a bitmap (RESULT_BITMAP)
                uint64_t pscatter_queries = 0, pscatter_docs = 0; // ... of them the unions k_psets runs although some of their terms have no plane (PSET_UNIT_SCATTER), and those terms'
                                                                  // documents over all such queries: the slots k_psets_prep lists them in, task by task
                uint64_t cand_lead_docs = 0, cand_terms = 0;         // (candidate-tile and probe queries: their leads' documents, their terms)
                uint64_t probe_demoted = 0, probe_demoted_bytes = 0; // (fill pass, a fragment's own) queries whose probes found no plane: candidate tiles after all
                uint32_t sparse_cap = 0;                             // k_planes: list entries a task's decoded slots can need
                uint32_t rich_R = 0;                                 // default mode: reportable terms of the widest NARROW query (at most RICH_NARROW_TERMS of them)
                uint64_t rich_wide_queries = 0;                      // default mode: wide-report queries (option rich_max_terms; their rows: BatchPlan::rich_wide)
                bool rich_allow = false;                             // default mode: the batch holds general trees (per match: which reportable terms the tree sits on)
                void merge(const PlanCounters &o) {
                        term_bytes += o.term_bytes, term_bytes_dense += o.term_bytes_dense, term_bytes_fused += o.term_bytes_fused, term_bytes_planes += o.term_bytes_planes;
                        term_bytes_phrase_hits += o.term_bytes_phrase_hits, term_bytes_pset += o.term_bytes_pset, term_bytes_probe += o.term_bytes_probe;
                        cand_needed_term_bytes += o.cand_needed_term_bytes;
                        dense_queries += o.dense_queries, pset_queries += o.pset_queries, probe_queries += o.probe_queries, cand_queries += o.cand_queries;
                        fused_queries += o.fused_queries, planes_queries += o.planes_queries, tree_queries += o.tree_queries;
                        bitmap_queries += o.bitmap_queries, pscatter_queries += o.pscatter_queries, pscatter_docs += o.pscatter_docs;
                        cand_lead_docs += o.cand_lead_docs, cand_terms += o.cand_terms;
                        probe_demoted += o.probe_demoted, probe_demoted_bytes += o.probe_demoted_bytes;
                        sparse_cap = std::max(sparse_cap, o.sparse_cap);
                        rich_R = std::max(rich_R, o.rich_R);
                        rich_wide_queries += o.rich_wide_queries;
                        rich_allow |= o.rich_allow;
                }
        };
} // namespace trip

// What tri_batch_create hands to the device and keeps on the host to read results back.  Every array is a SECTION of ONE block (64-byte aligned,
// Span::off = its byte offset; trip::for_each_section lists them): the device copy is one transfer of block[0, block_bytes) and a section's
// device address is arena + off.
struct BatchPlan : trip::PlanCounters {
        uint8_t *block = nullptr;
        size_t block_bytes = 0;
        Span<DevQuery> plan;        // one per lowered query, in query order
        Span<uint32_t> qterms;      // CNF term lists (QT_GROUP / QT_NOT marks)
        Span<DevTask> tasks;        // a query's tasks are consecutive
        Span<uint32_t> sched;       // task indices by kernel, heaviest first: [0, n_dense) TASK_DENSE, then TASK_PSET, TASK_PROBE, TASK_CAND, TASK_FUSED, TASK_FUSED16, TASK_FUSED_GEN, TASK_PLANES, TASK_PLANES8
        Span<DevFused> fused;       // slot maps of the one-pass queries (DevQuery::fused_idx)
        Span<uint32_t> qplane;      // parallel to qterms: the term's row in the batch's term planes, or PL_NONE (empty: no planes)
        Span<uint32_t> plane_terms; // row -> term
        Span<uint32_t> splane;      // parallel to sterms (scored batches with planes; else empty): the scorer's term's plane row, or PL_NONE — k_score reads a
                                    // match's frequency off planes B / C instead of decoding a block of the term
        Span<uint32_t> sterms;      // scored: scorer terms in the reference's summation order; default mode: reportable terms
        Span<double> sweights;      // scored: their ScorerWeights
        Span<DevPhrase> phrases;
        Span<uint32_t> pterms, ptasks;
        Span<DevPsetUnit> units;    // the TASK_PSET and TASK_PROBE tasks as k_psets / k_probe read them (task order) ...
        Span<uint32_t> pset_sched;  // ... and the order they are run in, as unit indices: [0, n_pset) TASK_PSET, docID window range by window range; then
                                    // the n_probe TASK_PROBE ones, heaviest first
        Span<uint32_t> cand_q;      // k_and's task queues, one per XCD: queue x = the TASK_CAND section of sched at [cand_q[x], cand_q[x + 1]) (CAND_QUEUES + 1 bounds)
        Span<uint32_t> tree;        // TASK_TREE records: TREE_HDR_WORDS header words + DevTreeNode per node (DevQuery::fused_idx: the record's first word)
        Span<uint32_t> tree_terms;  // the distinct term leaves of the batch's TASK_TREE queries, ascending: term -> row of the batch's tree rows
        Span<uint32_t> tree_hidden; // hidden phrase queries: their plan slots (position: the row of the batch's phrase rows)
        Span<DevRichWide> rich_wide; // default mode, batches with wide-report queries (else empty): per plan slot, where the query's wide rows and high masks lie
        Span<uint32_t> rich_sched;  // ... and k_rich's own schedule (else it runs off sched): sched's order with the wide-report queries' tasks moved to the end —
                                    // [0, tasks - n_rich_wide) the existing instantiations' launch, the last n_rich_wide the wide one's
        uint32_t n_rich_wide = 0;   // tasks of wide-report queries
        uint64_t rich_wide_cells = 0, rich_wide_slots = 0; // 16-bit cells of the wide frequency array; slots of the high-half mask arrays
        uint32_t n_tree = 0;        // TASK_TREE tasks (the last section of sched)
        uint32_t n_tree_wide = 0;   // ... of them the last n_tree_wide have WIDE records (k_tree_wide.hpp); the narrow ones come first
        uint64_t tree_scratch_bytes = 0;
        std::vector<uint32_t> slot_of_query; // caller query -> plan slot (UINT32_MAX: can never match)
        std::vector<int32_t> qstatus;        // per caller query: TRI_OK, or why the planner left it out of the batch (it then reports no matches)
        uint32_t n_dense = 0, n_pset = 0, n_probe = 0, n_cand = 0, n_fused = 0, n_fused16 = 0, n_fusedgen = 0, n_planes = 0, n_planes8 = 0;
        uint32_t plw = 0;        // words of one term plane
        uint32_t plane_rows = 0; // rows the batch may address: the terms eligible for a plane under the options it was planned with (row = df rank)
        uint64_t out_capacity = 0;
        uint64_t plane_decoded_bytes = 0, unsupported_queries = 0;
        // option account_needed_bytes (a diagnostic of bench.py, untimed): the bytes of the DISTINCT lists the batch's queries name — each
        // list once, however many queries share it: what a batch that shares decodes has to read at least — over the whole batch (doc bytes,
        // plus the hit bytes of the distinct phrase / reported terms) and per execution class (by task kind; [TASK_KINDS]: the phrases' hit bytes)
        uint64_t distinct_bytes = 0, distinct_bytes_kind[TASK_KINDS + 1] = {};
        std::string last_unsupported; // describes the last query that was left out
        double plan_ms[4] = {0, 0, 0, 0}; // lowering + classes, tasks, layout + fill, schedule + planes
};

namespace trip {
        constexpr size_t SECTION_ALIGN = 64;
        // how many elements each section of a plan's block holds: settled once the fragments' sums and the chosen planes are known (place_fragments,
        // choose_planes) — the three conditional ones (qplane, splane, sweights) there and nowhere else
        struct SectionCounts {
                size_t plan = 0, qterms = 0, tasks = 0, fused = 0, qplane = 0, plane_terms = 0, splane = 0, sterms = 0, sweights = 0, phrases = 0, pterms = 0, ptasks = 0, units = 0,
                       tree = 0, tree_terms = 0, tree_hidden = 0, rich_wide = 0, rich_sched = 0;
        };
        // THE list of the block's sections, in block order: fn(the section's Span, its element count).  The layout, the host spans, the device
        // addresses (tri_batch::dev_at) and the offsets the summary reports all come from it
        template <class Plan, class Fn>
        inline void for_each_section(Plan &P, const SectionCounts &n, Fn &&fn) {
                fn(P.plan, n.plan);
                fn(P.qterms, n.qterms);
                fn(P.tasks, n.tasks);
                fn(P.sched, n.tasks);
                fn(P.fused, n.fused);
                fn(P.qplane, n.qplane);
                fn(P.plane_terms, n.plane_terms);
                fn(P.splane, n.splane);
                fn(P.sterms, n.sterms);
                fn(P.sweights, n.sweights);
                fn(P.phrases, n.phrases);
                fn(P.pterms, n.pterms);
                fn(P.ptasks, n.ptasks);
                fn(P.units, n.units);
                fn(P.pset_sched, n.units);
                fn(P.cand_q, (size_t)CAND_QUEUES + 1);
                fn(P.tree, n.tree);
                fn(P.tree_terms, n.tree_terms);
                fn(P.tree_hidden, n.tree_hidden);
                if (n.rich_wide) { // (only a batch with wide-report queries has them: every other batch's block is what it was)
                        fn(P.rich_wide, n.rich_wide);
                        fn(P.rich_sched, n.rich_sched);
                }
        }
        // the sections one after the other from offset 0 (every Span's off and n); returns the block's size
        inline size_t layout_sections(BatchPlan &P, const SectionCounts &n) {
                size_t bytes = 0;
                for_each_section(P, n, [&](auto &s, const size_t count) {
                        s.off = bytes;
                        s.n = count;
                        bytes += (count * sizeof(*s.p) + SECTION_ALIGN + SECTION_ALIGN - 1) & ~(SECTION_ALIGN - 1); // (a spare 64 bytes behind every array: wide loads at an array's end stay inside the block)
                });
                return bytes;
        }
        // ... and, once the block is there, the spans pointed into it
        inline void point_sections(BatchPlan &P, const SectionCounts &n) {
                for_each_section(P, n, [&](auto &s, size_t) { s.p = reinterpret_cast<std::remove_reference_t<decltype(*s.p)> *>(P.block + s.off); });
        }

        constexpr uint32_t SCHED_NB = 64 * 4; // schedule buckets per kernel: cost octave + 2 bits
        constexpr uint32_t CAND_SUBS = 128, CAND_COST_SUBS = 16; // ... k_and's in row order have buckets of their own (behind the kernels': CAND_KEY0): per queue, 16 for the long and the
                                                               // row-less tasks by cost, 111 places for rows, one for the stragglers
        constexpr uint32_t PSET_RANGE_BKS = 64, PSET_SUBS = 64; // ... k_psets' by (docID window range, heaviest term of the query): the ranges of a long docID space share the 64 range buckets
        constexpr uint32_t CAND_KEY0 = TASK_KINDS * SCHED_NB, PSET_KEY0 = CAND_KEY0 + CAND_QUEUES * CAND_SUBS, SCHED_KEYS = PSET_KEY0 + PSET_RANGE_BKS * PSET_SUBS;
        // a TASK_PSET task's tcost word: its first window in the low half, the df rank of its query's heaviest term in the high half
        inline uint32_t pset_sub(const uint32_t rank) { return rank < PSET_SUBS / 2 ? rank : std::min(PSET_SUBS / 2 + (rank - PSET_SUBS / 2) / 8, PSET_SUBS - 1); }
        constexpr uint64_t CAND_ROWS_MIN_LEAD = 1024;
        // launch order of the task kinds: TASK_DENSE, TASK_PSET, TASK_PROBE, TASK_CAND, then the one-pass kinds as numbered
        constexpr uint32_t SCHED_RANK[TASK_KINDS] = {3, 0, 4, 5, 6, 7, 8, 1, 2, 9};
        // per task kind, the BatchPlan counter of its sched[] section
        constexpr uint32_t BatchPlan::*const SCHED_COUNT[TASK_KINDS] = {&BatchPlan::n_cand, &BatchPlan::n_dense, &BatchPlan::n_fused, &BatchPlan::n_fused16, &BatchPlan::n_fusedgen,
                                                                        &BatchPlan::n_planes, &BatchPlan::n_planes8, &BatchPlan::n_pset, &BatchPlan::n_probe, &BatchPlan::n_tree};
        // the first sched[] index of a kind's section: the sections of the kinds that launch before it come first
        inline uint32_t sched_first(const BatchPlan &P, const uint32_t kind) {
                uint32_t at = 0;
                for (uint32_t k = 0; k < TASK_KINDS; ++k)
                        if (SCHED_RANK[k] < SCHED_RANK[kind])
                                at += P.*SCHED_COUNT[k];
                return at;
        }
        // a cost's schedule bucket: its octave + 2 bits (tasks within a fifth of each other share one) — the schedule's and k_phrase's order
        inline uint32_t cost_bucket(const uint64_t cost) {
                const uint64_t c = std::max<uint64_t>(1, cost);
                const uint32_t lg = 63u - (uint32_t)__builtin_clzll(c);
                const uint32_t frac = lg >= 2 ? (uint32_t)((c >> (lg - 2)) & 3u) : (uint32_t)((c << (2 - lg)) & 3u);
                return lg * 4 + frac;
        }
        inline uint32_t sched_key(const uint32_t kind, const uint64_t cost) {
                if (kind == TASK_PSET) // by docID window range, ascending (`cost` holds the first window)
                        return SCHED_RANK[TASK_PSET] * SCHED_NB + (uint32_t)std::min<uint64_t>((cost & 0xffffffffull) / PSET_TASK_WINDOWS, SCHED_NB - 1);
                return SCHED_RANK[kind] * SCHED_NB + (SCHED_NB - 1 - cost_bucket(cost));
        }

        struct PNode {
                uint32_t op = 0, term = 0;
                uint32_t tok = 0; // index of the program token this node came from (caller-supplied ScorerWeights are per token)
                uint32_t kid_off = 0, kid_n = 0; // children: kidpool[kid_off, +kid_n)
                uint64_t cost = 0;
                bool empty = false;
        };

        // one fragment's scratch for parsing and lowering a query: reused from query to query (clear() keeps the capacity — a query costs
        // no allocation once the vectors have grown to the batch's widest query)
        struct Scratch {
                std::vector<PNode> nodes;
                std::vector<int> kidpool, st, tmpk;
                std::vector<uint64_t> cs;
                std::vector<uint32_t> gt, gs; // CNF groups, flat: group g = gt[gs[g], gs[g + 1])
                std::vector<uint32_t> gorder, leaves, leaf_tok, negs, opts, opt_tok, ts, ts_tok, u, uniq, rt, seen, phterms, slots;
                struct PhraseTmp {
                        uint32_t t0, n;
                        double weight;
                };
                std::vector<PhraseTmp> qphrases;
                std::vector<std::pair<uint32_t, double>> sc;
                const int *kids(const PNode &x) const { return kidpool.data() + x.kid_off; }
        };

        // a lowered query before it has its place in the batch
        struct Tmp {
                DevQuery q;
                uint64_t cost;
                uint32_t nlead;
                int32_t fz;   // index into the fragment's slot maps (-1: none): may run in one pass (k_fused / k_planes)
                bool truth;   // a general tree: runs as TASK_FUSED whatever its density (there is no other path for it)
                bool tree;    // ... one the truth table does not hold: TASK_TREE (q.fused_idx: its record in the fragment's treepool; tree_ub: its matches at most)
                bool hidden;  // a phrase evaluated for a TASK_TREE query of the batch (no caller query of its own); hidden_ord: which of the fragment's
                uint64_t tree_ub;
                bool tree_wide; // ... with a wide record (DevTreeNodeW)
                uint32_t hidden_ord;
                // execution class (second half of the first pass)
                uint64_t sumdf, lead_docs;
                uint32_t last_doc; // no match beyond the (required) group whose lists end first
                bool dense, fuse;
        };

        struct QUse { // a CNF term position that could read a plane
                uint32_t qpos, term;
        };
        struct FUse { // a one-pass slot that reads a plane
                uint32_t fidx, slot, term;
        };

        // everything a fragment (a contiguous range of the batch's queries) produces; offsets are relative to the fragment.  Its counters
        // (PlanCounters) are folded into the plan's between the passes
        struct Frag : PlanCounters {
                size_t q_lo = 0, q_hi = 0;
                Scratch S;
                std::vector<Tmp> tmp;
                std::vector<uint32_t> qterms, pterms, sterms;
                std::vector<double> sweights;
                std::vector<DevPhrase> phrases;
                std::vector<DevFused> fz; // slot maps of the queries that may run in one pass (Tmp::fz)
                std::vector<size_t> left_out; // queries the planner does not lower (status TRI_ERR_UNSUPPORTED)
                uint64_t onepass_queries = 0, fused_postings = 0, phrase_queries = 0;
                // second pass
                std::vector<DevTask> tasks; // slot: index into tmp; out_off: relative to the fragment's first output slot
                std::vector<uint64_t> tcost;
                std::vector<DevFused> fused;
                std::vector<uint32_t> ptasks;
                std::vector<DevPsetUnit> units; // tix: index into the fragment's tasks; row[]: filled once the planes are chosen
                std::vector<QUse> quses, suses; // (suses: scorer positions — qpos indexes the fragment's sterms)
                std::vector<FUse> fuses;
                std::vector<uint64_t> benefit; // per eligible term (by df rank): postings of decoding the batch's uses save
                std::vector<uint64_t> cand_row; // per eligible term: tiles (+ 1 a task) of the candidate-tile tasks whose first probed term it is
                std::vector<uint32_t> keys, hist; // (fill pass) per task its schedule bucket; tasks per bucket
                std::vector<uint32_t> treepool;   // TASK_TREE records (DevQuery::fused_idx: a record's first word)
                std::vector<uint32_t> tree_terms; // the term leaves of the fragment's TASK_TREE queries
                uint32_t n_hidden = 0;            // hidden phrase queries (Tmp::hidden_ord)
                uint64_t off = 0;
                // bases in the batch's arrays (settled between the passes)
                size_t b_plan = 0, b_qterms = 0, b_sterms = 0, b_phrases = 0, b_pterms = 0, b_tasks = 0, b_fused = 0, b_ptasks = 0, b_units = 0, b_tree = 0, b_hidden = 0;
                uint64_t b_off = 0;
                int rc = TRI_OK;
                std::string err;
                // A fragment of an earlier plan as a fresh one that keeps its buffers: every field takes its default, the vectors named below come back
                // EMPTY with their capacity (a vector not named here is simply allocated anew — never stale).  A caller that compiles a batch per step
                // otherwise mallocs, grows by doubling and page-faults about 10 MB of fragment arrays per plan (cfg2, one thread: 8.0 -> 6.4 ms of
                // planning with the memory recycled)
                void recycle() {
                        Frag fresh;
                        auto keep = [](auto &dst, auto &src) {
                                src.clear();
                                dst = std::move(src);
                        };
                        keep(fresh.S.nodes, S.nodes), keep(fresh.S.kidpool, S.kidpool), keep(fresh.S.st, S.st), keep(fresh.S.tmpk, S.tmpk), keep(fresh.S.cs, S.cs);
                        keep(fresh.S.gt, S.gt), keep(fresh.S.gs, S.gs), keep(fresh.S.gorder, S.gorder), keep(fresh.S.leaves, S.leaves), keep(fresh.S.leaf_tok, S.leaf_tok);
                        keep(fresh.S.negs, S.negs), keep(fresh.S.opts, S.opts), keep(fresh.S.opt_tok, S.opt_tok), keep(fresh.S.ts, S.ts), keep(fresh.S.ts_tok, S.ts_tok);
                        keep(fresh.S.u, S.u), keep(fresh.S.uniq, S.uniq), keep(fresh.S.rt, S.rt), keep(fresh.S.seen, S.seen), keep(fresh.S.phterms, S.phterms);
                        keep(fresh.S.slots, S.slots), keep(fresh.S.qphrases, S.qphrases), keep(fresh.S.sc, S.sc);
                        keep(fresh.tmp, tmp), keep(fresh.qterms, qterms), keep(fresh.pterms, pterms), keep(fresh.sterms, sterms), keep(fresh.sweights, sweights);
                        keep(fresh.phrases, phrases), keep(fresh.fz, fz), keep(fresh.left_out, left_out), keep(fresh.tasks, tasks), keep(fresh.tcost, tcost);
                        keep(fresh.fused, fused), keep(fresh.ptasks, ptasks), keep(fresh.units, units), keep(fresh.quses, quses), keep(fresh.suses, suses);
                        keep(fresh.fuses, fuses), keep(fresh.benefit, benefit), keep(fresh.cand_row, cand_row), keep(fresh.keys, keys), keep(fresh.hist, hist), keep(fresh.treepool, treepool);
                        keep(fresh.tree_terms, tree_terms);
                        *this = std::move(fresh);
                }
        };
        // the fragments of a caller's earlier plans (tri_dev keeps one; plan_batch takes what it needs out of it and puts it back)
        struct FragCache {
                std::vector<Frag> frags;
        };

        struct Ctx {
                const HostIndex &ix;
                const PlanEnv &env;
                const PlanInput &in;
                bool scored, rich;
                uint32_t mode;
                // term planes: a term is eligible when its df rank is below n_ok
                uint32_t n_ok = 0;
                bool plane_ok(uint32_t term) const { return ix.df_rank[term] < n_ok; }
                // settled after the first pass
                uint64_t planes_split = 2, fused_task_cost = 0, phrase_task_div = 1;
                uint32_t plw = 0; // words of a bitmap over the docID space (BatchPlan::plw)
                // the ScorerWeight contribution of one term (IndexSourceTermsScorer::new_scorer_weight sums it over a phrase's terms):
                // BM25 similarity.h:179-181 (float math), TF-IDF :85-87 (double), Trivial has none
                double term_weight(const uint32_t df) const {
                        if (in.similarity == TRI_SIM_TFIDF)
                                return std::log((double)((uint64_t)ix.info.docs_cnt + 1) / (double)(df + 1)) + 1.0;
                        if (in.similarity == TRI_SIM_TRIVIAL)
                                return 0.0;
                        const float num = (float)((uint64_t)ix.info.docs_cnt - (uint64_t)df) + 0.5f;
                        const float den = (float)df + 0.5f;
                        return (double)std::log(1 + num / den);
                }
                // first block of `t` whose last docID >= key: the docID-cell index when the list has one and key is a cell boundary (every
                // window boundary is), else a search of the directory column
                uint32_t first_block_ge(const DevTerm &t, const uint64_t key) const {
                        if (t.win_off != 0xffffffffu && !ix.win.empty() && !(key & (CELL_DOCS - 1)) && (key >> CELL_LOG2) < ix.nwin)
                                return ix.win[t.win_off + (key >> CELL_LOG2)];
                        const uint32_t *lb = &ix.blk_last[t.first_block];
                        return (uint32_t)(std::lower_bound(lb, lb + t.nblocks, (uint32_t)std::min<uint64_t>(key, 0xffffffffull)) - lb);
                }
        };

        // ---- helpers the lowering, the task cutter and the fill pass share
        // the docbytes of the DISTINCT terms among terms[0, n) (QT_ marks ignored); `seen` is scratch
        inline uint64_t distinct_docbytes(const HostIndex &ix, const uint32_t *terms, const size_t n, std::vector<uint32_t> &seen) {
                uint64_t bytes = 0;
                seen.clear();
                for (size_t k = 0; k < n; ++k) {
                        const uint32_t term = terms[k] & QT_TERM;
                        if (std::find(seen.begin(), seen.end(), term) == seen.end()) {
                                seen.push_back(term);
                                bytes += ix.docbytes[term];
                        }
                }
                return bytes;
        }
        // the unit record of task `tix` (TASK_PSET: windows [begin, end); TASK_PROBE: lead tiles) of query q, whose terms are qt[]: fragment-relative
        // like the task (row[] is filled once the planes are chosen)
        inline DevPsetUnit make_unit(const DevQuery &q, const uint32_t *qt, const uint32_t tix, const uint32_t begin, const uint32_t end, const uint64_t out_off, const uint32_t first) {
                DevPsetUnit u{};
                u.out_off = out_off;
                u.first = first;
                u.w_begin = begin, u.w_end = end;
                u.tix = tix;
                u.nterms = q.nterms;
                u.term_base = q.term_base;
                for (uint32_t k = 0; k < q.nterms && k < PSET_INLINE_TERMS; ++k)
                        u.tt[k] = qt[k];
                return u;
        }
        // fn(term) for the known terms among the first 16 tokens of caller query q's program (the prefetch walks of lower_range)
        template <class Fn>
        inline void for_each_term_token(const HostIndex &ix, const PlanInput &in, const size_t q, Fn &&fn) {
                const tri_query &t = in.queries[q];
                if ((uint64_t)t.prog_off + t.prog_len > in.prog_len)
                        return;
                for (uint32_t i = 0; i < t.prog_len && i < 16; ++i) {
                        const uint32_t tok = in.prog[t.prog_off + i];
                        const uint32_t x = tok & 0x0fffffffu;
                        if ((tok >> 28) == TRI_OP_TERM && x < ix.terms.size())
                                fn(x);
                }
        }
        // (the per-term records a query's lowering and cutting read, at term ids drawn from a vocabulary of millions)
        inline void prefetch_term(const HostIndex &ix, const uint32_t x) {
                __builtin_prefetch(&ix.terms[x]);
                __builtin_prefetch(&ix.docbytes[x]);
                __builtin_prefetch(&ix.df_rank[x]);
        }

        inline double ms_since(std::chrono::steady_clock::time_point &t0) {
                const auto now = std::chrono::steady_clock::now();
                const double ms = std::chrono::duration<double, std::milli>(now - t0).count();
                t0 = now;
                return ms;
        }
} // namespace trip

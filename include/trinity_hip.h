/*
 * trinity_hip.h — C-ABI of libtrinity_hip.so, the MI355X (gfx950) execution engine for Trinity's
 * query hot path: postings decode -> docset intersection/union -> per-document BM25 -> top-K.
 *
 * Plain C: opaque handles, plain pointers and sizes, int status codes.  Nothing throws across this
 * boundary.  Every entry point names the reference interface (file:line under the reference tree)
 * whose work it takes over; INTEGRATION.md shows the binding a Trinity maintainer would add.
 *
 * Threading: one tri_dev per (host thread, device) — with ONE exception, made for a caller that keeps the engine stream fed: while one
 * thread runs, awaits, reads and destroys batches of a device (tri_batch_run / _sync / the result calls / _destroy), other threads may
 * compile the next ones (tri_batch_create) on the same device; the handle's pools, the index's plane cache and everything that enqueues on
 * its streams are locked for that.  The result calls keep ONE rule: a result copy of a synced batch is enqueued on the handle's read-back stream
 * under that lock and awaited OUTSIDE it — no result call touches the engine stream, none holds the lock while it waits, so a read waits for nothing
 * queued behind its batch and holds up no thread that compiles or runs the next one.  The host planner — most of a create — runs outside that lock, in one of the handle's TWO planner
 * contexts (a pool of host threads each): two creates plan side by side, a third waits for a context.  Everything else (uploads, options,
 * the write side) stays one thread at a time.  tri_last_error() is per thread.
 */
#ifndef TRINITY_HIP_H
#define TRINITY_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRI_ABI_VERSION 9 /* 2: tri_batch_info grew (fused_*), tri_dev_set_option / tri_dev_get_option; 3: TRI_OP_SOME, tri_batch_info.cand_needed_bytes / phrase_*;
                             4: tri_batch_info grew (term planes, k_planes), tri_batch_query_status, tri_comm_create_custom; 5: tri_encode_google_payloads;
                             6: tri_batch_info.create_ms / create_plan_ms / *_bound_bytes, options plane_max_bytes / plan_threads, tri_cbatch_query_status;
                             7: TASK_TREE (any query tree), tri_batch_info.tree_ms / tree_queries / tree_scratch_bytes, tri_commit_* / tri_merge_google;
                             8: tri_batch_docsets (every query's docID set in one call), tri_merge_lucene, option planes_rebuild;
                             9: tri_dev_memory (HBM in use), tri_batch_docsets_mixed (dense sets delivered as bitmap words), two planner contexts per handle (two threads may compile at once), plane rows built by need;
                                within 9: tri_filter_create / tri_filter_from_docset / tri_filter_destroy / tri_batch_set_filters (per-query document filters on the device);
                                within 9: options tree_max_nodes / tree_wide_min_nodes (query trees of up to 1024 nodes; no new export, no struct grew);
                                within 9: option rich_max_terms, tri_batch_query_terms_wide / tri_batch_matched_terms_wide (the default mode reports up to 64 matched terms per query; no struct grew);
                                within 9: tri_decode_hits / tri_decode_hits_at (the codec seam's materialize_hits: the hits of whole lists and of chosen documents; no struct grew);
                                within 9: tri_batch_set_ranker / tri_batch_ranked (the default mode ranks its matches on the device: a proximity score, top-K per query; no struct grew),
                                tri_cbatch_ranked / tri_cbatch_matched_terms[_wide] / tri_cbatch_matched_payloads (the default mode over a collection);
                                within 9: tri_isect_run / _status / _results / _histogram / _get_info / _destroy, options isect_max_bytes / isect_max_masks / isect_max_runs
                                (Trinity::intersect: token-set co-occurrence counts; no existing struct grew);
                                within 9: tri_perc_create / _query_status / _set_enabled / _get_info / _destroy / _match, tri_perc_result_pairs / _doc_counts / _get_info / _destroy,
                                options perc_max_bytes / perc_prune (the percolator: documents matched against a resident set of stored queries; no existing struct grew);
                                within 9: tri_encode_lucene_payloads / tri_commit_lucene_payloads (the Lucene-shaped codec carries hit payloads: written, merged by
                                tri_merge_lucene, read by tri_decode_hits[_at] and tri_batch_matched_payloads; no struct grew);
                                within 9: tri_column_create / tri_column_destroy / tri_batch_set_facets / tri_batch_facets / tri_cbatch_facets, read-only option facet_last_us
                                (facet counts: per query a histogram of its docID set over per-document columns, counted on the device; no existing struct grew);
                                within 9: tri_batch_set_order / tri_batch_ordered / tri_cbatch_ordered, read-only option order_last_us
                                (order by a column: per query the first topk documents of its docID set by a column's value, selected on the device; no existing struct grew);
                                within 9: tri_batch_set_stats / tri_batch_stats / tri_cbatch_stats, read-only option stats_last_us
                                (stats of a column: per query and bucket the count, sum, min and max of a value column over the docID set, aggregated on the device; no existing
                                struct grew);
                                within 9: tri_filters_from_columns / tri_filter_bitmap (column predicates as document filters: RANGE / SET clauses over resident columns
                                become drop bitmaps on the device; any filter's bitmap read back; no existing struct grew) */

/* status codes */
#define TRI_OK 0
#define TRI_ERR_INVALID (-1)     /* bad argument / malformed program   (reference: Switch::invalid_argument) */
#define TRI_ERR_DEVICE (-2)      /* HIP runtime error                  */
#define TRI_ERR_UNSUPPORTED (-3) /* query shape not lowered yet        */
#define TRI_ERR_FORMAT (-4)      /* index bytes fail validation        (reference: Switch::data_error)      */
#define TRI_ERR_NOMEM (-5)
#define TRI_ERR_INTERNAL (-6)    /* the engine contradicts itself (a result block that does not add up): a bug, never a caller's error */

/* docIDs.  A segment may hold any ascending docIDs 1 .. 2^32 - 2 (tri_index_upload refuses only block deltas that run past 2^32); the bitmaps over the docID
 * space (term planes, masked documents, filters, result bitmaps) extend (max docID / 131072 + 2) * 4096 words, 512 MiB each at the top.  What the engine enforces
 * or decides by the segment's largest docID:
 *   - tri_isect_run: TRI_ERR_UNSUPPORTED for the whole call when the index's docIDs reach 2^31;
 *   - AccumulatedScore top-K in one pass: the bit-plane kernel takes queries only on segments whose largest docID is below 0x7fff0000, the window-word kernel
 *     only below 0xffffc000 (its last window would end past 2^32); from there on scored queries run match-then-score (tri_batch_info::cand_queries / dense_queries /
 *     pset_queries instead of ::planes_queries / ::fused_queries);
 *   - a query that only the window-word kernel takes (a matchsome or another general tree over at most eight distinct terms, in every mode) is LEFT OUT on a segment
 *     whose largest docID is 0xffffc000 or more: tri_batch_query_status TRI_ERR_UNSUPPORTED, tri_last_error names the limit;
 *   - DocumentsOnly unions of head terms and rare ones are scattered into a result bitmap only while the union's last document lies below 2^31 (4096 tasks of
 *     four 131072-document windows); from there on they run as bitmap windows and their result is ascending docIDs (tri_batch_docset_bitmap: form 0).
 * Only the third of these leaves a query out. */

/* codecs (segment `id` file codec name: indexer.cpp:266-270, segment_index_source.cpp:172-179) */
#define TRI_CODEC_GOOGLE 1
#define TRI_CODEC_LUCENE 2

/* exec.h:11-43 ExecFlags (same values) */
#define TRI_FLAG_DOCUMENTS_ONLY 1u
#define TRI_FLAG_ACCUMULATED_SCORE 2u
#define TRI_FLAG_HIT_PAYLOADS 8u  /* with TRI_FLAG_MATCHED_TERMS: every hit also comes with term_hit::payloadLen and ::payload (runtime.h:8-20) as
                                     Google::Decoder::materialize_hits leaves them (google_codec.cpp:533-594): tri_batch_matched_payloads */
#define TRI_FLAG_MATCHED_TERMS 4u /* exec_query's DEFAULT mode (no ExecFlags, exec.cpp:1350-1501): every match comes with the query
                                     terms that matched it and their hits — what consider(const matched_document &) receives
                                     (matches.h:109-130; queryexec_ctx.cpp:382-648).  Results: tri_batch_matched_terms */

/* similarity.h scorers: Trivial :56-72, TF-IDF :75-163, BM25 :165-255 */
#define TRI_SIM_BM25 0
#define TRI_SIM_TFIDF 1
#define TRI_SIM_TRIVIAL 2

/* postfix query program tokens: (op << 28) | arg.  The host-side planner (the mirror of
 * queryexec_ctx::build_iterator, exec.cpp:253-449) emits these from its iterator tree. */
#define TRI_OP_TERM 0u   /* arg = index into the uploaded term table                              */
#define TRI_OP_AND 1u    /* arg = #children   (DocsSetIterators::Conjuction[AllPLI])              */
#define TRI_OP_OR 2u     /* arg = #children   (DocsSetIterators::Disjunction[AllPLI] / union span) */
#define TRI_OP_PHRASE 3u /* arg = #terms, the preceding arg tokens are TERMs (DocsSetIterators::Phrase) */
#define TRI_OP_NOT 4u    /* operand = 2: the two preceding sub-programs are (required, excluded) — exec.cpp:424-427 logicalnot -> DocsSetIterators::Filter.
                            Lowered: NOT at the root or under AND, excluded side = a term or an OR of terms */
#define TRI_OP_OPT 5u    /* operand = 2: (main, optional) — consttrueexpr under an AND (`a <b>`) -> DocsSetIterators::Optional, exec.cpp:366-377: the
                            documents of main; the optional side (a term or an OR of terms) only adds its score / its matched terms */
#define TRI_OP_SOME 6u   /* operand = (min << 16) | #children — matchsome `[a, b, ...]` with a threshold -> DocsSetIterators::DisjunctionSome,
                            exec.cpp:276-283, docset_iterators.cpp:679-811: the documents at least `min` of the children match */
#define TRI_TOK(op, arg) (((uint32_t)(op) << 28) | ((uint32_t)(arg)&0x0fffffffu))

typedef struct tri_dev tri_dev;
typedef struct tri_index tri_index;
typedef struct tri_batch tri_batch;

/* == Trinity::term_index_ctx {documents, indexChunk{offset,len}} (codecs.h:17-55) */
typedef struct tri_term {
        uint32_t documents;
        uint32_t offset;
        uint32_t size;
} tri_term;

/* one query = a slice of the shared postfix program */
typedef struct tri_query {
        uint32_t prog_off;
        uint32_t prog_len;
} tri_query;

typedef struct tri_index_info {
        uint64_t index_bytes;    /* raw `index` bytes resident in HBM                                  */
        uint64_t directory_bytes; /* per-block directory built at upload                                */
        uint64_t blocks;
        uint64_t postings;       /* sum of documents over terms (field_statistics::sumTermsDocs)       */
        uint64_t doc_bytes;      /* header + delta + freq bytes of every chunk            */
        uint64_t hit_bytes;
        uint32_t nterms;
        uint32_t docs_cnt;
} tri_index_info;

typedef struct tri_batch_info {
        uint64_t nqueries;
        uint64_t algorithmic_bytes; /* sum_q [ sum_t docbytes(t) + out(q) ] of the LAST run */
        uint64_t matches;           /* total matches of the last run                                    */
        uint64_t out_capacity;      /* docID slots reserved for docsets                                 */
        float last_run_ms;          /* HIP-event time of the last tri_batch_run (kernels only)          */
        uint32_t launches;          /* kernel launches per run                                          */
        /* per matching kernel (HIP events on the engine stream around each launch; algorithmic bytes of the queries
         * each one processes): k_and_dense = bitmap windows, k_and = candidate tiles */
        float dense_ms, cand_ms;
        uint64_t dense_algorithmic_bytes, cand_algorithmic_bytes;
        uint64_t dense_queries, cand_queries;
        /* k_fused: AccumulatedScore top-K of dense queries in one pass (decode -> match -> score -> select per docID window) */
        float fused_ms, rest_ms; /* rest_ms: everything after the matching kernels and k_phrase (k_rich, k_score, k_topk_merge) */
        uint64_t fused_algorithmic_bytes;
        uint64_t fused_queries;
        /* k_and skips: its algorithmic bytes are no bound.  With the option account_needed_bytes = 1 at batch creation: the bytes a perfect
         * gallop must read for the candidate-tile queries — the lead lists, of every other list the blocks that can hold a lead candidate
         * (per lead block: the blocks its docID range meets, at most one per candidate; docbytes / nblocks each), + 4 B per match.  0: not asked */
        uint64_t cand_needed_bytes;
        /* k_phrase (positional constraints over the match segments): its time, the hit bytes of the phrases' terms (their SURVEY §8(d) share of
         * algorithmic_bytes — no longer counted under cand_algorithmic_bytes), the queries that hold a phrase; rest_ms no longer includes it */
        float phrase_ms, tree_ms; /* tree_ms (ABI 7): the TASK_TREE kernels (k_tree.hpp) — until then part of rest_ms */
        uint64_t phrase_algorithmic_bytes;
        uint64_t phrase_queries;
        /* term planes: the head terms the batch's queries share are decoded ONCE per launch (k_term_planes, first kernel of the run) into
         * two bitmaps over the docID space each (A: holds the term; B: frequency != 1), which k_and probes, k_and_dense ORs into its windows
         * and k_planes — AccumulatedScore top-K of CNF queries, predicates evaluated 32 documents per word — reads instead of decoding the
         * list again for every query that names it.  plane_terms: how many; plane_bytes: their scratch; term_planes_decoded_bytes: the
         * docbytes of those lists (read once per launch).  dense_ms no longer includes the launch's first memset: term_planes_ms does */
        float term_planes_ms, planes_ms;
        uint64_t planes_algorithmic_bytes; /* SURVEY §8(d) bytes of the queries k_planes runs (per query, as if every list were read) */
        uint64_t planes_queries;
        uint64_t plane_terms, plane_bytes, term_planes_decoded_bytes;
        uint64_t unsupported_queries; /* queries the planner left out of the batch (tri_batch_query_status) */
        /* what tri_batch_create itself took: all of it (host planning on the handle's host threads + arena / pool bookkeeping + enqueueing the plan's
         * one copy on the upload stream), and the host planner's share */
        float create_ms, create_plan_ms;
        /* With the option account_needed_bytes = 1 at creation (else 0): the BATCH-LEVEL bound — a batch that shares decodes must read every
         * DISTINCT list its queries name once (doc bytes; hit bytes of the distinct phrase / reported terms) and write every output once
         * (4 B per match, or 8 B x min(matches, K) when scored): bound_bytes for the whole batch, *_bound_bytes for the queries each kernel
         * runs (distinct lists of THOSE queries + their output; k_phrase: the distinct phrase terms' hit bytes).  SURVEY §8(d)'s per-query
         * count (algorithmic_bytes) charges a list once per query that names it, which no kernel that shares decodes reads */
        uint64_t bound_bytes, dense_bound_bytes, cand_bound_bytes, fused_bound_bytes, planes_bound_bytes, phrase_bound_bytes;
        /* k_psets: the bitmap-window queries ALL of whose terms have a term plane (word-wise algebra over the planes, then the expansion into
         * docIDs) — until ABI 6 part of k_and_dense's figures: its time, queries, SURVEY §8(d) bytes and batch-level bound */
        float pset_ms;
        /* k_probe: one short lead list against lists that all have a term plane (a wave decodes the lead's blocks into registers and tests every
         * document with one bit probe per list) — until ABI 6 part of k_and's figures */
        float probe_ms;
        uint64_t pset_queries, pset_algorithmic_bytes, pset_bound_bytes;
        uint64_t probe_queries, probe_algorithmic_bytes, probe_bound_bytes;
        /* TASK_TREE (ABI 7): the queries evaluated as set algebra over one bitmap per leaf (k_tree.hpp) — a multi-word phrase under OR / NOT /
         * matchsome / <optional>, trees over more distinct terms than the truth-table kernel holds, CNFs of more than 16 terms; the bitmap
         * scratch their leaves and match sets take (option tree_max_bytes bounds it: TRI_ERR_NOMEM, split the batch) */
        uint64_t tree_queries, tree_scratch_bytes;
        /* queries whose docID set the engine holds as a bitmap (ABI 7; DocumentsOnly unions / conjunctions of head terms expected to match one
         * document in 32 or more — option result_bitmaps, default 1): tri_batch_docset expands them on read-back, tri_batch_docset_bitmap hands
         * the words over; match counts, hashes and everything else read the same */
        uint64_t bitmap_queries;
} tri_batch_info;

const char *tri_last_error(void);
int tri_abi_version(void);

/* ---- device --------------------------------------------------------------------------------------- */
int tri_dev_open(int device, tri_dev **out);
void tri_dev_close(tri_dev *);
int tri_dev_sync(tri_dev *);
/* the engine's HIP stream (hipStream_t as void*), for callers that order their own work against it */
void *tri_dev_stream(tri_dev *);
/* Planner / launch options of this device handle; they apply to batches created afterwards.  The reference has no counterpart (its
 * planner's constants are compiled in, exec.cpp:35-110); these are the thresholds of the GPU planner:
 *   "dense_min_postings"  a multi-term query runs as bitmap / score windows when its lists hold at least this many postings (default 524288;
 *                         0 = every query whose lists allow it)
 *   "dense_task_cost"     postings per bitmap-window task (default 196608)
 *   "fused"               1 (default): AccumulatedScore top-K batches run their dense queries through the one-pass kernel; 0: match, then score
 *   "fused_task_cost"     postings per one-pass task (default 0: sized from the batch — 256 K .. 8 M, about two tasks per resident workgroup)
 *   "fused_freq_cap"      0 (default): a window field saturates at the largest freq its width holds; else at this freq (documents above it are
 *                         rescored from the postings — same results, slower)
 *   "fused_halfwords"     1 (default): one-pass queries of <= 5 distinct terms keep 16 bits per document (windows twice as long); 0: 32
 *   "overlap_dense_wgs" / "overlap_cand_wgs"  both non-zero: the two matching kernels run side by side with that many workgroups per CU
 *   "planes"              term planes, a bit set (default 7): 1 the candidate-tile kernel probes them, 2 the bitmap-window kernel ORs them into its
 *                         windows, 4 AccumulatedScore top-K CNF queries run over bit planes (k_planes); 0: every query decodes every list it names
 *   "planes_split"        a query that runs as bit planes (k_planes) is cut into this many docID ranges, one task each (default 0: two, or three in a batch that brings few tasks per workgroup; 65536 and up: cut by postings like k_fused's); the
 *                         ranges share the query's threshold, results do not depend on the cut
 *   "plane_div"           a term gets a plane when it holds at least docs_cnt / plane_div documents (default 1024) and the batch's uses repay one
 *                         decode of its list
 *   "account_needed_bytes" 1: tri_batch_create also works out tri_batch_info.cand_needed_bytes (a directory walk per candidate-tile query; default 0)
 *   "plane_max_bytes"     scratch budget of a batch's term planes (default 8 GiB): the terms eligible for a plane are the longest lists that fit
 *   "planes_rebuild"      1: every tri_batch_run decodes the plane rows its batch names again — a COLD plane cache, what a query stream whose head
 *                         terms were all just evicted pays per batch (default 0: a row is built once per index); a measurement switch, read by tri_batch_run
 *   "cand_xcd"            1 (default): the candidate-tile kernel's tasks are queued per XCD by the plane row they probe — a row's probes land in ONE 4 MB L2
 *                         (csrc/planner.hpp, "k_and's queues"); 0: the heaviest-first order dealt round the queues.  Results do not depend on it
 *   "probe_max_blocks"    > 0: a conjunction of ONE lead list of at most this many blocks with lists that all have planes runs in k_probe (a wave per
 *                         task, csrc/k_probe.hpp) instead of candidate tiles (default 0: off — measured slower at cfg2, planner_types.hpp)
 *   "overlap"             1: the candidate-tile kernel runs on a second stream beside the window kernels (default 0; measured: no gain, the persistent
 *                         grids do not interleave)
 *   "plan_threads"        host threads tri_batch_create plans large batches with (default 0: up to 16, by the host's cores; 1: the calling thread
 *                         only).  The threads belong to the handle, are pinned to distinct CPUs next to the creating thread's, and keep polling for
 *                         about 3 ms after a batch before they sleep (csrc/host_pool.hpp says why); read when the first large batch is created
 *   "tree_max_nodes"      a query tree of more than this many nodes is left out of the batch (TRI_ERR_UNSUPPORTED per query).  Default 64: what the narrow tree
 *                         kernels hold (csrc/k_tree.hpp).  64 .. 1024: trees above 64 nodes — a flat OR of 70 terms, an AND of 22 three-term ORs, a matchsome
 *                         over 100 alternatives — run in the wide tree kernels (csrc/k_tree_wide.hpp).  Any other value fails tri_batch_create with
 *                         TRI_ERR_INVALID.  Still left out: a tree whose evaluation needs more than 64 stack words (a word per nested AND / OR / NOT /
 *                         <optional> on the deepest path, ceil(log2(children + 1)) per nested matchsome), more reportable terms in the default mode than option
 *                         rich_max_terms allows
 *   "rich_max_terms"      default mode (TRI_FLAG_MATCHED_TERMS): a query of more reportable terms than this is left out of the batch (TRI_ERR_UNSUPPORTED per
 *                         query).  Default 16; 16 .. 64, any other value fails tri_batch_create with TRI_ERR_INVALID.  A query of 17 .. 64 reportable terms
 *                         (a WIDE-REPORT query: a flat OR of 20 synonyms, an OR of 40 two-term conjunctions, a matchsome over 60 alternatives) runs as a
 *                         tree query and is read through tri_batch_query_terms_wide / tri_batch_matched_terms_wide.  Off by default because of what such
 *                         a query reserves: 2 x (its terms rounded up to 8) bytes of frequency row + 8 bytes of masks per OUTPUT SLOT — the tree's upper
 *                         bound, not its matches: up to 136 bytes a slot; a flat OR of 64 head terms over 10 M documents reserves on the order of 1.3 GB.  A
 *                         create that cannot get the memory fails with TRI_ERR_NOMEM.  Batches whose queries all report at most 16 terms are unaffected
 *   "tree_wide_min_nodes" a tree query of at least this many nodes runs in the wide kernels (default 65: only the trees the narrow ones cannot hold; 0: every
 *                         tree query).  Results do not depend on it; it is there so that the wide kernels can be checked on trees with pinned answers
 *   "phrase_task_div"     the tasks of a query with phrases are cut this many times finer than a phrase-less query's: window tasks, plane-set tasks (at
 *                         least one window each) and candidate-tile tasks — they are the phrase kernel's tasks too, and its span is its longest task.
 *                         Default 0: by the batch's phrase queries per compute unit — 4 up to 8 a unit, 2 up to 16, else 1.  Results do not depend on it
 *   "dense_window_cost"   a docID window of a bitmap-window task counts this many postings whatever it holds, which bounds the windows per task of
 *                         queries over rare lists (default 16384; 0: such a task takes as many windows as dense_task_cost allows).  Results do not depend on it
 *   "scatter_bitmap_slack" a DocumentsOnly union of head terms with terms that have no plane runs over the planes — the other terms' documents set bit by
 *                         bit, the result a bitmap — when min(docs_cnt, its head terms' documents) x this value >= the 32-bit words of a bitmap over the
 *                         query's docID windows (default 4; 1: only where the bitmap is no larger than the docID list; 0 reads as 1).  The other such unions run
 *                         in the bitmap-window kernel and deliver ascending docIDs.  The docID sets do not depend on it; a result's FORM does
 *   "pset_order"          1 (default): the plane-set kernel's tasks run docID range by range, within a range by the query's heaviest term; 0: in batch order
 *                         within a range.  Results do not depend on it
 *   "planes_order"        the bit-plane kernel's (k_planes) tasks: 1 (default) docID range by range, within a range by the heaviest plane row; 2: row by row,
 *                         a query's ranges side by side; 0: heaviest task first.  A query's ranges share one threshold; results do not depend on the order
 *   "tree_max_bytes"      scratch budget of a batch's tree queries (default 16 GiB).  A batch needs (distinct term leaves x PL_PLANES + phrase leaves + tree
 *                         queries) x plane words x 4 bytes (tri_batch_info.tree_scratch_bytes); a batch that needs more fails tri_batch_create with
 *                         TRI_ERR_NOMEM and takes nothing from the handle's pool; one that needs exactly the budget is created
 * ("fused" also takes 2: only pure unions run in one pass.)  The options are read when a batch is CREATED, except "overlap", the two overlap_*_wgs ones and
 * planes_rebuild, which tri_batch_run reads (they change how existing batches are launched).  Unknown names fail with TRI_ERR_INVALID. */
int tri_dev_set_option(tri_dev *, const char *name, uint64_t value);
int tri_dev_get_option(tri_dev *, const char *name, uint64_t *value);

/* What the handle holds of the device's memory (no reference counterpart: Trinity mmaps its segments and mallocs per query — queryexec_ctx.cpp:187-249).
 * pool_*: the handle's buffer pool — batches' arenas, output regions, score streams, the indexes' plane caches; in use / idle (idle buffers go back to
 * the device beyond 64 GiB, or when an allocation fails).  device_*: hipMemGetInfo — everything on the device, other processes' memory included. */
typedef struct {
        uint64_t pool_in_use_bytes, pool_idle_bytes, pinned_idle_bytes;
        uint64_t device_free_bytes, device_total_bytes;
} tri_dev_memory_info;
int tri_dev_memory(tri_dev *, tri_dev_memory_info *out);

/* ---- index upload ---------------------------------------------------------------------------------
 * Replaces SegmentIndexSource's mmap of `index` (segment_index_source.cpp:84-93) + per-query
 * Codecs::Google::Decoder::init (google_codec.cpp:936-983): copies the segment's raw codec bytes to HBM
 * once and materialises a dense per-block directory {payload offset, last docID} (the analogue of the
 * decoder materialising its skiplist) plus a device term table.  `terms[i]` is what
 * IndexSource::resolve_term_ctx (index_source.h:103) returns for term i.
 * `hits`/`hits_len` are the Lucene codec's hits.data (lucene_codec.h:206); NULL/0 for GOOGLE. */
int tri_index_upload(tri_dev *, const uint8_t *index, size_t len, const uint8_t *hits, size_t hits_len, int codec,
                     const tri_term *terms, size_t nterms, uint32_t docs_cnt, tri_index **out);
void tri_index_destroy(tri_index *);
int tri_index_get_info(const tri_index *, tri_index_info *);
/* algorithmic doc bytes (SURVEY §8d docbytes(t)) of the given terms */
int tri_index_term_docbytes(const tri_index *, const uint32_t *terms, size_t n, uint64_t *out);

/* Masked documents of this segment: documents updated or deleted by newer segments, which exec_query drops right before
 * consider() — masked_documents_registry::test (docidupdates.h:90-119; exec.cpp:914-975, 1000-1030).  Replaces the set
 * (any order, duplicates allowed; n == 0 clears it).  Kept on the device as a bitmap over docIDs and applied inside the
 * matching kernels, so match counts, docsets, scores and top-K of batches run afterwards never contain a masked document.
 * Batches created before the call keep working; the set they see is the one in place when they RUN. */
int tri_index_set_masked(tri_index *, const uint32_t *docids, size_t n);

/* ---- per-query document filters --------------------------------------------------------------------
 * exec_query's IndexDocumentsFilter (matches.h:190-201): the application rules documents out BEFORE they are considered — an ACL, a tenant, a category,
 * a date range expressed as a docID set —, tested in addition to the masked documents (exec.cpp:1133-1150: the match handler hands a document to
 * consider(), and counts it, only when documentsFilter->filter(id) is false).  On the device a filter is a bitmap over the segment's docIDs, and every query of a
 * batch may name one: the matching kernels drop, for query q, the documents of the index's masked set as it stands when the batch RUNS and those of q's
 * filter, at the one place they test the mask today — DocumentsOnly sets, match counts, hashes, scores, top-K lists and the default mode's matched terms
 * never see a dropped document, so the K slots of a top-K go to documents the application would have kept.
 *
 * tri_filter_create: docids in any order, duplicates allowed, n == 0 legal, IDs above the segment's largest document ignored.  mode TRI_FILTER_DROP: docids =
 * the documents IndexDocumentsFilter::filter() returns true for; TRI_FILTER_KEEP: the only documents a query may match (an allow-list; complemented when the
 * bitmap is built).  tri_filter_from_docset: the filter is the docID set of query q of a synced DocumentsOnly batch, taken on the device in the form the
 * engine holds it (docIDs or bitmap); it belongs to the batch's index and outlives the batch.  Both return once the bitmap stands.  A filter is destroyed
 * before its index, and kept alive while a batch that names it may run — the rule batches follow towards their index.
 * tri_batch_set_filters: after tri_batch_create, before a run, again between runs; filters[] are stored by reference; filter_of_query[q] < nf names query
 * q's filter, 0xffffffff none; nf == 0 clears.  A filter of another index or an index >= nf is TRI_ERR_INVALID and changes nothing.  Runs already queued
 * keep the assignment they were launched with.  The parts of a tri_cbatch each carry their own filters. */
typedef struct tri_filter tri_filter;
#define TRI_FILTER_DROP 0 /* docids = the documents IndexDocumentsFilter::filter() returns true for */
#define TRI_FILTER_KEEP 1 /* docids = the only documents a query may match (allow-list)             */
int tri_filter_create(tri_index *, const uint32_t *docids, size_t n, int mode, tri_filter **out);
int tri_filter_from_docset(tri_batch *, size_t q, int mode, tri_filter **out);
void tri_filter_destroy(tri_filter *);
int tri_batch_set_filters(tri_batch *, tri_filter *const *filters, size_t nf, const uint32_t *filter_of_query /* [nq], 0xffffffff: none */);

/* ---- facet counts ----------------------------------------------------------------------------------
 * The third thing an application does in MatchedIndexDocumentsFilter::consider(id) / consider(ids, cnt) (exec.h:12-23: "just count or collect documents
 * matching a query") besides collecting and ranking: COUNT the matches by a per-document attribute — category, brand, price band, tenant.  A column holds
 * that attribute for every docID of a segment and stays resident in HBM; a batch that names columns (facets) counts, at the end of every run and on the
 * device, each query's docID set into a row per facet: a few hundred bytes a query cross PCIe instead of the docID set.
 *
 * tri_column_create: values[d] is the attribute of docID d; n must equal the index's docs_cnt + 1 (values[0] is never read), and the index may hold no docID
 * above docs_cnt.  The values are copied to HBM; the call returns once the column stands.  A column belongs to its index, is destroyed before it, and is kept
 * alive while a batch that names it may run — the filters' rules.
 * tri_batch_set_facets: after tri_batch_create, before a run, again between runs; n == 0 clears; columns are stored by reference.  Runs already queued keep the
 * specs they were launched with (the call waits for them before the rows they count into are released).  The rows of ALL facets live in one block taken from the
 * handle's buffer pool: nq x sum over the facets of (nbuckets + 1) x 4 bytes (+ 64 KB, the pool's smallest buffer), in caller query order (hidden phrase-leaf queries have no row) —
 * TRI_ERR_NOMEM when it cannot be had.  TRI_ERR_INVALID, nothing changed: a null column, a column of another index, n > TRI_FACETS_MAX, nbuckets of 0 or
 * above TRI_FACET_MAX_BUCKETS, reserved != 0, a batch created with TRI_FLAG_ACCUMULATED_SCORE (its one-pass queries keep no docID sets).  The parts of a
 * tri_cbatch each carry their own facets.
 * Every later tri_batch_run zeroes the block and counts again, on the engine stream behind the kernels that complete the docID sets (one more launch per run;
 * a batch without facets launches nothing more); the rows stand after tri_batch_sync.
 * tri_batch_facets: facet k's rows for the whole batch in one copy, counts[q * (nbuckets_k + 1) + v].  For every document d of query q's docID set — exactly what
 * tri_batch_docset delivers: the index's masked set and q's filter are applied, there is no second rule — counter min(values[d], nbuckets_k) goes up by one; the
 * last counter is the overflow bucket, so a row always sums to tri_batch_match_counts[q].  A query the planner left out, or one without matches, has an
 * all-zero row.  TRI_ERR_INVALID, nothing written: no facets set, k out of range, cap (in counters) below nq * (nbuckets_k + 1), no tri_batch_sync since
 * the last run, facets set or replaced since the last run.
 * tri_cbatch_facets: after tri_cbatch_sync, the parts' rows widened and summed (a docID that several sources deliver counts once per source, as tri_cbatch_docset
 * lists it).  TRI_ERR_INVALID, naming the part, when the parts disagree in the number of facets or in nbuckets_k.
 * tri_dev_get_option "facet_last_us" (read-only): the device time of the last faceted run's zeroing and counting kernel, read at tri_batch_sync. */
typedef struct tri_column tri_column;
int tri_column_create(tri_index *, const uint32_t *values, size_t n /* docs_cnt + 1 */, tri_column **out);
void tri_column_destroy(tri_column *);
#define TRI_FACETS_MAX 4
#define TRI_FACET_MAX_BUCKETS 65536u
typedef struct tri_facet {
        tri_column *column;
        uint32_t nbuckets; /* 1 .. TRI_FACET_MAX_BUCKETS; the row has nbuckets + 1 counters */
        uint32_t reserved; /* 0 */
} tri_facet;
int tri_batch_set_facets(tri_batch *, const tri_facet *facets, size_t n /* 0: clear */);
int tri_batch_facets(tri_batch *, size_t k, uint32_t *counts /* [nq][nbuckets_k + 1], caller query order */, size_t cap);
/* (tri_cbatch_facets is declared with the collection's calls below) */

/* ---- order by a column -----------------------------------------------------------------------------
 * The last thing an application does in MatchedIndexDocumentsFilter::consider(id) / consider(ids, cnt) (exec.h:12-23: "just count or collect documents
 * matching a query") besides counting and ranking: LIST the first K matches by a per-document attribute — newest first, cheapest first, highest rated first.
 * A batch that names a column and a K (an order) selects, at the end of every run and on the device, each query's first K documents: K x 8 bytes a query
 * cross PCIe instead of the docID set.
 *
 * tri_batch_set_order (exec.h:12-23): after tri_batch_create, before a run, again between runs; NULL removes; it holds for every later run until replaced or
 * removed; the column is stored by reference (the filters' lifetime rules: tri_column_create above).  Runs already queued keep the spec and the blocks they were
 * launched with (the call waits for them before it swaps).  The partial lists and the rows live in one block taken from the handle's buffer pool: (tasks + the
 * merge's intermediate lists + nq) x (topk x 8 + 4) bytes (+ 64 KB, the pool's smallest buffer) — TRI_ERR_NOMEM when it cannot be had.  TRI_ERR_INVALID, nothing
 * changed: a null batch, a null column, a column of another index, topk outside 1 .. TRI_ORDER_MAX_TOPK, reserved != 0, a batch created with
 * TRI_FLAG_ACCUMULATED_SCORE (its one-pass queries keep no docID sets).  An order, facets and a ranker may stand on one batch together.  Every later tri_batch_run
 * selects again, on the engine stream behind the kernels that complete the docID sets (one launch for the tasks and one per round of the merge: one round up to
 * 32 tasks a query, two up to 1024; a batch without an order, or without tasks, launches nothing more); the rows stand after tri_batch_sync.
 * tri_batch_ordered (exec.h:12-23): for every query q, in caller query order, the first counts[q] = min(|S|, topk) documents of its docID set S — exactly what
 * tri_batch_docset delivers: the index's masked set and q's filter are applied, the default mode's sets are included — sorted by (values[d] ascending, docID
 * ascending), or with descending != 0 by (values[d] descending, docID ASCENDING): ties go to the lower docID in both directions; values compare as unsigned
 * 32-bit.  values[q][i] is the column's value of docids[q][i]; entries past counts[q] are zero in both arrays; a query the planner left out has count 0.
 * Everything is integer: the same bits from run to run and under every option set.  TRI_ERR_INVALID, nothing written: no order set, no tri_batch_sync since
 * the last run, an order set or replaced since the last run, a null output.
 * tri_cbatch_ordered (exec.h:12-23): after tri_cbatch_sync, the parts' lists merged per query on the device by (value, docID, source ascending), the value
 * reversed when descending; a docID that several sources deliver is listed once per source, older source first, as tri_cbatch_ranked treats equal scores;
 * counts[q] = min(sum of the parts' counts, topk).  TRI_ERR_INVALID, naming the part, nothing written: a part has no order, the parts differ in topk or in
 * descending (each part's column is its own).  A collection none of whose parts has an order runs as it always did.
 * tri_dev_get_option "order_last_us" (read-only): the device time of the last ordered run's selection and merge kernels, read at tri_batch_sync. */
#define TRI_ORDER_MAX_TOPK 256 /* == TOPK_MAX */
typedef struct tri_order {
        tri_column *column;
        uint32_t topk;       /* 1 .. TRI_ORDER_MAX_TOPK */
        uint32_t descending; /* != 0: highest value first (ties still go to the lower docID) */
        uint32_t reserved;   /* 0 */
} tri_order;
int tri_batch_set_order(tri_batch *, const tri_order *spec /* NULL: remove */);
int tri_batch_ordered(tri_batch *, uint32_t *docids /* [nq][topk] */, uint32_t *values /* [nq][topk] */, uint32_t *counts /* [nq] */);
/* (tri_cbatch_ordered is declared with the collection's calls below) */

/* ---- stats of a column per query and bucket ---------------------------------------------------------
 * What an application adds up in MatchedIndexDocumentsFilter::consider(id) / consider(ids, cnt) (exec.h:12-23: "just count or collect documents matching a
 * query") beside the facet counts: the price range of the matches, the average rating per category, revenue per brand, the newest timestamp per tenant.  A
 * stat names a VALUE column and, optionally, a GROUP column of nbuckets (tri_column_create above: both belong to the batch's index); a batch that names stats
 * aggregates, at the end of every run and on the device, each query's docID set into a row of records per stat: 20 bytes a (query, bucket) cross PCIe instead
 * of the docID set.
 *
 * The contract (exec.h:12-23 is the consumer it stands for): for every document d of query q's docID set — exactly what tri_batch_docset delivers: the index's
 * masked set and q's filter are applied, there is no second rule — the record of bucket g = min(group[d], nbuckets) takes the document: count += 1,
 * sum += value[d] (an exact u64: one source cannot overflow it), min = min(min, value[d]), max = max(max, value[d]); values compare UNSIGNED.  A grouped row has
 * nbuckets + 1 records, the last is the overflow bucket, as in tri_batch_facets — its counts equal tri_batch_facets of the same column and nbuckets, integer for
 * integer.  Without a group column (group NULL, nbuckets 0) the row is the single record 0.  An empty bucket reads count 0, sum 0, min 0xffffffff, max 0.  A docID
 * at or past a column's end is never read (group: overflow, value: 0xffffffff); tri_column_create makes it unreachable.
 * tri_batch_set_stats (exec.h:12-23): after tri_batch_create, before a run, again between runs; n == 0 clears; columns are stored by reference and kept alive
 * while the batch may run.  Runs already queued keep the specs they were launched with (the call waits for them before the rows they aggregate into are
 * released).  The rows of ALL stats live in one block taken from the handle's buffer pool: nq x sum over the stats of (nbuckets + 1) x 20 bytes (+ 64 KB, the
 * pool's smallest buffer), per stat four planes — sums, counts, mins, maxs — in caller query order: TRI_ERR_NOMEM when it cannot be had.  TRI_ERR_INVALID,
 * nothing changed: a null value column, a column of another index, n > TRI_STATS_MAX, a group with nbuckets of 0 or above TRI_FACET_MAX_BUCKETS, no group with
 * nbuckets != 0, reserved != 0, a batch created with TRI_FLAG_ACCUMULATED_SCORE (its one-pass queries keep no docID sets).  Stats, facets, an order and a ranker
 * stand on one batch independently; the parts of a tri_cbatch each carry their own stats.
 * Every later tri_batch_run initialises the block and aggregates again, on the engine stream behind the kernels that complete the docID sets (one more launch
 * per run; a batch without stats launches nothing more); the rows stand after tri_batch_sync.
 * tri_batch_stats (exec.h:12-23): stat k's rows for the whole batch, each output [nq][nbuckets_k + 1] in caller query order, one copy per output; a NULL output
 * is skipped, all four NULL is invalid.  A query the planner left out, or one without matches, reads as empty records.  TRI_ERR_INVALID, nothing written: no
 * stats set, k out of range, cap (in records) below nq * (nbuckets_k + 1), no tri_batch_sync since the last run, stats set or replaced since the last run.
 * tri_cbatch_stats (exec.h:12-23): after tri_cbatch_sync, the parts' rows combined on the host — counts and sums added, mins and maxs folded (a docID that
 * several sources deliver counts once per source, as tri_cbatch_docset lists it).  TRI_ERR_INVALID, naming the part, when the parts disagree in the number of
 * stats, in stat k's nbuckets or in whether it is grouped; TRI_ERR_INVALID, naming the query and the bucket, nothing written, when a summed sum would wrap u64.
 * tri_dev_get_option "stats_last_us" (read-only; exec.h:12-23): the device time of the last run's initialisation of the rows and aggregating kernel, read at
 * tri_batch_sync. */
#define TRI_STATS_MAX 4
typedef struct tri_stat {
        tri_column *group; /* NULL: one bucket */
        tri_column *value;
        uint32_t nbuckets; /* grouped: 1 .. TRI_FACET_MAX_BUCKETS, the row has nbuckets + 1 records; ungrouped: 0 */
        uint32_t reserved; /* 0 */
} tri_stat;
int tri_batch_set_stats(tri_batch *, const tri_stat *stats, size_t n /* 0: clear */);
int tri_batch_stats(tri_batch *, size_t k, uint64_t *sums, uint32_t *counts, uint32_t *mins, uint32_t *maxs /* each [nq][nbuckets_k + 1], caller query order; NULL: skipped */,
                    size_t cap /* records */);
/* (tri_cbatch_stats is declared with the collection's calls below) */

/* ---- column predicates as document filters ----------------------------------------------------------
 * exec_query's IndexDocumentsFilter (matches.h:190-201; tested before consider(): exec.cpp:1133-1150) where the application's rule reads the documents' attributes —
 * "price between 10 and 50, in stock, category in {3, 17, 40}" — and those attributes are columns already resident in HBM (tri_column_create): the predicates
 * become drop bitmaps on the device, in one launch that reads every distinct column once; no docID list crosses PCIe.
 *
 * tri_filters_from_columns (matches.h:190-201 / exec.cpp:1133-1150): for each document d in 1 .. max_doc predicate p HOLDS when every one (any == 0) or at least
 * one (any != 0) of its clauses holds; a clause holds where its test is true (negate == 0) or false (negate != 0).  RANGE: lo <= values[d] <= hi, unsigned, both ends
 * inclusive, lo > hi true for no document.  SET: values[d] is one of set[0 .. nset); a value at or above TRI_FACET_MAX_BUCKETS is in no set.
 * mode TRI_FILTER_KEEP: the documents where p holds are the only ones a query may match; TRI_FILTER_DROP: they are dropped.  In both, whatever the `also`
 * filter drops is dropped as well.  out[i] is an ordinary tri_filter — the lifetime rules of tri_filter_create, used in tri_batch_set_filters and in the parts
 * of a tri_cbatch like one — that does not reference the columns, the `also` filters or the caller's arrays once the call has returned; the call returns when
 * all np bitmaps stand, and produces all np filters or none.
 * TRI_ERR_INVALID, nothing allocated, out untouched, the message naming the predicate and the clause: a null argument (preds, out, a predicate's clauses, a
 * clause's column, a SET's set with nset != 0), np of 0 or above TRI_PREDS_MAX, a column or an `also` filter of another index, more than TRI_PRED_MAX_COLUMNS
 * distinct columns across the call, nclauses out of range, an unknown kind, a SET value at or above TRI_FACET_MAX_BUCKETS, a non-zero reserved field, a bad mode.
 * TRI_ERR_NOMEM, out untouched, when the handle's pool cannot supply the np bitmaps.
 * tri_filter_bitmap (matches.h:190-201 / exec.cpp:1133-1150: what filter(id) answers, for every id at once): the drop bitmap of ANY filter, however it was made —
 * bit d & 31 of words[d >> 5] is document d, set: dropped.  *nwords receives the extent ((max_doc / 131072 + 2) * 4096 words), also when the call is refused
 * for cap below it (TRI_ERR_INVALID, nothing written to words).  Bit 0 and the bits past max_doc are unspecified: no kernel tests them.  One device-to-host copy
 * behind the engine stream. */
#define TRI_PRED_MAX_CLAUSES 8   /* per predicate */
#define TRI_PRED_MAX_COLUMNS 8   /* distinct columns per call */
#define TRI_PREDS_MAX        256 /* predicates per call */
#define TRI_CLAUSE_RANGE 0       /* lo <= values[d] <= hi, unsigned, both ends inclusive; lo > hi: holds for no document */
#define TRI_CLAUSE_SET   1       /* values[d] is one of set[0 .. nset); every set value < TRI_FACET_MAX_BUCKETS */
typedef struct tri_clause {
        tri_column *column;
        uint32_t kind, negate;   /* negate != 0: the clause holds where the test fails */
        uint32_t lo, hi;         /* RANGE */
        const uint32_t *set;     /* SET: any order, duplicates allowed, nset == 0 legal (holds for no document) */
        uint32_t nset, reserved; /* reserved 0 */
} tri_clause;
typedef struct tri_predicate {
        const tri_clause *clauses;
        uint32_t nclauses;       /* 1 .. TRI_PRED_MAX_CLAUSES */
        uint32_t any;            /* 0: every clause holds (AND); != 0: at least one (OR) */
        const tri_filter *also;  /* optional, same index: what it drops the result drops too */
        uint64_t reserved;       /* 0 */
} tri_predicate;
int tri_filters_from_columns(tri_index *, const tri_predicate *preds, size_t np, int mode, tri_filter **out /* [np] */);
int tri_filter_bitmap(const tri_filter *, uint32_t *words, size_t cap /* words */, size_t *nwords);

/* ---- postings decode (codec seam) -----------------------------------------------------------------
 * Replaces Codecs::PostingsListIterator::next() driven to exhaustion (google_codec.cpp:777-819,
 * unpack_block :596-639): decodes whole postings lists on the GPU.  out_offsets[n+1] receives the prefix
 * offsets into docs/freqs (host buffers with room for sum(documents)). */
int tri_decode_terms(tri_index *, const uint32_t *terms, size_t n, uint32_t *docs, uint32_t *freqs, uint64_t *out_offsets);

/* The hits of postings lists: Codecs::PostingsListIterator::materialize_hits(DocWordsSpace *, term_hit *) (codecs.h:211-246; google_codec.cpp:533-594;
 * lucene_codec.cpp:767-856) without a query around it — what an iterator the application keeps on the CPU (a proximity scorer, a DocsSetIterators subclass
 * of its own) asks of the codec for its candidates (candidate_document::materialize_term_hits, queryexec_ctx.cpp:317-351).
 *
 * Per hit k: positions[k] = term_hit::pos, the u16 running sum of the document's position deltas (it restarts at 0 with every document);
 * payload_lens[k] = term_hit::payloadLen; payloads[k] = term_hit::payload, the word as materialize_hits leaves it: the word and the current length restart at
 * 0 with each document, a new payload overwrites only the word's first min(len, 8) bytes, length 0 clears it (what tri_batch_matched_payloads delivers for the
 * matches of a query).  That is the GOOGLE codec's rule (google_codec.cpp:547-583).  A LUCENE index follows lucene_codec.cpp:767-856 instead: the word is cleared
 * and the hit's own payloadLen bytes are copied for EVERY hit, so a hit's length and word depend on that hit alone and nothing is carried from hit to hit — the
 * two codecs answer the same for the same postings exactly when, within every document, no non-zero length is shorter than an earlier non-zero length since
 * the last zero-length hit.  The upload validates a LUCENE segment's payloads (every length <= 8, a block's byte count against its lengths, the tail's end against
 * the term's chunk: TRI_ERR_FORMAT otherwise).  payload_lens and payloads are both NULL (positions only) or both given.
 *
 * tri_decode_hits — whole lists, for EVERY document of each term, in list order.  out_offsets[n + 1] are prefix offsets in hits; term i's hits lie document
 * after document, document j of the term owning freq[j] hits, freq being exactly what tri_decode_terms returns for it: the caller's cumulative sum of those
 * frequencies addresses a document.  A frequency-0 document owns no hits.  A document's hit count is its STORED frequency (u32), not the tokenpos_t wrap of
 * it: the reference's own walk decodes (u16)freq hits of a document of more than 65 535 and so loses its place in the block behind it; the
 * engine decodes all of that document's hits and stays in place for the next document.  positions == NULL: offsets only (the sizing call).
 *
 * tri_decode_hits_at — selected documents: the hits of term terms[i] in document docids[i].  Pairs come in any order and may repeat.  freqs[i] = the
 * document's stored frequency, or 0xffffffff when the term's list does not hold docids[i] (docID 0, UINT32_MAX and anything past the list's last document
 * included); an absent document owns no hits.  n == 0 is legal.  positions == NULL: freqs and offsets only.
 *
 * TRI_ERR_INVALID, nothing written: a term index >= the index's terms, a LUCENE index uploaded without hits.data, cap (in hits) smaller than the total, one
 * of payload_lens / payloads without the other. */
int tri_decode_hits(tri_index *, const uint32_t *terms, size_t n, uint16_t *positions, uint8_t *payload_lens, uint64_t *payloads, size_t cap /* hits */,
                    uint64_t *out_offsets /* [n + 1] */);
int tri_decode_hits_at(tri_index *, const uint32_t *terms, const uint32_t *docids, size_t n, uint32_t *freqs /* [n] */, uint16_t *positions, uint8_t *payload_lens,
                       uint64_t *payloads, size_t cap /* hits */, uint64_t *out_offsets /* [n + 1] */);

/* ---- token-set co-occurrence (Trinity::intersect) ----------------------------------------------------
 * Trinity::intersect_impl (intersect.h:25-37, intersect.cpp:5-170) — the engine behind intersection_alternatives' "drop a word" suggestions — for a BATCH of
 * requests over one index, synchronous like tri_decode_hits.  A request is a list of 1 .. 64 token GROUPS, each a set of synonymous terms (the reference's
 * std::vector<std::unordered_set<str8_t>>); bit i of a document's mask is set when the document holds a term of group i.  Request r's groups follow request
 * r - 1's: with G = the sum of all ngroups, group g's term ids are terms[group_first[g] .. group_first[g + 1]) (group_first[G + 1], ascending, an empty group is
 * legal).  A term id of 0xffffffff, or a term without documents, is an UNKNOWN token (intersect.cpp:27-43: term_ctx().documents == 0).  origMask = the groups
 * with a known term, forced to 0 when any term of the request is unknown (:33, :50-51).  A document is CONSIDERED when its mask is not origMask (:138), the
 * stop-word test passes, and the index's masked set as it stands at the call (tri_index_set_masked) does not hold it (:140); the considered masks, in docID
 * order, go through ctx::consider (:64-91) and finalize (:93-99).  A request without any known term is legal and yields empty lists (:47-48).
 *
 * Two things are consciously NOT copied.  (1) Stop words: the reference tests `first` / `last`, slot indices of its remaining[] array, not token indices
 * (:112-131, :139) — they equal the mask's lowest / highest set bit only while every group has one term and no list has ended.  The engine implements what
 * intersect.h:15-18 documents: a document is ignored when the LOWEST or the HIGHEST set bit of its mask is in stopwords_mask.  Parity with the reference's
 * code is claimed for stopwords_mask == 0 only — the value intersection_alternatives passes (:276).  (2) ctx::indexPrev is a uint8_t and wraps once the
 * antichain holds more than 255 entries; the engine's replay uses a full-width index.
 *
 * tri_isect_run (intersect.cpp:5-170): builds one docID bitmap row per distinct known term of the call in a scratch block of the call (the index's plane cache
 * is not touched), runs the two passes of csrc/k_isect.hpp and the replay of csrc/host/isect_rows.hpp, and returns a handle that holds every request's answer.
 * TRI_ERR_UNSUPPORTED for the whole call, *out untouched: the call's scratch would exceed option isect_max_bytes; an index whose docIDs reach 2^31.
 * tri_isect_status (no counterpart: the reference's vector grows without bound, intersect.cpp:89): status[r] = TRI_OK, or TRI_ERR_UNSUPPORTED when one of the request's tables overflowed (options isect_max_masks / isect_max_runs): the caller
 * keeps its CPU path for that request, as with tri_batch_query_status; the other requests of the call are unaffected.
 * tri_isect_results (intersect.cpp:160-169): request r's list as intersect_impl appends it — (mask, count) pairs in finalize's order, popcount descending, then
 * count descending; the reference's std::sort leaves ties unspecified, here they are broken by ascending mask.  masks == NULL: *n only.
 * tri_isect_histogram: table H, the exact order-free product — every distinct mask the merge loop builds (intersect.cpp:111-131) on a document that passes
 * :138-142, with its documents and its first docID, ascending mask.
 * masks == NULL: *n only.  Both fail with TRI_ERR_UNSUPPORTED on a request whose status is that.
 * tri_isect_get_info (the reference's only account of a run is its trace line, intersect.cpp:162-163): the kernels' constants and what the call used (the
 * per-request arrays belong to the handle).  tri_isect_destroy: the handle and every list in it (intersect.cpp:165-169 appends to the caller's vector instead).
 * TRI_ERR_INVALID, nothing written: a null argument, more than 65535 requests, ngroups of 0 or above 64, a non-zero `reserved`, a group_first that does not
 * ascend, a term id >= the index's terms that is not 0xffffffff, r >= the call's requests, a cap smaller than the list.
 * Options (tri_dev_set_option, read by tri_isect_run).  "isect_max_bytes": the scratch budget of a CALL — its rows (4 bytes per 32 docIDs and distinct known term:
 * 1.3 MB a term at 10 M documents), its requests' tables and 8 bytes per request and span of 4096 documents; default 2 GiB, a ceiling: the scratch is taken from the
 * handle's buffer pool for the call and goes back to it.  A call that would exceed it is TRI_ERR_UNSUPPORTED as a whole (split it).  "isect_max_masks": the most slots
 * of a request's table H (default 262144; 16 bytes each + 4 for the thresholds).  H is sized by the call's WIDEST request — g groups make fewer than 2^g masks: 2 x 2^g
 * slots, at least 64 — up to the option, the same for every request of the call.  "isect_max_runs": the most slots of a request's table C (default 524288; 12 bytes each).
 * C is keyed by (mask, epoch), so the group count does not bound it; it is sized AFTER pass 1 from H, which gives an exact upper bound — every mask that has a strict
 * superset adds one key per epoch from its threshold's on — twice the largest request's bound, at least 64, up to the option: a request whose runs fit the option is
 * never refused for them.  tri_isect_info.max_masks / max_runs: the slots the call used (max_runs 0: pass 2 was not needed). */
typedef struct tri_isect tri_isect;
typedef struct tri_isect_request {
        uint32_t ngroups;        /* 1 .. 64 */
        uint32_t reserved;       /* 0 */
        uint64_t stopwords_mask; /* bit i: group i is a stop word (intersect.h:15-18) */
} tri_isect_request;
typedef struct tri_isect_info {
        uint32_t span_docs;       /* documents a wave takes (k_isect.hpp ISECT_SPAN) */
        uint32_t lds_slots;       /* keys of a wave's LDS table (ISECT_LDS_SLOTS) */
        uint32_t nreq, nspans;
        uint32_t rows;            /* plane-0 rows built: the distinct known terms of the call */
        uint32_t max_masks, max_runs; /* the table sizes the call ran with */
        uint32_t passes;          /* kernels passes run: 0 (no known term), 1 (no mask has a strict superset: nothing to credit) or 2 */
        uint64_t row_bytes;       /* bytes of one row */
        uint64_t scratch_bytes;   /* rows + tables + per-span words: what counted against isect_max_bytes */
        const uint32_t *h_size;   /* [nreq] entries of H */
        const uint32_t *c_size;   /* [nreq] entries of C */
        const uint32_t *lds_spills; /* [nreq] (mask, step) groups that found their wave's LDS table full and went to the global one */
} tri_isect_info;
int tri_isect_run(tri_index *, const tri_isect_request *reqs, size_t nreq, const uint32_t *terms, const uint32_t *group_first, tri_isect **out);
int tri_isect_status(const tri_isect *, int32_t *status /* [nreq] */);
int tri_isect_results(const tri_isect *, size_t r, uint64_t *masks, uint32_t *counts, size_t cap, size_t *n);
int tri_isect_histogram(const tri_isect *, size_t r, uint64_t *masks, uint32_t *counts, uint32_t *first_docs, size_t cap, size_t *n);
int tri_isect_get_info(const tri_isect *, tri_isect_info *);
void tri_isect_destroy(tri_isect *);

/* ---- the percolator: documents matched against stored queries (percolator.h:1-60, percolator.cpp:5-137: percolator_query::match walks one exec_node tree per
 * (query, document) on one thread; its header names Twitter's predicate index as what it lacks, percolator.h:1-3).  Here a SET of stored queries is resident on the
 * device and a batch of documents that was never indexed is tested against all of them: no tri_index, no postings decoded; the answer is (query, document) pairs.
 * A stored query is a postfix program in the vocabulary above; TERM operands index the percolator's OWN dictionary, 0 .. nterms-1 (the application interns its
 * strings, as percolator_query::CCTX::resolve_query_term does, percolator.h:30-45).  For ONE document (percolator.cpp:9-137): TERM: the document holds the term
 * (match_term); AND / OR: all / any child (matchallterms, matchanyterms, logicaland, logicalor, matchallnodes, matchanynodes); NOT(2): lhs and not rhs (logicalnot,
 * :86-90); OPT(2): the main side (logicaland(x, consttrueexpr), :80-84, :129); SOME: at least `min` of the children (:98-107); PHRASE(n): match_phrase, which the
 * reference leaves to the document proxy and the device FIXES as the Phrase iterator's rule — some position p != 0 of the first word has p + j among the positions
 * of word j for every j (position 0 never starts a phrase; a phrase may repeat a word; at most 16 words).  Percolator programs only: NOT(1), unarynot (:45-46), is
 * true where its operand is false (tri_batch_create keeps refusing it).  The empty program is constfalse (:76-78): it never matches.
 * tri_perc_create (percolator_query::percolator_query, percolator.h:47-58): lowers and uploads the set once.  A malformed program (what tri_batch_create refuses, a
 * TERM >= nterms) fails the call with TRI_ERR_INVALID; a tree of more than 1024 nodes (a node per token, less a phrase's words) or one whose fold needs more than 64
 * stack words is left out ALONE — tri_perc_query_status: TRI_ERR_UNSUPPORTED for it, as tri_batch_query_status; it matches nothing and the rest of the set runs.
 * tri_perc_set_enabled: unregisters / registers queries again without a rebuild (every query starts enabled); an index >= nq is TRI_ERR_INVALID, nothing changed.
 * tri_perc_get_info: the set's size.  tri_perc_destroy: after every result of the set, before its tri_dev.
 * tri_perc_match (percolator_query::match, percolator.cpp:5-7, for every stored query and every document of the batch): synchronous, like tri_isect_run.  Documents
 * are numbered 0 .. ndocs-1 in the order given.  TRI_ERR_INVALID, nothing written, the message names the document and the term: a null argument, ndocs of 0 or above
 * 65536, doc_first that does not ascend, a document's terms not strictly ascending (0xffffffff, a term unknown to the dictionary, is ignored and stands last), a term
 * id >= nterms, frequencies that run past npositions, positions that descend within a posting, a non-zero `reserved`.  TRI_ERR_UNSUPPORTED for the whole call: its
 * pooled scratch would exceed option perc_max_bytes, or it answers 2^32 pairs or more (split the call).  TRI_ERR_NOMEM as elsewhere.
 * tri_perc_result_pairs: every matching pair, in the order asked for — TRI_PERC_BY_QUERY: query ascending, then document; TRI_PERC_BY_DOCUMENT: document ascending,
 * then query ("which rules fired for this document").  Both orders are made on the device and are deterministic.  queries == NULL: *n only; cap < the pairs, or an
 * order outside the two: TRI_ERR_INVALID, nothing written.  tri_perc_result_doc_counts: the queries that matched each document.
 * Options (tri_dev_set_option, read by tri_perc_match).  "perc_max_bytes": the pooled scratch of a call (default 4 GB).  "perc_prune": default 1 — a stored query is
 * evaluated only if the batch holds one of its leaves (a term it names, a phrase all of whose words occur in the batch), or if it matches a document holding none of
 * its terms (a pure negation, NOT(1)); 0: every enabled query is evaluated (for measurement: the pairs are the same).
 * Threading and teardown follow the rules at the top: one thread at a time per tri_dev; results before their set, sets before their tri_dev. */
typedef struct tri_perc tri_perc;               /* a resident set of stored queries, on one tri_dev */
typedef struct tri_perc_result tri_perc_result; /* the answer of one tri_perc_match */
typedef struct tri_perc_docs {                  /* a batch of documents */
        uint32_t ndocs;                         /* 1 .. 65536 a call (a leaf row is at most 8 KB; split longer streams) */
        const uint64_t *doc_first;              /* [ndocs + 1] into terms / freqs */
        const uint32_t *terms;                  /* per document strictly ascending */
        const uint32_t *freqs;                  /* positions of that (document, term); may be 0: held, but in no phrase */
        const uint16_t *positions;              /* concatenated, non-descending within a (document, term) */
        uint64_t npositions;
        uint32_t reserved;                      /* 0 */
} tri_perc_docs;
typedef struct tri_perc_info {
        uint64_t queries, unsupported; /* stored; of them left out (tri_perc_query_status) */
        uint64_t terms, phrases;       /* distinct terms the queries name, distinct multi-word phrases: the set's leaf table */
        uint64_t device_bytes;         /* resident */
        uint32_t nterms, reserved;     /* the dictionary's size as given */
} tri_perc_info;
typedef struct tri_perc_result_info {
        uint32_t ndocs, leaf_rows, phrase_rows; /* rows built: term leaves present in the batch, phrases all of whose words are */
        uint32_t evaluated, hit_queries;        /* queries evaluated after the prune; of them those with a match */
        uint32_t reserved;
        uint64_t pairs, scratch_bytes;
        float rows_ms, phrases_ms, select_ms, eval_ms, compact_ms, total_ms; /* device time per stage (HIP events); the call end to end on the host */
} tri_perc_result_info;
#define TRI_PERC_BY_QUERY 0
#define TRI_PERC_BY_DOCUMENT 1
int tri_perc_create(tri_dev *, const uint32_t *prog, size_t prog_len, const tri_query *queries, size_t nq, uint32_t nterms, tri_perc **out);
int tri_perc_query_status(const tri_perc *, int32_t *status /* [nq] */);
int tri_perc_set_enabled(tri_perc *, const uint32_t *queries, size_t n, int enabled);
int tri_perc_get_info(const tri_perc *, tri_perc_info *);
void tri_perc_destroy(tri_perc *);
int tri_perc_match(tri_perc *, const tri_perc_docs *, tri_perc_result **out);
int tri_perc_result_pairs(const tri_perc_result *, int order, uint32_t *queries, uint32_t *docs, size_t cap, size_t *n);
int tri_perc_result_doc_counts(const tri_perc_result *, uint32_t *counts /* [ndocs] */);
int tri_perc_result_get_info(const tri_perc_result *, tri_perc_result_info *);
void tri_perc_result_destroy(tri_perc_result *);

/* ---- batched query execution (span seam) -----------------------------------------------------------
 * Replaces, for a whole batch of queries at once: queryexec_ctx::build_iterator + build_span
 * (exec.cpp:253-505), DocsSetSpan::process(mp, 1, DocIDsEND) (docset_spans.cpp:98-173, 269-290, 681-790)
 * over Conjuction/Disjunction/Phrase iterators (docset_iterators.cpp:66-405), the IteratorScorer wrappers
 * (docset_iterators_scorers.cpp) with Similarity BM25 (similarity.h:165-255), and the application's
 * top-K MatchedIndexDocumentsFilter::consider(id, score) heap (matches.h:155-171).
 *
 * prog/queries: postfix programs.  flags — exactly one of: TRI_FLAG_DOCUMENTS_ONLY (results = ascending docID sets),
 * TRI_FLAG_ACCUMULATED_SCORE (topk >= 1: results = top-K by score desc, docID asc + total match counts;
 * topk == 0: every match's score is kept, see tri_batch_scores), TRI_FLAG_MATCHED_TERMS (exec_query's default mode:
 * ascending docID sets + per match the matched query terms with their hits, see tri_batch_matched_terms).
 * similarity: TRI_SIM_BM25 / TRI_SIM_TFIDF / TRI_SIM_TRIVIAL — which IndexSourceTermsScorer::score() the device evaluates.
 * weights: optional, one double per program token (TERM tokens: the term's ScorerWeight, PHRASE tokens:
 * the phrase's); NULL => BM25 idf computed from the index's own statistics exactly as
 * IndexSourcesCollectionBM25Scorer does for a single source (similarity.h:179-181, 202-226). */
int tri_batch_create(tri_index *, const uint32_t *prog, size_t prog_len, const tri_query *queries, size_t nq,
                     const double *weights, uint32_t flags, uint32_t topk, int similarity, tri_batch **out);
/* A query whose shape the planner does not lower (today: a tree of more nodes than option tree_max_nodes allows — 64 by default, up to 1024 —
 * or one whose evaluation needs more than 64 stack words, more reportable terms in the default mode than option rich_max_terms allows — 16 by
 * default, up to 64 —, a tree that matches documents
 * holding none of its terms) does NOT fail tri_batch_create: the query is left out of the batch — it reports no matches — and its status says so, so that one such
 * query among thousands costs the caller one CPU span (exec.cpp:509-1517 for that query alone), not the batch.  status[q]: TRI_OK or
 * TRI_ERR_UNSUPPORTED; tri_batch_info.unsupported_queries counts them; tri_last_error() after tri_batch_create describes the last one.
 * (A malformed program is the caller's bug and still fails the call with TRI_ERR_INVALID.) */
int tri_batch_query_status(const tri_batch *, int32_t *status /* [nq] */);
void tri_batch_destroy(tri_batch *);
/* enqueue the batch on the engine stream (asynchronous) */
int tri_batch_run(tri_batch *);
/* wait for THIS batch's completion (its own last event: batches launched behind it on the engine stream are not waited for, so a caller
 * may keep the next batch queued while it collects this one's results); also refreshes tri_batch_info */
int tri_batch_sync(tri_batch *);
int tri_batch_get_info(const tri_batch *, tri_batch_info *);

/* results (call after tri_batch_sync) */
int tri_batch_match_counts(tri_batch *, uint64_t *counts /* [nq] */);
/* Copy query q's ascending docID set; what MatchedIndexDocumentsFilter::consider(ids, cnt) (matches.h:161-165) receives.
 * DocumentsOnly, MatchedTerms and AccumulatedScore batches with topk == 0 materialise every query's set.  An AccumulatedScore batch
 * with topk >= 1 delivers top-K lists and match counts; queries it ran through the one-pass kernel have no materialised set and
 * the call fails with TRI_ERR_INVALID for them (tri_batch_docset_hashes likewise when the batch holds such a query). */
int tri_batch_docset(tri_batch *, size_t q, uint32_t *out, size_t cap, size_t *n);
/* The docID set of query q in the form the engine holds it.  *form = 0: ascending docIDs (tri_batch_docset copies them), nothing else is set.
 * *form = 1: a BITMAP — a DocumentsOnly union / conjunction of head terms expected to match one document in 32 or more keeps one bit per
 * document instead of four bytes per match (option result_bitmaps, default 1; tri_batch_info.bitmap_queries): bit j of words[i] set <=> document
 * *first_doc + 32 i + j matches; *nwords words (words == NULL: sizes only).  tri_batch_docset expands such a set on read-back; a caller that
 * replays consider(ids, cnt) (matches.h:161-165) or intersects further can take the words as they are. */
int tri_batch_docset_bitmap(tri_batch *, size_t q, int *form, uint32_t *words, size_t cap, uint32_t *first_doc, size_t *nwords);
/* EVERY query's docID set in one call — the batch form of the delivery above: out[offsets[q] .. offsets[q + 1]) = query q's ascending docIDs
 * (queries in the caller's order, offsets[nq] = the total; out == NULL: offsets only).  The sets are gathered on the device into one contiguous
 * buffer (task segments in order, bitmap-form results expanded) and cross to the host in ONE copy: with `out` in pinned memory that is PCIe's rate,
 * where tri_batch_docset pays a copy and a synchronisation per task segment.  What a caller that replays
 * MatchedIndexDocumentsFilter::consider(const docid_t *, size_t) (matches.h:161-165; exec.cpp:1213-1229 hands every match to consider()) loops
 * over.  Fails like tri_batch_docset for a query of an AccumulatedScore top-K batch whose set was never materialised. */
int tri_batch_docsets(tri_batch *, uint32_t *out, size_t cap, uint64_t *offsets /* [nq + 1] */);
/* ... each set in the form the engine holds it (the batch form of tri_batch_docset / tri_batch_docset_bitmap): forms[q] = 0: out[offsets[q] .. offsets[q + 1]) = query q's
 * ascending docIDs; 1 (a DocumentsOnly union / conjunction of head terms expected to match one document in 32 or more — option result_bitmaps): the words of a bitmap
 * over the query's docID range, bit j of word i = document 32 i + j matches (tri_batch_match_counts gives its matches).  A dense set crosses PCIe as one bit per document
 * instead of four bytes per match; the caller expands it into the ids of consider(const docid_t *, size_t) (matches.h:161-165), or keeps the bitmap.  Same calling
 * convention as tri_batch_docsets (out == NULL: offsets and forms only).  Both calls wait outside the handle's lock: another thread may compile or run meanwhile. */
int tri_batch_docsets_mixed(tri_batch *, uint32_t *out, size_t cap /* words */, uint64_t *offsets /* [nq + 1] */, uint32_t *forms /* [nq] */);
/* AccumulatedScore with topk == 0: the score of every match of query q, parallel to tri_batch_docset(q) — the
 * (id, score) stream MatchedIndexDocumentsFilter::consider(id, score) receives (matches.h:169; exec.cpp:1322-1341) */
int tri_batch_scores(tri_batch *, size_t q, double *out, size_t cap, size_t *n);
/* TRI_FLAG_MATCHED_TERMS batches.  tri_batch_query_terms: the query's reportable terms (every TERM / PHRASE-member of the
 * program outside the excluded side of a NOT, distinct, in order of first appearance; at most 16 — a query of more, option rich_max_terms, is read through the _wide calls below), i.e. the meaning of bit k
 * and column k below.  tri_batch_matched_terms, for the n matches of query q in ascending docID order (n and the docIDs as
 * returned by tri_batch_docset): present[i] bit k = term k matched document i; freq[i * nterms + k] = its frequency there
 * (term_hits::freq, 0 when absent); positions = the hits' positions, match-major then term-minor (the run of (i, k) starts at
 * the sum of all freq before it), *npos of them in all; pass positions == NULL to learn *npos. */
int tri_batch_query_terms(tri_batch *, size_t q, uint32_t *terms /* [16] */, uint32_t *nterms);
int tri_batch_matched_terms(tri_batch *, size_t q, uint32_t *present /* [n] */, uint16_t *freq /* [n * nterms] */, uint16_t *positions,
                            size_t pos_cap, size_t *npos);
/* ... the same two calls with 64-bit masks: up to 64 reportable terms (option rich_max_terms).  Same conventions — the sizing call with NULLs, dense
 * [n * nterms] frequencies, positions match-major then term-minor.  They serve EVERY query of a TRI_FLAG_MATCHED_TERMS batch (a query of at most 16 terms: its
 * mask zero-extended).  The two calls above, on a query of more than 16 reportable terms, fail with TRI_ERR_INVALID and write nothing: never past terms[16],
 * never a truncated mask. */
int tri_batch_query_terms_wide(tri_batch *, size_t q, uint32_t *terms /* [64] */, uint32_t *nterms);
int tri_batch_matched_terms_wide(tri_batch *, size_t q, uint64_t *present /* [n] */, uint16_t *freq /* [n * nterms] */, uint16_t *positions,
                                 size_t pos_cap, size_t *npos);
/* TRI_FLAG_MATCHED_TERMS | TRI_FLAG_HIT_PAYLOADS batches: the payloads of query q's hits, parallel to `positions` above (of either call; same order,
 * *n == *npos): lens[i] = term_hit::payloadLen, payloads[i] = term_hit::payload — the word as materialize_hits leaves it, i.e. only its
 * first lens[i] bytes belong to this hit (google_codec.cpp:533-594).  Pass lens == payloads == NULL to learn *n. */
int tri_batch_matched_payloads(tri_batch *, size_t q, uint8_t *lens, uint64_t *payloads, size_t cap, size_t *n);
/* TRI_FLAG_MATCHED_TERMS batches (with or without TRI_FLAG_HIT_PAYLOADS): RANK the matches on the device.  The default mode exists for application-side
 * relevance: consider(const matched_document &) receives matchedTerms[] and their hits (matches.h:109-153; queryexec_ctx.cpp:382-648) and the application
 * scores them, usually by proximity.  With a ranker set, tri_batch_sync computes that score on the device, from the masks, frequency rows and positions the
 * two k_rich passes wrote, and keeps per query the top-K (docID, score) pairs; only those leave the device.  The score is a function of exactly what
 * tri_batch_matched_terms reports.  Query q has reportable terms in slots 0 .. R-1, in tri_batch_query_terms[_wide]'s order; w[k] = the weight of the program
 * token where slot k's term first appears among the reportable tokens (every TERM token outside the excluded side of a NOT; weights: one double per program
 * token, as tri_batch_create's; NULL: 1.0 each).  For a match d, with freq[k] and pos(k) as tri_batch_matched_terms reports them:
 *
 *   score(d) = ( sum over present slots k, ascending k:  w[k] * double(min(freq[k], freq_cap)) )
 *              + adjacency * double( sum over k = 0 .. R-2 with slots k and k+1 both present:
 *                                    #{ hits h of slot k with pos(h) != 0 and pos(h) + 1 in pos(k+1) } )
 *
 * Position 0 never pairs: it is the position of a payload-only hit, and DocWordsSpace never holds it.  A term missing from the document contributes nothing,
 * nor does one the document holds but the query does not report there (the allow mask of general trees, the excluded side of a NOT).  IEEE double, in exactly
 * the order written — the sum over k first, then one multiply and one add for the pair term —, never contracted into fused multiply-adds: a sequential
 * restatement in host doubles is bit-equal.  Ranking: score descending, docID ascending (tri_batch_topk's rule).  Slots follow first appearance in the query, so
 * slots k and k+1 are consecutive query tokens: what an application detects with toNextSpan and dws->test(next, pos + 1).
 *
 * tri_batch_set_ranker: before tri_batch_run; holds for every later run until replaced or removed (spec == NULL).  TRI_ERR_INVALID, the batch left as it was:
 * another mode, topk 0 or above 256, freq_cap 0, an unknown kind, non-zero reserved, a non-finite weight or adjacency, a negative adjacency.  Negative weights
 * are legal.  tri_batch_ranked: after tri_batch_sync — docids / scores [nq][topk] row-major, counts[nq] = min(matches, topk); rows past counts[q] are zero; a
 * query the planner left out (tri_batch_query_status) has count 0.  TRI_ERR_INVALID when no ranker is set or the batch has not been synced since it was.
 * tri_batch_matched_terms*, tri_batch_docset and the rest keep working on a ranked batch; a caller that wants only the ranking does not call them, and then
 * nothing but the top-K block is copied.  (tri_dev_get_option "rich_write_last_us" / "rank_last_us", read-only: the device time of the last ranked batch's
 * WRITE pass and rank pass.)  A collection's parts merge their ranked lists on the device: tri_cbatch_ranked.  Not ranked: tri_gather_results. */
#define TRI_RANK_PROXIMITY 1u
typedef struct tri_ranker {
        uint32_t kind;     /* TRI_RANK_PROXIMITY */
        uint32_t topk;     /* 1 .. 256 (TOPK_MAX) */
        uint32_t freq_cap; /* >= 1: a term's frequency counts up to this */
        uint32_t reserved; /* 0 */
        double adjacency;  /* added per adjacent pair; finite, >= 0 */
} tri_ranker;
int tri_batch_set_ranker(tri_batch *, const tri_ranker *spec /* NULL: remove */, const double *weights /* one per program token, as tri_batch_create's; NULL: 1.0 */);
int tri_batch_ranked(tri_batch *, uint32_t *docids /* [nq][topk] */, double *scores /* [nq][topk] */, uint32_t *counts /* [nq] = min(matches, topk) */);
/* AccumulatedScore with topk >= 1: docids/scores are [nq][topk] row-major, counts[nq] = min(matches, topk) */
int tri_batch_topk(tri_batch *, uint32_t *docids, float *scores, uint32_t *counts);
/* device-resident result blocks for the multi-GPU gather (per rank: [nq][topk] u32 + f32, [nq] u32); valid once the run has
 * completed on the engine stream (tri_dev_stream) */
int tri_batch_topk_device(tri_batch *, void **docids, void **scores, void **counts);
/* device-resident per-query match counts of the last run, u64[nq] (every mode; rich mode: after the COUNT pass) */
int tri_batch_counts_device(tri_batch *, void **counts);
/* FNV-1a(64) of every query's docID set computed from the device results (tests at full size) */
int tri_batch_docset_hashes(tri_batch *, uint64_t *hashes /* [nq] */);

/* ---- collections of segments ------------------------------------------------------------------------
 * IndexSourcesCollection (index_source.cpp:3-30; exec.h:57-62: exec_query per source, every source masked by the documents the
 * newer ones update): one tri_batch per source — the SAME queries in the same order (term indices resolved against each source's
 * term table; per-token weights when the scores of the sources must share their statistics), same flags and topk, all on one device,
 * oldest source first, each index carrying its masked set (tri_index_set_masked).  The collection batch borrows them: run = the parts
 * back to back on the engine stream + a device merge — match counts add up, top-K lists merge K-way from the parts' partial lists
 * (score descending, docID ascending, as one application heap would hold them); docID sets concatenate source after source.
 *
 * The default mode (TRI_FLAG_MATCHED_TERMS parts) over a collection.  tri_cbatch_ranked: after tri_cbatch_sync, blocks laid out as tri_batch_ranked's — query q's
 * list is the best topk (docID, score) pairs over all parts, counts[q] = min(sum of the parts' ranked counts, topk), rows past counts[q] zero on every run.
 * Order: score descending, then docID ascending, then source index ascending — a STABLE sort by (-score, docID) of the parts' lists concatenated source after
 * source: where no masks are installed and two sources hold the same docID at the same score, both entries stay, the older source's first (both matches reach
 * consider() in the reference).  A merged score is bit for bit one part's score.  The collection "is ranked" for a run when at that tri_cbatch_run every part
 * carried a ranker (tri_batch_set_ranker) and all the parts' tri_ranker structs are bytewise equal; the weights are each part's own.  Otherwise run and sync
 * behave as they always did — nothing more is refused, allocated or launched — and tri_cbatch_ranked answers TRI_ERR_INVALID, names the reason ("no ranker on
 * part i", "part i's ranker differs from part 0's in <field>") and writes nothing; so it does before a sync and on a NULL argument.  (tri_dev_get_option
 * "crank_merge_last_us", read-only: the device time of the last ranked collection's merge kernel.)  A query the planner left
 * out of a part contributes nothing from that part, as with tri_cbatch_topk (tri_cbatch_query_status tells).
 * tri_cbatch_matched_terms[_wide] / tri_cbatch_matched_payloads: the rows of query q parallel to tri_cbatch_docset — each part's rows source after source, with
 * the conventions of the tri_batch_* calls (the sizing call with NULLs, dense [n * nterms] frequencies, positions match-major then term-minor) and their
 * refusals (a narrow call on a query of more than 16 terms, the wrong mode, a too-small cap).  Column k must mean the same slot in every part: when the parts
 * that report the query disagree in tri_batch_query_terms_wide's nterms (two of its terms unknown to one source and resolved to the same id), the call answers
 * TRI_ERR_INVALID, names both counts and writes nothing — the caller reads that query part by part. */
typedef struct tri_cbatch tri_cbatch;
int tri_cbatch_create(tri_batch *const *parts, size_t n, tri_cbatch **out);
void tri_cbatch_destroy(tri_cbatch *);
/* status[q]: TRI_OK, or TRI_ERR_UNSUPPORTED when the planner left query q out of any part (tri_batch_query_status): its answer over the
 * collection would be incomplete, the caller keeps its CPU path for it */
int tri_cbatch_query_status(const tri_cbatch *, int32_t *status /* [nq] */);
int tri_cbatch_run(tri_cbatch *);
int tri_cbatch_sync(tri_cbatch *);
int tri_cbatch_match_counts(tri_cbatch *, uint64_t *counts /* [nq] */);
int tri_cbatch_topk(tri_cbatch *, uint32_t *docids, float *scores, uint32_t *counts);
int tri_cbatch_docset(tri_cbatch *, size_t q, uint32_t *out, size_t cap, size_t *n);
int tri_cbatch_ranked(tri_cbatch *, uint32_t *docids /* [nq][topk] */, double *scores /* [nq][topk] */, uint32_t *counts /* [nq] */);
/* facet k's rows over the collection ("facet counts" above): the parts' rows widened and summed */
int tri_cbatch_facets(tri_cbatch *, size_t k, uint64_t *counts /* [nq][nbuckets_k + 1]: the parts' rows summed */, size_t cap);
/* the ordered rows over the collection ("order by a column" above; exec.h:12-23): the parts' lists merged on the device */
int tri_cbatch_ordered(tri_cbatch *, uint32_t *docids /* [nq][topk] */, uint32_t *values /* [nq][topk] */, uint32_t *counts /* [nq] */);
/* stat k's rows over the collection ("stats of a column" above; exec.h:12-23): the parts' rows combined on the host */
int tri_cbatch_stats(tri_cbatch *, size_t k, uint64_t *sums, uint64_t *counts, uint32_t *mins, uint32_t *maxs /* each [nq][nbuckets_k + 1]; NULL: skipped */, size_t cap /* records */);
int tri_cbatch_matched_terms(tri_cbatch *, size_t q, uint32_t *present, uint16_t *freq, uint16_t *positions, size_t pos_cap, size_t *npos);
int tri_cbatch_matched_terms_wide(tri_cbatch *, size_t q, uint64_t *present, uint16_t *freq, uint16_t *positions, size_t pos_cap, size_t *npos);
int tri_cbatch_matched_payloads(tri_cbatch *, size_t q, uint8_t *lens, uint64_t *payloads, size_t cap, size_t *n);

/* ---- multi-GPU result gather (RCCL over xGMI) -------------------------------------------------------
 * exec_query_par gives every source / shard its own result object and the caller combines them (exec.h:132-176).  One process per GPU,
 * queries sharded, index replicated: after a step every rank's fixed-shape result blocks are exchanged with one group of
 * ncclAllGather calls on the engine stream, straight from the device buffers (no host bounce).  RCCL is bound at run time (dlopen;
 * TRI_ERR_UNSUPPORTED when it cannot be loaded).  tri_comm_unique_id on rank 0, its 128 bytes handed to every rank by the launcher's
 * own means (an env var, a file, torch.distributed's store), tri_comm_create on every rank (collective).
 * tri_gather_results: counts_all u64[nranks][nq]; for AccumulatedScore top-K batches also docids_all u32[nranks][nq][k],
 * scores_all f32[nranks][nq][k], topk_counts_all u32[nranks][nq] — device buffers of the caller; enqueued behind the batch's run,
 * complete after tri_dev_sync.  (Every rank's batch has the same nq and topk.) */
typedef struct tri_comm tri_comm;
int tri_comm_unique_id(uint8_t id[128]);
int tri_comm_create(tri_dev *, const uint8_t id[128], int rank, int nranks, tri_comm **out);
/* The same gather over the caller's own transport (MPI, UCX, a test's gloo group): allgather(user, send, recv, bytes_per_rank, stream)
 * must leave, on every rank, rank r's bytes_per_rank bytes of `send` at recv + r * bytes_per_rank (both device memory), either ordered on
 * `stream` (the engine's hipStream_t) or complete when it returns; non-zero = failure.  tri_gather_results calls it once per block. */
typedef int (*tri_allgather_fn)(void *user, const void *send, void *recv, size_t bytes_per_rank, void *stream);
int tri_comm_create_custom(tri_dev *, int rank, int nranks, tri_allgather_fn allgather, void *user, tri_comm **out);
void tri_comm_destroy(tri_comm *);
int tri_gather_results(tri_batch *, tri_comm *, void *counts_all, void *docids_all, void *scores_all, void *topk_counts_all);

/* ---- write side ----------------------------------------------------------------------
 * Codecs::Google::Encoder (google_codec.cpp:9-176: begin_term / begin_document / new_hit / end_document / end_term, commit_block
 * :118-176) on the device: the postings of `nterms` terms, term after term — docs[] ascending and > 0 within a term, freqs[] the counted
 * hits of each posting, positions[npositions] those hits' positions in posting order (payload-less hits; > 0 — a position-0 hit without
 * payload is not a hit, google_codec.cpp:42-45 — and non-descending within a document, :49; sum(freqs) <= npositions), term_first[t] =
 * postings before term t ([nterms + 1]) — are encoded into the `index` bytes the reference's encoder writes for them, byte for byte
 * (skiplist cadence across terms included), and the term table (term_index_ctx: documents, chunk offset, chunk size).  Input that the
 * reference's encoder would not take (unsorted or zero positions, freqs[] reaching past positions[]) is refused with TRI_ERR_INVALID.
 * index_out == NULL: sizing call (*index_len and terms_out are filled). */
int tri_encode_google(tri_dev *, const uint32_t *docs, const uint32_t *freqs, const uint16_t *positions, size_t npositions, const uint64_t *term_first,
                      size_t nterms, uint8_t *index_out, size_t cap, size_t *index_len, tri_term *terms_out);

/* Codecs::Lucene::Encoder (lucene_codec.cpp:163-388) on the device (ABI 7): the same postings as tri_encode_google (payload-less hits) into the Lucene-shaped
 * segment — `index` (per term: the 14-byte header, 128-document blocks as two ints() groups, the prefix-varint tail, one 22-byte skiplist entry per block) and
 * `hits.data` (128-hit blocks of position deltas, varint tail) — with this repo's PFOR128 ints() payload (include/pfor128.md; the reference's FastPFor words
 * are absent from its tree): byte-identical to trinity_amd/csrc/host/lucene_encoder.hpp, the writer of every Lucene-shaped segment this engine reads.
 * index_out == NULL: sizing call (*index_len, *hits_len, terms_out). */
int tri_encode_lucene(tri_dev *, const uint32_t *docs, const uint32_t *freqs, const uint16_t *positions, size_t npositions, const uint64_t *term_first, size_t nterms,
                      uint8_t *index_out, size_t index_cap, size_t *index_len, uint8_t *hits_out, size_t hits_cap, size_t *hits_len, tri_term *terms_out);

/* SegmentIndexSession::commit (indexer.cpp:311-478) on the device (ABI 7).  The session's postings in INSERTION order — one entry per (document, term), as
 * document_proxy::insert serialised them (indexer.cpp:33-111): term_ids[i], doc_ids[i], freqs[i] = its counted hits, whose positions (and payloads) follow
 * each other in positions[] (payload_lens[] / payloads[]; NULL: none) in the same order — are sorted by (termID & 31, termID, documentID): the order the
 * reference's commit feeds its encoder in (it buckets by termID & 31 and sorts every bucket by (termID, documentID), :399-416; the Google encoder's skiplist
 * cadence runs across terms, so the order is part of the bytes), gathered, and encoded by the device encoder: index_out / *index_len = the `index` bytes,
 * term_ids_out[t] / terms_out[t] = the t-th term committed and its term_index_ctx, *nterms how many, *stats what commit adds to the field statistics
 * (:360 docsCnt, :457 sumTermHits, :470 sumTermsDocs, :476 totalTerms).  The bytes equal tri_encode_google_payloads over the same postings handed over
 * term after term in that order.  index_out == NULL: sizing call (*index_len, *nterms, *stats).  What commit or the encoder would refuse — document 0, the
 * same (term, document) twice, positions out of order — is TRI_ERR_INVALID naming the posting.  A hit at position 0 WITHOUT a payload is not a storable hit:
 * the reference's Encoder::new_hit skips it (google_codec.cpp:42-45) while commit still counts it in sumTermHits (indexer.cpp:447).  The caller drops such hits
 * before the call (freqs[i] = the hits it hands over) and adds their number to stats->sum_term_hits on its side — csrc/host/trinity_gpu_write.hpp's
 * SegmentIndexSession::insert / commit do exactly that; handed over as they are they are refused (TRI_ERR_INVALID) rather than silently re-counted. */
typedef struct tri_commit_stats {
        uint64_t docs_cnt, sum_terms_docs, sum_term_hits, total_terms;
} tri_commit_stats;
int tri_commit_google(tri_dev *, const uint32_t *term_ids, const uint32_t *doc_ids, const uint32_t *freqs, const uint16_t *positions, const uint8_t *payload_lens,
                      const uint64_t *payloads, size_t npostings, size_t npositions, uint8_t *index_out, size_t cap, size_t *index_len, uint32_t *term_ids_out,
                      tri_term *terms_out, size_t terms_cap, size_t *nterms, tri_commit_stats *stats);

/* Codecs::Google::IndexSession::merge (google_codec.cpp:186-438), for a whole dictionary at once (ABI 7): parts[0 .. nparts) are the participants' uploaded
 * google_codec indexes, MOST RECENT FIRST (merge.cpp:100-157 orders them so), each with the documents its newer segments mask installed by
 * tri_index_set_masked (its masked_documents_registry); part_terms[t * nparts + p] = output term t's index in participant p's term table (0xffffffff: the
 * participant does not hold it) — the caller walks its dictionaries as MergeCandidatesCollection::merge does (merge.cpp:100-157) and hands the output terms
 * over in the order it wants them encoded.  Per output term: the union of the participants' documents; a document several participants hold comes from the
 * most recent one; it is dropped when THAT participant's masked set holds it (google_codec.cpp:377-401) — hits and payloads copied, re-encoded by the device
 * encoder.  index_out / terms_out[t] as tri_encode_google_payloads (a term that keeps no document: documents == 0, its two chunk bytes are still in the
 * index — begin_term / end_term ran, merge.cpp:275-282 — and the caller leaves it out of the dictionary); *stats: what the merge adds to the field
 * statistics (docs_cnt is the caller's).  The bytes equal the device / host encoder's over the merged postings; the reference's raw-chunk fast path for a
 * term only one unmasked participant holds (append_index_chunk, merge.cpp:167-178) copies bytes this call re-encodes.  index_out == NULL: sizing call. */
int tri_merge_google(tri_dev *, tri_index *const *parts, size_t nparts, const uint32_t *part_terms, size_t nterms, uint8_t *index_out, size_t cap, size_t *index_len,
                     tri_term *terms_out, tri_commit_stats *stats);
/* Codecs::Lucene::IndexSession::merge (lucene_codec.cpp:963-1396), likewise for a whole dictionary (ABI 8): the same walk — participants most recent first, the most recent
 * holder's posting wins, dropped when that participant masks the document — over lucene_codec indexes uploaded WITH their hits.data; what is kept is re-encoded by the device's
 * Lucene-shaped encoder (tri_encode_lucene_payloads: PFOR128 ints() payload; a kept posting's hits go over with their payloads, length and bytes, as append_from copies
 * them): index_out / hits_out = the merged `index` and `hits.data`, terms_out[t] as tri_encode_lucene.  The bytes equal the host encoder's over the merged postings; the walk is the one
 * tests/golden/ref_merge.json pins for the Google codec (the reference's Lucene side needs FastPFor: unbuildable here, so this pair stays unpinned by reference bytes).
 * index_out == NULL: sizing call (*index_len, *hits_len). */
int tri_merge_lucene(tri_dev *, tri_index *const *parts, size_t nparts, const uint32_t *part_terms, size_t nterms, uint8_t *index_out, size_t cap, size_t *index_len,
                     uint8_t *hits_out, size_t hits_cap, size_t *hits_len, tri_term *terms_out, tri_commit_stats *stats);

/* tri_commit_google with the session's encoder being the Lucene-shaped codec's (commit is codec-agnostic: sess->new_encoder(), indexer.cpp:323): the same sort
 * and gather, then tri_encode_lucene's device encoder — `index` + `hits.data`; payload-less hits (with payloads: tri_commit_lucene_payloads below). */
int tri_commit_lucene(tri_dev *, const uint32_t *term_ids, const uint32_t *doc_ids, const uint32_t *freqs, const uint16_t *positions, size_t npostings, size_t npositions,
                      uint8_t *index_out, size_t cap, size_t *index_len, uint8_t *hits_out, size_t hits_cap, size_t *hits_len, uint32_t *term_ids_out, tri_term *terms_out,
                      size_t terms_cap, size_t *nterms, tri_commit_stats *stats);

/* The same with hit payloads (Encoder::new_hit(pos, payload), google_codec.cpp:38-74): payload_lens[h] (0 .. 8) and payloads[h] (the
 * payload's first byte in the low 8 bits) per hit, parallel to positions[].  A hit is written as varint(position delta << 1 | the
 * length differs from the previous hit's of the document) [u8 new length] payload bytes, the length state restarting with every
 * document (:34).  A position-0 hit WITH a payload is a counted hit (:42-45); one without is refused, as by tri_encode_google.
 * payload_lens == NULL: no hit has a payload (tri_encode_google). */
int tri_encode_google_payloads(tri_dev *, const uint32_t *docs, const uint32_t *freqs, const uint16_t *positions, const uint8_t *payload_lens,
                               const uint64_t *payloads, size_t npositions, const uint64_t *term_first, size_t nterms, uint8_t *index_out, size_t cap,
                               size_t *index_len, tri_term *terms_out);

/* tri_encode_lucene / tri_commit_lucene with hit payloads (Encoder::new_hit(pos, payload), lucene_codec.cpp:240-304, 342-366): payload_lens[h] (0 .. 8) and
 * payloads[h] (the payload's first byte in the low 8 bits) per hit, parallel to positions[], as in tri_encode_google_payloads / tri_commit_google.  In hits.data a
 * full block of 128 hits is ints(position deltas) ints(payload lengths) varbyte(sum of the lengths) the payloads' bytes in hit order; the tail of fewer than 128
 * hits is per hit varbyte(position delta << 1 | the length differs from the tail's previous hit's) [u8 new length] — that state starts at 0 with the tail and
 * runs across document boundaries — and then the tail's payload bytes.  The term header's positionsChunkSize and the skiplist's lastHitsBlockOffset count the
 * payload bytes.  A position-0 hit WITH a payload is a counted hit; one without is refused.  Byte-identical to trinity_amd/csrc/host/lucene_encoder.hpp.
 * payload_lens == NULL: no hit has a payload — tri_encode_lucene / tri_commit_lucene, byte for byte.  payload_lens without payloads: TRI_ERR_INVALID. */
int tri_encode_lucene_payloads(tri_dev *, const uint32_t *docs, const uint32_t *freqs, const uint16_t *positions, const uint8_t *payload_lens, const uint64_t *payloads,
                               size_t npositions, const uint64_t *term_first, size_t nterms, uint8_t *index_out, size_t index_cap, size_t *index_len, uint8_t *hits_out,
                               size_t hits_cap, size_t *hits_len, tri_term *terms_out);
int tri_commit_lucene_payloads(tri_dev *, const uint32_t *term_ids, const uint32_t *doc_ids, const uint32_t *freqs, const uint16_t *positions, const uint8_t *payload_lens,
                               const uint64_t *payloads, size_t npostings, size_t npositions, uint8_t *index_out, size_t cap, size_t *index_len, uint8_t *hits_out,
                               size_t hits_cap, size_t *hits_len, uint32_t *term_ids_out, tri_term *terms_out, size_t terms_cap, size_t *nterms, tri_commit_stats *stats);

#ifdef __cplusplus
}
#endif
#endif

// trinity_hip.hip — libtrinity_hip.so: MI355X (gfx950 / CDNA4) execution engine for Trinity's query hot
// path.  Hand-written HIP; wave64; no MFMA (integer/byte work bounded by HBM + LDS + VALU issue).
//
// Data layout in HBM (built once at tri_index_upload):
//   index[]        raw reference-format segment bytes (google_codec.cpp:9-176 layout), +64 B slack
//   blk_last[]     u32 last docID of every block, all terms concatenated      (SoA: searched, 4 B/blk)
//   blk_off[]      u32 byte offset of every block's payload (first delta byte) (SoA: touched on decode)
//   terms[]        {documents, first_block, nblocks, last_n} per term
// The reference discovers block boundaries by hopping headers serially (google_codec.cpp:641-697) and
// keeps a sparse skiplist; a dense directory is the GPU analogue of Decoder::init (936-983).
//
// Kernels
//   k_decode_terms   one lane per block: prefix-varint stream decode of deltas+freqs (unpack_block 596-639)
//   k_and            persistent workgroups pull queries; per query the lead (lowest-df) list is decoded in
//                    tiles of 256 blocks into an LDS candidate array; every other term filters the tile:
//                    block-driven (dense) or candidate-driven galloping (sparse) over the block directory,
//                    one lane per needed block, merging the decoded docs against the candidates in LDS
//                    (Conjuction::next_impl leapfrog, docset_iterators.cpp:308-348, as a set operation)
//
// The read side — every result call of a batch and of a collection batch — is read_side.hpp, included behind the batch runtime; the write side — the
// encoders, commit and merge on the device (tri_encode_*, tri_commit_*, tri_merge_*) — is write_side.hpp, included at the end of this file: the same
// translation unit, as the k_*.hpp kernel files are.
#include "../../include/trinity_hip.h"
#include <chrono>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <unistd.h>
#include <dlfcn.h>
#include <memory>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <unordered_map>
#include <functional>
#include <vector>

// ------------------------------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";
static int fail(int code, const char *fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(g_err, sizeof g_err, fmt, ap);
        va_end(ap);
        return code;
}
#define HIP_TRY(expr)                                                                                       \
        do {                                                                                                \
                hipError_t e_ = (expr);                                                                     \
                if (e_ != hipSuccess)                                                                       \
                        return fail(e_ == hipErrorOutOfMemory ? TRI_ERR_NOMEM : TRI_ERR_DEVICE, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
        } while (0)

extern "C" const char *tri_last_error(void) { return g_err; }
extern "C" int tri_abi_version(void) { return TRI_ABI_VERSION; }

// the host planner (planner.hpp: options, PlanEnv, BatchPlan, plan_batch), the upload-time walk (index_host.hpp) and the structures
// the planner shares with the kernels (dev_structs.hpp)
#include "planner.hpp"

// the consumers of a batch's finished docID sets (consumers.hpp), in the order a run enqueues them; the read-only option that holds the device time of each one's
// last run (its events' span, read at tri_batch_sync)
enum Consumer { CONSUMER_FACETS, CONSUMER_ORDER, CONSUMER_STATS, CONSUMER_COUNT };
static const char *const CONSUMER_LAST_US[CONSUMER_COUNT] = {"facet_last_us", "order_last_us", "stats_last_us"};

struct tri_dev {
        int device;
        hipStream_t stream, stream2; // stream2: the candidate-tile kernel when the two matching kernels run side by side
        hipStream_t stream_up;       // plans travel to the device on their own stream: a batch is compiled and uploaded while the previous one runs
        hipStream_t stream_rb;       // read-backs of a SYNCED batch's results (docID sets, scores, hashes): they wait for nothing queued behind that batch on the engine stream
        hipEvent_t ev_fork, ev_join;
        int cus;
        tri_options opt;
        uint64_t rich_write_last_us = 0, rank_last_us = 0; // the last ranked batch's WRITE pass and rank pass (tri_dev_get_option, read-only)
        uint64_t consumer_last_us[CONSUMER_COUNT] = {};    // per consumer: its last run's initialisation + kernels (facets: row zeroing + k_facet; order: k_order + merge rounds)
        uint64_t crank_merge_last_us = 0;                  // the last ranked collection's merge of its parts' lists (k_rank_merge_sources)
        int refs = 0;         // indexes and batches alive on this handle ...
        bool closing = false; // ... tri_dev_close with some left: the handle goes with the last of them
        // The large buffers of a batch (output regions, score streams, term planes, decoded lists) and its plan arena are recycled from
        // batch to batch: a caller that compiles a batch per step would otherwise hipMalloc and hipFree gigabytes per step — hipFree
        // synchronises the device (the next batch cannot be compiled while the current one runs), and a cold 15 GB hipMalloc was measured
        // anywhere between 10 ms and 1 s (bench.py's end_to_end.batch_create_cold_ms).  One tri_dev per host thread: no lock.
        struct Pool {
                std::vector<std::pair<size_t, void *>> idle;    // (bytes, buffer) not in use
                std::unordered_map<void *, size_t> size_of;     // every pooled buffer, in use or idle
                size_t idle_bytes = 0;
        } pool;
        // ... likewise the pinned host blocks the plans are laid out in (hipHostMalloc costs about a millisecond per megabyte) ...
        std::vector<std::pair<size_t, void *>> pinned_idle;
        // ... and the HIP events of a batch (EV_COUNT per batch)
        std::vector<hipEvent_t> events_idle;
        // The planner's host threads: PLAN_CTXS independent planner contexts — a pool of host threads and the per-fragment arrays it recycles, under a
        // lock of their own — so that TWO threads may compile batches of this device at the same time (a create is 0.6 - 1.1 ms of host planning for
        // 16 K queries on 8 - 16 threads and scales no further: a caller whose steps are shorter than that compiles two batches side by side).  A
        // context's pool is started by the first large batch that finds the context free; pool k pins its workers to its own stretch of the CPUs.
        static constexpr unsigned PLAN_CTXS = 2;
        struct PlanCtx {
                std::mutex mu;                  // one batch at a time per context
                std::unique_ptr<HostPool> pool; // (created under mu)
                trip::FragCache frag_cache;     // (under mu)
        } planners[PLAN_CTXS];
        int plan_anchor = -1; // where the handle's pools count their CPUs from among the pin candidates (HostPool::anchor of the first pool started): context k's stretch starts k pools further on
        // The batch calls of one handle may come from TWO host threads: one compiling the next batch (tri_batch_create) while the other runs,
        // awaits and releases earlier ones (tri_batch_run / _sync / _destroy) — bench.py's loop; the planner's share of a create (most of it)
        // runs outside the lock, the pools above, the index's plane cache and everything that enqueues on the streams inside it.  Every other
        // entry point (uploads, options, encoders): one thread at a time, as before.
        std::recursive_mutex mu;
};
using DevLock = std::lock_guard<std::recursive_mutex>;
// a batch's ticket words (zeroed at every run): [0, TICKET_CAND_WORD) one per kernel; then k_and's CAND_QUEUES, 64 bytes apart
constexpr size_t TICKET_DENSE_WORD = 16;      // k_and_dense
constexpr size_t TICKET_PSET_WORD = 20;       // k_psets
constexpr size_t TICKET_PROBE_WORD = 22;      // k_probe
constexpr size_t TICKET_PLANES_WORD = 24;     // k_planes: + 2 for the wide instantiation
constexpr size_t TICKET_SCORE_WORD = 32;      // k_score ...
constexpr size_t TICKET_RICH_COUNT_WORD = TICKET_SCORE_WORD; // ... and k_rich's count pass share it: a batch is either scored or reports matched terms, never both
                                                            // (tri_batch_create: the modes are mutually exclusive)
constexpr size_t TICKET_RICH_WRITE_WORD = 40; // k_rich's write pass (cleared again before it)
constexpr size_t TICKET_RICH_WIDE = 2;        // ... + this: the same pass of the wide-report instantiation (its own launch, its own section of rich_sched)
constexpr size_t TICKET_SCAT_WORD = 44;       // k_psets_prep's cursor into the batch's scatter list (+ 1: k_psets_prep_list's count of scatter queries)
constexpr size_t TICKET_PHRASE_WORD = 48;     // k_phrase
constexpr size_t TICKET_FUSED_WORD = 56;      // k_fused: + 2 * variant (32-bit window words, 16-bit ones, general trees)
constexpr size_t TICKET_CAND_WORD = 64;
static_assert(std::max({TICKET_DENSE_WORD, TICKET_PSET_WORD, TICKET_PROBE_WORD, TICKET_PLANES_WORD + 2, TICKET_SCORE_WORD, TICKET_RICH_COUNT_WORD + TICKET_RICH_WIDE, TICKET_RICH_WRITE_WORD + TICKET_RICH_WIDE,
                        TICKET_SCAT_WORD + 1, TICKET_PHRASE_WORD, TICKET_FUSED_WORD + 2 * 2}) < TICKET_CAND_WORD,
              "every kernel's ticket word lies below k_and's queues");
constexpr size_t TICKET_BYTES = (TICKET_CAND_WORD + CAND_QUEUES * CAND_TICKET_STRIDE) * 4;
constexpr size_t POOL_MIN_BYTES = 64u << 10;  // smaller buffers are not worth pooling
constexpr size_t POOL_IDLE_CAP = 64ull << 30; // idle buffers beyond this are given back to the device (largest first)
constexpr size_t PINNED_IDLE_MAX = 16;        // idle pinned blocks kept (the longest idle one is dropped for a newly released one)

static void dev_destroy(tri_dev *d) {
        hipSetDevice(d->device);
        for (auto &pc : d->planners)
                pc.pool.reset();
        hipEventDestroy(d->ev_fork);
        hipEventDestroy(d->ev_join);
        for (hipEvent_t e : d->events_idle)
                hipEventDestroy(e);
        hipStreamDestroy(d->stream_up);
        hipStreamDestroy(d->stream_rb);
        hipStreamDestroy(d->stream2);
        hipStreamDestroy(d->stream);
        for (auto &b : d->pool.idle)
                hipFree(b.second);
        for (auto &b : d->pinned_idle)
                hipHostFree(b.second);
        delete d;
}
static void dev_retain(tri_dev *d) {
        DevLock g(d->mu);
        ++d->refs;
}
static void dev_release(tri_dev *d) {
        if (!d)
                return;
        bool last;
        {
                DevLock g(d->mu);
                last = --d->refs == 0 && d->closing;
        }
        if (last)
                dev_destroy(d);
}

// a buffer of at least `bytes`: an idle one of the pool that is not more than twice as large, else a fresh allocation
static hipError_t pool_alloc(tri_dev *dev, void **out, const size_t bytes) {
        if (bytes < POOL_MIN_BYTES)
                return hipMalloc(out, bytes);
        DevLock g(dev->mu);
        auto &P = dev->pool;
        size_t best = SIZE_MAX;
        for (size_t i = 0; i < P.idle.size(); ++i)
                if (P.idle[i].first >= bytes && P.idle[i].first <= 2 * bytes && (best == SIZE_MAX || P.idle[i].first < P.idle[best].first))
                        best = i;
        if (best != SIZE_MAX) {
                *out = P.idle[best].second;
                P.idle_bytes -= P.idle[best].first;
                P.idle.erase(P.idle.begin() + (ptrdiff_t)best);
                return hipSuccess;
        }
        const size_t gran = bytes >= (8u << 20) ? (2u << 20) : (64u << 10);
        const size_t rounded = (bytes + gran - 1) & ~(gran - 1);
        static const bool dbg_pool = getenv("TRINITY_DEBUG_CREATE") != nullptr;
        if (dbg_pool) {
                std::string have;
                for (const auto &b : P.idle)
                        have += " " + std::to_string(b.first >> 20);
                fprintf(stderr, "[tri pool_alloc] COLD hipMalloc of %zu MB (idle buffers, MB:%s)\n", rounded >> 20, have.c_str());
        }
        hipError_t e = hipMalloc(out, rounded);
        if (e != hipSuccess && !P.idle.empty()) { // out of memory with idle buffers around: give them back and try again
                (void)hipGetLastError();
                for (auto &b : P.idle) {
                        P.size_of.erase(b.second);
                        hipFree(b.second);
                }
                P.idle.clear();
                P.idle_bytes = 0;
                e = hipMalloc(out, rounded);
        }
        if (e == hipSuccess)
                P.size_of[*out] = rounded;
        return e;
}
static void pool_free(tri_dev *dev, void *p) { // (p != nullptr: the owners' release, as pinned_free and event_put are)
        if (!dev) {
                hipFree(p);
                return;
        }
        DevLock g(dev->mu);
        auto &P = dev->pool;
        const auto it = P.size_of.find(p);
        if (it == P.size_of.end()) { // (below POOL_MIN_BYTES: never pooled)
                hipFree(p);
                return;
        }
        P.idle.emplace_back(it->second, p);
        P.idle_bytes += it->second;
        while (P.idle_bytes > POOL_IDLE_CAP) {
                size_t big = 0;
                for (size_t i = 1; i < P.idle.size(); ++i)
                        if (P.idle[i].first > P.idle[big].first)
                                big = i;
                P.idle_bytes -= P.idle[big].first;
                P.size_of.erase(P.idle[big].second);
                hipFree(P.idle[big].second);
                P.idle.erase(P.idle.begin() + (ptrdiff_t)big);
        }
}
// pinned host block of at least `bytes` (64-byte aligned: hipHostMalloc is page-aligned); *cap = its size
static uint8_t *pinned_alloc(tri_dev *dev, const size_t bytes, size_t *cap) {
        DevLock g(dev->mu);
        auto &I = dev->pinned_idle;
        size_t best = SIZE_MAX;
        for (size_t i = 0; i < I.size(); ++i)
                if (I[i].first >= bytes && I[i].first <= 4 * bytes + (1u << 20) && (best == SIZE_MAX || I[i].first < I[best].first))
                        best = i;
        if (best != SIZE_MAX) {
                void *p = I[best].second;
                *cap = I[best].first;
                I.erase(I.begin() + (ptrdiff_t)best);
                return static_cast<uint8_t *>(p);
        }
        const size_t rounded = (bytes + bytes / 4 + (256u << 10)) & ~(size_t)((64u << 10) - 1); // (a quarter of slack: the next batch of the same caller is about as large)
        void *p = nullptr;
        if (hipHostMalloc(&p, rounded, hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError();
                return nullptr;
        }
        *cap = rounded;
        return static_cast<uint8_t *>(p);
}
static void pinned_free(tri_dev *dev, void *p, const size_t cap) {
        DevLock g(dev->mu);
        if (dev->pinned_idle.size() >= PINNED_IDLE_MAX) { // full: the block idle for longest goes, the one just released stays — the list follows the
                hipHostFree(dev->pinned_idle.front().second); // caller's CURRENT batches (a list full of another workload's block sizes made every create
                dev->pinned_idle.erase(dev->pinned_idle.begin()); // of the next one a hipHostMalloc: bench.py's cfg2 loop after its cfg5 leg, 1.2 -> 4 ms a create)
        }
        dev->pinned_idle.emplace_back(cap, p);
}
static void event_put(tri_dev *dev, hipEvent_t e) {
        DevLock g(dev->mu);
        dev->events_idle.push_back(e);
}
static hipError_t event_get(tri_dev *dev, hipEvent_t *e) {
        DevLock g(dev->mu);
        if (!dev->events_idle.empty()) {
                *e = dev->events_idle.back();
                dev->events_idle.pop_back();
                return hipSuccess;
        }
        return hipEventCreate(e);
}

// the owning handles over the calls above: DevMem, Pooled, Pinned, PooledEvent, DevRef
#include "owners.hpp"
// the index's plane cache: its rows' bookkeeping, its buffers, its growth (PlaneRows, PlaneCache)
#include "plane_cache.hpp"

// An arena's sections, each named ONCE: carve(view, bytes) points `view` at the next section and moves on by `bytes`, rounded up to `align`.  Without a base
// (the sizing pass) no view is touched and only `at` advances; `have` == false: the object lacks the section — a null view, no room taken.
struct Carver {
        uint8_t *base;
        size_t at = 0, align = 256;
        template <class T>
        void operator()(T *&view, const size_t bytes, const bool have = true) {
                if (base)
                        view = have ? reinterpret_cast<T *>(base + at) : nullptr;
                if (have)
                        at += (bytes + align - 1) & ~(align - 1);
        }
};

// the uploaded segment: what the walk derived (HostIndex; the planner reads terms / blk_last / docbytes / hitbytes / win / the df order)
// plus its device copies
struct tri_index : HostIndex {
        DevRef dev; // FIRST: members go in reverse order of declaration, so the handle is let go of after every buffer and event below went back to it
        DevMem<uint8_t> d_index, d_hits;
        DevMem<uint32_t> d_blk_last, d_blk_off, d_win;
        DevMem<uint32_t> d_blk_hits, d_hdir; // where a directory row's hits start — LUCENE + hits.data: hit ordinal within the term
        DevMem<uint32_t> d_pdir;             // LUCENE + hits.data: [term] = the term's payload directory row in this same array (~0: no hit of it carries a payload), then the rows
        bool any_hit_payloads = false;       // ... and whether any term has one
                                                           // (+ hdir: the 128-hit blocks of hits.data); GOOGLE: byte offset into index[]
        // GOOGLE: the document deltas of every block re-laid out as one contiguous stream per term ([n][n-1 prefix varints] per
        // block, bytes exactly as in the chunk) with its own offset column.  In the chunk a block's deltas are followed by its
        // freqs and hits, so a DocumentsOnly scan of a head term drags ~3x the bytes it decodes through HBM; the matching kernels
        // (k_and_dense, k_and) read this stream instead.  Scoring and phrases keep reading the chunk itself.
        DevMem<uint8_t> d_dstream;
        DevMem<uint32_t> d_blk_doff;
        // LUCENE: one 16-byte record per directory row (a quarter of a 128-document block, or a run of the varbyte tail) with all a lane
        // needs to address the row's payload in ONE load: {offset of the deltas group (tail: of the pairs), exception index, header word of
        // the deltas group, header word of the freqs group}.  Exception index = where THIS quarter's exceptions sit in the two groups'
        // lists: e0_deltas | cnt_deltas << 8 | e0_freqs << 16 | cnt_freqs << 24 (a lane patches its quarter without scanning the other
        // three's).  Header word = the group's first payload word (width | nexc << 8 | excwidth << 16), or bit 31 | value for an
        // all-equal group (k_fused.hpp PfRegs)
        DevMem<uint4> d_blk_rec;
        DevMem<uint32_t> d_masked; // bitmap over docIDs of the masked documents (nullptr: none); max_doc / 32 + 2 words
        DevMem<DevTerm> d_terms;
        PlaneCache planes; // the term planes of the head terms, built by need and kept from batch to batch (plane_cache.hpp)
        ~tri_index() { // also runs when tri_index_upload fails half-way; the members release themselves behind it
                if (dev)
                        hipSetDevice(dev->device);
        }
};

// A per-query document filter (IndexDocumentsFilter, matches.h:190-201) as the device keeps it: a bitmap over the index's docIDs in DROP polarity, of the
// extent of d_masked (filter_words).  It belongs to its index — destroyed before it, like a batch — and is only read by the batches that name it
// (tri_batch_set_filters): their runs OR it with the mask of the moment into a row of their own (k_filter.hpp)
struct tri_filter {
        DevRef dev; // (first: released last)
        tri_index *ix = nullptr;
        Pooled<uint32_t> d_bits;
        size_t words = 0;
        ~tri_filter() {
                if (dev)
                        hipSetDevice(dev->device);
        }
};
// A per-document attribute column (tri_column_create): values[d] for docID d = 0 .. docs_cnt, resident in HBM.  It belongs to its index — destroyed before it — and
// is only read by the runs of the batches that name it (tri_batch_set_facets: k_facet.hpp)
struct tri_column {
        DevRef dev; // (first: released last)
        tri_index *ix = nullptr;
        DevMem<uint32_t> d_values; // an owning device buffer (hipFree waits for every run that may still read it)
        uint32_t n = 0;
        ~tri_column() {
                if (dev)
                        hipSetDevice(dev->device);
        }
};
// whole docID windows (the bitmap kernels read a window's worth of words at a time), one spare window: the extent of d_masked and of every filter
static size_t filter_words(const tri_index *ix) { return ((size_t)ix->max_doc / SPAN_BITS + 2) * SPAN_WORDS; }

// a batch's HIP events, in the order they are recorded: EV_UP, the plan has arrived (upload stream); then on the engine stream the run's start,
// the end of each of its stages (tri_batch_run), the run's end
enum BatchEvent { EV_UP, EV_START, EV_PLANE_ROWS, EV_DENSE, EV_PSET, EV_PROBE, EV_CAND, EV_FUSED, EV_PLANES, EV_PHRASE, EV_TREE, EV_END, EV_COUNT };

// a compiled batch: the plan (BatchPlan: the host block with every array the kernels read, laid out by the planner) and its device side —
// ONE arena that holds the block's copy followed by the batch's small device-only arrays, plus the large pooled buffers
struct tri_batch : BatchPlan {
        DevRef dev; // FIRST: members go in reverse order of declaration, so the handle is let go of after every buffer and event below went back to it
        tri_index *ix = nullptr;
        uint32_t flags, topk;
        int similarity = TRI_SIM_BM25;
        size_t nq;
        // ---- what the batch OWNS: each member releases itself (owners.hpp), behind ~tri_batch's waits
        Pinned<uint8_t> pinned;   // the pinned host block BatchPlan::block points at
        Pooled<uint8_t> d_arena;  // [copy of block], then batch_arena()'s sections: the run's small arrays, and last the ones zeroed at creation
        PooledEvent ev[EV_COUNT]; // (owned by the batch: two batches in flight on one device keep their own timings)
        Pooled<uint32_t> d_sparse; // k_planes: per resident workgroup, the lists of a task's decoded (non-plane) slots
        Pooled<uint32_t> d_out;
        Pooled<uint32_t> d_rich_allow; // default mode, batches that hold general trees: per match the reportable terms the tree sits on
        DevMem<uint64_t> d_hashes;
        // AccumulatedScoreScheme
        Pooled<uint32_t> d_part_docs;
        Pooled<double> d_part_scores, d_all_scores; // (d_all_scores: topk == 0, one double per out[] slot)
        // TRI_FLAG_MATCHED_TERMS (k_rich.hpp): sterms[] holds every query's reportable terms; R = the widest query's count
        Pooled<uint32_t> d_rich_present;
        Pooled<uint16_t> d_rich_freq;
        // ... with wide-report queries (option rich_max_terms; BatchPlan::rich_wide says where a query's share of each lies): their frequency rows, and the high
        // halves of their matches' present / allow masks — d_rich_present / d_rich_allow keep the low halves of every query, laid out as ever
        Pooled<uint16_t> d_rich_freq_wide;
        Pooled<uint32_t> d_rich_present_hi, d_rich_allow_hi;
        DevMem<uint16_t> d_rich_pool;
        DevMem<uint8_t> d_rich_plen;     // TRI_FLAG_HIT_PAYLOADS: per hit of the pool, term_hit::payloadLen ...
        DevMem<uint64_t> d_rich_payload; // ... and term_hit::payload
        Pooled<double> d_pscore; // phrases, per out[] slot: sum of the phrase scores of the match (scored mode)
        // TASK_TREE (k_tree.hpp): one scratch block — [tree rows: a PL_PLANES-plane row per distinct term leaf][phrase rows: a plane per hidden phrase query]
        // [a match bitmap per tree query][per query and chunk: matches][(term, row) pairs for k_term_planes]
        Pooled<uint32_t> d_tree_scratch;
        Pooled<double> d_tree_scores; // scored top-K batches: the tree queries' score stream (topk == 0: d_all_scores holds it)
        Pooled<uint32_t> d_scat_docs; // PSET_UNIT_SCATTER unions: the list k_psets_prep makes (k_psets.hpp)
        // per-query filters (tri_batch_set_filters; stored by reference): filter_rows[r - 1] = the filter behind row id r — the filters at least one query
        // names —, d_filter_tab = [row id per plan slot][the rows' source pointers], d_filter_rows = the rows every run rebuilds (filter | mask)
        Pooled<uint8_t> d_filter_tab;
        Pooled<uint32_t> d_filter_rows;
        Pooled<uint8_t> d_rank_block; // tri_batch_set_ranker (k_rich_rank.hpp): ONE block, rank_block()'s sections
        // the consumers of the finished docID sets (consumers.hpp: tri_batch_set_facets / _order / _stats), one slot each: ONE pooled block, the events around the
        // run's initialisation + kernels (option *_last_us), and where its lifecycle stands.  The blocks:
        //   facets  [facet][caller query][nbuckets + 1] counters, zeroed and recounted by every run (k_facet.hpp)
        //   order   the tasks' partial lists, the merge's two intermediate levels and the rows ([caller query][topk] keys), then a length per list and row (k_order.hpp)
        //   stats   per stat four planes (sums u64, counts, mins, maxs u32), each [caller query][nbuckets + 1], initialised and aggregated again by every run (k_stats.hpp)
        struct ConsumerSlot {
                Pooled<uint64_t> block;
                PooledEvent ev[2];
                bool on = false;                // a spec stands
                bool ran = false, done = false; // the last run consumed with the spec that stands; ... and tri_batch_sync has awaited it
                uint32_t launches = 0;          // kernels per run of the spec that stands: 1, 1 + the merge's rounds, 1
        } consumers[CONSUMER_COUNT];
        DevMem<DevOrderGroup> d_order_groups; // the order's merge groups (they depend on the plan alone: laid out by the first setter)
        // ---- VIEWS: plain pointers into the buffers above, released with them
        // a section of the plan (a Span of BatchPlan: planner_types.hpp, for_each_section) on the device — the block's copy opens the arena
        template <class T>
        T *dev_at(const Span<T> &s) const {
                return reinterpret_cast<T *>(d_arena + s.off);
        }
        template <class T>
        T *dev_opt(const Span<T> &s) const { // ... one that a batch may lack (qplane, splane): nullptr tells the kernels so
                return s.empty() ? nullptr : dev_at(s);
        }
        // into d_arena (batch_arena)
        uint32_t *d_counts = nullptr; // per task, indexed first_task + i in query order
        uint32_t *d_ticket = nullptr;
        uint32_t *d_build = nullptr; // (term, row) pairs of the plane rows a run has to build first
        unsigned long long *d_qthr = nullptr; // k_planes: per query, the best k-th score any of its tasks has seen (cleared at every run)
        uint32_t *d_part_counts = nullptr;
        uint32_t *d_score_order = nullptr; // AccumulatedScore: the tasks k_score runs, heaviest first by their match counts (k_score_order)
        uint32_t *d_task_hits = nullptr;
        uint64_t *d_task_pos_base = nullptr;
        uint32_t *d_scat_off = nullptr, *d_scat_cnt = nullptr; // PSET_UNIT_SCATTER unions: per task its slice of d_scat_docs
        uint32_t *d_scat_list = nullptr; // ... the scatter queries' first units (k_psets_prep_list)
        uint64_t *d_qcounts = nullptr; // per caller query: matches of the last run (device copy for the result gather)
        uint32_t *d_top_counts = nullptr, *d_top_docs = nullptr;
        float *d_top_scores = nullptr;
        // into d_tree_scratch (tree_scratch)
        uint32_t *d_tree_rows = nullptr, *d_tree_prows = nullptr, *d_tree_qbits = nullptr, *d_tree_cc = nullptr, *d_tree_build = nullptr;
        // into d_rank_block (rank_block): [a weight per sterms[] entry][the tasks' partial lists][the queries' ranked lists]
        double *d_rank_w = nullptr, *d_rank_part_scores = nullptr, *d_rank_scores = nullptr;
        uint32_t *d_rank_part_docs = nullptr, *d_rank_part_counts = nullptr, *d_rank_docs = nullptr, *d_rank_counts = nullptr;
        // ---- host state
        uint32_t scat_cap = 0;
        bool ran = false;
        bool planes_hi = false; // the batch reads the HIGH parts of its plane rows (k_planes, k_score's level words): its run builds them where they are missing
        std::vector<uint64_t> h_task_pos_base; // per task; [ntasks] = the pool's size
        size_t rich_pool_cap = 0;
        std::vector<uint32_t> h_counts;       // per task
        std::vector<uint64_t> h_query_counts; // per plan slot
        bool synced = false;
        std::vector<const tri_filter *> filter_rows;
        size_t filter_rows_cap = 0; // rows d_filter_rows holds
        // tri_batch_set_ranker: the spec, and the caller's program (kept by default-mode batches: the ranker's weights come one per program token)
        bool rank_on = false, rank_done = false;
        tri_ranker rank{};
        // the consumers' specs as the kernels take them (the columns by reference), each next to its slot's typed view
        DevFacets facets{};        // (n == 0: none)
        size_t facet_counters = 0; // counters of the facets' block
        uint32_t *facet_rows() const { return reinterpret_cast<uint32_t *>(consumers[CONSUMER_FACETS].block.get()); }
        DevStats stats{};       // (n == 0: none)
        size_t stats_words = 0; // 32-bit words of the stats' block
        uint32_t *stats_rows() const { return reinterpret_cast<uint32_t *>(consumers[CONSUMER_STATS].block.get()); }
        struct OrderRound {
                uint32_t first_group, ngroups; // of d_order_groups
        };
        DevOrder order{};
        bool order_laid_out = false;
        std::vector<OrderRound> order_rounds; // round r reads the tasks' lists (r == 0) or level (r - 1) & 1, and writes rows and level r & 1
        size_t order_level[2] = {0, 0};       // lists of the two intermediate levels
        size_t order_lists = 0;               // lists of the order's block ahead of its rows: tasks + both levels
        uint64_t *order_keys(const size_t list) const { return consumers[CONSUMER_ORDER].block.get() + list * order.topk; }
        uint32_t *order_counts(const size_t list) const { return reinterpret_cast<uint32_t *>(consumers[CONSUMER_ORDER].block.get() + (order_lists + nq) * order.topk) + list; }
        std::vector<uint32_t> h_prog;
        std::vector<tri_query> h_queries;
        tri_batch_info info{};
        ~tri_batch() { // also runs when tri_batch_create fails half-way.  Only the waits stand here: they come before any member is released
                if (!dev)
                        return;
                hipSetDevice(dev->device);
                if (ran && !synced) // (its large buffers go back to the device's pool: nothing of this batch may still be running on them)
                        hipStreamSynchronize(dev->stream);
                if (ev[EV_UP])
                        hipEventSynchronize(ev[EV_UP]); // (the pinned block goes back to the pool: its copy must have left)
        }
};


#include "dev_stream.hpp"
#include "k_decode.hpp"
#include "k_match.hpp"
#include "k_score.hpp"
#include "k_fused.hpp"
#include "k_planes.hpp"
#include "k_psets.hpp"
#include "k_probe.hpp"
#include "k_encode.hpp"
#include "k_phrase.hpp"
#include "k_rich.hpp"
#include "k_rich_rank.hpp"
#include "k_decode_hits.hpp"
#include "k_isect.hpp"
#include "k_tree.hpp"
#include "k_tree_wide.hpp"
#include "k_perc.hpp"
#include "k_facet.hpp"
#include "k_order.hpp"
#include "k_stats.hpp"
#include "k_commit.hpp"
#include "k_lencode.hpp"
#include "k_filter_columns.hpp" // (beside k_filter.hpp's own kernels: column predicates -> drop bitmaps)
#include "filtered_kernels.hpp"

// launch the instantiation of a codec-templated kernel that matches the uploaded segment: `pick` maps the codec (a std::integral_constant: the
// kernel template's first argument) to the kernel, and chooses the template's other arguments, if it has any.  The arguments are forwarded: an owner
// (owners.hpp) becomes the kernel's pointer at the kernel call
template <class Pick, class... Args>
static void tri_launch(const int codec, Pick pick, const dim3 grid, const dim3 block, const hipStream_t stream, Args &&...args) {
        if (codec == TRI_CODEC_LUCENE)
                hipLaunchKernelGGL(pick(std::integral_constant<int, CODEC_LUCENE>()), grid, block, 0, stream, std::forward<Args>(args)...);
        else
                hipLaunchKernelGGL(pick(std::integral_constant<int, CODEC_GOOGLE>()), grid, block, 0, stream, std::forward<Args>(args)...);
}
// ... of a kernel whose only template argument is the codec
#define TRI_LAUNCH(K, codec, grid, block, stream, ...) tri_launch(codec, [](auto c_) { return K<c_.value>; }, grid, block, stream, __VA_ARGS__)

// ------------------------------------------------------------------------------------------ host: device
extern "C" int tri_dev_open(int device, tri_dev **out) {
        if (!out)
                return fail(TRI_ERR_INVALID, "tri_dev_open: null out");
        int n = 0;
        HIP_TRY(hipGetDeviceCount(&n));
        if (device < 0 || device >= n)
                return fail(TRI_ERR_INVALID, "tri_dev_open: device %d out of range (%d devices)", device, n);
        HIP_TRY(hipSetDevice(device));
        auto d = std::make_unique<tri_dev>();
        d->device = device;
        HIP_TRY(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&d->stream2, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&d->stream_up, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&d->stream_rb, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&d->ev_fork, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&d->ev_join, hipEventDisableTiming));
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, device));
        d->cus = prop.multiProcessorCount;
        *out = d.release();
        return TRI_OK;
}

extern "C" void tri_dev_close(tri_dev *d) {
        if (!d)
                return;
        // indexes or batches of this handle still alive (a caller that closes first and destroys later): they keep using the handle's
        // streams and pools, and the last of them to go takes the handle along
        if (d->refs > 0) {
                d->closing = true;
                return;
        }
        dev_destroy(d);
}

namespace {
        uint64_t *option_slot(tri_options &o, const char *name) {
                static const struct {
                        const char *name;
                        uint64_t tri_options::*field;
                } table[] = {{"dense_min_postings", &tri_options::dense_min_postings}, {"dense_task_cost", &tri_options::dense_task_cost},
                             {"fused", &tri_options::fused},
                             {"fused_task_cost", &tri_options::fused_task_cost},
                             {"fused_freq_cap", &tri_options::fused_freq_cap},
                             {"fused_halfwords", &tri_options::fused_halfwords},
                             {"account_needed_bytes", &tri_options::account_needed_bytes},
                             {"overlap_dense_wgs", &tri_options::overlap_dense_wgs},
                             {"overlap_cand_wgs", &tri_options::overlap_cand_wgs},
                             {"overlap", &tri_options::overlap},
                             {"planes", &tri_options::planes},
                             {"plane_div", &tri_options::plane_div},
                             {"planes_split", &tri_options::planes_split},
                             {"plane_max_bytes", &tri_options::plane_max_bytes},
                             {"plane_amortize", &tri_options::plane_amortize},
                             {"planes_rebuild", &tri_options::planes_rebuild},
                             {"cand_xcd", &tri_options::cand_xcd},
                             {"plan_threads", &tri_options::plan_threads},
                             {"probe_max_blocks", &tri_options::probe_max_blocks}, {"phrase_task_div", &tri_options::phrase_task_div}, {"plan_hot_us", &tri_options::plan_hot_us}, {"plan_pin", &tri_options::plan_pin}, {"planes_order", &tri_options::planes_order}, {"pset_order", &tri_options::pset_order}, {"scatter_bitmap_slack", &tri_options::scatter_bitmap_slack}, {"tree_max_bytes", &tri_options::tree_max_bytes}, {"tree_max_nodes", &tri_options::tree_max_nodes}, {"tree_wide_min_nodes", &tri_options::tree_wide_min_nodes}, {"rich_max_terms", &tri_options::rich_max_terms}, {"result_bitmaps", &tri_options::result_bitmaps}, {"cand_task_cost", &tri_options::cand_task_cost}, {"dense_window_cost", &tri_options::dense_window_cost},
                             {"isect_max_bytes", &tri_options::isect_max_bytes}, {"isect_max_masks", &tri_options::isect_max_masks}, {"isect_max_runs", &tri_options::isect_max_runs},
                             {"perc_max_bytes", &tri_options::perc_max_bytes}, {"perc_prune", &tri_options::perc_prune}};
                for (const auto &e : table)
                        if (!strcmp(e.name, name))
                                return &(o.*(e.field));
                return nullptr;
        }
} // namespace

extern "C" int tri_dev_set_option(tri_dev *d, const char *name, uint64_t value) {
        if (!d || !name)
                return fail(TRI_ERR_INVALID, "tri_dev_set_option: null argument");
        uint64_t *slot = option_slot(d->opt, name);
        if (!slot)
                return fail(TRI_ERR_INVALID, "tri_dev_set_option: unknown option '%s'", name);
        *slot = value;
        return TRI_OK;
}

extern "C" int tri_dev_get_option(tri_dev *d, const char *name, uint64_t *value) {
        if (!d || !name || !value)
                return fail(TRI_ERR_INVALID, "tri_dev_get_option: null argument");
        // (read-only: the device time of the last ranked batch's WRITE pass and rank pass — HIP events around them, tri_batch_sync)
        if (!strcmp(name, "rich_write_last_us") || !strcmp(name, "rank_last_us")) {
                *value = !strcmp(name, "rich_write_last_us") ? d->rich_write_last_us : d->rank_last_us;
                return TRI_OK;
        }
        for (int i = 0; i < CONSUMER_COUNT; ++i) // (... of the last run of each docset consumer: facets, order, stats, tri_batch_sync)
                if (!strcmp(name, CONSUMER_LAST_US[i])) {
                        *value = d->consumer_last_us[i];
                        return TRI_OK;
                }
        if (!strcmp(name, "crank_merge_last_us")) { // (... and of the last ranked collection's merge kernel, tri_cbatch_sync)
                *value = d->crank_merge_last_us;
                return TRI_OK;
        }
        const uint64_t *slot = option_slot(d->opt, name);
        if (!slot)
                return fail(TRI_ERR_INVALID, "tri_dev_get_option: unknown option '%s'", name);
        *value = *slot;
        return TRI_OK;
}

extern "C" int tri_dev_memory(tri_dev *d, tri_dev_memory_info *out) {
        if (!d || !out)
                return fail(TRI_ERR_INVALID, "tri_dev_memory: null argument");
        HIP_TRY(hipSetDevice(d->device));
        size_t fr = 0, total = 0;
        HIP_TRY(hipMemGetInfo(&fr, &total));
        DevLock g(d->mu);
        uint64_t all = 0, pinned = 0;
        for (const auto &kv : d->pool.size_of)
                all += kv.second;
        for (const auto &pb : d->pinned_idle)
                pinned += pb.first;
        out->pool_idle_bytes = d->pool.idle_bytes;
        out->pool_in_use_bytes = all - d->pool.idle_bytes;
        out->pinned_idle_bytes = pinned;
        out->device_free_bytes = fr;
        out->device_total_bytes = total;
        return TRI_OK;
}

extern "C" int tri_dev_sync(tri_dev *d) {
        if (!d)
                return fail(TRI_ERR_INVALID, "null dev");
        HIP_TRY(hipStreamSynchronize(d->stream));
        return TRI_OK;
}

extern "C" void *tri_dev_stream(tri_dev *d) { return d ? (void *)d->stream : nullptr; }

// ------------------------------------------------------------------------------------------ host: upload
namespace {
        template <class T>
        int dev_upload(DevMem<T> &dst, const std::vector<T> &src, size_t extra = 0) {
                HIP_TRY(dst.alloc((src.size() + extra) * sizeof(T) + 16));
                if (!src.empty())
                        HIP_TRY(hipMemcpy(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
                return TRI_OK;
        }
} // namespace

extern "C" int tri_index_upload(tri_dev *dev, const uint8_t *index, size_t len, const uint8_t *hits, size_t hits_len, int codec,
                                const tri_term *terms, size_t nterms, uint32_t docs_cnt, tri_index **out) {
        if (!dev || !out || (!index && len) || (!terms && nterms) || (!hits && hits_len))
                return fail(TRI_ERR_INVALID, "tri_index_upload: null argument");
        HIP_TRY(hipSetDevice(dev->device));
        auto ix = std::make_unique<tri_index>();
        // One pass over every chunk on the host (index_host.hpp): hop block headers (google_codec.cpp:641-697), validate, record the
        // directory, the delta streams / row records, the docID-cell index and the algorithmic byte split of SURVEY §8(d)
        {
                std::string err;
                if (const int rc = build_host_index(index, len, hits, hits_len, codec, terms, nterms, docs_cnt, *ix, err))
                        return fail(rc, "%s", err.c_str());
        }
        ix->dev.retain(dev);
        if (!ix->dev_index.empty()) { // a LUCENE segment with FastPFor<4> payload words: the device gets its PFOR128 transcription (index_host.hpp)
                index = ix->dev_index.data();
                len = ix->dev_index.size();
                hits = ix->dev_hits.empty() ? nullptr : ix->dev_hits.data();
                hits_len = ix->dev_hits.size();
        }
        // device copies
        int rc;
        if ((rc = dev_upload(ix->d_win, ix->win, 3 * CELLS_PER_SPAN + 8))) // (lanes of terms without a row read entries 0, CELLS_PER_SPAN, 2 * CELLS_PER_SPAN and drop them)
                return rc;
        HIP_TRY(hipMemset(ix->d_win + ix->win.size(), 0, (3 * CELLS_PER_SPAN + 8) * sizeof(uint32_t)));
        HIP_TRY(ix->d_index.alloc(len + 256)); // over-read slack: the byte streams keep several qwords in flight past the cursor
        HIP_TRY(hipMemset(ix->d_index, 0, len + 256));
        if (len)
                HIP_TRY(hipMemcpy(ix->d_index, index, len, hipMemcpyHostToDevice));
        if ((rc = dev_upload(ix->d_blk_last, ix->blk_last)) || (rc = dev_upload(ix->d_blk_off, ix->blk_off)) || (rc = dev_upload(ix->d_terms, ix->terms)))
                return rc;
        if (codec == TRI_CODEC_GOOGLE) {
                ix->blk_doff.push_back((uint32_t)ix->dstream.size() + 1); // (sentinel: block b's delta bytes = blk_doff[b + 1] - blk_doff[b] - 1 for the last block too)
                ix->dstream.resize(ix->dstream.size() + 256, 0); // over-read slack, like index[]
                if ((rc = dev_upload(ix->d_dstream, ix->dstream)) || (rc = dev_upload(ix->d_blk_doff, ix->blk_doff)))
                        return rc;
        }
        if (hits_len) { // LUCENE: hits.data (positions) resident next to the index
                HIP_TRY(ix->d_hits.alloc(hits_len + 256));
                HIP_TRY(hipMemset(ix->d_hits, 0, hits_len + 256));
                HIP_TRY(hipMemcpy(ix->d_hits, hits, hits_len, hipMemcpyHostToDevice));
                if (ix->has_hdir && ((rc = dev_upload(ix->d_blk_hits, ix->blk_hits)) || (rc = dev_upload(ix->d_hdir, ix->hdir))))
                        return rc;
                if (ix->has_hdir) { // the payload directory (index_host.hpp), built on the image the device gets: the terms' rows made offsets into ONE array
                        std::vector<uint32_t> pd(ix->pdir_off);
                        for (uint32_t &o : pd)
                                if (o != 0xffffffffu)
                                        o += (uint32_t)nterms;
                        ix->any_hit_payloads = !ix->pdir.empty();
                        pd.insert(pd.end(), ix->pdir.begin(), ix->pdir.end());
                        if ((rc = dev_upload(ix->d_pdir, pd)))
                                return rc;
                }
        }
        if (codec == TRI_CODEC_GOOGLE && (rc = dev_upload(ix->d_blk_hits, ix->blk_hits)))
                return rc;
        if (codec == TRI_CODEC_LUCENE) {
                static_assert(sizeof(RowRec) == sizeof(uint4), "row records are read as uint4");
                HIP_TRY(ix->d_blk_rec.alloc(ix->blk_rec.size() * sizeof(uint4) + 16));
                if (!ix->blk_rec.empty())
                        HIP_TRY(hipMemcpy(ix->d_blk_rec, ix->blk_rec.data(), ix->blk_rec.size() * sizeof(uint4), hipMemcpyHostToDevice));
        }
        ix->release_device_columns(); // (the host keeps what the planner reads: terms, blk_last, docbytes / hitbytes, win, the df order)
        *out = ix.release();
        return TRI_OK;
}


extern "C" int tri_index_set_masked(tri_index *ix, const uint32_t *docids, size_t n) {
        if (!ix || (!docids && n))
                return fail(TRI_ERR_INVALID, "tri_index_set_masked: null argument");
        HIP_TRY(hipSetDevice(ix->dev->device));
        HIP_TRY(hipStreamSynchronize(ix->dev->stream)); // no batch of this device is reading the old bitmap
        if (!n) {
                ix->d_masked.reset();
                return TRI_OK;
        }
        // whole docID windows (the bitmap kernel reads a window's worth of words at a time), one spare window
        const size_t words = ((size_t)ix->max_doc / SPAN_BITS + 2) * (SPAN_BITS / 32);
        std::vector<uint32_t> bm(words, 0);
        for (size_t i = 0; i < n; ++i)
                if (docids[i] <= ix->max_doc) // a document this segment does not hold cannot match anyway
                        bm[docids[i] >> 5] |= 1u << (docids[i] & 31);
        if (!ix->d_masked)
                HIP_TRY(ix->d_masked.alloc(words * 4));
        HIP_TRY(hipMemcpy(ix->d_masked, bm.data(), words * 4, hipMemcpyHostToDevice));
        return TRI_OK;
}

extern "C" void tri_index_destroy(tri_index *ix) {
        delete ix; // its members release the device buffers
}

extern "C" int tri_index_get_info(const tri_index *ix, tri_index_info *info) {
        if (!ix || !info)
                return fail(TRI_ERR_INVALID, "null argument");
        *info = ix->info;
        return TRI_OK;
}

extern "C" int tri_index_term_docbytes(const tri_index *ix, const uint32_t *terms, size_t n, uint64_t *out) {
        if (!ix || (!terms && n) || (!out && n))
                return fail(TRI_ERR_INVALID, "null argument");
        for (size_t i = 0; i < n; ++i)
                out[i] = terms[i] < ix->docbytes.size() ? ix->docbytes[terms[i]] : 0;
        return TRI_OK;
}

// ------------------------------------------------------------------------------------------ host: decode
extern "C" int tri_decode_terms(tri_index *ix, const uint32_t *terms, size_t n, uint32_t *docs, uint32_t *freqs, uint64_t *out_offsets) {
        if (!ix || (!terms && n) || !out_offsets)
                return fail(TRI_ERR_INVALID, "null argument");
        tri_dev *dev = ix->dev;
        HIP_TRY(hipSetDevice(dev->device));
        std::vector<DecodeJob> jobs(n);
        uint64_t tot = 0, padded = 0;
        uint32_t maxblocks = 0;
        for (size_t i = 0; i < n; ++i) {
                if (terms[i] >= ix->terms.size())
                        return fail(TRI_ERR_INVALID, "term %u out of range", terms[i]);
                const DevTerm &t = ix->terms[terms[i]];
                jobs[i] = {terms[i], 0, padded};
                out_offsets[i] = tot;
                tot += t.documents;
                padded += (uint64_t)t.nblocks * 32;
                maxblocks = std::max(maxblocks, t.nblocks);
        }
        out_offsets[n] = tot;
        if (!tot || !docs)
                return TRI_OK;
        DevMem<DecodeJob> d_jobs; // (of this call: not pooled)
        DevMem<uint32_t> d_docs, d_freqs;
        HIP_TRY(d_jobs.alloc(n * sizeof(DecodeJob)));
        HIP_TRY(hipMemcpyAsync(d_jobs, jobs.data(), n * sizeof(DecodeJob), hipMemcpyHostToDevice, dev->stream));
        HIP_TRY(d_docs.alloc(padded * 4));
        if (freqs)
                HIP_TRY(d_freqs.alloc(padded * 4));
        dim3 grid(std::min<uint32_t>((maxblocks + 255) / 256, 4096), (uint32_t)n);
        TRI_LAUNCH(k_decode_terms, ix->codec, grid, dim3(256), dev->stream, ix->d_index, ix->d_blk_last, ix->d_blk_off, ix->d_terms, d_jobs, d_docs,
                           d_freqs);
        HIP_TRY(hipGetLastError());
        // blocks are full (32) except the last one of each term: the padded layout is dense per term
        for (size_t i = 0; i < n; ++i) {
                const DevTerm &t = ix->terms[terms[i]];
                if (!t.documents)
                        continue;
                HIP_TRY(hipMemcpyAsync(docs + out_offsets[i], d_docs + jobs[i].out_off, (size_t)t.documents * 4, hipMemcpyDeviceToHost, dev->stream));
                if (freqs)
                        HIP_TRY(hipMemcpyAsync(freqs + out_offsets[i], d_freqs + jobs[i].out_off, (size_t)t.documents * 4, hipMemcpyDeviceToHost, dev->stream));
        }
        HIP_TRY(hipStreamSynchronize(dev->stream));
        return TRI_OK;
}

// ---- the hits of whole lists / of (term, document) pairs (k_decode_hits.hpp)
namespace {
        int decode_hits_args(const tri_index *ix, const char *what, const uint32_t *terms, const size_t n, const uint8_t *payload_lens, const uint64_t *payloads) {
                if ((payload_lens == nullptr) != (payloads == nullptr))
                        return fail(TRI_ERR_INVALID, "%s: payload_lens and payloads are given together or not at all", what);
                if (ix->codec == TRI_CODEC_LUCENE && !ix->has_hdir)
                        return fail(TRI_ERR_INVALID, "%s: a LUCENE index uploaded without hits.data holds no positions", what);
                for (size_t i = 0; i < n; ++i)
                        if (terms[i] >= ix->terms.size())
                                return fail(TRI_ERR_INVALID, "%s: term %u out of range", what, terms[i]);
                return TRI_OK;
        }
        // the three output columns of `tot` hits on the device -> the caller's buffers
        int decode_hits_fetch(tri_dev *dev, const uint64_t tot, const uint16_t *d_pos, const uint8_t *d_len, const uint64_t *d_pay, uint16_t *positions, uint8_t *payload_lens, uint64_t *payloads) {
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipMemcpyAsync(positions, d_pos, tot * 2, hipMemcpyDeviceToHost, dev->stream));
                if (payload_lens) {
                        HIP_TRY(hipMemcpyAsync(payload_lens, d_len, tot, hipMemcpyDeviceToHost, dev->stream));
                        HIP_TRY(hipMemcpyAsync(payloads, d_pay, tot * 8, hipMemcpyDeviceToHost, dev->stream));
                }
                HIP_TRY(hipStreamSynchronize(dev->stream));
                return TRI_OK;
        }
} // namespace

extern "C" int tri_decode_hits(tri_index *ix, const uint32_t *terms, size_t n, uint16_t *positions, uint8_t *payload_lens, uint64_t *payloads, size_t cap, uint64_t *out_offsets) {
        if (!ix || (!terms && n) || !out_offsets)
                return fail(TRI_ERR_INVALID, "tri_decode_hits: null argument");
        if (const int rc = decode_hits_args(ix, "tri_decode_hits", terms, n, payload_lens, payloads))
                return rc;
        if (n > 0xffffffffull)
                return fail(TRI_ERR_INVALID, "tri_decode_hits: too many terms");
        tri_dev *dev = ix->dev;
        HIP_TRY(hipSetDevice(dev->device));
        std::vector<HitsJob> jobs(n);
        std::vector<uint64_t> totals(n + 1, 0), offs(n + 1, 0);
        uint64_t nblk = 0;
        uint32_t maxblocks = 0;
        for (size_t i = 0; i < n; ++i) {
                const DevTerm &t = ix->terms[terms[i]];
                jobs[i] = {terms[i], 0, nblk, 0};
                nblk += t.nblocks;
                maxblocks = std::max(maxblocks, t.nblocks);
        }
        const bool google = ix->codec == TRI_CODEC_GOOGLE;
        DevMem<HitsJob> d_jobs;
        DevMem<uint64_t> d_totals, d_cnt, d_pay;
        DevMem<uint16_t> d_pos;
        DevMem<uint8_t> d_len;
        const uint32_t nj = (uint32_t)n, gy = std::min<uint32_t>(nj, 32768), gx = std::min<uint32_t>((maxblocks + 255) / 256, 4096);
        if (nblk) {
                // pass 1: hits per block (GOOGLE) and per job
                HIP_TRY(d_jobs.alloc(n * sizeof(HitsJob)));
                HIP_TRY(d_totals.alloc(n * 8));
                HIP_TRY(hipMemcpyAsync(d_jobs, jobs.data(), n * sizeof(HitsJob), hipMemcpyHostToDevice, dev->stream));
                HIP_TRY(hipMemsetAsync(d_totals, 0, n * 8, dev->stream));
                if (google)
                        HIP_TRY(d_cnt.alloc(nblk * 8));
                TRI_LAUNCH(k_hits_count, ix->codec, google ? dim3(gx, gy) : dim3(1, gy), dim3(google ? 256 : 64), dev->stream, (const uint8_t *)ix->d_index, (const uint32_t *)ix->d_blk_off,
                           (const uint32_t *)ix->d_blk_hits, (const DevTerm *)ix->d_terms, (const HitsJob *)d_jobs, nj, d_cnt, d_totals);
                if (google)
                        hipLaunchKernelGGL(k_hits_scan, dim3(std::min<uint32_t>(nj, 4096)), dim3(256), 0, dev->stream, (const DevTerm *)ix->d_terms, (const HitsJob *)d_jobs, nj,
                                           d_cnt, d_totals);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipMemcpyAsync(totals.data(), d_totals, n * 8, hipMemcpyDeviceToHost, dev->stream));
                HIP_TRY(hipStreamSynchronize(dev->stream));
        }
        for (size_t i = 0; i < n; ++i) {
                jobs[i].hit_off = offs[i];
                offs[i + 1] = offs[i] + totals[i];
        }
        const uint64_t tot = offs[n];
        if (positions && tot > cap)
                return fail(TRI_ERR_INVALID, "tri_decode_hits: %llu hits, room for %zu", (unsigned long long)tot, cap);
        std::copy(offs.begin(), offs.end(), out_offsets);
        if (!positions || !tot)
                return TRI_OK;
        // pass 2: the hits
        HIP_TRY(hipMemcpyAsync(d_jobs, jobs.data(), n * sizeof(HitsJob), hipMemcpyHostToDevice, dev->stream));
        HIP_TRY(d_pos.alloc(tot * 2 + 64));
        if (payload_lens) {
                HIP_TRY(d_len.alloc(tot + 64));
                HIP_TRY(d_pay.alloc(tot * 8 + 64));
        }
        TRI_LAUNCH(k_decode_hits, ix->codec, dim3(gx, gy), dim3(256), dev->stream, (const uint8_t *)ix->d_index, (const uint8_t *)ix->d_hits, (const uint32_t *)ix->d_blk_off,
                   (const uint32_t *)ix->d_blk_hits, (const uint32_t *)ix->d_hdir, (const DevTerm *)ix->d_terms, (const HitsJob *)d_jobs, nj,
                   (const uint64_t *)d_cnt, d_pos, d_len, d_pay);
        // LUCENE: the payloads of the terms that carry some, over the zeros k_decode_hits stored (the same stream: behind it) — a wave per 128-hit block
        DevMem<LPayJob> d_pjobs;
        if (!google && payload_lens && ix->any_hit_payloads) {
                std::vector<LPayJob> pjobs;
                uint32_t maxunits = 0;
                for (size_t i = 0; i < n; ++i)
                        if ((ix->terms[terms[i]].flags & TERM_HIT_PAYLOADS) && totals[i]) {
                                pjobs.push_back({terms[i], (uint32_t)totals[i], offs[i]});
                                maxunits = std::max(maxunits, (uint32_t)((totals[i] + 127) / 128));
                        }
                if (!pjobs.empty()) {
                        HIP_TRY(d_pjobs.alloc(pjobs.size() * sizeof(LPayJob)));
                        HIP_TRY(hipMemcpyAsync(d_pjobs, pjobs.data(), pjobs.size() * sizeof(LPayJob), hipMemcpyHostToDevice, dev->stream));
                        const dim3 pgrid(std::min<uint32_t>((maxunits + 3) / 4, 4096), std::min<uint32_t>((uint32_t)pjobs.size(), 32768));
                        hipLaunchKernelGGL(k_decode_hit_payloads, pgrid, dim3(256), 0, dev->stream, (const uint8_t *)ix->d_hits, (const uint32_t *)ix->d_hdir, (const uint32_t *)ix->d_pdir,
                                           (const DevTerm *)ix->d_terms, (const LPayJob *)d_pjobs, (uint32_t)pjobs.size(), (uint8_t *)d_len, (uint64_t *)d_pay);
                        HIP_TRY(hipStreamSynchronize(dev->stream)); // (pjobs is pageable host memory the copy above reads)
                }
        }
        return decode_hits_fetch(dev, tot, d_pos, d_len, d_pay, positions, payload_lens, payloads);
}

extern "C" int tri_decode_hits_at(tri_index *ix, const uint32_t *terms, const uint32_t *docids, size_t n, uint32_t *freqs, uint16_t *positions, uint8_t *payload_lens, uint64_t *payloads,
                                  size_t cap, uint64_t *out_offsets) {
        if (!ix || ((!terms || !docids || !freqs) && n) || !out_offsets)
                return fail(TRI_ERR_INVALID, "tri_decode_hits_at: null argument");
        if (const int rc = decode_hits_args(ix, "tri_decode_hits_at", terms, n, payload_lens, payloads))
                return rc;
        if (n > 0xffffffffull)
                return fail(TRI_ERR_INVALID, "tri_decode_hits_at: too many pairs");
        if (!n) {
                out_offsets[0] = 0;
                return TRI_OK;
        }
        tri_dev *dev = ix->dev;
        HIP_TRY(hipSetDevice(dev->device));
        const uint32_t np = (uint32_t)n;
        const dim3 grid((np + 255) / 256);
        DevMem<uint32_t> d_terms, d_docs, d_freqs, d_loc;
        DevMem<uint64_t> d_off, d_pay;
        DevMem<uint16_t> d_pos;
        DevMem<uint8_t> d_len;
        HIP_TRY(d_terms.alloc(n * 4));
        HIP_TRY(d_docs.alloc(n * 4));
        HIP_TRY(d_freqs.alloc(n * 4));
        HIP_TRY(d_loc.alloc(n * 12)); // block, slot, hits of the block before the document
        HIP_TRY(hipMemcpyAsync(d_terms, terms, n * 4, hipMemcpyHostToDevice, dev->stream));
        HIP_TRY(hipMemcpyAsync(d_docs, docids, n * 4, hipMemcpyHostToDevice, dev->stream));
        uint32_t *at_block = d_loc, *at_slot = at_block + n, *at_before = at_slot + n;
        TRI_LAUNCH(k_hits_at_freq, ix->codec, grid, dim3(256), dev->stream, (const uint8_t *)ix->d_index, (const uint32_t *)ix->d_blk_last, (const uint32_t *)ix->d_blk_off,
                   (const DevTerm *)ix->d_terms, (const uint32_t *)d_terms, (const uint32_t *)d_docs, np, d_freqs, at_block, at_slot, at_before);
        HIP_TRY(hipGetLastError());
        std::vector<uint32_t> fr(n);
        HIP_TRY(hipMemcpyAsync(fr.data(), d_freqs, n * 4, hipMemcpyDeviceToHost, dev->stream));
        HIP_TRY(hipStreamSynchronize(dev->stream));
        std::vector<uint64_t> offs(n + 1, 0);
        for (size_t i = 0; i < n; ++i)
                offs[i + 1] = offs[i] + (fr[i] == DH_ABSENT ? 0u : fr[i]);
        const uint64_t tot = offs[n];
        if (positions && tot > cap)
                return fail(TRI_ERR_INVALID, "tri_decode_hits_at: %llu hits, room for %zu", (unsigned long long)tot, cap);
        std::copy(fr.begin(), fr.end(), freqs);
        std::copy(offs.begin(), offs.end(), out_offsets);
        if (!positions || !tot)
                return TRI_OK;
        HIP_TRY(d_off.alloc(n * 8));
        HIP_TRY(hipMemcpyAsync(d_off, offs.data(), n * 8, hipMemcpyHostToDevice, dev->stream));
        HIP_TRY(d_pos.alloc(tot * 2 + 64));
        if (payload_lens) {
                HIP_TRY(d_len.alloc(tot + 64));
                HIP_TRY(d_pay.alloc(tot * 8 + 64));
        }
        TRI_LAUNCH(k_hits_at_write, ix->codec, grid, dim3(256), dev->stream, (const uint8_t *)ix->d_index, (const uint8_t *)ix->d_hits, (const uint32_t *)ix->d_blk_off,
                   (const uint32_t *)ix->d_blk_hits, (const uint32_t *)ix->d_hdir, (const uint32_t *)ix->d_pdir, (const DevTerm *)ix->d_terms, (const uint32_t *)d_terms, np,
                   (const uint32_t *)d_freqs, (const uint32_t *)at_block, (const uint32_t *)at_slot, (const uint32_t *)at_before, (const uint64_t *)d_off,
                   d_pos, d_len, d_pay);
        return decode_hits_fetch(dev, tot, d_pos, d_len, d_pay, positions, payload_lens, payloads);
}

// ------------------------------------------------------------------------------------------ host: batches
// tri_batch_create = the host planner (planner.hpp: lowering, execution classes, tasks, term planes, schedule — on the device handle's
// host threads) + the plan's way to the device: ONE pinned block, ONE arena, ONE copy on the upload stream.  Everything a steady caller
// needs per batch comes from the handle's pools (arena, pinned block, output regions, events): no hipMalloc, no hipFree, no device
// synchronisation — the next batch is compiled and uploaded while the current one runs.
// ---- tri_batch_create's stages, in call order

static int create_check_args(const tri_index *ix, const uint32_t *prog, const size_t prog_len, const tri_query *queries, const size_t nq, const uint32_t flags, const uint32_t topk,
                             const int similarity, tri_batch *const *out) {
        if (!ix || !out || (!prog && prog_len) || (!queries && nq))
                return fail(TRI_ERR_INVALID, "tri_batch_create: null argument");
        const uint32_t mode = flags & (TRI_FLAG_DOCUMENTS_ONLY | TRI_FLAG_ACCUMULATED_SCORE | TRI_FLAG_MATCHED_TERMS);
        if (mode != TRI_FLAG_DOCUMENTS_ONLY && mode != TRI_FLAG_ACCUMULATED_SCORE && mode != TRI_FLAG_MATCHED_TERMS)
                return fail(TRI_ERR_INVALID, "exactly one of DocumentsOnly, AccumulatedScoreScheme, MatchedTerms (exec_query's default mode): the modes are mutually exclusive (exec.h:45-48)");
        if ((flags & TRI_FLAG_HIT_PAYLOADS) && mode != TRI_FLAG_MATCHED_TERMS)
                return fail(TRI_ERR_INVALID, "TRI_FLAG_HIT_PAYLOADS goes with TRI_FLAG_MATCHED_TERMS (the mode that delivers hits)");
        if (mode == TRI_FLAG_ACCUMULATED_SCORE && topk > TOPK_MAX)
                return fail(TRI_ERR_INVALID, "AccumulatedScoreScheme: topk <= %u (0 = keep every match's score instead of a top-K)", TOPK_MAX);
        if (similarity != TRI_SIM_BM25 && similarity != TRI_SIM_TFIDF && similarity != TRI_SIM_TRIVIAL)
                return fail(TRI_ERR_INVALID, "unknown similarity %d", similarity);
        return TRI_OK;
}
// (the modes are mutually exclusive: create_check_args)
static bool batch_scored(const tri_batch *b) { return b->flags & TRI_FLAG_ACCUMULATED_SCORE; }
static bool batch_rich(const tri_batch *b) { return b->flags & TRI_FLAG_MATCHED_TERMS; }

// plan on a free context (host; outside the handle's lock)
static int create_plan(tri_batch *b, const PlanInput &in) {
        tri_index *ix = b->ix;
        tri_dev *dev = b->dev;
        const size_t nq = in.nq;
        PlanEnv env;
        env.opt = dev->opt;
        env.cus = (uint32_t)dev->cus;
        env.fus_wgs_per_cu = FUS_WGS_PER_CU;
        env.plk_wgs_per_cu = PLK_WGS_PER_CU;
        std::string err;
        int rc;
        try {
                // a free planner context (the first one when both are busy: creates from more threads than contexts plan one after the other)
                unsigned which = 0;
                std::unique_lock<std::mutex> plan_lock(dev->planners[0].mu, std::try_to_lock);
                for (unsigned k = 1; k < tri_dev::PLAN_CTXS && !plan_lock.owns_lock(); ++k) {
                        plan_lock = std::unique_lock<std::mutex>(dev->planners[k].mu, std::try_to_lock);
                        which = k;
                }
                if (!plan_lock.owns_lock()) {
                        which = 0;
                        plan_lock = std::unique_lock<std::mutex>(dev->planners[0].mu);
                }
                tri_dev::PlanCtx &pc = dev->planners[which];
                if (nq >= 1024 && !pc.pool) { // (batches below a thousand queries are planned on the calling thread)
                        // (default: the handle's contexts share what the process may use — the affinity mask, capped by the cgroup's CPU quota — less six CPUs: the two
                        //  compiling callers, the thread that runs and awaits batches, the runtime's own threads, and slack — a process that uses its whole quota is
                        //  throttled at the first neighbour's burst: host_pool.hpp.  Under the GPU box's 16-CPU quota: 6 threads a context; measured there, 600 steps of cfg2
                        //  with the kernels at 1.18 ms, 5 / 7 threads x 2 compilers: 1.185 ms per step either way, 8 x 1: 1.39 - 1.49 (the planner is the bound), 12 x 1: 1.18;
                        //  at the round's end, kernels 1.11 ms, 100 steps, threads a context -> ms per step, a create's median / longest: 4 -> 1.29, 2.65 / 41;
                        //  5 -> 1.121, 2.0 - 2.2 / 2.6 - 39; 6 -> 1.114, 1.58 / 1.97; 7 -> 1.117, 1.59 / 1.88; 8 -> 1.127, 1.56 / 44 — six: four CPUs of the quota stay free)
                        const unsigned budget = host_cpu_budget();
                        const unsigned fair = budget >= 10 ? std::min(16u, (budget - 4) / tri_dev::PLAN_CTXS) : budget >= 4 ? 2u : 1u;
                        const unsigned want = dev->opt.plan_threads ? (unsigned)std::min<uint64_t>(dev->opt.plan_threads, 64) : fair;
                        if (want > 1) {
                                try {
                                        // (every pool of the handle counts its stretch of CPUs from the FIRST pool's anchor, not from its own creator's CPU;
                                        //  under the handle's lock: two contexts starting their pools at once agree on it)
                                        DevLock g(dev->mu);
                                        pc.pool = std::make_unique<HostPool>(want, dev->opt.plan_pin != 0, (unsigned)dev->opt.plan_hot_us, which, tri_dev::PLAN_CTXS, dev->plan_anchor, dev->opt.plan_pin == 2);
                                        if (dev->plan_anchor < 0)
                                                dev->plan_anchor = pc.pool->anchor();
                                } catch (...) { // (no threads to be had: the calling thread plans alone)
                                }
                        }
                }
                rc = plan_batch(*ix, env, in, pc.pool.get(), [&](size_t bytes) { return b->pinned.alloc(dev, bytes); }, *b, err, &pc.frag_cache);
        } catch (const std::bad_alloc &) {
                return fail(TRI_ERR_NOMEM, "tri_batch_create: out of host memory");
        }
        if (rc != TRI_OK)
                return fail(rc, "%s", err.c_str());
        if (!b->last_unsupported.empty())
                fail(TRI_ERR_UNSUPPORTED, "%s", b->last_unsupported.c_str()); // (tri_last_error() describes the last query that was left out; the call succeeds)
        return TRI_OK;
}

// The arena's layout: the block's copy, then the batch's small device-only arrays; the part that must start out zero comes last (from *zero_from).  Every
// section is named here and nowhere else: called without a base to size the arena, with the arena to point the batch's views into it
static size_t batch_arena(tri_batch *b, uint8_t *base, size_t *zero_from) {
        const size_t nt = b->tasks.size(), np = b->plan.size(), nq = b->nq, topk = b->topk;
        const bool scored = batch_scored(b), rich = batch_rich(b), scatter = b->pscatter_queries;
        Carver carve{base, b->block_bytes};
        carve(b->d_counts, (nt + 1) * 4);
        carve(b->d_ticket, TICKET_BYTES);
        carve(b->d_build, (b->plane_terms.size() + 1) * 8);
        carve(b->d_qthr, (np + 1) * 8, b->n_planes + b->n_planes8 != 0);
        carve(b->d_part_counts, (nt + 1) * 4, scored);
        carve(b->d_score_order, (nt + 1) * 4, scored);
        carve(b->d_task_hits, (nt + 1) * 4, rich);
        carve(b->d_task_pos_base, (nt + 1) * 8, rich);
        carve(b->d_scat_off, (nt + 1) * 4, scatter);
        carve(b->d_scat_cnt, (nt + 1) * 4, scatter);
        carve(b->d_scat_list, (b->pscatter_queries + 1) * 4, scatter);
        *zero_from = carve.at;
        carve(b->d_qcounts, (nq + 1) * 8); // queries that can never match keep count 0 ...
        carve(b->d_top_counts, (nq + 1) * 4, scored);
        carve(b->d_top_docs, (nq * topk + 1) * 4, scored); // ... and zeroed rows (k_topk_merge only writes the rows of queries that have a plan slot;
        carve(b->d_top_scores, (nq * topk + 1) * 4, scored); // the blocks travel whole to the host and to the other ranks)
        return carve.at;
}

// the arena, the scatter list its sections index, the batch's events, and the plan's copy on its way
static int create_arena(tri_batch *b) {
        tri_dev *dev = b->dev;
        size_t a_zero = 0;
        const size_t a = batch_arena(b, nullptr, &a_zero);
        HIP_TRY(b->d_arena.alloc(dev, a + 256));
        batch_arena(b, b->d_arena, &a_zero);
        if (b->pscatter_queries) {
                if (b->pscatter_docs + 64 > 0xffffffffull)
                        return fail(TRI_ERR_UNSUPPORTED, "tri_batch_create: the unions' terms without a plane hold more than 2^32 documents");
                b->scat_cap = (uint32_t)b->pscatter_docs;
                HIP_TRY(b->d_scat_docs.alloc(dev, ((size_t)b->scat_cap + 64) * 4));
        }
        for (PooledEvent &e : b->ev)
                HIP_TRY(e.take(dev));
        if (b->block_bytes)
                HIP_TRY(hipMemcpyAsync(b->d_arena, b->block, b->block_bytes, hipMemcpyHostToDevice, dev->stream_up));
        HIP_TRY(hipMemsetAsync(b->d_arena + a_zero, 0, a - a_zero, dev->stream_up));
        return TRI_OK;
}

// the trees' scratch block, its sections in words one after the other (tri_batch::d_tree_scratch), 64 spare words behind the last
static size_t tree_scratch(tri_batch *b, uint32_t *base) {
        const size_t plw = b->plw, nterms = b->tree_terms.size(), nhid = b->tree_hidden.size(), nchunks = (plw + TREE_CHUNK_WORDS - 1) / TREE_CHUNK_WORDS;
        Carver carve{reinterpret_cast<uint8_t *>(base), 0, 4};
        carve(b->d_tree_rows, nterms * PL_PLANES * plw * 4);
        carve(b->d_tree_prows, nhid * plw * 4);
        carve(b->d_tree_qbits, (size_t)b->n_tree * plw * 4);
        carve(b->d_tree_cc, ((size_t)b->n_tree * nchunks + 64) * 4);
        carve(b->d_tree_build, 2 * nterms * 4);
        return carve.at + 64 * 4;
}

// the large buffers (the device handle's pool): what every mode takes, then the default mode's, AccumulatedScore's, the trees'
template <class Lap>
static int create_buffers(tri_batch *b, const PlanInput &in, Lap &&lap) {
        tri_dev *dev = b->dev;
        const uint64_t off = b->out_capacity;
        const bool planes_tasks = b->n_planes + b->n_planes8 != 0, scored = batch_scored(b);
        if (!b->plane_terms.empty() || planes_tasks) {
                b->planes_hi = planes_tasks || !b->splane.empty(); // (a scored batch whose one-pass kernel or scorers read planes)
                if (const int rc = b->ix->planes.fit(dev, *b->ix, b->plane_rows, b->plw, b->planes_hi))
                        return rc;
        }
        if (planes_tasks) {
                const uint64_t wgs = std::min<uint64_t>(std::max(b->n_planes, b->n_planes8), (uint64_t)dev->cus * PLK_WGS_PER_CU);
                HIP_TRY(b->d_sparse.alloc(dev, (2 * wgs * b->sparse_cap + 64) * 4)); // (per workgroup: the lists' entries, then their frequencies)
        }
        lap(2);
        HIP_TRY(b->d_out.alloc(dev, (off + 64) * 4));
        lap(3);
        if (!b->phrases.empty() && scored) {
                HIP_TRY(b->d_pscore.alloc(dev, (off + 64) * 8)); // (no clearing: k_phrase writes the entry of every match it keeps, and only
                                                                 //  the matches of queries that hold a phrase are ever read — k_score, k_tree_leaves)
        }
        if (batch_rich(b)) {
                b->h_prog.assign(in.prog, in.prog + in.prog_len); // (tri_batch_set_ranker maps its per-token weights onto the reportable terms)
                b->h_queries.assign(in.queries, in.queries + in.nq);
                b->rich_R = std::max<uint32_t>(b->rich_R, 1);
                HIP_TRY(b->d_rich_present.alloc(dev, (off + 64) * 4));
                HIP_TRY(b->d_rich_freq.alloc(dev, (off + 64) * 2 * b->rich_R));
                if (b->rich_allow) {
                        HIP_TRY(b->d_rich_allow.alloc(dev, (off + 64) * 4));
                        HIP_TRY(hipMemsetAsync(b->d_rich_allow, 0xff, (off + 64) * 4, dev->stream_up)); // (every other query's matches: all terms allowed)
                }
                if (b->n_rich_wide) { // wide-report queries: rows and high mask halves of their own (2 x stride + 8 bytes per output slot of theirs)
                        HIP_TRY(b->d_rich_freq_wide.alloc(dev, (b->rich_wide_cells + 64) * 2));
                        HIP_TRY(b->d_rich_present_hi.alloc(dev, (b->rich_wide_slots + 64) * 4));
                        HIP_TRY(b->d_rich_allow_hi.alloc(dev, (b->rich_wide_slots + 64) * 4));
                        HIP_TRY(hipMemsetAsync(b->d_rich_allow_hi, 0xff, (b->rich_wide_slots + 64) * 4, dev->stream_up));
                }
        }
        if (scored) {
                const size_t nt = b->tasks.size(), topk = b->topk;
                if (!topk)
                        HIP_TRY(b->d_all_scores.alloc(dev, (off + 64) * 8));
                HIP_TRY(b->d_part_docs.alloc(dev, (nt * topk + 1) * 4));
                HIP_TRY(b->d_part_scores.alloc(dev, (nt * topk + 1) * 8));
        }
        if (b->n_tree) {
                const size_t nterms = b->tree_terms.size();
                HIP_TRY(b->d_tree_scratch.alloc(dev, tree_scratch(b, nullptr)));
                tree_scratch(b, b->d_tree_scratch);
                std::vector<uint32_t> build(2 * nterms);
                for (size_t i = 0; i < nterms; ++i)
                        build[2 * i] = b->tree_terms[i], build[2 * i + 1] = (uint32_t)i;
                if (nterms)
                        HIP_TRY(hipMemcpyAsync(b->d_tree_build, build.data(), build.size() * 4, hipMemcpyHostToDevice, dev->stream_up)); // (pageable source: staged before the call returns)
                if (scored && b->topk)
                        HIP_TRY(b->d_tree_scores.alloc(dev, (off + 64) * 8));
        }
        return TRI_OK;
}

static void create_info(tri_batch *b) {
        const bool scored = batch_scored(b), rich = batch_rich(b);
        const uint32_t topk = b->topk;
        b->info.nqueries = b->nq;
        b->info.tree_queries = b->tree_queries;
        b->info.bitmap_queries = b->bitmap_queries;
        b->info.tree_scratch_bytes = b->tree_scratch_bytes;
        b->info.out_capacity = b->out_capacity;
        b->info.dense_queries = b->dense_queries;
        b->info.cand_queries = b->cand_queries;
        b->info.fused_queries = b->fused_queries;
        b->info.planes_queries = b->planes_queries;
        b->info.unsupported_queries = b->unsupported_queries;
        b->info.plane_terms = b->plane_terms.size();
        b->info.plane_bytes = (uint64_t)b->plane_terms.size() * (b->planes_hi ? PL_PLANES : 1u) * b->plw * 4; // (what this batch reads of its rows of the index's plane cache: plane 0, a scored batch the high parts too)
        b->info.launches = (!b->plane_terms.empty()) + (!b->ptasks.empty()) + (rich ? 2 : 0) + (b->n_rich_wide ? 2 : 0) + ((scored && trip::sched_first(*b, TASK_FUSED)) ? 1 : 0) + ((scored && topk) ? 1 : 0);
        for (uint32_t kind = 0; kind < TASK_KINDS; ++kind) // (a launch per schedule section; the tree kernels are not counted)
                b->info.launches += kind != TASK_TREE && b->*trip::SCHED_COUNT[kind];
        b->info.create_plan_ms = (float)(b->plan_ms[0] + b->plan_ms[1] + b->plan_ms[2] + b->plan_ms[3]);
}

extern "C" int tri_batch_create(tri_index *ix, const uint32_t *prog, size_t prog_len, const tri_query *queries, size_t nq, const double *weights,
                                uint32_t flags, uint32_t topk, int similarity, tri_batch **out) {
        if (const int rc = create_check_args(ix, prog, prog_len, queries, nq, flags, topk, similarity, out))
                return rc;
        tri_dev *dev = ix->dev;
        HIP_TRY(hipSetDevice(dev->device));
        const auto t_create = std::chrono::steady_clock::now();
        static const bool dbg_create = getenv("TRINITY_DEBUG_CREATE") != nullptr; // (stderr: where a create's time goes past the planner)
        double dbg_t[4] = {0, 0, 0, 0};
        auto dbg_lap = [&](int i) {
                if (dbg_create)
                        dbg_t[i] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_create).count();
        };
        auto b = std::make_unique<tri_batch>();
        b->ix = ix;
        b->dev.retain(dev);
        b->flags = flags;
        b->topk = topk;
        b->similarity = similarity;
        b->nq = nq;
        const PlanInput in{prog, prog_len, queries, nq, weights, flags, topk, similarity};
        if (const int rc = create_plan(b.get(), in))
                return rc;
        dbg_lap(0);
        DevLock dev_lock(dev->mu); // (from here on: the device's pools, the index's plane cache, the streams — see tri_dev::mu)
        if (const int rc = create_arena(b.get()))
                return rc;
        dbg_lap(1);
        if (const int rc = create_buffers(b.get(), in, dbg_lap))
                return rc;
        HIP_TRY(hipEventRecord(b->ev[EV_UP], dev->stream_up));
        create_info(b.get());
        b->info.create_ms = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_create).count();
        if (dbg_create)
                fprintf(stderr, "[tri create] nq %zu: plan %.3f  arena+copy %.3f  planes/sparse %.3f  out(%.1f MB) %.3f  rest %.3f  total %.3f ms\n", nq, dbg_t[0], dbg_t[1] - dbg_t[0],
                        dbg_t[2] - dbg_t[1], (double)b->out_capacity * 4 / 1e6, dbg_t[3] - dbg_t[2], b->info.create_ms - dbg_t[3], b->info.create_ms);
        *out = b.release();
        return TRI_OK;
}

extern "C" void tri_batch_destroy(tri_batch *b) {
        delete b; // ~tri_batch waits, then the members release the device buffers
}

// ---- tri_batch_run's stages, in launch order: each ends with the event that closes its time (EV_PLANE_ROWS .. EV_TREE)

// what the matching kernels are handed beside the index's mask (k_filter.hpp): nothing, for a batch without filters
static FilterSel filter_sel(const tri_batch *b) {
        if (b->filter_rows.empty())
                return FilterSel{nullptr, nullptr, nullptr, 0u};
        return FilterSel{b->d_filter_rows, (const uint32_t *)b->d_filter_tab.get(), b->dev_at(b->tasks), (uint32_t)filter_words(b->ix)};
}
// A persistent matching kernel for batch b: the kernel of this file (tri_launch), or — the batch has filters — its twin of filtered_kernels.hip, which takes the
// same arguments and a FilterSel behind them
template <class F>
struct FilteredKernel;
template <class... A>
struct FilteredKernel<void (*)(A...)> {
        using type = void (*)(A..., FilterSel);
};
template <class Pick, class... Args>
static void tri_launch_matching(const tri_batch *b, const int kernel, const int variant, Pick pick, const dim3 grid, const dim3 block, const hipStream_t stream, Args &&...args) {
        const FilterSel fsel = filter_sel(b);
        if (!fsel.rows)
                return tri_launch(b->ix->codec, pick, grid, block, stream, std::forward<Args>(args)...);
        using Plain = decltype(+pick(std::integral_constant<int, CODEC_GOOGLE>()));
        const auto twin = reinterpret_cast<typename FilteredKernel<Plain>::type>(const_cast<void *>(filtered_kernel(kernel, b->ix->codec == TRI_CODEC_LUCENE ? CODEC_LUCENE : CODEC_GOOGLE, variant)));
        hipLaunchKernelGGL(twin, grid, block, 0, stream, std::forward<Args>(args)..., fsel);
}
// where the rows' source pointers lie in d_filter_tab: behind the row ids of the plan's slots
static size_t filter_tab_ptrs_off(const tri_batch *b) { return (b->plan.size() * 4 + 15) & ~(size_t)15; }

// A launch with a row per gridDim.y, cut to the limit of 65535: launch(y0, ny) enqueues rows y0 .. y0 + ny, cut after cut; the first error ends it
template <class Launch>
static int for_grid_y(const uint32_t n, Launch &&launch) {
        for (uint32_t y0 = 0; y0 < n; y0 += 65535u)
                if (const int rc = launch(y0, std::min(65535u, n - y0)))
                        return rc;
        return TRI_OK;
}

// a batch with filters: the rows its queries select from — every named filter OR-ed with the index's masked documents AS THEY STAND NOW (the set a batch
// sees is the one in place when it runs) — in one launch, before anything reads them (timed with the plane rows)
static int run_filter_rows(tri_batch *b) {
        if (b->filter_rows.empty())
                return TRI_OK;
        tri_dev *dev = b->dev;
        const size_t n4 = filter_words(b->ix) / 4;
        const uint32_t nrows = (uint32_t)b->filter_rows.size();
        return for_grid_y(nrows, [&](const uint32_t y0, const uint32_t ny) -> int {
                hipLaunchKernelGGL(k_filter_rows, dim3((unsigned)std::min<size_t>((n4 + FILTER_WG - 1) / FILTER_WG, 1024), ny), dim3(FILTER_WG), 0, dev->stream,
                                   (const uint4 *const *)(b->d_filter_tab + filter_tab_ptrs_off(b)) + y0, (const uint4 *)b->ix->d_masked.get(), (uint4 *)b->d_filter_rows.get() + (size_t)y0 * n4, n4);
                HIP_TRY(hipGetLastError());
                return TRI_OK;
        });
}

// the head terms the batch's queries share: the rows of the index's plane cache that no earlier run has built are decoded now — once for the
// index, not once per batch (every word of a row is written: no memset)
static int run_plane_rows(tri_batch *b) {
        tri_dev *dev = b->dev;
        tri_index *ix = b->ix;
        PlaneCache &pc = ix->planes;
        const std::vector<uint32_t> build = pc.missing_rows(*ix, b->plane_terms.data(), b->plane_terms.size(), b->planes_hi, dev->opt.planes_rebuild, b->info.term_planes_decoded_bytes);
        if (!build.empty()) {
                HIP_TRY(hipMemcpyAsync(b->d_build, build.data(), build.size() * 4, hipMemcpyHostToDevice, dev->stream)); // (pageable source: staged before the call returns)
                const uint32_t nwin = b->plw / PL_WORDS;
                const int rc = for_grid_y((uint32_t)(build.size() / 2), [&](const uint32_t y0, const uint32_t ny) -> int {
                        if (b->planes_hi) // (a row that gains its high part is decoded whole again: plane 0 is rewritten with the words it holds)
                                TRI_LAUNCH(k_term_planes, ix->codec, dim3(nwin, ny), dim3(AND_WG), dev->stream, ix->d_index, ix->d_blk_last, ix->d_blk_off, ix->d_blk_rec,
                                           ix->d_blk_doff, ix->d_win, ix->d_terms, (const uint32_t *)b->d_build + 2 * (size_t)y0, pc.plane0(), (size_t)b->plw, pc.high(),
                                           (size_t)PL_HI * b->plw, b->plw, (uint32_t *)nullptr);
                        else // plane 0 alone, P0_GROUP windows to a workgroup (the rank records: built when a phrase batch asks for them, run_phrases)
                                TRI_LAUNCH(k_term_plane0, ix->codec, dim3((nwin + P0_GROUP - 1) / P0_GROUP, ny), dim3(AND_WG), dev->stream, ix->d_index, ix->d_blk_last, ix->d_blk_off,
                                           ix->d_blk_rec, ix->d_blk_doff, ix->d_win, ix->d_terms, (const uint32_t *)b->d_build + 2 * (size_t)y0, pc.plane0(), b->plw, (uint32_t *)nullptr);
                        HIP_TRY(hipGetLastError());
                        return TRI_OK;
                });
                if (rc)
                        return rc;
                pc.mark_built(build, b->planes_hi);
        }
        HIP_TRY(hipEventRecord(b->ev[EV_PLANE_ROWS], dev->stream));
        return TRI_OK;
}

// the docset-materialising kernels: the window kernels (k_and_dense, k_psets, k_probe), then the candidate tiles (k_and) — persistent kernels back
// to back on the engine stream, or k_and on the second stream beside the others (options overlap, overlap_dense_wgs / overlap_cand_wgs)
static int run_matching(tri_batch *b) {
        tri_dev *dev = b->dev;
        tri_index *ix = b->ix;
        // GOOGLE: matching reads the contiguous delta streams, not the chunks (see tri_index::d_dstream)
        const uint8_t *match_bytes = ix->codec == TRI_CODEC_GOOGLE ? ix->d_dstream : ix->d_index;
        const uint32_t *match_off = ix->codec == TRI_CODEC_GOOGLE ? ix->d_blk_doff : ix->d_blk_off;
        uint32_t dense_wgs = TRI_DENSE_WAVES * 256 / DENSE_WG, cand_wgs = 4; // workgroups per CU
        bool overlap = false;
        if (dev->opt.overlap_dense_wgs && dev->opt.overlap_cand_wgs && (b->n_dense || b->n_pset) && b->n_cand) { // the window kernels and the candidate-tile kernel side by side
                overlap = true;
                dense_wgs = (uint32_t)dev->opt.overlap_dense_wgs;
                cand_wgs = (uint32_t)dev->opt.overlap_cand_wgs;
        } else if (dev->opt.overlap && b->n_cand && trip::sched_first(*b, TASK_CAND)) // (any window kernel's tasks)
                overlap = true; // (full grids: the second kernel's workgroups take the slots the first one's tail leaves)
        hipStream_t cand_stream = dev->stream;
        if (overlap) {
                HIP_TRY(hipEventRecord(dev->ev_fork, dev->stream));
                HIP_TRY(hipStreamWaitEvent(dev->stream2, dev->ev_fork, 0));
                cand_stream = dev->stream2;
        }
        const DevPsetUnit *units = b->dev_at(b->units);
        const uint32_t *pset_sched = b->dev_at(b->pset_sched);
        const FilterSel fsel = filter_sel(b);
        // unions with terms that have no plane (PSET_UNIT_SCATTER): those terms' documents listed task by task, a workgroup per query (units[] holds the TASK_PROBE units
        // too) — on the second stream, beside k_and_dense, where that stream is not k_and's (option overlap)
        const bool prep = b->n_pset && b->pscatter_queries, prep_forked = prep && !overlap && b->n_dense;
        if (prep) {
                if (prep_forked) {
                        HIP_TRY(hipEventRecord(dev->ev_fork, dev->stream));
                        HIP_TRY(hipStreamWaitEvent(dev->stream2, dev->ev_fork, 0));
                }
                hipStream_t prep_stream = prep_forked ? dev->stream2 : dev->stream;
                const uint32_t nunits = b->n_pset + b->n_probe, nscat = (uint32_t)b->pscatter_queries;
                hipLaunchKernelGGL(k_psets_prep_list, dim3((nunits + 255) / 256), dim3(256), 0, prep_stream, units, nunits, b->d_ticket + TICKET_SCAT_WORD + 1, b->d_scat_list, nscat);
                HIP_TRY(hipGetLastError());
                TRI_LAUNCH(k_psets_prep, ix->codec, dim3(nscat), dim3(PSCAT_WG), prep_stream, units, (const uint32_t *)b->d_scat_list, (const uint32_t *)(b->d_ticket + TICKET_SCAT_WORD + 1),
                           b->dev_at(b->plan), b->dev_at(b->tasks), (const uint32_t *)b->dev_at(b->qterms), (const uint32_t *)b->dev_opt(b->qplane), ix->d_masked, ix->d_index, ix->d_blk_last, ix->d_blk_off, ix->d_blk_rec,
                           ix->d_blk_doff, ix->d_terms, b->d_ticket + TICKET_SCAT_WORD, b->d_scat_off, b->d_scat_cnt, b->d_scat_docs, b->scat_cap, fsel);
                HIP_TRY(hipGetLastError());
                if (prep_forked)
                        HIP_TRY(hipEventRecord(dev->ev_join, dev->stream2));
        }
        if (b->n_dense) {
                tri_launch_matching(b, FK_AND_DENSE, 0, [](auto c) { return k_and_dense<c.value>; }, dim3(std::min<uint32_t>(b->n_dense, (uint32_t)dev->cus * dense_wgs)), dim3(DENSE_WG), dev->stream, match_bytes, ix->d_blk_last,
                           match_off, ix->d_win, ix->d_terms, b->dev_at(b->plan), b->dev_at(b->tasks), b->dev_at(b->sched) + trip::sched_first(*b, TASK_DENSE), b->dev_at(b->qterms), b->n_dense,
                           b->d_ticket + TICKET_DENSE_WORD, b->d_out, b->d_counts, ix->d_masked, (const uint32_t *)b->dev_opt(b->qplane), (const uint32_t *)ix->planes.plane0(), b->plw);
                HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(b->ev[EV_DENSE], dev->stream));
        if (prep_forked) // (k_psets reads the lists k_psets_prep made beside k_and_dense)
                HIP_TRY(hipStreamWaitEvent(dev->stream, dev->ev_join, 0));
        if (b->n_pset) {
                // the queries all of whose terms have planes: word-wise algebra over the planes + expansion (k_psets.hpp)
                const uint32_t pset_wgs = TRI_PSET_WAVES * 256 / PSET_WG;
                tri_launch_matching(b, FK_PSETS, 0, [](auto c) { return k_psets<c.value>; }, dim3(std::min<uint32_t>(b->n_pset, (uint32_t)dev->cus * (overlap && dev->opt.overlap_dense_wgs ? std::min<uint32_t>(dense_wgs, pset_wgs) : pset_wgs))),
                           dim3(PSET_WG), dev->stream, units, pset_sched, b->n_pset, b->d_ticket + TICKET_PSET_WORD, (const uint32_t *)b->dev_at(b->qterms), (const uint32_t *)b->dev_opt(b->qplane), b->d_out,
                           b->d_counts, ix->d_masked, (const uint32_t *)ix->planes.plane0(), b->plw, (const uint32_t *)b->d_scat_off, (const uint32_t *)b->d_scat_cnt,
                           (const uint32_t *)b->d_scat_docs);
                HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(b->ev[EV_PSET], dev->stream));
        if (b->n_probe) {
                // one short lead list against lists that all have planes: a wave per task, the lead's documents probed from registers (k_probe.hpp);
                // its units run behind k_psets' in pset_sched[]
                tri_launch_matching(b, FK_PROBE, 0, [](auto c) { return k_probe<c.value>; }, dim3(std::min<uint32_t>((b->n_probe + PROBE_WG / 64 - 1) / (PROBE_WG / 64), (uint32_t)dev->cus * (TRI_PROBE_WAVES * 256 / PROBE_WG))),
                           dim3(PROBE_WG), dev->stream, match_bytes, ix->d_blk_last, match_off, ix->d_terms, units, pset_sched + b->n_pset, b->n_probe, b->d_ticket + TICKET_PROBE_WORD,
                           (const uint32_t *)b->dev_at(b->qterms), (const uint32_t *)b->dev_opt(b->qplane), b->d_out, b->d_counts, ix->d_masked, (const uint32_t *)ix->planes.plane0(), b->plw);
                HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(b->ev[EV_PROBE], dev->stream));
        if (b->n_cand)
                tri_launch_matching(b, FK_AND, 0, [](auto c) { return k_and<c.value>; }, dim3(std::min<uint32_t>(b->n_cand, (uint32_t)dev->cus * cand_wgs)), dim3(AND_WG), cand_stream, match_bytes, ix->d_blk_last, match_off,
                           ix->d_win, ix->d_terms, b->dev_at(b->plan), b->dev_at(b->tasks), b->dev_at(b->sched) + trip::sched_first(*b, TASK_CAND), b->dev_at(b->qterms), b->dev_at(b->cand_q),
                           b->d_ticket + TICKET_CAND_WORD, b->d_out, b->d_counts, ix->d_masked, (const uint32_t *)b->dev_opt(b->qplane), (const uint32_t *)ix->planes.plane0(), b->plw);
        HIP_TRY(hipGetLastError());
        if (overlap) {
                HIP_TRY(hipEventRecord(dev->ev_join, dev->stream2));
                HIP_TRY(hipStreamWaitEvent(dev->stream, dev->ev_join, 0));
        }
        HIP_TRY(hipEventRecord(b->ev[EV_CAND], dev->stream));
        return TRI_OK;
}

// AccumulatedScore top-K of the dense queries: decode -> match -> score -> select in one pass; as many workgroups per CU as its LDS holds.
// Three instantiations: 32-bit window words, 16-bit ones (queries of <= 5 distinct terms: windows twice as long), general trees (32-bit words)
static int run_fused(tri_batch *b) {
        tri_dev *dev = b->dev;
        tri_index *ix = b->ix;
        for (uint32_t kind = TASK_FUSED; kind <= TASK_FUSED_GEN; ++kind) {
                const uint32_t nf = b->*trip::SCHED_COUNT[kind], variant = kind - TASK_FUSED;
                if (!nf)
                        continue;
                tri_launch_matching(b, FK_FUSED, (int)variant, [&](auto c) { return std::array{k_fused<c.value, 0, 0>, k_fused<c.value, 1, 0>, k_fused<c.value, 0, 1>}[variant]; },
                           dim3(std::min<uint32_t>(nf, (uint32_t)dev->cus * FUS_WGS_PER_CU)), dim3(FUS_WG), dev->stream, ix->d_index, ix->d_blk_last, ix->d_blk_off, ix->d_blk_rec,
                           ix->d_blk_doff, ix->d_win, ix->d_terms, b->dev_at(b->plan), b->dev_at(b->fused), b->dev_at(b->tasks), (const uint32_t *)b->dev_at(b->sched) + trip::sched_first(*b, kind), b->dev_at(b->sterms),
                           b->dev_at(b->sweights), nf, b->d_ticket + TICKET_FUSED_WORD + 2 * variant, b->d_counts, b->topk, b->d_part_docs, b->d_part_scores, b->d_part_counts, ix->d_masked,
                           b->similarity, b->d_out, b->d_all_scores, b->d_rich_allow);
                HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(b->ev[EV_FUSED], dev->stream));
        return TRI_OK;
}

// AccumulatedScore top-K of the CNF queries over bit planes: the head terms' planes from k_term_planes, the other lists decoded per window into
// LDS planes; union / conjunction predicates and the candidate filter 32 documents per word (two instantiations: queries of up to five slots,
// wider ones)
static int run_planes(tri_batch *b) {
        tri_dev *dev = b->dev;
        tri_index *ix = b->ix;
        if (b->d_qthr)
                HIP_TRY(hipMemsetAsync(b->d_qthr, 0, (b->plan.size() + 1) * 8, dev->stream));
        for (uint32_t kind = TASK_PLANES; kind <= TASK_PLANES8; ++kind) {
                const uint32_t np = b->*trip::SCHED_COUNT[kind], wide = kind - TASK_PLANES;
                if (!np)
                        continue;
                tri_launch_matching(b, FK_PLANES, (int)wide, [&](auto c) { return wide ? k_planes<c.value, FUS_MAX_SLOTS> : k_planes<c.value, PLK_NS_SMALL>; },
                           dim3(std::min<uint32_t>(np, (uint32_t)dev->cus * PLK_WGS_PER_CU)), dim3(PLK_WG), dev->stream, ix->d_index, ix->d_blk_last, ix->d_blk_off, ix->d_blk_rec,
                           ix->d_blk_doff, ix->d_win, ix->d_terms, b->dev_at(b->plan), b->dev_at(b->fused), b->dev_at(b->tasks), (const uint32_t *)b->dev_at(b->sched) + trip::sched_first(*b, kind), b->dev_at(b->sterms),
                           b->dev_at(b->sweights), np, b->d_ticket + TICKET_PLANES_WORD + 2 * wide, b->d_counts, b->topk, b->d_part_docs, b->d_part_scores, b->d_part_counts, ix->d_masked,
                           b->similarity, (const uint32_t *)ix->planes.plane0(), (const uint32_t *)ix->planes.high(), b->plw, ix->planes.cap(), b->d_sparse, b->sparse_cap, b->d_qthr);
                HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(b->ev[EV_PLANES], dev->stream));
        return TRI_OK;
}

// positional constraints: filter + compact the match segments of the queries that hold phrases
static int run_phrases(tri_batch *b) {
        tri_dev *dev = b->dev;
        tri_index *ix = b->ix;
        PlaneCache &pc = ix->planes;
        if (!b->ptasks.empty() && ix->codec == TRI_CODEC_GOOGLE) {
                // the phrases' head terms are located by RANK in plane 0 (k_phrase.hpp): rows (plane 0 + rank directory) and per-posting hits entries of the
                // phrase terms that have none yet are built now — once for the index
                PhraseRows pr;
                const uint32_t *d_pairs = nullptr;
                if (const int rc = pc.phrase_rows(*ix, b->pterms.data(), b->pterms.size(), dev->stream, pr, &d_pairs))
                        return rc;
                // plane 0 + rank records in ONE launch over the list (a grid per row was 711 launches, 11 ms, the first time cfg4's phrases met an index)
                const uint32_t npairs = (uint32_t)(pr.pairs.size() / 2);
                int rc = for_grid_y(npairs, [&](const uint32_t y0, const uint32_t ny) -> int {
                        const dim3 grid((b->plw / PL_WORDS + P0_GROUP - 1) / P0_GROUP, ny);
                        TRI_LAUNCH(k_term_plane0, ix->codec, grid, dim3(AND_WG), dev->stream, ix->d_index, ix->d_blk_last, ix->d_blk_off, ix->d_blk_rec, ix->d_blk_doff, ix->d_win,
                                   ix->d_terms, d_pairs + 2 * (size_t)y0, pc.plane0(), b->plw, pc.rank());
                        HIP_TRY(hipGetLastError());
                        return TRI_OK;
                });
                if (rc)
                        return rc;
                // (a small index at a high plane_div makes almost every term eligible)
                rc = for_grid_y(npairs, [&](const uint32_t y0, const uint32_t ny) -> int {
                        hipLaunchKernelGGL(k_term_hits, dim3((pr.max_blocks + 255) / 256, ny), dim3(256), 0, dev->stream, ix->d_index, ix->d_blk_off, ix->d_blk_hits, ix->d_terms,
                                           d_pairs + 2 * (size_t)y0, (const uint64_t *)pc.hits_off(), pc.hits(), pc.term_row());
                        HIP_TRY(hipGetLastError());
                        return TRI_OK;
                });
                if (rc)
                        return rc;
        }
        if (!b->ptasks.empty()) {
                const uint32_t np = (uint32_t)b->ptasks.size();
                TRI_LAUNCH(k_phrase, ix->codec, dim3(std::min<uint32_t>(np, (uint32_t)dev->cus * PHRASE_WGS_PER_CU)), dim3(AND_WG), dev->stream, ix->d_index, ix->d_hits,
                           ix->d_blk_hits, ix->d_hdir, ix->d_blk_last, ix->d_blk_off, ix->d_win, ix->d_terms, b->dev_at(b->plan), b->dev_at(b->tasks), b->dev_at(b->ptasks), np, b->dev_at(b->phrases), b->dev_at(b->pterms),
                           b->d_ticket + TICKET_PHRASE_WORD, b->d_out, b->d_counts, b->d_pscore,
                           (b->flags & TRI_FLAG_ACCUMULATED_SCORE) ? 65535u : 1u, // exec.cpp:296 trackCnt
                           b->similarity, (const uint32_t *)pc.plane0(), pc.plw(), (const uint32_t *)pc.rank(), (const unsigned long long *)pc.hits(),
                           (const uint64_t *)pc.hits_off(), ix->codec == TRI_CODEC_GOOGLE ? (const uint32_t *)pc.term_row() : nullptr);
                HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(b->ev[EV_PHRASE], dev->stream));
        return TRI_OK;
}

// the queries no other kernel takes (k_tree.hpp): leaf bitmaps — the distinct term leaves decoded once, the phrase leaves from their hidden
// queries' match lists (k_phrase has just filtered them) —, the trees word by word, the match bitmaps expanded
static int run_trees(tri_batch *b) {
        tri_dev *dev = b->dev;
        tri_index *ix = b->ix;
        if (b->n_tree) {
                const uint32_t plw = b->plw, nterms = (uint32_t)b->tree_terms.size(), nhid = (uint32_t)b->tree_hidden.size();
                const uint32_t nchunks = (plw + TREE_CHUNK_WORDS - 1) / TREE_CHUNK_WORDS;
                const uint32_t *tsched = b->dev_at(b->sched) + trip::sched_first(*b, TASK_TREE);
                const uint32_t *d_tree = b->dev_at(b->tree);
                int rc = for_grid_y(nterms, [&](const uint32_t y0, const uint32_t ny) -> int {
                        TRI_LAUNCH(k_term_planes, ix->codec, dim3(plw / PL_WORDS, ny), dim3(AND_WG), dev->stream, ix->d_index, ix->d_blk_last, ix->d_blk_off, ix->d_blk_rec, ix->d_blk_doff, ix->d_win,
                                   ix->d_terms, (const uint32_t *)b->d_tree_build + 2 * (size_t)y0, b->d_tree_rows, (size_t)PL_PLANES * plw, b->d_tree_rows + plw,
                                   (size_t)PL_PLANES * plw, plw, (uint32_t *)nullptr); // (a tree row keeps its two parts side by side: plane k at k * plw)
                        HIP_TRY(hipGetLastError());
                        return TRI_OK;
                });
                if (rc)
                        return rc;
                if (nhid) {
                        HIP_TRY(hipMemsetAsync(b->d_tree_prows, 0, (size_t)nhid * plw * 4, dev->stream));
                        hipLaunchKernelGGL(k_tree_gather, dim3(nhid), dim3(TREE_WG), 0, dev->stream, b->dev_at(b->plan), b->dev_at(b->tasks), b->dev_at(b->tree_hidden), b->d_out,
                                           b->d_counts, b->d_pscore, b->d_tree_prows, plw);
                        HIP_TRY(hipGetLastError());
                }
                const bool scored_run = b->flags & TRI_FLAG_ACCUMULATED_SCORE, rich_run = b->flags & TRI_FLAG_MATCHED_TERMS;
                double *tscores = !scored_run ? nullptr : b->topk ? (double *)b->d_tree_scores : (double *)b->d_all_scores;
                // the section's narrow records first (k_tree.hpp), then its wide ones (k_tree_wide.hpp: split_tree_section put them last); k_tree_expand reads no record
                const uint32_t n_narrow = b->n_tree - b->n_tree_wide;
                const auto eval = [&](const bool wide, const uint32_t y0, const uint32_t ny) -> int {
                        const dim3 grid(nchunks, ny);
                        uint32_t *qbits = b->d_tree_qbits + (size_t)y0 * plw, *cc = b->d_tree_cc + (size_t)y0 * nchunks;
#define TREE_EVAL_ARGS b->dev_at(b->plan), b->dev_at(b->tasks), tsched + y0, d_tree, (const uint32_t *)b->d_tree_rows, (const uint32_t *)b->d_tree_prows, (const uint32_t *)ix->d_masked, qbits, cc, plw, filter_sel(b)
                        if (wide)
                                hipLaunchKernelGGL(k_tree_eval_wide, grid, dim3(TREE_WG), 0, dev->stream, TREE_EVAL_ARGS);
                        else
                                hipLaunchKernelGGL(k_tree_eval, grid, dim3(TREE_WG), 0, dev->stream, TREE_EVAL_ARGS);
#undef TREE_EVAL_ARGS
                        hipLaunchKernelGGL(k_tree_expand, grid, dim3(TREE_WG), 0, dev->stream, b->dev_at(b->plan), b->dev_at(b->tasks), tsched + y0, (const uint32_t *)qbits, (const uint32_t *)cc,
                                           b->d_out, b->d_counts, plw);
                        if (scored_run || rich_run) {
#define TREE_LEAVES_ARGS                                                                                                                                                                   \
        ix->d_index, ix->d_blk_last, ix->d_blk_off, ix->d_terms, b->dev_at(b->plan), b->dev_at(b->tasks), tsched + y0, d_tree, (const uint32_t *)b->d_tree_rows,                          \
                (const uint32_t *)b->d_tree_prows, (const uint32_t *)cc, (const uint32_t *)b->d_out, (const uint32_t *)b->d_counts, (const double *)b->dev_at(b->sweights),               \
                (const double *)b->d_pscore, tscores, rich_run ? (uint32_t *)b->d_rich_allow : nullptr, plw, b->similarity, b->d_rich_allow_hi,                                                     \
                (const DevRichWide *)b->dev_opt(b->rich_wide)
                                if (wide)
                                        TRI_LAUNCH(k_tree_leaves_wide, ix->codec, grid, dim3(TREE_WG), dev->stream, TREE_LEAVES_ARGS);
                                else
                                        TRI_LAUNCH(k_tree_leaves, ix->codec, grid, dim3(TREE_WG), dev->stream, TREE_LEAVES_ARGS);
#undef TREE_LEAVES_ARGS
                        }
                        HIP_TRY(hipGetLastError());
                        return TRI_OK;
                };
                if ((rc = for_grid_y(n_narrow, [&](const uint32_t y0, const uint32_t ny) { return eval(false, y0, ny); })))
                        return rc;
                if ((rc = for_grid_y(b->n_tree_wide, [&](const uint32_t y0, const uint32_t ny) { return eval(true, n_narrow + y0, ny); })))
                        return rc;
                if (scored_run && b->topk) {
                        hipLaunchKernelGGL(k_tree_topk, dim3(b->n_tree), dim3(AND_WG), 0, dev->stream, tsched, b->dev_at(b->tasks), (const uint32_t *)b->d_out, (const uint32_t *)b->d_counts,
                                           (const double *)tscores, b->topk, b->d_part_docs, b->d_part_scores, b->d_part_counts);
                        HIP_TRY(hipGetLastError());
                }
        }
        HIP_TRY(hipEventRecord(b->ev[EV_TREE], dev->stream));
        return TRI_OK;
}

// TRI_FLAG_MATCHED_TERMS, over every task: the COUNT pass (which reportable terms hold each match, with what frequency; hit totals per task) or
// the WRITE pass (the positions, into the pool at the offsets tri_batch_sync made of the totals)
template <bool WRITE>
static int launch_rich(tri_batch *b) {
        tri_dev *dev = b->dev;
        tri_index *ix = b->ix;
        // a batch with wide-report queries runs off its own schedule (BatchPlan::rich_sched): every other task first — the launch below, what it always
        // covered —, the wide-report queries' tasks last: a second launch, of k_rich_wide, with a ticket word of its own
        const uint32_t n_wide = b->n_rich_wide, n = (uint32_t)b->tasks.size() - n_wide;
        const uint32_t *sched = n_wide ? b->dev_at(b->rich_sched) : b->dev_at(b->sched);
        const RichWideArgs wd{b->d_rich_present_hi, b->d_rich_allow_hi, b->d_rich_freq_wide, b->dev_opt(b->rich_wide)};
#define RICH_ARGS(SCHED, N, TICKET)                                                                                                                                                        \
        ix->d_index, ix->d_hits, ix->d_blk_hits, ix->d_hdir, ix->d_pdir, ix->d_blk_last, ix->d_blk_off, ix->d_terms, b->dev_at(b->plan), b->dev_at(b->tasks), SCHED, b->dev_at(b->sterms), N,         \
                b->d_ticket + (WRITE ? TICKET_RICH_WRITE_WORD : TICKET_RICH_COUNT_WORD) + TICKET, b->d_out, b->d_counts, b->rich_R, b->d_rich_present, b->d_rich_freq, b->d_task_hits,     \
                WRITE ? (const uint64_t *)b->d_task_pos_base : nullptr, WRITE ? (uint16_t *)b->d_rich_pool : nullptr, (const uint32_t *)b->d_rich_allow, WRITE ? (uint8_t *)b->d_rich_plen : nullptr,             \
                WRITE ? (uint64_t *)b->d_rich_payload : nullptr
        if (n)
                tri_launch(ix->codec, [](auto c) { return k_rich<c.value, WRITE>; }, dim3(std::min<uint32_t>(n, (uint32_t)dev->cus * 3)), dim3(AND_WG), dev->stream, RICH_ARGS(sched, n, 0));
        if (n_wide)
                tri_launch(ix->codec, [](auto c) { return k_rich_wide<c.value, WRITE>; }, dim3(std::min<uint32_t>(n_wide, (uint32_t)dev->cus * 3)), dim3(AND_WG), dev->stream,
                           RICH_ARGS(sched + n, n_wide, TICKET_RICH_WIDE), wd);
#undef RICH_ARGS
        HIP_TRY(hipGetLastError());
        return TRI_OK;
}

static int run_rich_count(tri_batch *b) {
        if (!(b->flags & TRI_FLAG_MATCHED_TERMS))
                return TRI_OK;
        tri_dev *dev = b->dev;
        HIP_TRY(hipMemsetAsync(b->d_rich_present, 0, (b->out_capacity + 64) * 4, dev->stream));
        HIP_TRY(hipMemsetAsync(b->d_rich_freq, 0, (b->out_capacity + 64) * 2 * b->rich_R, dev->stream));
        HIP_TRY(hipMemsetAsync(b->d_task_hits, 0, (b->tasks.size() + 1) * 4, dev->stream));
        if (b->n_rich_wide) { // (the wide-report queries' rows and high mask halves: cleared per run like the narrow ones)
                HIP_TRY(hipMemsetAsync(b->d_rich_present_hi, 0, (b->rich_wide_slots + 64) * 4, dev->stream));
                HIP_TRY(hipMemsetAsync(b->d_rich_freq_wide, 0, (b->rich_wide_cells + 64) * 2, dev->stream));
        }
        return launch_rich<false>(b);
}

// AccumulatedScore: the sets k_and_dense / k_psets / k_probe / k_and materialised — the schedule's sections before the one-pass kinds', which
// have scored themselves — scored heaviest first; then the queries' top-K merged from their tasks'
static int run_scores(tri_batch *b) {
        if (!(b->flags & TRI_FLAG_ACCUMULATED_SCORE))
                return TRI_OK;
        tri_dev *dev = b->dev;
        tri_index *ix = b->ix;
        const uint32_t nlegacy = trip::sched_first(*b, TASK_FUSED);
        if (nlegacy) {
                hipLaunchKernelGGL(k_score_order, dim3(1), dim3(SORD_WG), 0, dev->stream, (const uint32_t *)b->dev_at(b->sched), (const uint32_t *)b->d_counts, nlegacy, b->d_score_order);
                HIP_TRY(hipGetLastError());
                TRI_LAUNCH(k_score, ix->codec, dim3(std::min<uint32_t>(nlegacy, (uint32_t)dev->cus * SCORE_WGS_PER_CU)), dim3(AND_WG), dev->stream, ix->d_index, ix->d_blk_last,
                           ix->d_blk_off, ix->d_terms, b->dev_at(b->plan), b->dev_at(b->tasks), (const uint32_t *)b->d_score_order, b->dev_at(b->sterms), b->dev_at(b->sweights), nlegacy,
                           b->d_ticket + TICKET_SCORE_WORD, b->d_out, b->d_counts, b->topk, b->d_part_docs, b->d_part_scores, b->d_part_counts, b->d_all_scores, b->d_pscore,
                           b->similarity, ix->d_win, b->dev_opt(b->splane),
                           (const uint32_t *)ix->planes.high(), b->plw); // (the scorers read the level words: the rows' high parts)
        }
        HIP_TRY(hipGetLastError());
        const uint32_t nqs = (uint32_t)b->plan.size();
        if (b->topk)
                hipLaunchKernelGGL(k_topk_merge, dim3(std::min<uint32_t>(nqs, (uint32_t)dev->cus * 8)), dim3(AND_WG), 0, dev->stream, b->dev_at(b->plan), nqs, b->topk, b->d_part_docs,
                                   b->d_part_scores, b->d_part_counts, b->d_top_docs, b->d_top_scores, b->d_top_counts);
        HIP_TRY(hipGetLastError());
        return TRI_OK;
}

// per caller query: the matches of its tasks
static int run_query_counts(tri_batch *b) {
        if (!b->plan.empty()) {
                const uint32_t nqs = (uint32_t)b->plan.size();
                hipLaunchKernelGGL(k_query_counts, dim3((nqs + 255) / 256), dim3(256), 0, b->dev->stream, b->dev_at(b->plan), b->d_counts, nqs, b->d_qcounts);
                HIP_TRY(hipGetLastError());
        }
        return TRI_OK;
}

// the consumers of the finished docID sets — tri_batch_set_facets / _order / _stats, their columns, run_consumers, sync_consumers, consumer_ready
#include "consumers.hpp"

extern "C" int tri_batch_run(tri_batch *b) {
        if (!b)
                return fail(TRI_ERR_INVALID, "null batch");
        tri_dev *dev = b->dev;
        DevLock dev_lock(dev->mu);
        HIP_TRY(hipSetDevice(dev->device));
        b->synced = false;
        b->rank_done = false;
#ifdef TRI_TRACE
        if (!g_trace_host) {
                HIP_TRY(hipHostMalloc((void **)&g_trace_host, 64 * 16, hipHostMallocMapped | hipHostMallocCoherent));
                uint32_t *dptr = nullptr;
                HIP_TRY(hipHostGetDevicePointer((void **)&dptr, g_trace_host, 0));
                HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_trace), &dptr, sizeof dptr));
        }
        memset(g_trace_host, 0, 64 * 16);
#endif
        b->ran = true;
#ifdef TRI_TASKTIMES
        if (b->tasks.size()) {
                if (g_tt_cap < 8 * (size_t)b->tasks.size()) {
                        if (g_tt_host)
                                hipHostFree(g_tt_host);
                        g_tt_cap = 8 * (size_t)b->tasks.size() + 1024;
                        HIP_TRY(hipHostMalloc((void **)&g_tt_host, g_tt_cap * 8, hipHostMallocMapped | hipHostMallocCoherent));
                        unsigned long long *dptr = nullptr;
                        HIP_TRY(hipHostGetDevicePointer((void **)&dptr, g_tt_host, 0));
                        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_tt), &dptr, sizeof dptr));
                }
                memset(g_tt_host, 0, g_tt_cap * 8);
        }
#endif
        HIP_TRY(hipStreamWaitEvent(dev->stream, b->ev[EV_UP], 0)); // the plan's copy (upload stream) has arrived
        if (b->ix->planes.ready())
                HIP_TRY(hipStreamWaitEvent(dev->stream, b->ix->planes.ready(), 0)); // ... and so have the plane cache's rows, should it have been grown since
        HIP_TRY(hipEventRecord(b->ev[EV_START], dev->stream));
        if (b->tasks.empty()) {
                for (int e = EV_PLANE_ROWS; e <= EV_TREE; ++e)
                        HIP_TRY(hipEventRecord(b->ev[e], dev->stream));
        } else {
                HIP_TRY(hipMemsetAsync(b->d_ticket, 0, TICKET_BYTES, dev->stream)); // (timed with the plane rows)
                for (int (*stage)(tri_batch *) : {run_filter_rows, run_plane_rows, run_matching, run_fused, run_planes, run_phrases, run_trees, run_rich_count, run_scores})
                        if (const int rc = stage(b))
                                return rc;
        }
        if (const int rc = run_query_counts(b))
                return rc;
        if (const int rc = run_consumers(b))
                return rc;
        HIP_TRY(hipEventRecord(b->ev[EV_END], dev->stream));
        return TRI_OK;
}

#ifdef TRI_TASKTIMES
// -DTRI_TASKTIMES[=n] probe builds, with TRINITY_TASKTIMES set: the start and end stamps of one kernel's tasks, summarised on stderr
static void report_tasktimes(tri_batch *b) {
        const tri_dev *dev = b->dev;
        if (!b->tasks.size() || !getenv("TRINITY_TASKTIMES"))
                return;
#if TRI_TASKTIMES == 2 // (k_score: tickets run over the docset-materialising tasks, sched[0 ..))
        const uint32_t nc = trip::sched_first(*b, TASK_FUSED), first = 0;
#elif TRI_TASKTIMES == 5 // (k_phrase: tickets run over ptasks[])
        const uint32_t nc = (uint32_t)b->ptasks.size(), first = 0;
#elif TRI_TASKTIMES == 4 // (k_and_dense)
        const uint32_t nc = b->n_dense, first = trip::sched_first(*b, TASK_DENSE);
#elif TRI_TASKTIMES == 3 // (k_planes, the narrow instantiation)
        const uint32_t nc = b->n_planes, first = trip::sched_first(*b, TASK_PLANES);
#else
        const uint32_t nc = b->n_cand, first = trip::sched_first(*b, TASK_CAND);
#endif
        unsigned long long t0 = ~0ull, t1 = 0, busy = 0;
        std::vector<std::pair<unsigned long long, uint32_t>> by;
        for (uint32_t i = 0; i < nc; ++i) {
                const unsigned long long s = g_tt_host[8 * i], e = g_tt_host[8 * i + 1];
                if (!s || !e)
                        continue;
                t0 = std::min(t0, s), t1 = std::max(t1, e);
                busy += e - s;
                by.emplace_back(e - s, i);
        }
        std::sort(by.rbegin(), by.rend());
        const double span_us = (double)(t1 - t0) / 100.0;
        const unsigned wgs = std::min<uint32_t>(nc, (uint32_t)dev->cus * (TRI_TASKTIMES == 3 ? PLK_WGS_PER_CU : TRI_TASKTIMES == 2 ? SCORE_WGS_PER_CU : TRI_TASKTIMES == 5 ? PHRASE_WGS_PER_CU : 4));
        fprintf(stderr, "[tri tasktimes] k_and: %u tasks, span %.1f us, busy %.1f %% of %u workgroups; mean task %.2f us\n", nc, span_us,
                100.0 * (double)busy / ((double)(t1 - t0) * wgs), wgs, (double)busy / 100.0 / std::max<size_t>(1, by.size()));
        if (!by.empty()) { // (by: descending) the distribution, and what share of the workgroups' time the longest tasks take
                auto at = [&](double f) { return (double)by[std::min(by.size() - 1, (size_t)(f * by.size()))].first / 100.0; };
                unsigned long long top1 = 0, top5 = 0, top20 = 0;
                for (size_t i = 0; i < by.size(); ++i) {
                        if (i < by.size() / 100)
                                top1 += by[i].first;
                        if (i < by.size() / 20)
                                top5 += by[i].first;
                        if (i < by.size() / 5)
                                top20 += by[i].first;
                }
                fprintf(stderr, "   task us: max %.1f  p99 %.1f  p90 %.1f  p50 %.1f  p10 %.1f; the longest 1 %% / 5 %% / 20 %% of the tasks take %.1f / %.1f / %.1f %% of the time\n", at(0), at(0.01), at(0.1),
                        at(0.5), at(0.9), 100.0 * top1 / busy, 100.0 * top5 / busy, 100.0 * top20 / busy);
        }
        // the finish-time profile: tasks still running at 25 / 50 / 75 / 90 % of the span
        for (const double f : {0.25, 0.5, 0.75, 0.9}) {
                const unsigned long long at = t0 + (unsigned long long)((double)(t1 - t0) * f);
                unsigned running = 0;
                for (uint32_t i = 0; i < nc; ++i)
                        running += g_tt_host[8 * i] <= at && g_tt_host[8 * i + 1] > at;
                fprintf(stderr, "   at %2.0f %% of the span: %u tasks running\n", f * 100, running);
        }
#if TRI_TASKTIMES == 3 // (k_planes: stamps 2 .. 6 = lists decoded + filter filled, phase A done, tables ready, sweep done, queue drained; 1 = end)
        {
                const char *nm[8] = {"", "", "setup+lists", "phase A", "prune+tables", "sweep", "drain", "end"};
                double sum[8] = {0};
                std::vector<double> span[8];
                for (uint32_t i = 0; i < nc; ++i) {
                        unsigned long long prev = g_tt_host[8 * i];
                        for (int j = 2; j <= 7; ++j) {
                                const unsigned long long at = j == 7 ? g_tt_host[8 * i + 1] : g_tt_host[8 * i + j];
                                if (!at || !prev)
                                        continue;
                                const double d = (double)(at - prev) / 100.0;
                                sum[j] += d;
                                span[j].push_back(d);
                                prev = at;
                        }
                }
                fprintf(stderr, "   phases (us per task: mean / median / p90):");
                for (int j = 2; j <= 7; ++j)
                        if (!span[j].empty()) {
                                std::sort(span[j].begin(), span[j].end());
                                fprintf(stderr, "  %s %.1f / %.1f / %.1f", nm[j], sum[j] / span[j].size(), span[j][span[j].size() / 2], span[j][span[j].size() * 9 / 10]);
                        }
                fprintf(stderr, "\n");
                // ... and by the query's DENSE slots (the sweep's instantiation) and whether it holds sparse ones: where the kernel's time goes
                double tsum[9][2] = {}, ssum[9][2] = {}, asum[9][2] = {};
                unsigned tcnt[9][2] = {};
                for (uint32_t i = 0; i < nc; ++i) {
                        const unsigned long long s0 = g_tt_host[8 * i], e0 = g_tt_host[8 * i + 1];
                        if (!s0 || !e0)
                                continue;
                        const DevTask &tk = b->tasks[b->sched[first + i]];
                        const DevFused &z = b->fused[b->plan[tk.slot].fused_idx];
                        uint32_t nd = 0;
                        for (uint32_t k = 0; k < z.nslots; ++k)
                                nd += z.plane[k] != PL_NONE;
                        const int sp = nd < z.nslots;
                        nd = std::min(nd, 8u);
                        tsum[nd][sp] += (double)(e0 - s0) / 100.0;
                        if (g_tt_host[8 * i + 5] > g_tt_host[8 * i + 4] && g_tt_host[8 * i + 4])
                                ssum[nd][sp] += (double)(g_tt_host[8 * i + 5] - g_tt_host[8 * i + 4]) / 100.0;
                        if (g_tt_host[8 * i + 3] > g_tt_host[8 * i + 2] && g_tt_host[8 * i + 2])
                                asum[nd][sp] += (double)(g_tt_host[8 * i + 3] - g_tt_host[8 * i + 2]) / 100.0;
                        ++tcnt[nd][sp];
                }
                for (uint32_t nd = 0; nd <= 8; ++nd)
                        for (int sp = 0; sp < 2; ++sp)
                                if (tcnt[nd][sp])
                                        fprintf(stderr, "   %u dense slots%s: %u tasks, %.1f %% of the time; per task %.1f us (sweep %.1f, phase A %.1f)\n", nd, sp ? " + sparse" : "          ",
                                                tcnt[nd][sp], 100.0 * tsum[nd][sp] * 100.0 / (double)busy, tsum[nd][sp] / tcnt[nd][sp], ssum[nd][sp] / tcnt[nd][sp], asum[nd][sp] / tcnt[nd][sp]);
        }
#endif
#if TRI_TASKTIMES == 1 // (k_and: the mean of every stamp over all tasks, relative to the task's start)
        {
                double sum[8] = {0}, cnt[8] = {0};
                for (uint32_t i = 0; i < nc; ++i)
                        for (int j = 1; j < 8; ++j)
                                if (g_tt_host[8 * i + j] && g_tt_host[8 * i])
                                        sum[j] += (double)(g_tt_host[8 * i + j] - g_tt_host[8 * i]) / 100.0, cnt[j] += 1;
                fprintf(stderr, "   means over the tasks (us after the task's start): end %.1f  last tile's lead decoded %.1f", sum[1] / std::max(1.0, cnt[1]), sum[2] / std::max(1.0, cnt[2]));
                for (int j = 3; j < 8; ++j)
                        if (cnt[j])
                                fprintf(stderr, "  term %d %.1f (%.0f tasks)", j - 2, sum[j] / cnt[j], cnt[j]);
                fprintf(stderr, "\n");
        }
#endif
        for (size_t k = 0; k < std::min<size_t>(12, by.size()); ++k) {
#if TRI_TASKTIMES == 5
                const uint32_t ti = b->ptasks[by[k].second];
#else
                const uint32_t ti = b->sched[first + by[k].second];
#endif
                const DevTask &tk = b->tasks[ti];
                const DevQuery &q = b->plan[tk.slot];
                std::string tt;
                char buf[96];
                if (task_onepass(tk.kind)) {
                        const DevFused &z = b->fused[q.fused_idx];
                        for (uint32_t j = 0; j < z.nslots; ++j) {
                                snprintf(buf, sizeof buf, " %u(df %u%s)", z.term[j], b->ix->terms[z.term[j]].documents, z.plane[j] != PL_NONE ? " plane" : "");
                                tt += buf;
                        }
                        snprintf(buf, sizeof buf, " nreq %u", z.nreq);
                        tt += buf;
                } else
                for (uint32_t j = 0; j < q.nterms; ++j) {
                        const uint32_t term = b->qterms[q.term_base + j] & QT_TERM;
                        snprintf(buf, sizeof buf, " %s%u(df %u%s)", (b->qterms[q.term_base + j] & QT_GROUP) ? "|" : "", term, b->ix->terms[term].documents,
                                 (!b->qplane.empty() && b->qplane[q.term_base + j] != PL_NONE) ? " plane" : "");
                        tt += buf;
                }
                snprintf(buf, sizeof buf, "  matches %u phrases %u", b->h_counts.empty() ? 0u : b->h_counts[ti], q.nphrases);
                tt += buf;
                fprintf(stderr, "   %.1f us (started %.1f us in)  ticket %u  tiles [%u, %u)  query %u:%s\n", (double)by[k].first / 100.0,
                        (double)(g_tt_host[8 * by[k].second] - t0) / 100.0, by[k].second, tk.tile_begin, tk.tile_end, q.qid, tt.c_str());
                fprintf(stderr, "        last tile: lead decoded +%.1f us", ((double)g_tt_host[8 * by[k].second + 2] - (double)g_tt_host[8 * by[k].second]) / 100.0);
                for (int j = 3; j < 8; ++j)
                        if (g_tt_host[8 * by[k].second + j])
                                fprintf(stderr, "  term %d +%.1f", j - 2, ((double)g_tt_host[8 * by[k].second + j] - (double)g_tt_host[8 * by[k].second]) / 100.0);
                fprintf(stderr, "\n");
        }
}
#endif

// the run's HIP-event times: last_run_ms from start to end, and per stage the interval between two neighbouring events (term_planes_ms includes the
// ticket memset that precedes the plane rows)
static void read_stage_times(tri_batch *b) {
        static const struct { BatchEvent from; float tri_batch_info::*ms; } STAGES[] = { // (from event `from` to the next one)
                {EV_START, &tri_batch_info::term_planes_ms}, {EV_PLANE_ROWS, &tri_batch_info::dense_ms}, {EV_DENSE, &tri_batch_info::pset_ms}, {EV_PSET, &tri_batch_info::probe_ms},
                {EV_PROBE, &tri_batch_info::cand_ms}, {EV_CAND, &tri_batch_info::fused_ms}, {EV_FUSED, &tri_batch_info::planes_ms}, {EV_PLANES, &tri_batch_info::phrase_ms},
                {EV_PHRASE, &tri_batch_info::tree_ms}, {EV_TREE, &tri_batch_info::rest_ms}};
        float ms = 0;
        if (hipEventElapsedTime(&ms, b->ev[EV_START], b->ev[EV_END]) == hipSuccess)
                b->info.last_run_ms = ms;
        for (const auto &s : STAGES) {
                b->info.*s.ms = 0;
                if (!b->tasks.empty() && hipEventElapsedTime(&ms, b->ev[s.from], b->ev[s.from + 1]) == hipSuccess)
                        b->info.*s.ms = ms;
        }
}

// the matches per task and per query, and the SURVEY §8(d) byte counts the batch's info reports
static int account_matches(tri_batch *b) {
        b->h_counts.resize(b->tasks.size());
        if (!b->tasks.empty())
                HIP_TRY(hipMemcpy(b->h_counts.data(), b->d_counts, b->tasks.size() * 4, hipMemcpyDeviceToHost));
        const bool sc = b->flags & TRI_FLAG_ACCUMULATED_SCORE;
        // per task kind (that of the query's first task): the matches, and the bytes the results take in the form they are delivered in — a
        // bitmap: its words; a one-pass query: 8 B x min(matches, K) (the docIDs of a DocumentsOnly general tree); the docset-materialising
        // kinds of a top-K batch: 8 B x min(matches, K) as well (counted by the bound alone)
        uint64_t m = 0, m_kind[TASK_KINDS] = {}, out_kind[TASK_KINDS] = {};
        b->h_query_counts.assign(b->plan.size(), 0);
        for (size_t sidx = 0; sidx < b->plan.size(); ++sidx) {
                const DevQuery &q = b->plan[sidx];
                for (uint32_t t = 0; t < q.ntasks; ++t)
                        b->h_query_counts[sidx] += b->h_counts[q.first_task + t];
                if (q.qid == 0xffffffffu) // (a hidden phrase query: its matches are a leaf of a TASK_TREE query, not a result)
                        continue;
                const uint64_t c = b->h_query_counts[sidx];
                m += c;
                if (!q.ntasks)
                        continue;
                const uint32_t kind = b->tasks[q.first_task].kind;
                m_kind[kind] += c;
                if (task_onepass(kind))
                        out_kind[kind] += q.out_cap ? 4 * c : 8 * std::min<uint64_t>(c, b->topk);
                else if (kind != TASK_TREE)
                        out_kind[kind] += sc && b->topk ? 8 * std::min<uint64_t>(c, b->topk) : (kind == TASK_DENSE || kind == TASK_PSET) && q.form == RESULT_BITMAP ? 4ull * q.out_cap : 4 * c;
        }
        const uint64_t out_fused = out_kind[TASK_FUSED] + out_kind[TASK_FUSED16] + out_kind[TASK_FUSED_GEN], out_planes = out_kind[TASK_PLANES] + out_kind[TASK_PLANES8];
        b->info.dense_algorithmic_bytes = b->term_bytes_dense + 4 * m_kind[TASK_DENSE];
        b->info.pset_algorithmic_bytes = b->term_bytes_pset + 4 * m_kind[TASK_PSET];
        b->info.pset_queries = b->pset_queries;
        b->info.probe_algorithmic_bytes = b->term_bytes_probe + 4 * m_kind[TASK_PROBE];
        b->info.probe_queries = b->probe_queries;
        b->info.cand_algorithmic_bytes = (b->term_bytes - b->term_bytes_dense - b->term_bytes_pset - b->term_bytes_probe - b->term_bytes_fused - b->term_bytes_planes - b->term_bytes_phrase_hits) + 4 * m_kind[TASK_CAND];
        b->info.planes_algorithmic_bytes = b->term_bytes_planes + out_planes; // docbytes + 8 B x min(matches, K), per query — the lists
                                                                              // the batch's queries share are nevertheless decoded once per launch
        // (term_planes_decoded_bytes: set by tri_batch_run — the list bytes of the plane rows THAT run had to build; 0 once the index's cache holds them)
        b->info.phrase_algorithmic_bytes = b->term_bytes_phrase_hits; // what k_phrase streams by the SURVEY §8(d) count: the hit bytes of the phrases' terms
        b->info.phrase_queries = 0;
        for (const DevQuery &q : b->plan)
                b->info.phrase_queries += q.nphrases != 0;
        b->info.cand_needed_bytes = b->cand_needed_term_bytes ? b->cand_needed_term_bytes + 4 * (m_kind[TASK_CAND] + m_kind[TASK_PROBE]) : 0; // (the candidate-tile AND the probe queries: what a perfect gallop reads)
        b->info.fused_algorithmic_bytes = b->term_bytes_fused + out_fused; // docbytes + 8 B x min(matches, K)
        b->info.matches = m;
        if (b->distinct_bytes) { // (option account_needed_bytes: the batch-level bound — every distinct list once + every output once)
                b->info.pset_bound_bytes = b->distinct_bytes_kind[TASK_PSET] + out_kind[TASK_PSET];
                b->info.probe_bound_bytes = b->distinct_bytes_kind[TASK_PROBE] + out_kind[TASK_PROBE];
                b->info.dense_bound_bytes = b->distinct_bytes_kind[TASK_DENSE] + out_kind[TASK_DENSE];
                b->info.cand_bound_bytes = b->distinct_bytes_kind[TASK_CAND] + out_kind[TASK_CAND];
                b->info.fused_bound_bytes = b->distinct_bytes_kind[TASK_FUSED] + b->distinct_bytes_kind[TASK_FUSED16] + b->distinct_bytes_kind[TASK_FUSED_GEN] + out_fused;
                b->info.planes_bound_bytes = b->distinct_bytes_kind[TASK_PLANES] + b->distinct_bytes_kind[TASK_PLANES8] + out_planes;
                b->info.phrase_bound_bytes = b->distinct_bytes_kind[TASK_KINDS];
                b->info.bound_bytes = b->distinct_bytes;
                for (const uint64_t o : out_kind)
                        b->info.bound_bytes += o;
        }
        if (sc) {
                uint64_t outb = 0; // 8 B x min(matches, K) per query
                for (uint64_t c : b->h_query_counts)
                        outb += 8 * std::min<uint64_t>(c, b->topk);
                b->info.algorithmic_bytes = b->term_bytes + outb;
        } else
                b->info.algorithmic_bytes = b->term_bytes + 4 * m; // docbytes + 4 B per match (docs-only)
        return TRI_OK;
}

// a ranked default-mode batch (tri_batch_set_ranker), right behind the WRITE pass: every task's matches scored and cut to the task's best K (k_rich_rank,
// over the same two sections of the rich schedule as launch_rich), then the tasks' lists folded per query (k_rank_merge)
static int launch_rank(tri_batch *b) {
        tri_dev *dev = b->dev;
        const uint32_t n_wide = b->n_rich_wide, n = (uint32_t)b->tasks.size() - n_wide;
        const uint32_t *sched = n_wide ? b->dev_at(b->rich_sched) : b->dev_at(b->sched);
        const RichWideArgs wd{b->d_rich_present_hi, b->d_rich_allow_hi, b->d_rich_freq_wide, b->dev_opt(b->rich_wide)};
#define RANK_ARGS(SCHED, N)                                                                                                                                                                \
        b->dev_at(b->plan), b->dev_at(b->tasks), SCHED, N, (const uint32_t *)b->d_out, (const uint32_t *)b->d_counts, b->rich_R, (const uint32_t *)b->d_rich_present,                     \
                (const uint16_t *)b->d_rich_freq, (const uint64_t *)b->d_task_pos_base, (const uint16_t *)b->d_rich_pool, (const double *)b->d_rank_w, b->rank.freq_cap,                  \
                b->rank.adjacency, b->rank.topk, b->d_rank_part_docs, b->d_rank_part_scores, b->d_rank_part_counts
        if (n)
                hipLaunchKernelGGL(k_rich_rank<false>, dim3(std::min<uint32_t>(n, (uint32_t)dev->cus * 8)), dim3(AND_WG), 0, dev->stream, RANK_ARGS(sched, n), RichWideArgs{});
        if (n_wide)
                hipLaunchKernelGGL(k_rich_rank<true>, dim3(std::min<uint32_t>(n_wide, (uint32_t)dev->cus * 8)), dim3(AND_WG), 0, dev->stream, RANK_ARGS(sched + n, n_wide), wd);
#undef RANK_ARGS
        HIP_TRY(hipGetLastError());
        const uint32_t nqs = (uint32_t)b->plan.size();
        hipLaunchKernelGGL(k_rank_merge, dim3(std::min<uint32_t>(nqs, (uint32_t)dev->cus * 8)), dim3(AND_WG), 0, dev->stream, b->dev_at(b->plan), nqs, b->rank.topk,
                           (const uint32_t *)b->d_rank_part_docs, (const double *)b->d_rank_part_scores, (const uint32_t *)b->d_rank_part_counts, b->d_rank_docs, b->d_rank_scores,
                           b->d_rank_counts);
        HIP_TRY(hipGetLastError());
        return TRI_OK;
}

// TRI_FLAG_MATCHED_TERMS: the COUNT pass left every task's hit total — turned into pool offsets here (the pool is packed: task after task in
// query order, inside a task match-major then term-minor) —, then the WRITE pass fills in the positions
static int rich_write_pass(tri_batch *b) {
        if (!(b->flags & TRI_FLAG_MATCHED_TERMS) || b->tasks.empty())
                return TRI_OK;
        tri_dev *dev = b->dev;
        const size_t nt = b->tasks.size();
        std::vector<uint32_t> th(nt);
        HIP_TRY(hipMemcpy(th.data(), b->d_task_hits, nt * 4, hipMemcpyDeviceToHost));
        b->h_task_pos_base.assign(nt + 1, 0);
        for (size_t i = 0; i < nt; ++i)
                b->h_task_pos_base[i + 1] = b->h_task_pos_base[i] + th[i];
        const size_t total = b->h_task_pos_base[nt];
        if (total + 64 > b->rich_pool_cap) {
                b->rich_pool_cap = total + total / 8 + 64;
                HIP_TRY(b->d_rich_pool.alloc(b->rich_pool_cap * 2)); // (alloc: the old buffer is released first)
                if (b->flags & TRI_FLAG_HIT_PAYLOADS) {
                        b->d_rich_plen.reset();
                        b->d_rich_payload.reset();
                        HIP_TRY(b->d_rich_plen.alloc(b->rich_pool_cap));
                        HIP_TRY(b->d_rich_payload.alloc(b->rich_pool_cap * 8));
                }
        }
        HIP_TRY(hipMemcpy(b->d_task_pos_base, b->h_task_pos_base.data(), (nt + 1) * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemsetAsync(b->d_ticket + TICKET_RICH_WRITE_WORD, 0, (TICKET_RICH_WIDE + 1) * 4, dev->stream)); // (the wide instantiation's word too)
        // (a ranked batch: the WRITE pass and the rank pass timed apart — options rich_write_last_us / rank_last_us; the events go back to the handle's pool on
        //  every way out of the function)
        PooledEvent rev[3];
        if (b->rank_on) {
                for (PooledEvent &e : rev)
                        HIP_TRY(e.take(dev));
                HIP_TRY(hipEventRecord(rev[0], dev->stream));
        }
        if (const int rc = launch_rich<true>(b))
                return rc;
        if (b->rank_on) {
                HIP_TRY(hipEventRecord(rev[1], dev->stream));
                if (const int rc = launch_rank(b))
                        return rc;
                HIP_TRY(hipEventRecord(rev[2], dev->stream));
        }
        HIP_TRY(hipStreamSynchronize(dev->stream));
        if (b->rank_on) {
                float w_ms = 0, r_ms = 0;
                HIP_TRY(hipEventElapsedTime(&w_ms, rev[0], rev[1]));
                HIP_TRY(hipEventElapsedTime(&r_ms, rev[1], rev[2]));
                dev->rich_write_last_us = (uint64_t)(w_ms * 1000.0f);
                dev->rank_last_us = (uint64_t)(r_ms * 1000.0f);
                b->rank_done = true;
        }
        b->info.algorithmic_bytes += 2 * total + 4 * b->info.matches; // + the positions handed over and a present mask per match
        return TRI_OK;
}

extern "C" int tri_batch_sync(tri_batch *b) {
        if (!b)
                return fail(TRI_ERR_INVALID, "null batch");
        tri_dev *dev = b->ix->dev;
        HIP_TRY(hipSetDevice(dev->device));
        if (!b->ran)
                return fail(TRI_ERR_INVALID, "tri_batch_sync: the batch has not been run");
#if (defined(TRI_TRACE) && !defined(TRI_TRACE_NOPOLL)) || defined(TRI_POLL)
        {
                const char *w = getenv("TRINITY_WATCHDOG_S");
                const double limit = w ? atof(w) : 10.0;
                double waited = 0;
                while (hipEventQuery(b->ev[EV_END]) == hipErrorNotReady) {
                        struct timespec ts = {0, 50 * 1000 * 1000};
                        nanosleep(&ts, nullptr);
                        waited += 0.05;
                        if (waited > limit) {
                                fprintf(stderr, "[tri watchdog] kernel still running after %.1fs; per-workgroup markers {stage,a,b,count}:\n", waited);
#ifdef TRI_TRACE
                                for (int i = 0; i < 64; ++i)
                                        if (g_trace_host[i * 4 + 3])
                                                fprintf(stderr, "  wg%%64=%d stage=%u a=%u b=%u n=%u\n", i, g_trace_host[i * 4], g_trace_host[i * 4 + 1],
                                                        g_trace_host[i * 4 + 2], g_trace_host[i * 4 + 3]);
#endif
                                fflush(stderr);
                                _exit(3);
                        }
                }
        }
#endif
        // THIS batch's last event, not the engine stream: a caller that keeps the stream fed (the next batch launched before this one is
        // awaited — bench.py's loop) gets this batch's results when THEY are ready, not when everything queued behind them is
        HIP_TRY(hipEventSynchronize(b->ev[EV_END]));
        DevLock dev_lock(dev->mu); // (the wait above stands outside the lock; what follows may enqueue on the engine stream)
#ifdef TRI_TASKTIMES
        report_tasktimes(b);
#endif
        read_stage_times(b);
        sync_consumers(b);
        int rc;
        if ((rc = account_matches(b)) || (rc = rich_write_pass(b)))
                return rc;
        b->synced = true;
        return TRI_OK;
}

// tri_batch_set_ranker: which program tokens the default mode reports — every TERM token outside the excluded side of a NOT (the second operand's subtree)
static void reportable_tokens(const uint32_t *prog, const uint32_t plen, std::vector<uint8_t> &rep) {
        rep.assign(plen, 1);
        std::vector<uint32_t> start; // per sub-program on the evaluation stack: its first token
        for (uint32_t i = 0; i < plen; ++i) {
                const uint32_t op = prog[i] >> 28, arg = prog[i] & 0x0fffffffu;
                uint32_t kids = 0;
                if (op == TRI_OP_AND || op == TRI_OP_OR || op == TRI_OP_PHRASE)
                        kids = arg;
                else if (op == TRI_OP_NOT || op == TRI_OP_OPT)
                        kids = 2;
                else if (op == TRI_OP_SOME)
                        kids = arg & 0xffffu;
                if (op == TRI_OP_TERM || kids == 0 || kids > start.size()) { // (a malformed program never got past tri_batch_create)
                        start.push_back(i);
                        continue;
                }
                if (op == TRI_OP_NOT)
                        for (uint32_t t = start.back(); t < i; ++t)
                                rep[t] = 0;
                const uint32_t first = start[start.size() - kids];
                start.resize(start.size() - kids);
                start.push_back(first);
        }
}

// the ranker's block (tri_batch::d_rank_block) at topk K: its sections named once, as batch_arena's are; zeroed from *zero_from on
static size_t rank_block(tri_batch *b, uint8_t *base, const size_t K, size_t *zero_from) {
        const size_t ns = b->sterms.size(), nt = b->tasks.size(), nq = b->nq;
        Carver carve{base};
        carve(b->d_rank_w, (ns + 1) * 8);
        carve(b->d_rank_part_scores, (nt * K + 1) * 8);
        carve(b->d_rank_part_docs, (nt * K + 1) * 4);
        carve(b->d_rank_part_counts, (nt + 1) * 4);
        *zero_from = carve.at;
        carve(b->d_rank_scores, (nq * K + 1) * 8);
        carve(b->d_rank_docs, (nq * K + 1) * 4);
        carve(b->d_rank_counts, (nq + 1) * 4);
        return carve.at;
}

extern "C" int tri_batch_set_ranker(tri_batch *b, const tri_ranker *spec, const double *weights) {
        if (!b)
                return fail(TRI_ERR_INVALID, "tri_batch_set_ranker: null batch");
        if (!(b->flags & TRI_FLAG_MATCHED_TERMS))
                return fail(TRI_ERR_INVALID, "tri_batch_set_ranker: mode: not a TRI_FLAG_MATCHED_TERMS batch (the ranker scores the default mode's matched terms)");
        tri_dev *dev = b->dev;
        if (spec) {
                if (spec->kind != TRI_RANK_PROXIMITY)
                        return fail(TRI_ERR_INVALID, "tri_batch_set_ranker: kind %u is unknown (TRI_RANK_PROXIMITY)", spec->kind);
                if (spec->topk < 1 || spec->topk > TOPK_MAX)
                        return fail(TRI_ERR_INVALID, "tri_batch_set_ranker: topk %u (1 .. %u)", spec->topk, TOPK_MAX);
                if (spec->freq_cap < 1)
                        return fail(TRI_ERR_INVALID, "tri_batch_set_ranker: freq_cap 0 (>= 1)");
                if (spec->reserved)
                        return fail(TRI_ERR_INVALID, "tri_batch_set_ranker: reserved must be 0");
                if (!std::isfinite(spec->adjacency) || spec->adjacency < 0)
                        return fail(TRI_ERR_INVALID, "tri_batch_set_ranker: adjacency must be finite and >= 0");
                if (weights)
                        for (size_t i = 0; i < b->h_prog.size(); ++i)
                                if (!std::isfinite(weights[i]))
                                        return fail(TRI_ERR_INVALID, "tri_batch_set_ranker: weights[%zu] is not finite", i);
        }
        DevLock dev_lock(dev->mu);
        HIP_TRY(hipSetDevice(dev->device));
        const uint32_t had = b->rank_on ? 2u + (b->n_rich_wide && b->tasks.size() > b->n_rich_wide ? 1u : 0u) : 0u; // (k_rich_rank per section of the schedule + k_rank_merge)
        if (!spec) {
                b->d_rank_block.reset();
                b->rank_on = b->rank_done = false;
                b->info.launches -= had;
                return TRI_OK;
        }
        // slot k's weight: that of the first reportable token that names the slot's term
        const size_t ns = b->sterms.size(), nt = b->tasks.size(), nq = b->nq, K = spec->topk;
        std::vector<double> w(ns + 1, 1.0);
        if (weights) {
                std::vector<uint8_t> rep;
                for (size_t qi = 0; qi < nq; ++qi) {
                        const uint32_t slot = b->slot_of_query[qi];
                        if (slot == UINT32_MAX)
                                continue;
                        const DevQuery &dq = b->plan[slot];
                        const uint32_t *prog = b->h_prog.data() + b->h_queries[qi].prog_off;
                        const uint32_t plen = b->h_queries[qi].prog_len;
                        reportable_tokens(prog, plen, rep);
                        for (uint32_t k = 0; k < dq.nscore; ++k) {
                                const uint32_t term = b->sterms[dq.score_base + k];
                                uint32_t at = UINT32_MAX;
                                for (uint32_t i = 0; i < plen && at == UINT32_MAX; ++i)
                                        if ((prog[i] >> 28) == TRI_OP_TERM && (prog[i] & 0x0fffffffu) == term && rep[i])
                                                at = i;
                                if (at != UINT32_MAX)
                                        w[dq.score_base + k] = weights[b->h_queries[qi].prog_off + at];
                        }
                }
        }
        size_t a_zero = 0;
        const size_t a = rank_block(b, nullptr, K, &a_zero);
        Pooled<uint8_t> blk; // (the batch keeps the block it has until the new one stands)
        HIP_TRY(blk.alloc(dev, a + 256));
        // (the rows of queries the planner left out are never written: they stay zero; the weights open the block)
        if (hipMemsetAsync(blk + a_zero, 0, a - a_zero, dev->stream) != hipSuccess || hipMemcpyAsync(blk, w.data(), (ns + 1) * 8, hipMemcpyHostToDevice, dev->stream) != hipSuccess ||
            hipStreamSynchronize(dev->stream) != hipSuccess)
                return fail(TRI_ERR_DEVICE, "tri_batch_set_ranker: %s", hipGetErrorString(hipGetLastError()));
        b->d_rank_block = std::move(blk);
        rank_block(b, b->d_rank_block, K, &a_zero);
        b->rank = *spec;
        b->rank_on = true;
        b->rank_done = false;
        b->info.launches += 2u + (b->n_rich_wide && nt > b->n_rich_wide ? 1u : 0u) - had;
        return TRI_OK;
}

// a collection batch (tri_cbatch_create ... below: "collections of segments"; here, because its result calls are read_side.hpp's too)
struct tri_cbatch {
        DevRef dev; // (first: released last.  The collection's own reference: its parts may be destroyed before it)
        std::vector<tri_batch *> parts;
        std::vector<DevMem<uint32_t>> d_slots; // per part: caller query -> plan slot
        DevMem<DevSource> d_src;
        DevMem<uint32_t> d_top_docs, d_top_counts;
        DevMem<float> d_top_scores;
        DevMem<uint64_t> d_counts;
        // tri_cbatch_ranked (k_rank_merge_sources): the merged [nq][rank_k] blocks and the parts' {docs, scores, counts} table — allocated by the first run that finds
        // the collection ranked (every part carries a ranker, all tri_ranker structs bytewise equal), re-sized when topk changed; rank_why: why a run was not ranked
        bool ranked = false;
        uint32_t rank_k = 0;
        DevMem<uint32_t> d_rank_docs, d_rank_counts;
        DevMem<double> d_rank_scores;
        DevMem<DevRankSource> d_rank_src;
        std::vector<DevRankSource> rank_src;
        std::string rank_why;
        PooledEvent rank_ev[2]; // around the merge kernel (option crank_merge_last_us)
        bool rank_timed = false;
        // tri_cbatch_ordered (k_order_merge<true>): the merged [nq][order_k] keys and counts and the parts' {rows, counts} table, as the ranked blocks above — a run
        // finds the collection ordered when every part carries an order of the same topk and direction; order_why: why a run was not
        bool ordered = false;
        uint32_t order_k = 0;
        DevMem<uint64_t> d_order_keys;
        DevMem<uint32_t> d_order_counts;
        DevMem<DevOrderLists> d_order_src;
        std::vector<DevOrderLists> order_src;
        std::string order_why;
        bool ran = false, synced = false;
        ~tri_cbatch() {
                if (dev)
                        hipSetDevice(dev->device);
        }
};

// ------------------------------------------------------------------------------------------ read side
// every result call of a batch and of a collection batch: one query view, one segment walk, one read-back rule
#include "read_side.hpp"

// ------------------------------------------------------------------------------------------ per-query document filters
// IndexDocumentsFilter (matches.h:190-201; exec.cpp:1133-1150: tested where the masked documents are, before consider()) as a device bitmap per filter and a
// row id per query: k_filter.hpp.  A filter's bitmap is built on the engine stream — behind every run already queued, ahead of every later one — and the call
// returns once it stands (the docID list's staging buffer is released then)
namespace {
        // the bitmap's buffer and handle; the caller fills it under the handle's lock
        int filter_new(tri_index *ix, std::unique_ptr<tri_filter> &f) {
                f = std::make_unique<tri_filter>();
                f->ix = ix;
                f->dev.retain(ix->dev);
                f->words = filter_words(ix);
                HIP_TRY(f->d_bits.alloc(ix->dev, f->words * 4));
                return TRI_OK;
        }
        // KEEP: the allow-list's bitmap becomes the drop bitmap; then wait for the filter to stand
        int filter_finish(tri_filter *f, const int mode, std::unique_lock<std::recursive_mutex> &lock) {
                tri_dev *dev = f->dev;
                if (mode == TRI_FILTER_KEEP) {
                        const size_t n4 = f->words / 4;
                        hipLaunchKernelGGL(k_filter_complement, dim3((unsigned)std::min<size_t>((n4 + FILTER_WG - 1) / FILTER_WG, 1024)), dim3(FILTER_WG), 0, dev->stream, (uint4 *)f->d_bits.get(), n4);
                        HIP_TRY(hipGetLastError());
                }
                PooledEvent done;
                HIP_TRY(done.take(dev));
                const hipError_t e = hipEventRecord(done, dev->stream);
                lock.unlock(); // (the wait stands outside the lock, like tri_batch_sync's)
                HIP_TRY(e == hipSuccess ? hipEventSynchronize(done) : e);
                return TRI_OK;
        }
} // namespace

extern "C" int tri_filter_create(tri_index *ix, const uint32_t *docids, size_t n, int mode, tri_filter **out) {
        if (!ix || !out || (!docids && n))
                return fail(TRI_ERR_INVALID, "tri_filter_create: null argument");
        if (mode != TRI_FILTER_DROP && mode != TRI_FILTER_KEEP)
                return fail(TRI_ERR_INVALID, "tri_filter_create: mode %d is neither TRI_FILTER_DROP nor TRI_FILTER_KEEP", mode);
        tri_dev *dev = ix->dev;
        HIP_TRY(hipSetDevice(dev->device));
        std::unique_ptr<tri_filter> f;
        if (const int rc = filter_new(ix, f))
                return rc;
        Pooled<uint32_t> d_ids; // (the docID list's staging buffer: released on every way out)
        std::unique_lock<std::recursive_mutex> lock(dev->mu);
        HIP_TRY(hipMemsetAsync(f->d_bits, 0, f->words * 4, dev->stream));
        if (n) {
                HIP_TRY(d_ids.alloc(dev, n * 4));
                HIP_TRY(hipMemcpyAsync(d_ids, docids, n * 4, hipMemcpyHostToDevice, dev->stream)); // (pageable source: staged before the call returns)
                hipLaunchKernelGGL(k_filter_scatter, dim3((unsigned)std::min<size_t>((n + FILTER_WG - 1) / FILTER_WG, 4096)), dim3(FILTER_WG), 0, dev->stream, (const uint32_t *)d_ids, n,
                                   ix->max_doc, f->d_bits);
                HIP_TRY(hipGetLastError());
        }
        if (const int rc = filter_finish(f.get(), mode, lock))
                return rc;
        *out = f.release();
        return TRI_OK;
}

extern "C" int tri_filter_from_docset(tri_batch *b, size_t q, int mode, tri_filter **out) {
        if (!b || !out)
                return fail(TRI_ERR_INVALID, "tri_filter_from_docset: null argument");
        if (mode != TRI_FILTER_DROP && mode != TRI_FILTER_KEEP)
                return fail(TRI_ERR_INVALID, "tri_filter_from_docset: mode %d is neither TRI_FILTER_DROP nor TRI_FILTER_KEEP", mode);
        if (q >= b->nq)
                return fail(TRI_ERR_INVALID, "tri_filter_from_docset: query %zu of %zu", q, b->nq);
        if (!(b->flags & TRI_FLAG_DOCUMENTS_ONLY))
                return fail(TRI_ERR_INVALID, "tri_filter_from_docset: a filter is made of a DocumentsOnly batch's docID set");
        if (!b->synced)
                return fail(TRI_ERR_INVALID, "tri_filter_from_docset: tri_batch_sync first");
        tri_index *ix = b->ix;
        tri_dev *dev = b->dev;
        HIP_TRY(hipSetDevice(dev->device));
        std::unique_ptr<tri_filter> f;
        if (const int rc = filter_new(ix, f))
                return rc;
        std::unique_lock<std::recursive_mutex> lock(dev->mu);
        HIP_TRY(hipMemsetAsync(f->d_bits, 0, f->words * 4, dev->stream));
        const uint32_t slot = b->slot_of_query[q];
        if (slot != UINT32_MAX && b->plan[slot].ntasks) { // (else: a query that can never match — the empty set)
                const DevQuery &dq = b->plan[slot];
                uint32_t most = 0; // the longest task segment: docIDs, or the words of its docID windows
                for_each_segment(b, dq, [&](size_t, const uint32_t t, uint64_t, const uint32_t c) {
                        most = std::max(most, dq.form == RESULT_BITMAP ? (b->tasks[t].tile_end - b->tasks[t].tile_begin) * SPAN_WORDS : c);
                });
                if (dq.ntasks > 65535u) // (gridDim.y; a query is cut into a few hundred tasks at the most)
                        return fail(TRI_ERR_UNSUPPORTED, "tri_filter_from_docset: query %zu has more than 65535 tasks", q);
                if (most) {
                        hipLaunchKernelGGL(k_filter_from_docset, dim3(std::min<uint32_t>((most + FILTER_WG - 1) / FILTER_WG, 256u), dq.ntasks), dim3(FILTER_WG), 0, dev->stream,
                                           (const DevQuery *)b->dev_at(b->plan), (const DevTask *)b->dev_at(b->tasks), slot, (const uint32_t *)b->d_out, (const uint32_t *)b->d_counts,
                                           ix->max_doc, f->d_bits, f->words);
                        HIP_TRY(hipGetLastError());
                }
        }
        if (const int rc = filter_finish(f.get(), mode, lock))
                return rc;
        *out = f.release();
        return TRI_OK;
}

extern "C" void tri_filter_destroy(tri_filter *f) {
        delete f; // its d_bits hands the bitmap back
}

extern "C" int tri_batch_set_filters(tri_batch *b, tri_filter *const *filters, size_t nf, const uint32_t *filter_of_query) {
        if (!b || (nf && (!filters || !filter_of_query)))
                return fail(TRI_ERR_INVALID, "tri_batch_set_filters: null argument");
        tri_dev *dev = b->dev;
        DevLock dev_lock(dev->mu);
        if (!nf) {
                b->filter_rows.clear(); // (the table and the rows stay with the batch until it goes)
                return TRI_OK;
        }
        for (size_t i = 0; i < nf; ++i)
                if (!filters[i] || filters[i]->ix != b->ix)
                        return fail(TRI_ERR_INVALID, "tri_batch_set_filters: filter %zu %s", i, filters[i] ? "belongs to another index" : "is null");
        for (size_t q = 0; q < b->nq; ++q)
                if (filter_of_query[q] != 0xffffffffu && filter_of_query[q] >= nf)
                        return fail(TRI_ERR_INVALID, "tri_batch_set_filters: query %zu names filter %u of %zu", q, filter_of_query[q], nf);
        // row ids, in the order the plan's slots first name a filter (a hidden phrase query — no caller query — takes the index's mask: the tree's root applies the owner's filter)
        const size_t nslots = b->plan.size(), ptrs_off = filter_tab_ptrs_off(b);
        std::vector<uint32_t> row_of_filter(nf, 0), row_of_slot(nslots, 0);
        std::vector<const tri_filter *> rows;
        for (size_t s = 0; s < nslots; ++s) {
                const uint32_t qid = b->plan[s].qid;
                if (qid == 0xffffffffu || filter_of_query[qid] == 0xffffffffu)
                        continue;
                uint32_t &r = row_of_filter[filter_of_query[qid]];
                if (!r) {
                        rows.push_back(filters[filter_of_query[qid]]);
                        r = (uint32_t)rows.size();
                }
                row_of_slot[s] = r;
        }
        if (rows.empty()) {
                b->filter_rows.clear();
                return TRI_OK;
        }
        HIP_TRY(hipSetDevice(dev->device));
        const size_t stride = filter_words(b->ix);
        if (rows.size() > b->filter_rows_cap || !b->d_filter_tab) {
                if (b->ran && !b->synced) // (a run in flight reads the buffers that are about to go back to the pool)
                        HIP_TRY(hipStreamSynchronize(dev->stream));
                b->d_filter_tab.reset();
                b->d_filter_rows.reset();
                b->filter_rows_cap = 0;
                b->filter_rows.clear();
                HIP_TRY(b->d_filter_tab.alloc(dev, ptrs_off + std::max(rows.size(), b->nq) * sizeof(void *)));
                HIP_TRY(b->d_filter_rows.alloc(dev, rows.size() * stride * 4));
                b->filter_rows_cap = rows.size();
        }
        // one block — [row id per slot][source pointer per row] — on the engine stream: behind the runs already queued, which keep the assignment they were launched with
        std::vector<uint8_t> tab(ptrs_off + rows.size() * sizeof(void *), 0);
        memcpy(tab.data(), row_of_slot.data(), nslots * 4);
        for (size_t r = 0; r < rows.size(); ++r) {
                const uint32_t *bits = rows[r]->d_bits;
                memcpy(tab.data() + ptrs_off + r * sizeof(void *), &bits, sizeof(void *));
        }
        HIP_TRY(hipMemcpyAsync(b->d_filter_tab, tab.data(), tab.size(), hipMemcpyHostToDevice, dev->stream)); // (pageable source: staged before the call returns)
        b->filter_rows = std::move(rows);
        return TRI_OK;
}

// column predicates as document filters (tri_filters_from_columns), and any filter's bitmap read back (tri_filter_bitmap)
#include "colfilter_side.hpp"

// ------------------------------------------------------------------------------------------ collections of segments
// IndexSourcesCollection (index_source.cpp:3-30): a query runs over every source of the collection, each source masked by what the
// newer ones update (tri_index_set_masked), and the application's filter sees the matches of all of them (exec_query per source,
// exec.h:57-62).  A tri_cbatch borrows one tri_batch per source — the same queries, term indices resolved per source — runs them back
// to back on the engine stream and merges on the device: match counts add up, top-K lists merge K-way from the parts' partial lists.
extern "C" int tri_cbatch_create(tri_batch *const *parts, size_t n, tri_cbatch **out) {
        if (!parts || !n || !out)
                return fail(TRI_ERR_INVALID, "tri_cbatch_create: null argument");
        for (size_t i = 0; i < n; ++i) {
                if (!parts[i])
                        return fail(TRI_ERR_INVALID, "tri_cbatch_create: null part %zu", i);
                if (parts[i]->ix->dev != parts[0]->ix->dev || parts[i]->nq != parts[0]->nq || parts[i]->flags != parts[0]->flags ||
                    parts[i]->topk != parts[0]->topk)
                        return fail(TRI_ERR_INVALID, "tri_cbatch_create: part %zu differs from part 0 in device, query count, flags or topk", i);
        }
        tri_dev *dev = parts[0]->ix->dev;
        HIP_TRY(hipSetDevice(dev->device));
        auto c = std::make_unique<tri_cbatch>();
        c->dev.retain(dev);
        c->parts.assign(parts, parts + n);
        const size_t nq = parts[0]->nq, k = parts[0]->topk;
        std::vector<DevSource> src(n);
        c->d_slots.resize(n);
        for (size_t i = 0; i < n; ++i) {
                if (const int rc = dev_upload(c->d_slots[i], parts[i]->slot_of_query))
                        return rc;
                src[i] = {parts[i]->dev_at(parts[i]->plan), c->d_slots[i], parts[i]->d_part_docs, parts[i]->d_part_scores, parts[i]->d_part_counts, parts[i]->d_qcounts};
        }
        int rc;
        if ((rc = dev_upload(c->d_src, src)))
                return rc;
        HIP_TRY(c->d_counts.alloc((nq + 1) * 8));
        if ((parts[0]->flags & TRI_FLAG_ACCUMULATED_SCORE) && k) {
                HIP_TRY(c->d_top_docs.alloc((nq * k + 1) * 4));
                HIP_TRY(c->d_top_scores.alloc((nq * k + 1) * 4));
                HIP_TRY(c->d_top_counts.alloc((nq + 1) * 4));
        }
        *out = c.release();
        return TRI_OK;
}

extern "C" void tri_cbatch_destroy(tri_cbatch *c) { delete c; }

// per query: TRI_OK, or TRI_ERR_UNSUPPORTED when the planner left the query out of ANY part (its answer over the collection is then
// incomplete: the caller keeps its CPU path for that query, as with tri_batch_query_status)
extern "C" int tri_cbatch_query_status(const tri_cbatch *c, int32_t *status) {
        if (!c || !status)
                return fail(TRI_ERR_INVALID, "null argument");
        const size_t nq = c->parts[0]->nq;
        for (size_t q = 0; q < nq; ++q) {
                status[q] = TRI_OK;
                for (const tri_batch *p : c->parts)
                        if (p->qstatus[q] != TRI_OK)
                                status[q] = p->qstatus[q];
        }
        return TRI_OK;
}

// tri_cbatch_ranked, at tri_cbatch_run: is the collection ranked for this run?  Every part carries a ranker and the tri_ranker structs are bytewise equal (the
// weights are each part's own).  If so the merged blocks exist at the rankers' topk and the parts' table — a part's ranker block moves when its ranker is
// replaced — goes to the device on the engine stream, ahead of the merge tri_cbatch_sync queues.  If not, nothing is allocated, copied or launched.
static int cbatch_rank_prepare(tri_cbatch *c) {
        c->ranked = false;
        const tri_batch *p0 = c->parts[0];
        char why[160];
        for (size_t i = 0; i < c->parts.size(); ++i) {
                const tri_batch *p = c->parts[i];
                const char *field = nullptr;
                if (!p->rank_on) {
                        snprintf(why, sizeof why, "no ranker on part %zu (tri_batch_set_ranker)", i);
                        c->rank_why = why;
                        return TRI_OK;
                }
                if (p->rank.kind != p0->rank.kind)
                        field = "kind";
                else if (p->rank.topk != p0->rank.topk)
                        field = "topk";
                else if (p->rank.freq_cap != p0->rank.freq_cap)
                        field = "freq_cap";
                else if (p->rank.reserved != p0->rank.reserved)
                        field = "reserved";
                else if (memcmp(&p->rank.adjacency, &p0->rank.adjacency, sizeof(double)))
                        field = "adjacency";
                if (field) {
                        snprintf(why, sizeof why, "part %zu's ranker differs from part 0's in %s", i, field);
                        c->rank_why = why;
                        return TRI_OK;
                }
        }
        tri_dev *dev = p0->ix->dev;
        const size_t nq = p0->nq, n = c->parts.size(), k = p0->rank.topk;
        DevLock dev_lock(dev->mu);
        HIP_TRY(hipSetDevice(dev->device));
        if (c->rank_k != k) { // (no merge of an earlier run is in flight: tri_cbatch_sync waits for the one it queues)
                c->d_rank_docs.reset();
                c->d_rank_scores.reset();
                c->d_rank_counts.reset();
                c->rank_k = 0;
                HIP_TRY(c->d_rank_docs.alloc((nq * k + 1) * 4));
                HIP_TRY(c->d_rank_scores.alloc((nq * k + 1) * 8));
                HIP_TRY(c->d_rank_counts.alloc((nq + 1) * 4));
                c->rank_k = (uint32_t)k;
        }
        if (!c->d_rank_src)
                HIP_TRY(c->d_rank_src.alloc(n * sizeof(DevRankSource)));
        c->rank_src.resize(n);
        for (size_t i = 0; i < n; ++i)
                c->rank_src[i] = {c->parts[i]->d_rank_docs, c->parts[i]->d_rank_scores, c->parts[i]->d_rank_counts};
        HIP_TRY(hipMemcpyAsync(c->d_rank_src, c->rank_src.data(), n * sizeof(DevRankSource), hipMemcpyHostToDevice, dev->stream));
        c->ranked = true;
        return TRI_OK;
}

// ... and at tri_cbatch_sync, behind the last part's own sync: one lane per (query, source, rank) entry
static int cbatch_rank_merge(tri_cbatch *c) {
        if (!c->ranked)
                return TRI_OK;
        for (size_t i = 0; i < c->parts.size(); ++i) { // (a ranker replaced or removed between the run and the sync: the part ranked nothing under the table's block)
                const tri_batch *p = c->parts[i];
                if (!p->rank_on || p->d_rank_docs != c->rank_src[i].docs || (!p->rank_done && !p->tasks.empty())) {
                        c->ranked = false;
                        c->rank_why = "part " + std::to_string(i) + "'s ranker was replaced after tri_cbatch_run";
                        return TRI_OK;
                }
        }
        tri_dev *dev = c->parts[0]->ix->dev;
        const uint64_t lanes = (uint64_t)c->parts[0]->nq * c->parts.size() * c->rank_k;
        if (!lanes)
                return TRI_OK;
        DevLock dev_lock(dev->mu);
        HIP_TRY(hipSetDevice(dev->device));
        for (PooledEvent &e : c->rank_ev)
                if (!e)
                        HIP_TRY(e.take(dev));
        HIP_TRY(hipEventRecord(c->rank_ev[0], dev->stream));
        hipLaunchKernelGGL(k_rank_merge_sources, dim3((uint32_t)((lanes + AND_WG - 1) / AND_WG)), dim3(AND_WG), 0, dev->stream, (const DevRankSource *)c->d_rank_src,
                           (uint32_t)c->parts.size(), (uint32_t)c->parts[0]->nq, c->rank_k, c->d_rank_docs, c->d_rank_scores, c->d_rank_counts);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(c->rank_ev[1], dev->stream));
        c->rank_timed = true;
        return TRI_OK;
}

// tri_cbatch_ordered, at tri_cbatch_run: is the collection ordered for this run?  Every part carries an order, all of one topk and direction (each part's column
// is its own).  If so the merged block exists at that topk and the parts' table goes to the device on the engine stream, ahead of the merge tri_cbatch_sync
// queues.  If not — also: no part has an order — nothing is allocated, copied or launched.
static int cbatch_order_prepare(tri_cbatch *c) {
        c->ordered = false;
        const tri_batch *p0 = c->parts[0];
        bool any = false;
        for (const tri_batch *p : c->parts)
                any |= p->consumers[CONSUMER_ORDER].on;
        if (!any) {
                c->order_why = "no order is set on the parts (tri_batch_set_order)";
                return TRI_OK;
        }
        char why[160];
        for (size_t i = 0; i < c->parts.size(); ++i) {
                const tri_batch *p = c->parts[i];
                if (!p->consumers[CONSUMER_ORDER].on)
                        snprintf(why, sizeof why, "part %zu has no order (tri_batch_set_order)", i);
                else if (p->order.topk != p0->order.topk)
                        snprintf(why, sizeof why, "part %zu's order has topk %u, part 0's has %u", i, p->order.topk, p0->order.topk);
                else if (p->order.flip != p0->order.flip)
                        snprintf(why, sizeof why, "part %zu's order is %s, part 0's is not", i, p->order.flip ? "descending" : "ascending");
                else
                        continue;
                c->order_why = why;
                return TRI_OK;
        }
        tri_dev *dev = p0->ix->dev;
        const size_t nq = p0->nq, n = c->parts.size(), k = p0->order.topk;
        DevLock dev_lock(dev->mu);
        HIP_TRY(hipSetDevice(dev->device));
        if (c->order_k != k) { // (no merge of an earlier run is in flight: tri_cbatch_sync waits for the one it queues)
                c->d_order_keys.reset();
                c->d_order_counts.reset();
                c->order_k = 0;
                HIP_TRY(c->d_order_keys.alloc((nq * k + 1) * 8));
                HIP_TRY(c->d_order_counts.alloc((nq + 1) * 4));
                c->order_k = (uint32_t)k;
        }
        if (!c->d_order_src)
                HIP_TRY(c->d_order_src.alloc(n * sizeof(DevOrderLists)));
        c->order_src.resize(n);
        for (size_t i = 0; i < n; ++i)
                c->order_src[i] = {c->parts[i]->order_keys(c->parts[i]->order_lists), c->parts[i]->order_counts(c->parts[i]->order_lists)};
        HIP_TRY(hipMemcpyAsync(c->d_order_src, c->order_src.data(), n * sizeof(DevOrderLists), hipMemcpyHostToDevice, dev->stream));
        c->ordered = true;
        return TRI_OK;
}

// ... and at tri_cbatch_sync, behind the last part's own sync: a workgroup per query folds the parts' rows into the collection's
static int cbatch_order_merge(tri_cbatch *c) {
        if (!c->ordered)
                return TRI_OK;
        for (size_t i = 0; i < c->parts.size(); ++i) { // (an order replaced or removed between the run and the sync: the part selected nothing into the table's block)
                const tri_batch *p = c->parts[i];
                if (!p->consumers[CONSUMER_ORDER].on || !p->consumers[CONSUMER_ORDER].done || p->order_keys(p->order_lists) != c->order_src[i].keys) {
                        c->ordered = false;
                        c->order_why = "part " + std::to_string(i) + "'s order was replaced after tri_cbatch_run";
                        return TRI_OK;
                }
        }
        tri_dev *dev = c->parts[0]->ix->dev;
        const uint32_t nq = (uint32_t)c->parts[0]->nq;
        if (!nq)
                return TRI_OK;
        DevLock dev_lock(dev->mu);
        HIP_TRY(hipSetDevice(dev->device));
        hipLaunchKernelGGL(k_order_merge<true>, dim3(nq), dim3(ORDER_WG), 0, dev->stream, (const DevOrderLists *)c->d_order_src, DevOrderLists{nullptr, nullptr},
                           (const DevOrderGroup *)nullptr, (uint32_t)c->parts.size(), c->order_k, (uint64_t *)nullptr, (uint32_t *)nullptr, c->d_order_keys.get(), c->d_order_counts.get());
        HIP_TRY(hipGetLastError());
        return TRI_OK;
}

extern "C" int tri_cbatch_run(tri_cbatch *c) {
        if (!c)
                return fail(TRI_ERR_INVALID, "null collection batch");
        for (tri_batch *p : c->parts)
                if (int rc = tri_batch_run(p))
                        return rc;
        tri_dev *dev = c->parts[0]->ix->dev;
        const uint32_t nq = (uint32_t)c->parts[0]->nq;
        const uint32_t k = c->d_top_docs ? c->parts[0]->topk : 0u;
        if (nq) {
                hipLaunchKernelGGL(k_topk_merge_sources, dim3(std::min<uint32_t>(nq, (uint32_t)dev->cus * 8)), dim3(AND_WG), 0, dev->stream, c->d_src,
                                   (uint32_t)c->parts.size(), nq, k, c->d_top_docs, c->d_top_scores, c->d_top_counts, c->d_counts);
                HIP_TRY(hipGetLastError());
        }
        c->ran = true;
        c->synced = false;
        if (const int rc = cbatch_rank_prepare(c))
                return rc;
        return cbatch_order_prepare(c);
}

extern "C" int tri_cbatch_sync(tri_cbatch *c) {
        if (!c || !c->ran)
                return fail(TRI_ERR_INVALID, "tri_cbatch_sync: the collection batch has not been run");
        for (tri_batch *p : c->parts)
                if (int rc = tri_batch_sync(p))
                        return rc;
        if (int rc = cbatch_rank_merge(c)) // (a part's list stands once its own sync has run the WRITE and rank passes: behind the last of them)
                return rc;
        if (int rc = cbatch_order_merge(c))
                return rc;
        HIP_TRY(hipStreamSynchronize(c->parts[0]->ix->dev->stream));
        if (c->rank_timed) {
                float ms = 0;
                HIP_TRY(hipEventElapsedTime(&ms, c->rank_ev[0], c->rank_ev[1]));
                c->parts[0]->ix->dev->crank_merge_last_us = (uint64_t)(ms * 1000.0f);
                c->rank_timed = false;
        }
        c->synced = true;
        return TRI_OK;
}

// ------------------------------------------------------------------------------------------ multi-GPU result gather (RCCL)
// exec_query_par hands every source / shard its own result object and the caller combines them (exec.h:132-176).  With the queries
// sharded over one process per GPU, the fixed-shape result blocks of a batch — per-query match counts and, for top-K batches, the
// [nq][k] docID / score blocks and list lengths — are exchanged with ONE group of ncclAllGather calls on the engine stream, straight
// from the device buffers.  RCCL is bound at run time (dlopen): the library has no link-time dependency on it, and inside a process
// that already holds an RCCL (PyTorch's) the same one is used.
namespace {
        struct RcclApi {
                struct UniqueId {
                        char internal[128];
                };
                int (*GetUniqueId)(UniqueId *) = nullptr;
                int (*CommInitRank)(void **, int, UniqueId, int) = nullptr;
                int (*CommDestroy)(void *) = nullptr;
                int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
                int (*GroupStart)() = nullptr;
                int (*GroupEnd)() = nullptr;
                const char *(*GetErrorString)(int) = nullptr;
                bool ok = false;
        };
        RcclApi &rccl() {
                static RcclApi api;
                static bool tried = false;
                if (tried)
                        return api;
                tried = true;
                void *h = nullptr;
                for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
                        if ((h = dlopen(name, RTLD_NOW | RTLD_GLOBAL)))
                                break;
                if (!h)
                        return api;
                api.GetUniqueId = (decltype(api.GetUniqueId))dlsym(h, "ncclGetUniqueId");
                api.CommInitRank = (decltype(api.CommInitRank))dlsym(h, "ncclCommInitRank");
                api.CommDestroy = (decltype(api.CommDestroy))dlsym(h, "ncclCommDestroy");
                api.AllGather = (decltype(api.AllGather))dlsym(h, "ncclAllGather");
                api.GroupStart = (decltype(api.GroupStart))dlsym(h, "ncclGroupStart");
                api.GroupEnd = (decltype(api.GroupEnd))dlsym(h, "ncclGroupEnd");
                api.GetErrorString = (decltype(api.GetErrorString))dlsym(h, "ncclGetErrorString");
                api.ok = api.GetUniqueId && api.CommInitRank && api.CommDestroy && api.AllGather && api.GroupStart && api.GroupEnd;
                return api;
        }
        int nccl_fail(const char *what, int rc) { return fail(TRI_ERR_DEVICE, "%s: %s", what, rccl().GetErrorString ? rccl().GetErrorString(rc) : "RCCL error"); }
} // namespace

struct tri_comm {
        tri_dev *dev = nullptr;
        void *comm = nullptr;
        int rank = 0, nranks = 1;
        tri_allgather_fn custom = nullptr; // the caller's own transport instead of RCCL (tri_comm_create_custom)
        void *custom_user = nullptr;
};

extern "C" int tri_comm_unique_id(uint8_t id[128]) {
        if (!id)
                return fail(TRI_ERR_INVALID, "null argument");
        if (!rccl().ok)
                return fail(TRI_ERR_UNSUPPORTED, "librccl could not be loaded");
        RcclApi::UniqueId u;
        if (int rc = rccl().GetUniqueId(&u))
                return nccl_fail("ncclGetUniqueId", rc);
        memcpy(id, u.internal, 128);
        return TRI_OK;
}

extern "C" int tri_comm_create(tri_dev *dev, const uint8_t id[128], int rank, int nranks, tri_comm **out) {
        if (!dev || !id || !out || nranks < 1 || rank < 0 || rank >= nranks)
                return fail(TRI_ERR_INVALID, "tri_comm_create: bad argument");
        if (!rccl().ok)
                return fail(TRI_ERR_UNSUPPORTED, "librccl could not be loaded");
        HIP_TRY(hipSetDevice(dev->device));
        auto c = std::make_unique<tri_comm>();
        c->dev = dev;
        c->rank = rank;
        c->nranks = nranks;
        RcclApi::UniqueId u;
        memcpy(u.internal, id, 128);
        if (int rc = rccl().CommInitRank(&c->comm, nranks, u, rank))
                return nccl_fail("ncclCommInitRank", rc);
        *out = c.release();
        return TRI_OK;
}

extern "C" int tri_comm_create_custom(tri_dev *dev, int rank, int nranks, tri_allgather_fn allgather, void *user, tri_comm **out) {
        if (!dev || !out || !allgather || nranks < 1 || rank < 0 || rank >= nranks)
                return fail(TRI_ERR_INVALID, "tri_comm_create_custom: bad argument");
        auto c = std::make_unique<tri_comm>();
        c->dev = dev;
        c->rank = rank;
        c->nranks = nranks;
        c->custom = allgather;
        c->custom_user = user;
        *out = c.release();
        return TRI_OK;
}

extern "C" void tri_comm_destroy(tri_comm *c) {
        if (!c)
                return;
        if (c->comm && rccl().ok)
                rccl().CommDestroy(c->comm);
        delete c;
}

// every rank's blocks of batch b (same nq and topk on every rank) into [nranks][...] device buffers: counts_all u64[nranks][nq]; and for
// AccumulatedScore top-K batches docids_all u32[nranks][nq][k], scores_all f32[nranks][nq][k], topk_counts_all u32[nranks][nq] (NULL
// for the other modes).  Enqueued on the engine stream behind the batch's run; complete after tri_dev_sync / a stream wait.
extern "C" int tri_gather_results(tri_batch *b, tri_comm *c, void *counts_all, void *docids_all, void *scores_all, void *topk_counts_all) {
        if (!b || !c || !counts_all)
                return fail(TRI_ERR_INVALID, "null argument");
        if (b->ix->dev != c->dev)
                return fail(TRI_ERR_INVALID, "tri_gather_results: the batch and the communicator live on different device handles");
        const bool topk = (b->flags & TRI_FLAG_ACCUMULATED_SCORE) && b->topk;
        if (topk && (!docids_all || !scores_all || !topk_counts_all))
                return fail(TRI_ERR_INVALID, "tri_gather_results: a top-K batch needs all four receive buffers");
        tri_dev *dev = c->dev;
        HIP_TRY(hipSetDevice(dev->device));
        if (c->custom) { // the same blocks, the same [nranks][...] layout, over the caller's transport
                struct {
                        const void *send;
                        void *recv;
                        size_t bytes;
                } blocks[4] = {{b->d_qcounts, counts_all, b->nq * 8},
                               {topk ? b->d_top_docs : nullptr, docids_all, b->nq * b->topk * 4},
                               {topk ? b->d_top_scores : nullptr, scores_all, b->nq * b->topk * 4},
                               {topk ? b->d_top_counts : nullptr, topk_counts_all, b->nq * 4}};
                for (const auto &x : blocks)
                        if (x.send)
                                if (int rc = c->custom(c->custom_user, x.send, x.recv, x.bytes, (void *)dev->stream))
                                        return fail(TRI_ERR_DEVICE, "tri_gather_results: the caller's allgather returned %d", rc);
                return TRI_OK;
        }
        const RcclApi &R = rccl();
        const int U8 = 1; // ncclUint8: the blocks travel as bytes
        int rc = R.GroupStart();
        if (!rc)
                rc = R.AllGather(b->d_qcounts, counts_all, b->nq * 8, U8, c->comm, dev->stream);
        if (!rc && topk) {
                rc = R.AllGather(b->d_top_docs, docids_all, b->nq * b->topk * 4, U8, c->comm, dev->stream);
                if (!rc)
                        rc = R.AllGather(b->d_top_scores, scores_all, b->nq * b->topk * 4, U8, c->comm, dev->stream);
                if (!rc)
                        rc = R.AllGather(b->d_top_counts, topk_counts_all, b->nq * 4, U8, c->comm, dev->stream);
        }
        const int rc2 = R.GroupEnd();
        if (rc || rc2)
                return nccl_fail("ncclAllGather", rc ? rc : rc2);
        return TRI_OK;
}

// ------------------------------------------------------------------------------------------ write side
// the encoders, commit and merge on the device: tri_encode_*, tri_commit_*, tri_merge_* and the scratch they allocate from
#include "write_side.hpp"
#include "isect_side.hpp"
#include "perc_side.hpp"

#ifdef TRI_PROF
// perf-probe builds: read back and reset the per-phase cycle totals (dev_stream.hpp)
extern "C" int tri_debug_prof(uint64_t *out32) {
        unsigned long long h[32];
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_prof), sizeof h));
        for (int i = 0; i < 32; ++i)
                out32[i] = h[i];
        memset(h, 0, sizeof h);
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_prof), h, sizeof h));
        return TRI_OK;
}
#endif

// plane_cache.hpp — the index's plane cache: the term planes live with the index (they are a function of its lists alone).  Two parts:
//   * the rows' BOOKKEEPING (PlaneRows: which parts of which row have been built, the row tables, how a request grows the cache) — plain C++17 over
//     HostIndex, no HIP type: tests/cpp/plane_cache_plan_test.cpp compiles it with g++;
//   * the cache itself (PlaneCache: the device buffers, the growth on the upload stream, the pairs a run copies) — included by trinity_hip.hip behind owners.hpp
//     (the same translation unit), the one member of tri_index that holds any of this.
// Three moments write the cache: tri_batch_create (fit), run_plane_rows (missing_rows .. mark_built) and run_phrases (take_phrase_rows); every launch that takes
// planes reads its views.
#pragma once
#include "index_host.hpp"

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

// ------------------------------------------------------------------------------------------ the rows' bookkeeping (plain C++)
// the parts of a row, a bit each in PlaneRows::built: the part's build has been enqueued on the engine stream (every later kernel of the stream sees it)
enum RowPart : uint8_t {
        ROW_PLANE0 = 1, // plane 0: all a DocumentsOnly batch reads
        ROW_HIGH = 2,   // the high part (nested planes 1 .. 3 + level words): batches that read it (tri_batch::planes_hi)
        ROW_RANK = 4,   // k_phrase's rank path: the rank records over plane 0 (k_term_plane0, with plane 0) AND the hits entries of the row's postings (k_term_hits) —
                        // one run builds both, and nothing clears either: one bit
};
constexpr uint32_t ROW_NO_TERM = 0xffffffffu; // PlaneRowTables::rank_term of a rank that no term has

// How a request — plane_rows rows (row = df rank), with or without their high parts — grows a cache of `cap` rows: pure arithmetic over the five inputs.
struct PlaneGrowth {
        bool resize = false;    // every row buffer is replaced by one of `cap` rows (else: only the high region is new)
        bool new_high = false;  // a high region of `cap` rows is taken: the first batch that reads high parts, or the existing one resized with the rows —
                                // whether or not THIS batch reads it
        bool copy_rows = false; // plane 0, the rank records, the hits entries and their pairs move into the fresh buffers
        bool copy_high = false; // ... and so do the high parts
        uint32_t cap = 0;       // the capacity behind the growth
        size_t n_outgrown = 0;  // buffers the growth replaces, each retired on an event of its own: plane 0 + the four rank buffers, the high region
        bool nothing() const { return !resize && !new_high; }
};
inline PlaneGrowth plan_plane_growth(const uint32_t cap, const bool rows_exist, const bool high_exists, const uint32_t plane_rows, const bool needs_high) {
        const uint32_t want = std::max<uint32_t>(1, plane_rows);
        PlaneGrowth g;
        g.resize = want > cap;
        g.new_high = (needs_high || high_exists) && (g.resize || !high_exists);
        g.copy_rows = g.resize && rows_exist;
        g.copy_high = g.new_high && high_exists;
        g.cap = std::max(want, cap);
        g.n_outgrown = (g.copy_rows ? 5 : 0) + (g.copy_high ? 1 : 0);
        return g;
}

// the row tables of a cache of `cap` rows (k_phrase's rank path): sized for every row the cache can hold
struct PlaneRowTables {
        std::vector<uint32_t> rank_term; // [cap]: the term of df rank r (ROW_NO_TERM: none)
        std::vector<uint64_t> hs_off;    // [cap + 1]: prefix sums of the rows' document counts — a row's offset depends on the rows before it alone, so what was
                                         // built stays where it was when the cache grows
};
inline PlaneRowTables plane_row_tables(const HostIndex &ix, const uint32_t cap) {
        PlaneRowTables t;
        t.rank_term.assign(cap, ROW_NO_TERM);
        t.hs_off.assign((size_t)cap + 1, 0);
        for (size_t term = 0; term < ix.terms.size(); ++term)
                if (ix.df_rank[term] < cap)
                        t.rank_term[ix.df_rank[term]] = (uint32_t)term;
        for (uint32_t r = 0; r < cap; ++r)
                t.hs_off[r + 1] = t.hs_off[r] + (t.rank_term[r] != ROW_NO_TERM ? ix.terms[t.rank_term[r]].documents : 0u);
        return t;
}

// the phrase terms' rows whose hits entries a run builds (PlaneRows::take_phrase_rows)
struct PhraseRows {
        std::vector<uint32_t> pairs; // (term, row): each needs its rank records — with them plane 0 — and then its hits entries
        uint32_t max_blocks = 0;     // the longest of the lists, in blocks
        size_t first = 0;            // where the pairs go in the cache's pairs buffer, in pairs
};

struct PlaneRows {
        uint32_t cap = 0;           // rows; each region holds one all-zero row more (index cap)
        bool high = false;          // the high region exists
        std::vector<uint8_t> built; // [cap]: RowPart bits.  A row's parts move with every growth
        PlaneRowTables tab;
        size_t pairs_n = 0; // (term, row) pairs of the rows that have ROW_RANK, appended run after run (a row is built once: cap pairs at the most)

        PlaneGrowth plan(const uint32_t plane_rows, const bool needs_high) const { return plan_plane_growth(cap, cap != 0, high, plane_rows, needs_high); }
        // the growth is on its way (PlaneCache::fit): cannot fail
        void adopt(const PlaneGrowth &g, PlaneRowTables &&t) {
                if (g.resize)
                        tab = std::move(t);
                if (g.new_high && !g.copy_high)
                        for (uint8_t &b : built)
                                b &= (uint8_t)~ROW_HIGH; // (a fresh high region: no row has its high part yet)
                high = high || g.new_high;
                cap = g.cap;
                built.resize(cap, 0);
        }
        // run_plane_rows: the (term, row) pairs of the batch's plane terms whose row lacks a part the batch reads — with `rebuild` (option planes_rebuild) of all
        // of them —, and the bytes of their lists.  The caller marks them once their build is enqueued (mark_built)
        static uint8_t parts_read(const bool needs_high) { return needs_high ? ROW_PLANE0 | ROW_HIGH : ROW_PLANE0; }
        std::vector<uint32_t> missing_rows(const HostIndex &ix, const uint32_t *plane_terms, const size_t n, const bool needs_high, const bool rebuild, uint64_t &decoded_bytes) const {
                std::vector<uint32_t> pairs;
                const uint8_t needs = parts_read(needs_high);
                decoded_bytes = 0;
                for (size_t i = 0; i < n; ++i) {
                        const uint32_t term = plane_terms[i], row = ix.df_rank[term];
                        if (row < cap && ((built[row] & needs) != needs || rebuild)) {
                                pairs.push_back(term);
                                pairs.push_back(row);
                                decoded_bytes += ix.docbytes[term];
                        }
                }
                return pairs;
        }
        void mark_built(const std::vector<uint32_t> &pairs, const uint8_t parts) {
                for (size_t i = 1; i < pairs.size(); i += 2)
                        built[pairs[i]] |= parts;
        }
        // run_phrases: the phrase terms (lists of full blocks) whose row has no rank records and hits entries yet, each ONCE however often the batch names it —
        // so the rows are marked here, ahead of the enqueues, and their pairs counted
        PhraseRows take_phrase_rows(const HostIndex &ix, const uint32_t *pterms, const size_t n) {
                PhraseRows out;
                for (size_t i = 0; i < n; ++i) {
                        const uint32_t term = pterms[i], r = ix.df_rank[term];
                        if (r >= cap || (built[r] & ROW_RANK))
                                continue;
                        const DevTerm &t = ix.terms[term];
                        if (!(t.flags & TERM_FULL_BLOCKS) || !t.documents)
                                continue;
                        out.max_blocks = std::max(out.max_blocks, t.nblocks);
                        built[r] |= ROW_PLANE0 | ROW_RANK;
                        out.pairs.push_back(term);
                        out.pairs.push_back(r);
                }
                out.first = pairs_n;
                pairs_n += out.pairs.size() / 2;
                return out;
        }
};

// ------------------------------------------------------------------------------------------ the cache (HIP)
#if defined(__HIPCC__)
// Row r = the planes of the term of df rank r, built by k_term_planes the first time a batch's run wants them and kept — a caller that compiles a batch per
// step does not decode the same head terms step after step.  Two regions, built BY NEED (dev_structs.hpp: PL_HI): d_plane0 holds every row's PLANE 0 (plw
// words a row: all a DocumentsOnly batch reads), d_high the rows' HIGH parts (nested planes 1 .. 3 + level words, PL_HI * plw words a row) — allocated by the
// first scored batch that reads planes, a row's part built when such a batch names the row.  cap rows + one all-zero row (index cap) in each region: what a
// k_planes slot WITHOUT term planes reads (so its sweep needs no select).  Grown (rows moved on the upload stream) when a batch is planned with more eligible
// terms than it holds.
// ... and what k_phrase needs to find a head term's hits WITHOUT walking its blocks: per row a RANK DIRECTORY over plane 0 — a 64-byte record per docID group g
// of 256 documents at d_rank[(row * (plw / 8) + g) * 16]: the posting index of the group's first document and the group's eight plane-0 words, filled by
// k_term_plane0 —, and per posting the hits locator and frequency entry phrase_locate_block would compute (d_hits[hs_off[row] + posting]; k_term_hits; GOOGLE,
// lists of full blocks).  d_term_row[term] = its row once both are there.
// The width of a plane, plw, is a function of the segment alone (planner.hpp: eligible_planes, of max_doc): the first fit sets it for good.
class PlaneCache {
        PlaneRows rows;
        uint32_t plw_ = 0;
        Pooled<uint32_t> d_plane0, d_high; // (pooled, like the four below: tri_batch_create grows them without a device-wide synchronisation)
        Pooled<uint32_t> d_rank;
        DevMem<uint32_t> d_term_row;
        Pooled<unsigned long long> d_hits;
        Pooled<uint64_t> d_hs_off;
        Pooled<uint32_t> d_pairs; // the pairs of PlaneRows::pairs_n
        PooledEvent ev_ready;     // the last growth's move of the rows (upload stream): every run waits for it
        std::vector<std::pair<Pooled<void>, PooledEvent>> retired; // outgrown row buffers and the upload-stream point their last readers precede

        // everything a growth takes, in local owners until adopt()
        struct Fresh {
                Pooled<uint32_t> plane0, high, pairs, rank;
                Pooled<unsigned long long> hits;
                Pooled<uint64_t> hs_off;
                DevMem<uint32_t> term_row;
                PooledEvent drained, ready;
                std::vector<PooledEvent> retire;
        };
        // a row's bytes in plane 0, in the high region and in the rank directory
        static size_t row_bytes(const uint32_t plw) { return (size_t)plw * 4; }
        static size_t high_bytes(const uint32_t plw) { return (size_t)PL_HI * plw * 4; }
        static size_t rank_bytes(const uint32_t plw) { return (size_t)(plw / 8) * PL_RANK_WORDS * 4; }

        // ---- fit's stages, in call order
        // rows whose readers are through go back to the pool: no call here waits for the device
        void drop_retired() {
                for (size_t i = 0; i < retired.size();)
                        if (hipEventQuery(retired[i].second) == hipSuccess)
                                retired.erase(retired.begin() + (long)i);
                        else
                                ++i;
        }
        // every buffer and event first
        int take(tri_dev *dev, const HostIndex &ix, const uint32_t plw, const PlaneGrowth &g, const PlaneRowTables &t, Fresh &f) const {
                hipError_t e = hipSuccess;
                auto buf = [&](auto &b, const size_t bytes) { e = e == hipSuccess ? b.alloc(dev, bytes) : e; };
                if (g.resize)
                        buf(f.plane0, ((size_t)g.cap + 1) * row_bytes(plw) + 64);
                if (g.new_high)
                        buf(f.high, ((size_t)g.cap + 1) * high_bytes(plw) + 64);
                if (g.resize) {
                        buf(f.pairs, (size_t)g.cap * 8 + POOL_MIN_BYTES);
                        buf(f.rank, (size_t)g.cap * rank_bytes(plw) + 64);
                        buf(f.hits, (t.hs_off[g.cap] + 8) * 8);
                        buf(f.hs_off, ((size_t)g.cap + 1) * 8 + POOL_MIN_BYTES);
                        if (e == hipSuccess && !d_term_row)
                                e = f.term_row.alloc((ix.terms.size() + 1) * 4);
                }
                if (e == hipSuccess)
                        e = f.drained.take(dev);
                if (e == hipSuccess && !ev_ready)
                        e = f.ready.take(dev);
                f.retire.resize(g.n_outgrown);
                for (PooledEvent &r : f.retire)
                        if (e == hipSuccess)
                                e = r.take(dev);
                if (e != hipSuccess)
                        return fail(e == hipErrorOutOfMemory ? TRI_ERR_NOMEM : TRI_ERR_DEVICE, "tri_batch_create: growing the plane cache: %s", hipGetErrorString(e));
                return TRI_OK;
        }
        // then the rows move: from the cache's buffers, which stay in place, into the fresh ones
        int move(tri_dev *dev, const HostIndex &ix, const uint32_t plw, const PlaneGrowth &g, const PlaneRowTables &t, Fresh &f) const {
                HIP_TRY(hipEventRecord(f.drained, dev->stream));
                HIP_TRY(hipStreamWaitEvent(dev->stream_up, f.drained, 0));
                if (f.plane0) {
                        if (g.copy_rows)
                                HIP_TRY(hipMemcpyAsync(f.plane0, d_plane0, (size_t)rows.cap * row_bytes(plw), hipMemcpyDeviceToDevice, dev->stream_up));
                        HIP_TRY(hipMemsetAsync((uint8_t *)f.plane0.get() + (size_t)g.cap * row_bytes(plw), 0, row_bytes(plw) + 64, dev->stream_up));
                }
                if (f.high) {
                        if (g.copy_high)
                                HIP_TRY(hipMemcpyAsync(f.high, d_high, (size_t)rows.cap * high_bytes(plw), hipMemcpyDeviceToDevice, dev->stream_up));
                        HIP_TRY(hipMemsetAsync((uint8_t *)f.high.get() + (size_t)g.cap * high_bytes(plw), 0, high_bytes(plw) + 64, dev->stream_up));
                }
                if (g.resize) {
                        if (g.copy_rows) {
                                HIP_TRY(hipMemcpyAsync(f.pairs, d_pairs, rows.pairs_n * 8, hipMemcpyDeviceToDevice, dev->stream_up));
                                HIP_TRY(hipMemcpyAsync(f.rank, d_rank, (size_t)rows.cap * rank_bytes(plw), hipMemcpyDeviceToDevice, dev->stream_up));
                                HIP_TRY(hipMemcpyAsync(f.hits, d_hits, rows.tab.hs_off[rows.cap] * 8, hipMemcpyDeviceToDevice, dev->stream_up));
                        }
                        HIP_TRY(hipMemcpyAsync(f.hs_off, t.hs_off.data(), ((size_t)g.cap + 1) * 8, hipMemcpyHostToDevice, dev->stream_up)); // (t outlives the copy: adopt keeps it)
                        if (f.term_row)
                                HIP_TRY(hipMemsetAsync(f.term_row, 0xff, (ix.terms.size() + 1) * 4, dev->stream_up));
                }
                HIP_TRY(hipEventRecord(f.ready ? f.ready : ev_ready, dev->stream_up));
                // the buffers this growth replaces are retired on events recorded on the UPLOAD stream, behind the copies that read them — that point is past
                // the engine stream's earlier readers too (stream_up waits for `drained`); an event recorded on the engine stream BEFORE the copies were enqueued
                // would let the next tri_batch_create pool a buffer the copy had not read yet
                for (PooledEvent &r : f.retire)
                        HIP_TRY(hipEventRecord(r, dev->stream_up));
                return TRI_OK;
        }
        // nothing here can fail: the cache takes the fresh buffers, and what a member held is retired on the next event
        void adopt(tri_dev *dev, const uint32_t plw, const PlaneGrowth &g, PlaneRowTables &&t, Fresh &f) {
                size_t nret = 0;
                auto swap_in = [&](auto &member, auto &with) {
                        if (member)
                                retired.emplace_back(Pooled<void>(member.release(), FreePooled{dev}), std::move(f.retire[nret++]));
                        member = std::move(with);
                };
                if (g.resize) {
                        swap_in(d_rank, f.rank), swap_in(d_hits, f.hits), swap_in(d_hs_off, f.hs_off), swap_in(d_pairs, f.pairs);
                        swap_in(d_plane0, f.plane0);
                        if (f.term_row)
                                d_term_row = std::move(f.term_row);
                }
                if (g.new_high)
                        swap_in(d_high, f.high);
                if (f.ready)
                        ev_ready = std::move(f.ready);
                plw_ = plw; // (the first fit sets it; every later one found it the same)
                rows.adopt(g, std::move(t));
        }

public:
        // ---- the views the launches pass (device pointers: the kernels that build a row's parts write through them)
        uint32_t *plane0() const { return d_plane0; }
        uint32_t *high() const { return d_high; }
        uint32_t *rank() const { return d_rank; }
        unsigned long long *hits() const { return d_hits; }
        uint64_t *hits_off() const { return d_hs_off; }
        uint32_t *term_row() const { return d_term_row; }
        uint32_t cap() const { return rows.cap; } // (also the index of the all-zero row)
        uint32_t plw() const { return plw_; }
        hipEvent_t ready() const { return ev_ready; } // null: never grown

        // The cache holds a row for every term the batch could name (row = df rank < plane_rows), plus an all-zero row: what a
        // k_planes slot WITHOUT term planes reads (so its sweep needs no select).  Grown WITHOUT draining the engine stream (synchronising it
        // here would be a stall in the serving loop whenever a batch was planned with more eligible terms): the rows move on the upload stream behind
        // everything the engine stream holds so far (runs that read or build the old rows), later runs wait for the move's event (tri_batch_run),
        // and the old buffers are retired — pooled again once that point has passed.  Everything a growth needs is taken before the cache is
        // touched, in local owners, and the cache's members change hands behind the last call that can fail: an error anywhere leaves the index as it was and
        // hands back what was taken.
        int fit(tri_dev *dev, const HostIndex &ix, const uint32_t plane_rows, const uint32_t plw, const bool needs_high) {
                drop_retired();
                if (rows.cap && plw != plw_)
                        return fail(TRI_ERR_INVALID, "tri_batch_create: a plan of %u words a plane on an index whose plane cache holds rows of %u", plw, plw_);
                const PlaneGrowth g = rows.plan(plane_rows, needs_high);
                if (g.nothing())
                        return TRI_OK;
                PlaneRowTables t;
                if (g.resize)
                        t = plane_row_tables(ix, g.cap);
                Fresh f;
                if (const int rc = take(dev, ix, plw, g, t, f))
                        return rc;
                if (const int rc = move(dev, ix, plw, g, t, f)) {
                        hipStreamSynchronize(dev->stream_up); // (the fresh buffers go back to the pool: no copy queued above may still be writing them)
                        return rc;
                }
                adopt(dev, plw, g, std::move(t), f);
                return TRI_OK;
        }

        // run_plane_rows: the (term, row) pairs of the rows this run must build (PlaneRows::missing_rows); once their build is enqueued, mark_built() marks them
        std::vector<uint32_t> missing_rows(const HostIndex &ix, const uint32_t *plane_terms, const size_t n, const bool needs_high, const bool rebuild, uint64_t &decoded_bytes) const {
                return rows.missing_rows(ix, plane_terms, n, needs_high, rebuild, decoded_bytes);
        }
        void mark_built(const std::vector<uint32_t> &pairs, const bool needs_high) { rows.mark_built(pairs, PlaneRows::parts_read(needs_high)); }
        // run_phrases (GOOGLE): the pairs of the phrase terms' rows that lack ROW_RANK (PlaneRows::take_phrase_rows), appended to the pairs buffer on
        // `stream`; *d_pairs = where they lie on the device
        int phrase_rows(const HostIndex &ix, const uint32_t *pterms, const size_t n, const hipStream_t stream, PhraseRows &out, const uint32_t **d_out) {
                out = rows.cap ? rows.take_phrase_rows(ix, pterms, n) : PhraseRows{};
                *d_out = d_pairs + 2 * out.first; // (every row is built once: the pairs of all runs fit 2 * cap words)
                if (!out.pairs.empty())
                        HIP_TRY(hipMemcpyAsync(d_pairs + 2 * out.first, out.pairs.data(), out.pairs.size() * 4, hipMemcpyHostToDevice, stream)); // (pageable source: staged before the call returns)
                return TRI_OK;
        }
};
#endif

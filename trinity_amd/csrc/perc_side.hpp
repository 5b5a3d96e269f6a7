// perc_side.hpp — tri_perc_*: the percolator (percolator.h:1-60, percolator.cpp:5-137).  A set of stored queries lowered once (host/perc_lower.hpp) and resident
// in one pooled block; a call uploads a batch of documents and launches k_perc.hpp's stages.  Included at the end of trinity_hip.hip: the same translation unit.
#pragma once
#include "host/perc_lower.hpp"

struct tri_perc {
        DevRef dev; // (first: released after the block below)
        Pooled<uint8_t> block;
        PercSet S{};
        perc::Lowered L; // recs / qleaves are dropped after the upload; status, qflags, term_leaf and the phrases stay (the host sizes a call's rows from them)
        std::vector<uint32_t> seen; // per leaf: the call that last saw it (tri_perc_match: an exact count of the rows the call builds)
        uint32_t call = 0;
        uint64_t device_bytes = 0;
        uint32_t *d_qflags = nullptr;
};
struct tri_perc_result {
        std::vector<uint32_t> q_by_q, d_by_q, q_by_d, d_by_d, dstart; // both orders; dstart[ndocs + 1]: where a document's run begins
        tri_perc_result_info info{};
};

namespace {
        inline uint64_t perc_up(const uint64_t x) { return (x + 255u) & ~(uint64_t)255u; }
        inline uint32_t perc_blocks(const uint64_t n, const uint32_t per) { return (uint32_t)std::max<uint64_t>(1, (n + per - 1) / per); }

        // exclusive scan of in[0 .. n) into out (in == out is fine); tmp: perc_blocks(n, PERC_SCAN_BLOCK) words; total: two words, the sum as 64 bits
        template <bool NZ>
        int perc_scan(hipStream_t st, const uint32_t *in, uint32_t *out, const uint32_t n, uint32_t *tmp, uint32_t *total) {
                const uint32_t nb = perc_blocks(n, PERC_SCAN_BLOCK);
                hipLaunchKernelGGL(k_perc_scan_sums<NZ>, dim3(nb), dim3(PERC_WG), 0, st, in, n, tmp);
                hipLaunchKernelGGL(k_perc_scan_tops, dim3(1), dim3(PERC_WG), 0, st, tmp, nb, total);
                hipLaunchKernelGGL(k_perc_scan_apply<NZ>, dim3(nb), dim3(PERC_WG), 0, st, in, n, (const uint32_t *)tmp, out);
                HIP_TRY(hipGetLastError());
                return TRI_OK;
        }
} // namespace

extern "C" int tri_perc_create(tri_dev *dev, const uint32_t *prog, size_t prog_len, const tri_query *queries, size_t nq, uint32_t nterms, tri_perc **out) {
        if (!dev || !out || (!prog && prog_len) || (!queries && nq))
                return fail(TRI_ERR_INVALID, "tri_perc_create: null argument");
        if (nq >= 0x7fffffffu)
                return fail(TRI_ERR_INVALID, "tri_perc_create: %zu queries (fewer than 2^31 a set)", nq);
        auto h = std::make_unique<tri_perc>();
        std::string err;
        if (const int rc = perc::lower(prog, prog_len, queries, nq, nterms, h->L, err))
                return fail(rc, "%s", err.c_str());
        if (!err.empty())
                fail(TRI_ERR_UNSUPPORTED, "%s", err.c_str()); // (the last query left out: tri_last_error describes it, as after tri_batch_create)
        perc::Lowered &L = h->L;
        HIP_TRY(hipSetDevice(dev->device));
        const std::vector<uint32_t> *parts[] = {&L.recs, &L.rec_off, &L.qflags, &L.qleaf_first, &L.qleaves, &L.term_leaf, &L.leaf_term, &L.phrase_first, &L.phrase_leaves};
        uint64_t off[10] = {0};
        for (int i = 0; i < 9; ++i)
                off[i + 1] = off[i] + perc_up(parts[i]->size() * 4 + 16); // (+ 16: a table of no entries still has an address of its own)
        h->dev.retain(dev);
        HIP_TRY(h->block.alloc(dev, std::max<uint64_t>(off[9], POOL_MIN_BYTES)));
        h->device_bytes = off[9];
        hipStream_t st = dev->stream;
        const uint32_t *d[9];
        for (int i = 0; i < 9; ++i) {
                d[i] = reinterpret_cast<const uint32_t *>(h->block + off[i]);
                if (!parts[i]->empty())
                        HIP_TRY(hipMemcpyAsync(h->block + off[i], parts[i]->data(), parts[i]->size() * 4, hipMemcpyHostToDevice, st));
        }
        HIP_TRY(hipStreamSynchronize(st));
        h->S = PercSet{d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], (uint32_t)nq, nterms, (uint32_t)L.leaf_term.size(), (uint32_t)L.phrase_first.size() - 1u};
        h->d_qflags = reinterpret_cast<uint32_t *>(h->block + off[2]);
        h->seen.assign(L.leaf_term.size(), 0u);
        std::vector<uint32_t>().swap(L.recs);
        std::vector<uint32_t>().swap(L.qleaves);
        std::vector<uint32_t>().swap(L.qleaf_first);
        *out = h.release();
        return TRI_OK;
}

extern "C" int tri_perc_query_status(const tri_perc *h, int32_t *status) {
        if (!h || !status)
                return fail(TRI_ERR_INVALID, "tri_perc_query_status: null argument");
        std::copy(h->L.status.begin(), h->L.status.end(), status);
        return TRI_OK;
}

extern "C" int tri_perc_set_enabled(tri_perc *h, const uint32_t *queries, size_t n, int enabled) {
        if (!h || (!queries && n))
                return fail(TRI_ERR_INVALID, "tri_perc_set_enabled: null argument");
        for (size_t i = 0; i < n; ++i)
                if (queries[i] >= h->S.nq)
                        return fail(TRI_ERR_INVALID, "tri_perc_set_enabled: query %u of a set of %u", queries[i], h->S.nq);
        if (!n)
                return TRI_OK;
        for (size_t i = 0; i < n; ++i)
                h->L.qflags[queries[i]] = (h->L.qflags[queries[i]] & ~perc::Q_ENABLED) | (enabled ? perc::Q_ENABLED : 0u);
        HIP_TRY(hipSetDevice(h->dev->device));
        HIP_TRY(hipMemcpyAsync(h->d_qflags, h->L.qflags.data(), h->L.qflags.size() * 4, hipMemcpyHostToDevice, h->dev->stream));
        HIP_TRY(hipStreamSynchronize(h->dev->stream));
        return TRI_OK;
}

extern "C" int tri_perc_get_info(const tri_perc *h, tri_perc_info *info) {
        if (!h || !info)
                return fail(TRI_ERR_INVALID, "tri_perc_get_info: null argument");
        *info = tri_perc_info{};
        info->queries = h->S.nq;
        info->unsupported = h->L.unsupported;
        info->terms = h->S.nT;
        info->phrases = h->S.nP;
        info->device_bytes = h->device_bytes;
        info->nterms = h->S.nterms;
        return TRI_OK;
}

extern "C" void tri_perc_destroy(tri_perc *h) { delete h; }

extern "C" int tri_perc_match(tri_perc *h, const tri_perc_docs *docs, tri_perc_result **out) {
        if (!h || !docs || !out)
                return fail(TRI_ERR_INVALID, "tri_perc_match: null argument");
        const auto t_begin = std::chrono::steady_clock::now();
        std::string err;
        if (const int rc = perc::check_docs(docs, h->S.nterms, err))
                return fail(rc, "%s", err.c_str());
        tri_dev *dev = h->dev;
        const PercSet &S = h->S;
        const uint32_t ndocs = docs->ndocs, W = (ndocs + 31u) / 32u, nT = S.nT, nP = S.nP, nL = nT + nP, nq = S.nq;
        const uint64_t p0 = docs->doc_first[0], np64 = docs->doc_first[ndocs] - p0;
        // the rows the call builds, exactly: the term leaves among the batch's terms, the phrases all of whose words are among them; and the positions the postings name
        uint64_t npos = 0;
        uint32_t term_rows = 0, phrase_rows = 0;
        if (!++h->call) { // (the counter wrapped)
                std::fill(h->seen.begin(), h->seen.end(), 0u);
                h->call = 1;
        }
        for (uint64_t i = 0; i < np64; ++i) {
                npos += docs->freqs[p0 + i];
                const uint32_t t = docs->terms[p0 + i];
                const uint32_t l = t == perc::NONE ? perc::NONE : h->L.term_leaf[t];
                if (l != perc::NONE && h->seen[l] != h->call) {
                        h->seen[l] = h->call;
                        ++term_rows;
                }
        }
        for (uint32_t p = 0; p < nP; ++p) {
                bool all = true;
                for (uint32_t k = h->L.phrase_first[p]; k < h->L.phrase_first[p + 1] && all; ++k)
                        all = h->seen[h->L.phrase_leaves[k]] == h->call;
                phrase_rows += all;
        }
        if (np64 >= 0xffffffffull || npos >= 0xffffffffull)
                return fail(TRI_ERR_UNSUPPORTED, "tri_perc_match: %llu postings, %llu positions (fewer than 2^32 a call: split it)", (unsigned long long)np64, (unsigned long long)npos);
        const uint32_t np = (uint32_t)np64, nrows = term_rows + phrase_rows;
        const uint64_t max_bytes = dev->opt.perc_max_bytes;
        HIP_TRY(hipSetDevice(dev->device));
        hipStream_t st = dev->stream;

        // ---- scratch, block 1: the batch, the rows, the leaf and query tables of the call
        const uint32_t scan_tmp = perc_blocks(std::max<uint64_t>({nL + 1ull, ndocs, nq}), PERC_SCAN_BLOCK);
        uint64_t o = 0;
        auto take = [&](const uint64_t bytes) {
                const uint64_t at = o;
                o += perc_up(bytes + 16);
                return at;
        };
        const uint64_t o_dfirst = take((ndocs + 1ull) * 4), o_terms = take(np * 4ull), o_freqs = take(np * 4ull), o_pos = take(npos * 2ull), o_pfirst = take(np * 4ull), o_dsum = take(ndocs * 4ull),
                       o_lflag = take(nL * 4ull), o_loff = take((nL + 1ull) * 4), o_lrow = take(nL * 4ull), o_plist = take(nP * 4ull), o_tmp = take(scan_tmp * 4ull), o_tot = take(64),
                       o_sel = take(nq * 4ull), o_seloff = take(nq * 4ull), o_cand = take(nq * 4ull), o_rows = take((uint64_t)nrows * W * 4), total1 = o;
        if (total1 > max_bytes)
                return fail(TRI_ERR_UNSUPPORTED, "tri_perc_match: %u documents, %u postings, %u rows of %u bytes, %u queries: %llu bytes of scratch exceed perc_max_bytes = %llu", ndocs, np, nrows, W * 4u,
                            nq, (unsigned long long)total1, (unsigned long long)max_bytes);
        auto R = std::make_unique<tri_perc_result>();
        tri_perc_result_info &I = R->info;
        I.ndocs = ndocs;
        R->dstart.assign(ndocs + 1, 0u);
        auto finish = [&]() {
                I.total_ms = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
                *out = R.release();
                return TRI_OK;
        };
        if (!nq)
                return finish();
        Pooled<uint8_t> s1, s2, s3;
        HIP_TRY(s1.alloc(dev, std::max<uint64_t>(total1, POOL_MIN_BYTES)));
        I.scratch_bytes = total1;
        PooledEvent ev[6];
        for (auto &e : ev)
                HIP_TRY(e.take(dev));
        auto u32 = [&](Pooled<uint8_t> &b, const uint64_t off) { return reinterpret_cast<uint32_t *>(b + off); };
        std::vector<uint32_t> dfirst(ndocs + 1);
        for (uint32_t d = 0; d <= ndocs; ++d)
                dfirst[d] = (uint32_t)(docs->doc_first[d] - p0);
        HIP_TRY(hipMemcpyAsync(s1 + o_dfirst, dfirst.data(), dfirst.size() * 4, hipMemcpyHostToDevice, st));
        if (np) {
                HIP_TRY(hipMemcpyAsync(s1 + o_terms, docs->terms + p0, np * 4ull, hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemcpyAsync(s1 + o_freqs, docs->freqs + p0, np * 4ull, hipMemcpyHostToDevice, st));
        }
        if (npos) { // (the positions of the call's postings begin where those of the postings before doc_first[0] end)
                uint64_t skip = 0;
                for (uint64_t i = 0; i < p0; ++i)
                        skip += docs->freqs[i];
                HIP_TRY(hipMemcpyAsync(s1 + o_pos, docs->positions + skip, npos * 2ull, hipMemcpyHostToDevice, st));
        }
        HIP_TRY(hipMemsetAsync(s1 + o_lflag, 0, nL * 4ull + 16, st));
        HIP_TRY(hipMemsetAsync(s1 + o_plist, 0, nP * 4ull + 16, st)); // (an entry the device does not fill names phrase 0: harmless, and never read when the counts agree)
        if (nrows)
                HIP_TRY(hipMemsetAsync(s1 + o_rows, 0, (uint64_t)nrows * W * 4, st)); // a smaller call after a bigger one sees no stale bit
        HIP_TRY(hipStreamSynchronize(st));                                            // (the host buffers are the caller's, and pageable: the copies have left them)
        const PercDocs D{u32(s1, o_dfirst), u32(s1, o_terms), u32(s1, o_freqs), reinterpret_cast<const uint16_t *>(s1 + o_pos), ndocs, W};
        uint32_t *leaf_flag = u32(s1, o_lflag), *leaf_off = u32(s1, o_loff), *leaf_row = u32(s1, o_lrow), *plist = u32(s1, o_plist), *tmp = u32(s1, o_tmp), *tot = u32(s1, o_tot);
        uint32_t *rows = u32(s1, o_rows), *pos_first = u32(s1, o_pfirst), *dsum = u32(s1, o_dsum), *sel = u32(s1, o_sel), *seloff = u32(s1, o_seloff), *cand = u32(s1, o_cand);

        // ---- rows
        HIP_TRY(hipEventRecord(ev[0], st));
        const uint32_t doc_blocks = perc_blocks(ndocs, PERC_WG / 64);
        hipLaunchKernelGGL(k_perc_docs, dim3(doc_blocks), dim3(PERC_WG), 0, st, D, S.term_leaf, S.nterms, leaf_flag, dsum);
        if (nP)
                hipLaunchKernelGGL(k_perc_phrase_flag, dim3(perc_blocks(nP, PERC_WG)), dim3(PERC_WG), 0, st, S, leaf_flag);
        HIP_TRY(hipGetLastError());
        if (const int rc = perc_scan<false>(st, dsum, dsum, ndocs, tmp, tot + 2))
                return rc;
        if (nL) {
                // (leaf_off has nL + 1 entries and leaf_flag[nL] is 0: leaf_off[nT] exists when the set has no phrase)
                if (const int rc = perc_scan<false>(st, leaf_flag, leaf_off, nL + 1u, tmp, tot))
                        return rc;
                hipLaunchKernelGGL(k_perc_leaf_rows, dim3(perc_blocks(nL, PERC_WG)), dim3(PERC_WG), 0, st, (const uint32_t *)leaf_flag, (const uint32_t *)leaf_off, nT, nL, nrows, leaf_row, plist);
        }
        hipLaunchKernelGGL(k_perc_rows, dim3(doc_blocks), dim3(PERC_WG), 0, st, D, S.term_leaf, S.nterms, (const uint32_t *)leaf_row, (const uint32_t *)dsum, pos_first, rows);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev[1], st));
        // ---- phrases
        if (phrase_rows) {
                const uint64_t tasks = (uint64_t)phrase_rows * W;
                hipLaunchKernelGGL(k_perc_phrases, dim3((uint32_t)std::min<uint64_t>(perc_blocks(tasks, PERC_WG / 64), 1u << 20)), dim3(PERC_WG), 0, st, S, D, (const uint32_t *)leaf_row,
                                   (const uint32_t *)plist, phrase_rows, (const uint32_t *)pos_first, rows);
                HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(ev[2], st));
        // ---- the prune: the candidates, ascending
        hipLaunchKernelGGL(k_perc_select, dim3(perc_blocks(nq, PERC_WG)), dim3(PERC_WG), 0, st, S, (const uint32_t *)leaf_row, (uint32_t)(dev->opt.perc_prune != 0), sel);
        HIP_TRY(hipGetLastError());
        if (const int rc = perc_scan<false>(st, sel, seloff, nq, tmp, tot + 4))
                return rc;
        hipLaunchKernelGGL(k_perc_compact, dim3(perc_blocks(nq, PERC_WG)), dim3(PERC_WG), 0, st, (const uint32_t *)sel, (const uint32_t *)seloff, nq, cand, nq);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev[3], st));
        uint32_t counts[8] = {0};
        HIP_TRY(hipMemcpyAsync(counts, tot, sizeof counts, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const uint32_t ncand = counts[4];
        I.leaf_rows = term_rows;
        I.phrase_rows = phrase_rows;
        I.evaluated = ncand;
        if (nL && counts[0] != nrows)
                return fail(TRI_ERR_INTERNAL, "tri_perc_match: the device built %u rows, the host counted %u", counts[0], nrows);
        auto stage_ms = [&](const int a, const int b) {
                float ms = 0.f;
                (void)hipEventElapsedTime(&ms, ev[a], ev[b]);
                return ms;
        };
        I.rows_ms = stage_ms(0, 1), I.phrases_ms = stage_ms(1, 2), I.select_ms = stage_ms(2, 3);
        if (!ncand)
                return finish();

        // ---- block 2: the candidates' match words and counts; the fold
        o = 0;
        const uint64_t o_mw = take((uint64_t)ncand * W * 4), o_qcount = take(ncand * 4ull), o_qoff = take(ncand * 4ull), o_hitoff = take(ncand * 4ull), o_hits = take(ncand * 4ull),
                       o_tmp2 = take(perc_blocks(ncand, PERC_SCAN_BLOCK) * 4ull), o_tot2 = take(64), total2 = o;
        if (total1 + total2 > max_bytes)
                return fail(TRI_ERR_UNSUPPORTED, "tri_perc_match: %u candidate queries of %u match words bring the call's scratch to %llu bytes: above perc_max_bytes = %llu", ncand, W,
                            (unsigned long long)(total1 + total2), (unsigned long long)max_bytes);
        HIP_TRY(s2.alloc(dev, std::max<uint64_t>(total2, POOL_MIN_BYTES)));
        I.scratch_bytes += total2;
        uint32_t *mw = u32(s2, o_mw), *qcount = u32(s2, o_qcount), *qoff = u32(s2, o_qoff), *hitoff = u32(s2, o_hitoff), *hits = u32(s2, o_hits), *tmp2 = u32(s2, o_tmp2), *tot2 = u32(s2, o_tot2);
        HIP_TRY(hipMemsetAsync(qcount, 0, ncand * 4ull, st));
        HIP_TRY(hipEventRecord(ev[3], st));
        const uint32_t tiles = (W + PERC_TILE_WORDS - 1) / PERC_TILE_WORDS;
        const uint32_t stack_words = std::min(std::max(h->L.stack_max, 1u), TREE_WIDE_STACK);
        hipLaunchKernelGGL(k_perc_eval, dim3((uint32_t)std::min<uint64_t>((uint64_t)ncand * tiles, 1u << 22)), dim3(64), stack_words * 64u * 4u, st, S, (const uint32_t *)cand, ncand,
                           (const uint32_t *)leaf_row, (const uint32_t *)rows, ndocs, W, stack_words, mw, qcount);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev[4], st));
        // ---- compaction: the queries that hit, where each one's pairs begin
        if (const int rc = perc_scan<true>(st, qcount, hitoff, ncand, tmp2, tot2))
                return rc;
        if (const int rc = perc_scan<false>(st, qcount, qoff, ncand, tmp2, tot2 + 2))
                return rc;
        hipLaunchKernelGGL(k_perc_compact, dim3(perc_blocks(ncand, PERC_WG)), dim3(PERC_WG), 0, st, (const uint32_t *)qcount, (const uint32_t *)hitoff, ncand, hits, ncand);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(counts, tot2, 16, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const uint32_t nhit = counts[0];
        const uint64_t npairs = counts[2] | (uint64_t)counts[3] << 32;
        I.hit_queries = nhit;
        I.pairs = npairs;
        I.eval_ms = stage_ms(3, 4);
        if (npairs >= 0xffffffffull)
                return fail(TRI_ERR_UNSUPPORTED, "tri_perc_match: %llu pairs (fewer than 2^32 a call: split it)", (unsigned long long)npairs);
        if (!npairs)
                return finish();

        // ---- block 3: the pairs in both orders
        const uint32_t nseg = perc_blocks(nhit, PERC_SEG), np32 = (uint32_t)npairs;
        const uint64_t nsegcnt = (uint64_t)W * 32u * nseg;
        if (nsegcnt >= 0xffffffffull)
                return fail(TRI_ERR_UNSUPPORTED, "tri_perc_match: %u queries hit on %u documents (split the call)", nhit, ndocs);
        o = 0;
        const uint64_t o_seg = take(nsegcnt * 4), o_tmp3 = take(perc_blocks(nsegcnt, PERC_SCAN_BLOCK) * 4ull), o_tot3 = take(64), o_qq = take(npairs * 4), o_qd = take(npairs * 4), o_dq = take(npairs * 4),
                       o_dd = take(npairs * 4), o_dstart = take((ndocs + 1ull) * 4), total3 = o;
        if (total1 + total2 + total3 > max_bytes)
                return fail(TRI_ERR_UNSUPPORTED, "tri_perc_match: %llu pairs bring the call's scratch to %llu bytes: above perc_max_bytes = %llu", (unsigned long long)npairs,
                            (unsigned long long)(total1 + total2 + total3), (unsigned long long)max_bytes);
        HIP_TRY(s3.alloc(dev, std::max<uint64_t>(total3, POOL_MIN_BYTES)));
        I.scratch_bytes += total3;
        uint32_t *seg = u32(s3, o_seg);
        const uint32_t seg_blocks = perc_blocks((uint64_t)nseg * W, PERC_WG / 64);
        hipLaunchKernelGGL(k_perc_fill_q, dim3(std::min(perc_blocks(nhit, PERC_WG / 64), 1u << 20)), dim3(PERC_WG), 0, st, (const uint32_t *)cand, (const uint32_t *)hits, nhit, (const uint32_t *)qoff,
                           (const uint32_t *)mw, W, np32, u32(s3, o_qq), u32(s3, o_qd));
        hipLaunchKernelGGL(k_perc_seg_count, dim3(seg_blocks), dim3(PERC_WG), 0, st, (const uint32_t *)hits, nhit, (const uint32_t *)mw, W, nseg, seg);
        HIP_TRY(hipGetLastError());
        if (const int rc = perc_scan<false>(st, seg, seg, (uint32_t)nsegcnt, u32(s3, o_tmp3), u32(s3, o_tot3)))
                return rc;
        hipLaunchKernelGGL(k_perc_fill_d, dim3(seg_blocks), dim3(PERC_WG), 0, st, (const uint32_t *)cand, (const uint32_t *)hits, nhit, (const uint32_t *)mw, W, nseg, (const uint32_t *)seg, np32,
                           u32(s3, o_dq), u32(s3, o_dd));
        hipLaunchKernelGGL(k_perc_doc_starts, dim3(perc_blocks(ndocs + 1ull, PERC_WG)), dim3(PERC_WG), 0, st, (const uint32_t *)seg, nseg, ndocs, W, np32, u32(s3, o_dstart));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev[5], st));
        R->q_by_q.resize(np32), R->d_by_q.resize(np32), R->q_by_d.resize(np32), R->d_by_d.resize(np32);
        HIP_TRY(hipMemcpyAsync(R->q_by_q.data(), s3 + o_qq, npairs * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(R->d_by_q.data(), s3 + o_qd, npairs * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(R->q_by_d.data(), s3 + o_dq, npairs * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(R->d_by_d.data(), s3 + o_dd, npairs * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(R->dstart.data(), s3 + o_dstart, (ndocs + 1ull) * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        I.compact_ms = stage_ms(4, 5);
        return finish();
}

extern "C" int tri_perc_result_pairs(const tri_perc_result *r, int order, uint32_t *queries, uint32_t *docs, size_t cap, size_t *n) {
        if (!r || !n || (!queries != !docs))
                return fail(TRI_ERR_INVALID, "tri_perc_result_pairs: null argument");
        if (order != TRI_PERC_BY_QUERY && order != TRI_PERC_BY_DOCUMENT)
                return fail(TRI_ERR_INVALID, "tri_perc_result_pairs: order %d (TRI_PERC_BY_QUERY or TRI_PERC_BY_DOCUMENT)", order);
        const size_t have = r->q_by_q.size();
        if (queries) {
                if (cap < have)
                        return fail(TRI_ERR_INVALID, "tri_perc_result_pairs: %zu pairs, room for %zu", have, cap);
                const bool by_q = order == TRI_PERC_BY_QUERY;
                std::copy_n((by_q ? r->q_by_q : r->q_by_d).begin(), have, queries);
                std::copy_n((by_q ? r->d_by_q : r->d_by_d).begin(), have, docs);
        }
        *n = have;
        return TRI_OK;
}

extern "C" int tri_perc_result_doc_counts(const tri_perc_result *r, uint32_t *counts) {
        if (!r || !counts)
                return fail(TRI_ERR_INVALID, "tri_perc_result_doc_counts: null argument");
        for (uint32_t d = 0; d < r->info.ndocs; ++d)
                counts[d] = r->dstart[d + 1] - r->dstart[d];
        return TRI_OK;
}

extern "C" int tri_perc_result_get_info(const tri_perc_result *r, tri_perc_result_info *info) {
        if (!r || !info)
                return fail(TRI_ERR_INVALID, "tri_perc_result_get_info: null argument");
        *info = r->info;
        return TRI_OK;
}

extern "C" void tri_perc_result_destroy(tri_perc_result *r) { delete r; }

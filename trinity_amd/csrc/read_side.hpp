// read_side.hpp — every result call of a batch (tri_batch_*) and of a collection batch (tri_cbatch_*): what a caller reads once tri_batch_sync has returned.
// Included once by trinity_hip.hip, behind the batch runtime (the same translation unit, as write_side.hpp is); what each call delivers is documented in
// include/trinity_hip.h.  Three things exist once here:
//   read_check / query_view   the arguments, the mode, "tri_batch_sync first", and — per query — the plan slot, the DevQuery and the match count
//   for_each_segment          a query's result is the in-order concatenation of its task segments
//   ReadBack                  THE stream rule: a result copy is enqueued on the read-back stream under the handle's lock and awaited outside it
// The transforms between the device's layout and the caller's (mask widening, frequency-row narrowing, bitmap expansion) are host/result_rows.hpp; a collection's
// facet rows are summed by host/facet_rows.hpp; an ordered row's keys are split into docIDs and values by host/order_rows.hpp; a collection's
// stats rows are combined by host/stats_rows.hpp.
#pragma once
#include "host/result_rows.hpp"
#include "host/facet_rows.hpp"
#include "host/order_rows.hpp"
#include "host/stats_rows.hpp"

namespace {
        // what every result call opens with: its arguments, the flags the batch must have been created with, and (must_sync) that its results stand
        int read_check(const tri_batch *b, const bool args_ok, const char *fn, const uint32_t need, const bool must_sync, const size_t *q = nullptr) {
                if (!b || !args_ok)
                        return fail(TRI_ERR_INVALID, "%s: null argument", fn);
                if (q && *q >= b->nq)
                        return fail(TRI_ERR_INVALID, "%s: query %zu of %zu", fn, *q, b->nq);
                if ((b->flags & need) != need)
                        return fail(TRI_ERR_INVALID, "%s: the batch was not created with %s%s%s", fn, need & TRI_FLAG_ACCUMULATED_SCORE ? "TRI_FLAG_ACCUMULATED_SCORE" : "",
                                    need & TRI_FLAG_MATCHED_TERMS ? "TRI_FLAG_MATCHED_TERMS" : "", need & TRI_FLAG_HIT_PAYLOADS ? " | TRI_FLAG_HIT_PAYLOADS" : "");
                if (must_sync && !b->synced)
                        return fail(TRI_ERR_INVALID, "%s: tri_batch_sync first", fn);
                return TRI_OK;
        }

        // ... and what a per-query call starts from
        struct QueryView {
                uint32_t slot = UINT32_MAX;
                const DevQuery *dq = nullptr; // nullptr: the planner left the query out — it has no matches, the outputs are zeroed
                uint64_t count = 0;           // its matches (of a synced batch)
        };
        int query_view(const tri_batch *b, const size_t q, const bool args_ok, const char *fn, const uint32_t need, const bool must_sync, QueryView &v) {
                if (const int rc = read_check(b, args_ok, fn, need, must_sync, &q))
                        return rc;
                v.slot = b->slot_of_query[q];
                if (v.slot != UINT32_MAX) {
                        v.dq = &b->plan[v.slot];
                        v.count = b->synced ? b->h_query_counts[v.slot] : 0;
                }
                return TRI_OK;
        }

        // f(w, t, out_off, c) for every non-empty task segment of the query, in order: w = the matches of the segments before it (the running destination index),
        // t = the task, out_off = its first out[] slot, c = its matches
        template <class F>
        void for_each_segment(const tri_batch *b, const DevQuery &dq, F &&f) {
                size_t w = 0;
                for (uint32_t t = dq.first_task; t < dq.first_task + dq.ntasks; ++t)
                        if (const uint32_t c = b->h_counts[t]) {
                                f(w, t, b->tasks[t].out_off, c);
                                w += c;
                        }
        }

        // The read-backs of one result call.  The batch is synced, its results are complete: the copies go on the read-back stream and wait for nothing queued behind
        // the batch on the engine stream; the handle's lock covers each enqueue and never the wait — a thread that compiles or runs the next batch is not held up by
        // the time a large result spends on PCIe.  The first error sticks: what follows it is skipped, wait() returns it.
        struct ReadBack {
                tri_dev *dev;
                hipError_t e;
                explicit ReadBack(tri_dev *d) : dev(d), e(hipSetDevice(d->device)) {}
                template <class F>
                void enqueue(F &&f) { // f(stream): a kernel or a gather ahead of the copy
                        if (e != hipSuccess)
                                return;
                        DevLock g(dev->mu);
                        e = f(dev->stream_rb);
                }
                ReadBack &copy(void *dst, const void *src, const size_t bytes) { // (an output the caller did not ask for, an empty result: nothing)
                        if (dst && bytes)
                                enqueue([&](hipStream_t s) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s); });
                        return *this;
                }
                hipError_t wait() { return e != hipSuccess ? e : (e = hipStreamSynchronize(dev->stream_rb)); }
                int done() { HIP_TRY(wait()); return TRI_OK; } // ... as the call's status
        };

        bool no_docset(const tri_batch *b, const DevQuery &dq) { // a top-K batch's one-pass queries keep top-K lists and match counts, no docID sets
                return dq.ntasks && !dq.out_cap && task_onepass(b->tasks[dq.first_task].kind);
        }

        // tri_batch_query_terms (width 16: never past terms[16]) and tri_batch_query_terms_wide (width 64)
        int query_terms(tri_batch *b, const size_t q, uint32_t *terms, uint32_t *nterms, const uint32_t width, const char *fn) {
                QueryView v;
                if (const int rc = query_view(b, q, terms && nterms, fn, TRI_FLAG_MATCHED_TERMS, false, v))
                        return rc;
                *nterms = 0;
                if (!v.dq)
                        return TRI_OK;
                if (v.dq->nscore > width && width < RICH_WIDE_TERMS)
                        return fail(TRI_ERR_INVALID, "%s: query %zu reports %u terms (option rich_max_terms): call tri_batch_query_terms_wide", fn, q, v.dq->nscore);
                *nterms = std::min(v.dq->nscore, width);
                std::copy_n(b->sterms.data() + v.dq->score_base, *nterms, terms);
                return TRI_OK;
        }

        // tri_batch_matched_terms (present: 32-bit masks) and tri_batch_matched_terms_wide (present64: a narrow query's mask zero-extended)
        int matched_terms(tri_batch *b, const size_t q, uint32_t *present, uint64_t *present64, uint16_t *freq, uint16_t *positions, const size_t pos_cap, size_t *npos, const bool wide_call,
                          const char *fn) {
                QueryView v;
                if (const int rc = query_view(b, q, npos != nullptr, fn, TRI_FLAG_MATCHED_TERMS, true, v))
                        return rc;
                *npos = 0;
                if (!v.dq)
                        return TRI_OK;
                const DevQuery &dq = *v.dq;
                const bool wide_q = dq.nscore > RICH_NARROW_TERMS; // a wide-report query: rows and high mask halves of its own (BatchPlan::rich_wide)
                if (wide_q && !wide_call) // (a 32-bit mask would be truncated)
                        return fail(TRI_ERR_INVALID, "%s: query %zu reports %u terms (option rich_max_terms): call tri_batch_matched_terms_wide", fn, q, dq.nscore);
                // the query's tasks are consecutive, so its hits are one contiguous run of the pool
                const uint64_t p0 = b->h_task_pos_base[dq.first_task];
                *npos = (size_t)(b->h_task_pos_base[dq.first_task + dq.ntasks] - p0);
                if (positions && pos_cap < *npos)
                        return fail(TRI_ERR_INVALID, "%s: positions need %zu slots, %zu given", fn, *npos, pos_cap);
                ReadBack rb(b->dev);
                rb.copy(positions, b->d_rich_pool + p0, *npos * 2);
                // per-match rows live at the tasks' out[] slots.  Frequency rows are `stride` cells apart on the device (a wide-report query's in its own share of the
                // wide array), nscore wide for the caller: where the two differ, a segment's rows are staged, awaited and narrowed before the next segment's
                const DevRichWide *rw = wide_q ? &b->rich_wide[v.slot] : nullptr;
                const uint32_t stride = wide_q ? rw->stride : b->rich_R;
                const uint16_t *d_rows = wide_q ? b->d_rich_freq_wide + rw->cells : b->d_rich_freq + dq.out_off * b->rich_R;
                std::vector<uint16_t> rows;
                // present64: a segment's low words are copied into the UPPER half of the segment's own u64 cells and widened in place once the copies have landed
                // (result_rows::widen); a wide-report query's high words wait in a staging array meanwhile
                std::vector<uint32_t> hi(present64 && wide_q ? v.count : 0);
                std::vector<result_rows::Segment> segs;
                for_each_segment(b, dq, [&](const size_t w, uint32_t, const uint64_t off, const uint32_t c) {
                        const uint64_t rel = off - dq.out_off;
                        rb.copy(present ? present + w : nullptr, b->d_rich_present + off, (size_t)c * 4);
                        if (present64) {
                                rb.copy(reinterpret_cast<uint32_t *>(present64 + w) + c, b->d_rich_present + off, (size_t)c * 4);
                                if (wide_q)
                                        rb.copy(hi.data() + w, b->d_rich_present_hi + rw->slots + rel, (size_t)c * 4);
                                segs.push_back({w, c});
                        }
                        if (freq && stride == dq.nscore)
                                rb.copy(freq + w * dq.nscore, d_rows + rel * stride, (size_t)c * 2 * stride);
                        else if (freq) {
                                rows.resize((size_t)c * stride);
                                rb.copy(rows.data(), d_rows + rel * stride, (size_t)c * 2 * stride);
                                if (rb.wait() == hipSuccess)
                                        result_rows::narrow(freq + w * dq.nscore, rows.data(), c, stride, dq.nscore);
                        }
                });
                HIP_TRY(rb.wait());
                result_rows::widen(present64, segs.data(), segs.size(), wide_q ? hi.data() : nullptr);
                return TRI_OK;
        }

        // (forms == nullptr: every set as ascending docIDs — tri_batch_docsets; else tri_batch_docsets_mixed: a RESULT_BITMAP query's region goes out as its words)
        int docsets_deliver(tri_batch *b, uint32_t *out, const size_t cap, uint64_t *offsets, uint32_t *forms, const char *fn) {
                if (const int rc = read_check(b, offsets != nullptr, fn, 0, true))
                        return rc;
                tri_dev *dev = b->dev;
                const size_t nslots = b->plan.size();
                std::vector<uint64_t> slot_off(nslots + 1, 0);
                uint64_t total = 0;
                for (size_t q = 0; q < b->nq; ++q) {
                        const uint32_t slot = b->slot_of_query[q];
                        offsets[q] = total;
                        if (forms)
                                forms[q] = RESULT_DOCIDS;
                        if (slot == UINT32_MAX)
                                continue;
                        const DevQuery &dq = b->plan[slot];
                        if (no_docset(b, dq) && b->h_query_counts[slot])
                                return fail(TRI_ERR_INVALID, "%s: query %zu ran through the one-pass scored kernel: an AccumulatedScore top-K batch keeps top-K lists and match counts, not docID sets", fn, q);
                        slot_off[slot] = total;
                        if (forms && dq.form == RESULT_BITMAP) {
                                forms[q] = RESULT_BITMAP;
                                total += dq.out_cap; // (the region's words: one bit per document of the query's docID range, from document 0)
                        } else
                                total += b->h_query_counts[slot];
                }
                offsets[b->nq] = total;
                if (!out || !total)
                        return TRI_OK;
                if (cap < total)
                        return fail(TRI_ERR_INVALID, "%s: the docID sets need %llu slots, %zu given", fn, (unsigned long long)total, cap);
                // the sets are gathered on the device into one contiguous buffer and come over in a single copy (the lock covers the pool too)
                Pooled<uint32_t> d_flat;
                Pooled<uint64_t> d_slot_off;
                ReadBack rb(dev);
                rb.enqueue([&](hipStream_t s) {
                        hipError_t e = d_flat.alloc(dev, (total + 64) * 4);
                        if (e == hipSuccess)
                                e = d_slot_off.alloc(dev, (nslots + 1) * 8 + POOL_MIN_BYTES);
                        if (e == hipSuccess)
                                e = hipMemcpyAsync(d_slot_off, slot_off.data(), (nslots + 1) * 8, hipMemcpyHostToDevice, s); // (pageable source: staged before the call returns)
                        if (e != hipSuccess)
                                return e;
                        hipLaunchKernelGGL(k_deliver_docsets, dim3((uint32_t)b->tasks.size()), dim3(256), 0, s, (const DevQuery *)b->dev_at(b->plan), (const DevTask *)b->dev_at(b->tasks),
                                           (const uint32_t *)b->d_counts, (const uint32_t *)b->d_out, (const uint64_t *)d_slot_off, d_flat, forms ? 1u : 0u);
                        return hipGetLastError();
                });
                HIP_TRY(rb.copy(out, d_flat, total * 4).wait()); // (the wait comes first on every way out: the two buffers go back to the pool behind it)
                return TRI_OK;
        }

        int cbatch_check(const tri_cbatch *c, const bool args_ok, const char *fn) {
                if (!c || !args_ok)
                        return fail(TRI_ERR_INVALID, "%s: null argument", fn);
                if (!c->synced)
                        return fail(TRI_ERR_INVALID, "%s: tri_cbatch_sync first", fn);
                return TRI_OK;
        }

        // the default mode's rows over a collection: column k must mean the same slot in every part that reports the query at all (a part that left it out, or
        // to which all of its terms are unknown, reports no terms and holds no row)
        int cbatch_query_width(tri_cbatch *c, const size_t q, const char *fn, uint32_t &nterms) {
                uint32_t terms[RICH_WIDE_TERMS];
                nterms = 0;
                for (size_t i = 0; i < c->parts.size(); ++i) {
                        uint32_t nt = 0;
                        if (const int rc = tri_batch_query_terms_wide(c->parts[i], q, terms, &nt))
                                return rc;
                        if (nt && nterms && nt != nterms)
                                return fail(TRI_ERR_INVALID, "%s: query %zu reports %u terms in part %zu and %u in an older part (terms unknown to a source that resolve to one id?): read it part by part", fn,
                                            q, nt, i, nterms);
                        if (nt)
                                nterms = nt;
                }
                return TRI_OK;
        }

        // tri_cbatch_matched_terms[_wide]: the parts' own calls source after source — a sizing pass first (it also takes every refusal before anything is written)
        int cbatch_matched_terms(tri_cbatch *c, const size_t q, uint32_t *present, uint64_t *present64, uint16_t *freq, uint16_t *positions, const size_t pos_cap, size_t *npos,
                                 const bool wide_call, const char *fn) {
                if (const int rc = cbatch_check(c, npos != nullptr, fn))
                        return rc;
                auto part_call = [&](tri_batch *p, uint32_t *pr, uint64_t *pr64, uint16_t *f, uint16_t *pos, const size_t cap, size_t *np) {
                        return wide_call ? tri_batch_matched_terms_wide(p, q, pr64, f, pos, cap, np) : tri_batch_matched_terms(p, q, pr, f, pos, cap, np);
                };
                size_t total = 0;
                for (tri_batch *p : c->parts) {
                        size_t np = 0;
                        if (const int rc = part_call(p, nullptr, nullptr, nullptr, nullptr, 0, &np))
                                return rc;
                        total += np;
                }
                uint32_t nterms = 0;
                if (const int rc = cbatch_query_width(c, q, fn, nterms))
                        return rc;
                *npos = total;
                if (positions && pos_cap < total)
                        return fail(TRI_ERR_INVALID, "%s: positions need %zu slots, %zu given", fn, total, pos_cap);
                size_t m = 0, w = 0;
                for (tri_batch *p : c->parts) {
                        size_t n = 0, np = 0;
                        if (const int rc = tri_batch_docset(p, q, nullptr, 0, &n))
                                return rc;
                        if (const int rc = part_call(p, present ? present + m : nullptr, present64 ? present64 + m : nullptr, freq ? freq + m * nterms : nullptr,
                                                     positions ? positions + w : nullptr, total - w, &np))
                                return rc;
                        m += n;
                        w += np;
                }
                return TRI_OK;
        }
} // namespace

extern "C" int tri_batch_query_terms(tri_batch *b, size_t q, uint32_t *terms, uint32_t *nterms) { return query_terms(b, q, terms, nterms, RICH_NARROW_TERMS, __func__); }
extern "C" int tri_batch_query_terms_wide(tri_batch *b, size_t q, uint32_t *terms, uint32_t *nterms) { return query_terms(b, q, terms, nterms, RICH_WIDE_TERMS, __func__); }

extern "C" int tri_batch_matched_terms(tri_batch *b, size_t q, uint32_t *present, uint16_t *freq, uint16_t *positions, size_t pos_cap, size_t *npos) {
        return matched_terms(b, q, present, nullptr, freq, positions, pos_cap, npos, false, __func__);
}
extern "C" int tri_batch_matched_terms_wide(tri_batch *b, size_t q, uint64_t *present, uint16_t *freq, uint16_t *positions, size_t pos_cap, size_t *npos) {
        return matched_terms(b, q, nullptr, present, freq, positions, pos_cap, npos, true, __func__);
}

// the payloads of query q's hits, parallel to the positions the matched_terms calls return (same order, same count)
extern "C" int tri_batch_matched_payloads(tri_batch *b, size_t q, uint8_t *lens, uint64_t *payloads, size_t cap, size_t *n) {
        QueryView v;
        if (const int rc = query_view(b, q, n != nullptr, __func__, TRI_FLAG_MATCHED_TERMS | TRI_FLAG_HIT_PAYLOADS, true, v))
                return rc;
        *n = 0;
        if (!v.dq)
                return TRI_OK;
        const uint64_t p0 = b->h_task_pos_base[v.dq->first_task];
        *n = (size_t)(b->h_task_pos_base[v.dq->first_task + v.dq->ntasks] - p0);
        if (!lens && !payloads)
                return TRI_OK;
        if (cap < *n)
                return fail(TRI_ERR_INVALID, "%s: payloads need %zu slots, %zu given", __func__, *n, cap);
        return ReadBack(b->dev).copy(lens, b->d_rich_plen + p0, *n).copy(payloads, b->d_rich_payload + p0, *n * 8).done();
}

extern "C" int tri_batch_ranked(tri_batch *b, uint32_t *docids, double *scores, uint32_t *counts) {
        if (const int rc = read_check(b, docids && scores && counts, __func__, 0, false))
                return rc;
        if (!b->rank_on)
                return fail(TRI_ERR_INVALID, "%s: no ranker is set (tri_batch_set_ranker)", __func__);
        if (!b->synced || (!b->rank_done && !b->tasks.empty()))
                return fail(TRI_ERR_INVALID, "%s: tri_batch_sync first (a run that follows tri_batch_set_ranker)", __func__);
        const size_t K = b->rank.topk;
        return ReadBack(b->dev).copy(docids, b->d_rank_docs, b->nq * K * 4).copy(scores, b->d_rank_scores, b->nq * K * 8).copy(counts, b->d_rank_counts, b->nq * 4).done();
}

extern "C" int tri_batch_get_info(const tri_batch *b, tri_batch_info *info) {
        if (const int rc = read_check(b, info != nullptr, __func__, 0, false))
                return rc;
        *info = b->info;
        return TRI_OK;
}

extern "C" int tri_batch_query_status(const tri_batch *b, int32_t *status) {
        if (const int rc = read_check(b, status != nullptr, __func__, 0, false))
                return rc;
        std::copy_n(b->qstatus.begin(), b->nq, status);
        return TRI_OK;
}

extern "C" int tri_batch_match_counts(tri_batch *b, uint64_t *counts) {
        if (const int rc = read_check(b, counts != nullptr, __func__, 0, true))
                return rc;
        for (size_t q = 0; q < b->nq; ++q)
                counts[q] = b->slot_of_query[q] == UINT32_MAX ? 0 : b->h_query_counts[b->slot_of_query[q]];
        return TRI_OK;
}

extern "C" int tri_batch_docset(tri_batch *b, size_t q, uint32_t *out, size_t cap, size_t *n) {
        QueryView v;
        if (const int rc = query_view(b, q, n != nullptr, __func__, 0, true, v))
                return rc;
        *n = v.count;
        if (!*n || !out)
                return TRI_OK;
        const DevQuery &dq = *v.dq;
        if (no_docset(b, dq))
                return fail(TRI_ERR_INVALID, "%s: query %zu ran through the one-pass scored kernel: an AccumulatedScore top-K batch keeps top-K lists and match counts, not docID sets (use topk == 0 or DocumentsOnly)", __func__, q);
        if (cap < *n)
                return fail(TRI_ERR_INVALID, "%s: docset needs %zu slots, %zu given", __func__, *n, cap);
        ReadBack rb(b->dev);
        if (dq.form == RESULT_BITMAP) { // one bit per document: the region's words come over as they are, the docIDs are written out here
                const uint32_t w_lo = b->tasks[dq.first_task].tile_begin, w_hi = b->tasks[dq.first_task + dq.ntasks - 1].tile_end;
                std::vector<uint32_t> words((size_t)(w_hi - w_lo) * SPAN_WORDS);
                HIP_TRY(rb.copy(words.data(), b->d_out + dq.out_off, words.size() * 4).wait());
                size_t got = 0;
                switch (result_rows::expand(words.data(), words.size(), (size_t)w_lo * SPAN_WORDS, out, *n, &got)) {
                case result_rows::EXPAND_MORE:
                        return fail(TRI_ERR_INTERNAL, "%s: query %zu: its bitmap holds more documents than its tasks counted", __func__, q);
                case result_rows::EXPAND_FEWER:
                        return fail(TRI_ERR_INTERNAL, "%s: query %zu: its bitmap holds %zu documents, its tasks counted %zu", __func__, q, got, *n);
                }
                return TRI_OK;
        }
        for_each_segment(b, dq, [&](const size_t w, uint32_t, const uint64_t off, const uint32_t c) { rb.copy(out + w, b->d_out + off, (size_t)c * 4); });
        return rb.done();
}

extern "C" int tri_batch_docset_bitmap(tri_batch *b, size_t q, int *form, uint32_t *words, size_t cap, uint32_t *first_doc, size_t *nwords) {
        QueryView v;
        if (const int rc = query_view(b, q, form && first_doc && nwords, __func__, 0, true, v))
                return rc;
        *form = 0, *first_doc = 0, *nwords = 0;
        if (!v.dq || v.dq->form != RESULT_BITMAP)
                return TRI_OK;
        const DevQuery &dq = *v.dq;
        const uint32_t w_lo = b->tasks[dq.first_task].tile_begin, w_hi = b->tasks[dq.first_task + dq.ntasks - 1].tile_end;
        *form = 1, *first_doc = w_lo * SPAN_BITS, *nwords = (size_t)(w_hi - w_lo) * SPAN_WORDS;
        if (!words)
                return TRI_OK;
        if (cap < *nwords)
                return fail(TRI_ERR_INVALID, "%s: bitmap needs %zu words, %zu given", __func__, *nwords, cap);
        return ReadBack(b->dev).copy(words, b->d_out + dq.out_off, *nwords * 4).done();
}

extern "C" int tri_batch_docset_hashes(tri_batch *b, uint64_t *hashes) {
        if (const int rc = read_check(b, hashes != nullptr, __func__, 0, true))
                return rc;
        if ((b->n_fused + b->n_fused16 + b->n_fusedgen + b->n_planes + b->n_planes8) && (b->flags & TRI_FLAG_ACCUMULATED_SCORE)) // (DocumentsOnly: the one-pass kernel's tasks wrote their matches)
                return fail(TRI_ERR_INVALID, "%s: the batch holds queries that ran through the one-pass scored kernel: their docID sets are not materialised", __func__);
        const uint32_t n = (uint32_t)b->plan.size();
        std::vector<uint64_t> h(n);
        if (n) {
                ReadBack rb(b->dev);
                rb.enqueue([&](hipStream_t s) {
                        if (!b->d_hashes)
                                if (const hipError_t e = b->d_hashes.alloc((size_t)n * 8))
                                        return e;
                        hipLaunchKernelGGL(k_hash_docsets, dim3((n + 63) / 64), dim3(64), 0, s, b->dev_at(b->plan), b->dev_at(b->tasks), b->d_counts, n, b->d_out, b->d_hashes);
                        return hipGetLastError();
                });
                HIP_TRY(rb.copy(h.data(), b->d_hashes, (size_t)n * 8).wait());
        }
        for (size_t q = 0; q < b->nq; ++q)
                hashes[q] = b->slot_of_query[q] == UINT32_MAX ? 1469598103934665603ull : h[b->slot_of_query[q]];
        return TRI_OK;
}

extern "C" int tri_batch_topk(tri_batch *b, uint32_t *docids, float *scores, uint32_t *counts) {
        if (const int rc = read_check(b, docids && scores && counts, __func__, TRI_FLAG_ACCUMULATED_SCORE, true))
                return rc;
        const size_t nq = b->nq, k = b->topk;
        return ReadBack(b->dev).copy(docids, b->d_top_docs, nq * k * 4).copy(scores, b->d_top_scores, nq * k * 4).copy(counts, b->d_top_counts, nq * 4).done();
}

extern "C" int tri_batch_scores(tri_batch *b, size_t q, double *out, size_t cap, size_t *n) {
        QueryView v;
        if (const int rc = query_view(b, q, n != nullptr, __func__, TRI_FLAG_ACCUMULATED_SCORE, true, v))
                return rc;
        if (b->topk)
                return fail(TRI_ERR_INVALID, "%s: per-match scores are kept only for AccumulatedScoreScheme batches created with topk == 0", __func__);
        *n = v.count;
        if (!*n || !out)
                return TRI_OK;
        if (cap < *n)
                return fail(TRI_ERR_INVALID, "%s: scores need %zu slots, %zu given", __func__, *n, cap);
        ReadBack rb(b->dev);
        for_each_segment(b, *v.dq, [&](const size_t w, uint32_t, const uint64_t off, const uint32_t c) { rb.copy(out + w, b->d_all_scores + off, (size_t)c * 8); });
        return rb.done();
}

// every query's docID set in ONE call: gathered on the device into one contiguous buffer (k_deliver_docsets), over in a single copy ...
extern "C" int tri_batch_docsets(tri_batch *b, uint32_t *out, size_t cap, uint64_t *offsets) { return docsets_deliver(b, out, cap, offsets, nullptr, __func__); }

// ... and each set in the form the engine holds it: a RESULT_BITMAP query's region crosses PCIe as its words, a bit per document
extern "C" int tri_batch_docsets_mixed(tri_batch *b, uint32_t *out, size_t cap, uint64_t *offsets, uint32_t *forms) {
        if (!forms)
                return fail(TRI_ERR_INVALID, "%s: null forms", __func__);
        return docsets_deliver(b, out, cap, offsets, forms, __func__);
}

extern "C" int tri_batch_counts_device(tri_batch *b, void **counts) {
        if (const int rc = read_check(b, counts != nullptr, __func__, 0, false))
                return rc;
        *counts = b->d_qcounts;
        return TRI_OK;
}

extern "C" int tri_batch_topk_device(tri_batch *b, void **docids, void **scores, void **counts) {
        if (const int rc = read_check(b, docids && scores && counts, __func__, TRI_FLAG_ACCUMULATED_SCORE, false))
                return rc;
        *docids = b->d_top_docs, *scores = b->d_top_scores, *counts = b->d_top_counts;
        return TRI_OK;
}

// facet counts (tri_batch_set_facets; k_facet.hpp): one facet's rows of the whole batch: they lie in caller query order, one after the other — ONE read-back copy
extern "C" int tri_batch_facets(tri_batch *b, size_t k, uint32_t *counts, size_t cap) {
        if (const int rc = read_check(b, counts != nullptr, __func__, 0, false))
                return rc;
        if (b->facets.n && k >= b->facets.n) // (none set: consumer_ready says so)
                return fail(TRI_ERR_INVALID, "%s: facet %zu of %u", __func__, k, b->facets.n);
        if (const int rc = consumer_ready(b, CONSUMER_FACETS, __func__, "tri_batch_set_facets"))
                return rc;
        const size_t need = b->nq * ((size_t)b->facets.nb[k] + 1);
        if (cap < need)
                return fail(TRI_ERR_INVALID, "%s: the rows need %zu counters, %zu given", __func__, need, cap);
        return ReadBack(b->dev).copy(counts, b->facet_rows() + b->facets.rows_off[k], need * 4).done();
}

// stats of a column (tri_batch_set_stats; k_stats.hpp): one stat's four planes of the whole batch: each lies in caller query order — ONE read-back copy per plane asked for
extern "C" int tri_batch_stats(tri_batch *b, size_t k, uint64_t *sums, uint32_t *counts, uint32_t *mins, uint32_t *maxs, size_t cap) {
        if (const int rc = read_check(b, sums || counts || mins || maxs, __func__, 0, false))
                return rc;
        if (b->stats.n && k >= b->stats.n) // (none set: consumer_ready says so)
                return fail(TRI_ERR_INVALID, "%s: stat %zu of %u", __func__, k, b->stats.n);
        if (const int rc = consumer_ready(b, CONSUMER_STATS, __func__, "tri_batch_set_stats"))
                return rc;
        const size_t need = b->nq * ((size_t)b->stats.nb[k] + 1);
        if (cap < need)
                return fail(TRI_ERR_INVALID, "%s: the rows need %zu records, %zu given", __func__, need, cap);
        const uint32_t *base = b->stats_rows() + b->stats.off[k];
        return ReadBack(b->dev).copy(sums, base, need * 8).copy(counts, base + 2 * need, need * 4).copy(mins, base + 3 * need, need * 4).copy(maxs, base + 4 * need, need * 4).done();
}

namespace {
        // rows of topk keys and their counts, read back in two copies and split into the caller's arrays
        int ordered_rows(tri_dev *dev, const uint64_t *d_keys, const uint32_t *d_counts, const size_t nq, const size_t k, const bool descending, uint32_t *docids, uint32_t *values,
                         uint32_t *counts) {
                Pinned<uint64_t> pinned; // (the keys are staged in a pinned block of the handle's pool; pageable memory where none is to be had)
                std::unique_ptr<uint64_t[]> pageable;
                uint64_t *keys = pinned.alloc(dev, nq * k * 8 + 8);
                if (!keys)
                        keys = (pageable = std::make_unique<uint64_t[]>(nq * k + 1)).get();
                if (const int rc = ReadBack(dev).copy(keys, d_keys, nq * k * 8).copy(counts, d_counts, nq * 4).done())
                        return rc;
                order_rows::split(keys, counts, nq, k, descending, docids, values);
                return TRI_OK;
        }
} // namespace

// order by a column (tri_batch_set_order; k_order.hpp): every query's first topk documents by (value, docID) — the rows lie in caller query order
extern "C" int tri_batch_ordered(tri_batch *b, uint32_t *docids, uint32_t *values, uint32_t *counts) {
        if (const int rc = read_check(b, docids && values && counts, __func__, 0, false))
                return rc;
        if (const int rc = consumer_ready(b, CONSUMER_ORDER, __func__, "tri_batch_set_order"))
                return rc;
        return ordered_rows(b->dev, b->order_keys(b->order_lists), b->order_counts(b->order_lists), b->nq, b->order.topk, b->order.flip != 0, docids, values, counts);
}

// ---- a collection batch's results: merged on the device by tri_cbatch_run (match counts add up, top-K lists merge K-way)
extern "C" int tri_cbatch_match_counts(tri_cbatch *c, uint64_t *counts) {
        if (const int rc = cbatch_check(c, counts != nullptr, __func__))
                return rc;
        return ReadBack(c->parts[0]->dev).copy(counts, c->d_counts, c->parts[0]->nq * 8).done();
}

extern "C" int tri_cbatch_topk(tri_cbatch *c, uint32_t *docids, float *scores, uint32_t *counts) {
        if (const int rc = cbatch_check(c, docids && scores && counts, __func__))
                return rc;
        if (!c->d_top_docs)
                return fail(TRI_ERR_INVALID, "%s: the parts were not created with TRI_FLAG_ACCUMULATED_SCORE and topk >= 1", __func__);
        const size_t nq = c->parts[0]->nq, k = c->parts[0]->topk;
        return ReadBack(c->parts[0]->dev).copy(docids, c->d_top_docs, nq * k * 4).copy(scores, c->d_top_scores, nq * k * 4).copy(counts, c->d_top_counts, nq * 4).done();
}

// the docID set of query q over the collection: the sources' sets one after the other (each ascending; the sources are disjoint where
// the newer ones mask the older) — the order exec_query delivers them in when it is called source after source
extern "C" int tri_cbatch_docset(tri_cbatch *c, size_t q, uint32_t *out, size_t cap, size_t *n) {
        if (const int rc = cbatch_check(c, n != nullptr, __func__))
                return rc;
        size_t total = 0;
        for (tri_batch *p : c->parts) {
                size_t m = 0;
                if (int rc = tri_batch_docset(p, q, nullptr, 0, &m))
                        return rc;
                total += m;
        }
        *n = total;
        if (!out)
                return TRI_OK;
        if (cap < total)
                return fail(TRI_ERR_INVALID, "%s: docset needs %zu slots, %zu given", __func__, total, cap);
        size_t w = 0;
        for (tri_batch *p : c->parts) {
                size_t m = 0;
                if (int rc = tri_batch_docset(p, q, out + w, cap - w, &m))
                        return rc;
                w += m;
        }
        return TRI_OK;
}

// a collection's ranked list (k_rank_merge_sources, queued by tri_cbatch_sync): the best topk (docID, score) pairs of every query over all parts
extern "C" int tri_cbatch_ranked(tri_cbatch *c, uint32_t *docids, double *scores, uint32_t *counts) {
        if (const int rc = cbatch_check(c, docids && scores && counts, __func__))
                return rc;
        if (!c->ranked)
                return fail(TRI_ERR_INVALID, "%s: the collection is not ranked: %s", __func__, c->rank_why.c_str());
        const size_t nq = c->parts[0]->nq, k = c->rank_k;
        return ReadBack(c->parts[0]->dev).copy(docids, c->d_rank_docs, nq * k * 4).copy(scores, c->d_rank_scores, nq * k * 8).copy(counts, c->d_rank_counts, nq * 4).done();
}

// the default mode's rows of query q over the collection, parallel to tri_cbatch_docset: each part's rows source after source (host walks over the parts' calls)
extern "C" int tri_cbatch_matched_terms(tri_cbatch *c, size_t q, uint32_t *present, uint16_t *freq, uint16_t *positions, size_t pos_cap, size_t *npos) {
        return cbatch_matched_terms(c, q, present, nullptr, freq, positions, pos_cap, npos, false, __func__);
}
extern "C" int tri_cbatch_matched_terms_wide(tri_cbatch *c, size_t q, uint64_t *present, uint16_t *freq, uint16_t *positions, size_t pos_cap, size_t *npos) {
        return cbatch_matched_terms(c, q, nullptr, present, freq, positions, pos_cap, npos, true, __func__);
}

extern "C" int tri_cbatch_matched_payloads(tri_cbatch *c, size_t q, uint8_t *lens, uint64_t *payloads, size_t cap, size_t *n) {
        if (const int rc = cbatch_check(c, n != nullptr, __func__))
                return rc;
        size_t total = 0;
        for (tri_batch *p : c->parts) {
                size_t m = 0;
                if (const int rc = tri_batch_matched_payloads(p, q, nullptr, nullptr, 0, &m))
                        return rc;
                total += m;
        }
        *n = total;
        if (!lens && !payloads)
                return TRI_OK;
        if (cap < total)
                return fail(TRI_ERR_INVALID, "%s: payloads need %zu slots, %zu given", __func__, total, cap);
        size_t w = 0;
        for (tri_batch *p : c->parts) {
                size_t m = 0;
                if (const int rc = tri_batch_matched_payloads(p, q, lens ? lens + w : nullptr, payloads ? payloads + w : nullptr, total - w, &m))
                        return rc;
                w += m;
        }
        return TRI_OK;
}

// facet k's rows over a collection (tri_batch_facets above): the parts' rows widened and summed (a document of several sources counts once per source that delivers it, as tri_cbatch_docset lists it)
extern "C" int tri_cbatch_facets(tri_cbatch *c, size_t k, uint64_t *counts, size_t cap) {
        if (const int rc = cbatch_check(c, counts != nullptr, __func__))
                return rc;
        const tri_batch *p0 = c->parts[0];
        for (size_t i = 0; i < c->parts.size(); ++i) {
                const tri_batch *p = c->parts[i];
                if (p->facets.n != p0->facets.n)
                        return fail(TRI_ERR_INVALID, "%s: part %zu carries %u facets, part 0 carries %u", __func__, i, p->facets.n, p0->facets.n);
                if (k < p->facets.n && p->facets.nb[k] != p0->facets.nb[k])
                        return fail(TRI_ERR_INVALID, "%s: facet %zu has %u buckets in part %zu and %u in part 0", __func__, k, p->facets.nb[k], i, p0->facets.nb[k]);
        }
        if (!p0->facets.n)
                return fail(TRI_ERR_INVALID, "%s: no facets are set on the parts (tri_batch_set_facets)", __func__);
        if (k >= p0->facets.n)
                return fail(TRI_ERR_INVALID, "%s: facet %zu of %u", __func__, k, p0->facets.n);
        const size_t need = p0->nq * ((size_t)p0->facets.nb[k] + 1);
        if (cap < need)
                return fail(TRI_ERR_INVALID, "%s: the rows need %zu counters, %zu given", __func__, need, cap);
        std::vector<uint32_t> part(need);
        std::vector<uint64_t> sum(need, 0); // (nothing is written to counts[] before every part has answered)
        for (tri_batch *p : c->parts) {
                if (const int rc = tri_batch_facets(p, k, part.data(), need))
                        return rc;
                facet_rows::add(sum.data(), part.data(), need);
        }
        std::copy(sum.begin(), sum.end(), counts);
        return TRI_OK;
}

// a collection's ordered rows (k_order_merge<true>, queued by tri_cbatch_sync): the first topk (docID, value) pairs of every query over all parts
extern "C" int tri_cbatch_ordered(tri_cbatch *c, uint32_t *docids, uint32_t *values, uint32_t *counts) {
        if (const int rc = cbatch_check(c, docids && values && counts, __func__))
                return rc;
        if (!c->ordered)
                return fail(TRI_ERR_INVALID, "%s: %s", __func__, c->order_why.c_str());
        return ordered_rows(c->parts[0]->ix->dev, c->d_order_keys, c->d_order_counts, c->parts[0]->nq, c->order_k, c->parts[0]->order.flip != 0, docids, values, counts);
}

// stat k's rows over a collection (tri_batch_stats above; exec.h:12-23): the parts' rows combined on the host — counts and sums added, mins and maxs folded (a document
// of several sources counts once per source that delivers it, as tri_cbatch_docset lists it)
extern "C" int tri_cbatch_stats(tri_cbatch *c, size_t k, uint64_t *sums, uint64_t *counts, uint32_t *mins, uint32_t *maxs, size_t cap) {
        if (const int rc = cbatch_check(c, sums || counts || mins || maxs, __func__))
                return rc;
        const tri_batch *p0 = c->parts[0];
        for (size_t i = 0; i < c->parts.size(); ++i) {
                const tri_batch *p = c->parts[i];
                if (p->stats.n != p0->stats.n)
                        return fail(TRI_ERR_INVALID, "%s: part %zu carries %u stats, part 0 carries %u", __func__, i, p->stats.n, p0->stats.n);
                if (k < p->stats.n && !p->stats.group[k] != !p0->stats.group[k])
                        return fail(TRI_ERR_INVALID, "%s: stat %zu is %s in part %zu and %s in part 0", __func__, k, p->stats.group[k] ? "grouped" : "ungrouped", i,
                                    p0->stats.group[k] ? "grouped" : "ungrouped");
                if (k < p->stats.n && p->stats.nb[k] != p0->stats.nb[k])
                        return fail(TRI_ERR_INVALID, "%s: stat %zu has %u buckets in part %zu and %u in part 0", __func__, k, p->stats.nb[k], i, p0->stats.nb[k]);
        }
        if (!p0->stats.n)
                return fail(TRI_ERR_INVALID, "%s: no stats are set on the parts (tri_batch_set_stats)", __func__);
        if (k >= p0->stats.n)
                return fail(TRI_ERR_INVALID, "%s: stat %zu of %u", __func__, k, p0->stats.n);
        const size_t row = (size_t)p0->stats.nb[k] + 1, need = p0->nq * row;
        if (cap < need)
                return fail(TRI_ERR_INVALID, "%s: the rows need %zu records, %zu given", __func__, need, cap);
        std::vector<uint64_t> psums(need);
        std::vector<uint32_t> pcounts(need), pmins(need), pmaxs(need);
        std::vector<stats_rows::Record> total(need); // (nothing is written to the outputs before every part has answered)
        for (size_t i = 0; i < c->parts.size(); ++i) {
                if (const int rc = tri_batch_stats(c->parts[i], k, psums.data(), pcounts.data(), pmins.data(), pmaxs.data(), need))
                        return rc;
                const size_t at = stats_rows::add(total.data(), psums.data(), pcounts.data(), pmins.data(), pmaxs.data(), need);
                if (at != need)
                        return fail(TRI_ERR_INVALID, "%s: stat %zu: the sum of query %zu, bucket %zu wraps 64 bits at part %zu", __func__, k, at / row, at % row, i);
        }
        for (size_t i = 0; i < need; ++i) {
                if (sums)
                        sums[i] = total[i].sum;
                if (counts)
                        counts[i] = total[i].count;
                if (mins)
                        mins[i] = total[i].min;
                if (maxs)
                        maxs[i] = total[i].max;
        }
        return TRI_OK;
}

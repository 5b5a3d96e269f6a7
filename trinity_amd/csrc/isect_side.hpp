// isect_side.hpp — tri_isect_*: Trinity::intersect (intersect.cpp:5-170) for a batch of requests over one index.  The launches of k_isect.hpp's two passes, the
// host step between them and the replay of host/isect_rows.hpp.  Included at the end of trinity_hip.hip: the same translation unit.
#pragma once
#include "host/isect_rows.hpp"

struct tri_isect {
        struct Req {
                int32_t status = TRI_OK;
                std::vector<std::pair<uint64_t, uint32_t>> results; // finalize's order
                std::vector<isect_rows::HEntry> hist;               // ascending mask
        };
        std::vector<Req> reqs;
        std::vector<uint32_t> h_size, c_size, spills;
        tri_isect_info info{};
};

namespace {
        // what the host works out of a request before anything is launched
        struct IsectPlan {
                std::vector<IsectReq> reqs;
                std::vector<uint2> rowtab;   // (scratch row, group) per known term occurrence, request after request
                std::vector<uint32_t> build; // (term, row) pairs: k_term_plane0's build list
        };

        int isect_plan(const tri_index *ix, const tri_isect_request *reqs, const size_t nreq, const uint32_t *terms, const uint32_t *group_first, IsectPlan &P) {
                if (nreq > 65535)
                        return fail(TRI_ERR_INVALID, "tri_isect_run: %zu requests (at most 65535 a call)", nreq);
                size_t G = 0;
                for (size_t r = 0; r < nreq; ++r) {
                        if (reqs[r].ngroups == 0 || reqs[r].ngroups > 64)
                                return fail(TRI_ERR_INVALID, "tri_isect_run: request %zu names %u groups (1 .. 64)", r, reqs[r].ngroups);
                        if (reqs[r].reserved)
                                return fail(TRI_ERR_INVALID, "tri_isect_run: request %zu: reserved is not 0", r);
                        G += reqs[r].ngroups;
                }
                for (size_t g = 0; g < G; ++g)
                        if (group_first[g + 1] < group_first[g])
                                return fail(TRI_ERR_INVALID, "tri_isect_run: group_first does not ascend at group %zu", g);
                for (size_t i = group_first[0]; i < group_first[G]; ++i)
                        if (terms[i] != 0xffffffffu && terms[i] >= ix->terms.size())
                                return fail(TRI_ERR_INVALID, "tri_isect_run: term %u out of range", terms[i]);
                std::unordered_map<uint32_t, uint32_t> row_of;
                P.reqs.resize(nreq);
                size_t g0 = 0;
                for (size_t r = 0; r < nreq; ++r) {
                        IsectReq &q = P.reqs[r];
                        q = IsectReq{};
                        q.stop_mask = reqs[r].stopwords_mask;
                        q.row_first = (uint32_t)P.rowtab.size();
                        bool unknown = false;
                        for (uint32_t g = 0; g < reqs[r].ngroups; ++g)
                                for (size_t i = group_first[g0 + g]; i < group_first[g0 + g + 1]; ++i) {
                                        const uint32_t t = terms[i];
                                        if (t == 0xffffffffu || !ix->terms[t].documents) { // intersect.cpp:27, :38-43
                                                unknown = true;
                                                continue;
                                        }
                                        auto it = row_of.find(t);
                                        if (it == row_of.end()) {
                                                it = row_of.emplace(t, (uint32_t)row_of.size()).first;
                                                P.build.push_back(t);
                                                P.build.push_back(it->second);
                                        }
                                        P.rowtab.push_back(make_uint2(it->second, g));
                                        q.orig_mask |= 1ull << g; // :33
                                }
                        q.nrows = (uint32_t)P.rowtab.size() - q.row_first;
                        if (unknown)
                                q.orig_mask = 0; // :50-51
                        g0 += reqs[r].ngroups;
                }
                return TRI_OK;
        }
} // namespace

extern "C" int tri_isect_run(tri_index *ix, const tri_isect_request *reqs, size_t nreq, const uint32_t *terms, const uint32_t *group_first, tri_isect **out) {
        if (!ix || !reqs || !terms || !group_first || !out)
                return fail(TRI_ERR_INVALID, "tri_isect_run: null argument");
        IsectPlan P;
        if (const int rc = isect_plan(ix, reqs, nreq, terms, group_first, P))
                return rc;
        if (ix->max_doc >= 0x80000000u)
                return fail(TRI_ERR_UNSUPPORTED, "tri_isect_run: the index's docIDs reach 2^31");
        tri_dev *dev = ix->dev;
        HIP_TRY(hipSetDevice(dev->device));
        const uint32_t plw = ((ix->max_doc >> 17) + 2u) * (SPAN_BITS / 32u); // words of a row: the extent of a term plane and of d_masked (planner.hpp, filter_words)
        const uint32_t nrows = (uint32_t)(P.build.size() / 2), nspans = ix->max_doc / ISECT_SPAN + 1u, nr = (uint32_t)nreq;
        // H's slots: what the call's widest request can need — g groups make fewer than 2^g masks; twice that keeps the probes short — up to option isect_max_masks
        // (the table is cleared and read back whole: a two-token request should not pay for a sixteen-token one's).  C is keyed by (mask, epoch): it is sized after
        // pass 1, from H (below)
        uint32_t gmax = 1;
        for (size_t r = 0; r < nreq; ++r)
                gmax = std::max(gmax, reqs[r].ngroups);
        const uint64_t by_groups = gmax >= 28 ? 1ull << 30 : std::max<uint64_t>(64, 2ull << gmax);
        const uint32_t h_cap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(dev->opt.isect_max_masks, 1), by_groups);
        const uint64_t rows_bytes = (uint64_t)nrows * plw * 4u;
        // ---- scratch of the call, pass 1: ONE pooled block (write_side.hpp's way: no hipMalloc / hipFree per call once the pool is warm), carved 256 bytes apart.
        //      [H keys | H counts | flags + spills] are cleared together, [H first docIDs] is set to all ones
        auto up = [](const uint64_t x) { return (x + 255u) & ~(uint64_t)255u; };
        const uint64_t hk_b = (uint64_t)nr * h_cap * 8, h32_b = (uint64_t)nr * h_cap * 4, span_b = (uint64_t)nr * nspans * 8;
        const uint64_t o_hk = 0, o_hcnt = o_hk + up(hk_b), o_flags = o_hcnt + up(h32_b), o_hfirst = o_flags + up((uint64_t)nr * 8), o_span = o_hfirst + up(h32_b), o_build = o_span + up(span_b),
                       o_rowtab = o_build + up(P.build.size() * 4), o_reqs = o_rowtab + up(P.rowtab.size() * sizeof(uint2)), o_rows = o_reqs + up(nreq * sizeof(IsectReq)),
                       total1 = o_rows + up(rows_bytes);
        if (nrows && total1 > dev->opt.isect_max_bytes)
                return fail(TRI_ERR_UNSUPPORTED, "tri_isect_run: %u rows of %llu bytes, %u requests' tables of %u slots and %u spans: %llu bytes exceed isect_max_bytes = %llu", nrows,
                            (unsigned long long)plw * 4u, nr, h_cap, nspans, (unsigned long long)total1, (unsigned long long)dev->opt.isect_max_bytes);
        auto h = std::make_unique<tri_isect>();
        h->reqs.resize(nreq);
        h->h_size.assign(nreq, 0);
        h->c_size.assign(nreq, 0);
        h->spills.assign(nreq, 0);
        tri_isect_info &I = h->info;
        I.span_docs = ISECT_SPAN;
        I.lds_slots = ISECT_LDS_SLOTS;
        I.nreq = nr;
        I.nspans = nspans;
        I.rows = nrows;
        I.max_masks = h_cap;
        I.row_bytes = (uint64_t)plw * 4u;
        auto finish = [&]() {
                I.h_size = h->h_size.data();
                I.c_size = h->c_size.data();
                I.lds_spills = h->spills.data();
                *out = h.release();
                return TRI_OK;
        };
        if (!nrows || !nreq) // no known term anywhere: empty lists (intersect.cpp:47-48)
                return finish();

        Pooled<uint8_t> s1, s2; // the pooled blocks of this call
        HIP_TRY(s1.alloc(dev, total1));
        I.scratch_bytes = total1;
        hipStream_t st = dev->stream;
        HIP_TRY(hipMemcpyAsync(s1 + o_build, P.build.data(), P.build.size() * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(s1 + o_rowtab, P.rowtab.data(), P.rowtab.size() * sizeof(uint2), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(s1 + o_reqs, P.reqs.data(), nreq * sizeof(IsectReq), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(s1 + o_hk, 0, o_hfirst - o_hk, st));
        HIP_TRY(hipMemsetAsync(s1 + o_hfirst, 0xff, h32_b, st));
        IsectTables T{};
        T.h_key = reinterpret_cast<unsigned long long *>(s1 + o_hk);
        T.h_cnt = reinterpret_cast<uint32_t *>(s1 + o_hcnt);
        T.h_first = reinterpret_cast<uint32_t *>(s1 + o_hfirst);
        T.flags = reinterpret_cast<uint32_t *>(s1 + o_flags);
        T.spills = T.flags + nr;
        T.h_cap = h_cap;
        T.c_cap = 0;
        const uint64_t *d_rows = reinterpret_cast<const uint64_t *>(s1 + o_rows);
        const uint2 *d_rowtab = reinterpret_cast<const uint2 *>(s1 + o_rowtab);
        const IsectReq *d_reqs = reinterpret_cast<const IsectReq *>(s1 + o_reqs);
        unsigned long long *d_span = reinterpret_cast<unsigned long long *>(s1 + o_span);

        // ---- the rows: plane 0 of every distinct known term (k_term_plane0 writes every word of a row: no memset), the index's plane cache untouched
        const uint32_t nwin = plw / PL_WORDS;
        for (uint32_t y0 = 0; y0 < nrows; y0 += 65535u) {
                const uint32_t ny = std::min(65535u, nrows - y0);
                TRI_LAUNCH(k_term_plane0, ix->codec, dim3((nwin + P0_GROUP - 1) / P0_GROUP, ny), dim3(AND_WG), st, ix->d_index, ix->d_blk_last, ix->d_blk_off, ix->d_blk_rec, ix->d_blk_doff, ix->d_win,
                           ix->d_terms, reinterpret_cast<const uint32_t *>(s1 + o_build) + 2 * (size_t)y0, reinterpret_cast<uint32_t *>(s1 + o_rows), plw, (uint32_t *)nullptr);
                HIP_TRY(hipGetLastError());
        }
        // ---- pass 1
        const size_t plw64 = plw / 2;
        hipLaunchKernelGGL(k_isect_hist, dim3(nspans, nr), dim3(64), 0, st, d_rows, plw64, d_rowtab, d_reqs, (const uint32_t *)ix->d_masked, T, d_span, nspans);
        HIP_TRY(hipGetLastError());
        I.passes = 1;
        std::vector<uint64_t> hk((size_t)nr * h_cap);
        std::vector<uint32_t> hcnt((size_t)nr * h_cap), hfirst((size_t)nr * h_cap), flags((size_t)nr * 2);
        HIP_TRY(hipMemcpyAsync(hk.data(), s1 + o_hk, hk_b, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(hcnt.data(), s1 + o_hcnt, h32_b, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(hfirst.data(), s1 + o_hfirst, h32_b, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(flags.data(), s1 + o_flags, (size_t)nr * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));

        // ---- the host step: H by first docID, the thresholds (per slot of H), the epoch bounds, and what C can hold at most: a mask with a threshold adds one
        //      key per epoch from its threshold's epoch on — an exact upper bound, known before pass 2 is launched
        std::vector<std::vector<isect_rows::HEntry>> H(nreq);
        std::vector<uint32_t> thr((size_t)nr * h_cap, ISECT_NEVER), bounds;
        uint64_t c_bound = 0;
        for (size_t r = 0; r < nreq; ++r) {
                h->spills[r] = flags[nr + r];
                if (flags[r] & ISECT_OVF_MASKS) {
                        h->reqs[r].status = TRI_ERR_UNSUPPORTED;
                        P.reqs[r].skip = 1;
                        fail(TRI_ERR_UNSUPPORTED, "tri_isect_run: request %zu holds more distinct masks than its table's %u slots (option isect_max_masks)", r, h_cap);
                        continue;
                }
                std::vector<uint32_t> slot_of;
                for (uint32_t s = 0; s < h_cap; ++s)
                        if (hk[r * h_cap + s]) {
                                H[r].push_back({hk[r * h_cap + s], hcnt[r * h_cap + s], hfirst[r * h_cap + s]});
                                slot_of.push_back(s);
                        }
                h->h_size[r] = (uint32_t)H[r].size();
                std::vector<uint32_t> order(H[r].size());
                std::iota(order.begin(), order.end(), 0u);
                std::sort(order.begin(), order.end(), [&](const uint32_t a, const uint32_t b) { return H[r][a].first < H[r][b].first; });
                std::vector<isect_rows::HEntry> sorted(H[r].size());
                for (size_t i = 0; i < order.size(); ++i)
                        sorted[i] = H[r][order[i]];
                const std::vector<uint32_t> t = isect_rows::thresholds(sorted);
                P.reqs[r].bounds_off = (uint32_t)bounds.size();
                P.reqs[r].nbounds = (uint32_t)sorted.size();
                for (size_t i = 0; i < sorted.size(); ++i)
                        bounds.push_back(sorted[i].first);
                const uint64_t need = isect_rows::runs_bound(sorted, t);
                for (size_t i = 0; i < sorted.size(); ++i)
                        thr[r * h_cap + slot_of[order[i]]] = t[i];
                P.reqs[r].skip = need ? 0u : 1u;
                c_bound = std::max(c_bound, need);
                H[r] = std::move(sorted);
        }

        // ---- pass 2 (only when some mask has a strict superset: otherwise nothing is ever credited).  C's slots: twice the largest request's bound (short
        //      probes), up to option isect_max_runs — a request whose runs fit the option cannot overflow
        const bool any_run = c_bound != 0;
        const uint32_t c_cap = any_run ? (uint32_t)std::min<uint64_t>(std::max<uint64_t>(dev->opt.isect_max_runs, 1), std::max<uint64_t>(64, 2 * c_bound)) : 0u;
        I.max_runs = c_cap;
        std::vector<uint64_t> ck;
        std::vector<uint32_t> ccnt;
        if (any_run) {
                const uint64_t ck_b = (uint64_t)nr * c_cap * 8, c32_b = (uint64_t)nr * c_cap * 4;
                const uint64_t o_ck = 0, o_ccnt = o_ck + up(ck_b), o_thr = o_ccnt + up(c32_b), o_bounds = o_thr + up(h32_b), total2 = o_bounds + up(bounds.size() * 4 + 16);
                if (total1 + total2 > dev->opt.isect_max_bytes)
                        return fail(TRI_ERR_UNSUPPORTED, "tri_isect_run: the run tables (%u requests of %u slots) bring the call's scratch to %llu bytes: above isect_max_bytes = %llu", nr, c_cap,
                                    (unsigned long long)(total1 + total2), (unsigned long long)dev->opt.isect_max_bytes);
                HIP_TRY(s2.alloc(dev, total2));
                I.scratch_bytes += total2;
                T.c_key = reinterpret_cast<unsigned long long *>(s2 + o_ck);
                T.c_cnt = reinterpret_cast<uint32_t *>(s2 + o_ccnt);
                T.c_cap = c_cap;
                HIP_TRY(hipMemsetAsync(s2 + o_ck, 0, o_thr - o_ck, st));
                HIP_TRY(hipMemcpyAsync(s2 + o_thr, thr.data(), h32_b, hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemcpyAsync(s2 + o_bounds, bounds.data(), bounds.size() * 4, hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemcpyAsync(s1 + o_reqs, P.reqs.data(), nreq * sizeof(IsectReq), hipMemcpyHostToDevice, st));
                hipLaunchKernelGGL(k_isect_runs, dim3(nspans, nr), dim3(64), 0, st, d_rows, plw64, d_rowtab, d_reqs, (const uint32_t *)ix->d_masked, T, (const unsigned long long *)d_span, nspans,
                                   reinterpret_cast<const uint32_t *>(s2 + o_thr), reinterpret_cast<const uint32_t *>(s2 + o_bounds));
                HIP_TRY(hipGetLastError());
                I.passes = 2;
                ck.resize((size_t)nr * c_cap);
                ccnt.resize((size_t)nr * c_cap);
                HIP_TRY(hipMemcpyAsync(ck.data(), s2 + o_ck, ck_b, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipMemcpyAsync(ccnt.data(), s2 + o_ccnt, c32_b, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipMemcpyAsync(flags.data(), s1 + o_flags, (size_t)nr * 4, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
        }

        // ---- the replay
        for (size_t r = 0; r < nreq; ++r) {
                tri_isect::Req &R = h->reqs[r];
                if (R.status != TRI_OK)
                        continue;
                if (flags[r] & ISECT_OVF_RUNS) {
                        R.status = TRI_ERR_UNSUPPORTED;
                        fail(TRI_ERR_UNSUPPORTED, "tri_isect_run: request %zu holds more than isect_max_runs = %u (mask, epoch) runs", r, (unsigned)dev->opt.isect_max_runs);
                        continue;
                }
                std::vector<isect_rows::CEntry> Cv;
                if (any_run && !P.reqs[r].skip)
                        for (uint32_t s = 0; s < c_cap; ++s)
                                if (const uint64_t k = ck[r * c_cap + s])
                                        Cv.push_back({hk[r * h_cap + (uint32_t)(k >> 32)], (uint32_t)k, ccnt[r * c_cap + s]});
                h->c_size[r] = (uint32_t)Cv.size();
                R.results = isect_rows::replay(H[r], std::move(Cv));
                R.hist = std::move(H[r]);
                std::sort(R.hist.begin(), R.hist.end(), [](const isect_rows::HEntry &a, const isect_rows::HEntry &b) { return a.mask < b.mask; });
        }
        return finish();
}

extern "C" int tri_isect_status(const tri_isect *h, int32_t *status) {
        if (!h || !status)
                return fail(TRI_ERR_INVALID, "tri_isect_status: null argument");
        for (size_t r = 0; r < h->reqs.size(); ++r)
                status[r] = h->reqs[r].status;
        return TRI_OK;
}

namespace {
        int isect_request(const tri_isect *h, const char *what, const size_t r, const size_t *n) {
                if (!h || !n)
                        return fail(TRI_ERR_INVALID, "%s: null argument", what);
                if (r >= h->reqs.size())
                        return fail(TRI_ERR_INVALID, "%s: request %zu of %zu", what, r, h->reqs.size());
                if (h->reqs[r].status != TRI_OK)
                        return fail(TRI_ERR_UNSUPPORTED, "%s: request %zu overflowed a table (tri_isect_status)", what, r);
                return TRI_OK;
        }
} // namespace

extern "C" int tri_isect_results(const tri_isect *h, size_t r, uint64_t *masks, uint32_t *counts, size_t cap, size_t *n) {
        if (const int rc = isect_request(h, "tri_isect_results", r, n))
                return rc;
        const auto &v = h->reqs[r].results;
        if (masks || counts) {
                if (!masks || !counts)
                        return fail(TRI_ERR_INVALID, "tri_isect_results: null argument");
                if (cap < v.size())
                        return fail(TRI_ERR_INVALID, "tri_isect_results: %zu entries, room for %zu", v.size(), cap);
                for (size_t i = 0; i < v.size(); ++i) {
                        masks[i] = v[i].first;
                        counts[i] = v[i].second;
                }
        }
        *n = v.size();
        return TRI_OK;
}

extern "C" int tri_isect_histogram(const tri_isect *h, size_t r, uint64_t *masks, uint32_t *counts, uint32_t *first_docs, size_t cap, size_t *n) {
        if (const int rc = isect_request(h, "tri_isect_histogram", r, n))
                return rc;
        const auto &v = h->reqs[r].hist;
        if (masks || counts || first_docs) {
                if (!masks || !counts || !first_docs)
                        return fail(TRI_ERR_INVALID, "tri_isect_histogram: null argument");
                if (cap < v.size())
                        return fail(TRI_ERR_INVALID, "tri_isect_histogram: %zu entries, room for %zu", v.size(), cap);
                for (size_t i = 0; i < v.size(); ++i) {
                        masks[i] = v[i].mask;
                        counts[i] = v[i].count;
                        first_docs[i] = v[i].first;
                }
        }
        *n = v.size();
        return TRI_OK;
}

extern "C" int tri_isect_get_info(const tri_isect *h, tri_isect_info *info) {
        if (!h || !info)
                return fail(TRI_ERR_INVALID, "tri_isect_get_info: null argument");
        *info = h->info;
        return TRI_OK;
}

extern "C" void tri_isect_destroy(tri_isect *h) { delete h; }

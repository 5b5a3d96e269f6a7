// k_rich_rank.hpp — the default mode's device ranker: a proximity score per match from what k_rich left in HBM, top-K per task, merged per query
// Part of libtrinity_hip.so (MI355X / gfx950); included by trinity_hip.hip.  New code, no reference source.
#pragma once
#include "k_rich.hpp"

// tri_batch_set_ranker (TRI_RANK_PROXIMITY).  exec_query's default mode hands every match to consider(const matched_document &) (matches.h:109-153) with
// matchedTerms[] and their hits (queryexec_ctx.cpp:382-648), and the application scores them — usually by proximity: query tokens that follow each other in
// the query follow each other in the document (toNextSpan / dws->test(next, pos + 1)).  The two k_rich passes have written, per match, the present mask, the
// frequency row and the hit positions; k_rich_rank reads them back — it decodes nothing — and computes
//
//   score(d) = ( sum over present slots k, ascending:  w[k] * double(min(freq[k], freq_cap)) )
//              + adjacency * double( sum over k with slots k and k + 1 both present:  #{ hits h of slot k : pos(h) != 0 and pos(h) + 1 is a position of slot k + 1 } )
//
// in IEEE double, in exactly that order, uncontracted (rank_add / rank_finish), so that a sequential restatement in host doubles is bit-equal.  Position 0 is the
// position of a payload-only hit and never pairs.  A term the document lacks, or holds without the query tree sitting on it (the allow mask), has a clear
// present bit and a zero cell: it adds nothing.
//
// Work split.  One match per lane, tiles of AND_WG matches.  A match's first hit in the pool is the task's base plus the row totals of the matches before it:
// a workgroup scan per tile, carried from tile to tile (what the WRITE pass's rowoff is).  Within a match the pool is term-minor, so when slots k and k + 1
// are both present their runs lie next to each other, both ascending: the pair count is one merge walk over freq[k] + freq[k + 1] contiguous u16.  Rows are
// walked by the SET bits of the present mask (a cell is zero wherever its bit is clear), narrow and wide alike.
//   RANK_LANE_RUN = 128: a pair of runs of more hits than this together is not walked by its lane — a document may hold thousands of hits of one term
//   (positions reach 16 383), and 63 lanes would wait for one.  Such matches are queued in LDS and taken by whole waves after the lane pass: the lanes stride
//   over run k and bisect run k + 1 (64 hits per step instead of one); the owner lane adds the wave's count to its own before it scores.
// Scores are offered to the task's top-K (topk_offer / topk_prune of k_score.hpp: score descending, docID ascending — tri_batch_topk's rule) and the task's
// best K written as a partial list; k_rank_merge folds a query's tasks like k_topk_merge, but keeps the scores double (k_topk_merge narrows to float: its
// signature does not fit, and it stays as it is).
constexpr uint32_t RANK_LANE_RUN = 128;

struct RankShared {
        TopK tk;
        uint32_t scan[8];
        uint32_t rowoff[AND_WG]; // hits of the task before the lane's match
        uint32_t extra[AND_WG];  // pairs the wave pass found for the lane's match
        uint32_t longq[AND_WG];  // lanes whose match holds a pair of runs longer than RANK_LANE_RUN
        uint32_t nlong;
};

__device__ __forceinline__ double rank_add(const double sum, const double w, const uint32_t f) {
#pragma clang fp contract(off)
        const double term = w * (double)f;
        return sum + term;
}
__device__ __forceinline__ double rank_finish(const double sum, const double adjacency, const uint32_t pairs) {
#pragma clang fp contract(off)
        const double bonus = adjacency * (double)pairs;
        return sum + bonus;
}

// hits of the ascending run a[0 .. la) that are not at position 0 and whose successor position is in the ascending run b[0 .. lb): one merge walk
__device__ __forceinline__ uint32_t rank_pairs_lane(const uint16_t *__restrict__ a, const uint32_t la, const uint16_t *__restrict__ b, const uint32_t lb) {
        uint32_t j = 0, c = 0;
        for (uint32_t i = 0; i < la; ++i) {
                const uint32_t p = a[i];
                if (!p)
                        continue;
                while (j < lb && b[j] < p + 1u)
                        ++j;
                c += (j < lb && b[j] == p + 1u) ? 1u : 0u;
        }
        return c;
}

// ... the same count by a whole wave (every lane calls it with the same arguments): lanes stride over a, each bisects b; the wave's total in every lane
__device__ __forceinline__ uint32_t rank_pairs_wave(const uint16_t *__restrict__ a, const uint32_t la, const uint16_t *__restrict__ b, const uint32_t lb, const uint32_t lane) {
        uint32_t c = 0;
        for (uint32_t i = lane; i < la; i += 64) {
                const uint32_t p = a[i];
                if (!p)
                        continue;
                const uint32_t lo = first_ge(b, 0u, lb, p + 1u);
                c += (lo < lb && b[lo] == p + 1u) ? 1u : 0u;
        }
        for (int d = 32; d; d >>= 1)
                c += (uint32_t)__shfl_xor((int)c, d, 64);
        return c;
}

// the tasks sched[0 .. ntasks) of the batch's rich schedule: WIDE = false the section k_rich runs, true the one k_rich_wide runs
template <bool WIDE>
__global__ __launch_bounds__(AND_WG) void k_rich_rank(const DevQuery *__restrict__ plan, const DevTask *__restrict__ tasks, const uint32_t *__restrict__ sched, const uint32_t ntasks,
                                                      const uint32_t *__restrict__ out, const uint32_t *__restrict__ counts, const uint32_t R,
                                                      const uint32_t *__restrict__ present, const uint16_t *__restrict__ freq, const uint64_t *__restrict__ task_pos_base,
                                                      const uint16_t *__restrict__ pool, const double *__restrict__ weights /* per sterms[] entry */, const uint32_t freq_cap,
                                                      const double adjacency, const uint32_t k, uint32_t *__restrict__ part_docs, double *__restrict__ part_scores,
                                                      uint32_t *__restrict__ part_counts, const RichWideArgs wd) {
        __shared__ RankShared sh;
        const uint32_t tid = threadIdx.x;
        const uint32_t wave = uni(tid >> 6), lane = tid & 63u;
        for (uint32_t tno = blockIdx.x; tno < ntasks; tno += gridDim.x) {
                const uint32_t tix = sched[tno];
                const DevTask task = tasks[tix];
                const DevQuery q = plan[task.slot];
                if (uni(q.qid) == 0xffffffffu) { // (a hidden phrase query of a TASK_TREE query: no caller query, no row)
                        if (tid == 0)
                                part_counts[tix] = 0;
                        continue;
                }
                const uint32_t M = uni(counts[tix]);
                const uint32_t *seg = out + task.out_off;
                const uint16_t *tpool = pool + task_pos_base[tix];
                const double *w = weights + q.score_base;
                uint64_t wslot0 = 0, wcell0 = 0;
                uint32_t wstride = 0;
                if constexpr (WIDE) {
                        const DevRichWide rw = wd.tab[task.slot];
                        wstride = uni(rw.stride);
                        wslot0 = rw.slots + (task.out_off - q.out_off);
                        wcell0 = rw.cells + (task.out_off - q.out_off) * wstride;
                }
                // the present mask and the frequency row of the match at index m of the task's segment
                auto mask_of = [&](const uint32_t m) -> uint64_t {
                        uint64_t pm = present[(uint64_t)task.out_off + m];
                        if constexpr (WIDE)
                                pm |= (uint64_t)wd.present_hi[wslot0 + m] << 32;
                        return pm;
                };
                auto row_of = [&](const uint32_t m) -> const uint16_t * {
                        if constexpr (WIDE)
                                return wd.freq + wcell0 + (uint64_t)m * wstride;
                        else
                                return freq + ((uint64_t)task.out_off + m) * R;
                };
                sh.tk.n = 0;
                sh.tk.full = 0;
                uint32_t tile_base = 0; // hits of the task before this tile
                __syncthreads();
                for (uint32_t tb = 0; tb < M; tb += AND_WG) {
                        const uint32_t j = tb + tid;
                        const bool valid = j < M;
                        const uint64_t pm = valid ? mask_of(j) : 0ull;
                        const uint16_t *row = row_of(valid ? j : 0u);
                        uint32_t total_f = 0;
                        for (uint64_t m = pm; m; m &= m - 1ull)
                                total_f += row[__builtin_ctzll(m)];
                        uint32_t wtot;
                        const uint32_t ex = wave_excl_scan(total_f, wtot);
                        sh.scan[wave] = wtot;
                        sh.extra[tid] = 0;
                        if (tid == 0)
                                sh.nlong = 0;
                        __syncthreads();
                        uint32_t wbase = 0, total = 0;
                        for (uint32_t v = 0; v < AND_WG / 64; ++v) {
                                if (v < wave)
                                        wbase += sh.scan[v];
                                total += sh.scan[v];
                        }
                        const uint32_t my_off = tile_base + wbase + ex;
                        sh.rowoff[tid] = my_off;
                        tile_base += uni(total);
                        // the lane pass: the frequency sum, and the pairs of every two neighbouring runs short enough for one lane
                        double sum = 0.0;
                        uint32_t pairs = 0;
                        bool has_long = false;
                        {
                                const uint16_t *p = tpool + my_off, *prun = p;
                                uint32_t prev = 0xfffffffeu, plen = 0;
                                for (uint64_t m = pm; m; m &= m - 1ull) {
                                        const uint32_t kb = (uint32_t)__builtin_ctzll(m);
                                        const uint32_t f = row[kb];
                                        sum = rank_add(sum, w[kb], min(f, freq_cap));
                                        if (kb == prev + 1u && plen && f) {
                                                if (plen + f <= RANK_LANE_RUN)
                                                        pairs += rank_pairs_lane(prun, plen, p, f);
                                                else
                                                        has_long = true;
                                        }
                                        prev = kb;
                                        prun = p;
                                        plen = f;
                                        p += f;
                                }
                        }
                        if (has_long)
                                sh.longq[atomicAdd(&sh.nlong, 1u)] = tid;
                        __syncthreads();
                        // the wave pass: the long pairs of the queued matches, a match per wave at a time
                        const uint32_t nl = uni(sh.nlong);
                        for (uint32_t e = wave; e < nl; e += AND_WG / 64) {
                                const uint32_t lt = uni(sh.longq[e]);
                                const uint64_t lm64 = mask_of(tb + lt);
                                const uint64_t lm = (uint64_t)uni((uint32_t)lm64) | ((uint64_t)uni((uint32_t)(lm64 >> 32)) << 32);
                                const uint16_t *lrow = row_of(tb + lt);
                                const uint16_t *p = tpool + uni(sh.rowoff[lt]), *prun = p;
                                uint32_t prev = 0xfffffffeu, plen = 0, found = 0;
                                for (uint64_t m = lm; m; m &= m - 1ull) {
                                        const uint32_t kb = (uint32_t)__builtin_ctzll(m);
                                        const uint32_t f = uni(lrow[kb]);
                                        if (kb == prev + 1u && plen && f && plen + f > RANK_LANE_RUN)
                                                found += rank_pairs_wave(prun, plen, p, f, lane);
                                        prev = kb;
                                        prun = p;
                                        plen = f;
                                        p += f;
                                }
                                if (lane == 0)
                                        sh.extra[lt] = found;
                        }
                        __syncthreads();
                        const double score = rank_finish(sum, adjacency, pairs + sh.extra[tid]);
                        topk_offer(sh.tk, k, valid, score, valid ? seg[j] : 0u, sh.scan);
                }
                topk_prune(sh.tk, k, sh.scan);
                const uint32_t n = uni(sh.tk.n);
                for (uint32_t i = tid; i < n; i += AND_WG) {
                        part_docs[(uint64_t)tix * k + i] = sh.tk.d[i];
                        part_scores[(uint64_t)tix * k + i] = sh.tk.s[i];
                }
                if (tid == 0)
                        part_counts[tix] = n;
                __syncthreads();
        }
}

// one workgroup per query: the tasks' partial lists through the same top-K structure (k_topk_merge with the scores kept double); rows past the count are zero
__global__ __launch_bounds__(AND_WG) void k_rank_merge(const DevQuery *__restrict__ plan, const uint32_t nq, const uint32_t k, const uint32_t *__restrict__ part_docs,
                                                       const double *__restrict__ part_scores, const uint32_t *__restrict__ part_counts, uint32_t *__restrict__ top_docs,
                                                       double *__restrict__ top_scores, uint32_t *__restrict__ top_counts) {
        __shared__ TopK tk;
        __shared__ uint32_t scan[8];
        const uint32_t tid = threadIdx.x;
        for (uint32_t slot = blockIdx.x; slot < nq; slot += gridDim.x) {
                const DevQuery q = plan[slot];
                if (q.qid == 0xffffffffu)
                        continue;
                tk.n = 0;
                tk.full = 0;
                __syncthreads();
                for (uint32_t t = 0; t < q.ntasks; ++t) {
                        const uint32_t tix = q.first_task + t;
                        const uint32_t c = part_counts[tix];
                        for (uint32_t base = 0; base < c; base += AND_WG) {
                                const uint32_t i = base + tid;
                                const bool v = i < c;
                                topk_offer(tk, k, v, v ? part_scores[(uint64_t)tix * k + i] : 0.0, v ? part_docs[(uint64_t)tix * k + i] : 0u, scan);
                        }
                }
                topk_prune(tk, k, scan);
                const uint32_t n = uni(tk.n);
                for (uint32_t i = tid; i < k; i += AND_WG) {
                        top_docs[(uint64_t)q.qid * k + i] = i < n ? tk.d[i] : 0u;
                        top_scores[(uint64_t)q.qid * k + i] = i < n ? tk.s[i] : 0.0;
                }
                if (tid == 0)
                        top_counts[q.qid] = n;
                __syncthreads();
        }
}

// tri_cbatch_ranked: the ranked lists of a collection's parts merged per query.  Each part's [nq][k] list is sorted already (k_rank_merge: score descending,
// docID ascending), and a query holds at most nsrc * 256 entries: they are not pushed through the LDS top-K again — every entry's final rank is COUNTED.
// One lane per entry (q, s, i).  A live entry (i < count_s[q]) stands at rank i + sum over the other sources j of #{ live entries of j that precede it }, where
// "precede" is (score descending, docID ascending, source ascending): the stable sort by (-score, docID) of the parts' lists concatenated source after source
// — the older source first where two sources hold the same docID at the same score (a collection without masks).  Those that precede form a prefix of j's
// list, so the count is one lower-bound search — taken in a fixed number of steps (the bits of k's highest power of two: wave-uniform, no lane waits for
// another's longer search).  rank < k: the pair is stored at out[q][rank].  The ranks of a query's live entries are a permutation of 0 .. sum(count) - 1, and
// the lanes of source 0 zero the positions from min(sum(count), k) on: every output word is written exactly once a run — no LDS, no barrier, no atomics.
// Scores are compared as doubles with > and ==: -0.0 and 0.0 tie and the docID decides; the score stored is the part's own 64 bits.
struct DevRankSource {
        const uint32_t *docs;   // [nq][k]
        const double *scores;   // [nq][k]
        const uint32_t *counts; // [nq]
};

__global__ __launch_bounds__(AND_WG) void k_rank_merge_sources(const DevRankSource *__restrict__ src, const uint32_t nsrc, const uint32_t nq, const uint32_t k,
                                                               uint32_t *__restrict__ top_docs, double *__restrict__ top_scores, uint32_t *__restrict__ top_counts) {
        const uint64_t e = (uint64_t)blockIdx.x * AND_WG + threadIdx.x;
        const uint64_t per_q = (uint64_t)nsrc * k;
        if (e >= per_q * nq)
                return;
        const uint32_t q = (uint32_t)(e / per_q);
        const uint32_t r = (uint32_t)(e - (uint64_t)q * per_q);
        const uint32_t s = r / k, i = r - s * k;
        const uint64_t row = (uint64_t)q * k;
        uint32_t total = 0, mine = 0;
        for (uint32_t j = 0; j < nsrc; ++j) {
                const uint32_t c = min(src[j].counts[q], k);
                total += c;
                mine = j == s ? c : mine;
        }
        const uint32_t n = min(total, k);
        if (s == 0) {
                if (i >= n) {
                        top_docs[row + i] = 0u;
                        top_scores[row + i] = 0.0;
                }
                if (i == 0)
                        top_counts[q] = n;
        }
        if (i >= mine)
                return;
        const double sc = src[s].scores[row + i];
        const uint32_t doc = src[s].docs[row + i];
        const uint32_t top_step = 1u << (31 - __builtin_clz(k)); // (2 * top_step - 1 >= k: the steps reach every count up to k)
        uint32_t rank = i;
        for (uint32_t j = 0; j < nsrc; ++j) {
                if (j == s)
                        continue;
                const uint32_t c = min(src[j].counts[q], k);
                const double *js = src[j].scores + row;
                const uint32_t *jd = src[j].docs + row;
                uint32_t lo = 0; // entries of j known to precede
                for (uint32_t step = top_step; step; step >>= 1) {
                        const uint32_t at = lo + step;
                        if (at <= c) {
                                const double x = js[at - 1];
                                const uint32_t d = jd[at - 1];
                                if (x > sc || (x == sc && (d < doc || (d == doc && j < s))))
                                        lo = at;
                        }
                }
                rank += lo;
        }
        if (rank < k) {
                top_docs[row + rank] = doc;
                top_scores[row + rank] = sc;
        }
}

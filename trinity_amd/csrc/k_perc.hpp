// k_perc.hpp — the percolator's kernels (perc_side.hpp: tri_perc_match): a resident set of stored queries evaluated against a small batch of documents that
// was never indexed.  The inverse of every other kernel here: the queries are the data at rest, the documents arrive.  Part of libtrinity_hip.so (MI355X /
// gfx950, wave64); included by trinity_hip.hip behind k_tree_wide.hpp.  New code, no reference source.
//
// A ROW is one bit per document of the call, W = ceil(ndocs / 32) words (at most 8 KB); a LEAF of the set (host/perc_lower.hpp) is a distinct term the
// queries name or a distinct multi-word phrase; only the leaves the batch holds get a row.
//   k_perc_docs        a wave per document: flags the term leaves among its terms, sums its frequencies (where its positions start, after a scan)
//   k_perc_phrase_flag a thread per phrase: flagged when every word's leaf is
//   k_perc_scan_*      the exclusive scan every stage below uses (2048 elements a workgroup, three launches), k_perc_compact the list of the non-zero ones
//   k_perc_leaf_rows   flags + their scan -> the leaf's row or NONE, and the list of the phrases that get one
//   k_perc_rows        a wave per document: where each posting's positions start, and bit d of the row of each of its leaves (atomicOr)
//   k_perc_phrases     a wave per (phrase with a row, word): candidates = AND of the words' rows; per candidate document each word is found by binary search
//                      in the document's ascending terms, the lanes go over the first word's positions, PERC_PHRASE_PASS a pass
//   k_perc_select      a thread per stored query: the prune — enabled, lowered, and (one of its leaves has a row, or it holds on a document without any)
//   k_perc_eval        a wave per (candidate query, tile of 64 row words = 2048 documents): tree_fold.hpp's fold, the record read through uniform loads,
//                      the stack a few LDS words a lane; masked to ndocs at the root; the match words and a popcount per query
//   k_perc_fill_q      a wave per query that hit: its pairs, query-major
//   k_perc_seg_count / k_perc_fill_d   a wave per (segment of PERC_SEG hit queries, word): per document the segment's matches — ballots over the lanes'
//                      words —, scanned document-major, then the same walk writes each document's run in ascending query order (ballot + mbcnt)
// Every index below is bounded by a count the host passed or a count read from the scan's total; a row index is checked against the rows the call allocated.
#pragma once

constexpr uint32_t PERC_NONE = 0xffffffffu;
constexpr uint32_t PERC_WG = 256;         // the flat kernels: four waves
constexpr uint32_t PERC_TILE_WORDS = 64;  // row words a wave of k_perc_eval takes: a word per lane
constexpr uint32_t PERC_PHRASE_PASS = 64; // positions of a phrase's first word a wave of k_perc_phrases checks per pass: one per lane
constexpr uint32_t PERC_SEG = 1024;       // hit queries per segment of the document-major fill
constexpr uint32_t PERC_SCAN_PER_THREAD = 8, PERC_SCAN_BLOCK = PERC_WG * PERC_SCAN_PER_THREAD;
constexpr uint32_t PERC_Q_RUNS = 1u, PERC_Q_ABSENT = 2u, PERC_Q_ENABLED = 4u; // host/perc_lower.hpp: Q_*

// the set, resident
struct PercSet {
        const uint32_t *recs, *rec_off, *qflags, *qleaf_first, *qleaves, *term_leaf, *leaf_term, *phrase_first, *phrase_leaves;
        uint32_t nq, nterms, nT, nP;
};
// the batch
struct PercDocs {
        const uint32_t *dfirst, *terms, *freqs; // dfirst[ndocs + 1]: rebased to the call's first posting
        const uint16_t *positions;
        uint32_t ndocs, W;
};

// ---- block-wide exclusive scan of one value per thread (every thread of the workgroup calls it: wave_prims.hpp's contract); returns the prefix, total = the block's sum
__device__ __forceinline__ uint32_t perc_block_scan(uint32_t *red /* [PERC_WG / 64 + 1] */, const uint32_t v, uint32_t &total) {
        uint32_t wtot;
        const uint32_t ex = wave_excl_scan(v, wtot);
        const uint32_t wave = threadIdx.x >> 6;
        __syncthreads(); // (red may still be read from an earlier call)
        if ((threadIdx.x & 63u) == 0)
                red[wave] = wtot;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t k = 0; k < PERC_WG / 64; ++k) {
                const uint32_t t = red[k];
                before += k < wave ? t : 0u;
                all += t;
        }
        total = all;
        return ex + before;
}
template <bool NZ>
__device__ __forceinline__ uint32_t perc_scan_in(const uint32_t v) {
        return NZ ? (v != 0u) : v;
}
// sums[b] = the sum of block b's elements
template <bool NZ>
__global__ __launch_bounds__(PERC_WG) void k_perc_scan_sums(const uint32_t *__restrict__ in, const uint32_t n, uint32_t *__restrict__ sums) {
        __shared__ uint32_t red[PERC_WG / 64 + 1];
        const uint32_t base = blockIdx.x * PERC_SCAN_BLOCK + threadIdx.x * PERC_SCAN_PER_THREAD;
        uint32_t s = 0;
        for (uint32_t k = 0; k < PERC_SCAN_PER_THREAD; ++k)
                if (base + k < n)
                        s += perc_scan_in<NZ>(in[base + k]);
        uint32_t total;
        perc_block_scan(red, s, total);
        if (threadIdx.x == 0)
                sums[blockIdx.x] = total;
}
// one workgroup: sums[] becomes its exclusive scan; total[0 .. 1] = the sum of everything, 64 bits
__global__ __launch_bounds__(PERC_WG) void k_perc_scan_tops(uint32_t *__restrict__ sums, const uint32_t nb, uint32_t *__restrict__ total) {
        __shared__ uint32_t red[PERC_WG / 64 + 1];
        __shared__ unsigned long long part[PERC_WG / 64];
        uint32_t run = 0;            // the offsets: 32 bits
        unsigned long long mine = 0; // the total, this thread's share: ONE round of 256 block sums can reach 2^32 and more, so the round's 32-bit `tot` cannot carry it
        for (uint32_t b0 = 0; b0 < nb; b0 += PERC_WG) { // (uniform)
                const uint32_t i = b0 + threadIdx.x;
                const uint32_t v = i < nb ? sums[i] : 0u;
                uint32_t tot;
                const uint32_t ex = perc_block_scan(red, v, tot);
                if (i < nb)
                        sums[i] = run + ex; // (a call of 2^32 pairs or more is refused from total[]: the wrapped offsets are never used)
                run += tot;
                mine += v;
        }
        for (int k = 32; k; k >>= 1)
                mine += __shfl_xor(mine, k);
        if ((threadIdx.x & 63u) == 0)
                part[threadIdx.x >> 6] = mine;
        __syncthreads();
        if (threadIdx.x == 0) {
                unsigned long long all = 0;
                for (uint32_t k = 0; k < PERC_WG / 64; ++k)
                        all += part[k];
                total[0] = (uint32_t)all;
                total[1] = (uint32_t)(all >> 32);
        }
}
// out[i] = the sum of the elements before i (in == out is fine: a thread reads its elements before it writes them)
template <bool NZ>
__global__ __launch_bounds__(PERC_WG) void k_perc_scan_apply(const uint32_t *in, const uint32_t n, const uint32_t *__restrict__ sums, uint32_t *out) {
        __shared__ uint32_t red[PERC_WG / 64 + 1];
        const uint32_t base = blockIdx.x * PERC_SCAN_BLOCK + threadIdx.x * PERC_SCAN_PER_THREAD;
        uint32_t v[PERC_SCAN_PER_THREAD], s = 0;
        for (uint32_t k = 0; k < PERC_SCAN_PER_THREAD; ++k) {
                v[k] = base + k < n ? perc_scan_in<NZ>(in[base + k]) : 0u;
                s += v[k];
        }
        uint32_t total;
        uint32_t at = perc_block_scan(red, s, total) + sums[blockIdx.x];
        for (uint32_t k = 0; k < PERC_SCAN_PER_THREAD; ++k) {
                if (base + k < n)
                        out[base + k] = at;
                at += v[k];
        }
}
// list[off[i]] = i for every i whose flag is non-zero (off: the exclusive scan of the flags): ascending
__global__ __launch_bounds__(PERC_WG) void k_perc_compact(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ off, const uint32_t n, uint32_t *__restrict__ list,
                                                          const uint32_t cap) {
        const uint32_t i = blockIdx.x * PERC_WG + threadIdx.x;
        if (i < n && flag[i] && off[i] < cap)
                list[off[i]] = i;
}

// ---- the documents, pass 1.  A wave per document; grid: ceil(ndocs / 4)
__global__ __launch_bounds__(PERC_WG) void k_perc_docs(const PercDocs D, const uint32_t *__restrict__ term_leaf, const uint32_t nterms, uint32_t *__restrict__ leaf_flag,
                                                       uint32_t *__restrict__ dsum) {
        const uint32_t lane = threadIdx.x & 63u, d = uni(blockIdx.x * (PERC_WG / 64) + (threadIdx.x >> 6));
        if (d >= D.ndocs)
                return; // (the whole wave)
        const uint32_t lo = uni(D.dfirst[d]), hi = uni(D.dfirst[d + 1]);
        uint32_t s = 0;
        for (uint32_t i0 = lo; i0 < hi; i0 += 64u) { // (uniform)
                const uint32_t i = i0 + lane;
                if (i < hi) {
                        s += D.freqs[i];
                        const uint32_t t = D.terms[i];
                        if (t < nterms) {
                                const uint32_t l = term_leaf[t];
                                if (l != PERC_NONE)
                                        leaf_flag[l] = 1u; // (every writer stores the same value)
                        }
                }
        }
        uint32_t total;
        wave_excl_scan(s, total);
        if (lane == 0)
                dsum[d] = total;
}
__global__ __launch_bounds__(PERC_WG) void k_perc_phrase_flag(const PercSet S, uint32_t *__restrict__ leaf_flag) {
        const uint32_t p = blockIdx.x * PERC_WG + threadIdx.x;
        if (p >= S.nP)
                return;
        uint32_t all = 1u;
        for (uint32_t k = S.phrase_first[p]; k < S.phrase_first[p + 1]; ++k)
                all &= leaf_flag[S.phrase_leaves[k]];
        leaf_flag[S.nT + p] = all;
}
// leaf_off: the scan of the flags.  leaf_row[l]: the leaf's row, or NONE; plist: the phrases with a row, ascending
__global__ __launch_bounds__(PERC_WG) void k_perc_leaf_rows(const uint32_t *__restrict__ leaf_flag, const uint32_t *__restrict__ leaf_off, const uint32_t nT, const uint32_t nL,
                                                            const uint32_t rows_cap, uint32_t *__restrict__ leaf_row, uint32_t *__restrict__ plist) {
        const uint32_t l = blockIdx.x * PERC_WG + threadIdx.x;
        if (l >= nL)
                return;
        const uint32_t off = leaf_off[l];
        const bool has = leaf_flag[l] && off < rows_cap;
        if (has && l >= nT)
                plist[off - leaf_off[nT]] = l - nT; // (at most nP entries: off - leaf_off[nT] counts the flagged phrases before this one)
        leaf_row[l] = has ? off : PERC_NONE;
}

// ---- the documents, pass 2: rows.  A wave per document; dbase: the scan of dsum
__global__ __launch_bounds__(PERC_WG) void k_perc_rows(const PercDocs D, const uint32_t *__restrict__ term_leaf, const uint32_t nterms, const uint32_t *__restrict__ leaf_row,
                                                       const uint32_t *__restrict__ dbase, uint32_t *__restrict__ pos_first, uint32_t *__restrict__ rows) {
        const uint32_t lane = threadIdx.x & 63u, d = uni(blockIdx.x * (PERC_WG / 64) + (threadIdx.x >> 6));
        if (d >= D.ndocs)
                return;
        const uint32_t lo = uni(D.dfirst[d]), hi = uni(D.dfirst[d + 1]);
        uint32_t run = uni(dbase[d]);
        for (uint32_t i0 = lo; i0 < hi; i0 += 64u) { // (uniform)
                const uint32_t i = i0 + lane;
                const bool in = i < hi;
                uint32_t tot;
                const uint32_t ex = wave_excl_scan(in ? D.freqs[i] : 0u, tot);
                if (in) {
                        pos_first[i] = run + ex;
                        const uint32_t t = D.terms[i];
                        if (t < nterms) {
                                const uint32_t l = term_leaf[t];
                                const uint32_t r = l != PERC_NONE ? leaf_row[l] : PERC_NONE;
                                if (r != PERC_NONE)
                                        atomicOr(&rows[(size_t)r * D.W + (d >> 5)], 1u << (d & 31u));
                        }
                }
                run += tot;
        }
}

// ---- the phrases with a row.  A wave per (phrase of plist, word); nrows_total[0] - leaf_row-scan at nT = how many plist holds (read from the device: `nplist`)
// (the bisections are dev_search.hpp's first_ge: over a document's ascending terms, over a posting's positions)
__device__ __forceinline__ bool perc_has_position(const uint16_t *__restrict__ a, const uint32_t lo, const uint32_t hi, const uint32_t x) {
        const uint32_t i = first_ge(a, lo, hi, x);
        return i < hi && a[i] == x;
}
__global__ __launch_bounds__(PERC_WG) void k_perc_phrases(const PercSet S, const PercDocs D, const uint32_t *__restrict__ leaf_row, const uint32_t *__restrict__ plist,
                                                          const uint32_t nplist, const uint32_t *__restrict__ pos_first, uint32_t *__restrict__ rows) {
        const uint32_t lane = threadIdx.x & 63u;
        const uint64_t ntasks = (uint64_t)nplist * D.W;
        for (uint64_t task = (uint64_t)blockIdx.x * (PERC_WG / 64) + (threadIdx.x >> 6); task < ntasks; task += (uint64_t)gridDim.x * (PERC_WG / 64)) {
                const uint32_t p = uni(plist[task / D.W]), w = uni((uint32_t)(task % D.W));
                const uint32_t k0 = uni(S.phrase_first[p]), n = uni(S.phrase_first[p + 1]) - k0;
                const uint32_t out_row = uni(leaf_row[S.nT + p]);
                if (out_row == PERC_NONE || n > 64u)
                        continue;
                uint32_t cand = 0xffffffffu;
                for (uint32_t j = 0; j < n; ++j) {
                        const uint32_t r = uni(leaf_row[S.phrase_leaves[k0 + j]]);
                        cand &= r != PERC_NONE ? uni(rows[(size_t)r * D.W + w]) : 0u;
                }
                uint32_t out = 0;
                while (cand) { // (uniform)
                        const uint32_t b = (uint32_t)__builtin_ctz(cand), d = w * 32u + b;
                        cand &= cand - 1u;
                        const uint32_t lo = uni(D.dfirst[d]), hi = uni(D.dfirst[d + 1]);
                        // lane j < n: where word j's positions lie in this document (its bit in the word's row says the term is there)
                        uint32_t start = 0, count = 0;
                        if (lane < n) {
                                const uint32_t t = S.leaf_term[S.phrase_leaves[k0 + lane]];
                                const uint32_t i = first_ge(D.terms, lo, hi, t);
                                if (i < hi && D.terms[i] == t) {
                                        start = pos_first[i];
                                        count = D.freqs[i];
                                }
                        }
                        const uint32_t s0 = (uint32_t)__builtin_amdgcn_readlane((int)start, 0), c0 = (uint32_t)__builtin_amdgcn_readlane((int)count, 0);
                        bool found = false;
                        for (uint32_t k = 0; k < c0 && !found; k += PERC_PHRASE_PASS) { // (uniform)
                                const uint32_t pos = k + lane < c0 ? D.positions[s0 + k + lane] : 0u;
                                bool ok = pos != 0u; // position 0 starts no phrase
                                for (uint32_t j = 1; j < n; ++j) {
                                        const uint32_t sj = (uint32_t)__builtin_amdgcn_readlane((int)start, j), cj = (uint32_t)__builtin_amdgcn_readlane((int)count, j);
                                        ok = ok && pos + j <= 0xffffu && perc_has_position(D.positions, sj, sj + cj, pos + j);
                                }
                                found = __ballot(ok) != 0ull;
                        }
                        out |= found ? 1u << b : 0u;
                }
                if (lane == 0)
                        rows[(size_t)out_row * D.W + w] = out;
        }
}

// ---- the prune.  A thread per stored query
__global__ __launch_bounds__(PERC_WG) void k_perc_select(const PercSet S, const uint32_t *__restrict__ leaf_row, const uint32_t prune, uint32_t *__restrict__ sel) {
        const uint32_t q = blockIdx.x * PERC_WG + threadIdx.x;
        if (q >= S.nq)
                return;
        const uint32_t fl = S.qflags[q];
        bool take = (fl & (PERC_Q_RUNS | PERC_Q_ENABLED)) == (PERC_Q_RUNS | PERC_Q_ENABLED);
        if (take && prune && !(fl & PERC_Q_ABSENT)) {
                take = false;
                for (uint32_t k = S.qleaf_first[q]; k < S.qleaf_first[q + 1] && !take; ++k)
                        take = leaf_row[S.qleaves[k]] != PERC_NONE;
        }
        sel[q] = take ? 1u : 0u;
}

// ---- the fold.  One wave a workgroup; a task = (candidate, tile), drawn by a flat index
// (the stack: dynamic LDS, `stack_words` columns of 64 lanes — the deepest any record of the SET needs, host/perc_lower.hpp: a set of three-node queries
//  takes 512 bytes a wave where TREE_WIDE_STACK words would take 16 KB)
__global__ __launch_bounds__(64) void k_perc_eval(const PercSet S, const uint32_t *__restrict__ cand, const uint32_t ncand, const uint32_t *__restrict__ leaf_row,
                                                  const uint32_t *__restrict__ rows, const uint32_t ndocs, const uint32_t W, const uint32_t stack_words, uint32_t *__restrict__ mw,
                                                  uint32_t *__restrict__ qcount) {
        extern __shared__ uint32_t perc_stk[]; // [stack_words][64]
        const uint32_t lane = threadIdx.x, tiles = (W + PERC_TILE_WORDS - 1) / PERC_TILE_WORDS;
        const uint64_t ntasks = (uint64_t)ncand * tiles;
        for (uint64_t task = blockIdx.x; task < ntasks; task += gridDim.x) {
                const uint32_t ci = (uint32_t)(task / tiles), w = (uint32_t)(task % tiles) * PERC_TILE_WORDS + lane;
                const uint32_t q = uni(cand[ci]);
                const uint32_t *rec = S.recs + uni(S.rec_off[q]);
                const uint32_t nn = min(uni(rec[0]), TREE_WIDE_MAX_NODES);
                const uint4 *node4 = reinterpret_cast<const uint4 *>(rec + TREE_HDR_WORDS);
                const bool in = w < W;
                uint32_t m = tree_wide_fold<true>(
                        nn, [&](const uint32_t n, uint4 &a, uint4 &b) { a = node4[2 * n], b = node4[2 * n + 1]; },
                        [&](const uint4 &a) {
                                const uint32_t r = uni(leaf_row[uni(a.z)]); // a leaf without a row: absent from every document of the batch
                                return r != PERC_NONE && in ? rows[(size_t)r * W + w] : 0u;
                        },
                        [&](const uint32_t slot) -> uint32_t & { return perc_stk[min(slot, stack_words - 1u) * 64u + lane]; });
                // the root: a negation holds on the documents beyond ndocs too — none of them is one
                const uint32_t tail = ndocs & 31u;
                m &= !in ? 0u : (w == W - 1u && tail) ? (1u << tail) - 1u : 0xffffffffu;
                if (in)
                        mw[(size_t)ci * W + w] = m;
                uint32_t total;
                wave_excl_scan((uint32_t)__popc(m), total);
                if (lane == 0 && total)
                        atomicAdd(&qcount[ci], total);
        }
}

// ---- the pairs, query-major.  A wave per query that hit; qoff: the scan of qcount
__global__ __launch_bounds__(PERC_WG) void k_perc_fill_q(const uint32_t *__restrict__ cand, const uint32_t *__restrict__ hits, const uint32_t nhit, const uint32_t *__restrict__ qoff,
                                                         const uint32_t *__restrict__ mw, const uint32_t W, const uint32_t npairs, uint32_t *__restrict__ out_q, uint32_t *__restrict__ out_d) {
        const uint32_t lane = threadIdx.x & 63u, nwaves = gridDim.x * (PERC_WG / 64);
        for (uint32_t h = uni(blockIdx.x * (PERC_WG / 64) + (threadIdx.x >> 6)); h < nhit; h += nwaves) {
                const uint32_t ci = uni(hits[h]), q = uni(cand[ci]);
                uint32_t run = uni(qoff[ci]);
                for (uint32_t w0 = 0; w0 < W; w0 += 64u) { // (uniform)
                        const uint32_t w = w0 + lane;
                        uint32_t m = w < W ? mw[(size_t)ci * W + w] : 0u, tot;
                        uint32_t o = run + wave_excl_scan((uint32_t)__popc(m), tot);
                        for (; m && o < npairs; m &= m - 1u, ++o) {
                                out_q[o] = q;
                                out_d[o] = w * 32u + (uint32_t)__builtin_ctz(m);
                        }
                        run += tot;
                }
        }
}

// ---- the pairs, document-major.  A wave per (segment of the hit list, word)
__device__ __forceinline__ uint32_t perc_rank(const uint64_t mask) { // the lanes below this one in the mask
        return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
// segcnt[(w * 32 + b) * nseg + seg] = the segment's queries that match document w * 32 + b
__global__ __launch_bounds__(PERC_WG) void k_perc_seg_count(const uint32_t *__restrict__ hits, const uint32_t nhit, const uint32_t *__restrict__ mw, const uint32_t W, const uint32_t nseg,
                                                            uint32_t *__restrict__ segcnt) {
        const uint32_t lane = threadIdx.x & 63u;
        const uint64_t task = (uint64_t)blockIdx.x * (PERC_WG / 64) + (threadIdx.x >> 6);
        if (task >= (uint64_t)nseg * W)
                return;
        const uint32_t seg = uni((uint32_t)(task / W)), w = uni((uint32_t)(task % W));
        uint32_t cnt[32];
#pragma unroll
        for (uint32_t b = 0; b < 32; ++b)
                cnt[b] = 0;
        const uint32_t h_end = min(nhit, (seg + 1u) * PERC_SEG);
        for (uint32_t h0 = seg * PERC_SEG; h0 < h_end; h0 += 64u) { // (uniform)
                const uint32_t h = h0 + lane;
                const uint32_t word = h < h_end ? mw[(size_t)hits[h] * W + w] : 0u;
#pragma unroll
                for (uint32_t b = 0; b < 32; ++b)
                        cnt[b] += (uint32_t)__popcll(__ballot((word >> b) & 1u));
        }
        uint32_t mine = 0;
#pragma unroll
        for (uint32_t b = 0; b < 32; ++b)
                mine = lane == b ? cnt[b] : mine;
        if (lane < 32u)
                segcnt[(size_t)(w * 32u + lane) * nseg + seg] = mine;
}
// segoff: the scan of segcnt — a document's run begins at segoff[d * nseg], the segment's share of it at segoff[d * nseg + seg]
__global__ __launch_bounds__(PERC_WG) void k_perc_fill_d(const uint32_t *__restrict__ cand, const uint32_t *__restrict__ hits, const uint32_t nhit, const uint32_t *__restrict__ mw,
                                                         const uint32_t W, const uint32_t nseg, const uint32_t *__restrict__ segoff, const uint32_t npairs, uint32_t *__restrict__ out_q,
                                                         uint32_t *__restrict__ out_d) {
        const uint32_t lane = threadIdx.x & 63u;
        const uint64_t task = (uint64_t)blockIdx.x * (PERC_WG / 64) + (threadIdx.x >> 6);
        if (task >= (uint64_t)nseg * W)
                return;
        const uint32_t seg = uni((uint32_t)(task / W)), w = uni((uint32_t)(task % W));
        uint32_t at[32];
#pragma unroll
        for (uint32_t b = 0; b < 32; ++b)
                at[b] = uni(segoff[(size_t)(w * 32u + b) * nseg + seg]);
        const uint32_t h_end = min(nhit, (seg + 1u) * PERC_SEG);
        for (uint32_t h0 = seg * PERC_SEG; h0 < h_end; h0 += 64u) { // (uniform)
                const uint32_t h = h0 + lane;
                const uint32_t ci = h < h_end ? hits[h] : 0u;
                const uint32_t word = h < h_end ? mw[(size_t)ci * W + w] : 0u, q = h < h_end ? cand[ci] : 0u;
#pragma unroll
                for (uint32_t b = 0; b < 32; ++b) {
                        const uint64_t mask = __ballot((word >> b) & 1u);
                        const uint32_t o = at[b] + perc_rank(mask);
                        if (((word >> b) & 1u) && o < npairs) {
                                out_q[o] = q;
                                out_d[o] = w * 32u + b;
                        }
                        at[b] += (uint32_t)__popcll(mask);
                }
        }
}
// dstart[d] = where document d's run begins, d = 0 .. ndocs (the last: the pairs)
__global__ __launch_bounds__(PERC_WG) void k_perc_doc_starts(const uint32_t *__restrict__ segoff, const uint32_t nseg, const uint32_t ndocs, const uint32_t W, const uint32_t npairs,
                                                             uint32_t *__restrict__ dstart) {
        const uint32_t d = blockIdx.x * PERC_WG + threadIdx.x;
        if (d <= ndocs)
                dstart[d] = d < W * 32u ? segoff[(size_t)d * nseg] : npairs;
}

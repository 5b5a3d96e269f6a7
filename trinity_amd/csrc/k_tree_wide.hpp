// k_tree_wide.hpp — TASK_TREE queries with WIDE records (dev_structs.hpp: DevTreeNodeW): trees of more than TREE_MAX_NODES nodes, up to
// TREE_WIDE_MAX_NODES (option tree_max_nodes) — a flat OR of 70 terms, an AND of 22 three-term ORs, a matchsome over 100 alternatives: a prefix
// expanded to every term that carries it, a rewrite's alternatives per token.  Part of libtrinity_hip.so (MI355X / gfx950); included by
// trinity_hip.hip behind k_tree.hpp.  New code, no reference source.
//
// k_tree.hpp's kernels keep a value per NODE: an LDS word per node per thread (k_tree_eval), a bit of a 64-bit word per node per match
// (k_tree_leaves) — that is where its 64 comes from.  Here a tree is a FOLD over its postfix node list, and what a thread keeps grows with the
// tree's DEPTH: a node that completes is handed to its parent at once —
//   * the first child (ord == 0) BECOMES the parent's accumulator, pushed on the thread's stack: a word for AND / OR / NOT / OPT, the parent's
//     counter planes (a bit-sliced count of the children that hold, seeded with the child's word) for a matchsome;
//   * a later child is folded into the accumulator on top: &=, |=, &= ~v (NOT's excluded side), nothing (OPT's optional side), a ripple add;
//   * when the list reaches the parent itself its accumulator is on top: popped, a matchsome's planes compared with its threshold.
// The node list is the same for every thread of the workgroup, so the stack pointer is uniform and the stack is LDS columns, one per thread.  The
// planner (lower_tree) works out the deepest stack a record needs — header word 2 — and leaves out a tree that needs more than TREE_WIDE_STACK.
//   k_tree_eval_wide     k_tree_eval's grid, arguments and output (qbits, chunk_counts).  Static LDS: the record 32 KB + stk[64][256] 64 KB = 96 KB
//   k_tree_leaves_wide   k_tree_leaves' grid, arguments and output (all_scores, allow).  Per match the same fold over BITS with a count per open
//                        inner node (header word 3: the depth), every node's value kept as a bit of an LDS column, turned into "an iterator sits
//                        here" top-down in place, and the reached leaves scored in node order, in double — the stream k_tree_leaves gives for the
//                        same tree.  Static LDS: the record 32 KB + bits[32][256] 32 KB + cnt[64][256] 64 KB = 128 KB
// (a workgroup may declare 160 KB on gfx950).  k_tree_expand, k_tree_gather, k_tree_topk, k_term_planes and k_rich read no node record: as they are.
#pragma once
#include "tree_fold.hpp" // the fold itself (tree_wide_fold, tree_wide_slot): k_perc.hpp runs it too

struct TreeWideNodes {
        uint4 node4[2 * TREE_WIDE_MAX_NODES]; // DevTreeNodeW as two 16-byte halves: a { op | cbits << 8 | parent << 16, arg, row, score }, b { rmask, ord | nkids << 16, thr | pop << 16 | pcbits << 24, pad (a leaf: the report mask's high word) }
        uint32_t red[TREE_WG / 64];
};
static_assert(sizeof(DevTreeNodeW) == 2 * sizeof(uint4), "a node is two 16-byte loads");

// the query's wide record into LDS (every thread of the workgroup calls it); returns the node count
__device__ __forceinline__ uint32_t tree_wide_load(TreeWideNodes &sh, const uint32_t *__restrict__ rec) {
        const uint32_t nn = min(uni(rec[0]), TREE_WIDE_MAX_NODES);
        const uint4 *src = reinterpret_cast<const uint4 *>(rec + TREE_HDR_WORDS); // (records start at multiples of eight words of a 64-byte aligned section)
        for (uint32_t i = threadIdx.x; i < 2 * nn; i += TREE_WG)
                sh.node4[i] = src[i];
        __syncthreads();
        return nn;
}
// plane A of a leaf's row
__device__ __forceinline__ const uint32_t *tree_wide_row(const uint32_t row, const uint32_t *__restrict__ trows, const uint32_t *__restrict__ prows, const uint32_t plw) {
        return (row & TREE_ROW_PHRASE) ? prows + (size_t)(row & ~TREE_ROW_PHRASE) * plw : trows + (size_t)row * PL_PLANES * plw;
}
// ---- the tree per bitmap word.  grid: (chunks of the docID space, wide tree queries); sched[y]: the query's task
struct TreeEvalWideShared {
        TreeWideNodes t;
        uint32_t stk[TREE_WIDE_STACK][TREE_WG]; // per thread a column: the accumulators of the inner nodes that are open
};
__global__ __launch_bounds__(TREE_WG) void k_tree_eval_wide(const DevQuery *__restrict__ plan, const DevTask *__restrict__ tasks, const uint32_t *__restrict__ sched,
                                                            const uint32_t *__restrict__ tree, const uint32_t *__restrict__ trows, const uint32_t *__restrict__ prows,
                                                            const uint32_t *__restrict__ masked_, uint32_t *__restrict__ qbits, uint32_t *__restrict__ chunk_counts,
                                                            const uint32_t plw, const FilterSel fsel) {
        __shared__ TreeEvalWideShared sh;
        const uint32_t tid = threadIdx.x, chunk = blockIdx.x, nchunks = gridDim.x, qi = blockIdx.y;
        const uint32_t slot = tasks[sched[qi]].slot;
        const DevQuery q = plan[slot];
        // the root drops the index's masked documents and the query's own filter (its hidden phrase queries ran against the mask alone)
        const uint32_t *const masked = filter_pick_if(masked_, fsel, uni(slot));
        const uint32_t nn = tree_wide_load(sh.t, tree + q.fused_idx);
        uint32_t count = 0;
        for (uint32_t pass = 0; pass < TREE_PASSES; ++pass) {
                const uint32_t w = chunk * TREE_CHUNK_WORDS + pass * TREE_WG + tid;
                if (w >= plw)
                        continue;
                uint32_t m = tree_wide_fold<false>(
                        nn, [&](const uint32_t n, uint4 &a, uint4 &b) { a = sh.t.node4[2 * n], b = sh.t.node4[2 * n + 1]; },
                        [&](const uint4 &a) { return tree_wide_row(uni(a.z), trows, prows, plw)[w]; }, [&](const uint32_t slot) -> uint32_t & { return sh.stk[slot][tid]; });
                if (masked) // masked_documents_registry::test (docidupdates.h:90-119): documents updated / deleted elsewhere never match
                        m &= ~masked[w];
                qbits[(size_t)qi * plw + w] = m;
                count += __popc(m);
        }
        const uint32_t total = tree_block_sum(sh.t, count);
        if (tid == 0)
                chunk_counts[(size_t)qi * nchunks + chunk] = total;
}

// ---- per match: which leaves' iterators sit on it, what they score / report.  Same grid (a workgroup takes the matches of its chunk)
struct TreeLeavesWideShared {
        TreeWideNodes t;
        uint32_t bits[TREE_WIDE_MAX_NODES / 32][TREE_WG]; // per thread a column: a bit per node — its value for the match, then "reached"
        uint32_t cnt[TREE_WIDE_STACK][TREE_WG];           // per thread a column: per open inner node, its children that hold (NOT / OPT: the node's value so far)
};
template <int CODEC>
__global__ __launch_bounds__(TREE_WG) void k_tree_leaves_wide(const uint8_t *__restrict__ index, const uint32_t *__restrict__ blk_last, const uint32_t *__restrict__ blk_off,
                                                              const DevTerm *__restrict__ terms, const DevQuery *__restrict__ plan, const DevTask *__restrict__ tasks,
                                                              const uint32_t *__restrict__ sched, const uint32_t *__restrict__ tree, const uint32_t *__restrict__ trows,
                                                              const uint32_t *__restrict__ prows, const uint32_t *__restrict__ chunk_counts, const uint32_t *__restrict__ out,
                                                              const uint32_t *__restrict__ counts, const double *__restrict__ sweights, const double *__restrict__ pscore,
                                                              double *__restrict__ all_scores, uint32_t *__restrict__ allow, const uint32_t plw, const int sim,
                                                              uint32_t *__restrict__ allow_hi, const DevRichWide *__restrict__ rwide) {
        // (allow_hi / rwide: as in k_tree_leaves — the high word of a wide-report query's report masks)
        __shared__ TreeLeavesWideShared sh;
        const uint32_t tid = threadIdx.x, chunk = blockIdx.x, nchunks = gridDim.x, qi = blockIdx.y;
        const uint32_t slot = tasks[sched[qi]].slot;
        const DevQuery q = plan[slot];
        uint32_t *hi = nullptr;
        if (allow_hi && rwide[slot].stride)
                hi = allow_hi + rwide[slot].slots;
        const uint32_t nn = tree_wide_load(sh.t, tree + q.fused_idx);
        const uint32_t *cc = chunk_counts + (size_t)qi * nchunks;
        const uint32_t base = tree_chunk_base(sh.t, cc, chunk), cnt = uni(cc[chunk]);
        if (!nn)
                return;
        for (uint32_t j = tid; j < cnt; j += TREE_WG) {
                if (base + j >= q.out_cap)
                        break;
                const uint64_t o = q.out_off + base + j;
                const uint32_t doc = out[o], wi = doc >> 5, bit = doc & 31u;
                // node values for this document, leaves up: the fold of k_tree_eval_wide over one bit
                uint32_t sp = 0, cur = 0;
                for (uint32_t n = 0; n < nn; ++n) {
                        const uint4 a = sh.t.node4[2 * n], b = sh.t.node4[2 * n + 1];
                        const uint32_t op = a.x & 0xffu;
                        uint32_t v;
                        if (op == TRI_OP_TERM || op == TRI_OP_PHRASE)
                                v = (tree_wide_row(a.z, trows, prows, plw)[wi] >> bit) & 1u;
                        else {
                                const uint32_t c = sh.cnt[tree_wide_slot(--sp)][tid], nk = b.y >> 16;
                                v = op == TRI_OP_AND ? c == nk : op == TRI_OP_SOME ? c >= (b.z & 0xffffu) : c != 0u; // (OR: any; NOT / OPT: the value the sides left)
                        }
                        cur |= v << (n & 31u);
                        if ((n & 31u) == 31u || n + 1 == nn) {
                                sh.bits[n >> 5][tid] = cur;
                                cur = 0;
                        }
                        if ((a.x >> 16) == TREE_NO_PARENT)
                                continue;
                        const uint32_t ord = b.y & 0xffffu, pop = (b.z >> 16) & 0xffu;
                        if (ord == 0)
                                sh.cnt[tree_wide_slot(sp++)][tid] = v;
                        else if (pop == TRI_OP_NOT)
                                sh.cnt[tree_wide_slot(sp - 1)][tid] &= v ^ 1u;
                        else if (pop != TRI_OP_OPT)
                                sh.cnt[tree_wide_slot(sp - 1)][tid] += v;
                }
                // reached nodes, root down, in place: the iterators the reference's recursion visits on this document (a parent comes after its children in the
                // list, so its bit already says "reached" when a child reads it, and the child's own still says "holds")
                cur = 0;
                for (uint32_t n = nn; n-- > 0;) {
                        if ((n & 31u) == 31u || n + 1 == nn)
                                cur = sh.bits[n >> 5][tid];
                        const uint4 a = sh.t.node4[2 * n], b = sh.t.node4[2 * n + 1];
                        const uint32_t parent = a.x >> 16;
                        uint32_t r = 1u;
                        if (parent != TREE_NO_PARENT) {
                                const uint32_t ord = b.y & 0xffffu, pop = (b.z >> 16) & 0xffu;
                                const uint32_t pword = (parent >> 5) == (n >> 5) ? cur : sh.bits[(parent >> 5) & (TREE_WIDE_MAX_NODES / 32 - 1u)][tid];
                                const bool mine = (cur >> (n & 31u)) & 1u;
                                const bool via = pop == TRI_OP_AND ? true : (pop == TRI_OP_OR || pop == TRI_OP_SOME) ? mine : pop == TRI_OP_NOT ? ord == 0 : (ord == 0 || mine);
                                r = ((pword >> (parent & 31u)) & 1u) && via;
                        }
                        cur = (cur & ~(1u << (n & 31u))) | (r << (n & 31u));
                        if ((n & 31u) == 0u)
                                sh.bits[n >> 5][tid] = cur;
                }
                double s = 0.0;
                uint32_t rep = 0, rep_hi = 0;
                for (uint32_t n = 0; n < nn; ++n) {
                        if ((n & 31u) == 0u)
                                cur = sh.bits[n >> 5][tid];
                        const uint4 a = sh.t.node4[2 * n];
                        const uint32_t op = a.x & 0xffu;
                        if (!((cur >> (n & 31u)) & 1u) || (op != TRI_OP_TERM && op != TRI_OP_PHRASE))
                                continue;
                        rep |= sh.t.node4[2 * n + 1].x;    // rmask
                        rep_hi |= sh.t.node4[2 * n + 1].w; // ... and its bits 32 .. 63 (DevTreeNodeW::pad)
                        if (!all_scores || a.w == 0xffffffffu)
                                continue;
                        if (op == TRI_OP_TERM) {
                                const uint32_t *pa = tree_wide_row(a.z, trows, prows, plw);
                                // (the row's interleaved level words: the frequency itself up to PL_NESTED - 1; the top level: read it from the postings)
                                const uint32_t *lv = pa + (size_t)PL_STORED * plw + 3u * wi;
                                uint32_t f = ((lv[0] >> bit) & 1u) | (((lv[1] >> bit) & 1u) << 1) | (((lv[2] >> bit) & 1u) << 2);
                                if (f == PL_NESTED || !f)
                                        f = fused_lookup_freq<CODEC>(index, blk_last, blk_off, terms[a.y], doc);
                                s += (double)sim_score(sim, sweights[q.score_base + a.w], f);
                        } else { // the phrase's score for this document: its hidden query's list holds it (k_phrase: scorer->score(id, matchCnt, weight))
                                const DevQuery hq = plan[a.y];
                                s += pscore[hq.out_off + first_ge(out + hq.out_off, 0u, counts[hq.first_task], doc)];
                        }
                }
                if (all_scores)
                        all_scores[o] = s;
                if (allow)
                        allow[o] = rep;
                if (hi)
                        hi[base + j] = rep_hi; // (base + j < q.out_cap: the query's share of the array)
        }
}

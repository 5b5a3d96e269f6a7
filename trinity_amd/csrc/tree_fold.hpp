// tree_fold.hpp — the fold over a WIDE tree record (dev_structs.hpp: DevTreeNodeW), one bitmap word per thread: what k_tree_eval_wide (k_tree_wide.hpp, a
// query over an index's rows) and k_perc_eval (k_perc.hpp, a stored query over a batch's rows) both run.  The record, the stack and where a leaf's word comes
// from are the caller's: three callables.  Part of libtrinity_hip.so (MI355X / gfx950).  New code, no reference source.
//
// A tree is a FOLD over its postfix node list, and what a thread keeps grows with the tree's DEPTH: a node that completes is handed to its parent at once —
//   * the first child (ord == 0) BECOMES the parent's accumulator, pushed on the thread's stack: a word for AND / OR / NOT / OPT, the parent's
//     counter planes (a bit-sliced count of the children that hold, seeded with the child's word) for a matchsome;
//   * a later child is folded into the accumulator on top: &=, |=, &= ~v (NOT's excluded side), nothing (OPT's optional side), a ripple add;
//   * when the list reaches the parent itself its accumulator is on top: popped, a matchsome's planes compared with its threshold.
// The node list is the same for every thread that folds it together, so the stack pointer is uniform.
#pragma once

// a stack slot (uniform).  The lowering bounds a record's stack: the mask only keeps a damaged record's stores inside the array
__device__ __forceinline__ uint32_t tree_wide_slot(const uint32_t sp) { return sp & (TREE_WIDE_STACK - 1u); }
static_assert((TREE_WIDE_STACK & (TREE_WIDE_STACK - 1u)) == 0, "tree_wide_slot masks");

// node_at(n, a, b): node n's two 16-byte halves — a { op | cbits << 8 | parent << 16, arg, row, score }, b { rmask, ord | nkids << 16, thr | pop << 16 | pcbits << 24, pad };
// leaf(a): the thread's word of a TERM / PHRASE leaf; stk(slot): the thread's stack word `slot` (already masked), an lvalue.  Returns the root's word.
// UNARY_NOT: a NOT node with ONE child is its complement (the percolator's unarynot; no batch record holds one).
template <bool UNARY_NOT, class NodeAt, class Leaf, class Stk>
__device__ __forceinline__ uint32_t tree_wide_fold(const uint32_t nn, NodeAt &&node_at, Leaf &&leaf, Stk &&stk) {
        uint32_t sp = 0, m = 0;
        for (uint32_t n = 0; n < nn; ++n) { // (uniform: the record, and with it sp, is the same for every thread)
                uint4 a, b;
                node_at(n, a, b);
                const uint32_t op = uni(a.x & 0xffu);
                uint32_t v;
                if (op == TRI_OP_TERM || op == TRI_OP_PHRASE)
                        v = leaf(a);
                else if (op == TRI_OP_SOME) { // DisjunctionSome: count >= thr, from the top plane down — greater so far, or equal so far and this bit decides
                        const uint32_t cb = uni((a.x >> 8) & 0xffu), thr = uni(b.z & 0xffffu);
                        uint32_t gt = 0, eq = 0xffffffffu;
                        for (uint32_t p = cb; p-- > 0;) {
                                const uint32_t c = stk(tree_wide_slot(sp - cb + p));
                                const uint32_t tb = ((thr >> p) & 1u) ? 0xffffffffu : 0u;
                                gt |= eq & c & ~tb;
                                eq &= ~(c ^ tb);
                        }
                        v = (thr >> cb) ? 0u : (gt | eq); // (a threshold the planes cannot reach: never — the parser drops such a matchsome)
                        sp -= cb;
                } else { // AND / OR / NOT / OPT: the accumulator is the node's word
                        v = stk(tree_wide_slot(--sp));
                        if (UNARY_NOT && op == TRI_OP_NOT && uni(b.y >> 16) == 1u)
                                v = ~v;
                }
                if ((a.x >> 16) == TREE_NO_PARENT) { // (uniform) the root: the last node
                        m = v;
                        continue;
                }
                const uint32_t ord = uni(b.y & 0xffffu), pop = uni((b.z >> 16) & 0xffu), pcb = uni(b.z >> 24);
                if (ord == 0) { // the parent's accumulator begins as this word
                        stk(tree_wide_slot(sp)) = v;
                        if (pop == TRI_OP_SOME) {
                                for (uint32_t p = 1; p < pcb; ++p)
                                        stk(tree_wide_slot(sp + p)) = 0u;
                                sp += pcb;
                        } else
                                ++sp;
                } else if (pop == TRI_OP_AND)
                        stk(tree_wide_slot(sp - 1)) &= v;
                else if (pop == TRI_OP_OR)
                        stk(tree_wide_slot(sp - 1)) |= v;
                else if (pop == TRI_OP_NOT) // Filter (docset_iterators.cpp:652-677): required AND NOT excluded
                        stk(tree_wide_slot(sp - 1)) &= ~v;
                else if (pop == TRI_OP_SOME) { // one more child into the bit-sliced count
                        uint32_t carry = v;
                        for (uint32_t p = 0; p < pcb; ++p) {
                                uint32_t &c = stk(tree_wide_slot(sp - pcb + p));
                                const uint32_t t = c & carry;
                                c ^= carry;
                                carry = t;
                        }
                } // (TRI_OP_OPT, its optional side: Optional's documents are its main side's, docset_iterators.h:174-206)
        }
        return m;
}

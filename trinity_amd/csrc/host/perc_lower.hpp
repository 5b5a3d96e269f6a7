// perc_lower.hpp — the host half of the percolator (perc_side.hpp, tri_perc_*): a set of stored postfix programs lowered to wide tree records
// (dev_structs.hpp: DevTreeNodeW, the records k_tree_wide.hpp folds) whose leaves index ONE leaf table of the set — the distinct terms the queries
// name, then the distinct multi-word phrases —, and the validation of a batch of documents.  percolator.cpp:9-137 is one exec_node tree walked per
// (query, document); here the tree is data and the documents are the bits of a word.  Host-only C++17, no HIP: libtrinity_hip.so and
// libtrinity_host.so (the CPU tests) include the same file.  New code, no reference source.
#pragma once
#include "../../../include/trinity_hip.h"
#include "../dev_structs.hpp"

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

namespace perc {
        constexpr uint32_t NONE = 0xffffffffu;
        constexpr uint32_t Q_RUNS = 1u;    // qflags: the query has a record (supported, not the empty program)
        constexpr uint32_t Q_ABSENT = 2u;  // ... it holds on a document that has none of its leaves (a pure negation, NOT(1)): the prune may not skip it
        constexpr uint32_t Q_ENABLED = 4u; // ... tri_perc_set_enabled

        struct Lowered {
                std::vector<int32_t> status;        // per query: TRI_OK / TRI_ERR_UNSUPPORTED
                std::vector<uint32_t> qflags;       // per query: Q_*
                std::vector<uint32_t> rec_off;      // per query: its record's first word in recs (NONE: no record)
                std::vector<uint32_t> recs;         // TREE_HDR_WORDS + 8 words a node, record after record
                std::vector<uint32_t> qleaf_first;  // [nq + 1] into qleaves
                std::vector<uint32_t> qleaves;      // per query: its distinct leaves
                std::vector<uint32_t> leaf_term;    // term leaf l: its term (leaves 0 .. nT-1; phrase p is leaf nT + p)
                std::vector<uint32_t> term_leaf;    // [nterms]: the term's leaf or NONE
                std::vector<uint32_t> phrase_first; // [nP + 1] into phrase_leaves
                std::vector<uint32_t> phrase_leaves; // per phrase: the TERM LEAVES of its words, in order
                uint32_t unsupported = 0;
                uint32_t stack_max = 1;             // the deepest evaluation stack a record needs, in words (k_perc_eval's LDS)
        };

        inline int lerr(std::string &err, const int code, const char *fmt, ...) {
                char buf[384];
                va_list ap;
                va_start(ap, fmt);
                vsnprintf(buf, sizeof buf, fmt, ap);
                va_end(ap);
                err = buf;
                return code;
        }

        // Every program of the set.  A malformed program fails the call (TRI_ERR_INVALID, what tri_batch_create refuses, except that NOT may have ONE
        // operand: unarynot, percolator.cpp:45-46); a tree of more than TREE_WIDE_MAX_NODES nodes, or one whose fold needs more than TREE_WIDE_STACK words
        // (planner_lower.hpp, lower_tree: the accumulators of a leaf's ancestors), is left out alone.  A node per token, less a phrase's words.
        inline int lower(const uint32_t *prog, const size_t prog_len, const tri_query *queries, const size_t nq, const uint32_t nterms, Lowered &L, std::string &err) {
                struct HNode {
                        uint32_t op, thr, leaf, parent, ord, nkids;
                };
                L = Lowered{};
                L.status.assign(nq, TRI_OK);
                L.qflags.assign(nq, Q_ENABLED);
                L.rec_off.assign(nq, NONE);
                L.qleaf_first.assign(nq + 1, 0);
                L.term_leaf.assign(nterms, NONE);
                L.phrase_first.assign(1, 0);
                std::map<std::vector<uint32_t>, uint32_t> phrase_of;
                std::vector<std::vector<uint32_t>> phrases;
                std::vector<HNode> tn;
                std::vector<uint32_t> st, words, seen_at;
                std::vector<uint8_t> val;
                auto term_leaf = [&](const uint32_t t) {
                        if (L.term_leaf[t] == NONE) {
                                L.term_leaf[t] = (uint32_t)L.leaf_term.size();
                                L.leaf_term.push_back(t);
                        }
                        return L.term_leaf[t];
                };
                // pass 1: the nodes of every query, phrase leaves numbered from 0 (the term leaves are not all known yet)
                struct QNodes {
                        size_t first, n;
                };
                std::vector<QNodes> qn(nq);
                std::vector<HNode> all;
                constexpr uint32_t PHRASE_BIT = 0x80000000u;
                for (size_t q = 0; q < nq; ++q) {
                        const tri_query &tq = queries[q];
                        qn[q] = {all.size(), 0};
                        if ((uint64_t)tq.prog_off + tq.prog_len > prog_len)
                                return lerr(err, TRI_ERR_INVALID, "tri_perc_create: query %zu: its program reaches past prog_len", q);
                        const uint32_t *p = prog + tq.prog_off;
                        tn.clear();
                        st.clear();
                        bool oversize = false;
                        for (uint32_t i = 0; i < tq.prog_len; ++i) {
                                const uint32_t op = p[i] >> 28, arg = p[i] & 0x0fffffffu;
                                HNode d{op, 0, NONE, NONE, 0, 0};
                                if (op == TRI_OP_TERM) {
                                        if (arg >= nterms)
                                                return lerr(err, TRI_ERR_INVALID, "tri_perc_create: query %zu, token %u: term %u of a dictionary of %u", q, i, arg, nterms);
                                        d.leaf = term_leaf(arg);
                                } else {
                                        const uint32_t nk = op == TRI_OP_SOME ? (arg & 0xffffu) : arg;
                                        if (nk < 1 || nk > st.size())
                                                return lerr(err, TRI_ERR_INVALID, "tri_perc_create: query %zu, token %u: %u operands, %zu on the stack", q, i, nk, st.size());
                                        const uint32_t *kids = st.data() + st.size() - nk;
                                        if (op == TRI_OP_PHRASE) {
                                                if (nk > MAX_PHRASE_TERMS)
                                                        return lerr(err, TRI_ERR_INVALID, "tri_perc_create: query %zu, token %u: a phrase of %u words (at most %u)", q, i, nk, MAX_PHRASE_TERMS);
                                                std::vector<uint32_t> w;
                                                for (uint32_t k = 0; k < nk; ++k) {
                                                        // (a phrase's words are the nk TERM tokens right before it)
                                                        if (kids[k] != tn.size() - nk + k || tn[kids[k]].op != TRI_OP_TERM)
                                                                return lerr(err, TRI_ERR_INVALID, "tri_perc_create: query %zu, token %u: a phrase's operands are TERM tokens", q, i);
                                                        w.push_back(tn[kids[k]].leaf);
                                                }
                                                st.resize(st.size() - nk);
                                                if (nk == 1) { // a one-word phrase is its word
                                                        st.push_back((uint32_t)tn.size() - 1);
                                                        continue;
                                                }
                                                tn.resize(tn.size() - nk);
                                                auto it = phrase_of.find(w);
                                                if (it == phrase_of.end()) {
                                                        it = phrase_of.emplace(w, (uint32_t)phrases.size()).first;
                                                        phrases.push_back(w);
                                                }
                                                d.leaf = PHRASE_BIT | it->second;
                                        } else {
                                                if (op == TRI_OP_SOME) {
                                                        d.thr = arg >> 16;
                                                        if (!d.thr || d.thr > nk)
                                                                return lerr(err, TRI_ERR_INVALID, "tri_perc_create: query %zu, token %u: at least %u of %u", q, i, d.thr, nk);
                                                } else if (op == TRI_OP_OPT ? nk != 2 : op == TRI_OP_NOT ? nk > 2 : (op != TRI_OP_AND && op != TRI_OP_OR))
                                                        return lerr(err, TRI_ERR_INVALID, "tri_perc_create: query %zu, token %u: operator %u with %u operands", q, i, op, nk);
                                                for (uint32_t k = 0; k < nk; ++k) {
                                                        tn[kids[k]].parent = (uint32_t)tn.size();
                                                        tn[kids[k]].ord = k;
                                                }
                                                d.nkids = nk;
                                                st.resize(st.size() - nk);
                                        }
                                }
                                st.push_back((uint32_t)tn.size());
                                tn.push_back(d);
                        }
                        if (tq.prog_len && st.size() != 1)
                                return lerr(err, TRI_ERR_INVALID, "tri_perc_create: query %zu: the program leaves %zu values", q, st.size());
                        const uint32_t nn = (uint32_t)tn.size();
                        oversize = nn > TREE_WIDE_MAX_NODES;
                        if (!oversize && nn) {
                                words.assign(nn, 0);
                                for (uint32_t i = nn; i-- > 0;) {
                                        if (tn[i].parent != NONE) {
                                                const HNode &pa = tn[tn[i].parent];
                                                words[i] = words[tn[i].parent] + (pa.op == TRI_OP_SOME ? tree_counter_planes(pa.nkids) : 1u);
                                        }
                                        if (!tn[i].nkids && words[i] > TREE_WIDE_STACK)
                                                oversize = true;
                                }
                                if (!oversize)
                                        for (uint32_t i = 0; i < nn; ++i)
                                                L.stack_max = std::max(L.stack_max, words[i]);
                        }
                        if (oversize) {
                                L.status[q] = TRI_ERR_UNSUPPORTED;
                                ++L.unsupported;
                                lerr(err, TRI_ERR_UNSUPPORTED, "tri_perc_create: query %zu: a tree of more than %u nodes or %u stack words", q, TREE_WIDE_MAX_NODES, TREE_WIDE_STACK);
                                continue;
                        }
                        qn[q].n = nn;
                        all.insert(all.end(), tn.begin(), tn.end());
                }
                // pass 2: the leaf table is complete — the records
                const uint32_t nT = (uint32_t)L.leaf_term.size();
                for (const auto &w : phrases) {
                        L.phrase_leaves.insert(L.phrase_leaves.end(), w.begin(), w.end());
                        L.phrase_first.push_back((uint32_t)L.phrase_leaves.size());
                }
                seen_at.assign(nT + phrases.size(), NONE);
                for (size_t q = 0; q < nq; ++q) {
                        L.qleaf_first[q] = (uint32_t)L.qleaves.size();
                        const uint32_t nn = (uint32_t)qn[q].n;
                        if (!nn)
                                continue; // (left out, or the empty program: constfalse, percolator.cpp:76-78)
                        const HNode *t = all.data() + qn[q].first;
                        if (L.recs.size() + TREE_HDR_WORDS + 8ull * nn > 0xfffffff0ull)
                                return lerr(err, TRI_ERR_UNSUPPORTED, "tri_perc_create: the set's records exceed 2^32 words at query %zu", q);
                        L.rec_off[q] = (uint32_t)L.recs.size();
                        L.recs.resize(L.recs.size() + TREE_HDR_WORDS + 8u * nn, 0u);
                        uint32_t *rec = &L.recs[L.rec_off[q]];
                        rec[0] = nn, rec[1] = TREE_KIND_WIDE;
                        DevTreeNodeW *out = reinterpret_cast<DevTreeNodeW *>(rec + TREE_HDR_WORDS);
                        val.assign(nn, 0);
                        std::vector<uint32_t> &ntrue = words;
                        ntrue.assign(nn, 0);
                        for (uint32_t i = 0; i < nn; ++i) {
                                const HNode &h = t[i];
                                DevTreeNodeW d{};
                                d.op = (uint8_t)h.op;
                                d.cbits = h.op == TRI_OP_SOME ? (uint8_t)tree_counter_planes(h.nkids) : 0;
                                d.parent = h.parent == NONE ? (uint16_t)TREE_NO_PARENT : (uint16_t)h.parent;
                                d.score = NONE;
                                d.ord = (uint16_t)h.ord, d.nkids = (uint16_t)h.nkids, d.thr = (uint16_t)h.thr;
                                if (h.parent != NONE) {
                                        d.pop = (uint8_t)t[h.parent].op;
                                        d.pcbits = t[h.parent].op == TRI_OP_SOME ? (uint8_t)tree_counter_planes(t[h.parent].nkids) : 0;
                                }
                                bool v = false; // the node on a document that holds none of the leaves
                                if (!h.nkids) {
                                        const uint32_t leaf = (h.leaf & PHRASE_BIT) ? nT + (h.leaf & ~PHRASE_BIT) : h.leaf;
                                        d.arg = (h.leaf & PHRASE_BIT) ? 0u : L.leaf_term[leaf];
                                        d.row = leaf;
                                        if (seen_at[leaf] != (uint32_t)q) {
                                                seen_at[leaf] = (uint32_t)q;
                                                L.qleaves.push_back(leaf);
                                        }
                                } else if (h.op == TRI_OP_AND)
                                        v = ntrue[i] == h.nkids;
                                else if (h.op == TRI_OP_SOME)
                                        v = ntrue[i] >= h.thr;
                                else if (h.op == TRI_OP_NOT && h.nkids == 1)
                                        v = !ntrue[i];
                                else // OR: any; NOT(2) / OPT: what the sides left (below)
                                        v = ntrue[i] != 0;
                                val[i] = v;
                                if (h.parent != NONE) {
                                        const HNode &pa = t[h.parent];
                                        if (pa.op == TRI_OP_NOT && pa.nkids == 2)
                                                ntrue[h.parent] = h.ord == 0 ? v : (ntrue[h.parent] && !v);
                                        else if (pa.op == TRI_OP_OPT)
                                                ntrue[h.parent] = h.ord == 0 ? v : ntrue[h.parent];
                                        else
                                                ntrue[h.parent] += v;
                                }
                                out[i] = d;
                        }
                        L.qflags[q] |= Q_RUNS | (val[nn - 1] ? Q_ABSENT : 0u);
                }
                L.qleaf_first[nq] = (uint32_t)L.qleaves.size();
                return TRI_OK;
        }

        // A batch of documents as tri_perc_match takes it: every refusal of the header, naming the document and the term.
        inline int check_docs(const tri_perc_docs *D, const uint32_t nterms, std::string &err) {
                if (!D->doc_first)
                        return lerr(err, TRI_ERR_INVALID, "tri_perc_match: null argument");
                if (D->reserved)
                        return lerr(err, TRI_ERR_INVALID, "tri_perc_match: reserved is not 0");
                if (D->ndocs == 0 || D->ndocs > 65536)
                        return lerr(err, TRI_ERR_INVALID, "tri_perc_match: %u documents (1 .. 65536 a call)", D->ndocs);
                for (uint32_t d = 0; d < D->ndocs; ++d)
                        if (D->doc_first[d + 1] < D->doc_first[d])
                                return lerr(err, TRI_ERR_INVALID, "tri_perc_match: doc_first does not ascend at document %u", d);
                if (D->doc_first[D->ndocs] != D->doc_first[0] && (!D->terms || !D->freqs))
                        return lerr(err, TRI_ERR_INVALID, "tri_perc_match: null argument");
                uint64_t at = 0; // (positions[] runs beside freqs[] from its first entry: the postings before doc_first[0] have theirs too)
                for (uint64_t i = 0; i < D->doc_first[0]; ++i)
                        at += D->freqs[i];
                for (uint32_t d = 0; d < D->ndocs; ++d)
                        for (uint64_t i = D->doc_first[d]; i < D->doc_first[d + 1]; ++i) {
                                const uint32_t t = D->terms[i];
                                if (t != NONE && t >= nterms)
                                        return lerr(err, TRI_ERR_INVALID, "tri_perc_match: document %u: term %u of a dictionary of %u", d, t, nterms);
                                // (strictly ascending; the unknown terms, 0xffffffff, stand at the end and may repeat)
                                if (i > D->doc_first[d] && (t == NONE ? D->terms[i - 1] > t : D->terms[i - 1] >= t))
                                        return lerr(err, TRI_ERR_INVALID, "tri_perc_match: document %u: term %u after term %u (strictly ascending)", d, t, D->terms[i - 1]);
                                const uint64_t f = D->freqs[i];
                                if (at + f > D->npositions)
                                        return lerr(err, TRI_ERR_INVALID, "tri_perc_match: document %u, term %u: %llu positions run past npositions = %llu", d, t, (unsigned long long)f,
                                                    (unsigned long long)D->npositions);
                                if (f && !D->positions)
                                        return lerr(err, TRI_ERR_INVALID, "tri_perc_match: null argument");
                                for (uint64_t k = 1; k < f; ++k)
                                        if (D->positions[at + k] < D->positions[at + k - 1])
                                                return lerr(err, TRI_ERR_INVALID, "tri_perc_match: document %u, term %u: position %u after %u", d, t, D->positions[at + k], D->positions[at + k - 1]);
                                at += f;
                        }
                return TRI_OK;
        }
} // namespace perc

// planner_lower.hpp — the planner's first pass (planner.hpp): a postfix program parsed into a tree with the reference's flattening and cost
// model, lowered into a conjunctive normal form over terms, a truth table (general trees of few terms) or a TASK_TREE record, and classed.
// Host-only C++17, no HIP.  New code, no reference source.
#pragma once
#include "planner_types.hpp"

namespace trip {
        // Parse one postfix program into a tree with the reference's flattening (exec.cpp:339-358, 382-393), emptiness propagation and cost
        // model (exec.cpp:35-110).  Returns root index or -1.
        inline int parse_program(const HostIndex &ix, const uint32_t *prog, uint32_t len, Scratch &S) {
                auto &nodes = S.nodes;
                auto &st = S.st;
                auto &pool = S.kidpool;
                nodes.clear();
                st.clear();
                pool.clear();
                for (uint32_t i = 0; i < len; ++i) {
                        const uint32_t op = prog[i] >> 28, arg = prog[i] & 0x0fffffffu;
                        PNode n;
                        n.op = op;
                        n.tok = i;
                        if (op == TRI_OP_TERM) {
                                n.term = arg;
                                n.cost = arg < ix.terms.size() ? ix.terms[arg].documents : 0;
                                n.empty = n.cost == 0; // unknown term == no documents (index_source.h:60-72)
                        } else {
                                const uint32_t nk = op == TRI_OP_SOME ? (arg & 0xffffu) : arg; // operands taken off the stack
                                if (nk < 1 || nk > st.size())
                                        return -1;
                                S.tmpk.assign(st.end() - nk, st.end());
                                st.resize(st.size() - nk);
                                const std::vector<int> &kids = S.tmpk;
                                n.kid_off = (uint32_t)pool.size();
                                if (op == TRI_OP_SOME) {
                                        // matchsome (exec.cpp:276-283): operands that can never match are dropped; fewer live operands than
                                        // the threshold: never matches.  cost: docset_iterators.cpp:733-742, the (cnt - min + 1) cheapest
                                        const uint32_t mn = arg >> 16;
                                        if (!mn || mn > nk)
                                                return -1;
                                        for (int k : kids)
                                                if (!nodes[k].empty)
                                                        pool.push_back(k);
                                        n.kid_n = (uint32_t)pool.size() - n.kid_off;
                                        n.term = mn; // (the threshold rides in the otherwise unused field)
                                        n.empty = n.kid_n < mn;
                                        S.cs.clear();
                                        for (uint32_t k = 0; k < n.kid_n; ++k)
                                                S.cs.push_back(nodes[pool[n.kid_off + k]].cost);
                                        std::sort(S.cs.begin(), S.cs.end());
                                        for (size_t k = 0; k + mn <= S.cs.size(); ++k)
                                                n.cost += S.cs[k];
                                } else if (op == TRI_OP_PHRASE) {
                                        if (arg > MAX_PHRASE_TERMS) // trinity_limits.h:12 MaxPhraseSize
                                                return -1;
                                        for (int k : kids) {
                                                if (nodes[k].op != TRI_OP_TERM)
                                                        return -1;
                                                n.empty |= nodes[k].empty;
                                                pool.push_back(k);
                                        }
                                        n.kid_n = nk;
                                        n.cost = nodes[kids[0]].cost + UINT32_MAX + (uint64_t)UINT16_MAX * arg;
                                } else if (op == TRI_OP_AND) {
                                        for (int k : kids) {
                                                n.empty |= nodes[k].empty;
                                                if (nodes[k].op == TRI_OP_AND)
                                                        for (uint32_t j = 0; j < nodes[k].kid_n; ++j)
                                                                pool.push_back(pool[nodes[k].kid_off + j]);
                                                else
                                                        pool.push_back(k);
                                        }
                                        n.kid_n = (uint32_t)pool.size() - n.kid_off;
                                        if (n.kid_n <= 16) { // stable insertion sort (std::stable_sort takes a heap buffer per call: a malloc per AND of two terms)
                                                int *kb = pool.data() + n.kid_off;
                                                for (uint32_t a = 1; a < n.kid_n; ++a) {
                                                        const int v = kb[a];
                                                        uint32_t b = a;
                                                        for (; b && nodes[kb[b - 1]].cost > nodes[v].cost; --b)
                                                                kb[b] = kb[b - 1];
                                                        kb[b] = v;
                                                }
                                        } else
                                                std::stable_sort(pool.begin() + n.kid_off, pool.end(), [&](int a, int b) { return nodes[a].cost < nodes[b].cost; });
                                        n.cost = nodes[pool[n.kid_off]].cost;
                                } else if (op == TRI_OP_OR) {
                                        for (int k : kids) {
                                                if (nodes[k].empty)
                                                        continue;
                                                if (nodes[k].op == TRI_OP_OR)
                                                        for (uint32_t j = 0; j < nodes[k].kid_n; ++j)
                                                                pool.push_back(pool[nodes[k].kid_off + j]);
                                                else
                                                        pool.push_back(k);
                                        }
                                        n.kid_n = (uint32_t)pool.size() - n.kid_off;
                                        n.empty = n.kid_n == 0;
                                        for (uint32_t k = 0; k < n.kid_n; ++k)
                                                n.cost += nodes[pool[n.kid_off + k]].cost;
                                } else if (op == TRI_OP_OPT) {
                                        if (arg != 2)
                                                return -1;
                                        if (nodes[kids[1]].empty) { // an optional side that can never match adds nothing
                                                st.push_back(kids[0]);
                                                continue;
                                        }
                                        pool.push_back(kids[0]); // {main, optional}
                                        pool.push_back(kids[1]);
                                        n.kid_n = 2;
                                        n.empty = nodes[kids[0]].empty;
                                        n.cost = nodes[kids[0]].cost;
                                } else if (op == TRI_OP_NOT) {
                                        if (arg != 2)
                                                return -1;
                                        if (nodes[kids[1]].empty) { // [a NOT <never matches>] => a
                                                st.push_back(kids[0]);
                                                continue;
                                        }
                                        pool.push_back(kids[0]); // {required, excluded}
                                        pool.push_back(kids[1]);
                                        n.kid_n = 2;
                                        n.empty = nodes[kids[0]].empty;
                                        n.cost = nodes[kids[0]].cost; // exec.cpp:55-60
                                } else
                                        return -1;
                        }
                        nodes.push_back(n);
                        st.push_back((int)nodes.size() - 1);
                }
                return st.size() == 1 ? st[0] : -1;
        }

        // ---- general trees: what the CNF lowering does not take (matchsome, NOT / Optional of any subtree, AND under OR ...) runs as
        // TASK_FUSED with a truth table over the presence of the query's distinct terms (<= FUS_MAX_SLOTS, no multi-word phrase).
        struct TruthPlan {
                std::vector<uint32_t> slots;            // distinct terms, order of first appearance
                std::vector<uint32_t> leaves, leaf_tok; // scorer leaves (positive TERM nodes) in tree order, and their program tokens
                std::vector<uint32_t> leaf_slot;
                uint32_t tt[8] = {};
                std::vector<std::array<uint32_t, 8>> ctt;
        };
        struct TruthBuilder {
                const Scratch &S;
                TruthPlan &tp;
                std::vector<int> leaf_of_node; // node -> scorer leaf index (-1: none)
                bool ok = true;
                uint32_t slot_of(uint32_t term) {
                        for (size_t i = 0; i < tp.slots.size(); ++i)
                                if (tp.slots[i] == term)
                                        return (uint32_t)i;
                        tp.slots.push_back(term);
                        return (uint32_t)tp.slots.size() - 1;
                }
                // first walk: slots for every term, scorer leaves for the terms an iterator of the tree can report
                void scan(int ni, bool positive) {
                        const PNode &x = S.nodes[ni];
                        if (x.op == TRI_OP_TERM || (x.op == TRI_OP_PHRASE && x.kid_n == 1)) {
                                const PNode &t = x.op == TRI_OP_TERM ? x : S.nodes[S.kids(x)[0]];
                                const uint32_t sl = slot_of(t.term);
                                if (positive) {
                                        leaf_of_node[ni] = (int)tp.leaves.size();
                                        tp.leaves.push_back(t.term);
                                        tp.leaf_tok.push_back(t.tok);
                                        tp.leaf_slot.push_back(sl);
                                }
                                return;
                        }
                        if (x.op == TRI_OP_PHRASE) {
                                ok = false; // a positional constraint is not a function of presence
                                return;
                        }
                        for (uint32_t k = 0; k < x.kid_n; ++k)
                                scan(S.kids(x)[k], positive && !(x.op == TRI_OP_NOT && k == 1));
                }
                uint32_t slot_const(uint32_t term) const {
                        for (size_t i = 0; i < tp.slots.size(); ++i)
                                if (tp.slots[i] == term)
                                        return (uint32_t)i;
                        return 0;
                }
                bool eval(int ni, uint32_t p) const {
                        const PNode &x = S.nodes[ni];
                        const int *kd = S.kids(x);
                        switch (x.op) {
                                case TRI_OP_TERM:
                                        return (p >> slot_const(x.term)) & 1u;
                                case TRI_OP_PHRASE:
                                        return (p >> slot_const(S.nodes[kd[0]].term)) & 1u;
                                case TRI_OP_AND:
                                        for (uint32_t k = 0; k < x.kid_n; ++k)
                                                if (!eval(kd[k], p))
                                                        return false;
                                        return true;
                                case TRI_OP_OR:
                                        for (uint32_t k = 0; k < x.kid_n; ++k)
                                                if (eval(kd[k], p))
                                                        return true;
                                        return false;
                                case TRI_OP_SOME: {
                                        uint32_t c = 0;
                                        for (uint32_t k = 0; k < x.kid_n; ++k)
                                                c += eval(kd[k], p) ? 1u : 0u;
                                        return c >= x.term;
                                }
                                case TRI_OP_NOT: // Filter (docset_iterators.cpp:652-677)
                                        return eval(kd[0], p) && !eval(kd[1], p);
                                case TRI_OP_OPT: // Optional (docset_iterators.h:174-206): the documents of main
                                        return eval(kd[0], p);
                        }
                        return false;
                }
                // the scorer leaves that sit on a document of pattern p, through the tree (node ni matches p): what the reference's score() /
                // collect_doc_matching_terms recursion reaches (docset_iterators_scorers.cpp:38-57, 77-104, 107-193; queryexec_ctx.cpp:382-520)
                void collect(int ni, uint32_t p, uint32_t &mask) const {
                        const PNode &x = S.nodes[ni];
                        const int *kd = S.kids(x);
                        switch (x.op) {
                                case TRI_OP_TERM:
                                case TRI_OP_PHRASE:
                                        if (leaf_of_node[ni] >= 0)
                                                mask |= 1u << leaf_of_node[ni];
                                        break;
                                case TRI_OP_AND:
                                        for (uint32_t k = 0; k < x.kid_n; ++k)
                                                collect(kd[k], p, mask);
                                        break;
                                case TRI_OP_OR:
                                case TRI_OP_SOME:
                                        for (uint32_t k = 0; k < x.kid_n; ++k)
                                                if (eval(kd[k], p))
                                                        collect(kd[k], p, mask);
                                        break;
                                case TRI_OP_NOT:
                                        collect(kd[0], p, mask);
                                        break;
                                case TRI_OP_OPT:
                                        collect(kd[0], p, mask);
                                        if (eval(kd[1], p))
                                                collect(kd[1], p, mask);
                                        break;
                        }
                }
        };
        inline bool build_truth(const Scratch &S, int root, TruthPlan &tp) {
                TruthBuilder tb{S, tp, std::vector<int>(S.nodes.size(), -1)};
                tb.scan(root, true);
                if (!tb.ok || tp.slots.size() > FUS_MAX_SLOTS || tp.leaves.size() > FUS_MAX_LEAVES || tp.leaves.empty())
                        return false;
                tp.ctt.assign(tp.leaves.size(), std::array<uint32_t, 8>{});
                for (uint32_t p = 0; p < (1u << tp.slots.size()); ++p) {
                        if (!tb.eval(root, p))
                                continue;
                        tp.tt[p >> 5] |= 1u << (p & 31u);
                        uint32_t mask = 0;
                        tb.collect(root, p, mask);
                        for (size_t j = 0; j < tp.leaves.size(); ++j)
                                if ((mask >> j) & 1u)
                                        tp.ctt[j][p >> 5] |= 1u << (p & 31u);
                }
                return !(tp.tt[0] & 1u); // (a tree that matches documents holding none of its terms cannot be enumerated from postings)
        }

        inline int lower_tree(const Ctx &C, Frag &f, size_t qi, const uint32_t *prog, uint32_t plen, const double *wq, int root);

        // ---- conjunctive normal form over terms: AND of (term | OR of terms); a root OR is one group.  Collected in the fragment's Scratch:
        //      the groups (gt / gs), every TERM leaf in evaluation order (one scorer each) with its token, the phrases, the excluded and
        //      the optional sides
        inline uint32_t cnf_ngroups(const Scratch &S) { return (uint32_t)S.gs.size() - 1; }
        inline bool cnf_single_seen(const Scratch &S, const uint32_t x) {
                for (uint32_t g = 0; g < cnf_ngroups(S); ++g)
                        if (S.gs[g + 1] - S.gs[g] == 1 && S.gt[S.gs[g]] == x)
                                return true;
                return false;
        }
        inline bool cnf_add_group(const Ctx &C, Scratch &S, const PNode &g, const double *wq) {
                const std::vector<PNode> &nodes = S.nodes;
                auto &gt = S.gt;
                auto &gs = S.gs;
                const int *kd = S.kids(g);
                if (g.op == TRI_OP_PHRASE && g.kid_n > 1) {
                        // Phrase = conjunction of its terms + a positional constraint on the matches (k_phrase);
                        // it scores as ONE iterator with the summed idf (docset_iterators_scorers.cpp:195-228)
                        Scratch::PhraseTmp ph{(uint32_t)S.phterms.size(), g.kid_n, 0.0};
                        for (uint32_t k = 0; k < g.kid_n; ++k) {
                                const uint32_t x = nodes[kd[k]].term;
                                S.phterms.push_back(x);
                                ph.weight += C.term_weight(C.ix.terms[x].documents);
                                if (!cnf_single_seen(S, x)) {
                                        gt.push_back(x);
                                        gs.push_back((uint32_t)gt.size());
                                }
                        }
                        if (wq) // the PHRASE token's own ScorerWeight, when the caller supplies weights (by token position: two phrases
                                // that start with the same term keep their own weights)
                                ph.weight = wq[g.tok];
                        S.qphrases.push_back(ph);
                        return true;
                }
                auto &ts = S.ts;
                auto &ts_tok = S.ts_tok;
                ts.clear();
                ts_tok.clear();
                if (g.op == TRI_OP_PHRASE) {
                        ts.push_back(nodes[kd[0]].term); // a one-word phrase is a term (exec.cpp: phrase of size 1)
                        ts_tok.push_back(nodes[kd[0]].tok);
                } else if (g.op == TRI_OP_TERM) {
                        ts.push_back(g.term);
                        ts_tok.push_back(g.tok);
                } else if (g.op == TRI_OP_OR) {
                        for (uint32_t k = 0; k < g.kid_n; ++k) {
                                if (nodes[kd[k]].op != TRI_OP_TERM)
                                        return false;
                                ts.push_back(nodes[kd[k]].term);
                                ts_tok.push_back(nodes[kd[k]].tok);
                        }
                } else
                        return false;
                S.leaves.insert(S.leaves.end(), ts.begin(), ts.end());
                S.leaf_tok.insert(S.leaf_tok.end(), ts_tok.begin(), ts_tok.end());
                // a term repeated inside a group, or a single-term group seen before, adds nothing to the docID set
                auto &u = S.u;
                u.clear();
                for (uint32_t x : ts)
                        if (std::find(u.begin(), u.end(), x) == u.end())
                                u.push_back(x);
                if (u.size() == 1 && cnf_single_seen(S, u[0]))
                        return true;
                gt.insert(gt.end(), u.begin(), u.end());
                gs.push_back((uint32_t)gt.size());
                return true;
        }
        // the excluded / optional side `e` of a NOT / Optional — a term or an OR of terms — into `terms` (and its tokens into `toks`); anything else: not a CNF
        inline void cnf_side(const Scratch &S, const PNode &e, std::vector<uint32_t> &terms, std::vector<uint32_t> *toks, bool &ok) {
                const std::vector<PNode> &nodes = S.nodes;
                const int *kd = S.kids(e);
                if (e.op == TRI_OP_TERM) {
                        terms.push_back(e.term);
                        if (toks)
                                toks->push_back(e.tok);
                } else if (e.op == TRI_OP_PHRASE && e.kid_n == 1) {
                        terms.push_back(nodes[kd[0]].term);
                        if (toks)
                                toks->push_back(nodes[kd[0]].tok);
                } else if (e.op == TRI_OP_OR) {
                        for (uint32_t k = 0; k < e.kid_n; ++k) {
                                if (nodes[kd[k]].op != TRI_OP_TERM)
                                        ok = false;
                                else {
                                        terms.push_back(nodes[kd[k]].term);
                                        if (toks)
                                                toks->push_back(nodes[kd[k]].tok);
                                }
                        }
                } else
                        ok = false;
        }
        // logicalnot at the root or under an AND: its required side joins the conjunction, its excluded side (a term or an
        // OR of terms) joins the query's excluded set: A B -C == A ∧ B ∧ ¬C (Filter semantics, docset_iterators.cpp:652-677)
        inline void cnf_lower(const Ctx &C, Scratch &S, const int ni, const double *wq, bool &ok) {
                const PNode &x = S.nodes[ni];
                const int *kd = S.kids(x);
                if (x.op == TRI_OP_OPT) {
                        // Optional(main, opt): the documents of main; opt's terms score (and are reported) where they match —
                        // exactly how k_score / k_rich treat a term a match does not hold
                        cnf_lower(C, S, kd[0], wq, ok);
                        cnf_side(S, S.nodes[kd[1]], S.opts, &S.opt_tok, ok);
                } else if (x.op == TRI_OP_NOT) {
                        cnf_lower(C, S, kd[0], wq, ok);
                        cnf_side(S, S.nodes[kd[1]], S.negs, nullptr, ok);
                } else if (x.op == TRI_OP_AND) {
                        for (uint32_t k = 0; k < x.kid_n; ++k)
                                cnf_lower(C, S, kd[k], wq, ok);
                } else
                        ok &= cnf_add_group(C, S, x, wq);
        }
        // the parsed tree under `root` as a CNF in f.S; false: it is none (a general tree)
        inline bool extract_cnf(const Ctx &C, Frag &f, const int root, const double *wq) {
                Scratch &S = f.S;
                S.gt.clear();
                S.gs.assign(1, 0u);
                S.leaves.clear();   // every TERM leaf in evaluation order: one scorer each
                S.leaf_tok.clear(); // ... and the program token it came from
                S.qphrases.clear();
                S.phterms.clear();
                S.negs.clear();
                S.opts.clear();
                S.opt_tok.clear();
                bool ok = true;
                cnf_lower(C, S, root, wq, ok);
                if (!ok || !cnf_ngroups(S))
                        return false;
                // (a general tree counts every term once through its slot list)
                for (size_t oi = 0; oi < S.opts.size(); ++oi)
                        if (const uint32_t x = S.opts[oi]; C.ix.terms[x].documents) {
                                S.leaves.push_back(x); // one more scorer / reportable term each; never part of the docID set
                                S.leaf_tok.push_back(S.opt_tok[oi]);
                                if (C.mode != TRI_FLAG_DOCUMENTS_ONLY)
                                        f.term_bytes += C.ix.docbytes[x]; // its postings are read by k_score / k_rich
                        }
                return true;
        }

        inline uint64_t group_docs(const HostIndex &ix, const Scratch &S, const uint32_t g) {
                uint64_t c = 0;
                for (uint32_t i = S.gs[g]; i < S.gs[g + 1]; ++i)
                        c += ix.terms[S.gt[i]].documents;
                return c;
        }
        // the groups by their documents, cheapest first (S.gorder), and the query's term list (S.uniq): group by group, QT_GROUP on the first of
        // each group; the excluded terms are one more group, the last, marked QT_NOT
        inline void order_groups(const HostIndex &ix, Scratch &S) {
                const uint32_t ng = cnf_ngroups(S);
                auto &gorder = S.gorder;
                gorder.resize(ng);
                std::iota(gorder.begin(), gorder.end(), 0u);
                if (ng == 2) { // (the common case: a stable two-element sort)
                        if (group_docs(ix, S, 1) < group_docs(ix, S, 0))
                                std::swap(gorder[0], gorder[1]);
                } else if (ng > 2)
                        std::stable_sort(gorder.begin(), gorder.end(), [&](uint32_t x, uint32_t y) { return group_docs(ix, S, x) < group_docs(ix, S, y); });
                auto &uniq = S.uniq;
                uniq.clear();
                for (uint32_t g : gorder)
                        for (uint32_t i = S.gs[g]; i < S.gs[g + 1]; ++i)
                                uniq.push_back(S.gt[i] | (i == S.gs[g] ? QT_GROUP : 0u));
                auto &u = S.u;
                u.clear();
                for (uint32_t x : S.negs)
                        if (ix.terms[x].documents && std::find(u.begin(), u.end(), x) == u.end())
                                u.push_back(x);
                for (size_t i = 0; i < u.size(); ++i)
                        uniq.push_back(u[i] | (i == 0 ? (QT_GROUP | QT_NOT) : 0u));
        }
        // (default mode) the reportable terms into S.rt — every postings iterator collect_doc_matching_terms can reach (queryexec_ctx.cpp:382-520):
        //  group members and phrase terms, not the excluded side of a NOT —, distinct, in order of first appearance in the program
        inline void reportable_terms(Scratch &S, const uint32_t *prog, const uint32_t plen) {
                auto &rt = S.rt;
                for (uint32_t pi = 0; pi < plen; ++pi) {
                        const uint32_t tok = prog[pi];
                        if ((tok >> 28) != TRI_OP_TERM)
                                continue;
                        const uint32_t x = tok & 0x0fffffffu;
                        const bool positive = std::find(S.leaves.begin(), S.leaves.end(), x) != S.leaves.end() ||
                                              std::find(S.phterms.begin(), S.phterms.end(), x) != S.phterms.end();
                        if (positive && std::find(rt.begin(), rt.end(), x) == rt.end())
                                rt.push_back(x);
                }
        }
        // the query's phrases, and its scorers (scored) or reported terms (default mode), appended to the fragment's arrays
        inline void emit_phrases_and_scorers(const Ctx &C, Frag &f, Tmp &t, const double *wq, const bool rich) {
                const HostIndex &ix = C.ix;
                const Scratch &S = f.S;
                t.q.phrase_base = (uint32_t)f.phrases.size();
                t.q.nphrases = (uint32_t)S.qphrases.size();
                f.phrase_queries += t.q.nphrases ? 1 : 0;
                for (const auto &ph : S.qphrases) {
                        f.phrases.push_back({(uint32_t)f.pterms.size(), ph.n, ph.weight});
                        for (uint32_t k = 0; k < ph.n; ++k) {
                                const uint32_t x = S.phterms[ph.t0 + k];
                                f.pterms.push_back(x);
                                f.term_bytes += ix.hitbytes[x]; // phrase queries also stream the hit bytes
                                f.term_bytes_phrase_hits += ix.hitbytes[x];
                        }
                }
                t.q.score_base = (uint32_t)f.sterms.size();
                t.q.nscore = 0;
                if (rich) {
                        for (uint32_t x : S.rt) {
                                f.sterms.push_back(x);
                                f.term_bytes += ix.hitbytes[x]; // the hits of every reported term are read
                        }
                        t.q.nscore = (uint32_t)S.rt.size();
                        f.rich_R = std::max<uint32_t>(f.rich_R, t.q.nscore);
                }
                if (C.scored) {
                        // one scorer per PostingsListIterator of the conjunction, summed in iterator order
                        // (docset_iterators_scorers.cpp:173-193); weight = BM25 idf (similarity.h:179-181, float math)
                        // unless the caller supplied ScorerWeights per TERM token — the leaf's OWN token (a term that also sits
                        // inside a phrase or on an excluded side has another token with another weight)
                        for (size_t li = 0; li < S.leaves.size(); ++li) {
                                f.sterms.push_back(S.leaves[li]);
                                f.sweights.push_back(wq ? wq[S.leaf_tok[li]] : C.term_weight(ix.terms[S.leaves[li]].documents));
                        }
                        t.q.nscore = (uint32_t)S.leaves.size();
                }
        }

        // ---- slot maps for the one-pass scored path (k_fused.hpp): the query's distinct terms, CNF terms first
        // the fields of a slot map of `nslots` slots in 16-bit (hw) or 32-bit window words: width, saturation point; returns a field's mask
        inline uint32_t slot_geometry(DevFused &z, const uint32_t nslots, const bool hw, const tri_options &opt) {
                z.nslots = nslots;
                z.hw = hw ? 1u : 0u;
                z.fbits = z.hw ? std::min(8u, 16u / z.nslots) : (z.nslots <= 4 ? 8u : 4u);
                z.cap = (1u << z.fbits) - 2u;
                if (opt.fused_freq_cap && opt.fused_freq_cap < z.cap)
                        z.cap = (uint32_t)opt.fused_freq_cap;
                return (1u << z.fbits) - 1u;
        }
        inline void slot_map_from_truth(const Ctx &C, Frag &f, Tmp &t, const TruthPlan &tp, const bool rich) {
                DevFused z{};
                const uint32_t fm = slot_geometry(z, (uint32_t)tp.slots.size(), false, C.env.opt); // (general trees run in their own instantiation, 32-bit window words)
                for (size_t i = 0; i < tp.slots.size(); ++i)
                        z.term[i] = tp.slots[i];
                // DocumentsOnly, the default mode and the full score stream (topk == 0) need the docID set; top-K batches do not
                z.mode = FUS_MODE_TT | ((C.scored && C.in.topk) ? 0u : FUS_MODE_EMIT);
                memcpy(z.tt, tp.tt, sizeof z.tt);
                if (rich) {
                        // per REPORTABLE term (distinct, f.sterms order): reported where any of its leaves sits on the document
                        z.nleaf = t.q.nscore;
                        for (uint32_t j = 0; j < t.q.nscore; ++j) {
                                const uint32_t term = f.sterms[t.q.score_base + j];
                                for (size_t l = 0; l < tp.leaves.size(); ++l)
                                        if (tp.leaves[l] == term) {
                                                z.leaf_slot[j] = (uint8_t)tp.leaf_slot[l];
                                                for (int wd = 0; wd < 8; ++wd)
                                                        z.ctt[j][wd] |= tp.ctt[l][wd];
                                        }
                        }
                        f.rich_allow = true;
                } else {
                        z.nleaf = (uint32_t)tp.leaves.size();
                        for (size_t j = 0; j < tp.leaves.size(); ++j) {
                                z.leaf_slot[j] = (uint8_t)tp.leaf_slot[j];
                                memcpy(z.ctt[j], tp.ctt[j].data(), sizeof z.ctt[j]);
                        }
                }
                // window skipping needs groups of slots one of which every match holds: the slots of the scorer leaves if no
                // matching pattern lacks them all (else every slot: pattern 0 never matches), then every slot all matches hold
                const uint32_t npat = 1u << z.nslots;
                auto matches = [&](uint32_t p) { return (tp.tt[p >> 5] >> (p & 31u)) & 1u; };
                uint32_t gl = 0;
                for (uint32_t sl : tp.leaf_slot)
                        gl |= 1u << sl;
                for (uint32_t p = 0; p < npat; ++p)
                        if (matches(p) && !(p & gl))
                                gl = npat - 1;
                auto add_req = [&](uint32_t gsl) {
                        z.gslots[z.nreq] = gsl;
                        for (uint32_t sl = 0; sl < z.nslots; ++sl)
                                if ((gsl >> sl) & 1u)
                                        z.gmask[z.nreq] |= fm << (sl * z.fbits);
                        ++z.nreq;
                };
                add_req(gl);
                for (uint32_t sl = 0; sl < z.nslots && z.nreq < FUS_MAX_SLOTS; ++sl) {
                        bool all = gl != (1u << sl);
                        for (uint32_t p = 0; p < npat && all; ++p)
                                all = !matches(p) || ((p >> sl) & 1u);
                        if (all)
                                add_req(1u << sl);
                }
                t.fz = (int32_t)f.fz.size();
                f.fz.push_back(z);
        }
        // (a CNF of more distinct terms, or of more required groups, than a slot map holds gets none: t.fz stays -1)
        inline void slot_map_from_cnf(const Ctx &C, Frag &f, Tmp &t) {
                Scratch &S = f.S;
                auto &slots = S.slots;
                slots.clear();
                auto slot_of = [&](uint32_t term) {
                        for (size_t i = 0; i < slots.size(); ++i)
                                if (slots[i] == term)
                                        return (uint32_t)i;
                        slots.push_back(term);
                        return (uint32_t)slots.size() - 1;
                };
                for (uint32_t tt : S.uniq)
                        slot_of(tt & QT_TERM);
                for (uint32_t x : S.leaves)
                        slot_of(x);
                if (slots.size() > FUS_MAX_SLOTS)
                        return;
                DevFused z{};
                const uint32_t fm = slot_geometry(z, (uint32_t)slots.size(), C.env.opt.fused_halfwords && slots.size() <= 5, C.env.opt);
                for (size_t i = 0; i < slots.size(); ++i)
                        z.term[i] = slots[i];
                int g = -1;
                bool in_not = false;
                uint32_t nreq_groups = 0;
                for (uint32_t tt : S.uniq)
                        nreq_groups += (tt & QT_GROUP) && !(tt & QT_NOT);
                for (uint32_t tt : S.uniq) {
                        if (nreq_groups > FUS_MAX_SLOTS)
                                break; // (a CNF that repeats its terms over more groups than the slot map holds)
                        if (tt & QT_GROUP) {
                                in_not = tt & QT_NOT;
                                if (!in_not)
                                        ++g;
                        }
                        const uint32_t sidx = slot_of(tt & QT_TERM);
                        if (in_not)
                                z.nmask |= fm << (sidx * z.fbits);
                        else {
                                z.gmask[g] |= fm << (sidx * z.fbits);
                                z.gslots[g] |= 1u << sidx;
                        }
                }
                z.nreq = (uint32_t)(g + 1);
                if (z.nreq >= 1 && nreq_groups <= FUS_MAX_SLOTS) {
                        t.fz = (int32_t)f.fz.size();
                        f.fz.push_back(z);
                }
        }

        // ---- execution class.  TASK_DENSE (bitmap windows) when the lead group is an OR (it has to be materialised as a set
        //      anyway), or when every other list is within a factor 32 of the lead (no block could be skipped) and there is
        //      enough work per docID window to keep 256 lanes busy; one pass (TASK_FUSED / TASK_PLANES) when such a query
        //      asks for a top-K, or is a general tree
        // k_fused forms a window's end — w0 + W, wlast, a row's hint — in 32 bits (k_fused.hpp find_window), and W (14 or 28 cells) does not divide 2^32: on a segment
        // whose last window of either width would end past 2^32 — a largest docID of FUSED_MAX_DOC or more — no query is given to it.  A scored CNF query then runs
        // match-then-score; a truth-table query, which no other kernel takes, is left out by name (lower_query)
        constexpr uint32_t FUSED_MAX_DOC = (uint32_t)((1ull << 32) / (2ull * FUS_W) * (2ull * FUS_W)); // (0xffffc000 at the default FUS_CELLS = 14)
        static_assert(FUSED_MAX_DOC <= (1ull << 32) / FUS_W * FUS_W, "the wider window's bound is the lower one");
        inline bool fused_windows_fit(const HostIndex &ix) { return ix.max_doc < FUSED_MAX_DOC; }

        inline void classify(const Ctx &C, Frag &f, Tmp &t, const uint64_t lead_docs) {
                const HostIndex &ix = C.ix;
                const tri_options &opt = C.env.opt;
                const auto &uniq = f.S.uniq;
                t.sumdf = 0;
                t.lead_docs = lead_docs;
                t.last_doc = 0xffffffffu;
                t.dense = uniq.size() >= 2;
                uint32_t glast = 0;
                bool in_neg = false;
                for (size_t k = 0; k < uniq.size(); ++k) {
                        const DevTerm &tk = ix.terms[uniq[k] & QT_TERM];
                        t.sumdf += tk.documents;
                        t.dense &= tk.nblocks <= lead_docs;
                        if (k && (uniq[k] & QT_GROUP)) {
                                t.last_doc = std::min(t.last_doc, glast);
                                glast = 0;
                                in_neg = uniq[k] & QT_NOT;
                        }
                        if (!in_neg)
                                glast = std::max(glast, ix.blk_last[tk.first_block + tk.nblocks - 1]);
                }
                if (!in_neg)
                        t.last_doc = std::min(t.last_doc, glast);
                t.dense &= t.sumdf >= opt.dense_min_postings;
                t.dense |= t.nlead > 1;
                const bool fusable = t.fz >= 0;
                t.fuse = t.truth || (t.dense && fusable && (opt.fused != 2 || f.fz[t.fz].nreq == 1)); // (fused == 2: only pure unions)
                if (t.fuse) {
                        ++f.onepass_queries;
                        const DevFused &z = f.fz[t.fz];
                        for (uint32_t sidx = 0; sidx < z.nslots; ++sidx)
                                f.fused_postings += ix.terms[z.term[sidx]].documents;
                }
        }

        // ---- first pass, one query: the program prog[0, plen) of caller query qi lowered into `f` and classed.  wq: the ScorerWeights of the
        //      program's tokens (or null); hidden: a phrase that a TASK_TREE query of the batch reads as a leaf (lower_tree) — it has a plan
        //      slot and tasks like any phrase query, and no caller query of its own
        inline int lower_query(const Ctx &C, Frag &f, const size_t qi, const uint32_t *prog, const uint32_t plen, const double *wq, const bool hidden) {
                const HostIndex &ix = C.ix;
                const bool rich = C.rich && !hidden;
                Scratch &S = f.S;
                const int root = parse_program(ix, prog, plen, S);
                if (root < 0)
                        return herr(f.err, TRI_ERR_INVALID, "query %zu: malformed postfix program", qi);
                if (S.nodes[root].empty)
                        return TRI_OK; // matches nothing (compiles to constfalse in the reference)
                TruthPlan tp;
                bool truth = false;
                if (!extract_cnf(C, f, root, wq)) {
                        // not a CNF of terms: a general tree over <= FUS_MAX_SLOTS distinct terms runs off a truth table (k_fused.hpp);
                        // anything else — a multi-word phrase below the root conjunction, more terms or leaves — over leaf bitmaps (k_tree.hpp)
                        if (!build_truth(S, root, tp))
                                return hidden ? herr(f.err, TRI_ERR_INVALID, "query %zu: a phrase leaf that is not a phrase", qi) : lower_tree(C, f, qi, prog, plen, wq, root);
                        if (!fused_windows_fit(ix)) { // (nothing of the query is recorded yet: left out cleanly)
                                f.left_out.push_back(qi);
                                herr(f.err, TRI_ERR_UNSUPPORTED, "query %zu: a truth-table query on a segment whose docIDs reach 0x%x (the window-word kernel's last window would end past 2^32)", qi, FUSED_MAX_DOC);
                                return TRI_OK;
                        }
                        truth = true;
                        S.gt = tp.slots; // (one group of every slot: the bookkeeping below — term list, cost, output bound — sees a union)
                        S.gs.assign({0u, (uint32_t)S.gt.size()});
                        S.negs.clear();
                        S.leaves = tp.leaves;
                        S.leaf_tok = tp.leaf_tok;
                        S.qphrases.clear();
                        S.phterms.clear();
                }
                order_groups(ix, S);
                const auto &uniq = S.uniq;
                if (uniq.size() > MAX_QTERMS) // a conjunctive normal form wider than the CNF kernels' term lists: the tree path
                        return hidden ? herr(f.err, TRI_ERR_INVALID, "query %zu: a phrase of more than %u terms", qi, MAX_QTERMS) : lower_tree(C, f, qi, prog, plen, wq, root);
                // (the reportable terms are counted before anything of the query is recorded, so that a query with too many of them can still be left out cleanly)
                S.rt.clear();
                if (rich) {
                        reportable_terms(S, prog, plen);
                        if (S.rt.size() > RICH_NARROW_TERMS) {
                                // (a wide-report query — option rich_max_terms — is always a TASK_TREE query: the tree path holds its 64-bit report masks)
                                if (S.rt.size() <= C.env.opt.rich_max_terms)
                                        return lower_tree(C, f, qi, prog, plen, wq, root);
                                f.left_out.push_back(qi);
                                herr(f.err, TRI_ERR_UNSUPPORTED, "query %zu: more than %u reportable terms", qi, (unsigned)C.env.opt.rich_max_terms);
                                return TRI_OK;
                        }
                }
                const uint32_t g0 = S.gorder[0];
                const uint32_t nlead = S.gs[g0 + 1] - S.gs[g0];
                const uint64_t lead_docs = group_docs(ix, S, g0);
                Tmp t{};
                if (!S.qphrases.empty() && ix.codec == TRI_CODEC_LUCENE && !ix.has_hdir)
                        return herr(f.err, TRI_ERR_INVALID, "query %zu: phrase over a LUCENE segment that was uploaded without hits.data", qi);
                emit_phrases_and_scorers(C, f, t, wq, rich);
                t.fz = -1;
                t.truth = truth;
                if (truth)
                        slot_map_from_truth(C, f, t, tp, rich);
                else if (C.scored && C.in.topk && S.qphrases.empty() && C.env.opt.fused && fused_windows_fit(ix))
                        slot_map_from_cnf(C, f, t);
                t.q.fused_idx = 0;
                t.q.form = RESULT_DOCIDS;
                t.q.nterms = (uint32_t)uniq.size();
                t.q.term_base = (uint32_t)f.qterms.size();
                t.q.out_cap = 0;
                t.q.out_off = 0;
                t.q.qid = (uint32_t)qi;
                t.nlead = nlead;
                f.qterms.insert(f.qterms.end(), uniq.begin(), uniq.end());
                f.term_bytes += distinct_docbytes(ix, uniq.data(), uniq.size(), S.seen);
                // cost estimate: the lead group is decoded fully; every other list costs min(its blocks x 32, lead docs x 32)
                t.cost = 0;
                for (size_t i = 0; i < uniq.size(); ++i) {
                        const DevTerm &tk = ix.terms[uniq[i] & QT_TERM];
                        t.cost += i < nlead ? tk.documents : 32ull * std::min<uint64_t>(tk.nblocks, lead_docs);
                }
                classify(C, f, t, lead_docs);
                t.hidden = hidden;
                f.tmp.push_back(t);
                return TRI_OK;
        }

        // ---- first pass: lower the queries [q_lo, q_hi) of the batch into `f` and class them
        inline int lower_range(const Ctx &C, Frag &f) {
                const PlanInput &in = C.in;
                const HostIndex &ix = C.ix;
                // a query's lowering reads a handful of per-term records (directory entry, list bytes, rank by document count) at term ids drawn from
                // a vocabulary of millions: the pass is a chain of cache misses (cfg2: 280 ns per 2-term query on one thread).  The term ids stand in
                // the program's TERM tokens, so the records of the query AHEAD queries on are requested while this one is lowered
                constexpr size_t AHEAD = 6;
                auto prefetch_query = [&](const size_t q) { for_each_term_token(ix, in, q, [&](const uint32_t x) { prefetch_term(ix, x); }); };
                // ... and, half as far ahead, what hangs off those records: the directory entry of the list's last block (the query's docID range)
                auto prefetch_tails = [&](const size_t q) {
                        for_each_term_token(ix, in, q, [&](const uint32_t x) {
                                const DevTerm &tk = ix.terms[x];
                                if (tk.nblocks)
                                        __builtin_prefetch(&ix.blk_last[tk.first_block + tk.nblocks - 1]);
                        });
                };
                for (size_t q = f.q_lo; q < std::min(f.q_hi, f.q_lo + AHEAD); ++q)
                        prefetch_query(q);
                for (size_t qi = f.q_lo; qi < f.q_hi; ++qi) {
                        if (qi + AHEAD < f.q_hi)
                                prefetch_query(qi + AHEAD);
                        if (qi + AHEAD / 2 < f.q_hi)
                                prefetch_tails(qi + AHEAD / 2);
                        const tri_query &tq = in.queries[qi];
                        if ((uint64_t)tq.prog_off + tq.prog_len > in.prog_len || !tq.prog_len)
                                return herr(f.err, TRI_ERR_INVALID, "query %zu: program slice out of range", qi);
                        if (const int rc = lower_query(C, f, qi, in.prog + tq.prog_off, tq.prog_len, in.weights ? in.weights + tq.prog_off : nullptr, false))
                                return rc;
                }
                return TRI_OK;
        }

        // ---- a query the CNF lowering and the truth table leave: the tree itself goes to the device (TASK_TREE, k_tree.hpp).  Every leaf
        //      becomes a bitmap over the docID space — a term's plane row (k_term_planes, once per run for every tree query of the batch that
        //      names it), a multi-word phrase's matches (a HIDDEN query of the same batch: the conjunction of its terms + the positional check,
        //      through the kernels every phrase query takes; its match list is scattered into the row) —, the inner nodes are word-wise algebra
        //      (DocsSetIterators::Conjuction / Disjunction / DisjunctionSome / Filter / Optional, docset_iterators.cpp:226-677, as set operations),
        //      and scores / reported terms follow the reference's recursion over the iterators that sit on a match
        //      (docset_iterators_scorers.cpp:38-228, queryexec_ctx.cpp:382-520) document by document.
        inline int lower_tree(const Ctx &C, Frag &f, const size_t qi, const uint32_t *prog, const uint32_t plen, const double *wq, const int root) {
                const HostIndex &ix = C.ix;
                Scratch &S = f.S;
                auto leave_out = [&](const char *why) {
                        f.left_out.push_back(qi);
                        herr(f.err, TRI_ERR_UNSUPPORTED, "query %zu: %s", qi, why);
                        return TRI_OK;
                };
                struct PhraseLeaf {
                        uint32_t node, t0, n, tok;
                };
                struct HNode { // a node before it is written as a DevTreeNode or a DevTreeNodeW
                        uint32_t op = 0, thr = 0, arg = 0, row = 0, score = 0xffffffffu, rmask = 0, rmask_hi = 0, parent = UINT32_MAX, ord = 0, nkids = 0, kid0 = 0, kid1 = 0;
                };
                const uint32_t max_nodes = (uint32_t)C.env.opt.tree_max_nodes;
                std::vector<HNode> tn;
                std::vector<PhraseLeaf> phl;
                std::vector<uint32_t> phterms, leaf_tok; // phrase leaves' terms; per node, the program token of a leaf
                std::vector<uint8_t> positive;           // per node: a leaf an iterator of the tree can report (not under an excluded side)
                bool ok = true;
                // postfix emission (children first); returns the node's index
                std::function<int(int, bool)> emit = [&](const int ni, const bool pos) -> int {
                        const PNode x = S.nodes[ni];
                        const int *kd = S.kids(x);
                        HNode d;
                        uint32_t tok = x.tok;
                        if (x.op == TRI_OP_TERM || (x.op == TRI_OP_PHRASE && x.kid_n == 1)) {
                                const PNode &t = x.op == TRI_OP_TERM ? x : S.nodes[kd[0]];
                                d.op = TRI_OP_TERM;
                                d.arg = t.term;
                                tok = t.tok;
                                if (t.term >= ix.terms.size() || !ix.terms[t.term].documents)
                                        ok = false; // (parse_program drops what can never match: not reached)
                        } else if (x.op == TRI_OP_PHRASE) {
                                d.op = TRI_OP_PHRASE;
                                phl.push_back({(uint32_t)tn.size(), (uint32_t)phterms.size(), x.kid_n, x.tok});
                                for (uint32_t k = 0; k < x.kid_n; ++k)
                                        phterms.push_back(S.nodes[kd[k]].term);
                        } else {
                                d.op = x.op;
                                d.thr = x.op == TRI_OP_SOME ? x.term : 0;
                                std::vector<int> kids;
                                for (uint32_t k = 0; k < x.kid_n && ok; ++k)
                                        kids.push_back(emit(kd[k], pos && !(x.op == TRI_OP_NOT && k == 1)));
                                if (!ok || tn.size() + 1 > max_nodes)
                                        return ok = false, -1;
                                for (size_t k = 0; k < kids.size(); ++k) {
                                        tn[kids[k]].parent = (uint32_t)tn.size();
                                        tn[kids[k]].ord = (uint32_t)k;
                                }
                                d.nkids = (uint32_t)kids.size();
                                if (x.op == TRI_OP_NOT || x.op == TRI_OP_OPT)
                                        d.kid0 = (uint32_t)kids[0], d.kid1 = (uint32_t)kids[1];
                        }
                        if (tn.size() + 1 > max_nodes)
                                return ok = false, -1;
                        tn.push_back(d);
                        leaf_tok.push_back(tok);
                        positive.push_back(pos && (d.op == TRI_OP_TERM || d.op == TRI_OP_PHRASE));
                        return (int)tn.size() - 1;
                };
                emit(root, true);
                if (!ok) {
                        char why[64];
                        snprintf(why, sizeof why, "a tree of more than %u nodes", max_nodes);
                        return leave_out(why);
                }
                const uint32_t nn = (uint32_t)tn.size();
                // a WIDE record (k_tree_wide.hpp) for what the narrow kernels do not hold, or from tree_wide_min_nodes on.  What its kernels need per thread: the
                // evaluation stack holds, while a leaf is read, the accumulator of every ancestor — a word, or a matchsome's counter planes —, the counter stack
                // of k_tree_leaves_wide a count per ancestor: the deepest path decides
                const bool wide = nn > TREE_MAX_NODES || nn >= C.env.opt.tree_wide_min_nodes;
                uint32_t stack_need = 0, depth_need = 0;
                if (wide) {
                        std::vector<uint32_t> words(nn, 0), depth(nn, 0);
                        for (uint32_t i = nn; i-- > 0;) {
                                if (tn[i].parent != UINT32_MAX) {
                                        const HNode &p = tn[tn[i].parent];
                                        words[i] = words[tn[i].parent] + (p.op == TRI_OP_SOME ? tree_counter_planes(p.nkids) : 1u);
                                        depth[i] = depth[tn[i].parent] + 1;
                                }
                                if (!tn[i].nkids)
                                        stack_need = std::max(stack_need, words[i]), depth_need = std::max(depth_need, depth[i]);
                        }
                        if (stack_need > TREE_WIDE_STACK) {
                                char why[96];
                                snprintf(why, sizeof why, "a tree that needs more than %u words of evaluation stack (it needs %u)", TREE_WIDE_STACK, stack_need);
                                return leave_out(why);
                        }
                }
                if (C.scored && std::find(positive.begin(), positive.end(), 1) == positive.end())
                        return leave_out("a tree without a scoring leaf");
                // the value of every node for a document that holds none of the leaves, and an upper bound of a node's matches
                uint64_t ub_root = 0;
                {
                        std::vector<uint8_t> val(nn, 0);
                        std::vector<uint32_t> ntrue(nn, 0);           // per inner node: its children that hold
                        std::vector<uint64_t> ub(nn, 0), sum(nn, 0), mn(nn, UINT64_MAX); // ... the sum and the least of their bounds
                        for (uint32_t i = 0; i < nn; ++i) {
                                const HNode &d = tn[i];
                                bool v = false;
                                uint64_t u = 0;
                                switch (d.op) {
                                        case TRI_OP_TERM:
                                                u = ix.terms[d.arg].documents;
                                                break;
                                        case TRI_OP_PHRASE:
                                                u = UINT64_MAX;
                                                for (const PhraseLeaf &p : phl)
                                                        if (p.node == i)
                                                                for (uint32_t k = 0; k < p.n; ++k)
                                                                        u = std::min<uint64_t>(u, ix.terms[phterms[p.t0 + k]].documents);
                                                break;
                                        case TRI_OP_AND:
                                                v = ntrue[i] == d.nkids;
                                                u = mn[i];
                                                break;
                                        case TRI_OP_OR:
                                                v = ntrue[i] != 0;
                                                u = sum[i];
                                                break;
                                        case TRI_OP_SOME:
                                                v = ntrue[i] >= d.thr;
                                                u = sum[i];
                                                break;
                                        case TRI_OP_NOT:
                                                v = val[d.kid0] && !val[d.kid1];
                                                u = ub[d.kid0];
                                                break;
                                        case TRI_OP_OPT:
                                                v = val[d.kid0];
                                                u = ub[d.kid0];
                                                break;
                                }
                                val[i] = v;
                                ub[i] = std::min<uint64_t>(u, ix.max_doc);
                                if (d.parent != UINT32_MAX)
                                        ntrue[d.parent] += v, sum[d.parent] += ub[i], mn[d.parent] = std::min(mn[d.parent], ub[i]);
                        }
                        if (val[nn - 1])
                                return leave_out("a tree that matches documents holding none of its terms cannot be enumerated from postings");
                        if (ub[nn - 1] > 0xffffffffull)
                                return leave_out("a tree of more than 2^32 possible matches");
                        ub_root = ub[nn - 1];
                }
                // the reportable terms (default mode): what the positive leaves' iterators are, distinct, in order of first appearance in the program
                std::vector<uint32_t> rt;
                if (C.rich) {
                        auto is_pos = [&](uint32_t term) {
                                for (uint32_t i = 0; i < nn; ++i)
                                        if (positive[i] && tn[i].op == TRI_OP_TERM && tn[i].arg == term)
                                                return true;
                                for (const PhraseLeaf &p : phl)
                                        if (positive[p.node])
                                                for (uint32_t k = 0; k < p.n; ++k)
                                                        if (phterms[p.t0 + k] == term)
                                                                return true;
                                return false;
                        };
                        for (uint32_t pi = 0; pi < plen; ++pi) {
                                if ((prog[pi] >> 28) != TRI_OP_TERM)
                                        continue;
                                const uint32_t x = prog[pi] & 0x0fffffffu;
                                if (std::find(rt.begin(), rt.end(), x) == rt.end() && is_pos(x))
                                        rt.push_back(x);
                        }
                        if (rt.size() > C.env.opt.rich_max_terms) {
                                char why[64];
                                snprintf(why, sizeof why, "more than %u reportable terms", (unsigned)C.env.opt.rich_max_terms);
                                return leave_out(why);
                        }
                        // a leaf's report mask: 64 bits, the low word in rmask, the high one in rmask_hi (a phrase's terms may fall on both sides of bit 32)
                        auto bit_of = [&](uint32_t term) { return 1ull << (uint32_t)(std::find(rt.begin(), rt.end(), term) - rt.begin()); };
                        auto report = [&](HNode &h, const uint64_t m) { h.rmask |= (uint32_t)m, h.rmask_hi |= (uint32_t)(m >> 32); };
                        for (uint32_t i = 0; i < nn; ++i)
                                if (positive[i] && tn[i].op == TRI_OP_TERM)
                                        report(tn[i], bit_of(tn[i].arg));
                        for (const PhraseLeaf &p : phl)
                                if (positive[p.node])
                                        for (uint32_t k = 0; k < p.n; ++k)
                                                report(tn[p.node], bit_of(phterms[p.t0 + k]));
                }
                if (!phl.empty() && ix.codec == TRI_CODEC_LUCENE && !ix.has_hdir)
                        return herr(f.err, TRI_ERR_INVALID, "query %zu: phrase over a LUCENE segment that was uploaded without hits.data", qi);
                // ---- the phrase leaves: one hidden query each (S is reused by their lowering: nothing of this query's parse is read below)
                std::vector<double> pweight(phl.size(), 0.0);
                for (size_t pi = 0; pi < phl.size(); ++pi) {
                        const PhraseLeaf &p = phl[pi];
                        std::vector<uint32_t> hp;
                        std::vector<double> hw;
                        for (uint32_t k = 0; k < p.n; ++k)
                                hp.push_back((TRI_OP_TERM << 28) | phterms[p.t0 + k]);
                        hp.push_back((TRI_OP_PHRASE << 28) | p.n);
                        if (wq) {
                                hw.assign(p.n + 1, 0.0);
                                hw[p.n] = wq[p.tok];
                        }
                        const size_t before = f.tmp.size(), lo_before = f.left_out.size();
                        if (const int rc = lower_query(C, f, qi, hp.data(), (uint32_t)hp.size(), wq ? hw.data() : nullptr, true))
                                return rc;
                        if (f.tmp.size() != before + 1 || f.left_out.size() != lo_before) {
                                f.left_out.resize(lo_before);
                                return leave_out("a phrase leaf the planner does not lower");
                        }
                        Tmp &h = f.tmp.back();
                        h.hidden_ord = f.n_hidden++;
                        tn[p.node].arg = (uint32_t)before;                 // (fragment-relative plan slot: rebased in the fill pass)
                        tn[p.node].row = TREE_ROW_PHRASE | h.hidden_ord;   // (likewise)
                        pweight[pi] = f.phrases[h.q.phrase_base].weight;
                }
                // ---- the query itself
                Tmp t{};
                t.tree = true;
                t.tree_ub = ub_root;
                t.fz = -1;
                t.q.qid = (uint32_t)qi;
                t.q.term_base = (uint32_t)f.qterms.size();
                t.q.phrase_base = (uint32_t)f.phrases.size();
                t.q.score_base = (uint32_t)f.sterms.size();
                t.cost = ub_root;
                const size_t first_leaf = f.tree_terms.size();
                for (uint32_t i = 0; i < nn; ++i)
                        if (tn[i].op == TRI_OP_TERM)
                                f.tree_terms.push_back(tn[i].arg);
                f.term_bytes += distinct_docbytes(ix, f.tree_terms.data() + first_leaf, f.tree_terms.size() - first_leaf, S.seen);
                if (C.rich) {
                        for (uint32_t x : rt) {
                                f.sterms.push_back(x);
                                f.term_bytes += ix.hitbytes[x];
                        }
                        t.q.nscore = (uint32_t)rt.size();
                        if (t.q.nscore > RICH_NARROW_TERMS) // a wide-report query: rows of its own (BatchPlan::rich_wide), the batch-wide R stays the narrow queries'
                                ++f.rich_wide_queries;
                        else
                                f.rich_R = std::max<uint32_t>(f.rich_R, t.q.nscore);
                        f.rich_allow = true;
                } else if (C.scored) {
                        // one scorer per positive leaf, summed in tree order (docset_iterators_scorers.cpp:38-228)
                        for (uint32_t i = 0; i < nn; ++i) {
                                if (!positive[i])
                                        continue;
                                tn[i].score = t.q.nscore++;
                                if (tn[i].op == TRI_OP_TERM) {
                                        f.sterms.push_back(tn[i].arg);
                                        f.sweights.push_back(wq ? wq[leaf_tok[i]] : C.term_weight(ix.terms[tn[i].arg].documents));
                                } else { // (a phrase leaf's score comes with its hidden query's matches — k_phrase; the slot keeps the arrays parallel)
                                        size_t pi = 0;
                                        while (phl[pi].node != i)
                                                ++pi;
                                        f.sterms.push_back(phterms[phl[pi].t0]);
                                        f.sweights.push_back(pweight[pi]);
                                }
                        }
                }
                t.tree_wide = wide;
                t.q.fused_idx = (uint32_t)f.treepool.size();
                f.treepool.resize(f.treepool.size() + TREE_HDR_WORDS + nn * (sizeof(DevTreeNode) / 4), 0u);
                uint32_t *const rec = &f.treepool[t.q.fused_idx];
                rec[0] = nn;
                if (wide) {
                        rec[1] = TREE_KIND_WIDE, rec[2] = stack_need, rec[3] = depth_need;
                        DevTreeNodeW *out = reinterpret_cast<DevTreeNodeW *>(rec + TREE_HDR_WORDS);
                        for (uint32_t i = 0; i < nn; ++i) {
                                const HNode &h = tn[i];
                                DevTreeNodeW d{};
                                d.op = (uint8_t)h.op;
                                d.cbits = h.op == TRI_OP_SOME ? (uint8_t)tree_counter_planes(h.nkids) : 0;
                                d.parent = h.parent == UINT32_MAX ? (uint16_t)TREE_NO_PARENT : (uint16_t)h.parent;
                                d.arg = h.arg, d.row = h.row, d.score = h.score, d.rmask = h.rmask;
                                d.ord = (uint16_t)h.ord, d.nkids = (uint16_t)h.nkids, d.thr = (uint16_t)std::min<uint32_t>(h.thr, 0xffffu);
                                d.pad = h.rmask_hi;
                                if (h.parent != UINT32_MAX) {
                                        d.pop = (uint8_t)tn[h.parent].op;
                                        d.pcbits = tn[h.parent].op == TRI_OP_SOME ? (uint8_t)tree_counter_planes(tn[h.parent].nkids) : 0;
                                }
                                out[i] = d;
                        }
                } else {
                        DevTreeNode *out = reinterpret_cast<DevTreeNode *>(rec + TREE_HDR_WORDS);
                        for (uint32_t i = 0; i < nn; ++i) {
                                const HNode &h = tn[i];
                                DevTreeNode d{};
                                d.op = (uint8_t)h.op;
                                d.parent = h.parent == UINT32_MAX ? 0xff : (uint8_t)h.parent;
                                d.ord = (uint8_t)h.ord;
                                d.thr = (uint8_t)std::min<uint32_t>(h.thr, 255);
                                d.arg = h.arg, d.row = h.row, d.score = h.score, d.rmask = h.rmask;
                                if (h.op == TRI_OP_NOT || h.op == TRI_OP_OPT)
                                        d.kid0 = (uint8_t)h.kid0, d.kid1 = (uint8_t)h.kid1;
                                d.kids = h.rmask_hi; // (a leaf; an inner node's is 0 here and gets its children below)
                                out[i] = d;
                        }
                        for (uint32_t i = 0; i + 1 < nn; ++i)
                                out[tn[i].parent].kids |= 1ull << i;
                }
                f.tmp.push_back(t);
                return TRI_OK;
        }
} // namespace trip

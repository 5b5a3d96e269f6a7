// perc_host_eval.cpp — tools/probe_perc.py's host baseline (tooling, not part of any library of the product: the probe compiles it into build/ when it runs).
// percolator_query::match's shape (percolator.cpp:5-137: one walk over the query's nodes per (query, document), one thread) BEHIND a term -> queries candidate
// index, so that a document is only tested against the stored queries that name one of its terms (and those that hold on a document without any of theirs): the
// comparison the device's prune deserves.  Pairs come out document-major, queries ascending: tri_perc_result_pairs' TRI_PERC_BY_DOCUMENT order.
#include <algorithm>
#include <cstdint>
#include <vector>

namespace {
        struct Set {
                const uint32_t *prog;
                std::vector<uint32_t> off, len;
                std::vector<uint32_t> tq_first, tq; // term -> the queries that name it
                std::vector<uint32_t> always;       // queries that hold on the empty document
                std::vector<uint32_t> stamp;
                uint32_t round = 0;
        };
        struct Doc {
                const uint32_t *terms, *freqs;
                const uint16_t *pos;
                const uint64_t *pfirst;
                uint32_t n;
                int find(uint32_t t) const {
                        const uint32_t *p = std::lower_bound(terms, terms + n, t);
                        return p != terms + n && *p == t ? int(p - terms) : -1;
                }
        };
        bool eval(const uint32_t *p, const uint32_t n, const Doc &d) {
                struct V {
                        bool v;
                        uint32_t term;
                };
                V st[64];
                uint32_t sp = 0;
                for (uint32_t i = 0; i < n; ++i) {
                        const uint32_t op = p[i] >> 28, arg = p[i] & 0x0fffffffu;
                        if (op == 0) {
                                st[sp++] = {d.n && d.find(arg) >= 0, arg};
                                continue;
                        }
                        const uint32_t k = op == 6 ? (arg & 0xffffu) : arg;
                        const V *kid = st + sp - k;
                        uint32_t cnt = 0;
                        for (uint32_t j = 0; j < k; ++j)
                                cnt += kid[j].v;
                        bool v = false;
                        if (op == 1)
                                v = cnt == k;
                        else if (op == 2)
                                v = cnt != 0;
                        else if (op == 4)
                                v = k == 1 ? !kid[0].v : kid[0].v && !kid[1].v;
                        else if (op == 5)
                                v = kid[0].v;
                        else if (op == 6)
                                v = cnt >= (arg >> 16);
                        else if (cnt == k) { // a phrase whose words are all there
                                int at[16];
                                for (uint32_t j = 0; j < k; ++j)
                                        at[j] = d.find(kid[j].term);
                                for (uint64_t a = d.pfirst[at[0]]; a < d.pfirst[at[0]] + d.freqs[at[0]] && !v; ++a) {
                                        const uint32_t x = d.pos[a];
                                        bool ok = x != 0;
                                        for (uint32_t j = 1; j < k && ok; ++j) {
                                                const uint16_t *b = d.pos + d.pfirst[at[j]], *e = b + d.freqs[at[j]];
                                                ok = x + j <= 0xffffu && std::binary_search(b, e, uint16_t(x + j));
                                        }
                                        v = ok;
                                }
                        }
                        sp -= k;
                        st[sp++] = {v, 0};
                }
                return sp == 1 && st[0].v;
        }
} // namespace

extern "C" void *perc_host_build(const uint32_t *prog, const uint32_t *queries2, const uint64_t nq, const uint32_t nterms) {
        Set *s = new Set;
        s->prog = prog;
        std::vector<uint32_t> count(nterms + 1, 0);
        const Doc none{nullptr, nullptr, nullptr, nullptr, 0};
        for (int pass = 0; pass < 2; ++pass) {
                for (uint64_t q = 0; q < nq; ++q) {
                        const uint32_t *p = prog + queries2[2 * q], n = queries2[2 * q + 1];
                        if (!pass) {
                                s->off.push_back(queries2[2 * q]);
                                s->len.push_back(n);
                                if (eval(p, n, none))
                                        s->always.push_back(uint32_t(q));
                        }
                        for (uint32_t i = 0; i < n; ++i)
                                if ((p[i] >> 28) == 0) {
                                        if (!pass)
                                                ++count[p[i] & 0x0fffffffu];
                                        else
                                                s->tq[s->tq_first[p[i] & 0x0fffffffu] + count[p[i] & 0x0fffffffu]++] = uint32_t(q);
                                }
                }
                if (!pass) {
                        s->tq_first.assign(nterms + 1, 0);
                        for (uint32_t t = 0; t < nterms; ++t)
                                s->tq_first[t + 1] = s->tq_first[t] + count[t];
                        s->tq.resize(s->tq_first[nterms]);
                        std::fill(count.begin(), count.end(), 0u);
                }
        }
        s->stamp.assign(nq, 0);
        return s;
}
extern "C" void perc_host_free(void *h) { delete static_cast<Set *>(h); }

// returns the pairs (at most cap are stored); *evaluated: the (query, document) walks it took
extern "C" uint64_t perc_host_match(void *h, const uint64_t *doc_first, const uint32_t *terms, const uint32_t *freqs, const uint16_t *positions, const uint32_t ndocs, uint32_t *out_q,
                                    uint32_t *out_d, const uint64_t cap, uint64_t *evaluated) {
        Set &s = *static_cast<Set *>(h);
        std::vector<uint64_t> pfirst(doc_first[ndocs] + 1, 0);
        for (uint64_t i = 0; i < doc_first[ndocs]; ++i)
                pfirst[i + 1] = pfirst[i] + freqs[i];
        uint64_t n = 0, walks = 0;
        std::vector<uint32_t> cand;
        for (uint32_t d = 0; d < ndocs; ++d) {
                const uint64_t lo = doc_first[d];
                const Doc doc{terms + lo, freqs + lo, positions, pfirst.data() + lo, uint32_t(doc_first[d + 1] - lo)};
                ++s.round;
                cand = s.always;
                for (const uint32_t q : cand)
                        s.stamp[q] = s.round;
                for (uint32_t i = 0; i < doc.n; ++i) {
                        if (doc.terms[i] + 1 >= s.tq_first.size())
                                continue;
                        for (uint32_t k = s.tq_first[doc.terms[i]]; k < s.tq_first[doc.terms[i] + 1]; ++k)
                                if (s.stamp[s.tq[k]] != s.round) {
                                        s.stamp[s.tq[k]] = s.round;
                                        cand.push_back(s.tq[k]);
                                }
                }
                std::sort(cand.begin(), cand.end());
                walks += cand.size();
                for (const uint32_t q : cand)
                        if (eval(s.prog + s.off[q], s.len[q], doc)) {
                                if (n < cap)
                                        out_q[n] = q, out_d[n] = d;
                                ++n;
                        }
        }
        *evaluated = walks;
        return n;
}

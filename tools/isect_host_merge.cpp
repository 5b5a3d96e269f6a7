// isect_host_merge.cpp — tools/probe_isect.py's host baseline (tooling, not part of any library of the product: the probe compiles it into build/ when it runs).
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

// Trinity::intersect (intersect.cpp:5-170) over lists that are already decoded (tri_decode_terms) — the merge is the reference's
// shape, a linear scan over the open lists per document for the lowest current docID (:107-158), and the antichain with its `map == mapPrev` shortcut
// (:64-91); the order is finalize's with ties by ascending mask (tri_isect_results' order).  One thread.  docs[offs[i] .. offs[i + 1]) = list i, ascending;
// group[i] = its token group; masked: a bitmap over docIDs or null.  Returns the entries (at most cap are stored).
extern "C" uint64_t tri_host_isect_merge(const uint32_t *docs, const uint64_t *offs, const uint8_t *group, const uint32_t nlists, const uint64_t orig_mask, const uint64_t stop_mask,
                                         const uint32_t *masked, uint64_t *masks_out, uint32_t *counts_out, const uint64_t cap) {
        struct Open {
                const uint32_t *p, *e;
                uint8_t g;
        };
        std::vector<Open> open;
        for (uint32_t i = 0; i < nlists; ++i)
                if (offs[i + 1] > offs[i])
                        open.push_back({docs + offs[i], docs + offs[i + 1], group[i]});
        std::vector<std::pair<uint64_t, uint32_t>> m;
        uint64_t prev = 0;
        size_t iprev = 0;
        std::vector<size_t> sel;
        while (!open.empty()) {
                uint32_t lowest = *open[0].p;
                uint64_t mask = 1ull << open[0].g;
                sel.assign(1, 0);
                for (size_t i = 1; i < open.size(); ++i) {
                        const uint32_t d = *open[i].p;
                        if (d == lowest) {
                                mask |= 1ull << open[i].g;
                                sel.push_back(i);
                        } else if (d < lowest) {
                                lowest = d;
                                mask = 1ull << open[i].g;
                                sel.assign(1, i);
                        }
                }
                const uint64_t ends = (mask & (0ull - mask)) | (1ull << (63 - __builtin_clzll(mask)));
                if (mask != orig_mask && !(stop_mask & ends) && !(masked && ((masked[lowest >> 5] >> (lowest & 31u)) & 1u))) {
                        if (mask == prev)
                                ++m[iprev].second;
                        else {
                                prev = mask;
                                size_t i = 0;
                                bool covered = false;
                                while (i < m.size()) {
                                        const uint64_t v = m[i].first;
                                        if ((v & mask) == mask) {
                                                m[i].second += v == mask;
                                                iprev = i;
                                                covered = true;
                                                break;
                                        }
                                        if ((mask & v) == v) {
                                                m[i] = m.back();
                                                m.pop_back();
                                        } else
                                                ++i;
                                }
                                if (!covered) {
                                        iprev = m.size();
                                        m.emplace_back(mask, 1u);
                                }
                        }
                }
                while (!sel.empty()) { // (from the back: a list that ends is replaced by the last open one, which has been advanced already)
                        const size_t i = sel.back();
                        sel.pop_back();
                        if (++open[i].p == open[i].e) {
                                open[i] = open.back();
                                open.pop_back();
                        }
                }
        }
        std::sort(m.begin(), m.end(), [](const std::pair<uint64_t, uint32_t> &a, const std::pair<uint64_t, uint32_t> &b) {
                const int pa = __builtin_popcountll(a.first), pb = __builtin_popcountll(b.first);
                return pa != pb ? pa > pb : a.second != b.second ? a.second > b.second : a.first < b.first;
        });
        for (size_t i = 0; i < m.size() && i < cap; ++i) {
                masks_out[i] = m[i].first;
                counts_out[i] = m[i].second;
        }
        return m.size();
}

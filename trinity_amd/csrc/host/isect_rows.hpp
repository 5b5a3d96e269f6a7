// isect_rows.hpp — the host half of tri_isect_run (isect_side.hpp): Trinity::intersect's answer (intersect.cpp:5-170) derived from the two order-free tables the
// device builds (k_isect.hpp).  Plain functions over vectors, no HIP, so that they compile and are tested on a CPU alone (tests/cpp/isect_rows_cpu_test.cpp).
//
// The reference walks the union of the tokens' lists in docID order and hands every CONSIDERED document's mask to ctx::consider (:64-91), which keeps an
// antichain in a vector: a mask with a superset-or-equal entry is dropped (an equal one is counted), a mask without one deletes its strict subsets by
// swap-removal (their counts are lost) and is pushed.  The shortcut `map == mapPrev` (:65-66) credits the 2nd, 3rd ... document of a run of equal masks to
// matches[indexPrev] — for a mask that is NOT in the vector that is the first entry, in vector order, that covers it.  The vector changes only when a mask
// occurs for the first time (a mask a superset removed never returns: a superset of it stays), so:
//   H   per distinct considered mask: its documents, its first docID
//   C   per (mask m, epoch e): the considered documents of mask m whose preceding considered document has mask m too — epoch e = the distinct masks first
//       seen at or before the document; only documents at or past threshold(m), from where m is absent from the vector, are counted
// give the list exactly: the vector is replayed over the distinct masks in order of first docID (same scan, same swap-removal, same push), after step e the C
// entries of epoch e are credited to the first covering entry, and a surviving entry counts H[mask] + its credits.
// NOT copied (include/trinity_hip.h says so too): indexPrev is a uint8_t in the reference and wraps once the vector holds more than 255 entries; here it is
// full-width.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace isect_rows {
        struct HEntry {
                uint64_t mask;
                uint32_t count, first;
        };
        struct CEntry {
                uint64_t mask;
                uint32_t epoch, count;
        };
        constexpr uint32_t NEVER = 0xffffffffu;

        inline void sort_by_first(std::vector<HEntry> &h) {
                std::sort(h.begin(), h.end(), [](const HEntry &a, const HEntry &b) { return a.first < b.first; });
        }

        // h sorted by first docID -> per entry the docID from which its mask is absent from the reference's vector: the later of its own first document and the
        // earliest first document of a strict superset; NEVER: it has no strict superset (it stays, all its documents are counted by H).  A mask with a superset
        // stops at the first one; only the maximal masks — the antichain, small — look at every entry
        inline std::vector<uint32_t> thresholds(const std::vector<HEntry> &h) {
                std::vector<uint32_t> thr(h.size(), NEVER);
                for (size_t i = 0; i < h.size(); ++i)
                        for (size_t j = 0; j < h.size(); ++j) // (ascending first docID: the first strict superset met is the earliest)
                                if (j != i && (h[j].mask & h[i].mask) == h[i].mask) {
                                        thr[i] = std::max(h[i].first, h[j].first);
                                        break;
                                }
                return thr;
        }

        // h sorted by first docID, thr = thresholds(h) -> the most entries table C can hold: a mask with a threshold is counted under the epochs from its
        // threshold's on — one key each —, a mask without one under none
        inline uint64_t runs_bound(const std::vector<HEntry> &h, const std::vector<uint32_t> &thr) {
                uint64_t n = 0;
                for (size_t i = 0; i < h.size(); ++i)
                        if (thr[i] != NEVER) {
                                const size_t e = size_t(std::upper_bound(h.begin(), h.end(), thr[i], [](const uint32_t d, const HEntry &x) { return d < x.first; }) - h.begin());
                                n += h.size() - e + 1; // (e: the epoch at the threshold — the entries first seen at or before it)
                        }
                return n;
        }

        inline int popcnt(const uint64_t v) { return __builtin_popcountll(v); }

        // finalize (:93-99): popcount descending, then count descending; the reference's std::sort leaves ties unspecified — here ascending mask
        inline void finalize(std::vector<std::pair<uint64_t, uint32_t>> &v) {
                std::sort(v.begin(), v.end(), [](const std::pair<uint64_t, uint32_t> &a, const std::pair<uint64_t, uint32_t> &b) {
                        const int pa = popcnt(a.first), pb = popcnt(b.first);
                        if (pa != pb)
                                return pa > pb;
                        if (a.second != b.second)
                                return a.second > b.second;
                        return a.first < b.first;
                });
        }

        // the reference's list from H and C (c in any order; entries whose mask is in the vector at their epoch are ignored: H counts those documents)
        inline std::vector<std::pair<uint64_t, uint32_t>> replay(std::vector<HEntry> h, std::vector<CEntry> c) {
                sort_by_first(h);
                std::sort(c.begin(), c.end(), [](const CEntry &a, const CEntry &b) { return a.epoch < b.epoch; });
                struct Match {
                        uint64_t v;
                        uint32_t cnt; // H's documents, then the credits
                };
                std::vector<Match> matches;
                size_t ci = 0;
                while (ci < c.size() && c[ci].epoch == 0)
                        ++ci;
                for (size_t e = 1; e <= h.size(); ++e) {
                        const uint64_t map = h[e - 1].mask;
                        size_t n = matches.size(), i = 0;
                        bool covered = false;
                        while (i < n) { // :72-86
                                const uint64_t v = matches[i].v;
                                if ((v & map) == map) {
                                        covered = true;
                                        break;
                                } else if ((map & v) == v) {
                                        matches[i] = matches.back();
                                        matches.pop_back();
                                        --n;
                                } else
                                        ++i;
                        }
                        if (!covered)
                                matches.push_back({map, h[e - 1].count}); // (it stays until a strict superset arrives: every document of it is counted while it is here)
                        for (; ci < c.size() && c[ci].epoch == e; ++ci)
                                for (Match &m : matches)
                                        if ((m.v & c[ci].mask) == c[ci].mask) {
                                                if (m.v != c[ci].mask)
                                                        m.cnt += c[ci].count; // (uint32_t, wraps as the reference's cnt does)
                                                break;
                                        }
                }
                std::vector<std::pair<uint64_t, uint32_t>> out;
                out.reserve(matches.size());
                for (const Match &m : matches)
                        out.emplace_back(m.v, m.cnt);
                finalize(out);
                return out;
        }
} // namespace isect_rows

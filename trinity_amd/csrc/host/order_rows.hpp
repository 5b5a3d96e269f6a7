// order_rows.hpp — ordering by a column on the host: the rule k_order.hpp applies on the device, as plain functions over pointers and counts, no HIP, so that they
// compile and are tested on a CPU alone (tests/cpp/order_cpu_test.cpp).  ColumnOrder's replay path (trinity_gpu.hpp) selects with them; tri_batch_ordered and
// tri_cbatch_ordered split the device's keys with them.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace order_rows {
        // the key of document `id`: (descending ? ~value : value) << 32 | id — smaller is better, ties in the value go to the lower docID in both directions.  A docID
        // the column (n entries) does not cover is never read: it takes the value 0xffffffff
        inline uint64_t key(const uint32_t *values, const size_t n, const bool descending, const uint32_t id) {
                const uint32_t v = id < n ? values[id] : 0xffffffffu;
                return uint64_t(descending ? ~v : v) << 32 | id;
        }
        inline uint32_t docid_of(const uint64_t key) { return uint32_t(key); }
        inline uint32_t value_of(const uint64_t key, const bool descending) { return descending ? ~uint32_t(key >> 32) : uint32_t(key >> 32); }

        // consider(id) / consider(ids, cnt): `best` holds the k smallest keys seen so far, ascending; cnt more documents are offered
        inline void offer(std::vector<uint64_t> &best, const uint32_t *values, const size_t n, const size_t k, const bool descending, const uint32_t *ids, const size_t cnt) {
                for (size_t i = 0; i < cnt; ++i) {
                        const uint64_t x = key(values, n, descending, ids[i]);
                        if (best.size() == k && (!k || x >= best.back()))
                                continue;
                        best.insert(std::upper_bound(best.begin(), best.end(), x), x);
                        if (best.size() > k)
                                best.pop_back();
                }
        }

        // the first k of a docID set: its keys, ascending
        inline std::vector<uint64_t> first_k(const uint32_t *ids, const size_t cnt, const uint32_t *values, const size_t n, const size_t k, const bool descending) {
                std::vector<uint64_t> best;
                offer(best, values, n, k, descending, ids, cnt);
                return best;
        }

        // a collection: the parts' ascending lists (oldest source first) merged by (key, source), cut at k — equal keys of different sources both stay
        inline std::vector<uint64_t> blend(const std::vector<std::vector<uint64_t>> &parts, const size_t k) {
                std::vector<uint64_t> out;
                for (const auto &p : parts) {
                        const size_t mid = out.size();
                        out.insert(out.end(), p.begin(), p.end());
                        std::inplace_merge(out.begin(), out.begin() + ptrdiff_t(mid), out.end()); // (stable: of equal keys the older source's stays first)
                }
                if (out.size() > k)
                        out.resize(k);
                return out;
        }

        // rows of k keys -> the caller's docids[] and values[] (entries past a row's count hold zero keys: zero in both)
        inline void split(const uint64_t *keys, const uint32_t *counts, const size_t rows, const size_t k, const bool descending, uint32_t *docids, uint32_t *values) {
                for (size_t r = 0; r < rows; ++r)
                        for (size_t i = 0; i < k; ++i) {
                                const bool live = i < counts[r];
                                docids[r * k + i] = live ? docid_of(keys[r * k + i]) : 0u;
                                values[r * k + i] = live ? value_of(keys[r * k + i], descending) : 0u;
                        }
        }
} // namespace order_rows

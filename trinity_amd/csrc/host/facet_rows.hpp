// facet_rows.hpp — facet counting on the host: the rule k_facet.hpp applies on the device, as plain functions over pointers and counts, no HIP, so that they
// compile and are tested on a CPU alone (tests/cpp/facet_cpu_test.cpp).  FacetCounter's replay path (trinity_gpu.hpp) and tri_cbatch_facets' sum use them.
#pragma once
#include <cstddef>
#include <cstdint>

namespace facet_rows {
        // the counter of a row of nbuckets + 1 that document `id` falls into: min(values[id], nbuckets) — the last counter is the overflow bucket; a docID the
        // column (n entries) does not cover is never read and counts there too
        inline uint32_t bucket(const uint32_t *values, const size_t n, const uint32_t nbuckets, const uint32_t id) {
                const uint32_t v = id < n ? values[id] : 0xffffffffu;
                return v < nbuckets ? v : nbuckets;
        }

        // consider(id) / consider(ids, cnt): row[bucket] goes up by one per document
        inline void count(uint32_t *row, const uint32_t *values, const size_t n, const uint32_t nbuckets, const uint32_t *ids, const size_t cnt) {
                for (size_t i = 0; i < cnt; ++i)
                        ++row[bucket(values, n, nbuckets, ids[i])];
        }

        // a collection: a part's 32-bit counters added to the 64-bit sums
        inline void add(uint64_t *sum, const uint32_t *part, const size_t counters) {
                for (size_t i = 0; i < counters; ++i)
                        sum[i] += part[i];
        }
} // namespace facet_rows

// stats_rows.hpp — stats of a column per bucket on the host: the rule k_stats.hpp applies on the device, as plain functions over pointers and counts, no HIP, so that
// they compile and are tested on a CPU alone (tests/cpp/stats_cpu_test.cpp).  StatsCounter's replay path (trinity_gpu.hpp) aggregates with them; tri_cbatch_stats
// combines the parts' rows with them.
#pragma once
#include <cstddef>
#include <cstdint>

namespace stats_rows {
        // what a bucket knows of the documents it took; an empty one reads count 0, sum 0, min 0xffffffff, max 0
        struct Record {
                uint64_t sum = 0;
                uint64_t count = 0; // (32 bits hold one source's; a collection's is the sum of its parts')
                uint32_t min = 0xffffffffu, max = 0;
        };

        // the record of a row of nbuckets + 1 that document `id` falls into: min(group[id], nbuckets) — the last is the overflow bucket; a docID the column (n entries)
        // does not cover is never read and falls there too.  No group column: the one record 0
        inline uint32_t bucket(const uint32_t *group, const size_t n, const uint32_t nbuckets, const uint32_t id) {
                if (!group)
                        return 0;
                const uint32_t g = id < n ? group[id] : 0xffffffffu;
                return g < nbuckets ? g : nbuckets;
        }

        // ... and the value it brings (a docID the column does not cover: 0xffffffff, never read)
        inline uint32_t value_of(const uint32_t *value, const size_t n, const uint32_t id) { return id < n ? value[id] : 0xffffffffu; }

        // consider(id) / consider(ids, cnt): the record of every document's bucket takes its value.  row: nbuckets + 1 records (one when group is null)
        inline void count(Record *row, const uint32_t *group, const uint32_t *value, const size_t n, const uint32_t nbuckets, const uint32_t *ids, const size_t cnt) {
                for (size_t i = 0; i < cnt; ++i) {
                        Record &r = row[bucket(group, n, nbuckets, ids[i])];
                        const uint32_t v = value_of(value, n, ids[i]);
                        r.count += 1;
                        r.sum += v;
                        r.min = v < r.min ? v : r.min;
                        r.max = v > r.max ? v : r.max;
                }
        }

        // a collection: a part's records combined into the totals — counts and sums added, mins and maxs folded.  part(i) is the part's record i.  Returns `records`
        // when all were combined; the index of the FIRST record whose summed sum would wrap 64 bits otherwise, with nothing of the totals changed
        template <class Part>
        inline size_t add_records(Record *total, const size_t records, Part &&part) {
                for (size_t i = 0; i < records; ++i)
                        if (total[i].sum + part(i).sum < total[i].sum)
                                return i;
                for (size_t i = 0; i < records; ++i) {
                        const Record p = part(i);
                        Record &r = total[i];
                        r.sum += p.sum;
                        r.count += p.count;
                        r.min = p.min < r.min ? p.min : r.min;
                        r.max = p.max > r.max ? p.max : r.max;
                }
                return records;
        }
        // ... a part as the four planes tri_batch_stats delivers (tri_cbatch_stats, StatsCounter::read)
        inline size_t add(Record *total, const uint64_t *sums, const uint32_t *counts, const uint32_t *mins, const uint32_t *maxs, const size_t records) {
                return add_records(total, records, [&](const size_t i) {
                        Record r;
                        r.sum = sums[i], r.count = counts[i], r.min = mins[i], r.max = maxs[i];
                        return r;
                });
        }
        // ... and a part held as records (StatsCounter::combine)
        inline size_t add(Record *total, const Record *part, const size_t records) {
                return add_records(total, records, [&](const size_t i) { return part[i]; });
        }
} // namespace stats_rows

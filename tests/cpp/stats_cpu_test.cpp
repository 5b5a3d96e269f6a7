// stats_cpu_test.cpp — csrc/host/stats_rows.hpp (the host aggregation behind StatsCounter::consider and tri_cbatch_stats' combine) over the cases of
// tests/stats_cases.py, on a CPU alone.  Built and run by tests/test_stats_cases.py with -fsanitize=address,undefined.      usage: stats_cpu_test <vectors>
// The vectors are words of text:  ncols  { n values[n] }*   ncases  { group (or -1) value nbuckets cnt ids[cnt] sums[w] counts[w] mins[w] maxs[w] }*  with w = nbuckets + 1
// Every case is aggregated twice — document by document (consider(id)) and in uneven runs (consider(ids, cnt)) — and compared with the file's planes; both halves of
// its documents, aggregated apart, are combined by add() and compared again; then the edges no file holds: a docID the columns do not cover, an empty run, and two
// parts whose sums wrap 64 bits, which add() must refuse with nothing changed.
#include "../../trinity_amd/csrc/host/stats_rows.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

using stats_rows::Record;

static bool read_u64(FILE *f, uint64_t &v) {
        unsigned long long x = 0;
        if (fscanf(f, "%llu", &x) != 1)
                return false;
        v = x;
        return true;
}
static bool read_u32(FILE *f, uint32_t &v) {
        uint64_t x = 0;
        if (!read_u64(f, x))
                return false;
        v = (uint32_t)x;
        return true;
}
static bool read_i64(FILE *f, long long &v) { return fscanf(f, "%lld", &v) == 1; }

static bool equal(const std::vector<Record> &a, const std::vector<Record> &b) {
        for (size_t i = 0; i < a.size(); ++i)
                if (a[i].sum != b[i].sum || a[i].count != b[i].count || a[i].min != b[i].min || a[i].max != b[i].max)
                        return false;
        return a.size() == b.size();
}

// a row as the four planes a part delivers
struct Planes {
        std::vector<uint64_t> sums;
        std::vector<uint32_t> counts, mins, maxs;
        explicit Planes(const std::vector<Record> &r) {
                for (const Record &x : r) {
                        sums.push_back(x.sum);
                        counts.push_back((uint32_t)x.count);
                        mins.push_back(x.min);
                        maxs.push_back(x.max);
                }
        }
};

int main(int argc, char **argv) {
        if (argc != 2)
                return fprintf(stderr, "usage: stats_cpu_test <vectors>\n"), 2;
        FILE *f = fopen(argv[1], "r");
        if (!f)
                return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
        uint32_t ncols = 0, ncases = 0;
        if (!read_u32(f, ncols))
                return 2;
        std::vector<std::vector<uint32_t>> cols(ncols);
        for (auto &c : cols) {
                uint32_t n = 0;
                if (!read_u32(f, n))
                        return 2;
                c.resize(n);
                for (auto &v : c)
                        if (!read_u32(f, v))
                                return 2;
        }
        if (!read_u32(f, ncases))
                return 2;
        int bad = 0;
        for (uint32_t i = 0; i < ncases; ++i) {
                long long grp = 0;
                uint32_t val = 0, nb = 0, cnt = 0;
                if (!read_i64(f, grp) || !read_u32(f, val) || !read_u32(f, nb) || !read_u32(f, cnt) || val >= ncols || grp >= (long long)ncols || (grp < 0 && nb))
                        return 2;
                std::vector<uint32_t> ids(cnt);
                for (auto &v : ids)
                        if (!read_u32(f, v))
                                return 2;
                std::vector<Record> want(nb + 1), one(nb + 1), runs(nb + 1), lo(nb + 1), hi(nb + 1), both(nb + 1);
                for (auto &r : want)
                        if (!read_u64(f, r.sum))
                                return 2;
                for (auto &r : want)
                        if (!read_u64(f, r.count))
                                return 2;
                for (auto &r : want)
                        if (!read_u32(f, r.min))
                                return 2;
                for (auto &r : want)
                        if (!read_u32(f, r.max))
                                return 2;
                const uint32_t *g = grp < 0 ? nullptr : cols[(size_t)grp].data();
                const std::vector<uint32_t> &v = cols[val];
                for (uint32_t k = 0; k < cnt; ++k)
                        stats_rows::count(one.data(), g, v.data(), v.size(), nb, &ids[k], 1);
                for (size_t at = 0, step = 1; at < cnt; at += step, step = step * 3 + 1) // runs of 1, 4, 13, ... documents
                        stats_rows::count(runs.data(), g, v.data(), v.size(), nb, ids.data() + at, std::min<size_t>(step, cnt - at));
                stats_rows::count(lo.data(), g, v.data(), v.size(), nb, ids.data(), cnt / 2);
                stats_rows::count(hi.data(), g, v.data(), v.size(), nb, ids.data() + cnt / 2, cnt - cnt / 2);
                for (const auto *part : {&lo, &hi}) {
                        const Planes p(*part);
                        if (stats_rows::add(both.data(), p.sums.data(), p.counts.data(), p.mins.data(), p.maxs.data(), nb + 1) != nb + 1)
                                ++bad;
                }
                if (!equal(one, want) || !equal(runs, want) || !equal(both, want)) {
                        fprintf(stderr, "case %u (group %lld, value %u, %u buckets, %u documents): rows differ\n", i, grp, val, nb, cnt);
                        ++bad;
                }
        }
        fclose(f);
        // ---- edges
        const uint32_t grp[4] = {9, 0, 2, 1}, val[4] = {7, 0xffffffffu, 5, 0xffffffffu};
        const uint32_t ids[5] = {1, 2, 3, 4, 0xffffffffu}; // (4 and 0xffffffff: past the columns — the overflow bucket and the value 0xffffffff, never read)
        std::vector<Record> row(3), single(1);
        stats_rows::count(row.data(), grp, val, 4, 2, ids, 5);
        stats_rows::count(row.data(), grp, val, 4, 2, ids, 0);
        stats_rows::count(row.data(), grp, val, 4, 2, nullptr, 0);
        stats_rows::count(single.data(), nullptr, val, 4, 0, ids, 5);
        const bool row_ok = row[0].count == 1 && row[0].sum == 0xffffffffull && row[0].min == 0xffffffffu && row[0].max == 0xffffffffu && // docID 1: group 0
                            row[1].count == 1 && row[1].sum == 0xffffffffull &&                                                           // docID 3: group 1
                            row[2].count == 3 && row[2].sum == 5 + 2 * 0xffffffffull && row[2].min == 5 && row[2].max == 0xffffffffu;     // docIDs 2 (group 2), 4 and 0xffffffff
        const bool single_ok = single[0].count == 5 && single[0].sum == 5 + 4 * 0xffffffffull && single[0].min == 5 && single[0].max == 0xffffffffu;
        if (!row_ok || !single_ok) {
                fprintf(stderr, "edges: a docID the columns do not cover, empty runs\n");
                ++bad;
        }
        const Record none;
        if (none.count || none.sum || none.min != 0xffffffffu || none.max) {
                fprintf(stderr, "edges: the empty record\n");
                ++bad;
        }
        // two parts' sums that wrap 64 bits in record 1: refused, naming the record, NOTHING changed (record 0 included)
        std::vector<Record> total(2);
        const uint64_t a_sums[2] = {3, 0xfffffffffffffff0ull}, b_sums[2] = {4, 0x10};
        const uint32_t cnts[2] = {1, 2}, mins[2] = {3, 1}, maxs[2] = {3, 9};
        const size_t first = stats_rows::add(total.data(), a_sums, cnts, mins, maxs, 2);
        const size_t second = stats_rows::add(total.data(), b_sums, cnts, mins, maxs, 2);
        if (first != 2 || second != 1 || total[0].sum != 3 || total[0].count != 1 || total[1].sum != 0xfffffffffffffff0ull || total[1].count != 2) {
                fprintf(stderr, "edges: a wrapping sum must be refused with nothing changed (%zu %zu)\n", first, second);
                ++bad;
        }
        const uint64_t c_sums[2] = {4, 0xf}; // ... and one below the wrap is taken: 2^64 - 1
        if (stats_rows::add(total.data(), c_sums, cnts, mins, maxs, 2) != 2 || total[1].sum != 0xffffffffffffffffull || total[1].count != 4 || total[0].sum != 7) {
                fprintf(stderr, "edges: 2^64 - 1 is a sum\n");
                ++bad;
        }
        printf("cases %u bad %d\n", ncases, bad);
        return bad ? 1 : 0;
}

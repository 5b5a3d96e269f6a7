// facet_cpu_test.cpp — csrc/host/facet_rows.hpp (the host counting behind FacetCounter::consider, trinity_gpu.hpp) over the cases of tests/facet_cases.py, on a CPU alone.
// Built and run by tests/test_facet_cases.py with -fsanitize=address,undefined.      usage: facet_cpu_test <vectors>
// The vectors are words of text:  ncols  { n values[n] }*   ncases  { col nbuckets cnt ids[cnt] row[nbuckets + 1] }*
// Every case is counted twice — document by document (consider(id)) and in uneven runs (consider(ids, cnt)) — and compared with the file's row; then the edges no
// file holds: a docID the column does not cover, an empty run, a part added to 64-bit sums that pass 2^32.
#include "../../trinity_amd/csrc/host/facet_rows.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

static bool read_u32(FILE *f, uint32_t &v) {
        unsigned long long x = 0;
        if (fscanf(f, "%llu", &x) != 1)
                return false;
        v = (uint32_t)x;
        return true;
}

int main(int argc, char **argv) {
        if (argc != 2)
                return fprintf(stderr, "usage: facet_cpu_test <vectors>\n"), 2;
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
                uint32_t col = 0, nb = 0, cnt = 0;
                if (!read_u32(f, col) || !read_u32(f, nb) || !read_u32(f, cnt) || col >= ncols)
                        return 2;
                std::vector<uint32_t> ids(cnt), want(nb + 1), one(nb + 1, 0), runs(nb + 1, 0);
                for (auto &v : ids)
                        if (!read_u32(f, v))
                                return 2;
                for (auto &v : want)
                        if (!read_u32(f, v))
                                return 2;
                const std::vector<uint32_t> &c = cols[col];
                for (uint32_t k = 0; k < cnt; ++k)
                        facet_rows::count(one.data(), c.data(), c.size(), nb, &ids[k], 1);
                for (size_t at = 0, step = 1; at < cnt; at += step, step = step * 3 + 1) // runs of 1, 4, 13, ... documents
                        facet_rows::count(runs.data(), c.data(), c.size(), nb, ids.data() + at, std::min<size_t>(step, cnt - at));
                if (one != want || runs != want) {
                        fprintf(stderr, "case %u (column %u, %u buckets, %u documents): rows differ\n", i, col, nb, cnt);
                        ++bad;
                }
        }
        fclose(f);
        // ---- edges
        const uint32_t vals[4] = {9, 0, 2, 0xffffffffu};
        uint32_t row[3] = {0, 0, 0};
        const uint32_t ids[5] = {1, 2, 3, 4, 0xffffffffu}; // (4 and 0xffffffff: past the column — overflow, never read)
        facet_rows::count(row, vals, 4, 2, ids, 5);
        facet_rows::count(row, vals, 4, 2, ids, 0);
        facet_rows::count(row, vals, 4, 2, nullptr, 0);
        if (row[0] != 1 || row[1] != 0 || row[2] != 4) {
                fprintf(stderr, "edges: row %u %u %u, want 1 0 4\n", row[0], row[1], row[2]);
                ++bad;
        }
        uint64_t sum[2] = {0xfffffffful, 5};
        const uint32_t part[2] = {0xffffffffu, 0};
        facet_rows::add(sum, part, 2);
        facet_rows::add(sum, part, 0);
        if (sum[0] != 0x1fffffffeull || sum[1] != 5) {
                fprintf(stderr, "edges: the 64-bit sums are wrong\n");
                ++bad;
        }
        printf("cases %u bad %d\n", ncases, bad);
        return bad ? 1 : 0;
}

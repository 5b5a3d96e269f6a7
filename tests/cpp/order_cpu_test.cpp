// order_cpu_test.cpp — csrc/host/order_rows.hpp (the host selection behind ColumnOrder::consider, trinity_gpu.hpp, and the split of the device's keys) over the cases of
// tests/order_cases.py, on a CPU alone.  Built and run by tests/test_order_cases.py with -fsanitize=address,undefined.      usage: order_cpu_test <vectors>
// The vectors are words of text:  ncols  { n values[n] }*   ncases  { col k descending cnt ids[cnt] want want_ids[want] want_values[want] }*
//                                 nblends { k descending nparts { col cnt ids[cnt] }* want want_ids[want] want_values[want] }*
// Every case is selected twice — document by document (consider(id)) and in uneven runs (consider(ids, cnt)) — and compared with the file's row; a blend selects each
// part with first_k and merges; then the edges no file holds: a docID the column does not cover, k = 0, an empty run, equal keys of two parts, split's zeros.
#include "../../trinity_amd/csrc/host/order_rows.hpp"
#include <cstdio>
#include <cstdlib>

static bool read_u32(FILE *f, uint32_t &v) {
        unsigned long long x = 0;
        if (fscanf(f, "%llu", &x) != 1)
                return false;
        v = (uint32_t)x;
        return true;
}

static bool read_vec(FILE *f, std::vector<uint32_t> &v) {
        uint32_t n = 0;
        if (!read_u32(f, n))
                return false;
        v.resize(n);
        for (auto &x : v)
                if (!read_u32(f, x))
                        return false;
        return true;
}

// keys -> (ids, values) through split, one row
static bool same(const std::vector<uint64_t> &keys, const size_t k, const bool desc, const std::vector<uint32_t> &ids, const std::vector<uint32_t> &vals) {
        std::vector<uint64_t> row(keys);
        row.resize(k, 0);
        const uint32_t cnt = (uint32_t)keys.size();
        std::vector<uint32_t> d(k, 77), v(k, 77);
        order_rows::split(row.data(), &cnt, 1, k, desc, d.data(), v.data());
        if (keys.size() != ids.size())
                return false;
        for (size_t i = 0; i < k; ++i)
                if (d[i] != (i < cnt ? ids[i] : 0u) || v[i] != (i < cnt ? vals[i] : 0u))
                        return false;
        return true;
}

int main(int argc, char **argv) {
        if (argc != 2)
                return fprintf(stderr, "usage: order_cpu_test <vectors>\n"), 2;
        FILE *f = fopen(argv[1], "r");
        if (!f)
                return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
        uint32_t ncols = 0, ncases = 0, nblends = 0;
        if (!read_u32(f, ncols))
                return 2;
        std::vector<std::vector<uint32_t>> cols(ncols);
        for (auto &c : cols)
                if (!read_vec(f, c))
                        return 2;
        if (!read_u32(f, ncases))
                return 2;
        int bad = 0;
        for (uint32_t i = 0; i < ncases; ++i) {
                uint32_t col = 0, k = 0, desc = 0;
                std::vector<uint32_t> ids, want_ids, want_vals;
                if (!read_u32(f, col) || !read_u32(f, k) || !read_u32(f, desc) || col >= ncols || !read_vec(f, ids) || !read_vec(f, want_ids))
                        return 2;
                want_vals.resize(want_ids.size());
                for (auto &x : want_vals)
                        if (!read_u32(f, x))
                                return 2;
                const std::vector<uint32_t> &c = cols[col];
                std::vector<uint64_t> one, runs;
                for (size_t j = 0; j < ids.size(); ++j)
                        order_rows::offer(one, c.data(), c.size(), k, desc != 0, &ids[j], 1);
                for (size_t at = 0, step = 1; at < ids.size(); at += step, step = step * 3 + 1) // runs of 1, 4, 13, ... documents
                        order_rows::offer(runs, c.data(), c.size(), k, desc != 0, ids.data() + at, std::min<size_t>(step, ids.size() - at));
                if (one != runs || one != order_rows::first_k(ids.data(), ids.size(), c.data(), c.size(), k, desc != 0) || !same(one, k, desc != 0, want_ids, want_vals)) {
                        fprintf(stderr, "case %u (column %u, k %u, descending %u, %zu documents): rows differ\n", i, col, k, desc, ids.size());
                        ++bad;
                }
        }
        if (!read_u32(f, nblends))
                return 2;
        for (uint32_t i = 0; i < nblends; ++i) {
                uint32_t k = 0, desc = 0, nparts = 0;
                if (!read_u32(f, k) || !read_u32(f, desc) || !read_u32(f, nparts))
                        return 2;
                std::vector<std::vector<uint64_t>> parts;
                for (uint32_t p = 0; p < nparts; ++p) {
                        uint32_t col = 0;
                        std::vector<uint32_t> ids;
                        if (!read_u32(f, col) || col >= ncols || !read_vec(f, ids))
                                return 2;
                        parts.push_back(order_rows::first_k(ids.data(), ids.size(), cols[col].data(), cols[col].size(), k, desc != 0));
                }
                std::vector<uint32_t> want_ids, want_vals;
                if (!read_vec(f, want_ids))
                        return 2;
                want_vals.resize(want_ids.size());
                for (auto &x : want_vals)
                        if (!read_u32(f, x))
                                return 2;
                if (!same(order_rows::blend(parts, k), k, desc != 0, want_ids, want_vals)) {
                        fprintf(stderr, "blend %u (k %u, descending %u, %u parts): rows differ\n", i, k, desc, nparts);
                        ++bad;
                }
        }
        fclose(f);
        // ---- edges
        const uint32_t vals[4] = {9, 5, 0xffffffffu, 5};
        const uint32_t ids[5] = {3, 1, 2, 4, 0xfffffffeu}; // (4 and 0xfffffffe: past the column — 0xffffffff, never read)
        const auto up = order_rows::first_k(ids, 5, vals, 4, 3, false), down = order_rows::first_k(ids, 5, vals, 4, 3, true);
        if (!same(up, 3, false, {1, 3, 2}, {5, 5, 0xffffffffu}) || !same(down, 3, true, {2, 4, 0xfffffffeu}, {0xffffffffu, 0xffffffffu, 0xffffffffu})) {
                fprintf(stderr, "edges: first_k is wrong\n");
                ++bad;
        }
        if (!order_rows::first_k(ids, 5, vals, 4, 0, false).empty() || !order_rows::first_k(ids, 0, vals, 4, 3, false).empty() || !order_rows::first_k(nullptr, 0, vals, 4, 3, true).empty()) {
                fprintf(stderr, "edges: k = 0 or an empty run lists something\n");
                ++bad;
        }
        const auto both = order_rows::blend({up, up, {}}, 4); // equal keys of two parts: both stay, the older part's first
        if (both.size() != 4 || both[0] != up[0] || both[1] != up[0] || both[2] != up[1] || both[3] != up[1] || !order_rows::blend({}, 4).empty()) {
                fprintf(stderr, "edges: blend is wrong\n");
                ++bad;
        }
        printf("cases %u blends %u bad %d\n", ncases, nblends, bad);
        return bad ? 1 : 0;
}

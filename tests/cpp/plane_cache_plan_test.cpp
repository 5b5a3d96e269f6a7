// plane_cache_plan_test.cpp — the plane cache's bookkeeping (trinity_amd/csrc/plane_cache.hpp: plan_plane_growth, plane_row_tables, PlaneRows) on the CPU.
// Stand-alone (tests/test_plane_cache_plan_cpu.py builds it with AddressSanitizer and UndefinedBehaviorSanitizer, runs it and compares the lines it prints with
// values written out by hand): how each (state, request) pair grows the cache, the row tables of a four-term index, and a sequence over one PlaneRows — rows
// built, a high region added, a growth, a phrase batch — that prints which parts every row has and what each run is asked to build.
#include "../../trinity_amd/csrc/plane_cache.hpp"

#include <cstdio>
#include <string>

static void growth(const uint32_t cap, const bool rows, const bool high, const uint32_t plane_rows, const bool needs_high) {
        const PlaneGrowth g = plan_plane_growth(cap, rows, high, plane_rows, needs_high);
        std::printf("(%u, %d, %d) <- (%u, %d): ", cap, rows, high, plane_rows, needs_high);
        if (g.nothing())
                std::printf("nothing\n");
        else
                std::printf("resize %d new_high %d copy_rows %d copy_high %d cap %u outgrown %zu\n", g.resize, g.new_high, g.copy_rows, g.copy_high, g.cap, g.n_outgrown);
}

static std::string parts(const PlaneRows &r) {
        std::string s;
        for (const uint8_t b : r.built)
                s += " " + std::to_string(b);
        return s;
}
static std::string list(const std::vector<uint32_t> &v) {
        std::string s;
        for (const uint32_t x : v)
                s += " " + std::to_string(x);
        return s;
}

int main() {
        growth(0, false, false, 0, false);
        growth(0, false, false, 3, true);
        growth(3, true, false, 2, false);
        growth(3, true, false, 2, true);
        growth(3, true, false, 5, false);
        growth(3, true, true, 5, false);
        growth(5, true, true, 3, true);

        // four terms: df ranks 2, 0, 5, 1 — rank 3 has no term, rank 5 lies past the capacity
        HostIndex ix;
        ix.df_rank = {2, 0, 5, 1};
        ix.docbytes = {70, 90, 40, 80};
        for (const uint32_t documents : {7u, 9u, 4u, 8u}) {
                DevTerm t{};
                t.documents = documents;
                t.nblocks = documents; // (told apart per term: max_blocks below)
                t.flags = TERM_FULL_BLOCKS;
                ix.terms.push_back(t);
        }
        const PlaneRowTables t4 = plane_row_tables(ix, 4);
        std::printf("rank_term:");
        for (const uint32_t t : t4.rank_term)
                t == ROW_NO_TERM ? std::printf(" none") : std::printf(" %u", t);
        std::printf("\nhs_off:");
        for (const uint64_t o : t4.hs_off)
                std::printf(" %llu", (unsigned long long)o);
        std::printf("\n");

        // one cache through its life: capacity 3 without a high region; rows 2 and 0 built (plane 0); a high region added; grown to 5; phrases
        PlaneRows r;
        PlaneGrowth g = r.plan(3, false);
        r.adopt(g, plane_row_tables(ix, g.cap));
        const uint32_t terms[] = {0, 1, 2}; // (term 2: rank 5, no row)
        uint64_t bytes = 0;
        std::vector<uint32_t> build = r.missing_rows(ix, terms, 3, false, false, bytes);
        std::printf("cap %u high %d build%s bytes %llu\n", r.cap, r.high, list(build).c_str(), (unsigned long long)bytes);
        r.mark_built(build, PlaneRows::parts_read(false));
        std::printf("built%s\n", parts(r).c_str());
        build = r.missing_rows(ix, terms, 3, false, false, bytes);
        std::printf("again: build%s bytes %llu\n", list(build).c_str(), (unsigned long long)bytes);
        build = r.missing_rows(ix, terms, 3, false, true, bytes);
        std::printf("rebuild: build%s bytes %llu\n", list(build).c_str(), (unsigned long long)bytes);
        g = r.plan(2, true);
        r.adopt(g, PlaneRowTables{});
        std::printf("high added: cap %u high %d built%s hs_off.size %zu\n", r.cap, r.high, parts(r).c_str(), r.tab.hs_off.size());
        const uint32_t one[] = {1};
        build = r.missing_rows(ix, one, 1, true, false, bytes);
        std::printf("scored: build%s bytes %llu\n", list(build).c_str(), (unsigned long long)bytes);
        r.mark_built(build, PlaneRows::parts_read(true));
        g = r.plan(5, false);
        r.adopt(g, plane_row_tables(ix, g.cap));
        std::printf("grown: cap %u high %d built%s hs_off.size %zu\n", r.cap, r.high, parts(r).c_str(), r.tab.hs_off.size());
        const uint32_t pterms[] = {3, 0, 3, 2}; // (term 3 twice: taken once; term 2: no row)
        PhraseRows pr = r.take_phrase_rows(ix, pterms, 4);
        std::printf("phrases: pairs%s max_blocks %u first %zu pairs_n %zu built%s\n", list(pr.pairs).c_str(), pr.max_blocks, pr.first, r.pairs_n, parts(r).c_str());
        const uint32_t pterms2[] = {1, 3, 2};
        ix.df_rank[2] = 4; // (term 2 moves to rank 4: a row now)
        pr = r.take_phrase_rows(ix, pterms2, 3);
        std::printf("phrases: pairs%s max_blocks %u first %zu pairs_n %zu built%s\n", list(pr.pairs).c_str(), pr.max_blocks, pr.first, r.pairs_n, parts(r).c_str());
        std::printf("ok\n");
        return 0;
}

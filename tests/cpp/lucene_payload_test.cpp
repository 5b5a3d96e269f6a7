// lucene_payload_test.cpp — hit payloads of the Lucene-shaped codec through the host-only layers, as a stand-alone program for the sanitizers
// (g++ -fsanitize=address,undefined; tests/test_lucene_payload_cases.py builds and runs it): the sequential host encoder (csrc/host/lucene_encoder.hpp), the device
// encoder's units in plain loops (csrc/lucene_enc_units.hpp) and the upload walk (csrc/index_host.hpp), over case files the Python side writes from
// tests/lucene_payload_cases.py.  Every output buffer is a heap block of EXACTLY the expected size, every input a heap block of exactly its own: a unit that writes
// or reads a byte too far ends the run.
//
// A case file: u32 magic, u32 refuse, then nine arrays, each u64 count + data: docs u32, freqs u32, positions u16, payload lengths u8, payloads u64, term_first u64,
// the expected index u8, the expected hits.data u8, the expected term table u32[3 n].  refuse == 1: only the bytes and the table count — the upload walk must refuse them.
#include "../../trinity_amd/csrc/host/plan_host.cpp"

#include <cstdio>
#include <memory>

namespace {
template <class T>
struct Arr {
        std::unique_ptr<T[]> p;
        uint64_t n = 0;
        bool read(FILE *f) {
                if (fread(&n, 8, 1, f) != 1)
                        return false;
                p.reset(new T[n]);
                return !n || fread(p.get(), sizeof(T), n, f) == n;
        }
};

int fail_case(const char *path, const char *what) {
        fprintf(stderr, "%s: %s\n", path, what);
        return 1;
}

int run(const char *path) {
        FILE *f = fopen(path, "rb");
        if (!f)
                return fail_case(path, "cannot open");
        uint32_t head[2];
        Arr<uint32_t> docs, freqs, table;
        Arr<uint16_t> pos;
        Arr<uint8_t> plens, index, hits;
        Arr<uint64_t> payloads, term_first;
        const bool ok = fread(head, 4, 2, f) == 2 && head[0] == 0x5041594Cu && docs.read(f) && freqs.read(f) && pos.read(f) && plens.read(f) && payloads.read(f) && term_first.read(f) &&
                        index.read(f) && hits.read(f) && table.read(f);
        fclose(f);
        if (!ok)
                return fail_case(path, "not a case file");
        const uint64_t nterms = table.n / 3;
        char err[600] = "";
        if (head[1]) {
                void *h = tri_host_index_build(index.p.get(), index.n, hits.p.get(), hits.n, TRI_CODEC_LUCENE, table.p.get(), nterms, 1u << 20, err, sizeof err);
                if (h) {
                        tri_host_index_free(h);
                        return fail_case(path, "the upload walk accepted a damaged segment");
                }
                return err[0] ? 0 : fail_case(path, "a refusal without a message");
        }
        if (term_first.n != nterms + 1)
                return fail_case(path, "term_first and the term table disagree");
        for (int units = 0; units < 2; ++units) {
                Arr<uint8_t> io, ho;
                Arr<uint32_t> tt;
                io.p.reset(new uint8_t[index.n]), ho.p.reset(new uint8_t[hits.n]), tt.p.reset(new uint32_t[3 * nterms]);
                uint64_t ilen = 0, hlen = 0;
                const auto fn = units ? tri_host_lucene_encode_units_payloads : tri_host_lucene_encode_payloads;
                if (fn(docs.p.get(), freqs.p.get(), pos.p.get(), plens.p.get(), payloads.p.get(), term_first.p.get(), nterms, io.p.get(), index.n, &ilen, ho.p.get(), hits.n, &hlen, tt.p.get()))
                        return fail_case(path, units ? "the units need more room than the expected bytes" : "the host encoder needs more room than the expected bytes");
                if (ilen != index.n || hlen != hits.n || memcmp(io.p.get(), index.p.get(), ilen) || memcmp(ho.p.get(), hits.p.get(), hlen) || memcmp(tt.p.get(), table.p.get(), 12 * nterms))
                        return fail_case(path, units ? "the units' bytes differ" : "the host encoder's bytes differ");
        }
        void *h = tri_host_index_build(index.p.get(), index.n, hits.p.get(), hits.n, TRI_CODEC_LUCENE, table.p.get(), nterms, 1u << 20, err, sizeof err);
        if (!h)
                return fail_case(path, err);
        uint64_t h0 = 0;
        for (uint64_t t = 0; t < nterms; ++t) { // the directory's offsets lie inside hits.data; a term is flagged exactly when one of its lengths is not zero
                uint64_t h1 = h0;
                for (uint64_t p = term_first.p[t]; p < term_first.p[t + 1]; ++p)
                        h1 += freqs.p[p];
                bool carries = false;
                for (uint64_t k = h0; k < h1; ++k)
                        carries |= plens.p[k] != 0;
                const uint32_t n = tri_host_index_payload_dir(h, (uint32_t)t, nullptr, 0);
                if ((n != 0) != carries || (n && n != 3 * ((h1 - h0) / 128) + 1)) {
                        tri_host_index_free(h);
                        return fail_case(path, "the payload directory's rows do not follow the terms' payloads");
                }
                Arr<uint32_t> row;
                row.p.reset(new uint32_t[n]);
                tri_host_index_payload_dir(h, (uint32_t)t, row.p.get(), n);
                for (uint32_t i = 0; i < n; ++i)
                        if (i % 3 != 2 && row.p[i] > hits.n) {
                                tri_host_index_free(h);
                                return fail_case(path, "a directory offset outside hits.data");
                        }
                h0 = h1;
        }
        tri_host_index_free(h);
        return 0;
}
} // namespace

int main(int argc, char **argv) {
        int bad = 0;
        for (int i = 1; i < argc; ++i)
                bad += run(argv[i]);
        printf("%d cases, %d failed\n", argc - 1, bad);
        return bad ? 1 : 0;
}

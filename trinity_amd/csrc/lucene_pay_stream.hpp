// lucene_pay_stream.hpp — the payloads of a Lucene-shaped term's hits, addressed by hit ordinal (the sibling of HitStream<CODEC_LUCENE>, k_phrase.hpp)
// Part of libtrinity_hip.so (MI355X / gfx950); included by k_rich.hpp and k_decode_hits.hpp.  New code, no reference source.
#pragma once
#include "k_phrase.hpp"

// hits.data keeps a term's payloads next to its positions (lucene_codec.cpp:240-304, 342-366): a full block of 128 hits is ints(position deltas) ints(payload
// lengths) varbyte(payload bytes) and the bytes in hit order; the tail is per hit varbyte(delta << 1 | flag) [u8 length] — the length state starts at 0 with
// the tail and runs across documents — and then the tail's payload bytes.  The reader (materialize_hits, :767-856) sets payload = 0 and copies `length` bytes
// for EVERY hit: (length, word) of a hit depend on its ordinal alone, unlike the Google codec's word, which carries its high bytes through a document.
//
// The upload (index_host.hpp) leaves, for every term flagged TERM_HIT_PAYLOADS, a row in pdir[]: per full block {offset of the length group, offset of the
// payload bytes, the payload bytes before quarters 1 | 2 << 10 | 3 << 20}, then where the tail's payload bytes start.  The device's copy is ONE array:
// pdir[term] = the term's row in that same array (~0: none).  From ordinal h the stream stands after at most 31 values of the length group (a quarter of a
// PFOR128 group is addressable: `width` words from word 1 + quarter * width) or after at most 127 hits of the tail — never after a walk from the term's start.
// The upload has checked every length (<= 8), every block's byte count against its lengths and the tail's end against the chunk's, so the 8-byte load at a
// payload's offset reaches at most 7 bytes past the chunk: inside the 256 bytes of slack behind d_hits.
typedef uint64_t lp_u64_a1 __attribute__((aligned(1)));
__device__ __forceinline__ uint64_t lpay_word(const uint8_t *__restrict__ hits, const uint32_t at, const uint32_t len) {
        if (!len)
                return 0;
        const uint64_t w = *(const lp_u64_a1 *)(hits + at);
        return len >= 8 ? w : w & ((1ull << (8 * len)) - 1ull);
}

struct LPayStream {
        const uint8_t *hits;
        const uint32_t *hd, *pd;
        uint32_t nfull, h, at, tlen;
        LValStream lv;
        VbStream vb;
        bool tail;
        __device__ __forceinline__ void seek() {
                const uint32_t hb = h >> 7;
                if (hb < nfull) {
                        tail = false;
                        const uint32_t q = (h & 127u) >> 5, before = pd[3 * hb + 2];
                        lv.init_group(hits, pd[3 * hb], q);
                        at = pd[3 * hb + 1] + (q ? (before >> (10 * (q - 1))) & 1023u : 0u);
                        for (uint32_t k = 0; k < (h & 31u); ++k)
                                at += lv.next();
                } else {
                        tail = true;
                        tlen = 0;
                        vb.init(hits + hd[1 + nfull]);
                        at = pd[3 * nfull];
                        for (uint32_t k = nfull * 128u; k < h; ++k) {
                                if (vb.next() & 1u)
                                        tlen = vb.byte();
                                at += tlen;
                        }
                }
        }
        // hdir_row: DevTerm::pad; pdir_row: pdir[term] (the caller has seen TERM_HIT_PAYLOADS); ordinal: the hit's within the term
        __device__ __forceinline__ void init(const uint8_t *__restrict__ hits_, const uint32_t *__restrict__ hdir, const uint32_t hdir_row, const uint32_t *__restrict__ pdir,
                                             const uint32_t pdir_row, const uint32_t ordinal) {
                hits = hits_;
                hd = hdir + hdir_row;
                pd = pdir + pdir_row;
                nfull = hd[0];
                h = ordinal;
                seek();
        }
        __device__ __forceinline__ uint64_t next(uint32_t &len) {
                if (tail) {
                        if (vb.next() & 1u)
                                tlen = vb.byte();
                        len = tlen;
                } else
                        len = lv.next();
                const uint64_t w = lpay_word(hits, at, len);
                at += len;
                if (!tail) {
                        ++h;
                        if (!(h & 31u))
                                seek();
                }
                return w;
        }
};

// n hits' (length, word) from `ordinal` on, one lane.  A function of its own, not inlined: the stream's state (a PFOR128 quarter, a varbyte window) then costs
// the kernels that call it — k_rich's WRITE pass, k_hits_at_write, k_merge_hits_lucene — registers only while it runs, and a payload-less term's path none
__device__ __noinline__ void lpay_fill(const uint8_t *__restrict__ hits, const uint32_t *__restrict__ hdir, const uint32_t hdir_row, const uint32_t *__restrict__ pdir,
                                       const uint32_t pdir_row, const uint32_t ordinal, const uint32_t n, uint8_t *__restrict__ plen_out, uint64_t *__restrict__ payload_out) {
        LPayStream ps;
        ps.init(hits, hdir, hdir_row, pdir, pdir_row, ordinal);
        for (uint32_t h = 0; h < n; ++h) {
                uint32_t len;
                const uint64_t w = ps.next(len);
                plen_out[h] = (uint8_t)len;
                payload_out[h] = w;
        }
}

// ---- whole lists (tri_decode_hits): a Lucene list's output order IS the term's hit ordinal order, so the payload fill runs over hit blocks, not documents.
// A wave takes one unit of a job's term: a full block of 128 hits — two hits a lane — or the tail.  The lanes put the length group's packed values into LDS, the
// exceptions' high parts are OR-ed in a lane per exception; the tail's lengths are parsed by one lane (<= 127 varbytes).  One wave prefix sum (wave_prims.hpp:
// every lane active — the scan stands outside every branch) turns the lane's two lengths into byte offsets; each lane loads its bytes and stores
// (length, zero-extended word).  Plain vector stores.
struct LPayJob {
        uint32_t term;
        uint32_t nhits;   // the term's hits
        uint64_t hit_off; // the term's first hit in the outputs
};
__global__ __launch_bounds__(256) void k_decode_hit_payloads(const uint8_t *__restrict__ hits, const uint32_t *__restrict__ hdir, const uint32_t *__restrict__ pdir,
                                                             const DevTerm *__restrict__ terms, const LPayJob *__restrict__ jobs, const uint32_t njobs,
                                                             uint8_t *__restrict__ plen_out, uint64_t *__restrict__ payload_out) {
        __shared__ uint32_t lens[4][128];
        const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
        for (uint32_t ji = blockIdx.y; ji < njobs; ji += gridDim.y) {
                const LPayJob job = jobs[ji];
                const DevTerm t = terms[job.term];
                const uint32_t *hd = hdir + t.pad, *pd = pdir + pdir[job.term];
                const uint32_t nfull = hd[0], ntail = job.nhits - 128u * nfull, nunits = nfull + (ntail ? 1u : 0u);
                for (uint32_t base = blockIdx.x * 4; base < nunits; base += gridDim.x * 4) { // (the same trips for every wave: barriers inside)
                        const uint32_t unit = base + wave;
                        const bool full = unit < nfull, is_tail = unit == nfull && unit < nunits;
                        // ---- the lengths of the unit's hits, in LDS
                        uint32_t width = 0, nexc = 0, eb = 0, bytes_at = 0, v0 = 0, v1 = 0;
                        const uint8_t *g = hits;
                        if (full) {
                                g = hits + pd[3 * unit];
                                bytes_at = pd[3 * unit + 1];
                                const uint32_t L = g[0];
                                if (!L) {
                                        uint32_t n;
                                        v0 = v1 = vb_decode((uint64_t)ld32u(g + 1) | ((uint64_t)ld32u(g + 5) << 32), n);
                                } else {
                                        const uint32_t w0 = ld32u(g + 1);
                                        width = w0 & 0xffu, nexc = (w0 >> 8) & 0xffu, eb = (w0 >> 16) & 0xffu;
                                        if (width) {
                                                const uint32_t mask = width >= 32 ? 0xffffffffu : ((1u << width) - 1u);
                                                for (uint32_t k = 0; k < 2; ++k) {
                                                        const uint32_t i = 2 * lane + k, bit = (i & 31u) * width;
                                                        const uint8_t *wp = g + 1 + 4 * (1 + (i >> 5) * width) + 4 * (bit >> 5);
                                                        const uint64_t win = (uint64_t)ld32u(wp) | ((uint64_t)ld32u(wp + 4) << 32);
                                                        (k ? v1 : v0) = (uint32_t)(win >> (bit & 31u)) & mask;
                                                }
                                        }
                                }
                        } else if (is_tail)
                                bytes_at = pd[3 * nfull];
                        lens[wave][2 * lane] = v0;
                        lens[wave][2 * lane + 1] = v1;
                        __syncthreads();
                        if (full) {
                                const uint8_t *epos = g + 1 + 4 * (1 + 4 * width), *ehigh = epos + 4 * ((nexc + 3) / 4);
                                for (uint32_t e = lane; e < nexc; e += 64) {
                                        const uint32_t eo = e * eb;
                                        const uint64_t hw = (uint64_t)ld32u(ehigh + 4 * (eo >> 5)) | ((uint64_t)ld32u(ehigh + 4 * (eo >> 5) + 4) << 32);
                                        const uint32_t high = (uint32_t)(hw >> (eo & 31u)) & (eb >= 32 ? 0xffffffffu : ((1u << eb) - 1u));
                                        if (width < 32)
                                                atomicOr(&lens[wave][epos[e] & 127u], high << width);
                                }
                        } else if (is_tail && lane == 0) {
                                VbStream vb;
                                vb.init(hits + hd[1 + nfull]);
                                uint32_t tlen = 0;
                                for (uint32_t k = 0; k < ntail; ++k) {
                                        if (vb.next() & 1u)
                                                tlen = vb.byte();
                                        lens[wave][k] = tlen;
                                }
                        }
                        __syncthreads();
                        const uint32_t l0 = lens[wave][2 * lane], l1 = lens[wave][2 * lane + 1];
                        uint32_t total;
                        const uint32_t before = wave_excl_scan(l0 + l1, total);
                        const uint32_t count = full ? 128u : is_tail ? ntail : 0u;
                        const uint64_t dst = job.hit_off + 128ull * unit + 2 * lane;
                        if (2 * lane < count) {
                                plen_out[dst] = (uint8_t)l0;
                                payload_out[dst] = lpay_word(hits, bytes_at + before, l0);
                        }
                        if (2 * lane + 1 < count) {
                                plen_out[dst + 1] = (uint8_t)l1;
                                payload_out[dst + 1] = lpay_word(hits, bytes_at + before + l0, l1);
                        }
                        __syncthreads(); // (lens[] is rewritten by the next trip)
                }
        }
}

// k_decode_hits.hpp — the hits of whole postings lists and of (term, document) pairs (codec seam: materialize_hits)
// Part of libtrinity_hip.so (MI355X / gfx950); included by trinity_hip.hip.  New code, no reference source.
#pragma once
#include "lucene_pay_stream.hpp"

// Codecs::PostingsListIterator::materialize_hits (codecs.h:211-246; google_codec.cpp:533-594; lucene_codec.cpp:767-856) for EVERY document of a
// list (tri_decode_hits) or for chosen documents (tri_decode_hits_at).  Per hit: term_hit::pos — the u16 running sum of the position deltas,
// restarting at 0 with every document —, term_hit::payloadLen and term_hit::payload as the reference's walk leaves them (the payload word and
// the current length restart with the document; a new payload overwrites the word's first min(len, 8) bytes; length 0 clears it).  A document
// owns as many hits as its STORED frequency says (u32), not the tokenpos_t wrap of it.
//
// Whole lists, three passes:
//   k_hits_count   hits per directory block.  GOOGLE: the sum of the block's frequencies (a lane per block); k_hits_scan then turns a job's
//                  sums into 64-bit exclusive offsets and its total.  LUCENE: blk_hits[] already holds every row's hit ordinal, so ONE lane
//                  per job adds the last row's frequencies to it for the total
//   k_decode_hits  a wave takes 64 directory blocks at a time.  A lane per block decodes the block's frequencies into an LDS row of prefix
//                  sums (the documents' hit offsets inside the block).  A GOOGLE block whose hits are not all single bytes (payloads, position
//                  deltas >= 64: no BLK_HITS_PLAIN) is walked by that lane there and then — where a hit starts is known only to the parse of
//                  the hits before it.  Every other block is then decoded a lane per DOCUMENT, two blocks per wave step: a BLK_HITS_PLAIN
//                  document's bytes start at the block's first hit + the prefix sum; a LUCENE document's at a hit ordinal, which
//                  HitStream<CODEC_LUCENE> turns into (128-hit group, quarter, slot) — or into a walk of the term's varbyte tail, at most
//                  127 hits long, which is why the tail gets no path of its own.  A document of more than DH_SPLIT hits would leave one lane
//                  looping while 63 wait (the reference fixture holds one of 70 000): the wave takes it together, a contiguous piece per
//                  lane — sum the piece's deltas, scan the sums across the wave, decode the piece again from its start position and store.
//                  That needs the pieces' starts without a parse, so a long document inside a walked GOOGLE block stays with its lane
// Pairs, two passes (a lane per pair): k_hits_at_freq brackets the block through blk_last[], finds the slot with DeltaStream and reads the
// frequency; the host scans the frequencies; k_hits_at_write locates the hits as k_phrase / k_rich do and stores them.
// LUCENE payloads (lucene_pay_stream.hpp): a hit's (length, word) depend on its ordinal alone, so for whole lists they are filled by a kernel of their own over
// the hit blocks of the terms flagged TERM_HIT_PAYLOADS (k_decode_hit_payloads, behind k_decode_hits, which has stored zeros), and for pairs by the lane that
// wrote the pair's positions, through LPayStream.  Terms without payloads, and calls without payload outputs, run what they ran before.
// All stores are plain vector stores; nothing here keeps state on the index.
struct HitsJob {
        uint32_t term;
        uint32_t pad;
        uint64_t blk_off; // the job's first entry in blk_cnt[] (GOOGLE)
        uint64_t hit_off; // the job's first hit in the outputs (k_decode_hits)
};
constexpr uint32_t DH_SPLIT = 128;    // hits of a document above which the wave shares it
constexpr uint32_t DH_ABSENT = 0xffffffffu; // tri_decode_hits_at: the list does not hold the document

__device__ __forceinline__ uint64_t dh_shfl64(const uint64_t v, const uint32_t src) {
        return (uint64_t)__shfl((uint32_t)v, src) | ((uint64_t)__shfl((uint32_t)(v >> 32), src) << 32);
}
__device__ __forceinline__ uint64_t dh_shfl_up64(const uint64_t v, const uint32_t d) {
        return (uint64_t)__shfl_up((uint32_t)v, d) | ((uint64_t)__shfl_up((uint32_t)(v >> 32), d) << 32);
}

// the frequencies of block b, after which (GOOGLE) the block's hits begin
template <int CODEC>
__device__ __forceinline__ void dh_freqs_init(FreqStream<CODEC> &fs, const uint8_t *__restrict__ index, const DevTerm &t, const uint32_t b, const uint32_t off, const uint32_t n) {
        DeltaStream<CODEC> s;
        if constexpr (CODEC == CODEC_GOOGLE) { // the freqs follow the n - 1 deltas in the same byte stream
                s.init(index, t, b, off);
                for (uint32_t i = 0; i + 1 < n; ++i)
                        (void)s.next();
        }
        fs.init(index, t, b, off, s);
}

template <int CODEC>
__global__ __launch_bounds__(256) void k_hits_count(const uint8_t *__restrict__ index, const uint32_t *__restrict__ blk_off, const uint32_t *__restrict__ blk_hits,
                                                    const DevTerm *__restrict__ terms, const HitsJob *__restrict__ jobs, const uint32_t njobs, uint64_t *__restrict__ blk_cnt,
                                                    uint64_t *__restrict__ totals) {
        for (uint32_t ji = blockIdx.y; ji < njobs; ji += gridDim.y) {
                const HitsJob job = jobs[ji];
                const DevTerm t = terms[job.term];
                if constexpr (CODEC == CODEC_LUCENE) { // (launched with one lane per job)
                        if (blockIdx.x == 0 && threadIdx.x == 0 && t.nblocks) {
                                const uint32_t b = t.nblocks - 1, gb = t.first_block + b, off = blk_off[gb];
                                const uint32_t n = TRI_BLOCK_N(t, b, index, off);
                                FreqStream<CODEC> fs;
                                dh_freqs_init<CODEC>(fs, index, t, b, off, n);
                                uint64_t sum = blk_hits[gb];
                                for (uint32_t i = 0; i < n; ++i)
                                        sum += fs.next();
                                totals[ji] = sum;
                        }
                } else {
                        for (uint32_t b = blockIdx.x * 256 + threadIdx.x; b < t.nblocks; b += gridDim.x * 256) {
                                const uint32_t off = blk_off[t.first_block + b];
                                const uint32_t n = TRI_BLOCK_N(t, b, index, off);
                                FreqStream<CODEC> fs;
                                dh_freqs_init<CODEC>(fs, index, t, b, off, n);
                                uint64_t sum = 0;
                                for (uint32_t i = 0; i < n; ++i)
                                        sum += fs.next();
                                blk_cnt[job.blk_off + b] = sum;
                        }
                }
        }
}

// blk_cnt[] of a job: sums -> exclusive 64-bit offsets; totals[job] = their sum.  A workgroup per job, 256 blocks a step
__global__ __launch_bounds__(256) void k_hits_scan(const DevTerm *__restrict__ terms, const HitsJob *__restrict__ jobs, const uint32_t njobs, uint64_t *__restrict__ blk_cnt,
                                                   uint64_t *__restrict__ totals) {
        __shared__ uint64_t wsum[4];
        const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
        for (uint32_t ji = blockIdx.x; ji < njobs; ji += gridDim.x) {
                const HitsJob job = jobs[ji];
                const uint32_t nblocks = terms[job.term].nblocks;
                uint64_t carry = 0;
                for (uint32_t base = 0; base < nblocks; base += 256) {
                        const uint32_t b = base + threadIdx.x;
                        const uint64_t v = b < nblocks ? blk_cnt[job.blk_off + b] : 0;
                        uint64_t x = v;
                        for (uint32_t d = 1; d < 64; d <<= 1) {
                                const uint64_t y = dh_shfl_up64(x, d);
                                if (lane >= d)
                                        x += y;
                        }
                        if (lane == 63)
                                wsum[wave] = x;
                        __syncthreads();
                        uint64_t before = 0, all = 0;
                        for (uint32_t k = 0; k < 4; ++k) {
                                before += k < wave ? wsum[k] : 0;
                                all += wsum[k];
                        }
                        if (b < nblocks)
                                blk_cnt[job.blk_off + b] = carry + before + x - v;
                        carry += all;
                        __syncthreads();
                }
                if (threadIdx.x == 0)
                        totals[ji] = carry;
        }
}

// ---- one document's hits from where they can be ADDRESSED: GOOGLE, a BLK_HITS_PLAIN block: bytes (delta << 1); LUCENE: hit ordinals
template <int CODEC>
struct DhPlainStream;
template <>
struct DhPlainStream<CODEC_GOOGLE> {
        const uint8_t *p;
        __device__ __forceinline__ void init(const HitCtx &c, const uint32_t, const uint32_t loc) { p = c.base + loc; }
        __device__ __forceinline__ uint32_t next() { return (uint32_t)(*p++) >> 1; }
};
template <>
struct DhPlainStream<CODEC_LUCENE> {
        HitStream<CODEC_LUCENE> s;
        __device__ __forceinline__ void init(const HitCtx &c, const uint32_t hdir_off, const uint32_t loc) { s.init(c, hdir_off, loc); }
        __device__ __forceinline__ uint32_t next() { return s.next(); }
};

struct DhOut {
        uint16_t *pos;
        uint8_t *plen;     // both null (positions only) or both given
        uint64_t *payload;
        __device__ __forceinline__ void put_plain(const uint64_t at, const uint32_t p) const {
                pos[at] = (uint16_t)p;
                if (plen) {
                        plen[at] = 0;
                        payload[at] = 0;
                }
        }
};

// f hits from `loc` (GOOGLE: byte offset into index[], LUCENE: hit ordinal of the term) to out[dst ..), one lane
template <int CODEC>
__device__ __forceinline__ void dh_plain_doc(const HitCtx &ctx, const uint32_t hdir_off, const uint32_t loc, const uint32_t f, const uint64_t dst, const DhOut &out) {
        DhPlainStream<CODEC> s;
        s.init(ctx, hdir_off, loc);
        uint32_t pos = 0;
        for (uint32_t h = 0; h < f; ++h) {
                pos = (pos + s.next()) & 0xffffu;
                out.put_plain(dst + h, pos);
        }
}
// ... the whole wave (every lane calls it with the same arguments): lane l takes hits [l * piece, (l + 1) * piece)
template <int CODEC>
__device__ __forceinline__ void dh_plain_doc_wave(const HitCtx &ctx, const uint32_t hdir_off, const uint32_t loc, const uint32_t f, const uint64_t dst, const DhOut &out, const uint32_t lane) {
        const uint32_t piece = (f + 63u) / 64u;
        const uint32_t h0 = min(lane * piece, f), h1 = min(h0 + piece, f);
        uint32_t sum = 0;
        if (h0 < h1) {
                DhPlainStream<CODEC> s;
                s.init(ctx, hdir_off, loc + h0);
                for (uint32_t h = h0; h < h1; ++h)
                        sum += s.next();
        }
        uint32_t x = sum; // the position before the piece = the sums of the lanes below
        for (uint32_t d = 1; d < 64; d <<= 1) {
                const uint32_t y = __shfl_up(x, d);
                if (lane >= d)
                        x += y;
        }
        if (h0 < h1) {
                DhPlainStream<CODEC> s;
                s.init(ctx, hdir_off, loc + h0);
                uint32_t pos = (x - sum) & 0xffffu;
                for (uint32_t h = h0; h < h1; ++h) {
                        pos = (pos + s.next()) & 0xffffu;
                        out.put_plain(dst + h, pos);
                }
        }
}
// f hits of a GOOGLE document parsed from the byte stream (google_codec.cpp:533-594), which is left behind the document
__device__ __forceinline__ void dh_walk_doc(VbStream &hs, const uint32_t f, const uint64_t dst, const DhOut &out) {
        uint32_t pos = 0, plen = 0; // position, payload length and payload word restart with every document
        uint64_t payload = 0;
        for (uint32_t h = 0; h < f; ++h) {
                const uint32_t v = hs.next();
                if (v & 1u)
                        plen = hs.byte();
                if (out.plen) {
                        if (!plen)
                                payload = 0;
                        for (uint32_t k = 0; k < plen; ++k) { // the payload bytes, little end first, over the word's low bytes
                                const uint64_t by = hs.byte();
                                if (k < 8)
                                        payload = (payload & ~(0xffull << (8 * k))) | (by << (8 * k));
                        }
                } else
                        hs.skip(plen);
                pos = (pos + (v >> 1)) & 0xffffu;
                out.pos[dst + h] = (uint16_t)pos;
                if (out.plen) {
                        out.plen[dst + h] = (uint8_t)plen;
                        out.payload[dst + h] = payload;
                }
        }
}
// ... stepped over (Google::Decoder::skip_block_doc, google_codec.cpp:497-531)
__device__ __forceinline__ void dh_skip_doc(VbStream &hs, const uint32_t f) {
        uint32_t plen = 0;
        for (uint32_t h = 0; h < f; ++h) {
                if (hs.next() & 1u)
                        plen = hs.byte();
                hs.skip(plen);
        }
}

// grid.x: chunks of 256 blocks (64 per wave) of job blockIdx.y
template <int CODEC>
__global__ __launch_bounds__(256) void k_decode_hits(const uint8_t *__restrict__ index, const uint8_t *__restrict__ hits, const uint32_t *__restrict__ blk_off,
                                                     const uint32_t *__restrict__ blk_hits, const uint32_t *__restrict__ hdir, const DevTerm *__restrict__ terms,
                                                     const HitsJob *__restrict__ jobs, const uint32_t njobs, const uint64_t *__restrict__ blk_cnt, uint16_t *__restrict__ pos_out,
                                                     uint8_t *__restrict__ plen_out, uint64_t *__restrict__ payload_out) {
        __shared__ uint32_t pre[4][64][33]; // [wave][block of the wave's 64][document]: the hits of the block before the document; [n]: the block's hits
        const HitCtx ctx{CODEC == CODEC_GOOGLE ? index : hits, blk_hits, hdir};
        const DhOut out{pos_out, plen_out, payload_out};
        const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
        for (uint32_t ji = blockIdx.y; ji < njobs; ji += gridDim.y) {
                const HitsJob job = jobs[ji];
                const DevTerm t = terms[job.term];
                for (uint32_t wg_base = blockIdx.x * 256; wg_base < t.nblocks; wg_base += gridDim.x * 256) { // (the same trips for every wave: barriers inside)
                        const uint32_t b = wg_base + wave * 64 + lane;
                        // ---- a lane per block: the documents' hit offsets; walked blocks are decoded here
                        uint32_t n = 0, loc = 0;
                        uint64_t first = 0; // the block's first hit in the job's output
                        bool per_doc = false;
                        if (b < t.nblocks) {
                                const uint32_t gb = t.first_block + b, off = blk_off[gb];
                                n = TRI_BLOCK_N(t, b, index, off);
                                FreqStream<CODEC> fs;
                                dh_freqs_init<CODEC>(fs, index, t, b, off, n);
                                uint32_t acc = 0;
                                for (uint32_t i = 0; i < n; ++i) {
                                        pre[wave][lane][i] = acc;
                                        acc += fs.next();
                                }
                                pre[wave][lane][n] = acc;
                                const uint32_t hits_at = blk_hits[gb];
                                if constexpr (CODEC == CODEC_GOOGLE) {
                                        first = blk_cnt[job.blk_off + b];
                                        loc = off + (hits_at & ~BLK_HITS_PLAIN);
                                        per_doc = (hits_at & BLK_HITS_PLAIN) != 0;
                                        if (!per_doc) { // the hits follow the frequencies: fs stands on the block's first hit
                                                uint64_t dst = job.hit_off + first;
                                                for (uint32_t i = 0; i < n; ++i) {
                                                        const uint32_t f = pre[wave][lane][i + 1] - pre[wave][lane][i];
                                                        dh_walk_doc(fs.s, f, dst, out);
                                                        dst += f;
                                                }
                                        }
                                } else {
                                        first = hits_at;
                                        loc = hits_at;
                                        per_doc = true;
                                }
                        }
                        __syncthreads();
                        // ---- a lane per document, two blocks a step
                        const uint32_t wave_base = wg_base + wave * 64;
                        const uint32_t nb = wave_base < t.nblocks ? min(64u, t.nblocks - wave_base) : 0u;
                        for (uint32_t step = 0; 2 * step < nb; ++step) {
                                const uint32_t bi = 2 * step + (lane >> 5), j = lane & 31u;
                                const uint32_t n_b = __shfl(n, bi), loc_b = __shfl(loc, bi);
                                const uint32_t per_doc_b = __shfl((uint32_t)per_doc, bi);
                                const uint64_t first_b = dh_shfl64(first, bi);
                                uint32_t p0 = 0, f = 0;
                                if (bi < nb && per_doc_b && j < n_b) {
                                        p0 = pre[wave][bi][j];
                                        f = pre[wave][bi][j + 1] - p0;
                                }
                                const uint64_t dst = job.hit_off + first_b + p0;
                                const bool big = f > DH_SPLIT;
                                if (f && !big)
                                        dh_plain_doc<CODEC>(ctx, t.pad, loc_b + p0, f, dst, out);
                                for (uint64_t m = __ballot(big); m; m &= m - 1) {
                                        const uint32_t src = (uint32_t)__builtin_ctzll(m);
                                        dh_plain_doc_wave<CODEC>(ctx, t.pad, __shfl(loc_b + p0, src), __shfl(f, src), dh_shfl64(dst, src), out, lane);
                                }
                        }
                        __syncthreads(); // (pre[] is rewritten by the next trip)
                }
        }
}

// ---- pairs
template <int CODEC>
__global__ __launch_bounds__(256) void k_hits_at_freq(const uint8_t *__restrict__ index, const uint32_t *__restrict__ blk_last, const uint32_t *__restrict__ blk_off,
                                                      const DevTerm *__restrict__ terms, const uint32_t *__restrict__ pair_term, const uint32_t *__restrict__ pair_doc, const uint32_t npairs,
                                                      uint32_t *__restrict__ freqs, uint32_t *__restrict__ at_block, uint32_t *__restrict__ at_slot, uint32_t *__restrict__ at_before) {
        const uint32_t i = blockIdx.x * 256 + threadIdx.x;
        if (i >= npairs)
                return;
        const DevTerm t = terms[pair_term[i]];
        const uint32_t target = pair_doc[i];
        uint32_t freq = DH_ABSENT, slot = DH_ABSENT, before = 0;
        const uint32_t *bl = blk_last + t.first_block;
        const uint32_t b = first_ge(bl, 0u, t.nblocks, target); // the first block whose last document is >= target
        if (b < t.nblocks && target) {
                const uint32_t off = blk_off[t.first_block + b];
                const uint32_t n = TRI_BLOCK_N(t, b, index, off);
                uint32_t doc = b ? bl[b - 1] : 0;
                DeltaStream<CODEC> s;
                s.init(index, t, b, off);
                for (uint32_t k = 0; k + 1 < n; ++k) { // (all of them: GOOGLE's frequencies start behind the last delta)
                        doc += s.next();
                        if (doc == target)
                                slot = k;
                }
                if (bl[b] == target)
                        slot = n - 1;
                if (slot != DH_ABSENT) {
                        FreqStream<CODEC> fs;
                        fs.init(index, t, b, off, s);
                        for (uint32_t k = 0; k < slot; ++k)
                                before += fs.next();
                        freq = fs.next();
                }
        }
        freqs[i] = freq;
        at_block[i] = b;
        at_slot[i] = slot;
        at_before[i] = before;
}

template <int CODEC>
__global__ __launch_bounds__(256) void k_hits_at_write(const uint8_t *__restrict__ index, const uint8_t *__restrict__ hits, const uint32_t *__restrict__ blk_off,
                                                       const uint32_t *__restrict__ blk_hits, const uint32_t *__restrict__ hdir, const uint32_t *__restrict__ pdir,
                                                       const DevTerm *__restrict__ terms,
                                                       const uint32_t *__restrict__ pair_term, const uint32_t npairs, const uint32_t *__restrict__ freqs, const uint32_t *__restrict__ at_block,
                                                       const uint32_t *__restrict__ at_slot, const uint32_t *__restrict__ at_before, const uint64_t *__restrict__ hit_off,
                                                       uint16_t *__restrict__ pos_out, uint8_t *__restrict__ plen_out, uint64_t *__restrict__ payload_out) {
        const uint32_t i = blockIdx.x * 256 + threadIdx.x;
        if (i >= npairs)
                return;
        const uint32_t f = freqs[i];
        if (f == DH_ABSENT || !f)
                return;
        const HitCtx ctx{CODEC == CODEC_GOOGLE ? index : hits, blk_hits, hdir};
        const DhOut out{pos_out, plen_out, payload_out};
        const DevTerm t = terms[pair_term[i]];
        const uint32_t b = at_block[i], slot = at_slot[i], gb = t.first_block + b;
        const uint32_t hits_at = blk_hits[gb];
        const uint64_t dst = hit_off[i];
        if constexpr (CODEC == CODEC_GOOGLE) {
                const uint32_t off = blk_off[gb];
                if (hits_at & BLK_HITS_PLAIN) { // one byte per hit: the document's start follows from the frequencies before it
                        dh_plain_doc<CODEC>(ctx, 0, off + (hits_at & ~BLK_HITS_PLAIN) + at_before[i], f, dst, out);
                        return;
                }
                // the hits of the slots before it are parsed, document by document (the payload length restarts with each)
                const uint32_t n = TRI_BLOCK_N(t, b, index, off);
                FreqStream<CODEC> fs;
                dh_freqs_init<CODEC>(fs, index, t, b, off, n);
                VbStream hs;
                hs.init(index + off + hits_at);
                for (uint32_t k = 0; k < slot; ++k)
                        dh_skip_doc(hs, fs.next());
                dh_walk_doc(hs, f, dst, out);
        } else {
                dh_plain_doc<CODEC>(ctx, t.pad, hits_at + at_before[i], f, dst, out);
                if (out.plen && (t.flags & TERM_HIT_PAYLOADS)) // (over the zeros dh_plain_doc stored: the same lane, in program order)
                        lpay_fill(hits, hdir, t.pad, pdir, pdir[pair_term[i]], hits_at + at_before[i], f, out.plen + dst, out.payload + dst);
        }
}

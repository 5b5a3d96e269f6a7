// write_side.hpp — the write side on the device: the codecs' encoders, SegmentIndexSession::commit and the codecs' merge — tri_encode_google[_payloads],
// tri_encode_lucene[_payloads], tri_commit_google / _lucene[_payloads], tri_merge_google / _lucene.  Host code only: the kernels are k_encode.hpp, k_lencode.hpp (lucene_enc_units.hpp),
// k_commit.hpp and commit_sort.hip.  Part of libtrinity_hip.so (MI355X / gfx950); included by trinity_hip.hip after the kernels.  New code, no reference source.
//
// Every public call creates ONE WriteScratch and passes it down; every device buffer of the call comes from it and goes back to the device handle's pool when
// the call returns, whichever way it returns.  The encoders read an EncIn (device arrays, term after term) and fill an EncOut (the caller's host buffers).
#pragma once

extern "C" int tri_sort_pairs_u64_u32(const unsigned long long *keys_in, unsigned long long *keys_out, const unsigned *vals_in, unsigned *vals_out, size_t n, void *tmp,
                                      size_t *tmp_bytes, hipStream_t stream); // (commit_sort.hip)

namespace {
// the device temporaries of one write-side call: from the device handle's buffer pool (a sizing call and the call that follows it use the same ones), back to
// it when the call returns — after the stream has drained, so that an early error return hands no buffer back that a kernel still works on
struct WriteScratch {
        tri_dev *dev;
        std::vector<Pooled<void>> held;
        uint64_t *scan_sums = nullptr; // (enc_scan's chunk sums, grown on demand)
        uint64_t scan_cap = 0;
        explicit WriteScratch(tri_dev *d) : dev(d) {}
        WriteScratch(const WriteScratch &) = delete;
        WriteScratch &operator=(const WriteScratch &) = delete;
        ~WriteScratch() { // (the drain comes first; `held` releases its buffers behind it)
                if (!held.empty())
                        hipStreamSynchronize(dev->stream);
        }
        template <class T>
        hipError_t get(T *&p, const size_t count) {
                Pooled<void> q;
                const hipError_t e = q.alloc(dev, count ? count * sizeof(T) : 8);
                p = (T *)q.get();
                if (e == hipSuccess)
                        held.push_back(std::move(q));
                return e;
        }
};

// what an encoder reads, on the device: np postings and nhits hits grouped by term as term_first (host) says, validated by the caller
struct EncIn {
        const uint32_t *docs = nullptr, *freqs = nullptr;
        const uint16_t *pos = nullptr;
        const uint8_t *plens = nullptr;     // (nullptr: no hit has a payload)
        const uint64_t *payloads = nullptr;
        uint64_t np = 0, nhits = 0;
};
// where an encoder delivers, on the host: `index` == nullptr is a sizing call (the lengths and the term table only); hits*: the Lucene-shaped codec's hits.data
struct EncOut {
        uint8_t *index;
        size_t index_cap, *index_len;
        uint8_t *hits;
        size_t hits_cap, *hits_len;
        tri_term *terms;
};

// one lane per element
inline dim3 grid_for(const uint64_t n) { return dim3((uint32_t)std::max<uint64_t>(1, (n + 255) / 256)); }
// one workgroup per (participant, term) job, at most 16 per compute unit
inline dim3 job_grid(const tri_dev *dev, const size_t njobs) { return dim3((uint32_t)std::min<size_t>(njobs, (size_t)dev->cus * 16)); }

// exclusive scan of n u32 into u64 over the whole device: chunk sums, chunk bases, chunks (k_encode.hpp)
int enc_scan(WriteScratch &s, const uint32_t *in, uint64_t *outp, const uint64_t n) {
        const hipStream_t stream = s.dev->stream;
        const uint64_t nchunks = (n + ENC_SCAN_CHUNK - 1) / ENC_SCAN_CHUNK;
        if (nchunks <= 1) {
                hipLaunchKernelGGL(k_enc_scan, dim3(1), dim3(1024), 0, stream, in, outp, n);
                return TRI_OK;
        }
        if (nchunks + 1 > s.scan_cap) { // (the smaller one may still be read by an earlier scan: it goes back with everything else)
                HIP_TRY(s.get(s.scan_sums, nchunks + 1));
                s.scan_cap = nchunks + 1;
        }
        hipLaunchKernelGGL(k_enc_scan_sums, dim3((uint32_t)nchunks), dim3(1024), 0, stream, in, s.scan_sums, n);
        hipLaunchKernelGGL(k_enc_scan_bases, dim3(1), dim3(1024), 0, stream, s.scan_sums, nchunks);
        hipLaunchKernelGGL(k_enc_scan_chunks, dim3((uint32_t)nchunks), dim3(1024), 0, stream, in, s.scan_sums, outp, n);
        return TRI_OK;
}

// stable sort of n (key, value) pairs by key (commit_sort.hip)
int sort_pairs(WriteScratch &s, const unsigned long long *keys, unsigned long long *keys_sorted, const uint32_t *vals, uint32_t *perm, const uint64_t n) {
        size_t bytes = 0;
        HIP_TRY((hipError_t)tri_sort_pairs_u64_u32(keys, keys_sorted, vals, perm, n, nullptr, &bytes, s.dev->stream));
        uint8_t *tmp;
        HIP_TRY(s.get(tmp, bytes));
        HIP_TRY((hipError_t)tri_sort_pairs_u64_u32(keys, keys_sorted, vals, perm, n, tmp, &bytes, s.dev->stream));
        return TRI_OK;
}

// ---- Codecs::Google::Encoder (google_codec.cpp:9-176) on the device: the segment's `index` bytes and term table, byte for byte what the reference's encoder
//      writes for the same begin_term / begin_document / new_hit / end_document / end_term calls.  See k_encode.hpp.
int encode_google_device(WriteScratch &s, const EncIn &in, const uint64_t *term_first, const size_t nterms, const EncOut &out) {
        const hipStream_t stream = s.dev->stream;
        // ---- host: the block structure (which block belongs to which term)
        std::vector<uint32_t> blk_first(nterms + 1, 0), blk_term;
        for (size_t t = 0; t < nterms; ++t) {
                const uint64_t nb = (term_first[t + 1] - term_first[t] + 31) / 32;
                if ((uint64_t)blk_first[t] + nb > 0xfffffff0ull)
                        return fail(TRI_ERR_UNSUPPORTED, "more than 2^32 blocks");
                blk_first[t + 1] = blk_first[t] + (uint32_t)nb;
                blk_term.insert(blk_term.end(), (size_t)nb, (uint32_t)t);
        }
        const uint32_t nblocks = blk_first[nterms];
        std::vector<uint64_t> term_off(nterms + 1, 0);
        std::vector<uint64_t> blk_off(nblocks + 1, 0);
        uint32_t *d_blk_first, *d_blk_term, *d_sizes, *d_tails = nullptr;
        uint64_t *d_hit_off, *d_term_first, *d_blk_off = nullptr, *d_term_off;
        EncArgs a{};
        if (nblocks) {
                HIP_TRY(s.get(d_hit_off, in.np + 1));
                HIP_TRY(s.get(d_term_first, nterms + 1));
                HIP_TRY(s.get(d_blk_first, nterms + 1));
                HIP_TRY(s.get(d_blk_term, nblocks));
                HIP_TRY(s.get(d_sizes, nblocks));
                HIP_TRY(s.get(d_tails, nblocks));
                HIP_TRY(s.get(d_blk_off, (size_t)nblocks + 1));
                HIP_TRY(hipMemcpyAsync(d_term_first, term_first, (nterms + 1) * 8, hipMemcpyHostToDevice, stream));
                HIP_TRY(hipMemcpyAsync(d_blk_first, blk_first.data(), (nterms + 1) * 4, hipMemcpyHostToDevice, stream));
                HIP_TRY(hipMemcpyAsync(d_blk_term, blk_term.data(), (size_t)nblocks * 4, hipMemcpyHostToDevice, stream));
                // hits before every posting, then the blocks' sizes and their running sum
                int rcs;
                if ((rcs = enc_scan(s, in.freqs, d_hit_off, in.np)))
                        return rcs;
                a = EncArgs{in.docs, in.freqs, in.pos, in.plens, in.payloads, d_hit_off, d_term_first, d_blk_first, d_blk_term, nblocks};
                hipLaunchKernelGGL(k_enc_size, grid_for(nblocks), dim3(256), 0, stream, a, d_sizes, d_tails);
                if ((rcs = enc_scan(s, d_sizes, d_blk_off, (uint64_t)nblocks)))
                        return rcs;
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipMemcpyAsync(blk_off.data(), d_blk_off, ((size_t)nblocks + 1) * 8, hipMemcpyDeviceToHost, stream));
                HIP_TRY(hipStreamSynchronize(stream));
        }
        // ---- host: where every term's chunk starts (2 bytes + its blocks + its skiplist entries)
        for (size_t t = 0; t < nterms; ++t) {
                const uint32_t g0 = blk_first[t], g1 = blk_first[t + 1];
                uint64_t entries = 0;
                if (g1 > g0) {
                        const uint32_t first_marked = (g0 + 8) / 8 * 8 - 1;
                        if (g1 - 1 >= first_marked)
                                entries = std::min<uint64_t>(65535, (g1 - 1 - first_marked) / 8 + 1);
                }
                const uint64_t size = 2 + (blk_off[g1] - blk_off[g0]) + 8 * entries;
                if (term_off[t] + size > 0xffffffffull)
                        return fail(TRI_ERR_UNSUPPORTED, "the index would exceed 4 GiB (term_index_ctx offsets are 32 bits)");
                out.terms[t] = {(uint32_t)(term_first[t + 1] - term_first[t]), (uint32_t)term_off[t], (uint32_t)size};
                term_off[t + 1] = term_off[t] + size;
        }
        *out.index_len = (size_t)term_off[nterms];
        if (!out.index)
                return TRI_OK; // (sizing call)
        if (out.index_cap < *out.index_len)
                return fail(TRI_ERR_INVALID, "tri_encode_google: the index needs %zu bytes, %zu given", *out.index_len, out.index_cap);
        if (!*out.index_len)
                return TRI_OK;
        uint8_t *d_out;
        HIP_TRY(s.get(d_out, *out.index_len));
        HIP_TRY(hipMemsetAsync(d_out, 0, *out.index_len, stream)); // (a term without documents is two zero bytes)
        if (nblocks) {
                HIP_TRY(s.get(d_term_off, nterms + 1));
                HIP_TRY(hipMemcpyAsync(d_term_off, term_off.data(), (nterms + 1) * 8, hipMemcpyHostToDevice, stream));
                hipLaunchKernelGGL(k_enc_write, grid_for(nblocks), dim3(256), 0, stream, a, d_blk_off, d_tails, d_term_off, d_out);
                HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(out.index, d_out, *out.index_len, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return TRI_OK;
}

// ---- Codecs::Lucene::Encoder (lucene_codec.cpp:163-388) on the device, PFOR128 payload (k_lencode.hpp, lucene_enc_units.hpp)
int encode_lucene_device(WriteScratch &s, const EncIn &in, const uint64_t *term_first, const size_t nterms, const EncOut &out) {
        const hipStream_t stream = s.dev->stream;
        const uint64_t np = in.np;
        uint32_t *d_hdelta, *d_dcnt, *d_hcnt, *d_dsize, *d_hsize, *d_tail_d, *d_tail_h, *d_isize, *d_hsz;
        uint64_t *d_hit_off, *d_term_first, *d_dblk_first, *d_hblk_first, *d_doff, *d_hoff, *d_term_off, *d_hterm_off;
        HIP_TRY(s.get(d_hdelta, in.nhits + 1));
        HIP_TRY(s.get(d_hit_off, np + 2));
        HIP_TRY(s.get(d_term_first, nterms + 1));
        HIP_TRY(s.get(d_dcnt, nterms + 1));
        HIP_TRY(s.get(d_hcnt, nterms + 1));
        HIP_TRY(s.get(d_dblk_first, nterms + 2));
        HIP_TRY(s.get(d_hblk_first, nterms + 2));
        HIP_TRY(s.get(d_tail_d, nterms + 1));
        HIP_TRY(s.get(d_tail_h, nterms + 1));
        HIP_TRY(s.get(d_isize, nterms + 1));
        HIP_TRY(s.get(d_hsz, nterms + 1));
        HIP_TRY(s.get(d_term_off, nterms + 2));
        HIP_TRY(s.get(d_hterm_off, nterms + 2));
        HIP_TRY(hipMemcpyAsync(d_term_first, term_first, (nterms + 1) * 8, hipMemcpyHostToDevice, stream));
        int rcs;
        if ((rcs = enc_scan(s, in.freqs, d_hit_off, np)))
                return rcs;
        const dim3 block(256);
        LencArgs a{in.docs, in.freqs, in.pos, d_hit_off, d_term_first, d_hdelta, d_dblk_first, d_hblk_first, (uint64_t)nterms, in.plens, in.payloads};
        hipLaunchKernelGGL(k_lenc_hdelta, grid_for(np), block, 0, stream, a, d_hdelta, np);
        hipLaunchKernelGGL(k_lenc_term_counts, grid_for(nterms), block, 0, stream, d_term_first, d_hit_off, (uint64_t)nterms, d_dcnt, d_hcnt);
        if ((rcs = enc_scan(s, d_dcnt, d_dblk_first, nterms)) || (rcs = enc_scan(s, d_hcnt, d_hblk_first, nterms)))
                return rcs;
        uint64_t nd = 0, nh = 0;
        HIP_TRY(hipMemcpyAsync(&nd, d_dblk_first + nterms, 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(&nh, d_hblk_first + nterms, 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(s.get(d_dsize, nd + 1));
        HIP_TRY(s.get(d_hsize, nh + 1));
        HIP_TRY(s.get(d_doff, nd + 2));
        HIP_TRY(s.get(d_hoff, nh + 2));
        hipLaunchKernelGGL(k_lenc_dblk_size, grid_for(nd), block, 0, stream, a, nd, d_dsize);
        hipLaunchKernelGGL(k_lenc_hblk_size, grid_for(nh), block, 0, stream, a, nh, d_hsize);
        hipLaunchKernelGGL(k_lenc_tail_size, grid_for(nterms), block, 0, stream, a, d_tail_d, d_tail_h);
        if ((rcs = enc_scan(s, d_dsize, d_doff, nd)) || (rcs = enc_scan(s, d_hsize, d_hoff, nh)))
                return rcs;
        LencPlace pl{d_doff, d_hoff, d_term_off, d_hterm_off, d_tail_d, d_tail_h};
        hipLaunchKernelGGL(k_lenc_term_sizes, grid_for(nterms), block, 0, stream, a, pl, d_isize, d_hsz);
        if ((rcs = enc_scan(s, d_isize, d_term_off, nterms)) || (rcs = enc_scan(s, d_hsz, d_hterm_off, nterms)))
                return rcs;
        HIP_TRY(hipGetLastError());
        std::vector<uint64_t> term_off(nterms + 1), hterm_off(nterms + 1);
        HIP_TRY(hipMemcpyAsync(term_off.data(), d_term_off, (nterms + 1) * 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(hterm_off.data(), d_hterm_off, (nterms + 1) * 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (term_off[nterms] > 0xffffffffull || hterm_off[nterms] > 0xffffffffull)
                return fail(TRI_ERR_UNSUPPORTED, "the index or hits.data would exceed 4 GiB (term_index_ctx offsets and the term header's hits offset are 32 bits)");
        for (size_t t = 0; t < nterms; ++t)
                out.terms[t] = {(uint32_t)(term_first[t + 1] - term_first[t]), (uint32_t)term_off[t], (uint32_t)(term_off[t + 1] - term_off[t])};
        *out.index_len = (size_t)term_off[nterms];
        *out.hits_len = (size_t)hterm_off[nterms];
        if (!out.index)
                return TRI_OK; // (sizing call)
        if (out.index_cap < *out.index_len || out.hits_cap < *out.hits_len || (*out.hits_len && !out.hits))
                return fail(TRI_ERR_INVALID, "tri_encode_lucene: the index needs %zu bytes (%zu given), hits.data %zu (%zu given)", *out.index_len, out.index_cap, *out.hits_len,
                            out.hits_cap);
        uint8_t *d_index, *d_hits;
        HIP_TRY(s.get(d_index, *out.index_len + 8));
        HIP_TRY(s.get(d_hits, *out.hits_len + 8));
        hipLaunchKernelGGL(k_lenc_dblk_write, grid_for(nd), block, 0, stream, a, pl, nd, d_index);
        hipLaunchKernelGGL(k_lenc_hblk_write, grid_for(nh), block, 0, stream, a, pl, nh, d_hits);
        hipLaunchKernelGGL(k_lenc_term_write, grid_for(nterms), block, 0, stream, a, pl, d_index, d_hits);
        HIP_TRY(hipGetLastError());
        if (*out.index_len)
                HIP_TRY(hipMemcpyAsync(out.index, d_index, *out.index_len, hipMemcpyDeviceToHost, stream));
        if (*out.hits_len)
                HIP_TRY(hipMemcpyAsync(out.hits, d_hits, *out.hits_len, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return TRI_OK;
}

// the encoder of a codec over postings that are already on the device: what the encode entry points upload, what commit sorts, what merge keeps
int encode_device(const int codec, WriteScratch &s, const EncIn &in, const uint64_t *term_first, const size_t nterms, const EncOut &out) {
        return codec == TRI_CODEC_LUCENE ? encode_lucene_device(s, in, term_first, nterms, out) : encode_google_device(s, in, term_first, nterms, out);
}

// ---- the encode entry points' host side: what the reference's encoders would refuse — term_first ascending; within a term, documents > 0 and strictly
//      ascending; freqs[] within positions[]; a payload of at most 8 bytes (google_codec.cpp:46, lucene_codec.cpp:262); within a document, positions non-descending
//      (google_codec.cpp:49: the encoder writes pos - lastPos) and > 0 for a hit without payload (new_hit drops such a hit, google_codec.cpp:42-45, as does
//      lucene_encoder.hpp: refused here rather than dropped silently; a position-0 hit WITH a payload is a counted hit).  *nhits: the hits in all.
int validate_postings(const char *fn, const uint32_t *docs, const uint32_t *freqs, const uint16_t *positions, const uint8_t *payload_lens, const size_t npositions,
                      const uint64_t *term_first, const size_t nterms, uint64_t *nhits_out) {
        uint64_t nhits = 0;
        for (size_t t = 0; t < nterms; ++t) {
                if (term_first[t + 1] < term_first[t])
                        return fail(TRI_ERR_INVALID, "%s: term_first must ascend", fn);
                if (term_first[t + 1] - term_first[t] > 0xffffffffull)
                        return fail(TRI_ERR_UNSUPPORTED, "term %zu: more than 2^32 documents", t);
                uint32_t prev = 0;
                for (uint64_t p = term_first[t]; p < term_first[t + 1]; ++p) {
                        if (!docs[p] || docs[p] <= prev)
                                return fail(TRI_ERR_INVALID, "term %zu: document IDs must be > 0 and strictly ascending (codecs.h:188-190)", t);
                        prev = docs[p];
                        // the posting's hits: positions[nhits .. nhits + freqs[p])
                        if ((uint64_t)freqs[p] > npositions - std::min<uint64_t>(npositions, nhits))
                                return fail(TRI_ERR_INVALID, "term %zu, document %u: freqs[] asks for more positions than the %zu given", t, docs[p], npositions);
                        uint32_t last_pos = 0;
                        for (uint64_t h = nhits; h < nhits + freqs[p]; ++h) {
                                const uint32_t plen = payload_lens ? payload_lens[h] : 0u;
                                if (plen > 8)
                                        return fail(TRI_ERR_INVALID, "term %zu, document %u: a payload of %u bytes (at most 8: google_codec.cpp:46, lucene_codec.cpp:262)", t, docs[p], plen);
                                if ((!positions[h] && !plen) || positions[h] < last_pos)
                                        return fail(TRI_ERR_INVALID, "term %zu, document %u: positions must be non-descending within a document, and > 0 for a hit without payload (google_codec.cpp:42-49)", t, docs[p]);
                                last_pos = positions[h];
                        }
                        nhits += freqs[p];
                }
        }
        *nhits_out = nhits;
        return TRI_OK;
}

// np postings and their nhits hits as the caller holds them, uploaded (payload_lens == nullptr: no hit has a payload)
int upload_postings(WriteScratch &s, const uint32_t *docs, const uint32_t *freqs, const uint16_t *positions, const uint8_t *payload_lens, const uint64_t *payloads, const uint64_t np,
                    const uint64_t nhits, EncIn &in) {
        const hipStream_t stream = s.dev->stream;
        uint32_t *d_docs, *d_freqs;
        uint16_t *d_pos;
        uint8_t *d_plens = nullptr;
        uint64_t *d_payloads = nullptr;
        HIP_TRY(s.get(d_docs, np + 1));
        HIP_TRY(s.get(d_freqs, np + 1));
        HIP_TRY(s.get(d_pos, nhits + 1));
        if (np) {
                HIP_TRY(hipMemcpyAsync(d_docs, docs, np * 4, hipMemcpyHostToDevice, stream));
                HIP_TRY(hipMemcpyAsync(d_freqs, freqs, np * 4, hipMemcpyHostToDevice, stream));
        }
        if (nhits)
                HIP_TRY(hipMemcpyAsync(d_pos, positions, nhits * 2, hipMemcpyHostToDevice, stream));
        if (nhits && payload_lens) {
                HIP_TRY(s.get(d_plens, nhits));
                HIP_TRY(s.get(d_payloads, nhits));
                HIP_TRY(hipMemcpyAsync(d_plens, payload_lens, nhits, hipMemcpyHostToDevice, stream));
                HIP_TRY(hipMemcpyAsync(d_payloads, payloads, nhits * 8, hipMemcpyHostToDevice, stream));
        }
        in = EncIn{d_docs, d_freqs, d_pos, d_plens, d_payloads, np, nhits};
        return TRI_OK;
}

// the encode entry points: the caller's postings validated on the host, uploaded, encoded
int encode_postings(const char *fn, const int codec, tri_dev *dev, const uint32_t *docs, const uint32_t *freqs, const uint16_t *positions, const uint8_t *payload_lens,
                    const uint64_t *payloads, const size_t npositions, const uint64_t *term_first, const size_t nterms, const EncOut &out) {
        if (!dev || !term_first || !out.index_len || (codec == TRI_CODEC_LUCENE && !out.hits_len) || (nterms && !out.terms) || (payload_lens && !payloads))
                return fail(TRI_ERR_INVALID, "%s: null argument", fn);
        HIP_TRY(hipSetDevice(dev->device));
        const uint64_t np = nterms ? term_first[nterms] : 0;
        if (np && (!docs || !freqs))
                return fail(TRI_ERR_INVALID, "%s: null postings", fn);
        if (npositions && !positions)
                return fail(TRI_ERR_INVALID, "%s: null positions", fn);
        uint64_t nhits = 0;
        if (int rc = validate_postings(fn, docs, freqs, positions, payload_lens, npositions, term_first, nterms, &nhits))
                return rc;
        WriteScratch s(dev);
        EncIn in;
        if (int rc = upload_postings(s, docs, freqs, positions, payload_lens, payloads, np, nhits, in))
                return rc;
        return encode_device(codec, s, in, term_first, nterms, out);
}
} // namespace

extern "C" int tri_encode_google(tri_dev *dev, const uint32_t *docs, const uint32_t *freqs, const uint16_t *positions, size_t npositions, const uint64_t *term_first,
                                 size_t nterms, uint8_t *index_out, size_t cap, size_t *index_len, tri_term *terms_out) {
        return tri_encode_google_payloads(dev, docs, freqs, positions, nullptr, nullptr, npositions, term_first, nterms, index_out, cap, index_len, terms_out);
}
extern "C" int tri_encode_google_payloads(tri_dev *dev, const uint32_t *docs, const uint32_t *freqs, const uint16_t *positions, const uint8_t *payload_lens,
                                          const uint64_t *payloads, size_t npositions, const uint64_t *term_first, size_t nterms, uint8_t *index_out, size_t cap,
                                          size_t *index_len, tri_term *terms_out) {
        return encode_postings("tri_encode_google", TRI_CODEC_GOOGLE, dev, docs, freqs, positions, payload_lens, payloads, npositions, term_first, nterms,
                               EncOut{index_out, cap, index_len, nullptr, 0, nullptr, terms_out});
}
extern "C" int tri_encode_lucene(tri_dev *dev, const uint32_t *docs, const uint32_t *freqs, const uint16_t *positions, size_t npositions, const uint64_t *term_first, size_t nterms,
                                 uint8_t *index_out, size_t index_cap, size_t *index_len, uint8_t *hits_out, size_t hits_cap, size_t *hits_len, tri_term *terms_out) {
        return tri_encode_lucene_payloads(dev, docs, freqs, positions, nullptr, nullptr, npositions, term_first, nterms, index_out, index_cap, index_len, hits_out, hits_cap, hits_len,
                                          terms_out);
}
extern "C" int tri_encode_lucene_payloads(tri_dev *dev, const uint32_t *docs, const uint32_t *freqs, const uint16_t *positions, const uint8_t *payload_lens, const uint64_t *payloads,
                                          size_t npositions, const uint64_t *term_first, size_t nterms, uint8_t *index_out, size_t index_cap, size_t *index_len, uint8_t *hits_out,
                                          size_t hits_cap, size_t *hits_len, tri_term *terms_out) {
        return encode_postings("tri_encode_lucene", TRI_CODEC_LUCENE, dev, docs, freqs, positions, payload_lens, payloads, npositions, term_first, nterms,
                               EncOut{index_out, index_cap, index_len, hits_out, hits_cap, hits_len, terms_out});
}

// ---- SegmentIndexSession::commit (indexer.cpp:311-478) on the device: sort, gather, encode (k_commit.hpp, commit_sort.hip, the codec's encoder)
// (codec: TRI_CODEC_GOOGLE — index_out only —, or TRI_CODEC_LUCENE — index_out + hits_out)
static int commit_device(tri_dev *dev, const int codec, const uint32_t *term_ids, const uint32_t *doc_ids, const uint32_t *freqs, const uint16_t *positions, const uint8_t *payload_lens,
                         const uint64_t *payloads, size_t npostings, size_t npositions, uint8_t *index_out, size_t cap, size_t *index_len, uint8_t *hits_out, size_t hits_cap,
                         size_t *hits_len, uint32_t *term_ids_out, tri_term *terms_out, size_t terms_cap, size_t *nterms, tri_commit_stats *stats) {
        const char *const fn = codec == TRI_CODEC_LUCENE ? "tri_commit_lucene" : "tri_commit_google";
        if (!dev || !index_len || !nterms || (npostings && (!term_ids || !doc_ids || !freqs)) || (payload_lens && !payloads) || (npositions && !positions))
                return fail(TRI_ERR_INVALID, "%s: null argument", fn);
        if (npostings > 0xfffffff0ull)
                return fail(TRI_ERR_UNSUPPORTED, "%s: more than 2^32 postings in one session: commit in parts", fn);
        HIP_TRY(hipSetDevice(dev->device));
        const hipStream_t stream = dev->stream;
        const uint64_t np = npostings;
        uint64_t nhits = 0, docs_cnt = 0;
        for (uint64_t i = 0; i < np; ++i) { // (the session's own bookkeeping: hits in all, documents = runs of one documentID in insertion order)
                nhits += freqs[i];
                docs_cnt += i == 0 || doc_ids[i] != doc_ids[i - 1];
        }
        if (nhits > npositions)
                return fail(TRI_ERR_INVALID, "%s: freqs[] asks for %llu positions, %zu given", fn, (unsigned long long)nhits, npositions);
        *nterms = 0;
        *index_len = 0;
        if (stats)
                *stats = tri_commit_stats{docs_cnt, np, nhits, 0};
        if (!np)
                return TRI_OK;
        WriteScratch s(dev);
        // ---- the session's postings, as inserted
        uint32_t *d_terms, *d_vals, *d_perm, *d_marks;
        unsigned long long *d_keys, *d_keys_sorted, *d_err;
        uint64_t *d_hit_off_in, *d_hit_off_out, *d_mark_rank;
        HIP_TRY(s.get(d_terms, np));
        HIP_TRY(s.get(d_keys, np));
        HIP_TRY(s.get(d_keys_sorted, np));
        HIP_TRY(s.get(d_vals, np));
        HIP_TRY(s.get(d_perm, np));
        HIP_TRY(s.get(d_marks, np));
        HIP_TRY(s.get(d_hit_off_in, np + 1));
        HIP_TRY(s.get(d_hit_off_out, np + 1));
        HIP_TRY(s.get(d_mark_rank, np + 1));
        HIP_TRY(s.get(d_err, 1));
        HIP_TRY(hipMemcpyAsync(d_terms, term_ids, np * 4, hipMemcpyHostToDevice, stream));
        EncIn raw;
        int rcs;
        if ((rcs = upload_postings(s, doc_ids, freqs, positions, payload_lens, payloads, np, nhits, raw)))
                return rcs;
        // ---- the sorted postings: what the encoder reads
        uint32_t *d_docs, *d_freqs;
        uint16_t *d_pos;
        uint8_t *d_plens = nullptr;
        uint64_t *d_payloads = nullptr;
        HIP_TRY(s.get(d_docs, np));
        HIP_TRY(s.get(d_freqs, np));
        HIP_TRY(s.get(d_pos, nhits + 1));
        if (nhits && payload_lens) {
                HIP_TRY(s.get(d_plens, nhits));
                HIP_TRY(s.get(d_payloads, nhits));
        }
        const dim3 grid = grid_for(np), block(256);
        // ---- keys in the order the reference's commit walks (bucket = termID & 31, then termID, then documentID), sorted with the postings' indices
        hipLaunchKernelGGL(k_commit_keys, grid, block, 0, stream, d_terms, raw.docs, d_keys, d_vals, np);
        if ((rcs = sort_pairs(s, d_keys, d_keys_sorted, d_vals, d_perm, np)))
                return rcs;
        // ---- documents and frequencies in sorted order; the hits follow their postings
        hipLaunchKernelGGL(k_commit_gather, grid, block, 0, stream, d_keys_sorted, d_perm, raw.freqs, d_docs, d_freqs, d_marks, np);
        if ((rcs = enc_scan(s, raw.freqs, d_hit_off_in, np)) || (rcs = enc_scan(s, d_freqs, d_hit_off_out, np)) || (rcs = enc_scan(s, d_marks, d_mark_rank, np)))
                return rcs;
        hipLaunchKernelGGL(k_commit_hits, grid, block, 0, stream, d_perm, d_hit_off_in, d_hit_off_out, d_freqs, raw.pos, d_pos, raw.plens, d_plens, raw.payloads, d_payloads, np);
        HIP_TRY(hipMemsetAsync(d_err, 0xff, 8, stream));
        hipLaunchKernelGGL(k_commit_validate, grid, block, 0, stream, d_keys_sorted, d_freqs, d_hit_off_out, d_pos, d_plens, np, d_err);
        HIP_TRY(hipGetLastError());
        unsigned long long err = 0;
        uint64_t nt = 0;
        HIP_TRY(hipMemcpyAsync(&err, d_err, 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(&nt, d_mark_rank + np, 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (err != ~0ull) {
                static const char *const why[] = {"", "document 0", "the same (term, document) twice (indexer.cpp:446: documentID > prevDID)",
                                                  "positions must be non-descending within a document, and > 0 for a hit without payload (google_codec.cpp:42-49)",
                                                  "a payload of more than 8 bytes (google_codec.cpp:46, lucene_codec.cpp:262)"};
                return fail(TRI_ERR_INVALID, "%s: sorted posting %llu: %s", fn, (unsigned long long)(err >> 8) - 1, why[std::min<unsigned long long>(err & 0xff, 4)]);
        }
        *nterms = (size_t)nt;
        if (stats)
                stats->total_terms = nt;
        // ---- the distinct terms: first postings and termIDs, commit order
        uint64_t *d_term_first;
        uint32_t *d_term_ids;
        HIP_TRY(s.get(d_term_first, nt + 1));
        HIP_TRY(s.get(d_term_ids, nt));
        hipLaunchKernelGGL(k_commit_terms, grid, block, 0, stream, d_keys_sorted, d_marks, d_mark_rank, d_term_first, d_term_ids, np);
        HIP_TRY(hipGetLastError());
        std::vector<uint64_t> term_first(nt + 1);
        std::vector<uint32_t> tids(nt);
        HIP_TRY(hipMemcpyAsync(term_first.data(), d_term_first, nt * 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(tids.data(), d_term_ids, nt * 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        term_first[nt] = np;
        std::vector<tri_term> tt(nt);
        uint8_t *const io = index_out && terms_cap >= nt ? index_out : nullptr;
        if (int rc = encode_device(codec, s, EncIn{d_docs, d_freqs, d_pos, d_plens, d_payloads, np, nhits}, term_first.data(), nt,
                                   EncOut{io, cap, index_len, hits_out, hits_cap, hits_len, tt.data()}))
                return rc;
        if (!index_out)
                return TRI_OK; // (sizing call: *index_len and *nterms)
        if (terms_cap < nt || !terms_out || !term_ids_out)
                return fail(TRI_ERR_INVALID, "%s: the session holds %llu distinct terms, room for %zu given", fn, (unsigned long long)nt, terms_cap);
        memcpy(terms_out, tt.data(), nt * sizeof(tri_term));
        memcpy(term_ids_out, tids.data(), nt * 4);
        return TRI_OK;
}

extern "C" int tri_commit_google(tri_dev *dev, const uint32_t *term_ids, const uint32_t *doc_ids, const uint32_t *freqs, const uint16_t *positions, const uint8_t *payload_lens,
                                 const uint64_t *payloads, size_t npostings, size_t npositions, uint8_t *index_out, size_t cap, size_t *index_len, uint32_t *term_ids_out,
                                 tri_term *terms_out, size_t terms_cap, size_t *nterms, tri_commit_stats *stats) {
        return commit_device(dev, TRI_CODEC_GOOGLE, term_ids, doc_ids, freqs, positions, payload_lens, payloads, npostings, npositions, index_out, cap, index_len, nullptr, 0, nullptr,
                             term_ids_out, terms_out, terms_cap, nterms, stats);
}
extern "C" int tri_commit_lucene(tri_dev *dev, const uint32_t *term_ids, const uint32_t *doc_ids, const uint32_t *freqs, const uint16_t *positions, size_t npostings, size_t npositions,
                                 uint8_t *index_out, size_t cap, size_t *index_len, uint8_t *hits_out, size_t hits_cap, size_t *hits_len, uint32_t *term_ids_out, tri_term *terms_out,
                                 size_t terms_cap, size_t *nterms, tri_commit_stats *stats) {
        return tri_commit_lucene_payloads(dev, term_ids, doc_ids, freqs, positions, nullptr, nullptr, npostings, npositions, index_out, cap, index_len, hits_out, hits_cap, hits_len,
                                          term_ids_out, terms_out, terms_cap, nterms, stats);
}
extern "C" int tri_commit_lucene_payloads(tri_dev *dev, const uint32_t *term_ids, const uint32_t *doc_ids, const uint32_t *freqs, const uint16_t *positions, const uint8_t *payload_lens,
                                          const uint64_t *payloads, size_t npostings, size_t npositions, uint8_t *index_out, size_t cap, size_t *index_len, uint8_t *hits_out,
                                          size_t hits_cap, size_t *hits_len, uint32_t *term_ids_out, tri_term *terms_out, size_t terms_cap, size_t *nterms, tri_commit_stats *stats) {
        if (!hits_len)
                return fail(TRI_ERR_INVALID, "tri_commit_lucene: null argument");
        *hits_len = 0;
        return commit_device(dev, TRI_CODEC_LUCENE, term_ids, doc_ids, freqs, positions, payload_lens, payloads, npostings, npositions, index_out, cap, index_len, hits_out, hits_cap,
                             hits_len, term_ids_out, terms_out, terms_cap, nterms, stats);
}

// ---- The codecs' merge for a whole dictionary, on the device (Codecs::Google::IndexSession::merge, google_codec.cpp:186-438; Codecs::Lucene::IndexSession::merge,
// lucene_codec.cpp:963-1396 — the same k-way walk over the participants' postings, most recent first, the winner kept unless its participant masks it; the codecs differ in how
// postings and hits are stored, i.e. in the decode and the encode at the two ends of the sort below; k_commit.hpp)
static int merge_device(tri_dev *dev, const int codec, tri_index *const *parts, size_t nparts, const uint32_t *part_terms, size_t nterms, uint8_t *index_out, size_t cap, size_t *index_len,
                        uint8_t *hits_out, size_t hits_cap, size_t *hits_len, tri_term *terms_out, tri_commit_stats *stats) {
        const char *const fn = codec == TRI_CODEC_LUCENE ? "tri_merge_lucene" : "tri_merge_google";
        if (!dev || !parts || !nparts || (nterms && (!part_terms || !terms_out)) || !index_len)
                return fail(TRI_ERR_INVALID, "%s: null argument", fn);
        if (nparts > 65535)
                return fail(TRI_ERR_INVALID, "%s: at most 65535 participants (google_codec.cpp:186 / lucene_codec.cpp:963: uint16_t participantsCnt)", fn);
        HIP_TRY(hipSetDevice(dev->device));
        const hipStream_t stream = dev->stream;
        for (size_t p = 0; p < nparts; ++p) {
                if (!parts[p] || parts[p]->dev != dev || parts[p]->codec != codec)
                        return fail(TRI_ERR_INVALID, "%s: participant %zu is not a %s index of this device", fn, p, codec == TRI_CODEC_GOOGLE ? "google_codec" : "lucene_codec");
                if (codec == TRI_CODEC_LUCENE && !parts[p]->d_hits && parts[p]->info.postings)
                        return fail(TRI_ERR_INVALID, "%s: participant %zu was uploaded without its hits.data (the merged segment needs every hit)", fn, p);
        }
        // ---- the jobs: every (participant, output term) that holds postings, participant-major — the most recent participant's postings first, so that
        //      a stable sort leaves them first among equal (term, document) keys
        std::vector<std::vector<MergeJob>> jobs(nparts);
        std::vector<uint64_t> part_first(nparts + 1, 0);
        uint64_t np = 0;
        for (size_t p = 0; p < nparts; ++p) {
                part_first[p] = np;
                for (size_t t = 0; t < nterms; ++t) {
                        const uint32_t idx = part_terms[t * nparts + p];
                        if (idx == 0xffffffffu)
                                continue;
                        if (idx >= parts[p]->terms.size())
                                return fail(TRI_ERR_INVALID, "%s: output term %zu: term %u out of range in participant %zu", fn, t, idx, p);
                        const DevTerm &dt = parts[p]->terms[idx];
                        if (!dt.documents)
                                continue; // (merge.cpp:263-270: a participant without documents for the term takes no part)
                        if (!(dt.flags & TERM_FULL_BLOCKS))
                                return fail(TRI_ERR_UNSUPPORTED, "%s: term %u of participant %zu has short blocks inside its list (not written by the reference's encoder)", fn, idx, p);
                        jobs[p].push_back({idx, (uint32_t)t, np});
                        np += dt.documents;
                }
        }
        part_first[nparts] = np;
        if (np > 0xfffffff0ull)
                return fail(TRI_ERR_UNSUPPORTED, "%s: more than 2^32 postings: merge in parts", fn);
        *index_len = 0;
        if (stats)
                *stats = tri_commit_stats{0, 0, 0, 0};
        WriteScratch s(dev);
        EncIn in; // the merged postings: what the encoder reads
        std::vector<uint64_t> term_first(nterms + 1, 0);
        if (np) {
                // ---- every participant's postings, concatenated: (output term, document) keys, frequencies, then the hits
                unsigned long long *d_keys, *d_keys_sorted;
                uint32_t *d_vals, *d_perm, *d_freqs_all, *d_keep, *d_term_cnt;
                uint64_t *d_hit_off_all, *d_rank, *d_part_first, *d_term_first;
                const uint32_t **d_masked;
                HIP_TRY(s.get(d_keys, np));
                HIP_TRY(s.get(d_keys_sorted, np));
                HIP_TRY(s.get(d_vals, np));
                HIP_TRY(s.get(d_perm, np));
                HIP_TRY(s.get(d_freqs_all, np));
                HIP_TRY(s.get(d_keep, np));
                HIP_TRY(s.get(d_hit_off_all, np + 1));
                HIP_TRY(s.get(d_rank, np + 1));
                HIP_TRY(s.get(d_part_first, nparts + 1));
                HIP_TRY(s.get(d_masked, nparts));
                HIP_TRY(s.get(d_term_cnt, nterms + 1));
                HIP_TRY(s.get(d_term_first, nterms + 2));
                std::vector<const uint32_t *> masked(nparts);
                for (size_t p = 0; p < nparts; ++p)
                        masked[p] = parts[p]->d_masked;
                HIP_TRY(hipMemcpyAsync(d_part_first, part_first.data(), (nparts + 1) * 8, hipMemcpyHostToDevice, stream));
                HIP_TRY(hipMemcpyAsync(d_masked, masked.data(), nparts * sizeof(void *), hipMemcpyHostToDevice, stream));
                std::vector<MergeJob *> d_jobs(nparts, nullptr);
                for (size_t p = 0; p < nparts; ++p) {
                        if (jobs[p].empty())
                                continue;
                        HIP_TRY(s.get(d_jobs[p], jobs[p].size()));
                        HIP_TRY(hipMemcpyAsync(d_jobs[p], jobs[p].data(), jobs[p].size() * sizeof(MergeJob), hipMemcpyHostToDevice, stream));
                        const tri_index *ix = parts[p];
                        TRI_LAUNCH(k_merge_decode, codec, job_grid(dev, jobs[p].size()), dim3(256), stream, ix->d_index, ix->d_blk_last, ix->d_blk_off, ix->d_terms,
                                   (const MergeJob *)d_jobs[p], (uint32_t)jobs[p].size(), d_freqs_all, d_keys, d_vals);
                }
                HIP_TRY(hipGetLastError());
                int rcs;
                if ((rcs = enc_scan(s, d_freqs_all, d_hit_off_all, np)))
                        return rcs;
                uint64_t nh_all = 0;
                HIP_TRY(hipMemcpyAsync(&nh_all, d_hit_off_all + np, 8, hipMemcpyDeviceToHost, stream));
                HIP_TRY(hipStreamSynchronize(stream));
                uint16_t *d_pos_all;
                uint8_t *d_plens_all;
                uint64_t *d_payloads_all;
                HIP_TRY(s.get(d_pos_all, nh_all + 1));
                HIP_TRY(s.get(d_plens_all, nh_all + 1));
                HIP_TRY(s.get(d_payloads_all, nh_all + 1));
                for (size_t p = 0; p < nparts; ++p) {
                        if (jobs[p].empty())
                                continue;
                        const tri_index *ix = parts[p];
                        if (codec == TRI_CODEC_LUCENE)
                                hipLaunchKernelGGL(k_merge_hits_lucene, job_grid(dev, jobs[p].size()), dim3(256), 0, stream, ix->d_hits, ix->d_blk_hits, ix->d_hdir, ix->d_pdir, ix->d_terms,
                                                   d_jobs[p], (uint32_t)jobs[p].size(), d_freqs_all, d_hit_off_all, d_pos_all, d_plens_all, d_payloads_all);
                        else
                                hipLaunchKernelGGL(k_merge_hits, job_grid(dev, jobs[p].size()), dim3(256), 0, stream, ix->d_index, ix->d_blk_off, ix->d_blk_hits, ix->d_terms,
                                                   d_jobs[p], (uint32_t)jobs[p].size(), d_freqs_all, d_hit_off_all, d_pos_all, d_plens_all, d_payloads_all);
                }
                HIP_TRY(hipGetLastError());
                // ---- sort by (output term, document); the first of equal keys is the most recent participant's
                if ((rcs = sort_pairs(s, d_keys, d_keys_sorted, d_vals, d_perm, np)))
                        return rcs;
                const dim3 grid = grid_for(np), block(256);
                hipLaunchKernelGGL(k_merge_select, grid, block, 0, stream, d_keys_sorted, d_perm, d_part_first, (uint32_t)nparts, d_masked, d_keep, np);
                if ((rcs = enc_scan(s, d_keep, d_rank, np)))
                        return rcs;
                uint64_t kept = 0, nh_out = 0;
                HIP_TRY(hipMemcpyAsync(&kept, d_rank + np, 8, hipMemcpyDeviceToHost, stream));
                HIP_TRY(hipStreamSynchronize(stream));
                // ---- the postings that stay, term after term, and their hits
                uint32_t *d_docs, *d_freqs, *d_src_of;
                uint64_t *d_hit_off_out;
                HIP_TRY(s.get(d_docs, kept + 1));
                HIP_TRY(s.get(d_freqs, kept + 1));
                HIP_TRY(s.get(d_src_of, kept + 1));
                HIP_TRY(s.get(d_hit_off_out, kept + 2));
                HIP_TRY(hipMemsetAsync(d_term_cnt, 0, (nterms + 1) * 4, stream));
                hipLaunchKernelGGL(k_merge_compact, grid, block, 0, stream, d_keys_sorted, d_perm, d_keep, d_rank, d_freqs_all, d_docs, d_freqs, d_src_of, d_term_cnt, np);
                if ((rcs = enc_scan(s, d_freqs, d_hit_off_out, kept)) || (rcs = enc_scan(s, d_term_cnt, d_term_first, nterms)))
                        return rcs;
                HIP_TRY(hipMemcpyAsync(&nh_out, d_hit_off_out + kept, 8, hipMemcpyDeviceToHost, stream));
                HIP_TRY(hipMemcpyAsync(term_first.data(), d_term_first, (nterms + 1) * 8, hipMemcpyDeviceToHost, stream));
                HIP_TRY(hipStreamSynchronize(stream));
                uint16_t *d_pos;
                uint8_t *d_plens;
                uint64_t *d_payloads;
                HIP_TRY(s.get(d_pos, nh_out + 1));
                HIP_TRY(s.get(d_plens, nh_out + 1));
                HIP_TRY(s.get(d_payloads, nh_out + 1));
                if (kept)
                        hipLaunchKernelGGL(k_commit_hits, grid_for(kept), block, 0, stream, d_src_of, d_hit_off_all, d_hit_off_out, d_freqs, d_pos_all, d_pos, d_plens_all, d_plens,
                                           d_payloads_all, d_payloads, kept);
                HIP_TRY(hipGetLastError());
                in = EncIn{d_docs, d_freqs, d_pos, d_plens, d_payloads, kept, nh_out};
        }
        if (int rc = encode_device(codec, s, in, term_first.data(), nterms, EncOut{index_out, cap, index_len, hits_out, hits_cap, hits_len, terms_out}))
                return rc;
        if (stats) {
                stats->sum_terms_docs = in.np;
                stats->sum_term_hits = in.nhits;
                for (size_t t = 0; t < nterms; ++t)
                        stats->total_terms += term_first[t + 1] > term_first[t]; // (merge.cpp:241: a term that keeps no document is dropped from the dictionary)
        }
        return TRI_OK;
}
extern "C" int tri_merge_google(tri_dev *dev, tri_index *const *parts, size_t nparts, const uint32_t *part_terms, size_t nterms, uint8_t *index_out, size_t cap, size_t *index_len,
                                tri_term *terms_out, tri_commit_stats *stats) {
        return merge_device(dev, TRI_CODEC_GOOGLE, parts, nparts, part_terms, nterms, index_out, cap, index_len, nullptr, 0, nullptr, terms_out, stats);
}
extern "C" int tri_merge_lucene(tri_dev *dev, tri_index *const *parts, size_t nparts, const uint32_t *part_terms, size_t nterms, uint8_t *index_out, size_t cap, size_t *index_len,
                                uint8_t *hits_out, size_t hits_cap, size_t *hits_len, tri_term *terms_out, tri_commit_stats *stats) {
        if (!hits_len)
                return fail(TRI_ERR_INVALID, "tri_merge_lucene: null argument");
        *hits_len = 0;
        return merge_device(dev, TRI_CODEC_LUCENE, parts, nparts, part_terms, nterms, index_out, cap, index_len, hits_out, hits_cap, hits_len, terms_out, stats);
}

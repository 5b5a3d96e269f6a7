// k_isect.hpp — Trinity::intersect (intersect.h:25-37, intersect.cpp:5-170) on the device: which subsets of a request's token groups co-occur in documents
// Part of libtrinity_hip.so (MI355X / gfx950); included by trinity_hip.hip.  New code, no reference source.
//
// The reference merges up to 512 postings iterators by a linear scan per document (:107-158).  Here every distinct known term of the call is decoded ONCE into
// a plane-0 row (k_term_plane0, k_planes.hpp: bit d = the list holds document d) in a scratch block of the call, and a document's mask is one bit per group
// read from those rows.  Two passes over the docID space build the two order-free tables csrc/host/isect_rows.hpp derives the reference's list from:
//   k_isect_hist  (pass 1) H: per distinct considered mask its documents and its first docID; and per span the last considered mask (0: none)
//   k_isect_runs  (pass 2) C: per (mask, epoch) the considered documents whose preceding considered document has the same mask, for masks that are absent from
//                 the reference's vector by then (the host computed thresholds and epoch bounds from H in between)
// Both: one wave64 per (span of ISECT_SPAN documents, request); a step is 64 documents, a lane owns one.  A lane first ORs the words of its OWN step of every
// row (one coalesced 512-byte read per row and span); the ballot of non-zero words names the steps that hold any document at all — the others (the common
// case for rare tokens) are skipped.  In a live step the row words are wave-uniform loads (they were just fetched), bit `lane` of each goes to its group's bit.
// A document is CONSIDERED when its mask is not origMask, neither its lowest nor its highest set bit is a stop word (what intersect.h:15-18 documents; the
// reference's code tests slot indices of remaining[] instead, :112-139 — equal only while stopwordsMask == 0, include/trinity_hip.h), and the index's masked
// bitmap does not hold it.
// Tables: open addressing, linear probing, key 0 = empty (a mask is never 0; a C key holds an epoch >= 1).  Pass 1 aggregates equal masks within the step
// (ballot), then in an LDS table of the wave (ISECT_LDS_SLOTS keys: 4 KB, SoA — probes are wave-uniform broadcast reads, stores come from one lane: no bank
// conflicts), flushed to the request's global table at the span's end; a mask that finds the LDS table full goes to the global table at once (counted:
// tri_isect_info.lds_spills).  A full global table sets the request's overflow flag: the request answers TRI_ERR_UNSUPPORTED, and every later insert of the
// request returns at once (a full table is walked whole by the inserts that find it full, not by everything after them).
// Every shuffle below runs with all 64 lanes active: the loops around them are driven by wave-uniform ballots.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr uint32_t ISECT_SPAN = 4096;              // documents a wave takes
constexpr uint32_t ISECT_STEPS = ISECT_SPAN / 64;  // ... in steps of 64: one 64-bit word of every row
constexpr uint32_t ISECT_LDS_SLOTS = 256;          // keys of a wave's LDS table
constexpr uint32_t ISECT_OVF_MASKS = 1u, ISECT_OVF_RUNS = 2u; // a request's overflow flags
constexpr uint32_t ISECT_NEVER = 0xffffffffu;      // threshold of a mask that never leaves the vector
static_assert(ISECT_STEPS == 64, "a lane prefetches the words of one step");
static_assert((ISECT_LDS_SLOTS & (ISECT_LDS_SLOTS - 1)) == 0, "the LDS probe wraps with a mask");

struct IsectReq {
        uint64_t orig_mask, stop_mask;
        uint32_t row_first, nrows;    // rowtab[row_first .. + nrows): (scratch row, group) of every known term of the request
        uint32_t bounds_off, nbounds; // pass 2: the request's epoch bounds (the distinct masks' first docIDs, ascending)
        uint32_t skip, pad;           // pass 2: nothing to count (no mask has a strict superset, or H overflowed)
};
struct IsectTables {
        unsigned long long *h_key; // [nreq][h_cap]
        uint32_t *h_cnt, *h_first;
        unsigned long long *c_key; // [nreq][c_cap]: slot of the mask in H << 32 | epoch
        uint32_t *c_cnt;
        uint32_t *flags, *spills; // [nreq]
        uint32_t h_cap, c_cap;
};

__device__ __forceinline__ uint32_t isect_hash(const uint64_t k) { return (uint32_t)((k * 0x9E3779B97F4A7C15ull) >> 32); }
__device__ __forceinline__ uint64_t isect_shfl(const uint64_t v, const uint32_t src) {
        const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, (int)src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), (int)src, 64);
        return (uint64_t)lo | ((uint64_t)hi << 32);
}
__device__ __forceinline__ uint32_t isect_low(const uint64_t b) { return (uint32_t)__builtin_ctzll(b); }
__device__ __forceinline__ uint32_t isect_high(const uint64_t b) { return 63u - (uint32_t)__builtin_clzll(b); }

// the words of the lane's own step of every row, OR-ed: bit s of the ballot <=> step s of the span holds a document of the request
__device__ __forceinline__ uint64_t isect_live_steps(const uint64_t *__restrict__ rows, const size_t plw64, const uint2 *__restrict__ rt, const uint32_t nrows, const size_t w0, const uint32_t lane) {
        uint64_t any = 0;
        for (uint32_t i = 0; i < nrows; ++i)
                any |= rows[(size_t)rt[i].x * plw64 + w0 + lane];
        return __ballot(any != 0);
}
// the lane's document's mask in step word w
__device__ __forceinline__ uint64_t isect_step_mask(const uint64_t *__restrict__ rows, const size_t plw64, const uint2 *__restrict__ rt, const uint32_t nrows, const size_t w, const uint32_t lane) {
        uint64_t mask = 0;
        for (uint32_t i = 0; i < nrows; ++i) {
                const uint2 e = rt[i];                                // (wave-uniform)
                const uint64_t word = rows[(size_t)e.x * plw64 + w]; // (wave-uniform)
                mask |= ((word >> lane) & 1ull) << e.y;
        }
        return mask;
}
__device__ __forceinline__ bool isect_considered(const uint64_t mask, const uint64_t orig, const uint64_t stop, const uint32_t *__restrict__ masked, const uint32_t d) {
        if (!mask || mask == orig)
                return false;
        if (stop & ((mask & (0ull - mask)) | (1ull << isect_high(mask))))
                return false;
        return !(masked && ((masked[d >> 5] >> (d & 31u)) & 1u));
}

// one lane: add (cnt documents, first docID) to mask's entry of request r's global table H
__device__ __forceinline__ void isect_h_add(const IsectTables &T, const uint32_t r, const uint64_t mask, const uint32_t cnt, const uint32_t first) {
        if (*(volatile uint32_t *)(T.flags + r) & ISECT_OVF_MASKS) // the request has overflowed already: its answer is void, no further insert walks the full table
                return;
        unsigned long long *keys = T.h_key + (size_t)r * T.h_cap;
        uint32_t s = isect_hash(mask) % T.h_cap;
        for (uint32_t i = 0; i < T.h_cap; ++i) {
                unsigned long long k = *(volatile unsigned long long *)(keys + s); // (a key only ever goes 0 -> mask: a stale 0 is settled by the CAS)
                if (k == 0ull) {
                        k = atomicCAS(keys + s, 0ull, (unsigned long long)mask);
                        if (k == 0ull)
                                k = mask;
                }
                if (k == mask) {
                        atomicAdd(T.h_cnt + (size_t)r * T.h_cap + s, cnt);
                        atomicMin(T.h_first + (size_t)r * T.h_cap + s, first);
                        return;
                }
                s = s + 1u == T.h_cap ? 0u : s + 1u;
        }
        atomicOr(T.flags + r, ISECT_OVF_MASKS);
}
// ... cnt documents to key's entry of its table C
__device__ __forceinline__ void isect_c_add(const IsectTables &T, const uint32_t r, const uint64_t key, const uint32_t cnt) {
        if (*(volatile uint32_t *)(T.flags + r) & ISECT_OVF_RUNS) // (as above)
                return;
        unsigned long long *keys = T.c_key + (size_t)r * T.c_cap;
        uint32_t s = isect_hash(key) % T.c_cap;
        for (uint32_t i = 0; i < T.c_cap; ++i) {
                unsigned long long k = *(volatile unsigned long long *)(keys + s);
                if (k == 0ull) {
                        k = atomicCAS(keys + s, 0ull, (unsigned long long)key);
                        if (k == 0ull)
                                k = key;
                }
                if (k == key) {
                        atomicAdd(T.c_cnt + (size_t)r * T.c_cap + s, cnt);
                        return;
                }
                s = s + 1u == T.c_cap ? 0u : s + 1u;
        }
        atomicOr(T.flags + r, ISECT_OVF_RUNS);
}

// ------------------------------------------------------------------------------------------ pass 1
__global__ __launch_bounds__(64) void k_isect_hist(const uint64_t *__restrict__ rows, const size_t plw64, const uint2 *__restrict__ rowtab, const IsectReq *__restrict__ reqs,
                                                   const uint32_t *__restrict__ masked, const IsectTables T, unsigned long long *__restrict__ span_last, const uint32_t nspans) {
        __shared__ unsigned long long l_key[ISECT_LDS_SLOTS];
        __shared__ uint32_t l_cnt[ISECT_LDS_SLOTS], l_first[ISECT_LDS_SLOTS];
        const uint32_t lane = threadIdx.x, p = blockIdx.x, r = blockIdx.y;
        const IsectReq q = reqs[r];
        const uint2 *rt = rowtab + q.row_first;
        for (uint32_t i = lane; i < ISECT_LDS_SLOTS; i += 64)
                l_key[i] = 0ull;
        __syncthreads();
        const size_t w0 = (size_t)p * ISECT_STEPS;
        uint64_t last = 0;
        for (uint64_t live = isect_live_steps(rows, plw64, rt, q.nrows, w0, lane); live; live &= live - 1) {
                const uint32_t s = isect_low(live), d = (uint32_t)((w0 + s) * 64u) + lane;
                const uint64_t mask = isect_step_mask(rows, plw64, rt, q.nrows, w0 + s, lane);
                const bool ok = isect_considered(mask, q.orig_mask, q.stop_mask, masked, d);
                uint64_t rem = __ballot(ok);
                if (!rem)
                        continue;
                last = isect_shfl(mask, isect_high(rem));
                while (rem) { // the step's distinct masks, each once
                        const uint32_t leader = isect_low(rem);
                        const uint64_t m0 = isect_shfl(mask, leader);
                        const uint64_t same = __ballot(ok && mask == m0);
                        rem &= ~same;
                        const uint32_t cnt = (uint32_t)__popcll(same), first = d - lane + leader;
                        uint32_t slot = isect_hash(m0) & (ISECT_LDS_SLOTS - 1);
                        unsigned long long k = 1ull;
                        bool found = false;
                        for (uint32_t i = 0; i < ISECT_LDS_SLOTS; ++i) { // (wave-uniform probe)
                                k = l_key[slot];
                                if (k == m0 || k == 0ull) {
                                        found = true;
                                        break;
                                }
                                slot = (slot + 1u) & (ISECT_LDS_SLOTS - 1);
                        }
                        if (found) {
                                if (lane == 0) {
                                        if (k == 0ull) {
                                                l_key[slot] = m0;
                                                l_cnt[slot] = cnt;
                                                l_first[slot] = first; // (documents ascend within a span: the first one seen is the lowest)
                                        } else
                                                l_cnt[slot] += cnt;
                                }
                                __syncthreads();
                        } else if (lane == 0) { // the LDS table is full: straight to the global one
                                isect_h_add(T, r, m0, cnt, first);
                                atomicAdd(T.spills + r, 1u);
                        }
                }
        }
        __syncthreads();
        for (uint32_t i = lane; i < ISECT_LDS_SLOTS; i += 64)
                if (l_key[i])
                        isect_h_add(T, r, l_key[i], l_cnt[i], l_first[i]);
        if (lane == 0)
                span_last[(size_t)r * nspans + p] = last;
}

// ------------------------------------------------------------------------------------------ pass 2
// thr[r][slot]: the docID from which the mask of H's slot is absent from the reference's vector (ISECT_NEVER: it stays); bounds: the requests' epoch bounds
__global__ __launch_bounds__(64) void k_isect_runs(const uint64_t *__restrict__ rows, const size_t plw64, const uint2 *__restrict__ rowtab, const IsectReq *__restrict__ reqs,
                                                   const uint32_t *__restrict__ masked, const IsectTables T, const unsigned long long *__restrict__ span_last, const uint32_t nspans,
                                                   const uint32_t *__restrict__ thr, const uint32_t *__restrict__ bounds) {
        const uint32_t lane = threadIdx.x, p = blockIdx.x, r = blockIdx.y;
        const IsectReq q = reqs[r];
        if (q.skip)
                return;
        const uint2 *rt = rowtab + q.row_first;
        const size_t w0 = (size_t)p * ISECT_STEPS;
        uint64_t live = isect_live_steps(rows, plw64, rt, q.nrows, w0, lane);
        if (!live)
                return;
        // the mask of the last considered document before the span: the nearest earlier span that holds one (pass 1 is complete), 64 spans a look
        uint64_t prev = 0;
        for (int64_t base = (int64_t)p - 1; base >= 0 && !prev; base -= 64) {
                const int64_t idx = base - (int64_t)lane;
                const uint64_t v = idx >= 0 ? span_last[(size_t)r * nspans + (size_t)idx] : 0ull;
                const uint64_t b = __ballot(v != 0);
                if (b)
                        prev = isect_shfl(v, isect_low(b));
        }
        const unsigned long long *hk = T.h_key + (size_t)r * T.h_cap;
        const uint32_t *bd = bounds + q.bounds_off;
        for (; live; live &= live - 1) {
                const uint32_t s = isect_low(live), d = (uint32_t)((w0 + s) * 64u) + lane;
                const uint64_t mask = isect_step_mask(rows, plw64, rt, q.nrows, w0 + s, lane);
                const bool ok = isect_considered(mask, q.orig_mask, q.stop_mask, masked, d);
                const uint64_t cons = __ballot(ok);
                if (!cons)
                        continue;
                // a considered lane's predecessor: the nearest lower considered lane, or the one the wave carries
                const uint64_t below = cons & ((1ull << lane) - 1ull);
                uint64_t pm = isect_shfl(mask, below ? isect_high(below) : 0u);
                if (!below)
                        pm = prev;
                const bool hit = ok && mask == pm;
                prev = isect_shfl(mask, isect_high(cons));
                uint64_t rem = __ballot(hit);
                while (rem) { // the step's distinct repeated masks
                        const uint32_t leader = isect_low(rem);
                        const uint64_t m0 = isect_shfl(mask, leader);
                        const uint64_t grp = __ballot(hit && mask == m0);
                        rem &= ~grp;
                        uint32_t slot = isect_hash(m0) % T.h_cap;
                        bool found = false;
                        for (uint32_t i = 0; i < T.h_cap; ++i) { // (wave-uniform; pass 1 put every considered mask there)
                                const unsigned long long k = hk[slot];
                                if (k == m0) {
                                        found = true;
                                        break;
                                }
                                if (k == 0ull)
                                        break;
                                slot = slot + 1u == T.h_cap ? 0u : slot + 1u;
                        }
                        if (!found)
                                continue;
                        const uint32_t t = thr[(size_t)r * T.h_cap + slot];
                        if (t == ISECT_NEVER)
                                continue;
                        const bool in = ((grp >> lane) & 1ull) && d >= t;
                        uint32_t e = 0;
                        if (in) { // epoch: the bounds at or below d
                                e = first_gt(bd, 0u, q.nbounds, d);
                        }
                        uint64_t rem2 = __ballot(in);
                        while (rem2) {
                                const uint32_t l2 = isect_low(rem2);
                                const uint32_t e0 = (uint32_t)__shfl((int)e, (int)l2, 64);
                                const uint64_t g2 = __ballot(in && e == e0);
                                rem2 &= ~g2;
                                if (lane == l2)
                                        isect_c_add(T, r, ((uint64_t)slot << 32) | e0, (uint32_t)__popcll(g2));
                        }
                }
        }
}

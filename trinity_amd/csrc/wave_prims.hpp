// wave_prims.hpp — what a wave does as one: readfirstlane pinning, the hardware lane number, the DPP prefix sums, the persistent kernels' task draw.
// Part of libtrinity_hip.so (MI355X / gfx950); included by k_match.hpp.  New code, no reference source.
//
// THE CONTRACT of everything below: wave64, and EVERY LANE ACTIVE at the call (uniform control flow).  The DPP prefixes are wrong otherwise — row_shr with
// bound_ctrl reads 0 from a disabled lane, row_bcast skips disabled lanes — and the draw would add less than 64 to its ticket word.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

// (row_shr / row_bcast:15 / row_bcast:31 are gfx9 DPP controls: gfx10 and later have no row_bcast.  The device pass only: the host pass defines no arch macro)
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__GFX9__)
#error "wave_prims.hpp: the DPP prefix sums are written for gfx9 (wave64, row_bcast)"
#endif

// Values that are workgroup-uniform by construction but read back from LDS look divergent to the compiler; a
// loop whose exit depends on one gets exec-masked structurisation, which is fatal around s_barrier (lanes
// "leave" the loop at different times).  uni() pins such values into an SGPR so the branch is scalar.
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// The lane's number in its wave, from the hardware lane count (nothing to keep in a register — or to spill — across calls: k_fused's sweep).
__device__ __forceinline__ uint32_t lane_id() {
        uint32_t l;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
        return l;
}

// Exclusive prefix sum across the wave's 64 lanes and the wave's total.  Six DPP adds — within each row of 16 lanes by row_shr:1 / 2 / 4 / 8, then
// row_bcast:15 carries rows 0 / 2's sums into rows 1 / 3 and row_bcast:31 the lower half's into the upper — and a v_readlane: no LDS crossbar trips (until round 6 this was
// six __shfl_up steps: a ds_bpermute_b32 and an s_waitcnt lgkmcnt(0) each, a chain of seven LDS round trips per scan in k_psets' / k_and's inner loops).
__device__ __forceinline__ uint32_t wave_excl_scan(uint32_t v, uint32_t &total) {
        uint32_t x = v;
        // (written out: left to the compiler, an update_dpp + add pair became v_mov 0 / v_mov_dpp / v_add — eighteen instructions — where registers were tight.  A VALU
        //  result read by a DPP instruction wants two wait states: the s_nop 1 between them; the ones at the ends stand for what the compiler cannot see into)
        asm volatile("s_nop 1\n\t"
                     "v_add_u32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "s_nop 1\n\t"
                     "v_add_u32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "s_nop 1\n\t"
                     "v_add_u32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "s_nop 1\n\t"
                     "v_add_u32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "s_nop 1\n\t"
                     "v_add_u32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                     "s_nop 1\n\t"
                     "v_add_u32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
                     "s_nop 1"
                     : "+v"(x));
        total = (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
        return x - v;
}

// Inclusive prefix sum over the first 8 lanes of every row of 16 (lanes 8 .. 15 of a row go on summing what they hold): the first three steps of the scan above.
__device__ __forceinline__ uint32_t row8_incl_scan(uint32_t v) {
        asm volatile("s_nop 1\n\t"
                     "v_add_u32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "s_nop 1\n\t"
                     "v_add_u32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "s_nop 1\n\t"
                     "v_add_u32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "s_nop 1"
                     : "+v"(v));
        return v;
}

// A persistent kernel's next task: wave 0's 64 lanes add 1 each (ONE +64 atomic — no single-lane branch), the number crosses through bcast[0], and the second
// barrier keeps the next draw's store behind every wave's read.  Returns the ticket number, uniform across the workgroup; the caller tests it against its task count.
// `wave` is the caller's uni(threadIdx.x >> 6).
__device__ __forceinline__ uint32_t draw_task(uint32_t *bcast, uint32_t *__restrict__ ticket, const uint32_t wave) {
        if (wave == 0) {
                const uint32_t old = atomicAdd(ticket, 1u);
                bcast[0] = uni(old) >> 6;
        }
        __syncthreads();
        const uint32_t ticket_no = uni(bcast[0]);
        __syncthreads();
        return ticket_no;
}

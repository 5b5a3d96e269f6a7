// filtered_kernels.hpp — the persistent matching kernels as a batch WITH per-query document filters runs them (k_filter.hpp): compiled in a translation unit of
// their own, filtered_kernels.hip, so that the kernels of trinity_hip.hip stay the code they were.  Part of libtrinity_hip.so (MI355X / gfx950).  New code, no reference source.
#pragma once

enum FilteredKernelId { FK_AND_DENSE, FK_AND, FK_PSETS, FK_PROBE, FK_FUSED /* variant: 0 32-bit words, 1 16-bit, 2 general trees */, FK_PLANES /* variant: 1 = wide */ };
// the kernel's launch handle (what hipLaunchKernelGGL takes): the plain kernel's signature with a FilterSel behind it (trinity_hip.hip: tri_launch_matching)
__attribute__((visibility("hidden"))) const void *filtered_kernel(int kernel, int codec, int variant);

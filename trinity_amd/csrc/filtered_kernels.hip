// filtered_kernels.hip — libtrinity_hip.so: k_and_dense, k_and, k_psets, k_probe, k_fused and k_planes for batches whose queries name document filters
// (tri_batch_set_filters).  The kernel headers once more, inside a namespace, with TRI_FILTERED_KERNELS defined: every kernel takes a FilterSel behind its
// arguments and, at the top of each task, swaps the index's masked-documents bitmap for the task's own row (k_filter.hpp says why this is a second
// translation unit and not a second instantiation).  New code, no reference source.
#include "../../include/trinity_hip.h"
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "dev_structs.hpp"
#include "filtered_kernels.hpp"

#define TRI_FILTERED_KERNELS 1
namespace filtered {
#include "k_planes.hpp" // (-> k_fused.hpp -> k_score.hpp -> k_match.hpp -> k_filter.hpp, the codec streams)
#include "k_psets.hpp"
#include "k_probe.hpp"
} // namespace filtered

const void *filtered_kernel(const int kernel, const int codec, const int variant) {
        using namespace filtered;
        const bool lucene = codec == CODEC_LUCENE;
#define BY_CODEC(K, ...) (lucene ? (const void *)&K<CODEC_LUCENE __VA_ARGS__> : (const void *)&K<CODEC_GOOGLE __VA_ARGS__>)
        switch (kernel) {
        case FK_AND_DENSE:
                return BY_CODEC(k_and_dense);
        case FK_AND:
                return BY_CODEC(k_and);
        case FK_PSETS:
                return BY_CODEC(k_psets);
        case FK_PROBE:
                return BY_CODEC(k_probe);
        case FK_FUSED:
                return variant == 0 ? BY_CODEC(k_fused, , 0, 0) : variant == 1 ? BY_CODEC(k_fused, , 1, 0) : BY_CODEC(k_fused, , 0, 1);
        case FK_PLANES:
                return variant ? BY_CODEC(k_planes, , FUS_MAX_SLOTS) : BY_CODEC(k_planes, , PLK_NS_SMALL);
        }
#undef BY_CODEC
        return nullptr;
}

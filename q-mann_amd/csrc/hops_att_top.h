// hops_att_top.h -- what every attended-slots build of a shared-plane or float kernel takes and every such call checks
// (hops_attended.h, hops_attended_float.h).
#pragma once
#include "hops_common.h"

namespace {

// launch argument of the kernels' TOP builds; the other builds take an EMPTY one and keep their device code
template <bool TOP> struct AttTop {};
template <> struct AttTop<true> {
    uint32_t *slot;          // [n_query][n_hop][k]
    float *p;                // [n_query][n_hop][k]
    uint32_t k;              // 1 .. QMANN_MAX_TOP_SLOTS
};

__device__ __forceinline__ float att_key(float p) { return p == p ? p : -INFINITY; }

// what both top calls refuse beyond their base calls
inline bool att_top_args_ok(uint32_t k, const uint32_t *top_slot, const float *top_p)
{
    return k >= 1 && k <= (uint32_t)QMANN_MAX_TOP_SLOTS && top_slot && top_p;
}

}  // namespace

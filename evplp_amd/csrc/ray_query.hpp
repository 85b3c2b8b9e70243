// Ray queries (evplp_trace_closest / evplp_trace_occluded): the argument block of the two kernels and of the ordering pass, and their
// launchers (kernels_query.hip).  A launch takes at most kQueryChunk rays: that bounds the host forms' staging and the ordering pass's
// arrays for any batch (include/evplp.h EVPLP_QUERY_CHUNK_RAYS).
#pragma once
#include "evplp_types.h"

namespace evplp {

constexpr int32_t kQueryChunk = EVPLP_QUERY_CHUNK_RAYS;
static_assert(sizeof(evplp_ray) == 32 && sizeof(evplp_hit) == 16, "the kernels move a ray as two float4 and a hit as one");

struct QueryArgs {
    SceneDev sc;
    const evplp_ray *rays;        // [n]
    const uint32_t *order;        // [n] lane i traces ray order[i] (the ordering pass), or null: ray i
    int32_t n, filter;
    evplp_hit *hits;              // [n] closest hit: written at the ray's own index
    uint8_t *occluded;            // [n] occlusion: likewise
};
// dynamic LDS of both kernels: the full [entry][lane] stack of the four-wide walk over the tree that was built (kernels.h lane_stack_bytes4)
size_t query_stack_bytes(const SceneDev &sc);
void launch_ray_closest(const QueryArgs &a, hipStream_t s);
void launch_ray_occluded(const QueryArgs &a, hipStream_t s);
// The ordering pass over n <= kQueryChunk rays: keys (the origin's 27-bit Morton code in the box lo .. lo + 1 / inv, the direction's octant
// in the three low bits) and indices into keys / index, then the radix sort into keys_sorted / index_sorted through `temp`.
// query_sort_temp_bytes: what the sort wants for kQueryChunk pairs.
struct QuerySortArrays { uint32_t *keys, *keys_sorted, *index, *index_sorted; void *temp; size_t temp_bytes; };
size_t query_sort_temp_bytes();
hipError_t launch_ray_order(const evplp_ray *rays, int32_t n, const float lo[3], const float inv[3], const QuerySortArrays &w, hipStream_t s);

}

// Ray queries: a caller's own rays against the scene's tree (evplp_trace_closest / evplp_trace_occluded, ray_query.cpp).
//   ray_closest_kernel   <- the closest-hit program as a free-standing batch: closest_lane4 with the far-origin slack (FAR)
//   ray_occluded_kernel  <- the any-hit program likewise: occluded_lane4 with FAR
//   ray_key_kernel       <- the ordering pass's keys (EVPLP_QUERY_ORDER)
// One ray per lane; nothing is known about the rays of a wave, so both walks are the per-lane four-wide ones with the full [entry][lane]
// LDS stack of the tree that was built (kernels.h lane_stack_bytes4).  The unit is built without floating-point contraction, as
// kernels_trace.hip is: t, beta and gamma are the oracle's bits.
#include "device_common.hpp"
#include "kernels.h"
#include "ray_query.hpp"

#include <hipcub/hipcub.hpp>

namespace evplp {

#ifndef EVPLP_QUERY_WAVES
#define EVPLP_QUERY_WAVES 8      // 64 registers per lane: the kernels take 62 and 54 and spill nothing (tests/test_ray_query_resources.py holds the counts)
#endif
#ifndef EVPLP_QUERY_SPEC
#define EVPLP_QUERY_SPEC 1       // light tracing's setting of the same walk (kernels_trace.hip EVPLP_LT_SPEC)
#endif

struct QueryRay { V3 o, d; float tmin, tmax; };
EV_DEV QueryRay load_ray(const evplp_ray *rays, uint32_t r) {
    const float4 *p = reinterpret_cast<const float4 *>(rays + r);
    const float4 a = p[0], b = p[1];
    QueryRay q; q.o = v3(a.x, a.y, a.z); q.tmin = a.w; q.d = v3(b.x, b.y, b.z); q.tmax = b.w;
    return q;
}
EV_DEV bool is_finite(float x) { return fabsf(x) <= 3.4028235e38f; }      // (false for a NaN)
// what evplp.h calls an invalid ray: such a ray is never walked.  The direction's largest component must lie in [2^-64, 2^64] (which a
// direction of three zeros does not): the walks' reciprocal replaces a component below 1e-30 by 1e-30, and only above 2^-64 is that a turn of the
// direction by less than 1e-30 / 2^-64 = 1.9e-11, which the boxes' pad absorbs; at 2^-100 it would be every component
EV_DEV bool ray_valid(const QueryRay &q) {
    const bool finite = is_finite(q.o.x) && is_finite(q.o.y) && is_finite(q.o.z) && is_finite(q.d.x) && is_finite(q.d.y) && is_finite(q.d.z) && is_finite(q.tmin) && is_finite(q.tmax);
    const float largest = fmaxf(fmaxf(fabsf(q.d.x), fabsf(q.d.y)), fabsf(q.d.z));
    const bool in_range = largest >= 0x1p-64f && largest <= 0x1p64f;
    return finite && in_range && !(q.tmin > q.tmax);
}

__global__ __launch_bounds__(64, EVPLP_QUERY_WAVES) void ray_closest_kernel(QueryArgs a) {
    extern __shared__ int32_t lds_stack[];   // [query_stack_bytes / 256][64 lanes]
    const int lane = threadIdx.x;
    const uint32_t i = blockIdx.x * 64u + lane;
    if (i >= (uint32_t)a.n) return;
    const uint32_t r = a.order ? a.order[i] : i;
    const QueryRay q = load_ray(a.rays, r);
    float4 *out = reinterpret_cast<float4 *>(a.hits + r);
    if (!ray_valid(q)) { *out = make_float4(0.f, 0.f, 0.f, __int_as_float(-2)); return; }
    float t = q.tmax, b = 0.f, g = 0.f;
    const int32_t tri = closest_lane4<64, 0, EVPLP_QUERY_SPEC, true, true>(a.sc, q.o, q.d, q.tmin, q.tmax, a.filter, t, b, g, lds_stack + lane);
    *out = make_float4(t, b, g, __int_as_float(tri));        // (a miss: tmax, 0, 0, -1 -- the walk leaves t, b, g alone)
}

__global__ __launch_bounds__(64, EVPLP_QUERY_WAVES) void ray_occluded_kernel(QueryArgs a) {
    extern __shared__ int32_t lds_stack[];
    const int lane = threadIdx.x;
    const uint32_t i = blockIdx.x * 64u + lane;
    if (i >= (uint32_t)a.n) return;
    const uint32_t r = a.order ? a.order[i] : i;
    const QueryRay q = load_ray(a.rays, r);
    if (!ray_valid(q)) { a.occluded[r] = 2; return; }
    a.occluded[r] = occluded_lane4<64, EVPLP_QUERY_SPEC, true>(a.sc, q.o, q.d, q.tmin, q.tmax, lds_stack + lane) ? 1 : 0;
}

// 27-bit Morton code of the origin in the scene's box (9 bits per axis), the direction's octant below it.  An origin outside the box, or
// one that is not a number, lands on the box's border: the key only orders the launch.
EV_DEV uint32_t spread9(uint32_t v) {
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
EV_DEV uint32_t cell9(float x, float lo, float inv) { return (uint32_t)fminf(fmaxf((x - lo) * inv * 512.0f, 0.0f), 511.0f); }
struct KeyArgs { const evplp_ray *rays; int32_t n; float lo[3], inv[3]; uint32_t *keys, *index; };
__global__ __launch_bounds__(256) void ray_key_kernel(KeyArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint32_t)a.n) return;
    const QueryRay q = load_ray(a.rays, i);
    const uint32_t m = spread9(cell9(q.o.x, a.lo[0], a.inv[0])) | (spread9(cell9(q.o.y, a.lo[1], a.inv[1])) << 1) | (spread9(cell9(q.o.z, a.lo[2], a.inv[2])) << 2);
    const uint32_t oct = (q.d.x < 0.0f ? 1u : 0u) | (q.d.y < 0.0f ? 2u : 0u) | (q.d.z < 0.0f ? 4u : 0u);
    a.keys[i] = (m << 3) | oct;
    a.index[i] = i;
}
constexpr int kQueryKeyBits = 30;

size_t query_stack_bytes(const SceneDev &sc) { return lane_stack_bytes4(sc); }
void launch_ray_closest(const QueryArgs &a, hipStream_t s) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL(ray_closest_kernel, dim3((uint32_t)(a.n + 63) / 64u), dim3(64), query_stack_bytes(a.sc), s, a);
}
void launch_ray_occluded(const QueryArgs &a, hipStream_t s) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL(ray_occluded_kernel, dim3((uint32_t)(a.n + 63) / 64u), dim3(64), query_stack_bytes(a.sc), s, a);
}
size_t query_sort_temp_bytes() {
    size_t need = 0;
    uint32_t *none = nullptr;
    if (hipcub::DeviceRadixSort::SortPairs(nullptr, need, none, none, none, none, kQueryChunk, 0, kQueryKeyBits, (hipStream_t) nullptr) != hipSuccess) return 0;
    return need;
}
hipError_t launch_ray_order(const evplp_ray *rays, int32_t n, const float lo[3], const float inv[3], const QuerySortArrays &w, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (n > kQueryChunk) return hipErrorInvalidValue;
    KeyArgs k; k.rays = rays; k.n = n; k.keys = w.keys; k.index = w.index;
    for (int c = 0; c < 3; c++) { k.lo[c] = lo[c]; k.inv[c] = inv[c]; }
    hipLaunchKernelGGL(ray_key_kernel, dim3((uint32_t)(n + 255) / 256u), dim3(256), 0, s, k);
    size_t bytes = w.temp_bytes;
    return hipcub::DeviceRadixSort::SortPairs(w.temp, bytes, w.keys, w.keys_sorted, w.index, w.index_sorted, n, 0, kQueryKeyBits, s);
}

} // namespace evplp

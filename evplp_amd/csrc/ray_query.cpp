// Ray queries (include/evplp.h "ray queries"): the host side of evplp_trace_closest / evplp_trace_occluded, their device forms and
// evplp_triangle_info.  A batch runs as launches of at most kQueryChunk rays (ray_query.hpp), so the staging of the host forms and the
// arrays of the ordering pass have one size whatever n is; the kernels and the sort are in kernels_query.hip.
#include "context.hpp"

#include <algorithm>
#include <cstring>

using namespace evplp;

namespace {
constexpr size_t kStageRays = sizeof(evplp_ray) * (size_t)kQueryChunk;              // the staged rays; the results lie behind them
constexpr size_t kStageBytes = kStageRays + sizeof(evplp_hit) * (size_t)kQueryChunk;
constexpr size_t kSortArrays = 4 * sizeof(uint32_t) * (size_t)kQueryChunk;          // keys, sorted keys, indices, sorted indices
// the largest dynamic LDS a workgroup may ask for without an attribute of its own; the walks' worst case (kMaxDepth levels) is 25 KB
constexpr size_t kMaxStackBytes = 64 * 1024;

int oom_or_hip(hipError_t e) { return e == hipErrorOutOfMemory ? EVPLP_ERR_OOM : EVPLP_ERR_HIP; }

// the host forms' staging, on the device and pinned
int stage_arrays(evplp_context *c, const char *name) {
    hipError_t e = grow_scratch_of(c, c->query_stage, kStageBytes);
    if (e == hipSuccess && !c->h_query_stage) {
        e = hipHostMalloc((void **)&c->h_query_stage, kStageBytes, hipHostMallocDefault);
        if (e != hipSuccess) { (void)hipGetLastError(); c->h_query_stage = nullptr; }
    }
    if (e != hipSuccess) { c->set_error("%s: cannot allocate the staging of %d rays (%zu bytes): %s", name, kQueryChunk, kStageBytes, hipGetErrorString(e)); return oom_or_hip(e); }
    return EVPLP_OK;
}
// the ordering pass's arrays and the sort's workspace
int sort_arrays(evplp_context *c, const char *name, QuerySortArrays *w) {
    if (c->query_sort_temp == 0) c->query_sort_temp = query_sort_temp_bytes();
    if (c->query_sort_temp == 0) { (void)hipGetLastError(); c->set_error("%s: the radix sort states no workspace size", name); return EVPLP_ERR_HIP; }
    const hipError_t e = grow_scratch_of(c, c->query_sort, kSortArrays + c->query_sort_temp);
    if (e != hipSuccess) { c->set_error("%s: cannot allocate the ordering pass's %zu bytes: %s", name, kSortArrays + c->query_sort_temp, hipGetErrorString(e)); return oom_or_hip(e); }
    uint32_t *p = (uint32_t *)c->query_sort.p;
    w->keys = p; w->keys_sorted = p + kQueryChunk; w->index = p + 2 * (size_t)kQueryChunk; w->index_sorted = p + 3 * (size_t)kQueryChunk;
    w->temp = (char *)c->query_sort.p + kSortArrays; w->temp_bytes = c->query_sort_temp;
    return EVPLP_OK;
}
// the box the keys quantise origins to: the meshes' vertices as the host copy holds them (a refit keeps the figures current)
void scene_box(const evplp_context *c, float lo[3], float inv[3]) {
    float hi[3];
    for (int k = 0; k < 3; k++) { lo[k] = 3.0e38f; hi[k] = -3.0e38f; }
    for (const HostMesh &m : c->meshes) for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], m.lo[k]); hi[k] = std::max(hi[k], m.hi[k]); }
    for (int k = 0; k < 3; k++) { const float ext = hi[k] - lo[k]; inv[k] = ext > 0.0f && ext < 3.0e38f ? 1.0f / ext : 0.0f; if (!(lo[k] < 3.0e38f)) lo[k] = 0.0f; }
}

// one batch, chunk by chunk.  device: rays / out are device pointers and nothing waits; else they are staged and every chunk is waited for.
int trace(evplp_context *c, const char *name, bool closest, bool device, const void *rays, int32_t n, int32_t filter, int32_t flags, void *out) {
    if (!ray_query_check(c, name, rays, n, filter, flags, out)) return EVPLP_ERR_INVALID;
    if (n == 0) return EVPLP_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const size_t lds = query_stack_bytes(c->sc);
    if (lds > kMaxStackBytes) { c->set_error("%s: the walk's stack of this tree (%zu bytes per wave) exceeds a workgroup's LDS", name, lds); return EVPLP_ERR_INVALID; }
    int rc;
    if (!device && (rc = stage_arrays(c, name))) return rc;
    const bool order = (flags & EVPLP_QUERY_ORDER) != 0;
    QuerySortArrays sort{}; float lo[3], inv[3];
    if (order) { if ((rc = sort_arrays(c, name, &sort))) return rc; scene_box(c, lo, inv); }
    const size_t out_size = closest ? sizeof(evplp_hit) : sizeof(uint8_t);
    for (int64_t at = 0; at < n; at += kQueryChunk) {
        const int32_t m = (int32_t)std::min<int64_t>(kQueryChunk, n - at);
        QueryArgs a; std::memset(&a, 0, sizeof(a));
        a.sc = c->sc; a.n = m; a.filter = filter;
        void *d_out;
        if (device) { a.rays = (const evplp_ray *)rays + at; d_out = (char *)out + out_size * (size_t)at; }
        else {
            std::memcpy(c->h_query_stage, (const evplp_ray *)rays + at, sizeof(evplp_ray) * (size_t)m);
            HIP_TRY(c, hipMemcpyAsync(c->query_stage.p, c->h_query_stage, sizeof(evplp_ray) * (size_t)m, hipMemcpyHostToDevice, c->stream));
            a.rays = (const evplp_ray *)c->query_stage.p; d_out = (char *)c->query_stage.p + kStageRays;
        }
        if (order) { HIP_TRY(c, launch_ray_order(a.rays, m, lo, inv, sort, c->stream)); a.order = sort.index_sorted; }
        if (closest) { a.hits = (evplp_hit *)d_out; launch_ray_closest(a, c->stream); }
        else { a.occluded = (uint8_t *)d_out; launch_ray_occluded(a, c->stream); }
        HIP_TRY(c, hipGetLastError());
        if (!device) {
            HIP_TRY(c, hipMemcpyAsync(c->h_query_stage + kStageRays, d_out, out_size * (size_t)m, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            std::memcpy((char *)out + out_size * (size_t)at, c->h_query_stage + kStageRays, out_size * (size_t)m);
        }
    }
    return EVPLP_OK;
}
}

namespace evplp {
bool ray_query_check(evplp_context *c, const char *name, const void *rays, int32_t n, int32_t filter, int32_t flags, const void *out) {
    if (!c->accel_built) { c->set_error("%s: scene not built (evplp_build_accel)", name); return false; }
    if (c->scene_dirty) { c->set_error("%s: vertices were updated (evplp_update_mesh): call evplp_refit_accel or evplp_build_accel first", name); return false; }
    if (n < 0) { c->set_error("%s: n = %d is negative", name, n); return false; }
    if (n > 0 && (!rays || !out)) { c->set_error("%s: null %s with n = %d", name, !rays ? "rays" : "destination", n); return false; }
    if (filter < 0 || filter > 2) { c->set_error("%s: filter %d is not 0 (all), 1 (without the light mesh) or 2 (the light mesh only)", name, filter); return false; }
    if (flags & ~EVPLP_QUERY_ORDER) { c->set_error("%s: unknown flag bits 0x%x", name, (unsigned)(flags & ~EVPLP_QUERY_ORDER)); return false; }
    return true;
}
void release_ray_query(evplp_context *c) {
    hipFree(c->query_stage.p); hipFree(c->query_sort.p); c->query_stage = DeviceScratch(); c->query_sort = DeviceScratch();
    if (c->h_query_stage) hipHostFree(c->h_query_stage);
    c->h_query_stage = nullptr;
}
}

extern "C" int evplp_trace_closest(evplp_context *c, const evplp_ray *rays, int32_t n, int32_t filter, int32_t flags, evplp_hit *hits) {
    CTX_CHECK(c);
    return trace(c, "evplp_trace_closest", true, false, rays, n, filter, flags, hits);
}
extern "C" int evplp_trace_occluded(evplp_context *c, const evplp_ray *rays, int32_t n, int32_t flags, uint8_t *out) {
    CTX_CHECK(c);
    return trace(c, "evplp_trace_occluded", false, false, rays, n, 0, flags, out);
}
extern "C" int evplp_trace_closest_device(evplp_context *c, const void *d_rays, int32_t n, int32_t filter, int32_t flags, void *d_hits) {
    CTX_CHECK(c);
    return trace(c, "evplp_trace_closest_device", true, true, d_rays, n, filter, flags, d_hits);
}
extern "C" int evplp_trace_occluded_device(evplp_context *c, const void *d_rays, int32_t n, int32_t flags, void *d_out) {
    CTX_CHECK(c);
    return trace(c, "evplp_trace_occluded_device", false, true, d_rays, n, 0, flags, d_out);
}
extern "C" int evplp_triangle_info(evplp_context *c, int32_t triangle, int32_t *mesh, int32_t *index_in_mesh) {
    CTX_CHECK(c);
    if (!c->accel_built) { c->set_error("evplp_triangle_info: scene not built (evplp_build_accel)"); return EVPLP_ERR_INVALID; }
    int64_t first = 0;
    for (size_t mi = 0; mi < c->meshes.size(); mi++) {
        const int64_t count = (int64_t)(c->meshes[mi].idx.size() / 3);
        if (triangle >= first && triangle < first + count) { if (mesh) *mesh = (int32_t)mi; if (index_in_mesh) *index_in_mesh = (int32_t)(triangle - first); return EVPLP_OK; }
        first += count;
    }
    c->set_error("evplp_triangle_info: triangle %d is outside the scene's %lld triangles", triangle, (long long)first);
    return EVPLP_ERR_INVALID;
}

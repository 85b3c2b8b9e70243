// Lightmap baking (include/evplp.h "lightmap baking"): the host side of evplp_surface_points, evplp_lightmap_samples, evplp_bake_lightmap
// and their device forms.  The points run as launches of at most kQueryChunk hits, as the ray queries that make hits do.  The atlas runs as
// bands of whole texel rows holding at most kLightmapChunk samples (EVPLP_LIGHTMAP_BAND in the environment lowers that, for the tests: the
// results do not depend on it): per band the tiles' triangle counts, their exclusive sum, ONE read-back of the total to size the lists --
// both forms wait there -- then the fill and the raster.  The bake chains, per band, raster -> points -> evplp_gather_surface_device ->
// resolve, and ends with the gutter passes over the whole atlas.  The kernels are in kernels_lightmap.hip, the integers in lightmap_raster.h.
// The progressive bake chains raster -> points -> evplp_gather_surface_progressive_device per band into the caller's states; its resolve
// reads the states alone (kernels_surface_prog.hip) and ends with the same gutter passes.  evplp_bake_lightmap_knn_device is the same
// chain with evplp_gather_surface_knn_device in the gather's place.
#include "context.hpp"
#include "lightmap.hpp"
#include "surface_gather.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>

using namespace evplp;

namespace {
// the host forms' staging for one chunk: hits, the eyes behind them, the points behind those (a band's hits fit the first part)
constexpr size_t kStageHits = sizeof(evplp_hit) * (size_t)kQueryChunk;
constexpr size_t kStageEyes = 3 * sizeof(float) * (size_t)kQueryChunk;
constexpr size_t kStageBytes = kStageHits + kStageEyes + sizeof(evplp_surface_point) * (size_t)kQueryChunk;
static_assert((kStageHits + kStageEyes) % 16 == 0 && kLightmapChunk <= kQueryChunk, "the staged points are written as float4; a band's hits fit a chunk's");
constexpr size_t kMaxStackBytes = 64 * 1024;       // as surface_gather.cpp

int oom_or_hip(hipError_t e) { return e == hipErrorOutOfMemory ? EVPLP_ERR_OOM : EVPLP_ERR_HIP; }
size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

int stage_arrays(evplp_context *c, const char *name) {
    hipError_t e = grow_scratch_of(c, c->lm_stage, kStageBytes);
    if (e == hipSuccess && !c->h_lm_stage) {
        e = hipHostMalloc((void **)&c->h_lm_stage, kStageBytes, hipHostMallocDefault);
        if (e != hipSuccess) { (void)hipGetLastError(); c->h_lm_stage = nullptr; }
    }
    if (e != hipSuccess) { c->set_error("%s: cannot allocate the staging of %d hits (%zu bytes): %s", name, kQueryChunk, kStageBytes, hipGetErrorString(e)); return oom_or_hip(e); }
    return EVPLP_OK;
}

// ---------------------------------------------------------------------------------------------------------------- points
bool points_check(evplp_context *c, const char *name, bool device, const void *hits, int32_t n, uint32_t flags, const void *eyes, const void *out) {
    if (!ray_query_check(c, name, hits, n, 0, 0, out)) return false;
    if (flags & ~(EVPLP_POINTS_WHITE | EVPLP_POINTS_FACE_EYES)) { c->set_error("%s: unknown flag bits 0x%x", name, (unsigned)(flags & ~(EVPLP_POINTS_WHITE | EVPLP_POINTS_FACE_EYES))); return false; }
    if ((flags & EVPLP_POINTS_FACE_EYES) && !eyes && n > 0) { c->set_error("%s: EVPLP_POINTS_FACE_EYES without eyes", name); return false; }
    if (device && n > 0 && ((((uintptr_t)out) | ((uintptr_t)hits)) & 15u) != 0) { c->set_error("%s: the hits or the destination are not 16-byte aligned", name); return false; }
    return true;
}
PointsArgs points_args(const evplp_context *c, const void *d_hits, const float *d_eyes, void *d_out, int32_t n, uint32_t flags) {
    PointsArgs a; std::memset(&a, 0, sizeof(a));
    a.sc = c->sc; a.hits = (const evplp_hit *)d_hits; a.eyes = (flags & EVPLP_POINTS_FACE_EYES) ? d_eyes : nullptr; a.out = (float4 *)d_out;
    a.n = n; a.ntris = c->scene_tris; a.flags = flags;
    return a;
}
int points(evplp_context *c, const char *name, bool device, const void *hits, int32_t n, uint32_t flags, const float *eyes, void *out) {
    if (!points_check(c, name, device, hits, n, flags, eyes, out)) return EVPLP_ERR_INVALID;
    if (n == 0) return EVPLP_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int rc;
    if (!device && (rc = stage_arrays(c, name))) return rc;
    const bool face = (flags & EVPLP_POINTS_FACE_EYES) != 0u;
    for (int64_t at = 0; at < n; at += kQueryChunk) {
        const int32_t m = (int32_t)std::min<int64_t>(kQueryChunk, n - at);
        if (device) {
            launch_lightmap_points(points_args(c, (const evplp_hit *)hits + at, face ? eyes + 3 * (size_t)at : nullptr, (evplp_surface_point *)out + at, m, flags), c->stream);
            HIP_TRY(c, hipGetLastError());
            continue;
        }
        char *h = c->h_lm_stage, *d = (char *)c->lm_stage.p;
        std::memcpy(h, (const evplp_hit *)hits + at, sizeof(evplp_hit) * (size_t)m);
        HIP_TRY(c, hipMemcpyAsync(d, h, sizeof(evplp_hit) * (size_t)m, hipMemcpyHostToDevice, c->stream));
        if (face) {
            std::memcpy(h + kStageHits, eyes + 3 * (size_t)at, 3 * sizeof(float) * (size_t)m);
            HIP_TRY(c, hipMemcpyAsync(d + kStageHits, h + kStageHits, 3 * sizeof(float) * (size_t)m, hipMemcpyHostToDevice, c->stream));
        }
        launch_lightmap_points(points_args(c, d, (const float *)(d + kStageHits), d + kStageHits + kStageEyes, m, flags), c->stream);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(h + kStageHits + kStageEyes, d + kStageHits + kStageEyes, sizeof(evplp_surface_point) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        std::memcpy((evplp_surface_point *)out + at, h + kStageHits + kStageEyes, sizeof(evplp_surface_point) * (size_t)m);
    }
    return EVPLP_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the rasteriser
bool atlas_check(evplp_context *c, const char *name, int32_t mesh, int32_t width, int32_t height, int32_t samples, int32_t *first, int32_t *count) {
    if (!c->accel_built) { c->set_error("%s: scene not built (evplp_build_accel)", name); return false; }
    if (c->scene_dirty) { c->set_error("%s: vertices were updated (evplp_update_mesh): call evplp_refit_accel or evplp_build_accel first", name); return false; }
    if (mesh < -1 || mesh >= (int32_t)c->meshes.size()) { c->set_error("%s: mesh %d is not -1 or one of the scene's %zu meshes", name, mesh, c->meshes.size()); return false; }
    if (width < 1 || width > LM_MAX_SIZE || height < 1 || height > LM_MAX_SIZE) { c->set_error("%s: an atlas of %d x %d is not within 1 .. %d", name, width, height, LM_MAX_SIZE); return false; }
    if (samples != 1 && samples != 2 && samples != 4) { c->set_error("%s: %d samples per axis is not 1, 2 or 4", name, samples); return false; }
    int64_t f = 0;
    for (int32_t mi = 0; mi < mesh; mi++) f += (int64_t)(c->meshes[(size_t)mi].idx.size() / 3);
    *first = mesh < 0 ? 0 : (int32_t)f;
    *count = mesh < 0 ? c->scene_tris : (int32_t)(c->meshes[(size_t)mesh].idx.size() / 3);
    return true;
}
// texel rows per band: whole rows holding at most the chunk's samples (a row of the widest atlas at 4 x 4 samples fits: lightmap.hpp)
int32_t band_rows(int32_t width, int32_t samples) {
    int64_t limit = kLightmapChunk;
    if (const char *env = std::getenv("EVPLP_LIGHTMAP_BAND")) { const long v = std::strtol(env, nullptr, 10); if (v >= 1 && v <= (long)kLightmapChunk) limit = v; }
    return (int32_t)std::max<int64_t>(1, limit / ((int64_t)width * samples * samples));
}
struct Raster { RasterArgs a; int32_t band; void *temp; size_t temp_bytes; };
// the selection set up on the device and the band's arrays.  uvs: null, a device pointer (device), or host memory (uploaded once, 24 B per triangle)
int raster_prepare(evplp_context *c, const char *name, bool device, int32_t first, int32_t count, const float *uvs, int32_t width, int32_t height, int32_t samples, Raster *r) {
    std::memset(r, 0, sizeof(*r));
    RasterArgs &a = r->a;
    a.attrs = c->sc.attrs; a.first = first; a.count = count; a.width = width; a.height = height; a.samples = samples;
    r->band = std::min(band_rows(width, samples), height);
    a.tiles_x = (width + kLightmapTile - 1) / kLightmapTile;
    const int32_t max_tiles = a.tiles_x * ((r->band + kLightmapTile - 1) / kLightmapTile);
    const size_t tris = align256(sizeof(lm_tri) * (size_t)std::max(count, 1)), given = uvs && !device ? align256(6 * sizeof(float) * (size_t)std::max(count, 1)) : 0;
    hipError_t e = grow_scratch_of(c, c->lm_tris, tris + given);
    if (e != hipSuccess) { c->set_error("%s: cannot allocate the set-up of %d triangles (%zu bytes): %s", name, count, tris + given, hipGetErrorString(e)); return oom_or_hip(e); }
    r->temp_bytes = lightmap_scan_temp_bytes(max_tiles);
    if (r->temp_bytes == 0) { (void)hipGetLastError(); c->set_error("%s: the exclusive sum states no workspace size", name); return EVPLP_ERR_HIP; }
    const size_t words = align256(sizeof(uint32_t) * ((size_t)max_tiles + 1));
    e = grow_scratch_of(c, c->lm_band, 3 * words + r->temp_bytes);
    if (e == hipSuccess && !c->h_lm_count) {
        e = hipHostMalloc((void **)&c->h_lm_count, 16, hipHostMallocDefault);
        if (e != hipSuccess) { (void)hipGetLastError(); c->h_lm_count = nullptr; }
    }
    if (e != hipSuccess) { c->set_error("%s: cannot allocate the arrays of %d tiles (%zu bytes): %s", name, max_tiles, 3 * words + r->temp_bytes, hipGetErrorString(e)); return oom_or_hip(e); }
    char *p = (char *)c->lm_band.p;
    a.counts = (uint32_t *)p; p += words; a.offsets = (uint32_t *)p; p += words; a.cursors = (uint32_t *)p; p += words;
    r->temp = p;
    a.tris = (lm_tri *)c->lm_tris.p;
    if (given) {
        float *d = (float *)((char *)c->lm_tris.p + tris);
        HIP_TRY(c, hipMemcpyAsync(d, uvs, 6 * sizeof(float) * (size_t)count, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));           // (the caller's memory is the caller's again)
        a.uvs = d;
    } else a.uvs = uvs;
    launch_lightmap_setup(a, c->stream);
    HIP_TRY(c, hipGetLastError());
    return EVPLP_OK;
}
// the samples of the texel rows [y0, y0 + rows) to d_out (enqueued, behind one wait for the band's pair count)
int raster_band(evplp_context *c, const char *name, Raster *r, int32_t y0, int32_t rows, evplp_hit *d_out) {
    RasterArgs &a = r->a;
    a.y0 = y0; a.rows = rows; a.tiles = a.tiles_x * ((rows + kLightmapTile - 1) / kLightmapTile); a.out = d_out;
    HIP_TRY(c, launch_lightmap_count(a, r->temp, r->temp_bytes, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->h_lm_count, a.offsets + a.tiles, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    a.pairs = *c->h_lm_count;
    const hipError_t e = grow_scratch_of(c, c->lm_pairs, sizeof(uint32_t) * (size_t)a.pairs);
    if (e != hipSuccess) { c->set_error("%s: cannot allocate the tiles' lists of %u (triangle, tile) pairs: %s", name, a.pairs, hipGetErrorString(e)); return oom_or_hip(e); }
    a.list = (uint32_t *)c->lm_pairs.p;
    launch_lightmap_fill_raster(a, c->stream);
    HIP_TRY(c, hipGetLastError());
    return EVPLP_OK;
}

int samples_call(evplp_context *c, const char *name, bool device, int32_t mesh, const float *uvs, int32_t width, int32_t height, int32_t samples, void *out) {
    int32_t first, count;
    if (!atlas_check(c, name, mesh, width, height, samples, &first, &count)) return EVPLP_ERR_INVALID;
    if (!out) { c->set_error("%s: null destination", name); return EVPLP_ERR_INVALID; }
    if (device && (((uintptr_t)out) & 15u) != 0) { c->set_error("%s: the destination is not 16-byte aligned", name); return EVPLP_ERR_INVALID; }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int rc;
    if (!device && (rc = stage_arrays(c, name))) return rc;
    Raster r;
    if ((rc = raster_prepare(c, name, device, first, count, uvs, width, height, samples, &r))) return rc;
    const size_t per_row = (size_t)width * samples * samples;
    for (int32_t y0 = 0; y0 < height; y0 += r.band) {
        const int32_t rows = std::min(r.band, height - y0);
        evplp_hit *dst = (evplp_hit *)out + per_row * (size_t)y0;
        if ((rc = raster_band(c, name, &r, y0, rows, device ? dst : (evplp_hit *)c->lm_stage.p))) return rc;
        if (!device) {
            const size_t bytes = sizeof(evplp_hit) * per_row * (size_t)rows;
            HIP_TRY(c, hipMemcpyAsync(c->h_lm_stage, c->lm_stage.p, bytes, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            std::memcpy(dst, c->h_lm_stage, bytes);
        }
    }
    return EVPLP_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the bake
int bake(evplp_context *c, const char *name, bool device, const evplp_frame_params *fp, uint32_t what, const evplp_lightmap_params *p, const float *uvs, void *out) {
    if (!p) { c->set_error("%s: null params", name); return EVPLP_ERR_INVALID; }
    int32_t first, count;
    if (!atlas_check(c, name, p->mesh, p->width, p->height, p->samples, &first, &count)) return EVPLP_ERR_INVALID;
    if (p->gutter < 0 || p->gutter > 8) { c->set_error("%s: a gutter of %d is not 0 .. 8", name, p->gutter); return EVPLP_ERR_INVALID; }
    if (p->flags & ~EVPLP_POINTS_WHITE) { c->set_error("%s: unknown flag bits 0x%x", name, (unsigned)(p->flags & ~EVPLP_POINTS_WHITE)); return EVPLP_ERR_INVALID; }
    if (!out) { c->set_error("%s: null destination", name); return EVPLP_ERR_INVALID; }
    if (device && (((uintptr_t)out) & 15u) != 0) { c->set_error("%s: the destination is not 16-byte aligned", name); return EVPLP_ERR_INVALID; }
    // what evplp_gather_surface refuses, before anything is written: its own checks on an empty batch, and the walk's stack
    int rc = evplp_gather_surface_device(c, fp, what, nullptr, nullptr, 0, nullptr);
    if (rc) return rc;
    if (surface_stack_bytes(c->sc) > kMaxStackBytes) { c->set_error("%s: the walk's stack of this tree (%zu bytes per wave) exceeds a workgroup's LDS", name, surface_stack_bytes(c->sc)); return EVPLP_ERR_INVALID; }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const int32_t W = p->width, H = p->height, S = p->samples, s2 = S * S;
    const size_t texels = (size_t)W * (size_t)H, atlas = align256(sizeof(evplp_lightmap_texel) * texels);
    // the atlas: the caller's (device form) or one of ours, and one more for the gutter's double buffering
    const int own = (device ? 0 : 1) + (p->gutter > 0 ? 1 : 0);
    hipError_t e = grow_scratch_of(c, c->lm_atlas, atlas * (size_t)own);
    if (e != hipSuccess) { c->set_error("%s: cannot allocate %d atlas buffers of %d x %d texels: %s", name, own, W, H, hipGetErrorString(e)); return oom_or_hip(e); }
    evplp_lightmap_texel *cur = device ? (evplp_lightmap_texel *)out : (evplp_lightmap_texel *)c->lm_atlas.p;
    evplp_lightmap_texel *other = p->gutter > 0 ? (evplp_lightmap_texel *)((char *)c->lm_atlas.p + (device ? 0 : atlas)) : nullptr;
    Raster r;
    if ((rc = raster_prepare(c, name, device, first, count, uvs, W, H, S, &r))) return rc;
    const size_t band_samples = (size_t)W * s2 * (size_t)r.band;
    const size_t hits_b = align256(sizeof(evplp_hit) * band_samples), points_b = align256(sizeof(evplp_surface_point) * band_samples), lights_b = align256(sizeof(evplp_surface_light) * band_samples);
    e = grow_scratch_of(c, c->lm_bake, hits_b + points_b + lights_b);
    if (e != hipSuccess) { c->set_error("%s: cannot allocate a band's %zu samples (%zu bytes): %s", name, band_samples, hits_b + points_b + lights_b, hipGetErrorString(e)); return oom_or_hip(e); }
    char *d_hits = (char *)c->lm_bake.p, *d_points = d_hits + hits_b, *d_lights = d_points + points_b;
    for (int32_t y0 = 0; y0 < H; y0 += r.band) {
        const int32_t rows = std::min(r.band, H - y0);
        const int32_t n = (int32_t)((size_t)W * s2 * (size_t)rows);
        if ((rc = raster_band(c, name, &r, y0, rows, (evplp_hit *)d_hits))) return rc;
        launch_lightmap_points(points_args(c, d_hits, nullptr, d_points, n, p->flags), c->stream);
        HIP_TRY(c, hipGetLastError());
        if ((rc = evplp_gather_surface_device(c, fp, what, d_points, nullptr, n, d_lights))) return rc;
        ResolveArgs ra; std::memset(&ra, 0, sizeof(ra));
        ra.points = (const float4 *)d_points; ra.lights = (const float4 *)d_lights; ra.out = cur + (size_t)W * (size_t)y0; ra.texels = W * rows; ra.s2 = s2;
        launch_lightmap_resolve(ra, c->stream);
        HIP_TRY(c, hipGetLastError());
    }
    for (int32_t d = 1; d <= p->gutter; d++) {
        GutterArgs g; g.from = cur; g.to = other; g.width = W; g.height = H; g.pass = d;
        launch_lightmap_gutter(g, c->stream);
        HIP_TRY(c, hipGetLastError());
        std::swap(cur, other);
    }
    if (device) {
        if (cur != out) HIP_TRY(c, hipMemcpyAsync(out, cur, sizeof(evplp_lightmap_texel) * texels, hipMemcpyDeviceToDevice, c->stream));
        return EVPLP_OK;
    }
    HIP_TRY(c, hipMemcpyAsync(out, cur, sizeof(evplp_lightmap_texel) * texels, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EVPLP_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the progressive bake
// one iteration over the atlas: per band raster -> points -> evplp_gather_surface_progressive_device on the band's slice of the states
// knn: the band's first photon half is evplp_gather_surface_knn_device's (what and alpha are then not read) instead of the progressive gather
int bake_progressive(evplp_context *c, const char *name, const evplp_frame_params *fp, uint32_t what, float alpha, const evplp_lightmap_params *p, const float *uvs, void *states, const evplp_knn_params *knn = nullptr) {
    const auto band_gather = [&](const void *d_points, int32_t n, void *band) {
        return knn ? evplp_gather_surface_knn_device(c, fp, knn, d_points, nullptr, n, band) : evplp_gather_surface_progressive_device(c, fp, what, alpha, d_points, nullptr, n, band);
    };
    if (!p) { c->set_error("%s: null params", name); return EVPLP_ERR_INVALID; }
    int32_t first, count;
    if (!atlas_check(c, name, p->mesh, p->width, p->height, p->samples, &first, &count)) return EVPLP_ERR_INVALID;
    // (params->gutter belongs to the resolve: not looked at here)
    if (p->flags & ~EVPLP_POINTS_WHITE) { c->set_error("%s: unknown flag bits 0x%x", name, (unsigned)(p->flags & ~EVPLP_POINTS_WHITE)); return EVPLP_ERR_INVALID; }
    if (!states) { c->set_error("%s: null states", name); return EVPLP_ERR_INVALID; }
    if ((((uintptr_t)states) & 15u) != 0) { c->set_error("%s: the states are not 16-byte aligned", name); return EVPLP_ERR_INVALID; }
    // what the progressive gather refuses, before anything is written: its own checks on an empty batch, and the walk's stack
    int rc = band_gather(nullptr, 0, nullptr);
    if (rc) return rc;
    if (surface_stack_bytes(c->sc) > kMaxStackBytes) { c->set_error("%s: the walk's stack of this tree (%zu bytes per wave) exceeds a workgroup's LDS", name, surface_stack_bytes(c->sc)); return EVPLP_ERR_INVALID; }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const int32_t W = p->width, H = p->height, s2 = p->samples * p->samples;
    Raster r;
    if ((rc = raster_prepare(c, name, true, first, count, uvs, W, H, p->samples, &r))) return rc;
    const size_t band_samples = (size_t)W * s2 * (size_t)r.band;
    const size_t hits_b = align256(sizeof(evplp_hit) * band_samples), points_b = align256(sizeof(evplp_surface_point) * band_samples);
    const hipError_t e = grow_scratch_of(c, c->lm_bake, hits_b + points_b);
    if (e != hipSuccess) { c->set_error("%s: cannot allocate a band's %zu samples (%zu bytes): %s", name, band_samples, hits_b + points_b, hipGetErrorString(e)); return oom_or_hip(e); }
    char *d_hits = (char *)c->lm_bake.p, *d_points = d_hits + hits_b;
    for (int32_t y0 = 0; y0 < H; y0 += r.band) {
        const int32_t rows = std::min(r.band, H - y0);
        const int32_t n = (int32_t)((size_t)W * s2 * (size_t)rows);
        if ((rc = raster_band(c, name, &r, y0, rows, (evplp_hit *)d_hits))) return rc;
        launch_lightmap_points(points_args(c, d_hits, nullptr, d_points, n, p->flags), c->stream);
        HIP_TRY(c, hipGetLastError());
        evplp_surface_state *band = (evplp_surface_state *)states + (size_t)W * s2 * (size_t)y0;
        if ((rc = band_gather(d_points, n, band))) return rc;
    }
    return EVPLP_OK;
}

// the states of an atlas -> its texels, then the gutter passes of the bake.  No raster: a state says itself whether its sample was covered.
int bake_resolve(evplp_context *c, const char *name, bool device, const evplp_lightmap_params *p, const void *states, void *out) {
    if (!p) { c->set_error("%s: null params", name); return EVPLP_ERR_INVALID; }
    if (p->width < 1 || p->width > LM_MAX_SIZE || p->height < 1 || p->height > LM_MAX_SIZE) { c->set_error("%s: an atlas of %d x %d is not within 1 .. %d", name, p->width, p->height, LM_MAX_SIZE); return EVPLP_ERR_INVALID; }
    if (p->samples != 1 && p->samples != 2 && p->samples != 4) { c->set_error("%s: %d samples per axis is not 1, 2 or 4", name, p->samples); return EVPLP_ERR_INVALID; }
    if (p->gutter < 0 || p->gutter > 8) { c->set_error("%s: a gutter of %d is not 0 .. 8", name, p->gutter); return EVPLP_ERR_INVALID; }
    if (!states || !out) { c->set_error("%s: null states or destination", name); return EVPLP_ERR_INVALID; }
    if ((((uintptr_t)states) & 15u) != 0 || (device && (((uintptr_t)out) & 15u) != 0)) { c->set_error("%s: the states or the destination are not 16-byte aligned", name); return EVPLP_ERR_INVALID; }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const int32_t W = p->width, H = p->height;
    const size_t texels = (size_t)W * (size_t)H, atlas = align256(sizeof(evplp_lightmap_texel) * texels);
    const int own = (device ? 0 : 1) + (p->gutter > 0 ? 1 : 0);
    const hipError_t e = grow_scratch_of(c, c->lm_atlas, atlas * (size_t)own);
    if (e != hipSuccess) { c->set_error("%s: cannot allocate %d atlas buffers of %d x %d texels: %s", name, own, W, H, hipGetErrorString(e)); return oom_or_hip(e); }
    evplp_lightmap_texel *cur = device ? (evplp_lightmap_texel *)out : (evplp_lightmap_texel *)c->lm_atlas.p;
    evplp_lightmap_texel *other = p->gutter > 0 ? (evplp_lightmap_texel *)((char *)c->lm_atlas.p + (device ? 0 : atlas)) : nullptr;
    // (a launch takes at most 2^31 - 1 texels: the largest atlas has 2^26)
    LightmapProgResolveArgs ra; ra.states = (const float4 *)states; ra.out = cur; ra.texels = (int32_t)texels; ra.s2 = p->samples * p->samples;
    launch_lightmap_prog_resolve(ra, c->stream);
    HIP_TRY(c, hipGetLastError());
    for (int32_t d = 1; d <= p->gutter; d++) {
        GutterArgs g; g.from = cur; g.to = other; g.width = W; g.height = H; g.pass = d;
        launch_lightmap_gutter(g, c->stream);
        HIP_TRY(c, hipGetLastError());
        std::swap(cur, other);
    }
    if (device) {
        if (cur != out) HIP_TRY(c, hipMemcpyAsync(out, cur, sizeof(evplp_lightmap_texel) * texels, hipMemcpyDeviceToDevice, c->stream));
        return EVPLP_OK;
    }
    HIP_TRY(c, hipMemcpyAsync(out, cur, sizeof(evplp_lightmap_texel) * texels, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EVPLP_OK;
}
}

namespace evplp {
void release_lightmap(evplp_context *c) {
    for (DeviceScratch *s : { &c->lm_stage, &c->lm_tris, &c->lm_band, &c->lm_pairs, &c->lm_bake, &c->lm_atlas }) { hipFree(s->p); *s = DeviceScratch(); }
    if (c->h_lm_stage) hipHostFree(c->h_lm_stage);
    if (c->h_lm_count) hipHostFree(c->h_lm_count);
    c->h_lm_stage = nullptr; c->h_lm_count = nullptr;
}
}

extern "C" int evplp_surface_points(evplp_context *c, const evplp_hit *hits, int32_t n, uint32_t flags, const float *eyes, evplp_surface_point *out) {
    CTX_CHECK(c);
    return points(c, "evplp_surface_points", false, hits, n, flags, eyes, out);
}
extern "C" int evplp_surface_points_device(evplp_context *c, const void *d_hits, int32_t n, uint32_t flags, const void *d_eyes, void *d_out) {
    CTX_CHECK(c);
    return points(c, "evplp_surface_points_device", true, d_hits, n, flags, (const float *)d_eyes, d_out);
}
extern "C" int evplp_lightmap_samples(evplp_context *c, int32_t mesh, const float *uvs, int32_t width, int32_t height, int32_t samples, evplp_hit *out) {
    CTX_CHECK(c);
    return samples_call(c, "evplp_lightmap_samples", false, mesh, uvs, width, height, samples, out);
}
extern "C" int evplp_lightmap_samples_device(evplp_context *c, int32_t mesh, const void *d_uvs, int32_t width, int32_t height, int32_t samples, void *d_out) {
    CTX_CHECK(c);
    return samples_call(c, "evplp_lightmap_samples_device", true, mesh, (const float *)d_uvs, width, height, samples, d_out);
}
extern "C" int evplp_bake_lightmap(evplp_context *c, const evplp_frame_params *fp, uint32_t what, const evplp_lightmap_params *p, const float *uvs, evplp_lightmap_texel *out) {
    CTX_CHECK(c);
    return bake(c, "evplp_bake_lightmap", false, fp, what, p, uvs, out);
}
extern "C" int evplp_bake_lightmap_device(evplp_context *c, const evplp_frame_params *fp, uint32_t what, const evplp_lightmap_params *p, const void *d_uvs, void *d_out) {
    CTX_CHECK(c);
    return bake(c, "evplp_bake_lightmap_device", true, fp, what, p, (const float *)d_uvs, d_out);
}
extern "C" int evplp_bake_lightmap_progressive_device(evplp_context *c, const evplp_frame_params *fp, uint32_t what, float alpha, const evplp_lightmap_params *p, const void *d_uvs, void *d_states) {
    CTX_CHECK(c);
    return bake_progressive(c, "evplp_bake_lightmap_progressive_device", fp, what, alpha, p, (const float *)d_uvs, d_states);
}
extern "C" int evplp_bake_lightmap_knn_device(evplp_context *c, const evplp_frame_params *fp, const evplp_knn_params *params, const evplp_lightmap_params *p, const void *d_uvs, void *d_states) {
    CTX_CHECK(c);
    if (!params) { c->set_error("evplp_bake_lightmap_knn_device: null k-nearest params"); return EVPLP_ERR_INVALID; }
    return bake_progressive(c, "evplp_bake_lightmap_knn_device", fp, EVPLP_SURFACE_PHOTONS, params->alpha, p, (const float *)d_uvs, d_states, params);
}
extern "C" int evplp_bake_lightmap_resolve(evplp_context *c, const evplp_lightmap_params *p, const void *d_states, evplp_lightmap_texel *out) {
    CTX_CHECK(c);
    return bake_resolve(c, "evplp_bake_lightmap_resolve", false, p, d_states, out);
}
extern "C" int evplp_bake_lightmap_resolve_device(evplp_context *c, const evplp_lightmap_params *p, const void *d_states, void *d_out) {
    CTX_CHECK(c);
    return bake_resolve(c, "evplp_bake_lightmap_resolve_device", true, p, d_states, d_out);
}

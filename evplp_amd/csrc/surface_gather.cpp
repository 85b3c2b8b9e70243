// Surface gather (include/evplp.h "surface gather"): the host side of evplp_gather_surface and its device form.  A batch runs as launches
// of at most kSurfaceChunk points (surface_gather.hpp), so the partial sums and the host form's staging have one size whatever n is; the
// photon grid is built once per call, before the first chunk, for the call's radius and the records as they are.  The kernels are in
// kernels_surface.hip, the grid's arithmetic in photon_grid.h.
// The progressive gather (include/evplp.h "progressive surface gather": evplp_gather_surface_progressive, evplp_surface_resolve and their
// device forms) lives here too, behind the same checks, chunks and grid build: its own kernels are in kernels_surface_prog.hip, a state's
// rule in surface_state.h.  evplp_gather_surface_knn ("k-nearest-photon start radii") is a first photon half behind the same checks and
// the same grid: its select and its seeding walk are in kernels_surface_knn.hip, the select's arithmetic in knn_select.h.
#include "context.hpp"
#include "photon_grid.h"
#include "surface_gather.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

using namespace evplp;

namespace {
// the host form's staging: the points, the eyes behind them, the results behind those
constexpr size_t kStagePoints = sizeof(evplp_surface_point) * (size_t)kSurfaceChunk;
constexpr size_t kStageEyes = 3 * sizeof(float) * (size_t)kSurfaceChunk;
constexpr size_t kStageBytes = kStagePoints + kStageEyes + sizeof(evplp_surface_light) * (size_t)kSurfaceChunk;
static_assert((kStagePoints + kStageEyes) % 16 == 0, "the staged results are written as float4");
constexpr size_t kMaxStackBytes = 64 * 1024;       // as ray_query.cpp: the largest dynamic LDS a workgroup may ask for without an attribute

int oom_or_hip(hipError_t e) { return e == hipErrorOutOfMemory ? EVPLP_ERR_OOM : EVPLP_ERR_HIP; }
size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// what both forms refuse, in evplp.h's order; ray_query_check serves for what the queries refuse as well
bool surface_check(evplp_context *c, const char *name, bool device, const evplp_frame_params *fp, uint32_t what, const void *points, const void *eyes, int32_t n, const void *out) {
    if (!ray_query_check(c, name, points, n, 0, 0, out)) return false;
    if (!fp) { c->set_error("%s: null frame params", name); return false; }
    if (what == 0u || (what & ~(EVPLP_SURFACE_VPL | EVPLP_SURFACE_PHOTONS)) != 0u) { c->set_error("%s: what = 0x%x asks for nothing, or for something unknown", name, (unsigned)what); return false; }
    if (fp->mis_mode > 5u) { c->set_error("%s: mis_mode %u is not 0 .. 5", name, (unsigned)fp->mis_mode); return false; }
    const uint64_t have = (uint64_t)c->cfg.num_light_paths * c->cfg.photons_per_path;
    if (fp->photons_per_path == 0u) { c->set_error("%s: photons_per_path is 0", name); return false; }
    if (what & EVPLP_SURFACE_VPL) {
        if (fp->num_vpl_light_paths == 0u) { c->set_error("%s: num_vpl_light_paths is 0", name); return false; }
        const uint64_t slots = (uint64_t)fp->num_vpl_light_paths * fp->photons_per_path;
        if (slots > have) { c->set_error("%s: %llu VPL record slots asked for, the context's record buffer holds %llu", name, (unsigned long long)slots, (unsigned long long)have); return false; }
    }
    if (what & EVPLP_SURFACE_PHOTONS) {
        if (!std::isfinite(fp->photon_radius) || !(fp->photon_radius > 0.0f)) { c->set_error("%s: photon_radius %g is not a positive finite number", name, (double)fp->photon_radius); return false; }
        if (fp->num_light_paths == 0u) { c->set_error("%s: num_light_paths is 0", name); return false; }
        const uint64_t slots = (uint64_t)fp->num_light_paths * fp->photons_per_path;
        if (slots > have) { c->set_error("%s: %llu photon record slots asked for, the context's record buffer holds %llu", name, (unsigned long long)slots, (unsigned long long)have); return false; }
    }
    if (device && n > 0 && ((((uintptr_t)out) | ((uintptr_t)points)) & 15u) != 0) { c->set_error("%s: the points or the destination are not 16-byte aligned", name); return false; }
    (void)eyes;
    return true;
}

// the scene's box: the meshes' vertices as the host copy holds them (a refit keeps the figures current), as the ordering pass of the ray queries takes it
void scene_box(const evplp_context *c, float lo[3], float hi[3]) {
    for (int k = 0; k < 3; k++) { lo[k] = 3.0e38f; hi[k] = -3.0e38f; }
    for (const HostMesh &m : c->meshes) for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], m.lo[k]); hi[k] = std::max(hi[k], m.hi[k]); }
    for (int k = 0; k < 3; k++) if (!(lo[k] <= hi[k])) lo[k] = hi[k] = 0.0f;
}

// the grid of this call: plan, arrays, build.  The bucket count comes from the SLOT count -- an upper bound of the usable photons the host
// knows without reading anything back, so the device form never waits; the results do not depend on it.
int build_grid(evplp_context *c, const char *name, const evplp_frame_params *fp, SurfaceGrid *out, SurfaceGridBuild *build = nullptr) {
    SurfaceGridBuild b; std::memset(&b, 0, sizeof(b));
    const uint32_t slots = fp->num_light_paths * fp->photons_per_path;           // (checked against the record buffer: it fits 32 bits)
    scene_box(c, b.g.lo, b.g.hi);
    b.g.radius = fp->photon_radius; b.g.slots = slots;
    if (!pg_plan(fp->photon_radius, b.g.lo, b.g.hi, slots, &b.g.edge, &b.g.bits)) { c->set_error("%s: no grid for radius %g over the scene's box", name, (double)fp->photon_radius); return EVPLP_ERR_INVALID; }
    if (const char *env = std::getenv("EVPLP_SURFACE_GRID_BITS")) { const long v = std::strtol(env, nullptr, 10); if (v >= 1 && v <= (long)PG_MAX_BITS) b.g.bits = (uint32_t)v; }
    const size_t temp = surface_sort_temp_bytes(slots, b.g.bits);
    if (temp == 0) { (void)hipGetLastError(); c->set_error("%s: the radix sort states no workspace size", name); return EVPLP_ERR_HIP; }
    const size_t compact = align256(sizeof(float4) * kSurfaceCompactF4 * (size_t)slots), words = align256(sizeof(uint32_t) * (size_t)slots);
    const size_t table = align256(sizeof(uint32_t) * (((size_t)1 << b.g.bits) + 2));
    const size_t need = compact + 4 * words + table + temp;
    const hipError_t e = grow_scratch_of(c, c->surface_grid, need);
    if (e != hipSuccess) { c->set_error("%s: cannot allocate the photon grid of %u slots (%zu bytes): %s", name, slots, need, hipGetErrorString(e)); return oom_or_hip(e); }
    char *p = (char *)c->surface_grid.p;
    b.compact = (float4 *)p; p += compact;
    b.keys = (uint32_t *)p; p += words; b.keys_sorted = (uint32_t *)p; p += words; b.vals = (uint32_t *)p; p += words; b.vals_sorted = (uint32_t *)p; p += words;
    b.start = (uint32_t *)p; p += table;
    b.temp = p; b.temp_bytes = temp;
    b.fp = *fp; b.records = (const evplp_record *)c->buf[EVPLP_BUF_RECORDS];
    b.g.start = b.start; b.g.compact = b.compact;
    HIP_TRY(c, launch_surface_grid(b, c->stream));
    *out = b.g;
    if (build) *build = b;                  // (the progressive gather rewrites the compact records' flux behind the build)
    return EVPLP_OK;
}

// one batch, chunk by chunk.  device: points / eyes / out are device pointers and nothing waits; else they are staged and every chunk is waited for.
int gather(evplp_context *c, const char *name, bool device, const evplp_frame_params *fp, uint32_t what, const void *points, const float *eyes, int32_t n, void *out) {
    if (!surface_check(c, name, device, fp, what, points, eyes, n, out)) return EVPLP_ERR_INVALID;
    if (n == 0) return EVPLP_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const size_t lds = surface_stack_bytes(c->sc);
    if (lds > kMaxStackBytes) { c->set_error("%s: the walk's stack of this tree (%zu bytes per wave) exceeds a workgroup's LDS", name, lds); return EVPLP_ERR_INVALID; }
    const bool vpl = (what & EVPLP_SURFACE_VPL) != 0u, photons = (what & EVPLP_SURFACE_PHOTONS) != 0u;
    const uint32_t slots = vpl ? fp->num_vpl_light_paths * fp->photons_per_path : 0u;
    const uint32_t slices = surface_slices(slots);
    hipError_t e = grow_scratch_of(c, c->surface_partial, surface_partial_bytes(slices));
    if (e != hipSuccess) { c->set_error("%s: cannot allocate the partial sums of %u slices (%zu bytes): %s", name, slices, surface_partial_bytes(slices), hipGetErrorString(e)); return oom_or_hip(e); }
    if (!device) {
        e = grow_scratch_of(c, c->surface_stage, kStageBytes);
        if (e == hipSuccess && !c->h_surface_stage) {
            e = hipHostMalloc((void **)&c->h_surface_stage, kStageBytes, hipHostMallocDefault);
            if (e != hipSuccess) { (void)hipGetLastError(); c->h_surface_stage = nullptr; }
        }
        if (e != hipSuccess) { c->set_error("%s: cannot allocate the staging of %d points (%zu bytes): %s", name, kSurfaceChunk, kStageBytes, hipGetErrorString(e)); return oom_or_hip(e); }
    }
    SurfaceGrid grid; std::memset(&grid, 0, sizeof(grid));
    int rc;
    if (photons && (rc = build_grid(c, name, fp, &grid))) return rc;
    if (photons && device) {
        SurfaceArgs a; std::memset(&a, 0, sizeof(a));
        a.fp = *fp; a.n = n; a.what = what; a.points = (const float4 *)points; a.eyes = eyes; a.out = (evplp_surface_light *)out; a.grid = grid;
        launch_surface_photons(a, c->stream);
    }
    for (int64_t at = 0; at < n; at += kSurfaceChunk) {
        const int32_t m = (int32_t)std::min<int64_t>(kSurfaceChunk, n - at);
        SurfaceArgs a; std::memset(&a, 0, sizeof(a));
        a.sc = c->sc; a.fp = *fp; a.records = (const evplp_record *)c->buf[EVPLP_BUF_RECORDS]; a.n = m; a.what = what; a.slots = slots; a.slices = slices;
        a.pdf_mc2 = fp->pdf_mc * fp->pdf_mc; a.paths = (float)fp->num_vpl_light_paths;
        a.partial = (float *)c->surface_partial.p;
        a.grid = grid;
        if (device) {
            a.points = (const float4 *)points + 4 * (size_t)at; a.eyes = eyes ? eyes + 3 * (size_t)at : nullptr; a.out = (evplp_surface_light *)out + at;
        } else {
            char *h = c->h_surface_stage, *d = (char *)c->surface_stage.p;
            std::memcpy(h, (const evplp_surface_point *)points + at, sizeof(evplp_surface_point) * (size_t)m);
            if (eyes) std::memcpy(h + kStagePoints, eyes + 3 * (size_t)at, 3 * sizeof(float) * (size_t)m);
            // (points and eyes lie apart in the staging: two copies when there are eyes)
            HIP_TRY(c, hipMemcpyAsync(d, h, sizeof(evplp_surface_point) * (size_t)m, hipMemcpyHostToDevice, c->stream));
            if (eyes) HIP_TRY(c, hipMemcpyAsync(d + kStagePoints, h + kStagePoints, 3 * sizeof(float) * (size_t)m, hipMemcpyHostToDevice, c->stream));
            a.points = (const float4 *)d; a.eyes = eyes ? (const float *)(d + kStagePoints) : nullptr; a.out = (evplp_surface_light *)(d + kStagePoints + kStageEyes);
        }
        // the photon query needs no scratch of its own: the device form ran it over the whole batch before the first chunk
        if (photons && !device) launch_surface_photons(a, c->stream);
        if (vpl) launch_surface_vpl(a, c->stream);
        launch_surface_reduce(a, c->stream);
        HIP_TRY(c, hipGetLastError());
        if (!device) {
            char *h = c->h_surface_stage + kStagePoints + kStageEyes;
            HIP_TRY(c, hipMemcpyAsync(h, a.out, sizeof(evplp_surface_light) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            std::memcpy((evplp_surface_light *)out + at, h, sizeof(evplp_surface_light) * (size_t)m);
        }
    }
    // (the overlapped light tracing may overwrite the records only behind their readers, as behind the gathers)
    if (c->aux_stream) HIP_TRY(c, hipEventRecord(c->ev_records_read, c->stream));
    return EVPLP_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the progressive gather
// the host forms' staging: the points, the eyes behind them, the states behind those (the resolve puts its states there and its results first)
constexpr size_t kProgStageStates = sizeof(evplp_surface_state) * (size_t)kSurfaceChunk;
constexpr size_t kProgStageBytes = kStagePoints + kStageEyes + kProgStageStates;
constexpr size_t kProgLightsBytes = sizeof(evplp_surface_light) * (size_t)kSurfaceChunk;
static_assert(sizeof(evplp_surface_light) <= sizeof(evplp_surface_point), "the resolve's results fit the points' part of the staging");

int prog_stage(evplp_context *c, const char *name) {
    hipError_t e = grow_scratch_of(c, c->surface_prog_stage, kProgStageBytes);
    if (e == hipSuccess && !c->h_surface_prog_stage) {
        e = hipHostMalloc((void **)&c->h_surface_prog_stage, kProgStageBytes, hipHostMallocDefault);
        if (e != hipSuccess) { (void)hipGetLastError(); c->h_surface_prog_stage = nullptr; }
    }
    if (e != hipSuccess) { c->set_error("%s: cannot allocate the staging of %d points (%zu bytes): %s", name, kSurfaceChunk, kProgStageBytes, hipGetErrorString(e)); return oom_or_hip(e); }
    return EVPLP_OK;
}

// One iteration.  Per chunk: today's VPL kernel into the partial sums, today's reduce into 32 B per point, the fold into the states; the
// query walks behind the fold -- chunk by chunk in the host form, once over the whole batch in the device form -- so both halves decide
// "flagged" from the state as it came in.
// what the progressive calls refuse on top of surface_check, in evplp.h's order (the k-nearest call refuses the same)
bool prog_check(evplp_context *c, const char *name, bool device, const evplp_frame_params *fp, uint32_t what, float alpha, const void *points, const float *eyes, int32_t n, const void *states) {
    // (the states first, by their name: surface_check would call them "the destination")
    if (n > 0 && !states) { c->set_error("%s: null states", name); return false; }
    if (device && n > 0 && (((uintptr_t)states) & 15u) != 0) { c->set_error("%s: the states are not 16-byte aligned", name); return false; }
    if (!surface_check(c, name, device, fp, what, points, eyes, n, states)) return false;
    if (fp->mis_mode >= 1u && fp->mis_mode <= 3u) {
        c->set_error("%s: mis_mode %u weighs by pdf_mc = n_vpl / n_light / (pi r^2), which a radius per point makes a per-point quantity in both halves: only modes 0, 4 and 5", name, (unsigned)fp->mis_mode);
        return false;
    }
    if (!std::isfinite(alpha) || !(alpha > 0.0f) || alpha > 1.0f) { c->set_error("%s: alpha %g is not within (0, 1]", name, (double)alpha); return false; }
    return true;
}

int gather_progressive(evplp_context *c, const char *name, bool device, const evplp_frame_params *fp, uint32_t what, float alpha, const void *points, const float *eyes, int32_t n, void *states) {
    if (!prog_check(c, name, device, fp, what, alpha, points, eyes, n, states)) return EVPLP_ERR_INVALID;
    if (n == 0) return EVPLP_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const size_t lds = surface_stack_bytes(c->sc);
    if (lds > kMaxStackBytes) { c->set_error("%s: the walk's stack of this tree (%zu bytes per wave) exceeds a workgroup's LDS", name, lds); return EVPLP_ERR_INVALID; }
    const bool vpl = (what & EVPLP_SURFACE_VPL) != 0u, photons = (what & EVPLP_SURFACE_PHOTONS) != 0u;
    const uint32_t slots = vpl ? fp->num_vpl_light_paths * fp->photons_per_path : 0u;
    const uint32_t slices = surface_slices(slots);
    if (vpl) {
        hipError_t e = grow_scratch_of(c, c->surface_partial, surface_partial_bytes(slices));
        if (e == hipSuccess) e = grow_scratch_of(c, c->surface_prog_lights, kProgLightsBytes);
        if (e != hipSuccess) { c->set_error("%s: cannot allocate the partial sums of %u slices (%zu bytes): %s", name, slices, surface_partial_bytes(slices) + kProgLightsBytes, hipGetErrorString(e)); return oom_or_hip(e); }
    }
    int rc;
    if (!device && (rc = prog_stage(c, name))) return rc;
    SurfaceProgArgs q; std::memset(&q, 0, sizeof(q));
    q.fp = *fp; q.what = what; q.alpha = alpha; q.r0sq = fp->photon_radius * fp->photon_radius;
    q.lights = (const float4 *)c->surface_prog_lights.p;
    if (photons) {
        SurfaceGridBuild b;
        if ((rc = build_grid(c, name, fp, &q.grid, &b))) return rc;
        launch_surface_prog_compact(b, c->stream);
        HIP_TRY(c, hipGetLastError());
    }
    for (int64_t at = 0; at < n; at += kSurfaceChunk) {
        const int32_t m = (int32_t)std::min<int64_t>(kSurfaceChunk, n - at);
        q.n = m;
        char *h = c->h_surface_prog_stage, *d = (char *)c->surface_prog_stage.p;
        if (device) {
            q.points = (const float4 *)points + 4 * (size_t)at; q.eyes = eyes ? eyes + 3 * (size_t)at : nullptr; q.states = (float4 *)states + 3 * (size_t)at;
        } else {
            std::memcpy(h, (const evplp_surface_point *)points + at, sizeof(evplp_surface_point) * (size_t)m);
            if (eyes) std::memcpy(h + kStagePoints, eyes + 3 * (size_t)at, 3 * sizeof(float) * (size_t)m);
            std::memcpy(h + kStagePoints + kStageEyes, (const evplp_surface_state *)states + at, sizeof(evplp_surface_state) * (size_t)m);
            HIP_TRY(c, hipMemcpyAsync(d, h, sizeof(evplp_surface_point) * (size_t)m, hipMemcpyHostToDevice, c->stream));
            if (eyes) HIP_TRY(c, hipMemcpyAsync(d + kStagePoints, h + kStagePoints, 3 * sizeof(float) * (size_t)m, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipMemcpyAsync(d + kStagePoints + kStageEyes, h + kStagePoints + kStageEyes, sizeof(evplp_surface_state) * (size_t)m, hipMemcpyHostToDevice, c->stream));
            q.points = (const float4 *)d; q.eyes = eyes ? (const float *)(d + kStagePoints) : nullptr; q.states = (float4 *)(d + kStagePoints + kStageEyes);
        }
        if (vpl) {
            SurfaceArgs a; std::memset(&a, 0, sizeof(a));
            a.sc = c->sc; a.fp = *fp; a.records = (const evplp_record *)c->buf[EVPLP_BUF_RECORDS]; a.n = m; a.what = EVPLP_SURFACE_VPL; a.slots = slots; a.slices = slices;
            a.pdf_mc2 = fp->pdf_mc * fp->pdf_mc; a.paths = (float)fp->num_vpl_light_paths;
            a.partial = (float *)c->surface_partial.p;
            a.points = q.points; a.eyes = q.eyes; a.out = (evplp_surface_light *)c->surface_prog_lights.p;
            launch_surface_vpl(a, c->stream);
            launch_surface_reduce(a, c->stream);
            launch_surface_prog_fold(q, c->stream);
        }
        if (photons && !device) launch_surface_prog_photons(q, c->stream);
        HIP_TRY(c, hipGetLastError());
        if (!device) {
            HIP_TRY(c, hipMemcpyAsync(h + kStagePoints + kStageEyes, q.states, sizeof(evplp_surface_state) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            std::memcpy((evplp_surface_state *)states + at, h + kStagePoints + kStageEyes, sizeof(evplp_surface_state) * (size_t)m);
        }
    }
    if (photons && device) {
        q.n = n; q.points = (const float4 *)points; q.eyes = eyes; q.states = (float4 *)states;
        launch_surface_prog_photons(q, c->stream);
        HIP_TRY(c, hipGetLastError());
    }
    if (c->aux_stream) HIP_TRY(c, hipEventRecord(c->ev_records_read, c->stream));
    return EVPLP_OK;
}

// --------------------------------------------------------------------------------------------------- k-nearest-photon start radii
bool knn_check(evplp_context *c, const char *name, const evplp_frame_params *fp, const evplp_knn_params *p) {
    if (p->k == 0u) { c->set_error("%s: k is 0", name); return false; }
    const float rminsq = p->r_min * p->r_min;
    if (!std::isfinite(p->r_min) || !(p->r_min > 0.0f) || p->r_min > fp->photon_radius || !(rminsq >= 0x1p-100f)) {
        c->set_error("%s: r_min %g is not a positive finite number up to photon_radius %g whose square is at least 2^-100", name, (double)p->r_min, (double)fp->photon_radius);
        return false;
    }
    if (p->flags != 0u) { c->set_error("%s: unknown flag bits 0x%x", name, (unsigned)p->flags); return false; }
    return true;
}

// The first photon half at the k-th nearest photon's distance: the progressive gather's grid and compact records, then the select and
// the seeding walk -- over the whole batch in the device form, chunk by chunk through the progressive gather's staging in the host form.
int gather_knn(evplp_context *c, const char *name, bool device, const evplp_frame_params *fp, const evplp_knn_params *p, const void *points, const float *eyes, int32_t n, void *states) {
    if (!p) { c->set_error("%s: null params", name); return EVPLP_ERR_INVALID; }
    if (!prog_check(c, name, device, fp, EVPLP_SURFACE_PHOTONS, p->alpha, points, eyes, n, states)) return EVPLP_ERR_INVALID;
    if (!knn_check(c, name, fp, p)) return EVPLP_ERR_INVALID;
    if (n == 0) return EVPLP_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const size_t lds = surface_stack_bytes(c->sc);      // (nothing here walks the tree; refused all the same, so that this call refuses what the progressive one does)
    if (lds > kMaxStackBytes) { c->set_error("%s: the walk's stack of this tree (%zu bytes per wave) exceeds a workgroup's LDS", name, lds); return EVPLP_ERR_INVALID; }
    int rc;
    if (!device && (rc = prog_stage(c, name))) return rc;
    const size_t radii = sizeof(float) * (size_t)(device ? n : std::min(n, kSurfaceChunk));
    const hipError_t e = grow_scratch_of(c, c->surface_knn_rk2, radii);
    if (e != hipSuccess) { c->set_error("%s: cannot allocate the selected radii (%zu bytes): %s", name, radii, hipGetErrorString(e)); return oom_or_hip(e); }
    SurfaceKnnArgs q; std::memset(&q, 0, sizeof(q));
    q.p.fp = *fp; q.p.what = EVPLP_SURFACE_PHOTONS; q.p.alpha = p->alpha; q.p.r0sq = fp->photon_radius * fp->photon_radius;
    q.rk2 = (float *)c->surface_knn_rk2.p; q.k = p->k; q.rminsq = p->r_min * p->r_min;
    SurfaceGridBuild b;
    if ((rc = build_grid(c, name, fp, &q.p.grid, &b))) return rc;
    launch_surface_prog_compact(b, c->stream);
    HIP_TRY(c, hipGetLastError());
    if (device) {
        q.p.n = n; q.p.points = (const float4 *)points; q.p.eyes = eyes; q.p.states = (float4 *)states;
        launch_surface_knn_select(q, c->stream);
        launch_surface_knn_photons(q, c->stream);
        HIP_TRY(c, hipGetLastError());
    } else for (int64_t at = 0; at < n; at += kSurfaceChunk) {
        const int32_t m = (int32_t)std::min<int64_t>(kSurfaceChunk, n - at);
        char *h = c->h_surface_prog_stage, *d = (char *)c->surface_prog_stage.p;
        const size_t off = kStagePoints + kStageEyes;
        std::memcpy(h, (const evplp_surface_point *)points + at, sizeof(evplp_surface_point) * (size_t)m);
        if (eyes) std::memcpy(h + kStagePoints, eyes + 3 * (size_t)at, 3 * sizeof(float) * (size_t)m);
        std::memcpy(h + off, (const evplp_surface_state *)states + at, sizeof(evplp_surface_state) * (size_t)m);
        HIP_TRY(c, hipMemcpyAsync(d, h, sizeof(evplp_surface_point) * (size_t)m, hipMemcpyHostToDevice, c->stream));
        if (eyes) HIP_TRY(c, hipMemcpyAsync(d + kStagePoints, h + kStagePoints, 3 * sizeof(float) * (size_t)m, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(d + off, h + off, sizeof(evplp_surface_state) * (size_t)m, hipMemcpyHostToDevice, c->stream));
        q.p.n = m; q.p.points = (const float4 *)d; q.p.eyes = eyes ? (const float *)(d + kStagePoints) : nullptr; q.p.states = (float4 *)(d + off);
        launch_surface_knn_select(q, c->stream);
        launch_surface_knn_photons(q, c->stream);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(h + off, q.p.states, sizeof(evplp_surface_state) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        std::memcpy((evplp_surface_state *)states + at, h + off, sizeof(evplp_surface_state) * (size_t)m);
    }
    if (c->aux_stream) HIP_TRY(c, hipEventRecord(c->ev_records_read, c->stream));
    return EVPLP_OK;
}

int resolve_states(evplp_context *c, const char *name, bool device, const void *states, int32_t n, void *out) {
    if (n < 0) { c->set_error("%s: n = %d", name, n); return EVPLP_ERR_INVALID; }
    if (n > 0 && (!states || !out)) { c->set_error("%s: null states or destination", name); return EVPLP_ERR_INVALID; }
    if (device && n > 0 && ((((uintptr_t)out) | ((uintptr_t)states)) & 15u) != 0) { c->set_error("%s: the states or the destination are not 16-byte aligned", name); return EVPLP_ERR_INVALID; }
    if (n == 0) return EVPLP_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    SurfaceResolveArgs a;
    if (device) {
        a.states = (const float4 *)states; a.out = (float4 *)out; a.n = n;
        launch_surface_prog_resolve(a, c->stream);
        HIP_TRY(c, hipGetLastError());
        return EVPLP_OK;
    }
    int rc;
    if ((rc = prog_stage(c, name))) return rc;
    char *h = c->h_surface_prog_stage, *d = (char *)c->surface_prog_stage.p;
    for (int64_t at = 0; at < n; at += kSurfaceChunk) {
        const int32_t m = (int32_t)std::min<int64_t>(kSurfaceChunk, n - at);
        const size_t off = kStagePoints + kStageEyes;
        std::memcpy(h + off, (const evplp_surface_state *)states + at, sizeof(evplp_surface_state) * (size_t)m);
        HIP_TRY(c, hipMemcpyAsync(d + off, h + off, sizeof(evplp_surface_state) * (size_t)m, hipMemcpyHostToDevice, c->stream));
        a.states = (const float4 *)(d + off); a.out = (float4 *)d; a.n = m;
        launch_surface_prog_resolve(a, c->stream);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(h, d, sizeof(evplp_surface_light) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        std::memcpy((evplp_surface_light *)out + at, h, sizeof(evplp_surface_light) * (size_t)m);
    }
    return EVPLP_OK;
}
}

namespace evplp {
void release_surface_gather(evplp_context *c) {
    hipFree(c->surface_partial.p); hipFree(c->surface_grid.p); hipFree(c->surface_stage.p);
    hipFree(c->surface_prog_lights.p); hipFree(c->surface_prog_stage.p); hipFree(c->surface_knn_rk2.p);
    c->surface_partial = DeviceScratch(); c->surface_grid = DeviceScratch(); c->surface_stage = DeviceScratch();
    c->surface_prog_lights = DeviceScratch(); c->surface_prog_stage = DeviceScratch(); c->surface_knn_rk2 = DeviceScratch();
    if (c->h_surface_stage) hipHostFree(c->h_surface_stage);
    if (c->h_surface_prog_stage) hipHostFree(c->h_surface_prog_stage);
    c->h_surface_stage = nullptr; c->h_surface_prog_stage = nullptr;
}
}

extern "C" int evplp_gather_surface(evplp_context *c, const evplp_frame_params *fp, uint32_t what, const evplp_surface_point *points, const float *eyes, int32_t n, evplp_surface_light *out) {
    CTX_CHECK(c);
    return gather(c, "evplp_gather_surface", false, fp, what, points, eyes, n, out);
}
extern "C" int evplp_gather_surface_device(evplp_context *c, const evplp_frame_params *fp, uint32_t what, const void *d_points, const void *d_eyes, int32_t n, void *d_out) {
    CTX_CHECK(c);
    return gather(c, "evplp_gather_surface_device", true, fp, what, d_points, (const float *)d_eyes, n, d_out);
}
extern "C" int evplp_gather_surface_progressive(evplp_context *c, const evplp_frame_params *fp, uint32_t what, float alpha, const evplp_surface_point *points, const float *eyes, int32_t n, evplp_surface_state *states) {
    CTX_CHECK(c);
    return gather_progressive(c, "evplp_gather_surface_progressive", false, fp, what, alpha, points, eyes, n, states);
}
extern "C" int evplp_gather_surface_progressive_device(evplp_context *c, const evplp_frame_params *fp, uint32_t what, float alpha, const void *d_points, const void *d_eyes, int32_t n, void *d_states) {
    CTX_CHECK(c);
    return gather_progressive(c, "evplp_gather_surface_progressive_device", true, fp, what, alpha, d_points, (const float *)d_eyes, n, d_states);
}
extern "C" int evplp_gather_surface_knn(evplp_context *c, const evplp_frame_params *fp, const evplp_knn_params *params, const evplp_surface_point *points, const float *eyes, int32_t n, evplp_surface_state *states) {
    CTX_CHECK(c);
    return gather_knn(c, "evplp_gather_surface_knn", false, fp, params, points, eyes, n, states);
}
extern "C" int evplp_gather_surface_knn_device(evplp_context *c, const evplp_frame_params *fp, const evplp_knn_params *params, const void *d_points, const void *d_eyes, int32_t n, void *d_states) {
    CTX_CHECK(c);
    return gather_knn(c, "evplp_gather_surface_knn_device", true, fp, params, d_points, (const float *)d_eyes, n, d_states);
}
extern "C" int evplp_surface_resolve(evplp_context *c, const evplp_surface_state *states, int32_t n, evplp_surface_light *out) {
    CTX_CHECK(c);
    return resolve_states(c, "evplp_surface_resolve", false, states, n, out);
}
extern "C" int evplp_surface_resolve_device(evplp_context *c, const void *d_states, int32_t n, void *d_out) {
    CTX_CHECK(c);
    return resolve_states(c, "evplp_surface_resolve_device", true, d_states, n, d_out);
}

// C-ABI implementation (include/evplp.h): context, scene upload, pass launchers, statistics.
// There is deliberately no CPU execution path here: every pass is a HIP kernel launch.
#include "context.hpp"
#include "host/gather_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>
#include <cstdlib>

using namespace evplp;

static thread_local char g_create_error[512] = "";
// default bounds of the gathers' two large scratch buffers (evplp_config.cut_scratch_bytes / vsl_mask_bytes = 0; include/evplp.h has the table)
constexpr size_t kDefaultCutScratchBytes = (size_t)8 << 30, kDefaultVslMaskBytes = (size_t)2 << 30;
static_assert(kPlanVplSplit == kVplSplit && kPlanDefaultSplitsPerWave == kDefaultSplitsPerWave && kPlanCutSlotBytes == kCutSlotBytes, "host/gather_plan.hpp restates these constants of kernels.h");

void evplp_context::set_error(const char *fmt, ...) {
    va_list ap; va_start(ap, fmt);
    vsnprintf(error, sizeof(error), fmt, ap);
    va_end(ap);
}

static size_t buffer_bytes(const evplp_context *c, int which) {
    const size_t px = (size_t)c->st.W * c->st.local_rows;
    if (which == EVPLP_BUF_RECORDS) return sizeof(evplp_record) * (size_t)c->cfg.num_light_paths * c->cfg.photons_per_path;
    return px * sizeof(float4);
}

// A pass's scratch that only grows: nothing to do while it holds `need` bytes; else wait for the context's streams (its kernels may still read
// the old allocation), free it and allocate `need`.  On failure the scratch is left empty, the sticky HIP error is cleared, and the caller
// says what that means: a fallback for the gather's cuts, an error in its own words for the rest.
static hipError_t grow_scratch(evplp_context *c, DeviceScratch &s, size_t need) {
    if (s.bytes >= need) return hipSuccess;
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess && c->aux_stream) e = hipStreamSynchronize(c->aux_stream);
    if (e != hipSuccess) return e;
    hipFree(s.p); s.p = nullptr; s.bytes = 0;
    if ((e = hipMalloc(&s.p, need)) != hipSuccess) { (void)hipGetLastError(); s.p = nullptr; return e; }
    s.bytes = need;
    return hipSuccess;
}
namespace evplp { hipError_t grow_scratch_of(evplp_context *ctx, DeviceScratch &s, size_t need) { return grow_scratch(ctx, s, need); } }   // (for ray_query.cpp)
// a buffer made by the first call of entry point `name` that needs it and kept (evplp_denoise's and evplp_denoise_temporal's planes)
static int alloc_once(evplp_context *c, const char *name, void **p, size_t bytes) {
    if (*p) return EVPLP_OK;
    const hipError_t e = hipMalloc(p, std::max<size_t>(bytes, 16));
    if (e == hipSuccess) return EVPLP_OK;
    (void)hipGetLastError(); *p = nullptr;
    c->set_error("%s: cannot allocate %zu bytes: %s", name, bytes, hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? EVPLP_ERR_OOM : EVPLP_ERR_HIP;
}

static int settle_splat(evplp_context *c);
static int adapt_reset(evplp_context *c);
namespace evplp { AdaptTiles adapt_view(const evplp_context *c, float scale); }

namespace evplp { void set_context_error(evplp_context *ctx, const char *text) { if (ctx) ctx->set_error("%s", text ? text : ""); } }

extern "C" int evplp_abi_version(void) { return EVPLP_ABI_VERSION; }

extern "C" const char *evplp_last_error(const evplp_context *ctx) { return ctx ? ctx->error : g_create_error; }

extern "C" int evplp_create(const evplp_config *cfg, evplp_context **out) {
    if (!cfg || !out) { snprintf(g_create_error, sizeof(g_create_error), "evplp_create: null argument"); return EVPLP_ERR_INVALID; }
    *out = nullptr;
    if (cfg->abi_version != EVPLP_ABI_VERSION) { snprintf(g_create_error, sizeof(g_create_error), "ABI version mismatch: caller %d, library %d", cfg->abi_version, EVPLP_ABI_VERSION); return EVPLP_ERR_INVALID; }
    if (cfg->res_x <= 0 || cfg->res_y <= 0 || cfg->photons_per_path == 0 || cfg->num_light_paths == 0) {
        snprintf(g_create_error, sizeof(g_create_error), "evplp_create: resolution, num_light_paths and photons_per_path must be positive"); return EVPLP_ERR_INVALID;
    }
    if (cfg->gather_splits_per_wave < 0 || cfg->gather_splits_per_wave > 32 || (cfg->gather_splits_per_wave & (cfg->gather_splits_per_wave - 1)) != 0) {
        snprintf(g_create_error, sizeof(g_create_error), "evplp_create: gather_splits_per_wave must be 0 (automatic) or a power of two <= 32"); return EVPLP_ERR_INVALID;
    }
    if (cfg->strip_capacity_rows < 0) { snprintf(g_create_error, sizeof(g_create_error), "evplp_create: strip_capacity_rows is negative"); return EVPLP_ERR_INVALID; }
    if (cfg->num_vpl_light_paths > cfg->num_light_paths) {
        snprintf(g_create_error, sizeof(g_create_error), "evplp_create: num_vpl_light_paths > num_light_paths (VPLs are the first paths of the same set, lighttracing.cu:368)"); return EVPLP_ERR_INVALID;
    }
    int strip_count = cfg->strip_count > 0 ? cfg->strip_count : 1;
    int strip_rows = strip_count == 1 ? ((cfg->res_y + 7) / 8) * 8 : cfg->strip_rows;
    if (strip_rows <= 0 || (strip_rows % 8) != 0 || cfg->strip_rank < 0 || cfg->strip_rank >= strip_count) {
        snprintf(g_create_error, sizeof(g_create_error), "evplp_create: strip_rows must be a positive multiple of 8 and 0 <= strip_rank < strip_count"); return EVPLP_ERR_INVALID;
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        snprintf(g_create_error, sizeof(g_create_error), "no HIP device available (%s); libevplp_hip has no CPU fallback", e != hipSuccess ? hipGetErrorString(e) : "device count 0");
        return EVPLP_ERR_NO_DEVICE;
    }
    if (cfg->device < 0 || cfg->device >= ndev) { snprintf(g_create_error, sizeof(g_create_error), "device %d out of range (%d devices)", cfg->device, ndev); return EVPLP_ERR_INVALID; }
    e = hipSetDevice(cfg->device);
    if (e != hipSuccess) { snprintf(g_create_error, sizeof(g_create_error), "hipSetDevice: %s", hipGetErrorString(e)); return EVPLP_ERR_NO_DEVICE; }

    int32_t ploc_radius = 0, ploc_iterations = -1;
    // (developer overrides of the PLOC builder, so that tests reach the window's edges and the pairing phase on small scenes)
    if (const char *env = std::getenv("EVPLP_PLOC_RADIUS")) {
        char *end = nullptr; const long v = strtol(env, &end, 10);
        if (end == env || *end || v < 1 || v > kPlocMaxRadius) { snprintf(g_create_error, sizeof(g_create_error), "evplp_create: EVPLP_PLOC_RADIUS=%s is not in 1 .. %d", env, kPlocMaxRadius); return EVPLP_ERR_INVALID; }
        ploc_radius = (int32_t)v;
    }
    if (const char *env = std::getenv("EVPLP_PLOC_ITERATIONS")) {
        char *end = nullptr; const long v = strtol(env, &end, 10);
        if (end == env || *end || v < 0 || v > kPlocSearchIterations) { snprintf(g_create_error, sizeof(g_create_error), "evplp_create: EVPLP_PLOC_ITERATIONS=%s is not in 0 .. %d", env, kPlocSearchIterations); return EVPLP_ERR_INVALID; }
        ploc_iterations = (int32_t)v;
    }
    evplp_context *c = new evplp_context();
    c->cfg = *cfg; c->cfg.strip_count = strip_count; c->cfg.strip_rows = strip_rows;
    if (const char *env = std::getenv("EVPLP_BVH_BUILDER"))
        c->env_bvh_builder = !std::strcmp(env, "sbvh") ? EVPLP_BVH_SBVH : !std::strcmp(env, "lbvh") ? EVPLP_BVH_LBVH : !std::strcmp(env, "gpu") ? EVPLP_BVH_LBVH_GPU : !std::strcmp(env, "ploc") ? EVPLP_BVH_PLOC_GPU : EVPLP_BVH_SAH;
    c->env_ploc_radius = ploc_radius; c->env_ploc_iterations = ploc_iterations;
    if (const char *env = std::getenv("EVPLP_CUTS")) c->env_cuts = atoi(env) != 0 ? 1 : 0;
    if (const char *env = std::getenv("EVPLP_ITEM_DEAL")) c->env_item_deal = atoi(env) != 0 ? 1 : 0;
    // The bounds of the gathers' cut scratch and VSL mask buffer: the test override, else evplp_config, else 8 GB / 2 GB (round 6; until round 5
    // a quarter and a twentieth of the device's memory -- 72 GB of 288, which let config #5's 68 GB of slots sit in one band, 0.7 % faster than
    // the eight it takes now, 1 167 against 1 174 ms, and its 8.6 GB of masks in one launch -- and took a quarter of the GPU from whoever else
    // lives on it: a library embedded in a host application asks for that much only when told to).  Configurations within the bound -- config
    // #2 / #3: 4.3 GB of cuts -- allocate what they need; larger ones are gathered band by band, group range by group range (host/gather_plan.cpp).
    size_t env_cut_bytes = 0, env_mask_bytes = 0;
    if (const char *env = std::getenv("EVPLP_CUT_BYTES")) env_cut_bytes = (size_t)strtoull(env, nullptr, 10);      // (tests: forces the band path)
    if (const char *env = std::getenv("EVPLP_MASK_BYTES")) env_mask_bytes = (size_t)strtoull(env, nullptr, 10);    // (tests: forces the group-range path)
    c->cut_cap = env_cut_bytes ? env_cut_bytes : cfg->cut_scratch_bytes ? (size_t)cfg->cut_scratch_bytes : kDefaultCutScratchBytes;
    c->mask_cap = env_mask_bytes ? env_mask_bytes : cfg->vsl_mask_bytes ? (size_t)cfg->vsl_mask_bytes : kDefaultVslMaskBytes;
    if (const char *env = std::getenv("EVPLP_GATHER_K")) { int v = atoi(env); if (v >= 1 && v <= 32 && (v & (v - 1)) == 0) c->env_gather_k = v; }
    if (const char *env = std::getenv("EVPLP_TILE_BLOCK_LOG2")) c->env_tile_block_log2 = std::max(0, atoi(env));
    if (const char *env = std::getenv("EVPLP_SPLIT_MIN")) c->env_split_min = std::max(0, atoi(env));
    c->st.W = cfg->res_x; c->st.H = cfg->res_y;
    c->st.strip_rank = cfg->strip_rank; c->st.strip_count = strip_count; c->st.strip_rows = strip_rows;
    int nblocks = (cfg->res_y + strip_rows - 1) / strip_rows;
    int owned = (nblocks + strip_count - 1) / strip_count;  // padded: equal on every rank (all-gather chunks)
    // strip_capacity_rows: room for more blocks than the equal share (a deal by cost gives a rank of cheap blocks more of them: evplp_set_blocks)
    if (strip_count > 1 && cfg->strip_capacity_rows > owned * strip_rows) owned = std::min((cfg->strip_capacity_rows + strip_rows - 1) / strip_rows, nblocks);
    c->st.local_rows = owned * strip_rows;
    c->st.cap_blocks = owned; c->image_blocks = nblocks;
    // rows of this strip that fall inside the image
    c->rows_in_image = 0;
    for (int l = 0; l < c->st.local_rows; l++) if (c->st.global_row(l) < c->st.H) c->rows_in_image++;

    auto fail = [&](const char *what, hipError_t err) {
        snprintf(g_create_error, sizeof(g_create_error), "%s: %s", what, hipGetErrorString(err));
        evplp_destroy(c); return err == hipErrorOutOfMemory ? EVPLP_ERR_OOM : EVPLP_ERR_HIP;
    };
    if ((e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking)) != hipSuccess) return fail("hipStreamCreate", e);
    c->stream = c->own_stream;
    if (cfg->overlap_light_tracing) {
        if ((e = hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking)) != hipSuccess) return fail("hipStreamCreate", e);
        if ((e = hipEventCreateWithFlags(&c->ev_records_read, hipEventDisableTiming)) != hipSuccess) return fail("hipEventCreate", e);
        if ((e = hipEventCreateWithFlags(&c->ev_light_done, hipEventDisableTiming)) != hipSuccess) return fail("hipEventCreate", e);
        if ((e = hipEventCreateWithFlags(&c->ev_back_read, hipEventDisableTiming)) != hipSuccess) return fail("hipEventCreate", e);
    }
    for (int i = 0; i < EVPLP_PASS_COUNT; i++) {
        if ((e = hipEventCreate(&c->ev_begin[i])) != hipSuccess) return fail("hipEventCreate", e);
        if ((e = hipEventCreate(&c->ev_end[i])) != hipSuccess) return fail("hipEventCreate", e);
        if ((e = hipEventCreate(&c->ev_dom_begin[i])) != hipSuccess) return fail("hipEventCreate", e);
        if ((e = hipEventCreate(&c->ev_dom_end[i])) != hipSuccess) return fail("hipEventCreate", e);
    }
    for (int b = 0; b < EVPLP_BUF_COUNT; b++) {
        size_t bytes = buffer_bytes(c, b);
        if ((e = hipMalloc(&c->buf[b], bytes)) != hipSuccess) return fail("hipMalloc(buffer)", e);
        if ((e = hipMemset(c->buf[b], 0, bytes)) != hipSuccess) return fail("hipMemset", e);
        c->buf_owned[b] = true;
    }
    const size_t nvpl_slots = nvpl_slot_count(cfg->num_vpl_light_paths, cfg->photons_per_path);
    if ((e = hipMalloc((void **)&c->d_vpls, sizeof(evplp_record) * nvpl_slots)) != hipSuccess) return fail("hipMalloc(vpls)", e);
    if ((e = hipMalloc((void **)&c->d_vpl_src, sizeof(uint32_t) * nvpl_slots)) != hipSuccess) return fail("hipMalloc(vpl_src)", e);
    if ((e = hipMalloc((void **)&c->d_scalars, 64 * sizeof(uint32_t))) != hipSuccess) return fail("hipMalloc(scalars)", e);
    if ((e = hipMemset(c->d_scalars, 0, 64 * sizeof(uint32_t))) != hipSuccess) return fail("hipMemset", e);
    if ((e = hipMalloc((void **)&c->d_counters, sizeof(PassCounters) * EVPLP_PASS_COUNT)) != hipSuccess) return fail("hipMalloc(counters)", e);
    if ((e = hipMemset(c->d_counters, 0, sizeof(PassCounters) * EVPLP_PASS_COUNT)) != hipSuccess) return fail("hipMemset", e);
    if ((e = hipMalloc((void **)&c->d_rgb, sizeof(float) * 3 * (size_t)c->st.W * c->st.local_rows)) != hipSuccess) return fail("hipMalloc(rgb)", e);
    // splat workspace
    c->tiles_x = (c->st.W + 7) / 8; c->tiles_y = c->st.local_rows / 8;
    const size_t ntiles = (size_t)c->tiles_x * c->tiles_y;
    const size_t nrec = (size_t)cfg->num_light_paths * cfg->photons_per_path;
    // photon bins: a slab of bin_stride slots per tile, 8x the mean occupancy to start with (a power of two >= 64), doubled
    // when a bin overflows (tiles that see a floor at grazing angle collect ~10x the mean)
    {
        size_t mean = ntiles ? nrec * 2 / std::max<size_t>(ntiles, 1) : 0, k = 64;
        while (k < 8 * mean && k < (1u << 20)) k <<= 1;
        c->bin_stride = (uint32_t)k;
        if (const char *env = std::getenv("EVPLP_BIN_STRIDE")) c->bin_stride = (uint32_t)std::max(1, atoi(env));   // tests: force the overflow / re-run path
        // coarse buckets of 128 tiles (16 x 8) for the two-level binning (kernels.h); larger ones (up to 32 x 16) for images
        // that would need more than kMaxBuckets of them
        c->bucket_w_log2 = 4; c->bucket_h_log2 = kBucketTilesLog2 - 4;
        auto count_buckets = [&]() {
            c->buckets_x = (c->tiles_x + (1 << c->bucket_w_log2) - 1) >> c->bucket_w_log2;
            c->num_buckets = c->buckets_x * ((c->tiles_y + (1 << c->bucket_h_log2) - 1) >> c->bucket_h_log2);
        };
        count_buckets();
        while (c->num_buckets > kMaxBuckets && c->bucket_w_log2 + c->bucket_h_log2 < kMaxBucketTilesLog2) {
            if (c->bucket_h_log2 < c->bucket_w_log2) c->bucket_h_log2++; else c->bucket_w_log2++;
            count_buckets();
        }
        if (c->num_buckets > kMaxBuckets) {
            snprintf(g_create_error, sizeof(g_create_error), "evplp_create: more than %d x %d image tiles in one context (use row strips)", kMaxBuckets, 1 << kMaxBucketTilesLog2);
            evplp_destroy(c); return EVPLP_ERR_INVALID;
        }
        c->num_bin_groups = (int32_t)((nrec + kBinGroup - 1) / kBinGroup);
    }
    if ((e = hipMalloc((void **)&c->d_tile_box, sizeof(float4) * 2 * std::max<size_t>(ntiles, 1))) != hipSuccess) return fail("hipMalloc(tile_box)", e);
    if ((e = hipMalloc((void **)&c->d_summary, sizeof(uint32_t) * (kSummaryFinal + kSummaryStride))) != hipSuccess) return fail("hipMalloc(summary)", e);
    if (const char *env = std::getenv("EVPLP_TILE_MIXED")) c->env_tile_mixed = atoi(env) != 0 ? 1 : 0;
    if (const char *env = std::getenv("EVPLP_TILE_HEAVY")) c->heavy_threshold = (uint32_t)std::max(atoi(env), 1);
    c->mixed_trigger = 2u * c->heavy_threshold;
    if (const char *env = std::getenv("EVPLP_TILE_MIXED_TRIGGER")) c->mixed_trigger = (uint32_t)std::max(atoi(env), 0);
    c->heavy_cap = (uint32_t)std::min<size_t>(std::max<size_t>((size_t)c->tiles_x * c->tiles_y, 1), 2048);
    if (const char *env = std::getenv("EVPLP_TILE_HEAVY_CAP")) c->heavy_cap = (uint32_t)std::max(atoi(env), 1);
    if ((e = hipMalloc((void **)&c->d_heavy_list, sizeof(uint32_t) * c->heavy_cap)) != hipSuccess) return fail("hipMalloc(heavy list)", e);
    if ((e = hipMalloc((void **)&c->d_tile_flags, std::max<size_t>((size_t)c->tiles_x * c->tiles_y, 1))) != hipSuccess) return fail("hipMalloc(tile flags)", e);
    if ((e = hipMemset(c->d_summary, 0, sizeof(uint32_t) * (kSummaryFinal + kSummaryStride))) != hipSuccess) return fail("hipMemset(summary)", e);
    if ((e = hipMalloc((void **)&c->d_tile_pairs, sizeof(uint32_t) * std::max<size_t>(ntiles, 1))) != hipSuccess) return fail("hipMalloc(tile_pairs)", e);
    if ((e = hipMalloc((void **)&c->d_tile_frags, sizeof(uint32_t) * std::max<size_t>(ntiles, 1))) != hipSuccess) return fail("hipMalloc(tile_frags)", e);
    if ((e = hipMalloc((void **)&c->d_tile_cursor, sizeof(uint32_t) * (ntiles + 1))) != hipSuccess) return fail("hipMalloc(tile_cursor)", e);
    const size_t ngroups = std::max(c->num_bin_groups, 1);
    if ((e = hipMalloc((void **)&c->d_seg, sizeof(uint32_t) * ngroups * kSegCap)) != hipSuccess) return fail("hipMalloc(seg)", e);
    if ((e = hipMalloc((void **)&c->d_seg_off, sizeof(uint16_t) * ngroups * (c->num_buckets + 1))) != hipSuccess) return fail("hipMalloc(seg_off)", e);
    if ((e = hipMalloc((void **)&c->d_big_list, sizeof(uint32_t) * ngroups * kBinGroup)) != hipSuccess) return fail("hipMalloc(big_list)", e);
    if ((e = hipMalloc((void **)&c->d_big_count, sizeof(uint32_t) * ngroups)) != hipSuccess) return fail("hipMalloc(big_count)", e);
    if ((e = hipMalloc((void **)&c->d_bin_items, sizeof(uint32_t) * std::max<size_t>(ntiles * c->bin_stride, 1))) != hipSuccess) return fail("hipMalloc(bin_items)", e);
    if (cfg->deterministic && (e = hipMalloc((void **)&c->d_bin_items_tmp, sizeof(uint32_t) * std::max<size_t>(ntiles * c->bin_stride, 1))) != hipSuccess) return fail("hipMalloc(bin_items_tmp)", e);
    if ((e = hipMalloc((void **)&c->d_compact, sizeof(float4) * kCompactF4 * nrec)) != hipSuccess) return fail("hipMalloc(compact)", e);
    if ((e = hipHostMalloc((void **)&c->h_summary, 8 * sizeof(uint32_t), hipHostMallocDefault)) != hipSuccess) return fail("hipHostMalloc(summary)", e);
    std::memset(c->h_summary, 0, 8 * sizeof(uint32_t));
    for (int i = 0; i < 2; i++) {
        if ((e = hipEventCreate(&c->pend[i].ev)) != hipSuccess) return fail("hipEventCreate", e);
        c->pend[i].h = c->h_summary + 4 * i;
    }
    *out = c;
    return EVPLP_OK;
}

static void free_scene_device(evplp_context *c) {
    hipFree((void *)c->sc.nodes); hipFree((void *)c->sc.nodes4); hipFree((void *)c->sc.leaves); hipFree((void *)c->sc.tri_flat); hipFree((void *)c->sc.tri_index); hipFree((void *)c->sc.attrs);
    hipFree((void *)c->sc.materials); hipFree((void *)c->sc.textures); hipFree((void *)c->sc.tex_pool); hipFree((void *)c->sc.light_cdf);
    std::memset(&c->sc, 0, sizeof(c->sc));
    release_scene_motion(c);        // (scene_motion.cpp: the refit's plan and staging, the cost kernel's output, rest pose, skins, morph targets, the rotating sweep's scratch)
}

extern "C" void evplp_destroy(evplp_context *c) {
    if (!c) return;
    hipSetDevice(c->cfg.device);
    c->npend = 0;
    if (c->aux_stream) hipStreamSynchronize(c->aux_stream);
    if (c->own_stream) hipStreamSynchronize(c->own_stream);
    for (int b = 0; b < EVPLP_BUF_COUNT; b++) if (c->buf_owned[b]) hipFree(c->buf[b]);
    free_scene_device(c);
    release_ray_query(c);
    release_probe_gather(c);
    release_surface_gather(c);
    release_lightmap(c);
    hipFree(c->d_vpls); hipFree(c->d_vpl_src); hipFree(c->d_scalars); hipFree(c->d_counters); hipFree(c->d_rgb); hipFree(c->d_primary_cuts);
    for (DeviceScratch *s : { &c->partial, &c->lt_overflow, &c->cuts, &c->vsl_masks, &c->pt_batch, &c->pt_table }) hipFree(s->p);
    hipFree(c->d_tile_cursor); hipFree(c->d_bin_items); hipFree(c->d_bin_items_tmp); hipFree(c->d_seg); hipFree(c->d_seg_off); hipFree(c->d_big_list); hipFree(c->d_big_count);
    hipFree(c->d_compact); hipFree(c->d_tile_box); hipFree(c->d_tile_pairs); hipFree(c->d_summary); hipFree(c->d_heavy_list); hipFree(c->d_tile_flags);
    hipFree(c->d_proxy_slabs); hipFree(c->d_proxy_hm); hipFree(c->d_tile_frags); hipFree(c->d_blocks); hipFree(c->d_block_cost);
    hipFree(c->d_err_ref); hipFree(c->d_err_keep); hipFree(c->d_err_rows);
    hipFree(c->d_noise); hipFree(c->d_noise_keep); hipFree(c->d_noise_rows);
    hipFree(c->d_adapt_tiles); hipFree(c->d_adapt_snap); hipFree(c->d_adapt_mask);
    hipFree(c->d_dn_var); hipFree(c->d_dn_pack); hipFree(c->d_dn_u);
    hipFree(c->d_tp_prev_v); hipFree(c->d_tp_prev); hipFree(c->d_tp_prev_frame); hipFree(c->d_tp_hist); hipFree(c->d_tp_counts);
    hipFree(c->d_pt_first); hipFree(c->d_tile_noise);
    for (int i = 0; i < EVPLP_PASS_COUNT; i++) {
        if (c->ev_begin[i]) hipEventDestroy(c->ev_begin[i]);
        if (c->ev_end[i]) hipEventDestroy(c->ev_end[i]);
        if (c->ev_dom_begin[i]) hipEventDestroy(c->ev_dom_begin[i]);
        if (c->ev_dom_end[i]) hipEventDestroy(c->ev_dom_end[i]);
    }
    for (int i = 0; i < 2; i++) if (c->pend[i].ev) hipEventDestroy(c->pend[i].ev);
    if (c->h_summary) hipHostFree(c->h_summary);
    if (c->aux_stream) hipStreamDestroy(c->aux_stream);
    if (c->ev_records_read) hipEventDestroy(c->ev_records_read);
    if (c->ev_light_done) hipEventDestroy(c->ev_light_done);
    if (c->ev_back_read) hipEventDestroy(c->ev_back_read);
    if (c->ev_refit_staged) hipEventDestroy(c->ev_refit_staged);
    for (int i = 0; i < 5; i++) if (c->ev_refit[i]) hipEventDestroy(c->ev_refit[i]);
    for (int i = 0; i < 2; i++) if (c->ev_cost[i]) hipEventDestroy(c->ev_cost[i]);
    hipFree(c->records_back);
    for (int k = 0; k < 4; k++) hipFree(c->gbuf_back[k]);
    hipFree(c->d_tile_box_back);
    if (c->own_stream) hipStreamDestroy(c->own_stream);
    delete c;
}

extern "C" int evplp_set_stream(evplp_context *c, void *s) {
    CTX_CHECK(c);
    if (c->aux_stream) HIP_TRY(c, hipStreamSynchronize(c->aux_stream));    // (its pending wait was enqueued on the old stream)
    c->stream = s ? (hipStream_t)s : c->own_stream;
    return EVPLP_OK;
}
extern "C" int evplp_synchronize(evplp_context *c) {
    CTX_CHECK(c);
    { int rc_ = settle_splat(c); if (rc_) return rc_; }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EVPLP_OK;
}

// ------------------------------------------------------------------------------ scene upload
extern "C" int evplp_add_texture(evplp_context *c, int32_t w, int32_t h, const float *rgba) {
    CTX_CHECK(c);
    if (w <= 0 || h <= 0 || !rgba) { c->set_error("evplp_add_texture: bad arguments"); return EVPLP_ERR_INVALID; }
    HostTexture t; t.w = w; t.h = h; t.rgba.assign(rgba, rgba + (size_t)w * h * 4);
    c->textures.push_back(std::move(t));
    return (int)c->textures.size() - 1;
}
extern "C" int evplp_add_material(evplp_context *c, const evplp_material *m) {
    CTX_CHECK(c);
    if (!m) { c->set_error("evplp_add_material: null"); return EVPLP_ERR_INVALID; }
    int nt = (int)c->textures.size();
    if (m->tex_kd >= nt || m->tex_ks >= nt || m->tex_ns >= nt) { c->set_error("evplp_add_material: texture id out of range"); return EVPLP_ERR_INVALID; }
    Material d; std::memset(&d, 0, sizeof(d));
    std::memcpy(d.kd, m->kd, 12); std::memcpy(d.ks, m->ks, 12); d.ns = m->ns;
    d.tex_kd = m->tex_kd < 0 ? -1 : m->tex_kd; d.tex_ks = m->tex_ks < 0 ? -1 : m->tex_ks; d.tex_ns = m->tex_ns < 0 ? -1 : m->tex_ns;
    c->materials.push_back(d);
    return (int)c->materials.size() - 1;
}
extern "C" int evplp_add_mesh(evplp_context *c, const float *vertices, const float *texcoords, int32_t nverts,
                              const int32_t *indices, int32_t ntris, int32_t material) {
    CTX_CHECK(c);
    if (!vertices || !indices || nverts <= 0 || ntris < 0) { c->set_error("evplp_add_mesh: bad arguments"); return EVPLP_ERR_INVALID; }
    if (material < 0 || material >= (int)c->materials.size()) { c->set_error("evplp_add_mesh: material %d out of range", material); return EVPLP_ERR_INVALID; }
    for (int64_t i = 0; i < (int64_t)ntris * 3; i++) if (indices[i] < 0 || indices[i] >= nverts) { c->set_error("evplp_add_mesh: vertex index out of range"); return EVPLP_ERR_INVALID; }
    HostMesh m; m.material = material;
    m.verts.assign(vertices, vertices + (size_t)nverts * 3);
    if (texcoords) m.uvs.assign(texcoords, texcoords + (size_t)nverts * 2); else m.uvs.assign((size_t)nverts * 2, 0.0f);  // rtcommon.h:701-705
    m.idx.assign(indices, indices + (size_t)ntris * 3);
    c->meshes.push_back(std::move(m));
    c->accel_built = false;
    return (int)c->meshes.size() - 1;
}
extern "C" int evplp_set_arealight(evplp_context *c, int32_t mesh, const float intensity[4]) {
    CTX_CHECK(c);
    if (mesh < 0 || mesh >= (int)c->meshes.size() || !intensity) { c->set_error("evplp_set_arealight: bad arguments"); return EVPLP_ERR_INVALID; }
    if (c->light_mesh >= 0) { c->set_error("only one area light is supported (rt/rtcommon.h:770-774)"); return EVPLP_ERR_INVALID; }
    // rtcommon.h:780-790: xyz scaled by pi, black emitter material carrying mLightIntensity
    Material d; std::memset(&d, 0, sizeof(d));
    d.tex_kd = d.tex_ks = d.tex_ns = -1;
    const float pi = 3.14159265358979323846f;
    for (int k = 0; k < 3; k++) { c->light_unscaled[k] = intensity[k]; c->light_scaled[k] = intensity[k] * pi; }
    c->light_unscaled[3] = c->light_scaled[3] = intensity[3];
    std::memcpy(d.light, c->light_scaled, 16);
    c->materials.push_back(d);
    c->meshes[mesh].material = (int)c->materials.size() - 1;
    c->light_mesh = mesh;
    c->accel_built = false;
    return EVPLP_OK;
}
// glm::lookAt (RH) basis + glm::perspective parameters (rt/rtcommon.h:586-591); evplp_set_camera and evplp_project_points
static void camera_basis(const evplp_camera *cam, CamBasis *out) {
    auto norm = [](float *v) { float inv = 1.0f / std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); v[0] *= inv; v[1] *= inv; v[2] *= inv; };
    float f[3] = { cam->lookat[0] - cam->origin[0], cam->lookat[1] - cam->origin[1], cam->lookat[2] - cam->origin[2] };
    norm(f);
    float s[3] = { f[1] * cam->up[2] - f[2] * cam->up[1], f[2] * cam->up[0] - f[0] * cam->up[2], f[0] * cam->up[1] - f[1] * cam->up[0] };
    norm(s);
    float u[3] = { s[1] * f[2] - s[2] * f[1], s[2] * f[0] - s[0] * f[2], s[0] * f[1] - s[1] * f[0] };
    std::memset(out, 0, sizeof(*out));
    std::memcpy(out->eye, cam->origin, 12); std::memcpy(out->s, s, 12); std::memcpy(out->u, u, 12); std::memcpy(out->f, f, 12);
    out->tan_half = std::tan(cam->fovy / 2.0f); out->aspect = cam->aspect;
}
extern "C" int evplp_project_points(const evplp_camera *cam, int32_t W, int32_t H, const float *xyz, int32_t n, float *out_xyd) {
    if (!cam || W < 1 || H < 1 || n < 0 || (n > 0 && (!xyz || !out_xyd))) return EVPLP_ERR_INVALID;
    CamBasis b; camera_basis(cam, &b);
    for (int32_t i = 0; i < n; i++) { float o[3]; evplp::project_point(b, W, H, xyz + 3 * (size_t)i, o); std::memcpy(out_xyd + 3 * (size_t)i, o, 12); }
    return EVPLP_OK;
}
extern "C" int evplp_set_camera(evplp_context *c, const evplp_camera *cam) {
    CTX_CHECK(c);
    if (!cam) { c->set_error("evplp_set_camera: null"); return EVPLP_ERR_INVALID; }
    camera_basis(cam, &c->cam);
    c->cam_in = *cam;
    c->camera_set = true; c->primary_cuts_valid = false;
    return EVPLP_OK;
}

extern "C" int evplp_get_camera(evplp_context *c, evplp_camera *out) {
    CTX_CHECK(c);
    if (!out || !c->camera_set) { c->set_error("evplp_get_camera: camera not set"); return EVPLP_ERR_INVALID; }
    *out = c->cam_in;
    return EVPLP_OK;
}

template <class T> static int upload_array(evplp_context *c, const T *host, size_t n, const T **dev) {
    void *p = nullptr;
    size_t bytes = sizeof(T) * std::max<size_t>(n, 1);
    HIP_TRY(c, hipMalloc(&p, bytes));
    if (n) HIP_TRY(c, hipMemcpy(p, host, sizeof(T) * n, hipMemcpyHostToDevice));
    *dev = (const T *)p;
    return EVPLP_OK;
}

// the triangle soup in mesh order, 9 floats per triangle; first[m] = mesh m's first triangle, first[meshes] = all of them
static void flatten_verts(const evplp_context *c, std::vector<float> &verts, std::vector<int32_t> &first) {
    size_t ntri = 0;
    first.clear();
    for (const HostMesh &m : c->meshes) { first.push_back((int32_t)ntri); ntri += m.idx.size() / 3; }
    first.push_back((int32_t)ntri);
    verts.resize(9 * ntri);
    float *o = verts.data();
    for (const HostMesh &m : c->meshes)
        for (size_t i = 0; i < m.idx.size(); i++, o += 3) std::memcpy(o, &m.verts[3 * (size_t)m.idx[i]], 12);
}
// What a scene carries besides its tree: the area-light CDF, light_area and the light's padded bounds, total_area, bounding_radius, and the
// builders' box pad.  All of them are folds of per-mesh figures: mesh_figures is the one body for a mesh (evplp_build_accel runs it over every
// mesh, evplp_refit_accel over the dirty ones), light_figures the one for the light mesh, and scene_fold adds the meshes up in mesh order.
// evplp_build_accel and evplp_refit_accel (scene_motion.cpp) both come here, so a refit's figures are a fresh build's.
static float tri_area(const float *v) {              // Triangle::ComputeArea
    float a[3] = { v[3] - v[0], v[4] - v[1], v[5] - v[2] }, b[3] = { v[6] - v[0], v[7] - v[1], v[8] - v[2] };
    float cx = a[1] * b[2] - a[2] * b[1], cy = a[2] * b[0] - a[0] * b[2], cz = a[0] * b[1] - a[1] * b[0];
    return std::sqrt(cx * cx + cy * cy + cz * cz) / 2.0f;
}
namespace evplp {
// mesh m's triangles, 9 floats each, from `from` (its positions or its rest pose)
void flatten_mesh(const HostMesh &m, const std::vector<float> &from, float *o) {
    for (size_t i = 0; i < m.idx.size(); i++, o += 3) std::memcpy(o, &from[3 * (size_t)m.idx[i]], 12);
}
// scene metrics (rtcommon.h:759-768, 805-814): the mesh's running float sum of areas and the box of all its vertices; the box of its triangles
// that the builders keep (tri_has_area).  flat: the mesh's triangles (flatten_mesh); has_area: null, or one byte per triangle of the mesh
void mesh_figures(HostMesh &m, const float *flat, char *has_area) {
    float ms = 0.f;
    for (int k = 0; k < 3; k++) { m.lo[k] = 3.4028235e38f; m.hi[k] = -3.4028235e38f; m.alo[k] = 3.0e38f; m.ahi[k] = -3.0e38f; }
    m.any_area = false;
    for (size_t t = 0; t < m.idx.size() / 3; t++) {
        const float *v = flat + 9 * t;
        ms += tri_area(v);
        const bool has = tri_has_area(v);
        if (has_area) has_area[t] = has;
        if (!has) continue;
        m.any_area = true;
        for (int k = 0; k < 9; k++) { m.alo[k % 3] = std::min(m.alo[k % 3], v[k]); m.ahi[k % 3] = std::max(m.ahi[k % 3], v[k]); }
    }
    m.area = ms;
    for (size_t v = 0; v < m.verts.size() / 3; v++) for (int k = 0; k < 3; k++) { m.lo[k] = std::min(m.lo[k], m.verts[3 * v + k]); m.hi[k] = std::max(m.hi[k], m.verts[3 * v + k]); }
}
// area-light CDF, rt/rtcommon.h:501-531 (running float sum, then normalised), light_area, and the unpadded bounds of the light's triangles
// (flat: the light mesh's triangles)
void light_figures(evplp_context *c, const float *flat, std::vector<float> &cdf) {
    const size_t n = c->meshes[(size_t)c->light_mesh].idx.size() / 3;
    cdf.resize(n);
    float sum = 0.f;
    for (int k = 0; k < 3; k++) { c->light_box_lo[k] = 3.0e38f; c->light_box_hi[k] = -3.0e38f; }
    for (size_t i = 0; i < n; i++) {
        const float *v = flat + 9 * i;
        sum += tri_area(v); cdf[i] = sum;
        for (int k = 0; k < 9; k++) { c->light_box_lo[k % 3] = std::min(c->light_box_lo[k % 3], v[k]); c->light_box_hi[k % 3] = std::max(c->light_box_hi[k % 3], v[k]); }
    }
    for (size_t i = 0; i < n; i++) cdf[i] /= sum;
    c->light_area = sum; c->sc.light_area = sum;
}
// the meshes' figures in mesh order; returns the builders' box pad for the bounds of the triangles they keep
float scene_fold(evplp_context *c) {
    float total = 0.f; float lo[3] = { 3.4028235e38f, 3.4028235e38f, 3.4028235e38f }, hi[3] = { -3.4028235e38f, -3.4028235e38f, -3.4028235e38f };
    float alo[3] = { 3.0e38f, 3.0e38f, 3.0e38f }, ahi[3] = { -3.0e38f, -3.0e38f, -3.0e38f };
    bool any = false;
    for (const HostMesh &m : c->meshes) {
        total += m.area; any = any || m.any_area;
        for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], m.lo[k]); hi[k] = std::max(hi[k], m.hi[k]); alo[k] = std::min(alo[k], m.alo[k]); ahi[k] = std::max(ahi[k], m.ahi[k]); }
    }
    float dg[3] = { std::max(hi[0] - lo[0], 0.f), std::max(hi[1] - lo[1], 0.f), std::max(hi[2] - lo[2], 0.f) };
    c->bounding_radius = std::sqrt(dg[0] * dg[0] + dg[1] * dg[1] + dg[2] * dg[2]) / 2.0f;
    c->total_area = total;
    // bounds of the light mesh, padded by far more than the rounding of a slab test
    const float pad = 1e-4f * (2.0f * c->bounding_radius) + 1e-30f;
    for (int k = 0; k < 3; k++) { c->sc.light_lo[k] = c->light_box_lo[k] - pad; c->sc.light_hi[k] = c->light_box_hi[k] + pad; }
    return bvh_pad(alo, ahi, any);
}

// evplp_build_accel, and the rebuild of a refit policy (policy_builder >= 0: that builder instead of the context's own)
int build_accel(evplp_context *c, int policy_builder) {
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    if (c->meshes.empty()) { c->set_error("evplp_build_accel: no meshes"); return EVPLP_ERR_INVALID; }
    if (c->light_mesh < 0) { c->set_error("evplp_build_accel: no area light set"); return EVPLP_ERR_INVALID; }
    free_scene_device(c);
    // flatten to a triangle soup in mesh order
    std::vector<float> verts; std::vector<int32_t> first; std::vector<TriAttr> attrs;
    flatten_verts(c, verts, first);
    attrs.reserve((size_t)first.back());
    for (size_t mi = 0; mi < c->meshes.size(); mi++) {
        const HostMesh &m = c->meshes[mi];
        for (size_t t = 0; t < m.idx.size() / 3; t++) {
            TriAttr a; std::memset(&a, 0, sizeof(a));
            std::memcpy(a.v, &verts[9 * attrs.size()], sizeof(a.v));
            for (int k = 0; k < 3; k++) { const int32_t vi = m.idx[3 * t + k]; a.uv[2 * k] = m.uvs[2 * (size_t)vi]; a.uv[2 * k + 1] = m.uvs[2 * (size_t)vi + 1]; }
            a.material = m.material;
            attrs.push_back(a);
        }
    }
    const int32_t light_first = first[(size_t)c->light_mesh], light_count = first[(size_t)c->light_mesh + 1] - light_first;
    if (light_count <= 0) { c->set_error("evplp_build_accel: the area-light mesh has no triangles"); return EVPLP_ERR_INVALID; }
    BvhBuild bb;
    int builder = policy_builder >= 0 ? policy_builder : c->env_bvh_builder >= 0 ? c->env_bvh_builder : c->cfg.bvh_builder;   // (override read by evplp_create)
    const bool on_device = builder == EVPLP_BVH_LBVH_GPU || builder == EVPLP_BVH_PLOC_GPU;
    if (on_device) {
        BvhDeviceBuild gb;
        const bool ploc = builder == EVPLP_BVH_PLOC_GPU;
        const int e = ploc ? build_bvh_gpu(verts.data(), (int32_t)attrs.size(), bvh_pad_scale(), c->stream, &gb, c->env_ploc_radius > 0 ? c->env_ploc_radius : kPlocRadius,
                                           c->env_ploc_iterations >= 0 ? c->env_ploc_iterations : kPlocSearchIterations)
                           : build_bvh_gpu(verts.data(), (int32_t)attrs.size(), bvh_pad_scale(), c->stream, &gb);
        if (e != 0) { c->set_error("evplp_build_accel: device %s build: %s", ploc ? "PLOC" : "LBVH", hipGetErrorString((hipError_t)e)); return EVPLP_ERR_HIP; }
        if (gb.bound_passed) { c->set_error("evplp_build_accel: device PLOC build: %d iterations and still more than one cluster (the bound is the search iterations + log2 of the triangles)", gb.iterations); return EVPLP_ERR_HIP; }
        if (gb.depth > kMaxDepth - 2) {
            // long radix-tree chains (clustered or duplicate Morton codes) or a tall PLOC tree can exceed the walks' 64-entry stacks: build
            // the binned-SAH tree on the host instead of failing the scene
            hipFree(gb.nodes); hipFree(gb.leaves); hipFree(gb.tri_flat); hipFree(gb.tri_index);
            builder = EVPLP_BVH_SAH;
        } else {
            c->sc.nodes = gb.nodes; c->sc.leaves = gb.leaves; c->sc.tri_flat = gb.tri_flat; c->sc.tri_index = gb.tri_index;
            bb.nnodes = gb.nnodes; bb.nleaves = gb.nleaves; bb.depth = gb.depth; bb.build_ms = gb.build_ms; bb.ntris = gb.ntris;
        }
    }
    if (builder != EVPLP_BVH_LBVH_GPU && builder != EVPLP_BVH_PLOC_GPU) {
        build_bvh(verts.data(), (int32_t)attrs.size(), builder, &bb);
        if (bb.depth > kMaxDepth - 2 && builder == EVPLP_BVH_LBVH) { free_bvh(&bb); bb = BvhBuild(); builder = EVPLP_BVH_SAH; build_bvh(verts.data(), (int32_t)attrs.size(), builder, &bb); }
    }
    c->accel_builder_used = builder;
    c->accel_nodes = bb.nnodes; c->accel_leaves = bb.nleaves; c->accel_depth = bb.depth; c->accel_build_ms = bb.build_ms;
    if (bb.depth > kMaxDepth - 2) { free_bvh(&bb); free_scene_device(c); c->set_error("BVH depth %d exceeds the traversal stack (%d)", bb.depth, kMaxDepth); return EVPLP_ERR_INVALID; }
    std::vector<float> cdf;
    {   // which triangles the builders dropped (a refit cannot bring one back), and the builders' pad of this scene
        std::vector<char> has_area((size_t)first.back(), 0);
        for (size_t mi = 0; mi < c->meshes.size(); mi++) mesh_figures(c->meshes[mi], &verts[9 * (size_t)first[mi]], has_area.data() + first[mi]);
        light_figures(c, &verts[9 * (size_t)light_first], cdf);
        c->accel_pad = scene_fold(c);
        c->tri_dropped.resize(has_area.size());
        for (size_t t = 0; t < has_area.size(); t++) c->tri_dropped[t] = !has_area[t];
    }
    c->scene_tris = first.back();
    const float sum = c->light_area;

    // textures -> one float4 pool
    std::vector<TexDesc> tdesc; std::vector<float4> pool;
    for (const HostTexture &t : c->textures) {
        TexDesc d; d.w = t.w; d.h = t.h; d.offset = (uint32_t)pool.size(); d.pad = 0;
        for (size_t i = 0; i < (size_t)t.w * t.h; i++) pool.push_back(make_float4(t.rgba[4 * i], t.rgba[4 * i + 1], t.rgba[4 * i + 2], t.rgba[4 * i + 3]));
        tdesc.push_back(d);
    }
    int rc;
    if (builder != EVPLP_BVH_LBVH_GPU && builder != EVPLP_BVH_PLOC_GPU) {
        if ((rc = upload_array(c, bb.nodes, (size_t)bb.nnodes, &c->sc.nodes))) { free_bvh(&bb); return rc; }
        if ((rc = upload_array(c, bb.leaves, (size_t)std::max(bb.nleaves, 1), &c->sc.leaves))) { free_bvh(&bb); return rc; }
        if ((rc = upload_array(c, bb.tri_index, (size_t)std::max(bb.nleaves, 1) * 4, &c->sc.tri_index))) { free_bvh(&bb); return rc; }
        if ((rc = upload_array(c, bb.tri_flat, (size_t)std::max(bb.nleaves, 1) * 4, &c->sc.tri_flat))) { free_bvh(&bb); return rc; }
    }
    c->sc.ntris = bb.ntris; c->sc.bvh_depth = bb.depth;
    {
        // Worst-case stack of the four-wide per-lane walk (closest_lane4: a visit pushes every entered grandchild but the nearest) over
        // the tree that was built: need(i) = (grandchildren of i) - 1 + max over inner grandchildren g of need(g).  Inner nodes are stored in
        // pre-order (children after parents), so one backward sweep does it.  The LDS stack is what limits the occupancy of light tracing.
        // (the device builder's nodes come back once, here; the copy is kept for the level plan of a refit)
        std::vector<BvhNode> &host_nodes = c->host_nodes;
        const BvhNode *hn = bb.nodes;
        if (!hn) { host_nodes.resize((size_t)bb.nnodes); HIP_TRY(c, hipMemcpy(host_nodes.data(), c->sc.nodes, sizeof(BvhNode) * (size_t)bb.nnodes, hipMemcpyDeviceToHost)); hn = host_nodes.data(); }
        std::vector<int32_t> need((size_t)bb.nnodes, 0);
        bool ordered = true;
        for (int32_t i = bb.nnodes - 1; i >= 0; i--) {
            int32_t g[4]; int m = 0;
            const int32_t ch[2] = { hn[i].c0, hn[i].c1 };
            for (int s2 = 0; s2 < 2; s2++) {
                if (ch[s2] >= 0) { if (ch[s2] <= i) ordered = false; g[m++] = hn[ch[s2]].c0; g[m++] = hn[ch[s2]].c1; }
                else if (ch[s2] != kNoChild) g[m++] = ch[s2];
            }
            int32_t valid = 0, deepest = 0;
            for (int q = 0; q < m; q++) if (g[q] != kNoChild) { valid++; if (g[q] >= 0) { if (g[q] <= i) ordered = false; else deepest = std::max(deepest, need[(size_t)g[q]]); } }
            need[(size_t)i] = std::max(valid - 1, 0) + deepest;
        }
        c->sc.stack4_entries = ordered && bb.nnodes > 0 ? need[0] + 2 : 0;      // (0: not pre-ordered -- the generic bound of the depth applies)
    }
    { BvhNode4 *n4 = nullptr; const int e4 = build_nodes4(c->sc.nodes, bb.nnodes, c->stream, &n4);
      if (e4 != 0) { free_bvh(&bb); c->set_error("evplp_build_accel: four-wide nodes: %s", hipGetErrorString((hipError_t)e4)); return EVPLP_ERR_HIP; }
      c->sc.nodes4 = n4; }
    free_bvh(&bb);
    if ((rc = upload_array(c, attrs.data(), attrs.size(), &c->sc.attrs))) return rc;
    if ((rc = upload_array(c, c->materials.data(), c->materials.size(), &c->sc.materials))) return rc;
    if ((rc = upload_array(c, tdesc.data(), tdesc.size(), &c->sc.textures))) return rc;
    if ((rc = upload_array(c, pool.data(), pool.size(), &c->sc.tex_pool))) return rc;
    if ((rc = upload_array(c, cdf.data(), cdf.size(), &c->sc.light_cdf))) return rc;
    c->sc.light_first = light_first; c->sc.light_count = light_count; c->sc.light_area = sum;
    std::memcpy(c->sc.light_intensity, c->light_scaled, 16); std::memcpy(c->sc.light_unscaled, c->light_unscaled, 16);
    c->accel_built = true; c->primary_cuts_valid = false; c->primary_current = false;
    c->mesh_dirty.assign(c->meshes.size(), MeshDirty::Clean); c->scene_dirty = false;
    c->built_cost = 0.0; c->built_cost_known = false; c->refits_since_build = 0; c->rotations_since_build = 0;
    if (c->policy_ratio > 0.0) {            // (a policy compares against the cost of the tree as built: one small launch and a wait)
        double q[5];
        if ((rc = measure_cost(c, q))) return rc;
    }
    return EVPLP_OK;
}
}
extern "C" int evplp_build_accel(evplp_context *c) {
    CTX_CHECK(c);
    const int rc = build_accel(c, -1);
    if (rc == EVPLP_OK) c->last_action = 0;
    return rc;
}

extern "C" int evplp_scene_metrics(evplp_context *c, float *r, float *total, float *light) {
    CTX_CHECK(c);
    if (!c->accel_built) { c->set_error("evplp_scene_metrics: call evplp_build_accel first"); return EVPLP_ERR_INVALID; }
    if (r) *r = c->bounding_radius; if (total) *total = c->total_area; if (light) *light = c->light_area;
    return EVPLP_OK;
}
extern "C" int evplp_accel_stack_entries(const evplp_context *c) { return (c && c->accel_built) ? c->sc.stack4_entries : -1; }
extern "C" int evplp_accel_info(evplp_context *c, int32_t *nodes, int32_t *leaves, int32_t *depth, float *build_ms) {
    CTX_CHECK(c);
    if (nodes) *nodes = c->accel_nodes; if (leaves) *leaves = c->accel_leaves; if (depth) *depth = c->accel_depth; if (build_ms) *build_ms = c->accel_build_ms;
    return EVPLP_OK;
}

extern "C" int evplp_accel_builder(const evplp_context *c) {
    if (!c || !c->accel_built) return -1;
    return c->accel_builder_used;
}

extern "C" int evplp_debug_accel(evplp_context *c, int32_t which, void *host_dst, size_t bytes) {
    CTX_CHECK(c);
    if (!c->accel_built || !host_dst) { c->set_error("evplp_debug_accel: no scene (evplp_build_accel) or a null destination"); return EVPLP_ERR_INVALID; }
    const size_t nn = (size_t)std::max(c->accel_nodes, 1), nl = (size_t)std::max(c->accel_leaves, 1);
    const void *src[5] = { c->sc.nodes, c->sc.leaves, c->sc.tri_flat, c->sc.tri_index, c->sc.nodes4 };
    const size_t want[8] = { sizeof(BvhNode) * nn, sizeof(LeafBlock) * nl, sizeof(TriFlat) * 4 * nl, sizeof(int32_t) * 4 * nl, sizeof(BvhNode4) * nn, sizeof(float), sizeof(float) * 4, sizeof(float) };
    if (which < 0 || which > 7 || bytes != want[which]) { c->set_error("evplp_debug_accel: array %d holds %zu bytes, not %zu", which, which >= 0 && which <= 7 ? want[which] : (size_t)0, bytes); return EVPLP_ERR_INVALID; }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    if (which == 5) { std::memcpy(host_dst, &c->accel_pad, sizeof(float)); return EVPLP_OK; }
    if (which == 6) {                       // the last refit's stages in ms: upload, leaf operands, boxes, four-wide nodes (zeros unless evplp_profile_kernels was on)
        float ms[4] = { 0.f, 0.f, 0.f, 0.f };
        if (c->refit_count > 0 && c->refit_stages_timed) {
            HIP_TRY(c, hipEventSynchronize(c->ev_refit[4]));
            for (int i = 0; i < 4; i++) HIP_TRY(c, hipEventElapsedTime(&ms[i], c->ev_refit[i], c->ev_refit[i + 1]));
        }
        std::memcpy(host_dst, ms, sizeof(ms));
        return EVPLP_OK;
    }
    if (which == 7) {                       // the last cost measurement in ms, the kernel and the copy of its sums (zero unless evplp_profile_passes was on)
        float ms = 0.f;
        if (c->cost_timed) HIP_TRY(c, hipEventElapsedTime(&ms, c->ev_cost[0], c->ev_cost[1]));
        std::memcpy(host_dst, &ms, sizeof(ms));
        return EVPLP_OK;
    }
    HIP_TRY(c, hipMemcpyAsync(host_dst, src[which], bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EVPLP_OK;
}

// ---------------------------------------------------------------------------------- passes
// Look at the bin summary of the last photon splat (see context.hpp).  Called at the start of every entry point that
// enqueues work, reads results or changes buffers.  Overflow is rare (the bins carry 25 % slack over the last pass and the
// radius only shrinks in a progressive run): then the bins grow and fill + tiles of that pass run again -- they wrote nothing.
// fullest bin from which the tile kernel runs four waves per tile (evplp_splat_photons explains; EVPLP_SPLIT_MIN: developer override)
static uint32_t split_threshold(const evplp_context *c, uint32_t footprint) {
    if (c->env_split_min > 0) return (uint32_t)c->env_split_min;
    // (the proxy variant keeps its four waves busy only in much fuller bins: at config #3, fullest bin ~1400, one wave per tile takes 136 us
    // and four take 178; the ideal kernel 87 / 82)
    return footprint == (uint32_t)EVPLP_FOOTPRINT_PROXY ? 1536u : 768u;
}
static int settle_one(evplp_context *c) {                                // the oldest pending pass
    if (c->npend == 0) return EVPLP_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipEventSynchronize(c->pend[0].ev));
    const uint32_t total = c->pend[0].h[0], biggest = c->pend[0].h[1], overflow = c->pend[0].h[2];
    SplatArgs a = c->pend[0].args;
    std::swap(c->pend[0], c->pend[1]); c->npend--;                       // (the slot keeps its event and its pinned words)
    c->last_bin_entries = total; c->last_bin_max = biggest;
    if (!overflow) return EVPLP_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    uint64_t want = 64; while (want < (uint64_t)overflow + overflow / 4) want <<= 1;     // overflow = slots the fullest bin wanted
    const size_t ntiles = (size_t)c->tiles_x * c->tiles_y;
    if (want * ntiles > 0xfffffff0ull) { c->set_error("photon bins: %llu slots per tile needed", (unsigned long long)overflow); return EVPLP_ERR_OOM; }
    if (want > c->bin_stride) {                                          // (a younger pending pass may have grown them already)
        hipFree(c->d_bin_items); c->d_bin_items = nullptr;
        if (c->d_bin_items_tmp) { hipFree(c->d_bin_items_tmp); c->d_bin_items_tmp = nullptr; }
        hipError_t e1 = hipMalloc((void **)&c->d_bin_items, sizeof(uint32_t) * ntiles * want);
        hipError_t e2 = c->cfg.deterministic ? hipMalloc((void **)&c->d_bin_items_tmp, sizeof(uint32_t) * ntiles * want) : hipSuccess;
        if (e1 != hipSuccess || e2 != hipSuccess) { c->set_error("photon bins: cannot allocate %zu x %llu slots", ntiles, (unsigned long long)want); return EVPLP_ERR_OOM; }
        c->bin_stride = (uint32_t)want;
    }
    a.bin_items = c->d_bin_items; a.bin_items_tmp = c->d_bin_items_tmp; a.bin_stride = c->bin_stride;
    for (int i = 0; i < c->npend; i++) {                                 // a younger pass ran with the old slabs: if IT has to run again, then with these
        c->pend[i].args.bin_items = c->d_bin_items; c->pend[i].args.bin_items_tmp = c->d_bin_items_tmp; c->pend[i].args.bin_stride = c->bin_stride;
    }
    HIP_TRY(c, hipEventRecord(c->ev_begin[EVPLP_PASS_SPLAT], c->stream));  // (the pass statistics then describe this re-run as a whole, not a mix of two passes)
    c->pass_timed[EVPLP_PASS_SPLAT] = true;
    launch_splat_bin(a, c->stream);                                       // (clears the overflow flag, the cursors and the summary)
    const bool split_tiles = c->cfg.deterministic ? true : biggest >= split_threshold(c, a.fp.splat_footprint);
    launch_splat_tiles(a, split_tiles, c->stream, c->ev_dom_begin[EVPLP_PASS_SPLAT], c->ev_dom_end[EVPLP_PASS_SPLAT]);
    HIP_TRY(c, hipEventRecord(c->ev_end[EVPLP_PASS_SPLAT], c->stream));
    // (the records this pass read may meanwhile be the BACK buffer of the overlapped light tracing: its readers' event then)
    if (c->aux_stream) HIP_TRY(c, hipEventRecord((const void *)a.records == c->buf[EVPLP_BUF_RECORDS] ? c->ev_records_read : c->ev_back_read, c->stream));
    HIP_TRY(c, hipGetLastError());
    return EVPLP_OK;
}
static int settle_splat(evplp_context *c) {
    while (c->npend > 0) { int rc = settle_one(c); if (rc) return rc; }
    return EVPLP_OK;
}
// the pending passes that read `records` or the G-buffer whose position plane is `g_pos` (and every older one) must be settled
// before those are overwritten
static int settle_readers_of(evplp_context *c, const void *records, const void *g_pos) {
    int upto = 0;
    for (int i = 0; i < c->npend; i++)
        if ((records && (const void *)c->pend[i].args.records == records) || (g_pos && (const void *)c->pend[i].args.g_pos == g_pos)) upto = i + 1;
    for (int i = 0; i < upto; i++) { int rc = settle_one(c); if (rc) return rc; }
    return EVPLP_OK;
}
static int pass_ready(evplp_context *c, const char *name, bool need_camera, bool settle = true) {
    if (!c->accel_built) { c->set_error("%s: scene not built (evplp_build_accel)", name); return EVPLP_ERR_INVALID; }
    if (c->scene_dirty) { c->set_error("%s: vertices were updated (evplp_update_mesh): call evplp_refit_accel or evplp_build_accel first", name); return EVPLP_ERR_INVALID; }
    if (need_camera && !c->camera_set) { c->set_error("%s: camera not set", name); return EVPLP_ERR_INVALID; }
    hipError_t e = hipSetDevice(c->cfg.device);
    if (e != hipSuccess) { c->set_error("hipSetDevice: %s", hipGetErrorString(e)); return EVPLP_ERR_HIP; }
    return settle ? settle_splat(c) : EVPLP_OK;
}
// device counters are written by the gathers and the path tracer (and by the counters build of the splat)
#ifndef EVPLP_TRAVERSAL_STATS
#define EVPLP_TRAVERSAL_STATS 0
#endif
static bool pass_uses_counters(int pass) {
    return pass == EVPLP_PASS_GATHER_VPL || pass == EVPLP_PASS_GATHER_VSL || pass == EVPLP_PASS_GATHER_LVC || pass == EVPLP_PASS_PATH_TRACE || EVPLP_TRAVERSAL_STATS || EVPLP_DEBUG_NAN;
}
// Every recorded event is a marker the command processor has to retire between two dispatches: the two per pass cost config #4's
// 0.6 ms iteration 18 us (measured, round 5).  evplp_profile_passes(ctx, 0) leaves only the events the library itself waits on.
static int pass_begin(evplp_context *c, int pass) {
    if (pass_uses_counters(pass)) HIP_TRY(c, hipMemsetAsync(&c->d_counters[pass], 0, sizeof(PassCounters), c->stream));
    if (c->profile_passes || pass == EVPLP_PASS_PRIMARY) HIP_TRY(c, hipEventRecord(c->ev_begin[pass], c->stream));    // (the overlapped light tracing starts beside the G-buffer pass)
    c->pass_ran[pass] = true; c->pass_has_dom[pass] = false; c->pass_timed[pass] = c->profile_passes;
    return EVPLP_OK;
}
static int pass_end(evplp_context *c, int pass) {
    if (c->pass_timed[pass]) HIP_TRY(c, hipEventRecord(c->ev_end[pass], c->stream));
    if (c->aux_stream && (pass == EVPLP_PASS_GATHER_VPL || pass == EVPLP_PASS_GATHER_VSL || pass == EVPLP_PASS_GATHER_LVC || pass == EVPLP_PASS_SPLAT))
        HIP_TRY(c, hipEventRecord(c->ev_records_read, c->stream));
    HIP_TRY(c, hipGetLastError());
    return EVPLP_OK;
}

static bool jitter_within_cuts(const evplp_context *c, const float jitter[2]) {
    return std::fabs(jitter[0]) <= 1.99f / (float)c->st.W && std::fabs(jitter[1]) <= 1.99f / (float)c->st.H;
}
// the eye's entry cuts: once per camera / tree (they hold for every jitter up to a pixel), 256 B per group of 2 x 2 tiles (2 x 1 where a
// strip's tile rows are not neighbours in the image); built on the stream if they are stale, and named in a (left alone if they cannot be had)
static void primary_cuts_into(evplp_context *c, PrimaryArgs &a) {
    PrimaryCutArgs pc; std::memset(&pc, 0, sizeof(pc));
    pc.nodes = c->sc.nodes; pc.st = c->st; pc.cam = c->cam; pc.tiles_x = c->tiles_x; pc.tiles_y = c->tiles_y;
    pc.gw_log2 = 1; pc.gh_log2 = tile_rows_are_neighbours(c->st.strip_count, c->st.strip_rows) ? 1 : 0;
    pc.groups_x = (c->tiles_x + (1 << pc.gw_log2) - 1) >> pc.gw_log2; pc.groups_y = (c->tiles_y + (1 << pc.gh_log2) - 1) >> pc.gh_log2;
    if (!c->d_primary_cuts) {
        hipError_t me = hipMalloc((void **)&c->d_primary_cuts, (size_t)pc.groups_x * pc.groups_y * (size_t)kCutSlotBytes);
        if (me != hipSuccess) { (void)hipGetLastError(); c->d_primary_cuts = nullptr; }
        c->primary_cuts_valid = false;
    }
    if (c->d_primary_cuts) {
        pc.cuts = c->d_primary_cuts;
        if (!c->primary_cuts_valid) { launch_primary_cuts(pc, c->stream); c->primary_cuts_valid = true; }
        a.cuts = c->d_primary_cuts; a.cut_gw_log2 = pc.gw_log2; a.cut_gh_log2 = pc.gh_log2; a.cut_groups_x = pc.groups_x;
    }
}

extern "C" int evplp_primary(evplp_context *c, const float jitter[2], int32_t clear_light) {
    CTX_CHECK(c);
    // A pending photon splat may have to run again from the G-buffer it was given (settle_splat).  With overlap_light_tracing the
    // G-buffer is double-buffered like the records: this pass writes the set that splat does not read and the host does not wait here
    // (every reader of that set is in front of this pass on the same stream).
    static const int kPlanes[4] = { EVPLP_BUF_GBUF_POSITION, EVPLP_BUF_GBUF_NORMAL, EVPLP_BUF_GBUF_DIFFUSE, EVPLP_BUF_GBUF_PHONG };
    bool flip = c->aux_stream && c->npend > 0 && !c->gbuf_exposed && !c->gbuf_pos_exposed;
    for (int k = 0; k < 4 && flip; k++) flip = c->buf_owned[kPlanes[k]];
    int rc = pass_ready(c, "evplp_primary", true, !flip); if (rc) return rc;
    if (flip && c->gbuf_back[0] && (rc = settle_readers_of(c, nullptr, c->gbuf_back[0]))) return rc;      // (a splat two passes old: long finished)
    if (flip) {
        for (int k = 0; k < 4; k++) if (!c->gbuf_back[k]) {
            hipError_t me = hipMalloc(&c->gbuf_back[k], buffer_bytes(c, kPlanes[k]));
            if (me != hipSuccess) { c->set_error("evplp_primary: second G-buffer: %s", hipGetErrorString(me)); return EVPLP_ERR_OOM; }
        }
        if (!c->d_tile_box_back) {
            hipError_t me = hipMalloc((void **)&c->d_tile_box_back, sizeof(float4) * 2 * std::max<size_t>((size_t)c->tiles_x * c->tiles_y, 1));
            if (me != hipSuccess) { c->set_error("evplp_primary: second tile-box table: %s", hipGetErrorString(me)); return EVPLP_ERR_OOM; }
        }
        for (int k = 0; k < 4; k++) std::swap(c->buf[kPlanes[k]], c->gbuf_back[k]);
        std::swap(c->d_tile_box, c->d_tile_box_back);
    }
    PrimaryArgs a; std::memset(&a, 0, sizeof(a));
    a.sc = c->sc; a.st = c->st; a.cam = c->cam;
    a.jitter[0] = jitter ? jitter[0] : 0.f; a.jitter[1] = jitter ? jitter[1] : 0.f; a.clear_light = clear_light;
    a.g_pos = (float4 *)c->buf[EVPLP_BUF_GBUF_POSITION]; a.g_nrm = (float4 *)c->buf[EVPLP_BUF_GBUF_NORMAL];
    a.g_dif = (float4 *)c->buf[EVPLP_BUF_GBUF_DIFFUSE]; a.g_phg = (float4 *)c->buf[EVPLP_BUF_GBUF_PHONG];
    a.g_light = (float4 *)c->buf[EVPLP_BUF_LIGHT];
    a.tile_box = c->d_tile_box;
    if (!std::isfinite(a.jitter[0]) || !std::isfinite(a.jitter[1])) { c->set_error("evplp_primary: jitter is not finite"); return EVPLP_ERR_INVALID; }
    // The eye's cuts are built for a pyramid opened by ONE PIXEL (2 / W, 2 / H in NDC) around every tile group (primary_cut_kernel): they
    // hold for the reference's jitter, (2u - 1) / resolution -- half a pixel at most (rtcomphoton.h:949) -- and for anything up to a whole
    // pixel.  A larger translation (the ABI takes any float) moves rays out of their group's pyramid: that call walks from the root.
    if (c->env_cuts != 0 && c->tiles_x * c->tiles_y > 0 && jitter_within_cuts(c, a.jitter)) primary_cuts_into(c, a);
    if ((rc = pass_begin(c, EVPLP_PASS_PRIMARY))) return rc;
    launch_primary(a, c->stream);
    c->tile_box_valid = !c->gbuf_pos_exposed;
    // (evplp_denoise_temporal repeats this walk: its jitter and flags, and whether the position plane in memory is this pass's own)
    c->primary_jitter[0] = a.jitter[0]; c->primary_jitter[1] = a.jitter[1]; c->primary_flags = clear_light;
    c->primary_current = c->buf_owned[EVPLP_BUF_GBUF_POSITION] && !c->gbuf_pos_exposed;
    c->stats_host[EVPLP_PASS_PRIMARY].rays = 2ull * (uint64_t)c->st.W * c->rows_in_image;
    return pass_end(c, EVPLP_PASS_PRIMARY);
}

extern "C" int evplp_trace_light_paths(evplp_context *c, uint32_t rng_seed, uint32_t path_begin, uint32_t path_count) {
    CTX_CHECK(c);
    // A photon splat that is still in flight may have to run again (bins too small: settle_splat), from the records and the G-buffer
    // it was given.  Waiting for its verdict here stalls the host once per iteration -- unless these light paths go to the OTHER
    // record buffer (double buffering below): then the pending splat keeps its inputs and the next evplp_primary settles it.
    const bool to_back_buffer = c->aux_stream && path_begin == 0 && path_count == c->cfg.num_light_paths && c->buf_owned[EVPLP_BUF_RECORDS] && !c->records_exposed;
    int rc = pass_ready(c, "evplp_trace_light_paths", false, !to_back_buffer); if (rc) return rc;
    if (to_back_buffer && c->records_back && (rc = settle_readers_of(c, c->records_back, nullptr))) return rc;   // (a splat two passes old)
    if ((uint64_t)path_begin + path_count > c->cfg.num_light_paths) { c->set_error("evplp_trace_light_paths: path range exceeds num_light_paths"); return EVPLP_ERR_INVALID; }
    LightTraceArgs a; std::memset(&a, 0, sizeof(a));
    a.sc = c->sc; a.rng_seed = rng_seed; a.path_begin = path_begin; a.path_count = path_count; a.photons_per_path = c->cfg.photons_per_path;
    a.records = (evplp_record *)c->buf[EVPLP_BUF_RECORDS];
    {   // overflow columns of the walk stack (kernels.h): sized for the largest launch so far
        const size_t threads = ((size_t)path_count + 63) / 64 * 64, need = threads * (size_t)lt_overflow_entries(c->sc) * sizeof(int32_t);
        const hipError_t me = grow_scratch(c, c->lt_overflow, need);
        if (me != hipSuccess) { c->set_error("evplp_trace_light_paths: stack overflow area: %s", hipGetErrorString(me)); return EVPLP_ERR_OOM; }
        a.stack_overflow = (int32_t *)c->lt_overflow.p; a.overflow_stride = (uint32_t)threads;
    }
    if (!c->aux_stream) {
        if ((rc = pass_begin(c, EVPLP_PASS_LIGHT_TRACE))) return rc;
        launch_light_trace(a, c->stream);
        return pass_end(c, EVPLP_PASS_LIGHT_TRACE);
    }
    // overlapped: behind the last reader of the records, beside whatever the main stream is doing now (the G-buffer pass of
    // this iteration), in front of everything the main stream is given from here on
    if (to_back_buffer) {
        // double buffer: write the records nobody reads any more, and make them EVPLP_BUF_RECORDS for every later call
        if (!c->records_back) {
            hipError_t me = hipMalloc(&c->records_back, buffer_bytes(c, EVPLP_BUF_RECORDS));
            if (me != hipSuccess) { c->set_error("evplp_trace_light_paths: second record buffer: %s", hipGetErrorString(me)); return EVPLP_ERR_OOM; }
        }
        std::swap(c->buf[EVPLP_BUF_RECORDS], c->records_back);
        std::swap(c->ev_records_read, c->ev_back_read);                  // (the event of the readers of the buffer that is now in front)
        a.records = (evplp_record *)c->buf[EVPLP_BUF_RECORDS];
    }
    HIP_TRY(c, hipStreamWaitEvent(c->aux_stream, c->ev_records_read, 0));
    // ... and not before the G-buffer pass most recently given to the main stream starts: a caller that calls evplp_primary first wants
    // the light paths beside IT, not beside the long gather that may still be running in front of it (they would share its CUs)
    if (c->pass_ran[EVPLP_PASS_PRIMARY]) HIP_TRY(c, hipStreamWaitEvent(c->aux_stream, c->ev_begin[EVPLP_PASS_PRIMARY], 0));
    if (c->profile_passes) HIP_TRY(c, hipEventRecord(c->ev_begin[EVPLP_PASS_LIGHT_TRACE], c->aux_stream));
    c->pass_ran[EVPLP_PASS_LIGHT_TRACE] = true; c->pass_has_dom[EVPLP_PASS_LIGHT_TRACE] = false; c->pass_timed[EVPLP_PASS_LIGHT_TRACE] = c->profile_passes;
    launch_light_trace(a, c->aux_stream);
    if (c->profile_passes) HIP_TRY(c, hipEventRecord(c->ev_end[EVPLP_PASS_LIGHT_TRACE], c->aux_stream));
    HIP_TRY(c, hipEventRecord(c->ev_light_done, c->aux_stream));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_light_done, 0));
    HIP_TRY(c, hipGetLastError());
    return EVPLP_OK;
}

// the pointers and parameters of a gather launch; how the frame is cut into launches is the plan's (run_gather)
static void fill_gather_args(evplp_context *c, const evplp_frame_params *fp, GatherArgs &a, int pass) {
    std::memset(&a, 0, sizeof(a));
    a.sc = c->sc; a.st = c->st; a.fp = *fp; a.pdf_mc2 = fp->pdf_mc * fp->pdf_mc;
    a.g_pos = (const float4 *)c->buf[EVPLP_BUF_GBUF_POSITION]; a.g_nrm = (const float4 *)c->buf[EVPLP_BUF_GBUF_NORMAL];
    a.g_dif = (const float4 *)c->buf[EVPLP_BUF_GBUF_DIFFUSE]; a.g_phg = (const float4 *)c->buf[EVPLP_BUF_GBUF_PHONG];
    a.vpls = c->d_vpls; a.vpl_src_index = c->d_vpl_src; a.nvpl = &c->d_scalars[0];
    a.out = (float4 *)c->buf[EVPLP_BUF_VPL_ACCUM];
    a.partial_stride = (size_t)c->st.W * c->st.local_rows;
    a.counters = &c->d_counters[pass];
    a.splits_per_wave = 1;
    a.block_cost = c->calibrate ? c->d_block_cost : nullptr;
}
static int check_fp(evplp_context *c, const evplp_frame_params *fp, const char *name) {
    if (!fp) { c->set_error("%s: null frame params", name); return EVPLP_ERR_INVALID; }
    if (fp->photons_per_path != c->cfg.photons_per_path || fp->num_light_paths != c->cfg.num_light_paths || fp->num_vpl_light_paths > c->cfg.num_vpl_light_paths) {
        c->set_error("%s: frame params disagree with the configuration (paths / photons per path)", name); return EVPLP_ERR_INVALID;
    }
    if (fp->mis_mode > 5u) { c->set_error("%s: mis_mode %u out of range", name, fp->mis_mode); return EVPLP_ERR_INVALID; }
    return EVPLP_OK;
}
static int run_gather(evplp_context *c, const evplp_frame_params *fp, bool vsl) {
    const int pass = vsl ? EVPLP_PASS_GATHER_VSL : EVPLP_PASS_GATHER_VPL;
    const char *name = vsl ? "evplp_gather_vsl" : "evplp_gather_vpl";
    int rc = pass_ready(c, name, false); if (rc) return rc;
    if ((rc = check_fp(c, fp, name))) return rc;
    if (fp->num_vpl_light_paths == 0) { c->set_error("%s: num_vpl_light_paths is 0 (the reference disables the pass, rtcomphoton.h:200-203)", name); return EVPLP_ERR_INVALID; }
    if (c->adapt_pt) { c->set_error("%s: adaptivity is on in path-trace mode (evplp_adaptive_enable_pt): evplp_path_trace only", name); return EVPLP_ERR_INVALID; }
    if (c->d_adapt_tiles && fp->do_accumulate == 0) { c->set_error("%s: adaptivity is on (evplp_adaptive_enable): a gather must accumulate", name); return EVPLP_ERR_INVALID; }
    GatherArgs a; fill_gather_args(c, fp, a, pass);
    // adaptivity (evplp_adaptive_enable): retired tiles' items end at once and the reduce writes their pixels from the snapshot.  A calibration
    // launch gathers every tile (its clocks price whole blocks) and so needs every cut slot: the cut kernel skips nothing then.
    AdaptArgs ad{};
    if (c->d_adapt_tiles) { ad.tiles = c->d_adapt_tiles; ad.snap = c->d_adapt_snap; ad.n1 = (int32_t)(c->adapt_n + 1); }
    // gather budget mode (evplp_adaptive_enable(ctx, 2)): the walks and the cut kernel read this call's mask in place of the records -- a tile
    // that skips the call looks retired to them -- and the mode's own reduce follows the same mask
    const bool gbudget = c->adapt_gather_budget;
    const int32_t ntiles_all = c->tiles_x * c->tiles_y, phase = (int32_t)(c->adapt_m % c->adapt_window);
    if (gbudget) ad.tiles = c->d_adapt_mask;
    // the plan (host/gather_plan.cpp): every count below is its arithmetic, and the result of the gather depends on none of it
    GatherPlanInput pin{};
    pin.W = c->st.W; pin.local_rows = c->st.local_rows; pin.rows_in_image = c->rows_in_image; pin.strip_count = c->st.strip_count; pin.strip_rows = c->st.strip_rows;
    pin.nvpl_slots = nvpl_slot_count(c->cfg.num_vpl_light_paths, c->cfg.photons_per_path); pin.vsl = vsl; pin.splits_per_wave = c->cfg.gather_splits_per_wave;
    pin.env_gather_k = c->env_gather_k; pin.env_item_deal = c->env_item_deal; pin.env_tile_block_log2 = c->env_tile_block_log2; pin.env_cuts = c->env_cuts;
    pin.cut_cap = c->cut_cap; pin.mask_cap = c->mask_cap; pin.cuts_available = true;
    GatherPlan plan = plan_gather(pin);
    if (plan.refused) {
        c->set_error("%s: %zu VSL record slots exceed the %d this build can gather in one pass", name, pin.nvpl_slots, 4094 * kVplSplit); return EVPLP_ERR_INVALID;
    }
    // the workspaces the plan names.  Without memory for the cut scratch the frame is planned again without cuts: one band, walks from the
    // root, and the masks of that band.
    const size_t partial_bytes = sizeof(float4) * (size_t)plan.groups * a.partial_stride;
    hipError_t me = grow_scratch(c, c->partial, partial_bytes);
    if (me != hipSuccess) { c->set_error("gather: cannot allocate %zu bytes of partial sums: %s", partial_bytes, hipGetErrorString(me)); return EVPLP_ERR_OOM; }
    if (plan.use_cuts && grow_scratch(c, c->cuts, plan.cut_bytes) != hipSuccess) { pin.cuts_available = false; plan = plan_gather(pin); }
    if ((me = grow_scratch(c, c->vsl_masks, plan.mask_bytes)) != hipSuccess) { c->set_error("gather_vsl: cannot allocate %zu bytes of lit masks: %s", plan.mask_bytes, hipGetErrorString(me)); return EVPLP_ERR_OOM; }
    a.splits_per_wave = plan.k; a.item_deal = plan.item_deal; a.block_h_log2 = plan.block_h_log2; a.partial = (float4 *)c->partial.p;
    a.masks_per_split = plan.masks_per_split; a.vsl_masks = vsl ? (unsigned long long *)c->vsl_masks.p : nullptr;
    CutArgs ca; std::memset(&ca, 0, sizeof(ca));
    if (plan.use_cuts) {
        ca.nodes = c->sc.nodes; ca.tile_box = c->d_tile_box; ca.tiles_x = c->tiles_x; ca.tiles_y = c->tiles_y;
        ca.gw_log2 = plan.gw_log2; ca.gh_log2 = plan.gh_log2; ca.groups_x = plan.groups_x;
        ca.vpls = c->d_vpls; ca.nvpl = &c->d_scalars[0]; ca.vpl_stride = plan.vpl_stride;
        ca.cuts = (char *)c->cuts.p;
        ca.adapt_tiles = c->calibrate ? nullptr : ad.tiles;
        a.cuts = ca.cuts; a.cut_vpl_stride = ca.vpl_stride; a.cut_gw_log2 = ca.gw_log2; a.cut_gh_log2 = ca.gh_log2; a.cut_groups_x = ca.groups_x;
    }
    if ((rc = pass_begin(c, pass))) return rc;
    const uint32_t nrec = fp->photons_per_path * fp->num_vpl_light_paths;   // lighttracing.cu:368
    if (gbudget) launch_gather_budget_mask(c->d_adapt_tiles, ntiles_all, phase, c->adapt_window, c->d_adapt_mask, c->stream);
    launch_compact_vpl((const evplp_record *)c->buf[EVPLP_BUF_RECORDS], nrec, c->d_vpls, c->d_vpl_src, &c->d_scalars[0], c->stream);
    if (plan.use_cuts && !c->tile_box_valid) {      // the G-buffer did not come from evplp_primary (or the caller may have written it): boxes of the tiles as they are now
        launch_tile_boxes(c->st, (const float4 *)c->buf[EVPLP_BUF_GBUF_POSITION], c->d_tile_box, c->tiles_x, c->tiles_y, c->stream);
        c->tile_box_valid = !c->gbuf_pos_exposed;
    }
    // band by band: the cuts of the band's tile groups, then its walks -- the VSL gather's one launch per group range
    // (the events bracket the cuts AND the walks: the cut kernel is part of the gather's work)
    HIP_TRY(c, hipEventRecord(c->ev_dom_begin[pass], c->stream));
    for (int i = 0; i < plan.nbands; i++) {
        const GatherBand band = gather_band(plan, i);
        a.band_first = band.first; a.band_rows = band.args_rows;
        if (plan.use_cuts) {
            ca.group_row_first = a.cut_group_row_first = band.group_row_first; ca.groups_y = band.groups_y;
            launch_gather_cuts(ca, c->stream);
        }
        if (vsl) {
            for (int j = 0; j < plan.group_launches; j++) {
                const GatherGroupRange r = gather_group_range(plan, j);
                a.group_first = r.first; a.group_count = r.count;
                launch_gather_vsl(a, c->stream, ad);
            }
            a.group_first = 0; a.group_count = 0;
        } else launch_gather_vpl_items(a, c->stream, ad);
    }
    a.band_first = 0; a.band_rows = 0;
    HIP_TRY(c, hipEventRecord(c->ev_dom_end[pass], c->stream));
    if (gbudget) {
        // R and the extrapolation, then n_t += takes on the device and in the host copy (the same rule on the same records)
        launch_gather_reduce_budget(a, vsl ? 0 : 1, c->d_adapt_tiles, c->d_adapt_mask, c->d_adapt_snap, ad.n1, c->stream);
        launch_gather_budget_step(c->d_adapt_tiles, c->d_adapt_mask, ntiles_all, c->stream);
        for (int4 &r : c->adapt_tiles) if (gather_tile_takes(r, phase, c->adapt_window)) r.x += 1;
        c->adapt_m++;
    } else launch_gather_reduce(a, vsl ? 0 : 1, c->stream, ad);
    c->pass_has_dom[pass] = true;
    if ((rc = pass_end(c, pass))) return rc;
    if (fp->do_accumulate) c->adapt_n++;
    return EVPLP_OK;
}
extern "C" int evplp_gather_vpl(evplp_context *c, const evplp_frame_params *fp) { CTX_CHECK(c); return run_gather(c, fp, false); }
extern "C" int evplp_gather_vsl(evplp_context *c, const evplp_frame_params *fp) { CTX_CHECK(c); return run_gather(c, fp, true); }

// lvclighttracing.cu:348-384: the window covers num_vpl_light_paths paths of ALL num_light_paths * P record slots
extern "C" int evplp_gather_lvc(evplp_context *c, const evplp_frame_params *fp) {
    CTX_CHECK(c);
    const int pass = EVPLP_PASS_GATHER_LVC;
    if (c->adapt_pt) { c->set_error("evplp_gather_lvc: adaptivity is on in path-trace mode (evplp_adaptive_enable_pt): evplp_path_trace only"); return EVPLP_ERR_INVALID; }
    if (c->d_adapt_tiles) { c->set_error("evplp_gather_lvc: adaptivity is on (evplp_adaptive_enable): VPL and VSL gathers only"); return EVPLP_ERR_INVALID; }
    int rc = pass_ready(c, "evplp_gather_lvc", false); if (rc) return rc;
    if ((rc = check_fp(c, fp, "evplp_gather_lvc"))) return rc;
    if (fp->num_vpl_light_paths == 0) { c->set_error("evplp_gather_lvc: num_vpl_light_paths is 0"); return EVPLP_ERR_INVALID; }
    GatherArgs a; fill_gather_args(c, fp, a, pass);
    if ((rc = pass_begin(c, pass))) return rc;
    launch_gather_lvc(a, (const evplp_record *)c->buf[EVPLP_BUF_RECORDS], c->stream);
    return pass_end(c, pass);
}

extern "C" int evplp_path_trace(evplp_context *c, const float camera_pos[3], uint32_t rng_seed, uint32_t max_bounces, int32_t do_accumulate) {
    CTX_CHECK(c);
    if (c->d_adapt_tiles && !c->adapt_pt) { c->set_error("evplp_path_trace: adaptivity is on (evplp_adaptive_enable): VPL and VSL gathers only"); return EVPLP_ERR_INVALID; }
    if (c->adapt_budget) { c->set_error("evplp_path_trace: budget mode (evplp_adaptive_enable_pt(ctx, 2)): evplp_path_trace_batch only"); return EVPLP_ERR_INVALID; }
    if (c->adapt_pt && !do_accumulate) { c->set_error("evplp_path_trace: adaptivity is on (evplp_adaptive_enable_pt): a sample must accumulate"); return EVPLP_ERR_INVALID; }
    int rc = pass_ready(c, "evplp_path_trace", false); if (rc) return rc;
    if (!camera_pos) { c->set_error("evplp_path_trace: null camera position"); return EVPLP_ERR_INVALID; }
    PathTraceArgs a; std::memset(&a, 0, sizeof(a));
    a.sc = c->sc; a.st = c->st;
    a.g_pos = (const float4 *)c->buf[EVPLP_BUF_GBUF_POSITION]; a.g_nrm = (const float4 *)c->buf[EVPLP_BUF_GBUF_NORMAL];
    a.g_dif = (const float4 *)c->buf[EVPLP_BUF_GBUF_DIFFUSE]; a.g_phg = (const float4 *)c->buf[EVPLP_BUF_GBUF_PHONG];
    for (int k = 0; k < 3; k++) a.camera_pos[k] = camera_pos[k];
    a.rng_seed = rng_seed; a.max_bounces = max_bounces; a.do_accumulate = do_accumulate ? 1u : 0u;
    a.out = (float4 *)c->buf[EVPLP_BUF_VPL_ACCUM];
    a.counters = &c->d_counters[EVPLP_PASS_PATH_TRACE];
    if ((rc = pass_begin(c, EVPLP_PASS_PATH_TRACE))) return rc;
    // path-trace mode (evplp_adaptive_enable_pt): retired tiles trace nothing and are written from the snapshot
    AdaptArgs ad{};
    if (c->adapt_pt) { ad.tiles = c->d_adapt_tiles; ad.snap = c->d_adapt_snap; ad.n1 = (int32_t)(c->adapt_n + 1); }
    launch_path_trace(a, c->stream, ad);
    if ((rc = pass_end(c, EVPLP_PASS_PATH_TRACE))) return rc;
    if (do_accumulate) c->adapt_n++;
    return EVPLP_OK;
}

// evplp_path_trace_batch (include/evplp.h has the contract; kernels.h PtBatchChunk the device side).  One sequence for every mode: count the
// items from the records' host copy, build the item table, run the items in chunks of as many as the staging buffer holds, close.  A chunk is
// primary -> trace -> accumulate on the stream, so the adds to a pixel stay in increasing s wherever the cuts fall, inside a tile's samples too.
extern "C" int evplp_path_trace_batch_scratch(evplp_context *c, uint64_t bytes) { CTX_CHECK(c); c->pt_batch_cap = bytes; return EVPLP_OK; }
extern "C" int evplp_path_trace_batch(evplp_context *c, const float camera_pos[3], int32_t samples, const float *jitters, const uint32_t *rng_seeds, uint32_t max_bounces) {
    CTX_CHECK(c);
    const char *name = "evplp_path_trace_batch";
    if (samples < 1 || samples > kPtBatchMaxSamples) { c->set_error("%s: samples must be 1 .. %d (got %d)", name, kPtBatchMaxSamples, samples); return EVPLP_ERR_INVALID; }
    if (!camera_pos || !jitters || !rng_seeds) { c->set_error("%s: null camera position, jitters or seeds", name); return EVPLP_ERR_INVALID; }
    if (c->d_adapt_tiles && !c->adapt_pt) { c->set_error("%s: adaptivity is on (evplp_adaptive_enable): VPL and VSL gathers only", name); return EVPLP_ERR_INVALID; }
    if (c->pt_batch_cap < kPtBatchSlotBytes) {
        c->set_error("%s: the scratch bound (%llu B, evplp_path_trace_batch_scratch) is below one tile x one sample (%zu B)", name, (unsigned long long)c->pt_batch_cap, kPtBatchSlotBytes);
        return EVPLP_ERR_INVALID;
    }
    const size_t ntiles = (size_t)c->tiles_x * (size_t)c->tiles_y;
    if (ntiles >= (size_t)kPtBatchMaxTiles) { c->set_error("%s: a context holds at most %d tiles", name, kPtBatchMaxTiles - 1); return EVPLP_ERR_INVALID; }
    PtBatchSamples sm; std::memset(&sm, 0, sizeof(sm));
    unsigned long long cut_mask = 0;
    for (int s = 0; s < samples; s++) {
        sm.jitter[s][0] = jitters[2 * s]; sm.jitter[s][1] = jitters[2 * s + 1]; sm.seed[s] = rng_seeds[s];
        if (!std::isfinite(sm.jitter[s][0]) || !std::isfinite(sm.jitter[s][1])) { c->set_error("%s: jitter %d is not finite", name, s); return EVPLP_ERR_INVALID; }
        if (jitter_within_cuts(c, sm.jitter[s])) cut_mask |= 1ull << s;
    }
    int rc = pass_ready(c, name, true); if (rc) return rc;
    if (ntiles > 0) {
        // the items: every tile's own sample count, from the records' host copy (current in every mode: evplp_adaptive_retire reads the records
        // back, budget mode follows them below); the device builds the table from the same function of the same records
        const int32_t mode = c->adapt_budget ? 2 : c->adapt_pt ? 1 : 0;
        auto tile_samples = [&](size_t t) { return pt_tile_samples(mode, mode ? c->adapt_tiles[t] : make_int4(0, 0, 0, 0), samples); };
        uint64_t items = 0;
        for (size_t t = 0; t < ntiles; t++) items += (uint64_t)tile_samples(t);
        // the staging buffer: what the call needs, within the bound; it only grows, unless the bound came down below it
        const uint64_t cap_slots = std::min<uint64_t>(c->pt_batch_cap / kPtBatchSlotBytes, 1u << 30);
        const uint64_t slots = std::min<uint64_t>(std::max<uint64_t>(items, 1), cap_slots);
        if (c->pt_batch.bytes > cap_slots * kPtBatchSlotBytes) c->pt_batch.bytes = 0;      // (it counts as holding nothing: the grow below frees it)
        if (grow_scratch(c, c->pt_batch, slots * kPtBatchSlotBytes) != hipSuccess) {
            c->set_error("%s: cannot allocate %llu B of staging (bound it with evplp_path_trace_batch_scratch)", name, (unsigned long long)(slots * kPtBatchSlotBytes));
            return EVPLP_ERR_OOM;
        }
        const uint64_t have = c->pt_batch.bytes / kPtBatchSlotBytes;
        if (!c->d_pt_first) HIP_TRY(c, hipMalloc((void **)&c->d_pt_first, sizeof(int32_t) * (ntiles + 1)));
        const hipError_t te = grow_scratch(c, c->pt_table, sizeof(uint32_t) * items);
        if (te != hipSuccess) { c->set_error("%s: cannot allocate %llu B of item table: %s", name, (unsigned long long)(sizeof(uint32_t) * items), hipGetErrorString(te)); return EVPLP_ERR_OOM; }

        PrimaryArgs pa; std::memset(&pa, 0, sizeof(pa));
        pa.sc = c->sc; pa.st = c->st; pa.cam = c->cam; pa.g_light = (float4 *)c->buf[EVPLP_BUF_LIGHT];
        if (c->env_cuts != 0 && cut_mask) primary_cuts_into(c, pa);
        PathTraceArgs ta; std::memset(&ta, 0, sizeof(ta));
        ta.sc = c->sc; ta.st = c->st;
        for (int k = 0; k < 3; k++) ta.camera_pos[k] = camera_pos[k];
        ta.max_bounces = max_bounces; ta.do_accumulate = 0u;                  // (a sample's radiance goes to its staging slot as 0 + radiance: kernels_ptbatch.hip)
        ta.counters = &c->d_counters[EVPLP_PASS_PATH_TRACE];
        float4 *out = (float4 *)c->buf[EVPLP_BUF_VPL_ACCUM];
        if ((rc = pass_begin(c, EVPLP_PASS_PATH_TRACE))) return rc;
        launch_pt_batch_table(c->d_adapt_tiles, (int32_t)ntiles, mode, samples, c->d_pt_first, (uint32_t *)c->pt_table.p, c->stream);
        PtBatchChunk ch; std::memset(&ch, 0, sizeof(ch));
        ch.table = (const uint32_t *)c->pt_table.p; ch.total = c->d_pt_first + ntiles; ch.staging = (float4 *)c->pt_batch.p; ch.cut_mask = cut_mask;
        for (uint64_t i0 = 0; i0 < items; i0 += have) {
            ch.item_first = (int32_t)i0; ch.item_count = (int32_t)std::min<uint64_t>(have, items - i0);
            launch_pt_batch_primary(pa, sm, ch, c->stream);
            launch_pt_batch_trace(ta, sm, ch, c->stream);
            launch_pt_batch_accumulate(c->st, mode == 2 ? c->d_adapt_snap : out, c->d_pt_first, (int32_t)ntiles, ch, c->stream);     // (budget mode: the raw sums R)
        }
        // mode 1: the retired tiles are written once from the snapshot, for N + S; mode 2: n_t += s_t on the device and here, and every tile from R
        if (mode) launch_pt_batch_close(c->st, c->d_adapt_tiles, mode, c->d_pt_first, c->d_adapt_snap, out, (int32_t)(c->adapt_n + samples), (int32_t)ntiles, c->stream);
        if (mode == 2) for (size_t t = 0; t < ntiles; t++) c->adapt_tiles[t].x += tile_samples(t);
        if ((rc = pass_end(c, EVPLP_PASS_PATH_TRACE))) return rc;
    }
    c->adapt_n += samples;
    // the whole-frame primary pass at the last jitter: G-buffer planes, tile boxes and pass record are then those of S single calls
    return evplp_primary(c, sm.jitter[samples - 1], 0);
}

// setupPhotonSplatIcosohedron (rtcomphoton.h:632-644): the proxy mesh of EVPLP_FOOTPRINT_PROXY -> slabs on the device
static int upload_proxy(evplp_context *c, const float *vertices, int32_t nverts, const int32_t *indices, int32_t ntris, const char *name) {
    ProxyHost ph; std::string why;
    if (!build_proxy_slabs(vertices, nverts, indices, ntris, &ph, &why)) { c->set_error("%s: %s", name, why.c_str()); return EVPLP_ERR_INVALID; }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));                          // (a splat in flight reads the old slabs)
    if (!c->d_proxy_slabs) {
        HIP_TRY(c, hipMalloc((void **)&c->d_proxy_slabs, sizeof(float4) * kMaxProxySlabs));
        HIP_TRY(c, hipMalloc((void **)&c->d_proxy_hm, sizeof(float) * kMaxProxySlabs));
    }
    HIP_TRY(c, hipMemcpy(c->d_proxy_slabs, ph.slabs.data(), sizeof(float4) * ph.slabs.size(), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->d_proxy_hm, ph.hm.data(), sizeof(float) * ph.hm.size(), hipMemcpyHostToDevice));
    c->proxy_count = (int32_t)ph.slabs.size(); c->proxy_rin = ph.rin; c->proxy_rout = ph.rout;
    return EVPLP_OK;
}
static int default_proxy(evplp_context *c, const char *name) {
    std::vector<float> v; std::vector<int32_t> t;
    default_splat_proxy(v, t);
    return upload_proxy(c, v.data(), (int32_t)(v.size() / 3), t.data(), (int32_t)(t.size() / 3), name);
}
extern "C" int evplp_set_splat_proxy(evplp_context *c, const float *vertices, int32_t nverts, const int32_t *indices, int32_t ntris) {
    CTX_CHECK(c);
    { int rc_ = settle_splat(c); if (rc_) return rc_; }
    if (!vertices) return default_proxy(c, "evplp_set_splat_proxy");
    return upload_proxy(c, vertices, nverts, indices, ntris, "evplp_set_splat_proxy");
}
extern "C" int evplp_default_splat_proxy(float *vertices, int32_t *indices) {
    std::vector<float> v; std::vector<int32_t> t;
    default_splat_proxy(v, t);
    if (vertices) std::memcpy(vertices, v.data(), sizeof(float) * v.size());
    if (indices) std::memcpy(indices, t.data(), sizeof(int32_t) * t.size());
    return (int)(t.size() / 3);
}

extern "C" int evplp_splat_photons(evplp_context *c, const evplp_frame_params *fp, int32_t clear) {
    CTX_CHECK(c);
    // (overlapped mode, accumulating: the previous pass may stay pending -- only look whether its verdict has arrived; a clearing pass
    // settles it first, its re-run would otherwise land in the cleared buffer)
    // Deterministic mode never leaves a pass pending behind a younger one: the re-run of an overflowed pass would otherwise be
    // enqueued before or after the younger pass depending on when its verdict arrives, and the float sums into the photon
    // accumulator would differ between runs.
    if (c->adapt_gather_budget) { c->set_error("evplp_splat_photons: gather budget mode (evplp_adaptive_enable(ctx, 2)): a tile's VPL part has n_t samples and its photon part N; one set of moments cannot price both"); return EVPLP_ERR_INVALID; }
    const bool relaxed = c->aux_stream && !clear && !c->cfg.deterministic;
    int rc = pass_ready(c, "evplp_splat_photons", true, !relaxed); if (rc) return rc;
    if (relaxed) {
        while (c->npend >= 2) if ((rc = settle_one(c))) return rc;
        while (c->npend > 0 && hipEventQuery(c->pend[0].ev) == hipSuccess) if ((rc = settle_one(c))) return rc;
    }
    if ((rc = check_fp(c, fp, "evplp_splat_photons"))) return rc;
    if (!(fp->photon_radius > 0.0f)) { c->set_error("evplp_splat_photons: photon_radius must be > 0"); return EVPLP_ERR_INVALID; }
    if (fp->splat_footprint > (uint32_t)EVPLP_FOOTPRINT_PROXY) { c->set_error("evplp_splat_photons: splat_footprint %u out of range", fp->splat_footprint); return EVPLP_ERR_INVALID; }
    if (fp->splat_footprint == (uint32_t)EVPLP_FOOTPRINT_PROXY && c->proxy_count == 0 && (rc = default_proxy(c, "evplp_splat_photons"))) return rc;
    SplatArgs a; std::memset(&a, 0, sizeof(a));
    a.st = c->st; a.cam = c->cam; a.fp = *fp;
    a.g_pos = (const float4 *)c->buf[EVPLP_BUF_GBUF_POSITION]; a.g_nrm = (const float4 *)c->buf[EVPLP_BUF_GBUF_NORMAL];
    a.g_dif = (const float4 *)c->buf[EVPLP_BUF_GBUF_DIFFUSE]; a.g_phg = (const float4 *)c->buf[EVPLP_BUF_GBUF_PHONG];
    a.records = (const evplp_record *)c->buf[EVPLP_BUF_RECORDS];
    a.num_records = c->cfg.num_light_paths * c->cfg.photons_per_path;   // instances = numLightPaths * P (:832)
    a.out = (float4 *)c->buf[EVPLP_BUF_PHOTON_ACCUM];
    a.tile_box = c->d_tile_box; a.tile_pairs = c->d_tile_pairs; a.tile_cursor = c->d_tile_cursor;
    a.bin_items = c->d_bin_items; a.bin_items_tmp = c->d_bin_items_tmp; a.bin_stride = c->bin_stride;
    a.compact = c->d_compact; a.overflow = &c->d_scalars[8]; a.summary = c->d_summary;
    a.seg = c->d_seg; a.seg_off = c->d_seg_off; a.big_list = c->d_big_list; a.big_count = c->d_big_count; a.num_bin_groups = c->num_bin_groups;
    a.bucket_w_log2 = c->bucket_w_log2; a.bucket_h_log2 = c->bucket_h_log2; a.buckets_x = c->buckets_x; a.num_buckets = c->num_buckets;
    a.tiles_x = c->tiles_x; a.tiles_y = c->tiles_y; a.deterministic = c->cfg.deterministic; a.boxes_valid = c->tile_box_valid ? 1 : 0;
    a.counters = &c->d_counters[EVPLP_PASS_SPLAT];
    a.proxy_slabs = c->d_proxy_slabs; a.proxy_hm = c->d_proxy_hm; a.proxy_count = c->proxy_count; a.proxy_rin = c->proxy_rin; a.proxy_rout = c->proxy_rout;
    a.tile_frags = c->d_tile_frags; c->last_splat_proxy = fp->splat_footprint == (uint32_t)EVPLP_FOOTPRINT_PROXY;
    // MIXED tile launch when the previous pass had bins at least twice the heavy threshold (a heuristic, like the choice between the pure
    // variants it replaces): below that the heavy list stays nearly empty and its bookkeeping costs more than four waves save
    if (c->env_tile_mixed && c->last_bin_max >= c->mixed_trigger) { a.heavy_list = c->d_heavy_list; a.tile_flags = c->d_tile_flags; a.heavy_cap = c->heavy_cap; a.heavy_threshold = c->heavy_threshold; }
    if ((rc = pass_begin(c, EVPLP_PASS_SPLAT))) return rc;
    c->splat_n++;
    if (clear) HIP_TRY(c, hipMemsetAsync(c->buf[EVPLP_BUF_PHOTON_ACCUM], 0, buffer_bytes(c, EVPLP_BUF_PHOTON_ACCUM), c->stream));
    launch_splat_bin(a, c->stream);                                       // (clears the overflow flag, the cursors and the summary)
    // Tile kernel variant.  (Round 5: when the previous pass had bins of >= mixed_trigger entries the launch is MIXED -- a.heavy_list above,
    // kernels_splat.hip -- and what follows only decides for deterministic contexts and EVPLP_TILE_MIXED=0.)
    // One wave per tile is cheapest while bins are short; when some bins are very full (tiles
    // that see a floor at grazing angle collect thousands of photons) those waves set the duration of the launch and
    // four waves per tile win.  Deterministic mode always uses one variant: the fold order is part of the result.
    // Measured (tiles kernel, ms): fullest bin 1405 entries (config #3): 0.31 with one wave, 0.18 with four; fullest bin 365
    // (config #4 shape): 0.12 / 0.22.  The fullest bin of the PREVIOUS pass decides (a heuristic either way).
    const bool split_tiles = c->cfg.deterministic ? true : c->last_bin_max >= split_threshold(c, fp->splat_footprint);
    const bool dom = c->profile_kernels;
    launch_splat_tiles(a, split_tiles, c->stream, dom ? c->ev_dom_begin[EVPLP_PASS_SPLAT] : nullptr, dom ? c->ev_dom_end[EVPLP_PASS_SPLAT] : nullptr);
    // The number of (photon, tile) bin entries depends on the photon set and the radius and is known on the device only.  The
    // whole pass is enqueued now; the summary travels to pinned memory and is checked by the next call (settle_splat).
    evplp_context::PendingSplat &slot = c->pend[c->npend];
    HIP_TRY(c, hipMemcpyAsync(slot.h, &c->d_summary[kSummaryFinal], 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));   // entries, fullest bin, overflow
    HIP_TRY(c, hipEventRecord(slot.ev, c->stream));
    slot.args = a; c->npend++;
    c->pass_has_dom[EVPLP_PASS_SPLAT] = dom;
    return pass_end(c, EVPLP_PASS_SPLAT);
}

// [finalize] composite of this context's strip into d_rgb (device); evplp_resolve downloads it, the group all-gathers it
namespace evplp {
// settle = false (the per-iteration composite of a running loop): the composite is enqueued behind the last splat without waiting for
// the verdict on its bins -- the host does not stall; in the rare iteration whose bins overflowed the presented frame lacks that one
// pass (it is run again and lands in the accumulator before the next composite).  Results that leave the device always settle.
// as_pass = false (the composite evplp_frame_error measures): the pass statistics of EVPLP_PASS_RESOLVE stay as they were
int resolve_to_device(evplp_context *c, float vs, float ps, float ls, int32_t mask_emitter, int32_t gamma, bool settle, bool as_pass) {
    CTX_CHECK(c);
    if (settle) { int rc_ = settle_splat(c); if (rc_) return rc_; }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int rc;
    if (as_pass && (rc = pass_begin(c, EVPLP_PASS_RESOLVE))) return rc;
    launch_resolve(c->st, (const float4 *)c->buf[EVPLP_BUF_VPL_ACCUM], (const float4 *)c->buf[EVPLP_BUF_PHOTON_ACCUM],
                   (const float4 *)c->buf[EVPLP_BUF_LIGHT], vs, ps, ls, mask_emitter, gamma, c->d_rgb, c->stream);
    if (!as_pass) { HIP_TRY(c, hipGetLastError()); return EVPLP_OK; }
    return pass_end(c, EVPLP_PASS_RESOLVE);
}
// every pending photon splat has its verdict (and its re-run, if its bins overflowed, is enqueued): the accumulators are final in
// stream order (the reduction of an EVPLP_PARTITION_ITERATIONS group reads them)
int settle(evplp_context *c) {
    CTX_CHECK(c);
    return settle_splat(c);
}
} // namespace evplp

extern "C" int evplp_resolve(evplp_context *c, float vs, float ps, float ls, int32_t mask_emitter, int32_t gamma, float *out_rgb) {
    CTX_CHECK(c);
    if (!out_rgb) { c->set_error("evplp_resolve: null output"); return EVPLP_ERR_INVALID; }
    int rc = evplp::resolve_to_device(c, vs, ps, ls, mask_emitter, gamma, true, true);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(out_rgb, c->d_rgb, sizeof(float) * 3 * (size_t)c->st.W * c->st.local_rows, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EVPLP_OK;
}

extern "C" int evplp_present(evplp_context *c, float vs, float ps, float ls, int32_t mask_emitter, int32_t gamma) {
    CTX_CHECK(c);
    return evplp::resolve_to_device(c, vs, ps, ls, mask_emitter, gamma, !c->aux_stream, true);      // (overlapped contexts keep the host an iteration ahead)
}

// ---- error against a reference image (include/evplp.h evplp_frame_error): reduced on the device, 32 bytes per row come to the host
static void release_error_reference(evplp_context *c) {
    hipFree(c->d_err_ref); hipFree(c->d_err_keep); hipFree(c->d_err_rows);
    c->d_err_ref = nullptr; c->d_err_keep = nullptr; c->d_err_rows = nullptr; c->err_rows.clear();
}
extern "C" int evplp_set_error_reference(evplp_context *c, const float *rgb, const uint8_t *mask) {
    CTX_CHECK(c);
    if (!rgb && mask) { c->set_error("evplp_set_error_reference: a mask without a reference image"); return EVPLP_ERR_INVALID; }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));      // (no composite or reduction of an earlier call still reads the old image)
    if (!rgb) { release_error_reference(c); return EVPLP_OK; }
    const size_t px = (size_t)c->st.W * c->st.H;
    std::vector<uint8_t> keep;
    if (mask) { keep.resize(px); for (size_t i = 0; i < px; i++) keep[i] = (mask[3 * i] | mask[3 * i + 1] | mask[3 * i + 2]) != 0 ? 1 : 0; }
    hipError_t e = hipSuccess;
    if (!c->d_err_ref) e = hipMalloc((void **)&c->d_err_ref, sizeof(float) * 3 * px);
    if (e == hipSuccess && !c->d_err_rows) e = hipMalloc((void **)&c->d_err_rows, sizeof(RowError) * (size_t)std::max(c->st.local_rows, 1));
    if (e == hipSuccess && mask && !c->d_err_keep) e = hipMalloc((void **)&c->d_err_keep, px);
    if (e != hipSuccess) {
        (void)hipGetLastError(); release_error_reference(c);
        c->set_error("evplp_set_error_reference: cannot allocate %zu bytes: %s", px * 13, hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? EVPLP_ERR_OOM : EVPLP_ERR_HIP;
    }
    if (!mask) { hipFree(c->d_err_keep); c->d_err_keep = nullptr; }
    e = hipMemcpy(c->d_err_ref, rgb, sizeof(float) * 3 * px, hipMemcpyHostToDevice);
    if (e == hipSuccess && mask) e = hipMemcpy(c->d_err_keep, keep.data(), px, hipMemcpyHostToDevice);
    if (e != hipSuccess) { release_error_reference(c); c->set_error("evplp_set_error_reference: upload: %s", hipGetErrorString(e)); return EVPLP_ERR_HIP; }
    c->err_rows.assign((size_t)std::max(c->st.local_rows, 1), RowError{});
    return EVPLP_OK;
}
namespace evplp {
// the partials of every local row of the composite in d_rgb, to c->err_rows (waits for them)
int frame_error_rows(evplp_context *c) {
    CTX_CHECK(c);
    if (!c->d_err_ref) { c->set_error("evplp_frame_error: no reference image (evplp_set_error_reference)"); return EVPLP_ERR_INVALID; }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    launch_frame_error(c->st, c->d_rgb, c->d_err_ref, c->d_err_keep, c->d_err_rows, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->err_rows.data(), c->d_err_rows, sizeof(RowError) * (size_t)c->st.local_rows, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EVPLP_OK;
}
// a context's per-local-row partials (c->err_rows, c->noise_rows) put at their image rows
void place_row_errors(const evplp_context *c, const std::vector<RowError> &local, std::vector<RowError> &rows, std::vector<char> &held) {
    for (int l = 0; l < c->st.local_rows; l++) {
        const int y = c->st.global_row(l);
        if (y < 0 || y >= c->st.H) continue;
        rows[(size_t)y] = local[(size_t)l]; held[(size_t)y] = 1;
    }
}
void sum_row_errors(const std::vector<RowError> &rows, const std::vector<char> &held, double npix, double out[3]) {
    RowError t{ 0.0, 0.0, 0.0, 0.0 };
    for (size_t y = 0; y < rows.size(); y++) {
        if (!held[y]) continue;
        t.num += rows[y].num; t.rel += rows[y].rel; t.rel_kept += rows[y].rel_kept; t.kept += rows[y].kept;
    }
    out[0] = npix > 0 ? t.num / npix : 0.0;
    out[1] = npix > 0 ? t.rel / npix : 0.0;
    out[2] = t.kept > 0 ? t.rel_kept / t.kept : 0.0;
}
} // namespace evplp
extern "C" int evplp_frame_error(evplp_context *c, float vs, float ps, float ls, int32_t mask_emitter, int32_t gamma, double out[3]) {
    CTX_CHECK(c);
    if (!out) { c->set_error("evplp_frame_error: null output"); return EVPLP_ERR_INVALID; }
    if (!c->d_err_ref) { c->set_error("evplp_frame_error: no reference image (evplp_set_error_reference)"); return EVPLP_ERR_INVALID; }
    int rc = evplp::resolve_to_device(c, vs, ps, ls, mask_emitter, gamma, true, false);
    if (rc) return rc;
    if ((rc = evplp::frame_error_rows(c))) return rc;
    std::vector<RowError> rows((size_t)c->st.H); std::vector<char> held((size_t)c->st.H, 0);
    evplp::place_row_errors(c, c->err_rows, rows, held);
    evplp::sum_row_errors(rows, held, (double)c->st.W * c->rows_in_image, out);
    return EVPLP_OK;
}

// ---- per-pixel noise from the running sums, without a reference (include/evplp.h evplp_noise_*)
static void release_noise(evplp_context *c) {
    hipFree(c->d_noise); hipFree(c->d_noise_keep); hipFree(c->d_noise_rows);
    c->d_noise = nullptr; c->d_noise_keep = nullptr; c->d_noise_rows = nullptr; c->noise_rows.clear(); c->noise_k = c->noise_b = 0;
}
namespace evplp {
// the tile records as the noise kernels read them (tiles = null: adaptivity is off)
AdaptTiles adapt_view(const evplp_context *c, float scale) {
    return AdaptTiles{ c->d_adapt_tiles, c->tiles_x, 0, (double)c->adapt_n, (double)scale };
}
NoisePlanes noise_planes(const evplp_context *c) {
    const size_t px = (size_t)c->st.W * c->st.local_rows;
    double *q = (double *)c->d_noise;
    float4 *prev = (float4 *)(q + 3 * c->noise_stride);
    return NoisePlanes{ q, prev, prev + px, c->noise_stride };
}
NoiseMoments noise_moments_of(const evplp_context *c) {
    const NoisePlanes m = noise_planes(c);
    return NoiseMoments{ m.q, nullptr, m.prev, m.start, m.stride };
}
// the records an estimate of the moments m reads: a context's own moments see its retired tiles; pooled shards (m.s) never have any
static AdaptTiles noise_adapt_view(const evplp_context *c, const NoiseMoments &m, float scale) {
    return (c->d_adapt_tiles && !m.s) ? adapt_view(c, scale) : AdaptTiles{};
}
size_t noise_bytes(const evplp_context *c) { return sizeof(double) * 3 * c->noise_stride + sizeof(float4) * 2 * (size_t)c->st.W * c->st.local_rows; }
int noise_rows(evplp_context *c, const NoiseMoments &m, const float4 *light, double K, double B, float scale, float ls, int32_t mask_emitter) {
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const double s2K = (double)scale * (double)scale * K;
    launch_noise_rows(c->st, m, K, B, s2K, light, ls, mask_emitter, c->d_rgb, c->d_noise_keep, c->d_noise_rows, noise_adapt_view(c, m, scale), c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->noise_rows.data(), c->d_noise_rows, sizeof(RowError) * (size_t)c->st.local_rows, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EVPLP_OK;
}
int noise_variance_to_device(evplp_context *c, const NoiseMoments &m, double K, double B, float scale) {
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    launch_noise_variance(c->st, m, K, B, (double)scale * (double)scale * K, c->d_rgb, noise_adapt_view(c, m, scale), c->stream);
    HIP_TRY(c, hipGetLastError());
    return EVPLP_OK;
}
} // namespace evplp
// tracking (re)starts from the accumulators as they are: c_prev = c_start = c, Q = 0, K = B = 0 (stream order)
static int noise_restart(evplp_context *c) {
    c->noise_k = c->noise_b = 0;
    launch_noise_fold(evplp::noise_planes(c), (const float4 *)c->buf[EVPLP_BUF_VPL_ACCUM], (const float4 *)c->buf[EVPLP_BUF_PHOTON_ACCUM],
                      c->st, evplp::adapt_view(c, 1.0f), 0, c->stream);
    HIP_TRY(c, hipGetLastError());
    return EVPLP_OK;
}
extern "C" int evplp_noise_track(evplp_context *c, int32_t on, const uint8_t *mask) {
    CTX_CHECK(c);
    if (!on && mask) { c->set_error("evplp_noise_track: a mask without tracking"); return EVPLP_ERR_INVALID; }
    if (c->d_adapt_tiles && c->adapt_n > 0) {
        c->set_error("evplp_noise_track: adaptivity is on and %lld gather(s) accumulated: the retired tiles' figures need this tracking", (long long)c->adapt_n);
        return EVPLP_ERR_INVALID;
    }
    { int rc_ = settle_splat(c); if (rc_) return rc_; }            // (the snapshot sees every splat enqueued so far)
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));                   // (no fold or estimate of an earlier call still reads the old planes)
    if (!on) { release_noise(c); return EVPLP_OK; }
    const size_t px = (size_t)c->st.W * c->st.local_rows, image_px = (size_t)c->st.W * c->st.H;
    c->noise_stride = (px + 1) & ~(size_t)1;
    std::vector<uint8_t> keep;
    if (mask) { keep.resize(image_px); for (size_t i = 0; i < image_px; i++) keep[i] = (mask[3 * i] | mask[3 * i + 1] | mask[3 * i + 2]) != 0 ? 1 : 0; }
    hipError_t e = hipSuccess;
    if (!c->d_noise) e = hipMalloc((void **)&c->d_noise, evplp::noise_bytes(c));
    if (e == hipSuccess && !c->d_noise_rows) e = hipMalloc((void **)&c->d_noise_rows, sizeof(RowError) * (size_t)std::max(c->st.local_rows, 1));
    if (e == hipSuccess && mask && !c->d_noise_keep) e = hipMalloc((void **)&c->d_noise_keep, image_px);
    if (e != hipSuccess) {
        (void)hipGetLastError(); release_noise(c);
        c->set_error("evplp_noise_track: cannot allocate %zu bytes: %s", evplp::noise_bytes(c), hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? EVPLP_ERR_OOM : EVPLP_ERR_HIP;
    }
    if (!mask) { hipFree(c->d_noise_keep); c->d_noise_keep = nullptr; }
    else if ((e = hipMemcpy(c->d_noise_keep, keep.data(), image_px, hipMemcpyHostToDevice)) != hipSuccess) {
        release_noise(c); c->set_error("evplp_noise_track: upload: %s", hipGetErrorString(e)); return EVPLP_ERR_HIP;
    }
    c->noise_rows.assign((size_t)std::max(c->st.local_rows, 1), RowError{});
    return noise_restart(c);
}
extern "C" int evplp_noise_fold(evplp_context *c, int32_t iterations) {
    CTX_CHECK(c);
    if (!c->d_noise) { c->set_error("evplp_noise_fold: tracking is off (evplp_noise_track)"); return EVPLP_ERR_INVALID; }
    if (iterations < 1) { c->set_error("evplp_noise_fold: a batch holds >= 1 iterations, not %d", iterations); return EVPLP_ERR_INVALID; }
    { int rc_ = settle_splat(c); if (rc_) return rc_; }            // (every splat of the batch has its verdict; a re-run is enqueued before the fold)
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    if (c->adapt_budget) {         // (per tile, k_t = n_t - K_t; the host copy of the records follows)
        launch_noise_fold_budget(evplp::noise_planes(c), c->st, c->d_adapt_tiles, c->d_adapt_snap, c->tiles_x * c->tiles_y, c->stream);
        for (int4 &r : c->adapt_tiles) if (r.x != r.y) { r.y = r.x; r.z += 1; }
    } else          // (with adaptivity on, retired pixels keep their Q and c_prev)
        launch_noise_fold(evplp::noise_planes(c), (const float4 *)c->buf[EVPLP_BUF_VPL_ACCUM], (const float4 *)c->buf[EVPLP_BUF_PHOTON_ACCUM],
                          c->st, evplp::adapt_view(c, 1.0f), iterations, c->stream);
    HIP_TRY(c, hipGetLastError());
    c->noise_k += iterations; c->noise_b += 1;
    return EVPLP_OK;
}
static int noise_ready(evplp_context *c, const char *name) {
    if (!c->d_noise) { c->set_error("%s: tracking is off (evplp_noise_track)", name); return EVPLP_ERR_INVALID; }
    if (c->noise_b < 2) { c->set_error("%s: %lld fold(s): the estimate needs >= 2", name, (long long)c->noise_b); return EVPLP_ERR_INVALID; }
    return EVPLP_OK;
}
extern "C" int evplp_noise_estimate(evplp_context *c, float scale, float ls, int32_t mask_emitter, double out[3]) {
    CTX_CHECK(c);
    if (!out) { c->set_error("evplp_noise_estimate: null output"); return EVPLP_ERR_INVALID; }
    int rc = noise_ready(c, "evplp_noise_estimate");
    if (rc) return rc;
    if ((rc = evplp::resolve_to_device(c, scale, scale, ls, mask_emitter, 0, true, false))) return rc;
    if ((rc = evplp::noise_rows(c, evplp::noise_moments_of(c), (const float4 *)c->buf[EVPLP_BUF_LIGHT], (double)c->noise_k, (double)c->noise_b, scale, ls, mask_emitter))) return rc;
    std::vector<RowError> rows((size_t)c->st.H); std::vector<char> held((size_t)c->st.H, 0);
    evplp::place_row_errors(c, c->noise_rows, rows, held);
    evplp::sum_row_errors(rows, held, (double)c->st.W * c->rows_in_image, out);
    return EVPLP_OK;
}
extern "C" int evplp_noise_variance(evplp_context *c, float scale, float *out_rgb) {
    CTX_CHECK(c);
    if (!out_rgb) { c->set_error("evplp_noise_variance: null output"); return EVPLP_ERR_INVALID; }
    int rc = noise_ready(c, "evplp_noise_variance");
    if (rc) return rc;
    if ((rc = evplp::noise_variance_to_device(c, evplp::noise_moments_of(c), (double)c->noise_k, (double)c->noise_b, scale))) return rc;
    HIP_TRY(c, hipMemcpyAsync(out_rgb, c->d_rgb, sizeof(float) * 3 * (size_t)c->st.W * c->st.local_rows, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EVPLP_OK;
}

// ---- the denoiser of a written frame (include/evplp.h evplp_denoise, kernels_denoise.hip)
namespace evplp {
bool denoise_settings(const evplp_denoise_params *p, DenoiseSettings *out, char *why, size_t cap) {
    DenoiseSettings d{ 5, 4.0f, 128.0f, 0.01f };
    if (p) {
        if (p->levels != 0) d.levels = p->levels;
        const float sig[3] = { p->sigma_luminance, p->sigma_normal, p->sigma_position };
        const char *names[3] = { "sigma_luminance", "sigma_normal", "sigma_position" };
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(sig[k]) || sig[k] < 0.0f) { std::snprintf(why, cap, "%s must be finite and >= 0 (0 = the default), not %g", names[k], (double)sig[k]); return false; }
        if (p->sigma_luminance != 0.0f) d.sigma_l = p->sigma_luminance;
        if (p->sigma_normal != 0.0f) d.sigma_n = p->sigma_normal;
        if (p->sigma_position != 0.0f) d.sigma_x = p->sigma_position;
    }
    if (d.levels < 1 || d.levels > 10) { std::snprintf(why, cap, "levels must be 1..10 (0 = the default 5), not %d", d.levels); return false; }
    *out = d;
    return true;
}
int denoise_keep_variance(evplp_context *c) {
    const size_t px = (size_t)c->st.W * c->st.local_rows;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int rc = alloc_once(c, "evplp_denoise", (void **)&c->d_dn_var, sizeof(float) * 3 * std::max<size_t>(px, 1));
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_dn_var, c->d_rgb, sizeof(float) * 3 * px, hipMemcpyDeviceToDevice, c->stream));
    return EVPLP_OK;
}
int denoise_prepare(evplp_context *c, const float4 *pos, const float4 *nrm, const float4 *dif, const float4 *phg, const float4 *light) {
    const size_t px = (size_t)c->st.W * c->st.local_rows;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int rc = alloc_once(c, "evplp_denoise", (void **)&c->d_dn_pack, sizeof(DenoisePixel) * std::max<size_t>(px, 1));
    if (rc) return rc;
    launch_denoise_prepare(c->st, c->d_rgb, c->d_dn_var, pos, nrm, dif, phg, light, (float4 *)c->d_dn_pack, c->stream);
    HIP_TRY(c, hipGetLastError());
    return EVPLP_OK;
}
int denoise_filter(evplp_context *c, const DenoisePixel *frame, int rows, const DenoiseSettings &ds, float radius, float *out_rgb) {
    const size_t px = (size_t)c->st.W * rows;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    if (c->d_dn_u && c->dn_u_px < px) { hipFree(c->d_dn_u); c->d_dn_u = nullptr; }
    int rc = alloc_once(c, "evplp_denoise", (void **)&c->d_dn_u, sizeof(float4) * 2 * std::max<size_t>(px, 1));
    if (rc) return rc;
    c->dn_u_px = std::max(c->dn_u_px, px);
    DenoiseLevelArgs a{};
    a.frame = frame; a.W = c->st.W; a.rows = rows;
    a.sigma_l = ds.sigma_l; a.sigma_n = ds.sigma_n; a.sigma_x_r = ds.sigma_x * radius;
    for (int i = 0; i < ds.levels; i++) {
        a.in = i == 0 ? &frame->u : c->d_dn_u + (size_t)((i - 1) & 1) * px;
        a.in_step = i == 0 ? kDenoiseFloats / 4 : 1;
        a.out = c->d_dn_u + (size_t)(i & 1) * px;
        a.h = 1 << i;
        launch_denoise_level(a, c->stream);
    }
    launch_denoise_finish(frame, c->d_dn_u + (size_t)((ds.levels - 1) & 1) * px, px, out_rgb, c->stream);
    HIP_TRY(c, hipGetLastError());
    return EVPLP_OK;
}
} // namespace evplp
extern "C" int evplp_denoise(evplp_context *c, float scale, float ls, int32_t mask_emitter, const evplp_denoise_params *p, float *out_rgb) {
    CTX_CHECK(c);
    evplp::DenoiseSettings ds; char why[200];
    if (!evplp::denoise_settings(p, &ds, why, sizeof why)) { c->set_error("evplp_denoise: %s", why); return EVPLP_ERR_INVALID; }
    if (!out_rgb) { c->set_error("evplp_denoise: null output"); return EVPLP_ERR_INVALID; }
    if (c->st.strip_count > 1) {
        c->set_error("evplp_denoise: a row-strip context (strip_count %d) cannot see its neighbours' rows: use evplp_group_denoise", c->st.strip_count);
        return EVPLP_ERR_INVALID;
    }
    if (!c->accel_built) { c->set_error("evplp_denoise: no scene (evplp_build_accel): the position term needs its bounding sphere"); return EVPLP_ERR_INVALID; }
    if (c->scene_dirty) { c->set_error("evplp_denoise: vertices were updated (evplp_update_mesh): call evplp_refit_accel or evplp_build_accel first"); return EVPLP_ERR_INVALID; }
    int rc = noise_ready(c, "evplp_denoise");
    if (rc) return rc;
    if ((rc = evplp::noise_variance_to_device(c, evplp::noise_moments_of(c), (double)c->noise_k, (double)c->noise_b, scale))) return rc;
    if ((rc = evplp::denoise_keep_variance(c))) return rc;
    if ((rc = evplp::resolve_to_device(c, scale, scale, ls, mask_emitter, 0, true, false))) return rc;
    if ((rc = evplp::denoise_prepare(c, (const float4 *)c->buf[EVPLP_BUF_GBUF_POSITION], (const float4 *)c->buf[EVPLP_BUF_GBUF_NORMAL],
                                     (const float4 *)c->buf[EVPLP_BUF_GBUF_DIFFUSE], (const float4 *)c->buf[EVPLP_BUF_GBUF_PHONG], (const float4 *)c->buf[EVPLP_BUF_LIGHT]))) return rc;
    if ((rc = evplp::denoise_filter(c, c->d_dn_pack, c->st.local_rows, ds, c->bounding_radius, c->d_rgb))) return rc;
    HIP_TRY(c, hipMemcpyAsync(out_rgb, c->d_rgb, sizeof(float) * 3 * (size_t)c->st.W * c->st.local_rows, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EVPLP_OK;
}

// ---- temporal accumulation in front of the a-trous passes (include/evplp.h evplp_denoise_temporal, kernels_temporal.hip)
namespace evplp {
bool temporal_settings(const evplp_temporal_params *p, TemporalSettings *out, char *why, size_t cap) {
    TemporalSettings t{ 16, 0.9f };
    if (p) {
        if (p->max_history != 0) t.max_history = p->max_history;
        if (!std::isfinite(p->normal_cos)) { std::snprintf(why, cap, "normal_cos must be in (0, 1] (0 = the default 0.9), not %g", (double)p->normal_cos); return false; }
        if (p->normal_cos != 0.0f) t.normal_cos = p->normal_cos;
    }
    if (t.max_history < 1 || t.max_history > 1024) { std::snprintf(why, cap, "max_history must be 1..1024 (0 = the default 16), not %d", t.max_history); return false; }
    if (!(t.normal_cos > 0.0f) || t.normal_cos > 1.0f) { std::snprintf(why, cap, "normal_cos must be in (0, 1] (0 = the default 0.9), not %g", (double)t.normal_cos); return false; }
    *out = t;
    return true;
}
bool temporal_check(evplp_context *c, const char *name, bool needs_primary) {
    if (!c->tp_on) { c->set_error("%s: temporal accumulation is off (evplp_temporal_enable)", name); return false; }
    if (!needs_primary) return true;
    if (c->gbuf_pos_exposed || !c->buf_owned[EVPLP_BUF_GBUF_POSITION]) {
        c->set_error("%s: EVPLP_BUF_GBUF_POSITION is bound or exposed to the caller: the previous-pose walk cannot vouch for a plane it did not write", name);
        return false;
    }
    if (!c->primary_current) {
        c->set_error("%s: no evplp_primary has written the G-buffer since the last evplp_build_accel / evplp_refit_accel / upload of the position plane", name);
        return false;
    }
    return true;
}
void temporal_forget(evplp_context *c) { c->tp_frames = 0; }
static void temporal_release(evplp_context *c) {
    hipFree(c->d_tp_prev_v); hipFree(c->d_tp_prev); hipFree(c->d_tp_prev_frame); hipFree(c->d_tp_hist); hipFree(c->d_tp_counts);
    c->d_tp_prev_v = nullptr; c->d_tp_prev = c->d_tp_prev_frame = nullptr; c->d_tp_hist = nullptr; c->d_tp_counts = nullptr;
    c->tp_tris = 0; c->tp_hist_px = 0; c->tp_count_slots = 0; c->tp_frames = 0; c->tp_cur = 0; c->tp_on = false;
}
// the previous pose follows the scene's triangle count: another count forgets the history and makes the array anew
int temporal_pose_array(evplp_context *c) {
    if (c->d_tp_prev_v && c->tp_tris == c->scene_tris) return EVPLP_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    hipFree(c->d_tp_prev_v); c->d_tp_prev_v = nullptr; c->tp_frames = 0;
    c->tp_tris = c->scene_tris;
    return alloc_once(c, "evplp_denoise_temporal", (void **)&c->d_tp_prev_v, sizeof(float) * 9 * (size_t)std::max(c->scene_tris, 1));
}
int temporal_enable(evplp_context *c, int32_t on) {
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    if (!on) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        temporal_release(c);
        return EVPLP_OK;
    }
    if (c->tp_on) return EVPLP_OK;
    int rc = temporal_pose_array(c);
    if (!rc) rc = alloc_once(c, "evplp_denoise_temporal", (void **)&c->d_tp_prev, sizeof(TemporalPrev) * (size_t)c->st.W * c->st.local_rows);
    if (rc) { temporal_release(c); return rc; }
    c->tp_on = true; c->tp_frames = 0;
    return EVPLP_OK;
}
static void temporal_primary_args(evplp_context *c, PrimaryArgs &a) {
    std::memset(&a, 0, sizeof(a));
    a.sc = c->sc; a.st = c->st; a.cam = c->cam;
    a.jitter[0] = c->primary_jitter[0]; a.jitter[1] = c->primary_jitter[1]; a.clear_light = c->primary_flags;
    // (the walk starts where evplp_primary's did: from the eye's entry cuts under the same test)
    if (c->env_cuts != 0 && c->tiles_x * c->tiles_y > 0 && jitter_within_cuts(c, a.jitter)) primary_cuts_into(c, a);
}
int temporal_prev_pose(evplp_context *c) {
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    PrimaryArgs a; temporal_primary_args(c, a);
    launch_prev_pose(a, c->d_tp_prev_v, c->d_tp_prev, nullptr, c->stream);
    HIP_TRY(c, hipGetLastError());
    return EVPLP_OK;
}
int temporal_accumulate(evplp_context *c, DenoisePixel *frame, const TemporalPrev *prev, int rows, const DenoiseSettings &ds, const TemporalSettings &ts, float radius) {
    const size_t px = std::max<size_t>((size_t)c->st.W * rows, 1);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    if (c->d_tp_hist && c->tp_hist_px != px) { HIP_TRY(c, hipStreamSynchronize(c->stream)); hipFree(c->d_tp_hist); c->d_tp_hist = nullptr; c->tp_frames = 0; }
    int rc = alloc_once(c, "evplp_denoise_temporal", (void **)&c->d_tp_hist, sizeof(float4) * 6 * px);
    const int slots = temporal_count_slots(c->st.W, rows);
    if (c->d_tp_counts && c->tp_count_slots < slots) { HIP_TRY(c, hipStreamSynchronize(c->stream)); hipFree(c->d_tp_counts); c->d_tp_counts = nullptr; }
    if (!rc) rc = alloc_once(c, "evplp_denoise_temporal", (void **)&c->d_tp_counts, sizeof(uint4) * (size_t)slots);
    if (rc) return rc;
    c->tp_hist_px = px; c->tp_count_slots = slots;
    TemporalArgs a{};
    a.frame = frame; a.prev = prev; a.px = px;
    a.h_in = c->d_tp_hist + (size_t)c->tp_cur * 3 * px; a.h_out = c->d_tp_hist + (size_t)(c->tp_cur ^ 1) * 3 * px;
    a.counts = c->d_tp_counts;
    a.W = c->st.W; a.rows = rows; a.H = c->st.H; a.has_history = c->tp_frames > 0 ? 1 : 0;
    a.cam = c->cam; a.prev_cam = c->tp_prev_cam;
    a.sigma_x_r = ds.sigma_x * radius; a.normal_cos = ts.normal_cos; a.max_history = (float)ts.max_history;
    launch_temporal_accumulate(a, c->stream);
    HIP_TRY(c, hipGetLastError());
    c->tp_cur ^= 1;
    return EVPLP_OK;
}
int temporal_snapshot(evplp_context *c) {
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    launch_pose_snapshot(c->sc.attrs, c->tp_tris, c->d_tp_prev_v, c->stream);
    HIP_TRY(c, hipGetLastError());
    c->tp_prev_cam = c->cam;
    c->tp_frames++;
    return EVPLP_OK;
}
int temporal_info(evplp_context *c, evplp_temporal_info *out) {
    unsigned long long n[4] = { 0, 0, 0, 0 };
    std::vector<uint4> slots((size_t)c->tp_count_slots);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipMemcpyAsync(slots.data(), c->d_tp_counts, sizeof(uint4) * slots.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (const uint4 &s : slots) { n[0] += s.x; n[1] += s.y; n[2] += s.z; n[3] += s.w; }
    std::memset(out, 0, sizeof(*out));
    out->filtered = (int64_t)n[0]; out->reprojected = (int64_t)n[1]; out->disoccluded = (int64_t)n[2]; out->history_sum = (int64_t)n[3];
    out->frames_since_reset = c->tp_frames;
    return EVPLP_OK;
}
} // namespace evplp
extern "C" int evplp_temporal_enable(evplp_context *c, int32_t on) {
    CTX_CHECK(c);
    return evplp::temporal_enable(c, on);
}
extern "C" int evplp_temporal_reset(evplp_context *c) {
    CTX_CHECK(c);
    if (!c->tp_on) { c->set_error("evplp_temporal_reset: temporal accumulation is off (evplp_temporal_enable)"); return EVPLP_ERR_INVALID; }
    evplp::temporal_forget(c);
    return EVPLP_OK;
}
extern "C" int evplp_denoise_temporal(evplp_context *c, float scale, float ls, int32_t mask_emitter, const evplp_denoise_params *p,
                                      const evplp_temporal_params *t, float *out_rgb, evplp_temporal_info *info) {
    CTX_CHECK(c);
    const char *name = "evplp_denoise_temporal";
    evplp::DenoiseSettings ds; evplp::TemporalSettings ts; char why[200];
    if (!evplp::denoise_settings(p, &ds, why, sizeof why) || !evplp::temporal_settings(t, &ts, why, sizeof why)) { c->set_error("%s: %s", name, why); return EVPLP_ERR_INVALID; }
    if (!out_rgb) { c->set_error("%s: null output", name); return EVPLP_ERR_INVALID; }
    if (c->st.strip_count > 1) {
        c->set_error("%s: a row-strip context (strip_count %d) cannot see its neighbours' rows: use evplp_group_denoise_temporal", name, c->st.strip_count);
        return EVPLP_ERR_INVALID;
    }
    if (!c->accel_built) { c->set_error("%s: no scene (evplp_build_accel)", name); return EVPLP_ERR_INVALID; }
    if (c->scene_dirty) { c->set_error("%s: vertices were updated (evplp_update_mesh): call evplp_refit_accel or evplp_build_accel first", name); return EVPLP_ERR_INVALID; }
    int rc = noise_ready(c, name);
    if (rc) return rc;
    if (!evplp::temporal_check(c, name, true)) return EVPLP_ERR_INVALID;
    if ((rc = evplp::temporal_pose_array(c))) return rc;                     // (another triangle count: a first call)
    if ((rc = evplp::noise_variance_to_device(c, evplp::noise_moments_of(c), (double)c->noise_k, (double)c->noise_b, scale))) return rc;
    if ((rc = evplp::denoise_keep_variance(c))) return rc;
    if ((rc = evplp::resolve_to_device(c, scale, scale, ls, mask_emitter, 0, true, false))) return rc;
    if ((rc = evplp::denoise_prepare(c, (const float4 *)c->buf[EVPLP_BUF_GBUF_POSITION], (const float4 *)c->buf[EVPLP_BUF_GBUF_NORMAL],
                                     (const float4 *)c->buf[EVPLP_BUF_GBUF_DIFFUSE], (const float4 *)c->buf[EVPLP_BUF_GBUF_PHONG], (const float4 *)c->buf[EVPLP_BUF_LIGHT]))) return rc;
    if (c->tp_frames > 0) { if ((rc = evplp::temporal_prev_pose(c))) return rc; }
    else HIP_TRY(c, hipMemsetAsync(c->d_tp_prev, 0, sizeof(evplp::TemporalPrev) * (size_t)c->st.W * c->st.local_rows, c->stream));
    if ((rc = evplp::temporal_accumulate(c, c->d_dn_pack, c->d_tp_prev, c->st.local_rows, ds, ts, c->bounding_radius))) return rc;
    if ((rc = evplp::denoise_filter(c, c->d_dn_pack, c->st.local_rows, ds, c->bounding_radius, c->d_rgb))) return rc;
    if ((rc = evplp::temporal_snapshot(c))) return rc;
    HIP_TRY(c, hipMemcpyAsync(out_rgb, c->d_rgb, sizeof(float) * 3 * (size_t)c->st.W * c->st.local_rows, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (info) return evplp::temporal_info(c, info);
    return EVPLP_OK;
}
extern "C" int evplp_temporal_download(evplp_context *c, int32_t which, float *out) {
    CTX_CHECK(c);
    const char *name = "evplp_temporal_download";
    if (!out || which < EVPLP_TEMPORAL_HISTORY_U || which > EVPLP_TEMPORAL_DEBUG_HIT) { c->set_error("%s: a null output or an unknown plane %d", name, which); return EVPLP_ERR_INVALID; }
    if (!evplp::temporal_check(c, name, false)) return EVPLP_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const size_t px = (size_t)c->st.W * c->st.local_rows;
    if (which <= EVPLP_TEMPORAL_HISTORY_NRM) {
        if (!c->d_tp_hist || c->tp_frames == 0 || c->tp_hist_px != std::max<size_t>(px, 1)) { c->set_error("%s: this context holds no history of its planes", name); return EVPLP_ERR_INVALID; }
        HIP_TRY(c, hipMemcpyAsync(out, c->d_tp_hist + ((size_t)c->tp_cur * 3 + (size_t)which) * c->tp_hist_px, sizeof(float4) * px, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return EVPLP_OK;
    }
    if (which == EVPLP_TEMPORAL_DEBUG_HIT) {
        if (!c->accel_built || c->scene_dirty) { c->set_error("%s: no scene, or vertices were updated since its last refit", name); return EVPLP_ERR_INVALID; }
        if (!evplp::temporal_check(c, name, true)) return EVPLP_ERR_INVALID;
        float4 *d = nullptr;
        HIP_TRY(c, hipMalloc((void **)&d, sizeof(float4) * std::max<size_t>(px, 1)));
        HIP_TRY(c, hipMemsetAsync(d, 0, sizeof(float4) * std::max<size_t>(px, 1), c->stream));
        PrimaryArgs a; evplp::temporal_primary_args(c, a);
        launch_prev_pose(a, c->d_tp_prev_v, nullptr, d, c->stream);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(out, d, sizeof(float4) * px, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        hipFree(d);
        if (e != hipSuccess) { c->set_error("%s: %s", name, hipGetErrorString(e)); return EVPLP_ERR_HIP; }
        return EVPLP_OK;
    }
    std::vector<evplp::TemporalPrev> host(px);
    HIP_TRY(c, hipMemcpyAsync(host.data(), c->d_tp_prev, sizeof(evplp::TemporalPrev) * px, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < px; i++) std::memcpy(out + 4 * i, which == EVPLP_TEMPORAL_PREV_POS ? &host[i].pos : &host[i].nrm, 16);
    return EVPLP_OK;
}

// ---- adaptive gather: tiles retire once their estimated noise is low enough (include/evplp.h evplp_adaptive_*)
static void release_adapt(evplp_context *c) {
    hipFree(c->d_adapt_tiles); hipFree(c->d_adapt_snap); hipFree(c->d_adapt_mask);
    c->d_adapt_tiles = nullptr; c->d_adapt_snap = nullptr; c->d_adapt_mask = nullptr; c->adapt_tiles.clear(); c->adapt_pt = false; c->adapt_budget = false;
    c->adapt_gather_budget = false; c->adapt_m = 0;
}
static size_t adapt_tile_count(const evplp_context *c) { return (size_t)c->tiles_x * (size_t)c->tiles_y; }
// every tile active (stream order); the records are (re)allocated when the planes' tiles have changed (a new block table)
static int adapt_reset(evplp_context *c) {
    const size_t nt = adapt_tile_count(c), px = (size_t)c->st.W * c->st.local_rows;
    if (c->adapt_tiles.size() != nt) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        hipFree(c->d_adapt_tiles); hipFree(c->d_adapt_snap); hipFree(c->d_adapt_mask); c->d_adapt_tiles = nullptr; c->d_adapt_snap = nullptr; c->d_adapt_mask = nullptr;
        hipFree(c->d_pt_first); hipFree(c->d_tile_noise); c->d_pt_first = nullptr; c->d_tile_noise = nullptr;       // (sized by the tile count too)
        hipError_t e = hipMalloc((void **)&c->d_adapt_tiles, sizeof(int4) * std::max<size_t>(nt, 1));
        if (e == hipSuccess) e = hipMalloc((void **)&c->d_adapt_snap, sizeof(float4) * std::max<size_t>(px, 1));
        if (e != hipSuccess) {
            (void)hipGetLastError(); release_adapt(c);
            c->set_error("evplp_adaptive_enable: cannot allocate %zu bytes: %s", sizeof(int4) * nt + sizeof(float4) * px, hipGetErrorString(e));
            return e == hipErrorOutOfMemory ? EVPLP_ERR_OOM : EVPLP_ERR_HIP;
        }
    }
    // gather budget mode alone pays for the per-call view of the records (16 B per tile); the other modes never touch it
    if (c->adapt_gather_budget && !c->d_adapt_mask) {
        const hipError_t e = hipMalloc((void **)&c->d_adapt_mask, sizeof(int4) * std::max<size_t>(nt, 1));
        if (e != hipSuccess) {
            (void)hipGetLastError(); release_adapt(c);
            c->set_error("evplp_adaptive_enable: cannot allocate %zu bytes: %s", sizeof(int4) * nt, hipGetErrorString(e));
            return e == hipErrorOutOfMemory ? EVPLP_ERR_OOM : EVPLP_ERR_HIP;
        }
    }
    c->adapt_tiles.assign(nt, make_int4(0, 0, 0, c->adapt_budget ? -1 : 0));
    c->adapt_m = 0;
    if (c->adapt_budget) {
        // budget mode: every record { 0, 0, 0, -1 } (all samples of a call), and the raw sums R start as the accumulator itself (N = 0)
        if (nt) HIP_TRY(c, hipMemcpyAsync(c->d_adapt_tiles, c->adapt_tiles.data(), sizeof(int4) * nt, hipMemcpyHostToDevice, c->stream));
        if (px) HIP_TRY(c, hipMemcpyAsync(c->d_adapt_snap, c->buf[EVPLP_BUF_VPL_ACCUM], sizeof(float4) * px, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return EVPLP_OK;
    }
    HIP_TRY(c, hipMemsetAsync(c->d_adapt_tiles, 0, sizeof(int4) * std::max<size_t>(nt, 1), c->stream));
    return EVPLP_OK;
}
// pt: path-trace mode (evplp_adaptive_enable_pt) -- the same records and snapshot; what differs is the pass that honours them
static int adaptive_enable_mode(evplp_context *c, int32_t on, bool pt, const char *name) {
    if (c->adapt_n > 0) {
        c->set_error("%s: %lld gather(s) have accumulated since the last clear: switch adaptivity before the first", name, (long long)c->adapt_n);
        return EVPLP_ERR_INVALID;
    }
    if (on && !c->d_noise) { c->set_error("%s: noise tracking is off (evplp_noise_track): retirement needs its estimate", name); return EVPLP_ERR_INVALID; }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    if (!on) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        release_adapt(c);
        return EVPLP_OK;
    }
    // on = 2: budget mode, the path tracer's (pt) or the gathers'
    const bool budget = on == 2;
    if (budget && !pt && c->splat_n > 0) {
        c->set_error("%s: %lld photon splat(s) since the last clear: gather budget mode has no place for them (evplp_clear_accumulators)", name, (long long)c->splat_n);
        return EVPLP_ERR_INVALID;
    }
    const bool was = c->adapt_budget, was_gather = c->adapt_gather_budget;
    c->adapt_budget = budget; c->adapt_gather_budget = budget && !pt;       // (adapt_reset allocates by these)
    const int rc = adapt_reset(c);
    if (rc == EVPLP_OK) {
        c->adapt_pt = pt; c->adapt_window = 16;
        if (!c->adapt_gather_budget && c->d_adapt_mask) { hipFree(c->d_adapt_mask); c->d_adapt_mask = nullptr; }     // (left the mode with N = 0: nothing in flight reads it)
    } else { c->adapt_budget = c->d_adapt_tiles ? was : false; c->adapt_gather_budget = c->d_adapt_tiles ? was_gather : false; }
    return rc;
}
extern "C" int evplp_adaptive_enable(evplp_context *c, int32_t on) { CTX_CHECK(c); return adaptive_enable_mode(c, on, false, "evplp_adaptive_enable"); }
extern "C" int evplp_adaptive_enable_pt(evplp_context *c, int32_t on) { CTX_CHECK(c); return adaptive_enable_mode(c, on, true, "evplp_adaptive_enable_pt"); }
extern "C" int evplp_adaptive_retire(evplp_context *c, float scale, float ls, int32_t mask_emitter, double tau, int32_t min_batches) {
    CTX_CHECK(c);
    if (!c->d_adapt_tiles) { c->set_error("evplp_adaptive_retire: adaptivity is off (evplp_adaptive_enable)"); return EVPLP_ERR_INVALID; }
    if (c->adapt_budget) { c->set_error("evplp_adaptive_retire: budget mode (evplp_adaptive_enable(ctx, 2) / evplp_adaptive_enable_pt(ctx, 2)): set the tile's budget to 0 instead (evplp_adaptive_set_budgets)"); return EVPLP_ERR_INVALID; }
    if (!c->d_noise) { c->set_error("evplp_adaptive_retire: noise tracking is off (evplp_noise_track)"); return EVPLP_ERR_INVALID; }
    if (!(tau >= 0.0)) { c->set_error("evplp_adaptive_retire: tile_rel_mse must be >= 0, not %g", tau); return EVPLP_ERR_INVALID; }
    if (min_batches < 2) { c->set_error("evplp_adaptive_retire: min_batches must be >= 2, not %d", min_batches); return EVPLP_ERR_INVALID; }
    c->adapt_last = 0;
    if (c->noise_b < min_batches || c->adapt_n < 1) return 0;
    // (the composite the estimate measures; the pending splat's verdict first, as a fold waits for it)
    int rc = evplp::resolve_to_device(c, scale, scale, ls, mask_emitter, 0, true, false);
    if (rc) return rc;
    const double K = (double)c->noise_k, B = (double)c->noise_b;
    launch_adaptive_retire(c->st, evplp::noise_moments_of(c), K, B, (double)scale * (double)scale * K, (const float4 *)c->buf[EVPLP_BUF_LIGHT], ls, mask_emitter,
                           c->d_rgb, tau, c->d_adapt_tiles, c->tiles_x, c->tiles_y, (int32_t)c->adapt_n, (const float4 *)c->buf[EVPLP_BUF_VPL_ACCUM], c->d_adapt_snap, c->stream);
    HIP_TRY(c, hipGetLastError());
    const size_t nt = adapt_tile_count(c);
    std::vector<int4> now(nt);
    if (nt) HIP_TRY(c, hipMemcpyAsync(now.data(), c->d_adapt_tiles, sizeof(int4) * nt, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    int32_t fresh = 0;
    for (size_t t = 0; t < nt; t++) fresh += (c->adapt_tiles[t].x == 0 && now[t].x != 0) ? 1 : 0;
    c->adapt_tiles.swap(now);
    c->adapt_last = fresh;
    return fresh;
}
namespace evplp {
void adaptive_tiles_into(const evplp_context *c, int32_t *out) {
    const int itx = (c->st.W + 7) / 8;
    for (int ty = 0; ty < c->tiles_y; ty++) {
        const int y = c->st.global_row(ty * 8);
        if (y < 0 || y >= c->st.H) continue;
        for (int tx = 0; tx < c->tiles_x; tx++) {
            const int32_t nt = c->adapt_tiles[(size_t)ty * c->tiles_x + tx].x;
            out[(size_t)(y / 8) * itx + tx] = nt != 0 || c->adapt_budget ? nt : (int32_t)c->adapt_n;
        }
    }
}
}
extern "C" int evplp_adaptive_tiles(evplp_context *c, int32_t *out, int32_t capacity) {
    CTX_CHECK(c);
    if (!c->d_adapt_tiles) { c->set_error("evplp_adaptive_tiles: adaptivity is off (evplp_adaptive_enable)"); return EVPLP_ERR_INVALID; }
    const int64_t n = (int64_t)((c->st.W + 7) / 8) * ((c->st.H + 7) / 8);
    if (!out || capacity < n) { c->set_error("evplp_adaptive_tiles: the image has %lld tiles, the output holds %d", (long long)n, capacity); return EVPLP_ERR_INVALID; }
    std::fill(out, out + n, 0);
    evplp::adaptive_tiles_into(c, out);
    return (int)n;
}

// ---- budget mode of the path tracer (include/evplp.h evplp_adaptive_set_budgets): the image-tile layout is evplp_adaptive_tiles'
static int64_t image_tile_count(const evplp_context *c) { return (int64_t)((c->st.W + 7) / 8) * ((c->st.H + 7) / 8); }
// f(local tile, image tile) for every tile of the planes that lies in the image
template <class F> static void for_own_tiles(const evplp_context *c, F f) {
    const int itx = (c->st.W + 7) / 8;
    for (int ty = 0; ty < c->tiles_y; ty++) {
        const int y = c->st.global_row(ty * 8);
        if (y < 0 || y >= c->st.H) continue;
        for (int tx = 0; tx < c->tiles_x; tx++) f((size_t)ty * c->tiles_x + tx, (size_t)(y / 8) * itx + tx);
    }
}
extern "C" int evplp_adaptive_set_budgets(evplp_context *c, const int32_t *samples_per_image_tile, int32_t count) {
    CTX_CHECK(c);
    const char *name = "evplp_adaptive_set_budgets";
    if (!c->adapt_budget) { c->set_error("%s: budget mode is off (evplp_adaptive_enable(ctx, 2) / evplp_adaptive_enable_pt(ctx, 2))", name); return EVPLP_ERR_INVALID; }
    const int64_t n = image_tile_count(c);
    if (!samples_per_image_tile || count != n) { c->set_error("%s: the image has %lld tiles, the call gives %d", name, (long long)n, samples_per_image_tile ? count : 0); return EVPLP_ERR_INVALID; }
    for (int64_t t = 0; t < n; t++)
        if (samples_per_image_tile[t] < 0 || samples_per_image_tile[t] > kPtBatchMaxSamples) {
            c->set_error("%s: tile %lld: a budget is 0 .. %d samples, not %d", name, (long long)t, kPtBatchMaxSamples, samples_per_image_tile[t]); return EVPLP_ERR_INVALID;
        }
    // (every tile then has B_t >= 2 and n_t >= 1 before one can fall behind: B_t - 1 and n_t are denominators)
    if (c->noise_b < 2) { c->set_error("%s: %lld fold(s): budgets need >= 2 (evplp_noise_fold)", name, (long long)c->noise_b); return EVPLP_ERR_INVALID; }
    if (c->noise_k != c->adapt_n) { c->set_error("%s: %lld of %lld samples are folded: fold first (evplp_noise_fold)", name, (long long)c->noise_k, (long long)c->adapt_n); return EVPLP_ERR_INVALID; }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    for_own_tiles(c, [&](size_t local, size_t image) { c->adapt_tiles[local].w = samples_per_image_tile[image]; });
    c->adapt_m = 0;                 // (gather budget mode: a new window starts)
    const size_t nt = adapt_tile_count(c);
    if (nt) HIP_TRY(c, hipMemcpyAsync(c->d_adapt_tiles, c->adapt_tiles.data(), sizeof(int4) * nt, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EVPLP_OK;
}
extern "C" int evplp_adaptive_budget_window(evplp_context *c, int32_t window) {
    CTX_CHECK(c);
    const char *name = "evplp_adaptive_budget_window";
    if (!c->adapt_gather_budget) { c->set_error("%s: gather budget mode is off (evplp_adaptive_enable(ctx, 2))", name); return EVPLP_ERR_INVALID; }
    if (window < 1 || window > kGatherBudgetMaxWindow) { c->set_error("%s: a window is 1 .. %d calls, not %d", name, kGatherBudgetMaxWindow, window); return EVPLP_ERR_INVALID; }
    c->adapt_window = window; c->adapt_m = 0;
    return EVPLP_OK;
}
extern "C" int evplp_adaptive_budgets(evplp_context *c, int32_t *out, int32_t capacity) {
    CTX_CHECK(c);
    if (!c->adapt_budget) { c->set_error("evplp_adaptive_budgets: budget mode is off (evplp_adaptive_enable(ctx, 2) / evplp_adaptive_enable_pt(ctx, 2))"); return EVPLP_ERR_INVALID; }
    const int64_t n = image_tile_count(c);
    if (!out || capacity < n) { c->set_error("evplp_adaptive_budgets: the image has %lld tiles, the output holds %d", (long long)n, capacity); return EVPLP_ERR_INVALID; }
    std::fill(out, out + n, 0);
    evplp::adaptive_budgets_into(c, out);
    return (int)n;
}
namespace evplp {
void adaptive_budgets_into(const evplp_context *c, int32_t *out) {
    for_own_tiles(c, [&](size_t local, size_t image) { out[image] = c->adapt_tiles[local].w; });
}
// (the composite the estimate measures first, as evplp_adaptive_retire forms it)
int adaptive_tile_noise_into(evplp_context *c, float scale, float ls, int32_t mask_emitter, double *out) {
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const size_t nt = adapt_tile_count(c);
    if (nt && !c->d_tile_noise) HIP_TRY(c, hipMalloc((void **)&c->d_tile_noise, sizeof(double) * nt));
    int rc = resolve_to_device(c, scale, scale, ls, mask_emitter, 0, true, false);
    if (rc) return rc;
    const double K = (double)c->noise_k, B = (double)c->noise_b;
    launch_tile_noise(c->st, noise_moments_of(c), K, B, (double)scale * (double)scale * K, (const float4 *)c->buf[EVPLP_BUF_LIGHT], ls, mask_emitter,
                      c->d_rgb, adapt_view(c, scale), (int32_t)nt, c->d_tile_noise, c->stream);
    HIP_TRY(c, hipGetLastError());
    std::vector<double> local(nt);
    if (nt) HIP_TRY(c, hipMemcpyAsync(local.data(), c->d_tile_noise, sizeof(double) * nt, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for_own_tiles(c, [&](size_t l, size_t image) { out[image] = local[l]; });
    return EVPLP_OK;
}
}
extern "C" int evplp_adaptive_tile_noise(evplp_context *c, float scale, float ls, int32_t mask_emitter, double *rel_per_image_tile, int32_t capacity) {
    CTX_CHECK(c);
    const char *name = "evplp_adaptive_tile_noise";
    if (!c->d_adapt_tiles) { c->set_error("%s: adaptivity is off (evplp_adaptive_enable)", name); return EVPLP_ERR_INVALID; }
    const int64_t n = image_tile_count(c);
    if (!rel_per_image_tile || capacity < n) { c->set_error("%s: the image has %lld tiles, the output holds %d", name, (long long)n, capacity); return EVPLP_ERR_INVALID; }
    int rc = noise_ready(c, name);
    if (rc) return rc;
    std::fill(rel_per_image_tile, rel_per_image_tile + n, 0.0);
    if ((rc = evplp::adaptive_tile_noise_into(c, scale, ls, mask_emitter, rel_per_image_tile))) return rc;
    return (int)n;
}

static void count_rows_in_image(evplp_context *c) {
    c->rows_in_image = 0;
    for (int l = 0; l < c->st.local_rows; l++) if (c->st.global_row(l) < c->st.H) c->rows_in_image++;
}

// ---- dealt blocks (include/evplp.h): the owned-block table of a row-strip context, and the per-block cost the deal is made from
extern "C" int evplp_set_blocks(evplp_context *c, const int32_t *image_blocks, int32_t count) {
    CTX_CHECK(c);
    { int rc_ = settle_splat(c); if (rc_) return rc_; }
    if (c->st.strip_count <= 1) { c->set_error("evplp_set_blocks: the context is not a row-strip context (strip_count > 1)"); return EVPLP_ERR_INVALID; }
    const int cap = c->st.cap_blocks, nb = c->image_blocks;
    if (image_blocks && (count < 0 || count > cap)) { c->set_error("evplp_set_blocks: %d blocks do not fit the context's %d (strip_capacity_rows)", count, cap); return EVPLP_ERR_INVALID; }
    std::vector<int32_t> table;
    if (image_blocks) {
        table.assign((size_t)cap + nb, -1);
        for (int l = 0; l < cap; l++) table[(size_t)l] = nb + l;                   // holds nothing: rows >= H
        for (int l = 0; l < count; l++) {
            const int b = image_blocks[l];
            if (b < 0 || b >= nb || table[(size_t)cap + b] >= 0) { c->set_error("evplp_set_blocks: block %d is outside the image's %d blocks or listed twice", b, nb); return EVPLP_ERR_INVALID; }
            table[(size_t)l] = b; table[(size_t)cap + b] = l;
        }
    }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); if (c->aux_stream) HIP_TRY(c, hipStreamSynchronize(c->aux_stream));
    if (image_blocks) {
        if (!c->d_blocks) HIP_TRY(c, hipMalloc((void **)&c->d_blocks, sizeof(int32_t) * ((size_t)cap + nb)));
        HIP_TRY(c, hipMemcpy(c->d_blocks, table.data(), sizeof(int32_t) * table.size(), hipMemcpyHostToDevice));
        c->blocks_host.swap(table);
        c->st.blocks = c->d_blocks; c->st.blocks_host = c->blocks_host.data();
    } else { c->st.blocks = nullptr; c->st.blocks_host = nullptr; c->blocks_host.clear(); }       // back to block b -> rank b % strip_count
    count_rows_in_image(c);
    c->primary_cuts_valid = false; c->tile_box_valid = false; c->primary_current = false;
    return evplp_clear_accumulators(c);
}
extern "C" int evplp_get_blocks(evplp_context *c, int32_t *image_blocks, int32_t capacity) {
    CTX_CHECK(c);
    int n = 0;
    const int cap = c->st.local_rows / c->st.strip_rows;
    for (int l = 0; l < cap; l++) {
        const int b = c->st.global_block(l);
        if (b >= c->image_blocks) continue;
        if (image_blocks && n < capacity) image_blocks[n] = b;
        n++;
    }
    return n;
}
extern "C" int evplp_calibrate_blocks(evplp_context *c, int32_t on) {
    CTX_CHECK(c);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const size_t bytes = sizeof(unsigned long long) * (size_t)std::max(c->st.local_rows / std::max(c->st.strip_rows, 1), 1);
    if (on) {
        if (!c->d_block_cost) HIP_TRY(c, hipMalloc((void **)&c->d_block_cost, bytes));
        HIP_TRY(c, hipMemsetAsync(c->d_block_cost, 0, bytes, c->stream));
    }
    c->calibrate = on != 0;
    return EVPLP_OK;
}
extern "C" int evplp_block_costs(evplp_context *c, uint64_t *cost_per_image_block, int32_t capacity) {
    CTX_CHECK(c);
    if (!cost_per_image_block || capacity < c->image_blocks) { c->set_error("evplp_block_costs: the output needs room for %d blocks", c->image_blocks); return EVPLP_ERR_INVALID; }
    if (!c->d_block_cost) { c->set_error("evplp_block_costs: no calibration has run (evplp_calibrate_blocks)"); return EVPLP_ERR_INVALID; }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const int cap = c->st.local_rows / c->st.strip_rows;
    std::vector<unsigned long long> local((size_t)cap);
    HIP_TRY(c, hipMemcpyAsync(local.data(), c->d_block_cost, sizeof(unsigned long long) * local.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int b = 0; b < c->image_blocks; b++) cost_per_image_block[b] = 0;
    int n = 0;
    for (int l = 0; l < cap; l++) {
        const int b = c->st.global_block(l);
        if (b < c->image_blocks) { cost_per_image_block[b] += local[(size_t)l]; n++; }
    }
    return n;
}

extern "C" int evplp_clear_accumulators(evplp_context *c) {
    CTX_CHECK(c);
    { int rc_ = settle_splat(c); if (rc_) return rc_; }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipMemsetAsync(c->buf[EVPLP_BUF_VPL_ACCUM], 0, buffer_bytes(c, EVPLP_BUF_VPL_ACCUM), c->stream));
    HIP_TRY(c, hipMemsetAsync(c->buf[EVPLP_BUF_PHOTON_ACCUM], 0, buffer_bytes(c, EVPLP_BUF_PHOTON_ACCUM), c->stream));
    HIP_TRY(c, hipMemsetAsync(c->buf[EVPLP_BUF_LIGHT], 0, buffer_bytes(c, EVPLP_BUF_LIGHT), c->stream));
    c->adapt_n = 0; c->splat_n = 0;
    if (c->d_adapt_tiles) { int rc_ = adapt_reset(c); if (rc_) return rc_; }     // (every tile is active again)
    if (c->d_noise) return noise_restart(c);                                  // (noise tracking starts again from the empty sums)
    return EVPLP_OK;
}

// ------------------------------------------------------------------------ buffers / stats
extern "C" int evplp_local_rows(const evplp_context *c) { return c ? c->st.local_rows : EVPLP_ERR_INVALID; }

extern "C" int evplp_buffer_info(evplp_context *c, int32_t which, void **ptr, size_t *bytes) {
    CTX_CHECK(c);
    if (which < 0 || which >= EVPLP_BUF_COUNT) { c->set_error("evplp_buffer_info: bad buffer id %d", which); return EVPLP_ERR_INVALID; }
    if (ptr) {
        *ptr = c->buf[which];
        if (which == EVPLP_BUF_GBUF_POSITION) { c->gbuf_pos_exposed = true; c->tile_box_valid = false; c->primary_current = false; }
        if (which >= EVPLP_BUF_GBUF_POSITION && which <= EVPLP_BUF_GBUF_PHONG) c->gbuf_exposed = true;
        if (which == EVPLP_BUF_RECORDS) c->records_exposed = true;       // the pointer must stay the record buffer: no double buffering
    }
    if (bytes) *bytes = buffer_bytes(c, which);
    return EVPLP_OK;
}
extern "C" int evplp_bind_buffer(evplp_context *c, int32_t which, void *ptr, size_t bytes) {
    CTX_CHECK(c);
    { int rc_ = settle_splat(c); if (rc_) return rc_; }
    if (which < 0 || which >= EVPLP_BUF_COUNT || !ptr) { c->set_error("evplp_bind_buffer: bad arguments"); return EVPLP_ERR_INVALID; }
    if (bytes < buffer_bytes(c, which)) { c->set_error("evplp_bind_buffer: %zu bytes given, %zu needed", bytes, buffer_bytes(c, which)); return EVPLP_ERR_INVALID; }
    if (((uintptr_t)ptr & 15u) != 0) { c->set_error("evplp_bind_buffer: pointer must be 16-byte aligned"); return EVPLP_ERR_INVALID; }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->buf_owned[which]) hipFree(c->buf[which]);
    c->buf[which] = ptr; c->buf_owned[which] = false;
    if (which == EVPLP_BUF_GBUF_POSITION) { c->gbuf_pos_exposed = true; c->tile_box_valid = false; c->primary_current = false; }
    if (which >= EVPLP_BUF_GBUF_POSITION && which <= EVPLP_BUF_GBUF_PHONG) c->gbuf_exposed = true;
    return EVPLP_OK;
}
extern "C" int evplp_download(evplp_context *c, int32_t which, void *dst, size_t bytes) {
    CTX_CHECK(c);
    { int rc_ = settle_splat(c); if (rc_) return rc_; }
    if (which < 0 || which >= EVPLP_BUF_COUNT || !dst || bytes > buffer_bytes(c, which)) { c->set_error("evplp_download: bad arguments"); return EVPLP_ERR_INVALID; }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipMemcpyAsync(dst, c->buf[which], bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EVPLP_OK;
}
extern "C" int evplp_upload(evplp_context *c, int32_t which, const void *src, size_t bytes) {
    CTX_CHECK(c);
    { int rc_ = settle_splat(c); if (rc_) return rc_; }
    if (which < 0 || which >= EVPLP_BUF_COUNT || !src || bytes > buffer_bytes(c, which)) { c->set_error("evplp_upload: bad arguments"); return EVPLP_ERR_INVALID; }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipMemcpyAsync(c->buf[which], src, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (which == EVPLP_BUF_GBUF_POSITION) { c->tile_box_valid = false; c->primary_current = false; }
    return EVPLP_OK;
}

// raw device counters of a pass (diagnostic builds fill the histogram part; see kernels.h PassCounters)
extern "C" int evplp_profile_kernels(evplp_context *c, int32_t on) { CTX_CHECK(c); c->profile_kernels = on != 0; return EVPLP_OK; }
extern "C" int evplp_profile_passes(evplp_context *c, int32_t on) { CTX_CHECK(c); c->profile_passes = on != 0; return EVPLP_OK; }

extern "C" int evplp_debug_counters(evplp_context *c, int32_t pass, uint64_t *out, int32_t capacity) {
    CTX_CHECK(c);
    { int rc_ = settle_splat(c); if (rc_) return rc_; }
    if (pass < 0 || pass >= EVPLP_PASS_COUNT || !out || capacity <= 0) { c->set_error("evplp_debug_counters: bad arguments"); return EVPLP_ERR_INVALID; }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    PassCounters pc;
    HIP_TRY(c, hipMemcpy(&pc, &c->d_counters[pass], sizeof(pc), hipMemcpyDeviceToHost));
    const int n = std::min<int>(capacity, (int)(sizeof(pc) / sizeof(uint64_t)));
    std::memcpy(out, &pc, sizeof(uint64_t) * (size_t)n);
    return n;
}

// what the binning of the last photon splat left behind (tests: which path the photons took, what every tile's bin wanted)
extern "C" int evplp_debug_splat_bins(evplp_context *c, uint32_t *big_count, int32_t n_groups, uint32_t *tile_cursor, int32_t n_tiles) {
    CTX_CHECK(c);
    { int rc_ = settle_splat(c); if (rc_) return rc_; }
    const int32_t groups = std::max(c->num_bin_groups, 0), tiles = c->tiles_x * c->tiles_y;
    if ((big_count && n_groups != groups) || (tile_cursor && n_tiles != tiles)) {
        c->set_error("evplp_debug_splat_bins: the context has %d bin groups and %d tiles, not %d and %d", groups, tiles, n_groups, n_tiles);
        return EVPLP_ERR_INVALID;
    }
    if (!c->pass_ran[EVPLP_PASS_SPLAT]) { c->set_error("evplp_debug_splat_bins: no photon splat has run"); return EVPLP_ERR_INVALID; }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (big_count && groups > 0) HIP_TRY(c, hipMemcpy(big_count, c->d_big_count, sizeof(uint32_t) * (size_t)groups, hipMemcpyDeviceToHost));
    if (tile_cursor && tiles > 0) HIP_TRY(c, hipMemcpy(tile_cursor, c->d_tile_cursor, sizeof(uint32_t) * (size_t)tiles, hipMemcpyDeviceToHost));
    return EVPLP_OK;
}

extern "C" int evplp_pass_stats_get(evplp_context *c, int32_t pass, evplp_pass_stats *out) {
    CTX_CHECK(c);
    { int rc_ = settle_splat(c); if (rc_) return rc_; }
    if (pass < 0 || pass >= EVPLP_PASS_COUNT || !out) { c->set_error("evplp_pass_stats_get: bad arguments"); return EVPLP_ERR_INVALID; }
    std::memset(out, 0, sizeof(*out));
    if (!c->pass_ran[pass]) return EVPLP_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    if (c->pass_timed[pass]) {
        HIP_TRY(c, hipEventSynchronize(c->ev_end[pass]));
        HIP_TRY(c, hipEventElapsedTime(&out->ms, c->ev_begin[pass], c->ev_end[pass]));
    } else {                                                              // (run with evplp_profile_passes off: counters only)
        HIP_TRY(c, hipStreamSynchronize(c->stream)); if (c->aux_stream) HIP_TRY(c, hipStreamSynchronize(c->aux_stream));
    }
    if (c->pass_has_dom[pass]) { HIP_TRY(c, hipEventElapsedTime(&out->dominant_kernel_ms, c->ev_dom_begin[pass], c->ev_dom_end[pass])); out->launches = 1; }
    else { out->dominant_kernel_ms = out->ms; out->launches = 1; }
    PassCounters pc; uint32_t scal[16];
    HIP_TRY(c, hipMemcpy(&pc, &c->d_counters[pass], sizeof(pc), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(scal, c->d_scalars, sizeof(scal), hipMemcpyDeviceToHost));
    const uint64_t px = (uint64_t)c->st.W * c->rows_in_image;
    if (pass == EVPLP_PASS_GATHER_VPL || pass == EVPLP_PASS_GATHER_VSL) {
        unsigned long long rays = 0, shaded = 0;
        for (int k = 0; k < kCounterShards; k++) { rays += pc.shard_rays[k]; shaded += pc.shard_shaded[k]; }
        out->usable = scal[0]; out->pairs = px * scal[0]; out->rays = rays; out->shaded = shaded; out->reserved[0] = (uint32_t)std::min<unsigned long long>(pc.nodes, 0xffffffffull);
        out->reserved[1] = (uint32_t)(pc.nodes >> 32);
        if (pass == EVPLP_PASS_GATHER_VSL && !EVPLP_TRAVERSAL_STATS) {     // VSL: sample-iterations of the estimators (64 shards), in the same two words
            unsigned long long samples = 0; for (int k = 0; k < 64; k++) samples += pc.hist[k];
            out->reserved[0] = (uint32_t)samples; out->reserved[1] = (uint32_t)(samples >> 32);
        }
    } else if (pass == EVPLP_PASS_SPLAT) {
        // per-tile pair counts (a single counter word would take one device-scope atomic per tile: measured 0.28 ms of
        // a 0.41 ms launch at 1920x1080), summed here
        std::vector<uint32_t> tp((size_t)c->tiles_x * c->tiles_y);
        HIP_TRY(c, hipMemcpy(tp.data(), c->d_tile_pairs, tp.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        uint64_t sum = 0; for (uint32_t v : tp) sum += v;
        uint64_t fragments = 0;
        if (c->last_splat_proxy) {                                        // EVPLP_FOOTPRINT_PROXY: fragments of the proxy mesh
            HIP_TRY(c, hipMemcpy(tp.data(), c->d_tile_frags, tp.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
            for (uint32_t v : tp) fragments += v;
        }
        out->pairs = sum; out->rays = fragments; out->usable = 0; out->reserved[0] = c->last_bin_entries; out->reserved[1] = c->last_bin_max;
        // `shaded`: (photon, pixel) pairs of ALL splat passes of this context so far (device-side running total)
        std::vector<uint32_t> sh((size_t)kSummaryFinal);
        HIP_TRY(c, hipMemcpy(sh.data(), c->d_summary, sh.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        uint64_t total = 0;
        for (int k = 0; k < kSummaryShards; k++) total += (uint64_t)sh[(size_t)k * kSummaryStride + 4] | ((uint64_t)sh[(size_t)k * kSummaryStride + 5] << 32);
        out->shaded = total;
    } else if (pass == EVPLP_PASS_PATH_TRACE) { out->pairs = pc.pairs; out->rays = pc.rays; }
    else if (pass == EVPLP_PASS_GATHER_LVC) { out->pairs = pc.pairs; out->rays = pc.rays; }
    else if (pass == EVPLP_PASS_PRIMARY) out->rays = c->stats_host[pass].rays;
    return EVPLP_OK;
}

/*
 * evplp.h -- C ABI of libevplp_hip.so: the MI355X (gfx950) implementation of evplp's
 * per-pixel indirect-radiance accumulation path (VPL/VSL gather with shadow rays,
 * image-space photon splat, and the feeders either side of them).
 *
 * This is the boundary a maintainer of jamornsriwasansak/evplp binds instead of OptiX +
 * OpenGL.  Every entry point names the reference interface it replaces (paths relative to
 * reflectcuts/; rt/ = realtimetechniques/).  Plain pointers and sizes only; no C++ types,
 * no exceptions cross the ABI.  Every call returns EVPLP_OK (0) or a negative evplp_status;
 * evplp_last_error() gives the message.  One caller thread per context; one context per GPU.
 * There is NO CPU fallback: without a usable HIP device evplp_create fails with
 * EVPLP_ERR_NO_DEVICE.
 *
 * Image convention: row-major, y = 0 at the BOTTOM row (OpenGL / OptiX launch index,
 * shaders/final.frag:22-23).  With row strips (multi-GPU) a context owns the rows of the
 * blocks  b = y / strip_rows  with  b % strip_count == strip_rank  and stores them compactly:
 * local_row = (b / strip_count) * strip_rows + y % strip_rows.
 */
#ifndef EVPLP_H
#define EVPLP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EVPLP_ABI_VERSION 5

typedef enum evplp_status {
    EVPLP_OK = 0,
    EVPLP_ERR_INVALID = -1,     /* bad argument / call order */
    EVPLP_ERR_NO_DEVICE = -2,   /* no HIP device / HIP runtime error at creation */
    EVPLP_ERR_HIP = -3,         /* HIP runtime error (message has the hipError string) */
    EVPLP_ERR_IO = -4,          /* file could not be read / written */
    EVPLP_ERR_PARSE = -5,       /* JSON / OBJ syntax or missing required key */
    EVPLP_ERR_OOM = -6
} evplp_status;

/* rt/rtcomphoton/rtphotonrecord.h:9-15 PhotonRecordFlag */
enum {
    EVPLP_USABLE_VPL = 1, EVPLP_USABLE_PHOTON = 2, EVPLP_LAMBERT_ONLY = 4, EVPLP_PHONG_ONLY = 8
};

/* rt/rtcomphoton/rtphotonrecord.h:17-25 RtPhotonRecord (GLSL mirror photonsplatinstanced.frag:25-33):
 * identical 96-byte array-of-structures layout, so record buffers are interchangeable. */
typedef struct evplp_record {
    float pos[3];      uint32_t flags;
    float normal[3];   float p_select_lambert;
    float flux[3];     float pad1;
    float flux_dir[3]; float pad2;
    float rho_d[3];    float pad3;
    float rho_s[3];    float phong_exp;
} evplp_record;

/* rt/rtcomphoton/rtcomphoton.h:64-72 EMis */
typedef enum evplp_mis_mode {
    EVPLP_MIS_ONE = 0, EVPLP_MIS_BALANCE = 1, EVPLP_MIS_MAX = 2, EVPLP_MIS_POWER2 = 3,
    EVPLP_MIS_GEOMETRY_CLAMP = 4, EVPLP_MIS_GEOMETRY_BRDF_CLAMP = 5
} evplp_mis_mode;

typedef enum evplp_bvh_builder {
    EVPLP_BVH_LBVH = 0,   /* Morton-code LBVH (Karras topology) */
    EVPLP_BVH_SAH = 1,    /* binned-SAH top-down build into the same flattened node format (default of the host side) */
    EVPLP_BVH_SBVH = 2,   /* binned SAH with spatial splits (triangle references clipped at split planes; ~20 % more leaf slots) */
    EVPLP_BVH_LBVH_GPU = 3, /* the LBVH built on the device (Morton sort, Karras hierarchy, bottom-up refit): for scenes that change */
    EVPLP_BVH_PLOC_GPU = 4  /* built on the device by locally-ordered clustering (PLOC, Meister & Bittner 2018) over the same Morton sort: every
                             * cluster merges with its nearest neighbour within 16 positions where the choice is mutual; one small host
                             * read-back per iteration, so a slower build than the device LBVH and a better tree (evplp_ploc_tree is its host twin) */
} evplp_bvh_builder;

/* Creation-time configuration: what RtComPhoton::render fixes before setup()
 * (rtcomphoton.h:107-223) plus the build-only device / strip block. */
typedef struct evplp_config {
    int32_t abi_version;         /* EVPLP_ABI_VERSION */
    int32_t device;              /* HIP device ordinal */
    int32_t res_x, res_y;        /* main.cpp:108,114 */
    int32_t strip_rank;          /* row-strip partition; {0,1,H} = whole image */
    int32_t strip_count;
    int32_t strip_rows;          /* block height in rows, multiple of 8 */
    uint32_t num_light_paths;    /* rtcomphoton.h:114 */
    uint32_t num_vpl_light_paths;/* rtcomphoton.h:115 */
    uint32_t photons_per_path;   /* numMaxBounces + 1, rtcomphoton.h:116-117 */
    int32_t bvh_builder;         /* evplp_bvh_builder */
    int32_t deterministic;       /* 1: photon bins are accumulated in record order (bitwise reproducible) */
    int32_t gather_splits_per_wave; /* VPL gather work-item size: consecutive VPL splits (of 128) one wavefront sums; a power of two
                                  * 1..32, 0 = the library's default.  Results do not depend on it (fixed summation tree). */
    int32_t overlap_light_tracing;  /* 1: evplp_trace_light_paths runs on a second HIP stream of the context, ordered only behind the last
                                  * pass that READ the record buffer (gathers, photon splat) and in front of everything enqueued on the
                                  * context's stream after it -- so a preceding evplp_primary overlaps with it (light paths are
                                  * latency-bound, 4.6 waves per SIMD).  Off by default: a caller with kernels of its own on the
                                  * context's stream that read the records between the last such pass and the next light tracing
                                  * needs them ordered.  The technique loops of evplp_render_json and bench.py switch it on.
                                  * What else it does, and what a caller has to know:
                                  *  - the library DOUBLE-BUFFERS what the pipelined passes write: EVPLP_BUF_RECORDS (when a call traces
                                  *    the whole path set), the four G-buffer planes and the tile boxes.  A call that writes one of them
                                  *    flips EVPLP_BUF_* to the copy nobody reads, so the device address behind an EVPLP_BUF_* id CHANGES
                                  *    between calls (evplp_download / evplp_upload always see the current one);
                                  *  - the second copies are allocated on first use: + num_light_paths x photons_per_path x 96 bytes of
                                  *    records (192 MB at config #3, 115 MB at #4) and + 4 x W x rows x 16 bytes of G-buffer;
                                  *  - taking a device pointer with evplp_buffer_info, or binding memory with evplp_bind_buffer, pins
                                  *    that buffer for good: it is never flipped again (the pointer stays valid) and the passes that
                                  *    write it wait for its readers as they do without this flag;
                                  *  - up to two photon splats may be waiting for the verdict on their bin sizes; with `deterministic`
                                  *    set none is ever left pending behind a younger one (bitwise reproducible accumulation). */
    /* Upper bounds of the two large scratch buffers of the gathers, in bytes; 0 = the library's default.  Both are allocated on the first
     * gather that needs them, grow to what the configuration asks for within the bound, and live until evplp_destroy.
     *  cut_scratch_bytes: the entry cuts of the VPL / VSL gathers, 256 bytes per (group of 2 x 2 tiles, VPL record slot).  Default 8 GB.
     *    A configuration that needs more is gathered in bands of tile rows (same results, every band's launches have a tail of their own:
     *    config #5 in nine bands and five launches instead of one and one: 1 174 against 1 167 ms per iteration, 0.7 %); a bound too small for one row of tile blocks, or an allocation that fails,
     *    makes the walks start at the root (same results, ~40 % slower).
     *  vsl_mask_bytes: the lit-lane masks between the two kernels of the VSL gather (8 bytes per (tile, VSL slot) of a launch).
     *    Default 2 GB; smaller bounds mean more launches.
     * What one context allocates on one GPU (whole image; a rank of an n-way group: ~1/n of the per-pixel rows, x 1.5 with the deal's capacity):
     *                                  config #2 (ir)   #3 (evplp)        #4 (ppm)        #5 (vsl)
     *   G-buffer, accumulators, RGB     0.16 GB          0.16 GB           0.30 GB         0.62 GB      (9 planes x 16 B + 12 B per pixel)
     *   records (x 2 when overlapped)   0.4 MB           192 (384) MB      115 (230) MB    115 (230) MB
     *   gather partial sums             1.07 GB          1.07 GB           -               8.6 GB       (64 / 128 groups x 16 B per pixel)
     *   entry cuts (bounded, above)     4.3 GB           4.3 GB            -               8 GB of 68   (in nine bands)
     *   VSL masks (bounded, above)      -                -                 -               2 GB of 8.6  (in five launches)
     *   photon bins + compact photons   -                0.5 GB            0.4 GB          0.5 GB
     *   scene (331 k triangles)         0.1 GB everywhere (nodes, leaf blocks in two layouts, attributes; textures on top)
     *   error reference (if set)        12 B + 1 B (mask) per pixel of the WHOLE image on every context (evplp_set_error_reference)
     *   noise tracking (if on)          56 B per pixel of the context's planes (+ 1 B per image pixel with a mask; evplp_noise_track)
     *   adaptive gather (if enabled)    16 B per pixel of the context's planes (snapshot) + 16 B per 8 x 8 tile (evplp_adaptive_enable; the same for
     *                                   adaptive path tracing, evplp_adaptive_enable_pt: one mode at a time, one allocation)
     *   batched path tracing            64 B per pixel-sample of one chunk: min(items, bound / 4096) slots of 4 KB, allocated on the first
     *   (after a call)                  evplp_path_trace_batch, bounded by evplp_path_trace_batch_scratch (default 1 GB: 1024^2 at S = 16 in one chunk);
     *                                   items = the (tile, sample) pairs of the call: tiles x S with adaptivity off, active tiles x S in
     *                                   path-trace adaptive mode, sum(s_t) in budget mode (evplp_adaptive_enable_pt(ctx, 2));
     *                                   + 4 B per tile and 4 B per item of the largest call (the item table);
     *                                   budget mode: + 8 B per tile after evplp_adaptive_tile_noise
     *   refit (after a call)            28 B per node + 36 B per triangle (+ 4 B per light triangle), and the same staging bytes in pinned host memory (evplp_refit_accel)
     *   rest pose (after a call)        36 B per triangle of the scene + 64 B per mesh, and 64 B per mesh in pinned host memory, made by the first
     *                                   evplp_transform_mesh of a scene and freed with it; a context that never transforms allocates none of it
     *                                   (evplp_pose_mesh counts as a transform here: the first of either makes it)
     *   skins (after a call)            72 B per triangle of the skinned meshes (per corner four 16-bit bone indices and four float weights) + 48 B
     *                                   per bone of their skins + 32 B per mesh, and the last two again in pinned host memory, made by the first
     *                                   refit behind an evplp_pose_mesh and freed with the scene; on the host 32 B per skinned vertex, and 72 B per
     *                                   triangle of the meshes whose corner skin the last posed refit sent; a context that never poses allocates none
     *   morph targets (after a call)    36 B x T per triangle of the meshes with T targets (per corner and target one float3 delta, target-major per
     *                                   mesh) + 4 B per target of their weight sets + 32 B per mesh, the last two again in pinned host memory, and,
     *                                   once a mesh under weights is also moved by a matrix or a pose, 36 B per triangle of the scene (the base
     *                                   array: a copy of the rest pose in which such a mesh's part is its morphed base), made by the first refit
     *                                   behind an evplp_morph_mesh and freed with the scene; the rest-pose row above as well (evplp_morph_mesh
     *                                   counts as a transform there); on the host 12 B x T per vertex with targets, 12 B per vertex under weights,
     *                                   and 36 B x T per triangle of the meshes whose corner deltas the last morphed refit sent; a context that
     *                                   never morphs allocates none
 *   PLOC build (during the call)    88 B per triangle on top of the device LBVH's scratch, freed before evplp_build_accel returns: 2 n clusters in ping-pong (28 B
 *                                   each), n nearest neighbours (4 B), n packed flags and their scan (16 B), children and counts of the inner nodes (12 B)
 *   tree cost (after a call)        24 B per 256 nodes + 8 B, and the same in pinned host memory; the refit's plan and staging (the row above) if no
 *                                   refit of this tree has made them yet: refit_prepare makes them (evplp_accel_quality, evplp_set_refit_policy)
 *   tree rotations (after a call)   12 B per node (the plan's level, the rotations taken below the node, its four-wide stack need) + 64 B, and 64 B in
 *                                   pinned host memory, made by the first evplp_optimize_accel or the first refit with evplp_set_refit_rotations > 0
 *                                   and freed with the scene; the refit's plan and staging too if no refit has made them; a context that never asks
 *                                   for rotations allocates and launches none of it
     *   denoiser (after a call)         124 B per pixel of the context's planes (evplp_denoise); a group's rank: 92 B per pixel of its planes
     *                                   + n x 80 B per pixel of the exchanged rows, and rank 0 + 112 B per image pixel (evplp_group_denoise)
     *   temporal accumulation (if on)   36 B per triangle + 32 B per pixel of the context's planes (evplp_temporal_enable), and on the context that
     *                                   filters 96 B per pixel of its frame after its first evplp_denoise_temporal; a group's rank under strips:
     *                                   + n x 32 B per pixel of the exchanged rows, and rank 0 + 32 B per image pixel (evplp_group_denoise_temporal)
     *   surface gather (after a call)   256 KB of partial sums per slice of 256 VPL slots, and with EVPLP_SURFACE_PHOTONS 96 B per photon
     *                                   slot + 4 B per bucket (at most the slots rounded up to a power of two) + the radix sort's workspace: the grid
     *                                   of one call, 200 MB at 2 M slots; the host form 108 B per point of a chunk of 16 384 on the device and pinned
     *                                   (evplp_gather_surface); none of it depends on the number of points.  The progressive calls: the same,
     *                                   + 512 KB (the reduced VPL half of a chunk) and their host forms 156 B per point of a chunk, device and pinned;
     *                                   evplp_gather_surface_knn: the grid, that staging, and 4 B per point of the batch (_device) or of a chunk
     * A caller that has the device to itself sets cut_scratch_bytes = 72 GB, vsl_mask_bytes = 14 GB for config #5 (one band, one launch). */
    uint64_t cut_scratch_bytes;
    uint64_t vsl_mask_bytes;
    /* Row strips (strip_count > 1): rows of strip storage, a multiple of strip_rows; 0 = the equal share, ceil(blocks / strip_count) blocks.
     * More than that leaves room for a deal by cost (evplp_set_blocks), which gives a rank of cheap blocks more of them. */
    int32_t strip_capacity_rows;
} evplp_config;

/* rt/rtcommon.h:278-308 RtMaterial: three RGBA32F textures (a constant is a 1x1 texture,
 * rtcommon.h:80-90) + mLightIntensity.  tex_* = id from evplp_add_texture or -1 for the constant. */
typedef struct evplp_material {
    float kd[3]; float ks[3]; float ns;
    int32_t tex_kd, tex_ks, tex_ns;
} evplp_material;

/* rt/rtcommon.h:546-598 RtStableCamera ("direction" of the JSON is a look-at point) */
typedef struct evplp_camera {
    float origin[3]; float lookat[3]; float up[3];
    float fovy;     /* radians; fovx is converted by the caller as rtcommon.h:559 */
    float aspect;
} evplp_camera;

/* The OptiX variables / GL uniforms RtComPhoton::run() sets per iteration
 * (rtcomphoton.h:895-930, 819-823, 1043-1061): the de-facto device ABI of the reference. */
typedef struct evplp_frame_params {
    float camera_pos[3];         /* cameraPosition / uCameraPosition */
    uint32_t mis_mode;           /* misMode / uMisMode */
    float pdf_mc;                /* pdfMc / uPdfMc */
    float clamping_value;        /* clampingValue / uClampingValue */
    float photon_radius;         /* radius / uPhotonRadius */
    float vsl_radius;            /* vslRadius */
    float vsl_inv_pi_radius2;    /* vslInvPiRadius2 */
    uint32_t num_light_paths;    /* numLightPaths (1/N = uInvNumLightPaths) */
    uint32_t num_vpl_light_paths;/* numVplLightPaths */
    uint32_t photons_per_path;   /* numPhotonsPerLightPath */
    uint32_t do_accumulate;      /* doAccumulate */
    uint32_t rng_seed;           /* rngSeed = numIterations + rngOffset (rtcomphoton.h:965) */
    float jitter[2];             /* NDC translation of the jitter matrix (rtcomphoton.h:949) */
    uint32_t splat_footprint;    /* evplp_splat_footprint: which pixels a photon reaches (evplp_splat_photons only) */
    uint32_t reserved;
} evplp_frame_params;

/* The footprint of a photon in evplp_splat_photons.
 *  EVPLP_FOOTPRINT_IDEAL: pixel p receives photon i once iff |X_p - P_i|^2 <= r^2 (the radius test of photonsplatinstanced.frag:152-154
 *    alone).
 *  EVPLP_FOOTPRINT_PROXY: the reference's coverage rule.  It draws an instanced proxy mesh (sphere/icosphere.obj, rtcomphoton.h:677,
 *    632-644) scaled by the radius around every photon (photonsplatinstanced.vert:28-33), un-culled (glEnable(GL_CULL_FACE) is commented
 *    out, rtcomphoton.h:653-655), depth-tested LEQUAL against the deferred pass without depth writes (:789-837), and runs the fragment
 *    shader once per rasterised FACE fragment (.geom:16-32, .frag:146-240): a pixel inside the radius receives the photon once per
 *    face of the scaled proxy that its eye ray crosses between the near plane and the visible surface -- 0, 1 or 2 times for a convex
 *    mesh.  The mesh is the one given to evplp_set_splat_proxy, or the generated 42-vertex / 80-face icosphere
 *    (evplp_default_splat_proxy) if none was given. */
typedef enum evplp_splat_footprint { EVPLP_FOOTPRINT_IDEAL = 0, EVPLP_FOOTPRINT_PROXY = 1 } evplp_splat_footprint;

/* Device buffers a caller may read back, bind to external memory, or hand to a collective. */
typedef enum evplp_buffer {
    EVPLP_BUF_RECORDS = 0,   /* evplp_record[num_light_paths * photons_per_path]  ("photons", rtcomphoton.h:910) */
    EVPLP_BUF_GBUF_POSITION, /* float4[local_rows * W]  deferredPositionTexture */
    EVPLP_BUF_GBUF_NORMAL,   /* float4[...]             deferredNormalTexture */
    EVPLP_BUF_GBUF_DIFFUSE,  /* float4[...]             deferredDiffuseTexture */
    EVPLP_BUF_GBUF_PHONG,    /* float4[...]             deferredPhongReflectanceTexture (rgb, exponent) */
    EVPLP_BUF_LIGHT,         /* float4[...]             mLightTexture */
    EVPLP_BUF_VPL_ACCUM,     /* float4[...]             outputBuffer (rtcomphoton.h:897) */
    EVPLP_BUF_PHOTON_ACCUM,  /* float4[...] (rgb used)  mPhotonSplatTexture */
    EVPLP_BUF_COUNT
} evplp_buffer;

/* Per-pass statistics of the last call (hipEvent timing on the context stream). */
typedef struct evplp_pass_stats {
    float ms;                /* device time of the pass */
    uint64_t pairs;          /* gather: (pixel, usable record) pairs; splat: (photon, covered pixel) pairs */
    uint64_t rays;           /* rays traced by the pass; photon splat with EVPLP_FOOTPRINT_PROXY: fragments of the proxy mesh (0, 1 or 2 per pair) */
    uint64_t usable;         /* usable VPL / photon records consumed */
    float dominant_kernel_ms;/* device time of the pass's dominant kernel alone (summed over its launches) */
    uint32_t reserved[3];    /* [0], [1]: a 64-bit count -- VSL gather: sample-iterations of the estimators; diagnostic builds: node visits; splat: bin entries, fullest bin */
    uint64_t shaded;         /* gather: pairs that passed the cosine test AND the visibility test (contributions evaluated);
                              * photon splat: (photon, pixel) pairs of ALL splat passes of the context so far (running total) */
    uint32_t launches;       /* launches of the dominant kernel in the pass */
    uint32_t pad;
} evplp_pass_stats;

typedef enum evplp_pass {
    EVPLP_PASS_PRIMARY = 0, EVPLP_PASS_LIGHT_TRACE, EVPLP_PASS_GATHER_VPL, EVPLP_PASS_GATHER_VSL,
    EVPLP_PASS_SPLAT, EVPLP_PASS_RESOLVE, EVPLP_PASS_PATH_TRACE, EVPLP_PASS_GATHER_LVC, EVPLP_PASS_COUNT
} evplp_pass;

typedef struct evplp_context evplp_context;

/* ---- lifetime.  Replaces RtComPhoton::setup()/destroy() (rtcomphoton.h:646-708, 1135-1138). ---- */
int evplp_create(const evplp_config *cfg, evplp_context **out);
void evplp_destroy(evplp_context *ctx);
const char *evplp_last_error(const evplp_context *ctx); /* ctx may be NULL: error of a failed create */
int evplp_abi_version(void);
/* Launch on a caller-owned hipStream_t (e.g. torch's current stream); NULL = context's own stream. */
int evplp_set_stream(evplp_context *ctx, void *hip_stream);
int evplp_synchronize(evplp_context *ctx);

/* ---- scene upload.  Replaces the createOptix.. / createOpengl.. uploads of RtMesh, RtMaterial and RtTexture
 * (rt/rtcommon.h:196-245, 357-429) and RtScene::addObject/addAreaLight's results (:644-798).
 * Host pointers; the library copies.  Call order: textures, materials, meshes, area light,
 * camera, then evplp_build_accel. ---- */
int evplp_add_texture(evplp_context *ctx, int32_t w, int32_t h, const float *rgba); /* returns id >= 0 */
int evplp_add_material(evplp_context *ctx, const evplp_material *m);                /* returns index >= 0 */
/* RtMesh SoA (rtcommon.h:460-467): vertices float3[nverts], texcoords float2[nverts] (NULL = zeros,
 * rtcommon.h:701-705), triangle indices int3[ntris], one material.  Returns mesh index >= 0. */
int evplp_add_mesh(evplp_context *ctx, const float *vertices, const float *texcoords, int32_t nverts,
                   const int32_t *indices, int32_t ntris, int32_t material);
/* RtScene::addAreaLight (rtcommon.h:772-798): mesh becomes the single emitter, its material is
 * replaced by the black emitter material; intensity = JSON [r,g,b,w] (xyz scaled by pi inside). */
int evplp_set_arealight(evplp_context *ctx, int32_t mesh, const float intensity[4]);
int evplp_set_camera(evplp_context *ctx, const evplp_camera *cam);
/* LoadScene (main.cpp:42-85) in one call: read the scene JSON (resX/resY, scene[], arealight, camera |
 * stablecamera), its OBJ/MTL files, upload everything and build the acceleration structure. */
int evplp_load_scene_json(evplp_context *ctx, const char *json_path);
int evplp_get_camera(evplp_context *ctx, evplp_camera *out);
/* OptiX "Trbvh" acceleration (rtcomphoton.h:705-707) + area-light CDF (rtcommon.h:501-531). */
int evplp_build_accel(evplp_context *ctx);
/* RtScene::findBoundingSphereRadius (rtcommon.h:805-814), totalArea (:759-768), light area (:529) */
int evplp_scene_metrics(evplp_context *ctx, float *bounding_sphere_radius, float *total_area, float *light_area);

/* ---- scenes that move: new vertex positions for a mesh, then a refit of the tree on the device (INTEGRATION B7) ----
 * evplp_update_mesh replaces the positions of mesh `mesh` (host pointer, float3[nverts], copied before the call returns); topology, texture
 * coordinates and material stay, so nverts must be the mesh's vertex count.  It touches the host copy only and marks the mesh dirty; several
 * calls may precede one refit.  EVPLP_ERR_INVALID, the context staying usable: no evplp_build_accel yet, mesh out of range, another vertex
 * count, a null pointer, a coordinate that is not finite.
 * While any mesh is dirty EVERY pass is refused (primary, light tracing, the gathers, the splat, both path tracers, the denoiser) with a
 * message that names the two ways out: a stale tree under new vertices never renders.
 *   evplp_refit_accel keeps the tree's topology and leaf assignment and recomputes, on the device and on the context's stream (behind every
 *     pass already enqueued, the light tracing of overlap_light_tracing included; no host wait in the steady state unless a refit policy is set, below): the dirty triangles'
 *     vertices, every leaf's triangle operands, all boxes bottom-up (one launch per height of the tree, padded once from the exact union
 *     with the builders' pad for the new scene bounds) and the four-wide nodes; and on the host the light's CDF and area, the light bounds,
 *     total_area and bounding_radius, by the code evplp_build_accel uses.  Visibility and closest hit are exact predicates over the
 *     triangles, so a frame over the refitted tree equals the frame of a fresh build bit for bit; what ages is the tree's quality -- after
 *     large motions the walks visit more nodes, and evplp_build_accel is the remedy (evplp_accel_quality measures it, evplp_set_refit_policy
 *     lets the refit act on it).  Nothing dirty: returns EVPLP_OK and launches nothing.
 *     The first refit of a tree makes its plan (evplp_refit_levels) and allocates 28 B per node + 36 B per triangle on the device.
 *   evplp_build_accel on a dirty context is the full rebuild from the updated meshes and clears the dirty state too.
 * Degenerate triangles (meshBound's rule: area not > 0 or not finite): one that BECOMES degenerate gets all-zero operands and adds nothing
 * to a box -- what a fresh build does by dropping it.  One that was dropped at build time and has an area now has no leaf to go to:
 * evplp_refit_accel returns EVPLP_ERR_INVALID, the context stays dirty, and evplp_build_accel is the way out.
 * A refit leaves the accumulators, the noise moments and the adaptive records alone: a caller who moves geometry under an accumulation
 * clears them (evplp_clear_accumulators) as after a camera change. */
int evplp_update_mesh(evplp_context *ctx, int32_t mesh, const float *vertices, int32_t nverts);
int evplp_refit_accel(evplp_context *ctx);
/* ---- moving a mesh by a matrix: nothing is uploaded but twelve floats (INTEGRATION B7) ----
 * m is a row-major 3 x 4 matrix.  A point p = (x, y, z) goes to out[r] = ((m[4r] x + m[4r+1] y) + m[4r+2] z) + m[4r+3]: fp32, every product and
 * every sum rounded on its own, in this order, nothing fused (transform_point in evplp_types.h, the one function the host and the device
 * call).  There is no special case for the identity: under it a coordinate of -0.0 becomes +0.0, everything else keeps its bits.
 * Rest pose: the positions a mesh had at evplp_add_mesh, or the ones the last evplp_update_mesh gave it.  evplp_transform_mesh sets the
 * mesh's current positions to transform_point(m, rest pose).  Transforms do NOT compose: a second call replaces the first, and the rest
 * pose's own bits are never overwritten, so a hundred frames of rotation do not drift.  evplp_update_mesh sets a new rest pose and forgets
 * the matrix.
 * The call marks the mesh dirty exactly as evplp_update_mesh does: every pass is refused until evplp_refit_accel or evplp_build_accel, and
 * several calls of either kind, on the same or on different meshes, may precede one refit.  The host copy of the mesh follows through the
 * same function, so the full rebuild on a dirty context, a policy's rebuild, the refit's degenerate-triangle refusal and the scene's figures
 * see the positions the device has.
 * EVPLP_ERR_INVALID, nothing marked, the context staying usable: no evplp_build_accel yet, mesh out of range, a null matrix, a matrix entry
 * that is not finite, a transformed coordinate that is not finite (checked on the host copy: refused here, never rendered).  A singular
 * matrix is legal: its triangles lose their area and fall under the degenerate rule above, and one that was dropped at build time and is
 * given an area is refused by the refit as above.
 * On the device the refit treats a mesh that is dirty by transform differently from one that is dirty by upload: its triangles are neither
 * staged nor copied (the host flattens a dirty mesh once, for the scene's figures).  The device keeps the rest pose (nine floats per triangle; a mesh's part is made at its first transform,
 * from the attributes it already holds if the mesh is clean and has no matrix, from the host's rest pose otherwise, and again after
 * evplp_update_mesh gave it a new one; after any evplp_build_accel or policy rebuild it is made again from the host's rest pose).  The
 * dirty meshes go up as a table of (first triangle, count, matrix) through pinned memory on the stream, and ONE launch per refit writes
 * the attributes of all of them; meshes dirty by upload keep the staging copy and the scatter, in the same refit.  The steady state still
 * has no host wait.
 * evplp_transform_points applies the same function to n points (host only, no GPU; in and out: float3[n], may be the same array):
 * the positions evplp_transform_mesh will use, bit for bit.  EVPLP_ERR_INVALID for a null pointer or n < 0. */
int evplp_transform_mesh(evplp_context *ctx, int32_t mesh, const float m[12]);
int evplp_transform_points(const float m[12], const float *in, float *out, int32_t n);
/* ---- moving a mesh by bones: linear-blend skinning of the rest pose on the device; 48 B per bone go up (INTEGRATION B7) ----
 * A skin gives every vertex four bone indices b[4] and four weights w[4]; a pose is a palette bones[nbones][12] of row-major 3 x 4 matrices.
 * A point p goes to
 *   q_k = transform_point(bones + 12 b[k], p) for k = 0 .. 3,   out[r] = ((w[0] q_0[r] + w[1] q_1[r]) + w[2] q_2[r]) + w[3] q_3[r]
 * in fp32, every product and every sum rounded on its own, in this order, nothing fused (skin_point in evplp_types.h, the one function the
 * host and the device call).  All four influences are always evaluated -- no special case for a zero weight, a repeated bone or the
 * identity -- and nothing is renormalised: the weights are used as given.  With weights (1, 0, 0, 0) and finite matrices the result is
 * transform_point of bone b[0] value for value (the sign of a zero may differ).
 * evplp_set_mesh_skin attaches a skin to mesh `mesh` (host pointers, int32[nverts][4] and float[nverts][4] in the vertex numbering of
 * evplp_update_mesh, copied before the call returns).  A skin is constant for the topology: the call moves nothing and marks nothing dirty,
 * and the skin survives evplp_update_mesh (a new rest pose under the same skin), evplp_build_accel and a policy's rebuild.  nbones = 0
 * removes the skin (the arrays are not looked at).  EVPLP_ERR_INVALID, nothing changed, the context staying usable: no evplp_build_accel yet,
 * mesh out of range, a vertex count other than the mesh's, a null pointer, nbones outside 0 .. 1024, an index outside [0, nbones) (also
 * where its weight is 0), a weight that is not finite or is negative, a vertex whose four weights, added in double, differ from 1 by more
 * than 1e-3 (the bound only keeps a wrong array out).  A new skin for a mesh whose pose no refit has taken yet leaves the posed positions
 * in place: that mesh goes up by upload.
 * evplp_pose_mesh sets the mesh's current positions to skin_point(rest pose) under the palette.  The rest pose is evplp_transform_mesh's:
 * what evplp_add_mesh or the last evplp_update_mesh gave, never overwritten, so poses do NOT compose and do not drift.  A pose replaces a
 * matrix of evplp_transform_mesh and a matrix replaces a pose; evplp_update_mesh forgets both and keeps the skin.  The mesh is dirty exactly
 * as after evplp_update_mesh (every pass is refused until the refit), and the host copy follows through the same function, so bounds, areas,
 * the light's CDF, evplp_scene_metrics, a rebuild and the refit's degenerate-triangle refusal see the positions the device has.
 * EVPLP_ERR_INVALID, nothing marked: not built, mesh out of range, the mesh has no skin, nbones is not the skin's, a null pointer, a matrix
 * entry that is not finite, a posed coordinate that is not finite (checked on the host copy).  A palette that collapses triangles is legal:
 * they fall under the degenerate rule above.
 * On the device the skin is expanded per triangle corner, because the attributes and the rest pose are per triangle: four 16-bit indices and
 * four floats, 24 B per corner, the skinned meshes one behind the other; a mesh's part is made by its first posed refit (and again after a
 * rebuild or a change of the set of skinned meshes).  A refit uploads nbones x 48 B per posed mesh and a table of (first triangle, count,
 * palette, corner skin) through pinned memory, and ONE launch writes the attributes of all posed meshes from the shared rest-pose array,
 * which it never writes; uploaded, transformed and posed meshes may share one refit, and the steady state still has no host wait (the
 * refit that sends a mesh's corner skin copies it from pageable memory and may wait for that copy).
 * evplp_skin_points applies the same function to n points (host only, no GPU; bone_index / weight: [n][4]; in and out: float3[n], may be the
 * same array): the positions evplp_pose_mesh will use, bit for bit.  It has the refusals above that apply to its arguments (here nbones is
 * 1 .. 1024, n >= 0), and a refused call writes nothing to out. */
int evplp_set_mesh_skin(evplp_context *ctx, int32_t mesh, int32_t nbones, const int32_t *bone_index /* [nverts][4] */,
                        const float *weight /* [nverts][4] */, int32_t nverts);
int evplp_pose_mesh(evplp_context *ctx, int32_t mesh, const float *bone_matrices /* [nbones][12] */, int32_t nbones);
int evplp_skin_points(const float *bone_matrices, int32_t nbones, const int32_t *bone_index, const float *weight,
                      const float *in, float *out, int32_t n);
/* ---- moving a mesh by morph targets (blend shapes): rest pose + the weighted deltas, blended on the device; 4 B per target go up (DESIGN
 * section 6b, INTEGRATION B7) ----
 * A set of T targets gives every vertex T offsets d_k (deltas[T][nverts][3]); a weight set is w[T].  A point p goes to
 *   out[r] = (((p[r] + w[0] d_0[r]) + w[1] d_1[r]) + ... ) + w[T-1] d_{T-1}[r]
 * in fp32, every product and every sum rounded on its own, in index order, nothing fused (morph_point in evplp_types.h, the one function the
 * host and the device call).  All targets are always evaluated -- no shortcut for a zero weight, so -0.0 may become +0.0 and every other bit
 * is kept -- and the weights are used as given: any finite value, so negative weights and extrapolation beyond 1 are legal.
 * evplp_set_mesh_morph attaches targets to mesh `mesh` (a host pointer, float[ntargets][nverts][3] in the vertex numbering of
 * evplp_update_mesh, copied before the call returns).  ntargets is 1 .. 64; ntargets = 0 removes the targets (the array is not looked at).
 * Targets are constant for the topology: the call moves nothing and marks nothing dirty, and they survive evplp_update_mesh (the deltas
 * are relative to whatever the rest pose is), evplp_build_accel and a policy's rebuild.  EVPLP_ERR_INVALID, nothing changed, the context
 * staying usable: no evplp_build_accel yet, mesh out of range, a vertex count other than the mesh's, a null pointer, ntargets outside
 * 0 .. 64, a delta that is not finite, morph weights in force on that mesh (take them away first).
 * evplp_morph_mesh puts weights in force: the mesh's BASE becomes morph_point(rest pose), and its positions become that base under whatever
 * moves the mesh -- nothing, the matrix of evplp_transform_mesh (transform_point of the base) or the palette of evplp_pose_mesh (skin_point
 * of the base): morphed first, then moved.  The rest pose is never overwritten, so weights do NOT compose and do not drift: each call
 * replaces the weights before it.  The weights are a state of their own beside matrix and pose: a matrix still replaces a pose and a pose a
 * matrix, neither touches the weights, and a later evplp_transform_mesh / evplp_pose_mesh acts on the morphed base; evplp_update_mesh
 * forgets the weights (as it forgets matrix and pose) and keeps the targets.  evplp_morph_mesh(ctx, mesh, NULL, 0) takes the weights away:
 * the positions are the un-morphed ones again, and the mesh is dirty if weights were in force (not otherwise).  The mesh is dirty exactly as
 * after evplp_update_mesh (every pass is refused until the refit), and the host copy follows through the same functions, so bounds, areas,
 * the light's CDF, evplp_scene_metrics, a rebuild and the refit's degenerate-triangle refusal see the positions the device has.
 * EVPLP_ERR_INVALID, nothing marked: not built, mesh out of range, the mesh has no targets, ntargets is not the targets' count, a null
 * pointer with a count > 0, a weight that is not finite, a final coordinate that is not finite (the base, or the base under the matrix or
 * the pose in force, checked on the host copy).  Weights that collapse triangles are legal: they fall under the degenerate rule above.
 * On the device the deltas are expanded per triangle corner, because the attributes and the rest pose are per triangle: 12 B per corner and
 * target, per mesh target-major [T][3 x triangles], the meshes with targets one behind the other; a mesh's part is made by its first morphed
 * refit (and again after a rebuild or a change of the set of meshes with targets).  A refit uploads 4 B x T per morphed mesh and a table of
 * (first triangle, count, weights, deltas, T, destination) through pinned memory, and ONE launch, in front of the transform and the skin
 * launch, writes every mesh whose base must be written: straight into the attributes where no matrix and no pose is in force, else into the
 * base array, which the two launches then read in place of the rest pose.  A mesh whose weights did not change since its base was written
 * (only its matrix or its pose did) is not morphed again.
 * evplp_morph_points applies the same function to n points (host only, no GPU; deltas: [ntargets][n][3]; in and out: float3[n], may be the
 * same array): the base evplp_morph_mesh will use, bit for bit.  It has the refusals above that apply to its arguments (ntargets 1 .. 64,
 * n >= 0, null pointers, a point, a delta, a weight or a result that is not finite), and a refused call writes nothing to out.
 * evplp_mesh_vertices(ctx, mesh, 2, ...) returns the morphed base of a mesh with targets (its rest pose while no weights are in force); a
 * mesh without targets has no morphed base, and which = 2 stays EVPLP_ERR_INVALID for it. */
#define EVPLP_MAX_MORPH_TARGETS 64
int evplp_set_mesh_morph(evplp_context *ctx, int32_t mesh, int32_t ntargets, const float *deltas /* [ntargets][nverts][3] */, int32_t nverts);
int evplp_morph_mesh(evplp_context *ctx, int32_t mesh, const float *weights /* [ntargets] */, int32_t ntargets);
int evplp_morph_points(const float *in, const float *deltas, const float *weights, int32_t ntargets, int32_t n, float *out);
/* The meshes as the host copy holds them, in the numbering evplp_update_mesh and evplp_set_mesh_skin expect -- what a caller of
 * evplp_load_scene_json needs to build a skin (the OBJ reader de-duplicates (v, vt) pairs per material group).  evplp_mesh_count: the number
 * of meshes (negative: an error code).  evplp_mesh_info: each pointer may be null.  evplp_mesh_vertices: float3[nverts] into out_xyz, which
 * holds capacity_verts vertices; which = 0 the current positions, 1 the rest pose (the same until a matrix or a pose moves the mesh), 2 the
 * base a matrix or a pose acts on (the rest pose morphed by the weights in force; the rest pose without weights; only for a mesh with morph targets).
 * EVPLP_ERR_INVALID: mesh out of range, another `which`, which = 2 for a mesh without morph targets, a null destination, too small a capacity. */
int evplp_mesh_count(evplp_context *ctx);
int evplp_mesh_info(evplp_context *ctx, int32_t mesh, int32_t *nverts, int32_t *ntris, int32_t *material);
int evplp_mesh_vertices(evplp_context *ctx, int32_t mesh, int32_t which /* 0 current, 1 rest pose, 2 morphed base */, float *out_xyz, int32_t capacity_verts);
/* refits since evplp_create, heights of the current tree's plan (0 before its first refit), HIP-event time of the last refit (0 while
 * evplp_profile_passes is off; waits for that refit).  Each pointer may be null. */
int evplp_refit_info(evplp_context *ctx, int32_t *refits, int32_t *levels, float *last_refit_ms);
/* The plan of a refit (host only, no GPU, deterministic): nodes64 = nnodes flattened nodes of 64 B, the child references two int32 at byte
 * 48 and 52 (>= 0: a node index; < 0: a leaf or an absent child); node 0 is the root.  height[i] (nnodes ints) = 0 for a node without inner
 * children, else 1 + the larger of its inner children's, -1 for a node the root does not reach; order (nnodes ints) = the reached nodes by
 * height, by index within a height; level_begin (level_capacity + 1 ints): height l is order[level_begin[l] .. level_begin[l + 1]).  No
 * storage order is assumed.  Returns the number of heights (>= 1), or EVPLP_ERR_INVALID -- always promptly -- for a child index >= nnodes, a
 * node reached twice (two parents, a cycle), more heights than level_capacity, null arrays, nnodes < 1. */
int evplp_refit_levels(const void *nodes64, int32_t nnodes, int32_t *height, int32_t *order, int32_t *level_begin, int32_t level_capacity);

/* ---- how good the tree still is: its SAH cost, measured on the device, and an opt-in rebuild policy (INTEGRATION B7) ----
 * The figure is the surface-area-heuristic cost of the flattened tree as it is on the device, from the boxes the walks test (the padded
 * centre / half-size child boxes of the 64-byte nodes).  Over every node the root reaches and each child slot s whose reference is not
 * absent: a = 8 (hx hy + hy hz + hz hx) in fp64 from the fp32 half-sizes; an inner child adds a to inner_area; a leaf of cnt triangles
 * (cnt = (~reference & 3) + 1) adds a * cnt to leaf_tri_area and a * ((cnt + 1) >> 1) to leaf_pair_area -- the packet walk tests a leaf two
 * triangles at a time.  A triangle that a refit zeroed as degenerate keeps its slot and still counts in its leaf's cnt, because the walk
 * still tests it; a box with a negative half-size (an absent child, a leaf whose triangles have ALL lost their area) holds nothing and
 * adds nothing.  root_area = the area of the union of the root's present child boxes, 2 (dx dy + dy dz + dz dx), 0 for the empty tree.
 *   cost = (15 (root_area + inner_area) + 40 leaf_pair_area) / root_area, 0 where root_area is 0
 * 15 and 40 are the vector instructions of a node visit and of a pair test of the packet walk; the three raw sums are reported so that a
 * caller can weigh them otherwise.  The frame never depends on the figure: it is the same whatever the tree.
 *   evplp_accel_cost is the host-only statement of that arithmetic (no GPU, deterministic): nodes64 as for evplp_refit_levels, whose order
 *     it takes and whose refusals it shares (not a tree: EVPLP_ERR_INVALID, promptly; any number of heights is accepted).  The terms are
 *     added in chunks of 256 entries of that order, within a chunk by halving strides over each run of 64 and then run by run, and the
 *     chunks in index order.  out = { cost, root_area, inner_area, leaf_pair_area, leaf_tri_area }.  Returns the number of reached nodes.
 *   evplp_accel_quality measures the same on the device: one 256-thread kernel over the refit's plan (a tree that has not been refitted
 *     gets its plan here, with the refit's allocations) plus 24 B per 256 nodes on the device and in pinned host memory, on the context's
 *     stream behind everything enqueued, and waits for it.  On the bytes evplp_debug_accel(ctx, 0, ...) returns, its five doubles equal
 *     evplp_accel_cost's bit for bit.  It changes no node, no plane and no counter.  EVPLP_ERR_INVALID before evplp_build_accel, and while
 *     vertices are dirty (as every pass: evplp_refit_accel or evplp_build_accel first).
 *     built_cost = the cost at the first measurement since the last evplp_build_accel, kept until the next one (0: not measured yet);
 *     reached_nodes, leaf_refs = the nodes and the leaf references the sums run over; refits_since_build = refits of this tree (counted
 *     with or without a policy); policy_rebuilds = rebuilds the policy has made since evplp_create; last_action = what the last
 *     evplp_refit_accel that had a policy and something to do did: 0 none, 1 refit kept, 2 rebuilt (evplp_build_accel resets it to 0).
 *   evplp_set_refit_policy(ctx, max_cost_ratio, rebuild_builder): max_cost_ratio = 0 switches the policy off, which is the default, and
 *     evplp_refit_accel is then exactly the call above.  With max_cost_ratio > 0 evplp_refit_accel, after its refit, measures the cost
 *     (one small launch and ONE HOST WAIT: the call is no longer free of host waits) and, when cost > max_cost_ratio * built_cost, runs
 *     the full rebuild -- the code of evplp_build_accel with rebuild_builder, an evplp_bvh_builder or -1 for the context's own --, measures
 *     the new built_cost and counts policy_rebuilds.  It returns EVPLP_OK either way; last_action says which.  A rebuild is what
 *     evplp_build_accel costs: 198 ms with the SAH builder, 13.9 ms with the device LBVH for 331 k triangles (profiles/refit_times.txt).
 *     Like a refit, a policy rebuild leaves accumulators, noise moments and adaptive records alone.  While a policy is set
 *     evplp_build_accel re-measures built_cost; setting one on a clean, built context without a built_cost measures it there and then.
 *     EVPLP_ERR_INVALID: a ratio that is negative or not finite, a builder outside -1 .. 3, vertices dirty.  No ratio is recommended
 *     here: DESIGN section 6b has what was measured.  rebuild_builder = EVPLP_BVH_PLOC_GPU (4) is refused too, for now; a context whose
 *     OWN builder is PLOC gets PLOC rebuilds from the policy through rebuild_builder = -1. */
struct evplp_accel_quality {            /* (the call below has the same name: C and C++ both need the word `struct` in front of the type) */
    double cost, root_area, inner_area, leaf_pair_area, leaf_tri_area;
    double built_cost;
    int32_t reached_nodes, leaf_refs;
    int32_t refits_since_build, policy_rebuilds;
    int32_t last_action, pad;
};
int evplp_accel_cost(const void *nodes64, int32_t nnodes, double out[5]);
int evplp_accel_quality(evplp_context *ctx, struct evplp_accel_quality *out);
int evplp_set_refit_policy(evplp_context *ctx, double max_cost_ratio, int32_t rebuild_builder);
/* ---- tree rotations inside the refit sweep: between "keep the aged topology" and "throw the tree away" (INTEGRATION B7) ----
 * Opt-in and off by default (Kensler 2008; Kopta et al. 2012).  A rotating sweep is the refit's sweep -- every node once, children before
 * parents, one launch per level of the refit's plan -- in which node N, besides its boxes, may swap one of its children with a grandchild
 * on the other side.  N's child slots are c[0], c[1]; the candidates (s, q) are visited in the order (0,0), (0,1), (1,0), (1,1): A = c[s]
 * moves down, B = c[1-s] must be an inner node, G = B.c[q] moves up, K = B.c[1-q] stays under B.  A candidate is admissible if none of A, G, K
 * is absent, none of their exact (unpadded) boxes is empty, and level(A) < level(B), where level is the node's level in the refit's PLAN
 * (evplp_refit_levels' height[] of the tree as it was when the plan was made; a leaf reference counts as -1), not its current height.
 * gain = area(box B) - area(box A u box K), area = ex ey + ey ez + ez ex in fp32 in that order, nothing fused; the largest gain > 0 is taken,
 * ties keep the first candidate.  Taken: N.c[s] = G, B.c[q] = A, B's box = A u K; the three touched child boxes are padded from the exact
 * boxes with the refit's pad.  Two 64-byte node records are rewritten; no node is allocated and no leaf moves.
 * The level condition keeps every parent on a strictly higher plan level than its children.  So the plan stays a valid schedule for this
 * pass, for further passes and for every later refit (nothing is planned again, nothing is downloaded; the levels are no tight heights any
 * more); two nodes of one launch are never parent and child, so the sweep needs no atomics and no fences; and no root-to-leaf path grows
 * longer than the plan has levels, so the depth, the walks' stacks and the plan's level count stay valid.
 * Visibility and closest hit are exact predicates over the triangles: a frame over a rotated tree equals a fresh build's bit for bit.
 *   evplp_optimize_accel(ctx, passes, rotations): passes = 1 .. 8 full sweeps (leaf boxes upward with rotations) and the four-wide nodes,
 *     on the context's stream behind everything enqueued, ONE host wait; *rotations (may be null) = the rotations taken in all passes.  The
 *     four-wide walk's stack bound (evplp_accel_stack_entries) is computed in the same sweep and becomes the rotated tree's.  It leaves
 *     accumulators, noise moments and adaptive records alone and sets evplp_accel_quality's last_action to 3.  EVPLP_ERR_INVALID, the
 *     context staying usable: before evplp_build_accel, while vertices are dirty (as every pass), passes outside 1 .. 8.
 *     evplp_accel_quality keeps summing in the plan's order, which after a rotation is no longer evplp_refit_levels' order of the rotated
 *     bytes: its sums then equal evplp_accel_cost's within the rounding of the additions (reached_nodes x 2^-52 of each sum), not bit
 *     for bit; the ranks of a group, which share the plan, still agree with each other bit for bit.
 *   evplp_set_refit_rotations(ctx, passes): 0 = off, the default -- evplp_refit_accel is then exactly the call above.  With passes = 1 .. 8
 *     the refit's own level launches are the rotating ones (the first pass IS the refit's sweep, further passes repeat it), and the refit
 *     has ONE HOST WAIT, for the root's counts: it is no longer free of host waits.  With a policy set as well it is the wait the cost
 *     measurement makes anyway, and the policy compares the cost AFTER the rotations.  last_action: 2 rebuilt, else 3 (kept, rotating
 *     sweeps ran); 1 only without rotations.  EVPLP_ERR_INVALID: passes outside 0 .. 8.
 *   evplp_rotation_info: rotations since the last evplp_build_accel (a policy rebuild included), rotations in the last call that swept
 *     (evplp_optimize_accel, or a refit with rotations on), the same per pass (8 ints, zeros behind the passes run), and the refit's
 *     setting.  Each pointer may be null.
 *   evplp_rotate_tree is the host-only statement of the sweep (no GPU, deterministic), with the functions the kernel calls: nodes64 as for
 *     evplp_refit_levels (the child references alone are read), tri_index = nslots ints (4 per leaf block: original triangle or -1), verts9 =
 *     9 floats per original triangle, level = the plan's level per node or null (null: evplp_refit_levels' heights of nodes64 as it is;
 *     given: every inner child must lie below its parent).  Out: children (2 nnodes ints, the new references), boxes (6 nnodes floats: lo,
 *     hi of the exact box under every reached node), rotations (passes ints, per pass), *need0 (the root's four-wide stack need:
 *     evplp_accel_stack_entries - 2).  Returns the plan's levels, or EVPLP_ERR_INVALID (not a tree, a null array, passes outside 1 .. 8,
 *     levels that are no schedule). */
int evplp_optimize_accel(evplp_context *ctx, int32_t passes, int32_t *rotations);
int evplp_set_refit_rotations(evplp_context *ctx, int32_t passes);
int evplp_rotation_info(evplp_context *ctx, int32_t *since_build, int32_t *last_call, int32_t per_pass[8], int32_t *refit_passes);
int evplp_rotate_tree(const void *nodes64, int32_t nnodes, const int32_t *tri_index, int32_t nslots, const float *verts9, int32_t ntri, const int32_t *level,
                      int32_t passes, int32_t *children, float *boxes, int32_t *rotations, int32_t *need0);
/* The tree EVPLP_BVH_PLOC_GPU builds, stated on the host (no GPU, deterministic): the device builder's steps run serially, with the same
 * Morton key, the same fp32 distance and the same tie rule, so the two produce one tree.  verts9 = 9 floats per triangle; triangles
 * without area (meshBound's rule) are left out.  radius = 1 .. 32 positions searched on either side, search_iterations = 0 .. 128 search
 * iterations before every further iteration pairs position 2k with 2k + 1 (0: pure pairing).  order (ntri ints; the first n are written) =
 * the valid triangles in Morton order, equal keys in triangle order: leaf ~p is order[p].  children (2 (ntri - 1) ints; 2 (n - 1) are
 * written) = the left and right child of inner node i at [2 i] and [2 i + 1], an inner index or ~p; node 0 is the root, and a child's
 * index is always above its parent's.  *iterations = the iterations run, at most search_iterations + ceil(log2 n).  Returns n, the valid
 * triangles, or EVPLP_ERR_INVALID for a null pointer, ntri < 0, a radius or search_iterations out of range. */
int evplp_ploc_tree(const float *verts9, int32_t ntri, int32_t radius, int32_t search_iterations, int32_t *order, int32_t *children, int32_t *iterations);

/* ---- ray queries: a caller's own rays against the scene's tree (INTEGRATION B8) ----
 * Replaces the second acceleration structure a host application would otherwise build over geometry the device already holds: picking,
 * dropping a probe onto a surface, a line of sight between two points of the moved scene, visibility baked for the caller's own points.
 * The rays walk the tree of evplp_build_accel as evplp_refit_accel last left it, with the per-lane walks light tracing uses.
 *   evplp_trace_closest: hits[i] is the closest hit of rays[i]: of the triangles the triangle test accepts with tmin < t < tmax the one
 *     with the smallest t, among equal t the lowest triangle index, whatever the builder.  What is guaranteed, with S = the larger of the
 *     scene's diagonal and its largest coordinate magnitude: a decidable ray -- one that misses every triangle, or that as an exact line
 *     crosses the bounding box of the triangle this rule names -- gets exactly the triangle test's answer; any reported hit is one the
 *     test accepts, with the test's own values; and this holds for origins within 1e4 S of the scene.  (A ray that grazes a triangle's
 *     edge so closely that only the test's rounding accepts it, outside that triangle's box, may report the next hit instead: DESIGN
 *     section 2.  Further out than 1e4 S the walk may miss triangles the test would accept.)  t, beta, gamma are the test's own values for
 *     that triangle (the hit point is (1 - beta - gamma) p0 + beta p1 + gamma p2); the direction is not normalised, so t is in units of
 *     it.  filter: 0 all triangles, 1 without the light mesh, 2 the light mesh only.  A miss: triangle = -1, t = tmax, beta = gamma = 0.
 *     triangle counts the scene's triangles in mesh order (the index of the attributes on the device); evplp_triangle_info turns it into
 *     the mesh and the triangle within that mesh, on the host.  A triangle without area is in no tree and is never reported.
 *   evplp_trace_occluded: out[i] = 1 iff any triangle is accepted in (tmin, tmax), else 0.
 *   An invalid ray -- an origin, a direction, a tmin or a tmax that is not finite, a direction whose largest component in magnitude lies
 *     outside [2^-64, 2^64] (a direction of three zeros among them), tmin > tmax -- is never walked: triangle = -2 with t = beta = gamma = 0,
 *     or out[i] = 2.  The kernel decides it, for the host and the device forms alike.  (Inside that range the length of the direction is
 *     free; beyond it the walk's reciprocals would bend the direction.)
 *   flags: EVPLP_QUERY_ORDER traces the rays of a launch in the order of a 32-bit key (the origin's Morton code in the scene's box, the
 *     direction's octant in the low bits; one key kernel and one radix sort per launch) and writes every result to its ray's own slot:
 *     the results do not depend on it.  What it gains and costs is in DESIGN section 6c.
 *   The host forms copy the rays through pinned memory, launch, copy the results back and wait.  The _device forms take device pointers
 *     (n evplp_ray; n evplp_hit or n bytes), enqueue on the context's stream and do not wait: evplp_synchronize, or work on that stream,
 *     comes behind them.  Both run a batch as launches of at most EVPLP_QUERY_CHUNK_RAYS rays, so what a context allocates does not depend
 *     on n: the first host-form call 48 B per ray of a chunk in pinned host memory and the same on the device (12 MB each), the first
 *     call with EVPLP_QUERY_ORDER 16 B per ray of a chunk plus the sort's workspace (about 5 MB); all grow-only scratch of the context,
 *     freed by evplp_destroy.  A walk's stack is LDS, sized from the tree (evplp_accel_stack_entries): no scratch memory, any depth the
 *     builders accept.
 *   EVPLP_ERR_INVALID, the context staying usable and nothing written: before evplp_build_accel; while vertices are dirty (as every pass:
 *     evplp_refit_accel or evplp_build_accel first); n < 0; a null pointer with n > 0; a filter outside 0 .. 2; unknown flag bits.
 *     n = 0 returns EVPLP_OK and touches nothing.
 *   evplp_triangle_info (host only): the mesh of scene triangle `triangle` and its index within that mesh; each pointer may be null.
 *     EVPLP_ERR_INVALID before evplp_build_accel and for a triangle outside the scene. */
#define EVPLP_QUERY_CHUNK_RAYS 262144
#define EVPLP_QUERY_ORDER 1
typedef struct evplp_ray { float origin[3]; float tmin; float direction[3]; float tmax; } evplp_ray;      /* 32 B */
typedef struct evplp_hit { float t, beta, gamma; int32_t triangle; } evplp_hit;                           /* 16 B */
int evplp_trace_closest(evplp_context *ctx, const evplp_ray *rays, int32_t n, int32_t filter, int32_t flags, evplp_hit *hits);
int evplp_trace_occluded(evplp_context *ctx, const evplp_ray *rays, int32_t n, int32_t flags, uint8_t *out);
int evplp_trace_closest_device(evplp_context *ctx, const void *d_rays, int32_t n, int32_t filter, int32_t flags, void *d_hits);
int evplp_trace_occluded_device(evplp_context *ctx, const void *d_rays, int32_t n, int32_t flags, void *d_out);
int evplp_triangle_info(evplp_context *ctx, int32_t triangle, int32_t *mesh, int32_t *index_in_mesh);

/* ---- probe gather: the VPL solution's indirect light at the caller's own points (INTEGRATION B9) ----
 * What lights something the G-buffer does not hold -- a character in front of a wall, particles, a lightmap texel, a point of a volume:
 * the incident indirect radiance of the records in EVPLP_BUF_RECORDS at n free-standing points, as nine real spherical-harmonic
 * coefficients (order 2) per colour channel.  A probe has no normal and no BRDF; the caller applies both (evplp_sh_irradiance).
 *   Slots read: record slot k < num_vpl_light_paths * photons_per_path, in slot order, counts iff its flags have EVPLP_USABLE_VPL.  The
 *     arithmetic is the light-subpath gather's (evplp_gather_lvc) with the receiver taken away:
 *       v12 = pos_k - x;  c2 = max(-((n_k.x v12.x + n_k.y v12.y) + n_k.z v12.z), 0), every operation rounded on its own;  c2 <= 0: no ray, no term.
 *       Shadow ray: origin pos_k, direction -v12, tmin 0.0001f, tmax 1.0f - 0.0001f -- walked as evplp_trace_occluded walks it, so the
 *       visibility of a pair is what evplp_trace_occluded answers for that ray.
 *       A pair whose dist2 = (v12.x v12.x + v12.y v12.y) + v12.z v12.z, each operation rounded to fp32 on its own, is not a normal finite
 *       number (!(dist2 >= 2^-126 && dist2 <= FLT_MAX)) casts no ray, adds no term and is not counted in lit: a probe within about
 *       1e-19 of a record, or 2^64 and more away from it.  A normal dist2 puts the largest |v12 component| at 2^-63 / sqrt(3) or above, a
 *       finite one below 2^64, so every ray walked is one evplp_trace_occluded accepts; and rsq(dist2), w, cos2 and 1 / max(dist2,
 *       min_distance^2) are finite: the position of a probe with finite coordinates never makes a byte of its answer non-finite.
 *       A lit pair: dist2 as above, w = v12 rsq(dist2), cos2 = c2 rsq(dist2),
 *         brdf2 = rho_d_k / pi + rho_s_k PhongEvalF(-w, flux_dir_k, n_k, e_k)    (0 for rho_s = 0; the power is exp2(e log2 d) on the hardware)
 *         E = flux_k brdf2 cos2 / max(dist2, min_distance^2),   c[i] += E Y_i(w)
 *     with Y_i the real SH basis of index l (l + 1) + m on w = (x, y, z): Y0 = 0.28209479, Y1 = 0.48860251 y, Y2 = 0.48860251 z,
 *     Y3 = 0.48860251 x, Y4 = 1.09254843 x y, Y5 = 1.09254843 y z, Y6 = 0.31539157 (3 z^2 - 1), Y7 = 1.09254843 x z, Y8 = 0.54627422 (x^2 - y^2).
 *     min_distance bounds the 1 / d^2 of a record next to the probe (a probe has no surface that would bound it).
 *   Result: lit = the number of lit pairs, c = the sum / (float)num_vpl_light_paths.
 *   Fixed association: the slots are cut into slices of EVPLP_PROBE_SLICE_SLOTS consecutive SLOTS (not usable records); a slice is summed in
 *     slot order in fp32, the slices' sums are added in slice order, then the division.  A probe's 112 bytes therefore depend on its
 *     position, the records and the tree alone: not on n, on its index in the batch, on the chunking, or on the host or device form.
 *   An invalid probe -- a coordinate that is not finite -- is never walked: c = 0, lit = -1.  The kernel decides it.
 *   The host form copies one chunk of EVPLP_PROBE_CHUNK probes at a time through pinned memory and waits; the _device form takes device
 *     pointers (n x 3 floats; n evplp_probe_sh, 16-byte aligned), enqueues on the context's stream and does not wait.  Scratch, grow-only and
 *     freed by evplp_destroy: EVPLP_PROBE_CHUNK * ceil(slots / EVPLP_PROBE_SLICE_SLOTS) * 112 bytes of partial sums (it depends on the slot
 *     count, never on n), and for the host form 124 B per probe of a chunk on the device and pinned.
 *   EVPLP_ERR_INVALID, the context staying usable and nothing written: before evplp_build_accel; while vertices are dirty; n < 0; a null
 *     pointer with n > 0; null params; min_distance not finite or <= 0; flags != 0; num_vpl_light_paths or photons_per_path 0; more slots
 *     than the context's record buffer holds (num_light_paths * photons_per_path of evplp_config); a _device destination that is not
 *     16-byte aligned.  n = 0 returns EVPLP_OK and touches nothing.
 *   Host only, no GPU: evplp_probe_pair is the term of one (record, point) pair with visibility 1 in fp32 with libm's powf, E Y_i as
 *     out27[3 i + channel], not divided (all zeros for c2 <= 0 and for a pair the dist2 test above skips, decided on the kernel's bits; the
 *     flags are not looked at); evplp_sh_basis is Y_0 .. Y_8 of a direction
 *     (taken as given: not normalised); evplp_sh_irradiance is the irradiance on a surface of unit `normal` -- the clamped-cosine
 *     convolution (Ramamoorthi and Hanrahan 2001): band l weighted pi, 2 pi / 3, pi / 4, the basis evaluated at the normal.  rho_d / pi
 *     times it is the diffuse radiance leaving that surface. */
#define EVPLP_PROBE_CHUNK 16384          /* probes per launch */
#define EVPLP_PROBE_SLICE_SLOTS 256      /* record slots summed by one wave, in slot order */
typedef struct evplp_probe_params { uint32_t num_vpl_light_paths, photons_per_path; float min_distance; uint32_t flags; } evplp_probe_params;
typedef struct evplp_probe_sh { float c[9][3]; float lit; } evplp_probe_sh;              /* 112 B */
int evplp_gather_probes(evplp_context *ctx, const evplp_probe_params *params, const float *positions /* n x 3 */, int32_t n, evplp_probe_sh *out);
int evplp_gather_probes_device(evplp_context *ctx, const evplp_probe_params *params, const void *d_positions, int32_t n, void *d_out);
void evplp_probe_pair(const evplp_record *r, const float x[3], float min_distance, float out27[27]);
void evplp_sh_basis(const float dir[3], float y[9]);
void evplp_sh_irradiance(const evplp_probe_sh *sh, const float normal[3], float rgb[3]);

/* ---- surface gather: the renderer's two estimates at the caller's own surface points (INTEGRATION B10) ----
 * A lightmap texel, a texture-space shading sample, the hit of a reflection ray (evplp_trace_closest + evplp_triangle_info), the G-buffer of
 * a second camera: a point with a normal and a BRDF that is no pixel of the context's frame.  It gets what a pixel gets -- the clamped VPL
 * sum with its glossy receiver and all six mis_modes, and the photon density estimate that pays the clamped energy back.
 *   A point is the four float4 of a G-buffer pixel; valid == 0 is the stencil (g_pos.w): eight zeros.  eyes: one eye per point (n x 3), or
 *     NULL: fp->camera_pos for all.  Of fp are read: mis_mode, pdf_mc, clamping_value, photon_radius, num_light_paths, num_vpl_light_paths,
 *     photons_per_path, and camera_pos when eyes is NULL.  Nothing else.
 *   EVPLP_SURFACE_VPL: vpl = splatColor's sum (evplp_gather_lvc's pair: the cosine test with every operation rounded on its own, the
 *     shadow ray [0.0001f, 1.0f - 0.0001f] from the record walked as evplp_trace_occluded walks it, vplSplat in the six modes) over the
 *     slots k < num_vpl_light_paths * photons_per_path with EVPLP_USABLE_VPL, divided by (float)num_vpl_light_paths; lit = the pairs that
 *     pass the cosine test and are unoccluded.  Fixed association, the probe gather's: slices of EVPLP_PROBE_SLICE_SLOTS consecutive slots
 *     summed in slot order, the slices in index order, then the division -- a function of the slot count alone.
 *   EVPLP_SURFACE_PHOTONS: pm = the sum of the fragment shader's value (1 / num_light_paths inside) over the slots
 *     k < num_light_paths * photons_per_path, k != 0, with EVPLP_USABLE_PHOTON and |X - P_k|^2 <= r^2 -- dv = P_k - X, (dv.x dv.x + dv.y dv.y)
 *     + dv.z dv.z > r r means outside, every operation rounded to fp32 on its own; the predecessor of photon k is slot k - 1, as in
 *     evplp_splat_photons; photons = the number of such pairs, those whose fragment is discarded included.
 *     The pairs come from a hashed uniform grid over the photon positions, built on the device once per call: origin = the low corner of
 *     the scene's box (the meshes as evplp_refit_accel last left them), 2^bits buckets (bits from the slot count, or the environment's
 *     EVPLP_SURFACE_GRID_BITS, 1 .. 24: the results do not depend on it), a stable radix sort of (bucket, slot).  A point visits the cells
 *     of its range in ascending (z, y, x) and takes, in each cell's bucket, exactly the photons whose own cell is the visited one, in
 *     ascending slot: collisions cost time and can neither drop nor repeat a pair.  A point's 16 photon bytes are a function of the
 *     point, its eye, the records, the radius and the scene's box -- not of n, its index, the chunking, the form or bits.
 *     The pad.  The test is fp32: a photon passes it at a true distance up to r (1 + 2^-22) per axis (2^-59 for radii whose squares
 *     underflow).  reach = max(r (1 + 2^-20), 2^-59) exceeds that, and since a photon's coordinate P is an fp32 number and rounding is
 *     monotone, fl(X - reach) <= P <= fl(X + reach).  cell(p) = floor(clamp(fl(fl(p - lo) / edge), -8, 2^17)) is monotone in p, so the
 *     photon's cell lies between the cells of those two ends whatever (x +- r - lo) / edge rounds to: the same function on both sides.
 *     edge = max(2 reach (1 + 2^-4), 2^-16 M), M bounding every magnitude involved, keeps the two ends less than one cell apart after
 *     their four roundings: at most 2 cells per axis (3 are promised).  A point farther than reach from the box on some axis is answered
 *     with zeros without touching the table: photons are surface points and lie inside the box.
 *   A point or an eye with a coordinate that is not finite is never walked: zeros with lit = photons = -1.  A half not asked for: zeros.
 *   Forms as the probe gather's: the host form copies one chunk of EVPLP_SURFACE_CHUNK points at a time through pinned memory and waits;
 *     the _device form takes device pointers (n evplp_surface_point and n evplp_surface_light, both 16-byte aligned; n x 3 floats or
 *     NULL), enqueues on the context's stream and does not wait.
 *   Scratch, grow-only, freed by evplp_destroy, a function of the slot counts and never of n:
 *       partial sums     EVPLP_SURFACE_CHUNK * ceil(vpl slots / EVPLP_PROBE_SLICE_SLOTS) * 16 B
 *       grid             photon slots * (80 B compact record + 16 B keys and slots, before and behind the sort) + (2^bits + 2) * 4 B + the
 *                        sort's workspace
 *       host form        108 B per point of a chunk (point, eye, result), on the device and pinned
 *   EVPLP_ERR_INVALID, the context staying usable and nothing written: what evplp_gather_probes refuses (before evplp_build_accel, dirty
 *     vertices, n < 0, a null pointer with n > 0, null fp, a count of 0 or more slots than the record buffer holds, for each half asked
 *     for); what == 0 or unknown bits; mis_mode > 5; with PHOTONS a radius that is not positive and finite; a walk stack above 64 KB; a
 *     _device pointer that is not 16-byte aligned.  n = 0 returns EVPLP_OK and touches nothing.
 *   Host only, no GPU, the functions the kernels call: evplp_photon_grid_plan gives the edge and bits for a radius, a box and a photon
 *     count (EVPLP_ERR_INVALID for a radius or a box that is not finite, radius <= 0, lo > hi); evplp_photon_grid_cell the cell of a
 *     position and, returned, its bucket; evplp_photon_grid_range the cells [cell_lo, cell_hi] a point visits, 0 when it is farther than
 *     the reach from the box and visits none, else 1. */
#define EVPLP_SURFACE_VPL      1u
#define EVPLP_SURFACE_PHOTONS  2u
#define EVPLP_SURFACE_CHUNK    16384      /* points per launch */
typedef struct evplp_surface_point {      /* 64 B: the four float4 of a G-buffer pixel */
    float pos[3];   float valid;          /* valid == 0: stencilled out, as g_pos.w */
    float normal[3]; float pad0;
    float rho_d[3]; float pad1;
    float rho_s[3]; float phong_exp;
} evplp_surface_point;
typedef struct evplp_surface_light { float vpl[3]; float lit; float pm[3]; float photons; } evplp_surface_light;   /* 32 B */
int evplp_gather_surface(evplp_context *ctx, const evplp_frame_params *fp, uint32_t what, const evplp_surface_point *points,
                         const float *eyes /* n x 3, or NULL: fp->camera_pos for all */, int32_t n, evplp_surface_light *out);
int evplp_gather_surface_device(evplp_context *ctx, const evplp_frame_params *fp, uint32_t what, const void *d_points, const void *d_eyes,
                                int32_t n, void *d_out);
int evplp_photon_grid_plan(float radius, const float box_lo[3], const float box_hi[3], uint32_t usable_photons, float *edge, uint32_t *bits);
uint32_t evplp_photon_grid_cell(const float p[3], const float box_lo[3], float edge, uint32_t bits, int32_t cell[3]);
int evplp_photon_grid_range(const float x[3], float radius, const float box_lo[3], const float box_hi[3], float edge, int32_t cell_lo[3], int32_t cell_hi[3]);

/* ---- lightmap baking: surface points from hits, the atlas rasteriser, the bake (INTEGRATION B11) ----
 * The two links between what a caller holds and what evplp_gather_surface wants, and the call that chains them, all on the device.
 *   evplp_surface_points: a hit (evplp_trace_closest's, the rasteriser's, the caller's own) becomes the four float4 a G-buffer pixel of
 *     that hit would hold, with evplp_primary's arithmetic, every operation rounded on its own: w0 = 1 - beta - gamma,
 *     P = (p1 beta + p2 gamma) + p0 w0 per component, N = the flat winding normal normalize(cross(p1 - p0, p2 - p0)) with the oracle's
 *     roundings, rho_d / rho_s / phong_exp the triangle's material, textured ones sampled bilinearly at the interpolated texcoords.
 *     valid = 1, pads 0.  hit.t is not read and nothing is walked.  flags: EVPLP_POINTS_WHITE writes rho_d = (1, 1, 1), rho_s = 0,
 *     phong_exp = 0 instead (the gather's result times pi is then the irradiance); EVPLP_POINTS_FACE_EYES flips the normal where
 *     (N.x e.x + N.y e.y) + N.z e.z < 0 with e = eye - P, every operation rounded on its own, and needs eyes (n x 3).
 *     64 zero bytes (valid = 0, which evplp_gather_surface answers with zeros) for: triangle < 0 (a miss -1, an invalid ray -2); a
 *     triangle at or above the scene's count; a beta or gamma that is not finite; a normal that is not finite (a triangle without area).
 *     Chunked as the queries are (EVPLP_QUERY_CHUNK_RAYS hits per launch): the host form stages through pinned memory and waits (92 B
 *     per hit of a chunk, on the device and pinned, made by the first host-form call of this section); the _device form takes device
 *     pointers (n evplp_hit and n evplp_surface_point, both 16-byte aligned; n x 3 floats or NULL), enqueues and does not wait.
 *     EVPLP_ERR_INVALID, nothing written: before evplp_build_accel; dirty vertices; n < 0; a null pointer with n > 0; unknown flags;
 *     EVPLP_POINTS_FACE_EYES without eyes; a _device pointer that is not 16-byte aligned.  n = 0 returns EVPLP_OK and touches nothing.
 *   evplp_lightmap_samples: for every sample of every texel of a width x height atlas (1 .. 8192 each; samples = 1, 2 or 4 per axis) the
 *     triangle of the selection that covers it in UV space.  mesh: one mesh, or -1 for every triangle of the scene.  uvs: 6 floats per
 *     triangle of the selection (u0 v0 u1 v1 u2 v2), or NULL for the selection's own texcoords.  out[((y width + x) S + j) S + i]:
 *     triangle = the scene triangle (evplp_trace_closest's numbering) or -1 where nothing covers the sample, t = 0, beta / gamma below.
 *     Row y = 0 lies at v = 0.  Coverage is integer arithmetic, hence watertight and the same on every device and on the host:
 *       X = rint(fl(fl(u * (float)width) * 256.0f)), Y with the height: nearest even, 8 sub-texel bits; a triangle with a uv that is not
 *         finite or a snapped magnitude above 2^22 is skipped.  Sample (x, y, i, j) lies at px = 256 x + (2 i + 1) 128 / S, py likewise.
 *         No wrap: what lies outside [0, 1]^2 is clipped by the atlas.
 *       A2 = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0) in int64.  0: skipped.  < 0: a mirrored chart, rasterised as (v0, v2, v1), beta and
 *         gamma swapped back.  The edge a -> b has E = (bx - ax)(py - ay) - (by - ay)(px - ax).  Inside iff for all three edges E > 0, or
 *         E == 0 and the edge owns: d = b - a, d.y > 0 || (d.y == 0 && d.x < 0).  Of the two directions of a shared edge exactly one owns.
 *       beta = (float)((double)E_ca / (double)A2), gamma = (float)((double)E_ab / (double)A2).  Among several covering triangles the
 *         lowest scene index wins.
 *     The atlas is worked on in bands of whole texel rows holding at most EVPLP_LIGHTMAP_CHUNK samples (the environment's
 *     EVPLP_LIGHTMAP_BAND lowers it: the results do not depend on it), so no allocation depends on width x height: the selection's
 *     set-up triangles (32 B each, 24 B more where uvs come from the host), a band's tile arrays (12 B per 8 x 8-texel tile and the
 *     scan's workspace), and the tiles' triangle lists, 4 B per (triangle, tile) pair of a band.  That last array alone follows the
 *     scene -- the overlap of its charts, not the atlas -- and its size is known only on the device: per band one 4-byte read-back sizes
 *     it, and BOTH forms wait there.  The _device form (d_uvs or NULL, d_out 16-byte aligned) enqueues the rest and does not wait again.
 *     EVPLP_ERR_INVALID, nothing written: before evplp_build_accel; dirty vertices; an unknown mesh; width, height or samples out of
 *     range; a null destination; a _device destination that is not 16-byte aligned.
 *   evplp_lightmap_cover (host only, no GPU): 1 iff sample (i, j) of texel (x, y) is covered by the one triangle uv6, with its beta and
 *     gamma -- the header the kernels include, compiled for the host.  0 for arguments out of range.
 *   evplp_bake_lightmap: per band, the rasteriser's samples become surface points (flags: EVPLP_POINTS_WHITE or 0), the points go through
 *     evplp_gather_surface_device with eyes NULL (fp->camera_pos is every sample's eye; fp and what as there), and a texel takes the fp32
 *     sums of vpl, pm and photons over its samples with valid = 1 in ascending (j, i), each divided by their count; coverage = count / S^2.
 *     A texel with no such sample is 32 zero bytes.  Then `gutter` (0 .. 8) passes over the whole atlas, each reading the state before
 *     it: in pass d = 1 .. gutter a texel still at coverage 0 with at least one of its eight neighbours at coverage != 0 takes the mean of
 *     those neighbours -- the fp32 sum in the order (-1,-1) (0,-1) (1,-1) (-1,0) (1,0) (-1,1) (0,1) (1,1), divided by their number -- and
 *     coverage = -d.  No wrap at the borders.  out: width * height texels, row y = 0 at v = 0.
 *     A covered texel's 32 bytes are a function of its samples' points, the records, the radius and the tree: not of the band size, the
 *     form, or the rest of the atlas.  The photon grid of the surface gather is built once per band.
 *     Scratch beyond the rasteriser's, grow-only: 112 B per sample of a band (hit, point, result); 32 B per texel of the atlas for the
 *     host form, and as much again when gutter > 0 (either form).  The host form waits and copies the atlas out; the _device form
 *     (d_out: width * height evplp_lightmap_texel, 16-byte aligned) waits only for the bands' pair counts.
 *     EVPLP_ERR_INVALID, nothing written and the context usable: everything evplp_gather_surface refuses; null params; an unknown
 *     mesh; width, height, samples or gutter out of range; unknown flags; a null or (_device) misaligned destination.
 *   All scratch of this section is grow-only and freed by evplp_destroy. */
#define EVPLP_POINTS_WHITE      1u  /* rho_d = (1,1,1), rho_s = 0, phong_exp = 0: lighting without the albedo (x pi = irradiance) */
#define EVPLP_POINTS_FACE_EYES  2u  /* flip the normal where dot_exact(n, eye - P) < 0; needs eyes */
#define EVPLP_LIGHTMAP_CHUNK    262144      /* samples per band */
typedef struct evplp_lightmap_params { int32_t mesh, width, height, samples, gutter /* 0..8 */; uint32_t flags /* EVPLP_POINTS_WHITE */; } evplp_lightmap_params;
typedef struct evplp_lightmap_texel { float vpl[3]; float coverage; float pm[3]; float photons; } evplp_lightmap_texel;   /* 32 B */
int evplp_surface_points(evplp_context *ctx, const evplp_hit *hits, int32_t n, uint32_t flags, const float *eyes /* n x 3 or NULL */, evplp_surface_point *out);
int evplp_surface_points_device(evplp_context *ctx, const void *d_hits, int32_t n, uint32_t flags, const void *d_eyes, void *d_out);
int evplp_lightmap_samples(evplp_context *ctx, int32_t mesh /* or -1: every triangle of the scene */, const float *uvs /* 6 floats per triangle of the
    selection, or NULL: the mesh's own texcoords */, int32_t width, int32_t height, int32_t samples /* 1, 2, 4 per axis */,
    evplp_hit *out /* width*height*samples^2, index ((y*width + x)*S + j)*S + i */);
int evplp_lightmap_samples_device(evplp_context *ctx, int32_t mesh, const void *d_uvs, int32_t width, int32_t height, int32_t samples, void *d_out);
int evplp_lightmap_cover(const float uv6[6], int32_t width, int32_t height, int32_t samples, int32_t x, int32_t y, int32_t i, int32_t j, float *beta, float *gamma);
int evplp_bake_lightmap(evplp_context *ctx, const evplp_frame_params *fp, uint32_t what /* EVPLP_SURFACE_VPL | _PHOTONS */, const evplp_lightmap_params *params,
                        const float *uvs, evplp_lightmap_texel *out /* width*height, row y = 0 at v = 0 */);
int evplp_bake_lightmap_device(evplp_context *ctx, const evplp_frame_params *fp, uint32_t what, const evplp_lightmap_params *params, const void *d_uvs, void *d_out);

/* ---- progressive surface gather: per-point photon statistics with per-point radii (INTEGRATION B12) ----
 * evplp_gather_surface answers one record buffer at one radius.  These calls fold one record buffer after another into a state the caller
 * keeps per point -- stochastic progressive photon mapping (Hachisuka and Jensen 2009): every point has its own squared radius, its own
 * photon count and its own unnormalised flux, and the radius shrinks where photons arrive.
 *   A state is 48 B; 48 zero bytes are a fresh state, the caller clears the array, there is no init call.
 *   Only mis_mode 0, 4 and 5.  pdf_mc = n_vpl / n_light / (pi r^2) would be a per-point quantity and enter both halves per pair in modes
 *     1 - 3; in modes 0, 4 and 5 nothing reads it, the VPL half does not depend on the radius and the photon-side weight is 1.
 *   One call, per point, with alpha in (0, 1] and r0sq = fl(fp->photon_radius * fp->photon_radius); every operation rounded to fp32 on
 *   its own, divisions IEEE's:
 *     valid == 0 (the stencil): the state is not touched at all.
 *     A point or eye that is not finite: flags |= EVPLP_STATE_INVALID, nothing else is touched, nothing is walked.  The same for a state
 *       with pm_calls > 0 whose radius2 is not finite, <= 0 or > r0sq, in a call that asks for photons: fp->photon_radius is the call's
 *       bound -- the grid is planned for it, and radii only shrink.
 *     EVPLP_SURFACE_VPL: vpl += v, lit_sum += lit with v, lit exactly the 16 bytes evplp_gather_surface writes for the point; vpl_calls++.
 *     EVPLP_SURFACE_PHOTONS: radius2 = r0sq first if pm_calls == 0.  The cells of the point's range in ascending (z, y, x), in a bucket in
 *       ascending slot, the photons whose own cell is the visited one (evplp_gather_surface's order); outside iff, with dv = P_k - X,
 *       (dv.x dv.x + dv.y dv.y) + dv.z dv.z > radius2.  M = the number inside (discarded fragments included, as `photons` counts them),
 *       Phi = the fp32 sum in visiting order of the fragment's value in modes 0 / 4 / 5 with the photon-side factor
 *       flux * rcp((float)num_light_paths): InvPi * uInvPhotonRadius2 is taken out.  If M > 0:
 *           Nn = n + alpha (float)M;  ratio = Nn / (n + (float)M);  radius2 = radius2 ratio;  tau = (tau + Phi) ratio;  n = Nn
 *       else tau, radius2 and n keep their bytes.  pm_calls++.
 *       The range is evplp_photon_grid_range's on the grid planned for fp->photon_radius, with a per-point bound of sqrt(radius2) that
 *       never exceeds fp->photon_radius and is made without a square root (surface_state.h states why the proof of the pad holds).
 *   A point's state after a call is a function of its state before, the point and its eye, the records, fp->photon_radius, alpha, the
 *     scene's box and the tree -- not of n, its index, the chunking, the form or EVPLP_SURFACE_GRID_BITS.
 *   Resolve, to an evplp_surface_light: vpl = vpl / (float)vpl_calls, lit = lit_sum / (float)vpl_calls,
 *     pm = (tau * InvPi) / (radius2 * (float)pm_calls), photons = n.  A half with 0 calls: zeros.  EVPLP_STATE_INVALID: zeros with
 *     lit = photons = -1.  A fresh state: 32 zero bytes.
 *   Forms, chunking and scratch as evplp_gather_surface: the host forms stage EVPLP_SURFACE_CHUNK points at a time (48 B more per point,
 *     each way) and wait; the _device forms take device pointers (states 16-byte aligned as the points are), enqueue and do not wait.
 *     evplp_surface_resolve (host) goes through the device kernel, staged.  Beyond evplp_gather_surface's scratch: 32 B per point of a chunk.
 *   EVPLP_ERR_INVALID, nothing written, the context usable: everything evplp_gather_surface refuses; mis_mode 1 - 3; an alpha that is
 *     not finite or outside (0, 1]; null states with n > 0; a _device state pointer that is not 16-byte aligned.  n = 0: EVPLP_OK.
 *   The bake.  evplp_bake_lightmap_progressive_device is one iteration over the atlas: per band raster -> points -> the progressive gather
 *     on that band's slice of d_states (width * height * samples^2 states, the samples' order; eyes NULL).  The raster is repeated per
 *     call, so the call keeps no per-atlas memory; an uncovered sample's point has valid = 0 and its state stays fresh.  params->flags is
 *     read by this call only; gutter by the resolve only.  evplp_bake_lightmap_resolve needs no raster: a sample counts when
 *     vpl_calls + pm_calls > 0 and EVPLP_STATE_INVALID is clear; a texel takes the fp32 sums of its samples' resolved vpl, pm and photons
 *     in ascending (j, i) divided by their count, coverage = count / S^2; then `gutter` passes with evplp_bake_lightmap's rule.  The
 *     states stay on the device in both forms of the resolve (201 MB at 1024^2, S = 2); the host form copies the atlas out and waits.
 *   Host only, no GPU, the functions the kernels call: evplp_surface_state_update applies one photon half (M photons, their summed value
 *     phi) to one state, the out-of-range decision included; evplp_surface_state_resolve resolves one. */
#define EVPLP_STATE_INVALID 1u
typedef struct evplp_surface_state {       /* 48 B, 16-byte aligned on the device */
    float tau[3];  float radius2;          /* unnormalised photon flux; the point's squared radius */
    float vpl[3];  float n;                /* running fp32 sum of the VPL half; N, the photons kept so far */
    float lit_sum; uint32_t vpl_calls, pm_calls, flags;   /* EVPLP_STATE_INVALID */
} evplp_surface_state;
int evplp_gather_surface_progressive(evplp_context *ctx, const evplp_frame_params *fp, uint32_t what, float alpha, const evplp_surface_point *points,
                                     const float *eyes /* n x 3 or NULL */, int32_t n, evplp_surface_state *states /* in and out */);
int evplp_gather_surface_progressive_device(evplp_context *ctx, const evplp_frame_params *fp, uint32_t what, float alpha, const void *d_points,
                                            const void *d_eyes, int32_t n, void *d_states);
int evplp_surface_resolve(evplp_context *ctx, const evplp_surface_state *states, int32_t n, evplp_surface_light *out);
int evplp_surface_resolve_device(evplp_context *ctx, const void *d_states, int32_t n, void *d_out);
int evplp_bake_lightmap_progressive_device(evplp_context *ctx, const evplp_frame_params *fp, uint32_t what, float alpha, const evplp_lightmap_params *params,
                                           const void *d_uvs, void *d_states /* width*height*samples^2 states */);
int evplp_bake_lightmap_resolve(evplp_context *ctx, const evplp_lightmap_params *params, const void *d_states, evplp_lightmap_texel *out /* host */);
int evplp_bake_lightmap_resolve_device(evplp_context *ctx, const evplp_lightmap_params *params, const void *d_states, void *d_out);
int evplp_surface_state_update(evplp_surface_state *state, uint32_t m, const float phi[3], float alpha, float r0sq);
int evplp_surface_state_resolve(const evplp_surface_state *state, evplp_surface_light *out);

/* ---- k-nearest-photon start radii for progressive states (INTEGRATION B13) ----
 * The progressive calls start every point at one radius, fp->photon_radius.  evplp_gather_surface_knn is a first photon half that starts
 * each point at the distance of its k-th nearest photon instead, found on the device by an exact select on the photon grid.
 *   For one point X, with r0 = fp->photon_radius, r0sq = fl(r0 r0), rminsq = fl(r_min r_min), and the d2 of a photon at P the value of
 *   the progressive test: dv = P - X, d2 = (dv.x dv.x + dv.y dv.y) + dv.z dv.z, every operation rounded to fp32 on its own:
 *     Candidates: the photons evplp_gather_surface's photon half counts at radius r0 -- the usable slots (slot != 0,
 *       slot < num_light_paths * photons_per_path, the photon flag set) with !(d2 > r0sq).  C is their number.  No candidate's d2 is a
 *       NaN (knn_select.h: a photon with a NaN coordinate lies on a cell no walked point's range holds), none is negative.
 *     kth: the k-th smallest d2 among the candidates, with multiplicity, where C >= k; otherwise r0sq.  (Non-negative floats order as
 *       their bit patterns do: the select works on uint32 and is exact.)
 *     rk2 = min(max(kth, rminsq), r0sq).
 *     The first photon half.  M = the number of candidates with !(d2 > rk2): ties with the k-th are inside, so M >= k may hold.
 *       Phi = their summed fragment value exactly as the progressive photon half forms it (flux * rcp((float)num_light_paths),
 *       mis_mode 0 / 4 / 5, the same visiting order, discarded fragments counted in M).  Then
 *           radius2 = rk2;  if M > 0: Nn = n + alpha (float)M; ratio = Nn / (n + (float)M); radius2 = radius2 ratio;
 *                                     tau = (tau + Phi) ratio; n = Nn;                       pm_calls = 1
 *   Which states.  Only a state with pm_calls == 0 and EVPLP_STATE_INVALID clear, on a valid point with a finite position and eye.
 *     A state with pm_calls > 0 or EVPLP_STATE_INVALID set: not a byte is touched.  valid == 0 (the stencil): not touched.  A point or
 *     eye that is not finite: flags |= EVPLP_STATE_INVALID and nothing else, as the progressive calls do.  vpl, lit_sum and vpl_calls
 *     are never touched: the call has no VPL half, evplp_gather_surface_progressive with EVPLP_SURFACE_VPL is that.
 *   What follows.  After the call such a state is an ordinary progressive state with radius2 in (0, r0sq]: every later progressive call
 *     with a bound >= this r0, the resolves and the bake accept it unchanged.  Fresh states, this call and evplp_surface_resolve are the
 *     classic k-nearest density estimate pm = Phi InvPi / rk2 (at alpha = 1).  A point with C < k gets exactly the bytes
 *     evplp_gather_surface_progressive(EVPLP_SURFACE_PHOTONS) would have written.  A point's 48 bytes do not depend on n, its index,
 *     the chunking, the form or EVPLP_SURFACE_GRID_BITS.
 *   params: k >= 1; r_min the smallest start radius, finite, > 0, <= fp->photon_radius, with fl(r_min r_min) >= 2^-100 (the range of a
 *     smaller radius2 is the call's anyway); alpha as the progressive calls take it; flags 0.
 *   Forms, chunking and staging are evplp_gather_surface_progressive's.  Scratch beyond it, grow-only and freed by evplp_destroy: 4 B per
 *     point of the batch (_device) or of a chunk (host) for the selected radii.
 *   evplp_bake_lightmap_knn_device is evplp_bake_lightmap_progressive_device with this call in the place of the progressive gather: per
 *     band raster -> points -> the k-nearest call on the band's slice of d_states.  An uncovered sample's state stays fresh.
 *   EVPLP_ERR_INVALID, nothing written, the context usable: everything evplp_gather_surface_progressive refuses for
 *     what = EVPLP_SURFACE_PHOTONS (mis_mode 1 - 3 and alpha included; the bake: everything the progressive bake refuses); null params;
 *     k == 0; an r_min that is not finite, <= 0, > fp->photon_radius or whose square is below 2^-100; nonzero flags.  n = 0: EVPLP_OK.
 *   Host only, no GPU, the functions the kernels call: evplp_knn_radius2 selects over an array of d2 values -- *radius2 = rk2 and *m = M
 *     of the definitions above, with the elements that pass !(d2 > r0sq) as the candidates; EVPLP_ERR_INVALID for a null pointer,
 *     k == 0, an rminsq that is not within (0, r0sq] or not finite, or an element that is a NaN or has its sign bit set.
 *     evplp_surface_state_seed applies "the first photon half" above to one state; EVPLP_ERR_INVALID and nothing written for a null
 *     pointer, a state with pm_calls > 0 or EVPLP_STATE_INVALID set, or a radius2 that is not within (0, r0sq]. */
typedef struct evplp_knn_params { uint32_t k; float r_min; float alpha; uint32_t flags /* 0 */; } evplp_knn_params;   /* 16 B */
int evplp_gather_surface_knn(evplp_context *ctx, const evplp_frame_params *fp, const evplp_knn_params *params, const evplp_surface_point *points,
                             const float *eyes /* n x 3 or NULL */, int32_t n, evplp_surface_state *states /* in and out */);
int evplp_gather_surface_knn_device(evplp_context *ctx, const evplp_frame_params *fp, const evplp_knn_params *params, const void *d_points,
                                    const void *d_eyes, int32_t n, void *d_states);
int evplp_bake_lightmap_knn_device(evplp_context *ctx, const evplp_frame_params *fp, const evplp_knn_params *params, const evplp_lightmap_params *lightmap,
                                   const void *d_uvs, void *d_states /* width*height*samples^2 states */);
int evplp_knn_radius2(const float *d2, uint32_t count, uint32_t k, float rminsq, float r0sq, float *radius2, uint32_t *m);
int evplp_surface_state_seed(evplp_surface_state *state, float radius2, uint32_t m, const float phi[3], float alpha, float r0sq);

/* ---- the per-iteration passes of RtComPhoton::run() (rtcomphoton.h:936-1068) ---- */
/* [deferredShading] + [lightRender]: runDeferredProgram (:710-754) + runLightProgram (:839-855);
 * jitter = (2u-1)/res NDC translation (:949).  light_flags (evplp_light_flags) restate :985-995:
 *   EVPLP_LIGHT_CLEAR       cleareveryframe: pixels that do not show the emitter are written 0 (glClear of the light framebuffer);
 *   EVPLP_LIGHT_UNOCCLUDED  cleareveryframe also clears the depth buffer the light pass shares with the deferred pass
 *                           (GL_DEPTH_BUFFER_BIT, :992): the emitter image is then NOT depth-tested against the scene;
 *   EVPLP_LIGHT_SKIP        run.lightRender = false: the light image is not touched at all.
 * The G-buffer itself is always depth-correct.
 * jitter: any finite NDC translation.  Up to one pixel (|jx| <= 2 / res_x, |jy| <= 2 / res_y; the reference's is at most half a pixel) the
 * rays start from per-tile-group entry cuts of the tree that are built once per camera; a larger one walks from the root (same result,
 * ~2x the pass's time). */
enum evplp_light_flags { EVPLP_LIGHT_CLEAR = 1, EVPLP_LIGHT_UNOCCLUDED = 2, EVPLP_LIGHT_SKIP = 4 };
int evplp_primary(evplp_context *ctx, const float jitter[2], int32_t light_flags);
/* [lightTracing]: launch(LightTrace, numLightPaths) (:869-881).  Traces paths
 * [path_begin, path_begin+path_count) into the record buffer (multi-GPU: each rank a slice). */
int evplp_trace_light_paths(evplp_context *ctx, uint32_t rng_seed, uint32_t path_begin, uint32_t path_count);
/* [vplSplat]: launch(VplSplat, W, H) with splatColor (rt/lighttracing.cu:348-379) */
int evplp_gather_vpl(evplp_context *ctx, const evplp_frame_params *fp);
/* [vplSplat] with forceVsl: splatSplotch (rt/lighttracing.cu:689-722) */
int evplp_gather_vsl(evplp_context *ctx, const evplp_frame_params *fp);
/* The "lvcphotonfam" variant of [vplSplat]: every pixel gathers the usable records of a window of
 * num_vpl_light_paths consecutive light paths starting at a per-pixel random path (mod num_light_paths):
 * splatColor of rt/lvclighttracing.cu:348-384, driven by RtLvcComPhoton (rt/rtcomphoton/rtlvccomphoton.h).
 * Uses fp->rng_seed for the per-pixel offset. */
int evplp_gather_lvc(evplp_context *ctx, const evplp_frame_params *fp);
/* The "pt" technique's device pass: launch(PathTrace, W, H) with splatColor/pathTraceSimple
 * (rt/pathtracing.cu:350-377, 240-348; host runOptixPtProgram rt/rtpt/rtpt2.h:561-573).  One camera path per
 * visible pixel continued from the G-buffer for at most max_bounces bounces, next-event estimation at every
 * vertex; radiance is ADDED to EVPLP_BUF_VPL_ACCUM when do_accumulate != 0, else replaces it ("outputBuffer"). */
int evplp_path_trace(evplp_context *ctx, const float camera_pos[3], uint32_t rng_seed, uint32_t max_bounces, int32_t do_accumulate);
/* S complete iterations of the "pt" technique in one call, for the ACTIVE tiles only.  It always accumulates, and the context's state after
 * the call is its state after
 *     for s in 0 .. samples - 1: evplp_primary(ctx, jitters + 2 s, 0); evplp_path_trace(ctx, camera_pos, rng_seeds[s], max_bounces, 1);
 * jitters: [samples][2], rng_seeds: [samples]; both are read before the call returns.  The work is enumerated as (tile, sample) items
 * from a table of the samples each 8 x 8 tile takes (all of them for an active tile and for every tile when adaptivity is off, none for a
 * retired one; budget mode, below, sets its own counts): one wavefront each, so a thin tail of noisy tiles
 * still fills the device and a retired tile costs nothing in either pass; there is no whole-frame G-buffer round trip between samples.
 * Point by point:
 *  - EVPLP_BUF_VPL_ACCUM, active tiles (every tile with adaptivity off): every in-image pixel is bit-identical to the sequence.  The samples
 *    are added to the old value one at a time, in fp32, in increasing s; this is why the per-sample results are staged and not summed
 *    first: out + r0 + r1 is not out + (r0 + r1).  A pixel whose stencil rejects sample s gains nothing for that s.
 *  - EVPLP_BUF_VPL_ACCUM, retired tiles (evplp_adaptive_enable_pt; retired before the call): written once as
 *    (float)((double)R * ((double)(N + samples) / (double)n_t)), the arithmetic of evplp_path_trace in that mode -- which is what the
 *    sequence leaves, since every step of it rewrites the pixel from R.
 *  - N advances by samples: evplp_adaptive_tiles, evplp_noise_fold(ctx, samples) and the frozen noise figures agree with the sequence.
 *  - The four G-buffer planes and the tile boxes equal the sequence's: the call ends with the ordinary whole-frame evplp_primary at
 *    jitters[samples - 1], flags 0 (the samples' own texels live in the staging buffer only).  The denoiser's guides and every other reader
 *    of the planes see no difference.
 *  - EVPLP_BUF_LIGHT, active tiles: bit-identical to the sequence -- every sample writes the emitter colour where evplp_primary would (all
 *    samples write the same colour, so the concurrent writes do not race).
 *  - EVPLP_BUF_LIGHT, retired tiles: a tile retired before the call receives only the closing pass's jitter, not the other samples'; every
 *    non-zero pixel it has equals the sequence's pixel, but an emitter edge pixel that only an earlier sample's jitter would have lit may
 *    stay as it was.
 *  - Pass statistics: the call is ONE EVPLP_PASS_PATH_TRACE pass whose rays and pairs are the sums of the sequence's per-call figures
 *    (retired tiles add nothing), and one EVPLP_PASS_PRIMARY pass (the closing one).
 *  - Staging: 64 B per pixel-sample, 4 KB per (tile, sample) item, allocated on the first call and bounded by
 *    evplp_path_trace_batch_scratch (default 1 GB): min(items, bound / 4096) slots.  If the items do not fit, the call runs them in chunks
 *    of as many as fit (primary -> trace -> accumulate each; a chunk may end inside a tile's samples), down to one (tile, sample) per
 *    chunk; the chunking changes no bit.  The item table -- each tile's first item and one (tile, s) entry per item, 4 B per tile and 4 B
 *    per item -- is built on the device without atomics and is the same on every run.  The launches are sized from the host's count of
 *    the items (the host's copy of the tile records: there is no round trip), so no chunk is an empty launch.
 *  - Refused with EVPLP_ERR_INVALID, the context staying usable: samples < 1 or > 64; a null array or camera position; a jitter that is not
 *    finite; adaptivity on in gather mode (evplp_adaptive_enable), as evplp_path_trace is; a scratch bound below one (tile, sample), 4096 B;
 *    a context of 2^25 tiles or more (an item is coded as tile * 64 + s in 32 bits; such planes hold more than 2^31 pixels).
 * The trace kernel of this call inlines the same source as evplp_path_trace's and is held to the same choice of fused multiply-adds
 * ("Adaptive path tracing, batched"; tests/test_pt_batch_same_arithmetic.py): a sample has evplp_path_trace's bits.
 * evplp_path_trace_batch_scratch sets the bound for the calls that follow (any value is taken; a buffer above a lowered bound is released
 * by the next call). */
int evplp_path_trace_batch(evplp_context *ctx, const float camera_pos[3], int32_t samples, const float *jitters /* [samples][2] */,
                           const uint32_t *rng_seeds /* [samples] */, uint32_t max_bounces);
int evplp_path_trace_batch_scratch(evplp_context *ctx, uint64_t bytes);
/* [photonSplat]: runPhotonSplat (:789-837); clear != 0 = cleareveryframe (:978-981); fp->splat_footprint selects the coverage rule */
int evplp_splat_photons(evplp_context *ctx, const evplp_frame_params *fp, int32_t clear);
/* setupPhotonSplatIcosohedron (rtcomphoton.h:632-644, called with "sphere/icosphere.obj" at :677): the proxy mesh of
 * EVPLP_FOOTPRINT_PROXY, in units of the photon radius around the photon (vertices float3[nverts], triangles int3[ntris]; any winding).
 * The mesh must be closed and convex with the origin strictly inside, and have at most EVPLP_MAX_PROXY_PLANES distinct face planes
 * (coplanar triangles count once: a ray crosses one of them); anything else is refused with EVPLP_ERR_INVALID -- the fragment count
 * of a non-convex proxy is not the entry / exit rule the kernel implements.  vertices = NULL restores the generated icosphere. */
#define EVPLP_MAX_PROXY_PLANES 128
int evplp_set_splat_proxy(evplp_context *ctx, const float *vertices, int32_t nverts, const int32_t *indices, int32_t ntris);
/* [finalize] / dumpImage: runFinalProgram(vplScale, photonScale, lightScale, gamma) (:756-787,
 * final.frag:19-35).  mask_emitter = on-screen composite (1) or saved-image sum (0, :1121-1132).
 * out_rgb: HOST pointer, 3 floats per pixel, local_rows * W pixels, y = 0 bottom. */
int evplp_resolve(evplp_context *ctx, float vpl_scale, float photon_scale, float light_scale,
                  int32_t mask_emitter, int32_t gamma, float *out_rgb);
/* The composite alone (what the reference draws to the screen every iteration, runFinalProgram(param, param, 1, true) :997-1004): the strip's RGB stays in
 * device memory, nothing is copied to the host.  evplp_resolve = this + the download.
 * With overlap_light_tracing the call does NOT wait for the verdict on the bins of a photon splat that is still in flight (the host stays an
 * iteration ahead): in the rare iteration whose bins overflowed, the presented frame lacks that one splat pass -- it runs again and is in
 * the accumulator before the next composite.  Frames that leave the device (evplp_resolve, evplp_download, evplp_group_resolve) always
 * settle first and are exact. */
int evplp_present(evplp_context *ctx, float vpl_scale, float photon_scale, float light_scale, int32_t mask_emitter, int32_t gamma);
int evplp_clear_accumulators(evplp_context *ctx);
/* Error against a reference image, reduced on the device (the regime of an equal-time comparison: error over time without reading frames back).
 * Reference image for evplp_frame_error: W x H RGB float, rows top to bottom (as evplp_load_image returns them).
 * The mask is optional: 3 bytes per pixel, top to bottom, as evplp_decode_image returns them; a pixel is kept when any of its bytes is
 * non-zero (as evplp_image_rel_mse_masked).  rgb = NULL releases the reference.  Every context keeps the whole image, so set_blocks /
 * rebalance need no re-upload.  The images are copied before the call returns.  Device memory: 12 B + 1 B (mask) per image pixel. */
int evplp_set_error_reference(evplp_context *ctx, const float *rgb_top_down, const uint8_t *mask_rgb8_top_down);
/* The composite (same arguments as evplp_present) against the reference, on the device, settled like evplp_resolve.
 * out = { mse, relMse, relMse over kept pixels (0 when none are kept) } over the pixels this context holds.  The per-pixel terms are fp32 in
 * the order of floatimage.cpp:64-112 (num = |img - ref|^2, rel = num / (|ref|^2 + 0.001), no contraction, a correctly rounded division); they
 * are summed in fp64, one image row at a time in a fixed order, and the rows in image row order on the host: the figures are a function of the
 * frame alone (one context and a group of any block table give the same doubles), not of a float accumulator as in the host evplp_image_*
 * functions.  No reference: EVPLP_ERR_INVALID.
 * Non-finite terms PROPAGATE: nothing is clamped or set aside.  A pixel whose composite or reference is Inf or NaN, whose |img - ref|^2 or
 * |ref|^2 overflows fp32 (a reference of 1e20: num = Inf, den = Inf, rel = NaN), or whose composite is negative under gamma (powf gives
 * NaN) makes every figure it enters Inf or NaN exactly as the fp32 expression does; the third figure stays finite when the mask keeps
 * such pixels out. */
int evplp_frame_error(evplp_context *ctx, float vpl_scale, float photon_scale, float light_scale,
                      int32_t mask_emitter, int32_t gamma, double out[3]);

/* Per-pixel noise without a reference image: the spread between the iterations of an accumulating run, tracked on the device.
 * Tracking follows the running sum c = rgb(EVPLP_BUF_VPL_ACCUM) + rgb(EVPLP_BUF_PHOTON_ACCUM) (fp32 per channel; the image a technique
 * saves is scale * c + light).  A fold closes batch j of k_j >= 1 iterations; its sample is D_j = c - c_prev, per channel in fp32.  Per pixel
 * and channel the library keeps, in fp64, Q = sum_j D_j^2 / k_j (a device plane); S = c_prev - c_start is taken in fp32 when it is needed
 * (c_prev: c at the last fold, c_start: c when tracking started or the accumulators were last cleared); K = sum_j k_j and B = the number of
 * folds are host counts.  The per-iteration variance is the batch-means estimator for batches of unequal size,
 *     s2 = max(0, (Q - S^2 / K) / (B - 1))      (exact in expectation for independent, identically distributed iterations),
 * and the variance of the image scale * c + light is scale^2 * K * s2 (the light plane is constant and adds nothing).
 * Not covered: bias -- VPL clamping, the photon radius: for those techniques the figure is a lower bound on the error, for path tracing it is
 * the error -- and DoProgressive runs, whose iterations are not identically distributed: there the figure is an approximation.
 * on = 1: allocates and zeroes the moments, settles the pending photon splat and snapshots c_prev = c_start = c (tracking may start in the
 * middle of a run; a second on = 1 starts again).  mask: optional, in evplp_set_error_reference's format (kept pixels of evplp_noise_estimate's
 * third figure).  on = 0 releases everything.  Device memory: 56 B per pixel of the context's planes (W x local_rows: Q 3 x 8 B, c_prev and
 * c_start 16 B each; 8 B more when that pixel count is odd), 1 B per IMAGE pixel with a mask, 32 B per local row.
 * evplp_clear_accumulators and evplp_set_blocks (so also a group's rebalance) start tracking again from the cleared sums: K = B = 0.
 * Non-finite sums.  A report says that it is broken; a decision works around the break.  A pixel is BROKEN when its den = |composite|^2 +
 * 0.001 is not finite, or any of its three v = (Q - S^2 / K) / (B - 1) is not finite -- the retired form's v for a retired pixel; v is
 * tested before the clamp and before the scale^2 * K factor.  An accumulator that is or ever was +Inf, -Inf or NaN at a fold gives such a
 * v (Inf - Inf, or Q = Inf).  An emitter pixel that mask_emitter hides reads no moments: only its den can break it.
 *   - Image figures (evplp_noise_estimate, evplp_group_noise_estimate, the technique loops' "noise" block): a broken pixel's num and rel
 *     are NaN, so every figure it enters is NaN (the third one only when the mask keeps the pixel).  An overflowed accumulator does not
 *     read as a converged pixel.
 *   - Tile figures and decisions (evplp_adaptive_tile_noise, evplp_adaptive_retire, their group forms, so evplp_plan_budgets' input): a
 *     broken pixel adds nothing and is not counted; the tile's figure is the mean over its SOUND in-image pixels, a tile without one
 *     reads 0 from evplp_adaptive_tile_noise and is never retired.  Sound pixels are unchanged to the bit.
 *   - evplp_noise_variance keeps its bytes, which evplp_denoise reads: a NaN v reads 0 (the clamp's comparison is false), a variance
 *     beyond fp32 reads Inf (an infinite v too -- times a scale of exactly 0 that is NaN). */
int evplp_noise_track(evplp_context *ctx, int32_t on, const uint8_t *mask_rgb8_top_down);
/* Closes a batch of `iterations` >= 1 accumulating iterations.  It settles the pending photon splat first, as evplp_resolve does, so it sees
 * every splat of its iterations exactly once (a pass re-run after a bins overflow included); then one element-wise pass, in stream order.
 * Tracking off, or iterations < 1: EVPLP_ERR_INVALID. */
int evplp_noise_fold(evplp_context *ctx, int32_t iterations);
/* The estimated error of the composite evplp_frame_error would measure at vpl_scale = photon_scale = scale (gamma off), reduced on the
 * device: per pixel num = sum over channels of the variance (0 on an emitter pixel where mask_emitter hides the sums), rel = num /
 * (|composite|^2 + 0.001), all in fp64; out = { mean num, mean rel, mean rel over kept pixels (0 when none) }.  The rows are reduced in a fixed
 * order and added on the host in image row order: one context and a row-strip group of any block table give the same doubles.
 * Tracking off or fewer than two folds: EVPLP_ERR_INVALID. */
int evplp_noise_estimate(evplp_context *ctx, float scale, float light_scale, int32_t mask_emitter, double out[3]);
/* The per-pixel variance scale^2 * K * s2 (fp32 per channel) in evplp_resolve's layout: local_rows x W x 3, y = 0 at the bottom.
 * Tracking off or fewer than two folds: EVPLP_ERR_INVALID. */
int evplp_noise_variance(evplp_context *ctx, float scale, float *out_rgb);
/* Denoiser of a written frame: the spatial part of SVGF (Schied et al. 2017), an a-trous wavelet filter (Dammertz et al. 2010) of the
 * composite evplp_noise_estimate describes -- (scale, light_scale, mask_emitter) mean what they mean there, so (1 / N, 1, 0) is the image
 * a photonfam run saves -- guided by the G-buffer and by the noise tracker's per-pixel variance (evplp_noise_variance at `scale`; with
 * adaptivity on, the retired tiles' frozen-rescaled variance).  It adds bias: evplp_noise_estimate does not describe the denoised image.
 * A pixel is filtered when its G-buffer position has w != 0, its light plane is zero in all three channels and it lies in the image; every
 * other pixel is the composite evplp_resolve(scale, scale, light_scale, mask_emitter, 0) gives, bit for bit, and is never a neighbour.
 * A pixel whose u or s below, as fp32 computes them, is not finite (an overflowed or NaN sample, c / a or a variance beyond fp32) is not
 * filtered either: it is that composite, is never a neighbour, and enters no history of evplp_denoise_temporal.
 * With c = the composite, v = its variance, a = max(diffuse + phong, 1e-3) per channel: u = c / a, s = sum_ch y_ch^2 v_ch / a_ch^2 with
 * y = (0.2126, 0.7152, 0.0722) (luminance l(u) = y . u).  Pass i = 0 .. levels - 1 at step h = 2^i: 5 x 5 taps at h (dx, dy), dy outer,
 * k = b(dx) b(dy) with b = [1, 4, 6, 4, 1] / 16, g_p = the 3 x 3 [1/4, 1/2, 1/4]^2 blur of s over filtered pixels (normalised), and
 *     w = k exp(-|l_p - l_q| / (sigma_luminance sqrt(g_p) + 1e-10) - |n_p . (x_q - x_p)| / (sigma_position R)) max(0, n_p . n_q)^sigma_normal
 * (R: evplp_scene_metrics' bounding-sphere radius); u' = sum w u_q / sum w, s' = sum w^2 s_q / (sum w)^2.  Output: a u (linear, no gamma).
 * Fixed summation order, no atomics: a call is bit-reproducible.  Output layout: evplp_resolve's (local_rows x W x 3, y = 0 at the bottom).
 * params: NULL or a zero field = the default (levels 5, sigma_luminance 4, sigma_normal 128, sigma_position 0.01).
 * Refused with EVPLP_ERR_INVALID (the context stays usable): tracking off, fewer than two folds, levels outside 1..10, a negative or
 * non-finite sigma, a null output, no scene (evplp_build_accel), and a row-strip context (strip_count > 1): a strip cannot see its
 * neighbours' rows -- evplp_group_denoise filters the whole frame.
 * Device memory, allocated on the first call and kept until evplp_destroy: 124 B per pixel of the context's planes (variance 12 B, packed
 * pixel 80 B, two pass planes 32 B). */
typedef struct evplp_denoise_params {
    int32_t levels;             /* a-trous passes, 1..10; 0 = 5 */
    float sigma_luminance;      /* 0 = 4 */
    float sigma_normal;         /* exponent of the normal term; 0 = 128 */
    float sigma_position;       /* plane distance in units of the bounding-sphere radius; 0 = 0.01 */
    int32_t reserved[4];
} evplp_denoise_params;
int evplp_denoise(evplp_context *ctx, float scale, float light_scale, int32_t mask_emitter, const evplp_denoise_params *p, float *out_rgb);

/* Temporal accumulation across the frames of a moving scene: the temporal half of SVGF, by backward reprojection, in front of evplp_denoise's
 * a-trous passes.  Off by default; evplp_denoise and every other call are unchanged by it.
 *
 * evplp_temporal_enable(ctx, 1) allocates 36 B per original triangle (the previous pose) and 32 B per pixel of the context's planes (the
 * hits evaluated on that pose); 0 releases them and the history.  A context that never enables it allocates nothing.  The context that
 * filters also holds the history, double-buffered, 2 x 48 B per pixel of the frame, allocated by its first evplp_denoise_temporal.
 * "Previous" is the state at the END of the previous successful evplp_denoise_temporal of this context: that call copies every
 * triangle's vertices as they then are on the device and remembers the camera.  Any number of evplp_update_mesh, evplp_transform_mesh,
 * evplp_refit_accel (rebuilds by its policy included), evplp_build_accel and evplp_set_camera calls may lie between two frames.
 * evplp_temporal_reset forgets the history: the next call behaves as a first call.  So does a change of the scene's triangle count.
 *
 * evplp_denoise_temporal(ctx, scale, light_scale, mask_emitter, denoise params, temporal params, out_rgb, info) is evplp_denoise with one
 * stage between the packing of the pixels and the first pass.  With (u, s), X, n the demodulated colour and luminance variance, the
 * position and the normal of a filtered pixel i = (x, y), and the history of the previous call per pixel h_u = (u, s), h_pos = (X,
 * filtered ? 1 : 0), h_nrm = (n, history length):
 *  1. The walk of the last evplp_primary is repeated (the same jitter, light flags and entry cuts: the hit (triangle, b, g) is the one of
 *     the G-buffer in memory) and the hit is evaluated on the previous pose: P_prev, N_prev by the G-buffer's own two expressions.  On a
 *     scene that did not move these equal EVPLP_BUF_GBUF_POSITION / _NORMAL bit for bit.
 *  2. Motion m = project(previous camera, P_prev) - project(camera, X) in pixels (evplp_project_points' function), (fx, fy) = (x, y) + m:
 *     the jitter cancels in the difference, and an unmoved point under an unmoved camera has m = 0 exactly.  No history (step 4 with n = 1,
 *     u_out = u, s_out = s) on a first call, for a P_prev at or behind the previous eye, and for (fx, fy) outside (-1, W) x (-1, H).
 *  3. Taps: (fx, fy) integral -> the one pixel, weight 1; otherwise the four pixels (floor fx + 0 / 1, floor fy + 0 / 1), x inner, with the
 *     bilinear weights ((1 - tx) or tx) * ((1 - ty) or ty).  A tap q counts when it lies in the image, h_pos[q].w != 0,
 *     |n_q . (P_prev - X_q)| <= sigma_position R and |N_prev . (X_q - P_prev)| <= sigma_position R (R and sigma_position: the a-trous
 *     passes'), and N_prev . n_q >= normal_cos.  With sw = the sum of the counted weights > 0: hist_u = sum w u_q / sw, hist_s = sum w^2 s_q
 *     / sw^2, n_hist = the smallest history length among the counted taps.  sw = 0: no history.
 *  4. n = min(n_hist + 1, max_history), a = 1 / n, u_out = (1 - a) hist_u + a u, s_out = (1 - a)^2 hist_s + a^2 s.  The variance rule
 *     ASSUMES THAT THE FRAMES ARE INDEPENDENT SAMPLES: render frame f with seeds and jitters no other frame within max_history uses (the
 *     technique JSON: "animation": {"rngAdvance": k} with k >= numMaxIteration).  With the same seeds in every frame the frames' noise is
 *     one pattern, accumulation removes none of it, and s_out understates what is left.
 *  5. (u_out, s_out) replace (u, s) for the passes, which run unchanged, and become the new history with X, n and the length n.  The
 *     history is the accumulated, unfiltered signal.  A pixel that is not filtered is copied and stores h_pos.w = 0.
 * Every operation is + - * /, floor, min, max or a compare in fp32, each rounded on its own, in a fixed order; the four counts of info are
 * integer sums.  A call is bit-reproducible, and the first call after a reset gives evplp_denoise's bytes.
 * Bias and lag: a surface whose shading changes (a moving shadow, a moving light's highlight) keeps up to max_history frames of its old
 * shading at weight (1 - 1 / n); lower max_history to trade noise for lag.  Bilinear taps blur the history slightly on every moving frame.
 * info (may be NULL): filtered pixels; those that found a history (reprojected); those that found none although the call had one
 * (disoccluded); the sum of the new history lengths over the filtered pixels; successful calls since the last reset, this one included.
 * Refused with EVPLP_ERR_INVALID, leaving the context usable and the history and the previous pose as they were: every refusal of
 * evplp_denoise; temporal not enabled; no evplp_primary since the last evplp_build_accel / evplp_refit_accel (the G-buffer in memory is
 * not the tree's); EVPLP_BUF_GBUF_POSITION bound, exposed (evplp_buffer_info) or uploaded by the caller -- the walk cannot vouch for a
 * plane it did not write; max_history outside 1..1024 (0 = 16) or normal_cos outside (0, 1] (0 = 0.9) or not finite.
 * evplp_temporal_download (tests and tools; waits): plane `which` of the last call, 4 floats per pixel of the context's planes, y = 0 at the
 * bottom: EVPLP_TEMPORAL_HISTORY_U / _POS / _NRM the history it wrote, EVPLP_TEMPORAL_PREV_POS / _PREV_NRM the hits on the previous pose
 * (zeros after a first call), EVPLP_TEMPORAL_DEBUG_HIT (the bits of the triangle index or of -1, b, g, 0) of the walk as it would run now
 * -- that plane is allocated for the call alone. */
typedef struct evplp_temporal_params {
    int32_t max_history;        /* longest history length, 1..1024; 0 = 16 */
    float normal_cos;           /* least cosine between N_prev and a tap's normal, (0, 1]; 0 = 0.9 */
    int32_t reserved[6];
} evplp_temporal_params;        /* 32 bytes */
typedef struct evplp_temporal_info {
    int64_t filtered, reprojected, disoccluded, history_sum;
    int32_t frames_since_reset, reserved;
} evplp_temporal_info;          /* 40 bytes */
#define EVPLP_TEMPORAL_HISTORY_U 0
#define EVPLP_TEMPORAL_HISTORY_POS 1
#define EVPLP_TEMPORAL_HISTORY_NRM 2
#define EVPLP_TEMPORAL_PREV_POS 3
#define EVPLP_TEMPORAL_PREV_NRM 4
#define EVPLP_TEMPORAL_DEBUG_HIT 5
int evplp_temporal_enable(evplp_context *ctx, int32_t on);
int evplp_temporal_reset(evplp_context *ctx);
int evplp_denoise_temporal(evplp_context *ctx, float scale, float light_scale, int32_t mask_emitter, const evplp_denoise_params *p,
                           const evplp_temporal_params *t, float *out_rgb, evplp_temporal_info *info);
int evplp_temporal_download(evplp_context *ctx, int32_t which, float *out);
/* n world points (3 floats each) on the screen of `cam` at W x H pixels: out_xyd = (x, y, view depth) per point, pixel-centre coordinates
 * (pixel (i, j) of a y-up image has its centre at (i, j); x to the right, y from the bottom).  With d = p - eye and (s, u, f) the
 * camera's right, up and forward: z = d . f, x = (((d . s / z) / (aspect tan(fovy / 2))) + 1) W / 2 - 0.5 and likewise y with u, H and no
 * aspect; fp32, every product and sum rounded on its own (dot products (x + y) + z).  A point with z <= 0 is at or behind the eye: (0, 0, z).
 * The function evplp_denoise_temporal measures motion with.  No GPU, no context.  EVPLP_ERR_INVALID: a null pointer, n < 0, W or H < 1. */
int evplp_project_points(const evplp_camera *cam, int32_t W, int32_t H, const float *xyz, int32_t n, float *out_xyd);

/* Adaptive gather:tiles whose estimated noise has converged stop receiving gather work (off by default; a run without it is unchanged).
 * Tile: an 8 x 8 pixel tile of the context's local rows (strip_rows is a multiple of 8: a tile never straddles two row blocks); one decision
 * per tile, independent of the partition.  N: the context's accumulating calls into EVPLP_BUF_VPL_ACCUM (evplp_gather_vpl / _vsl and
 * evplp_path_trace with do_accumulate != 0; so enabling either mode after an accumulated path-tracing sample without a clear is refused) since the accumulators were last cleared; evplp_clear_accumulators and evplp_set_blocks (so also a group's rebalance) reset N to 0 and make
 * every tile active again.
 * evplp_adaptive_retire retires an active tile when the noise tracker has closed B >= min_batches (>= 2) batches and the mean over the tile's
 * in-image pixels of the per-pixel relative variance -- rel = num / den exactly as evplp_noise_estimate forms it, with the same scale,
 * light_scale, mask_emitter and composite; the mean in fp64, summed in a fixed order (a shuffle-down tree over the tile's 64 lanes, lane =
 * (y % 8) * 8 + x % 8, 0 outside the image and for a broken pixel -- evplp_noise_track, "non-finite sums"; divided by the count of sound
 * in-image pixels; a tile without one is not retired) -- is <= tile_rel_mse.  Retirement is one-way until
 * the next clear: the tile records n_t = N and the tracker's K_t = K and B_t = B, and snapshots R = VPL_ACCUM of its pixels.  It settles
 * the pending photon splat first, as a fold does.  Returns the number of tiles this call retired (>= 0).
 * Later accumulating gathers skip a retired tile's items; the reduce writes VPL_ACCUM = (float)((double)R * ((double)(N + 1) / (double)n_t))
 * per channel (each operation rounded to nearest) for every in-image pixel of the tile, whatever that iteration's stencil says, and the
 * shadow-ray and pair counters get nothing from it: the accumulator always reads as a sum over N iterations (resolve, present, frame_error,
 * the strip exchange need nothing new).  Active tiles stay bit-identical to a run without adaptivity (VPL and photon accumulators, G-buffer,
 * light plane): a pixel's gather depends only on the pixel and the iteration's VPLs / VSLs.
 * Noise of a retired pixel: the fold leaves its Q and c_prev alone; evplp_noise_estimate and evplp_noise_variance take its variance as
 * noise_var(Q, S, K_t, B_t - 1, s2K_t) with s2K_t = ((scale * N) / n_t)^2 * K_t (fp64) -- the figure at retirement rescaled to today's
 * composite: at scale = 1 / N it equals the figure at retirement and it never shrinks.  With photons a retired pixel's photon part keeps
 * improving, so its figure is an upper bound.
 * Refused with EVPLP_ERR_INVALID (the context stays usable): evplp_adaptive_enable with N > 0, or on = 1 without noise tracking; while it
 * is on: evplp_gather_lvc, evplp_path_trace, a gather with do_accumulate == 0, evplp_noise_track (off, or a restart) with N > 0.
 * A calibration frame (evplp_calibrate_blocks) gathers every tile; the reduce still writes retired pixels from their snapshots.
 * on: 0 = off (releases the memory), 1 = the retirement mode described here, 2 = gather budget mode (described below, after the path
 * tracer's budget mode). */
int evplp_adaptive_enable(evplp_context *ctx, int32_t on);
/* Adaptive sampling for the path tracer ("render until every tile is at noise level x"): the same records, snapshot, pre-conditions and
 * memory as evplp_adaptive_enable (on = 0 releases), in path-trace mode: an accumulating evplp_path_trace honours retirement -- a retired
 * tile reads no G-buffer, traces no ray, adds nothing to the pass counters, and its in-image pixels are written as
 * (float)((double)R * ((double)(N + 1) / (double)n_t)), exactly as the gather's reduce writes them; an active tile is bit-identical to a run
 * without adaptivity (a pixel's generator is keyed by pixel and seed alone).  For the path tracer the noise figure is the error itself (no
 * clamping, no photon radius), so a retired tile's frozen figure is its error at retirement.  evplp_adaptive_retire and
 * evplp_adaptive_tiles serve both modes.  Refused with EVPLP_ERR_INVALID in this mode (the context stays usable): evplp_gather_vpl,
 * evplp_gather_vsl, evplp_gather_lvc, evplp_path_trace with do_accumulate == 0 (the snapshot describes the one plane the mode's pass owns),
 * and as above a switch of the mode or of the tracker with N > 0. */
int evplp_adaptive_enable_pt(evplp_context *ctx, int32_t on);
int evplp_adaptive_retire(evplp_context *ctx, float scale, float light_scale, int32_t mask_emitter,
                          double tile_rel_mse, int32_t min_batches);          /* >= 0: tiles retired by this call */
/* Per image tile, ceil(W / 8) x ceil(H / 8) in the planes' row order (tile row 0 = image rows 0..7 from the bottom): n_t for a retired tile,
 * N for an active one, 0 for tiles another rank owns.  Returns the number of tiles; adaptivity off or capacity too small: EVPLP_ERR_INVALID. */
int evplp_adaptive_tiles(evplp_context *ctx, int32_t *iterations_per_image_tile, int32_t capacity);

/* Budget mode of the path tracer: evplp_adaptive_enable_pt(ctx, 2).  Modes 0 and 1 know two kinds of tile, sampled at full rate or retired for
 * good; here every tile keeps improving and the caller says how fast: "this tile gets 16 samples of the next call, that one 2".  The
 * pre-conditions are those of on = 1 (noise tracking on, N = 0), the memory is the same (the item table of evplp_path_trace_batch, 4 B per
 * tile and 4 B per (tile, sample) item of the largest call, belongs to every mode).  Every tile carries a record { n_t, K_t, B_t, b_t }; its raw sum R lives in
 * the snapshot plane; b_t is its budget: -1, the state after enabling, means "all samples of the call", 0 .. 64 are set by the caller.
 * Point by point:
 *  - A batch call: evplp_path_trace_batch(ctx, cam, S, jitters, seeds, bounces) gives tile t the FIRST s_t = (b_t < 0 ? S : min(b_t, S))
 *    samples of the call, samples 0 .. s_t - 1 with their jitters and seeds.  N advances by S.  For every in-image pixel of the tile
 *    R = (((R + r_0) + r_1) + ..), fp32, one sample at a time in increasing s, a sample whose stencil rejects the pixel adding nothing;
 *    n_t += s_t; and EVPLP_BUF_VPL_ACCUM = (float)((double)R * ((double)N / (double)n_t)) per channel, each operation rounded to nearest,
 *    N the value after the call.  A tile with n_t == N holds R itself, and the accumulator reads as a sum over N iterations everywhere:
 *    resolve, present, frame_error, the strip exchange and the denoiser need nothing new.
 *  - A sample of a pixel has evplp_path_trace's bits (it is keyed by pixel, jitter and seed alone), so a tile's R equals, bit for bit, what a
 *    context with adaptivity off accumulates from a cleared accumulator when it is given exactly that tile's subsequence of (jitter, seed).
 *  - G-buffer and tile boxes: those of evplp_primary(jitters[S - 1], 0), the whole-frame pass that closes the call as it does in every mode.
 *  - EVPLP_BUF_LIGHT: each sample s < s_t writes the emitter colour for its tile; every non-zero pixel equals the full sequence's pixel
 *    (the caveat stated above for retired tiles).
 *  - Pass statistics: one EVPLP_PASS_PATH_TRACE pass whose rays and pairs cover the items actually traced, and the closing EVPLP_PASS_PRIMARY.
 *  - Staging: as stated at evplp_path_trace_batch, with sum(s_t) items: 4 KB per item, min(items, bound / 4096) slots; under
 *    evplp_path_trace_batch_scratch the items run in chunks, down to one (tile, sample) per chunk, and the chunking changes no bit.
 *  - Refused with EVPLP_ERR_INVALID in this mode, the context staying usable: evplp_path_trace (single calls); the gathers;
 *    evplp_adaptive_retire (set the tile's budget to 0 instead); a switch of the mode or of the tracker with N > 0.
 *  - evplp_clear_accumulators and evplp_set_blocks reset every record to { 0, 0, 0, -1 }.
 *  - Noise: evplp_noise_fold(ctx, iterations) keeps the host counts (K += iterations, B += 1); on the device it works per tile with
 *    k_t = n_t - K_t: a tile with k_t == 0 is left alone entirely (Q, c_prev, its record); otherwise per pixel and channel D = R - c_prev
 *    (fp32), Q += D * D / k_t (fp64, in the default fold's order), c_prev = R, then K_t = n_t and B_t += 1.  evplp_noise_estimate,
 *    evplp_noise_variance, the denoiser's variance and evplp_adaptive_tile_noise price EVERY tile as a retired one is priced:
 *    noise_var(Q, S, K_t, B_t - 1, ((scale * N) / n_t)^2 * K_t).
 * evplp_adaptive_set_budgets: the layout of evplp_adaptive_tiles (image tiles in row order); a rank takes its own tiles and ignores the
 * others.  Refused: a value outside 0 .. 64, a wrong count, a null pointer; outside budget mode; while the tracker has closed fewer than
 * two folds; while samples are unfolded (the tracker's K != N).  The last two guarantee every tile B_t >= 2 and n_t >= 1 before any tile
 * can fall behind: B_t - 1 and n_t are denominators.
 * evplp_adaptive_budgets reads the budgets back: -1 = full, 0 for tiles another rank owns; returns the number of tiles.  In this mode
 * evplp_adaptive_tiles returns n_t for every owned tile. */
int evplp_adaptive_set_budgets(evplp_context *ctx, const int32_t *samples_per_image_tile, int32_t count);
int evplp_adaptive_budgets(evplp_context *ctx, int32_t *samples_per_image_tile, int32_t capacity);
/* Gather budget mode: evplp_adaptive_enable(ctx, 2).  Retirement (on = 1) freezes a tile for good, so every threshold has an error floor;
 * here no tile stops improving and the noisy ones improve faster: a tile takes the first b_t of every S accumulating gather calls.  The
 * records { n_t, K_t, B_t, b_t }, the raw sums R in the snapshot plane, evplp_adaptive_set_budgets / _budgets / _tiles / _tile_noise and
 * evplp_plan_budgets (with samples = S) are those of the path tracer's budget mode above.  Point by point:
 *  - Entering: the pre-conditions and the memory of on = 1 (noise tracking on, N = 0; + 16 B per tile for the per-call mask), and no
 *    evplp_splat_photons since the last clear.  Every record starts as { 0, 0, 0, -1 } and R as the accumulator itself.
 *  - The window: evplp_adaptive_budget_window(ctx, S), S in 1 .. 64, 16 after entering (the path tracer's tool uses that S; a default, not
 *    a tuned number).  Gather budget mode only.
 *  - Which calls a tile takes: m counts the accumulating gather calls since the last evplp_adaptive_set_budgets,
 *    evplp_adaptive_budget_window, clear or evplp_set_blocks.  Tile t takes call m iff b_t < 0 || (m % S) < min(b_t, S).
 *  - A call: evplp_gather_vpl or evplp_gather_vsl with do_accumulate = 1; N becomes N + 1.  A tile that takes it: every in-image pixel the
 *    plain reduce would write (the plain call's stencil rule) gets R = (tree sum) / numVplLightPaths + R, the plain call's arithmetic, and
 *    n_t += 1.  A tile that skips it: its items end at once, the cut kernel gives no slots to a group whose tiles all skip, and the
 *    shadow-ray and pair counters get nothing from it.  Every in-image pixel of every tile:
 *    EVPLP_BUF_VPL_ACCUM = (float)((double)R * ((double)N / (double)n_t)) per channel, each operation rounded to nearest, N the value after
 *    the call.  A tile with n_t == N holds R itself; with budgets never set the mode equals a plain run in every bit.
 *  - A tile's R equals, bit for bit, what a context with adaptivity off accumulates from exactly that tile's subsequence of iterations.
 *  - Noise: the fold, the estimate, the variance image, the denoiser's variance and evplp_adaptive_tile_noise are those of the path
 *    tracer's budget mode (per tile k_t = n_t - K_t; every tile priced as a retired one).
 *  - evplp_adaptive_set_budgets (values 0 .. 64, refused with fewer than two folds or K != N), evplp_adaptive_budgets and
 *    evplp_adaptive_tiles (n_t) serve the mode unchanged.
 *  - Refused with EVPLP_ERR_INVALID, the context staying usable: evplp_splat_photons (the VPL part of a tile would have n_t samples and
 *    its photon part N, and one set of moments cannot price both); evplp_gather_lvc, evplp_path_trace, evplp_path_trace_batch; a gather
 *    with do_accumulate == 0; evplp_adaptive_retire (set the budget to 0 instead); a switch of the mode or of the tracker with N > 0.
 *  - A calibration frame (evplp_calibrate_blocks) walks every tile, as under on = 1; the reduce still follows the schedule. */
int evplp_adaptive_budget_window(evplp_context *ctx, int32_t window);
/* The per-tile mean of rel exactly as evplp_adaptive_retire forms it (the same lanes, the same shuffle-down tree, divided by the count of
 * sound in-image pixels), written out instead of compared with a threshold: a tile evplp_adaptive_retire(.., tau, ..) would retire is one
 * whose figure here is <= tau, the same doubles -- except a tile without a sound pixel, which reads 0 here and is never retired.  All three
 * adaptive modes; in modes 0 and 1 a tile retired earlier reports its frozen figure.  A broken pixel (evplp_noise_track, "non-finite sums")
 * adds nothing and is not counted, so the figures are finite and >= 0 for evplp_plan_budgets whatever single pixels hold.
 * Tiles another rank owns and tiles without a sound in-image pixel: 0.  Returns the number of tiles.  Refused with adaptivity or tracking
 * off, or with fewer than two folds. */
int evplp_adaptive_tile_noise(evplp_context *ctx, float scale, float light_scale, int32_t mask_emitter, double *rel_per_image_tile, int32_t capacity);
/* The planner (host only, no GPU; deterministic: separate processes agree).  rel: evplp_adaptive_tile_noise's figures, n_t:
 * evplp_adaptive_tiles'.  v_t = rel_t * n_t is the tile's per-sample relative variance.  Tiles with n_t <= 0 (not in the image, or
 * nobody's) get 0 and are left out of the quantile.  v_ref is the element at index min(m - 1, floor(q * m)) of the m remaining v_t, sorted
 * ascending, q = reference_quantile in (0, 1].  Per remaining tile, in this order: tile_rel_mse > 0 and rel_t <= tile_rel_mse: 0 (the stopping
 * rule "every tile at noise level x": a run ends when every budget is 0); v_ref not > 0: samples; otherwise
 * clamp((int)ceil(samples * sqrt(v_t / v_ref)), max(1, min_samples), samples), in plain double arithmetic.  For a fixed total of samples the
 * mean of v_t / n_t is least at n_t proportional to sqrt(v_t); with a floor of one sample no tile ever stops improving.
 * EVPLP_ERR_INVALID: samples outside 1 .. 64, min_samples outside 0 .. samples, q outside (0, 1], a null array, ntiles < 1, a rel that is
 * negative or not finite. */
int evplp_plan_budgets(const double *rel, const int32_t *n_t, int32_t ntiles, int32_t samples, int32_t min_samples, double tile_rel_mse,
                       double reference_quantile, int32_t *out_budgets);

/* Row-strip contexts (strip_count > 1): which blocks of strip_rows image rows this context owns.  By default block b belongs to rank
 * b % strip_count.  evplp_set_blocks replaces that by a table: local block l holds image block image_blocks[l], l < count <= the context's
 * capacity (evplp_config.strip_capacity_rows / strip_rows); image_blocks = NULL restores the default.  Every kernel, statistic and buffer
 * layout follows the table; per-pixel results do not depend on it.  The accumulators are cleared and the G-buffer is stale afterwards: call
 * between runs, not between the iterations of an accumulating run.  evplp_get_blocks returns the number of blocks owned (and up to `capacity` of them, in local order). */
int evplp_set_blocks(evplp_context *ctx, const int32_t *image_blocks, int32_t count);
int evplp_get_blocks(evplp_context *ctx, int32_t *image_blocks, int32_t capacity);
/* What a deal by cost is made from.  While calibration is on, the VPL / VSL gathers run self-clocking variants of their kernels (same
 * results; every wavefront adds the time it was resident to its block's counter; +1 % of the kernel); switching it on clears the counters.
 * evplp_block_costs: the counters by IMAGE block (cost_per_image_block[b], b < ceil(res_y / strip_rows), 0 for blocks of other ranks), in
 * 100 MHz clock ticks normalised to eight wavefronts per SIMD; returns the number of blocks this context owns. */
int evplp_calibrate_blocks(evplp_context *ctx, int32_t on);
int evplp_block_costs(evplp_context *ctx, uint64_t *cost_per_image_block, int32_t capacity);
/* The deal itself (host only, no GPU): longest-processing-time-first -- blocks in order of falling cost, each to the rank with the least
 * cost so far that still has room (at most capacity_blocks per rank) -- ties by block index, so that every process of a multi-process run
 * computes the same table from the same costs.  owner_rank: nblocks ints.  Returns 0, or EVPLP_ERR_INVALID when nranks * capacity_blocks
 * < nblocks. */
int evplp_deal_blocks(const uint64_t *cost_per_image_block, int32_t nblocks, int32_t nranks, int32_t capacity_blocks, int32_t *owner_rank);
/* The blocks a deal gives `rank`, in the order the rank stores (and launches) them: the most expensive first -- a strip's gather is a small
 * launch and its longest items must not start late in it (cost = NULL: image order).  Returns their number; out_blocks may be NULL. */
int evplp_rank_blocks(const uint64_t *cost_per_image_block, const int32_t *owner_rank, int32_t nblocks, int32_t rank, int32_t *out_blocks, int32_t capacity);

/* ---- buffers / statistics ---- */
int evplp_local_rows(const evplp_context *ctx);
/* device_ptr and bytes may each be null.  Taking the device pointer of EVPLP_BUF_GBUF_POSITION (or binding memory to it)
 * tells the library that the caller may write that plane unseen: the photon splat then rebuilds its per-tile position boxes
 * in every pass instead of taking them from evplp_primary. */
int evplp_buffer_info(evplp_context *ctx, int32_t which, void **device_ptr, size_t *bytes);
/* Use caller-owned device memory (e.g. a torch tensor passed to an RCCL collective). */
int evplp_bind_buffer(evplp_context *ctx, int32_t which, void *device_ptr, size_t bytes);
int evplp_download(evplp_context *ctx, int32_t which, void *host_dst, size_t bytes);
int evplp_upload(evplp_context *ctx, int32_t which, const void *host_src, size_t bytes);
int evplp_pass_stats_get(evplp_context *ctx, int32_t pass, evplp_pass_stats *out);
/* evplp_pass_stats.dominant_kernel_ms of the photon splat needs two HIP events BETWEEN the pass's three dependent launches, and they
 * hold the launches apart (18 us of a 227 us pass): they are recorded only while this is on (off by default; the gathers' dominant
 * kernels are bracketed always -- their events sit beside 50 ms kernels).  Off: the splat reports dominant_kernel_ms = ms. */
int evplp_profile_kernels(evplp_context *ctx, int32_t on);
/* evplp_pass_stats.ms comes from two HIP events around every pass; the command processor retires them between the dispatches, and a
 * loop of sub-millisecond iterations pays for that (config #4: 18 us of a 0.61 ms iteration).  Off (the default is on): a pass records
 * only the events the library itself waits on, and evplp_pass_stats_get reports ms = dominant_kernel_ms = 0 for passes run meanwhile
 * (their counters -- pairs, rays, shaded -- stay valid).  evplp_render_json switches it off for all iterations but the last. */
int evplp_profile_passes(evplp_context *ctx, int32_t on);
/* Raw device-side counters of the last run of `pass` (rays, node visits, pairs, aux, then the traversal histogram that
 * only -DEVPLP_TRAVERSAL_STATS=1 diagnostic builds fill).  Returns the number of 64-bit words written. */
int evplp_debug_counters(evplp_context *ctx, int32_t pass, uint64_t *out, int32_t capacity);
/* For tests: what the binning of the last photon splat left on the device.  Settles the pending splat as evplp_pass_stats_get does (an
 * overflowed pass has run again: the arrays describe the pass whose result is in the accumulator), waits for the stream, then copies
 * big_count (one word per bin group of 256 records: the photons of the group that went through the large-rectangle list, segment
 * overflow included) and tile_cursor (one word per 8x8-pixel tile of this context's rows, row-major over local tile rows: the entries
 * the tile's bin wanted).  n_groups / n_tiles must be the context's counts exactly ((records + 255) / 256, ((res_x + 7) / 8) x
 * (local rows / 8)); either array may be null (its count is then ignored).  Launches nothing. */
int evplp_debug_splat_bins(evplp_context *ctx, uint32_t *big_count, int32_t n_groups, uint32_t *tile_cursor, int32_t n_tiles);
/* For tests: the acceleration structure as it is on the device, copied to the host.  which = 0 nodes (64 B each), 1 leaf blocks (192 B),
 * 2 the flat triangle operands (48 B per slot, 4 slots per block), 3 the slots' original triangle indices (int32, -1 = empty), 4 the
 * four-wide nodes (128 B), 5 one float: the box pad of the last build or refit (the host builders' formula), 6 four floats: the last refit's
 * upload, leaf, box and four-wide stages in ms (zeros unless evplp_profile_kernels was on), 7 one float: the last cost measurement
 * (evplp_accel_quality, or a policy's) in ms, kernel and copy of its sums (zero unless evplp_profile_passes was on).  bytes must be the array's size exactly (counts
 * from evplp_accel_info, at least one node and one block): EVPLP_ERR_INVALID otherwise.  Waits for the stream. */
int evplp_debug_accel(evplp_context *ctx, int32_t which, void *host_dst, size_t bytes);
/* Flattened acceleration structure statistics: nodes, leaves, max depth, build ms */
int evplp_accel_info(evplp_context *ctx, int32_t *nodes, int32_t *leaves, int32_t *depth, float *build_ms);
/* The builder evplp_build_accel actually used (an evplp_bvh_builder value): cfg.bvh_builder unless the test override
 * EVPLP_BVH_BUILDER was set when the context was created, or an LBVH came out deeper than the walks' 64-entry stacks and the
 * binned-SAH builder took over.  < 0 before the first build. */
int evplp_accel_builder(const evplp_context *ctx);
/* Worst-case stack entries of the four-wide per-lane walk over the tree that was built (0: the generic bound of the depth applies). */
int evplp_accel_stack_entries(const evplp_context *ctx);
/* Device-side self checks: facts the kernels rely on, verified on the GPU they run on.  which = 0: the 7-instruction exact
 * reciprocal of the triangle predicates against the IEEE division on all 2^32 float bit patterns (under a second): out[0]
 * patterns whose bits differ, [1] of them zero / denormal inputs, [2] infinite / NaN inputs, [3] normal inputs, [4] / [5] the
 * smallest / largest biased exponent among those normal inputs (the kernels need [3] to be confined to exponents >= 253).
 * which = 1: d^e as exp2(e log2 d) on the hardware transcendentals (Phong lobes of the VPL gather and the splat) against the
 * double-precision pow for e = 1, 5, 20, 100, 1000, 10000 over 2^22 values of d in (1e-6, 1]: out[k] = largest relative error
 * where the lobe is >= 1e-4 of its peak, in units of 1e-12.
 * which = 2: the hand-written triangle-pair test of the packet walks against its C++ statement (tri_pair_test) on 4096 generated
 * pairs x 64 directions in six classes (random; small integers with rays through vertices, along edges and ending on the bounds;
 * rays in the plane; denormal denominators; an all-zero second triangle; coordinates at 1e-15 .. 1e15), for both register layouts:
 * out[0] lanes x triangles whose hit bit differs (must be 0), [1] cases, [2] hits, [3] / [4] / [5] hits of classes 0 and 1, 2 and 3,
 * 4 and 5 (the odd class in the upper 32 bits).
 * which = 3: the in-place visit of a synthetic node of an entry cut (the node read from LDS into the visit's own registers) against
 * the scalar-operand node visit on 4096 generated nodes x 64 rays with a common origin in six classes (random boxes around random
 * segments; an absent second entry, as the cut kernel writes an odd count; dead lanes among live ones; a box that ends exactly at a
 * segment end point; zero half-sizes; coordinates at 1e-15 .. 1e15): out[0] differences in the two entered-lane masks, the next
 * node, the stack pointer and the stack register (must be 0), [1] cases (lanes x children), [2] entered lanes x children of the
 * scalar-operand visit, [3] / [4] / [5] those of classes 0 and 1, 2 and 3, 4 and 5 (the odd class in the upper 32 bits).
 * which = 4: the hardware primitives of the VSL estimators against double precision, maxima in units of 1e-12: out[0] / [1] the absolute
 * error of v_sin_f32(u) / v_cos_f32(u) against sin / cos(2 pi u) over all 2^24 uniforms u = (k + 1) 2^-24; [2] the absolute error of
 * cos_t = exp2(log2(u) rcp(e + 1)) against u^(1 / (e + 1)) for e = 0, 0.5, 1, 20, 200, 1000, 10000 over 2^22 uniforms; [3] / [4] / [5] the
 * relative error of v_rcp_f32 / v_rsq_f32 / v_sqrt_f32 over 2^22 arguments in [2^-20, 2^20].
 * which = 5: the whole hand-written packet walk (EXEC = its live lanes) against the C++ walk on 4096 generated packets of 64 rays with a
 * common origin through a generated tree (255 nodes, 256 leaves of 1 - 4 triangles), in eight classes of lanes that start alive (all; all
 * but lane 0; lanes 32-63; lanes 0-31; only lane 63; only lane 0; a random quarter; none): out[0] lanes whose answers differ plus lanes
 * missing from EXEC behind the walk (must be 0), [1] cases (lanes), [2] occluded lanes, [3] / [4] / [5] those of classes 0 - 2, 3 - 5 and
 * 6 - 7, 21 bits each, the lowest class in the lowest bits.
 * Returns the number of words written or a negative status. */
int evplp_selftest(evplp_context *ctx, int32_t which, uint64_t *out, int32_t capacity);
/* The direction-sampling functions of light tracing (csrc/ev_math.h: evm_sincosf, evm_powf) as the DEVICE computes them, on host arrays of n
 * inputs: which = 0: out0 = sin(x), out1 = cos(x); which = 1: out0 = x^y.  For tests: the header is shared with the CPU oracle by #include,
 * so the byte-equality of the light-path records says nothing about these functions unless they give the same bits on both machines. */
int evplp_debug_ev_math(evplp_context *ctx, int32_t which, const float *x, const float *y, int32_t n, float *out0, float *out1);

/* ---- multi-GPU group (SURVEY 8b "Threading", 8e; the reference has one device, main.cpp:111-115).  One caller thread POSTS to
 * n_ranks contexts -- each driven by a worker thread of its own, bound to its GPU -- that own interleaved row strips of the image (see the top of this file); scene and
 * BVH are replicated; light paths are traced by every rank in full (same seed, identical records, no exchange) or 1/n per rank and shared by
 * an in-place all-gather of the record buffers (evplp_group_config.split_light_paths); every rank gathers / splats its own rows; evplp_group_resolve
 * composites the strips where they are and all-gathers them, so that every GPU holds the frame.  The collectives are RCCL
 * (ncclAllGather over xGMI; librccl is opened at run time).  Ranks that all share ONE device ("virtual ranks": tests, one-GPU
 * boxes) exchange by device copies instead.  Per-pixel results do not depend on the partition.  A pass call posts its arguments
 * (copied) to every rank's worker and returns; the workers run their ranks' calls in order.  Errors are sticky: a rank's first failing
 * call is returned by the next group call -- at the latest by evplp_group_synchronize / evplp_group_resolve, which wait for the
 * workers -- with the message in evplp_group_last_error.  evplp_* calls made directly on a rank's context (evplp_group_context) wait
 * until that rank's worker has nothing queued. ---- */
typedef struct evplp_group evplp_group;
typedef struct evplp_group_config {
    int32_t n_ranks;          /* contexts = row-strip ranks, 1..64 */
    const int32_t *devices;   /* HIP ordinal of every rank; NULL = 0, 1, .. n_ranks-1.  All distinct (RCCL) or all equal (virtual ranks) */
    int32_t strip_rows;       /* height of a row block, multiple of 8; 0 = 16 (keeps the gathers' 2 x 2-tile entry-cut groups whole) */
    int32_t use_rccl;         /* 1: a single-rank group goes through RCCL too (otherwise it needs no exchange at all) */
    int32_t partition;        /* evplp_group_partition: how the image is dealt to the ranks */
    int32_t strip_capacity_pct; /* EVPLP_PARTITION_STRIPS: a rank's strip storage in percent of the equal share; 0 = 150 (room for evplp_group_rebalance's deal by cost), 100 = none */
    /* Light tracing on n ranks: 1 = every rank traces 1/n of the paths and the record buffers are all-gathered in place (num_light_paths must be
     * a multiple of n_ranks, else as -1); -1 = every rank traces ALL paths with the same seed (identical records, no exchange); 0 = whichever
     * the library's cost model expects to be faster (evplp_group_split_model: a light-tracing launch has a latency floor, so a share of the
     * paths is not n times faster to trace, while the exchange moves num_light_paths x photons_per_path x 96 / n bytes over every xGMI link). */
    int32_t split_light_paths;
    int32_t reserved;
} evplp_group_config;
/* The model behind split_light_paths = 0 (host only): light tracing of N paths takes 0.20 ms + 1.2 us per 1 000 paths beyond 131 072 (two
 * wavefronts per SIMD; tools/lt_scale.py on one MI355X); an in-place all-gather of chunks of B bytes takes 0.02 ms + B / 48 GB/s (every chunk
 * crosses one xGMI link; 48 GB/s is an ASSUMED effective rate -- no second device was ever available to this build).  Returns 1 when
 * splitting is expected to save time, 0 when not; out_ms (optional): [0] all paths on every rank, [1] a share + the exchange. */
int evplp_group_split_model(uint32_t num_light_paths, uint32_t photons_per_path, int32_t n_ranks, double out_ms[2]);
/* EVPLP_PARTITION_STRIPS: interleaved blocks of strip_rows rows, block b to rank b % n (balanced by interleaving, at the price of every rank
 * walking the whole tree for a fraction of the rays), or dealt by measured cost (evplp_group_rebalance).  Per-pixel results do not depend on
 * the deal.  (1 was a partition into contiguous bands of rows, removed in ABI version 5: it is refused as unknown.) */
/* EVPLP_PARTITION_ITERATIONS: the ranks share out the ITERATIONS of a progressive run instead of the image.  Every rank is a whole-image
 * context (strip_count 1, no strip capacity) on the single-GPU kernel paths; ranks are distinct devices (RCCL) or virtual ranks on one device,
 * as above.  evplp_group_select_rank picks the rank that evplp_group_primary, _trace_light_paths, _gather, _splat_photons, _path_trace and
 * evplp_group_present_ex(.., exchange = 0) -- a composite of that rank's OWN accumulators -- go to (rank 0 by default); clear, load scene,
 * splat proxy and profile passes still go to every rank.  evplp_group_present (and present_ex with exchange != 0) and evplp_group_resolve
 * REDUCE: every rank settles its photon splats, the planes EVPLP_BUF_VPL_ACCUM, _PHOTON_ACCUM and _LIGHT of all ranks are exchanged (an
 * ncclAllGather per plane into a staging buffer, or read in place on a shared device), and every rank forms, on its GPU, the VPL and photon
 * sums in rank order 0, 1, .., n-1 in fp32 (every add rounded: the run reproduces itself bit for bit) and the light plane as the first
 * non-zero pixel in rank order -- every iteration writes the same emitter colour, so that is exactly one GPU's union over the iterations --
 * and composites them (every GPU holds the frame); evplp_group_resolve copies rank 0's composite to the caller.  A present / resolve with
 * no pass call since the last reduction composites the cached sums again and exchanges nothing; any pass call, a clear or an
 * evplp_group_context call (the caller may write through it) makes them stale.  Refused with EVPLP_ERR_INVALID (the group stays usable):
 * evplp_group_calibrate, evplp_group_rebalance (a single rank: EVPLP_OK), evplp_group_block_owners, split_light_paths = 1 at create
 * (0 does not consult the cost model: every rank traces its own iteration's paths).  Memory per rank beyond a single context: the sums,
 * 3 x W x local_rows x 16 B (1080p: 100 MB), allocated at the first reduction (a failed allocation is a sticky EVPLP_ERR_OOM), and with
 * RCCL a staging buffer of n x W x local_rows x 16 B (1080p, n = 8: 267 MB). */
typedef enum evplp_group_partition { EVPLP_PARTITION_STRIPS = 0, EVPLP_PARTITION_ITERATIONS = 2 } evplp_group_partition;
/* cfg: as for evplp_create; device / strip_* are set per rank by the group */
int evplp_group_create(const evplp_config *cfg, const evplp_group_config *gcfg, evplp_group **out);
void evplp_group_destroy(evplp_group *g);
const char *evplp_group_last_error(const evplp_group *g);   /* g may be NULL: error of a failed create */
int evplp_group_size(const evplp_group *g);
evplp_context *evplp_group_context(evplp_group *g, int32_t rank);   /* scene upload by hand, per-rank buffers and statistics */
int evplp_group_load_scene_json(evplp_group *g, const char *json_path);
int evplp_group_clear_accumulators(evplp_group *g);
int evplp_group_primary(evplp_group *g, const float jitter[2], int32_t light_flags);
int evplp_group_trace_light_paths(evplp_group *g, uint32_t rng_seed);
int evplp_group_gather(evplp_group *g, const evplp_frame_params *fp, int32_t kind);   /* 0 evplp_gather_vpl, 1 _vsl, 2 _lvc */
int evplp_group_splat_photons(evplp_group *g, const evplp_frame_params *fp, int32_t clear);
int evplp_group_set_splat_proxy(evplp_group *g, const float *vertices, int32_t nverts, const int32_t *indices, int32_t ntris);
/* evplp_update_mesh / evplp_refit_accel on every rank (both partitions; the calls wait for the ranks).  Refused on the caller's thread, the
 * group staying usable, where the plain context refuses. */
int evplp_group_update_mesh(evplp_group *g, int32_t mesh, const float *vertices, int32_t nverts);
int evplp_group_refit_accel(evplp_group *g);
/* evplp_transform_mesh on every rank (both partitions), refused on the caller's thread likewise; the matrix is copied before the call returns */
int evplp_group_transform_mesh(evplp_group *g, int32_t mesh, const float m[12]);
/* evplp_set_mesh_skin / evplp_pose_mesh on every rank (both partitions), refused on the caller's thread likewise; the arrays are copied
 * before the call returns */
int evplp_group_set_mesh_skin(evplp_group *g, int32_t mesh, int32_t nbones, const int32_t *bone_index, const float *weight, int32_t nverts);
int evplp_group_pose_mesh(evplp_group *g, int32_t mesh, const float *bone_matrices, int32_t nbones);
/* evplp_set_mesh_morph / evplp_morph_mesh on every rank (both partitions), refused on the caller's thread likewise; the arrays are copied
 * before the call returns */
int evplp_group_set_mesh_morph(evplp_group *g, int32_t mesh, int32_t ntargets, const float *deltas, int32_t nverts);
int evplp_group_morph_mesh(evplp_group *g, int32_t mesh, const float *weights, int32_t ntargets);
/* evplp_accel_quality / evplp_set_refit_policy on every rank (both partitions; the calls wait for the ranks).  Scene and tree are replicated,
 * so every rank computes the same doubles and a policy takes the same decision on each; the group returns rank 0's figures and fails
 * (EVPLP_ERR_INVALID) if any rank's differ.  Refused on the caller's thread, the group staying usable, where the plain context refuses. */
int evplp_group_accel_quality(evplp_group *g, struct evplp_accel_quality *out);
int evplp_group_set_refit_policy(evplp_group *g, double max_cost_ratio, int32_t rebuild_builder);
/* evplp_optimize_accel / evplp_set_refit_rotations on every rank (the tree is replicated): rank 0's rotation count is the group's, and a rank
 * whose count differs is EVPLP_ERR_INVALID, as a differing tree cost is for evplp_group_accel_quality */
int evplp_group_optimize_accel(evplp_group *g, int32_t passes, int32_t *rotations);
int evplp_group_set_refit_rotations(evplp_group *g, int32_t passes);
/* evplp_trace_closest / evplp_trace_occluded over the ranks (both partitions: scene and tree are replicated).  Rank r of N traces rays
 * [r n / N, (r + 1) n / N) into the caller's arrays, so the output is one context's byte for byte; the calls wait for the ranks.  Refused
 * on the caller's thread, the group staying usable, where the plain context refuses. */
int evplp_group_trace_closest(evplp_group *g, const evplp_ray *rays, int32_t n, int32_t filter, int32_t flags, evplp_hit *hits);
int evplp_group_trace_occluded(evplp_group *g, const evplp_ray *rays, int32_t n, int32_t flags, uint8_t *out);
int evplp_group_path_trace(evplp_group *g, const float camera_pos[3], uint32_t rng_seed, uint32_t max_bounces, int32_t do_accumulate);
/* evplp_path_trace_batch, routed like evplp_group_path_trace: a strips group runs it on every rank for its own rows (the result equals one
 * context's bit for bit; evplp_set_blocks / evplp_group_rebalance behave as for evplp_group_path_trace), an iterations group on the selected
 * rank.  The arrays are copied before the call returns.  Every refusal of evplp_path_trace_batch is raised here, on the caller's thread, and
 * leaves the group usable.  The scratch bound is per rank. */
int evplp_group_path_trace_batch(evplp_group *g, const float camera_pos[3], int32_t samples, const float *jitters /* [samples][2] */,
                                 const uint32_t *rng_seeds /* [samples] */, uint32_t max_bounces);
int evplp_group_path_trace_batch_scratch(evplp_group *g, uint64_t bytes);
int evplp_group_synchronize(evplp_group *g);
/* EVPLP_PARTITION_ITERATIONS: the rank the single-rank pass calls go to from now on (see the partition enum).  Other partitions, or a rank out
 * of range: EVPLP_ERR_INVALID. */
int evplp_group_select_rank(evplp_group *g, int32_t rank);
/* Waits for rank `rank`'s worker and its context's streams only (any partition); returns the group's sticky status. */
int evplp_group_synchronize_rank(evplp_group *g, int32_t rank);
/* Calibration for evplp_group_rebalance under EVPLP_PARTITION_STRIPS: evplp_calibrate_blocks on every rank (waits for the workers). */
int evplp_group_calibrate(evplp_group *g, int32_t on);
/* The owner of every image block (nblocks = ceil(res_y / strip_rows) ints, rank numbers); returns nblocks. */
int evplp_group_block_owners(evplp_group *g, int32_t *owner_rank, int32_t capacity);
/* EVPLP_PARTITION_STRIPS: waits for the ranks, collects the per-block costs their gathers clocked since evplp_group_calibrate(g, 1), deals
 * the blocks by cost (evplp_deal_blocks, capacity = strip_capacity_pct of the equal share), gives every rank its table (evplp_set_blocks),
 * switches the calibration off and uploads the table evplp_group_resolve assembles the frame by.  The all-gather of the strips then moves
 * max-blocks-per-rank x strip_rows rows per rank.  The accumulators are cleared and the G-buffers are stale afterwards: calibrate on a frame
 * in front of an accumulating run (the technique loop does: "device": {"deal": "cost"}, or by default when the run is long enough).
 * A single rank: nothing to do, EVPLP_OK.  No cost clocked (no calibration, or no gather ran): EVPLP_ERR_INVALID, nothing changes.  A rank
 * that refuses its table or a failed upload: every rank returns to the round-robin deal and the error is returned.
 * EVPLP_PARTITION_ITERATIONS with n > 1: EVPLP_ERR_INVALID (see the partition enum). */
int evplp_group_rebalance(evplp_group *g);
/* Host time of rank `rank`'s worker so far, in ms: out[0] inside its rank's pass calls (enqueueing; waits for a splat's verdict included),
 * out[1] inside exchanges (host barrier + collective / copies), out[2] commands run.  Waits until that worker is idle. */
int evplp_group_host_stats(evplp_group *g, int32_t rank, double out[3]);
/* evplp_profile_passes on every rank's context (waits until the workers are idle) */
int evplp_group_profile_passes(evplp_group *g, int32_t on);
/* evplp_resolve for the whole frame: out_rgb = HOST pointer, res_y * res_x * 3 floats, y = 0 bottom */
/* The per-frame exchange alone: composite every rank's strip on its GPU (final.frag:19-35) and all-gather the strips, so that every
 * GPU holds the frame; nothing is copied to the host.  evplp_group_resolve = this + the strips put into image order on rank 0's device
 * (no host-side assembly) + one copy of the W x H x 3 frame to the caller. */
/* (like evplp_present it does not wait for a pending splat's verdict when the contexts overlap light tracing; evplp_group_resolve does) */
int evplp_group_present(evplp_group *g, float vpl_scale, float photon_scale, float light_scale, int32_t mask_emitter, int32_t gamma);
/* exchange = 0: the composite alone, every rank for itself -- no host barrier, no collective (the reference needs the assembled frame only when
 * it is shown or written: rtcomphoton.h:997-1004, 1079-1102, 1124-1132); exchange != 0 = evplp_group_present.  The technique loop:
 * "device": {"exchangeEvery": k}. */
int evplp_group_present_ex(evplp_group *g, float vpl_scale, float photon_scale, float light_scale, int32_t mask_emitter, int32_t gamma, int32_t exchange);
int evplp_group_resolve(evplp_group *g, float vpl_scale, float photon_scale, float light_scale,
                        int32_t mask_emitter, int32_t gamma, float *out_rgb);
/* evplp_set_error_reference on every rank (through the workers; the caller's images are read before the call returns). */
int evplp_group_set_error_reference(evplp_group *g, const float *rgb_top_down, const uint8_t *mask_rgb8_top_down);
/* evplp_frame_error for the whole image.  EVPLP_PARTITION_STRIPS: every rank composites and reduces its own rows; about 32 bytes per row
 * come to the host and nothing is all-gathered.  EVPLP_PARTITION_ITERATIONS: the reduction of evplp_group_resolve first (or its cached
 * sums: a later resolve at the same scales does not reduce again), then rank 0 reduces the summed composite.  The result equals, bit for
 * bit, one context's over the same frame.  No reference, or a null out: EVPLP_ERR_INVALID on the caller's thread (the group stays usable). */
int evplp_group_frame_error(evplp_group *g, float vpl_scale, float photon_scale, float light_scale,
                            int32_t mask_emitter, int32_t gamma, double out[3]);
/* evplp_noise_* for a group.  EVPLP_PARTITION_STRIPS: every rank tracks and folds its own rows; an estimate posts about 32 bytes per row to
 * the host and all-gathers nothing, and equals one context's over the same frame bit for bit.  EVPLP_PARTITION_ITERATIONS: a fold closes a
 * batch of the SELECTED rank's iterations (evplp_group_select_rank); an estimate pools the ranks on the GPUs -- Q, S, K and B summed over the
 * ranks, Q and S in rank order on rank 0's device, read in place from virtual ranks and all-gathered from distinct devices (every rank then
 * holds n x the per-rank bytes of evplp_noise_track in a staging buffer; rank 0 holds 48 B per pixel of pooled moments) -- and composites
 * the ranks' summed accumulators as evplp_group_resolve does.  Tracking off, fewer than two folds in all, bad arguments: EVPLP_ERR_INVALID
 * on the caller's thread (the group stays usable).  evplp_group_noise_variance returns the whole image in evplp_group_resolve's layout. */
int evplp_group_noise_track(evplp_group *g, int32_t on, const uint8_t *mask_rgb8_top_down);
int evplp_group_noise_fold(evplp_group *g, int32_t iterations);
int evplp_group_noise_estimate(evplp_group *g, float scale, float light_scale, int32_t mask_emitter, double out[3]);
int evplp_group_noise_variance(evplp_group *g, float scale, float *out_rgb);
/* evplp_denoise for the whole frame, in evplp_group_resolve's layout, filtered on rank 0's GPU.  EVPLP_PARTITION_STRIPS: every rank packs
 * its rows (composite, variance, guides) and the packed rows are all-gathered and assembled as a resolve's strips are (80 B per pixel, and
 * n x a rank's rows on every rank); the inputs do not depend on the partition, so the output equals one context's over the same frame, bit for
 * bit, for any block table.  EVPLP_PARTITION_ITERATIONS: the composite and the light plane of evplp_group_resolve's reduction, the variance of
 * the pooled moments (evplp_group_noise_variance), and the guides of the rank that ran the last evplp_group_primary.  Device memory: see
 * the table of evplp_config.  Refusals as evplp_denoise's (strip_count aside), on the caller's thread; the group stays usable. */
int evplp_group_denoise(evplp_group *g, float scale, float light_scale, int32_t mask_emitter, const evplp_denoise_params *p, float *out_rgb);
/* evplp_temporal_enable / _reset / evplp_denoise_temporal / evplp_temporal_download for the whole frame, in evplp_group_resolve's layout (H x W,
 * y = 0 at the bottom).  Every rank keeps the previous pose and camera (36 B per triangle and 32 B per pixel of its planes each) and
 * evaluates its own rows on it.  EVPLP_PARTITION_STRIPS: the texels travel beside the packed pixels (one more all-gather, n x 32 B per
 * pixel of the exchanged rows per rank) and rank 0 assembles them (32 B per image pixel); rank 0 holds the history in IMAGE layout (96 B
 * per image pixel), so evplp_group_rebalance between two frames does not disturb it, and a group gives the single context's bits for any
 * block table.  EVPLP_PARTITION_ITERATIONS: the texels are those of the rank the last evplp_group_primary went to, whose G-buffer the
 * group's denoiser reads.  Refusals as evplp_denoise_temporal's, on the caller's thread.  evplp_group_temporal_download gives the three
 * history planes and the two previous-pose planes (not EVPLP_TEMPORAL_DEBUG_HIT: ask the rank's context). */
int evplp_group_temporal_enable(evplp_group *g, int32_t on);
int evplp_group_temporal_reset(evplp_group *g);
int evplp_group_denoise_temporal(evplp_group *g, float scale, float light_scale, int32_t mask_emitter, const evplp_denoise_params *p,
                                 const evplp_temporal_params *t, float *out_rgb, evplp_temporal_info *info);
int evplp_group_temporal_download(evplp_group *g, int32_t which, float *out);
/* evplp_adaptive_* for a group.  EVPLP_PARTITION_STRIPS: every rank decides for its own tiles, the retire call returns the sum of the ranks'
 * counts, and the tile map is assembled from the block owners (the whole image).  EVPLP_PARTITION_ITERATIONS: every call is refused --
 * pooling the ranks' decisions is not supported.  Refusals come on the caller's thread and leave the group usable. */
int evplp_group_adaptive_enable(evplp_group *g, int32_t on);
int evplp_group_adaptive_enable_pt(evplp_group *g, int32_t on);    /* path-trace mode: evplp_group_path_trace (accumulating) yes, evplp_group_gather no */
int evplp_group_adaptive_retire(evplp_group *g, float scale, float light_scale, int32_t mask_emitter,
                                double tile_rel_mse, int32_t min_batches);
int evplp_group_adaptive_tiles(evplp_group *g, int32_t *iterations_per_image_tile, int32_t capacity);
/* Budget mode for a group: evplp_group_adaptive_enable_pt(g, 2) and the three calls below, EVPLP_PARTITION_STRIPS only (refused under
 * EVPLP_PARTITION_ITERATIONS like every evplp_group_adaptive_* call).  A tile never straddles two row blocks, so a rank decides nothing: it
 * takes its own tiles from the whole-image array, and the ranks' figures are put together per tile -- budgets, tile counts, tile noise and the
 * accumulator equal one context's.  Argument errors are refused on the caller's thread and the group stays usable. */
int evplp_group_adaptive_set_budgets(evplp_group *g, const int32_t *samples_per_image_tile, int32_t count);
int evplp_group_adaptive_budgets(evplp_group *g, int32_t *samples_per_image_tile, int32_t capacity);
/* Gather budget mode for a group: evplp_group_adaptive_enable(g, 2), the window for every rank; row strips only.  evplp_group_splat_photons,
 * evplp_group_path_trace(_batch), a gather of kind 2 or without accumulation and evplp_group_adaptive_retire are refused in it. */
int evplp_group_adaptive_budget_window(evplp_group *g, int32_t window);
int evplp_group_adaptive_tile_noise(evplp_group *g, float scale, float light_scale, int32_t mask_emitter, double *rel_per_image_tile, int32_t capacity);

/* ---- host side of the reference interface (no GPU needed for these) ---- */
/* The anti-aliasing jitters of the first `count` iterations of a technique run with this rngOffset: NDC translations (x, y) =
 * (2 u - 1) / resolution with u = IndependentSampler(rngOffset).nextVec2() (rtcomphoton.h:887, 946-952) -- the reference's own
 * sampler headers as they behave under g++ / libstdc++ (tests/golden/jitter.npz); out_ndc_xy: 2 * count floats. */
int evplp_jitter_sequence(uint32_t rng_offset, int32_t count, int32_t res_x, int32_t res_y, float *out_ndc_xy);
/* The proxy EVPLP_FOOTPRINT_PROXY uses when no mesh was given: an icosahedron subdivided once onto the unit sphere (42 vertices, 80
 * faces -- the shape the 2178 bytes of the reference's sphere/icosphere.obj, a Git-LFS stub, imply), poles on the y axis.
 * vertices: 42 x 3 floats, indices: 80 x 3 ints (either may be NULL).  Returns the number of triangles (80). */
int evplp_default_splat_proxy(float *vertices, int32_t *indices);
/* The library's JSON reader as the technique blocks use it, for checking it against the reference's (vendored nlohmann::json
 * 2.1.1; main.cpp:105-121, rtcomphoton.h:107-223 -- tests/golden/json_pins.json): `path` = keys separated by '/', decimal indices
 * into arrays.  want: 0 `int v = json[..]`, 1 float, 2 bool, 3 std::string (into str, cap bytes), 4 size(), 5 kind (0 null, 1 bool,
 * 2 number, 3 string, 4 array, 5 object).  Returns 0 ok, 1 not JSON, 2 key missing / index out of range, 3 conversion error. */
int evplp_json_query(const char *text, const char *path, int32_t want, double *num, char *str, int32_t cap);
/* Progressive schedule, rtcomphoton.h:1033-1063; call after numIterations++ */
void evplp_progressive_step(int32_t num_iterations_done, float alpha, float clamp_start,
                            uint32_t n_vpl_paths, uint32_t n_light_paths,
                            float *photon_radius, float *clamping_value, float *pdf_mc,
                            int32_t force_vsl, float *vsl_radius, float *vsl_inv_pi_radius2);
/* FloatImage::Save by extension (common/floatimage/floatimage.cpp:260-273): .pfm / .hdr / .png.
 * rgb: top-down rows (after FlipY, rtcomphoton.h:1124-1127), 3 floats per pixel. */
int evplp_save_image(const char *path, int32_t w, int32_t h, const float *rgb_top_down);
int evplp_load_pfm(const char *path, int32_t *w, int32_t *h, float *rgb_top_down, size_t capacity_floats);
/* FloatImage::LoadPFM / LoadHDR by extension (floatimage.cpp:146-176, 201-221); rgb may be NULL to query the size */
int evplp_load_image(const char *path, int32_t *w, int32_t *h, float *rgb_top_down, size_t capacity_floats);
/* stbi_load(filepath, &width, &height, &channel, 3) as RtTexture calls it (rt/rtcommon.h:144): JPEG (baseline /
 * progressive) or PNG by content -> 8-bit RGB, rows top to bottom (no flip), bit-identical to the reference's
 * vendored decoder.  *channels = components in the file.  rgb may be NULL to query the size. */
int evplp_decode_image(const char *path, int32_t *w, int32_t *h, int32_t *channels, uint8_t *rgb, size_t capacity_bytes);
double evplp_image_mse(int32_t npix, const float *img, const float *ref);     /* floatimage.cpp:64-84 */
/* FloatImage::ComputeSquareErrorHeatImage (relative = 0) / ComputeRelSquareErrorHeatImage (floatimage.cpp:21-62):
 * per-pixel (relative) squared error / max_error, clamped to 1, through Color::Heat (math/color.h:83-88) */
int evplp_image_error_heat(int32_t npix, const float *img, const float *ref, float max_error, int32_t relative, float *out_rgb);
double evplp_image_rel_mse(int32_t npix, const float *img, const float *ref); /* floatimage.cpp:86-112 */
/* the same over the pixels a mask keeps (any non-zero channel; e.g. evplp_decode_image of scene/conference/conference_mask.png,
 * which blanks the emitters' aliased outlines, scene/conference/README.md); NULL mask = all pixels */
double evplp_image_rel_mse_masked(int32_t npix, const float *img, const float *ref, const uint8_t *mask_rgb8);
/* Writes a procedural closed "conference-like" room (OBJ + MTL + light OBJ + scene JSON in the
 * reference's schema) because every mesh of the reference is a Git-LFS stub.
 * Returns the number of scene triangles written (>= 0) or a negative evplp_status. */
int evplp_synth_scene(const char *out_dir, const char *name, int32_t target_triangles, uint32_t seed,
                      int32_t res_x, int32_t res_y);
/* style 0: the room of tessellated boxes above ("easy"); style 1: the same room, light and camera furnished with curved and
 * thin parts (ellipsoid cushions, cylinder legs, rotated clutter, ~2400 small occluders) -- closer to what the real
 * conference model (curved chairs, scene/conference/conference_exported.obj, an LFS stub) asks of an any-hit walk;
 * style 2: style 1 with image textures (map_Kd / map_Ks PNG files next to the OBJ) on the room shell and the table. */
int evplp_synth_scene_ex(const char *out_dir, const char *name, int32_t target_triangles, uint32_t seed,
                         int32_t res_x, int32_t res_y, int32_t style);
/* main() + LoadScene + RtComPhoton::render (main.cpp:87-121, rtcomphoton.h:107-223): parse the
 * scene JSON, load OBJ/MTL, run the `photonfam` technique, write the three images + stat file.
 * json_overrides: optional JSON object text merged over the technique block (may be NULL).
 * Build-only keys of a technique block: "bvhBuilder": "sah" | "sbvh" | "lbvh" | "gpu" | "ploc" (evplp_bvh_builder); "deterministic": bool (photon bins accumulated in record
 * order); "device": {"gpus": N, "virtual": bool, "stripRows": R, "rccl": bool, "deal": "cost" | "roundRobin", "exchangeEvery": k,
 * "stripCapacityPct": p, "splitLightPaths": bool, "cutScratchGB": g, "vslMaskGB": g} -- run on an evplp_group of N row-strip ranks (GPUs device .. device+N-1; "virtual": all ranks on `device`; "rccl": a
 * single rank goes through RCCL too; "deal": row blocks dealt by the cost a calibration frame clocks -- the default when that extra frame pays for
 * itself: from 5 iterations at six ranks and more, 25 at three to five, 100 at two -- or block b to rank b % N; "exchangeEvery": the strips are all-gathered in every k-th iteration's composite, 0 = only for
 * the frames that are written -- the default: the loop is headless; 1 = the reference's per-iteration draw; "splitLightPaths": evplp_group_config.split_light_paths, absent = the cost model; "cutScratchGB" /
 * "vslMaskGB": evplp_config.cut_scratch_bytes / vsl_mask_bytes).
 * "device": {"gpus": N, "partition": "iterations"} (photonfam / lvcphotonfam, frameMode accumulate): the N GPUs share out the ITERATIONS of the
 * progressive run instead of the image -- one evplp_group of N EVPLP_PARTITION_ITERATIONS ranks, GPU g renders iterations g, g + N, ... of the
 * whole frame, nothing is exchanged inside the loop ("exchangeEvery": k > 0 reduces in every k-th iteration), and the accumulators are summed
 * on the GPUs (rank order, reduce_shards_kernel) when a frame is written.  Under a time limit the loop waits only for the rank the next
 * iteration reuses.  N times the iterations per second with no replicated work; VPL and photon images agree with one GPU's to fp32
 * round-off (the sums are associated differently), not bit for bit; the emitter image is one GPU's exactly. */
int evplp_render_json(const char *json_path, const char *json_overrides, int32_t device, char *err, size_t err_cap);

#ifdef __cplusplus
}
#endif
#endif /* EVPLP_H */

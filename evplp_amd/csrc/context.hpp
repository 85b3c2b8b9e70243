// evplp_context: owns all device memory of one GPU's share of the frame.
#pragma once
#include "evplp_types.h"
#include "kernels.h"
#include "ray_query.hpp"

#include <string>
#include <thread>
#include <vector>

namespace evplp {
// bvh_gpu.hip: LBVH built on the device (arrays are device allocations owned by the caller)
int build_bvh_gpu(const float *verts_host, int32_t ntri, float pad_scale, hipStream_t stream, BvhDeviceBuild *out, int32_t ploc_radius = 0, int32_t ploc_search_iterations = 0);
int build_nodes4(const BvhNode *d_nodes, int32_t nnodes, hipStream_t stream, BvhNode4 **out);
void build_nodes4_into(const BvhNode *d_nodes, int32_t nnodes, hipStream_t stream, BvhNode4 *out);      // in place: enqueued, no allocation, no wait
// bvh_gpu.hip: the launches of evplp_refit_accel (enqueued; d_src: 9 floats per triangle of the run; d_order: the nodes of one height)
void refit_scatter(const float *d_src, int32_t first, int32_t count, TriAttr *attrs, hipStream_t stream);
// (meshes moved by a matrix: d_rest, 9 floats per original triangle of the scene, is filled for a run from the attributes; ONE transform
// launch per refit writes the attributes of every mesh of d_table from d_rest -- total: the moved triangles of the whole table)
void refit_rest(const TriAttr *attrs, int32_t first, int32_t count, float *d_rest, hipStream_t stream);
void refit_transform(const TransformDesc *d_table, int32_t nmesh, int32_t total, const float *d_rest, TriAttr *attrs, int32_t ntri, hipStream_t stream);
// (meshes posed by bones: ONE skin launch per refit writes the attributes of every mesh of d_table from d_rest, the corner skins d_skin
// (nskin corners) and the refit's palettes d_bones -- total: the posed triangles of the whole table)
void refit_skin(const SkinDesc *d_table, int32_t nmesh, int32_t total, const float *d_rest, const CornerSkin *d_skin, int32_t nskin, const float *d_bones, TriAttr *attrs, int32_t ntri, hipStream_t stream);
// (meshes under morph weights: ONE morph launch per refit, in front of the two above, writes every mesh of d_table from d_rest, the refit's
// weight sets d_weights (nweights floats) and the corner deltas d_deltas (ndelta float3) -- into the attributes, or into d_base (indexed like
// d_rest) for a mesh that a matrix or a pose then moves; total: the morphed triangles of the whole table)
void refit_morph(const MorphDesc *d_table, int32_t nmesh, int32_t total, const float *d_rest, const float *d_weights, int32_t nweights, const float *d_deltas, int64_t ndelta, float *d_base, TriAttr *attrs,
                 int32_t ntri, hipStream_t stream);
void refit_leaves(const RefitScene &r, hipStream_t stream);
void refit_level(const RefitScene &r, const int32_t *d_order, int32_t count, float pad, hipStream_t stream);
// (the level launch with tree rotations: d_level = the plan's level per node, d_taken / d_need = per-node scratch, d_root_out = { rotations, need } of the root)
void refit_rotate_level(const RefitScene &r, const int32_t *d_order, int32_t count, float pad, const int32_t *d_level, int32_t *d_taken, int32_t *d_need, int32_t *d_root_out, hipStream_t stream);
// bvh_gpu.hip: the launch of evplp_accel_quality (enqueued; d_out: 1 + 3 * ceil(count / 256) doubles -- the root's area, then a triple per workgroup)
void accel_cost(const BvhNode *d_nodes, int32_t nnodes, const int32_t *d_order, int32_t count, double *d_out, hipStream_t stream);
// How a mesh's vertices changed since the device scene was made, which is how the next evplp_refit_accel takes them to the device
// (evplp_context::mesh_dirty).  It is a record of the calls, not a function of the mesh's matrix, palette and weights: evplp_set_mesh_skin
// on a mesh whose pose no refit has consumed makes it Upload while morph weights may still be in force.
enum class MeshDirty : char {
    Clean,          // not at all
    Upload,         // evplp_update_mesh, or a mesh that nothing moves any more: its triangles go up through the staging array
    Matrix,         // evplp_transform_mesh: the transform launch writes it from the rest pose, or from the base of morph weights in force
    Pose,           // evplp_pose_mesh: the skin launch, likewise
    Morph,          // evplp_morph_mesh on a mesh that nothing else moves: the morph launch writes its attributes itself
};
inline bool moved_on_device(MeshDirty d) { return d == MeshDirty::Matrix || d == MeshDirty::Pose || d == MeshDirty::Morph; }   // (needs its rest pose there)
inline bool moves_base(MeshDirty d) { return d == MeshDirty::Matrix || d == MeshDirty::Pose; }      // (a matrix or a pose acts on the base)
// a mesh's part of the device's rest-pose array (HostMesh::rest_state)
enum class RestState {
    Absent,         // not there
    FromAttrs,      // the next refit makes it from the device's attributes, which still hold it
    FromHost,       // the next refit makes it from `rest`
    There,
};
// a mesh's part of the device's base array, once there is one (HostMesh::base_state)
enum class BaseState {
    Rest,           // the rest pose
    Weights,        // `base` under the weights in force
    StaleWeights,   // the base of weights that are no longer in force
};
// rest: the rest pose of a mesh that evplp_transform_mesh has moved (verts = transform_point(matrix, rest)); empty: verts is the rest pose.
// skin_bones > 0: the mesh has a skin (evplp_set_mesh_skin) -- four bone indices and four weights per vertex; palette: the
// bone matrices of the last evplp_pose_mesh (verts = skin_point(rest) under them) until a matrix or new vertices replace the pose;
// skin_at: where the mesh's corner skin lies in the device's array (in corners), -1 not there.  area, lo / hi (all vertices), alo / ahi / any_area (triangles with an area): the mesh's share of the scene's figures.
struct HostMesh {
    std::vector<float> verts, uvs; std::vector<int32_t> idx; int32_t material = 0;
    std::vector<float> rest; float matrix[12] = {}; RestState rest_state = RestState::Absent;
    float area = 0.f, lo[3] = {}, hi[3] = {}, alo[3] = {}, ahi[3] = {}; bool any_area = false;
    int32_t skin_bones = 0, skin_at = -1; std::vector<int32_t> skin_index; std::vector<float> skin_weight, palette;
    // has_matrix: a matrix of evplp_transform_mesh is in force (palette not empty: a pose is).  morph_targets > 0: the mesh has morph targets
    // (evplp_set_mesh_morph), morph_delta [targets][vertices][3]; morph_w: the weights in force (evplp_morph_mesh), empty: none; base: the
    // morphed rest pose while weights are in force (verts = base under the matrix or the pose in force), empty otherwise.  morph_at: where
    // the mesh's corner deltas lie in the device's array (in float3), -1 not there.
    bool has_matrix = false; int32_t morph_targets = 0, morph_at = -1; BaseState base_state = BaseState::Rest;
    std::vector<float> morph_delta, morph_w, base;
};
// what a matrix or a pose acts on: the morphed base while weights are in force, else the rest pose
inline const std::vector<float> &mesh_base(const HostMesh &m) { return !m.base.empty() ? m.base : m.rest.empty() ? m.verts : m.rest; }
// device scratch of a pass that only grows (context.cpp grow_scratch); freed by evplp_destroy
struct DeviceScratch { void *p = nullptr; size_t bytes = 0; };
struct HostTexture { int32_t w = 0, h = 0; std::vector<float> rgba; };
struct HostStats { uint64_t rays = 0; };
// host/proxy_mesh.cpp: the proxy mesh of EVPLP_FOOTPRINT_PROXY as slabs (kernels.h ProxyDev)
struct ProxyHost { std::vector<float4> slabs; std::vector<float> hm; int32_t planes = 0; float rin = 0.f, rout = 0.f; };
void default_splat_proxy(std::vector<float> &verts, std::vector<int32_t> &tris);
bool build_proxy_slabs(const float *verts, int32_t nverts, const int32_t *tris, int32_t ntris, ProxyHost *out, std::string *why);
// evplp_frame_error (context.cpp): the error figures from per-IMAGE-row partials, added in image row order (rows with held[y] = 0 are
// skipped): out = { sum num / npix, sum rel / npix, sum rel over kept pixels / kept pixels (0 when none) }.  The one place the rows are
// added, for a context and for a group alike: the figure is then a function of the frame alone, whatever holds which rows.
void sum_row_errors(const std::vector<RowError> &rows, const std::vector<char> &held, double npix, double out[3]);
}

struct evplp_context;
// every entry point of the C ABI that takes a context: a call from another thread than the group's worker waits for the worker first
#define CTX_CHECK(ctx) do { if (!(ctx)) return EVPLP_ERR_INVALID; if ((ctx)->quiesce && std::this_thread::get_id() != (ctx)->worker_tid) (ctx)->quiesce((ctx)->quiesce_arg); } while (0)
#define HIP_TRY(ctx, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { (ctx)->set_error("%s failed: %s", #expr, hipGetErrorString(e_)); return EVPLP_ERR_HIP; } } while (0)
namespace evplp {
// what context.cpp and scene_motion.cpp share.  context.cpp: a mesh's triangles flattened, the figures of a mesh, of the light and of the
// scene (a refit's are a fresh build's), and evplp_build_accel with the rebuild of a refit policy (policy_builder >= 0: that builder).
// (hidden: between the library's own units, no names of its dynamic symbol table)
#pragma GCC visibility push(hidden)
void flatten_mesh(const HostMesh &m, const std::vector<float> &from, float *o);
void mesh_figures(HostMesh &m, const float *flat, char *has_area);
void light_figures(evplp_context *c, const float *flat, std::vector<float> &cdf);
float scene_fold(evplp_context *c);
int build_accel(evplp_context *c, int policy_builder);
// scene_motion.cpp: the tree's SAH cost into out[5] (waits), and the release of everything that unit makes for a device scene
int measure_cost(evplp_context *c, double out[5]);
void release_scene_motion(evplp_context *c);
// context.cpp's grow_scratch for the library's other units; ray_query.cpp: the release of what the queries made (evplp_destroy)
hipError_t grow_scratch_of(evplp_context *ctx, DeviceScratch &s, size_t need);
void release_ray_query(evplp_context *c);
void release_probe_gather(evplp_context *c);         // probe_gather.cpp: likewise
void release_surface_gather(evplp_context *c);       // surface_gather.cpp: likewise
void release_lightmap(evplp_context *c);             // lightmap.cpp: likewise
#pragma GCC visibility pop
// what evplp_trace_closest / evplp_trace_occluded refuse (ray_query.cpp; name: the entry point), for the group's caller thread as well
bool ray_query_check(evplp_context *c, const char *name, const void *rays, int32_t n, int32_t filter, int32_t flags, const void *out);
// what evplp_update_mesh / evplp_refit_accel refuse (scene_motion.cpp), for the group's caller thread as well: false and the reason in c's error
bool update_mesh_check(evplp_context *c, int32_t mesh, const float *vertices, int32_t nverts);
bool transform_mesh_check(evplp_context *c, int32_t mesh, const float *m);
bool set_mesh_skin_check(evplp_context *c, int32_t mesh, int32_t nbones, const int32_t *bone_index, const float *weight, int32_t nverts);
bool pose_mesh_check(evplp_context *c, int32_t mesh, const float *bone_matrices, int32_t nbones, std::vector<float> *posed_out = nullptr);   // (posed_out: the posed positions)
int pose_mesh_apply(evplp_context *c, int32_t mesh, const float *bone_matrices, int32_t nbones, const float *posed);   // (behind the check, with its positions)
// (evplp_set_mesh_morph / evplp_morph_mesh; moved_out: the positions under the weights and whatever moves the mesh, base_out: the morphed base)
bool set_mesh_morph_check(evplp_context *c, int32_t mesh, int32_t ntargets, const float *deltas, int32_t nverts);
bool morph_mesh_check(evplp_context *c, int32_t mesh, const float *weights, int32_t ntargets, std::vector<float> *base_out = nullptr, std::vector<float> *moved_out = nullptr);
int morph_mesh_apply(evplp_context *c, int32_t mesh, const float *weights, int32_t ntargets, const float *base, const float *moved);    // (behind the check, with its positions)
bool refit_check(evplp_context *c);
// what evplp_accel_quality / evplp_set_refit_policy refuse without touching a device (name: the entry point, for the message)
bool accel_quality_check(evplp_context *c, const char *name);
bool refit_policy_check(evplp_context *c, double max_cost_ratio, int32_t rebuild_builder);
// what evplp_optimize_accel / evplp_set_refit_rotations refuse, likewise
bool optimize_accel_check(evplp_context *c, const char *name, int32_t passes);
bool refit_rotations_check(evplp_context *c, const char *name, int32_t passes);
// evplp_noise_* (context.cpp), for the group's workers as well
NoisePlanes noise_planes(const evplp_context *c);
NoiseMoments noise_moments_of(const evplp_context *c);           // a context's own moments (S = c_prev - c_start)
size_t noise_bytes(const evplp_context *c);                      // the NoisePlanes allocation
// the per-row figures of the moments m (K iterations in B folds) against the composite in d_rgb, to c->noise_rows (waits for them)
int noise_rows(evplp_context *c, const NoiseMoments &m, const float4 *light, double K, double B, float scale, float ls, int32_t mask_emitter);
// the variance image of the moments m into d_rgb (stream order)
int noise_variance_to_device(evplp_context *c, const NoiseMoments &m, double K, double B, float scale);
// evplp_adaptive_tiles' map of this context's tiles written into out [ceil(H / 8)][ceil(W / 8)] (rows from the bottom); other tiles untouched
void adaptive_tiles_into(const evplp_context *c, int32_t *out);
// budget mode: the own tiles' budgets / per-tile noise figures into a whole-image array (the other tiles are left as they are: a group's
// ranks fill one array); set_budgets checks nothing but takes the own tiles from the array
void adaptive_budgets_into(const evplp_context *c, int32_t *out);
int adaptive_tile_noise_into(evplp_context *c, float scale, float ls, int32_t mask_emitter, double *out);
// evplp_denoise (context.cpp), for the group's workers as well.  The parameters with the defaults filled in, checked: false and the reason in
// why when they are refused.
struct DenoiseSettings { int32_t levels; float sigma_l, sigma_n, sigma_x; };
bool denoise_settings(const evplp_denoise_params *p, DenoiseSettings *out, char *why, size_t cap);
// the variance image in d_rgb kept in d_dn_var (stream order)
int denoise_keep_variance(evplp_context *c);
// the composite in d_rgb, the kept variance and the given guides / light plane of this context's planes -> d_dn_pack (stream order)
int denoise_prepare(evplp_context *c, const float4 *pos, const float4 *nrm, const float4 *dif, const float4 *phg, const float4 *light);
// the a-trous passes and the remodulation over a frame of W x rows packed pixels on this context's device -> out_rgb (device, 3 floats per
// pixel; stream order).  radius: the scene's bounding-sphere radius
int denoise_filter(evplp_context *c, const DenoisePixel *frame, int rows, const DenoiseSettings &ds, float radius, float *out_rgb);
// evplp_denoise_temporal (context.cpp), for the group's workers as well.  The parameters with the defaults filled in, checked like
// denoise_settings.
struct TemporalSettings { int32_t max_history; float normal_cos; };
bool temporal_settings(const evplp_temporal_params *p, TemporalSettings *out, char *why, size_t cap);
// what the call refuses on one context beyond evplp_denoise's refusals (name: the entry point): false and the reason in c's error
bool temporal_check(evplp_context *c, const char *name, bool needs_primary);
int temporal_enable(evplp_context *c, int32_t on);
// the previous-pose array follows the scene's triangle count: another count makes it anew and forgets the history (waits then)
int temporal_pose_array(evplp_context *c);
// this context's hits evaluated on the previous pose -> d_tp_prev (stream order; needs tp_frames > 0)
int temporal_prev_pose(evplp_context *c);
// the accumulation stage over a frame of W x rows packed pixels with the previous-pose texels `prev` of the same pixels, on the context that
// filters (stream order): frame[i].u becomes the accumulated (u, s), the other history becomes the current one; counts to the device
int temporal_accumulate(evplp_context *c, DenoisePixel *frame, const TemporalPrev *prev, int rows, const DenoiseSettings &ds, const TemporalSettings &ts, float radius);
// the end of a successful call: pose and camera become the previous ones (stream order)
int temporal_snapshot(evplp_context *c);
// the last call's counts (waits)
int temporal_info(evplp_context *c, evplp_temporal_info *out);
void temporal_forget(evplp_context *c);
}

struct evplp_context {
    evplp_config cfg{};
    evplp::StripDev st{};
    int32_t rows_in_image = 0;
    // dealt blocks (evplp_set_blocks): the table behind st.blocks / st.blocks_host, [cap_blocks] local -> image block, then [image blocks] image -> local block
    std::vector<int32_t> blocks_host; int32_t *d_blocks = nullptr; int32_t image_blocks = 0;
    // evplp_calibrate_blocks: while on, the gathers run their self-clocking variants and add every item's resident time to its local block's counter
    bool calibrate = false; unsigned long long *d_block_cost = nullptr;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipEvent_t ev_begin[EVPLP_PASS_COUNT] = {}, ev_end[EVPLP_PASS_COUNT] = {};
    hipEvent_t ev_dom_begin[EVPLP_PASS_COUNT] = {}, ev_dom_end[EVPLP_PASS_COUNT] = {};
    bool pass_ran[EVPLP_PASS_COUNT] = {}, pass_has_dom[EVPLP_PASS_COUNT] = {};
    // evplp_profile_passes: off = a pass records only the events the library itself waits on (the G-buffer pass's start for the
    // overlapped light tracing, the record readers', a splat's verdict); its HIP-event time is then not available (pass_timed)
    bool profile_passes = true, pass_timed[EVPLP_PASS_COUNT] = {};
    // The events around the dominant kernel of the photon splat sit BETWEEN its three dependent launches and hold them apart (18 us of a
    // 227 us pass, round 3): recorded only after evplp_profile_kernels(ctx, 1)
    bool profile_kernels = false;
    evplp::HostStats stats_host[EVPLP_PASS_COUNT];

    void *buf[EVPLP_BUF_COUNT] = {};
    bool buf_owned[EVPLP_BUF_COUNT] = {};

    // host-side scene staging (the RtScene contract, rt/rtcommon.h:816-819)
    std::vector<evplp::HostMesh> meshes;
    std::vector<evplp::Material> materials;
    std::vector<evplp::HostTexture> textures;
    int32_t light_mesh = -1;
    float light_unscaled[4] = {}, light_scaled[4] = {};
    evplp::CamBasis cam{}; evplp_camera cam_in{};
    bool camera_set = false, accel_built = false;
    float bounding_radius = 0.f, total_area = 0.f, light_area = 0.f;
    float light_box_lo[3] = {}, light_box_hi[3] = {};     // the light's triangles, unpadded (sc.light_lo / light_hi: padded by the scene's size)
    int32_t accel_nodes = 0, accel_leaves = 0, accel_depth = 0, accel_builder_used = -1; float accel_build_ms = 0.f;

    // Moving vertices (scene_motion.cpp).  mesh_dirty[m]: how mesh m's vertices changed since the device scene was made (scene_dirty: any of
    // them did; every pass then refuses).  tri_dropped[t]: original triangle t had no area at the build and so has no leaf slot.  The rest is
    // made by the first refit and freed with the scene: the level plan (evplp_refit_levels over host_nodes, the node array of the build),
    // its order on the device, 6 floats per node of scratch, a device and a pinned host staging array for the moved vertices and the light's
    // CDF ([9 * triangles + light triangles] floats; ev_refit_staged: the last refit's copies have left the pinned one).
    // The first transform makes d_rest (the rest pose, 9 floats per triangle of
    // the scene; a mesh's part is filled at its first transform) and the descriptor table of a refit's one transform launch, pinned and on
    // the device ([meshes] TransformDesc each; ev_refit_staged guards the pinned one); both are freed with the scene.
    std::vector<evplp::MeshDirty> mesh_dirty; std::vector<char> tri_dropped; bool scene_dirty = false;
    float *d_rest = nullptr; evplp::TransformDesc *d_xform = nullptr, *h_xform = nullptr;
    // The first refit with a posed mesh (and the first after the set of skinned meshes changed: skin_stale)
    // lays the skinned meshes' corner skins out one behind the other in d_skin (skin_cap corners, 24 B each; a mesh's part goes up at its first
    // posed refit, from skin_upload, which the stream may read until ev_refit_staged) and sizes, for the bones of all skinned meshes together
    // (bone_cap matrices), the refit's palette array on the device and in pinned host memory, and the descriptor table of the one skin launch
    // likewise ([meshes] SkinDesc each).  All freed with the scene; a context that never poses allocates none of it.
    evplp::CornerSkin *d_skin = nullptr; int32_t skin_cap = 0, bone_cap = 0; bool skin_stale = true; std::vector<evplp::CornerSkin> skin_upload;
    float *d_bones = nullptr, *h_bones = nullptr; evplp::SkinDesc *d_sdesc = nullptr, *h_sdesc = nullptr;
    // (MeshDirty::Matrix and Pose stand for a mesh under morph weights as well.)  The first refit
    // with a mesh under weights (and the first after the set of meshes with targets changed: morph_stale) lays those meshes' corner deltas out one
    // behind the other in d_morph (morph_cap float3; a mesh's part goes up at its first morphed refit, from morph_upload, which the stream may
    // read until ev_refit_staged) and sizes the refit's weight array (weight_cap floats) and the descriptor table of the one morph launch
    // ([meshes] MorphDesc each), on the device and in pinned host memory.  d_base: a copy of d_rest in which the part of a mesh under weights
    // AND a matrix or a pose holds its morphed base; made by the first refit with such a mesh, kept in step with d_rest, and from then on
    // what the transform and the skin launch read.  All freed with the scene; a context that never morphs allocates none of it.
    float *d_morph = nullptr, *d_base = nullptr, *d_mweights = nullptr, *h_mweights = nullptr; evplp::MorphDesc *d_mdesc = nullptr, *h_mdesc = nullptr;
    int64_t morph_cap = 0; int32_t weight_cap = 0; bool morph_stale = true; std::vector<float> morph_upload;
    std::vector<evplp::BvhNode> host_nodes; std::vector<int32_t> refit_level_begin; int32_t refit_levels = 0;
    int32_t *d_refit_order = nullptr; float *d_refit_boxes = nullptr, *d_refit_stage = nullptr, *h_refit_stage = nullptr;
    hipEvent_t ev_refit_staged = nullptr, ev_refit[5] = {}; bool refit_timed = false, refit_stages_timed = false;
    int32_t refit_count = 0, scene_tris = 0; float accel_pad = 0.f;
    // evplp_accel_quality / evplp_set_refit_policy.  The plan is the refit's (refit_reached nodes in its order, refit_leaf_refs leaf references
    // among them); the kernel's output and its pinned host copy (1 + 3 * ceil(reached / 256) doubles each) are made by the first measurement
    // and freed with the scene.  built_cost: the first measurement since the last evplp_build_accel (0: none yet).
    int32_t refit_reached = 0, refit_leaf_refs = 0;
    double *d_cost = nullptr, *h_cost = nullptr; hipEvent_t ev_cost[2] = {}; bool cost_timed = false;
    double built_cost = 0.0, policy_ratio = 0.0; bool built_cost_known = false;
    int32_t policy_builder = -1, refits_since_build = 0, policy_rebuilds = 0, last_action = 0;
    // evplp_optimize_accel / evplp_set_refit_rotations.  refit_height: the plan's level per node, kept on the host from refit_prepare.  The
    // first call that asks for rotations uploads it and makes the sweep's scratch -- d_rotate: [3][nodes] ints, the level, the rotations
    // taken below a node in a pass, its four-wide stack need -- and the root's { rotations, need } per pass on the device and in pinned host
    // memory ([2 * 8] ints each); all freed with the scene.  rotate_passes: the refit's own passes (0: off, the default).
    std::vector<int32_t> refit_height; int32_t *d_rotate = nullptr, *d_rotate_out = nullptr, *h_rotate_out = nullptr;
    int32_t rotate_passes = 0, rotations_since_build = 0, rotations_last = 0, rotations_pass[8] = {};

    evplp::SceneDev sc{};
    evplp_record *d_vpls = nullptr; uint32_t *d_vpl_src = nullptr;
    uint32_t *d_scalars = nullptr;           // [0] usable VPL count, [8] splat overflow
    evplp::PassCounters *d_counters = nullptr;
    float *d_rgb = nullptr;
    // gather workspace (DeviceScratch: made by the first pass that needs it, so path-tracing / photon-only contexts never pay for it; it only grows)
    evplp::DeviceScratch partial;              // [groups][local_rows * W] float4 per-item partial sums
    evplp::DeviceScratch lt_overflow;          // light tracing: the walk stack beyond its LDS entries (kernels.h)
    char *d_primary_cuts = nullptr; bool primary_cuts_valid = false;   // the eye's entry cuts, one slot per tile group, rebuilt when the camera or the tree changes
    evplp::DeviceScratch cuts;                 // gathers: entry cuts of every (tile group, VPL) of a band (kernels.h CutArgs)
    evplp::DeviceScratch vsl_masks;            // VSL gather: lit masks + per-item ray counts of one launch (kernels.h GatherArgs)
    size_t cut_cap = 0, mask_cap = 0;          // bounds of cuts and vsl_masks, in bytes: EVPLP_CUT_BYTES / EVPLP_MASK_BYTES, else evplp_config, else the defaults (evplp_create)

    // splat workspace
    int32_t tiles_x = 0, tiles_y = 0; uint32_t bin_stride = 0, last_bin_entries = 0, last_bin_max = 0;   // bin_stride: slots per tile bin
    // overlap_light_tracing (evplp_config): light tracing on aux_stream, behind ev_records_read (recorded after every pass that reads
    // the record buffer), in front of whatever the main stream is given next (it waits for ev_light_done)
    hipStream_t aux_stream = nullptr; hipEvent_t ev_records_read = nullptr, ev_light_done = nullptr; bool light_in_flight = false;
    // ... and into a SECOND record buffer when the whole path set is traced and the library owns the records (nobody holds a pointer
    // to them): the call flips EVPLP_BUF_RECORDS to the buffer being written, so the light paths of iteration i + 1 do not wait for
    // the passes of iteration i that still read the other one (config #4: light tracing is the long pole and becomes a pipeline)
    void *records_back = nullptr; hipEvent_t ev_back_read = nullptr; bool records_exposed = false;
    // ... and the four G-buffer planes + the tile boxes likewise: evplp_primary writes the set the pending splat does not read, and it
    // is the next evplp_splat_photons call (by then that splat has long finished) that waits for its verdict
    void *gbuf_back[4] = { nullptr, nullptr, nullptr, nullptr }; float4 *d_tile_box_back = nullptr; bool gbuf_exposed = false;
    bool gbuf_pos_exposed = false;             // the caller holds a device pointer to the position plane (buffer_info / bind_buffer): it may write it unseen
    bool tile_box_valid = false;               // d_tile_box describes the current G-buffer (written by evplp_primary; any other way in clears it)
    int32_t num_bin_groups = 0, bucket_w_log2 = 0, bucket_h_log2 = 0, buckets_x = 0, num_buckets = 0;   // two-level binning (kernels.h)
    uint32_t *d_seg = nullptr, *d_big_list = nullptr, *d_big_count = nullptr; uint16_t *d_seg_off = nullptr;
    uint32_t *d_tile_cursor = nullptr, *d_bin_items = nullptr, *d_bin_items_tmp = nullptr;
    float4 *d_compact = nullptr; float4 *d_tile_box = nullptr; uint32_t *d_tile_pairs = nullptr; uint32_t *d_summary = nullptr;
    // EVPLP_FOOTPRINT_PROXY: the proxy mesh as slabs on the device (evplp_set_splat_proxy; the generated icosphere on first use)
    float4 *d_proxy_slabs = nullptr; float *d_proxy_hm = nullptr; int32_t proxy_count = 0; float proxy_rin = 0.f, proxy_rout = 0.f;
    uint32_t *d_tile_frags = nullptr; bool last_splat_proxy = false;
    // The bin sizes of a splat are known only on the device.  The pass is enqueued completely (fill and tiles kernels do
    // nothing when the bins overflowed); the summary arrives in pinned host memory behind ev_summary and is looked at by the
    // NEXT call on the context (settle_splat): no host round trip, no GPU bubble inside the pass.
    // MIXED tile launches of the photon splat (kernels.h SplatArgs): heavy list + per-tile flags; EVPLP_TILE_MIXED=0 keeps the pure variants
    uint32_t *d_heavy_list = nullptr; uint8_t *d_tile_flags = nullptr; uint32_t heavy_cap = 0, heavy_threshold = 256, mixed_trigger = 512; int env_tile_mixed = 1;
    uint32_t *h_summary = nullptr;            // pinned, 4 words per pending pass: [0] bin entries, [1] fullest bin, [2] overflow (slots the fullest bin needed)
    // Up to two passes wait for their verdict (oldest first).  One is the rule: every entry point settles it.  With
    // overlap_light_tracing a second may be in flight: evplp_splat_photons only LOOKS whether the previous one is known yet, and
    // evplp_primary / evplp_trace_light_paths wait for a pending splat only if they are about to overwrite what it read (by then
    // it is two passes old and long finished) -- the host then runs a whole iteration ahead of the GPU.
    struct PendingSplat { evplp::SplatArgs args; hipEvent_t ev = nullptr; uint32_t *h = nullptr; };
    PendingSplat pend[2];
    int npend = 0;

    // Test / developer overrides, read ONCE by evplp_create (never in a pass): EVPLP_BVH_BUILDER (every suite under every builder),
    // EVPLP_BIN_STRIDE (forces the photon-bin overflow path), EVPLP_GATHER_K, EVPLP_TILE_BLOCK_LOG2.  -1 / 0 = not set.  (EVPLP_CUT_BYTES and
    // EVPLP_MASK_BYTES -- tests: they force the gather's band and group-range paths -- are resolved there into cut_cap / mask_cap.)
    int32_t env_ploc_radius = 0, env_ploc_iterations = -1;                                         // EVPLP_PLOC_RADIUS, EVPLP_PLOC_ITERATIONS (0 / -1: not set)
    int32_t env_bvh_builder = -1, env_gather_k = 0, env_tile_block_log2 = -1, env_cuts = -1;      // env_cuts: EVPLP_CUTS=0 walks from the root
    int32_t env_item_deal = -1;                // EVPLP_ITEM_DEAL: 0 tiles dealt to XCDs, 1 a tile's items over all XCDs (default: by launch size)
    int32_t env_split_min = 0;                 // EVPLP_SPLIT_MIN: fullest bin from which the splat's tile kernel runs four waves per tile

    // A context that belongs to an evplp_group is driven by that rank's worker thread (group.cpp).  A call from any other thread -- the
    // caller reading statistics or buffers through evplp_group_context -- first waits until the worker has nothing queued for it.
    void (*quiesce)(void *) = nullptr; void *quiesce_arg = nullptr; std::thread::id worker_tid{};

    // evplp_set_error_reference: the WHOLE reference image (rows top to bottom, 3 floats per pixel) and the mask as one keep byte per pixel
    // (null: every pixel is kept), so that a new block table needs no new upload; evplp_frame_error's per-row partials, [local_rows]
    float *d_err_ref = nullptr; uint8_t *d_err_keep = nullptr;
    evplp::RowError *d_err_rows = nullptr; std::vector<evplp::RowError> err_rows;
    // evplp_noise_track: the moments (kernels.h NoisePlanes, null: tracking is off), the keep byte of every IMAGE pixel (null: every pixel
    // is kept), evplp_noise_estimate's per-row partials [local_rows]; noise_k = K (iterations folded), noise_b = B (folds)
    char *d_noise = nullptr; size_t noise_stride = 0; uint8_t *d_noise_keep = nullptr;
    evplp::RowError *d_noise_rows = nullptr; std::vector<evplp::RowError> noise_rows;
    int64_t noise_k = 0, noise_b = 0;
    // evplp_adaptive_*: adapt_n = N, the accumulating gather and path-tracing calls since the accumulators were last cleared (counted whether adaptivity is on
    // or not); the tile records [tiles_x * tiles_y] (kernels.h AdaptTiles; null: adaptivity is off), their host copy (they change only in
    // evplp_adaptive_retire and at a clear), the retired pixels' snapshot of VPL_ACCUM [W * local_rows]; adapt_last: tiles retired by the
    // last evplp_adaptive_retire (the group's workers leave it here)
    int64_t adapt_n = 0; int4 *d_adapt_tiles = nullptr; float4 *d_adapt_snap = nullptr; std::vector<int4> adapt_tiles; int32_t adapt_last = 0;
    bool adapt_pt = false;          // evplp_adaptive_enable_pt: evplp_path_trace owns the retirement (the gathers are refused)
    // evplp_path_trace_batch: the staging slots of one chunk (kernels.h PtBatchChunk; allocated on the first call, bounded by pt_batch_cap --
    // evplp_path_trace_batch_scratch), first [tiles + 1] and the item table (uint32 per item), which only grows
    evplp::DeviceScratch pt_batch, pt_table; uint64_t pt_batch_cap = 1ull << 30;
    int32_t *d_pt_first = nullptr;
    // budget mode (evplp_adaptive_enable_pt(ctx, 2)): adapt_pt is set too; the records' host copy follows the device's in every field (a call
    // adds s_t to n_t, a fold closes K_t and B_t: both are functions of the records alone); evplp_adaptive_tile_noise's per-tile doubles [tiles]
    bool adapt_budget = false; double *d_tile_noise = nullptr;
    // gather budget mode (evplp_adaptive_enable(ctx, 2)): adapt_budget is set, adapt_pt is not.  Tile t takes call m of the accumulating gathers
    // iff gather_tile_takes(record, m % S, S) (kernels.h); adapt_m restarts at set_budgets, at a new window, at a clear.  d_adapt_mask: the
    // per-call view of the records the gather kernels read [tiles].  splat_n: photon splats since the last clear (the mode has no place for them)
    bool adapt_gather_budget = false; int32_t adapt_window = 16; int64_t adapt_m = 0; int4 *d_adapt_mask = nullptr; int64_t splat_n = 0;
    // evplp_denoise: the variance image [W * local_rows][3], the packed pixels of the planes [W * local_rows] (kernels.h DenoisePixel), and
    // the two (u, s) planes of the a-trous passes [2][dn_u_px] (the frame the context filters: its planes, or a group's whole image on rank 0);
    // allocated on the first call, kept until evplp_destroy
    float *d_dn_var = nullptr; evplp::DenoisePixel *d_dn_pack = nullptr; float4 *d_dn_u = nullptr; size_t dn_u_px = 0;
    // evplp_primary's jitter and light flags of its last call (evplp_path_trace_batch ends with one), for prev_pose_kernel to repeat that walk;
    // primary_current: that pass wrote the G-buffer in memory and nothing has touched the tree or the position plane since (a build, a refit,
    // evplp_upload / evplp_bind_buffer of EVPLP_BUF_GBUF_POSITION clear it)
    float primary_jitter[2] = {}; int32_t primary_flags = 0; bool primary_current = false;
    // evplp_temporal_enable (tp_on): the previous pose [9 * tp_tris] floats and the previous-pose texels of the planes [W * local_rows]
    // (kernels.h TemporalPrev), both made by the enable; the camera of the previous call.  The context that filters also holds the two
    // histories [2][3][tp_hist_px] float4 (tp_cur: the one the last call wrote), the stage's counts per workgroup, and -- a group's rank 0 under
    // strips -- the assembled previous-pose texels of the frame; made by its first call.  tp_frames: successful calls since the last reset
    // (0: the next call is a first call).  All released by evplp_temporal_enable(ctx, 0) and evplp_destroy.
    bool tp_on = false; float *d_tp_prev_v = nullptr; int32_t tp_tris = 0; evplp::TemporalPrev *d_tp_prev = nullptr, *d_tp_prev_frame = nullptr;
    evplp::CamBasis tp_prev_cam{}; float4 *d_tp_hist = nullptr; size_t tp_hist_px = 0; int tp_cur = 0; int32_t tp_frames = 0;
    uint4 *d_tp_counts = nullptr; int tp_count_slots = 0;           // (one slot per workgroup of the stage's last launch)
    // evplp_trace_closest / evplp_trace_occluded (ray_query.cpp), all for ONE launch of kQueryChunk rays.  The host forms' staging: rays
    // then results, 48 B per ray, on the device and in pinned host memory (made by the first host-form call).  The ordering pass's keys and
    // indices, unsorted and sorted, 16 B per ray, then the radix sort's workspace (made by the first call with EVPLP_QUERY_ORDER).
    evplp::DeviceScratch query_stage, query_sort; char *h_query_stage = nullptr; size_t query_sort_temp = 0;
    // evplp_gather_probes (probe_gather.cpp), all for ONE launch of kProbeChunk probes.  The slices' partial sums, 112 B per probe of a chunk
    // and slice of the record slots (made by the first call, grown by a call with more slots).  The host form's staging: positions then
    // results, 124 B per probe, on the device and in pinned host memory (made by the first host-form call).
    evplp::DeviceScratch probe_partial, probe_stage; char *h_probe_stage = nullptr;
    // evplp_gather_surface (surface_gather.cpp): the slices' partial sums and the photon half of ONE launch of kSurfaceChunk points; the photon grid of
    // one call (keys, slots, bucket starts, compact records, the sort's workspace: sized by the record slots); the host form's staging, 108 B per point.
    evplp::DeviceScratch surface_partial, surface_grid, surface_stage; char *h_surface_stage = nullptr;
    // evplp_gather_surface_progressive / evplp_surface_resolve (surface_gather.cpp): the reduced VPL half of ONE launch of kSurfaceChunk points
    // (32 B per point), and the host forms' staging, 156 B per point (point, eye, state: the resolve's states and results fit it).
    evplp::DeviceScratch surface_prog_lights, surface_prog_stage; char *h_surface_prog_stage = nullptr;
    // evplp_gather_surface_knn (surface_gather.cpp): the selected squared radius of every point of a device-form batch or of a host-form chunk, 4 B each.
    evplp::DeviceScratch surface_knn_rk2;
    // evplp_surface_points / evplp_lightmap_samples / evplp_bake_lightmap (lightmap.cpp).  The host forms' staging of ONE chunk of kQueryChunk
    // hits (hit, eye, point: 92 B each; a band's hits fit it), on the device and pinned; the selection's set-up triangles (32 B each, and 24 B
    // each of uploaded uvs); a band's tile arrays (counts, offsets, cursors, the scan's workspace) and its pinned pair count; the tiles'
    // triangle lists (4 B per (triangle, tile) pair of the fullest band so far: the one array that follows the scene's overlap); the bake's
    // hits, points and results of one band (112 B per sample); the bake's atlas buffers (32 B per texel: the host form's, the gutter's second).
    evplp::DeviceScratch lm_stage, lm_tris, lm_band, lm_pairs, lm_bake, lm_atlas; char *h_lm_stage = nullptr; uint32_t *h_lm_count = nullptr;

    char error[512] = "";
    void set_error(const char *fmt, ...);
};

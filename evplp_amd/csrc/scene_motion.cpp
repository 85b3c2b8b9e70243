// Moving vertices (include/evplp.h): update, transform, pose and morph of a mesh on the host copy, evplp_refit_accel that takes them to the
// device and refits the tree there, the tree's SAH cost with the rebuild policy, and tree rotations.  context.cpp builds the scene
// (build_accel) and frees it; what the two units share is declared in context.hpp.
#include "device_arrays.hpp"
#include "host/morph.hpp"
#include "host/skin.hpp"
#include <algorithm>
#include <array>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

using namespace evplp;
static_assert(offsetof(BvhNode, c0) == 48 && offsetof(BvhNode, c1) == 52, "host/refit_levels.cpp reads the child references at these offsets");

// ---------------------------------------------------------------------------------- the arrays this unit makes for a device scene
// The sets of this unit (the sizes matter to alloc_arrays alone): made by the first transform, pose or morph of a scene; the first refit or
// measurement of a tree; the first call that asks for rotations; the first posed refit; the first morphed refit, and the first with a
// mesh under weights that a matrix or a pose moves too; the first measurement.  All are released with the scene.
template <size_t N> using ArraySet = std::array<ArrayWish, N>;
static ArraySet<3> rest_arrays(evplp_context *c, size_t tris = 0, size_t nm = 0) { return {{ on_device(c->d_rest, 9 * tris), on_device(c->d_xform, nm), pinned(c->h_xform, nm) }}; }
static ArraySet<4> plan_arrays(evplp_context *c, size_t nn = 0, size_t stage = 0) { return {{ on_device(c->d_refit_order, nn), on_device(c->d_refit_boxes, 6 * nn), on_device(c->d_refit_stage, stage), pinned(c->h_refit_stage, stage) }}; }
static ArraySet<3> rotate_arrays(evplp_context *c, size_t nn = 0) { return {{ on_device(c->d_rotate, 3 * nn), on_device(c->d_rotate_out, 16), pinned(c->h_rotate_out, 16) }}; }
static ArraySet<5> skin_arrays(evplp_context *c, size_t corners = 0, size_t bones = 0, size_t nm = 0) { return {{ on_device(c->d_skin, corners), on_device(c->d_bones, 12 * bones), pinned(c->h_bones, 12 * bones), on_device(c->d_sdesc, nm), pinned(c->h_sdesc, nm) }}; }
static ArraySet<5> morph_arrays(evplp_context *c, size_t vectors = 0, size_t weights = 0, size_t nm = 0) { return {{ on_device(c->d_morph, 3 * vectors), on_device(c->d_mweights, weights), pinned(c->h_mweights, weights), on_device(c->d_mdesc, nm), pinned(c->h_mdesc, nm) }}; }
static ArraySet<1> base_array(evplp_context *c, size_t tris = 0) { return {{ on_device(c->d_base, 9 * tris) }}; }
static ArraySet<2> cost_arrays(evplp_context *c, size_t n = 0) { return {{ on_device(c->d_cost, n), pinned(c->h_cost, n) }}; }
static void release_skin(evplp_context *c) { release_arrays(skin_arrays(c)); c->skin_cap = c->bone_cap = 0; }
static void release_morph(evplp_context *c) { release_arrays(morph_arrays(c)); c->morph_cap = 0; c->weight_cap = 0; }

namespace evplp {
// what of this unit belongs to the device scene (free_scene_device): the host keeps every rest pose, skin and target
void release_scene_motion(evplp_context *c) {
    release_arrays(plan_arrays(c));
    c->refit_levels = 0; c->refit_level_begin.clear(); std::vector<BvhNode>().swap(c->host_nodes);
    release_arrays(cost_arrays(c)); c->refit_reached = c->refit_leaf_refs = 0;
    release_arrays(rest_arrays(c));
    release_skin(c); c->skin_stale = true;
    release_morph(c); release_arrays(base_array(c)); c->morph_stale = true;
    for (HostMesh &m : c->meshes) { m.rest_state = RestState::Absent; m.skin_at = -1; m.morph_at = -1; m.base_state = BaseState::Rest; }
    release_arrays(rotate_arrays(c)); std::vector<int32_t>().swap(c->refit_height);
}

// ---------------------------------------------------------------------------------- moving vertices: update, transform, pose, morph
// what every call that names a mesh refuses first
static bool mesh_arg_check(evplp_context *c, const char *name, int32_t mesh, bool need_built) {
    if (need_built && !c->accel_built) { c->set_error("%s: scene not built (evplp_build_accel)", name); return false; }
    if (mesh < 0 || mesh >= (int32_t)c->meshes.size()) { c->set_error("%s: mesh %d out of range (%zu meshes)", name, mesh, c->meshes.size()); return false; }
    return true;
}
// evplp_update_mesh's refusals, for the group's caller thread as well (false: the reason is in c's error)
bool update_mesh_check(evplp_context *c, int32_t mesh, const float *vertices, int32_t nverts) {
    if (!mesh_arg_check(c, "evplp_update_mesh", mesh, true)) return false;
    if (!vertices) { c->set_error("evplp_update_mesh: null vertices"); return false; }
    const size_t have = c->meshes[(size_t)mesh].verts.size() / 3;
    if (nverts < 0 || (size_t)nverts != have) { c->set_error("evplp_update_mesh: mesh %d has %zu vertices, not %d (the topology stays)", mesh, have, nverts); return false; }
    for (size_t i = 0; i < 3 * have; i++) if (!std::isfinite(vertices[i])) { c->set_error("evplp_update_mesh: vertex %zu of mesh %d is not finite", i / 3, mesh); return false; }
    return true;
}
// evplp_transform_mesh's refusals, likewise.  The transformed coordinates are checked on the host copy's rest pose, by the function that
// will move it: a matrix that overflows a coordinate is refused here, not rendered.
bool transform_mesh_check(evplp_context *c, int32_t mesh, const float *matrix) {
    if (!mesh_arg_check(c, "evplp_transform_mesh", mesh, true)) return false;
    if (!matrix) { c->set_error("evplp_transform_mesh: null matrix"); return false; }
    for (int i = 0; i < 12; i++) if (!std::isfinite(matrix[i])) { c->set_error("evplp_transform_mesh: matrix entry %d is not finite", i); return false; }
    const HostMesh &m = c->meshes[(size_t)mesh];
    const std::vector<float> &rest = mesh_base(m);             // (the morphed base while morph weights are in force)
    for (size_t v = 0; v < rest.size() / 3; v++) {
        float o[3]; transform_point(matrix, &rest[3 * v], o);
        if (!std::isfinite(o[0]) || !std::isfinite(o[1]) || !std::isfinite(o[2])) { c->set_error("evplp_transform_mesh: vertex %zu of mesh %d is not finite under the matrix", v, mesh); return false; }
    }
    return true;
}
// evplp_set_mesh_skin's and evplp_pose_mesh's refusals, likewise (the arrays' own by host/skin.cpp).  The posed coordinates are checked on the
// host copy's rest pose, by the function that will move it.
bool set_mesh_skin_check(evplp_context *c, int32_t mesh, int32_t nbones, const int32_t *bone_index, const float *weight, int32_t nverts) {
    if (!mesh_arg_check(c, "evplp_set_mesh_skin", mesh, true)) return false;
    if (nbones == 0) return true;                   // (the skin is removed: the arrays are not looked at)
    const size_t have = c->meshes[(size_t)mesh].verts.size() / 3;
    if (nverts < 0 || (size_t)nverts != have) { c->set_error("evplp_set_mesh_skin: mesh %d has %zu vertices, not %d", mesh, have, nverts); return false; }
    if (!bone_index || !weight) { c->set_error("evplp_set_mesh_skin: null %s", !bone_index ? "bone_index" : "weight"); return false; }
    char why[256];
    if (!skin_arrays_ok(nbones, bone_index, weight, nverts, why, sizeof(why))) { c->set_error("evplp_set_mesh_skin: mesh %d: %s", mesh, why); return false; }
    return true;
}
bool pose_mesh_check(evplp_context *c, int32_t mesh, const float *bone_matrices, int32_t nbones, std::vector<float> *posed_out) {
    if (!mesh_arg_check(c, "evplp_pose_mesh", mesh, true)) return false;
    const HostMesh &m = c->meshes[(size_t)mesh];
    if (m.skin_bones <= 0) { c->set_error("evplp_pose_mesh: mesh %d has no skin (evplp_set_mesh_skin)", mesh); return false; }
    if (nbones != m.skin_bones) { c->set_error("evplp_pose_mesh: the skin of mesh %d has %d bones, not %d", mesh, m.skin_bones, nbones); return false; }
    char why[256];
    if (!skin_palette_ok(bone_matrices, nbones, why, sizeof(why))) { c->set_error("evplp_pose_mesh: mesh %d: %s", mesh, why); return false; }
    const std::vector<float> &rest = mesh_base(m);             // (the morphed base while morph weights are in force)
    std::vector<float> posed(rest.size());
    const int64_t bad = skin_apply(bone_matrices, m.skin_index.data(), m.skin_weight.data(), rest.data(), posed.data(), rest.size() / 3);
    if (bad >= 0) { c->set_error("evplp_pose_mesh: vertex %lld of mesh %d is not finite under the palette", (long long)bad, mesh); return false; }
    if (posed_out) posed_out->swap(posed);          // (the context's own call keeps the positions the check has just made)
    return true;
}
// evplp_set_mesh_morph's and evplp_morph_mesh's refusals, likewise (the arrays' own, and every loop over the vertices, by host/morph.cpp).  The
// final coordinates -- the morphed base under the matrix or the pose in force -- are checked on the host copy, by the functions that move it.
bool set_mesh_morph_check(evplp_context *c, int32_t mesh, int32_t ntargets, const float *deltas, int32_t nverts) {
    if (!mesh_arg_check(c, "evplp_set_mesh_morph", mesh, true)) return false;
    const HostMesh &m = c->meshes[(size_t)mesh];
    if (!m.morph_w.empty()) { c->set_error("evplp_set_mesh_morph: mesh %d has morph weights in force: take them away first (evplp_morph_mesh(ctx, mesh, NULL, 0))", mesh); return false; }
    if (ntargets == 0) return true;                 // (the targets are removed: the array is not looked at)
    const size_t have = m.verts.size() / 3;
    if (nverts < 0 || (size_t)nverts != have) { c->set_error("evplp_set_mesh_morph: mesh %d has %zu vertices, not %d", mesh, have, nverts); return false; }
    if (!deltas) { c->set_error("evplp_set_mesh_morph: null deltas"); return false; }
    char why[256];
    if (!morph_deltas_ok(ntargets, deltas, nverts, why, sizeof(why))) { c->set_error("evplp_set_mesh_morph: mesh %d: %s", mesh, why); return false; }
    return true;
}
bool morph_mesh_check(evplp_context *c, int32_t mesh, const float *weights, int32_t ntargets, std::vector<float> *base_out, std::vector<float> *moved_out) {
    if (!mesh_arg_check(c, "evplp_morph_mesh", mesh, true)) return false;
    const HostMesh &m = c->meshes[(size_t)mesh];
    const std::vector<float> &rest = m.rest.empty() ? m.verts : m.rest;
    const size_t n = rest.size() / 3;
    std::vector<float> base, moved(rest.size());
    if (ntargets != 0 || weights) {                 // (NULL, 0 takes the weights away: the positions are the rest pose's again)
        if (m.morph_targets <= 0) { c->set_error("evplp_morph_mesh: mesh %d has no morph targets (evplp_set_mesh_morph)", mesh); return false; }
        if (ntargets != m.morph_targets) { c->set_error("evplp_morph_mesh: mesh %d has %d morph targets, not %d", mesh, m.morph_targets, ntargets); return false; }
        char why[256];
        if (!morph_weights_ok(weights, ntargets, why, sizeof(why))) { c->set_error("evplp_morph_mesh: mesh %d: %s", mesh, why); return false; }
        base.resize(rest.size());
        const int64_t bad = morph_apply(m.morph_delta.data(), weights, ntargets, rest.data(), base.data(), n);
        if (bad >= 0) { c->set_error("evplp_morph_mesh: vertex %lld of mesh %d is not finite under the weights", (long long)bad, mesh); return false; }
    } else if (m.morph_w.empty()) {                 // (none in force: nothing moves)
        if (base_out) base_out->clear(); if (moved_out) moved_out->clear();
        return true;
    }
    const int64_t bad = morph_deform(base.empty() ? rest.data() : base.data(), m.palette.empty() && m.has_matrix ? m.matrix : nullptr, m.palette.empty() ? nullptr : m.palette.data(),
                                     m.skin_index.data(), m.skin_weight.data(), moved.data(), n);
    if (bad >= 0) { c->set_error("evplp_morph_mesh: vertex %lld of mesh %d is not finite under the weights and the %s in force", (long long)bad, mesh, m.palette.empty() ? "matrix" : "pose"); return false; }
    if (base_out) base_out->swap(base);
    if (moved_out) moved_out->swap(moved);
    return true;
}
// evplp_refit_accel's refusal: a triangle the build dropped (no area) that has one now has no leaf slot to go to
bool refit_check(evplp_context *c) {
    if (!c->accel_built) { c->set_error("evplp_refit_accel: scene not built (evplp_build_accel)"); return false; }
    size_t first = 0;
    for (size_t mi = 0; mi < c->meshes.size(); first += c->meshes[mi].idx.size() / 3, mi++) {
        if (!c->scene_dirty || c->mesh_dirty[mi] == MeshDirty::Clean) continue;
        const HostMesh &m = c->meshes[mi];
        for (size_t t = 0; t < m.idx.size() / 3; t++) {
            if (!c->tri_dropped[first + t]) continue;
            float v[9];
            for (int k = 0; k < 3; k++) std::memcpy(v + 3 * k, &m.verts[3 * (size_t)m.idx[3 * t + k]], 12);
            if (tri_has_area(v)) {
                c->set_error("evplp_refit_accel: triangle %zu of mesh %zu had no area when the tree was built and has one now: it has no leaf to go to, call evplp_build_accel", t, mi);
                return false;
            }
        }
    }
    return true;
}
}
// morph weights leave the mesh (new vertices, NULL weights) or give way to others: the device's base, if it holds theirs, is stale
static void drop_morph_weights(HostMesh &m) {
    std::vector<float>().swap(m.morph_w); std::vector<float>().swap(m.base);
    if (m.base_state == BaseState::Weights) m.base_state = BaseState::StaleWeights;
}

extern "C" int evplp_update_mesh(evplp_context *c, int32_t mesh, const float *vertices, int32_t nverts) {
    CTX_CHECK(c);
    if (!evplp::update_mesh_check(c, mesh, vertices, nverts)) return EVPLP_ERR_INVALID;
    HostMesh &m = c->meshes[(size_t)mesh];
    std::memcpy(m.verts.data(), vertices, sizeof(float) * 3 * (size_t)nverts);
    std::vector<float>().swap(m.rest); m.rest_state = RestState::Absent;    // (a new rest pose: the matrix is forgotten, the device's copy is stale)
    std::vector<float>().swap(m.palette); m.has_matrix = false; // (... and so is a pose; the skin stays)
    drop_morph_weights(m);                                      // (... and so are morph weights; the targets stay)
    c->mesh_dirty[(size_t)mesh] = MeshDirty::Upload; c->scene_dirty = true;
    return EVPLP_OK;
}
extern "C" int evplp_transform_points(const float *m, const float *in, float *out, int32_t n) {
    if (!m || n < 0 || (n > 0 && (!in || !out))) return EVPLP_ERR_INVALID;
    for (int32_t i = 0; i < n; i++) { float o[3]; evplp::transform_point(m, in + 3 * (size_t)i, o); std::memcpy(out + 3 * (size_t)i, o, 12); }
    return EVPLP_OK;
}
// the first transform or pose of this scene: the rest-pose array and the two descriptor tables of the transform launch
static int rest_prepare(evplp_context *c, const char *name) {
    if (c->d_rest) return EVPLP_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    return alloc_arrays(c, rest_arrays(c, (size_t)std::max(c->scene_tris, 1), c->meshes.size()), name, "the rest pose on the device");
}
// The first move of a mesh by matrix, pose or weights (name: the entry point).  The device's copy of its rest pose is made by the refit: from
// the attributes while they still hold it (a clean mesh that has no matrix), from the host's rest pose otherwise.
static int first_move(evplp_context *c, const char *name, int32_t mesh) {
    HostMesh &m = c->meshes[(size_t)mesh];
    { const int rc = rest_prepare(c, name); if (rc) return rc; }
    if (m.rest_state == RestState::Absent) m.rest_state = (c->mesh_dirty[(size_t)mesh] == MeshDirty::Clean && m.rest.empty()) ? RestState::FromAttrs : RestState::FromHost;
    if (m.rest.empty()) m.rest = m.verts;
    return EVPLP_OK;
}
extern "C" int evplp_transform_mesh(evplp_context *c, int32_t mesh, const float *matrix) {
    CTX_CHECK(c);
    if (!evplp::transform_mesh_check(c, mesh, matrix)) return EVPLP_ERR_INVALID;
    HostMesh &m = c->meshes[(size_t)mesh];
    { const int rc = first_move(c, "evplp_transform_mesh", mesh); if (rc) return rc; }
    const std::vector<float> &from = evplp::mesh_base(m);       // (morphed first, then moved: the base while morph weights are in force)
    for (size_t v = 0; v < from.size() / 3; v++) evplp::transform_point(matrix, &from[3 * v], &m.verts[3 * v]);
    std::memcpy(m.matrix, matrix, sizeof(m.matrix)); m.has_matrix = true;
    std::vector<float>().swap(m.palette);                       // (a matrix replaces a pose)
    c->mesh_dirty[(size_t)mesh] = MeshDirty::Matrix; c->scene_dirty = true;
    return EVPLP_OK;
}

// ---- moving a mesh by bones: the skin (constant for the topology), the pose (a palette of matrices over the rest pose), and the queries a
// caller needs to build a skin for a scene the library loaded
extern "C" int evplp_set_mesh_skin(evplp_context *c, int32_t mesh, int32_t nbones, const int32_t *bone_index, const float *weight, int32_t nverts) {
    CTX_CHECK(c);
    if (!evplp::set_mesh_skin_check(c, mesh, nbones, bone_index, weight, nverts)) return EVPLP_ERR_INVALID;
    HostMesh &m = c->meshes[(size_t)mesh];
    // A pose that no refit has taken to the device yet stays what it is on the host copy: the mesh goes up by upload instead (its rest pose is kept)
    // -- and the upload overwrites the attributes, so a rest pose that was still to be taken from them comes from the host's instead
    if (c->mesh_dirty[(size_t)mesh] == MeshDirty::Pose) { c->mesh_dirty[(size_t)mesh] = MeshDirty::Upload; if (m.rest_state == RestState::FromAttrs) m.rest_state = RestState::FromHost; }
    std::vector<float>().swap(m.palette);
    m.skin_bones = nbones; m.skin_at = -1; c->skin_stale = true;
    if (nbones == 0) { std::vector<int32_t>().swap(m.skin_index); std::vector<float>().swap(m.skin_weight); return EVPLP_OK; }
    m.skin_index.assign(bone_index, bone_index + 4 * (size_t)nverts);
    m.skin_weight.assign(weight, weight + 4 * (size_t)nverts);
    return EVPLP_OK;
}
namespace evplp {
// evplp_pose_mesh behind its check: posed = the mesh's posed positions as pose_mesh_check made them (float3 per vertex).  The group checks once,
// on the caller's thread against rank 0's copy, and hands the same positions to every rank: the ranks' scenes are the same.
int pose_mesh_apply(evplp_context *c, int32_t mesh, const float *bone_matrices, int32_t nbones, const float *posed) {
    HostMesh &m = c->meshes[(size_t)mesh];
    { const int rc = first_move(c, "evplp_pose_mesh", mesh); if (rc) return rc; }
    std::memcpy(m.verts.data(), posed, sizeof(float) * m.verts.size());    // (skin_apply of the rest pose, by the check)
    m.palette.assign(bone_matrices, bone_matrices + 12 * (size_t)nbones); m.has_matrix = false;   // (a pose replaces a matrix)
    c->mesh_dirty[(size_t)mesh] = MeshDirty::Pose; c->scene_dirty = true;
    return EVPLP_OK;
}
}
extern "C" int evplp_pose_mesh(evplp_context *c, int32_t mesh, const float *bone_matrices, int32_t nbones) {
    CTX_CHECK(c);
    std::vector<float> posed;
    if (!evplp::pose_mesh_check(c, mesh, bone_matrices, nbones, &posed)) return EVPLP_ERR_INVALID;
    return evplp::pose_mesh_apply(c, mesh, bone_matrices, nbones, posed.data());
}

// ---- moving a mesh by morph targets: the targets (constant for the topology) and the weights, a state of their own beside matrix and pose:
// the weights make the mesh's base from its rest pose, and the matrix or the pose in force acts on that base (morphed first, then moved)
extern "C" int evplp_set_mesh_morph(evplp_context *c, int32_t mesh, int32_t ntargets, const float *deltas, int32_t nverts) {
    CTX_CHECK(c);
    if (!evplp::set_mesh_morph_check(c, mesh, ntargets, deltas, nverts)) return EVPLP_ERR_INVALID;
    HostMesh &m = c->meshes[(size_t)mesh];
    m.morph_targets = ntargets; m.morph_at = -1; c->morph_stale = true;
    if (ntargets == 0) std::vector<float>().swap(m.morph_delta);
    else m.morph_delta.assign(deltas, deltas + 3 * (size_t)nverts * (size_t)ntargets);
    return EVPLP_OK;
}
namespace evplp {
// evplp_morph_mesh behind its check: base / moved = the mesh's morphed base and its positions as morph_mesh_check made them (float3 per vertex;
// ntargets = 0: moved alone, the positions without weights).  The group hands every rank the same positions, as for a pose.
int morph_mesh_apply(evplp_context *c, int32_t mesh, const float *weights, int32_t ntargets, const float *base, const float *moved) {
    HostMesh &m = c->meshes[(size_t)mesh];
    const MeshDirty kind = !m.palette.empty() ? MeshDirty::Pose : m.has_matrix ? MeshDirty::Matrix : MeshDirty::Morph;
    if (ntargets == 0 && m.morph_w.empty()) return EVPLP_OK;     // (none were in force: nothing moves, nothing is dirty)
    { const int rc = first_move(c, "evplp_morph_mesh", mesh); if (rc) return rc; }
    drop_morph_weights(m);                          // (those in force till now)
    std::memcpy(m.verts.data(), moved, sizeof(float) * m.verts.size());
    c->mesh_dirty[(size_t)mesh] = kind; c->scene_dirty = true;
    // (without weights, a mesh that nothing moves any more is at its rest pose: that goes up by upload, like new vertices, and the device's rest pose stays)
    if (ntargets == 0) { if (kind == MeshDirty::Morph) c->mesh_dirty[(size_t)mesh] = MeshDirty::Upload; return EVPLP_OK; }
    m.morph_w.assign(weights, weights + ntargets);
    m.base.assign(base, base + m.verts.size());
    return EVPLP_OK;
}
}
extern "C" int evplp_morph_mesh(evplp_context *c, int32_t mesh, const float *weights, int32_t ntargets) {
    CTX_CHECK(c);
    std::vector<float> base, moved;
    if (!evplp::morph_mesh_check(c, mesh, weights, ntargets, &base, &moved)) return EVPLP_ERR_INVALID;
    return evplp::morph_mesh_apply(c, mesh, weights, ntargets, base.data(), moved.data());
}

extern "C" int evplp_mesh_count(evplp_context *c) { CTX_CHECK(c); return (int)c->meshes.size(); }
extern "C" int evplp_mesh_info(evplp_context *c, int32_t mesh, int32_t *nverts, int32_t *ntris, int32_t *material) {
    CTX_CHECK(c);
    if (!evplp::mesh_arg_check(c, "evplp_mesh_info", mesh, false)) return EVPLP_ERR_INVALID;
    const HostMesh &m = c->meshes[(size_t)mesh];
    if (nverts) *nverts = (int32_t)(m.verts.size() / 3);
    if (ntris) *ntris = (int32_t)(m.idx.size() / 3);
    if (material) *material = m.material;
    return EVPLP_OK;
}
extern "C" int evplp_mesh_vertices(evplp_context *c, int32_t mesh, int32_t which, float *out_xyz, int32_t capacity_verts) {
    CTX_CHECK(c);
    if (!evplp::mesh_arg_check(c, "evplp_mesh_vertices", mesh, false)) return EVPLP_ERR_INVALID;
    if (which < 0 || which > 2) { c->set_error("evplp_mesh_vertices: which must be 0 (current), 1 (rest pose) or 2 (morphed base), not %d", which); return EVPLP_ERR_INVALID; }
    const HostMesh &m = c->meshes[(size_t)mesh];
    // (a mesh without morph targets has no morphed base: for it `which` is what it was before there were targets, 0 or 1)
    if (which == 2 && m.morph_targets <= 0) { c->set_error("evplp_mesh_vertices: which = 2 (morphed base): mesh %d has no morph targets (evplp_set_mesh_morph); which must be 0 (current) or 1 (rest pose)", mesh); return EVPLP_ERR_INVALID; }
    const std::vector<float> &src = which == 2 ? evplp::mesh_base(m) : (which == 1 && !m.rest.empty()) ? m.rest : m.verts;
    if (!out_xyz || capacity_verts < 0 || (size_t)capacity_verts < src.size() / 3) { c->set_error("evplp_mesh_vertices: mesh %d has %zu vertices: a null destination or too small a capacity (%d)", mesh, src.size() / 3, capacity_verts); return EVPLP_ERR_INVALID; }
    std::memcpy(out_xyz, src.data(), sizeof(float) * src.size());
    return EVPLP_OK;
}

// ---------------------------------------------------------------------------------- the refit
// the level plan, the scratch and the staging arrays of a tree: made by its first refit
static int refit_prepare(evplp_context *c) {
    if (c->refit_levels > 0) return EVPLP_OK;
    const int32_t nn = c->accel_nodes;
    if (c->host_nodes.empty()) {            // (a host builder's tree: its child references come back once; the device builder's were kept)
        c->host_nodes.resize((size_t)nn);
        HIP_TRY(c, hipMemcpyAsync(c->host_nodes.data(), c->sc.nodes, sizeof(BvhNode) * (size_t)nn, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    std::vector<int32_t> height((size_t)nn), order((size_t)nn);
    c->refit_level_begin.assign((size_t)kMaxDepth + 1, 0);
    const int levels = evplp_refit_levels(c->host_nodes.data(), nn, height.data(), order.data(), c->refit_level_begin.data(), kMaxDepth);
    if (levels >= 1) {                      // (what evplp_accel_quality reports beside its sums: the reached nodes and their leaf references)
        c->refit_reached = c->refit_level_begin[(size_t)levels]; c->refit_leaf_refs = 0;
        for (int32_t k = 0; k < c->refit_reached; k++) {
            const BvhNode &f = c->host_nodes[(size_t)order[(size_t)k]];
            c->refit_leaf_refs += (f.c0 < 0 && f.c0 != kNoChild) + (f.c1 < 0 && f.c1 != kNoChild);
        }
    }
    std::vector<BvhNode>().swap(c->host_nodes);
    c->refit_height.swap(height);           // (the plan's level per node: what a rotating sweep uploads, should one ever be asked for)
    if (levels < 1) { c->set_error("evplp_refit_accel: the node array is not a tree of at most %d levels", kMaxDepth); return EVPLP_ERR_INVALID; }
    const size_t stage = 9 * (size_t)c->scene_tris + (size_t)c->sc.light_count;
    const int rc = alloc_arrays(c, plan_arrays(c, (size_t)nn, stage), "evplp_refit_accel", "plan and staging"); if (rc) return rc;
    hipError_t e = hipMemcpy(c->d_refit_order, order.data(), sizeof(int32_t) * (size_t)nn, hipMemcpyHostToDevice);
    if (e == hipSuccess && !c->ev_refit_staged) e = hipEventCreateWithFlags(&c->ev_refit_staged, hipEventDisableTiming);
    for (int i = 0; i < 5 && e == hipSuccess; i++) if (!c->ev_refit[i]) e = hipEventCreate(&c->ev_refit[i]);
    if (e != hipSuccess) { release_arrays(plan_arrays(c)); return hip_failure(c, "evplp_refit_accel", "plan and staging", e); }
    c->refit_levels = levels;
    return EVPLP_OK;
}

// ---- tree rotations inside the sweep (evplp_optimize_accel, evplp_set_refit_rotations).  The scratch of the rotating launches, made by the
// first call that asks for rotations: the plan's level per node goes up once -- a rotation keeps every parent above its children IN THE PLAN,
// so the plan, its order and these levels hold for every later pass and refit of this tree, though the levels are no tight heights any more.
static int rotate_prepare(evplp_context *c) {
    if (c->d_rotate) return EVPLP_OK;
    const size_t nn = (size_t)c->accel_nodes;
    const int rc = alloc_arrays(c, rotate_arrays(c, nn), "tree rotations", "the sweep's scratch"); if (rc) return rc;
    hipError_t e = hipMemcpy(c->d_rotate, c->refit_height.data(), sizeof(int32_t) * nn, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(c->d_rotate + nn, 0, sizeof(int32_t) * 2 * nn);
    if (e != hipSuccess) { release_arrays(rotate_arrays(c)); return hip_failure(c, "tree rotations", "the sweep's scratch", e); }
    return EVPLP_OK;
}
// `passes` sweeps, the leaves' parents first and the root last, each launch the rotating one; enqueued, none waits
static void rotate_enqueue(evplp_context *c, const RefitScene &r, float pad, int32_t passes) {
    const size_t nn = (size_t)c->accel_nodes;
    for (int32_t p = 0; p < passes; p++)
        for (int32_t l = 0; l < c->refit_levels; l++)
            refit_rotate_level(r, c->d_refit_order + c->refit_level_begin[(size_t)l], c->refit_level_begin[(size_t)l + 1] - c->refit_level_begin[(size_t)l], pad,
                               c->d_rotate, c->d_rotate + nn, c->d_rotate + 2 * nn, c->d_rotate_out + 2 * p, c->stream);
}
// after the wait: the root's { rotations, need } of every pass are in the pinned words
static void rotate_finish(evplp_context *c, int32_t passes) {
    c->rotations_last = 0;
    for (int p = 0; p < 8; p++) { c->rotations_pass[p] = p < passes ? c->h_rotate_out[2 * p] : 0; c->rotations_last += c->rotations_pass[p]; }
    c->rotations_since_build += c->rotations_last;
    c->sc.stack4_entries = c->h_rotate_out[2 * (passes - 1) + 1] + 2;   // (kernels.h takes the smaller of this and the generic bound of the depth)
}
// the tree as the refit's launches see it
static RefitScene refit_scene(const evplp_context *c) {
    RefitScene r; std::memset(&r, 0, sizeof(r));
    r.nodes = (BvhNode *)c->sc.nodes; r.nnodes = c->accel_nodes; r.leaves = (LeafBlock *)c->sc.leaves; r.tri_flat = (TriFlat *)c->sc.tri_flat; r.tri_index = c->sc.tri_index;
    r.nslots = 4 * c->accel_leaves; r.attrs = c->sc.attrs; r.ntri = c->scene_tris; r.boxes = c->d_refit_boxes;
    return r;
}

// A refit with posed meshes (behind the wait for the last refit's copies).  begin[mi]: where skinned mesh mi's corner skin lies in d_skin --
// the skinned meshes one behind the other, in corners.  When the set of skinned meshes has changed (or nothing is there yet) the arrays are
// made for it: the corner skins, the palette array for all skinned meshes' bones on the device and in pinned memory, the descriptor tables;
// every mesh's part then goes up again at its next posed refit.  src[mi]: where the part of a posed mesh the device lacks lies in
// c->skin_upload, expanded here from the per-vertex skin through the mesh's index array.
static int skin_prepare(evplp_context *c, const std::vector<int32_t> &first, std::vector<int32_t> &begin, std::vector<size_t> &src) {
    const size_t nm = c->meshes.size();
    begin.assign(nm, 0); src.assign(nm, 0);
    int64_t corners = 0, bones = 0;
    for (size_t mi = 0; mi < nm; mi++) if (c->meshes[mi].skin_bones > 0) { begin[mi] = (int32_t)corners; corners += 3 * (int64_t)(first[mi + 1] - first[mi]); bones += c->meshes[mi].skin_bones; }
    if (corners > INT32_MAX) { c->set_error("evplp_refit_accel: %lld skinned triangle corners are more than the skin launch indexes", (long long)corners); return EVPLP_ERR_INVALID; }
    if (c->skin_stale) {
        for (HostMesh &m : c->meshes) m.skin_at = -1;
        if (!c->d_sdesc || corners > c->skin_cap || bones > c->bone_cap) {
            release_skin(c);
            const int rc = alloc_arrays(c, skin_arrays(c, (size_t)std::max<int64_t>(corners, 1), (size_t)std::max<int64_t>(bones, 1), nm), "evplp_refit_accel", "the skins on the device"); if (rc) return rc;
            c->skin_cap = (int32_t)corners; c->bone_cap = (int32_t)bones;
        }
        c->skin_stale = false;
    }
    c->skin_upload.clear();
    for (size_t mi = 0; mi < nm; mi++) if (c->mesh_dirty[mi] == MeshDirty::Pose && c->meshes[mi].skin_at < 0) {
        const HostMesh &m = c->meshes[mi];
        src[mi] = c->skin_upload.size();
        for (size_t k = 0; k < m.idx.size(); k++) {
            const size_t v = (size_t)m.idx[k];
            CornerSkin s;
            for (int q = 0; q < 4; q++) { s.b[q] = (uint16_t)m.skin_index[4 * v + q]; s.w[q] = m.skin_weight[4 * v + q]; }
            c->skin_upload.push_back(s);
        }
    }
    return EVPLP_OK;
}

// A refit with meshes under morph weights, the twin of skin_prepare: begin[mi] and src[mi] likewise for mesh mi's corner deltas in d_morph and
// c->morph_upload -- the meshes with targets one behind the other, in float3, each target-major [T][3 count].  need_base: a mesh under weights
// is also moved by a matrix or a pose -- the base array is made, as a copy of the rest-pose array as the stream finds it here.
static int morph_prepare(evplp_context *c, const std::vector<int32_t> &first, bool need_base, std::vector<int32_t> &begin, std::vector<size_t> &src) {
    const size_t nm = c->meshes.size();
    begin.assign(nm, 0); src.assign(nm, 0);
    int64_t vectors = 0, weights = 0;
    for (size_t mi = 0; mi < nm; mi++) if (c->meshes[mi].morph_targets > 0) {
        begin[mi] = (int32_t)vectors; vectors += 3 * (int64_t)(first[mi + 1] - first[mi]) * c->meshes[mi].morph_targets; weights += c->meshes[mi].morph_targets;
        if (vectors > INT32_MAX) { c->set_error("evplp_refit_accel: the corner deltas of the morph targets are more than the morph launch indexes"); return EVPLP_ERR_INVALID; }
    }
    if (c->morph_stale) {
        for (HostMesh &m : c->meshes) m.morph_at = -1;
        if (!c->d_mdesc || vectors > c->morph_cap || weights > c->weight_cap) {
            release_morph(c);
            const int rc = alloc_arrays(c, morph_arrays(c, (size_t)std::max<int64_t>(vectors, 1), (size_t)std::max<int64_t>(weights, 1), nm), "evplp_refit_accel", "the morph targets on the device"); if (rc) return rc;
            c->morph_cap = vectors; c->weight_cap = (int32_t)weights;
        }
        c->morph_stale = false;
    }
    if (need_base && !c->d_base) {
        const size_t tris = (size_t)std::max(c->scene_tris, 1), bytes = sizeof(float) * 9 * tris;
        const int rc = alloc_arrays(c, base_array(c, tris), "evplp_refit_accel", "the morphed base on the device"); if (rc) return rc;
        HIP_TRY(c, hipMemcpyAsync(c->d_base, c->d_rest, bytes, hipMemcpyDeviceToDevice, c->stream));
        for (HostMesh &m : c->meshes) m.base_state = BaseState::Rest;
    }
    c->morph_upload.clear();
    for (size_t mi = 0; mi < nm; mi++) if (moved_on_device(c->mesh_dirty[mi]) && !c->meshes[mi].morph_w.empty() && c->meshes[mi].morph_at < 0) {
        const HostMesh &m = c->meshes[mi];
        const size_t nv = m.verts.size() / 3;
        src[mi] = c->morph_upload.size();
        for (int32_t k = 0; k < m.morph_targets; k++)
            for (size_t q = 0; q < m.idx.size(); q++) {
                const float *d = &m.morph_delta[3 * ((size_t)k * nv + (size_t)m.idx[q])];
                c->morph_upload.insert(c->morph_upload.end(), d, d + 3);
            }
    }
    return EVPLP_OK;
}
// What the stages of evplp_refit_accel hand each other.  first[m]: mesh m's first triangle, first[meshes]: all of them.  flat: the dirty
// meshes' triangles, flattened once -- for the figures, and for the staging copy of those that are dirty by upload -- mesh m's at flat_at[m].
// cdf: the light's, if it moved.  uploaded: the floats of the meshes dirty by upload in the pinned array; the missing rest poses lie behind.
namespace { struct RefitWork {
    std::vector<int32_t> first, skin_begin, morph_begin; std::vector<size_t> flat_at, skin_src, morph_src; std::vector<float> flat, cdf;
    size_t uploaded = 0; float pad = 0.f; int32_t rot = 0; bool timed = false, stages = false;
}; }
// The host's figures, by the code evplp_build_accel uses, for the meshes that moved alone (in front of the launches, so that they follow
// each other without a gap)
static void refit_figures(evplp_context *c, RefitWork &w) {
    std::vector<int32_t> &first = w.first; std::vector<float> &cdf = w.cdf, &flat = w.flat; std::vector<size_t> &flat_at = w.flat_at;
    { int32_t n = 0; for (const HostMesh &m : c->meshes) { first.push_back(n); n += (int32_t)(m.idx.size() / 3); } first.push_back(n); }
    flat_at.assign(c->meshes.size(), 0);
    { size_t n = 0; for (size_t mi = 0; mi < c->meshes.size(); mi++) if (c->mesh_dirty[mi] != MeshDirty::Clean) { flat_at[mi] = n; n += 9 * (size_t)(first[mi + 1] - first[mi]); } flat.resize(n); }
    for (size_t mi = 0; mi < c->meshes.size(); mi++) if (c->mesh_dirty[mi] != MeshDirty::Clean) {
        flatten_mesh(c->meshes[mi], c->meshes[mi].verts, flat.data() + flat_at[mi]);
        mesh_figures(c->meshes[mi], flat.data() + flat_at[mi], nullptr);
    }
    if (c->mesh_dirty[(size_t)c->light_mesh] != MeshDirty::Clean) light_figures(c, flat.data() + flat_at[(size_t)c->light_mesh], cdf);
    w.pad = scene_fold(c);
}
// The wait for the last refit's copies, and behind it the arrays of the skin and the morph launch where posed or morphed meshes need them
static int refit_deformer_arrays(evplp_context *c, RefitWork &w) {
    int rc; bool any = false, need_base = false;
    if (c->refit_count > 0) HIP_TRY(c, hipEventSynchronize(c->ev_refit_staged));     // (the last refit's copies have left the pinned arrays: long ago)
    if (std::find(c->mesh_dirty.begin(), c->mesh_dirty.end(), MeshDirty::Pose) != c->mesh_dirty.end() && (rc = skin_prepare(c, w.first, w.skin_begin, w.skin_src))) return rc;
    for (size_t mi = 0; mi < c->meshes.size(); mi++) if (moved_on_device(c->mesh_dirty[mi]) && !c->meshes[mi].morph_w.empty()) { any = true; need_base = need_base || moves_base(c->mesh_dirty[mi]); }
    if (any && (rc = morph_prepare(c, w.first, need_base, w.morph_begin, w.morph_src))) return rc;
    return EVPLP_OK;
}
// The triangles of the meshes dirty by upload, packed, in one copy; one scatter per run of neighbouring such meshes.  Behind them in the
// pinned array, the rest pose of every mesh that was given a matrix and whose rest pose the device does not hold in any form.
// (one memcpy per mesh into the pinned array, as ever: what the copy engine then reads was written the way it was before there were matrices)
static int refit_stage_vertices(evplp_context *c, RefitWork &w) {
    const std::vector<int32_t> &first = w.first; const std::vector<float> &flat = w.flat; const std::vector<size_t> &flat_at = w.flat_at; const bool timed = w.timed;
    size_t staged = 0;
    for (size_t mi = 0; mi < c->meshes.size(); mi++) if (c->mesh_dirty[mi] == MeshDirty::Upload) {
        const size_t n = 9 * (size_t)(first[mi + 1] - first[mi]);
        std::memcpy(c->h_refit_stage + staged, flat.data() + flat_at[mi], sizeof(float) * n);
        staged += n;
    }
    const size_t uploaded = w.uploaded = staged;
    for (size_t mi = 0; mi < c->meshes.size(); mi++) if (moved_on_device(c->mesh_dirty[mi]) && c->meshes[mi].rest_state == RestState::FromHost) {
        const size_t n = 9 * (size_t)(first[mi + 1] - first[mi]);
        std::vector<float> rest(n);
        flatten_mesh(c->meshes[mi], c->meshes[mi].rest, rest.data());
        std::memcpy(c->h_refit_stage + staged, rest.data(), sizeof(float) * n);
        staged += n;
    }
    if (timed) HIP_TRY(c, hipEventRecord(c->ev_refit[0], c->stream));
    if (uploaded) HIP_TRY(c, hipMemcpyAsync(c->d_refit_stage, c->h_refit_stage, sizeof(float) * uploaded, hipMemcpyHostToDevice, c->stream));
    staged = 0;
    for (size_t mi = 0; mi < c->meshes.size();) {
        if (c->mesh_dirty[mi] != MeshDirty::Upload) { mi++; continue; }
        size_t me = mi; while (me < c->meshes.size() && c->mesh_dirty[me] == MeshDirty::Upload) me++;
        const int32_t count = first[me] - first[mi];
        refit_scatter(c->d_refit_stage + staged, first[mi], count, (TriAttr *)c->sc.attrs, c->stream);
        staged += 9 * (size_t)count; mi = me;
    }
    return EVPLP_OK;
}
// The meshes dirty by transform: their rest pose where the device lacks it (once per mesh and rest pose), the table of their matrices
// through pinned memory, and ONE launch that writes the attributes of all of them from the rest pose.  Nothing of them is staged or copied.
// The meshes dirty by pose likewise: the same rest pose, each mesh's corner skin where the device lacks it (once per mesh and skin),
// the palettes one behind the other and the table of their places through pinned memory, and ONE launch that writes all of them.
// The meshes under morph weights: each mesh's corner deltas where the device lacks them (once per mesh and set of targets), the weight
// sets one behind the other and the table through pinned memory, and ONE launch, in front of the two above, that writes the attributes of
// the meshes nothing else moves and the base of the others -- which the two launches then read in place of the rest pose: the base array
// is a copy of the rest-pose array but for those meshes' parts, kept in step here.  A mesh whose base the device holds is not written again.
static int refit_deform(evplp_context *c, RefitWork &w) {
    const std::vector<int32_t> &first = w.first, &skin_begin = w.skin_begin, &morph_begin = w.morph_begin; const std::vector<size_t> &skin_src = w.skin_src, &morph_src = w.morph_src;
    const bool stages = w.stages; size_t staged = w.uploaded;             // (staged: the rest poses in the pinned array, behind the uploaded meshes)
    int32_t nx = 0, moved = 0, ns = 0, posed = 0, nbone = 0, nmo = 0, morphed = 0, nweight = 0;
    for (size_t mi = 0; mi < c->meshes.size(); mi++) if (moved_on_device(c->mesh_dirty[mi])) {
        HostMesh &m = c->meshes[mi];
        const int32_t count = first[mi + 1] - first[mi];
        if (m.rest_state == RestState::FromAttrs) refit_rest(c->sc.attrs, first[mi], count, c->d_rest, c->stream);
        else if (m.rest_state == RestState::FromHost) {
            if (count > 0) HIP_TRY(c, hipMemcpyAsync(c->d_rest + 9 * (size_t)first[mi], c->h_refit_stage + staged, sizeof(float) * 9 * (size_t)count, hipMemcpyHostToDevice, c->stream));
            staged += 9 * (size_t)count;
        }
        if (m.rest_state != RestState::There && c->d_base) {
            if (count > 0) HIP_TRY(c, hipMemcpyAsync(c->d_base + 9 * (size_t)first[mi], c->d_rest + 9 * (size_t)first[mi], sizeof(float) * 9 * (size_t)count, hipMemcpyDeviceToDevice, c->stream));
            m.base_state = BaseState::Rest;
        }
        m.rest_state = RestState::There;
        if (count <= 0) continue;
        if (!m.morph_w.empty() && (!moves_base(c->mesh_dirty[mi]) || m.base_state != BaseState::Weights)) {
            if (m.morph_at < 0) {
                m.morph_at = morph_begin[mi];
                HIP_TRY(c, hipMemcpyAsync(c->d_morph + 3 * (size_t)m.morph_at, c->morph_upload.data() + morph_src[mi], sizeof(float) * 9 * (size_t)count * (size_t)m.morph_targets, hipMemcpyHostToDevice, c->stream));
            }
            MorphDesc &d = c->h_mdesc[nmo++];
            d.first = first[mi]; d.count = count; d.begin = morphed; d.weight_at = nweight; d.delta_at = m.morph_at; d.ntargets = m.morph_targets; d.to_base = moves_base(c->mesh_dirty[mi]); d.pad = 0;
            std::memcpy(c->h_mweights + nweight, m.morph_w.data(), sizeof(float) * (size_t)m.morph_targets);
            morphed += count; nweight += m.morph_targets;
            if (d.to_base) m.base_state = BaseState::Weights;
        } else if (m.morph_w.empty() && c->d_base && m.base_state != BaseState::Rest) {       // (the weights were taken away: the base is the rest pose again)
            HIP_TRY(c, hipMemcpyAsync(c->d_base + 9 * (size_t)first[mi], c->d_rest + 9 * (size_t)first[mi], sizeof(float) * 9 * (size_t)count, hipMemcpyDeviceToDevice, c->stream));
            m.base_state = BaseState::Rest;
        }
        if (!moves_base(c->mesh_dirty[mi])) continue;
        if (c->mesh_dirty[mi] == MeshDirty::Pose) {
            if (m.skin_at < 0) {
                m.skin_at = skin_begin[mi];
                HIP_TRY(c, hipMemcpyAsync(c->d_skin + m.skin_at, c->skin_upload.data() + skin_src[mi], sizeof(CornerSkin) * 3 * (size_t)count, hipMemcpyHostToDevice, c->stream));
            }
            SkinDesc &s = c->h_sdesc[ns++];
            s.first = first[mi]; s.count = count; s.begin = posed; s.bone_at = nbone; s.nbones = m.skin_bones; s.skin_at = m.skin_at; s.pad[0] = s.pad[1] = 0;
            std::memcpy(c->h_bones + 12 * (size_t)nbone, m.palette.data(), sizeof(float) * 12 * (size_t)m.skin_bones);
            posed += count; nbone += m.skin_bones;
            continue;
        }
        TransformDesc &d = c->h_xform[nx++];
        d.first = first[mi]; d.count = count; d.begin = moved; d.pad = 0; std::memcpy(d.m, m.matrix, sizeof(d.m));
        moved += count;
    }
    if (nmo) {
        HIP_TRY(c, hipMemcpyAsync(c->d_mdesc, c->h_mdesc, sizeof(MorphDesc) * (size_t)nmo, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->d_mweights, c->h_mweights, sizeof(float) * (size_t)nweight, hipMemcpyHostToDevice, c->stream));
        refit_morph(c->d_mdesc, nmo, morphed, c->d_rest, c->d_mweights, c->weight_cap, c->d_morph, c->morph_cap, c->d_base, (TriAttr *)c->sc.attrs, c->scene_tris, c->stream);
    }
    const float *based = c->d_base ? c->d_base : c->d_rest;     // (what a matrix and a pose act on)
    if (nx) {
        HIP_TRY(c, hipMemcpyAsync(c->d_xform, c->h_xform, sizeof(TransformDesc) * (size_t)nx, hipMemcpyHostToDevice, c->stream));
        refit_transform(c->d_xform, nx, moved, based, (TriAttr *)c->sc.attrs, c->scene_tris, c->stream);
    }
    if (ns) {
        HIP_TRY(c, hipMemcpyAsync(c->d_sdesc, c->h_sdesc, sizeof(SkinDesc) * (size_t)ns, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->d_bones, c->h_bones, sizeof(float) * 12 * (size_t)nbone, hipMemcpyHostToDevice, c->stream));
        refit_skin(c->d_sdesc, ns, posed, based, c->d_skin, c->skin_cap, c->d_bones, (TriAttr *)c->sc.attrs, c->scene_tris, c->stream);
    }
    if (stages) HIP_TRY(c, hipEventRecord(c->ev_refit[1], c->stream));
    return EVPLP_OK;
}
// The tree: leaf operands; boxes, one launch per height; four-wide nodes; the rotations' counts on their way back
static int refit_tree(evplp_context *c, const RefitWork &w) {
    const int32_t rot = w.rot; const float pad = w.pad; const bool stages = w.stages;
    const RefitScene r = refit_scene(c);
    refit_leaves(r, c->stream);
    if (stages) HIP_TRY(c, hipEventRecord(c->ev_refit[2], c->stream));
    if (rot > 0) rotate_enqueue(c, r, pad, rot);             // (the first pass IS the refit's sweep; further passes repeat it)
    else for (int32_t l = 0; l < c->refit_levels; l++)
        refit_level(r, c->d_refit_order + c->refit_level_begin[(size_t)l], c->refit_level_begin[(size_t)l + 1] - c->refit_level_begin[(size_t)l], pad, c->stream);
    if (stages) HIP_TRY(c, hipEventRecord(c->ev_refit[3], c->stream));
    build_nodes4_into(c->sc.nodes, c->accel_nodes, c->stream, (BvhNode4 *)c->sc.nodes4);
    if (rot > 0) HIP_TRY(c, hipMemcpyAsync(c->h_rotate_out, c->d_rotate_out, sizeof(int32_t) * 2 * (size_t)rot, hipMemcpyDeviceToHost, c->stream));
    return EVPLP_OK;
}
// The light's CDF, which goes up only if the light moved; the events that close the refit; what the new tree invalidates; nothing is dirty
static int refit_close(evplp_context *c, const RefitWork &w) {
    const std::vector<float> &cdf = w.cdf; const bool timed = w.timed;
    if (c->mesh_dirty[(size_t)c->light_mesh] != MeshDirty::Clean) {
        float *h = c->h_refit_stage + 9 * (size_t)c->scene_tris;
        std::memcpy(h, cdf.data(), sizeof(float) * cdf.size());
        HIP_TRY(c, hipMemcpyAsync((void *)c->sc.light_cdf, h, sizeof(float) * cdf.size(), hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(c, hipEventRecord(c->ev_refit_staged, c->stream));
    if (timed) HIP_TRY(c, hipEventRecord(c->ev_refit[4], c->stream));
    if (c->aux_stream) HIP_TRY(c, hipStreamWaitEvent(c->aux_stream, c->ev_refit_staged, 0));      // (light paths given to the second stream from here on see the new tree)
    HIP_TRY(c, hipGetLastError());
    c->accel_pad = w.pad; c->refit_timed = timed; c->refit_stages_timed = w.stages; c->refit_count++; c->refits_since_build++;
    c->primary_cuts_valid = false; c->tile_box_valid = false; c->primary_current = false;
    std::fill(c->mesh_dirty.begin(), c->mesh_dirty.end(), MeshDirty::Clean); c->scene_dirty = false;
    return EVPLP_OK;
}
// The policy (evplp_set_refit_policy): the cost of the refitted tree against the cost of the tree as built.  One small launch and
// one host wait; a rebuild is evplp_build_accel's code (which measures the new built_cost, the policy being on).
// With rotations on, the cost is the rotated tree's, and the wait is the one that brings the rotations' counts back.
static int refit_policy(evplp_context *c, const RefitWork &w) {
    const int32_t rot = w.rot; int rc;
    if (c->policy_ratio > 0.0) {
        double q[5];
        if ((rc = measure_cost(c, q))) return rc;
        if (rot > 0) rotate_finish(c, rot);
        if (q[0] > c->policy_ratio * c->built_cost) {
            if ((rc = build_accel(c, c->policy_builder))) return rc;
            c->policy_rebuilds++; c->last_action = 2;
        } else c->last_action = rot > 0 ? 3 : 1;
    } else if (rot > 0) {                   // the refit with rotations is not free of host waits: the root's counts and stack need come back
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        rotate_finish(c, rot);
        c->last_action = 3;
    }
    return EVPLP_OK;
}

extern "C" int evplp_refit_accel(evplp_context *c) {
    CTX_CHECK(c);
    if (!evplp::refit_check(c)) return EVPLP_ERR_INVALID;
    if (!c->scene_dirty) return EVPLP_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    // (a photon splat whose verdict is still out is not waited for: a splat reads records and the G-buffer, never the scene)
    int rc = refit_prepare(c); if (rc) return rc;
    RefitWork w;
    w.rot = c->rotate_passes;               // (evplp_set_refit_rotations; 0, the default: the call is what it always was)
    if (w.rot > 0 && (rc = rotate_prepare(c))) return rc;
    refit_figures(c, w);
    // Everything below is enqueued on the context's stream, behind every pass it was given -- the light tracing of overlap_light_tracing
    // included: the call that put it on the second stream made this stream wait for it.
    w.timed = c->profile_passes; w.stages = w.timed && c->profile_kernels;
    if ((rc = refit_deformer_arrays(c, w))) return rc;
    if ((rc = refit_stage_vertices(c, w))) return rc;
    if ((rc = refit_deform(c, w))) return rc;
    if ((rc = refit_tree(c, w))) return rc;
    if ((rc = refit_close(c, w))) return rc;
    return refit_policy(c, w);
}

// ---------------------------------------------------------------------------------- the tree's SAH cost, and the refit policy
namespace evplp {
// The cost of the tree as it is on the device into out[5], behind everything on the context's stream; waits.  The first measurement
// since a build is kept as built_cost.
int measure_cost(evplp_context *c, double out[5]) {
    int rc = refit_prepare(c); if (rc) return rc;              // (the plan is the refit's; made here if no refit has made it)
    const int32_t nchunks = (c->refit_reached + kCostChunk - 1) / kCostChunk;
    const size_t bytes = sizeof(double) * (1 + 3 * (size_t)nchunks);
    if (!c->d_cost && (rc = alloc_arrays(c, cost_arrays(c, 1 + 3 * (size_t)nchunks), "evplp_accel_quality", "the sums' arrays"))) return rc;
    const bool timed = c->profile_passes;
    for (int i = 0; i < 2 && timed; i++) if (!c->ev_cost[i]) HIP_TRY(c, hipEventCreate(&c->ev_cost[i]));
    if (timed) HIP_TRY(c, hipEventRecord(c->ev_cost[0], c->stream));
    accel_cost(c->sc.nodes, c->accel_nodes, c->d_refit_order, c->refit_reached, c->d_cost, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->h_cost, c->d_cost, bytes, hipMemcpyDeviceToHost, c->stream));
    if (timed) HIP_TRY(c, hipEventRecord(c->ev_cost[1], c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->cost_timed = timed;
    accel_cost_finish(c->h_cost + 1, nchunks, c->h_cost[0], out);
    if (!c->built_cost_known) { c->built_cost = out[0]; c->built_cost_known = true; }
    return EVPLP_OK;
}
bool accel_quality_check(evplp_context *c, const char *name) {
    if (!c->accel_built) { c->set_error("%s: scene not built (evplp_build_accel)", name); return false; }
    if (c->scene_dirty) { c->set_error("%s: vertices were updated (evplp_update_mesh): call evplp_refit_accel or evplp_build_accel first", name); return false; }
    return true;
}
bool refit_policy_check(evplp_context *c, double max_cost_ratio, int32_t rebuild_builder) {
    if (!(max_cost_ratio >= 0.0) || !std::isfinite(max_cost_ratio)) { c->set_error("evplp_set_refit_policy: max_cost_ratio must be finite and >= 0 (0: off)"); return false; }
    if (rebuild_builder < -1 || rebuild_builder > EVPLP_BVH_LBVH_GPU) { c->set_error("evplp_set_refit_policy: rebuild_builder %d is neither an evplp_bvh_builder nor -1", rebuild_builder); return false; }
    if (c->scene_dirty) { c->set_error("evplp_set_refit_policy: vertices were updated (evplp_update_mesh): call evplp_refit_accel or evplp_build_accel first"); return false; }
    return true;
}
}
extern "C" int evplp_accel_quality(evplp_context *c, struct evplp_accel_quality *out) {
    CTX_CHECK(c);
    if (!out) { c->set_error("evplp_accel_quality: null destination"); return EVPLP_ERR_INVALID; }
    if (!evplp::accel_quality_check(c, "evplp_accel_quality")) return EVPLP_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    double q[5];
    const int rc = measure_cost(c, q); if (rc) return rc;
    std::memset(out, 0, sizeof(*out));
    out->cost = q[0]; out->root_area = q[1]; out->inner_area = q[2]; out->leaf_pair_area = q[3]; out->leaf_tri_area = q[4];
    out->built_cost = c->built_cost; out->reached_nodes = c->refit_reached; out->leaf_refs = c->refit_leaf_refs;
    out->refits_since_build = c->refits_since_build; out->policy_rebuilds = c->policy_rebuilds; out->last_action = c->last_action;
    return EVPLP_OK;
}
extern "C" int evplp_set_refit_policy(evplp_context *c, double max_cost_ratio, int32_t rebuild_builder) {
    CTX_CHECK(c);
    if (!evplp::refit_policy_check(c, max_cost_ratio, rebuild_builder)) return EVPLP_ERR_INVALID;
    if (max_cost_ratio > 0.0 && c->accel_built && !c->built_cost_known) {
        HIP_TRY(c, hipSetDevice(c->cfg.device));
        double q[5];
        const int rc = measure_cost(c, q); if (rc) return rc;
    }
    c->policy_ratio = max_cost_ratio; c->policy_builder = rebuild_builder;
    return EVPLP_OK;
}

// ---------------------------------------------------------------------------------- tree rotations
namespace evplp {
bool optimize_accel_check(evplp_context *c, const char *name, int32_t passes) {
    if (!accel_quality_check(c, name)) return false;
    if (passes < 1 || passes > 8) { c->set_error("%s: passes must be 1 .. 8, not %d", name, passes); return false; }
    return true;
}
bool refit_rotations_check(evplp_context *c, const char *name, int32_t passes) {
    if (passes < 0 || passes > 8) { c->set_error("%s: passes must be 0 .. 8 (0: off), not %d", name, passes); return false; }
    return true;
}
}
extern "C" int evplp_optimize_accel(evplp_context *c, int32_t passes, int32_t *rotations) {
    CTX_CHECK(c);
    if (!evplp::optimize_accel_check(c, "evplp_optimize_accel", passes)) return EVPLP_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int rc = refit_prepare(c); if (rc) return rc;
    if ((rc = rotate_prepare(c))) return rc;
    // behind everything on the context's stream: `passes` sweeps from the leaves' boxes upward (the triangles have not moved, so the leaf
    // operands stay), the four-wide nodes again, and the root's counts back in one small copy; one host wait
    rotate_enqueue(c, refit_scene(c), c->accel_pad, passes);
    build_nodes4_into(c->sc.nodes, c->accel_nodes, c->stream, (BvhNode4 *)c->sc.nodes4);
    HIP_TRY(c, hipMemcpyAsync(c->h_rotate_out, c->d_rotate_out, sizeof(int32_t) * 2 * (size_t)passes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    rotate_finish(c, passes);
    c->primary_cuts_valid = false; c->tile_box_valid = false; c->primary_current = false;
    c->last_action = 3;
    if (rotations) *rotations = c->rotations_last;
    return EVPLP_OK;
}
extern "C" int evplp_set_refit_rotations(evplp_context *c, int32_t passes) {
    CTX_CHECK(c);
    if (!evplp::refit_rotations_check(c, "evplp_set_refit_rotations", passes)) return EVPLP_ERR_INVALID;
    c->rotate_passes = passes;
    return EVPLP_OK;
}
extern "C" int evplp_rotation_info(evplp_context *c, int32_t *since_build, int32_t *last_call, int32_t *per_pass, int32_t *refit_passes) {
    CTX_CHECK(c);
    if (since_build) *since_build = c->rotations_since_build;
    if (last_call) *last_call = c->rotations_last;
    if (per_pass) std::memcpy(per_pass, c->rotations_pass, sizeof(c->rotations_pass));
    if (refit_passes) *refit_passes = c->rotate_passes;
    return EVPLP_OK;
}
extern "C" int evplp_refit_info(evplp_context *c, int32_t *refits, int32_t *levels, float *last_refit_ms) {
    CTX_CHECK(c);
    if (refits) *refits = c->refit_count;
    if (levels) *levels = c->refit_levels;
    if (last_refit_ms) {
        *last_refit_ms = 0.f;
        if (c->refit_count > 0 && c->refit_timed) {
            HIP_TRY(c, hipSetDevice(c->cfg.device));
            HIP_TRY(c, hipEventSynchronize(c->ev_refit[4]));
            HIP_TRY(c, hipEventElapsedTime(last_refit_ms, c->ev_refit[0], c->ev_refit[4]));
        }
    }
    return EVPLP_OK;
}

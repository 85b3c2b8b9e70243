// Internal data layout of libevplp_hip.so (host + device).  See DESIGN.md "Data layout in HBM".
#pragma once
#include <math.h>
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "../../include/evplp.h"

namespace evplp {

// Flattened binary BVH node, 64 B = one s_load_dwordx16 / one cache line.  A node stores the boxes
// of BOTH children, interleaved component by component so that the two slab tests run as one
// stream of packed-fp32 instructions (half 0 = child 0, half 1 = child 1).  Boxes are stored as
// centre + half-size: with A = ctr * (1/d) - o/d and B = hal * |1/d| the slab entry / exit parameters
// are A - B and A + B, i.e. three v_pk_fma_f32 per axis for BOTH children and no per-lane min/max to
// sort the near and far plane.  child >= 0: inner node index; child < 0: leaf, id = ~child,
// leaf block = id >> 2, triangle count = (id & 3) + 1.  An absent child has a negative half-size and
// child = kNoChild.
struct BvhNode {
    float ctr[3][2];  // box centre   [axis][child]
    float hal[3][2];  // box half-size [axis][child] (>= 0; an absent child has hal = -big: never hit)
    int32_t c0, c1;
    int32_t pad[2];
};
static_assert(sizeof(BvhNode) == 64, "BvhNode must be 64 bytes");
// Four-wide node for the per-lane walks (incoherent rays: light tracing, path tracer, light-path windows): the two children of
// a binary node replaced by its (up to four) grandchildren -- half the dependent fetches per ray.  node4[i] is derived from
// binary node i on the device (bvh_gpu.hip build_nodes4); the walks only ever visit every second level of it.
struct BvhNode4 {
    float lo[3][4], hi[3][4];   // [axis][child]; an absent child has lo > hi
    int32_t child[4];           // binary node index (>= 0), ~leaf reference, or kNoChild
    int32_t pad[4];
};
static_assert(sizeof(BvhNode4) == 128, "BvhNode4 must be 128 bytes");
constexpr int32_t kNoChild = INT32_MIN;
constexpr int kMaxLeafTris = 4;
constexpr int kMaxDepth = 64;

// Leaf block, 192 B = three s_load_dwordx16: up to four triangles as TWO PAIRS; every operand of
// optix::intersect_triangle_branchless (p0, e0 = p1-p0, e1 = p0-p2, n = cross(e1, e0)) is stored as
// {triangle A, triangle B} so that a pair is tested with packed-fp32 instructions.  Unused slots
// are zero (den = 0 -> the test is false).
struct TriPair {
    float p0[3][2], e0[3][2], e1[3][2], n[3][2];   // [component][A|B]
};
static_assert(sizeof(TriPair) == 96, "TriPair must be 96 bytes");
struct LeafBlock { TriPair pair[2]; };
static_assert(sizeof(LeafBlock) == 192, "LeafBlock must be 192 bytes");
// The same operands once more, one triangle per 48 contiguous bytes (slot = 4 * leaf block + k): the per-lane walks
// fetch a triangle with three 16-byte loads instead of twelve strided words of the pair layout.
struct TriFlat { float p0[3], e0[3], e1[3], n[3]; };
static_assert(sizeof(TriFlat) == 48, "TriFlat must be 48 bytes");

// Shading attributes per ORIGINAL triangle.
struct TriAttr {
    float v[9];      // p0,p1,p2 as uploaded (G-buffer position / normal use the originals)
    float uv[6];
    int32_t material;
};
static_assert(sizeof(TriAttr) == 64, "TriAttr must be 64 bytes");

struct Material {   // 64 B
    float kd[3]; float ns;
    float ks[3]; int32_t tex_kd;
    float light[4];           // mLightIntensity (I*pi, w); zeros for non-emitters
    int32_t tex_ks, tex_ns, pad0, pad1;
};
static_assert(sizeof(Material) == 64, "Material must be 64 bytes");

struct TexDesc { int32_t w, h; uint32_t offset; uint32_t pad; };  // offset in float4 units into the pool

// Camera basis (glm::lookAt RH + glm::perspective, rt/rtcommon.h:586-591)
struct CamBasis {
    float eye[3]; float tan_half;
    float s[3];   float aspect;
    float u[3];   float pad0;
    float f[3];   float pad1;
};

// Everything a traversal kernel needs, passed by value as a kernel argument (all pointers
// wave-uniform => scalar loads).
struct SceneDev {
    const BvhNode *nodes;
    const BvhNode4 *nodes4;      // per-lane walks
    const LeafBlock *leaves;     // one block per leaf
    const TriFlat *tri_flat;     // 4 slots per leaf (per-lane walks)
    const int32_t *tri_index;    // 4 slots per leaf: original triangle index or -1
    const TriAttr *attrs;        // original order
    const Material *materials;
    const TexDesc *textures;
    const float4 *tex_pool;
    const float *light_cdf;      // normalised area CDF of the light mesh
    int32_t ntris;               // triangles in the BVH (degenerate ones dropped)
    int32_t bvh_depth;           // deepest leaf: sizes the per-lane traversal stacks (dynamic LDS)
    int32_t stack4_entries;      // worst-case stack of the four-wide per-lane walk over THIS tree (computed at build time; see evplp_build_accel)
    int32_t pad_sc;
    int32_t light_first, light_count; // ORIGINAL triangle index range of the light mesh
    float light_area;
    float light_intensity[4];    // (I*pi, w)
    float light_unscaled[4];     // (I, w)
    float light_lo[3], light_hi[3];   // bounds of the light mesh, padded (primary_kernel skips its walk for tiles that cannot see it)
};

// Strip geometry shared by all per-pixel kernels.
struct StripDev {
    int32_t W, H;
    int32_t strip_rank, strip_count, strip_rows;
    int32_t local_rows;
    // DEALT blocks (evplp_set_blocks; strip_count > 1): the owned-block table replaces "block b belongs to rank b % strip_count".
    //   blocks[l], l < cap_blocks = local_rows / strip_rows: the image block stored in local block l; a local block that holds nothing carries an
    //     index >= the image's block count, i.e. rows >= H: outside the image, as the padding rows of the round-robin deal are;
    //   blocks[cap_blocks + b], b < image blocks: the local block that holds image block b, or -1 (another rank's).
    // nullptr = the round-robin deal.  Two copies of the same table: `blocks` in device memory, `blocks_host` for the host side of global_row.
    const int32_t *blocks, *blocks_host;
    int32_t cap_blocks, pad_st;
    __host__ __device__ inline int32_t global_block(int32_t local_blk) const {
#if defined(__HIP_DEVICE_COMPILE__)
        const int32_t *t = blocks;
#else
        const int32_t *t = blocks_host;
#endif
        return t ? t[local_blk] : local_blk * strip_count + strip_rank;
    }
    __host__ __device__ inline int32_t global_row(int32_t local) const {
        int32_t blk = local / strip_rows;
        return global_block(blk) * strip_rows + (local - blk * strip_rows);
    }
    // the local block that holds image block b, or -1 (strip_count > 1 only)
    __host__ __device__ inline int32_t local_block(int32_t b) const {
#if defined(__HIP_DEVICE_COMPILE__)
        const int32_t *t = blocks;
#else
        const int32_t *t = blocks_host;
#endif
        if (t) return t[cap_blocks + b];
        return b % strip_count == strip_rank ? b / strip_count : -1;
    }
};

// meshBound's rule (rt/triangleintersect.cu:62-81): a triangle is in the tree iff area = |cross(v1-v0, v2-v0)| is > 0 and finite.  v: 9 floats.
// Every operation rounds on its own (no contraction), on the host and on the device alike: the builders and a refit must agree on it.
__host__ __device__ inline bool tri_has_area(const float *v) {
#pragma clang fp contract(off)
    const float a[3] = { v[3] - v[0], v[4] - v[1], v[5] - v[2] }, b[3] = { v[6] - v[0], v[7] - v[1], v[8] - v[2] };
    const float c[3] = { a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0] };
    const float area = sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    return area > 0.0f && area <= 3.4028235e38f;                          // (> 0 and not infinite; a NaN fails the first)
}

// What the refit kernels of bvh_gpu.hip work on (evplp_refit_accel): the tree in place, the attributes with the moved vertices, and
// boxes = 6 floats per node of scratch (the unpadded box under every node, handed from one height's launch to the next)
struct RefitScene {
    BvhNode *nodes; int32_t nnodes;
    LeafBlock *leaves; TriFlat *tri_flat; const int32_t *tri_index; int32_t nslots;     // nslots = 4 * leaf blocks
    const TriAttr *attrs; int32_t ntri;                                                // ORIGINAL triangles
    float *boxes;
};

// ---- the SAH cost of the flattened tree (evplp_accel_quality on the device, evplp_accel_cost on the host: include/evplp.h).
// The weights are the vector instructions of a node visit and of a pair test of the packet walk.  Host and device
// form every term with the functions below and add them in one fixed shape: entry 256 k + i of the plan's order is thread i of chunk k,
// a chunk is reduced by halving strides within each run of 64 (the wavefront's shuffle-down), the four runs are added in order, and the
// chunks' sums are added in index order.  Every operation rounds on its own (no contraction), so the two agree bit for bit.
constexpr double kCostNodeVisit = 15.0, kCostPairTest = 40.0;
constexpr int kCostChunk = 256;
// a box with a negative half-size holds nothing (an absent child; a leaf whose triangles have all lost their area): area 0
__host__ __device__ inline bool cost_box_present(const BvhNode &f, int s) {
    return (s ? f.c1 : f.c0) != kNoChild && f.hal[0][s] >= 0.0f && f.hal[1][s] >= 0.0f && f.hal[2][s] >= 0.0f;
}
// t[0] += inner_area, t[1] += leaf_pair_area, t[2] += leaf_tri_area of node f (child 0, then child 1)
__host__ __device__ inline void accel_cost_terms(const BvhNode &f, double t[3]) {
#pragma clang fp contract(off)
    for (int s = 0; s < 2; s++) {
        if (!cost_box_present(f, s)) continue;
        const int32_t ref = s ? f.c1 : f.c0;
        const double hx = (double)f.hal[0][s], hy = (double)f.hal[1][s], hz = (double)f.hal[2][s];
        const double a = 8.0 * (hx * hy + hy * hz + hz * hx);             // (fp32 x fp32 is exact in fp64)
        if (ref >= 0) t[0] += a;
        else {
            const int32_t cnt = (~ref & 3) + 1;                               // a zeroed (degenerate) triangle keeps its slot: the walk still tests it
            t[1] += a * (double)((cnt + 1) >> 1);
            t[2] += a * (double)cnt;
        }
    }
}
// the area of the union of the root's present child boxes (0: none)
__host__ __device__ inline double accel_root_area(const BvhNode &f) {
#pragma clang fp contract(off)
    double lo[3] = { 0.0, 0.0, 0.0 }, hi[3] = { 0.0, 0.0, 0.0 };
    bool any = false;
    for (int s = 0; s < 2; s++) {
        if (!cost_box_present(f, s)) continue;
        for (int k = 0; k < 3; k++) {
            const double l = (double)f.ctr[k][s] - (double)f.hal[k][s], h = (double)f.ctr[k][s] + (double)f.hal[k][s];
            lo[k] = any ? (l < lo[k] ? l : lo[k]) : l; hi[k] = any ? (h > hi[k] ? h : hi[k]) : h;
        }
        any = true;
    }
    const double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    return any ? 2.0 * (dx * dy + dy * dz + dz * dx) : 0.0;
}
// out = { cost, root_area, inner_area, leaf_pair_area, leaf_tri_area } from the chunks' triples { inner, pair, tri }, added in index order
inline void accel_cost_finish(const double *parts, int32_t nchunks, double root_area, double out[5]) {
#pragma clang fp contract(off)
    double t[3] = { 0.0, 0.0, 0.0 };
    for (int32_t k = 0; k < nchunks; k++) for (int j = 0; j < 3; j++) t[j] += parts[3 * (size_t)k + j];
    out[1] = root_area; out[2] = t[0]; out[3] = t[1]; out[4] = t[2];
    out[0] = root_area > 0.0 ? (kCostNodeVisit * (root_area + t[0]) + kCostPairTest * t[1]) / root_area : 0.0;
}

// ---- PLOC (Meister & Bittner 2018), the device builder EVPLP_BVH_PLOC_GPU of bvh_gpu.hip and its host twin evplp_ploc_tree (host/ploc.cpp).
// kPlocRadius: positions searched on either side for the nearest neighbour (EVPLP_PLOC_RADIUS overrides it, 1 .. kPlocMaxRadius);
// kPlocSearchIterations: search iterations before every further iteration pairs position 2k with 2k + 1 (EVPLP_PLOC_ITERATIONS, 0 .. 128).
constexpr int kPlocRadius = 16, kPlocMaxRadius = 32, kPlocSearchIterations = 128;
// the distance of two clusters: half the area of the union of their boxes (a, b: lo[3] then hi[3]).  fp32, every operation rounds on its
// own, in this order, on the host and on the device: the nearest neighbour hangs on a compare of two of these.
__host__ __device__ inline float ploc_distance(const float *a, const float *b) {
#pragma clang fp contract(off)
    const float ex = fmaxf(fmaxf(a[3], b[3]) - fminf(a[0], b[0]), 0.0f);
    const float ey = fmaxf(fmaxf(a[4], b[4]) - fminf(a[1], b[1]), 0.0f);
    const float ez = fmaxf(fmaxf(a[5], b[5]) - fminf(a[2], b[2]), 0.0f);
    return ex * ey + ey * ez + ez * ex;
}
// ---- evplp_transform_mesh: a point under a row-major 3 x 4 matrix, out[r] = ((m[4r] x + m[4r+1] y) + m[4r+2] z) + m[4r+3].  fp32, every
// product and every sum rounds on its own, in this order, and nothing is fused: the host copy of a mesh and refit_transform_kernel
// (bvh_gpu.hip) both call this and nothing else, and a test restates it in numpy.  No special case for the identity (-0.0 becomes +0.0).
__host__ __device__ inline void transform_point(const float m[12], const float p[3], float out[3]) {
#pragma clang fp contract(off)
    const float x = p[0], y = p[1], z = p[2];
    for (int r = 0; r < 3; r++) {
        const float a = m[4 * r] * x, b = m[4 * r + 1] * y, c = m[4 * r + 2] * z;
        out[r] = ((a + b) + c) + m[4 * r + 3];
    }
}
// ---- evplp_pose_mesh: a point under linear-blend skinning.  bones: a palette of row-major 3 x 4 matrices, b / w: the point's four bone
// indices and weights.  q_k = transform_point(bones + 12 b[k], p), out[r] = ((w[0] q_0[r] + w[1] q_1[r]) + w[2] q_2[r]) + w[3] q_3[r]: fp32,
// every product and every sum rounds on its own, in this order, and nothing is fused.  All four influences are always evaluated -- no special
// case for a zero weight, a repeated bone or the identity -- and nothing is renormalised, so weights (1, 0, 0, 0) over finite matrices give
// transform_point of bone b[0] value for value (the sign of a zero may differ).  The host copy of a mesh, evplp_skin_points (host/skin.cpp)
// and refit_skin_kernel (bvh_gpu.hip) call this and nothing else, and a test restates it in numpy.  out may be p.
__host__ __device__ inline void skin_point(const float *bones, const int32_t b[4], const float w[4], const float p[3], float out[3]) {
#pragma clang fp contract(off)
    float q[4][3];
    for (int k = 0; k < 4; k++) transform_point(bones + 12 * (size_t)b[k], p, q[k]);
    for (int r = 0; r < 3; r++) {
        const float a0 = w[0] * q[0][r], a1 = w[1] * q[1][r], a2 = w[2] * q[2][r], a3 = w[3] * q[3][r];
        out[r] = ((a0 + a1) + a2) + a3;
    }
}
// ---- evplp_morph_mesh: a point under morph targets (blend shapes).  delta: the point's offset in target 0 -- target k's lies `stride` floats
// further on each -- and w: the T weights.  out[r] = (((p[r] + w[0] d_0[r]) + w[1] d_1[r]) + ...) + w[T-1] d_{T-1}[r]: fp32, every product and
// every sum rounds on its own, in index order, and nothing is fused.  All targets are always evaluated -- no shortcut for a zero weight, so
// -0.0 may become +0.0 and every other bit of p is kept -- and the weights are used as given (negative and beyond 1 are legal).  The host copy
// of a mesh and evplp_morph_points (both through host/morph.cpp) and refit_morph_kernel (bvh_gpu.hip) call this and nothing else, and a test
// restates it in numpy.  out may be p.
__host__ __device__ inline void morph_point(const float *p, const float *delta, size_t stride, const float *w, int32_t T, float *out) {
#pragma clang fp contract(off)
    float x = p[0], y = p[1], z = p[2];
    for (int32_t k = 0; k < T; k++) {
        const float *d = delta + (size_t)k * stride;
        const float a = w[k] * d[0], b = w[k] * d[1], c = w[k] * d[2];
        x = x + a; y = y + b; z = z + c;
    }
    out[0] = x; out[1] = y; out[2] = z;
}
// ---- evplp_project_points / evplp_denoise_temporal: a world point on the screen of a camera, in pixel-centre coordinates (x to the right, y
// from the bottom: pixel (i, j) has its centre at (i, j)) and its view depth.  fp32, every product and every sum rounds on its own, in this
// order, and nothing is fused:
//   d = p - eye;  z = (d.x f.x + d.y f.y) + d.z f.z;  a = (d.x s.x + d.y s.y) + d.z s.z;  b = (d.x u.x + d.y u.y) + d.z u.z
//   cx = (a / z) / (aspect * tan_half);  cy = (b / z) / tan_half;  x = ((cx + 1) * W) / 2 - 0.5;  y = ((cy + 1) * H) / 2 - 0.5
// out = { x, y, z } and true; z <= 0 (or not a number): out = { 0, 0, z } and false -- the point is at or behind the eye.  The host entry
// point and temporal_accumulate_kernel (kernels_temporal.hip) both call this and nothing else, and a test restates it in numpy.
__host__ __device__ inline bool project_point(const CamBasis &cam, int32_t W, int32_t H, const float p[3], float out[3]) {
#pragma clang fp contract(off)
    const float dx = p[0] - cam.eye[0], dy = p[1] - cam.eye[1], dz = p[2] - cam.eye[2];
    const float zx = dx * cam.f[0], zy = dy * cam.f[1], zz = dz * cam.f[2];
    const float z = (zx + zy) + zz;
    out[0] = 0.0f; out[1] = 0.0f; out[2] = z;
    if (!(z > 0.0f)) return false;
    const float ax = dx * cam.s[0], ay = dy * cam.s[1], az = dz * cam.s[2];
    const float bx = dx * cam.u[0], by = dy * cam.u[1], bz = dz * cam.u[2];
    const float a = (ax + ay) + az, b = (bx + by) + bz;
    const float at = cam.aspect * cam.tan_half;
    const float cx = (a / z) / at, cy = (b / z) / cam.tan_half;
    const float sx = (cx + 1.0f) * (float)W, sy = (cy + 1.0f) * (float)H;
    out[0] = sx / 2.0f - 0.5f; out[1] = sy / 2.0f - 0.5f;
    return true;
}
// ---- tree rotations inside the refit sweep (Kensler 2008; Kopta et al. 2012): evplp_optimize_accel / evplp_set_refit_rotations on the device
// (refit_rotate_level_kernel, bvh_gpu.hip) and evplp_rotate_tree on the host (host/rotate.cpp) both decide with rotate_choice and count the
// four-wide walk's stack with rotate_need, and with nothing else.  A box is lo[3] then hi[3], exact and unpadded.
// Node N, processed at level l of the refit's PLAN, has the child slots ref[0], ref[1] (box[s], lvl[s] = the plan level of an inner child, -1
// for a leaf reference); an inner child ref[s] has the children gref[s][0], gref[s][1] with the boxes gbox[s][.] (kNoChild where ref[s] is
// no inner node).  Candidate (s, q), visited in the order (0,0), (0,1), (1,0), (1,1): A = ref[s] moves down, B = ref[1-s] must be an inner
// node, G = gref[1-s][q] moves up, K = gref[1-s][1-q] stays under B.  Admissible: none of A, G, K absent, none of their boxes empty
// (hi < lo on an axis: a leaf whose triangles have all lost their area), and lvl(A) < lvl(B) -- the PLAN's levels, not the current heights:
// every parent then keeps a strictly higher plan level than its children, so the plan stays a children-before-parents schedule, two nodes of
// one launch are never parent and child, and no path grows longer than the plan has levels.  (The levels stop being tight heights; nothing
// needs them to be.)  gain = area(box B) - area(box A u box K) with ploc_distance's fp32 area; the largest gain > 0 wins, ties keep the
// first candidate.  Returns 2 s + q, or -1: nothing to take.
__host__ __device__ inline bool rotate_box_empty(const float *b) { return b[3] < b[0] || b[4] < b[1] || b[5] < b[2]; }
__host__ __device__ inline int rotate_choice(const int32_t ref[2], const int32_t lvl[2], const float box[2][6], const int32_t gref[2][2], const float gbox[2][2][6]) {
#pragma clang fp contract(off)
    int best = -1;
    float best_gain = 0.0f;
#pragma unroll
    for (int s = 0; s < 2; s++) {
        if (ref[s] == kNoChild || ref[1 - s] < 0 || !(lvl[s] < lvl[1 - s]) || rotate_box_empty(box[s])) continue;
#pragma unroll
        for (int q = 0; q < 2; q++) {
            if (gref[1 - s][q] == kNoChild || gref[1 - s][1 - q] == kNoChild || rotate_box_empty(gbox[1 - s][q]) || rotate_box_empty(gbox[1 - s][1 - q])) continue;
            const float gain = ploc_distance(box[1 - s], box[1 - s]) - ploc_distance(box[s], gbox[1 - s][1 - q]);
            if (gain > best_gain) { best_gain = gain; best = 2 * s + q; }
        }
    }
    return best;
}
// the union of the boxes of a node's two child slots, folded from the empty box in slot order -- as refit_level_kernel folds them
__host__ __device__ inline void rotate_union(const float *b0, const float *b1, float *out) {
    for (int k = 0; k < 3; k++) { out[k] = fminf(fminf(3.0e38f, b0[k]), b1[k]); out[3 + k] = fmaxf(fmaxf(-3.0e38f, b0[3 + k]), b1[3 + k]); }
}
// The four-wide walk's stack need of a node (evplp_build_accel's sweep): g = what node4 puts in its four slots -- the two children of an
// inner child, or a leaf child itself and kNoChild --, need = the per-node array of the levels below.  max(valid - 1, 0) + the largest need
// among the inner ones.
__host__ __device__ inline int32_t rotate_need(const int32_t g[4], const int32_t *need, int32_t nnodes) {
    int32_t valid = 0, deepest = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        if (g[q] == kNoChild) continue;
        valid++;
        if (g[q] >= 0 && g[q] < nnodes) { const int32_t d = need[g[q]]; deepest = d > deepest ? d : deepest; }
    }
    return (valid > 1 ? valid - 1 : 0) + deepest;
}

// one moved mesh of a refit, as refit_transform_kernel finds it: its run of original triangles, where the run starts among the moved
// triangles of the launch (ascending over the table), and its matrix
struct TransformDesc { int32_t first, count, begin, pad; float m[12]; };
static_assert(sizeof(TransformDesc) == 64, "one descriptor per 64 bytes");
// evplp_set_mesh_skin on the device: the skin of one triangle corner -- the vertex's four bone indices (evplp_set_mesh_skin keeps them below
// 1024) and its four weights as given.  Expanded per corner because TriAttr and the rest pose are per triangle: 72 B per triangle.
struct CornerSkin { uint16_t b[4]; float w[4]; };
static_assert(sizeof(CornerSkin) == 24, "one corner per 24 bytes");
constexpr int32_t kMaxSkinBones = 1024;
// one posed mesh of a refit, as refit_skin_kernel finds it: its run of original triangles, where the run starts among the posed triangles of
// the launch (ascending over the table), where its palette starts in the refit's bone array (in matrices) and has how many, and where its
// corner skin starts (in corners)
struct SkinDesc { int32_t first, count, begin, bone_at, nbones, skin_at, pad[2]; };
static_assert(sizeof(SkinDesc) == 32, "one descriptor per 32 bytes");
constexpr int32_t kMaxMorphTargets = 64;
// one morphed mesh of a refit, as refit_morph_kernel finds it: its run of original triangles, where the run starts among the morphed triangles
// of the launch (ascending over the table), where its weights start in the refit's weight array (in floats) and its deltas in the delta array
// (in float3: target-major, [T][3 count corners]), T, and where the result goes: 0 TriAttr::v, 1 the base array (indexed like the rest pose)
struct MorphDesc { int32_t first, count, begin, weight_at, delta_at, ntargets, to_base, pad; };
static_assert(sizeof(MorphDesc) == 32, "one descriptor per 32 bytes");

// the bound on the iterations of a build of n clusters: the search iterations, then halvings
inline int32_t ploc_iteration_bound(int32_t n, int32_t search_iterations) {
    int32_t lg = 0;
    while (((int64_t)1 << lg) < (int64_t)n) lg++;
    return search_iterations + lg;
}

// Host-side acceleration structure build result
struct BvhBuild {
    BvhNode *nodes = nullptr; int32_t nnodes = 0;
    LeafBlock *leaves = nullptr;  int32_t *tri_index = nullptr; int32_t ntris = 0;
    TriFlat *tri_flat = nullptr;
    int32_t nleaves = 0, depth = 0;
    float build_ms = 0.f;
};
// Device-side build (bvh_gpu.hip): the four arrays are device allocations handed to the caller.
struct BvhDeviceBuild {
    BvhNode *nodes = nullptr; LeafBlock *leaves = nullptr; TriFlat *tri_flat = nullptr; int32_t *tri_index = nullptr;
    int32_t nnodes = 0, nleaves = 0, ntris = 0, depth = 0;
    float build_ms = 0.f;
    int32_t iterations = 0;          // PLOC: iterations run; bound_passed: the build stopped because they passed ploc_iteration_bound
    bool bound_passed = false;
};
// verts: 9 floats per original triangle.  Degenerate triangles (rt/triangleintersect.cu:62-81
// meshBound invalidates them) are dropped.  Returns 0 on success.
int build_bvh(const float *verts, int32_t ntri, int builder, BvhBuild *out);
// box padding of both builders, as a fraction of the scene diagonal (bvh_build.cpp explains the value)
float bvh_pad_scale();
// the pad itself for a scene whose valid triangles lie in [lo, hi] (any = false: there are none)
float bvh_pad(const float lo[3], const float hi[3], bool any);
void free_bvh(BvhBuild *b);

} // namespace evplp

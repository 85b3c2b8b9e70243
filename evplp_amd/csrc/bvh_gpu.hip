// LBVH built on the device: the same flattened node / leaf-block format as the host builders (bvh_build.cpp), for scenes
// that change between frames or are too large to wait for a host build.
// Replaces OptiX's closed-source "Trbvh" acceleration build (rt/rtcomphoton/rtcomphoton.h:705-707) and the meshBound
// program (rt/triangleintersect.cu:62-81).
//
//   1. tri_setup    : per triangle its box, box centre and validity (meshBound: area > 0 and finite); scene bounds.
//   2. morton       : 63-bit Morton code of the box centre (21 bits per axis, same quantisation as the host LBVH);
//                     invalid triangles get the largest key.  hipCUB radix sort of (code, triangle) pairs (stable: equal
//                     codes keep triangle order, as std::sort of the pairs does on the host).
//   3. hierarchy    : Karras 2012 -- every internal node of the binary radix tree finds its range and split on its own
//                     (keys made unique by their position).
//   4. refit        : leaf boxes, then internal boxes bottom-up (the second thread to arrive at a node owns it).
//   3' - 4'. PLOC   : EVPLP_BVH_PLOC_GPU replaces 3 - 4 by locally-ordered clustering over the same sort (the ploc_* kernels below);
//                     5 - 6 consume its tree unchanged.
//   5. collapse     : subtrees of <= 4 triangles become leaf blocks (the walks test triangles two at a time, 4 per block);
//                     nodes with more than 4 triangles are kept and renumbered by a prefix sum.
//   6. emit         : kept nodes with both child boxes (padded, centre / half-size form), leaf blocks with the
//                     precomputed operands of the exact triangle test.
//
// Refit (evplp_refit_accel, for a tree of ANY builder whose vertices moved; the topology and the leaf assignment stay):
//   a. refit_scatter : the moved triangles' vertices from a packed staging array into TriAttr::v.
//   a'. refit_transform: the triangles of meshes moved by a matrix (evplp_transform_mesh) from their rest pose on the device into
//                      TriAttr::v, ONE launch for all such meshes of a refit (a thread finds its mesh in a small table); nothing is uploaded.
//   a''. refit_skin  : the triangles of meshes posed by bones (evplp_pose_mesh) likewise, from the rest pose, the corner skin and the refit's
//                      palettes, ONE launch for all such meshes of a refit; 48 B per bone are uploaded.
//   a*. refit_morph  : the triangles of meshes under morph weights (evplp_morph_mesh), rest pose + the weighted deltas, ONE launch for all such
//                      meshes of a refit, BEFORE a' and a'': into TriAttr::v where no matrix and no pose is in force, else into the base
//                      array, which a' and a'' then read in place of the rest pose; 4 B per target are uploaded.
//   b. refit_leaves  : every live leaf slot's operands again, in both layouts (the arithmetic emit_leaves_kernel uses).
//   c. refit_level   : the boxes, one launch per height of the tree, the parents of leaves first and the root last.  The end of a
//                      launch is the only hand-over between heights: a thread owns one node, reads its children's unpadded boxes
//                      (a leaf's from its triangles, an inner child's from a scratch array the launch before wrote), writes its own
//                      union there and the padded child boxes into its node -- padded once, from the exact union.
//   c'. refit_rotate_level: c with tree rotations (evplp_optimize_accel, evplp_set_refit_rotations; off by default): where it shrinks the box
//                      between them, a node swaps a child with a grandchild on the other side -- two node records rewritten, nothing moved.
//   d. node4         : the four-wide nodes again, into the allocation they have.
// Quality (evplp_accel_quality): accel_cost, one launch over the refit plan's order, sums the SAH cost's terms of the tree as it is.
#include "evplp_types.h"
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

namespace evplp {
namespace {

struct Bx { float lo[3], hi[3]; };

// order-preserving float <-> uint (for atomicMin / atomicMax on floats)
__device__ __forceinline__ uint32_t f2o(float f) { uint32_t u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__host__ __device__ __forceinline__ float o2f(uint32_t o) {
    uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
#ifdef __HIP_DEVICE_COMPILE__
    return __uint_as_float(u);
#else
    float f; std::memcpy(&f, &u, 4); return f;
#endif
}

// bounds[0..2] centroid lo, [3..5] centroid hi, [6..8] scene lo, [9..11] scene hi (ordered uints); bounds[12] = valid count
__global__ __launch_bounds__(256) void tri_setup_kernel(const float *verts, int ntri, Bx *tbox, uint32_t *bounds, uint8_t *valid) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    float clo[3] = { 3.0e38f, 3.0e38f, 3.0e38f }, chi[3] = { -3.0e38f, -3.0e38f, -3.0e38f }, slo[3] = { 3.0e38f, 3.0e38f, 3.0e38f }, shi[3] = { -3.0e38f, -3.0e38f, -3.0e38f };
    uint32_t ok = 0u;
    if (i < ntri) {
        const float *v = verts + 9 * (size_t)i;
        Bx t;
        for (int k = 0; k < 3; k++) { t.lo[k] = fminf(fminf(v[k], v[3 + k]), v[6 + k]); t.hi[k] = fmaxf(fmaxf(v[k], v[3 + k]), v[6 + k]); }
        tbox[i] = t;
        ok = tri_has_area(v) ? 1u : 0u;                                   // meshBound's rule (evplp_types.h)
        valid[i] = (uint8_t)ok;
        if (ok) for (int k = 0; k < 3; k++) { const float ce = 0.5f * (t.lo[k] + t.hi[k]); clo[k] = chi[k] = ce; slo[k] = t.lo[k]; shi[k] = t.hi[k]; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        for (int k = 0; k < 3; k++) {
            clo[k] = fminf(clo[k], __shfl_xor(clo[k], off)); chi[k] = fmaxf(chi[k], __shfl_xor(chi[k], off));
            slo[k] = fminf(slo[k], __shfl_xor(slo[k], off)); shi[k] = fmaxf(shi[k], __shfl_xor(shi[k], off));
        }
        ok += __shfl_xor(ok, off);
    }
    if ((threadIdx.x & 63) == 0 && ok) {
        for (int k = 0; k < 3; k++) {
            atomicMin(&bounds[k], f2o(clo[k])); atomicMax(&bounds[3 + k], f2o(chi[k]));
            atomicMin(&bounds[6 + k], f2o(slo[k])); atomicMax(&bounds[9 + k], f2o(shi[k]));
        }
        atomicAdd(&bounds[12], ok);
    }
}

__device__ __forceinline__ uint64_t expand21(uint64_t v) {
    v &= 0x1fffffull;
    v = (v | v << 32) & 0x1f00000000ffffull;
    v = (v | v << 16) & 0x1f0000ff0000ffull;
    v = (v | v << 8) & 0x100f00f00f00f00full;
    v = (v | v << 4) & 0x10c30c30c30c30c3ull;
    v = (v | v << 2) & 0x1249249249249249ull;
    return v;
}
__global__ __launch_bounds__(256) void morton_kernel(const Bx *tbox, const uint8_t *valid, int ntri, const uint32_t *bounds, uint64_t *keys, int32_t *ids) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= ntri) return;
    ids[i] = i;
    if (!valid[i]) { keys[i] = ~0ull; return; }
    uint64_t q[3];
    for (int k = 0; k < 3; k++) {
        const float lo = o2f(bounds[k]), ext = fmaxf(o2f(bounds[3 + k]) - lo, 1e-30f);
        const float c = 0.5f * (tbox[i].lo[k] + tbox[i].hi[k]);
        double t = ((double)c - (double)lo) / (double)ext;
        t = fmin(fmax(t, 0.0), 1.0);
        q[k] = (uint64_t)fmin(t * 2097152.0, 2097151.0);
    }
    keys[i] = (expand21(q[0]) << 2) | (expand21(q[1]) << 1) | expand21(q[2]);
}

// Karras 2012.  Internal node i < n - 1; a child reference is an internal index, or ~leaf for sorted position `leaf`.
__device__ __forceinline__ int delta(const uint64_t *keys, int n, int i, int j) {
    if (j < 0 || j >= n) return -1;
    const uint64_t x = keys[i] ^ keys[j];
    return x ? __clzll((long long)x) : 64 + __clz(i ^ j);
}
struct Topo { int32_t left, right, first, last; };
__global__ __launch_bounds__(256) void hierarchy_kernel(const uint64_t *keys, int n, Topo *topo, int32_t *parent_int, int32_t *parent_leaf) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n - 1) return;
    const int d = delta(keys, n, i, i + 1) - delta(keys, n, i, i - 1) >= 0 ? 1 : -1;
    const int dmin = delta(keys, n, i, i - d);
    int lmax = 2;
    while (delta(keys, n, i, i + lmax * d) > dmin) lmax *= 2;
    int l = 0;
    for (int t = lmax / 2; t >= 1; t /= 2) if (delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
    const int j = i + l * d;
    const int dnode = delta(keys, n, i, j);
    int s = 0, t = l;
    do { t = (t + 1) / 2; if (delta(keys, n, i, i + (s + t) * d) > dnode) s += t; } while (t > 1);
    const int gamma = i + s * d + min(d, 0);
    const int first = min(i, j), last = max(i, j);
    Topo tp; tp.first = first; tp.last = last;
    if (first == gamma) { tp.left = ~gamma; parent_leaf[gamma] = i; } else { tp.left = gamma; parent_int[gamma] = i; }
    if (last == gamma + 1) { tp.right = ~(gamma + 1); parent_leaf[gamma + 1] = i; } else { tp.right = gamma + 1; parent_int[gamma + 1] = i; }
    topo[i] = tp;
    if (i == 0) parent_int[0] = -1;
}

// a box another workgroup (possibly on another XCD) wrote before it bumped the visit counter: loads that bypass this CU's L1
__device__ __forceinline__ Bx load_box_agent(const Bx *p) {
    Bx b;
    for (int k = 0; k < 3; k++) {
        b.lo[k] = __hip_atomic_load(&p->lo[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        b.hi[k] = __hip_atomic_load(&p->hi[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return b;
}
// bottom-up boxes; also the height of the tree in KEPT nodes (more than 4 triangles), carried up with the boxes: the second
// arrival at a node owns it and takes max(children) + 1.  (Round 2 let every leaf thread walk its whole ancestor chain to count:
// O(n depth), quadratic on the long chains that clustered or duplicate Morton codes produce.)
__global__ __launch_bounds__(256) void refit_kernel(const Bx *tbox, const int32_t *ids, int n, const Topo *topo, const int32_t *parent_int, const int32_t *parent_leaf,
                                                    Bx *lbox, Bx *ibox, uint32_t *visits, uint32_t *height, uint32_t *max_depth) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    Bx b = tbox[ids[j]];
    lbox[j] = b;
    if (n == 1) return;
    __threadfence();
    int cur = parent_leaf[j];
    while (cur >= 0) {
        if (atomicAdd(&visits[cur], 1u) == 0u) break;                    // the first arrival leaves; its subtree is complete and visible
        __threadfence();
        const Topo tp = topo[cur];
        const Bx l = load_box_agent(tp.left < 0 ? &lbox[~tp.left] : &ibox[tp.left]), r = load_box_agent(tp.right < 0 ? &lbox[~tp.right] : &ibox[tp.right]);
        const uint32_t hl = tp.left < 0 ? 0u : __hip_atomic_load(&height[tp.left], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t hr = tp.right < 0 ? 0u : __hip_atomic_load(&height[tp.right], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t h = max(hl, hr) + (tp.last - tp.first + 1 > kMaxLeafTris ? 1u : 0u);
        Bx u;
        for (int k = 0; k < 3; k++) { u.lo[k] = fminf(l.lo[k], r.lo[k]); u.hi[k] = fmaxf(l.hi[k], r.hi[k]); }
        ibox[cur] = u;
        height[cur] = h;
        __threadfence();
        const int up = parent_int[cur];
        if (up < 0) *max_depth = h;                                       // the root: one writer
        cur = up;
    }
}

// kept[i] = node i has more than 4 triangles; head[p] = triangles of the leaf block that starts at sorted position p (0: none)
__global__ __launch_bounds__(256) void collapse_kernel(const Topo *topo, int n, uint32_t *kept, uint32_t *head) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n - 1) return;
    const Topo tp = topo[i];
    const bool k = tp.last - tp.first + 1 > kMaxLeafTris;
    kept[i] = k ? 1u : 0u;
    if (!k) { if (i == 0) head[0] = (uint32_t)n; return; }            // (the whole tree is one block)
    const int32_t ch[2] = { tp.left, tp.right };
    for (int s = 0; s < 2; s++) {
        if (ch[s] < 0) head[~ch[s]] = 1u;
        else { const Topo c = topo[ch[s]]; const int cnt = c.last - c.first + 1; if (cnt <= kMaxLeafTris) head[c.first] = (uint32_t)cnt; }
    }
}
__global__ __launch_bounds__(256) void flag_kernel(const uint32_t *head, int n, uint32_t *flag) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) flag[i] = head[i] ? 1u : 0u;
}

__device__ __forceinline__ void set_box(BvhNode &f, int child, const Bx &b, float pad) {
#pragma clang fp contract(off)
    for (int k = 0; k < 3; k++) {
        const float lo = b.lo[k] - pad, hi = b.hi[k] + pad;
        const float c = 0.5f * (lo + hi);
        float h = fmaxf(hi - c, c - lo);
        h = h + fabsf(h) * 1e-6f + 1e-30f;
        f.ctr[k][child] = c; f.hal[k][child] = h;
    }
}
__global__ __launch_bounds__(256) void emit_nodes_kernel(const Topo *topo, int n, const uint32_t *kept, const uint32_t *new_id, const uint32_t *head, const uint32_t *block_id,
                                                         const Bx *lbox, const Bx *ibox, const uint32_t *bounds, float pad_scale, BvhNode *nodes) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const float dx = o2f(bounds[9]) - o2f(bounds[6]), dy = o2f(bounds[10]) - o2f(bounds[7]), dz = o2f(bounds[11]) - o2f(bounds[8]);
    float coord = 0.f;
    for (int k = 0; k < 3; k++) coord = fmaxf(coord, fmaxf(fabsf(o2f(bounds[6 + k])), fabsf(o2f(bounds[9 + k]))));
    const float pad = pad_scale * fmaxf(sqrtf(dx * dx + dy * dy + dz * dz), coord) + 1e-30f;
    if (n - 1 < 1 || !kept[0]) {
        // at most 4 triangles: a root with the block as its only child
        if (i == 0) {
            BvhNode f; for (int k = 0; k < 3; k++) { f.ctr[k][1] = 0.f; f.hal[k][1] = -3.0e38f; }
            set_box(f, 0, n == 1 ? lbox[0] : ibox[0], pad);
            f.c0 = ~((0 << 2) | (n - 1)); f.c1 = kNoChild; f.pad[0] = f.pad[1] = 0;
            nodes[0] = f;
        }
        return;
    }
    if (i >= n - 1 || !kept[i]) return;
    const Topo tp = topo[i];
    BvhNode f; f.pad[0] = f.pad[1] = 0;
    const int32_t ch[2] = { tp.left, tp.right };
    int32_t ref[2];
    for (int s = 0; s < 2; s++) {
        if (ch[s] < 0) { set_box(f, s, lbox[~ch[s]], pad); ref[s] = ~((int32_t)(block_id[~ch[s]] << 2) | 0); }
        else {
            set_box(f, s, ibox[ch[s]], pad);
            if (kept[ch[s]]) ref[s] = (int32_t)new_id[ch[s]];
            else { const int first = topo[ch[s]].first; ref[s] = ~((int32_t)(block_id[first] << 2) | (int32_t)(head[first] - 1u)); }
        }
    }
    f.c0 = ref[0]; f.c1 = ref[1];
    nodes[new_id[i]] = f;
}
// The operands of the exact triangle test of one leaf slot, in both layouts: the same operation order as the host builder and the
// oracle's tri_test: e0 = p1-p0, e1 = p0-p2, n = cross(e1, e0).  live = false: all zero (den = 0 -> the test is false).
__device__ __forceinline__ void store_operands(const float *v, bool live, size_t slot, LeafBlock *leaves, TriFlat *tri_flat) {
#pragma clang fp contract(off)
    float p0[3] = { 0.f, 0.f, 0.f }, e0[3] = { 0.f, 0.f, 0.f }, e1[3] = { 0.f, 0.f, 0.f }, nn[3] = { 0.f, 0.f, 0.f };
    if (live) {
        for (int c = 0; c < 3; c++) { p0[c] = v[c]; e0[c] = v[3 + c] - v[c]; e1[c] = v[c] - v[6 + c]; }
        nn[0] = e1[1] * e0[2] - e1[2] * e0[1]; nn[1] = e1[2] * e0[0] - e1[0] * e0[2]; nn[2] = e1[0] * e0[1] - e1[1] * e0[0];
    }
    TriPair &tp = leaves[slot >> 2].pair[(slot >> 1) & 1]; const int h = (int)(slot & 1);
    TriFlat &tf = tri_flat[slot];
    for (int c = 0; c < 3; c++) {
        tp.p0[c][h] = p0[c]; tp.e0[c][h] = e0[c]; tp.e1[c][h] = e1[c]; tp.n[c][h] = nn[c];
        tf.p0[c] = p0[c]; tf.e0[c] = e0[c]; tf.e1[c] = e1[c]; tf.n[c] = nn[c];
    }
}
__global__ __launch_bounds__(256) void emit_leaves_kernel(const float *verts, const int32_t *ids, int n, const uint32_t *head, const uint32_t *block_id,
                                                          LeafBlock *leaves, TriFlat *tri_flat, int32_t *tri_index) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n || !head[p]) return;
    const uint32_t blk = block_id[p], cnt = head[p];
    for (uint32_t k = 0; k < (uint32_t)kMaxLeafTris; k++) {
        const size_t slot = 4 * (size_t)blk + k;
        if (k >= cnt) { tri_index[slot] = -1; continue; }
        const int32_t tri = ids[p + k];
        tri_index[slot] = tri;
        store_operands(verts + 9 * (size_t)tri, true, slot, leaves, tri_flat);
    }
}

// ---- PLOC (EVPLP_BVH_PLOC_GPU): steps 3 - 4 by locally-ordered clustering instead of the radix tree.  The n sorted valid triangles are the
// first clusters (position p: reference ~p, its triangle's box).  One iteration over c clusters is four launches and nothing else hands
// over: ploc_nn (search iterations only) finds every position's nearest neighbour within `radius` positions; ploc_merge flags the mutual
// pairs (the lower position of a pair merges, the upper is vacated); one exclusive scan of the packed flags (low word merges, high word
// survivors) numbers both; ploc_scatter writes the new nodes -- m merges among c clusters get indices c - 1 - m + rank, so the last merge
// of the build is node 0 -- and the surviving clusters in position order into the other half of the ping-pong.  The host reads c back.
// ploc_place then gives every leaf and inner node its first position in the tree's own left-to-right order (up its parent chain: + the
// left sibling's triangles wherever it is a right child) and fills what stages 5 - 6 consume.  host/ploc.cpp states the same serially.
struct PlocKids { int32_t left, right; };
__device__ __forceinline__ int32_t ploc_partner(const int32_t *nn, int pairing, int i, int c) { return pairing ? ((i ^ 1) < c ? (i ^ 1) : i) : nn[i]; }
__device__ __forceinline__ int32_t ploc_count(const int32_t *ncnt, int32_t ref) { return ref < 0 ? 1 : ncnt[ref]; }

__global__ __launch_bounds__(256) void ploc_init_kernel(const Bx *tbox, const int32_t *ids, int n, int32_t *cref, Bx *cbox) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    cref[p] = ~p;
    cbox[p] = tbox[ids[p]];
}
// the workgroup's 256 positions and `radius` on either side, staged once (component by component: a wavefront reads 64 consecutive words)
__global__ __launch_bounds__(256) void ploc_nn_kernel(const Bx *cbox, int c, int radius, int32_t *nn) {
#pragma clang fp contract(off)
    __shared__ float tile[6][256 + 2 * kPlocMaxRadius];
    const int tid = (int)threadIdx.x, base = (int)blockIdx.x * 256 - radius;
    for (int t = tid; t < 256 + 2 * radius; t += 256) {
        const int p = base + t;
        if (p >= 0 && p < c) { const Bx b = cbox[p]; for (int k = 0; k < 3; k++) { tile[k][t] = b.lo[k]; tile[3 + k][t] = b.hi[k]; } }
    }
    __syncthreads();
    const int i = base + radius + tid;
    if (i >= c) return;
    float own[6];
    for (int k = 0; k < 6; k++) own[k] = tile[k][tid + radius];
    float best = 0.f; int bj = -1;
    const int j0 = max(0, i - radius), j1 = min(c - 1, i + radius);
    for (int j = j0; j <= j1; j++) {
        if (j == i) continue;
        float other[6];
        for (int k = 0; k < 6; k++) other[k] = tile[k][j - base];
        const float d = ploc_distance(own, other);
        if (bj < 0 || d < best) { best = d; bj = j; }                        // ties keep the lowest j: the globally closest pair is always mutual
    }
    nn[i] = bj < 0 ? i : bj;
}
// flags[i] = (position i survives) << 32 | (position i is the lower one of a mutual pair)
__global__ __launch_bounds__(256) void ploc_merge_kernel(const int32_t *nn, int pairing, int c, unsigned long long *flags) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= c) return;
    const int32_t j = ploc_partner(nn, pairing, i, c);
    const bool merged = j != i && j >= 0 && j < c && ploc_partner(nn, pairing, j, c) == i;
    flags[i] = ((unsigned long long)((!merged || i < j) ? 1u : 0u) << 32) | (unsigned long long)((merged && i < j) ? 1u : 0u);
}
// scan = the exclusive sums of flags.  Only the lower position of a pair writes its node.  scal[0] = the root's height in kept nodes, scal[1] = c after this iteration
__global__ __launch_bounds__(256) void ploc_scatter_kernel(const int32_t *nn, int pairing, int c, int n, const unsigned long long *flags, const unsigned long long *scan,
                                                           const int32_t *cref_in, const Bx *cbox_in, int32_t *cref_out, Bx *cbox_out, PlocKids *kids, Bx *ibox,
                                                           int32_t *ncnt, uint32_t *height, int32_t *parent_int, int32_t *parent_leaf, uint32_t *scal) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= c) return;
    const unsigned long long total = scan[c - 1] + flags[c - 1], f = flags[i], s = scan[i];
    const int m = (int)(uint32_t)total, cn = (int)(total >> 32);
    if (i == c - 1) scal[1] = (uint32_t)cn;
    if (!(f >> 32)) return;
    const int pos = (int)(s >> 32);
    if (pos >= cn) return;
    int32_t ref = cref_in[i];
    Bx box = cbox_in[i];
    if (f & 1ull) {
        const int32_t j = ploc_partner(nn, pairing, i, c), idx = c - 1 - m + (int)(uint32_t)s;
        if (j < 0 || j >= c || idx < 0 || idx > n - 2) return;
        const int32_t rref = cref_in[j];
        const Bx rb = cbox_in[j];
        for (int k = 0; k < 3; k++) { box.lo[k] = fminf(box.lo[k], rb.lo[k]); box.hi[k] = fmaxf(box.hi[k], rb.hi[k]); }
        const int32_t cnt = ploc_count(ncnt, ref) + ploc_count(ncnt, rref);
        const uint32_t hl = ref < 0 ? 0u : height[ref], hr = rref < 0 ? 0u : height[rref];
        const uint32_t h = max(hl, hr) + (cnt > kMaxLeafTris ? 1u : 0u);     // (what refit_kernel carries up)
        PlocKids kd; kd.left = ref; kd.right = rref;
        kids[idx] = kd; ibox[idx] = box; ncnt[idx] = cnt; height[idx] = h;
        if (ref < 0) parent_leaf[~ref] = idx; else parent_int[ref] = idx;
        if (rref < 0) parent_leaf[~rref] = idx; else parent_int[rref] = idx;
        if (idx == 0) { parent_int[0] = -1; scal[0] = h; }
        ref = idx;
    }
    cref_out[pos] = ref;
    cbox_out[pos] = box;
}
// thread t < n: the leaf at sorted position t; t >= n: inner node t - n.  ids_out / lbox in tree order, topo as the radix tree's
__global__ __launch_bounds__(256) void ploc_place_kernel(int n, const PlocKids *kids, const int32_t *ncnt, const int32_t *parent_int, const int32_t *parent_leaf,
                                                         const int32_t *ids, const Bx *tbox, int32_t *ids_out, Bx *lbox, Topo *topo) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= 2 * n - 1) return;
    const bool leaf = t < n;
    int32_t me = leaf ? ~t : t - n, up = leaf ? (n > 1 ? parent_leaf[t] : -1) : parent_int[t - n];
    int32_t first = 0;
    for (int step = 0; up >= 0 && up < n - 1 && step < n; step++) {       // (the chain is as long as the binary tree is high)
        const PlocKids kd = kids[up];
        if (kd.right == me) first += ploc_count(ncnt, kd.left);
        me = up; up = parent_int[up];
    }
    if (first < 0 || first >= n) return;
    if (leaf) { const int32_t tri = ids[t]; ids_out[first] = tri; lbox[first] = tbox[tri]; return; }
    const PlocKids kd = kids[t - n];
    const int32_t cl = ploc_count(ncnt, kd.left);
    Topo tp;
    tp.left = kd.left < 0 ? ~first : kd.left; tp.right = kd.right < 0 ? ~(first + cl) : kd.right;
    tp.first = first; tp.last = first + ncnt[t - n] - 1;
    topo[t - n] = tp;
}

// ---- refit
// a. src: 9 floats per triangle of the run [first, first + count) of original triangles
__global__ __launch_bounds__(256) void refit_scatter_kernel(const float *src, int32_t first, int32_t count, TriAttr *attrs) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 9 * count) return;
    attrs[(size_t)first + (size_t)(i / 9)].v[i % 9] = src[i];
}
// a'. the rest pose of a mesh that is transformed for the first time, from what the device holds: the reverse of refit_scatter_kernel
// (rest: 9 floats per original triangle of the scene)
__global__ __launch_bounds__(256) void refit_rest_kernel(const TriAttr *attrs, int32_t first, int32_t count, float *rest) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 9 * count) return;
    rest[9 * (size_t)first + (size_t)i] = attrs[(size_t)first + (size_t)(i / 9)].v[i % 9];
}
// One thread per vertex of the moved triangles of ALL meshes of the table (total of them): the last descriptor whose run begins at or
// before the thread's triangle is its mesh.  Reads the rest pose, writes TriAttr::v; the rest pose is never written here.
__global__ __launch_bounds__(256) void refit_transform_kernel(const TransformDesc *table, int32_t nmesh, int32_t total, const float *rest, TriAttr *attrs, int32_t ntri) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int j = i / 3, p = i - 3 * j;
    if (j >= total) return;
    int lo = 0, hi = nmesh - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].begin <= j) lo = mid; else hi = mid - 1;
    }
    const int32_t tri = table[lo].first + (j - table[lo].begin);
    if (tri < 0 || tri >= ntri) return;
    transform_point(table[lo].m, rest + 9 * (size_t)tri + 3 * p, attrs[tri].v + 3 * p);
}
// The same for the meshes posed by bones (evplp_pose_mesh): one thread per corner of the posed triangles of ALL meshes of the table, its mesh
// found by the same bisection.  Reads the rest pose, the corner's four indices and weights (skin: nskin corners) and four matrices of the
// mesh's palette (bones: the refit's palettes one behind the other; a gather from at most 48 KB per mesh, which stays in cache), writes
// TriAttr::v through skin_point; the rest pose is never written here.  evplp_set_mesh_skin keeps every index below the mesh's bone count;
// an index at or beyond it reads bone 0 of the mesh rather than memory past the palette.
__global__ __launch_bounds__(256) void refit_skin_kernel(const SkinDesc *table, int32_t nmesh, int32_t total, const float *rest, const CornerSkin *skin, int32_t nskin, const float *bones,
                                                         TriAttr *attrs, int32_t ntri) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int j = i / 3, p = i - 3 * j;
    if (j >= total) return;
    int lo = 0, hi = nmesh - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].begin <= j) lo = mid; else hi = mid - 1;
    }
    const SkinDesc d = table[lo];
    const int32_t tri = d.first + (j - d.begin), corner = d.skin_at + 3 * (j - d.begin) + p;
    if (j - d.begin >= d.count || tri < 0 || tri >= ntri || corner < 0 || corner >= nskin) return;      // (count: a bad table cannot reach a neighbour's triangles)
    const CornerSkin s = skin[corner];
    int32_t b[4];
    for (int k = 0; k < 4; k++) b[k] = (int32_t)s.b[k] < d.nbones ? (int32_t)s.b[k] : 0;
    skin_point(bones + 12 * (size_t)d.bone_at, b, s.w, rest + 9 * (size_t)tri + 3 * p, attrs[tri].v + 3 * p);
}
// Morph targets (evplp_morph_mesh): one thread per corner of the morphed triangles of ALL meshes of the table, its mesh found by the same
// bisection; launched before the two launches above, which then read the base array in place of the rest pose.  Reads the rest pose, the
// mesh's T weights (weights: the refit's weight sets one behind the other, nweights floats) and the corner's T deltas (deltas: ndelta float3,
// per mesh target-major [T][3 count], so that neighbouring threads read neighbouring 12 bytes of one target's plane), and writes through
// morph_point either TriAttr::v (a mesh with no matrix and no pose in force) or the base array (indexed like the rest pose).  A descriptor
// whose weights or deltas would lie outside their arrays writes nothing.
__global__ __launch_bounds__(256) void refit_morph_kernel(const MorphDesc *table, int32_t nmesh, int32_t total, const float *rest, const float *weights, int32_t nweights, const float *deltas,
                                                          int64_t ndelta, float *base, TriAttr *attrs, int32_t ntri) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int j = i / 3, p = i - 3 * j;
    if (j >= total) return;
    int lo = 0, hi = nmesh - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].begin <= j) lo = mid; else hi = mid - 1;
    }
    const MorphDesc d = table[lo];
    const int32_t tri = d.first + (j - d.begin);
    if (j - d.begin >= d.count || j < d.begin || tri < 0 || tri >= ntri) return;                             // (count: a bad table cannot reach a neighbour's triangles)
    const int64_t plane = 3 * (int64_t)d.count;                                                              // (one target's plane of the mesh, in float3)
    if (d.ntargets < 1 || d.ntargets > kMaxMorphTargets || d.weight_at < 0 || d.weight_at + d.ntargets > nweights || d.delta_at < 0 || d.delta_at + d.ntargets * plane > ndelta) return;
    const size_t at = 9 * (size_t)tri + 3 * p;
    float *out = d.to_base ? base + at : attrs[tri].v + 3 * p;
    morph_point(rest + at, deltas + 3 * ((size_t)d.delta_at + 3 * (size_t)(j - d.begin) + p), (size_t)(3 * plane), weights + d.weight_at, d.ntargets, out);
}
// b. one thread per leaf slot.  A triangle that has become degenerate (tri_has_area: meshBound's rule) gets zero operands, which is what a
// fresh build does by dropping it; an empty slot (tri_index < 0) is zero already and stays.
__global__ __launch_bounds__(256) void refit_leaves_kernel(const int32_t *tri_index, int32_t nslots, const TriAttr *attrs, int32_t ntri, LeafBlock *leaves, TriFlat *tri_flat) {
    const int slot = blockIdx.x * 256 + threadIdx.x;
    if (slot >= nslots) return;
    const int32_t tri = tri_index[slot];
    if (tri < 0 || tri >= ntri) return;
    const float *v = attrs[tri].v;
    store_operands(v, tri_has_area(v), (size_t)slot, leaves, tri_flat);
}
// c. one thread per node of one height (order[0 .. count)); boxes[i] = the unpadded box of everything under node i
__global__ __launch_bounds__(256) void refit_level_kernel(BvhNode *nodes, int32_t nnodes, const int32_t *order, int32_t count, const int32_t *tri_index, int32_t nslots,
                                                          const TriAttr *attrs, int32_t ntri, Bx *boxes, float pad) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= count) return;
    const int32_t i = order[t];
    if (i < 0 || i >= nnodes) return;
    BvhNode f = nodes[i];
    Bx u;
    for (int k = 0; k < 3; k++) { u.lo[k] = 3.0e38f; u.hi[k] = -3.0e38f; }
    const int32_t ch[2] = { f.c0, f.c1 };
    for (int s = 0; s < 2; s++) {
        if (ch[s] == kNoChild) continue;                                  // (ctr = 0, hal = -3e38 as the builder left them)
        Bx b;
        for (int k = 0; k < 3; k++) { b.lo[k] = 3.0e38f; b.hi[k] = -3.0e38f; }
        if (ch[s] >= 0) { if (ch[s] < nnodes) b = boxes[ch[s]]; }
        else {
            const int32_t id = ~ch[s], cnt = (id & 3) + 1;
            for (int32_t q = 0; q < cnt; q++) {
                const int32_t slot = (id & ~3) + q;
                const int32_t tri = slot < nslots ? tri_index[slot] : -1;
                if (tri < 0 || tri >= ntri) continue;
                const float *v = attrs[tri].v;
                if (!tri_has_area(v)) continue;
                for (int k = 0; k < 3; k++) { b.lo[k] = fminf(b.lo[k], fminf(fminf(v[k], v[3 + k]), v[6 + k])); b.hi[k] = fmaxf(b.hi[k], fmaxf(fmaxf(v[k], v[3 + k]), v[6 + k])); }
            }
        }
        set_box(f, s, b, pad);
        for (int k = 0; k < 3; k++) { u.lo[k] = fminf(u.lo[k], b.lo[k]); u.hi[k] = fmaxf(u.hi[k], b.hi[k]); }
    }
    boxes[i] = u;
    nodes[i] = f;
}

// c'. the same sweep with tree rotations (evplp_optimize_accel, evplp_set_refit_rotations): one thread per node N of one level of the PLAN.
// It does what refit_level_kernel does and, where rotate_choice (evplp_types.h) finds a gain, swaps a child A of N with a grandchild G on the
// other side: N.c[s] = G, B.c[q] = A, boxes[B] = A u K.  The thread that owns N writes N and its child B and nobody else touches either in
// this launch: a rotation needs level(A) < level(B) in the plan, so every parent keeps a strictly higher plan level than its children, the
// nodes of one launch are never parent and child, and the end of the launch stays the only hand-over.  (The plan's levels are no tight
// heights after a rotation; nothing needs them to be.)  Two more values ride up the sweep: taken[i] = the rotations in the subtree of i in
// this pass, need[i] = the four-wide walk's stack need of i; the root's pair goes to root_out.
// The exact box under a child reference, as refit_level_kernel forms it: an inner node's from the scratch, a leaf's from its live triangles.
__device__ __forceinline__ void rotate_ref_box(int32_t ref, int32_t nnodes, const Bx *boxes, const int32_t *tri_index, int32_t nslots, const TriAttr *attrs, int32_t ntri, float *out) {
    Bx b;
    for (int k = 0; k < 3; k++) { b.lo[k] = 3.0e38f; b.hi[k] = -3.0e38f; }
    if (ref >= 0) { if (ref < nnodes) b = boxes[ref]; }
    else if (ref != kNoChild) {
        const int32_t id = ~ref, cnt = (id & 3) + 1;
        for (int32_t q = 0; q < cnt; q++) {
            const int32_t slot = (id & ~3) + q;
            const int32_t tri = slot < nslots ? tri_index[slot] : -1;
            if (tri < 0 || tri >= ntri) continue;
            const float *v = attrs[tri].v;
            if (!tri_has_area(v)) continue;
            for (int k = 0; k < 3; k++) { b.lo[k] = fminf(b.lo[k], fminf(fminf(v[k], v[3 + k]), v[6 + k])); b.hi[k] = fmaxf(b.hi[k], fmaxf(fmaxf(v[k], v[3 + k]), v[6 + k])); }
        }
    }
    for (int k = 0; k < 3; k++) { out[k] = b.lo[k]; out[3 + k] = b.hi[k]; }
}
__device__ __forceinline__ void rotate_set_box(BvhNode &f, int child, const float *b6, float pad) {
    Bx b;
    for (int k = 0; k < 3; k++) { b.lo[k] = b6[k]; b.hi[k] = b6[3 + k]; }
    set_box(f, child, b, pad);
}
// the two child references of inner node i (kNoChild twice for anything else)
__device__ __forceinline__ void rotate_kids(const BvhNode *nodes, int32_t nnodes, int32_t i, int32_t out[2]) {
    out[0] = out[1] = kNoChild;
    if (i >= 0 && i < nnodes) { out[0] = nodes[i].c0; out[1] = nodes[i].c1; }
}
__global__ __launch_bounds__(256) void refit_rotate_level_kernel(BvhNode *nodes, int32_t nnodes, const int32_t *order, int32_t count, const int32_t *tri_index, int32_t nslots,
                                                                 const TriAttr *attrs, int32_t ntri, Bx *boxes, float pad, const int32_t *level, int32_t *taken, int32_t *need,
                                                                 int32_t *root_out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= count) return;
    const int32_t i = order[t];
    if (i < 0 || i >= nnodes) return;
    BvhNode f = nodes[i];
    int32_t ref[2] = { f.c0, f.c1 }, lvl[2], gref[2][2];
    float box[2][6], gbox[2][2][6];
#pragma unroll
    for (int s = 0; s < 2; s++) {
        rotate_ref_box(ref[s], nnodes, boxes, tri_index, nslots, attrs, ntri, box[s]);
        lvl[s] = ref[s] >= 0 && ref[s] < nnodes ? level[ref[s]] : -1;
        rotate_kids(nodes, nnodes, ref[s], gref[s]);
#pragma unroll
        for (int q = 0; q < 2; q++) rotate_ref_box(gref[s][q], nnodes, boxes, tri_index, nslots, attrs, ntri, gbox[s][q]);
    }
    const int pick = rotate_choice(ref, lvl, box, gref, gbox);
    int32_t own = 0, sub[2];                                          // sub[s] = taken[] of child slot s
#pragma unroll
    for (int s = 0; s < 2; s++) sub[s] = ref[s] >= 0 && ref[s] < nnodes ? taken[ref[s]] : 0;
    int32_t g4[4];                                                    // what node4 will put in N's four slots
#pragma unroll
    for (int s = 0; s < 2; s++) {
        if (ref[s] >= 0) { g4[2 * s] = gref[s][0]; g4[2 * s + 1] = gref[s][1]; }
        else { g4[2 * s] = ref[s]; g4[2 * s + 1] = kNoChild; }
    }
#pragma unroll
    for (int s = 0; s < 2; s++) {
#pragma unroll
        for (int q = 0; q < 2; q++) {
            if (pick != 2 * s + q) continue;
            const int32_t a = ref[s], b = ref[1 - s], g = gref[1 - s][q], k = gref[1 - s][1 - q];
            // B: slot q takes A (padded from A's exact box), slot 1 - q keeps K and the bytes B's own thread wrote in an earlier launch
            BvhNode fb = nodes[b];
            if (q == 0) fb.c0 = a; else fb.c1 = a;
            rotate_set_box(fb, q, box[s], pad);
            nodes[b] = fb;
            float ub[6];
            if (q == 0) rotate_union(box[s], gbox[1 - s][1], ub); else rotate_union(gbox[1 - s][0], box[s], ub);
            Bx bb;
            for (int c = 0; c < 3; c++) { bb.lo[c] = ub[c]; bb.hi[c] = ub[3 + c]; }
            boxes[b] = bb;
            // B's own count and need over its new children A and K
            int32_t ka[2] = { gref[s][0], gref[s][1] }, kk[2], kg[2];
            rotate_kids(nodes, nnodes, k, kk);
            rotate_kids(nodes, nnodes, g, kg);
            int32_t gb[4];
            if (a >= 0) { gb[0] = ka[0]; gb[1] = ka[1]; } else { gb[0] = a; gb[1] = kNoChild; }
            if (k >= 0) { gb[2] = kk[0]; gb[3] = kk[1]; } else { gb[2] = k; gb[3] = kNoChild; }
            const int32_t need_b = rotate_need(gb, need, nnodes);
            need[b] = need_b;
            const int32_t taken_b = sub[1 - s] - (g >= 0 && g < nnodes ? taken[g] : 0) + sub[s];
            taken[b] = taken_b;
            // N: slot s takes G, slot 1 - s keeps B with its new box
            if (g >= 0) { g4[2 * s] = kg[0]; g4[2 * s + 1] = kg[1]; } else { g4[2 * s] = g; g4[2 * s + 1] = kNoChild; }
            g4[2 * (1 - s)] = q == 0 ? a : k; g4[2 * (1 - s) + 1] = q == 0 ? k : a;
            sub[s] = g >= 0 && g < nnodes ? taken[g] : 0; sub[1 - s] = taken_b;
            ref[s] = g;
            for (int c = 0; c < 6; c++) { box[s][c] = gbox[1 - s][q][c]; box[1 - s][c] = ub[c]; }
            own = 1;
        }
    }
    f.c0 = ref[0]; f.c1 = ref[1];
#pragma unroll
    for (int s = 0; s < 2; s++) {
        if (ref[s] == kNoChild) continue;                                 // (ctr = 0, hal = -3e38 as the builder left them)
        rotate_set_box(f, s, box[s], pad);
    }
    float un[6];
    rotate_union(box[0], box[1], un);
    Bx u;
    for (int c = 0; c < 3; c++) { u.lo[c] = un[c]; u.hi[c] = un[3 + c]; }
    boxes[i] = u;
    nodes[i] = f;
    const int32_t taken_n = own + sub[0] + sub[1], need_n = rotate_need(g4, need, nnodes);
    taken[i] = taken_n; need[i] = need_n;
    if (i == 0) { root_out[0] = taken_n; root_out[1] = need_n; }
}

// node4[i] from binary node i: child s of i, if it is an inner node, is replaced by ITS two children (their boxes are stored in
// that child's own record); a leaf or absent child stays.  lo / hi are computed exactly as the binary per-lane walk computes them.
__global__ __launch_bounds__(256) void node4_kernel(const BvhNode *nodes, int n, BvhNode4 *out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const BvhNode b = nodes[i];
    BvhNode4 r;
    for (int q = 0; q < 4; q++) { r.child[q] = kNoChild; r.pad[q] = 0; for (int k = 0; k < 3; k++) { r.lo[k][q] = 3.0e38f; r.hi[k][q] = -3.0e38f; } }
    const int32_t ch[2] = { b.c0, b.c1 };
    for (int s = 0; s < 2; s++) {
        if (ch[s] >= 0) {
            const BvhNode c = nodes[ch[s]];
            const int32_t gc[2] = { c.c0, c.c1 };
            for (int q = 0; q < 2; q++) {
                r.child[2 * s + q] = gc[q];
                for (int k = 0; k < 3; k++) { r.lo[k][2 * s + q] = c.ctr[k][q] - c.hal[k][q]; r.hi[k][2 * s + q] = c.ctr[k][q] + c.hal[k][q]; }
            }
        } else if (ch[s] != kNoChild) {
            r.child[2 * s] = ch[s];
            for (int k = 0; k < 3; k++) { r.lo[k][2 * s] = b.ctr[k][s] - b.hal[k][s]; r.hi[k][2 * s] = b.ctr[k][s] + b.hal[k][s]; }
        }
    }
    out[i] = r;
}

// ---- the SAH cost of the tree as it is (evplp_accel_quality).  Thread i of workgroup k takes entry 256 k + i of the refit plan's order
// (every node the root reaches, once) and reads that node's 64 bytes alone: the leaf counts are in the references.  The three sums of a
// workgroup are added in one fixed shape, reduce_row's (kernels_stats.hip): shuffle-down by 32 .. 1 in each wavefront, lane 0 of each to
// LDS, thread 0 adds waves 0 .. 3 in order and writes out[1 + 3 k ..]; the thread that holds node 0 writes the root's area to out[0].
// Entries past the end add +0.0.  The host adds the workgroups' triples in index order after the launch, which is the only hand-over.
__global__ __launch_bounds__(kCostChunk) void accel_cost_kernel(const BvhNode *nodes, int32_t nnodes, const int32_t *order, int32_t count, double *out) {
    __shared__ double wave_sums[kCostChunk / 64][3];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int e = (int)blockIdx.x * kCostChunk + tid;
    double s[3] = { 0.0, 0.0, 0.0 };
    if (e < count) {
        const int32_t i = order[e];
        if (i >= 0 && i < nnodes) {
            const BvhNode f = nodes[i];
            accel_cost_terms(f, s);
            if (i == 0) out[0] = accel_root_area(f);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++)
        for (int off = 32; off > 0; off >>= 1) s[k] += __shfl_down(s[k], off, 64);
    if (lane == 0) for (int k = 0; k < 3; k++) wave_sums[wave][k] = s[k];
    __syncthreads();
    if (tid == 0)
        for (int k = 0; k < 3; k++) {
            double t = wave_sums[0][k];
            for (int w = 1; w < kCostChunk / 64; w++) t += wave_sums[w][k];
            out[1 + 3 * (size_t)blockIdx.x + k] = t;
        }
}

#define GB_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { err = e_; goto done; } } while (0)

} // namespace

// The four-wide nodes of a flattened binary tree that is already on the device (all builders), into an allocation of nnodes of them: enqueued, no wait.
void build_nodes4_into(const BvhNode *d_nodes, int32_t nnodes, hipStream_t stream, BvhNode4 *out) {
    if (nnodes > 0) hipLaunchKernelGGL(node4_kernel, dim3((unsigned)((nnodes + 255) / 256)), dim3(256), 0, stream, d_nodes, nnodes, out);
}
// ... into a device allocation of its own (*out), complete when the call returns
int build_nodes4(const BvhNode *d_nodes, int32_t nnodes, hipStream_t stream, BvhNode4 **out) {
    BvhNode4 *p = nullptr;
    hipError_t e = hipMalloc((void **)&p, sizeof(BvhNode4) * (size_t)std::max(nnodes, 1));
    if (e != hipSuccess) return (int)e;
    build_nodes4_into(d_nodes, nnodes, stream, p);
    e = hipStreamSynchronize(stream);
    if (e != hipSuccess) { hipFree(p); return (int)e; }
    *out = p;
    return 0;
}

// The refit's launches (context.cpp evplp_refit_accel owns the memory and the order); all enqueued, none waits.
void refit_scatter(const float *d_src, int32_t first, int32_t count, TriAttr *attrs, hipStream_t stream) {
    if (count > 0) hipLaunchKernelGGL(refit_scatter_kernel, dim3((unsigned)((9 * (size_t)count + 255) / 256)), dim3(256), 0, stream, d_src, first, count, attrs);
}
void refit_rest(const TriAttr *attrs, int32_t first, int32_t count, float *d_rest, hipStream_t stream) {
    if (count > 0) hipLaunchKernelGGL(refit_rest_kernel, dim3((unsigned)((9 * (size_t)count + 255) / 256)), dim3(256), 0, stream, attrs, first, count, d_rest);
}
void refit_transform(const TransformDesc *d_table, int32_t nmesh, int32_t total, const float *d_rest, TriAttr *attrs, int32_t ntri, hipStream_t stream) {
    if (nmesh > 0 && total > 0) hipLaunchKernelGGL(refit_transform_kernel, dim3((unsigned)((3 * (size_t)total + 255) / 256)), dim3(256), 0, stream, d_table, nmesh, total, d_rest, attrs, ntri);
}
void refit_skin(const SkinDesc *d_table, int32_t nmesh, int32_t total, const float *d_rest, const CornerSkin *d_skin, int32_t nskin, const float *d_bones, TriAttr *attrs, int32_t ntri, hipStream_t stream) {
    if (nmesh > 0 && total > 0)
        hipLaunchKernelGGL(refit_skin_kernel, dim3((unsigned)((3 * (size_t)total + 255) / 256)), dim3(256), 0, stream, d_table, nmesh, total, d_rest, d_skin, nskin, d_bones, attrs, ntri);
}
void refit_morph(const MorphDesc *d_table, int32_t nmesh, int32_t total, const float *d_rest, const float *d_weights, int32_t nweights, const float *d_deltas, int64_t ndelta, float *d_base, TriAttr *attrs,
                 int32_t ntri, hipStream_t stream) {
    if (nmesh > 0 && total > 0)
        hipLaunchKernelGGL(refit_morph_kernel, dim3((unsigned)((3 * (size_t)total + 255) / 256)), dim3(256), 0, stream, d_table, nmesh, total, d_rest, d_weights, nweights, d_deltas, ndelta, d_base, attrs, ntri);
}
void refit_leaves(const RefitScene &r, hipStream_t stream) {
    if (r.nslots > 0) hipLaunchKernelGGL(refit_leaves_kernel, dim3((unsigned)((r.nslots + 255) / 256)), dim3(256), 0, stream, r.tri_index, r.nslots, r.attrs, r.ntri, r.leaves, r.tri_flat);
}
void refit_level(const RefitScene &r, const int32_t *d_order, int32_t count, float pad, hipStream_t stream) {
    if (count > 0) hipLaunchKernelGGL(refit_level_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, r.nodes, r.nnodes, d_order, count, r.tri_index, r.nslots,
                                      r.attrs, r.ntri, (Bx *)r.boxes, pad);
}
// the rotating level launch (d_level: the plan's level per node; d_taken, d_need: per-node scratch; d_root_out: two ints the root's thread writes)
void refit_rotate_level(const RefitScene &r, const int32_t *d_order, int32_t count, float pad, const int32_t *d_level, int32_t *d_taken, int32_t *d_need, int32_t *d_root_out, hipStream_t stream) {
    if (count > 0) hipLaunchKernelGGL(refit_rotate_level_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, r.nodes, r.nnodes, d_order, count, r.tri_index, r.nslots,
                                      r.attrs, r.ntri, (Bx *)r.boxes, pad, d_level, d_taken, d_need, d_root_out);
}

// evplp_accel_quality's launch: d_order = the refit plan's whole order (count reached nodes), d_out = 1 + 3 * ceil(count / 256) doubles
// (accel_cost_parts); enqueued, no wait
void accel_cost(const BvhNode *d_nodes, int32_t nnodes, const int32_t *d_order, int32_t count, double *d_out, hipStream_t stream) {
    if (count > 0) hipLaunchKernelGGL(accel_cost_kernel, dim3((unsigned)((count + kCostChunk - 1) / kCostChunk)), dim3(kCostChunk), 0, stream, d_nodes, nnodes, d_order, count, d_out);
}

// Builds on `stream` from the host triangle list; the four output arrays are device allocations owned by the caller
// (hipFree).  Returns hipSuccess or the failing HIP status.  ploc_radius > 0: the hierarchy by PLOC (1 .. kPlocMaxRadius, with
// ploc_search_iterations search iterations, 0 .. kPlocSearchIterations) instead of the radix tree; out->bound_passed with hipSuccess: the
// iterations passed ploc_iteration_bound and the build was stopped (nothing is handed over).
// PLOC's scratch on top of the radix tree's, allocated and freed in the call: 2 n clusters in ping-pong (a 4 B reference and a 24 B box
// each), n nearest neighbours (4 B), n packed flags and their scan (8 B each), and per inner node its children (8 B) and triangle count (4 B).
int build_bvh_gpu(const float *verts_host, int32_t ntri, float pad_scale, hipStream_t stream, BvhDeviceBuild *out, int32_t ploc_radius, int32_t ploc_search_iterations) {
    auto t0 = std::chrono::steady_clock::now();
    hipError_t err = hipSuccess;
    const int nt = std::max(ntri, 1);
    float *d_verts = nullptr; Bx *tbox = nullptr, *lbox = nullptr, *ibox = nullptr; uint8_t *valid = nullptr; uint32_t *bounds = nullptr;
    uint64_t *keys = nullptr, *keys2 = nullptr; int32_t *ids = nullptr, *ids2 = nullptr, *parent_int = nullptr, *parent_leaf = nullptr;
    Topo *topo = nullptr; uint32_t *visits = nullptr, *kept = nullptr, *new_id = nullptr, *head = nullptr, *flag = nullptr, *block_id = nullptr, *scal = nullptr;
    void *tmp = nullptr; size_t tmp_bytes = 0, need = 0;
    uint32_t h_bounds[13], h_counts[4];
    int n = 0, nnodes = 0, nblocks = 0;
    const unsigned gt = (unsigned)((nt + 255) / 256);
    BvhNode *nodes = nullptr; LeafBlock *leaves = nullptr; TriFlat *tri_flat = nullptr; int32_t *tri_index = nullptr;
    const bool ploc = ploc_radius > 0;
    Bx *cbox[2] = { nullptr, nullptr }; int32_t *cref[2] = { nullptr, nullptr }, *nn = nullptr, *ncnt = nullptr; PlocKids *kids = nullptr;
    unsigned long long *pflags = nullptr, *pscan = nullptr;
    const int32_t *leaf_ids = nullptr;                                    // triangle per position, in the order the emitted tree has
    out->iterations = 0; out->bound_passed = false;
    if (ploc && (ploc_radius > kPlocMaxRadius || ploc_search_iterations < 0 || ploc_search_iterations > kPlocSearchIterations)) { err = hipErrorInvalidValue; goto done; }

    GB_TRY(hipMalloc((void **)&d_verts, sizeof(float) * 9 * (size_t)nt));
    GB_TRY(hipMalloc((void **)&tbox, sizeof(Bx) * (size_t)nt)); GB_TRY(hipMalloc((void **)&lbox, sizeof(Bx) * (size_t)nt)); GB_TRY(hipMalloc((void **)&ibox, sizeof(Bx) * (size_t)nt));
    GB_TRY(hipMalloc((void **)&valid, (size_t)nt)); GB_TRY(hipMalloc((void **)&bounds, sizeof(uint32_t) * 16));
    GB_TRY(hipMalloc((void **)&keys, 8 * (size_t)nt)); GB_TRY(hipMalloc((void **)&keys2, 8 * (size_t)nt));
    GB_TRY(hipMalloc((void **)&ids, 4 * (size_t)nt)); GB_TRY(hipMalloc((void **)&ids2, 4 * (size_t)nt));
    GB_TRY(hipMalloc((void **)&parent_int, 4 * (size_t)nt)); GB_TRY(hipMalloc((void **)&parent_leaf, 4 * (size_t)nt));
    GB_TRY(hipMalloc((void **)&topo, sizeof(Topo) * (size_t)nt));
    GB_TRY(hipMalloc((void **)&visits, 4 * (size_t)nt)); GB_TRY(hipMalloc((void **)&kept, 4 * (size_t)nt)); GB_TRY(hipMalloc((void **)&new_id, 4 * (size_t)nt));
    GB_TRY(hipMalloc((void **)&head, 4 * (size_t)nt)); GB_TRY(hipMalloc((void **)&flag, 4 * (size_t)nt)); GB_TRY(hipMalloc((void **)&block_id, 4 * (size_t)nt));
    GB_TRY(hipMalloc((void **)&scal, 4 * 4));
    if (ploc) {
        for (int h = 0; h < 2; h++) { GB_TRY(hipMalloc((void **)&cbox[h], sizeof(Bx) * (size_t)nt)); GB_TRY(hipMalloc((void **)&cref[h], 4 * (size_t)nt)); }
        GB_TRY(hipMalloc((void **)&nn, 4 * (size_t)nt)); GB_TRY(hipMalloc((void **)&ncnt, 4 * (size_t)nt)); GB_TRY(hipMalloc((void **)&kids, sizeof(PlocKids) * (size_t)nt));
        GB_TRY(hipMalloc((void **)&pflags, 8 * (size_t)nt)); GB_TRY(hipMalloc((void **)&pscan, 8 * (size_t)nt));
    }
    if (ntri > 0) GB_TRY(hipMemcpyAsync(d_verts, verts_host, sizeof(float) * 9 * (size_t)ntri, hipMemcpyHostToDevice, stream));
    {
        const uint32_t init[13] = { 0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u, 0u };
        GB_TRY(hipMemcpyAsync(bounds, init, sizeof(init), hipMemcpyHostToDevice, stream));
    }
    hipLaunchKernelGGL(tri_setup_kernel, dim3(gt), dim3(256), 0, stream, d_verts, ntri, tbox, bounds, valid);
    hipLaunchKernelGGL(morton_kernel, dim3(gt), dim3(256), 0, stream, tbox, valid, ntri, bounds, keys, ids);
    if (ntri > 0) {
        GB_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, need, keys, keys2, ids, ids2, ntri, 0, 64, stream));
        tmp_bytes = need;
        GB_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, need, kept, new_id, nt, stream));
        tmp_bytes = std::max(tmp_bytes, need);
        if (ploc) { GB_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, need, pflags, pscan, nt, stream)); tmp_bytes = std::max(tmp_bytes, need); }
        GB_TRY(hipMalloc(&tmp, tmp_bytes));
        need = tmp_bytes;
        GB_TRY(hipcub::DeviceRadixSort::SortPairs(tmp, need, keys, keys2, ids, ids2, ntri, 0, 64, stream));
    }
    GB_TRY(hipMemcpyAsync(h_bounds, bounds, sizeof(h_bounds), hipMemcpyDeviceToHost, stream));
    GB_TRY(hipStreamSynchronize(stream));
    n = (int)h_bounds[12];                                                // valid triangles: the first n sorted positions
    GB_TRY(hipMemsetAsync(visits, 0, 4 * (size_t)nt, stream)); GB_TRY(hipMemsetAsync(head, 0, 4 * (size_t)nt, stream));
    GB_TRY(hipMemsetAsync(kept, 0, 4 * (size_t)nt, stream)); GB_TRY(hipMemsetAsync(scal, 0, 16, stream));
    if (n > 0) {
        const unsigned gn = (unsigned)((n + 255) / 256);
        leaf_ids = ids2;
        if (ploc) {
            hipLaunchKernelGGL(ploc_init_kernel, dim3(gn), dim3(256), 0, stream, tbox, ids2, n, cref[0], cbox[0]);
            const int32_t bound = ploc_iteration_bound(n, ploc_search_iterations);
            int c = n, cur = 0, it = 0;
            while (c > 1) {
                if (it >= bound) { out->bound_passed = true; out->iterations = it; goto done; }
                const unsigned gc = (unsigned)((c + 255) / 256);
                const int pairing = it >= ploc_search_iterations ? 1 : 0;
                if (!pairing) hipLaunchKernelGGL(ploc_nn_kernel, dim3(gc), dim3(256), 0, stream, cbox[cur], c, (int)ploc_radius, nn);
                hipLaunchKernelGGL(ploc_merge_kernel, dim3(gc), dim3(256), 0, stream, nn, pairing, c, pflags);
                need = tmp_bytes; GB_TRY(hipcub::DeviceScan::ExclusiveSum(tmp, need, pflags, pscan, c, stream));
                hipLaunchKernelGGL(ploc_scatter_kernel, dim3(gc), dim3(256), 0, stream, nn, pairing, c, n, pflags, pscan, cref[cur], cbox[cur], cref[cur ^ 1], cbox[cur ^ 1], kids, ibox,
                                   ncnt, new_id /* free until the scan below: node heights */, parent_int, parent_leaf, scal);
                GB_TRY(hipMemcpyAsync(&h_counts[0], &scal[1], 4, hipMemcpyDeviceToHost, stream));
                GB_TRY(hipStreamSynchronize(stream));                             // the one read-back of an iteration: c
                const int cn = (int)h_counts[0];
                if (cn < 1 || cn >= c) { out->bound_passed = true; out->iterations = it; goto done; }      // (an iteration that merged nothing: never, by the tie rule)
                c = cn; cur ^= 1; it++;
            }
            out->iterations = it;
            hipLaunchKernelGGL(ploc_place_kernel, dim3((unsigned)((2 * (size_t)n - 1 + 255) / 256)), dim3(256), 0, stream, n, kids, ncnt, parent_int, parent_leaf, ids2, tbox, ids, lbox, topo);
            leaf_ids = ids;                                                   // (free since the sort)
        } else {
            if (n > 1) hipLaunchKernelGGL(hierarchy_kernel, dim3(gn), dim3(256), 0, stream, keys2, n, topo, parent_int, parent_leaf);
            hipLaunchKernelGGL(refit_kernel, dim3(gn), dim3(256), 0, stream, tbox, ids2, n, topo, parent_int, parent_leaf, lbox, ibox, visits, new_id /* free until the scan below: node heights */, &scal[0]);
        }
        if (n > 1) hipLaunchKernelGGL(collapse_kernel, dim3(gn), dim3(256), 0, stream, topo, n, kept, head);
        else GB_TRY(hipMemsetAsync(head, 0, 4, stream));
        if (n == 1) { const uint32_t one = 1u; GB_TRY(hipMemcpyAsync(head, &one, 4, hipMemcpyHostToDevice, stream)); }
        hipLaunchKernelGGL(flag_kernel, dim3(gn), dim3(256), 0, stream, head, n, flag);
        need = tmp_bytes; GB_TRY(hipcub::DeviceScan::ExclusiveSum(tmp, need, kept, new_id, n, stream));
        need = tmp_bytes; GB_TRY(hipcub::DeviceScan::ExclusiveSum(tmp, need, flag, block_id, n, stream));
        // counts: kept nodes = new_id[n-2] + kept[n-2] (n >= 2), blocks = block_id[n-1] + flag[n-1]
        GB_TRY(hipMemcpyAsync(&h_counts[0], &block_id[n - 1], 4, hipMemcpyDeviceToHost, stream));
        GB_TRY(hipMemcpyAsync(&h_counts[1], &flag[n - 1], 4, hipMemcpyDeviceToHost, stream));
        if (n > 1) { GB_TRY(hipMemcpyAsync(&h_counts[2], &new_id[n - 2], 4, hipMemcpyDeviceToHost, stream)); GB_TRY(hipMemcpyAsync(&h_counts[3], &kept[n - 2], 4, hipMemcpyDeviceToHost, stream)); }
        else h_counts[2] = h_counts[3] = 0;
        GB_TRY(hipStreamSynchronize(stream));
        nblocks = (int)(h_counts[0] + h_counts[1]);
        nnodes = std::max((int)(h_counts[2] + h_counts[3]), 1);           // (<= 4 triangles: the wrapper root)
    } else nnodes = 1;

    GB_TRY(hipMalloc((void **)&nodes, sizeof(BvhNode) * (size_t)nnodes));
    GB_TRY(hipMalloc((void **)&leaves, sizeof(LeafBlock) * (size_t)std::max(nblocks, 1)));
    GB_TRY(hipMalloc((void **)&tri_flat, sizeof(TriFlat) * 4 * (size_t)std::max(nblocks, 1)));
    GB_TRY(hipMalloc((void **)&tri_index, sizeof(int32_t) * 4 * (size_t)std::max(nblocks, 1)));
    GB_TRY(hipMemsetAsync(leaves, 0, sizeof(LeafBlock) * (size_t)std::max(nblocks, 1), stream));
    GB_TRY(hipMemsetAsync(tri_flat, 0, sizeof(TriFlat) * 4 * (size_t)std::max(nblocks, 1), stream));
    GB_TRY(hipMemsetAsync(tri_index, 0xff, sizeof(int32_t) * 4 * (size_t)std::max(nblocks, 1), stream));
    if (n > 0) {
        const unsigned gn = (unsigned)((n + 255) / 256);
        hipLaunchKernelGGL(emit_nodes_kernel, dim3(gn), dim3(256), 0, stream, topo, n, kept, new_id, head, block_id, lbox, ibox, bounds, pad_scale, nodes);
        hipLaunchKernelGGL(emit_leaves_kernel, dim3(gn), dim3(256), 0, stream, d_verts, leaf_ids, n, head, block_id, leaves, tri_flat, tri_index);
    } else {
        BvhNode r; std::memset(&r, 0, sizeof(r));
        for (int k = 0; k < 3; k++) { r.hal[k][0] = r.hal[k][1] = -3.0e38f; }
        r.c0 = r.c1 = kNoChild;
        GB_TRY(hipMemcpyAsync(nodes, &r, sizeof(r), hipMemcpyHostToDevice, stream));
    }
    GB_TRY(hipMemcpyAsync(&h_counts[0], &scal[0], 4, hipMemcpyDeviceToHost, stream));
    GB_TRY(hipStreamSynchronize(stream));
    GB_TRY(hipGetLastError());
    out->nodes = nodes; out->leaves = leaves; out->tri_flat = tri_flat; out->tri_index = tri_index;
    out->nnodes = nnodes; out->nleaves = nblocks; out->ntris = n; out->depth = (int32_t)h_counts[0] + 2;
    nodes = nullptr; leaves = nullptr; tri_flat = nullptr; tri_index = nullptr;
done:
    hipFree(d_verts); hipFree(tbox); hipFree(lbox); hipFree(ibox); hipFree(valid); hipFree(bounds); hipFree(keys); hipFree(keys2); hipFree(ids); hipFree(ids2);
    hipFree(parent_int); hipFree(parent_leaf); hipFree(topo); hipFree(visits); hipFree(kept); hipFree(new_id); hipFree(head); hipFree(flag); hipFree(block_id); hipFree(scal);
    for (int h = 0; h < 2; h++) { hipFree(cbox[h]); hipFree(cref[h]); }
    hipFree(nn); hipFree(ncnt); hipFree(kids); hipFree(pflags); hipFree(pscan);
    hipFree(tmp); hipFree(nodes); hipFree(leaves); hipFree(tri_flat); hipFree(tri_index);
    out->build_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return (int)err;
}

} // namespace evplp

// The host twin of the refit's tree rotations (include/evplp.h evplp_rotate_tree): host only, no device, like the level plan, the tree cost
// and the PLOC twin beside it.  It runs refit_rotate_level_kernel's sweep (bvh_gpu.hip) serially in the plan's order -- exact boxes from the
// leaves upward and, at every node, the one rule both sides call (evplp_types.h rotate_choice, rotate_union, rotate_need) -- so the two take
// the same rotations.  It deals in topology and unpadded boxes; the padded bytes of a node are the device's business.
#include "../evplp_types.h"

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

using namespace evplp;

namespace {
struct Tree {
    std::vector<int32_t> kids;          // [2 * nnodes]
    std::vector<float> boxes;           // [6 * nnodes]
    const int32_t *tri_index; int32_t nslots; const float *verts9; int32_t ntri; int32_t nnodes;
    // the exact box under a child reference, as the refit's kernels form it
    void ref_box(int32_t ref, float *out) const {
        for (int k = 0; k < 3; k++) { out[k] = 3.0e38f; out[3 + k] = -3.0e38f; }
        if (ref >= 0) { if (ref < nnodes) std::memcpy(out, &boxes[6 * (size_t)ref], 24); return; }
        if (ref == kNoChild) return;
        const int32_t id = ~ref, cnt = (id & 3) + 1;
        for (int32_t q = 0; q < cnt; q++) {
            const int32_t slot = (id & ~3) + q;
            const int32_t tri = slot < nslots ? tri_index[slot] : -1;
            if (tri < 0 || tri >= ntri) continue;
            const float *v = verts9 + 9 * (size_t)tri;
            if (!tri_has_area(v)) continue;
            for (int k = 0; k < 3; k++) { out[k] = fminf(out[k], fminf(fminf(v[k], v[3 + k]), v[6 + k])); out[3 + k] = fmaxf(out[3 + k], fmaxf(fmaxf(v[k], v[3 + k]), v[6 + k])); }
        }
    }
    void kids_of(int32_t i, int32_t out[2]) const {
        out[0] = out[1] = kNoChild;
        if (i >= 0 && i < nnodes) { out[0] = kids[2 * (size_t)i]; out[1] = kids[2 * (size_t)i + 1]; }
    }
};
void slots_of(int32_t ref, const int32_t kids[2], int32_t *g) {        // what node4 puts in the two slots of one child
    if (ref >= 0) { g[0] = kids[0]; g[1] = kids[1]; } else { g[0] = ref; g[1] = kNoChild; }
}
}

extern "C" int evplp_rotate_tree(const void *nodes64, int32_t nnodes, const int32_t *tri_index, int32_t nslots, const float *verts9, int32_t ntri, const int32_t *level,
                                 int32_t passes, int32_t *children, float *boxes, int32_t *rotations, int32_t *need0) {
    if (!nodes64 || !children || !boxes || !rotations || !need0 || nnodes < 1 || nslots < 0 || ntri < 0 || (nslots > 0 && !tri_index) || (ntri > 0 && !verts9)) return EVPLP_ERR_INVALID;
    if (passes < 1 || passes > 8) return EVPLP_ERR_INVALID;
    // the plan: the tight heights of the tree as it is, or the caller's levels (a tree that was rotated before keeps the plan it had)
    std::vector<int32_t> height((size_t)nnodes), order((size_t)nnodes), begin((size_t)nnodes + 1);
    const int levels = evplp_refit_levels(nodes64, nnodes, height.data(), order.data(), begin.data(), nnodes);
    if (levels < 1) return EVPLP_ERR_INVALID;
    const int32_t reached = begin[(size_t)levels];
    Tree t;
    t.kids.resize(2 * (size_t)nnodes); t.boxes.assign(6 * (size_t)nnodes, 0.f);
    t.tri_index = tri_index; t.nslots = nslots; t.verts9 = verts9; t.ntri = ntri; t.nnodes = nnodes;
    for (int32_t i = 0; i < nnodes; i++) {
        std::memcpy(&t.kids[2 * (size_t)i], (const unsigned char *)nodes64 + sizeof(BvhNode) * (size_t)i + offsetof(BvhNode, c0), 8);
        for (int k = 0; k < 3; k++) { t.boxes[6 * (size_t)i + k] = 3.0e38f; t.boxes[6 * (size_t)i + 3 + k] = -3.0e38f; }
    }
    std::vector<int32_t> lvl(height);
    int32_t nlevels = levels;
    if (level) {
        nlevels = 0;
        for (int32_t e = 0; e < reached; e++) {
            const int32_t i = order[(size_t)e];
            if (level[i] < 0) return EVPLP_ERR_INVALID;
            for (int s = 0; s < 2; s++) { const int32_t c = t.kids[2 * (size_t)i + s]; if (c >= 0 && !(level[c] < level[i])) return EVPLP_ERR_INVALID; }
            lvl[(size_t)i] = level[i]; nlevels = std::max(nlevels, level[i] + 1);
        }
        std::stable_sort(order.begin(), order.begin() + reached, [&](int32_t a, int32_t b) { return lvl[(size_t)a] != lvl[(size_t)b] ? lvl[(size_t)a] < lvl[(size_t)b] : a < b; });
    }
    std::vector<int32_t> taken((size_t)nnodes, 0), need((size_t)nnodes, 0);
    for (int32_t p = 0; p < passes; p++) {
        for (int32_t e = 0; e < reached; e++) {                             // level by level, by index within a level: the launches' order
            const int32_t i = order[(size_t)e];
            int32_t ref[2] = { t.kids[2 * (size_t)i], t.kids[2 * (size_t)i + 1] }, l2[2], gref[2][2];
            float box[2][6], gbox[2][2][6];
            for (int s = 0; s < 2; s++) {
                t.ref_box(ref[s], box[s]);
                l2[s] = ref[s] >= 0 && ref[s] < nnodes ? lvl[(size_t)ref[s]] : -1;
                t.kids_of(ref[s], gref[s]);
                for (int q = 0; q < 2; q++) t.ref_box(gref[s][q], gbox[s][q]);
            }
            const int pick = rotate_choice(ref, l2, box, gref, gbox);
            int32_t own = 0, sub[2], g4[4];
            for (int s = 0; s < 2; s++) { sub[s] = ref[s] >= 0 && ref[s] < nnodes ? taken[(size_t)ref[s]] : 0; slots_of(ref[s], gref[s], g4 + 2 * s); }
            if (pick >= 0) {
                const int s = pick >> 1, q = pick & 1;
                const int32_t a = ref[s], b = ref[1 - s], g = gref[1 - s][q], k = gref[1 - s][1 - q];
                t.kids[2 * (size_t)b + q] = a;
                float ub[6];
                if (q == 0) rotate_union(box[s], gbox[1 - s][1], ub); else rotate_union(gbox[1 - s][0], box[s], ub);
                std::memcpy(&t.boxes[6 * (size_t)b], ub, 24);
                int32_t kk[2], kg[2], gb[4];
                t.kids_of(k, kk); t.kids_of(g, kg);
                slots_of(a, gref[s], gb); slots_of(k, kk, gb + 2);
                need[(size_t)b] = rotate_need(gb, need.data(), nnodes);
                const int32_t taken_g = g >= 0 && g < nnodes ? taken[(size_t)g] : 0, taken_b = sub[1 - s] - taken_g + sub[s];
                taken[(size_t)b] = taken_b;
                slots_of(g, kg, g4 + 2 * s);
                g4[2 * (1 - s)] = q == 0 ? a : k; g4[2 * (1 - s) + 1] = q == 0 ? k : a;
                sub[s] = taken_g; sub[1 - s] = taken_b;
                ref[s] = g;
                std::memcpy(box[s], gbox[1 - s][q], 24); std::memcpy(box[1 - s], ub, 24);
                own = 1;
            }
            t.kids[2 * (size_t)i] = ref[0]; t.kids[2 * (size_t)i + 1] = ref[1];
            rotate_union(box[0], box[1], &t.boxes[6 * (size_t)i]);
            taken[(size_t)i] = own + sub[0] + sub[1];
            need[(size_t)i] = rotate_need(g4, need.data(), nnodes);
        }
        rotations[p] = taken[0];
    }
    std::memcpy(children, t.kids.data(), sizeof(int32_t) * 2 * (size_t)nnodes);
    std::memcpy(boxes, t.boxes.data(), sizeof(float) * 6 * (size_t)nnodes);
    *need0 = need[0];
    return nlevels;
}

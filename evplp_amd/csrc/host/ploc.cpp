// The host twin of the device PLOC builder (include/evplp.h evplp_ploc_tree): host only, no device, like the level plan and the tree cost
// beside it.  It runs the steps of bvh_gpu.hip's PLOC path serially -- the Morton key of the host LBVH (bvh_build.cpp, the device's
// quantisation), a stable sort, then per iteration nearest neighbour, merge of the mutual pairs, compaction -- with the distance function the
// kernel calls (evplp_types.h ploc_distance) and the same tie rule, so the two produce one tree.
#include "../evplp_types.h"

#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

using namespace evplp;

namespace {
struct Box6 { float v[6]; };      // lo[3], hi[3]
uint64_t expand21(uint64_t v) {
    v &= 0x1fffffull;
    v = (v | v << 32) & 0x1f00000000ffffull;
    v = (v | v << 16) & 0x1f0000ff0000ffull;
    v = (v | v << 8) & 0x100f00f00f00f00full;
    v = (v | v << 4) & 0x10c30c30c30c30c3ull;
    v = (v | v << 2) & 0x1249249249249249ull;
    return v;
}
}

extern "C" int evplp_ploc_tree(const float *verts9, int32_t ntri, int32_t radius, int32_t search_iterations, int32_t *order, int32_t *children, int32_t *iterations) {
    if (!order || !children || !iterations || ntri < 0 || (ntri > 0 && !verts9)) return EVPLP_ERR_INVALID;
    if (radius < 1 || radius > kPlocMaxRadius || search_iterations < 0 || search_iterations > kPlocSearchIterations) return EVPLP_ERR_INVALID;
    *iterations = 0;
    // 1. boxes, validity (meshBound's rule), the bounds of the valid triangles' box centres
    std::vector<Box6> tbox((size_t)ntri);
    std::vector<int32_t> ids;
    float clo[3] = { 3.0e38f, 3.0e38f, 3.0e38f }, chi[3] = { -3.0e38f, -3.0e38f, -3.0e38f };
    for (int32_t i = 0; i < ntri; i++) {
        const float *v = verts9 + 9 * (size_t)i;
        Box6 &t = tbox[(size_t)i];
        for (int k = 0; k < 3; k++) { t.v[k] = fminf(fminf(v[k], v[3 + k]), v[6 + k]); t.v[3 + k] = fmaxf(fmaxf(v[k], v[3 + k]), v[6 + k]); }
        if (!tri_has_area(v)) continue;
        ids.push_back(i);
        for (int k = 0; k < 3; k++) { const float ce = 0.5f * (t.v[k] + t.v[3 + k]); clo[k] = fminf(clo[k], ce); chi[k] = fmaxf(chi[k], ce); }
    }
    const int32_t n = (int32_t)ids.size();
    // 2. Morton keys; equal keys keep triangle order
    std::vector<std::pair<uint64_t, int32_t>> keyed((size_t)n);
    for (int32_t p = 0; p < n; p++) {
        const Box6 &t = tbox[(size_t)ids[(size_t)p]];
        uint64_t q[3];
        for (int k = 0; k < 3; k++) {
            const float ext = std::max(chi[k] - clo[k], 1e-30f), c = 0.5f * (t.v[k] + t.v[3 + k]);
            double x = ((double)c - (double)clo[k]) / (double)ext;
            x = std::min(std::max(x, 0.0), 1.0);
            q[k] = (uint64_t)std::min(x * 2097152.0, 2097151.0);
        }
        keyed[(size_t)p] = { (expand21(q[0]) << 2) | (expand21(q[1]) << 1) | expand21(q[2]), ids[(size_t)p] };
    }
    std::sort(keyed.begin(), keyed.end());
    // the initial clusters: position p holds leaf ~p and its triangle's box
    std::vector<int32_t> ref((size_t)n), ref2((size_t)n), nn((size_t)n);
    std::vector<Box6> box((size_t)n), box2((size_t)n);
    for (int32_t p = 0; p < n; p++) { order[p] = keyed[(size_t)p].second; ref[(size_t)p] = ~p; box[(size_t)p] = tbox[(size_t)order[p]]; }
    int32_t c = n, it = 0;
    const int32_t bound = ploc_iteration_bound(n, search_iterations);
    while (c > 1) {
        if (it >= bound) return EVPLP_ERR_INVALID;                          // (cannot happen: every iteration merges, the pairing halves)
        if (it < search_iterations) {
            for (int32_t i = 0; i < c; i++) {
                float best = 0.f; int32_t bj = -1;
                for (int32_t j = std::max(0, i - radius); j <= std::min(c - 1, i + radius); j++) {
                    if (j == i) continue;
                    const float d = ploc_distance(box[(size_t)i].v, box[(size_t)j].v);
                    if (bj < 0 || d < best) { best = d; bj = j; }                // ties keep the lowest j
                }
                nn[(size_t)i] = bj;
            }
        } else for (int32_t i = 0; i < c; i++) nn[(size_t)i] = (i ^ 1) < c ? (i ^ 1) : i;
        int32_t m = 0;
        for (int32_t i = 0; i < c; i++) { const int32_t j = nn[(size_t)i]; if (j > i && nn[(size_t)j] == i) m++; }
        int32_t rank = 0, out = 0;
        for (int32_t i = 0; i < c; i++) {
            const int32_t j = nn[(size_t)i];
            const bool merged = j != i && nn[(size_t)j] == i;
            if (merged && j < i) continue;                                   // the partner's position is vacated
            if (merged) {
                const int32_t idx = c - 1 - m + rank++;
                children[2 * (size_t)idx] = ref[(size_t)i]; children[2 * (size_t)idx + 1] = ref[(size_t)j];
                Box6 u;
                for (int k = 0; k < 3; k++) { u.v[k] = fminf(box[(size_t)i].v[k], box[(size_t)j].v[k]); u.v[3 + k] = fmaxf(box[(size_t)i].v[3 + k], box[(size_t)j].v[3 + k]); }
                ref2[(size_t)out] = idx; box2[(size_t)out] = u;
            } else { ref2[(size_t)out] = ref[(size_t)i]; box2[(size_t)out] = box[(size_t)i]; }
            out++;
        }
        ref.swap(ref2); box.swap(box2);
        c = out; it++;
    }
    *iterations = it;
    return n;
}

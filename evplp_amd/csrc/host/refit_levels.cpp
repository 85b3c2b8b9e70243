// The level plan of evplp_refit_accel (include/evplp.h): host only, no device, nothing but the standard library, like the deal of row
// blocks beside it (deal.cpp).  A refit recomputes the boxes of a tree bottom-up, one kernel launch per height; this is the order.
#include "../../../include/evplp.h"

#include <cstdint>
#include <cstring>
#include <vector>

namespace {
constexpr size_t kNodeBytes = 64, kChild0 = 48, kChild1 = 52;     // evplp_types.h BvhNode: c0 and c1 behind the twelve box floats
inline int32_t child_of(const unsigned char *nodes, int32_t i, int which) {
    int32_t c; std::memcpy(&c, nodes + kNodeBytes * (size_t)i + (which ? kChild1 : kChild0), 4); return c;
}
}

// height[i] = 0 for a node with no inner child, else 1 + the larger height of its inner children; order = the nodes reached from node 0
// sorted by height, by node index within a height; level_begin[l] .. level_begin[l + 1] = the nodes of height l in `order`.  The walk
// from the root marks what it reaches, so a second arrival at a node (two parents, a self-loop, a longer cycle) is seen at once and
// nothing is followed twice: at most nnodes pushes.  No storage order is assumed (the device builder's nodes are not in pre-order).
extern "C" int evplp_refit_levels(const void *nodes64, int32_t nnodes, int32_t *height, int32_t *order, int32_t *level_begin, int32_t level_capacity) {
    if (!nodes64 || !height || !order || !level_begin || nnodes < 1 || level_capacity < 1) return EVPLP_ERR_INVALID;
    const unsigned char *nodes = (const unsigned char *)nodes64;
    std::vector<int32_t> pre; pre.reserve((size_t)nnodes);          // the reached nodes, parents in front of their children
    std::vector<int32_t> stack; stack.reserve(64);
    std::vector<char> seen((size_t)nnodes, 0);
    stack.push_back(0); seen[0] = 1;
    while (!stack.empty()) {
        const int32_t i = stack.back(); stack.pop_back();
        pre.push_back(i);
        for (int s = 0; s < 2; s++) {
            const int32_t c = child_of(nodes, i, s);
            if (c < 0) continue;                                     // a leaf reference or an absent child
            if (c >= nnodes || seen[(size_t)c]) return EVPLP_ERR_INVALID;
            seen[(size_t)c] = 1; stack.push_back(c);
        }
    }
    for (int32_t i = 0; i < nnodes; i++) height[i] = -1;
    int32_t top = 0;
    for (size_t k = pre.size(); k-- > 0;) {                          // children are behind their parent in `pre`: backwards they come first
        const int32_t i = pre[k];
        int32_t h = 0;
        for (int s = 0; s < 2; s++) { const int32_t c = child_of(nodes, i, s); if (c >= 0 && height[c] + 1 > h) h = height[c] + 1; }
        height[i] = h; if (h > top) top = h;
    }
    const int32_t levels = top + 1;
    if (levels > level_capacity) return EVPLP_ERR_INVALID;
    for (int32_t l = 0; l <= levels; l++) level_begin[l] = 0;
    for (int32_t i = 0; i < nnodes; i++) if (height[i] >= 0) level_begin[height[i] + 1]++;
    for (int32_t l = 0; l < levels; l++) level_begin[l + 1] += level_begin[l];
    std::vector<int32_t> cursor(level_begin, level_begin + levels);
    for (int32_t i = 0; i < nnodes; i++) if (height[i] >= 0) order[cursor[(size_t)height[i]]++] = i;
    return levels;
}

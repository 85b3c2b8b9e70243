// The SAH cost of a flattened tree (include/evplp.h evplp_accel_cost): host only, no device, like the level plan beside it
// (refit_levels.cpp), whose order it takes.  It is the reference of accel_cost_kernel (bvh_gpu.hip): the terms come from the functions the
// kernel calls (evplp_types.h) and are added in the kernel's shape, so the two agree bit for bit on the same node bytes.
#include "../evplp_types.h"

#include <cstring>
#include <vector>

using namespace evplp;

extern "C" int evplp_accel_cost(const void *nodes64, int32_t nnodes, double out[5]) {
    if (!nodes64 || !out || nnodes < 1) return EVPLP_ERR_INVALID;
    // (a tree of nnodes nodes has at most nnodes heights: the plan refuses what is not a tree, never a deep one)
    std::vector<int32_t> height((size_t)nnodes), order((size_t)nnodes), begin((size_t)nnodes + 1);
    const int levels = evplp_refit_levels(nodes64, nnodes, height.data(), order.data(), begin.data(), nnodes);
    if (levels < 1) return EVPLP_ERR_INVALID;
    const int32_t reached = begin[(size_t)levels], nchunks = (reached + kCostChunk - 1) / kCostChunk;
    const unsigned char *bytes = (const unsigned char *)nodes64;
    std::vector<double> parts(3 * (size_t)nchunks);
    double root_area = 0.0;
    for (int32_t k = 0; k < nchunks; k++) {
        double v[kCostChunk][3];                                             // thread i of workgroup k
        for (int i = 0; i < kCostChunk; i++) {
            v[i][0] = v[i][1] = v[i][2] = 0.0;
            const int32_t e = kCostChunk * k + i;
            if (e >= reached) continue;
            BvhNode f; std::memcpy(&f, bytes + sizeof(BvhNode) * (size_t)order[(size_t)e], sizeof(f));
            accel_cost_terms(f, v[i]);
            if (order[(size_t)e] == 0) root_area = accel_root_area(f);
        }
        for (int j = 0; j < 3; j++) {
            for (int w = 0; w < kCostChunk; w += 64)                         // a wavefront: shuffle-down by 32 .. 1 (what lane 0 ends with)
                for (int off = 32; off > 0; off >>= 1)
                    for (int l = 0; l < off; l++) v[w + l][j] += v[w + l + off][j];
            double t = v[0][j];
            for (int w = 64; w < kCostChunk; w += 64) t += v[w][j];          // thread 0 adds the waves in order
            parts[3 * (size_t)k + j] = t;
        }
    }
    accel_cost_finish(parts.data(), nchunks, root_area, out);
    return reached;
}

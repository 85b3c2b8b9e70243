// Linear-blend skinning on the host (include/evplp.h evplp_skin_points): host only, no device, like the level plan, the block deal and the
// rotation twin beside it.  The validation of a skin and of a palette lives here for the context's and the group's entry points as well
// (skin.hpp); every point moves through skin_point (evplp_types.h), the function refit_skin_kernel calls on the device.
#include "skin.hpp"
#include "../evplp_types.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

namespace evplp {
bool skin_arrays_ok(int32_t nbones, const int32_t *bone_index, const float *weight, int32_t nverts, char *why, size_t cap) {
    if (nbones < 1 || nbones > kMaxSkinBones) { std::snprintf(why, cap, "nbones must be 1 .. %d, not %d", kMaxSkinBones, nbones); return false; }
    if (nverts < 0) { std::snprintf(why, cap, "a negative vertex count (%d)", nverts); return false; }
    if (nverts > 0 && (!bone_index || !weight)) { std::snprintf(why, cap, "null %s", !bone_index ? "bone_index" : "weight"); return false; }
    for (size_t v = 0; v < (size_t)nverts; v++) {
        double sum = 0.0;
        for (int k = 0; k < 4; k++) {
            const int32_t b = bone_index[4 * v + k]; const float w = weight[4 * v + k];
            if (b < 0 || b >= nbones) { std::snprintf(why, cap, "bone index %d of vertex %zu (influence %d) is outside [0, %d)", b, v, k, nbones); return false; }
            if (!std::isfinite(w) || w < 0.0f) { std::snprintf(why, cap, "weight %d of vertex %zu is not finite or is negative", k, v); return false; }
            sum += (double)w;
        }
        if (!(std::fabs(sum - 1.0) <= 1e-3)) { std::snprintf(why, cap, "the weights of vertex %zu add up to %.9g, not to 1 within 1e-3", v, sum); return false; }
    }
    return true;
}

bool skin_palette_ok(const float *bone_matrices, int32_t nbones, char *why, size_t cap) {
    if (!bone_matrices) { std::snprintf(why, cap, "null bone_matrices"); return false; }
    for (size_t i = 0; i < 12 * (size_t)(nbones > 0 ? nbones : 0); i++)
        if (!std::isfinite(bone_matrices[i])) { std::snprintf(why, cap, "entry %zu of bone matrix %zu is not finite", i % 12, i / 12); return false; }
    return true;
}

int64_t skin_apply(const float *bone_matrices, const int32_t *bone_index, const float *weight, const float *in, float *out, size_t n) {
    int64_t bad = -1;
    for (size_t v = 0; v < n; v++) {
        float o[3];
        skin_point(bone_matrices, bone_index + 4 * v, weight + 4 * v, in + 3 * v, o);
        if (bad < 0 && (!std::isfinite(o[0]) || !std::isfinite(o[1]) || !std::isfinite(o[2]))) bad = (int64_t)v;
        std::memcpy(out + 3 * v, o, 12);
    }
    return bad;
}
}

extern "C" int evplp_skin_points(const float *bone_matrices, int32_t nbones, const int32_t *bone_index, const float *weight, const float *in, float *out, int32_t n) {
    char why[256];
    if (n < 0 || (n > 0 && (!in || !out))) return EVPLP_ERR_INVALID;
    if (!evplp::skin_arrays_ok(nbones, bone_index, weight, n, why, sizeof(why)) || !evplp::skin_palette_ok(bone_matrices, nbones, why, sizeof(why))) return EVPLP_ERR_INVALID;
    // (a refusal writes nothing: the points go to a scratch array first)
    std::vector<float> tmp(3 * (size_t)n);
    if (evplp::skin_apply(bone_matrices, bone_index, weight, in, tmp.data(), (size_t)n) >= 0) return EVPLP_ERR_INVALID;
    if (n > 0) std::memcpy(out, tmp.data(), sizeof(float) * tmp.size());
    return EVPLP_OK;
}

// Morph targets on the host (include/evplp.h evplp_morph_points): host only, no device, like the skinning beside it.  The validation of a set of
// targets and of a set of weights lives here for the context's and the group's entry points as well (morph.hpp), and so does the composition
// with the matrix or the pose in force for the host copy of a mesh; every point is morphed through morph_point (evplp_types.h), the function
// refit_morph_kernel calls on the device.
#include "morph.hpp"
#include "skin.hpp"
#include "../evplp_types.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

namespace evplp {
bool morph_deltas_ok(int32_t ntargets, const float *deltas, int32_t nverts, char *why, size_t cap) {
    if (ntargets < 1 || ntargets > kMaxMorphTargets) { std::snprintf(why, cap, "ntargets must be 1 .. %d, not %d", kMaxMorphTargets, ntargets); return false; }
    if (nverts < 0) { std::snprintf(why, cap, "a negative vertex count (%d)", nverts); return false; }
    if (nverts > 0 && !deltas) { std::snprintf(why, cap, "null deltas"); return false; }
    const size_t per = 3 * (size_t)nverts;
    for (size_t i = 0; i < per * (size_t)ntargets; i++)
        if (!std::isfinite(deltas[i])) { std::snprintf(why, cap, "the delta of vertex %zu in target %zu is not finite", (i % per) / 3, i / per); return false; }
    return true;
}

bool morph_weights_ok(const float *weights, int32_t ntargets, char *why, size_t cap) {
    if (!weights) { std::snprintf(why, cap, "null weights"); return false; }
    for (int32_t k = 0; k < ntargets; k++)
        if (!std::isfinite(weights[k])) { std::snprintf(why, cap, "weight %d is not finite", k); return false; }
    return true;
}

int64_t morph_apply(const float *deltas, const float *weights, int32_t ntargets, const float *in, float *out, size_t n) {
    int64_t bad = -1;
    for (size_t v = 0; v < n; v++) {
        float o[3];
        morph_point(in + 3 * v, deltas + 3 * v, 3 * n, weights, ntargets, o);
        if (bad < 0 && (!std::isfinite(o[0]) || !std::isfinite(o[1]) || !std::isfinite(o[2]))) bad = (int64_t)v;
        std::memcpy(out + 3 * v, o, 12);
    }
    return bad;
}

int64_t morph_deform(const float *base, const float *matrix, const float *palette, const int32_t *bone_index, const float *bone_weight, float *out, size_t n) {
    if (palette) return skin_apply(palette, bone_index, bone_weight, base, out, n);
    int64_t bad = -1;
    for (size_t v = 0; v < n; v++) {
        float o[3];
        if (matrix) transform_point(matrix, base + 3 * v, o); else std::memcpy(o, base + 3 * v, 12);
        if (bad < 0 && (!std::isfinite(o[0]) || !std::isfinite(o[1]) || !std::isfinite(o[2]))) bad = (int64_t)v;
        std::memcpy(out + 3 * v, o, 12);
    }
    return bad;
}
}

extern "C" int evplp_morph_points(const float *in, const float *deltas, const float *weights, int32_t ntargets, int32_t n, float *out) {
    char why[256];
    if (n < 0 || (n > 0 && (!in || !out))) return EVPLP_ERR_INVALID;
    if (!evplp::morph_deltas_ok(ntargets, deltas, n, why, sizeof(why)) || !evplp::morph_weights_ok(weights, ntargets, why, sizeof(why))) return EVPLP_ERR_INVALID;
    for (size_t i = 0; i < 3 * (size_t)n; i++) if (!std::isfinite(in[i])) return EVPLP_ERR_INVALID;
    // (a refusal writes nothing: the points go to a scratch array first)
    std::vector<float> tmp(3 * (size_t)n);
    if (evplp::morph_apply(deltas, weights, ntargets, in, tmp.data(), (size_t)n) >= 0) return EVPLP_ERR_INVALID;
    if (n > 0) std::memcpy(out, tmp.data(), sizeof(float) * tmp.size());
    return EVPLP_OK;
}

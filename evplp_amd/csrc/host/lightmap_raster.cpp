// Lightmap baking, host only (include/evplp.h "lightmap baking"): whether one sample of one atlas texel is covered by one triangle, and its
// barycentrics, exported from the header the kernels of kernels_lightmap.hip include (lightmap_raster.h).  No GPU, no context: the tests hold
// the rasteriser's rules against an int64 restatement with this.
#include "../../../include/evplp.h"
#include "../lightmap_raster.h"

extern "C" int evplp_lightmap_cover(const float uv6[6], int32_t width, int32_t height, int32_t samples, int32_t x, int32_t y, int32_t i, int32_t j, float *beta, float *gamma) {
    if (!uv6 || width < 1 || width > LM_MAX_SIZE || height < 1 || height > LM_MAX_SIZE || (samples != 1 && samples != 2 && samples != 4)) return 0;
    if (x < 0 || x >= width || y < 0 || y >= height || i < 0 || i >= samples || j < 0 || j >= samples) return 0;
    lm_tri t;
    lm_setup(uv6, width, height, &t);
    float b = 0.0f, g = 0.0f;
    const int in = lm_cover(&t, lm_sample(x, i, samples), lm_sample(y, j, samples), &b, &g);
    if (in) { if (beta) *beta = b; if (gamma) *gamma = g; }
    return in;
}

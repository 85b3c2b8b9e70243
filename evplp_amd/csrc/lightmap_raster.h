/*
 * lightmap_raster.h -- the integer arithmetic of the atlas rasteriser (evplp_lightmap_samples, evplp_bake_lightmap), written once for the
 * host (host/lightmap_raster.cpp exports it as evplp_lightmap_cover) and for the kernels of kernels_lightmap.hip, as photon_grid.h is for
 * the surface gather.  After the snap everything is int32 / int64, so coverage is exact: watertight, and the same on both sides bit for bit.
 *
 * The snap.  X = rint(fl(fl(u * (float)width) * 256.0f)), Y likewise with the height: round to nearest even, 8 sub-texel bits.  A triangle
 * with a snapped magnitude above 2^22 (a NaN or an infinity among them) is skipped.  Sample (i, j) of texel (x, y) at S samples per axis
 * lies at px = 256 x + (2 i + 1) 128 / S, py likewise: never on a texel's border, and for S = 1, 2, 4 an integer.
 * Orientation.  A2 = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0); 0: skipped; < 0: a mirrored chart, rasterised as (v0, v2, v1) with beta and
 * gamma swapped back.  The edge a -> b has E(p) = (bx - ax)(py - ay) - (by - ay)(px - ax); with |X| <= 2^22 and px < 2^21 + 2^8 every
 * difference is below 2^24 and every product below 2^47: int64 holds them all.  A sample is inside iff for the three edges v0 -> v1,
 * v1 -> v2, v2 -> v0 of the oriented triangle E > 0, or E == 0 and the edge owns its line: d = b - a, d.y > 0 || (d.y == 0 && d.x < 0).
 * Of the two directions of an edge that two triangles share exactly one owns, so a sample on it belongs to exactly one of them.
 * The kernels fold the rule into the constant: E - (own ? 0 : 1) >= 0 is the same test on integers.
 * Barycentrics.  beta = (float)((double)E_ca / (double)A2), gamma = (float)((double)E_ab / (double)A2) of the oriented triangle: both
 * integers are exact doubles, the division and the conversion round to nearest.
 */
#ifndef EVPLP_LIGHTMAP_RASTER_H
#define EVPLP_LIGHTMAP_RASTER_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LM_FN __host__ __device__ static inline
#else
#define LM_FN static inline
#endif
#if defined(__clang__)
#define LM_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define LM_NO_CONTRACT
#endif

#define LM_SUB_BITS 8
#define LM_SUB 256
#define LM_MAX_SNAP 4194304.0f       /* 2^22 */
#define LM_MAX_SIZE 8192
#define LM_TRI_VALID 1u
#define LM_TRI_MIRRORED 2u

/* a triangle after the snap and the orientation: v[0..5] = X0 Y0 X1 Y1 X2 Y2 with A2 > 0 (flags has LM_TRI_MIRRORED where v1 and v2 were
 * swapped for that); flags without LM_TRI_VALID: skipped, the rest is zeros */
typedef struct lm_tri { int32_t v[6]; uint32_t flags; int32_t pad; } lm_tri;

/* one snapped coordinate; false: not representable */
LM_FN int lm_snap1(float u, int32_t size, int32_t *out) {
    LM_NO_CONTRACT
    const float a = u * (float)size;
    const float b = a * 256.0f;
    const float r = rintf(b);
    if (!(fabsf(r) <= LM_MAX_SNAP)) return 0;
    *out = (int32_t)r;
    return 1;
}
LM_FN int64_t lm_edge(int32_t ax, int32_t ay, int32_t bx, int32_t by, int32_t px, int32_t py) {
    return (int64_t)(bx - ax) * (int64_t)(py - ay) - (int64_t)(by - ay) * (int64_t)(px - ax);
}
LM_FN int lm_owns(int32_t dx, int32_t dy) { return dy > 0 || (dy == 0 && dx < 0); }
LM_FN int32_t lm_sample(int32_t texel, int32_t k, int32_t samples) { return LM_SUB * texel + (2 * k + 1) * (128 / samples); }

/* uv6: TriAttr::uv's layout (u0 v0 u1 v1 u2 v2) */
LM_FN void lm_setup(const float uv6[6], int32_t width, int32_t height, lm_tri *t) {
    int32_t v[6];
    int ok = 1;
    for (int k = 0; k < 3; k++) { ok &= lm_snap1(uv6[2 * k], width, &v[2 * k]); ok &= lm_snap1(uv6[2 * k + 1], height, &v[2 * k + 1]); }
    for (int k = 0; k < 6; k++) t->v[k] = 0;
    t->flags = 0u; t->pad = 0;
    if (!ok) return;
    const int64_t a2 = lm_edge(v[0], v[1], v[2], v[3], v[4], v[5]);
    if (a2 == 0) return;
    t->flags = LM_TRI_VALID;
    if (a2 < 0) { int32_t s = v[2]; v[2] = v[4]; v[4] = s; s = v[3]; v[3] = v[5]; v[5] = s; t->flags |= LM_TRI_MIRRORED; }
    for (int k = 0; k < 6; k++) t->v[k] = v[k];
}
/* the sample at (px, py) against an oriented triangle: 1 and its barycentrics (of the triangle as given: the mirror is undone), or 0 */
LM_FN int lm_cover(const lm_tri *t, int32_t px, int32_t py, float *beta, float *gamma) {
    if (!(t->flags & LM_TRI_VALID)) return 0;
    const int32_t *v = t->v;
    const int64_t eab = lm_edge(v[0], v[1], v[2], v[3], px, py), ebc = lm_edge(v[2], v[3], v[4], v[5], px, py), eca = lm_edge(v[4], v[5], v[0], v[1], px, py);
    if (!(eab > 0 || (eab == 0 && lm_owns(v[2] - v[0], v[3] - v[1])))) return 0;
    if (!(ebc > 0 || (ebc == 0 && lm_owns(v[4] - v[2], v[5] - v[3])))) return 0;
    if (!(eca > 0 || (eca == 0 && lm_owns(v[0] - v[4], v[1] - v[5])))) return 0;
    const int64_t a2 = lm_edge(v[0], v[1], v[2], v[3], v[4], v[5]);
    const float b = (float)((double)eca / (double)a2), g = (float)((double)eab / (double)a2);
    const int mirrored = (t->flags & LM_TRI_MIRRORED) != 0u;
    *beta = mirrored ? g : b; *gamma = mirrored ? b : g;
    return 1;
}

#endif
